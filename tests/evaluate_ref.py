"""Host side of the held-out evaluation tests (test_gpu_evaluate.py, test_evaluate_host.py): the examples, weights whose BN moving statistics
fit those examples, the float64 oracle's outputs on them and the float64 restatement of the evaluation's metrics.  No GPU.

Examples: random boards; policy targets in visit-count style -- small integer counts, row-normalised, so most rows have SEVERAL equal maxima
(the arg-max rule "lowest index among equal maxima" decides them) -- with every fifth row one-hot; z in {-1, 0, +1} with about a fifth zeros.
A random network hardly ever agrees with a random target, so a third of the rows get the float64 oracle's own move as ONE of their equal
maxima (a hit only where no lower index ties), a third as their only maximum, and half of the one-hot rows are that move.
Weights: init_weights(randomize_all=True) with the moving mean / variance of every BN layer set, layer by layer in float64, to the statistics
of the 70 examples themselves ("statistics set from the batch"): inference-mode activations then have unit scale in every layer, so the range
guard of the trainer's f16x2 mode is not what a parity test exercises.
"""
import functools

import numpy as np

N_EXAMPLES = 70            # two full batches of 32 and a short one of 6
SEED = 5                   # (test_evaluate_host.py checks that the oracle alone has no near-tie on these examples)


@functools.lru_cache(maxsize=None)
def boards(n, N=N_EXAMPLES, seed=SEED):
    rs = np.random.RandomState(seed + 100 * n)
    valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
    own = rs.randint(0, 2**63, size=N, dtype=np.uint64) & valid
    opp = rs.randint(0, 2**63, size=N, dtype=np.uint64) & valid & ~own
    own.setflags(write=False); opp.setflags(write=False)
    return own, opp


@functools.lru_cache(maxsize=None)
def calibrated_weights(n, C, seed=SEED):
    """the 40 float32 arrays; moving statistics = the float64 statistics of boards(n) under these very weights"""
    from oracle import nn_numpy as O
    from othellozero_amd.weights import init_weights
    own, opp = boards(n)
    w = [a.astype(np.float64) for a in init_weights(n, seed=seed, channels=C, randomize_all=True)]
    x = O.planes(own, opp, n)
    for l, same in enumerate((True, True, False, False)):
        zz = O._conv3x3(x, w[6 * l], w[6 * l + 1], same)
        w[6 * l + 4], w[6 * l + 5] = zz.mean(axis=(0, 1, 2)), zz.var(axis=(0, 1, 2))
        x = np.maximum(O._bn(zz, *w[6 * l + 2:6 * l + 6]), 0)
    x = x.reshape(x.shape[0], -1)
    for l in (4, 5):
        zz = x @ w[6 * l] + w[6 * l + 1]
        w[6 * l + 4], w[6 * l + 5] = zz.mean(axis=0), zz.var(axis=0)
        x = np.maximum(O._bn(zz, *w[6 * l + 2:6 * l + 6]), 0)
    out = [a.astype(np.float32) for a in w]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_outputs(n, C):
    """(p (N, A), v (N,)) of the float64 inference network on boards(n) with calibrated_weights(n, C)"""
    from oracle import nn_numpy as O
    own, opp = boards(n)
    p, v = O.forward(calibrated_weights(n, C), own, opp, n, dtype=np.float64)
    return p, v


@functools.lru_cache(maxsize=None)
def examples(n, C, seed=SEED):
    """(own, opp, pi, z) of the N_EXAMPLES examples for the network calibrated_weights(n, C): see the module docstring"""
    rs = np.random.RandomState(seed + 100 * n + 1)
    own, opp = boards(n)
    N, A = own.size, n * n
    best = np.argmax(oracle_outputs(n, C)[0], axis=1)
    counts = rs.randint(0, 4, size=(N, A)).astype(np.float64)
    counts[:, 0] += (counts.sum(axis=1) == 0)                       # (no empty row)
    i = np.arange(N)
    hot = i % 5 == 4
    counts[hot] = 0
    counts[hot, np.where(i[hot] % 2 == 0, best[hot], rs.randint(0, A, int(hot.sum())))] = 1
    tie, top = (i % 3 == 0) & ~hot, (i % 3 == 1) & ~hot
    counts[tie, best[tie]] = counts[tie].max(axis=1)                # the network's move is ONE of the equal maxima: the lowest index decides
    counts[top, best[top]] = counts[top].max(axis=1) + 1            # the network's move is the only maximum
    pi = (counts / counts.sum(axis=1, keepdims=True)).astype(np.float32)
    z = rs.choice([-1.0, 0.0, 1.0], N, p=[0.4, 0.2, 0.4]).astype(np.float32)
    pi.setflags(write=False); z.setflags(write=False)               # shared among the tests: left unchanged
    return own, opp, pi, z


def metrics(p, v, pi, z, n, policy_loss):
    """float64 restatement of the evaluation on given outputs: dict of the per-example arrays pi_loss, v_loss (float64) and top1, sign,
    decided (bool).  The policy loss is the trainer's clipped cross entropy: "rows" on the (n, n) view with every board row renormalised
    and the rows averaged, "flat" on the renormalised whole row; clip [1e-7, 1 - 1e-7].  Both arg-maxes take the lowest index."""
    p = np.asarray(p, np.float64); v = np.asarray(v, np.float64)
    t = np.asarray(pi, np.float64); z = np.asarray(z, np.float64)
    N = p.shape[0]
    if policy_loss == "rows":
        q = p.reshape(N, n, n)
        q = np.clip(q / q.sum(axis=2, keepdims=True), 1e-7, 1 - 1e-7)
        lp = -(t.reshape(N, n, n) * np.log(q)).sum(axis=2).mean(axis=1)
    else:
        q = np.clip(p / p.sum(axis=1, keepdims=True), 1e-7, 1 - 1e-7)
        lp = -(t * np.log(q)).sum(axis=1)
    return dict(pi_loss=lp, v_loss=(v - z) ** 2, top1=np.argmax(p, axis=1) == np.argmax(t, axis=1), sign=v * z > 0, decided=z != 0)


def summary(m):
    """the evaluation's dict from metrics()"""
    N, D = len(m["top1"]), int(m["decided"].sum())
    lp, lv = float(m["pi_loss"].mean()), float(m["v_loss"].mean())
    return {"loss": lp + lv, "pi-reshaped_loss": lp, "v_loss": lv, "policy_top1": float(m["top1"].sum()) / N,
            "value_sign": float((m["sign"] & m["decided"]).sum()) / D if D else 0.0, "examples": N, "decided": D}


def top2_gap(p):
    s = np.sort(np.asarray(p, np.float64), axis=1)
    return s[:, -1] - s[:, -2]
