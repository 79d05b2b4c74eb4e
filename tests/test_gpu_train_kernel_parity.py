"""Per-kernel parity of the trainer's kernels BETWEEN the GEMMs at fp32-rounding tolerance (pytest -m gpu): BN forward (three regimes), BN backward
(two), the heads with their weight and bias gradients, conv1's forward and weight gradient, Adam.  Third and last group after
test_gpu_layer_parity.py (network forward) and test_gpu_train_layer_parity.py (the trainer's GEMMs).

Every kernel is compared with the float64 reference OF THAT KERNEL evaluated from the device's own tensors of the step (tests/train_kernel_ref.py:
references, statistic, margins), in units of E32 = the same reference code in NumPy float32 on the same inputs.  Every margin is a constant of
train_kernel_ref.MARGIN; tests/test_train_kernel_parity_cpu.py derives them on every run from float32 models that add in each kernel's own order
(healthy ratio and every modelled single defect; the figures are in its docstring).  One case = one trainer; a case of fewer than 64 boards runs
ceil(64 / B) steps on fresh batches with the same weights and takes norm_c of the row tensors over all of them (train_layer_ref, few-row samples);
every element of every step is compared.  f32 at 128 filters unless the case says otherwise, dropout 0.3, clipvalue 0.5, the dense test network
(every parameter kind randomised).  Every case asserts the regime it exists for from the launch plan (Trainer.plan: bn_fwd, bn_bwd, bn_bwd_rs,
conv1_s1), so a threshold that moves fails the test instead of emptying it; test_every_regime_was_seen closes the list.

Exact, not statistical: an element that dropout dropped, or whose float64 BN output lies below -1e-5 x the channel's norm (closer to 0 the sign is
not decided at fp32 precision), is exactly 0.0 in a[l]; a column whose reference is identically zero is exactly 0.0; the device's dgamma / dbeta
follow the device's a (the reference with ONE masked element flipped to live misses the bound that the unflipped one holds); a call below the
capacity leaves a, dz, the BN gradients and the moving statistics bit for bit what a fresh trainer of that capacity computes; the moving statistics
are unchanged before apply.

The clip cases scale the policy head's kernel (train_kernel_ref.CLIP_SCALE, chosen on the CPU) so that 13 .. 418 row-normalised q with a positive
target fall below 1e-7; the reference uses the same rule; no reference q lies within a relative 1e-3 of a threshold (asserted; 0.04 .. 0.27 on the
CPU).  Only the LOWER threshold is reached: the largest q stays 4e-5 below 1, and in fp32 1 - q resolves to 6e-8, so a q near 1 - 1e-7 could not be
placed on a side at all.  These cases judge the heads alone, on one step (the scale was chosen for that batch).
Left out: the streaming BN forward on a DENSE layer needs more than 4096 boards; at 6x6 and 128 filters the trainer's per-board buffers are
73k floats (z, a, dz, two dA, capture) = 1.2 GB at 4097 boards plus 0.3 GB of split-K scratch -- at the 1.5 GB this file allows itself -- and
the float64 references of 147k x 128 rows per conv tensor take well over a few seconds.  The streaming regime runs on conv1 / conv2 (4160 and
9216 rows); the dense layers share its kernels (k_t_colreduce with 64 lanes per row is reached by fc1's BN backward at 257 rows).
One line per (case, kernel, layer) is printed: the worst step's err, E32 and ratio (the table of one run: profiles/train_kernel_parity_ratios.txt)."""
import numpy as np
import pytest

import train_kernel_ref as K
import train_layer_ref as T

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
RATE, SEED, MOM = 0.3, 77, 0.99
TRAINABLE = [i for i in range(40) if i >= 36 or i % 6 not in (4, 5)]


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _trainer(n, C, Bmax, precision="f32", cin=2, policy_loss="rows", weights=None, capture=True, **kw):
    from othellozero_amd.trainer import Trainer
    tr = Trainer(n, C, cin, max_batch=Bmax, lr=1e-3, clipvalue=0.5, dropout=RATE, seed=SEED, precision=precision, policy_loss=policy_loss, **kw)
    tr.set_weights(weights if weights is not None else K.network(n, C, cin))
    if capture:
        tr.set_capture(True)
    return tr


def _interior(tr, n, C, l, B):
    g = T.geometry(n, C, l) if l else dict(zoff=0, Hout=n)
    dz = tr.dz(l, B)
    return dz[:, g["zoff"]:g["zoff"] + g["Hout"], g["zoff"]:g["zoff"] + g["Hout"], :]


def measure_heads(tr, w, n, B, batch, flat, losses, a5):
    own, opp, pit, zt = batch
    p, v = tr.outputs(B)
    dl, dv = tr.head_grads(B)
    args = (a5, w[36], w[37], w[38], w[39], pit, zt, n, flat)
    h64, h32 = K.heads(*args, F64), K.heads(*args, F32)
    recs = [("heads_p", 5, "rows", p, h32["p"], h64["p"]), ("heads_v", 5, "vec", v, h32["v"], h64["v"]),
            ("heads_dlogit", 5, "rows", dl, h32["dlogit"], h64["dlogit"]), ("heads_dvpre", 5, "vec", dv, h32["dvpre"], h64["dvpre"]),
            ("heads_loss", 5, "small", np.array(losses, F32), K.mean_losses(h32["lpi"], h32["lv"], F32), K.mean_losses(h64["lpi"], h64["lv"], F64))]
    r64, r32 = K.heads_reduce(a5, dl, dv, F64), K.heads_reduce(a5, dl, dv, F32)
    recs += [("heads_dwpi", 5, "rows", tr.get_grad(36), r32["dwpi"], r64["dwpi"]), ("heads_dwv", 5, "vec", tr.get_grad(38), r32["dwv"], r64["dwv"]),
             ("heads_dbpi", 5, "vec", tr.get_grad(37), r32["dbpi"], r64["dbpi"]), ("heads_dbv", 5, "colsum_small", tr.get_grad(39), dv.reshape(-1, 1), None)]
    return recs, h64


def measure(tr, w, n, C, B, batch, flat, first):
    """one step -> (records [(key, layer, kind, gpu, ref32, ref64, ...)], plan, (f32, f64) of the BN forwards)"""
    losses = tr.forward_backward(*batch)
    own, opp = batch[:2]
    cin = np.asarray(w[0]).shape[2]
    plan = tr.plan()
    recs, fwd = [], []
    acts = [tr.activation(l, B) for l in range(6)]
    for l in range(6):
        z = tr.preact(l, B)
        mean, rstd = tr.bn_stats(l)
        args = (z, w[6 * l + 2], w[6 * l + 3], w[6 * l + 4], w[6 * l + 5], l, MOM, RATE, SEED, tr.step)
        f64, f32 = K.bn_forward(*args, F64), K.bn_forward(*args, F32)
        fwd.append((f32, f64))
        post = K.post_scale(l, RATE)
        recs += [("bnf_a", l, "a", acts[l], f32, f64, post), ("bnf_mean", l, "vec", mean, f32["mean"], f64["mean"]), ("bnf_rstd", l, "vec", rstd, f32["rstd"], f64["rstd"])]
        dA, dzi = tr.dgrad(l, B), _interior(tr, n, C, l, B)
        b64, b32 = K.bn_backward(dA, acts[l], z, w[6 * l + 2], post, F64), K.bn_backward(dA, acts[l], z, w[6 * l + 2], post, F32)
        dgamma, dbeta = tr.get_grad(6 * l + 2), tr.get_grad(6 * l + 3)
        recs += [("bnb_dz", l, "rows", dzi, b32["dz"], b64["dz"]), ("bnb_dgamma", l, "vec", dgamma, b32["dgamma"], b64["dgamma"]),
                 ("bnb_dbeta", l, "vec", dbeta, b32["dbeta"], b64["dbeta"]), ("bnb_dbias", l, "colsum", tr.get_grad(6 * l + 1), K.rows_of(dzi), None)]
        if first:
            # the device's sums follow the device's a: flip the reference's mask at the masked element with the largest |dA| -- the flipped reference
            # must miss the bound that the unflipped one holds
            live = K.rows_of(acts[l]) > 0
            dAr, zr = K.rows_of(dA).astype(F64), K.rows_of(z).astype(F64)
            xh = (zr - f64["mean"]) * f64["rstd"]
            for got, ref, key, delta in ((dbeta, b64["dbeta"], "bnb_dbeta", dAr * post), (dgamma, b64["dgamma"], "bnb_dgamma", dAr * post * xh)):
                m, c = np.unravel_index(np.argmax(np.where(live, 0.0, np.abs(delta))), delta.shape)
                assert not live[m, c] and delta[m, c] != 0
                bound = K.MARGIN[key] * K.statistic(K.vec(b32[key[4:]]), K.vec(ref))[0] * np.abs(ref).max()
                assert abs(float(got[c]) - ref[c]) <= bound < abs(float(got[c]) - (ref[c] + delta[m, c])), (l, key, m, c, float(got[c]), ref[c], delta[m, c], bound)
    z0_64, z0_32 = K.conv1_forward(own, opp, n, w[0], w[1], F64), K.conv1_forward(own, opp, n, w[0], w[1], F32)
    dz0 = _interior(tr, n, C, 0, B)
    recs += [("conv1_fwd", 0, "rows", tr.preact(0, B), z0_32, z0_64),
             ("conv1_wgrad", 0, "rows", tr.get_grad(0), K.conv1_wgrad(own, opp, n, cin, dz0, F32), K.conv1_wgrad(own, opp, n, cin, dz0, F64))]
    recs += measure_heads(tr, w, n, B, batch, flat, losses, acts[5])[0]
    return recs, plan, fwd


def _judge(r, norm):
    """-> (err, e32, kept) of one record"""
    key, l, kind, gpu, r32, r64 = r[:6]
    if kind == "a":
        err, kept, _ = K.a_statistic(gpu, r64, r[6], norm)
        return err, K.a_statistic(r32["a"], r64, r[6], norm)[0], kept
    if kind == "rows":
        err, kept = K.statistic(gpu, r64, norm)
        return err, K.statistic(r32, r64, norm)[0], kept
    if kind in ("vec", "small"):
        err, kept = K.statistic(K.vec(gpu), K.vec(r64))
        e32 = K.statistic(K.vec(r32), K.vec(r64))[0]
        return err, max(e32, K.E32_FLOOR) if kind == "small" else e32, kept
    rows = r32                                                      # colsum: the float64 and float32 sums of the device's own rows
    err, kept = K.colsum_statistic(gpu, rows)
    e32 = K.colsum_statistic(rows.sum(axis=0, dtype=F32), rows)[0]
    return err, max(e32, K.E32_FLOOR) if kind == "colsum_small" else e32, kept


def evaluate(steps):
    """steps: the record lists of ONE trainer -> rows dict(key, layer, step, err, e32, kept, margin)"""
    rows = []
    for i in range(len(steps[0])):
        key, l, kind = steps[0][i][:3]
        norm = None
        if kind == "rows":
            norm = np.max([T.column_norm(s[i][5]) for s in steps], axis=0)
        elif kind == "a":
            norm = np.max([np.abs(s[i][5]["y"]).max(axis=0) * s[i][6] for s in steps], axis=0)
        for k, s in enumerate(steps):
            err, e32, kept = _judge(s[i], norm)
            rows.append(dict(key=key, layer=l, step=k, err=err, e32=e32, kept=kept, margin=K.MARGIN[key]))
    return rows


def report(name, rows, B, count, plan):
    worst = {}
    for r in rows:
        k = (r["key"], r["layer"])
        if k not in worst or r["err"] / r["e32"] > worst[k]["err"] / worst[k]["e32"]:
            worst[k] = r
    for (key, l), r in worst.items():
        regime = ""
        if key.startswith("bnf"):
            regime = plan[l]["bn_fwd"]
        elif key.startswith("bnb"):
            regime = f"{plan[l]['bn_bwd']} RS {plan[l]['bn_bwd_rs']}"
        elif key == "conv1_wgrad":
            regime = f"S1 {plan[0]['conv1_s1']}"
        print(f"kernel-parity {name:18s} {key:13s} layer {l} B {B:4d} steps {count:2d} {regime:13s} err {r['err']:.3e}  E32 {r['e32']:.3e}  "
              f"ratio {r['err'] / r['e32']:6.2f}  margin {r['margin']:4.1f}  kept {r['kept']:.2f}")


def assert_rows(rows):
    assert all(r["e32"] > 0 for r in rows)
    assert all(r["kept"] >= 0.5 for r in rows), [(r["key"], r["layer"], r["kept"]) for r in rows if r["kept"] < 0.5]
    bad = [(r["key"], r["layer"], r["step"], round(r["err"] / r["e32"], 2), r["margin"]) for r in rows if not r["err"] <= r["margin"] * r["e32"]]
    assert not bad, f"(kernel, layer, step, err / E32, margin) above the margin: {bad}"


def check_moving_statistics(tr, w, fwd, key_mv="bnf_mv"):
    """before apply the moving statistics are unchanged (staged); after it they are the reference's, from the device's z[l] of the last step"""
    before = tr.get_weights()
    for l in range(6):
        assert np.array_equal(before[6 * l + 4], w[6 * l + 4]) and np.array_equal(before[6 * l + 5], w[6 * l + 5]), l
    step = tr.step
    tr.apply()
    assert tr.step == step + 1
    after = tr.get_weights()
    rows = []
    for l in range(6):
        f32, f64 = fwd[l]
        for key, i, t in (("bnf_mm", 4, "mm_new"), (key_mv, 5, "mv_new")):
            err, kept = K.statistic(K.vec(after[6 * l + i]), K.vec(f64[t]))
            rows.append(dict(key=key, layer=l, step=0, err=err, e32=K.statistic(K.vec(f32[t]), K.vec(f64[t]))[0], kept=kept, margin=K.MARGIN[key]))
    return rows


# ------------------------------------------------------------------ the matrix
def _case(name, n, B, expect, C=128, precision="f32", cin=2, policy_loss="rows", Bmax=None, zero_row=None):
    return dict(name=name, n=n, B=B, C=C, precision=precision, cin=cin, policy_loss=policy_loss, Bmax=Bmax or B, expect=expect, zero_row=zero_row)


_F, _S = dict(bn_bwd="fused", bn_bwd_rs=1), lambda rs: dict(bn_bwd="split", bn_bwd_rs=rs)
CASES = [
    # BN backward at exactly 256 rows (conv1 / conv2: the float64 kernel at its limit); conv1's weight gradient at S1 = 16
    _case("8x8-b4", 8, 4, {0: dict(_F, conv1_s1=16, bn_fwd="fused32"), 1: _F, 2: _F, 3: _F, 4: _F, 5: _F}),
    # 320 rows: the first split case of the 8x8 layers (RS 16), conv3 / conv4 still fused
    _case("8x8-b5", 8, 5, {0: _S(16), 1: _S(16), 2: _F, 3: _F}),
    _case("8x8-b17", 8, 17, {3: _S(16), 2: _S(16)}),                                        # conv4 at 272 rows: the first split case of the 4x4 layer
    _case("8x8-b32", 8, 32, {0: dict(_S(32), bn_fwd="fused32"), 1: dict(bn_fwd="fused32")}),     # <32> at its limit: 2048 rows, every register row live
    _case("8x8-b33", 8, 33, {0: dict(_S(64), bn_fwd="fused64"), 1: dict(bn_fwd="fused64"), 2: dict(bn_fwd="fused32")}),   # <64> with a 64-row tail; conv3 at 1188 rows
    _case("8x8-b64", 8, 64, {0: dict(_S(64), bn_fwd="fused64"), 1: dict(bn_fwd="fused64")}),     # <64> at its limit
    _case("8x8-b65", 8, 65, {0: dict(_S(128), bn_fwd="stream"), 1: dict(bn_fwd="stream"), 2: dict(bn_fwd="fused64")}),   # the streaming path at 4160 rows
    # M no multiple of 64 on every layer (252, 252, 112, 28, 7, 7); conv1's kernels <6> with one input plane; heads with A = 36 (idle lanes, 6-lane rows)
    _case("6x6-b7-cin1", 6, 7, {0: dict(_F, conv1_s1=16, bn_fwd="fused32"), 1: _F, 2: _F, 3: _F, 4: _F, 5: _F}, cin=1),
    # dense layers at 256 rows (fused) and 257 (split, about 4 rows per slot); conv4 (2x2) at 1024 / 1028 rows; conv1 / conv2 stream at 9216 rows
    _case("6x6-b256", 6, 256, {4: _F, 5: _F, 3: _S(16), 0: dict(bn_fwd="stream", conv1_s1=256)}),
    _case("6x6-b257", 6, 257, {4: _S(16), 5: _S(16), 3: _S(32), 0: dict(bn_fwd="stream")}),
    # 384 filters: Q = 96 float4 columns, the second block of k_t_colreduce / k_t_bnb_apply is half idle; 512 rows > 256
    _case("8x8-c384-b8", 8, 8, {0: _S(16), 1: _S(16)}, C=384),
    # the same kernels behind the split-precision GEMMs (f16x2 also takes the dzmax branch); the bounds are those of f32
    # (256 filters: a row of 64 float4 lanes, 4 rows per pass -- 2112 rows split 128 ways)
    _case("h2-c256-b33", 8, 33, {0: dict(_S(128), bn_fwd="fused64"), 2: dict(bn_fwd="fused32")}, C=256, precision="f16x2"),
    _case("b3-c256-b33", 8, 33, {0: dict(_S(128), bn_fwd="fused64"), 2: dict(bn_fwd="fused32")}, C=256, precision="bf16x3"),
    # both policy losses x both board sizes, 9 boards: one all-zero target row, one dense Dirichlet row
    _case("rows-6x6-b9", 6, 9, {}, zero_row=3), _case("flat-6x6-b9", 6, 9, {}, policy_loss="flat", zero_row=3),
    _case("rows-8x8-b9", 8, 9, {}, zero_row=3), _case("flat-8x8-b9", 8, 9, {}, policy_loss="flat", zero_row=3),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
_results = {}
_seen = dict(bn_fwd=set(), bn_bwd=set(), rs=set(), conv1=set(), loss=set())


def run_case(case):
    name = case["name"]
    if name not in _results:
        n, B, C, cin = case["n"], case["B"], case["C"], case["cin"]
        flat = case["policy_loss"] == "flat"
        w = K.network(n, C, cin)
        tr = _trainer(n, C, case["Bmax"], case["precision"], cin, case["policy_loss"])
        count = 1 if B >= T.ROWS_FOR_NORM else -(-T.ROWS_FOR_NORM // B)
        steps = [measure(tr, w, n, C, B, K.batch(n, B, 900 + 17 * k, zero_row=case["zero_row"]), flat, k == 0) for k in range(count)]
        plan = steps[0][1]
        assert all(s[1] == plan for s in steps)
        rows = evaluate([s[0] for s in steps]) + check_moving_statistics(tr, w, steps[-1][2])
        report(name, rows, B, count, plan)
        for l in range(6):
            _seen["bn_fwd"].add(plan[l]["bn_fwd"]); _seen["bn_bwd"].add(plan[l]["bn_bwd"]); _seen["rs"].add(plan[l]["bn_bwd_rs"])
        _seen["conv1"].add(n); _seen["loss"].add(case["policy_loss"])
        _results[name] = (rows, plan)
    return _results[name]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_train_kernel_parity(oz, name):
    case = CASE_BY_NAME[name]
    rows, plan = run_case(case)
    for layer, fields in case["expect"].items():
        for k, v in fields.items():
            assert plan[layer][k] == v, (layer, k, plan[layer])
    P = [case["n"] ** 2, case["n"] ** 2, (case["n"] - 2) ** 2, (case["n"] - 4) ** 2, 1, 1]
    for l in range(6):                     # the plan against the launchers' rules, on every layer
        M = case["B"] * P[l]
        assert plan[l]["bn_fwd"] == K.bnf_regime(M), (l, plan[l])
        assert plan[l]["bn_bwd"] == ("fused" if M <= K.BNB_MIN_ROWS else "split"), (l, plan[l])
        if M > K.BNB_MIN_ROWS:
            assert plan[l]["bn_bwd_rs"] == K.bnb_row_splits(M, case["C"] if l < 4 else (1024, 512)[l - 4]), (l, plan[l])
    assert plan[0]["conv1_s1"] == K.conv1_row_splits(case["B"] * P[0])
    assert_rows(rows)


def test_every_regime_was_seen(oz):
    """every regime name the plan can report was reached by some case of the matrix"""
    for case in CASES:
        run_case(case)
    assert _seen["bn_fwd"] == {"fused32", "fused64", "stream"}, _seen
    assert _seen["bn_bwd"] == {"fused", "split"}, _seen
    assert len(_seen["rs"] - {1}) >= 2 and {16, 64, 128} <= _seen["rs"], _seen
    assert _seen["conv1"] == {6, 8} and _seen["loss"] == {"rows", "flat"}, _seen


# ------------------------------------------------------------------ the clip threshold of the policy loss
@pytest.mark.parametrize("n,policy_loss", [(6, "rows"), (6, "flat"), (8, "rows"), (8, "flat")])
def test_heads_clip(oz, n, policy_loss):
    C, B, flat = 128, 9, policy_loss == "flat"
    w = K.clip_weights(K.network(n, C), n, flat)
    tr = _trainer(n, C, B, policy_loss=policy_loss, weights=w)
    batch = K.batch(n, B, 900, dense_rows="all")
    losses = tr.forward_backward(*batch)
    recs, h64 = measure_heads(tr, w, n, B, batch, flat, losses, tr.activation(5, B))
    gap_lo, gap_hi = K.clip_gap(h64["q"])
    below = (h64["q"] < K.CLIP_LO) & (batch[2] > 0)
    print(f"kernel-parity clip-{policy_loss}-{n}x{n}: {int(below.sum())} q with a target below 1e-7, {int((~below & (batch[2] > 0)).sum())} above; gap to the lower "
          f"threshold {gap_lo:.3g}, largest q {gap_hi + 1:.3g} x 1e-7 below 1 (upper threshold not reached)")
    assert gap_lo > 1e-3 and gap_hi > 1e-3                             # no reference q within a relative 1e-3 of either threshold
    assert below.any() and (~below & (batch[2] > 0)).any() and not np.any(h64["q"] > K.CLIP_HI)
    assert np.all(h64["inside"] == ~(h64["q"] < K.CLIP_LO))
    rows = evaluate([recs])
    report(f"clip-{policy_loss}-{n}x{n}", rows, B, 1, tr.plan())
    assert_rows(rows)


# ------------------------------------------------------------------ the kind of the moving variance
def test_moving_variance_kind(oz):
    """from moving statistics that are zero the new moving variance is the batch variance x (1 - momentum): unbiased on the conv layers, biased on the
    dense ones, a relative 1 / (M - 1) apart (under a moving variance of order 1 the kind cannot be told: test_train_kernel_parity_cpu.py).
    8x8 at 65 boards: 4160 (stream), 2340 (fused64), 1040 (fused32) and 65 rows"""
    n, C, B = 8, 128, 65
    w = [np.array(a) for a in K.network(n, C)]
    for l in range(6):
        w[6 * l + 4][:] = 0; w[6 * l + 5][:] = 0
    tr = _trainer(n, C, B, weights=w, capture=False)
    tr.forward_backward(*K.batch(n, B, 900))
    fwd = []
    for l in range(6):
        args = (tr.preact(l, B), w[6 * l + 2], w[6 * l + 3], w[6 * l + 4], w[6 * l + 5], l, MOM, RATE, SEED, 0)
        fwd.append((K.bn_forward(*args, F32), K.bn_forward(*args, F64)))
    plan = tr.plan()
    assert [plan[l]["bn_fwd"] for l in range(6)] == ["stream", "stream", "fused64", "fused32", "fused32", "fused32"]
    rows = check_moving_statistics(tr, w, fwd, key_mv="bnf_mv0")
    report("mv-kind-8x8-b65", rows, B, 1, plan)
    assert_rows(rows)


# ------------------------------------------------------------------ a call below the capacity
def test_short_call_on_a_used_trainer_is_bit_identical(oz):
    """6x6, 37 boards on a trainer of capacity 64 that has just run 64: the rows past the call enter no statistic -- a, dz, the BN gradients and the
    moving statistics are bit for bit those of a fresh trainer of capacity 37"""
    n, C = 6, 128
    w = K.network(n, C)
    used, fresh = _trainer(n, C, 64, capture=False), _trainer(n, C, 37, capture=False)
    used.forward_backward(*K.batch(n, 64, 31))
    batch = K.batch(n, 37, 32)
    out = []
    for tr in (used, fresh):
        tr.forward_backward(*batch)
        got = [tr.activation(l, 37) for l in range(6)] + [tr.dz(l, 37) for l in range(6)] + [tr.get_grad(6 * l + j) for l in range(6) for j in (1, 2, 3)]
        got += [x for l in range(6) for x in tr.bn_stats(l)]
        tr.apply()
        after = tr.get_weights()
        out.append(got + [after[6 * l + j] for l in range(6) for j in (4, 5)])
    assert len(out[0]) == len(out[1]) == 12 + 18 + 12 + 12
    for i, (a, b) in enumerate(zip(*out)):
        assert a.shape == b.shape and np.array_equal(a, b), i
    assert all(np.any(x != 0) for x in out[0][:12])


# ------------------------------------------------------------------ Adam
def test_adam_three_steps(oz):
    """three consecutive optimiser steps, each judged on its own from the device's parameters, gradients and moments before it; the gradients are a
    step's own, rewritten in the (external) arena so that they hold exact zeros, values beyond +-clip and values near 1e-20 and 1e-6"""
    import torch
    from othellozero_amd.trainer import Trainer
    n, C, B = 6, 128, 7
    arena = torch.zeros(Trainer.arena_size(n, C, 2), dtype=torch.float32, device="cuda")
    tr = _trainer(n, C, B, capture=False, external_grads_ptr=arena.data_ptr())
    rows = []
    for step in (1, 2, 3):
        tr.forward_backward(*K.batch(n, B, 50 + step))
        tr.sync()
        arena.copy_(torch.from_numpy(K.adam_gradients(arena.cpu().numpy())))
        torch.cuda.synchronize()
        p, g = tr.get_weights(), tr.get_grads()
        mv = {i: tr.adam_state(i) for i in TRAINABLE}
        flat = np.concatenate([g[i].ravel() for i in TRAINABLE])
        assert np.any(flat == 0) and np.any(np.abs(flat) > 0.5) and np.any(np.abs(flat) == F32(1e-20)) and np.any(np.abs(flat) == F32(1e-6))
        if step == 1:
            assert all(not m.any() and not v.any() for m, v in mv.values())
        tr.apply()
        assert tr.step == step
        after = tr.get_weights()
        lr_t = K.adam_lr_t(1e-3, step)
        for i in TRAINABLE:
            m2, v2 = tr.adam_state(i)
            r64, r32 = K.adam(p[i], g[i], *mv[i], lr_t, 0.5, F64), K.adam(p[i], g[i], *mv[i], lr_t, 0.5, F32)
            for key, got, j in (("adam_p", after[i], 0), ("adam_m", m2, 1), ("adam_v", v2, 2)):
                err, kept = K.statistic(K.vec(got), K.vec(r64[j]))
                e32 = K.statistic(K.vec(r32[j]), K.vec(r64[j]))[0]
                rows.append(dict(key=key, layer=i, step=step, err=err, e32=max(e32, K.E32_FLOOR) if got.size < 16 else e32, kept=kept, margin=K.MARGIN[key]))
    worst = {}
    for r in rows:
        k = (r["key"], r["step"])
        if k not in worst or r["err"] / r["e32"] > worst[k]["err"] / worst[k]["e32"]:
            worst[k] = r
    for (key, step), r in worst.items():
        print(f"kernel-parity adam step {step} {key:7s} worst array {r['layer']:2d} err {r['err']:.3e}  E32 {r['e32']:.3e}  ratio {r['err'] / r['e32']:6.2f}  margin {r['margin']:4.1f}")
    assert_rows(rows)


# ------------------------------------------------------------------ the views
@pytest.mark.parametrize("precision,C", [("f32", 128), ("f16x2", 256), ("bf16x3", 256)])
def test_views_change_no_bit(oz, precision, C):
    """a step's gradients, outputs and updated weights are bit-identical whether or not bn_stats / adam_state / plan are called around it"""
    n, B = 6, 16
    tr = _trainer(n, C, B, precision, capture=False)
    batch = K.batch(n, B, 5)

    def step(views):
        if views:
            tr.plan(); tr.adam_state(6)
        losses = tr.forward_backward(*batch)
        if views:
            for l in range(6):
                tr.bn_stats(l)
            tr.plan(); tr.adam_state(0)
        g = tr.get_grads()
        return [np.array(losses)] + [g[i] for i in sorted(g)] + list(tr.outputs(B))
    off, on, again = step(False), step(True), step(False)
    for a, b, c in zip(off, on, again):
        assert a.shape == b.shape and np.array_equal(a, b) and np.array_equal(a, c)


def test_new_views_refuse_bad_arguments(oz):
    tr = _trainer(6, 128, 4, capture=False)
    lib = oz.load()
    buf, buf2 = np.zeros(1024, F32), np.zeros(1024, F32)
    with pytest.raises(oz.OzError) as e:
        oz.check(lib.oz_trainer_get_bn_stats(tr._h, 0, oz.p_f32(buf), oz.p_f32(buf2)))         # no step has run yet
    assert e.value.code == oz.OZ_ERR_STATE
    tr.forward_backward(*K.batch(6, 4, 1))
    for layer in (-1, 6):
        with pytest.raises(oz.OzError) as e:
            oz.check(lib.oz_trainer_get_bn_stats(tr._h, layer, oz.p_f32(buf), oz.p_f32(buf2)))
        assert e.value.code == oz.OZ_ERR_ARG, layer
    for args in ((tr._h, 0, None, oz.p_f32(buf2)), (tr._h, 0, oz.p_f32(buf), None), (None, 0, oz.p_f32(buf), oz.p_f32(buf2))):
        with pytest.raises(oz.OzError) as e:
            oz.check(lib.oz_trainer_get_bn_stats(*args))
        assert e.value.code == oz.OZ_ERR_ARG
    for index in (-1, 40, 4, 5, 34, 35):                               # outside the arrays; a moving statistic has no moments
        with pytest.raises(oz.OzError) as e:
            oz.check(lib.oz_trainer_get_adam_state(tr._h, index, oz.p_f32(buf), oz.p_f32(buf2)))
        assert e.value.code == oz.OZ_ERR_ARG, index
    with pytest.raises(oz.OzError) as e:
        oz.check(lib.oz_trainer_get_adam_state(tr._h, 1, None, oz.p_f32(buf2)))
    assert e.value.code == oz.OZ_ERR_ARG
    with pytest.raises(oz.OzError) as e:
        oz.check(lib.oz_trainer_get_plan(tr._h, oz.p_i32(np.zeros(5 * oz.TRAINER_PLAN_FIELDS, np.int32)), 5 * oz.TRAINER_PLAN_FIELDS))
    assert e.value.code == oz.OZ_ERR_ARG
    mean, rstd = tr.bn_stats(4)
    assert mean.shape == rstd.shape == (1024,) and np.all(rstd > 0)
    m, v = tr.adam_state(36)
    assert m.shape == v.shape == (512, 36)
