"""Auxiliary heads without a GPU: the target's one definition on the host (oz_aux_targets) against the NumPy restatement, the symmetry of a pair,
the arena size, the refusals, and the float32 summation-order models of the aux kernels that the per-kernel margins of
tests/test_gpu_aux_heads.py rest on (tests/aux_heads_ref.py, MARGIN).

Margins, by train_kernel_ref's rule (a few times the modelled healthy ratio, at least twice it; at least four times below the weakest modelled
defect).  What the models print -- 6x6 and 8x8 at 9 boards, 8x8 at 33, weights (1.0, 0.25), 128 filters, ratios err / E32:
  k_t_aux_heads, the kernel's own order (fmaf chain in k; the score head's 64 lanes and the shuffle tree) against the float32 evaluation:
      o 1.00 .. 1.32, s 1.00 .. 1.57; the pre-activation gradients from that forward: dopre 1.00 .. 1.25, dspre 1.00           -> MARGIN 8 (the heads')
      defects of the forward, o / s: the bias not added >= 1.3e5 / 1.7e5, the last 64 k lost >= 1.5e6 / 3.1e6, tanh missing >= 2.8e6 / 7.9e6
      defects, dopre: a dead sample trained >= 8.6e5, 1 / A missing >= 4.2e7, the factor 2 >= 4.5e5, tanh' >= 4.5e6, the pair swapped >= 3.4e6;
      dspre: a dead sample >= 1.7e6, the factor 2 >= 1.1e6, tanh' >= 4.4e6, the pair swapped >= 1.9e6
      the two batch means in batch order (k_t_aux_losses; floor 2^-24) 0.51 .. 2.95; the mean over the live samples instead of B >= 6.3e6  -> MARGIN 8
  weight and bias gradients in batch order: dWown 1.00 .. 1.12, dWsc 1.00, dbown 1.00, dbsc 0.51 .. 0.63; a lost board >= 9.2e5 -> MARGIN 6 (the heads')
  k_t_heads_dgrad, add set: df2 + (dspre Wsc, then fmaf over a ascending) 1.00 .. 2.22; the score term missing >= 3.0e6, the last square >= 1.3e5 -> MARGIN 8
Every tensor separates at the heads' margins: none is changed."""
import numpy as np
import pytest

import aux_heads_ref as R
import train_kernel_ref as K

C = 128
F64, F32 = np.float64, np.float32
W_OWN, W_SC = 1.0, 0.25


# ------------------------------------------------------------------ the target on the host
def _oracle_records(n):
    """records of a few of the CPU oracle's games (tests/resign_ref.py: oracle.Mcts on the stub evaluator), a playout cap and a resignation rule on
    so that some carry the flags by themselves; then one record of each kind flagged by hand"""
    from resign_ref import episodes
    rec = np.concatenate([episodes(n, 4, None, 0.9, 31, range(3), salt=3, cap=(2, 0.5))[0],            # some fast records
                          episodes(n, 4, (0.05, 2, 4, 0.0), 0.9, 31, [3], salt=3)[0]])                 # one game that may be adjudicated
    plain = np.flatnonzero((rec["pad"][:, 0] == 0) & (rec["pad"][:, 1] == 0))
    assert plain.size >= 3, "the games must leave unflagged records"
    rec["pad"][plain[0], 0] = 1                      # a fast record by hand
    rec["pad"][plain[1], 1] = 1                      # a record of an adjudicated game by hand
    return rec, plain[2:]


@pytest.mark.parametrize("n", [6, 8])
def test_aux_targets_match_the_restatement(n):
    from othellozero_amd import _lib
    from othellozero_amd.agents import rules_aux_targets
    rec, plain = _oracle_records(n)
    rec = np.ascontiguousarray(rec.astype(_lib.RECORD_DTYPE))
    fo, fp = rules_aux_targets(rec)
    wo, wp = R.aux_target(rec)
    assert fo.dtype == np.uint64 and np.array_equal(fo, wo) and np.array_equal(fp, wp)
    flagged = (rec["pad"][:, 0] == 1) | (rec["pad"][:, 1] == 1)
    assert flagged.sum() >= 2 and np.all(fo[flagged] == 0) and np.all(fp[flagged] == 0)
    assert (rec["pad"][:, 0] == 1).any() and (rec["pad"][:, 1] == 1).any()
    assert np.all((fo[~flagged] | fp[~flagged]) != 0), "a real final board is never empty: the zero pair is the mask"
    assert np.all((fo & fp) == 0)
    black = rec["player"][plain] == 1
    assert black.any() and (~black).any()                          # both movers: the swap is exercised
    assert np.array_equal(fo[plain], np.where(black, rec["final_black"][plain], rec["final_white"][plain]))
    # targets of one record, spelled out
    i = int(plain[0])
    t = R.own_targets(fo[i:i + 1], fp[i:i + 1], n)[0]
    for a in range(n * n):
        sq = (a // n) * 8 + a % n
        assert t[a] == ((int(fo[i]) >> sq) & 1) - ((int(fp[i]) >> sq) & 1)
    assert R.score_targets(fo[i:i + 1], fp[i:i + 1], n)[0] == (bin(int(fo[i])).count("1") - bin(int(fp[i])).count("1")) / (n * n)


@pytest.mark.parametrize("n", [6, 8])
def test_all_eight_symmetries_of_a_pair(n):
    from othellozero_amd.agents import rules_sym_boards
    fo, fp = R.final_pairs(n, 12, 5)
    for t in range(8):
        go, gp = rules_sym_boards(fo, n, t), rules_sym_boards(fp, n, t)
        for b in range(fo.size):
            assert (int(go[b]), int(gp[b])) == R.sym_pair(t, n, fo[b], fp[b]), (t, b)
        # a symmetry moves discs, it neither makes nor loses any: mask and score target are invariant
        assert np.array_equal(R.masks(go, gp), R.masks(fo, fp))
        assert np.array_equal(R.score_targets(go, gp, n), R.score_targets(fo, fp, n))
    assert np.array_equal(rules_sym_boards(fo, n, 7), fo)             # the identity is symmetry 7


@pytest.mark.parametrize("n,C_,cin", [(6, 128, 2), (8, 512, 2), (8, 256, 1)])
def test_arena_size_with_the_heads(n, C_, cin):
    from othellozero_amd.trainer import Trainer
    A = n * n
    assert Trainer.arena_size(n, C_, cin, aux=True) - Trainer.arena_size(n, C_, cin) == 512 * A + A + 512 + 1
    assert Trainer.arena_size(n, C_, cin, aux=False) == Trainer.arena_size(n, C_, cin)


# ------------------------------------------------------------------ refusals, before a GPU is touched
class _Net:
    in_channels = 2
    policy_loss = "rows"


def _training(**kw):
    from othellozero_amd import loop
    net = _Net()
    net.in_channels = kw.pop("in_channels", 2)
    return loop.training(6, 1, 2, 2, 1.0, 1.0, net, 0.9, 1, 1, 0, False, 1, 2, 1, "unused.h5", 64, **kw)


def test_refusals_raise_before_a_gpu_is_touched():
    from othellozero_amd import _lib
    from othellozero_amd.trainer import Trainer
    on = dict(ownership=1.0, score=0.25)
    with pytest.raises(ValueError, match="replay='device'"):
        _training(aux_heads=on, replay="host", alias_final_boards=False)
    with pytest.raises(ValueError, match="distributed"):
        _training(aux_heads=on, replay="host", distributed=True, alias_final_boards=False)
    with pytest.raises(ValueError, match="alias_final_boards=False"):
        _training(aux_heads=on, replay="device", alias_final_boards=True)
    # a one-plane network's examples are the positions at the move whatever alias_final_boards says: not refused by the rule
    assert _lib.check_aux_heads_loop(on, "device", False, True, in_channels=1) == on
    assert _lib.check_aux_heads_loop(on, "device", False, False, in_channels=2) == on
    assert _lib.check_aux_heads_loop(None, "host", True, True) is None
    for bad in (dict(ownership=-1.0), dict(score=float("nan")), dict(ownership=float("inf")), dict(owner=1.0), (1.0, 0.25), dict(ownership="1")):
        with pytest.raises(ValueError):
            _lib.check_aux_heads(bad)
        with pytest.raises(ValueError):
            Trainer(6, 128, 2, max_batch=4, aux_heads=bad)               # (the check precedes the library)
    # an external gradient arena (the data-parallel fit's) is sized for the forty arrays: refused before the library is touched
    with pytest.raises(ValueError, match="external_grads_ptr"):
        Trainer(6, 128, 2, max_batch=4, external_grads_ptr=0x1000, aux_heads=on)
    # a network that cannot train the heads gets the clear message, not an AttributeError
    with pytest.raises(ValueError, match="aux_heads needs a network"):
        _training(aux_heads=on, replay="device", alias_final_boards=False)
    assert _lib.check_aux_heads(dict(ownership=2)) == (2.0, 0.0) and _lib.check_aux_heads(False) is None


# ------------------------------------------------------------------ the models of the aux kernels
def _ratio(got, ref, e32, as_vec=False):
    f = K.vec if as_vec else (lambda x: x)
    return K.statistic(f(got), f(ref))[0] / max(K.statistic(f(e32), f(ref))[0], 1e-300)


def _check(name, key, healthy, defects):
    m = R.MARGIN[key]
    weakest = min(defects.values()) if defects else float("inf")
    print(f"model {name:18s} {key:10s} healthy {healthy:6.2f}  margin {m:4.1f}  defects " + "  ".join(f"{k} {v:.3g}" for k, v in defects.items()))
    assert 2 * healthy <= m, (name, key, healthy)
    assert weakest >= 4 * m, (name, key, defects)


_inputs = {}


def _aux_inputs(n, B):
    """a[5] of the oracle's step (post-dropout, as the heads read it), the heads' gradient wrt it, random heads and final pairs"""
    if (n, B) not in _inputs:
        w = K.network(n, C)
        own, opp, pit, zt = K.batch(n, B, 900)
        s = K.oracle_step(n, C, B)
        a5 = K.bn_forward(s["z"][5], w[32], w[33], w[34], w[35], 5, 0.99, 0.3, 77, 0, F64)["a"].astype(F32)
        h = K.heads(a5, w[36], w[37], w[38], w[39], pit, zt, n, 0, F32)
        df2 = (h["dlogit"] @ np.asarray(w[36], F32).T + np.outer(h["dvpre"], np.asarray(w[38], F32).reshape(-1))).astype(F32)
        _inputs[n, B] = (a5, df2, R.glorot_aux(n, 40 + n), R.final_pairs(n, B, 7 + B))
    return _inputs[n, B]


@pytest.mark.parametrize("n,B", [(6, 9), (8, 9), (8, 33)])
def test_aux_kernel_margins(n, B):
    a5, df2, (wown, bown, wsc, bsc), (fo, fp) = _aux_inputs(n, B)
    assert (R.masks(fo, fp) == 0).any() and (R.masks(fo, fp) == 1).any()
    name = f"aux n={n} B={B}"
    args = (a5, wown, bown, wsc, bsc, fo, fp, n, W_OWN, W_SC)
    r64, r32 = R.aux_heads(*args, F64), R.aux_heads(*args, F32)
    # forward: the kernel's own order against the float32 evaluation
    mo, ms = R.model_aux_forward(a5, wown, bown, wsc, bsc)
    fwd_bad = {d: R.model_aux_forward(a5, wown, bown, wsc, bsc, defect=d) for d in ("no_bias", "lost_k", "no_tanh")}
    _check(name, "aux_o", max(1.0, _ratio(mo, r64["o"], r32["o"])), {d: _ratio(v[0], r64["o"], r32["o"]) for d, v in fwd_bad.items()})
    _check(name, "aux_s", max(1.0, _ratio(ms, r64["s"], r32["s"], True)), {d: _ratio(v[1], r64["s"], r32["s"], True) for d, v in fwd_bad.items()})
    # the pre-activation gradients and per-sample losses from the kernel's own forward; every single defect is far away
    rev = R.aux_heads(*args, F32, forward=(mo, ms))
    bad = {d: R.aux_heads(*args, F32, defect=d) for d in ("mask", "normA", "two", "tanh", "swap")}
    _check(name, "aux_dopre", max(1.0, _ratio(rev["dopre"], r64["dopre"], r32["dopre"])),
           {d: _ratio(bad[d]["dopre"], r64["dopre"], r32["dopre"]) for d in ("mask", "normA", "two", "tanh", "swap")})
    _check(name, "aux_dspre", max(1.0, _ratio(rev["dspre"], r64["dspre"], r32["dspre"], True)),
           {d: _ratio(bad[d]["dspre"], r64["dspre"], r32["dspre"], True) for d in ("mask", "two", "tanh", "swap")})
    # the two batch means, in batch order (k_t_aux_losses); the mean over the live samples is the defect the issue names
    l64, l32 = R.aux_mean_losses(r64["lo"], r64["ls"], F64), R.aux_mean_losses(r32["lo"], r32["ls"], F32)
    e32 = max(K.statistic(K.vec(l32), K.vec(l64))[0], K.E32_FLOOR)
    seq = np.array([np.add.accumulate(rev["lo"].astype(F32))[-1] / F32(B), np.add.accumulate(rev["ls"].astype(F32))[-1] / F32(B)], F32)
    live = seq * F32(B) / F32(R.masks(fo, fp).sum())
    _check(name, "aux_loss", K.statistic(K.vec(seq), K.vec(l64))[0] / e32, {"live_mean": K.statistic(K.vec(live), K.vec(l64))[0] / e32})
    # weight and bias gradients from the heads' own pre-activation gradients, batch order
    red64, red32 = R.aux_reduce(a5, r32["dopre"], r32["dspre"], F64), R.aux_reduce(a5, r32["dopre"], r32["dspre"], F32)
    mod, lost = R.model_aux_reduce(a5, r32["dopre"], r32["dspre"]), R.model_aux_reduce(a5, r32["dopre"], r32["dspre"], lost_board=True)
    assert R.masks(fo, fp)[-1] == 1, "the board that the defect loses must be a live one"
    for t in ("dwown", "dwsc", "dbown"):
        as_vec = t != "dwown"
        _check(name, "aux_" + t, _ratio(mod[t], red64[t], red32[t], as_vec), {"lost_board": _ratio(lost[t], red64[t], red32[t], as_vec)})
    dv = r32["dspre"].reshape(-1, 1)
    e32 = max(K.colsum_statistic(dv.sum(dtype=F32), dv)[0], K.E32_FLOOR)
    _check(name, "aux_dbsc", K.colsum_statistic(mod["dbsc"], dv)[0] / e32, {"lost_board": K.colsum_statistic(lost["dbsc"], dv)[0] / e32})
    # the data gradient: df2 as the policy and value heads left it, plus the aux term
    term64 = R.aux_dgrad(r32["dopre"], r32["dspre"], wown, wsc, F64)
    ref = df2.astype(F64) + term64
    e = (df2 + R.aux_dgrad(r32["dopre"], r32["dspre"], wown, wsc, F32)).astype(F32)
    got = {d: R.model_aux_dgrad(r32["dopre"], r32["dspre"], wown, wsc, df2, defect=d) for d in (None, "no_score", "lost_a")}
    _check(name, "aux_df2", max(1.0, _ratio(got[None], ref, e)), {d: _ratio(got[d], ref, e) for d in ("no_score", "lost_a")})


def test_restatement_without_pairs_is_the_oracle():
    """AuxTrainRef with every mask 0 gives the oracle's own losses and forty gradients (the restated forward IS the oracle's), zero aux gradients"""
    from oracle.train_ref import TrainRef
    n, B = 6, 4
    w = K.network(n, C)
    batch = K.batch(n, B, 11)
    ref = TrainRef(w, n, dropout=0.3, seed=77)
    aux = R.AuxTrainRef(list(w) + R.glorot_aux(n, 3), n, 1.0, 0.25, dropout=0.3, seed=77)
    l0 = ref.forward_backward(*batch)
    l1 = aux.forward_backward(*batch)
    assert l1[:3] == l0 and l1[3:] == (0.0, 0.0)
    for i, g in ref.grads.items():
        assert np.array_equal(g.numpy(), aux.grads[i].numpy()), i
    assert all(float(aux.grads[i].abs().max()) == 0.0 for i in R.AUX)
    # with pairs the aux gradients live, the total is the weighted sum
    fo, fp = R.final_pairs(n, B, 2)
    l2 = aux.forward_backward(*batch, fin_own=fo, fin_opp=fp)
    assert l2[3] > 0 and l2[4] > 0 and abs(l2[0] - (l2[1] + l2[2] + 1.0 * l2[3] + 0.25 * l2[4])) < 1e-12
    assert all(float(aux.grads[i].abs().max()) > 0.0 for i in R.AUX)
