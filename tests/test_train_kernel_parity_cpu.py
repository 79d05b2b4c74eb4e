"""The margins of tests/test_gpu_train_kernel_parity.py can detect a defect: shown on the CPU with float32 NumPy models that add in each kernel's own
order (tests/train_kernel_ref.py: model_*), on the real tensors of a float64 oracle step (oracle/train_ref.py, the dense network at 128 filters,
dropout 0.3) -- never by breaking a kernel on the GPU, and never from what a kernel returns.

Evaluated on every run, relative to E32 (the float64 reference's own code in NumPy float32 on the same inputs): the healthy model, and the model
with each single defect.  The rule (layer_ref): a margin is at least twice the modelled healthy ratio and at least four times below the weakest
modelled defect; what cannot separate by that is named and carries the coarse bound MARGIN_DENSE = 16.

What the models printed when the constants of train_kernel_ref.MARGIN were written (one line per shape and tensor is printed again on every run,
pytest -s; healthy = model / E32 over all shapes of the group, defect = the smallest ratio over those shapes):
  BN forward, 10 shapes of 7 .. 4160 rows (6x6 at 7 boards: 252 / 112 / 28 / 7 rows; 8x8 at 5, 33, 65 boards), by regime
      fused32   a 0.38 .. 1.29  mean 0.45 .. 1.27  rstd 0.35 .. 1.00  moving mean 0.85 .. 1.00  moving variance 1.00
                unbiased variance in rstd >= 622 (a), 756 (rstd); last partial pass of 64 rows lost >= 3.2e4 (213 on the moving variance);
                statistics over 9 / 8 of the rows >= 1.9e4 (391 on the moving variance); 1 / (1 - rate) missing >= 1.1e6
      fused64   a 0.22  mean 0.14  rstd 0.24 (2112 rows); unbiased rstd >= 180; capacity rows >= 1.4e4 (228 on the moving variance)
      stream    a 0.32  mean 0.24  rstd 0.21 (4160 rows); unbiased rstd >= 72; capacity rows >= 1.5e4 (234 on the moving variance)
      -> MARGIN 4 for all five tensors (>= 2 x 1.29, <= 72 / 4)
      the KIND of the moving variance moves mv_new by var (1 - momentum) / (M - 1): 3.7 x E32 at 252 rows under a moving variance of order 1 -- it
      cannot separate there.  From ZERO moving statistics (bnf_mv0; the GPU test runs such a step): healthy 0.20 .. 1.00, wrong kind >= 108 (4160 rows)
      .. 2.5e5 (28 rows) -> MARGIN 4
  BN backward, 11 shapes
      fused (float64, 7 .. 256 rows)  dz 0.48 .. 0.79  dgamma 0.18 .. 0.78  dbeta 0.05 .. 1.00  dbias 0.15 .. 0.81
      split (fp32, 257 .. 4160 rows)  dz 0.30 .. 0.66  dgamma 0.14 .. 0.58  dbeta 0.14 .. 0.57  dbias 0.16 .. 0.44
      S0 / M missing >= 2.5e3, xhat S1 / M missing >= 1.0e4, post_scale missing >= 2.8e5, one row split's partial lost >= 926 (dz at RS 128) .. 3.1e4,
      dbias = dbeta instead of the column sum of dz >= 6.7e4        -> MARGIN 4 for all four tensors
      the 256-row boundary (the same 256 rows of conv1, 8x8 at 4 boards, through both paths, then the split path where it starts):
          256 rows fused (float64)  dz 0.48  dgamma 0.18  dbeta 0.05  dbias 0.20
          256 rows split (fp32)     dz 0.66  dgamma 0.45  dbeta 0.16  dbias 0.73
          320 rows split 0.66 / 0.55 / 0.28 / 0.44    272 rows (4x4) 0.54 / 0.36 / 0.57 / 0.38    257 rows (fc2) 0.64 / 0.58 / 0.48 / 0.38
      the fp32 path loses 0.2 .. 0.5 x E32 against the float64 path and stays below NumPy float32 itself: it holds the bound the float64 path
      holds, OZ_BNB_MIN_ROWS stays where it is
  heads, 6x6 and 8x8 at 9 boards, 8x8 at 64, both losses, and the four clip cases (healthy: the float32 evaluation in reversed k order)
      p 1.00 .. 1.81  v 2.07 .. 2.74  dlogit 1.00 .. 2.58  dvpre 1.56 .. 2.00  batch-mean losses 0.17 .. 3.60           -> MARGIN 8
      1 / B for 1 / (B n) >= 2.7e4; gradient kept outside the clip >= 3.8e5 (clip cases); factor 2 missing >= 1.9e6; 1 - v^2 missing >= 6.3e6;
      the mean over the board rows missing from the loss >= 7.5e6
      weight / bias gradients in batch order: dWpi 1.00 .. 1.49  dWv 1.00 .. 1.82  dbpi 1.00 -> MARGIN 6; dbv 0.03 .. 0.77 -> MARGIN 4; a lost board >= 1.8e4
  conv1: forward 1.00 (at most 18 products of 0 / +-1 inputs), a lost tap >= 1.4e6; weight gradient over S1 = 16 / 256 row splits 0.56 .. 0.83, a lost
      split >= 6.0e4                                                                                                      -> MARGIN 4
  Adam (elementwise: the kernel is the float32 evaluation, 1.00): clip after the moments >= 2.3e5 (p), 5e7 (m), 3e10 (v); eps inside the root >= 2.5e5;
      a bias correction missing >= 1.9e5                                                                                 -> MARGIN 4
Every tensor of every shape separates: no shape of this group needs the coarse bound.
"""
import numpy as np
import pytest

import train_kernel_ref as K

C = 128
F64, F32 = np.float64, np.float32


def _ratio(got, ref, e32, as_vec=False):
    f = K.vec if as_vec else (lambda x: x)
    return K.statistic(f(got), f(ref))[0] / max(K.statistic(f(e32), f(ref))[0], 1e-300)


def _check(name, key, healthy, defects):
    m = K.MARGIN[key]
    weakest = min(defects.values()) if defects else float("inf")
    print(f"model {name:34s} {key:12s} healthy {healthy:6.2f}  margin {m:4.1f}  defects " + "  ".join(f"{k} {v:.3g}" for k, v in defects.items()))
    assert 2 * healthy <= m, (name, key, healthy)
    if m < K.MARGIN_COARSE:
        assert weakest >= 4 * m, (name, key, defects)


# ------------------------------------------------------------------ BN forward
# (board, boards, layer): every regime and the tails -- fused32 with rows that are no multiple of 64, fused64 with a tail, the stream; a dense layer
BNF_SHAPES = [(6, 7, 0), (6, 7, 2), (6, 7, 3), (6, 7, 4), (8, 5, 1), (8, 33, 0), (8, 33, 2), (8, 33, 5), (8, 65, 0), (8, 65, 4)]


@pytest.mark.parametrize("n,B,layer", BNF_SHAPES)
def test_bn_forward_margins(n, B, layer):
    s = K.oracle_step(n, C, B)
    w, z = s["w"], K.rows_of(s["z"][layer])
    M = z.shape[0]
    args = (z, w[6 * layer + 2], w[6 * layer + 3], w[6 * layer + 4], w[6 * layer + 5], layer, 0.99, 0.3, 77, 0)
    r64, r32 = K.bn_forward(*args, F64), K.bn_forward(*args, F32)
    models = {None: K.model_bn_forward(*args)}
    for d in ("unbiased_rstd", "mv_kind") + (("tail",) if M % 64 else ()) + (("scale",) if layer >= 4 else ()):
        models[d] = K.model_bn_forward(*args, defect=d)
    # statistics over the capacity's rows instead of the call's: the reference's own code with the rows past M read as zeros
    cap = K.bn_forward(*args, F32, stat_rows=M + max(M // 8, 1))
    name = f"bnf n={n} B={B} l={layer} rows={M} {K.bnf_regime(M)}"
    post = K.post_scale(layer, 0.3)
    for key, t, v in (("bnf_a", "a", False), ("bnf_mean", "mean", True), ("bnf_rstd", "rstd", True), ("bnf_mm", "mm_new", True), ("bnf_mv", "mv_new", True)):
        if t == "a":                           # under the norm of the BN output before the ReLU; the exact zeros are asserted on the healthy model only
            e32 = K.a_statistic(r32["a"], r64, post)[0]
            stat = lambda x, exact: (K.a_statistic(x, r64, post)[0] if exact else float((np.abs(x - r64["a"]) / K.a_statistic(r32["a"], r64, post)[2]).max())) / e32
            ratio = {d: stat(m[t], d is None) for d, m in models.items()}
            ratio["cap_rows"] = stat(cap[t], False)
        else:
            ratio = {d: _ratio(m[t], r64[t], r32[t], v) for d, m in models.items()}
            ratio["cap_rows"] = _ratio(cap[t], r64[t], r32[t], v)
        healthy = ratio.pop(None)
        # the defects a tensor can see: the rstd defects do not touch the mean, the moving-variance kind only mv_new, the dropout scale only a
        sees = {"bnf_a": ("unbiased_rstd", "tail", "scale", "cap_rows"), "bnf_mean": ("tail", "cap_rows"), "bnf_rstd": ("unbiased_rstd", "tail", "cap_rows"),
                "bnf_mm": ("tail", "cap_rows"), "bnf_mv": ("tail", "cap_rows")}[key]
        _check(name, key, healthy, {d: r for d, r in ratio.items() if d in sees})
    # the KIND of the moving variance (unbiased on conv layers, biased on dense ones) moves mv_new by var (1 - momentum) / (M - 1): under a moving
    # variance of order 1 that is a few E32 at 252 rows and nothing at 4160 -- it cannot separate.  From moving statistics that are ZERO the new
    # value is the batch statistic times (1 - momentum), and the kind is a relative 1 / (M - 1) of it: the GPU test runs a step from such a network too
    zero = np.zeros(z.shape[1], F32)
    a0 = args[:3] + (zero, zero) + args[5:]
    r64, r32, m0, bad = K.bn_forward(*a0, F64), K.bn_forward(*a0, F32), K.model_bn_forward(*a0), K.model_bn_forward(*a0, defect="mv_kind")
    if M > 1:
        _check(name, "bnf_mv0", _ratio(m0["mv_new"], r64["mv_new"], r32["mv_new"], True), {"mv_kind": _ratio(bad["mv_new"], r64["mv_new"], r32["mv_new"], True)})


# ------------------------------------------------------------------ BN backward
# (board, boards, layer): the fused path at its limit (256 rows), the split path just above it (257 .. 320 rows: the worst-conditioned), larger splits, dense layers
BNB_SHAPES = [(8, 4, 0), (8, 5, 0), (8, 5, 3), (8, 17, 3), (8, 33, 1), (8, 65, 0), (6, 7, 0), (6, 7, 4), (6, 257, 4), (6, 257, 5), (6, 256, 5)]


def _bnb_ratios(n, B, layer, path=None, defects=()):
    s = K.oracle_step(n, C, B)
    dA, a, z, g, post = K.oracle_layer(s, layer)
    r64, r32 = K.bn_backward(dA, a, z, g, post, F64), K.bn_backward(dA, a, z, g, post, F32)
    out = {}
    for d in (None,) + tuple(defects):
        m = K.model_bn_backward(dA, a, z, g, post, path=path, defect=d)
        out[d] = dict(dz=_ratio(m["dz"], r64["dz"], r32["dz"]), dgamma=_ratio(m["dgamma"], r64["dgamma"], r32["dgamma"], True),
                      dbeta=_ratio(m["dbeta"], r64["dbeta"], r32["dbeta"], True),
                      dbias=K.colsum_statistic(m["dbias"], m["dz"])[0] / max(K.colsum_statistic(m["dz"].sum(axis=0, dtype=F32), m["dz"])[0], 1e-300))
    return out, z.shape[0]


@pytest.mark.parametrize("n,B,layer", BNB_SHAPES)
def test_bn_backward_margins(n, B, layer):
    M = B * [n * n, n * n, (n - 2) ** 2, (n - 4) ** 2, 1, 1][layer]
    split = M > K.BNB_MIN_ROWS
    defects = ("s0", "s1", "dbias") + (("post",) if layer >= 4 else ()) + (("lost_split",) if split else ())
    r, rows = _bnb_ratios(n, B, layer, defects=defects)
    assert rows == M
    name = f"bnb n={n} B={B} l={layer} rows={M} {'split RS ' + str(K.bnb_row_splits(M, C)) if split else 'fused'}"
    sees = {"dz": ("s0", "s1", "post", "lost_split"), "dgamma": ("post", "lost_split"), "dbeta": ("post", "lost_split"), "dbias": ("dbias",)}
    for t in ("dz", "dgamma", "dbeta", "dbias"):
        _check(name, "bnb_" + t, r[None][t], {d: r[d][t] for d in defects if d in sees[t]})


@pytest.mark.parametrize("n,B", [(8, 4), (8, 5), (6, 7), (6, 9), (8, 9), (8, 8)])
def test_small_batches_keep_half_their_columns(n, B):
    """the GPU matrix leaves a column out only when its float64 reference is identically zero (a unit dead or dropped in every row) and asks every
    tensor to keep at least half of its columns: holds for the smallest batches of the matrix on the oracle's step (fc1 / fc2 at 4 boards: 0.88)"""
    s = K.oracle_step(n, C, B)
    for layer in range(6):
        dA, a, z, g, post = K.oracle_layer(s, layer)
        kept = K.statistic(K.bn_backward(dA, a, z, g, post, F32)["dz"], K.bn_backward(dA, a, z, g, post, F64)["dz"])[1]
        assert kept >= (0.8 if layer >= 4 else 1.0), (layer, kept)


def test_bn_backward_boundary():
    """the 256-row boundary: the SAME 256 rows (conv1 of 8x8 at 4 boards) through the float64 path and through the fp32 split path, then the split
    path where it really starts (320 rows, conv4 at 272).  The fp32 path must hold the bound that the float64 path holds"""
    fused, _ = _bnb_ratios(8, 4, 0, path="fused")
    forced, _ = _bnb_ratios(8, 4, 0, path="split")
    at320, _ = _bnb_ratios(8, 5, 0)
    at272, _ = _bnb_ratios(8, 17, 3)
    at257, _ = _bnb_ratios(6, 257, 5)
    for name, r in (("256 rows fused (float64)", fused), ("256 rows forced split (fp32)", forced), ("320 rows split", at320), ("272 rows split (4x4)", at272),
                    ("257 rows split (fc2)", at257)):
        print(f"boundary {name:30s} dz {r[None]['dz']:.2f}  dgamma {r[None]['dgamma']:.2f}  dbeta {r[None]['dbeta']:.2f}  dbias {r[None]['dbias']:.2f}")
        for t in ("dz", "dgamma", "dbeta", "dbias"):
            assert 2 * r[None][t] <= K.MARGIN["bnb_" + t], (name, t)


# ------------------------------------------------------------------ heads
@pytest.mark.parametrize("flat", [0, 1])
@pytest.mark.parametrize("n,B,clip", [(6, 9, False), (8, 9, False), (8, 64, False), (6, 9, True), (8, 9, True)])
def test_heads_margins(n, B, clip, flat):
    w, own, opp, pit, zt, a5 = _heads_inputs(n, B, clip)
    if clip:
        w = K.clip_weights(w, n, flat)
    args = (a5, w[36], w[37], w[38], w[39], pit, zt, n, flat)
    r64, r32 = K.heads(*args, F64), K.heads(*args, F32)
    name = f"heads n={n} B={B} {'flat' if flat else 'rows'}{' clip' if clip else ''}"
    sees = {"dlogit": ("norm",) + (("noclip",) if clip else ()), "dvpre": ("two", "tanh"), "p": (), "v": ()}
    bad = {d: K.heads(*args, F32, defect=d) for d in ("norm", "noclip", "two", "tanh")}
    for t in ("p", "v", "dlogit", "dvpre"):
        as_vec = t in ("v", "dvpre")
        # the healthy kernel IS the float32 evaluation up to the order of 512-term dot products and of the softmax sums: ratio 1 by construction; the
        # reversed-order float32 evaluation brackets it
        rev = K.heads(a5[:, ::-1], w[36][::-1], w[37], w[38][::-1], w[39], pit, zt, n, flat, F32)
        healthy = max(1.0, _ratio(rev[t], r64[t], r32[t], as_vec))
        _check(name, "heads_" + t, healthy, {d: _ratio(bad[d][t], r64[t], r32[t], as_vec) for d in sees[t]})
    if clip:
        lo = (r64["q"] < K.CLIP_LO) & (pit > 0)
        assert lo.any() and ((r64["q"] > K.CLIP_LO) & (pit > 0)).any()
        gap_lo, gap_hi = K.clip_gap(r64["q"])
        assert gap_lo > 2e-2 and gap_hi > 100          # the GPU test asserts 1e-3 on its own reference; the upper threshold is not reached
        print(f"      clip: {int(lo.sum())} elements with a target below the lower threshold, gap {gap_lo:.3g}; the largest q is {gap_hi + 1:.3g} x 1e-7 below 1")
    # weight and bias gradients: batch order
    red64, red32, mod = K.heads_reduce(a5, r32["dlogit"], r32["dvpre"], F64), K.heads_reduce(a5, r32["dlogit"], r32["dvpre"], F32), K.model_heads_reduce(a5, r32["dlogit"], r32["dvpre"])
    lost = K.model_heads_reduce(a5[:-1], r32["dlogit"][:-1], r32["dvpre"][:-1])                                                 # the last board left out
    for t in ("dwpi", "dwv", "dbpi"):
        as_vec = t != "dwpi"
        _check(name, "heads_" + t, _ratio(mod[t], red64[t], red32[t], as_vec), {"lost_board": _ratio(lost[t], red64[t], red32[t], as_vec)})
    # two tensors of one and three numbers: the yardstick has the floor E32_FLOOR (one rounding of the stored result)
    dv = r32["dvpre"].reshape(-1, 1)
    e32 = max(K.colsum_statistic(dv.sum(dtype=F32), dv)[0], K.E32_FLOOR)
    _check(name, "heads_dbv", K.colsum_statistic(mod["dbv"], dv)[0] / e32, {"lost_board": K.colsum_statistic(lost["dbv"], dv)[0] / e32})
    # the batch-mean losses through the whole chain (k_t_heads' per-sample losses, then k_t_heads_bias' means in batch order), as the GPU test compares them
    rev = K.heads(a5[:, ::-1], w[36][::-1], w[37], w[38][::-1], w[39], pit, zt, n, flat, F32)
    l64, l32 = K.mean_losses(r64["lpi"], r64["lv"], F64), K.mean_losses(r32["lpi"], r32["lv"], F32)
    e32 = max(K.statistic(K.vec(l32), K.vec(l64))[0], K.E32_FLOOR)
    wrong = K.model_mean_losses(rev["lpi"] * F32(1 if flat else n), rev["lv"])           # the mean over the board rows missing (rows) -- flat: the same loss, no defect to show
    _check(name, "heads_loss", K.statistic(K.vec(K.model_mean_losses(rev["lpi"], rev["lv"])), K.vec(l64))[0] / e32,
           {} if flat else {"rows_mean": K.statistic(K.vec(wrong), K.vec(l64))[0] / e32})


_heads_cache = {}


def _heads_inputs(n, B, clip):
    if (n, B, clip) not in _heads_cache:
        w = K.network(n, C)
        own, opp, pit, zt = K.batch(n, B, 900, zero_row=None if clip else 3, dense_rows="all" if clip else (0,))
        s = K.oracle_step(n, C, B)                                    # a[5] of the oracle's step on the same boards (the targets do not enter a[5])
        f = K.bn_forward(s["z"][5], w[32], w[33], w[34], w[35], 5, 0.99, 0.3, 77, 0, F64)
        _heads_cache[n, B, clip] = (w, own, opp, pit, zt, f["a"].astype(F32))
    return _heads_cache[n, B, clip]


# ------------------------------------------------------------------ conv1
@pytest.mark.parametrize("n,B,cin", [(8, 4, 2), (8, 33, 2), (6, 7, 1), (6, 257, 2)])
def test_conv1_margins(n, B, cin):
    s = K.oracle_step(n, C, B, in_channels=cin)
    own, opp = s["batch"][:2]
    w = s["w"]
    z64, z32 = K.conv1_forward(own, opp, n, w[0], w[1], F64), K.conv1_forward(own, opp, n, w[0], w[1], F32)
    assert np.allclose(z64, s["z"][0], rtol=0, atol=1e-5)
    # forward: at most 18 products of a 0 / +-1 input plus the bias -- the kernel's tap order against NumPy's; a lost tap is the defect
    k = np.array(w[0]); k[2, 2] = 0
    lost = K.conv1_forward(own, opp, n, k, w[1], F32)
    _check(f"conv1 fwd n={n} B={B} cin={cin}", "conv1_fwd", 1.0, {"lost_tap": _ratio(lost, z64, z32)})
    dz0 = s["dz"][0]
    g64, g32 = K.conv1_wgrad(own, opp, n, cin, dz0, F64), K.conv1_wgrad(own, opp, n, cin, dz0, F32)
    mod, lost = K.model_conv1_wgrad(own, opp, n, cin, dz0), K.model_conv1_wgrad(own, opp, n, cin, dz0, lost_split=True)
    _check(f"conv1 wgrad n={n} B={B} cin={cin} S1={K.conv1_row_splits(B * n * n)}", "conv1_wgrad", _ratio(mod, g64, g32), {"lost_split": _ratio(lost, g64, g32)})


# ------------------------------------------------------------------ Adam
def test_adam_margins():
    s = K.oracle_step(6, C, 7)
    p = np.asarray(s["w"][30], F32).reshape(-1)                         # fc2's kernel
    rs = np.random.RandomState(3)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step in (1, 2, 3):
        g = K.adam_gradients(rs.standard_normal(p.size) * 1e-3)
        assert np.any(g == 0) and np.any(np.abs(g) > 0.5) and np.any(np.abs(g) == F32(1e-20))
        lr_t = K.adam_lr_t(1e-3, step)
        r64, r32 = K.adam(p, g, m, v, lr_t, 0.5, F64), K.adam(p, g, m, v, lr_t, 0.5, F32)
        bad = {d: K.adam(p, g, m, v, lr_t, 0.5, F32, defect=d) for d in ("clip_after", "eps_inside")}
        bad["no_b1_correction"] = K.adam(p, g, m, v, lr_t * (1 - 0.9 ** step), 0.5, F32)
        bad["no_b2_correction"] = K.adam(p, g, m, v, lr_t / np.sqrt(1 - 0.999 ** step), 0.5, F32)
        sees = {"adam_p": tuple(bad), "adam_m": ("clip_after",), "adam_v": ("clip_after",)}
        for i, key in enumerate(("adam_p", "adam_m", "adam_v")):
            # elementwise: the kernel is the float32 evaluation (healthy 1 by construction)
            _check(f"adam step {step}", key, 1.0, {d: _ratio(bad[d][i], r64[i], r32[i], True) for d in sees[key]})
        p, m, v = r32
