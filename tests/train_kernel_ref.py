"""Per-kernel references, yardsticks and summation-order models of the trainer's kernels BETWEEN the GEMMs -- TEST INFRASTRUCTURE ONLY (CPU, NumPy).

Third group after tests/layer_ref.py (network forward) and tests/train_layer_ref.py (the trainer's GEMMs): BN forward (k_t_bn_fwd_fused<32|64>, the
streaming k_t_colreduce<0|1> / k_t_fin_mean / k_t_fin_var / k_t_bn_fwd), BN backward (k_t_bn_bwd_fused; k_t_colreduce<2> + k_t_bnb_apply +
k_t_sum_partials), the heads (k_t_heads, k_t_heads_wgrad, k_t_heads_bias), conv1 (k_t_conv1_fwd, k_t_conv1_wgrad<6|8>) and k_t_adam.

Every reference is ONE kernel in float64, evaluated from the device's own tensors of the step (Trainer.preact / activation / dgrad / dz / head_grads
/ get_grad / get_weights / adam_state), and takes a `dtype`: the same code in float32 is the yardstick E32.  The kernels' own parameters enter with
the values the device holds: momentum, dropout rate, the Adam constants and lr_t are the float32 roundings (F32(0.99) is not 0.99; against the
decimal value a healthy moving statistic would be 'wrong' by 2e-8 relative).

Statistic (train_layer_ref.statistic): err = max |gpu - ref64| / norm_c, norm_c = max over the rows of |ref64[:, c]| per channel, a column whose
reference is identically zero must be exactly 0.0 and is left out.  A per-channel vector (mean, rstd, the moving statistics, dgamma, dbeta, the
heads' bias gradients) is ONE column of C rows (`vec`): its norm is the largest |entry| -- under its own entry alone a sum that nearly cancels has
an unbounded relative error in any fp32 arithmetic (train_layer_ref's docstring, few-row samples).
The bias gradient behind a training-mode BN is the column sum of dz, which is 0 in exact arithmetic: its float64 reference is the sum of the
DEVICE's dz over the rows, and its norm_c is sum |dz[:, c]| (the scale the rounding of that sum lives on), `colsum_statistic`.

Models (model_*): float32 NumPy versions that add in each kernel's own order, with switches for single defects.  tests/test_train_kernel_parity_cpu.py
evaluates them on the real tensors of an oracle step on every run; the margins below come from what they print (figures in that test's docstring),
by layer_ref's rule: a few times the modelled healthy ratio (at least twice) and at least four times below the weakest modelled defect; what
cannot separate is named there and carries the coarse bound layer_ref.MARGIN_DENSE."""
import numpy as np

import layer_ref as R
import train_layer_ref as T
from oracle import nn_numpy
from oracle.train_ref import dropout_keep

F32 = np.float32
BN_EPS = float(F32(1e-3))
CLIP_LO = float(F32(1e-7))
CLIP_HI = float(F32(1.0) - F32(1e-7))          # the kernel's 1.0f - 1e-7f
ADAM_B1, ADAM_B2, ADAM_EPS = float(F32(0.9)), float(F32(0.999)), float(F32(1e-7))
ADAM_1MB1, ADAM_1MB2 = float(F32(0.1)), float(F32(0.001))     # the kernel's literals 0.1f / 0.001f
RED_S = 256                                   # row splits of the streaming column reductions
BN_RL = 64                                    # row lanes of the fused BN kernels
BNB_MIN_ROWS = 256                            # OZ_BNB_MIN_ROWS: at most this many rows take k_t_bn_bwd_fused
MARGIN_COARSE = R.MARGIN_DENSE

# margins, x E32, per (kernel group, tensor): tests/test_train_kernel_parity_cpu.py asserts each against the models (rule above)
MARGIN = {
    # BN forward: a is an elementwise map of z under the batch statistics; the statistics are column sums
    "bnf_a": 4.0, "bnf_mean": 4.0, "bnf_rstd": 4.0, "bnf_mm": 4.0, "bnf_mv": 4.0, "bnf_mv0": 4.0,
    # BN backward
    "bnb_dz": 4.0, "bnb_dgamma": 4.0, "bnb_dbeta": 4.0, "bnb_dbias": 4.0,
    # heads
    "heads_p": 8.0, "heads_v": 8.0, "heads_dlogit": 8.0, "heads_dvpre": 8.0, "heads_loss": 8.0,
    "heads_dwpi": 6.0, "heads_dwv": 6.0, "heads_dbpi": 6.0, "heads_dbv": 4.0,
    # conv1
    "conv1_fwd": 4.0, "conv1_wgrad": 4.0,
    # Adam (elementwise)
    "adam_p": 4.0, "adam_m": 4.0, "adam_v": 4.0,
}


def rows_of(x):
    x = np.asarray(x)
    return x.reshape(-1, x.shape[-1])


def vec(x):
    """a per-channel vector as ONE column (see the module docstring)"""
    return np.asarray(x).reshape(-1, 1)


def statistic(out, ref64, norm=None):
    return T.statistic(out, ref64, norm)


KINK = 1e-5                             # relative to the channel's norm: closer to 0 than this, the sign of a BN output is not decided at fp32 precision


def a_statistic(got, f64, post, norm=None):
    """the BN forward's output a against bn_forward(...)'s float64 result f64: (err, kept, norm_c).  norm_c = max |y| post_scale over the rows, y the
    BN output BEFORE the ReLU (never zero: layer_ref's norm).  Exact: an element that dropout dropped, or whose y lies below -KINK norm_c, is 0.0"""
    y, a, keep = f64["y"], f64["a"], f64["keep"]
    own = np.abs(y).max(axis=0) * post                        # post: post_scale(layer, rate)
    norm = own if norm is None else norm
    got = rows_of(got).astype(np.float64)
    assert np.all(norm >= own) and np.all(norm > 0)
    assert np.all(got[~keep] == 0.0), "an element that dropout dropped is not exactly 0.0"
    assert np.all(got[y < -KINK * norm] == 0.0), "an element whose BN output is negative is not exactly 0.0"
    return float((np.abs(got - a) / norm).max()), 1.0, own


def colsum_statistic(out, dz_rows):
    """the bias gradient: |out[c] - sum64 dz[:, c]| / sum |dz[:, c]|, max over the columns with a non-zero dz; -> (err, kept)"""
    d = rows_of(dz_rows).astype(np.float64)
    norm = np.abs(d).sum(axis=0)
    live = norm > 0
    got = np.asarray(out, np.float64).reshape(-1)
    assert np.all(got[~live] == 0.0) and live.any()
    return float((np.abs(got - d.sum(axis=0))[live] / norm[live]).max()), float(live.mean())


# ------------------------------------------------------------------ BN forward
def post_scale(layer, rate):
    return 1.0 / (1.0 - float(F32(rate))) if layer >= 4 and rate > 0 else 1.0


def bn_stats(z, dtype):
    """(mean, biased variance, rstd) over the rows of z in `dtype`"""
    z = rows_of(z).astype(dtype)
    M = dtype(z.shape[0])
    mean = z.sum(axis=0) / M
    d = z - mean
    var = (d * d).sum(axis=0) / M
    rstd = dtype(1) / np.sqrt(var + dtype(BN_EPS))
    return mean, var, rstd


def bn_forward(z, gamma, beta, mm, mv, layer, momentum, rate, seed, step, dtype, unbiased=None, stat_rows=None, scale=True):
    """-> dict(y, a, keep, mean, rstd, mm_new, mv_new); z (boards, H, H, C) or (rows, C); layer 0 .. 5 (4 / 5 = fc1 / fc2: dropout layers 0 / 1,
    element index m C + c).  unbiased / stat_rows / scale: the defect switches of the CPU models (default: the kernel's rule)"""
    z = rows_of(z).astype(dtype)
    M, C = z.shape
    mean, var, rstd = bn_stats(z, dtype)
    if stat_rows is not None:                  # defect: statistics over Bmax P rows (the rows past M read as zeros)
        zz = np.zeros((stat_rows, C), dtype); zz[:M] = z
        mean, var, rstd = bn_stats(zz, dtype)
    g, b = np.asarray(gamma, dtype), np.asarray(beta, dtype)
    y = (z - mean) * rstd * g + b
    a = np.maximum(y, dtype(0))
    keep = np.ones((M, C), bool)
    if layer >= 4 and rate > 0:
        keep = dropout_keep(seed, step, layer - 4, M * C, rate).reshape(M, C)
        a = np.where(keep, a / (dtype(1) - dtype(F32(rate))) if scale else a, dtype(0))
    mom = dtype(F32(momentum))
    unb = (layer < 4) if unbiased is None else unbiased
    Ms = stat_rows or M
    uv = var * (dtype(Ms) / dtype(max(Ms - 1, 1))) if unb else var
    out = dict(y=y, a=a, keep=keep, mean=mean, rstd=rstd, mm_new=np.asarray(mm, dtype) * mom + mean * (dtype(1) - mom),
               mv_new=np.asarray(mv, dtype) * mom + uv * (dtype(1) - mom))
    assert all(v.dtype == dtype for k, v in out.items() if k != "keep")
    return out


def _seq_lanes(x, lanes=BN_RL):
    """column sums of x (rows, C) in float32 as the fused kernels add: row lane r adds rows r, r + lanes, ... in order, then the lane sums in lane order"""
    x = np.asarray(x, F32)
    M, C = x.shape
    pad = np.zeros((-(-M // lanes) * lanes, C), F32); pad[:M] = x
    part = np.zeros((lanes, C), F32)
    for blk in pad.reshape(-1, lanes, C):
        part = part + blk
    s = np.zeros(C, F32)
    for r in range(lanes):
        s = s + part[r]
    return s


def _split_sums(x, splits, rpp):
    """k_t_colreduce: split sp, row group rsub adds rows (sp rpp + rsub) + k splits rpp in order; the rpp groups of a block in order -> (splits, C)"""
    x = np.asarray(x, F32)
    M, C = x.shape
    stride = splits * rpp
    pad = np.zeros((-(-M // stride) * stride, C), F32); pad[:M] = x
    acc = np.zeros((stride, C), F32)
    for blk in pad.reshape(-1, stride, C):
        acc = acc + blk
    acc = acc.reshape(splits, rpp, C)
    out = acc[:, 0].copy()
    for k in range(1, rpp):
        out = out + acc[:, k]
    return out


def _in_order(parts):
    s = np.zeros_like(parts[0])
    for p in parts:
        s = s + p
    return s


def rows_per_pass(C):
    q = C // 4
    return 256 // min(q, 64)


def bnb_row_splits(M, C):
    """t_bn_backward's RS"""
    rs = 16
    while rs < 256 and M > rs * rows_per_pass(C) * 8:
        rs *= 2
    return rs


def conv1_row_splits(rows):
    s1 = 8
    while s1 < RED_S and rows > 16 * s1:
        s1 *= 2
    return s1


def bnf_regime(M):
    return "fused32" if M <= 2048 else "fused64" if M <= 4096 else "stream"


def model_bn_forward(z, gamma, beta, mm, mv, layer, momentum, rate, seed, step, defect=None):
    """float32 BN forward in the order of the regime that M rows take (bnf_regime).  defect: None | 'unbiased_rstd' | 'tail' (the rows of the
    last partial pass of 64 left out of the sums) | 'scale' (1 / (1 - rate) missing) | 'mv_kind' (the moving variance of the other kind of layer)"""
    z = rows_of(z).astype(F32)
    M, C = z.shape
    regime = bnf_regime(M)
    zs = z[:M - M % BN_RL] if defect == "tail" and M % BN_RL else z
    if regime == "stream":
        add = lambda x: _in_order(_split_sums(x, RED_S, rows_per_pass(C)))
    else:
        add = _seq_lanes
    mean = add(zs) / F32(M)
    d = zs - mean
    var = add(d * d) / F32(M)
    if defect == "unbiased_rstd":
        var = var * (F32(M) / F32(M - 1))
    rstd = F32(1) / np.sqrt(var + F32(1e-3))
    y = (z - mean) * rstd * np.asarray(gamma, F32) + np.asarray(beta, F32)
    a = np.maximum(y, F32(0))
    if layer >= 4 and rate > 0:
        keep = dropout_keep(seed, step, layer - 4, M * C, rate).reshape(M, C)
        a = np.where(keep, a if defect == "scale" else a / (F32(1) - F32(rate)), F32(0))
    mom = F32(momentum)
    unb = (layer < 4) != (defect == "mv_kind")
    uv = var * (F32(M) / F32(max(M - 1, 1))) if unb else var
    return dict(a=a, mean=mean, rstd=rstd, mm_new=np.asarray(mm, F32) * mom + mean * (F32(1) - mom), mv_new=np.asarray(mv, F32) * mom + uv * (F32(1) - mom))


# ------------------------------------------------------------------ BN backward
def bn_backward(dA, a, z, gamma, post, dtype, live=None):
    """-> dict(dz (rows, C), dgamma, dbeta, dbias); dy = dA post where a > 0 (or where `live`, a mask given by hand), else 0"""
    dA, z = rows_of(dA).astype(dtype), rows_of(z).astype(dtype)
    live = rows_of(a) > 0 if live is None else live
    M = dtype(z.shape[0])
    mean, _, rstd = bn_stats(z, dtype)
    dy = np.where(live, dA * dtype(post), dtype(0))
    xh = (z - mean) * rstd
    S0, S1 = dy.sum(axis=0), (dy * xh).sum(axis=0)
    dz = np.asarray(gamma, dtype) * rstd * (dy - S0 / M - xh * S1 / M)
    out = dict(dz=dz, dgamma=S1, dbeta=S0, dbias=dz.sum(axis=0))
    assert all(v.dtype == dtype for v in out.values())
    return out


def model_bn_backward(dA, a, z, gamma, post, mean32=None, rstd32=None, path=None, defect=None):
    """float32 / float64 BN backward in the kernels' own arithmetic.  path 'fused' (k_t_bn_bwd_fused: float64 sums over 64 row lanes, centred on its
    own float64 mean, the forward's fp32 rstd, dz rounded once) or 'split' (fp32, the forward's rounded mean and rstd, RS x rpp row splits, RS
    partials over rpp lanes, bias gradient = the RS block sums in order); default: by the row count.
    defect: None | 's0' (the S0 / M term missing) | 's1' (xhat S1 / M missing) | 'post' | 'lost_split' (one row split's partial) | 'dbias' (= dbeta)"""
    dA, a, z = rows_of(dA).astype(F32), rows_of(a), rows_of(z).astype(F32)
    M, C = z.shape
    if mean32 is None:
        f = model_bn_forward(z, np.ones(C), np.zeros(C), np.zeros(C), np.zeros(C), 0, 0.99, 0.0, 0, 0)
        mean32, rstd32 = f["mean"], f["rstd"]
    path = path or ("fused" if M <= BNB_MIN_ROWS else "split")
    ps = F32(1) if defect == "post" else F32(post)
    dy = np.where(a > 0, dA * ps, F32(0)).astype(F32)
    g = np.asarray(gamma, F32)
    if path == "fused":
        dy64, z64, rs = dy.astype(np.float64), z.astype(np.float64), rstd32.astype(np.float64)
        S0 = dy64.sum(axis=0)
        mu = z64.sum(axis=0) / M
        S1 = ((dy64 * z64).sum(axis=0) - mu * S0) * rs
        xh = (z64 - mu) * rs
        gd = g.astype(np.float64) * rs * (dy64 - (0 if defect == "s0" else S0 / M) - (0 if defect == "s1" else xh * S1 / M))
        return dict(dz=gd.astype(F32), dgamma=S1.astype(F32), dbeta=S0.astype(F32), dbias=(S0 if defect == "dbias" else gd.sum(axis=0)).astype(F32))
    RS, rpp = bnb_row_splits(M, C), rows_per_pass(C)
    xh = (z - mean32) * rstd32
    p0, p1 = _split_sums(dy, RS, rpp), _split_sums(dy * xh, RS, rpp)           # (fmaf(dy, xh, s1): the product is not rounded; below the model's resolution)
    if defect == "lost_split":
        p0, p1 = p0[:-1], p1[:-1]
    # k_t_bnb_apply: row lane r adds the partials r, r + rpp, ..., then the rpp lane sums in order
    fin = lambda p: _in_order([_in_order(list(p[r::rpp])) for r in range(min(rpp, len(p)))])
    S0, S1 = fin(p0), fin(p1)
    inv = F32(1) / F32(M)
    dz = g * rstd32 * (dy - (F32(0) if defect == "s0" else S0 * inv) - (F32(0) if defect == "s1" else xh * S1 * inv))
    dz = dz.astype(F32)
    dbias = S0 if defect == "dbias" else _in_order(list(_split_sums(dz, RS, rpp)))
    return dict(dz=dz, dgamma=S1, dbeta=S0, dbias=dbias.astype(F32))


# ------------------------------------------------------------------ heads
def heads(a5, wpi, bpi, wv, bv, pit, zt, n, flat, dtype, defect=None):
    """-> dict(p, v, lpi, lv (per sample), dlogit, dvpre); flat: OZ_POLICY_LOSS_FLAT (one group of n n lanes) or rows (n groups of n).
    defect (CPU models): None | 'norm' (1 / B for 1 / (B n) and back) | 'noclip' (gradient kept outside the clip) | 'two' | 'tanh'"""
    x = np.asarray(a5, dtype)
    B, A = x.shape[0], n * n
    logit = x @ np.asarray(wpi, dtype) + np.asarray(bpi, dtype)
    e = np.exp(logit - logit.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    v = np.tanh(x @ np.asarray(wv, dtype).reshape(-1) + np.asarray(bv, dtype).reshape(-1)[0])
    grp = (B, 1, A) if flat else (B, n, n)
    t = np.asarray(pit, dtype).reshape(grp)
    pg = p.reshape(grp)
    S = pg.sum(axis=2, keepdims=True)
    q = pg / S
    inside = (q >= dtype(CLIP_LO)) & (q <= dtype(CLIP_HI))
    qc = np.clip(q, dtype(CLIP_LO), dtype(CLIP_HI))
    lpi = -(t * np.log(qc)).sum(axis=(1, 2)) / dtype(1 if flat else n)
    with np.errstate(divide="ignore", invalid="ignore"):
        gq = np.where(inside | (defect == "noclip"), -t / q, dtype(0))
    rowdot = (gq * q).sum(axis=2, keepdims=True)
    normp = dtype(1) / dtype(B) if bool(flat) != (defect == "norm") else dtype(1) / (dtype(B) * dtype(n))
    gp = ((gq - rowdot) / S * normp).reshape(B, A)
    dlogit = p * (gp - (gp * p).sum(axis=1, keepdims=True))
    d = v - np.asarray(zt, dtype).reshape(-1)
    dvpre = dtype(1 if defect == "two" else 2) * d / dtype(B) * (dtype(1) if defect == "tanh" else dtype(1) - v * v)
    out = dict(p=p, v=v, lpi=lpi, lv=d * d, dlogit=dlogit, dvpre=dvpre, q=q.reshape(B, A), inside=inside.reshape(B, A))
    assert all(o.dtype == dtype for k, o in out.items() if k != "inside")
    return out


def heads_reduce(a5, dlogit, dvpre, dtype):
    """from the heads' own outputs: dict(dwpi (512, A), dwv (512,), dbpi (A,), dbv ())"""
    x, dl, dv = np.asarray(a5, dtype), np.asarray(dlogit, dtype), np.asarray(dvpre, dtype).reshape(-1)
    return dict(dwpi=x.T @ dl, dwv=x.T @ dv, dbpi=dl.sum(axis=0), dbv=dv.sum())


def mean_losses(lpi, lv, dtype):
    lp, lvm = np.asarray(lpi, dtype).sum() / dtype(len(lpi)), np.asarray(lv, dtype).sum() / dtype(len(lv))
    return np.array([lp + lvm, lp, lvm], dtype)


def model_heads_reduce(a5, dlogit, dvpre):
    """k_t_heads_wgrad / k_t_heads_bias: float32, batch order"""
    x, dl, dv = np.asarray(a5, F32), np.asarray(dlogit, F32), np.asarray(dvpre, F32).reshape(-1)
    dw, dwv, db, dbv = np.zeros((x.shape[1], dl.shape[1]), F32), np.zeros(x.shape[1], F32), np.zeros(dl.shape[1], F32), F32(0)
    for b in range(x.shape[0]):
        dw = (dw.astype(np.float64) + np.outer(x[b], dl[b]).astype(np.float64)).astype(F32)          # fmaf: one rounding per term
        dwv = (dwv.astype(np.float64) + x[b].astype(np.float64) * float(dv[b])).astype(F32)
        db = db + dl[b]
        dbv = F32(dbv + dv[b])
    return dict(dwpi=dw, dwv=dwv, dbpi=db, dbv=dbv)


E32_FLOOR = 2.0 ** -24                 # a tensor of a few numbers: E32 of one run is a single draw; the rounding of the stored fp32 result alone is this


def model_mean_losses(lpi, lv):
    """k_t_heads_bias: float32, batch order"""
    lp, lvm = F32(0), F32(0)
    for a, b in zip(np.asarray(lpi, F32), np.asarray(lv, F32)):
        lp, lvm = F32(lp + a), F32(lvm + b)
    lp, lvm = lp / F32(len(lpi)), lvm / F32(len(lv))
    return np.array([lp + lvm, lp, lvm], F32)


# ------------------------------------------------------------------ conv1
def conv1_planes(own, opp, n, in_channels, dtype):
    x = nn_numpy.planes(own, opp, n, dtype)
    return x[..., 0:1] - x[..., 1:2] if in_channels == 1 else x


def conv1_forward(own, opp, n, kernel, bias, dtype):
    """z[0] (boards, n, n, C)"""
    k = np.asarray(kernel, dtype)
    x = conv1_planes(own, opp, n, k.shape[2], dtype)
    return nn_numpy._conv3x3(x, k, np.asarray(bias, dtype), True).reshape(x.shape[0], n, n, -1)


def conv1_wgrad(own, opp, n, in_channels, dz0, dtype):
    """dW1 (3, 3, in_channels, C) from the boards and dz[0]"""
    return T.wgrad(1, conv1_planes(own, opp, n, in_channels, dtype), np.asarray(dz0, dtype), dtype)


def model_conv1_wgrad(own, opp, n, in_channels, dz0, lost_split=False):
    """k_t_conv1_wgrad: float32, split sp adds the rows sp, sp + S1, ... in order (every term is +-dz or 0: the fmaf is an add), then the S1 partials in order"""
    x = conv1_planes(own, opp, n, in_channels, F32)
    B = x.shape[0]
    dz = np.asarray(dz0, F32).reshape(B * n * n, -1)
    S1 = conv1_row_splits(B * n * n)
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((3, 3, in_channels, dz.shape[1]), F32)
    for ty in range(3):
        for tx in range(3):
            win = xp[:, ty:ty + n, tx:tx + n, :].reshape(B * n * n, in_channels)
            for ch in range(in_channels):
                parts = _split_sums(win[:, ch:ch + 1] * dz, S1, 1)
                out[ty, tx, ch] = _in_order(list(parts[:-1] if lost_split else parts))
    return out


# ------------------------------------------------------------------ Adam
def adam_lr_t(lr, step):
    """the host's lr_t of optimiser step `step` (1-based), as the float the kernel receives"""
    return float(F32(float(F32(lr)) * np.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step)))


def adam_gradients(g):
    """the Adam cases' gradients: a step's own (any shape, returned flat), with every 7th element exactly 0, every 7th beyond +-clip (x 1e4), every 7th
    +-1e-20 and every 7th +-1e-6 (where eps and sqrt(v) are of one size)"""
    g = np.array(g, F32).reshape(-1)
    g[0::7] = 0
    g[1::7] *= F32(1e4)
    g[2::7] = np.where(g[2::7] < 0, F32(-1e-20), F32(1e-20))
    g[3::7] = np.where(g[3::7] < 0, F32(-1e-6), F32(1e-6))
    return g


def adam(p, g, m, v, lr_t, clip, dtype, defect=None):
    """-> (p, m, v) after the step.  defect (CPU models): None | 'clip_after' | 'eps_inside' (lr_t comes from adam_lr_t; its defects are made there)"""
    p, g, m, v = (np.asarray(x, dtype) for x in (p, g, m, v))
    gc = np.clip(g, dtype(-clip), dtype(clip)) if clip > 0 else g
    gm = g if defect == "clip_after" else gc
    m2 = dtype(ADAM_B1) * m + dtype(ADAM_1MB1) * gm
    v2 = dtype(ADAM_B2) * v + dtype(ADAM_1MB2) * gm * gm
    if defect == "clip_after" and clip > 0:
        m2 = np.clip(m2, dtype(-clip), dtype(clip))
    den = np.sqrt(v2 + dtype(ADAM_EPS)) if defect == "eps_inside" else np.sqrt(v2) + dtype(ADAM_EPS)
    p2 = p - dtype(lr_t) * m2 / den
    assert p2.dtype == dtype and m2.dtype == dtype and v2.dtype == dtype
    return p2, m2, v2


# ------------------------------------------------------------------ batches and the oracle step (shared by the CPU and the GPU test)
def batch(n, B, seed, zero_row=None, dense_rows=(0,)):
    """random boards, one-hot policy targets, Dirichlet targets on `dense_rows` ('all': every board), an all-zero target on board `zero_row`, z = +-1"""
    rs = np.random.RandomState(seed)
    valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
    own = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid
    opp = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid & ~own
    pi = np.zeros((B, n * n), F32)
    pi[np.arange(B), rs.randint(0, n * n, B)] = 1
    for b in (range(B) if dense_rows == "all" else dense_rows):
        pi[b] = rs.dirichlet(np.ones(n * n)).astype(F32)
    if zero_row is not None:
        pi[zero_row] = 0
    z = rs.choice([-1.0, 1.0], B).astype(F32)
    return own, opp, pi, z


# The clip case: the policy head's kernel times CLIP_SCALE[board, flat], so that logits differ by more than ln 1e7 = 16.1 and some q = p / S fall below
# 1e-7.  Chosen on the CPU (a scan of the scale in steps of 1 / 8 on a[5] of the oracle's step on batch(n, 9, 900), dense targets on every board) for the
# widest gap between any q and the lower threshold: 0.27 / 0.06 / 0.044 / 0.08 relative, with 13 / 219 / 32 / 418 elements below it.  The largest q
# stays 4e-5 or more below 1: the UPPER threshold is not reached (in fp32 1 - q resolves to 6e-8, so a q near 1 - 1e-7 cannot be placed on a side).
CLIP_SCALE = {(6, 0): 4.25, (6, 1): 7.375, (8, 0): 4.125, (8, 1): 7.875}


def clip_weights(w, n, flat):
    w = [np.array(a) for a in w]
    w[36] = (w[36] * F32(CLIP_SCALE[n, int(flat)])).astype(F32)
    return w


def clip_gap(q):
    """(the smallest relative distance of any q to the lower threshold, the smallest (1 - q) / 1e-7 - 1 towards the upper one)"""
    q = np.asarray(q, np.float64)
    return float(np.abs(q / CLIP_LO - 1).min()), float(((1 - q) / (1 - CLIP_HI) - 1).min())


_oracle_cache = {}


def oracle_step(n, C, B, in_channels=2, seed=900, rate=0.3):
    """one float64 oracle step (oracle/train_ref.py) on the dense network as fp32 tensors: dict(w, batch, z[0..5], dy[0..5] (the gradient wrt the BN
    output: the masked, scaled dA), dz[0..5], a5)"""
    key = (n, C, B, in_channels, seed, rate)
    if key not in _oracle_cache:
        import torch
        from oracle.train_ref import TrainRef
        w = network(n, C, in_channels)

        class Tap(TrainRef):
            def _bn_train(self, z, blk, fused):
                z.retain_grad()
                y = super()._bn_train(z, blk, fused)
                y.retain_grad()
                self.zs.append(z); self.ys.append(y)
                return y
        t = Tap(w, n, dropout=rate, seed=77)
        t.zs, t.ys = [], []
        bt = batch(n, B, seed)
        t.forward_backward(*bt)
        f = lambda x: x.detach().numpy().astype(F32)
        _oracle_cache[key] = dict(w=w, batch=bt, z=[f(z) for z in t.zs], dy=[f(y.grad) for y in t.ys], dz=[f(z.grad) for z in t.zs])
    return _oracle_cache[key]


def network(n, C, in_channels=2):
    """the dense test network (layer_ref.network_weights: every parameter kind randomised, gamma and beta included); in_channels 1: conv1's kernel
    is the difference of its two input planes' kernels (BaseNN's single +-1 plane)"""
    w = R.network_weights(n, C, "dense")
    if in_channels == 1:
        w = list(w)
        w[0] = np.ascontiguousarray(w[0][:, :, 0:1, :] - w[0][:, :, 1:2, :])
    return w


def oracle_layer(step, layer, rate=0.3, seed=77):
    """(dA, a, z, gamma, post) of BN layer `layer` of an oracle step, as the BN backward kernels receive them: a from the float64 BN forward of z, dA =
    dy / post where a > 0 and a value of dy's scale elsewhere (it must not enter)"""
    w, z, dy = step["w"], step["z"][layer], step["dy"][layer]
    f = bn_forward(z, w[6 * layer + 2], w[6 * layer + 3], w[6 * layer + 4], w[6 * layer + 5], layer, 0.99, rate, seed, 0, np.float64)
    post = post_scale(layer, rate)
    a = f["a"].astype(F32)
    d = rows_of(dy).astype(np.float64)
    noise = np.random.RandomState(5 + layer).standard_normal(d.shape) * (np.abs(d).mean() + 1e-30)
    dA = np.where(a > 0, d / post, noise).astype(F32)
    return dA, a, rows_of(z), np.asarray(w[6 * layer + 2]), post
