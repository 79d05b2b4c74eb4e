"""Per-kernel references and yardsticks of the TRAINER's GEMMs -- TEST INFRASTRUCTURE ONLY (CPU, NumPy).  Builds on tests/layer_ref.py.

One GEMM of one layer l = 1 .. 5 (conv2 .. fc2) of one training step at a time, each evaluated in float64 from the device's OWN tensors of that
step (Trainer.activation / preact / dz / dgrad), so that every kernel is judged on its own -- BN conditioning, dropout and upstream rounding do not enter:
  forward          z[l]        = conv_or_matmul(a[l - 1]) + bias                      against Trainer.preact(l)
  data gradient    dA[l - 1]   = conv(dz[l] interior, reversed and swapped kernel)    against Trainer.dgrad(l - 1)   (dense: dz . W^T; the raw GEMM output)
  weight gradient  dW[t,ci,co] = sum over the rows (b, pixel) of x . dz               against Trainer.get_grads()[6 l]
and the heads' data gradient dlogit . Wpi^T + dvpre . Wv^T against Trainer.dgrad(5).

Statistic (as layer_ref): err = max |gpu - ref64| / norm_c, norm_c = max over the compared rows of |ref64[:, c]| per output column of THAT GEMM -- the
output channel for the forward, the input channel for the data gradient, co over all (tap, ci) for the weight gradient.  A column whose float64
reference is identically zero (a unit dead in every row: its dz is 0) must be exactly 0.0 on the device and is left out of the ratio.  Yardstick:
E32 = the same statistic for the same operation evaluated in NumPy float32 from the same inputs.

Margins.  Two classes.  SHARP: a short sum, where the accuracy of the PRODUCTS is what is left -- the forward and the data gradient on the
'bisparse' network (layer_ref.bisparse_kernel: 8 entries per output column AND per input channel), the weight gradient of conv4 over at most 36 rows and k_wgrad_h2's up to 4096 (its sum
runs over the rows B x P; the weights do not enter, so a short sum is the only lever).  COARSE: everything else (the dense network; the weight
gradient of many rows), bound layer_ref.MARGIN_DENSE.  The sharp margins come from NumPy models of the two split arithmetics on these contractions
(model_dgrad, model_wgrad below), evaluated by tests/test_train_layer_parity_cpu.py on every run -- complete arithmetic and every single kept term
removed, relative to E32 -- never from what a kernel returns; the rule is layer_ref's: a few times the modelled healthy ratio and at least four
times below the weakest single-term defect.  Which (arithmetic, contraction, rows) is sharp is `wgrad_class` / the constants below; the CPU test
asserts that the model agrees, and names the shapes that cannot separate (they are coarse).  The figures the model printed when the constants were
written are in that test's docstring.
Few-row samples: a dense layer of a B-board step has B rows; under the norm of a few rows the statistic is an element's relative error (layer_ref's
docstring).  A case of fewer than ROWS_FOR_NORM boards therefore runs several steps on fresh batches (same weights) and takes norm_c over the rows of
all of them; every element of every step is still compared."""
import numpy as np

import layer_ref as R
from oracle import nn_numpy

ROWS_FOR_NORM = 64                     # as the forward matrix: a case's norm rests on at least 64 boards

# sharp margins, x E32 (derivation: the module docstring and tests/test_train_layer_parity_cpu.py)
MARGIN_FWD = R.MARGIN                                            # the forward on 8 entries per output column: the merged forward work's margins
MARGIN_DGRAD = {"f32": 8.0, "bf16x3": 8.0, "f16x2": 16.0}       # bisparse data gradient; the exact-fp32 kernels are held to bf16x3's margin
MARGIN_WGRAD = {"f32": 4.5, "bf16x3": 4.5, "f16x2": 6.0}        # weight gradient of a 3x3 layer over few rows
# where the model separates: (layers, rows B x P inclusive).  bf16x3 / f32: conv4 up to 36 rows; f16x2 (k_wgrad_h2): every 3x3 layer, 128 .. 4096 rows
WGRAD_SHARP = {"f32": ((3,), 1, 36), "bf16x3": ((3,), 1, 36), "f16x2": ((1, 2, 3), 128, 4096)}
MARGIN_COARSE = R.MARGIN_DENSE


def wgrad_class(arith, layer, rows):
    """'sharp' or 'coarse' for the weight gradient of `layer` summed over `rows` = B x P rows by a kernel of arithmetic `arith` (f32: k_wgrad_f32 /
    k_wgrad_conv, f16x2: k_wgrad_h2, bf16x3: k_wgrad_b3).  Only the 3x3 layers are modelled: the dense layers' weight gradients are coarse"""
    layers, lo, hi = WGRAD_SHARP[arith]
    return "sharp" if layer in layers and lo <= rows <= hi else "coarse"


# ------------------------------------------------------------------ geometry
def geometry(n, C, layer):
    """dict(Hin, Hout, same, taps, Cin, Co, zoff, Hz) of layer 1 .. 5; zoff / Hz: conv3 and conv4 keep dz in a zero-bordered Hz x Hz buffer"""
    hin, hout, same, taps, K, N = R.layer_geometry(n, C, layer)
    zoff = 2 if layer in (2, 3) else 0
    return dict(Hin=hin, Hout=hout, same=same, taps=taps, Cin=K // taps, Co=N, zoff=zoff, Hz=hout + 2 * zoff)


# ------------------------------------------------------------------ the three contractions of a layer, in any dtype
def forward_z(weights, layer, x_in, dtype):
    """z = conv_or_matmul(x_in) + bias: (boards, Hout, Hout, Co), dense layers (boards, 1, 1, Co)"""
    k, bias = (np.asarray(a, dtype) for a in weights[6 * layer:6 * layer + 2])
    x = np.asarray(x_in, dtype)
    if layer <= 3:
        hout = x.shape[1] - (0 if layer == 1 else 2)
        return nn_numpy._conv3x3(x, k, bias, same=(layer == 1)).reshape(x.shape[0], hout, hout, -1)
    return (x.reshape(x.shape[0], -1) @ k + bias).reshape(x.shape[0], 1, 1, -1)


def dgrad(weights, layer, dz_int, dtype):
    """the gradient wrt the layer's input from dz (interior, (boards, Hout, Hout, Co)): (boards, Hin, Hin, Cin) -- tap by tap,
    dX[b, oy + ty - pad, ox + tx - pad, ci] += dz[b, oy, ox, :] . W[ty, tx, ci, :]; dense: dz . W^T as (boards, 1, 1, K)"""
    k = np.asarray(weights[6 * layer], dtype)
    dz = np.asarray(dz_int, dtype)
    if layer > 3:
        return (dz.reshape(dz.shape[0], -1) @ k.T).reshape(dz.shape[0], 1, 1, -1)
    B, hout = dz.shape[0], dz.shape[1]
    pad = 1 if layer == 1 else 0
    hin = hout + 2 - 2 * pad
    out = np.zeros((B, hin + 2 * pad, hin + 2 * pad, k.shape[2]), dtype)
    flat = np.ascontiguousarray(dz).reshape(B * hout * hout, -1)
    for ty in range(3):
        for tx in range(3):
            out[:, ty:ty + hout, tx:tx + hout, :] += (flat @ np.ascontiguousarray(k[ty, tx].T)).reshape(B, hout, hout, -1)
    assert out.dtype == dtype
    return out[:, pad:pad + hin, pad:pad + hin, :]


def wgrad(layer, x_in, dz_int, dtype):
    """dW[ty, tx, ci, co] = sum over (b, oy, ox) of x[b, oy + ty - pad, ox + tx - pad, ci] dz[b, oy, ox, co]; dense: x^T . dz as (K, N)"""
    x, dz = np.asarray(x_in, dtype), np.asarray(dz_int, dtype)
    if layer > 3:
        return x.reshape(x.shape[0], -1).T @ dz.reshape(dz.shape[0], -1)
    B, hout = dz.shape[0], dz.shape[1]
    if layer == 1:
        x = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    flat = np.ascontiguousarray(dz).reshape(B * hout * hout, -1)
    out = np.zeros((3, 3, x.shape[3], flat.shape[1]), dtype)
    for ty in range(3):
        for tx in range(3):
            win = np.ascontiguousarray(x[:, ty:ty + hout, tx:tx + hout, :]).reshape(B * hout * hout, -1)
            out[ty, tx] = win.T @ flat
    assert out.dtype == dtype
    return out


def heads_dgrad(weights, dlogit, dvpre, dtype):
    """the gradient wrt fc2's output: dlogit . Wpi^T + dvpre . Wv^T, (boards, 1, 1, 512)"""
    wpi, wv = np.asarray(weights[36], dtype), np.asarray(weights[38], dtype).reshape(-1)
    dl, dv = np.asarray(dlogit, dtype), np.asarray(dvpre, dtype).reshape(-1, 1)
    return (dl @ wpi.T + dv * wv[None, :]).reshape(dl.shape[0], 1, 1, -1)


# ------------------------------------------------------------------ statistic
def column_norm(ref64):
    """norm_c = max over everything but the last axis of |ref64[..., c]|"""
    r = np.abs(np.asarray(ref64, np.float64))
    return r.reshape(-1, r.shape[-1]).max(axis=0)


def statistic(out, ref64, norm=None):
    """(max |out - ref64| / norm_c over the columns with norm_c > 0, fraction of such columns); a column whose reference is identically zero must be
    exactly 0.0 in `out` (asserted).  `norm`: norm_c over a larger sample of rows of the same tensor which includes these"""
    ref = np.asarray(ref64, np.float64)
    ref = ref.reshape(-1, ref.shape[-1])
    got = np.asarray(out, np.float64).reshape(ref.shape)
    own = column_norm(ref)
    if norm is None:
        norm = own
    assert np.all(norm >= own)
    dead = own == 0
    assert np.all(got[:, dead] == 0.0), "a column whose float64 reference is identically zero is not exactly 0.0"
    live = norm > 0
    assert live.any()
    return float((np.abs(got - ref)[:, live] / norm[live]).max()), float((~dead).mean())


# ------------------------------------------------------------------ NumPy models of the split arithmetics on the trainer's contractions (CPU test only)
def dz_like(rs, rows, C):
    """rows of a gradient tensor: dense (the BN backward leaves no zeros), a scale per channel (gamma x rstd of the BN) spread over a few binary
    orders, so that most elements lie well below the tensor's maximum -- what the per-tensor scaling of the f16x2 mode has to cope with"""
    return (rs.standard_normal((rows, C)) * np.exp(rs.normal(0, 1, C))[None, :] * 1e-3).astype(np.float32)


def act_like(rs, rows, C):
    """rows of a post-ReLU activation: a third zeros (layer_ref's CPU test uses the same draw)"""
    return np.maximum(rs.normal(0.1, 0.4, size=(rows, C)), 0).astype(np.float32)


def dgrad_table(kernel):
    """the data-gradient operand of a bisparse 3x3 kernel (3, 3, Cin, Co) as the GEMM sees it: per input channel (= output column of that GEMM) the k'
    indices (ascending) and values of its entries, k' = (slice * 9 + (8 - tap)) * 32 + c32 with co = slice * 32 + c32 (t_kp_tap_channel, t_wd_load8:
    the reversed, channel-swapped taps) -> (idx (nnz, Cin), val (nnz, Cin), K')"""
    w = np.asarray(kernel, np.float32)
    _, _, cin, co = w.shape
    t, ci, o = np.nonzero(w.reshape(9, cin, co))
    kp = ((o // 32) * 9 + (8 - t)) * 32 + o % 32
    nnz = np.bincount(ci, minlength=cin)
    assert np.all(nnz == nnz[0])
    order = np.lexsort((kp, ci))
    idx = kp[order].reshape(cin, nnz[0]).T
    val = w.reshape(9, cin, co)[t[order], ci[order], o[order]].reshape(cin, nnz[0]).T
    return idx, val, 9 * co


def _tensor_exp(x, target):
    """t_exp_for: the power of two that brings the tensor's |maximum| to <= target"""
    return int(np.floor(np.log2(target / np.abs(x).max())))


def model_dgrad(kernel, dz_rows, arith, drop=None):
    """the data gradient of a bisparse 3x3 layer on rows `dz_rows` (rows, K') (a pixel whose nine taps all lie inside the buffer) in a split arithmetic:
    bf16x3 -- both operands as three bf16 planes, the kept cross terms (R.B3_TERMS without `drop`) accumulated in fp32 per 32-wide k-tile, small terms
    first; f16x2 -- dz moved by the power of two that brings the TENSOR's maximum to 8192 (k_t_dz_to_h2), the weights by the one that brings theirs to
    1000 (k_t_w_to_h2), two fp16 planes each, the kept terms of R.H2_TERMS, the inverse powers multiplied back in fp32 (exact)"""
    idx, val, _ = dgrad_table(kernel)
    a = np.asarray(dz_rows, np.float32)
    if arith == "bf16x3":
        ap, wp, terms, back = R.b3_planes(a), R.b3_planes(val), R.B3_TERMS, 0
    else:
        ez, kexp = _tensor_exp(a, 8192.0), _tensor_exp(np.asarray(kernel), 1000.0)
        ap, wp, terms, back = R.h2_planes(np.ldexp(a, ez)), R.h2_planes(np.ldexp(val, kexp)), R.H2_TERMS, -(ez + kexp)
    prods = [ap[i - 1][:, idx].transpose(1, 0, 2).astype(np.float64) * wp[j - 1][:, None, :].astype(np.float64) for (i, j) in terms if (i, j) != drop]
    return np.ldexp(R._accumulate(idx, prods), back).astype(np.float32)


def wgrad_groups(B, hout):
    """the k-steps of the octet weight gradient (wgrad_oct_body) as lists of rows m = (b * hout + oy) * hout + ox: per octet of 8 boards, per output
    row, two quads of four pixel slots x 8 boards (slots >= hout and boards >= B hold zeros: left out, an empty k-step adds nothing)"""
    groups = []
    for oct_ in range((B + 7) // 8):
        for oy in range(hout):
            for quad in range(2):
                rows = [(b * hout + oy) * hout + ox for ox in range(quad * 4, min(quad * 4 + 4, hout)) for b in range(oct_ * 8, min(oct_ * 8 + 8, B))]
                if rows:
                    groups.append((oct_, rows))
    return groups


def wgrad_msplit(B, tiles, arith):
    """t_wgrad_oct's octet split (the slab budget never binds at these sizes)"""
    noct, msplit = (B + 7) // 8, 1
    while msplit < 32 and tiles * msplit < 256 and msplit * 2 <= noct:
        msplit *= 2
    return msplit


def model_wgrad(x_rows, dz_rows, B, hout, arith, msplit=1, drop=None, inner="exact"):
    """one tap of the octet weight gradient on x_rows (B hout^2, Ci), dz_rows (B hout^2, Co): per k-step (wgrad_groups) one MFMA per kept plane
    product, in mac()'s order (small terms first: R.B3_TERMS / R.H2_TERMS read as (plane of x, plane of dz)), each adding its exact products to the
    fp32 accumulator; octets split over `msplit` slabs that are summed in fp32 in slab order (k_t_sum_partials).  f16x2: dz moved by the power of
    two that brings the tensor's maximum to 8192 (k_t_z_octets), x unscaled (post-ReLU values), the power taken back in the epilogue.
    inner: how one MFMA adds its (up to) 32 products to the accumulator, which the instruction set does not specify -- "exact": their exact sum,
    rounded to fp32 once (the most a 16-bit matrix core can do); "sequential": one by one in k order, each sum rounded to fp32 (the least an
    fp32 accumulator can do).  The hardware lies between the two; in the sparse forward / data-gradient models an MFMA holds about one non-zero
    product, so the two coincide there"""
    x, z = np.asarray(x_rows, np.float32), np.asarray(dz_rows, np.float32)
    if arith == "bf16x3":
        xp, zp, terms, back = R.b3_planes(x), R.b3_planes(z), R.B3_TERMS, 0
    else:
        ez = _tensor_exp(z, 8192.0)
        xp, zp, terms, back = R.h2_planes(x), R.h2_planes(np.ldexp(z, ez)), R.H2_TERMS, -ez
    xp, zp = [p.astype(np.float64) for p in xp], [p.astype(np.float64) for p in zp]
    noct = (B + 7) // 8
    per = -(-noct // msplit)
    slabs = [np.zeros((x.shape[1], z.shape[1]), np.float32) for _ in range(msplit)]
    for oct_, rows in wgrad_groups(B, hout):
        s = oct_ // per
        for (i, j) in terms:
            if (i, j) != drop:
                if inner == "exact":
                    slabs[s] = (slabs[s].astype(np.float64) + xp[i - 1][rows].T @ zp[j - 1][rows]).astype(np.float32)
                else:
                    for r in rows:
                        slabs[s] = (slabs[s].astype(np.float64) + np.outer(xp[i - 1][r], zp[j - 1][r])).astype(np.float32)
    if msplit == 1:
        acc = slabs[0]
    else:
        acc = np.zeros_like(slabs[0])
        for s in slabs:
            acc = acc + s
    return np.ldexp(acc, back).astype(np.float32)
