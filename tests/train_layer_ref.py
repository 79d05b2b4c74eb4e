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
all of them; every element of every step is still compared.
The launchers' choice of row tile and k-split for a trainer GEMM is restated below (tile_rule, trainer_kslices, tile_plan), so that the batch sizes
which reach the 192 / 256-row tiles are asserted on the CPU and a moved threshold shows without a device; the GPU matrix compares it with Trainer.plan."""
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


# ------------------------------------------------------------------ the launchers' tile rule (oz_gemm_h2_launch, oz_gemm_b3_launch), restated
B3_BIG_ROUND_COST = 0.93               # oz_net.hip: a round of 256 x 256 tiles against two rounds of 128 x 256 tiles
BIG_GRID_BLOCKS = 192                  # the 256-row tiles' grid must have at least this many blocks (of the chip's 256 CUs)


def tile_cost(rows, N, bm):
    """oz_net.hip's tile_cost: rounds of the 256 CUs x tile height that a grid of bm-row tiles (256 columns each) pays for rows x N outputs"""
    return -(-(-(-rows // bm) * (N // 256)) // 256) * bm


def tile_rule(arith, rows, N, pad):
    """'low' / 'mid' / 'big': the row tile (128 / 192 / 256 rows) of a trainer GEMM of `rows` x N outputs -- rows = the launch's boards (f16x2: the
    call's, bf16x3: the trainer's capacity) x output pixels; pad: 1 for a 'same' layer.  f16x2 (oz_gemm_h2_launch): the ping-pong tiles once
    ceil(rows / 256) x (N / 256) >= 192, of the two the one whose grid pays fewer tile-rows (H2MidPP only if strictly fewer).  bf16x3
    (oz_gemm_b3_launch: b3_big_rows(rows, N, false)): the 256-row tile for a 'valid' layer with that many blocks whose grid costs, at
    B3_BIG_ROUND_COST, no more than the 128-row tiles'; there is no mid tile"""
    big = -(-rows // 256) * (N // 256) >= BIG_GRID_BLOCKS
    if arith == "f16x2":
        return "low" if not big else "mid" if tile_cost(rows, N, 192) < tile_cost(rows, N, 256) else "big"
    assert arith == "bf16x3"
    return "big" if pad == 0 and big and B3_BIG_ROUND_COST * tile_cost(rows, N, 256) <= tile_cost(rows, N, 128) else "low"


TILE_KERNEL = {("f16x2", "low"): "h2_lowpp", ("f16x2", "mid"): "h2_midpp", ("f16x2", "big"): "h2_bigpp", ("bf16x3", "low"): "b3", ("bf16x3", "big"): "b3_big"}
UNSPLIT_KERNELS = ("h2_midpp", "h2_bigpp", "b3_big")        # one k-slice; h2_lowpp / b3 always split the k loop in the trainer


PARTIAL_FLOATS = 40 << 20              # oz_train.hip: the trainer's split-K buffer (gpartial_floats)


def trainer_kslices(arith, rows, N, K, pad):
    """the k-slices of that launch: 1 on the mid / big tiles; on the 128-row tile oz_net.hip's trainer_ksplit -- the largest split <= 16 that keeps
    the grid within one round of the 256 CUs, at least 8 k-tiles of 32 per slice, the slabs within the buffer.  So a 128-row launch of more than
    128 blocks (more than 8192 rows at 512 filters) is not split either"""
    if tile_rule(arith, rows, N, pad) != "low":
        return 1
    blocks, nk, ksplit = -(-rows // 128) * (N // 256), K // 32, 1
    while ksplit < 16 and blocks * (ksplit + 1) <= 256 and nk // (ksplit + 1) >= 8 and (ksplit + 1) * rows * N <= PARTIAL_FLOATS:
        ksplit += 1
    return ksplit


def tile_plan(arith, n, C, B):
    """{layer 1 .. 3: dict(fwd_kernel, fwd_kslices, dgrad_kernel, dgrad_kslices)} of a launch of B boards as tile_rule / trainer_kslices have it:
    the forward's rows are B x Hout^2, the data gradient's B x Hin^2 (its output is the layer's input; 'same' exactly where the layer is)"""
    out = {}
    for l in (1, 2, 3):
        g = geometry(n, C, l)
        pad = int(g["same"])
        fwd, dg = (B * g["Hout"] ** 2, g["Co"], pad), (B * g["Hin"] ** 2, g["Cin"], pad)
        out[l] = dict(fwd_kernel=TILE_KERNEL[arith, tile_rule(arith, *fwd)], fwd_kslices=trainer_kslices(arith, fwd[0], fwd[1], 9 * g["Cin"], pad),
                      dgrad_kernel=TILE_KERNEL[arith, tile_rule(arith, *dg)], dgrad_kslices=trainer_kslices(arith, dg[0], dg[1], 9 * g["Co"], pad))
    return out


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


WGRAD_CI_STRIDE = 16                   # the sampled weight gradient: every 16th input channel -- one or more in every 32- and 64-wide input-channel tile


def sampled_ci(a, axis):
    """every WGRAD_CI_STRIDE-th input channel of an activation (axis 3) or of a 3x3 weight gradient (axis 2), as a copy.  The sampled weight-gradient
    reference of a 3x3 layer is wgrad(layer, sampled_ci(x, 3), dz, dtype) against sampled_ci(device's dW, 2): all nine taps, all output columns and
    ALL rows -- every element is a sum over every (board, pixel) of the step, so rows, octets and slabs that go missing show as in the whole
    tensor; norm_c over the sampled (tap, ci) is at most the whole tensor's, so the statistic is no looser"""
    return np.ascontiguousarray(a[(slice(None),) * axis + (slice(None, None, WGRAD_CI_STRIDE),)])


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


def model_wgrad(x_rows, dz_rows, B, hout, arith, msplit=1, drop=None, inner="exact", drop_octet=None, drop_slab=None):
    """one tap of the octet weight gradient on x_rows (B hout^2, Ci), dz_rows (B hout^2, Co): per k-step (wgrad_groups) one MFMA per kept plane
    product, in mac()'s order (small terms first: R.B3_TERMS / R.H2_TERMS read as (plane of x, plane of dz)), each adding its exact products to the
    fp32 accumulator; octets split over `msplit` slabs that are summed in fp32 in slab order (k_t_sum_partials).  f16x2: dz moved by the power of
    two that brings the tensor's maximum to 8192 (k_t_z_octets), x unscaled (post-ReLU values), the power taken back in the epilogue.
    inner: how one MFMA adds its (up to) 32 products to the accumulator, which the instruction set does not specify -- "exact": their exact sum,
    rounded to fp32 once (the most a 16-bit matrix core can do); "sequential": one by one in k order, each sum rounded to fp32 (the least an
    fp32 accumulator can do).  The hardware lies between the two; in the sparse forward / data-gradient models an MFMA holds about one non-zero
    product, so the two coincide there.
    drop_octet / drop_slab: a model that loses the k-steps of that octet of 8 boards / never adds that slab of the split (defects of the row
    bookkeeping, not of the arithmetic: what the coarse bound of a long sum can still see)"""
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
        if oct_ == drop_octet:
            continue
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
        for k, s in enumerate(slabs):
            if k != drop_slab:
                acc = acc + s
    return np.ldexp(acc, back).astype(np.float32)
