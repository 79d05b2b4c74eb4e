"""Per-layer reference and yardstick of the network forward -- TEST INFRASTRUCTURE ONLY (CPU, NumPy).

One GEMM layer of oracle/nn_numpy.py at a time: `layer64` evaluates conv2 .. fc2 in float64 from the GPU's OWN output of the previous layer (read
through NNetWrapper.activation), so that every kernel is judged on its own -- upstream rounding and ReLU flips do not enter.

Statistic of a layer:   err = max over the sampled rows and all channels of |gpu - relu(z64)| / norm_c,   norm_c = max over the sampled rows of
|z64[:, c]| (the BN output BEFORE the ReLU: never zero).  Yardstick: E32 = the same statistic for the same layer evaluated on the host in NumPy
float32 from the same input -- what fp32 arithmetic itself loses on this layer and these rows; it depends on the reference alone.

Margins (a healthy kernel stays at or below margin x E32).  They come from NumPy models of the two split arithmetics (model_b3, model_h2 below),
evaluated by tests/test_layer_parity_cpu.py on every run, never from what a kernel gives:
  E32 2.2e-7 .. 3.4e-7 on the five shapes of that test
  bf16x3, complete six-term product 1.2 .. 1.6 x E32, any single kept term removed >= 24 x E32   -> MARGIN_B3 = MARGIN_F32 = 6
  f16x2, complete three-term product 2.8 .. 3.5 x E32, any single term removed >= 1500 x E32      -> MARGIN_H2 = 16
  (at the five shapes of 384 / 768 / 1024 filters added later, K = 3072 .. 12288, still 8 terms a column: E32 2.3e-7 .. 2.7e-7, bf16x3 complete
   1.3 .. 2.2 x, weakest term removed >= 25 x; f16x2 complete 3.2 .. 4.0 x, weakest >= 1900 x -- the same margins hold)
(a margin is a few times the modelled healthy value and at least four times below the weakest single-term defect; the exact-fp32 kernels are
held to the bf16x3 margin: bf16x3 claims fp32's accuracy)
Few-row samples.  norm_c is the SCALE of channel c; taken over one row (a dense layer of a one-board call) it is |z64| of that single element, the
statistic becomes the largest RELATIVE error of an element, and an element near zero -- the k-sum cancelling the BN shift -- has an unbounded
relative error in any fp32-class arithmetic: the complete f16x2 model then reaches 650 x E32 on some rows and the complete bf16x3 model 39 x, above
what a lost term costs on others (test_layer_parity_cpu.py::test_one_row_samples_need_the_norm_of_many_rows asserts it), and E32 itself, a single
element's float32 error, moves with the host's BLAS.  So the GPU test takes norm_c over the sampled rows of ALL the calls a case makes on a network
(full capacity first, small networks several times on fresh boards): for the full-capacity call that is the sample's own norm up to the other
calls' rows; every output of every sampled row is still compared, against the same margins, and a single row under the norm of many separates
again (complete <= 3.4 / 8.2 x E32, any term removed >= 11 / 1000 x E32 for bf16x3 / f16x2).
On the SPARSE network: exactly 8 non-zero kernel entries per output column, so that the fp32 accumulation noise of a K = 2304 .. 8192 dot product
nearly vanishes and what is left is the accuracy of the products.  On dense weights a lost bf16x3 term separates by 2.5 x only: the dense network is
the realistic data (and what f16x2's placement depends on), bound MARGIN_DENSE = 16 in every precision.
"""
import numpy as np

from oracle import nn_numpy
from othellozero_amd.weights import init_weights

MARGIN_F32 = 6.0
MARGIN_B3 = 6.0
MARGIN_H2 = 16.0
MARGIN_DENSE = 16.0
MARGIN = {"f32": MARGIN_F32, "bf16x3": MARGIN_B3, "f16x2": MARGIN_H2}
SPARSE_NNZ = 8
KERNELS = (6, 12, 18, 24, 30)          # conv2, conv3, conv4, fc1, fc2 kernels in get_weights() order (layer l = 1 .. 5 -> KERNELS[l - 1])


# ------------------------------------------------------------------ networks
def sparse_columns(kernel, rs, nnz=SPARSE_NNZ):
    """`kernel` (any shape, output channels last) with exactly `nnz` entries kept per output column, at random k; kept entries that are exactly zero
    (never, for a continuous draw) would break the count, so they are asserted against"""
    w = np.asarray(kernel)
    flat = w.reshape(-1, w.shape[-1])
    K, N = flat.shape
    keep = np.zeros((K, N), bool)
    for c in range(N):
        keep[rs.choice(K, nnz, replace=False), c] = True
    # the kept entries are scaled by sqrt(K / nnz): the layer's pre-activations keep the variance they have in the dense network, so that the k-sum
    # (the part a lost product term damages) and not the BN shift dominates norm_c, and the activations downstream stay in the dense network's range
    out = (np.where(keep, flat, np.float32(0)) * np.float32(np.sqrt(K / nnz))).astype(np.float32)
    assert np.all((out != 0).sum(axis=0) == nnz)
    return out.reshape(w.shape)


def _biregular(rows, cols, per_row, per_col, rs):
    """a random 0/1 pattern (rows, cols) with exactly per_row ones in every row and per_col in every column: the row stubs against a random
    permutation of the column stubs, a stub pair that repeats an earlier (row, col) re-dealt by swapping its column with a random other stub's"""
    assert rows * per_row == cols * per_col and per_row <= cols and per_col <= rows, \
        f"no biregular pattern for a kernel of shape ({rows}, {cols}): {per_row} entries a row are {rows * per_row / cols:g} a column"
    r = np.repeat(np.arange(rows), per_row)
    c = rs.permutation(np.repeat(np.arange(cols), per_col))
    for _ in range(1000):
        key = r * cols + c
        _, first = np.unique(key, return_index=True)
        dup = np.setdiff1d(np.arange(key.size), first)
        if dup.size == 0:
            break
        for i in dup:
            j = rs.randint(key.size)
            c[i], c[j] = c[j], c[i]
    keep = np.zeros((rows, cols), bool)
    keep[r, c] = True
    assert np.all(keep.sum(axis=1) == per_row) and np.all(keep.sum(axis=0) == per_col)
    return keep


def dense_per_row(K, N, nnz=SPARSE_NNZ):
    """entries per input row of a bisparse dense kernel (K, N): max(2, N nnz / K), lowered (never below 2) until the entries per column, per_row K / N,
    are whole -- fc1 of 6x6 at 384 filters, (1536, 1024): 5 a row would be 7.5 a column, 4 a row are 6.  Every kernel whose first value is whole keeps it"""
    per_row = max(2, N * nnz // K)
    while per_row > 2 and per_row * K % N:
        per_row -= 1
    return per_row


def bisparse_kernel(kernel, rs, nnz=SPARSE_NNZ):
    """`kernel` thinned in BOTH directions, so that the forward sum (over k, for an output column) and the data-gradient sum (over (tap, co), for
    an input channel) are both short.  3x3 kernels (3, 3, Cin, Co): exactly nnz entries per output channel and exactly nnz per input channel, each
    at a random tap (the (ci, co) pairs are a biregular pattern, so no position repeats).  Dense kernels (K, N): exactly `per_row` = dense_per_row(K, N)
    = max(2, N nnz / K) entries per input row and per_row K / N per output column (= nnz wherever N nnz / K >= 2 and divides).  Kept entries are scaled by sqrt(K / entries per
    column), as sparse_columns does"""
    w = np.asarray(kernel)
    if w.ndim == 4:
        _, _, ci, co = w.shape
        pair = _biregular(ci, co, nnz * co // ci, nnz, rs)
        i, o = np.nonzero(pair)
        keep = np.zeros(w.shape, bool)
        keep[rs.randint(3, size=i.size), rs.randint(3, size=i.size), i, o] = True
        K, per_col = 9 * ci, nnz
    else:
        K, N = w.shape
        per_row = dense_per_row(K, N, nnz)
        per_col = per_row * K // N
        keep = _biregular(K, N, per_row, per_col, rs)
    out = (np.where(keep, w, np.float32(0)) * np.float32(np.sqrt(K / per_col))).astype(np.float32)
    assert np.count_nonzero(out) == np.count_nonzero(keep)
    return out


_weights_cache = {}


def network_weights(n, channels, kind):
    """the two test networks, built once per (board, filters, kind) and never modified: 'dense' = init_weights(randomize_all=True) as the existing
    tests use it; 'sparse' = the same draw with the kernels of conv2, conv3, conv4, fc1 and fc2 thinned to SPARSE_NNZ entries per output column
    and scaled by sqrt(K / SPARSE_NNZ) (sparse_columns); 'bisparse' = the same draw thinned per output column AND per input channel / row
    (bisparse_kernel: the trainer's data gradient contracts over the output channels); biases and all four BN arrays stay random"""
    key = (n, channels, kind)
    if key not in _weights_cache:
        w = init_weights(n, seed=1000 + n + channels, channels=channels, randomize_all=True)
        if kind == "sparse":
            rs = np.random.RandomState(77 + n + channels)
            for i in KERNELS:
                w[i] = sparse_columns(w[i], rs)
        elif kind == "bisparse":
            rs = np.random.RandomState(4177 + n + channels)
            for i in KERNELS:
                w[i] = bisparse_kernel(w[i], rs)
        else:
            assert kind == "dense", kind
        for a in w:
            a.setflags(write=False)
        _weights_cache[key] = w
    return _weights_cache[key]


# ------------------------------------------------------------------ one layer
def layer_geometry(n, channels, layer):
    """(input side, output side, 'same' padding, taps, K, N) of layer 1 .. 5 = conv2, conv3, conv4, fc1, fc2"""
    C = channels
    return {1: (n, n, True, 9, 9 * C, C), 2: (n, n - 2, False, 9, 9 * C, C), 3: (n - 2, n - 4, False, 9, 9 * C, C),
            4: (1, 1, False, 1, (n - 4) ** 2 * C, 1024), 5: (1, 1, False, 1, 1024, 512)}[layer]


def layer_z(weights, layer, x_in, dtype=np.float64):
    """BN output BEFORE the ReLU of layer 1 .. 5 (conv2 .. fc2) for the input x_in -- conv layers (boards, H, W, C), dense layers (boards, K) with fc1's
    K in (h, w, c) order -- evaluated in `dtype` with nn_numpy's own convolution and BN (moving statistics)"""
    k, bias, g, b, mu, var = (np.asarray(a, dtype=dtype) for a in weights[6 * layer:6 * layer + 6])
    x = np.asarray(x_in, dtype=dtype)
    if layer <= 3:
        y = nn_numpy._conv3x3(x, k, bias, same=(layer == 1))
        y = y.reshape(-1, y.shape[-1])
    else:
        y = x.reshape(x.shape[0], -1) @ k + bias
    z = nn_numpy._bn(y, g, b, mu, var)
    assert z.dtype == dtype
    return z


def layer64(weights, layer, x_in):
    return layer_z(weights, layer, x_in, np.float64)


def conv1_out(weights, own, opp, n, dtype):
    """relu(BN(conv1)) of the boards as (boards, n, n, C) in `dtype` (the table modes never materialise it: the reference of conv2 starts here)"""
    w = [np.asarray(a, dtype=dtype) for a in weights[:6]]
    x = nn_numpy.planes(own, opp, n, dtype)
    if w[0].shape[2] == 1:
        x = x[..., 0:1] - x[..., 1:2]
    return np.maximum(nn_numpy._bn(nn_numpy._conv3x3(x, w[0], w[1], True), *w[2:6]), 0)


def channel_norm(z64):
    """norm_c = max over the rows of |z64[:, c]|"""
    return np.abs(np.asarray(z64, np.float64)).max(axis=0)


def statistic(out, z64, norm=None):
    """max |out - relu(z64)| / norm_c over all rows and channels; norm_c = max over the rows of |z64[:, c]|, or `norm` = that maximum over a
    larger sample of rows of the same layer of the same network which includes these (see the module docstring: few-row samples)"""
    z64 = np.asarray(z64, np.float64)
    if norm is None:
        norm = channel_norm(z64)
    assert np.all(norm > 0) and np.all(norm >= channel_norm(z64))
    return float((np.abs(np.asarray(out, np.float64) - np.maximum(z64, 0)) / norm).max())


def e32(weights, layer, x_in, z64):
    """the yardstick: the statistic of the layer evaluated in NumPy float32 from the same input"""
    return statistic(np.maximum(layer_z(weights, layer, x_in, np.float32), 0), z64)


def sample_runs(count, pixels):
    """the sampled boards of a call of `count` boards for a layer of `pixels` output pixels per board: three runs of ceil(256 / pixels) + 1 consecutive
    boards at the start, in the middle and at the very end of the call -- every row position inside a 256-row tile and the partly filled last tile --
    as a sorted list of disjoint (first board, boards) intervals"""
    nb = min(count, -(-256 // pixels) + 1)
    starts = sorted({0, max(0, (count - nb) // 2), count - nb})
    runs = []
    for s in starts:
        if runs and s <= runs[-1][0] + runs[-1][1]:
            runs[-1] = (runs[-1][0], max(runs[-1][1], s + nb - runs[-1][0]))
        else:
            runs.append((s, nb))
    return runs


# ------------------------------------------------------------------ NumPy models of the split arithmetics (CPU test only)
def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def b3_planes(x):
    x = np.asarray(x, np.float32)
    b1 = bf16_round(x)
    r1 = x - b1
    b2 = bf16_round(r1)
    b3 = bf16_round(r1 - b2)
    return b1, b2, b3


def h2_planes(x):
    x = np.asarray(x, np.float32)
    h1 = x.astype(np.float16).astype(np.float32)
    return h1, (x - h1).astype(np.float16).astype(np.float32)


def _sparse_table(kernel):
    """per output column the k indices (ascending) and values of its SPARSE_NNZ entries: (idx (nnz, N), val (nnz, N))"""
    flat = np.asarray(kernel, np.float32).reshape(-1, kernel.shape[-1])
    idx = np.stack([np.flatnonzero(flat[:, c]) for c in range(flat.shape[1])], axis=1)
    assert idx.shape[0] == SPARSE_NNZ
    return idx, np.take_along_axis(flat, idx, axis=0)


def _accumulate(idx, prods):
    """fp32 accumulator of one output tile the way the 16-bit matrix cores build it: k-tile by k-tile (32 wide), inside a k-tile one MFMA per plane
    product in the given order, each adding its exact products of that k-tile to the fp32 accumulator.  prods: list (in issue order) of arrays
    (nnz, rows, N) = the products of a column's entries, float64 (a 16-bit x 16-bit product is exact in it)"""
    nnz, rows, N = prods[0].shape
    tile = idx // 32
    group = np.concatenate([np.zeros((1, N), int), np.cumsum(tile[1:] != tile[:-1], axis=0)], axis=0)     # rank of an entry's k-tile inside its column
    acc = np.zeros((rows, N), np.float32)
    for g in range(nnz):
        for p in prods:
            s = np.zeros((rows, N))
            for j in range(nnz):
                s += np.where(group[j] == g, p[j], 0.0)
            acc = (acc.astype(np.float64) + s).astype(np.float32)
    return acc


def _fold(weights, layer):
    """the folded BN scale / shift of oz_net_commit: float64, rounded to fp32"""
    bias, g, b, mu, var = (np.asarray(a, np.float64) for a in weights[6 * layer + 1:6 * layer + 6])
    s = g / np.sqrt(var + nn_numpy.BN_EPS)
    return s.astype(np.float32), ((bias - mu) * s + b).astype(np.float32)


def _fma32(a, sc, sh):
    return (np.asarray(a, np.float64) * np.asarray(sc, np.float64) + np.asarray(sh, np.float64)).astype(np.float32)


B3_TERMS = ((3, 1), (1, 3), (2, 2), (2, 1), (1, 2), (1, 1))       # (plane of a, plane of b): the six kept cross terms, small terms first
H2_TERMS = ((2, 1), (1, 2), (1, 1))


def model_b3(weights, layer, a, drop=None):
    """relu(BN) of a sparse layer on rows `a` (rows, K) fp32 in the bf16x3 arithmetic: x = b1 + b2 + b3, the kept cross terms (B3_TERMS without `drop`)
    accumulated in fp32 per 32-wide k-tile, small terms first, then fmaf(acc, scale, shift) and the ReLU"""
    idx, val = _sparse_table(weights[KERNELS[layer - 1]])
    ap, wp = b3_planes(a), b3_planes(val)
    prods = [ap[i - 1][:, idx].transpose(1, 0, 2).astype(np.float64) * wp[j - 1][:, None, :].astype(np.float64) for (i, j) in B3_TERMS if (i, j) != drop]
    sc, sh = _fold(weights, layer)
    return np.maximum(_fma32(_accumulate(idx, prods), sc, sh), 0)


def _pow2_exponents(mx, top=-2):
    """exponents e with mx * 2^e in [2^(top - 1), 2^top) (pick_exponents of oz_net_commit)"""
    _, ex = np.frexp(np.asarray(mx, np.float64))
    return top - ex


def model_h2(weights, layer, a, chan_of_k, drop=None):
    """the same layer in the f16x2 arithmetic: every input channel moved by an exact power of two so that its largest value over the rows lands in
    [2^-3, 2^-2), the power divided out of the weight rows, every weight column moved into [2^-3, 2^-2) likewise; both operands split into two fp16
    planes, the kept terms of a1 w1 + a1 w2 + a2 w1 (H2_TERMS without `drop`) accumulated in fp32 per k-tile, small terms first; the column's power folded into the BN scale"""
    idx, val = _sparse_table(weights[KERNELS[layer - 1]])
    a = np.asarray(a, np.float32)
    nchan = int(chan_of_k.max()) + 1
    cmax = np.zeros(nchan)
    np.maximum.at(cmax, chan_of_k, np.abs(a).max(axis=0))
    cmax[cmax == 0] = np.median(cmax[cmax > 0])
    aexp = _pow2_exponents(cmax)[chan_of_k]                                   # per k
    a_s = np.ldexp(a, aexp[None, :]).astype(np.float32)
    w_s = np.ldexp(val, -aexp[idx]).astype(np.float32)
    wexp = _pow2_exponents(np.abs(w_s).max(axis=0))
    w_s = np.ldexp(w_s, wexp[None, :]).astype(np.float32)
    ap, wp = h2_planes(a_s), h2_planes(w_s)
    prods = [ap[i - 1][:, idx].transpose(1, 0, 2).astype(np.float64) * wp[j - 1][:, None, :].astype(np.float64) for (i, j) in H2_TERMS if (i, j) != drop]
    sc, sh = _fold(weights, layer)
    sc = np.ldexp(sc, -wexp).astype(np.float32)
    return np.maximum(_fma32(_accumulate(idx, prods), sc, sh), 0)
