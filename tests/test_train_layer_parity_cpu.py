"""The margins of the trainer's per-kernel parity tests (tests/test_gpu_train_layer_parity.py) can detect a defect: shown on the CPU with NumPy
models of the two split arithmetics on the trainer's own contractions (tests/train_layer_ref.py: model_dgrad, model_wgrad) -- never by breaking a
kernel on the GPU, and never from what a kernel returns.

Evaluated on every run, relative to E32 (NumPy float32 on the same inputs): the complete arithmetic, and the arithmetic with each single kept term
removed.  The rule (layer_ref): a SHARP margin is a few times the modelled healthy ratio (here: at least twice it) and at least four times below
the weakest single-term defect.  A shape that cannot separate by that factor is COARSE (bound MARGIN_DENSE = 16 of the forward work); the tests
print the class of every shape and assert that every shape train_layer_ref declares sharp separates.

What the models printed when the constants of train_layer_ref were written (one line per shape is printed again on every run, pytest -s):
  data gradient, bisparse 3x3 layers (8 entries per input channel over taps x co), 96 rows, four shapes
      bf16x3  complete 2.1 .. 3.0 x E32   weakest single term removed 35 x E32    -> MARGIN_DGRAD 8  (= floor(35 / 4); 2.7 x the healthy maximum)
      f16x2   complete 1.8 .. 2.8 x E32   weakest single term removed 2670 x E32  -> MARGIN_DGRAD 16 (the f16x2 margin of the forward work)
  weight gradient
      bf16x3, the real rows of an oracle step (float64 autograd, bisparse network, 256 filters, half of x zero), all nine taps, all 256 x 256 channels.
      How one MFMA adds its 32 products is not specified, so the healthy ratio is bracketed: one rounding per MFMA / one rounding per product.
          conv4, 8 .. 36 rows (6x6 at 2, 5, 8, 9 boards, 8x8 at 2): complete 0.63 .. 1.67 / 1.08 .. 2.07, weakest term removed 18.9 .. 33.3
              -> sharp, MARGIN_WGRAD 4.5 (>= 2 x 2.07, <= 18.9 / 4)
          conv3 and conv2, 32 .. 144 rows: complete 0.5 .. 1.0 / 1.4 .. 1.9, weakest 9.5 .. 19.1: below 4 x 4.5 at 72 rows and more (E32 grows with the
              length of the sum, the lost term does not), 19.1 and 18.3 at 32 and 80 rows of conv3 of 6x6 -- a twentieth above the limit; these stay
              coarse, so that the sharp class is one statement (conv4, at most 36 rows) and not a list of lucky shapes
      f16x2 (k_wgrad_h2 runs from 32 boards on), synthetic rows, one tap, 64 x 64 channels, 128 .. 4096 rows: complete 0.26 .. 0.61 / 0.75 .. 1.83,
          weakest 489 -> sharp, MARGIN_WGRAD 6
  The exact-fp32 kernels have no term to lose; they are held to bf16x3's margins on the same shapes (bf16x3 claims fp32's accuracy).
What changed in the model, and why: its first form evaluated one tap of 64 x 64 channels on synthetic draws and let an MFMA add the exact sum of its
32 products with one rounding; it put the healthy bf16x3 weight gradient at 0.5 .. 0.9 x E32 and the margin at 3.  The first run on the device
returned 1.2 .. 2.3 for the healthy kernel, within 1.3 x of that margin: the model was wrong, not the kernel (the exact-fp32 kernel returned 1.00 on the
same shapes).  The real rows and the full tensor move the one-rounding figure little (0.6 .. 1.7); what the first form left out is that a dense
k-step holds 32 non-zero products whose summation inside the instruction is unspecified -- in the sparse forward and data-gradient models a k-step
holds about one, and nothing is left out there.  The second bracket (every product rounded into the fp32 accumulator on its own: the least exact an
fp32 accumulator can be) gives 1.1 .. 2.1, and the margin is now taken from it.
So the issue's expectation that a weight gradient over 72 .. 512 rows separates a lost bf16x3 term does not hold under this yardstick: such a term
costs 9 .. 17 x E32 there, inside the coarse bound.
The chip-filling tiles (the GPU matrix's `chip` cases, 383 boards and more at 8x8 / 512 filters): the launchers' tile and k-split rule is restated
in train_layer_ref (tile_rule, trainer_kslices) and every case's batch is shown here to reach the kernels it names, 64 boards fewer not to.  Their
weight gradients sum 6000 .. 100 000 rows; the coarse bound cannot see a lost plane product there.  What it does see is lost ROWS: on conv3 at 383
boards (13788 rows, a block of 32 x 64 channels) the complete models give 1.7 (bf16x3) and 1.2 (f16x2) x E32, one octet of boards skipped 4 x 10^5,
one slab of the octet split never added 9 x 10^5 and more."""
import numpy as np
import pytest

import layer_ref as R
import train_layer_ref as T

ROWS = 96
DGRAD_SHAPES = [(8, 256, 1), (8, 256, 2), (6, 256, 3), (6, 512, 2)]                       # (board, filters, layer)
DGRAD_SHAPES += [(8, 384, 1), (8, 768, 2), (6, 1024, 3)]                                  # the widths of the GPU matrix's WIDTH_CASES: K' = 3456, 6912, 9216
TERMS = {"bf16x3": R.B3_TERMS, "f16x2": R.H2_TERMS}
WGRAD_TILES = {"bf16x3": 16, "f16x2": 8}                                                 # (Cin / CI) x (Co / CO) at 256 filters: decides the octet split


def _stat(out, ref):
    return T.statistic(out, ref)[0]


# ------------------------------------------------------------------ networks
@pytest.mark.parametrize("n,C", [(8, 128), (6, 128), (8, 256), (6, 256), (6, 512), (6, 384), (8, 384), (8, 768), (6, 768), (6, 1024)])
def test_bisparse_counts(n, C):
    w = R.network_weights(n, C, "bisparse")
    dense = R.network_weights(n, C, "dense")
    for layer in (1, 2, 3):
        keep = np.asarray(w[6 * layer]) != 0
        assert np.all(keep.sum(axis=(0, 1, 2)) == R.SPARSE_NNZ), layer                   # per output channel, over taps x ci
        assert np.all(keep.sum(axis=(0, 1, 3)) == R.SPARSE_NNZ), layer                   # per input channel, over taps x co
    for layer in (4, 5):
        keep = np.asarray(w[6 * layer]) != 0
        K, N = keep.shape
        per_row = max(2, N * R.SPARSE_NNZ // K)
        if (K, N) == (1536, 1024):                                                        # fc1 of 6x6 at 384 filters: 5 a row would be 7.5 a column
            per_row = 4
        assert per_row * K % N == 0 and R.dense_per_row(K, N) == per_row
        assert np.all(keep.sum(axis=1) == per_row) and np.all(keep.sum(axis=0) == per_row * K // N), layer
        # a column holds the 8 entries of the convolutions wherever 8 N / K is whole and at least 2 (else: 2 a row, or the whole number below 8 N / K)
        assert per_row * K // N == R.SPARSE_NNZ or N * R.SPARSE_NNZ // K < 2 or (N * R.SPARSE_NNZ) % K, (K, N)
    for i in range(40):                                                                   # everything else is the dense network's own draw
        if i not in R.KERNELS:
            assert np.array_equal(w[i], dense[i])


def test_biregular_refusal_names_the_shape():
    """every accepted width thins (fc1 of 6x6 at 384 filters, (1536, 1024), by lowering 5 entries a row to 4: dense_per_row); a pattern that cannot exist
    is refused with its shape, not with a bare assertion"""
    assert R.dense_per_row(1536, 1024) == 4 and R.dense_per_row(4096, 1024) == 2 and R.dense_per_row(1024, 512) == 4 and R.dense_per_row(6144, 1024) == 2
    for C in range(128, 2049, 128):
        for K in (4 * C, 16 * C):
            assert R.dense_per_row(K, 1024) * K % 1024 == 0 and R.dense_per_row(K, 1024) >= 2, (C, K)
    with pytest.raises(AssertionError, match=r"shape \(3, 2\)"):
        R._biregular(3, 2, 1, 1, np.random.RandomState(0))


def test_sparse_and_dense_networks_are_unchanged():
    """'sparse' and 'dense' are what the merged forward tests were measured on: the same draws, whether or not a bisparse network was built first"""
    import zlib
    from othellozero_amd.weights import init_weights
    R.network_weights(6, 256, "bisparse")
    dense, sparse = R.network_weights(6, 256, "dense"), R.network_weights(6, 256, "sparse")
    plain = init_weights(6, seed=1000 + 6 + 256, channels=256, randomize_all=True)
    rs = np.random.RandomState(77 + 6 + 256)
    for i in range(40):
        assert np.array_equal(dense[i], plain[i])
        want = R.sparse_columns(plain[i], rs) if i in R.KERNELS else plain[i]
        assert np.array_equal(sparse[i], want), i
    # a fingerprint of the bytes, recorded when this test was written (the merged forward margins rest on these very numbers)
    crc = lambda w: zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in w))
    assert (crc(dense), crc(sparse)) == (0x69b59c0e, 0xac96fdd9)


# ------------------------------------------------------------------ data gradient
_dgrad_cache = {}


def _dgrad_case(n, C, layer):
    key = (n, C, layer)
    if key not in _dgrad_cache:
        k = np.asarray(R.network_weights(n, C, "bisparse")[6 * layer])
        idx, val, KP = T.dgrad_table(k)
        assert idx.shape == (R.SPARSE_NNZ, C) and np.all(np.diff(idx, axis=0) > 0)
        a = T.dz_like(np.random.RandomState(5 + layer + C), ROWS, KP)
        Wd = np.zeros((KP, C), np.float32)
        Wd[idx, np.arange(C)[None, :]] = val
        ref = a.astype(np.float64) @ Wd.astype(np.float64)
        _dgrad_cache[key] = (k, a, ref, _stat(a @ Wd, ref))
    return _dgrad_cache[key]


def test_dgrad_table_is_the_transposed_contraction():
    """the model's operand against the plain definition: one pixel whose nine taps are inside, dX[ci] = sum over (t, co) of dz[shifted by t][co] W[t][ci][co]"""
    k, a, ref, _ = _dgrad_case(6, 256, 3)
    C = k.shape[2]
    rows = a[:4].astype(np.float64).reshape(4, C // 32, 9, 32)               # k' = (slice * 9 + (8 - t)) * 32 + c32
    want = np.zeros((4, C))
    for t in range(9):
        want += rows[:, :, 8 - t, :].reshape(4, C) @ k.reshape(9, C, C)[t].astype(np.float64).T
    assert np.allclose(ref[:4], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("n,C,layer", DGRAD_SHAPES)
def test_dgrad_margin_separates_every_single_term_defect(n, C, layer, arith):
    k, a, ref, E32 = _dgrad_case(n, C, layer)
    margin = T.MARGIN_DGRAD[arith]
    full = _stat(T.model_dgrad(k, a, arith), ref) / E32
    drops = {t: _stat(T.model_dgrad(k, a, arith, drop=t), ref) / E32 for t in TERMS[arith]}
    print(f"dgrad {arith:6s} n={n} C={C} layer={layer}: E32 {E32:.3g}  complete {full:.2f}  weakest term removed {min(drops.values()):.1f}  "
          f"({', '.join(f'a{i}w{j} {v:.3g}' for (i, j), v in drops.items())})  -> sharp, margin {margin:g}")
    assert 2 * full <= margin
    assert min(drops.values()) >= 4 * margin
    assert T.MARGIN_DGRAD["f32"] == T.MARGIN_DGRAD["bf16x3"]


# ------------------------------------------------------------------ weight gradient
# bf16x3 / f32: the REAL rows of a step -- a[l - 1] and dz[l] of the float64 oracle (oracle/train_ref.py) on the bisparse network at 256 filters, the batches
# of the GPU matrix, rounded to fp32 -- the whole tensor: all nine taps, all 256 x 256 channels, max over all of it as the GPU test takes it.
_step_cache = {}


def _oracle_step(n, B, C=256):
    """(a[0 .. 3], dz[0 .. 5]) of one oracle step on the bisparse network, as fp32"""
    if (n, B, C) not in _step_cache:
        from oracle.train_ref import TrainRef

        class Tap(TrainRef):
            def _bn_train(self, z, blk, fused):
                z.retain_grad()
                self.zs.append(z)
                return super()._bn_train(z, blk, fused)

            def _relu(self, y, layer):
                r = super()._relu(y, layer)
                self.acts.append(r.detach().numpy().astype(np.float32))
                return r
        t = Tap(R.network_weights(n, C, "bisparse"), n, dropout=0.3, seed=77)
        t.zs, t.acts = [], []
        rs = np.random.RandomState(900)
        valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
        own = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid
        opp = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid & ~own
        pi = np.zeros((B, n * n), np.float32)
        pi[np.arange(B), rs.randint(0, n * n, B)] = 1
        t.forward_backward(own, opp, pi, rs.choice([-1.0, 1.0], B).astype(np.float32))
        _step_cache[n, B, C] = (t.acts, [z.grad.numpy().astype(np.float32) for z in t.zs])
    return _step_cache[n, B, C]


def _model_wgrad_tensor(x, dz, layer, B, arith, msplit, drop=None, inner="exact"):
    """model_wgrad for all nine taps of a 3x3 layer: (3, 3, Ci, Co)"""
    hout = dz.shape[1]
    if layer == 1:
        x = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    flat = np.ascontiguousarray(dz).reshape(B * hout * hout, -1)
    out = np.zeros((3, 3, x.shape[3], flat.shape[1]), np.float32)
    for ty in range(3):
        for tx in range(3):
            win = np.ascontiguousarray(x[:, ty:ty + hout, tx:tx + hout, :]).reshape(B * hout * hout, -1)
            out[ty, tx] = T.model_wgrad(win, flat, B, hout, arith, msplit, drop, inner)
    return out


def _separates(arith, healthy, weakest):
    m = T.MARGIN_WGRAD[arith]
    return 2 * healthy <= m and weakest >= 4 * m


def test_wgrad_groups_cover_every_row_once():
    for hout, B in [(h, B) for h in (2, 4, 6, 8) for B in (2, 5, 8, 9, 32, 64)]:
        rows = sorted(r for _, g in T.wgrad_groups(B, hout) for r in g)
        assert rows == list(range(B * hout * hout)) and all(len(g) <= 32 for _, g in T.wgrad_groups(B, hout))
    assert T.wgrad_msplit(8, 16, "bf16x3") == 1 and T.wgrad_msplit(9, 16, "bf16x3") == 2 and T.wgrad_msplit(64, 8, "f16x2") == 8


SEQ_MAX_ROWS = 80                      # the sequential model costs rows x 54 outer products of 256 x 256: evaluated up to here (every sharp shape is far below)
# (board, boards, layer): conv4 and conv3 at every small batch of the GPU matrix, conv2 where its sum is shortest
WGRAD_B3_SHAPES = [(6, B, l) for B in (2, 5, 8, 9) for l in (3, 2)] + [(8, 2, 3), (8, 2, 2), (6, 2, 1), (8, 2, 1)]


@pytest.mark.parametrize("n,B,layer", WGRAD_B3_SHAPES)
def test_wgrad_bf16x3_classes(n, B, layer):
    """every shape the matrix holds sharp separates -- margin >= 2 x the healthy ratio of the LESS exact of the two MFMA models, and <= a quarter of the
    weakest single-term defect; every other shape is printed with its figures and carries the coarse bound"""
    acts, dzs = _oracle_step(n, B)
    x, dz = acts[layer - 1], dzs[layer]
    rows = B * dz.shape[1] ** 2
    ref = T.wgrad(layer, x, dz, np.float64)
    E32 = _stat(T.wgrad(layer, x, dz, np.float32), ref)
    ms = T.wgrad_msplit(B, WGRAD_TILES["bf16x3"], "bf16x3")
    exact = _stat(_model_wgrad_tensor(x, dz, layer, B, "bf16x3", ms), ref) / E32
    seq = _stat(_model_wgrad_tensor(x, dz, layer, B, "bf16x3", ms, inner="sequential"), ref) / E32 if rows <= SEQ_MAX_ROWS else float("nan")
    weakest = min(_stat(_model_wgrad_tensor(x, dz, layer, B, "bf16x3", ms, drop=t), ref) / E32 for t in R.B3_TERMS)
    cls = T.wgrad_class("bf16x3", layer, rows)
    print(f"wgrad bf16x3 n={n} B={B} layer={layer} rows={rows} msplit={ms} zeros in x {np.mean(x == 0):.2f}: E32 {E32:.3g}  complete {exact:.2f} (one rounding per MFMA) "
          f"{seq:.2f} (one per product)  weakest term removed {weakest:.1f}  -> {cls}, margin {T.MARGIN_WGRAD['bf16x3'] if cls == 'sharp' else T.MARGIN_COARSE:g}")
    assert T.wgrad_class("f32", layer, rows) == cls and T.MARGIN_WGRAD["f32"] == T.MARGIN_WGRAD["bf16x3"]      # the exact-fp32 kernels: same shapes, same margin
    if cls == "sharp":
        assert rows <= SEQ_MAX_ROWS and _separates("bf16x3", max(exact, seq), weakest)
    else:
        assert exact <= T.MARGIN_COARSE


# f16x2 (k_wgrad_h2 runs from 32 boards on): synthetic rows (act_like, dz_like), one tap, 64 x 64 channels, both MFMA models
WGRAD_H2_SHAPES = [(2, 32), (4, 32), (6, 32), (4, 64), (6, 64), (8, 64)]


@pytest.mark.parametrize("hout,B", WGRAD_H2_SHAPES)
def test_wgrad_f16x2_classes(hout, B):
    rs = np.random.RandomState(9 + hout + B)
    rows = B * hout * hout
    x, z = T.act_like(rs, rows, 64), T.dz_like(rs, rows, 64)
    ref = x.astype(np.float64).T @ z.astype(np.float64)
    E32 = _stat(x.T @ z, ref)
    ms = T.wgrad_msplit(B, WGRAD_TILES["f16x2"], "f16x2")
    exact = _stat(T.model_wgrad(x, z, B, hout, "f16x2", ms), ref) / E32
    seq = _stat(T.model_wgrad(x, z, B, hout, "f16x2", ms, inner="sequential"), ref) / E32
    weakest = min(_stat(T.model_wgrad(x, z, B, hout, "f16x2", ms, drop=t), ref) / E32 for t in R.H2_TERMS)
    cls = T.wgrad_class("f16x2", 3, rows)
    print(f"wgrad f16x2  Hout={hout} B={B} rows={rows} msplit={ms}: E32 {E32:.3g}  complete {exact:.2f} (one rounding per MFMA) {seq:.2f} (one per product)  "
          f"weakest term removed {weakest:.1f}  -> {cls}, margin {T.MARGIN_WGRAD['f16x2']:g}")
    assert cls == "sharp" and _separates("f16x2", max(exact, seq), weakest)


def test_dense_weight_gradients_and_long_sums_are_coarse():
    assert T.wgrad_class("f32", 4, 32) == "coarse" and T.wgrad_class("f32", 5, 32) == "coarse"
    assert T.wgrad_class("bf16x3", 1, 72) == "coarse" and T.wgrad_class("bf16x3", 2, 32) == "coarse" and T.wgrad_class("bf16x3", 3, 64) == "coarse"
    assert T.wgrad_class("f16x2", 1, 8192) == "coarse"               # beyond what the model was evaluated on


# ------------------------------------------------------------------ the chip-filling tiles: which batch reaches which kernel
# the GPU matrix's chip cases (8x8, 512 filters): boards -> {layer: (forward kernel, data-gradient kernel)} of the 3x3 layers.  f16x2 is keyed on
# the call's boards, bf16x3 on the trainer's capacity
CHIP_PLANS = {
    ("f16x2", 383): {1: ("h2_midpp", "h2_midpp"), 2: ("h2_lowpp", "h2_midpp"), 3: ("h2_lowpp", "h2_lowpp")},
    ("f16x2", 447): {1: ("h2_bigpp", "h2_bigpp"), 2: ("h2_lowpp", "h2_bigpp"), 3: ("h2_lowpp", "h2_lowpp")},
    ("f16x2", 684): {1: ("h2_midpp", "h2_midpp"), 2: ("h2_bigpp", "h2_midpp"), 3: ("h2_lowpp", "h2_bigpp")},
    ("f16x2", 1023): {1: ("h2_bigpp", "h2_bigpp"), 2: ("h2_midpp", "h2_bigpp"), 3: ("h2_lowpp", "h2_midpp")},
    ("f16x2", 1535): {1: ("h2_bigpp", "h2_bigpp"), 2: ("h2_bigpp", "h2_bigpp"), 3: ("h2_midpp", "h2_bigpp")},
    ("f16x2", 1598): {1: ("h2_midpp", "h2_midpp"), 2: ("h2_bigpp", "h2_midpp"), 3: ("h2_bigpp", "h2_bigpp")},
    ("bf16x3", 383): {1: ("b3", "b3"), 2: ("b3", "b3_big"), 3: ("b3", "b3")},
    ("bf16x3", 684): {1: ("b3", "b3"), 2: ("b3_big", "b3"), 3: ("b3", "b3_big")},
    ("bf16x3", 1535): {1: ("b3", "b3"), 2: ("b3_big", "b3_big"), 3: ("b3_big", "b3_big")},
}
# what each of the three smallest exists for: (layer, side, kernel) that 64 boards fewer must NOT reach
CHIP_FIRST = {
    ("f16x2", 383): [(1, 0, "h2_midpp"), (1, 1, "h2_midpp"), (2, 1, "h2_midpp")],
    ("f16x2", 447): [(1, 0, "h2_bigpp"), (1, 1, "h2_bigpp"), (2, 1, "h2_bigpp")],
    ("f16x2", 684): [(2, 0, "h2_bigpp"), (3, 1, "h2_bigpp")],
    ("bf16x3", 383): [(2, 1, "b3_big")],
    ("bf16x3", 684): [(2, 0, "b3_big"), (3, 1, "b3_big")],
}
TILE_ROWS = {"h2_lowpp": 128, "h2_midpp": 192, "h2_bigpp": 256, "b3": 128, "b3_big": 256}


def _kernels(arith, B):
    p = T.tile_plan(arith, 8, 512, B)
    return {l: (p[l]["fwd_kernel"], p[l]["dgrad_kernel"]) for l in p}, p


@pytest.mark.parametrize("arith,B", sorted(CHIP_PLANS))
def test_chip_cases_reach_their_tiles(arith, B):
    """the launchers' tile rule restated (train_layer_ref.tile_rule / trainer_kslices): every chip case of the GPU matrix reaches the kernels it
    names, with one k-slice on the mid / big tiles and a partly filled last row tile; 64 boards fewer do not reach them"""
    kernels, plan = _kernels(arith, B)
    assert kernels == CHIP_PLANS[arith, B]
    for l in (1, 2, 3):
        g = T.geometry(8, 512, l)
        for side, rows in (("fwd", B * g["Hout"] ** 2), ("dgrad", B * g["Hin"] ** 2)):
            kernel, split = plan[l][side + "_kernel"], plan[l][side + "_kslices"]
            blocks128 = -(-rows // 128) * 2
            assert split == 1 if kernel in T.UNSPLIT_KERNELS else (split > 1) == (2 * blocks128 <= 256), (l, side, kernel, split)
            # the last row tile is partly filled -- but for 684 boards x 64 pixels = 228 whole 192-row tiles (conv2 and the data gradients of conv2 /
            # conv3 on H2MidPP, which 383 boards run with a partly filled one); what 684 exists for, H2BigPP on 36-pixel layers, is partly filled
            if kernel in T.UNSPLIT_KERNELS and (arith, B, kernel) != ("f16x2", 684, "h2_midpp"):
                assert rows % TILE_ROWS[kernel] != 0, (l, side, kernel, rows)
    for l, side, kernel in CHIP_FIRST.get((arith, B), []):
        assert kernels[l][side] == kernel and _kernels(arith, B - 64)[0][l][side] != kernel, (l, side, kernel)


def test_tile_rule_thresholds():
    """the rule at its edges, 512 columns: 192 blocks of 256 rows = more than 95 row tiles = 24321 rows and more; bf16x3 needs a 'valid' layer and a grid
    that costs no more than the 128-row tiles' at 0.93 a round"""
    assert T.tile_cost(36864, 512, 256) == 2 * 256 and T.tile_cost(36864, 512, 192) == 2 * 192          # oz_net.hip's own example: 1024 boards of conv3
    assert T.tile_rule("f16x2", 24320, 512, 0) == "low" and T.tile_rule("f16x2", 24321, 512, 1) == "mid"
    assert T.tile_rule("f16x2", 447 * 64, 512, 1) == "big"                                               # 224 blocks in one round; 192-row tiles would need a second
    assert T.tile_rule("bf16x3", 24320, 512, 0) == "low" and T.tile_rule("bf16x3", 24321, 512, 0) == "big" and T.tile_rule("bf16x3", 24321, 512, 1) == "low"
    assert T.tile_rule("bf16x3", 684 * 64, 512, 0) == "low"                                              # 342 big blocks pay two rounds of 256 rows, 684 small ones three of 128
    assert T.trainer_kslices("bf16x3", 8192, 512, 9 * 512, 0) == 2 and T.trainer_kslices("bf16x3", 8193, 512, 9 * 512, 0) == 1
    assert T.trainer_kslices("f16x2", 64 * 16, 256, 9 * 256, 0) == 9                                     # at least 8 k-tiles a slice: 72 // 9
    assert T.wgrad_msplit(383, 64, "bf16x3") == 4 and T.wgrad_msplit(383, 32, "f16x2") == 8 and T.wgrad_msplit(37, 64, "bf16x3") == 4


# ------------------------------------------------------------------ widths other than 128 / 256 / 512
# the GPU matrix's WIDTH_CASES of the split modes: (arithmetic, board, filters, capacity) -> forward / data-gradient k-slices of conv2, conv3, conv4
WIDTH_PLANS = {
    ("f16x2", 8, 768, 64): ((2, 4, 10), (2, 2, 4)),
    ("f16x2", 6, 768, 32): ((9, 16, 16), (9, 9, 16)),
    ("bf16x3", 8, 768, 64): ((2, 4, 10), (2, 2, 4)),
    ("bf16x3", 6, 768, 32): ((9, 16, 16), (9, 9, 16)),
    ("bf16x3", 6, 768, 9): ((16, 16, 16), (16, 16, 16)),
    ("bf16x3", 6, 1024, 32): ((7, 16, 16), (7, 7, 16)),
}


@pytest.mark.parametrize("arith,n,C,B", sorted(WIDTH_PLANS))
def test_width_cases_tile_plan(arith, n, C, B):
    """three (768) and four (1024) column tiles: every launch stays on the 128-row tile with its k loop split, and of each shape's slice counts at
    least one does not divide the 216 / 288 k-tiles (the slices then differ in length by one k-tile: kbeg = nk ks / ksplit)"""
    plan = T.tile_plan(arith, n, C, B)
    low = T.TILE_KERNEL[arith, "low"]
    fwd, dgrad = WIDTH_PLANS[arith, n, C, B]
    assert tuple(plan[l]["fwd_kslices"] for l in (1, 2, 3)) == fwd and tuple(plan[l]["dgrad_kslices"] for l in (1, 2, 3)) == dgrad, plan
    assert all(plan[l]["fwd_kernel"] == low and plan[l]["dgrad_kernel"] == low for l in (1, 2, 3)), plan
    nk = 9 * C // 32
    assert nk in (216, 288) and any(nk % k for k in fwd + dgrad), (nk, fwd, dgrad)
    assert all(nk // k >= 8 for k in fwd + dgrad)                                       # trainer_ksplit: at least 8 k-tiles a slice


def test_tile_rule_at_three_column_tiles():
    """768 columns: the 256-row tiles need ceil(rows / 256) x 3 >= 192 blocks = 64 row tiles = more than 16128 rows; the split of the 128-row tile fills one
    round of the chip with blocks = row tiles x 3"""
    assert T.tile_rule("f16x2", 16128, 768, 0) == "low" and T.tile_rule("f16x2", 16129, 768, 0) != "low"
    assert T.tile_rule("bf16x3", 16128, 768, 0) == "low" and T.tile_rule("bf16x3", 16129, 768, 0) == "big" and T.tile_rule("bf16x3", 16129, 768, 1) == "low"
    assert T.tile_cost(16129, 768, 256) == 256 and T.tile_cost(16129, 768, 128) == 2 * 128                 # 192 big blocks: one round; 381 small ones: two
    # 8x8 conv4 at 64 boards: 8 row tiles x 3 = 24 blocks -> 10 slices (240 blocks; 11 would be 264), 216 k-tiles in slices of 21 or 22
    assert T.trainer_kslices("bf16x3", 64 * 16, 768, 9 * 768, 0) == 10 and T.trainer_kslices("f16x2", 64 * 16, 768, 9 * 768, 0) == 10
    assert sorted({216 * (k + 1) // 10 - 216 * k // 10 for k in range(10)}) == [21, 22]
    # 6x6 conv2 at 32 boards and 1024 filters: 9 row tiles x 4 = 36 blocks -> 7 slices (252), 288 k-tiles in slices of 41 or 42
    assert T.trainer_kslices("bf16x3", 32 * 36, 1024, 9 * 1024, 1) == 7 and sorted({288 * (k + 1) // 7 - 288 * k // 7 for k in range(7)}) == [41, 42]
    # f32 at 384 filters has no tile rule to restate (GmStd; N % 256 keeps it off the 256 x 256 tile); the octet split at 72 / 144 / 256 tiles
    assert T.wgrad_msplit(64, 72, "f16x2") == 4 and T.wgrad_msplit(32, 72, "f16x2") == 4 and T.wgrad_msplit(64, 144, "bf16x3") == 2
    assert T.wgrad_msplit(9, 144, "bf16x3") == 2 and T.wgrad_msplit(37, 144, "bf16x3") == 2 and T.wgrad_msplit(32, 256, "bf16x3") == 1


# every trainer shape of the GPU matrix's WIDTH_CASES: (board, filters, boards of a step)
WIDTH_STEPS = [(6, 384, 8), (8, 384, 64), (8, 384, 65), (8, 384, 192), (8, 768, 64), (8, 768, 37), (6, 768, 32), (6, 768, 9), (6, 1024, 32)]


@pytest.mark.parametrize("n,C,B", WIDTH_STEPS)
def test_width_cases_keep_their_columns(n, C, B):
    """the float64 oracle alone (oracle/train_ref.py, a batch of that size drawn as the GPU matrix draws its own): at least half of the dz columns of every layer are
    alive -- the condition under which the GPU test may leave a column out -- checked before the batch sizes of WIDTH_CASES were fixed"""
    _, dzs = _oracle_step(n, B, C)
    kept = [float((np.abs(dz.reshape(-1, dz.shape[-1])).max(axis=0) > 0).mean()) for dz in dzs]
    print(f"kept dz columns n={n} C={C} B={B}: " + " ".join(f"{k:.2f}" for k in kept))
    assert len(kept) == 6 and min(kept) >= 0.5, kept
    assert all(k == 1.0 for k in kept[:4]), kept                                         # conv1 and the 3x3 layers lose no column


# ------------------------------------------------------------------ the chip cases' weight gradient: what the coarse bound still sees
CHIP_WGRAD_TILES = {"bf16x3": 64, "f16x2": 32}                                            # (Cin / CI) x (Co / CO) at 512 filters
_chip_wgrad_cache = {}


def _chip_wgrad_block():
    """conv3 at 383 boards (13788 rows, 48 octets), a block of 32 input channels x 64 output columns, one tap, synthetic rows"""
    if not _chip_wgrad_cache:
        B, hout = 383, 6
        rs = np.random.RandomState(383)
        x, z = T.act_like(rs, B * hout * hout, 32), T.dz_like(rs, B * hout * hout, 64)
        ref = x.astype(np.float64).T @ z.astype(np.float64)
        _chip_wgrad_cache["v"] = (B, hout, x, z, ref, _stat(x.T @ z, ref))
    return _chip_wgrad_cache["v"]


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
def test_chip_wgrad_bound_sees_lost_rows(arith):
    """over 13788 rows E32 has grown to where a lost plane product hides inside the coarse bound (the module docstring: 9 .. 17 x E32 at 72 .. 512 rows
    already); what MARGIN_COARSE does catch at the chip cases' sizes is BOOKKEEPING: an octet of 8 boards whose k-steps are skipped, or a slab
    of the octet split that is never added -- each must exceed the bound at least fourfold, while the complete model stays within it"""
    B, hout, x, z, ref, E32 = _chip_wgrad_block()
    ms = T.wgrad_msplit(B, CHIP_WGRAD_TILES[arith], arith)
    noct = (B + 7) // 8
    full = _stat(T.model_wgrad(x, z, B, hout, arith, ms), ref) / E32
    octets = {o: _stat(T.model_wgrad(x, z, B, hout, arith, ms, drop_octet=o), ref) / E32 for o in (0, noct // 2, noct - 1)}     # (the last one holds 7 boards)
    slabs = {s: _stat(T.model_wgrad(x, z, B, hout, arith, ms, drop_slab=s), ref) / E32 for s in range(ms)}
    print(f"wgrad {arith:6s} conv3 B={B} rows={B * hout * hout} msplit={ms}: E32 {E32:.3g}  complete {full:.2f}  octet lost {min(octets.values()):.0f} .. "
          f"{max(octets.values()):.0f}  slab lost {min(slabs.values()):.0f} .. {max(slabs.values()):.0f}  -> coarse, margin {T.MARGIN_COARSE:g}")
    assert T.wgrad_class(arith, 2, B * hout * hout) == "coarse"
    assert full <= T.MARGIN_COARSE
    assert min(octets.values()) >= 4 * T.MARGIN_COARSE and min(slabs.values()) >= 4 * T.MARGIN_COARSE


def test_sampled_weight_gradient_is_a_slice_of_the_whole():
    """the chip cases' weight-gradient reference (every 16th input channel) is the same slice of the whole tensor's reference (float64, to the
    order of the sums), and its norm_c is at most the whole one's"""
    rs = np.random.RandomState(2)
    for layer, hin in ((1, 4), (2, 6)):
        hout = hin if layer == 1 else hin - 2
        x, dz = rs.standard_normal((3, hin, hin, 64)), rs.standard_normal((3, hout, hout, 8))
        whole = T.wgrad(layer, x, dz, np.float64)
        part = T.wgrad(layer, T.sampled_ci(x, 3), dz, np.float64)
        assert part.shape == (3, 3, 64 // T.WGRAD_CI_STRIDE, 8) and np.allclose(part, T.sampled_ci(whole, 2), rtol=1e-12, atol=1e-12)
        assert np.all(T.column_norm(part) <= T.column_norm(whole) * (1 + 1e-12))
    assert T.WGRAD_CI_STRIDE <= 32                                       # at least one sampled channel in every 32-wide input-channel tile


# ------------------------------------------------------------------ few-row samples
def test_few_row_samples_need_the_norm_of_many_rows():
    """the dense layers' data gradient of a B-board step has B rows.  Two healthy fp32 evaluations of fc2's data gradient (NumPy's, and the same sums
    in float32 in the opposite order) differ, on some single row under that row's OWN norm, by more than the margin x E32 of that row -- an element
    that nearly cancels has an unbounded relative error -- and stay within it on every row under the norm of all the rows: the GPU matrix takes
    norm_c over at least ROWS_FOR_NORM boards (several steps at small batches)"""
    w = R.network_weights(8, 256, "bisparse")
    k = np.asarray(w[30], np.float32)                                   # fc2 (1024, 512): 4 entries per input row
    dz = T.dz_like(np.random.RandomState(11), ROWS, 512)
    ref = dz.astype(np.float64) @ k.astype(np.float64).T
    a32 = dz @ k.T
    other = np.zeros_like(a32)
    for c in range(511, -1, -1):                                        # float32, descending column order
        other = other + dz[:, c:c + 1] * k[:, c][None, :]
    norm = T.column_norm(ref)
    assert T.statistic(other, ref)[0] <= T.MARGIN_DGRAD["f32"] * T.statistic(a32, ref)[0]
    own = np.array([T.statistic(other[i:i + 1], ref[i:i + 1])[0] / max(T.statistic(a32[i:i + 1], ref[i:i + 1])[0], 1e-300) for i in range(ROWS)])
    many = np.array([T.statistic(other[i:i + 1], ref[i:i + 1], norm)[0] for i in range(ROWS)])
    e_many = np.array([T.statistic(a32[i:i + 1], ref[i:i + 1], norm)[0] for i in range(ROWS)])
    print(f"few rows: one row under its own norm, worst ratio of two healthy fp32 evaluations {own.max():.1f}; under the norm of {ROWS} rows, worst err "
          f"{many.max():.3g} against E32 of the sample {T.statistic(a32, ref)[0]:.3g}")
    assert own.max() > T.MARGIN_DGRAD["f32"]
    assert many.max() <= T.MARGIN_DGRAD["f32"] * T.statistic(a32, ref)[0] and e_many.max() <= T.statistic(a32, ref)[0]
    assert T.ROWS_FOR_NORM >= 64


def test_zero_columns_must_be_exactly_zero():
    ref = np.array([[1.0, 0.0], [2.0, 0.0]])
    assert T.statistic(np.array([[1.0, 0.0], [2.0, 0.0]]), ref) == (0.0, 0.5)
    with pytest.raises(AssertionError):
        T.statistic(np.array([[1.0, 1e-30], [2.0, 0.0]]), ref)


# ------------------------------------------------------------------ the references against a plain definition
def test_references_match_plain_definitions():
    """dgrad / wgrad (tap-wise BLAS products) against the defining sums on a tiny layer, 'same' and 'valid'"""
    rs = np.random.RandomState(1)
    for layer, hin in ((1, 4), (2, 5)):
        pad = 1 if layer == 1 else 0
        hout = hin + 2 * pad - 2
        w = [None] * 40
        w[6 * layer] = rs.standard_normal((3, 3, 3, 2))
        w[6 * layer + 1] = rs.standard_normal(2)
        x, dz = rs.standard_normal((2, hin, hin, 3)), rs.standard_normal((2, hout, hout, 2))
        z = np.zeros((2, hout, hout, 2)) + w[6 * layer + 1]
        dx, dw = np.zeros_like(x), np.zeros((3, 3, 3, 2))
        for b in range(2):
            for oy in range(hout):
                for ox in range(hout):
                    for ty in range(3):
                        for tx in range(3):
                            iy, ix = oy + ty - pad, ox + tx - pad
                            if 0 <= iy < hin and 0 <= ix < hin:
                                z[b, oy, ox] += x[b, iy, ix] @ w[6 * layer][ty, tx]
                                dx[b, iy, ix] += w[6 * layer][ty, tx] @ dz[b, oy, ox]
                                dw[ty, tx] += np.outer(x[b, iy, ix], dz[b, oy, ox])
        assert np.allclose(T.forward_z(w, layer, x, np.float64), z, rtol=1e-12, atol=1e-12)
        assert np.allclose(T.dgrad(w, layer, dz, np.float64), dx, rtol=1e-12, atol=1e-12)
        assert np.allclose(T.wgrad(layer, x, dz, np.float64), dw, rtol=1e-12, atol=1e-12)
