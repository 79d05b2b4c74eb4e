"""The margins of the per-layer parity tests (tests/test_gpu_layer_parity.py) can detect a defect: shown on the CPU, with NumPy models of the
two split arithmetics (tests/layer_ref.py), on the sparse layer shapes of the GPU matrix -- never by breaking a kernel on the GPU.

For every shape: the complete bf16x3 / f16x2 product stays at or below margin x E32, and the product with ANY single kept term removed lies above
2 x margin x E32 -- a kernel that lost a term cannot pass the bound the healthy kernel is held to, with a factor of two to spare.  The margins
are re-derived here on every run; the figures in layer_ref's docstring are what this test printed when they were chosen."""
import numpy as np
import pytest

import layer_ref as R

ROWS = 96
# (board, filters, layer): K = 2304 and 4608 for the convolutions, 4096 and 8192 for fc1, 1024 for fc2
SHAPES = [(8, 256, 2, 2304), (8, 512, 2, 4608), (8, 256, 4, 4096), (8, 512, 4, 8192), (8, 256, 5, 1024)]
# ... and the widths of the GPU matrix's WIDTH_CASES: K = 3456 (384 filters), 6912 (768), 9216 (1024) for the convolutions, fc1 at 12288 (8x8, 768) and 3072
# (6x6, 768).  The sums are still 8 terms long, so the margins separate as they do above (the figures are printed on every run)
SHAPES += [(8, 384, 2, 3456), (8, 768, 2, 6912), (6, 1024, 2, 9216), (8, 768, 4, 12288), (6, 768, 4, 3072)]
_case_cache = {}


def _case(n, C, layer, K):
    """the layer's sparse weights, random ReLU inputs (a third of them zero, like a ReLU output), z64 and E32 -- computed once per shape"""
    key = (n, C, layer)
    if key not in _case_cache:
        w = R.network_weights(n, C, "sparse")
        geo = R.layer_geometry(n, C, layer)
        assert geo[4] == K and np.asarray(w[R.KERNELS[layer - 1]]).size == K * geo[5]
        rs = np.random.RandomState(100 + layer + C)
        a = np.maximum(rs.normal(0.1, 0.4, size=(ROWS, K)), 0).astype(np.float32)
        chan = np.arange(K) % (C if layer <= 4 else 1024)

        def z(dt):          # the layer on plain rows (a convolution's output pixel whose nine taps are all inside the image is this dot product)
            k, bias, g, b, mu, var = (np.asarray(x, dt) for x in w[6 * layer:6 * layer + 6])
            return R.nn_numpy._bn(a.astype(dt) @ k.reshape(K, -1) + bias, g, b, mu, var)
        z64 = z(np.float64)
        _case_cache[key] = (w, a, chan, z64, R.statistic(np.maximum(z(np.float32), 0), z64))
    return _case_cache[key]


@pytest.mark.parametrize("n,C,layer,K", SHAPES)
def test_sparse_columns_and_yardstick(n, C, layer, K):
    w, a, chan, z64, E32 = _case(n, C, layer, K)
    for i in R.KERNELS:
        nz = (np.asarray(w[i]).reshape(-1, w[i].shape[-1]) != 0).sum(axis=0)
        assert np.all(nz == R.SPARSE_NNZ), (i, np.unique(nz))
    for i in range(40):                                  # everything else is the dense network's own draw
        if i not in R.KERNELS:
            assert np.array_equal(w[i], R.network_weights(n, C, "dense")[i])
    assert E32 > 0
    print(f"shape n={n} C={C} layer={layer} K={K}: E32 = {E32:.3g}")


@pytest.mark.parametrize("n,C,layer,K", SHAPES)
def test_bf16x3_margin_separates_every_single_term_defect(n, C, layer, K):
    w, a, chan, z64, E32 = _case(n, C, layer, K)
    full = R.statistic(R.model_b3(w, layer, a), z64)
    print(f"bf16x3 K={K}: complete {full / E32:.2f} x E32")
    assert full <= R.MARGIN_B3 * E32
    assert R.MARGIN_F32 == R.MARGIN_B3
    for term in R.B3_TERMS:
        d = R.statistic(R.model_b3(w, layer, a, drop=term), z64)
        print(f"bf16x3 K={K}: without a{term[0]} b{term[1]} {d / E32:.1f} x E32")
        assert d > 2 * R.MARGIN_B3 * E32, term


@pytest.mark.parametrize("n,C,layer,K", SHAPES)
def test_f16x2_margin_separates_every_single_term_defect(n, C, layer, K):
    w, a, chan, z64, E32 = _case(n, C, layer, K)
    full = R.statistic(R.model_h2(w, layer, a, chan), z64)
    print(f"f16x2 K={K}: complete {full / E32:.2f} x E32")
    assert full <= R.MARGIN_H2 * E32
    for term in R.H2_TERMS:
        d = R.statistic(R.model_h2(w, layer, a, chan, drop=term), z64)
        print(f"f16x2 K={K}: without a{term[0]} w{term[1]} {d / E32:.0f} x E32")
        assert d > 2 * R.MARGIN_H2 * E32, term


@pytest.mark.parametrize("n,C,layer,K", SHAPES)
def test_one_row_samples_need_the_norm_of_many_rows(n, C, layer, K):
    """a one-row sample under its OWN norm (|z64| of the single element) cannot be held to the margins: the complete bf16x3 product exceeds them on
    some row; under the norm of the whole sample every single row separates again -- complete within the margin, any single term removed above it"""
    w, a, chan, z64, _ = _case(n, C, layer, K)
    k, bias, g, b, mu, var = (np.asarray(x, np.float32) for x in w[6 * layer:6 * layer + 6])
    out32 = np.maximum(R.nn_numpy._bn(a @ k.reshape(K, -1) + bias, g, b, mu, var), 0)
    norm = R.channel_norm(z64)
    per_row = lambda out, nm: np.array([R.statistic(out[i:i + 1], z64[i:i + 1], nm) for i in range(ROWS)])
    own = lambda out: np.array([R.statistic(out[i:i + 1], z64[i:i + 1]) for i in range(ROWS)])
    full_b3, full_h2 = R.model_b3(w, layer, a), R.model_h2(w, layer, a, chan)
    assert (own(full_b3) / own(out32)).max() > R.MARGIN_B3              # a healthy product, refused by the one-row norm
    e = per_row(out32, norm)
    assert np.all(per_row(full_b3, norm) <= R.MARGIN_B3 * e) and np.all(per_row(full_h2, norm) <= R.MARGIN_H2 * e)
    for term in R.B3_TERMS:
        assert np.all(per_row(R.model_b3(w, layer, a, drop=term), norm) > R.MARGIN_B3 * e), term
    for term in R.H2_TERMS:
        assert np.all(per_row(R.model_h2(w, layer, a, chan, drop=term), norm) > 2 * R.MARGIN_H2 * e), term


def test_split_planes_are_exact():
    """the models' own planes: three bf16 planes hold an fp32 value exactly, two fp16 planes hold a value placed in [2^-3, 2^-2) to the 2^-25
    of fp16's subnormal step (the absolute floor oz_net_h2.h states)"""
    rs = np.random.RandomState(3)
    x = (rs.standard_normal(4096) * np.exp(rs.uniform(-20, 20, 4096))).astype(np.float32)
    b1, b2, b3 = R.b3_planes(x)
    assert np.array_equal((b1.astype(np.float64) + b2) + b3, x.astype(np.float64))
    for p in (b1, b2, b3):
        assert np.all(p.view(np.uint32) & 0xFFFF == 0)
    y = rs.uniform(2.0 ** -3, 2.0 ** -2, 4096).astype(np.float32)
    h1, h2 = R.h2_planes(y)
    assert np.abs((h1.astype(np.float64) + h2) - y).max() <= 2.0 ** -25


def test_sample_runs_cover_start_middle_and_end():
    assert R.sample_runs(1, 36) == [(0, 1)]
    assert R.sample_runs(5, 36) == [(0, 5)]
    runs = R.sample_runs(683, 36)
    assert runs == [(0, 9), (337, 9), (674, 9)]
    assert R.sample_runs(1024, 1)[-1] == (1024 - 257, 257)
    for count, px in ((37, 16), (430, 36), (12, 64), (300, 1)):
        runs = R.sample_runs(count, px)
        assert runs[0][0] == 0 and sum(runs[-1]) == count
        assert all(a[0] + a[1] < b[0] for a, b in zip(runs, runs[1:]))
