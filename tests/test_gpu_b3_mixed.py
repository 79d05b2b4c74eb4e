"""precision bf16x3, the mixed plan of conv3 / conv4 (oz_net.hip launch_b3: the layer's leading rows on k_gemm_b3_big's 256-row tiles, the rows behind them
on k_gemm_b3's 128-row tiles, the second launch's row tiles offset by B3Geom::mt0): OZ_NET_OPT_B3_MIX_ROWS puts the boundary into a small network, and
every (pi, v) must be BIT-identical to the 128-row tile alone -- both tiles add every output element's products in the same order -- and within 1e-5 of
the float64 oracle, wherever the end of the batch falls relative to the boundary."""
import numpy as np
import pytest

import oracle
from oracle import nn_numpy

pytestmark = pytest.mark.gpu

TOL = 1e-5
C_ = 512
MB = 160


@pytest.fixture(scope="module")
def oz():
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _boards(n, count, seed):
    rs = np.random.RandomState(seed)
    own, opp = [], []
    for _ in range(count):
        a = rs.rand(n, n) < 0.4
        b = (rs.rand(n, n) < 0.4) & ~a
        o, p = oracle.pack_board(np.stack([a, b], axis=2))
        own.append(o); opp.append(p)
    return np.array(own, np.uint64), np.array(opp, np.uint64)


_CACHE = {}


def _case(n):
    """network, MB boards and their float64 (pi, v) -- once per board size; every parameter kind random, logits lifted away from uniform"""
    if n not in _CACHE:
        from othellozero_amd.NNet import NNetWrapper
        from othellozero_amd.weights import init_weights
        w = init_weights(n, seed=13, channels=C_, randomize_all=True)
        for i in (36, 38):
            w[i] = w[i] * 4.0
        own, opp = _boards(n, MB, seed=n + C_)
        pi64, v64 = nn_numpy.forward(w, own, opp, n)
        assert pi64.std() > 2e-3 and np.abs(v64).max() > 0.05
        net = NNetWrapper((n, n), num_channels_1=C_, max_batch=MB, weights=w, precision="bf16x3")
        assert net.arithmetic() == "bf16x3"
        _CACHE[n] = (net, own, opp, pi64, v64)
    return _CACHE[n]


def _rows_around(mix, rows):
    """row ranges of a layer's output on both sides of the boundary, clipped to the call"""
    lo, hi = max(mix - 96, 0), min(mix + 96, rows)
    return (lo, hi - lo) if hi > lo else None


def _check(oz, n, mix, count, layers):
    """one call of `count` boards: the 128-row tile alone, then three times the mixed plan with `mix` leading rows; `layers` = {plan layer: pixels} that must mix"""
    net, own, opp, pi64, v64 = _case(n)
    net.set_option(oz.NET_OPT_B3_MIX_ROWS, mix)
    net.set_option(oz.NET_OPT_B3_TILE, 128)
    p0, v0 = net.predict_batch(own[:count], opp[:count])
    plan0 = net.layer_plan()
    assert all(plan0[l]["kernel"] == "b3" and plan0[l]["big_rows"] == 0 for l in layers), plan0
    act0 = {l: net.activation(l, *_rows_around(mix, count * px)) for l, px in layers.items() if _rows_around(mix, count * px)}
    assert np.abs(p0.reshape(count, -1) - pi64[:count]).max() <= TOL and np.abs(v0 - v64[:count]).max() <= TOL
    net.set_option(oz.NET_OPT_B3_TILE, 0)
    for rep in range(3):                                      # (repeated: a DMA visibility race would be intermittent)
        p, v = net.predict_batch(own[:count], opp[:count])
        assert np.array_equal(p, p0) and np.array_equal(v, v0), (n, mix, count, rep)
        assert np.abs(p.reshape(count, -1) - pi64[:count]).max() <= TOL and np.abs(v - v64[:count]).max() <= TOL
    plan = net.layer_plan()
    for l in layers:
        assert plan[l] == dict(tile_rows=128, kslices=plan0[l]["kslices"], kernel="b3_mixed", big_rows=mix), (l, plan[l])
    assert net.conv3_tile_rows() == 128
    for l, a0 in act0.items():                                # the layer's own output on both sides of the boundary, bit for bit
        a = net.activation(l, *_rows_around(mix, count * layers[l]))
        assert a.shape == a0.shape and np.array_equal(a, a0) and np.abs(a).max() > 0, (n, mix, count, l)
    net.set_option(oz.NET_OPT_B3_MIX_ROWS, 0)


# 8x8: conv3 has 36 rows per board, so 256 rows end inside board 7 and 512 rows inside board 14.  5 boards end below either boundary; 8 and 15
# put a boundary inside the last board; 37 boards (1332 rows) leave the last 128-row tile of the remainder partly filled; 160 = the capacity; 1
@pytest.mark.parametrize("count", [5, 8, 15, 37, MB, 1])
@pytest.mark.parametrize("mix", [256, 512])
def test_conv3_rows_on_both_tiles_8x8(oz, mix, count):
    _check(oz, 8, mix, count, {2: 36})


@pytest.mark.parametrize("mix,count", [(256, 16), (256, 17), (512, 100), (512, MB)])
def test_board_edges_on_tile_edges_6x6(oz, mix, count):
    """6x6: conv3 has 16 rows per board -- the boundary is a board edge, and 16 boards end exactly on it (no second launch at all)"""
    _check(oz, 6, mix, count, {2: 16, 3: 4})


@pytest.mark.parametrize("mix,count", [(256, 15), (256, 17), (512, 37), (512, MB)])
def test_conv4_through_the_same_option(oz, mix, count):
    """conv4 of the 8x8 network (16 rows per board, 2560 at capacity, 8 k-slices): the option cuts it too, 15 boards end below the 256-row boundary"""
    _check(oz, 8, mix, count, {2: 36, 3: 16})


def test_the_option_by_default_and_refused_values(oz):
    net, own, opp, _, _ = _case(8)
    p0, v0 = net.predict_batch(own, opp)
    plan = net.layer_plan()
    assert plan[2]["kernel"] == "b3" and plan[3]["kernel"] == "b3" and plan[2]["big_rows"] == 0      # a network of 160 boards never mixes on its own
    for value in (-1, 256 * 40):                              # never mix; a boundary beyond the capacity's rows is ignored
        net.set_option(oz.NET_OPT_B3_MIX_ROWS, value)
        p, v = net.predict_batch(own, opp)
        assert net.layer_plan() == plan and np.array_equal(p, p0) and np.array_equal(v, v0)
    for value in (100, 384):
        with pytest.raises(oz.OzError):
            net.set_option(oz.NET_OPT_B3_MIX_ROWS, value)
    net.set_option(oz.NET_OPT_B3_MIX_ROWS, 0)
