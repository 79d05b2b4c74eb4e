"""Per-layer parity of the network forward at fp32-rounding tolerance (pytest -m gpu).

Every GEMM layer (conv2, conv3, conv4, fc1, fc2) of one forward is compared with the float64 reference OF THAT LAYER evaluated from the GPU's own
output of the previous layer (NNetWrapper.activation), in units of E32 = what NumPy float32 loses on the same layer and rows (tests/layer_ref.py:
statistic, yardstick, networks, margins; tests/test_layer_parity_cpu.py shows on the CPU that the margins separate every single-term defect of the
two split arithmetics).  The bounds: err <= margin x E32 on the sparse network (f32 and bf16x3: 6, f16x2: 16), err <= 16 x E32 on the dense one.
norm_c of the statistic is taken over the sampled rows of all the calls a case makes on a network, not over one call's rows alone: a one-board call
has ONE row in the dense layers, and under that row's own norm the statistic is an element's relative error, which no fp32-class arithmetic bounds
(measured: f16x2 fc1, 8x8 / 256 filters, one board: 34.6 x E32 under its own norm, 3.1 x under the case's; layer_ref's docstring has the reasoning,
the CPU test the demonstration).  The ratio under the call's own norm is printed next to the asserted one.

The matrix runs every tile / split-K / reduce / main-loop configuration the three forwards can select, each at three call sizes (full capacity, an
odd size that is no multiple of a tile height, one board), and proves which kernel ran from NNetWrapper.layer_plan(); the last test asserts that
the configurations seen are exactly the list REQUIRED.  WIDTH_CASES repeat the matrix at 384 (f32), 768 (all three) and 1024 filters, where only the
index arithmetic differs -- odd column-tile counts in both block mappings, k splits that do not divide the k-tiles, fc1 at K = 12288 -- under the
same margins; REQUIRED_WIDTHS names every (precision, kernel, filters) they must reach.  One line per (precision, case, layer, network kind, call
size) is printed: err, E32, ratio, and one per case with its time (the table of one run: profiles/layer_parity_ratios.txt)."""
import time

import numpy as np
import pytest

import layer_ref as R
import minimax_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    yield _lib
    _nets.clear()


# ------------------------------------------------------------------ inputs
_board_cache = {}


def _boards(n, count, first=0):
    """`count` mover-canonical positions from `first` on: every position of two random playouts first (openings .. full boards, what a search feeds the
    network), then random fillings; the same sequence for every count"""
    if n not in _board_cache:
        games = minimax_ref.playout_positions(n, 31 + n, 2)
        own = [b if p == 1 else w for b, w, p in games]
        opp = [w if p == 1 else b for b, w, p in games]
        rs = np.random.RandomState(500 + n)
        a = rs.rand(1536, 8, 8) < 0.4
        b = (rs.rand(1536, 8, 8) < 0.4) & ~a
        a[:, n:, :] = a[:, :, n:] = b[:, n:, :] = b[:, :, n:] = False
        bit = (np.uint64(1) << np.arange(64, dtype=np.uint64)).reshape(8, 8)
        pack = lambda m: (m * bit).sum(axis=(1, 2), dtype=np.uint64)
        _board_cache[n] = (np.concatenate([np.array(own, np.uint64), pack(a)])[:1536], np.concatenate([np.array(opp, np.uint64), pack(b)])[:1536])
    own, opp = _board_cache[n]
    assert first + count <= own.size
    return own[first:first + count], opp[first:first + count]


# ------------------------------------------------------------------ networks (built once per shape and kind, shared by the cases that only flip forward-time switches)
_nets = {}
_self_check = {}


def _net(oz, precision, n, C, mb, kind):
    from othellozero_amd.NNet import NNetWrapper
    key = (precision, n, C, mb, kind)
    if key not in _nets:
        w = R.network_weights(n, C, kind)
        try:
            net = NNetWrapper((n, n), num_channels_1=C, max_batch=mb, weights=w, precision=precision)
        except oz.OzError as e:
            # precision f16x2 may refuse a network at commit for a stated conditioning reason (self-check on, guards armed): that leg then runs with
            # the self-check in measure-only mode; the layer assertions stay as they are
            if not (precision == "f16x2" and e.code == oz.OZ_ERR_STATE):
                raise
            print(f"f16x2 commit refused {key}: {e}")
            net = NNetWrapper((n, n), num_channels_1=C, max_batch=mb, weights=R.network_weights(n, C, "dense"), precision=precision)
            net.set_option(oz.NET_OPT_SELF_CHECK, 2)
            net.set_weights(w)
        if precision == "f16x2":
            _self_check[key] = net.self_check() + (net.self_check_guard(),)
            print(f"f16x2 self-check {key}: max|d pi| {_self_check[key][0]:.3g} max|d v| {_self_check[key][1]:.3g} on {_self_check[key][2]} positions, guard bits {_self_check[key][3]}")
        _nets[key] = net
    return _nets[key]


FORWARD_SWITCHES = ("tables", "simple_loop", "conv3_tile", "low_loop_phases", "b3_tile", "f32_std_tile")


def _apply(oz, net, setup):
    s = dict(tables=-1, simple_loop=0, conv3_tile=0, low_loop_phases=1, b3_tile=0, f32_std_tile=0)
    assert set(setup) <= set(s), setup
    s.update(setup)
    net.set_tables(s["tables"])
    net.set_option(oz.NET_OPT_SIMPLE_LOOP, s["simple_loop"])
    net.set_option(oz.NET_OPT_CONV3_TILE, s["conv3_tile"])
    net.set_option(oz.NET_OPT_LOW_LOOP_PHASES, s["low_loop_phases"])
    net.set_option(oz.NET_OPT_B3_TILE, s["b3_tile"])
    net.set_option(oz.NET_OPT_F32_STD_TILE, s["f32_std_tile"])


# ------------------------------------------------------------------ one forward, layer by layer
def _rows(net, layer, runs, pixels):
    return np.concatenate([net.activation(layer, b0 * pixels, nb * pixels) for b0, nb in runs])


def measure(oz, net, weights, n, C, own, opp):
    """one predict_batch of the boards, then for every GEMM layer its sampled rows -- (gpu, relu of the float32 evaluation, z64) -- and the launch plan"""
    count = own.size
    assert count <= net.max_batch
    net.predict_batch(own, opp)
    plan = net.layer_plan()
    try:
        net.activation(0, 0, 1)
        conv1_materialised = True
    except oz.OzError as e:
        assert e.code == oz.OZ_ERR_STATE, e
        conv1_materialised = False
    out = {}
    for layer in range(1, 6):
        hin, hout, _, taps, K, N = R.layer_geometry(n, C, layer)
        pix_out = hout * hout
        pix_in = (n - 4) ** 2 if layer == 4 else hin * hin
        runs = R.sample_runs(count, pix_out)
        gpu = _rows(net, layer, runs, pix_out)
        boards = sum(nb for _, nb in runs)
        assert gpu.shape == (boards * pix_out, N)                    # every output of every sampled row is compared
        if layer == 1 and not conv1_materialised:
            # the table modes: conv2's input never exists -- the reference is conv1 -> conv2 from the boards, in float64 and in float32
            sel = np.concatenate([np.arange(b0, b0 + nb) for b0, nb in runs])
            x64, x32 = (R.conv1_out(weights, own[sel], opp[sel], n, dt) for dt in (np.float64, np.float32))
        else:
            x64 = _rows(net, layer - 1, runs, pix_in)
            x64 = x64.reshape(boards, hin, hin, -1) if layer <= 3 else x64.reshape(boards, -1)
            x32 = x64.astype(np.float32)
            assert np.array_equal(x32.astype(np.float64), x64)       # what a kernel multiplies is an fp32 value
        out[layer] = (gpu, np.maximum(R.layer_z(weights, layer, x32, np.float32), 0), R.layer64(weights, layer, x64))
    return out, plan


def evaluate(calls):
    """calls: list of (count, measure()'s layers, plan) of ONE network -> rows dict(count, layer, err, e32, own, plan): err and E32 under norm_c = max
    over the sampled rows of all these calls (layer_ref: few-row samples); own = err / E32 under the call's own rows' norm, printed for the record"""
    rows = []
    for layer in range(1, 6):
        norm = np.max([R.channel_norm(res[layer][2]) for _, res, _ in calls], axis=0)
        for count, res, plan in calls:
            gpu, out32, z64 = res[layer]
            err, e32 = R.statistic(gpu, z64, norm), R.statistic(out32, z64, norm)
            assert e32 > 0
            rows.append(dict(count=count, layer=layer, err=err, e32=e32, own=R.statistic(gpu, z64) / R.statistic(out32, z64), plan=plan[layer]))
    return rows


# ------------------------------------------------------------------ the matrix
# Shapes: the smallest capacity at which the launcher's own condition selects the configuration (oz_net.hip: oz_gemm_f32_launch, part32_mult, conv_ksplit,
# conv4_low, conv_b3_ksplit, fc1_b3_ksplit, b3_big_tile_pays), 256 filters unless the configuration needs 512.  `expect`: layer -> (kernel, k-slices) the
# plan must report at FULL capacity (smaller calls may take another tile: whatever they take is compared and recorded too).
def _case(name, precision, n, C, mb, sizes, expect, **setup):
    return dict(name=name, precision=precision, n=n, C=C, mb=mb, sizes=sizes, expect=expect, setup=setup)


CASES = [
    # ---- f32
    # 6x6, four boards: conv3 (64 rows), conv4, fc1, fc2 are weight streams (k_gemm_f32_skinny; fc2's slices added by the heads); conv2 the thread-per-pixel gather
    _case("f32-skinny", "f32", 6, 256, 4, (4, 3, 1), {1: ("lut", 1), 2: ("f32_skinny", 36), 3: ("f32_skinny", 36), 4: ("f32_skinny", 16), 5: ("f32_skinny", 16)}),
    # 32 < max_batch <= 128: GmStd with the k loop split 8 / 16 ways + k_splitk_reduce_f32; fc2 four slices, added by the heads
    _case("f32-splitk", "f32", 8, 256, 96, (96, 85, 1), {1: ("lut", 1), 2: ("f32_std", 8), 3: ("f32_std", 8), 4: ("f32_std", 16), 5: ("f32_std", 4)}),
    # conv2 as a GEMM on pixel-major tiles: tables off, capacity >= 256
    _case("f32-pixmajor", "f32", 8, 256, 256, (256, 203, 1), {1: ("f32_std_pixmajor", 1), 2: ("f32_std", 2)}, tables=0),
    # 512 filters, 683 boards of 8x8: conv3 fills the chip with 256 x 256 tiles (97 x 2 >= 192 blocks); no slabs above 512 boards: conv4, fc1, fc2 unsplit GmStd
    _case("f32-big", "f32", 8, 512, 683, (683, 611, 1), {1: ("lut_xcd", 1), 2: ("f32_big", 1), 3: ("f32_std", 1), 4: ("f32_std", 1), 5: ("f32_std", 1)}),
    # max_batch <= 32 at 512 filters: the gather computes its pattern ids inline
    _case("f32-inline-ids", "f32", 6, 512, 8, (8, 7, 1), {1: ("lut_xcd_inline", 1), 2: ("f32_std", 16)}),
    # ---- f16x2
    _case("h2-small2", "f16x2", 8, 256, 8, (8, 7, 1), {1: ("lut", 1), 2: ("h2_small2", 16), 3: ("h2_small2", 16), 4: ("h2_small2", 16), 5: ("h2_thin2", 8)}),
    _case("h2-lowpp1", "f16x2", 8, 256, 128, (128, 101, 1), {1: ("lut", 1), 2: ("h2_lowpp1", 8), 3: ("h2_lowpp1", 8), 4: ("h2_lowpp1", 16), 5: ("h2_thin", 8)}),
    _case("h2-lowpp", "f16x2", 8, 256, 128, (128, 101, 1), {2: ("h2_lowpp", 8), 3: ("h2_lowpp", 8), 4: ("h2_lowpp", 16)}, low_loop_phases=2),
    _case("h2-midpp", "f16x2", 8, 256, 128, (128, 101, 1), {2: ("h2_midpp", 8)}, conv3_tile=192),
    _case("h2-bigpp", "f16x2", 8, 256, 128, (128, 101, 1), {1: ("h2_bigpp", 8), 2: ("h2_bigpp", 8)}, conv3_tile=256, tables=0),
    _case("h2-bigpp-lut", "f16x2", 8, 256, 128, (128, 101, 1), {1: ("h2_bigpp_lut", 8)}, tables=1),
    _case("h2-simple-loop", "f16x2", 8, 256, 128, (128, 101, 1), {1: ("h2_big", 8), 2: ("h2_mid", 8), 3: ("h2_big", 8), 4: ("h2_small", 16)}, simple_loop=1, tables=0),
    # 6x6 at 1024 boards: conv3 on the 256-row tile (16 whole boards), fc1 on H2BigPP with four slices (max_batch >= 1024, call >= 1024), fc2 unsplit on H2Thin4w
    _case("h2-fc1-bigpp", "f16x2", 6, 256, 1024, (1024, 947, 1), {2: ("h2_bigpp", 4), 3: ("h2_lowpp1", 8), 4: ("h2_bigpp", 4), 5: ("h2_thin4w", 1)}),
    # ---- bf16x3
    _case("b3-k4-k8", "bf16x3", 8, 256, 192, (192, 157, 1), {1: ("lut", 1), 2: ("b3", 4), 3: ("b3", 8), 4: ("b3", 8), 5: ("b3", 4)}),
    _case("b3-conv2-gemm", "bf16x3", 8, 256, 192, (192, 157, 1), {1: ("b3", 2)}, tables=0),
    _case("b3-k1-k2", "bf16x3", 8, 512, 384, (384, 317, 1), {1: ("lut_xcd", 1), 2: ("b3", 1), 3: ("b3", 2), 4: ("b3", 8), 5: ("b3", 4)}),
    _case("b3-big", "bf16x3", 8, 512, 384, (384, 317, 1), {2: ("b3_big", 1)}, b3_tile=256),
]
# ---- widths other than 256 and 512: the same kernels under other index arithmetic -- 384 filters (f32: three 128-column tiles, never the 256 x 256
# tile) and 768 (the split precisions: three 256-column tiles, 216 k-tiles per 3x3 layer, fc1 with K = 12288 on 8x8), one case at 1024 (four column
# tiles).  Capacities as above: the smallest at which the launcher's own condition selects the configuration at THAT width.
WIDTH_CASES = [
    # ---- f32, 384 filters
    # the weight streams: kb must divide Cin = 384 -- 256 does not, 128 leaves 3 x 27 = 81 blocks, so the loop ends on 64 (54 slices of conv3 / conv4)
    _case("f32-c384-skinny", "f32", 6, 384, 4, (4, 3, 1), {1: ("lut", 1), 2: ("f32_skinny", 54), 3: ("f32_skinny", 54), 4: ("f32_skinny", 24), 5: ("f32_skinny", 16)}),
    # GmStd with the k loop split + k_splitk_reduce_f32: 108 k-tiles; conv4's eight slices do not divide them (13.5 each).  The generic gather at 384
    _case("f32-c384-splitk", "f32", 8, 384, 96, (96, 85, 1), {1: ("lut", 1), 2: ("f32_std", 4), 3: ("f32_std", 8), 4: ("f32_std", 16), 5: ("f32_std", 4)}),
    _case("f32-c384-pixmajor", "f32", 8, 384, 256, (256, 203, 1), {1: ("f32_std_pixmajor", 1), 2: ("f32_std", 2), 3: ("f32_std", 4)}, tables=0),
    # 1359 boards: conv3's 48924 rows are 192 tiles of 256 rows, where 256 and 512 filters move to the 256 x 256 tile; N % 256 keeps 384 on GmStd, unsplit
    _case("f32-c384-unsplit", "f32", 8, 384, 1359, (1359, 1201, 1), {1: ("lut", 1), 2: ("f32_std", 1), 3: ("f32_std", 1), 4: ("f32_std", 1), 5: ("f32_std", 1)}),
    # ---- f16x2, 768 filters
    # the small-capacity tiles: 16 slices of 216 k-tiles (13.5 each); fc1 with K = 12288
    _case("h2-c768-small2", "f16x2", 8, 768, 8, (8, 7, 1), {1: ("lut", 1), 2: ("h2_small2", 16), 3: ("h2_small2", 16), 4: ("h2_small2", 16), 5: ("h2_thin2", 8)}),
    # capacity 128: conv_ksplit with three column tiles stops at 4 slices (72 x 3 blocks want 8 at 256 filters)
    _case("h2-c768-lowpp1", "f16x2", 8, 768, 128, (128, 101, 1), {1: ("lut", 1), 2: ("h2_lowpp1", 4), 3: ("h2_lowpp1", 4), 4: ("h2_lowpp1", 16), 5: ("h2_thin", 8)}),
    _case("h2-c768-lowpp", "f16x2", 8, 768, 128, (128, 101, 1), {2: ("h2_lowpp", 4), 3: ("h2_lowpp", 4), 4: ("h2_lowpp", 16)}, low_loop_phases=2),
    _case("h2-c768-midpp", "f16x2", 8, 768, 128, (128, 101, 1), {2: ("h2_midpp", 4)}, conv3_tile=192),
    # ---- bf16x3, 768 filters (capacity >= B3_MIN_BATCH: k_gemm_b3 runs)
    _case("b3-c768-split", "bf16x3", 8, 768, 128, (128, 101, 1), {1: ("lut", 1), 2: ("b3", 2), 3: ("b3", 4), 4: ("b3", 8), 5: ("b3", 4)}),
    # conv_b3_ksplit stops splitting conv3 where ceil(36 mb / 128) x 3 >= 192 blocks: 64 row tiles, 225 boards (224 boards are 63 tiles)
    _case("b3-c768-unsplit", "bf16x3", 8, 768, 225, (225, 187, 1), {1: ("lut", 1), 2: ("b3", 1), 3: ("b3", 4), 4: ("b3", 8), 5: ("b3", 4)}),
    _case("b3-c768-conv2-gemm", "bf16x3", 8, 768, 225, (225, 187, 1), {1: ("b3", 1)}, tables=0),
    _case("b3-c768-big", "bf16x3", 8, 768, 225, (225, 187, 1), {2: ("b3_big", 1)}, b3_tile=256),
    # ---- 1024 filters, 6x6 (the weights stay at 126 MB): four column tiles, 288 k-tiles
    _case("h2-c1024-6x6", "f16x2", 6, 1024, 128, (128, 101, 1), {1: ("lut", 1), 2: ("h2_bigpp", 8), 3: ("h2_lowpp1", 8), 4: ("h2_lowpp1", 16), 5: ("h2_thin", 8)}),
]
CASES += WIDTH_CASES
CASE_BY_NAME = {c["name"]: c for c in CASES}


def config_ids(precision, C, layer, p, count):
    """the configurations of the issue's list that plan entry `p` of `layer` stands for"""
    k, ks = p["kernel"], p["kslices"]
    ids = set()
    if precision == "f32":
        ids.add({"f32_skinny": "f32:skinny", "f32_std": "f32:std_splitk" if ks > 1 else "f32:std_unsplit", "f32_std_pixmajor": "f32:std_pixmajor",
                 "f32_big": "f32:big", "lut": "f32:gather", "lut_xcd": "f32:gather_xcd", "lut_xcd_inline": "f32:gather_xcd_inline_ids"}[k])
        if ks > 1:
            ids.add("f32:fc2_reduce_by_heads" if layer == 5 else "f32:splitk_reduce_f32")
    elif precision == "f16x2":
        ids.add("f16x2:gather" if k.startswith("lut") else "f16x2:" + k)
        if layer == 4 and k == "h2_bigpp" and ks == 4 and count >= 1024:
            ids.add("f16x2:fc1_bigpp_4_slices")
        if ks > 1:
            ids.add("f16x2:fc2_reduce_by_heads" if layer == 5 else "f16x2:splitk_reduce_h2")
    else:
        if k.startswith("lut"):
            ids.add(f"bf16x3:gather_c{C}")
        else:
            ids.add("bf16x3:b3_big" if k == "b3_big" else f"bf16x3:b3_k{ks}")
            if layer == 1:
                ids.add("bf16x3:conv2_gemm")
            if layer == 4 and ks > 1:
                ids.add("bf16x3:fc1_split")
            if layer == 5 and ks == 4:
                ids.add("bf16x3:fc2_4_slices_by_heads")
            if ks > 1 and layer < 5:
                ids.add("bf16x3:splitk_reduce_b3")
    return ids


REQUIRED = {
    "f32:skinny", "f32:std_unsplit", "f32:std_splitk", "f32:splitk_reduce_f32", "f32:std_pixmajor", "f32:big", "f32:fc2_reduce_by_heads",
    "f32:gather", "f32:gather_xcd", "f32:gather_xcd_inline_ids",
    "f16x2:h2_small2", "f16x2:h2_small", "f16x2:h2_bigpp", "f16x2:h2_bigpp_lut", "f16x2:h2_midpp", "f16x2:h2_lowpp1", "f16x2:h2_lowpp", "f16x2:h2_big",
    "f16x2:h2_mid", "f16x2:fc1_bigpp_4_slices", "f16x2:h2_thin2", "f16x2:h2_thin", "f16x2:h2_thin4w", "f16x2:splitk_reduce_h2",
    "f16x2:gather", "f16x2:fc2_reduce_by_heads",      # not named by the list, run by every default f16x2 case: the gather writing h2 rows, fc2's slices left to the heads
    "bf16x3:b3_k1", "bf16x3:b3_k2", "bf16x3:b3_k4", "bf16x3:b3_k8", "bf16x3:splitk_reduce_b3", "bf16x3:b3_big", "bf16x3:conv2_gemm", "bf16x3:fc1_split",
    "bf16x3:fc2_4_slices_by_heads", "bf16x3:gather_c256", "bf16x3:gather_c512", "bf16x3:gather_c768",
}


def width_ids(precision, C, layer, p):
    """the width tag of a configuration: (precision, kernel, filters) of conv2 .. fc1 -- the layers whose N or K is the filter count (fc2 is 1024 x 512
    at every width)"""
    return {(precision, p["kernel"], C)} if layer <= 4 else set()


# every (precision, kernel) the WIDTH_CASES exist for, at its width: required like REQUIRED, no more, no fewer
REQUIRED_WIDTHS = {
    ("f32", "lut", 384), ("f32", "f32_skinny", 384), ("f32", "f32_std", 384), ("f32", "f32_std_pixmajor", 384),
    ("f16x2", "lut", 768), ("f16x2", "h2_small2", 768), ("f16x2", "h2_lowpp1", 768), ("f16x2", "h2_lowpp", 768), ("f16x2", "h2_midpp", 768),
    ("bf16x3", "lut", 768), ("bf16x3", "b3", 768), ("bf16x3", "b3_big", 768),
    ("f16x2", "lut", 1024), ("f16x2", "h2_bigpp", 1024), ("f16x2", "h2_lowpp1", 1024),
}
BASE_WIDTHS = (256, 512)            # the widths of the cases above WIDTH_CASES

_results = {}


def run_case(oz, case):
    """every (network kind, call size, layer) of a case, measured once per session: list of dict(kind, count, layer, err, e32, plan)"""
    name = case["name"]
    if name not in _results:
        rows, t0 = [], time.perf_counter()
        n, C, mb, precision = case["n"], case["C"], case["mb"], case["precision"]
        for kind in ("sparse", "dense"):
            net = _net(oz, precision, n, C, mb, kind)
            assert net.arithmetic() == precision
            _apply(oz, net, case["setup"])
            try:
                # full capacity first -- networks of fewer than 64 boards several times, on fresh boards, so that the case's norm rests on >= 64 boards
                calls = [(case["sizes"][0], i * mb) for i in range(_full_calls(mb))] + [(count, 0) for count in case["sizes"][1:]]
                done = []
                for count, first in calls:
                    own, opp = _boards(n, count, first)
                    res, plan = measure(oz, net, R.network_weights(n, C, kind), n, C, own, opp)
                    done.append((count, res, plan))
            finally:
                _apply(oz, net, {})
            for r in evaluate(done):
                r["kind"] = kind
                rows.append(r)
                print(_line(precision, name, r))
        print(f"layer-parity {precision:7s} {name:16s} {C} filters, capacity {mb}: {time.perf_counter() - t0:.2f} s (networks built and committed on first use)")
        _results[name] = rows
    return _results[name]


def _full_calls(mb):
    return max(1, min(16, -(-64 // mb)))


def _line(precision, name, r):
    p = r["plan"]
    return (f"layer-parity {precision:7s} {name:16s} layer {r['layer']} {r['kind']:6s} count {r['count']:5d} {p['kernel']:16s} rows {p['tile_rows']:3d} slices {p['kslices']:3d}  "
            f"err {r['err']:.3e}  E32 {r['e32']:.3e}  ratio {r['err'] / r['e32']:6.2f}  (own-rows norm {r['own']:6.2f})")


def check_rows(rows, precision):
    bad = [(r["kind"], r["count"], r["layer"], r["plan"]["kernel"], round(r["err"] / r["e32"], 2)) for r in rows
           if not r["err"] <= (R.MARGIN[precision] if r["kind"] == "sparse" else R.MARGIN_DENSE) * r["e32"]]
    assert not bad, f"(kind, count, layer, kernel, err / E32) above the margin ({R.MARGIN[precision]} sparse, {R.MARGIN_DENSE} dense): {bad}"


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_layer_parity(oz, name):
    case = CASE_BY_NAME[name]
    rows = run_case(oz, case)
    # the plan proves that the case ran the kernels it names (at full capacity, on both networks)
    for layer, (kernel, kslices) in case["expect"].items():
        for r in rows:
            if r["layer"] == layer and r["count"] == case["sizes"][0]:
                assert (r["plan"]["kernel"], r["plan"]["kslices"]) == (kernel, kslices), (layer, r["plan"])
    assert len(rows) == 2 * (_full_calls(case["mb"]) + len(case["sizes"]) - 1) * 5
    check_rows(rows, case["precision"])


def test_activation_view_arguments(oz):
    """the hook's refusals: rows outside the last call, a stub network, a layer that was never materialised, no forward since the commit"""
    from othellozero_amd.NNet import StubNetWrapper
    net = _net(oz, "f32", 6, 256, 4, "dense")
    own, opp = _boards(6, 3)
    net.commit()
    with pytest.raises(oz.OzError) as e:
        net.activation(2, 0, 1)
    assert e.value.code == oz.OZ_ERR_STATE
    net.predict_batch(own, opp)
    assert net.activation(2).shape == (3 * 16, 256) and net.activation(5, 2, 1).shape == (1, 512)
    for layer, first, rows in ((2, 0, 3 * 16 + 1), (2, 3 * 16, 1), (2, -1, 2), (5, 3, 1), (6, 0, 1), (2, 0, 0)):
        with pytest.raises(oz.OzError) as e:
            net.activation(layer, first, rows) if layer < 6 else oz.check(oz.load().oz_net_get_activation(net._h, 6, 0, 1, oz.p_f64(np.zeros(8))))
        assert e.value.code == oz.OZ_ERR_ARG, (layer, first, rows)
    with pytest.raises(oz.OzError) as e:
        net.activation(0, 0, 1)                                  # conv1 is folded into the tables
    assert e.value.code == oz.OZ_ERR_STATE
    stub = StubNetWrapper((6, 6), 1, 0, max_batch=4)
    stub.predict_batch(own, opp)
    with pytest.raises(oz.OzError) as e:
        oz.check(oz.load().oz_net_get_activation(stub._h, 2, 0, 1, oz.p_f64(np.zeros(256))))
    assert e.value.code == oz.OZ_ERR_ARG
    # reading changes nothing: the same call again gives the same bits, and so does the next forward
    pi, v = net.predict_batch(own, opp)
    a = net.activation(4)
    assert np.array_equal(a, net.activation(4))
    pi2, v2 = net.predict_batch(own, opp)
    assert np.array_equal(pi, pi2) and np.array_equal(v, v2)


# ------------------------------------------------------------------ the two launch-plan switches without a test
def _bits(net, own, opp, layers=()):
    pi, v = net.predict_batch(own, opp)
    return [pi.copy(), v.copy()] + [net.activation(layer) for layer in layers]


def test_low_loop_phases_bit_identical(oz):
    """OZ_NET_OPT_LOW_LOOP_PHASES 1 (the default one-phase loop of the 128 x 256 tile) against 2: bit-identical (pi, v) and bit-identical outputs of
    conv3, conv4 and fc1, at call sizes on either side of conv3's tile choice (512: 192-row tile; 430 and 37: the 128-row tile)"""
    net = _net(oz, "f16x2", 8, 512, 512, "dense")
    try:
        for count in (512, 430, 37):
            own, opp = _boards(8, count)
            got = {}
            for phases in (1, 2):
                net.set_option(oz.NET_OPT_LOW_LOOP_PHASES, phases)
                got[phases] = _bits(net, own, opp, (2, 3, 4))
                plan = net.layer_plan()
                low = "h2_lowpp1" if phases == 1 else "h2_lowpp"
                assert plan[3]["kernel"] == low and plan[4]["kernel"] == low, plan
                assert plan[2]["kernel"] == ("h2_midpp" if count == 512 else low), plan
            for a, b in zip(got[1], got[2]):
                assert a.shape == b.shape and np.array_equal(a, b), count
    finally:
        net.set_option(oz.NET_OPT_LOW_LOOP_PHASES, 1)


def test_latency_splits(oz):
    """OZ_NET_OPT_LATENCY_SPLITS 0 against 1 (max_batch 512, 512 filters): the plan reports another conv3 split; both networks satisfy the per-layer
    bounds; they agree on (pi, v) within 4e-6, the bound the suite uses between two fp32-class roundings; with the option on, a position's bits do not
    depend on the size of the call (512 vs 15 vs 1)"""
    from othellozero_amd.NNet import NNetWrapper
    own, opp = _boards(8, 512)
    outs, splits = {}, {}
    for kind in ("sparse", "dense"):
        w = R.network_weights(8, 512, kind)
        base = _net(oz, "f16x2", 8, 512, 512, kind)
        lat = NNetWrapper((8, 8), num_channels_1=512, max_batch=512, weights=R.network_weights(8, 512, "dense"), precision="f16x2")
        lat.set_option(oz.NET_OPT_LATENCY_SPLITS, 1)
        try:
            lat.set_weights(w)
        except oz.OzError as e:                                     # a refusal for a stated conditioning reason: measure only (see _net)
            assert e.code == oz.OZ_ERR_STATE, e
            lat.set_option(oz.NET_OPT_SELF_CHECK, 2)
            lat.set_weights(w)
        for tag, net in (("base", base), ("latency", lat)):
            res, plan = measure(oz, net, w, 8, 512, own, opp)
            splits[kind, tag] = plan[2]["kslices"]
            rows = evaluate([(512, res, plan)])
            for r in rows:
                r["kind"] = kind
                print(_line("f16x2", "latency-" + tag, r))
            check_rows(rows, "f16x2")
            outs[kind, tag] = net.predict_batch(own, opp)
        assert splits[kind, "base"] != splits[kind, "latency"], splits
        if kind == "dense":
            (pa, va), (pb, vb) = outs[kind, "base"], outs[kind, "latency"]
            assert np.abs(pa - pb).max() <= 4e-6 and np.abs(va - vb).max() <= 4e-6
            pi, v = outs[kind, "latency"]
            for count in (15, 1):
                p2, v2 = lat.predict_batch(own[:count], opp[:count])
                assert np.array_equal(p2, pi[:count]) and np.array_equal(v2, v[:count]), count


def test_every_configuration_ran(oz):
    """the union of the cases runs every configuration of the list, as reported by layer_plan() -- no more, no fewer"""
    seen, widths = set(), set()
    for case in CASES:
        for r in run_case(oz, case):
            seen |= config_ids(case["precision"], case["C"], r["layer"], r["plan"], r["count"])
            widths |= width_ids(case["precision"], case["C"], r["layer"], r["plan"])
    assert seen == REQUIRED, f"missing {sorted(REQUIRED - seen)}, not in the list {sorted(seen - REQUIRED)}"
    # ... and the widths outside 256 / 512: every (precision, kernel, filters) of REQUIRED_WIDTHS, required and not merely tolerated
    widths = {w for w in widths if w[2] not in BASE_WIDTHS}
    assert widths == REQUIRED_WIDTHS, f"missing {sorted(REQUIRED_WIDTHS - widths)}, not in the list {sorted(widths - REQUIRED_WIDTHS)}"


def _row_tiles(case, r):
    """row tiles of the launch that produced row r: the call's boards x output pixels over the plan's tile rows (pixel-major tiles hold one pixel of
    128 consecutive boards each)"""
    pix = R.layer_geometry(case["n"], case["C"], r["layer"])[1] ** 2
    T = r["plan"]["tile_rows"]
    return -(-r["count"] // T) * pix if r["plan"]["kernel"] == "f32_std_pixmajor" else -(-r["count"] * pix // T)


def test_both_block_mappings_ran_at_an_odd_column_tile_count(oz):
    """k_gemm_h2, k_gemm_b3 and k_gemm_b3_big map a block to (row tile, column tile, k-slice) in two ways: launches of fewer than 8 row tiles send
    the blocks of one row tile round the XCDs (q = (jb / num_mt) * 8 + xcd, blocks with q >= per_mt return), the others send the row tiles round
    (mt = (jb / per_mt) * 8 + xcd).  Read from the plan's tile rows and the call's rows, not from the case list: at 768 filters -- three column tiles,
    per_mt = 3 x k-slices -- each family ran both, the one-board call the first and the full call the second; likewise k_gemm_f32 at 384 filters, whose
    grid pads the row tiles to a multiple of 8.  And a k split that does not divide the k-tiles ran in f32 and f16x2 (bf16x3's are in the trainer matrix)"""
    family = lambda k: "h2" if k.startswith("h2_") else k if k in ("b3", "b3_big") else "f32" if k.startswith("f32_std") else None
    ran, ragged = set(), set()
    for case in WIDTH_CASES:
        C = case["C"]
        for r in run_case(oz, case):
            fam = family(r["plan"]["kernel"])
            if fam is None or r["layer"] > 3:
                continue
            ran.add((fam, C, _row_tiles(case, r) >= 8))
            if (9 * C // 32) % r["plan"]["kslices"]:
                ragged.add(fam)
    for fam, C, column_tile in (("h2", 768, 256), ("b3", 768, 256), ("b3_big", 768, 256), ("f32", 384, 128)):
        assert (C // column_tile) % 2 == 1
        assert {(fam, C, False), (fam, C, True)} <= ran, (fam, C, sorted(ran))
    assert {"f32", "h2"} <= ragged, ragged
