"""The network forward with fewer live rows than it was launched for -- the regime every search runs it in (pytest -m gpu).

A search calls the forward with a FIXED launch size (its games, games x leaves, or the batch cap: the grid and the tile plan come from it) and a live
count on the device that moves between 0 and that size from step to step.  oz_net_predict always launches exactly the boards it is given, so the
direct network tests never cut a tile of the capacity's plan in the middle, never leave whole tiles empty, never run fc1's 256-row tile or the
16-position heads block with a handful of rows.  oz_net_forward_launched (NNetWrapper.forward_launched) launches `launch` boards with `count` live,
and this file holds every tile / split-K / reduce / main-loop configuration of test_gpu_layer_parity.REQUIRED to the contract written above
oz_net_forward_device (oz_internal.h):

  plan    the plan of a short launch is the plan of the full one (layer_plan()), and the configurations seen here are exactly REQUIRED;
  bits    rows [0, count) of (pi, v) and the layers' activations equal, bit for bit, what predict_batch of those boards alone gives -- the header's
          "a position's (pi, v) does not depend on the size of the call" makes the tested count == launch path an exact reference;
  beyond  rows [count, launch) of (pi, v) come back byte for byte (the searches keep evaluation-cache hits there);
  state   a short call leaves nothing behind that changes the next full one;
  guards  the f16x2 range guards see live rows only, and still see those.

The counts of a case are derived from its plan (tests/short_batch_ref.py: 0, 1, launch - 1, and per GEMM layer a count that cuts a tile with whole
empty tiles behind it and one that ends on a tile edge; below / at / above the boundary of a bf16x3 mixed plan).  Dense networks only."""
import time

import numpy as np
import pytest

import layer_ref as R
import short_batch_ref as S
import test_gpu_layer_parity as LP
from test_gpu_layer_parity import CASE_BY_NAME, REQUIRED, WIDTH_CASES, _apply, _boards, _net, config_ids

# the layer matrix at 256 / 512 filters, and of its other widths one f32 case at 384 and one bf16x3 case at 768 filters: the dead rows behind a short
# count sit at other strides there (three column tiles; slabs of 384 / 768 floats a row)
SHORT_WIDTH_CASES = ("f32-c384-splitk", "b3-c768-split")
CASES = [c for c in LP.CASES if c not in WIDTH_CASES] + [CASE_BY_NAME[name] for name in SHORT_WIDTH_CASES]

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FD5A5A5               # a quiet NaN with a payload: no kernel produces it, and a float copy that went through arithmetic would canonicalise it
HEADS_P, HEADS_LP_MIN = 8, 3072     # launch_heads (oz_net.hip): launch >= 3072 -> k_heads_t<16>; launch > HEADS_P -> k_heads_t<4>; else k_heads_t<HEADS_P>


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    yield _lib
    LP._nets.clear()


def _nan(shape):
    return np.full(shape, NAN_BITS, np.uint32).view(np.float32)


def _pixels(n):
    return {0: n * n, 1: n * n, 2: (n - 2) ** 2, 3: (n - 4) ** 2, 4: 1, 5: 1}


def _merge(iv):
    out = []
    for lo, hi in sorted(iv):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def compared_rows(count, pixels, plan_entry):
    """row intervals [lo, hi) of a layer's output that are compared: every row of boards 0 and count - 1, every live row of the last live tile of
    the LAUNCH's plan (the gather has no tiles: 256 rows), and layer_ref.sample_runs"""
    live, T = count * pixels, plan_entry["tile_rows"] if plan_entry else 0
    iv = [(0, pixels), (live - pixels, live)]
    if plan_entry and plan_entry["kernel"] == "f32_std_pixmajor":
        iv.append(((count - 1) // T * T * pixels, live))        # one pixel of T consecutive boards per tile: the last board group, every pixel
    else:
        T = T if T > 0 else 256
        iv.append(((live - 1) // T * T, live))
    iv += [(b0 * pixels, (b0 + nb) * pixels) for b0, nb in R.sample_runs(count, pixels)]
    return _merge(iv)


def _materialised(oz, net, layer):
    try:
        net.activation(layer, 0, 1)
        return True
    except oz.OzError as e:
        assert e.code == oz.OZ_ERR_STATE, e
        return False


def _read(oz, net, n, live_boards, plan):
    """{layer: [(lo, rows as float64)]} of the last forward, layers 0 .. 5 where materialised"""
    out = {}
    for layer in range(6):
        if layer == 0 and not _materialised(oz, net, 0):
            continue
        px = _pixels(n)[layer]
        out[layer] = [(lo, net.activation(layer, lo, hi - lo)) for lo, hi in compared_rows(live_boards, px, plan.get(layer))]
    return out


def short_call(oz, net, n, own_L, opp_L, count, plan_L, rows_per_board=1, tag=""):
    """checks 3 and 4 of one (launch, count): predict_batch of the live boards alone, then the launch of all the boards with `count` live into
    NaN-filled (pi, v).  rows_per_board: 8 under the "mean" evaluation symmetry (the forward then sees 8 rows per position)"""
    L = own_L.size
    if count:
        pa, va = net.predict_batch(own_L[:count], opp_L[:count])
        acts_a = _read(oz, net, n, count * rows_per_board, plan_L)
    pb, vb = net.forward_launched(own_L, opp_L, count, _nan((L, n, n)), _nan((L,)))
    assert net.layer_plan() == plan_L, (tag, count, net.layer_plan(), plan_L)                               # 1: the plan of the launch, not of the count
    assert pb[count:].tobytes() == _nan((L - count, n, n)).tobytes(), (tag, count, "pi rows beyond the count were written")     # 4
    assert vb[count:].tobytes() == _nan((L - count,)).tobytes(), (tag, count, "v rows beyond the count were written")
    if count:
        assert np.array_equal(pb[:count], pa) and np.array_equal(vb[:count], va), (tag, count, "live (pi, v) rows differ from predict_batch's")     # 3
        assert np.all(np.isfinite(pa)) and np.all(np.isfinite(va))
        acts_b = _read(oz, net, n, count * rows_per_board, plan_L)
        assert set(acts_a) == set(acts_b) and {1, 2, 3, 4, 5} <= set(acts_b), (tag, count, sorted(acts_a), sorted(acts_b))
        for layer, runs in acts_b.items():
            for (lo, b), (lo_a, a) in zip(runs, acts_a[layer]):
                assert lo == lo_a and a.shape == b.shape and np.array_equal(a, b), (tag, count, f"layer {layer} rows from {lo} differ")
            assert any(np.abs(b).max() > 0 for _, b in runs), (tag, count, layer)
    return pb, vb


# ------------------------------------------------------------------ every configuration of the layer matrix, short
_seen = {}                          # case name -> set of config ids that ran with count < launch
_wall = {}


def _launch_boards(n, L):
    return _boards(n, L)


def run_case(oz, name):
    """every count of one case of the layer matrix, once per session -> the configuration ids that ran with count < launch"""
    if name in _seen:
        return _seen[name]
    case = CASE_BY_NAME[name]
    n, C, L, precision = case["n"], case["C"], case["mb"], case["precision"]
    t0 = time.perf_counter()
    net = _net(oz, precision, n, C, L, "dense")
    _apply(oz, net, case["setup"])
    try:
        own_L, opp_L = _launch_boards(n, L)
        # the full launch: the plan the case names, the same bits as the tested path
        p_full, v_full = net.forward_launched(own_L, opp_L, L)
        plan_L = net.layer_plan()
        for layer, (kernel, kslices) in case["expect"].items():
            assert (plan_L[layer]["kernel"], plan_L[layer]["kslices"]) == (kernel, kslices), (layer, plan_L[layer])
        pp, vp = net.predict_batch(own_L, opp_L)
        assert net.layer_plan() == plan_L and np.array_equal(pp, p_full) and np.array_equal(vp, v_full)
        counts, why = S.counts_of_plan(plan_L, _pixels(n), L)
        assert {0, 1, L - 1} <= set(counts)
        ids = set()
        for count in counts:
            short_call(oz, net, n, own_L, opp_L, count, plan_L, tag=name)
            for layer in range(1, 6):
                ids |= config_ids(precision, C, layer, plan_L[layer], L)        # (the launch size decides the configuration: fc1's 256-row tile needs >= 1024)
        _seen[name] = ids
        _wall[name] = (time.perf_counter() - t0, len(counts))
        print(f"short-batches {precision:7s} {name:16s} launch {L:5d} counts " + " ".join(f"{c}[{','.join(why[c])}]" for c in counts) + f"  {_wall[name][0]:.2f} s")
    finally:
        _apply(oz, net, {})
    return _seen[name]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_short_counts(oz, name):
    assert run_case(oz, name)


# ------------------------------------------------------------------ the bf16x3 mixed plan, boundary forced into the 192-board network
@pytest.mark.parametrize("mix", [256, 512])
def test_short_counts_on_the_mixed_plan(oz, mix):
    """conv3 (36 rows per board) and conv4 (16) of the bf16x3 network of 192 boards with their first `mix` rows on 256-row tiles: counts below, at
    (conv4: 16 / 32 boards; conv3's boundary falls inside a board) and above the boundary, and the tile classes of both launches"""
    n, C, L = 8, 256, 192
    net = _net(oz, "bf16x3", n, C, L, "dense")
    _apply(oz, net, {})
    net.set_option(oz.NET_OPT_B3_MIX_ROWS, mix)
    try:
        own_L, opp_L = _launch_boards(n, L)
        net.forward_launched(own_L, opp_L, L)
        plan_L = net.layer_plan()
        for layer in (2, 3):
            assert plan_L[layer]["kernel"] == "b3_mixed" and plan_L[layer]["big_rows"] == mix and plan_L[layer]["tile_rows"] == 128, plan_L[layer]
        counts, why = S.counts_of_plan(plan_L, _pixels(n), L)
        reasons = {r for rs in why.values() for r in rs}
        assert {"layer2:below", "layer2:above", "layer3:below", "layer3:at", "layer3:above"} <= reasons, reasons
        for count in counts:
            short_call(oz, net, n, own_L, opp_L, count, plan_L, tag=f"mixed-{mix}")
        print(f"short-batches bf16x3  mixed-{mix} launch {L} counts " + " ".join(f"{c}[{','.join(why[c])}]" for c in counts))
    finally:
        net.set_option(oz.NET_OPT_B3_MIX_ROWS, 0)


# ------------------------------------------------------------------ 5: a short call leaves nothing behind
@pytest.mark.parametrize("tables", [-1, 0])
@pytest.mark.parametrize("precision,n,C,L", [("f32", 8, 256, 256), ("f16x2", 8, 256, 128), ("bf16x3", 8, 256, 192)])
def test_a_short_call_leaves_no_state(oz, precision, n, C, L, tables):
    net = _net(oz, precision, n, C, L, "dense")
    _apply(oz, net, {"tables": tables})
    try:
        own_L, opp_L = _launch_boards(n, L)
        other_own, other_opp = _boards(n, L, first=L)
        p1, v1 = net.forward_launched(own_L, opp_L, L, _nan((L, n, n)), _nan((L,)))
        assert np.all(np.isfinite(p1)) and np.all(np.isfinite(v1))
        net.forward_launched(other_own, other_opp, L // 2 + 1, _nan((L, n, n)), _nan((L,)))
        net.forward_launched(other_own, other_opp, 0)
        p2, v2 = net.forward_launched(own_L, opp_L, L, _nan((L, n, n)), _nan((L,)))
        assert np.array_equal(p1, p2) and np.array_equal(v1, v2)
    finally:
        _apply(oz, net, {})


# ------------------------------------------------------------------ 6: the f16x2 guards
@pytest.mark.parametrize("n,mb", [(8, 64), (8, 4), (6, 1024)])
def test_f16x2_guards_see_live_rows_only(oz, n, mb):
    """mb 64: the guards of the tile epilogues; mb 4: those of the latency path's reduces.  POISON: a full-capacity forward under calibration maxima
    at 2^18 raises "fp16 range" (a reported error) and leaves above-range values in every row of the activation buffers and k-slice slabs; with the
    option restored, short launches over those buffers must return OK with the bits of a fresh network.  CONVERSE: with every row "low", no live row
    raises nothing and one live row still raises.
    mb 1024 (6x6): the restoring commit calibrates on 512 positions in calls of max_batch, so in the two small networks its own forwards rewrite every
    row of every buffer before the short launch runs; at 1024 boards rows 512 .. 1023 still hold what the poisoned forward left -- read back below --
    and the counts 1 and 513 leave them behind live rows"""
    from othellozero_amd.NNet import NNetWrapper
    C = 256
    w = R.network_weights(n, C, "dense")
    own_L, opp_L = _launch_boards(n, mb)
    fresh = NNetWrapper((n, n), num_channels_1=C, max_batch=mb, weights=w, precision="f16x2")
    net = NNetWrapper((n, n), num_channels_1=C, max_batch=mb, weights=w, precision="f16x2")
    net.set_option(oz.NET_OPT_ACT_TARGET_LOG2, 18)
    net.commit()
    with pytest.raises(oz.OzError) as ei:
        net.predict_batch(own_L, opp_L)
    assert ei.value.code == oz.OZ_ERR_STATE and "fp16 range" in str(ei.value)
    net.set_option(oz.NET_OPT_ACT_TARGET_LOG2, -2)
    net.commit()
    for count in (1, mb // 2 + 1):
        pb, vb = net.forward_launched(own_L, opp_L, count, _nan((mb, n, n)), _nan((mb,)))        # returns OK
        if mb > 512:
            # the stale rows are still above the range: conv3's output of the last board, as this forward's exponents decode it
            px = _pixels(n)[2]
            stale = net.activation(2, (mb - 1) * px, px)
            fresh.forward_launched(own_L, opp_L, mb)
            healthy = fresh.activation(2, (mb - 1) * px, px)
            print(f"short-batches guards mb {mb} count {count}: stale rows max {np.abs(stale).max():.3g} against {np.abs(healthy).max():.3g} of a healthy forward")
            assert not np.all(np.isfinite(stale)) or np.abs(stale).max() > 1024 * np.abs(healthy).max()
        pa, va = fresh.predict_batch(own_L[:count], opp_L[:count])
        assert np.array_equal(pb[:count], pa) and np.array_equal(vb[:count], va), count
        assert pb[count:].tobytes() == _nan((mb - count, n, n)).tobytes() and vb[count:].tobytes() == _nan((mb - count,)).tobytes()
    # converse
    net.set_option(oz.NET_OPT_LOW_GUARD_LOG2, 12)
    net.set_option(oz.NET_OPT_SELF_CHECK, 0)
    net.commit()
    net.forward_launched(own_L, opp_L, 0)                      # no live row: nothing to guard
    with pytest.raises(oz.OzError) as ei:
        net.forward_launched(own_L, opp_L, 1)
    assert ei.value.code == oz.OZ_ERR_STATE and "fell below" in str(ei.value)


# ------------------------------------------------------------------ 7: the heads' three instantiations
_heads_ran = set()                  # (instantiation, fc2 slices left to the heads?) that ran with count < launch
_heads_done = set()


def _heads_of(launch):
    return 16 if launch >= HEADS_LP_MIN else 4 if launch > HEADS_P else HEADS_P


# (precision, max_batch, launches).  6x6 at 256 filters.  bf16x3 leaves fc2's four slices to the heads at every size; f32 leaves them where its
# capacity splits k (max_batch <= 512) and writes fc2 itself at 3072
HEADS_RUNS = [("f32", 3072, (3072,)), ("f32", 24, (24, 9, 8)), ("bf16x3", 3072, (3072, 24, 9, 8))]


def run_heads(oz, precision, mb, launches):
    if (precision, mb) in _heads_done:
        return
    n, C = 6, 256
    net = _net(oz, precision, n, C, mb, "dense")
    _apply(oz, net, {})
    for L in launches:
        lp = _heads_of(L)
        own_L, opp_L = _launch_boards(n, min(L, 1536))
        if L > 1536:                                           # _boards holds 1536 positions: the launch repeats them
            own_L, opp_L = np.resize(own_L, L), np.resize(opp_L, L)
        net.forward_launched(own_L, opp_L, L)
        plan_L = net.layer_plan()
        deferred = plan_L[5]["kslices"] > 1
        # 0, 1, inside the first block, inside a later block with whole empty blocks behind, the last row missing
        counts = sorted({0, 1, lp - 1 if lp > 2 else 1, min(L - 1, (L // 2) // lp * lp + 1), L - 1})
        assert any(c % lp for c in counts)
        for count in counts:
            short_call(oz, net, n, own_L, opp_L, count, plan_L, tag=f"heads<{lp}>")
        _heads_ran.add((lp, deferred))
        print(f"short-batches heads<{lp}> {precision} launch {L} fc2 slices {plan_L[5]['kslices']} counts {counts}")
    _heads_done.add((precision, mb))


@pytest.mark.parametrize("precision,mb,launches", HEADS_RUNS)
def test_heads_short(oz, precision, mb, launches):
    run_heads(oz, precision, mb, launches)


# ------------------------------------------------------------------ 8: the evaluation symmetry and the stub network
@pytest.mark.parametrize("mode", ["random", "mean"])
def test_short_counts_under_the_evaluation_symmetry(oz, mode):
    """"random": k_sym_boards / k_sym_policy around the forward, bounded by the same count; "mean": the forward runs 8 * count live rows under a launch of
    8 * L, and k_sym_policy writes rows [0, count) only"""
    n, C, mb = 8, 256, 96
    net = _net(oz, "f32", n, C, mb, "dense")
    _apply(oz, net, {})
    L = mb if mode == "random" else mb // 8
    mult = 1 if mode == "random" else 8
    own_L, opp_L = _launch_boards(n, L)
    net.set_eval_symmetry(mode, 2024)
    try:
        net.forward_launched(own_L, opp_L, L)
        plan_L = net.layer_plan()
        counts, _ = S.counts_of_plan(plan_L, _pixels(n), L * mult)
        counts = sorted({0, 1, L - 1} | {c // mult for c in counts if 0 < c // mult < L})
        for count in counts:
            short_call(oz, net, n, own_L, opp_L, count, plan_L, rows_per_board=mult, tag=f"sym-{mode}")
        if mode == "mean":
            with pytest.raises(oz.OzError) as ei:              # 8 * launch beyond max_batch: refused, nothing launched
                net.forward_launched(*_launch_boards(n, L + 1), 1)
            assert ei.value.code == oz.OZ_ERR_ARG
    finally:
        net.set_eval_symmetry("off", 0)


def test_stub_network_and_arguments(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, L = 6, 40
    stub = StubNetWrapper((n, n), 3, 0, max_batch=L)
    own_L, opp_L = _launch_boards(n, L)
    pa, va = stub.predict_batch(own_L, opp_L)
    for count in (0, 1, 17, L - 1, L):
        pb, vb = stub.forward_launched(own_L, opp_L, count, _nan((L, n, n)), _nan((L,)))
        assert np.array_equal(pb[:count], pa[:count]) and np.array_equal(vb[:count], va[:count]), count
        assert pb[count:].tobytes() == _nan((L - count, n, n)).tobytes() and vb[count:].tobytes() == _nan((L - count,)).tobytes(), count
    # refusals: nothing is launched, (pi, v) come back as they went in
    net = _net(oz, "f32", 6, 256, 4, "dense")
    own4, opp4 = _launch_boards(6, 5)
    for own, opp, count in ((own4[:4], opp4[:4], 5), (own4[:4], opp4[:4], -1), (own4, opp4, 1), (own4[:0], opp4[:0], 0)):
        with pytest.raises(oz.OzError) as ei:
            net.forward_launched(own, opp, count)
        assert ei.value.code == oz.OZ_ERR_ARG, (own.size, count)
    assert oz.load().oz_version() == 230


# ------------------------------------------------------------------ last: what ran
def test_every_configuration_ran_short(oz):
    """every configuration of the layer file's list ran with count < launch -- no more, no fewer -- and so did the three heads instantiations, each
    with fc2's slices left to it, the 16-position one without them too"""
    seen = set()
    for case in CASES:
        seen |= run_case(oz, case["name"])
    for run in HEADS_RUNS:
        run_heads(oz, *run)
    assert seen == REQUIRED, f"missing {sorted(REQUIRED - seen)}, not in the list {sorted(seen - REQUIRED)}"
    assert all(name in _seen for name in SHORT_WIDTH_CASES)
    assert {(16, True), (16, False), (4, True), (HEADS_P, True)} <= _heads_ran, _heads_ran
    total = sum(t for t, _ in _wall.values())
    print(f"short-batches: {sum(k for _, k in _wall.values())} (launch, count) pairs of the matrix in {total:.1f} s")
