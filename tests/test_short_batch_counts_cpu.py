"""The count rule of the short-batch test (tests/short_batch_ref.py) yields every class of count, or says rightly that a class cannot exist.  No GPU.

Run over the (pixels, tile rows, capacity, big rows) tuples the GPU test meets: every full-capacity line of the committed table
profiles/layer_parity_ratios.txt (the plans of test_gpu_layer_parity's cases) and the plans of tests/test_b3_mix_plan_cpu.py.  Every answer is held
against a search over ALL counts below the capacity: a count that is returned has the property of its class, and None is returned only where no count
has it."""
import os
import re

import pytest

import layer_ref as R
import short_batch_ref as S
from test_gpu_layer_parity import CASE_BY_NAME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LINE = re.compile(r"^layer-parity\s+(\S+)\s+(\S+)\s+layer (\d) (\w+)\s+count\s+(\d+)\s+(\S+)\s+rows\s+(\d+)\s+slices\s+(\d+)")


def table_tuples():
    """(case, layer, kernel, pixels, tile rows, capacity) of every full-capacity line of the table, once each"""
    out = set()
    with open(os.path.join(ROOT, "profiles", "layer_parity_ratios.txt")) as f:
        for line in f:
            m = _LINE.match(line)
            if not m:
                continue
            _, name, layer, _, count, kernel, rows, _ = m.groups()
            case = CASE_BY_NAME.get(name)                     # (the table also holds the lines of test_latency_splits: no case of the matrix)
            if case is None or int(count) != case["mb"]:
                continue
            hout = R.layer_geometry(case["n"], case["C"], int(layer))[1]
            out.add((name, int(layer), kernel, hout * hout, int(rows), case["mb"]))
    return sorted(out)


def test_the_table_covers_every_case():
    seen = {t[0] for t in table_tuples()}
    assert seen == set(CASE_BY_NAME), sorted(set(CASE_BY_NAME) ^ seen)
    assert len(table_tuples()) >= 5 * len(CASE_BY_NAME) - 5


def _check_tiles(pixels, tile_rows, launch, tag):
    got = S.tile_counts(pixels, tile_rows, launch)
    cuts = [c for c in range(launch + 1) if tile_rows > 0 and S.is_cut(c, pixels, tile_rows, launch)]
    edges = [c for c in range(launch + 1) if tile_rows > 0 and S.is_edge(c, pixels, tile_rows, launch)]
    # the two predicates, restated: live rows, tiles that hold a live row, tiles of the launch
    for c in cuts:
        live, tiles = c * pixels, -(-launch * pixels // tile_rows)
        assert 0 < c < launch and live % tile_rows and live // tile_rows + 1 <= tiles - 1, (tag, c)
    for c in edges:
        assert 0 < c < launch and c * pixels >= tile_rows and c * pixels % tile_rows == 0, (tag, c)
    assert (got["cut"] in cuts) if cuts else got["cut"] is None, (tag, got)
    assert (got["edge"] in edges) if edges else got["edge"] is None, (tag, got)
    return got


def test_every_class_or_the_reason_on_the_table():
    missing = {}
    for name, layer, kernel, pixels, rows, cap in table_tuples():
        got = _check_tiles(S.layer_pixels(kernel, pixels), rows, cap, (name, layer))
        for cls, c in got.items():
            if c is None:
                missing[name, layer, cls] = (kernel, pixels, rows, cap)
    # which classes cannot exist, and why: the gather has no row tiles; a layer whose whole launch is ONE tile (the weight streams of four boards, the
    # dense layers of 8 / 96 / 128 boards on 128-row tiles, ...) has no tile behind the live rows and no tile edge below the capacity
    for (name, layer, cls), (kernel, pixels, rows, cap) in missing.items():
        px = S.layer_pixels(kernel, pixels)
        one_tile = rows > 0 and cap * px <= rows
        no_edge = rows > 0 and all((c * px) % rows for c in range(1, cap))
        no_cut = rows > 0 and all((c * px) % rows == 0 or -(-c * px // rows) == -(-cap * px // rows) for c in range(1, cap))
        assert rows == 0 or one_tile or (cls == "edge" and no_edge) or (cls == "cut" and no_cut), (name, layer, cls, kernel, pixels, rows, cap)
    # every GEMM case has at least one layer with a cut tile and whole empty tiles behind it, except the launches that are one tile in every layer
    for name, case in CASE_BY_NAME.items():
        layers = [t for t in table_tuples() if t[0] == name and t[4] > 0]
        if any(t[5] * S.layer_pixels(t[2], t[3]) > t[4] for t in layers):
            assert any((name, t[1], "cut") not in missing for t in layers), name


# the plans of tests/test_b3_mix_plan_cpu.py: (n, channels, capacity, layer, kslices, mix_rows option)
B3_PLANS = [(8, 512, 4096, 2, 1, 0), (8, 512, 911, 2, 1, 0), (8, 512, 160, 2, 4, 256), (8, 512, 160, 3, 8, 512), (6, 512, 160, 2, 8, 256),
            # ... and the two the GPU test forces into test_gpu_layer_parity's 192-board network
            (8, 256, 192, 2, 4, 256), (8, 256, 192, 3, 8, 256), (8, 256, 192, 2, 4, 512), (8, 256, 192, 3, 8, 512)]


@pytest.mark.parametrize("n,channels,cap,layer,kslices,mix", B3_PLANS)
def test_every_class_or_the_reason_on_the_mixed_plans(n, channels, cap, layer, kslices, mix):
    from othellozero_amd.NNet import b3_plan
    p = b3_plan(n, channels, cap, layer, kslices=kslices, mix_rows=mix)
    assert p["kernel"] == "b3_mixed", p
    hout = R.layer_geometry(n, channels, layer)[1]
    pixels, big = hout * hout, p["big_rows"]
    got = S.mixed_counts(pixels, big, cap)
    below = [c for c in range(1, cap) if c * pixels < big]
    at = [c for c in range(1, cap) if c * pixels == big]
    above = [c for c in range(1, cap) if c * pixels > big]
    assert below and got["below"] in below, got
    # 'above' cannot exist only where the boundary lies inside the LAST board of the capacity (911 boards: 32768 rows end inside board 910)
    assert (got["above"] in above) if above else (got["above"] is None and (cap - 1) * pixels <= big < cap * pixels), got
    assert bool(above) == ((n, cap) != (8, 911))
    assert (got["at"] in at) if at else (got["at"] is None and big % pixels != 0), got      # 'at' cannot exist: the boundary falls inside a board
    assert got["below"] == max(below)
    _check_tiles(pixels, 128, cap, (n, cap, layer))


def test_counts_of_plan_keeps_every_class_and_the_three_fixed_counts():
    plan = {1: dict(kernel="lut", tile_rows=0, kslices=1, big_rows=0), 2: dict(kernel="b3_mixed", tile_rows=128, kslices=4, big_rows=256),
            3: dict(kernel="b3", tile_rows=128, kslices=8, big_rows=0), 4: dict(kernel="b3", tile_rows=128, kslices=2, big_rows=0),
            5: dict(kernel="b3", tile_rows=128, kslices=4, big_rows=0)}
    counts, why = S.counts_of_plan(plan, {1: 64, 2: 36, 3: 16, 4: 1, 5: 1}, 192)
    assert counts == sorted(set(counts)) and {0, 1, 191} <= set(counts) and all(0 <= c < 192 for c in counts)
    reasons = {r for rs in why.values() for r in rs}
    assert {"empty", "one", "launch-1", "layer2:cut", "layer2:edge", "layer2:below", "layer2:above", "layer3:cut", "layer3:edge", "layer4:cut",
            "layer4:edge", "layer5:cut", "layer5:edge"} <= reasons, reasons
    assert "layer2:at" not in reasons and not any(r.startswith("layer1") for r in reasons)       # 256 rows end inside board 7; the gather has no tiles
    assert why[7] == ["layer2:below"] or "layer2:below" in why[7]
