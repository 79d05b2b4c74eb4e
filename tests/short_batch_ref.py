"""Which live counts a short-batch test runs under a launch of `launch` positions -- TEST INFRASTRUCTURE ONLY (CPU, pure functions).

A forward is launched for `launch` positions (grid and tile plan) while `count` of them are live (tests/test_gpu_short_batches.py).  For a GEMM layer
of `pixels` output rows per position on row tiles of `tile_rows` rows the live rows end at count * pixels; the classes of counts that matter:
  cut    count * pixels is no multiple of the tile (the last live tile is cut in the middle) AND at least one whole tile of the launch lies behind it
  edge   count * pixels is a positive multiple of the tile and count < launch (the live rows end on a tile edge, only empty tiles behind)
and, for a bf16x3 layer on the mixed plan (its first `big_rows` rows on 256-row tiles, the rest on 128-row tiles in a second launch):
  below  0 < count * pixels < big_rows          (the second launch has nothing to do)
  at     count * pixels == big_rows             (the live rows end exactly on the boundary; exists only where pixels divides big_rows)
  above  count * pixels > big_rows, count < launch
A class that cannot exist for a layer is returned as None; tests/test_short_batch_counts_cpu.py holds every answer, the None ones included, against a
search over all counts.  Where several counts qualify the one nearest to half the launch is taken (ties: the smaller): away from both ends, where the
always-present counts 0, 1 and launch - 1 already are ('below': the largest, next to the boundary).
A layer without row tiles (tile_rows == 0: the table gather, one thread per pixel) has no class.  The pixel-major conv2 tile holds ONE pixel of
tile_rows consecutive positions: its rule is the dense one, pixels = 1 (layer_pixels)."""


def _nearest_half(candidates, launch):
    best = None
    for c in candidates:
        if best is None or abs(2 * c - launch) < abs(2 * best - launch):
            best = c
    return best


def is_cut(count, pixels, tile_rows, launch):
    rows, total = count * pixels, launch * pixels
    return 0 < count < launch and rows % tile_rows != 0 and -(-rows // tile_rows) < -(-total // tile_rows)


def is_edge(count, pixels, tile_rows, launch):
    return 0 < count < launch and (count * pixels) % tile_rows == 0


def tile_counts(pixels, tile_rows, launch):
    """dict(cut=count or None, edge=count or None) of one layer"""
    if tile_rows <= 0:
        return dict(cut=None, edge=None)
    # cut: a multiple of the tile is at most lcm(pixels, tile_rows) / pixels counts away, so scanning outwards from the middle is short
    return dict(cut=_nearest_half((c for c in range(1, launch) if is_cut(c, pixels, tile_rows, launch)), launch),
                edge=_nearest_half((c for c in range(1, launch) if is_edge(c, pixels, tile_rows, launch)), launch))


def mixed_counts(pixels, big_rows, launch):
    """dict(below=, at=, above=) of a layer on the mixed plan with the boundary at big_rows; None where the class cannot exist"""
    assert big_rows > 0
    below = min((big_rows - 1) // pixels, launch - 1)                                   # the largest count whose rows end before the boundary
    return dict(below=below if below >= 1 else None,
                at=big_rows // pixels if big_rows % pixels == 0 and 0 < big_rows // pixels < launch else None,
                above=_nearest_half((c for c in range(1, launch) if c * pixels > big_rows), launch))


def layer_pixels(kernel, pixels):
    """rows of a position inside ONE tile of the layer: the pixel-major tile holds one pixel of consecutive positions"""
    return 1 if kernel == "f32_std_pixmajor" else pixels


def counts_of_plan(plan, pixels_of_layer, launch):
    """the count list of a launch: 0, 1, launch - 1 and every class of every GEMM layer of layer_plan()'s `plan` (pixels_of_layer: layer -> output
    pixels per position) -> (sorted counts below `launch`, {count: [reasons]})"""
    why = {}

    def add(c, reason):
        if c is not None and 0 <= c < launch:
            why.setdefault(c, []).append(reason)
    add(0, "empty")
    add(1, "one")
    add(launch - 1, "launch-1")
    for layer, p in sorted(plan.items()):
        px = layer_pixels(p["kernel"], pixels_of_layer[layer])
        for cls, c in sorted(tile_counts(px, p["tile_rows"], launch).items()):
            add(c, f"layer{layer}:{cls}")
        if p["kernel"] == "b3_mixed":
            for cls, c in sorted(mixed_counts(px, p["big_rows"], launch).items()):
                add(c, f"layer{layer}:{cls}")
    return sorted(why), why
