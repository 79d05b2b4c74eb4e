"""Tree collection: what the option costs and what it frees ("Tree collection").

    python tools/tree_gc_bench.py --out profiles/tree_gc_bench.json [--parts parent,demand,big,arena] [--parent-tree DIR]
                                  [--games 4096] [--sims 100] [--big-sims 800] [--arena-games 512] [--precision bf16x3]
                                  [--warmup 60] [--rounds 40] [--big-rounds 8] [--bench-steps 20] [--bench-warmup 5]

Four parts, each written into --out as it finishes (an existing file is read, updated and written back), runs taking turns in one process,
three repetitions, as the other option benches do:
  parent  the default path against the parent commit (`--parent-tree`: a directory that holds the parent commit's built package): moves/s of
          an engine without any option from either package (tools/proofs_bench.py's child processes) and bench.py's expansions/s.  Off, the
          device code is the parent's, so the ratios are expected to straddle 1 inside the repetitions' own spread.
  demand  --games games of 8x8 at --sims simulations: a pilot with tree_gc="every" at the default capacity measures peak_kept; then "demand" at
          node_cap = peak_kept + 2 * sims against off at the default capacity: moves/s, peak_nodes / peak_kept, the kept share, collections
          per game, time per collection launch (HIP events, a run of its own) and the device memory of the tree.
  big     the configuration the option is for: --big-sims simulations.  A pilot ("every", node_cap = 16 * sims) measures peak_kept; then
          "demand" at node_cap = peak_kept + sims: that it runs, at what memory, at how many moves/s.
  arena   --arena-games games at --big-sims: "every" measures peak_kept per agent, then "demand" at the capacity sized from it against off.
Playing strength is neither gated nor claimed: the option changes no move."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REPEATS = 3


def spread(values):
    import numpy as np
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def next_pow2(x):
    p = 64
    while p < x:
        p <<= 1
    return p


def tree_bytes(n, games, node_cap, collecting):
    """records + hash table (+ the collection's scratch map) of one search object, as mcts_create sizes them"""
    row_cap = min(n * n - 4, 41)
    rec = (32 + 24 * row_cap + 63) & ~63
    return games * (node_cap * rec + 4 * next_pow2(2 * node_cap) + (4 * node_cap if collecting else 0))


def default_cap(n, sims):
    return sims * (n * n - 4 + 1) + 64


def make_engine(net, games, sims, rounds_total, **kw):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, 8, games, sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=games, refill=True,
                          record_cap=games * (rounds_total + 64), **kw)


def timed(eng, name, rep, rounds):
    s0 = eng.stats()
    t0 = time.perf_counter()
    eng.run(rounds)
    wall = time.perf_counter() - t0
    s1 = eng.stats()
    assert s1["overflow"] == 0, s1
    moves = s1["moves"] - s0["moves"]
    return dict(engine=name, repetition=rep, rounds=rounds, wall_s=wall, moves=moves, moves_per_s=moves / wall,
                games=s1["games_completed"] - s0["games_completed"], expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall)


def gc_summary(eng, n, games, node_cap):
    st = eng.tree_gc_stats()
    done = max(eng.stats()["games_completed"], 1)
    return dict(st, node_cap=node_cap, kept_share=st["nodes_kept_sum"] / max(st["nodes_before_sum"], 1), collections_per_game=st["collections"] / done,
                tree_bytes=tree_bytes(n, games, node_cap, st["mode"] != "off"))


def launch_time(eng, rounds):
    eng.tree_gc_profile(True)
    eng.tree_gc_profile_read(reset=True)
    eng.run(rounds)
    ms, count = eng.tree_gc_profile_read()
    eng.tree_gc_profile(False)
    return dict(launches=count, ms_per_launch=ms / max(count, 1))


def pilot(net, games, sims, node_cap, rounds):
    """an engine with tree_gc="every" over a whole game's plies -> its statistics (peak_kept: a property of the games, not of the mode)"""
    eng = make_engine(net, games, sims, rounds, tree_gc="every", node_cap=node_cap)
    t0 = time.perf_counter()
    eng.run(rounds)
    out = dict(gc_summary(eng, 8, games, node_cap), rounds=rounds, wall_s=time.perf_counter() - t0, launch=launch_time(eng, 2))
    assert eng.stats()["overflow"] == 0
    return out


def part_demand(args, net):
    G, sims = args.games, args.sims
    cap0 = default_cap(8, sims)
    pl = pilot(net, G, sims, cap0, 62)
    print(json.dumps(dict(pilot=pl)), flush=True)
    cap = pl["peak_kept"] + 2 * sims
    rounds_total = args.warmup + REPEATS * args.rounds + 4
    engines = dict(off=make_engine(net, G, sims, rounds_total), demand=make_engine(net, G, sims, rounds_total, tree_gc="demand", node_cap=cap))
    for e in engines.values():
        e.run(args.warmup)
    rows = []
    for rep in range(REPEATS):
        for name, e in engines.items():
            rows.append(timed(e, name, rep, args.rounds))
            print(json.dumps(rows[-1]), flush=True)
    by = lambda name, rep: next(r for r in rows if r["engine"] == name and r["repetition"] == rep)      # noqa: E731
    ratios = [by("demand", rep)["moves_per_s"] / by("off", rep)["moves_per_s"] for rep in range(REPEATS)]
    same = engines["off"].records().tobytes() == engines["demand"].records().tobytes()
    return dict(games=G, sims=sims, pilot_every=pl, node_cap_off=cap0, node_cap_demand=cap, runs=rows, demand_over_off_moves_per_s=ratios, summary=spread(ratios),
                moves_per_s={k: spread([by(k, rep)["moves_per_s"] for rep in range(REPEATS)]) for k in engines}, records_identical=same,
                demand=dict(gc_summary(engines["demand"], 8, G, cap), launch=launch_time(engines["demand"], 4)),
                tree_bytes_off=tree_bytes(8, G, cap0, False))


def part_big(args, net):
    G, sims = args.games, args.big_sims
    pl = pilot(net, G, sims, 16 * sims, 62)
    print(json.dumps(dict(pilot=pl)), flush=True)
    cap = pl["peak_kept"] + sims
    eng = make_engine(net, G, sims, 62 + REPEATS * args.big_rounds + 4, tree_gc="demand", node_cap=cap)
    eng.run(62)
    rows = [timed(eng, "demand", rep, args.big_rounds) for rep in range(REPEATS)]
    return dict(games=G, sims=sims, pilot_every=pl, node_cap=cap, node_cap_default=default_cap(8, sims), runs=rows,
                moves_per_s=spread([r["moves_per_s"] for r in rows]), demand=dict(gc_summary(eng, 8, G, cap), launch=launch_time(eng, 2)),
                tree_bytes_default=tree_bytes(8, G, default_cap(8, sims), False), overflow=eng.stats()["overflow"])


def part_arena(args, net):
    import numpy as np
    from othellozero_amd.agents import arena_batch
    G, sims = args.arena_games, args.big_sims
    cap0 = sims * (64 // 2 + 2) + 64

    def run(name, **kw):
        t0 = time.perf_counter()
        r = arena_batch(net, net, 8, G, sims, seed=7, **kw)
        wall = time.perf_counter() - t0
        row = dict(run=name, wall_s=wall, moves=int(r["n_moves"].sum()), moves_per_s=int(r["n_moves"].sum()) / wall, tree_gc_stats=r.get("tree_gc_stats"))
        print(json.dumps(row), flush=True)
        return r, row
    ev, ev_row = run("every_default_cap", tree_gc="every")
    cap = max(s["peak_kept"] for s in ev["tree_gc_stats"]) + 2 * sims
    rows = [ev_row]
    results = {}
    for rep in range(REPEATS):
        for name, kw in (("off", {}), ("demand", dict(tree_gc="demand", node_cap=cap))):
            results[name], row = run(name, **kw)
            rows.append(dict(row, repetition=rep))
    same = all(np.array_equal(results["off"][k], results["demand"][k]) for k in ("winner", "points", "n_moves", "actions", "stats_black", "stats_white"))
    rate = lambda name: [r["moves_per_s"] for r in rows if r["run"] == name]      # noqa: E731
    ratios = [d / o for d, o in zip(rate("demand"), rate("off"))]
    return dict(games=G, sims=sims, node_cap_off=cap0, node_cap_demand=cap, runs=rows, results_identical=same, demand_over_off_moves_per_s=ratios,
                summary=spread(ratios), tree_bytes_off=2 * tree_bytes(8, G, cap0, False), tree_bytes_demand=2 * tree_bytes(8, G, cap, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="parent,demand,big,arena")
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--big-sims", type=int, default=800)
    ap.add_argument("--arena-games", type=int, default=512)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--warmup", type=int, default=60, help="move rounds before the first timed one")
    ap.add_argument("--rounds", type=int, default=40, help="move rounds per repetition")
    ap.add_argument("--big-rounds", type=int, default=8, help="move rounds per repetition at --big-sims")
    ap.add_argument("--parent-tree", default=None, help="directory with the parent commit's built package, for the part `parent`")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    args = ap.parse_args()
    import proofs_bench                                    # the part `parent` is that tool's measurement (child processes included) and selection_bench's
    import selection_bench
    results = dict(board=8, precision=args.precision, driver="lock-step", repetitions=REPEATS)
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
    parts = args.parts.split(",")
    if "parent" in parts:
        assert args.parent_tree, "--parent-tree"
        results["default_against_parent"] = proofs_bench.against_parent(args)
        save()
        results["bench_py_against_parent"] = selection_bench.bench_against_parent(args)
        save()
    net = None
    if set(parts) & {"demand", "big", "arena"}:
        sys.path.insert(0, ROOT)
        from othellozero_amd.NNet import NNetWrapper
        net = NNetWrapper((8, 8), max_batch=args.games, seed=1, precision=args.precision)
    for name, fn in (("demand", part_demand), ("big", part_big), ("arena", part_arena)):
        if name in parts:
            results[name] = fn(args, net)
            print(json.dumps({name: {k: v for k, v in results[name].items() if k != "runs"}}), flush=True)
            save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
