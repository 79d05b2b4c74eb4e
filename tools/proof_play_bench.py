#!/usr/bin/env python3
"""What proof play (proof_play=True on top of proofs=True, oz_selfplay_set_proof_play) costs and what it does.

    python tools/proof_play_bench.py [--out profiles/proof_play_bench.json] [--games 4096] [--sims 100] [--precision bf16x3] [--warmup 60]
                                     [--rounds 40] [--solve-leaves 8] [--solve-records 12] [--parent-tree DIR] [--only-parent]

The BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a random-init 512-filter OthelloNN,
bf16x3, refilled slots) on the lock-step driver, value_signs="sound", proofs=True; every engine is warmed up by `--warmup` move rounds
(untimed), then three repetitions of `--rounds` move rounds, the engines taking turns inside every repetition.

(a) proof_play on against off: two engines in this process; the same pair again with solve_leaves=`--solve-leaves`.  Per pair: moves/s on
    over off within the same repetition and the spread; the four counters of proof_play_stats() as shares of the searched moves; and
    solve_records(`--solve-records`) over the records of the LAST repetition of either engine: mean_disc_loss and the share of optimal moves
    among the records it solves -- the plies near the end of the game, where roots are proven.
(b) the default path against the parent commit (`--parent-tree`: a directory that holds the parent commit's built package), as
    tools/proofs_bench.py measures it: two child processes with one engine without any option each, taking turns.

No threshold is set here and no value is promised: everything is written down as measured, with the spread of the repetitions."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REPEATS = 3
STATS = ("proven_roots", "rows_changed", "moves_changed", "fallbacks")


def spread(values):
    import numpy as np
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def make_engine(net, args, rounds_total, **kw):
    from othellozero_amd.training import SelfPlayEngine
    n, G = 8, args.games
    eng = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=G, refill=True, record_cap=G * (rounds_total + n * n), **kw)
    t0 = time.perf_counter()
    eng.run(args.warmup)
    return eng, time.perf_counter() - t0


def timed(eng, name, rep, rounds, on):
    s0, p0 = eng.stats(), eng.proof_play_stats() if on else None
    t0 = time.perf_counter()
    eng.run(rounds)
    wall = time.perf_counter() - t0
    s1, p1 = eng.stats(), eng.proof_play_stats() if on else None
    assert s1["overflow"] == 0, s1
    moves, games, records = (s1[k] - s0[k] for k in ("moves", "games_completed", "records"))
    row = dict(engine=name, repetition=rep, rounds=rounds, wall_s=wall, moves_per_s=moves / wall, moves=moves, games=games,
               expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall, mean_plies_per_game=records / max(games, 1),
               records_before=s0["records"])
    if on:
        row.update({k + "_share_of_moves": (p1[k] - p0[k]) / max(moves, 1) for k in STATS})
    return row


def in_process(args):
    sys.path.insert(0, ROOT)
    from othellozero_amd.NNet import NNetWrapper
    net = NNetWrapper((8, 8), max_batch=args.games, seed=1, precision=args.precision)
    rounds_total = args.warmup + REPEATS * args.rounds
    base = {"value_signs": "sound", "proofs": True}
    E = args.solve_leaves
    plan = [("off", dict(base), False), ("on", dict(base, proof_play=True), True),
            (f"solve{E}_off", dict(base, solve_leaves=E), False), (f"solve{E}_on", dict(base, solve_leaves=E, proof_play=True), True)]
    engines, warm = {}, {}
    for name, kw, _ in plan:
        engines[name], warm[name] = make_engine(net, args, rounds_total, **kw)
    rows = []
    for rep in range(REPEATS):
        for name, _, on in plan:
            rows.append(timed(engines[name], name, rep, args.rounds, on))
            print(json.dumps(rows[-1]), flush=True)
    by = lambda name, rep: next(r for r in rows if r["engine"] == name and r["repetition"] == rep)      # noqa: E731
    if args.out:                                           # (the timing rows are kept even if the solver step does not finish)
        with open(args.out, "w") as f:
            json.dump(dict(runs=rows), f, indent=1)
    endgame = {}
    for name, _, _ in plan:                                # the records completed during the last repetition (games that ended in it)
        t0 = time.perf_counter()
        st = engines[name].solve_records(args.solve_records, first_record=by(name, REPEATS - 1)["records_before"])
        st["wall_s"] = time.perf_counter() - t0
        st["mean_disc_loss"] = st["disc_loss_sum"] / max(st["solved"], 1)
        st["optimal_share"] = st["optimal_moves"] / max(st["solved"], 1)
        endgame[name] = st
        print(json.dumps({name: st}), flush=True)
    pairs = {}
    for label, off, on in (("plain", "off", "on"), (f"solve_leaves_{E}", f"solve{E}_off", f"solve{E}_on")):
        ratios = [by(on, rep)["moves_per_s"] / by(off, rep)["moves_per_s"] for rep in range(REPEATS)]
        p = dict(on_over_off_moves_per_s=ratios, summary=spread(ratios))
        for side, name in (("off", off), ("on", on)):
            p["moves_per_s_" + side] = spread([by(name, rep)["moves_per_s"] for rep in range(REPEATS)])
            p["mean_plies_per_game_" + side] = [by(name, rep)["mean_plies_per_game"] for rep in range(REPEATS)]
            p["solve_records_" + side] = endgame[name]
        for k in STATS:
            p[k + "_share_of_moves"] = [by(on, rep)[k + "_share_of_moves"] for rep in range(REPEATS)]
        pairs[label] = p
    return dict(warmup_wall_s=warm, runs=rows, proof_play_on_over_off=pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--warmup", type=int, default=60, help="move rounds before the first timed one")
    ap.add_argument("--rounds", type=int, default=40, help="move rounds per repetition")
    ap.add_argument("--solve-leaves", type=int, default=8, help="E of the second pair")
    ap.add_argument("--solve-records", type=int, default=12, help="max_empties of the disc-loss measure")
    ap.add_argument("--parent-tree", default=None, help="directory with the parent commit's built package, for (b)")
    ap.add_argument("--only-parent", action="store_true", help="(b) alone; --out is then read, updated and written back")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import proofs_bench                                    # (b) is that tool's measurement, child processes included
    if args.child:
        return proofs_bench.child(args)
    results = dict(board=8, games=args.games, sims=args.sims, precision=args.precision, driver="lock-step", warmup_rounds=args.warmup,
                   rounds_per_repetition=args.rounds, repetitions=REPEATS, solve_leaves=args.solve_leaves, solve_records=args.solve_records)
    if args.only_parent and args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    if args.parent_tree:
        results["default_against_parent"] = proofs_bench.against_parent(args)
        print(json.dumps(dict(default_against_parent=results["default_against_parent"]["summary"])), flush=True)
    if not args.only_parent:
        results.update(in_process(args))
        print(json.dumps({k: v["summary"] for k, v in results["proof_play_on_over_off"].items()}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
