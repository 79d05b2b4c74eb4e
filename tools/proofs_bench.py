#!/usr/bin/env python3
"""What the proofs of the search (proofs=True on top of value_signs="sound", oz_selfplay_set_proofs) cost and what they do.

    python tools/proofs_bench.py [--out profiles/proofs_bench.json] [--games 4096] [--sims 100] [--precision bf16x3] [--warmup 60]
                                 [--rounds 40] [--parent-tree DIR] [--solve-leaves 8] [--resign 0.05,2,20,0.1]

The BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a random-init 512-filter OthelloNN,
bf16x3, refilled slots) on the lock-step driver; every engine is warmed up by `--warmup` move rounds (untimed: one game's length, after
which the refills have begun), then three repetitions of `--rounds` move rounds, the engines taking turns inside every repetition.

(a) the default path against the parent commit: `--parent-tree` names a directory that holds the parent commit's built package
    (othellozero_amd/ with its lib/).  Two child processes of this tool, one importing the package from there and one from this tree, each
    with ONE engine without any option, take turns repetition by repetition (a process can load one build of the library).  moves/s.
(b) proofs on against off: two engines in this process, both value_signs="sound", one with proofs=True; the same pair again with
    solve_leaves=`--solve-leaves`.  Per pair: moves/s on over off within the same repetition and the spread; proof_stats per move; the share
    of simulations that ended on a proof; network rows (leaves_evaluated) and expansions per move.
(c) the resign audit of tools/resign_bench.py's first setting (`--resign`), sound signs, with and without proofs: exempt_wrong /
    exempt_triggered summed over the repetitions, and mean plies per finished game.

No threshold is set here: (a) and (b) are to be read against the spread of the repetitions, the rest is written down as measured.  Playing
strength is not measured."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 3
COUNTERS = ("games_adjudicated", "adjudicated_plies_sum", "games_exempt", "exempt_triggered", "exempt_wrong", "exempt_trigger_ply_sum")
PROOF_STATS = ("edges_proven", "edge_stops", "node_stops", "roots_proven")


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


def timed(eng, name, rep, rounds, resign, proofs):
    s0, r0, p0 = eng.stats(), eng.resign_stats() if resign else None, eng.proof_stats() if proofs else None
    t0 = time.perf_counter()
    eng.run(rounds)
    wall = time.perf_counter() - t0
    s1, r1, p1 = eng.stats(), eng.resign_stats() if resign else None, eng.proof_stats() if proofs else None
    assert s1["overflow"] == 0, s1
    moves, games, records, sims = (s1[k] - s0[k] for k in ("moves", "games_completed", "records", "simulations"))
    row = dict(engine=name, repetition=rep, rounds=rounds, wall_s=wall, wall_ms_per_round=1e3 * wall / rounds, moves_per_s=moves / wall,
               expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall, games=games, mean_plies_per_game=records / max(games, 1),
               simulations_per_move=sims / max(moves, 1), expansions_per_move=(s1["expansions"] - s0["expansions"]) / max(moves, 1),
               network_rows_per_move=(s1["leaves_evaluated"] - s0["leaves_evaluated"]) / max(moves, 1),
               terminal_hits_per_move=(s1["terminal_hits"] - s0["terminal_hits"]) / max(moves, 1))
    if resign:
        row.update({k: r1[k] - r0[k] for k in COUNTERS})
    if proofs:
        d = {k: p1[k] - p0[k] for k in PROOF_STATS}
        row.update({k + "_per_move": d[k] / max(moves, 1) for k in PROOF_STATS})
        row["share_of_simulations_ended_on_a_proof"] = (d["edge_stops"] + d["node_stops"]) / max(sims, 1)
    return row


def child(args):
    """one engine without any option, from the package under --package-root: 'ready' after the warm-up, then one timed repetition per line
    read from stdin, its row written as one JSON line"""
    sys.path.insert(0, args.package_root)
    from othellozero_amd.NNet import NNetWrapper
    net = NNetWrapper((8, 8), max_batch=args.games, seed=1, precision=args.precision)
    eng, warm = make_engine(net, args, args.warmup + REPEATS * args.rounds)
    print(json.dumps(dict(ready=True, warmup_wall_s=warm)), flush=True)
    rep = 0
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(json.dumps(timed(eng, args.child, rep, args.rounds, False, False)), flush=True)
        rep += 1
    return 0


def against_parent(args):
    procs = {}
    for name, root in (("parent", os.path.abspath(args.parent_tree)), ("this_commit", ROOT)):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--package-root", root, "--games", str(args.games), "--sims", str(args.sims),
               "--precision", args.precision, "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        procs[name] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
    rows = []
    try:
        for name, p in procs.items():
            assert json.loads(p.stdout.readline())["ready"], name
        for rep in range(REPEATS):
            for name, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                rows.append(json.loads(p.stdout.readline()))
                print(json.dumps(rows[-1]), flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=120)
    by = lambda name, rep: next(r for r in rows if r["engine"] == name and r["repetition"] == rep)      # noqa: E731
    ratios = [by("this_commit", rep)["moves_per_s"] / by("parent", rep)["moves_per_s"] for rep in range(REPEATS)]
    own = {name: spread([by(name, rep)["moves_per_s"] for rep in range(REPEATS)]) for name in procs}
    return dict(runs=rows, this_commit_over_parent_moves_per_s=ratios, summary=spread(ratios), moves_per_s=own)


def in_process(args):
    sys.path.insert(0, ROOT)
    from othellozero_amd.NNet import NNetWrapper
    net = NNetWrapper((8, 8), max_batch=args.games, seed=1, precision=args.precision)
    rounds_total = args.warmup + REPEATS * args.rounds
    sound = {"value_signs": "sound"}
    E = args.solve_leaves
    # (name, options, resign, proofs)
    plan = [("off", dict(sound), False, False), ("on", dict(sound, proofs=True), False, True),
            (f"solve{E}_off", dict(sound, solve_leaves=E), False, False), (f"solve{E}_on", dict(sound, solve_leaves=E, proofs=True), False, True)]
    if args.resign is not None:
        plan += [("resign_off", dict(sound, resign=args.resign), True, False), ("resign_on", dict(sound, resign=args.resign, proofs=True), True, True)]
    engines, warm = {}, {}
    for name, kw, _, _ in plan:
        engines[name], warm[name] = make_engine(net, args, rounds_total, **kw)
    rows = []
    for rep in range(REPEATS):
        for name, _, resign, proofs in plan:
            rows.append(timed(engines[name], name, rep, args.rounds, resign, proofs))
            print(json.dumps(rows[-1]), flush=True)
    by = lambda name, rep: next(r for r in rows if r["engine"] == name and r["repetition"] == rep)      # noqa: E731
    pairs = {}
    for label, off, on in (("plain", "off", "on"), (f"solve_leaves_{E}", f"solve{E}_off", f"solve{E}_on")):
        ratios = [by(on, rep)["moves_per_s"] / by(off, rep)["moves_per_s"] for rep in range(REPEATS)]
        p = dict(on_over_off_moves_per_s=ratios, summary=spread(ratios))
        for side, name in (("off", off), ("on", on)):
            p["moves_per_s_" + side] = spread([by(name, rep)["moves_per_s"] for rep in range(REPEATS)])
            for k in ("network_rows_per_move", "expansions_per_move", "simulations_per_move", "mean_plies_per_game"):
                p[k + "_" + side] = [by(name, rep)[k] for rep in range(REPEATS)]
        for k in [s + "_per_move" for s in PROOF_STATS] + ["share_of_simulations_ended_on_a_proof"]:
            p[k] = [by(on, rep)[k] for rep in range(REPEATS)]
        pairs[label] = p
    audit = None
    if args.resign is not None:
        audit = dict(setting=list(args.resign))
        for side in ("off", "on"):
            tot = {k: sum(by("resign_" + side, rep)[k] for rep in range(REPEATS)) for k in COUNTERS}
            tot["false_positive_rate"] = tot["exempt_wrong"] / tot["exempt_triggered"] if tot["exempt_triggered"] else None
            tot["mean_plies_per_game"] = [by("resign_" + side, rep)["mean_plies_per_game"] for rep in range(REPEATS)]
            audit["proofs_" + side] = tot
    return dict(warmup_wall_s=warm, runs=rows, proofs_on_over_off=pairs, resign_audit=audit)


def resign_setting(text):
    v, r, min_ply, keep = text.split(",")
    return (float(v), int(r), int(min_ply), float(keep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--warmup", type=int, default=60, help="move rounds before the first timed one")
    ap.add_argument("--rounds", type=int, default=40, help="move rounds per repetition")
    ap.add_argument("--parent-tree", default=None, help="directory with the parent commit's built package, for (a)")
    ap.add_argument("--solve-leaves", type=int, default=8, help="E of the second pair of (b)")
    ap.add_argument("--resign", type=resign_setting, default=(0.05, 2, 20, 0.1), help="v,r,min_ply,keep_prob of (c)")
    ap.add_argument("--no-resign", action="store_true", help="leave (c) out")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.no_resign:
        args.resign = None
    results = dict(board=8, games=args.games, sims=args.sims, precision=args.precision, driver="lock-step", warmup_rounds=args.warmup,
                   rounds_per_repetition=args.rounds, repetitions=REPEATS, solve_leaves=args.solve_leaves)
    if args.parent_tree:
        results["default_against_parent"] = against_parent(args)
        print(json.dumps(dict(default_against_parent=results["default_against_parent"]["summary"])), flush=True)
        if args.out:                                       # (kept even if a later part does not finish)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
    results.update(in_process(args))
    print(json.dumps(dict(proofs_on_over_off={k: v["summary"] for k, v in results["proofs_on_over_off"].items()},
                          resign_audit=results["resign_audit"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
