#!/usr/bin/env python3
"""What the selection option (selection=dict(fpu=, cpuct_growth=, prior_first=), oz_selfplay_set_selection) costs and what it does.

    python tools/selection_bench.py [--out profiles/selection_bench.json] [--games 4096] [--sims 100] [--precision bf16x3] [--warmup 60]
                                    [--rounds 40] [--parent-tree DIR] [--bench-steps 20] [--bench-warmup 5] [--solve-records 12]
                                    [--no-bench | --only-parent | --only-bench]

The BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a random-init 512-filter OthelloNN,
bf16x3, refilled slots) on the lock-step driver; every engine is warmed up by `--warmup` move rounds (untimed), then three repetitions of
`--rounds` move rounds, the engines taking turns inside every repetition.

(1) the default path against the parent commit (`--parent-tree`: a directory that holds the parent commit's built package), as
    tools/proofs_bench.py measures it: two child processes with one engine without any option each, taking turns: moves/s.  And bench.py
    (`--gpus 1 --steps --bench-steps --warmup --bench-warmup`) from both trees taking turns, three times each: its node expansions/s.  The
    device code of the default path is the parent's, so the ratios are expected to straddle 1 inside the repetitions' own spread.
(2) the option on against off: five engines in this process -- off, each part alone (fpu=(0.2, 0.1), cpuct_growth=(19652, 1),
    prior_first=True) and all three.  Per setting: moves/s over off within the same repetition and the spread; network rows and expansions
    per move; and, from a short profiled run after the timed ones, the time of the descent launches (the `select` slot of the tree
    kernels' HIP-event timing: the fused expand + backup + descent kernel) per launch.
(3) solve_records(`--solve-records`) over the records of the LAST repetition of "off" and of "all": mean_disc_loss and the share of optimal
    moves among the records it solves.

No threshold is set here and no value is promised: everything is written down as measured, with the spread of the repetitions.  Playing
strength is neither gated nor claimed: the network is a random-init one."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REPEATS = 3
SETTINGS = (("off", None), ("fpu", dict(fpu=(0.2, 0.1))), ("growth", dict(cpuct_growth=(19652, 1.0))), ("prior_first", dict(prior_first=True)),
            ("all", dict(fpu=(0.2, 0.1), cpuct_growth=(19652, 1.0), prior_first=True)))


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


def timed(eng, name, rep, rounds):
    s0 = eng.stats()
    t0 = time.perf_counter()
    eng.run(rounds)
    wall = time.perf_counter() - t0
    s1 = eng.stats()
    assert s1["overflow"] == 0, s1
    moves, games, records = (s1[k] - s0[k] for k in ("moves", "games_completed", "records"))
    return dict(engine=name, repetition=rep, rounds=rounds, wall_s=wall, moves_per_s=moves / wall, moves=moves, games=games,
                expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall, mean_plies_per_game=records / max(games, 1),
                expansions_per_move=(s1["expansions"] - s0["expansions"]) / max(moves, 1),
                network_rows_per_move=(s1["leaves_evaluated"] - s0["leaves_evaluated"]) / max(moves, 1),
                terminal_hits_per_move=(s1["terminal_hits"] - s0["terminal_hits"]) / max(moves, 1), records_before=s0["records"])


def bench_against_parent(args):
    """bench.py's one JSON line from the parent's tree and from this one, taking turns"""
    rows = []
    for rep in range(REPEATS):
        for name, root in (("parent", os.path.abspath(args.parent_tree)), ("this_commit", ROOT)):
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            rows.append(dict(tree=name, repetition=rep, metric=line["metric"], value=line["value"], ms_per_step=line["ms_per_step"]))
            print(json.dumps(rows[-1]), flush=True)
    by = lambda name, rep: next(r for r in rows if r["tree"] == name and r["repetition"] == rep)      # noqa: E731
    ratios = [by("this_commit", rep)["value"] / by("parent", rep)["value"] for rep in range(REPEATS)]
    return dict(runs=rows, this_commit_over_parent_expansions_per_s=ratios, summary=spread(ratios),
                expansions_per_s={name: spread([by(name, rep)["value"] for rep in range(REPEATS)]) for name in ("parent", "this_commit")})


def in_process(args):
    sys.path.insert(0, ROOT)
    from othellozero_amd.NNet import NNetWrapper
    net = NNetWrapper((8, 8), max_batch=args.games, seed=1, precision=args.precision)
    rounds_total = args.warmup + REPEATS * args.rounds + args.profile_rounds
    engines, warm = {}, {}
    for name, sel in SETTINGS:
        engines[name], warm[name] = make_engine(net, args, rounds_total, **({"selection": sel} if sel is not None else {}))
    rows = []
    for rep in range(REPEATS):
        for name, _ in SETTINGS:
            rows.append(timed(engines[name], name, rep, args.rounds))
            print(json.dumps(rows[-1]), flush=True)
    by = lambda name, rep: next(r for r in rows if r["engine"] == name and r["repetition"] == rep)      # noqa: E731
    if args.out:                                           # (the timing rows are kept even if a later step does not finish)
        with open(args.out, "w") as f:
            json.dump(dict(runs=rows), f, indent=1)
    endgame = {}
    for name in ("off", "all"):                            # the records completed during the last repetition (games that ended in it)
        t0 = time.perf_counter()
        st = engines[name].solve_records(args.solve_records, first_record=by(name, REPEATS - 1)["records_before"])
        st["wall_s"] = time.perf_counter() - t0
        st["mean_disc_loss"] = st["disc_loss_sum"] / max(st["solved"], 1)
        st["optimal_share"] = st["optimal_moves"] / max(st["solved"], 1)
        endgame[name] = st
        print(json.dumps({name: st}), flush=True)
    descent = {}
    for name, _ in SETTINGS:                               # the tree kernels under HIP events: a run of its own, after the timed ones
        eng = engines[name]
        eng.profile(True)
        eng.profile_read(reset=True)
        eng.run(args.profile_rounds)
        eng.sync()
        k = eng.profile_read()
        eng.profile(False)
        descent[name] = dict(select_ms_per_launch=k["select"][0] / max(k["select"][1], 1), select_launches=k["select"][1],
                             expand_backup_ms_per_launch=k["expand_backup"][0] / max(k["expand_backup"][1], 1))
        print(json.dumps({name: descent[name]}), flush=True)
    out = {}
    for name, sel in SETTINGS:
        ratios = [by(name, rep)["moves_per_s"] / by("off", rep)["moves_per_s"] for rep in range(REPEATS)]
        p = dict(selection=sel, over_off_moves_per_s=ratios, summary=spread(ratios), moves_per_s=spread([by(name, rep)["moves_per_s"] for rep in range(REPEATS)]),
                 descent_launch=descent[name])
        for k in ("network_rows_per_move", "expansions_per_move", "terminal_hits_per_move", "mean_plies_per_game"):
            p[k] = [by(name, rep)[k] for rep in range(REPEATS)]
        if name in endgame:
            p["solve_records"] = endgame[name]
        out[name] = p
    return dict(warmup_wall_s=warm, runs=rows, selection_on_over_off=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--warmup", type=int, default=60, help="move rounds before the first timed one")
    ap.add_argument("--rounds", type=int, default=40, help="move rounds per repetition")
    ap.add_argument("--profile-rounds", type=int, default=4, help="move rounds of the profiled run of (2)")
    ap.add_argument("--solve-records", type=int, default=12, help="max_empties of the disc-loss measure")
    ap.add_argument("--parent-tree", default=None, help="directory with the parent commit's built package, for (1)")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--no-bench", action="store_true", help="(1) without the bench.py runs")
    ap.add_argument("--only-parent", action="store_true", help="(1) alone; --out is then read, updated and written back")
    ap.add_argument("--only-bench", action="store_true", help="the bench.py runs of (1) alone; --out is then read, updated and written back")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import proofs_bench                                    # (1)'s engines are that tool's measurement, child processes included
    if args.child:
        return proofs_bench.child(args)
    results = dict(board=8, games=args.games, sims=args.sims, precision=args.precision, driver="lock-step", warmup_rounds=args.warmup,
                   rounds_per_repetition=args.rounds, repetitions=REPEATS, solve_records=args.solve_records)
    if (args.only_parent or args.only_bench) and args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
    if not (args.only_parent or args.only_bench):
        results.update(in_process(args))
        print(json.dumps({k: v["summary"] for k, v in results["selection_on_over_off"].items()}), flush=True)
        save()
    if args.parent_tree:
        if not args.only_bench:
            results["default_against_parent"] = proofs_bench.against_parent(args)
            print(json.dumps(dict(default_against_parent=results["default_against_parent"]["summary"])), flush=True)
            save()
        if not args.no_bench:
            results["bench_py_against_parent"] = bench_against_parent(args)
            print(json.dumps(dict(bench_py_against_parent=results["bench_py_against_parent"]["summary"])), flush=True)
            save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
