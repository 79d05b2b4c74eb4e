#!/usr/bin/env python3
"""What resignation (resign=(v, r, min_ply, keep_prob), oz_selfplay_set_resign) costs where it never fires and buys where it does.

    python tools/resign_bench.py [--out profiles/resign_bench.json] [--games 4096] [--sims 100] [--precision bf16x3] [--warmup 60]
                                 [--rounds 75] [--v 0.05] [--r 2] [--min-ply 20] [--keep-prob 0.1]

One process, one network, the BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a random-init
512-filter OthelloNN, refilled slots) on the lock-step driver, the only one the option holds for.  Three engines on the same network, all
with record_values on: "off" (no rule), "armed" (v = 1.0, r = 8, keep_prob = 0: the armed move kernel, a rule that practically never fires)
and "firing" (the setting given).  stagger() is refused with the rule, so every engine is warmed up by `--warmup` plain move rounds
(untimed; one game's length, after which the refills have begun).  They take turns: three repetitions, in each of them `--rounds` move
rounds on the one, then on the next.  Per run: moves/s, finished games/s, records/s (the records of the finished games), mean plies per
finished game and the rule's counters over the run.  Without stagger() the games of an engine start together and end in waves, so the games
counted in a window are lumpy; steady_games_per_s = moves/s over mean plies per finished game is the rate the refilled slots settle at
(every slot plays one move per round whatever the rule does).  (a) armed over off in moves/s is the cost of the armed kernel; (b) firing
over off in games/s and records/s is what the rule buys, and the audit counters say how often it was wrong.  The default firing setting
suits the random-init network this tool plays with, whose root values stay near 0 until the searches reach finished boards a few plies
before the end: it is a setting that fires, not one to train with.  Comparisons are against off IN THE SAME REPETITION; no threshold is set
here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 3
RATES = ("moves_per_s", "games_per_s", "steady_games_per_s", "records_per_s", "mean_plies_per_game")
COUNTERS = ("games_adjudicated", "adjudicated_plies_sum", "games_exempt", "exempt_triggered", "exempt_wrong", "exempt_trigger_ply_sum")


def spread(values):
    import numpy as np
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)))


def bench(args):
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G = 8, args.games
    firing = (args.v, args.r, args.min_ply, args.keep_prob)
    net = NNetWrapper((n, n), max_batch=G, seed=1, precision=args.precision)
    rounds_total = args.warmup + REPEATS * args.rounds
    engines, warm_s = {}, {}
    for name, kw in (("off", {"record_values": True}), ("armed", {"resign": (1.0, 8, 0, 0.0)}), ("firing", {"resign": firing})):
        eng = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=G, refill=True, record_cap=G * (rounds_total + n * n), **kw)
        t0 = time.perf_counter()
        eng.run(args.warmup)
        warm_s[name] = time.perf_counter() - t0
        engines[name] = eng
    rows = []
    for rep in range(REPEATS):
        for name, eng in engines.items():
            s0, r0 = eng.stats(), eng.resign_stats()
            t0 = time.perf_counter()
            eng.run(args.rounds)
            wall = time.perf_counter() - t0
            s1, r1 = eng.stats(), eng.resign_stats()
            assert s1["overflow"] == 0, s1
            moves, games, records = (s1[k] - s0[k] for k in ("moves", "games_completed", "records"))
            rows.append(dict(engine=name, repetition=rep, rounds=args.rounds, wall_s=wall, wall_ms_per_round=1e3 * wall / args.rounds,
                             expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall, moves_per_s=moves / wall, games_per_s=games / wall,
                             steady_games_per_s=moves / wall / (records / games) if games and records else 0.0,
                             records_per_s=records / wall, mean_plies_per_game=records / max(games, 1), games=games,
                             **{k: r1[k] - r0[k] for k in COUNTERS}))
            print(json.dumps(rows[-1]), flush=True)
    by = lambda name, rep: next(r for r in rows if r["engine"] == name and r["repetition"] == rep)      # noqa: E731
    ratios = {name: [{k: by(name, rep)[k] / by("off", rep)[k] if by("off", rep)[k] else float("nan") for k in RATES} for rep in range(REPEATS)]
              for name in ("armed", "firing")}
    summary = {name + "_over_off": {k: spread([r[k] for r in ratios[name]]) for k in RATES} for name in ratios}
    audit = {k: sum(by("firing", rep)[k] for rep in range(REPEATS)) for k in COUNTERS}
    audit["false_positive_rate"] = audit["exempt_wrong"] / audit["exempt_triggered"] if audit["exempt_triggered"] else None
    audit["mean_plies_adjudicated"] = audit["adjudicated_plies_sum"] / audit["games_adjudicated"] if audit["games_adjudicated"] else None
    armed_fired = sum(by("armed", rep)["games_adjudicated"] for rep in range(REPEATS))
    print(json.dumps(dict(summary=summary, firing_audit=audit, armed_games_adjudicated=armed_fired)), flush=True)
    return dict(board=n, games=G, sims=args.sims, precision=args.precision, driver="lock-step", warmup_rounds=args.warmup,
                rounds_per_repetition=args.rounds, warmup_wall_s=warm_s, armed=[1.0, 8, 0, 0.0], firing=list(firing), runs=rows,
                over_off_by_repetition=ratios, summary=summary, firing_audit=audit, armed_games_adjudicated=armed_fired)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--warmup", type=int, default=60, help="plain move rounds before the first timed one")
    ap.add_argument("--rounds", type=int, default=75, help="move rounds per repetition")
    ap.add_argument("--v", type=float, default=0.05)
    ap.add_argument("--r", type=int, default=2)
    ap.add_argument("--min-ply", type=int, default=20)
    ap.add_argument("--keep-prob", type=float, default=0.1)
    args = ap.parse_args()
    results = bench(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
