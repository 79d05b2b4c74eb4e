#!/usr/bin/env python3
"""What a playout cap (playout_cap=(fast_sims, full_prob), oz_selfplay_set_playout_cap) buys in games per second.

    python tools/playout_cap_bench.py [--out profiles/playout_cap_bench.json] [--games 4096] [--sims 100] [--precision bf16x3]
                                      [--steps 200] [--sims-pre 8] [--fast-sims 20] [--full-prob 0.25]

One process, one network, the BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a random-init
512-filter OthelloNN, refilled slots, the free-running driver).  The cap is set before an engine's first driver call, so "off" and "capped"
are two engines on the same network, created alike and both spread over the plies of a game first (SelfPlayEngine.stagger at `--sims-pre`
simulations per move, untimed; a staggered round is never capped).  They take turns: three repetitions, in each of them `--steps` network
batches of run_steps() on the one, then on the other.  Per run: expansions/s, leaves per batch, moves/s, completed games/s and full records/s
(the moves searched on the full budget: the training examples; without a cap that is every move).  The comparison is against off IN THE SAME
REPETITION; no threshold is set here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 3
RATES = ("expansions_per_s", "leaves_per_batch", "moves_per_s", "games_per_s", "full_records_per_s")


def bench(args):
    import numpy as np
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G = 8, args.games
    cap = (args.fast_sims, args.full_prob)
    net = NNetWrapper((n, n), max_batch=G, seed=1, precision=args.precision)
    mean_budget = cap[1] * args.sims + (1 - cap[1]) * cap[0]
    engines, stagger_s = {}, {}
    for name, kw in (("off", {}), ("capped", {"playout_cap": cap})):
        budget = args.sims if name == "off" else mean_budget
        eng = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=G, refill=True,
                             record_cap=int(G * ((1 + REPEATS) * args.steps / budget + n * n + 2) * 1.5), **kw)
        t0 = time.perf_counter()
        eng.stagger(args.sims_pre)
        stagger_s[name] = time.perf_counter() - t0
        eng.run_steps(args.steps)                                        # warm-up
        engines[name] = eng
    rows = []
    for rep in range(REPEATS):
        for name, eng in engines.items():
            s0, p0 = eng.stats(), eng.playout_stats()
            t0 = time.perf_counter()
            eng.run_steps(args.steps)
            wall = time.perf_counter() - t0
            s1, p1 = eng.stats(), eng.playout_stats()
            assert s1["overflow"] == 0, s1
            moves = s1["moves"] - s0["moves"]
            full = p1["full_moves"] - p0["full_moves"] if name == "capped" else moves
            rows.append(dict(cap=name, repetition=rep, batches=args.steps, wall_ms_per_batch=1e3 * wall / args.steps,
                             expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall,
                             leaves_per_batch=(s1["leaves_evaluated"] - s0["leaves_evaluated"]) / args.steps,
                             simulations_per_move=(s1["simulations"] - s0["simulations"]) / max(moves, 1),
                             moves_per_s=moves / wall, games_per_s=(s1["games_completed"] - s0["games_completed"]) / wall,
                             full_records_per_s=full / wall, full_share_of_moves=full / max(moves, 1)))
            print(json.dumps(rows[-1]), flush=True)
    ratios = []
    for rep in range(REPEATS):
        off, capped = (next(r for r in rows if r["cap"] == name and r["repetition"] == rep) for name in ("off", "capped"))
        ratios.append({k: capped[k] / off[k] if off[k] else float("nan") for k in RATES})
    median = {k: float(np.median([r[k] for r in ratios])) for k in RATES}
    print(json.dumps(dict(capped_over_off_median=median)), flush=True)
    return dict(board=n, games=G, sims=args.sims, precision=args.precision, batches_per_repetition=args.steps, stagger_sims=args.sims_pre,
                stagger_wall_s=stagger_s, playout_cap=list(cap), mean_budget_by_arithmetic=mean_budget, runs=rows,
                capped_over_off_by_repetition=ratios, capped_over_off_median=median)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=200, help="network batches per repetition")
    ap.add_argument("--sims-pre", type=int, default=8, help="simulations per move while the slots are spread over the plies")
    ap.add_argument("--fast-sims", type=int, default=20)
    ap.add_argument("--full-prob", type=float, default=0.25)
    args = ap.parse_args()
    results = bench(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
