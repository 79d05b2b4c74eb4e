#!/usr/bin/env python3
"""What forced playouts and policy target pruning (forced_playouts=k, oz_selfplay_set_forced_playouts) do to the self-play engine.

    python tools/forced_playouts_bench.py [--out profiles/forced_playouts_bench.json] [--games 4096] [--sims 100] [--precision bf16x3]
                                          [--steps 200] [--sims-pre 8] [--k 2.0] [--alpha 0.3] [--eps 0.25]

One process, one network, the BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a random-init
512-filter OthelloNN, refilled slots, the free-running driver) with root_noise=(alpha, eps) and record_visits.  The option is set before an
engine's first driver call, so "off" and "forced" are two engines on the same network, created alike and both spread over the plies of a game
first (SelfPlayEngine.stagger at `--sims-pre` simulations per move, untimed).  They take turns: three repetitions, in each of them `--steps`
network batches of run_steps() on the one, then on the other.  Per run: moves/s, expansions/s, leaves per batch, and for the forced engine the
share of the visits that pruning took out of the recorded rows and the share of the moves whose row changed (the engine's counters,
SelfPlayEngine.forced_playout_stats).  The comparison is against off IN THE SAME REPETITION; no threshold is set here: that off is unchanged is
shown by bit identity in the tests, not by timing."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 3
RATES = ("moves_per_s", "expansions_per_s", "leaves_per_batch", "games_per_s")


def bench(args):
    import numpy as np
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G = 8, args.games
    noise = (args.alpha, args.eps)
    net = NNetWrapper((n, n), max_batch=G, seed=1, precision=args.precision)
    engines, stagger_s = {}, {}
    for name, kw in (("off", {}), ("forced", {"forced_playouts": args.k})):
        eng = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=G, refill=True, record_visits=True, root_noise=noise,
                             record_cap=int(G * ((1 + REPEATS) * args.steps / args.sims + n * n + 2) * 1.5), **kw)
        t0 = time.perf_counter()
        eng.stagger(args.sims_pre)
        stagger_s[name] = time.perf_counter() - t0
        eng.run_steps(args.steps)                                        # warm-up
        engines[name] = eng
    rows = []
    for rep in range(REPEATS):
        for name, eng in engines.items():
            s0, f0 = eng.stats(), eng.forced_playout_stats()
            t0 = time.perf_counter()
            eng.run_steps(args.steps)
            wall = time.perf_counter() - t0
            s1, f1 = eng.stats(), eng.forced_playout_stats()
            assert s1["overflow"] == 0, s1
            moves = s1["moves"] - s0["moves"]
            raw, kept = f1["visits_raw"] - f0["visits_raw"], f1["visits_kept"] - f0["visits_kept"]
            rows.append(dict(option=name, repetition=rep, batches=args.steps, wall_ms_per_batch=1e3 * wall / args.steps,
                             moves=moves, moves_per_s=moves / wall, games_per_s=(s1["games_completed"] - s0["games_completed"]) / wall,
                             expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall,
                             leaves_per_batch=(s1["leaves_evaluated"] - s0["leaves_evaluated"]) / args.steps,
                             simulations_per_move=(s1["simulations"] - s0["simulations"]) / max(moves, 1),
                             visits_raw=raw, visits_kept=kept, share_of_visits_pruned=(raw - kept) / raw if raw else 0.0,
                             share_of_moves_with_a_changed_row=(f1["moves_pruned"] - f0["moves_pruned"]) / max(moves, 1)))
            print(json.dumps(rows[-1]), flush=True)
    ratios = []
    for rep in range(REPEATS):
        off, forced = (next(r for r in rows if r["option"] == name and r["repetition"] == rep) for name in ("off", "forced"))
        ratios.append({k: forced[k] / off[k] if off[k] else float("nan") for k in RATES})
    forced_rows = [r for r in rows if r["option"] == "forced"]
    median = {k: float(np.median([r[k] for r in ratios])) for k in RATES}
    summary = dict(moves_per_s_off=float(np.median([r["moves_per_s"] for r in rows if r["option"] == "off"])),
                   moves_per_s_forced=float(np.median([r["moves_per_s"] for r in forced_rows])),
                   share_of_visits_pruned=float(np.median([r["share_of_visits_pruned"] for r in forced_rows])),
                   share_of_moves_with_a_changed_row=float(np.median([r["share_of_moves_with_a_changed_row"] for r in forced_rows])))
    print(json.dumps(dict(forced_over_off_median=median, **summary)), flush=True)
    return dict(board=n, games=G, sims=args.sims, precision=args.precision, batches_per_repetition=args.steps, stagger_sims=args.sims_pre,
                stagger_wall_s=stagger_s, root_noise=list(noise), forced_playouts=args.k, runs=rows, forced_over_off_by_repetition=ratios,
                forced_over_off_median=median, medians=summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=200, help="network batches per repetition")
    ap.add_argument("--sims-pre", type=int, default=8, help="simulations per move while the slots are spread over the plies")
    ap.add_argument("--k", type=float, default=2.0, help="the forcing constant")
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--eps", type=float, default=0.25)
    args = ap.parse_args()
    results = bench(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
