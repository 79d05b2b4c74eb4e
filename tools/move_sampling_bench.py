#!/usr/bin/env python3
"""What move sampling costs a lock-step move round, measured against the same engine without it IN THE SAME PROCESS.

    python tools/move_sampling_bench.py [--games 4096] [--sims 100] [--board 8] [--rounds 6] [--reps 3] [--precision bf16x3] [--off-only]

Per setting (sampling off / on, alternating, --reps engines each): a continuous engine (refill) is staggered over the plies of a game, warmed up,
then `rounds` move rounds run with the HIP-event profile of the tree kernels on (oz_selfplay_profile_read).  The move kernel is timed in slot 4,
roots_move (roots kernel + move kernel, two launches per round); slot 3, expand_backup, is the closing launch of a round.  "on" samples EVERY
ply (plies = 64, e_greedy = 1): each of the `games` moves of a round runs the sampler.  One JSON line per engine and a summary: ms per round and
slot, and the difference of slot 4 per move.  --off-only: the unarmed engine alone (a tree without the feature can run it)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one_engine(args, net, sample_moves):
    from othellozero_amd import _lib
    from othellozero_amd.training import SelfPlayEngine
    kw = {} if sample_moves is None else {"sample_moves": sample_moves}
    eng = SelfPlayEngine(net, args.board, args.games, args.sims, 1.0, 1.0, 1.0, seed=7, refill=True, **kw)
    eng.stagger(args.stagger_sims)
    eng.profile(True)
    eng.run(args.warmup)
    eng.profile_read(reset=True)
    s0 = eng.stats()
    t0 = time.perf_counter()
    eng.run(args.rounds)
    wall = time.perf_counter() - t0
    prof, s1 = eng.profile_read(), eng.stats()
    out = {"sample_moves": sample_moves, "rounds": args.rounds, "wall_ms_per_round": 1e3 * wall / args.rounds,
           "ms_per_round": {k: prof[k][0] / args.rounds for k in _lib.TREE_KERNELS},
           "launches_per_round": {k: prof[k][1] / args.rounds for k in _lib.TREE_KERNELS}}
    out["gpu_ms_per_round"] = sum(out["ms_per_round"].values())
    out["moves_per_round"] = (s1["moves"] - s0["moves"]) / args.rounds
    out["expansions_per_round"] = (s1["expansions"] - s0["expansions"]) / args.rounds
    del eng
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--board", type=int, default=8)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stagger-sims", type=int, default=8)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    from othellozero_amd import _lib
    from othellozero_amd.NNet import NNetWrapper
    _lib.require_gpu()
    net = NNetWrapper((args.board, args.board), num_channels_1=args.channels, max_batch=args.games, seed=0, precision=args.precision)
    settings = [("off", None)] if args.off_only else [("off", None), ("on", (args.temperature, 64))]
    runs = {name: [] for name, _ in settings}
    for _ in range(args.reps):
        for name, sample_moves in settings:
            r = one_engine(args, net, sample_moves)
            runs[name].append(r)
            print(json.dumps({"setting": name, **r}), flush=True)

    def mean(name, f):
        return sum(f(r) for r in runs[name]) / len(runs[name])
    summary = {"games": args.games, "sims": args.sims, "board": args.board, "precision": args.precision}
    for name in runs:
        summary[f"gpu_ms_per_round_{name}"] = mean(name, lambda r: r["gpu_ms_per_round"])
        summary[f"expand_backup_ms_per_round_{name}"] = mean(name, lambda r: r["ms_per_round"]["expand_backup"])
        summary[f"roots_move_ms_per_round_{name}"] = mean(name, lambda r: r["ms_per_round"]["roots_move"])
    if "on" in runs:
        d = summary["roots_move_ms_per_round_on"] - summary["roots_move_ms_per_round_off"]
        summary["sample_moves"] = [args.temperature, 64]
        summary["sampler_ms_per_round"] = d
        summary["sampler_ns_per_move"] = 1e6 * d / mean("on", lambda r: r["moves_per_round"])
        summary["sampler_share_of_round"] = d / summary["gpu_ms_per_round_on"]
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
