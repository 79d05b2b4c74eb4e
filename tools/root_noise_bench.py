#!/usr/bin/env python3
"""What root noise costs a lock-step move round, measured against the same engine without it IN THE SAME PROCESS.

    python tools/root_noise_bench.py [--games 4096] [--sims 100] [--board 8] [--rounds 6] [--reps 2] [--precision bf16x3]

Per setting (noise off / on, alternating, --reps engines each): a continuous engine (refill) is staggered over the plies of a game, warmed up,
then `rounds` move rounds run with the HIP-event profile of the tree kernels on (oz_selfplay_profile_read).  k_root_noise is timed in the
roots_move slot (roots kernel + k_root_noise + move kernel), the noisy PUCT loop in the select slot (the fused expand + backup + descent
launches).  One JSON line per engine and a summary: ms per round and slot, the two differences, and their share of the round's GPU time."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one_engine(args, net, noise):
    from othellozero_amd import _lib
    from othellozero_amd.training import SelfPlayEngine
    eng = SelfPlayEngine(net, args.board, args.games, args.sims, 1.0, 1.0, 0.9, seed=7, refill=True, root_noise=noise)
    eng.stagger(args.stagger_sims)
    eng.profile(True)
    eng.run(args.warmup)
    eng.profile_read(reset=True)
    s0 = eng.stats()
    t0 = time.perf_counter()
    eng.run(args.rounds)
    wall = time.perf_counter() - t0
    prof, s1 = eng.profile_read(), eng.stats()
    out = {"noise": noise, "rounds": args.rounds, "wall_ms_per_round": 1e3 * wall / args.rounds,
           "ms_per_round": {k: prof[k][0] / args.rounds for k in _lib.TREE_KERNELS},
           "launches_per_round": {k: prof[k][1] / args.rounds for k in _lib.TREE_KERNELS}}
    out["gpu_ms_per_round"] = sum(out["ms_per_round"].values())
    # (cross-game de-duplication: games that search alike reach the same boards in the same step and share one evaluation)
    out["expansions_per_round"] = (s1["expansions"] - s0["expansions"]) / args.rounds
    out["leaves_evaluated_per_round"] = (s1["leaves_evaluated"] - s0["leaves_evaluated"]) / args.rounds
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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--stagger-sims", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--epsilon", type=float, default=0.25)
    args = ap.parse_args()
    from othellozero_amd import _lib
    from othellozero_amd.NNet import NNetWrapper
    _lib.require_gpu()
    net = NNetWrapper((args.board, args.board), num_channels_1=args.channels, max_batch=args.games, seed=0, precision=args.precision)
    runs = {"off": [], "on": []}
    for _ in range(args.reps):
        for name, noise in (("off", None), ("on", (args.alpha, args.epsilon))):
            r = one_engine(args, net, noise)
            runs[name].append(r)
            print(json.dumps({"setting": name, **r}), flush=True)

    def mean(name, f):
        return sum(f(r) for r in runs[name]) / len(runs[name])
    off, on = (mean(s, lambda r: r["gpu_ms_per_round"]) for s in ("off", "on"))
    d_roots = mean("on", lambda r: r["ms_per_round"]["roots_move"]) - mean("off", lambda r: r["ms_per_round"]["roots_move"])
    d_select = mean("on", lambda r: r["ms_per_round"]["select"]) - mean("off", lambda r: r["ms_per_round"]["select"])
    print(json.dumps({"summary": {"games": args.games, "sims": args.sims, "board": args.board, "precision": args.precision, "root_noise": [args.alpha, args.epsilon],
                                  "gpu_ms_per_round_off": off, "gpu_ms_per_round_on": on,
                                  "wall_ms_per_round_off": mean("off", lambda r: r["wall_ms_per_round"]), "wall_ms_per_round_on": mean("on", lambda r: r["wall_ms_per_round"]),
                                  "leaves_evaluated_per_round_off": mean("off", lambda r: r["leaves_evaluated_per_round"]),
                                  "leaves_evaluated_per_round_on": mean("on", lambda r: r["leaves_evaluated_per_round"]),
                                  "network_ms_per_round_off": mean("off", lambda r: r["ms_per_round"]["network"]),
                                  "network_ms_per_round_on": mean("on", lambda r: r["ms_per_round"]["network"]),
                                  "k_root_noise_ms_per_round": d_roots, "select_change_ms_per_round": d_select,
                                  "k_root_noise_share_of_round": d_roots / on, "select_change_share_of_round": d_select / on}}), flush=True)


if __name__ == "__main__":
    main()
