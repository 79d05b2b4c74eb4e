#!/usr/bin/env python3
"""What the Gumbel search costs a lock-step move round, measured against the same engine without it IN THE SAME PROCESS.

    python tools/gumbel_bench.py [--games 4096] [--sims 100] [--board 8] [--rounds 6] [--reps 3] [--precision bf16x3] [--out profiles/gumbel_bench.json]

Per setting (option off / on, taking turns, --reps engines each): a continuous engine (refill) is warmed up, then `rounds` move rounds of
oz_selfplay_run are timed on the wall clock with the HIP-event profile of the tree kernels on (oz_selfplay_profile_read).  The two kernels the
option adds to a round, k_gumbel_arm (after the roots kernel) and the Gumbel move (k_sp_move<VALUES+GUMBEL> with the improved policy, in place of
k_sp_move), are both timed in the roots_move slot: their cost is that slot's difference; the depth-0 pick sits in the select slot (the fused
expand + backup + descent launches).  One JSON line per engine, and a summary -- moves/s per setting, the on-over-off ratio per repetition with
its spread -- printed and written to --out.  Playing strength is not measured.

Cross-game leaf de-duplication is OFF in both engines (--dedup to switch it on): a fresh engine's games all start from the opening, and
without Gumbel noise thousands of them walk the same few positions for many plies, so with de-duplication the option-off engine evaluates a
twentieth of the leaves the option-on engine does (11.8 k against 227 k per round, measured) and the comparison measures the network's batch
size, not the search.  With it off both engines evaluate one leaf per game and step."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one_engine(args, net, gumbel):
    from othellozero_amd import _lib
    from othellozero_amd.training import SelfPlayEngine
    eng = SelfPlayEngine(net, args.board, args.games, args.sims, 1.0, 1.0, 0.9, seed=7, refill=True, dedup=args.dedup, gumbel=gumbel)
    eng.profile(True)
    eng.run(args.warmup)
    eng.profile_read(reset=True)
    s0 = eng.stats()
    t0 = time.perf_counter()
    eng.run(args.rounds)
    wall = time.perf_counter() - t0
    prof, s1 = eng.profile_read(), eng.stats()
    out = {"gumbel": gumbel, "rounds": args.rounds, "wall_ms_per_round": 1e3 * wall / args.rounds,
           "moves_per_s": (s1["moves"] - s0["moves"]) / wall,
           "ms_per_round": {k: prof[k][0] / args.rounds for k in _lib.TREE_KERNELS},
           "launches_per_round": {k: prof[k][1] / args.rounds for k in _lib.TREE_KERNELS}}
    out["gpu_ms_per_round"] = sum(out["ms_per_round"].values())
    out["leaves_evaluated_per_round"] = (s1["leaves_evaluated"] - s0["leaves_evaluated"]) / args.rounds
    out["gumbel_moves"] = eng.gumbel_stats()["moves"]
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
    ap.add_argument("--max-considered", type=int, default=16)
    ap.add_argument("--c-visit", type=float, default=50.0)
    ap.add_argument("--c-scale", type=float, default=1.0)
    ap.add_argument("--dedup", action="store_true", help="cross-game leaf de-duplication on (see the module docstring)")
    ap.add_argument("--out", default=os.path.join("profiles", "gumbel_bench.json"))
    args = ap.parse_args()
    from othellozero_amd import _lib
    from othellozero_amd.NNet import NNetWrapper
    _lib.require_gpu()
    net = NNetWrapper((args.board, args.board), num_channels_1=args.channels, max_batch=args.games, seed=0, precision=args.precision)
    gumbel = (args.max_considered, args.c_visit, args.c_scale)
    runs = {"off": [], "on": []}
    for _ in range(args.reps):
        for name, opt in (("off", None), ("on", gumbel)):
            r = one_engine(args, net, opt)
            runs[name].append(r)
            print(json.dumps({"setting": name, **r}), flush=True)

    def mean(name, f):
        return sum(f(r) for r in runs[name]) / len(runs[name])

    def spread(name):
        v = [r["moves_per_s"] for r in runs[name]]
        return (max(v) - min(v)) / (sum(v) / len(v))
    ratios = [on["moves_per_s"] / off["moves_per_s"] for off, on in zip(runs["off"], runs["on"])]
    d_roots = mean("on", lambda r: r["ms_per_round"]["roots_move"]) - mean("off", lambda r: r["ms_per_round"]["roots_move"])
    d_select = mean("on", lambda r: r["ms_per_round"]["select"]) - mean("off", lambda r: r["ms_per_round"]["select"])
    summary = {"games": args.games, "sims": args.sims, "board": args.board, "precision": args.precision, "gumbel": list(gumbel),
               "rounds": args.rounds, "reps": args.reps, "dedup": bool(args.dedup),
               "moves_per_s_off": [r["moves_per_s"] for r in runs["off"]], "moves_per_s_on": [r["moves_per_s"] for r in runs["on"]],
               "on_over_off": ratios, "on_over_off_median": sorted(ratios)[len(ratios) // 2],
               "spread_off": spread("off"), "spread_on": spread("on"),
               "gpu_ms_per_round_off": mean("off", lambda r: r["gpu_ms_per_round"]), "gpu_ms_per_round_on": mean("on", lambda r: r["gpu_ms_per_round"]),
               "network_ms_per_round_off": mean("off", lambda r: r["ms_per_round"]["network"]),
               "network_ms_per_round_on": mean("on", lambda r: r["ms_per_round"]["network"]),
               "leaves_evaluated_per_round_off": mean("off", lambda r: r["leaves_evaluated_per_round"]),
               "leaves_evaluated_per_round_on": mean("on", lambda r: r["leaves_evaluated_per_round"]),
               "arm_plus_gumbel_move_ms_per_round": d_roots, "select_change_ms_per_round": d_select,
               "select_change_us_per_launch": 1e3 * d_select / args.sims}
    print(json.dumps({"summary": summary}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"summary": summary, "runs": runs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
