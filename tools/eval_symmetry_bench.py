#!/usr/bin/env python3
"""What the evaluation symmetry (NNetWrapper.set_eval_symmetry, oz_net_set_eval_symmetry) costs the self-play engine.

    python tools/eval_symmetry_bench.py [--out profiles/eval_symmetry_bench.json] [--games 4096] [--sims 100] [--precision bf16x3]
                                        [--steps 200] [--sims-pre 8] [--mean-games 512]

One process, ONE network of max_batch = `--games` (a random-init 512-filter OthelloNN), the BASELINE configs[1] shape: `--games` concurrent
8x8 self-play games, `--sims` simulations per move, refilled slots, the free-running driver.  The option lives in the network, so "off" and
"random" are two engines created alike on that network, both spread over the plies of a game first (SelfPlayEngine.stagger at `--sims-pre`
simulations per move, untimed), and the network is switched before each engine's turn.  They take turns: three repetitions, in each of them
`--steps` network batches of run_steps() on the one, then on the other.  Per run: expansions/s, moves/s, leaves per batch.  One more turn of
the "random" engine runs with HIP events around the option's two kernels (k_sym_boards, k_sym_policy): their cost per batch; it is not among
the timed repetitions.  Then the same with `--mean-games` games and "mean" (8 boards per leaf: 8 x games <= max_batch) against off.  The
comparison is against off IN THE SAME REPETITION; no threshold is set here: that off is unchanged is shown by bit identity in the tests."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 3
RATES = ("expansions_per_s", "moves_per_s", "leaves_per_batch")


def compare(net, mode, G, args):
    """off against `mode` with G games on `net`: (rows, ratios by repetition, kernel times of one profiled turn)"""
    import numpy as np
    from othellozero_amd.training import SelfPlayEngine
    n = 8
    engines, stagger_s = {}, {}
    for name in ("off", mode):
        net.set_eval_symmetry(name, 1)
        eng = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=G, refill=True,
                             record_cap=int(G * ((3 + REPEATS) * args.steps / args.sims + n * n + 2) * 1.5))
        t0 = time.perf_counter()
        eng.stagger(args.sims_pre)
        stagger_s[name] = time.perf_counter() - t0
        eng.run_steps(args.steps)                                        # warm-up
        engines[name] = eng
    rows = []
    for rep in range(REPEATS):
        for name, eng in engines.items():
            net.set_eval_symmetry(name, 1)
            s0 = eng.stats()
            t0 = time.perf_counter()
            eng.run_steps(args.steps)
            s1 = eng.stats()                                             # (waits for the engine's stream)
            wall = time.perf_counter() - t0
            assert s1["overflow"] == 0, s1
            rows.append(dict(games=G, option=name, repetition=rep, batches=args.steps, wall_ms_per_batch=1e3 * wall / args.steps,
                             moves_per_s=(s1["moves"] - s0["moves"]) / wall, expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall,
                             leaves_per_batch=(s1["leaves_evaluated"] - s0["leaves_evaluated"]) / args.steps))
            print(json.dumps(rows[-1]), flush=True)
    # the option's two kernels, event-timed, in a turn of their own
    net.set_eval_symmetry(mode, 1)
    net.eval_symmetry_profile(True, reset=True)
    engines[mode].run_steps(args.steps)
    engines[mode].stats()
    prof = net.eval_symmetry_profile(False)
    kernels = {k: dict(launches=c, us_per_launch=1e3 * ms / c if c else None) for k, (ms, c) in prof.items()}
    net.set_eval_symmetry("off")
    ratios = []
    for rep in range(REPEATS):
        off, on = (next(r for r in rows if r["option"] == name and r["repetition"] == rep) for name in ("off", mode))
        ratios.append({k: on[k] / off[k] if off[k] else float("nan") for k in RATES})
    summary = {f"{k}_{name}": float(np.median([r[k] for r in rows if r["option"] == name])) for name in ("off", mode) for k in ("expansions_per_s", "wall_ms_per_batch")}
    summary[f"{mode}_over_off_median"] = {k: float(np.median([r[k] for r in ratios])) for k in RATES}
    print(json.dumps(dict(games=G, mode=mode, kernels=kernels, **summary)), flush=True)
    return dict(games=G, mode=mode, stagger_wall_s=stagger_s, runs=rows, ratio_by_repetition=ratios, kernels_us=kernels, medians=summary)


def bench(args):
    from othellozero_amd.NNet import NNetWrapper
    net = NNetWrapper((8, 8), max_batch=args.games, seed=1, precision=args.precision)
    out = dict(board=8, sims=args.sims, precision=args.precision, max_batch=args.games, batches_per_repetition=args.steps, stagger_sims=args.sims_pre,
               random=compare(net, "random", args.games, args))
    if args.mean_games:
        assert 8 * args.mean_games <= args.games, "mean needs 8 x games <= max_batch"
        out["mean"] = compare(net, "mean", args.mean_games, args)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=200, help="network batches per repetition")
    ap.add_argument("--sims-pre", type=int, default=8, help="simulations per move while the slots are spread over the plies")
    ap.add_argument("--mean-games", type=int, default=512, help='games of the "mean" comparison on the same network (0: skip it)')
    args = ap.parse_args()
    results = bench(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
