#!/usr/bin/env python3
"""What solved leaves cost per search step (solve_leaves=E, oz_selfplay_set_solve_leaves), and the sign-only solve next to the full one.

    python tools/solve_leaves_bench.py [--out profiles/solve_leaves_bench.json] [--games 4096] [--sims 100] [--precision bf16x3]
                                       [--steps 200] [--sims-pre 8]

One process, one engine at the BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a
random-init 512-filter OthelloNN, refilled slots) whose slots are spread over the plies of a game (SelfPlayEngine.stagger at `--sims-pre`
simulations per move, untimed), so that every batch holds leaves of every stage of the game.  E alternates over 0 / 4 / 6 / 8 / 10, three
repetitions each; a repetition is `--steps` network batches of the free-running driver (run_steps): wall ms per batch, the HIP-event ms of
k_solve_leaves per batch, rows solved per batch.  The comparison is against E = 0 in the same process; no threshold is set here.

Then oz_rules_solve_sign against oz_rules_solve on the 64-position sets of tools/solve_bench.py (HIP-event ms of one launch, median of 5
after a warm-up; the signs must equal the signs of the full solve's values)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
EMPTIES = (0, 4, 6, 8, 10)
REPEATS = 3


def bench_steps(args):
    import numpy as np
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G = 8, args.games
    net = NNetWrapper((n, n), max_batch=G, seed=1, precision=args.precision)
    eng = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=G, refill=True,
                         record_cap=int(G * ((1 + REPEATS * len(EMPTIES)) * args.steps / args.sims + n * n + 2) * 1.25))
    t0 = time.perf_counter()
    eng.stagger(args.sims_pre)
    stagger_s = time.perf_counter() - t0
    plies = eng.state()["ply"]
    eng.solve_leaves_profile(True)
    eng.run_steps(args.steps)                                            # warm-up, E = 0
    rows = []
    for rep in range(REPEATS):
        for E in EMPTIES:
            eng.set_solve_leaves(E)
            eng.solve_leaves_profile_read(reset=True)
            before, st0 = eng.rows_solved(), eng.stats()
            t0 = time.perf_counter()
            eng.run_steps(args.steps)
            wall = time.perf_counter() - t0
            ms, launches = eng.solve_leaves_profile_read(reset=True)
            st1 = eng.stats()
            assert launches == (args.steps if E else 0), (E, launches)
            rows.append(dict(E=E, repetition=rep, batches=args.steps, wall_ms_per_batch=1e3 * wall / args.steps,
                             kernel_ms_per_batch=ms / args.steps, rows_solved_per_batch=(eng.rows_solved() - before) / args.steps,
                             expansions_per_batch=(st1["expansions"] - st0["expansions"]) / args.steps,
                             moves=st1["moves"] - st0["moves"]))
            print(json.dumps(rows[-1]), flush=True)
    by_e = {}
    for E in EMPTIES:
        mine = [r for r in rows if r["E"] == E]
        by_e[str(E)] = {k: float(np.median([r[k] for r in mine])) for k in ("wall_ms_per_batch", "kernel_ms_per_batch", "rows_solved_per_batch")}
        by_e[str(E)]["wall_ms_per_batch_min_max"] = [min(r["wall_ms_per_batch"] for r in mine), max(r["wall_ms_per_batch"] for r in mine)]
    return dict(board=n, games=G, sims=args.sims, precision=args.precision, batches_per_repetition=args.steps, stagger_sims=args.sims_pre,
                stagger_wall_s=stagger_s, plies_min_median_max=[int(plies.min()), float(np.median(plies)), int(plies.max())],
                runs=rows, median_by_E=by_e)


def bench_sign():
    import numpy as np
    from othellozero_amd import _lib
    from othellozero_amd.agents import rules_solve, rules_solve_sign
    from solve_bench import SETS, playout_positions, timed
    _lib.check(_lib.load().oz_rules_profile(1))
    out = []
    for n, empties in SETS:
        pos = playout_positions(n, empties, seed=1000 * n + empties)
        b, w, p = ([q[i] for q in pos] for i in range(3))
        sign, solved = rules_solve_sign(b, w, p, n, empties)                 # warm-up, and the check
        _, _, value, _ = rules_solve(b, w, p, n, empties)
        assert solved.all() and np.array_equal(sign, np.sign(value).astype(np.int8)), (n, empties)
        ts = timed(lambda: rules_solve_sign(b, w, p, n, empties), 5)
        tf = timed(lambda: rules_solve(b, w, p, n, empties), 5)
        out.append(dict(board=n, empties=empties, positions=len(pos), sign_launch_ms_median=float(np.median(ts)), sign_launch_ms_runs=ts,
                        full_launch_ms_median=float(np.median(tf)), full_launch_ms_runs=tf,
                        wins_draws_losses=[int((sign > 0).sum()), int((sign == 0).sum()), int((sign < 0).sum())]))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=200, help="network batches per repetition")
    ap.add_argument("--sims-pre", type=int, default=8, help="simulations per move while the slots are spread over the plies")
    args = ap.parse_args()
    results = dict(steps=bench_steps(args), sign_vs_full=bench_sign())
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
