#!/usr/bin/env python3
"""What recording policy surprise (record_surprise=True, oz_selfplay_set_record_surprise) costs the self-play engine, and what one pass of
oz_selfplay_surprise_weights and one weighted append into the device replay buffer cost.

    python tools/surprise_bench.py [--out profiles/surprise_bench.json] [--games 4096] [--sims 100] [--precision bf16x3]
                                   [--steps 200] [--sims-pre 8] [--frac 0.5]

One process, one network, the BASELINE configs[1] shape (`--games` concurrent 8x8 self-play games, `--sims` simulations per move, a random-init
512-filter OthelloNN, refilled slots, the free-running driver), record_visits on in BOTH arms.  The option is set before an engine's first
driver call, so "off" and "on" are two engines on the same network, created alike and both spread over the plies of a game first
(SelfPlayEngine.stagger at `--sims-pre` simulations per move, untimed).  They take turns: three repetitions, in each of them `--steps` network
batches of run_steps() on the one, then on the other.  Per run: moves/s, expansions/s, leaves per batch.  After each repetition the "on"
engine computes the weights of every record it holds (SelfPlayEngine.surprise_weights, a synchronous call: wall time, records), and the
records are appended to a device replay buffer with room for all their examples, once plainly (8 examples per record) and once weighted
(c_i examples per record; its time includes the weights pass it starts with); the histogram of the copy counts of the last repetition is
kept.  The comparison is against off IN THE SAME REPETITION and against the spread of the repetitions; no threshold is set here: that off is
unchanged is shown by bit identity in the tests, not by timing.  Run it under a time limit (timeout 600 python tools/surprise_bench.py ...)."""
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
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.training import SelfPlayEngine
    n, G = 8, args.games
    net = NNetWrapper((n, n), max_batch=G, seed=1, precision=args.precision)
    record_cap = int(G * ((1 + REPEATS) * args.steps / args.sims + n * n + 2) * 1.5)
    engines, stagger_s = {}, {}
    for name, kw in (("off", {}), ("on", {"record_surprise": True})):
        eng = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, game_id_stride=G, refill=True, record_cap=record_cap,
                             record_visits=True, **kw)
        t0 = time.perf_counter()
        eng.stagger(args.sims_pre)
        stagger_s[name] = time.perf_counter() - t0
        eng.run_steps(args.steps)                                        # warm-up
        engines[name] = eng
    buf = ReplayBuffer(n, 10 * record_cap)
    rows, passes, histogram = [], [], {}
    for rep in range(REPEATS):
        for name, eng in engines.items():
            s0 = eng.stats()
            t0 = time.perf_counter()
            eng.run_steps(args.steps)
            wall = time.perf_counter() - t0
            s1 = eng.stats()
            assert s1["overflow"] == 0, s1
            moves = s1["moves"] - s0["moves"]
            rows.append(dict(option=name, repetition=rep, batches=args.steps, wall_ms_per_batch=1e3 * wall / args.steps,
                             moves=moves, moves_per_s=moves / wall, games_per_s=(s1["games_completed"] - s0["games_completed"]) / wall,
                             expansions_per_s=(s1["expansions"] - s0["expansions"]) / wall,
                             leaves_per_batch=(s1["leaves_evaluated"] - s0["leaves_evaluated"]) / args.steps,
                             simulations_per_move=(s1["simulations"] - s0["simulations"]) / max(moves, 1)))
            print(json.dumps(rows[-1]), flush=True)
        eng = engines["on"]
        eng.surprise_weights(args.frac, 99 + rep)                        # (the first call allocates the outputs)
        t0 = time.perf_counter()
        stats = eng.surprise_weights(args.frac, 99 + rep)
        weights_ms = 1e3 * (time.perf_counter() - t0)
        timed = {}
        for mode, kw in (("plain", {}), ("weighted", {"surprise_weight": (args.frac, 99 + rep)})):
            buf.clear()
            buf.append_engine(eng, policy_target="visits", **kw)         # (the first call allocates the staging)
            buf.clear()
            t0 = time.perf_counter()
            records = buf.append_engine(eng, policy_target="visits", **kw)
            timed[mode] = 1e3 * (time.perf_counter() - t0)
            timed[mode + "_examples"] = buf.total
        passes.append(dict(repetition=rep, frac=args.frac, records=stats["records"], examples=stats["examples"], max_copies=stats["max_copies"],
                           zero_copies=stats["zero_copies"], weights_wall_ms=weights_ms, append_records=records,
                           append_plain_wall_ms=timed["plain"], append_plain_examples=timed["plain_examples"],
                           append_weighted_wall_ms=timed["weighted"], append_weighted_examples=timed["weighted_examples"],
                           weighted_over_plain=timed["weighted"] / timed["plain"]))
        print(json.dumps(passes[-1]), flush=True)
        _, sur, (w, c, _) = eng.records(with_surprise=True, with_weights=True)
        values, counts = np.unique(c, return_counts=True)
        histogram = {str(int(v)): int(k) for v, k in zip(values, counts)}
        surprise = dict(mean=float(sur.mean()), median=float(np.median(sur)), max=float(sur.max()), zero=int((sur == 0).sum()),
                        mean_weight=float(w.astype(np.float64).mean()), max_weight=float(w.max()))
    ratios = []
    for rep in range(REPEATS):
        off, on = (next(r for r in rows if r["option"] == name and r["repetition"] == rep) for name in ("off", "on"))
        ratios.append({k: on[k] / off[k] if off[k] else float("nan") for k in RATES})
    median = {k: float(np.median([r[k] for r in ratios])) for k in RATES}
    per_option = {name: [r["moves_per_s"] for r in rows if r["option"] == name] for name in ("off", "on")}
    summary = dict(moves_per_s_off=float(np.median(per_option["off"])), moves_per_s_on=float(np.median(per_option["on"])),
                   moves_per_s_spread_off=(max(per_option["off"]) - min(per_option["off"])) / float(np.median(per_option["off"])),
                   moves_per_s_spread_on=(max(per_option["on"]) - min(per_option["on"])) / float(np.median(per_option["on"])),
                   weights_wall_ms=float(np.median([p["weights_wall_ms"] for p in passes])),
                   weights_records=int(np.median([p["records"] for p in passes])),
                   append_plain_wall_ms=float(np.median([p["append_plain_wall_ms"] for p in passes])),
                   append_weighted_wall_ms=float(np.median([p["append_weighted_wall_ms"] for p in passes])),
                   weighted_over_plain=float(np.median([p["weighted_over_plain"] for p in passes])))
    print(json.dumps(dict(on_over_off_median=median, **summary)), flush=True)
    return dict(board=n, games=G, sims=args.sims, precision=args.precision, batches_per_repetition=args.steps, stagger_sims=args.sims_pre,
                frac=args.frac, stagger_wall_s=stagger_s, runs=rows, weight_passes=passes, on_over_off_by_repetition=ratios,
                on_over_off_median=median, medians=summary, copies_histogram_last_repetition=histogram, surprise_last_repetition=surprise)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=200, help="network batches per repetition")
    ap.add_argument("--sims-pre", type=int, default=8, help="simulations per move while the slots are spread over the plies")
    ap.add_argument("--frac", type=float, default=0.5, help="frac of the timed weights pass and weighted append")
    args = ap.parse_args()
    results = bench(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
