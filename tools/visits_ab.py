"""Same-process A/B of oz_selfplay_config.record_visits: expansions/s of the free-running engine with the switch off and on, in
alternating legs on one network, then the time of oz_examples_expand_visits on the records the `on` engine completed.

    python tools/visits_ab.py [--games 4096] [--sims 100] [--channels 512] [--precision bf16x3] [--steps 10] [--rounds 2]

Defaults are bench.py's configs[1] size (4096 8x8 games, 100 simulations per move, bf16x3, free-running, refill, staggered slots).
Prints one JSON line: per leg the expansions/s, the on/off ratio of the sums, and the expansion's wall time (host copies included) and
records per call."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--board", type=int, default=8)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=10, help="timed steps per leg (a step = `sims` network batches)")
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs")
    ap.add_argument("--save", default=None, help="write the `on` engine's records and visit counts to this .npz (e.g. to profile the expansion alone)")
    args = ap.parse_args()
    from othellozero_amd import _lib
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.training import SelfPlayEngine, expand_examples, preferred_batch_cap
    n, G = args.board, args.games
    net = NNetWrapper((n, n), num_channels_1=args.channels, max_batch=G, seed=0, precision=args.precision)
    engines = {}
    for on in (False, True):
        e = SelfPlayEngine(net, n, G, args.sims, 1.0, 1.0, 0.9, seed=1234, q_mode=_lib.QMODE_F64, refill=True,
                           record_cap=int(G * (args.rounds * args.steps + 4 + n * n) * 1.25), dedup=False,
                           batch_cap=preferred_batch_cap(n, G, args.channels, args.precision), record_visits=on)
        e.stagger(args.sims)
        e.run_steps(2 * args.sims)                   # warm-up
        engines[on] = e
    legs = []
    for _ in range(args.rounds):
        for on in (False, True):
            e = engines[on]
            a = e.stats()["expansions"]
            t = time.perf_counter()
            e.run_steps(args.steps * args.sims)
            dt = time.perf_counter() - t
            legs.append({"record_visits": on, "expansions_per_s": (e.stats()["expansions"] - a) / dt, "s": dt})
    tot = {on: sum(x["expansions_per_s"] for x in legs if x["record_visits"] == on) for on in (False, True)}
    rec, cnt = engines[True].records(with_visits=True)
    if args.save:
        import numpy as np
        np.savez(args.save, records=rec, counts=cnt)
    times = []
    for _ in range(3):
        t = time.perf_counter()
        expand_examples(rec, n, visits=cnt, target_temperature=1.0)
        times.append(time.perf_counter() - t)
    t = time.perf_counter()
    expand_examples(rec, n)
    onehot_s = time.perf_counter() - t
    print(json.dumps({"games": G, "sims": args.sims, "precision": args.precision, "legs": legs,
                      "on_over_off": tot[True] / tot[False], "records": int(rec.size),
                      "expand_visits_wall_s": min(times), "expand_onehot_wall_s": onehot_s}))


if __name__ == "__main__":
    main()
