"""Times the held-out evaluation (oz_trainer_evaluate_dataset: inference-mode forward + metrics) next to a training epoch
(oz_trainer_fit_epoch) over the same resident examples, in one process on one GPU.

    python tools/evaluate_bench.py [--board 8] [--channels 512] [--examples 32768] [--batches 32,1024] [--reps 3] [--out profiles/evaluate_bench.json]

Per precision (f32, f16x2, bf16x3) and batch size: one trainer (max_batch = the batch), the examples uploaded once, both calls warmed up on four
batches, then `reps` repetitions that ALTERNATE one evaluation pass and one training epoch over all examples.  Both calls are synchronous (they end
in a stream synchronise), so the host clock around them is the device time plus one call's overhead.  Reported: ms per example of each (median, min
and max of the repetitions) and their ratio.  Expectation, not a threshold: a forward is roughly a third of a step's GEMM work (forward + data
gradient + weight gradient), and at batch 32 the per-launch boundaries dominate both.  Needs a GPU: no fall-back.  Synthetic data (random boards,
one-hot targets): the epochs really train, so the weights drift from their initial values during the run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=8)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--examples", type=int, default=32768)
    ap.add_argument("--batches", default="32,1024")
    ap.add_argument("--precisions", default="f32,f16x2,bf16x3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    from othellozero_amd import _lib
    from othellozero_amd.trainer import Trainer
    from othellozero_amd.weights import init_weights
    n, C, N = args.board, args.channels, args.examples
    rs = np.random.RandomState(0)
    valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
    own = rs.randint(0, 2**63, size=N, dtype=np.uint64) & valid
    opp = rs.randint(0, 2**63, size=N, dtype=np.uint64) & valid & ~own
    pi = np.zeros((N, n * n), np.float32)
    pi[np.arange(N), rs.randint(0, n * n, N)] = 1
    z = rs.choice([-1.0, 0.0, 1.0], N, p=[0.45, 0.1, 0.45]).astype(np.float32)
    order = np.arange(N, dtype=np.int32)
    rows = []
    for precision in args.precisions.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            row = {"precision": precision, "batch": B}
            try:
                tr = Trainer(n, C, 2, max_batch=B, seed=1, precision=precision)
                tr.set_weights(init_weights(n, seed=0, channels=C))
                tr.set_dataset(own, opp, pi, z)
                warm = order[:min(N, 4 * B)]
                tr.evaluate_dataset(warm, B)
                tr.fit_epoch(warm, B)
                tr.evaluate_dataset(warm, B)
                ev, fit = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    res = tr.evaluate_dataset(order, B)
                    t1 = time.perf_counter()
                    losses = tr.fit_epoch(order, B)
                    t2 = time.perf_counter()
                    ev.append(1e3 * (t1 - t0) / N)
                    fit.append(1e3 * (t2 - t1) / N)
                row.update(evaluate_ms_per_example=_spread(ev), fit_epoch_ms_per_example=_spread(fit),
                           evaluate_over_fit=_spread(ev)["median"] / _spread(fit)["median"], evaluate_ms_per_example_reps=ev,
                           fit_epoch_ms_per_example_reps=fit, last_evaluation=res, last_epoch_losses=[float(x) for x in losses])
                del tr
            except _lib.OzError as e:                       # recorded, not hidden: the row says what failed
                row["error"] = str(e)
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"metric": "evaluate_vs_fit_epoch_ms_per_example", "board": n, "channels": C, "examples": N, "reps": args.reps, "data": "synthetic",
           "clock": "host perf_counter around synchronous calls", "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
