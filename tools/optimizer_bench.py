"""What the trainer's optimiser options cost on one GPU: the step with the options off and on, alternating in ONE process.

    python tools/optimizer_bench.py [--board 8] [--channels 512] [--batches 32,1024] [--steps 20] [--reps 3] [--out profiles/optimizer_bench.json]

Per batch size and repetition, in turn: options off (k_t_adam, the kernel every earlier version launched: the comparison), the decoupled decay alone
(k_t_adam_x on the same 7 streams), and everything (decay + global-norm clip + weight average + cosine schedule: 9 streams and the norm's read of
G).  Recorded: the wall time per step (forward_backward + apply), the HIP-event time of the optimiser kernel and of the norm's two kernels
(oz_trainer_time_optimizer: back-to-back launches on an idle device).  What the bytes predict: decay alone 1.0 x k_t_adam, everything 9 / 7 x, the
norm at most one read of G.  Prints one JSON document and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {
    "off": {},
    "decay": dict(weight_decay=1e-2),
    "all": dict(weight_decay=1e-2, global_clipnorm=1.0, average_decay=0.999, schedule=("cosine", 100, 10000, 0.1)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=8)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--batches", default="32,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "optimizer_bench.json"))
    args = ap.parse_args()
    from othellozero_amd.trainer import Trainer
    from othellozero_amd.weights import init_weights
    n, C = args.board, args.channels
    arena = Trainer.arena_size(n, C, 2)
    result = {"board": n, "channels": C, "arena_floats": arena, "arena_mb": arena * 4 / 1e6, "steps": args.steps, "reps": args.reps,
              "kernel_iters": args.kernel_iters, "modes": {k: {kk: list(vv) if isinstance(vv, tuple) else vv for kk, vv in v.items()} for k, v in MODES.items()},
              "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        tr = Trainer(n, C, 2, max_batch=B, seed=1)
        tr.set_weights(init_weights(n, seed=0, channels=C))
        rs = np.random.RandomState(0)
        valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
        own = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid
        opp = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid & ~own
        pi = rs.dirichlet(np.ones(n * n), B).astype(np.float32)
        z = rs.choice([-1.0, 1.0], B).astype(np.float32)
        rows = {m: {"ms_per_step": [], "kernel_ms": [], "reduction_ms": []} for m in MODES}
        for _ in range(args.reps):
            for mode, opt in MODES.items():
                tr.set_optimizer(**opt)
                for _ in range(args.warmup):
                    tr.forward_backward(own, opp, pi, z)
                    tr.apply()
                tr.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    tr.forward_backward(own, opp, pi, z)
                    tr.apply()
                tr.sync()
                rows[mode]["ms_per_step"].append(1e3 * (time.perf_counter() - t0) / args.steps)
                tr.forward_backward(own, opp, pi, z)               # a fresh gradient in the arena for the kernels' own timing
                tm = tr.time_optimizer(args.kernel_iters)
                rows[mode]["kernel_ms"].append(tm["kernel_ms"])
                rows[mode]["reduction_ms"].append(tm["reduction_ms"])
                tr.set_weights(init_weights(n, seed=0, channels=C))      # the timing hook moved the weights: every mode starts from the same ones
        for mode in MODES:
            for key in ("ms_per_step", "kernel_ms", "reduction_ms"):
                rows[mode][key + "_median"] = float(np.median(rows[mode][key]))
        base = rows["off"]["kernel_ms_median"]
        for mode in MODES:
            rows[mode]["kernel_vs_k_t_adam"] = rows[mode]["kernel_ms_median"] / base
            streams = 9 if "average_decay" in MODES[mode] else 7
            rows[mode]["kernel_gb_per_s"] = streams * arena * 4 / (rows[mode]["kernel_ms_median"] * 1e-3) / 1e9
        red = rows["all"]["reduction_ms_median"]
        rows["all"]["reduction_gb_per_s"] = arena * 4 / (red * 1e-3) / 1e9 if red > 0 else None
        result["batches"][str(B)] = rows
        del tr
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
