"""What the trainer's auxiliary heads cost, and that the default path costs what it did (one GPU).

    python tools/aux_heads_bench.py [--parent DIR] [--out profiles/aux_heads_bench.json] [--reps 3]

Three measurements, every one with the two sides taking turns and `reps` repetitions (the median and the spread max - min of the repetitions
are what is reported; a difference inside the spread is no difference):
  step      8x8, 512 filters, batch 32 and 1024, precision f32 and bf16x3: a trainer with the heads off and one with them on (weights 1.0 / 0.25)
            in ONE process, the step-wise step (forward_backward + apply, a host synchronisation per step) and the resident epoch
            (oz_trainer_fit_epoch: the steps back to back on the device), ms per step;
  default   tools/train_bench.py of this tree and of the parent commit's tree (--parent: a checkout of the parent with its library built), one
            process per run, the same four shapes: the default path against the parent's;
  append    about 35 k records of an 8x8 engine (stub network, 8 simulations, visit counts and surprises recorded) appended plain (8 examples per
            record) and weighted (policy surprise weighting) into a buffer with and without the final pairs, ms per append.
Without --parent the `default` section is left out (and says so)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, "f32"), (32, "bf16x3"), (1024, "f32"), (1024, "bf16x3")]
N, C = 8, 512


def summary(xs):
    return dict(reps=[round(x, 4) for x in xs], median=round(statistics.median(xs), 4), spread=round(max(xs) - min(xs), 4))


def batch(B, seed):
    rs = np.random.RandomState(seed)
    valid = np.uint64(sum(1 << (r * 8 + c) for r in range(N) for c in range(N)))
    own = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid
    opp = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid & ~own
    pi = np.zeros((B, N * N), np.float32)
    pi[np.arange(B), rs.randint(0, N * N, B)] = 1
    z = rs.choice([-1.0, 1.0], B).astype(np.float32)
    fo = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid
    fp = valid & ~fo
    dead = rs.rand(B) < 0.25                       # a quarter of the examples without a final board, as adjudicated games leave them
    fo[dead] = 0
    fp[dead] = 0
    return own, opp, pi, z, fo, fp


def bench_step(reps):
    from othellozero_amd.trainer import Trainer
    from othellozero_amd.weights import init_weights
    out = []
    w = init_weights(N, seed=0, channels=C)
    for B, precision in SHAPES:
        steps = 60 if B == 32 else 12
        own, opp, pi, z, fo, fp = batch(B, 1)
        data = [np.tile(a, (steps,) + (1,) * (a.ndim - 1)) for a in (own, opp, pi, z, fo, fp)]
        order = np.arange(steps * B, dtype=np.int32)
        sides = {}
        for name, aux in (("off", None), ("on", dict(ownership=1.0, score=0.25))):
            tr = Trainer(N, C, 2, max_batch=B, seed=1, precision=precision, aux_heads=aux)
            tr.set_weights(w)
            extra = (fo, fp) if aux else ()
            for _ in range(3):
                tr.forward_backward(own, opp, pi, z, *extra)
                tr.apply()
            tr.set_dataset(*data[:4], *(data[4:] if aux else ()))
            tr.fit_epoch(order[:3 * B], B)
            tr.sync()
            sides[name] = (tr, extra)
        t = {(name, kind): [] for name in sides for kind in ("stepwise", "resident")}
        for _ in range(reps):
            for name, (tr, extra) in sides.items():          # the two trainers take turns
                t0 = time.perf_counter()
                for _ in range(steps):
                    tr.forward_backward(own, opp, pi, z, *extra)
                    tr.apply()
                tr.sync()
                t[name, "stepwise"].append(1e3 * (time.perf_counter() - t0) / steps)
                t0 = time.perf_counter()
                tr.fit_epoch(order, B)
                tr.sync()
                t[name, "resident"].append(1e3 * (time.perf_counter() - t0) / steps)
        row = dict(batch=B, precision=precision, steps=steps)
        for kind in ("stepwise", "resident"):
            off, on = summary(t["off", kind]), summary(t["on", kind])
            row[kind] = dict(off_ms_per_step=off, on_ms_per_step=on, cost_us_per_step=round(1e3 * (on["median"] - off["median"]), 1))
        print(json.dumps(row), flush=True)
        out.append(row)
        del sides
    return out


def bench_default(parent, reps):
    if not parent:
        return dict(skipped="no --parent tree given")
    out = []
    for B, precision in SHAPES:
        steps = 60 if B == 32 else 12
        t = {"this": [], "parent": []}
        for _ in range(reps):
            for name, cwd in (("this", ROOT), ("parent", os.path.abspath(parent))):      # the two trees take turns, one process per run
                r = subprocess.run([sys.executable, os.path.join("tools", "train_bench.py"), "--batch", str(B), "--precision", precision, "--steps", str(steps)],
                                   cwd=cwd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"train_bench.py failed in {cwd}:\n{r.stdout}\n{r.stderr}")
                t[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
        a, b = summary(t["this"]), summary(t["parent"])
        row = dict(batch=B, precision=precision, steps=steps, this_ms_per_step=a, parent_ms_per_step=b,
                   difference_ms=round(a["median"] - b["median"], 4), inside_spread=abs(a["median"] - b["median"]) <= max(a["spread"], b["spread"]))
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_append(reps):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.training import SelfPlayEngine
    G = 600
    eng = SelfPlayEngine(StubNetWrapper((N, N), 21, 0, max_batch=G), N, G, 8, 1.0, 1.0, 0.8, seed=5, record_visits=True, record_surprise=True)
    eng.play_to_end()
    records = int(eng.stats()["records"])
    bufs = {"plain": ReplayBuffer(N, 16 * records), "aux": ReplayBuffer(N, 16 * records, aux=True)}
    kinds = {"plain_append": dict(policy_target="visits"), "weighted_append": dict(policy_target="visits", surprise_weight=(0.5, 9))}
    eng.surprise_weights(0.5, 9)                     # (the weighted append recomputes them every time: part of what it costs on both sides)
    t = {(k, b): [] for k in kinds for b in bufs}
    for rep in range(reps + 1):                      # repetition 0 warms both buffers and both kernels up
        for k, kw in kinds.items():
            for b, buf in bufs.items():
                buf.clear()
                t0 = time.perf_counter()
                buf.append_engine(eng, **kw)
                if rep:
                    t[k, b].append(1e3 * (time.perf_counter() - t0))
    out = dict(records=records)
    for k in kinds:
        p, a = summary(t[k, "plain"]), summary(t[k, "aux"])
        out[k] = dict(plain_ms=p, aux_ms=a, cost_ms=round(a["median"] - p["median"], 4), examples=len(bufs["aux"]) if k == "weighted_append" else 8 * records)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_heads_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from othellozero_amd import _lib
    _lib.require_gpu()
    result = dict(board=N, channels=C, reps=args.reps, aux_weights=dict(ownership=1.0, score=0.25),
                  step=bench_step(args.reps), append=bench_append(args.reps), default_path_vs_parent=bench_default(args.parent, args.reps))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
