#!/usr/bin/env python3
"""The launch plan of the network forward and the training step over a fixed matrix of shapes: which kernel, on which grid, with how much LDS.

    rocprofv3 --kernel-trace --output-format csv -d TRACE -- python tools/launch_plan_probe.py [--out DIR]     (kernel trace alone)
    python tools/launch_plan_probe.py --plan TRACE > profiles/launch_plan.txt

The first form creates, row by row, a network with seeded random weights (board 6 / 8 x max_batch 1 .. 4096 x the three precisions x the pattern
tables on / off) and runs one forward at full capacity and one at a ragged count, then one training step per (board, batch) of TRAIN_SHAPES in
the three precisions; --out keeps every row's (pi, v) as one .npy and, of a training row, every gradient and every weight after the step as one
.npz.  In front of a row's set-up and of each of its calls it launches the stub evaluator on a number of positions that encodes (row, phase), so
that the trace says where each begins.  The second form turns the trace into the launches of
the calls, in launch order: kernel, grid (threads; `a | b` = the full and the ragged call), workgroup, LDS bytes.  --plan TRACE --full lists
every launch of the run instead, set-up (commit, calibration) included: what two builds are compared on.
A change that is meant to leave every launch decision alone leaves both lists alone: diff the first against profiles/launch_plan.txt."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHANNELS = 512
PHASES = 3                                                           # markers per row: set-up, first call, second call
RAGGED = {32: 27, 128: 108, 512: 430, 1024: 860, 4096: 3640}        # (430 / 3640: the arena's and the bench's batch caps)
# training steps, in row order (rows are only ever appended: a row keeps its number).  8x8 at 32 / 1024: the reference's batch and a large one;
# 8: below the f16x2 weight-gradient kernel's smallest batch, one-launch BN both ways; 37: a partly filled octet; 256: the board-resident fp32
# weight gradient; 6x6 at 64: the second board size
TRAIN_SHAPES = ((8, 32), (8, 1024), (8, 8), (8, 37), (8, 256), (6, 64))


def rows():
    """the matrix, in run order: (label, kind, board, max_batch, precision, tables mode, counts)"""
    out = []
    for n in (6, 8):
        for mb in (1, 32, 128, 512, 1024, 4096):
            for prec in ("f32", "f16x2", "bf16x3"):
                for tables in (2, 0):
                    out.append((f"net {n}x{n} max_batch {mb} {prec} tables {tables}", "net", n, mb, prec, tables, [mb] + ([RAGGED[mb]] if mb in RAGGED else [])))
    for n, B in TRAIN_SHAPES:
        for prec in ("f32", "f16x2", "bf16x3"):
            out.append((f"train {n}x{n} batch {B} {prec}", "train", n, B, prec, 2, [B]))
    return out


def boards(n, count, seed):
    rs = np.random.RandomState(seed)
    a = rs.rand(count, n, n) < 0.4
    b = (rs.rand(count, n, n) < 0.4) & ~a
    bit = (np.uint64(1) << (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(8) + np.arange(n, dtype=np.uint64)[None, :]))
    return (a * bit).sum(axis=(1, 2), dtype=np.uint64), (b * bit).sum(axis=(1, 2), dtype=np.uint64)


def run(out_dir):
    from othellozero_amd.NNet import NNetWrapper, StubNetWrapper
    from othellozero_amd.trainer import Trainer
    from othellozero_amd.weights import init_weights
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    table = rows()
    stub = StubNetWrapper((8, 8), 1, 0, max_batch=PHASES * len(table))

    def marker(row, phase):                                  # phase 0: the row's set-up follows; 1, 2: its first / second call
        k = PHASES * row + phase + 1
        stub.predict_batch(np.ones(k, np.uint64), np.full(k, 2, np.uint64))
    weights = {n: init_weights(n, seed=70 + n, channels=CHANNELS, randomize_all=True) for n in (6, 8)}
    for i, (label, kind, n, mb, prec, tables, counts) in enumerate(table):
        marker(i, 0)
        own, opp = boards(n, mb, seed=1000 + i)
        if kind == "net":
            net = NNetWrapper((n, n), num_channels_1=CHANNELS, max_batch=mb, weights=weights[n], precision=prec)
            net.set_tables(tables)
            res = []
            for k, c in enumerate(counts):
                marker(i, k + 1)
                pi, v = net.predict_batch(own[:c], opp[:c])
                res.append(np.hstack([pi.reshape(c, -1), v[:, None]]))
            res = np.vstack(res)
            del net
        else:
            tr = Trainer(n, CHANNELS, 2, max_batch=mb, seed=1, precision=prec)
            tr.set_weights(init_weights(n, seed=0, channels=CHANNELS))
            rs = np.random.RandomState(i)
            pit = np.zeros((mb, n * n), np.float32)
            pit[np.arange(mb), rs.randint(0, n * n, mb)] = 1
            marker(i, 1)
            tr.forward_backward(own, opp, pit, rs.choice([-1.0, 1.0], mb).astype(np.float32))
            p, v = tr.outputs(mb)                           # the forward's heads, before the step is applied
            grads = tr.get_grads()
            tr.apply()
            tr.sync()
            res = np.hstack([p, v[:, None]])
            if out_dir:
                np.savez(os.path.join(out_dir, f"row{i:03d}_step.npz"), **{f"grad{k:02d}": g for k, g in grads.items()},
                         **{f"weight{k:02d}": w for k, w in enumerate(tr.get_weights())})
            del tr
        assert np.isfinite(res).all(), label
        if out_dir:
            np.save(os.path.join(out_dir, f"row{i:03d}.npy"), res)
        print(f"row {i + 1:3d} {label}: {res.shape[0]} positions", flush=True)


def plan(trace_dir, full=False):
    from trace_gaps import read_kernel_trace
    table = rows()
    calls = {}                                               # (row, phase) -> [(kernel, grid, workgroup, LDS bytes)]
    cur = None
    for r in sorted(read_kernel_trace(trace_dir), key=lambda r: int(r["Dispatch_Id"])):     # dispatch order = the host's launch order, whatever the stream
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        dims = lambda what: "x".join(r[f"{what}_Size_{a}"] for a in "XYZ").replace("x1x1", "")
        if name.endswith("k_stub"):
            cur = divmod(int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]) - 1, PHASES)
        elif cur and not name.startswith("__amd") and (full or cur[1]):       # (the runtime's own copy / fill kernels vary from run to run of one build)
            calls.setdefault(cur, []).append((name, dims("Grid"), dims("Workgroup"), r["LDS_Block_Size"]))
    lines, seen = [], {}
    for i, (label, kind, n, mb, prec, tables, counts) in enumerate(table):
        a, b = calls.get((i, 1), []), calls.get((i, 2), [])
        what = "one step" if kind == "train" else "calls of " + " | ".join(str(c) for c in counts) + " positions"
        lines.append(f"# row {i + 1}: {label} -- {what}")
        if full:
            body = [" ".join(x) for ph in range(PHASES) for x in [("## phase", str(ph), "", "")] + calls.get((i, ph), [])]
        elif b and [(x[0], x[2], x[3]) for x in a] == [(x[0], x[2], x[3]) for x in b]:
            body = [f"{x[0]}  {x[1]}{'' if x[1] == y[1] else ' | ' + y[1]}  wg {x[2]}  lds {x[3]}" for x, y in zip(a, b)]
        else:                                                # the two calls run different kernels (a tile chosen from the call's count): one after the other
            body = [f"{x[0]}  {x[1]}  wg {x[2]}  lds {x[3]}" for x in a] + ([f"-- the call of {counts[1]} positions"] if b else []) + \
                   [f"{x[0]}  {x[1]}  wg {x[2]}  lds {x[3]}" for x in b]
        key = "\n".join(body) or "(no launch of this row in the trace)"
        if not full and key in seen:
            lines.append(f"same launches as row {seen[key]}")
        else:
            seen.setdefault(key, i + 1)
            lines.extend(key.split("\n"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="directory for one .npy of (pi | v) per row (+ one .npz of gradients and stepped weights per training row)")
    ap.add_argument("--plan", default="", help="a rocprofv3 output directory of the probe: print its launch plan and exit")
    ap.add_argument("--full", action="store_true", help="with --plan: every launch of the run, set-up included")
    args = ap.parse_args()
    if args.plan:
        print("\n".join(plan(args.plan, args.full)))
    else:
        run(args.out)


if __name__ == "__main__":
    main()
