#!/usr/bin/env python3
"""What the minimax opponent costs in an evaluation arena, and that it is harder than the random mover.

    python tools/minimax_arena_depths.py [--games 512] [--sims 100] [--board 8] [--reps 1] [--precision bf16x3] [--out FILE]

One process, one device.  For a `--games`-game arena of a random-init 512-filter network (BLACK) at `--sims` simulations per move: the wall time
against the random mover (the default), then against minimax at depths 1, 2, 3, 4 and 6 (weighted), with the HIP-event time per launch of
k_arena_minimax_move (oz_arena_opponent_time).  From network-free arenas of the same size: the games a random BLACK wins against each of
those opponents as WHITE, and the other way round.  Writes a text table (default: stdout)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEPTHS = (1, 2, 3, 4, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--board", type=int, default=8)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from othellozero_amd import _lib
    from othellozero_amd.agents import arena_batch
    from othellozero_amd.NNet import NNetWrapper
    _lib.require_gpu()
    n, G = args.board, args.games
    net = NNetWrapper((n, n), max_batch=G, seed=1, precision=args.precision)
    lines = [f"{G}-game {n}x{n} evaluation arena, {args.sims} simulations per move, random-init 512-filter network ({args.precision}) as BLACK, "
             f"one process, {args.reps} repetition(s) per row (the first arena of the process, not in the table, pays allocation and code load)",
             "", "opponent (WHITE)       wall s    plies  network wins   k_arena_minimax_move: launches   ms total   ms per launch"]

    def row(label, opponent, out):
        for rep in range(args.reps):
            t0 = time.perf_counter()
            r = arena_batch(net, None, n, G, args.sims, 1.0, seed=7, opponent=opponent, profile=True)
            dt = time.perf_counter() - t0
            ms, cnt = r.get("opponent_kernel") or (0.0, 0)
            out.append(f"{label:<20} {dt:8.3f} {int(r['n_moves'].sum()):8d} {int((r['winner'] == 1).sum()):8d}/{G}"
                       + (f" {cnt:32d} {ms:10.3f} {ms / max(cnt, 1):14.4f}" if cnt else ""))
            print(out[-1], flush=True)

    row("warm-up", None, [])
    row("random", None, lines)
    for d in DEPTHS:
        row(f"minimax depth {d}", ("minimax", d, "weighted"), lines)
    lines += ["", f"network-free arenas, {G} games each (4 'simulations' configured, none run): games won by the minimax side against the random mover",
              "minimax (weighted)    as WHITE   as BLACK   (a draw goes to BLACK)"]
    for d in DEPTHS:
        w = arena_batch(None, None, n, G, 4, 1.0, seed=9, opponent={"white": ("minimax", d)})
        b = arena_batch(None, None, n, G, 4, 1.0, seed=9, opponent={"black": ("minimax", d)})
        lines.append(f"depth {d:<14} {int((w['winner'] == -1).sum()):8d}/{G} {int((b['winner'] == 1).sum()):6d}/{G}")
        print(lines[-1], flush=True)
    rr = arena_batch(None, None, n, G, 4, 1.0, seed=9)
    lines.append(f"random (for scale)   {int((rr['winner'] == -1).sum()):8d}/{G} {int((rr['winner'] == 1).sum()):6d}/{G}")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
