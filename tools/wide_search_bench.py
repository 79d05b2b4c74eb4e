#!/usr/bin/env python3
"""What leaves_per_step (K descents per game and network batch under virtual loss) buys, measured against K = 1 IN THE SAME PROCESS
(K = 1 is the default code path).  K values alternate, --reps repetitions each, after a warm-up of every shape; one JSON line per
measurement and a summary table (mean, min .. max over the repetitions) at the end.

    python tools/wide_search_bench.py arena    [--games 512] [--sims 800] [--plies 4] [--precision f16x2] [--ks 1,2,4,8]
    python tools/wide_search_bench.py selfplay [--games 100] [--sims 25] [--board 6] [--ks 1,4,8]     (main.py's defaults)
    python tools/wide_search_bench.py episode  [--sims 25] [--ks 1,4,8]                               (one 8x8 drop-in game, configs[0])
    python tools/wide_search_bench.py strength [--games 512] [--sims 100]                             (one network against itself)

arena:    two real 512-filter networks, `plies` move rounds; us per SIMULATION = wall of oz_arena_run_rounds / (plies x sims), the mean
          number of leaves per network batch, and (one extra profiled run per K) the tree kernels' share of the GPU time.
          Every K gets networks created with max_batch = games x K: the network picks its tiles from that capacity.
strength: NOT a gate.  Random-initialised networks say little about playing strength."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arena_once(_lib, nets, n, G, sims, plies, k, profile=False):
    """one arena through the C ABI, timing oz_arena_run_rounds alone (creation allocates and clears the tables)"""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.oz_arena_create(C.byref(h), n, G, sims, 1.0, _lib.QMODE_F64, 11, 0, nets[0]._h, nets[1]._h, sims * (plies // 2 + 2) + 64))
    try:
        _lib.check(lib.oz_arena_set_dedup(h, 0))
        if k != 1:
            _lib.check(lib.oz_arena_set_leaves_per_step(h, k, k))
        if profile:
            _lib.check(lib.oz_arena_profile(h, 1))
        t0 = time.perf_counter()
        _lib.check(lib.oz_arena_run_rounds(h, plies))
        dt = time.perf_counter() - t0
        sa, sb = np.zeros(5, np.int64), np.zeros(5, np.int64)
        _lib.check(lib.oz_arena_stats(h, _lib.p_i64(sa), _lib.p_i64(sb)))
        ea, eb = C.c_int64(), C.c_int64()
        _lib.check(lib.oz_arena_leaves_evaluated(h, C.byref(ea), C.byref(eb)))
        tree = None
        if profile:
            ms, cnt = np.zeros(len(_lib.TREE_KERNELS), np.float64), np.zeros(len(_lib.TREE_KERNELS), np.int64)
            _lib.check(lib.oz_arena_profile_read(h, _lib.p_f64(ms), _lib.p_i64(cnt), 0))
            tree = {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(_lib.TREE_KERNELS)}
    finally:
        lib.oz_arena_destroy(h)
    return dt, sa + sb, ea.value + eb.value, tree


def table_arena(args):
    from othellozero_amd import _lib
    from othellozero_amd.NNet import NNetWrapper
    n, G = 8, args.games
    nets = {k: [NNetWrapper((n, n), num_channels_1=512, max_batch=G * k, seed=sd, precision=args.precision) for sd in (0, 1)] for k in args.ks}
    for k in args.ks:                                          # warm-up of every shape
        arena_once(_lib, nets[k], n, G, 16, 2, k)
    rows = {k: [] for k in args.ks}
    for rep in range(args.reps):
        for k in args.ks:
            dt, st, leaves, _ = arena_once(_lib, nets[k], n, G, args.sims, args.plies, k)
            us = dt / (args.plies * args.sims) * 1e6
            rows[k].append(us)
            print(json.dumps({"table": "arena", "precision": args.precision, "k": k, "rep": rep, "seconds": round(dt, 4), "us_per_simulation": round(us, 2),
                              "simulations": int(st[0]), "expansions": int(st[2]), "leaves_evaluated": int(leaves)}), flush=True)
    prof = {}
    for k in args.ks:
        dt, st, leaves, tree = arena_once(_lib, nets[k], n, G, args.sims, args.plies, k, profile=True)
        total = sum(ms for ms, _ in tree.values())
        batches = tree["network"][1]
        prof[k] = {"leaves_per_batch": round(leaves / max(batches, 1), 1), "network_batches": batches,
                   "tree_share": round(1.0 - tree["network"][0] / total, 4),
                   "us_per_launch": {name: round(ms / max(cnt, 1) * 1e3, 1) for name, (ms, cnt) in tree.items()}}
        print(json.dumps({"table": "arena_profile", "precision": args.precision, "k": k, **prof[k]}), flush=True)
    print(f"\narena, {G} games x {args.sims} sims x {args.plies} plies, {args.precision}: us per simulation (mean, min .. max of {args.reps}), leaves per batch, tree kernels' share of the GPU time")
    for k in args.ks:
        r = rows[k]
        print(f"  K = {k:2d}: {np.mean(r):8.1f}  ({min(r):.1f} .. {max(r):.1f})   {prof[k]['leaves_per_batch']:7.1f} leaves/batch   tree {100 * prof[k]['tree_share']:.1f} %   "
              f"descent {prof[k]['us_per_launch']['select']} us, network {prof[k]['us_per_launch']['network']} us per launch")


def table_selfplay(args):
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G = args.board, args.games
    nets = {k: NNetWrapper((n, n), num_channels_1=512, max_batch=max(128, G * k), seed=0, precision=args.precision) for k in args.ks}

    def once(k, seed):
        eng = SelfPlayEngine(nets[k], n, G, args.sims, 1.0, 1.0, 0.9, seed=seed, leaves_per_step=k)
        t0 = time.perf_counter()
        eng.play_to_end()
        dt = time.perf_counter() - t0
        return dt, eng.stats()
    for k in args.ks:
        once(k, 1)
    rows = {k: [] for k in args.ks}
    for rep in range(args.reps):
        for k in args.ks:
            dt, st = once(k, 1234)
            rows[k].append(dt)
            print(json.dumps({"table": "selfplay", "k": k, "rep": rep, "seconds": round(dt, 4), "moves": st["moves"], "simulations": st["simulations"],
                              "expansions": st["expansions"]}), flush=True)
    print(f"\nself-play, {G} games of {n}x{n} x {args.sims} sims to the end, {args.precision}: seconds (mean, min .. max of {args.reps})")
    for k in args.ks:
        print(f"  K = {k:2d}: {np.mean(rows[k]):7.3f}  ({min(rows[k]):.3f} .. {max(rows[k]):.3f})")


def table_episode(args):
    from othellozero_amd import training
    from othellozero_amd.NNet import NNetWrapper
    n = 8
    nets = {k: NNetWrapper((n, n), num_channels_1=512, max_batch=k, seed=0, precision=args.precision) for k in args.ks}
    made = []
    orig = training.OthelloMCTS

    def capture(*a, **kw):
        made.append(orig(*a, **kw))
        return made[-1]
    training.OthelloMCTS = capture

    def once(k):
        import random
        random.seed(5); np.random.seed(5)
        t0 = time.perf_counter()
        ex = training.execute_episode(n, nets[k], 1.0, args.sims, 1, 0.9, leaves_per_step=k)
        dt = time.perf_counter() - t0
        m = made.pop()
        batches = m.wide_stats()["steps"] if k > 1 else m.stats()["simulations"]
        return dt, len(ex) // 8, batches, m.stats()["expansions"]
    for k in args.ks:
        once(k)
    rows = {k: [] for k in args.ks}
    info = {}
    for rep in range(args.reps):
        for k in args.ks:
            dt, plies, batches, leaves = once(k)
            rows[k].append(dt)
            info[k] = (plies, batches, leaves)
            print(json.dumps({"table": "episode", "k": k, "rep": rep, "seconds": round(dt, 4), "plies": plies, "network_launches": batches, "leaves": leaves}), flush=True)
    print(f"\none 8x8 drop-in game, {args.sims} sims per move, {args.precision}: seconds per game (mean, min .. max of {args.reps}), network launches and leaves per game")
    for k in args.ks:
        print(f"  K = {k:2d}: {np.mean(rows[k]):7.3f}  ({min(rows[k]):.3f} .. {max(rows[k]):.3f})   {info[k][1]} launches, {info[k][2]} leaves, {info[k][0]} plies")


def table_strength(args):
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.agents import arena_batch
    n, G = 8, args.games
    net = NNetWrapper((n, n), num_channels_1=512, max_batch=G * 4, seed=0, precision=args.precision)
    print(f"one random-initialised network against itself, {G} games, {args.sims} sims per move, {args.precision} (weak evidence: an untrained network)")
    for ks in ((1, 1), (1, 4), (4, 1)):
        r = arena_batch(net, net, n, G, args.sims, 1.0, seed=3, first_game_id=0, leaves_per_step=ks)
        bw = r["winner"] == 1
        row = {"table": "strength", "k_black": ks[0], "k_white": ks[1], "black_wins": int(bw.sum()), "white_wins": int((~bw).sum()),
               "black_mean_points_when_winning": round(float(r["points"][bw].mean()) if bw.any() else 0.0, 2),
               "white_mean_points_when_winning": round(float(r["points"][~bw].mean()) if (~bw).any() else 0.0, 2)}
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("table", choices=["arena", "selfplay", "episode", "strength"])
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--sims", type=int, default=None)
    ap.add_argument("--plies", type=int, default=4)
    ap.add_argument("--board", type=int, default=6)
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--ks", default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dflt = {"arena": (512, 800, "1,2,4,8"), "selfplay": (100, 25, "1,4,8"), "episode": (1, 25, "1,4,8"), "strength": (512, 100, "1,4")}[args.table]
    args.games = args.games or dflt[0]
    args.sims = args.sims or dflt[1]
    args.ks = [int(x) for x in (args.ks or dflt[2]).split(",")]
    from othellozero_amd import _lib
    _lib.require_gpu()
    {"arena": table_arena, "selfplay": table_selfplay, "episode": table_episode, "strength": table_strength}[args.table](args)


if __name__ == "__main__":
    main()
