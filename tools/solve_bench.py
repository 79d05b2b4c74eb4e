#!/usr/bin/env python3
"""What the exact endgame solver costs (oz_rules_solve, oz_selfplay_solve_records).

    python tools/solve_bench.py [--out profiles/solve_bench.json] [--games 4096] [--sims 100] [--precision bf16x3] [--step-timeout 300]

Sets of 64 positions from fixed-seed random playouts at 6, 8, 10 and 12 empties on 8x8 and at 10 on 6x6.  Per set: the HIP-event time of one
oz_rules_solve launch over the 64 positions (median of 5 after one warm-up; oz_rules_profile) and the slowest single position (each of the 64
solved alone, one launch each).  On the 6-empties set also oz_rules_minimax(depth 6, discs), the same function there, in the same run.  Then
solve_records(10) after `--games` self-play games of 8x8 on a random-init 512-filter network, next to the wall time of those games.

Every step is a child process of its own under `timeout`; the first one that fails, faults or runs out of time ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETS = [(8, 6), (8, 8), (8, 10), (6, 10), (8, 12)]                  # the longest launches last
POSITIONS = 64


def playout_positions(n, empties, seed, want=POSITIONS, games=512):
    """the first `want` games (by index) of `games` uniformly random playouts that reach `empties` empties unfinished: their positions there"""
    import numpy as np
    from othellozero_amd import _lib
    lib = _lib.require_gpu()
    rng = np.random.RandomState(seed)
    h = n // 2
    white0 = (1 << ((h - 1) * 8 + h - 1)) | (1 << (h * 8 + h))
    black0 = (1 << ((h - 1) * 8 + h)) | (1 << (h * 8 + h - 1))
    black, white = np.full(games, black0, np.uint64), np.full(games, white0, np.uint64)
    player, fin = np.ones(games, np.int8), np.zeros(games, np.uint8)
    found = {}
    for _ in range(n * n):
        occupied = np.array([bin(int(b | w)).count("1") for b, w in zip(black, white)])
        for g in np.nonzero((n * n - occupied == empties) & (fin == 0))[0]:
            found.setdefault(int(g), (int(black[g]), int(white[g]), int(player[g])))
        live = np.nonzero(fin == 0)[0]
        if live.size == 0 or occupied[live].min() > n * n - empties:
            break
        own = np.where(player[live] == 1, black[live], white[live]).astype(np.uint64)
        opp = np.where(player[live] == 1, white[live], black[live]).astype(np.uint64)
        legal = np.zeros(live.size, np.uint64)
        _lib.check(lib.oz_rules_legal_moves(_lib.p_u64(own), _lib.p_u64(opp), n, live.size, _lib.p_u64(legal)))
        sq = np.zeros(live.size, np.uint8)
        for i, m in enumerate(legal):
            moves = [s for s in range(64) if (int(m) >> s) & 1]
            sq[i] = moves[rng.randint(len(moves))]
        b, w, p, f = (np.ascontiguousarray(a[live]) for a in (black, white, player, fin))
        bo, wo, po, fo = np.zeros_like(b), np.zeros_like(w), np.zeros_like(p), np.zeros_like(f)
        _lib.check(lib.oz_rules_play(_lib.p_u64(b), _lib.p_u64(w), _lib.p_i8(p), _lib.p_u8(sq), n, live.size, _lib.p_u64(bo), _lib.p_u64(wo),
                                     _lib.p_i8(po), _lib.p_u8(fo)))
        black[live], white[live], player[live], fin[live] = bo, wo, po, fo
    picked = [found[g] for g in sorted(found)][:want]
    assert len(picked) == want, f"only {len(picked)} of {games} playouts reach {empties} empties unfinished"
    return picked


def timed(call, runs):
    """HIP-event ms of the kernel of each of `runs` calls"""
    import ctypes as C
    from othellozero_amd import _lib
    lib, out = _lib.load(), []
    for _ in range(runs):
        _lib.check(lib.oz_rules_profile_read(None, None, 1))
        call()
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(lib.oz_rules_profile_read(C.byref(ms), C.byref(cnt), 1))
        assert cnt.value == 1
        out.append(ms.value)
    return out


def step_set(n, empties):
    import numpy as np
    from othellozero_amd import _lib
    from othellozero_amd.agents import rules_minimax, rules_solve
    pos = playout_positions(n, empties, seed=1000 * n + empties)
    _lib.check(_lib.load().oz_rules_profile(1))
    b, w, p = ([q[i] for q in pos] for i in range(3))
    rules_solve(b, w, p, n, empties)                                               # warm-up
    batch = timed(lambda: rules_solve(b, w, p, n, empties), 5)
    alone = [timed(lambda i=i: rules_solve(b[i:i + 1], w[i:i + 1], p[i:i + 1], n, empties), 1)[0] for i in range(len(pos))]
    out = dict(board=n, empties=empties, positions=len(pos), launch_ms_median=float(np.median(batch)), launch_ms_runs=batch,
               slowest_position_ms=max(alone), median_position_ms=float(np.median(alone)), fastest_position_ms=min(alone))
    if empties == 6:
        values, bests, _, _ = rules_solve(b, w, p, n, empties)
        mv, mb = rules_minimax(b, w, p, n, 6, "discs")
        assert np.array_equal(values, mv) and np.array_equal(bests, mb)
        mm = timed(lambda: rules_minimax(b, w, p, n, 6, "discs"), 5)
        out.update(minimax_depth6_discs_ms_median=float(np.median(mm)), minimax_depth6_discs_ms_runs=mm)
    return out


def step_records(games, sims, precision):
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n = 8
    net = NNetWrapper((n, n), max_batch=games, seed=1, precision=precision)
    eng = SelfPlayEngine(net, n, games, sims, 1.0, 1.0, 0.9, seed=1234)
    t0 = time.perf_counter()
    for _ in range(n * n):
        eng.run(4)
        if eng.stats()["live_games"] == 0:
            break
    selfplay_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    stats = eng.solve_records(10)
    solve_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    again = eng.solve_records(10)
    second_s = time.perf_counter() - t0
    assert again["z_changed"] == 0 and again["solved"] == stats["solved"]
    return dict(board=n, games=games, sims=sims, precision=precision, selfplay_wall_s=selfplay_s, solve_records_10_wall_s=solve_s,
                solve_records_10_second_call_wall_s=second_s, stats=stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        kind, *rest = args.step.split(":")
        res = step_set(int(rest[0]), int(rest[1])) if kind == "set" else step_records(args.games, args.sims, args.precision)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results = {"sets": [], "records": None}
    for step in [f"set:{n}:{e}" for n, e in SETS] + ["records"]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--games", str(args.games),
               "--sims", str(args.sims), "--precision", args.precision]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"step {step} ended with status {r.returncode}: nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            results["failed_step"] = dict(step=step, status=r.returncode)
            break
        res = json.loads(line[len("RESULT "):])
        print(step, json.dumps(res), flush=True)
        if step == "records":
            results["records"] = res
        else:
            results["sets"].append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 1 if "failed_step" in results else 0


if __name__ == "__main__":
    sys.exit(main())
