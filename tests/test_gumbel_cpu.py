"""The Gumbel search without a GPU: the host-only twins (oz_gumbel_considered_visits, oz_gumbel_draws, oz_gumbel_root,
oz_examples_expand_policy) against the restatement in tests/gumbel_ref.py, the restatement's own properties, and the argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import gumbel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_mcts_set_gumbel", "oz_mcts_sample_gumbel", "oz_mcts_get_gumbel", "oz_mcts_gumbel_policy", "oz_mcts_gumbel_scores",
               "oz_mcts_node_value", "oz_gumbel_considered_visits", "oz_gumbel_draws", "oz_gumbel_from_units", "oz_gumbel_root",
               "oz_examples_expand_policy"]
ROOT_SEED, ROOT_ROWS = 20240, 2000
NEAR_TIE = 1e-9


@pytest.fixture(scope="module")
def oz():
    from othellozero_amd import _lib
    _lib.load()
    return _lib


def ulps(a, b):
    """distance of two finite float64 in units in the last place"""
    ia, ib = (np.asarray(x, np.float64).view(np.int64).astype(object) for x in (a, b))
    f = np.vectorize(lambda v: v if v >= 0 else -(v & 0x7FFFFFFFFFFFFFFF), otypes=[object])
    return np.abs(f(ia) - f(ib)).astype(np.float64)


# ------------------------------------------------------------------ the schedule
def test_schedule_hand_example():
    assert R.considered_visits(4, 16) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert R.considered_visits(1, 5) == [0, 1, 2, 3, 4]


def test_schedule_vs_restatement():
    from othellozero_amd import agents
    for m in range(1, 34):
        for n in (1, 2, 7, 16, 25, 100):
            got, want = agents.rules_gumbel_considered_visits(m, n), R.considered_visits(m, n)
            assert len(want) == n and got.shape == (n,)
            assert list(got) == want, (m, n)
    assert list(agents.rules_gumbel_considered_visits(4, 16)) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


# ------------------------------------------------------------------ the draws
def test_draws_vs_restatement():
    from othellozero_amd import agents
    rng = np.random.default_rng(3)
    legal = [int(x) for x in rng.integers(0, 2 ** 63, 40, dtype=np.uint64)] + [1, 1 << 63, 0, 2 ** 64 - 1]
    ids = [int(x) for x in rng.integers(0, 2 ** 40, len(legal))]
    plies = [int(x) for x in rng.integers(0, 60, len(legal))]
    for seed in (0, 77):
        g = agents.rules_gumbel_draws(seed, ids, plies, legal)
        for i, lg in enumerate(legal):
            want = R.gumbel_row(lg, seed, ids[i], plies[i])
            assert np.isfinite(g[i]).all()
            assert all(g[i][sq] == 0.0 for sq in range(64) if not (lg >> sq) & 1)
            assert ulps(g[i], want).max() <= 4, (seed, i)
    # rows differ across game id, ply and square
    full = 2 ** 64 - 1
    a = agents.rules_gumbel_draws(9, [4, 5, 4], [11, 11, 12], [full] * 3)
    assert len(set(a.ravel().tolist())) == 3 * 64


def test_endpoint_draws_are_finite(oz):
    u = np.array([0.0, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53], np.float64)
    g = np.zeros(4)
    oz.check(oz.load().oz_gumbel_from_units(oz.p_f64(u), 4, oz.p_f64(g)))
    assert np.isfinite(g).all() and g[0] < g[1] < g[2] < g[3]
    for i in range(4):
        assert ulps(g[i], R.gumbel_from_unit(float(u[i]))).max() <= 4
        assert math.isfinite(R.gumbel_from_unit(float(u[i])))
    assert g[0] == pytest.approx(-math.log(54 * math.log(2.0))) and g[3] == pytest.approx(53 * math.log(2.0), rel=1e-9)
    bad = np.array([1.0], np.float64)
    assert oz.load().oz_gumbel_from_units(oz.p_f64(bad), 1, oz.p_f64(g)) == oz.OZ_ERR_ARG


# ------------------------------------------------------------------ the root function
def _random_rows(count, seed):
    """root rows by square: mixed visited / unvisited squares, sumN == 0, one legal move, a legal square with P == 0, fresh and reused roots"""
    rng = np.random.default_rng(seed)
    N, N0 = np.zeros((count, 64), np.int32), np.zeros((count, 64), np.int32)
    Q, P, g = np.zeros((count, 64)), np.zeros((count, 64)), np.zeros((count, 64))
    legal, vhat = np.zeros(count, np.uint64), np.zeros(count)
    kinds = []
    for i in range(count):
        kind = ("mixed", "fresh", "zero", "single", "pzero", "reuse", "over")[i % 7]
        kinds.append(kind)
        cnt = 1 if kind == "single" else int(rng.integers(2, 34))
        sqs = sorted(rng.choice(64, cnt, replace=False).tolist())
        legal[i] = np.uint64(sum(1 << s for s in sqs))
        p = rng.dirichlet(np.full(cnt, 0.5))
        if kind == "pzero" and cnt > 1:
            p[int(rng.integers(cnt))] = 0.0
            p = p / p.sum()
        vhat[i] = float(np.float32(rng.uniform(-1, 1)))
        for j, s in enumerate(sqs):
            P[i, s] = p[j]
            g[i, s] = R.gumbel_from_unit(float(rng.integers(0, 2 ** 53)) * R.UNIT)
            if kind == "zero":
                continue
            visited = rng.random() < 0.6
            if visited:
                if kind == "fresh":
                    N[i, s] = int(rng.integers(1, 7))
                elif kind == "over":
                    N[i, s] = int(rng.integers(8, 40))            # more visits than the budget: the max-n rule
                else:
                    N0[i, s] = int(rng.integers(0, 20))
                    N[i, s] = N0[i, s] + int(rng.integers(0, 5)) + (1 if N0[i, s] == 0 else 0)
                Q[i, s] = rng.uniform(-1, 1)
    return N, N0, Q, P, g, legal, vhat, kinds


@pytest.mark.parametrize("params", [(4, 50.0, 1.0, 16), (16, 50.0, 1.0, 100), (1, 0.0, 0.1, 25), (33, 50.0, 1.0, 7)])
def test_root_function_vs_restatement(params):
    from othellozero_amd import agents
    m, c_visit, c_scale, budget = params
    N, N0, Q, P, g, legal, vhat, kinds = _random_rows(ROOT_ROWS, ROOT_SEED + m)
    assert set(kinds) == {"mixed", "fresh", "zero", "single", "pzero", "reuse", "over"}
    pick, move, pi, score, gaps = agents.rules_gumbel_root(N, N0, Q, P, g, legal, vhat, (m, c_visit, c_scale), budget, with_scores=True)
    near, worst_pi = 0, 0.0
    for i in range(ROOT_ROWS):
        lg = int(legal[i])
        r = R.root(N[i], N0[i], Q[i], P[i], g[i], lg, vhat[i], m, c_visit, c_scale, budget)
        # the seeds are chosen so that the restatement alone meets no near-tie
        assert r["gap_pick"] >= NEAR_TIE and r["gap_move"] >= NEAR_TIE, (i, r["gap_pick"], r["gap_move"])
        assert (int(pick[i]), int(move[i])) == (r["pick"], r["move"]), (i, kinds[i])
        assert (lg >> int(pick[i])) & 1 and (lg >> int(move[i])) & 1
        d = float(np.abs(pi[i].astype(np.float64) - r["pi"].astype(np.float64)).max())
        worst_pi = max(worst_pi, d)
        assert d <= 2e-7, (i, d)
        assert abs(float(pi[i].astype(np.float64).sum()) - 1.0) <= 1e-6
        assert all(pi[i][s] == 0.0 for s in range(64) if not (lg >> s) & 1)
        for s in range(64):
            if (lg >> s) & 1 and math.isfinite(r["score"][s]):
                assert abs(score[i][s] - r["score"][s]) <= 1e-12 * max(1.0, abs(r["score"][s]))
        assert gaps[i][0] == pytest.approx(r["gap_pick"], abs=1e-12) and gaps[i][1] == pytest.approx(r["gap_move"], abs=1e-12)
        if kinds[i] == "zero":                             # nothing visited: sigma is the same for every move and pi' is the prior
            assert np.abs(pi[i].astype(np.float64) - P[i].astype(np.float32).astype(np.float64)).max() <= 2e-7
        if kinds[i] == "single":
            assert pi[i].max() == 1.0 and int(pick[i]) == int(move[i]) == int(math.log2(lg))
    print(f"params {params}: worst |pi - restatement| {worst_pi:.3e}, near-ties left out {near}")
    assert near <= ROOT_ROWS // 1000


def test_root_pick_follows_the_schedule():
    """a fresh root driven by the restatement alone: m = 4 over 16 simulations gives 6, 6, 2, 2; m = 1 puts every visit on one move; beyond
    the budget the pick follows max n"""
    rng = np.random.default_rng(5)
    sqs = [3, 9, 17, 20, 33, 41, 50]
    legal = sum(1 << s for s in sqs)
    P, g = np.zeros(64), np.zeros(64)
    P[sqs] = rng.dirichlet(np.ones(len(sqs)))
    g[sqs] = [R.gumbel_from_unit(float(u)) for u in rng.uniform(0.01, 0.99, len(sqs))]
    for m, want in ((4, [2, 2, 6, 6]), (1, [16]), (2, [8, 8])):
        N, Q = np.zeros(64, np.int32), np.zeros(64)
        for t in range(16):
            r = R.root(N, np.zeros(64, np.int32), Q, P, g, legal, 0.1, m, 50.0, 1.0, 16)
            assert r["t"] == t and r["cv"] == R.considered_visits(min(m, len(sqs)), 16)[t]
            a = r["pick"]
            q = rng.uniform(-1, 1)
            Q[a] = (N[a] * Q[a] + q) / (N[a] + 1)
            N[a] += 1
        assert sorted(int(x) for x in N if x) == want, (m, N[sqs])
        top = int(np.argmax(N))
        for t in range(3):                                 # beyond the budget
            r = R.root(N, np.zeros(64, np.int32), Q, P, g, legal, 0.1, m, 50.0, 1.0, 16)
            assert r["cv"] == N.max() and N[r["pick"]] == N.max()
            N[r["pick"]] += 1
        assert N.max() == want[-1] + 3 and (m != 1 or int(np.argmax(N)) == top)


# ------------------------------------------------------------------ examples
@pytest.mark.parametrize("n", [4, 6, 8])
@pytest.mark.parametrize("alias_final", [0, 1])
def test_expand_policy_is_bit_exact_against_the_symmetries(oz, n, alias_final):
    from othellozero_amd.training import training_example_symmetries
    rng = np.random.default_rng(n)
    R_ = 5
    rec = np.zeros(R_, oz.RECORD_DTYPE)
    valid = sum(1 << (r * 8 + c) for r in range(n) for c in range(n))
    for f in ("black", "white", "final_black", "final_white"):
        rec[f] = rng.integers(0, 2 ** 63, R_, dtype=np.uint64) & np.uint64(valid)
    rec["z"] = rng.choice([-1, 1], R_)
    rows = np.zeros((R_, 64), np.float32)
    for r in range(n):
        for c in range(n):
            rows[:, r * 8 + c] = rng.random(R_).astype(np.float32)
    boards, pi, z = np.zeros((R_ * 8, n, n, 2), np.uint8), np.zeros((R_ * 8, n, n), np.float32), np.zeros(R_ * 8, np.int8)
    oz.check(oz.load().oz_examples_expand_policy(rec.ctypes.data_as(C.c_void_p), oz.p_f32(rows), R_, n, alias_final, oz.p_u8(boards), oz.p_f32(pi),
                                                 oz.p_i8(z)))
    for i in range(R_):
        b, w = (int(rec[i]["final_black" if alias_final else "black"]), int(rec[i]["final_white" if alias_final else "white"]))
        board = np.array([[[(b >> (r * 8 + c)) & 1, (w >> (r * 8 + c)) & 1] for c in range(n)] for r in range(n)], np.uint8)
        policy = np.array([[rows[i, r * 8 + c] for c in range(n)] for r in range(n)], np.float32)
        for t, (sb, sp) in enumerate(training_example_symmetries(board, policy)):
            assert np.array_equal(boards[i * 8 + t], sb) and z[i * 8 + t] == rec[i]["z"]
            assert np.array_equal(pi[i * 8 + t].view(np.uint32), np.ascontiguousarray(sp).view(np.uint32)), (i, t)


# ------------------------------------------------------------------ arguments and symbols
@pytest.mark.parametrize("bad", [(0, 50.0, 1.0, 16), (65, 50.0, 1.0, 16), (4, -1.0, 1.0, 16), (4, 50.0, 0.0, 16), (4, 50.0, -1.0, 16),
                                 (4, float("nan"), 1.0, 16), (4, 50.0, float("nan"), 16), (4, 50.0, 1.0, 0), (4, 50.0, 1.0, -3)])
def test_argument_errors(oz, bad):
    m, c_visit, c_scale, budget = bad
    z32, z64, lg = np.zeros(64, np.int32), np.zeros(64), np.array([1], np.uint64)
    pick, move, pi = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(64, np.float32)
    rc = oz.load().oz_gumbel_root(oz.p_i32(z32), oz.p_i32(z32), oz.p_f64(z64), oz.p_f64(z64), oz.p_f64(z64), oz.p_u64(lg), oz.p_f64(np.zeros(1)),
                                  1, m, c_visit, c_scale, budget, oz.p_i32(pick), oz.p_i32(move), oz.p_f32(pi), None, None)
    assert rc == oz.OZ_ERR_ARG
    if budget >= 1:
        with pytest.raises(ValueError):
            oz.check_gumbel((m, c_visit, c_scale))


def test_schedule_argument_errors(oz):
    out = np.zeros(4, np.int32)
    for m, n in ((0, 4), (65, 4), (4, 0)):
        assert oz.load().oz_gumbel_considered_visits(m, n, oz.p_i32(out)) == oz.OZ_ERR_ARG
    assert oz.check_gumbel(None) is None and oz.check_gumbel(True) == (16, 50.0, 1.0) and oz.check_gumbel([4, 50, 1]) == (4, 50.0, 1.0)
    for bad in ("ab", (4, 50.0), (4.5, 50.0, 1.0), 3):
        with pytest.raises(ValueError):
            oz.check_gumbel(bad)


def test_new_symbols_in_header_and_bindings(oz):
    lib = oz.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in oz.SIGNATURES and hasattr(lib, name), name
    assert lib.oz_version() == 230
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        common = f.read()
    assert re.search(r"OZ_RNG_GUMBEL\s*=\s*7\b", common)
    # stream 7 + 256 sq collides with none of 0 .. 6 and none of 3 + 256 sq' + 65536 i
    gumbel = {7 + 256 * sq for sq in range(64)}
    noise = {3 + 256 * sq + 65536 * i for sq in range(64) for i in range(49)}
    assert not gumbel & noise and not gumbel & set(range(7))
