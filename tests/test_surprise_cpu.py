"""Policy surprise weighting without a GPU: the new symbols in header, bindings and library; oz_policy_surprises against the plain Python
restatement (tests/surprise_ref.py) within the rounding bound of its definition; oz_surprise_weights and oz_surprise_copies against it
bit for bit; preservation of the amount of data; unbiased copy counts; the argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surprise_ref as ref
from replay_ref import RECORD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_selfplay_set_record_surprise", "oz_selfplay_surprises", "oz_selfplay_surprises_device", "oz_policy_surprises",
               "oz_policy_surprises_f32", "oz_selfplay_surprise_weights", "oz_selfplay_weights", "oz_surprise_weights", "oz_surprise_copies",
               "oz_replay_append_selfplay_weighted"]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "---- policy surprise weighting" in header
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        common = f.read()
    for name in ("oz_surprise_term", "oz_surprise_sum", "oz_surprise_weight", "oz_surprise_copies"):
        assert re.search(r"\b%s\(" % name, common), name
    assert re.search(r"\bOZ_RNG_SURPRISE = 8\b", common)


# ------------------------------------------------------------------ surprise
def _rows(rng, count):
    """root rows as a search leaves them: a few legal squares with counts and priors that sum to 1, 0 elsewhere"""
    N, P = np.zeros((count, 64), np.int32), np.zeros((count, 64), np.float64)
    for i in range(count):
        k = int(rng.integers(1, 14))
        sq = rng.choice(64, size=k, replace=False)
        N[i, sq] = rng.integers(0, 60, size=k)
        if N[i].sum() == 0:
            N[i, sq[0]] = 5
        p = rng.dirichlet(np.full(k, 0.5)).astype(np.float32).astype(np.float64)
        P[i, sq] = p
    return N, P


def _check(got, rows, P):
    want, abs_sum = ref.surprises(rows, P)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.isfinite(got).all() and (got >= 0).all()
    err = np.abs(got - want)
    assert (err <= ref.bound(abs_sum)).all(), (err.max(), ref.bound(abs_sum).min())


def test_surprises_of_count_rows_within_the_bound():
    from othellozero_amd import agents
    N, P = _rows(np.random.default_rng(21), 300)
    got = agents.rules_policy_surprise(N, P)
    _check(got, N, P)
    assert np.count_nonzero(got > 0) > 250


def test_surprises_of_float32_rows_within_the_bound():
    from othellozero_amd import agents
    rng = np.random.default_rng(22)
    N, P = _rows(rng, 300)
    q = np.zeros((300, 64), np.float32)
    for i in range(300):
        sq = np.flatnonzero(P[i] > 0)
        q[i, sq] = rng.dirichlet(np.full(sq.size, 0.3)).astype(np.float32)
    got = agents.rules_policy_surprise(q, P)
    _check(got, q, P)
    assert np.count_nonzero(got > 0) > 250


def test_surprise_edge_rows():
    from othellozero_amd import _lib, agents
    N, P = np.zeros((6, 64), np.int32), np.zeros((6, 64), np.float64)
    N[0, 19] = 7; P[0, 19] = 1.0                               # one legal move: q == p == 1 -> exactly 0
    N[1, [3, 9, 40]] = [10, 20, 10]; P[1, [3, 9, 40]] = [0.25, 0.5, 0.25]      # q == p in dyadic numbers: exactly 0
    N[2, [3, 9, 40]] = [1, 1, 1]; P[2, [3, 9, 40]] = 1.0 / 3.0               # q == p: 0 or a non-negative value within the bound
    N[3, [5, 6]] = [30, 3]; P[3, [5, 6]] = [1e-300, 1.0]       # a tiny prior on the most visited move: large, finite
    N[4, [5, 6]] = [30, 3]; P[4, [5, 6]] = [0.0, 1.0]          # a zero prior on a visited move: log(DBL_MIN), finite
    N[5, [5, 6]] = [0, 12]; P[5, [5, 6]] = [0.9, 0.1]          # an unvisited move adds nothing: log(1 / 0.1)
    got = agents.rules_policy_surprise(N, P)
    _check(got, N, P)
    assert got[0] == 0.0 and got[1] == 0.0
    assert 0.0 <= got[2] <= ref.bound(np.log(3.0))
    assert 600 < got[3] < 700 and 600 < got[4] < 700 and got[4] > got[3]
    assert abs(got[5] - np.log(10.0)) < 1e-15 * 4
    q = np.zeros((2, 64), np.float32)
    q[0, [5, 6]] = [0.5, 0.5]                                  # q == p in float32 rows
    q[1, [5, 6]] = [1.0, 0.0]
    Pq = np.zeros((2, 64)); Pq[0, [5, 6]] = 0.5; Pq[1, [5, 6]] = [0.0, 1.0]
    gq = agents.rules_policy_surprise(q, Pq)
    _check(gq, q, Pq)
    assert gq[0] == 0.0 and np.isfinite(gq[1]) and gq[1] > 700
    assert agents.rules_policy_surprise(N[3], P[3]).shape == () and agents.rules_policy_surprise(N.reshape(2, 3, 64), P.reshape(2, 3, 64)).shape == (2, 3)
    assert agents.rules_policy_surprise(np.zeros((0, 64), np.int32), np.zeros((0, 64))).shape == (0,)
    with pytest.raises(ValueError):
        agents.rules_policy_surprise(N, P[:, :32])
    with pytest.raises(ValueError):
        agents.rules_policy_surprise(N.astype(np.float64), P)
    bad = N.copy()
    bad[2, 9] = -1
    with pytest.raises(_lib.OzError):
        agents.rules_policy_surprise(bad, P)


# ------------------------------------------------------------------ weights and copies
def synthetic_games(seed=3, games=9, shuffle=True):
    """records of made-up games of 5 .. 60 plies: about a quarter of the records fast-flagged (one game all fast but one record, one game
    with every surprise 0), random surprises elsewhere; in shuffled order"""
    rng = np.random.default_rng(seed)
    recs, sur = [], []
    for g in range(games):
        T = 60 if g == 0 else int(rng.integers(5, 40))
        r = np.zeros(T, RECORD_DTYPE)
        r["game_id"] = 1000 + 17 * g
        r["ply"] = np.arange(T)
        r["player"] = 1
        r["z"] = 1
        fast = rng.random(T) < 0.25
        if g == 1:
            fast[:] = True
            fast[2] = False
        if g == 2:
            fast[:] = False
        r["pad"][:, 0] = fast
        s = rng.gamma(0.3, 0.5, size=T)
        if g == 3:
            s[~fast] = 0.0                                     # S == 0: every fully searched record weighs 1
        recs.append(r)
        sur.append(s)
    rec, sur = np.concatenate(recs), np.concatenate(sur)
    if shuffle:
        order = rng.permutation(rec.size)
        rec, sur = rec[order], sur[order]
    return rec, sur


@pytest.mark.parametrize("frac", [0.5, 1.0, 0.3])
def test_weights_and_copies_equal_the_restatement(frac):
    from othellozero_amd import agents
    rec, sur = synthetic_games()
    w = agents.rules_surprise_weights(rec, sur, frac)
    assert _same_bits(w, ref.weights(rec, sur, frac))
    fast = rec["pad"][:, 0] != 0
    assert fast.any() and (w[fast] == 0).all() and (w[~fast] >= np.float32(1.0 - frac)).all()
    flat = rec["game_id"] == 1000 + 17 * 3
    assert (w[flat & ~fast] == 1.0).all()
    c, t0 = agents.rules_surprise_copies(rec, w, 99)
    rc, rt0 = ref.copies(rec, w, 99)
    assert _same_bits(c, rc) and _same_bits(t0, rt0)
    assert (c[fast] == 0).all() and (c > 8).any() and ((c < 8) & ~fast).any()
    # the order the records arrive in does not matter
    back = np.argsort(rec["game_id"].astype(np.int64) * 64 + rec["ply"], kind="stable")
    assert _same_bits(agents.rules_surprise_weights(rec[back], sur[back], frac), w[back])
    c2, t2 = agents.rules_surprise_copies(rec[back], w[back], 99)
    assert _same_bits(c2, c[back]) and _same_bits(t2, t0[back])


@pytest.mark.parametrize("frac", [0.5, 1.0])
def test_weights_preserve_the_amount_of_data(frac):
    from othellozero_amd import agents
    rec, sur = synthetic_games(seed=8, games=12)
    w = agents.rules_surprise_weights(rec, sur, frac)
    for gid in np.unique(rec["game_id"]):
        m = rec["game_id"] == gid
        K = int((rec["pad"][m, 0] == 0).sum())
        wg = w[m].astype(np.float64)
        assert abs(wg.sum() - K) <= K * 2.0 ** -23 * wg.max(), (gid, K, wg.sum())


def test_copies_are_unbiased_and_first_symmetries_cover_all():
    from othellozero_amd import agents
    R = 20000
    rec = np.zeros(R, RECORD_DTYPE)
    rec["game_id"] = np.arange(R) // 50 + 7
    rec["ply"] = np.arange(R) % 50
    for wv in (0.3, 1.0, 1.27, 0.06, 3.9):
        w = np.full(R, wv, np.float32)
        c, t0 = agents.rules_surprise_copies(rec, w, 4242)
        assert abs(c.mean() - 8.0 * float(np.float32(wv))) <= 0.018, (wv, c.mean())
        lo = int(np.floor(8.0 * float(np.float32(wv))))
        assert set(np.unique(c)) <= {lo, lo + 1}
        assert set(np.unique(t0)) == set(range(8))
    c1, _ = agents.rules_surprise_copies(rec, np.full(R, 0.3, np.float32), 4243)
    assert not np.array_equal(c, c1) and (c1 != agents.rules_surprise_copies(rec, np.full(R, 0.3, np.float32), 4242)[0]).any()


def test_argument_errors():
    from othellozero_amd import _lib, agents
    lib = _lib.load()
    rec, sur = synthetic_games(games=3)
    for frac in (0.0, -0.5, 1.0001, float("nan"), "0.5", True, None):
        with pytest.raises(ValueError):
            agents.rules_surprise_weights(rec, sur, frac)
    w = np.zeros(rec.size, np.float32)
    p = rec.ctypes.data_as(C.c_void_p)
    for frac in (0.0, 1.5, float("nan")):
        assert lib.oz_surprise_weights(p, _lib.p_f64(sur), rec.size, frac, _lib.p_f32(w)) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_weights(None, _lib.p_f64(sur), rec.size, 0.5, _lib.p_f32(w)) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_weights(p, None, rec.size, 0.5, _lib.p_f32(w)) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_weights(p, _lib.p_f64(sur), rec.size, 0.5, None) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_weights(p, _lib.p_f64(sur), -1, 0.5, _lib.p_f32(w)) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_weights(None, None, 0, 0.5, None) == _lib.OZ_OK
    c, t0 = np.zeros(rec.size, np.int32), np.zeros(rec.size, np.uint8)
    assert lib.oz_surprise_copies(None, _lib.p_f32(w), rec.size, 1, _lib.p_i32(c), _lib.p_u8(t0)) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_copies(p, None, rec.size, 1, _lib.p_i32(c), _lib.p_u8(t0)) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_copies(p, _lib.p_f32(w), rec.size, 1, None, _lib.p_u8(t0)) == _lib.OZ_ERR_ARG
    assert lib.oz_surprise_copies(p, _lib.p_f32(w), rec.size, 1, _lib.p_i32(c), None) == _lib.OZ_ERR_ARG
    w[1] = np.nan
    assert lib.oz_surprise_copies(p, _lib.p_f32(w), rec.size, 1, _lib.p_i32(c), _lib.p_u8(t0)) == _lib.OZ_ERR_ARG
    N, P, out = np.zeros((2, 64), np.int32), np.zeros((2, 64)), np.zeros(2)
    assert lib.oz_policy_surprises(None, _lib.p_f64(P), 2, _lib.p_f64(out)) == _lib.OZ_ERR_ARG
    assert lib.oz_policy_surprises(_lib.p_i32(N), None, 2, _lib.p_f64(out)) == _lib.OZ_ERR_ARG
    assert lib.oz_policy_surprises(_lib.p_i32(N), _lib.p_f64(P), 2, None) == _lib.OZ_ERR_ARG
    assert lib.oz_policy_surprises_f32(None, _lib.p_f64(P), 2, _lib.p_f64(out)) == _lib.OZ_ERR_ARG
    assert lib.oz_policy_surprises(_lib.p_i32(N), _lib.p_f64(P), -1, _lib.p_f64(out)) == _lib.OZ_ERR_ARG
    bad = rec.copy()
    bad["ply"][0] = 64
    with pytest.raises(_lib.OzError):
        agents.rules_surprise_weights(bad, sur, 0.5)
    with pytest.raises(ValueError):
        agents.rules_surprise_weights(rec, sur[:-1], 0.5)
    with pytest.raises(ValueError):
        agents.rules_surprise_copies(rec, w[:-1], 1)


def test_engine_and_loop_refusals_need_no_gpu():
    from othellozero_amd import _lib
    assert _lib.check_surprise_frac(0.5) == 0.5 and _lib.check_surprise_frac(1) == 1.0
    for frac in (0, 1.5, float("nan"), "x", None, False):
        with pytest.raises(ValueError):
            _lib.check_surprise_frac(frac)
