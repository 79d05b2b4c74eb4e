"""Resignation without a GPU: the new symbols in header, bindings and library; oz_resign_scan / oz_resign_exempt (the functions the move
kernels evaluate, run on the host) against the restatement bit for bit; the validators; the restatement's own games at the settings of the GPU
test against the figures they were checked with."""
import math
import os
import re

import numpy as np
import pytest

import resign_ref as ref
from replay_ref import RECORD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_selfplay_set_resign", "oz_selfplay_get_resign", "oz_resign_scan", "oz_resign_exempt"]
# the settings of tests/test_gpu_resign.py
N, SIMS, EG, SEED, FIRST, G, SALT, RESIGN = 6, 12, 0.8, 41, 200, 16, 21, (0.3, 2, 8, 0.25)


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "OZ_RNG_RESIGN = 9" in header and "} oz_resign_stats;" in header
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        assert re.search(r"\bOZ_RNG_RESIGN = 9\b", f.read())
    # 9 is none of the streams 0 .. 8, none of 3 + 256 sq + 65536 i and none of 7 + 256 sq
    assert _lib.RNG_RESIGN == ref.RNG_RESIGN == 9 and (9 - 3) % 256 != 0 and (9 - 7) % 256 != 0
    assert [k for k, _ in _lib.ResignStats._fields_] == list(ref.STAT_KEYS)
    assert _lib.RECORD_DTYPE == RECORD_DTYPE                                             # the layout and the field names stay
    rec = np.zeros(3, _lib.RECORD_DTYPE)
    rec["pad"][1] = (0, 1, 0)
    assert _lib.record_adjudicated(rec).tolist() == [0, 1, 0] and _lib.record_fast(rec).tolist() == [0, 0, 0]
    assert rec.tobytes()[48 + 46] == 1                                                   # byte 46 of the 48: the second spare one


# ------------------------------------------------------------------ the rule: the library's host entries against the restatement
def _sequences(rng, v):
    """random games whose b = p q is often exactly +-v, sometimes NaN, with sign flips in the middle of a streak and long runs"""
    pool = np.array([v, -v, np.nextafter(v, 0.0), np.nextafter(-v, 0.0), np.nextafter(v, 2.0), np.nextafter(-v, -2.0), 1.0, -1.0, 0.0, -0.0,
                     math.nan, 0.5 * v, -0.5 * v])
    lengths = [0, 1, 2, 7, 8, 9, 32, 60, 64, 300] + [int(x) for x in rng.integers(1, 61, 40)]
    players, values = [], []
    for k, length in enumerate(lengths):
        p = rng.choice(np.array([1, -1], np.int8), length)
        if k % 3 == 0:                                     # one side keeps winning: long streaks, broken by a flip or a NaN now and then
            b = np.where(rng.random(length) < 0.9, pool[k % 2], rng.choice(pool, length))
        else:
            b = np.where(rng.random(length) < 0.5, rng.choice(pool, length), rng.uniform(-1.0, 1.0, length))
        players.append(p)
        values.append(p * b)                               # p * (p b) == b exactly for p = +-1
    return np.concatenate(players).astype(np.int8), np.concatenate(values), np.array(lengths, np.int32)


@pytest.mark.parametrize("v", [0.3, 1.0, 0.9501])
def test_scan_equals_the_restatement(v):
    from othellozero_amd import agents
    players, values, lengths = _sequences(np.random.default_rng(5), v)
    assert np.isnan(values).any() and (players * values == v).any() and (players * values == -v).any() and lengths.max() > 255
    seen = set()
    for r in (1, 2, 5, 8):
        for min_ply in (0, 3, 8, 61, 64):                  # 61, 64: beyond the length of most (all but the 300-ply) sequences
            got = agents.rules_resign_scan(players, values, lengths, v, r, min_ply)
            want = ref.scan(players, values, lengths, v, r, min_ply)
            assert got[0].dtype == np.int32 and got[1].dtype == np.int8
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (v, r, min_ply)
            assert ((got[0] < 0) == (got[1] == 0)).all() and (got[0][got[0] >= 0] >= min_ply).all()
            seen.update(got[1].tolist())
            if min_ply == 64:
                assert (got[0][lengths <= 64] == -1).all()
    assert seen == {-1, 0, 1}
    # the 300-ply run of one sign saturates its streak at 255 and still triggers, at min_ply
    one = agents.rules_resign_scan(np.ones(300, np.int8), np.full(300, v), [300], v, 8, 64)
    assert (int(one[0][0]), int(one[1][0])) == (64, 1) and ref.step(1, 255, 1, v, v, 8, 64, 299) == (1, 255, True)


def test_scan_by_hand():
    from othellozero_amd import agents
    scan = lambda b, r, m=0: tuple(int(x[0]) for x in agents.rules_resign_scan(np.ones(len(b), np.int8), b, [len(b)], 0.5, r, m))      # noqa: E731
    assert scan([0.5, 0.5], 2) == (1, 1)                   # b == v counts
    assert scan([-0.5, -0.5], 2) == (1, -1)                # b == -v counts
    assert scan([0.5, 0.4999, 0.5, 0.5], 2) == (3, 1)      # a value inside (-v, v) resets
    assert scan([0.9, -0.9, -0.9], 2) == (2, -1)           # a flip starts the other side's streak at 1
    assert scan([0.9, math.nan, 0.9], 2) == (-1, 0)        # NaN resets
    assert scan([0.9, 0.9, 0.9, 0.9], 2, 3) == (3, 1)      # min_ply delays the trigger, the streak goes on
    assert scan([0.9], 1) == (0, 1) and scan([], 1) == (-1, 0)
    # the mover's sign: a WHITE mover who sees -0.9 is BLACK at +0.9
    got = agents.rules_resign_scan(np.array([1, -1], np.int8), [0.9, -0.9], [2], 0.5, 2, 0)
    assert (int(got[0][0]), int(got[1][0])) == (1, 1)


def test_exempt_equals_the_restatement():
    """4 000 game ids at keep_prob 0.25: within 5 binomial standard deviations of 1 000 (sigma = sqrt(4000 * 0.25 * 0.75) = 27.4)"""
    from othellozero_amd import agents
    ids = np.arange(150, 4150, dtype=np.uint64)
    got = agents.rules_resign_exempt(SEED, ids, 0.25)
    want = np.array([ref.exempt(SEED, int(g), 0.25) for g in ids])
    assert got.dtype == bool and np.array_equal(got, want) and abs(int(got.sum()) - 1000) <= 137
    assert not agents.rules_resign_exempt(SEED, ids, 0.0).any() and agents.rules_resign_exempt(SEED, ids, 1.0).all()
    assert not np.array_equal(agents.rules_resign_exempt(SEED + 1, ids, 0.25), got)
    assert agents.rules_resign_exempt(SEED, [], 0.5).size == 0


# ------------------------------------------------------------------ the validators
def test_library_refusals():
    from othellozero_amd import _lib
    lib = _lib.load()
    p, q, n = np.ones(4, np.int8), np.zeros(4), np.array([4], np.int32)
    ply, side = np.full(1, -7, np.int32), np.full(1, -7, np.int8)
    call = lambda v, r, m, pl=p, nn=n: lib.oz_resign_scan(_lib.p_i8(pl), _lib.p_f64(q), _lib.p_i32(nn), 1, v, r, m, _lib.p_i32(ply), _lib.p_i8(side))      # noqa: E731
    for v, r, m in ((0.0, 2, 8), (-0.3, 2, 8), (1.5, 2, 8), (math.nan, 2, 8), (0.3, 0, 8), (0.3, 9, 8), (0.3, -1, 8), (0.3, 2, -1), (0.3, 2, 65)):
        assert call(v, r, m) == _lib.OZ_ERR_ARG and lib.oz_last_error() and ply[0] == -7 and side[0] == -7, (v, r, m)
    assert call(0.3, 2, 8, np.array([1, 0, 1, 1], np.int8)) == _lib.OZ_ERR_ARG
    assert call(0.3, 2, 8, p, np.array([-1], np.int32)) == _lib.OZ_ERR_ARG
    assert call(1.0, 8, 64) == 0 and (int(ply[0]), int(side[0])) == (-1, 0)
    assert lib.oz_resign_scan(None, None, None, 0, 0.3, 2, 8, None, None) == 0
    out = np.full(2, 9, np.uint8)
    ids = np.arange(2, dtype=np.uint64)
    for kp in (-0.1, 1.1, math.nan):
        assert lib.oz_resign_exempt(1, _lib.p_u64(ids), 2, kp, _lib.p_u8(out)) == _lib.OZ_ERR_ARG and (out == 9).all()
    assert lib.oz_resign_exempt(1, None, 0, 0.5, None) == 0


GOOD = [((0.3, 2, 8, 0.25), (0.3, 2, 8, 0.25)), ([1, 8, 64, 1], (1.0, 8, 64, 1.0)), ((np.float32(0.5), np.int32(1), 0, 0), (0.5, 1, 0, 0.0)),
        ((1e-9, 3.0, 10.0, 0.5), (1e-9, 3, 10, 0.5))]
BAD = [(0.0, 2, 8, 0.25), (-0.3, 2, 8, 0.25), (1.01, 2, 8, 0.25), (math.nan, 2, 8, 0.25), (0.3, 0, 8, 0.25), (0.3, 9, 8, 0.25), (0.3, 2.5, 8, 0.25),
       (0.3, 2, -1, 0.25), (0.3, 2, 65, 0.25), (0.3, 2, 8.5, 0.25), (0.3, 2, 8, -0.01), (0.3, 2, 8, 1.01), (0.3, 2, 8, math.nan), (0.3, 2, 8),
       (0.3, 2, 8, 0.25, 1), 0.3, "resign", (True, 2, 8, 0.25), (0.3, True, 8, 0.25), ("0.3", 2, 8, 0.25), (0.3, 2, 8, None), (0.3, math.nan, 8, 0.25),
       {"v": 0.3}]


def test_check_resign_accepts_and_refuses():
    from othellozero_amd import _lib
    assert _lib.check_resign(None) is None
    for given, want in GOOD:
        got = _lib.check_resign(given)
        assert got == want and [type(x) for x in got] == [float, int, int, float], given
    with pytest.raises(ValueError, match="gumbel"):
        _lib.check_resign(RESIGN, gumbel=(16, 50.0, 1.0))
    with pytest.raises(ValueError, match="lock-step"):
        _lib.check_resign(RESIGN, free_running=True)


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_bad_resign_options_are_a_value_error_before_any_library_call(bad):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, loop, training
    with pytest.raises(ValueError):
        _lib.check_resign(bad)
    with pytest.raises(ValueError):
        training.SelfPlayEngine(object(), 6, 4, 12, resign=bad)
    with pytest.raises(ValueError):
        training.selfplay_batch(object(), 6, 4, 12, resign=bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, 12, 1.0, 1, object(), 0.9, 1, 1, None, True, 1, 2, 1, "unused", 100, resign=bad)


def test_resign_and_gumbel_are_refused_together_before_any_library_call():
    from othellozero_amd import loop, training
    with pytest.raises(ValueError, match="gumbel"):
        training.SelfPlayEngine(object(), 6, 4, 12, resign=RESIGN, gumbel=True)
    with pytest.raises(ValueError, match="gumbel"):
        training.selfplay_batch(object(), 6, 4, 12, resign=RESIGN, gumbel=True)
    with pytest.raises(ValueError, match="gumbel"):
        loop.training(6, 1, 2, 12, 1.0, 1, object(), 0.9, 1, 1, None, True, 1, 2, 1, "unused", 100, resign=RESIGN, gumbel=True)


# ------------------------------------------------------------------ the restatement itself
def test_restatement_gives_the_figures_it_was_checked_with():
    """6x6, 16 games, ids 200 .. 215, seed 41, 12 simulations, e_greedy 0.8, stub salt 21, resign (0.3, 2, 8, .).  Every natural game has 32
    plies.  Ignoring exemption the rule triggers before the last ply in 15 games (never at the last ply only), never in 1 (id 208), calls the
    natural loser in 9 of the 15 and cuts 27 plies.  keep_prob 0.25 exempts ids 200, 202, 206, 210, 215: 10 adjudicated games of 300 plies,
    5 exempt games that all triggered (plies 148 in sum), 2 of them wrongly."""
    ids = range(FIRST, FIRST + G)
    plain = ref.episodes(N, SIMS, None, EG, SEED, ids, SALT)
    audit = ref.episodes(N, SIMS, RESIGN[:3] + (1.0,), EG, SEED, ids, SALT)
    assert plain[0].tobytes() == audit[0].tobytes() and np.array_equal(plain[1], audit[1]) and plain[2].tobytes() == audit[2].tobytes()
    assert all(int((plain[0]["game_id"] == g).sum()) == 32 for g in ids) and not plain[0]["pad"].any()
    assert audit[3] == dict(games_adjudicated=0, adjudicated_plies_sum=0, games_exempt=16, exempt_triggered=15, exempt_wrong=9,
                            exempt_trigger_ply_sum=438)
    trig = {g: i["trigger_ply"] for g, i in audit[4].items()}
    assert [g for g, t in trig.items() if t < 0] == [208] and max(trig.values()) == 30 and sum(31 - t for t in trig.values() if t >= 0) == 27
    # the scan over the recorded values finds the same first triggers
    p, s = ref.scan(plain[0]["player"], plain[2], [32] * G, *RESIGN[:3])
    assert p.tolist() == [trig[g] for g in ids] and s.tolist() == [audit[4][g]["trigger_side"] for g in ids]

    rec, rows, vals, stats, infos = ref.episodes(N, SIMS, RESIGN, EG, SEED, ids, SALT)
    assert stats == dict(games_adjudicated=10, adjudicated_plies_sum=300, games_exempt=5, exempt_triggered=5, exempt_wrong=2,
                         exempt_trigger_ply_sum=148)
    assert sorted(g for g, i in infos.items() if i["exempt"]) == [200, 202, 206, 210, 215]
    assert (rec.size, int(rec["pad"][:, 1].sum()), int((rec["z"] == 1).sum())) == (492, 300, 252) and not rec["pad"][:, [0, 2]].any()
    assert rows.shape == (492, 64) and vals.shape == (492,) and np.abs(vals).max() <= 1.0
    # the minima the GPU test relies on
    right = stats["exempt_triggered"] - stats["exempt_wrong"]
    none = [g for g, i in infos.items() if i["trigger_ply"] < 0]
    assert stats["games_adjudicated"] >= 3 and stats["exempt_triggered"] >= 2 and stats["exempt_wrong"] >= 1 and right >= 1 and len(none) >= 1
    for g in ids:
        mine, theirs = rec[rec["game_id"] == g], plain[0][plain[0]["game_id"] == g]
        info = infos[g]
        k = mine.size
        # a stopped game is the natural game up to the stop: boards, moves, movers and coins; z and the final board are those of the stop
        for f in ("black", "white", "ply", "action", "player", "greedy"):
            assert np.array_equal(mine[f], theirs[f][:k]), (g, f)
        assert vals[rec["game_id"] == g].tobytes() == plain[2][plain[0]["game_id"] == g][:k].tobytes()
        if info["adjudicated"]:
            assert k == info["trigger_ply"] + 1 < 32 and (mine["pad"][:, 1] == 1).all() and not info["exempt"]
            assert (mine["z"] == np.where(mine["player"] == info["trigger_side"], 1, -1)).all()
            assert (int(mine["final_black"][0]), int(mine["final_white"][0])) == (int(theirs["black"][k]), int(theirs["white"][k]))
        else:
            assert mine.tobytes() == theirs.tobytes() and (info["exempt"] or info["trigger_ply"] < 0)
