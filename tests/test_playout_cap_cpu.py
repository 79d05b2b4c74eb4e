"""The playout cap without a GPU: the new symbols in header, bindings and library; oz_playout_budgets (the function the kernels evaluate, run on
the host) against the restatement's draw; the two Python record filters on synthetic records; check_playout_cap; the restatement itself against
the figures it was checked with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import playout_cap_ref as ref
from replay_ref import RECORD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_selfplay_set_playout_cap", "oz_selfplay_get_playout_cap", "oz_playout_budgets"]


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "OZ_RNG_PLAYOUT = 6" in header
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        assert re.search(r"\bOZ_RNG_PLAYOUT = 6\b", f.read())
    assert _lib.RNG_PLAYOUT == ref.RNG_PLAYOUT == 6 and (6 - 3) % 256 != 0               # 6 is none of 0 .. 5 and not 3 + 256 sq + 65536 i
    assert _lib.RECORD_DTYPE == RECORD_DTYPE                                             # the layout and the field names stay
    rec = np.zeros(3, _lib.RECORD_DTYPE)
    rec["pad"][1] = (1, 0, 0)
    assert _lib.record_fast(rec).tolist() == [0, 1, 0] and rec.tobytes()[48 + 45] == 1  # byte 45 of the 48: the first spare one


# ------------------------------------------------------------------ the budget: the library's host entry against the restatement
def test_budgets_equal_the_restatements_draw():
    """100 000 (game, ply) pairs: seed 7, ids 0 .. 1999, plies 0 .. 49, p = 0.25.  The number of full draws of a fair stream lies within 5
    binomial standard deviations of 25 000 (sigma = sqrt(100000 * 0.25 * 0.75) = 136.9: +- 685); the restatement gives 25 010."""
    from othellozero_amd import _lib
    seed, sims, cap = 7, 100, (20, 0.25)
    ids, plies = np.repeat(np.arange(2000, dtype=np.uint64), 50), np.tile(np.arange(50, dtype=np.int32), 2000)
    got = _lib.playout_budgets(seed, ids, plies, sims, cap)
    want = np.array([ref.budget(seed, int(g), int(p), sims, cap)[0] for g, p in zip(ids, plies)], np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    full = int((got == sims).sum())
    print(f"full draws: {full} of {got.size}")
    assert full + int((got == cap[0]).sum()) == got.size and abs(full - 25000) <= 685 and full == 25010
    # off, and full_prob 1: every move is full; another seed: other draws
    assert (_lib.playout_budgets(seed, ids[:500], plies[:500], sims, None) == sims).all()
    assert (_lib.playout_budgets(seed, ids[:500], plies[:500], sims, (20, 1.0)) == sims).all()
    assert not np.array_equal(_lib.playout_budgets(seed + 1, ids, plies, sims, cap), got)


def test_budgets_refusals():
    from othellozero_amd import _lib
    lib = _lib.load()
    ids, plies, out = np.arange(4, dtype=np.uint64), np.zeros(4, np.int32), np.full(4, -7, np.int32)
    call = lambda sims, fs, p, pl=plies: lib.oz_playout_budgets(7, _lib.p_u64(ids), _lib.p_i32(pl), 4, sims, fs, p, _lib.p_i32(out))      # noqa: E731
    for sims, fs, p in ((12, 1, 0.25), (12, 13, 0.25), (12, -4, 0.25), (12, 4, 0.0), (12, 4, 1.5), (12, 4, -0.1), (12, 4, float("nan")), (1, 0, 0.5)):
        assert call(sims, fs, p) == _lib.OZ_ERR_ARG and lib.oz_last_error() and (out == -7).all(), (sims, fs, p)
    assert call(12, 4, 0.25, np.array([0, -1, 0, 0], np.int32)) == _lib.OZ_ERR_ARG
    assert call(12, 12, 1.0) == 0 and (out == 12).all()
    assert call(12, 0, 7.0) == 0 and (out == 12).all()                                   # off: full_prob is not looked at
    assert lib.oz_playout_budgets(7, None, None, 0, 12, 4, 0.25, None) == 0


# ------------------------------------------------------------------ the two Python filters
def _synthetic(flags):
    rec = np.zeros(len(flags), RECORD_DTYPE)
    rec["game_id"] = 900 + np.arange(len(flags)) // 4
    rec["ply"] = np.arange(len(flags)) % 4
    rec["black"], rec["white"] = 1 + np.arange(len(flags)), 1 << 40
    rec["action"] = 8 + np.arange(len(flags)) % 5
    rec["player"], rec["z"], rec["greedy"] = 1, -1, 1
    rec["pad"][:, 0] = flags
    visits = (np.arange(len(flags) * 64, dtype=np.int32).reshape(-1, 64) * 3 + 1)
    return rec, visits


class _FakeLib:
    """stands where the GPU library would: keeps what expand_examples hands to the device"""

    def __init__(self):
        self.records, self.counts = None, None

    def oz_examples_expand(self, ptr, R, n, alias, boards, pol, z):
        self.records = np.frombuffer(C.string_at(ptr, R * 48), RECORD_DTYPE).copy()
        return 0

    def oz_examples_expand_visits(self, ptr, counts, R, n, alias, T, boards, pi, z):
        self.records = np.frombuffer(C.string_at(ptr, R * 48), RECORD_DTYPE).copy()
        self.counts = np.ctypeslib.as_array(counts, shape=(R, 64)).copy()
        return 0


@pytest.mark.parametrize("flags", [[0, 1, 1, 0, 1, 0, 0, 1, 1, 1], [0] * 6, [1] * 5, [1, 0]], ids=["mixed", "none", "all", "two"])
def test_the_python_filters_keep_exactly_the_unflagged_records(flags, monkeypatch):
    from othellozero_amd import _lib, loop, training
    rec, visits = _synthetic(flags)
    keep = np.array(flags) == 0
    kept = int(keep.sum())
    # _lib.full_records, the one filter both use
    r, v = _lib.full_records(rec, visits)
    assert r.tobytes() == rec[keep].tobytes() and np.array_equal(v, visits[keep])
    assert _lib.full_records(rec)[1] is None and _lib.full_records(rec)[0].tobytes() == rec[keep].tobytes()
    # training.expand_examples: what reaches the device
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "require_gpu", lambda: fake)
    boards, pol, z = training.expand_examples(rec, 6)
    assert boards.shape == (8 * kept, 6, 6, 2) and pol.shape == z.shape == (8 * kept,)
    assert (fake.records.tobytes() == rec[keep].tobytes()) if kept else fake.records is None
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "require_gpu", lambda: fake)
    boards, pi, z = training.expand_examples(rec, 6, visits=visits, target_temperature=1.0)
    assert boards.shape == (8 * kept, 6, 6, 2) and pi.shape == (8 * kept, 6, 6)
    if kept:
        assert fake.records.tobytes() == rec[keep].tobytes() and np.array_equal(fake.counts, visits[keep])
    # loop.examples_from_records: what it hands on, and the number of examples it returns
    seen = []
    inner = loop.expand_examples

    def spy(records, board_size, **kw):
        seen.append((np.array(records), None if kw.get("visits") is None else np.array(kw["visits"])))
        return inner(records, board_size, **kw)
    monkeypatch.setattr(loop, "expand_examples", spy)
    assert len(loop.examples_from_records(rec, 6, alias_final=False)) == 8 * kept
    assert len(loop.examples_from_records(rec, 6, alias_final=False, visits=visits)) == 8 * kept
    assert all(s[0].tobytes() == rec[keep].tobytes() for s in seen) and seen[0][1] is None and np.array_equal(seen[1][1], visits[keep])


# ------------------------------------------------------------------ check_playout_cap
GOOD = [((4, 0.25), None, (4, 0.25)), ((2, 1), 12, (2, 1.0)), ([12, 0.5], 12, (12, 0.5)), ((np.int32(6), np.float32(0.5)), 12, (6, 0.5)),
        ((20.0, 1e-9), 100, (20, 1e-9))]
BAD = [((1, 0.25), 12), ((0, 0.25), 12), ((-3, 0.25), 12), ((13, 0.25), 12), ((4, 0.0), 12), ((4, 1.5), 12), ((4, -0.25), 12), ((4, float("nan")), 12),
       ((4.5, 0.25), 12), ((True, 0.25), 12), (("4", 0.25), 12), ((4,), 12), ((4, 0.25, 1), 12), (4, 12), ("fast", 12), ((4, None), 12), ((None, 0.5), 12),
       ({"fast_sims": 4}, 12), ((1, 0.25), None)]


def test_check_playout_cap_accepts_and_refuses():
    from othellozero_amd import _lib
    assert _lib.check_playout_cap(None) is None and _lib.check_playout_cap(None, 12) is None
    for cap, sims, want in GOOD:
        got = _lib.check_playout_cap(cap, sims)
        assert got == want and type(got[0]) is int and type(got[1]) is float, cap
    assert _lib.check_playout_cap((500, 0.25)) == (500, 0.25)                            # no num_simulations given: no upper bound to hold it to


@pytest.mark.parametrize("bad, sims", BAD, ids=repr)
def test_bad_playout_caps_are_a_value_error_before_any_library_call(bad, sims):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, loop, training
    with pytest.raises(ValueError):
        _lib.check_playout_cap(bad, sims)
    if sims is None:
        return
    with pytest.raises(ValueError):
        training.SelfPlayEngine(object(), 6, 4, sims, playout_cap=bad)
    with pytest.raises(ValueError):
        training.selfplay_batch(object(), 6, 4, sims, playout_cap=bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, sims, 1.0, 1, object(), 0.9, 1, 1, None, True, 1, 2, 1, "unused", 100, playout_cap=bad)


# ------------------------------------------------------------------ the restatement itself
def test_restatement_gives_the_figures_it_was_checked_with():
    """6x6, 16 games, ids 200 .. 215, seed 41, 12 simulations, e_greedy 0.8, stub salt 21: (4, 0.25) -> 123 full and 389 fast records, every
    game 32 plies; the flags are the draws; (2, 0.25) runs to the end without the KeyError path; full_prob 1 is the episode without a cap"""
    n, sims, eg, seed, first, G, salt = 6, 12, 0.8, 41, 200, 16, 21
    rec, rows, spent = ref.episodes(n, sims, (4, 0.25), eg, seed, first, G, salt)
    fast = rec["pad"][:, 0]
    assert (int((fast == 0).sum()), int((fast == 1).sum())) == (123, 389) and spent == 123 * sims + 389 * 4
    assert all(int((rec["game_id"] == first + g).sum()) == 32 for g in range(G))
    assert all(int(f) == (0 if ref.is_full(seed, int(g), int(p), 0.25) else 1) for f, g, p in zip(fast, rec["game_id"], rec["ply"]))
    assert (rows.sum(axis=1) >= 3).all() and rows.shape == (rec.size, 64) and not rec["pad"][:, 1:].any()
    low = ref.episodes(n, sims, (2, 0.25), eg, seed, first, G, salt)
    assert low[0].size > 0 and low[2] == int((low[0]["pad"][:, 0] == 0).sum()) * sims + int((low[0]["pad"][:, 0] == 1).sum()) * 2
    plain, one = ref.episodes(n, sims, None, eg, seed, first, 4, salt), ref.episodes(n, sims, (4, 1.0), eg, seed, first, 4, salt)
    assert plain[0].tobytes() == one[0].tobytes() and np.array_equal(plain[1], one[1]) and plain[2] == one[2] == plain[0].size * sims
    assert plain[0].tobytes() != rec[rec["game_id"] < first + 4].tobytes()
