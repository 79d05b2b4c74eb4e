"""Arena openings without a GPU: the new symbols in header, bindings and library; the argument checks of the Python surface (a ValueError before
any library call); loop.pair_statistics on hand-made boards; the restatement (tests/openings_ref.py) against facts that need no kernel."""
import collections
import os
import re

import numpy as np
import pytest

import minimax_ref as mref
import openings_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_arena_set_openings", "oz_arena_set_opening_moves", "oz_arena_opening_plies", "oz_rules_random_openings"]


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"^#define OZ_OPENING_MAX_PLIES 16\b", header, flags=re.M)
    assert _lib.OPENING_MAX_PLIES == ref.MAX_PLIES == 16
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        assert re.search(r"\bOZ_RNG_OPENING = 5\b", f.read())
    assert ref.RNG_OPENING == 5 and (5 - 3) % 256 != 0                        # 5 is not 3 + 256 sq + 65536 i
    assert lib.oz_version() == 230


# ------------------------------------------------------------------ bad arguments
def _moves(g=4, cols=16, dtype=np.uint8):
    return np.zeros((g, cols), dtype)


BAD_OPENINGS = [(1.5, 3), (True, 3), ("4", 3), (17, 3), (-1, 3), (4,), (4, 3, 1), 4, "random", (4, -1), (4, 2.5), (4, None), (4, 2 ** 64), {"plies": 4}]
BAD_MOVES = [(_moves(), ), (_moves(), np.zeros(4, np.int32), 0), _moves(), (_moves(cols=15), np.zeros(4, np.int32)),
             (_moves(dtype=np.int32), np.zeros(4, np.int32)), (_moves(), np.zeros(4, np.int64)), (_moves(), np.zeros(3, np.int32)),
             (_moves(), np.full(4, 17, np.int32)), (_moves(), np.full(4, -1, np.int32)), (_moves().tolist(), [0, 0, 0, 0]),
             (_moves(g=5), np.zeros(5, np.int32)), (_moves().ravel(), np.zeros(4, np.int32)), (_moves(), np.zeros((4, 1), np.int32))]


@pytest.mark.parametrize("bad", BAD_OPENINGS, ids=repr)
def test_bad_openings_are_a_value_error_before_any_library_call(bad):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, agents, loop
    with pytest.raises(ValueError):
        _lib.check_openings(bad)
    with pytest.raises(ValueError):
        agents.arena_batch(object(), None, 6, 4, 8, openings=bad)
    with pytest.raises(ValueError):
        loop.paired_match(6, object(), object(), 4, 8, 1.0, bad)
    with pytest.raises(ValueError):
        loop.self_play_match(6, object(), object(), 4, 8, 1.0, openings=bad)
    with pytest.raises(ValueError):
        loop.evaluate_against_random_batch(6, object(), 4, 8, 1.0, openings=bad)
    with pytest.raises(ValueError):
        loop.evaluate_against_opponent_batch(6, object(), 4, 8, 1.0, ("minimax", 2), openings=bad)
    for option in ("match_openings", "evaluation_openings"):
        with pytest.raises(ValueError):
            loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, True, 1, 2, 1, "unused", 100, batched_evaluation=True, **{option: bad})


@pytest.mark.parametrize("bad", range(len(BAD_MOVES)))
def test_bad_opening_moves_are_a_value_error_before_any_library_call(bad):
    from othellozero_amd import _lib, agents
    with pytest.raises(ValueError):
        _lib.check_openings(None, 0, BAD_MOVES[bad], 4)
    with pytest.raises(ValueError):
        agents.arena_batch(object(), None, 6, 4, 8, opening_moves=BAD_MOVES[bad])


def test_the_other_refusals():
    from othellozero_amd import _lib, agents, loop
    good_moves = (_moves(), np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="one of them"):
        _lib.check_openings((4, 3), 0, good_moves)
    with pytest.raises(ValueError, match="one of them"):
        agents.arena_batch(object(), None, 6, 4, 8, openings=(4, 3), opening_moves=good_moves)
    for bad_id in (-1, 1.5, True, "0", 2 ** 64, None):
        with pytest.raises(ValueError, match="first_opening_id"):
            _lib.check_openings((4, 3), bad_id)
        with pytest.raises(ValueError, match="first_opening_id"):
            agents.arena_batch(object(), None, 6, 4, 8, openings=(4, 3), first_opening_id=bad_id)
    with pytest.raises(ValueError, match="needs openings"):
        loop.paired_match(6, object(), object(), 4, 8, 1.0, None)
    for pairs in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="pairs"):
            loop.paired_match(6, object(), object(), pairs, 8, 1.0, (4, 3))
    for total in (7, 1, 0):
        with pytest.raises(ValueError, match="even"):
            loop.self_play_match(6, object(), object(), total, 8, 1.0, openings=(4, 3))
    with pytest.raises(ValueError, match="even"):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, True, 1, 7, 1, "unused", 100, match_openings=(4, 3))
    with pytest.raises(ValueError, match="batched_evaluation"):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, evaluation_openings=(4, 3),
                      batched_evaluation=False)
    for args in ((6, 4, 17, 7), (6, 4, -1, 7), (6, 4, 2.0, 7), (6, 4, True, 7), (6, -1, 4, 7), (6, 2 ** 22 + 1, 4, 7), (6, 4, 4, -7), (6, 4, 4, 7, -1)):
        with pytest.raises(ValueError):
            agents.rules_random_openings(*args)


def test_good_openings_pass_the_check():
    from othellozero_amd import _lib
    assert _lib.check_openings() is None and _lib.check_openings(None, 5) is None
    assert _lib.check_openings((0, 0)) == ("random", 0, 0, 0)
    assert _lib.check_openings([16, 2 ** 64 - 1], np.int64(9)) == ("random", 16, 2 ** 64 - 1, 9)
    assert _lib.check_openings((np.int32(6), np.uint64(5)), 2 ** 40 + 3) == ("random", 6, 5, 2 ** 40 + 3)
    moves, n_plies = _moves(), np.array([0, 16, 3, 1], np.int32)
    kind, m, k = _lib.check_openings(None, 0, (moves, n_plies), 4)
    assert kind == "moves" and m.flags.c_contiguous and np.array_equal(m, moves) and np.array_equal(k, n_plies)
    assert _lib.check_openings(None, 0, (moves[::2], n_plies[::2]))[1].flags.c_contiguous


# ------------------------------------------------------------------ pair_statistics
def _board(black_discs, white_discs):
    assert black_discs + white_discs <= 64
    return (1 << black_discs) - 1, ((1 << white_discs) - 1) << (64 - white_discs) if white_discs else 0


def test_pair_statistics_on_hand_made_boards():
    """four pairs; (new as BLACK | old as BLACK), discs black-white:
         0: 40-24 | 35-29   new +16, -6    each network wins one game: split
         1: 32-32 | 32-32   two real draws: the first goes to BLACK = new by the reference's rule, the second to BLACK = old
         2: 20-44 | 10-54   new -24, +44   split the other way round
         3: 50-14 | 30-34   new +36, +4    new wins both"""
    from othellozero_amd.loop import pair_statistics
    first = [_board(40, 24), _board(32, 32), _board(20, 44), _board(50, 14)]
    second = [_board(35, 29), _board(32, 32), _board(10, 54), _board(30, 34)]
    u = lambda xs: np.array(xs, np.uint64)          # noqa: E731
    plies = np.array([4, 4, 3, 4], np.int32)
    s = pair_statistics(u([b for b, _ in first]), u([w for _, w in first]), u([b for b, _ in second]), u([w for _, w in second]), plies)
    assert s["pairs"] == 4 and s["margin"].tolist() == [[16, -6], [0, 0], [-24, 44], [36, 4]]
    assert s["pair_margin"].tolist() == [10, 0, 20, 40]
    assert (s["wins"], s["wins_true"], s["draws"], s["losses"]) == (5, 4, 2, 2)
    assert s["wins_true"] + s["draws"] + s["losses"] == 8
    assert s["split_pairs"] == 2 and s["opening_plies"] is plies
    want = np.array([10, 0, 20, 40], np.float64)
    assert s["mean_margin"] == want.mean() == 17.5
    assert s["se"] == pytest.approx(want.std(ddof=1) / 2.0, rel=1e-15)
    # the draw alone: a win by the reference's rule only where new was BLACK
    d = pair_statistics(u([first[1][0]]), u([first[1][1]]), u([second[1][0]]), u([second[1][1]]))
    assert (d["wins"], d["wins_true"], d["draws"], d["losses"], d["split_pairs"]) == (1, 0, 2, 0, 0)
    assert d["mean_margin"] == 0.0 and np.isnan(d["se"]) and d["opening_plies"] is None
    with pytest.raises(ValueError):
        pair_statistics(u([1, 2]), u([4]), u([1]), u([4]))


# ------------------------------------------------------------------ the restatement itself
def _check_is_a_game(n, plies, o):
    (black, white), player, fin = mref.initial_board(n), 1, 0
    assert o["n_plies"] == len(o["actions"]) == len(o["players"]) <= plies
    for sq, who in zip(o["actions"], o["players"]):
        assert not fin and who == player and (mref.legal(black, white, player, n) >> sq) & 1
        black, white, player, fin = mref.play(black, white, player, n, sq)
    assert (black, white, player, fin) == (o["black"], o["white"], o["player"], o["finished"])
    assert fin or o["n_plies"] == plies


@pytest.mark.parametrize("n, plies", [(4, 8), (6, 12), (8, 16), (8, 1), (6, 0)])
def test_restatement_plays_legal_games_and_is_deterministic(n, plies):
    a = ref.openings(n, plies, 7, 0, 48)
    assert a == ref.openings(n, plies, 7, 0, 48)
    for o in a:
        _check_is_a_game(n, plies, o)
    if plies == 0:
        assert all(o["n_plies"] == 0 and (o["black"], o["white"]) == mref.initial_board(n) and o["player"] == 1 for o in a)
    elif plies > 1:
        assert len({tuple(o["actions"]) for o in a}) > 24                      # the ids do spread the games
        assert a != ref.openings(n, plies, 8, 0, 48)                           # and so does the seed


def test_4x4_exercises_passes_and_early_ends():
    """4x4, 8 plies, seed 7, ids 0..255: the case the GPU tests lean on for passes and games that end inside their opening"""
    a = ref.openings(4, 8, 7, 0, 256)
    passes, early = sum(o["passes"] > 0 for o in a), sum(o["finished"] and o["n_plies"] < 8 for o in a)
    print(f"4x4, 8 plies, seed 7: {passes} openings with a pass, {early} ended early")
    assert passes >= 1 and early >= 1
    assert all(o["n_plies"] == 8 or o["finished"] for o in a)


def test_first_moves_are_uniform():
    """4 000 one-ply 8x8 openings at seed 7: each of BLACK's four first moves 1 000 times +- 50 (a binomial's sigma is 27)"""
    hits = collections.Counter(ref.opening(8, 1, 7, k)["actions"][0] for k in range(4000))
    print(sorted(hits.items()))
    assert sorted(hits) == mref.squares(mref.legal(*mref.initial_board(8), 1, 8)) and len(hits) == 4
    assert all(950 <= c <= 1050 for c in hits.values()), hits


def test_windows_of_opening_ids_overlap():
    w0, w3 = ref.openings(6, 6, 5, 0, 12), ref.openings(6, 6, 5, 3, 12)
    assert all(w0[k] == w3[k - 3] for k in range(3, 12))
    assert w0[:3] != w3[:3]
    big = 2 ** 40 + 3
    assert ref.openings(6, 6, 5, big, 4)[1:] == ref.openings(6, 6, 5, big + 1, 3)
