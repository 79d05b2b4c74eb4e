"""Move sampling without a GPU: the properties of the restatement (tests/move_sampling_ref.py), its distribution against N ** (1 / T) / sum,
the new symbols in header and bindings, and the argument checks of the Python surface."""
import math
import os
import re

import pytest

from move_sampling_ref import RNG_SAMPLE, sample, sample_with, selfplay_move, unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_mcts_sample_moves", "oz_selfplay_set_move_sampling"]
COUNTS = {2: 1, 11: 3, 20: 7, 29: 12, 42: 2}              # the distribution test's root: five visited squares ...
UNVISITED = 33                                             # ... and a legal one the search never went to
TOP = 1.0 - 2.0 ** -53                                     # the largest unit draw


def _row(counts):
    row = [0] * 64
    for s, c in counts.items():
        row[s] = c
    return row


def _mask(squares):
    m = 0
    for s in squares:
        m |= 1 << s
    return m


@pytest.mark.parametrize("T", [0.01, 0.25, 1.0, 3.0, 100.0])
def test_an_unvisited_square_is_never_picked(T):
    counts = {0: 0, 5: 4, 9: 0, 17: 1, 40: 0, 63: 0}       # unvisited squares first, last and in between
    row, legal = _row(counts), _mask(counts)
    for i in range(2001):
        for u in (i / 2001.0, min(i / 2001.0 + 1e-17, TOP)):
            assert sample_with(row, legal, T, u)[0] in (5, 17), (T, u)
    for u in (0.0, TOP, 1.0):
        assert sample_with(row, legal, T, u)[0] in (5, 17), (T, u)
    for g in range(500):
        assert sample(row, legal, T, 7, g, g % 5)[0] in (5, 17)


@pytest.mark.parametrize("T", [0.01, 1.0, 100.0])
def test_a_single_visited_move_is_always_played(T):
    for sq, legal in ((0, 1), (19, _mask((3, 19, 44))), (63, _mask((0, 63))), (44, _mask((3, 19, 44)))):
        row = _row({sq: 11})
        for u in (0.0, 0.5, TOP, 1.0):
            assert sample_with(row, legal, T, u)[0] == sq
        for g in range(50):
            action, margin = sample(row, legal, T, 3, g, 0)
            assert action == sq and margin >= 0.0


def test_the_top_of_the_range_takes_the_fallback():
    """the fallback (no legal square with cum > r) is for r == c_total.  u * c with u <= 1 - 2**-53 is below c for every float c (the
    decrement c * 2**-53 is at least half an ulp of c, and exactly representable where it is half), so the branch is exercised with u = 1.0:
    the last legal square WITH A VISIT, not the last legal square"""
    row, legal = _row(COUNTS), _mask(list(COUNTS) + [UNVISITED, 50])
    action, margin = sample_with(row, legal, 1.0, 1.0)
    assert action == 42 and margin == 0.0                  # 50 is legal and later, but unvisited
    assert sample_with(row, legal, 1.0, TOP)[0] == 42      # just below the top: still the last visited square, by the first rule
    assert sample_with(row, legal, 1.0, 0.0)[0] == 2
    assert sample_with(_row({2: 1, 11: 1}), _mask((2, 11)), 1.0, 0.5)[0] == 11       # r == cum[2] exactly: `>` is strict


def test_maximum_gets_weight_one_and_boundaries_follow_the_counts():
    """T = 1 on counts (1, 3, 4): w = (0.25, 0.75, 1.0), cum = (0.25, 1.0, 2.0): u picks by r = 2 u"""
    row, legal = _row({1: 1, 8: 3, 9: 4}), _mask((1, 8, 9))
    for u, want in ((0.0, 1), (0.124, 1), (0.125, 8), (0.49, 8), (0.5, 9), (0.99, 9)):
        assert sample_with(row, legal, 1.0, u)[0] == want, u
    assert sample_with(row, legal, 1.0, 0.25)[1] == pytest.approx(0.125)          # r = 0.5: a quarter off 0.25, of c = 2


@pytest.mark.parametrize("T", [0.25, 0.5, 1.0, 3.0])
@pytest.mark.parametrize("seed", [41, 1234])
def test_distribution_is_n_to_the_one_over_t(seed, T):
    """20 000 draws keyed (seed, g, g % 7): Pearson's chi-square over the five visited squares against N ** (1 / T) / sum stays below 18.47,
    the 99.9 % point at 4 degrees of freedom"""
    draws = 20000
    row, legal = _row(COUNTS), _mask(list(COUNTS) + [UNVISITED])
    seen, smallest = dict.fromkeys(COUNTS, 0), math.inf
    for g in range(draws):
        action, margin = sample(row, legal, T, seed, g, g % 7)
        assert action != UNVISITED
        seen[action] += 1
        smallest = min(smallest, margin)
    total = sum(c ** (1.0 / T) for c in COUNTS.values())
    chi2 = sum((seen[s] - draws * c ** (1.0 / T) / total) ** 2 / (draws * c ** (1.0 / T) / total) for s, c in COUNTS.items())
    print(f"seed {seed} T {T}: chi-square {chi2:.2f} (bound 18.47), smallest margin {smallest:.2e}, counts {seen}")
    assert chi2 < 18.47, (seed, T, chi2, seen)


def test_the_draw_is_one_stream_of_its_own():
    assert RNG_SAMPLE == 4 and all(RNG_SAMPLE != 3 + 256 * sq + 65536 * i for sq in range(64) for i in range(49))
    u = unit(9, 4, 11, RNG_SAMPLE)
    assert 0.0 <= u < 1.0 and len({u, unit(9, 4, 11, 0), unit(9, 4, 11, 1), unit(9, 4, 11, 2), unit(9, 5, 11, RNG_SAMPLE), unit(9, 4, 12, RNG_SAMPLE),
                                   unit(10, 4, 11, RNG_SAMPLE)}) == 7


def test_selfplay_move_rule_of_the_restatement():
    """the coin first; sampling only on its greedy branch and only below `plies`; everything else is the rule without sampling"""
    row, legal = _row(COUNTS), _mask(list(COUNTS) + [UNVISITED])
    kinds = set()
    for g in range(400):
        ply = g % 10
        plain = selfplay_move(row, legal, 0.8, 5, g, ply)
        got = selfplay_move(row, legal, 0.8, 5, g, ply, (1.0, 6))
        assert plain[1] in (0, 1) and (plain[1] == 0 or plain[0] == 29)
        if plain[1] == 0 or ply >= 6:
            assert got == plain
        else:
            assert got[1] == 2 and got[0] == sample(row, legal, 1.0, 5, g, ply)[0]
        kinds.add(got[1])
        assert selfplay_move(row, legal, 0.8, 5, g, ply, (1.0, 0)) == plain
    assert kinds == {0, 1, 2}


def test_new_symbols_in_header_and_bindings():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.oz_version() == 230
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        assert re.search(r"OZ_RNG_SAMPLE\s*=\s*4\b", f.read())


@pytest.mark.parametrize("bad", [(1.0,), (1.0, 6, 1), (0.001, 6), (100.5, 6), (float("nan"), 6), (float("inf"), 6), (-1.0, 6), (1.0, -1), (1.0, 65),
                                 (1.0, 2.5), (1.0, float("nan")), (1.0, "x"), ("x", 6), (1.0, None), "ab", 1.0])
def test_bad_sample_moves_is_a_value_error_before_any_library_call(bad):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, loop, training
    with pytest.raises(ValueError):
        _lib.check_sample_moves(bad)
    with pytest.raises(ValueError):
        training.SelfPlayEngine(object(), 6, 4, 8, sample_moves=bad)
    with pytest.raises(ValueError):
        training.selfplay_batch(object(), 6, 4, 8, sample_moves=bad)
    with pytest.raises(ValueError):
        training.execute_episode(6, object(), 1.0, 8, 1, 1.0, sample_moves=bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, sample_moves=bad)


def test_good_sample_moves_pass_the_check():
    from othellozero_amd import _lib
    assert _lib.check_sample_moves(None) is None
    assert _lib.check_sample_moves((1, 6)) == (1.0, 6) and isinstance(_lib.check_sample_moves((1, 6))[1], int)
    assert _lib.check_sample_moves([0.01, 0]) == (0.01, 0) and _lib.check_sample_moves((100.0, 64)) == (100.0, 64)
    assert _lib.check_sample_moves((0.5, 6.0)) == (0.5, 6)
