"""The minimax opponent without a GPU: the new symbols in header, bindings and library; the restatement (tests/minimax_ref.py) against facts that
need no kernel; the argument checks of the Python surface."""
import os
import re

import pytest

import minimax_ref as ref
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_rules_minimax", "oz_arena_set_opponent", "oz_arena_opponent_time"]

TABLE = {
    4: [[100, -20, -20, 100],
        [-20, -50, -50, -20],
        [-20, -50, -50, -20],
        [100, -20, -20, 100]],
    6: [[100, -20, 10, 10, -20, 100],
        [-20, -50, -2, -2, -50, -20],
        [10, -2, 1, 1, -2, 10],
        [10, -2, 1, 1, -2, 10],
        [-20, -50, -2, -2, -50, -20],
        [100, -20, 10, 10, -20, 100]],
    8: [[100, -20, 10, 10, 10, 10, -20, 100],
        [-20, -50, -2, -2, -2, -2, -50, -20],
        [10, -2, 1, 1, 1, 1, -2, 10],
        [10, -2, 1, 1, 1, 1, -2, 10],
        [10, -2, 1, 1, 1, 1, -2, 10],
        [10, -2, 1, 1, 1, 1, -2, 10],
        [-20, -50, -2, -2, -2, -2, -50, -20],
        [100, -20, 10, 10, 10, 10, -20, 100]],
}


def _mask(squares):
    m = 0
    for s in squares:
        m |= 1 << s
    return m


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    for name, val in (("OZ_MINIMAX_EVAL_DISCS", "0"), ("OZ_MINIMAX_EVAL_WEIGHTED", "1"), ("OZ_MINIMAX_MAX_DEPTH", "6"), ("OZ_MINIMAX_NONE", "INT32_MIN"),
                      ("OZ_AGENT_RANDOM", "0"), ("OZ_AGENT_MINIMAX", "1")):
        assert re.search(r"^#define %s %s\b" % (name, val), header, flags=re.M), name
    assert header.count("agents.py:27-41") >= len(NEW_SYMBOLS)
    assert lib.oz_version() == 230
    assert (_lib.MINIMAX_EVAL_DISCS, _lib.MINIMAX_EVAL_WEIGHTED, _lib.MINIMAX_MAX_DEPTH, _lib.MINIMAX_NONE) == (0, 1, 6, ref.NONE)
    assert (_lib.AGENT_RANDOM, _lib.AGENT_MINIMAX) == (0, 1)


@pytest.mark.parametrize("n", [4, 6, 8])
def test_weight_table_written_out(n):
    assert [[ref.weight(n, r, c) for c in range(n)] for r in range(n)] == TABLE[n]
    flat = [x for row in TABLE[n] for x in row]
    if n == 8:
        assert sum(x for x in flat if x > 0) == 576 and sum(flat) == 184
        assert sum(abs(x) for x in flat) == 968 < 1000       # the largest |E|: any decided game (|T| >= 1000) outranks every static value
    full = _mask(r * 8 + c for r in range(n) for c in range(n))
    assert ref.static(full, 0, 1, n, ref.WEIGHTED) == sum(flat) == -ref.static(full, 0, -1, n, ref.WEIGHTED)
    assert ref.static(full, 0, 1, n, ref.DISCS) == n * n


@pytest.mark.parametrize("n", [6, 8])
def test_depth_one_on_discs_is_the_greedy_agent(n):
    """a move that flips f discs leaves own + 1 + f against opp - f, finished or not: depth 1 on the disc count picks the moves that flip the most"""
    L = oracle.lib()
    seen = 0
    for black, white, player in ref.playout_positions(n, 77, 3):
        moves = ref.legal(black, white, player, n)
        flips = {sq: ref.popcount(L.orc_flip_mask(black, white, n, 0 if player == 1 else 1, sq)) for sq in ref.squares(moves)}
        values, bests = ref.root(black, white, player, n, 1, ref.DISCS)
        own, opp = (black, white) if player == 1 else (white, black)
        for sq, f in flips.items():
            assert values[sq] == ref.popcount(own) - ref.popcount(opp) + 1 + 2 * f
        assert bests == _mask(sq for sq, f in flips.items() if f == max(flips.values()))
        assert all(values[sq] == ref.NONE for sq in range(64) if not (moves >> sq) & 1)
        seen += len(flips) > 1
    assert seen > 20


def test_a_reply_that_is_a_pass_keeps_the_sign():
    """Rows 0 and 7 each hold B W _ from the left, BLACK to move.  BLACK plays (0, 2): WHITE's only disc (7, 1) brackets nothing, BLACK still has
    (7, 2): the turn passes back (s = +1).  BLACK then takes the last WHITE disc: 6 - 0 and the game is over."""
    n, black, white = 8, _mask((0, 56)), _mask((1, 57))
    assert ref.legal(black, white, 1, n) == _mask((2, 58))
    b, w, p, f = ref.play(black, white, 1, n, 2)
    assert (b, w, p, f) == (_mask((0, 1, 2, 56)), _mask((57,)), 1, 0)          # the same mover again
    stats = {}
    values, bests = ref.root(black, white, 1, n, 2, ref.DISCS, stats)
    assert values[2] == values[58] == 6 and bests == _mask((2, 58)) and stats["passes"] == 2
    assert ref.root(black, white, 1, n, 1, ref.DISCS)[0][2] == 3               # E of the child, for BLACK: 4 - 1
    # weighted, depth 1: own a1 (100), b1 (-20), c1 (10), a8 (100) against b8 (-20): 190 + 20; depth 2: the decided game, 1000 * 6
    assert ref.root(black, white, 1, n, 1, ref.WEIGHTED)[0][2] == 210
    assert ref.root(black, white, 1, n, 2, ref.WEIGHTED)[0][2] == 6000
    # the same position seen by WHITE (colours swapped): antisymmetric in the mover
    assert ref.root(white, black, -1, n, 2, ref.DISCS) == (values, bests)


@pytest.mark.parametrize("depth", [1, 2, 6])
def test_one_move_from_the_end_takes_the_terminal_value(depth):
    """B W _ : BLACK takes the only WHITE disc, nobody can move: T whatever the depth, x 1000 under the weighted evaluation; the finished child's
    stored player is WHITE (orc_game_play switches before it looks), T for WHITE is -3, s = -1"""
    n, black, white = 8, _mask((0,)), _mask((1,))
    assert ref.play(black, white, 1, n, 2) == (_mask((0, 1, 2)), 0, -1, 1)
    assert ref.root(black, white, 1, n, depth, ref.DISCS) == ([3 if s == 2 else ref.NONE for s in range(64)], 1 << 2)
    assert ref.root(black, white, 1, n, depth, ref.WEIGHTED)[0][2] == 3000
    # a finished board, and a mover without a move: nothing to play
    assert ref.root(_mask((0, 1, 2)), 0, -1, n, depth, ref.DISCS) == ([ref.NONE] * 64, 0)
    assert ref.root(_mask((0, 1, 2, 56)), _mask((57,)), -1, n, depth, ref.DISCS) == ([ref.NONE] * 64, 0)


def test_arena_move_is_the_kth_best_by_the_tie_stream():
    bests = _mask((3, 19, 44))
    picks = {ref.arena_move(bests, 5, g, g % 9) for g in range(60)}
    assert picks == {3, 19, 44}
    assert ref.arena_move(1 << 17, 5, 0, 0) == 17
    assert ref.arena_move(bests, 5, 7, 3) == ref.kth_bit(bests, ref.rng(5, 7, 3, 2) % 3)


BAD_OPPONENTS = ["greedy", ("greedy", 2), ("minimax",), ("minimax", 0), ("minimax", 7), ("minimax", 2, "mobility"), ("minimax", 2.5), ("minimax", "2"),
                 ("minimax", True), ("minimax", 2, "discs", 1), ("minimax", 2, None), 3, ("random", 2)]


@pytest.mark.parametrize("bad", BAD_OPPONENTS)
def test_bad_opponent_is_a_value_error_before_any_library_call(bad):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, agents, loop
    with pytest.raises(ValueError):
        _lib.check_opponent(bad)
    with pytest.raises(ValueError):
        agents.arena_batch(object(), None, 6, 4, 8, opponent=bad)
    with pytest.raises(ValueError):
        loop.evaluate_against_random_batch(6, object(), 4, 8, 1.0, opponent=bad)
    with pytest.raises(ValueError):
        loop.evaluate_against_random(6, object(), 4, 8, 1.0, opponent=bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, evaluation_opponent=bad)


@pytest.mark.parametrize("depth, evaluation", [(0, "weighted"), (7, "weighted"), (-1, "discs"), (2.0, "discs"), ("3", "discs"), (True, "discs"),
                                               (3, "mobility"), (3, 1), (3, None)])
def test_bad_minimax_agent_arguments(depth, evaluation):
    from othellozero_amd import _lib, agents
    from othellozero_amd.Othello import OthelloGame
    with pytest.raises(ValueError):
        _lib.check_minimax(depth, evaluation)
    with pytest.raises(ValueError):
        agents.MinimaxOthelloAgent(OthelloGame(6), depth, evaluation)
    with pytest.raises(ValueError):
        agents.rules_minimax([1], [2], [1], 6, depth, evaluation)


def test_good_opponents_pass_the_check():
    from othellozero_amd import _lib, agents
    from othellozero_amd.Othello import OthelloGame
    assert _lib.check_opponent(None) is None and _lib.check_opponent("random") is None
    assert _lib.check_opponent(("minimax", 1)) == (1, _lib.MINIMAX_EVAL_WEIGHTED)
    assert _lib.check_opponent(["minimax", 6, "discs"]) == (6, _lib.MINIMAX_EVAL_DISCS)
    assert _lib.check_opponent(("minimax", 3, "weighted")) == (3, _lib.MINIMAX_EVAL_WEIGHTED)
    a = agents.MinimaxOthelloAgent(OthelloGame(6))
    assert (a.depth, a.evaluation) == (3, "weighted")
    with pytest.raises(ValueError, match="both colours"):
        agents.arena_batch(object(), object(), 6, 4, 8, opponent=("minimax", 2))
