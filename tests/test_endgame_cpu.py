"""The exact endgame solver without a GPU: the new symbols in header, bindings and library; the restatement (tests/endgame_ref.py) against the
minimax restatement at depth = empties; the z rule; the argument checks of the Python surface."""
import os
import re

import pytest

import endgame_ref as eg
import minimax_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_rules_solve", "oz_selfplay_solve_records", "oz_rules_profile", "oz_rules_profile_read"]


def _mask(squares):
    m = 0
    for s in squares:
        m |= 1 << s
    return m


def test_new_symbols_in_header_bindings_and_library():
    import ctypes as C
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"^#define OZ_SOLVE_MAX_EMPTIES 12\b", header, flags=re.M) and _lib.SOLVE_MAX_EMPTIES == eg.MAX_EMPTIES == 12
    assert "oz_endgame_stats" in header and C.sizeof(_lib.EndgameStats) == 48
    assert [name for name, _ in _lib.EndgameStats._fields_] == ["records", "solved", "z_changed", "optimal_moves", "disc_loss_sum", "disc_loss_max", "pad"]
    assert lib.oz_version() == 230
    assert C.sizeof(_lib.SelfplayConfig) == 96                  # the new state goes through a call, not through the config
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(name in text for name in NEW_SYMBOLS)


def test_restatement_equals_the_minimax_restatement_at_depth_empties_on_4x4():
    """S is V on the disc count with the horizon at the end of the game: depth = empties reaches every finished board"""
    n, seen, deepest = 4, 0, 0
    for black, white, player in ref.playout_positions(n, 11, 3):
        e = eg.empties(black, white, n)
        if e > 9:                                               # (the unmemoised minimax restatement walks the whole tree)
            continue
        values, bests = ref.root(black, white, player, n, max(e, 1), ref.DISCS)
        got = eg.root(black, white, player, n)
        assert (got[0], got[1]) == (values, bests), (black, white, player)
        assert got[2] == max(v for v in values if v != eg.NONE)
        seen, deepest = seen + 1, max(deepest, e)
    assert seen >= 20 and deepest == 9


def test_pass_finished_board_and_early_end():
    n, black, white = 8, _mask((0, 56)), _mask((1, 57))        # rows 0 and 7 hold B W _ : either BLACK move makes WHITE pass, then 6 - 0
    values, bests, s = eg.root(black, white, 1, n)
    assert values[2] == values[58] == 6 and bests == _mask((2, 58)) and s == 6
    assert eg.facts(black, white, 1, n) == (True, True)
    assert eg.root(white, black, -1, n) == (values, bests, s)  # antisymmetric in the mover
    # a finished board, for either mover
    assert eg.root(_mask((0, 1, 2)), 0, 1, n) == ([eg.NONE] * 64, 0, 3)
    assert eg.root(_mask((0, 1, 2)), 0, -1, n) == ([eg.NONE] * 64, 0, -3)
    # WHITE has no move, BLACK takes (7, 2) and the last WHITE disc: the value after the pass, for WHITE
    assert eg.root(_mask((0, 1, 2, 56)), _mask((57,)), -1, n) == ([eg.NONE] * 64, 0, -6)


@pytest.mark.parametrize("player", [1, -1])
def test_z_rule(player):
    assert eg.z_of(5, player) == 1 and eg.z_of(-1, player) == -1
    assert eg.z_of(0, player) == (1 if player == 1 else -1)    # a draw goes to BLACK: +1 for BLACK's records, -1 for WHITE's
    # a drawn position through relabel: the record had the other sign
    import numpy as np
    from othellozero_amd import _lib
    n = 4
    drawn = [(b, w, p) for b, w, p in ref.playout_positions(n, 5, 40) if eg.empties(b, w, n) <= 6 and p == player and eg.value(b, w, p, n) == 0]
    assert drawn, "no drawn position for this mover among the playouts"
    b, w, p = drawn[0]
    rec = np.zeros(1, _lib.RECORD_DTYPE)
    rec["black"], rec["white"], rec["player"], rec["z"] = b, w, p, -eg.z_of(0, p)
    rec["action"] = ref.squares(eg.root(b, w, p, n)[1])[0]
    z, stats = eg.relabel(rec, n, 6)
    assert z == [1 if p == 1 else -1] and stats == dict(records=1, solved=1, z_changed=1, optimal_moves=1, disc_loss_sum=0, disc_loss_max=0)
    assert eg.relabel(rec, n, 1)[1]["solved"] == (1 if eg.empties(b, w, n) <= 1 else 0)


@pytest.mark.parametrize("bad", [-1, 13, 2.0, "8", True, None])
def test_bad_empties_are_value_errors_before_any_library_call(bad):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, agents, loop, training
    from othellozero_amd.Othello import OthelloGame
    with pytest.raises(ValueError):
        _lib.check_solve_empties(bad)
    with pytest.raises(ValueError):
        agents.rules_solve([1], [2], [1], 6, bad)
    with pytest.raises(ValueError):
        agents.MinimaxOthelloAgent(OthelloGame(6), solve_empties=bad)
    with pytest.raises(ValueError):
        training.selfplay_batch(object(), 6, 4, 8, endgame_targets=bad)
    with pytest.raises(ValueError):
        training.SelfPlayEngine.solve_records(object(), bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, alias_final_boards=False, endgame_targets=bad)


def test_endgame_targets_need_the_position_of_the_move():
    from othellozero_amd import _lib, loop, training
    with pytest.raises(ValueError, match="alias_final_boards=False"):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, endgame_targets=8)
    with pytest.raises(ValueError, match="alias_final"):
        training.selfplay_batch(object(), 6, 4, 8, expand=True, alias_final=True, endgame_targets=8)
    with pytest.raises(ValueError):
        training.SelfPlayEngine.solve_records(object(), 0)      # 0 is "off" for the keywords, not a bound to solve to
    assert _lib.check_endgame_targets(0, True) == 0 and _lib.check_endgame_targets(12, False) == 12
    assert _lib.check_solve_empties(0) == 0 and _lib.check_solve_empties(12) == 12


def test_default_agent_is_todays_agent():
    from othellozero_amd import agents
    from othellozero_amd.Othello import OthelloGame
    a = agents.MinimaxOthelloAgent(OthelloGame(6))
    assert (a.depth, a.evaluation, a.solve_empties) == (3, "weighted", 0)
    assert agents.MinimaxOthelloAgent(OthelloGame(6), 2, "discs", solve_empties=8).solve_empties == 8
