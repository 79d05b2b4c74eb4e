"""Solved leaves without a GPU: the new symbols in header, bindings and library; the restatement's wrapper (tests/solve_leaves_ref.py)
against the endgame restatement; the argument checks of the Python surface; the defaults."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import endgame_ref as eg
import minimax_ref as ref
import oracle
import solve_leaves_ref as slr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_rules_solve_sign", "oz_mcts_set_solve_leaves", "oz_mcts_get_solve_leaves", "oz_selfplay_set_solve_leaves",
               "oz_arena_set_solve_leaves", "oz_selfplay_get_solve_leaves", "oz_arena_get_solve_leaves", "oz_mcts_solve_leaves_profile",
               "oz_mcts_solve_leaves_profile_read", "oz_selfplay_solve_leaves_profile", "oz_selfplay_solve_leaves_profile_read"]
BAD = [-1, 11, 2.0, "8", True, None]


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
    assert re.search(r"^#define OZ_SOLVE_LEAVES_MAX_EMPTIES 10\b", header, flags=re.M) and _lib.SOLVE_LEAVES_MAX_EMPTIES == 10
    assert _lib.SOLVE_LEAVES_MAX_EMPTIES < _lib.SOLVE_MAX_EMPTIES
    assert lib.oz_version() == 230
    assert C.sizeof(_lib.SelfplayConfig) == 96                  # the option goes through a call, not through the config
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(name in text for name in NEW_SYMBOLS[:5])


def _wrapper_vs_restatement(n, E, salt, positions, seen):
    ev = slr.evaluator(E, slr.stub(salt))
    above, solved, draws = 0, 0, 0
    for b, w, p in positions:
        own, opp = (b, w) if p == 1 else (w, b)
        pi0, v0 = oracle.stub_predict(own, opp, n, salt, 0)
        pi, v = ev(own, opp, n)
        assert np.array_equal(pi, pi0)
        if eg.empties(b, w, n) <= E:
            s = slr.sign(eg.root(own, opp, 1, n)[2])
            assert float(v) == float(s) and isinstance(v, np.float32) and s == slr.sign(eg.root(b, w, p, n)[2])
            seen[s] += 1
            solved, draws = solved + 1, draws + (s == 0)
        else:
            assert v == v0
            above += 1
    assert solved >= 20 and above >= 20, (n, solved, above)
    assert (ev.calls, ev.solved, ev.draws) == (solved + above, solved, draws)


def test_wrapper_equals_the_sign_of_the_endgame_restatement():
    """v = float(sign(S)) with S = endgame_ref.root(...)[2] for own to move where the board has at most E empties, the inner evaluator's v
    above; pi is the inner evaluator's always.  Among the positions: a drawn one and one whose mover must pass."""
    salt = 3
    seen = {-1: 0, 0: 0, 1: 0}
    for n, E, positions in ((6, 7, ref.playout_positions(6, 2024, 6)), (4, 6, ref.playout_positions(4, 5, 40))):
        _wrapper_vs_restatement(n, E, salt, positions, seen)
    assert min(seen.values()) >= 1, seen                                 # wins, losses and draws
    n = 6
    # the mover must pass: row 0 = B W _ on an otherwise full 6x6 board of BLACK discs, WHITE to move has nothing, BLACK takes (0, 2)
    full = _mask(r * 8 + c for r in range(n) for c in range(n))
    black, white = full & ~_mask((1, 2)), _mask((1,))
    assert ref.legal(black, white, -1, n) == 0 and ref.legal(black, white, 1, n) == _mask((2,))
    assert eg.root(white, black, 1, n)[2] == -n * n                      # own = WHITE's discs
    assert float(slr.evaluator(2, slr.stub(salt))(white, black, n)[1]) == -1.0
    assert float(slr.evaluator(2, slr.stub(salt))(black, white, n)[1]) == 1.0
    # a finished drawn board
    half = _mask(r * 8 + c for r in range(3) for c in range(n))
    assert float(slr.evaluator(0, slr.stub(salt))(half, full & ~half, n)[1]) == 0.0


def test_search_inputs_of_the_gpu_tables():
    """the first case of tests/test_gpu_solve_leaves.py's table test, on the oracle alone: roots, evaluations, solved leaves, draws"""
    n, E, sims, salt = 6, 6, 64, 3
    roots = [p for p in ref.playout_positions(n, 2025, 3) if 8 <= eg.empties(p[0], p[1], n) <= 11]
    ev = slr.evaluator(E, slr.stub(salt))
    for b, w, p in roots:
        m = oracle.Mcts(n, 1.0, 1, evaluator=ev)
        for _ in range(sims):
            m.simulate(b, w, p)
    assert (len(roots), ev.calls, ev.solved, ev.draws) == (12, 750, 391, 3)


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_bad_values_are_value_errors_before_any_library_call(bad):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, agents, loop, training
    from othellozero_amd.Othello import OthelloGame
    from othellozero_amd.othelo_mcts import OthelloMCTS
    with pytest.raises(ValueError):
        _lib.check_solve_leaves(bad)
    with pytest.raises(ValueError):
        OthelloMCTS(6, object(), 1.0, solve_leaves=bad)
    with pytest.raises(ValueError):
        agents.NeuralNetworkOthelloAgent(OthelloGame(6), object(), 8, 1.0, solve_leaves=bad)
    with pytest.raises(ValueError):
        training.SelfPlayEngine(object(), 6, 4, 8, solve_leaves=bad)
    with pytest.raises(ValueError):
        training.SelfPlayEngine.set_solve_leaves(object(), bad)
    with pytest.raises(ValueError):
        training.selfplay_batch(object(), 6, 4, 8, solve_leaves=bad)
    with pytest.raises(ValueError):
        training.execute_episode(6, object(), 1.0, 8, 1, 0.9, solve_leaves=bad)
    with pytest.raises(ValueError):
        agents.arena_batch(object(), object(), 6, 4, 8, solve_leaves=bad)
    with pytest.raises(ValueError):
        agents.arena_batch(object(), object(), 6, 4, 8, solve_leaves=(6, bad))
    with pytest.raises(ValueError):
        loop.evaluate_against_random_batch(6, object(), 4, 8, 1.0, solve_leaves=bad)
    with pytest.raises(ValueError):
        loop.evaluate_against_opponent_batch(6, object(), 4, 8, 1.0, ("minimax", 1), solve_leaves=bad)
    with pytest.raises(ValueError):
        loop.self_play_match(6, object(), object(), 4, 8, 1.0, solve_leaves=bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, solve_leaves=bad)


def test_pairs_and_the_bound():
    from othellozero_amd import _lib, agents
    assert _lib.check_solve_leaves(0) == 0 and _lib.check_solve_leaves(10) == 10 and _lib.check_solve_leaves(np.int64(6)) == 6
    assert _lib.check_solve_leaves_pair(6) == (6, 6) and _lib.check_solve_leaves_pair((6, 0)) == (6, 0) and _lib.check_solve_leaves_pair([0, 10]) == (0, 10)
    for bad in [(6,), (6, 6, 6), (6, 11), "66"]:
        with pytest.raises(ValueError):
            _lib.check_solve_leaves_pair(bad)
    with pytest.raises(ValueError):
        agents.rules_solve_sign([1], [2], [1], 6, 13)           # the batch entry keeps the solver's own bound, 12
    with pytest.raises(ValueError):
        agents.rules_solve_sign([1], [2], [1], 6, True)


def test_a_duck_typed_network_cannot_have_solved_leaves():
    from othellozero_amd.othelo_mcts import OthelloMCTS

    class Net:
        network_type = None

        def predict(self, board):
            raise AssertionError("never called")
    with pytest.raises(ValueError, match="native"):
        OthelloMCTS(6, Net(), 1.0, solve_leaves=6)


def test_defaults_are_zero_everywhere():
    from othellozero_amd import agents, loop, training
    from othellozero_amd.othelo_mcts import OthelloMCTS
    for fn in (OthelloMCTS.__init__, agents.NeuralNetworkOthelloAgent.__init__, training.SelfPlayEngine.__init__, training.selfplay_batch,
               training.execute_episode, agents.arena_batch, loop.evaluate_against_random_batch, loop.evaluate_against_opponent_batch,
               loop.self_play_match, loop.training):
        assert inspect.signature(fn).parameters["solve_leaves"].default == 0, fn


def test_default_search_makes_no_new_library_call(monkeypatch):
    """an OthelloMCTS built without the argument calls what it called before: the library is replaced by a recorder"""
    from othellozero_amd import _lib
    from othellozero_amd.othelo_mcts import OthelloMCTS
    calls = []

    class Recorder:
        def __getattr__(self, name):
            def call(*args):
                calls.append(name)
                return 0
            return call

    class Net:
        network_type = None
        _h = C.c_void_p(1)
    monkeypatch.setattr(_lib, "require_gpu", lambda: Recorder())
    monkeypatch.setattr(_lib, "load", lambda: Recorder())
    m = OthelloMCTS(6, Net(), 1.0)
    assert m.solve_leaves == 0 and calls == ["oz_mcts_create"]
    del m
    calls.clear()
    m = OthelloMCTS(6, Net(), 1.0, solve_leaves=6)
    assert m.solve_leaves == 6 and calls == ["oz_mcts_create", "oz_mcts_set_solve_leaves"]
    del m
