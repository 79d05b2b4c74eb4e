"""Value signs of the backup without a GPU: the library's host functions (oz_search_backup_values / oz_search_terminal_value through
agents.rules_*) against the plain-Python restatement in tests/value_signs_ref.py, bit for bit; the restatement's search in reference mode
against WideSearch; and the argument checks of the Python surface."""
import itertools
import random
import struct

import numpy as np
import pytest

from value_signs_ref import MODES, POSITIONS_6, SoundSearch, backup_values, random_position, terminal_value
from wide_search_ref import WideSearch, initial_board

LEAVES = (1.0, -1.0, 0.0, -0.0, 0.37, -0.8125, float(np.float32(0.1)), 1e-30)


@pytest.fixture(scope="module")
def agents():
    from othellozero_amd import agents
    return agents


def bits(x):
    return struct.pack("<d", float(x))


def check(agents, mode, sigma, leaf):
    got, last = agents.rules_backup_values(mode, sigma, leaf)
    want, want_last = backup_values(mode, list(sigma), leaf)
    assert got.dtype == np.float64 and len(got) == len(sigma)
    assert [bits(x) for x in got] == [bits(x) for x in want], (mode, sigma, leaf)
    assert bits(last) == bits(want_last), (mode, sigma, leaf)


def test_positions_are_what_random_position_gives():
    assert tuple(random_position(6, 8, seed) for seed in (0, 2, 7, 23)) == POSITIONS_6


@pytest.mark.parametrize("mode", MODES)
def test_backup_values_all_patterns_to_depth_6(agents, mode):
    for depth in range(7):
        for sigma in itertools.product((0, 1), repeat=depth):
            for leaf in LEAVES:
                check(agents, mode, sigma, leaf)


@pytest.mark.parametrize("mode", MODES)
def test_backup_values_random_patterns_to_depth_60(agents, mode):
    rng = random.Random(5)
    for _ in range(300):
        depth = rng.randint(7, 60)
        sigma = [rng.randint(0, 1) if rng.random() < 0.8 else 1 for _ in range(depth)]
        check(agents, mode, sigma, rng.choice(LEAVES) if rng.random() < 0.5 else rng.uniform(-1.0, 1.0))
    check(agents, mode, [1] * 64, 0.25)
    check(agents, mode, [0] * 64, -0.25)


def test_backup_values_mean_what_the_definition_says(agents):
    # no pass anywhere: the two rules agree
    for depth in range(1, 9):
        a, la = agents.rules_backup_values("sound", [1] * depth, 0.5)
        b, lb = agents.rules_backup_values("reference", [1] * depth, 0.5)
        assert np.array_equal(a, b) and la == lb
        assert a[-1] == -0.5                               # the side that moved into the leaf sees the leaf's mover's value negated
    # depth 0: minus the leaf's value in both
    for mode in MODES:
        vals, last = agents.rules_backup_values(mode, [], 0.75)
        assert len(vals) == 0 and last == -0.75
    # one pass directly above the leaf (the last edge left the same side to move): sound keeps the sign on that edge, and every level above
    # it differs from the reference by exactly that one negation
    sigma = [1, 1, 1, 0]
    s, ls = agents.rules_backup_values("sound", sigma, 0.5)
    r, lr = agents.rules_backup_values("reference", sigma, 0.5)
    assert list(s) == [-0.5, 0.5, -0.5, 0.5] and list(r) == [0.5, -0.5, 0.5, -0.5]
    assert np.array_equal(s, -r) and ls == -lr == 0.5
    # a pass in the middle flips exactly the levels at and above it
    sigma = [1, 0, 1, 1]
    s, _ = agents.rules_backup_values("sound", sigma, 0.5)
    r, _ = agents.rules_backup_values("reference", sigma, 0.5)
    assert list(s[2:]) == list(r[2:]) and list(s[:2]) == list(-r[:2])


def test_terminal_values(agents):
    rng = random.Random(9)
    cases = [(0b111, 0b1), (0b1, 0b111), (0b11, 0b1100), (0, 0), (2**64 - 1, 0), (0, 2**64 - 1)]
    for _ in range(200):
        own = rng.getrandbits(64)
        cases.append((own, rng.getrandbits(64) & ~own))
    for own, opp in cases:
        for mode in MODES:
            assert agents.rules_terminal_value(mode, own, opp) == terminal_value(mode, own, opp), (mode, own, opp)
    assert [agents.rules_terminal_value("sound", *c) for c in cases[:3]] == [1, -1, 0]
    assert [agents.rules_terminal_value("reference", *c) for c in cases[:3]] == [1, -1, 1]


def test_hand_cases_of_the_last_move(agents):
    """the move that ends the game leaves its mover as `own` (sigma = 0); what its edge stores: a win +1 sound / -1 reference, a draw 0 / -1,
    a loss -1 / +1"""
    for (own, opp), sound, ref in (((0b111, 0b1), 1.0, -1.0), ((0b11, 0b1100), 0.0, -1.0), ((0b1, 0b111), -1.0, 1.0)):
        for mode, want in (("sound", sound), ("reference", ref)):
            leaf = float(agents.rules_terminal_value(mode, own, opp))
            vals, last = agents.rules_backup_values(mode, [1, 1, 0], leaf)
            assert vals[-1] == want, (mode, own, opp)
            assert bits(last) == bits(-vals[0])


@pytest.mark.parametrize("K", [1, 4])
def test_sound_search_in_reference_mode_is_wide_search(K):
    cases = [(4, *initial_board(4), 120, 3), (6, *initial_board(6), 60, 5)] + [(6, own, opp, 60, 7) for own, opp in POSITIONS_6]
    for n, own, opp, sims, salt in cases:
        a, b = WideSearch(n, 1.0, K, salt=salt), SoundSearch(n, 1.0, K, salt=salt, mode="reference")
        for chunk in (sims // 3, sims - sims // 3):
            a.simulate(own, opp, chunk)
            b.simulate(own, opp, chunk)
            assert bits(a.last_value) == bits(b.last_value)
        assert len(a.nodes) == len(b.nodes) and (a.steps, a.leaves, a.collisions, a.sims, a.terminals) == (b.steps, b.leaves, b.collisions, b.sims, b.terminals)
        for x, y in zip(a.nodes, b.nodes):
            assert (x.own, x.opp, x.Ns, x.acts, x.N, x.P) == (y.own, y.opp, y.Ns, y.acts, y.N, y.P)
            assert {s: bits(q) for s, q in x.Q.items()} == {s: bits(q) for s, q in y.Q.items()}


def coverage(cases):
    """the restatement's counters over (n, own, opp, sims, salt, K) cases -> (pass backups, finished leaves by value, cases whose root counts
    differ from reference mode)"""
    passes, term, differ = 0, {-1: 0, 0: 0, 1: 0}, 0
    for n, own, opp, sims, salt, K in cases:
        s, r = SoundSearch(n, 1.0, K, salt=salt), SoundSearch(n, 1.0, K, salt=salt, mode="reference")
        s.simulate(own, opp, sims)
        r.simulate(own, opp, sims)
        passes += s.pass_backups
        for k in term:
            term[k] += s.term[k]
        differ += not np.array_equal(s.counts(own, opp)[0], r.counts(own, opp)[0])
    return passes, term, differ


def test_sound_mode_differs_on_the_coverage_set():
    b4 = initial_board(4)
    cases = [(4, *b4, sims, salt, K) for sims in (100, 200) for salt in (3, 11) for K in (1, 4)]
    cases += [(6, own, opp, 60, 7, K) for own, opp in POSITIONS_6 for K in (1, 4)]
    passes, term, differ = coverage(cases)
    assert passes >= 20 and min(term.values()) >= 1 and differ >= 4, (passes, term, differ)


def test_argument_checks_of_the_python_surface(agents):
    from othellozero_amd import _lib, loop, training
    from othellozero_amd.othelo_mcts import OthelloMCTS
    assert _lib.check_value_signs("reference") == 0 and _lib.check_value_signs("sound") == 1
    assert _lib.check_value_signs_pair("sound") == (1, 1) and _lib.check_value_signs_pair(("sound", "reference")) == (1, 0)
    for bad in ("Sound", "", None, 1, True, b"sound", ("sound",)):
        with pytest.raises(ValueError):
            _lib.check_value_signs(bad)
    for bad in (("sound",), ("sound", "reference", "sound"), ("sound", 1), 0):
        with pytest.raises(ValueError):
            _lib.check_value_signs_pair(bad)
    # every entry point refuses before it touches the library (none of these needs a device to fail)
    with pytest.raises(ValueError):
        OthelloMCTS(6, object(), 1.0, value_signs="negamax")
    with pytest.raises(ValueError):
        training.SelfPlayEngine(object(), 6, 4, 10, value_signs="negamax")
    with pytest.raises(ValueError):
        training.selfplay_batch(object(), 6, 4, 10, value_signs="negamax")
    with pytest.raises(ValueError):
        training.execute_episode(6, object(), 1.0, 10, 1, 1.0, value_signs="negamax")
    with pytest.raises(ValueError):
        agents.arena_batch(object(), object(), 6, 4, 10, value_signs=("sound", "negamax"))
    with pytest.raises(ValueError):
        agents.NeuralNetworkOthelloAgent(None, object(), 10, 1.0, value_signs="negamax")
    with pytest.raises(ValueError):
        loop.self_play_match(6, object(), object(), 4, 10, 1.0, value_signs="negamax")
    with pytest.raises(ValueError):
        loop.paired_match(6, object(), object(), 2, 10, 1.0, (4, 1), value_signs="negamax")
    with pytest.raises(ValueError):
        loop.evaluate_against_random_batch(6, object(), 4, 10, 1.0, value_signs="negamax")
    with pytest.raises(ValueError):
        loop.evaluate_against_opponent_batch(6, object(), 4, 10, 1.0, ("minimax", 2), value_signs="negamax")
    with pytest.raises(ValueError):
        agents.rules_backup_values("negamax", [1], 1.0)
    with pytest.raises(ValueError):
        agents.rules_backup_values("sound", [1] * 65, 1.0)
    with pytest.raises(ValueError):
        agents.rules_terminal_value("negamax", 1, 2)


def test_the_library_refuses_what_the_python_surface_lets_through():
    import ctypes as C
    from othellozero_amd import _lib
    lib = _lib.load()
    out, last, v = np.zeros(4), C.c_double(), C.c_int()
    assert lib.oz_search_backup_values(2, 0, 1, 1.0, _lib.p_f64(out), C.byref(last)) == _lib.OZ_ERR_ARG
    assert lib.oz_search_backup_values(1, 0, 65, 1.0, _lib.p_f64(out), C.byref(last)) == _lib.OZ_ERR_ARG
    assert lib.oz_search_backup_values(1, 0, -1, 1.0, _lib.p_f64(out), C.byref(last)) == _lib.OZ_ERR_ARG
    assert lib.oz_search_terminal_value(-1, 1, 2, C.byref(v)) == _lib.OZ_ERR_ARG
    # bits of swap_bits at or above depth are not read
    _lib.check(lib.oz_search_backup_values(1, 0xFFFFFFFFFFFFFFF0 | 0b0101, 4, 1.0, _lib.p_f64(out), C.byref(last)))
    assert list(out) == [1.0, -1.0, -1.0, 1.0] and last.value == -1.0
