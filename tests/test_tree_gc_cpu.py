"""Tree collection without a GPU: the liveness rule's host twin (oz_search_tree_keep) against a restatement in Python, the keyword
validation of the Python surface, and the new symbols of the built library."""
import inspect
import random

import numpy as np
import pytest

from tree_gc_ref import keep_plan, popcount, tree_keep

M64 = (1 << 64) - 1


def random_board(rng, discs=None):
    """(own, opp): disjoint random disc sets; `discs` fixes their number"""
    k = rng.randrange(0, 65) if discs is None else discs
    squares = rng.sample(range(64), k)
    own = opp = 0
    for s in squares:
        if rng.random() < 0.5:
            own |= 1 << s
        else:
            opp |= 1 << s
    return own, opp


def library(root, nodes):
    from othellozero_amd import _lib
    keep, new_index, kept = _lib.search_tree_keep(root[0], root[1], [a for a, _ in nodes], [b for _, b in nodes])
    return [int(x) for x in keep], [int(x) for x in new_index], kept


def check(root, nodes):
    keep, new_index, kept = keep_plan(root, nodes)
    got = library(root, nodes)
    assert got == (keep, new_index, kept), (root, nodes)
    # stable: the kept nodes are numbered 0, 1, 2, ... in the order they stand in
    assert [i for i in new_index if i >= 0] == list(range(kept))
    assert kept == sum(keep)


def test_restatement_is_the_rule_of_the_issue():
    root = (0b0110, 0b1001)
    assert tree_keep(root, root)
    assert not tree_keep(root, (root[1], root[0]))                  # colours swapped: same discs, not the root
    assert not tree_keep(root, (0b0111, 0b1000))                    # D discs
    assert tree_keep(root, (0b10110, 0b1001))                       # D + 1 discs
    assert popcount(M64) == 64


def test_hand_built_cases():
    rng = random.Random(5)
    root = random_board(rng, 20)
    D = 20
    swapped = (root[1], root[0])
    same_d = random_board(rng, D)
    one_more = random_board(rng, D + 1)
    fewer = random_board(rng, D - 3)
    full = random_board(rng, 64)
    check(root, [root])                                             # count = 1: the root itself
    check(root, [swapped])                                          # count = 1: dropped
    check(root, [])                                                 # an empty table
    check(root, [same_d, one_more, root, swapped, fewer, full, one_more, root])
    keep, new_index, kept = library(root, [same_d, one_more, root, swapped, fewer, full])
    assert keep == [0, 1, 1, 0, 0, 1] and new_index == [-1, 0, 1, -1, -1, 2] and kept == 3
    check((0, 0), [(0, 0), (1, 0), (0, 0)])                         # an empty root: everything with a disc stays, and the root
    check(full, [full, root, (full[1], full[0])])                   # a full root: only the root stays


def test_random_tables():
    rng = random.Random(11)
    for _ in range(200):
        d = rng.randrange(4, 61)
        root = random_board(rng, d)
        nodes = []
        for _ in range(rng.randrange(0, 150)):
            r = rng.random()
            if r < 0.1:
                nodes.append(root)
            elif r < 0.2:
                nodes.append((root[1], root[0]))
            else:
                nodes.append(random_board(rng, max(0, min(64, d + rng.randrange(-3, 4)))))
        check(root, nodes)


def test_empty_table_takes_null_arrays():
    import ctypes as C
    from othellozero_amd import _lib
    kept = C.c_int64(-1)
    assert _lib.load().oz_search_tree_keep(1, 2, None, None, 0, None, None, C.byref(kept)) == _lib.OZ_OK
    assert kept.value == 0
    assert _lib.load().oz_search_tree_keep(1, 2, None, None, 3, None, None, C.byref(kept)) == _lib.OZ_ERR_ARG
    assert _lib.load().oz_search_tree_keep(1, 2, None, None, -1, None, None, C.byref(kept)) == _lib.OZ_ERR_ARG


def test_unknown_modes_raise_before_the_library_is_touched(monkeypatch):
    from othellozero_amd import _lib, agents, loop, othelo_mcts, training

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    for bad in ("on", "", None, 1, True, "EVERY", ("every",)):
        with pytest.raises(ValueError):
            _lib.check_tree_gc(bad)
        with pytest.raises(ValueError):
            training.SelfPlayEngine(object(), 6, 4, 8, tree_gc=bad)
        with pytest.raises(ValueError):
            training.selfplay_batch(object(), 6, 4, 8, tree_gc=bad)
        with pytest.raises(ValueError):
            training.execute_episode(6, object(), 1.0, 8, 1.0, 0.9, tree_gc=bad)
        with pytest.raises(ValueError):
            othelo_mcts.OthelloMCTS(6, object(), 1.0, tree_gc=bad)
        with pytest.raises(ValueError):
            agents.arena_batch(object(), object(), 6, 4, 8, tree_gc=bad)
        with pytest.raises(ValueError):
            agents.arena_batch(object(), object(), 6, 4, 8, tree_gc=("every", bad))
        with pytest.raises(ValueError):
            loop.self_play_match(6, object(), object(), 2, 8, 1.0, tree_gc=bad)
        with pytest.raises(ValueError):
            loop.evaluate_against_random_batch(6, object(), 2, 8, 1.0, tree_gc=bad)
    with pytest.raises(ValueError):
        agents.arena_batch(object(), object(), 6, 4, 8, tree_gc=("every", "off", "off"))
    assert [_lib.check_tree_gc(m) for m in ("off", "demand", "every")] == [0, 1, 2]
    assert _lib.check_tree_gc_pair("demand") == (1, 1) and _lib.check_tree_gc_pair(("off", "every")) == (0, 2)
    kw = lambda tree_gc: _lib.search_kw(_lib.check_search_options(tree_gc=tree_gc, pairs=True))
    assert kw("off") == {} and kw(("off", "off")) == {} and kw("every") == {"tree_gc": "every"}


def test_keyword_is_on_every_surface_and_defaults_to_off():
    from othellozero_amd import agents, loop, othelo_mcts, training
    for fn in (training.SelfPlayEngine.__init__, training.selfplay_batch, training.execute_episode, othelo_mcts.OthelloMCTS.__init__,
               agents.arena_batch, agents.NeuralNetworkOthelloAgent.__init__, loop.self_play_match, loop.paired_match,
               loop.evaluate_against_random_batch, loop.evaluate_against_opponent_batch, loop.training):
        assert inspect.signature(fn).parameters["tree_gc"].default == "off", fn
    assert hasattr(training.SelfPlayEngine, "tree_gc_stats") and hasattr(othelo_mcts.OthelloMCTS, "collect")


def test_new_symbols_are_exported_and_the_version_stays():
    from othellozero_amd import _lib
    lib = _lib.load()
    for name in ("oz_search_tree_keep", "oz_mcts_collect", "oz_mcts_tree_gc_stats", "oz_selfplay_set_tree_gc", "oz_selfplay_get_tree_gc",
                 "oz_selfplay_tree_gc_profile", "oz_selfplay_tree_gc_profile_read", "oz_arena_set_tree_gc", "oz_arena_get_tree_gc"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.oz_version() == 230
    assert np.dtype(np.int64).itemsize * 5 == __import__("ctypes").sizeof(_lib.TreeGcStats)
