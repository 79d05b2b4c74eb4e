"""Proofs of the search without a GPU: the restatement tests/proofs_ref.py (ProvenSearch) is sound -- every proof it stores is the exact
value of tests/solve_leaves_ref.py -- and covers what the GPU tests (tests/test_gpu_proofs.py) rely on; the library's host functions
(oz_search_proof_value / _candidates / _backup through agents.rules_proof_*) equal it on every node and path of those searches and on a
hand-written table; and the Python surface refuses what it must before the library is touched."""
import functools

import numpy as np
import pytest

import solve_leaves_ref as SL
from proofs_ref import DRAW_POSITION, ProvenSearch
from value_signs_ref import POSITIONS_6, SoundSearch, random_position, terminal_value
from wide_search_ref import apply_move, initial_board, legal_mask

SALT6 = 7
# the case set of tests/test_gpu_value_signs.py: (n, own, opp, simulations, stub salt)
CASES = [(4, *initial_board(4), sims, salt) for sims in (100, 200) for salt in (3, 11)] + [(6, own, opp, 60, SALT6) for own, opp in POSITIONS_6]
DRAW_CASE = (6, *DRAW_POSITION, 120, SALT6)


@functools.lru_cache(maxsize=None)
def proven(n, own, opp, sims, salt, K, solve=0, log=False):
    """the restatement's search of one case, computed once and shared (read only)"""
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    s = ProvenSearch(n, 1.0, K, salt=salt, evaluator=ev, solve=solve)
    if log:
        s.log = []
    s.simulate(own, opp, sims)
    return s


@functools.lru_cache(maxsize=None)
def sound(n, own, opp, sims, salt, K, solve=0):
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    s = SoundSearch(n, 1.0, K, salt=salt, evaluator=ev)
    s.simulate(own, opp, sims)
    return s


def exact_edge(own, opp, n, sq):
    """the exact value of the move sq for the side to move at (own, opp)"""
    o2, p2 = apply_move(own, opp, n, sq)
    if legal_mask(p2, o2, n) == 0 and legal_mask(o2, p2, n) == 0:
        return terminal_value("sound", o2, p2)
    return -SL.exact_sign(p2, o2, n)


def check_sound(s, n):
    """every stored proof against the exact value -> the number of proofs checked"""
    checked = 0
    for i, nd in enumerate(s.nodes):
        for sq, e in s.edge[i].items():
            assert sq in nd.acts and e == exact_edge(nd.own, nd.opp, n, sq), (i, sq, e)
            checked += 1
        if s.own[i] is not None:
            assert s.own[i] == SL.exact_sign(nd.own, nd.opp, n), i
            checked += 1
        v = s.val(i)
        if v is not None:
            assert v == SL.exact_sign(nd.own, nd.opp, n), (i, v)
            checked += 1
    assert not s.corrupt
    return checked


def test_the_draw_position_is_random_position_6_4_10():
    assert random_position(6, 4, 10) == DRAW_POSITION


def test_every_proof_is_the_exact_value_and_the_set_covers_the_rule():
    checked = 0
    cover = dict(edge_stops=0, node_stops=0, root_win=0, root_loss=0, draw_edges=0, own_nodes=0, counts_differ=0)
    for K in (1, 4):
        for solve in (0, 4):
            for case in CASES:
                n, own, opp = case[:3]
                s = proven(*case, K, solve)
                checked += check_sound(s, n)
                rv = s.root_proof(own, opp)[0]
                print(n, case[3], case[4], "K", K, "E", solve, "nodes", len(s.nodes), "stops", s.edge_stops, s.node_stops, "root", rv, "first at",
                      s.first_root_proof, "by value", s.proofs_by_value, "own", s.own_nodes)
                cover["edge_stops"] += s.edge_stops
                cover["node_stops"] += s.node_stops
                cover["root_win"] += rv == 1
                cover["root_loss"] += rv == -1
                cover["draw_edges"] += s.proofs_by_value[0]
                cover["own_nodes"] += s.own_nodes
                cover["counts_differ"] += not np.array_equal(s.counts(own, opp)[0], sound(*case, K, solve).counts(own, opp)[0])
                assert s.own_nodes == 0 or solve
                assert (rv is None) == (s.first_root_proof is None)
    print("proofs checked", checked, cover)
    assert checked >= 100
    assert all(v >= 1 for v in cover.values()), cover


@pytest.mark.parametrize("K,first", [(1, 35), (4, 42)])
def test_a_root_proven_a_draw(K, first):
    s = proven(*DRAW_CASE, K)
    check_sound(s, 6)
    assert s.root_proof(*DRAW_POSITION)[0] == 0
    assert s.first_root_proof == first, s.first_root_proof
    assert SL.exact_sign(*DRAW_POSITION, 6) == 0


def test_once_the_root_is_proven_descents_end_after_one_level():
    """the root never stops, its candidates are the edges that prove it, and each of them is known: depth 1, nothing expanded"""
    s = ProvenSearch(6, 1.0, 1, salt=SALT6)
    s.simulate(*DRAW_POSITION, 120)
    nodes, leaves = len(s.nodes), s.leaves
    before = s.counts(*DRAW_POSITION)[0].copy()
    stops = s.edge_stops
    s.simulate(*DRAW_POSITION, 10)
    assert (len(s.nodes), s.leaves, s.edge_stops) == (nodes, leaves, stops + 10)
    after = s.counts(*DRAW_POSITION)[0]
    val, edge = s.root_proof(*DRAW_POSITION)
    assert int((after - before).sum()) == 10 and all(edge.get(sq) == val for sq in np.nonzero(after - before)[0])


# ------------------------------------------------------------------ the host functions
def _edges64(e):
    return [e.get(s) for s in range(64)]


def test_host_functions_equal_the_restatement_on_every_node_and_path():
    from othellozero_amd.agents import rules_proof_backup, rules_proof_candidates, rules_proof_value
    nodes = backups = 0
    for K in (1, 4):
        for case, solve in [(c, e) for c in CASES[2:] + [DRAW_CASE] for e in (0, 4)]:
            s = proven(*case, K, solve, True)
            for ev in s.log:
                if ev[0] == "node":
                    _, lg, edge, own, val, cands = ev
                    assert rules_proof_candidates(lg, _edges64(edge), val) == (sum(1 << c for c in cands), False)
                    if val is not None or own is None:                 # (the log keeps val at the root only: below it the node was unknown)
                        assert rules_proof_value(lg, _edges64(edge), own) == val
                    nodes += 1
                else:
                    _, before, leaf, after, marked, fresh, root = ev
                    got = rules_proof_backup([dict(lv, edge=_edges64(lv["edge"])) for lv in before], leaf)
                    assert got == ([_edges64(e) for e in after], marked, fresh, root, False), (case, K, solve)
                    backups += 1
            for i, nd in enumerate(s.nodes):                           # ... and val(S) of every node as the search left it
                assert rules_proof_value(sum(1 << a for a in nd.acts), _edges64(s.edge[i]), s.own[i]) == s.val(i)
    print("nodes", nodes, "backups", backups)
    assert nodes >= 1000 and backups >= 100


def test_host_functions_on_the_small_cases():
    from othellozero_amd.agents import rules_proof_backup, rules_proof_candidates, rules_proof_value
    legal = 0b1011                                                      # squares 0, 1, 3

    def E(**kw):
        e = [None] * 64
        for k, v in kw.items():
            e[int(k[1:])] = v
        return e
    # val(S)
    assert rules_proof_value(legal, E()) is None
    assert rules_proof_value(legal, E(s0=-1, s1=0)) is None             # one edge unknown, none wins
    assert rules_proof_value(legal, E(s0=-1, s3=1)) == 1                # a win beats everything, known or not
    assert rules_proof_value(legal, E(s0=-1, s1=0, s3=-1)) == 0         # all known: the maximum
    assert rules_proof_value(legal, E(s0=-1, s1=-1, s3=-1)) == -1
    assert rules_proof_value(legal, E(s0=-1, s1=-1, s3=-1), own_value=0) == 0     # an own value wins
    assert rules_proof_value(legal, E(s3=1), own_value=-1) == -1
    assert rules_proof_value(legal, E(s2=1)) is None                    # a proof off the legal set is not read
    assert rules_proof_value(0, E()) is None
    # candidates
    assert rules_proof_candidates(legal, E(), None) == (legal, False)
    assert rules_proof_candidates(legal, E(s0=-1), None) == (0b1010, False)         # never a proven loss while something else is left
    assert rules_proof_candidates(legal, E(s0=-1, s1=0, s3=1), 1) == (0b1000, False)
    assert rules_proof_candidates(legal, E(s0=-1, s1=0, s3=0), 0) == (0b1010, False)
    assert rules_proof_candidates(legal, E(s0=-1, s1=-1, s3=-1), -1) == (legal, False)
    assert rules_proof_candidates(legal, E(s0=-1, s1=0), 1) == (0b1010, False)      # the root falls back where no edge matches its (own) value
    assert rules_proof_candidates(legal, E(s0=-1, s1=-1, s3=-1), 1) == (legal, True)
    # backup: a win goes up as the parent's loss and stops where a sibling is unknown
    lv = [dict(legal=0b11, edge=E(), own_value=None, square=0, sigma=1), dict(legal=0b101, edge=E(), own_value=None, square=2, sigma=1)]
    edges, marked, fresh, root, conflict = rules_proof_backup(lv, -1)
    assert (edges[1][2], edges[0][0], marked, fresh, root, conflict) == (1, -1, 2, 2, False, False)
    # ... all siblings known: the maximum travels on, and the root's value becomes known
    lv[0]["edge"] = E(s1=-1)
    edges, marked, fresh, root, conflict = rules_proof_backup(lv, -1)
    assert (edges[0][0], edges[0][1], marked, fresh, root) == (-1, -1, 2, 2, True)
    # ... a pass (sigma 0) keeps the sign; an unknown node stops the loop after one level
    lv = [dict(legal=0b11, edge=E(), own_value=None, square=0, sigma=1), dict(legal=0b101, edge=E(), own_value=None, square=2, sigma=0)]
    edges, marked, fresh, root, conflict = rules_proof_backup(lv, 0)
    assert (edges[1][2], edges[0][0], marked, fresh) == (0, None, 1, 1)
    # ... a known edge that differs is a conflict and stays
    lv = [dict(legal=0b1, edge=E(s0=1), own_value=None, square=0, sigma=1)]
    edges, marked, fresh, root, conflict = rules_proof_backup(lv, 1)
    assert (edges[0][0], fresh, conflict) == (1, 0, True)
    assert rules_proof_backup([], 1) == ([], 0, 0, False, False)


def test_host_functions_refuse_bad_arguments():
    import ctypes as C
    from othellozero_amd import _lib
    lib = _lib.load()
    v, m, bad = C.c_int(), C.c_uint64(), C.c_int()
    assert lib.oz_search_proof_value(1, 0, 0, 2, C.byref(v)) == _lib.OZ_ERR_ARG
    assert lib.oz_search_proof_value(1, 0, 0, 0, None) == _lib.OZ_ERR_ARG
    assert lib.oz_search_proof_candidates(1, 0, 0, 5, C.byref(m), C.byref(bad)) == _lib.OZ_ERR_ARG
    one = dict(sigma=np.zeros(1, np.uint8), sq=np.array([3], np.int32), legal=np.array([1], np.uint64), lo=np.zeros(1, np.uint64),
               hi=np.zeros(1, np.uint64), own=np.full(1, _lib.PROOF_UNKNOWN, np.int8), out=np.zeros(3, np.int32))

    def call(depth, leaf):
        return lib.oz_search_proof_backup(_lib.p_u8(one["sigma"]), _lib.p_i32(one["sq"]), depth, leaf, _lib.p_u64(one["legal"]), _lib.p_u64(one["lo"]),
                                          _lib.p_u64(one["hi"]), _lib.p_i8(one["own"]), _lib.p_i32(one["out"]), C.byref(bad))
    assert call(1, 1) == _lib.OZ_ERR_ARG                                # square 3 is not legal
    assert call(65, 1) == _lib.OZ_ERR_ARG and call(-1, 1) == _lib.OZ_ERR_ARG and call(0, 2) == _lib.OZ_ERR_ARG
    assert _lib.PROOF_UNKNOWN == -128


# ------------------------------------------------------------------ the Python surface: refusals that need no GPU
def test_python_surface_refuses_before_the_library_is_touched(monkeypatch):
    from othellozero_amd import _lib, agents, loop, training
    from othellozero_amd.othelo_mcts import OthelloMCTS

    def no_library(*a, **kw):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    monkeypatch.setattr(_lib, "load", no_library)

    class Net:
        network_type = None
        _h = 1
    net = Net()
    with pytest.raises(ValueError, match="sound"):
        OthelloMCTS(6, net, 1.0, proofs=True)
    with pytest.raises(ValueError, match="sound"):
        OthelloMCTS(6, net, 1.0, value_signs="reference", proofs=True)
    with pytest.raises(ValueError, match="True or False"):
        OthelloMCTS(6, net, 1.0, value_signs="sound", proofs="yes")
    with pytest.raises(ValueError, match="Gumbel"):
        OthelloMCTS(6, net, 1.0, value_signs="sound", proofs=True, gumbel=True)
    with pytest.raises(ValueError, match="forced"):
        OthelloMCTS(6, net, 1.0, value_signs="sound", proofs=True, forced_playouts=2.0)
    with pytest.raises(ValueError, match="sound"):
        training.SelfPlayEngine(net, 6, 8, 12, proofs=True)
    with pytest.raises(ValueError, match="Gumbel"):
        training.SelfPlayEngine(net, 6, 8, 12, value_signs="sound", proofs=True, gumbel=True)
    with pytest.raises(ValueError, match="forced"):
        training.SelfPlayEngine(net, 6, 8, 12, value_signs="sound", proofs=True, root_noise=(0.5, 0.25), forced_playouts=2.0)
    with pytest.raises(ValueError, match="sound"):
        training.selfplay_batch(net, 6, 8, 12, proofs=True)
    with pytest.raises(ValueError, match="sound"):
        training.execute_episode(6, net, 1.0, 12, 1.0, 0.9, proofs=True)
    with pytest.raises(ValueError, match="sound"):
        agents.arena_batch(net, net, 6, 8, 12, proofs=True)
    with pytest.raises(ValueError, match=r"proofs\[white\]"):
        agents.arena_batch(net, net, 6, 8, 12, value_signs=("sound", "reference"), proofs=(True, True))
    with pytest.raises(ValueError, match="black, white"):
        agents.arena_batch(net, net, 6, 8, 12, value_signs=("sound", "reference"), proofs=True)
    with pytest.raises(ValueError, match="black, white"):
        agents.arena_batch(net, net, 6, 8, 12, value_signs="sound", proofs=(True, False, True))
    with pytest.raises(ValueError, match="sound"):
        agents.NeuralNetworkOthelloAgent(None, net, 12, 1.0, proofs=True)
    for fn in (loop.self_play_match, loop.paired_match):
        with pytest.raises(ValueError, match="sound"):
            fn(6, net, net, 4, 12, 1.0, **({"openings": (2, 1)} if fn is loop.paired_match else {}), proofs=True)
    with pytest.raises(ValueError, match="sound"):
        loop.evaluate_against_random_batch(6, net, 4, 12, 1.0, proofs=True)
    with pytest.raises(ValueError, match="sound"):
        loop.evaluate_against_opponent_batch(6, net, 4, 12, 1.0, ("minimax", 1), proofs=True)
    assert _lib.check_proofs_pair((True, False), ("sound", "reference")) == (True, False)
    assert _lib.check_proofs_pair(False, ("sound", "reference")) == (False, False)
    kw = lambda proofs: _lib.search_kw(_lib.check_search_options(value_signs="sound", proofs=proofs, pairs=True))
    assert "proofs" not in kw(False) and "proofs" not in kw((False, False)) and kw((True, False))["proofs"] == (True, False)
