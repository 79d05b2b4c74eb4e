"""The selection option without a GPU: the library's host twins (oz_search_select_c / oz_search_select_scores through agents.rules_select_*)
against the plain-Python restatement in tests/selection_ref.py, bit for bit; the restatement's classes with the option off against their
parents; the argument checks and the refusals of the Python surface that need no device; and the coverage of the case set the GPU tests
(tests/test_gpu_selection.py) run."""
import ctypes as C
import functools
import math
import random
import struct

import numpy as np
import pytest

import selection_ref as R
import solve_leaves_ref as SL
from proofs_ref import ProvenSearch
from selection_ref import CASES, CLAMP, SALT6, SETTINGS, SelectProvenSearch, SelectSearch, select_scores
from value_signs_ref import POSITIONS_6, SoundSearch
from wide_search_ref import initial_board

EVERY = dict(SETTINGS, clamp=CLAMP, growth_az=dict(cpuct_growth=(19652, 1.0)), root0=dict(fpu=(0.2, 0.0), prior_first=True))


@pytest.fixture(scope="module")
def agents():
    from othellozero_amd import agents
    return agents


def bits(x):
    return struct.pack("<d", float(x))


def same_node(agents, N, Q, P, legal, n, vhat, level, c, sel, where):
    got = agents.rules_select_scores(N, Q, P, legal, n, vhat, level, c, sel)
    want = select_scores(N, Q, P, legal, n, vhat, level, c, sel, R.library_log)
    assert [bits(x) for x in got["U"]] == [bits(x) for x in want["U"]], where
    for k in ("F", "V", "c_S"):
        assert bits(got[k]) == bits(want[k]), (where, k, got[k], want[k])
    assert got["pick"] == want["pick"], where
    return want


def random_node(rng, kind):
    """(N, Q, P, legal, n, vhat) of one node; kind picks the edge case"""
    legal = rng.getrandbits(64) | (1 << rng.randrange(64))
    if kind == "one_move":
        legal = 1 << rng.randrange(64)
    acts = [s for s in range(64) if (legal >> s) & 1]
    N = [0] * 64
    for s in acts:
        N[s] = rng.choice([0, 0, 0, 1, 2, 5, 17, 400]) if kind != "all_visited" else rng.randint(1, 50)
    if kind == "fresh":
        N = [0] * 64
    Q = [rng.uniform(-1.0, 1.0) if N[s] else 0.0 for s in range(64)]
    w = [rng.random() if (legal >> s) & 1 else 0.0 for s in range(64)]
    tot = sum(w)
    P = [x / tot for x in w]
    if kind == "zero_prior_visited":
        P = [0.0 if N[s] else P[s] for s in range(64)]
    n = sum(N) + (rng.randint(0, 3) if kind != "fresh" else 0)        # (in-flight descents that ended at the node count in n only)
    return N, Q, P, legal, n, rng.uniform(-1.0, 1.0)


def test_tree_sum_is_the_balanced_binary_tree():
    rng = random.Random(3)
    x = [rng.uniform(-1.0, 1.0) * 10.0 ** rng.randint(-8, 8) for _ in range(64)]
    y = list(x)
    for _ in range(6):
        y = [y[2 * i] + y[2 * i + 1] for i in range(len(y) // 2)]
    assert bits(R.tree_sum(x)) == bits(y[0])
    # the xor butterfly of the kernels: every lane ends with the tree's bits
    s = list(x)
    for r in range(6):
        s = [s[i] + s[i ^ (1 << r)] for i in range(64)]
    assert all(bits(v) == bits(y[0]) for v in s)


@pytest.mark.parametrize("kind", ["plain", "fresh", "one_move", "all_visited", "zero_prior_visited"])
def test_host_twin_vs_restatement_on_random_nodes(agents, kind):
    rng = random.Random(sum(map(ord, kind)))
    clamped = 0
    for t in range(150):
        N, Q, P, legal, n, vhat = random_node(rng, kind)
        for name, sel in EVERY.items():
            for level in (0, 1, 5):
                clamped += same_node(agents, N, Q, P, legal, n, vhat, level, 1.0 + 0.5 * (t % 3), sel, (kind, t, name, level))["clamped"]
    assert clamped >= 1 or kind != "plain"                     # (a fresh node's F is vhat itself: never clamped)


def test_host_twin_where_the_prior_sum_rounds_above_one(agents):
    """every edge visited and tree_sum(P) > 1.0: sqrt(SP) > 1, nothing special-cased"""
    rng = random.Random(11)
    found = 0
    for t in range(4000):
        legal = rng.getrandbits(64) | 1
        w = [rng.random() if (legal >> s) & 1 else 0.0 for s in range(64)]
        tot = math.fsum(w)
        P = [x / tot for x in w]
        if not R.tree_sum(P) > 1.0:
            continue
        found += 1
        N = [rng.randint(1, 9) if (legal >> s) & 1 else 0 for s in range(64)]
        Q = [rng.uniform(-1.0, 1.0) if N[s] else 0.0 for s in range(64)]
        for name, sel in EVERY.items():
            same_node(agents, N, Q, P, legal, sum(N), 0.25, 1, 1.0, sel, (t, name))
        if found >= 20:
            break
    assert found >= 20


def test_select_c_against_math_log(agents):
    """oz_log_cr is good to 2^-85 and libm's log to under one ulp: the two logarithms differ by at most one ulp of L; the product and the
    sum add one rounding each"""
    rng = random.Random(7)
    for t in range(3000):
        c = rng.choice([0.0, 1.0, 1.25, 4.0, rng.uniform(0.0, 5.0)])
        base = rng.choice([20.0, 19652.0, 38739.0, rng.uniform(0.5, 1e5)])
        factor = rng.choice([0.0, 1.0, 2.0, 3.9, rng.uniform(0.0, 5.0)])
        n = rng.choice([0, 1, 2, 100, 800, rng.randint(0, 10 ** 6)])
        L = R.MATH_LOG(n, base)
        got = agents.rules_select_c(c, base, factor, n)
        want = c + factor * L
        assert abs(got - want) <= 2.0 * 2.0 ** -52 * (abs(c) + factor * abs(L)), (c, base, factor, n, got, want)
    assert bits(agents.rules_select_c(1.5, 20.0, 0.0, 7)) == bits(1.5)


# ------------------------------------------------------------------ the option off is the parent class
@functools.lru_cache(maxsize=None)
def searched(cls, n, own, opp, sims, salt, K, mode, solve, setting):
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    sel = None if setting is None else EVERY[setting] if setting in EVERY else OFF[setting]
    if cls == "sound":
        s = SoundSearch(n, 1.0, K, salt=salt, evaluator=ev, mode=mode)
    elif cls == "select":
        s = SelectSearch(n, 1.0, K, salt=salt, evaluator=ev, mode=mode, selection=sel, growth_log=R.library_log)
    elif cls == "proven":
        s = ProvenSearch(n, 1.0, K, salt=salt, evaluator=ev, solve=solve)
    else:
        s = SelectProvenSearch(n, 1.0, K, salt=salt, evaluator=ev, solve=solve, selection=sel, growth_log=R.library_log)
    s.simulate(own, opp, sims)
    return s


OFF = {"none_parts": dict(fpu=None, cpuct_growth=None, prior_first=False), "empty": {}}


def same_search(a, b, where):
    assert len(a.nodes) == len(b.nodes), where
    for x, y in zip(a.nodes, b.nodes):
        assert (x.own, x.opp, x.Ns, x.acts) == (y.own, y.opp, y.Ns, y.acts), where
        assert x.N == y.N and x.P == y.P and [bits(x.Q[s]) for s in x.acts] == [bits(y.Q[s]) for s in y.acts], where
    assert bits(a.last_value) == bits(b.last_value), where


@pytest.mark.parametrize("K", [1, 4])
def test_option_off_is_the_parent_restatement(K):
    for case in CASES:
        for mode in ("reference", "sound"):
            for off in (None, "none_parts", "empty"):
                s = searched("select", *case, K, mode, 0, off)
                assert s.selection is None
                same_search(s, searched("sound", *case, K, mode, 0, None), (case, mode, off))
                assert len(s.vhat) == len(s.nodes)
    for case in CASES[4:]:
        p = searched("select_proven", *case, K, "sound", 6, None)
        q = searched("proven", *case, K, "sound", 6, None)
        same_search(p, q, case)
        assert p.edge == q.edge and p.own == q.own and p.stats() == q.stats()


# ------------------------------------------------------------------ coverage of the case set
def test_coverage_of_the_case_set():
    """every counter of the restatement is at least 1 over the set, and each part switched on alone changes the root counts of at least one
    case"""
    total = dict(fpu_clamped=0, prior_first_moved=0, inflight_unvisited=0, growth_changed=0)
    differ = dict(fpu=0, growth=0, prior_first=0)
    for K in (1, 4):
        for case in CASES:
            off = searched("sound", *case, K, "sound", 0, None)
            for name in list(SETTINGS) + ["clamp"]:
                s = searched("select", *case, K, "sound", 0, name)
                for k in total:
                    total[k] += getattr(s, k)
                if name in differ:
                    differ[name] += not np.array_equal(s.counts(case[1], case[2])[0], off.counts(case[1], case[2])[0])
    print(total, differ)
    assert min(total.values()) >= 1, total
    assert min(differ.values()) >= 1, differ
    # the proofs-based class meets proven edges under the option, at unvisited edges too
    stops = sum(searched("select_proven", *case, K, "sound", 6, "all").edge_stops for case in CASES[4:] for K in (1, 4))
    assert stops >= 1


def test_restated_vhat_is_the_evaluators_value():
    import oracle
    n, own, opp, sims, salt = CASES[4]
    s = searched("select", n, own, opp, sims, salt, 1, "sound", 0, "all")
    assert s.vhat == [float(oracle.stub_predict(nd.own, nd.opp, n, salt, 0)[1]) for nd in s.nodes]


# ------------------------------------------------------------------ the Python surface
def test_check_selection_arguments():
    from othellozero_amd import _lib
    ck = _lib.check_selection
    assert ck(None) == (0, 0.0, 0.0, 0.0, 0.0)
    assert ck({}) == ck(dict(fpu=None, cpuct_growth=None, prior_first=False)) == (0, 0.0, 0.0, 0.0, 0.0)
    assert ck(dict(fpu=(0.2, 0.1))) == (_lib.SELECT_FPU, 0.2, 0.1, 0.0, 0.0)
    assert ck(dict(cpuct_growth=(19652, 1))) == (_lib.SELECT_GROWTH, 0.0, 0.0, 19652.0, 1.0)
    assert ck(dict(prior_first=True)) == (_lib.SELECT_PRIOR_FIRST, 0.0, 0.0, 0.0, 0.0)
    assert ck(SETTINGS["all"]) == (7, 0.2, 0.1, 20.0, 2.0)
    assert ck(dict(fpu=(0.0, 4.0), cpuct_growth=(1e-9, 0.0)))[0] == 3
    assert _lib.selection_dict(ck(SETTINGS["all"])) == dict(fpu=(0.2, 0.1), cpuct_growth=(20.0, 2.0), prior_first=True)
    kw = lambda selection: _lib.search_kw(_lib.check_search_options(selection=selection, pairs=True))
    assert _lib.selection_dict(ck(None)) is None and kw(None) == {} and kw({}) == {}
    assert kw(SETTINGS["fpu"]) == {"selection": SETTINGS["fpu"]}
    assert kw((None, SETTINGS["fpu"])) == {"selection": (None, SETTINGS["fpu"])} and kw((None, None)) == {}
    nan, inf = float("nan"), float("inf")
    for bad in ("fpu", 1, (0.2, 0.1), dict(fpu=0.2), dict(fpu=(0.2,)), dict(fpu=(0.2, 0.1, 0.0)), dict(fpu=(-0.1, 0.1)), dict(fpu=(0.2, 4.5)),
                dict(fpu=(nan, 0.1)), dict(fpu=(0.2, nan)), dict(fpu=("a", 0.1)), dict(fpu=(True, 0.1)), dict(cpuct_growth=(0.0, 1.0)),
                dict(cpuct_growth=(-5, 1.0)), dict(cpuct_growth=(20, -1.0)), dict(cpuct_growth=(inf, 1.0)), dict(cpuct_growth=(20, inf)),
                dict(cpuct_growth=(nan, 1.0)), dict(cpuct_growth=(20, nan)), dict(cpuct_growth=20), dict(prior_first=1), dict(prior_first="yes"),
                dict(fpu_reduction=0.2), dict(fpu=(0.2, 0.1), extra=1)):
        with pytest.raises(ValueError):
            ck(bad)
    assert _lib.check_selection_pair(SETTINGS["fpu"]) == (ck(SETTINGS["fpu"]),) * 2
    assert _lib.check_selection_pair((None, SETTINGS["growth"])) == (ck(None), ck(SETTINGS["growth"]))
    with pytest.raises(ValueError):
        _lib.check_selection_pair((None, None, None))
    with pytest.raises(ValueError):
        _lib.check_selection_pair((None, dict(fpu=(9, 9))))


def test_host_side_validation_of_the_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    out = C.c_double()
    nan, inf = float("nan"), float("inf")
    for base, factor in ((0.0, 1.0), (-1.0, 1.0), (nan, 1.0), (inf, 1.0), (20.0, -0.5), (20.0, nan), (20.0, inf)):
        assert lib.oz_search_select_c(1.0, base, factor, 3, C.byref(out)) == _lib.OZ_ERR_ARG, (base, factor)
    assert lib.oz_search_select_c(1.0, 20.0, 1.0, -1, C.byref(out)) == _lib.OZ_ERR_ARG
    assert lib.oz_search_select_c(1.0, 20.0, 1.0, 3, None) == _lib.OZ_ERR_ARG
    N, Q, P, U = np.zeros(64, np.int32), np.zeros(64), np.full(64, 1.0 / 64), np.zeros(64)

    def scores(flags, f, fr, b, k, legal=0xFF, Ns=0, level=0):
        return lib.oz_search_select_scores(_lib.p_i32(N), _lib.p_f64(Q), _lib.p_f64(P), legal, Ns, 0.0, level, 1.0, flags, f, fr, b, k, _lib.p_f64(U),
                                           None, None, None, None)
    assert scores(7, 0.2, 0.1, 20.0, 2.0) == _lib.OZ_OK
    assert scores(0, nan, nan, nan, nan) == _lib.OZ_OK                         # a part that is off reads no parameter
    for bad in ((8, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (1, -0.1, 0, 0, 0), (1, 0, 4.5, 0, 0), (1, nan, 0, 0, 0), (1, 0, nan, 0, 0), (2, 0, 0, 0.0, 1.0),
                (2, 0, 0, 20.0, -1.0), (2, 0, 0, nan, 1.0), (2, 0, 0, 20.0, nan), (2, 0, 0, inf, 1.0)):
        assert scores(*bad) == _lib.OZ_ERR_ARG, bad
    assert scores(1, 0.2, 0.1, 0, 0, Ns=-1) == _lib.OZ_ERR_ARG and scores(1, 0.2, 0.1, 0, 0, level=-1) == _lib.OZ_ERR_ARG
    # the setters check their handle first, and say so
    for fn in (lib.oz_mcts_set_selection, lib.oz_selfplay_set_selection):
        assert fn(None, 1, 0.2, 0.1, 0.0, 0.0) == _lib.OZ_ERR_ARG
    assert lib.oz_arena_set_selection(None, 1, 1, 0.2, 0.1, 0.0, 0.0) == _lib.OZ_ERR_ARG
    # no legal square: no pick
    pick = C.c_int32(5)
    _lib.check(lib.oz_search_select_scores(_lib.p_i32(N), _lib.p_f64(Q), _lib.p_f64(P), 0, 0, 0.0, 0, 1.0, 7, 0.2, 0.1, 20.0, 2.0, _lib.p_f64(U), None, None,
                                           None, C.byref(pick)))
    assert pick.value == -1 and np.isneginf(U).all()


def test_refusals_that_need_no_device():
    """the Gumbel search and forced playouts beside the option: ValueError before the library is touched, whichever keyword comes first"""
    from othellozero_amd import _lib, loop
    from othellozero_amd.agents import NeuralNetworkOthelloAgent, arena_batch
    from othellozero_amd.othelo_mcts import OthelloMCTS
    from othellozero_amd.training import SelfPlayEngine, execute_episode, selfplay_batch
    sel = SETTINGS["fpu"]
    for kw in (dict(gumbel=True), dict(gumbel=(4, 50.0, 1.0)), dict(forced_playouts=2.0)):
        with pytest.raises(ValueError, match="selection"):
            _lib.check_selection(sel, **kw)
        with pytest.raises(ValueError, match="selection"):
            OthelloMCTS(6, None, 1.0, selection=sel, **kw)
        with pytest.raises(ValueError, match="selection"):
            SelfPlayEngine(None, 6, 8, 16, selection=sel, root_noise=(0.5, 0.25), **kw)
        with pytest.raises(ValueError, match="selection"):
            selfplay_batch(None, 6, 8, 16, selection=sel, root_noise=(0.5, 0.25), **kw)
        with pytest.raises(ValueError, match="selection"):
            execute_episode(6, None, 1.0, 16, 1.0, 0.9, selection=sel, root_noise=(0.5, 0.25), **kw)
        assert _lib.check_selection(None, **kw) == _lib.check_selection({}, **kw) == (0, 0.0, 0.0, 0.0, 0.0)       # off beside them is fine
    bad = dict(fpu=(5.0, 0.1))
    for call in (lambda: OthelloMCTS(6, None, 1.0, selection=bad), lambda: SelfPlayEngine(None, 6, 8, 16, selection=bad),
                 lambda: selfplay_batch(None, 6, 8, 16, selection=bad), lambda: execute_episode(6, None, 1.0, 16, 1.0, 0.9, selection=bad),
                 lambda: arena_batch(None, None, 6, 8, 16, selection=bad), lambda: arena_batch(None, None, 6, 8, 16, selection=(None, bad)),
                 lambda: NeuralNetworkOthelloAgent(None, None, 16, 1.0, selection=bad),
                 lambda: loop.self_play_match(6, None, None, 8, 16, 1.0, selection=bad), lambda: loop.paired_match(6, None, None, 4, 16, 1.0, (4, 1), selection=bad),
                 lambda: loop.evaluate_against_random_batch(6, None, 8, 16, 1.0, selection=bad),
                 lambda: loop.evaluate_against_opponent_batch(6, None, 8, 16, 1.0, ("minimax", 2), selection=bad)):
        with pytest.raises(ValueError, match="selection"):
            call()


def test_nep50_restatement_with_the_option_off_is_the_oracle():
    """Nep50SelectSearch restates the float32 regime of the Q update for the GPU test in that regime: with the option off and the reference
    signs it must be the C oracle in OZ_QMODE_NEP50, tables and Q type tags"""
    import oracle
    for n, sims, salt in ((4, 200, 3), (4, 100, 11), (6, 150, 5)):
        own, opp = initial_board(n)
        a = oracle.Mcts(n, 1.0, oracle.QMODE_NEP50, salt=salt)
        for _ in range(sims):
            a.simulate(own, opp, 1)
        b = R.Nep50SelectSearch(n, 1.0, salt=salt, mode="reference")
        b.simulate(own, opp, sims)
        dump = a.dump()
        assert len(dump) == len(b.nodes)
        tagged = 0
        for i, (d, nd) in enumerate(zip(dump, b.nodes)):
            assert (d["k0"], d["k1"], d["Ns"]) == (nd.own, nd.opp, nd.Ns), (n, salt, i)
            for s in nd.acts:
                assert int(d["N"][s]) == nd.N[s] and bits(d["Q"][s]) == bits(nd.Q[s]) and bits(d["P"][s]) == bits(nd.P[s]), (n, salt, i, s)
                assert bool(d["qtag"][s]) == b.q32[i].get(s, False), (n, salt, i, s)
                tagged += bool(d["qtag"][s])
        assert tagged > 0
