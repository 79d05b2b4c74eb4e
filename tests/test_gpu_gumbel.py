"""The Gumbel search on the GPU (pytest -m gpu), through the C ABI: the bare search with host-supplied and device-drawn draws against the
hand-driven restatement in tests/gumbel_ref.py (root rows after every simulation, whole tables bit for bit), the value kept in the node
header, tree reuse across moves, the improved policy rows (2e-7: one float32 rounding of a value <= 1 is 6e-8, the float64 differences of
device and host libm are below 1e-15), off-is-off, the host-evaluator split and the refusals.  A decision whose best and second-best scores
are closer than 1e-9 could fall either way between device and host libm: the restatement reports its smallest gap and the tests check that
the searches they drive meet none."""
import ctypes as C

import numpy as np
import pytest

import gumbel_ref as R
import oracle
from test_gpu_wide_search import Search, _golden_roots
from wide_search_ref import WideSearch, assert_same_tables, initial_board, legal_mask, next_state, popcount

pytestmark = pytest.mark.gpu

SALT, SEED = 13, 41
M, C_VISIT, C_SCALE, BUDGET = 4, 50.0, 1.0, 16
NEAR_TIE = 1e-9


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def ulps(a, b):
    ia, ib = (np.asarray(x, np.float64).view(np.int64).astype(object) for x in (a, b))
    f = np.vectorize(lambda v: v if v >= 0 else -(v & 0x7FFFFFFFFFFFFFFF), otypes=[object])
    return np.abs(f(ia) - f(ib)).astype(np.float64)


def _set(oz, s, g, armed=None, m=M, c_visit=C_VISIT, c_scale=C_SCALE, budget=BUDGET):
    gp = None if g is None else oz.p_f64(np.ascontiguousarray(g, np.float64))
    ap = None if armed is None else oz.p_u8(np.array(armed, np.uint8))
    return s.lib.oz_mcts_set_gumbel(s.h, m, float(c_visit), float(c_scale), budget, gp, ap)


def _sample(oz, s, seed, ids, plies, m=M, c_visit=C_VISIT, c_scale=C_SCALE, budget=BUDGET):
    return s.lib.oz_mcts_sample_gumbel(s.h, m, float(c_visit), float(c_scale), budget, int(seed), oz.p_u64(np.array(ids, np.uint64)),
                                       oz.p_i32(np.array(plies, np.int32)))


def _get(oz, s):
    g, armed, n0 = np.zeros((s.G, 64), np.float64), np.zeros(s.G, np.uint8), np.zeros((s.G, 64), np.int32)
    m, budget, cv, cs = C.c_int32(-1), C.c_int32(-1), C.c_double(-1), C.c_double(-1)
    oz.check(s.lib.oz_mcts_get_gumbel(s.h, oz.p_f64(g), oz.p_u8(armed), oz.p_i32(n0), C.byref(m), C.byref(cv), C.byref(cs), C.byref(budget)))
    return g, armed, n0, (m.value, cv.value, cs.value, budget.value)


def _policy(oz, s):
    pi, action, rc = np.zeros((s.G, 64), np.float32), np.zeros(s.G, np.int32), np.zeros(s.G, np.int32)
    oz.check(s.lib.oz_mcts_gumbel_policy(s.h, oz.p_f32(pi), oz.p_i32(action), oz.p_i32(rc)))
    score = np.zeros((s.G, 64), np.float64)
    oz.check(s.lib.oz_mcts_gumbel_scores(s.h, oz.p_f64(score)))
    return pi, action, rc, score


def _node_values(oz, s, g):
    out = []
    for i in range(int(s.num_nodes()[g])):
        v = C.c_double(-9.0)
        oz.check(s.lib.oz_mcts_node_value(s.h, g, i, C.byref(v)))
        out.append(v.value)
    return out


def _four_roots(n):
    """the opening, a mid-game root, a root with one legal move and a near-end root"""
    pool = _golden_roots(n, 64)
    b, w = initial_board(n)
    one = next(r for r in pool if popcount(legal_mask(*r, n)) == 1)
    wide = [r for r in pool if popcount(legal_mask(*r, n)) >= 5]
    mid = min(wide, key=lambda r: abs(popcount(r[0] | r[1]) - n * n // 2))
    late = max(wide, key=lambda r: popcount(r[0] | r[1]))
    assert len({(b, w), one, mid, late}) == 4
    return [(b, w), mid, one, late]


def _check_policy(oz, s, refs, roots, live=None):
    pi, action, rc, score = _policy(oz, s)
    for gi, ref in enumerate(refs):
        if live is not None and not live[gi]:
            assert rc[gi] == 3 and action[gi] == -1 and not pi[gi].any()
            continue
        r = ref.root_eval(*roots[gi])
        assert r["gap_move"] >= NEAR_TIE, (gi, r["gap_move"])
        assert rc[gi] == 0 and int(action[gi]) == r["move"], (gi, int(action[gi]), r["move"])
        d = float(np.abs(pi[gi].astype(np.float64) - r["pi"].astype(np.float64)).max())
        assert d <= 2e-7, (gi, d)
        lg = legal_mask(*roots[gi], s.n)
        assert abs(float(pi[gi].astype(np.float64).sum()) - 1.0) <= 1e-6 and all(pi[gi][q] == 0.0 for q in range(64) if not (lg >> q) & 1)
        for q in range(64):
            if (lg >> q) & 1 and np.isfinite(r["score"][q]):
                assert abs(score[gi][q] - r["score"][q]) <= 1e-9, (gi, q)
            else:
                assert score[gi][q] == -np.inf
    return pi, action


# ------------------------------------------------------------------ 1. the bare search with host-supplied g, simulation by simulation
@pytest.mark.parametrize("m", [4, 1])
@pytest.mark.parametrize("n", [6, 8])
def test_bare_search_vs_restatement(oz, n, m):
    from othellozero_amd.NNet import StubNetWrapper
    roots = _four_roots(n)
    G = len(roots)
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    s = Search(oz, n, G)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    g = np.array([R.gumbel_row(legal_mask(o, p, n), SEED, gi, 0) for gi, (o, p) in enumerate(roots)])
    oz.check(_set(oz, s, g, m=m))
    got, armed, n0, params = _get(oz, s)
    assert np.array_equal(got, g) and armed.all() and not n0.any() and params == (m, C_VISIT, C_SCALE, BUDGET)
    refs = [R.GumbelSearch(n, 1.0, salt=SALT) for _ in range(G)]
    for gi, ref in enumerate(refs):
        ref.arm(*roots[gi], g[gi], m, C_VISIT, C_SCALE, BUDGET)
    for sim in range(BUDGET + 1 + 4):                       # one simulation expands the root, BUDGET follow the schedule, 4 the max-n rule
        before = s.counts()
        oz.check(s.simulate(net, 1))
        cnt = s.counts()
        for gi, ref in enumerate(refs):
            ref.simulate(*roots[gi], 1)
            assert np.array_equal(cnt[gi], ref.counts(*roots[gi])[0]), (n, m, gi, sim)
            if sim > BUDGET:                                # beyond the budget: the visit went to a move with the most visits
                assert before[gi][int(np.argmax(cnt[gi] - before[gi]))] == before[gi].max()
        if sim == BUDGET:
            for gi in range(G):
                nz = sorted(int(x) for x in cnt[gi] if x)
                k = popcount(legal_mask(*roots[gi], n))
                assert nz == ([16] if m == 1 or k == 1 else [2, 2, 6, 6]), (n, m, gi, nz)
            _check_policy(oz, s, refs, roots)
    assert min(r.min_gap for r in refs) >= NEAR_TIE
    for gi, ref in enumerate(refs):
        assert_same_tables(s.dump(gi), ref, (n, m, gi))
        # the header keeps the network's v of every node expanded under the option
        assert _node_values(oz, s, gi) == [ref.vhat[i] for i in range(len(ref.nodes))]
        assert any(v != 0.0 for v in ref.vhat.values())
    _check_policy(oz, s, refs, roots)


# ------------------------------------------------------------------ 2. device-drawn g
def test_device_drawn_g_and_the_search_fed_with_it(oz):
    from othellozero_amd import agents
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 8, 16
    roots = _golden_roots(n, G)
    legal = [legal_mask(o, p, n) for o, p in roots]
    ids, plies = [1000 + gi for gi in range(G)], [popcount(o | p) - 4 for o, p in roots]
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    s = Search(oz, n, G)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(_sample(oz, s, SEED, ids, plies))
    g, armed, n0, _ = _get(oz, s)
    want = agents.rules_gumbel_draws(SEED, ids, plies, legal)
    worst = ulps(g, want).max()
    print(f"largest distance of the device's g from oz_gumbel_draws over {sum(popcount(x) for x in legal)} draws: {worst:.0f} ulp")
    assert armed.all() and not n0.any() and np.isfinite(g).all()
    assert all(g[gi][q] == 0.0 for gi in range(G) for q in range(64) if not (legal[gi] >> q) & 1)
    assert worst <= 4
    refs = [R.GumbelSearch(n, 1.0, salt=SALT) for _ in range(G)]
    for gi, ref in enumerate(refs):
        ref.arm(*roots[gi], g[gi], M, C_VISIT, C_SCALE, BUDGET)      # the search fed its own read-back g
        ref.simulate(*roots[gi], BUDGET + 1)
    oz.check(s.simulate(net, BUDGET + 1))
    assert min(r.min_gap for r in refs) >= NEAR_TIE
    for gi, ref in enumerate(refs):
        assert_same_tables(s.dump(gi), ref, gi)
    _check_policy(oz, s, refs, roots)


# ------------------------------------------------------------------ 3. tree reuse: two consecutive moves
def test_tree_reuse_over_two_moves(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims = 6, 8, 12
    roots = _golden_roots(n, G)
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    s = Search(oz, n, G)
    refs = [R.GumbelSearch(n, 1.0, salt=SALT) for _ in range(G)]
    live = [True] * G
    reused = 0
    for mv in range(2):
        s.set_roots([r[0] for r in roots], [r[1] for r in roots], [1 if x else 0 for x in live])
        if mv:
            assert not _get(oz, s)[1].any()                 # another board: the slot lost its draw
        g = np.array([R.gumbel_row(legal_mask(o, p, n), SEED, gi, mv) for gi, (o, p) in enumerate(roots)])
        oz.check(_set(oz, s, g, budget=sims))
        _, armed, n0, _ = _get(oz, s)
        assert list(armed) == [1 if x else 0 for x in live]
        known = [live[gi] and roots[gi] in refs[gi].index for gi in range(G)]
        for gi, ref in enumerate(refs):
            if not live[gi]:
                continue
            ref.arm(*roots[gi], g[gi], M, C_VISIT, C_SCALE, sims)
            assert list(n0[gi]) == ref.gum["n0"], (mv, gi)   # the leftover counts of the first search
            reused += 1 if mv and any(ref.gum["n0"]) else 0
        oz.check(s.simulate(net, sims))
        cnt = s.counts()
        for gi, ref in enumerate(refs):
            if not live[gi]:
                continue
            ref.simulate(*roots[gi], sims)
            assert_same_tables(s.dump(gi), ref, (mv, gi))
            nv = np.array(ref.visits(*roots[gi]))
            assert np.array_equal(cnt[gi] - n0[gi], nv) and nv.sum() == sims - (0 if known[gi] else 1)
            if known[gi] and popcount(legal_mask(*roots[gi], n)) >= 4:      # considered_visits(4, 12) = 0 0 0 0 1 1 2 2 3 3 4 4
                assert sorted(int(x) for x in nv if x) == [1, 1, 5, 5], (mv, gi, nv)
        assert min(r.min_gap for r in refs) >= NEAR_TIE
        _, action = _check_policy(oz, s, refs, roots, live)
        for gi in range(G):
            if live[gi]:
                roots[gi] = next_state(*roots[gi], n, int(action[gi]))
                live[gi] = legal_mask(*roots[gi], n) != 0
    assert reused >= 1                                      # not vacuous: a second search started from a root with visits


# ------------------------------------------------------------------ 4. off is off
def test_off_is_off_and_disarmed_is_puct(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 4
    roots = _golden_roots(n, 8)[:G]
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    want = [WideSearch(n, 1.0, 1, salt=SALT) for _ in range(G)]
    for r, (o, p) in zip(want, roots):
        r.simulate(o, p, 30)
    a = Search(oz, n, G)                                    # never switched on
    a.set_roots([r[0] for r in roots], [r[1] for r in roots])
    g, armed, n0, params = _get(oz, a)
    assert not g.any() and not armed.any() and not n0.any() and params == (0, 0.0, 0.0, 0)
    oz.check(a.simulate(net, 30))
    pi, action, rc = np.zeros((G, 64), np.float32), np.zeros(G, np.int32), np.zeros(G, np.int32)
    assert a.lib.oz_mcts_gumbel_policy(a.h, oz.p_f32(pi), oz.p_i32(action), oz.p_i32(rc)) == oz.OZ_ERR_STATE
    for gi in range(G):
        assert_same_tables(a.dump(gi), want[gi], ("never", gi))
        assert _node_values(oz, a, gi) == [0.0] * len(want[gi].nodes)
    b = Search(oz, n, G)                                    # switched on, every slot disarmed: PUCT, and the header keeps v
    b.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(_set(oz, b, None))
    assert not _get(oz, b)[1].any()
    c = Search(oz, n, G)                                    # armed slots next to disarmed ones
    c.set_roots([r[0] for r in roots], [r[1] for r in roots])
    gg = np.array([R.gumbel_row(legal_mask(o, p, n), SEED, gi, 0) for gi, (o, p) in enumerate(roots)])
    oz.check(_set(oz, c, gg, [1, 0, 1, 0]))
    assert list(_get(oz, c)[1]) == [1, 0, 1, 0]
    oz.check(b.simulate(net, 30))
    oz.check(c.simulate(net, 30))
    ref, puct = [R.GumbelSearch(n, 1.0, salt=SALT) for _ in range(G)], [R.GumbelSearch(n, 1.0, salt=SALT) for _ in range(G)]
    for gi, (o, p) in enumerate(roots):
        if gi in (0, 2):
            ref[gi].arm(o, p, gg[gi], M, C_VISIT, C_SCALE, BUDGET)
        ref[gi].simulate(o, p, 30)
        puct[gi].simulate(o, p, 30)
    for gi in range(G):
        assert_same_tables(b.dump(gi), want[gi], ("disarmed", gi))
        assert _node_values(oz, b, gi) == [puct[gi].vhat[i] for i in range(len(puct[gi].nodes))]
        assert_same_tables(c.dump(gi), ref[gi], ("mixed", gi))
        assert _node_values(oz, c, gi) == [ref[gi].vhat[i] for i in range(len(ref[gi].nodes))]
    # other boards: the draw is dropped -- except where the board stays
    other = _golden_roots(n, 8)[G:]
    moved = [roots[0]] + list(other[1:])
    oz.check(_set(oz, c, gg))
    c.set_roots([r[0] for r in moved], [r[1] for r in moved])
    assert list(_get(oz, c)[1]) == [1, 0, 0, 0]


# ------------------------------------------------------------------ 5. the host-evaluator split
def test_host_evaluator_split_honours_the_option(oz):
    n, G, sims = 6, 4, BUDGET + 1
    roots = _four_roots(n)
    s = Search(oz, n, G)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    g = np.array([R.gumbel_row(legal_mask(o, p, n), SEED, gi, 0) for gi, (o, p) in enumerate(roots)])
    oz.check(_set(oz, s, g))
    refs = [R.GumbelSearch(n, 1.0, salt=SALT) for _ in range(G)]
    for gi, ref in enumerate(refs):
        ref.arm(*roots[gi], g[gi], M, C_VISIT, C_SCALE, BUDGET)
        ref.simulate(*roots[gi], sims)
    for _ in range(sims):
        oz.check(s.lib.oz_mcts_select(s.h))
        status, own, opp = np.zeros(G, np.int32), np.zeros(G, np.uint64), np.zeros(G, np.uint64)
        oz.check(s.lib.oz_mcts_leaves(s.h, oz.p_i32(status), oz.p_u64(own), oz.p_u64(opp)))
        pi, v = np.zeros((G, n * n), np.float32), np.zeros(G, np.float32)
        for gi in range(G):
            if status[gi] == oz.LEAF_EVAL:
                p, val = oracle.stub_predict(int(own[gi]), int(opp[gi]), n, SALT, 0)
                pi[gi], v[gi] = p.ravel(), val
        oz.check(s.lib.oz_mcts_backup(s.h, oz.p_f32(pi), oz.p_f32(v)))
    for gi, ref in enumerate(refs):
        assert_same_tables(s.dump(gi), ref, gi)
        assert _node_values(oz, s, gi) == [ref.vhat[i] for i in range(len(ref.nodes))]


# ------------------------------------------------------------------ 6. refusals
def test_refusals(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 4
    roots = _golden_roots(n, 8)[:G]
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G * 2)
    g = np.array([R.gumbel_row(legal_mask(o, p, n), SEED, gi, 0) for gi, (o, p) in enumerate(roots)])
    ids, plies = oz.p_u64(np.arange(G, dtype=np.uint64)), oz.p_i32(np.zeros(G, np.int32))

    def fresh():
        s = Search(oz, n, G)
        s.set_roots([r[0] for r in roots], [r[1] for r in roots])
        return s
    # arguments
    s = fresh()
    for kw in (dict(m=0), dict(m=65), dict(c_visit=-1.0), dict(c_scale=0.0), dict(c_scale=-2.0), dict(c_visit=float("nan")),
               dict(c_scale=float("nan")), dict(budget=0), dict(budget=-1)):
        assert _set(oz, s, g, **kw) == oz.OZ_ERR_ARG, kw
        assert _sample(oz, s, SEED, list(range(G)), [0] * G, **kw) == oz.OZ_ERR_ARG, kw
    bad = g.copy()
    bad[1, 5] = np.inf
    assert _set(oz, s, bad) == oz.OZ_ERR_ARG
    assert _get(oz, s)[3] == (0, 0.0, 0.0, 0)               # a refused call leaves the object as it was
    # a non-empty tree
    oz.check(s.simulate(net, 3))
    assert _set(oz, s, g) == oz.OZ_ERR_STATE and _sample(oz, s, SEED, list(range(G)), [0] * G) == oz.OZ_ERR_STATE
    oz.check(s.lib.oz_mcts_reset(s.h, -1))
    oz.check(_set(oz, s, g))                                # after a reset of every game it may be switched on
    oz.check(s.simulate(net, 3))
    oz.check(_set(oz, s, g))                                # and, once on, armed again over its own tree
    # what the Gumbel search replaces
    eta = np.full((G, 64), 1.0 / 64)
    assert s.lib.oz_mcts_set_root_noise(s.h, 0.25, oz.p_f64(eta), None) == oz.OZ_ERR_STATE
    assert s.lib.oz_mcts_sample_root_noise(s.h, 0.5, 0.25, 1, ids, plies) == oz.OZ_ERR_STATE
    act, rc = np.zeros(G, np.int32), np.zeros(G, np.int32)
    assert s.lib.oz_mcts_sample_moves(s.h, 1.0, 1, ids, plies, oz.p_i32(act), oz.p_i32(rc)) == oz.OZ_ERR_STATE
    assert s.lib.oz_mcts_set_forced_playouts(s.h, 2.0) == oz.OZ_ERR_STATE
    assert s.set_k(2) == oz.OZ_ERR_STATE and s.lib.oz_mcts_use_wide_kernels(s.h, 1) == oz.OZ_ERR_STATE
    oz.check(s.set_k(1))
    # a pending host-evaluated step
    oz.check(s.lib.oz_mcts_select(s.h))
    assert _set(oz, s, g) == oz.OZ_ERR_STATE
    # objects that already run what it replaces
    t = fresh()
    oz.check(t.lib.oz_mcts_set_root_noise(t.h, 0.25, oz.p_f64(eta), None))
    assert _set(oz, t, g) == oz.OZ_ERR_STATE
    u = fresh()
    oz.check(u.set_k(2))
    assert _set(oz, u, g) == oz.OZ_ERR_STATE


# ------------------------------------------------------------------ 7. the engine: whole games replayed by the restatement
RNG_COIN, RNG_EXPLORE = 0, 1
ENG_SEED = 777


def _coin(seed, gid, ply):
    return float(int(oracle.lib().orc_rng(seed, gid, ply, RNG_COIN)) >> 11) * R.UNIT


def _replay_games(n, rec, rows, sims, m, e_greedy, seed, values=None, evaluator=None):
    """every record of every game against a hand-driven GumbelSearch per game (the engine's tree persists across the moves of a game)"""
    picked = explored = 0
    for gid in sorted(set(int(x) for x in rec["game_id"])):
        idx = [i for i in range(rec.size) if int(rec[i]["game_id"]) == gid]
        assert [int(rec[i]["ply"]) for i in idx] == list(range(len(idx)))
        ref = R.GumbelSearch(n, 1.0, salt=SALT, evaluator=evaluator)
        for i in idx:
            r = rec[i]
            ply, player = int(r["ply"]), int(r["player"])
            own, opp = (int(r["black"]), int(r["white"])) if player == 1 else (int(r["white"]), int(r["black"]))
            lg = legal_mask(own, opp, n)
            ref.arm(own, opp, R.gumbel_row(lg, seed, gid, ply), m, C_VISIT, C_SCALE, sims)
            ref.simulate(own, opp, sims)
            ev = ref.root_eval(own, opp)
            assert ev["gap_move"] >= NEAR_TIE and ref.min_gap >= NEAR_TIE, (gid, ply)
            d = float(np.abs(rows[i].astype(np.float64) - ev["pi"].astype(np.float64)).max())
            assert d <= 2e-7, (gid, ply, d)
            if _coin(seed, gid, ply) <= e_greedy:
                assert (int(r["action"]), int(r["greedy"])) == (ev["move"], 3), (gid, ply)
                picked += 1
            else:
                squares = [q for q in range(64) if (lg >> q) & 1]
                assert (int(r["action"]), int(r["greedy"])) == (squares[int(oracle.lib().orc_rng(seed, gid, ply, RNG_EXPLORE)) % len(squares)], 0)
                explored += 1
            if values is not None:                         # the root value keeps its definition: the visit-weighted mean of Q over the raw counts
                N, Q, _, _ = ref.rows(own, opp)
                assert values[i] == oracle.pairwise_sum(np.array([float(N[q]) * Q[q] if N[q] > 0 else 0.0 for q in range(64)])) / float(sum(N))
    return picked, explored


@pytest.mark.parametrize("e_greedy", [0.8, 1.0])
def test_whole_games_vs_restatement(oz, e_greedy):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine, selfplay_batch
    n, G, sims, m = 6, 8, 16, 4
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    rec, rows = selfplay_batch(net, n, G, sims, 1.0, 1.0, e_greedy, ENG_SEED, 100, gumbel=(m, C_VISIT, C_SCALE))
    assert rows.shape == (rec.size, 64) and rows.dtype == np.float32 and len(set(rec["game_id"])) == G
    picked, explored = _replay_games(n, rec, rows, sims, m, e_greedy, ENG_SEED)
    assert picked == int((rec["greedy"] == 3).sum()) and explored == int((rec["greedy"] == 0).sum()) and picked + explored == rec.size
    assert selfplay_batch.gumbel_stats == dict(max_considered=m, c_visit=C_VISIT, c_scale=C_SCALE, moves=picked)
    assert (explored > 0) == (e_greedy < 1.0)
    for i in range(rec.size):
        lg = legal_mask(*((int(rec[i]["black"]), int(rec[i]["white"])) if rec[i]["player"] == 1 else (int(rec[i]["white"]), int(rec[i]["black"]))), n)
        assert abs(float(rows[i].astype(np.float64).sum()) - 1.0) <= 1e-6 and all(rows[i][q] == 0.0 for q in range(64) if not (lg >> q) & 1)
    # recorded root values keep their definition
    eng = SelfPlayEngine(net, n, G, sims, 1.0, 1.0, e_greedy, ENG_SEED, 100, record_values=True, gumbel=(m, C_VISIT, C_SCALE))
    eng.play_to_end()
    rec2, values, rows2 = eng.records(with_values=True, with_policies=True)
    assert rec2.tobytes() == rec.tobytes() and rows2.tobytes() == rows.tobytes()
    _replay_games(n, rec2, rows2, sims, m, e_greedy, ENG_SEED, values=values)


def test_whole_games_with_solved_leaves(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import selfplay_batch
    n, G, sims, m, E = 6, 8, 16, 4, 6
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    rec, rows = selfplay_batch(net, n, G, sims, 1.0, 1.0, 1.0, ENG_SEED, 100, gumbel=(m, C_VISIT, C_SCALE), solve_leaves=E)
    assert selfplay_batch.rows_solved > 0
    import solve_leaves_ref as SL
    ev = SL.evaluator(E, SL.stub(SALT, 0))
    _replay_games(n, rec, rows, sims, m, 1.0, ENG_SEED, evaluator=ev)
    assert ev.solved > 0


# ------------------------------------------------------------------ 8. the engine: tree reuse between two moves, off is off, examples, refusals
def test_engine_tree_reuse(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G, sims, m = 6, 8, 12, 4
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    eng = SelfPlayEngine(net, n, G, sims, 1.0, 1.0, 1.0, ENG_SEED, 100, gumbel=(m, C_VISIT, C_SCALE))
    refs = [R.GumbelSearch(n, 1.0, salt=SALT) for _ in range(G)]
    reused = 0
    for mv in range(2):
        st = eng.state()
        roots = [((int(b), int(w)) if p == 1 else (int(w), int(b))) for b, w, p in zip(st["black"], st["white"], st["player"])]
        eng.run(1)
        g, armed, n0 = eng.last_gumbel()
        cnt = eng.last_counts()
        assert armed.all()
        for gi, ref in enumerate(refs):
            lg = legal_mask(*roots[gi], n)
            want = R.gumbel_row(lg, ENG_SEED, 100 + gi, mv)
            assert ulps(g[gi], want).max() <= 4
            ref.arm(*roots[gi], g[gi], m, C_VISIT, C_SCALE, sims)
            assert list(n0[gi]) == ref.gum["n0"], (mv, gi)   # the second search starts from the first one's leftover counts
            known = any(ref.gum["n0"])
            reused += 1 if mv and known else 0
            ref.simulate(*roots[gi], sims)
            assert np.array_equal(cnt[gi], ref.counts(*roots[gi])[0]), (mv, gi)
            nv = np.array(ref.visits(*roots[gi]))
            if roots[gi] in ref.index and (mv == 0 or known) and popcount(lg) >= 4:
                assert sorted(int(x) for x in nv if x) == ([1, 1, 4, 5] if mv == 0 else [1, 1, 5, 5]), (mv, gi, nv)
            assert ref.min_gap >= NEAR_TIE
        st2 = eng.state()
        for gi, ref in enumerate(refs):                    # the move the engine played is the restatement's
            ev = ref.root_eval(*roots[gi])
            nb, nw = next_state(*roots[gi], n, ev["move"])
            mover = int(st2["player"][gi])
            assert ((int(st2["black"][gi]), int(st2["white"][gi])) if mover == 1 else (int(st2["white"][gi]), int(st2["black"][gi]))) == (nb, nw)
    assert reused >= 1


def test_engine_off_is_off(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G, sims = 6, 8, 16
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    out = []
    for kw in ({}, {"gumbel": None}):
        eng = SelfPlayEngine(net, n, G, sims, 1.0, 1.0, 0.9, ENG_SEED, 100, record_visits=True, **kw)
        rec, counts = eng.play_to_end(with_visits=True)
        st = {k: v for k, v in eng.stats().items()}
        out.append((rec.tobytes(), counts.tobytes(), st))
        assert eng.gumbel_stats() == dict(max_considered=0, c_visit=0.0, c_scale=0.0, moves=0)
        g, armed, n0 = eng.last_gumbel()
        assert not g.any() and not armed.any() and not n0.any()    # nothing was ever allocated: the readers give zeros
        with pytest.raises(oz.OzError):
            eng.records(with_policies=True)
        assert not (rec["greedy"] == 3).any()
    assert out[0] == out[1]


def test_examples_from_policy_rows(oz):
    from othellozero_amd import loop
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import selfplay_batch, training_example_symmetries
    n, G = 6, 4
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    rec, rows = selfplay_batch(net, n, G, 8, 1.0, 1.0, 1.0, ENG_SEED, 100, gumbel=(4, C_VISIT, C_SCALE))
    for alias in (False, True):
        ex = loop.examples_from_records(rec, n, alias_final=alias, policies=rows)
        plain = loop.examples_from_records(rec, n, alias_final=alias)
        assert len(ex) == len(plain) == rec.size * 8
        for i in range(rec.size):
            policy = np.array([[rows[i, r * 8 + c] for c in range(n)] for r in range(n)], np.float32)
            for t, (_, sp) in enumerate(training_example_symmetries(np.zeros((n, n)), policy)):
                b, p, z = ex[i * 8 + t]
                assert np.array_equal(b, plain[i * 8 + t][0]) and z == plain[i * 8 + t][2]
                assert p.dtype == np.float32 and np.array_equal(p.view(np.uint32), np.ascontiguousarray(sp).view(np.uint32))


def test_engine_refusals(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine, selfplay_batch
    n, G, sims = 6, 4, 8
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G * 2)
    lib = oz.load()
    gum = (4, C_VISIT, C_SCALE)
    # the Python surface refuses before any library call
    for kw in (dict(root_noise=(0.5, 0.25)), dict(root_noise=(0.5, 0.25), forced_playouts=2.0), dict(sample_moves=(1.0, 8)),
               dict(playout_cap=(4, 0.5)), dict(leaves_per_step=2)):
        with pytest.raises(ValueError):
            SelfPlayEngine(net, n, G, sims, gumbel=gum, **kw)
        with pytest.raises(ValueError):
            selfplay_batch(net, n, G, sims, gumbel=gum, **kw)
    with pytest.raises(ValueError):
        selfplay_batch(net, n, G, sims, gumbel=gum, expand=True)
    for bad in ((0, 50.0, 1.0), (65, 50.0, 1.0), (4, -1.0, 1.0), (4, 50.0, 0.0), (4, float("nan"), 1.0)):
        with pytest.raises(ValueError):
            SelfPlayEngine(net, n, G, sims, gumbel=bad)
    # the C ABI: whichever comes second is refused, in either order
    eng = SelfPlayEngine(net, n, G, sims, gumbel=gum)
    assert lib.oz_selfplay_set_root_noise(eng._h, 0.5, 0.25) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_set_move_sampling(eng._h, 1.0, 8) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_set_playout_cap(eng._h, 4, 0.5) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_set_forced_playouts(eng._h, 2.0) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_set_leaves_per_step(eng._h, 2) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_set_gumbel(eng._h, 0, 50.0, 1.0) == oz.OZ_ERR_ARG
    assert lib.oz_selfplay_stagger(eng._h, sims) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_run_steps(eng._h, 1) == oz.OZ_ERR_STATE
    eng.run(1)
    assert lib.oz_selfplay_run_steps(eng._h, 1) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_set_gumbel(eng._h, 4, 50.0, 1.0) == oz.OZ_ERR_STATE      # after the first driver call
    for kw in (dict(root_noise=(0.5, 0.25)), dict(sample_moves=(1.0, 8)), dict(playout_cap=(4, 0.5)), dict(leaves_per_step=2)):
        other = SelfPlayEngine(net, n, G, sims, **kw)
        assert lib.oz_selfplay_set_gumbel(other._h, 4, 50.0, 1.0) == oz.OZ_ERR_STATE, kw
    driven = SelfPlayEngine(net, n, G, sims)
    driven.run(1)
    assert lib.oz_selfplay_set_gumbel(driven._h, 4, 50.0, 1.0) == oz.OZ_ERR_STATE


# ------------------------------------------------------------------ 9. the device replay buffer and the training loop
@pytest.mark.parametrize("alias_final", [False, True])
def test_device_replay_of_improved_rows(oz, alias_final):
    from othellozero_amd import loop
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.trainer import pack_examples
    from othellozero_amd.training import SelfPlayEngine
    n, G, sims = 6, 4, 8
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    eng = SelfPlayEngine(net, n, G, sims, 1.0, 1.0, 0.9, ENG_SEED, 100, gumbel=(4, C_VISIT, C_SCALE))
    eng.play_to_end()
    rec, rows = eng.records(with_policies=True)
    want = pack_examples(loop.examples_from_records(rec, n, alias_final=alias_final, policies=rows), n)
    E = rec.size * 8
    cap = E - 8 * 3 - 5                                     # smaller than the append: the first examples are dropped and a record straddles the wrap
    big, small = ReplayBuffer(n, E + 7), ReplayBuffer(n, cap)
    assert big.append_engine(eng, alias_final=alias_final, target="improved") == rec.size
    got = big.read()
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    small.append_examples(*(x[:11] for x in want))          # move the write position off a record boundary first
    assert small.append_engine(eng, alias_final=alias_final, policy_target="improved") == rec.size
    held, _, total = small.info()
    assert (held, total) == (cap, 11 + E)
    got = small.read()
    for k in range(total - cap, total):                     # running index k lives in slot k % cap
        j = k - 11
        for a, b in zip(got, want):
            assert a[k % cap].tobytes() == b[j].tobytes(), k
    # refusals: host records with the new target, an engine without the option
    with pytest.raises(ValueError):
        big.append_records(rec, policy_target="improved")
    lib = oz.load()
    assert lib.oz_replay_append_records(big._h, rec.ctypes.data_as(C.c_void_p), None, rec.size, 0, oz.REPLAY_TARGET_POLICY, 1.0) == oz.OZ_ERR_ARG
    plain = SelfPlayEngine(net, n, G, sims, 1.0, 1.0, 0.9, ENG_SEED, 100)
    plain.play_to_end()
    with pytest.raises(oz.OzError):
        big.append_engine(plain, target="improved")


def _loop_kw(tmp_path, n):
    return dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
                evaluation_interval=2, evaluation_iterations=2, temperature_threshold=0, self_play_training=False, self_play_interval=1,
                self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
                training_buffer_size=8 * 40 * 8, seed=13)


def test_training_loop_on_improved_policy_targets(oz, tmp_path, monkeypatch):
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.trainer import pack_examples
    monkeypatch.chdir(tmp_path)
    n = 6
    seen = {}
    for replay in ("host", "device"):
        net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8, policy_loss="flat")
        net.set_weights(seen["weights"]) if "weights" in seen else seen.setdefault("weights", net.get_weights())
        fit = net.train

        def spy(data, *a, _replay=replay, _fit=fit, **kw):
            if _replay == "device":
                seen[_replay] = data.read()
            else:                                           # the host path shuffles its buffer before the fit: compare as sorted rows
                seen[_replay] = pack_examples(list(data), n)
            h = _fit(data, *a, **kw)
            seen[_replay + "_loss"] = [float(x) for x in h.history["loss"]]
            return h
        monkeypatch.setattr(net, "train", spy)
        assert loop.training(neural_network=net, replay=replay, gumbel=(4, 50, 1), policy_target="improved", alias_final_boards=False,
                             **_loop_kw(tmp_path, n)) == []
        assert seen[replay + "_loss"] and np.isfinite(seen[replay + "_loss"]).all()

    def rows(t):
        own, opp, pi, z = t
        return sorted(zip(own.tolist(), opp.tolist(), (p.tobytes() for p in pi), z.tolist()))
    assert len(seen["host"][0]) > 0 and rows(seen["host"]) == rows(seen["device"])
    pi = seen["device"][2]
    assert np.abs(pi.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6 and ((pi > 0) & (pi < 1)).any()
    # refusals of the loop
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8, policy_loss="flat")
    for kw in (dict(policy_target="improved"), dict(gumbel=True, policy_target="improved", alias_final_boards=True),
               dict(gumbel=True, root_noise=(0.5, 0.25)), dict(gumbel=True, sample_moves=(1.0, 4)), dict(gumbel=True, playout_cap=(2, 0.5)),
               dict(gumbel=True, leaves_per_step=2), dict(gumbel=True, distributed=True)):
        with pytest.raises(ValueError):
            loop.training(neural_network=net, **{**dict(alias_final_boards=False), **kw}, **_loop_kw(tmp_path, n))


# ------------------------------------------------------------------ 10. the drop-ins
def test_drop_in_search_and_episode(oz, monkeypatch):
    import random
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.othelo_mcts import OthelloMCTS
    from othellozero_amd.training import execute_episode, selfplay_batch
    n, sims, seed = 6, 16, ENG_SEED
    net = StubNetWrapper((n, n), SALT, 0, max_batch=1)
    # one search through OthelloMCTS against the restatement
    own, opp = _golden_roots(n, 8)[3]
    state = oz.unpack_board(own, opp, n)
    mcts = OthelloMCTS(n, net, 1.0, gumbel=(M, C_VISIT, C_SCALE))
    from othellozero_amd.Othello import OthelloPlayer
    mcts.sample_gumbel(sims, seed, 5, 2, state=state, player=OthelloPlayer.BLACK)
    g, armed, n0 = mcts.gumbel_root()
    assert armed and not n0.any() and ulps(g, R.gumbel_row(legal_mask(own, opp, n), seed, 5, 2)).max() <= 4
    mcts.simulate_n(state, OthelloPlayer.BLACK, sims)
    ref = R.GumbelSearch(n, 1.0, salt=SALT)
    ref.arm(own, opp, g, M, C_VISIT, C_SCALE, sims)
    ref.simulate(own, opp, sims)
    ev = ref.root_eval(own, opp)
    assert ref.min_gap >= NEAR_TIE and ev["gap_move"] >= NEAR_TIE
    action, pi = mcts.gumbel_policy(state)
    assert action == (ev["move"] >> 3, ev["move"] & 7) and pi.shape == (n, n) and pi.dtype == np.float32
    assert np.abs(pi.astype(np.float64) - ev["pi"].reshape(8, 8)[:n, :n].astype(np.float64)).max() <= 2e-7
    with pytest.raises(ValueError):
        OthelloMCTS(n, net, 1.0).gumbel_policy(state)
    with pytest.raises(ValueError):
        OthelloMCTS(n, net, 1.0, gumbel=True, leaves_per_step=2)
    with pytest.raises(KeyError):
        OthelloMCTS(n, net, 1.0, gumbel=True).gumbel_policy(state)
    # a whole episode is game 0 of the engine with the same seed (coin and explore draws keyed like the engine's)
    L = oracle.lib()
    ply = [0]
    monkeypatch.setattr(random, "random", lambda: (L.orc_rng(seed, 0, ply[0], 0) >> 11) * (1.0 / 9007199254740992.0))
    monkeypatch.setattr(np.random, "choice", lambda k: L.orc_rng(seed, 0, ply[0], 1) % k)
    rec, rows = selfplay_batch(StubNetWrapper((n, n), SALT, 0, max_batch=1), n, 1, sims, 1.0, 1.0, 0.8, seed, 0, gumbel=(M, C_VISIT, C_SCALE))
    from othellozero_amd import training as T
    play = T.OthelloGame.play

    def counted(self, *a, **kw):
        r = play(self, *a, **kw)
        ply[0] += 1
        return r
    monkeypatch.setattr(T.OthelloGame, "play", counted)
    ex = execute_episode(n, net, 1.0, sims, 1.0, 0.8, snapshot_boards=True, policy_target="improved", gumbel=(M, C_VISIT, C_SCALE), gumbel_seed=seed)
    assert len(ex) == rec.size * 8
    for i in range(rec.size):
        want = rows[i].reshape(8, 8)[:n, :n]
        assert np.abs(ex[i * 8 + 7][1].astype(np.float64) - want.astype(np.float64)).max() <= 2e-7, i        # (the identity is the last of the 8)
    for kw in (dict(root_noise=(0.5, 0.25)), dict(sample_moves=(1.0, 4)), dict(leaves_per_step=2)):
        with pytest.raises(ValueError):
            execute_episode(n, net, 1.0, sims, 1.0, 0.8, gumbel=True, **kw)
    with pytest.raises(ValueError):
        execute_episode(n, net, 1.0, sims, 1.0, 0.8, policy_target="improved")
    with pytest.raises(ValueError):
        execute_episode(n, net, 1.0, sims, 1.0, 0.8, policy_target="improved", gumbel=True)
