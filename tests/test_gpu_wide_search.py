"""Leaf-parallel search on the GPU (pytest -m gpu): the wide kernels at K = 1 against the reference's golden traces, at K > 1
against the restatement in tests/wide_search_ref.py.  Every comparison is equality of bits."""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import load_golden
from wide_search_ref import (WideSearch, apply_move, assert_same_tables, initial_board, legal_mask, next_state, popcount,
                             tie_draw)

pytestmark = pytest.mark.gpu

SPARSE = 0x0F0F0F0F0F0F0F0F


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


class Search:
    """a bare oz_mcts with G slots"""

    def __init__(self, oz, n, G, c=1.0, qmode=1, node_cap=2048):
        self.oz, self.lib, self.n, self.G = oz, oz.load(), n, G
        self.h = C.c_void_p()
        oz.check(self.lib.oz_mcts_create(C.byref(self.h), n, G, node_cap, float(c), qmode))

    def __del__(self):
        if self.h:
            self.lib.oz_mcts_destroy(self.h)
            self.h = C.c_void_p()

    def set_k(self, k):
        return self.lib.oz_mcts_set_leaves_per_step(self.h, k)

    def get_k(self):
        k = C.c_int()
        self.oz.check(self.lib.oz_mcts_get_leaves_per_step(self.h, C.byref(k)))
        return k.value

    def set_roots(self, own, opp, active=None):
        a, b = np.array(own, np.uint64), np.array(opp, np.uint64)
        act = None if active is None else self.oz.p_u8(np.array(active, np.uint8))
        self.oz.check(self.lib.oz_mcts_set_roots(self.h, self.oz.p_u64(a), self.oz.p_u64(b), act))

    def simulate(self, net, nsims):
        return self.lib.oz_mcts_simulate(self.h, net._h, int(nsims))

    def num_nodes(self):
        nn = np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_num_nodes(self.h, self.oz.p_i32(nn)))
        return nn

    def dump(self, g):
        nn = self.num_nodes()
        out = []
        for i in range(int(nn[g])):
            own, opp, legal, Ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
            N, Q, qt, P = np.zeros(64, np.int32), np.zeros(64, np.float64), np.zeros(64, np.uint8), np.zeros(64, np.float64)
            self.oz.check(self.lib.oz_mcts_dump_node(self.h, g, i, C.byref(own), C.byref(opp), C.byref(Ns), C.byref(legal),
                                                     self.oz.p_i32(N), self.oz.p_f64(Q), self.oz.p_u8(qt), self.oz.p_f64(P)))
            out.append(dict(k0=own.value, k1=opp.value, Ns=Ns.value, legal=legal.value, N=N, Q=Q, qtag=qt, P=P))
        return out

    def wide_stats(self):
        s = np.zeros(3, np.int64)
        self.oz.check(self.lib.oz_mcts_wide_stats(self.h, self.oz.p_i64(s)))
        return tuple(int(x) for x in s)

    def stats(self):
        s = np.zeros(5, np.int64)
        self.oz.check(self.lib.oz_mcts_stats(self.h, self.oz.p_i64(s)))
        return [int(x) for x in s]

    def counts(self):
        cnt, legal, rc = np.zeros((self.G, 64), np.int32), np.zeros(self.G, np.uint64), np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_root_counts(self.h, self.oz.p_i32(cnt), self.oz.p_u64(legal), self.oz.p_i32(rc)))
        return cnt


def _golden_roots(n, count):
    """distinct mover-canonical positions with a legal move out of the golden episodes of board size n"""
    g = load_golden("episodes.npz")
    seen, out = set(), []
    for name in g["names"]:
        name = str(name)
        if int(g[f"{name}/meta"][0]) != n:
            continue
        for b, w, p in zip(g[f"{name}/black"], g[f"{name}/white"], g[f"{name}/player"]):
            own, opp = (int(b), int(w)) if int(p) == 1 else (int(w), int(b))
            if (own, opp) not in seen and legal_mask(own, opp, n):
                seen.add((own, opp))
                out.append((own, opp))
    assert len(out) >= count, (n, len(out))
    step = len(out) // count
    return out[::step][:count]


def _first_max(cnt):
    return int(np.argmax(cnt))                         # the first maximum = the lowest square


# ------------------------------------------------------------------ 1. the wide kernels at K = 1 against the reference's traces
QT_F32 = 1


def _check_tables(dump, g, prefix):
    boards = g[prefix + "boards"]
    assert len(dump) == len(boards)
    for i, nd in enumerate(dump):
        assert (nd["k0"], nd["k1"]) == (int(boards[i][0]), int(boards[i][1])), (prefix, i)
        assert nd["Ns"] == int(g[prefix + "Ns"][i]) and nd["legal"] == int(g[prefix + "legal"][i])
        assert np.array_equal(nd["P"], g[prefix + "P"][i]), (prefix, i)
        assert np.array_equal(nd["N"], g[prefix + "N"][i]), (prefix, i)
        assert np.array_equal(nd["Q"], g[prefix + "Q"][i]), (prefix, i)
        if g[prefix + "edges_init"][i]:
            for sq in oracle.mask_to_squares(nd["legal"]):
                if nd["N"][sq]:
                    assert (nd["qtag"][sq] == 1) == (g[prefix + "qtype"][i][sq] == QT_F32), (prefix, i, sq)


def test_wide_kernels_at_k1_vs_golden_traces(oz, golden_mcts):
    """tests/golden/mcts.npz through oz_mcts_use_wide_kernels(1): tables, return values and their types, both Q regimes"""
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    g = golden_mcts
    regimes = set()
    for name in g["names"]:
        name = str(name)
        n, player, salt, keep, qmode, nsims = (int(x) for x in g[f"{name}/meta"])
        regimes.add(qmode)
        c = float(g[f"{name}/c"][0])
        root = oz.unpack_board(int(g[f"{name}/root"][0]), int(g[f"{name}/root"][1]), n)
        net = StubNetWrapper((n, n), salt, keep)
        m = OthelloMCTS(n, net, c, q_mode=qmode, node_cap=1024)
        oz.check(oz.load().oz_mcts_use_wide_kernels(m._h, 1))
        pl = OthelloPlayer(player)
        done, rets, rts = 0, [], []
        for cp in g[f"{name}/cps"]:
            while done < int(cp):
                r = m.simulate(root, pl)
                rets.append(float(r))
                rts.append(0 if isinstance(r, int) else (1 if isinstance(r, np.float32) else 2))
                done += 1
            _check_tables(m.dump(), g, f"{name}/cp{int(cp)}/")
        assert np.array_equal(np.array(rets), g[f"{name}/ret"]), name
        assert np.array_equal(np.array(rts, np.uint8), g[f"{name}/ret_type"]), name
        steps, coll, leaves = (m.wide_stats()[k] for k in ("steps", "collisions", "leaves"))
        assert (steps, coll) == (done, 0) and leaves == m.stats()["expansions"], name
    assert regimes == {0, 1}


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide_at_1"])
@pytest.mark.parametrize("qmode", [0, 1], ids=["nep50", "f64"])
def test_simulate_call_sizes_compose_at_k1(oz, qmode, wide):
    """simulate(0), (1), (1), (3) == simulate(5), bit for bit: one descent per step, so a call boundary changes nothing (the single-step, the
    fused and the empty launch sequence).  Not so at K > 1, where a call boundary changes which descents are in flight together."""
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 4
    roots = _golden_roots(n, G)
    net = StubNetWrapper((n, n), 13, 0, max_batch=G)
    a, b = Search(oz, n, G, qmode=qmode), Search(oz, n, G, qmode=qmode)
    for s in (a, b):
        oz.check(oz.load().oz_mcts_use_wide_kernels(s.h, 1 if wide else 0))
        s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    nodes0, stats0 = a.num_nodes(), a.stats()
    oz.check(a.simulate(net, 0))
    assert np.array_equal(a.num_nodes(), nodes0) and a.stats() == stats0
    for nsims in (1, 1, 3):
        oz.check(a.simulate(net, nsims))
    oz.check(b.simulate(net, 5))
    assert np.array_equal(a.num_nodes(), b.num_nodes()) and int(b.num_nodes().min()) > 0
    for gi in range(G):
        for x, y in zip(a.dump(gi), b.dump(gi)):
            assert (x["k0"], x["k1"], x["Ns"], x["legal"]) == (y["k0"], y["k1"], y["Ns"], y["legal"]), gi
            for key in ("N", "Q", "qtag", "P"):
                assert np.array_equal(x[key], y[key]), (gi, key)
    assert a.stats() == b.stats() and a.stats()[0] == 5 * G
    assert np.array_equal(a.counts(), b.counts())


# ------------------------------------------------------------------ 2. K > 1 against the restatement
def _run_vs_restatement(oz, n, K, keep, G, nsims_seq=(2, 25, 100), moves=3, move_sims=25):
    from othellozero_amd.NNet import StubNetWrapper
    salt = 13
    roots = _golden_roots(n, G)
    net = StubNetWrapper((n, n), salt, keep, max_batch=G * K)
    s = Search(oz, n, G)
    oz.check(s.set_k(K))
    assert s.get_k() == K
    refs = [WideSearch(n, 1.0, K, salt=salt, keep_mask=keep) for _ in range(G)]
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])

    def check(where):
        for gi in range(G):
            assert_same_tables(s.dump(gi), refs[gi], (n, K, keep, G, gi, where))
        want = tuple(sum(getattr(r, k) for r in refs) for k in ("steps", "collisions", "leaves"))
        assert s.wide_stats() == want, (where, s.wide_stats(), want)
        st = s.stats()
        assert st[0] == sum(r.sims for r in refs) and st[2] == want[2] and st[3] == sum(r.terminals for r in refs), where

    for nsims in nsims_seq:
        oz.check(s.simulate(net, nsims))
        for r, (own, opp) in zip(refs, roots):
            r.simulate(own, opp, nsims)
        check(("simulate", nsims))
    # a sequence of moves with the table kept: the first max-count square, then move_sims simulations from the new root
    live = [True] * G
    for mv in range(moves):
        cnt = s.counts()
        for gi in range(G):
            if not live[gi]:
                continue
            ref_cnt, _ = refs[gi].counts(*roots[gi])
            assert np.array_equal(cnt[gi], ref_cnt), (gi, mv)
            own, opp = next_state(*roots[gi], n, _first_max(cnt[gi]))
            roots[gi] = (own, opp)
            live[gi] = legal_mask(own, opp, n) != 0          # (a finished board: the slot idles from here on)
        s.set_roots([r[0] for r in roots], [r[1] for r in roots], [1 if x else 0 for x in live])
        oz.check(s.simulate(net, move_sims))
        for gi in range(G):
            if live[gi]:
                refs[gi].simulate(*roots[gi], move_sims)
        check(("move", mv))
    return refs


@pytest.mark.parametrize("keep", [0, SPARSE], ids=["dense", "sparse"])
@pytest.mark.parametrize("K", [2, 4, 8, 16])
@pytest.mark.parametrize("n", [6, 8])
def test_wide_search_vs_restatement_one_game(oz, n, K, keep):
    refs = _run_vs_restatement(oz, n, K, keep, 1)
    assert refs[0].sims == 2 + 25 + 100 + 3 * 25


def test_wide_search_vs_restatement_64_games(oz):
    refs = _run_vs_restatement(oz, 6, 4, 0, 64)
    assert sum(r.sims for r in refs) > 64 * 127 and sum(r.steps for r in refs) < sum(r.sims for r in refs) // 2


# ------------------------------------------------------------------ 3. independence of the slot and the neighbours
def test_a_game_does_not_depend_on_its_engine(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, sims, K, seed = 6, 20, 4, 41
    out = {}
    for G, first in ((64, 0), (8, 16), (1, 19)):
        net = StubNetWrapper((n, n), 5, 0, max_batch=G * K)
        eng = SelfPlayEngine(net, n, G, sims, 1.0, 1.0, 0.85, seed=seed, first_game_id=first, record_visits=True, leaves_per_step=K)
        rec, vis = eng.play_to_end(with_visits=True)
        st = eng.stats()
        assert st["live_games"] == 0 and st["simulations"] == st["moves"] * sims          # exactly `sims` per move
        assert st["leaves_evaluated"] == st["expansions"]
        out[G] = (rec, vis)
    for G, ids in ((8, range(16, 24)), (1, [19])):
        for gid in ids:
            a, b = out[64][0]["game_id"] == gid, out[G][0]["game_id"] == gid
            assert a.sum() > 0 and out[64][0][a].tobytes() == out[G][0][b].tobytes(), (G, gid)
            assert np.array_equal(out[64][1][a], out[G][1][b]), (G, gid)


# ------------------------------------------------------------------ 4. the lock-step self-play engine
def test_selfplay_engine_visit_rows_vs_restatement(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G, sims, K, seed, first, salt = 6, 8, 30, 4, 77, 300, 21
    net = StubNetWrapper((n, n), salt, 0, max_batch=G * K)
    eng = SelfPlayEngine(net, n, G, sims, 1.0, 0.0, 0.8, seed=seed, first_game_id=first, record_visits=True, leaves_per_step=K)
    rec, vis = eng.play_to_end(with_visits=True)
    assert eng.stats()["live_games"] == 0
    explored = 0
    for gid in range(first, first + G):
        sel = rec["game_id"] == gid
        r, v = rec[sel], vis[sel]
        assert r.size > 0 and np.array_equal(r["ply"], np.arange(r.size))
        W = WideSearch(n, 1.0, K, salt=salt)
        for i in range(r.size):
            b, w, p = int(r["black"][i]), int(r["white"][i]), int(r["player"][i])
            own, opp = (b, w) if p == 1 else (w, b)
            W.simulate(own, opp, sims)
            cnt, lg = W.counts(own, opp)
            assert np.array_equal(v[i], cnt), (gid, i)
            if r["greedy"][i]:
                assert int(r["action"][i]) == W.best_move(own, opp, tie_draw(seed, gid, i)), (gid, i)
            else:
                explored += 1
                assert (lg >> int(r["action"][i])) & 1, (gid, i)
    assert explored > 0


# ------------------------------------------------------------------ 5. the arena
def _replay_arena(r, gi, n, sims, seed, gid, salts, ks):
    """each agent's restatement replays its own plies from the move list"""
    agents = {1: WideSearch(n, 1.0, ks[0], salt=salts[0]), -1: WideSearch(n, 1.0, ks[1], salt=salts[1])}
    black, white = initial_board(n)
    k = int(r["n_moves"][gi])
    for ply in range(k):
        p = int(r["players"][gi][ply])
        own, opp = (black, white) if p == 1 else (white, black)
        assert legal_mask(own, opp, n), (gi, ply)
        W = agents[p]
        W.simulate(own, opp, sims)
        assert int(r["actions"][gi][ply]) == W.best_move(own, opp, tie_draw(seed, gid, ply)), (gi, ply, ks)
        own, opp = apply_move(own, opp, n, int(r["actions"][gi][ply]))
        black, white = (own, opp) if p == 1 else (opp, own)
    assert legal_mask(black, white, n) == 0 and legal_mask(white, black, n) == 0
    assert (int(r["final_black"][gi]), int(r["final_white"][gi])) == (black, white)
    assert int(r["winner"][gi]) == (1 if popcount(black) >= popcount(white) else -1)


@pytest.mark.parametrize("ks", [(4, 4), (1, 4)])
def test_arena_vs_restatement(oz, ks):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.agents import arena_batch
    n, G, sims, seed, first = 6, 16, 50, 7, 900
    na, nb = StubNetWrapper((n, n), 41, 0, max_batch=G * ks[0]), StubNetWrapper((n, n), 42, 0, max_batch=G * ks[1])
    r = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=1, leaves_per_step=ks)
    for gi in range(G):
        _replay_arena(r, gi, n, sims, seed, first + gi, (41, 42), ks)
    moves = int(r["n_moves"].sum())
    assert int(r["stats_black"][0] + r["stats_white"][0]) == moves * sims


def test_arena_k11_through_the_setter_is_todays_arena(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.agents import arena_batch
    n, G, sims = 6, 16, 50
    na, nb = StubNetWrapper((n, n), 41, 0, max_batch=G), StubNetWrapper((n, n), 42, 0, max_batch=G)
    a = arena_batch(na, nb, n, G, sims, 1.0, seed=7, first_game_id=900, q_mode=0)
    b = arena_batch(na, nb, n, G, sims, 1.0, seed=7, first_game_id=900, q_mode=0, leaves_per_step=(1, 1))
    for key in ("winner", "points", "n_moves", "actions", "players", "final_black", "final_white", "stats_black", "stats_white"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["leaves_evaluated"] == b["leaves_evaluated"]


# ------------------------------------------------------------------ 6. a real network
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_wide_search_with_real_network_vs_restatement(oz, precision):
    """128 games, K = 4, three plies with the table kept: the tables of 4 sampled games == the restatement fed the GPU network's own
    (pi, v) for those boards (so rounding in the network cannot excuse a divergent table)"""
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.weights import init_weights
    n, G, K, sims, C_ = 6, 128, 4, 24, 256
    w = init_weights(n, seed=2, channels=C_, randomize_all=True)
    for i in (36, 38):
        w[i] = w[i] * 4.0
    net = NNetWrapper((n, n), num_channels_1=C_, max_batch=G * K, weights=w, precision=precision)
    cache = {}

    def ev(own, opp, nn):
        # (a batch of the capacity the search launches the network for, so that nothing about the launch differs)
        if (own, opp) not in cache:
            p, v = net.predict_batch([own] * (G * K), [opp] * (G * K))
            cache[(own, opp)] = (p[0].ravel(), float(v[0]))
        return cache[(own, opp)]

    base = _golden_roots(n, 64)
    roots = [base[i % 64] for i in range(G)]
    sampled = (0, 37, 90, 127)
    refs = {gi: WideSearch(n, 1.0, K, evaluator=ev) for gi in sampled}
    s = Search(oz, n, G)
    oz.check(s.set_k(K))
    live = [True] * G
    for ply in range(3):
        s.set_roots([r[0] for r in roots], [r[1] for r in roots], [1 if x else 0 for x in live])
        oz.check(s.simulate(net, sims))
        for gi in sampled:
            if live[gi]:
                refs[gi].simulate(*roots[gi], sims)
            assert_same_tables(s.dump(gi), refs[gi], (precision, gi, ply))
        cnt = s.counts()
        for gi in range(G):
            if live[gi]:
                roots[gi] = next_state(*roots[gi], n, _first_max(cnt[gi]))
                live[gi] = legal_mask(*roots[gi], n) != 0
    st = s.stats()
    assert st[0] >= 100 * 3 * sims and s.wide_stats()[2] == st[2]
    oz.check(oz.load().oz_net_check(net._h))


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_objects_usable(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    n, G = 6, 4
    small, big = StubNetWrapper((n, n), 3, 0, max_batch=G), StubNetWrapper((n, n), 3, 0, max_batch=G * 16)
    roots = _golden_roots(n, G)
    s = Search(oz, n, G)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    for bad in (0, -1, 17):
        assert s.set_k(bad) == oz.OZ_ERR_ARG and "leaves_per_step" in lib.oz_last_error().decode()
    assert s.get_k() == 1
    # a network that is too small
    oz.check(s.set_k(4))
    assert s.simulate(small, 5) == oz.OZ_ERR_ARG and "max_batch" in lib.oz_last_error().decode()
    # the host-evaluator split
    status, lo, lp = np.zeros(G, np.int32), np.zeros(G, np.uint64), np.zeros(G, np.uint64)
    pi, v = np.zeros((G, n * n), np.float32), np.zeros(G, np.float32)
    assert lib.oz_mcts_select(s.h) == oz.OZ_ERR_STATE and "leaves_per_step" in lib.oz_last_error().decode()
    assert lib.oz_mcts_leaves(s.h, oz.p_i32(status), oz.p_u64(lo), oz.p_u64(lp)) == oz.OZ_ERR_STATE
    assert lib.oz_mcts_backup(s.h, oz.p_f32(pi), oz.p_f32(v)) == oz.OZ_ERR_STATE
    # a change while a step is pending
    oz.check(s.set_k(1))
    oz.check(lib.oz_mcts_select(s.h))
    assert s.set_k(4) == oz.OZ_ERR_STATE and "pending" in lib.oz_last_error().decode()
    assert lib.oz_mcts_use_wide_kernels(s.h, 1) == oz.OZ_ERR_STATE
    oz.check(lib.oz_mcts_leaves(s.h, oz.p_i32(status), oz.p_u64(lo), oz.p_u64(lp)))
    for gi in range(G):
        p, val = oracle.stub_predict(int(lo[gi]), int(lp[gi]), n, 3, 0)
        pi[gi], v[gi] = p.ravel(), val
    oz.check(lib.oz_mcts_backup(s.h, oz.p_f32(pi), oz.p_f32(v)))
    # ... and the object is usable at K = 1: the same tables as a fresh search
    oz.check(s.simulate(small, 20))
    t = Search(oz, n, G)
    t.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(t.simulate(small, 21))
    for gi in range(G):
        a, b = s.dump(gi), t.dump(gi)
        assert len(a) == len(b) and all(x["Ns"] == y["Ns"] and np.array_equal(x["Q"], y["Q"]) and np.array_equal(x["N"], y["N"]) for x, y in zip(a, b))
    # the engines
    eng = SelfPlayEngine(small, n, G, 10, leaves_per_step=1)
    assert lib.oz_selfplay_set_leaves_per_step(eng._h, 4) == oz.OZ_ERR_ARG and "max_batch" in lib.oz_last_error().decode()
    assert lib.oz_selfplay_set_leaves_per_step(eng._h, 17) == oz.OZ_ERR_ARG
    eng.run(1)
    assert lib.oz_selfplay_set_leaves_per_step(eng._h, 1) == oz.OZ_ERR_STATE
    eng.run_steps(3)                                       # K = 1: the free-running driver still works
    wide = SelfPlayEngine(big, n, G, 10, leaves_per_step=4)
    with pytest.raises(oz.OzError) as ei:
        wide.run_steps(1)
    assert ei.value.code == oz.OZ_ERR_STATE and "free-running" in str(ei.value)
    wide.run(2)
    assert wide.stats()["simulations"] == 2 * G * 10
    # the arena
    h = C.c_void_p()
    oz.check(lib.oz_arena_create(C.byref(h), n, G, 10, 1.0, 1, 1, 0, small._h, big._h, 0))
    try:
        assert lib.oz_arena_set_leaves_per_step(h, 2, 2) == oz.OZ_ERR_ARG and "max_batch" in lib.oz_last_error().decode()
        assert lib.oz_arena_set_leaves_per_step(h, 1, 0) == oz.OZ_ERR_ARG
        oz.check(lib.oz_arena_set_leaves_per_step(h, 1, 4))
        oz.check(lib.oz_arena_run_rounds(h, 2))
        assert lib.oz_arena_set_leaves_per_step(h, 1, 1) == oz.OZ_ERR_STATE
    finally:
        lib.oz_arena_destroy(h)
    # the Python mirror: a host-side (duck-typed) network cannot take K > 1
    from othellozero_amd.othelo_mcts import OthelloMCTS

    class HostNet:
        network_type = None

        def predict(self, board):
            raise AssertionError("not reached")
    with pytest.raises(ValueError):
        OthelloMCTS(n, HostNet(), 1.0, leaves_per_step=4)


def test_capacity_overflow_through_the_wide_kernels(oz):
    """the wide counterpart of test_gpu_parity.py's capacity error: a full node table ends the simulate call with the clean error code"""
    from othellozero_amd.NNet import StubNetWrapper
    lib = oz.load()
    n, G, K = 6, 8, 4
    roots = _golden_roots(n, G)
    net = StubNetWrapper((n, n), 13, 0, max_batch=G * K)
    s = Search(oz, n, G, node_cap=16)
    oz.check(s.set_k(K))
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    assert s.simulate(net, 40) == oz.OZ_ERR_CAPACITY and "node table" in lib.oz_last_error().decode()
    h, s.h = s.h, C.c_void_p()
    assert lib.oz_mcts_destroy(h) == oz.OZ_OK


# ------------------------------------------------------------------ 8. the drop-in episode
def test_execute_episode_dropin_with_leaves_per_step(oz):
    from othellozero_amd import training
    from othellozero_amd.NNet import StubNetWrapper
    n, sims, K, salt = 6, 25, 4, 17
    net = StubNetWrapper((n, n), salt, 0, max_batch=K)
    ex = training.execute_episode(n, net, 1.0, sims, 1, 1.0, snapshot_boards=True, leaves_per_step=K)
    # e_greedy = 1: every move is the first max-count square; entry 7 of every group of 8 is the unrotated example
    W = WideSearch(n, 1.0, K, salt=salt)
    black, white = initial_board(n)
    player, ply = 1, 0
    while True:
        own, opp = (black, white) if player == 1 else (white, black)
        if legal_mask(own, opp, n) == 0:
            if legal_mask(opp, own, n) == 0:
                break
            player = -player
            continue
        W.simulate(own, opp, sims)
        cnt, _ = W.counts(own, opp)
        sq = _first_max(cnt)
        board, policy, _z = ex[8 * ply + 7]
        assert oracle.pack_board(board) == (black, white), ply
        r, c = np.argwhere(policy == 1.0)[0]
        assert int(r) * 8 + int(c) == sq, ply
        own, opp = apply_move(own, opp, n, sq)
        black, white = (own, opp) if player == 1 else (opp, own)
        player = -player
        ply += 1
    assert len(ex) == 8 * ply
