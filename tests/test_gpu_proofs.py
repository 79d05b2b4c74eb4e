"""Proofs of the search on the GPU (pytest -m gpu): the proven instantiations of the tree kernels against the restatement in
tests/proofs_ref.py (ProvenSearch), bit for bit -- tables, last values, root counts and the proof of every edge and node; the bare search
at K = 1 and K = 4, one game and 64 games in one object, solved leaves, the self-play engine through run(), the arena with the option on one
agent -- and the option off against an object that was never given it, the setter's rule and the refusals.  Stub network and q_mode F64."""
import ctypes as C
import functools

import numpy as np
import pytest

import solve_leaves_ref as SL
from move_sampling_ref import selfplay_move
from proofs_ref import DRAW_POSITION, STATS, ProvenSearch, episode, replay_arena_game
from root_noise_ref import dirichlet
from value_signs_ref import POSITIONS_6, SoundSearch
from wide_search_ref import assert_same_tables, initial_board, legal_mask, popcount

pytestmark = pytest.mark.gpu

REFERENCE, SOUND = 0, 1
SALT6 = 7
# (n, own, opp, simulations, stub salt): the case set of tests/test_gpu_value_signs.py and the position whose root is proven a draw
CASES = [(4, *initial_board(4), sims, salt) for sims in (100, 200) for salt in (3, 11)] + [(6, own, opp, 60, SALT6) for own, opp in POSITIONS_6]
DRAW_CASE = (6, *DRAW_POSITION, 120, SALT6)


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@functools.lru_cache(maxsize=None)
def proven(n, own, opp, sims, salt, K, solve=0):
    """the restatement's search of one case, computed once and shared (read only)"""
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    s = ProvenSearch(n, 1.0, K, salt=salt, evaluator=ev, solve=solve)
    s.simulate(own, opp, sims)
    return s


@functools.lru_cache(maxsize=None)
def sound(n, own, opp, sims, salt, K):
    s = SoundSearch(n, 1.0, K, salt=salt)
    s.simulate(own, opp, sims)
    return s


def same_proofs(dump, ref, where, oz):
    """dump: per node dict(edge int8 [64], value, val) as oz_mcts_dump_proofs gives them; ref: a ProvenSearch"""
    U = oz.PROOF_UNKNOWN
    assert len(dump) == len(ref.nodes), where
    for i, (d, nd) in enumerate(zip(dump, ref.nodes)):
        want = [ref.edge[i].get(s, U) for s in range(64)]
        assert [int(x) for x in d["edge"]] == want, (where, i)
        assert d["value"] == (U if ref.own[i] is None else ref.own[i]), (where, i)
        v = ref.val(i)
        assert d["val"] == (U if v is None else v), (where, i)


class Search:
    """a bare oz_mcts with G slots"""

    def __init__(self, oz, n, G, node_cap=1024, signs=SOUND, proofs=1, K=1):
        self.oz, self.lib, self.n, self.G = oz, oz.load(), n, G
        self.h = C.c_void_p()
        oz.check(self.lib.oz_mcts_create(C.byref(self.h), n, G, node_cap, 1.0, oz.QMODE_F64))
        if signs is not None:
            oz.check(self.lib.oz_mcts_set_value_signs(self.h, signs))
        if proofs is not None:
            oz.check(self.lib.oz_mcts_set_proofs(self.h, proofs))
        if K != 1:
            oz.check(self.lib.oz_mcts_set_leaves_per_step(self.h, K))

    def __del__(self):
        if self.h:
            self.lib.oz_mcts_destroy(self.h)
            self.h = C.c_void_p()

    def set_roots(self, roots, active=None):
        a, b = np.array([r[0] for r in roots], np.uint64), np.array([r[1] for r in roots], np.uint64)
        act = None if active is None else self.oz.p_u8(np.array(active, np.uint8))
        self.oz.check(self.lib.oz_mcts_set_roots(self.h, self.oz.p_u64(a), self.oz.p_u64(b), act))

    def simulate(self, net, nsims):
        self.oz.check(self.lib.oz_mcts_simulate(self.h, net._h, int(nsims)))

    def num_nodes(self):
        nn = np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_num_nodes(self.h, self.oz.p_i32(nn)))
        return nn

    def dump(self, g):
        out = []
        for i in range(int(self.num_nodes()[g])):
            own, opp, legal, Ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
            N, Q, qt, P = np.zeros(64, np.int32), np.zeros(64, np.float64), np.zeros(64, np.uint8), np.zeros(64, np.float64)
            self.oz.check(self.lib.oz_mcts_dump_node(self.h, g, i, C.byref(own), C.byref(opp), C.byref(Ns), C.byref(legal),
                                                     self.oz.p_i32(N), self.oz.p_f64(Q), self.oz.p_u8(qt), self.oz.p_f64(P)))
            out.append(dict(k0=own.value, k1=opp.value, Ns=Ns.value, legal=legal.value, N=N, Q=Q, qtag=qt, P=P))
        return out

    def dump_proofs(self, g):
        out = []
        for i in range(int(self.num_nodes()[g])):
            edge, value, val = np.zeros(64, np.int8), C.c_int8(), C.c_int8()
            self.oz.check(self.lib.oz_mcts_dump_proofs(self.h, g, i, self.oz.p_i8(edge), C.byref(value), C.byref(val)))
            out.append(dict(edge=edge, value=value.value, val=val.value))
        return out

    def last_values(self):
        v = np.zeros(self.G, np.float64)
        self.oz.check(self.lib.oz_mcts_last_value(self.h, self.oz.p_f64(v), None, None))
        return v

    def counts(self):
        cnt, legal, rc = np.zeros((self.G, 64), np.int32), np.zeros(self.G, np.uint64), np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_root_counts(self.h, self.oz.p_i32(cnt), self.oz.p_u64(legal), self.oz.p_i32(rc)))
        return cnt

    def root_proofs(self):
        edge, val, rc = np.zeros((self.G, 64), np.int8), np.zeros(self.G, np.int8), np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_root_proofs(self.h, self.oz.p_i8(edge), self.oz.p_i8(val), self.oz.p_i32(rc)))
        return edge, val, rc

    def proof_stats(self):
        s = np.zeros(4, np.int64)
        self.oz.check(self.lib.oz_mcts_proof_stats(self.h, self.oz.p_i64(s)))
        return [int(x) for x in s]

    def proofs(self):
        on = C.c_int(-1)
        self.oz.check(self.lib.oz_mcts_get_proofs(self.h, C.byref(on)))
        return on.value

    def signs(self):
        mode = C.c_int(-1)
        self.oz.check(self.lib.oz_mcts_get_value_signs(self.h, C.byref(mode)))
        return mode.value


def check_slot(oz, s, g, ref, own, opp, last, cnt, rp, where):
    assert_same_tables(s.dump(g), ref, where)
    same_proofs(s.dump_proofs(g), ref, where, oz)
    assert last[g] == ref.last_value, where
    assert np.array_equal(cnt[g], ref.counts(own, opp)[0]), where
    val, edge = ref.root_proof(own, opp)
    assert rp[2][g] == 0 and rp[1][g] == (oz.PROOF_UNKNOWN if val is None else val), where
    assert [int(x) for x in rp[0][g]] == [edge.get(sq, oz.PROOF_UNKNOWN) for sq in range(64)], where


# ------------------------------------------------------------------ 1. the drop-in search, one game
@pytest.mark.parametrize("K", [1, 4])
def test_othello_mcts_vs_restatement(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    roots_proven = 0
    for n, own, opp, sims, salt in CASES + [DRAW_CASE]:
        net = StubNetWrapper((n, n), salt, 0, max_batch=K)
        m = OthelloMCTS(n, net, 1.0, q_mode=oz.QMODE_F64, node_cap=1024, leaves_per_step=K, value_signs="sound", proofs=True)
        assert m.proofs is True and m.value_signs == "sound"
        board = oz.unpack_board(own, opp, n)
        last = m.simulate_n(board, OthelloPlayer.BLACK, sims)
        ref = proven(n, own, opp, sims, salt, K)
        where = (n, sims, salt, K)
        dump = m.dump()
        assert_same_tables(dump, ref, where)
        assert float(last) == ref.last_value, (where, last, ref.last_value)
        assert np.array_equal(m._counts(board)[1], ref.counts(own, opp)[0]), where
        same_proofs([d["proofs"] for d in dump], ref, where, oz)
        same_proofs(m.dump_proofs(), ref, where, oz)
        val, edge = m.root_proof(board)
        want_val, want_edge = ref.root_proof(own, opp)
        assert val == want_val and [int(x) for x in edge] == [want_edge.get(sq, oz.PROOF_UNKNOWN) for sq in range(64)], where
        assert list(m.proof_stats().values()) == ref.stats() and tuple(m.proof_stats()) == STATS, where
        roots_proven += val is not None
        if (n, own, opp) == DRAW_CASE[:3]:
            assert val == 0
    assert roots_proven >= 2


# ------------------------------------------------------------------ 2. 64 games in one object
@pytest.mark.parametrize("K", [1, 4])
def test_64_games_in_one_object(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims = 6, 64, 60
    roots = [POSITIONS_6[g % len(POSITIONS_6)] for g in range(G)]
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * K)
    s = Search(oz, n, G, K=K)
    assert s.signs() == SOUND and s.proofs() == 1          # (the third instantiation is internal: the signs read back as sound)
    s.set_roots(roots)
    s.simulate(net, sims)
    last, cnt, rp = s.last_values(), s.counts(), s.root_proofs()
    total = [0, 0, 0, 0]
    for g in range(G):
        ref = proven(n, *roots[g], sims, SALT6, K)
        if g < 8 or g >= G - 4:
            check_slot(oz, s, g, ref, *roots[g], last, cnt, rp, (K, g))
        else:                                              # (every slot's tables and last value; the node-by-node proof dump on twelve of them)
            assert_same_tables(s.dump(g), ref, (K, g))
            assert last[g] == ref.last_value and np.array_equal(cnt[g], ref.counts(*roots[g])[0]), (K, g)
        total = [a + b for a, b in zip(total, ref.stats())]
    assert s.proof_stats() == total and total[0] > 0 and total[1] > 0, (s.proof_stats(), total)
    # the 4x4 start, where the passes are, in an object of 64 slots too (two salts: two objects)
    b4 = initial_board(4)
    for salt in (3, 11):
        t = Search(oz, 4, G, K=K)
        t.set_roots([b4] * G)
        t.simulate(StubNetWrapper((4, 4), salt, 0, max_batch=G * K), 100)
        ref = proven(4, *b4, 100, salt, K)
        last, cnt, rp = t.last_values(), t.counts(), t.root_proofs()
        for g in (0, 31, 63):
            check_slot(oz, t, g, ref, *b4, last, cnt, rp, (4, salt, K, g))
        assert t.proof_stats() == [G * x for x in ref.stats()]


# ------------------------------------------------------------------ 3. solved leaves: the nodes' own values
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("E", [4, 6])
def test_solved_leaves_vs_restatement(oz, K, E):
    from othellozero_amd.NNet import StubNetWrapper
    n, sims = 6, 60
    roots = list(POSITIONS_6) + [DRAW_POSITION]
    G = len(roots)
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * K)
    s = Search(oz, n, G, K=K)
    oz.check(s.lib.oz_mcts_set_solve_leaves(s.h, E))
    s.set_roots(roots)
    s.simulate(net, sims)
    last, cnt, rp = s.last_values(), s.counts(), s.root_proofs()
    own_nodes, total = 0, [0, 0, 0, 0]
    for g, (own, opp) in enumerate(roots):
        ref = proven(n, own, opp, sims, SALT6, K, E)
        check_slot(oz, s, g, ref, own, opp, last, cnt, rp, (K, E, g))
        assert sum(d["value"] != oz.PROOF_UNKNOWN for d in s.dump_proofs(g)) == ref.own_nodes, (K, E, g)
        own_nodes += ref.own_nodes
        total = [a + b for a, b in zip(total, ref.stats())]
    assert own_nodes > 0 and s.proof_stats() == total
    # the 4x4 start: 12 empties, so the solved leaves come late in the tree
    b4 = initial_board(4)
    t = Search(oz, 4, 1, K=K)
    oz.check(t.lib.oz_mcts_set_solve_leaves(t.h, E))
    t.set_roots([b4])
    t.simulate(StubNetWrapper((4, 4), 3, 0, max_batch=K), 200)
    ref = proven(4, *b4, 200, 3, K, E)
    check_slot(oz, t, 0, ref, *b4, t.last_values(), t.counts(), t.root_proofs(), (4, K, E))
    assert ref.own_nodes > 0


# ------------------------------------------------------------------ 4. the self-play engine
def _engine(net, K, **kw):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, 6, 8, 12, 1.0, 1.0, 0.8, seed=77, first_game_id=300, record_visits=True, record_values=True,
                          leaves_per_step=K, value_signs="sound", proofs=True, **kw)


@pytest.mark.parametrize("K", [1, 4])
def test_selfplay_engine_vs_restatement(oz, K):
    """8 games of 6x6 at 12 simulations played to the end through run(): moves, records, visit rows and root values, bit for bit"""
    from othellozero_amd.NNet import StubNetWrapper
    net = StubNetWrapper((6, 6), 21, 0, max_batch=8 * K)
    eng = _engine(net, K)
    eng.play_to_end()
    assert eng.stats()["live_games"] == 0
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    total = [0, 0, 0, 0]
    for gid in range(300, 308):
        sel = rec["game_id"] == gid
        r, v, q = rec[sel], vis[sel], val[sel]
        W = ProvenSearch(6, 1.0, K, salt=21)
        want = episode(W, 6, 12, 77, gid, 0.8)
        assert r.size == len(want) > 0, gid
        for i, w in enumerate(want):
            got = tuple(int(r[k][i]) for k in ("black", "white", "player", "ply", "action", "greedy"))
            assert got == (w["black"], w["white"], w["player"], w["ply"], w["action"], w["greedy"]), (gid, i)
            assert np.array_equal(v[i], w["counts"]), (gid, i)
            assert q[i] == w["value"], (gid, i, q[i], w["value"])
        fb, fw = int(r["final_black"][0]), int(r["final_white"][0])
        assert legal_mask(fb, fw, 6) == 0 and legal_mask(fw, fb, 6) == 0
        assert all(int(r["z"][i]) == (1 if popcount(fb) >= popcount(fw) else -1) * int(r["player"][i]) for i in range(r.size)), gid
        assert not W.corrupt
        total = [a + b for a, b in zip(total, W.stats())]
    print("K =", K, dict(zip(STATS, total)))
    assert total[3] >= 1 and total[1] >= 1                 # the games proved roots, and descents ended on proofs
    assert list(eng.proof_stats().values()) == total, (eng.proof_stats(), total)
    # ... and they are not the games of the sound search without proofs
    from othellozero_amd.training import SelfPlayEngine
    plain = SelfPlayEngine(net, 6, 8, 12, 1.0, 1.0, 0.8, seed=77, first_game_id=300, record_visits=True, record_values=True,
                           leaves_per_step=K, value_signs="sound")
    plain.play_to_end()
    assert plain.records(with_visits=True)[1].tobytes() != vis.tobytes()
    assert list(plain.proof_stats().values()) == [0, 0, 0, 0]


def test_selfplay_engine_with_root_noise_and_move_sampling(oz):
    """round by round: the device's own eta (held against root_noise_ref.dirichlet) goes into the restatement, whose counts and root values
    must then agree exactly; the move is move_sampling_ref's"""
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims, seed, first, salt, alpha, eps, sample = 6, 8, 12, 77, 300, 21, 0.5, 0.25, (1.0, 6)
    net = StubNetWrapper((n, n), salt, 0, max_batch=G)
    eng = _engine(net, 1, root_noise=(alpha, eps), sample_moves=sample)
    W = [ProvenSearch(n, 1.0, 1, salt=salt) for _ in range(G)]
    searched = sampled = 0
    for rnd in range(n * n):
        st = eng.state()
        if st["finished"].all():
            break
        eng.run(1)
        eta, armed = eng.last_root_noise()
        cnt, after = eng.last_counts(), eng.state()
        for g in range(G):
            if st["finished"][g]:
                continue
            b, w, p, ply, gid = int(st["black"][g]), int(st["white"][g]), int(st["player"][g]), int(st["ply"][g]), int(st["game_id"][g])
            own, opp = (b, w) if p == 1 else (w, b)
            lg = legal_mask(own, opp, n)
            assert armed[g] and np.abs(eta[g] - dirichlet(n, lg, alpha, seed, gid, ply)[0]).max() <= 1e-9, (rnd, g)
            W[g].set_noise(own, opp, eta[g], eps)
            W[g].simulate(own, opp, sims)
            assert np.array_equal(cnt[g], W[g].counts(own, opp)[0]), (rnd, g)
            action, greedy, margin = selfplay_move(cnt[g], lg, 0.8, seed, gid, ply, sample)
            placed = (int(after["black"][g]) | int(after["white"][g])) & ~(b | w)
            if margin >= 1e-9:
                assert placed == 1 << action, (rnd, g, greedy)
            searched += 1
            sampled += greedy == 2
    assert eng.stats()["live_games"] == 0 and searched == eng.stats()["moves"] and sampled >= G
    rec, val = eng.records(with_values=True)
    for g in range(G):                                      # the last searched root of every game: its recorded value is the restatement's
        r = rec[rec["game_id"] == first + g][-1]
        own, opp = (int(r["black"]), int(r["white"])) if r["player"] == 1 else (int(r["white"]), int(r["black"]))
        assert val[rec["game_id"] == first + g][-1] == W[g].root_value(own, opp), g
    total = [sum(x) for x in zip(*(w.stats() for w in W))]
    assert total[3] >= 1 and list(eng.proof_stats().values()) == total


# ------------------------------------------------------------------ 5. the arena: the option on one agent
def test_arena_with_proofs_on_one_agent(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.agents import arena_batch
    n, G, sims, seed, first = 6, 8, 25, 7, 900
    na, nb = StubNetWrapper((n, n), 41, 0, max_batch=G), StubNetWrapper((n, n), 42, 0, max_batch=G)
    r = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, value_signs="sound", proofs=(True, False))
    stops = 0
    for gi in range(G):
        agents = {1: ProvenSearch(n, 1.0, 1, salt=41), -1: SoundSearch(n, 1.0, 1, salt=42)}
        replay_arena_game(r, gi, n, sims, seed, first + gi, agents)
        stops += agents[1].edge_stops + agents[1].node_stops
    assert stops >= 1
    both = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, value_signs="sound", proofs=True)
    for gi in range(G):
        replay_arena_game(both, gi, n, sims, seed, first + gi, {1: ProvenSearch(n, 1.0, 1, salt=41), -1: ProvenSearch(n, 1.0, 1, salt=42)})


# ------------------------------------------------------------------ 6. off is off, the setter's rule and the refusals
def _same_dumps(a, b, where):
    assert len(a) == len(b), where
    for x, y in zip(a, b):
        assert (x["k0"], x["k1"], x["Ns"], x["legal"]) == (y["k0"], y["k1"], y["Ns"], y["legal"]), where
        for key in ("N", "Q", "qtag", "P"):
            assert np.array_equal(x[key], y[key]), (where, key)


def test_off_through_the_setter_is_the_search_without_the_option(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    n, G, sims = 6, len(POSITIONS_6), 60
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * 4)
    for K in (1, 4):
        a, b = Search(oz, n, G, proofs=None, K=K), Search(oz, n, G, proofs=0, K=K)
        assert a.proofs() == b.proofs() == 0 and a.proof_stats() == [0, 0, 0, 0]
        for s in (a, b):
            s.set_roots(list(POSITIONS_6))
            s.simulate(net, sims)
        for g in range(G):
            _same_dumps(a.dump(g), b.dump(g), (K, g))
            assert_same_tables(a.dump(g), sound(n, *POSITIONS_6[g], sims, SALT6, K), (K, g))
        assert a.last_values().tobytes() == b.last_values().tobytes()
        edge, val = np.zeros(64, np.int8), C.c_int8()
        assert lib.oz_mcts_dump_proofs(b.h, 0, 0, oz.p_i8(edge), C.byref(val), C.byref(val)) == oz.OZ_ERR_STATE
        # a used tree keeps its rule: the setter refuses and the object goes on as before
        for on in (1, 0):
            assert lib.oz_mcts_set_proofs(b.h, on) == oz.OZ_ERR_STATE and "oz_mcts_reset" in lib.oz_last_error().decode()
        assert lib.oz_mcts_set_value_signs(b.h, 2) == oz.OZ_ERR_ARG
        assert b.proofs() == 0 and b.signs() == SOUND
        for s in (a, b):
            s.simulate(net, 20)
        for g in range(G):
            _same_dumps(a.dump(g), b.dump(g), (K, g, "after the refusal"))
        # an emptied tree takes the option, and a tree with proofs that is emptied holds none
        for again in range(2):
            oz.check(lib.oz_mcts_reset(b.h, -1))
            assert not b.num_nodes().any()
            oz.check(lib.oz_mcts_set_proofs(b.h, 1))
            b.set_roots(list(POSITIONS_6))
            assert (b.root_proofs()[2] == 1).all() and (b.root_proofs()[1] == oz.PROOF_UNKNOWN).all()
            b.simulate(net, sims)
            for g in range(G):
                ref = proven(n, *POSITIONS_6[g], sims, SALT6, K)
                assert_same_tables(b.dump(g), ref, (K, g, "after the reset", again))
                same_proofs(b.dump_proofs(g), ref, (K, g, "after the reset", again), oz)
        # ... one game's tree alone: the slot's nodes are searched again from nothing, with nothing inherited
        oz.check(lib.oz_mcts_reset(b.h, 2))
        b.set_roots(list(POSITIONS_6), [0, 0, 1, 0])
        b.simulate(net, sims)
        same_proofs(b.dump_proofs(2), proven(n, *POSITIONS_6[2], sims, SALT6, K), (K, "slot 2 again"), oz)
    # the engine: proofs off by name plays the bytes of the sound engine without the option
    kw = dict(seed=5, first_game_id=40, record_visits=True, record_values=True, value_signs="sound")
    for K in (1, 4):
        x, y = SelfPlayEngine(net, n, 4, 12, leaves_per_step=K, **kw), SelfPlayEngine(net, n, 4, 12, leaves_per_step=K, proofs=False, **kw)
        oz.check(lib.oz_selfplay_set_proofs(y._h, 0))
        for e in (x, y):
            e.play_to_end()
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x.records(with_visits=True, with_values=True), y.records(with_visits=True, with_values=True)))
        assert lib.oz_selfplay_set_proofs(y._h, 1) == oz.OZ_ERR_STATE and "before the first driver call" in lib.oz_last_error().decode()


def test_refusals_leave_the_object_usable(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    n, G, sims = 6, len(POSITIONS_6), 60
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G)
    ids, plies = np.arange(G, dtype=np.uint64), np.zeros(G, np.int32)

    def err():
        return lib.oz_last_error().decode()

    def runs_as(s, ref_of):
        s.set_roots(list(POSITIONS_6))
        s.simulate(net, sims)
        for g in range(G):
            assert_same_tables(s.dump(g), ref_of(g), g)
    # reference signs: proofs are an error, and the object stays the reference search
    s = Search(oz, n, G, signs=None, proofs=None)
    assert lib.oz_mcts_set_proofs(s.h, 1) == oz.OZ_ERR_STATE and "sound" in err()
    assert s.proofs() == 0 and s.signs() == REFERENCE
    s.set_roots(list(POSITIONS_6))
    s.simulate(net, sims)
    # proofs first: the Gumbel search, forced playouts and the reference signs are refused, and the object stays the proven search
    s = Search(oz, n, G)
    assert lib.oz_mcts_set_gumbel(s.h, 4, 50.0, 1.0, 1, None, None) == oz.OZ_ERR_STATE and "proofs" in err()
    assert lib.oz_mcts_set_forced_playouts(s.h, 2.0) == oz.OZ_ERR_STATE and "proofs" in err()
    assert lib.oz_mcts_set_value_signs(s.h, REFERENCE) == oz.OZ_ERR_STATE and "proofs" in err()
    assert s.proofs() == 1 and s.signs() == SOUND
    runs_as(s, lambda g: proven(n, *POSITIONS_6[g], sims, SALT6, 1))
    # the Gumbel search first: proofs are refused, and the object stays the Gumbel object (unarmed: the sound search)
    s = Search(oz, n, G, proofs=None)
    oz.check(lib.oz_mcts_set_gumbel(s.h, 4, 50.0, 1.0, 1, None, None))
    assert lib.oz_mcts_set_proofs(s.h, 1) == oz.OZ_ERR_STATE and "Gumbel" in err()
    assert s.proofs() == 0
    runs_as(s, lambda g: sound(n, *POSITIONS_6[g], sims, SALT6, 1))
    # forced playouts first (they need armed noise): proofs are refused
    s = Search(oz, n, G, proofs=None)
    s.set_roots(list(POSITIONS_6))
    oz.check(lib.oz_mcts_sample_root_noise(s.h, 0.5, 0.25, 9, oz.p_u64(ids), oz.p_i32(plies)))
    oz.check(lib.oz_mcts_set_forced_playouts(s.h, 2.0))
    assert lib.oz_mcts_set_proofs(s.h, 1) == oz.OZ_ERR_STATE and "forced" in err()
    oz.check(lib.oz_mcts_set_forced_playouts(s.h, 0.0))
    oz.check(lib.oz_mcts_set_proofs(s.h, 1))               # ... and accepted once they are off
    s.simulate(net, sims)
    # the engine: the free-running driver and stagger refuse, run() goes on
    eng = SelfPlayEngine(net, n, G, 12, seed=5, first_game_id=40, value_signs="sound", proofs=True, refill=True)
    assert lib.oz_selfplay_run_steps(eng._h, 1) == oz.OZ_ERR_STATE and "proofs" in err()
    assert lib.oz_selfplay_stagger(eng._h, 4) == oz.OZ_ERR_STATE and "proofs" in err()
    assert lib.oz_selfplay_set_gumbel(eng._h, 4, 50.0, 1.0) == oz.OZ_ERR_STATE and "proofs" in err()
    eng.run(2)
    assert eng.stats()["moves"] == 2 * G
    assert lib.oz_selfplay_run_steps(eng._h, 1) == oz.OZ_ERR_STATE
    # the arena: per agent, before the first run; an agent with reference signs cannot take proofs
    h = C.c_void_p()
    oz.check(lib.oz_arena_create(C.byref(h), n, 4, 10, 1.0, oz.QMODE_F64, 1, 0, net._h, net._h, 0))
    try:
        oz.check(lib.oz_arena_set_value_signs(h, SOUND, REFERENCE))
        assert lib.oz_arena_set_proofs(h, 1, 1) == oz.OZ_ERR_STATE and "sound" in err()
        oz.check(lib.oz_arena_set_proofs(h, 1, 0))
        oz.check(lib.oz_arena_run_rounds(h, 2))
        assert lib.oz_arena_set_proofs(h, 0, 0) == oz.OZ_ERR_STATE
    finally:
        lib.oz_arena_destroy(h)


# ------------------------------------------------------------------ 7. loop.training: one setting for self-play, the match and the evaluation
@pytest.mark.parametrize("replay", ["host", "device"])
def test_training_loop_passes_the_option_on(oz, tmp_path, monkeypatch, replay):
    from othellozero_amd import loop, training
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    seen = []
    real_engine, real_arena = training.SelfPlayEngine, loop.arena_batch

    class Engine(real_engine):
        def __init__(self, *a, **kw):
            seen.append(("engine", kw.get("value_signs"), kw.get("proofs")))
            super().__init__(*a, **kw)

    def arena(*a, **kw):
        seen.append(("arena", kw.get("value_signs"), kw.get("proofs")))
        return real_arena(*a, **kw)
    monkeypatch.setattr(training, "SelfPlayEngine", Engine)
    monkeypatch.setattr(loop, "arena_batch", arena)
    n = 6
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    kw = dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
              evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0, self_play_training=True, self_play_interval=1,
              self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
              training_buffer_size=8 * 40 * 8, seed=13, alias_final_boards=False, batched_evaluation=True, reference_aliasing=False)
    historic = loop.training(neural_network=net, replay=replay, value_signs="sound", proofs=True, **kw)
    assert len(historic) == 1
    assert [k for k, _, _ in seen].count("engine") == 1 and [k for k, _, _ in seen].count("arena") >= 4      # a match (2 arenas) and two evaluations
    assert all(v == "sound" and p is True for _, v, p in seen), seen
    assert len(loop.training.proof_history) == 1 and tuple(loop.training.proof_history[0]) == STATS
    with pytest.raises(ValueError):
        loop.training(neural_network=net, replay=replay, proofs=True, **kw)
    with pytest.raises(ValueError):
        loop.training(neural_network=net, replay=replay, value_signs="sound", proofs=True, gumbel=True, **kw)
