"""Value signs of the backup on the GPU (pytest -m gpu): the sound instantiations of the tree kernels against the restatement in
tests/value_signs_ref.py (SoundSearch), bit for bit -- the bare search at K = 1 and K = 4, one game and 64 games in one object, the self-play
engine through its drivers, solved leaves, the Gumbel kernels, the arena with one mode per agent and a real network -- and "reference" given
through the setter against an object that was never given the option.  Stub network and q_mode F64 unless a test says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import solve_leaves_ref as SL
from move_sampling_ref import selfplay_move
from root_noise_ref import dirichlet
from value_signs_ref import POSITIONS_6, SoundSearch, episode, replay_arena_game
from wide_search_ref import apply_move, assert_same_tables, initial_board, legal_mask, next_state, popcount

pytestmark = pytest.mark.gpu

REFERENCE, SOUND = 0, 1
SALT6 = 7
# (n, own, opp, simulations, stub salt): the 4x4 start at 100 and 200 simulations under two salts, the 6x6 positions with 8 empties at 60
CASES = [(4, *initial_board(4), sims, salt) for sims in (100, 200) for salt in (3, 11)] + [(6, own, opp, 60, SALT6) for own, opp in POSITIONS_6]


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@functools.lru_cache(maxsize=None)
def restated(n, own, opp, sims, salt, K, mode="sound", solve=0):
    """the restatement's search of one case, computed once and shared (read only)"""
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    s = SoundSearch(n, 1.0, K, salt=salt, evaluator=ev, mode=mode)
    s.simulate(own, opp, sims)
    return s


class Search:
    """a bare oz_mcts with G slots"""

    def __init__(self, oz, n, G, node_cap=1024, signs=None, K=1):
        self.oz, self.lib, self.n, self.G = oz, oz.load(), n, G
        self.h = C.c_void_p()
        oz.check(self.lib.oz_mcts_create(C.byref(self.h), n, G, node_cap, 1.0, oz.QMODE_F64))
        if signs is not None:
            oz.check(self.lib.oz_mcts_set_value_signs(self.h, signs))
        if K != 1:
            oz.check(self.lib.oz_mcts_set_leaves_per_step(self.h, K))

    def __del__(self):
        if self.h:
            self.lib.oz_mcts_destroy(self.h)
            self.h = C.c_void_p()

    def signs(self):
        mode = C.c_int(-1)
        self.oz.check(self.lib.oz_mcts_get_value_signs(self.h, C.byref(mode)))
        return mode.value

    def set_roots(self, roots, active=None):
        a, b = np.array([r[0] for r in roots], np.uint64), np.array([r[1] for r in roots], np.uint64)
        act = None if active is None else self.oz.p_u8(np.array(active, np.uint8))
        self.oz.check(self.lib.oz_mcts_set_roots(self.h, self.oz.p_u64(a), self.oz.p_u64(b), act))

    def simulate(self, net, nsims):
        self.oz.check(self.lib.oz_mcts_simulate(self.h, net._h, int(nsims)))

    def dump(self, g):
        nn = np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_num_nodes(self.h, self.oz.p_i32(nn)))
        out = []
        for i in range(int(nn[g])):
            own, opp, legal, Ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
            N, Q, qt, P = np.zeros(64, np.int32), np.zeros(64, np.float64), np.zeros(64, np.uint8), np.zeros(64, np.float64)
            self.oz.check(self.lib.oz_mcts_dump_node(self.h, g, i, C.byref(own), C.byref(opp), C.byref(Ns), C.byref(legal),
                                                     self.oz.p_i32(N), self.oz.p_f64(Q), self.oz.p_u8(qt), self.oz.p_f64(P)))
            out.append(dict(k0=own.value, k1=opp.value, Ns=Ns.value, legal=legal.value, N=N, Q=Q, qtag=qt, P=P))
        return out

    def last_values(self):
        v = np.zeros(self.G, np.float64)
        self.oz.check(self.lib.oz_mcts_last_value(self.h, self.oz.p_f64(v), None, None))
        return v

    def counts(self):
        cnt, legal, rc = np.zeros((self.G, 64), np.int32), np.zeros(self.G, np.uint64), np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_root_counts(self.h, self.oz.p_i32(cnt), self.oz.p_u64(legal), self.oz.p_i32(rc)))
        return cnt

    def node_values(self, g):
        out = []
        for i in range(len(self.dump(g))):
            v = C.c_double(-9.0)
            self.oz.check(self.lib.oz_mcts_node_value(self.h, g, i, C.byref(v)))
            out.append(v.value)
        return out


def _same_dumps(a, b, where):
    assert len(a) == len(b), where
    for x, y in zip(a, b):
        assert (x["k0"], x["k1"], x["Ns"], x["legal"]) == (y["k0"], y["k1"], y["Ns"], y["legal"]), where
        for key in ("N", "Q", "qtag", "P"):
            assert np.array_equal(x[key], y[key]), (where, key)


# ------------------------------------------------------------------ 0. the case set covers what the option changes
def test_coverage_of_the_case_set():
    """from the restatement's own counters: evaluated leaves backed up across a pass, finished leaves of every value, and root counts that
    differ from reference mode"""
    passes, term, differ = 0, {-1: 0, 0: 0, 1: 0}, 0
    for K in (1, 4):
        for case in CASES:
            s, r = restated(*case, K), restated(*case, K, "reference")
            print(case[0], case[3], case[4], K, "pass backups", s.pass_backups, "finished", s.term)
            passes += s.pass_backups
            for k in term:
                term[k] += s.term[k]
            differ += not np.array_equal(s.counts(case[1], case[2])[0], r.counts(case[1], case[2])[0])
    assert passes >= 1 and min(term.values()) >= 1 and differ >= 1, (passes, term, differ)


# ------------------------------------------------------------------ 1. the drop-in search, one game
@pytest.mark.parametrize("K", [1, 4])
def test_othello_mcts_vs_restatement(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    for n, own, opp, sims, salt in CASES:
        net = StubNetWrapper((n, n), salt, 0, max_batch=K)
        m = OthelloMCTS(n, net, 1.0, q_mode=oz.QMODE_F64, node_cap=1024, leaves_per_step=K, value_signs="sound")
        assert m.value_signs == "sound"
        last = m.simulate_n(oz.unpack_board(own, opp, n), OthelloPlayer.BLACK, sims)
        ref = restated(n, own, opp, sims, salt, K)
        assert_same_tables(m.dump(), ref, (n, sims, salt, K))
        assert float(last) == ref.last_value, (n, sims, salt, K, last, ref.last_value)
        assert np.array_equal(m._counts(oz.unpack_board(own, opp, n))[1], ref.counts(own, opp)[0])


# ------------------------------------------------------------------ 2. 64 games in one object
@pytest.mark.parametrize("K", [1, 4])
def test_64_games_in_one_object(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims = 6, 64, 60
    roots = [POSITIONS_6[g % len(POSITIONS_6)] for g in range(G)]
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * K)
    s = Search(oz, n, G, signs=SOUND, K=K)
    assert s.signs() == SOUND
    s.set_roots(roots)
    s.simulate(net, sims)
    last = s.last_values()
    for g in range(G):
        ref = restated(n, *roots[g], sims, SALT6, K)
        assert_same_tables(s.dump(g), ref, (K, g))
        assert last[g] == ref.last_value, (K, g)
    # the 4x4 start, where the passes are, in an object of 64 slots too (two salts: two objects)
    b4 = initial_board(4)
    for salt in (3, 11):
        t = Search(oz, 4, G, signs=SOUND, K=K)
        t.set_roots([b4] * G)
        t.simulate(StubNetWrapper((4, 4), salt, 0, max_batch=G * K), 100)
        for g in (0, 31, 63):
            assert_same_tables(t.dump(g), restated(4, *b4, 100, salt, K), (4, salt, K, g))


# ------------------------------------------------------------------ 3. the self-play engine
def _engine(net, K, **kw):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, 6, 8, 12, 1.0, 1.0, 0.8, seed=77, first_game_id=300, record_visits=True, record_values=True,
                          leaves_per_step=K, value_signs="sound", **kw)


def _check_games(rec, vis, val, K, salt, sample_moves=None):
    passes, term = 0, {-1: 0, 0: 0, 1: 0}
    for gid in range(300, 308):
        sel = rec["game_id"] == gid
        r, v, q = rec[sel], vis[sel], val[sel]
        W = SoundSearch(6, 1.0, K, salt=salt)
        want = episode(W, 6, 12, 77, gid, 0.8, sample_moves=sample_moves)
        assert r.size == len(want) > 0, gid
        for i, w in enumerate(want):
            assert w["margin"] >= 1e-9, (gid, i)           # (a sampled draw this close to a boundary could fall either way: none here)
            got = tuple(int(r[k][i]) for k in ("black", "white", "player", "ply", "action", "greedy"))
            assert got == (w["black"], w["white"], w["player"], w["ply"], w["action"], w["greedy"]), (gid, i)
            assert np.array_equal(v[i], w["counts"]), (gid, i)
            assert q[i] == w["value"], (gid, i, q[i], w["value"])
        fb, fw = int(r["final_black"][0]), int(r["final_white"][0])
        assert legal_mask(fb, fw, 6) == 0 and legal_mask(fw, fb, 6) == 0
        assert all(int(r["z"][i]) == (1 if popcount(fb) >= popcount(fw) else -1) * int(r["player"][i]) for i in range(r.size)), gid
        passes += W.pass_backups
        for k in term:
            term[k] += W.term[k]
    return passes, term


@pytest.mark.parametrize("K", [1, 4])
def test_selfplay_engine_vs_restatement(oz, K):
    """8 games of 6x6 at 12 simulations played to the end: moves, records, visit rows and root values, bit for bit; and the free-running driver
    reaches the same records (K = 1: it runs one leaf per game and step)"""
    from othellozero_amd.NNet import StubNetWrapper
    net = StubNetWrapper((6, 6), 21, 0, max_batch=8 * K)
    eng = _engine(net, K)
    eng.play_to_end()
    assert eng.stats()["live_games"] == 0
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    passes, term = _check_games(rec, vis, val, K, 21)
    print("K =", K, "pass backups", passes, "finished leaves", term)
    assert passes >= 1 and term[1] + term[-1] >= 1          # the games' last plies search across passes and into finished boards
    if K == 1:
        free = _engine(net, 1)
        for _ in range(400):
            free.run_steps(32)
            if free.stats()["live_games"] == 0:
                break
        assert free.stats()["live_games"] == 0
        rec2, vis2, val2 = free.records(with_visits=True, with_values=True)
        assert rec2.tobytes() == rec.tobytes() and vis2.tobytes() == vis.tobytes() and val2.tobytes() == val.tobytes()
        # ... and they are not the reference rule's games
        from othellozero_amd.training import SelfPlayEngine
        ref = SelfPlayEngine(net, 6, 8, 12, 1.0, 1.0, 0.8, seed=77, first_game_id=300, record_visits=True, record_values=True)
        ref.play_to_end()
        assert ref.records(with_values=True)[1].tobytes() != val.tobytes()


def test_selfplay_engine_with_root_noise_and_move_sampling(oz):
    """round by round, as tests/test_gpu_root_noise.py does: the device's own eta (held against root_noise_ref.dirichlet) goes into the
    restatement, whose counts and root values must then agree exactly; the move is move_sampling_ref's"""
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims, seed, first, salt, alpha, eps, sample = 6, 8, 12, 77, 300, 21, 0.5, 0.25, (1.0, 6)
    net = StubNetWrapper((n, n), salt, 0, max_batch=G)
    eng = _engine(net, 1, root_noise=(alpha, eps), sample_moves=sample)
    W = [SoundSearch(n, 1.0, 1, salt=salt) for _ in range(G)]
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


# ------------------------------------------------------------------ 4. solved leaves
@pytest.mark.parametrize("K", [1, 4])
def test_solved_leaves_vs_restatement(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims, E = 6, len(POSITIONS_6), 60, 6
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * K)
    s = Search(oz, n, G, signs=SOUND, K=K)
    oz.check(s.lib.oz_mcts_set_solve_leaves(s.h, E))
    s.set_roots(list(POSITIONS_6))
    s.simulate(net, sims)
    solved = 0
    for g, (own, opp) in enumerate(POSITIONS_6):
        ref = restated(n, own, opp, sims, SALT6, K, "sound", E)
        assert_same_tables(s.dump(g), ref, (K, g))
        assert s.last_values()[g] == ref.last_value
        solved += ref.evaluator.solved
    rows = C.c_int64()
    oz.check(s.lib.oz_mcts_get_solve_leaves(s.h, None, C.byref(rows)))
    assert solved > 0 and rows.value > 0


# ------------------------------------------------------------------ 5. the Gumbel kernels
def test_gumbel_kernels_store_the_sound_values(oz):
    """GumbelSearch and SoundSearch each restate the whole descent, so they do not compose by inheritance.  Instead: a search with the Gumbel
    option on and no root armed descends by PUCT through the *_g kernels and keeps every node's own value; its tables must be SoundSearch's
    (the stored Q of every edge, the root's among them, by the definition), and oz_mcts_node_value the evaluator's v of the node's board: the
    value for the node's own mover, which is what the definition calls V_L."""
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims = 6, len(POSITIONS_6), 60
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G)
    s = Search(oz, n, G, signs=SOUND)
    oz.check(s.lib.oz_mcts_set_gumbel(s.h, 4, 50.0, 1.0, 1, None, None))
    s.set_roots(list(POSITIONS_6))
    s.simulate(net, sims)
    for g, (own, opp) in enumerate(POSITIONS_6):
        ref = restated(n, own, opp, sims, SALT6, 1)
        assert_same_tables(s.dump(g), ref, g)
        want = [float(oracle.stub_predict(nd.own, nd.opp, n, SALT6, 0)[1]) for nd in ref.nodes]
        assert s.node_values(g) == want, g


def test_gumbel_engine_plays_whole_games(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import selfplay_batch
    n, G = 6, 8
    net = StubNetWrapper((n, n), 21, 0, max_batch=G)
    kw = dict(gumbel=(4, 50.0, 1.0), value_target=("td", 0.8))
    rec, targets, rows = selfplay_batch(net, n, G, 16, 1.0, 1.0, 1.0, 77, 300, value_signs="sound", **kw)
    assert len(set(rec["game_id"])) == G and rows.shape == (rec.size, 64) and np.isfinite(targets).all()
    assert np.allclose(rows.astype(np.float64).sum(axis=1), 1.0, atol=1e-6)
    rec0, targets0, rows0 = selfplay_batch(net, n, G, 16, 1.0, 1.0, 1.0, 77, 300, **kw)
    assert rec0.tobytes() != rec.tobytes() or rows0.tobytes() != rows.tobytes()


# ------------------------------------------------------------------ 6. the arena: a mode per agent
def test_arena_with_a_mode_per_agent(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.agents import arena_batch
    n, G, sims, seed, first = 6, 8, 25, 7, 900
    na, nb = StubNetWrapper((n, n), 41, 0, max_batch=G), StubNetWrapper((n, n), 42, 0, max_batch=G)
    r = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, value_signs=("sound", "reference"))
    passes = 0
    for gi in range(G):
        agents = {1: SoundSearch(n, 1.0, 1, salt=41, mode="sound"), -1: SoundSearch(n, 1.0, 1, salt=42, mode="reference")}
        replay_arena_game(r, gi, n, sims, seed, first + gi, agents)
        passes += agents[1].pass_backups + agents[1].term[1] + agents[1].term[-1] + agents[1].term[0]
    assert passes >= 1
    both = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, value_signs="sound")
    for gi in range(G):
        replay_arena_game(both, gi, n, sims, seed, first + gi, {1: SoundSearch(n, 1.0, 1, salt=41), -1: SoundSearch(n, 1.0, 1, salt=42)})


# ------------------------------------------------------------------ 7. a real network
def test_real_network_vs_restatement(oz):
    """4 games of 6x6 from the positions with 8 empties, f32, 16 simulations per move with the table kept, played on to the end: the tables ==
    SoundSearch fed the GPU network's own (pi, v) for those boards"""
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.weights import init_weights
    n, G, sims, C_ = 6, 4, 16, 128
    w = init_weights(n, seed=2, channels=C_, randomize_all=True)
    net = NNetWrapper((n, n), num_channels_1=C_, max_batch=G, weights=w, precision="f32")
    cache = {}

    def ev(own, opp, nn):
        if (own, opp) not in cache:                        # (a batch of the capacity the search launches the network for)
            p, v = net.predict_batch([own] * G, [opp] * G)
            cache[(own, opp)] = (p[0].ravel(), float(v[0]))
        return cache[(own, opp)]

    roots, live = list(POSITIONS_6), [True] * G
    refs = [SoundSearch(n, 1.0, 1, evaluator=ev) for _ in range(G)]
    s = Search(oz, n, G, signs=SOUND)
    for ply in range(8):
        if not any(live):
            break
        s.set_roots(roots, [1 if x else 0 for x in live])
        s.simulate(net, sims)
        cnt = s.counts()
        for g in range(G):
            if live[g]:
                refs[g].simulate(*roots[g], sims)
            assert_same_tables(s.dump(g), refs[g], (g, ply))
            if live[g]:
                roots[g] = next_state(*roots[g], n, int(np.argmax(cnt[g])))
                live[g] = legal_mask(*roots[g], n) != 0
    assert sum(r.pass_backups + sum(r.term.values()) for r in refs) >= 1
    oz.check(oz.load().oz_net_check(net._h))


# ------------------------------------------------------------------ 8. off is off, and the setter's rule
def test_reference_through_the_setter_is_the_search_without_the_option(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    n, G, sims = 6, len(POSITIONS_6), 60
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * 4)
    for K in (1, 4):
        a, b = Search(oz, n, G, K=K), Search(oz, n, G, signs=REFERENCE, K=K)
        assert a.signs() == b.signs() == REFERENCE
        for s in (a, b):
            s.set_roots(list(POSITIONS_6))
            s.simulate(net, sims)
        for g in range(G):
            _same_dumps(a.dump(g), b.dump(g), (K, g))
            assert_same_tables(a.dump(g), restated(n, *POSITIONS_6[g], sims, SALT6, K, "reference"), (K, g))
        assert a.last_values().tobytes() == b.last_values().tobytes()
        # a used tree keeps its rule: the setter refuses and the object goes on as before
        for mode in (SOUND, REFERENCE):
            assert lib.oz_mcts_set_value_signs(b.h, mode) == oz.OZ_ERR_STATE and "oz_mcts_reset" in lib.oz_last_error().decode()
        assert lib.oz_mcts_set_value_signs(b.h, 2) == oz.OZ_ERR_ARG
        assert b.signs() == REFERENCE
        for s in (a, b):
            s.simulate(net, 20)
        for g in range(G):
            _same_dumps(a.dump(g), b.dump(g), (K, g, "after the refusal"))
        # an emptied tree takes the other rule
        oz.check(lib.oz_mcts_reset(b.h, -1))
        oz.check(lib.oz_mcts_set_value_signs(b.h, SOUND))
        b.set_roots(list(POSITIONS_6))
        b.simulate(net, sims)
        for g in range(G):
            assert_same_tables(b.dump(g), restated(n, *POSITIONS_6[g], sims, SALT6, K), (K, g, "after the reset"))
    # the engine: "reference" by name plays the bytes of the engine without the option; the setter closes with the first driver call
    kw = dict(seed=5, first_game_id=40, record_visits=True, record_values=True)
    x, y = SelfPlayEngine(net, n, 8, 12, **kw), SelfPlayEngine(net, n, 8, 12, value_signs="reference", **kw)
    for e in (x, y):
        e.play_to_end()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x.records(with_visits=True, with_values=True), y.records(with_visits=True, with_values=True)))
    assert lib.oz_selfplay_set_value_signs(y._h, SOUND) == oz.OZ_ERR_STATE and "before the first driver call" in lib.oz_last_error().decode()
    mode = C.c_int(-1)
    oz.check(lib.oz_selfplay_get_value_signs(y._h, C.byref(mode)))
    assert mode.value == REFERENCE
    # the arena
    h = C.c_void_p()
    oz.check(lib.oz_arena_create(C.byref(h), n, 4, 10, 1.0, oz.QMODE_F64, 1, 0, net._h, net._h, 0))
    try:
        assert lib.oz_arena_set_value_signs(h, SOUND, 2) == oz.OZ_ERR_ARG
        oz.check(lib.oz_arena_set_value_signs(h, SOUND, REFERENCE))
        oz.check(lib.oz_arena_run_rounds(h, 2))
        assert lib.oz_arena_set_value_signs(h, REFERENCE, REFERENCE) == oz.OZ_ERR_STATE
    finally:
        lib.oz_arena_destroy(h)


# ------------------------------------------------------------------ 9. loop.training: one setting for self-play, the match and the evaluation
@pytest.mark.parametrize("replay", ["host", "device"])
def test_training_loop_passes_the_option_on(oz, tmp_path, monkeypatch, replay):
    from othellozero_amd import loop, training
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    seen = []
    real_engine, real_arena = training.SelfPlayEngine, loop.arena_batch

    class Engine(real_engine):
        def __init__(self, *a, **kw):
            seen.append(("engine", kw.get("value_signs")))
            super().__init__(*a, **kw)

    def arena(*a, **kw):
        seen.append(("arena", kw.get("value_signs")))
        return real_arena(*a, **kw)
    monkeypatch.setattr(training, "SelfPlayEngine", Engine)
    monkeypatch.setattr(loop, "arena_batch", arena)
    n = 6
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    kw = dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
              evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0, self_play_training=True, self_play_interval=1,
              self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
              training_buffer_size=8 * 40 * 8, seed=13, alias_final_boards=False, batched_evaluation=True, reference_aliasing=False)
    historic = loop.training(neural_network=net, replay=replay, value_signs="sound", **kw)
    assert len(historic) == 1
    assert [k for k, _ in seen].count("engine") == 1 and [k for k, _ in seen].count("arena") >= 4      # a match (2 arenas) and two evaluations
    assert all(v == "sound" for _, v in seen), seen
    with pytest.raises(ValueError):
        loop.training(neural_network=net, replay=replay, value_signs="negamax", **kw)
