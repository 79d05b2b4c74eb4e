"""The selection option on the GPU (pytest -m gpu): the *_sel instantiations of the tree kernels against the restatement in
tests/selection_ref.py (SelectSearch / SelectProvenSearch), bit for bit -- tables, vhat of every node, root counts and last values; the
drop-in search at K = 1 and K = 4 in both value signs, 64 slots in one object, proofs with solved leaves and proof play, root noise, the
host-evaluator split, the self-play engine, the arena with a setting per agent, the float32 regime of the Q update -- and the option off
against an object that was never given it, and the refusals.  Stub network and q_mode F64 unless a test says otherwise; the restatement's
logarithm is the library's host twin (selection_ref.library_log)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import oracle
import selection_ref as R
import solve_leaves_ref as SL
from move_sampling_ref import selfplay_move
from root_noise_ref import dirichlet
from selection_ref import CASES, CLAMP, SALT6, SETTINGS, Nep50SelectSearch, SelectProvenSearch, SelectSearch
from value_signs_ref import POSITIONS_6, episode, replay_arena_game
from wide_search_ref import assert_same_tables, initial_board, legal_mask, popcount

pytestmark = pytest.mark.gpu

REFERENCE, SOUND = 0, 1
EVERY = dict(SETTINGS, clamp=CLAMP)
OFF_ROW = (0, 0.0, 0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@functools.lru_cache(maxsize=None)
def restated(n, own, opp, sims, salt, K, mode, setting, solve=0, proofs=False):
    """the restatement's search of one case, computed once and shared (read only)"""
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    sel = EVERY[setting] if setting is not None else None
    if proofs:
        s = SelectProvenSearch(n, 1.0, K, salt=salt, evaluator=ev, solve=solve, selection=sel, growth_log=R.library_log)
    else:
        s = SelectSearch(n, 1.0, K, salt=salt, evaluator=ev, mode=mode, selection=sel, growth_log=R.library_log)
    s.simulate(own, opp, sims)
    return s


class Search:
    """a bare oz_mcts with G slots"""

    def __init__(self, oz, n, G, node_cap=1024, signs=None, proofs=None, K=1, selection="absent", q_mode=None):
        self.oz, self.lib, self.n, self.G = oz, oz.load(), n, G
        self.h = C.c_void_p()
        oz.check(self.lib.oz_mcts_create(C.byref(self.h), n, G, node_cap, 1.0, oz.QMODE_F64 if q_mode is None else q_mode))
        if signs is not None:
            oz.check(self.lib.oz_mcts_set_value_signs(self.h, signs))
        if proofs is not None:
            oz.check(self.lib.oz_mcts_set_proofs(self.h, proofs))
        if selection != "absent":
            oz.check(self.lib.oz_mcts_set_selection(self.h, *oz.check_selection(selection)))
        if K != 1:
            oz.check(self.lib.oz_mcts_set_leaves_per_step(self.h, K))

    def __del__(self):
        if self.h:
            self.lib.oz_mcts_destroy(self.h)
            self.h = C.c_void_p()

    def selection(self):
        flags, v = C.c_int(-1), [C.c_double(-1.0) for _ in range(4)]
        self.oz.check(self.lib.oz_mcts_get_selection(self.h, C.byref(flags), *(C.byref(x) for x in v)))
        return (flags.value, *(x.value for x in v))

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

    def node_values(self, g):
        out = []
        for i in range(int(self.num_nodes()[g])):
            v = C.c_double(-9.0)
            self.oz.check(self.lib.oz_mcts_node_value(self.h, g, i, C.byref(v)))
            out.append(v.value)
        return out

    def last_values(self):
        v = np.zeros(self.G, np.float64)
        self.oz.check(self.lib.oz_mcts_last_value(self.h, self.oz.p_f64(v), None, None))
        return v

    def counts(self):
        cnt, legal, rc = np.zeros((self.G, 64), np.int32), np.zeros(self.G, np.uint64), np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_root_counts(self.h, self.oz.p_i32(cnt), self.oz.p_u64(legal), self.oz.p_i32(rc)))
        return cnt


def same_proofs(dump, ref, where, oz):
    U = oz.PROOF_UNKNOWN
    assert len(dump) == len(ref.nodes), where
    for i, d in enumerate(dump):
        assert [int(x) for x in d["edge"]] == [ref.edge[i].get(s, U) for s in range(64)], (where, i)
        assert d["value"] == (U if ref.own[i] is None else ref.own[i]), (where, i)
        v = ref.val(i)
        assert d["val"] == (U if v is None else v), (where, i)


def _same_dumps(a, b, where):
    assert len(a) == len(b), where
    for x, y in zip(a, b):
        assert (x["k0"], x["k1"], x["Ns"], x["legal"]) == (y["k0"], y["k1"], y["Ns"], y["legal"]), where
        for key in ("N", "Q", "qtag", "P"):
            assert np.array_equal(x[key], y[key]), (where, key)


# ------------------------------------------------------------------ 1. the drop-in search, one game
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("setting", list(EVERY))
def test_othello_mcts_vs_restatement(oz, K, setting):
    """each part alone, all three together and the clamp setting, in reference and in sound signs, over the case set"""
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    sel = EVERY[setting]
    for n, own, opp, sims, salt in CASES:
        net = StubNetWrapper((n, n), salt, 0, max_batch=K)
        for mode in ("reference", "sound"):
            m = OthelloMCTS(n, net, 1.0, q_mode=oz.QMODE_F64, node_cap=1024, leaves_per_step=K, value_signs=mode, selection=sel)
            assert m.selection == oz.selection_dict(oz.check_selection(sel))
            board = oz.unpack_board(own, opp, n)
            last = m.simulate_n(board, OthelloPlayer.BLACK, sims)
            ref = restated(n, own, opp, sims, salt, K, mode, setting)
            where = (n, sims, salt, K, mode, setting)
            assert_same_tables(m.dump(), ref, where)
            assert m.node_values() == ref.vhat, where
            assert float(last) == ref.last_value, (where, last, ref.last_value)
            assert np.array_equal(m._counts(board)[1], ref.counts(own, opp)[0]), where


# ------------------------------------------------------------------ 2. 64 slots in one object
@pytest.mark.parametrize("K", [1, 4])
def test_64_slots_in_one_object(oz, K):
    """slots cycle through the cases of one board size, every fifth slot inactive; all three parts on, sound signs"""
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims = 6, 64, 60
    roots = [POSITIONS_6[g % len(POSITIONS_6)] for g in range(G)]
    active = [0 if g % 5 == 3 else 1 for g in range(G)]
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * K)
    s = Search(oz, n, G, signs=SOUND, K=K, selection=SETTINGS["all"])
    assert s.selection() == (7, 0.2, 0.1, 20.0, 2.0)
    s.set_roots(roots, active)
    s.simulate(net, sims)
    last, cnt, nn = s.last_values(), s.counts(), s.num_nodes()
    for g in range(G):
        if not active[g]:
            assert nn[g] == 0, (K, g)
            continue
        ref = restated(n, *roots[g], sims, SALT6, K, "sound", "all")
        assert_same_tables(s.dump(g), ref, (K, g))
        assert last[g] == ref.last_value and np.array_equal(cnt[g], ref.counts(*roots[g])[0]), (K, g)
        if g < 8:
            assert s.node_values(g) == ref.vhat, (K, g)
    b4 = initial_board(4)
    for salt, setting in ((3, "fpu"), (11, "all")):         # the 4x4 start, reference signs (two salts: two objects)
        t = Search(oz, 4, G, K=K, selection=SETTINGS[setting])
        t.set_roots([b4] * G, active)
        t.simulate(StubNetWrapper((4, 4), salt, 0, max_batch=G * K), 100)
        ref = restated(4, *b4, 100, salt, K, "reference", setting)
        for g in (0, 31, 62):
            assert_same_tables(t.dump(g), ref, (4, salt, K, g))
            assert t.node_values(g) == ref.vhat
        assert t.num_nodes()[3] == 0 and t.num_nodes()[63] == 0


# ------------------------------------------------------------------ 3. proofs with solved leaves; proof play
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("setting", ["fpu", "all"])
def test_proofs_with_solved_leaves_vs_restatement(oz, K, setting):
    from othellozero_amd.NNet import StubNetWrapper
    n, sims, E = 6, 60, 6
    roots = list(POSITIONS_6)
    G = len(roots)
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=G * K)
    s = Search(oz, n, G, signs=SOUND, proofs=1, K=K, selection=SETTINGS[setting])
    oz.check(s.lib.oz_mcts_set_solve_leaves(s.h, E))
    s.set_roots(roots)
    s.simulate(net, sims)
    last, cnt = s.last_values(), s.counts()
    stops = 0
    for g, (own, opp) in enumerate(roots):
        ref = restated(n, own, opp, sims, SALT6, K, "sound", setting, E, True)
        where = (K, setting, g)
        assert_same_tables(s.dump(g), ref, where)
        same_proofs(s.dump_proofs(g), ref, where, oz)
        assert s.node_values(g) == ref.vhat, where                      # (the solved sign where the leaf was solved)
        assert last[g] == ref.last_value and np.array_equal(cnt[g], ref.counts(own, opp)[0]), where
        stops += ref.edge_stops + ref.node_stops
    st = np.zeros(4, np.int64)
    oz.check(s.lib.oz_mcts_proof_stats(s.h, oz.p_i64(st)))
    assert stops > 0 and int(st[1] + st[2]) == stops


def test_proof_play_through_the_drop_in_search(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    n, sims, E, K = 6, 60, 6, 1
    own, opp = POSITIONS_6[1]
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=K)
    m = OthelloMCTS(n, net, 1.0, node_cap=1024, value_signs="sound", proofs=True, proof_play=True, solve_leaves=E, selection=SETTINGS["all"])
    board = oz.unpack_board(own, opp, n)
    m.simulate_n(board, OthelloPlayer.BLACK, sims)
    ref = restated(n, own, opp, sims, SALT6, K, "sound", "all", E, True)
    dump = m.dump()
    assert_same_tables(dump, ref, "proof play")
    same_proofs([d["proofs"] for d in dump], ref, "proof play", oz)
    val, edge = ref.root_proof(own, opp)
    raw = ref.counts(own, opp)[0]
    keep = ref.candidates(ref.index[(own, opp)], val)
    if not any(raw[s] > 0 for s in keep):
        keep = list(ref.nodes[ref.index[(own, opp)]].acts)
    want = np.array([raw[s] if s in keep else 0 for s in range(64)], np.int32)
    assert np.array_equal(m.proven_counts(board), want)
    if val is not None:
        assert m.root_value(board, proven=True) == float(val)


# ------------------------------------------------------------------ 4. root noise with host-supplied eta
@pytest.mark.parametrize("K", [1, 4])
def test_root_noise_on_the_4x4_cases(oz, K):
    """FPU at the noisy root sums Pn into SP and subtracts root_reduction"""
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    eps, seen = 0.25, 0
    for n, own, opp, sims, salt in CASES[:4]:
        lg = legal_mask(own, opp, n)
        rng = random.Random(salt * 1000 + sims)
        w = [rng.random() if (lg >> s) & 1 else 0.0 for s in range(64)]
        eta = np.array(w) / sum(w)
        for setting, mode in (("fpu", "reference"), ("all", "sound")):
            net = StubNetWrapper((n, n), salt, 0, max_batch=K)
            m = OthelloMCTS(n, net, 1.0, node_cap=1024, leaves_per_step=K, value_signs=mode, selection=SETTINGS[setting])
            board = oz.unpack_board(own, opp, n)
            m.set_root_noise(eta, eps, state=board, player=OthelloPlayer.BLACK)
            last = m.simulate_n(board, OthelloPlayer.BLACK, sims)
            ref = SelectSearch(n, 1.0, K, salt=salt, mode=mode, selection=SETTINGS[setting], growth_log=R.library_log)
            ref.set_noise(own, opp, eta, eps)
            ref.simulate(own, opp, sims)
            where = (sims, salt, K, setting)
            assert_same_tables(m.dump(), ref, where)
            assert float(last) == ref.last_value and m.node_values() == ref.vhat, where
            plain = restated(n, own, opp, sims, salt, K, mode, setting)
            seen += not np.array_equal(ref.counts(own, opp)[0], plain.counts(own, opp)[0])
    assert seen >= 4                                            # the noise was seen: most searches' root counts moved


# ------------------------------------------------------------------ 5. the host-evaluator split
class HostStub:
    """a duck-typed network: OthelloMCTS hands it every leaf on the host (oz_mcts_select / leaves / backup)"""

    class network_type:
        name = "ONN"

    def __init__(self, oz, n, salt):
        self.oz, self.n, self.salt, self.calls = oz, n, salt, 0

    def predict(self, board):
        own, opp = self.oz.pack_board(board)
        self.calls += 1
        pi, v = oracle.stub_predict(own, opp, self.n, self.salt, 0)
        return np.asarray(pi, np.float32), float(v)


def test_host_evaluator_split_gives_the_tables_of_simulate(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    for n, own, opp, sims, salt in (CASES[0], CASES[5]):
        for mode in ("reference", "sound"):
            board = oz.unpack_board(own, opp, n)
            host = HostStub(oz, n, salt)
            a = OthelloMCTS(n, host, 1.0, node_cap=1024, value_signs=mode, selection=SETTINGS["all"])
            b = OthelloMCTS(n, StubNetWrapper((n, n), salt, 0, max_batch=1), 1.0, node_cap=1024, value_signs=mode, selection=SETTINGS["all"])
            la, lb = a.simulate_n(board, OthelloPlayer.BLACK, sims), b.simulate_n(board, OthelloPlayer.BLACK, sims)
            assert host.calls > 0 and not a._native and b._native
            _same_dumps(a.dump(), b.dump(), (n, mode))
            assert a.node_values() == b.node_values() and float(la) == float(lb)
            assert_same_tables(a.dump(), restated(n, own, opp, sims, salt, 1, mode, "all"), (n, mode))


# ------------------------------------------------------------------ 6. the self-play engine
def _engine(net, K, selection, **kw):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, 6, 8, 16, 1.0, 1.0, 0.8, seed=77, first_game_id=300, record_visits=True, record_values=True,
                          leaves_per_step=K, selection=selection, **kw)


@pytest.mark.parametrize("K", [1, 4])
def test_selfplay_engine_vs_restatement(oz, K):
    """8 games of 6x6 at 16 simulations through run() to the end: records, visit rows and root values, bit for bit"""
    from othellozero_amd.NNet import StubNetWrapper
    salt = 21
    net = StubNetWrapper((6, 6), salt, 0, max_batch=8 * K)
    eng = _engine(net, K, SETTINGS["all"], value_signs="sound")
    assert eng.selection == dict(fpu=(0.2, 0.1), cpuct_growth=(20.0, 2.0), prior_first=True)
    eng.play_to_end()
    assert eng.stats()["live_games"] == 0
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    moved = 0
    for gid in range(300, 308):
        pick = rec["game_id"] == gid
        r, v, q = rec[pick], vis[pick], val[pick]
        W = SelectSearch(6, 1.0, K, salt=salt, mode="sound", selection=SETTINGS["all"], growth_log=R.library_log)
        want = episode(W, 6, 16, 77, gid, 0.8)
        assert r.size == len(want) > 0, gid
        for i, w in enumerate(want):
            got = tuple(int(r[k][i]) for k in ("black", "white", "player", "ply", "action", "greedy"))
            assert got == (w["black"], w["white"], w["player"], w["ply"], w["action"], w["greedy"]), (gid, i)
            assert np.array_equal(v[i], w["counts"]), (gid, i)
            assert q[i] == w["value"], (gid, i, q[i], w["value"])
        fb, fw = int(r["final_black"][0]), int(r["final_white"][0])
        assert legal_mask(fb, fw, 6) == 0 and legal_mask(fw, fb, 6) == 0
        assert all(int(r["z"][i]) == (1 if popcount(fb) >= popcount(fw) else -1) * int(r["player"][i]) for i in range(r.size)), gid
        moved += W.prior_first_moved + W.growth_changed
    assert moved >= 1
    off = _engine(net, K, None, value_signs="sound")
    off.play_to_end()
    assert off.records(with_values=True)[1].tobytes() != val.tobytes()          # ... and they are not the games of the engine without it


@pytest.mark.parametrize("K", [1, 4])
def test_selfplay_engine_with_root_noise_move_sampling_and_playout_cap(oz, K):
    """round by round: the device's own eta (held against root_noise_ref.dirichlet) goes into the restatement, the budget of every move is
    the playout cap's, and counts, root values and moves must then agree exactly"""
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims, seed, first, salt, alpha, eps, sample, cap = 6, 8, 16, 77, 300, 21, 0.5, 0.25, (1.0, 6), (6, 0.5)
    sel = SETTINGS["all"]
    net = StubNetWrapper((n, n), salt, 0, max_batch=G * K)
    eng = _engine(net, K, sel, root_noise=(alpha, eps), sample_moves=sample, playout_cap=cap)
    W = [SelectSearch(n, 1.0, K, salt=salt, mode="reference", selection=sel, growth_log=R.library_log) for _ in range(G)]
    values, searched, fast_moves = {}, 0, 0
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
            budget = int(oz.playout_budgets(seed, [gid], [ply], sims, cap)[0])
            if budget == sims:
                assert armed[g] and np.abs(eta[g] - dirichlet(n, lg, alpha, seed, gid, ply)[0]).max() <= 1e-9, (rnd, g)
                W[g].set_noise(own, opp, eta[g], eps)
            else:
                assert not armed[g], (rnd, g)
                W[g].noise = None
                fast_moves += 1
            W[g].simulate(own, opp, budget)
            assert np.array_equal(cnt[g], W[g].counts(own, opp)[0]), (rnd, g)
            values[(gid, ply)] = W[g].root_value(own, opp)
            action, greedy, margin = selfplay_move(cnt[g], lg, 0.8, seed, gid, ply, sample)
            placed = (int(after["black"][g]) | int(after["white"][g])) & ~(b | w)
            if margin >= 1e-9:
                assert placed == 1 << action, (rnd, g, greedy)
            searched += 1
    assert eng.stats()["live_games"] == 0 and searched == eng.stats()["moves"] and 0 < fast_moves < searched
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    assert rec.size == searched
    for i in range(rec.size):
        assert val[i] == values[(int(rec["game_id"][i]), int(rec["ply"][i]))], i


# ------------------------------------------------------------------ 7. the arena: a setting per agent
def test_arena_with_a_setting_per_agent(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.agents import arena_batch
    n, G, sims, seed, first = 6, 8, 16, 7, 900
    na, nb = StubNetWrapper((n, n), 41, 0, max_batch=G), StubNetWrapper((n, n), 42, 0, max_batch=G)
    pair = (SETTINGS["all"], SETTINGS["fpu"])
    r = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, selection=pair)
    for gi in range(G):
        agents = {1: SelectSearch(n, 1.0, 1, salt=41, mode="reference", selection=pair[0], growth_log=R.library_log),
                  -1: SelectSearch(n, 1.0, 1, salt=42, mode="reference", selection=pair[1], growth_log=R.library_log)}
        replay_arena_game(r, gi, n, sims, seed, first + gi, agents)
    one = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, selection=(None, SETTINGS["growth"]),
                      value_signs="sound")
    for gi in range(G):
        agents = {1: SelectSearch(n, 1.0, 1, salt=41, mode="sound"),
                  -1: SelectSearch(n, 1.0, 1, salt=42, mode="sound", selection=SETTINGS["growth"], growth_log=R.library_log)}
        replay_arena_game(one, gi, n, sims, seed, first + gi, agents)
    plain = arena_batch(na, nb, n, G, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64)
    assert plain["actions"].tobytes() != r["actions"].tobytes()


# ------------------------------------------------------------------ 8. the float32 regime of the Q update
def test_qmode_nep50_vs_restatement(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    n, own, opp, sims, salt = CASES[2]
    for mode in ("reference", "sound"):
        m = OthelloMCTS(n, StubNetWrapper((n, n), salt, 0, max_batch=1), 1.0, q_mode=oz.QMODE_NEP50, node_cap=1024, value_signs=mode,
                        selection=SETTINGS["all"])
        m.simulate_n(oz.unpack_board(own, opp, n), OthelloPlayer.BLACK, sims)
        ref = Nep50SelectSearch(n, 1.0, salt=salt, mode=mode, selection=SETTINGS["all"], growth_log=R.library_log)
        ref.simulate(own, opp, sims)
        dump = m.dump()
        assert_same_tables(dump, ref, mode)
        assert m.node_values() == ref.vhat
        tagged = 0
        for i, d in enumerate(dump):
            for s in ref.nodes[i].acts:
                assert bool(d["qtag"][s]) == ref.q32[i].get(s, False), (mode, i, s)
                tagged += bool(d["qtag"][s])
        assert tagged > 0


# ------------------------------------------------------------------ 9. off is off
def test_all_parts_off_through_the_setter_is_the_search_without_the_option(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    for K in (1, 4):
        for n, own, opp, sims, salt in CASES:
            net = StubNetWrapper((n, n), salt, 0, max_batch=K)
            a = Search(oz, n, 1, K=K)
            b = Search(oz, n, 1, K=K, selection=dict(fpu=None, cpuct_growth=None, prior_first=False))
            assert a.selection() == b.selection() == OFF_ROW
            for s in (a, b):
                s.set_roots([(own, opp)])
                s.simulate(net, sims)
            _same_dumps(a.dump(0), b.dump(0), (K, n, sims, salt))
            assert a.last_values().tobytes() == b.last_values().tobytes()
            assert set(b.node_values(0)) == {0.0}                               # no vhat is kept without the option
            assert_same_tables(b.dump(0), restated(n, own, opp, sims, salt, K, "reference", None), (K, n, sims, salt))
    # parameters of a part that is off are not kept, and not checked
    c = Search(oz, 6, 1)
    oz.check(c.lib.oz_mcts_set_selection(c.h, oz.SELECT_PRIOR_FIRST, 9.0, float("nan"), -3.0, float("nan")))
    assert c.selection() == (oz.SELECT_PRIOR_FIRST, 0.0, 0.0, 0.0, 0.0)
    oz.check(c.lib.oz_mcts_set_selection(c.h, 0, 0.0, 0.0, 0.0, 0.0))
    assert c.selection() == OFF_ROW
    # the engine: the keyword with every part off plays the bytes of the engine without it
    net = StubNetWrapper((6, 6), SALT6, 0, max_batch=8)
    kw = dict(seed=5, first_game_id=40, record_visits=True, record_values=True)
    x, y = SelfPlayEngine(net, 6, 8, 12, **kw), SelfPlayEngine(net, 6, 8, 12, selection={}, **kw)
    assert x.selection is None and y.selection is None
    for e in (x, y):
        e.play_to_end()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x.records(with_visits=True, with_values=True), y.records(with_visits=True, with_values=True)))


# ------------------------------------------------------------------ 10. the refusals, in both orders
def test_refusals_in_both_orders(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    n = 6
    own, opp = POSITIONS_6[0]
    net = StubNetWrapper((n, n), SALT6, 0, max_batch=8)
    on = oz.check_selection(SETTINGS["all"])

    def err():
        return lib.oz_last_error().decode()
    # argument checks on a live object
    s = Search(oz, n, 1)
    nan = float("nan")
    for bad in ((8, 0, 0, 0, 0), (1, -0.1, 0.1, 0, 0), (1, 0.2, 4.5, 0, 0), (1, nan, 0.1, 0, 0), (2, 0, 0, 0.0, 1.0), (2, 0, 0, 20.0, -1.0),
                (2, 0, 0, nan, 1.0), (2, 0, 0, 20.0, nan)):
        assert lib.oz_mcts_set_selection(s.h, *bad) == oz.OZ_ERR_ARG, bad
    assert s.selection() == OFF_ROW
    # the Gumbel search
    oz.check(lib.oz_mcts_set_selection(s.h, *on))
    assert lib.oz_mcts_set_gumbel(s.h, 4, 50.0, 1.0, 1, None, None) == oz.OZ_ERR_STATE and "selection" in err()
    g = Search(oz, n, 1)
    oz.check(lib.oz_mcts_set_gumbel(g.h, 4, 50.0, 1.0, 1, None, None))
    assert lib.oz_mcts_set_selection(g.h, *on) == oz.OZ_ERR_STATE and "Gumbel" in err()
    oz.check(lib.oz_mcts_set_selection(g.h, 0, 0.0, 0.0, 0.0, 0.0))             # off beside it is fine
    # forced playouts (they need armed root noise)
    eta = np.zeros((1, 64))
    lg = legal_mask(own, opp, n)
    for sq in range(64):
        if (lg >> sq) & 1:
            eta[0, sq] = 1.0 / popcount(lg)
    s.set_roots([(own, opp)])
    oz.check(lib.oz_mcts_set_root_noise(s.h, 0.25, oz.p_f64(eta), None))
    assert lib.oz_mcts_set_forced_playouts(s.h, 2.0) == oz.OZ_ERR_STATE and "selection" in err()
    f = Search(oz, n, 1)
    f.set_roots([(own, opp)])
    oz.check(lib.oz_mcts_set_root_noise(f.h, 0.25, oz.p_f64(eta), None))
    oz.check(lib.oz_mcts_set_forced_playouts(f.h, 2.0))
    assert lib.oz_mcts_set_selection(f.h, *on) == oz.OZ_ERR_STATE and "forced playouts" in err()
    oz.check(lib.oz_mcts_set_forced_playouts(f.h, 0.0))
    oz.check(lib.oz_mcts_set_selection(f.h, *on))
    # a tree that holds nodes keeps its rule, and goes on as before
    s.simulate(net, 30)
    assert lib.oz_mcts_set_selection(s.h, 0, 0.0, 0.0, 0.0, 0.0) == oz.OZ_ERR_STATE and "oz_mcts_reset" in err()
    assert lib.oz_mcts_set_selection(s.h, *oz.check_selection(SETTINGS["fpu"])) == oz.OZ_ERR_STATE
    assert s.selection() == on
    s.simulate(net, 30)
    ref = SelectSearch(n, 1.0, 1, salt=SALT6, mode="reference", selection=SETTINGS["all"], growth_log=R.library_log)
    ref.set_noise(own, opp, eta[0], 0.25)
    ref.simulate(own, opp, 60)
    assert_same_tables(s.dump(0), ref, "after the refusal")
    p = Search(oz, n, 1)
    p.set_roots([(own, opp)])
    p.simulate(net, 10)
    assert lib.oz_mcts_set_selection(p.h, *on) == oz.OZ_ERR_STATE and "oz_mcts_reset" in err()
    oz.check(lib.oz_mcts_reset(p.h, -1))
    oz.check(lib.oz_mcts_set_selection(p.h, *on))
    # a pending host-evaluated step
    q = Search(oz, n, 1)
    q.set_roots([(own, opp)])
    oz.check(lib.oz_mcts_select(q.h))
    assert lib.oz_mcts_set_selection(q.h, *on) == oz.OZ_ERR_STATE and "pending" in err()
    # the engine: the free-running family refuses it, and the setter closes with the first driver call
    kw = dict(seed=5, first_game_id=40)
    e = SelfPlayEngine(net, n, 8, 12, selection=SETTINGS["all"], **kw)
    assert lib.oz_selfplay_run_steps(e._h, 1) == oz.OZ_ERR_STATE and "selection" in err()
    e.run(1)                                                                    # ... and is as usable as before
    e2 = SelfPlayEngine(net, n, 8, 12, refill=True, selection=SETTINGS["all"], **kw)
    assert lib.oz_selfplay_stagger(e2._h, 4) == oz.OZ_ERR_STATE and "selection" in err()
    for first in ("run_steps", "stagger", "run"):
        e3 = SelfPlayEngine(net, n, 8, 12, refill=True, **kw)
        if first == "run_steps":
            oz.check(lib.oz_selfplay_run_steps(e3._h, 1))
        elif first == "stagger":
            oz.check(lib.oz_selfplay_stagger(e3._h, 4))
        else:
            e3.run(1)
        assert lib.oz_selfplay_set_selection(e3._h, *on) == oz.OZ_ERR_STATE and "before the first driver call" in err(), first
    e4 = SelfPlayEngine(net, n, 8, 12, root_noise=(0.5, 0.25), selection=SETTINGS["all"], **kw)
    assert lib.oz_selfplay_set_forced_playouts(e4._h, 2.0) == oz.OZ_ERR_STATE and "selection" in err()
    assert lib.oz_selfplay_set_gumbel(e4._h, 4, 50.0, 1.0) == oz.OZ_ERR_STATE
    e5 = SelfPlayEngine(net, n, 8, 12, gumbel=(4, 50.0, 1.0), **kw)
    assert lib.oz_selfplay_set_selection(e5._h, *on) == oz.OZ_ERR_STATE and "Gumbel" in err()
    e6 = SelfPlayEngine(net, n, 8, 12, root_noise=(0.5, 0.25), forced_playouts=2.0, **kw)
    assert lib.oz_selfplay_set_selection(e6._h, *on) == oz.OZ_ERR_STATE and "forced playouts" in err()
    flags = C.c_int(-1)
    oz.check(lib.oz_selfplay_get_selection(e6._h, C.byref(flags), None, None, None, None))
    assert flags.value == 0
    # the arena
    h = C.c_void_p()
    oz.check(lib.oz_arena_create(C.byref(h), n, 4, 10, 1.0, oz.QMODE_F64, 1, 0, net._h, net._h, 0))
    try:
        assert lib.oz_arena_set_selection(h, 0, *on) == oz.OZ_ERR_ARG
        assert lib.oz_arena_set_selection(h, 1, 1, 5.0, 0.0, 0.0, 0.0) == oz.OZ_ERR_ARG
        oz.check(lib.oz_arena_set_selection(h, 1, *on))
        oz.check(lib.oz_arena_set_selection(h, -1, *oz.check_selection(SETTINGS["fpu"])))
        oz.check(lib.oz_arena_run_rounds(h, 2))
        assert lib.oz_arena_set_selection(h, 1, 0, 0.0, 0.0, 0.0, 0.0) == oz.OZ_ERR_STATE and "before the first run" in err()
    finally:
        lib.oz_arena_destroy(h)


# ------------------------------------------------------------------ 11. loop.training: one setting for self-play, the match and the evaluation
def test_training_loop_passes_the_option_on(oz, tmp_path, monkeypatch):
    from othellozero_amd import loop, training
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    seen = []
    real_engine, real_arena = training.SelfPlayEngine, loop.arena_batch

    class Engine(real_engine):
        def __init__(self, *a, **kw):
            seen.append(("engine", kw.get("selection")))
            super().__init__(*a, **kw)

    def arena(*a, **kw):
        seen.append(("arena", kw.get("selection")))
        return real_arena(*a, **kw)
    monkeypatch.setattr(training, "SelfPlayEngine", Engine)
    monkeypatch.setattr(loop, "arena_batch", arena)
    n = 6
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    kw = dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
              evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0, self_play_training=True, self_play_interval=1,
              self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
              training_buffer_size=8 * 40 * 8, seed=13, alias_final_boards=False, batched_evaluation=True, reference_aliasing=False)
    historic = loop.training(neural_network=net, replay="device", selection=SETTINGS["all"], **kw)
    assert len(historic) == 1
    assert [k for k, _ in seen].count("engine") == 1 and [k for k, _ in seen].count("arena") >= 4      # a match (2 arenas) and two evaluations
    assert all(v == SETTINGS["all"] for _, v in seen), seen
    with pytest.raises(ValueError):
        loop.training(neural_network=net, replay="device", selection=dict(fpu=(9.0, 0.1)), **kw)
    with pytest.raises(ValueError):
        loop.training(neural_network=net, replay="device", selection=SETTINGS["all"], gumbel=True, policy_target="improved", **kw)
