"""Tree collection on the GPU (pytest -m gpu): k_tree_collect drops exactly the nodes the rule of tests/tree_gc_ref.py calls dead and changes
nothing else.  An object that collects is held, node for node and bit for bit, against the host-filtered dump of an object that never
does; the engine, the arena and the drop-in search with the option against themselves without it; the refusals; and the option off against
an engine that never heard of it.  Stub networks, q_mode F64, 6x6 throughout."""
import ctypes as C
import random

import numpy as np
import pytest

from tree_gc_ref import tree_keep
from value_signs_ref import POSITIONS_6
from wide_search_ref import initial_board, legal_mask, next_state

pytestmark = pytest.mark.gpu

N, SIMS, SALT = 6, 24, 7
ALL_SELECTION = dict(fpu=(0.2, 0.1), cpuct_growth=(19652.0, 1.25), prior_first=True)
CONFIGS = {
    "k1-reference": dict(K=1, signs=0),
    "k4-reference": dict(K=4, signs=0),
    "k1-sound": dict(K=1, signs=1),
    "k4-sound": dict(K=4, signs=1),
    "proofs-solve6": dict(K=1, signs=1, proofs=True, solve=6),
    "selection-all": dict(K=1, signs=0, selection=ALL_SELECTION),
}


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def net(oz):
    from othellozero_amd.NNet import StubNetWrapper
    return StubNetWrapper((N, N), salt=SALT, max_batch=256)


class Search:
    """a bare oz_mcts with G slots"""

    def __init__(self, oz, G, node_cap, K=1, signs=0, proofs=False, solve=0, selection=None):
        self.oz, self.lib, self.G, self.proofs, self.vhat = oz, oz.load(), G, proofs, selection is not None
        self.h = C.c_void_p()
        oz.check(self.lib.oz_mcts_create(C.byref(self.h), N, G, node_cap, 1.0, oz.QMODE_F64))
        if signs:
            oz.check(self.lib.oz_mcts_set_value_signs(self.h, signs))
        if proofs:
            oz.check(self.lib.oz_mcts_set_proofs(self.h, 1))
        if selection is not None:
            oz.check(self.lib.oz_mcts_set_selection(self.h, *oz.check_selection(selection)))
        if K != 1:
            oz.check(self.lib.oz_mcts_set_leaves_per_step(self.h, K))
        if solve:
            oz.check(self.lib.oz_mcts_set_solve_leaves(self.h, solve))

    def __del__(self):
        if self.h:
            self.lib.oz_mcts_destroy(self.h)
            self.h = C.c_void_p()

    def set_roots(self, roots, active=None):
        a, b = np.array([r[0] for r in roots], np.uint64), np.array([r[1] for r in roots], np.uint64)
        act = None if active is None else self.oz.p_u8(np.array(active, np.uint8))
        self.oz.check(self.lib.oz_mcts_set_roots(self.h, self.oz.p_u64(a), self.oz.p_u64(b), act))

    def simulate_rc(self, net, nsims):
        return self.lib.oz_mcts_simulate(self.h, net._h, int(nsims))

    def simulate(self, net, nsims):
        self.oz.check(self.simulate_rc(net, nsims))

    def collect(self):
        out = np.zeros(2, np.int64)
        self.oz.check(self.lib.oz_mcts_collect(self.h, self.oz.p_i64(out)))
        return int(out[0]), int(out[1])

    def num_nodes(self):
        nn = np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_num_nodes(self.h, self.oz.p_i32(nn)))
        return nn

    def node(self, g, i):
        """everything the library tells of node i of slot g, as a tuple of hashable bits: key, Ns, legal, N, Q, tags, P, vhat, proofs"""
        own, opp, legal, Ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
        Nn, Q, qt, P = np.zeros(64, np.int32), np.zeros(64, np.float64), np.zeros(64, np.uint8), np.zeros(64, np.float64)
        self.oz.check(self.lib.oz_mcts_dump_node(self.h, g, i, C.byref(own), C.byref(opp), C.byref(Ns), C.byref(legal),
                                                 self.oz.p_i32(Nn), self.oz.p_f64(Q), self.oz.p_u8(qt), self.oz.p_f64(P)))
        out = [own.value, opp.value, Ns.value, legal.value, Nn.tobytes(), Q.tobytes(), qt.tobytes(), P.tobytes()]
        if self.vhat:
            v = C.c_double(-9.0)
            self.oz.check(self.lib.oz_mcts_node_value(self.h, g, i, C.byref(v)))
            out.append(np.float64(v.value).tobytes())
        if self.proofs:
            edge, value, val = np.zeros(64, np.int8), C.c_int8(), C.c_int8()
            self.oz.check(self.lib.oz_mcts_dump_proofs(self.h, g, i, self.oz.p_i8(edge), C.byref(value), C.byref(val)))
            out += [edge.tobytes(), value.value, val.value]
        return tuple(out)

    def dump(self, g):
        return [self.node(g, i) for i in range(int(self.num_nodes()[g]))]

    def counts(self):
        cnt, legal, rc = np.zeros((self.G, 64), np.int32), np.zeros(self.G, np.uint64), np.zeros(self.G, np.int32)
        self.oz.check(self.lib.oz_mcts_root_counts(self.h, self.oz.p_i32(cnt), self.oz.p_u64(legal), self.oz.p_i32(rc)))
        return cnt, rc

    def last_values(self):
        v = np.zeros(self.G, np.float64)
        self.oz.check(self.lib.oz_mcts_last_value(self.h, self.oz.p_f64(v), None, None))
        return v


class FilteredDump:
    """the dump of one slot of an object that never collects, filtered by the rule: node order is append-only there, so the keys are read
    once per node and only the kept nodes are read in full"""

    def __init__(self, search, g):
        self.s, self.g, self.keys = search, g, []

    def under(self, root):
        nn = int(self.s.num_nodes()[self.g])
        for i in range(len(self.keys), nn):
            self.keys.append(self.s.node(self.g, i)[:2])
        return [self.s.node(self.g, i) for i, k in enumerate(self.keys) if tree_keep(root, k)], nn


def squares(mask):
    return [s for s in range(64) if (mask >> s) & 1]


def play_without_collection(oz, net, cfg, start, rule):
    """object A: the whole game, after every move its dump filtered under that move's root -> (trace, final node count)"""
    A = Search(oz, 1, 1024, **cfg)
    fd = FilteredDump(A, 0)
    own, opp = start
    trace, ply, passes, total = [], 0, 0, 0
    while legal_mask(own, opp, N) != 0:
        A.set_roots([(own, opp)])
        A.simulate(net, SIMS)
        nodes, total = fd.under((own, opp))
        (cnt, rc), last = A.counts(), A.last_values()
        trace.append(dict(root=(own, opp), nodes=nodes, counts=cnt[0].copy(), rc=int(rc[0]), last=float(last[0])))
        legal = squares(legal_mask(own, opp, N))
        if rule == "search":
            sq = int(np.argmax(cnt[0]))                                 # the first maximum of the root's counts
        elif rule == "alternate":
            sq = legal[0] if ply % 2 == 0 else legal[-1]
        else:
            sq = legal[0]
        assert sq in legal
        nxt = next_state(own, opp, N, sq)
        if legal_mask(nxt[0], nxt[1], N) != 0 and same_mover(own, nxt):
            passes += 1
        own, opp = nxt
        ply += 1
    return trace, total, passes


def same_mover(own, nxt):
    """the opponent had to pass: next_state swaps the sides unless it did, and a mover's discs only grow with its move"""
    return (nxt[0] & own) == own


def collected_replay(oz, net, cfg, trace, cap):
    """object B: the same roots, oz_mcts_collect before every move's simulations; equality with A's filtered dump after every move"""
    B = Search(oz, 1, cap, **cfg)
    for i, t in enumerate(trace):
        B.set_roots([t["root"]])
        before, kept = B.collect()
        assert before >= kept >= 0, i
        assert int(B.num_nodes()[0]) == kept, i
        first = B.dump(0)
        assert B.collect() == (kept, kept), i                          # a second collection straight after the first changes nothing
        assert B.dump(0) == first, i
        B.simulate(net, SIMS)
        assert int(B.num_nodes()[0]) == len(t["nodes"]), (i, int(B.num_nodes()[0]), len(t["nodes"]))
        assert B.dump(0) == t["nodes"], i
        (cnt, rc), last = B.counts(), B.last_values()
        assert np.array_equal(cnt[0], t["counts"]) and int(rc[0]) == t["rc"], i
        assert np.float64(last[0]).tobytes() == np.float64(t["last"]).tobytes(), i
    return B


def overflows_without_collection(oz, net, cfg, trace, cap):
    """object C: B's capacity and no collection -> the library's capacity error (an error flag it has always raised)"""
    Cc = Search(oz, 1, cap, **cfg)
    for t in trace:
        Cc.set_roots([t["root"]])
        rc = Cc.simulate_rc(net, SIMS)
        if rc == oz.OZ_ERR_CAPACITY:
            return True
        assert rc == oz.OZ_OK, rc
    return False


# every configuration plays the game its own search picks; three of them also a game from the start position whose moves are fixed
# (the lowest legal square on even plies, the highest on odd ones) and which contains passes at 6x6
GAMES = [(c, "search") for c in CONFIGS] + [(c, "alternate") for c in ("k1-reference", "k4-sound", "proofs-solve6")]


@pytest.mark.parametrize("config,rule", GAMES, ids=[f"{c}-{r}" for c, r in GAMES])
def test_node_for_node_over_a_game(oz, net, config, rule):
    cfg = CONFIGS[config]
    trace, total, passes = play_without_collection(oz, net, cfg, initial_board(N), rule)
    if rule == "alternate":
        assert passes >= 1                                             # the sequence with a pass
    cap = max(len(t["nodes"]) for t in trace) + SIMS                    # live + 24 of every move
    assert cap < total, (cap, total)
    collected_replay(oz, net, cfg, trace, cap)
    assert overflows_without_collection(oz, net, cfg, trace, cap)


@pytest.mark.parametrize("config", ["k1-reference", "k1-sound", "proofs-solve6"])
@pytest.mark.parametrize("position", [1, 2])
def test_node_for_node_across_passes_near_the_end(oz, net, config, position):
    """the 8-empties positions of the value-signs tests, played by the lowest legal square: position 1 passes twice, position 2 five times
    in six plies.  The trees are tiny there, so nothing is claimed about the capacity: the equality alone."""
    cfg = CONFIGS[config]
    trace, total, passes = play_without_collection(oz, net, cfg, POSITIONS_6[position], "lowest")
    assert passes == {1: 2, 2: 5}[position]
    collected_replay(oz, net, cfg, trace, max(len(t["nodes"]) for t in trace) + SIMS)


def test_64_slots_at_different_plies(oz, net):
    """one object, 64 slots: every slot plays its own fixed game, a third of the slots sits out each round, some roots jump two plies ahead
    (not in the table).  Slot by slot the collecting object equals the filtered dump of the one that never collects; a slot that is
    inactive in a round is untouched."""
    G, sims, rounds = 64, 10, 4
    A, B = Search(oz, G, 256), Search(oz, G, 256)
    fds = [FilteredDump(A, g) for g in range(G)]
    pos = [initial_board(N) for _ in range(G)]
    for g in range(G):                                                  # different plies: slot g starts g % 7 plies into its game
        for _ in range(g % 7):
            pos[g] = next_state(*pos[g], N, squares(legal_mask(*pos[g], N))[g % 2 - 1])
    last_root = [None] * G
    for r in range(rounds):
        active = [1 if (g + r) % 3 != 0 else 0 for g in range(G)]
        idle = [g for g in range(G) if not active[g]]
        for s in (A, B):
            s.set_roots(pos, active)
        before = {g: B.dump(g) for g in idle[:6]}
        nb, nk = B.collect()
        assert nb >= nk
        for g in idle[:6]:
            assert B.dump(g) == before[g], (r, g)
        for s in (A, B):
            s.simulate(net, sims)
        for g in range(G):
            if active[g]:
                last_root[g] = pos[g]
        nn = B.num_nodes()
        for g in range(G):
            if last_root[g] is None:
                assert nn[g] == 0, (r, g)
                continue
            want, _ = fds[g].under(last_root[g])
            assert nn[g] == len(want), (r, g)
            if g % 4 == r % 4 or r == rounds - 1:                       # the full dump of a quarter of the slots per round, of all at the end
                assert B.dump(g) == want, (r, g)
        ca, cb = A.counts(), B.counts()
        act = np.array(active, bool)
        assert np.array_equal(ca[0][act], cb[0][act]) and np.array_equal(ca[1][act], cb[1][act]), r
        assert A.last_values()[act].tobytes() == B.last_values()[act].tobytes(), r
        for g in range(G):                                              # on: one ply, or two for every fifth slot (its next root was never searched from)
            for _ in range(2 if g % 5 == 0 else 1):
                legal = squares(legal_mask(*pos[g], N))
                if active[g] and legal:
                    pos[g] = next_state(*pos[g], N, legal[(g + r) % len(legal)])
        assert all(legal_mask(*p, N) for p in pos)                      # (no game is over after so few plies: no root ever goes back)
    st = oz.TreeGcStats()
    oz.check(oz.load().oz_mcts_tree_gc_stats(B.h, C.byref(st)))
    assert st.collections > 0 and st.nodes_before_sum > st.nodes_kept_sum > 0 and st.peak_nodes >= st.peak_kept > 0


# ---------------------------------------------------------------- the engine
ROUNDS = 64                                                             # a 6x6 game has at most 32 plies: about two games per slot
ENGINE_VARIANTS = {
    "plain": {},
    "k4": dict(leaves_per_step=4),
    "noise-sampling-cap": dict(root_noise=(0.5, 0.25), sample_moves=(1.0, 6), playout_cap=(8, 0.5)),
    "gumbel": dict(gumbel=(4, 50.0, 1.0)),
    "proofs-play-solve": dict(value_signs="sound", proofs=True, proof_play=True, solve_leaves=6),
    "resign": dict(resign=(0.9, 3, 10, 0.25)),
}


def engine_run(net, tree_gc, node_cap, opts):
    from othellozero_amd.training import SelfPlayEngine
    eng = SelfPlayEngine(net, N, 64, SIMS, 1.0, 1.0, 0.9, seed=77, refill=True, node_cap=node_cap, record_visits=True, record_values=True,
                         tree_gc=tree_gc, **opts)
    eng.run(ROUNDS)
    rows = eng.records(with_visits=True, with_values=True, with_policies="gumbel" in opts)
    return dict(stats=eng.stats(), rows=tuple(np.ascontiguousarray(x).tobytes() for x in rows), last=eng.last_counts().tobytes(),
                gc=eng.tree_gc_stats())


@pytest.mark.parametrize("variant", list(ENGINE_VARIANTS))
def test_engine_records_are_those_of_off(oz, net, variant):
    opts = ENGINE_VARIANTS[variant]
    off = engine_run(net, "off", 0, opts)
    assert off["stats"]["overflow"] == 0 and off["stats"]["games_completed"] >= 64
    assert off["gc"] == dict(mode="off", collections=0, nodes_before_sum=0, nodes_kept_sum=0, peak_nodes=0, peak_kept=0)
    every = engine_run(net, "every", 0, opts)
    demand = engine_run(net, "demand", 0, opts)
    for got in (every, demand):
        assert got["stats"] == off["stats"] and got["rows"] == off["rows"] and got["last"] == off["last"]
    assert every["gc"]["collections"] > 0 and every["gc"]["peak_nodes"] >= every["gc"]["peak_kept"] > 0
    assert demand["gc"]["collections"] == 0                             # the default capacity holds a whole game: nothing is ever due
    cap = every["gc"]["peak_kept"] + 2 * SIMS
    small = engine_run(net, "demand", cap, opts)
    assert small["stats"] == off["stats"] and small["rows"] == off["rows"] and small["last"] == off["last"]
    assert small["gc"]["collections"] > 0 and small["gc"]["peak_nodes"] <= cap
    with pytest.raises(oz.OzError) as e:
        engine_run(net, "off", cap, opts)
    assert e.value.code == oz.OZ_ERR_CAPACITY


def test_arena_with_a_mode_per_agent(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.agents import arena_batch
    a, b = StubNetWrapper((N, N), salt=3, max_batch=16), StubNetWrapper((N, N), salt=4, max_batch=16)
    keys = ("winner", "points", "n_moves", "actions", "players", "final_black", "final_white", "stats_black", "stats_white")

    def same(x, y):
        assert all(np.array_equal(x[k], y[k]) for k in keys) and x["leaves_evaluated"] == y["leaves_evaluated"]
    off = arena_batch(a, b, N, 16, 32, seed=3)
    assert "tree_gc_stats" not in off
    mixed = arena_batch(a, b, N, 16, 32, seed=3, tree_gc=("every", "demand"))
    same(off, mixed)
    black, white = mixed["tree_gc_stats"]
    assert black["collections"] > 0 and white["collections"] == 0
    cap = black["peak_kept"] + 2 * 32 + 32                              # (the other agent's trees are of the same kind; a margin of one move)
    small = arena_batch(a, b, N, 16, 32, seed=3, tree_gc=("demand", "every"), node_cap=cap)
    same(off, small)
    assert small["tree_gc_stats"][0]["collections"] > 0 and small["tree_gc_stats"][1]["collections"] > 0
    with pytest.raises(oz.OzError) as e:
        arena_batch(a, b, N, 16, 32, seed=3, node_cap=cap)
    assert e.value.code == oz.OZ_ERR_CAPACITY


def test_drop_in_search_through_execute_episode(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import execute_episode
    net1 = StubNetWrapper((N, N), salt=SALT, max_batch=1)

    def episode(**kw):
        random.seed(4)
        np.random.seed(4)
        return execute_episode(N, net1, 1.0, SIMS, 1.0, 0.9, snapshot_boards=True, policy_target="visits", **kw)

    def same(x, y):
        assert len(x) == len(y)
        for (b0, p0, z0), (b1, p1, z1) in zip(x, y):
            assert np.array_equal(b0, b1) and np.asarray(p0).tobytes() == np.asarray(p1).tobytes() and z0 == z1
    off = episode()
    cap = 160                                                           # a whole game's nodes at 24 simulations: about 640
    same(off, episode(tree_gc="every", node_cap=cap))
    same(off, episode(tree_gc="demand", node_cap=cap))
    with pytest.raises(oz.OzError) as e:
        episode(node_cap=cap)
    assert e.value.code == oz.OZ_ERR_CAPACITY


def test_refusals_in_both_orders(oz, net):
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()

    def refused(call, word):
        with pytest.raises(oz.OzError) as e:
            call()
        assert e.value.code == oz.OZ_ERR_STATE and word in str(e.value), str(e.value)
    mk = lambda **kw: SelfPlayEngine(net, N, 8, 8, 1.0, 1.0, 0.9, seed=5, refill=True, **kw)      # noqa: E731
    eng = mk(tree_gc="demand")
    refused(lambda: eng.run_steps(2), "oz_selfplay_run_steps")
    refused(lambda: eng.stagger(), "oz_selfplay_stagger")
    eng.run(2)                                                          # the engine stays usable
    assert eng.stats()["moves"] == 16
    for drive, again in ((lambda e: e.run(1), lambda e: e.run(1)), (lambda e: e.run_steps(4), lambda e: e.run_steps(40)),
                         (lambda e: e.stagger(4), lambda e: e.run(1))):
        eng = mk()
        drive(eng)
        refused(lambda: oz.check(lib.oz_selfplay_set_tree_gc(eng._h, 2)), "oz_selfplay_set_tree_gc")
        moves = eng.stats()["moves"]
        again(eng)
        assert eng.stats()["moves"] > moves and eng.tree_gc_stats()["mode"] == "off"
    eng = mk()
    assert lib.oz_selfplay_set_tree_gc(eng._h, 3) == oz.OZ_ERR_ARG
    # the bare search: no collection while a host-evaluated step is pending
    s = Search(oz, 2, 64)
    s.set_roots([initial_board(N)] * 2)
    oz.check(lib.oz_mcts_select(s.h))
    refused(s.collect, "oz_mcts_collect")
    pi, v = np.full((2, N * N), 1.0 / (N * N), np.float32), np.zeros(2, np.float32)
    oz.check(lib.oz_mcts_backup(s.h, oz.p_f32(pi), oz.p_f32(v)))
    assert s.collect() == (2, 2)
    s.simulate(net, 4)


def test_off_is_off(oz, net):
    """an engine given "off" through the setter arms nothing, counts nothing and issues the launches of an engine that never heard of it
    (the scratch map itself is not visible through the interface: the counters that live beside it read zero and no launch is timed)"""
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    out = []
    for setter in (False, True):
        eng = SelfPlayEngine(net, N, 16, 12, 1.0, 1.0, 0.9, seed=9, refill=True)
        if setter:
            oz.check(lib.oz_selfplay_set_tree_gc(eng._h, 0))
        eng.profile(True)
        eng.tree_gc_profile(True)
        eng.run(6)
        launches = {k: c for k, (_, c) in eng.profile_read().items()}
        assert eng.tree_gc_profile_read() == (0.0, 0)
        assert eng.tree_gc_stats() == dict(mode="off", collections=0, nodes_before_sum=0, nodes_kept_sum=0, peak_nodes=0, peak_kept=0)
        out.append((launches, eng.stats(), eng.records().tobytes()))
    assert out[0] == out[1]
    on = SelfPlayEngine(net, N, 16, 12, 1.0, 1.0, 0.9, seed=9, refill=True, tree_gc="every")
    on.profile(True)
    on.tree_gc_profile(True)
    on.run(6)
    assert {k: c for k, (_, c) in on.profile_read().items()} == out[0][0]       # no slot of the tree kernels' profile is added or counted twice
    ms, count = on.tree_gc_profile_read()
    assert count == 6 and ms > 0.0
    assert on.records().tobytes() == out[0][2]
