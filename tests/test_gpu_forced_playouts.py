"""Forced playouts and policy target pruning on the GPU (pytest -m gpu): the search against ForcedWideSearch (tests/forced_playouts_ref.py) bit
for bit, the pruned rows against the restatement's prune, off-means-off, the lock-step engine round by round, the drivers, a playout cap next
to it, the refusals and the Python surface.  Stub network, a handful of games, a few dozen simulations."""
import ctypes as C
import random

import numpy as np
import pytest

import forced_playouts_ref as ref
from forced_playouts_ref import ForcedWideSearch
from root_noise_ref import NoisyWideSearch
from test_gpu_wide_search import Search, _golden_roots
from wide_search_ref import assert_same_tables, legal_mask, tie_draw

pytestmark = pytest.mark.gpu

ALPHA, EPS, KF = ref.SEARCH_ALPHA, ref.SEARCH_EPS, ref.SEARCH_K


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _set_noise(oz, s, eps, eta):
    return s.lib.oz_mcts_set_root_noise(s.h, float(eps), oz.p_f64(np.ascontiguousarray(eta, np.float64)), None)


def _set_forced(s, k):
    return s.lib.oz_mcts_set_forced_playouts(s.h, float(k))


def _get_forced(s):
    k = C.c_double(-1.0)
    s.oz.check(s.lib.oz_mcts_get_forced_playouts(s.h, C.byref(k)))
    return k.value


def _pruned(s):
    cnt, legal, rc = np.zeros((s.G, 64), np.int32), np.zeros(s.G, np.uint64), np.zeros(s.G, np.int32)
    s.oz.check(s.lib.oz_mcts_pruned_counts(s.h, s.oz.p_i32(cnt), s.oz.p_u64(legal), s.oz.p_i32(rc)))
    return cnt, legal, rc


def _mode_search(oz, n, G, mode):
    K = mode if isinstance(mode, int) else 1
    s = Search(oz, n, G)
    if mode == "wide1":
        oz.check(s.lib.oz_mcts_use_wide_kernels(s.h, 1))
    elif K > 1:
        oz.check(s.set_k(K))
    return s, K


# ------------------------------------------------------------------ 1. the search with host-supplied eta, bit for bit
@pytest.mark.parametrize("mode", ["narrow", "wide1", 4, 16])
@pytest.mark.parametrize("n", [6, 8])
def test_forced_search_vs_restatement(oz, n, mode):
    from othellozero_amd.NNet import StubNetWrapper
    G = ref.SEARCH_G
    s, K = _mode_search(oz, n, G, mode)
    roots, eta, refs = ref.search_case(n, K)
    forced, changed = ref.case_is_not_vacuous(n, K)
    assert forced >= 1 and changed >= 1, (n, mode, forced, changed)          # the restatement alone says that forcing and pruning happen here
    net = StubNetWrapper((n, n), ref.SEARCH_SALT, 0, max_batch=G * K)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(_set_noise(oz, s, EPS, eta))
    oz.check(_set_forced(s, KF))
    assert _get_forced(s) == KF
    oz.check(s.simulate(net, ref.SEARCH_SIMS))
    for gi in range(G):
        assert_same_tables(s.dump(gi), refs[gi], (n, mode, gi))
    assert s.stats()[0] == sum(r.sims for r in refs)
    if mode != "narrow":
        assert s.wide_stats() == tuple(sum(getattr(r, k) for r in refs) for k in ("steps", "collisions", "leaves"))
    raw = s.counts()
    got, legal, rc = _pruned(s)
    assert not rc.any()
    differ = 0
    for gi, (o, p) in enumerate(roots):
        assert np.array_equal(raw[gi], refs[gi].root_row(o, p)[0]), (n, mode, gi)
        assert np.array_equal(got[gi], refs[gi].pruned(o, p)), (n, mode, gi, got[gi], refs[gi].pruned(o, p))
        assert int(legal[gi]) == legal_mask(o, p, n)
        differ += int(not np.array_equal(got[gi], raw[gi]))
    assert differ == changed
    # another board in slot 0: its noise goes with the old one, and with it the pruning of that slot alone
    other = _golden_roots(n, 8)[7]
    assert other not in roots
    s.set_roots([other[0]] + [r[0] for r in roots[1:]], [other[1]] + [r[1] for r in roots[1:]], [1, 0, 0, 0])
    oz.check(s.simulate(net, 5))
    got2, _, rc2 = _pruned(s)
    assert not rc2.any() and np.array_equal(got2[0], s.counts()[0]) and np.array_equal(got2[1:], got[1:])


# ------------------------------------------------------------------ 2. off means off
def _engine(net, G, K=1, n=6, sims=16, seed=77, first=300, temperature=0.0, e_greedy=1.0, **kw):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, n, G, sims, 1.0, temperature, e_greedy, seed=seed, first_game_id=first, leaves_per_step=K, record_visits=True,
                          root_noise=(ALPHA, EPS), **kw)


@pytest.mark.parametrize("K", [1, 4])
def test_off_means_off(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 4
    lib = oz.load()
    net = StubNetWrapper((n, n), 21, 0, max_batch=G * K)

    def played(setter, **kw):
        eng = _engine(net, G, K, temperature=1.0, e_greedy=0.85, **kw)
        if setter is not None:
            oz.check(lib.oz_selfplay_set_forced_playouts(eng._h, setter))
        eng.run(3)
        last = eng.last_counts()
        rec, rows = eng.play_to_end(with_visits=True)
        return rec.tobytes(), rows.tobytes(), last.tobytes(), eng.forced_playout_stats()
    today = played(None)                                   # an engine that never hears of the option
    assert len(today[0]) > 0
    for setter, kw in ((0.0, {}), (None, dict(forced_playouts=0)), (None, dict(forced_playouts=None))):
        got = played(setter, **kw)
        assert got[:3] == today[:3], (K, setter, kw)
        assert got[3] == dict(k=0.0, moves_pruned=0, visits_raw=0, visits_kept=0)
    assert played(KF)[:2] != today[:2]                     # ... and on, it is another run
    # the node tables of a bare search: k = 0 and never set are the noisy search of today
    roots, eta, _ = ref.search_case(n, K)
    want = []
    for gi, (o, p) in enumerate(roots):
        r = NoisyWideSearch(n, 1.0, K, salt=ref.SEARCH_SALT)
        r.set_noise(o, p, eta[gi], EPS)
        r.simulate(o, p, ref.SEARCH_SIMS)
        want.append(r)
    snet = StubNetWrapper((n, n), ref.SEARCH_SALT, 0, max_batch=ref.SEARCH_G * K)
    for k in (None, 0.0):
        s, _ = _mode_search(oz, n, ref.SEARCH_G, K if K > 1 else "narrow")
        s.set_roots([r[0] for r in roots], [r[1] for r in roots])
        oz.check(_set_noise(oz, s, EPS, eta))
        if k is not None:
            oz.check(_set_forced(s, k))
        assert _get_forced(s) == 0.0
        oz.check(s.simulate(snet, ref.SEARCH_SIMS))
        for gi in range(ref.SEARCH_G):
            assert_same_tables(s.dump(gi), want[gi], (K, k, gi))
        assert np.array_equal(_pruned(s)[0], s.counts())


# ------------------------------------------------------------------ 3. the lock-step engine, round by round
def _round_by_round(oz, eng, W, n, G, sims, seed, cap=None):
    """plays the engine to the end one round at a time next to the restatements W -> {(game id, ply): (raw row, pruned row, full)}; checks
    last_counts and the move of every round"""
    rows = {}
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
            budget = sims if cap is None else int(oz.playout_budgets(seed, [gid], [ply], sims, cap)[0])
            full = budget == sims
            assert bool(armed[g]) == full, (rnd, g)
            if full:
                W[g].set_noise(own, opp, eta[g], EPS)      # the device's own eta: the counts must then agree exactly
            else:
                W[g].clear_noise()                         # a fast move: no noise, so nothing forced and nothing pruned
            W[g].simulate(own, opp, budget)
            raw = W[g].counts(own, opp)[0]
            assert np.array_equal(cnt[g], raw), (rnd, g, cnt[g][raw > 0], raw[raw > 0])          # last_counts stays on the raw counts
            placed = (int(after["black"][g]) | int(after["white"][g])) & ~(b | w)
            assert placed == 1 << W[g].best_move(own, opp, tie_draw(seed, gid, ply)), (rnd, g)   # ... and so does the move
            rows[(gid, ply)] = (raw, W[g].pruned(own, opp), full)
    assert eng.stats()["live_games"] == 0
    return rows


@pytest.mark.parametrize("K", [1, 4])
def test_lockstep_engine_round_by_round(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims, seed, first, salt = 6, 6, 16, 77, 300, 21
    net = StubNetWrapper((n, n), salt, 0, max_batch=G * K)
    eng = _engine(net, G, K, n=n, sims=sims, seed=seed, first=first, forced_playouts=KF)
    W = [ForcedWideSearch(n, 1.0, K, salt=salt, k=KF) for _ in range(G)]
    want = _round_by_round(oz, eng, W, n, G, sims, seed)
    rec, rows = eng.records(with_visits=True)
    assert rec.size == len(want) == eng.stats()["moves"]
    changed = 0
    for r, row in zip(rec, rows):
        raw, pruned, _ = want[(int(r["game_id"]), int(r["ply"]))]
        assert np.array_equal(row, pruned), (int(r["game_id"]), int(r["ply"]), row[raw > 0], pruned[raw > 0], raw[raw > 0])
        changed += int(not np.array_equal(raw, pruned))
    forced = sum(w.forced for w in W)
    st = eng.forced_playout_stats()
    print(f"K = {K}: {rec.size} moves, {forced} forced descents, {changed} rows changed, visits {st['visits_raw']} -> {st['visits_kept']}")
    assert forced >= 1 and changed >= 1
    assert st == dict(k=KF, moves_pruned=changed, visits_raw=sum(int(v[0].sum()) for v in want.values()),
                      visits_kept=sum(int(v[1].sum()) for v in want.values()))
    assert int(rows.sum()) == st["visits_kept"] < st["visits_raw"]


# ------------------------------------------------------------------ 4. the drivers
def _free_run(eng):
    for _ in range(300):
        eng.run_steps(32)
        if eng.stats()["live_games"] == 0:
            break
    assert eng.stats()["live_games"] == 0
    return eng


def test_drivers_and_determinism(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 8
    net = StubNetWrapper((n, n), 5, 0, max_batch=G)
    kw = dict(n=n, sims=12, seed=41, first=16, temperature=1.0, e_greedy=0.85, forced_playouts=KF)
    a = _engine(net, G, **kw)
    rec, rows = a.play_to_end(with_visits=True)
    b = _engine(net, G, **kw)
    rec2, rows2 = b.play_to_end(with_visits=True)
    assert rec.size > 0 and rec.tobytes() == rec2.tobytes() and rows.tobytes() == rows2.tobytes()          # two runs, one seed
    assert a.forced_playout_stats() == b.forced_playout_stats() and a.forced_playout_stats()["moves_pruned"] >= 1
    free = _free_run(_engine(net, G, **kw))
    frec, frows = free.records(with_visits=True)
    assert frec.tobytes() == rec.tobytes() and frows.tobytes() == rows.tobytes()                           # run_steps: the records and rows of run
    assert free.forced_playout_stats() == a.forced_playout_stats()
    one = _engine(net, 1, **dict(kw, first=19))                                                           # another engine size, another slot
    orec, orows = one.play_to_end(with_visits=True)
    pick = rec["game_id"] == 19
    assert orec.size > 0 and orec.tobytes() == rec[pick].tobytes() and orows.tobytes() == rows[pick].tobytes()
    # a staggered engine forces and prunes its rounds too (they draw noise)
    from othellozero_amd.training import SelfPlayEngine
    st = SelfPlayEngine(net, n, G, 12, 1.0, 1.0, 0.85, seed=41, first_game_id=16, refill=True, record_visits=True, root_noise=(ALPHA, EPS),
                        forced_playouts=KF)
    st.stagger(8)
    fs = st.forced_playout_stats()
    assert fs["visits_raw"] > 0 and fs["visits_kept"] <= fs["visits_raw"] and st.stats()["moves"] > 0


# ------------------------------------------------------------------ 5. next to a playout cap
def test_fast_moves_are_neither_forced_nor_pruned(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims, seed, first, salt, cap = 6, 6, 16, 77, 300, 21, (4, 0.5)
    net = StubNetWrapper((n, n), salt, 0, max_batch=G)
    eng = _engine(net, G, 1, n=n, sims=sims, seed=seed, first=first, forced_playouts=KF, playout_cap=cap)
    W = [ForcedWideSearch(n, 1.0, 1, salt=salt, k=KF) for _ in range(G)]
    want = _round_by_round(oz, eng, W, n, G, sims, seed, cap=cap)
    rec, rows = eng.records(with_visits=True)
    assert rec.size == len(want)
    fast = oz.record_fast(rec)
    full_changed = 0
    for r, row, f in zip(rec, rows, fast):
        raw, pruned, full = want[(int(r["game_id"]), int(r["ply"]))]
        assert bool(f) != full
        if full:
            assert np.array_equal(row, pruned)
            full_changed += int(not np.array_equal(raw, pruned))
        else:
            assert np.array_equal(row, raw) and np.array_equal(raw, pruned)                                 # a fast move's row is raw
    st, ps = eng.forced_playout_stats(), eng.playout_stats()
    assert 0 < ps["fast_moves"] == int(fast.sum()) and ps["full_moves"] == int((fast == 0).sum()) > 0
    assert st["moves_pruned"] == full_changed >= 1
    assert st["visits_raw"] == sum(int(v[0].sum()) for v in want.values() if v[2])
    assert st["visits_kept"] == sum(int(v[1].sum()) for v in want.values() if v[2]) <= st["visits_raw"]
    # the free-running driver under both options: the same records and rows
    free = _free_run(_engine(net, G, 1, n=n, sims=sims, seed=seed, first=first, forced_playouts=KF, playout_cap=cap))
    frec, frows = free.records(with_visits=True)
    assert frec.tobytes() == rec.tobytes() and frows.tobytes() == rows.tobytes() and free.forced_playout_stats() == st


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_objects_usable(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    n, K = 6, 1
    roots, eta, refs = ref.search_case(n, K)
    G = ref.SEARCH_G
    net = StubNetWrapper((n, n), ref.SEARCH_SALT, 0, max_batch=G)
    s = Search(oz, n, G)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    assert _set_forced(s, KF) == oz.OZ_ERR_STATE and "noise" in lib.oz_last_error().decode()          # before root noise
    assert _set_forced(s, 0.0) == oz.OZ_OK and _get_forced(s) == 0.0                                  # switching off needs nothing
    oz.check(_set_noise(oz, s, EPS, eta))
    for bad in (-0.5, 16.5, float("nan"), float("inf")):
        assert _set_forced(s, bad) == oz.OZ_ERR_ARG and "k" in lib.oz_last_error().decode()
    assert _get_forced(s) == 0.0
    oz.check(lib.oz_mcts_select(s.h))                                                                 # a change while a step is pending
    assert _set_forced(s, KF) == oz.OZ_ERR_STATE and "pending" in lib.oz_last_error().decode()
    import oracle
    status, lo, lp = np.zeros(G, np.int32), np.zeros(G, np.uint64), np.zeros(G, np.uint64)
    pi, v = np.zeros((G, n * n), np.float32), np.zeros(G, np.float32)
    oz.check(lib.oz_mcts_leaves(s.h, oz.p_i32(status), oz.p_u64(lo), oz.p_u64(lp)))
    for gi in range(G):
        p, val = oracle.stub_predict(int(lo[gi]), int(lp[gi]), n, ref.SEARCH_SALT, 0)
        pi[gi], v[gi] = p.ravel(), val
    oz.check(lib.oz_mcts_backup(s.h, oz.p_f32(pi), oz.p_f32(v)))
    # ... and the object is usable: forced now, it is the restatement's search (its first simulation forces nothing: the root is new)
    oz.check(_set_forced(s, KF))
    oz.check(s.simulate(net, ref.SEARCH_SIMS - 1))
    for gi in range(G):
        assert_same_tables(s.dump(gi), refs[gi], ("after refusals", gi))
    # the engine
    eng = SelfPlayEngine(net, n, G, 8, record_visits=True)
    assert lib.oz_selfplay_set_forced_playouts(eng._h, KF) == oz.OZ_ERR_STATE and "noise" in lib.oz_last_error().decode()
    oz.check(lib.oz_selfplay_set_root_noise(eng._h, ALPHA, EPS))
    for bad in (-1.0, 17.0, float("nan")):
        assert lib.oz_selfplay_set_forced_playouts(eng._h, bad) == oz.OZ_ERR_ARG
    oz.check(lib.oz_selfplay_set_forced_playouts(eng._h, KF))
    eng.run(1)
    assert lib.oz_selfplay_set_forced_playouts(eng._h, 1.0) == oz.OZ_ERR_STATE and "driven" in lib.oz_last_error().decode()
    assert lib.oz_selfplay_set_forced_playouts(eng._h, 0.0) == oz.OZ_ERR_STATE
    eng.run(1)
    assert eng.forced_playout_stats()["k"] == KF and eng.stats()["moves"] == 2 * G


# ------------------------------------------------------------------ 7. the Python surface
def test_host_evaluator_split_honours_forcing(oz):
    """OthelloMCTS with a duck-typed network: oz_mcts_select / leaves / backup run the same descent; pruned_counts is the restatement's row"""
    import oracle
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    n, K = 6, 1
    roots, eta, refs = ref.search_case(n, K)
    own, opp = roots[2]

    class HostNet:
        network_type = None

        def predict(self, board):
            o, p = oz.pack_board(board)
            return oracle.stub_predict(o, p, n, ref.SEARCH_SALT, 0)
    m = OthelloMCTS(n, HostNet(), 1.0, node_cap=256, forced_playouts=KF)
    state = oz.unpack_board(own, opp, n)
    m.set_root_noise(eta[2], EPS, state=state, player=OthelloPlayer.BLACK)
    m.simulate_n(state, OthelloPlayer.BLACK, ref.SEARCH_SIMS)
    assert_same_tables(m.dump(), refs[2], "host evaluator")
    want = refs[2].pruned(own, opp)
    assert np.array_equal(m.pruned_counts(state), want)
    pol = m.get_policy_action_probabilities(state, 1.0, pruned=True)
    assert np.array_equal(pol, (want.reshape(8, 8)[:n, :n] / want.sum()).astype(np.float64))


def test_execute_episode_dropin_with_forced_playouts(oz):
    from othellozero_amd import training
    from othellozero_amd.NNet import StubNetWrapper
    n = 6
    net = StubNetWrapper((n, n), 17, 0, max_batch=1)

    def episode(**kw):
        random.seed(1)
        np.random.seed(1)
        return training.execute_episode(n, net, 1, 16, 1, 1.0, root_noise=(ALPHA, EPS), snapshot_boards=True, policy_target="visits", **kw)
    ex = episode(forced_playouts=2)
    assert len(ex) > 0 and len(ex) % 8 == 0 and all(abs(float(p.sum()) - 1.0) <= 1e-12 and z in (-1, 1) for _, p, z in ex)
    quiet = episode()
    assert len(ex) != len(quiet) or any(not np.array_equal(a[1], b[1]) for a, b in zip(ex, quiet))
    assert [e[1].tobytes() for e in episode(forced_playouts=0)] == [e[1].tobytes() for e in quiet]


def _loop_kw(tmp_path, n):
    return dict(board_size=n, num_iterations=1, num_episodes=6, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
                evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0, self_play_training=False, self_play_interval=1,
                self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "forced.h5"), training_buffer_size=8 * 40 * 6,
                seed=12, batched_evaluation=True, root_noise=(ALPHA, EPS), policy_target="visits", alias_final_boards=False, forced_playouts=2)


def _spy_engines(monkeypatch):
    from othellozero_amd import training
    made = []

    class Spy(training.SelfPlayEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(training, "SelfPlayEngine", Spy)
    return made


def test_training_loop_with_forced_playouts(oz, tmp_path, monkeypatch):
    """one tiny iteration: the argument reaches the self-play engine, whose rows are the pruned ones"""
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    random.seed(4)
    np.random.seed(4)
    n = 6
    made = _spy_engines(monkeypatch)
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8, policy_loss="flat")
    historic = loop.training(neural_network=net, **_loop_kw(tmp_path, n))
    assert len(historic) == 1 and len(made) == 1 and made[0].forced_playouts == 2.0 and made[0].root_noise == (ALPHA, EPS)
    st = made[0].forced_playout_stats()
    rec, rows = made[0].records(with_visits=True)
    print(f"{rec.size} records, {st}")
    assert st["k"] == 2.0 and st["moves_pruned"] >= 1 and int(rows.sum()) == st["visits_kept"] < st["visits_raw"]
    assert all(np.isfinite(a).all() for a in net.get_weights())


def test_training_loop_on_the_device_buffer_gets_the_pruned_rows(oz, tmp_path, monkeypatch):
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.replay import ReplayBuffer
    monkeypatch.chdir(tmp_path)
    random.seed(4)
    np.random.seed(4)
    n = 6
    made = _spy_engines(monkeypatch)
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8, policy_loss="flat")
    seen, orig = [], net.train

    def spy(examples, **k):
        assert isinstance(examples, ReplayBuffer)
        seen.append(examples.read())
        return orig(examples, **k)
    net.train = spy
    loop.training(neural_network=net, replay="device", **_loop_kw(tmp_path, n))
    assert len(made) == 1 and len(seen) == 1
    st = made[0].forced_playout_stats()
    rec, rows = made[0].records(with_visits=True)
    assert st["moves_pruned"] >= 1 and int(rows.sum()) == st["visits_kept"] < st["visits_raw"]            # the engine's rows are the pruned ones
    again = ReplayBuffer(n, 8 * 40 * 6)
    assert again.append_records(rec, rows, policy_target="visits") == rec.size                              # ... and they are what the buffer holds
    for a, b in zip(seen[0], again.read()):
        assert a.tobytes() == b.tobytes()
