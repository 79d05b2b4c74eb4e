"""Root noise on the GPU (pytest -m gpu): the device's Dirichlet sampler against the restatement in tests/root_noise_ref.py (1e-9: libm
ulps against differences of 1e-2 for a wrong stream, draw order or normaliser; that the accept / reject margins of these draws are >= 1e-6 is
checked without a GPU, test_root_noise_cpu.test_decision_margins_of_the_roots_the_gpu_test_draws_for), the
search with noise against NoisyWideSearch bit for bit, and the engines, drivers, refusals and drop-ins around them."""
import ctypes as C
import random

import numpy as np
import pytest

from root_noise_ref import NoisyWideSearch, dirichlet
from test_gpu_wide_search import Search, _first_max, _golden_roots
from wide_search_ref import WideSearch, assert_same_tables, legal_mask, next_state, popcount, tie_draw

pytestmark = pytest.mark.gpu

SAMPLER_ALPHAS = (0.03, 0.3, 1.0, 2.5)
SAMPLER_SEEDS = (1234, 77)
SAMPLER_FIRST_ID = 1000
SALT, EPS, ALPHA, ETA_SEED = 13, 0.25, 0.5, 5             # the search tests: stub network salt, mixing weight, and the restatement's draws


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _set_noise(oz, s, eps, eta, armed=None):
    e = None if eta is None else oz.p_f64(np.ascontiguousarray(eta, np.float64))
    a = None if armed is None else oz.p_u8(np.array(armed, np.uint8))
    return s.lib.oz_mcts_set_root_noise(s.h, float(eps), e, a)


def _sample(oz, s, alpha, eps, seed, ids, plies):
    return s.lib.oz_mcts_sample_root_noise(s.h, float(alpha), float(eps), int(seed), oz.p_u64(np.array(ids, np.uint64)),
                                           oz.p_i32(np.array(plies, np.int32)))


def _get_noise(oz, s):
    eta, armed, eps = np.zeros((s.G, 64), np.float64), np.zeros(s.G, np.uint8), C.c_double(-1.0)
    oz.check(s.lib.oz_mcts_get_root_noise(s.h, oz.p_f64(eta), oz.p_u8(armed), C.byref(eps)))
    return eta, armed, eps.value


def _ref_eta(n, roots, seed=ETA_SEED, ply=0, alpha=ALPHA):
    return np.array([dirichlet(n, legal_mask(o, p, n), alpha, seed, gi, ply)[0] for gi, (o, p) in enumerate(roots)])


# ------------------------------------------------------------------ 1. the sampler
@pytest.mark.parametrize("n", [6, 8])
def test_device_sampler_vs_restatement(oz, n):
    G = 64
    roots = _golden_roots(n, G)
    legal = [legal_mask(o, p, n) for o, p in roots]
    assert min(popcount(x) for x in legal) == 1 and max(popcount(x) for x in legal) >= 9          # one-move roots are among them
    ids = [SAMPLER_FIRST_ID + gi for gi in range(G)]
    plies = [popcount(o | p) - 4 for o, p in roots]
    s = Search(oz, n, G, node_cap=64)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    worst = 0.0
    for seed in SAMPLER_SEEDS:
        for alpha in SAMPLER_ALPHAS:
            oz.check(_sample(oz, s, alpha, EPS, seed, ids, plies))
            eta, armed, eps = _get_noise(oz, s)
            assert armed.all() and eps == EPS
            for gi in range(G):
                want = dirichlet(n, legal[gi], alpha, seed, ids[gi], plies[gi])[0]
                diff = float(np.abs(eta[gi] - want).max())
                worst = max(worst, diff)
                assert diff <= 1e-9, (n, seed, alpha, gi, diff)
                assert all(eta[gi][sq] == 0.0 for sq in range(64) if not (legal[gi] >> sq) & 1), (n, seed, alpha, gi)
                assert abs(float(eta[gi].sum()) - 1.0) <= 1e-12
                if popcount(legal[gi]) == 1:
                    assert eta[gi].max() == 1.0
    print(f"n = {n}: largest |eta_device - eta_restatement| over {len(SAMPLER_SEEDS) * len(SAMPLER_ALPHAS) * G} roots = {worst:.3e}")


# ------------------------------------------------------------------ 2. the search with host-supplied eta, bit for bit
@pytest.mark.parametrize("mode", ["narrow", "wide1", 4, 16])
@pytest.mark.parametrize("n", [6, 8])
def test_noisy_search_vs_restatement(oz, n, mode):
    from othellozero_amd.NNet import StubNetWrapper
    G, K = 8, (mode if isinstance(mode, int) else 1)
    roots = _golden_roots(n, G)
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G * K)
    s = Search(oz, n, G)
    if mode == "wide1":
        oz.check(s.lib.oz_mcts_use_wide_kernels(s.h, 1))
    elif K > 1:
        oz.check(s.set_k(K))
    refs = [NoisyWideSearch(n, 1.0, K, salt=SALT) for _ in range(G)]
    plain = [WideSearch(n, 1.0, K, salt=SALT) for _ in range(G)]
    first_roots = list(roots)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    live = [True] * G

    def arm(stage):
        eta = _ref_eta(n, roots, ply=stage)
        oz.check(_set_noise(oz, s, EPS, eta, [1 if x else 0 for x in live]))
        got, armed, eps = _get_noise(oz, s)
        assert np.array_equal(got, eta) and list(armed) == [1 if x else 0 for x in live] and eps == EPS
        for gi in range(G):
            refs[gi].set_noise(*roots[gi], eta[gi], EPS)

    def check(where):
        for gi in range(G):
            assert_same_tables(s.dump(gi), refs[gi], (n, mode, gi, where))
        assert s.stats()[0] == sum(r.sims for r in refs), where
        if mode != "narrow":
            assert s.wide_stats() == tuple(sum(getattr(r, k) for r in refs) for k in ("steps", "collisions", "leaves")), where

    arm(0)
    for nsims in (2, 25, 60):
        oz.check(s.simulate(net, nsims))
        for gi in range(G):
            refs[gi].simulate(*roots[gi], nsims)
            plain[gi].simulate(*roots[gi], nsims)
        check(("simulate", nsims))
    # not vacuous: the restatement alone says the noise changed where the visits went
    changed = sum(not np.array_equal(refs[gi].counts(*first_roots[gi])[0], plain[gi].counts(*first_roots[gi])[0]) for gi in range(G))
    assert changed >= 1, changed
    for mv in range(3):
        cnt = s.counts()
        for gi in range(G):
            if not live[gi]:
                continue
            assert np.array_equal(cnt[gi], refs[gi].counts(*roots[gi])[0]), (gi, mv)
            roots[gi] = next_state(*roots[gi], n, _first_max(cnt[gi]))
            live[gi] = legal_mask(*roots[gi], n) != 0
        s.set_roots([r[0] for r in roots], [r[1] for r in roots], [1 if x else 0 for x in live])
        assert not _get_noise(oz, s)[1].any()              # every slot got another board: the noise went with the old ones
        arm(1 + mv)                                        # a new root gets fresh eta before it is searched
        oz.check(s.simulate(net, 25))
        for gi in range(G):
            if live[gi]:
                refs[gi].simulate(*roots[gi], 25)
        check(("move", mv))


# ------------------------------------------------------------------ 3. off means off
def test_off_means_off(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 4
    roots = _golden_roots(n, 8)[:G]
    other = _golden_roots(n, 8)[G:]
    net = StubNetWrapper((n, n), SALT, 0, max_batch=G)
    eta = _ref_eta(n, roots)

    def plain_refs(rs, nsims):
        out = [WideSearch(n, 1.0, 1, salt=SALT) for _ in rs]
        for r, (o, p) in zip(out, rs):
            r.simulate(o, p, nsims)
        return out

    def same(s, refs, where, slots=None):
        for gi in (range(G) if slots is None else slots):
            assert_same_tables(s.dump(gi), refs[gi], (where, gi))

    want = plain_refs(roots, 40)
    # a never-armed object
    a = Search(oz, n, G)
    a.set_roots([r[0] for r in roots], [r[1] for r in roots])
    assert _get_noise(oz, a)[2] == 0.0 and not _get_noise(oz, a)[0].any() and not _get_noise(oz, a)[1].any()
    oz.check(a.simulate(net, 40))
    same(a, want, "never armed")
    # eps = 0 with eta supplied
    b = Search(oz, n, G)
    b.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(_set_noise(oz, b, 0.0, eta))
    assert _get_noise(oz, b)[2] == 0.0 and not _get_noise(oz, b)[1].any()
    oz.check(b.simulate(net, 40))
    same(b, want, "eps 0")
    # armed, then eps = 0: disarmed again
    oz.check(_set_noise(oz, b, EPS, eta))
    oz.check(_set_noise(oz, b, 0.0, eta))
    assert not _get_noise(oz, b)[1].any()
    # disarmed slots next to armed ones
    c = Search(oz, n, G)
    c.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(_set_noise(oz, c, EPS, eta, [1, 0, 1, 0]))
    oz.check(c.simulate(net, 40))
    same(c, want, "disarmed slot", slots=(1, 3))
    noisy = [NoisyWideSearch(n, 1.0, 1, salt=SALT) for _ in range(G)]
    for gi in (0, 2):
        noisy[gi].set_noise(*roots[gi], eta[gi], EPS)
        noisy[gi].simulate(*roots[gi], 40)
    same(c, noisy, "armed slot", slots=(0, 2))
    # other boards: the noise is dropped -- except where the board stays
    d = Search(oz, n, G)
    d.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(_set_noise(oz, d, EPS, eta))
    assert _get_noise(oz, d)[1].all()
    moved = [roots[0]] + list(other[1:])
    d.set_roots([r[0] for r in moved], [r[1] for r in moved])
    assert list(_get_noise(oz, d)[1]) == [1, 0, 0, 0]
    d.set_roots([r[0] for r in other], [r[1] for r in other])
    assert not _get_noise(oz, d)[1].any()
    oz.check(d.simulate(net, 40))
    same(d, plain_refs(other, 40), "another board")


# ------------------------------------------------------------------ 4. the lock-step engine
@pytest.mark.parametrize("K", [1, 4])
def test_lockstep_engine_round_by_round(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G, sims, seed, first, salt = 6, 8, 16, 77, 300, 21
    net = StubNetWrapper((n, n), salt, 0, max_batch=G * K)
    eng = SelfPlayEngine(net, n, G, sims, 1.0, 0.0, 1.0, seed=seed, first_game_id=first, leaves_per_step=K, root_noise=(ALPHA, EPS))
    W = [NoisyWideSearch(n, 1.0, K, salt=salt) for _ in range(G)]
    worst, searched = 0.0, 0
    for rnd in range(n * n):
        st = eng.state()
        if st["finished"].all():
            break
        eng.run(1)
        eta, armed = eng.last_root_noise()
        cnt, after = eng.last_counts(), eng.state()
        for g in range(G):
            if st["finished"][g]:
                assert not armed[g], (rnd, g)
                continue
            b, w, p, ply, gid = int(st["black"][g]), int(st["white"][g]), int(st["player"][g]), int(st["ply"][g]), int(st["game_id"][g])
            own, opp = (b, w) if p == 1 else (w, b)
            assert armed[g] and gid == first + g
            want = dirichlet(n, legal_mask(own, opp, n), ALPHA, seed, gid, ply)[0]
            worst = max(worst, float(np.abs(eta[g] - want).max()))
            assert np.abs(eta[g] - want).max() <= 1e-9, (rnd, g)
            W[g].set_noise(own, opp, eta[g], EPS)          # the device's own eta: the counts must then agree exactly
            W[g].simulate(own, opp, sims)
            assert np.array_equal(cnt[g], W[g].counts(own, opp)[0]), (rnd, g)
            placed = (int(after["black"][g]) | int(after["white"][g])) & ~(b | w)
            assert placed == 1 << W[g].best_move(own, opp, tie_draw(seed, gid, ply)), (rnd, g)
            searched += 1
        if rnd == 0:                                       # one board, eight game ids: eight different draws
            assert len({eta[g].tobytes() for g in range(G)}) == G
    assert eng.stats()["live_games"] == 0 and searched == eng.stats()["moves"]
    print(f"K = {K}: {searched} searched moves, largest |eta_device - eta_restatement| = {worst:.3e}")


# ------------------------------------------------------------------ 5. drivers and determinism
def _engine(net, G, first, noise, n=6, sims=12, seed=41):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, n, G, sims, 1.0, 1.0, 0.85, seed=seed, first_game_id=first, root_noise=noise)


def test_drivers_and_determinism(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, noise = 6, (ALPHA, EPS)
    net = StubNetWrapper((n, n), 5, 0, max_batch=16)
    a = _engine(net, 16, 16, noise).play_to_end()
    b = _engine(net, 16, 16, noise).play_to_end()
    assert a.size > 0 and a.tobytes() == b.tobytes()       # twice the same bytes
    free = _engine(net, 16, 16, noise)
    for _ in range(200):
        free.run_steps(32)
        if free.stats()["live_games"] == 0:
            break
    assert free.stats()["live_games"] == 0
    assert free.records().tobytes() == a.tobytes()         # the free-running driver: the records of run(), game for game
    one = _engine(net, 1, 19, noise).play_to_end()         # another engine size, another slot
    assert one.size > 0 and one.tobytes() == a[a["game_id"] == 19].tobytes()
    quiet = _engine(net, 16, 16, None).play_to_end()
    assert quiet.tobytes() != a.tobytes()
    assert quiet.tobytes() == _engine(net, 16, 16, (ALPHA, 0.0)).play_to_end().tobytes()       # epsilon 0 is no noise


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_objects_usable(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    import oracle
    lib = oz.load()
    n, G = 6, 4
    net = StubNetWrapper((n, n), 3, 0, max_batch=G)
    roots = _golden_roots(n, G)
    eta = _ref_eta(n, roots)
    ids, plies = list(range(G)), [0] * G
    s = Search(oz, n, G)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    for alpha in (0.001, 100.5, float("nan"), float("inf"), -1.0):
        assert _sample(oz, s, alpha, EPS, 1, ids, plies) == oz.OZ_ERR_ARG and "alpha" in lib.oz_last_error().decode()
    for eps in (-0.1, 1.5, float("nan")):
        assert _sample(oz, s, ALPHA, eps, 1, ids, plies) == oz.OZ_ERR_ARG and "eps" in lib.oz_last_error().decode()
        assert _set_noise(oz, s, eps, eta) == oz.OZ_ERR_ARG and "eps" in lib.oz_last_error().decode()
    bad = eta.copy()
    bad[1, 5] = 1.5
    assert _set_noise(oz, s, EPS, bad) == oz.OZ_ERR_ARG
    assert _get_noise(oz, s)[2] == 0.0 and not _get_noise(oz, s)[1].any()          # nothing was armed by a refused call
    # a change while a step is pending
    oz.check(lib.oz_mcts_select(s.h))
    assert _set_noise(oz, s, EPS, eta) == oz.OZ_ERR_STATE and "pending" in lib.oz_last_error().decode()
    assert _sample(oz, s, ALPHA, EPS, 1, ids, plies) == oz.OZ_ERR_STATE and "pending" in lib.oz_last_error().decode()
    status, lo, lp = np.zeros(G, np.int32), np.zeros(G, np.uint64), np.zeros(G, np.uint64)
    pi, v = np.zeros((G, n * n), np.float32), np.zeros(G, np.float32)
    oz.check(lib.oz_mcts_leaves(s.h, oz.p_i32(status), oz.p_u64(lo), oz.p_u64(lp)))
    for gi in range(G):
        p, val = oracle.stub_predict(int(lo[gi]), int(lp[gi]), n, 3, 0)
        pi[gi], v[gi] = p.ravel(), val
    oz.check(lib.oz_mcts_backup(s.h, oz.p_f32(pi), oz.p_f32(v)))
    # ... and the object is usable: armed now, it is the restatement's noisy search (the pending simulation included)
    oz.check(_set_noise(oz, s, EPS, eta))
    oz.check(s.simulate(net, 20))
    for gi in range(G):
        ref = NoisyWideSearch(n, 1.0, 1, salt=3)
        ref.simulate(*roots[gi], 1)
        ref.set_noise(*roots[gi], eta[gi], EPS)
        ref.simulate(*roots[gi], 20)
        assert_same_tables(s.dump(gi), ref, ("after refusals", gi))
    # the engine
    eng = SelfPlayEngine(net, n, G, 8)
    for alpha, eps in ((0.001, EPS), (101.0, EPS), (ALPHA, 1.01), (ALPHA, -1.0)):
        assert lib.oz_selfplay_set_root_noise(eng._h, alpha, eps) == oz.OZ_ERR_ARG
    oz.check(lib.oz_selfplay_set_root_noise(eng._h, ALPHA, EPS))
    eng.run(1)
    assert lib.oz_selfplay_set_root_noise(eng._h, ALPHA, EPS) == oz.OZ_ERR_STATE and "driven" in lib.oz_last_error().decode()
    assert lib.oz_selfplay_set_root_noise(eng._h, ALPHA, 0.0) == oz.OZ_ERR_STATE
    eng.run(1)
    assert eng.last_root_noise()[1].all() and eng.stats()["moves"] == 2 * G


# ------------------------------------------------------------------ 7. the drop-ins
def test_host_evaluator_split_honours_the_noise(oz):
    """OthelloMCTS with a duck-typed network: oz_mcts_select / leaves / backup run the same descent"""
    import oracle
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    n, salt = 6, 13
    own, opp = _golden_roots(n, 8)[2]

    class HostNet:
        network_type = None

        def predict(self, board):
            o, p = oz.pack_board(board)
            return oracle.stub_predict(o, p, n, salt, 0)
    m = OthelloMCTS(n, HostNet(), 1.0, node_cap=256)
    state = oz.unpack_board(own, opp, n)
    eta = dirichlet(n, legal_mask(own, opp, n), ALPHA, ETA_SEED, 0, 0)[0]
    m.set_root_noise(eta, EPS, state=state, player=OthelloPlayer.BLACK)
    got, armed, eps = m.root_noise()
    assert np.array_equal(got, eta) and armed and eps == EPS
    m.simulate_n(state, OthelloPlayer.BLACK, 30)
    ref = NoisyWideSearch(n, 1.0, 1, salt=salt)
    ref.set_noise(own, opp, eta, EPS)
    ref.simulate(own, opp, 30)
    assert_same_tables(m.dump(), ref, "host evaluator")


def test_execute_episode_dropin_with_root_noise(oz):
    from othellozero_amd import training
    from othellozero_amd.NNet import StubNetWrapper
    n = 6
    net = StubNetWrapper((n, n), 17, 0, max_batch=1)
    random.seed(1)
    np.random.seed(1)
    ex = training.execute_episode(n, net, 1, 8, 1, 1.0, root_noise=(ALPHA, EPS), snapshot_boards=True)
    assert len(ex) > 0 and len(ex) % 8 == 0 and all(p.sum() == 1 and z in (-1, 1) for _, p, z in ex)
    quiet = training.execute_episode(n, net, 1, 8, 1, 1.0, snapshot_boards=True)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(ex, quiet)) or len(ex) != len(quiet)        # e_greedy = 1: only the noise can differ
    vis = training.execute_episode(n, net, 1, 8, 1, 1.0, root_noise=(ALPHA, EPS), snapshot_boards=True, policy_target="visits")
    assert len(vis) == len(ex) and all(abs(float(p.sum()) - 1.0) <= 1e-12 for _, p, _ in vis)
    again = training.execute_episode(n, net, 1, 8, 1, 1.0, root_noise=(ALPHA, EPS), snapshot_boards=True, noise_seed=1)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(ex, again)) or len(ex) != len(again)           # another noise seed, another game


def test_training_loop_with_root_noise(oz, tmp_path, monkeypatch):
    """one tiny iteration: the argument reaches the self-play engine and nothing else"""
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    random.seed(4)
    np.random.seed(4)
    n, seen = 6, []
    inner = loop.selfplay_batch

    def spy(*args, **kw):
        seen.append(kw.get("root_noise"))
        return inner(*args, **kw)
    monkeypatch.setattr(loop, "selfplay_batch", spy)
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    historic = loop.training(board_size=n, num_iterations=1, num_episodes=6, num_simulations=6, degree_exploration=1, temperature=1,
                             neural_network=net, e_greedy=0.9, evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0,
                             self_play_training=False, self_play_interval=1, self_play_total_games=2, self_play_threshold=1,
                             checkpoint_filepath=str(tmp_path / "noise.h5"), training_buffer_size=8 * 40, seed=12, batched_evaluation=True,
                             root_noise=(ALPHA, EPS))
    assert len(historic) == 1 and seen == [(ALPHA, EPS)]
    assert all(np.isfinite(a).all() for a in net.get_weights())
