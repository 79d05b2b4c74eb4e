"""The playout cap on the GPU (pytest -m gpu): the engine against the restatement in tests/playout_cap_ref.py byte for byte, the drivers, leaf-parallel
search, off-means-off, the record consumers, the training loop and the refusals.  6x6, 16 games, 12 simulations throughout."""
import math
import random

import numpy as np
import pytest

import playout_cap_ref as ref
import replay_ref

pytestmark = pytest.mark.gpu

N, G, SIMS, SEED, FIRST, EG, SALT = 6, 16, 12, 41, 200, 0.8, 21
CAP = (4, 0.25)
FULL, FAST = 123, 389                                      # the restatement's records at these settings (tests/test_playout_cap_cpu.py holds it to them)


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def want():
    """the restatement's games, computed once: (records, count rows, sum of budgets)"""
    return ref.episodes(N, SIMS, CAP, EG, SEED, FIRST, G, SALT)


def _net(K=1, salt=SALT):
    from othellozero_amd.NNet import StubNetWrapper
    return StubNetWrapper((N, N), salt, 0, max_batch=G * K)


def _engine(net, cap, games=G, first=FIRST, seed=SEED, **kw):
    from othellozero_amd.training import SelfPlayEngine
    extra = {} if cap == "absent" else {"playout_cap": cap}
    return SelfPlayEngine(net, N, games, SIMS, 1.0, 1.0, EG, seed=seed, first_game_id=first, **extra, **kw)


def _free_run(eng):
    for _ in range(200):
        eng.run_steps(32)
        if eng.stats()["live_games"] == 0:
            break
    assert eng.stats()["live_games"] == 0
    return eng.records()


def _draws(rec, full_prob=CAP[1], seed=SEED):
    """the restatement's flag for every record's (game id, ply)"""
    return np.array([0 if ref.is_full(seed, int(g), int(p), full_prob) else 1 for g, p in zip(rec["game_id"], rec["ply"])], np.uint8)


# ------------------------------------------------------------------ 1. the engine against the restatement
def test_engine_against_the_restatement(oz, want):
    wrec, wrows, wspent = want
    eng = _engine(_net(), CAP, record_visits=True)
    rec, rows = eng.play_to_end(with_visits=True)
    fast = oz.record_fast(rec)
    print(f"records {rec.size}: full {int((fast == 0).sum())}, fast {int((fast == 1).sum())}; simulations {eng.stats()['simulations']} (want {wspent})")
    assert rec.dtype == wrec.dtype and rec.size == wrec.size
    for field in ("black", "white", "final_black", "final_white", "game_id", "ply", "action", "player", "z", "greedy", "pad"):
        assert np.array_equal(rec[field], wrec[field]), field
    assert rec.tobytes() == wrec.tobytes()
    assert rows.dtype == wrows.dtype and rows.tobytes() == wrows.tobytes()
    assert eng.stats()["simulations"] == wspent == FULL * SIMS + FAST * CAP[0]
    assert eng.stats()["games_completed"] == G and eng.stats()["moves"] == rec.size
    ps = eng.playout_stats()
    assert (ps["fast_sims"], ps["full_prob"], ps["full_moves"], ps["fast_moves"]) == (CAP[0], CAP[1], FULL, FAST)
    assert int((fast == 0).sum()) == FULL >= 64 and int((fast == 1).sum()) == FAST >= 64 and not rec["pad"][:, 1:].any()


# ------------------------------------------------------------------ 2. the drivers
def test_drivers(oz, want):
    net = _net()
    a = _engine(net, CAP).play_to_end()
    assert a.tobytes() == want[0].tobytes()
    assert _free_run(_engine(net, CAP)).tobytes() == a.tobytes()                         # run_steps: the bytes of run()
    assert _engine(net, CAP).play_to_end().tobytes() == a.tobytes()                      # twice the same
    one = _engine(net, CAP, games=1, first=203).play_to_end()                            # another engine size, another slot
    assert one.size > 0 and one.tobytes() == a[a["game_id"] == 203].tobytes()
    assert _engine(net, CAP, seed=SEED + 1).play_to_end().tobytes() != a.tobytes()


def test_drivers_with_root_noise(oz):
    net = _net()
    noise = (0.5, 0.25)
    a = _engine(net, CAP, root_noise=noise).play_to_end()
    fast = oz.record_fast(a)
    assert np.array_equal(fast, _draws(a)) and 0 < int(fast.sum()) < a.size
    assert _free_run(_engine(net, CAP, root_noise=noise)).tobytes() == a.tobytes()
    assert a.tobytes() != _engine(net, CAP).play_to_end().tobytes()                      # the full moves did see noise
    # after one round the slots of the games whose ply-0 move is full are armed, the others are not
    eng = _engine(net, CAP, root_noise=noise)
    eng.run(1)
    eta, armed = eng.last_root_noise()
    full0 = np.array([ref.is_full(SEED, FIRST + g, 0, CAP[1]) for g in range(G)])
    assert 0 < int(full0.sum()) < G and np.array_equal(armed.astype(bool), full0)
    assert np.allclose(eta[full0].sum(axis=1), 1.0) and not eta[~full0].any()
    eng.play_to_end()
    assert eng.stats()["games_completed"] == G


# ------------------------------------------------------------------ 3. leaf-parallel search
def test_leaf_parallel_search(oz):
    K = 4
    net = _net(K)
    eng = _engine(net, CAP, leaves_per_step=K)
    rec = eng.play_to_end()
    fast = oz.record_fast(rec)
    assert eng.stats()["games_completed"] == G and rec.size == eng.stats()["moves"]
    assert np.array_equal(fast, _draws(rec)) and int((fast == 0).sum()) >= G and int((fast == 1).sum()) >= G
    budgets = np.where(fast == 1, CAP[0], SIMS)
    assert np.array_equal(budgets, oz.playout_budgets(SEED, rec["game_id"], rec["ply"], SIMS, CAP))
    assert eng.stats()["simulations"] == int(budgets.sum())
    ps = eng.playout_stats()
    assert (ps["full_moves"], ps["fast_moves"]) == (int((fast == 0).sum()), int((fast == 1).sum()))
    plain = _engine(net, "absent", leaves_per_step=K).play_to_end()
    assert plain.size > 0 and not oz.record_fast(plain).any()
    assert _engine(net, (4, 1.0), leaves_per_step=K).play_to_end().tobytes() == plain.tobytes()
    assert rec.tobytes() != plain.tobytes()


# ------------------------------------------------------------------ 4. off means off
def test_off_means_off(oz):
    from othellozero_amd.agents import arena_batch
    net = _net()
    today = _engine(net, "absent").play_to_end()
    assert today.size > 0 and not today["pad"].any()
    for cap in (None, (4, 1.0), (SIMS, 1.0)):
        assert _engine(net, cap).play_to_end().tobytes() == today.tobytes(), cap
        assert _free_run(_engine(net, cap)).tobytes() == today.tobytes(), cap
    every = _engine(net, (4, 1.0))
    every.play_to_end()
    assert (every.playout_stats()["full_moves"], every.playout_stats()["fast_moves"]) == (today.size, 0)
    assert every.stats()["simulations"] == today.size * SIMS
    assert _engine(net, CAP).play_to_end().tobytes() != today.tobytes()
    # the arena is never capped: a capped engine alive (and driven) on the same network changes nothing
    other = _net(salt=SALT + 1)
    before = arena_batch(net, other, N, 8, 10, 1.0, seed=3)
    capped = _engine(net, CAP)
    capped.run(2)
    after = arena_batch(net, other, N, 8, 10, 1.0, seed=3)
    for key in ("winner", "points", "n_moves", "actions", "players"):
        assert np.array_equal(before[key], after[key]), key
    capped.run(1)


def test_stagger_is_not_capped(oz):
    """stagger() plays slot g's first (g * 32) // 16 plies at sims_pre with flag 0, capped engine or not; the plies after it follow the draw"""
    net = _net()
    eng = _engine(net, CAP, refill=True)
    eng.stagger()
    offsets = (np.arange(G) * (N * N - 4)) // G
    staggered = int(offsets.sum())                         # slot g searched and moved in offsets[g] rounds
    assert eng.stats()["moves"] == staggered and eng.stats()["simulations"] == staggered * SIMS
    assert eng.playout_stats()["full_moves"] == eng.playout_stats()["fast_moves"] == 0
    for _ in range(12):
        eng.run(4)
        if eng.stats()["games_completed"] >= G:
            break
    rec = eng.records()
    first = rec[rec["game_id"] < FIRST + G]                 # the first game of every slot
    assert first.size > 0 and len(set(first["game_id"].tolist())) >= G // 2
    opening = first["ply"] < offsets[(first["game_id"] - FIRST).astype(np.int64)]
    fast = oz.record_fast(first)
    assert opening.sum() > 2 * G and not fast[opening].any()
    assert np.array_equal(fast[~opening], _draws(first[~opening])) and fast[~opening].sum() > G
    ps = eng.playout_stats()
    assert ps["full_moves"] + ps["fast_moves"] == eng.stats()["moves"] - staggered


# ------------------------------------------------------------------ 5. the consumers
def test_selfplay_batch_expands_the_full_records_only(oz, want):
    from othellozero_amd.training import selfplay_batch
    net = _net()
    args = (net, N, G, SIMS, 1.0, 1.0, EG, SEED, FIRST)
    boards, pol, z = selfplay_batch(*args, expand=True, playout_cap=CAP)
    assert boards.shape[0] == pol.shape[0] == z.shape[0] == 8 * FULL
    assert selfplay_batch.playout_stats["full_moves"] == FULL and selfplay_batch.playout_stats["fast_moves"] == FAST
    boards_v, pi, z_v = selfplay_batch(*args, expand=True, record_visits=True, playout_cap=CAP)
    assert boards_v.shape[0] == pi.shape[0] == z_v.shape[0] == 8 * FULL and pi.shape[1:] == (N, N)
    assert np.array_equal(boards_v, boards) and np.array_equal(z_v, z) and np.allclose(pi.sum(axis=(1, 2)), 1.0)
    rec = selfplay_batch(*args, playout_cap=CAP)            # not expanded: all records, the fast ones flagged
    assert rec.tobytes() == want[0].tobytes()
    plain = selfplay_batch(*args, expand=True)
    assert plain[0].shape[0] > 8 * (FULL + FAST) // 2 and selfplay_batch.playout_stats is None


@pytest.mark.parametrize("capacity", [8 * (FULL + FAST), 8 * 50 + 3], ids=["roomy", "wraps"])
def test_replay_buffer_appends_the_full_records_only(oz, want, capacity):
    from othellozero_amd.replay import ReplayBuffer
    wrec, wrows, _ = want
    keep = wrec["pad"][:, 0] == 0
    eng = _engine(_net(), CAP, record_visits=True)
    rec, rows = eng.play_to_end(with_visits=True)
    assert rec.tobytes() == wrec.tobytes()
    for target, T in (("onehot", 1.0), ("visits", 0.7)):
        model = replay_ref.Ring(capacity, N)
        model.append(*replay_ref.examples(wrec[keep], N, False, wrows[keep] if target == "visits" else None, T))
        buf = ReplayBuffer(N, capacity)
        assert buf.append_engine(eng, policy_target=target, target_temperature=T) == FULL
        assert buf.info() == (min(8 * FULL, capacity), capacity, 8 * FULL) and model.total == 8 * FULL
        assert replay_ref.same(buf.read(), model.read()), (target, capacity)
        host = ReplayBuffer(N, capacity)                    # the same records handed in from the host, shuffled
        p = np.random.RandomState(5).permutation(rec.size)
        assert host.append_records(rec[p], rows[p] if target == "visits" else None, policy_target=target, target_temperature=T) == FULL
        assert host.info() == buf.info() and replay_ref.same(host.read(), model.read()), (target, capacity)
    none = ReplayBuffer(N, 64)
    assert none.append_records(rec[~keep][:20]) == 0 and none.info() == (0, 64, 0)
    assert none.append_engine(eng, first_record=rec.size) == 0 and len(none) == 0


# ------------------------------------------------------------------ 6. the training loop
@pytest.mark.parametrize("replay", ["host", "device"])
def test_training_loop_with_a_playout_cap(oz, tmp_path, monkeypatch, replay):
    """one tiny iteration: the option reaches the self-play engine, and the fit sees 8 examples per fully searched move"""
    from othellozero_amd import loop, training
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    random.seed(4)
    np.random.seed(4)
    engines, fits = [], []
    init, fit = training.SelfPlayEngine.__init__, NNetWrapper.train

    def spy_init(self, *args, **kw):
        engines.append((self, kw.get("playout_cap")))
        return init(self, *args, **kw)

    def spy_fit(self, examples, *args, **kw):
        fits.append(len(examples))
        return fit(self, examples, *args, **kw)
    monkeypatch.setattr(training.SelfPlayEngine, "__init__", spy_init)
    monkeypatch.setattr(NNetWrapper, "train", spy_fit)
    net = NNetWrapper((N, N), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    historic = loop.training(board_size=N, num_iterations=1, num_episodes=6, num_simulations=6, degree_exploration=1, temperature=1,
                             neural_network=net, e_greedy=0.9, evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0,
                             self_play_training=False, self_play_interval=1, self_play_total_games=2, self_play_threshold=1,
                             checkpoint_filepath=str(tmp_path / "cap.h5"), training_buffer_size=8 * 6 * 32, seed=12, batched_evaluation=True,
                             alias_final_boards=False, replay=replay, playout_cap=CAP)
    assert len(historic) == 1 and math.isfinite(historic[0][1])
    assert len(engines) == 1 and engines[0][1] == CAP and len(fits) == 1
    eng = engines[0][0]
    ps, st = eng.playout_stats(), eng.stats()
    assert st["games_completed"] == 6 and ps["full_moves"] + ps["fast_moves"] == st["moves"] and ps["full_moves"] >= 6 and ps["fast_moves"] >= 6
    assert fits[0] == 8 * ps["full_moves"]
    assert all(np.isfinite(a).all() for a in net.get_weights())


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_engine_usable(oz):
    lib = oz.load()
    net = _net()
    eng = _engine(net, "absent")
    for fast_sims, full_prob, word in ((1, 0.25, "fast_sims"), (SIMS + 1, 0.25, "fast_sims"), (-2, 0.25, "fast_sims"), (4, 0.0, "full_prob"),
                                       (4, 1.5, "full_prob"), (4, float("nan"), "full_prob")):
        assert lib.oz_selfplay_set_playout_cap(eng._h, fast_sims, full_prob) == oz.OZ_ERR_ARG, (fast_sims, full_prob)
        assert word in lib.oz_last_error().decode()
    assert eng.playout_stats()["fast_sims"] == 0
    oz.check(lib.oz_selfplay_set_playout_cap(eng._h, 4, 0.25))
    oz.check(lib.oz_selfplay_set_playout_cap(eng._h, 0, 0.0))               # disarmed again ...
    assert eng.playout_stats()["fast_sims"] == 0
    oz.check(lib.oz_selfplay_set_playout_cap(eng._h, *CAP))                 # ... and armed
    eng.run(1)
    assert lib.oz_selfplay_set_playout_cap(eng._h, 4, 0.5) == oz.OZ_ERR_STATE and "driven" in lib.oz_last_error().decode()
    assert lib.oz_selfplay_set_playout_cap(eng._h, 0, 0.0) == oz.OZ_ERR_STATE
    rec = eng.play_to_end()
    assert eng.stats()["games_completed"] == G and rec.tobytes() == _engine(net, CAP).play_to_end().tobytes()
    # a refusal after the first driver call of an engine without the option: it plays on as it was
    plain = _engine(net, "absent")
    plain.run(1)
    assert lib.oz_selfplay_set_playout_cap(plain._h, *CAP) == oz.OZ_ERR_STATE
    assert plain.play_to_end().tobytes() == _engine(net, None).play_to_end().tobytes() and not plain.playout_stats()["fast_moves"]
    with pytest.raises(ValueError):
        _engine(net, (1, 0.25))
    with pytest.raises(ValueError):
        _engine(net, (SIMS + 1, 0.25))
