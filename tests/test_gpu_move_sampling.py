"""Move sampling on the GPU (pytest -m gpu): the device's sampler against the restatement in tests/move_sampling_ref.py fed with the device's
own visit counts, the engines from their own records, the drivers, off-means-off, the refusals and the drop-ins.  Device and host pow differ
by ulps, so a draw whose restated margin is below 1e-9 is left out of a comparison (expected share about 1e-7); more than 1 in 1000 left out
fails the test."""
import math
import random

import numpy as np
import pytest

from move_sampling_ref import sample, selfplay_move
from test_gpu_wide_search import Search, _golden_roots
from wide_search_ref import legal_mask, popcount

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
SAMPLE = (1.0, 6)


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _sample_moves(oz, s, T, seed, ids, plies):
    action, rc = np.full(s.G, -7, np.int32), np.full(s.G, -7, np.int32)
    code = s.lib.oz_mcts_sample_moves(s.h, float(T), int(seed), oz.p_u64(np.array(ids, np.uint64)), oz.p_i32(np.array(plies, np.int32)),
                                      oz.p_i32(action), oz.p_i32(rc))
    return code, action, rc


def _root_counts(oz, s):
    cnt, legal, rc = np.zeros((s.G, 64), np.int32), np.zeros(s.G, np.uint64), np.zeros(s.G, np.int32)
    oz.check(s.lib.oz_mcts_root_counts(s.h, oz.p_i32(cnt), oz.p_u64(legal), oz.p_i32(rc)))
    return cnt, legal, rc


class Tally:
    """the margin rule: compared and left-out draws"""

    def __init__(self):
        self.compared, self.left_out = 0, 0

    def check(self, got, want, margin, where):
        if margin < MARGIN:
            self.left_out += 1
            return
        self.compared += 1
        assert got == want, (where, got, want, margin)

    def close(self, at_least):
        assert self.compared >= at_least, (self.compared, at_least)
        assert self.left_out * 1000 <= self.compared + self.left_out, (self.left_out, self.compared)


# ------------------------------------------------------------------ 1. the sampler
@pytest.mark.parametrize("n", [6, 8])
def test_device_sampler_vs_restatement(oz, n):
    from othellozero_amd.NNet import StubNetWrapper
    G, seeds = 64, (41, 1234)
    roots = _golden_roots(n, G)
    ids = [1000 + gi for gi in range(G)]
    plies = [popcount(o | p) - 4 for o, p in roots]
    net = StubNetWrapper((n, n), 13, 0, max_batch=G)
    s = Search(oz, n, G, node_cap=256)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    # unknown roots, and roots expanded but never selected from: rc as oz_mcts_root_counts, no move
    for nsims, want_rc in ((0, 1), (1, 2)):
        if nsims:
            oz.check(s.simulate(net, nsims))
        code, action, rc = _sample_moves(oz, s, 1.0, 1, ids, plies)
        assert code == 0 and (rc == want_rc).all() and np.array_equal(rc, _root_counts(oz, s)[2]) and (action == -1).all()
    oz.check(s.simulate(net, 23))                          # 24 simulations in all
    cnt, legal, rc0 = _root_counts(oz, s)
    assert (rc0 == 0).all() and (cnt.sum(axis=1) == 23).all()
    assert all(int(legal[gi]) == legal_mask(*roots[gi], n) for gi in range(G))
    tally, picked = Tally(), set()
    for seed in seeds:
        for T in (0.25, 1.0, 3.0):
            code, action, rc = _sample_moves(oz, s, T, seed, ids, plies)
            assert code == 0 and (rc == 0).all()
            for gi in range(G):
                want, margin = sample(cnt[gi], int(legal[gi]), T, seed, ids[gi], plies[gi])
                assert cnt[gi][action[gi]] > 0 and (int(legal[gi]) >> int(action[gi])) & 1, (n, seed, T, gi)
                tally.check(int(action[gi]), want, margin, (n, seed, T, gi))
                picked.add((gi, int(action[gi])))
    tally.close(6 * G - 1)
    assert len(picked) > G                                 # not vacuous: some root got different moves from different draws
    assert np.array_equal(_root_counts(oz, s)[0], cnt)     # sampling is a read: the tables are as they were
    # an idle slot gets no move
    active = [gi % 2 for gi in range(G)]
    s.set_roots([r[0] for r in roots], [r[1] for r in roots], active)
    code, action, rc = _sample_moves(oz, s, 1.0, 41, ids, plies)
    assert code == 0 and all((action[gi] >= 0) == bool(active[gi]) for gi in range(G)) and (rc == 0).all()


# ------------------------------------------------------------------ 2. the engine, from its own records
def _check_records(rec, counts, n, e_greedy, seed, sample_moves, tally):
    kinds = {0: 0, 1: 0, 2: 0}
    for r, row in zip(rec, counts):
        b, w, p, ply, gid = int(r["black"]), int(r["white"]), int(r["player"]), int(r["ply"]), int(r["game_id"])
        own, opp = (b, w) if p == 1 else (w, b)
        legal = legal_mask(own, opp, n)
        assert all(row[sq] == 0 for sq in range(64) if not (legal >> sq) & 1)
        want, greedy, margin = selfplay_move(row, legal, e_greedy, seed, gid, ply, sample_moves)
        assert int(r["greedy"]) == greedy, (gid, ply, int(r["greedy"]), greedy)
        assert (greedy == 2) == (sample_moves is not None and ply < sample_moves[1] and greedy != 0)
        kinds[greedy] += 1
        if greedy == 2:
            assert row[int(r["action"])] > 0
            tally.check(int(r["action"]), want, margin, (gid, ply))
        else:
            assert int(r["action"]) == want, (gid, ply, greedy)
    return kinds


@pytest.mark.parametrize("K", [1, 4])
def test_engine_from_its_own_records(oz, K):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G, sims, seed, first, eg = 6, 16, 12, 41, 200, 0.8
    net = StubNetWrapper((n, n), 21, 0, max_batch=G * K)
    eng = SelfPlayEngine(net, n, G, sims, 1.0, 1.0, eg, seed=seed, first_game_id=first, record_visits=True, leaves_per_step=K,
                         sample_moves=SAMPLE)
    rec, counts = eng.play_to_end(with_visits=True)
    assert eng.stats()["games_completed"] == G and rec.size == eng.stats()["moves"]
    tally = Tally()
    kinds = _check_records(rec, counts, n, eg, seed, SAMPLE, tally)
    tally.close(kinds[2] - 1)
    assert kinds[2] >= 3 * G and kinds[1] >= G and kinds[0] >= G // 2, kinds           # all three branches were played
    # not vacuous: somewhere the sampled move is not the arg-max
    sampled = rec["greedy"] == 2
    assert (rec["action"][sampled] != np.argmax(counts[sampled], axis=1)).any()
    assert (rec[sampled]["ply"] < SAMPLE[1]).all() and not (rec[~sampled]["greedy"] == 2).any()


# ------------------------------------------------------------------ 3. the drivers
def _engine(net, G, first, sample_moves, n=6, sims=12, seed=41, noise=None, eg=0.85, **kw):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, n, G, sims, 1.0, 1.0, eg, seed=seed, first_game_id=first, root_noise=noise, sample_moves=sample_moves, **kw)


def _free_run(eng):
    for _ in range(200):
        eng.run_steps(32)
        if eng.stats()["live_games"] == 0:
            break
    assert eng.stats()["live_games"] == 0
    return eng.records()


@pytest.mark.parametrize("noise", [None, (0.5, 0.25)])
def test_free_running_driver_and_determinism(oz, noise):
    from othellozero_amd.NNet import StubNetWrapper
    net = StubNetWrapper((6, 6), 5, 0, max_batch=16)
    a = _engine(net, 16, 16, SAMPLE, noise=noise).play_to_end()
    assert a.size > 0 and (a["greedy"] == 2).sum() >= 3 * 16
    assert _engine(net, 16, 16, SAMPLE, noise=noise).play_to_end().tobytes() == a.tobytes()         # twice the same bytes
    assert _free_run(_engine(net, 16, 16, SAMPLE, noise=noise)).tobytes() == a.tobytes()            # run_steps: the records of run()
    one = _engine(net, 1, 19, SAMPLE, noise=noise).play_to_end()                                    # another engine size, another slot
    assert one.size > 0 and one.tobytes() == a[a["game_id"] == 19].tobytes()
    other = _engine(net, 16, 16, SAMPLE, noise=noise, seed=42).play_to_end()
    assert other.tobytes() != a.tobytes()
    assert _engine(net, 16, 16, (3.0, 6), noise=noise).play_to_end().tobytes() != a.tobytes()       # another temperature, other games


def test_stagger_samples_too(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G, seed = 6, 16, 9
    net = StubNetWrapper((n, n), 5, 0, max_batch=G)
    eng = _engine(net, G, 0, SAMPLE, seed=seed, eg=1.0, refill=True, record_visits=True)
    eng.stagger()
    assert (eng.state()["ply"][1:] > 0).any()
    eng.run(6)
    rec, counts = eng.records(with_visits=True)
    assert rec.size > 0
    staggered = rec[rec["game_id"] < G]                    # first games of their slots: their opening plies were played by stagger()
    assert staggered.size > 0 and (staggered["greedy"][staggered["ply"] < SAMPLE[1]] == 2).all()
    tally = Tally()
    kinds = _check_records(rec, counts, n, 1.0, seed, SAMPLE, tally)
    tally.close(kinds[2] - 1)
    assert kinds[0] == 0 and kinds[2] > 0 and kinds[1] > 0


# ------------------------------------------------------------------ 4. off means off
def test_off_means_off(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.agents import arena_batch
    n, G = 6, 16
    net = StubNetWrapper((n, n), 5, 0, max_batch=G)
    never = _engine(net, G, 16, None).play_to_end()
    zero = _engine(net, G, 16, (1.0, 0)).play_to_end()
    assert never.size > 0 and never.tobytes() == zero.tobytes() and not (never["greedy"] == 2).any()
    assert _free_run(_engine(net, G, 16, (1.0, 0))).tobytes() == never.tobytes()
    assert _engine(net, G, 16, SAMPLE).play_to_end().tobytes() != never.tobytes()
    # the arena never samples: a sampling engine alive (and driven) on the same network changes nothing
    other = StubNetWrapper((n, n), 6, 0, max_batch=G)
    before = arena_batch(net, other, n, 8, 10, 1.0, seed=3)
    armed = _engine(net, G, 16, SAMPLE)
    armed.run(2)
    after = arena_batch(net, other, n, 8, 10, 1.0, seed=3)
    for key in ("winner", "points", "n_moves", "actions", "players"):
        assert np.array_equal(before[key], after[key]), key
    armed.run(1)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_objects_usable(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    n, G = 6, 4
    net = StubNetWrapper((n, n), 3, 0, max_batch=G)
    roots = _golden_roots(n, G)
    ids, plies = list(range(G)), [0] * G
    s = Search(oz, n, G)
    s.set_roots([r[0] for r in roots], [r[1] for r in roots])
    oz.check(s.simulate(net, 10))
    for T in (0.001, 100.5, 0.0, -1.0, float("nan"), float("inf")):
        code, action, rc = _sample_moves(oz, s, T, 1, ids, plies)
        assert code == oz.OZ_ERR_ARG and "temperature" in lib.oz_last_error().decode() and (action == -7).all()
    assert _sample_moves(oz, s, 1.0, 1, ids, [0, -1, 0, 0])[0] == oz.OZ_ERR_ARG
    code, action, rc = _sample_moves(oz, s, 1.0, 1, ids, plies)
    assert code == 0 and (rc == 0).all() and (action >= 0).all()
    # the engine
    eng = SelfPlayEngine(net, n, G, 8, 1.0, 1.0, 1.0, seed=5)
    for T, plies_ in ((0.001, 6), (101.0, 6), (float("nan"), 6), (1.0, -1), (1.0, 65)):
        assert lib.oz_selfplay_set_move_sampling(eng._h, T, plies_) == oz.OZ_ERR_ARG
    oz.check(lib.oz_selfplay_set_move_sampling(eng._h, 1.0, 6))
    oz.check(lib.oz_selfplay_set_move_sampling(eng._h, 1.0, 0))           # disarmed again ...
    oz.check(lib.oz_selfplay_set_move_sampling(eng._h, 1.0, 64))          # ... and armed for every ply
    eng.run(1)
    assert lib.oz_selfplay_set_move_sampling(eng._h, 1.0, 6) == oz.OZ_ERR_STATE and "driven" in lib.oz_last_error().decode()
    assert lib.oz_selfplay_set_move_sampling(eng._h, 1.0, 0) == oz.OZ_ERR_STATE
    rec = eng.play_to_end()
    assert eng.stats()["games_completed"] == G and (rec["greedy"] == 2).all()          # e_greedy 1, plies 64: every move was sampled
    want = SelfPlayEngine(net, n, G, 8, 1.0, 1.0, 1.0, seed=5, sample_moves=(1.0, 64)).play_to_end()
    assert rec.tobytes() == want.tobytes()


# ------------------------------------------------------------------ 6. the drop-ins
def test_execute_episode_plays_the_engines_game(oz):
    from othellozero_amd import training
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, sims, seed = 6, 12, 77
    net = StubNetWrapper((n, n), 17, 0, max_batch=1)
    random.seed(1)
    np.random.seed(1)
    ex = training.execute_episode(n, net, 1.0, sims, 1.0, 1.0, sample_moves=SAMPLE, sample_seed=seed, snapshot_boards=True)
    rec = SelfPlayEngine(net, n, 1, sims, 1.0, 1.0, 1.0, seed=seed, first_game_id=0, sample_moves=SAMPLE).play_to_end()
    assert len(ex) == 8 * rec.size and rec.size > SAMPLE[1]
    for i, r in enumerate(rec):
        board, policy, _ = ex[8 * i + 7]                   # the eighth symmetry is the identity
        assert oz.pack_board(board) == (int(r["black"]), int(r["white"])), i
        row, col = divmod(int(np.argmax(policy)), n)
        assert policy.sum() == 1.0 and row * 8 + col == int(r["action"]), i
        assert int(r["greedy"]) == (2 if i < SAMPLE[1] else 1)
    quiet = training.execute_episode(n, net, 1.0, sims, 1.0, 1.0, snapshot_boards=True)
    again = training.execute_episode(n, net, 1.0, sims, 1.0, 1.0, sample_moves=SAMPLE, sample_seed=seed + 1, snapshot_boards=True)
    differs = [len(x) != len(ex) or any(not np.array_equal(a[1], b[1]) for a, b in zip(x, ex)) for x in (quiet, again)]
    assert any(differs), differs                           # the arg-max game or another seed's game: not both the same as this one


def test_sample_action_of_the_bare_search(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    n = 6
    own, opp = _golden_roots(n, 8)[2]
    net = StubNetWrapper((n, n), 13, 0, max_batch=1)
    m = OthelloMCTS(n, net, 1.0, node_cap=256)
    state = oz.unpack_board(own, opp, n)
    with pytest.raises(KeyError):
        m.sample_action(state, 1.0, 5, 0, 0)               # unknown to the search
    m.simulate_n(state, OthelloPlayer.BLACK, 24)
    rc, cnt, legal = m._counts(state)
    assert rc == 0
    tally = Tally()
    for g in range(40):
        row, col = m.sample_action(state, 0.5, 5, g, 3)
        want, margin = sample(cnt, legal, 0.5, 5, g, 3)
        tally.check(row * 8 + col, want, margin, g)
    tally.close(39)
    with pytest.raises(ValueError):
        m.sample_action(state, 0.0, 5, 0, 0)


def test_training_loop_with_move_sampling(oz, tmp_path, monkeypatch):
    """one tiny iteration: the argument reaches the self-play engine and nothing else"""
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    random.seed(4)
    np.random.seed(4)
    n, seen = 6, []
    inner = loop.selfplay_batch

    def spy(*args, **kw):
        seen.append(kw.get("sample_moves"))
        out = inner(*args, **kw)
        seen.append(int((out["greedy"] == 2).sum()))
        return out
    monkeypatch.setattr(loop, "selfplay_batch", spy)
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    historic = loop.training(board_size=n, num_iterations=1, num_episodes=6, num_simulations=6, degree_exploration=1, temperature=1,
                             neural_network=net, e_greedy=0.9, evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0,
                             self_play_training=False, self_play_interval=1, self_play_total_games=2, self_play_threshold=1,
                             checkpoint_filepath=str(tmp_path / "sample.h5"), training_buffer_size=8 * 40, seed=12, batched_evaluation=True,
                             sample_moves=SAMPLE)
    assert len(historic) == 1 and seen[0] == SAMPLE and seen[1] >= 6 and len(seen) == 2
    assert all(np.isfinite(a).all() for a in net.get_weights())
    assert math.isfinite(historic[0][1])
