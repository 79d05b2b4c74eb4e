"""The device-resident replay buffer (pytest -m gpu, real MI355X): slots against the reference's own examples, the NumPy model
(tests/replay_ref.py) and the existing host path pack_examples(examples_from_records(...)), bit for bit; independence of the order the
records arrive in; the ring; the trainer reading the buffer in place; loop.training(replay="device"); the refusals."""
import ctypes as C
import random

import numpy as np
import pytest

import replay_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

TARGETS = [("onehot", None), ("visits", 1.0), ("visits", 0.5), ("visits", 0.7)]          # 1 / 0.7 is no integer: the device's pow


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _stub_engine(n, salt, keep, G, sims, c, T, eg, seed, first, qmode, **kw):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(StubNetWrapper((n, n), salt, keep, max_batch=G), n, G, sims, c, T, eg, seed=seed, first_game_id=first,
                          q_mode=qmode, **kw)


_GAMES = {}


def _games(n):
    """16 finished games of n x n at 8 simulations, played once per board size: (engine, sorted records, their visit counts)"""
    if n not in _GAMES:
        eng = _stub_engine(n, 9, 0, 16, 8, 1.25, 1.0, 0.8, 777, 1000, 1, record_visits=True)
        rec, cnt = eng.play_to_end(with_visits=True)
        assert eng.stats()["games_completed"] == 16
        _GAMES[n] = (eng, rec, cnt)
    return _GAMES[n]


def _host_path(rec, cnt, n, alias_final, target, T):
    from othellozero_amd.loop import examples_from_records
    from othellozero_amd.trainer import pack_examples
    ex = examples_from_records(rec, n, alias_final=alias_final, visits=cnt if target == "visits" else None, target_temperature=T or 1.0)
    return pack_examples(ex, n)


def _kw(alias_final, target, T):
    return dict(alias_final=bool(alias_final), policy_target=target, target_temperature=T or 1.0)


# ------------------------------------------------------------------ contents
def test_slots_equal_the_reference_examples(oz, golden_episodes):
    """every episode of episodes.npz through a one-game engine and append_engine (one-hot, final-board aliasing): the slots are the
    examples execute_episode returned"""
    from othellozero_amd.replay import ReplayBuffer
    g = golden_episodes
    for name in (str(x) for x in g["names"]):
        n, sims, seed, game, salt, keep, qmode, k = (int(x) for x in g[f"{name}/meta"])
        c, T, eg = (float(x) for x in g[f"{name}/params"])
        eng = _stub_engine(n, salt, keep, 1, sims, c, T, eg, seed, game, qmode)
        eng.play_to_end()
        buf = ReplayBuffer(n, 8 * k)
        assert buf.append_engine(eng, alias_final=True) == k and len(buf) == 8 * k == buf.total, name
        own, opp, pi, z = buf.read()
        eb, ep, ez = g[f"{name}/ex_board"], g[f"{name}/ex_policy"], g[f"{name}/ex_z"]
        assert np.array_equal(own, eb[:, 0]) and np.array_equal(opp, eb[:, 1]), name
        want = np.zeros((8 * k, n * n), np.float32)
        want[np.arange(8 * k), ep] = 1
        assert pi.tobytes() == want.tobytes() and z.tobytes() == ez.astype(np.float32).tobytes(), name


def test_slots_equal_the_reference_visit_targets(oz):
    """ep6_T05 of policy_temps.npz (every move's pi at T = 0.5, computed by the reference): slot 8i+7 holds float32(pi[i]), the other
    seven its training_example_symmetries, the boards are those at the moves"""
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.training import training_example_symmetries
    g = load_golden("policy_temps.npz")
    name = "ep6_T05"
    n, sims, seed, game, salt, keep, qmode, k = (int(x) for x in g[f"{name}/meta"])
    c, T, eg = (float(x) for x in g[f"{name}/params"])
    eng = _stub_engine(n, salt, keep, 1, sims, c, T, eg, seed, game, qmode, record_visits=True)
    eng.play_to_end()
    buf = ReplayBuffer(n, 8 * k)
    assert buf.append_engine(eng, policy_target="visits", target_temperature=0.5) == k
    own, opp, pi, z = buf.read()
    assert np.array_equal(own[7::8], g[f"{name}/black"]) and np.array_equal(opp[7::8], g[f"{name}/white"])
    assert z.tobytes() == g[f"{name}/ex_z"].astype(np.float32).tobytes()
    for i in range(k):
        p32 = g[f"{name}/pi"][i].astype(np.float32)
        assert pi[8 * i + 7].tobytes() == p32.tobytes(), i
        want = [p for _, p in training_example_symmetries(np.zeros((n, n)), p32)]
        assert all(np.array_equal(pi[8 * i + t].reshape(n, n), want[t]) for t in range(8)), i
    assert replay_ref.same((own, opp, pi, z), replay_ref.examples(replay_ref.episode_records(g, name), n, False, g[f"{name}/counts"], 0.5))


@pytest.mark.parametrize("n", [4, 6, 8])
def test_slots_equal_the_model_and_the_host_path(oz, n):
    """16 concurrent games, both alias settings, one-hot and visit targets at T = 1, 0.5, 0.7: the buffer equals the NumPy model AND
    pack_examples(examples_from_records(...)) on the same records, byte for byte"""
    from othellozero_amd.replay import ReplayBuffer
    eng, rec, cnt = _games(n)
    buf = ReplayBuffer(n, 8 * rec.size)
    for alias_final in (0, 1):
        for target, T in TARGETS:
            buf.clear()
            assert buf.append_engine(eng, **_kw(alias_final, target, T)) == rec.size
            got = buf.read()
            assert buf.info() == (8 * rec.size, 8 * rec.size, 8 * rec.size)
            model = replay_ref.examples(rec, n, alias_final, cnt if target == "visits" else None, T)
            host = _host_path(rec, cnt, n, alias_final, target, T)
            assert replay_ref.same(got, model), (alias_final, target, T)
            assert replay_ref.same(got, host), (alias_final, target, T)
            if target == "visits":
                assert np.allclose(got[2].sum(axis=1), 1.0, rtol=0, atol=1e-5)


# ------------------------------------------------------------------ order independence
@pytest.mark.parametrize("n", [4, 6, 8])
def test_contents_do_not_depend_on_the_order_of_the_records(oz, n):
    """append_records with the records (and their counts) randomly permuted gives the buffer of append_engine, byte for byte; a
    first_record > 0 appends the engine's remaining records in (game_id, ply) order too"""
    from othellozero_amd.replay import ReplayBuffer
    eng, rec, cnt = _games(n)
    a, b = ReplayBuffer(n, 8 * rec.size), ReplayBuffer(n, 8 * rec.size)
    rs = np.random.RandomState(n)
    for target, T in (("onehot", None), ("visits", 0.7)):
        a.clear(); b.clear()
        a.append_engine(eng, **_kw(0, target, T))
        p = rs.permutation(rec.size)
        assert b.append_records(rec[p], cnt[p] if target == "visits" else None, **_kw(0, target, T)) == rec.size
        assert replay_ref.same(a.read(), b.read()), target
        b.clear()
        b.append_records(rec, cnt if target == "visits" else None, **_kw(0, target, T))
        assert replay_ref.same(a.read(), b.read()), target
    # the tail of the engine's own buffer (completion order, not sorted): compare with the model on exactly those records
    raw = np.zeros(rec.size, oz.RECORD_DTYPE)
    got = C.c_int64()
    oz.check(oz.load().oz_selfplay_records(eng._h, raw.ctypes.data_as(C.c_void_p), rec.size, C.byref(got)))
    first = rec.size // 3
    a.clear()
    assert a.append_engine(eng, first_record=first) == rec.size - first
    assert replay_ref.same(a.read(), replay_ref.examples(raw[first:], n, False))
    assert a.append_engine(eng, first_record=rec.size) == 0 and a.total == 8 * (rec.size - first)


# ------------------------------------------------------------------ ring
@pytest.mark.parametrize("target,T", [("onehot", None), ("visits", 1.0)])
def test_ring(oz, tmp_path, target, T):
    """capacity 100 (no multiple of 8: records straddle the wrap), appends of 3, 10, 1, 30 (more than the capacity) and 2 records: info and
    every held slot follow the model's ring after each; save / load, append_examples and clear"""
    from othellozero_amd.replay import ReplayBuffer
    n, cap = 6, 100
    _, rec, cnt = _games(n)
    buf, ring = ReplayBuffer(n, cap), replay_ref.Ring(cap, n)
    at = 0
    for R in (3, 10, 1, 30, 2):
        part, pc = rec[at:at + R], cnt[at:at + R] if target == "visits" else None
        at += R
        buf.append_records(part[::-1], None if pc is None else pc[::-1], **_kw(0, target, T))
        ring.append(*replay_ref.examples(part, n, False, pc, T))
        assert buf.info() == (ring.held, cap, ring.total) and len(buf) == ring.held and buf.capacity == cap and buf.total == ring.total
        assert replay_ref.same(buf.read(), ring.read()), R
    assert buf.total == 368
    assert replay_ref.same(buf.read(10, 5), tuple(x[10:15] for x in ring.read()))
    # save / load: the same slots and the same running index, so later appends land where they would have
    path = str(tmp_path / "replay.npz")
    buf.save(path)
    back = ReplayBuffer.load(path)
    assert back.info() == buf.info() and back.n == n and replay_ref.same(back.read(), buf.read())
    more = replay_ref.examples(rec[at:at + 4], n, False, cnt[at:at + 4] if target == "visits" else None, T)
    for x in (buf, back):
        x.append_examples(*more)
    ring.append(*more)
    assert replay_ref.same(buf.read(), ring.read()) and replay_ref.same(back.read(), ring.read()) and back.total == ring.total == 400
    # a buffer saved before it wrapped
    small = ReplayBuffer(n, cap)
    small.append_examples(*(x[:44] for x in more))                      # (more holds 32: all of it)
    small.save(path)
    again = ReplayBuffer.load(path)
    assert again.info() == small.info() == (32, cap, 32) and replay_ref.same(again.read(), small.read())
    # append_examples larger than the capacity keeps the last `capacity`
    big = tuple(np.concatenate([x, x, x, x]) for x in more)             # 128 examples
    ring2, buf2 = replay_ref.Ring(cap, n), ReplayBuffer(n, cap)
    for part in (more, big):
        ring2.append(*part)
        buf2.append_examples(*part)
    assert buf2.info() == (cap, cap, 160) and replay_ref.same(buf2.read(), ring2.read())
    buf.clear()
    assert buf.info() == (0, cap, 0) and buf.read()[0].size == 0
    with pytest.raises(oz.OzError):
        buf.read(0, 1)


# ------------------------------------------------------------------ trainer
@pytest.mark.parametrize("precision,C_", [("f32", 128), ("bf16x3", 256)])
def test_fit_from_the_buffer_equals_the_resident_fit(oz, precision, C_):
    """44 examples (the last batch of 8 is short), 2 epochs: fit_replay from the buffer and fit(resident=True) on the buffer's read()
    with the same shuffle_seed take the same steps -- identical weights (all 40 arrays) and identical loss histories"""
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.trainer import Trainer, fit, fit_replay
    from othellozero_amd.weights import init_weights
    n, bs = 6, 8
    _, rec, cnt = _games(n)
    buf = ReplayBuffer(n, 44)
    buf.append_records(rec[:6], cnt[:6], policy_target="visits", target_temperature=1.0)        # 48 examples: the last 44 stay
    assert len(buf) == 44 and buf.total == 48
    runs = []
    for from_buffer in (True, False):
        tr = Trainer(n, C_, 2, max_batch=bs, seed=9, precision=precision, policy_loss="flat")
        tr.set_weights(init_weights(n, seed=1, channels=C_))
        if from_buffer:
            h = fit_replay(tr, buf, batch_size=bs, epochs=2, shuffle_seed=5)
        else:
            h = fit(tr, *buf.read(), batch_size=bs, epochs=2, shuffle_seed=5, resident=True)
        runs.append((tr.get_weights(), h.history, tr.step))
    (w0, h0, s0), (w1, h1, s1) = runs
    assert s0 == s1 == 2 * 6
    assert len(w0) == 40 and all(np.array_equal(a, b) for a, b in zip(w0, w1))
    assert h0 == h1 and len(h0["loss"]) == 2 and np.isfinite(h0["loss"]).all()
    # a data set set AFTER an epoch from the buffer still works (the two paths share the order buffer)
    tr.set_dataset(*buf.read())
    assert np.isfinite(tr.fit_epoch(np.arange(44), bs)).all()


# ------------------------------------------------------------------ loop
def _loop_kw(tmp_path, n):
    return dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
                evaluation_interval=2, evaluation_iterations=2, temperature_threshold=0, self_play_training=False, self_play_interval=1,
                self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
                training_buffer_size=8 * 40 * 8, seed=13)


def test_training_loop_on_the_device_buffer(oz, tmp_path, monkeypatch):
    """one iteration of training(replay="device") with one-hot and with visit targets: it trains (finite losses, changed weights) without
    ever building example tuples; the default replay="host" still goes through examples_from_records"""
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    random.seed(5)
    np.random.seed(5)
    n = 6

    def no_tuples(*a, **k):
        raise AssertionError("the host tuple path was taken")
    monkeypatch.setattr(loop, "examples_from_records", no_tuples)
    for kw in (dict(policy_target="onehot"), dict(policy_target="visits", alias_final_boards=False)):
        net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8,
                          policy_loss="flat" if kw["policy_target"] == "visits" else "rows")
        before = net.get_weights()
        hists, orig = [], net.train

        def spy(examples, orig=orig, hists=hists, **k):
            from othellozero_amd.replay import ReplayBuffer
            assert isinstance(examples, ReplayBuffer) and len(examples) > 8 * 8 * 8
            hists.append(orig(examples, **k))
            return hists[-1]
        net.train = spy
        assert loop.training(neural_network=net, replay="device", **kw, **_loop_kw(tmp_path, n)) == []
        assert len(hists) == 1 and all(len(v) == 1 and np.isfinite(v).all() for v in hists[0].history.values()), hists[0].history
        after = loop.training.last_network.get_weights()
        assert loop.training.last_network is net and any(not np.array_equal(a, b) for a, b in zip(before, after))
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    with pytest.raises(AssertionError, match="host tuple path"):
        loop.training(neural_network=net, **_loop_kw(tmp_path, n))


# ------------------------------------------------------------------ errors
def test_refusals(oz):
    """each is OZ_ERR_ARG with a message that names the problem"""
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.trainer import Trainer
    lib = oz.load()

    def refused(call, word):
        with pytest.raises(oz.OzError) as e:
            call()
        assert e.value.code == oz.OZ_ERR_ARG and word in str(e.value), str(e.value)
    eng6, rec, cnt = _games(6)
    plain = _stub_engine(4, 9, 0, 2, 4, 1.0, 1.0, 0.9, 1, 0, 1)                  # no record_visits
    plain.play_to_end()
    buf4, buf6 = ReplayBuffer(4, 64), ReplayBuffer(6, 64)
    refused(lambda: buf4.append_engine(eng6), "6 x 6")
    refused(lambda: buf4.append_engine(plain, policy_target="visits"), "record_visits")
    refused(lambda: buf6.append_engine(eng6, policy_target="visits", target_temperature=0.0), "temperature")
    refused(lambda: buf6.append_records(rec[:2], None, policy_target="visits"), "counts")
    refused(lambda: buf6.append_engine(eng6, first_record=-1), "first_record")
    refused(lambda: ReplayBuffer(6, 0), "capacity")
    refused(lambda: ReplayBuffer(5, 8), "board size")
    h = C.c_void_p()
    assert lib.oz_replay_create(C.byref(h), 6, 1 << 31) == oz.OZ_ERR_ARG and b"capacity" in lib.oz_last_error()
    assert lib.oz_replay_append_selfplay(buf6._h, eng6._h, 0, 2, 0, 1.0, None) == oz.OZ_ERR_ARG and b"alias_final" in lib.oz_last_error()
    assert lib.oz_replay_append_selfplay(buf6._h, eng6._h, 0, 0, 2, 1.0, None) == oz.OZ_ERR_ARG and b"target" in lib.oz_last_error()
    assert buf6.total == 0 and buf4.total == 0                               # a refused call appends nothing
    buf6.append_records(rec[:2])
    refused(lambda: buf6.read(0, 17), "holds 16")
    refused(lambda: buf6.read(16, 1), "holds 16")
    tr = Trainer(6, 128, 2, max_batch=8, seed=1)
    refused(lambda: tr.fit_epoch_replay(buf6, [0, 16], 8), "index 16")
    refused(lambda: tr.fit_epoch_replay(buf6, [-1], 8), "index -1")
    refused(lambda: tr.fit_epoch_replay(buf6, [0, 1], 9), "batch 9")
    refused(lambda: tr.fit_epoch_replay(buf6, [0, 1], 0), "batch 0")
    buf8 = ReplayBuffer(8, 8)
    refused(lambda: tr.fit_epoch_replay(buf8, [0], 8), "8 x 8")
    assert tr.step == 0
