"""Policy surprise weighting on the GPU (pytest -m gpu): the recorded surprises against a hand-driven oracle search, the switch changing no
record, the drivers agreeing (forced playouts, Gumbel, playout cap), the device weights against the host functions bit for bit, the contents
of the replay buffer after weighted appends against the restatement (tests/surprise_ref.py), and one iteration of the loop.  Stub network
(the loop: a tiny real one), a handful of small games."""
import ctypes as C
import logging

import numpy as np
import pytest

import oracle
import replay_ref
import surprise_ref as ref

pytestmark = pytest.mark.gpu

SALT, C_PUCT, EG, SEED, FIRST, G = 9, 1.25, 0.8, 777, 1000, 16


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _engine(n, keep, games, sims, T, qmode, salt=SALT, K=1, **kw):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(StubNetWrapper((n, n), salt, keep, max_batch=games * K), n, games, sims, C_PUCT, T, EG, seed=SEED, first_game_id=FIRST,
                          q_mode=qmode, leaves_per_step=K, **kw)


_PLAYED = {}


def _played(n, sims, qmode, keep):
    """16 finished games, played once per configuration: (engine, records, counts, values, surprises), sorted by (game_id, ply)"""
    key = (n, sims, qmode, keep)
    if key not in _PLAYED:
        eng = _engine(n, keep, G, sims, 1.0, qmode, record_visits=True, record_values=True, record_surprise=True)
        eng.play_to_end()
        assert eng.stats()["games_completed"] == G
        _PLAYED[key] = (eng,) + eng.records(with_visits=True, with_values=True, with_surprise=True)
    return _PLAYED[key]


_PRIORS = {}


def _oracle_priors(n, rec, keep=0, salt=SALT):
    """the stored priors of the roots of `rec`, float64 (R, 64) by square: a position's priors do not depend on the search that reaches it,
    so two oracle simulations from the position give them"""
    P = np.zeros((rec.size, 64), np.float64)
    for i in range(rec.size):
        black, white, player = int(rec["black"][i]), int(rec["white"][i]), int(rec["player"][i])
        key = (n, keep, salt, black, white, player)
        if key not in _PRIORS:
            m = oracle.Mcts(n, C_PUCT, 1, salt=salt, keep_mask=keep)
            m.simulate(black, white, player)
            m.simulate(black, white, player)
            own, opp = (black, white) if player == 1 else (white, black)
            _PRIORS[key] = m.dump_node(m.L.orc_mcts_find(m.h, own, opp))["P"].astype(np.float64)
        P[i] = _PRIORS[key]
    return P


def _within_bound(got, rows, P):
    want, abs_sum = ref.surprises(rows, P)
    return bool((np.abs(got - want) <= ref.bound(abs_sum)).all())


# ------------------------------------------------------------------ 1. surprises against the oracle
@pytest.mark.parametrize("n,sims,qmode,keep", [(6, 30, 0, 7), (4, 50, 1, 3)])
def test_surprises_vs_hand_driven_oracle(oz, n, sims, qmode, keep):
    """every recorded move: `sims` oracle simulations from the record's position in the game's own tree, then the root's N must be the
    recorded counts, the host function of the root's N and P the recorded surprise bit for bit, and the restatement within its bound"""
    from othellozero_amd import agents
    _, rec, cnt, _, sur = _played(n, sims, qmode, keep)
    assert rec.size == cnt.shape[0] == sur.size and sur.dtype == np.float64
    N, P = np.zeros((rec.size, 64), np.int32), np.zeros((rec.size, 64), np.float64)
    for gid in range(FIRST, FIRST + G):
        sel = np.flatnonzero(rec["game_id"] == gid)
        assert rec["ply"][sel].tolist() == list(range(sel.size))
        m = oracle.Mcts(n, C_PUCT, qmode, salt=SALT, keep_mask=keep)
        for i in sel:
            black, white, player = int(rec["black"][i]), int(rec["white"][i]), int(rec["player"][i])
            for _ in range(sims):
                m.simulate(black, white, player)
            own, opp = (black, white) if player == 1 else (white, black)
            root = m.dump_node(m.L.orc_mcts_find(m.h, own, opp))
            assert (root["k0"], root["k1"]) == (own, opp)
            assert np.array_equal(root["N"], cnt[i]), (gid, i)
            N[i], P[i] = root["N"], root["P"]
    want = agents.rules_policy_surprise(N, P)
    assert _same_bits(sur, want)
    assert _within_bound(sur, N, P)
    assert np.isfinite(sur).all() and (sur >= 0).all() and np.count_nonzero(sur > 0) > sur.size // 2


# ------------------------------------------------------------------ 2. the switch is inert
def test_switch_changes_no_record(oz):
    n, sims = 6, 12

    def played(**kw):
        eng = _engine(n, 0, 8, sims, 1.0, 1, record_visits=True, **kw)
        eng.play_to_end()
        return eng
    off, on = played(), played(record_surprise=True)
    assert off.stats() == on.stats() and off.stats()["games_completed"] == 8
    a, b = off.records(with_visits=True), on.records(with_visits=True)
    assert a[0].size > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(ValueError):
        off.records(with_surprise=True)
    with pytest.raises(oz.OzError):
        off.surprise_weights(0.5, 1)
    with pytest.raises(oz.OzError):
        on.records(with_weights=True)                      # before the first surprise_weights()
    lib = oz.load()
    # before the first driver call only
    assert lib.oz_selfplay_set_record_surprise(on._h, 0) == oz.OZ_ERR_STATE
    assert lib.oz_selfplay_set_record_surprise(off._h, 1) == oz.OZ_ERR_STATE
    fresh = _engine(n, 0, 8, sims, 1.0, 1, record_visits=True)
    assert lib.oz_selfplay_set_record_surprise(fresh._h, 2) == oz.OZ_ERR_ARG
    assert lib.oz_selfplay_set_record_surprise(None, 1) == oz.OZ_ERR_ARG
    for enable in (1, 0, 1):
        oz.check(lib.oz_selfplay_set_record_surprise(fresh._h, enable))
    fresh.record_surprise = True
    fresh.play_to_end()
    assert _same_bits(fresh.records(with_surprise=True)[1], on.records(with_surprise=True)[1])
    # it needs a recorded policy target
    bare = _engine(n, 0, 8, sims, 1.0, 1)
    assert lib.oz_selfplay_set_record_surprise(bare._h, 1) == oz.OZ_ERR_ARG
    with pytest.raises(ValueError, match="record_visits"):
        _engine(n, 0, 8, sims, 1.0, 1, record_surprise=True)
    for frac in (0.0, 1.5, float("nan")):
        assert lib.oz_selfplay_surprise_weights(on._h, 0, frac, 1, None) == oz.OZ_ERR_ARG
    assert lib.oz_selfplay_surprise_weights(on._h, -1, 0.5, 1, None) == oz.OZ_ERR_ARG


# ------------------------------------------------------------------ 3. the drivers agree
def _by_key(rec, val):
    return {(int(g), int(p)): v.tobytes() for g, p, v in zip(rec["game_id"], rec["ply"], val)}


def test_drivers_agree(oz):
    """lock-step with dedup against free-running with refill and without dedup, 64 games: one surprise per (game_id, ply); and the same
    with move sampling and recorded values switched on as well"""
    n, sims, games = 6, 10, 64
    kw = dict(record_visits=True, record_surprise=True)
    lock = _engine(n, 0, games, sims, 1.0, 1, **kw)
    lock.play_to_end()
    rec_l, sur_l = lock.records(with_surprise=True)
    free = _engine(n, 0, games, sims, 1.0, 1, refill=True, game_id_stride=games, dedup=False, **kw)
    free.run_steps(2 * sims * (n * n - 4) + 8 * sims)
    rec_f, sur_f = free.records(with_surprise=True)
    want, got = _by_key(rec_l, sur_l), _by_key(rec_f, sur_f)
    assert len(want) == rec_l.size and np.unique(rec_f["game_id"]).size > games
    assert all(got[k] == v for k, v in want.items())
    kw = dict(record_visits=True, record_surprise=True, record_values=True, sample_moves=(1.0, 4))
    a = _engine(n, 0, 16, sims, 1.0, 1, **kw)
    a.play_to_end()
    b = _engine(n, 0, 16, sims, 1.0, 1, **kw)
    for _ in range(64):
        b.run_steps(4 * sims)
        if b.stats()["live_games"] == 0:
            break
    assert b.stats()["games_completed"] == 16
    ra, ca, va, sa = a.records(with_visits=True, with_values=True, with_surprise=True)
    rb, cb, vb, sb = b.records(with_visits=True, with_values=True, with_surprise=True)
    assert ra.tobytes() == rb.tobytes() and _same_bits(sa, sb) and _same_bits(va, vb) and _same_bits(ca, cb) and (ra["greedy"] == 2).any()
    # leaves_per_step = 4 goes through the same move
    k4 = _engine(n, 0, 8, 12, 1.0, 1, K=4, record_visits=True, record_surprise=True)
    k4.play_to_end()
    r4, c4, s4 = k4.records(with_visits=True, with_surprise=True)
    from othellozero_amd import agents
    assert _same_bits(s4, agents.rules_policy_surprise(c4, _oracle_priors(n, r4)))


def test_forced_playouts_surprise_is_that_of_the_pruned_row(oz):
    """forced playouts under root noise, lock-step and free-running: the surprise is the host function of the RECORDED (pruned) row and the
    root's stored priors (the oracle's: noise never touches them)"""
    from othellozero_amd import agents
    n, sims = 6, 24
    kw = dict(record_visits=True, record_surprise=True, root_noise=(0.6, 0.25), forced_playouts=2.0)
    lock = _engine(n, 0, G, sims, 1.0, 1, **kw)
    lock.run(1)
    raw = lock.last_counts()
    lock.play_to_end()
    rec, cnt, sur = lock.records(with_visits=True, with_surprise=True)
    assert lock.forced_playout_stats()["moves_pruned"] > 0
    P = _oracle_priors(n, rec)
    assert _same_bits(sur, agents.rules_policy_surprise(cnt, P)) and _within_bound(sur, cnt, P)
    first = np.flatnonzero(rec["ply"] == 0)
    differ = [g for g in range(G) if not np.array_equal(cnt[first[g]], raw[g])]
    assert differ                                          # some first move's row is pruned: its surprise is not that of the raw counts
    g = differ[0]
    assert sur[first[g]] != float(agents.rules_policy_surprise(raw[g], P[first[g]]))
    free = _engine(n, 0, G, sims, 1.0, 1, **kw)
    for _ in range(64):
        free.run_steps(4 * sims)
        if free.stats()["live_games"] == 0:
            break
    rf, cf, sf = free.records(with_visits=True, with_surprise=True)
    assert rf.tobytes() == rec.tobytes() and _same_bits(cf, cnt) and _same_bits(sf, sur)


def test_gumbel_surprise_is_that_of_the_improved_row(oz):
    from othellozero_amd import agents
    n, sims = 6, 16
    eng = _engine(n, 0, G, sims, 1.0, 1, gumbel=(4, 50.0, 1.0), record_surprise=True)
    eng.play_to_end()
    rec, rows, sur = eng.records(with_policies=True, with_surprise=True)
    assert rows.dtype == np.float32 and (rec["greedy"] == 3).any()
    P = _oracle_priors(n, rec)
    assert _same_bits(sur, agents.rules_policy_surprise(rows, P)) and _within_bound(sur, rows, P)
    assert np.count_nonzero(sur > 0) > sur.size // 2
    plain = _engine(n, 0, G, sims, 1.0, 1, gumbel=(4, 50.0, 1.0))
    plain.play_to_end()
    r0, rows0 = plain.records(with_policies=True)
    assert r0.tobytes() == rec.tobytes() and rows0.tobytes() == rows.tobytes()


def _check_weights(oz, eng, frac, seed):
    """the device's weights, copies and first symmetries against the host functions and the restatement; -> (records, surprises, w, c, t0)"""
    from othellozero_amd import agents
    stats = eng.surprise_weights(frac, seed)
    rec, sur, (w, c, t0) = eng.records(with_surprise=True, with_weights=True)
    assert w.dtype == np.float32 and c.dtype == np.int32 and t0.dtype == np.uint8
    hw = agents.rules_surprise_weights(rec, sur, frac)
    hc, ht = agents.rules_surprise_copies(rec, hw, seed)
    assert _same_bits(w, hw) and _same_bits(c, hc) and _same_bits(t0, ht)
    assert _same_bits(hw, ref.weights(rec, sur, frac))
    rc, rt = ref.copies(rec, hw, seed)
    assert _same_bits(hc, rc) and _same_bits(ht, rt)
    full = oz.record_fast(rec) == 0
    assert stats == dict(records=rec.size, full_records=int(full.sum()), examples=int(c.sum()), zero_copies=int((c[full] == 0).sum()),
                         max_copies=int(c.max()))
    return rec, sur, w, c, t0


def test_playout_cap_fast_records_weigh_nothing(oz):
    n = 6
    eng = _engine(n, 0, G, 20, 1.0, 1, record_visits=True, record_surprise=True, playout_cap=(10, 0.5))
    eng.play_to_end()
    rec, sur, w, c, t0 = _check_weights(oz, eng, 0.5, 31)
    fast = oz.record_fast(rec) != 0
    assert 0 < fast.sum() < rec.size and (w[fast] == 0).all() and (c[fast] == 0).all()
    assert (sur[fast] > 0).any()                           # recorded, never used
    for gid in np.unique(rec["game_id"]):
        m = (rec["game_id"] == gid) & ~fast
        K = int(m.sum())
        if K:
            wg = w[m].astype(np.float64)
            assert abs(wg.sum() - K) <= K * 2.0 ** -23 * wg.max()


# ------------------------------------------------------------------ 4. device outputs against the host functions
def test_weights_equal_the_host_functions(oz):
    from othellozero_amd import agents
    n = 6
    eng = _played(n, 30, 0, 7)[0]
    for frac, seed in ((0.5, 11), (1.0, 12), (0.25, 2 ** 63 + 5)):
        rec, sur, w, c, t0 = _check_weights(oz, eng, frac, seed)
    assert (c > 8).any() and ((c < 8) & (c >= 0)).any() and set(np.unique(t0)) == set(range(8))
    # first_record in the middle of a game: that game is still normalised over all of its records; earlier entries stay
    eng.surprise_weights(0.5, 11)
    R = rec.size
    lib, got = oz.load(), C.c_int64()
    ring = np.zeros(R, oz.RECORD_DTYPE)
    oz.check(lib.oz_selfplay_records(eng._h, ring.ctypes.data_as(C.c_void_p), R, C.byref(got)))
    rsur = np.zeros(R, np.float64)
    oz.check(lib.oz_selfplay_surprises(eng._h, oz.p_f64(rsur), R, C.byref(got)))

    def raw():
        w, c, t = np.zeros(R, np.float32), np.zeros(R, np.int32), np.zeros(R, np.uint8)
        oz.check(lib.oz_selfplay_weights(eng._h, oz.p_f32(w), oz.p_i32(c), oz.p_u8(t), R, C.byref(got)))
        assert got.value == R
        return w, c, t
    before = raw()
    first = next(i for i in range(5, R) if ring["ply"][i] >= 2 and ring["game_id"][i + 1] == ring["game_id"][i])
    stats = eng.surprise_weights(0.8, 77, first_record=first)
    after = raw()
    assert stats["records"] == R - first and all(_same_bits(a[:first], b[:first]) for a, b in zip(after, before))
    hw = agents.rules_surprise_weights(ring, rsur, 0.8)
    hc, ht = agents.rules_surprise_copies(ring, hw, 77)
    assert _same_bits(after[0][first:], hw[first:]) and _same_bits(after[1][first:], hc[first:]) and _same_bits(after[2][first:], ht[first:])
    assert stats["examples"] == int(hc[first:].sum()) and stats["max_copies"] == int(hc[first:].max())
    assert eng.surprise_weights(0.5, 1, first_record=R + 5)["records"] == 0


# ------------------------------------------------------------------ 5. the replay buffer
def _read_equals(buf, ring):
    return replay_ref.same(buf.read(), ring.read()) and buf.info() == (ring.held, ring.capacity, ring.total)


def test_replay_buffer_writes_the_copies(oz):
    """visit and one-hot targets, with and without TD value targets, both alias settings: a buffer smaller than the append whose capacity
    is no multiple of 8 wraps and skips; a second append lands on top of the first; total advances by the sum of the copy counts"""
    from othellozero_amd import agents
    from othellozero_amd.replay import ReplayBuffer
    n, frac, vt = 6, 0.5, ("td", 0.7)
    eng, rec, cnt, val, sur = _played(n, 30, 0, 7)
    tgt = agents.rules_value_targets(rec, val, n, vt)
    w = ref.weights(rec, sur, frac)
    cases = [("visits", 1.0, False, None), ("onehot", None, False, None), ("onehot", None, True, None), ("visits", 0.5, False, vt),
             ("onehot", None, False, vt)]
    for target, T, alias, value_target in cases:
        (c1, t1), (c2, t2) = ref.copies(rec, w, 5), ref.copies(rec, w, 6)
        assert (c1 > 8).any() and (c1 < 8).any()
        E1, E2 = int(c1.sum()), int(c2.sum())
        cap = E1 - 8 * 3 - 5
        assert cap % 8 != 0 and 0 < cap < E1
        buf, ring = ReplayBuffer(n, cap), replay_ref.Ring(cap, n)
        kw = dict(alias_final=alias, policy_target=target, target_temperature=T or 1.0, **({"value_target": value_target} if value_target else {}))
        rkw = dict(alias_final=alias, counts=cnt if target == "visits" else None, T=T, z=tgt if value_target else None)
        assert buf.append_engine(eng, surprise_weight=(frac, 5), **kw) == rec.size
        assert buf.last_examples == E1 and buf.total == E1
        ring.append(*ref.examples(rec, n, c1, t1, **rkw))
        assert _read_equals(buf, ring), (target, T, alias, value_target)
        assert buf.append_engine(eng, surprise_weight=(frac, 6), **kw) == rec.size
        assert buf.total == E1 + E2
        ring.append(*ref.examples(rec, n, c2, t2, **rkw))
        assert _read_equals(buf, ring), (target, T, alias, value_target)
        # a buffer with room for everything holds every example in order
        big = ReplayBuffer(n, E1 + 3)
        big.append_engine(eng, surprise_weight=(frac, 5), **kw)
        assert replay_ref.same(big.read(), ref.examples(rec, n, c1, t1, **rkw)) and big.info() == (E1, E1 + 3, E1)
    # without the option the append is what it was
    plain = ReplayBuffer(n, 8 * rec.size)
    assert plain.append_engine(eng, policy_target="visits") == rec.size
    assert replay_ref.same(plain.read(), replay_ref.examples(rec, n, False, cnt, 1.0))
    # a first_record past the first games appends the later records only
    part = ReplayBuffer(n, 8 * rec.size)
    lib, got = oz.load(), C.c_int64()
    ring_rec = np.zeros(rec.size, oz.RECORD_DTYPE)
    oz.check(lib.oz_selfplay_records(eng._h, ring_rec.ctypes.data_as(C.c_void_p), rec.size, C.byref(got)))
    first = next(i for i in range(5, rec.size) if ring_rec["ply"][i] == 0)
    later = np.isin(rec["game_id"].astype(np.int64) * 64 + rec["ply"], ring_rec["game_id"][first:].astype(np.int64) * 64 + ring_rec["ply"][first:])
    assert part.append_engine(eng, first_record=first, policy_target="visits", surprise_weight=(frac, 5)) == int(later.sum())
    c1, t1 = ref.copies(rec, w, 5)
    assert replay_ref.same(part.read(), ref.examples(rec[later], n, c1[later], t1[later], counts=cnt[later], T=1.0))
    with pytest.raises(ValueError):
        plain.append_engine(eng, surprise_weight=(0.0, 1))
    with pytest.raises(ValueError):
        plain.append_engine(eng, surprise_weight=0.5)
    bare = _engine(n, 0, 4, 8, 1.0, 1, record_visits=True)
    bare.play_to_end()
    with pytest.raises(oz.OzError):
        plain.append_engine(bare, surprise_weight=(0.5, 1))


def test_replay_buffer_improved_targets_and_playout_cap(oz):
    from othellozero_amd.replay import ReplayBuffer
    n, frac = 6, 0.5
    eng = _engine(n, 0, G, 16, 1.0, 1, gumbel=(4, 50.0, 1.0), record_surprise=True)
    eng.play_to_end()
    rec, rows, sur = eng.records(with_policies=True, with_surprise=True)
    c, t0 = ref.copies(rec, ref.weights(rec, sur, frac), 9)
    E = int(c.sum())
    cap = E - 21
    buf, ring = ReplayBuffer(n, cap), replay_ref.Ring(cap, n)
    assert buf.append_engine(eng, policy_target="improved", surprise_weight=(frac, 9)) == rec.size and buf.total == E
    ring.append(*ref.examples(rec, n, c, t0, policies=rows))
    assert _read_equals(buf, ring)
    # a playout cap: the fast records stay out, the return value counts the fully searched ones
    cap_eng = _engine(n, 0, G, 20, 1.0, 1, record_visits=True, record_surprise=True, playout_cap=(10, 0.5))
    cap_eng.play_to_end()
    rec, cnt, sur = cap_eng.records(with_visits=True, with_surprise=True)
    full = oz.record_fast(rec) == 0
    c, t0 = ref.copies(rec, ref.weights(rec, sur, frac), 9)
    buf = ReplayBuffer(n, int(c.sum()) + 1)
    assert buf.append_engine(cap_eng, policy_target="visits", surprise_weight=(frac, 9)) == int(full.sum()) and buf.total == int(c.sum())
    assert replay_ref.same(buf.read(), ref.examples(rec, n, c, t0, counts=cnt, T=1.0))


def test_selfplay_batch_returns_the_weights(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import selfplay_batch
    n = 6
    net = StubNetWrapper((n, n), SALT, 0, max_batch=8)
    plain = selfplay_batch(net, n, 8, 10, C_PUCT, 1.0, EG, seed=5, record_visits=True)
    rec, cnt, sur, (w, c, t0) = selfplay_batch(net, n, 8, 10, C_PUCT, 1.0, EG, seed=5, record_visits=True, surprise_weight=(0.5, 3))
    assert rec.tobytes() == plain[0].tobytes() and cnt.tobytes() == plain[1].tobytes()
    assert _same_bits(w, ref.weights(rec, sur, 0.5)) and _same_bits(c, ref.copies(rec, w, 3)[0]) and _same_bits(t0, ref.copies(rec, w, 3)[1])
    assert selfplay_batch.surprise_stats["examples"] == int(c.sum())
    with pytest.raises(ValueError):
        selfplay_batch(net, n, 8, 10, surprise_weight=(0.5, 3))
    with pytest.raises(ValueError):
        selfplay_batch(net, n, 8, 10, record_visits=True, expand=True, surprise_weight=(0.5, 3))


# ------------------------------------------------------------------ 6. the loop
def _loop_kw(tmp_path, n):
    return dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
                evaluation_interval=2, evaluation_iterations=2, temperature_threshold=0, self_play_training=False, self_play_interval=1,
                self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
                training_buffer_size=8 * 40 * 8, seed=13)


def test_training_with_surprise_weighting(oz, tmp_path, monkeypatch, caplog):
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    n = 6
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8, policy_loss="flat")
    given = []
    fit = net.train

    def spy(data, *a, **kw):
        given.append(len(data))
        return fit(data, *a, **kw)
    monkeypatch.setattr(net, "train", spy)
    kw = dict(neural_network=net, alias_final_boards=False, surprise_weight=0.5, **_loop_kw(tmp_path, n))
    with pytest.raises(ValueError, match="replay='device'"):
        loop.training(replay="host", policy_target="visits", **kw)
    with pytest.raises(ValueError, match="distributed"):
        loop.training(replay="device", policy_target="visits", distributed=True, **kw)
    with pytest.raises(ValueError, match="policy_target"):
        loop.training(replay="device", policy_target="onehot", **kw)
    with pytest.raises(ValueError):
        loop.training(replay="device", policy_target="visits", **{**kw, "surprise_weight": 1.5})
    assert given == []
    with caplog.at_level(logging.INFO):
        assert loop.training(replay="device", policy_target="visits", **kw) == []
    (st,) = loop.training.surprise_history
    assert given == [st["examples"]] and st["examples"] > 0 and st["records"] > 0
    assert abs(st["mean_copies"] - 8.0) < 1.0 and st["max_copies"] >= 8 and st["mean_surprise"] > 0
    assert any("surprise weighting: %d examples" % st["examples"] in r.getMessage() for r in caplog.records)
