"""Value targets on the GPU (pytest -m gpu): the recorded root values against a hand-driven oracle search bit for bit, the switch changing no
record, the drivers agreeing, forced playouts leaving the value on the raw counts, the device targets against the host function, the replay
buffer, the drop-in search and one iteration of the loop.  Stub network (the loop: a tiny real one), a handful of small games."""
import ctypes as C

import numpy as np
import pytest

import oracle
import value_targets_ref as ref

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
    """16 finished games, played once per configuration: (engine, records, counts, values), sorted by (game_id, ply)"""
    key = (n, sims, qmode, keep)
    if key not in _PLAYED:
        eng = _engine(n, keep, G, sims, 1.0, qmode, record_values=True, record_visits=True)
        eng.play_to_end()
        assert eng.stats()["games_completed"] == G
        _PLAYED[key] = (eng,) + eng.records(with_visits=True, with_values=True)
    return _PLAYED[key]


# ------------------------------------------------------------------ 1. root values against the oracle
@pytest.mark.parametrize("n,sims,qmode,keep", [(6, 30, 0, 7), (4, 50, 1, 3)])
def test_root_values_vs_hand_driven_oracle(oz, n, sims, qmode, keep):
    """every recorded move: `sims` oracle simulations from the record's position in the game's own tree, then the root's N must be the
    recorded counts and pairwise_sum(N Q) / sum N the recorded value, bit for bit"""
    _, rec, cnt, val = _played(n, sims, qmode, keep)
    assert rec.size == cnt.shape[0] == val.size and val.dtype == np.float64
    assert sorted(set(rec["game_id"].tolist())) == list(range(FIRST, FIRST + G))
    passes = 0
    for gid in range(FIRST, FIRST + G):
        sel = np.flatnonzero(rec["game_id"] == gid)
        assert rec["ply"][sel].tolist() == list(range(sel.size))
        passes += int((rec["player"][sel][1:] == rec["player"][sel][:-1]).any())
        m = oracle.Mcts(n, C_PUCT, qmode, salt=SALT, keep_mask=keep)
        for i in sel:
            black, white, player = int(rec["black"][i]), int(rec["white"][i]), int(rec["player"][i])
            for _ in range(sims):
                m.simulate(black, white, player)
            own, opp = (black, white) if player == 1 else (white, black)
            root = m.dump_node(m.L.orc_mcts_find(m.h, own, opp))             # the node of dump() whose key is the root's
            assert (root["k0"], root["k1"]) == (own, opp)
            assert np.array_equal(root["N"], cnt[i]), (gid, i)
            want = float(oracle.pairwise_sum(root["N"].astype(np.float64) * root["Q"])) / float(int(root["N"].sum()))
            assert np.float64(want).tobytes() == val[i].tobytes(), (gid, int(rec["ply"][i]), want, val[i])
            assert want == ref.root_value(root["N"], root["Q"])
    assert passes >= 1                                     # two consecutive records of one player: the sign comes from `player`
    assert np.abs(val).max() <= 1.0 and np.count_nonzero(val) > val.size // 2


# ------------------------------------------------------------------ 2. the switch is inert
@pytest.mark.parametrize("visits", [False, True])
def test_switch_changes_no_record(oz, visits):
    n, sims = 6, 12

    def played(**kw):
        eng = _engine(n, 0, 8, sims, 1.0, 1, record_visits=visits, **kw)
        eng.play_to_end()
        return eng
    off, on = played(), played(record_values=True)
    assert off.stats() == on.stats() and off.stats()["games_completed"] == 8
    a, b = off.records(with_visits=visits), on.records(with_visits=visits)
    if visits:
        assert a[1].tobytes() == b[1].tobytes()
        a, b = a[0], b[0]
    assert a.size > 0 and a.tobytes() == b.tobytes()
    with pytest.raises(oz.OzError):
        off.records(with_values=True)
    with pytest.raises(oz.OzError):
        off.value_targets(("td", 0.5))
    # before the first driver call only
    assert oz.load().oz_selfplay_set_record_values(on._h, 0) == oz.OZ_ERR_STATE
    assert oz.load().oz_selfplay_set_record_values(off._h, 1) == oz.OZ_ERR_STATE
    fresh = _engine(n, 0, 8, sims, 1.0, 1)
    assert oz.load().oz_selfplay_set_record_values(fresh._h, 2) == oz.OZ_ERR_ARG
    for enable in (1, 0, 1):
        oz.check(oz.load().oz_selfplay_set_record_values(fresh._h, enable))
    fresh.play_to_end()
    assert _same_bits(fresh.records(with_values=True)[1], on.records(with_values=True)[1])


# ------------------------------------------------------------------ 3. the drivers agree
def _by_key(rec, val):
    return {(int(g), int(p)): v.tobytes() for g, p, v in zip(rec["game_id"], rec["ply"], val)}


def test_drivers_agree(oz):
    """lock-step with dedup against free-running with refill and without dedup, 64 games: one value per (game_id, ply); and the same
    with the free-running kernel of the engines with extras"""
    n, sims, games = 6, 10, 64
    lock = _engine(n, 0, games, sims, 1.0, 1, record_values=True)
    lock.play_to_end()
    rec_l, val_l = lock.records(with_values=True)
    free = _engine(n, 0, games, sims, 1.0, 1, record_values=True, refill=True, game_id_stride=games, dedup=False)
    free.run_steps(2 * sims * (n * n - 4) + 8 * sims)
    rec_f, val_f = free.records(with_values=True)
    want, got = _by_key(rec_l, val_l), _by_key(rec_f, val_f)
    assert len(want) == rec_l.size and np.unique(rec_f["game_id"]).size > games
    assert all(got[k] == v for k, v in want.items())
    # free-running with the extras instantiation (move sampling switches it on) against lock-step with the same option
    kw = dict(record_values=True, sample_moves=(1.0, 4))
    a = _engine(n, 0, 16, sims, 1.0, 1, **kw)
    a.play_to_end()
    b = _engine(n, 0, 16, sims, 1.0, 1, **kw)
    for _ in range(64):
        b.run_steps(4 * sims)
        if b.stats()["live_games"] == 0:
            break
    assert b.stats()["games_completed"] == 16
    ra, va = a.records(with_values=True)
    rb, vb = b.records(with_values=True)
    assert ra.tobytes() == rb.tobytes() and _same_bits(va, vb) and (ra["greedy"] == 2).any()


def test_leaves_per_step_and_stagger(oz):
    """leaves_per_step = 4 and staggered rounds go through the same move: an engine that plays its games in lock step and a refilled
    one brought to its steady state by stagger() agree on the game both play from its first ply, and every record of either has a value"""
    n, sims = 6, 12
    a = _engine(n, 0, 8, sims, 1.0, 1, K=4, record_values=True, record_visits=True)
    a.play_to_end()
    ra, ca, va = a.records(with_visits=True, with_values=True)
    b = _engine(n, 0, 8, sims, 1.0, 1, K=4, record_values=True, record_visits=True, refill=True, game_id_stride=8)
    b.stagger()
    b.run(n * n)
    rb, cb, vb = b.records(with_visits=True, with_values=True)
    assert a.stats()["games_completed"] == 8 and np.abs(va).max() <= 1.0 and np.count_nonzero(va) > va.size // 2
    # slot 0 is not advanced by stagger ((0 * P) // G == 0 plies): its first game is game FIRST of both engines
    sa, sb = ra["game_id"] == FIRST, rb["game_id"] == FIRST
    assert sa.any() and ra[sa].tobytes() == rb[sb].tobytes() and _same_bits(va[sa], vb[sb]) and np.array_equal(ca[sa], cb[sb])
    # staggered rounds record values like any move: every record of the refilled engine has one in range
    assert vb.size == rb.size and np.abs(vb).max() <= 1.0


# ------------------------------------------------------------------ 4. forced playouts: the value reads the raw counts
def test_forced_playouts_leave_the_value_on_the_raw_counts(oz):
    from othellozero_amd import agents
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.othelo_mcts import OthelloMCTS
    n, sims = 6, 24
    kw = dict(record_values=True, record_visits=True, root_noise=(0.6, 0.25))
    forced = _engine(n, 0, G, sims, 1.0, 1, forced_playouts=2.0, **kw)
    forced.run(1)                                          # one move round: every game searched its first root
    raw = forced.last_counts()
    forced.play_to_end()
    rec, cnt, val = forced.records(with_visits=True, with_values=True)
    assert forced.forced_playout_stats()["moves_pruned"] > 0
    first = np.flatnonzero(rec["ply"] == 0)                # (sorted by game id = by slot, like last_counts)
    assert first.size == G
    differ = [g for g in range(G) if not np.array_equal(cnt[first[g]], raw[g])]
    assert differ                                          # some first move's recorded row is pruned ...
    slot = differ[0]
    # ... and its value is that of the raw counts.  The drop-in search of that game's first move (same seed, game id, ply, noise and
    # forcing) gives the raw row, the pruned row and the edge values of one tree
    net = StubNetWrapper((n, n), SALT, 0, max_batch=1)
    from othellozero_amd.Othello import OthelloGame, OthelloPlayer, BoardView
    game = OthelloGame(n)
    m = OthelloMCTS(n, net, C_PUCT, q_mode=1, forced_playouts=2.0)
    state = game.board(BoardView.TWO_CHANNELS)
    m.sample_root_noise(0.6, 0.25, SEED, FIRST + slot, 0, state=state, player=OthelloPlayer.BLACK)
    m.simulate_n(state, OthelloPlayer.BLACK, sims)
    own, opp = oz.pack_board(state)
    (root,) = [d for d in m.dump() if (d["k0"], d["k1"]) == (own, opp)]
    pruned = m.pruned_counts(state)
    assert not np.array_equal(pruned, root["N"]) and np.array_equal(pruned, m.pruned_counts(state))
    v = m.root_value(state)
    assert np.float64(v).tobytes() == agents.rules_root_values(root["N"], root["Q"]).tobytes()
    assert v != float(agents.rules_root_values(pruned, root["Q"]))
    assert v == ref.root_value(root["N"], root["Q"])
    i = int(first[slot])
    assert int(rec["game_id"][i]) == FIRST + slot
    assert np.array_equal(raw[slot], root["N"]) and np.array_equal(cnt[i], pruned) and val[i].tobytes() == np.float64(v).tobytes()
    unknown = np.zeros((n, n, 2), bool)
    unknown[0, 0, 0] = unknown[0, 1, 1] = True              # a board no search has seen
    with pytest.raises(KeyError):
        m.root_value(unknown)


# ------------------------------------------------------------------ 5. targets
def _check_targets(oz, eng, n, E):
    from othellozero_amd import agents
    for vt in (("blend", 0.5), ("td", 0.7)):
        stats = eng.value_targets(vt, exact_empties=E)
        rec, val, tgt = eng.records(with_values=True, with_targets=True)
        want = agents.rules_value_targets(rec, val, n, vt, exact_empties=E)
        assert tgt.dtype == np.float32 and _same_bits(tgt, want), (vt, E)
        assert _same_bits(want, ref.value_targets(rec, val, n, vt, E))
        exact = np.array([E > 0 and ref._empties(r, n) <= E for r in rec])
        assert stats == dict(records=rec.size, exact=int(exact.sum()), sign_changed=int((np.sign(tgt).astype(np.int64) != rec["z"]).sum()))
        assert not set(np.unique(tgt[~exact]).tolist()) <= {-1.0, 0.0, 1.0}
    return rec, val


def test_targets_equal_the_host_function(oz):
    from othellozero_amd import agents
    n = 6
    eng = _played(n, 30, 0, 7)[0]
    rec, val = _check_targets(oz, eng, n, 0)
    z = rec["z"].astype(np.float32)
    # the identities
    for vt, want in (("outcome", z), (("td", 1.0), z), (("blend", 0.0), z), (("td", 0.0), val.astype(np.float32)), (("blend", 1.0), val.astype(np.float32))):
        eng.value_targets(vt)
        assert _same_bits(eng.records(with_targets=True)[1], want), vt
    # first_record in the middle of a game: the chain still runs to that game's end; earlier targets stay
    eng.value_targets(("td", 0.7))
    total = C.c_int64()
    ring = np.zeros(rec.size, oz.RECORD_DTYPE)
    oz.check(oz.load().oz_selfplay_records(eng._h, ring.ctypes.data_as(C.c_void_p), rec.size, C.byref(total)))
    first = next(i for i in range(5, rec.size) if ring["ply"][i] >= 2 and ring["game_id"][i + 1] == ring["game_id"][i])
    before = np.zeros(rec.size, np.float32)
    oz.check(oz.load().oz_selfplay_targets(eng._h, oz.p_f32(before), rec.size, C.byref(total)))
    stats = eng.value_targets(("td", 0.2), first_record=first)
    after = np.zeros(rec.size, np.float32)
    oz.check(oz.load().oz_selfplay_targets(eng._h, oz.p_f32(after), rec.size, C.byref(total)))
    vals = np.zeros(rec.size, np.float64)
    oz.check(oz.load().oz_selfplay_values(eng._h, oz.p_f64(vals), rec.size, C.byref(total)))
    assert stats["records"] == rec.size - first and _same_bits(after[:first], before[:first])
    assert _same_bits(after[first:], agents.rules_value_targets(ring, vals, n, ("td", 0.2))[first:])
    assert eng.value_targets(("td", 0.2), first_record=rec.size + 5)["records"] == 0
    for bad in ((3, 0.5, 0), (2, 1.5, 0), (2, 0.5, 13), (2, 0.5, -1)):
        assert oz.load().oz_selfplay_value_targets(eng._h, 0, bad[0], bad[1], bad[2], None) == oz.OZ_ERR_ARG
    assert oz.load().oz_selfplay_value_targets(eng._h, -1, 2, 0.5, 0, None) == oz.OZ_ERR_ARG


def test_targets_after_the_endgame_solver(oz):
    n, E = 6, 6
    eng = _engine(n, 7, G, 12, 1.0, 0, record_values=True)
    eng.play_to_end()
    before = eng.records()
    solved = eng.solve_records(E)
    assert solved["solved"] > 0 and solved["z_changed"] > 0
    rec, _ = _check_targets(oz, eng, n, E)
    assert (rec["z"] != before["z"]).sum() == solved["z_changed"]
    exact = np.array([ref._empties(r, n) <= E for r in rec])
    eng.value_targets(("td", 0.7), exact_empties=E)
    tgt = eng.records(with_targets=True)[1]
    assert _same_bits(tgt[exact], rec["z"][exact].astype(np.float32))


def test_targets_under_a_playout_cap(oz):
    n = 6
    eng = _engine(n, 0, G, 20, 1.0, 1, record_values=True, playout_cap=(10, 0.5))
    eng.play_to_end()
    rec, _ = _check_targets(oz, eng, n, 0)
    fast = oz.record_fast(rec)
    assert 0 < fast.sum() < rec.size


# ------------------------------------------------------------------ 6. the replay buffer
def test_replay_buffer_takes_the_targets(oz):
    from othellozero_amd import agents
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.training import expand_examples
    from othellozero_amd.loop import examples_from_records
    n, vt = 6, ("td", 0.7)
    eng = _engine(n, 0, G, 20, 1.0, 1, record_values=True, record_visits=True, playout_cap=(10, 0.5))
    eng.play_to_end()
    rec, cnt, val = eng.records(with_visits=True, with_values=True)
    keep = oz.record_fast(rec) == 0
    assert 0 < keep.sum() < rec.size
    want = agents.rules_value_targets(rec, val, n, vt)
    for target in ("onehot", "visits"):
        today = ReplayBuffer(n, 8 * rec.size)
        assert today.append_engine(eng, policy_target=target) == keep.sum()
        dev = ReplayBuffer(n, 8 * rec.size)
        assert dev.append_engine(eng, policy_target=target, value_target=vt) == keep.sum()
        own, opp, pi, z = dev.read()
        assert _same_bits(z, np.repeat(want[keep], 8))
        assert all(a.tobytes() == b.tobytes() for a, b in zip((own, opp, pi), today.read()[:3]))
        host = ReplayBuffer(n, 8 * rec.size)
        order = np.random.default_rng(1).permutation(rec.size)
        assert host.append_records(rec[order], visits=cnt[order], policy_target=target, values=want[order]) == keep.sum()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host.read(), (own, opp, pi, z)))
        outcome = ReplayBuffer(n, 8 * rec.size)
        outcome.append_engine(eng, policy_target=target, value_target="outcome")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outcome.read(), today.read()))
    assert _same_bits(eng.records(with_targets=True)[1], want)         # what the append computed stays readable
    # the host consumers: 8 float32 targets per fully searched record
    b, p, z8 = expand_examples(rec, n, visits=cnt, values=want)
    assert z8.dtype == np.float32 and _same_bits(z8, np.repeat(want[keep], 8)) and b.shape[0] == 8 * keep.sum()
    assert expand_examples(rec, n)[2].dtype == np.int8
    ex = examples_from_records(rec, n, alias_final=False, values=want)
    assert [e[2] for e in ex] == [float(t) for t in np.repeat(want[keep], 8)] and all(isinstance(e[2], float) for e in ex)
    with pytest.raises(ValueError, match="alias_final"):
        dev.append_engine(eng, alias_final=True, value_target=vt)
    plain = _engine(n, 0, 4, 8, 1.0, 1)
    plain.play_to_end()
    with pytest.raises(oz.OzError):
        dev.append_engine(plain, value_target=vt)


def test_selfplay_batch_returns_the_targets(oz):
    from othellozero_amd import agents
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import selfplay_batch
    n = 6
    net = StubNetWrapper((n, n), SALT, 0, max_batch=8)
    plain = selfplay_batch(net, n, 8, 10, C_PUCT, 1.0, EG, seed=5)
    rec, tgt = selfplay_batch(net, n, 8, 10, C_PUCT, 1.0, EG, seed=5, value_target=("blend", 0.5))
    assert rec.tobytes() == plain.tobytes() and tgt.dtype == np.float32 and selfplay_batch.value_target_stats["records"] == rec.size
    rec6, cnt6, tgt6 = selfplay_batch(net, n, 8, 10, C_PUCT, 1.0, EG, seed=5, value_target=("td", 0.7), endgame_targets=6, record_visits=True)
    exact = np.array([ref._empties(r, n) <= 6 for r in rec6])
    assert selfplay_batch.value_target_stats["exact"] == exact.sum() > 0 and _same_bits(tgt6[exact], rec6["z"][exact].astype(np.float32))
    b, p, z = selfplay_batch(net, n, 8, 10, C_PUCT, 1.0, EG, seed=5, value_target=("blend", 0.5), expand=True)
    assert _same_bits(z, np.repeat(tgt, 8))


def test_pooled_rows_carry_the_targets(oz):
    """the torch path of the exchange step on one rank: record || [counts ||] target rows, device to device, split after the sort"""
    import torch
    from othellozero_amd.distributed import pooled_selfplay_records
    eng, rec, cnt, _ = _played(6, 30, 0, 7)
    eng.value_targets(("td", 0.7))
    want = eng.records(with_targets=True)[1]
    dev = torch.device("cuda", 0)
    r, c, t = pooled_selfplay_records(eng, dev, with_visits=True, with_values=True)
    assert r.tobytes() == rec.tobytes() and np.array_equal(c, cnt) and _same_bits(t, want)
    r, t = pooled_selfplay_records(eng, dev, with_values=True)
    assert r.tobytes() == rec.tobytes() and _same_bits(t, want)
    assert pooled_selfplay_records(eng, dev).tobytes() == rec.tobytes()


# ------------------------------------------------------------------ 7. the drop-in search and execute_episode
def test_drop_in_root_value_equals_the_engine(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.Othello import BoardView, OthelloGame, OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    n, sims = 6, 16
    eng = _engine(n, 0, 1, sims, 1.0, 1, record_values=True)
    eng.play_to_end()
    rec, val = eng.records(with_values=True)
    net = StubNetWrapper((n, n), SALT, 0, max_batch=1)
    m = OthelloMCTS(n, net, C_PUCT, q_mode=1, node_cap=sims * (n * n - 3) + 64)
    game = OthelloGame(n)
    with pytest.raises(KeyError):
        m.root_value(game.board(BoardView.TWO_CHANNELS))
    for i in range(rec.size):
        state = game.board(BoardView.TWO_CHANNELS)
        assert oz.pack_board(state) == (int(rec["black"][i]), int(rec["white"][i]))
        m.simulate_n(state, game.current_player, sims)
        if game.current_player == OthelloPlayer.WHITE:
            state = OthelloGame.invert_board(state)
        assert np.float64(m.root_value(state)).tobytes() == val[i].tobytes(), i
        game.play(int(rec["action"][i]) >> 3, int(rec["action"][i]) & 7)
    assert game.has_finished()


def test_execute_episode_float_targets(oz, monkeypatch):
    import random
    from othellozero_amd import agents
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.othelo_mcts import OthelloMCTS
    from othellozero_amd.training import execute_episode
    n, sims, vt = 6, 10, ("blend", 0.5)
    net = StubNetWrapper((n, n), SALT, 0, max_batch=1)
    seen = []
    root_value = OthelloMCTS.root_value

    def spy(self, state):
        seen.append(root_value(self, state))
        return seen[-1]
    monkeypatch.setattr(OthelloMCTS, "root_value", spy)

    def episode(**kw):
        random.seed(3)
        np.random.seed(3)
        return execute_episode(n, net, C_PUCT, sims, 1.0, 0.9, snapshot_boards=True, **kw)
    plain = episode()
    assert seen == []                                      # the default never asks
    ex = episode(value_target=vt)
    assert len(ex) == len(plain) and len(ex) == 8 * len(seen) > 0
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(ex, plain))
    assert all(isinstance(e[2], float) for e in ex) and all(isinstance(e[2], int) for e in plain)
    # the host targets of the same game: z from the plain run, q as the search gave it (a blend does not look at the mover)
    T = len(seen)
    rec = np.zeros(T, oz.RECORD_DTYPE)
    rec["ply"], rec["player"], rec["z"] = np.arange(T), 1, [plain[8 * i][2] for i in range(T)]
    for i in range(T):
        rec["black"][i], rec["white"][i] = oz.pack_board(plain[8 * i + 7][0])          # (the identity is the last of the 8)
    want = agents.rules_value_targets(rec, seen, n, vt)
    assert [e[2] for e in ex] == [float(t) for t in np.repeat(want, 8)]
    assert _same_bits(want, ref.value_targets(rec, seen, n, vt))
    assert np.abs(seen).max() <= 1.0 and not set(np.unique(want).tolist()) <= {-1.0, 0.0, 1.0}
    with pytest.raises(ValueError, match="alias_final_boards"):
        execute_episode(n, net, C_PUCT, sims, 1.0, 0.9, value_target=vt)


# ------------------------------------------------------------------ 8. the loop
def _loop_kw(tmp_path, n):
    return dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
                evaluation_interval=2, evaluation_iterations=2, temperature_threshold=0, self_play_training=False, self_play_interval=1,
                self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
                training_buffer_size=8 * 40 * 8, seed=13)


@pytest.mark.parametrize("replay", ["device", "host"])
def test_training_with_value_targets(oz, tmp_path, monkeypatch, replay):
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    n = 6
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    given = []
    fit = net.train

    def spy(data, *a, **kw):
        given.append(data.read()[3] if replay == "device" else np.array([e[2] for e in data], np.float32))
        return fit(data, *a, **kw)
    monkeypatch.setattr(net, "train", spy)
    with pytest.raises(ValueError, match="alias_final_boards"):
        loop.training(neural_network=net, replay=replay, value_target=("td", 0.7), alias_final_boards=True, **_loop_kw(tmp_path, n))
    assert given == []
    assert loop.training(neural_network=net, replay=replay, value_target=("td", 0.7), endgame_targets=6, alias_final_boards=False,
                         **_loop_kw(tmp_path, n)) == []
    (z,) = given
    assert z.size > 0 and z.size % 8 == 0 and np.isfinite(z).all() and np.abs(z).max() <= 1.0
    assert not set(np.unique(z).tolist()) <= {-1.0, 0.0, 1.0}
    (stats,) = loop.training.endgame_history
    assert stats["solved"] > 0 and (np.abs(z) == 1.0).sum() >= 8 * stats["solved"]          # the solved records keep their exact z
