"""The exact endgame solver on the GPU (pytest -m gpu), all through the C ABI: oz_rules_solve against the restatement in tests/endgame_ref.py
(a memoised negamax without pruning over the oracle's rules) value for value, against oz_rules_minimax at depth 6 on the disc count, the batch
shapes, oz_selfplay_solve_records against a relabelling on the host, and the plumbing: the replay buffer, the drop-in agent, loop.training."""
import ctypes as C
import functools
import logging
import random

import numpy as np
import pytest

import endgame_ref as eg
import minimax_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _mask(squares):
    m = 0
    for s in squares:
        m |= 1 << s
    return m


def _solve(n, positions, max_empties=eg.MAX_EMPTIES):
    from othellozero_amd.agents import rules_solve
    return rules_solve([p[0] for p in positions], [p[1] for p in positions], [p[2] for p in positions], n, max_empties)


def _compare(got, positions, n, where):
    values, bests, value, solved = got
    for i, (b, w, p) in enumerate(positions):
        want = eg.root(b, w, p, n)
        assert int(solved[i]) == 1, (where, i)
        assert int(value[i]) == want[2], (where, i, int(value[i]), want[2])
        assert int(bests[i]) == want[1], (where, i, hex(int(bests[i])), hex(want[1]))
        assert values[i].tolist() == want[0], (where, i)


@functools.lru_cache(maxsize=None)
def _late(n, games=6, most=8, seed=2024):
    """every position with at most `most` empties of `games` seeded random playouts"""
    return tuple(p for p in ref.playout_positions(n, seed, games) if eg.empties(p[0], p[1], n) <= most)


# ------------------------------------------------------------------ 1. values, bests and value
@pytest.mark.parametrize("n", [8, 6])
def test_rules_solve_vs_restatement(oz, n):
    positions = _late(n)
    assert len(positions) >= 40 and {p[2] for p in positions} == {1, -1} and max(eg.empties(p[0], p[1], n) for p in positions) == 8
    facts = [eg.facts(*p, n) for p in positions]
    assert any(f[0] for f in facts) and any(f[1] for f in facts)                           # a pass in a tree; a game that ends before the board is full
    assert any(ref.popcount(eg.root(*p, n)[1]) >= 2 for p in positions)                     # two or more best moves
    _compare(_solve(n, positions), positions, n, n)


# ------------------------------------------------------------------ 2. deep cases
def _at(n, seed, game_count, empties):
    return [p for p in ref.playout_positions(n, seed, game_count) if eg.empties(p[0], p[1], n) == empties]


def test_ten_empties_on_6x6(oz):
    positions = _at(6, 41, 2, 10)
    assert len(positions) == 2
    _compare(_solve(6, positions), positions, 6, "6x6 at 10")


def test_ten_empties_on_8x8(oz):
    positions = _at(8, 43, 1, 10)
    assert len(positions) == 1
    _compare(_solve(8, positions), positions, 8, "8x8 at 10")


def test_whole_4x4_games(oz):
    """the opening has 12 empties = OZ_SOLVE_MAX_EMPTIES: the deepest frame stack; then every position of 8 playouts"""
    n = 4
    opening = [(*ref.initial_board(n), 1)]
    assert eg.empties(*opening[0][:2], n) == 12 == oz.SOLVE_MAX_EMPTIES
    _compare(_solve(n, opening), opening, n, "4x4 opening")
    positions = ref.playout_positions(n, 7, 8)
    assert len(positions) >= 60
    _compare(_solve(n, positions), positions, n, "4x4 playouts")


# ------------------------------------------------------------------ 3. the minimax at depth 6 on the disc count is the same function there
def test_equals_minimax_depth_six_on_discs(oz):
    from othellozero_amd.agents import rules_minimax
    n = 8
    positions = _late(n, 20, 6, 99)
    assert len(positions) >= 100
    values, bests, value, solved = _solve(n, positions, 6)
    mv, mb = rules_minimax([p[0] for p in positions], [p[1] for p in positions], [p[2] for p in positions], n, 6, "discs")
    assert solved.all() and np.array_equal(values, mv) and np.array_equal(bests, mb)
    assert all(int(value[i]) == int(values[i].max()) for i in range(len(positions)) if bests[i])


# ------------------------------------------------------------------ 4. batch shapes
@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_batch_counts(oz, count):
    n, base = 8, _late(8)
    positions = [base[(7 * i) % len(base)] for i in range(count)]
    got = _solve(n, positions)
    assert got[0].shape == (count, 64) and got[1].shape == got[2].shape == got[3].shape == (count,)
    _compare(got, positions, n, count)


def test_positions_above_the_bound_are_skipped_not_refused(oz):
    n = 8
    pool = ref.playout_positions(n, 2024, 2)
    positions = pool[::5] + list(_late(8)[:12])
    cap = 5
    values, bests, value, solved = _solve(n, positions, cap)
    small = [eg.empties(p[0], p[1], n) <= cap for p in positions]
    assert 4 <= sum(small) < len(positions) - 4 and solved.tolist() == [int(s) for s in small]
    for i, p in enumerate(positions):
        if small[i]:
            assert (values[i].tolist(), int(bests[i]), int(value[i])) == eg.root(*p, n), i
        else:
            assert (values[i] == eg.NONE).all() and bests[i] == 0 and value[i] == 0, i
    # max_empties 0: finished full boards only; the same call twice: identical outputs
    assert not _solve(n, positions, 0)[3].any()
    again = _solve(n, positions, cap)
    assert all(np.array_equal(x, y) for x, y in zip((values, bests, value, solved), again))
    deep = list(_late(8)) * 3
    assert all(np.array_equal(x, y) for x, y in zip(_solve(n, deep), _solve(n, deep)))


@pytest.mark.parametrize("n", [6, 8])
def test_nothing_to_play_is_no_error(oz, n):
    """finished boards (three empties nobody can fill, for either mover; a full board) and a mover without a move (the other side has one): bests
    0, no move value, the value of the finished board / of the position after the pass; NULL outputs; the refusals"""
    full = _mask(r * 8 + c for r in range(n) for c in range(n))
    positions = [(full & ~_mask((0, 1, 2)), 0, 1), (full & ~_mask((0, 1, 2)), 0, -1),       # all BLACK: nobody brackets anything
                 (full & ~_mask((1, 2)), _mask((1,)), -1),                                    # row 0 = B W _ : WHITE has no move, BLACK has (0, 2)
                 (full & ~1, 1, 1)]
    assert [eg.root(*p, n)[1:] for p in positions] == [(0, n * n - 3), (0, 3 - n * n), (0, -n * n), (0, n * n - 2)]
    got = _solve(n, positions)
    _compare(got, positions, n, "nothing to play")
    assert (got[0] == eg.NONE).all() and not got[1].any()
    b, w, p = (np.array([q[i] for q in positions], dt) for i, dt in ((0, np.uint64), (1, np.uint64), (2, np.int8)))
    lib, only = oz.load(), np.zeros(4, np.int32)
    assert lib.oz_rules_solve(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, 12, None, None, oz.p_i32(only), None) == 0
    assert only.tolist() == got[2].tolist()
    assert lib.oz_rules_solve(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, 12, None, None, None, None) == 0
    assert lib.oz_rules_solve(None, None, None, n, 0, 12, None, None, None, None) == 0       # count 0
    for bad in (-1, 13):
        assert lib.oz_rules_solve(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, bad, None, None, oz.p_i32(only), None) == oz.OZ_ERR_ARG
    assert lib.oz_rules_solve(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), 5, 4, 12, None, None, oz.p_i32(only), None) == oz.OZ_ERR_ARG
    p[0] = 0
    assert lib.oz_rules_solve(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, 12, None, None, oz.p_i32(only), None) == oz.OZ_ERR_ARG


# ------------------------------------------------------------------ 5. solve_records
SP = dict(n=6, games=64, sims=8, e_greedy=0.5, seed=2718, cap=8)


def _raw(eng):
    """records and visit rows in the engine's own (ring) order"""
    from othellozero_amd import _lib
    total = eng.stats()["records"]
    rec, got = np.zeros(total, dtype=_lib.RECORD_DTYPE), C.c_int64()
    _lib.check(_lib.load().oz_selfplay_records(eng._h, rec.ctypes.data_as(C.c_void_p), total, C.byref(got)))
    assert got.value == total
    cnt = np.zeros((total, 64), np.int32)
    _lib.check(_lib.load().oz_selfplay_visits(eng._h, _lib.p_i32(cnt), total, C.byref(got)))
    return rec, cnt


@pytest.fixture(scope="module")
def relabelled(oz):
    """the engine of the issue's setup played to the end, its records before and after solve_records(8), and the host's relabelling"""
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    n, G = SP["n"], SP["games"]
    eng = SelfPlayEngine(StubNetWrapper((n, n), 9, 0, max_batch=G), n, G, SP["sims"], 1.25, 1.0, SP["e_greedy"], seed=SP["seed"],
                         record_visits=True)
    eng.play_to_end()
    assert eng.stats()["games_completed"] == G
    before, visits_before = _raw(eng)
    stats = eng.solve_records(SP["cap"])
    after, visits_after = _raw(eng)
    z, want = eg.relabel(before, n, SP["cap"])
    return dict(eng=eng, before=before, after=after, visits=(visits_before, visits_after), stats=stats, z=np.array(z, np.int8), want=want)


def test_solve_records_relabels_z_and_nothing_else(oz, relabelled):
    before, after, z = relabelled["before"], relabelled["after"], relabelled["z"]
    n = SP["n"]
    assert np.array_equal(after["z"], z)
    small = np.array([eg.empties(int(r["black"]), int(r["white"]), n) <= SP["cap"] for r in before])
    changed = after["z"] != before["z"]
    assert changed.any() and (small & ~changed).any() and not (changed & ~small).any()       # at least one z changes, at least one stays
    restored = after.copy()
    restored["z"] = before["z"]
    assert restored.tobytes() == before.tobytes()                                          # every other byte of every record
    assert np.array_equal(*relabelled["visits"])


def test_solve_records_statistics(oz, relabelled):
    stats, want = relabelled["stats"], relabelled["want"]
    assert {k: stats[k] for k in want} == want
    assert 64 * 4 <= stats["solved"] <= 64 * SP["cap"] < stats["records"] == len(relabelled["before"])
    assert stats["mean_disc_loss"] == want["disc_loss_sum"] / want["solved"] and stats["disc_loss_max"] > 0 < stats["optimal_moves"]
    again = relabelled["eng"].solve_records(SP["cap"])
    assert again == dict(stats, z_changed=0)
    assert _raw(relabelled["eng"])[0].tobytes() == relabelled["after"].tobytes()
    # from a later record on; nothing to do beyond the end; the refusals
    eng, total = relabelled["eng"], len(relabelled["before"])
    part = eng.solve_records(SP["cap"], first_record=total - 10)
    assert part["records"] == 10 and part["z_changed"] == 0
    assert eng.solve_records(SP["cap"], first_record=total + 5)["records"] == 0
    lib = oz.load()
    for bad in (0, 13, -1):
        assert lib.oz_selfplay_solve_records(eng._h, 0, bad, None) == oz.OZ_ERR_ARG
    assert lib.oz_selfplay_solve_records(eng._h, -1, 8, None) == oz.OZ_ERR_ARG
    assert lib.oz_selfplay_solve_records(eng._h, 0, 1, None) == 0


# ------------------------------------------------------------------ 6. plumbing
def test_replay_buffer_holds_the_relabelled_z(oz, relabelled):
    from othellozero_amd.replay import ReplayBuffer
    eng, after = relabelled["eng"], relabelled["after"]
    buf = ReplayBuffer(SP["n"], 8 * len(after))
    assert buf.append_engine(eng) == len(after)
    order = np.lexsort((after["ply"], after["game_id"]))
    z = buf.read()[3].reshape(-1, 8)
    assert (z == z[:, :1]).all() and np.array_equal(z[:, 0], after["z"][order].astype(np.float32))
    assert not np.array_equal(z[:, 0], relabelled["before"]["z"][order].astype(np.float32))


def test_agent_plays_perfectly_below_its_bound(oz, monkeypatch):
    """one whole 6x6 game of MinimaxOthelloAgent(solve_empties=8) against itself: from 8 empties on every move is one of the restatement's best
    (the first, random.choice patched); above, the depth-1 agent's"""
    from othellozero_amd.agents import MinimaxOthelloAgent, duel_between_agents
    from othellozero_amd.Othello import OthelloGame, OthelloPlayer
    monkeypatch.setattr(random, "choice", lambda seq: seq[0])
    n = 6
    game = OthelloGame(n, current_player=OthelloPlayer.BLACK)
    played, inner = [], game.play

    def spy(row, col):
        played.append(int(row) * 8 + int(col))
        inner(row, col)
    game.play = spy
    duel_between_agents(game, MinimaxOthelloAgent(game, 1, "discs", solve_empties=8), MinimaxOthelloAgent(game, 1, "discs", solve_empties=8))
    (black, white), player, fin, exact = ref.initial_board(n), 1, 0, 0
    for sq in played:
        assert not fin
        if eg.empties(black, white, n) <= 8:
            assert sq == ref.squares(eg.root(black, white, player, n)[1])[0]
            exact += 1
        else:
            assert sq == ref.squares(ref.root(black, white, player, n, 1, ref.DISCS)[1])[0]
        black, white, player, fin = ref.play(black, white, player, n, sq)
    assert fin and exact >= 6 and len(played) > exact


def _loop_kw(tmp_path, n):
    return dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
                evaluation_interval=2, evaluation_iterations=2, temperature_threshold=0, self_play_training=False, self_play_interval=1,
                self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
                training_buffer_size=8 * 40 * 8, seed=13, alias_final_boards=False)


@pytest.mark.parametrize("replay", ["host", "device"])
def test_training_with_endgame_targets(oz, tmp_path, monkeypatch, caplog, replay):
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    n = 6
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    with caplog.at_level(logging.INFO):
        assert loop.training(neural_network=net, replay=replay, endgame_targets=6, **_loop_kw(tmp_path, n)) == []
    (stats,) = loop.training.endgame_history
    assert 0 < stats["solved"] <= 8 * 6 and stats["records"] > stats["solved"] and stats["mean_disc_loss"] >= 0
    line = [r.getMessage() for r in caplog.records if "endgame targets" in r.getMessage()]
    assert len(line) == 1 and f"solved {stats['solved']} / z_changed {stats['z_changed']} / mean_disc_loss" in line[0]


def test_endgame_targets_off_changes_no_record(oz):
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import selfplay_batch
    n, G = 6, 8
    net = StubNetWrapper((n, n), 9, 0, max_batch=G)
    plain = selfplay_batch(net, n, G, 8, 1.25, 1.0, 0.5, seed=5)
    off = selfplay_batch(net, n, G, 8, 1.25, 1.0, 0.5, seed=5, endgame_targets=0)
    on = selfplay_batch(net, n, G, 8, 1.25, 1.0, 0.5, seed=5, endgame_targets=8)
    assert plain.tobytes() == off.tobytes() and selfplay_batch.endgame_stats["solved"] > 0
    z, want = eg.relabel(plain, n, 8)
    assert np.array_equal(on["z"], np.array(z, np.int8)) and {k: selfplay_batch.endgame_stats[k] for k in want} == want
    restored = on.copy()
    restored["z"] = plain["z"]
    assert restored.tobytes() == plain.tobytes()
