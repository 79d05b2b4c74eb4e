"""The minimax opponent on the GPU (pytest -m gpu): oz_rules_minimax against the restatement in tests/minimax_ref.py bit for bit, the arena's
minimax side replayed move for move on the host, the default that stays the random mover, the refusals, the drop-in agent, the batched evaluation
and loop.training(evaluation_opponent=...)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import minimax_ref as ref

pytestmark = pytest.mark.gpu

EVALS = {ref.DISCS: "discs", ref.WEIGHTED: "weighted"}


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


def _empties(n, black, white):
    return n * n - ref.popcount(black | white)


@functools.lru_cache(maxsize=None)
def _positions(n):
    """~48 positions over all plies of six seeded random playouts (both movers), the widest of them, the late ones (<= 4 empties: the tree ends
    above the horizon), and two hand-built ones whose only reply to either move is a pass (rows 0 and n - 1 hold B W _ from the left; the second
    with the colours swapped and WHITE to move)"""
    pool = ref.playout_positions(n, 2024, 6)
    picked = pool[::max(1, len(pool) // 38)]
    picked.append(max(pool, key=lambda p: ref.popcount(ref.legal(*p, n))))
    picked += [p for p in pool if _empties(n, p[0], p[1]) <= 4][:6]
    low = (n - 1) * 8
    picked.append((_mask((0, low)), _mask((1, low + 1)), 1))
    picked.append((_mask((1, low + 1)), _mask((0, low)), -1))
    return picked


@functools.lru_cache(maxsize=None)
def _reference(n, depth, evaluation):
    """the restatement over _positions(n), computed once: ([(values, bests)], positions whose tree holds a pass)"""
    out, passes = [], 0
    for black, white, player in _positions(n):
        stats = {}
        out.append(ref.root(black, white, player, n, depth, evaluation, stats))
        passes += stats.get("passes", 0) > 0
    return out, passes


def _device(n, positions, depth, evaluation):
    from othellozero_amd.agents import rules_minimax
    return rules_minimax([p[0] for p in positions], [p[1] for p in positions], [p[2] for p in positions], n, depth, EVALS[evaluation])


def _compare(values, bests, want, where):
    for i, (v, b) in enumerate(want):
        assert int(bests[i]) == b, (where, i, hex(int(bests[i])), hex(b))
        assert values[i].tolist() == v, (where, i)


# ------------------------------------------------------------------ 1. the batch entry
@pytest.mark.parametrize("evaluation", [ref.DISCS, ref.WEIGHTED])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [8, 6])
def test_rules_minimax_vs_restatement(oz, n, depth, evaluation):
    positions = _positions(n)
    assert 44 <= len(positions) <= 52 and {p[2] for p in positions} == {1, -1}
    assert max(ref.popcount(ref.legal(*p, n)) for p in positions) >= 10
    assert sum(_empties(n, p[0], p[1]) <= 4 for p in positions) >= 4
    want, passes = _reference(n, depth, evaluation)
    assert passes >= 2
    values, bests = _device(n, positions, depth, evaluation)
    _compare(values, bests, want, (n, depth, evaluation))
    assert all(b for _, b in want)                          # every one of these movers has a move


@pytest.mark.parametrize("evaluation", [ref.DISCS, ref.WEIGHTED])
def test_rules_minimax_full_stack_on_4x4(oz, evaluation):
    """depth 6 = OZ_MINIMAX_MAX_DEPTH: the deepest frame stack, from the first plies of two playouts (the tree also runs into the end of the game)"""
    n = 4
    positions = [p for g in range(2) for p in ref.playout_positions(n, 31 + g, 1)[:4]]
    assert len(positions) == 8 and oz.MINIMAX_MAX_DEPTH == 6
    values, bests = _device(n, positions, 6, evaluation)
    _compare(values, bests, [ref.root(b, w, p, n, 6, evaluation) for b, w, p in positions], ("4x4", evaluation))


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_rules_minimax_batch_counts(oz, count):
    n, depth = 8, 2
    base, (want, _) = _positions(n), _reference(n, depth, ref.WEIGHTED)
    positions = [base[(7 * i) % len(base)] for i in range(count)]
    values, bests = _device(n, positions, depth, ref.WEIGHTED)
    assert values.shape == (count, 64) and bests.shape == (count,)
    _compare(values, bests, [want[(7 * i) % len(base)] for i in range(count)], count)


@pytest.mark.parametrize("n", [6, 8])
def test_nothing_to_play_is_no_error(oz, n):
    """a finished board (for either mover) and a mover without a move (the other side has one): bests == 0, no value, no error; NULL outputs"""
    low = (n - 1) * 8
    positions = [(_mask((0, 1, 2)), 0, 1), (_mask((0, 1, 2)), 0, -1), (_mask((0, 1, 2, low)), _mask((low + 1,)), -1), _positions(n)[3]]
    for depth in (1, 3, 6):
        values, bests = _device(n, positions, depth, ref.WEIGHTED)
        assert bests[:3].tolist() == [0, 0, 0] and (values[:3] == ref.NONE).all() and bests[3] != 0
        assert [ref.root(b, w, p, n, min(depth, 3), ref.WEIGHTED)[1] for b, w, p in positions[:3]] == [0, 0, 0]
    b, w, p = (np.array([q[i] for q in positions], dt) for i, dt in ((0, np.uint64), (1, np.uint64), (2, np.int8)))
    lib, only = oz.load(), np.zeros(4, np.uint64)
    assert lib.oz_rules_minimax(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, 2, 1, None, oz.p_u64(only)) == 0
    assert lib.oz_rules_minimax(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, 2, 1, None, None) == 0
    assert only.tolist() == _device(n, positions, 2, ref.WEIGHTED)[1].tolist()
    for depth, evaluation in ((0, 1), (7, 1), (2, 2), (2, -1)):
        assert lib.oz_rules_minimax(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, depth, evaluation, None, oz.p_u64(only)) == oz.OZ_ERR_ARG
    p[0] = 0
    assert lib.oz_rules_minimax(oz.p_u64(b), oz.p_u64(w), oz.p_i8(p), n, 4, 2, 1, None, oz.p_u64(only)) == oz.OZ_ERR_ARG


# ------------------------------------------------------------------ 2. / 3. the arena
def _replay(res, gi, n, seed, game_id, mover_of):
    """game gi of an arena result replayed through the oracle's rules: mover_of(player) -> "random", or a function position -> bests for the minimax
    side, or None for a side whose moves are taken as played (a network); -> the positions where the minimax side moved, with the move played"""
    (black, white), player, fin = ref.initial_board(n), 1, 0
    nm, seen = int(res["n_moves"][gi]), []
    for ply in range(nm):
        assert not fin and int(res["players"][gi, ply]) == player, (gi, ply)
        action, who = int(res["actions"][gi, ply]), mover_of(player)
        assert (ref.legal(black, white, player, n) >> action) & 1, (gi, ply, action)
        if who == "random":
            assert action == ref.random_move(black, white, player, n, seed, game_id, ply), (gi, ply)
        elif who is not None:
            bests = who((black, white, player))
            if bests is not None:
                assert action == ref.arena_move(bests, seed, game_id, ply), (gi, ply, hex(bests))
            seen.append(((black, white, player), ply, action))
        black, white, player, fin = ref.play(black, white, player, n, action)
    assert fin and (int(res["final_black"][gi]), int(res["final_white"][gi])) == (black, white), gi
    pb, pw = ref.popcount(black), ref.popcount(white)
    assert int(res["winner"][gi]) == (1 if pb >= pw else -1) and int(res["points"][gi]) == max(pb, pw), gi
    assert (res["actions"][gi, nm:] == 0).all() and (res["players"][gi, nm:] == 0).all()
    return seen


@pytest.mark.parametrize("minimax_side", [-1, 1])
def test_arena_random_against_minimax_replayed(oz, minimax_side):
    """32 games on 6x6 without any network: the random mover as k_arena_random_move defines it, the minimax side (depth 2, weighted) = the kth bit
    of the restatement's bests; boards, winner, points and n_moves equal the replay"""
    from othellozero_amd.agents import arena_batch
    n, G, seed, first = 6, 32, 17, 400
    key = "white" if minimax_side == -1 else "black"
    res = arena_batch(None, None, n, G, 4, 1.0, seed=seed, first_game_id=first, opponent={key: ("minimax", 2)})
    plies = 0
    for gi in range(G):
        plies += len(_replay(res, gi, n, seed, first + gi,
                             lambda player: (lambda p: ref.root(*p, n, 2, ref.WEIGHTED)[1]) if player == minimax_side else "random"))
    assert plies > 8 * G and (res["stats_black"] == 0).all() and (res["stats_white"] == 0).all()
    wins = int((res["winner"] == minimax_side).sum())
    print(f"minimax depth 2 as {key}: {wins} of {G} games against the random mover")


@pytest.mark.parametrize("net_side", [1, -1])
def test_arena_stub_network_against_minimax(oz, net_side):
    """8 games on 8x8 per colour (16 in all), a stub network with 16 simulations against minimax depth 3 weighted: every minimax move is the kth
    bit of oz_rules_minimax's bests for the position rebuilt through the oracle's rules, and on every third of those plies of the restatement's"""
    from othellozero_amd.agents import arena_batch
    from othellozero_amd.NNet import StubNetWrapper
    n, G, seed, first = 8, 8, 23, 90
    net = StubNetWrapper((n, n), 13, 0, max_batch=G)
    res = arena_batch(net if net_side == 1 else None, None if net_side == 1 else net, n, G, 16, 1.0, seed=seed, first_game_id=first,
                      opponent=("minimax", 3, "weighted"))
    seen = []
    for gi in range(G):
        seen += [(gi,) + s for s in _replay(res, gi, n, seed, first + gi, lambda player: None if player == net_side else (lambda p: None))]
    assert len(seen) > 20 * G
    _, bests = _device(n, [s[1] for s in seen], 3, ref.WEIGHTED)
    checked = 0
    for k, (gi, position, ply, action) in enumerate(seen):
        assert bests[k] != 0 and action == ref.arena_move(int(bests[k]), seed, first + gi, ply), (gi, ply)
        if k % 3 == 0:
            assert ref.root(*position, n, 3, ref.WEIGHTED)[1] == int(bests[k]), (gi, ply)
            checked += 1
    assert 4 * checked >= len(seen)
    stats = res["stats_black"] if net_side == 1 else res["stats_white"]
    assert stats[0] > 0 and (res["stats_white"] if net_side == 1 else res["stats_black"])[0] == 0


# ------------------------------------------------------------------ 4. the default stays the random mover
def _raw_arena(oz, n, G, sims, seed, net_a, net_b, before=None, after=None):
    lib, h = oz.load(), C.c_void_p()
    oz.check(lib.oz_arena_create(C.byref(h), n, G, sims, 1.0, oz.QMODE_F64, seed, 0, net_a._h if net_a else None, net_b._h if net_b else None, 0))
    try:
        if before:
            before(lib, h)
        oz.check(lib.oz_arena_run(h))
        if after:
            after(lib, h)
        winner, points, nm = np.zeros(G, np.int8), np.zeros(G, np.int32), np.zeros(G, np.int32)
        acts, pls = np.zeros((G, 128), np.uint8), np.zeros((G, 128), np.int8)
        fb, fw = np.zeros(G, np.uint64), np.zeros(G, np.uint64)
        oz.check(lib.oz_arena_results(h, oz.p_i8(winner), oz.p_i32(points), oz.p_i32(nm), oz.p_u8(acts), oz.p_i8(pls), oz.p_u64(fb), oz.p_u64(fw)))
    finally:
        lib.oz_arena_destroy(h)
    return [winner, points, nm, acts, pls, fb, fw]


def test_set_opponent_random_is_the_default_and_the_refusals(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 8
    net = StubNetWrapper((n, n), 5, 0, max_batch=G)
    plain = _raw_arena(oz, n, G, 8, 3, net, None)

    def before(lib, h):
        assert lib.oz_arena_set_opponent(h, 1, oz.AGENT_RANDOM, 1, 0) == oz.OZ_ERR_ARG          # BLACK has a network
        assert lib.oz_arena_set_opponent(h, 1, oz.AGENT_MINIMAX, 2, 1) == oz.OZ_ERR_ARG
        assert "network" in lib.oz_last_error().decode()
        for side, kind, depth, evaluation in ((0, 1, 2, 1), (2, 1, 2, 1), (-1, 2, 2, 1), (-1, -1, 2, 1), (-1, 1, 0, 1), (-1, 1, 7, 1), (-1, 1, 2, 2)):
            assert lib.oz_arena_set_opponent(h, side, kind, depth, evaluation) == oz.OZ_ERR_ARG, (side, kind, depth, evaluation)
        assert lib.oz_arena_set_opponent(h, -1, oz.AGENT_RANDOM, 99, 99) == 0                    # depth and eval are not read for the random mover

    def after(lib, h):
        assert lib.oz_arena_set_opponent(h, -1, oz.AGENT_MINIMAX, 2, 1) == oz.OZ_ERR_STATE
        assert lib.oz_arena_set_opponent(h, -1, oz.AGENT_RANDOM, 1, 0) == oz.OZ_ERR_STATE
        assert "before the first run" in lib.oz_last_error().decode()
    explicit = _raw_arena(oz, n, G, 8, 3, net, None, before, after)
    assert all(np.array_equal(x, y) for x, y in zip(plain, explicit))

    def back_and_forth(lib, h):                                                                  # the last call before the run counts
        oz.check(lib.oz_arena_set_opponent(h, -1, oz.AGENT_MINIMAX, 2, 1))
        oz.check(lib.oz_arena_set_opponent(h, -1, oz.AGENT_RANDOM, 0, 0))
    assert all(np.array_equal(x, y) for x, y in zip(plain, _raw_arena(oz, n, G, 8, 3, net, None, back_and_forth)))
    minimax = _raw_arena(oz, n, G, 8, 3, net, None, lambda lib, h: oz.check(lib.oz_arena_set_opponent(h, -1, oz.AGENT_MINIMAX, 2, 1)))
    assert not np.array_equal(plain[3], minimax[3])


# ------------------------------------------------------------------ 5. the drop-in agent
def test_minimax_agent_plays_the_restatements_game(oz, monkeypatch):
    """one whole 6x6 game, BLACK depth 2 weighted against WHITE depth 1 on discs (the greedy agent), random.choice patched to take the first"""
    from othellozero_amd.agents import MinimaxOthelloAgent, duel_between_agents
    from othellozero_amd.Othello import BoardView, OthelloGame, OthelloPlayer
    monkeypatch.setattr(random, "choice", lambda seq: seq[0])
    n = 6
    game = OthelloGame(n, current_player=OthelloPlayer.BLACK)
    played, inner = [], game.play

    def spy(row, col):
        played.append(int(row) * 8 + int(col))
        inner(row, col)
    game.play = spy
    black_agent, white_agent = MinimaxOthelloAgent(game, 2, "weighted"), MinimaxOthelloAgent(game, depth=1, evaluation="discs")
    winner, points = duel_between_agents(game, black_agent, white_agent)
    (black, white), player, fin, want = ref.initial_board(n), 1, 0, []
    while not fin:
        bests = ref.root(black, white, player, n, 2 if player == 1 else 1, ref.WEIGHTED if player == 1 else ref.DISCS)[1]
        want.append(ref.squares(bests)[0])
        black, white, player, fin = ref.play(black, white, player, n, want[-1])
    assert played == want and len(want) >= 20
    assert oz.pack_board(game.board(BoardView.TWO_CHANNELS)) == (black, white)
    pb, pw = ref.popcount(black), ref.popcount(white)
    assert winner is (black_agent if pb >= pw else white_agent) and points == max(pb, pw)


# ------------------------------------------------------------------ 6. / 7. evaluation and the loop
def test_batched_evaluation_against_minimax(oz):
    from othellozero_amd import loop
    from othellozero_amd.agents import arena_batch
    from othellozero_amd.NNet import StubNetWrapper
    n, games, sims, seed = 6, 7, 8, 5
    net = StubNetWrapper((n, n), 9, 0, max_batch=4)
    r = loop.evaluate_against_random_batch(n, net, games, sims, 1.0, seed=seed, opponent=("minimax", 2))
    assert sorted(r) == ["black_games", "black_wins", "white_games", "white_wins", "wins"] and all(isinstance(v, int) for v in r.values())
    as_black = arena_batch(net, None, n, 4, sims, 1.0, seed=seed, opponent=("minimax", 2))
    as_white = arena_batch(None, net, n, 3, sims, 1.0, seed=seed, first_game_id=4, opponent=("minimax", 2))
    bw, ww = int((as_black["winner"] == 1).sum()), int((as_white["winner"] == -1).sum())
    assert r == dict(wins=bw + ww, black_wins=bw, white_wins=ww, black_games=bw + (3 - ww), white_games=ww + (4 - bw))
    assert r == loop.evaluate_against_opponent_batch(n, net, games, sims, 1.0, ("minimax", 2, "weighted"), seed=seed)
    plain = loop.evaluate_against_random_batch(n, net, games, sims, 1.0, seed=seed)
    assert plain == loop.evaluate_against_random_batch(n, net, games, sims, 1.0, seed=seed, opponent="random")
    assert "opponent_kernel" not in arena_batch(net, None, n, 4, sims, 1.0, seed=seed) and "opponent_kernel" in as_black


def test_training_with_a_minimax_evaluation_opponent(oz, tmp_path, monkeypatch):
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    n, seen = 6, []
    inner = loop.evaluate_against_random_batch

    def spy(*args, **kw):
        seen.append(kw.get("opponent"))
        return inner(*args, **kw)
    monkeypatch.setattr(loop, "evaluate_against_random_batch", spy)
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    historic = loop.training(board_size=n, num_iterations=1, num_episodes=6, num_simulations=6, degree_exploration=1, temperature=1,
                             neural_network=net, e_greedy=0.9, evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0,
                             self_play_training=False, self_play_interval=1, self_play_total_games=2, self_play_threshold=1,
                             checkpoint_filepath=str(tmp_path / "minimax.h5"), training_buffer_size=8 * 40, seed=12, batched_evaluation=True,
                             evaluation_opponent=("minimax", 1, "discs"))
    assert len(historic) == 1 and historic[0][0] == 6 and 0 <= historic[0][1] <= 1
    assert seen == [("minimax", 1, "discs")] * 2
