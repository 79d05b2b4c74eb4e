"""Arena openings on the GPU (pytest -m gpu): oz_rules_random_openings against the restatement in tests/openings_ref.py, arenas that start from
openings replayed move for move on the host (random mover, minimax, oracle.Mcts for the searched moves), lists handed back through
opening_moves, loop.paired_match recomputed from the final boards, openings off, the refusals, and the sharding rule.  Integers and bitboards
only: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import minimax_ref as mref
import openings_ref as ref
import oracle

pytestmark = pytest.mark.gpu

ARRAYS = ("winner", "points", "n_moves", "actions", "players", "final_black", "final_white", "opening_plies")


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@functools.lru_cache(maxsize=None)
def _reference(n, plies, seed, first, count):
    return ref.openings(n, plies, seed, first, count)


def _lists(want):
    """the restatement's openings as the (moves, n_plies) arrays opening_moves takes"""
    moves, n_plies = np.zeros((len(want), 16), np.uint8), np.zeros(len(want), np.int32)
    for k, o in enumerate(want):
        moves[k, :o["n_plies"]] = o["actions"]
        n_plies[k] = o["n_plies"]
    return moves, n_plies


# ------------------------------------------------------------------ 1. the batch entry
@pytest.mark.parametrize("first", [0, 2 ** 40 + 3])
@pytest.mark.parametrize("n, plies", [(4, 8), (6, 12), (8, 16), (8, 1)])
def test_rules_random_openings_vs_restatement(oz, n, plies, first):
    from othellozero_amd.agents import rules_random_openings
    count, seed = 256, 7
    got, want = rules_random_openings(n, count, plies, seed, first), _reference(n, plies, seed, first, count)
    assert {k: v.shape for k, v in got.items()} == dict(black=(count,), white=(count,), player=(count,), finished=(count,), actions=(count, 16),
                                                        n_plies=(count,))
    for k, o in enumerate(want):
        assert (int(got["black"][k]), int(got["white"][k]), int(got["player"][k]), int(got["finished"][k]), int(got["n_plies"][k])) == \
            (o["black"], o["white"], o["player"], o["finished"], o["n_plies"]), (n, plies, first, k)
        assert got["actions"][k].tolist() == o["actions"] + [0] * (16 - o["n_plies"]), (n, plies, first, k)
    if (n, plies, first) == (4, 8, 0):
        assert sum(o["passes"] > 0 for o in want) >= 1 and sum(o["finished"] for o in want) >= 1
    # NULL outputs, an empty batch and the refusals
    lib, only = oz.load(), np.zeros(count, np.int32)
    assert lib.oz_rules_random_openings(n, count, plies, seed, first, None, None, None, None, None, oz.p_i32(only)) == 0
    assert only.tolist() == got["n_plies"].tolist()
    assert lib.oz_rules_random_openings(n, 0, plies, seed, first, None, None, None, None, None, None) == 0
    for bad_n, bad_count, bad_plies in ((n, count, 17), (n, count, -1), (n, -1, plies), (n, 2 ** 22 + 1, plies), (5, count, plies)):
        assert lib.oz_rules_random_openings(bad_n, bad_count, bad_plies, seed, first, None, None, None, None, None, None) == oz.OZ_ERR_ARG


# ------------------------------------------------------------------ replay of an arena game that began with an opening
def _replay(res, gi, n, seed, game_id, opening, mover_of):
    """game gi of an arena result through the oracle's rules: its first opening_plies moves are `opening`'s (the restatement's), every later move
    is mover_of(player)'s: "random" (k_arena_random_move, keyed (seed, game id, true ply)), a function position -> bests for the minimax side, or
    None for moves taken as played; -> [(position, ply, action)] of the moves taken as played"""
    (black, white), player, fin = mref.initial_board(n), 1, 0
    nm, k, seen = int(res["n_moves"][gi]), int(res["opening_plies"][gi]), []
    assert k == opening["n_plies"] <= nm, gi
    assert res["actions"][gi, :k].tolist() == opening["actions"] and res["players"][gi, :k].tolist() == opening["players"], gi
    for ply in range(nm):
        assert not fin and int(res["players"][gi, ply]) == player, (gi, ply)
        action = int(res["actions"][gi, ply])
        assert (mref.legal(black, white, player, n) >> action) & 1, (gi, ply, action)
        if ply >= k:
            who = mover_of(player)
            if who == "random":
                assert action == mref.random_move(black, white, player, n, seed, game_id, ply), (gi, ply)
            elif who is not None:
                assert action == mref.arena_move(who((black, white, player)), seed, game_id, ply), (gi, ply)
            else:
                seen.append(((black, white, player), ply, action))
        black, white, player, fin = mref.play(black, white, player, n, action)
        if ply == k - 1:
            assert (black, white, player, fin) == (opening["black"], opening["white"], opening["player"], opening["finished"]), gi
    assert fin and (int(res["final_black"][gi]), int(res["final_white"][gi])) == (black, white), gi
    pb, pw = mref.popcount(black), mref.popcount(white)
    assert int(res["winner"][gi]) == (1 if pb >= pw else -1) and int(res["points"][gi]) == max(pb, pw), gi
    assert (res["actions"][gi, nm:] == 0).all() and (res["players"][gi, nm:] == 0).all()
    return seen


# ------------------------------------------------------------------ 2. without networks: the random mover against minimax
@pytest.mark.parametrize("minimax_side", [-1, 1])
def test_arena_random_against_minimax_from_openings(oz, minimax_side):
    from othellozero_amd.agents import arena_batch
    n, G, seed, first, plies, oseed, ofirst = 6, 32, 17, 400, 6, 5, 9
    key = "white" if minimax_side == -1 else "black"
    res = arena_batch(None, None, n, G, 4, 1.0, seed=seed, first_game_id=first, opponent={key: ("minimax", 2)}, openings=(plies, oseed),
                      first_opening_id=ofirst)
    want = _reference(n, plies, oseed, ofirst, G)
    assert res["opening_plies"].dtype == np.int32 and res["opening_plies"].tolist() == [o["n_plies"] for o in want] == [plies] * G
    for gi in range(G):
        _replay(res, gi, n, seed, first + gi, want[gi],
                lambda player: (lambda p: mref.root(*p, n, 2, mref.WEIGHTED)[1]) if player == minimax_side else "random")
    assert len({tuple(a[:plies]) for a in res["actions"].tolist()}) > G // 2             # the games do start differently
    assert (res["stats_black"] == 0).all() and (res["stats_white"] == 0).all()
    # the openings do not depend on the games' seed and ids
    other = arena_batch(None, None, n, G, 4, 1.0, seed=seed + 1, first_game_id=0, max_rounds=1, openings=(plies, oseed), first_opening_id=ofirst)
    assert np.array_equal(other["actions"][:, :plies], res["actions"][:, :plies])


# ------------------------------------------------------------------ 3. games that end inside their opening
def test_4x4_games_that_end_inside_the_opening(oz):
    from othellozero_amd.agents import arena_batch
    n, G, seed, first, plies, oseed = 4, 256, 3, 50, 8, 7
    want = _reference(n, plies, oseed, 0, G)
    early = [k for k, o in enumerate(want) if o["finished"] and o["n_plies"] < plies]
    assert len(early) >= 1 and sum(o["passes"] > 0 for o in want) >= 1
    res = arena_batch(None, None, n, G, 4, 1.0, seed=seed, first_game_id=first, openings=(plies, oseed))
    for gi in range(G):
        _replay(res, gi, n, seed, first + gi, want[gi], lambda player: "random")
    for k in early:
        assert int(res["n_moves"][k]) == int(res["opening_plies"][k]) == want[k]["n_plies"] < plies
    assert all(int(res["n_moves"][k]) > want[k]["n_plies"] for k in range(G) if not want[k]["finished"])


# ------------------------------------------------------------------ 4. the searches start where the opening ends
def _stub_arena(n, G, sims, seed, first, sa=41, sb=42, **kw):
    from othellozero_amd.agents import arena_batch
    from othellozero_amd.NNet import StubNetWrapper
    return arena_batch(StubNetWrapper((n, n), sa, 0, max_batch=G), StubNetWrapper((n, n), sb, 0, max_batch=G), n, G, sims, 1.0, seed=seed,
                       first_game_id=first, **kw)


def test_searches_start_where_the_opening_ends(oz):
    n, G, sims, seed, first, plies, oseed = 6, 8, 8, 11, 30, 6, 3
    res = _stub_arena(n, G, sims, seed, first, openings=(plies, oseed))
    want = _reference(n, plies, oseed, 0, G)
    for gi in (0, 5):
        seen = _replay(res, gi, n, seed, first + gi, want[gi], lambda player: None)
        assert len(seen) == int(res["n_moves"][gi]) - plies > 10
        trees = {1: oracle.Mcts(n, 1.0, 1, salt=41), -1: oracle.Mcts(n, 1.0, 1, salt=42)}       # empty at the first searched move, kept from then on
        for (black, white, player), ply, action in seen:
            for _ in range(sims):
                trees[player].simulate(black, white, player)
            own, opp = (black, white) if player == 1 else (white, black)
            rc, cnt, legal = trees[player].counts(own, opp)
            assert rc == 0 and legal == mref.legal(black, white, player, n)
            top = max(int(cnt[s]) for s in mref.squares(legal))
            bests = sum(1 << s for s in mref.squares(legal) if int(cnt[s]) == top)
            assert action == mref.arena_move(bests, seed, first + gi, ply), (gi, ply)
    # the same openings handed back as lists: identical arrays
    again = _stub_arena(n, G, sims, seed, first, opening_moves=_lists(want))
    for name in ARRAYS + ("stats_black", "stats_white"):
        assert np.array_equal(res[name], again[name]), name
    plain = _stub_arena(n, G, sims, seed, first)
    assert "opening_plies" not in plain and not np.array_equal(plain["actions"], res["actions"])


# ------------------------------------------------------------------ 5. pairing
def test_paired_match_and_self_play_match(oz):
    from othellozero_amd import loop
    from othellozero_amd.NNet import StubNetWrapper
    n, pairs, sims, seed, openings = 6, 8, 8, 4, (6, 3)
    new, old = StubNetWrapper((n, n), 61, 0, max_batch=pairs), StubNetWrapper((n, n), 62, 0, max_batch=pairs)
    s = loop.paired_match(n, new, old, pairs, sims, 1.0, openings, seed=seed)
    a, b = s["games"]
    want = _reference(n, 6, 3, 0, pairs)
    for i in range(pairs):                                  # game i of both arenas starts with opening i; the colours are swapped
        for r in (a, b):
            assert r["actions"][i, :6].tolist() == want[i]["actions"] and int(r["opening_plies"][i]) == 6
    assert s["opening_plies"].tolist() == [6] * pairs
    assert np.array_equal(a["winner"], _stub_arena(n, pairs, sims, seed, 0, 61, 62, openings=openings)["winner"])            # new is BLACK
    assert np.array_equal(b["final_black"], _stub_arena(n, pairs, sims, seed, pairs, 62, 61, openings=openings)["final_black"])   # old is BLACK
    pop = lambda xs: np.array([mref.popcount(x) for x in xs], np.int64)          # noqa: E731
    ab, aw, bb, bw = pop(a["final_black"]), pop(a["final_white"]), pop(b["final_black"]), pop(b["final_white"])
    margin = np.stack([ab - aw, bw - bb], axis=1)
    assert s["margin"].tolist() == margin.tolist() and s["pair_margin"].tolist() == margin.sum(axis=1).tolist()
    assert s["wins"] == int((a["winner"] == 1).sum() + (b["winner"] == -1).sum()) == int((ab >= aw).sum() + (bw > bb).sum())
    assert (s["wins_true"], s["draws"], s["losses"]) == (int((margin > 0).sum()), int((margin == 0).sum()), int((margin < 0).sum()))
    assert s["split_pairs"] == sum(1 for x, y in margin.tolist() if x * y < 0)
    assert s["mean_margin"] == float(margin.sum(axis=1).mean()) and s["pairs"] == pairs
    assert loop.self_play_match(n, new, old, 2 * pairs, sims, 1.0, seed=seed, openings=openings) == s["wins"]
    assert loop.self_play_match.stats["margin"].tolist() == margin.tolist() and "games" not in loop.self_play_match.stats
    loop.self_play_match(n, new, old, 2, sims, 1.0, seed=seed)
    assert loop.self_play_match.stats is None


def test_batched_evaluation_with_openings(oz):
    from othellozero_amd import loop
    from othellozero_amd.agents import arena_batch
    from othellozero_amd.NNet import StubNetWrapper
    n, games, sims, seed, openings = 6, 7, 8, 5, (4, 2)
    net = StubNetWrapper((n, n), 9, 0, max_batch=4)
    r = loop.evaluate_against_opponent_batch(n, net, games, sims, 1.0, ("minimax", 1, "discs"), seed=seed, openings=openings)
    as_black = arena_batch(net, None, n, 4, sims, 1.0, seed=seed, opponent=("minimax", 1, "discs"), openings=openings)
    as_white = arena_batch(None, net, n, 3, sims, 1.0, seed=seed, first_game_id=4, opponent=("minimax", 1, "discs"), openings=openings)
    assert np.array_equal(as_black["actions"][:3, :4], as_white["actions"][:, :4])        # both halves meet the same openings
    bw, ww = int((as_black["winner"] == 1).sum()), int((as_white["winner"] == -1).sum())
    assert r == dict(wins=bw + ww, black_wins=bw, white_wins=ww, black_games=bw + (3 - ww), white_games=ww + (4 - bw))


# ------------------------------------------------------------------ 6. off is off, and the refusals
def _raw_arena(oz, n, G, sims, seed, net_a, net_b, before=None, after=None):
    lib, h = oz.load(), C.c_void_p()
    oz.check(lib.oz_arena_create(C.byref(h), n, G, sims, 1.0, oz.QMODE_F64, seed, 0, net_a._h if net_a else None, net_b._h if net_b else None, 0))
    try:
        if before:
            before(lib, h)
        oz.check(lib.oz_arena_run(h))
        if after:
            after(lib, h)
        winner, points, nm, op = np.zeros(G, np.int8), np.zeros(G, np.int32), np.zeros(G, np.int32), np.full(G, -1, np.int32)
        acts, pls = np.zeros((G, 128), np.uint8), np.zeros((G, 128), np.int8)
        fb, fw = np.zeros(G, np.uint64), np.zeros(G, np.uint64)
        oz.check(lib.oz_arena_results(h, oz.p_i8(winner), oz.p_i32(points), oz.p_i32(nm), oz.p_u8(acts), oz.p_i8(pls), oz.p_u64(fb), oz.p_u64(fw)))
        oz.check(lib.oz_arena_opening_plies(h, oz.p_i32(op)))
    finally:
        lib.oz_arena_destroy(h)
    return [winner, points, nm, acts, pls, fb, fw, op]


def test_openings_off_is_the_untouched_arena_and_the_refusals(oz):
    from othellozero_amd.NNet import StubNetWrapper
    n, G = 6, 8
    net = StubNetWrapper((n, n), 5, 0, max_batch=G)
    plain = _raw_arena(oz, n, G, 8, 3, net, None)
    assert plain[7].tolist() == [0] * G
    moves, n_plies = _lists(_reference(n, 6, 3, 0, G))
    zeros = np.zeros(G, np.int32)

    def refused(lib, rc, *words):
        assert rc == oz.OZ_ERR_ARG, rc
        msg = lib.oz_last_error().decode()
        assert all(w in msg for w in words), msg

    def before(lib, h):
        for plies in (17, -1):
            refused(lib, lib.oz_arena_set_openings(h, plies, 1, 0), "plies")
        bad = moves.copy()
        bad[3, 2] = bad[3, 1]                                            # an occupied square
        refused(lib, lib.oz_arena_set_opening_moves(h, oz.p_u8(bad), oz.p_i32(n_plies)), "game 3", "ply 2")
        bad[3, 2] = 7                                                    # off the 6x6 board
        refused(lib, lib.oz_arena_set_opening_moves(h, oz.p_u8(bad), oz.p_i32(n_plies)), "game 3", "ply 2")
        long = n_plies.copy()
        long[5] = 17
        refused(lib, lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(long)), "game 5", "plies")
        long[5] = -1
        refused(lib, lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(long)), "game 5", "plies")
        oz.check(lib.oz_arena_set_openings(h, 0, 99, 99))                # plies 0: off

    def after(lib, h):
        assert lib.oz_arena_set_openings(h, 4, 1, 0) == oz.OZ_ERR_STATE
        assert "before the first run" in lib.oz_last_error().decode()
        assert lib.oz_arena_set_openings(h, 0, 1, 0) == oz.OZ_ERR_STATE
        assert lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(n_plies)) == oz.OZ_ERR_STATE
        assert "before the first run" in lib.oz_last_error().decode()
    assert all(np.array_equal(x, y) for x, y in zip(plain, _raw_arena(oz, n, G, 8, 3, net, None, before, after)))
    # lists of no plies at all; and the later setter wins
    empty = _raw_arena(oz, n, G, 8, 3, net, None, lambda lib, h: oz.check(lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(zeros))))
    assert all(np.array_equal(x, y) for x, y in zip(plain, empty))

    def armed_then_off(lib, h):
        oz.check(lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(n_plies)))
        oz.check(lib.oz_arena_set_openings(h, 6, 3, 0))
        oz.check(lib.oz_arena_set_openings(h, 0, 0, 0))
    assert all(np.array_equal(x, y) for x, y in zip(plain, _raw_arena(oz, n, G, 8, 3, net, None, armed_then_off)))

    def random_then_lists(lib, h):
        oz.check(lib.oz_arena_set_openings(h, 2, 77, 5))
        oz.check(lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(n_plies)))
    by_lists = _raw_arena(oz, n, G, 8, 3, net, None, random_then_lists)
    by_seed = _raw_arena(oz, n, G, 8, 3, net, None, lambda lib, h: oz.check(lib.oz_arena_set_openings(h, 6, 3, 0)))
    assert all(np.array_equal(x, y) for x, y in zip(by_lists, by_seed)) and by_seed[7].tolist() == [6] * G
    assert not np.array_equal(by_seed[3], plain[3])


def test_a_listed_move_after_the_end_of_the_game_is_refused(oz):
    n, plies, oseed = 4, 8, 7
    want = _reference(n, plies, oseed, 0, 256)
    k = next(i for i, o in enumerate(want) if o["finished"] and o["n_plies"] < plies)
    picked = [want[0], want[k], want[1]]
    moves, n_plies = _lists(picked)

    def before(lib, h):
        longer = n_plies.copy()
        longer[1] += 1
        assert lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(longer)) == oz.OZ_ERR_ARG
        msg = lib.oz_last_error().decode()
        assert "game 1" in msg and f"ply {want[k]['n_plies']}" in msg and "ended" in msg, msg
        oz.check(lib.oz_arena_set_opening_moves(h, oz.p_u8(moves), oz.p_i32(n_plies)))
    out = _raw_arena(oz, n, 3, 4, 2, None, None, before)
    assert out[7].tolist() == n_plies.tolist() and int(out[2][1]) == want[k]["n_plies"]
    assert (int(out[5][1]), int(out[6][1])) == (want[k]["black"], want[k]["white"])


# ------------------------------------------------------------------ 7. what arena_sharded does with a shard
def test_two_shards_equal_the_whole_arena(oz):
    n, G, sims, seed, openings, ofirst = 6, 16, 8, 21, (5, 13), 100
    whole = _stub_arena(n, G, sims, seed, 0, openings=openings, first_opening_id=ofirst)
    lo = _stub_arena(n, 8, sims, seed, 0, openings=openings, first_opening_id=ofirst)
    hi = _stub_arena(n, 8, sims, seed, 8, openings=openings, first_opening_id=ofirst + 8)
    for name in ARRAYS:
        assert np.array_equal(np.concatenate([lo[name], hi[name]]), whole[name]), name


def test_arena_sharded_passes_the_openings_on(oz):
    """one process = one shard holding every game (first game index 0): the pooled result is the arena's.  (Run alone, most of this test's time is
    the import of torch behind othellozero_amd.distributed.)"""
    from othellozero_amd.distributed import arena_sharded
    from othellozero_amd.NNet import StubNetWrapper
    n, G, sims, seed, openings, ofirst = 6, 16, 8, 21, (5, 13), 100
    whole = _stub_arena(n, G, sims, seed, 0, openings=openings, first_opening_id=ofirst)
    pooled = arena_sharded(StubNetWrapper((n, n), 41, 0, max_batch=G), StubNetWrapper((n, n), 42, 0, max_batch=G), n, G, sims, 1.0, seed=seed,
                           openings=openings, first_opening_id=ofirst)
    assert all(np.array_equal(pooled[name], whole[name]) for name in ("winner", "points", "n_moves"))
    with pytest.raises(ValueError):
        arena_sharded(None, None, n, G, sims, 1.0, seed=seed, openings=(17, 1))
