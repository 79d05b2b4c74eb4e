"""Proof play without a GPU: the library's host function of the rule (oz_search_proof_play through agents.rules_proof_play) against the
restatement tests/proof_play_ref.py on every root of the proofs' case set and on a hand table; what the case set and the 8-game engine
setting cover; the proof-targets pass and the value targets with exact_proven against the restatement, bit for bit, and the old entry points
against the new ones with the flag 0; and the Python surface's refusals before the library is touched."""
import functools

import numpy as np
import pytest

import proof_play_ref as PP
import solve_leaves_ref as SL
from proofs_ref import DRAW_POSITION, ProvenSearch
from value_signs_ref import POSITIONS_6
from wide_search_ref import initial_board, legal_mask

SALT6 = 7
# the case set of tests/test_gpu_proofs.py: (n, own, opp, simulations, stub salt)
CASES = [(4, *initial_board(4), sims, salt) for sims in (100, 200) for salt in (3, 11)] + [(6, own, opp, 60, SALT6) for own, opp in POSITIONS_6]
DRAW_CASE = (6, *DRAW_POSITION, 120, SALT6)
ENGINE = dict(n=6, games=8, sims=12, salt=21, seed=77, first=300, e_greedy=0.8)


@functools.lru_cache(maxsize=None)
def proven(n, own, opp, sims, salt, K, solve=0):
    """the restatement's search of one case, computed once and shared (read only)"""
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    s = ProvenSearch(n, 1.0, K, salt=salt, evaluator=ev, solve=solve)
    s.simulate(own, opp, sims)
    return s


@functools.lru_cache(maxsize=None)
def engine_games(K, solve=0):
    """the 8 games of the engine setting under the rule -> (list of episodes, the four counters)"""
    e = ENGINE
    stats, games = {}, []
    for gid in range(e["first"], e["first"] + e["games"]):
        ev = SL.evaluator(solve, SL.stub(e["salt"], 0)) if solve else None
        W = ProvenSearch(e["n"], 1.0, K, salt=e["salt"], evaluator=ev, solve=solve)
        games.append(PP.episode(W, e["n"], e["sims"], e["seed"], gid, e["e_greedy"], stats=stats))
        assert not W.corrupt
    return games, stats


def host(legal, edge, own_value, counts):
    from othellozero_amd import agents
    return agents.rules_proof_play(legal, [edge.get(s) for s in range(64)], own_value, counts)


def same(got, want, where):
    assert got["val"] == want["val"], where
    assert got["keep"] == want["keep"], where
    assert np.array_equal(got["row"], want["row"]) and got["row"].dtype == np.int32, where
    assert got["fallback"] == want["fallback"] and got["inconsistent"] == want["inconsistent"], where


def row_of(mask_counts):
    cnt = np.zeros(64, np.int32)
    for s, c in mask_counts.items():
        cnt[s] = c
    return cnt


# (legal squares, edge proofs, own value, counts) -> (val, kept squares, fallback, inconsistent)
HAND = [
    # a win root: only the winning edges stay
    ("win", [1, 2, 3], {1: -1, 2: 1}, None, {1: 9, 2: 3, 3: 5}, (1, [2], False, False)),
    ("two wins", [1, 2, 3], {1: 1, 2: 1}, None, {1: 9, 2: 3, 3: 5}, (1, [1, 2], False, False)),
    # a draw root: every edge known, the best a draw
    ("draw", [4, 9], {4: -1, 9: 0}, None, {4: 4, 9: 115}, (0, [9], False, False)),
    # a loss root keeps its whole row: every edge is a candidate
    ("loss", [4, 9, 20], {4: -1, 9: -1, 20: -1}, None, {4: 4, 9: 11, 20: 2}, (-1, [4, 9, 20], False, False)),
    # known by its own value only, no edge equal to it: the edges not proven lost
    ("own win", [1, 2, 3], {1: -1}, 1, {1: 9, 2: 3, 3: 5}, (1, [2, 3], False, False)),
    ("own draw", [1, 2], {}, 0, {1: 9, 2: 3}, (0, [1, 2], False, False)),
    ("own loss, one edge lost", [1, 2], {1: -1}, -1, {1: 9, 2: 3}, (-1, [1], False, False)),
    # unknown with a proven-loss edge: the arg-max moves off it
    ("unknown, lost edge", [7, 8, 30], {7: -1}, None, {7: 50, 8: 5, 30: 4}, (None, [8, 30], False, False)),
    ("unknown, draw edge", [7, 8, 30], {7: 0}, None, {7: 50, 8: 5, 30: 4}, (None, [7, 8, 30], False, False)),
    ("unknown, nothing proven", [7, 8], {}, None, {7: 1, 8: 1}, (None, [7, 8], False, False)),
    # every candidate unvisited: the fallback to the legal set
    ("fallback, win unvisited", [1, 2, 3], {2: 1}, None, {1: 9, 3: 5}, (1, [1, 2, 3], True, False)),
    ("fallback, open edges unvisited", [7, 8, 30], {7: -1}, None, {7: 12}, (None, [7, 8, 30], True, False)),
    # an inconsistent entry: own value +1 with every edge proven lost -- no edge equals it and none is left unlost: the legal set
    ("inconsistent", [1, 2], {1: -1, 2: -1}, 1, {1: 9, 2: 3}, (1, [1, 2], False, True)),
    # proofs off the legal set are not read
    ("off the legal set", [1, 2], {1: -1, 40: 1}, None, {1: 9, 2: 3}, (None, [2], False, False)),
    ("square 63", [62, 63], {62: -1, 63: 1}, None, {62: 7, 63: 1}, (1, [63], False, False)),
]


def test_host_function_on_the_hand_table():
    seen = set()
    for name, acts, edge, own, counts, (val, kept, fallback, bad) in HAND:
        legal = sum(1 << s for s in acts)
        cnt = row_of(counts)
        want = PP.rule(legal, edge, own, cnt)
        assert (want["val"], PP.squares_of(want["keep"]), want["fallback"], want["inconsistent"]) == (val, kept, fallback, bad), name
        assert want["row"].tolist() == [int(cnt[s]) if s in kept else 0 for s in range(64)], name
        same(host(legal, edge, own, cnt), want, name)
        seen.add((val, fallback, bad, own is not None))
    assert {v for v, _, _, _ in seen} == {1, 0, -1, None}
    assert any(f for _, f, _, _ in seen) and any(b for _, _, b, _ in seen) and any(o for _, _, _, o in seen)
    from othellozero_amd import _lib
    with pytest.raises(_lib.OzError):                       # a count off the legal set is not a root's row
        host(0b110, {}, None, row_of({5: 1}))
    with pytest.raises(_lib.OzError):
        host(0b110, {1: 2}, None, row_of({1: 1}))


def test_host_function_and_coverage_over_the_case_set():
    cover = dict(win_one_square=0, draw_root=0, loss_unchanged=0, unknown_argmax_moves=0, fallbacks=0, roots=0)
    for K in (1, 4):
        for solve in (0, 4):
            for case in CASES + [DRAW_CASE]:
                n, own, opp = case[:3]
                s = proven(*case, K, solve)
                for nd_i, nd in enumerate(s.nodes):          # every node the search holds is a root some game could stand on
                    if nd.Ns == 0:
                        continue
                    pl = PP.root_play(s, nd.own, nd.opp)
                    same(host(pl["legal"], s.edge[nd_i], s.own[nd_i], pl["raw"]), pl, (case, K, solve, nd_i))
                    cover["fallbacks"] += pl["fallback"]
                pl = PP.root_play(s, own, opp)
                raw, row = pl["raw"], pl["row"]
                lg = PP.squares_of(pl["legal"])
                cover["roots"] += 1
                print(n, case[3], case[4], "K", K, "E", solve, "val", pl["val"], [int(raw[q]) for q in lg], "->", [int(row[q]) for q in lg])
                if pl["val"] == 1 and np.count_nonzero(row) == 1 and np.count_nonzero(raw) > 1:
                    cover["win_one_square"] += 1
                if pl["val"] == 0:
                    cover["draw_root"] += 1
                if pl["val"] == -1:
                    assert np.array_equal(row, raw)
                    cover["loss_unchanged"] += 1
                if pl["val"] is None and int(np.argmax(row)) != int(np.argmax(raw)):
                    cover["unknown_argmax_moves"] += 1
    print(cover)
    assert cover["win_one_square"] >= 1 and cover["draw_root"] >= 1 and cover["loss_unchanged"] >= 1 and cover["unknown_argmax_moves"] >= 1
    # the rows the issue names, at K = 1 without solved leaves
    pl = PP.root_play(proven(6, *POSITIONS_6[2], 60, SALT6, 1), *POSITIONS_6[2])
    assert pl["val"] == 1 and [int(x) for x in pl["raw"] if x] == [1, 1, 1, 1, 6, 1, 6, 42] and [int(x) for x in pl["row"] if x] == [42]
    pl = PP.root_play(proven(*DRAW_CASE, 1), *DRAW_POSITION)
    assert pl["val"] == 0 and [int(pl["raw"][q]) for q in PP.squares_of(pl["legal"])] == [4, 115]
    assert [int(pl["row"][q]) for q in PP.squares_of(pl["legal"])] == [0, 115]
    pl = PP.root_play(proven(6, *POSITIONS_6[1], 60, SALT6, 1), *POSITIONS_6[1])
    assert pl["val"] is None and [int(pl["raw"][q]) for q in PP.squares_of(pl["legal"])] == [50, 5, 4]
    assert [int(pl["row"][q]) for q in PP.squares_of(pl["legal"])] == [0, 5, 4]
    pl = PP.root_play(proven(6, *POSITIONS_6[3], 60, SALT6, 1, 4), *POSITIONS_6[3])
    assert [int(pl["raw"][q]) for q in PP.squares_of(pl["legal"])] == [34, 25] and [int(pl["row"][q]) for q in PP.squares_of(pl["legal"])] == [0, 25]


@pytest.mark.parametrize("K,solve", [(1, 0), (4, 0), (1, 4), (4, 4)])
def test_engine_setting_proven_values_are_exact_and_moves_change(K, solve):
    games, stats = engine_games(K, solve)
    moves = sum(len(g) for g in games)
    proven_roots = masked_unknown = changed = 0
    for g in games:
        for w in g:
            if w["val"] is not None:
                assert w["val"] == SL.exact_sign(w["own"], w["opp"], ENGINE["n"]), (K, solve, w["ply"])
                assert w["value"] == float(w["val"]) and w["code"] == w["val"] + 2
                proven_roots += 1
            else:
                assert w["code"] == 0
                masked_unknown += not np.array_equal(w["counts"], w["raw"])
            changed += w["greedy"] != 0 and w["action"] != w["raw_action"]
            assert legal_mask(w["own"], w["opp"], ENGINE["n"]) >> w["action"] & 1
    print("K", K, "E", solve, "moves", moves, "proven", proven_roots, "masked rows at unknown roots", masked_unknown, stats)
    assert stats["proven_roots"] == proven_roots >= 1 and masked_unknown >= 1
    assert stats["moves_changed"] == changed >= 1
    assert stats["rows_changed"] >= masked_unknown and stats["fallbacks"] == 0


def _records(K=1, solve=0):
    """the engine setting's games as records (RECORD_DTYPE) with pad[2] = the proof code, z the played-out outcome, and their root values"""
    from othellozero_amd import _lib
    from wide_search_ref import apply_move, popcount
    games, _ = engine_games(K, solve)
    recs, vals = [], []
    for gi, g in enumerate(games):
        last = g[-1]
        own, opp = apply_move(last["own"], last["opp"], ENGINE["n"], last["action"])
        fb, fw = (own, opp) if last["player"] == 1 else (opp, own)
        winner = 1 if popcount(fb) >= popcount(fw) else -1
        for w in g:
            r = np.zeros((), _lib.RECORD_DTYPE)
            r["black"], r["white"], r["final_black"], r["final_white"] = w["black"], w["white"], fb, fw
            r["game_id"], r["ply"], r["action"], r["player"], r["greedy"] = ENGINE["first"] + gi, w["ply"], w["action"], w["player"], w["greedy"]
            r["z"] = 1 if winner == w["player"] else -1
            r["pad"][2] = w["code"]
            recs.append(r)
            vals.append(w["value"])
    return np.array(recs, _lib.RECORD_DTYPE), np.array(vals, np.float64)


def test_proof_targets_and_value_targets_against_the_restatement():
    from othellozero_amd import _lib, agents
    rec, val = _records(1, 4)
    assert np.count_nonzero(rec["pad"][:, 2]) >= 1
    assert np.array_equal(_lib.record_proven(rec), np.where(rec["pad"][:, 2] == 0, _lib.PROOF_UNKNOWN, rec["pad"][:, 2].astype(int) - 2))
    # a proven draw of either mover, a proven loss and a proven win whose z is the other sign, by hand
    hand = np.zeros(6, _lib.RECORD_DTYPE)
    hand["game_id"], hand["ply"] = 5, np.arange(6)
    hand["player"] = [1, -1, 1, -1, 1, -1]
    hand["z"] = [-1, 1, 1, -1, 1, 1]
    hand["pad"][:, 2] = [2, 2, 1, 3, 0, 0]
    hand["black"], hand["white"] = 0x0000001008000000, 0x0000000810000000
    want, st = PP.proof_targets(hand)
    want_hand = want
    assert want["z"].tolist() == [1, -1, -1, 1, 1, 1] and st == dict(records=6, proven=4, z_changed=4)
    got = hand.copy()
    assert _lib.proof_targets(got) == st and got.tobytes() == want.tobytes()
    assert _lib.proof_targets(got) == dict(records=6, proven=4, z_changed=0) and got.tobytes() == want.tobytes()      # idempotent
    # the games
    want, st = PP.proof_targets(rec)
    got = rec.copy()
    assert _lib.proof_targets(got) == st and got.tobytes() == want.tobytes() and st["proven"] >= 1
    print("proof targets", st)
    n = ENGINE["n"]
    differs = 0
    hand_val = np.array([0.0, 0.0, -1.0, 1.0, 0.25, -0.5])      # (a proven draw's root value is 0 while its z is +-1: there the flag shows)
    for got, val, vt, E in [(r, v, vt, E) for r, v in ((got, val), (want_hand, hand_val))
                            for vt in ("outcome", ("blend", 0.5), ("td", 0.7), ("td", 1.0), ("td", 0.0)) for E in (0, 4)]:
        if True:
            for xp in (False, True):
                a = agents.rules_value_targets(got, val, n, vt, exact_empties=E, exact_proven=xp)
                b = PP.value_targets(got, val, n, vt, exact_empties=E, exact_proven=xp)
                assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), (vt, E, xp)
                if not xp:                                  # the old entry point is the new one with the flag 0
                    import ctypes as C
                    out = np.zeros(got.size, np.float32)
                    mode, param = _lib.check_value_target(vt)
                    _lib.check(_lib.load().oz_value_targets_x(got.ctypes.data_as(C.c_void_p), _lib.p_f64(val), got.size, n, mode, param, E, 0,
                                                              _lib.p_f32(out)))
                    assert out.tobytes() == a.tobytes(), (vt, E)
                    import value_targets_ref
                    assert value_targets_ref.value_targets(got, val, n, vt, exact_empties=E).tobytes() == a.tobytes(), (vt, E)
                else:
                    differs += a.tobytes() != agents.rules_value_targets(got, val, n, vt, exact_empties=E).tobytes()
    assert differs >= 1                                      # exact_proven restarts a chain somewhere
    with pytest.raises(_lib.OzError):
        import ctypes as C
        _lib.check(_lib.load().oz_value_targets_x(got.ctypes.data_as(C.c_void_p), _lib.p_f64(val), got.size, n, 0, 0.0, 0, 2,
                                                  _lib.p_f32(np.zeros(got.size, np.float32))))


def test_refusals_before_the_library_is_touched(monkeypatch):
    from othellozero_amd import _lib, agents, loop, training
    from othellozero_amd.othelo_mcts import OthelloMCTS

    def boom(*a, **kw):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "require_gpu", boom)
    monkeypatch.setattr(_lib, "load", boom)
    net = object()
    with pytest.raises(ValueError, match="proofs=True"):
        training.SelfPlayEngine(net, 6, 8, 12, value_signs="sound", proof_play=True)
    with pytest.raises(ValueError, match="proofs=True"):
        training.selfplay_batch(net, 6, 8, 12, proof_play=True)
    with pytest.raises(ValueError, match="proof_play=True"):
        training.selfplay_batch(net, 6, 8, 12, value_signs="sound", proofs=True, proof_targets=True)
    with pytest.raises(ValueError, match="proofs=True"):
        training.execute_episode(6, net, 1.0, 12, 1.0, 0.9, proof_play=True)
    with pytest.raises(ValueError, match="proofs=True"):
        OthelloMCTS(6, net, 1.0, value_signs="sound", proof_play=True)
    with pytest.raises(ValueError, match="proofs=True"):
        agents.NeuralNetworkOthelloAgent(None, net, 12, 1.0, proof_play=True)
    with pytest.raises(ValueError, match="proofs=True"):
        agents.arena_batch(net, net, 6, 8, 12, value_signs="sound", proof_play=True)
    with pytest.raises(ValueError, match=r"proof_play\[white\]"):
        agents.arena_batch(net, net, 6, 8, 12, value_signs="sound", proofs=(True, False), proof_play=(True, True))
    with pytest.raises(ValueError, match="black, white"):
        agents.arena_batch(net, net, 6, 8, 12, value_signs="sound", proofs=(True, False), proof_play=True)
    with pytest.raises(ValueError, match="True or False"):
        training.SelfPlayEngine(net, 6, 8, 12, value_signs="sound", proofs=True, proof_play="yes")
    with pytest.raises(ValueError, match="proofs=True"):
        loop.self_play_match(net, net, 6, 8, 12, 1.0, proof_play=True)
    kw = dict(neural_network=net, board_size=6, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1,
              e_greedy=0.9, evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0, self_play_training=True, self_play_interval=1,
              self_play_total_games=2, self_play_threshold=1, checkpoint_filepath="unused.npz", training_buffer_size=64, alias_final_boards=False)
    with pytest.raises(ValueError, match="proofs=True"):
        loop.training(proof_play=True, **kw)
    with pytest.raises(ValueError, match="proof_play=True"):
        loop.training(value_signs="sound", proofs=True, proof_targets=True, **kw)
    kw = lambda proof_play: _lib.search_kw(_lib.check_search_options(value_signs="sound", proofs=True, proof_play=proof_play, pairs=True))
    assert "proof_play" not in kw(False) and "proof_play" not in kw((False, False)) and kw((True, False))["proof_play"] == (True, False)
