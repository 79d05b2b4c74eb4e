"""Proof play on the GPU (pytest -m gpu): the proven rows and root values of the bare search, the self-play engine's moves, records, visit
rows, root values, proof codes and counters, the proof-targets pass, the option beside root noise, move sampling, recorded surprise,
resignation and TD targets, the arena with the option on one agent -- all against the restatement tests/proof_play_ref.py, bit for bit --
and the option off against objects never given it, the setters' refusals and the training loop.  Stub network and q_mode F64."""
import ctypes as C
import functools
import logging

import numpy as np
import pytest

import proof_play_ref as PP
import resign_ref
import solve_leaves_ref as SL
import surprise_ref
from move_sampling_ref import selfplay_move
from proofs_ref import DRAW_POSITION, ProvenSearch
from root_noise_ref import dirichlet
from value_signs_ref import POSITIONS_6, SoundSearch
from wide_search_ref import initial_board, legal_mask, popcount

pytestmark = pytest.mark.gpu

SOUND = 1
SALT6 = 7
CASES = [(4, *initial_board(4), sims, salt) for sims in (100, 200) for salt in (3, 11)] + [(6, own, opp, 60, SALT6) for own, opp in POSITIONS_6]
DRAW_CASE = (6, *DRAW_POSITION, 120, SALT6)
N, G, SIMS, SALT, SEED, FIRST, EG = 6, 8, 12, 21, 77, 300, 0.8          # the engine setting of tests/test_gpu_proofs.py


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@functools.lru_cache(maxsize=None)
def proven(n, own, opp, sims, salt, K, solve=0):
    """the restatement's search of one case, computed once and shared (read only)"""
    ev = SL.evaluator(solve, SL.stub(salt, 0)) if solve else None
    s = ProvenSearch(n, 1.0, K, salt=salt, evaluator=ev, solve=solve)
    s.simulate(own, opp, sims)
    return s


@functools.lru_cache(maxsize=None)
def ref_games(K, solve=0, sample=None):
    """the 8 games of the engine setting under the rule, computed once and shared (read only) -> ({game id: episode}, the four counters)"""
    stats, games = {}, {}
    for gid in range(FIRST, FIRST + G):
        ev = SL.evaluator(solve, SL.stub(SALT, 0)) if solve else None
        W = ProvenSearch(N, 1.0, K, salt=SALT, evaluator=ev, solve=solve)
        games[gid] = PP.episode(W, N, SIMS, SEED, gid, EG, sample_moves=sample, stats=stats)
        assert not W.corrupt
    return games, stats


def _engine(net, K=1, proof_play=True, **kw):
    from othellozero_amd.training import SelfPlayEngine
    return SelfPlayEngine(net, N, G, SIMS, 1.0, 1.0, EG, seed=SEED, first_game_id=FIRST, record_visits=True, record_values=True,
                          leaves_per_step=K, value_signs="sound", proofs=True, proof_play=proof_play, **kw)


def _stub(K=1, n=N, salt=SALT, games=G):
    from othellozero_amd.NNet import StubNetWrapper
    return StubNetWrapper((n, n), salt, 0, max_batch=games * K)


def same_game(r, v, q, want, where):
    """records r, visit rows v and root values q of one game against the restatement's episode"""
    assert r.size == len(want) > 0, where
    for i, w in enumerate(want):
        got = tuple(int(r[k][i]) for k in ("black", "white", "player", "ply", "action", "greedy"))
        assert got == (w["black"], w["white"], w["player"], w["ply"], w["action"], w["greedy"]), (where, i)
        assert int(r["pad"][i][2]) == w["code"] and int(r["pad"][i][0]) == 0 and int(r["pad"][i][1]) == 0, (where, i)
        assert np.array_equal(v[i], w["counts"]), (where, i)
        assert q[i] == w["value"], (where, i, q[i], w["value"])


# ------------------------------------------------------------------ 1. the bare search
class Search:
    """a bare oz_mcts with G slots, sound signs and proofs"""

    def __init__(self, oz, n, slots, K=1, proofs=1, solve=0):
        self.oz, self.lib, self.G = oz, oz.load(), slots
        self.h = C.c_void_p()
        oz.check(self.lib.oz_mcts_create(C.byref(self.h), n, slots, 1024, 1.0, oz.QMODE_F64))
        oz.check(self.lib.oz_mcts_set_value_signs(self.h, SOUND))
        if proofs:
            oz.check(self.lib.oz_mcts_set_proofs(self.h, 1))
        if K != 1:
            oz.check(self.lib.oz_mcts_set_leaves_per_step(self.h, K))
        if solve:
            oz.check(self.lib.oz_mcts_set_solve_leaves(self.h, solve))

    def __del__(self):
        if self.h:
            self.lib.oz_mcts_destroy(self.h)
            self.h = C.c_void_p()

    def search(self, net, roots, sims):
        a, b = np.array([r[0] for r in roots], np.uint64), np.array([r[1] for r in roots], np.uint64)
        self.oz.check(self.lib.oz_mcts_set_roots(self.h, self.oz.p_u64(a), self.oz.p_u64(b), None))
        self.oz.check(self.lib.oz_mcts_simulate(self.h, net._h, int(sims)))

    def counts(self, fn):
        cnt, legal, rc = np.zeros((self.G, 64), np.int32), np.zeros(self.G, np.uint64), np.zeros(self.G, np.int32)
        self.oz.check(getattr(self.lib, fn)(self.h, self.oz.p_i32(cnt), self.oz.p_u64(legal), self.oz.p_i32(rc)))
        return cnt, legal, rc

    def values(self, fn):
        val, rc = np.zeros(self.G, np.float64), np.zeros(self.G, np.int32)
        self.oz.check(getattr(self.lib, fn)(self.h, self.oz.p_f64(val), self.oz.p_i32(rc)))
        return val, rc


@pytest.mark.parametrize("K", [1, 4])
def test_bare_search_vs_restatement(oz, K):
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    changed = known = 0
    for n, own, opp, sims, salt in CASES + [DRAW_CASE]:
        m = OthelloMCTS(n, _stub(K, n, salt, 1), 1.0, q_mode=oz.QMODE_F64, node_cap=1024, leaves_per_step=K, value_signs="sound", proofs=True,
                        proof_play=True)
        board = oz.unpack_board(own, opp, n)
        m.simulate_n(board, OthelloPlayer.BLACK, sims)
        ref = proven(n, own, opp, sims, salt, K)
        pl = PP.root_play(ref, own, opp)
        where = (n, sims, salt, K)
        assert np.array_equal(m.proven_counts(board), pl["row"]), where
        assert np.array_equal(m._counts(board)[1], pl["raw"]), where                     # root_counts is still the raw one
        assert m.root_value(board, proven=True) == PP.root_value(ref, own, opp, pl["val"]), where
        assert m.root_value(board) == ref.root_value(own, opp), where                    # ... and so is root_values
        pol = m.get_policy_action_probabilities(board, 1.0, proven=True)
        total = float(pl["row"].sum())
        assert np.array_equal(pol, (pl["row"].astype(np.float64).reshape(8, 8)[:n, :n] ** 1.0) / total), where
        changed += not np.array_equal(pl["row"], pl["raw"])
        known += pl["val"] is not None
    assert changed >= 2 and known >= 2


@pytest.mark.parametrize("K", [1, 4])
def test_bare_search_64_games_in_one_object(oz, K):
    n, slots, sims = 6, 64, 60
    roots = [(list(POSITIONS_6) + [DRAW_POSITION])[g % 5] for g in range(slots)]
    s = Search(oz, n, slots, K=K)
    s.search(_stub(K, n, SALT6, slots), roots, sims)
    row, legal, rc = s.counts("oz_mcts_proven_counts")
    raw, legal2, rc2 = s.counts("oz_mcts_root_counts")
    val, vrc = s.values("oz_mcts_proven_root_values")
    rawv, _ = s.values("oz_mcts_root_values")
    assert not rc.any() and not rc2.any() and not vrc.any() and np.array_equal(legal, legal2)
    for g in range(slots):
        ref = proven(n, *roots[g], sims, SALT6, K)
        pl = PP.root_play(ref, *roots[g])
        assert np.array_equal(row[g], pl["row"]) and np.array_equal(raw[g], pl["raw"]) and int(legal[g]) == pl["legal"], (K, g)
        assert val[g] == PP.root_value(ref, *roots[g], pl["val"]) and rawv[g] == ref.root_value(*roots[g]), (K, g)
    # a root that is not in the table: rc 1 and zero rows, like oz_mcts_root_counts
    a, b = np.array([r[1] for r in roots], np.uint64), np.array([r[0] for r in roots], np.uint64)
    oz.check(s.lib.oz_mcts_set_roots(s.h, oz.p_u64(a), oz.p_u64(b), None))
    row, _, rc = s.counts("oz_mcts_proven_counts")
    val, vrc = s.values("oz_mcts_proven_root_values")
    assert (rc == 1).all() and not row.any() and (vrc == 1).all() and not val.any()
    # an object without proofs refuses, and goes on
    t = Search(oz, n, 4, proofs=0)
    t.search(_stub(1, n, SALT6, 4), list(POSITIONS_6), 20)
    cnt, lg, rcs = np.zeros((4, 64), np.int32), np.zeros(4, np.uint64), np.zeros(4, np.int32)
    assert t.lib.oz_mcts_proven_counts(t.h, oz.p_i32(cnt), oz.p_u64(lg), oz.p_i32(rcs)) == oz.OZ_ERR_STATE
    assert t.lib.oz_mcts_proven_root_values(t.h, oz.p_f64(np.zeros(4)), oz.p_i32(rcs)) == oz.OZ_ERR_STATE
    assert not t.counts("oz_mcts_root_counts")[2].any()


# ------------------------------------------------------------------ 2. the engine through play_to_end()
@pytest.mark.parametrize("K", [1, 4])
def test_selfplay_engine_vs_restatement(oz, K):
    net = _stub(K)
    eng = _engine(net, K)
    eng.play_to_end()
    assert eng.stats()["live_games"] == 0
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    games, stats = ref_games(K)
    for gid, want in games.items():
        sel = rec["game_id"] == gid
        same_game(rec[sel], vis[sel], val[sel], want, (K, gid))
        r = rec[sel]
        fb, fw = int(r["final_black"][0]), int(r["final_white"][0])
        assert all(int(r["z"][i]) == (1 if popcount(fb) >= popcount(fw) else -1) * int(r["player"][i]) for i in range(r.size)), gid
    assert eng.proof_play_stats() == stats and tuple(eng.proof_play_stats()) == PP.STATS, (eng.proof_play_stats(), stats)
    assert np.array_equal(oz.record_proven(rec), np.where(rec["pad"][:, 2] == 0, oz.PROOF_UNKNOWN, rec["pad"][:, 2].astype(int) - 2))
    # at least one move is another than the raw counts' one: these are not the games of proofs=True alone
    assert stats["moves_changed"] >= 1 and stats["proven_roots"] >= 1 and stats["rows_changed"] >= 1
    plain = _engine(net, K, proof_play=False)
    plain.play_to_end()
    prec = plain.records()
    assert prec["action"].tobytes() != rec["action"].tobytes() or prec.size != rec.size
    assert not prec["pad"].any() and plain.proof_play_stats() == dict.fromkeys(PP.STATS, 0)


def test_last_counts_stay_raw(oz):
    """one round from a position whose rule row differs: after a few rounds some slot's last_counts differ from its recorded row"""
    eng = _engine(_stub())
    games, _ = ref_games(1)
    seen = 0
    for rnd in range(N * N):
        st = eng.state()
        if st["finished"].all():
            break
        eng.run(1)
        cnt = eng.last_counts()
        for g in range(G):
            if st["finished"][g]:
                continue
            w = games[int(st["game_id"][g])][int(st["ply"][g])]
            assert np.array_equal(cnt[g], w["raw"]), (rnd, g)
            seen += not np.array_equal(w["raw"], w["counts"])
    assert seen >= 1


# ------------------------------------------------------------------ 3. solved leaves, then the proof-targets pass
def test_solved_leaves_and_proof_targets(oz):
    from othellozero_amd import agents
    eng = _engine(_stub(), solve_leaves=4)
    eng.play_to_end()
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    games, stats = ref_games(1, 4)
    for gid, want in games.items():
        sel = rec["game_id"] == gid
        same_game(rec[sel], vis[sel], val[sel], want, gid)
    assert eng.proof_play_stats() == stats
    want, st = PP.proof_targets(rec)
    assert eng.proof_targets() == st and st["proven"] >= 1
    after = eng.records()
    assert after.tobytes() == want.tobytes()
    assert eng.proof_targets() == dict(st, z_changed=0) and eng.records().tobytes() == want.tobytes()            # a second call changes nothing
    assert eng.proof_targets(first_record=5) == dict(records=st["records"] - 5, proven=int(np.count_nonzero(rec["pad"][5:, 2])), z_changed=0)
    # every flagged record's value is the exact solver's sign (6x6: at most 12 empties wherever a root was proven here)
    flagged = after[after["pad"][:, 2] != 0]
    _, _, score, solved = agents.rules_solve(flagged["black"], flagged["white"], flagged["player"], N)
    assert solved.all() and np.array_equal(oz.record_proven(flagged), np.sign(score).astype(np.int8))


# ------------------------------------------------------------------ 4. beside the other options
def test_with_root_noise_and_move_sampling(oz):
    """round by round, as tests/test_gpu_proofs.py does: the device's own eta goes into the restatement, whose raw counts must then agree
    exactly; the move is move_sampling_ref's over the rule's row; at the end the recorded rows, values, codes and counters are the rule's"""
    alpha, eps, sample = 0.5, 0.25, (1.0, 6)
    eng = _engine(_stub(), root_noise=(alpha, eps), sample_moves=sample)
    W = [ProvenSearch(N, 1.0, 1, salt=SALT) for _ in range(G)]
    stats = dict.fromkeys(PP.STATS, 0)
    want, sampled, tight = {}, 0, 0
    for rnd in range(N * N):
        st = eng.state()
        if st["finished"].all():
            break
        eng.run(1)
        eta, armed = eng.last_root_noise()
        cnt, after = eng.last_counts(), eng.state()
        for g in range(G):
            if st["finished"][g]:
                continue
            b, w, p, ply, gid = int(st["black"][g]), int(st["white"][g]), int(st["player"][g]), int(st["ply"][g]), int(st["game_id"][g])
            own, opp = (b, w) if p == 1 else (w, b)
            lg = legal_mask(own, opp, N)
            assert armed[g] and np.abs(eta[g] - dirichlet(N, lg, alpha, SEED, gid, ply)[0]).max() <= 1e-9, (rnd, g)
            W[g].set_noise(own, opp, eta[g], eps)
            W[g].simulate(own, opp, SIMS)
            pl = PP.root_play(W[g], own, opp)
            assert np.array_equal(cnt[g], pl["raw"]), (rnd, g)
            action, greedy, margin = selfplay_move(pl["row"], lg, EG, SEED, gid, ply, sample)
            raw_action, _, raw_margin = selfplay_move(pl["raw"], lg, EG, SEED, gid, ply, sample)
            placed = (int(after["black"][g]) | int(after["white"][g])) & ~(b | w)
            if margin >= 1e-9:
                assert placed == 1 << action, (rnd, g, greedy)
            tight += min(margin, raw_margin) < 1e-9
            changed = not np.array_equal(pl["row"], pl["raw"])
            stats["proven_roots"] += pl["val"] is not None
            stats["rows_changed"] += changed
            stats["moves_changed"] += bool(changed and greedy != 0 and raw_action != action)
            stats["fallbacks"] += pl["fallback"]
            want[(gid, ply)] = (pl["row"], PP.root_value(W[g], own, opp, pl["val"]), PP.code_of(pl["val"]), greedy)
            sampled += greedy == 2
    assert eng.stats()["live_games"] == 0 and sampled >= G
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    assert rec.size == len(want)
    for i in range(rec.size):
        row, value, code, greedy = want[(int(rec["game_id"][i]), int(rec["ply"][i]))]
        assert np.array_equal(vis[i], row) and val[i] == value and int(rec["pad"][i][2]) == code and int(rec["greedy"][i]) == greedy, i
    assert stats["proven_roots"] >= 1
    if not tight:                                          # (a draw within 1e-9 of a boundary may fall either way: about 1 in 1e7)
        assert eng.proof_play_stats() == stats


def test_with_recorded_surprise(oz):
    """the surprise of a move is that of the masked row against the root's stored priors"""
    from othellozero_amd import agents
    eng = _engine(_stub(), record_surprise=True)
    eng.play_to_end()
    rec, vis, sur = eng.records(with_visits=True, with_surprise=True)
    games, stats = ref_games(1)
    P = np.zeros((rec.size, 64), np.float64)
    rows = np.zeros((rec.size, 64), np.int32)
    W = {gid: ProvenSearch(N, 1.0, 1, salt=SALT) for gid in games}
    for i in range(rec.size):                              # (records are in ascending (game, ply) per game: replay each game's searches in order)
        gid, ply = int(rec["game_id"][i]), int(rec["ply"][i])
        w = games[gid][ply]
        W[gid].simulate(w["own"], w["opp"], SIMS)
        P[i], rows[i] = PP.root_priors(W[gid], w["own"], w["opp"]), w["counts"]
        assert np.array_equal(vis[i], w["counts"]), i
    assert sur.tobytes() == agents.rules_policy_surprise(rows, P).tobytes()
    want, abs_sum = surprise_ref.surprises(rows, P)
    assert (np.abs(sur - want) <= surprise_ref.bound(abs_sum)).all()
    raw = np.stack([games[int(rec["game_id"][i])][int(rec["ply"][i])]["raw"] for i in range(rec.size)])
    assert agents.rules_policy_surprise(raw, P).tobytes() != sur.tobytes()              # ... and not that of the raw row
    assert eng.proof_play_stats() == stats


def test_with_resignation_a_proven_root_triggers(oz):
    """resign = (0.9, 1, 0, 0.0): the first searched move whose root value reaches +-0.9 stops the game; a proven win or loss is +-1 exactly"""
    v, r, min_ply = 0.9, 1, 0
    eng = _engine(_stub(), resign=(v, r, min_ply, 0.0))
    eng.play_to_end()
    rec, vis, val = eng.records(with_visits=True, with_values=True)
    games, _ = ref_games(1)
    on_proof = adjudicated = 0
    for gid, want in games.items():
        sel = rec["game_id"] == gid
        rr, vv, qq = rec[sel], vis[sel], val[sel]
        side, streak, stop = 0, 0, None
        for i, w in enumerate(want):
            side, streak, trig = resign_ref.step(side, streak, w["player"], w["value"], v, r, min_ply, i)
            if trig:
                stop = i
                break
        n_rec = len(want) if stop is None else stop + 1
        assert rr.size == n_rec, (gid, rr.size, n_rec)
        ends_itself = stop is not None and stop == len(want) - 1
        for i in range(n_rec):
            w = want[i]
            assert (int(rr["action"][i]), int(rr["greedy"][i]), int(rr["pad"][i][2])) == (w["action"], w["greedy"], w["code"]), (gid, i)
            assert np.array_equal(vv[i], w["counts"]) and qq[i] == w["value"], (gid, i)
            if stop is not None and not ends_itself:
                assert int(rr["pad"][i][1]) == 1 and int(rr["z"][i]) == (1 if side == int(rr["player"][i]) else -1), (gid, i)
            else:
                assert int(rr["pad"][i][1]) == 0, (gid, i)
        if stop is not None and not ends_itself:
            adjudicated += 1
            on_proof += want[stop]["code"] in (1, 3) and abs(want[stop]["value"]) == 1.0
    assert eng.resign_stats()["games_adjudicated"] == adjudicated >= 1 and on_proof >= 1


def test_with_td_targets_and_exact_proven(oz):
    eng = _engine(_stub(), solve_leaves=4)
    eng.play_to_end(proof_targets=True, value_target=("td", 0.7))
    rec, val, tgt = eng.records(with_values=True, with_targets=True)
    assert eng.proof_target_stats["proven"] == int(np.count_nonzero(rec["pad"][:, 2])) >= 1
    want = PP.value_targets(rec, val, N, ("td", 0.7), exact_proven=True)
    assert tgt.dtype == np.float32 and tgt.tobytes() == want.tobytes()
    assert eng.value_target_stats["exact"] == int(np.count_nonzero(rec["pad"][:, 2]))
    from othellozero_amd import agents
    assert agents.rules_value_targets(rec, val, N, ("td", 0.7), exact_proven=True).tobytes() == tgt.tobytes()
    # the entry without the flag is the one with the flag 0
    a = eng.value_targets(("blend", 0.5), exact_empties=4)
    t_old = eng.records(with_targets=True)[1].copy()
    s = oz.ValueTargetStats()
    oz.check(oz.load().oz_selfplay_value_targets_x(eng._h, 0, oz.VALUE_TARGET_BLEND, 0.5, 4, 0, C.byref(s)))
    assert eng.records(with_targets=True)[1].tobytes() == t_old.tobytes() and a == {k: int(getattr(s, k)) for k, _ in s._fields_}
    assert t_old.tobytes() == PP.value_targets(rec, val, N, ("blend", 0.5), exact_empties=4).tobytes()
    b = eng.value_targets(("blend", 0.5), exact_empties=4, exact_proven=True)
    assert eng.records(with_targets=True)[1].tobytes() == PP.value_targets(rec, val, N, ("blend", 0.5), exact_empties=4, exact_proven=True).tobytes()
    assert b["exact"] >= a["exact"]
    assert oz.load().oz_selfplay_value_targets_x(eng._h, 0, oz.VALUE_TARGET_BLEND, 0.5, 4, 2, None) == oz.OZ_ERR_ARG


# ------------------------------------------------------------------ 5. the arena: the option on BLACK alone
def test_arena_with_proof_play_on_one_agent(oz):
    from othellozero_amd.agents import arena_batch
    n, games, sims, seed, first = 6, 8, 12, 7, 900
    na, nb = _stub(1, n, 41, games), _stub(1, n, 42, games)
    kw = dict(seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, value_signs="sound", proofs=(True, False))
    r = arena_batch(na, nb, n, games, sims, 1.0, proof_play=(True, False), **kw)
    differ = 0
    for gi in range(games):
        agents = {1: ProvenSearch(n, 1.0, 1, salt=41), -1: SoundSearch(n, 1.0, 1, salt=42)}
        actions, players, fb, fw, d = PP.play_arena_game(n, sims, seed, first + gi, agents, {1})
        k = int(r["n_moves"][gi])
        assert k == len(actions) and r["actions"][gi][:k].tolist() == actions and r["players"][gi][:k].tolist() == players, gi
        assert (int(r["final_black"][gi]), int(r["final_white"][gi])) == (fb, fw), gi
        differ += d
    assert differ >= 1
    plain = arena_batch(na, nb, n, games, sims, 1.0, **kw)
    assert plain["actions"].tobytes() != r["actions"].tobytes()
    both = arena_batch(na, nb, n, games, sims, 1.0, seed=seed, first_game_id=first, q_mode=oz.QMODE_F64, value_signs="sound", proofs=True,
                       proof_play=True)
    for gi in range(games):
        agents = {1: ProvenSearch(n, 1.0, 1, salt=41), -1: ProvenSearch(n, 1.0, 1, salt=42)}
        actions, players, fb, fw, _ = PP.play_arena_game(n, sims, seed, first + gi, agents, {1, -1})
        k = int(both["n_moves"][gi])
        assert both["actions"][gi][:k].tolist() == actions and (int(both["final_black"][gi]), int(both["final_white"][gi])) == (fb, fw), gi


# ------------------------------------------------------------------ 6. off is off; the setters' refusals
def _arena(oz, net, setter):
    lib, h = oz.load(), C.c_void_p()
    games = 4
    oz.check(lib.oz_arena_create(C.byref(h), N, games, 10, 1.0, oz.QMODE_F64, 1, 0, net._h, net._h, 0))
    try:
        oz.check(lib.oz_arena_set_value_signs(h, SOUND, SOUND))
        oz.check(lib.oz_arena_set_proofs(h, 1, 1))
        setter(lib, h)
        oz.check(lib.oz_arena_run_rounds(h, 0))
        winner, points, nm = np.zeros(games, np.int8), np.zeros(games, np.int32), np.zeros(games, np.int32)
        acts, pls = np.zeros((games, 128), np.uint8), np.zeros((games, 128), np.int8)
        fb, fw = np.zeros(games, np.uint64), np.zeros(games, np.uint64)
        oz.check(lib.oz_arena_results(h, oz.p_i8(winner), oz.p_i32(points), oz.p_i32(nm), oz.p_u8(acts), oz.p_i8(pls), oz.p_u64(fb), oz.p_u64(fw)))
        return b"".join(x.tobytes() for x in (winner, points, nm, acts, pls, fb, fw))
    finally:
        lib.oz_arena_destroy(h)


def test_off_is_off_and_the_setters_refuse(oz):
    from othellozero_amd.training import SelfPlayEngine
    lib = oz.load()
    net = _stub(4)

    def err():
        return lib.oz_last_error().decode()
    for K in (1, 4):
        x, y = _engine(net, K, proof_play=False), _engine(net, K, proof_play=False)
        oz.check(lib.oz_selfplay_set_proof_play(y._h, 1))
        oz.check(lib.oz_selfplay_set_proof_play(y._h, 0))
        for e in (x, y):
            e.play_to_end()
        a, b = x.records(with_visits=True, with_values=True), y.records(with_visits=True, with_values=True)
        assert a[0].size > 0 and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
        assert not a[0]["pad"][:, 2].any() and not b[0]["pad"][:, 2].any()
        assert y.proof_play_stats() == dict.fromkeys(PP.STATS, 0)
        # after the first driver call the setter refuses, and the engine goes on
        assert lib.oz_selfplay_set_proof_play(y._h, 1) == oz.OZ_ERR_STATE and "before the first driver call" in err()
        assert y.proof_targets() == dict(records=a[0].size, proven=0, z_changed=0)
    # without proofs: refused, and the engine plays the games of the engine never asked
    kw = dict(seed=5, first_game_id=40, record_visits=True, record_values=True, value_signs="sound")
    x, y = SelfPlayEngine(net, N, 4, 12, **kw), SelfPlayEngine(net, N, 4, 12, **kw)
    assert lib.oz_selfplay_set_proof_play(y._h, 1) == oz.OZ_ERR_STATE and "proofs" in err()
    assert lib.oz_selfplay_set_proof_play(y._h, 2) == oz.OZ_ERR_ARG
    for e in (x, y):
        e.play_to_end()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x.records(with_visits=True, with_values=True), y.records(with_visits=True, with_values=True)))
    # proofs cannot be switched off under proof play
    z = SelfPlayEngine(net, N, 4, 12, proofs=True, proof_play=True, **kw)
    assert lib.oz_selfplay_set_proofs(z._h, 0) == oz.OZ_ERR_STATE and "proof play" in err()
    z.run(2)
    assert z.stats()["moves"] == 8
    # the arena: never given the option against enable = 0
    never = _arena(oz, net, lambda lib, h: None)
    off = _arena(oz, net, lambda lib, h: (oz.check(lib.oz_arena_set_proof_play(h, 1, 1)), oz.check(lib.oz_arena_set_proof_play(h, 0, 0))))
    assert never == off
    h = C.c_void_p()
    oz.check(lib.oz_arena_create(C.byref(h), N, 4, 10, 1.0, oz.QMODE_F64, 1, 0, net._h, net._h, 0))
    try:
        assert lib.oz_arena_set_proof_play(h, 1, 0) == oz.OZ_ERR_STATE and "proofs" in err()
        oz.check(lib.oz_arena_set_value_signs(h, SOUND, SOUND))
        oz.check(lib.oz_arena_set_proofs(h, 1, 0))
        assert lib.oz_arena_set_proof_play(h, 1, 1) == oz.OZ_ERR_STATE and "proofs" in err()
        oz.check(lib.oz_arena_set_proof_play(h, 1, 0))
        assert lib.oz_arena_set_proofs(h, 0, 0) == oz.OZ_ERR_STATE and "proof play" in err()
        oz.check(lib.oz_arena_run_rounds(h, 2))
        assert lib.oz_arena_set_proof_play(h, 0, 0) == oz.OZ_ERR_STATE and "before the first run" in err()
        oz.check(lib.oz_arena_run_rounds(h, 2))
    finally:
        lib.oz_arena_destroy(h)


# ------------------------------------------------------------------ 7. loop.training: one setting for self-play, the match and the evaluation
@pytest.mark.parametrize("replay", ["host", "device"])
def test_training_loop_passes_the_options_on(oz, tmp_path, monkeypatch, caplog, replay):
    from othellozero_amd import loop, training
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    seen, passes = [], []
    real_engine, real_arena = training.SelfPlayEngine, loop.arena_batch

    class Engine(real_engine):
        def __init__(self, *a, **kw):
            seen.append(("engine", kw.get("proofs"), kw.get("proof_play")))
            super().__init__(*a, **kw)

        def proof_targets(self, *a, **kw):
            passes.append("proof_targets")
            return super().proof_targets(*a, **kw)

        def value_targets(self, *a, **kw):
            passes.append(("value_targets", kw.get("exact_proven")))
            return super().value_targets(*a, **kw)

    def arena(*a, **kw):
        seen.append(("arena", kw.get("proofs"), kw.get("proof_play")))
        return real_arena(*a, **kw)
    monkeypatch.setattr(training, "SelfPlayEngine", Engine)
    monkeypatch.setattr(loop, "arena_batch", arena)
    n = 6
    net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    kw = dict(board_size=n, num_iterations=1, num_episodes=8, num_simulations=6, degree_exploration=1, temperature=1, e_greedy=0.9,
              evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0, self_play_training=True, self_play_interval=1,
              self_play_total_games=2, self_play_threshold=1, checkpoint_filepath=str(tmp_path / "net.npz"),
              training_buffer_size=8 * 40 * 8, seed=13, alias_final_boards=False, batched_evaluation=True, reference_aliasing=False)
    with caplog.at_level(logging.INFO):
        historic = loop.training(neural_network=net, replay=replay, value_signs="sound", proofs=True, proof_play=True, proof_targets=True,
                                 value_target=("td", 0.7), **kw)
    assert len(historic) == 1
    assert [k for k, _, _ in seen].count("engine") == 1 and [k for k, _, _ in seen].count("arena") >= 4      # a match (2 arenas) and two evaluations
    assert all(p is True and pp is True for _, p, pp in seen), seen
    assert passes == ["proof_targets", ("value_targets", True)], passes                 # the pass first, then the targets that read it
    assert len(loop.training.proof_play_history) == 1
    h = loop.training.proof_play_history[0]
    assert tuple(h)[:4] == PP.STATS and set(h["targets"]) == {"records", "proven", "z_changed"}
    assert any("proof play:" in m and "proof targets:" in m for m in caplog.messages)
    with pytest.raises(ValueError):
        loop.training(neural_network=net, replay=replay, value_signs="sound", proof_play=True, **kw)
    with pytest.raises(ValueError):
        loop.training(neural_network=net, replay=replay, value_signs="sound", proofs=True, proof_targets=True, **kw)


# ------------------------------------------------------------------ 8. the drop-in search and episode
def test_drop_in_search_and_episode(oz):
    """OthelloMCTS(proof_play=True): the arg-max and the sampled move over the proven row of the [50, 5, 4] root, whose 50 is a proven loss;
    execute_episode at e_greedy = 1 (every move greedy: no host random number decides) against the restatement's episode"""
    from move_sampling_ref import sample
    from othellozero_amd.Othello import OthelloPlayer
    from othellozero_amd.othelo_mcts import OthelloMCTS
    from othellozero_amd.training import execute_episode
    n = 6
    own, opp = POSITIONS_6[1]
    m = OthelloMCTS(n, _stub(1, n, SALT6, 1), 1.0, q_mode=oz.QMODE_F64, node_cap=1024, value_signs="sound", proofs=True, proof_play=True)
    board = oz.unpack_board(own, opp, n)
    m.simulate_n(board, OthelloPlayer.BLACK, 60)
    pl = PP.root_play(proven(n, own, opp, 60, SALT6, 1), own, opp)
    lost, best = int(np.argmax(pl["raw"])), int(np.argmax(pl["row"]))
    assert pl["row"][lost] == 0 and lost != best
    hot = m.get_policy_action_probabilities(board, 0, proven=True)
    assert hot.sum() == 1 and hot[best >> 3, best & 7] == 1
    assert m.get_policy_action_probabilities(board, 0)[lost >> 3, lost & 7] == 1           # the raw counts still say the lost move
    for ply in range(8):
        a, margin = sample(pl["row"], pl["legal"], 1.0, 5, 9, ply)
        got = m.sample_action(board, 1.0, 5, 9, ply, proven=True)
        assert got != (lost >> 3, lost & 7), ply
        if margin >= 1e-9:
            assert got == (a >> 3, a & 7), ply
    ex = execute_episode(N, _stub(), 1.0, SIMS, 1.0, 1.0, snapshot_boards=True, policy_target="visits", value_signs="sound", proofs=True,
                         proof_play=True)
    want = PP.episode(ProvenSearch(N, 1.0, 1, salt=SALT), N, SIMS, 0, 0, 1.0)
    assert len(ex) == 8 * len(want)
    for i, w in enumerate(want):
        b, pol, _ = ex[8 * i + 7]                           # (the eighth symmetry is the identity)
        assert oz.pack_board(b) == (w["black"], w["white"]), i
        row = w["counts"].astype(np.float64).reshape(8, 8)[:N, :N]
        assert np.array_equal(pol, row / row.sum()), i
    assert any(not np.array_equal(w["counts"], w["raw"]) for w in want)
