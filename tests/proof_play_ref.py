"""Restatement of proof play (include/othellozero_amd.h, "proof play") in plain Python over tests/proofs_ref.py, whose ProvenSearch is
imported unchanged: the rule that turns a root's proofs and raw counts into the row, the move, the root value and the proof code; a
self-play episode and an arena replay whose moves follow it; the proof-targets pass; the value targets with exact_proven.

The rule, for a root with legal set L, edge proofs e, own value and raw counts cnt:
    val  = ProvenSearch.val(root);  C = ProvenSearch.candidates(root, val) -- the very set the descent picks from at the root
    keep = C if some square of C has cnt > 0, else L (a fallback)
    row  = cnt on keep, 0 elsewhere;  root value = float(val) if val is known else the raw mean;  code = val + 2, or 0"""
import numpy as np

import move_sampling_ref as ms
import oracle
from proofs_ref import ProvenSearch  # noqa: F401
from value_targets_ref import _empties
from wide_search_ref import apply_move, initial_board, legal_mask, tie_draw

STATS = ("proven_roots", "rows_changed", "moves_changed", "fallbacks")


def squares_of(mask):
    return [s for s in range(64) if (int(mask) >> s) & 1]


def rule(legal, edge, own_value, counts):
    """legal: mask; edge: {square: -1 / 0 / +1}; own_value: -1 / 0 / +1 or None; counts: 64 raw counts -> dict(val, keep, row, fallback,
    inconsistent), stated from scratch (no ProvenSearch needed: the hand tables use it)"""
    acts = squares_of(legal)
    if own_value is not None:
        val = own_value
    elif any(edge.get(s) == 1 for s in acts):
        val = 1
    elif acts and all(s in edge for s in acts):
        val = max(edge[s] for s in acts)
    else:
        val = None
    cands = [s for s in acts if edge.get(s) == val] if val is not None else []
    if not cands:
        cands = [s for s in acts if edge.get(s) != -1]
    bad = not cands
    if bad:
        cands = list(acts)
    fallback = not any(int(counts[s]) > 0 for s in cands)
    keep = list(acts) if fallback else cands
    row = np.zeros(64, np.int32)
    for s in keep:
        row[s] = int(counts[s])
    return dict(val=val, keep=sum(1 << s for s in keep), row=row, fallback=fallback, inconsistent=bad)


def root_play(search, own, opp):
    """the rule at the node of (own, opp) of a ProvenSearch, through the search's own val / candidates -> rule()'s dict plus raw (the counts)"""
    idx = search.index[(own, opp)]
    cnt, lg = search.counts(own, opp)
    was = search.corrupt
    val = search.val(idx)
    cands = search.candidates(idx, val)
    bad, search.corrupt = search.corrupt and not was, was          # (asking is not searching: the search's flag stays what it was)
    fallback = not any(int(cnt[s]) > 0 for s in cands)
    keep = list(search.nodes[idx].acts) if fallback else cands
    row = np.zeros(64, np.int32)
    for s in keep:
        row[s] = int(cnt[s])
    out = dict(val=val, keep=sum(1 << s for s in keep), row=row, fallback=fallback, inconsistent=bad, raw=cnt, legal=lg)
    mine = rule(lg, search.edge[idx], search.own[idx], cnt)
    assert (mine["val"], mine["keep"], mine["fallback"]) == (val, out["keep"], fallback) and np.array_equal(mine["row"], row)
    return out


def root_value(search, own, opp, val):
    return float(val) if val is not None else search.root_value(own, opp)


def code_of(val):
    return 0 if val is None else val + 2


def episode(search, n, sims, seed, game_id, e_greedy, sample_moves=None, stats=None):
    """value_signs_ref.episode with the rule: one self-play game at policy temperature 1 over a ProvenSearch -> list of dict(black, white,
    player, ply, action, greedy, counts = the row, raw = the raw counts, value, code, margin, raw_action) per searched move; stats: a dict
    that takes the four counters (STATS)"""
    black, white = initial_board(n)
    player, ply, out = 1, 0, []
    st = stats if stats is not None else {}
    for k in STATS:
        st.setdefault(k, 0)
    while True:
        own, opp = (black, white) if player == 1 else (white, black)
        lg = legal_mask(own, opp, n)
        if lg == 0:
            if legal_mask(opp, own, n) == 0:
                return out
            player = -player
            continue
        search.simulate(own, opp, sims)
        pl = root_play(search, own, opp)
        action, greedy, margin = ms.selfplay_move(pl["row"], lg, e_greedy, seed, game_id, ply, sample_moves)
        raw_action, _, raw_margin = ms.selfplay_move(pl["raw"], lg, e_greedy, seed, game_id, ply, sample_moves)
        changed = not np.array_equal(pl["row"], pl["raw"])
        st["proven_roots"] += pl["val"] is not None
        st["rows_changed"] += changed
        st["moves_changed"] += bool(changed and greedy != 0 and raw_action != action)
        st["fallbacks"] += pl["fallback"]
        out.append(dict(black=black, white=white, player=player, ply=ply, action=action, greedy=greedy, counts=pl["row"], raw=pl["raw"],
                        value=root_value(search, own, opp, pl["val"]), code=code_of(pl["val"]), margin=min(margin, raw_margin),
                        raw_action=raw_action, val=pl["val"], own=own, opp=opp))
        own, opp = apply_move(own, opp, n, action)
        black, white = (own, opp) if player == 1 else (opp, own)
        player = -player
        ply += 1


def best_move(n, row, legal, tie_u):
    """the square temperature 0 picks from a row: of its maxima the one the tie draw selects (wide_search_ref.WideSearch.best_move)"""
    pol = oracle.policy_from_counts(n, np.asarray(row, np.int32), legal, 0.0, tie_u)
    r, c = np.argwhere(pol == 1.0)[0]
    return int(r) * 8 + int(c)


def play_arena_game(n, sims, seed, gid, agents, proof_play):
    """one arena game from the start: agents = {+1: search of BLACK, -1: search of WHITE}, each searching on its own plies; the colours in
    proof_play move by the rule -> (actions, players, final black, final white, plies whose move differs from the raw counts' one)"""
    black, white = initial_board(n)
    p, ply, actions, players, differ = 1, 0, [], [], 0
    while True:
        own, opp = (black, white) if p == 1 else (white, black)
        if not legal_mask(own, opp, n):
            if not legal_mask(opp, own, n):
                return actions, players, black, white, differ
            p = -p
            continue
        W = agents[p]
        W.simulate(own, opp, sims)
        raw = W.best_move(own, opp, tie_draw(seed, gid, ply))
        want = raw
        if p in proof_play:
            pl = root_play(W, own, opp)
            want = best_move(n, pl["row"], pl["legal"], tie_draw(seed, gid, ply))
        differ += want != raw
        actions.append(want)
        players.append(p)
        own, opp = apply_move(own, opp, n, want)
        black, white = (own, opp) if p == 1 else (opp, own)
        p = -p
        ply += 1


def proven_z(code, player):
    """the sign oz_record.z takes from a proof code != 0: a proven draw is BLACK's win"""
    return 1 if code == 3 else -1 if code == 1 else (1 if player == 1 else -1)


def proof_targets(records):
    """records (RECORD_DTYPE) -> (a copy with z of the proven records set, dict(records, proven, z_changed))"""
    out = np.array(records, copy=True)
    st = dict(records=len(out), proven=0, z_changed=0)
    for i in range(len(out)):
        code = int(out["pad"][i][2])
        if code == 0:
            continue
        z = proven_z(code, int(out["player"][i]))
        st["proven"] += 1
        st["z_changed"] += z != int(out["z"][i])
        out["z"][i] = z
    return out, st


def value_targets(records, values, n, value_target, exact_empties=0, exact_proven=False):
    """value_targets_ref.value_targets where a record with a proof code is exact too (exact_proven)"""
    R = len(records)
    out = np.zeros(R, np.float32)
    mode, param = (value_target, 0.0) if isinstance(value_target, str) else (value_target[0], float(value_target[1]))
    one_minus = 1.0 - param
    games = {}
    for i in range(R):
        games.setdefault(int(records["game_id"][i]), []).append(i)
    for ids in games.values():
        ids.sort(key=lambda i: int(records["ply"][i]))
        last = ids[-1]
        B = float(int(records["player"][last]) * int(records["z"][last]))
        for i in reversed(ids):
            p, z, q = float(int(records["player"][i])), float(int(records["z"][i])), float(values[i])
            exact = (exact_empties > 0 and _empties(records[i], n) <= exact_empties) or (exact_proven and int(records["pad"][i][2]) != 0)
            if mode == "outcome":
                t = z
            elif mode == "blend":
                if exact:
                    t = z
                else:
                    a = one_minus * z
                    b = param * q
                    t = a + b
            else:
                assert mode == "td", mode
                if exact:
                    B = p * z
                else:
                    a = one_minus * (p * q)
                    b = param * B
                    B = a + b
                t = p * B
            out[i] = np.float32(t)
    return out


def root_priors(search, own, opp):
    """the stored priors of the node of (own, opp), float64 (64,) by square (what record_surprise holds the row against)"""
    nd = search.nodes[search.index[(own, opp)]]
    P = np.zeros(64, np.float64)
    for s in nd.acts:
        P[s] = nd.P[s]
    return P
