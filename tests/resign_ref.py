"""Restatement of resignation (include/othellozero_amd.h, "resignation") as a plain Python episode loop over the CPU oracle: per move
`sims` oracle.Mcts.simulate calls on the game's one persistent tree (or the budget of a playout cap), the root's counts and edge values from
dump_node(orc_mcts_find(...)), the root value of tests/value_targets_ref.root_value, the move rule of tests/move_sampling_ref.selfplay_move,
then the state machine of the rule in Python floats (IEEE float64, never contracted) and the exemption draw over the oracle's stream
primitive (stream 9)."""
import ctypes as C

import numpy as np

import oracle
from move_sampling_ref import selfplay_move, unit
from playout_cap_ref import budget
from replay_ref import RECORD_DTYPE
from value_targets_ref import root_value

RNG_RESIGN = 9
STAT_KEYS = ("games_adjudicated", "adjudicated_plies_sum", "games_exempt", "exempt_triggered", "exempt_wrong", "exempt_trigger_ply_sum")


def step(side, streak, p, q, v, r, min_ply, ply):
    """one searched move -> (side, streak, trigger)"""
    b = float(p) * float(q)
    c = 1 if b >= v else -1 if b <= -v else 0              # NaN fails both compares
    if c == 0:
        side, streak = 0, 0
    elif c == side:
        streak = min(streak + 1, 255)
    else:
        side, streak = c, 1
    return side, streak, streak >= r and ply >= min_ply


def scan(players, values, plies_per_game, v, r, min_ply):
    """the first trigger of every game's sequence -> (ply int32 (games,), side int8 (games,)); -1 and 0 where there is none"""
    ply, sd, at = [], [], 0
    for length in plies_per_game:
        side, streak, first = 0, 0, (-1, 0)
        for i in range(int(length)):
            side, streak, trig = step(side, streak, int(players[at + i]), float(values[at + i]), v, r, min_ply, i)
            if trig and first[0] < 0:
                first = (i, side)
        at += int(length)
        ply.append(first[0])
        sd.append(first[1])
    return np.array(ply, np.int32), np.array(sd, np.int8)


def exempt(seed, game_id, keep_prob):
    """the game is played out regardless iff the unit draw of (seed, game id, 0, stream 9) is below keep_prob"""
    return unit(seed, game_id, 0, RNG_RESIGN) < keep_prob


def episode(n, sims, resign, e_greedy, seed, game_id, salt, keep=0, c=1.0, cap=None):
    """one self-play game under resign = None or (v, r, min_ply, keep_prob) -> (records with the flag in pad[1], count rows int32 (R, 64),
    root values float64 (R,), info): info = dict(adjudicated, exempt, trigger_ply, trigger_side, winner) -- the first trigger where the rule
    is on (-1, 0: none), whether the game was stopped by it, and the winner the records carry"""
    L = oracle.lib()
    m = oracle.Mcts(n, c, oracle.QMODE_F64, salt=salt, keep_mask=keep)
    black, white, player, fin = C.c_uint64(), C.c_uint64(), C.c_int(1), C.c_int(0)
    L.orc_initial_board(n, C.byref(black), C.byref(white))
    is_exempt = resign is not None and exempt(seed, game_id, resign[3])
    moves, rows, vals, ply = [], [], [], 0
    side, streak, first, adjudicated = 0, 0, (-1, 0), False
    while not fin.value:
        b, w, p = black.value, white.value, player.value
        k, fast = budget(seed, game_id, ply, sims, cap)
        for _ in range(k):
            m.simulate(b, w, p)
        own, opp = (b, w) if p == 1 else (w, b)
        rc, cnt, legal = m.counts(own, opp)
        if rc:
            raise KeyError((game_id, ply, rc))
        root = m.dump_node(L.orc_mcts_find(m.h, own, opp))
        assert np.array_equal(root["N"], cnt)
        q = root_value(root["N"], root["Q"])
        action, greedy, _margin = selfplay_move(cnt, legal, e_greedy, seed, game_id, ply)
        moves.append((b, w, p, action, greedy, fast))
        rows.append(cnt)
        vals.append(q)
        trig = False
        if resign is not None:
            side, streak, trig = step(side, streak, p, q, resign[0], resign[1], resign[2], ply)
            if trig and first[0] < 0:
                first = (ply, side)
        L.orc_game_play(C.byref(black), C.byref(white), n, C.byref(player), C.byref(fin), action)
        ply += 1
        if trig and not is_exempt and not fin.value:       # the move was played as ever; the game stops here
            adjudicated = True
            break
    fb, fw = black.value, white.value
    winner = first[1] if adjudicated else (1 if bin(fb).count("1") >= bin(fw).count("1") else -1)         # a draw goes to BLACK
    rec = np.zeros(len(moves), RECORD_DTYPE)
    for i, (b, w, p, action, greedy, fast) in enumerate(moves):
        rec[i] = (b, w, fb, fw, game_id, i, action, p, 1 if winner == p else -1, greedy, (fast, 1 if adjudicated else 0, 0))
    info = dict(adjudicated=adjudicated, exempt=is_exempt, trigger_ply=first[0], trigger_side=first[1], winner=winner)
    return rec, np.array(rows, np.int32).reshape(-1, 64), np.array(vals, np.float64), info


def stats_of(infos, records):
    """the engine's counters from the games' infos (records: to count an adjudicated game's plies)"""
    s = dict.fromkeys(STAT_KEYS, 0)
    for gid, info in infos.items():
        if info["adjudicated"]:
            s["games_adjudicated"] += 1
            s["adjudicated_plies_sum"] += int((records["game_id"] == gid).sum())
        elif info["exempt"]:
            s["games_exempt"] += 1
            if info["trigger_ply"] >= 0:
                s["exempt_triggered"] += 1
                s["exempt_trigger_ply_sum"] += info["trigger_ply"]
                s["exempt_wrong"] += int(info["winner"] != info["trigger_side"])
    return s


def episodes(n, sims, resign, e_greedy, seed, game_ids, salt, keep=0, c=1.0, cap=None):
    """the games with the ids given -> (records, count rows, values) in ascending (game_id, ply), the stats, {game id: info}"""
    ids = sorted(int(g) for g in game_ids)
    out = {g: episode(n, sims, resign, e_greedy, seed, g, salt, keep, c, cap) for g in ids}
    rec = np.concatenate([out[g][0] for g in ids])
    infos = {g: out[g][3] for g in ids}
    return rec, np.concatenate([out[g][1] for g in ids]), np.concatenate([out[g][2] for g in ids]), stats_of(infos, rec), infos
