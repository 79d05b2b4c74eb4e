"""Restatement of the playout cap (include/othellozero_amd.h, "playout cap") as a plain Python episode loop over the CPU oracle: per move the
budget from the oracle's stream primitive (stream 6), that many oracle.Mcts.simulate calls on the game's one persistent tree, the root's counts,
the move rule of tests/move_sampling_ref.selfplay_move (policy temperature != 0: first maximum, e-greedy coin, explore branch) and
orc_game_play.  No root noise here: a fast move has none by definition, and the noise of the full moves has its own restatement
(tests/root_noise_ref.py)."""
import ctypes as C

import numpy as np

import oracle
from move_sampling_ref import selfplay_move, unit
from replay_ref import RECORD_DTYPE

RNG_PLAYOUT = 6


def is_full(seed, game_id, ply, full_prob):
    """the draw: the searched move of (game_id, ply) is full iff u < full_prob"""
    return unit(seed, game_id, ply, RNG_PLAYOUT) < full_prob


def budget(seed, game_id, ply, sims, cap):
    """cap = None or (fast_sims, full_prob) -> (simulations of the move, flag: 0 full / 1 fast)"""
    if cap is None or is_full(seed, game_id, ply, cap[1]):
        return sims, 0
    return cap[0], 1


def episode(n, sims, cap, e_greedy, seed, game_id, salt, keep=0, c=1.0, sample_moves=None):
    """one self-play game -> (records with the flag in pad[0], count rows int32 (R, 64), sum of the budgets).  KeyError where the reference
    raises it (a root expanded but never selected from)."""
    L = oracle.lib()
    m = oracle.Mcts(n, c, oracle.QMODE_F64, salt=salt, keep_mask=keep)
    black, white, player, fin = C.c_uint64(), C.c_uint64(), C.c_int(1), C.c_int(0)
    L.orc_initial_board(n, C.byref(black), C.byref(white))
    moves, rows, spent, ply = [], [], 0, 0
    while not fin.value:
        b, w, p = black.value, white.value, player.value
        k, fast = budget(seed, game_id, ply, sims, cap)
        for _ in range(k):
            m.simulate(b, w, p)
        spent += k
        rc, cnt, legal = m.counts(*((b, w) if p == 1 else (w, b)))
        if rc:
            raise KeyError((game_id, ply, rc))
        action, greedy, _margin = selfplay_move(cnt, legal, e_greedy, seed, game_id, ply, sample_moves)
        moves.append((b, w, p, action, greedy, fast))
        rows.append(cnt)
        L.orc_game_play(C.byref(black), C.byref(white), n, C.byref(player), C.byref(fin), action)
        ply += 1
    fb, fw = black.value, white.value
    winner = 1 if bin(fb).count("1") >= bin(fw).count("1") else -1         # a draw goes to BLACK
    rec = np.zeros(len(moves), RECORD_DTYPE)
    for i, (b, w, p, action, greedy, fast) in enumerate(moves):
        rec[i] = (b, w, fb, fw, game_id, i, action, p, 1 if winner == p else -1, greedy, (fast, 0, 0))
    return rec, np.array(rows, np.int32).reshape(-1, 64), spent


def episodes(n, sims, cap, e_greedy, seed, first_game_id, games, salt, keep=0, c=1.0, sample_moves=None):
    """`games` games with consecutive ids -> (records, count rows) in ascending (game_id, ply), the sum of all budgets"""
    out = [episode(n, sims, cap, e_greedy, seed, first_game_id + g, salt, keep, c, sample_moves) for g in range(games)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), sum(o[2] for o in out)
