"""Plain restatement of the random openings (include/othellozero_amd.h, oz_rules_random_openings) over the CPU oracle's rules (orc_legal_mask,
orc_game_play) and its counter-based stream (orc_rng, stream 5).  It shares nothing with the kernels but the definition.

Opening `opening_id` of (plies, seed) on the n x n board: from the standard position with BLACK to move, while ply < plies and the game is not
over, the mover orc_game_play left plays the k-th legal square in ascending order, k = rng(seed, opening_id, ply, 5) % (number of legal moves)."""
from minimax_ref import initial_board, kth_bit, legal, play, popcount, rng

RNG_OPENING = 5
MAX_PLIES = 16


def opening(n, plies, seed, opening_id):
    """-> dict(black, white, player, finished: the position reached; actions, players: the squares played and who played them; n_plies;
    passes: plies after which the same side moved again)"""
    (black, white), player, fin = initial_board(n), 1, 0
    actions, players, passes = [], [], 0
    while len(actions) < plies and not fin:
        moves = legal(black, white, player, n)
        sq = kth_bit(moves, rng(seed, opening_id, len(actions), RNG_OPENING) % popcount(moves))
        actions.append(sq)
        players.append(player)
        black, white, mover, fin = play(black, white, player, n, sq)
        passes += (mover == player and not fin)
        player = mover
    return dict(black=black, white=white, player=player, finished=fin, actions=actions, players=players, n_plies=len(actions), passes=passes)


def openings(n, plies, seed, first_opening_id, count):
    return [opening(n, plies, seed, first_opening_id + k) for k in range(count)]
