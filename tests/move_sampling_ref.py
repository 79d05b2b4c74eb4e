"""Restatement of move sampling (include/othellozero_amd.h, "move sampling") in plain Python floats over the oracle's stream primitive: the
move drawn in proportion to N ** (1 / T) from a root's visit counts, and the self-play move rule around it (coin, explore, arg-max).  Device and
host pow may differ by ulps, and a draw can only flip where r sits that close to a boundary of the cumulative sum: every draw comes back with
its margin = min over the legal squares of |cum[sq] - r| / c_total, and the tests leave out the (about 1 in 1e7) draws below 1e-9."""
import math

import oracle

RNG_COIN, RNG_EXPLORE, RNG_SAMPLE = 0, 1, 4
UNIT = 1.0 / 9007199254740992.0


def unit(seed, game_id, ply, stream):
    return float(int(oracle.lib().orc_rng(seed, game_id, ply, stream)) >> 11) * UNIT


def squares_of(legal):
    return [s for s in range(64) if (int(legal) >> s) & 1]


def sample_with(counts, legal, temperature, u):
    """counts: 64 visit counts by square row*8+col (at least one legal square visited), u: the unit draw -> (action, margin)"""
    squares = squares_of(legal)
    mx = max(int(counts[s]) for s in squares)
    assert mx >= 1
    inv = 1.0 / temperature
    w, cum, c = {}, {}, 0.0
    for s in squares:                                      # ascending: the order of the additions is part of the definition
        w[s] = 0.0 if int(counts[s]) == 0 else math.pow(float(int(counts[s])) / float(mx), inv)
        c = c + w[s]
        cum[s] = c
    r = u * c
    action = next((s for s in squares if cum[s] > r), None)
    if action is None:                                     # u * c rounded up to c
        action = max(s for s in squares if w[s] > 0.0)
    return action, min(abs(cum[s] - r) for s in squares) / c


def sample(counts, legal, temperature, seed, game_id, ply):
    return sample_with(counts, legal, temperature, unit(seed, game_id, ply, RNG_SAMPLE))


def selfplay_move(counts, legal, e_greedy, seed, game_id, ply, sample_moves=None):
    """the engine's move rule at policy temperature != 0 -> (action, greedy, margin): the coin first; explore = the (draw % count)-th legal
    square; greedy = the first maximum of the counts, or for ply < plies the sampled move (greedy 2)"""
    squares = squares_of(legal)
    if not unit(seed, game_id, ply, RNG_COIN) <= e_greedy:
        return squares[int(oracle.lib().orc_rng(seed, game_id, ply, RNG_EXPLORE)) % len(squares)], 0, math.inf
    if sample_moves is not None and ply < sample_moves[1]:
        action, margin = sample(counts, legal, sample_moves[0], seed, game_id, ply)
        return action, 2, margin
    mx = max(int(counts[s]) for s in squares)
    return next(s for s in squares if int(counts[s]) == mx), 1, math.inf
