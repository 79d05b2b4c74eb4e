"""Plain restatement of the fixed-depth minimax opponent (include/othellozero_amd.h, oz_rules_minimax): a recursive negamax without pruning over
the CPU oracle's rules (orc_legal_mask, orc_game_play) and its counter-based stream (orc_rng).  It shares nothing with the kernel's search order.

A position is (black, white, player) with player +1 BLACK / -1 WHITE.  V(P, d), from the viewpoint of P's mover: T(P) if P is finished, else
E(P) if d == 0, else max over legal a of s * V(child(P, a), d - 1), s = +1 where the child's mover is P's mover (the turn passed back), else -1;
a finished child's T is taken from the player orc_game_play leaves in it, with the same s.  Depth counts moves made."""
import ctypes as C
import functools

import oracle

DISCS, WEIGHTED = 0, 1
EVALS = {"discs": DISCS, "weighted": WEIGHTED}
NONE = -2 ** 31
RNG_TIE = 2
WEIGHTS = {(0, 0): 100, (0, 1): -20, (1, 1): -50, (0, 2): 10, (1, 2): -2, (2, 2): 1}


def popcount(x):
    return int(x).bit_count()


def squares(mask):
    """set bits, ascending"""
    m, out = int(mask), []
    while m:
        low = m & -m
        out.append(low.bit_length() - 1)
        m ^= low
    return out


def kth_bit(mask, k):
    return squares(mask)[k]


def weight(n, r, c):
    dr, dc = min(r, n - 1 - r), min(c, n - 1 - c)
    return WEIGHTS[(min(min(dr, dc), 2), min(max(dr, dc), 2))]


@functools.lru_cache(maxsize=None)
def weight_masks(n):
    """[(weight, mask of the n x n board's squares that carry it)]"""
    masks = {}
    for r in range(n):
        for c in range(n):
            masks[weight(n, r, c)] = masks.get(weight(n, r, c), 0) | 1 << (r * 8 + c)
    return sorted(masks.items())


# (the caches only spare repeated calls into the oracle: the same tree is walked once per depth and evaluation)
@functools.lru_cache(maxsize=1 << 17)
def legal(black, white, player, n):
    return int(oracle.lib().orc_legal_mask(black, white, n, 0 if player == 1 else 1))


@functools.lru_cache(maxsize=1 << 17)
def play(black, white, player, n, sq):
    """orc_game_play -> (black, white, player, finished)"""
    b, w, p, f = C.c_uint64(black), C.c_uint64(white), C.c_int(player), C.c_int(0)
    oracle.lib().orc_game_play(C.byref(b), C.byref(w), n, C.byref(p), C.byref(f), sq)
    return int(b.value), int(w.value), int(p.value), int(f.value)


def finished(black, white, n):
    return legal(black, white, 1, n) == 0 and legal(black, white, -1, n) == 0


def static(black, white, player, n, evaluation):
    """E, for `player`"""
    own, opp = (black, white) if player == 1 else (white, black)
    if evaluation == DISCS:
        return popcount(own) - popcount(opp)
    return sum(wt * (popcount(own & m) - popcount(opp & m)) for wt, m in weight_masks(n))


def terminal(black, white, player, evaluation):
    """T, for `player`"""
    own, opp = (black, white) if player == 1 else (white, black)
    return (popcount(own) - popcount(opp)) * (1 if evaluation == DISCS else 1000)


def value(black, white, player, is_finished, n, depth, evaluation, stats=None):
    """V(P, depth) for P = (black, white, player) whose `finished` flag is is_finished"""
    if is_finished:
        return terminal(black, white, player, evaluation)
    if depth == 0:
        return static(black, white, player, n, evaluation)
    best = None
    for sq in squares(legal(black, white, player, n)):
        b, w, p, f = play(black, white, player, n, sq)
        s = 1 if p == player else -1
        if stats is not None and s == 1 and not f:
            stats["passes"] = stats.get("passes", 0) + 1
        v = s * value(b, w, p, f, n, depth - 1, evaluation, stats)
        best = v if best is None or v > best else best
    return best


def root(black, white, player, n, depth, evaluation, stats=None):
    """-> (values[64] by square, NONE off the legal set; bests mask) as oz_rules_minimax defines them"""
    values, moves = [NONE] * 64, 0
    if not finished(black, white, n):
        moves = legal(black, white, player, n)
    for sq in squares(moves):
        b, w, p, f = play(black, white, player, n, sq)
        s = 1 if p == player else -1
        if stats is not None and s == 1 and not f:
            stats["passes"] = stats.get("passes", 0) + 1
        values[sq] = s * value(b, w, p, f, n, depth - 1, evaluation, stats)
    bests = 0
    if moves:
        top = max(values[sq] for sq in squares(moves))
        for sq in squares(moves):
            if values[sq] == top:
                bests |= 1 << sq
    return values, bests


def rng(seed, game_id, ply, stream=RNG_TIE):
    return int(oracle.lib().orc_rng(seed, game_id, ply, stream))


def arena_move(bests, seed, game_id, ply):
    """the move of the arena's minimax side: kth bit of bests by the RNG_TIE draw"""
    return kth_bit(bests, rng(seed, game_id, ply) % popcount(bests))


def random_move(black, white, player, n, seed, game_id, ply):
    """k_arena_random_move: kth legal move by the RNG_TIE draw"""
    moves = legal(black, white, player, n)
    return kth_bit(moves, rng(seed, game_id, ply) % popcount(moves))


def initial_board(n):
    b, w = C.c_uint64(), C.c_uint64()
    oracle.lib().orc_initial_board(n, C.byref(b), C.byref(w))
    return int(b.value), int(w.value)


def playout_positions(n, seed, games):
    """every position (black, white, player) of `games` random playouts, their moves drawn as k_arena_random_move draws them for (seed, game, ply)"""
    out = []
    for g in range(games):
        (black, white), player, fin, ply = initial_board(n), 1, 0, 0
        while not fin:
            out.append((black, white, player))
            black, white, player, fin = play(black, white, player, n, random_move(black, white, player, n, seed, g, ply))
            ply += 1
    return out
