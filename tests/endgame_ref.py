"""Plain restatement of the exact endgame solver (include/othellozero_amd.h, oz_rules_solve / oz_selfplay_solve_records): a memoised negamax
without pruning over the CPU oracle's rules, built on minimax_ref.legal / play.  It shares nothing with the kernel's search order.

S(P), from the viewpoint of P's mover: own discs - opponent discs if P is finished, else max over legal a of s * S(child(P, a)), s = +1 where
the child's mover is P's mover (the turn passed back), else -1; a finished child's difference is taken for the player orc_game_play leaves in
it, with the same s.  Empties are not awarded."""
import functools

import minimax_ref as ref

NONE = ref.NONE
MAX_EMPTIES = 12


def empties(black, white, n):
    return n * n - ref.popcount(black | white)


def disc_difference(black, white, player):
    d = ref.popcount(black) - ref.popcount(white)
    return d if player == 1 else -d


@functools.lru_cache(maxsize=None)
def _walk(black, white, player, is_finished, n):
    """-> (S, the tree below holds a pass, a game in it ends before the board is full)"""
    if is_finished:
        return disc_difference(black, white, player), False, empties(black, white, n) > 0
    best, passes, early = None, False, False
    for sq in ref.squares(ref.legal(black, white, player, n)):
        b, w, p, f = ref.play(black, white, player, n, sq)
        s = 1 if p == player else -1
        v, cp, ce = _walk(b, w, p, f, n)
        passes |= cp or (s == 1 and not f)
        early |= ce
        best = s * v if best is None or s * v > best else best
    return best, passes, early


def after_pass(black, white, player, n):
    """the position to solve: the mover of a position that is not finished but has no move passes"""
    if not ref.finished(black, white, n) and ref.legal(black, white, player, n) == 0:
        return black, white, -player, -1
    return black, white, player, 1


def value(black, white, player, n):
    """S of any position; that of the position after the pass, seen by `player`, where `player` has no move"""
    b, w, p, sign = after_pass(black, white, player, n)
    return sign * _walk(b, w, p, int(ref.finished(b, w, n)), n)[0]


def facts(black, white, player, n):
    """(the tree holds a pass, a game in it ends before the board is full)"""
    return _walk(black, white, player, int(ref.finished(black, white, n)), n)[1:]


def root(black, white, player, n):
    """-> (values[64] by square, NONE off the legal set; bests mask; S) as oz_rules_solve defines them"""
    values, moves = [NONE] * 64, 0
    if not ref.finished(black, white, n):
        moves = ref.legal(black, white, player, n)
    for sq in ref.squares(moves):
        b, w, p, f = ref.play(black, white, player, n, sq)
        values[sq] = (1 if p == player else -1) * _walk(b, w, p, f, n)[0]
    bests = 0
    if moves:
        top = max(values[sq] for sq in ref.squares(moves))
        for sq in ref.squares(moves):
            if values[sq] == top:
                bests |= 1 << sq
    return values, bests, value(black, white, player, n)


def z_of(s, player):
    """the value target of a record whose position has the exact value s for its mover `player`: a draw goes to BLACK"""
    return 1 if s > 0 else -1 if s < 0 else 1 if player == 1 else -1


def relabel(records, n, max_empties):
    """oz_selfplay_solve_records over a structured array of records (_lib.RECORD_DTYPE): -> (z per record, stats dict)"""
    z, stats = [], dict(records=len(records), solved=0, z_changed=0, optimal_moves=0, disc_loss_sum=0, disc_loss_max=0)
    for r in records:
        black, white, player = int(r["black"]), int(r["white"]), int(r["player"])
        if empties(black, white, n) > max_empties:
            z.append(int(r["z"]))
            continue
        values, _, s = root(black, white, player, n)
        loss = s - values[int(r["action"])]
        assert loss >= 0
        z.append(z_of(s, player))
        stats["solved"] += 1
        stats["z_changed"] += z[-1] != int(r["z"])
        stats["optimal_moves"] += loss == 0
        stats["disc_loss_sum"] += loss
        stats["disc_loss_max"] = max(stats["disc_loss_max"], loss)
    return z, stats
