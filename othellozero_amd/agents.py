"""Agents and arena -- drop-in for agents.py:9-84 plus the batched arena (config 5).

`NeuralNetworkOthelloAgent` / `RandomOthelloAgent` / `duel_between_agents` keep the reference's
behaviour (one OthelloMCTS per agent, temperature forced to 0, BLACK = agent_1, a draw goes to BLACK).
`arena_batch` plays many deterministic best-vs-candidate games in lock step on the GPU.
The reference's GreedyOthelloAgent is dead code (undefined names, agents.py:27-41); its intent -- play the move that gains the most discs --
is `MinimaxOthelloAgent(game, depth=1, evaluation="discs")`, and the same fixed-depth minimax plays a colour of `arena_batch` on the device.
"""
import ctypes as C
import logging
import random

import numpy as np

from . import _lib
from .Othello import BoardView, OthelloGame, OthelloPlayer
from .othelo_mcts import OthelloMCTS


class OthelloAgent:
    """agents.py:9-17: an agent is bound to ONE game object and moves on it when asked"""

    def __init__(self, game):
        self.game = game

    def play(self):
        raise NotImplementedError


class RandomOthelloAgent(OthelloAgent):
    def play(self):
        """agents.py:20-24: one `random.choice` over the valid actions in row-major order"""
        moves = tuple(self.game.get_valid_actions())
        self.game.play(*random.choice(moves))


def rules_minimax(black, white, player, n, depth, evaluation="weighted"):
    """oz_rules_minimax over a batch of positions (black, white bitboards, player +1 / -1): -> (values int32 (count, 64) by square row*8+col,
    OZ_MINIMAX_NONE off the legal set; bests uint64 (count,) = the moves of maximal root value, 0 where the mover has none)"""
    depth, code = _lib.check_minimax(depth, evaluation)
    black = np.ascontiguousarray(black, dtype=np.uint64).ravel()
    white = np.ascontiguousarray(white, dtype=np.uint64).ravel()
    player = np.ascontiguousarray(player, dtype=np.int8).ravel()
    k = black.size
    values, bests = np.zeros((k, 64), np.int32), np.zeros(k, np.uint64)
    _lib.check(_lib.require_gpu().oz_rules_minimax(_lib.p_u64(black), _lib.p_u64(white), _lib.p_i8(player), n, k, depth, code,
                                                   _lib.p_i32(values), _lib.p_u64(bests)))
    return values, bests


def rules_solve(black, white, player, n, max_empties=_lib.SOLVE_MAX_EMPTIES):
    """oz_rules_solve, the exact endgame solver, over a batch of positions: -> (values int32 (count, 64) = the final disc difference for the mover
    after each legal move under perfect play, OZ_MINIMAX_NONE elsewhere; bests uint64 (count,) = the moves of maximal value; value int32 (count,) =
    the position's own; solved uint8 (count,) = 0 where the position has more than max_empties empties and was left alone: no values, bests 0,
    value 0)"""
    max_empties = _lib.check_solve_empties(max_empties)
    black = np.ascontiguousarray(black, dtype=np.uint64).ravel()
    white = np.ascontiguousarray(white, dtype=np.uint64).ravel()
    player = np.ascontiguousarray(player, dtype=np.int8).ravel()
    k = black.size
    values, bests, value, solved = np.zeros((k, 64), np.int32), np.zeros(k, np.uint64), np.zeros(k, np.int32), np.zeros(k, np.uint8)
    _lib.check(_lib.require_gpu().oz_rules_solve(_lib.p_u64(black), _lib.p_u64(white), _lib.p_i8(player), n, k, max_empties,
                                                 _lib.p_i32(values), _lib.p_u64(bests), _lib.p_i32(value), _lib.p_u8(solved)))
    return values, bests, value, solved


def rules_solve_sign(black, white, player, n, max_empties=_lib.SOLVE_MAX_EMPTIES):
    """oz_rules_solve_sign over a batch of positions: -> (sign int8 (count,) = -1 / 0 / +1, who wins under perfect play as the mover sees it;
    solved uint8 (count,) = 0 where the position has more than max_empties empties and was left alone: sign 0).  The solver under the window
    (-1, +1): much cheaper than rules_solve, and it says nothing about the moves.  What solve_leaves=E puts into a search's leaves."""
    max_empties = _lib.check_solve_empties(max_empties)
    black = np.ascontiguousarray(black, dtype=np.uint64).ravel()
    white = np.ascontiguousarray(white, dtype=np.uint64).ravel()
    player = np.ascontiguousarray(player, dtype=np.int8).ravel()
    k = black.size
    sign, solved = np.zeros(k, np.int8), np.zeros(k, np.uint8)
    _lib.check(_lib.require_gpu().oz_rules_solve_sign(_lib.p_u64(black), _lib.p_u64(white), _lib.p_i8(player), n, k, max_empties,
                                                      _lib.p_i8(sign), _lib.p_u8(solved)))
    return sign, solved


def rules_backup_values(value_signs, swaps, leaf_value):
    """oz_search_backup_values: what one backup stores, on the host (no GPU needed).  swaps = sigma_d of the descent's edges d = 0 .. depth-1, a
    sequence of 0 / 1 (1: the sides swapped after the edge; 0: the same side moves again, a pass or the end of the game), leaf_value = the leaf's
    value for the side to move there.  -> (values float64 (depth,), what edge d gets; last_value, what OthelloMCTS reports as the simulation's
    value).  value_signs "reference" | "sound" (include/othellozero_amd.h, "value signs")."""
    mode = _lib.check_value_signs(value_signs)
    swaps = [int(bool(b)) for b in swaps]
    depth = len(swaps)
    if depth > 64:
        raise ValueError(f"rules_backup_values: at most 64 levels (got {depth})")
    bits = sum(b << d for d, b in enumerate(swaps))
    out, last = np.zeros(max(depth, 1), np.float64), C.c_double()
    _lib.check(_lib.load().oz_search_backup_values(mode, bits, depth, float(leaf_value), _lib.p_f64(out), C.byref(last)))
    return out[:depth], last.value


def rules_terminal_value(value_signs, own, opp):
    """oz_search_terminal_value: a finished board's value for `own`, the side the descent leaves to move there (bitboards), on the host:
    "sound" the sign of the disc difference (a draw is 0), "reference" +1 unless own has fewer discs (a draw is own's win)."""
    mode = _lib.check_value_signs(value_signs)
    v = C.c_int()
    _lib.check(_lib.load().oz_search_terminal_value(mode, int(own), int(opp), C.byref(v)))
    return v.value


def rules_select_c(c, base, factor, n):
    """oz_search_select_c: the visit-scaled exploration constant of a node with n visits, on the host (no GPU needed):
    c + factor * log(((1.0 + n) + base) / base) with the library's correctly rounded logarithm (include/othellozero_amd.h, "selection")"""
    out = C.c_double()
    _lib.check(_lib.load().oz_search_select_c(float(c), float(base), float(factor), int(n), C.byref(out)))
    return out.value


def rules_select_scores(N, Q, P, legal, Ns, vhat, level, c, selection):
    """oz_search_select_scores: the selection rule at one node, on the host (no GPU needed).  N, Q, P = 64 entries by square as selection sees
    them (the caller's in-flight view and noisy prior), legal = the mask, Ns = the node's visits in that view, vhat = the value its expansion
    backed up, level = its depth in the descent, c = the exploration constant, selection = the keyword's dict (or None).
    -> dict(U float64 (64,) with -inf off the legal set, F, V (0.0 with FPU off), c_S, pick = the first maximum or -1)"""
    flags, f, fr, b, k = _lib.check_selection(selection)
    N = np.ascontiguousarray(N, dtype=np.int32).ravel()
    Q = np.ascontiguousarray(Q, dtype=np.float64).ravel()
    P = np.ascontiguousarray(P, dtype=np.float64).ravel()
    if not (N.size == Q.size == P.size == 64):
        raise ValueError("rules_select_scores: N, Q and P take 64 entries by square")
    U, F, V, cS, pick = np.zeros(64, np.float64), C.c_double(), C.c_double(), C.c_double(), C.c_int32()
    _lib.check(_lib.load().oz_search_select_scores(_lib.p_i32(N), _lib.p_f64(Q), _lib.p_f64(P), int(legal), int(Ns), float(vhat), int(level), float(c),
                                                   flags, f, fr, b, k, _lib.p_f64(U), C.byref(F), C.byref(V), C.byref(cS), C.byref(pick)))
    return dict(U=U, F=F.value, V=V.value, c_S=cS.value, pick=pick.value)


def _proof_masks(edge):
    """edge proofs by square (-1 / 0 / +1, anything else = unknown) -> the two masks (lo, hi) of the library's entry: state = e + 2"""
    lo = hi = 0
    for sq, e in enumerate(edge):
        if int(e) in (-1, 0, 1):
            st = int(e) + 2
            lo |= (st & 1) << sq
            hi |= (st >> 1) << sq
    return lo, hi


def _proof_in(v):
    return _lib.PROOF_UNKNOWN if v is None else int(v)


def _proof_out(v):
    return None if v == _lib.PROOF_UNKNOWN else int(v)


def rules_proof_value(legal, edge, own_value=None):
    """oz_search_proof_value: val(S) of a node, on the host (no GPU needed).  legal = the node's legal mask, edge = 64 proofs by square
    (-1 / 0 / +1, None or _lib.PROOF_UNKNOWN = unknown), own_value = the node's own value or None.  -> -1 / 0 / +1 or None: the own value if
    set; else +1 if a legal edge wins; else the maximum if every legal edge is known (include/othellozero_amd.h, "proofs")."""
    lo, hi = _proof_masks([_proof_in(e) for e in edge])
    v = C.c_int()
    _lib.check(_lib.load().oz_search_proof_value(int(legal), lo, hi, _proof_in(own_value), C.byref(v)))
    return _proof_out(v.value)


def rules_proof_candidates(legal, edge, node_val=None):
    """oz_search_proof_candidates: the edges a descent may take at a node whose val(S) is node_val (None below the root) -> (mask,
    inconsistent): the legal edges proven node_val; else, and where there is none, those not proven lost; none either: the legal set and
    inconsistent = True."""
    lo, hi = _proof_masks([_proof_in(e) for e in edge])
    cand, bad = C.c_uint64(), C.c_int()
    _lib.check(_lib.load().oz_search_proof_candidates(int(legal), lo, hi, _proof_in(node_val), C.byref(cand), C.byref(bad)))
    return cand.value, bool(bad.value)


def rules_proof_backup(path, leaf_value):
    """oz_search_proof_backup: the proof loop of one backup.  path = one dict per level d = 0 .. depth-1 with legal (mask), edge (64 proofs
    by square, None = unknown), own_value (or None), square (the edge taken) and sigma (0 / 1); leaf_value = V_L in -1 / 0 / +1.  -> (edges:
    the levels' proofs after the loop, a list of 64-lists; marked = levels marked from the bottom; fresh = edges newly proven; root = level 0's
    value became known; conflict = a known edge differed)."""
    depth = len(path)
    if depth > 64:
        raise ValueError(f"rules_proof_backup: at most 64 levels (got {depth})")
    k = max(depth, 1)
    sigma, square = np.zeros(k, np.uint8), np.zeros(k, np.int32)
    legal, lo, hi, own = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.full(k, _lib.PROOF_UNKNOWN, np.int8)
    for d, lv in enumerate(path):
        sigma[d], square[d], legal[d], own[d] = int(bool(lv["sigma"])), int(lv["square"]), int(lv["legal"]), _proof_in(lv.get("own_value"))
        lo[d], hi[d] = _proof_masks([_proof_in(e) for e in lv["edge"]])
    out3, conflict = np.zeros(3, np.int32), C.c_int()
    _lib.check(_lib.load().oz_search_proof_backup(_lib.p_u8(sigma), _lib.p_i32(square), depth, int(leaf_value), _lib.p_u64(legal), _lib.p_u64(lo),
                                                  _lib.p_u64(hi), _lib.p_i8(own), _lib.p_i32(out3), C.byref(conflict)))
    edges = []
    for d in range(depth):
        l, h = int(lo[d]), int(hi[d])
        edges.append([(((h >> s) & 1) * 2 + ((l >> s) & 1) - 2) if ((l | h) >> s) & 1 else None for s in range(64)])
    return edges, int(out3[0]), int(out3[1]), bool(out3[2]), bool(conflict.value)


def rules_proof_play(legal, edge, own_value, counts):
    """oz_search_proof_play: what a root's proofs leave of its raw counts, on the host (no GPU needed).  legal = the root's legal mask,
    edge = 64 proofs by square (-1 / 0 / +1, None or _lib.PROOF_UNKNOWN = unknown), own_value = the root's own value or None, counts = its 64
    raw visit counts (0 off the legal set).  -> dict(val: -1 / 0 / +1 or None; keep: the mask of the squares whose counts stay -- the
    candidates of the descent at the root, or the legal set where none of them was visited; row: int32 (64,) the counts on keep, 0
    elsewhere; fallback; inconsistent).  The rule the move kernels apply (include/othellozero_amd.h, "proof play")."""
    e = np.array([_proof_in(None if x is None else x) for x in edge], np.int8)
    cnt = np.ascontiguousarray(counts, dtype=np.int32).ravel()
    if e.size != 64 or cnt.size != 64:
        raise ValueError(f"rules_proof_play: 64 proofs and 64 counts (got {e.size} and {cnt.size})")
    val, keep, row, fall, bad = C.c_int8(), C.c_uint64(), np.zeros(64, np.int32), C.c_int(), C.c_int()
    _lib.check(_lib.load().oz_search_proof_play(int(legal), _lib.p_i8(e), _proof_in(own_value), _lib.p_i32(cnt), C.byref(val), C.byref(keep),
                                                _lib.p_i32(row), C.byref(fall), C.byref(bad)))
    return dict(val=_proof_out(val.value), keep=keep.value, row=row, fallback=bool(fall.value), inconsistent=bool(bad.value))


def rules_prune_counts(N, Q, P, eta, legal, Ns, c, epsilon, k):
    """oz_forced_playouts_prune, policy target pruning over a batch of root rows, on the host (no GPU needed): N int32, Q, P, eta float64
    (count, 64) by square row*8+col, legal uint64 (count,), Ns int32 (count,) = the roots' stored statistics, their noise and visits; c, epsilon =
    the search's exploration constant and the noise's mixing weight, k = the forcing constant (0: the rows come back as they are, 0 off the
    legal set).  -> pruned int32 (count, 64): the rows a search with forced_playouts=k records as policy targets."""
    k = _lib.check_forced_playouts(k, need_noise=False)
    N = np.ascontiguousarray(N, dtype=np.int32).reshape(-1, 64)
    Q, P, eta = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 64) for x in (Q, P, eta))
    legal = np.ascontiguousarray(legal, dtype=np.uint64).ravel()
    Ns = np.ascontiguousarray(Ns, dtype=np.int32).ravel()
    count = N.shape[0]
    if not (Q.shape[0] == P.shape[0] == eta.shape[0] == legal.size == Ns.size == count):
        raise ValueError(f"rules_prune_counts: {count} count rows, {Q.shape[0]} / {P.shape[0]} / {eta.shape[0]} Q / P / eta rows, {legal.size} legal "
                         f"masks, {Ns.size} Ns")
    pruned = np.zeros((count, 64), np.int32)
    _lib.check(_lib.load().oz_forced_playouts_prune(_lib.p_i32(N), _lib.p_f64(Q), _lib.p_f64(P), _lib.p_f64(eta), _lib.p_u64(legal), _lib.p_i32(Ns),
                                                    count, float(c), float(epsilon), k, _lib.p_i32(pruned)))
    return pruned


def rules_root_values(N, Q):
    """oz_root_values: the root value of searches from their root rows, on the host (no GPU needed).  N int32 (..., 64) raw visit counts by
    square, Q float64 (..., 64) the stored edge values -> float64 (...): pairwise_sum(N * Q) / sum(N), the visit-weighted mean of Q for the
    player to move; 0.0 where nothing was visited.  The function the kernels evaluate (include/othellozero_amd.h, "value targets")."""
    n_ = np.ascontiguousarray(N, dtype=np.int32)
    q_ = np.ascontiguousarray(Q, dtype=np.float64)
    if n_.shape != q_.shape or n_.ndim < 1 or n_.shape[-1] != 64:
        raise ValueError(f"N and Q must both have shape (..., 64) (got {n_.shape} and {q_.shape})")
    out = np.zeros(n_.shape[:-1], np.float64)
    _lib.check(_lib.load().oz_root_values(_lib.p_i32(n_), _lib.p_f64(q_), out.size, _lib.p_f64(out)))
    return out


def rules_value_targets(records, values, n, value_target, exact_empties=0, exact_proven=False):
    """oz_value_targets: the value targets of move records (_lib.RECORD_DTYPE, any order; records of one game_id are one game) with their
    root values (float64 (R,)), on the host (no GPU needed) -> float32 (R,), target i for record i.  value_target = "outcome", ("blend", w)
    or ("td", lam); exact_empties=E > 0: a record with at most E empties keeps its z (an exact value of SelfPlayEngine.solve_records(E)) and
    restarts the TD chain.  exact_proven=True: a record with a proof code (_lib.record_proven; after _lib.proof_targets) does the same
    (oz_value_targets_x).  The function k_value_targets evaluates (include/othellozero_amd.h, "value targets")."""
    mode, param = _lib.check_value_target(value_target)
    exact_empties = _lib.check_solve_empties(exact_empties, 0, "exact_empties")
    rec = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE).ravel()
    val = np.ascontiguousarray(values, dtype=np.float64).ravel()
    if val.size != rec.size:
        raise ValueError(f"{val.size} root values for {rec.size} records")
    out = np.zeros(rec.size, np.float32)
    if exact_proven:
        _lib.check(_lib.load().oz_value_targets_x(rec.ctypes.data_as(C.c_void_p), _lib.p_f64(val), rec.size, int(n), mode, param, exact_empties,
                                                  1, _lib.p_f32(out)))
        return out
    _lib.check(_lib.load().oz_value_targets(rec.ctypes.data_as(C.c_void_p), _lib.p_f64(val), rec.size, int(n), mode, param, exact_empties,
                                            _lib.p_f32(out)))
    return out


def rules_resign_scan(players, values, plies_per_game, v, r, min_ply):
    """oz_resign_scan: the first trigger of the resignation rule in each of several games, on the host (no GPU needed).  players int8 (+-1)
    and values float64: the movers and root values of the games' searched moves, one game after the other, ply 0 first; plies_per_game int32
    (games,): how many entries each game has; v, r, min_ply: the rule (the exemption is not looked at here).  -> (trigger_ply
    int32 (games,), trigger_side int8 (games,)): the ply of the first trigger and the side it calls the game for, -1 and 0 where the rule
    never triggers.  The function the move kernels evaluate (include/othellozero_amd.h, "resignation")."""
    v, r, min_ply, _keep = _lib.check_resign((v, r, min_ply, 0.0))
    p_ = np.ascontiguousarray(players, dtype=np.int8).ravel()
    q_ = np.ascontiguousarray(values, dtype=np.float64).ravel()
    n_ = np.ascontiguousarray(plies_per_game, dtype=np.int32).ravel()
    if p_.size != q_.size or (n_ < 0).any() or int(n_.sum(dtype=np.int64)) != p_.size:
        raise ValueError(f"{p_.size} players and {q_.size} values for games of {int(n_.sum(dtype=np.int64))} plies in all")
    ply, side = np.full(n_.size, -1, np.int32), np.zeros(n_.size, np.int8)
    _lib.check(_lib.load().oz_resign_scan(_lib.p_i8(p_), _lib.p_f64(q_), _lib.p_i32(n_), n_.size, v, r, min_ply, _lib.p_i32(ply), _lib.p_i8(side)))
    return ply, side


def rules_resign_exempt(seed, game_ids, keep_prob):
    """oz_resign_exempt on the host (no GPU needed): bool (count,), True where the game with that id is played out regardless of the
    resignation rule under (seed, keep_prob) -- the unit draw of stream (seed, game id, 0, OZ_RNG_RESIGN) is below keep_prob"""
    keep_prob = float(keep_prob)
    if not 0.0 <= keep_prob <= 1.0:
        raise ValueError(f"resign: keep_prob must be in [0, 1] (got {keep_prob})")
    ids = np.ascontiguousarray(game_ids, dtype=np.uint64).ravel()
    out = np.zeros(ids.size, np.uint8)
    _lib.check(_lib.load().oz_resign_exempt(int(seed) & (2 ** 64 - 1), _lib.p_u64(ids), ids.size, keep_prob, _lib.p_u8(out)))
    return out.astype(bool)


def rules_gumbel_considered_visits(m, n):
    """oz_gumbel_considered_visits on the host (no GPU needed): the sequential-halving schedule of a Gumbel root that considers m moves over n
    simulations -> int32 (n,): the visit count the pick of simulation t must match (include/othellozero_amd.h, "Gumbel search")"""
    out = np.zeros(max(int(n), 0), np.int32)
    _lib.check(_lib.load().oz_gumbel_considered_visits(int(m), int(n), _lib.p_i32(out)))
    return out


def rules_gumbel_draws(seed, game_ids, plies, legal):
    """oz_gumbel_draws on the host (no GPU needed): the Gumbel draws of roots from their keys (seed, game id, ply) and legal sets (uint64 masks)
    -> float64 (count, 64) by square row*8+col, 0 off the legal set -- the function k_gumbel_arm evaluates"""
    ids = np.ascontiguousarray(game_ids, dtype=np.uint64).ravel()
    pl = np.ascontiguousarray(plies, dtype=np.int32).ravel()
    lg = np.ascontiguousarray(legal, dtype=np.uint64).ravel()
    if not (ids.size == pl.size == lg.size):
        raise ValueError(f"rules_gumbel_draws: {ids.size} game ids, {pl.size} plies, {lg.size} legal masks")
    g = np.zeros((ids.size, 64), np.float64)
    _lib.check(_lib.load().oz_gumbel_draws(int(seed), _lib.p_u64(ids), _lib.p_i32(pl), _lib.p_u64(lg), ids.size, _lib.p_f64(g)))
    return g


def rules_gumbel_root(N, N0, Q, P, g, legal, vhat, gumbel, budget, with_scores=False):
    """oz_gumbel_root on the host (no GPU needed): the Gumbel root rule over a batch of root rows.  N, N0 int32, Q, P, g float64 (count, 64) by
    square row*8+col, legal uint64 (count,), vhat float64 (count,) = the roots' stored statistics, their snapshots at arming, their draws and own
    values; gumbel = (max_considered, c_visit, c_scale), budget = the simulations of the search.  -> (pick int32 (count,) = the root edge the
    next descent takes, move int32 (count,), pi float32 (count, 64) = the improved policy rows); with_scores=True adds (score float64 (count, 64),
    gaps float64 (count, 2) = best minus second-best score among the candidates of the pick and of the move)."""
    m, c_visit, c_scale = _lib.check_gumbel(gumbel)
    N, N0 = (np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 64) for x in (N, N0))
    Q, P, g = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 64) for x in (Q, P, g))
    legal = np.ascontiguousarray(legal, dtype=np.uint64).ravel()
    vhat = np.ascontiguousarray(vhat, dtype=np.float64).ravel()
    count = N.shape[0]
    if not (N0.shape[0] == Q.shape[0] == P.shape[0] == g.shape[0] == legal.size == vhat.size == count):
        raise ValueError(f"rules_gumbel_root: {count} N rows, {N0.shape[0]} / {Q.shape[0]} / {P.shape[0]} / {g.shape[0]} N0 / Q / P / g rows, "
                         f"{legal.size} legal masks, {vhat.size} values")
    pick, move, pi = np.zeros(count, np.int32), np.zeros(count, np.int32), np.zeros((count, 64), np.float32)
    score, gaps = np.zeros((count, 64), np.float64), np.zeros((count, 2), np.float64)
    _lib.check(_lib.load().oz_gumbel_root(_lib.p_i32(N), _lib.p_i32(N0), _lib.p_f64(Q), _lib.p_f64(P), _lib.p_f64(g), _lib.p_u64(legal),
                                          _lib.p_f64(vhat), count, m, c_visit, c_scale, int(budget), _lib.p_i32(pick), _lib.p_i32(move),
                                          _lib.p_f32(pi), _lib.p_f64(score), _lib.p_f64(gaps)))
    return (pick, move, pi, score, gaps) if with_scores else (pick, move, pi)


def rules_policy_surprise(target, P):
    """oz_policy_surprises on the host (no GPU needed): the surprise s = KL(q || p) of searched moves from their rows by square.  target =
    int32 (..., 64) count rows (the recorded, possibly pruned counts: normalised at T = 1) or float32 (..., 64) policy rows (the improved
    policy of a Gumbel search: widened to float64); P float64 (..., 64) the root's stored priors, 0 off the legal set -> float64 (...).
    The function the move kernels evaluate (include/othellozero_amd.h, "policy surprise weighting")."""
    t = np.asarray(target)
    p_ = np.ascontiguousarray(P, dtype=np.float64)
    if t.shape != p_.shape or t.ndim < 1 or t.shape[-1] != 64:
        raise ValueError(f"target and P must both have shape (..., 64) (got {t.shape} and {p_.shape})")
    out = np.zeros(t.shape[:-1], np.float64)
    if np.issubdtype(t.dtype, np.integer):
        t = np.ascontiguousarray(t, dtype=np.int32)
        _lib.check(_lib.load().oz_policy_surprises(_lib.p_i32(t), _lib.p_f64(p_), out.size, _lib.p_f64(out)))
    elif t.dtype == np.float32:
        t = np.ascontiguousarray(t)
        _lib.check(_lib.load().oz_policy_surprises_f32(_lib.p_f32(t), _lib.p_f64(p_), out.size, _lib.p_f64(out)))
    else:
        raise ValueError(f"target must be int32 count rows or float32 policy rows (got dtype {t.dtype})")
    return out


def rules_surprise_weights(records, surprises, frac):
    """oz_surprise_weights on the host (no GPU needed): the float32 weights (R,) of move records (_lib.RECORD_DTYPE, any order; records of one
    game_id are one game) from their surprises (float64 (R,)): (1 - frac) + frac s K / S over the game's K fully searched records, 1 where
    their surprises sum to 0, 0 for a fast record.  The function k_surprise_weights evaluates."""
    frac = _lib.check_surprise_frac(frac, "rules_surprise_weights")
    rec = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE).ravel()
    sur = np.ascontiguousarray(surprises, dtype=np.float64).ravel()
    if sur.size != rec.size:
        raise ValueError(f"{sur.size} surprises for {rec.size} records")
    w = np.zeros(rec.size, np.float32)
    _lib.check(_lib.load().oz_surprise_weights(rec.ctypes.data_as(C.c_void_p), _lib.p_f64(sur), rec.size, frac, _lib.p_f32(w)))
    return w


def rules_surprise_copies(records, weights, seed):
    """oz_surprise_copies on the host (no GPU needed): (copies int32 (R,), first_sym uint8 (R,)) of move records from their float32 weights:
    floor(8 w + u) examples, the first of them symmetry d & 7, d the draw of (seed, game id, ply).  The function k_surprise_weights evaluates."""
    rec = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE).ravel()
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if w.size != rec.size:
        raise ValueError(f"{w.size} weights for {rec.size} records")
    c, t0 = np.zeros(rec.size, np.int32), np.zeros(rec.size, np.uint8)
    _lib.check(_lib.load().oz_surprise_copies(rec.ctypes.data_as(C.c_void_p), _lib.p_f32(w), rec.size, int(seed) & (2 ** 64 - 1), _lib.p_i32(c), _lib.p_u8(t0)))
    return c, t0


def rules_eval_symmetries(own, opp, seed):
    """oz_eval_symmetries on the host (no GPU needed): the orientation t in 0..7 (int32) a network set to ("random", seed) evaluates each
    mover-canonical position (own[i], opp[i]) in -- the function the kernels evaluate"""
    _, seed = _lib.check_eval_symmetry("random", seed)
    own = np.ascontiguousarray(own, dtype=np.uint64).ravel()
    opp = np.ascontiguousarray(opp, dtype=np.uint64).ravel()
    if own.size != opp.size:
        raise ValueError(f"rules_eval_symmetries: {own.size} own boards, {opp.size} opp boards")
    t = np.zeros(own.size, np.int32)
    _lib.check(_lib.load().oz_eval_symmetries(seed, _lib.p_u64(own), _lib.p_u64(opp), own.size, _lib.p_i32(t)))
    return t


def rules_sym_boards(boards, n, t):
    """oz_sym_boards on the host (no GPU needed): the bitboards `boards` of an n x n board in orientation t (one number, or one per board;
    the numbering of the training symmetries, 7 = the identity) -> uint64, same shape"""
    b = np.ascontiguousarray(boards, dtype=np.uint64)
    tt = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.int32), b.shape)).ravel()
    out = np.zeros(b.size, np.uint64)
    _lib.check(_lib.load().oz_sym_boards(_lib.p_i32(tt), int(n), _lib.p_u64(b.ravel()), b.size, _lib.p_u64(out)))
    return out.reshape(b.shape)


def rules_aux_targets(records):
    """oz_aux_targets on the host (no GPU needed): (fin_own, fin_opp) uint64 (R,) of move records (_lib.RECORD_DTYPE) -- the game's final board
    from the mover's side, the target of the trainer's auxiliary heads; 0 / 0 ("no auxiliary target") for a record of an adjudicated game and
    for a fast record of a playout cap.  The function the replay buffer's append kernels evaluate."""
    rec = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE).ravel()
    fo, fp = np.zeros(rec.size, np.uint64), np.zeros(rec.size, np.uint64)
    _lib.check(_lib.load().oz_aux_targets(rec.ctypes.data_as(C.c_void_p), rec.size, _lib.p_u64(fo), _lib.p_u64(fp)))
    return fo, fp


def rules_random_openings(n, count, plies, seed, first_opening_id=0):
    """oz_rules_random_openings: the random openings first_opening_id .. first_opening_id + count - 1 of (plies, seed) on the n x n board, what
    arena_batch(openings=(plies, seed), first_opening_id=...) lets its games start with.  -> dict(black, white uint64 (count,) = the position
    reached, player int8 (+1 BLACK / -1 WHITE to move), finished uint8 (the game ended inside the opening), actions uint8 (count, 16) = the
    squares played, row*8+col, 0 beyond n_plies, n_plies int32 (count,)).  (actions, n_plies) is what opening_moves= takes."""
    plies = _lib.check_opening_plies(plies, "rules_random_openings")
    if not _lib._whole(count, 0, 1 << 22):
        raise ValueError(f"rules_random_openings: count must be a whole number in 0..2^22 (got {count!r})")
    for what, x in (("seed", seed), ("first_opening_id", first_opening_id)):
        if not _lib._whole(x, 0, 2 ** 64 - 1):
            raise ValueError(f"rules_random_openings: {what} must be a whole number in 0..2^64 - 1 (got {x!r})")
    k = int(count)
    black, white, player, finished = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.int8), np.zeros(k, np.uint8)
    actions, n_plies = np.zeros((k, _lib.OPENING_MAX_PLIES), np.uint8), np.zeros(k, np.int32)
    _lib.check(_lib.require_gpu().oz_rules_random_openings(n, k, plies, int(seed), int(first_opening_id), _lib.p_u64(black), _lib.p_u64(white),
                                                           _lib.p_i8(player), _lib.p_u8(finished), _lib.p_u8(actions), _lib.p_i32(n_plies)))
    return dict(black=black, white=white, player=player, finished=finished, actions=actions, n_plies=n_plies)


class MinimaxOthelloAgent(OthelloAgent):
    """Fixed-depth minimax on the device (oz_rules_minimax): what the reference's GreedyOthelloAgent (agents.py:27-41, dead code) was meant to
    be at depth=1, evaluation="discs", and harder by one integer.  One call for the game's position, then `random.choice` over the moves of
    maximal root value in ascending row-major order (Python's own `random`, like RandomOthelloAgent).
    solve_empties=E > 0: a position with E empties or fewer is played perfectly -- the same `random.choice`, over the exact solver's best
    moves (oz_rules_solve).  The default 0 never asks the solver."""

    def __init__(self, game, depth=3, evaluation="weighted", solve_empties=0):
        _lib.check_minimax(depth, evaluation)
        solve_empties = _lib.check_solve_empties(solve_empties, 0, "solve_empties")
        super().__init__(game)
        self.depth, self.evaluation, self.solve_empties = int(depth), evaluation, solve_empties

    def play(self):
        game = self.game
        black, white = _lib.pack_board(game.board(BoardView.TWO_CHANNELS))
        if self.solve_empties > 0 and game.board_size ** 2 - bin(black | white).count("1") <= self.solve_empties:
            _, bests, _, _ = rules_solve([black], [white], [game.current_player.value], game.board_size, self.solve_empties)
        else:
            _, bests = rules_minimax([black], [white], [game.current_player.value], game.board_size, self.depth, self.evaluation)
        mask = int(bests[0])
        moves = tuple((s >> 3, s & 7) for s in range(64) if (mask >> s) & 1)
        game.play(*random.choice(moves))


class NeuralNetworkOthelloAgent(OthelloAgent):
    """agents.py:44-68: a private OthelloMCTS per agent (its table persists over the game), `num_simulations`
    simulations before every move, the temperature argument ignored and forced to 0 (agents.py:46), the move =
    the first valid action with the largest policy entry."""

    def __init__(self, game, neural_network, num_simulations, degree_exploration, temperature=0,
                 q_mode=_lib.QMODE_F64, leaves_per_step=1, solve_leaves=0, value_signs="reference", proofs=False, proof_play=False,
                 selection=None, tree_gc="off", node_cap=0):
        """proof_play=True (needs proofs=True): the move is the arg-max of the row the root's proofs keep (OthelloMCTS.proven_counts)
        selection: the selection rule of the agent's search (OthelloMCTS, selection)
        tree_gc: the agent's search drops the nodes the game has passed (OthelloMCTS, tree_gc); node_cap > 0: its capacity in place of the default"""
        _lib.check_tree_gc(tree_gc)
        solve_leaves = _lib.check_solve_leaves(solve_leaves)
        _lib.check_selection(selection)
        _lib.check_value_signs(value_signs)
        _lib.check_proofs(proofs, value_signs)
        self.proof_play = _lib.check_proof_play(proof_play, proofs)
        super().__init__(game)
        self.neural_network, self.num_simulations, self.temperature = neural_network, num_simulations, 0
        side = game.board_size
        # an agent searches on its own turns only: about half the plies
        self.mcts = OthelloMCTS(side, neural_network, degree_exploration, q_mode=q_mode,
                                node_cap=int(node_cap) if node_cap else num_simulations * (side * side // 2) + 64, leaves_per_step=leaves_per_step,
                                solve_leaves=solve_leaves, value_signs=value_signs,
                                **_lib.search_kw(dict(proofs=proofs, proof_play=self.proof_play, selection=selection, tree_gc=tree_gc)))

    def play(self):
        game = self.game
        mover = game.current_player
        board = game.board(BoardView.TWO_CHANNELS)
        self.mcts.simulate_n(board, mover, self.num_simulations)
        canonical = board if mover == OthelloPlayer.BLACK else OthelloGame.invert_board(board)
        policy = self.mcts.get_policy_action_probabilities(canonical, self.temperature, **({"proven": True} if self.proof_play else {}))
        best = None
        for action in game.get_valid_actions():               # max() keeps the FIRST maximum: strict '>' below
            if best is None or policy[tuple(action)] > policy[tuple(best)]:
                best = action
        game.play(*best)


def duel_between_agents(game, agent_1, agent_2):
    """agents.py:71-84: agent_1 moves for BLACK, agent_2 for WHITE, until the game is over.
    -> (winning agent, its points); a draw goes to BLACK's agent (get_winning_player)."""
    by_colour = {OthelloPlayer.BLACK: agent_1, OthelloPlayer.WHITE: agent_2}
    logging.info('Duel - Started')
    while not game.has_finished():
        logging.info(f'Duel - Round: {game.round}')
        by_colour[game.current_player].play()
    colour, points = game.get_winning_player()
    return by_colour[colour], points


def arena_batch(net_a, net_b, board_size=8, num_games=512, num_simulations=800, degree_exploration=1.0, seed=0,
                first_game_id=0, q_mode=_lib.QMODE_F64, node_cap=0, max_rounds=0, dedup=True, profile=False, eval_cache=False,
                leaves_per_step=1, opponent=None, solve_leaves=0, openings=None, first_opening_id=0, opening_moves=None,
                value_signs="reference", proofs=False, proof_play=False, selection=None, tree_gc="off"):
    """num_games games of net_a (BLACK) vs net_b (WHITE), temperature 0, max-visit ties broken by the RNG_TIE
    stream keyed (seed, game id, ply).  One of the two may be None: RandomOthelloAgent plays that colour, or with
    opponent=("minimax", depth) / ("minimax", depth, "discs" | "weighted") the fixed-depth minimax (oz_arena_set_opponent; ties between its
    best moves drawn from the same RNG_TIE stream); opponent=None / "random" is the random mover.  Both may be None (no network at all: a
    yardstick for the opponents themselves): then opponent={"black": ..., "white": ...} says who plays which, a missing key the random mover.
    With profile=True the result then carries opponent_kernel = (ms, launches) of the minimax move kernel.
    max_rounds > 0 stops after that many plies per game (unfinished boards: winner / points then describe the position reached).
    Returns dict(winner (+1 = BLACK's agent), points, n_moves, actions, players, final boards, stats_black / stats_white =
    the two agents' search counters [simulations, node visits, expansions, terminal hits, fallbacks], leaves_evaluated = positions the
    networks evaluated: fewer than the expansions with dedup=True (the default), where a board several games reach in one step is evaluated once;
    tree_kernels = {slot: (ms, launches)} of both searches' tree kernels with profile=True, else None).
    leaves_per_step = k or (k_black, k_white): descents per game and network batch of the two agents' searches under virtual loss
    (oz_arena_set_leaves_per_step); an agent's network needs max_batch >= num_games * its k.
    solve_leaves = E or (E_black, E_white): the agent's search takes the exact win / draw / loss of a leaf with at most E empties in place of
    its network's value (oz_arena_set_solve_leaves; 0 = off); the result then carries rows_solved = (black, white).
    value_signs = "reference" | "sound" or (black, white): the rule by which the agent's search backs its values up (oz_arena_set_value_signs;
    OthelloMCTS, value_signs).
    proofs = True | False or (black, white): the agent's search keeps exact values as proofs and backs them up the tree (oz_arena_set_proofs;
    OthelloMCTS, proofs); an agent with proofs needs value_signs "sound".  The moves read the raw counts as before.
    proof_play = True | False or (black, white): the agent's move is the arg-max -- ties as ever -- of the row its root's proofs keep
    (oz_arena_set_proof_play; include/othellozero_amd.h, "proof play"); needs that agent's proofs.
    selection = None | dict(fpu=, cpuct_growth=, prior_first=) or (black, white): the selection rule of the agent's search
    (oz_arena_set_selection; OthelloMCTS, selection); an agent without a network searches nothing.
    tree_gc = "off" | "demand" | "every" or (black, white): the agent's search drops the stored nodes its games have passed, right after its
    roots are set (oz_arena_set_tree_gc; include/othellozero_amd.h, "tree collection"); no result changes, a smaller node_cap suffices.  The
    result then carries tree_gc_stats = (black, white), each dict(collections, nodes_before_sum, nodes_kept_sum, peak_nodes, peak_kept).
    openings = (plies, opening_seed): every game first plays a random opening of `plies` plies (at most 16) without any search
    (oz_arena_set_openings, rules_random_openings); game slot g plays opening first_opening_id + g whatever seed and first_game_id are, so two
    arenas given the same (openings, first_opening_id) start from the same positions.  opening_moves = (moves uint8 (num_games, 16), n_plies int32
    (num_games,)): game g plays that list instead (oz_arena_set_opening_moves; an illegal move is an OzError naming game and ply).  The opening
    plies are part of actions / players / n_moves; the result then carries opening_plies int32 (num_games,) = how many each game played (fewer
    than asked for where the game ended first)."""
    opening = _lib.check_openings(openings, first_opening_id, opening_moves, num_games)
    eb_, ew_ = _lib.check_solve_leaves_pair(solve_leaves)
    vb_, vw_ = _lib.check_value_signs_pair(value_signs)
    pb_, pw_ = _lib.check_proofs_pair(proofs, value_signs)
    ppb_, ppw_ = _lib.check_proof_play_pair(proof_play, (pb_, pw_))
    sel_pair = _lib.check_selection_pair(selection)
    gc_pair = _lib.check_tree_gc_pair(tree_gc)
    kb, kw = (leaves_per_step, leaves_per_step) if np.isscalar(leaves_per_step) else leaves_per_step
    minimax = _lib.check_opponents(opponent, net_a is None, net_b is None)
    lib = _lib.require_gpu()
    h = C.c_void_p()
    _lib.check(lib.oz_arena_create(C.byref(h), board_size, num_games, num_simulations, float(degree_exploration), q_mode,
                                   seed, first_game_id, net_a._h if net_a is not None else None,
                                   net_b._h if net_b is not None else None, node_cap))
    try:
        if not dedup:                                        # every expansion evaluated by itself (identical results; bench.py's config5 headline)
            _lib.check(lib.oz_arena_set_dedup(h, 0))
        if eval_cache:                                       # leaves looked up in / inserted into the two networks' evaluation caches (net.set_eval_cache first)
            _lib.check(lib.oz_arena_set_eval_cache(h, 1))
        if not (np.isscalar(leaves_per_step) and leaves_per_step == 1):
            _lib.check(lib.oz_arena_set_leaves_per_step(h, int(kb), int(kw)))
        if not (np.isscalar(solve_leaves) and solve_leaves == 0):
            _lib.check(lib.oz_arena_set_solve_leaves(h, eb_, ew_))
        if vb_ or vw_:
            _lib.check(lib.oz_arena_set_value_signs(h, vb_, vw_))
        if pb_ or pw_:
            _lib.check(lib.oz_arena_set_proofs(h, int(pb_), int(pw_)))
        if ppb_ or ppw_:
            _lib.check(lib.oz_arena_set_proof_play(h, int(ppb_), int(ppw_)))
        for side, sel in zip((1, -1), sel_pair):
            if sel[0]:
                _lib.check(lib.oz_arena_set_selection(h, side, *sel))
        for side, net, mode in zip((1, -1), (net_a, net_b), gc_pair):
            if mode and net is not None:
                _lib.check(lib.oz_arena_set_tree_gc(h, side, mode))
        if opening is not None and opening[0] == "random":
            _lib.check(lib.oz_arena_set_openings(h, opening[1], opening[2], opening[3]))
        elif opening is not None:
            _lib.check(lib.oz_arena_set_opening_moves(h, _lib.p_u8(opening[1]), _lib.p_i32(opening[2])))
        for side, spec in zip((1, -1), minimax):             # a colour without a network
            if spec is not None:
                _lib.check(lib.oz_arena_set_opponent(h, side, _lib.AGENT_MINIMAX, spec[0], spec[1]))
        if profile:                                          # HIP events around the tree kernels of both searches (bench.py's config5 kernels[])
            _lib.check(lib.oz_arena_profile(h, 1))
        _lib.check(lib.oz_arena_run_rounds(h, int(max_rounds)))
        rows = None
        if not (np.isscalar(solve_leaves) and solve_leaves == 0):
            rb, rw = C.c_int64(), C.c_int64()
            _lib.check(lib.oz_arena_get_solve_leaves(h, C.byref(rb), C.byref(rw)))
            rows = (rb.value, rw.value)
        gc_stats = None
        if any(gc_pair):
            gc_stats = []
            for side in (1, -1):
                st = _lib.TreeGcStats()
                _lib.check(lib.oz_arena_get_tree_gc(h, side, None, C.byref(st)))
                gc_stats.append(_lib.tree_gc_stats_dict(st))
            gc_stats = tuple(gc_stats)
        tree = opp_kernel = None
        if profile and any(minimax):
            ms1, cnt1 = C.c_double(), C.c_int64()
            _lib.check(lib.oz_arena_opponent_time(h, C.byref(ms1), C.byref(cnt1)))
            opp_kernel = (ms1.value, cnt1.value)
        if profile:
            ms, cnt = np.zeros(len(_lib.TREE_KERNELS), np.float64), np.zeros(len(_lib.TREE_KERNELS), np.int64)
            _lib.check(lib.oz_arena_profile_read(h, _lib.p_f64(ms), _lib.p_i64(cnt), 0))
            tree = {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(_lib.TREE_KERNELS)}
        G = num_games
        sa, sb = np.zeros(5, np.int64), np.zeros(5, np.int64)
        _lib.check(lib.oz_arena_stats(h, _lib.p_i64(sa), _lib.p_i64(sb)))
        ea, eb = C.c_int64(), C.c_int64()
        _lib.check(lib.oz_arena_leaves_evaluated(h, C.byref(ea), C.byref(eb)))
        opening_plies = None
        if opening is not None:
            opening_plies = np.zeros(G, np.int32)
            _lib.check(lib.oz_arena_opening_plies(h, _lib.p_i32(opening_plies)))
        winner, points, nm = np.zeros(G, np.int8), np.zeros(G, np.int32), np.zeros(G, np.int32)
        acts, pls = np.zeros((G, 128), np.uint8), np.zeros((G, 128), np.int8)
        fb, fw = np.zeros(G, np.uint64), np.zeros(G, np.uint64)
        _lib.check(lib.oz_arena_results(h, _lib.p_i8(winner), _lib.p_i32(points), _lib.p_i32(nm), _lib.p_u8(acts),
                                        _lib.p_i8(pls), _lib.p_u64(fb), _lib.p_u64(fw)))
    finally:
        lib.oz_arena_destroy(h)
    return dict(winner=winner, points=points, n_moves=nm, actions=acts, players=pls, final_black=fb, final_white=fw,
                stats_black=sa, stats_white=sb, leaves_evaluated=ea.value + eb.value, tree_kernels=tree,
                **({"opponent_kernel": opp_kernel} if any(minimax) else {}), **({"rows_solved": rows} if rows is not None else {}),
                **({"opening_plies": opening_plies} if opening is not None else {}),
                **({"tree_gc_stats": gc_stats} if gc_stats is not None else {}))
