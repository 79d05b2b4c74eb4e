"""Restatement of the value signs of the backup (include/othellozero_amd.h, "value signs") in plain Python over tests/wide_search_ref.py.

A descent takes the edges 0 .. depth-1; sigma_d = 1 where the sides swapped after edge d, 0 where the same side moves again (a pass, or the
game is over).  V_L = the leaf's value for the side to move there.  "sound": edge d gets V_L * (-1)^(sigma_d + .. + sigma_{depth-1}) and a
finished board is worth sign(discs own - discs opp); "reference": edge d gets V_L * (-1)^(depth - d) and a finished board is worth +1 to own
unless it has fewer discs.  last_value = minus what edge 0 got (-V_L at depth 0).  SoundSearch in reference mode must be WideSearch bit for
bit (tests/test_value_signs_cpu.py asserts it); in sound mode the GPU tests hold the kernels against it."""
import math

import numpy as np

import move_sampling_ref as ms
import oracle
from wide_search_ref import WideSearch, apply_move, initial_board, legal_mask, popcount, tie_draw

MODES = ("reference", "sound")
# 6x6 positions with 8 empties (value_signs_ref.random_position(6, 8, seed) for seed 0, 2, 7, 23), picked by the restatement's counters at 60
# simulations of stub salt 7: finished leaves of value +1, 0 and -1, leaves backed up across a pass, and root counts that differ between modes
POSITIONS_6 = ((0x51f0d1d0f09, 0x282022222000), (0x1c1c24001c02, 0x20010b3d2325), (0x30200000023f, 0x81e3e1e1d00), (0x201138343e3f, 0x70604090000))


def terminal_value(mode, own, opp):
    a, b = popcount(own), popcount(opp)
    if mode == "sound":
        return (a > b) - (a < b)
    return 1 if a >= b else -1


def backup_values(mode, sigma, leaf):
    """-> ([value of edge d], last_value); sigma: the 0 / 1 list of the descent; leaf: V_L.  Negations only."""
    depth = len(sigma)
    out = []
    for d in range(depth):
        flips = sum(sigma[d:]) if mode == "sound" else depth - d
        out.append(-leaf if flips & 1 else leaf)
    return out, -(out[0] if depth else leaf)


class SoundSearch(WideSearch):
    """WideSearch whose descents record sigma and whose backup is backup_values(mode, ...).  A path entry is (node, square, sigma): the
    in-flight view of WideSearch reads the first two.  set_noise: the root noise of tests/root_noise_ref.py (Pn at depth 0 of that root).
    Counters: pass_backups = evaluated leaves backed up across a pass (a 0 among their sigma), term[v] = finished leaves of value v."""

    def __init__(self, n, c, K, salt=0, keep_mask=0, evaluator=None, mode="sound"):
        assert mode in MODES, mode
        super().__init__(n, c, K, salt=salt, keep_mask=keep_mask, evaluator=evaluator)
        self.mode = mode
        self.noise = None
        self.pass_backups = 0
        self.term = {-1: 0, 0: 0, 1: 0}

    def set_noise(self, own, opp, eta, eps):
        self.noise = (own, opp, float(eps), [float(x) for x in eta]) if eps > 0 else None

    def _descend(self, own, opp, inflight):
        n = self.n
        nz = self.noise if self.noise is not None and (self.noise[0], self.noise[1]) == (own, opp) else None
        path = []
        lg = legal_mask(own, opp, n)
        while True:
            if lg == 0 and legal_mask(opp, own, n) == 0:
                return path, ("term", terminal_value(self.mode, own, opp))
            idx = self.index.get((own, opp))
            if idx is None:
                return path, ("leaf", own, opp, lg)
            nd = self.nodes[idx]
            d = len(path)
            ks, ke = 0, {}
            for p, _ in inflight:
                if len(p) > d and p[d][0] == idx:
                    ks += 1
                    ke[p[d][1]] = ke.get(p[d][1], 0) + 1
            best, bu = -1, 0.0
            for sq in nd.acts:
                N, Q, P = nd.N[sq], nd.Q[sq], nd.P[sq]
                k = ke.get(sq, 0)
                if k:
                    Q = (float(N) * Q - float(k)) / float(N + k)
                    N = N + k
                if nz is not None and d == 0:
                    P = (1.0 - nz[2]) * P + nz[2] * nz[3][sq]
                u = Q + (self.c * P) * (math.sqrt(float(nd.Ns + ks)) / float(1 + N))
                if best < 0 or u > bu:
                    best, bu = sq, u
            own, opp = apply_move(own, opp, n, best)
            theirs = legal_mask(opp, own, n)
            path.append((idx, best, 1 if theirs else 0))
            if theirs:
                own, opp, lg = opp, own, theirs
            else:
                lg = legal_mask(own, opp, n)

    def step(self, own, opp, budget):
        inflight = []
        for _ in range(min(self.K, budget)):
            path, res = self._descend(own, opp, inflight)
            if res[0] == "leaf" and any(r[0] == "leaf" and r[1] == res[1] and r[2] == res[2] for _, r in inflight):
                self.collisions += 1
                break
            inflight.append((path, res))
        for path, res in inflight:
            sigma = [e[2] for e in path]
            if res[0] == "leaf":
                leaf = -self._expand(res[1], res[2], res[3])           # (_expand returns the reference's -v)
                self.leaves += 1
                self.pass_backups += 0 in sigma
            else:
                leaf = float(res[1])
                self.terminals += 1
                self.term[res[1]] += 1
            vals, self.last_value = backup_values(self.mode, sigma, leaf)
            for (idx, sq, _), val in zip(path, vals):
                nd = self.nodes[idx]
                nd.Q[sq] = (float(nd.N[sq]) * nd.Q[sq] + val) / float(nd.N[sq] + 1)
                nd.N[sq] += 1
                nd.Ns += 1
        self.steps += 1
        self.sims += len(inflight)
        return len(inflight)

    def root_value(self, own, opp):
        """the visit-weighted mean of the root's Q (oz_root_value): pairwise_sum(N * Q over the 64 squares) / sum N; 0.0 unvisited"""
        nd = self.root(own, opp)
        a, total = np.zeros(64), 0
        for s in nd.acts:
            if nd.N[s] > 0:
                a[s] = float(nd.N[s]) * nd.Q[s]
                total += nd.N[s]
        return oracle.pairwise_sum(a) / float(total) if total else 0.0


def random_position(n, empties, seed):
    """a position with `empties` empties and a legal move, reached from the start by random legal moves (random.Random(seed)) -> (own, opp) of
    the side to move, or None where the game ended first"""
    import random
    rng = random.Random(seed)
    own, opp = initial_board(n)
    while n * n - popcount(own | opp) > empties:
        lg = legal_mask(own, opp, n)
        if not lg:
            if not legal_mask(opp, own, n):
                return None
            own, opp = opp, own
            continue
        own, opp = apply_move(own, opp, n, rng.choice([s for s in range(64) if (lg >> s) & 1]))
        own, opp = opp, own
    return (own, opp) if legal_mask(own, opp, n) else None


def episode(search, n, sims, seed, game_id, e_greedy, sample_moves=None):
    """one self-play game of the engine at policy temperature 1 (the greedy move is the first maximum of the counts) over `search`, its table
    kept over the game -> list of dict(black, white, player, ply, action, greedy, counts int32 [64], value, margin) per searched move;
    sample_moves=(temperature, plies) as the engine's (margin: move_sampling_ref's, inf for the other branches)"""
    black, white = initial_board(n)
    player, ply, out = 1, 0, []
    while True:
        own, opp = (black, white) if player == 1 else (white, black)
        lg = legal_mask(own, opp, n)
        if lg == 0:
            if legal_mask(opp, own, n) == 0:
                return out
            player = -player
            continue
        search.simulate(own, opp, sims)
        cnt, _ = search.counts(own, opp)
        action, greedy, margin = ms.selfplay_move(cnt, lg, e_greedy, seed, game_id, ply, sample_moves)
        out.append(dict(black=black, white=white, player=player, ply=ply, action=action, greedy=greedy, counts=cnt,
                        value=search.root_value(own, opp), margin=margin))
        own, opp = apply_move(own, opp, n, action)
        black, white = (own, opp) if player == 1 else (opp, own)
        player = -player
        ply += 1


def replay_arena_game(r, gi, n, sims, seed, gid, agents):
    """tests/test_gpu_wide_search.py's arena replay: agents = {+1: search of BLACK, -1: search of WHITE}; each replays its own plies"""
    black, white = initial_board(n)
    for ply in range(int(r["n_moves"][gi])):
        p = int(r["players"][gi][ply])
        own, opp = (black, white) if p == 1 else (white, black)
        assert legal_mask(own, opp, n), (gi, ply)
        W = agents[p]
        W.simulate(own, opp, sims)
        assert int(r["actions"][gi][ply]) == W.best_move(own, opp, tie_draw(seed, gid, ply)), (gi, ply, W.mode)
        own, opp = apply_move(own, opp, n, int(r["actions"][gi][ply]))
        black, white = (own, opp) if p == 1 else (opp, own)
    assert legal_mask(black, white, n) == 0 and legal_mask(white, black, n) == 0
    assert (int(r["final_black"][gi]), int(r["final_white"][gi])) == (black, white)
