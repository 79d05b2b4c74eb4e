"""Restatement of the leaf-parallel search (include/othellozero_amd.h, "leaf-parallel search"): K descents per step under virtual
loss, in plain Python floats over the oracle's rules / stub-network primitives.  The tests compare it with the kernels bit for bit;
at K = 1 it is oracle.Mcts (the C oracle the golden traces pin to the reference).  Float64 Q regime only.

evaluator: None -> the oracle's stub network (salt, keep_mask); else a callable (own, opp, n) -> (pi (n*n,) float32, v)."""
import ctypes as C
import math

import numpy as np

import oracle

RNG_TIE = 2


def _lib():
    return oracle.lib()


def legal_mask(own, opp, n):
    return int(_lib().orc_legal_mask(own, opp, n, 0))


def apply_move(own, opp, n, sq):
    a, b = C.c_uint64(own), C.c_uint64(opp)
    _lib().orc_apply_move(C.byref(a), C.byref(b), n, 0, sq)
    return a.value, b.value


def next_state(own, opp, n, sq):
    """the mover-canonical state after `sq`: the sides swap unless the opponent has to pass"""
    own, opp = apply_move(own, opp, n, sq)
    return (opp, own) if legal_mask(opp, own, n) else (own, opp)


def popcount(x):
    return bin(x).count("1")


def initial_board(n):
    b, w = C.c_uint64(), C.c_uint64()
    _lib().orc_initial_board(n, C.byref(b), C.byref(w))
    return b.value, w.value


def tie_draw(seed, game_id, ply):
    return int(_lib().orc_rng(seed, game_id, ply, RNG_TIE))


class Node:
    __slots__ = ("own", "opp", "Ns", "acts", "N", "Q", "P")


class WideSearch:
    def __init__(self, n, c, K, salt=0, keep_mask=0, evaluator=None):
        self.n, self.c, self.K, self.salt, self.keep, self.evaluator = n, float(c), K, salt, keep_mask, evaluator
        self.nodes, self.index = [], {}
        self.steps = self.leaves = self.collisions = self.sims = self.terminals = 0
        self.last_value = None

    # ---- one descent, seen through the descents of this step already in flight
    def _descend(self, own, opp, inflight):
        n = self.n
        path = []
        lg = legal_mask(own, opp, n)
        while True:
            if lg == 0 and legal_mask(opp, own, n) == 0:
                return path, ("term", -1 if popcount(own) >= popcount(opp) else 1)
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
                N, Q = nd.N[sq], nd.Q[sq]
                k = ke.get(sq, 0)
                if k:
                    Q = (float(N) * Q - float(k)) / float(N + k)
                    N = N + k
                u = Q + (self.c * nd.P[sq]) * (math.sqrt(float(nd.Ns + ks)) / float(1 + N))
                if best < 0 or u > bu:
                    best, bu = sq, u
            path.append((idx, best))
            own, opp = apply_move(own, opp, n, best)
            theirs = legal_mask(opp, own, n)
            if theirs:
                own, opp, lg = opp, own, theirs
            else:
                lg = legal_mask(own, opp, n)

    def _evaluate(self, own, opp):
        if self.evaluator is None:
            pi, v = oracle.stub_predict(own, opp, self.n, self.salt, self.keep)
        else:
            pi, v = self.evaluator(own, opp, self.n)
        return np.asarray(pi, dtype=np.float32).ravel(), np.float32(v)

    def _expand(self, own, opp, lg):
        n = self.n
        pi, v = self._evaluate(own, opp)
        nd = Node()
        nd.own, nd.opp, nd.Ns = own, opp, 0
        nd.acts = [s for s in range(64) if (lg >> s) & 1]
        arr = np.zeros(n * n)
        for s in nd.acts:
            arr[(s >> 3) * n + (s & 7)] = float(pi[(s >> 3) * n + (s & 7)])
        total = oracle.pairwise_sum(arr)
        nd.N = {s: 0 for s in nd.acts}
        nd.Q = {s: 0.0 for s in nd.acts}
        if total > 0:
            nd.P = {s: arr[(s >> 3) * n + (s & 7)] / total for s in nd.acts}
        else:
            nd.P = {s: 1.0 / len(nd.acts) for s in nd.acts}
        self.index[(own, opp)] = len(self.nodes)
        self.nodes.append(nd)
        return -float(v)

    def step(self, own, opp, budget):
        inflight = []
        for _ in range(min(self.K, budget)):
            path, res = self._descend(own, opp, inflight)
            if res[0] == "leaf" and any(r[0] == "leaf" and r[1] == res[1] and r[2] == res[2] for _, r in inflight):
                self.collisions += 1
                break
            inflight.append((path, res))
        for path, res in inflight:
            if res[0] == "leaf":
                value = self._expand(res[1], res[2], res[3])
                self.leaves += 1
            else:
                value = float(res[1])
                self.terminals += 1
            depth = len(path)
            for lvl, (idx, sq) in enumerate(path):
                val = -value if ((depth - 1 - lvl) & 1) else value
                nd = self.nodes[idx]
                nd.Q[sq] = (float(nd.N[sq]) * nd.Q[sq] + val) / float(nd.N[sq] + 1)
                nd.N[sq] += 1
                nd.Ns += 1
            self.last_value = -value if (depth & 1) else value
        self.steps += 1
        self.sims += len(inflight)
        return len(inflight)

    def simulate(self, own, opp, nsims):
        left = nsims
        while left:
            left -= self.step(own, opp, left)

    # ---- inspection
    def root(self, own, opp):
        return self.nodes[self.index[(own, opp)]]

    def counts(self, own, opp):
        """root visit counts by square (int32 [64]) and the legal mask"""
        nd = self.root(own, opp)
        cnt = np.zeros(64, np.int32)
        for s in nd.acts:
            cnt[s] = nd.N[s]
        return cnt, legal_mask(own, opp, self.n)

    def best_move(self, own, opp, tie_u):
        """the square temperature 0 picks: of the max-count squares the one the tie draw selects"""
        cnt, lg = self.counts(own, opp)
        pol = oracle.policy_from_counts(self.n, cnt, lg, 0.0, tie_u)
        r, c = np.argwhere(pol == 1.0)[0]
        return int(r) * 8 + int(c)


def assert_same_tables(dump, ref, where=""):
    """dump: list of dicts as OthelloMCTS.dump() / oracle.Mcts.dump() give them; ref: a WideSearch.  Equality of bits."""
    assert len(dump) == len(ref.nodes), (where, len(dump), len(ref.nodes))
    for i, (a, nd) in enumerate(zip(dump, ref.nodes)):
        assert (a["k0"], a["k1"], a["Ns"]) == (nd.own, nd.opp, nd.Ns), (where, i)
        for s in range(64):
            if s in nd.N:
                assert int(a["N"][s]) == nd.N[s] and float(a["Q"][s]) == nd.Q[s] and float(a["P"][s]) == nd.P[s], (where, i, s, a["N"][s], nd.N[s], a["Q"][s], nd.Q[s])
            else:
                assert int(a["N"][s]) == 0 and float(a["Q"][s]) == 0.0 and float(a["P"][s]) == 0.0, (where, i, s)
