"""Restatement of the root noise (include/othellozero_amd.h, "root noise") in plain Python floats: the counter-based Dirichlet sampler over
the oracle's stream primitive, and the search that mixes it into the root's priors at selection time.  The tests compare the kernels with it:
the sampler within 1e-9 (device and host libm differ by ulps; the accept / reject margins are checked to be far wider), the search bit for bit."""
import math

import numpy as np

import oracle
from wide_search_ref import WideSearch, apply_move, legal_mask, popcount

RNG_NOISE = 3
ATTEMPTS = 16
UNIT = 1.0 / 9007199254740992.0


def unit(seed, game_id, ply, sq, i):
    """u(sq, i): the unit draw of stream RNG_NOISE + 256 sq + 65536 i"""
    return float(int(oracle.lib().orc_rng(seed, game_id, ply, RNG_NOISE + 256 * sq + 65536 * i)) >> 11) * UNIT


def gamma(alpha, seed, game_id, ply, sq):
    """Marsaglia-Tsang Gamma(alpha) of one square -> (g, smallest decision margin met, attempts used)"""
    a = alpha + 1.0 if alpha < 1.0 else alpha
    d = a - 1.0 / 3.0
    cc = 1.0 / math.sqrt(9.0 * d)
    g, margin, used = d, math.inf, ATTEMPTS
    for t in range(ATTEMPTS):
        w0 = 1.0 - unit(seed, game_id, ply, sq, 3 * t)
        u1 = unit(seed, game_id, ply, sq, 3 * t + 1)
        x = math.sqrt(-2.0 * math.log(w0)) * math.cos(2.0 * math.pi * u1)
        v = 1.0 + cc * x
        margin = min(margin, abs(v))
        if v <= 0.0:
            continue
        v = v * v * v
        w2 = 1.0 - unit(seed, game_id, ply, sq, 3 * t + 2)
        lhs, rhs = math.log(w2), 0.5 * x * x + d - d * v + d * math.log(v)
        margin = min(margin, abs(lhs - rhs))
        if lhs < rhs:
            g, used = d * v, t + 1
            break
    if alpha < 1.0:
        g *= math.pow(1.0 - unit(seed, game_id, ply, sq, 48), 1.0 / alpha)
    return g, margin, used


def dirichlet(n, legal, alpha, seed, game_id, ply):
    """eta by square (float64 [64], 0 off `legal`) -> (eta, smallest decision margin, most attempts)"""
    squares = [s for s in range(64) if (legal >> s) & 1]
    eta = np.zeros(64)
    if not squares:
        return eta, math.inf, 0
    arr, g, margin, used = np.zeros(n * n), {}, math.inf, 0
    for s in squares:
        g[s], m, k = gamma(alpha, seed, game_id, ply, s)
        margin, used = min(margin, m), max(used, k)
        arr[(s >> 3) * n + (s & 7)] = g[s]
    S = oracle.pairwise_sum(arr)
    for s in squares:
        eta[s] = g[s] / S if (S > 0.0 and math.isfinite(S)) else 1.0 / len(squares)
    return eta, margin, used


class NoisyWideSearch(WideSearch):
    """WideSearch whose descents see Pn = (1.0 - eps) * P + eps * eta[sq] at depth 0 of the root the noise was set for.  With no noise set it is
    WideSearch: _descend hands over to it."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.noise = None                                  # (own, opp, eps, eta[64])

    def set_noise(self, own, opp, eta, eps):
        self.noise = (own, opp, float(eps), [float(x) for x in eta]) if eps > 0 else None

    def clear_noise(self):
        self.noise = None

    def _descend(self, own, opp, inflight):
        nz = self.noise
        if nz is None or (nz[0], nz[1]) != (own, opp):
            return super()._descend(own, opp, inflight)
        eps, eta = nz[2], nz[3]
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
                N, Q, P = nd.N[sq], nd.Q[sq], nd.P[sq]
                k = ke.get(sq, 0)
                if k:
                    Q = (float(N) * Q - float(k)) / float(N + k)
                    N = N + k
                if d == 0:
                    P = (1.0 - eps) * P + eps * eta[sq]
                u = Q + (self.c * P) * (math.sqrt(float(nd.Ns + ks)) / float(1 + N))
                if best < 0 or u > bu:
                    best, bu = sq, u
            path.append((idx, best))
            own, opp = apply_move(own, opp, n, best)
            theirs = legal_mask(opp, own, n)
            if theirs:
                own, opp, lg = opp, own, theirs
            else:
                lg = legal_mask(own, opp, n)
