"""Restatement of forced playouts and policy target pruning (include/othellozero_amd.h, "forced playouts") in plain Python floats: the search
that forces the tried children of the noisy root up to their quota, and the pruning of the root's count row.  The tests compare the kernels and
the host entry oz_forced_playouts_prune with it bit for bit."""
import math

import numpy as np

from root_noise_ref import NoisyWideSearch
from wide_search_ref import apply_move, legal_mask, popcount

INT_MAX = 2147483647


class ForcedWideSearch(NoisyWideSearch):
    """NoisyWideSearch whose depth-0 rule on the noisy root forces: a child with N' > 0 and (double)N' < sqrt((k * Pn) * (Ns + ks)) gets
    U = +inf.  `forced` counts the descents that took an infinite U.  k == 0, or no noise set for the root, is NoisyWideSearch."""

    def __init__(self, *args, k=0.0, **kw):
        super().__init__(*args, **kw)
        self.k = float(k)
        self.forced = 0

    def _descend(self, own, opp, inflight):
        nz = self.noise
        if not self.k > 0.0 or nz is None or (nz[0], nz[1]) != (own, opp):
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
                if d == 0 and N > 0 and float(N) < math.sqrt((self.k * P) * float(nd.Ns + ks)):
                    u = math.inf
                if best < 0 or u > bu:
                    best, bu = sq, u
            if d == 0 and bu == math.inf:
                self.forced += 1
            path.append((idx, best))
            own, opp = apply_move(own, opp, n, best)
            theirs = legal_mask(opp, own, n)
            if theirs:
                own, opp, lg = opp, own, theirs
            else:
                lg = legal_mask(own, opp, n)

    def root_row(self, own, opp):
        """(N int32 [64], Q, P float64 [64], legal, Ns) of the root record: the operands of prune"""
        nd = self.root(own, opp)
        N, Q, P = np.zeros(64, np.int32), np.zeros(64), np.zeros(64)
        for s in nd.acts:
            N[s], Q[s], P[s] = nd.N[s], nd.Q[s], nd.P[s]
        return N, Q, P, legal_mask(own, opp, self.n), nd.Ns

    def pruned(self, own, opp):
        """the pruned count row of the root under the noise set for it (the raw row if none is, or k == 0)"""
        N, Q, P, lg, Ns = self.root_row(own, opp)
        nz = self.noise
        if not self.k > 0.0 or nz is None or (nz[0], nz[1]) != (own, opp):
            return N
        return prune(N, Q, P, nz[3], lg, Ns, self.c, nz[2], self.k)


def prune(N, Q, P, eta, legal, Ns, c, eps, k):
    """the pruned row (int32 [64]) of one root: N int [64], Q, P, eta float [64] by square, legal the mask, Ns the root's visits"""
    c, eps, k, Ns = float(c), float(eps), float(k), int(Ns)
    out = np.zeros(64, np.int32)
    squares = [s for s in range(64) if (legal >> s) & 1]
    if not squares:
        return out
    star = squares[0]
    for s in squares:
        if int(N[s]) > int(N[star]):
            star = s
    root = math.sqrt(float(Ns))
    pn_star = (1.0 - eps) * float(P[star]) + eps * float(eta[star])
    ustar = float(Q[star]) + (c * pn_star) * (root / float(1 + int(N[star])))
    for s in squares:
        n = int(N[s])
        if s == star or n <= 0 or not k > 0.0:
            out[s] = n
            continue
        pn = (1.0 - eps) * float(P[s]) + eps * float(eta[s])
        f = math.sqrt((k * pn) * float(Ns))
        F = int(math.ceil(f)) if math.isfinite(f) and math.ceil(f) < INT_MAX else INT_MAX
        gap = ustar - float(Q[s])
        np_ = n
        if gap > 0.0:
            need = ((c * pn) * root) / gap - 1.0
            m = (int(math.ceil(need)) if need > 0.0 else 0) if need < float(n) else n
            np_ = min(n, max(n - F, m))
        if np_ < n and np_ <= 1:
            np_ = 0
        out[s] = np_
    return out


# ---- the searches the tests share: 4 golden roots per board size, host-supplied eta, 40 simulations.  The seeds were picked without a GPU so
# that every (n, K) forces at least one descent and changes at least one row (test_forced_playouts_cpu asserts it, and so does the GPU test).
SEARCH_G, SEARCH_SIMS, SEARCH_SALT, SEARCH_ETA_SEED, SEARCH_ALPHA, SEARCH_EPS, SEARCH_K = 4, 40, 13, 5, 0.5, 0.25, 2.0
_CASES = {}


def search_roots(n):
    from test_gpu_wide_search import _golden_roots
    return _golden_roots(n, SEARCH_G)


def search_eta(n, roots, ply=0):
    from root_noise_ref import dirichlet
    return np.array([dirichlet(n, legal_mask(o, p, n), SEARCH_ALPHA, SEARCH_ETA_SEED, gi, ply)[0] for gi, (o, p) in enumerate(roots)])


def search_case(n, K):
    """(roots, eta, [ForcedWideSearch after SEARCH_SIMS simulations from its root]) -- computed once per (n, K) and left unchanged"""
    if (n, K) not in _CASES:
        roots = search_roots(n)
        eta = search_eta(n, roots)
        refs = []
        for gi, (o, p) in enumerate(roots):
            r = ForcedWideSearch(n, 1.0, K, salt=SEARCH_SALT, k=SEARCH_K)
            r.set_noise(o, p, eta[gi], SEARCH_EPS)
            r.simulate(o, p, SEARCH_SIMS)
            refs.append(r)
        _CASES[(n, K)] = (roots, eta, refs)
    return _CASES[(n, K)]


def case_is_not_vacuous(n, K):
    """(forced descents, rows the pruning changed) of search_case(n, K)"""
    roots, _, refs = search_case(n, K)
    forced = sum(r.forced for r in refs)
    changed = sum(not np.array_equal(r.root_row(o, p)[0], r.pruned(o, p)) for r, (o, p) in zip(refs, roots))
    return forced, changed
