"""Restatement of the Gumbel search (include/othellozero_amd.h, "Gumbel search") in plain Python floats: the draw over the oracle's stream
primitive, the sequential-halving schedule, the root's pick / move / improved policy row, and a hand-driven search over the oracle's rules
that picks by them at depth 0 of the root it was armed for.  No library code: the tests hold the kernels and the host-only twins against it."""
import math

import numpy as np

import oracle
from wide_search_ref import WideSearch, apply_move, legal_mask, popcount

RNG_GUMBEL = 7
UNIT = 1.0 / 9007199254740992.0
W_ZERO = 2.0 ** -54                                        # what the endpoint draw u == 0 maps to


# ------------------------------------------------------------------ the draw
def gumbel_from_unit(u):
    w = u if u > 0.0 else W_ZERO
    return -math.log(-math.log(w))


def unit(seed, game_id, ply, sq):
    return float(int(oracle.lib().orc_rng(seed, game_id, ply, RNG_GUMBEL + 256 * sq)) >> 11) * UNIT


def gumbel_row(legal, seed, game_id, ply):
    """g by square (float64 [64]), 0 off `legal`"""
    g = np.zeros(64)
    for sq in range(64):
        if (legal >> sq) & 1:
            g[sq] = gumbel_from_unit(unit(seed, game_id, ply, sq))
    return g


# ------------------------------------------------------------------ the schedule
def considered_visits(m, n):
    if m <= 1:
        return list(range(n))
    L = int(math.ceil(math.log2(m)))
    visits, k, out = [0] * m, m, []
    while len(out) < n:
        extra = max(1, n // (L * k))
        for _ in range(extra):
            out.extend(visits[:k])
            for i in range(k):
                visits[i] += 1
        k = max(2, k // 2)
    return out[:n]


# ------------------------------------------------------------------ one root
def _log(p):
    return math.log(p) if p > 0.0 else -math.inf


def root(N, N0, Q, P, g, legal, vhat, max_considered, c_visit, c_scale, budget):
    """the root quantities from rows by square -> dict(pick, move, pi float32 [64], score [64], x [64], gap_pick, gap_move, t, cv)"""
    acts = [s for s in range(64) if (legal >> s) & 1]
    sumN, maxN, Pvis, PQ = 0, 0, 0.0, 0.0
    for s in acts:
        sumN += int(N[s])
        maxN = max(maxN, int(N[s]))
        if N[s] > 0:
            Pvis = Pvis + float(P[s])
            PQ = PQ + float(P[s]) * float(Q[s])
    if sumN == 0:
        vmix = float(vhat)
    else:
        term = (float(sumN) / Pvis) * PQ if Pvis > 0.0 else 0.0          # (only zero-prior squares visited: the term is 0)
        vmix = (float(vhat) + term) / (1.0 + float(sumN))
    x, score = [-math.inf] * 64, [-math.inf] * 64
    for s in acts:
        qhat = float(Q[s]) if N[s] > 0 else vmix
        sigma = ((float(c_visit) + float(maxN)) * float(c_scale)) * ((qhat + 1.0) * 0.5)
        x[s] = _log(float(P[s])) + sigma
        score[s] = (float(g[s]) + _log(float(P[s]))) + sigma
    out = dict(pick=-1, move=-1, pi=np.zeros(64, np.float32), score=score, x=x, gap_pick=math.inf, gap_move=math.inf, t=0, cv=0)
    if not acts:
        return out
    n = {s: int(N[s]) - int(N0[s]) for s in acts}
    t, maxn = sum(n.values()), max(n.values())
    m_eff = min(max_considered, len(acts))
    cv = considered_visits(m_eff, budget)[t] if t < budget else maxn
    out["t"], out["cv"] = t, cv

    def first_max(want):
        cand = [s for s in acts if n[s] == want] or acts
        best = cand[0]
        for s in cand[1:]:
            if score[s] > score[best]:
                best = s
        rest = [score[s] for s in cand if s != best]
        return best, (score[best] - max(rest) if rest and max(rest) > -math.inf else math.inf)

    out["pick"], out["gap_pick"] = first_max(cv)
    out["move"], out["gap_move"] = first_max(maxn)
    mx = max(x[s] for s in acts)
    if mx == -math.inf:
        for s in acts:
            out["pi"][s] = np.float32(1.0 / len(acts))
        return out
    e, total = {}, 0.0
    for s in acts:
        e[s] = math.exp(x[s] - mx)
        total = total + e[s]
    for s in acts:
        out["pi"][s] = np.float32(e[s] / total)
    return out


# ------------------------------------------------------------------ the search
class GumbelSearch(WideSearch):
    """WideSearch at K = 1 that keeps every node's own value (vhat) and, at depth 0 of the root it was armed for, picks by the Gumbel rule.
    Unarmed it is WideSearch."""

    def __init__(self, n, c, salt=0, keep_mask=0, evaluator=None):
        super().__init__(n, c, 1, salt=salt, keep_mask=keep_mask, evaluator=evaluator)
        self.vhat = {}
        self.gum = None
        self.min_gap = math.inf

    def _expand(self, own, opp, lg):
        value = super()._expand(own, opp, lg)
        self.vhat[len(self.nodes) - 1] = -value            # the value the expansion backs up, before negation
        return value

    def arm(self, own, opp, g, max_considered, c_visit, c_scale, budget):
        idx = self.index.get((own, opp))
        n0 = [0] * 64
        if idx is not None:
            for s, v in self.nodes[idx].N.items():
                n0[s] = v
        self.gum = dict(own=own, opp=opp, g=[float(v) for v in g], n0=n0, m=max_considered, cv=float(c_visit), cs=float(c_scale), budget=budget)

    def disarm(self):
        self.gum = None

    def rows(self, own, opp):
        """(N, Q, P by square, vhat) of a known root"""
        idx = self.index[(own, opp)]
        nd = self.nodes[idx]
        N, Q, P = [0] * 64, [0.0] * 64, [0.0] * 64
        for s in nd.acts:
            N[s], Q[s], P[s] = nd.N[s], nd.Q[s], nd.P[s]
        return N, Q, P, self.vhat[idx]

    def root_eval(self, own, opp):
        gm = self.gum
        assert gm is not None and (gm["own"], gm["opp"]) == (own, opp)
        N, Q, P, vhat = self.rows(own, opp)
        return root(N, gm["n0"], Q, P, gm["g"], legal_mask(own, opp, self.n), vhat, gm["m"], gm["cv"], gm["cs"], gm["budget"])

    def visits(self, own, opp):
        """n(a) by square: this search's visits of the armed root"""
        N = self.rows(own, opp)[0]
        return [N[s] - self.gum["n0"][s] for s in range(64)]

    def _descend(self, own, opp, inflight):
        gm = self.gum
        if gm is None or (gm["own"], gm["opp"]) != (own, opp) or (own, opp) not in self.index:
            return super()._descend(own, opp, inflight)
        assert not inflight
        n = self.n
        if legal_mask(own, opp, n) == 0:
            return super()._descend(own, opp, inflight)
        r = self.root_eval(own, opp)
        self.min_gap = min(self.min_gap, r["gap_pick"])
        best = r["pick"]
        path = [(self.index[(own, opp)], best)]
        own, opp = apply_move(own, opp, n, best)
        theirs = legal_mask(opp, own, n)
        if theirs:
            own, opp, lg = opp, own, theirs
        else:
            lg = legal_mask(own, opp, n)
        # below the root: PUCT, as WideSearch walks it
        while True:
            if lg == 0 and legal_mask(opp, own, n) == 0:
                return path, ("term", -1 if popcount(own) >= popcount(opp) else 1)
            idx = self.index.get((own, opp))
            if idx is None:
                return path, ("leaf", own, opp, lg)
            nd = self.nodes[idx]
            best, bu = -1, 0.0
            for sq in nd.acts:
                u = nd.Q[sq] + (self.c * nd.P[sq]) * (math.sqrt(float(nd.Ns)) / float(1 + nd.N[sq]))
                if best < 0 or u > bu:
                    best, bu = sq, u
            path.append((idx, best))
            own, opp = apply_move(own, opp, n, best)
            theirs = legal_mask(opp, own, n)
            if theirs:
                own, opp, lg = opp, own, theirs
            else:
                lg = legal_mask(own, opp, n)
