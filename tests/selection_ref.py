"""Restatement of the selection option (include/othellozero_amd.h, "selection") in plain Python over tests/value_signs_ref.py and
tests/proofs_ref.py: first-play urgency (FPU) reduction, a visit-scaled exploration constant and a prior-first first visit.

At a node S at level d, for a legal square a, with N', Q' the statistics as selection sees them (the virtual-loss view where descents of
the step are in flight), n = Ns + k(S), P the prior in use (the noisy one at an armed root) and vhat the value the node's expansion backed
up -- every product, sum and quotient one Python float operation in the order written:
    growth:      c_S = c + factor * L,  L = log(((1.0 + float(n)) + base) / base)                    off: c_S = c
    prior_first: r = sqrt(float(n)) if n > 0 else 1.0                                                 off: r = sqrt(float(n))
    fpu:         f = root_reduction if d == 0 else reduction;  SN = sum of N';  SQ = tree_sum(float(N') * Q' where N' > 0 else 0.0);
                 SP = tree_sum(P where N' > 0 else 0.0);  V = (vhat + SQ) / (1.0 + float(SN));  F = V - f * sqrt(SP), at least -1.0;
                 Q' := F on every legal edge with N' == 0
    U = Q' + (c_S * P) * (r / float(1 + N'))                  (under proofs a known edge value replaces Q' after the FPU step)
tree_sum: the balanced binary tree over the squares 0 .. 63, zeros off the legal set.

The logarithm is an argument: growth_log(n, base) -> L.  MATH_LOG is math.log; the tests that compare tables hand in the library's host twin
(library_log: agents.rules_select_c(0.0, base, 1.0, n) = 0.0 + 1.0 * L = L), as the surprise tests hand in oz_log_cr.

SelectSearch (over SoundSearch: reference and sound signs, root noise, K descents) and SelectProvenSearch (over ProvenSearch) override
_descend with it and keep vhat per node.  selection=None is the parent class bit for bit (tests/test_selection_cpu.py asserts it).
Counters: fpu_clamped = levels whose F hit the -1 clamp, prior_first_moved = fresh nodes (n == 0) where prior_first picked a square other
than the first legal one, inflight_unvisited = levels where an edge with stored N == 0 was seen with an in-flight visit,
growth_changed = levels where c_S != c changed the pick."""
import math

from proofs_ref import ProvenSearch
from value_signs_ref import POSITIONS_6, SoundSearch, terminal_value
from wide_search_ref import apply_move, initial_board, legal_mask, popcount

KEYS = ("fpu", "cpuct_growth", "prior_first")
# the case set of tests/test_gpu_value_signs.py, re-stated: (n, own, opp, simulations, stub salt) -- the 4x4 start at 100 and 200 simulations
# under the stub salts 3 and 11, and the four 6x6 positions with 8 empties (POSITIONS_6) at 60 simulations under salt 7.  Run at K = 1 and 4
# under SETTINGS and CLAMP it leaves no counter of the classes below at 0 (tests/test_selection_cpu.py asserts it), so no position was added.
SALT6 = 7
CASES = [(4, *initial_board(4), sims, salt) for sims in (100, 200) for salt in (3, 11)] + [(6, own, opp, 60, SALT6) for own, opp in POSITIONS_6]
SETTINGS = {"fpu": dict(fpu=(0.2, 0.1)), "growth": dict(cpuct_growth=(20, 2.0)), "prior_first": dict(prior_first=True),
            "all": dict(fpu=(0.2, 0.1), cpuct_growth=(20, 2.0), prior_first=True)}
CLAMP = dict(fpu=(2.5, 2.5))                                    # one more setting, for the -1 clamp of F


def MATH_LOG(n, base):
    return math.log(((1.0 + float(n)) + base) / base)


def library_log(n, base):
    from othellozero_amd import agents
    return agents.rules_select_c(0.0, base, 1.0, n)


def tree_sum(x):
    x = list(x)
    assert len(x) == 64
    while len(x) > 1:
        x = [x[2 * i] + x[2 * i + 1] for i in range(len(x) // 2)]
    return x[0]


def parts(selection):
    """(fpu or None, growth or None, prior_first) of the keyword's dict"""
    if selection is None:
        return None, None, False
    assert all(k in KEYS for k in selection), selection
    return selection.get("fpu"), selection.get("cpuct_growth"), bool(selection.get("prior_first", False))


def select_scores(N, Q, P, legal, n, vhat, level, c, selection, growth_log=MATH_LOG, proven=None):
    """one node: N, Q, P = 64 entries by square as selection sees them, legal = the mask, n = the node's visits in the same view, vhat, level,
    c, selection = the keyword's dict; proven = {square: e} of the edges with a known value (proofs).
    -> dict(U = [64] with -inf off the legal set, F, V (0.0 with fpu off), c_S, pick = the first maximum or -1, clamped)"""
    fpu, growth, prior_first = parts(selection)
    acts = [s for s in range(64) if (legal >> s) & 1]
    c_S = float(c)
    if growth is not None:
        c_S = float(c) + float(growth[1]) * growth_log(n, float(growth[0]))
    r = 1.0 if (prior_first and n <= 0) else math.sqrt(float(n))
    F = V = 0.0
    clamped = False
    q = {s: float(Q[s]) for s in acts}
    if fpu is not None:
        f = float(fpu[1]) if level == 0 else float(fpu[0])
        SN = sum(int(N[s]) for s in acts)
        SQ = tree_sum([float(int(N[s])) * float(Q[s]) if (s in q and N[s] > 0) else 0.0 for s in range(64)])
        SP = tree_sum([float(P[s]) if (s in q and N[s] > 0) else 0.0 for s in range(64)])
        V = (float(vhat) + SQ) / (1.0 + float(SN))
        F = V - f * math.sqrt(SP)
        if F < -1.0:
            F, clamped = -1.0, True
        for s in acts:
            if N[s] == 0:
                q[s] = F
    if proven:
        for s, e in proven.items():
            if s in q:
                q[s] = float(e)
    U = [-math.inf] * 64
    pick = -1
    for s in acts:
        U[s] = q[s] + (c_S * float(P[s])) * (r / float(1 + int(N[s])))
        if pick < 0 or U[s] > U[pick]:
            pick = s
    return dict(U=U, F=F, V=V, c_S=c_S, pick=pick, clamped=clamped)


def first_max(U, cands):
    best = -1
    for s in cands:
        if best < 0 or U[s] > U[best]:
            best = s
    return best


class _Selection:
    """what both classes share: the option, vhat per node, the counters and the pick at one level"""

    def _init_selection(self, selection, growth_log):
        self.selection = selection if selection is not None and any(parts(selection)) else None
        self.growth_log = growth_log
        self.vhat = []
        self.fpu_clamped = self.prior_first_moved = self.inflight_unvisited = self.growth_changed = 0

    def _expand(self, own, opp, lg):
        r = super()._expand(own, opp, lg)
        self.vhat.append(-r)                                    # (_expand returns the reference's -v: vhat is v, for the side to move there)
        return r

    def _pick(self, idx, d, cands, inflight, nz, proven=None):
        """the square the descent takes at node idx, level d, among cands (ascending); nz = the root-noise view or None"""
        nd = self.nodes[idx]
        ks, ke = 0, {}
        for p, _ in inflight:
            if len(p) > d and p[d][0] == idx:
                ks += 1
                ke[p[d][1]] = ke.get(p[d][1], 0) + 1
        N, Q, P, legal = [0] * 64, [0.0] * 64, [0.0] * 64, 0
        for sq in nd.acts:
            n_, q_, p_ = nd.N[sq], nd.Q[sq], nd.P[sq]
            k = ke.get(sq, 0)
            if k:
                q_ = (float(n_) * q_ - float(k)) / float(n_ + k)
                n_ = n_ + k
            if nz is not None and d == 0:
                p_ = (1.0 - nz[2]) * p_ + nz[2] * nz[3][sq]
            N[sq], Q[sq], P[sq] = n_, q_, p_
            legal |= 1 << sq
        n = nd.Ns + ks
        r = select_scores(N, Q, P, legal, n, self.vhat[idx], d, self.c, self.selection, self.growth_log, proven)
        best = first_max(r["U"], cands)
        fpu, growth, prior_first = parts(self.selection)
        self.fpu_clamped += r["clamped"]
        self.prior_first_moved += prior_first and n == 0 and best != cands[0]
        self.inflight_unvisited += any(nd.N[sq] == 0 for sq in ke)
        if growth is not None and r["c_S"] != self.c:
            flat = dict(self.selection, cpuct_growth=None)
            self.growth_changed += first_max(select_scores(N, Q, P, legal, n, self.vhat[idx], d, self.c, flat, self.growth_log, proven)["U"], cands) != best
        return best


class SelectSearch(_Selection, SoundSearch):
    def __init__(self, n, c, K, salt=0, keep_mask=0, evaluator=None, mode="sound", selection=None, growth_log=MATH_LOG):
        super().__init__(n, c, K, salt=salt, keep_mask=keep_mask, evaluator=evaluator, mode=mode)
        self._init_selection(selection, growth_log)

    def _descend(self, own, opp, inflight):
        if self.selection is None:
            return super()._descend(own, opp, inflight)
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
            best = self._pick(idx, len(path), self.nodes[idx].acts, inflight, nz)
            own, opp = apply_move(own, opp, n, best)
            theirs = legal_mask(opp, own, n)
            path.append((idx, best, 1 if theirs else 0))
            if theirs:
                own, opp, lg = opp, own, theirs
            else:
                lg = legal_mask(own, opp, n)


class SelectProvenSearch(_Selection, ProvenSearch):
    def __init__(self, n, c, K, salt=0, keep_mask=0, evaluator=None, solve=0, selection=None, growth_log=MATH_LOG):
        super().__init__(n, c, K, salt=salt, keep_mask=keep_mask, evaluator=evaluator, solve=solve)
        self._init_selection(selection, growth_log)

    def _descend(self, own, opp, inflight):
        if self.selection is None:
            return super()._descend(own, opp, inflight)
        n = self.n
        nz = self.noise if self.noise is not None and (self.noise[0], self.noise[1]) == (own, opp) else None
        path = []
        lg = legal_mask(own, opp, n)
        while True:
            if lg == 0 and legal_mask(opp, own, n) == 0:
                a, b = popcount(own), popcount(opp)
                return path, ("term", (a > b) - (a < b), "board")
            idx = self.index.get((own, opp))
            if idx is None:
                return path, ("leaf", own, opp, lg)
            d = len(path)
            v = self.val(idx)
            if d > 0 and v is not None:
                self.node_stops += 1
                return path, ("term", v, "node")
            cands = self.candidates(idx, v)
            e = self.edge[idx]
            best = self._pick(idx, d, cands, inflight, nz, proven=e)
            own, opp = apply_move(own, opp, n, best)
            theirs = legal_mask(opp, own, n)
            path.append((idx, best, 1 if theirs else 0))
            if best in e:
                self.edge_stops += 1
                return path, ("term", -e[best] if theirs else e[best], "edge")
            if theirs:
                own, opp, lg = opp, own, theirs
            else:
                lg = legal_mask(own, opp, n)


class Nep50SelectSearch(SelectSearch):
    """SelectSearch in the OZ_QMODE_NEP50 regime (what NumPy >= 2 computes for the reference's Q update), K = 1: a Q that has met a float32
    value is float32 from then on -- the update's product, sum and quotient are float32 operations -- and selection reads it widened to
    float64.  With selection=None and mode "reference" it is oracle.Mcts(qmode=QMODE_NEP50) (tests/test_selection_cpu.py asserts it)."""

    def __init__(self, n, c, salt=0, mode="sound", selection=None, growth_log=MATH_LOG):
        super().__init__(n, c, 1, salt=salt, mode=mode, selection=selection, growth_log=growth_log)
        self.q32 = []                                           # per node: {square: the stored Q is float32}

    def _expand(self, own, opp, lg):
        r = super()._expand(own, opp, lg)
        self.q32.append({})
        return r

    def step(self, own, opp, budget):
        import numpy as np
        from value_signs_ref import backup_values
        f32 = np.float32
        path, res = self._descend(own, opp, [])
        sigma = [e[2] for e in path]
        if res[0] == "leaf":
            leaf, is32 = -self._expand(res[1], res[2], res[3]), True
            self.leaves += 1
        else:
            leaf, is32 = float(res[1]), False
            self.terminals += 1
        vals, self.last_value = backup_values(self.mode, sigma, leaf)
        for (idx, sq, _), val in zip(path, vals):
            nd, tag = self.nodes[idx], self.q32[idx]
            N, Q = nd.N[sq], nd.Q[sq]
            if not tag.get(sq, False) and not is32:
                nd.Q[sq] = (float(N) * Q + val) / float(N + 1)
            else:
                prod = f32(N) * f32(Q) if tag.get(sq, False) else f32(float(N) * Q)
                nd.Q[sq] = float((prod + f32(val)) / f32(N + 1))
                tag[sq] = True
            nd.N[sq] += 1
            nd.Ns += 1
        self.steps += 1
        self.sims += 1
        return 1
