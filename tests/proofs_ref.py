"""Restatement of the proofs of the search (include/othellozero_amd.h, "proofs") in plain Python over tests/value_signs_ref.py: SoundSearch
whose exact results -- finished boards, descents stopped on a proof, leaves expanded under solve_leaves -- are kept as proofs of edges and
nodes and backed up the path, and whose descent reads them.

Values are -1 / 0 / +1 for the side to move at the node, None = unknown.  edge[i] = {square: e} of node i, own[i] = the node's own value.
val(S) = own if set; else +1 if a legal edge has e = +1; else max e if every legal edge is known; else None.
Descent at node S, level d (after the finished-board check and the table lookup): d > 0 and val(S) known -> the descent ends here with
V_L = val(S); candidates = the legal edges with e == val(S) if known (the root), else / where empty those with e != -1, else the legal set
(inconsistent); U as SoundSearch with Q = float(e) where e is known; first maximum among the candidates; the taken edge's e known -> the
descent ends after the move with V_L = sigma ? -e : e.
Backup: Q / N / Ns as SoundSearch; then for an exact result, from the bottom with x = V_L: x = sigma_d ? -x : x; e(path[d]) = x; stop if
val(node) is unknown, else x = val(node).

Counters: edge_stops, node_stops, edges_proven, roots_proven (a root whose value went from unknown to known, or that was expanded with an
own value), first_root_proof (the simulation, counted from 1 over the object's life, at which that first happened), proofs_by_value,
own_nodes, corrupt.  log: a list to collect ("node", ...) / ("backup", ...) events for the host functions' tests, None = off."""
from value_signs_ref import SoundSearch, episode, random_position, replay_arena_game  # noqa: F401  (episode / replay over a ProvenSearch)
from wide_search_ref import apply_move, legal_mask, popcount

import math

DRAW_POSITION = (0x18120e0010, 0x1f072d313f0e)      # random_position(6, 4, 10): proven a draw at stub salt 7
STATS = ("edges_proven", "edge_stops", "node_stops", "roots_proven")


class ProvenSearch(SoundSearch):
    def __init__(self, n, c, K, salt=0, keep_mask=0, evaluator=None, solve=0):
        """solve = E of solve_leaves (the evaluator is then solve_leaves_ref.evaluator(E, ...): a leaf with <= E empties has the exact sign)"""
        super().__init__(n, c, K, salt=salt, keep_mask=keep_mask, evaluator=evaluator, mode="sound")
        self.solve = int(solve)
        self.edge, self.own = [], []
        self.edge_stops = self.node_stops = self.edges_proven = self.roots_proven = self.own_nodes = 0
        self.first_root_proof = None
        self.proofs_by_value = {-1: 0, 0: 0, 1: 0}
        self.corrupt = False
        self.log = None
        self._sim = 0

    def val(self, idx):
        if self.own[idx] is not None:
            return self.own[idx]
        nd, e = self.nodes[idx], self.edge[idx]
        if any(e.get(s) == 1 for s in nd.acts):
            return 1
        if nd.acts and all(s in e for s in nd.acts):
            return max(e[s] for s in nd.acts)
        return None

    def candidates(self, idx, v):
        nd, e = self.nodes[idx], self.edge[idx]
        cands = [s for s in nd.acts if e.get(s) == v] if v is not None else []
        if not cands:
            cands = [s for s in nd.acts if e.get(s) != -1]
        if not cands:
            cands, self.corrupt = list(nd.acts), True
        return cands

    def _expand(self, own, opp, lg):
        r = super()._expand(own, opp, lg)
        self.edge.append({})
        self.own.append(None)
        return r

    def _descend(self, own, opp, inflight):
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
            nd = self.nodes[idx]
            d = len(path)
            v = self.val(idx)
            if d > 0 and v is not None:
                self.node_stops += 1
                return path, ("term", v, "node")
            cands = self.candidates(idx, v)
            if self.log is not None:
                self.log.append(("node", lg, dict(self.edge[idx]), self.own[idx], v if d == 0 else None, list(cands)))
            e = self.edge[idx]
            ks, ke = 0, {}
            for p, _ in inflight:
                if len(p) > d and p[d][0] == idx:
                    ks += 1
                    ke[p[d][1]] = ke.get(p[d][1], 0) + 1
            best, bu = -1, 0.0
            for sq in cands:
                N, Q, P = nd.N[sq], nd.Q[sq], nd.P[sq]
                k = ke.get(sq, 0)
                if k:
                    Q = (float(N) * Q - float(k)) / float(N + k)
                    N = N + k
                if sq in e:
                    Q = float(e[sq])
                if nz is not None and d == 0:
                    P = (1.0 - nz[2]) * P + nz[2] * nz[3][sq]
                u = Q + (self.c * P) * (math.sqrt(float(nd.Ns + ks)) / float(1 + N))
                if best < 0 or u > bu:
                    best, bu = sq, u
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

    def _root_proven(self):
        self.roots_proven += 1
        if self.first_root_proof is None:
            self.first_root_proof = self._sim

    def _prove(self, path, leaf):
        if self.log is not None:
            before = [dict(legal=sum(1 << s for s in self.nodes[i].acts), edge=dict(self.edge[i]), own_value=self.own[i], square=sq, sigma=sg)
                      for i, sq, sg in path]
        x, marked, fresh, root = leaf, 0, 0, False
        for d in range(len(path) - 1, -1, -1):
            idx, sq, sg = path[d]
            x = -x if sg else x
            was = self.val(idx)
            e = self.edge[idx]
            marked += 1
            if sq in e:
                self.corrupt = self.corrupt or e[sq] != x
            else:
                e[sq] = x
                fresh += 1
                self.edges_proven += 1
                self.proofs_by_value[x] += 1
            v = self.val(idx)
            if v is None:
                break
            if d == 0 and was is None:
                root = True
                self._root_proven()
            x = v
        if self.log is not None:
            self.log.append(("backup", before, leaf, [dict(self.edge[i]) for i, _, _ in path], marked, fresh, root))

    def step(self, own, opp, budget):
        inflight = []
        for _ in range(min(self.K, budget)):
            path, res = self._descend(own, opp, inflight)
            if res[0] == "leaf" and any(r[0] == "leaf" and r[1] == res[1] and r[2] == res[2] for _, r in inflight):
                self.collisions += 1
                break
            inflight.append((path, res))
        for path, res in inflight:
            self._sim += 1
            sigma = [e[2] for e in path]
            exact = None
            if res[0] == "leaf":
                leaf = -self._expand(res[1], res[2], res[3])           # (_expand returns the reference's -v)
                self.leaves += 1
                self.pass_backups += 0 in sigma
                if self.solve > 0 and self.n * self.n - popcount(res[1] | res[2]) <= self.solve:
                    exact = self.own[-1] = int(leaf)
                    self.own_nodes += 1
                    if not path:
                        self._root_proven()
            else:
                leaf = float(res[1])
                exact = res[1]
                self.terminals += 1
                if res[2] == "board":
                    self.term[res[1]] += 1
            vals, self.last_value = self.backup_values(sigma, leaf)
            for (idx, sq, _), val in zip(path, vals):
                nd = self.nodes[idx]
                nd.Q[sq] = (float(nd.N[sq]) * nd.Q[sq] + val) / float(nd.N[sq] + 1)
                nd.N[sq] += 1
                nd.Ns += 1
            if exact is not None:
                self._prove(path, exact)
        self.steps += 1
        self.sims += len(inflight)
        return len(inflight)

    @staticmethod
    def backup_values(sigma, leaf):
        from value_signs_ref import backup_values
        return backup_values("sound", sigma, leaf)

    def stats(self):
        return [self.edges_proven, self.edge_stops, self.node_stops, self.roots_proven]

    def root_proof(self, own, opp):
        """(val, {square: e}) of the node of (own, opp)"""
        idx = self.index[(own, opp)]
        return self.val(idx), dict(self.edge[idx])
