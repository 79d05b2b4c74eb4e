"""Restatement of the evaluation symmetry (include/othellozero_amd.h, "evaluation symmetry") in plain Python: splitmix64, the selection
t = sm64(sm64(seed ^ own) + opp) >> 61, the board transform from oracle.symmetry_perms(n) (cell j = r*n+c of orientation t is cell
perms[t][j] of the original), and an evaluator wrapper for the references that take one -- oracle.Mcts(evaluator=...), Mcts.episode,
wide_search_ref.WideSearch(evaluator=...).  "random": the inner evaluator on the position in orientation t, pi mapped back; "mean": all
eight orientations, pi and v = float32 0.125 * (((x_0 + x_1) + x_2) + ... + x_7) in NumPy float32, x_t mapped back to the original cells."""
import functools

import numpy as np

import minimax_ref as mm
import oracle

M64 = (1 << 64) - 1
IDENTITY = 7


def sm64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def symmetry(seed, own, opp):
    return sm64((sm64((int(seed) ^ int(own)) & M64) + int(opp)) & M64) >> 61


@functools.lru_cache(maxsize=None)
def perms(n):
    return tuple(tuple(int(x) for x in row) for row in oracle.symmetry_perms(n))


@functools.lru_cache(maxsize=None)
def inverse(t, n):
    """the orientation that undoes t"""
    p = perms(n)
    (u,) = [u for u in range(8) if all(p[t][p[u][j]] == j for j in range(n * n))]
    return u


@functools.lru_cache(maxsize=1 << 18)
def sym_board(t, n, b):
    out, p = 0, perms(n)[t]
    for j in range(n * n):
        src = p[j]
        if (int(b) >> ((src // n) * 8 + src % n)) & 1:
            out |= 1 << ((j // n) * 8 + j % n)
    return out


def unpermute(t, n, pi_t):
    """pi of the original board from the pi of orientation t: pi[perms[t][j]] = pi_t[j]"""
    pi = np.zeros(n * n, np.float32)
    pi[list(perms(n)[t])] = np.asarray(pi_t, np.float32).ravel()
    return pi


def mean8(xs):
    """float32 0.125 * (((x_0 + x_1) + x_2) + ... + x_7), element by element"""
    acc = np.asarray(xs[0], np.float32) + np.asarray(xs[1], np.float32)
    for x in xs[2:]:
        acc = acc + np.asarray(x, np.float32)
    assert acc.dtype == np.float32
    return np.float32(0.125) * acc


def stub(salt=0, keep_mask=0):
    """the oracle's stub network as an evaluator callable"""
    def inner(own, opp, n):
        return oracle.stub_predict(own, opp, n, salt, keep_mask)
    return inner


class evaluator:
    """evaluator(mode, seed, inner)(own, opp, n) -> (pi (n, n) float32, v float32); mode "off" / None, "random" or "mean";
    .calls counts the positions asked for, .moved those evaluated in another orientation than the identity"""

    def __init__(self, mode, seed, inner):
        assert mode in (None, "off", "random", "mean"), mode
        self.mode, self.seed, self.inner = mode, int(seed), inner
        self.calls = self.moved = 0

    def _one(self, t, own, opp, n):
        pi_t, v = self.inner(sym_board(t, n, own), sym_board(t, n, opp), n)
        return unpermute(t, n, pi_t), np.float32(v)

    def __call__(self, own, opp, n):
        own, opp = int(own), int(opp)
        self.calls += 1
        if self.mode in (None, "off"):
            return self.inner(own, opp, n)
        if self.mode == "random":
            t = symmetry(self.seed, own, opp)
            self.moved += t != IDENTITY
            pi, v = self._one(t, own, opp, n)
            return pi.reshape(n, n), v
        outs = [self._one(t, own, opp, n) for t in range(8)]
        self.moved += 1
        return mean8([o[0] for o in outs]).reshape(n, n), mean8([np.array([o[1]], np.float32) for o in outs])[0]


def canon(p):
    """(black, white, player) -> (own, opp) of the mover"""
    return (p[0], p[1]) if p[2] == 1 else (p[1], p[0])


@functools.lru_cache(maxsize=None)
def positions(n, seed=2026, games=4):
    """the distinct mover-canonical positions of a few seeded random playouts, in playout order"""
    return tuple(dict.fromkeys(canon(p) for p in mm.playout_positions(n, seed, games)))


# ---- the searches the CPU and the GPU tests share: name -> (n, mode, leaves_per_step, simulations)
SALT, SEED = 3, 11
SEARCH_CASES = {"6x6_random": (6, "random", 1, 60), "8x8_random": (8, "random", 1, 60), "6x6_random_k4": (6, "random", 4, 60),
                "8x8_random_k4": (8, "random", 4, 60), "6x6_mean": (6, "mean", 1, 60)}


def search_roots(name):
    """four mid-game roots (own, opp) of the case's board"""
    n = SEARCH_CASES[name][0]
    pool = [p for p in positions(n, 2025, 3) if n * n // 3 <= mm.popcount(p[0] | p[1]) <= 2 * n * n // 3]
    return pool[::max(1, len(pool) // 4)][:4]


@functools.lru_cache(maxsize=None)
def search_reference(name):
    """per root: (the reference search over the wrapped stub, the same search over the plain stub); K = 1: oracle.Mcts dumps,
    K > 1: WideSearch objects.  And the wrapper, for its counts."""
    from wide_search_ref import WideSearch
    n, mode, K, sims = SEARCH_CASES[name]
    ev = evaluator(mode, SEED, stub(SALT))
    out = []
    for own, opp in search_roots(name):
        if K == 1:
            m, m0 = oracle.Mcts(n, 1.0, 1, evaluator=ev), oracle.Mcts(n, 1.0, 1, salt=SALT)
            for _ in range(sims):
                m.simulate(own, opp, 1)
                m0.simulate(own, opp, 1)
            out.append((m.dump(), m0.dump()))
        else:
            w, w0 = WideSearch(n, 1.0, K, evaluator=ev), WideSearch(n, 1.0, K, salt=SALT)
            w.simulate(own, opp, sims)
            w0.simulate(own, opp, sims)
            out.append((w, w0))
    return out, ev


def same_node(a, b):
    """identical records: key, Ns, legal set, N, the bits of Q and P"""
    return ((a["k0"], a["k1"], a["Ns"], a["legal"]) == (b["k0"], b["k1"], b["Ns"], b["legal"]) and np.array_equal(a["N"], b["N"])
            and a["Q"].tobytes() == b["Q"].tobytes() and a["P"].tobytes() == b["P"].tobytes())


def same_tables(x, y):
    return len(x) == len(y) and all(same_node(a, b) for a, b in zip(x, y))


# ---- the self-play games the engine test compares: 64 games of 6x6 at 25 simulations on the stub network
EP = dict(n=6, games=64, sims=25, c=1.25, T=1.0, e_greedy=0.8, seed=777, first=1000, salt=9, es_seed=21)


@functools.lru_cache(maxsize=None)
def episodes(es_seed=EP["es_seed"], mode="random"):
    ev = evaluator(mode, es_seed, stub(EP["salt"]))
    return [oracle.Mcts(EP["n"], EP["c"], 1, evaluator=ev).episode(EP["sims"], EP["T"], EP["e_greedy"], EP["seed"], EP["first"] + g)
            for g in range(EP["games"])], ev
