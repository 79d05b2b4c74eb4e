"""Plain Python restatement of policy surprise weighting (include/othellozero_amd.h, "policy surprise weighting"): the surprise of a searched
move, the per-game weights, the copy counts and first symmetries, and the expansion of weighted records into example arrays.  Python floats
are IEEE float64 and Python never contracts a * b + c, so every product, quotient and sum below is rounded on its own, as the definition
says; the 64-term sums are the oracle's pairwise_sum (NumPy's np.sum order); the logarithm is math.log (the library's is oz_log_cr: the
tests bound the difference); the random stream is restated in Python integers."""
import math

import numpy as np

import oracle
import replay_ref

DBL_MIN = 2.2250738585072014e-308
RNG_SURPRISE = 8
_M = (1 << 64) - 1


def _sm64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def rng(seed, game, move, stream):
    """oz_rng: the counter-based stream keyed (seed, game id, ply, purpose)"""
    a = _sm64((seed + 0x632BE59BD9B4E019 * game) & _M)
    return _sm64(a ^ ((move * 0x9E3779B97F4A7C15) & _M) ^ ((stream * 0xD1B54A32D192ED03) & _M))


def rng_unit(u):
    return float(u >> 11) * (1.0 / 9007199254740992.0)


def target_row(row):
    """a count row (integers) at T = 1, or a float32 policy row widened -> 64 Python floats"""
    row = np.asarray(row)
    if np.issubdtype(row.dtype, np.integer):
        x = [float(int(v)) for v in row]
        s = float(oracle.pairwise_sum(x))
        d = s if s != 0 else 1.0
        return [v / d for v in x]
    assert row.dtype == np.float32, row.dtype
    return [float(v) for v in row]


def surprise_terms(row, P):
    q = target_row(row)
    out = []
    for a in range(64):
        if q[a] > 0.0:
            p = float(P[a])
            pp = p if p > DBL_MIN else DBL_MIN
            out.append(q[a] * (math.log(q[a]) - math.log(pp)))
        else:
            out.append(0.0)
    return out


def surprise(row, P):
    """-> (s, sum of |term|): s = max(0, pairwise_sum(term)); the second value sizes the tolerance against the library"""
    t = surprise_terms(row, P)
    s = float(oracle.pairwise_sum(t))
    return (s if s > 0.0 else 0.0), sum(abs(v) for v in t)


def surprises(rows, P):
    rows, P = np.asarray(rows), np.asarray(P, np.float64).reshape(-1, 64)
    rows = rows.reshape(-1, 64)
    got = [surprise(rows[i], P[i]) for i in range(rows.shape[0])]
    return np.array([g[0] for g in got], np.float64), np.array([g[1] for g in got], np.float64)


def bound(abs_sum):
    """8 * 2^-53 * (sum |term| + 1): one rounding each for the two logarithms, the subtraction and the product, six levels of pairwise sum"""
    return 8.0 * 2.0 ** -53 * (abs_sum + 1.0)


def _games(records):
    games = {}
    for i in range(len(records)):
        games.setdefault(int(records["game_id"][i]), []).append(i)
    for ids in games.values():
        ids.sort(key=lambda i: int(records["ply"][i]))
    return games


def weights(records, sur, frac):
    """records (RECORD_DTYPE, any order), their surprises -> float32 (R,) weights, weight i for record i"""
    out = np.zeros(len(records), np.float32)
    frac = float(frac)
    om = 1.0 - frac
    for ids in _games(records).values():
        arr = [0.0] * 64
        K = 0
        for i in ids:
            if int(records["pad"][i][0]) == 0:
                K += 1
                arr[int(records["ply"][i])] = float(sur[i])
        S = float(oracle.pairwise_sum(arr))
        for i in ids:
            if int(records["pad"][i][0]) != 0:
                out[i] = 0.0
            elif S == 0.0:
                out[i] = 1.0
            else:
                a = float(sur[i]) * float(K)
                b = a / S
                c = frac * b
                out[i] = np.float32(om + c)                       # one rounding, float64 -> float32
    return out


def copies(records, w, seed):
    """-> (copies int32 (R,), first_sym uint8 (R,))"""
    R = len(records)
    c, t0 = np.zeros(R, np.int32), np.zeros(R, np.uint8)
    for i in range(R):
        d = rng(int(seed), int(records["game_id"][i]), int(records["ply"][i]), RNG_SURPRISE)
        a = 8.0 * float(w[i])
        c[i] = int(math.floor(a + rng_unit(d)))
        t0[i] = d & 7
    return c, t0


def examples(records, n, c, t0, alias_final=False, counts=None, T=None, policies=None, z=None):
    """the example arrays (own, opp, pi, z) of weighted records: the non-fast records in ascending (game_id, ply), record i copies c[i] times,
    copy k = symmetry (t0[i] + k) & 7 of the record's 8 examples (replay_ref.examples).  counts: visit targets at temperature T; policies:
    float32 (R, 64) rows by square copied as they are; neither: one-hot.  z: float32 (R,) value targets in place of the records' z."""
    rec = np.asarray(records)
    keep = np.flatnonzero(rec["pad"][:, 0] == 0)
    order = keep[np.lexsort((rec["ply"][keep], rec["game_id"][keep]))]
    srt = rec[order]
    own8, opp8, pi8, z8 = replay_ref.examples(srt, n, alias_final, None if counts is None else np.asarray(counts).reshape(-1, 64)[order], T)
    A = n * n
    if policies is not None:
        P = replay_ref.perm(n)
        cell = np.arange(A)
        row = np.asarray(policies, np.float32).reshape(-1, 64)[order][:, (cell // n) * 8 + cell % n]
        pi8 = np.stack([row[:, P[t]] for t in range(8)], axis=1).reshape(-1, A)
    if z is not None:
        z8 = np.repeat(np.asarray(z, np.float32)[order], 8)
    idx = []
    for i, r in enumerate(order):
        idx.extend(8 * i + ((int(t0[r]) + k) & 7) for k in range(int(c[r])))
    idx = np.asarray(idx, np.int64)
    return own8[idx], opp8[idx], np.ascontiguousarray(pi8[idx]).reshape(-1, A), z8[idx]
