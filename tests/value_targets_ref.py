"""Plain Python restatement of the value targets (include/othellozero_amd.h, "value targets"): the root value of a search and the three
target modes.  Python floats are IEEE float64 and Python never contracts a * b + c, so every product and every sum below is rounded on its
own, as the definition says; the 64-term sum is the oracle's pairwise_sum (NumPy's np.sum order)."""
import numpy as np

import oracle


def root_value(N, Q):
    """N, Q: 64 counts and 64 edge values by square -> pairwise_sum(N * Q) / sum(N) as a Python float; 0.0 where nothing was visited"""
    a = [float(int(N[sq])) * float(Q[sq]) if int(N[sq]) > 0 else 0.0 for sq in range(64)]
    total = sum(int(N[sq]) for sq in range(64) if int(N[sq]) > 0)
    if total == 0:
        return 0.0
    return float(oracle.pairwise_sum(a)) / float(total)


def root_values(N, Q):
    N, Q = np.asarray(N).reshape(-1, 64), np.asarray(Q, np.float64).reshape(-1, 64)
    return np.array([root_value(N[i], Q[i]) for i in range(N.shape[0])], np.float64)


def _empties(rec, n):
    return n * n - bin(int(rec["black"]) | int(rec["white"])).count("1")


def value_targets(records, values, n, value_target, exact_empties=0):
    """records (RECORD_DTYPE, any order), values (their root values) -> float32 (R,) targets, target i for record i.  value_target =
    "outcome", ("blend", w) or ("td", lam)."""
    R = len(records)
    out = np.zeros(R, np.float32)
    mode, param = (value_target, 0.0) if isinstance(value_target, str) else (value_target[0], float(value_target[1]))
    one_minus = 1.0 - param
    games = {}
    for i in range(R):
        games.setdefault(int(records["game_id"][i]), []).append(i)
    for ids in games.values():
        ids.sort(key=lambda i: int(records["ply"][i]))           # (stable: equal plies keep their order)
        last = ids[-1]
        B = float(int(records["player"][last]) * int(records["z"][last]))
        for i in reversed(ids):
            p, z, q = float(int(records["player"][i])), float(int(records["z"][i])), float(values[i])
            exact = exact_empties > 0 and _empties(records[i], n) <= exact_empties
            if mode == "outcome":
                t = z
            elif mode == "blend":
                if exact:
                    t = z
                else:
                    a = one_minus * z
                    b = param * q
                    t = a + b
            else:
                assert mode == "td", mode
                if exact:
                    B = p * z
                else:
                    a = one_minus * (p * q)
                    b = param * B
                    B = a + b
                t = p * B
            out[i] = np.float32(t)                                # one rounding, float64 -> float32
    return out
