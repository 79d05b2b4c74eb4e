"""NumPy model of the device-resident replay buffer (include/othellozero_amd.h, "replay buffer"): the 8 examples of a move record in the
trainer's data-set layout, built from the reference's own symmetry tables (tests/golden/symmetries.npz) and NumPy's own `**`, np.sum and
float32 cast, and the ring rule "running index k lives in slot k % capacity".  The tests compare the library with it bit for bit."""
import numpy as np

from conftest import load_golden
from wide_search_ref import apply_move, popcount

RECORD_DTYPE = np.dtype([("black", "<u8"), ("white", "<u8"), ("final_black", "<u8"), ("final_white", "<u8"), ("game_id", "<u8"),
                         ("ply", "u1"), ("action", "u1"), ("player", "i1"), ("z", "i1"), ("greedy", "u1"), ("pad", "u1", (3,))])
_PERM = {}


def perm(n):
    """(8, n*n): source cell of every output cell, training_example_symmetries' order (the identity is row 7)"""
    if n not in _PERM:
        _PERM[n] = load_golden("symmetries.npz")[f"perm_{n}"].astype(np.int64)
    return _PERM[n]


def _squares(n):
    """square row*8+col of cell row*n+col"""
    cell = np.arange(n * n)
    return (cell // n) * 8 + cell % n


def _cells(boards, n):
    """uint64 (R,) -> {0, 1} (R, n*n) by cell"""
    return ((boards[:, None] >> _squares(n).astype(np.uint64)[None, :]) & np.uint64(1)).astype(np.uint64)


def _pack(cells, n):
    return (cells << _squares(n).astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def examples(records, n, alias_final, counts=None, T=None):
    """records (any order; counts = their visit-count rows for the visit-distribution target at temperature T, None = one-hot targets)
    -> (own u64, opp u64, pi f32 (8R, n*n), z f32) in ascending (game_id, ply), example 8i+t = symmetry t of record i"""
    rec = np.asarray(records)
    order = np.lexsort((rec["ply"], rec["game_id"]))
    rec = rec[order]
    R, A, P = rec.size, n * n, perm(n)
    black = _cells(rec["final_black" if alias_final else "black"], n)
    white = _cells(rec["final_white" if alias_final else "white"], n)
    if counts is None:
        row = np.zeros((R, A), np.float32)
        row[np.arange(R), (rec["action"] >> 3).astype(np.int64) * n + (rec["action"] & 7)] = 1
    else:
        x = np.asarray(counts).reshape(-1, 64)[order][:, _squares(n)].astype(np.float64) ** (1.0 / T)      # 0 off the legal set
        row = np.zeros((R, A), np.float32)
        for i in range(R):
            s = np.sum(x[i].reshape(n, n))
            row[i] = (x[i] / (s if s != 0 else 1.0)).astype(np.float32)
    own, opp = np.zeros((R, 8), np.uint64), np.zeros((R, 8), np.uint64)
    pi = np.zeros((R, 8, A), np.float32)
    for t in range(8):
        own[:, t], opp[:, t] = _pack(black[:, P[t]], n), _pack(white[:, P[t]], n)
        pi[:, t] = row[:, P[t]]
    z = np.repeat(rec["z"].astype(np.float32), 8)
    return own.reshape(-1), opp.reshape(-1), pi.reshape(R * 8, A), z


def episode_records(g, name, game_id=None):
    """the move records of a golden episode (black / white / player / action per move): the final board by playing the last move with the
    oracle's rules, z by counting it (a draw goes to BLACK)"""
    n = int(g[f"{name}/meta"][0])
    black, white, player, action = (g[f"{name}/{k}"] for k in ("black", "white", "player", "action"))
    k = black.size
    b, w, sq = int(black[-1]), int(white[-1]), int(action[-1])
    if player[-1] == 1:
        b, w = apply_move(b, w, n, sq)
    else:
        w, b = apply_move(w, b, n, sq)
    winner = 1 if popcount(b) >= popcount(w) else -1
    rec = np.zeros(k, RECORD_DTYPE)
    rec["black"], rec["white"], rec["player"], rec["action"] = black, white, player, action
    rec["final_black"], rec["final_white"] = b, w
    rec["game_id"] = int(g[f"{name}/meta"][3]) if game_id is None else game_id
    rec["ply"] = np.arange(k)
    rec["z"] = np.where(player == winner, 1, -1)
    return rec


class Ring:
    """the slot rule: the example with running index k (from creation / clear) lives in slot k % capacity; an append of more than
    `capacity` examples keeps its last `capacity`"""

    def __init__(self, capacity, n):
        self.capacity, self.total = capacity, 0
        self.own, self.opp = np.zeros(capacity, np.uint64), np.zeros(capacity, np.uint64)
        self.pi, self.z = np.zeros((capacity, n * n), np.float32), np.zeros(capacity, np.float32)

    def append(self, own, opp, pi, z):
        E = len(z)
        for e in range(max(0, E - self.capacity), E):
            s = (self.total + e) % self.capacity
            self.own[s], self.opp[s], self.pi[s], self.z[s] = own[e], opp[e], pi[e], z[e]
        self.total += E

    def clear(self):
        self.total = 0

    @property
    def held(self):
        return min(self.total, self.capacity)

    def read(self):
        h = self.held
        return self.own[:h].copy(), self.opp[:h].copy(), self.pi[:h].copy(), self.z[:h].copy()


def same(a, b):
    """two (own, opp, pi, z) tuples, byte for byte"""
    return len(a) == len(b) == 4 and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
