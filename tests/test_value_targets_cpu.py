"""Value targets without a GPU: the new symbols in header, bindings and library; oz_root_values and oz_value_targets (the functions the
kernels evaluate, run on the host) against the plain Python restatement (tests/value_targets_ref.py), bit for bit; the identities between
the modes; the argument validators; the targets column of the pooled record rows."""
import os
import re

import numpy as np
import pytest

import value_targets_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_root_values", "oz_mcts_root_values", "oz_selfplay_set_record_values", "oz_selfplay_values", "oz_selfplay_values_device",
               "oz_selfplay_value_targets", "oz_selfplay_targets", "oz_selfplay_targets_device", "oz_value_targets",
               "oz_replay_append_selfplay_targets", "oz_replay_append_records_values"]
MODES = ["outcome", ("blend", 0.5), ("blend", 0.3), ("td", 0.7), ("td", 0.25)]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "---- value targets" in header
    for k, v in (("OUTCOME", 0), ("BLEND", 1), ("TD", 2)):
        assert re.search(r"^#define OZ_VALUE_TARGET_%s %d$" % (k, v), header, flags=re.M) and getattr(_lib, "VALUE_TARGET_" + k) == v
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        common = f.read()
    for name in ("oz_root_value", "oz_root_term", "oz_root_mean", "oz_value_target_blend", "oz_value_target_td_step", "oz_value_target_exact"):
        assert re.search(r"\b%s\(" % name, common), name


# ------------------------------------------------------------------ root values
def _rows(rng, count, f32=False):
    """edge rows as a search leaves them: a few legal squares with counts and values in [-1, 1], 0 elsewhere"""
    N, Q = np.zeros((count, 64), np.int32), np.zeros((count, 64), np.float64)
    for i in range(count):
        k = int(rng.integers(1, 14))
        sq = rng.choice(64, size=k, replace=False)
        N[i, sq] = rng.integers(0, 60, size=k)
        q = rng.uniform(-1.0, 1.0, size=k)
        Q[i, sq] = q.astype(np.float32).astype(np.float64) if f32 else q
    return N, Q


@pytest.mark.parametrize("f32", [False, True])
def test_root_values_equal_the_restatement(f32):
    from othellozero_amd import agents
    rng = np.random.default_rng(11 + f32)
    N, Q = _rows(rng, 300, f32)
    got = agents.rules_root_values(N, Q)
    assert _same_bits(got, ref.root_values(N, Q))
    assert np.abs(got).max() <= 1.0 and np.count_nonzero(got) > 250


def test_root_values_edge_rows():
    from othellozero_amd import agents
    rng = np.random.default_rng(5)
    N, Q = _rows(rng, 8)
    N[0] = 0                                               # nothing visited: 0.0, whatever Q holds
    Q[0, 3] = np.nan
    N[1] = 0; Q[1] = 0; N[1, 19] = 7; Q[1, 19] = -0.3     # one legal move: its own Q, up to the rounding of (7 q) / 7
    N[2, N[2] > 0] = 1                                     # every visited child once: the mean of the Qs
    Q[3, N[3] == 0] = np.inf                               # values of unvisited squares are never read
    N[4] = 2 ** 20; Q[4] = rng.uniform(-1, 1, 64)          # a full row of large counts
    got = agents.rules_root_values(N, Q)
    assert _same_bits(got, ref.root_values(N, Q))
    assert got[0] == 0.0 and got[1] == (7 * -0.3) / 7 and np.isfinite(got).all()
    assert agents.rules_root_values(N[2], Q[2]).shape == () and agents.rules_root_values(N.reshape(2, 4, 64), Q.reshape(2, 4, 64)).shape == (2, 4)
    assert agents.rules_root_values(np.zeros((0, 64), np.int32), np.zeros((0, 64))).shape == (0,)
    with pytest.raises(ValueError):
        agents.rules_root_values(N, Q[:, :32])
    bad = N.copy()
    bad[5, 9] = -1
    from othellozero_amd import _lib
    with pytest.raises(_lib.OzError):
        agents.rules_root_values(bad, Q)


# ------------------------------------------------------------------ value targets
def synthetic_games(n=6, seed=3, games=7, shuffle=True):
    """records of made-up games with passes (consecutive plies of one mover), one fast-flagged record per game with ply >= 3, boards whose
    number of empties falls by one per ply to 0 .. 2 at the end, and random root values; in shuffled order"""
    from othellozero_amd import _lib
    rng = np.random.default_rng(seed)
    squares = [r * 8 + c for r in range(n) for c in range(n)]
    recs, vals = [], []
    for g in range(games):
        T = int(rng.integers(1, 13)) if g else 1           # (a game of one ply among them)
        left = int(rng.integers(0, 3))
        player = 1
        winner = 1 if rng.random() < 0.5 else -1
        for ply in range(T):
            empties = left + (T - ply)
            occ = [int(s) for s in rng.permutation(squares)[: n * n - empties]]
            black = sum(1 << s for s in occ[::2])
            white = sum(1 << s for s in occ[1::2])
            r = np.zeros((), _lib.RECORD_DTYPE)
            r["black"], r["white"], r["game_id"], r["ply"], r["player"] = black, white, 1000 + 17 * g, ply, player
            r["z"] = 1 if winner == player else -1
            if ply == 3:
                r["pad"][0] = 1
            recs.append(r)
            vals.append(float(rng.uniform(-1, 1)))
            if rng.random() < 0.8:                         # else: a pass, the same mover again
                player = -player
    rec, val = np.array(recs, _lib.RECORD_DTYPE), np.array(vals, np.float64)
    if shuffle:
        order = rng.permutation(rec.size)
        rec, val = rec[order], val[order]
    return rec, val


def test_synthetic_games_have_what_the_test_is_about():
    from othellozero_amd import _lib
    rec, _ = synthetic_games()
    srt = rec[np.lexsort((rec["ply"], rec["game_id"]))]
    same_game = srt["game_id"][1:] == srt["game_id"][:-1]
    assert (same_game & (srt["player"][1:] == srt["player"][:-1])).any()           # a pass
    assert len(set(rec["game_id"].tolist())) == 7 and _lib.record_fast(rec).sum() >= 2
    assert not np.array_equal(rec, srt)                                            # shuffled
    empties = np.array([ref._empties(r, 6) for r in rec])
    assert (empties <= 4).any() and (empties > 4).any()


@pytest.mark.parametrize("E", [0, 4])
@pytest.mark.parametrize("mode", MODES, ids=str)
def test_value_targets_equal_the_restatement(mode, E):
    from othellozero_amd import agents
    for seed in (3, 4):
        rec, val = synthetic_games(seed=seed)
        got = agents.rules_value_targets(rec, val, 6, mode, exact_empties=E)
        assert got.dtype == np.float32 and _same_bits(got, ref.value_targets(rec, val, 6, mode, E)), (mode, E, seed)
        # the order the records come in does not matter
        back = np.argsort(np.lexsort((rec["ply"], rec["game_id"])))
        srt = np.lexsort((rec["ply"], rec["game_id"]))
        assert _same_bits(agents.rules_value_targets(rec[srt], val[srt], 6, mode, exact_empties=E)[back], got)


@pytest.mark.parametrize("E", [0, 4])
def test_identities(E):
    from othellozero_amd import agents
    rec, val = synthetic_games(seed=9)
    z = rec["z"].astype(np.float32)
    exact = np.array([E > 0 and ref._empties(r, 6) <= E for r in rec])
    f = lambda vt: agents.rules_value_targets(rec, val, 6, vt, exact_empties=E)          # noqa: E731
    assert _same_bits(f("outcome"), z) and _same_bits(f(None), z)
    assert _same_bits(f(("td", 1.0)), z) and _same_bits(f(("blend", 0.0)), z)
    q32 = val.astype(np.float32)
    if E == 0:
        assert _same_bits(f(("td", 0.0)), q32)
    else:
        assert exact.any() and not exact.all()
        assert _same_bits(f(("td", 0.0))[~exact], q32[~exact]) and _same_bits(f(("td", 0.0))[exact], z[exact])
    b1 = f(("blend", 1.0))
    assert _same_bits(b1[~exact], q32[~exact]) and _same_bits(b1[exact], z[exact])
    # an exact record restarts the chain: what follows it changes nothing before it
    if E:
        srt = np.lexsort((rec["ply"], rec["game_id"]))
        r2, v2 = rec[srt].copy(), val[srt].copy()
        ex = np.array([ref._empties(r, 6) <= E for r in r2])
        gid = r2["game_id"]
        first_exact = next(i for i in range(r2.size) if ex[i] and i + 1 < r2.size and gid[i + 1] == gid[i] and i > 0 and gid[i - 1] == gid[i])
        v3 = v2.copy()
        later = (gid == gid[first_exact]) & (np.arange(r2.size) > first_exact)
        v3[later] = -v3[later]
        a, b = (agents.rules_value_targets(r2, v, 6, ("td", 0.6), exact_empties=E) for v in (v2, v3))
        before = (gid == gid[first_exact]) & (np.arange(r2.size) <= first_exact)
        assert _same_bits(a[before], b[before])
        a0, b0 = (agents.rules_value_targets(r2, v, 6, ("td", 0.6), exact_empties=0) for v in (v2, v3))
        assert not _same_bits(a0[before], b0[before])      # ... which, without the exact records, it does


def test_validators():
    from othellozero_amd import _lib, agents
    ok = _lib.check_value_target
    assert ok(None) == (0, 0.0) and ok("outcome") == (0, 0.0) and ok(("blend", 0.5)) == (1, 0.5) and ok(["td", 1]) == (2, 1.0)
    assert ok("outcome", True) == (0, 0.0)                 # the outcome belongs to every position of the game
    for bad in ("td", ("td",), ("td", 0.5, 1), ("blend", -0.1), ("td", 1.5), ("td", float("nan")), ("mean", 0.5), ("td", "0.5"), ("td", True),
                ("td", None), 0.5, (0, 0.5)):
        with pytest.raises(ValueError):
            ok(bad)
    with pytest.raises(ValueError, match="alias_final_boards"):
        ok(("td", 0.5), True)
    rec, val = synthetic_games()
    with pytest.raises(ValueError):
        agents.rules_value_targets(rec, val[:-1], 6, ("td", 0.5))
    with pytest.raises(ValueError):
        agents.rules_value_targets(rec, val, 6, ("td", 0.5), exact_empties=13)
    lib, out = _lib.load(), np.zeros(rec.size, np.float32)
    call = lambda n, mode, param, E: lib.oz_value_targets(rec.ctypes.data, _lib.p_f64(val), rec.size, n, mode, param, E, _lib.p_f32(out))    # noqa: E731
    assert call(6, 2, 0.5, 0) == _lib.OZ_OK
    for args in ((5, 2, 0.5, 0), (6, 3, 0.5, 0), (6, -1, 0.5, 0), (6, 2, 1.5, 0), (6, 1, float("nan"), 0), (6, 2, 0.5, -1), (6, 2, 0.5, 13)):
        assert call(*args) == _lib.OZ_ERR_ARG, args
    assert call(6, 0, 7.0, 0) == _lib.OZ_OK                # the outcome has no parameter to check
    assert lib.oz_value_targets(None, None, 0, 6, 2, 0.5, 0, None) == _lib.OZ_OK
    from othellozero_amd.training import execute_episode, expand_examples, selfplay_batch
    from othellozero_amd import loop
    with pytest.raises(ValueError, match="alias_final_boards"):
        execute_episode(6, None, 1.0, 4, 1.0, 0.9, value_target=("td", 0.5))              # snapshot_boards=False
    with pytest.raises(ValueError, match="alias_final_boards"):
        selfplay_batch(None, 6, 4, 4, expand=True, alias_final=True, value_target=("blend", 0.5))
    with pytest.raises(ValueError, match="alias_final_boards"):
        loop.training(6, 1, 4, 4, 1.0, 1.0, None, 0.9, 1, 1, 0, False, 1, 2, 1, "x", 64, value_target=("td", 0.7), alias_final_boards=True)
    with pytest.raises(AssertionError):
        expand_examples(rec, 6, values=np.zeros(rec.size - 1, np.float32))


def test_split_record_rows_with_a_targets_column():
    import torch
    from othellozero_amd import distributed as D
    rec, val = synthetic_games()
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 50, size=(rec.size, 64)).astype(np.int32)
    tgt = val.astype(np.float32)
    raw = rec.view(np.uint8).reshape(-1, 48)
    order = np.lexsort((rec["ply"], rec["game_id"]))
    rows = torch.from_numpy(np.concatenate([raw, counts.view(np.uint8).reshape(-1, 256), tgt.view(np.uint8).reshape(-1, 4)], axis=1))
    r, c, t = D.split_record_rows(rows, with_targets=True)
    assert np.array_equal(r, rec[order]) and np.array_equal(c, counts[order]) and _same_bits(t, tgt[order])
    rows = torch.from_numpy(np.concatenate([raw, tgt.view(np.uint8).reshape(-1, 4)], axis=1))
    r, t = D.split_record_rows(rows, with_targets=True, with_visits=False)
    assert np.array_equal(r, rec[order]) and _same_bits(t, tgt[order])
    # the default is the call of before: (records, counts)
    rows = torch.from_numpy(np.concatenate([raw, counts.view(np.uint8).reshape(-1, 256)], axis=1))
    r, c = D.split_record_rows(rows)
    assert np.array_equal(r, rec[order]) and np.array_equal(c, counts[order])
