"""Forced playouts and policy target pruning without a GPU: the new symbols in header, bindings and library; oz_forced_playouts_prune (the
function the kernels evaluate, run on the host) against the restatement's prune, bit for bit, on rows of restated searches and on hand-made
edge rows; the properties of a pruned row; the refusals; check_forced_playouts; and that the searches the GPU test compares are not vacuous."""
import os
import re

import numpy as np
import pytest

import forced_playouts_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_forced_playouts_prune", "oz_mcts_set_forced_playouts", "oz_mcts_get_forced_playouts", "oz_mcts_pruned_counts",
               "oz_selfplay_set_forced_playouts", "oz_selfplay_get_forced_playouts"]
CASES = [(n, K) for n in (6, 8) for K in (1, 4, 16)]


def _host(N, Q, P, eta, legal, Ns, c, eps, k):
    from othellozero_amd import agents
    return agents.rules_prune_counts(N, Q, P, eta, legal, Ns, c, eps, k)


def _raw(oz, N, Q, P, eta, legal, Ns, c, eps, k):
    """the C entry itself, nothing checked in Python: (rc, pruned)"""
    N = np.ascontiguousarray(N, np.int32).reshape(-1, 64)
    Q, P, eta = (np.ascontiguousarray(x, np.float64).reshape(-1, 64) for x in (Q, P, eta))
    legal, Ns = np.ascontiguousarray(legal, np.uint64).ravel(), np.ascontiguousarray(Ns, np.int32).ravel()
    out = np.full((N.shape[0], 64), -7, np.int32)
    rc = oz.load().oz_forced_playouts_prune(oz.p_i32(N), oz.p_f64(Q), oz.p_f64(P), oz.p_f64(eta), oz.p_u64(legal), oz.p_i32(Ns), N.shape[0],
                                            float(c), float(eps), float(k), oz.p_i32(out))
    return rc, out


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "---- forced playouts" in header and "MOVE CHOICE IS EXPLORATION" in header
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        assert re.search(r"\bint oz_forced_prune\(", f.read())
    assert lib.oz_version() == 230


@pytest.mark.parametrize("n,K", CASES)
def test_the_searches_of_the_gpu_test_force_and_prune(n, K):
    forced, changed = ref.case_is_not_vacuous(n, K)
    assert forced >= 1 and changed >= 1, (n, K, forced, changed)


def _properties(N, legal, pruned, where):
    squares = [s for s in range(64) if (legal >> s) & 1]
    assert all(0 <= pruned[s] <= N[s] for s in range(64)), where
    assert all(pruned[s] == 0 for s in range(64) if s not in squares), where
    if squares:
        star = max(squares, key=lambda s: (int(N[s]), -s))                 # the first legal square with the largest count
        assert pruned[star] == N[star], where
        if N[star] > 0:
            assert int(pruned.sum()) >= 1, where
    assert all(pruned[s] != 1 or N[s] == 1 for s in squares), where        # nothing is cut down TO one visit


@pytest.mark.parametrize("n,K", CASES)
def test_host_prune_vs_restatement_on_searched_rows(n, K):
    roots, eta, refs = ref.search_case(n, K)
    rows = [r.root_row(o, p) for r, (o, p) in zip(refs, roots)]
    N, Q, P = (np.array([x[i] for x in rows]) for i in range(3))
    legal, Ns = [x[3] for x in rows], [x[4] for x in rows]
    for k in (0.5, 2.0, 16.0):
        for eps in (ref.SEARCH_EPS, 0.9):
            got = _host(N, Q, P, eta, legal, Ns, 1.0, eps, k)
            for gi in range(len(rows)):
                want = ref.prune(N[gi], Q[gi], P[gi], eta[gi], legal[gi], Ns[gi], 1.0, eps, k)
                assert np.array_equal(got[gi], want), (n, K, k, eps, gi, got[gi], want)
                _properties(N[gi], legal[gi], got[gi], (n, K, k, eps, gi))
    # k == 0 is the identity on the legal set
    assert np.array_equal(_host(N, Q, P, eta, legal, Ns, 1.0, ref.SEARCH_EPS, 0.0), N)
    # ... and the restatement's own pruned() is prune() of its root under its noise
    for gi, (r, (o, p)) in enumerate(zip(refs, roots)):
        assert np.array_equal(r.pruned(o, p), ref.prune(N[gi], Q[gi], P[gi], eta[gi], legal[gi], Ns[gi], 1.0, ref.SEARCH_EPS, ref.SEARCH_K))


def _row(entries, Ns=None):
    """entries: {sq: (N, Q, P, eta)} -> one row's arrays"""
    N, Q, P, eta, legal = np.zeros(64, np.int32), np.zeros(64), np.zeros(64), np.zeros(64), 0
    for s, (n_, q, p, e) in entries.items():
        N[s], Q[s], P[s], eta[s] = n_, q, p, e
        legal |= 1 << s
    return N, Q, P, eta, legal, int(N.sum()) if Ns is None else Ns


EDGE_ROWS = {
    # the other child's Q alone reaches Ustar: kept whatever forcing added
    "gap <= 0": (_row({3: (30, -0.2, 0.5, 0.5), 9: (4, 0.9, 0.01, 0.4), 20: (2, -0.15, 0.2, 0.1)}), 1.0, 0.25, 2.0),
    # PUCT would have granted more than it has (need >= N): kept
    "need above N": (_row({3: (20, 0.1, 0.3, 0.3), 9: (19, 0.09, 0.6, 0.6), 20: (1, -0.9, 0.1, 0.1)}), 1.0, 0.25, 2.0),
    # N - F and need both land on one visit: dropped to 0
    "reduced to 1": (_row({3: (35, 0.5, 0.7, 0.5), 9: (3, -0.5, 0.1, 0.3), 20: (2, -0.4, 0.2, 0.2)}), 1.0, 0.25, 2.0),
    "one legal move": (_row({17: (39, 0.3, 1.0, 1.0)}), 1.0, 0.25, 2.0),
    # hand-made: counts on a root whose own visit counter is 0 (root == 0, F == 0: nothing can be taken)
    "Ns == 0": (_row({3: (5, 0.2, 0.5, 0.5), 9: (3, -0.2, 0.5, 0.5)}, Ns=0), 1.0, 0.25, 2.0),
    # all noise: Pn is eta, the stored prior does not matter
    "eps == 1": (_row({3: (30, 0.2, 0.0, 0.6), 9: (6, -0.3, 1.0, 0.3), 20: (3, -0.1, 0.0, 0.1)}), 1.0, 1.0, 2.0),
    "ties for star": (_row({3: (10, -0.1, 0.3, 0.3), 9: (10, 0.1, 0.3, 0.3), 20: (10, 0.0, 0.4, 0.4)}), 1.0, 0.25, 2.0),
    "unvisited squares": (_row({3: (0, 0.0, 0.3, 0.3), 9: (12, 0.1, 0.3, 0.3), 20: (0, 0.0, 0.4, 0.4)}), 1.0, 0.25, 2.0),
    "nothing visited": (_row({3: (0, 0.0, 0.5, 0.5), 9: (0, 0.0, 0.5, 0.5)}), 1.0, 0.25, 2.0),
    "no legal move": ((np.zeros(64, np.int32), np.zeros(64), np.zeros(64), np.zeros(64), 0, 0), 1.0, 0.25, 2.0),
    "large c, k = 16": (_row({3: (50, 0.2, 0.4, 0.2), 9: (25, 0.1, 0.3, 0.5), 20: (25, -0.6, 0.3, 0.3)}), 4.0, 0.5, 16.0),
}


@pytest.mark.parametrize("name", sorted(EDGE_ROWS))
def test_host_prune_vs_restatement_on_edge_rows(name):
    (N, Q, P, eta, legal, Ns), c, eps, k = EDGE_ROWS[name]
    got = _host(N, Q, P, eta, [legal], [Ns], c, eps, k)[0]
    want = ref.prune(N, Q, P, eta, legal, Ns, c, eps, k)
    assert np.array_equal(got, want), (name, got[N > 0], want[N > 0])
    _properties(N, legal, got, name)
    assert np.array_equal(_host(N, Q, P, eta, [legal], [Ns], c, eps, 0.0)[0], N), name          # k == 0: the identity


def test_the_edge_rows_are_the_edges_they_are_named_for():
    def out(name):
        (N, Q, P, eta, legal, Ns), c, eps, k = EDGE_ROWS[name]
        return N, ref.prune(N, Q, P, eta, legal, Ns, c, eps, k)
    N, p = out("gap <= 0")
    assert p[9] == N[9] == 4 and p[3] == 30
    N, p = out("need above N")
    assert p[9] == N[9] == 19
    N, p = out("reduced to 1")
    assert N[9] == 3 and p[9] == 0 and N[20] == 2 and p[20] == 0 and p[3] == 35
    N, p = out("one legal move")
    assert p[17] == 39 and int(p.sum()) == 39
    N, p = out("Ns == 0")
    assert np.array_equal(N, p)
    N, p = out("eps == 1")
    assert p[3] == 30 and p[9] < N[9]
    N, p = out("ties for star")
    assert p[3] == 10                                   # the first of the equal counts is star, whatever its Q
    N, p = out("nothing visited")
    assert not p.any()


def test_a_batch_is_its_rows(tmp_path):
    names = sorted(k for k, v in EDGE_ROWS.items() if v[1:] == (1.0, 0.25, 2.0))
    rows = [EDGE_ROWS[k][0] for k in names]
    N, Q, P, eta = (np.array([r[i] for r in rows]) for i in range(4))
    got = _host(N, Q, P, eta, [r[4] for r in rows], [r[5] for r in rows], 1.0, 0.25, 2.0)
    for i, r in enumerate(rows):
        assert np.array_equal(got[i], ref.prune(*r, 1.0, 0.25, 2.0)), names[i]


def test_argument_refusals_of_the_host_entry():
    from othellozero_amd import _lib as oz
    lib = oz.load()
    (N, Q, P, eta, legal, Ns), c, eps, k = EDGE_ROWS["reduced to 1"]
    for bad in (-0.5, 16.5, float("nan"), float("inf")):
        rc, out = _raw(oz, N, Q, P, eta, [legal], [Ns], c, eps, bad)
        assert rc == oz.OZ_ERR_ARG and "k" in lib.oz_last_error().decode() and (out == -7).all(), bad
    for bad in (-0.1, 1.5, float("nan")):
        rc, out = _raw(oz, N, Q, P, eta, [legal], [Ns], c, bad, k)
        assert rc == oz.OZ_ERR_ARG and "eps" in lib.oz_last_error().decode() and (out == -7).all(), bad
    assert _raw(oz, N, Q, P, eta, [legal], [Ns], float("nan"), eps, k)[0] == oz.OZ_ERR_ARG
    neg = N.copy()
    neg[9] = -1
    assert _raw(oz, neg, Q, P, eta, [legal], [Ns], c, eps, k)[0] == oz.OZ_ERR_ARG
    assert _raw(oz, N, Q, P, eta, [legal], [-3], c, eps, k)[0] == oz.OZ_ERR_ARG
    assert lib.oz_forced_playouts_prune(None, None, None, None, None, None, 1, 1.0, 0.25, 2.0, None) == oz.OZ_ERR_ARG
    assert lib.oz_forced_playouts_prune(None, None, None, None, None, None, -1, 1.0, 0.25, 2.0, None) == oz.OZ_ERR_ARG
    assert lib.oz_forced_playouts_prune(None, None, None, None, None, None, 0, 1.0, 0.25, 2.0, None) == oz.OZ_OK      # nothing to do
    rc, out = _raw(oz, N, Q, P, eta, [legal], [Ns], c, eps, k)                                                     # ... and it still works
    assert rc == oz.OZ_OK and np.array_equal(out[0], ref.prune(N, Q, P, eta, legal, Ns, c, eps, k))


@pytest.mark.parametrize("bad", [-1.0, 16.5, float("nan"), float("inf"), "2", True, (2.0,), [2.0, 1.0], object()])
def test_bad_forced_playouts_is_a_value_error_before_any_library_call(bad):
    from othellozero_amd import _lib, loop, training
    with pytest.raises(ValueError):
        _lib.check_forced_playouts(bad, (0.5, 0.25))
    with pytest.raises(ValueError):
        training.SelfPlayEngine(None, 6, 4, 8, root_noise=(0.5, 0.25), forced_playouts=bad)
    with pytest.raises(ValueError):
        training.selfplay_batch(None, 6, 4, 8, root_noise=(0.5, 0.25), forced_playouts=bad)
    with pytest.raises(ValueError):
        training.execute_episode(6, None, 1, 8, 1, 1.0, root_noise=(0.5, 0.25), forced_playouts=bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, 8, 1, 1, None, 0.9, 1, 2, 0, False, 1, 2, 1, "x.h5", 64, root_noise=(0.5, 0.25), forced_playouts=bad)


def test_forced_playouts_needs_root_noise():
    from othellozero_amd import _lib, agents, loop, training
    assert _lib.check_forced_playouts(None) == 0.0 and _lib.check_forced_playouts(0) == 0.0 and _lib.check_forced_playouts(0.0, None) == 0.0
    assert _lib.check_forced_playouts(2, (0.5, 0.25)) == 2.0 and _lib.check_forced_playouts(np.float32(0.5), (0.5, 0.25)) == 0.5
    assert _lib.check_forced_playouts(16, need_noise=False) == 16.0
    for noise in (None, (0.5, 0.0)):
        with pytest.raises(ValueError, match="root_noise"):
            _lib.check_forced_playouts(2.0, noise)
        with pytest.raises(ValueError, match="root_noise"):
            training.SelfPlayEngine(None, 6, 4, 8, root_noise=noise, forced_playouts=2)
        with pytest.raises(ValueError, match="root_noise"):
            training.selfplay_batch(None, 6, 4, 8, root_noise=noise, forced_playouts=2)
        with pytest.raises(ValueError, match="root_noise"):
            training.execute_episode(6, None, 1, 8, 1, 1.0, root_noise=noise, forced_playouts=2)
        with pytest.raises(ValueError, match="root_noise"):
            loop.training(6, 1, 2, 8, 1, 1, None, 0.9, 1, 2, 0, False, 1, 2, 1, "x.h5", 64, root_noise=noise, forced_playouts=2)
    with pytest.raises(ValueError):
        agents.rules_prune_counts(np.zeros((2, 64)), np.zeros((1, 64)), np.zeros((2, 64)), np.zeros((2, 64)), [0, 0], [0, 0], 1.0, 0.25, 2.0)
    with pytest.raises(ValueError):
        agents.rules_prune_counts(np.zeros((1, 64)), np.zeros((1, 64)), np.zeros((1, 64)), np.zeros((1, 64)), [0], [0], 1.0, 0.25, 17.0)
