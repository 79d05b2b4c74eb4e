"""Root noise without a GPU: the restatement's sampler (tests/root_noise_ref.py) against the Dirichlet law, its exact edge cases, the
restatement's search against WideSearch, the new symbols in header and bindings, and the argument checks of the Python surface."""
import math
import os
import re

import numpy as np
import pytest

from root_noise_ref import NoisyWideSearch, dirichlet, gamma
from test_gpu_wide_search import _golden_roots
from wide_search_ref import WideSearch, assert_same_tables, legal_mask, popcount

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_mcts_set_root_noise", "oz_mcts_sample_root_noise", "oz_mcts_get_root_noise", "oz_selfplay_set_root_noise",
               "oz_selfplay_root_noise"]


def _beta_moments(a, b):
    """mean, variance and fourth central moment of Beta(a, b) from its raw moments E[X^k] = prod_{j<k} (a + j) / (a + b + j)"""
    m = [1.0]
    for k in range(4):
        m.append(m[-1] * (a + k) / (a + b + k))
    mean = m[1]
    var = m[2] - mean ** 2
    m4 = m[4] - 4 * mean * m[3] + 6 * mean ** 2 * m[2] - 3 * mean ** 4
    return mean, var, m4


@pytest.mark.parametrize("alpha", [0.3, 1.0])
def test_sampler_mean_and_variance_against_the_dirichlet_law(alpha):
    """R = 2000 draws of Dir(alpha) over K = 8 squares.  A component is Beta(alpha, (K - 1) alpha): mean 1 / K, variance
    (1 / K)(1 - 1 / K) / (K alpha + 1).  The sample mean of one component over R independent draws has standard error sqrt(var / R); the
    sample variance has standard error sqrt((m4 - var^2) / R) (m4 = the fourth central moment), and pooling the K identically distributed
    components of a draw cannot make that larger.  Both bounds are 5 standard errors: alpha = 0.3 -> 0.0201 on a mean, 0.0083 on the
    variance; alpha = 1.0 -> 0.0123 and 0.0027."""
    R, K, seed = 2000, 8, 1234
    legal = 0xFF                                           # the sampler sees a legal mask only
    rows = np.array([dirichlet(8, legal, alpha, seed, gid, 3)[0][:K] for gid in range(R)])
    mean, var, m4 = _beta_moments(alpha, (K - 1) * alpha)
    assert mean == pytest.approx(1.0 / K) and var == pytest.approx((1 / K) * (1 - 1 / K) / (K * alpha + 1))
    tol_mean, tol_var = 5 * math.sqrt(var / R), 5 * math.sqrt((m4 - var * var) / R)
    got_mean, got_var = rows.mean(axis=0), float(((rows - 1.0 / K) ** 2).mean())
    print(f"alpha {alpha}: means {got_mean.min():.4f} .. {got_mean.max():.4f} (1/K +- {tol_mean:.4f}), variance {got_var:.5f} (theory {var:.5f} +- {tol_var:.5f})")
    assert np.abs(got_mean - 1.0 / K).max() <= tol_mean
    assert abs(got_var - var) <= tol_var
    assert np.abs(rows.sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("alpha", [0.03, 0.3, 1.0, 2.5])
def test_sampler_edge_cases_are_exact(alpha):
    for sq in (0, 19, 63):
        eta, _, _ = dirichlet(8, 1 << sq, alpha, 9, 4, 11)
        assert eta[sq] == 1.0 and eta.sum() == 1.0         # one legal move
    legal = (1 << 2) | (1 << 11) | (1 << 29) | (1 << 34)
    eta, margin, used = dirichlet(6, legal, alpha, 9, 4, 11)
    assert all(eta[s] == 0.0 for s in range(64) if not (legal >> s) & 1) and all(eta[s] > 0.0 for s in (2, 11, 29, 34))
    assert abs(eta.sum() - 1.0) <= 1e-12 and 1 <= used <= 16 and margin > 0
    assert dirichlet(6, 0, alpha, 9, 4, 11)[0].sum() == 0.0
    # streams: another square, game, ply or seed is another draw
    g0 = gamma(alpha, 9, 4, 11, 2)[0]
    assert len({g0, gamma(alpha, 9, 4, 11, 3)[0], gamma(alpha, 9, 5, 11, 2)[0], gamma(alpha, 9, 4, 12, 2)[0], gamma(alpha, 10, 4, 11, 2)[0]}) == 5


@pytest.mark.parametrize("n", [6, 8])
def test_decision_margins_of_the_roots_the_gpu_test_draws_for(n):
    """test_gpu_root_noise compares the device's draws with the restatement's within 1e-9: no accept / reject decision of those draws may sit
    within reach of a last-bit difference in log / cos / sqrt"""
    import test_gpu_root_noise as T
    roots = _golden_roots(n, 64)
    for seed in T.SAMPLER_SEEDS:
        for alpha in T.SAMPLER_ALPHAS:
            worst = min(dirichlet(n, legal_mask(o, p, n), alpha, seed, T.SAMPLER_FIRST_ID + gi, popcount(o | p) - 4)[1] for gi, (o, p) in enumerate(roots))
            assert worst >= 1e-6, (n, seed, alpha, worst)


@pytest.mark.parametrize("K", [1, 4])
def test_noisy_search_without_noise_is_wide_search(K):
    n, salt = 6, 13
    own, opp = _golden_roots(n, 8)[3]
    A, B = WideSearch(n, 1.0, K, salt=salt), NoisyWideSearch(n, 1.0, K, salt=salt)
    eta = dirichlet(n, legal_mask(own, opp, n), 0.5, 5, 0, 0)[0]
    B.set_noise(own, opp, eta, 0.0)                        # eps == 0 is no noise
    C = NoisyWideSearch(n, 1.0, K, salt=salt)
    C.set_noise(opp, own, eta, 0.25)                       # noise of another board
    for nsims in (2, 25, 60):
        for s in (A, B, C):
            s.simulate(own, opp, nsims)

    def as_dump(s):
        return [dict(k0=nd.own, k1=nd.opp, Ns=nd.Ns, N=[nd.N.get(q, 0) for q in range(64)], Q=[nd.Q.get(q, 0.0) for q in range(64)],
                     P=[nd.P.get(q, 0.0) for q in range(64)]) for nd in s.nodes]
    assert_same_tables(as_dump(B), A, "eps 0")
    assert_same_tables(as_dump(C), A, "another board")
    assert (A.steps, A.collisions, A.leaves) == (B.steps, B.collisions, B.leaves)


def test_noise_changes_the_search_and_never_the_stored_priors():
    n, salt, K = 6, 13, 4
    changed = 0
    for gi, (own, opp) in enumerate(_golden_roots(n, 8)):
        A, B = WideSearch(n, 1.0, K, salt=salt), NoisyWideSearch(n, 1.0, K, salt=salt)
        B.set_noise(own, opp, dirichlet(n, legal_mask(own, opp, n), 0.5, 5, gi, 0)[0], 0.25)
        A.simulate(own, opp, 60)
        B.simulate(own, opp, 60)
        assert A.root(own, opp).P == B.root(own, opp).P
        assert sum(B.root(own, opp).N.values()) == sum(A.root(own, opp).N.values()) == 59
        changed += not np.array_equal(A.counts(own, opp)[0], B.counts(own, opp)[0])
    assert changed >= 1


def test_new_symbols_in_header_and_bindings():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.oz_version() >= 220
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        assert re.search(r"OZ_RNG_NOISE\s*=\s*3\b", f.read())


@pytest.mark.parametrize("bad", [(0.5,), (0.5, 0.25, 1), (0.001, 0.25), (101.0, 0.25), (float("nan"), 0.25), (float("inf"), 0.25), (0.5, -0.1),
                                 (0.5, 1.5), (0.5, float("nan")), "ab", 0.5])
def test_bad_root_noise_is_a_value_error_before_any_library_call(bad):
    """(without a GPU the library calls behind these would raise OzLibraryError: a ValueError shows the check came first)"""
    from othellozero_amd import _lib, loop, training
    with pytest.raises(ValueError):
        _lib.check_root_noise(bad)
    with pytest.raises(ValueError):
        training.SelfPlayEngine(object(), 6, 4, 8, root_noise=bad)
    with pytest.raises(ValueError):
        training.selfplay_batch(object(), 6, 4, 8, root_noise=bad)
    with pytest.raises(ValueError):
        training.execute_episode(6, object(), 1.0, 8, 1, 1.0, root_noise=bad)
    with pytest.raises(ValueError):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, root_noise=bad)
    assert _lib.check_root_noise(None) is None and _lib.check_root_noise((0.5, 0.25)) == (0.5, 0.25) and _lib.check_root_noise([1, 0]) == (1.0, 0.0)
