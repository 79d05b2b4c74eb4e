"""The device-resident replay buffer without a GPU: the NumPy model the GPU tests compare against (tests/replay_ref.py) reproduces the
reference's own examples, its ring follows a brute-force list, the new symbols are in header, bindings and library, and the loop refuses
the combinations it cannot run before any library call."""
import os
import re

import numpy as np
import pytest

import replay_ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_replay_create", "oz_replay_destroy", "oz_replay_clear", "oz_replay_info", "oz_replay_append_selfplay",
               "oz_replay_append_records", "oz_replay_append_examples", "oz_replay_restore", "oz_replay_read", "oz_trainer_fit_epoch_replay"]


def test_model_reproduces_the_reference_examples_of_every_golden_episode(golden_episodes):
    """episodes.npz holds what execute_episode returned: two-plane boards aliased to the final position, one-hot policies, z"""
    g = golden_episodes
    for name in (str(x) for x in g["names"]):
        n = int(g[f"{name}/meta"][0])
        rec = replay_ref.episode_records(g, name)
        own, opp, pi, z = replay_ref.examples(rec, n, alias_final=True)
        eb, ep, ez = g[f"{name}/ex_board"], g[f"{name}/ex_policy"], g[f"{name}/ex_z"]
        assert own.dtype == np.uint64 and pi.dtype == np.float32 and z.dtype == np.float32 and pi.shape == (8 * rec.size, n * n), name
        assert np.array_equal(own, eb[:, 0]) and np.array_equal(opp, eb[:, 1]), name
        want = np.zeros_like(pi)
        want[np.arange(ep.size), ep] = 1
        assert np.array_equal(pi, want) and np.array_equal(z, ez.astype(np.float32)), name
        # without the aliasing the identity (example 7) shows the board at the move
        own_m, opp_m, pi_m, z_m = replay_ref.examples(rec, n, alias_final=False)
        assert np.array_equal(own_m[7::8], rec["black"]) and np.array_equal(opp_m[7::8], rec["white"]), name
        assert np.array_equal(pi_m, pi) and np.array_equal(z_m, z), name
        # a shuffled copy of the records gives the same examples
        shuffled = rec[np.random.RandomState(3).permutation(rec.size)]
        assert replay_ref.same(replay_ref.examples(shuffled, n, alias_final=True), (own, opp, pi, z)), name


def test_model_reproduces_the_reference_visit_targets():
    """ep6_T05 of policy_temps.npz: example 8i+7 is float32(pi[i]) of the reference, the other seven its training_example_symmetries"""
    from othellozero_amd.training import training_example_symmetries
    g = load_golden("policy_temps.npz")
    name = "ep6_T05"
    n, k = int(g[f"{name}/meta"][0]), int(g[f"{name}/meta"][7])
    rec = replay_ref.episode_records(g, name)
    cnt, pis = g[f"{name}/counts"], g[f"{name}/pi"]
    own, opp, pi, z = replay_ref.examples(rec, n, alias_final=False, counts=cnt, T=0.5)
    assert pi.shape == (8 * k, n * n) and np.array_equal(z, g[f"{name}/ex_z"].astype(np.float32))
    for i in range(k):
        assert np.array_equal(pi[8 * i + 7].reshape(n, n), pis[i].astype(np.float32)), i
        want = [p for _, p in training_example_symmetries(np.zeros((n, n)), pis[i].astype(np.float32))]
        assert all(np.array_equal(pi[8 * i + t].reshape(n, n), want[t]) for t in range(8)), i
    perm = np.random.RandomState(5).permutation(k)
    assert replay_ref.same(replay_ref.examples(rec[perm], n, False, counts=cnt[perm], T=0.5), (own, opp, pi, z))


def test_ring_against_a_brute_force_list():
    """capacity 100 (no multiple of 8), appends of 24, 80, 8, 240 (more than the capacity) and 16 examples: slot s holds the newest example
    whose running index is s modulo the capacity"""
    cap, n = 100, 4
    ring, everything = replay_ref.Ring(cap, n), []
    rs = np.random.RandomState(11)
    for E in (24, 80, 8, 240, 16):
        own, opp = rs.randint(0, 2**62, E).astype(np.uint64), rs.randint(0, 2**62, E).astype(np.uint64)
        pi, z = rs.rand(E, n * n).astype(np.float32), rs.choice([-1.0, 1.0], E).astype(np.float32)
        ring.append(own, opp, pi, z)
        everything.extend(zip(own, opp, pi, z))
        total = len(everything)
        assert ring.total == total and ring.held == min(total, cap)
        got = ring.read()
        for s in range(ring.held):
            newest = max(k for k in range(total) if k % cap == s)
            want = everything[newest]
            assert got[0][s] == want[0] and got[1][s] == want[1] and np.array_equal(got[2][s], want[2]) and got[3][s] == want[3], (E, s)
    assert ring.total == 368
    ring.clear()
    assert ring.total == 0 and ring.held == 0 and ring.read()[0].size == 0


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define OZ_REPLAY_TARGET_ONEHOT 0" in header and "#define OZ_REPLAY_TARGET_VISITS 1" in header
    assert (_lib.REPLAY_TARGET_ONEHOT, _lib.REPLAY_TARGET_VISITS) == (0, 1)
    assert lib.oz_version() == 230
    assert replay_ref.RECORD_DTYPE == _lib.RECORD_DTYPE


@pytest.mark.parametrize("kw", [dict(replay="x"), dict(replay=None), dict(replay="device", distributed=True),
                                dict(replay="device", dump_examples=True)])
def test_loop_refuses_a_bad_replay_mode_before_any_library_call(kw):
    """(without a GPU the library calls behind these would raise OzLibraryError, and object() is no network: a ValueError shows the check
    came first)"""
    from othellozero_amd import loop
    with pytest.raises(ValueError, match="replay"):
        loop.training(6, 1, 2, 4, 1.0, 1, object(), 0.9, 1, 1, None, False, 1, 2, 1, "unused", 100, **kw)


def test_train_refuses_a_replay_buffer_with_an_allreduce():
    """NNetWrapper.train(ReplayBuffer) is single-process: ValueError before the trainer is touched"""
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.replay import ReplayBuffer
    net, buf = object.__new__(NNetWrapper), object.__new__(ReplayBuffer)
    buf._h = None
    with pytest.raises(ValueError, match="single-process"):
        NNetWrapper.train(net, buf, allreduce=object())
