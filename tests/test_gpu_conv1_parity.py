"""Parity of the inference conv1 kernels (k_conv1; k_conv1_h2; in bf16x3 k_conv1's rows split into three planes) on their own (pytest -m gpu).

The networks run with set_tables(0), so that conv1 is a kernel of its own and its output is materialised; NNetWrapper.activation(0) reads it
(asserted to succeed).  The inputs are 0 / 1 planes, every product is exact, and tests/conv1_ref.py restates the kernels in float32 with an exact
final FMA:
  precision f32 and bf16x3 (three bf16 planes that add up to the float32 value exactly): EQUALITY with the restatement, every channel of every
    pixel of every board, no tolerance (a zero's sign aside: the hook returns float64 values and -0.0 == 0.0);
  precision f16x2: the hook returns (h1 + h2) 2^-e; held to the representation bound of the h2 layout around the same restatement,
    |hook - v32| <= max(2^-22 |v32|, 2^-25 2^-e) per element (conv1_ref.h2_bound; derived there, checked on the CPU by
    tests/test_heads_parity_cpu.py::test_h2_representation_bound), a ReLU zero exactly 0.
For the record every case prints err, E32 and their ratio under layer_ref's statistic, with scale / shift as layer_ref._fold derives them.

Boards (conv1_ref.edge_boards + playouts): the empty board (in f32 and bf16x3 the device's rows must be relu(shift) exactly; in f16x2 the exact
relu(shift) is asserted of the restatement, and the device's rows are held to the h2 bound around it like every other row), all own, all opponent, both checkerboards,
one disc on each of the n^2 squares for own and for the opponent -- every tap at every border -- then playout positions; an odd total, in one call,
and a call of a single board.

Boards with bits outside the n x n square: include/othellozero_amd.h promises NOTHING for them -- oz_net_predict takes "canonical boards", the
conventions say "n x n corner of an 8x8 grid", and neither masking nor refusal is stated (k_conv1_h2 relies on it: "columns >= n are never
occupied").  So there is no test of such boards here."""
import numpy as np
import pytest

import conv1_ref as C1
import heads_ref as H
import layer_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    yield _lib
    _nets.clear()


# (name, precision, board, filters, planes of the network's input: 2 = ONN, 1 = BNN)
CASES = [
    ("f32-8x8-onn", "f32", 8, 128, 2),
    ("f32-6x6-bnn", "f32", 6, 128, 1),
    ("h2-8x8", "f16x2", 8, 256, 2),
    ("h2-6x6", "f16x2", 6, 256, 2),
    ("b3-8x8", "bf16x3", 8, 256, 2),
]
PLAYOUT_BOARDS = {8: 58, 6: 50}        # + 5 + 2 n^2 edge boards = 191 / 127 boards: odd, and >= 128 on 8x8 (precision bf16x3 runs its own kernels from 128 on)
_nets = {}


def _weights(n, C, planes):
    if planes == 2:
        return R.network_weights(n, C, "dense")
    from othellozero_amd.weights import init_weights
    return init_weights(n, seed=2000 + n + C, channels=C, randomize_all=True, in_channels=1)


def _boards(n):
    own, opp = C1.edge_boards(n)
    o2, p2 = H.boards(n, PLAYOUT_BOARDS[n])
    own, opp = np.concatenate([own, o2]), np.concatenate([opp, p2])
    assert own.size % 2 == 1 and not np.any(own & opp)
    return own, opp


def _net(oz, name, precision, n, C, planes):
    from othellozero_amd.NNet import NNetWrapper, NeuralNets
    if name not in _nets:
        own, _ = _boards(n)
        net = NNetWrapper((n, n), num_channels_1=C, max_batch=own.size, weights=_weights(n, C, planes), precision=precision,
                          network=NeuralNets.ONN if planes == 2 else NeuralNets.BNN)
        assert net.arithmetic() == precision
        if precision == "f16x2":
            # the boards are built to hit borders, not to look like play: the low-side guard of f16x2 (a refusal of the CALL, not a change of any
            # number conv1 writes) is switched off for this network
            net.set_option(oz.NET_OPT_LOW_GUARD_LOG2, -100)
            net.commit()
        net.set_tables(0)
        _nets[name] = net
    return _nets[name]


def _check(precision, name, tag, got, w, own, opp, n, aexp):
    want, recomputed = C1.model(w, own, opp, n)
    assert got.shape == want.shape == (own.size * n * n, want.shape[1])
    z = C1.z64(w, own, opp, n)
    err, e32 = R.statistic(got, z), R.statistic(C1.out32(w, own, opp, n), z)
    if precision == "f16x2":
        bound = C1.h2_bound(want, aexp[None, :])
        d = np.abs(got - want.astype(np.float64))
        same = float(np.mean(got == C1.h2_value(want, aexp[None, :])))
        worst = float((d / bound).max())
        print(f"conv1-parity {precision:7s} {name:12s} {tag:6s} boards {own.size:4d}  err {err:.3e}  E32 {e32:.3e}  ratio {err / e32:6.2f}  "
              f"largest |hook - v32| / bound {worst:.3f}, {100 * same:.2f} % equal to h2_planes' split, {recomputed} FMAs rounded exactly")
        assert np.all(d <= bound), f"{int((d > bound).sum())} elements beyond the h2 representation bound, worst {worst:.3f} x"
        assert np.all(got[want == 0] == 0.0)
    else:
        equal = got == want.astype(np.float64)
        print(f"conv1-parity {precision:7s} {name:12s} {tag:6s} boards {own.size:4d}  err {err:.3e}  E32 {e32:.3e}  ratio {err / e32:6.2f}  "
              f"{int((~equal).sum())} of {equal.size} elements differ from the float32 restatement, {recomputed} FMAs rounded exactly")
        assert np.all(equal), f"{int((~equal).sum())} of {equal.size} elements differ, first at {np.argwhere(~equal)[:4].tolist()}, largest {np.abs(got - want).max():.3g}"
    return want


@pytest.mark.parametrize("name,precision,n,C,planes", CASES)
def test_conv1_parity(oz, name, precision, n, C, planes):
    net = _net(oz, name, precision, n, C, planes)
    w = _weights(n, C, planes)
    aexp = net.scaling(0) if precision == "f16x2" else None
    own, opp = _boards(n)
    pi, v = net.predict_batch(own, opp)
    got = net.activation(0)                                         # materialised: the hook must not refuse
    want = _check(precision, name, "all", got, w, own, opp, n, aexp)
    # the empty board (board 0): relu(shift) on every pixel -- of the restatement, and of the device's rows where they are fp32 values (f32, bf16x3)
    _, sh = R._fold(w, 0)
    empty = want.reshape(own.size, n * n, C)[0]
    assert np.array_equal(empty, np.broadcast_to(np.maximum(sh, 0), empty.shape))
    if precision != "f16x2":
        assert np.array_equal(got.reshape(own.size, n * n, C)[0], empty.astype(np.float64))
    # reading changed nothing
    pi2, v2 = net.predict_batch(own, opp)
    assert np.array_equal(pi, pi2) and np.array_equal(v, v2)
    # one board per call: a checkerboard (board 3) and the last playout position; the same rows as in the large call
    for b in (3, own.size - 1):
        net.predict_batch(own[b:b + 1], opp[b:b + 1])
        one = net.activation(0)
        _check(precision, name, f"one:{b}", one, w, own[b:b + 1], opp[b:b + 1], n, aexp)
        assert np.array_equal(one, got.reshape(own.size, n * n, C)[b])
