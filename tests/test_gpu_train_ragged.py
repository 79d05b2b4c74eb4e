"""Short and varying batches on a USED trainer against the float64 oracle (oracle/train_ref.py).

Everywhere else the trainer meets the oracle as a fresh object that steps exactly max_batch boards.  Training does neither: fit() and
NNetWrapper.train() run full batches and then a short last one on the same object, down to one board.  After a full step every buffer sized
for the capacity (activations, the zero-bordered dz, the packed h2 / b3 operands, the octet images, the split-K and row-split partials) holds
the previous batch's rows beyond *d_count, the bf16x3 GEMMs are launched for the capacity with few live rows, and the kernel of most launches
changes with the live batch.  The tests here step one trainer through batch sizes on both sides of those thresholds, after a step that left
large unrelated values in every row, and compare every step with autograd.

Tolerances are the suite's own (test_gpu_train.py): losses and outputs 2e-5 (5e-5 step-locked), gradients 3e-4 * max|g| + 1e-7 per tensor,
step-locked weights and moving statistics 2e-6, gradients that are exactly 0 in exact arithmetic <= 1e-5 absolute.

A step of ONE board: the dense BatchNormalizations see M = 1 (variance 0, xhat 0), so dz of fc2 is exactly 0 and with it the true gradient of
every tensor below fc2's beta (indices 0 .. 32); 33 and 36 .. 39 are not.  tests/test_train_cpu.py pins the oracle's side of that.

Measured on one MI355X when these tests were written (test_short_steps_on_a_used_trainer_match_autograd, over all its cases):
  * worst gradient error / tolerance over the short steps: f32 0.435, f16x2 0.144, bf16x3 0.686 -- all three at B = 2, where the dense BNs
    have xhat = +-1 and the gradients below them survive only through eps (max |g| 57 .. 166 instead of 1 .. 10); without B = 2:
    f32 0.086 (B = 3), f16x2 0.048, bf16x3 0.161 (B = 5 at capacity 512)
  * B = 1: every true-zero tensor is exactly 0.0 on the GPU in all three precisions, no range error in f16x2
  * the full batch after the short steps reproduces its first run bit for bit in every case
The biases behind a BN (BN_BIASES, <= 1e-5 absolute in _check_grads) at B = 2: the one-launch BN backward (k_t_bn_bwd_fused, at most 256 rows) used
  to leave 1.38e-5 (f32, 8x8, capacity 40), 1.75e-5 (f32, 6x6, capacity 40) and 1.91e-5 (f16x2, 8x8, capacity 72) in conv1's bias gradient
  (tensor 1), the column sum of dz, 0 in exact arithmetic.  With 2 boards the gradients below the dense BNs are large (|dbeta| of conv1 2.4 ..
  6.7 against <= 0.65 at every other B) and the fp32 errors that all rows of a column share -- the rounding of sum dy, and the forward pass's
  rounded mean inside xhat -- are multiplied by gamma * rstd^2 (~1000 on conv1) and by the row count.  The kernel now forms its sums
  and dz in float64 around the float64 mean of z.  Measured after that, largest |bias gradient behind a BN| over all steps of all cases:
  3.3e-6 (f32), 4.0e-6 (f16x2), 2.7e-6 (bf16x3), each at B = 5 (the two-launch path); at most 1.3e-6 at B = 2 and 0.0 at B = 1.
"""
import types

import numpy as np
import pytest

from test_gpu_train import BN_BIASES, _batch, _both, _check_grads, _pair

pytestmark = pytest.mark.gpu

SEED, DROPOUT, CLIP = 77, 0.3, 0.5          # what _pair gives the trainer
ZERO_TOL = 1e-5                             # a gradient that is exactly 0 in exact arithmetic (the bound of BN_BIASES)


def _check_grads_zero_aware(ref, gpu):
    """_check_grads, with the tensors whose oracle gradient is identically 0 (a one-board step) asserted <= ZERO_TOL instead of being given
    the relative tolerance of max|g| = 0; -> (worst err / tol of the others, largest |GPU value| on a true-zero tensor, number of those)"""
    g = gpu.get_grads()
    zero = [i for i, gr in ref.grads.items() if i not in BN_BIASES and float(gr.abs().max()) == 0.0]
    zmax = 0.0
    for i in zero:
        m = float(np.abs(g[i]).max())
        assert np.isfinite(g[i]).all() and m <= ZERO_TOL, f"gradient {i} is exactly 0 for this batch, the GPU gave max |g| {m:.3e}"
        zmax = max(zmax, m)
    rest = types.SimpleNamespace(grads={i: gr for i, gr in ref.grads.items() if i not in zero})
    return _check_grads(rest, gpu), zmax, len(zero)


def _step_vs_oracle(gpu, weights, batch, n, seed=SEED, dropout=DROPOUT, clip=CLIP, loss_tol=2e-5, ref=None):
    """one forward_backward of `batch` on `gpu` (whatever it ran before) against a fresh oracle at `weights`: losses, outputs, every gradient.
    -> (losses, grads, worst gradient err / tol, largest value on a true-zero tensor)"""
    from oracle.train_ref import TrainRef
    if ref is None:
        ref = TrainRef(weights, n, lr=1e-3, clipvalue=clip, dropout=dropout, seed=seed)
    ref.step = gpu.step                                    # the dropout mask is keyed on the step
    B = len(batch[3])
    lg, lr_ = _both(ref, gpu, batch)                       # (ReLU masks from gpu.activation(l, B) at the live B)
    assert np.isfinite(lg).all() and np.allclose(lg, lr_, atol=loss_tol, rtol=loss_tol), (B, lg, lr_)
    p, v = gpu.outputs(B)
    assert np.abs(p - ref.outputs["p"]).max() <= 2e-5 and np.abs(v - ref.outputs["v"]).max() <= 2e-5, B
    worst, zmax, nzero = _check_grads_zero_aware(ref, gpu)
    if B == 1:
        assert nzero == 17, nzero                          # every trainable tensor below fc2's beta: 0 .. 32 without the six BN biases
    return lg, gpu.get_grads(), worst, zmax


def _poison(gpu, n, cin, seed):
    """a full batch with z * 500: every row of every buffer up to the capacity then holds large, unrelated values (and, in f16x2, dzmax is large)"""
    own, opp, pi, z = _batch(n, gpu.max_batch, seed, cin)
    losses = gpu.forward_backward(own, opp, pi, z * 500.0)
    assert np.isfinite(losses).all() and losses[2] > 1e5                         # (v - +-500)^2: the step really was a large one


def _same_step(a, b, what):
    (la, ga), (lb, gb) = a, b
    assert la == lb, (what, la, lb)
    for i in ga:
        assert np.array_equal(ga[i], gb[i]), f"{what}: gradient {i} differs"


# (precision, n, C, cin, Bmax, [(B, why this B)]) -- the smallest shapes that reach each branch.  P = pixels per board of a layer.
RAGGED = [
    pytest.param("f32", 8, 128, 2, 257, [
        (257, "full capacity; above the pixel-major GEMM tile's 256 boards (ceil to 128 no longer within cap + cap / 8)"),
        (256, "pixel-major GEMM tiles (cap >= 256 and tile-filling); conv4's BN backward 4096 rows: RS 64"),
        (255, "below the pixel-major tiles; conv2's forward grid of 128 row tiles: k-split 2"),
        (254, "conv2's forward grid of 127 row tiles: k-split 4"),
        (228, "conv3's BN backward above 8192 rows: RS 256"),
        (227, "conv3's BN backward at most 8192 rows: RS 128"),
        (193, "board-resident weight gradient, an odd board count over its 16 board splits"),
        (192, "first batch of the board-resident weight gradient"),
        (191, "last batch of the tap-per-block weight gradient"),
    ], id="f32-8x8-128-cap257"),
    pytest.param("f32", 8, 128, 2, 130, [
        (129, "conv1-2 BN backward above 8192 rows (RS 256); conv4 BN backward above 2048 rows (RS 64)"),
        (128, "conv1-2 BN backward 8192 rows (RS 128); conv4 2048 rows (RS 32); whole 128-row GEMM tiles"),
        (114, "conv3's BN forward above 4096 rows: streaming reductions"),
        (113, "conv3's BN forward at most 4096 rows: k_t_bn_fwd_fused<64>"),
        (65, "conv1-2 BN forward above 4096 rows: streaming; dense GEMMs above the weight-stream kernel's 64 rows"),
        (64, "conv1-2 BN forward 4096 rows: fused<64>; dense layers on the weight-stream kernel; tap-per-block wgrad msplit 16"),
        (63, "tap-per-block weight gradient of conv2: 126 row tiles, msplit 8"),
        (57, "conv3's BN forward above 2048 rows: fused<64>"),
        (56, "conv3's BN forward at most 2048 rows: fused<32>"),
    ], id="f32-8x8-128-cap130"),
    pytest.param("f32", 8, 128, 2, 40, [
        (33, "conv1-2 BN forward above 2048 rows (fused<64>), BN backward RS 64, S1 256"),
        (32, "conv1-2 BN forward 2048 rows (fused<32>), BN backward RS 32; the reference's batch"),
        (31, "tap-per-block wgrad of conv2 below 64 row tiles: msplit 4"),
        (29, "conv3's BN backward above 1024 rows: RS 32"),
        (28, "conv3's BN backward at most 1024 rows: RS 16"),
        (17, "conv1-2 BN backward above 1024 rows (RS 32); conv4 BN backward above 256 rows (two launches); S1 128"),
        (16, "conv1-2 BN backward 1024 rows (RS 16); conv4 BN backward 256 rows (one launch); S1 64; wgrad msplit 4"),
        (15, "tap-per-block wgrad of conv2 below 32 row tiles: msplit 2"),
        (9, "S1 64; conv3's BN backward 324 rows on the two-launch path"),
        (8, "conv3's BN backward above 256 rows; S1 32; wgrad msplit 2"),
        (7, "conv3's BN backward at most 256 rows (one launch); wgrad msplit 1"),
        (5, "conv1-2 BN backward above 256 rows; conv4 above the weight-stream GEMM's 64 rows; S1 32"),
        (4, "conv1-2 BN backward 256 rows (one launch); conv4 on the weight-stream GEMM (64 rows); S1 16"),
        (3, "S1 16"),
        (2, "S1 8; dense BN with M = 2: xhat = +-1, gradients survive only through eps"),
        (1, "one board: dense BN M = 1, every conv layer on the weight-stream GEMM or a single 128-row tile, true-zero gradients"),
    ], id="f32-8x8-128-cap40"),
    pytest.param("f32", 6, 128, 1, 40, [
        (40, "full capacity, BNN input (one plane of -1 / 0 / +1)"),
        (17, "conv4 (P = 4) above the weight-stream GEMM's 64 rows; conv3 (P = 16) BN backward above 256 rows"),
        (16, "conv4 on the weight-stream GEMM at exactly 64 rows; conv3 BN backward 256 rows (one launch)"),
        (8, "conv1-2 (P = 36) BN backward above 256 rows"),
        (7, "conv1-2 BN backward at most 256 rows (one launch)"),
        (5, "conv3 above the weight-stream GEMM's 64 rows"),
        (4, "conv3 on the weight-stream GEMM at exactly 64 rows"),
        (2, "dense BN with M = 2"),
        (1, "one board on the 6x6 geometry: conv4 BN over 4 rows"),
    ], id="f32-6x6-128-bnn-cap40"),
    pytest.param("f16x2", 8, 256, 2, 72, [
        (72, "full capacity: nine whole octets; conv2's h2 GEMM 36 row tiles, k-split 7"),
        (65, "a ninth octet with one live board; h2 GEMM k-split 7; BN forward streaming"),
        (64, "eight whole octets; h2 GEMM k-split 8; BN forward fused<64>"),
        (57, "k_wgrad_h2 msplit 8 (eight octets); conv2's h2 GEMM 29 row tiles: k-split 8"),
        (56, "k_wgrad_h2 msplit 4 (seven octets); conv2's h2 GEMM 28 row tiles: k-split 9"),
        (41, "a sixth octet with one live board"),
        (40, "five whole octets"),
        (39, "a fifth octet with one empty board"),
        (33, "k_wgrad_h2 with one live board in its fifth octet; conv1-2 BN backward RS 128"),
        (32, "WH_MIN_BATCH: first batch of k_wgrad_h2; conv1-2 BN backward RS 64"),
        (31, "last batch of the fp32 weight gradient in f16x2"),
        (17, "conv1-2 BN backward above 1024 rows: RS 64"),
        (16, "conv1-2 BN backward 1024 rows: RS 32"),
        (9, "conv1-2 BN backward above 512 rows: RS 32"),
        (8, "conv1-2 BN backward 512 rows: RS 16"),
        (7, "conv3's BN backward at most 256 rows (one launch)"),
        (2, "dense BN with M = 2: tiny dz, dzmax small after the poison step's large one"),
        (1, "one board: dzmax of every layer below fc2 is 0, the step must not raise the range error"),
    ], id="f16x2-8x8-256-cap72"),
    pytest.param("f16x2", 6, 256, 1, 48, [
        (48, "full capacity, BNN input, six whole octets on the 6x6 geometry"),
        (33, "k_wgrad_h2 with one live board in its fifth octet, 6x6 rows of 6 / 4 / 2 real pixels"),
        (32, "WH_MIN_BATCH on the 6x6 geometry"),
        (31, "last batch of the fp32 weight gradient"),
        (1, "one board"),
    ], id="f16x2-6x6-256-bnn-cap48"),
    pytest.param("bf16x3", 8, 256, 2, 136, [
        (136, "full capacity: 17 whole octets, k_wgrad_b3 msplit 16"),
        (129, "a 17th octet with one live board"),
        (128, "16 whole octets"),
        (127, "a 16th octet with one empty board"),
        (121, "k_wgrad_b3 msplit 16 (16 octets)"),
        (120, "k_wgrad_b3 msplit 8 (15 octets)"),
        (65, "BN forward streaming; a ninth octet with one live board"),
        (64, "BN forward fused<64>"),
        (57, "k_wgrad_b3 msplit 8 (eight octets)"),
        (56, "k_wgrad_b3 msplit 4 (seven octets)"),
        (33, "a fifth octet with one live board"),
        (32, "the reference's batch"),
        (25, "k_wgrad_b3 msplit 4 (four octets)"),
        (24, "k_wgrad_b3 msplit 2 (three octets)"),
        (9, "k_wgrad_b3 msplit 2 (two octets, the second with one live board)"),
        (8, "k_wgrad_b3 msplit 1: one whole octet"),
        (7, "one partly filled octet"),
        (2, "dense BN with M = 2"),
        (1, "b3 GEMMs and conversions launched for 136 boards with 1 live"),
    ], id="bf16x3-8x8-256-cap136"),
    pytest.param("bf16x3", 6, 256, 1, 48, [
        (48, "full capacity, BNN input"),
        (37, "a partly filled octet on the 6x6 geometry"),
        (8, "one whole octet"),
        (1, "one board"),
    ], id="bf16x3-6x6-256-bnn-cap48"),
    # the launch form of test_bf16x3_step_at_a_large_batch / test_f16x2_step_at_a_large_batch (256 x 256 tiles, unsplit), full and then mostly
    # empty; the float64 oracle of 512 boards x 512 filters is most of a case's time, so the full step is a case of its own
    pytest.param("bf16x3", 8, 512, 2, 512, [
        (512, "full capacity on the used trainer: the 256 x 256 b3 tile"),
    ], id="bf16x3-8x8-512-cap512-full"),
    pytest.param("bf16x3", 8, 512, 2, 512, [
        (37, "37 live boards in a launch shaped for 512"),
        (5, "one partly filled octet in a launch shaped for 512"),
        (1, "one live board in a launch shaped for 512"),
    ], id="bf16x3-8x8-512-cap512-short"),
    pytest.param("f16x2", 8, 512, 2, 512, [
        (512, "full capacity on the used trainer: the 256 x 256 ping-pong h2 tile"),
    ], id="f16x2-8x8-512-cap512-full"),
    pytest.param("f16x2", 8, 512, 2, 512, [
        (37, "k_wgrad_h2 with a partly filled fifth octet; the h2 GEMMs shaped for 37 boards after 512"),
        (5, "the fp32 weight gradient after k_wgrad_h2"),
        (1, "one board after 512"),
    ], id="f16x2-8x8-512-cap512-short"),
]


@pytest.mark.parametrize("precision,n,C,cin,Bmax,sizes", RAGGED)
def test_short_steps_on_a_used_trainer_match_autograd(precision, n, C, cin, Bmax, sizes):
    """One trainer of capacity Bmax, weights set once, no apply() (the step counter and with it the dropout mask stay fixed): a poison step, a
    full batch, then a batch of every B in the list -- each against the oracle -- and the full batch again, which must reproduce its first
    run bit for bit: a short step leaves nothing behind (the reductions are fixed-order)."""
    ref0, gpu = _pair(n, C, cin, Bmax, seed=3, precision=precision)
    w = ref0.weights()
    _poison(gpu, n, cin, seed=901)
    full = _batch(n, Bmax, 11, cin)
    first = (gpu.forward_backward(*full), gpu.get_grads())
    worst = zmax = 0.0
    failed = []                                            # every B runs, whatever an earlier one did: a wrong step is reported with its B
    for k, (B, _why) in enumerate(sizes):
        assert 1 <= B <= Bmax
        try:
            _, _, e, zm = _step_vs_oracle(gpu, w, _batch(n, B, 100 + k, cin), n)
            worst, zmax = max(worst, e), max(zmax, zm)
        except AssertionError as err:
            failed.append(f"B = {B}: {str(err).splitlines()[0]}")
    _same_step(first, (gpu.forward_backward(*full), gpu.get_grads()), "the full batch after the short steps")
    assert gpu.step == 0
    print(f"\nragged {precision} n={n} C={C} cap={Bmax}: worst gradient err / tol {worst:.3f}, largest value on a true-zero tensor {zmax:.3e}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("precision,C", [("f32", 128), ("f16x2", 256), ("bf16x3", 256)])
def test_adam_steps_and_moving_statistics_match_with_varying_batch(precision, C):
    """test_adam_steps_and_moving_statistics_match on one trainer of capacity 16 whose batch changes every step (16, 5, 16, 1, 9, 2): gradients
    against autograd at the matched weights, both sides apply the GPU's gradients, all 40 arrays within 2e-6.  Pins the unbiased-variance
    factor M / (M - 1), the staged moving statistics and the rebuilt packed weight operands at the LIVE M, M = 1 of the dense BNs included."""
    import torch
    n, Bmax = 6, 16
    ref, gpu = _pair(n, C, 2, Bmax, seed=5, precision=precision)
    w0 = ref.weights()
    sizes = [16, 5, 16, 1, 9, 2]
    for s, B in enumerate(sizes):
        _step_vs_oracle(gpu, None, _batch(n, B, 20 + s), n, loss_tol=5e-5, ref=ref)
        assert ref.step == s
        ref.apply(grads={i: torch.tensor(g.astype(np.float64)) for i, g in gpu.get_grads().items()})
        gpu.apply()
        wr, wg = ref.weights(), gpu.get_weights()
        for i in range(40):
            err = np.abs(wg[i].astype(np.float64) - wr[i]).max()
            assert err <= 2e-6, f"step {s} (batch {B}), weight {i}: {err:.3e}"
    assert gpu.step == len(sizes)
    assert np.abs(wg[6] - w0[6]).max() > 5e-4                 # the steps really moved the weights (~lr per element per step)
    assert np.abs(wg[4] - w0[4]).max() > 1e-4 and np.abs(wg[29] - w0[29]).max() > 1e-4      # moving statistics too


@pytest.mark.parametrize("precision,C", [("f32", 128), ("f16x2", 256), ("bf16x3", 256)])
def test_a_step_does_not_depend_on_the_trainers_past(precision, C):
    """trainer A runs a poison step, a 7-board step and a 33-board step with z * 500, then batch X (33 boards) and batch Y (9 boards); trainer B
    is fresh (same capacity, seed, weights) and runs only X and Y: losses and every gradient of X and of Y are bit-equal between the two, and A's
    match the oracle.  6x6 / capacity 33: reaches k_wgrad_h2, leaves a partly filled octet, has both 'valid' layers; dropout on, no apply()."""
    n, Bmax = 6, 33
    ref0, a = _pair(n, C, 2, Bmax, seed=9, precision=precision)
    w = ref0.weights()
    _, b = _pair(n, C, 2, Bmax, seed=9, precision=precision)
    X, Y = _batch(n, 33, 21), _batch(n, 9, 22)
    _poison(a, n, 2, seed=902)
    a.forward_backward(*_batch(n, 7, 23))
    own, opp, pi, z = _batch(n, 33, 24)
    a.forward_backward(own, opp, pi, z * 500.0)
    for name, batch in (("X", X), ("Y", Y)):
        la, ga, _, _ = _step_vs_oracle(a, w, batch, n)
        _same_step((la, ga), (b.forward_backward(*batch), b.get_grads()), f"batch {name} on the used and on the fresh trainer")
