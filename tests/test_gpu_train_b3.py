"""Trainer precision "bf16x3": the 3x3 layers' forward, data gradient and weight gradient with every fp32 operand carried exactly as
three bf16 planes on the bf16 matrix cores (six products per fp32 product, fp32 accumulation).  Compared with oracle/train_ref.py (the
float64 autograd restatement) at the exact-fp32 trainer's tolerances: losses and outputs 2e-5, gradients 3e-4 * max|g| + 1e-7 per tensor.
"""
import numpy as np
import pytest

from test_gpu_train import BN_BIASES, DP_WORKER, _batch, _both, _check_grads, _pair

pytestmark = pytest.mark.gpu


KERNELS = [0, 6, 12, 18, 24, 30, 36, 38]      # the kernel tensor of every layer (conv1..4, fc1, fc2, policy and value heads)


def _grad_errors(ref, gpu):
    """{index: max |error| / tolerance} of every trainable tensor but the BN-shadowed biases"""
    g, out = gpu.get_grads(), {}
    for i, gr in ref.grads.items():
        if i in BN_BIASES:
            continue
        gr = gr.numpy()
        out[i] = np.abs(g[i].astype(np.float64) - gr).max() / (3e-4 * np.abs(gr).max() + 1e-7)
    return out


def _step_matches(ref, gpu, batch, check=True):
    lg, lr_ = _both(ref, gpu, batch)
    assert np.allclose(lg, lr_, atol=2e-5, rtol=2e-5), (lg, lr_)
    B = len(batch[3])
    p, v = gpu.outputs(B)
    assert np.abs(p - ref.outputs["p"]).max() <= 2e-5 and np.abs(v - ref.outputs["v"]).max() <= 2e-5
    if check:
        _check_grads(ref, gpu)
    return _grad_errors(ref, gpu)


@pytest.mark.parametrize("n,C,cin,B", [(8, 256, 2, 32), (8, 512, 2, 37), (6, 512, 1, 64), (6, 256, 1, 37), (8, 512, 1, 64), (6, 256, 2, 32)])
def test_forward_backward_bf16x3_matches_autograd(n, C, cin, B):
    """both board sizes, 256 / 512 filters, ONN / BNN, a partly filled octet (37): the f32 trainer's tolerances, and a worst kernel-gradient
    error no more than twice the f32 trainer's on the same batch.  (Kernel tensors: a one-element bias such as the value head's is a sum of B
    terms that cancel, so its error is rounding-level noise of the forward amplified by the cancellation, large or small by chance on either
    side.  Below 1/50 of the tolerance both are noise: floor 0.02.)"""
    batch = _batch(n, B, 11, cin)
    ref, gpu = _pair(n, C, cin, B, seed=3, precision="bf16x3")
    e_b3 = _step_matches(ref, gpu, batch)
    ref32, gpu32 = _pair(n, C, cin, B, seed=3, precision="f32")
    e_f32 = _step_matches(ref32, gpu32, batch)
    worst_b3, worst_f32 = max(e_b3[i] for i in KERNELS), max(e_f32[i] for i in KERNELS)
    assert worst_b3 <= 2 * max(worst_f32, 0.02), (worst_b3, worst_f32)


def test_bf16x3_step_at_a_large_batch():
    """512 boards x 512 filters: unsplit GEMMs on the 256 x 256 tile for the 'valid' layers, the weight gradient's board splits; same
    tolerances; a second call reproduces the first bit for bit"""
    n, C, B = 8, 512, 512
    ref, gpu = _pair(n, C, 2, B, seed=2, precision="bf16x3")
    batch = _batch(n, B, 5)
    lg, lr_ = _both(ref, gpu, batch)
    assert np.allclose(lg, lr_, atol=2e-5, rtol=2e-5), (lg, lr_)
    _check_grads(ref, gpu)
    g1 = gpu.get_grads()
    l2 = gpu.forward_backward(*batch)
    g2 = gpu.get_grads()
    assert lg == l2 and all(np.array_equal(g1[i], g2[i]) for i in g1)


def test_bf16x3_adam_steps_and_moving_statistics_match():
    """step-locked Adam and BN moving statistics (test_adam_steps_and_moving_statistics_match in bf16x3): the b3 weight operands are
    rebuilt from the moved weights after every step"""
    import torch
    n, C, B, steps = 6, 256, 8, 4
    ref, gpu = _pair(n, C, 2, B, seed=5, precision="bf16x3")
    w0 = ref.weights()
    for s in range(steps):
        lg, lr_ = _both(ref, gpu, _batch(n, B, 20 + s))
        assert np.allclose(lg, lr_, atol=5e-5, rtol=5e-5), (s, lg, lr_)
        _check_grads(ref, gpu)
        ref.apply(grads={i: torch.tensor(g.astype(np.float64)) for i, g in gpu.get_grads().items()})
        gpu.apply()
        wr, wg = ref.weights(), gpu.get_weights()
        for i in range(40):
            err = np.abs(wg[i].astype(np.float64) - wr[i]).max()
            assert err <= 2e-6, f"step {s}, weight {i}: {err:.3e}"
    assert gpu.step == steps
    assert np.abs(wg[6] - w0[6]).max() > 5e-4
    assert np.abs(wg[4] - w0[4]).max() > 1e-4 and np.abs(wg[29] - w0[29]).max() > 1e-4


def test_bf16x3_determinism():
    """two trainers with the same seed and batches hold bit-identical weights after several steps; a repeated step on the same state
    gives bit-identical gradients (fixed-order k-split reduces and board-split sums)"""
    from othellozero_amd.trainer import Trainer
    from othellozero_amd.weights import init_weights
    n, C, B, steps = 8, 256, 37, 3
    w = init_weights(n, seed=4, channels=C, randomize_all=True)
    runs = []
    for _ in range(2):
        t = Trainer(n, C, 2, max_batch=B, seed=13, precision="bf16x3")
        t.set_weights(w)
        for s in range(steps):
            t.forward_backward(*_batch(n, B, 60 + s))
            t.apply()
        runs.append(t)
    wa, wb = runs[0].get_weights(), runs[1].get_weights()
    assert all(np.array_equal(a, b) for a, b in zip(wa, wb))
    batch = _batch(n, B, 99)
    l1 = runs[0].forward_backward(*batch)
    g1 = runs[0].get_grads()
    l2 = runs[0].forward_backward(*batch)
    g2 = runs[0].get_grads()
    assert l1 == l2 and all(np.array_equal(g1[i], g2[i]) for i in g1)


@pytest.mark.parametrize("N", [75, 65])      # 65 = 4 * 16 + 1: the last batch of every epoch is ONE board
def test_bf16x3_resident_dataset_fit_equals_stepwise_fit(N):
    from othellozero_amd.trainer import Trainer, fit
    from othellozero_amd.weights import init_weights
    n, bs, C = 6, 16, 256
    own, opp, pi, z = _batch(n, N, seed=77)
    runs = []
    for resident in (False, True):
        tr = Trainer(n, C, 2, max_batch=bs, seed=9, precision="bf16x3")
        tr.set_weights(init_weights(n, seed=1, channels=C))
        h = fit(tr, own, opp, pi, z, batch_size=bs, epochs=2, shuffle_seed=5, resident=resident)
        runs.append((tr.get_weights(), h.history, tr.step))
    (w0, h0, s0), (w1, h1, s1) = runs
    assert s0 == s1 == 2 * 5
    assert all(np.array_equal(a, b) for a, b in zip(w0, w1))
    for k in h0:
        assert np.isfinite(h0[k]).all() and np.isfinite(h1[k]).all(), (k, h0[k], h1[k])
        assert np.allclose(h0[k], h1[k], rtol=1e-6, atol=1e-7), (k, h0[k], h1[k])


def test_bf16x3_data_parallel_two_ranks_equal_hand_averaged_gradients(tmp_path):
    """GradientAllReduce + fit on two ranks (gloo, both on GPU 0) in bf16x3: identical weights across ranks, equal bit for bit to a
    single-process run that averages the two gradient arenas by hand"""
    import os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    select = 'C = 256 if precision == "f16x2" else 128'
    assert DP_WORKER.count(select) == 1
    script = tmp_path / "dp_gpu_worker_b3.py"
    script.write_text(DP_WORKER.replace(select, "C = 256"))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), root, "bf16x3"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"RANK_OK {rank}" in out, out


def test_bf16x3_has_no_range_path():
    """the weights and batch that make the f16x2 trainer raise its range error (activations ~1e7): bf16x3 carries fp32's exponent range,
    so the step succeeds and matches the float64 oracle at the f32 tolerances -- except where the exact-fp32 trainer does not either
    (conv1's kernel gradient becomes a cancelling sum of ~1e7-scale terms here): there no more than twice the f32 trainer's error"""
    from oracle.train_ref import TrainRef
    from othellozero_amd.trainer import Trainer
    from othellozero_amd.weights import init_weights
    n, C, B = 6, 256, 16
    w = init_weights(n, seed=5, channels=C, randomize_all=True)
    big = [a.copy() for a in w]
    big[2] = big[2] * 1e7                                     # gamma of the first BN: activations ~1e7
    batch = _batch(n, B, 3)
    errs = {}
    for prec in ("bf16x3", "f32"):
        ref = TrainRef(big, n, lr=1e-3, clipvalue=0.5, dropout=0.0, seed=1)
        gpu = Trainer(n, C, 2, max_batch=B, lr=1e-3, clipvalue=0.5, dropout=0.0, seed=1, precision=prec)
        gpu.set_weights(big)
        errs[prec] = _step_matches(ref, gpu, batch, check=False)
        if prec == "bf16x3":
            assert gpu.activation(0, B).max() > 1e6           # (the construction really leaves the fp16 range)
    for i, e in errs["bf16x3"].items():
        assert e <= max(1.0, 2 * errs["f32"][i]), (i, e, errs["f32"][i])


def _examples(n, N, seed):
    rs = np.random.RandomState(seed)
    examples = []
    for _ in range(N):
        occ = rs.rand(n, n) < 0.7
        black = occ & (rs.rand(n, n) < 0.5)
        pol = np.zeros((n, n))
        pol[rs.randint(n), rs.randint(n)] = 1
        examples.append((np.stack([black, occ & ~black], axis=2), pol, int(rs.choice([-1, 1]))))
    return examples, rs


def test_nnetwrapper_trains_in_bf16x3_and_the_default_mapping_is_unchanged():
    """train_precision="bf16x3" trains in bf16x3 (hist.train_precision), the trained weights evaluated by the bf16x3 network match the
    float64 forward within 1e-5; without train_precision the same wrapper trains in f32, an f16x2 wrapper of 256 filters in f16x2"""
    from oracle import nn_numpy
    from othellozero_amd.NNet import NNetWrapper
    n = 6
    examples, rs = _examples(n, 128, 5)
    net = NNetWrapper((n, n), num_channels_1=256, batch_size=32, epochs=5, max_batch=128, precision="bf16x3", train_precision="bf16x3")
    hist = net.train(examples)                                             # 20 Adam steps
    assert hist.train_precision == "bf16x3" and np.isfinite(hist.history["loss"]).all()
    w = net.get_weights()
    valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
    own = rs.randint(0, 2**63, size=64, dtype=np.uint64) & valid
    opp = rs.randint(0, 2**63, size=64, dtype=np.uint64) & valid & ~own
    pi, v = net.predict_batch(own, opp)
    pr, vr = nn_numpy.forward(w, own, opp, n)
    assert np.abs(pi.reshape(64, -1) - pr).max() <= 1e-5 and np.abs(v - vr).max() <= 1e-5
    assert np.abs(np.asarray(w[4])).max() > 1e-3 and np.abs(np.asarray(w[5]) - 1).max() > 1e-3     # BN statistics moved
    small = examples[:32]
    plain = NNetWrapper((n, n), num_channels_1=256, batch_size=32, epochs=1, max_batch=128, precision="bf16x3")
    assert plain.train(small).train_precision == "f32"
    h2 = NNetWrapper((n, n), num_channels_1=256, batch_size=32, epochs=1, max_batch=4, precision="f16x2")
    assert h2.train(small).train_precision == "f16x2"


def test_bf16x3_refusals():
    """bf16x3 needs channels % 256 == 0 (k_gemm_b3's column tile); mode 3 does not exist"""
    from othellozero_amd import _lib
    from othellozero_amd.trainer import Trainer
    with pytest.raises(_lib.OzError) as e:
        Trainer(6, 128, 2, max_batch=8, precision="bf16x3")
    assert "channels % 256" in str(e.value) and "bf16x3" in str(e.value)
    t = Trainer(6, 256, 2, max_batch=8)
    with pytest.raises(_lib.OzError):
        _lib.check(_lib.load().oz_trainer_set_precision(t._h, 3))
