"""Auxiliary heads on the GPU (pytest -m gpu): the trainer's ownership and score heads against the float64 autograd restatement
(tests/aux_heads_ref.py: AuxTrainRef), per-kernel parity of the aux kernels from the device's own tensors, non-interference with the forty
gradients, Adam steps on all 44 arrays, the replay buffer's final pairs against the host definition, checkpoints and the training loop.

Tolerances are tests/test_gpu_train.py's: losses atol = rtol = 2e-5, outputs 2e-5, gradients max|d| <= 3e-4 max|g_ref| + 1e-7 per tensor
(_check_grads), the step-locked Adam test's 5e-5 / 2e-6; the per-kernel margins are aux_heads_ref.MARGIN (x E32; held to the models by
tests/test_aux_heads_cpu.py).  Everything about the pairs and the files is compared bit for bit."""
import math

import numpy as np
import pytest

import aux_heads_ref as R
import optimizer_ref as O
import train_kernel_ref as K
from test_gpu_train import _batch, _check_grads

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
WEIGHTS = (1.0, 0.25)


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _weights(n, C, cin, seed):
    from othellozero_amd.weights import init_weights
    return list(init_weights(n, seed=seed, channels=C, randomize_all=True, in_channels=cin)) + R.glorot_aux(n, seed + 100)


def _gpu(n, C, cin, B, w, weights=WEIGHTS, precision="f32", dropout=0.3, clip=0.5, **kw):
    from othellozero_amd.trainer import Trainer
    aux = None if weights is None else dict(ownership=weights[0], score=weights[1])
    gpu = Trainer(n, C, cin, max_batch=B, lr=1e-3, clipvalue=clip, dropout=dropout, seed=77, precision=precision, aux_heads=aux, **kw)
    gpu.set_weights(w if aux else w[:40])
    return gpu


def _pair(n, C, cin, B, weights=WEIGHTS, precision="f32", seed=3, **kw):
    w = _weights(n, C, cin, seed)
    ref = R.AuxTrainRef(w, n, weights[0], weights[1], lr=1e-3, clipvalue=0.5, dropout=0.3, seed=77)
    return ref, _gpu(n, C, cin, B, w, weights, precision, **kw), w


def _both(ref, gpu, batch, fin):
    """GPU step first, then the restatement with the GPU's ReLU decisions near the kink (test_gpu_train._both)"""
    own, opp, pi, z = batch
    lg = gpu.forward_backward(own, opp, pi, z, fin[0], fin[1])
    masks = [(gpu.activation(l, len(z)) > 0).astype(np.float64) for l in range(6)]
    lr_ = ref.forward_backward(own, opp, pi, z, fin[0], fin[1], relu_masks=masks)
    return lg, lr_


# ------------------------------------------------------------------ 1. a step against autograd
@pytest.mark.parametrize("n,C,cin,B,precision", [(6, 128, 2, 8, "f32"), (8, 128, 2, 5, "f32"), (6, 128, 1, 7, "f32"),
                                                 (8, 256, 2, 32, "f16x2"), (8, 256, 2, 32, "bf16x3")])
def test_step_matches_autograd(oz, n, C, cin, B, precision):
    ref, gpu, _ = _pair(n, C, cin, B, precision=precision)
    batch, fin = _batch(n, B, 11, cin), R.final_pairs(n, B, 13)
    m = R.masks(*fin)
    assert (m == 0).any() and (m == 1).any()
    lg, lr_ = _both(ref, gpu, batch, fin)
    print("losses gpu", lg, "ref", lr_)
    assert len(lg) == 5 and np.allclose(lg, lr_, atol=2e-5, rtol=2e-5), (lg, lr_)
    assert lr_[3] > 1e-3 and lr_[4] > 1e-4                                   # both heads are really trained on something
    p, v = gpu.outputs(B)
    o, s = gpu.aux_outputs(B)
    errs = [np.abs(p - ref.outputs["p"]).max(), np.abs(v - ref.outputs["v"]).max(), np.abs(o - ref.outputs["o"]).max(), np.abs(s - ref.outputs["s"]).max()]
    print("output errors p v o s", errs)
    assert max(errs) <= 2e-5
    worst = _check_grads(ref, gpu)
    print("worst gradient err / tol", worst)
    assert set(gpu.get_grads()) == set(ref.grads) and len(ref.grads) == 32
    # a second call repeats the first bit for bit
    g1 = gpu.get_grads()
    l2 = gpu.forward_backward(*batch, *fin)
    g2 = gpu.get_grads()
    assert l2 == lg and all(np.array_equal(g1[i], g2[i]) for i in g1)
    assert np.array_equal(gpu.aux_outputs(B)[0], o)


# ------------------------------------------------------------------ 2. per-kernel parity from the device's own tensors
def _stat(kind, got, r32, r64):
    if kind == "rows":
        return K.statistic(got, r64)[0], K.statistic(r32, r64)[0]
    err, e32 = K.statistic(K.vec(got), K.vec(r64))[0], K.statistic(K.vec(r32), K.vec(r64))[0]
    return err, max(e32, K.E32_FLOOR) if kind == "small" else e32


@pytest.mark.parametrize("n,B", [(6, 5), (8, 5), (8, 32)])
def test_aux_kernel_parity(oz, n, B):
    """k_t_aux_heads, the weight and bias gradients, k_t_heads_dgrad's adding launch and the batch means, each from the device's own inputs of the step"""
    C = 128
    w = _weights(n, C, 2, 5)
    gpu = _gpu(n, C, 2, B, w)
    gpu.set_capture(True)
    batch, fin = _batch(n, B, 21), R.final_pairs(n, B, 23)
    losses = gpu.forward_backward(*batch, *fin)
    a5 = gpu.activation(5, B).reshape(B, 512)
    o, s = gpu.aux_outputs(B)
    dopre, dspre, df2_before = gpu.aux_head_grads(B, before=True)
    df2_after = gpu.dgrad(5, B).reshape(B, 512)
    args = (a5, w[40], w[41], w[42], w[43], fin[0], fin[1], n, WEIGHTS[0], WEIGHTS[1])
    h64, h32 = R.aux_heads(*args, F64), R.aux_heads(*args, F32)
    recs = [("aux_o", "rows", o, h32["o"], h64["o"]), ("aux_s", "vec", s, h32["s"], h64["s"]),
            ("aux_dopre", "rows", dopre, h32["dopre"], h64["dopre"]), ("aux_dspre", "vec", dspre, h32["dspre"], h64["dspre"]),
            ("aux_loss", "small", np.array(losses[3:], F32), R.aux_mean_losses(h32["lo"], h32["ls"], F32), R.aux_mean_losses(h64["lo"], h64["ls"], F64))]
    r64, r32 = R.aux_reduce(a5, dopre, dspre, F64), R.aux_reduce(a5, dopre, dspre, F32)
    recs += [("aux_dwown", "rows", gpu.get_grad(40), r32["dwown"], r64["dwown"]), ("aux_dwsc", "vec", gpu.get_grad(42), r32["dwsc"], r64["dwsc"]),
             ("aux_dbown", "vec", gpu.get_grad(41), r32["dbown"], r64["dbown"])]
    term32, term64 = R.aux_dgrad(dopre, dspre, w[40], w[42], F32), R.aux_dgrad(dopre, dspre, w[40], w[42], F64)
    recs += [("aux_df2", "rows", df2_after, (df2_before + term32).astype(F32), df2_before.astype(F64) + term64)]
    bad = []
    for key, kind, got, e, ref in recs:
        err, e32 = _stat(kind, got, e, ref)
        print(f"kernel-parity aux n {n} B {B:3d} {key:10s} err {err:.3e}  E32 {e32:.3e}  ratio {err / e32:6.2f}  margin {R.MARGIN[key]:4.1f}")
        assert e32 > 0
        if not err <= R.MARGIN[key] * e32:
            bad.append((key, err / e32))
    dv = dspre.reshape(-1, 1)
    err, e32 = K.colsum_statistic(gpu.get_grad(43), dv)[0], max(K.colsum_statistic(dv.sum(axis=0, dtype=F32), dv)[0], K.E32_FLOOR)
    print(f"kernel-parity aux n {n} B {B:3d} aux_dbsc   err {err:.3e}  E32 {e32:.3e}  ratio {err / e32:6.2f}  margin {R.MARGIN['aux_dbsc']:4.1f}")
    if not err <= R.MARGIN["aux_dbsc"] * e32:
        bad.append(("aux_dbsc", err / e32))
    assert not bad, f"(tensor, err / E32) above the margin: {bad}"
    # the term really arrived: the sum differs from what the policy and value heads left, and a dead sample's rows are exactly zero
    assert not np.array_equal(df2_after, df2_before)
    dead = R.masks(*fin) == 0
    assert dead.any() and np.all(dopre[dead] == 0.0) and np.all(dspre[dead] == 0.0)
    assert np.array_equal(df2_after[dead], df2_before[dead])


# ------------------------------------------------------------------ 3. non-interference
def test_zero_weights_leave_the_forty_gradients_alone(oz):
    """weights (0, 0): no backward kernel of the heads is launched -- the 40 gradients and three losses are an aux-off trainer's bit for bit, the
    two aux losses still match the restatement, the four aux gradients stay zero"""
    n, C, B = 8, 128, 5
    w = _weights(n, C, 2, 7)
    batch, fin = _batch(n, B, 31), R.final_pairs(n, B, 33)
    off = _gpu(n, C, 2, B, w, weights=None)
    l_off = off.forward_backward(*batch)
    g_off = off.get_grads()
    ref = R.AuxTrainRef(w, n, 0.0, 0.0, lr=1e-3, clipvalue=0.5, dropout=0.3, seed=77)
    on = _gpu(n, C, 2, B, w, weights=(0.0, 0.0))
    l_on, l_ref = _both(ref, on, batch, fin)
    g_on = on.get_grads()
    assert len(l_off) == 3 and l_on[:3] == l_off, (l_on, l_off)
    for i, g in g_off.items():
        assert g.tobytes() == g_on[i].tobytes(), f"gradient {i} differs from the aux-off trainer's"
    assert all(np.all(g_on[i] == 0.0) for i in R.AUX)
    assert l_ref[3] > 1e-3 and np.allclose(l_on[3:], l_ref[3:], atol=2e-5, rtol=2e-5), (l_on, l_ref)


def test_dead_masks_train_nothing(oz):
    """weights (1, 1) and every mask 0 (given as zero pairs, and not given at all): zero aux losses and gradients, and the 40 gradients of an
    aux-off trainer.  k_t_heads_dgrad's second launch then adds a signed zero into every element of df2, and (-0) + (+0) = +0 is another bit pattern than -0 with
    the same value: the comparison of the forty is by value (np.array_equal), which is exact for everything but the sign of a zero"""
    n, C, B = 6, 128, 7
    w = _weights(n, C, 2, 9)
    batch = _batch(n, B, 41)
    off = _gpu(n, C, 2, B, w, weights=None)
    l_off = off.forward_backward(*batch)
    g_off = off.get_grads()
    on = _gpu(n, C, 2, B, w, weights=(1.0, 1.0))
    zero = np.zeros(B, np.uint64)
    for l_on in (on.forward_backward(*batch, zero, zero), on.forward_backward(*batch)):
        g_on = on.get_grads()
        assert l_on[:3] == l_off and l_on[3:] == (0.0, 0.0), (l_on, l_off)
        assert all(np.array_equal(g, g_on[i]) for i, g in g_off.items())
        assert all(np.all(g_on[i] == 0.0) for i in R.AUX)


def test_entry_points_refuse_what_they_must(oz):
    from othellozero_amd.trainer import Trainer
    n, B = 6, 4
    plain = Trainer(n, 128, 2, max_batch=B)
    lib = oz.load()
    own, opp, pi, z = _batch(n, B, 1)
    fo, fp = R.final_pairs(n, B, 2)
    five = np.zeros(5, np.float32)
    rc = lib.oz_trainer_forward_backward_aux(plain._h, oz.p_u64(own), oz.p_u64(opp), oz.p_f32(pi), oz.p_f32(z), oz.p_u64(fo), oz.p_u64(fp), B, oz.p_f32(five))
    assert rc == oz.OZ_ERR_STATE and "auxiliary heads" in lib.oz_last_error().decode()
    assert lib.oz_trainer_set_aux_heads(plain._h, -1.0, 0.0) == oz.OZ_ERR_ARG
    assert lib.oz_trainer_set_aux_heads(plain._h, float("nan"), 0.0) == oz.OZ_ERR_ARG
    assert lib.oz_trainer_set_aux_heads(plain._h, 0.0, float("inf")) == oz.OZ_ERR_ARG
    plain.forward_backward(own, opp, pi, z)
    assert lib.oz_trainer_set_aux_heads(plain._h, 1.0, 1.0) == oz.OZ_ERR_STATE      # after the first step
    assert len(plain.get_weights()) == 40 and Trainer.arena_size(n, 128) == plain.grad_arena()[1]
    aux = Trainer(n, 128, 2, max_batch=B, aux_heads=dict(ownership=1.0, score=1.0))
    assert aux.grad_arena()[1] == Trainer.arena_size(n, 128, aux=True) and len(aux.get_weights()) == 44
    w = aux.get_weights()
    assert np.all(w[41] == 0) and np.all(w[43] == 0) and np.abs(w[40]).max() <= math.sqrt(6.0 / (512 + n * n)) and np.abs(w[40]).max() > 0
    assert np.abs(w[42]).max() <= math.sqrt(6.0 / 513) and np.unique(w[42]).size > 500
    again = Trainer(n, 128, 2, max_batch=B, aux_heads=dict(ownership=0.5, score=2.0))      # the same seed: the same fresh heads
    assert all(np.array_equal(a, b) for a, b in zip(w[40:], again.get_weights()[40:]))
    # an external gradient arena is sized for the forty arrays: the library refuses the heads on it (and so do Trainer and NNetWrapper.train)
    import ctypes as C
    ptr, count = plain.grad_arena()
    assert count == Trainer.arena_size(n, 128)
    ext = C.c_void_p()
    oz.check(lib.oz_trainer_create(C.byref(ext), n, 128, 2, B, 1e-3, 0.5, 0.3, 0.99, 0, C.c_void_p(ptr)))
    try:
        assert lib.oz_trainer_set_aux_heads(ext, 1.0, 1.0) == oz.OZ_ERR_ARG and "external gradient arena" in lib.oz_last_error().decode()
    finally:
        oz.check(lib.oz_trainer_destroy(ext))
    with pytest.raises(ValueError, match="external_grads_ptr"):
        Trainer(n, 128, 2, max_batch=B, external_grads_ptr=ptr, aux_heads=dict(ownership=1.0, score=1.0))
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.trainer import fit_replay
    buf = ReplayBuffer(n, 16)
    buf.append_examples(own, opp, pi, z)
    with pytest.raises(ValueError, match="aux=True"):
        fit_replay(aux, buf, batch_size=B, epochs=1)
    with pytest.raises(oz.OzError) as e:
        aux.fit_epoch_replay(buf, np.arange(4), B)
    assert e.value.code == oz.OZ_ERR_ARG and "oz_replay_create_aux" in str(e.value)
    with pytest.raises(oz.OzError) as e:
        buf.read_aux()
    assert e.value.code == oz.OZ_ERR_STATE


# ------------------------------------------------------------------ 4. Adam on all 44 arrays
def test_two_adam_steps_and_the_global_norm(oz):
    """step-locked as test_gpu_train's multi-step test: both sides apply Adam to the GPU's gradients; then global_clipnorm on a second trainer:
    the norm of step_info() is the float64 norm over all 44 arrays' gradients"""
    import torch
    n, C, B = 8, 128, 5
    ref, gpu, w0 = _pair(n, C, 2, B, seed=5)
    for step in range(2):
        batch, fin = _batch(n, B, 20 + step), R.final_pairs(n, B, 50 + step)
        lg, lr_ = _both(ref, gpu, batch, fin)
        assert np.allclose(lg, lr_, atol=5e-5, rtol=5e-5), (step, lg, lr_)
        _check_grads(ref, gpu)
        ref.apply(grads={i: torch.tensor(g.astype(np.float64)) for i, g in gpu.get_grads().items()})
        gpu.apply()
        wr, wg = ref.weights(), gpu.get_weights()
        assert len(wr) == len(wg) == 44
        for i in range(44):
            err = np.abs(wg[i].astype(np.float64) - wr[i]).max()
            assert err <= 2e-6, f"step {step}, weight {i}: {err:.3e}"
    assert gpu.step == 2
    assert all(np.abs(wg[i] - w0[i]).max() > 5e-4 for i in R.AUX)                  # the steps moved every aux array (~lr per element per step)
    clipped = _gpu(n, C, 2, B, w0, optimizer=dict(global_clipnorm=1e-3))
    batch, fin = _batch(n, B, 20), R.final_pairs(n, B, 50)
    clipped.forward_backward(*batch, *fin)
    grads = clipped.get_grads()
    assert len(grads) == 32
    exact, count = O.exact_sqsum(grads.values())
    without, _ = O.exact_sqsum([grads[i] for i in grads if i < 40])
    clipped.apply()
    info = clipped.step_info()
    assert abs(info["grad_norm"] - np.sqrt(exact)) <= O.norm_bound(count) * np.sqrt(exact)
    assert abs(np.sqrt(without) - np.sqrt(exact)) > 1e3 * O.norm_bound(count) * np.sqrt(exact)      # the aux arrays are a visible part of it
    assert info["clip_scale"] == 1e-3 / info["grad_norm"] < 1.0
    assert abs(clipped.sqsum("gradients") - exact) <= O.norm_bound(count) * exact
    # the fused step moved the last array too (the arena ends inside a 16-byte unit)
    assert clipped.get_weights()[43][0] != w0[43][0]


# ------------------------------------------------------------------ 5. the replay buffer
N, G, SIMS, SEED, EG, SALT = 6, 16, 8, 41, 0.8, 21
RESIGN, CAP = (0.3, 2, 8, 0.25), (4, 0.5)


@pytest.fixture(scope="module")
def played(oz):
    """a small engine run with a resignation rule and a playout cap (the seed: tests/resign_ref.py's games at these settings have 10 adjudicated
    and 6 natural games, 240 fast records -- asserted below, not assumed)"""
    from othellozero_amd.NNet import StubNetWrapper
    from othellozero_amd.training import SelfPlayEngine
    eng = SelfPlayEngine(StubNetWrapper((N, N), SALT, 0, max_batch=G), N, G, SIMS, 1.0, 1.0, EG, seed=SEED, first_game_id=0, record_visits=True,
                         record_values=True, record_surprise=True, resign=RESIGN, playout_cap=CAP)
    eng.play_to_end()
    rec, cnt = eng.records(with_visits=True)
    adjudicated = {int(g) for g in rec["game_id"][oz.record_adjudicated(rec) == 1]}
    natural = {int(g) for g in rec["game_id"]} - adjudicated
    assert adjudicated and natural and (oz.record_fast(rec) == 1).any(), (adjudicated, natural)
    return eng, rec, cnt


def _expected_pairs(rec, copies=None, first_sym=None):
    """the slots' pairs of one append into an empty buffer with room for everything: records in (game_id, ply) order without the fast ones,
    8 symmetries each -- or, weighted, copies[i] examples of record i, example k in symmetry (first_sym[i] + k) & 7"""
    fo, fp = R.aux_target(rec)
    out = []
    for i in range(rec.size):
        if rec["pad"][i, 0] == 1:
            continue
        syms = range(8) if copies is None else [(int(first_sym[i]) + k) & 7 for k in range(int(copies[i]))]
        out += [R.sym_pair(t, N, fo[i], fp[i]) for t in syms]
    return np.array([p[0] for p in out], np.uint64), np.array([p[1] for p in out], np.uint64)


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_replay_buffer_keeps_the_final_pairs(oz, played, tmp_path):
    from othellozero_amd import agents
    from othellozero_amd.replay import ReplayBuffer
    eng, rec, cnt = played
    host = agents.rules_aux_targets(rec)
    assert _same(host, R.aux_target(rec))
    full = oz.record_fast(rec) == 0
    live = full & (oz.record_adjudicated(rec) == 0)
    assert live.any() and (full & ~live).any()
    # plain append from the engine, and the same records from the host: every slot's pair, bit for bit; the four arrays are a plain buffer's
    E = 8 * int(full.sum())
    want = _expected_pairs(rec)
    assert want[0].size == E and ((want[0] | want[1]) != 0).sum() == 8 * int(live.sum())
    for alias in (False, True):
        aux, plain = ReplayBuffer(N, E + 3, aux=True), ReplayBuffer(N, E + 3)
        assert aux.append_engine(eng, alias_final=alias) == plain.append_engine(eng, alias_final=alias) == int(full.sum())
        assert _same(aux.read_aux(), want) and _same(aux.read(), plain.read()) and aux.info() == plain.info()
    sub = np.sort(np.random.RandomState(3).permutation(rec.size)[:64])                  # 64 records through the host entry points
    sub_rec, sub_cnt = np.ascontiguousarray(rec[sub]), np.ascontiguousarray(cnt[sub])
    assert (sub_rec["pad"][:, 0] == 1).any() and (sub_rec["pad"][:, 1] == 1).any() and ((sub_rec["pad"][:, 0] == 0) & (sub_rec["pad"][:, 1] == 0)).any()
    aux, plain = ReplayBuffer(N, 8 * 64, aux=True), ReplayBuffer(N, 8 * 64)
    for buf in (aux, plain):
        buf.append_records(sub_rec, visits=sub_cnt, policy_target="visits")
    assert _same(aux.read_aux(), _expected_pairs(sub_rec)) and _same(aux.read(), plain.read())
    vals = np.linspace(-1, 1, 64).astype(np.float32)
    aux2, plain2 = ReplayBuffer(N, 8 * 64, aux=True), ReplayBuffer(N, 8 * 64)
    for buf in (aux2, plain2):
        buf.append_records(sub_rec, values=vals)
    assert _same(aux2.read_aux(), _expected_pairs(sub_rec)) and _same(aux2.read(), plain2.read())
    # the weighted append: copies and first symmetries as the engine computed them
    wa, wp = ReplayBuffer(N, 16 * rec.size, aux=True), ReplayBuffer(N, 16 * rec.size)
    for buf in (wa, wp):
        buf.append_engine(eng, policy_target="visits", surprise_weight=(0.5, 9))
    _, (_, c, t0) = eng.records(with_weights=True)
    assert (c > 8).any() and (c[full] < 8).any() and wa.last_examples == int(c.sum()) == len(wa)
    assert _same(wa.read_aux(), _expected_pairs(rec, c, t0)) and _same(wa.read(), wp.read())
    # a ring smaller than the append (capacity no multiple of 8) keeps the newest examples' pairs in their slots
    cap = E - 8 * 5 - 3
    small = ReplayBuffer(N, cap, aux=True)
    small.append_engine(eng)
    ring = [np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)]
    for e in range(E - cap, E):
        ring[0][e % cap], ring[1][e % cap] = want[0][e], want[1][e]
    assert _same(small.read_aux(), ring)
    # example appends: with the pairs, and without them (zeros); a plain buffer ignores them
    own, opp, pi, z = aux.read()
    fo, fp = aux.read_aux()
    ex = ReplayBuffer(N, 600, aux=True)
    ex.append_examples(own, opp, pi, z, fo, fp)
    ex.append_examples(own[:9], opp[:9], pi[:9], z[:9])
    assert _same(ex.read_aux(), (np.concatenate([fo, np.zeros(9, np.uint64)]), np.concatenate([fp, np.zeros(9, np.uint64)])))
    ign = ReplayBuffer(N, 600)
    ign.append_examples(own, opp, pi, z, fo, fp)
    assert _same(ign.read(), (own, opp, pi, z))
    # save / load: the pairs travel; an old-format file loads with zero pairs; a file with pairs loads into a plain buffer
    small.save(str(tmp_path / "aux.npz"))
    back = ReplayBuffer.load(str(tmp_path / "aux.npz"), aux=True)
    assert back.aux and _same(back.read_aux(), small.read_aux()) and _same(back.read(), small.read()) and back.info() == small.info()
    as_plain = ReplayBuffer.load(str(tmp_path / "aux.npz"))
    assert not as_plain.aux and _same(as_plain.read(), small.read())
    plain.save(str(tmp_path / "old.npz"))
    assert "fin_own" not in np.load(str(tmp_path / "old.npz")).files
    old = ReplayBuffer.load(str(tmp_path / "old.npz"), aux=True)
    assert _same(old.read(), plain.read()) and all(np.all(a == 0) for a in old.read_aux()) and len(old.read_aux()[0]) == len(plain)


def test_fit_replay_equals_fit_on_the_arrays_read_back(oz, played):
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.trainer import fit, fit_replay
    eng, rec, cnt = played
    sub = np.ascontiguousarray(rec[::7])
    buf = ReplayBuffer(N, 8 * sub.size, aux=True)
    buf.append_records(sub)
    own, opp, pi, z = buf.read()
    fo, fp = buf.read_aux()
    assert ((fo | fp) != 0).any() and ((fo | fp) == 0).any() and len(z) % 32 != 0          # live and dead masks, a short last batch
    w = _weights(N, 128, 2, 15)
    a, b, c = (_gpu(N, 128, 2, 32, w) for _ in range(3))
    ha = fit_replay(a, buf, batch_size=32, epochs=1, shuffle_seed=4)
    hb = fit(b, own, opp, pi, z, batch_size=32, epochs=1, shuffle_seed=4, fin_own=fo, fin_opp=fp)
    hc = fit(c, own, opp, pi, z, batch_size=32, epochs=1, shuffle_seed=4, fin_own=fo, fin_opp=fp, resident=False)
    assert list(ha.history) == ["loss", "pi-reshaped_loss", "v_loss", "ownership_loss", "score_loss"]
    assert ha.history == hb.history and ha.history["ownership_loss"][0] > 0 and ha.history["score_loss"][0] > 0
    wa, wb, wc = a.get_weights(), b.get_weights(), c.get_weights()
    assert len(wa) == 44 and all(x.tobytes() == y.tobytes() == v.tobytes() for x, y, v in zip(wa, wb, wc))
    assert any(not np.array_equal(wa[i], w[i]) for i in R.AUX)
    # the step-wise loop accumulates the same per-step float32 losses on the host: equal up to the float64 sum's rounding
    for k in ha.history:
        assert abs(ha.history[k][0] - hc.history[k][0]) <= 1e-6 * max(1.0, abs(ha.history[k][0])), k
    # without the option the history has the keys it had
    plain = _gpu(N, 128, 2, 32, w, weights=None)
    assert list(fit(plain, own, opp, pi, z, batch_size=32, epochs=1).history) == ["loss", "pi-reshaped_loss", "v_loss"]


# ------------------------------------------------------------------ 6. checkpoints and the loop
def test_checkpoints_carry_the_heads_and_the_inference_network_ignores_them(oz, played, tmp_path):
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.replay import ReplayBuffer
    eng, rec, cnt = played
    buf = ReplayBuffer(N, 8 * 40, aux=True)
    buf.append_records(np.ascontiguousarray(rec[::11][:40]))
    on = dict(ownership=1.0, score=0.25)
    make = lambda **kw: NNetWrapper((N, N), num_channels_1=128, batch_size=32, epochs=1, max_batch=16, seed=3, **kw)
    net = make(aux_heads=on)
    fresh = net.aux_weights()
    hist = net.train(buf)
    assert hist.history["ownership_loss"][0] > 0 and len(hist.history["score_loss"]) == 1
    trained = net.aux_weights()
    assert len(trained) == 4 and any(not np.array_equal(a, b) for a, b in zip(fresh, trained))
    for name in ("aux.h5", "aux.npz"):
        path = str(tmp_path / name)
        net.save_checkpoint(path)
        other = make(aux_heads=on, weights=None)
        assert any(not np.array_equal(a, b) for a, b in zip(other.aux_weights(), trained))
        other.load_checkpoint(path)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other.get_weights(), net.get_weights()))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other.aux_weights(), trained)), name
        late = make(aux_heads=on)                                  # loaded before the trainer exists: the arrays wait for it
        late.load_checkpoint(path)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(late.aux_weights(), trained)), name
    # a file without the heads keeps the fresh ones
    plain = make(weights=net.get_weights())
    plain.save_checkpoint(str(tmp_path / "plain.h5"))
    keep = make(aux_heads=on)
    mine = keep.aux_weights()
    keep.load_checkpoint(str(tmp_path / "plain.h5"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(keep.aux_weights(), mine))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(keep.get_weights(), net.get_weights()))
    # the inference network ignores the two layers: predictions from the 44-array file and from the 40-array file are the same bits
    inf44, inf40 = make(), make()
    inf44.load_checkpoint(str(tmp_path / "aux.h5"))
    inf40.load_checkpoint(str(tmp_path / "plain.h5"))
    own = np.where(rec["player"] == 1, rec["black"], rec["white"])[:16]
    opp = np.where(rec["player"] == 1, rec["white"], rec["black"])[:16]
    (p44, v44), (p40, v40) = inf44.predict_batch(own, opp), inf40.predict_batch(own, opp)
    assert p44.tobytes() == p40.tobytes() and v44.tobytes() == v40.tobytes()
    assert len(inf44.get_weights()) == 40 and inf44.aux_weights() is None
    # a data-parallel fit is refused for a network with the heads, before and after its trainer exists: no trainer on an all-reduce's arena
    class _AllReduce:
        ptr, group = 0x1000, None
    for wrapper in (net, make(aux_heads=on)):
        with pytest.raises(ValueError, match="data-parallel"):
            wrapper.train([(np.zeros((N, N, 2), bool), np.zeros((N, N)), 1)], allreduce=_AllReduce())
    # set_aux_heads compares the checked weights, not the dicts: the same option spelled without a zero key is no change
    half = make(aux_heads=dict(ownership=1.0))
    half.aux_weights()                                             # (its trainer exists now)
    half.set_aux_heads(dict(ownership=1.0, score=0.0))
    with pytest.raises(ValueError, match="trainer exists"):
        half.set_aux_heads(dict(ownership=1.0, score=0.5))
    # with use_average the network plays the weight average, but the heads reported, copied and saved are always the trainer's raw iterate
    avg = make(aux_heads=on, optimizer=dict(average_decay=0.5, use_average=True))
    avg.train(buf)
    raw = avg._trainer.get_weights()[40:]
    assert any(not np.array_equal(a, b) for a, b in zip(raw, avg._trainer.get_weights(average=True)[40:]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(avg.aux_weights(), raw))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(avg.copy().aux_weights(), raw))


def test_training_loop_with_the_heads(oz, tmp_path):
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    net = NNetWrapper((N, N), num_channels_1=128, batch_size=32, epochs=1, max_batch=8)
    historic = loop.training(board_size=N, num_iterations=1, num_episodes=6, num_simulations=6, degree_exploration=1, temperature=1,
                             neural_network=net, e_greedy=0.9, evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0,
                             self_play_training=False, self_play_interval=1, self_play_total_games=2, self_play_threshold=1,
                             checkpoint_filepath=str(tmp_path / "loop.h5"), training_buffer_size=8 * 6 * 32, seed=12, batched_evaluation=True,
                             alias_final_boards=False, replay="device", aux_heads=dict(ownership=1.0, score=0.25))
    assert len(historic) == 1 and math.isfinite(historic[0][1])
    assert len(loop.training.aux_history) == 1
    h = loop.training.aux_history[0]
    assert set(h) == {"ownership_loss", "score_loss"} and 0 < h["ownership_loss"] < 4 and 0 < h["score_loss"] < 4
    last = loop.training.last_network
    assert last.aux_heads == dict(ownership=1.0, score=0.25) and len(last.aux_weights()) == 4
    from othellozero_amd import keras_h5
    names = [name for name, ws in keras_h5.load_keras_weights(str(tmp_path / "loop.h5")) if ws]
    assert len(names) == 16 and tuple(names[14:]) == keras_h5.AUX_LAYERS
