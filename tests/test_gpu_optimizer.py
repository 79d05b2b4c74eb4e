"""The trainer's optimiser options on the GPU (pytest -m gpu): L2 term, decoupled weight decay, decay mask, global-norm clip, weight average,
learning-rate schedule -- oz_trainer_set_optimizer and what goes with it (include/othellozero_amd.h states the per-element order of a step).

All cases run the smallest trainer (6x6, 128 filters, 7 boards, f32: the optimiser does not depend on the GEMM precision; an arena of 1.5 M
floats) with an EXTERNAL gradient arena, so that the test decides G as test_adam_three_steps does: the three arenas of three real steps, rewritten
by train_kernel_ref.adam_gradients (exact zeros, values beyond +-clipvalue, 1e-20, 1e-6), computed once and shared.

Parity: every step is judged on its own from the device's p, g, m, v, e before it and the step's own s and lr_s (step_info) against
optimizer_ref.step in float64, within optimizer_ref.MARGIN (the existing Adam margin, 4) x E32, E32 = the same code in float32;
tests/test_optimizer_cpu.py shows on the CPU that each modelled single defect lies above twice that margin at the option values used here.  The
worst ratio per (case, step, tensor) is printed (the table of one run: profiles/optimizer_parity_ratios.txt).
Exact: options off change no bit; arrays outside the decay mask are bit-identical to an off trainer's; the norm ignores the arena's padding bit
for bit; two runs are bit-identical; the resident epoch equals the step-wise loop bit for bit; the average is seeded with the weights."""
import ctypes as C

import numpy as np
import pytest

import optimizer_ref as O
import train_kernel_ref as K

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
N, CH, B = 6, 128, 7
RATE, SEED = 0.3, 77
TRAINABLE, STATS = O.TRAINABLE, O.STATS


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


class Rig:
    """one trainer on an external arena the test writes"""

    def __init__(self, weights=None, max_batch=B, **options):
        import torch
        from othellozero_amd.trainer import Trainer
        self.torch = torch
        self.arena = torch.zeros(Trainer.arena_size(N, CH, 2), dtype=torch.float32, device="cuda")
        self.tr = Trainer(N, CH, 2, max_batch=max_batch, lr=O.LR, clipvalue=O.CLIPVALUE, dropout=RATE, seed=SEED, external_grads_ptr=self.arena.data_ptr())
        self.tr.set_weights(weights if weights is not None else K.network(N, CH, 2))
        if options:
            self.tr.set_optimizer(**options)

    def load(self, k, G):
        """the forward / backward of step k (the BN statistics that apply commits), then the test's own gradients in the arena"""
        self.tr.forward_backward(*K.batch(N, B, 50 + k))
        self.tr.sync()
        self.arena.copy_(self.torch.from_numpy(np.array(G)))
        self.torch.cuda.synchronize()

    def state(self, average=False):
        """(weights[40], {i: (m, v)}, average[40] or None)"""
        return self.tr.get_weights(), {i: self.tr.adam_state(i) for i in TRAINABLE}, self.tr.get_weights(average=True) if average else None

    def run(self, grads, average=False):
        for k, G in enumerate(grads, 1):
            self.load(k, G)
            self.tr.apply()
        return self.state(average)


def _flat(state):
    w, mv, e = state
    return list(w) + [x for i in TRAINABLE for x in mv[i]] + (list(e) if e is not None else [])


def _same(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb)
    return [i for i, (x, y) in enumerate(zip(fa, fb)) if not (x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)))]


@pytest.fixture(scope="module")
def grads(oz):
    """the gradient arenas of three real consecutive steps, rewritten by adam_gradients -- computed once, never changed"""
    rig, out = Rig(), []
    for k in (1, 2, 3):
        rig.tr.forward_backward(*K.batch(N, B, 50 + k))
        rig.tr.sync()
        G = K.adam_gradients(rig.arena.cpu().numpy())
        assert np.any(G == 0) and np.any(np.abs(G) > 0.5) and np.any(np.abs(G) == F32(1e-20)) and np.any(np.abs(G) == F32(1e-6))
        G.setflags(write=False)
        out.append(G)
        rig.arena.copy_(rig.torch.from_numpy(G.copy()))
        rig.torch.cuda.synchronize()
        rig.tr.apply()
    return out


def _arrays(tr, flat):
    """the arena's array elements by get_weights() index (padding left out)"""
    out, off = {}, 0
    for i in TRAINABLE:
        n = int(np.prod(tr.shapes[i]))
        out[i] = flat[off:off + n]
        off += n + (-n % 4)
    assert off == flat.size
    return out


def _norms(tr, grads):
    return [float(np.sqrt(O.exact_sqsum(_arrays(tr, G).values())[0])) for G in grads]


# ------------------------------------------------------------------ 1. off is off
def test_options_off_change_no_bit(oz, grads):
    """three steps on a trainer never touched, one after set_optimizer(NULL) and one with every field at its off value: weights, moments and the
    step count bit for bit; the average of a trainer without one is refused"""
    never, null, off = Rig(), Rig(), Rig()
    oz.check(oz.load().oz_trainer_set_optimizer(null.tr._h, None))
    off.tr.set_optimizer(l2=0.0, weight_decay=0.0, decay_mask=None, global_clipnorm=0.0, average_decay=0.0, schedule=("constant", 0, 0, 1.0))
    a, b, c = never.run(grads), null.run(grads), off.run(grads)
    assert not _same(a, b) and not _same(a, c)
    assert never.tr.step == null.tr.step == off.tr.step == 3
    assert never.tr.step_info() == null.tr.step_info() == off.tr.step_info() == dict(lr_s=float(F32(O.LR)), grad_norm=0.0, clip_scale=1.0)
    for rig in (never, null, off):
        with pytest.raises(oz.OzError) as e:
            rig.tr.get_weights(average=True)
        assert e.value.code == oz.OZ_ERR_STATE
    assert off.tr.optimizer() == dict(l2=0.0, weight_decay=0.0, decay_mask=None, global_clipnorm=0.0, average_decay=0.0, schedule=("constant", 0, 0, 1.0))


# ------------------------------------------------------------------ 2. per-option parity
def _judge_step(rig, before, after, info, step, mask, c=0.0, lam=0.0, d=0.0, clipped=False):
    """rows dict(key, array, step, err, e32) of one step against the restatement, from the device's tensors before it"""
    (p, mv, e), (p2, mv2, e2) = before, after
    g = _arrays(rig.tr, rig.arena.cpu().numpy())
    o = O.options(info["lr_s"], step, s=info["clip_scale"] if clipped else None, c=c, lam=lam, d=d)
    rows = []
    for i in TRAINABLE:
        args = (p[i], g[i], mv[i][0], mv[i][1], e[i] if e is not None else None, o, i in mask)
        r64, r32 = O.step(*args, F64), O.step(*args, F32)
        got = (p2[i], mv2[i][0], mv2[i][1], e2[i] if e2 is not None else None)
        for j, key in enumerate("pmve"):
            if got[j] is None:
                continue
            err, e32 = O.ratio(got[j], r64[j], r32[j], floor=got[j].size < 16)
            rows.append(dict(key=key, array=i, step=step, err=err, e32=e32))
    return rows


def _report_and_assert(case, rows):
    worst = {}
    for r in rows:
        k = (r["step"], r["key"])
        if k not in worst or r["err"] / r["e32"] > worst[k]["err"] / worst[k]["e32"]:
            worst[k] = r
    for (step, key), r in sorted(worst.items()):
        print(f"optimizer-parity {case:16s} step {step} {key} worst array {r['array']:2d} err {r['err']:.3e}  E32 {r['e32']:.3e}  "
              f"ratio {r['err'] / r['e32']:6.2f}  margin {O.MARGIN[key]:4.1f}")
    assert all(r["e32"] > 0 for r in rows)
    bad = [(r["key"], r["array"], r["step"], round(r["err"] / r["e32"], 2)) for r in rows if not r["err"] <= O.MARGIN[r["key"]] * r["e32"]]
    assert not bad, f"{case}: (tensor, array, step, err / E32) above the margin: {bad}"


PARITY_CASES = {
    "l2": dict(l2=O.L2_C),
    "decoupled": dict(weight_decay=O.WEIGHT_DECAY),
    "clipnorm": dict(global_clipnorm="between"),
    "average": dict(average_decay=O.AVERAGE_DECAY),
    "cosine": dict(schedule=O.COSINE),
    "everything_l2": dict(l2=O.L2_C, global_clipnorm="between", average_decay=O.AVERAGE_DECAY, schedule=O.COSINE),
    "everything_decoupled": dict(weight_decay=O.WEIGHT_DECAY, global_clipnorm="between", average_decay=O.AVERAGE_DECAY, schedule=O.COSINE),
}


@pytest.mark.parametrize("case", list(PARITY_CASES))
def test_parity_three_steps(oz, grads, case):
    """three consecutive steps, each judged on its own; clipvalue 0.5 throughout.  The clip cases take global_clipnorm midway between the two
    smallest of the three arenas' norms, so that both branches occur: s == 1 on one step, s < 1 on the others (asserted)"""
    opt = dict(PARITY_CASES[case])
    rig = Rig()
    clipped, average = "global_clipnorm" in opt, "average_decay" in opt
    if clipped:
        norms = sorted(_norms(rig.tr, grads))
        assert norms[0] < norms[1] * (1 - 1e-6)
        opt["global_clipnorm"] = 0.5 * (norms[0] + norms[1])
    rig.tr.set_optimizer(**opt)
    sched = opt.get("schedule", ("constant", 0, 0, 1.0))
    rows, scales = [], []
    for step, G in enumerate(grads, 1):
        rig.load(step, G)
        before = rig.state(average)
        rig.tr.apply()
        after, info = rig.state(average), rig.tr.step_info()
        assert rig.tr.step == step
        want = O.schedule(O.LR, step, *sched)
        assert abs(info["lr_s"] - want) <= 4 * 2.0 ** -52 * want and info["lr_s"] == oz_lr_at(step, sched)
        if clipped:
            assert info["clip_scale"] == min(1.0, opt["global_clipnorm"] / info["grad_norm"])
            scales.append(info["clip_scale"])
        else:
            assert info["grad_norm"] == 0.0 and info["clip_scale"] == 1.0
        rows += _judge_step(rig, before, after, info, step, O.DEFAULT_MASK, c=opt.get("l2", 0.0), lam=opt.get("weight_decay", 0.0),
                            d=opt.get("average_decay", 0.0), clipped=clipped)
        for i in STATS:                           # the average of a moving statistic is the statistic
            assert after[2] is None or np.array_equal(after[2][i], after[0][i])
    if clipped:
        assert any(s == 1.0 for s in scales) and any(s < 1.0 for s in scales), scales
    _report_and_assert(case, rows)


def oz_lr_at(step, sched):
    from othellozero_amd import trainer
    return trainer.lr_schedule_at(O.LR, step, schedule=sched)


# ------------------------------------------------------------------ 3. the mask, exactly
def test_mask_exact(oz, grads):
    """the same G into an off trainer and decoupled-decay trainers: arrays outside the mask bit for bit (weights and moments), every array inside
    differs (weights; the decoupled decay leaves the moments alone).  Default mask; indices 6 and 36 only; and 37 (36 elements) with 39 (one element,
    padded to four), which must take correct steps"""
    off = Rig()
    base = off.run(grads[:1])
    for mask in (None, [6, 36], [37, 39]):
        rig = Rig(weight_decay=O.WEIGHT_DECAY, decay_mask=mask)
        rig.load(1, grads[0])
        before = rig.state()
        rig.tr.apply()
        got, info = rig.state(), rig.tr.step_info()
        inside = O.DEFAULT_MASK if mask is None else mask
        assert rig.tr.optimizer()["decay_mask"] == (None if mask is None else sum(1 << i for i in mask))
        for i in range(40):
            same_w = np.array_equal(got[0][i].view(np.uint32), base[0][i].view(np.uint32))
            assert same_w != (i in inside), (mask, i)
            if i in TRAINABLE:
                assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got[1][i], base[1][i])), (mask, i)
        rows = [r for r in _judge_step(rig, before, got, info, 1, inside, lam=O.WEIGHT_DECAY) if r["array"] in inside or r["array"] in (37, 39)]
        _report_and_assert(f"mask {mask}", rows)


# ------------------------------------------------------------------ 4. the norm
def test_norm_and_sqsum(oz, grads):
    """grad_norm against math.fsum of the exact float64 squares of the arena's array elements, relative bound (N + 2) 2^-53 (any summation order
    of non-negative terms, plus the root); 1000.0 in the arena's padding changes no bit of it; sqsum likewise, over the masked arrays"""
    G = grads[1]
    rig = Rig(global_clipnorm=1e-3)
    rig.load(1, G)
    w0 = rig.tr.get_weights()
    exact, count = O.exact_sqsum(_arrays(rig.tr, G).values())
    got = rig.tr.sqsum("gradients")
    assert abs(got - exact) <= O.norm_bound(count) * exact
    rig.tr.apply()
    info = rig.tr.step_info()
    assert abs(info["grad_norm"] - np.sqrt(exact)) <= O.norm_bound(count) * np.sqrt(exact)
    assert info["clip_scale"] == 1e-3 / info["grad_norm"] < 1.0
    assert rig.tr.sqsum("gradients") == got                        # apply reads the arena, it does not write it
    # the padding
    pad = O.padding_mask({i: int(np.prod(rig.tr.shapes[i])) for i in TRAINABLE})
    assert pad.size == G.size and pad.sum() == 3                   # the value bias, one element in a unit of four
    G2 = G.copy()
    G2[pad] = 1000.0
    other = Rig(global_clipnorm=1e-3)
    other.load(1, G2)
    assert other.tr.sqsum("gradients") == got
    other.tr.apply()
    assert other.tr.step_info() == info
    assert not _same(rig.state(), other.state())
    # the decayed weights: default mask, then 6 and 36 only
    for mask, tr in ((O.DEFAULT_MASK, rig.tr), ([6, 36], other.tr)):
        if mask != O.DEFAULT_MASK:
            tr.set_optimizer(weight_decay=1e-2, decay_mask=mask)
        w = tr.get_weights()
        exact_w, count_w = O.exact_sqsum([w[i] for i in mask])
        assert abs(tr.sqsum("weights") - exact_w) <= O.norm_bound(count_w) * exact_w, mask
    plain = Rig()                                                  # a trainer without options answers too (default mask)
    exact_w, count_w = O.exact_sqsum([w0[i] for i in O.DEFAULT_MASK])
    assert abs(plain.tr.sqsum("weights") - exact_w) <= O.norm_bound(count_w) * exact_w


# ------------------------------------------------------------------ 5. determinism
def test_two_runs_are_bit_identical(oz, grads):
    norms = sorted(_norms(Rig().tr, grads))
    opt = dict(weight_decay=O.WEIGHT_DECAY, decay_mask=[0, 6, 30, 36, 37, 39], global_clipnorm=0.5 * (norms[0] + norms[1]), average_decay=O.AVERAGE_DECAY,
               schedule=O.COSINE)
    out = []
    for _ in range(2):
        rig, infos = Rig(**opt), []
        for k, G in enumerate(grads, 1):
            rig.load(k, G)
            rig.tr.apply()
            infos.append(rig.tr.step_info())
        out.append((rig.state(average=True), infos))
    assert not _same(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] and all(i["grad_norm"] > 0 for i in out[0][1])


# ------------------------------------------------------------------ 6. the resident epoch = the step-wise loop
def test_resident_epoch_equals_stepwise_loop(oz):
    """one fit_epoch of 5 batches (37 examples at batch 8: a short last batch) with schedule + decay + average + clip against forward_backward /
    apply over the same order, bit for bit; then set_lr between two applies changes the next step and only that"""
    from othellozero_amd import trainer as T
    sched = ("linear", 2, 10, 0.25)
    opt = dict(weight_decay=O.WEIGHT_DECAY, global_clipnorm=0.05, average_decay=O.AVERAGE_DECAY, schedule=sched)
    own, opp, pi, z = K.batch(N, 37, 9, dense_rows="all")
    order = np.random.RandomState(4).permutation(37)
    res, loop = Rig(max_batch=8, **opt), Rig(max_batch=8, **opt)
    res.tr.set_dataset(own, opp, pi, z)
    res.tr.fit_epoch(order, 8)
    for s in range(0, 37, 8):
        idx = order[s:s + 8]
        loop.tr.forward_backward(own[idx], opp[idx], pi[idx], z[idx])
        loop.tr.apply()
    assert res.tr.step == loop.tr.step == 5
    assert not _same(res.state(average=True), loop.state(average=True))
    info = res.tr.step_info()
    assert info == loop.tr.step_info() and info["lr_s"] == T.lr_schedule_at(O.LR, 5, schedule=sched) and 0 < info["clip_scale"] < 1
    # set_lr
    idx = order[:8]
    loop.tr.forward_backward(own[idx], opp[idx], pi[idx], z[idx])
    before = loop.state(average=True)
    loop.tr.set_lr(2e-3)
    assert not _same(before, loop.state(average=True)) and loop.tr.step_info() == info          # nothing moves before the next apply
    loop.tr.apply()
    after, info6 = loop.state(average=True), loop.tr.step_info()
    assert info6["lr_s"] == T.lr_schedule_at(2e-3, 6, schedule=sched) > 1.9 * T.lr_schedule_at(O.LR, 6, schedule=sched)
    rows = _judge_step(loop, before, after, info6, 6, O.DEFAULT_MASK, lam=O.WEIGHT_DECAY, d=O.AVERAGE_DECAY, clipped=True)
    _report_and_assert("after set_lr", rows)
    loop.tr.forward_backward(own[idx], opp[idx], pi[idx], z[idx])
    loop.tr.apply()
    assert loop.tr.step_info()["lr_s"] == T.lr_schedule_at(2e-3, 7, schedule=sched)           # the new rate stays


# ------------------------------------------------------------------ 7. seeding
def test_average_is_seeded_with_the_weights(oz, grads):
    rig = Rig()
    rig.run(grads[:1])
    rig.tr.set_optimizer(average_decay=O.AVERAGE_DECAY)
    w, e = rig.tr.get_weights(), rig.tr.get_weights(average=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(w, e))           # E == P exactly when switched on
    rig.load(2, grads[1])
    rig.tr.apply()
    w, e = rig.tr.get_weights(), rig.tr.get_weights(average=True)
    # (the one-element value bias has an exact-zero gradient in both arenas: it does not move, and its average equals it)
    assert all(not np.array_equal(w[i], e[i]) for i in TRAINABLE if w[i].size > 1) and all(np.array_equal(w[i], e[i]) for i in STATS)
    fresh = K.network(N, CH, 2)
    rig.tr.set_weights(fresh)
    w, e = rig.tr.get_weights(), rig.tr.get_weights(average=True)
    assert all(np.array_equal(a, b) and np.array_equal(a, np.asarray(f, F32)) for a, b, f in zip(w, e, fresh))
    # changing another option while the average is on keeps it; switching it off and on seeds it again
    rig.load(3, grads[2])
    rig.tr.apply()
    e1 = rig.tr.get_weights(average=True)
    rig.tr.set_optimizer(average_decay=0.5, weight_decay=1e-2)
    assert all(np.array_equal(a, b) for a, b in zip(e1, rig.tr.get_weights(average=True)))
    rig.tr.set_optimizer()
    rig.tr.set_optimizer(average_decay=0.5)
    assert all(np.array_equal(a, b) for a, b in zip(rig.tr.get_weights(), rig.tr.get_weights(average=True)))


# ------------------------------------------------------------------ 8. the wrapper
def _examples(count, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        cells = rs.randint(0, 3, size=(N, N))
        board = np.stack([cells == 1, cells == 2], axis=2).astype(np.float32)
        out.append((board, rs.dirichlet(np.ones(N * N)).astype(F32).reshape(N, N), float(rs.choice([-1.0, 1.0]))))
    return out


def test_wrapper_trains_on_the_raw_iterate_and_plays_on_the_average(oz):
    from othellozero_amd import trainer as T
    from othellozero_amd.NNet import NNetWrapper
    settings = dict(average_decay=0.9, use_average=True, weight_decay=1e-2)
    net = NNetWrapper((N, N), num_channels_1=CH, batch_size=16, epochs=1, optimizer=settings)
    w0 = net.get_weights()
    examples = _examples(64, 1)
    bits = lambda ws: [np.asarray(a, F32).view(np.uint32) for a in ws]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))
    hist = net.train(examples)
    assert hist.lr == [float(F32(net.lr))] and hist.grad_norm == [None] and list(hist.history) == ["loss", "pi-reshaped_loss", "v_loss"]
    raw, avg = net._trainer.get_weights(), net._trainer.get_weights(average=True)
    assert same(net.get_weights(), avg)
    assert all(not np.array_equal(raw[i], avg[i]) for i in TRAINABLE)
    net.train(examples)
    assert same(net.get_weights(), net._trainer.get_weights(average=True))
    # a bare trainer that runs the two fits without re-seeding
    bare = T.Trainer(N, CH, 2, max_batch=16, lr=net.lr, clipvalue=0.5, dropout=net.dropout, seed=net._model_index,
                     optimizer=dict(average_decay=0.9, weight_decay=1e-2))
    bare.set_weights(w0)
    data = T.pack_examples(examples, N, 2)
    for call in (0, 1):
        T.fit(bare, *data, batch_size=16, epochs=1, shuffle_seed=1000003 * call + net._model_index)
    assert bare.step == net._trainer.step == 8
    assert same(bare.get_weights(), net._trainer.get_weights()) and same(bare.get_weights(average=True), net._trainer.get_weights(average=True))
    # somebody else sets the network's weights: the trainer starts from them (moments and step stay, as ever)
    net.set_weights(w0)
    net.train(examples)
    bare.set_weights(w0)
    T.fit(bare, *data, batch_size=16, epochs=1, shuffle_seed=1000003 * 2 + net._model_index)
    assert same(bare.get_weights(), net._trainer.get_weights()) and same(bare.get_weights(average=True), net.get_weights())
    # copy() carries the settings, not the state
    twin = net.copy()
    assert twin.optimizer == settings and twin.optimizer is not net.optimizer and getattr(twin, "_trainer", None) is None
    assert same(twin.get_weights(), net.get_weights())
    twin.epochs = 1                                  # (copy() has never carried batch_size / epochs: one batch of 16, one epoch)
    twin.train(examples[:16])
    assert twin._trainer.step == 1 and twin._trainer.optimizer()["average_decay"] == 0.9 and twin._trainer.optimizer()["weight_decay"] == 1e-2


# ------------------------------------------------------------------ 9. refusals on the device
def test_refusals_on_the_device(oz):
    rig = Rig()
    lib, tr = oz.load(), rig.tr
    buf = np.zeros(9 * 2 * CH, F32)
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    assert lib.oz_trainer_get_step_info(tr._h, C.byref(a), C.byref(b), C.byref(c)) == oz.OZ_ERR_STATE           # no step applied yet
    for index in (4, 5, 34, 35):
        with pytest.raises(oz.OzError) as e:
            tr.set_optimizer(weight_decay=1e-2, decay_mask=[index])
        assert e.value.code == oz.OZ_ERR_ARG, index
    with pytest.raises(oz.OzError) as e:
        tr.set_optimizer(l2=1e-4, weight_decay=1e-2)
    assert e.value.code == oz.OZ_ERR_ARG
    assert tr.optimizer()["weight_decay"] == 0.0 and tr.optimizer()["l2"] == 0.0                                 # a refused call changes nothing
    assert lib.oz_trainer_get_weight_average(tr._h, 0, oz.p_f32(buf), buf.size) == oz.OZ_ERR_STATE               # the average is off
    tr.set_optimizer(average_decay=0.5)
    assert lib.oz_trainer_get_weight_average(tr._h, 0, oz.p_f32(buf), buf.size) == oz.OZ_OK
    for index, nelem in ((0, buf.size - 1), (0, buf.size + 1), (1, buf.size), (39, 4), (4, CH + 1), (40, 1), (-1, 1)):
        assert lib.oz_trainer_get_weight_average(tr._h, index, oz.p_f32(buf), nelem) == oz.OZ_ERR_ARG, (index, nelem)
    assert lib.oz_trainer_get_weight_average(tr._h, 0, None, buf.size) == oz.OZ_ERR_ARG
    assert lib.oz_trainer_sqsum(tr._h, 2, C.byref(a)) == oz.OZ_ERR_ARG and lib.oz_trainer_sqsum(tr._h, 0, None) == oz.OZ_ERR_ARG
    assert lib.oz_trainer_set_lr(tr._h, -1.0) == oz.OZ_ERR_ARG
    assert lib.oz_trainer_set_optimizer(None, None) == oz.OZ_ERR_ARG and lib.oz_trainer_get_optimizer(tr._h, None) == oz.OZ_ERR_ARG
