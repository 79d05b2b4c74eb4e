"""Training step on the GPU -- host mirror of NNetWrapper.train (Net/NNet.py:53-68); C ABI: oz_trainer_*.

`Trainer` is the step-level object (forward + backward into a gradient arena, Adam apply); `fit(...)` is the epoch loop
of keras Model.fit as the reference drives it (shuffle every epoch, batches of `batch_size`, last batch may be short,
per-epoch mean losses in a History-like object).  Data-parallel training: every rank runs `fit` on its shard of the
examples with the same seed and weights, gradients are averaged with one all-reduce per step (distributed.py).
"""
import ctypes as C

import numpy as np

from . import _lib
from .weights import onn_shapes

TRAINABLE = [i for i in range(40) if i >= 36 or i % 6 not in (4, 5)]
AUX_ARRAYS = (40, 41, 42, 43)          # get_weights() indices of the auxiliary heads: Wown (512, n*n), bown (n*n,), Wsc (512, 1), bsc (1,)
AUX_KEYS = ("ownership_loss", "score_loss")      # History.history gains these two with the auxiliary heads on
PRECISION_MODES = {"f32": 0, "f16x2": 1, "bf16x3": 2}      # oz_trainer_set_precision
POLICY_LOSSES = {"rows": _lib.POLICY_LOSS_ROWS, "flat": _lib.POLICY_LOSS_FLAT}      # oz_trainer_set_policy_loss


class History:
    """what keras Model.fit returns, as far as the reference uses it (main.py:108: kept, never read).  `lr` / `grad_norm`: the scheduled rate and the
    gradient's global norm (None with global_clipnorm off) of each epoch's LAST step -- attributes, Keras' history holds the three losses only"""

    def __init__(self, aux=False):
        self.history = {"loss": [], "pi-reshaped_loss": [], "v_loss": []}
        if aux:
            self.history.update({k: [] for k in AUX_KEYS})
        self.epoch = []
        self.lr, self.grad_norm = [], []


OPTIMIZER_KEYS = ("l2", "weight_decay", "decay_mask", "global_clipnorm", "average_decay", "schedule")


def make_optimizer(l2=0.0, weight_decay=0.0, decay_mask=None, global_clipnorm=0.0, average_decay=0.0, schedule=None):
    """the options as an oz_optimizer (_lib.Optimizer).  decay_mask: None = the default (the eight kernels), an int bit mask or an iterable of
    get_weights() indices; schedule: None or (kind, warmup_steps, total_steps, final_ratio), kind "constant" / "linear" / "cosine".  Values are
    passed on as given: the library validates them (OzError OZ_ERR_ARG)."""
    o = _lib.Optimizer()
    o.l2, o.weight_decay, o.global_clipnorm, o.average_decay = float(l2), float(weight_decay), float(global_clipnorm), float(average_decay)
    if decay_mask is None:
        o.decay_mask = 0
    elif isinstance(decay_mask, (int, np.integer)):
        o.decay_mask = int(decay_mask)
    else:
        idx = [int(i) for i in decay_mask]
        assert idx and all(0 <= i < 64 for i in idx), "decay_mask: a non-empty list of get_weights() indices (None: the default)"
        o.decay_mask = sum(1 << i for i in set(idx))
    kind, warmup, total, ratio = schedule if schedule is not None else ("constant", 0, 0, 1.0)
    assert kind in _lib.LR_SCHEDULES, kind
    o.schedule, o.warmup_steps, o.total_steps, o.final_ratio = _lib.LR_SCHEDULES[kind], int(warmup), int(total), float(ratio)
    return o


def aux_shapes(board_size):
    """shapes of the four arrays of the auxiliary heads, get_weights() indices 40 .. 43"""
    A = board_size * board_size
    return [(512, A), (A,), (512, 1), (1,)]


def lr_schedule_at(lr, step, schedule=None, **options):
    """lr_s of optimiser step `step` (1-based) under `schedule` (oz_lr_schedule_at: the library's one definition; no GPU needed)"""
    out = C.c_double()
    _lib.check(_lib.load().oz_lr_schedule_at(C.byref(make_optimizer(schedule=schedule, **options)), float(lr), int(step), C.byref(out)))
    return out.value


class Trainer:
    def __init__(self, board_size=8, channels=512, in_channels=2, max_batch=32, lr=1e-3, clipvalue=0.5, dropout=0.3,
                 bn_momentum=0.99, seed=0, external_grads_ptr=None, precision="f32", policy_loss="rows", optimizer=None, aux_heads=None):
        """optimizer: None or a dict of set_optimizer's keyword arguments
        aux_heads: None or dict(ownership=w, score=w) -- an ownership and a score head trained on the games' final boards beside the policy and
        value heads (oz_trainer_set_aux_heads): four more arrays behind the forty, two more losses; fed through forward_backward / set_dataset's
        fin_own / fin_opp or a ReplayBuffer(aux=True)
        precision: arithmetic of the 3x3 layers -- "f32" (fp32 matrix cores), "f16x2" (forward / data-gradient GEMMs: fp32 values
        as two fp16 planes on the fp16 matrix cores, per-step power-of-two scaling and a range guard; channels % 256 == 0) or "bf16x3"
        (forward, data gradient and weight gradient: every fp32 value exactly as three bf16 planes on the bf16 matrix cores, no scaling,
        no guard; channels % 256 == 0)
        policy_loss: "rows" -- the reference's categorical cross entropy on the (n, n)-reshaped softmax (each board row renormalised, rows
        averaged); "flat" -- on the whole (n*n,) softmax, the loss for dense visit-distribution targets"""
        assert precision in PRECISION_MODES, precision
        assert policy_loss in POLICY_LOSSES, policy_loss
        aux = _lib.check_aux_heads(aux_heads)
        if aux is not None and external_grads_ptr:
            raise ValueError("aux_heads is not offered with external_grads_ptr (a data-parallel fit): the external gradient arena is sized for the "
                             "forty arrays -- the heads' four gradients would be written past its end -- and the pooled rows carry no final pairs")
        lib = _lib.require_gpu()
        self.n, self.channels, self.in_channels, self.max_batch = board_size, channels, in_channels, int(max_batch)
        self._h = C.c_void_p()
        _lib.check(lib.oz_trainer_create(C.byref(self._h), board_size, channels, in_channels, self.max_batch, lr,
                                         clipvalue if clipvalue else 0.0, dropout, bn_momentum, seed,
                                         C.c_void_p(external_grads_ptr) if external_grads_ptr else None))
        self.shapes = onn_shapes(board_size, channels, in_channels)
        self.precision = precision
        if precision != "f32":
            _lib.check(lib.oz_trainer_set_precision(self._h, PRECISION_MODES[precision]))
        self.policy_loss = policy_loss
        if policy_loss != "rows":
            _lib.check(lib.oz_trainer_set_policy_loss(self._h, POLICY_LOSSES[policy_loss]))
        self.aux = aux is not None
        if self.aux:
            _lib.check(lib.oz_trainer_set_aux_heads(self._h, aux[0], aux[1]))
            self.shapes = list(self.shapes) + aux_shapes(board_size)
        if optimizer:
            self.set_optimizer(**optimizer)

    def __del__(self):
        try:
            if self._h:
                _lib.load().oz_trainer_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @staticmethod
    def arena_size(board_size, channels, in_channels=2, aux=False):
        """floats of the parameter / gradient / Adam arenas (aux: of a trainer with the auxiliary heads)"""
        n, lib = C.c_int64(), _lib.load()
        _lib.check((lib.oz_trainer_arena_size_aux if aux else lib.oz_trainer_arena_size)(board_size, channels, in_channels, C.byref(n)))
        return n.value

    def set_weights(self, weights):
        """the 40 arrays (the auxiliary heads, if any, keep theirs) or, with the auxiliary heads, all 44"""
        lib = _lib.load()
        assert len(weights) in (40, len(self.shapes)), len(weights)
        for i, (w, shp) in enumerate(zip(weights, self.shapes)):
            a = np.ascontiguousarray(w, dtype=np.float32)
            assert a.shape == tuple(shp), f"weight {i}: shape {a.shape} != {shp}"
            _lib.check(lib.oz_trainer_set_weight(self._h, i, _lib.p_f32(a), a.size))

    def get_weights(self, average=False):
        """the 40 arrays (44 with the auxiliary heads); average=True: the weight average E in place of every trainable array (the BN moving
        statistics as they are); OzError(OZ_ERR_STATE) with average_decay off"""
        lib, out = _lib.load(), []
        get = lib.oz_trainer_get_weight_average if average else lib.oz_trainer_get_weight
        for i, shp in enumerate(self.shapes):
            a = np.zeros(shp, dtype=np.float32)
            _lib.check(get(self._h, i, _lib.p_f32(a), a.size))
            out.append(a)
        return out

    # ---- optimiser options (oz_trainer_set_optimizer: they act inside apply, so the resident and the step-wise paths see the same steps)
    def set_optimizer(self, l2=0.0, weight_decay=0.0, decay_mask=None, global_clipnorm=0.0, average_decay=0.0, schedule=None):
        """l2: c of Keras' kernel_regularizer=l2(c), 2 c w joins the gradient before clipvalue; weight_decay: decoupled (AdamW), w -= lr_s lambda w;
        decay_mask: the arrays both act on (None: the eight kernels); global_clipnorm: the gradient is scaled by min(1, clipnorm / its global norm);
        average_decay: d of the weight average E = d E + (1 - d) w, read with get_weights(average=True); schedule: (kind, warmup_steps,
        total_steps, final_ratio).  No argument: everything off.  The per-element order of a step is defined in othellozero_amd.h."""
        o = make_optimizer(l2, weight_decay, decay_mask, global_clipnorm, average_decay, schedule)
        _lib.check(_lib.load().oz_trainer_set_optimizer(self._h, C.byref(o)))

    def optimizer(self):
        """the options in force, as set_optimizer's keyword arguments"""
        o = _lib.Optimizer()
        _lib.check(_lib.load().oz_trainer_get_optimizer(self._h, C.byref(o)))
        kind = {v: k for k, v in _lib.LR_SCHEDULES.items()}[o.schedule]
        return dict(l2=o.l2, weight_decay=o.weight_decay, decay_mask=int(o.decay_mask) or None, global_clipnorm=o.global_clipnorm,
                    average_decay=o.average_decay, schedule=(kind, int(o.warmup_steps), int(o.total_steps), o.final_ratio))

    def set_lr(self, lr):
        """the base learning rate from the next apply on"""
        _lib.check(_lib.load().oz_trainer_set_lr(self._h, float(lr)))

    def step_info(self):
        """dict(lr_s, grad_norm, clip_scale) of the last applied step (the two norm fields are 0 and 1 with global_clipnorm off)"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _lib.check(_lib.load().oz_trainer_get_step_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(lr_s=a.value, grad_norm=b.value, clip_scale=c.value)

    def time_optimizer(self, iters=20):
        """benchmark hook: dict(kernel_ms, reduction_ms), mean HIP-event time of `iters` launches of the step's optimiser kernel and of the norm's
        two kernels (0 with global_clipnorm off).  The launches are real: for a scratch trainer"""
        ms = np.zeros(3, np.float64)
        _lib.check(_lib.load().oz_trainer_time_optimizer(self._h, int(iters), _lib.p_f64(ms)))
        return dict(kernel_ms=float(ms[0]), reduction_ms=float(ms[1]))

    def sqsum(self, what):
        """the sum of squares of the gradient arena ("gradients") or of the decayed arrays' weights ("weights": c times this is the L2 term), float64"""
        out = C.c_double()
        _lib.check(_lib.load().oz_trainer_sqsum(self._h, _lib.SQSUM_KINDS[what], C.byref(out)))
        return out.value

    def get_grads(self):
        """{index: gradient} of the trainable arrays after forward_backward"""
        lib, out = _lib.load(), {}
        for i in TRAINABLE + (list(AUX_ARRAYS) if self.aux else []):
            a = np.zeros(self.shapes[i], dtype=np.float32)
            _lib.check(lib.oz_trainer_get_grad(self._h, i, _lib.p_f32(a), a.size))
            out[i] = a
        return out

    def get_grad(self, index):
        """the gradient of trainable array `index` after forward_backward"""
        a = np.zeros(self.shapes[index], dtype=np.float32)
        _lib.check(_lib.load().oz_trainer_get_grad(self._h, index, _lib.p_f32(a), a.size))
        return a

    def grad_arena(self):
        ptr, n = C.c_void_p(), C.c_int64()
        _lib.check(_lib.load().oz_trainer_grad_arena(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def _fin(self, fin_own, fin_opp, count):
        """the examples' final pairs as two uint64 arrays, or None without them"""
        if fin_own is None and fin_opp is None:
            return None
        assert self.aux, "fin_own / fin_opp feed the auxiliary heads: Trainer(..., aux_heads=dict(ownership=w, score=w))"
        fo = np.ascontiguousarray(fin_own, dtype=np.uint64).ravel()
        fp = np.ascontiguousarray(fin_opp, dtype=np.uint64).ravel()
        assert fo.size == count and fp.size == count, (fo.size, fp.size, count)
        return fo, fp

    def forward_backward(self, own, opp, pi_target, z_target, fin_own=None, fin_opp=None):
        """-> (loss, pi loss, v loss) of the batch; gradients of the batch-mean loss are left in the arena.  With the auxiliary heads:
        -> (loss, pi loss, v loss, ownership loss, score loss); fin_own / fin_opp: the examples' final pairs (rules_aux_targets; without them
        every mask is 0)"""
        own = np.ascontiguousarray(own, dtype=np.uint64).ravel()
        opp = np.ascontiguousarray(opp, dtype=np.uint64).ravel()
        B = own.size
        pit = np.ascontiguousarray(pi_target, dtype=np.float32).reshape(B, self.n * self.n)
        zt = np.ascontiguousarray(z_target, dtype=np.float32).reshape(B)
        fin = self._fin(fin_own, fin_opp, B)
        losses = np.zeros(5, np.float32)
        if fin is not None:
            _lib.check(_lib.load().oz_trainer_forward_backward_aux(self._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pit), _lib.p_f32(zt),
                                                                   _lib.p_u64(fin[0]), _lib.p_u64(fin[1]), B, _lib.p_f32(losses)))
        else:
            _lib.check(_lib.load().oz_trainer_forward_backward(self._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pit),
                                                               _lib.p_f32(zt), B, _lib.p_f32(losses)))
            if self.aux:
                losses[3:] = self.aux_losses()
        return tuple(float(x) for x in losses[:5 if self.aux else 3])

    def set_dataset(self, own, opp, pi, z, fin_own=None, fin_opp=None):
        """upload the examples of a fit once; they stay in HBM until the next set_dataset.  fin_own / fin_opp: their final pairs for the
        auxiliary heads (without them every mask is 0)"""
        own = np.ascontiguousarray(own, dtype=np.uint64); opp = np.ascontiguousarray(opp, dtype=np.uint64)
        pi = np.ascontiguousarray(pi, dtype=np.float32).reshape(own.size, self.n * self.n)
        z = np.ascontiguousarray(z, dtype=np.float32)
        fin = self._fin(fin_own, fin_opp, own.size)
        if fin is not None:
            _lib.check(_lib.load().oz_trainer_set_dataset_aux(self._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z),
                                                              _lib.p_u64(fin[0]), _lib.p_u64(fin[1]), own.size))
            return
        _lib.check(_lib.load().oz_trainer_set_dataset(self._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z), own.size))

    # ---- auxiliary heads: read-outs of the last step / epoch
    def aux_outputs(self, B):
        """(ownership (B, n*n) in [-1, 1] for the mover, score (B,)) of the last forward pass"""
        o, s = np.zeros((B, self.n * self.n), np.float32), np.zeros(B, np.float32)
        _lib.check(_lib.load().oz_trainer_aux_outputs(self._h, B, _lib.p_f32(o), _lib.p_f32(s)))
        return o, s

    def aux_losses(self, epoch=False):
        """(ownership loss, score loss): the last step's batch means (float32), or with epoch=True the float64 sample-weighted means of the last
        fit_epoch / fit_epoch_replay call"""
        if epoch:
            out = np.zeros(2, np.float64)
            _lib.check(_lib.load().oz_trainer_get_aux_losses(self._h, None, _lib.p_f64(out)))
        else:
            out = np.zeros(2, np.float32)
            _lib.check(_lib.load().oz_trainer_get_aux_losses(self._h, _lib.p_f32(out), None))
        return out

    def aux_head_grads(self, B, before=False):
        """(dopre (B, n*n), dspre (B,)) of the last step: the gradients wrt the two heads' pre-activations, loss weights included; before=True
        adds the gradient wrt f2 (B, 512) as the policy and value heads left it, before the auxiliary term (needs set_capture(True))"""
        do, ds = np.zeros((B, self.n * self.n), np.float32), np.zeros(B, np.float32)
        d0 = np.zeros((B, 512), np.float32) if before else None
        _lib.check(_lib.load().oz_trainer_get_aux_head_grads(self._h, B, _lib.p_f32(do), _lib.p_f32(ds), _lib.p_f32(d0) if before else None))
        return (do, ds, d0) if before else (do, ds)

    def fit_epoch(self, order, batch_size):
        """the optimiser steps of one epoch over the resident examples in `order` (batches of batch_size, last one short);
        -> sample-weighted mean (loss, policy loss, value loss)"""
        order = np.ascontiguousarray(order, dtype=np.int32)
        out = np.zeros(3, np.float32)
        _lib.check(_lib.load().oz_trainer_fit_epoch(self._h, _lib.p_i32(order), order.size, int(batch_size), _lib.p_f32(out)))
        return out

    def fit_epoch_replay(self, replay, order, batch_size):
        """fit_epoch with a ReplayBuffer's slots as the resident examples: order = slot indices in [0, len(replay))"""
        order = np.ascontiguousarray(order, dtype=np.int32)
        out = np.zeros(3, np.float32)
        _lib.check(_lib.load().oz_trainer_fit_epoch_replay(self._h, replay._h, _lib.p_i32(order), order.size, int(batch_size), _lib.p_f32(out)))
        return out

    # ---- held-out evaluation in inference mode (oz_trainer_evaluate*): moving BN statistics, no dropout, the trainer's raw iterate; no state of
    # a fit is touched (outputs() / activation() afterwards show the evaluation's last batch)
    @staticmethod
    def _eval_dict(out):
        return {"loss": float(out[0]), "pi-reshaped_loss": float(out[1]), "v_loss": float(out[2]), "policy_top1": float(out[3]),
                "value_sign": float(out[4]), "examples": int(out[5]), "decided": int(out[6])}

    def evaluate(self, own, opp, pi, z, batch_size=None):
        """keras Model.evaluate on host examples (the resident data set of a fit stays): dict(loss, pi-reshaped_loss, v_loss -- the fit's loss
        definitions --, policy_top1 = share of examples whose policy arg-max is the target's (lowest index on ties), value_sign = share of the
        `decided` examples (z != 0) whose v has z's sign, examples, decided).  batch_size None: max_batch"""
        own = np.ascontiguousarray(own, dtype=np.uint64).ravel()
        opp = np.ascontiguousarray(opp, dtype=np.uint64).ravel()
        pi = np.ascontiguousarray(pi, dtype=np.float32).reshape(own.size, self.n * self.n)
        z = np.ascontiguousarray(z, dtype=np.float32).reshape(own.size)
        out = np.zeros(_lib.EVAL_FIELDS, np.float64)
        _lib.check(_lib.load().oz_trainer_evaluate(self._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z), own.size,
                                                   int(self.max_batch if batch_size is None else batch_size), _lib.p_f64(out)))
        return self._eval_dict(out)

    def evaluate_dataset(self, order, batch_size):
        """evaluate() on the examples `order` indexes in the resident data set (set_dataset)"""
        order = np.ascontiguousarray(order, dtype=np.int32)
        out = np.zeros(_lib.EVAL_FIELDS, np.float64)
        _lib.check(_lib.load().oz_trainer_evaluate_dataset(self._h, _lib.p_i32(order), order.size, int(batch_size), _lib.p_f64(out)))
        return self._eval_dict(out)

    def evaluate_replay(self, replay, order, batch_size):
        """evaluate() on a ReplayBuffer's slots `order` (indices in [0, len(replay))), read in place on the device"""
        order = np.ascontiguousarray(order, dtype=np.int32)
        out = np.zeros(_lib.EVAL_FIELDS, np.float64)
        _lib.check(_lib.load().oz_trainer_evaluate_replay(self._h, replay._h, _lib.p_i32(order), order.size, int(batch_size), _lib.p_f64(out)))
        return self._eval_dict(out)

    def apply(self):
        _lib.check(_lib.load().oz_trainer_apply(self._h))

    def sync(self):
        _lib.check(_lib.load().oz_trainer_sync(self._h))

    def outputs(self, B):
        p, v = np.zeros((B, self.n * self.n), np.float32), np.zeros(B, np.float32)
        _lib.check(_lib.load().oz_trainer_outputs(self._h, B, _lib.p_f32(p), _lib.p_f32(v)))
        return p, v

    def activation(self, layer, B):
        """post-activation output of block `layer` (0-3 conv: (B, H, H, C); 4-5 dense: (B, units)) of the last forward pass"""
        n, C_ = self.n, self.channels
        shape = [(B, n, n, C_), (B, n, n, C_), (B, n - 2, n - 2, C_), (B, n - 4, n - 4, C_), (B, 1024), (B, 512)][layer]
        a = np.zeros(shape, np.float32)
        _lib.check(_lib.load().oz_trainer_get_activation(self._h, layer, B, _lib.p_f32(a), a.size))
        return a

    # ---- read-only views of the last step (diagnostics: the per-kernel parity tests)
    def _layer_shape(self, layer, border=False):
        n, C_ = self.n, self.channels
        side = [n, n, n - 2, n - 4][layer] + (4 if border and layer in (2, 3) else 0) if layer < 4 else 1
        return (side, side, C_) if layer < 4 else (1, 1, (1024, 512)[layer - 4])

    def _view(self, fn, layer, B, border=False):
        a = np.zeros((B,) + self._layer_shape(layer, border), np.float32)
        _lib.check(fn(self._h, layer, B, _lib.p_f32(a), a.size))
        return a

    def preact(self, layer, B):
        """z[layer] of the last forward pass: the GEMM output plus bias BEFORE the BN, (B, Hout, Hout, Co); layer 0 .. 5 (dense: Hout = 1)"""
        return self._view(_lib.load().oz_trainer_get_preact, layer, B)

    def dz(self, layer, B):
        """the whole buffer of the gradient wrt z[layer] of the last step, (B, Hz, Hz, Co): conv3 / conv4 keep it zero-bordered (Hz = Hout + 4)"""
        return self._view(_lib.load().oz_trainer_get_dz, layer, B, border=True)

    def set_capture(self, on):
        """while on, a step keeps a copy of every raw data gradient (dgrad); off by default, and then the launch sequence is unchanged"""
        _lib.check(_lib.load().oz_trainer_set_capture(self._h, 1 if on else 0))

    def dgrad(self, layer, B):
        """the captured gradient wrt a[layer] (the raw output of the data-gradient GEMM of layer + 1, of the heads for layer 5), (B, Hout, Hout, Co)"""
        return self._view(_lib.load().oz_trainer_get_dgrad, layer, B)

    def head_grads(self, B):
        """(dlogit (B, n*n), dvpre (B,)) of the last step: the gradients wrt the policy logits and the value head's pre-activation"""
        dl, dv = np.zeros((B, self.n * self.n), np.float32), np.zeros(B, np.float32)
        _lib.check(_lib.load().oz_trainer_get_head_grads(self._h, B, _lib.p_f32(dl), _lib.p_f32(dv)))
        return dl, dv

    def bn_stats(self, layer):
        """(mean, rstd) of the batch as the BN forward of `layer` (0 .. 5) left them: rstd = 1 / sqrt(biased variance + 1e-3)"""
        co = self._layer_shape(layer)[2]
        mean, rstd = np.zeros(co, np.float32), np.zeros(co, np.float32)
        _lib.check(_lib.load().oz_trainer_get_bn_stats(self._h, layer, _lib.p_f32(mean), _lib.p_f32(rstd)))
        return mean, rstd

    def adam_state(self, index):
        """(m, v): the two Adam moments of trainable array `index` (get_weights() order)"""
        m, v = np.zeros(self.shapes[index], np.float32), np.zeros(self.shapes[index], np.float32)
        _lib.check(_lib.load().oz_trainer_get_adam_state(self._h, index, _lib.p_f32(m), _lib.p_f32(v)))
        return m, v

    def plan(self):
        """{layer 1 .. 5: dict(fwd_kernel, fwd_kslices, dgrad_kernel, dgrad_kslices, dgrad_tap_skip, wgrad_kernel, wgrad_msplit, bn_fwd, bn_bwd,
        bn_bwd_rs), 0 (conv1, no GEMM): dict(bn_fwd, bn_bwd, bn_bwd_rs, conv1_s1)} of the last step, as the launchers reported it
        (oz_trainer_get_plan); bn_fwd: fused32 / fused64 / stream, bn_bwd: fused / split"""
        F = _lib.TRAINER_PLAN_FIELDS
        v = np.zeros(_lib.TRAINER_PLAN_ROWS * F, np.int32)
        _lib.check(_lib.load().oz_trainer_get_plan(self._h, _lib.p_i32(v), v.size))
        out = {}
        for l in range(6):
            row = l - 1 if l else _lib.TRAINER_PLAN_ROWS - 1
            f = [int(x) for x in v[row * F:(row + 1) * F]]
            bn = dict(bn_fwd=_lib.TRAINER_BN_FWD_NAMES[f[8]], bn_bwd=_lib.TRAINER_BN_BWD_NAMES[f[9]], bn_bwd_rs=f[10])
            if l == 0:
                out[l] = dict(bn, conv1_s1=f[11])
            else:
                out[l] = dict(fwd_kslices=f[0], fwd_kernel=_lib.NET_KERNEL_NAMES[f[1]], dgrad_kslices=f[2], dgrad_kernel=_lib.NET_KERNEL_NAMES[f[3]],
                              dgrad_tap_skip=bool(f[4]), wgrad_kernel=_lib.TRAINER_WGRAD_NAMES[f[5]], wgrad_msplit=f[6], **bn)
        return out

    @property
    def step(self):
        s = C.c_int64()
        _lib.check(_lib.load().oz_trainer_step_count(self._h, C.byref(s)))
        return s.value


def pack_examples(examples, board_size, in_channels=2):
    """the reference's example tuples (board, policy (n,n), z) -> (own u64[N], opp u64[N], pi f32[N, n*n], z f32[N]).
    ONN boards are (n,n,2) {0,1} (channel 0 -> own, 1 -> opp); BNN boards are (n,n) with +1 / -1."""
    N, n = len(examples), board_size
    boards = np.asarray([e[0] for e in examples])
    if in_channels == 1:
        boards = np.stack([boards == 1, boards == -1], axis=-1)
    boards = boards.astype(bool).reshape(N, n, n, 2)
    weights = (np.uint64(1) << (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(8) + np.arange(n, dtype=np.uint64)[None, :]))
    own = (boards[..., 0] * weights).sum(axis=(1, 2), dtype=np.uint64)
    opp = (boards[..., 1] * weights).sum(axis=(1, 2), dtype=np.uint64)
    pi = np.asarray([e[1] for e in examples], dtype=np.float32).reshape(N, n * n)
    z = np.asarray([e[2] for e in examples], dtype=np.float32).reshape(N)
    return own, opp, pi, z


VAL_KEYS = ("loss", "pi-reshaped_loss", "v_loss", "policy_top1", "value_sign")      # History.history gains "val_" + each with validation data


def holdout_slots(held, capacity, total, new_examples, share):
    """the newest examples of a ReplayBuffer as a validation split: (train_slots, validation_slots), int32.  held / capacity / total: the buffer's
    info() after an append that wrote `new_examples` examples; V = floor(share * min(new_examples, held)) validation examples, the running
    indices [total - V, total) modulo capacity (the ring's slot rule); the training slots are every other held slot, ascending.  0 < share <= 0.5.
    A pure function (no GPU)."""
    if not 0.0 < share <= 0.5:
        raise ValueError(f"share={share!r}: the held-out share of the new examples lies in (0, 0.5]")
    held, capacity, total, new_examples = int(held), int(capacity), int(total), int(new_examples)
    assert 0 <= held <= capacity and held == min(total, capacity) and new_examples >= 0, (held, capacity, total, new_examples)
    V = int(np.floor(share * min(new_examples, held)))
    val = (np.arange(total - V, total, dtype=np.int64) % max(capacity, 1)).astype(np.int32)
    keep = np.ones(held, bool)
    keep[val] = False
    return np.flatnonzero(keep).astype(np.int32), val


def _record_epoch(hist, ep, epochs, means, verbose, trainer=None, val=None, aux_means=None):
    for k, mean in zip(("loss", "pi-reshaped_loss", "v_loss"), means):
        hist.history[k].append(float(mean))
    if aux_means is not None:
        for k, mean in zip(AUX_KEYS, aux_means):
            hist.history[k].append(float(mean))
    if val is not None:
        for k in VAL_KEYS:
            hist.history.setdefault("val_" + k, []).append(float(val[k]))
    hist.epoch.append(ep)
    if hasattr(trainer, "step_info") and trainer.step > 0:
        info = trainer.step_info()
        hist.lr.append(info["lr_s"])
        hist.grad_norm.append(info["grad_norm"] if trainer.optimizer()["global_clipnorm"] > 0 else None)
    if verbose:
        print(f"Epoch {ep + 1}/{epochs} - loss: {hist.history['loss'][-1]:.4f} - pi-reshaped_loss: "
              f"{hist.history['pi-reshaped_loss'][-1]:.4f} - v_loss: {hist.history['v_loss'][-1]:.4f}"
              + ("" if aux_means is None else "".join(f" - {k}: {m:.4f}" for k, m in zip(AUX_KEYS, aux_means)))
              + ("" if val is None else "".join(f" - val_{k}: {val[k]:.4f}" for k in VAL_KEYS)))


def fit_replay(trainer, replay, batch_size=32, epochs=10, shuffle_seed=0, verbose=None, validation_slots=None):
    """`fit(..., resident=True)` on the examples a ReplayBuffer holds, read in place on the device (oz_trainer_fit_epoch_replay): the same
    per-epoch order RandomState(shuffle_seed + ep).permutation(len(replay)) over the slots, the same batches, steps, weights and losses
    as fit() on replay.read().  Single-process training.

    validation_slots (None: as ever): slots held out of the fit (holdout_slots) -- the epochs train on the other held slots, ascending, in the
    order train_slots[RandomState(shuffle_seed + ep).permutation(len(train_slots))], and after every epoch the held-out slots are evaluated in
    inference mode (Trainer.evaluate_replay): History.history gains val_loss, val_pi-reshaped_loss, val_v_loss, val_policy_top1, val_value_sign."""
    N = len(replay)
    aux = bool(getattr(trainer, "aux", False))
    if aux and not getattr(replay, "aux", False):
        raise ValueError("fit_replay: a trainer with auxiliary heads needs a replay buffer that keeps the final pairs: ReplayBuffer(..., aux=True)")
    hist = History(aux)
    train_slots = None
    if validation_slots is not None:
        validation_slots = np.ascontiguousarray(validation_slots, dtype=np.int32).ravel()
        keep = np.ones(N, bool)
        keep[validation_slots] = False
        train_slots = np.flatnonzero(keep).astype(np.int32)
        N = len(train_slots)
    for ep in range(epochs if N else 0):
        order = np.random.RandomState(shuffle_seed + ep).permutation(N)
        if train_slots is not None:
            order = train_slots[order]
        means = np.asarray(trainer.fit_epoch_replay(replay, order, batch_size), dtype=np.float64)
        val = trainer.evaluate_replay(replay, validation_slots, batch_size) if validation_slots is not None and validation_slots.size else None
        _record_epoch(hist, ep, epochs, means, verbose, trainer, val, trainer.aux_losses(epoch=True) if aux else None)
    trainer.sync()
    return hist


def fit(trainer, own, opp, pi, z, batch_size=32, epochs=10, shuffle_seed=0, allreduce=None, verbose=None, resident=None, validation=None,
        fin_own=None, fin_opp=None):
    """keras Model.fit(x, y, batch_size, epochs) with shuffle=True (the default the reference relies on).
    `allreduce(trainer)` -- if given -- averages the gradient arena across ranks between backward and apply.

    resident (default: True without an all-reduce): the examples are uploaded ONCE (oz_trainer_set_dataset) and every
    epoch is one library call that runs its optimiser steps back to back on the device (oz_trainer_fit_epoch) -- the
    same shuffled order, batches, steps and weights as the step-wise loop, without a host copy or a synchronisation
    per step.  With an all-reduce (data-parallel training) the loop stays step-wise: the collective sits between
    backward and apply.

    validation (None: as ever): (own, opp, pi, z) of held-out examples, evaluated in inference mode after every epoch (Trainer.evaluate: moving BN
    statistics, no dropout); History.history gains val_loss, val_pi-reshaped_loss, val_v_loss, val_policy_top1, val_value_sign (Keras' names).
    With an all-reduce each rank evaluates its own validation examples: no collective is added.

    fin_own / fin_opp (a trainer with auxiliary heads): the examples' final pairs; History.history gains ownership_loss and score_loss,
    accumulated per epoch in float64 in example order like the three losses.  Without them such a trainer trains with every mask 0."""
    N = len(z)
    aux = bool(getattr(trainer, "aux", False))
    assert aux or (fin_own is None and fin_opp is None), "fin_own / fin_opp feed the auxiliary heads (Trainer(..., aux_heads=...))"
    fin = None
    if fin_own is not None:
        fin = (np.ascontiguousarray(fin_own, dtype=np.uint64).ravel(), np.ascontiguousarray(fin_opp, dtype=np.uint64).ravel())
    hist = History(aux)
    if resident is None:
        resident = allreduce is None
    assert not (resident and allreduce is not None), "the resident path has no room for a per-step all-reduce"
    if resident:
        if fin is not None:
            trainer.set_dataset(own, opp, pi, z, fin[0], fin[1])
        else:
            trainer.set_dataset(own, opp, pi, z)
    for ep in range(epochs):
        order = np.random.RandomState(shuffle_seed + ep).permutation(N)
        aux_means = None
        if resident:
            means = np.asarray(trainer.fit_epoch(order, batch_size), dtype=np.float64)
            if aux:
                aux_means = trainer.aux_losses(epoch=True)
        else:
            tot, seen = np.zeros(5 if aux else 3), 0
            for s in range(0, N, batch_size):
                idx = order[s:s + batch_size]
                failed = None
                try:
                    if fin is not None:
                        losses = trainer.forward_backward(own[idx], opp[idx], pi[idx], z[idx], fin[0][idx], fin[1][idx])
                    else:
                        losses = trainer.forward_backward(own[idx], opp[idx], pi[idx], z[idx])
                except Exception as e:                           # the f16x2 range guard, a bad batch shape, an out-of-memory: this rank's step is invalid
                    if allreduce is None:
                        raise
                    failed, losses = e, np.zeros(5 if aux else 3)
                if allreduce is not None:
                    # a rank that failed still joins the collective (with a poisoned arena), so no peer blocks in the all-reduce and
                    # EVERY rank raises together
                    allreduce(trainer, failed=failed)
                trainer.apply()
                tot += np.asarray(losses) * len(idx)            # keras reports the sample-weighted running mean
                seen += len(idx)
            means = tot / max(seen, 1)
            if aux:
                means, aux_means = means[:3], means[3:]
        val = trainer.evaluate(*validation, batch_size=batch_size) if validation is not None and len(validation[3]) else None
        _record_epoch(hist, ep, epochs, means, verbose, trainer, val, aux_means)
    trainer.sync()
    return hist
