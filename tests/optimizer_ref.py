"""Restatement of the trainer's optimiser options -- TEST INFRASTRUCTURE ONLY (CPU, NumPy).

`step` is ONE optimiser step of ONE array in the per-element order that include/othellozero_amd.h defines (scale by the global-norm clip, L2 term,
clipvalue, the two moments, the Adam update with the decoupled decay, the weight average), in float64; evaluated in float32 the same code is the
yardstick E32 (tests/train_kernel_ref.py's method, whose Adam constants, statistic and margin it shares).  The kernel's own parameters enter with the
values the device holds: s, 2 c, lr_s lambda, d and 1 - d are float32 roundings of numbers formed in double on the host, lr_t as train_kernel_ref.adam_lr_t
forms it.  `defect` switches in one modelled single defect (tests/test_optimizer_cpu.py shows that each lies above the margin at the option values
below, which the GPU test uses).

`schedule` restates oz_lr_schedule_at; `norm_bound` is the bound of the float64 sum of squares."""
import math

import numpy as np

import train_kernel_ref as K

F32, F64 = np.float32, np.float64
TRAINABLE = [i for i in range(40) if i >= 36 or i % 6 not in (4, 5)]
STATS = [i for i in range(40) if i not in TRAINABLE]
DEFAULT_MASK = [0, 6, 12, 18, 24, 30, 36, 38]                  # the eight kernels
DEFECTS = ("l2_after_clip", "c_not_2c", "wd_lr_t", "wd_from_new", "e_old_w", "s_after_l2", "s_after_clip", "mask_shift")
# the tensors (p, m, v, e) a defect must show in, given the options it is evaluated under (see test_optimizer_cpu.py)
SEES = {"l2_after_clip": "pmve", "c_not_2c": "pmve", "wd_lr_t": "pe", "wd_from_new": "p", "e_old_w": "e", "s_after_l2": "pmve",
        "s_after_clip": "pmve", "mask_shift": "pe"}
MARGIN = {k: K.MARGIN["adam_p"] for k in "pmve"}               # the existing Adam margin, 4 x E32, for all four tensors

# the option values of the GPU parity cases: chosen on the CPU (test_optimizer_cpu.py) so that every modelled defect lies above twice the margin --
# AlphaZero's c = 1e-4 moves a weight by less than fp32 resolves in three steps, so the cases use larger ones
LR, CLIPVALUE = 1e-3, 0.5
L2_C, WEIGHT_DECAY, AVERAGE_DECAY = 1e-2, 0.25, 0.9
COSINE = ("cosine", 2, 4, 0.1)                                  # step 1 inside the warm-up (f = 0.5), step 2 at its end (1), step 3 on the cosine (q = 0.5, f = 0.55)


def schedule(lr, step, kind="constant", warmup=0, total=0, ratio=1.0):
    """lr_s of the 1-based step, in double like the host; lr as the float32 the library receives"""
    base = float(F32(lr))
    if step <= warmup:
        return base * (step / warmup)
    if kind == "constant":
        return base
    q = min(1.0, (step - warmup) / max(1, total - warmup))
    if kind == "linear":
        return base * (1.0 - (1.0 - ratio) * q)
    assert kind == "cosine", kind
    return base * (ratio + (1.0 - ratio) * (0.5 * (1.0 + math.cos(math.pi * q))))


def lr_t_of(lr_s, step):
    """the float32 lr_t the kernel receives for the scheduled rate lr_s (train_kernel_ref.adam_lr_t with lr_s in place of lr)"""
    return float(F32(lr_s * np.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step)))


def options(lr_s, step, clip=CLIPVALUE, s=None, c=0.0, lam=0.0, d=0.0):
    """one step's parameters: lr_s (double), its lr_t, clipvalue, the clip scale s (None: the global-norm clip is off), c, lambda, d"""
    return dict(lr_s=float(lr_s), lr_t=lr_t_of(lr_s, step), clip=clip, s=s, c=c, lam=lam, d=d)


def step(p, g, m, v, e, o, dec, dtype, defect=None):
    """-> (p, m, v, e) after the step; `dec`: the array is under the decay mask; e None: no average (returned as None)"""
    p, g, m, v = (np.asarray(x, dtype).reshape(-1) for x in (p, g, m, v))
    clip = lambda x: np.clip(x, dtype(-o["clip"]), dtype(o["clip"])) if o["clip"] > 0 else x
    s = dtype(F32(o["s"])) if o["s"] is not None else None
    c2 = dtype(F32(2.0 * o["c"] if defect != "c_not_2c" else o["c"]))
    l2 = dec and o["c"] > 0
    if defect == "s_after_l2":
        g = g + c2 * p if l2 else g
        g = clip(g * s if s is not None else g)
    elif defect == "s_after_clip":
        g = clip(g + c2 * p if l2 else g)
        g = g * s if s is not None else g
    elif defect == "l2_after_clip":
        g = clip(g * s if s is not None else g)
        g = g + c2 * p if l2 else g
    else:
        g = g * s if s is not None else g
        g = g + c2 * p if l2 else g
        g = clip(g)
    m2 = dtype(K.ADAM_B1) * m + dtype(K.ADAM_1MB1) * g
    v2 = dtype(K.ADAM_B2) * v + dtype(K.ADAM_1MB2) * g * g
    w = p - dtype(o["lr_t"]) * m2 / (np.sqrt(v2) + dtype(K.ADAM_EPS))
    if dec and o["lam"] > 0:
        lam = dtype(F32((o["lr_t"] if defect == "wd_lr_t" else o["lr_s"]) * o["lam"]))
        w = w - lam * (w if defect == "wd_from_new" else p)
    e2 = None
    if e is not None:
        e = np.asarray(e, dtype).reshape(-1)
        e2 = dtype(F32(o["d"])) * e + dtype(F32(1.0 - o["d"])) * (p if defect == "e_old_w" else w)
        assert e2.dtype == dtype
    assert w.dtype == dtype and m2.dtype == dtype and v2.dtype == dtype
    return w, m2, v2, e2


def ratio(got, r64, r32, floor=False):
    """err / E32 of one tensor under train_kernel_ref's statistic (one column: the norm is the largest |entry|); -> (err, e32)"""
    err = K.statistic(K.vec(got), K.vec(r64))[0]
    e32 = K.statistic(K.vec(r32), K.vec(r64))[0]
    return err, (max(e32, K.E32_FLOOR) if floor else e32)


def exact_sqsum(arrays):
    """(math.fsum of the exact float64 squares, element count): a float32 squared is exact in float64"""
    flat = np.concatenate([np.asarray(a, F32).reshape(-1) for a in arrays]).astype(F64)
    return math.fsum((flat * flat).tolist()), flat.size


def norm_bound(count):
    """relative bound of the float64 sum of `count` non-negative terms in ANY order, plus one rounding for the root (or the read-back)"""
    return (count + 2) * 2.0 ** -53


def padding_mask(sizes_by_index):
    """a bool mask over the arena (t_layout: every trainable array padded to a multiple of four floats, in get_weights() order) that is True on the padding"""
    parts = []
    for i in TRAINABLE:
        n = int(sizes_by_index[i])
        parts.append(np.concatenate([np.zeros(n, bool), np.ones(-n % 4, bool)]))
    return np.concatenate(parts)
