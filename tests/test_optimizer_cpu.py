"""The trainer's optimiser options without a GPU: the new symbols in header, bindings and library; oz_lr_schedule_at (the one definition of the
schedule, a pure host function) against the Python restatement; the refusals; and that the margin of tests/test_gpu_optimizer.py can detect each
modelled single defect of the six-step order.

Margins, by the project's method (tests/test_train_kernel_parity_cpu.py): optimizer_ref.step restates one step of one array in float64; the same
code in float32 is E32; the margin is the existing Adam one, 4 x E32, for p, m, v and e.  The kernel is elementwise, so its healthy ratio is the
float32 evaluation itself (1.00).  Every modelled defect -- the L2 term added after clipvalue, c for 2 c, the decoupled decay with lr_t for lr_s,
the decay taken from w_new, the average fed with the old w, the clip scale applied after the L2 term or after clipvalue, the mask shifted by one
array -- must lie above TWICE the margin in every tensor it acts on (optimizer_ref.SEES), on fc2's kernel (decayed) and bias (not decayed) of the
oracle step at (6, 128, 7), at the option values optimizer_ref holds for the GPU cases (L2_C, WEIGHT_DECAY, AVERAGE_DECAY, the cosine schedule).
The GPU test judges each of three consecutive steps on its own, so a defect counts as caught by the step that shows it most: at step 1 Adam's
update m / sqrt(v) is the gradient's sign whatever its size, and a wrong L2 term shows in the moments only.  The ratios are printed (pytest -s).
What one run printed (err / E32, the largest of the three steps):
  l2 only      L2 after clipvalue 344 (p), 4.0e4 (m, v)   c for 2 c 4.4e5 (p), 1.9e4 (m, v)   mask shifted 4.5e5 (kernel), 5.3e5 (bias)
  decoupled    lr_t for lr_s 1.7e3 (p)   decay from w_new 35 (p)   mask shifted 2.2e3 (kernel), 6.9e3 (bias)
  everything   scale after the L2 term 4.4e5 (p), 1.7e4 (m)   scale after clipvalue 4.4e5 (p), 6.9e6 (m)   average from the old w 1.8e4 (e)
               L2 after clipvalue 338 (p), 25 (e)   decay from w_new 36 (p)
The decay taken from w_new differs from the definition by lr_s lambda (w_new - w), a product of two small numbers: at lambda = 0.25 it stands at 35 x E32
in p (and at 5 x in e, which is why SEES asks for p alone); at AdamW's usual lambda = 0.01 it would be 1.4 x, below any margin -- hence the large
lambda of the GPU cases.  The margin was not widened."""
import os
import re

import numpy as np
import pytest

import optimizer_ref as O
import train_kernel_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
NEW_SYMBOLS = ["oz_trainer_set_optimizer", "oz_trainer_get_optimizer", "oz_trainer_set_lr", "oz_lr_schedule_at", "oz_trainer_get_step_info",
               "oz_trainer_get_weight_average", "oz_trainer_sqsum", "oz_trainer_time_optimizer"]


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "ONE STEP, PER ELEMENT, IN THIS ORDER" in header and "THE L2 TERM IS NOT PART OF THE CLIPPED NORM" in header
    # the struct of the bindings is the header's: same fields in the same order
    body = re.search(r"typedef struct \{([^}]*)\} oz_optimizer;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.Optimizer._fields_]
    import ctypes
    assert ctypes.sizeof(_lib.Optimizer) == 72


# ------------------------------------------------------------------ the schedule
def _at(kind, warmup, total, ratio, lr, step):
    from othellozero_amd import trainer
    return trainer.lr_schedule_at(lr, step, schedule=(kind, warmup, total, ratio))


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_schedule_against_the_restatement(kind):
    """every kind; steps 1 .. 300; warmup 0, 1, 17; a total below, at and above the step (50, 150, 400 and the step itself); final ratio 0 and 0.1.
    4 x 2^-52 relative: cos is within an ulp of the two libms and three roundings follow; constant is compared exactly"""
    worst = 0.0
    for warmup in (0, 1, 17):
        for ratio in (0.0, 0.1):
            for step in range(1, 301):
                for total in {50, 150, 400, max(step, warmup)}:
                    got, want = _at(kind, warmup, total, ratio, 1e-3, step), O.schedule(1e-3, step, kind, warmup, total, ratio)
                    if kind == "constant":
                        assert got == want, (warmup, total, ratio, step)
                    elif want == 0.0:
                        assert abs(got) <= 4 * 2.0 ** -52 * float(F32(1e-3)), (warmup, total, ratio, step, got)      # (cos(pi) + 1 need not cancel exactly)
                    else:
                        rel = abs(got - want) / want
                        worst = max(worst, rel)
                        assert rel <= 4 * 2.0 ** -52, (kind, warmup, total, ratio, step, got, want)
    print(f"schedule {kind}: worst relative difference {worst:.3g}")


def test_schedule_exact_cases():
    """constant with a warm-up, and linear with exactly representable inputs (lr = 2^-10, ratio 0.25, spans that are powers of two): bit for bit"""
    lr = 2.0 ** -10
    for step in range(1, 80):
        assert _at("constant", 16, 0, 1.0, lr, step) == lr * min(1.0, step / 16)
        assert _at("linear", 0, 64, 0.25, lr, step) == lr * (1.0 - 0.75 * min(1.0, step / 64))
        assert _at("linear", 8, 72, 0.25, lr, step) == (lr * (step / 8) if step <= 8 else lr * (1.0 - 0.75 * min(1.0, (step - 8) / 64)))
    assert _at("linear", 0, 64, 0.25, lr, 64) == lr * 0.25 == _at("linear", 0, 64, 0.25, lr, 10 ** 9)
    assert _at("cosine", 0, 64, 0.5, lr, 10 ** 9) == lr * 0.5
    from othellozero_amd import _lib
    import ctypes as C
    out = C.c_double()
    _lib.check(_lib.load().oz_lr_schedule_at(None, 0.125, 7, C.byref(out)))              # NULL: no schedule
    assert out.value == 0.125


def test_refusals():
    from othellozero_amd import _lib, trainer
    bad = [dict(l2=-1e-4), dict(weight_decay=-1e-2), dict(l2=1e-4, weight_decay=1e-2), dict(l2=float("nan")), dict(average_decay=1.0),
           dict(average_decay=1.5), dict(average_decay=-0.1), dict(global_clipnorm=-1.0), dict(schedule=("linear", 0, 10, -0.1)),
           dict(schedule=("cosine", 0, 10, 1.5)), dict(schedule=("linear", 11, 10, 0.5)), dict(schedule=("cosine", 11, 10, 0.5)),
           dict(schedule=("linear", -1, 10, 0.5)), dict(decay_mask=[4]), dict(decay_mask=[35]), dict(decay_mask=1 << 40)]
    for kw in bad:
        with pytest.raises(_lib.OzError) as e:
            trainer.lr_schedule_at(1e-3, 1, **kw)
        assert e.value.code == _lib.OZ_ERR_ARG, kw
    import ctypes as C
    o, out = trainer.make_optimizer(), C.c_double()
    o.schedule = 3
    assert _lib.load().oz_lr_schedule_at(C.byref(o), 1e-3, 1, C.byref(out)) == _lib.OZ_ERR_ARG
    o.schedule = 0
    assert _lib.load().oz_lr_schedule_at(C.byref(o), 1e-3, 0, C.byref(out)) == _lib.OZ_ERR_ARG          # steps count from 1
    assert _lib.load().oz_lr_schedule_at(C.byref(o), 1e-3, 1, None) == _lib.OZ_ERR_ARG
    # what is allowed: one decay at a time, the ends of the ranges, a constant schedule that never looks at total_steps
    for kw in (dict(l2=1e-4), dict(weight_decay=1e-2), dict(average_decay=0.999), dict(schedule=("linear", 10, 10, 0.0)), dict(schedule=("cosine", 0, 10, 1.0)),
               dict(schedule=("constant", 17, 0, 1.0)), dict(decay_mask=[6, 36]), dict(decay_mask=[39])):
        assert trainer.lr_schedule_at(1e-3, 5, **kw) > 0


# ------------------------------------------------------------------ the margins
def _case_options(case, step):
    lr_s = O.schedule(O.LR, step, *O.COSINE) if case == "everything" else O.schedule(O.LR, step)
    if case == "l2":
        return O.options(lr_s, step, c=O.L2_C)
    if case == "decoupled":
        return O.options(lr_s, step, lam=O.WEIGHT_DECAY)
    return O.options(lr_s, step, s=0.37, lam=O.WEIGHT_DECAY, d=O.AVERAGE_DECAY), O.options(lr_s, step, s=0.37, c=O.L2_C, d=O.AVERAGE_DECAY)


CASES = {"l2": ("l2_after_clip", "c_not_2c", "mask_shift"), "decoupled": ("wd_lr_t", "wd_from_new", "mask_shift"),
         "everything": ("s_after_l2", "s_after_clip", "e_old_w", "wd_from_new", "l2_after_clip")}


@pytest.mark.parametrize("case", list(CASES))
def test_margins_detect_every_modelled_defect(case):
    """three consecutive steps on fc2's kernel (decayed) and bias (not decayed); 'everything' runs the scale and the average with the decoupled
    decay and, for the defects of the L2 term, with the L2 term (the two decays exclude each other)"""
    st = K.oracle_step(6, 128, 7)
    arrays = {30: np.asarray(st["w"][30], F32).reshape(-1), 31: np.asarray(st["w"][31], F32).reshape(-1)}
    rs = np.random.RandomState(3)
    state = {i: (p, np.zeros_like(p), np.zeros_like(p), p.copy()) for i, p in arrays.items()}
    seen = {}                                               # the GPU test judges every step: a defect is caught by the step that shows it most
    for stp in (1, 2, 3):
        opts = _case_options(case, stp)
        new = {}
        for i, (p, m, v, e) in state.items():
            g = K.adam_gradients(rs.standard_normal(p.size) * 1e-3)
            assert np.any(g == 0) and np.any(np.abs(g) > 0.5) and np.any(np.abs(g) == F32(1e-20))
            for defect in CASES[case]:
                o = opts if isinstance(opts, dict) else opts[1 if defect in ("s_after_l2", "s_after_clip", "l2_after_clip") else 0]
                avg = e if o["d"] > 0 else None
                dec = i == 30
                if defect == "mask_shift":
                    bad = O.step(p, g, m, v, avg, o, not dec, F32)
                elif not dec:
                    continue
                else:
                    bad = O.step(p, g, m, v, avg, o, dec, F32, defect=defect)
                r64, r32 = O.step(p, g, m, v, avg, o, dec, F64), O.step(p, g, m, v, avg, o, dec, F32)
                for j, key in enumerate("pmve"):
                    if key not in O.SEES[defect] or r64[j] is None:
                        continue
                    err, e32 = O.ratio(bad[j], r64[j], r32[j])
                    k = (defect, key, i)
                    seen[k] = max(seen.get(k, 0.0), err / e32)
            o = opts if isinstance(opts, dict) else opts[0]
            new[i] = O.step(p, g, m, v, e, o, i == 30, F32)
            if o["d"] == 0:
                new[i] = new[i][:3] + (e,)
        state = new
    for (defect, key, i), r in sorted(seen.items()):
        print(f"optimiser model {case:10s} {defect:14s} {key} array {i}  largest ratio of the 3 steps {r:.3g}  margin {O.MARGIN[key]:.1f}")
        assert r > 2 * O.MARGIN[key], (case, defect, key, i, r)
    assert {d for d, _, _ in seen} == set(CASES[case])
