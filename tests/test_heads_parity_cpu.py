"""The margins of the heads and conv1 parity tests (tests/test_gpu_heads_parity.py, tests/test_gpu_conv1_parity.py) come from NumPy models, and can
detect a defect: shown here on the CPU, on every run, never by breaking a kernel on the GPU.

Heads (tests/heads_ref.py).  f2 rows: fc2's float32 output of oracle/nn_numpy.forward on the dense test networks of board size 6 and 8 (A = 36, 64),
the head kernels at gain 1, 4 and 16 (at 16: logits to +-13, the smallest pi64 1e-11, |vpre| to 8.4 -- no pi64 comes near the 1e-35 floor).  For
every (board, gain):
  * the complete float32 model of k_heads_t, and its two healthy variants -- the bias added before the wave combine (an ORDER change: the
    statistics do not and need not separate it, which is asserted: it stays inside the margin) and exp / tanh moved by the assumed 2 ulp of the
    device functions -- stay at or below margin x E32 in all three statistics;
  * every defect exceeds 2 x margin x E32 in at least one asserted statistic: f2 on two bf16 planes in the LOGIT statistic at every gain (6.96 ..
    8.65 against 2 x 2.5; in rowmax 5.7 .. 7.2: above the margin, not always by 2 x) and in the value at gain 1 (17.8, 19.4 against 2 x 4; at
    gain 4 it shows 8.2 and 18.2, and at gain 16, where most |vpre| sit on tanh's flat part, 0.5 and 1.7: printed, not asserted); a wave's
    partial missing from the value sum in the value at every gain (>= 3.4e4; the policy is bit-identical, asserted); a slice missing from the
    deferred sum and the deferred ReLU missing in both policy statistics at every gain, for 4 and for 16 slices (>= 2e5).
  * how the margins were chosen (layer_ref's rule): MARGIN_PI = 3, MARGIN_LOGIT = 2.5 and MARGIN_V = 4 are at least 2 x the complete model (rowmax
    1.16, logit 0.85, value 0.81), at least 1.25 x the healthy variants (libm_ulp: rowmax 1.37, logit 1.56, value 2.73 -- the assumed 2 ulp of
    tanhf at |v| near 1 are 2.2 x the float32 reference's own error there) and at most half the weakest defect asserted in that statistic
    (logit 6.96, value 17.8, rowmax 2.1e5).  test_margins_follow_the_rule recomputes both sides on every run.
  * the figures are maxima of rounding noise and move with the boards drawn and with the host (E32 and the f2 rows go through NumPy float32
    matrix products in the host BLAS's order; heads_ref's docstring has an example).  What is asserted keeps at least 15 % of room on the
    figures above (tightest: value 1.25 x 2.73 = 3.4 against 4; logit 1.95 against 2.5 and 6.96 against 5); the bf16_2 value at gain 4, which
    would have 2 % of room, is printed only.
conv1 (tests/conv1_ref.py): the exact float32 FMA, and the representation bound of the h2 layout around it."""
from fractions import Fraction

import numpy as np
import pytest

import conv1_ref as C1
import heads_ref as H
import layer_ref as R
from oracle import nn_numpy

ROWS = 128
NETS = {6: 128, 8: 256}                      # board -> filters: the smallest networks of the GPU matrix on each board
_cache = {}


def _trunk(n):
    """(weights, f1 rows, f2 rows) float32 of ROWS boards through the oracle"""
    if n not in _cache:
        w = R.network_weights(n, NETS[n], "dense")
        own, opp = H.boards(n, ROWS)
        _, _, acts, _ = nn_numpy.forward(w, own, opp, n, dtype=np.float32, return_activations=True)
        assert acts[5].dtype == np.float32 and acts[5].shape == (ROWS, 512)
        _cache[n] = (w, acts[4], acts[5])
    return _cache[n]


def _case(n, gain):
    key = (n, gain)
    if key not in _cache:
        w, f1, f2 = _trunk(n)
        hw = H.head_weights(H.scaled_heads(w, gain))
        ref = H.heads64(f2, *hw)
        p32 = H.heads32(f2, *hw)
        _cache[key] = (hw, f2, ref, H.statistics(p32[1], p32[3], ref))
    return _cache[key]


def _ratios(n, gain, pi, v):
    _, _, ref, e32 = _case(n, gain)
    s = H.statistics(pi, v, ref)
    return {k: s[k] / e32[k] for k in s}


def _fmt(r):
    return "  ".join(f"{k} {r[k]:9.3g}" for k in ("rowmax", "logit", "value"))


CASES = [(n, g) for n in (6, 8) for g in H.GAINS]


@pytest.mark.parametrize("n,gain", CASES)
def test_gain_keeps_log_pi_finite(n, gain):
    """the float64 policy of the scaled network stays a normal float32 (>= PI_FLOOR): log pi is finite for the logit statistic"""
    _, _, (lg, pi, vpre, v), e32 = _case(n, gain)
    print(f"heads n={n} gain={gain:g}: max|logit| {np.abs(lg).max():.3g}  min pi64 {pi.min():.3g}  max|vpre| {np.abs(vpre).max():.3g}  "
          f"E32 rowmax {e32['rowmax']:.3g} logit {e32['logit']:.3g} value {e32['value']:.3g}")
    assert pi.min() >= H.PI_FLOOR
    assert all(e > 0 for e in e32.values())


@pytest.mark.parametrize("n,gain", CASES)
def test_healthy_model_and_variants_stay_inside_the_margins(n, gain):
    hw, f2, _, _ = _case(n, gain)
    for variant in (None,) + H.HEALTHY_VARIANTS:
        r = _ratios(n, gain, *H.model_heads(f2, *hw, defect=variant))
        print(f"heads-model n={n} gain={gain:4g} {str(variant or 'complete'):14s} {_fmt(r)}   x E32")
        for k in r:
            assert r[k] <= H.MARGIN[k], (variant, k, r[k])
    # the order change moves bits (it IS another rounding sequence) and still cannot be told from the kernel's order by an accuracy statistic
    a, b = H.model_heads(f2, *hw), H.model_heads(f2, *hw, defect="bias_first")
    assert not np.array_equal(a[0], b[0])


@pytest.mark.parametrize("n,gain", CASES)
def test_head_defects_exceed_twice_the_margin(n, gain):
    hw, f2, _, _ = _case(n, gain)
    r = _ratios(n, gain, *H.model_heads(f2, *hw, defect="bf16_2"))
    print(f"heads-model n={n} gain={gain:4g} {'bf16_2':14s} {_fmt(r)}   x E32")
    assert r["logit"] > 2 * H.MARGIN_LOGIT and r["rowmax"] > H.MARGIN_PI
    if gain == 1.0:
        assert r["value"] > 2 * H.MARGIN_V                          # gain 4: 8 .. 21 depending on the host's BLAS, printed only (module docstring)
    healthy = H.model_heads(f2, *hw)
    pi, v = H.model_heads(f2, *hw, defect="drop_wave_v")
    r = _ratios(n, gain, pi, v)
    print(f"heads-model n={n} gain={gain:4g} {'drop_wave_v':14s} {_fmt(r)}   x E32")
    assert np.array_equal(pi, healthy[0])                          # the policy never sees it
    assert r["value"] > 2 * H.MARGIN_V


def _slices(n, ksplit):
    """fc2's raw k-slices (ksplit, rows, 512) float32 from the oracle's f1 rows, with the folded scale / shift"""
    w, f1, _ = _trunk(n)
    k = np.asarray(w[30], np.float32)
    step = 1024 // ksplit
    part = np.stack([f1[:, s * step:(s + 1) * step] @ k[s * step:(s + 1) * step] for s in range(ksplit)]).astype(np.float32)
    return (part,) + R._fold(w, 5)


def _deferred(n, gain, ksplit):
    """(head weights, heads64 of the staged rows, E32 of them, slices, scale, shift)"""
    key = (n, gain, ksplit)
    if key not in _cache:
        w, _, _ = _trunk(n)
        hw = H.head_weights(H.scaled_heads(w, gain))
        part, sc, sh = _slices(n, ksplit)
        rows = H.model_deferred_rows(part, ksplit, sc, sh)
        assert np.all(rows >= 0) and (rows == 0).any()
        ref = H.heads64(rows, *hw)
        assert ref[1].min() >= H.PI_FLOOR
        p32 = H.heads32(rows, *hw)
        _cache[key] = (hw, ref, H.statistics(p32[1], p32[3], ref), part, sc, sh)
    return _cache[key]


@pytest.mark.parametrize("n,gain", CASES)
@pytest.mark.parametrize("ksplit", [4, 16])
def test_deferred_defects_exceed_twice_the_margin(n, gain, ksplit):
    """the reference of the GPU test is evaluated from the rows the diagnostic kernel forms (slices in order, scale, shift, ReLU); a heads kernel
    that staged other rows is judged against those"""
    hw, ref, e32, part, sc, sh = _deferred(n, gain, ksplit)
    s = H.statistics(*H.model_heads(H.model_deferred_rows(part, ksplit, sc, sh), *hw), ref)
    r = {k: s[k] / e32[k] for k in s}
    print(f"heads-model n={n} gain={gain:4g} deferred x{ksplit:<2d} {'complete':14s} {_fmt(r)}   x E32")
    for k in r:
        assert r[k] <= H.MARGIN[k], (k, r[k])
    for defect in H.DEFERRED_DEFECTS:
        bad = H.model_deferred_rows(part, ksplit, sc, sh, defect=defect)
        s = H.statistics(*H.model_heads(bad, *hw), ref)
        r = {k: s[k] / e32[k] for k in s}
        print(f"heads-model n={n} gain={gain:4g} deferred x{ksplit:<2d} {defect:14s} {_fmt(r)}   x E32")
        assert r["rowmax"] > 2 * H.MARGIN_PI and r["logit"] > 2 * H.MARGIN_LOGIT, defect


def test_margins_follow_the_rule():
    """over all (board, gain): every margin >= 2 x the complete model's largest ratio, >= 1.25 x the healthy variants' and <= half the weakest defect
    ratio among the (defect, statistic, gain) combinations that are asserted to separate"""
    complete = {k: 0.0 for k in H.MARGIN}
    variants = {k: 0.0 for k in H.MARGIN}
    weakest = {k: np.inf for k in H.MARGIN}
    for n, gain in CASES:
        hw, f2, _, _ = _case(n, gain)
        r = _ratios(n, gain, *H.model_heads(f2, *hw))
        complete = {k: max(complete[k], r[k]) for k in r}
        for variant in H.HEALTHY_VARIANTS:
            r = _ratios(n, gain, *H.model_heads(f2, *hw, defect=variant))
            variants = {k: max(variants[k], r[k]) for k in r}
        r = _ratios(n, gain, *H.model_heads(f2, *hw, defect="bf16_2"))
        weakest["logit"] = min(weakest["logit"], r["logit"])
        if gain == 1.0:
            weakest["value"] = min(weakest["value"], r["value"])
        weakest["value"] = min(weakest["value"], _ratios(n, gain, *H.model_heads(f2, *hw, defect="drop_wave_v"))["value"])
        for ksplit in (4, 16):
            hw, ref, e32, part, sc, sh = _deferred(n, gain, ksplit)
            for defect in H.DEFERRED_DEFECTS:
                s = H.statistics(*H.model_heads(H.model_deferred_rows(part, ksplit, sc, sh, defect=defect), *hw), ref)
                weakest["rowmax"], weakest["logit"] = min(weakest["rowmax"], s["rowmax"] / e32["rowmax"]), min(weakest["logit"], s["logit"] / e32["logit"])
    for k in H.MARGIN:
        print(f"heads-margin {k:6s}: complete <= {complete[k]:.2f}  healthy variants <= {variants[k]:.2f}  margin {H.MARGIN[k]:g}  weakest asserted defect {weakest[k]:.3g}   x E32")
        assert 2 * complete[k] <= H.MARGIN[k] and 1.25 * variants[k] <= H.MARGIN[k] <= 0.5 * weakest[k], k


# ------------------------------------------------------------------ conv1
def _fma_fraction(a, b, c):
    """fmaf by exact rational arithmetic, element by element (slow: the check of fma32_exact)"""
    out = np.empty(a.shape, np.float32)
    for i in range(a.size):
        q = Fraction(float(a.flat[i])) * Fraction(float(b.flat[i])) + Fraction(float(c.flat[i]))
        r = np.float32(float(q))                         # float(q) is correctly rounded to float64: r is a float32 neighbour of q
        lo = r if Fraction(float(r)) <= q else np.nextafter(r, np.float32(-np.inf))
        hi = lo if Fraction(float(lo)) == q else np.nextafter(lo, np.float32(np.inf))
        out.flat[i] = lo if lo == hi else C1._round_fraction_to_f32(q, lo, hi)
    return out


def test_fma32_exact_is_exact():
    """against rational arithmetic on random operands, and on operands BUILT to sit at a float32 midpoint +- less than a float64 ulp, where rounding
    the float64 sum again is wrong: fma32_exact must find and repair every one"""
    rs = np.random.RandomState(3)
    a = rs.normal(0, 1, 4000).astype(np.float32)
    b = rs.uniform(0.5, 1.5, 4000).astype(np.float32)
    c = rs.uniform(-0.2, 0.2, 4000).astype(np.float32)
    got, _ = C1.fma32_exact(a, b, c)
    assert np.array_equal(got, _fma_fraction(a, b, c))
    # a = 1 + q 2^-23 (q odd), b = 3: a b = 3 + 3 q 2^-23 exactly, an ODD multiple of 2^-23 = the midpoint of two float32 neighbours in [2, 4)
    # (spacing 2^-22); c = +-2^-60 decides the side and is lost by the float64 sum (its ulp there is 2^-51), which lands ON the midpoint: the
    # second rounding then goes to the even neighbour, the wrong one for about half of these
    q = np.arange(1, 129, 2)
    a = (1 + q * 2.0 ** -23).astype(np.float32)
    b = np.full(q.size, 3, np.float32)
    c = np.where(np.arange(q.size) // 2 % 2 == 0, 2.0 ** -60, -2.0 ** -60).astype(np.float32)      # (the even neighbour alternates with q: signs in pairs)
    assert np.array_equal(a.astype(np.float64), 1 + q * 2.0 ** -23) and np.all(c != 0)
    got, exact = C1.fma32_exact(a, b, c)
    want = _fma_fraction(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    print(f"conv1 fma32_exact: {exact} of {q.size} built operands recomputed exactly, the twice-rounded sum is wrong on {(naive != want).sum()}")
    assert exact == q.size and (naive != want).sum() >= q.size // 4       # the repair path is exercised on real double-rounding cases ...
    assert np.array_equal(got, want)                                      # ... and repairs every one


def test_conv1_model_is_the_reference_and_uses_the_exact_fma():
    """the float32 restatement agrees with the float64 reference within float32's own error (E32-class), on the one- and the two-plane network"""
    from othellozero_amd.weights import init_weights
    for n, cin in ((6, 1), (8, 2)):
        w = init_weights(n, seed=5 + n, channels=128, randomize_all=True, in_channels=cin)
        own, opp = C1.edge_boards(n)
        got, _ = C1.model(w, own, opp, n)
        z = C1.z64(w, own, opp, n)
        err, e32 = R.statistic(got, z), R.statistic(C1.out32(w, own, opp, n), z)
        print(f"conv1-model n={n} planes={cin}: err {err:.3g} E32 {e32:.3g} ratio {err / e32:.2f}")
        assert err <= 4 * e32
        sc, sh = R._fold(w, 0)
        empty = got.reshape(own.size, n * n, -1)[0]
        assert np.array_equal(empty, np.broadcast_to(np.maximum(sh, 0), empty.shape))     # the empty board: relu(shift), exactly


def test_h2_representation_bound():
    """conv1_ref.h2_bound holds for layer_ref.h2_planes on every kind of value (normal, residual below fp16's normal range, s below it, zero), and is
    tight within 2 x: the f16x2 conv1 test may hold the device to it"""
    rs = np.random.RandomState(9)
    s = np.concatenate([rs.uniform(0, 0.25, 20000), 2.0 ** rs.uniform(-40, -2, 20000), [0.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 0.25 - 2.0 ** -26]]).astype(np.float32)
    aexp = rs.randint(-3, 6, s.size)
    v = np.ldexp(s, -aexp).astype(np.float32)                     # an exact scaling: v 2^aexp == s
    assert np.array_equal(np.ldexp(v, aexp), s)
    err = np.abs(C1.h2_value(v, aexp) - v.astype(np.float64))
    bound = C1.h2_bound(v, aexp)
    assert np.all(err <= bound)
    rel = (np.ldexp(err, aexp) / np.maximum(s.astype(np.float64) * 2.0 ** -22, 2.0 ** -25)).max()
    print(f"conv1 h2 bound: largest err / bound {rel:.3f}")
    assert rel > 0.5
