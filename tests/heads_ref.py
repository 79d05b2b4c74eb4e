"""Reference, yardstick and arithmetic model of the inference heads (k_heads_t<4 / 8 / 16>) -- TEST INFRASTRUCTURE ONLY (CPU, NumPy).

The heads map fc2's rows f2 (rows, 512) to   logits = f2 . Wpi + bpi,  pi = softmax(logits) (row maximum subtracted, as the kernel does),
vpre = f2 . Wv + bv,  v = tanh(vpre).  heads64 / heads32 evaluate that in float64 / NumPy float32 and return (logits, pi, vpre, v).

Statistics (denominators from the float64 reference only; a case's E32 and its logit denominator are taken over ALL the rows of the case -- a
one-board call has one row, 36 or 64 policy entries and ONE value, and the float32 reference's error on so few numbers is anything between 0
and its bound: layer_ref's few-row reasoning):
  rowmax = max over rows and entries of |pi - pi64| / (the row's largest pi64)
  logit  = max |d| / max |logits64|,  d = log pi - log pi64 with the row's mean of d subtracted (the softmax does not see a row constant)
  value  = max |v - v64|
Yardstick: E32 = the same statistics for heads32.  Both policy statistics are asserted: rowmax weighs the entries a search acts on, logit sees a
damaged small entry (at head gain 16 the smallest pi is near 1e-11 and rowmax is blind to it).

model_heads restates the kernel in float32: wave w adds k in [128 w, 128 w + 128) by sequential FMA (the FMA emulated with the exact float64
product, rounded once more to float32), the four partials combined ((p0 + p1) + p2) + p3, then the bias; exp(lg - mx), summed over the A lanes
by the xor butterfly, divided.  The value: lane l of wave w adds k = 128 w + 2 l and + 1 by FMA, the 64 lanes are added by the xor butterfly
(offsets 32, 16, .., 1), the four partials combined the same way, then bv, then tanh.  exp and tanh are taken as the float32 rounding of the
float64 function.  model_deferred_rows restates the staging of a forward whose fc2 left its k-slices to the heads (oz_deferred_finish).

Defects, selected by `defect=` (tests/test_heads_parity_cpu.py evaluates all of them on every run):
  "bf16_2"        f2 carried with 16 significand bits (two bf16 planes instead of three)
  "drop_wave_v"   wave 3's partial missing from the value sum (the policy is untouched)
  "slice_missing" model_deferred_rows: the deferred sum starts one slice late
  "no_relu"       model_deferred_rows: the deferred finish without its ReLU
and two variants a HEALTHY kernel may show, which must stay inside the margins (HEALTHY_VARIANTS):
  "bias_first"    the bias added before the wave combine instead of after -- an order change, kept to show what the statistics do NOT separate
  "libm_ulp"      every exp and tanh result moved by LIBM_ULP float32 ulps, sign at random: the accuracy of the device's expf / tanhf.  ROCm's own
                  documentation on the build machine holds no accuracy table for HIP's device math functions (searched: the installed headers and
                  documents for an ulp figure of expf / tanhf; none), so LIBM_ULP = 2 for both is an ASSUMPTION, not a quoted bound.

Margins (a healthy kernel stays at or below margin x E32), from the models alone, re-derived by tests/test_heads_parity_cpu.py on every run over
board sizes 6 and 8 (A = 36, 64) and head gains 1, 4, 16 -- layer_ref's rule: at least twice the complete model, at least 1.25 x the healthy
variants, at most half the weakest defect asserted in that statistic.  Figures of the run the margins were chosen from (x E32; E32 in brackets):
  rowmax [3.1e-7 .. 2.3e-6]  complete 0.47 .. 1.16  bias_first 0.44 .. 0.93  libm_ulp 0.47 .. 1.37  bf16_2 5.7 .. 7.2 (above the margin, not 2 x)
                             slice_missing >= 2.1e5  no_relu >= 3.7e5                                                    -> MARGIN_PI = 3
  logit  [3.8e-7 .. 4.8e-7]  complete 0.62 .. 0.85  bias_first 0.61 .. 0.90  libm_ulp 0.69 .. 1.56  bf16_2 6.96 .. 8.65
                             slice_missing, no_relu above 2e5                                                            -> MARGIN_LOGIT = 2.5
  value  [5.4e-8 .. 1.4e-7]  complete 0.50 .. 0.81  libm_ulp 1.26 .. 2.73  bf16_2 17.8, 19.4 at gain 1 (asserted; 8.2, 18.2 at gain 4; 0.5, 1.7 at
                             gain 16 with most |vpre| on tanh's flat part: printed)  drop_wave_v >= 3.4e4 at every gain   -> MARGIN_V = 4
These figures are maxima of rounding noise: they move with the boards drawn (an earlier draw gave libm_ulp 1.25 / 1.41 and bf16_2 value 10.3 at
gain 4) and with the host, since E32 and the f2 rows go through NumPy float32 matrix products in the host BLAS's order.  The relations the CPU test
asserts keep at least 15 % of room on them (tightest: value 1.25 x 2.73 = 3.4 against 4; logit 1.25 x 1.56 = 1.95 against 2.5 and 6.96 against 5).
At gain 16 the networks give logits to +-13, a smallest pi64 of 1e-11 and |vpre| to 8.4 (PI_FLOOR is never approached).
"""
import numpy as np

from layer_ref import b3_planes

F32, F64 = np.float32, np.float64
WAVES, WAVE_K, LANES = 4, 128, 64
LIBM_ULP = 2.0
MARGIN_PI = 3.0
MARGIN_LOGIT = 2.5
MARGIN_V = 4.0
MARGIN = {"rowmax": MARGIN_PI, "logit": MARGIN_LOGIT, "value": MARGIN_V}
GAINS = (1.0, 4.0, 16.0)
PI_FLOOR = 1e-35                      # the logit statistic needs log pi finite: no pi64 of a test network may fall below this
HEALTHY_VARIANTS = ("bias_first", "libm_ulp")
HEAD_DEFECTS = ("bf16_2", "drop_wave_v")
DEFERRED_DEFECTS = ("slice_missing", "no_relu")


def scaled_heads(weights, gain):
    """the network with its two head kernels (get_weights() indices 36 and 38) multiplied by `gain`; everything else shared, nothing modified"""
    w = list(weights)
    if gain != 1.0:
        w[36] = (np.asarray(w[36], F32) * F32(gain)).astype(F32)
        w[38] = (np.asarray(w[38], F32) * F32(gain)).astype(F32)
    return w


def head_weights(weights):
    """(wpi (512, A), bpi (A,), wv (512,), bv scalar array (1,)) of a get_weights() list, float32"""
    return (np.asarray(weights[36], F32), np.asarray(weights[37], F32), np.asarray(weights[38], F32).reshape(-1), np.asarray(weights[39], F32).reshape(1))


def _heads(f2, wpi, bpi, wv, bv, dt):
    x, wpi, bpi, wv, bv = (np.asarray(a, dt) for a in (f2, wpi, bpi, wv, bv))
    logits = x @ wpi + bpi
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    pi = e / e.sum(axis=1, keepdims=True)
    vpre = x @ wv.reshape(-1) + bv.reshape(-1)[0]
    v = np.tanh(vpre)
    assert logits.dtype == dt and pi.dtype == dt and v.dtype == dt
    return logits, pi, vpre, v


def heads64(f2, wpi, bpi, wv, bv):
    return _heads(f2, wpi, bpi, wv, bv, F64)


def heads32(f2, wpi, bpi, wv, bv):
    return _heads(f2, wpi, bpi, wv, bv, F32)


# ------------------------------------------------------------------ statistics
def rowmax_statistic(pi, pi64):
    pi64 = np.asarray(pi64, F64)
    return float((np.abs(np.asarray(pi, F64) - pi64) / pi64.max(axis=1, keepdims=True)).max())


def logit_norm(logits64):
    return float(np.abs(np.asarray(logits64, F64)).max())


def logit_statistic(pi, pi64, norm):
    """norm = logit_norm over all the rows of the case (which include these)"""
    pi, pi64 = np.asarray(pi, F64), np.asarray(pi64, F64)
    assert np.all(pi > 0) and np.all(pi64 > 0) and norm > 0
    d = np.log(pi) - np.log(pi64)
    d -= d.mean(axis=1, keepdims=True)
    return float(np.abs(d).max() / norm)


def value_statistic(v, v64):
    return float(np.abs(np.asarray(v, F64) - np.asarray(v64, F64)).max())


def statistics(pi, v, ref64, norm=None):
    """dict(rowmax, logit, value) of (pi, v) against ref64 = heads64(...)'s tuple"""
    logits64, pi64, _, v64 = ref64
    norm = logit_norm(logits64) if norm is None else norm
    assert norm >= logit_norm(logits64)
    return dict(rowmax=rowmax_statistic(pi, pi64), logit=logit_statistic(pi, pi64, norm), value=value_statistic(v, v64))


# ------------------------------------------------------------------ the kernel's arithmetic in float32
def _round32(x64):
    return np.asarray(x64, F64).astype(F32)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum rounded to float64 and then to float32"""
    return _round32(np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64))


def _add32(a, b):
    return (np.asarray(a, F32) + np.asarray(b, F32)).astype(F32)


def _combine(parts, first=None):
    """((p0 + p1) + p2) + p3 in float32; `first` (the bias_first variant) is added to p0 before"""
    s = parts[0] if first is None else _add32(parts[0], first)
    for p in parts[1:]:
        s = _add32(s, p)
    return s


def _butterfly(x):
    """the xor butterfly over the last axis (64 lanes, offsets 32 .. 1): every lane ends with the same float32 sum"""
    lanes = np.arange(x.shape[-1])
    for off in (32, 16, 8, 4, 2, 1):
        x = _add32(x, x[..., lanes ^ off])
    return x


def _ulp_nudge(x32, rs):
    """every element moved by LIBM_ULP of its float32 ulps, up or down at random"""
    x32 = np.asarray(x32, F32)
    sign = rs.choice(np.array([-1.0, 1.0]), size=x32.shape)
    return _round32(x32.astype(F64) + sign * LIBM_ULP * np.spacing(np.abs(x32)).astype(F64))


def model_heads(f2, wpi, bpi, wv, bv, defect=None):
    """(pi, v) float32 of the rows f2 in the kernel's own order (module docstring); defect: None, a HEAD_DEFECTS name or a HEALTHY_VARIANTS name"""
    assert defect in (None,) + HEAD_DEFECTS + HEALTHY_VARIANTS, defect
    x = np.asarray(f2, F32)
    wpi, bpi, wv, bv = np.asarray(wpi, F32), np.asarray(bpi, F32), np.asarray(wv, F32).reshape(-1), np.asarray(bv, F32).reshape(-1)[0]
    rows, K = x.shape
    A = wpi.shape[1]
    assert K == WAVES * WAVE_K and wpi.shape[0] == K and wv.size == K and A <= LANES
    if defect == "bf16_2":
        b1, b2, _ = b3_planes(x)
        x = (b1 + b2).astype(F32)                     # exact: two bf16 planes fit float32
    rs = np.random.RandomState(12345)
    parts, vparts = [], []
    for w in range(WAVES):
        acc = np.zeros((rows, A), F32)
        for k in range(w * WAVE_K, (w + 1) * WAVE_K):
            acc = _fma32(x[:, k:k + 1], wpi[k:k + 1, :], acc)
        parts.append(acc)
        k0 = w * WAVE_K + 2 * np.arange(LANES)
        vp = _fma32(x[:, k0 + 1], wv[k0 + 1], _fma32(x[:, k0], wv[k0], np.zeros((rows, LANES), F32)))
        vparts.append(_butterfly(vp)[:, 0])
    lg = _combine(parts, bpi) if defect == "bias_first" else _add32(_combine(parts), bpi)
    mx = lg.max(axis=1, keepdims=True)
    e = _round32(np.exp((lg - mx).astype(F32).astype(F64)))
    if defect == "libm_ulp":
        e = _ulp_nudge(e, rs)
    pad = np.zeros((rows, LANES), F32)
    pad[:, :A] = e                                    # lanes beyond A contribute exact zeros
    s = _butterfly(pad)[:, :1]
    pi = (e / s).astype(F32)
    if defect == "drop_wave_v":
        vparts[3] = np.zeros(rows, F32)
    vpre = _add32(_combine(vparts), bv)
    v = _round32(np.tanh(vpre.astype(F64)))
    if defect == "libm_ulp":
        v = np.clip(_ulp_nudge(v, rs), -1.0, 1.0).astype(F32)
    return pi, v


def model_deferred_rows(partial, ksplit, scale, shift, defect=None):
    """the f2 rows the heads stage from fc2's k-slices `partial` (ksplit, rows, 512) float32: the slices added in order s = 0, 1, ..., then
    fmaf(a, scale, shift) and the ReLU (oz_deferred_finish); defect: None or a DEFERRED_DEFECTS name"""
    assert defect in (None,) + DEFERRED_DEFECTS, defect
    partial = np.asarray(partial, F32)
    assert partial.shape[0] == ksplit and ksplit > 1
    first = 1 if defect == "slice_missing" else 0
    a = partial[first]
    for s in range(first + 1, ksplit):
        a = _add32(a, partial[s])
    y = _fma32(a, np.asarray(scale, F32), np.asarray(shift, F32))
    return y if defect == "no_relu" else np.where(y < 0, F32(0), y).astype(F32)


# ------------------------------------------------------------------ inputs
_board_cache = {}
MAX_BOARDS = 3200


def boards(n, count, first=0):
    """`count` mover-canonical positions from `first` on, the same sequence for every count: every position of two random playouts (openings ..
    full boards), then random fillings of the n x n square"""
    import minimax_ref
    if n not in _board_cache:
        games = minimax_ref.playout_positions(n, 57 + n, 2)
        own = [b if p == 1 else w for b, w, p in games]
        opp = [w if p == 1 else b for b, w, p in games]
        rs = np.random.RandomState(900 + n)
        a = rs.rand(MAX_BOARDS, 8, 8) < 0.4
        b = (rs.rand(MAX_BOARDS, 8, 8) < 0.4) & ~a
        a[:, n:, :] = a[:, :, n:] = b[:, n:, :] = b[:, :, n:] = False
        bit = (np.uint64(1) << np.arange(64, dtype=np.uint64)).reshape(8, 8)
        pack = lambda m: (m * bit).sum(axis=(1, 2), dtype=np.uint64)
        _board_cache[n] = (np.concatenate([np.array(own, np.uint64), pack(a)])[:MAX_BOARDS], np.concatenate([np.array(opp, np.uint64), pack(b)])[:MAX_BOARDS])
    own, opp = _board_cache[n]
    assert first + count <= own.size
    return own[first:first + count], opp[first:first + count]
