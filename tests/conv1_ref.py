"""Reference and exact float32 restatement of the inference conv1 kernels (k_conv1, k_conv1_h2) -- TEST INFRASTRUCTURE ONLY (CPU, NumPy).

conv1 maps the two 0 / 1 planes of a board to relu(BN(conv 3x3 'same')), C channels per pixel.  The planes are 0 / 1, so every product is exact and
the kernels' float32 result is DETERMINED by their order of additions: the live taps in (ky, kx) order, own plane then opponent plane (a tap
outside the board is skipped by k_conv1 and adds an exact zero in k_conv1_h2), then fmaf(acc, scale, shift), then the ReLU.  `model` restates
that, and its final FMA is exact (`fma32_exact`): computed in float64 -- product exact, ONE rounding -- and every element whose float64 value lies
within a few float64 ulps of a float32 rounding boundary is rounded again from the exact rational value (fractions.Fraction).  So precision f32
and bf16x3 (whose three planes add up to the float32 value exactly) are held to EQUALITY with the model, no tolerance, no element left out.

precision f16x2 stores the row in the h2 layout: with s = v * 2^e (e the channel's power of two, an exact scaling), h1 = fp16(s), h2 = fp16(s - h1),
and the diagnostic hook returns (h1 + h2) * 2^-e.  The representation bound (`h2_bound`), derived here and checked by
tests/test_heads_parity_cpu.py::test_h2_representation_bound against layer_ref.h2_planes:
  fp16 keeps 11 significand bits: |s - h1| <= 2^-11 |s| for s in fp16's normal range, and s - h1 is exact in float32;
  r = s - h1 rounds to h2 with |r - h2| <= 2^-11 |r| <= 2^-22 |s| while |r| >= 2^-14 (fp16 normal), else on fp16's subnormal grid of spacing 2^-24:
  |r - h2| <= 2^-25.  An s below 2^-14 makes h1 itself subnormal: |s - h1| <= 2^-25, r is then a multiple of 2^-149 .. below 2^-25 and h2 rounds it
  to the same grid: |r - h2| <= 2^-25 again.
  => |(h1 + h2) - s| <= max(2^-22 |s|, 2^-25) for 0 <= s <= 65504, and in the network's units that bound times 2^-e.
The commit-time scaling folds 2^e into the BN scale and shift (both exact), so s is the float32 restatement's value times 2^e, bit for bit.

For the record the GPU test also prints err / E32 under layer_ref's statistic (norm_c = max |z64[:, c]| before the ReLU)."""
from fractions import Fraction

import numpy as np

import layer_ref as R
from oracle import nn_numpy

F32, F64 = np.float32, np.float64
H2_MAX = 65504.0


def kernel_weights(weights):
    """conv1's kernel as the device holds it, (9, 2, C) float32: as stored for the two-plane network; for the one-plane network (x = own - opp)
    plane 0 = w, plane 1 = -w"""
    k = np.asarray(weights[0], F32)
    C = k.shape[3]
    if k.shape[2] == 1:
        k = np.concatenate([k, -k], axis=2)
    return k.reshape(9, 2, C)


def z64(weights, own, opp, n):
    """conv1's BN output BEFORE the ReLU in float64, (boards n n, C)"""
    w = [np.asarray(a, F64) for a in weights[:6]]
    x = nn_numpy.planes(own, opp, n, F64)
    if w[0].shape[2] == 1:
        x = x[..., 0:1] - x[..., 1:2]
    z = nn_numpy._bn(nn_numpy._conv3x3(x, w[0], w[1], True), *w[2:6])
    return z.reshape(-1, z.shape[-1])


def out32(weights, own, opp, n):
    """the yardstick: relu(BN(conv1)) in NumPy float32, (boards n n, C)"""
    return R.conv1_out(weights, own, opp, n, F32).reshape(-1, np.asarray(weights[0]).shape[3])


def accumulate(weights, own, opp, n):
    """the kernels' float32 accumulator, (boards, n, n, C): the live taps added in (ky, kx) order, own then opponent"""
    k = kernel_weights(weights)
    x = nn_numpy.planes(own, opp, n, F32)
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros(x.shape[:3] + (k.shape[2],), F32)
    for ky in range(3):
        for kx in range(3):
            for plane in range(2):
                bit = xp[:, ky:ky + n, kx:kx + n, plane, None] != 0
                acc = (acc + np.where(bit, k[ky * 3 + kx, plane], F32(0))).astype(F32)     # fmaf(1, w, acc) = acc + w rounded once; fmaf(0, w, acc) = acc
    return acc


def _round_fraction_to_f32(q, lo, hi):
    """the float32 nearest to the rational q, lo <= q <= hi adjacent float32 values (ties to even)"""
    mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
    if q != mid:
        return lo if q < mid else hi
    return lo if (np.array(lo, F32).view(np.uint32) & 1) == 0 else hi


def fma32_exact(a, b, c):
    """fmaf(a, b, c) on float32 arrays (broadcast), correctly rounded for EVERY element; -> (result float32, elements recomputed exactly)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    s = a.astype(F64) * b.astype(F64) + c.astype(F64)         # exact product, one rounding (to float64)
    r = s.astype(F32)                                         # second rounding: wrong only where s sits at a float32 midpoint +- the first rounding
    r64 = r.astype(F64)
    away = np.where(s >= r64, F32(np.inf), F32(-np.inf))
    nb64 = np.nextafter(r, away).astype(F64)                  # the float32 neighbour on s's side of r
    mid = 0.5 * (r64 + nb64)
    near = np.isfinite(nb64) & (np.abs(s - mid) <= 2 * np.spacing(np.abs(s)))
    r = r.copy()
    for i in zip(*np.nonzero(near)):
        q = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((F32(r64[i]), F32(nb64[i])))
        r[i] = _round_fraction_to_f32(q, lo, hi)
    return r, int(near.sum())


def model(weights, own, opp, n, scale=None, shift=None):
    """what k_conv1 writes, (boards n n, C) float32, exactly; scale / shift default to layer_ref._fold's (oz_net_commit's fold)"""
    if scale is None:
        scale, shift = R._fold(weights, 0)
    acc = accumulate(weights, own, opp, n)
    y, exact = fma32_exact(acc, scale, shift)
    y = np.where(y > 0, y, F32(0)).astype(F32)
    return y.reshape(-1, y.shape[-1]), exact


def h2_bound(v32, aexp):
    """per element: the largest |hook - v32| the h2 layout allows for the float32 value v32 >= 0 of a channel scaled by 2^aexp (module docstring)"""
    s = np.ldexp(np.asarray(v32, F64), np.asarray(aexp))
    assert np.all(s >= 0) and np.all(s <= H2_MAX)
    return np.ldexp(np.maximum(s * 2.0 ** -22, 2.0 ** -25), -np.asarray(aexp))


def h2_value(v32, aexp):
    """the value the hook returns if the kernel splits as layer_ref.h2_planes does (printed for the record: not asserted)"""
    s = np.ldexp(np.asarray(v32, F32), np.asarray(aexp)).astype(F32)
    h1, h2 = R.h2_planes(s)
    return np.ldexp(h1.astype(F64) + h2.astype(F64), -np.asarray(aexp))


# ------------------------------------------------------------------ boards
def pack(mask):
    """(boards, 8, 8) bool -> uint64 bitboards, bit = row * 8 + col"""
    bit = (np.uint64(1) << np.arange(64, dtype=np.uint64)).reshape(8, 8)
    return (np.asarray(mask, bool) * bit).sum(axis=(1, 2), dtype=np.uint64)


def edge_boards(n):
    """boards that hit every tap and border of an n x n board: empty, all own, all opp, both checkerboards, one disc on each square for own and
    for opp -> (own, opp) uint64 arrays of 5 + 2 n^2 boards"""
    sq = np.zeros((8, 8), bool)
    sq[:n, :n] = True
    yy, xx = np.mgrid[0:8, 0:8]
    chk = ((yy + xx) % 2 == 0) & sq
    zero = np.zeros((8, 8), bool)
    own, opp = [zero, sq, zero, chk, sq & ~chk], [zero, zero, sq, sq & ~chk, chk]
    for y in range(n):
        for x in range(n):
            one = zero.copy()
            one[y, x] = True
            own += [one, zero]
            opp += [zero, one]
    return pack(np.array(own)), pack(np.array(opp))
