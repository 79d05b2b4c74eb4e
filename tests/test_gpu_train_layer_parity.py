"""Per-kernel parity of the trainer's GEMMs at fp32-rounding tolerance (pytest -m gpu).

Every GEMM of one training step -- forward, data gradient and weight gradient of conv2 .. fc2, and the heads' data gradient -- is compared with the
float64 reference OF THAT GEMM evaluated from the device's own tensors of the step (Trainer.activation / preact / dz / dgrad / head_grads), in units
of E32 = what NumPy float32 loses on the same operation and inputs (tests/train_layer_ref.py: references, statistic, margin classes;
tests/test_train_layer_parity_cpu.py derives the sharp margins from CPU models of the split arithmetics and names the shapes that cannot separate).
Dropout stays on (0.3): the references start from the device's a[l - 1], so the masks do not enter.

Bounds.  On the 'bisparse' network (8 kernel entries per output column and per input channel): forward <= MARGIN_FWD (6 / 6 / 16 for f32 / bf16x3 /
f16x2), data gradient <= MARGIN_DGRAD (8 / 8 / 16), weight gradient <= MARGIN_WGRAD (4.5 / 4.5 / 6) where train_layer_ref.wgrad_class says 'sharp'
(f32 / bf16x3: conv4 up to 36 rows; k_wgrad_h2: 128 .. 4096 rows), else the coarse bound 16; the heads' data gradient (a dense sum of n^2 + 1 terms) and everything on the dense network: 16.  The arithmetic
of a tensor is read from the launch plan (Trainer.plan), which every case also asserts: a threshold that moves fails the test instead of emptying it.
norm_c of the forward and the data gradients is taken over the sampled boards of all the steps of a case (a case of fewer than 64 boards runs
ceil(64 / B) steps on fresh batches with the same weights: train_layer_ref's docstring, few-row samples); every element of every step is compared.
Every tensor must keep at least half of its columns (a column is left out only when its float64 reference is identically zero, and must then be
exactly 0.0 on the device); confirmed on the CPU with oracle/train_ref.py before the batch sizes were chosen: 2 boards keep 0.69 .. 0.72 of the
dz columns of fc1 / fc2 (units dead or dropped in both rows) and every column of the 3x3 layers, 5 boards 0.93.

Shapes: the smallest that reach each path, read off the launchers (oz_gemm_f32_launch, oz_gemm_h2_launch, oz_gemm_b3_launch, t_wgrad) and proven from
the plan.

The chip-filling tiles (the `chip` cases: 8x8, 512 filters, 383 .. 1598 boards).  f16x2 H2MidPP / H2BigPP (the 192 / 256-row ping-pong tiles) and
bf16x3's k_gemm_b3_big (256 rows, 'valid' layers only) need ceil(M / 256) x (N / 256) >= 192 blocks: at 512 filters more than 24320 rows = 381
boards of 64 pixels (conv2; conv3's data gradient), 676 of 36 (conv3; conv4's data gradient), 1521 of 16 (conv4).  What is particular to the
trainer on them is the fp32-row epilogue with relu = 0, scale = wscale[l] / dscale[l], and the gather over the zero-bordered dz with pad = 0.
The cases reach H2MidPP and H2BigPP on every forward and every data gradient of the 3x3 layers (h2-b1023-mid36 and h2-b1598-big16 add what the
sizes shared with bf16x3 leave: H2MidPP on the 36-pixel launches, H2BigPP on conv4's forward, which takes H2MidPP from 1521 to 1536 boards and
H2BigPP from 1537 on) and k_gemm_b3_big on the forward of conv3 / conv4 and the data gradients of conv3 / conv4 -- every launch it can serve,
conv2 and its data gradient being 'same' -- each with a partly filled last row tile (but H2MidPP at 684 boards: 228 whole tiles; 383 boards
have the partly filled one).  b3-b37-of-684 runs the 684-board launches on 37 live boards of a trainer that has done a full step.
Which B reaches which kernel is train_layer_ref.tile_rule, asserted without a device by test_train_layer_parity_cpu.py and here against the
plan.  The k-slices are asserted exactly: 1 on the mid / big tiles, trainer_kslices on the 128-row tile -- which is 1 as well once that launch
has more than 128 blocks (more than 8192 rows: the split must fit one round of the chip), so at these sizes H2LowPP and k_gemm_b3 run unsplit too.
Forward and data gradient: the sharp margins, on the sampled boards (three runs: every row position of a 256-row tile; the first, a middle and the
last tile) -- per-row properties of an 8-term sum, the same at any batch.  Weight gradients of the 3x3 layers: every 16th input channel, all taps
and output columns, ALL rows (train_layer_ref.sampled_ci), at the coarse bound; what that bound sees over 24 000 rows and more is rows, octets
and slabs that go missing, not a lost plane product (test_chip_wgrad_bound_sees_lost_rows).  Kept columns, confirmed with oracle/train_ref.py on
this network before the sizes were fixed: at 37 and at 383 boards every dz column of every layer is alive (1.00).
Budget: one layer's tensors at a time on the host (of each downloaded tensor only the sampled boards stay), the trainer deleted before the next
case.  Measured: a bf16x3 trainer of 1535 boards holds 7.3 GB on the device (3.8 GB at 684, 2.5 GB at 383), the test process 1.7 GB on the host
at its peak, a case takes 1 .. 2.2 s; the cases below 383 boards stay within 1 GB.

Other widths (WIDTH_CASES): f32 at 384 filters, both split modes at 768, bf16x3 at 1024 -- the same kernels where the column tiles are three or four,
the 216 / 288 k-tiles are cut into slices that do not divide them (8x8, 768 filters, 64 boards: 2 / 4 / 10 forward slices; 6x6, 32 boards: 9 / 16 / 16;
1024 filters: 7 / 16 / 16) and the slabs sit three tiles apart; same margins, same classes (wgrad_class), plans asserted against tile_plan.  Kept
columns on these shapes: tests/test_train_layer_parity_cpu.py (the float64 oracle, every shape before its batch was fixed).

Left out, with the reason:
  * H2Small cannot be reached from the trainer: oz_gemm_h2_launch takes it only without a split-K buffer, and the trainer always passes one.
  * H2MidPP / H2BigPP from a short call on a large f16x2 trainer: that launcher is keyed on the call's boards, so a short call IS a small case.
  * k_gemm_b3_big with k-slices > 1 or on a 'same' layer, and the network object's mixed plan (b3_big_rows with may_mix): oz_gemm_b3_launch asks
    for neither (test_gpu_layer_parity.py and test_b3_mix_plan_cpu.py hold them on the inference side).
  * 6x6 on the chip-filling tiles: the same kernels and the same gather at other strides, 676 boards and more; not run.
One line per (case, tensor, layer) is printed: the worst step's err, E32 and ratio, and one per case with its time (the table of one run: profiles/train_layer_parity_ratios.txt)."""
import time

import numpy as np
import pytest

import layer_ref as R
import train_layer_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _batch(n, B, seed):
    """test_gpu_train.py's batches: random boards, one-hot policy targets and one dense one, z = +-1"""
    rs = np.random.RandomState(seed)
    valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
    own = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid
    opp = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid & ~own
    pi = np.zeros((B, n * n), np.float32)
    pi[np.arange(B), rs.randint(0, n * n, B)] = 1
    pi[0] = rs.dirichlet(np.ones(n * n)).astype(np.float32)
    z = rs.choice([-1.0, 1.0], B).astype(np.float32)
    return own, opp, pi, z


def _trainer(precision, n, C, Bmax, kind, capture=True):
    from othellozero_amd.trainer import Trainer
    tr = Trainer(n, C, 2, max_batch=Bmax, lr=1e-3, clipvalue=0.5, dropout=0.3, seed=77, precision=precision)
    tr.set_weights(R.network_weights(n, C, kind))
    if capture:
        tr.set_capture(True)
    return tr


def _arith(kernel):
    return "f16x2" if kernel.startswith(("h2_", "oct_h2")) else "bf16x3" if kernel.startswith(("b3", "oct_b3")) else "f32"


def _sel(B, pixels):
    return np.concatenate([np.arange(b0, b0 + nb) for b0, nb in R.sample_runs(B, pixels)])


def measure(tr, w, n, C, B, batch, sampled_wgrad=False):
    """one step; -> (sampled records [(tensor, layer, gpu, ref32, ref64)], weight-gradient rows [(layer, err, e32, kept)], plan).
    One layer at a time: of every downloaded tensor only the sampled boards are kept (and, with sampled_wgrad, every 16th input channel of the 3x3
    layers' inputs for the weight gradient: train_layer_ref.sampled_ci) before the next one is fetched"""
    tr.forward_backward(*batch)                                    # raises on an f16x2 range refusal
    plan = tr.plan()
    sampled, wrows = [], []
    x = tr.activation(0, B)
    for l in range(1, 6):
        g = T.geometry(n, C, l)
        if l > 3:
            x = x.reshape(B, -1)
        dz = tr.dz(l, B)
        assert dz.shape == (B, g["Hz"], g["Hz"], g["Co"])
        dzi = dz[:, g["zoff"]:g["zoff"] + g["Hout"], g["zoff"]:g["zoff"] + g["Hout"], :]
        if g["zoff"]:
            dzi = np.ascontiguousarray(dzi)                        # (the bordered buffer goes)
        del dz
        s = _sel(B, g["Hout"] ** 2)
        z = tr.preact(l, B)[s]
        sampled.append(("fwd", l, z, T.forward_z(w, l, x[s], np.float32), T.forward_z(w, l, x[s], np.float64)))
        s = _sel(B, g["Hin"] ** 2)
        da = tr.dgrad(l - 1, B)[s]
        r64 = T.dgrad(w, l, dzi[s], np.float64)
        sampled.append(("dgrad", l, da.reshape(r64.shape), T.dgrad(w, l, dzi[s], np.float32), r64))
        got = tr.get_grad(6 * l)
        if sampled_wgrad and l <= 3:
            x, got = T.sampled_ci(x, 3), T.sampled_ci(got, 2)
        r64 = T.wgrad(l, x, dzi, np.float64)
        err, kept = T.statistic(got, r64)
        wrows.append((l, err, T.statistic(T.wgrad(l, x, dzi, np.float32), r64)[0], kept))
        del x, dzi, r64, got
        x = tr.activation(l, B) if l < 5 else None
    dl, dv = tr.head_grads(B)
    r64 = T.heads_dgrad(w, dl, dv, np.float64)
    sampled.append(("heads", 5, tr.dgrad(5, B).reshape(r64.shape), T.heads_dgrad(w, dl, dv, np.float32), r64))
    return sampled, wrows, plan


def evaluate(steps, precision, n, C, B, kind):
    """steps: measure()'s results of ONE trainer -> rows dict(tensor, layer, step, err, e32, kept, kernel, split, cls, margin)"""
    rows = []
    plan = steps[0][2]
    assert all(s[2] == plan for s in steps)
    for i in range(len(steps[0][0])):
        tensor, l = steps[0][0][i][:2]
        norm = np.max([T.column_norm(s[0][i][4]) for s in steps], axis=0)
        if tensor == "fwd":
            kernel, split = plan[l]["fwd_kernel"], plan[l]["fwd_kslices"]
            margin = T.MARGIN_FWD[_arith(kernel)]
        elif tensor == "dgrad":
            kernel, split = plan[l]["dgrad_kernel"], plan[l]["dgrad_kslices"]
            margin = T.MARGIN_DGRAD[_arith(kernel)]
        else:
            kernel, split, margin = "heads", 1, T.MARGIN_COARSE
        cls = "sharp" if kind == "bisparse" and tensor != "heads" else "coarse"
        for k, s in enumerate(steps):
            _, _, gpu, r32, r64 = s[0][i]
            err, kept = T.statistic(gpu, r64, norm)
            rows.append(dict(tensor=tensor, layer=l, step=k, err=err, e32=T.statistic(r32, r64, norm)[0], kept=kept, kernel=kernel, split=split, cls=cls,
                             margin=margin if cls == "sharp" else T.MARGIN_COARSE))
    for k, s in enumerate(steps):
        for l, err, e32, kept in s[1]:
            kernel = plan[l]["wgrad_kernel"]
            g = T.geometry(n, C, l)
            cls = T.wgrad_class(_arith(kernel), l, B * g["Hout"] ** 2) if kind == "bisparse" else "coarse"
            rows.append(dict(tensor="wgrad", layer=l, step=k, err=err, e32=e32, kept=kept, kernel=kernel, split=plan[l]["wgrad_msplit"], cls=cls,
                             margin=T.MARGIN_WGRAD[_arith(kernel)] if cls == "sharp" else T.MARGIN_COARSE))
    return rows, plan


# ------------------------------------------------------------------ the matrix
# expect: layer -> the plan fields the case exists for.  f32 runs 128 filters, the split modes 256 (their minimum).
def _case(name, precision, n, C, B, expect, Bmax=None, kind="bisparse", sharp_wgrad=(), chip=False):
    """chip: a case of the chip-filling tiles (8x8, 512 filters, 383 boards and more) -- the 3x3 layers' weight gradients on the sampled input
    channels, and a full Bmax-board step first where the call is shorter (a used trainer: stale packed operands lie behind the live rows)"""
    return dict(name=name, precision=precision, n=n, C=C, B=B, Bmax=Bmax or B, kind=kind, expect=expect, sharp_wgrad=sharp_wgrad, chip=chip)


def _chip(name, precision, B, tiles, Bmax=None):
    """tiles: {layer: (forward kernel, data-gradient kernel)}; the weight gradients run on the octet kernels, split 8 (f16x2: 32 tiles) / 4 (bf16x3: 64)"""
    wg = dict(wgrad_kernel="oct_h2", wgrad_msplit=8) if precision == "f16x2" else dict(wgrad_kernel="oct_b3", wgrad_msplit=4)
    return _case(name, precision, 8, 512, B, {l: dict(wg, fwd_kernel=f, dgrad_kernel=d) for l, (f, d) in tiles.items()}, Bmax=Bmax, chip=True)


_PIX = dict(dgrad_kernel="f32_std_pixmajor", dgrad_tap_skip=True, dgrad_kslices=1)
_NOPIX = dict(dgrad_kernel="f32_std", dgrad_tap_skip=False)
CASES = [
    # ---- f32
    # capacity >= 2 x 128 boards, a multiple of the 128-board tile: the data gradients of conv2 ('same') and of the zero-bordered conv3 / conv4 on
    # pixel-major tiles that skip the taps outside [core_lo, core_hi); the board-resident weight gradient
    _case("f32-b256-tapskip", "f32", 8, 128, 256, {1: dict(_PIX, wgrad_kernel="boards_f32"), 2: dict(_PIX, wgrad_kernel="boards_f32"), 3: dict(_PIX, wgrad_kernel="boards_f32")}),
    _case("f32-b255-noskip", "f32", 8, 128, 255, {1: _NOPIX, 2: _NOPIX, 3: _NOPIX}),
    _case("f32-b192-wconv", "f32", 6, 128, 192, {l: dict(wgrad_kernel="boards_f32") for l in (1, 2, 3)}),
    _case("f32-b191-wtaps16", "f32", 8, 128, 191, {1: dict(wgrad_kernel="taps_f32", wgrad_msplit=16), 2: dict(wgrad_kernel="taps_f32", wgrad_msplit=16),
                                                  3: dict(wgrad_kernel="taps_f32"), 4: dict(wgrad_kernel="taps_f32", wgrad_msplit=1)}),
    # dense layers on 65 / 64 rows: just above / on the weight-stream kernel (forward of fc1 and fc2, data gradient of fc2 and fc1)
    _case("f32-b65-dense-std", "f32", 6, 128, 65, {4: dict(fwd_kernel="f32_std", dgrad_kernel="f32_std"), 5: dict(fwd_kernel="f32_std", dgrad_kernel="f32_std")}),
    _case("f32-b64-dense-skinny", "f32", 6, 128, 64, {4: dict(fwd_kernel="f32_skinny", dgrad_kernel="f32_skinny"), 5: dict(fwd_kernel="f32_skinny", dgrad_kernel="f32_skinny")}),
    # the sharp weight-gradient cases: conv4 over at most 36 rows -- 6x6 at 8, 5 and 2 boards (32, 20, 8 rows), 8x8 at 2 boards (32 rows)
    _case("f32-b8", "f32", 6, 128, 8, {l: dict(wgrad_kernel="taps_f32", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("f32-b5", "f32", 6, 128, 5, {l: dict(wgrad_kernel="taps_f32", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("f32-b2", "f32", 6, 128, 2, {l: dict(wgrad_kernel="taps_f32", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("f32-b2-8x8", "f32", 8, 128, 2, {l: dict(wgrad_kernel="taps_f32", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("f32-dense-net", "f32", 6, 128, 64, {}, kind="dense"),
    # ---- f16x2: forward and data gradient of the 3x3 layers on H2LowPP with the k loop split (trainer_ksplit > 1) at every capacity below the big grid
    _case("h2-b32-woct", "f16x2", 6, 256, 32, {l: dict(fwd_kernel="h2_lowpp", dgrad_kernel="h2_lowpp", wgrad_kernel="oct_h2") for l in (1, 2, 3)}, sharp_wgrad=(1, 2, 3)),
    _case("h2-b31-wf32", "f16x2", 6, 256, 31, {l: dict(fwd_kernel="h2_lowpp", dgrad_kernel="h2_lowpp", wgrad_kernel="taps_f32") for l in (1, 2, 3)}),
    _case("h2-b64", "f16x2", 8, 256, 64, {l: dict(fwd_kernel="h2_lowpp", dgrad_kernel="h2_lowpp", wgrad_kernel="oct_h2", wgrad_msplit=8) for l in (1, 2, 3)}, sharp_wgrad=(1, 2, 3)),
    _case("h2-dense-net", "f16x2", 6, 256, 32, {1: dict(fwd_kernel="h2_lowpp", wgrad_kernel="oct_h2")}, kind="dense"),
    # ---- bf16x3: every capacity takes k_gemm_b3 / k_wgrad_b3
    _case("b3-b2", "bf16x3", 6, 256, 2, {l: dict(fwd_kernel="b3", dgrad_kernel="b3", wgrad_kernel="oct_b3", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("b3-b2-8x8", "bf16x3", 8, 256, 2, {l: dict(wgrad_kernel="oct_b3", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("b3-b5", "bf16x3", 6, 256, 5, {l: dict(wgrad_kernel="oct_b3", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("b3-b8", "bf16x3", 6, 256, 8, {l: dict(wgrad_kernel="oct_b3", wgrad_msplit=1) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("b3-b9-second-octet", "bf16x3", 6, 256, 9, {l: dict(wgrad_kernel="oct_b3", wgrad_msplit=2) for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    # the 128-row tile with trainer_ksplit > 1 (forward and data gradient), the octet split 4
    _case("b3-b32-ksplit", "bf16x3", 8, 256, 32, {l: dict(fwd_kernel="b3", dgrad_kernel="b3", wgrad_kernel="oct_b3", wgrad_msplit=4) for l in (1, 2, 3)}),
    _case("b3-b64", "bf16x3", 8, 256, 64, {l: dict(fwd_kernel="b3", dgrad_kernel="b3", wgrad_kernel="oct_b3", wgrad_msplit=8) for l in (1, 2, 3)}),
    # a call below the capacity: the b3 launches are sized for Bmax (grid, k split), the rows beyond the call must not enter
    _case("b3-b37-of-64", "bf16x3", 8, 256, 37, {l: dict(fwd_kernel="b3", dgrad_kernel="b3", wgrad_kernel="oct_b3") for l in (1, 2, 3)}, Bmax=64),
    _case("b3-dense-net", "bf16x3", 6, 256, 32, {1: dict(fwd_kernel="b3", wgrad_kernel="oct_b3")}, kind="dense"),
    # ---- the chip-filling tiles: 8x8, 512 filters, B chosen so that the last row tile of the named launches is partly filled (train_layer_ref.tile_rule,
    # asserted on the CPU by test_train_layer_parity_cpu.py).  f16x2: H2MidPP (192 rows) / H2BigPP (256 rows); conv3's data gradient reads the zero-bordered dz
    _chip("h2-b383-mid", "f16x2", 383, {1: ("h2_midpp", "h2_midpp"), 2: ("h2_lowpp", "h2_midpp"), 3: ("h2_lowpp", "h2_lowpp")}),
    _chip("h2-b447-big", "f16x2", 447, {1: ("h2_bigpp", "h2_bigpp"), 2: ("h2_lowpp", "h2_bigpp"), 3: ("h2_lowpp", "h2_lowpp")}),
    _chip("h2-b684", "f16x2", 684, {1: ("h2_midpp", "h2_midpp"), 2: ("h2_bigpp", "h2_midpp"), 3: ("h2_lowpp", "h2_bigpp")}),
    # (what the sizes shared with bf16x3 leave to H2MidPP: the 36-pixel launches -- conv3's forward, conv4's data gradient)
    _chip("h2-b1023-mid36", "f16x2", 1023, {1: ("h2_bigpp", "h2_bigpp"), 2: ("h2_midpp", "h2_bigpp"), 3: ("h2_lowpp", "h2_midpp")}),
    _chip("h2-b1535", "f16x2", 1535, {1: ("h2_bigpp", "h2_bigpp"), 2: ("h2_bigpp", "h2_bigpp"), 3: ("h2_midpp", "h2_bigpp")}),
    # (and to H2BigPP: conv4's forward, 1537 boards and more)
    _chip("h2-b1598-big16", "f16x2", 1598, {1: ("h2_midpp", "h2_midpp"), 2: ("h2_bigpp", "h2_midpp"), 3: ("h2_bigpp", "h2_bigpp")}),
    # bf16x3: k_gemm_b3_big on the 'valid' layers only (conv2 and its data gradient stay on the 128-row tile at every size)
    _chip("b3-b383-big", "bf16x3", 383, {1: ("b3", "b3"), 2: ("b3", "b3_big"), 3: ("b3", "b3")}),
    _chip("b3-b684-big", "bf16x3", 684, {1: ("b3", "b3"), 2: ("b3_big", "b3"), 3: ("b3", "b3_big")}),
    _chip("b3-b1535-big", "bf16x3", 1535, {1: ("b3", "b3"), 2: ("b3_big", "b3_big"), 3: ("b3_big", "b3_big")}),
    # 37 boards on a trainer of 684 that has done a full step: 1332 rows of conv3's forward = five whole 256-row tiles, one partly filled, 91 dead.
    # (No f16x2 twin: that launcher is keyed on the call's boards, so a short call is one of the small cases above)
    _chip("b3-b37-of-684", "bf16x3", 37, {1: ("b3", "b3"), 2: ("b3_big", "b3"), 3: ("b3", "b3_big")}, Bmax=684),
]


# ---- widths other than 128 / 256 / 512: 384 filters (f32) and 768 (the split modes: three
# column tiles, 216 k-tiles that trainer_ksplit cuts into 2 .. 16 slices, 9 / 10 / 16 of which do not divide them), one case at 1024 (288 k-tiles in 7).
# The forward k-slices are named here as well as taken from train_layer_ref.tile_plan; the octet split: 72 (f16x2) / 144 (bf16x3) tiles at 768 filters
def _width(name, precision, n, C, B, fwd_slices, wgrad, msplit, Bmax=None, sharp_wgrad=()):
    tile = "h2_lowpp" if precision == "f16x2" else "b3"
    return _case(name, precision, n, C, B, {l: dict(fwd_kernel=tile, dgrad_kernel=tile, fwd_kslices=fwd_slices[l - 1], wgrad_kernel=wgrad, wgrad_msplit=msplit)
                                            for l in (1, 2, 3)}, Bmax=Bmax, sharp_wgrad=sharp_wgrad)


_TAPS1 = dict(wgrad_kernel="taps_f32", wgrad_msplit=1)
WIDTH_CASES = [
    # ---- f32, 384 filters: three 128-column tiles, 108 k-tiles
    # (6x6: conv4 sums 32 rows, the sharp class; fc1 is (1536, 1024), thinned to 4 entries a row: layer_ref.dense_per_row)
    _case("f32-c384-b8", "f32", 6, 384, 8, {l: _TAPS1 for l in (1, 2, 3)}, sharp_wgrad=(3,)),
    _case("f32-c384-b192-wconv", "f32", 8, 384, 192, {l: dict(wgrad_kernel="boards_f32", wgrad_msplit=16) for l in (1, 2, 3)}),      # 6 x 3 tiles
    _case("f32-c384-b65-dense-std", "f32", 8, 384, 65, {4: dict(fwd_kernel="f32_std", dgrad_kernel="f32_std"), 5: dict(fwd_kernel="f32_std", dgrad_kernel="f32_std")}),
    _case("f32-c384-b64-dense-skinny", "f32", 8, 384, 64, {4: dict(fwd_kernel="f32_skinny", dgrad_kernel="f32_skinny"), 5: dict(fwd_kernel="f32_skinny", dgrad_kernel="f32_skinny")}),
    # ---- f16x2, 768 filters
    _width("h2-c768-b64", "f16x2", 8, 768, 64, (2, 4, 10), "oct_h2", 4, sharp_wgrad=(1, 2, 3)),
    _width("h2-c768-b32-6x6", "f16x2", 6, 768, 32, (9, 16, 16), "oct_h2", 4, sharp_wgrad=(1, 2, 3)),
    # ---- bf16x3, 768 filters
    _width("b3-c768-b64", "bf16x3", 8, 768, 64, (2, 4, 10), "oct_b3", 2),
    _width("b3-c768-b32-6x6", "bf16x3", 6, 768, 32, (9, 16, 16), "oct_b3", 2),
    _width("b3-c768-b9-second-octet", "bf16x3", 6, 768, 9, (16, 16, 16), "oct_b3", 2, sharp_wgrad=(3,)),
    _width("b3-c768-b37-of-64", "bf16x3", 8, 768, 37, (2, 4, 10), "oct_b3", 2, Bmax=64),
    # ---- 1024 filters, 6x6: four column tiles; 256 octet tiles leave the weight gradient unsplit
    _width("b3-c1024-b32-6x6", "bf16x3", 6, 1024, 32, (7, 16, 16), "oct_b3", 1),
]
CASES += WIDTH_CASES
CASE_BY_NAME = {c["name"]: c for c in CASES}
_results = {}


def run_case(case):
    name = case["name"]
    if name not in _results:
        precision, n, C, B, kind = (case[k] for k in ("precision", "n", "C", "B", "kind"))
        t0 = time.perf_counter()
        w = R.network_weights(n, C, kind)
        tr = _trainer(precision, n, C, case["Bmax"], kind)
        if case["chip"] and B < case["Bmax"]:
            tr.forward_backward(*_batch(n, case["Bmax"], 899))       # a used trainer: every packed operand filled up to its capacity
        count = 1 if B >= T.ROWS_FOR_NORM else -(-T.ROWS_FOR_NORM // B)
        steps = [measure(tr, w, n, C, B, _batch(n, B, 900 + 17 * k), sampled_wgrad=case["chip"]) for k in range(count)]
        del tr                                                       # (the device memory goes before the next case)
        rows, plan = evaluate(steps, precision, n, C, B, kind)
        worst = {}
        for r in rows:
            key = (r["tensor"], r["layer"])
            if key not in worst or r["err"] / r["e32"] > worst[key]["err"] / worst[key]["e32"]:
                worst[key] = r
        for r in worst.values():
            print(f"train-parity {precision:7s} {name:22s} {r['tensor']:5s} layer {r['layer']} {kind:8s} B {B:4d} steps {count:2d} {r['kernel']:16s} split {r['split']:2d} "
                  f"{r['cls']:6s} err {r['err']:.3e}  E32 {r['e32']:.3e}  ratio {r['err'] / r['e32']:6.2f}  margin {r['margin']:4.1f}  kept {r['kept']:.2f}")
        print(f"train-parity {precision:7s} {name:22s} {C} filters, B {B}, {count} step(s): {time.perf_counter() - t0:.2f} s")
        _results[name] = (rows, plan, count)
    return _results[name]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_train_layer_parity(oz, name):
    case = CASE_BY_NAME[name]
    rows, plan, count = run_case(case)
    # the plan proves that the case ran the kernels, tiles and splits it names
    for layer, fields in case["expect"].items():
        for k, v in fields.items():
            assert plan[layer][k] == v, (layer, k, plan[layer])
    precision = case["precision"]
    if precision != "f32":
        want = {"f16x2": "h2_", "bf16x3": "b3"}[precision]
        # the launchers' rule restated (train_layer_ref.tile_plan): f16x2 is keyed on the call's boards, bf16x3 on the trainer's capacity
        rule = T.tile_plan(precision, case["n"], case["C"], case["B"] if precision == "f16x2" else case["Bmax"])
        for l in (1, 2, 3):
            assert plan[l]["fwd_kernel"].startswith(want) and plan[l]["dgrad_kernel"].startswith(want), plan[l]
            for side in ("fwd", "dgrad"):
                kernel, split = plan[l][side + "_kernel"], plan[l][side + "_kslices"]
                assert (kernel, split) == (rule[l][side + "_kernel"], rule[l][side + "_kslices"]), (l, side, plan[l], rule[l])
                if kernel in T.UNSPLIT_KERNELS:
                    assert split == 1, plan[l]                       # the mid / big tiles never split the k loop
                else:
                    # the 128-row tile: split until one round of the chip is full -- always > 1 below the chip-filling sizes; at those, a launch
                    # of more than 128 blocks of 128 rows has no room for a second slice (trainer_kslices)
                    assert kernel in ("h2_lowpp", "b3") and (split > 1 or case["chip"]), plan[l]
    for l in (4, 5):
        assert plan[l]["fwd_kernel"].startswith("f32_") and plan[l]["dgrad_kernel"].startswith("f32_") and plan[l]["wgrad_kernel"] == "taps_f32", plan[l]
    assert len(rows) == count * (5 * 3 + 1)
    sharp = {r["layer"] for r in rows if r["tensor"] == "wgrad" and r["cls"] == "sharp"}
    assert sharp == set(case["sharp_wgrad"]), sharp
    assert all(r["e32"] > 0 for r in rows)
    assert all(r["kept"] >= 0.5 for r in rows), [(r["tensor"], r["layer"], r["kept"]) for r in rows if r["kept"] < 0.5]
    bad = [(r["tensor"], r["layer"], r["step"], r["kernel"], r["cls"], round(r["err"] / r["e32"], 2), r["margin"]) for r in rows if not r["err"] <= r["margin"] * r["e32"]]
    assert not bad, f"(tensor, layer, step, kernel, class, err / E32, margin) above the margin: {bad}"


# ------------------------------------------------------------------ structure
@pytest.mark.parametrize("precision,C", [("f32", 128), ("f16x2", 256), ("bf16x3", 256)])
def test_dz_border_stays_zero(oz, precision, C):
    """the border of every dz[l] (outside zoff .. zoff + Hout; conv3 and conv4 have one) is exactly 0.0 after a full step and after the short step
    that follows it, on all Bmax boards of the buffer; the interior of the boards of the call is not"""
    n, Bmax = 6, 32
    tr = _trainer(precision, n, C, Bmax, "dense")
    for B in (Bmax, 11):
        tr.forward_backward(*_batch(n, B, 40 + B))
        for l in range(6):
            g = T.geometry(n, C, l) if l else dict(Hz=n, zoff=0, Hout=n)
            dz = tr.dz(l, Bmax)
            inner = np.zeros(dz.shape[1:3], bool)
            inner[g["zoff"]:g["zoff"] + g["Hout"], g["zoff"]:g["zoff"] + g["Hout"]] = True
            assert dz.shape[1] == g["Hz"] and (g["zoff"] == 2) == (l in (2, 3))
            assert np.all(dz[:, ~inner, :] == 0.0), (B, l)
            assert np.any(dz[:B][:, inner, :] != 0.0), (B, l)


@pytest.mark.parametrize("precision,C", [("f32", 128), ("f16x2", 256), ("bf16x3", 256)])
def test_capture_changes_no_bit_and_is_refused_when_off(oz, precision, C):
    n, B = 6, 16
    tr = _trainer(precision, n, C, B, "dense", capture=False)
    batch = _batch(n, B, 5)

    def step():
        losses = tr.forward_backward(*batch)
        g = tr.get_grads()
        return [np.array(losses)] + [g[i] for i in sorted(g)] + list(tr.outputs(B))
    off = step()
    with pytest.raises(oz.OzError) as e:
        tr.dgrad(3, B)                                               # capture off: an error, not stale data
    assert e.value.code == oz.OZ_ERR_STATE
    tr.set_capture(True)
    with pytest.raises(oz.OzError) as e:
        tr.dgrad(3, B)                                               # on, but no step has been captured yet
    assert e.value.code == oz.OZ_ERR_STATE
    on = step()
    assert tr.dgrad(3, B).shape == (B, n - 4, n - 4, C) and np.any(tr.dgrad(0, B) != 0)
    tr.set_capture(False)
    again = step()
    with pytest.raises(oz.OzError) as e:
        tr.dgrad(3, B)
    assert e.value.code == oz.OZ_ERR_STATE
    for a, b, c in zip(off, on, again):
        assert a.shape == b.shape and np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize("precision,C", [("f32", 128), ("f16x2", 256), ("bf16x3", 256)])
def test_one_board_step_is_exactly_zero_below_fc2(oz, precision, C):
    """one board: every training-mode BN sees one row (the dense layers) or few, and below fc2's beta everything is exactly zero -- the BN backward
    of a one-row layer is dy - mean(dy) - xhat mean(dy xhat) with xhat = 0.  Compared for equality only, never used for ratios"""
    n = 6
    tr = _trainer(precision, n, C, 4, "bisparse")
    tr.forward_backward(*_batch(n, 1, 3))
    g = tr.get_grads()
    for l in range(6):
        assert np.all(tr.dz(l, 1) == 0.0), l
        assert np.all(g[6 * l] == 0.0), l
        if l < 5:
            assert np.all(tr.dgrad(l, 1) == 0.0), l
    assert np.any(tr.dgrad(5, 1) != 0.0) and np.any(g[6 * 5 + 3] != 0.0)          # the heads' data gradient and fc2's beta are alive


def test_views_refuse_bad_arguments(oz):
    tr = _trainer("f32", 6, 128, 4, "dense")
    tr.forward_backward(*_batch(6, 4, 1))
    lib = oz.load()
    buf = np.zeros(8, np.float32)
    for fn in (lib.oz_trainer_get_preact, lib.oz_trainer_get_dz, lib.oz_trainer_get_dgrad):
        for layer, B, nelem in ((6, 1, 8), (-1, 1, 8), (5, 5, 8), (5, 0, 8), (5, 1, 8)):
            with pytest.raises(oz.OzError) as e:
                oz.check(fn(tr._h, layer, B, oz.p_f32(buf), nelem))
            assert e.value.code == oz.OZ_ERR_ARG, (layer, B, nelem)
    with pytest.raises(oz.OzError) as e:
        oz.check(lib.oz_trainer_get_plan(tr._h, oz.p_i32(np.zeros(3, np.int32)), 3))
    assert e.value.code == oz.OZ_ERR_ARG
    assert tr.preact(2, 4).shape == (4, 4, 4, 128) and tr.dz(2, 4).shape == (4, 8, 8, 128) and tr.dz(5, 3).shape == (3, 1, 1, 512)
