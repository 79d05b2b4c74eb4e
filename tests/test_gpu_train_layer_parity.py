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
the plan.  Left out, with the reason:
  * f16x2 H2BigPP / H2MidPP (the 256 / 192-row ping-pong tiles) and the bf16x3 256-row tile need ceil(M / 256) x (N / 256) >= 192 row tiles: at 512
    filters more than 24320 rows = 381 boards of 8x8 (conv2; conv3's data gradient) or 676 of 6x6, the same 50 MB per full-size tensor either
    way -- a trainer of about 1.4 GB, above the 1 GB this file allows itself, and a whole-tensor float64 weight-gradient reference of more than
    100 GFLOP per layer.  The forward and the data gradient of such a case could be checked on the sampled boards alone, without that reference;
    that is not done here, so the trainer's big-tile data gradient through the zero-bordered buffer stays untested (the inference matrix,
    test_gpu_layer_parity.py, runs the same tile configurations on the forward).
  * H2Small cannot be reached from the trainer: oz_gemm_h2_launch takes it only without a split-K buffer, and the trainer always passes one.
One line per (case, tensor, layer) is printed: the worst step's err, E32 and ratio (the table of one run: profiles/train_layer_parity_ratios.txt)."""
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


def measure(tr, w, n, C, B, batch):
    """one step; -> (sampled records [(tensor, layer, gpu, ref32, ref64)], weight-gradient rows [(layer, err, e32, kept)], plan)"""
    tr.forward_backward(*batch)                                    # raises on an f16x2 range refusal
    plan = tr.plan()
    acts = [tr.activation(l, B) for l in range(6)]
    sampled, wrows = [], []
    for l in range(1, 6):
        g = T.geometry(n, C, l)
        x = acts[l - 1] if l <= 3 else acts[l - 1].reshape(B, -1)
        dz = tr.dz(l, B)
        assert dz.shape == (B, g["Hz"], g["Hz"], g["Co"])
        dzi = dz[:, g["zoff"]:g["zoff"] + g["Hout"], g["zoff"]:g["zoff"] + g["Hout"], :]
        s = _sel(B, g["Hout"] ** 2)
        z = tr.preact(l, B)[s]
        sampled.append(("fwd", l, z, T.forward_z(w, l, x[s], np.float32), T.forward_z(w, l, x[s], np.float64)))
        s = _sel(B, g["Hin"] ** 2)
        da = tr.dgrad(l - 1, B)[s]
        r64 = T.dgrad(w, l, dzi[s], np.float64)
        sampled.append(("dgrad", l, da.reshape(r64.shape), T.dgrad(w, l, dzi[s], np.float32), r64))
        r64 = T.wgrad(l, x, dzi, np.float64)
        err, kept = T.statistic(tr.get_grad(6 * l), r64)
        wrows.append((l, err, T.statistic(T.wgrad(l, x, dzi, np.float32), r64)[0], kept))
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
def _case(name, precision, n, C, B, expect, Bmax=None, kind="bisparse", sharp_wgrad=()):
    return dict(name=name, precision=precision, n=n, C=C, B=B, Bmax=Bmax or B, kind=kind, expect=expect, sharp_wgrad=sharp_wgrad)


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
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
_results = {}


def run_case(case):
    name = case["name"]
    if name not in _results:
        precision, n, C, B, kind = (case[k] for k in ("precision", "n", "C", "B", "kind"))
        w = R.network_weights(n, C, kind)
        tr = _trainer(precision, n, C, case["Bmax"], kind)
        count = 1 if B >= T.ROWS_FOR_NORM else -(-T.ROWS_FOR_NORM // B)
        steps = [measure(tr, w, n, C, B, _batch(n, B, 900 + 17 * k)) for k in range(count)]
        rows, plan = evaluate(steps, precision, n, C, B, kind)
        worst = {}
        for r in rows:
            key = (r["tensor"], r["layer"])
            if key not in worst or r["err"] / r["e32"] > worst[key]["err"] / worst[key]["e32"]:
                worst[key] = r
        for r in worst.values():
            print(f"train-parity {precision:7s} {name:22s} {r['tensor']:5s} layer {r['layer']} {kind:8s} B {B:4d} steps {count:2d} {r['kernel']:16s} split {r['split']:2d} "
                  f"{r['cls']:6s} err {r['err']:.3e}  E32 {r['e32']:.3e}  ratio {r['err'] / r['e32']:6.2f}  margin {r['margin']:4.1f}  kept {r['kept']:.2f}")
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
        for l in (1, 2, 3):
            assert plan[l]["fwd_kernel"].startswith(want) and plan[l]["dgrad_kernel"].startswith(want), plan[l]
            assert plan[l]["fwd_kslices"] > 1 and plan[l]["dgrad_kslices"] > 1, plan[l]           # below the big grid the trainer always splits the k loop
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
