"""References of the trainer's auxiliary heads (ownership and score from the games' final boards) -- TEST INFRASTRUCTURE ONLY (CPU, NumPy / torch).

Three groups:
  * the target in plain NumPy: aux_target (oz_aux_target), sym_pair (the symmetry of a pair, cell by cell from the symmetry table's rule),
    own_targets / score_targets / masks;
  * AuxTrainRef: the float64 torch-autograd restatement of a training step WITH the two heads.  oracle/train_ref.py's forward_backward is one
    block, so the forward is restated here with the two heads and the two loss terms behind it; _bn_train, _relu, dropout_keep, planes and apply
    are the oracle's own;
  * per-kernel references of k_t_aux_heads / the weight and bias gradients / k_t_heads_dgrad's adding launch in a `dtype` (float64: the reference, float32: the
    yardstick E32, as in train_kernel_ref), and float32 models in the kernels' own summation order with switches for single defects.

Margins (x E32) of the per-kernel tests: the arithmetic has the shape of the policy / value heads', so they start from train_kernel_ref's heads
margins; tests/test_aux_heads_cpu.py checks each against the models by train_kernel_ref's rule (figures in that test's docstring)."""
import numpy as np
import torch

import train_kernel_ref as K
from oracle.train_ref import TRAINABLE, TrainRef, dropout_keep, planes

F32, F64 = np.float32, np.float64
AUX = (40, 41, 42, 43)                 # Wown (512, A), bown (A,), Wsc (512, 1), bsc (1,)

MARGIN = {
    "aux_o": 8.0, "aux_s": 8.0, "aux_dopre": 8.0, "aux_dspre": 8.0, "aux_loss": 8.0,      # k_t_aux_heads (+ k_t_aux_losses' batch means)
    "aux_dwown": 6.0, "aux_dwsc": 6.0, "aux_dbown": 6.0, "aux_dbsc": 6.0,                 # weight and bias gradients, sums in batch order
    "aux_df2": 8.0,                                                                       # the heads' term of the gradient wrt f2 (k_t_heads_dgrad, add)
}


# ------------------------------------------------------------------ the target
def aux_target(records):
    """oz_aux_target: (fin_own, fin_opp) uint64 of move records; 0 / 0 for a record of an adjudicated game (pad[1] == 1) or a fast one (pad[0] == 1)"""
    rec = np.asarray(records)
    black = rec["player"] == 1
    none = (rec["pad"][:, 0] == 1) | (rec["pad"][:, 1] == 1)
    fo = np.where(black, rec["final_black"], rec["final_white"]).astype(np.uint64)
    fp = np.where(black, rec["final_white"], rec["final_black"]).astype(np.uint64)
    fo[none] = 0
    fp[none] = 0
    return fo, fp


def sym_src(t, n, r, c):
    """training_example_symmetries (training.py:13-23): the source cell of output cell (r, c) under symmetry t -- rot90 k = t // 2 + 1 (CCW), first
    with fliplr (t even) then without"""
    k, flip = (t >> 1) + 1, not (t & 1)
    rr, cc = r, (n - 1 - c) if flip else c
    for _ in range(k & 3):
        rr, cc = cc, n - 1 - rr
    return rr, cc


def sym_board(t, n, b):
    b, out = int(b), 0
    for r in range(n):
        for c in range(n):
            sr, sc = sym_src(t, n, r, c)
            out |= ((b >> (sr * 8 + sc)) & 1) << (r * 8 + c)
    return out


def sym_pair(t, n, fin_own, fin_opp):
    """the pair under symmetry t: both boards, cell by cell"""
    return sym_board(t, n, fin_own), sym_board(t, n, fin_opp)


def _bits(boards, n):
    b = np.asarray(boards, dtype=np.uint64).reshape(-1, 1)
    sq = np.array([r * 8 + c for r in range(n) for c in range(n)], dtype=np.uint64).reshape(1, -1)
    return ((b >> sq) & np.uint64(1)).astype(np.float64)


def own_targets(fin_own, fin_opp, n):
    """t[b][a] = +1 / -1 / 0 for a square of fin_own / of fin_opp / empty, a = row * n + col"""
    return _bits(fin_own, n) - _bits(fin_opp, n)


def score_targets(fin_own, fin_opp, n):
    return (_bits(fin_own, n).sum(axis=1) - _bits(fin_opp, n).sum(axis=1)) / float(n * n)


def masks(fin_own, fin_opp):
    return ((np.asarray(fin_own, np.uint64) | np.asarray(fin_opp, np.uint64)) != 0).astype(np.float64)


def final_pairs(n, B, seed, dead_share=0.25):
    """random final pairs: about `dead_share` of the masks 0 (never sample 1), sample 0 with empties on its final board, the rest full boards"""
    rs = np.random.RandomState(seed)
    valid = np.uint64(sum(1 << (r * 8 + c) for r in range(n) for c in range(n)))
    fo = rs.randint(0, 2**63, size=B, dtype=np.uint64) & valid
    fp = valid & ~fo
    holes = rs.randint(0, 2**63, size=B, dtype=np.uint64) & rs.randint(0, 2**63, size=B, dtype=np.uint64)
    some = rs.rand(B) < 0.5
    some[0] = True
    fo = np.where(some, fo & ~holes, fo)
    fp = np.where(some, fp & ~holes, fp)
    dead = rs.rand(B) < dead_share
    dead[0] = dead[-1] = False                      # (the last sample live: the models' "lost board" must lose something)
    if B > 2:
        dead[1] = True
    fo[dead] = 0
    fp[dead] = 0
    assert (fo[0] | fp[0]) != valid and (fo[0] | fp[0]) != 0
    return fo, fp


def glorot_aux(n, seed):
    """four arrays for the heads, every one randomised (biases too: a zero bias hides its gradient path)"""
    rs = np.random.RandomState(seed)
    A = n * n
    lim = np.sqrt(6.0 / (512 + A))
    return [rs.uniform(-lim, lim, (512, A)).astype(F32), rs.uniform(-0.1, 0.1, A).astype(F32),
            rs.uniform(-0.1, 0.1, (512, 1)).astype(F32), rs.uniform(-0.1, 0.1, 1).astype(F32)]


# ------------------------------------------------------------------ the float64 autograd restatement
class AuxTrainRef(TrainRef):
    def __init__(self, weights, n, w_own, w_score, **kw):
        assert len(weights) == 44
        super().__init__(weights[:40], n, **kw)
        self.w_own, self.w_score = float(w_own), float(w_score)
        self.w += [torch.tensor(np.asarray(a, dtype=np.float64)) for a in weights[40:]]
        for i in AUX:
            self.m[i], self.v[i] = torch.zeros_like(self.w[i]), torch.zeros_like(self.w[i])

    def forward_backward(self, own, opp, pi_target, z_target, fin_own=None, fin_opp=None, relu_masks=None):
        """-> (loss, pi loss, v loss, ownership loss, score loss); the oracle's forward (oracle/train_ref.py:105-139) with the two heads on f"""
        n, A = self.n, self.n * self.n
        self.relu_masks, self.kink_units = relu_masks, 0
        x = torch.tensor(planes(own, opp, n, self.in_channels))
        B = x.shape[0]
        train = TRAINABLE + list(AUX)
        for i in train:
            self.w[i].requires_grad_(True)
            self.w[i].grad = None
        self._new_stats = {}
        h = x.permute(0, 3, 1, 2)
        for layer, same in enumerate((True, True, False, False)):
            blk = 6 * layer
            k = self.w[blk].permute(3, 2, 0, 1)
            zc = torch.nn.functional.conv2d(h, k, self.w[blk + 1], padding=1 if same else 0)
            zc = self._bn_train(zc.permute(0, 2, 3, 1), blk, fused=True)
            h = self._relu(zc, layer).permute(0, 3, 1, 2)
        f = h.permute(0, 2, 3, 1).reshape(B, -1)
        for j, blk in enumerate((24, 30)):
            zd = f @ self.w[blk] + self.w[blk + 1]
            a = self._relu(self._bn_train(zd, blk, fused=False), 4 + j)
            if self.rate > 0:
                keep = torch.tensor(dropout_keep(self.seed, self.step, j, a.numel(), self.rate).reshape(a.shape))
                a = a * keep / (1.0 - self.rate)
            f = a
        f.retain_grad()
        logits = f @ self.w[36] + self.w[37]
        p = torch.softmax(logits, dim=1).reshape(B, n, n)
        v = torch.tanh(f @ self.w[38] + self.w[39])
        t = torch.tensor(np.asarray(pi_target, dtype=np.float64).reshape(B, n, n))
        q = torch.clamp(p / p.sum(dim=2, keepdim=True), 1e-7, 1 - 1e-7)
        loss_pi = (-(t * torch.log(q)).sum(dim=2)).mean()
        zt = torch.tensor(np.asarray(z_target, dtype=np.float64).reshape(B, 1))
        loss_v = ((v - zt) ** 2).mean()
        # the two auxiliary heads on the same post-dropout f
        fo = np.zeros(B, np.uint64) if fin_own is None else np.asarray(fin_own, np.uint64)
        fp = np.zeros(B, np.uint64) if fin_opp is None else np.asarray(fin_opp, np.uint64)
        m = torch.tensor(masks(fo, fp))
        o = torch.tanh(f @ self.w[40] + self.w[41])                                   # (B, A)
        s = torch.tanh(f @ self.w[42] + self.w[43])[:, 0]                             # (B,)
        loss_own = (m * ((o - torch.tensor(own_targets(fo, fp, n))) ** 2).sum(dim=1) / A).sum() / B
        loss_sc = (m * (s - torch.tensor(score_targets(fo, fp, n))) ** 2).sum() / B
        loss = loss_pi + loss_v + self.w_own * loss_own + self.w_score * loss_sc
        loss.backward()
        zero = lambda i: torch.zeros_like(self.w[i])
        self.grads = {i: (self.w[i].grad.detach().clone() if self.w[i].grad is not None else zero(i)) for i in train}
        self.df2 = f.grad.detach().numpy().copy()
        for i in train:
            self.w[i].requires_grad_(False)
        self.outputs = dict(p=p.detach().numpy().reshape(B, A), v=v.detach().numpy()[:, 0], o=o.detach().numpy(), s=s.detach().numpy())
        return loss.item(), loss_pi.item(), loss_v.item(), loss_own.item(), loss_sc.item()

    def apply(self, grads=None):
        """the oracle's Adam step on the forty, then the same step (same t) on the four"""
        grads = grads if grads is not None else self.grads
        super().apply(grads)
        t, b1, b2 = self.step, 0.9, 0.999
        lr_t = self.lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        for i in AUX:
            g = grads[i]
            if self.clip and self.clip > 0:
                g = torch.clamp(g, -self.clip, self.clip)
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            self.w[i] = self.w[i].detach() - lr_t * self.m[i] / (torch.sqrt(self.v[i]) + 1e-7)


# ------------------------------------------------------------------ per-kernel references (dtype: float64 reference / float32 yardstick)
def aux_heads(a5, wown, bown, wsc, bsc, fin_own, fin_opp, n, w_own, w_sc, dtype, defect=None, forward=None):
    """k_t_aux_heads: dict(o (B, A), s (B,), lo, ls (per sample, masked), dopre, dspre (loss weights included)).
    forward: (o, s) computed elsewhere (model_aux_forward: the kernel's own order) in place of this function's dot products.
    defect (CPU models): None | 'mask' (a dead sample trained) | 'normA' (1 / A missing in the ownership gradient) | 'two' | 'tanh' | 'swap' (the pair swapped)"""
    x = np.asarray(a5, dtype)
    B, A = x.shape[0], n * n
    if defect == "swap":
        fin_own, fin_opp = fin_opp, fin_own
    if forward is not None:
        o, s = (np.asarray(v, dtype) for v in forward)
    else:
        o = np.tanh(x @ np.asarray(wown, dtype) + np.asarray(bown, dtype))
        s = np.tanh(x @ np.asarray(wsc, dtype).reshape(-1) + np.asarray(bsc, dtype).reshape(-1)[0])
    m = masks(fin_own, fin_opp).astype(dtype)
    mg = np.ones_like(m) if defect == "mask" else m
    d = o - own_targets(fin_own, fin_opp, n).astype(dtype)
    ds = s - (score_targets(fin_own, fin_opp, n) * A).astype(dtype) / dtype(A)
    two = dtype(1 if defect == "two" else 2)
    da = dtype(1) if defect == "tanh" else dtype(1) - o * o
    dsa = dtype(1) if defect == "tanh" else dtype(1) - s * s
    normA = dtype(B) if defect == "normA" else dtype(B) * dtype(A)
    out = dict(o=o, s=s, lo=m * ((d * d).sum(axis=1) / dtype(A)), ls=m * ds * ds,
               dopre=mg[:, None] * (dtype(F32(w_own)) * (two * d / normA) * da), dspre=mg * (dtype(F32(w_sc)) * (two * ds / dtype(B)) * dsa))
    assert all(v.dtype == dtype for v in out.values())
    return out


def aux_mean_losses(lo, ls, dtype):
    return np.array([np.asarray(lo, dtype).sum() / dtype(len(lo)), np.asarray(ls, dtype).sum() / dtype(len(ls))], dtype)


def aux_reduce(a5, dopre, dspre, dtype):
    """the heads' weight and bias gradients from their own pre-activation gradients: dict(dwown (512, A), dwsc (512,), dbown (A,), dbsc ())"""
    r = K.heads_reduce(a5, dopre, dspre, dtype)
    return dict(dwown=r["dwpi"], dwsc=r["dwv"], dbown=r["dbpi"], dbsc=r["dbv"])


def aux_dgrad(dopre, dspre, wown, wsc, dtype):
    """the term k_t_heads_dgrad's second launch adds: (B, 512) = dopre Wown^T + dspre Wsc^T"""
    return np.asarray(dopre, dtype) @ np.asarray(wown, dtype).T + np.outer(np.asarray(dspre, dtype).reshape(-1), np.asarray(wsc, dtype).reshape(-1))


# ------------------------------------------------------------------ float32 models in the kernels' own order
def _fma(a, b, c):
    """fmaf on float32 arrays: the product is not rounded (float64 holds a 24 x 24 bit product exactly), one rounding of the sum"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def model_aux_forward(a5, wown, bown, wsc, bsc, defect=None):
    """k_t_aux_heads' pre-activations: lane a runs the fmaf chain in k order, then + bias; the score head: lane l adds k = l, l + 64, ... by fmaf,
    the 64 lane sums through the xor-shuffle tree, then + bias.  -> (o, s) float32.  defect: None | 'no_bias' (the bias not added) | 'lost_k' (the
    last block of 64 k left out of both dot products) | 'no_tanh'"""
    x, W = np.asarray(a5, F32), np.asarray(wown, F32)
    K_ = 448 if defect == "lost_k" else 512
    act = (lambda v: v) if defect == "no_tanh" else np.tanh
    acc = np.zeros((x.shape[0], W.shape[1]), F32)
    for k in range(K_):
        acc = _fma(x[:, k:k + 1], W[k:k + 1, :], acc)
    o = act(acc if defect == "no_bias" else (acc + np.asarray(bown, F32)).astype(F32))
    w = np.asarray(wsc, F32).reshape(-1)
    lane = np.zeros((x.shape[0], 64), F32)
    for k0 in range(0, K_, 64):
        lane = _fma(x[:, k0:k0 + 64], w[None, k0:k0 + 64], lane)
    for off in (32, 16, 8, 4, 2, 1):
        lane = (lane + lane[:, np.arange(64) ^ off]).astype(F32)
    s = act(lane[:, 0] if defect == "no_bias" else (lane[:, 0] + np.asarray(bsc, F32).reshape(-1)[0]).astype(F32))
    return o.astype(F32), s.astype(F32)


def model_aux_reduce(a5, dopre, dspre, lost_board=False):
    """the weight and bias gradients in batch order (k_t_heads_wgrad's and k_t_heads_bias' sums on the heads' tensors)"""
    sl = slice(None, -1) if lost_board else slice(None)
    r = K.model_heads_reduce(np.asarray(a5)[sl], np.asarray(dopre)[sl], np.asarray(dspre)[sl])
    return dict(dwown=r["dwpi"], dwsc=r["dwv"], dbown=r["dbpi"], dbsc=r["dbv"])


def model_aux_dgrad(dopre, dspre, wown, wsc, df2_before, defect=None):
    """k_t_heads_dgrad with add set: acc = dspre[b] Wsc[k] (rounded), fmaf over a ascending, df2 += acc.  defect: None | 'no_score' | 'lost_a' (the last square left out)"""
    do, ds = np.asarray(dopre, F32), np.asarray(dspre, F32).reshape(-1)
    W, w = np.asarray(wown, F32), np.asarray(wsc, F32).reshape(-1)
    acc = np.zeros((do.shape[0], 512), F32) if defect == "no_score" else (ds[:, None] * w[None, :]).astype(F32)
    for a in range(W.shape[1] - (1 if defect == "lost_a" else 0)):
        acc = _fma(do[:, a:a + 1], W[None, :, a], acc)
    return (np.asarray(df2_before, F32) + acc).astype(F32)
