// oz_train.hip -- one optimiser step of OthelloNN / BaseNN on gfx950.
//
// Replaces NNetWrapper.train (Net/NNet.py:53-68) = keras Model.fit on the graph of Net/OthelloNN.py:42-56 compiled
// with loss=['categorical_crossentropy','mean_squared_error'], Adam(lr, clipvalue=0.5) (BaseNN.py:57: no clipvalue).
// Semantics (restated in oracle/train_ref.py, which is what the parity tests compare with):
//   * BatchNormalization in training mode: batch mean / BIASED batch variance, eps 1e-3, momentum 0.99; the 4-D conv BNs
//     run Keras' fused kernel whose moving-variance update uses the UNBIASED variance, the dense BNs the biased one.
//   * the policy loss is Keras' probability-path categorical cross-entropy applied to the RESHAPED (B, n, n) output:
//     every board row is renormalised, clipped to [1e-7, 1-1e-7], -sum(t log q) per row, mean over batch x rows.
//   * value loss: mean squared error; total = pi + v.   * Dropout: inverted, counter-based keep mask.
//   * Adam as tf.keras: lr_t = lr sqrt(1-b2^t)/(1-b1^t); var -= lr_t m / (sqrt(v) + 1e-7); clipvalue clips g first.
//
// All contractions run on the fp32 matrix cores: forward and data-gradient passes reuse k_gemm_f32 (oz_net.hip; the
// data gradient of a 3x3 convolution is a 3x3 convolution with the taps reversed and the channel roles swapped, 'valid'
// layers through a zero-bordered buffer), the weight gradient is k_wgrad_f32 below (a "TN" implicit GEMM whose k
// index is the batch x pixel row).  Column reductions (BN statistics, BN backward sums, bias gradients) use a
// fixed-order two-stage reduction, so a step is deterministic.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "oz_internal.h"

#define BN_EPS 1e-3f
#define RED_S 256         // row splits of the column reductions (2048 waves of 1 KB loads at 512 channels: the passes are HBM streams)

// ---------------------------------------------------------------- dropout hash (same formula in oracle/train_ref.py)
OZ_HD bool oz_dropout_keep(uint64_t seed, uint64_t step, uint64_t layer, uint64_t idx, float rate) {
    const uint64_t a = oz_sm64(seed + 0x632BE59BD9B4E019ULL * step);
    const uint64_t h = oz_sm64(a ^ ((layer + 1) * 0xD1B54A32D192ED03ULL) ^ (idx * 0x9E3779B97F4A7C15ULL));
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
    return u >= rate;
}

#include "oz_train_fused.h"

// ---------------------------------------------------------------- conv1 forward (raw, + bias) and its weight gradient
// x[b][iy][ix][ch]: cin = 2 -> (own bit, opp bit); cin = 1 -> own bit - opp bit (Net/BaseNN.py:41-44)
__device__ __forceinline__ float t_plane(uint64_t o, uint64_t p, int sq, int ch, int cin) {
    const float a = (float)((o >> sq) & 1), b = (float)((p >> sq) & 1);
    return cin == 2 ? (ch == 0 ? a : b) : a - b;
}

// one thread = one pixel row m x 4 consecutive output channels (16-byte weight loads and stores)
__global__ __launch_bounds__(256) void k_t_conv1_fwd(const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp,
                                                     const int* __restrict__ d_count, int n, int C, int cin,
                                                     const float* __restrict__ W /*[9][cin][C]*/, const float* __restrict__ bias,
                                                     float* __restrict__ z /*[B][n*n][C]*/) {
    const int P = n * n, Q = C / 4;
    const long long M = (long long)(*d_count) * P;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long m = idx / Q;
    if (m >= M) return;
    const int co = (int)(idx % Q) * 4;
    const int b = (int)(m / P), pix = (int)(m % P), y = pix / n, x = pix % n;
    const uint64_t o = own[b], p = opp[b];
    // all 9 * cin weight vectors of this thread's four channels in flight at once (the tap loop with its border test was a chain of 18 dependent
    // L2 round trips: 33 us per launch at the reference's batch, round 5); the products are added in the same tap / plane order, a tap outside
    // the board is skipped as before
    f32x4 w[18];                                            // [tap][plane]: static register indices whatever cin is
#pragma unroll
    for (int i = 0; i < 18; ++i) if ((i & 1) < cin) w[i] = *reinterpret_cast<const f32x4*>(W + (size_t)((i >> 1) * cin + (i & 1)) * C + co);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + co);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
        if (iy < 0 || iy >= n || ix < 0 || ix >= n) continue;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            if (ch >= cin) break;
            const float xv = t_plane(o, p, iy * 8 + ix, ch, cin);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(xv, w[2 * t + ch][k], acc[k]);
        }
    }
    *reinterpret_cast<f32x4*>(z + (size_t)m * C + co) = acc + bv;
}

// dW1[t][ch][co] = sum_m x[m shifted by t][ch] * dz[m][co]: ONE pass over dz -- a thread owns an output channel and keeps the
// 9 * cin sums of its row split in registers (the input planes are bits of the two bitboards, wave-uniform per row)
template <int NB>                          // board size as a constant: the row -> (board, pixel) split is a shift / a multiply, not a 64-bit division per row
__global__ __launch_bounds__(256) void k_t_conv1_wgrad(const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp,
                                                       const int* __restrict__ d_count, int C, int cin,
                                                       const float* __restrict__ dz, float* __restrict__ partial /*[S][9*cin][C]*/, int S) {
    constexpr int n = NB, P = NB * NB;
    const int co = blockIdx.x * 256 + threadIdx.x, sp = blockIdx.y;
    if (co >= C) return;
    const int M = (*d_count) * P;
    float acc[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) acc[i] = 0.f;
    // four rows of the split per trip: their loads (a dz element and two bitboards each) are issued together, the sums stay in row order
    for (int m0 = sp; m0 < M; m0 += 4 * S) {
        float d[4];
        uint64_t o[4], p[4];
        int pixs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int m = m0 + u * S;
            const bool in = m < M;
            const int mm = in ? m : m0;
            const int b = mm / P;
            pixs[u] = in ? mm % P : -1;
            o[u] = own[b]; p[u] = opp[b];
            d[u] = dz[(size_t)mm * C + co];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (pixs[u] < 0) continue;
            const int y0 = pixs[u] / n, x0 = pixs[u] % n;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int y = y0 + t / 3 - 1, x = x0 + t % 3 - 1;
                if (y < 0 || y >= n || x < 0 || x >= n) continue;
                const int sq = y * 8 + x;
                const float a = (float)((o[u] >> sq) & 1), bb = (float)((p[u] >> sq) & 1);
                if (cin == 2) { acc[2 * t] = fmaf(a, d[u], acc[2 * t]); acc[2 * t + 1] = fmaf(bb, d[u], acc[2 * t + 1]); }
                else acc[t] = fmaf(a - bb, d[u], acc[t]);
            }
        }
    }
    for (int tc = 0; tc < 9 * cin; ++tc) partial[((size_t)sp * 9 * cin + tc) * C + co] = acc[tc];
}

// out[i] = sum_s partial[s][i] in fixed order
__global__ void k_t_sum_partials(const float* __restrict__ partial, int S, long long count, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float a = 0.f;
    _Pragma("unroll 8") for (int s = 0; s < S; ++s) a += partial[(size_t)s * count + i];     // the loads are independent: 8 in flight, the adds stay in order
    out[i] = a;
}

// ---------------------------------------------------------------- column reductions over the rows of [M][C] matrices
// MODE 0: sum x            MODE 1: sum (x - mean)^2
// MODE 2: BN backward sums: dy = (a > 0 ? dA * post_scale : 0); s0 = sum dy, s1 = sum dy * xhat, xhat = (z - mean) * rstd
struct RedArgs {
    const float *x, *a, *z, *mean, *rstd;
    float post_scale;
    int P, C;
};
// Streaming form: a thread owns 4 consecutive channels (16-byte loads), the lanes of a row cover up to 256 channels
// (1 KB per wave instruction), the 256 threads of a block cover 4 rows (8 at 128 channels) per pass, rows strided RED_S
// passes apart; the row groups of a block are combined through LDS in fixed order.
template <int MODE>
__global__ __launch_bounds__(256) void k_t_colreduce(RedArgs r, const int* __restrict__ d_count, float* __restrict__ partial /*[RED_S][2][C]*/) {
    const int Q = r.C / 4;                                   // float4 columns
    const int lpr = Q < 64 ? Q : 64, rpp = 256 / lpr;        // lanes per row, rows per pass
    const int q = blockIdx.x * 64 + (int)(threadIdx.x % lpr), rsub = threadIdx.x / lpr, sp = blockIdx.y;
    const bool valid = q < Q;                                // (channel counts that are not a multiple of 256: the last block is partly idle)
    const int c = valid ? q * 4 : 0;
    const long long M = valid ? (long long)(*d_count) * r.P : 0;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    f32x4 mu = s0, rs = s0;
    if (MODE == 1 || MODE == 2) mu = *reinterpret_cast<const f32x4*>(r.mean + c);
    if (MODE == 2) rs = *reinterpret_cast<const f32x4*>(r.rstd + c);
    for (long long m = (long long)sp * rpp + rsub; m < M; m += (long long)gridDim.y * rpp) {      // gridDim.y row splits (RED_S for the streaming passes)
        const size_t o = (size_t)m * r.C + c;
        if (MODE == 0) s0 += *reinterpret_cast<const f32x4*>(r.x + o);
        if (MODE == 1) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(r.x + o) - mu;
#pragma unroll
            for (int k = 0; k < 4; ++k) s0[k] = fmaf(d[k], d[k], s0[k]);
        }
        if (MODE == 2) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(r.a + o), xv = *reinterpret_cast<const f32x4*>(r.x + o),
                        zv = *reinterpret_cast<const f32x4*>(r.z + o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dy = av[k] > 0.f ? xv[k] * r.post_scale : 0.f;
                s0[k] += dy;
                s1[k] = fmaf(dy, (zv[k] - mu[k]) * rs[k], s1[k]);
            }
        }
    }
    __shared__ f32x4 sh[2][256];
    sh[0][threadIdx.x] = s0;
    sh[1][threadIdx.x] = s1;
    __syncthreads();
    if (rsub == 0 && valid) {
        f32x4 a0 = sh[0][threadIdx.x], a1 = sh[1][threadIdx.x];
        for (int k = 1; k < rpp; ++k) { a0 += sh[0][threadIdx.x + k * lpr]; a1 += sh[1][threadIdx.x + k * lpr]; }
        *reinterpret_cast<f32x4*>(partial + ((size_t)sp * 2 + 0) * r.C + c) = a0;
        *reinterpret_cast<f32x4*>(partial + ((size_t)sp * 2 + 1) * r.C + c) = a1;
    }
}
__device__ __forceinline__ float t_sum_s(const float* partial, int which, int C, int c) {
    float a = 0.f;
    for (int s = 0; s < RED_S; ++s) a += partial[((size_t)s * 2 + which) * C + c];
    return a;
}
// mean[c] = sum / M
__global__ void k_t_fin_mean(const float* __restrict__ partial, const int* __restrict__ d_count, int P, int C, float* __restrict__ mean) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) mean[c] = t_sum_s(partial, 0, C, c) / (float)((long long)(*d_count) * P);
}
// rstd[c] = 1/sqrt(var + eps); staged moving statistics: new = old * mom + batch * (1 - mom) (var unbiased when fused)
__global__ void k_t_fin_var(const float* __restrict__ partial, const int* __restrict__ d_count, int P, int C, const float* __restrict__ mean,
                            float* __restrict__ rstd, const float* __restrict__ mm, const float* __restrict__ mv,
                            float* __restrict__ mm_new, float* __restrict__ mv_new, float mom, int fused) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long long M = (long long)(*d_count) * P;
    const float var = t_sum_s(partial, 0, C, c) / (float)M;
    rstd[c] = 1.0f / sqrtf(var + BN_EPS);
    const float uv = fused ? var * ((float)M / (float)(M > 1 ? M - 1 : 1)) : var;
    mm_new[c] = mm[c] * mom + mean[c] * (1.0f - mom);
    mv_new[c] = mv[c] * mom + uv * (1.0f - mom);
}
// a = relu((z - mean) * rstd * gamma + beta) [* keep / (1 - rate)]; 4 consecutive channels per thread
__global__ __launch_bounds__(256) void k_t_bn_fwd(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ a,
                                                  const int* __restrict__ d_count, int P, int C, float rate, uint64_t seed, uint64_t step, int dlayer) {
    const long long total = (long long)(*d_count) * P * C;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= total) return;
    const int c = (int)(i % C);
    const f32x4 zv = *reinterpret_cast<const f32x4*>(z + i), mu = *reinterpret_cast<const f32x4*>(mean + c),
                rs = *reinterpret_cast<const f32x4*>(rstd + c), ga = *reinterpret_cast<const f32x4*>(gamma + c),
                be = *reinterpret_cast<const f32x4*>(beta + c);
    f32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float y = (zv[k] - mu[k]) * rs[k] * ga[k] + be[k];
        y = y > 0.f ? y : 0.f;
        if (rate > 0.f) y = oz_dropout_keep(seed, step, (uint64_t)dlayer, (uint64_t)(i + k), rate) ? y / (1.0f - rate) : 0.f;
        out[k] = y;
    }
    *reinterpret_cast<f32x4*>(a + i) = out;
}
// inference mode (held-out evaluation): a = relu((z - moving_mean) * (1 / sqrtf(moving_var + eps)) * gamma + beta); 4 consecutive channels per
// thread.  Writes nothing but `a`: no batch statistics, no staged moving statistics, no dropout
__global__ __launch_bounds__(256) void k_t_bn_infer(const float* __restrict__ z, const float* __restrict__ mm, const float* __restrict__ mv,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ a,
                                                    const int* __restrict__ d_count, int P, int C) {
    const long long total = (long long)(*d_count) * P * C;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= total) return;
    const int c = (int)(i % C);
    const f32x4 zv = *reinterpret_cast<const f32x4*>(z + i), mu = *reinterpret_cast<const f32x4*>(mm + c),
                va = *reinterpret_cast<const f32x4*>(mv + c), ga = *reinterpret_cast<const f32x4*>(gamma + c),
                be = *reinterpret_cast<const f32x4*>(beta + c);
    f32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float y = (zv[k] - mu[k]) * (1.0f / sqrtf(va[k] + BN_EPS)) * ga[k] + be[k];
        out[k] = y > 0.f ? y : 0.f;
    }
    *reinterpret_cast<f32x4*>(a + i) = out;
}
// ---------------------------------------------------------------- heads: forward, losses, gradient wrt f2
// The two matvecs of a head pair on one sample's f2 row x[512], one 64-lane wave per sample; k_t_heads, k_t_eval_heads and k_t_aux_heads all
// run these bodies, so their sums have one order.
// t_head_cols: lane a's column of W[512][A], sum_k x[k] W[k][a] (lanes >= A read column 0; the caller adds the bias and drops them).
// 64 weight rows in flight per batch (buffer loads: one per-lane offset register + a scalar row offset each), the fmaf chain stays in k order:
// the loop is a chain of L2 round trips, 32 of them with 16 rows in flight = 19 us per launch at the reference's batch (round 5)
__device__ __forceinline__ float t_head_cols(const float* __restrict__ x, const float* __restrict__ W, int A, int lane) {
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, 512 * A * 4, 0x00020000);
    const int lo = (lane < A ? lane : 0) * 4;
    float acc = 0.f;
#pragma unroll 1
    for (int k0 = 0; k0 < 512; k0 += 64) {
        float wv[64];
#pragma unroll
        for (int j = 0; j < 64; ++j) wv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrs, lo, (k0 + j) * A * 4, 0));
#pragma unroll
        for (int j = 0; j < 64; ++j) acc = fmaf(x[k0 + j], wv[j], acc);
    }
    return acc;
}
// t_head_dot: x . w[512] for the scalar head, every lane a strided fmaf chain, then the xor-shuffle tree (every lane holds the sum)
__device__ __forceinline__ float t_head_dot(const float* __restrict__ x, const float* __restrict__ w, int lane) {
    float acc = 0.f;
    for (int k = lane; k < 512; k += 64) acc = fmaf(x[k], w[k], acc);
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    return acc;
}
// The policy loss of one sample from its logits (lane = action, -inf on lanes >= A): softmax p, the renormalised q = p / S, the clipped cross
// entropy summed over the lanes.  k_t_heads adds the gradient, k_t_eval_heads the arg-max metrics.
// flat = 0 (OZ_POLICY_LOSS_ROWS): the reference's loss on the (n, n) view, every row renormalised and the rows averaged;
// flat = 1 (OZ_POLICY_LOSS_FLAT): the same clipped cross entropy with ONE group of A lanes -- whole-board sums, no mean over rows
struct TPolicyLoss { float p, t, S, q, lpi; int row, width; };     // lpi: the sum over the lanes (ROWS: the caller divides by n)
__device__ __forceinline__ TPolicyLoss t_policy_loss(float logit, const float* __restrict__ pit_b /*[A]*/, int n, int A, int flat, int lane) {
    TPolicyLoss r;
    float mx = logit;
    for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float e = lane < A ? expf(logit - mx) : 0.f;
    float se = e;
    for (int o = 32; o; o >>= 1) se += __shfl_xor(se, o);
    r.p = e / se;
    // row-normalised, clipped cross entropy on the (n, n) view; the lanes of one board row are n consecutive lanes
    // (every lane runs the shuffles; lanes >= A read a clamped source and their results are unused).  flat: one group of A lanes
    r.row = flat ? 0 : lane / n; r.width = flat ? A : n;
    r.t = lane < A ? pit_b[lane] : 0.f;
    r.S = 0.f;
    for (int c = 0; c < r.width; ++c) { const int src = r.row * n + c; r.S += __shfl(r.p, src < 63 ? src : 63); }
    r.q = lane < A ? r.p / r.S : 0.5f;
    const float qc = fminf(fmaxf(r.q, 1e-7f), 1.0f - 1e-7f);
    r.lpi = lane < A ? -r.t * logf(qc) : 0.f;
    for (int o = 32; o; o >>= 1) r.lpi += __shfl_xor(r.lpi, o);
    return r;
}
// one 64-thread block per sample (A = n*n <= 64 policy outputs, lane = action)
__global__ __launch_bounds__(64) void k_t_heads(const float* __restrict__ f2 /*[B][512]*/, const int* __restrict__ d_count, int n, int flat,
                                                const float* __restrict__ Wpi /*[512][A]*/, const float* __restrict__ bpi,
                                                const float* __restrict__ Wv /*[512]*/, const float* __restrict__ bv,
                                                const float* __restrict__ pit /*[B][A]*/, const float* __restrict__ zt /*[B]*/,
                                                float* __restrict__ p_out, float* __restrict__ v_out,
                                                float* __restrict__ dlogit /*[B][A]*/, float* __restrict__ dvpre /*[B]*/,
                                                float* __restrict__ loss /*[B][2]*/) {
    const int b = blockIdx.x, lane = threadIdx.x, A = n * n, B = *d_count;
    if (b >= B) return;
    const float* x = f2 + (size_t)b * 512;
    const float acc = t_head_cols(x, Wpi, A, lane);
    const float logit = lane < A ? acc + bpi[lane] : -INFINITY;
    const float vacc = t_head_dot(x, Wv, lane);
    const TPolicyLoss pl = t_policy_loss(logit, pit + (size_t)b * A, n, A, flat, lane);
    const float p = pl.p, t = pl.t, S = pl.S, q = pl.q, lpi = pl.lpi;
    const float v = tanhf(vacc + bv[0]);
    // dL/dq = -t/q inside the clip range (0 outside); q = p / S  =>  dL/dp_j = g_j / S - (sum_{c in row} g_c q_c) / S
    const bool inside = q >= 1e-7f && q <= 1.0f - 1e-7f;
    const float gq = (lane < A && inside) ? -t / q : 0.f;
    const float gqq = gq * q;
    float rowdot = 0.f;
    for (int c = 0; c < pl.width; ++c) { const int src = pl.row * n + c; rowdot += __shfl(gqq, src < 63 ? src : 63); }
    const float normp = flat ? 1.0f / (float)B : 1.0f / ((float)B * (float)n);
    const float gp = lane < A ? (gq - rowdot) / S * normp : 0.f;
    // softmax backward: dlogit_j = p_j (gp_j - sum_k gp_k p_k)
    float dot = gp * p;
    for (int o = 32; o; o >>= 1) dot += __shfl_xor(dot, o);
    if (lane < A) {
        dlogit[(size_t)b * A + lane] = p * (gp - dot);
        p_out[(size_t)b * A + lane] = p;
    }
    if (lane == 0) {
        const float d = v - zt[b];
        v_out[b] = v;
        dvpre[b] = 2.0f * d / (float)B * (1.0f - v * v);
        loss[2 * b] = flat ? lpi : lpi / (float)n;          // per-sample mean over rows (ROWS)
        loss[2 * b + 1] = d * d;
    }
}
// ---------------------------------------------------------------- held-out evaluation: heads without gradients, per-example metrics
// k_t_heads' forward (t_head_cols, t_head_dot and t_policy_loss as there, flat as there) with no gradient stores; per example one row of
// OZ_EVAL_ROW floats: [0] the policy loss of the mode, [1] (v - z)^2, [2] arg-max of p == arg-max of the target (lowest index among equal
// maxima on both sides), [3] v z > 0, [4] z != 0
#define OZ_EVAL_ROW 5
__device__ __forceinline__ int t_argmax_lowest(float val, int lane) {      // wave reduction on (value, index): the larger value, the lower index on a tie
    int idx = lane;
    for (int o = 32; o; o >>= 1) {
        const float ov = __shfl_xor(val, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
    return idx;
}
__global__ __launch_bounds__(64) void k_t_eval_heads(const float* __restrict__ f2 /*[B][512]*/, const int* __restrict__ d_count, int n, int flat,
                                                     const float* __restrict__ Wpi /*[512][A]*/, const float* __restrict__ bpi,
                                                     const float* __restrict__ Wv /*[512]*/, const float* __restrict__ bv,
                                                     const float* __restrict__ pit /*[B][A]*/, const float* __restrict__ zt /*[B]*/,
                                                     float* __restrict__ p_out, float* __restrict__ v_out, float* __restrict__ rows /*[B][OZ_EVAL_ROW]*/) {
    const int b = blockIdx.x, lane = threadIdx.x, A = n * n, B = *d_count;
    if (b >= B) return;
    const float* x = f2 + (size_t)b * 512;
    const float acc = t_head_cols(x, Wpi, A, lane);
    const float logit = lane < A ? acc + bpi[lane] : -INFINITY;
    const float vacc = t_head_dot(x, Wv, lane);
    const TPolicyLoss pl = t_policy_loss(logit, pit + (size_t)b * A, n, A, flat, lane);
    const float p = pl.p, t = pl.t, lpi = pl.lpi;
    const float v = tanhf(vacc + bv[0]);
    const int ap = t_argmax_lowest(lane < A ? p : -INFINITY, lane), at = t_argmax_lowest(lane < A ? t : -INFINITY, lane);      // idle lanes never win
    if (lane < A) p_out[(size_t)b * A + lane] = p;
    if (lane == 0) {
        const float z = zt[b], d = v - z;
        v_out[b] = v;
        float* r = rows + (size_t)b * OZ_EVAL_ROW;
        r[0] = flat ? lpi : lpi / (float)n;
        r[1] = d * d;
        r[2] = ap == at ? 1.f : 0.f;
        r[3] = v * z > 0.f ? 1.f : 0.f;
        r[4] = z != 0.f ? 1.f : 0.f;
    }
}
// one block adds the B rows of a batch into the accumulator: thread i sums rows i, i + 256, ... in example order, then a fixed tree over the 256
// partial sums -- the order depends on nothing but B (no atomics)
struct TEvalAcc { double sum[2]; long long cnt[3]; long long examples; };
__global__ __launch_bounds__(256) void k_t_acc_eval(const float* __restrict__ rows, int B, TEvalAcc* __restrict__ acc) {
    __shared__ double sd[2][256];
    __shared__ int sc[3][256];
    const int i = threadIdx.x;
    double d0 = 0.0, d1 = 0.0;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int b = i; b < B; b += 256) {
        const float* r = rows + (size_t)b * OZ_EVAL_ROW;
        d0 += (double)r[0]; d1 += (double)r[1];
        c0 += r[2] != 0.f; c1 += r[3] != 0.f; c2 += r[4] != 0.f;
    }
    sd[0][i] = d0; sd[1][i] = d1; sc[0][i] = c0; sc[1][i] = c1; sc[2][i] = c2;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if (i < o) {
            sd[0][i] += sd[0][i + o]; sd[1][i] += sd[1][i + o];
            sc[0][i] += sc[0][i + o]; sc[1][i] += sc[1][i + o]; sc[2][i] += sc[2][i + o];
        }
        __syncthreads();
    }
    if (i == 0) {
        acc->sum[0] += sd[0][0]; acc->sum[1] += sd[1][0];
        acc->cnt[0] += sc[0][0]; acc->cnt[1] += sc[1][0]; acc->cnt[2] += sc[2][0];
        acc->examples += B;
    }
}
// The three backward kernels of a head pair (t_head_pair_backward): the policy / value heads and, with the auxiliary heads on, theirs
// (dopre, dspre, Wown, Wsc in the places of dlogit, dvpre, Wpi, Wv).
// dWpi[k][a] = sum_b f2[b][k] dlogit[b][a];  dWv[k] = sum_b f2[b][k] dvpre[b]   (block = k, thread = a; a == A handles v)
__global__ __launch_bounds__(128) void k_t_heads_wgrad(const float* __restrict__ f2, const float* __restrict__ dlogit, const float* __restrict__ dvpre,
                                                       const int* __restrict__ d_count, int A, float* __restrict__ dWpi, float* __restrict__ dWv) {
    const int k = blockIdx.x, a = threadIdx.x, B = *d_count;
    if (a > A) return;
    float acc = 0.f;
    _Pragma("unroll 8") for (int b = 0; b < B; ++b) acc = fmaf(f2[(size_t)b * 512 + k], a < A ? dlogit[(size_t)b * A + a] : dvpre[b], acc);    // 8 loads in flight, sums in batch order
    if (a < A) dWpi[(size_t)k * A + a] = acc; else dWv[k] = acc;
}
// dbpi[a] = sum_b dlogit[b][a]; dbv = sum_b dvpre[b]; sums in batch order.  loss (nullable, with losses: the auxiliary pair has k_t_aux_losses):
// losses[0..2] = total, pi, v (batch means)
__global__ __launch_bounds__(128) void k_t_heads_bias(const float* __restrict__ dlogit, const float* __restrict__ dvpre, const float* __restrict__ loss,
                                                      const int* __restrict__ d_count, int A, float* __restrict__ dbpi, float* __restrict__ dbv,
                                                      float* __restrict__ losses, unsigned* __restrict__ zero6 /* nullable: six words cleared here */) {
    const int a = threadIdx.x, B = *d_count;
    if (zero6 && a >= 120 && a < 126) zero6[a - 120] = 0u;   // the per-layer |dz| maxima of the f16x2 mode (a 24-byte memset was two fill launches on the chain)
    if (a < A) { float s = 0.f; _Pragma("unroll 8") for (int b = 0; b < B; ++b) s += dlogit[(size_t)b * A + a]; dbpi[a] = s; }
    if (a == A) { float s = 0.f; _Pragma("unroll 8") for (int b = 0; b < B; ++b) s += dvpre[b]; dbv[0] = s; }
    if (loss && a == A + 1) {
        float lp = 0.f, lv = 0.f;
        _Pragma("unroll 8") for (int b = 0; b < B; ++b) { lp += loss[2 * b]; lv += loss[2 * b + 1]; }
        lp /= (float)B; lv /= (float)B;
        losses[0] = lp + lv; losses[1] = lp; losses[2] = lv;
    }
}
// df2[b][k] = sum_a dlogit[b][a] Wpi[k][a] + dvpre[b] Wv[k]; add (the auxiliary pair, behind the first launch): the same sum, then df2 += it.
// One launch per pair: a single sum over both pairs would round differently and could not leave df2's bits alone with both weights 0
__global__ __launch_bounds__(256) void k_t_heads_dgrad(const float* __restrict__ dlogit, const float* __restrict__ dvpre, const float* __restrict__ Wpi,
                                                       const float* __restrict__ Wv, const int* __restrict__ d_count, int A, int add, float* __restrict__ df2) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)(*d_count) * 512) return;
    const int b = (int)(i / 512), k = (int)(i % 512);
    float acc = dvpre[b] * Wv[k];
    for (int a = 0; a < A; ++a) acc = fmaf(dlogit[(size_t)b * A + a], Wpi[(size_t)k * A + a], acc);
    df2[i] = add ? df2[i] + acc : acc;
}

// ---------------------------------------------------------------- auxiliary heads (oz_trainer_set_aux_heads): ownership and score from the final boards
// Two more heads on f2, trained and then thrown away: o[a] = tanh(f2 . Wown[:, a] + bown[a]) against who owns square a at the end of the game
// (+1 mover / -1 opponent / 0 empty), s = tanh(f2 . Wsc + bsc) against the final disc margin / A, both from the mover's side (oz_aux_target,
// oz_common.h).  m = (fin_own | fin_opp) != 0 masks an example without a final board; the batch means divide by B as the value loss does:
//   L_own = (1/B) sum_b m_b (1/A) sum_a (o - t)^2        L_sc = (1/B) sum_b m_b (s - s_target)^2
// fp32 in every trainer precision.  The loss weights are folded into the pre-activation gradients, so the three backward kernels know nothing of
// them; with both weights 0 the backward kernels are not launched at all (forward and losses only: the 40 gradients keep their bits).
// k_t_aux_heads: one 64-thread block per sample, lane = cell a = row*n+col, k_t_heads' matvecs (t_head_cols, t_head_dot).  Every sum over
// lanes is the xor-shuffle tree: a fixed order
__global__ __launch_bounds__(64) void k_t_aux_heads(const float* __restrict__ f2 /*[B][512]*/, const int* __restrict__ d_count, int n,
                                                    const float* __restrict__ Wown /*[512][A]*/, const float* __restrict__ bown,
                                                    const float* __restrict__ Wsc /*[512]*/, const float* __restrict__ bsc,
                                                    const uint64_t* __restrict__ fin_own, const uint64_t* __restrict__ fin_opp, float w_own, float w_sc,
                                                    float* __restrict__ o_out /*[B][A]*/, float* __restrict__ s_out /*[B]*/,
                                                    float* __restrict__ dopre /*[B][A]*/, float* __restrict__ dspre /*[B]*/,
                                                    float* __restrict__ loss /*[B][2]*/) {
    const int b = blockIdx.x, lane = threadIdx.x, A = n * n, B = *d_count;
    if (b >= B) return;
    const float* x = f2 + (size_t)b * 512;
    const float acc = t_head_cols(x, Wown, A, lane);
    const float opre = lane < A ? acc + bown[lane] : 0.f;
    const float sacc = t_head_dot(x, Wsc, lane);
    const uint64_t fo = fin_own[b], fp = fin_opp[b];
    const bool live = (fo | fp) != 0;
    const float o = tanhf(opre), s = tanhf(sacc + bsc[0]);
    const float d = lane < A ? o - oz_aux_own_target(fo, fp, (lane / n) * 8 + lane % n) : 0.f;
    float lo_ = d * d;
    for (int off = 32; off; off >>= 1) lo_ += __shfl_xor(lo_, off);
    if (lane < A) {
        o_out[(size_t)b * A + lane] = o;
        dopre[(size_t)b * A + lane] = live ? w_own * (2.0f * d / ((float)B * (float)A)) * (1.0f - o * o) : 0.f;
    }
    if (lane == 0) {
        const float ds = s - oz_aux_score_target(fo, fp, A);
        s_out[b] = s;
        dspre[b] = live ? w_sc * (2.0f * ds / (float)B) * (1.0f - s * s) : 0.f;
        loss[2 * b] = live ? lo_ / (float)A : 0.f;
        loss[2 * b + 1] = live ? ds * ds : 0.f;
    }
}
// aux[0..1] = L_own, L_sc (batch means, sums in batch order); with a weight on, losses[0] (k_t_heads_bias' total) gains w_own L_own + w_sc L_sc.
// A kernel of its own, not a part of k_t_heads_bias' second launch: it runs with both weights 0 too, when the pair's backward is not launched,
// and it adds into losses[0] only after the first k_t_heads_bias has written it
__global__ __launch_bounds__(64) void k_t_aux_losses(const float* __restrict__ loss, const int* __restrict__ d_count, float w_own, float w_sc,
                                                     float* __restrict__ aux /*[2]*/, float* __restrict__ losses) {
    if (threadIdx.x != 0) return;
    const int B = *d_count;
    float lo = 0.f, ls = 0.f;
    _Pragma("unroll 8") for (int b = 0; b < B; ++b) { lo += loss[2 * b]; ls += loss[2 * b + 1]; }
    lo /= (float)B; ls /= (float)B;
    aux[0] = lo; aux[1] = ls;
    if (w_own > 0.f || w_sc > 0.f) losses[0] = losses[0] + (w_own * lo + w_sc * ls);
}
// (the pair's weight, bias and f2 gradients are a second launch each of k_t_heads_wgrad, k_t_heads_bias and k_t_heads_dgrad)

// ---------------------------------------------------------------- weight gradient: TN implicit GEMM on fp32 MFMA
// dW[t][ci][co] = sum_m Xs_t[m][ci] * dZ[m][co], m = (b, oy, ox).  Block tile 128 ci x 128 co for one tap, 4 waves of
// 64x64 (2x2 v_mfma_f32_32x32x2_f32); the k index is the row m: both operand tiles are staged [32 rows][128 channels]
// straight from their row-major tensors (coalesced, no transpose) and the MFMA operands are read k-major from LDS
// (lane (i, kk) reads element [k0 + kk][i]: 32 consecutive floats per half wave, row stride padded by 32 banks).
#define WG_STRIDE 160
struct WgradGeom { int Hin, Hout, pad, Cin, Cout, taps, Hz, zoff; };
__global__ __launch_bounds__(256) void k_wgrad_f32(const float* __restrict__ X, const float* __restrict__ dZ, const int* __restrict__ d_count,
                                                   WgradGeom g, float* __restrict__ dW, int msplit, float* __restrict__ partial, long long slab) {
    __shared__ __attribute__((aligned(16))) float lds[2][32 * WG_STRIDE];
    const int nci = g.Cin / 128, nco = g.Cout / 128;
    const int tap = blockIdx.x / (nci * nco), rem = blockIdx.x % (nci * nco), ci0 = (rem / nco) * 128, co0 = (rem % nco) * 128;
    const int P = g.Hout * g.Hout;
    const long long M = (long long)(*d_count) * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int srow = tid >> 5, c4 = (tid & 31) * 4;              // staging: rows srow + 8 i, 4 consecutive channels
    const int dy = g.taps == 9 ? tap / 3 : 0, dx = g.taps == 9 ? tap % 3 : 0;

    f32x4 ra[4], rb[4];
    auto gload = [&](long long m0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long m = m0 + srow + 8 * i;
            f32x4 za = {0.f, 0.f, 0.f, 0.f}, zb = za;
            if (m < M) {
                const int b = (int)(m / P), pix = (int)(m % P), oy = pix / g.Hout, ox = pix % g.Hout;
                const int iy = oy - g.pad + dy, ix = ox - g.pad + dx;
                if (iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Hin)
                    za = *reinterpret_cast<const f32x4*>(X + (((size_t)b * g.Hin + iy) * g.Hin + ix) * g.Cin + ci0 + c4);
                zb = *reinterpret_cast<const f32x4*>(dZ + (((size_t)b * g.Hz + oy + g.zoff) * g.Hz + ox + g.zoff) * g.Cout + co0 + c4);
            }
            ra[i] = za; rb[i] = zb;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(&lds[0][(srow + 8 * i) * WG_STRIDE + c4]) = ra[i];
            *reinterpret_cast<f32x4*>(&lds[1][(srow + 8 * i) * WG_STRIDE + c4]) = rb[i];
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int r32 = lane & 31, kk = lane >> 5;
    // rows (the k index) split over blockIdx.y when the launch is small: partial sums to partial[split], reduced in fixed order
    const long long nk_all = (M + 31) / 32, nk_s = (nk_all + msplit - 1) / msplit, kt0 = blockIdx.y * nk_s;
    const long long nk = nk_all < kt0 + nk_s ? nk_all : kt0 + nk_s;
    float* __restrict__ outp = msplit > 1 ? partial + (size_t)blockIdx.y * slab : dW;
    if (kt0 < nk) { gload(kt0 * 32); lstore(); }
    __syncthreads();
    for (long long kt = kt0; kt < nk; ++kt) {
        if (kt + 1 < nk) gload((kt + 1) * 32);
        const float* At = &lds[0][kk * WG_STRIDE + wm * 64 + r32];
        const float* Bt = &lds[1][kk * WG_STRIDE + wn * 64 + r32];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float a0 = At[2 * s * WG_STRIDE], a1 = At[2 * s * WG_STRIDE + 32];
            const float b0 = Bt[2 * s * WG_STRIDE], b1 = Bt[2 * s * WG_STRIDE + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if (kt + 1 < nk) lstore();
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31 (co), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (ci)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                const int co = co0 + wn * 64 + j * 32 + r32;
                outp[((size_t)tap * g.Cin + ci) * g.Cout + co] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------- weight gradient of a 3x3 convolution, board-resident
// dW[tap][ci][co] = sum over boards b and output pixels p of X[b][p + tap][ci] * dZ[b][p][co].
// k_wgrad_f32 above (kept for the dense layers) gives every (tap, 128 ci, 128 co) tile its own block, so the two operand
// matrices stream through 9 x 4 x 4 blocks: 32 FLOP per byte staged, the launch is bound by the memory system (measured
// 30-49 TFLOP/s at batch 1024).  Here a block owns a 64 (ci) x 128 (co) tile for ALL NINE taps: one board's X tile (with its
// zero border for 'same' layers) and dZ tile are staged in LDS once and every tap reads the SAME staged pixels at a shifted
// address -- 9 accumulators per wave (one 32 x 32 MFMA tile per tap = 144 registers), 190 FLOP per byte staged, one barrier
// per board, next board prefetched into registers during the 288 MFMAs of the current one.  The k index of
// v_mfma_f32_32x32x2_f32 is the output pixel: k-steps of two pixels (Hout^2 is even for every layer of either board size).
#define WC_CI 64
#define WC_CO 128
struct WconvGeom { int Hin, Hout, pad, Cin, Cout, Hz, zoff; };
__global__ __launch_bounds__(512) void k_wgrad_conv(const float* __restrict__ X, const float* __restrict__ dZ, const int* __restrict__ d_count,
                                                    WconvGeom g, float* __restrict__ dW, int msplit, float* __restrict__ partial, long long slab) {
    extern __shared__ __attribute__((aligned(16))) float wc_lds[];
    const int XW = g.Hin + 2 * g.pad, XP = XW * XW, P = g.Hout * g.Hout;
    const int stage_floats = XP * WC_CI + P * WC_CO;
    const int nco = g.Cout / WC_CO;
    const int ci0 = (blockIdx.x / nco) * WC_CI, co0 = (blockIdx.x % nco) * WC_CO;
    const int B = *d_count;
    const int per = (B + msplit - 1) / msplit, b0 = blockIdx.y * per, b1 = b0 + per < B ? b0 + per : B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 2, wn = wave & 3, r32 = lane & 31, kk = lane >> 5;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // staging: float4 units; X tile = XP pixels x 16 units (border pixels are zeros), dZ tile = P pixels x 32 units
    const int xu = XP * (WC_CI / 4), zu = P * (WC_CO / 4);
    f32x4 rx[4], rz[4];
    auto gload = [&](int b) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + 512 * i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (u < xu) {
                const int px = u >> 4, c4 = (u & 15) * 4, iy = px / XW - g.pad, ix = px % XW - g.pad;
                if (iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Hin)
                    v = *reinterpret_cast<const f32x4*>(X + (((size_t)b * g.Hin + iy) * g.Hin + ix) * g.Cin + ci0 + c4);
            }
            rx[i] = v;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            if (u < zu) {
                const int px = u >> 5, c4 = (u & 31) * 4, oy = px / g.Hout, ox = px % g.Hout;
                z = *reinterpret_cast<const f32x4*>(dZ + (((size_t)b * g.Hz + oy + g.zoff) * g.Hz + ox + g.zoff) * g.Cout + co0 + c4);
            }
            rz[i] = z;
        }
    };
    auto lstore = [&](int st) {
        float* Xs = wc_lds + st * stage_floats;
        float* Zs = Xs + XP * WC_CI;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + 512 * i;
            if (u < xu) *reinterpret_cast<f32x4*>(Xs + u * 4) = rx[i];
            if (u < zu) *reinterpret_cast<f32x4*>(Zs + u * 4) = rz[i];
        }
    };
    if (b0 < b1) { gload(b0); lstore(0); }
    __syncthreads();
    for (int b = b0; b < b1; ++b) {
        const int st = (b - b0) & 1;
        if (b + 1 < b1) gload(b + 1);
        const float* Xs = wc_lds + st * stage_floats + wm * 32 + r32;
        const float* Zs = wc_lds + st * stage_floats + XP * WC_CI + wn * 32 + r32;
        for (int s2 = 0; s2 < P / 2; ++s2) {
            const int p = 2 * s2 + kk, oy = p / g.Hout, ox = p - oy * g.Hout;
            const float zb = Zs[p * WC_CO];
            const float* xa = Xs + (oy * XW + ox) * WC_CI;
#pragma unroll
            for (int t = 0; t < 9; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[((t / 3) * XW + (t % 3)) * WC_CI], zb, acc[t], 0, 0, 0);
        }
        if (b + 1 < b1) lstore(st ^ 1);             // the other stage was last read before the previous barrier
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31 (co), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (ci)
    float* __restrict__ outp = msplit > 1 ? partial + (size_t)blockIdx.y * slab : dW;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
            const int co = co0 + wn * 32 + r32;
            outp[((size_t)t * g.Cin + ci) * g.Cout + co] = acc[t][r];
        }
}

// ---------------------------------------------------------------- operand layouts derived from the Keras-layout masters
// out[c][r] = in[r][c]   (forward operand Wt[N][K] of k_gemm_f32 from the Keras kernel [K][N])
__global__ __launch_bounds__(256) void k_t_transpose(const float* __restrict__ in, int R, int Cc, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) if (by + i < R && bx + tx < Cc) tile[i][tx] = in[(size_t)(by + i) * Cc + bx + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8) if (bx + i < Cc && by + tx < R) out[(size_t)(bx + i) * R + by + tx] = tile[tx][i];
}
// data-gradient operand of a 3x3 convolution: Wd[ci][(8 - t) * Cout + co] = W[t][ci][co]
__global__ __launch_bounds__(256) void k_t_dgrad_operand(const float* __restrict__ W, int Cin, int Cout, float* __restrict__ Wd) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9LL * Cin * Cout) return;
    const int co = (int)(i % Cout), ci = (int)((i / Cout) % Cin), t = (int)(i / ((long long)Cout * Cin));
    Wd[(size_t)ci * 9 * Cout + (size_t)(8 - t) * Cout + co] = W[i];
}

// ---------------------------------------------------------------- f16x2 mode of the 3x3 layers (forward and data gradient on k_gemm_h2)
// An fp32 value travels as two fp16 planes (oz_net_h2.h: 22 significand bits, 3 fp16 MFMA products per fp32 product at 16x the fp32
// matrix rate).  fp16 has 5 exponent bits, so every tensor is moved into range by an exact power of two taken from its own
// maximum, on the device and per step: weights to max |w| ~ 2^9 (as at oz_net_commit), data gradients to max |dz| ~ 2^13; the
// inverse powers ride in the GEMM's per-column scale, so scaling itself changes no bit.  Small elements of a gradient tensor
// (below 2^-11 of its maximum) lose relative precision in the second plane -- an absolute error of 2^-37 of the tensor's
// maximum, far below the fp32 rounding of the sums they enter.  Activations are post-ReLU values < 65504 (sticky flag otherwise).
// Where in the fp16 window the per-step scales put a tensor's maximum: 2^9 .. 2^10 for the weights, 2^13 for the data gradients.  The inference path
// moved its maxima to 2^-2 in round 4 (fewer residual bits for small elements = a higher sustained clock, tools/target_probe.py); that is NOT copied here:
// these scales are per TENSOR, and a gradient tensor's elements lie many binary orders below its maximum -- at a maximum of 2^-2 an element 2^-10 of it
// would keep 13 bits, at 2^13 it keeps all 22.
#define T_W_TARGET 1000.0f
#define T_DZ_TARGET 8192.0f
struct AbsMaxArgs { const float* p[3]; long long n[3]; };
// out[l] = bits of max |p[l][i]| (non-negative floats order like their bit patterns); out is zeroed by the caller
__global__ __launch_bounds__(256) void k_t_absmax(AbsMaxArgs a, unsigned* __restrict__ out) {
    const int l = blockIdx.y;
    const float* p = a.p[l];
    float m = 0.f;
    // twelve 16-byte loads in flight per trip (the one-load-per-trip loop took 40 us for 28 MB at the reference's batch, round 5)
    const long long stride = (long long)gridDim.x * 1024;
    for (long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i0 < a.n[l]; i0 += 12 * stride) {
        f32x4 v[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) { const long long i = i0 + q * stride; v[q] = i < a.n[l] ? *reinterpret_cast<const f32x4*>(p + i) : f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            m = fmaxf(fmaxf(fabsf(v[q][0]), fabsf(v[q][1])), fmaxf(m, fmaxf(fabsf(v[q][2]), fabsf(v[q][3]))));
            if (v[q][0] != v[q][0] || v[q][1] != v[q][1] || v[q][2] != v[q][2] || v[q][3] != v[q][3]) m = INFINITY;   // fmaxf drops NaNs: a NaN weight must not pass as finite
        }
    }
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    // ONE atomic per block: an atomic on one address costs ~12 ns whoever issues it, and the 3072 per-wave atomics of this launch were its 40 us
    // (round 5: the loads in flight changed nothing)
    __shared__ float wmaxs[4];
    if ((threadIdx.x & 63) == 0) wmaxs[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(out + l, __float_as_uint(fmaxf(fmaxf(wmaxs[0], wmaxs[1]), fmaxf(wmaxs[2], wmaxs[3]))));
}
// power-of-two exponent that brings a tensor whose |maximum| has bit pattern max_bits to ~target; a non-finite maximum (a diverged
// step) gives exponent 0 and t_bad_max() -- the converting kernels raise the sticky flag (bit 2) so that the step fails loudly
__device__ __forceinline__ bool t_bad_max(unsigned max_bits) { return !(__uint_as_float(max_bits) <= 3.402823466e38f); }      // Inf or NaN
__device__ __forceinline__ int t_exp_for(unsigned max_bits, float target) {
    const float mx = __uint_as_float(max_bits);
    if (!(mx > 0.f) || t_bad_max(max_bits)) return 0;
    const int e = (int)floorf(log2f(target / mx));
    return e < -120 ? -120 : e > 120 ? 120 : e;
}
// The k order of a 3x3 weight operand of k_gemm_h2 / k_gemm_b3 is k' = (slice * 9 + tap) * 32 + c32: the group of 8 k' starting at kp lies in one tap,
// at 8 consecutive channels from ch = slice * 32 + c32
__device__ __forceinline__ void t_kp_tap_channel(int kp, int& tap, int& ch) {
    const int tile = kp >> 5, slice = tile / 9;
    tap = tile - slice * 9; ch = slice * 32 + (kp & 31);
}
// Data-gradient weight operand (both split formats): row n = ci, channel of k' = co, value W[8 - tap][ci][co] (the reversed, channel-swapped taps).
// One thread per (row, group of 8 k'), the groups of a row adjacent: thread idx -> its row, its kp and its 8 values = 8 consecutive co (one 32-byte
// read); false beyond the operand
__device__ __forceinline__ bool t_wd_load8(const float* __restrict__ W, int Cin, int Cout, long long idx, int& nrow, int& kp, float* v) {
    const int ng = 9 * Cout / 8;
    if (idx >= (long long)Cin * ng) return false;
    nrow = (int)(idx / ng); kp = (int)(idx % ng) * 8;
    int tap, ch;
    t_kp_tap_channel(kp, tap, ch);
    const float* q = W + ((size_t)(8 - tap) * Cin + nrow) * Cout + ch;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = q[j];
    return true;
}
// dz (zero-bordered [B][Hz][Hz][C] fp32, interior Hout^2 at offset zoff) -> the same geometry in a split format, one thread per (interior pixel, 8
// channels): thread idx -> the pixel's row in the zero-bordered buffer and the group's first channel; false beyond the *d_count boards.  Only the
// interior is written: the packed buffers are zeroed once at allocation, so their border stays zero.
__device__ __forceinline__ bool t_dz_row8(long long idx, const int* __restrict__ d_count, int Hout, int Hz, int zoff, int C, size_t& row, int& c8) {
    const int cg = C >> 3, P = Hout * Hout;
    const long long m = idx / cg;
    if (m >= (long long)(*d_count) * P) return false;
    const int b = (int)(m / P), pix = (int)(m % P);
    row = ((size_t)b * Hz + pix / Hout + zoff) * Hz + pix % Hout + zoff;
    c8 = (int)(idx % cg) * 8;
    return true;
}
// Keras kernel W[9][Cin][Cout] fp32 -> a k_gemm_h2 weight operand in the h2 layout, scaled by 2^kexp (kexp from the tensor's maximum), straight
// from the master weights (no fp32 intermediate):
//   DGRAD = 0  forward operand:       row n = co, channel of k' = ci:  W[tap][ci][co]        (threads adjacent in co: coalesced reads)
//   DGRAD = 1  data-gradient operand: t_wd_load8
// scale_out[n] = 2^-kexp (forward only).  One thread per (row, group of 8 k').
template <int DGRAD>
__global__ __launch_bounds__(256) void k_t_w_to_h2(const float* __restrict__ W, int Cin, int Cout, const unsigned* __restrict__ wmax,
                                                   uint4* __restrict__ out, float* __restrict__ scale_out, int* __restrict__ flag) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int kexp = t_exp_for(*wmax, T_W_TARGET);
    if (idx == 0 && t_bad_max(*wmax)) atomicOr(flag, 2);
    int nrow, kp;
    float v[8];
    if (DGRAD) {
        if (!t_wd_load8(W, Cin, Cout, idx, nrow, kp, v)) return;
    } else {
        if (idx >= (long long)Cout * (9 * Cin / 8)) return;
        nrow = (int)(idx % Cout); kp = (int)(idx / Cout) * 8;
        int tap, ch;
        t_kp_tap_channel(kp, tap, ch);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = W[((size_t)tap * Cin + ch + j) * Cout + nrow];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ldexpf(v[j], kexp);
    h2_store8(out, nrow, 9 * (DGRAD ? Cout : Cin), kp, v);
    if (!DGRAD && kp == 0) scale_out[nrow] = ldexpf(1.0f, -kexp);
}
// activation rows [M][C] fp32 -> h2 layout (the next layer's A operand)
__global__ __launch_bounds__(256) void k_t_act_to_h2(const float* __restrict__ a, const int* __restrict__ d_count, int P, int C,
                                                     uint4* __restrict__ out, int* __restrict__ flag) {
    const int cg = C >> 3;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, m = idx / cg;
    if (m >= (long long)(*d_count) * P) return;
    const int g8 = (int)(idx % cg);
    const float* q = a + (size_t)m * C + g8 * 8;
    float v[8];
    bool over = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v[j] = q[j]; over |= fabsf(v[j]) > 65504.0f; }
    h2_store8(out, m, C, g8 * 8, v);
    if (over) atomicOr(flag, 1);
}
// dz -> the h2 layout (t_dz_row8), scaled by 2^ez with ez from the tensor's maximum (dzmax, left by the BN backward);
// dscale[c] = 2^-(ez + kexp of the data-gradient weights)
__global__ __launch_bounds__(256) void k_t_dz_to_h2(const float* __restrict__ dz, const int* __restrict__ d_count, int Hout, int Hz, int zoff, int C,
                                                    const unsigned* __restrict__ dzmax, const unsigned* __restrict__ wmax,
                                                    uint4* __restrict__ out, float* __restrict__ dscale, int ncols, int* __restrict__ flag) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ez = t_exp_for(*dzmax, T_DZ_TARGET);
    if (idx == 0 && (t_bad_max(*dzmax) || t_bad_max(*wmax))) atomicOr(flag, 2);
    if (idx < ncols) dscale[idx] = ldexpf(1.0f, -(ez + t_exp_for(*wmax, T_W_TARGET)));
    size_t row;
    int c8;
    if (!t_dz_row8(idx, d_count, Hout, Hz, zoff, C, row, c8)) return;
    const float* q = dz + row * C + c8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ldexpf(q[j], ez);
    h2_store8(out, row, C, c8, v);
}

// ---------------------------------------------------------------- bf16x3 mode of the 3x3 layers (oz_trainer_set_precision 2)
// Every fp32 operand travels EXACTLY as three bf16 planes (oz_net_b3.h: b3_split, the b3 layout, six products per fp32 product in the order
// a3 b1 + a1 b3 + a2 b2 + a2 b1 + a1 b2 + a1 b1, fp32 accumulation).  bf16 has fp32's exponent range: no scaling, no maxima, no range flag.
// Forward and data gradient of conv2..conv4 run on k_gemm_b3 (oz_gemm_b3_launch), their weight gradients on k_wgrad_b3 below; conv1, the
// dense layers, the heads, BN and Adam stay exact fp32.  The operands are converted per step from the fp32 masters / tensors.
// Fallback rule: none.  Every trainer capacity (Bmax) takes these kernels: the GEMMs split their k loop until the grid fills the chip (keyed on
// Bmax), the weight gradient splits its board range; at the reference's batch of 32 both already beat the exact-fp32 kernels they replace.
//
// The forward weight operand is k_w_to_b3's (oz_w_to_b3_launch, taps = 9); the data-gradient operand is t_wd_load8's, unscaled.
__global__ __launch_bounds__(256) void k_t_w_to_b3(const float* __restrict__ W, int Cin, int Cout, uint4* __restrict__ out) {
    int nrow, kp;
    float v[8];
    if (!t_wd_load8(W, Cin, Cout, (long long)blockIdx.x * blockDim.x + threadIdx.x, nrow, kp, v)) return;
    b3_store8(out, nrow, 9 * Cout, kp, v);
}
// dz -> the b3 layout (t_dz_row8), unscaled
__global__ __launch_bounds__(256) void k_t_dz_to_b3(const float* __restrict__ dz, const int* __restrict__ d_count, int Hout, int Hz, int zoff, int C,
                                                    uint4* __restrict__ out) {
    size_t row;
    int c8;
    if (!t_dz_row8((long long)blockIdx.x * blockDim.x + threadIdx.x, d_count, Hout, Hz, zoff, C, row, c8)) return;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(dz + row * C + c8), hi = *reinterpret_cast<const f32x4*>(dz + row * C + c8 + 4);
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    b3_store8(out, row, C, c8, v);
}

// ---------------------------------------------------------------- weight gradient of the 3x3 layers on the fp16 / bf16 matrix cores (f16x2: round 3, bf16x3: round 7)
// dW[tap][ci][co] = sum over boards b and output pixels p of X[b][p + tap][ci] * dZ[b][p][co]: the contraction runs over (board, pixel),
// the WRONG major for the 16-bit operand map (v_mfma_f32_16x16x32_{f16,bf16} wants, per lane, 8 consecutive k of one row / column; the tensors are
// stored pixel-major with the channels contiguous).  The k-groups of 8 are therefore 8 BOARDS at one pixel: a tap shift changes the pixel,
// never the alignment of a k-group, and the four k-groups of one MFMA are four neighbouring output pixels.  Both tensors are first written
// as "octet images" -- [octet of 8 boards][row][pixel slot][plane][channel][8 boards] 16-bit, 16 bytes per (pixel, plane, channel) --
// by two bandwidth-bound kernels (X with its zero border for 'same' layers and zero columns up to WH_XW; dZ with zero columns up to WH_ZW, in f16x2
// scaled into the fp16 range by the power of two the data gradient uses: a row of either is two whole k-quads for every layer), so the GEMM kernel
// stages with LDS-DMA only: no transposes, no staging registers.
// wgrad_oct_body: a block of 8 waves owns a CI x CO tile for ALL NINE taps (9 x NJ accumulator tiles of 16 x 16 per wave).  Per octet it walks the
// output rows: three X rows (a ring of four row slots: the row of the next step streams in during the MFMAs of this one) and one dZ row (two
// buffers) are resident; every tap reads the SAME staged rows at a shifted pixel slot, and the dZ fragments of a pixel quad are read once for all
// nine taps.  fp32 accumulation.  Octet ranges split over blockIdx.y until every CU has a block (raw slabs + k_t_sum_partials, fixed order).  Rows
// of fewer than 8 real pixels (conv3: 6, conv4: 4) pay for the zero columns (+24 % MFMA work over the three layers) -- the price of one uniform
// step shape.  What differs between the two precisions is in WgradH2 / WgradB3 below.
#define WH_MIN_BATCH 32     // f16x2: batches from here on take k_wgrad_h2 (round 6: was 128; at the reference's batch of 32 the fp32 weight gradients on the second stream -- 52 + 82 +
                            // 151 us -- WERE the critical path of the backward pass)
#define WH_XW 10           // pixel slots of an X row (columns >= Hin + 2 pad hold zeros)
#define WH_ZW 8            // pixel slots of a dZ row (columns >= Hout hold zeros)
// Octet images, PLANES = 2 (f16x2: h1 | h2 in fp16, dZ scaled) or 3 (bf16x3: the three bf16 planes, unscaled); a 16-byte entry holds one
// (pixel, plane, channel) of 8 boards, split by oz_split8_store.
// X octet image of a[l - 1] ([B][Hin][Hin][C] fp32): out[octet][row < Hin + 2 pad][slot < WH_XW][plane][C] x 16 B (zero border, zero columns,
// zero boards >= B).  One thread per (cell, 4 channels): eight 16-byte loads (one per board), 4 x PLANES 16-byte stores.
template <int PLANES>
__device__ __forceinline__ void t_store_octet4(uint4* __restrict__ dst, int C, const f32x4* v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float x[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) x[b] = v[b][q];
        oz_split8_store<PLANES>(dst + q, C, x);
    }
}
template <int PLANES>
__global__ __launch_bounds__(256) void k_t_x_octets(const float* __restrict__ a, const int* __restrict__ d_count, int Hin, int pad, int C, uint4* __restrict__ out) {
    const int B = *d_count, XR = Hin + 2 * pad, noct = (B + 7) >> 3, C4 = C >> 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)noct * XR * WH_XW * C4) return;
    const int ch = (int)(idx % C4) * 4;
    const long long cell = idx / C4;
    const int c = (int)(cell % WH_XW), r = (int)((cell / WH_XW) % XR), oct = (int)(cell / ((long long)WH_XW * XR));
    const int iy = r - pad, ix = c - pad;
    const bool inside = iy >= 0 && iy < Hin && ix >= 0 && ix < Hin;
    f32x4 v[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int bb = oct * 8 + b;
        v[b] = (inside && bb < B) ? *reinterpret_cast<const f32x4*>(a + (((size_t)bb * Hin + iy) * Hin + ix) * C + ch) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    t_store_octet4<PLANES>(out + (size_t)cell * PLANES * C + ch, C, v);
}
// dZ octet image of dz[l] (zero-bordered [B][Hz][Hz][C] fp32, interior Hout^2 at offset zoff): out[octet][row < Hout][slot < WH_ZW][plane][C] x 16 B;
// f16x2 only: scaled by 2^ez (ez from the tensor's maximum dzmax), a non-finite maximum raises flag bit 2
template <int PLANES>
__global__ __launch_bounds__(256) void k_t_z_octets(const float* __restrict__ dz, const int* __restrict__ d_count, int Hout, int Hz, int zoff, int C,
                                                    const unsigned* __restrict__ dzmax, uint4* __restrict__ out, int* __restrict__ flag) {
    const int B = *d_count, noct = (B + 7) >> 3, C4 = C >> 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (PLANES == 2) {
        if (idx == 0 && t_bad_max(*dzmax)) atomicOr(flag, 2);
    }
    if (idx >= (long long)noct * Hout * WH_ZW * C4) return;
    const int ez = PLANES == 2 ? t_exp_for(*dzmax, T_DZ_TARGET) : 0;
    const int ch = (int)(idx % C4) * 4;
    const long long cell = idx / C4;
    const int c = (int)(cell % WH_ZW), r = (int)((cell / WH_ZW) % Hout), oct = (int)(cell / ((long long)WH_ZW * Hout));
    f32x4 v[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int bb = oct * 8 + b;
        v[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < Hout && bb < B) {
            v[b] = *reinterpret_cast<const f32x4*>(dz + (((size_t)bb * Hz + r + zoff) * Hz + c + zoff) * C + ch);
            if constexpr (PLANES == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[b][q] = ldexpf(v[b][q], ez);
            }
        }
    }
    t_store_octet4<PLANES>(out + (size_t)cell * PLANES * C + ch, C, v);
}
struct WhGeom { int XR, Hout, Cin, Cout; };
// What a precision brings to wgrad_oct_body: PLANES per value, the block's CI x CO tile as 8 waves = (CI / 16) x WN with NJ 16-wide co tiles per
// wave, the fragment type, and mac() = the MFMA products of one fp32 product IN ACCUMULATION ORDER (small terms first; the order is the bits).
// k_wgrad_h2: 64 ci x 128 co, 8 waves = 4 x 16 ci by 2 x 64 co; X row 20 KB, dZ row 32 KB, 144 KB of LDS; 26 ds_read_b128 per 108 MFMAs per wave;
// three fp16 products per fp32 product (x2 z1 + x1 z2 + x1 z1), 2^-ez of the scaled dZ folded into the epilogue.
struct WgradH2 {
    typedef f16x8 Frag;
    static constexpr int PLANES = 2, CI = 64, CO = 128, NJ = 4, WN = 2;
    static constexpr bool SCALED = true;
    static __device__ __forceinline__ f32x4 mac(const Frag* x, const Frag (*z)[NJ], int j, f32x4 acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(x[1], z[0][j], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(x[0], z[1][j], acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(x[0], z[0][j], acc, 0, 0, 0);
    }
};
// k_wgrad_b3: six bf16 products per fp32 product (x3 z1, x1 z3, x2 z2, x2 z1, x1 z2, x1 z1), unscaled.
// LDS plan: with three planes k_wgrad_h2's 64 ci x 128 co tile would need 4 X rows of 30 KB + 2 dZ rows of 48 KB = 216 KB, more than a CU's
// 160 KB.  This kernel uses 32 ci x 128 co: 4 x 15 KB + 2 x 48 KB = 156 KB (one block per CU), which keeps the ring's one-row prefetch; a
// 64 x 64 tile would fit only with a 3-row X ring (138 KB), which cannot stream the next row in beside the MFMAs of the current one, and was not built.
// 8 waves = 2 (16 ci) x 4 (32 co); per pixel quad a wave reads 6 dZ + 27 X fragments (ds_read_b128) for 108 MFMAs.
// Measured in the training step (8x8, 512 filters, rocprofv3): 56 us per layer at batch 32, 406 us at batch 256 -- bound by the operand stream
// (every dZ row is staged by C / 32 blocks), not the matrix pipe (profiles/r7_train_b{32,256}_bf16x3_kernel_stats.csv, docs/HISTORY.md round 7).
struct WgradB3 {
    typedef bf16x8 Frag;
    static constexpr int PLANES = 3, CI = 32, CO = 128, NJ = 2, WN = 4;
    static constexpr bool SCALED = false;
    static __device__ __forceinline__ f32x4 mac(const Frag* x, const Frag (*z)[NJ], int j, f32x4 acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[2], z[0][j], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[0], z[2][j], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[1], z[1][j], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[1], z[0][j], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[0], z[1][j], acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[0], z[0][j], acc, 0, 0, 0);
    }
};
template <typename T> struct WgradLds {
    static constexpr int XROW = T::PLANES * WH_XW * T::CI * 16;      // bytes of one staged X row: [plane][slot][ci] x 16 B
    static constexpr int ZROW = T::PLANES * WH_ZW * T::CO * 16;      // bytes of one staged dZ row: [plane][slot][co] x 16 B
    static constexpr int BYTES = 4 * XROW + 2 * ZROW;
    static_assert(T::CI * T::WN == 128 && T::CO == T::WN * T::NJ * 16 && T::CO == 128 && 64 % T::CI == 0, "8 waves of 16 ci x NJ x 16 co; a dZ row in halves of 64 co");
    static_assert(BYTES <= 160 * 1024, "a CU's LDS");
};
template <typename T>
__device__ __forceinline__ void wgrad_oct_body(unsigned char* const lds, const uint4* __restrict__ Xt, const uint4* __restrict__ Zt, const int* __restrict__ d_count,
                                               WhGeom g, const unsigned* __restrict__ dzmax, float* __restrict__ dW, int msplit, float* __restrict__ partial,
                                               long long slab) {
    typedef typename T::Frag Frag;
    constexpr int PLANES = T::PLANES, CI = T::CI, CO = T::CO, NJ = T::NJ, XROW = WgradLds<T>::XROW, ZROW = WgradLds<T>::ZROW;
    unsigned char* const Xring = lds;
    unsigned char* const Zbuf = lds + 4 * XROW;
    const int nco = g.Cout / CO;
    const int ci0 = (blockIdx.x / nco) * CI, co0 = (blockIdx.x % nco) * CO;
    const int noct = (*d_count + 7) >> 3;
    const int per = (noct + msplit - 1) / msplit, o0 = blockIdx.y * per, o1 = o0 + per < noct ? o0 + per : noct;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wm = wave / T::WN, wn = wave % T::WN, r16 = lane & 15, g4 = lane >> 4;

    // LDS-DMA: one instruction = 64 consecutive 16-byte entries, and a staged row is its instructions in order (instruction q lands at q x 1 KB).
    // X row: the (plane, slot) pairs in plane-major order, 64 / CI of them per instruction (WH_XW is a multiple of that: both in one plane), lanes =
    // pairs x the CI channels of the tile -- 20 instructions at 64 ci, 15 at 32 ci.  dZ row: (plane, slot, half) with lanes = 64 of the tile's 128
    // co -- 32 / 48 instructions.  Wave w issues q = w, w + 8, ...
    auto dma_x = [&](int oct, int row, int slot) {
        constexpr int PER = 64 / CI;
        const uint4* src = Xt + (((size_t)oct * g.XR + row) * WH_XW) * PLANES * g.Cin + ci0 + (lane & (CI - 1));
        for (int q = wave; q < PLANES * WH_XW / PER; q += 8) {
            const int pc = PER * q + lane / CI, p = pc / WH_XW, c = pc - p * WH_XW;
            __builtin_amdgcn_global_load_lds((oz_gptr)(src + ((size_t)c * PLANES + p) * g.Cin), (oz_lptr)(Xring + slot * XROW + q * 1024), 16, 0, 0);
        }
    };
    auto dma_z = [&](int oct, int row, int buf) {
        const uint4* src = Zt + (((size_t)oct * g.Hout + row) * WH_ZW) * PLANES * g.Cout + co0 + lane;
        for (int q = wave; q < PLANES * WH_ZW * 2; q += 8) {
            const int h = q & 1, pc = q >> 1, p = pc / WH_ZW, c = pc - p * WH_ZW;
            __builtin_amdgcn_global_load_lds((oz_gptr)(src + ((size_t)c * PLANES + p) * g.Cout + h * 64), (oz_lptr)(Zbuf + buf * ZROW + q * 1024), 16, 0, 0);
        }
    };

    f32x4 acc[9][NJ];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int oct = o0; oct < o1; ++oct) {
        // the three X rows and the dZ row of output row 0 (the previous octet's last step ended with a barrier: every slot is free)
        dma_x(oct, 0, 0); dma_x(oct, 1, 1); dma_x(oct, 2, 2); dma_z(oct, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int oy = 0; oy < g.Hout; ++oy) {
            if (oy + 1 < g.Hout) { dma_x(oct, oy + 3, (oy + 3) & 3); dma_z(oct, oy + 1, (oy + 1) & 1); }     // slots last read in step oy - 1
            const unsigned char* Zr = Zbuf + (oy & 1) * ZROW + (wn * NJ * 16 + r16) * 16;
#pragma unroll
            for (int quad = 0; quad < 2; ++quad) {
                const int px = quad * 4 + g4;
                Frag z[PLANES][NJ];
#pragma unroll
                for (int p = 0; p < PLANES; ++p)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) z[p][j] = *reinterpret_cast<const Frag*>(Zr + ((p * WH_ZW + px) * CO + j * 16) * 16);
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int dy = t / 3, dx = t - 3 * dy;
                    const unsigned char* Xr = Xring + ((oy + dy) & 3) * XROW + (wm * 16 + r16) * 16;
                    Frag x[PLANES];
#pragma unroll
                    for (int p = 0; p < PLANES; ++p) x[p] = *reinterpret_cast<const Frag*>(Xr + ((p * WH_XW + px + dx) * CI) * 16);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[t][j] = T::mac(x, z, j, acc[t][j]);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next step's rows have landed (this wave's pieces) ...
            __syncthreads();                                       // ... everybody's, and everybody is done reading this step's
        }
    }
    // C/D layout of the 16 x 16 MFMA: col = lane & 15 (co), row = (lane >> 4) * 4 + reg (ci).  The scale is read HERE: read at the top it lives
    // through the main loop in registers the accumulators need
    float sc = 1.0f;
    if constexpr (T::SCALED) sc = ldexpf(1.0f, -t_exp_for(*dzmax, T_DZ_TARGET));
    float* __restrict__ outp = msplit > 1 ? partial + (size_t)blockIdx.y * slab : dW;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = ci0 + wm * 16 + g4 * 4 + r, co = co0 + (wn * NJ + j) * 16 + r16;
                outp[((size_t)t * g.Cin + ci) * g.Cout + co] = T::SCALED ? acc[t][j][r] * sc : acc[t][j][r];
            }
}
__global__ __launch_bounds__(512, 2) void k_wgrad_h2(const uint4* __restrict__ Xt, const uint4* __restrict__ Zt, const int* __restrict__ d_count, WhGeom g,
                                                     const unsigned* __restrict__ dzmax, float* __restrict__ dW, int msplit, float* __restrict__ partial,
                                                     long long slab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wh_lds[];
    wgrad_oct_body<WgradH2>(wh_lds, Xt, Zt, d_count, g, dzmax, dW, msplit, partial, slab);
}
__global__ __launch_bounds__(512) void k_wgrad_b3(const uint4* __restrict__ Xt, const uint4* __restrict__ Zt, const int* __restrict__ d_count, WhGeom g,
                                                  float* __restrict__ dW, int msplit, float* __restrict__ partial, long long slab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wb_lds[];
    wgrad_oct_body<WgradB3>(wb_lds, Xt, Zt, d_count, g, nullptr, dW, msplit, partial, slab);
}

// ---------------------------------------------------------------- Adam (tf.keras formulation) with clipvalue
__global__ __launch_bounds__(256) void k_t_adam(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M1, float* __restrict__ V2,
                                                long long count, float lr_t, float clip) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float g = G[i];
    if (clip > 0.f) g = fminf(fmaxf(g, -clip), clip);
    const float m = 0.9f * M1[i] + 0.1f * g;
    const float v = 0.999f * V2[i] + 0.001f * g * g;
    M1[i] = m; V2[i] = v;
    P[i] -= lr_t * m / (sqrtf(v) + 1e-7f);
}

// ---------------------------------------------------------------- optimiser options (oz_trainer_set_optimizer): the fused step and the norm
// The arena as 16-byte units: every array starts on one and is padded to whole ones (t_layout), so a unit never straddles two arrays.  The
// decayed arrays reach the kernel as at most T_OPT_SEGS merged unit ranges, BY VALUE in the kernel arguments: the range loop's index is uniform,
// so the bounds are scalar loads and the test costs two compares per range and unit (eight ranges under the default mask) beside nine 16-byte
// streams -- no table in memory, no per-lane indexing of the arguments (which would go to scratch).
#define T_OPT_SEGS 28                        // trainable arrays of the network
#define T_OPT_ARRAYS (T_OPT_SEGS + 4)        // ... and of a trainer with the auxiliary heads (the norm's table alone: decayed arrays that follow each other merge into one range)
struct TUnitRanges { int n; int lo[T_OPT_SEGS], hi[T_OPT_SEGS]; };             // units [lo, hi)
struct TSegs { int n; long long off[T_OPT_ARRAYS], len[T_OPT_ARRAYS]; };       // arrays: offset in the arena (floats, a multiple of 4) and ELEMENT count
struct TAdamX { float lr_t, clip, c2 /* 2 c */, lam /* lr_s lambda */, d, omd /* 1 - d */; };
struct TNormOut { double sumsq, norm, scale; float scale32, pad; };
#define T_OPT_ADAM_BLOCKS 2048               // grid caps: the rest is grid-stride
#define T_OPT_SQ_BLOCKS 1024

// one element of the six-step order in the header; what it shares with k_t_adam is spelled as there (bit-identical where no option acts)
__device__ __forceinline__ void t_adam_x_elem(float& p, float g, float& m1, float& v2, float& e, bool scaled, float s, bool dec, bool avg, const TAdamX& a) {
    if (scaled) g = g * s;
    if (dec && a.c2 > 0.f) g = g + a.c2 * p;
    if (a.clip > 0.f) g = fminf(fmaxf(g, -a.clip), a.clip);
    const float m = 0.9f * m1 + 0.1f * g;
    const float v = 0.999f * v2 + 0.001f * g * g;
    m1 = m; v2 = v;
    float w = p - a.lr_t * m / (sqrtf(v) + 1e-7f);
    if (dec && a.lam > 0.f) w = w - a.lam * p;
    p = w;
    if (avg) e = a.d * e + a.omd * w;
}
__global__ __launch_bounds__(256) void k_t_adam_x(float4* __restrict__ P, const float4* __restrict__ G, float4* __restrict__ M1, float4* __restrict__ V2,
                                                  float4* __restrict__ E /* nullptr: no average */, int units, TAdamX a,
                                                  const float* __restrict__ scale /* nullptr: no global-norm clip */, TUnitRanges decay) {
    const bool scaled = scale != nullptr, avg = E != nullptr;
    const float s = scaled ? *scale : 1.0f;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < units; q += gridDim.x * 256) {
        bool dec = false;
        for (int r = 0; r < decay.n; ++r) dec |= q >= decay.lo[r] && q < decay.hi[r];
        float4 p = P[q], m = M1[q], v = V2[q], e = avg ? E[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 g = G[q];
        t_adam_x_elem(p.x, g.x, m.x, v.x, e.x, scaled, s, dec, avg, a);
        t_adam_x_elem(p.y, g.y, m.y, v.y, e.y, scaled, s, dec, avg, a);
        t_adam_x_elem(p.z, g.z, m.z, v.z, e.z, scaled, s, dec, avg, a);
        t_adam_x_elem(p.w, g.w, m.w, v.w, e.w, scaled, s, dec, avg, a);
        P[q] = p; M1[q] = m; V2[q] = v;
        if (avg) E[q] = e;
    }
}

// Sum of squares of the ELEMENTS of the listed arrays (the padding behind an array is never read into the sum), float64, two stages, every
// partial sum combined in a fixed order (no atomics): thread -> wave (shuffle tree) -> block (the four wave sums in order) -> partial[block];
// then one block adds the partials, thread i taking i, i + 256, .., and finishes.
__device__ __forceinline__ double t_block_sum(double acc, double* sh) {
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ __launch_bounds__(256) void k_t_sqsum(const float* __restrict__ X, TSegs sg, double* __restrict__ partial) {
    __shared__ double sh[4];
    const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    double acc = 0.0;
    for (int r = 0; r < sg.n; ++r) {
        const float* x = X + sg.off[r];
        const long long len = sg.len[r], n4 = len >> 2;
        for (long long q = tid; q < n4; q += nth) {
            const float4 f = reinterpret_cast<const float4*>(x)[q];
            acc += (double)f.x * (double)f.x; acc += (double)f.y * (double)f.y; acc += (double)f.z * (double)f.z; acc += (double)f.w * (double)f.w;
        }
        if (tid == 0) for (long long i = n4 * 4; i < len; ++i) acc += (double)x[i] * (double)x[i];      // the array's last, partial unit
    }
    const double sum = t_block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}
__global__ __launch_bounds__(256) void k_t_sqsum_fin(const double* __restrict__ partial, int count, double clipnorm, TNormOut* __restrict__ out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) acc += partial[i];
    const double sum = t_block_sum(acc, sh);
    if (threadIdx.x == 0) {
        const double norm = sqrt(sum), sc = clipnorm > 0.0 && norm > clipnorm ? clipnorm / norm : 1.0;
        out->sumsq = sum; out->norm = norm; out->scale = sc; out->scale32 = (float)sc; out->pad = 0.f;
    }
}

// ---------------------------------------------------------------- host object
// Layer l = 0 .. 5 (conv1 .. conv4, fc1, fc2) as the step sees it: the GEMM shape (conv1 is no GEMM: its Cin is the input planes), P = Hout^2
// output pixels, and the dz buffer's geometry -- conv3 / conv4 ('valid') keep dz in a zero-bordered Hz x Hz buffer (zoff = 2) so that their data
// gradient is a plain valid convolution.  Built once in oz_trainer_create from oz_onn_layers; every buffer size and launch reads it.
struct TLayer { int Hin, Hout, pad, Cin, taps, Co, P, Hz, zoff; };
// The operands of conv2 .. conv4 (l = 1 .. 3) in a split format, PLANES 16-bit planes per fp32 value: f16x2 (2, the h2 layout) or bf16x3 (3, the b3
// layout).  W / Wd: forward / data-gradient weight operand; act[l - 1]: the layer's input rows; dz: its zero-bordered data gradient;
// xoct / zoct: the octet images of the weight gradient (k_t_x_octets / k_t_z_octets).
struct TPacked { uint4 *W[4] = {}, *Wd[4] = {}, *act[3] = {}, *dz[4] = {}, *xoct[4] = {}, *zoct[4] = {}; };
struct oz_trainer {
    int n = 8, C = 512, cin = 2, Bmax = 32, device = 0;
    TLayer L[6];
    float lr = 1e-3f, clip = 0.5f, rate = 0.3f, mom = 0.99f;
    uint64_t seed = 0;
    int64_t step = 0;
    int policy_loss = OZ_POLICY_LOSS_ROWS;   // oz_trainer_set_policy_loss
    hipStream_t s = nullptr;
    int64_t size[44], toff[44];          // element counts; offset in the trainable arena (-1: moving statistic); 40 .. 43: the auxiliary heads
    int64_t total = 0;
    // auxiliary heads (oz_trainer_set_aux_heads): nw = 44 arrays, the four new ones at the end of the arenas; the staged batch's final pairs
    // (pinned mirror h_fin), the heads' outputs, pre-activation gradients, per-sample losses and the two batch means; the resident data set's pairs
    bool aux = false;
    int nw = 40;
    float w_own = 0.f, w_sc = 0.f;
    uint64_t *d_fin = nullptr, *h_fin = nullptr;         // [2][Bmax]: fin_own, fin_opp
    float *ao = nullptr, *as = nullptr, *dopre = nullptr, *dspre = nullptr, *aux_loss = nullptr, *aux_losses = nullptr;
    float* cap_f2 = nullptr;             // capture: the gradient wrt f2 as k_t_heads_dgrad left it, before its second launch's add
    uint64_t *ds_fo = nullptr, *ds_fp = nullptr;
    int64_t ds_fin_cap = 0;
    double epoch_aux[2] = {0.0, 0.0};    // the last fit epoch's sample-weighted means of the two losses
    float *P = nullptr, *G = nullptr, *M1 = nullptr, *V2 = nullptr;
    bool own_grads = true;
    float *stats[40] = {}, *stats_new[40] = {};
    float *Wt[6] = {}, *Wd[6] = {};
    uint64_t *d_own = nullptr, *d_opp = nullptr;
    float *d_pit = nullptr, *d_zt = nullptr;
    int* d_count = nullptr;
    unsigned char *d_in = nullptr, *h_in = nullptr;      // the device block the five pointers above point into, and its pinned host mirror
    size_t in_bytes = 0;
    float *z[6] = {}, *a[6] = {}, *mean[6] = {}, *rstd[6] = {}, *dz[6] = {};
    float *dA[2] = {}, *partial = nullptr, *ones = nullptr, *zeros = nullptr;
    float *p = nullptr, *v = nullptr, *dlogit = nullptr, *dvpre = nullptr, *loss = nullptr, *losses = nullptr;
    float* gpartial = nullptr;           // split-K scratch of the small-batch GEMMs
    float* wpartial = nullptr;           // row-split scratch of the weight-gradient launches (they run on s2, beside the data-gradient chain)
    hipStream_t s2 = nullptr;
    hipEvent_t ev_dz[6] = {}, ev_w = nullptr;
    hipEvent_t ev_pre = nullptr, ev_wt = nullptr, ev_wd = nullptr;      // derived weight operands are rebuilt on s2 beside the first forward kernels
    hipEvent_t ev_wl[4] = {nullptr, nullptr, nullptr, nullptr};         // f16x2 / bf16x3: the packed forward operand of layer l = 1 .. 3 is ready (the main stream waits layer by layer)
    bool wait_wt = false, wait_wd = false, wait_wl[4] = {false, false, false, false};
    // oz_trainer_set_precision: 0 f32; 1 f16x2 (conv2..4 forward and data gradient on k_gemm_h2, weight gradient on k_wgrad_h2); 2 bf16x3 (k_gemm_b3,
    // k_wgrad_b3).  pk[mode - 1] is allocated at the first use of a split mode and kept; the scales, maxima and the range flag are f16x2's alone
    int mode = 0;
    TPacked pk[2];
    float *wscale[4] = {}, *dscale[4] = {};
    unsigned *wmax = nullptr, *dzmax = nullptr;          // [3] max |w| of conv2..4, [6] max |dz| per layer (bit patterns)
    int* h2flag = nullptr;
    float* bnb2[6] = {};                 // per-layer row-block partials of the bias gradient (mid-size BN backward)
    long long gpartial_floats = 40LL << 20;      // 160 MB each: 16 row-split slabs of a 3x3 x 512 x 512 weight gradient
    // HBM-resident data set of a fit (oz_trainer_set_dataset / oz_trainer_fit_epoch)
    uint64_t *ds_own = nullptr, *ds_opp = nullptr;
    float *ds_pi = nullptr, *ds_z = nullptr;
    int* ds_order = nullptr;
    double* ds_acc = nullptr;
    int64_t ds_n = 0, ds_cap = 0, ds_order_cap = 0;
    // held-out evaluation (oz_trainer_evaluate*): an order buffer, example arrays (the host-array entry point), per-example rows and an accumulator of
    // its own -- the resident data set, ds_order and ds_acc of a fit are never touched
    int* ev_order = nullptr;
    uint64_t *ev_own = nullptr, *ev_opp = nullptr;
    float *ev_pi = nullptr, *ev_z = nullptr, *ev_rows = nullptr;
    TEvalAcc* ev_acc = nullptr;
    int64_t ev_order_cap = 0, ev_cap = 0;
    // diagnostics (oz_trainer_set_capture / get_dgrad / get_plan): the raw data gradients of a step, copied out of the ping-pong buffers, and its launch plan
    bool capture = false, cap_valid = false, ran = false;      // ran: a step has been enqueued (the views below have something to show)
    float* cap[6] = {};                  // cap[l] = the gradient wrt a[l] as the heads / the data-gradient launch of layer l + 1 left it (allocated at the first capture)
    int plan[OZ_TRAINER_PLAN_ROWS][OZ_TRAINER_PLAN_FIELDS] = {};      // rows 0 .. 4: layers 1 .. 5, row 5: conv1 (t_plan_row)
    // optimiser options (oz_trainer_set_optimizer).  fused: one of l2 / weight_decay / global_clipnorm / average_decay is on and the step runs
    // k_t_adam_x; otherwise t_apply_locked launches k_t_adam as it always did (a schedule alone only changes lr_t)
    oz_optimizer opt = {};
    bool fused = false, applied = false, last_clipped = false;
    float* E = nullptr;                  // the weight average: one more arena, allocated when average_decay is first switched on
    double* sq_partial = nullptr;        // T_OPT_SQ_BLOCKS partial sums of k_t_sqsum
    TNormOut* norm_out = nullptr;        // [0]: the last step's norm and scale (k_t_adam_x reads scale32), [1]: oz_trainer_sqsum's
    double last_lr_s = 0.0;
    TSegs seg_all = {}, seg_dec = {};    // the trainable arrays; the decayed ones (current or default mask)
    TUnitRanges dec_units = {};
    std::vector<void*> allocs;
    bool dirty = true;                   // derived operands need a refresh
    std::mutex mu;                       // one caller at a time (ThreadWorker-style Python threads)

    ~oz_trainer() {
        hipSetDevice(device);
        if (s) hipStreamSynchronize(s);
        for (void* q : allocs) hipFree(q);
        for (void* q : {(void*)ds_own, (void*)ds_opp, (void*)ds_pi, (void*)ds_z, (void*)ds_order, (void*)ds_acc}) if (q) hipFree(q);
        for (void* q : {(void*)ev_order, (void*)ev_own, (void*)ev_opp, (void*)ev_pi, (void*)ev_z, (void*)ds_fo, (void*)ds_fp}) if (q) hipFree(q);
        if (h_in) hipHostFree(h_in);
        if (h_fin) hipHostFree(h_fin);
        for (hipEvent_t e : ev_dz) if (e) hipEventDestroy(e);
        if (ev_w) hipEventDestroy(ev_w);
        for (hipEvent_t e : {ev_pre, ev_wt, ev_wd, ev_wl[1], ev_wl[2], ev_wl[3]}) if (e) hipEventDestroy(e);
        if (s2) hipStreamDestroy(s2);
        if (s) hipStreamDestroy(s);
    }
    float* param(int idx) { return toff[idx] >= 0 ? P + toff[idx] : stats[idx]; }
    float* grad(int idx) { return G + toff[idx]; }
};

// element counts of the 40 get_weights() arrays and their offsets in the trainable arena (-1: moving statistic);
// every array starts 16-byte aligned.  Returns the arena size in floats.  aux: the four arrays of the auxiliary heads (40 Wown [512][A],
// 41 bown [A], 42 Wsc [512], 43 bsc [1]) follow the forty, so the forty keep their offsets
static int64_t t_layout(int n, int C, int cin, int64_t* size, int64_t* toff, bool aux = false) {
    const int64_t A = n * n;
    const OzLayers net = oz_onn_layers(n, C);
    for (int l = 0; l < 6; ++l) {          // kernel [K][N], then bias, gamma, beta and the two moving statistics [N]
        const int64_t K = l ? net[l - 1].K() : 9 * cin, N = l ? net[l - 1].N : C;
        size[6 * l] = K * N;
        for (int j = 1; j < 6; ++j) size[6 * l + j] = N;
    }
    size[36] = 512 * A; size[37] = A; size[38] = 512; size[39] = 1;
    int64_t total = 0;
    for (int i = 0; i < 40; ++i) {
        const bool stat = i < 36 && (i % 6 == 4 || i % 6 == 5);
        toff[i] = stat ? -1 : total;
        if (!stat) total += (size[i] + 3) / 4 * 4;
    }
    if (aux) {
        size[40] = 512 * A; size[41] = A; size[42] = 512; size[43] = 1;
        for (int i = 40; i < 44; ++i) { toff[i] = total; total += i < 43 ? (size[i] + 3) / 4 * 4 : size[i]; }     // (the arena ends with bsc: no padding behind it)
    }
    return total;
}
// what a library-owned arena of `total` floats is allocated with: whole 16-byte units (an arena with the auxiliary heads ends inside one)
static int64_t t_arena_alloc(int64_t total) { return (total + 3) / 4 * 4; }

static int t_alloc(oz_trainer* t, void** out, size_t bytes, bool zero = true) {
    OZ_HIP(hipMalloc(out, bytes ? bytes : 16));
    t->allocs.push_back(*out);
    if (zero) OZ_HIP(hipMemsetAsync(*out, 0, bytes ? bytes : 16, t->s));
    return OZ_OK;
}
#define T_LOCK(t) std::lock_guard<std::mutex> lock__((t)->mu)
#define T_ALLOC(ptr, count) do { if (int rc__ = t_alloc(t, (void**)&(ptr), (size_t)(count) * sizeof(*(ptr)))) return rc__; } while (0)

// ---------------------------------------------------------------- optimiser options: validation, the schedule (host only), the segment tables
static bool t_is_stat(int i) { return i < 36 && (i % 6 == 4 || i % 6 == 5); }
static uint64_t t_decay_mask(const oz_optimizer& o, bool aux = false) {      // 0 = the default: the eight kernels (with the auxiliary heads: and their two)
    if (o.decay_mask) return o.decay_mask;
    uint64_t m = (1ull << 36) | (1ull << 38);
    for (int l = 0; l < 6; ++l) m |= 1ull << (6 * l);
    if (aux) m |= (1ull << 40) | (1ull << 42);
    return m;
}
static int t_opt_check(const oz_optimizer* o, const char* who) {
    if (!o) return OZ_OK;
    OZ_REQUIRE(o->l2 >= 0.0 && std::isfinite(o->l2), "%s: l2 %g (>= 0)", who, o->l2);
    OZ_REQUIRE(o->weight_decay >= 0.0 && std::isfinite(o->weight_decay), "%s: weight_decay %g (>= 0)", who, o->weight_decay);
    OZ_REQUIRE(!(o->l2 > 0.0 && o->weight_decay > 0.0), "%s: l2 and weight_decay are both positive (one decay at a time)", who);
    OZ_REQUIRE(o->global_clipnorm >= 0.0 && std::isfinite(o->global_clipnorm), "%s: global_clipnorm %g (>= 0)", who, o->global_clipnorm);
    OZ_REQUIRE(o->average_decay >= 0.0 && o->average_decay < 1.0, "%s: average_decay %g outside [0, 1)", who, o->average_decay);
    OZ_REQUIRE(o->schedule == OZ_LR_CONSTANT || o->schedule == OZ_LR_LINEAR || o->schedule == OZ_LR_COSINE, "%s: schedule %d", who, (int)o->schedule);
    OZ_REQUIRE(o->final_ratio >= 0.0 && o->final_ratio <= 1.0, "%s: final_ratio %g outside [0, 1]", who, o->final_ratio);
    OZ_REQUIRE(o->warmup_steps >= 0 && o->total_steps >= 0, "%s: negative warmup_steps / total_steps", who);
    OZ_REQUIRE(o->schedule == OZ_LR_CONSTANT || o->warmup_steps <= o->total_steps, "%s: warmup_steps %lld > total_steps %lld", who,
               (long long)o->warmup_steps, (long long)o->total_steps);
    OZ_REQUIRE(!(o->decay_mask >> 40), "%s: decay_mask has a bit past get_weights() index 39", who);
    for (int i = 0; i < 40; ++i)
        OZ_REQUIRE(!((o->decay_mask >> i) & 1) || !t_is_stat(i), "%s: decay_mask bit %d is a BN moving statistic (not trained, not decayed)", who, i);
    return OZ_OK;
}
// lr_s = lr f(s): the one definition (othellozero_amd.h); `o` is valid or NULL
static double t_lr_at(const oz_optimizer* o, float lr, int64_t step) {
    const double base = (double)lr;
    if (!o) return base;
    if (step <= o->warmup_steps) return base * ((double)step / (double)o->warmup_steps);
    if (o->schedule == OZ_LR_CONSTANT) return base;
    const int64_t span = o->total_steps - o->warmup_steps;
    double q = (double)(step - o->warmup_steps) / (double)(span > 1 ? span : 1);
    if (q > 1.0) q = 1.0;
    const double r = o->final_ratio;
    const double f = o->schedule == OZ_LR_LINEAR ? 1.0 - (1.0 - r) * q : r + (1.0 - r) * (0.5 * (1.0 + cos(M_PI * q)));
    return base * f;
}
OZ_API int oz_lr_schedule_at(const oz_optimizer* opt, float lr, int64_t step, double* out) {
    OZ_REQUIRE(out && step >= 1, "oz_lr_schedule_at: out is NULL or step < 1");
    if (int rc = t_opt_check(opt, "oz_lr_schedule_at")) return rc;
    *out = t_lr_at(opt, lr, step);
    return OZ_OK;
}
// the segment tables of the current options: every trainable array (the norm), the decayed ones (oz_trainer_sqsum), and the decayed ones as
// merged 16-byte-unit ranges (k_t_adam_x)
static void t_opt_tables(oz_trainer* t) {
    const uint64_t mask = t_decay_mask(t->opt, t->aux);
    t->seg_all.n = t->seg_dec.n = t->dec_units.n = 0;
    for (int i = 0; i < t->nw; ++i) {
        if (t->toff[i] < 0) continue;
        TSegs& a = t->seg_all;
        a.off[a.n] = t->toff[i]; a.len[a.n] = t->size[i]; a.n += 1;
        if (!((mask >> i) & 1)) continue;
        TSegs& d = t->seg_dec;
        d.off[d.n] = t->toff[i]; d.len[d.n] = t->size[i]; d.n += 1;
        TUnitRanges& u = t->dec_units;
        const int lo = (int)(t->toff[i] / 4), hi = (int)((t->toff[i] + (t->size[i] + 3) / 4 * 4) / 4);
        if (u.n && u.hi[u.n - 1] == lo) u.hi[u.n - 1] = hi;
        else { u.lo[u.n] = lo; u.hi[u.n] = hi; u.n += 1; }
    }
}

OZ_API int oz_trainer_create(oz_trainer** out, int n, int channels, int in_channels, int max_batch, float lr, float clipvalue,
                             float dropout, float bn_momentum, uint64_t seed, float* external_grads) {
    OZ_REQUIRE(out, "oz_trainer_create: out is NULL");
    OZ_REQUIRE(n == 6 || n == 8, "oz_trainer_create: board size %d (6 or 8: conv3/conv4 are 'valid')", n);
    OZ_REQUIRE(channels >= 128 && channels % 128 == 0, "oz_trainer_create: channels %d must be a multiple of 128", channels);
    OZ_REQUIRE(in_channels == 1 || in_channels == 2, "oz_trainer_create: in_channels %d", in_channels);
    OZ_REQUIRE(max_batch >= 1 && max_batch <= 65536, "oz_trainer_create: max_batch %d", max_batch);
    OZ_REQUIRE(dropout >= 0.f && dropout < 1.f, "oz_trainer_create: dropout %f", dropout);
    oz_trainer* t = new oz_trainer();
    t->n = n; t->C = channels; t->cin = in_channels; t->Bmax = max_batch; t->lr = lr; t->clip = clipvalue; t->rate = dropout;
    t->mom = bn_momentum; t->seed = seed; t->device = oz_current_device();
    auto fail = [&](int rc) { delete t; return rc; };
    if (hipSetDevice(t->device) != hipSuccess || hipStreamCreate(&t->s) != hipSuccess) { oz_set_error("oz_trainer_create: no GPU stream"); return fail(OZ_ERR_HIP); }
    const int C = channels, A = n * n, F = (n - 4) * (n - 4) * C;
    t->total = t_layout(n, C, in_channels, t->size, t->toff);
    t_opt_tables(t);
    int rc = [&]() -> int {
        T_ALLOC(t->P, t->total); T_ALLOC(t->M1, t->total); T_ALLOC(t->V2, t->total);
        if (external_grads) { t->G = external_grads; t->own_grads = false; } else T_ALLOC(t->G, t->total);
        for (int i = 0; i < 36; ++i) if (t->toff[i] < 0) { T_ALLOC(t->stats[i], t->size[i]); T_ALLOC(t->stats_new[i], t->size[i]); }
        const OzLayers net = oz_onn_layers(n, C);            // layer l >= 1 is GEMM layer l - 1; layer 0 = conv1 ('same', C filters)
        for (int l = 0; l < 6; ++l) {
            const OzLayerShape sh = l ? net[l - 1] : OzLayerShape{n, n, 1, in_channels, 9, C};
            const int zoff = sh.taps == 9 && sh.pad == 0 ? 2 : 0;
            const TLayer& L = t->L[l] = {sh.Hin, sh.Hout, sh.pad, sh.Cin, sh.taps, sh.N, sh.pixels(), sh.Hout + 2 * zoff, zoff};
            const size_t rows = (size_t)max_batch * L.P;
            T_ALLOC(t->z[l], rows * L.Co); T_ALLOC(t->a[l], rows * L.Co);
            T_ALLOC(t->dz[l], (size_t)max_batch * L.Hz * L.Hz * L.Co);
            T_ALLOC(t->mean[l], L.Co); T_ALLOC(t->rstd[l], L.Co);
        }
        const size_t amax = (size_t)max_batch * (size_t)A * C > (size_t)max_batch * 1024 ? (size_t)max_batch * A * C : (size_t)max_batch * 1024;
        T_ALLOC(t->dA[0], amax); T_ALLOC(t->dA[1], amax);
        size_t pmax = (size_t)RED_S * 2 * 1024;
        if ((size_t)RED_S * 2 * C > pmax) pmax = (size_t)RED_S * 2 * C;
        if ((size_t)RED_S * 9 * in_channels * C > pmax) pmax = (size_t)RED_S * 9 * in_channels * C;
        T_ALLOC(t->partial, pmax);
        const int vmax = F > 8192 ? F : 8192;
        T_ALLOC(t->ones, vmax); T_ALLOC(t->zeros, vmax);
        std::vector<float> one(vmax, 1.0f);
        OZ_HIP(hipMemcpyAsync(t->ones, one.data(), vmax * sizeof(float), hipMemcpyHostToDevice, t->s));
        OZ_HIP(hipStreamSynchronize(t->s));
        for (int l = 1; l < 6; ++l) T_ALLOC(t->Wt[l], t->size[6 * l]);
        for (int l = 1; l < 4; ++l) T_ALLOC(t->Wd[l], t->size[6 * l]);
        // the inputs of a step live in ONE device block [own | opp | pi targets | z targets | count] mirrored by a pinned host block: the step-wise
        // oz_trainer_forward_backward uploads it with one copy (five copies were five blit launches, ~30 us, in front of every step)
        t->in_bytes = (size_t)max_batch * (8 + 8 + 4 * A + 4) + 16;
        T_ALLOC(t->d_in, t->in_bytes);
        OZ_HIP(hipHostMalloc((void**)&t->h_in, t->in_bytes, hipHostMallocDefault));
        t->d_own = reinterpret_cast<uint64_t*>(t->d_in);
        t->d_opp = t->d_own + max_batch;
        t->d_pit = reinterpret_cast<float*>(t->d_opp + max_batch);
        t->d_zt = t->d_pit + (size_t)max_batch * A;
        t->d_count = reinterpret_cast<int*>(t->d_zt + max_batch);
        T_ALLOC(t->p, (size_t)max_batch * A); T_ALLOC(t->v, max_batch); T_ALLOC(t->dlogit, (size_t)max_batch * A); T_ALLOC(t->dvpre, max_batch);
        T_ALLOC(t->loss, 2 * (size_t)max_batch); T_ALLOC(t->losses, 4);
        T_ALLOC(t->gpartial, t->gpartial_floats);
        T_ALLOC(t->wpartial, t->gpartial_floats);
        OZ_HIP(hipStreamCreateWithFlags(&t->s2, hipStreamNonBlocking));
        for (int l = 0; l < 6; ++l) OZ_HIP(hipEventCreateWithFlags(&t->ev_dz[l], hipEventDisableTiming));
        OZ_HIP(hipEventCreateWithFlags(&t->ev_w, hipEventDisableTiming));
        for (hipEvent_t* e : {&t->ev_pre, &t->ev_wt, &t->ev_wd, &t->ev_wl[1], &t->ev_wl[2], &t->ev_wl[3]}) OZ_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        for (int l = 0; l < 6; ++l) T_ALLOC(t->bnb2[l], (size_t)OZ_BNB_MAX_RB * t->L[l].Co);
        OZ_HIP(hipStreamSynchronize(t->s));
        return OZ_OK;
    }();
    if (rc) return fail(rc);
    *out = t;
    return OZ_OK;
}

OZ_API int oz_trainer_destroy(oz_trainer* t) { delete t; return OZ_OK; }

// sticky range flag of the f16x2 mode (an activation above the fp16 range): reported at the synchronising calls
static int t_check_range(oz_trainer* t) {
    if (t->mode != 1 || !t->h2flag) return OZ_OK;
    int f = 0;
    OZ_HIP(hipMemcpyAsync(&f, t->h2flag, sizeof(int), hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    if (f) {
        // reported once: the flag is cleared, so the trainer is usable again after set_weights reloads good weights (the step that raised it is invalid)
        OZ_HIP(hipMemsetAsync(t->h2flag, 0, sizeof(int), t->s));
        OZ_HIP(hipStreamSynchronize(t->s));
        if (f & 2) oz_set_error("a weight or gradient tensor holds Inf / NaN in the trainer's f16x2 mode (the optimisation diverged): the step is invalid");
        else oz_set_error("an activation exceeded the fp16 range (65504) in the trainer's f16x2 mode: the step is invalid; use precision 0 (f32)");
        return OZ_ERR_STATE;
    }
    return OZ_OK;
}

OZ_API int oz_trainer_set_policy_loss(oz_trainer* t, int mode) {
    OZ_REQUIRE(t && (mode == OZ_POLICY_LOSS_ROWS || mode == OZ_POLICY_LOSS_FLAT), "oz_trainer_set_policy_loss: mode 0 (rows) or 1 (flat)");
    T_LOCK(t);
    t->policy_loss = mode;              // read at the next launch of the heads kernel (stream order)
    return OZ_OK;
}

// the packed operands of one split mode (planes 16-bit planes per value: values x planes / 8 uint4 units); zeroed, and the dz border stays zero
static int t_alloc_packed(oz_trainer* t, TPacked& k, int planes) {
    const size_t C = t->C, Bmax = t->Bmax, noct = (Bmax + 7) / 8, wq = C * 9 * C * planes / 8;
    for (int l = 1; l < 4; ++l) {
        const TLayer& L = t->L[l];
        T_ALLOC(k.W[l], wq); T_ALLOC(k.Wd[l], wq);
        T_ALLOC(k.act[l - 1], Bmax * t->L[l - 1].P * C * planes / 8);
        T_ALLOC(k.dz[l], Bmax * L.Hz * L.Hz * C * planes / 8);
        T_ALLOC(k.xoct[l], noct * (L.Hout + 2) * WH_XW * planes * C);
        T_ALLOC(k.zoct[l], noct * L.Hout * WH_ZW * planes * C);
    }
    return OZ_OK;
}

OZ_API int oz_trainer_set_precision(oz_trainer* t, int mode) {
    OZ_REQUIRE(t && (mode == 0 || mode == 1 || mode == 2), "oz_trainer_set_precision: mode 0 (f32), 1 (f16x2) or 2 (bf16x3)");
    T_LOCK(t);
    OZ_REQUIRE(t->C % 256 == 0 || mode == 0, "oz_trainer_set_precision: %s needs channels %% 256 == 0 (got %d)", mode == 1 ? "f16x2" : "bf16x3", t->C);
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipStreamSynchronize(t->s));
    if (mode && !t->pk[mode - 1].W[1]) {
        if (int rc = t_alloc_packed(t, t->pk[mode - 1], mode + 1)) return rc;
        if (mode == 1) {
            for (int l = 1; l < 4; ++l) { T_ALLOC(t->wscale[l], t->C); T_ALLOC(t->dscale[l], t->C); }
            T_ALLOC(t->wmax, 4); T_ALLOC(t->dzmax, 8); T_ALLOC(t->h2flag, 1);
        }
        OZ_HIP(hipStreamSynchronize(t->s));
    }
    t->mode = mode;
    t->dirty = true;
    return OZ_OK;
}

OZ_API int oz_trainer_set_weight(oz_trainer* t, int index, const float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && index >= 0 && index < t->nw, "oz_trainer_set_weight: bad argument");
    T_LOCK(t);
    OZ_REQUIRE(nelem == t->size[index], "oz_trainer_set_weight: weight %d has %lld elements, got %lld", index, (long long)t->size[index], (long long)nelem);
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipMemcpyAsync(t->param(index), data, nelem * sizeof(float), hipMemcpyHostToDevice, t->s));
    if (t->opt.average_decay > 0.0 && t->toff[index] >= 0)      // the weight average of this array starts again from what was set
        OZ_HIP(hipMemcpyAsync(t->E + t->toff[index], data, nelem * sizeof(float), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    t->dirty = true;
    return OZ_OK;
}
OZ_API int oz_trainer_get_weight(oz_trainer* t, int index, float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && index >= 0 && index < t->nw && nelem == t->size[index], "oz_trainer_get_weight: bad argument");
    T_LOCK(t);
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipMemcpyAsync(data, t->param(index), nelem * sizeof(float), hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}
OZ_API int oz_trainer_get_grad(oz_trainer* t, int index, float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && index >= 0 && index < t->nw && nelem == t->size[index] && t->toff[index] >= 0, "oz_trainer_get_grad: bad argument");
    T_LOCK(t);
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipMemcpyAsync(data, t->grad(index), nelem * sizeof(float), hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}
OZ_API int oz_trainer_grad_arena(oz_trainer* t, void** device_ptr, int64_t* nelem) {
    OZ_REQUIRE(t && device_ptr && nelem, "oz_trainer_grad_arena: bad argument");
    T_LOCK(t);
    *device_ptr = t->G; *nelem = t->total;
    return OZ_OK;
}
OZ_API int oz_trainer_arena_size(int n, int channels, int in_channels, int64_t* nelem) {
    OZ_REQUIRE(nelem, "oz_trainer_arena_size: bad argument");
    int64_t size[40], toff[40];
    const int64_t tot = t_layout(n, channels, in_channels, size, toff);
    *nelem = tot;
    return OZ_OK;
}
OZ_API int oz_trainer_arena_size_aux(int n, int channels, int in_channels, int64_t* nelem) {
    OZ_REQUIRE(nelem, "oz_trainer_arena_size_aux: bad argument");
    int64_t size[44], toff[44];
    *nelem = t_layout(n, channels, in_channels, size, toff, true);
    return OZ_OK;
}

// ---------------------------------------------------------------- auxiliary heads: switching them on
// Glorot-uniform array of `count` floats from (seed, stream): limit sqrt(6 / (fan_in + fan_out)), the unit draws of oz_rng
static void t_glorot(std::vector<float>& w, int64_t count, int fan_in, int fan_out, uint64_t seed, uint64_t stream) {
    const double lim = sqrt(6.0 / (double)(fan_in + fan_out));
    w.resize((size_t)count);
    for (int64_t i = 0; i < count; ++i) w[(size_t)i] = (float)((2.0 * oz_rng_unit(oz_rng(seed, (uint64_t)i, stream, 0x617578ULL)) - 1.0) * lim);
}
OZ_API int oz_trainer_set_aux_heads(oz_trainer* t, float w_own, float w_score) {
    OZ_REQUIRE(t, "oz_trainer_set_aux_heads: NULL");
    OZ_REQUIRE(w_own >= 0.f && w_score >= 0.f && std::isfinite(w_own) && std::isfinite(w_score),
               "oz_trainer_set_aux_heads: weights (%g, %g) must be finite and >= 0", (double)w_own, (double)w_score);
    T_LOCK(t);
    if (t->ran || t->step > 0) { oz_set_error("oz_trainer_set_aux_heads: a step has run on this trainer (the heads are switched on before the first one)"); return OZ_ERR_STATE; }
    // (the library cannot see how large a caller's arena is, and the four gradients would be written behind a forty-array one)
    OZ_REQUIRE(t->own_grads, "oz_trainer_set_aux_heads: not offered for a trainer created on an external gradient arena (a data-parallel fit): the arena was sized for the forty arrays");
    OZ_HIP(hipSetDevice(t->device));
    if (t->aux) { t->w_own = w_own; t->w_sc = w_score; return OZ_OK; }      // (again before the first step: the weights alone)
    OZ_HIP(hipStreamSynchronize(t->s));
    const int64_t old_total = t->total, A = t->n * t->n;
    const int64_t total = t_layout(t->n, t->C, t->cin, t->size, t->toff, true);
    // the three (four, five) arenas grow by the aux arrays: new allocations, the forty's contents carried over, the old ones freed
    auto grow = [&](float*& arena) -> int {
        float* neu = nullptr;
        if (int rc = t_alloc(t, (void**)&neu, (size_t)t_arena_alloc(total) * sizeof(float))) return rc;
        OZ_HIP(hipMemcpyAsync(neu, arena, old_total * sizeof(float), hipMemcpyDeviceToDevice, t->s));
        OZ_HIP(hipStreamSynchronize(t->s));
        for (void*& q : t->allocs) if (q == (void*)arena) { q = t->allocs.back(); t->allocs.pop_back(); break; }
        hipFree(arena);
        arena = neu;
        return OZ_OK;
    };
    if (int rc = grow(t->P)) return rc;
    if (int rc = grow(t->M1)) return rc;
    if (int rc = grow(t->V2)) return rc;
    if (int rc = grow(t->G)) return rc;
    if (t->E) { if (int rc = grow(t->E)) return rc; }
    t->total = total; t->nw = 44; t->aux = true; t->w_own = w_own; t->w_sc = w_score;
    const size_t Bm = (size_t)t->Bmax;
    T_ALLOC(t->d_fin, 2 * Bm);
    OZ_HIP(hipHostMalloc((void**)&t->h_fin, 2 * Bm * sizeof(uint64_t), hipHostMallocDefault));
    T_ALLOC(t->ao, Bm * A); T_ALLOC(t->as, Bm); T_ALLOC(t->dopre, Bm * A); T_ALLOC(t->dspre, Bm); T_ALLOC(t->aux_loss, 2 * Bm); T_ALLOC(t->aux_losses, 2);
    if (t->capture) T_ALLOC(t->cap_f2, Bm * 512);
    std::vector<float> w;
    t_glorot(w, 512 * A, 512, (int)A, t->seed, 40);
    OZ_HIP(hipMemcpyAsync(t->param(40), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, t->s));
    if (t->E) OZ_HIP(hipMemcpyAsync(t->E + t->toff[40], w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    t_glorot(w, 512, 512, 1, t->seed, 42);
    OZ_HIP(hipMemcpyAsync(t->param(42), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, t->s));
    if (t->E) OZ_HIP(hipMemcpyAsync(t->E + t->toff[42], w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    t_opt_tables(t);
    return OZ_OK;
}
OZ_API int oz_trainer_get_aux_heads(oz_trainer* t, int* on, float* w_own, float* w_score) {
    OZ_REQUIRE(t && on && w_own && w_score, "oz_trainer_get_aux_heads: bad argument");
    T_LOCK(t);
    *on = t->aux ? 1 : 0; *w_own = t->w_own; *w_score = t->w_sc;
    return OZ_OK;
}
OZ_API int oz_trainer_sync(oz_trainer* t) {
    OZ_REQUIRE(t, "oz_trainer_sync: NULL");
    T_LOCK(t);
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}
OZ_API int oz_trainer_step_count(oz_trainer* t, int64_t* step) {
    OZ_REQUIRE(t && step, "oz_trainer_step_count: bad argument");
    T_LOCK(t);
    *step = t->step;
    return OZ_OK;
}

// The weights changed (optimiser step, set_weight): rebuild the GEMM operands derived from them.  The launches run on the SECOND stream,
// after everything already queued on the main stream (the optimiser step that wrote the weights, the previous step's readers of Wt / Wd),
// and the main stream only waits where it first needs them -- the forward operands before conv2's GEMM, the data-gradient operands before
// conv4's dgrad -- so the uploads, conv1 and its BN run beside them instead of behind them (~70 us of a 1.4 ms step at batch 32).
static int t_refresh(oz_trainer* t) {
    const int C = t->C;
    hipStream_t r = t->s2;
    OZ_HIP(hipEventRecord(t->ev_pre, t->s));
    OZ_HIP(hipStreamWaitEvent(r, t->ev_pre, 0));
    const TPacked* k = t->mode ? &t->pk[t->mode - 1] : nullptr;
    const unsigned wd_blocks = (unsigned)(((long long)C * (9 * C / 8) + 255) / 256);      // one thread per (row, group of 8 k') of a packed 3x3 operand
    if (t->mode == 1) {  // f16x2: per-tensor maxima -> power-of-two scales (the forward operands below, the data-gradient operands further down)
        OZ_HIP(hipMemsetAsync(t->wmax, 0, 3 * sizeof(unsigned), r));
        AbsMaxArgs am;
        for (int l = 1; l < 4; ++l) { am.p[l - 1] = t->param(6 * l); am.n[l - 1] = 9LL * C * C; }
        hipLaunchKernelGGL(k_t_absmax, dim3(192, 3), dim3(256), 0, r, am, t->wmax);      // (12 x 16-byte loads per thread cover 9 x 512 x 512 floats in one trip)
    }
    // forward operands: the packed ones of conv2..4 straight from the masters, each with its own event -- conv2's GEMM waits for ITS operand only
    // (round 5: it waited for all five forward operands, 64 us of an idle main stream per step) -- then the fp32 ones (the dense layers; the 3x3
    // layers too in f32 mode)
    for (int l = 1; k && l < 4; ++l) {
        if (t->mode == 1)
            hipLaunchKernelGGL(k_t_w_to_h2<0>, dim3(wd_blocks), dim3(256), 0, r, t->param(6 * l), C, C, t->wmax + (l - 1), k->W[l], t->wscale[l], t->h2flag);
        else if (int rc = oz_w_to_b3_launch(t->param(6 * l), 9 * C, C, 9, k->W[l], r)) return rc;
        OZ_HIP(hipEventRecord(t->ev_wl[l], r));
        t->wait_wl[l] = true;
    }
    OZ_HIP(hipGetLastError());
    for (int l = k ? 4 : 1; l < 6; ++l) {
        const int K = t->L[l].taps * t->L[l].Cin, N = t->L[l].Co;
        hipLaunchKernelGGL(k_t_transpose, dim3((N + 31) / 32, (K + 31) / 32), dim3(256), 0, r, t->param(6 * l), K, N, t->Wt[l]);
        OZ_HIP(hipGetLastError());
    }
    OZ_HIP(hipEventRecord(t->ev_wt, r));
    for (int l = 1; l < 4; ++l) {      // data-gradient operands of the 3x3 layers
        switch (t->mode) {
        case 1: hipLaunchKernelGGL(k_t_w_to_h2<1>, dim3(wd_blocks), dim3(256), 0, r, t->param(6 * l), C, C, t->wmax + (l - 1), k->Wd[l], (float*)nullptr, t->h2flag); break;
        case 2: hipLaunchKernelGGL(k_t_w_to_b3, dim3(wd_blocks), dim3(256), 0, r, t->param(6 * l), C, C, k->Wd[l]); break;
        default: hipLaunchKernelGGL(k_t_dgrad_operand, dim3((unsigned)((9LL * C * C + 255) / 256)), dim3(256), 0, r, t->param(6 * l), C, C, t->Wd[l]);
        }
        OZ_HIP(hipGetLastError());
    }
    OZ_HIP(hipEventRecord(t->ev_wd, r));
    t->wait_wt = t->wait_wd = true;
    t->dirty = false;
    return OZ_OK;
}

// the plan row of layer l = 0 .. 5 (conv1 has the last row: the rows of the GEMM layers keep their places)
static int* t_plan_row(oz_trainer* t, int l) { return t->plan[l ? l - 1 : OZ_TRAINER_PLAN_ROWS - 1]; }

template <int MODE>
static int t_reduce(oz_trainer* t, RedArgs r) {
    hipLaunchKernelGGL(k_t_colreduce<MODE>, dim3((r.C / 4 + 63) / 64, RED_S), dim3(256), 0, t->s, r, t->d_count, t->partial);
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// BN (training mode) + ReLU (+ dropout) of layer l: z[l] -> a[l]
static int t_bn_forward(oz_trainer* t, int l, int B) {
    const int Cc = t->L[l].Co, P = t->L[l].P;
    int& regime = t_plan_row(t, l)[OZ_TRAINER_PLAN_BN_FWD];
    if ((long long)B * P <= OZ_BN_FUSED_MAX_ROWS) {      // small batch: the whole layer in one launch (oz_train_fused.h)
        regime = (long long)B * P <= 32 * OZ_BN_RL ? OZ_TRAINER_BN_FWD_FUSED32 : OZ_TRAINER_BN_FWD_FUSED64;
        if ((long long)B * P <= 32 * OZ_BN_RL)
            hipLaunchKernelGGL(k_t_bn_fwd_fused<32>, dim3(Cc / OZ_BN_COLS), dim3(1024), 0, t->s, t->z[l], t->a[l], t->d_count, P, Cc, t->param(6 * l + 2),
                               t->param(6 * l + 3), t->mean[l], t->rstd[l], t->stats[6 * l + 4], t->stats[6 * l + 5], t->stats_new[6 * l + 4],
                               t->stats_new[6 * l + 5], t->mom, l < 4 ? 1 : 0, l >= 4 ? t->rate : 0.f, t->seed, (uint64_t)t->step, l - 4);
        else
            hipLaunchKernelGGL(k_t_bn_fwd_fused<64>, dim3(Cc / OZ_BN_COLS), dim3(1024), 0, t->s, t->z[l], t->a[l], t->d_count, P, Cc, t->param(6 * l + 2),
                               t->param(6 * l + 3), t->mean[l], t->rstd[l], t->stats[6 * l + 4], t->stats[6 * l + 5], t->stats_new[6 * l + 4],
                               t->stats_new[6 * l + 5], t->mom, l < 4 ? 1 : 0, l >= 4 ? t->rate : 0.f, t->seed, (uint64_t)t->step, l - 4);
        OZ_HIP(hipGetLastError());
        return OZ_OK;
    }
    regime = OZ_TRAINER_BN_FWD_STREAM;
    RedArgs r = {}; r.x = t->z[l]; r.P = P; r.C = Cc;
    if (int rc = t_reduce<0>(t, r)) return rc;
    hipLaunchKernelGGL(k_t_fin_mean, dim3((Cc + 255) / 256), dim3(256), 0, t->s, t->partial, t->d_count, P, Cc, t->mean[l]);
    r.mean = t->mean[l];
    if (int rc = t_reduce<1>(t, r)) return rc;
    hipLaunchKernelGGL(k_t_fin_var, dim3((Cc + 255) / 256), dim3(256), 0, t->s, t->partial, t->d_count, P, Cc, t->mean[l], t->rstd[l],
                       t->stats[6 * l + 4], t->stats[6 * l + 5], t->stats_new[6 * l + 4], t->stats_new[6 * l + 5], t->mom, l < 4 ? 1 : 0);
    const long long total = (long long)B * P * Cc;
    hipLaunchKernelGGL(k_t_bn_fwd, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, t->s, t->z[l], t->mean[l], t->rstd[l], t->param(6 * l + 2),
                       t->param(6 * l + 3), t->a[l], t->d_count, P, Cc, l >= 4 ? t->rate : 0.f, t->seed, (uint64_t)t->step, l - 4);
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// BN (inference mode: the moving statistics) + ReLU of layer l: z[l] -> a[l], nothing else written
static int t_bn_infer(oz_trainer* t, int l, int B) {
    const int Cc = t->L[l].Co, P = t->L[l].P;
    const long long total = (long long)B * P * Cc;
    hipLaunchKernelGGL(k_t_bn_infer, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, t->s, t->z[l], t->stats[6 * l + 4], t->stats[6 * l + 5],
                       t->param(6 * l + 2), t->param(6 * l + 3), t->a[l], t->d_count, P, Cc);
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// the main stream waits for an operand of t_refresh where it first reads it, once per refresh
static int t_wait_once(hipStream_t s, hipEvent_t e, bool& pending) {
    if (pending) { OZ_HIP(hipStreamWaitEvent(s, e, 0)); pending = false; }
    return OZ_OK;
}

// The pieces of a step.  Everything is enqueued on the trainer's two streams, nothing is waited for on the host.  The data-gradient chain (BN
// backward -> dgrad -> BN backward of the layer below -> ...) stays on the main stream; what only needs a[l - 1] and dz[l] -- the weight gradient
// and the bias gradient's last sum -- runs on the second stream behind ev_dz[l], beside the chain, whose small-batch launches leave most CUs idle.

// forward: boards -> conv1 .. fc2 (each with its BN) -> heads and losses.  infer (held-out evaluation): the same conv1 and GEMM launches, the BN
// on the moving statistics without dropout (k_t_bn_infer), and k_t_eval_heads (metrics rows, no gradients) at the end
static int t_forward(oz_trainer* t, int B, bool infer = false) {
    hipStream_t s = t->s;
    const int n = t->n, C = t->C, A = n * n;
    const long long tot = (long long)B * A * (C / 4);
    hipLaunchKernelGGL(k_t_conv1_fwd, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, t->d_own, t->d_opp, t->d_count, n, C, t->cin,
                       t->param(0), t->param(1), t->z[0]);
    OZ_HIP(hipGetLastError());
    if (int rc = infer ? t_bn_infer(t, 0, B) : t_bn_forward(t, 0, B)) return rc;
    for (int l = 1; l < 6; ++l) {
        const TLayer& L = t->L[l];
        const int Pin = t->L[l - 1].P;
        switch (l < 4 ? t->mode : 0) {      // the 3x3 layers of a split mode: the previous layer's activation in the packed layout, then the GEMM on the 16-bit matrix cores
        case 0:
            if (int rc = t_wait_once(s, t->ev_wt, t->wait_wt)) return rc;          // the first fp32 operand of the step: conv2's, or fc1's in a split mode
            if (int rc = oz_gemm_f32_launch(t->a[l - 1], t->Wt[l], t->ones, t->param(6 * l + 1), t->z[l], t->d_count, B, L.Hin, L.Hout, L.pad,
                                            L.Cin, L.taps, L.Co, 0, s, t->gpartial, t->gpartial_floats, 0, 0, -1, nullptr, 0, nullptr,
                                            &t->plan[l - 1][OZ_TRAINER_PLAN_FWD_KSLICES])) return rc;
            break;
        case 1: {
            const TPacked& k = t->pk[0];
            const long long thr = (long long)B * Pin * (C / 8);
            hipLaunchKernelGGL(k_t_act_to_h2, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, s, t->a[l - 1], t->d_count, Pin, C, k.act[l - 1], t->h2flag);
            if (int rc = t_wait_once(s, t->ev_wl[l], t->wait_wl[l])) return rc;
            if (int rc = oz_gemm_h2_launch(k.act[l - 1], k.W[l], t->wscale[l], t->param(6 * l + 1), t->z[l], t->d_count, B, L.Hin, L.Hout, L.pad,
                                           L.Cin, 9, L.Co, s, t->gpartial, t->gpartial_floats, t->zeros, t->h2flag, &t->plan[l - 1][OZ_TRAINER_PLAN_FWD_KSLICES])) return rc;
            break;
        }
        case 2: {        // (z is pre-BN: no ReLU)
            const TPacked& k = t->pk[1];
            if (int rc = oz_f32_to_b3_launch(t->a[l - 1], t->d_count, t->Bmax, Pin, C, k.act[l - 1], s)) return rc;
            if (int rc = t_wait_once(s, t->ev_wl[l], t->wait_wl[l])) return rc;
            if (int rc = oz_gemm_b3_launch(k.act[l - 1], k.W[l], t->ones, t->param(6 * l + 1), t->z[l], t->d_count, t->Bmax, L.Hin, L.Hout, L.pad,
                                           L.Cin, 9, L.Co, 0, s, t->gpartial, t->gpartial_floats, t->zeros, 0, &t->plan[l - 1][OZ_TRAINER_PLAN_FWD_KSLICES])) return rc;
        }
        }
        if (int rc = infer ? t_bn_infer(t, l, B) : t_bn_forward(t, l, B)) return rc;
    }
    if (infer) {
        hipLaunchKernelGGL(k_t_eval_heads, dim3(B), dim3(64), 0, s, t->a[5], t->d_count, n, t->policy_loss, t->param(36), t->param(37), t->param(38),
                           t->param(39), t->d_pit, t->d_zt, t->p, t->v, t->ev_rows);
        OZ_HIP(hipGetLastError());
        return OZ_OK;
    }
    hipLaunchKernelGGL(k_t_heads, dim3(B), dim3(64), 0, s, t->a[5], t->d_count, n, t->policy_loss, t->param(36), t->param(37), t->param(38), t->param(39),
                       t->d_pit, t->d_zt, t->p, t->v, t->dlogit, t->dvpre, t->loss);
    if (t->aux)
        hipLaunchKernelGGL(k_t_aux_heads, dim3(B), dim3(64), 0, s, t->a[5], t->d_count, n, t->param(40), t->param(41), t->param(42), t->param(43),
                           t->d_fin, t->d_fin + t->Bmax, t->w_own, t->w_sc, t->ao, t->as, t->dopre, t->dspre, t->aux_loss);
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// capture on: the live rows of dA (the gradient wrt a[l], B boards) are copied to cap[l] behind the launch that wrote them, on the main stream
static int t_capture(oz_trainer* t, int l, int B, const float* dA) {
    if (!t->capture) return OZ_OK;
    OZ_HIP(hipMemcpyAsync(t->cap[l], dA, (size_t)B * t->L[l].P * t->L[l].Co * sizeof(float), hipMemcpyDeviceToDevice, t->s));
    return OZ_OK;
}

// heads backward: their weight and bias gradients, the batch-mean losses, dA = the gradient wrt a[5]
static int t_heads_backward(oz_trainer* t, int B, float* dA) {
    hipStream_t s = t->s;
    const int A = t->n * t->n;
    // one head pair: arrays p .. p + 3 of the arena are its W[512][A], b[A], w[512], b[1]; dcol / dsc the gradients wrt its pre-activations.
    // aux: the second pair adds into dA and leaves the losses and the |dz| maxima to the first
    auto pair_backward = [&](int p, const float* dcol, const float* dsc, bool aux) {
        hipLaunchKernelGGL(k_t_heads_wgrad, dim3(512), dim3(128), 0, s, t->a[5], dcol, dsc, t->d_count, A, t->grad(p), t->grad(p + 2));
        hipLaunchKernelGGL(k_t_heads_bias, dim3(1), dim3(128), 0, s, dcol, dsc, aux ? (const float*)nullptr : t->loss, t->d_count, A, t->grad(p + 1),
                           t->grad(p + 3), aux ? (float*)nullptr : t->losses, !aux && t->mode == 1 ? t->dzmax : (unsigned*)nullptr);
        hipLaunchKernelGGL(k_t_heads_dgrad, dim3((unsigned)(((long long)B * 512 + 255) / 256)), dim3(256), 0, s, dcol, dsc, t->param(p), t->param(p + 2),
                           t->d_count, A, (int)aux, dA);
    };
    pair_backward(36, t->dlogit, t->dvpre, false);
    OZ_HIP(hipGetLastError());
    if (!t->aux) return t_capture(t, 5, B, dA);
    // auxiliary heads: their batch-mean losses behind k_t_heads_bias (whose total they join); with a weight on, their weight and bias gradients
    // and their term of dA behind k_t_heads_dgrad.  Both weights 0: nothing more is launched (adding a signed zero into dA would change bits)
    hipLaunchKernelGGL(k_t_aux_losses, dim3(1), dim3(64), 0, s, t->aux_loss, t->d_count, t->w_own, t->w_sc, t->aux_losses, t->losses);
    if (t->w_own > 0.f || t->w_sc > 0.f) {
        if (t->capture) OZ_HIP(hipMemcpyAsync(t->cap_f2, dA, (size_t)B * 512 * sizeof(float), hipMemcpyDeviceToDevice, s));
        pair_backward(40, t->dopre, t->dspre, true);
    }
    OZ_HIP(hipGetLastError());
    return t_capture(t, 5, B, dA);
}

// BN backward of layer l: dA (the gradient wrt a[l]) -> dz[l], the gradients of gamma, beta and the bias; f16x2 also leaves max |dz[l]| in dzmax[l]
static int t_bn_backward(oz_trainer* t, int l, int B, const float* dA) {
    hipStream_t s = t->s;
    const TLayer& L = t->L[l];
    const int Cc = L.Co;
    const long long M = (long long)B * L.P;
    const float post = l >= 4 && t->rate > 0.f ? 1.0f / (1.0f - t->rate) : 1.0f;
    unsigned* dzmax = t->mode == 1 ? t->dzmax + l : nullptr;
    int* const plan = t_plan_row(t, l);
    if (M <= OZ_BNB_MIN_ROWS) {         // small batch: BN backward, dgamma / dbeta / bias gradient in one launch
        plan[OZ_TRAINER_PLAN_BN_BWD] = OZ_TRAINER_BN_BWD_FUSED; plan[OZ_TRAINER_PLAN_BN_BWD_RS] = 1;
        hipLaunchKernelGGL(k_t_bn_bwd_fused, dim3(Cc / OZ_BN_COLS), dim3(1024), 0, s, dA, t->a[l], t->z[l], t->rstd[l],
                           t->param(6 * l + 2), post, t->d_count, L.Hout, Cc, L.Hz, L.zoff, t->dz[l], t->grad(6 * l + 2),
                           t->grad(6 * l + 3), t->grad(6 * l + 1), dzmax);
        OZ_HIP(hipGetLastError());
        return OZ_OK;
    }
    // partial sums over row splits, then one launch that finishes the sums and writes dz (oz_train_fused.h)
    const int Q = Cc / 4, lpr = Q < 64 ? Q : 64, rpp = 256 / lpr;
    int RS = 16; while (RS < OZ_BNB_MAX_RB && M > (long long)RS * rpp * 8) RS *= 2;          // ~8 rows per thread
    plan[OZ_TRAINER_PLAN_BN_BWD] = OZ_TRAINER_BN_BWD_SPLIT; plan[OZ_TRAINER_PLAN_BN_BWD_RS] = RS;
    RedArgs r = {}; r.x = dA; r.a = t->a[l]; r.z = t->z[l]; r.mean = t->mean[l]; r.rstd = t->rstd[l]; r.post_scale = post; r.P = L.P; r.C = Cc;
    hipLaunchKernelGGL(k_t_colreduce<2>, dim3((Q + 63) / 64, RS), dim3(256), 0, s, r, t->d_count, t->partial);
    hipLaunchKernelGGL(k_t_bnb_apply, dim3((Q + 63) / 64, RS), dim3(256), 0, s, dA, t->a[l], t->z[l], t->mean[l], t->rstd[l], t->param(6 * l + 2),
                       post, t->d_count, L.Hout, Cc, L.Hz, L.zoff, t->partial, RS, t->dz[l], t->grad(6 * l + 2), t->grad(6 * l + 3), t->bnb2[l], dzmax);
    // the bias gradient (column sums of dz) is off the dgrad chain: finished beside it (conv1 has no chain below it: on the main stream)
    hipStream_t sb = s;
    if (l > 0) {
        OZ_HIP(hipEventRecord(t->ev_dz[l], s));
        OZ_HIP(hipStreamWaitEvent(t->s2, t->ev_dz[l], 0));
        sb = t->s2;
    }
    hipLaunchKernelGGL(k_t_sum_partials, dim3((unsigned)((Cc + 255) / 256)), dim3(256), 0, sb, t->bnb2[l], RS, (long long)Cc, t->grad(6 * l + 1));
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// weight gradient of conv1 (its input is the bitboards): on the main stream, nothing runs beside it
static int t_wgrad_conv1(oz_trainer* t, int B) {
    hipStream_t s = t->s;
    const int n = t->n, C = t->C;
    int S1 = 8;                                    // row splits: ~16 rows per thread (each a dependent ~1 us load at small batch), at most RED_S (the partial buffer's capacity)
    while (S1 < RED_S && (long long)B * n * n > 16LL * S1) S1 *= 2;
    t_plan_row(t, 0)[OZ_TRAINER_PLAN_CONV1_S1] = S1;
    if (n == 8) hipLaunchKernelGGL(k_t_conv1_wgrad<8>, dim3((C + 255) / 256, S1), dim3(256), 0, s, t->d_own, t->d_opp, t->d_count, C, t->cin, t->dz[0], t->partial, S1);
    else hipLaunchKernelGGL(k_t_conv1_wgrad<6>, dim3((C + 255) / 256, S1), dim3(256), 0, s, t->d_own, t->d_opp, t->d_count, C, t->cin, t->dz[0], t->partial, S1);
    const long long cnt = 9LL * t->cin * C;
    hipLaunchKernelGGL(k_t_sum_partials, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, t->partial, S1, cnt, t->grad(0));
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// the octet-image weight gradient of 3x3 layer l on stream sw: octet images of a[l - 1] and dz[l], then k_wgrad_h2 (two planes of the scaled dz
// on the fp16 matrix cores) or k_wgrad_b3 (three planes on the bf16 matrix cores); returns the number of slabs left in wp
template <typename T>
static int t_wgrad_oct(oz_trainer* t, int l, int B, hipStream_t sw, float* wp, int& msplit) {
    const TLayer& L = t->L[l];
    const TPacked& k = t->pk[T::PLANES - 2];
    const unsigned* dzmax = T::SCALED ? t->dzmax + l : nullptr;
    int* flag = T::SCALED ? t->h2flag : nullptr;
    const int noct = (B + 7) / 8, XR = L.Hout + 2, tiles = (L.Cin / T::CI) * (L.Co / T::CO), lds = WgradLds<T>::BYTES;
    const long long wcount = 9LL * L.Cin * L.Co;
    msplit = 1;
    while (msplit < 32 && tiles * msplit < 256 && msplit * 2 <= noct && wcount * msplit * 2 <= t->gpartial_floats) msplit *= 2;
    const long long xthr = (long long)noct * XR * WH_XW * (L.Cin / 4), zthr = (long long)noct * L.Hout * WH_ZW * (L.Co / 4);
    hipLaunchKernelGGL(k_t_x_octets<T::PLANES>, dim3((unsigned)((xthr + 255) / 256)), dim3(256), 0, sw, t->a[l - 1], t->d_count, L.Hin, L.pad, L.Cin, k.xoct[l]);
    hipLaunchKernelGGL(k_t_z_octets<T::PLANES>, dim3((unsigned)((zthr + 255) / 256)), dim3(256), 0, sw, t->dz[l], t->d_count, L.Hout, L.Hz, L.zoff, L.Co,
                       dzmax, k.zoct[l], flag);
    const WhGeom wg = {XR, L.Hout, L.Cin, L.Co};
    if constexpr (T::SCALED) {
        if (int rc = set_max_lds_once<k_wgrad_h2>(lds)) return rc;
        hipLaunchKernelGGL(k_wgrad_h2, dim3(tiles, msplit), dim3(512), lds, sw, k.xoct[l], k.zoct[l], t->d_count, wg, dzmax, t->grad(6 * l), msplit, wp, wcount);
    } else {
        if (int rc = set_max_lds_once<k_wgrad_b3>(lds)) return rc;
        hipLaunchKernelGGL(k_wgrad_b3, dim3(tiles, msplit), dim3(512), lds, sw, k.xoct[l], k.zoct[l], t->d_count, wg, t->grad(6 * l), msplit, wp, wcount);
    }
    return OZ_OK;
}

// weight gradient of layer l = 1 .. 5 from a[l - 1] and dz[l], on the second stream
static int t_wgrad(oz_trainer* t, int l, int B) {
    const TLayer& L = t->L[l];
    hipStream_t sw = t->s2;
    float* wp = t->wpartial;
    OZ_HIP(hipEventRecord(t->ev_dz[l], t->s));
    OZ_HIP(hipStreamWaitEvent(sw, t->ev_dz[l], 0));
    const long long wcount = (long long)L.taps * L.Cin * L.Co;
    // The kernel of the launch.  Dense layers: the tap-per-block fp32 kernel.  3x3 layers: bf16x3 always takes k_wgrad_b3 (no fallback rule); f16x2
    // takes k_wgrad_h2 from WH_MIN_BATCH boards on; otherwise the board-resident fp32 kernel from 192 boards on, the tap-per-block one below
    // (measured on one MI355X, 8x8 / 512 filters: the board-resident kernel wins from batch 256 on -- 6.01 vs 6.36 ms per step, 17.0 vs
    //  19.9 at 1024 -- and loses 3-4 % at 32 .. 128, where the tap-per-block kernel's 144 x 4 short blocks finish sooner)
    enum { TAPS_F32, BOARDS_F32, OCT_H2, OCT_B3 } kernel = TAPS_F32;
    if (L.taps == 9) {
        if (t->mode == 2) kernel = OCT_B3;
        else if (t->mode == 1 && B >= WH_MIN_BATCH && L.Cin % WgradH2::CI == 0 && L.Co % WgradH2::CO == 0) kernel = OCT_H2;
        else if (B >= 192 && L.Cin % WC_CI == 0 && L.Co % WC_CO == 0) kernel = BOARDS_F32;
    }
    int msplit = 1;
    switch (kernel) {
    case OCT_B3: if (int rc = t_wgrad_oct<WgradB3>(t, l, B, sw, wp, msplit)) return rc; break;
    case OCT_H2: if (int rc = t_wgrad_oct<WgradH2>(t, l, B, sw, wp, msplit)) return rc; break;
    case BOARDS_F32: {
        // board-resident kernel: (Cin / 64) x (Cout / 128) tiles, boards split over blockIdx.y until every CU has a block
        const WconvGeom cg = {L.Hin, L.Hout, L.pad, L.Cin, L.Co, L.Hz, L.zoff};
        const int tiles = (L.Cin / WC_CI) * (L.Co / WC_CO);
        while (msplit < 16 && tiles * msplit < 256 && msplit * 2 <= B && wcount * msplit * 2 <= t->gpartial_floats) msplit *= 2;
        const int XW = L.Hin + 2 * L.pad;
        const size_t lds_bytes = 2 * sizeof(float) * ((size_t)XW * XW * WC_CI + (size_t)L.P * WC_CO);
        if (int rc = set_max_lds_once<k_wgrad_conv>(160 * 1024 - 1024)) return rc;
        hipLaunchKernelGGL(k_wgrad_conv, dim3(tiles, msplit), dim3(512), lds_bytes, sw, t->a[l - 1], t->dz[l], t->d_count, cg, t->grad(6 * l), msplit, wp, wcount);
        break;
    }
    case TAPS_F32: {
        const WgradGeom g = {L.Hin, L.Hout, L.pad, L.Cin, L.Co, L.taps, L.Hz, L.zoff};
        const int wblocks = L.taps * (L.Cin / 128) * (L.Co / 128);
        const long long wtiles = ((long long)B * L.P + 31) / 32;
        while (msplit < 16 && wblocks * msplit < 512 && wtiles / (msplit * 2) >= 8 && wcount * msplit * 2 <= t->gpartial_floats) msplit *= 2;
        // (round 5, measured and removed: 3 splits instead of 4 so that 144 tiles x splits stays below 512 blocks -- the launch got SLOWER, 147 -> 227 us on
        //  conv2: more than two of these 40 KB-LDS blocks share a CU, 576 blocks are one round)
        hipLaunchKernelGGL(k_wgrad_f32, dim3(wblocks, msplit), dim3(256), 0, sw, t->a[l - 1], t->dz[l], t->d_count, g, t->grad(6 * l), msplit, wp, wcount);
    }
    }
    t->plan[l - 1][OZ_TRAINER_PLAN_WGRAD_KERNEL] = kernel == TAPS_F32 ? OZ_TRAINER_WGRAD_TAPS_F32 : kernel == BOARDS_F32 ? OZ_TRAINER_WGRAD_BOARDS_F32
                                                 : kernel == OCT_H2 ? OZ_TRAINER_WGRAD_OCT_H2 : OZ_TRAINER_WGRAD_OCT_B3;
    t->plan[l - 1][OZ_TRAINER_PLAN_WGRAD_MSPLIT] = msplit;
    if (msplit > 1)
        hipLaunchKernelGGL(k_t_sum_partials, dim3((unsigned)((wcount + 255) / 256)), dim3(256), 0, sw, wp, msplit, wcount, t->grad(6 * l));
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// data gradient of layer l = 1 .. 5: dz[l] -> dA = the gradient wrt a[l - 1]
static int t_dgrad_launch(oz_trainer* t, int l, int B, float* dA) {
    hipStream_t s = t->s;
    const TLayer& L = t->L[l];
    int* const plan = &t->plan[l - 1][OZ_TRAINER_PLAN_DGRAD_KSLICES];      // [0] k-slices, [1] kernel: what the launchers report
    if (l >= 4)            // dense: dX = dZ . W^T; the Keras kernel [in][out] already is the [N = in][K = out] operand
        return oz_gemm_f32_launch(t->dz[l], t->param(6 * l), t->ones, t->zeros, dA, t->d_count, B, 1, 1, 0, L.Co, 1, L.Cin, 0, s, t->gpartial, t->gpartial_floats,
                                  0, 0, -1, nullptr, 0, nullptr, plan);
    // 3x3 conv: conv of dz (zero-bordered for 'valid' layers) with the reversed, channel-swapped taps
    const int same = L.pad ? 1 : 0;
    if (int rc = t_wait_once(s, t->ev_wd, t->wait_wd)) return rc;
    switch (t->mode) {
    case 2: {              // bf16x3: dz in the b3 layout, same zero-bordered geometry, unscaled
        const TPacked& k = t->pk[1];
        const long long thr = (long long)B * L.P * (L.Co / 8);
        hipLaunchKernelGGL(k_t_dz_to_b3, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, s, t->dz[l], t->d_count, L.Hout, L.Hz, L.zoff, L.Co, k.dz[l]);
        return oz_gemm_b3_launch(k.dz[l], k.Wd[l], t->ones, t->zeros, dA, t->d_count, t->Bmax, L.Hz, L.Hin, same, L.Co, 9, L.Cin, 0, s, t->gpartial,
                                 t->gpartial_floats, t->zeros, 1, plan);
    }
    case 1: {              // f16x2: dz scaled into the fp16 range by its own maximum, h2 layout, same zero-bordered geometry
        const TPacked& k = t->pk[0];
        long long thr = (long long)B * L.P * (L.Co / 8);
        if (thr < L.Cin) thr = L.Cin;                      // (the kernel's first Cin threads also write dscale)
        hipLaunchKernelGGL(k_t_dz_to_h2, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, s, t->dz[l], t->d_count, L.Hout, L.Hz, L.zoff, L.Co,
                           t->dzmax + l, t->wmax + (l - 1), k.dz[l], t->dscale[l], L.Cin, t->h2flag);
        return oz_gemm_h2_launch(k.dz[l], k.Wd[l], t->dscale[l], t->zeros, dA, t->d_count, B, L.Hz, L.Hin, same, L.Co, 9, L.Cin, s, t->gpartial,
                                 t->gpartial_floats, t->zeros, t->h2flag, plan);
    }
    default:               // (the non-zero core of the zero-bordered dz buffer: taps that only read the border are skipped at large batch)
        return oz_gemm_f32_launch(t->dz[l], t->Wd[l], t->ones, t->zeros, dA, t->d_count, B, L.Hz, L.Hin, same, L.Co, 9, L.Cin, 0, s, t->gpartial,
                                  t->gpartial_floats, 0, L.zoff, L.zoff + L.Hout, nullptr, 0, nullptr, plan);
    }
}
static int t_dgrad(oz_trainer* t, int l, int B, float* dA) {
    if (int rc = t_dgrad_launch(t, l, B, dA)) return rc;
    t->plan[l - 1][OZ_TRAINER_PLAN_DGRAD_TAP_SKIP] = t->plan[l - 1][OZ_TRAINER_PLAN_DGRAD_KERNEL] == OZ_NET_KERNEL_F32_STD_PIXMAJOR;
    return t_capture(t, l - 1, B, dA);
}

// forward + backward of the batch staged in d_own / d_opp / d_pit / d_zt / d_count (B boards): gradients land in the arena, the batch-mean
// losses in t->losses
static int t_forward_backward_async(oz_trainer* t, int B) {
    if (t->dirty) if (int rc = t_refresh(t)) return rc;
    if (int rc = t_forward(t, B)) return rc;
    int cur = 1;                                   // dA[cur] = gradient wrt a[l]
    if (int rc = t_heads_backward(t, B, t->dA[cur])) return rc;
    for (int l = 5; l >= 0; --l) {
        if (int rc = t_bn_backward(t, l, B, t->dA[cur])) return rc;
        if (l == 0) { if (int rc = t_wgrad_conv1(t, B)) return rc; break; }
        if (int rc = t_wgrad(t, l, B)) return rc;
        if (int rc = t_dgrad(t, l, B, t->dA[cur ^ 1])) return rc;
        cur ^= 1;
    }
    OZ_HIP(hipEventRecord(t->ev_w, t->s2));        // every gradient is complete before the caller (Adam, all-reduce, get_grad) sees the arena
    OZ_HIP(hipStreamWaitEvent(t->s, t->ev_w, 0));
    t->cap_valid = t->capture;
    t->ran = true;
    return OZ_OK;
}

// the staged batch's final pairs of a trainer with the auxiliary heads, from the host (fin_own == NULL: every mask 0), on the main stream
static int t_stage_fin(oz_trainer* t, const uint64_t* fin_own, const uint64_t* fin_opp, int B) {
    if (!fin_own) { OZ_HIP(hipMemsetAsync(t->d_fin, 0, 2 * (size_t)t->Bmax * sizeof(uint64_t), t->s)); return OZ_OK; }
    memcpy(t->h_fin, fin_own, B * sizeof(uint64_t));
    memcpy(t->h_fin + t->Bmax, fin_opp, B * sizeof(uint64_t));
    OZ_HIP(hipMemcpyAsync(t->d_fin, t->h_fin, 2 * (size_t)t->Bmax * sizeof(uint64_t), hipMemcpyHostToDevice, t->s));
    return OZ_OK;
}

// losses: {total, policy, value} and, aux5, {ownership, score} behind them
static int t_forward_backward_host(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target,
                                   const uint64_t* fin_own, const uint64_t* fin_opp, int B, float* losses3, bool aux5) {
    OZ_REQUIRE(B >= 1 && B <= t->Bmax, "oz_trainer_forward_backward: batch %d outside [1, %d]", B, t->Bmax);
    OZ_HIP(hipSetDevice(t->device));
    hipStream_t s = t->s;
    const int A = t->n * t->n;
    if (t->aux) if (int rc = t_stage_fin(t, fin_own, fin_opp, B)) { hipStreamSynchronize(s); return rc; }
    {   // one upload (the call synchronises before it returns, so the pinned block is free again at the next call)
        unsigned char* h = t->h_in;
        memcpy(h + ((unsigned char*)t->d_own - t->d_in), own, B * sizeof(uint64_t));
        memcpy(h + ((unsigned char*)t->d_opp - t->d_in), opp, B * sizeof(uint64_t));
        memcpy(h + ((unsigned char*)t->d_pit - t->d_in), pi_target, (size_t)B * A * sizeof(float));
        memcpy(h + ((unsigned char*)t->d_zt - t->d_in), z_target, B * sizeof(float));
        memcpy(h + ((unsigned char*)t->d_count - t->d_in), &B, sizeof(int));
        OZ_HIP(hipMemcpyAsync(t->d_in, h, t->in_bytes, hipMemcpyHostToDevice, s));
    }
    if (int rc = t_forward_backward_async(t, B)) {
        hipStreamSynchronize(s);                   // the upload out of h_in may still be in flight: a retrying caller's next memcpy into it must not race with that DMA
        return rc;
    }
    float h[4], ha[2] = {0.f, 0.f};
    OZ_HIP(hipMemcpyAsync(h, t->losses, 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (aux5) OZ_HIP(hipMemcpyAsync(ha, t->aux_losses, 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    OZ_HIP(hipStreamSynchronize(s));
    if (losses3) { losses3[0] = h[0]; losses3[1] = h[1]; losses3[2] = h[2]; }
    if (losses3 && aux5) { losses3[3] = ha[0]; losses3[4] = ha[1]; }
    return t_check_range(t);
}
OZ_API int oz_trainer_forward_backward(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target,
                                       int B, float* losses3) {
    OZ_REQUIRE(t && own && opp && pi_target && z_target, "oz_trainer_forward_backward: NULL argument");
    T_LOCK(t);
    return t_forward_backward_host(t, own, opp, pi_target, z_target, nullptr, nullptr, B, losses3, false);
}
static int t_need_aux(oz_trainer* t, const char* who) {
    if (t->aux) return OZ_OK;
    oz_set_error("%s: this trainer has no auxiliary heads (oz_trainer_set_aux_heads)", who);
    return OZ_ERR_STATE;
}
OZ_API int oz_trainer_forward_backward_aux(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target,
                                           const uint64_t* fin_own, const uint64_t* fin_opp, int B, float* losses5) {
    OZ_REQUIRE(t && own && opp && pi_target && z_target && fin_own && fin_opp, "oz_trainer_forward_backward_aux: NULL argument");
    T_LOCK(t);
    if (int rc = t_need_aux(t, "oz_trainer_forward_backward_aux")) return rc;
    return t_forward_backward_host(t, own, opp, pi_target, z_target, fin_own, fin_opp, B, losses5, true);
}

// ---------------------------------------------------------------- HBM-resident data set: one upload per fit, one read-back per epoch
// keras Model.fit (Net/NNet.py:67) walks the examples in shuffled batches; here the examples live on the device for the
// whole fit, a step gathers its batch by index on the device, and the optimiser steps of an epoch are enqueued back to back
// (no host copy, no synchronisation per step); the sample-weighted loss sums are accumulated on the device.
// ds_fo / ds_fp (nullable, with fo / fp): the examples' final pairs for the auxiliary heads, gathered beside the boards
__global__ void k_t_gather_batch(const uint64_t* __restrict__ ds_own, const uint64_t* __restrict__ ds_opp, const float* __restrict__ ds_pi,
                                 const float* __restrict__ ds_z, const uint64_t* __restrict__ ds_fo, const uint64_t* __restrict__ ds_fp,
                                 const int* __restrict__ order, int first, int B, int A,
                                 uint64_t* __restrict__ own, uint64_t* __restrict__ opp, float* __restrict__ pit, float* __restrict__ zt,
                                 uint64_t* __restrict__ fo, uint64_t* __restrict__ fp, int* __restrict__ d_count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *d_count = B;
    if (i >= B * A) return;
    const int b = i / A, a = i % A, src = order[first + b];
    pit[i] = ds_pi[(size_t)src * A + a];
    if (a == 0) {
        own[b] = ds_own[src]; opp[b] = ds_opp[src]; zt[b] = ds_z[src];
        if (ds_fo) { fo[b] = ds_fo[src]; fp[b] = ds_fp[src]; }
    }
}
#define T_DS_ACC 6                       // doubles of ds_acc: 3 weighted loss sums, the samples, the two auxiliary sums
__global__ void k_t_acc_losses(const float* __restrict__ losses, const float* __restrict__ aux /*nullable*/, int B, double* __restrict__ acc /*[T_DS_ACC]*/) {
    if (threadIdx.x < 3) acc[threadIdx.x] += (double)losses[threadIdx.x] * (double)B;
    if (threadIdx.x == 3) acc[3] += (double)B;
    if (aux && (threadIdx.x == 4 || threadIdx.x == 5)) acc[threadIdx.x] += (double)aux[threadIdx.x - 4] * (double)B;
}

// Device arrays that grow with what a caller brings (`per` elements each per example, `cap` examples so far): when n exceeds cap, wait for the
// stream, free them, null the pointers and zero cap BEFORE allocating (a failed hipMalloc leaves no dangling pointer), then cap = n
struct TGrowArray { void** p; size_t bytes_per; };
#define T_GROW(ptr, per) TGrowArray{(void**)&(ptr), (size_t)(per) * sizeof(*(ptr))}
static int t_grow(oz_trainer* t, int64_t n, int64_t& cap, std::initializer_list<TGrowArray> arrays) {
    if (n <= cap) return OZ_OK;
    OZ_HIP(hipStreamSynchronize(t->s));
    for (const TGrowArray& a : arrays) { if (*a.p) hipFree(*a.p); *a.p = nullptr; }
    cap = 0;
    for (const TGrowArray& a : arrays) OZ_HIP(hipMalloc(a.p, (size_t)n * a.bytes_per));
    cap = n;
    return OZ_OK;
}

static int t_set_dataset(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target,
                         const uint64_t* fin_own, const uint64_t* fin_opp, int64_t N) {
    OZ_HIP(hipSetDevice(t->device));
    const int A = t->n * t->n;
    if (t->aux) {                      // the pairs beside the data set (no arrays given: every mask 0)
        if (int rc = t_grow(t, N, t->ds_fin_cap, {T_GROW(t->ds_fo, 1), T_GROW(t->ds_fp, 1)})) return rc;
        if (fin_own) {
            OZ_HIP(hipMemcpyAsync(t->ds_fo, fin_own, N * sizeof(uint64_t), hipMemcpyHostToDevice, t->s));
            OZ_HIP(hipMemcpyAsync(t->ds_fp, fin_opp, N * sizeof(uint64_t), hipMemcpyHostToDevice, t->s));
        } else {
            OZ_HIP(hipMemsetAsync(t->ds_fo, 0, N * sizeof(uint64_t), t->s));
            OZ_HIP(hipMemsetAsync(t->ds_fp, 0, N * sizeof(uint64_t), t->s));
        }
    }
    if (int rc = t_grow(t, N, t->ds_cap, {T_GROW(t->ds_own, 1), T_GROW(t->ds_opp, 1), T_GROW(t->ds_pi, A), T_GROW(t->ds_z, 1)})) return rc;
    if (int rc = t_grow(t, N, t->ds_order_cap, {T_GROW(t->ds_order, 1)})) return rc;      // (an epoch from a replay buffer may have sized it already)
    if (!t->ds_acc) OZ_HIP(hipMalloc((void**)&t->ds_acc, T_DS_ACC * sizeof(double)));
    OZ_HIP(hipMemcpyAsync(t->ds_own, own, N * sizeof(uint64_t), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipMemcpyAsync(t->ds_opp, opp, N * sizeof(uint64_t), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipMemcpyAsync(t->ds_pi, pi_target, (size_t)N * A * sizeof(float), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipMemcpyAsync(t->ds_z, z_target, N * sizeof(float), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));                       // the host arrays may go away
    t->ds_n = N;
    return OZ_OK;
}
OZ_API int oz_trainer_set_dataset(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target, int64_t N) {
    OZ_REQUIRE(t && own && opp && pi_target && z_target && N >= 1 && N < (1ll << 31), "oz_trainer_set_dataset: bad argument");
    T_LOCK(t);
    return t_set_dataset(t, own, opp, pi_target, z_target, nullptr, nullptr, N);
}
OZ_API int oz_trainer_set_dataset_aux(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target,
                                      const uint64_t* fin_own, const uint64_t* fin_opp, int64_t N) {
    OZ_REQUIRE(t && own && opp && pi_target && z_target && fin_own && fin_opp && N >= 1 && N < (1ll << 31), "oz_trainer_set_dataset_aux: bad argument");
    T_LOCK(t);
    if (int rc = t_need_aux(t, "oz_trainer_set_dataset_aux")) return rc;
    return t_set_dataset(t, own, opp, pi_target, z_target, fin_own, fin_opp, N);
}

static int t_apply_locked(oz_trainer* t);

// What an epoch reads its examples from: the trainer's own resident data set (oz_trainer_set_dataset) or a replay buffer's slots
// (oz_replay.hip) -- `n` examples in the same four arrays; fo / fp: their final pairs for the auxiliary heads (NULL: none, every mask 0).
struct TDataView { const uint64_t *own, *opp; const float *pi, *z; int64_t n; const uint64_t *fo = nullptr, *fp = nullptr; };

// What the epoch and evaluation entry points (`who`) check alike: the batch in [1, Bmax] and every index of `order` inside the resident data
// set or, r given (and locked), inside what the replay buffer holds -- then also r's board size and device and, need_fo, that it keeps the final pairs
static int t_check_batches(oz_trainer* t, const char* who, oz_replay* r, bool need_fo, const int32_t* order, int64_t count, int batch) {
    if (r) {
        OZ_REQUIRE(r->n == t->n, "%s: the trainer's boards are %d x %d, the replay buffer's %d x %d", who, t->n, t->n, r->n, r->n);
        OZ_REQUIRE(r->device == t->device, "%s: the trainer lives on device %d, the replay buffer on device %d", who, t->device, r->device);
    }
    OZ_REQUIRE(batch >= 1 && batch <= t->Bmax, "%s: batch %d outside [1, %d]", who, batch, t->Bmax);
    const int64_t limit = r ? r->held() : t->ds_n;
    for (int64_t i = 0; i < count; ++i) {
        if (order[i] >= 0 && order[i] < limit) continue;
        if (r) oz_set_error("%s: index %d outside the %lld examples the replay buffer holds", who, order[i], (long long)limit);
        else oz_set_error("%s: index %d outside the data set", who, order[i]);
        return OZ_ERR_ARG;
    }
    OZ_REQUIRE(!need_fo || r->fo, "%s: a trainer with the auxiliary heads needs a replay buffer that keeps the final pairs (oz_replay_create_aux)", who);
    return OZ_OK;
}

// the optimiser steps of one epoch over `d` in the order `order` (validated by the caller's entry point): per step one device-side gather of
// the batch, forward + backward, the loss accumulation and Adam, back to back on the stream; one read-back at the end
static int t_fit_epoch_view(oz_trainer* t, const TDataView& d, const int32_t* order, int64_t count, int batch, float* losses3) {
    OZ_HIP(hipSetDevice(t->device));
    hipStream_t s = t->s;
    const int A = t->n * t->n;
    if (int rc = t_grow(t, count, t->ds_order_cap, {T_GROW(t->ds_order, 1)})) return rc;      // (never on the resident path: oz_trainer_set_dataset sized it)
    if (!t->ds_acc) OZ_HIP(hipMalloc((void**)&t->ds_acc, T_DS_ACC * sizeof(double)));
    OZ_HIP(hipMemcpyAsync(t->ds_order, order, count * sizeof(int), hipMemcpyHostToDevice, s));
    OZ_HIP(hipMemsetAsync(t->ds_acc, 0, T_DS_ACC * sizeof(double), s));
    if (t->aux && !d.fo) OZ_HIP(hipMemsetAsync(t->d_fin, 0, 2 * (size_t)t->Bmax * sizeof(uint64_t), s));      // no pairs: every mask 0, for the whole epoch
    uint64_t* const fin_own = d.fo ? t->d_fin : nullptr, * const fin_opp = d.fo ? t->d_fin + t->Bmax : nullptr;      // (d.fo only with the auxiliary heads)
    for (int64_t first = 0; first < count; first += batch) {
        const int B = (int)(count - first < batch ? count - first : batch);            // the last batch may be short, as in keras
        hipLaunchKernelGGL(k_t_gather_batch, dim3((B * A + 255) / 256), dim3(256), 0, s, d.own, d.opp, d.pi, d.z, d.fo, d.fp, t->ds_order,
                           (int)first, B, A, t->d_own, t->d_opp, t->d_pit, t->d_zt, fin_own, fin_opp, t->d_count);
        if (int rc = t_forward_backward_async(t, B)) return rc;
        hipLaunchKernelGGL(k_t_acc_losses, dim3(1), dim3(64), 0, s, t->losses, t->aux ? t->aux_losses : (const float*)nullptr, B, t->ds_acc);
        if (int rc = t_apply_locked(t)) return rc;
    }
    double h[T_DS_ACC];
    OZ_HIP(hipMemcpyAsync(h, t->ds_acc, sizeof h, hipMemcpyDeviceToHost, s));
    OZ_HIP(hipStreamSynchronize(s));
    if (losses3) for (int k = 0; k < 3; ++k) losses3[k] = (float)(h[k] / (h[3] > 0 ? h[3] : 1.0));
    for (int k = 0; k < 2; ++k) t->epoch_aux[k] = h[4 + k] / (h[3] > 0 ? h[3] : 1.0);
    return t_check_range(t);
}

OZ_API int oz_trainer_fit_epoch(oz_trainer* t, const int32_t* order, int64_t count, int batch, float* losses3) {
    OZ_REQUIRE(t && order && count >= 1, "oz_trainer_fit_epoch: bad argument");
    T_LOCK(t);
    OZ_REQUIRE(t->ds_n > 0 && count <= t->ds_n, "oz_trainer_fit_epoch: %lld indices but the resident data set holds %lld examples (oz_trainer_set_dataset first)",
               (long long)count, (long long)t->ds_n);
    if (int rc = t_check_batches(t, "oz_trainer_fit_epoch", nullptr, false, order, count, batch)) return rc;
    return t_fit_epoch_view(t, {t->ds_own, t->ds_opp, t->ds_pi, t->ds_z, t->ds_n, t->aux ? t->ds_fo : nullptr, t->aux ? t->ds_fp : nullptr}, order, count, batch, losses3);
}

// the same epoch with a replay buffer's slots as the resident data set (trainer locked before the replay buffer; the appends are synchronous,
// so every held slot is complete)
OZ_API int oz_trainer_fit_epoch_replay(oz_trainer* t, oz_replay* r, const int32_t* order, int64_t count, int batch, float* losses3) {
    OZ_REQUIRE(t && r && order && count >= 1 && count < (1ll << 31), "oz_trainer_fit_epoch_replay: bad argument");
    T_LOCK(t);
    std::lock_guard<std::mutex> rlock(r->mu);
    if (int rc = t_check_batches(t, "oz_trainer_fit_epoch_replay", r, t->aux, order, count, batch)) return rc;
    return t_fit_epoch_view(t, {r->own, r->opp, r->pi, r->z, r->held(), t->aux ? r->fo : nullptr, t->aux ? r->fp : nullptr}, order, count, batch, losses3);
}

// ---------------------------------------------------------------- held-out evaluation in inference mode
// `count` examples of `d` in the order `order` (validated by the caller's entry point), batches of `batch`: per batch the device-side gather, the
// inference forward (the raw iterate t->P, the CURRENT moving statistics, no dropout) and the accumulation, back to back on the main stream; one
// synchronisation and one read-back.  Leaves alone: the weights, Adam moments, the weight average, step, the staged moving statistics (stats_new),
// the gradient arena, t->losses, the resident data set and ds_order.  Overwrites: z[l], a[l], p, v, the batch staging buffers (d_own .. d_count),
// the packed activations of a split mode and the plan rows' forward fields
static int t_evaluate_view(oz_trainer* t, const TDataView& d, const int32_t* order, int64_t count, int batch, double* out) {
    OZ_HIP(hipSetDevice(t->device));
    hipStream_t s = t->s;
    const int A = t->n * t->n;
    if (int rc = t_grow(t, count, t->ev_order_cap, {T_GROW(t->ev_order, 1)})) return rc;
    if (!t->ev_rows) T_ALLOC(t->ev_rows, (size_t)t->Bmax * OZ_EVAL_ROW);
    if (!t->ev_acc) T_ALLOC(t->ev_acc, 1);
    OZ_HIP(hipMemcpyAsync(t->ev_order, order, count * sizeof(int), hipMemcpyHostToDevice, s));
    OZ_HIP(hipMemsetAsync(t->ev_acc, 0, sizeof(TEvalAcc), s));
    if (t->dirty) if (int rc = t_refresh(t)) return rc;
    for (int64_t first = 0; first < count; first += batch) {
        const int B = (int)(count - first < batch ? count - first : batch);
        hipLaunchKernelGGL(k_t_gather_batch, dim3((B * A + 255) / 256), dim3(256), 0, s, d.own, d.opp, d.pi, d.z, nullptr, nullptr, t->ev_order,
                           (int)first, B, A, t->d_own, t->d_opp, t->d_pit, t->d_zt, nullptr, nullptr, t->d_count);
        if (int rc = t_forward(t, B, /*infer=*/true)) return rc;
        hipLaunchKernelGGL(k_t_acc_eval, dim3(1), dim3(256), 0, s, t->ev_rows, B, t->ev_acc);
    }
    OZ_HIP(hipGetLastError());
    TEvalAcc h;
    OZ_HIP(hipMemcpyAsync(&h, t->ev_acc, sizeof h, hipMemcpyDeviceToHost, s));
    OZ_HIP(hipStreamSynchronize(s));
    const double N = (double)h.examples;
    out[1] = h.sum[0] / N; out[2] = h.sum[1] / N; out[0] = out[1] + out[2];
    out[3] = (double)h.cnt[0] / N;
    out[4] = h.cnt[2] > 0 ? (double)h.cnt[1] / (double)h.cnt[2] : 0.0;
    out[5] = N; out[6] = (double)h.cnt[2]; out[7] = 0.0;
    return t_check_range(t);
}

OZ_API int oz_trainer_evaluate(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, int64_t N, int batch, double* out) {
    OZ_REQUIRE(t && own && opp && pi && z && out && N >= 1 && N < (1ll << 31), "oz_trainer_evaluate: bad argument");
    T_LOCK(t);
    if (int rc = t_check_batches(t, "oz_trainer_evaluate", nullptr, false, nullptr, 0, batch)) return rc;      // (the order is the identity)
    OZ_HIP(hipSetDevice(t->device));
    const int A = t->n * t->n;
    // arrays of the evaluation's own: the resident data set of a fit stays what it is
    if (int rc = t_grow(t, N, t->ev_cap, {T_GROW(t->ev_own, 1), T_GROW(t->ev_opp, 1), T_GROW(t->ev_pi, A), T_GROW(t->ev_z, 1)})) return rc;
    OZ_HIP(hipMemcpyAsync(t->ev_own, own, N * sizeof(uint64_t), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipMemcpyAsync(t->ev_opp, opp, N * sizeof(uint64_t), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipMemcpyAsync(t->ev_pi, pi, (size_t)N * A * sizeof(float), hipMemcpyHostToDevice, t->s));
    OZ_HIP(hipMemcpyAsync(t->ev_z, z, N * sizeof(float), hipMemcpyHostToDevice, t->s));
    std::vector<int32_t> order((size_t)N);
    for (int64_t i = 0; i < N; ++i) order[(size_t)i] = (int32_t)i;
    const int rc = t_evaluate_view(t, {t->ev_own, t->ev_opp, t->ev_pi, t->ev_z, N}, order.data(), N, batch, out);
    if (rc) hipStreamSynchronize(t->s);            // (a successful call has synchronised) the uploads out of the caller's arrays and `order` may still be in flight
    return rc;
}

OZ_API int oz_trainer_evaluate_dataset(oz_trainer* t, const int32_t* order, int64_t count, int batch, double* out) {
    OZ_REQUIRE(t && order && out && count >= 1 && count < (1ll << 31), "oz_trainer_evaluate_dataset: bad argument");
    T_LOCK(t);
    OZ_REQUIRE(t->ds_n > 0, "oz_trainer_evaluate_dataset: the resident data set is empty (oz_trainer_set_dataset first)");
    if (int rc = t_check_batches(t, "oz_trainer_evaluate_dataset", nullptr, false, order, count, batch)) return rc;
    return t_evaluate_view(t, {t->ds_own, t->ds_opp, t->ds_pi, t->ds_z, t->ds_n}, order, count, batch, out);
}

// (trainer locked before the replay buffer, as in oz_trainer_fit_epoch_replay)
OZ_API int oz_trainer_evaluate_replay(oz_trainer* t, oz_replay* r, const int32_t* order, int64_t count, int batch, double* out) {
    OZ_REQUIRE(t && r && order && out && count >= 1 && count < (1ll << 31), "oz_trainer_evaluate_replay: bad argument");
    T_LOCK(t);
    std::lock_guard<std::mutex> rlock(r->mu);
    if (int rc = t_check_batches(t, "oz_trainer_evaluate_replay", r, false, order, count, batch)) return rc;
    return t_evaluate_view(t, {r->own, r->opp, r->pi, r->z, r->held()}, order, count, batch, out);
}

// the two stages of the sum of squares of `X`'s arrays `sg` on the main stream -> norm_out[slot] (clipnorm > 0: the clip scale too)
static int t_sqsum_launch(oz_trainer* t, const float* X, const TSegs& sg, double clipnorm, int slot) {
    if (!t->norm_out) {
        T_ALLOC(t->sq_partial, T_OPT_SQ_BLOCKS);
        T_ALLOC(t->norm_out, 2);
    }
    int64_t units = 0;
    for (int r = 0; r < sg.n; ++r) if (sg.len[r] / 4 > units) units = sg.len[r] / 4;      // every thread walks every array: the grid covers the largest
    int blocks = (int)((units + 255) / 256);
    blocks = blocks < 1 ? 1 : blocks > T_OPT_SQ_BLOCKS ? T_OPT_SQ_BLOCKS : blocks;
    hipLaunchKernelGGL(k_t_sqsum, dim3(blocks), dim3(256), 0, t->s, X, sg, t->sq_partial);
    hipLaunchKernelGGL(k_t_sqsum_fin, dim3(1), dim3(256), 0, t->s, t->sq_partial, blocks, clipnorm, t->norm_out + slot);
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

// the optimiser kernel of one step at the rates (lr_s, lr_t): k_t_adam, or with an option on the norm (global-norm clip) and k_t_adam_x
static int t_launch_optimizer(oz_trainer* t, double lr_s, float lr_t, bool with_norm = true) {
    if (!t->fused)
        hipLaunchKernelGGL(k_t_adam, dim3((unsigned)((t->total + 255) / 256)), dim3(256), 0, t->s, t->P, t->G, t->M1, t->V2, (long long)t->total, lr_t, t->clip);
    else {
        const oz_optimizer& o = t->opt;
        const bool clipped = o.global_clipnorm > 0.0, avg = o.average_decay > 0.0;
        if (clipped && with_norm) {       // between the last gradient (the main stream has waited for the weight gradients) and the optimiser
            if (int rc = t_sqsum_launch(t, t->G, t->seg_all, o.global_clipnorm, 0)) return rc;
            t->last_clipped = true;
        }
        const TAdamX a = {lr_t, t->clip, (float)(2.0 * o.l2), (float)(lr_s * o.weight_decay), (float)o.average_decay, (float)(1.0 - o.average_decay)};
        const int units = (int)(t_arena_alloc(t->total) / 4);      // (whole units: only an arena with the auxiliary heads ends inside one, and that one is always library-owned)
        const int blocks = (units + 255) / 256 < T_OPT_ADAM_BLOCKS ? (units + 255) / 256 : T_OPT_ADAM_BLOCKS;
        hipLaunchKernelGGL(k_t_adam_x, dim3(blocks), dim3(256), 0, t->s, (float4*)t->P, (const float4*)t->G, (float4*)t->M1, (float4*)t->V2,
                           avg ? (float4*)t->E : (float4*)nullptr, units, a, clipped ? &t->norm_out[0].scale32 : (const float*)nullptr, t->dec_units);
    }
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

static int t_apply_locked(oz_trainer* t) {
    t->step += 1;
    const double b1t = pow(0.9, (double)t->step), b2t = pow(0.999, (double)t->step);
    const double lr_s = t_lr_at(&t->opt, t->lr, t->step);               // (no schedule: (double)lr, the value this line always used)
    const float lr_t = (float)(lr_s * sqrt(1.0 - b2t) / (1.0 - b1t));
    t->last_lr_s = lr_s; t->applied = true; t->last_clipped = false;
    if (int rc = t_launch_optimizer(t, lr_s, lr_t)) return rc;
    for (int i = 0; i < 36; ++i)            // the staged moving statistics become the current ones (pointer swap, stream-ordered use)
        if (t->toff[i] < 0) { float* tmp = t->stats[i]; t->stats[i] = t->stats_new[i]; t->stats_new[i] = tmp; }
    t->dirty = true;
    // the operands derived from the new weights are rebuilt now, on the second stream, behind the optimiser step -- not at the next forward's
    // first launch: what the host does between two steps (the next batch's upload) no longer delays them
    return t_refresh(t);
}
OZ_API int oz_trainer_apply(oz_trainer* t) {
    OZ_REQUIRE(t, "oz_trainer_apply: NULL");
    T_LOCK(t);
    OZ_HIP(hipSetDevice(t->device));
    return t_apply_locked(t);
}

// ---------------------------------------------------------------- optimiser options: the entry points
OZ_API int oz_trainer_set_optimizer(oz_trainer* t, const oz_optimizer* opt) {
    OZ_REQUIRE(t, "oz_trainer_set_optimizer: NULL");
    if (int rc = t_opt_check(opt, "oz_trainer_set_optimizer")) return rc;
    T_LOCK(t);
    const oz_optimizer o = opt ? *opt : oz_optimizer{};
    const bool fused = o.l2 > 0.0 || o.weight_decay > 0.0 || o.global_clipnorm > 0.0 || o.average_decay > 0.0;
    OZ_REQUIRE(!fused || ((uintptr_t)t->G & 15) == 0, "oz_trainer_set_optimizer: the external gradient arena is not 16-byte aligned");
    OZ_HIP(hipSetDevice(t->device));
    if (o.average_decay > 0.0 && !(t->opt.average_decay > 0.0)) {        // switched on: E = the weights as they are now (stream order)
        if (!t->E) T_ALLOC(t->E, t_arena_alloc(t->total));
        OZ_HIP(hipMemcpyAsync(t->E, t->P, t->total * sizeof(float), hipMemcpyDeviceToDevice, t->s));
        OZ_HIP(hipStreamSynchronize(t->s));
    }
    t->opt = o;
    t->fused = fused;
    t_opt_tables(t);
    return OZ_OK;
}
OZ_API int oz_trainer_get_optimizer(oz_trainer* t, oz_optimizer* opt) {
    OZ_REQUIRE(t && opt, "oz_trainer_get_optimizer: bad argument");
    T_LOCK(t);
    *opt = t->opt;
    return OZ_OK;
}
OZ_API int oz_trainer_set_lr(oz_trainer* t, float lr) {
    OZ_REQUIRE(t && lr >= 0.f && std::isfinite(lr), "oz_trainer_set_lr: bad argument");
    T_LOCK(t);
    t->lr = lr;                          // read on the host at the next apply
    return OZ_OK;
}
OZ_API int oz_trainer_get_step_info(oz_trainer* t, double* lr_s, double* grad_norm, double* clip_scale) {
    OZ_REQUIRE(t && lr_s && grad_norm && clip_scale, "oz_trainer_get_step_info: bad argument");
    T_LOCK(t);
    if (!t->applied) { oz_set_error("oz_trainer_get_step_info: no optimiser step has been applied yet"); return OZ_ERR_STATE; }
    *lr_s = t->last_lr_s; *grad_norm = 0.0; *clip_scale = 1.0;
    OZ_HIP(hipSetDevice(t->device));
    if (t->last_clipped) {
        TNormOut h;
        OZ_HIP(hipMemcpyAsync(&h, t->norm_out, sizeof h, hipMemcpyDeviceToHost, t->s));
        OZ_HIP(hipStreamSynchronize(t->s));
        *grad_norm = h.norm; *clip_scale = h.scale;
    } else OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}
OZ_API int oz_trainer_get_weight_average(oz_trainer* t, int index, float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && index >= 0 && index < t->nw, "oz_trainer_get_weight_average: bad argument");
    T_LOCK(t);
    OZ_REQUIRE(nelem == t->size[index], "oz_trainer_get_weight_average: weight %d has %lld elements, got %lld", index, (long long)t->size[index], (long long)nelem);
    if (!(t->opt.average_decay > 0.0)) { oz_set_error("oz_trainer_get_weight_average: the weight average is off (oz_optimizer.average_decay)"); return OZ_ERR_STATE; }
    OZ_HIP(hipSetDevice(t->device));
    const float* src = t->toff[index] >= 0 ? t->E + t->toff[index] : t->stats[index];
    OZ_HIP(hipMemcpyAsync(data, src, nelem * sizeof(float), hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}
OZ_API int oz_trainer_sqsum(oz_trainer* t, int what, double* out) {
    OZ_REQUIRE(t && out && (what == OZ_SQSUM_GRADIENTS || what == OZ_SQSUM_DECAYED_WEIGHTS), "oz_trainer_sqsum: bad argument");
    T_LOCK(t);
    OZ_REQUIRE(((uintptr_t)t->G & 15) == 0, "oz_trainer_sqsum: the external gradient arena is not 16-byte aligned");
    OZ_HIP(hipSetDevice(t->device));
    const bool grads = what == OZ_SQSUM_GRADIENTS;
    if (int rc = t_sqsum_launch(t, grads ? t->G : t->P, grads ? t->seg_all : t->seg_dec, 0.0, 1)) return rc;
    TNormOut h;
    OZ_HIP(hipMemcpyAsync(&h, t->norm_out + 1, sizeof h, hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    *out = h.sumsq;
    return OZ_OK;
}

// Benchmark hook (tools/optimizer_bench.py): HIP-event time of the step's optimiser kernel and of the norm's two kernels, `iters` launches each on an
// otherwise idle device.  It RUNS the kernels on the trainer's arrays with the arena as it is: the weights, moments and average move as under
// `iters` steps (the step count does not) -- for a scratch trainer.
OZ_API int oz_trainer_time_optimizer(oz_trainer* t, int iters, double* ms3) {
    OZ_REQUIRE(t && ms3 && iters >= 1 && iters <= 10000, "oz_trainer_time_optimizer: bad argument");
    T_LOCK(t);
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipStreamSynchronize(t->s));
    OZ_HIP(hipStreamSynchronize(t->s2));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    OZ_HIP(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); oz_set_error("oz_trainer_time_optimizer: no event"); return OZ_ERR_HIP; }
    const int rc = [&]() -> int {
        float ms = 0.f;
        ms3[0] = ms3[1] = ms3[2] = 0.0;
        const double lr_s = t_lr_at(&t->opt, t->lr, t->step + 1);
        const float lr_t = (float)(lr_s * sqrt(1.0 - pow(0.999, (double)t->step + 1)) / (1.0 - pow(0.9, (double)t->step + 1)));
        if (t->fused && t->opt.global_clipnorm > 0.0) {
            OZ_HIP(hipEventRecord(e0, t->s));
            for (int i = 0; i < iters; ++i) if (int r = t_sqsum_launch(t, t->G, t->seg_all, t->opt.global_clipnorm, 0)) return r;
            OZ_HIP(hipEventRecord(e1, t->s));
            OZ_HIP(hipEventSynchronize(e1));
            OZ_HIP(hipEventElapsedTime(&ms, e0, e1));
            ms3[1] = (double)ms / iters;
        }
        OZ_HIP(hipEventRecord(e0, t->s));
        for (int i = 0; i < iters; ++i) if (int r = t_launch_optimizer(t, lr_s, lr_t, false)) return r;
        OZ_HIP(hipEventRecord(e1, t->s));
        OZ_HIP(hipEventSynchronize(e1));
        OZ_HIP(hipEventElapsedTime(&ms, e0, e1));
        ms3[0] = (double)ms / iters;
        t->dirty = true;
        return OZ_OK;
    }();
    hipEventDestroy(e0); hipEventDestroy(e1);
    return rc;
}

OZ_API int oz_trainer_get_activation(oz_trainer* t, int layer, int B, float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && layer >= 0 && layer < 6 && B >= 1 && B <= t->Bmax, "oz_trainer_get_activation: bad argument");
    T_LOCK(t);
    OZ_REQUIRE(nelem == (int64_t)B * t->L[layer].P * t->L[layer].Co, "oz_trainer_get_activation: expected %lld elements", (long long)B * t->L[layer].P * t->L[layer].Co);
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipMemcpyAsync(data, t->a[layer], nelem * sizeof(float), hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}

OZ_API int oz_trainer_outputs(oz_trainer* t, int B, float* p, float* v) {
    OZ_REQUIRE(t && B >= 1 && B <= t->Bmax, "oz_trainer_outputs: bad argument");
    T_LOCK(t);
    OZ_HIP(hipSetDevice(t->device));
    if (p) OZ_HIP(hipMemcpyAsync(p, t->p, (size_t)B * t->n * t->n * sizeof(float), hipMemcpyDeviceToHost, t->s));
    if (v) OZ_HIP(hipMemcpyAsync(v, t->v, B * sizeof(float), hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}

// ---------------------------------------------------------------- diagnostics: read-only views of the last step (the per-kernel parity tests)
// a device buffer of the last step -> host, on the main stream (every entry point that ran the step has synchronised it)
static int t_read(oz_trainer* t, const float* src, float* data, int64_t nelem) {
    OZ_HIP(hipSetDevice(t->device));
    OZ_HIP(hipMemcpyAsync(data, src, nelem * sizeof(float), hipMemcpyDeviceToHost, t->s));
    OZ_HIP(hipStreamSynchronize(t->s));
    return OZ_OK;
}
static int t_need_step(oz_trainer* t, const char* who) {
    if (t->ran) return OZ_OK;
    oz_set_error("%s: no step has run on this trainer yet", who);
    return OZ_ERR_STATE;
}
OZ_API int oz_trainer_get_preact(oz_trainer* t, int layer, int B, float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && layer >= 0 && layer < 6 && B >= 1 && B <= t->Bmax, "oz_trainer_get_preact: bad argument");
    T_LOCK(t);
    const TLayer& L = t->L[layer];
    OZ_REQUIRE(nelem == (int64_t)B * L.P * L.Co, "oz_trainer_get_preact: expected %lld elements", (long long)B * L.P * L.Co);
    if (int rc = t_need_step(t, "oz_trainer_get_preact")) return rc;
    return t_read(t, t->z[layer], data, nelem);
}
OZ_API int oz_trainer_get_dz(oz_trainer* t, int layer, int B, float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && layer >= 0 && layer < 6 && B >= 1 && B <= t->Bmax, "oz_trainer_get_dz: bad argument");
    T_LOCK(t);
    const TLayer& L = t->L[layer];
    OZ_REQUIRE(nelem == (int64_t)B * L.Hz * L.Hz * L.Co, "oz_trainer_get_dz: expected %lld elements", (long long)B * L.Hz * L.Hz * L.Co);
    if (int rc = t_need_step(t, "oz_trainer_get_dz")) return rc;
    return t_read(t, t->dz[layer], data, nelem);
}
OZ_API int oz_trainer_set_capture(oz_trainer* t, int on) {
    OZ_REQUIRE(t, "oz_trainer_set_capture: NULL");
    T_LOCK(t);
    OZ_HIP(hipSetDevice(t->device));
    if (on && !t->cap[5]) {              // (the last of the six: an allocation that failed part-way is repeated, never half used)
        for (int l = 0; l < 6; ++l) T_ALLOC(t->cap[l], (size_t)t->Bmax * t->L[l].P * t->L[l].Co);
        OZ_HIP(hipStreamSynchronize(t->s));
    }
    if (on && t->aux && !t->cap_f2) {
        T_ALLOC(t->cap_f2, (size_t)t->Bmax * 512);
        OZ_HIP(hipStreamSynchronize(t->s));
    }
    t->capture = on != 0;
    t->cap_valid = false;                 // what an earlier step captured is not the next reader's step
    return OZ_OK;
}
OZ_API int oz_trainer_get_dgrad(oz_trainer* t, int layer, int B, float* data, int64_t nelem) {
    OZ_REQUIRE(t && data && layer >= 0 && layer < 6 && B >= 1 && B <= t->Bmax, "oz_trainer_get_dgrad: bad argument");
    T_LOCK(t);
    if (!t->capture || !t->cap_valid) {
        oz_set_error("oz_trainer_get_dgrad: no captured step (oz_trainer_set_capture(t, 1), then a step)");
        return OZ_ERR_STATE;
    }
    const TLayer& L = t->L[layer];
    OZ_REQUIRE(nelem == (int64_t)B * L.P * L.Co, "oz_trainer_get_dgrad: expected %lld elements", (long long)B * L.P * L.Co);
    return t_read(t, t->cap[layer], data, nelem);
}
OZ_API int oz_trainer_get_head_grads(oz_trainer* t, int B, float* dlogit, float* dvpre) {
    OZ_REQUIRE(t && dlogit && dvpre && B >= 1 && B <= t->Bmax, "oz_trainer_get_head_grads: bad argument");
    T_LOCK(t);
    if (int rc = t_need_step(t, "oz_trainer_get_head_grads")) return rc;
    if (int rc = t_read(t, t->dlogit, dlogit, (int64_t)B * t->n * t->n)) return rc;
    return t_read(t, t->dvpre, dvpre, B);
}
// ---------------------------------------------------------------- auxiliary heads: read-outs of the last step
OZ_API int oz_trainer_aux_outputs(oz_trainer* t, int B, float* own, float* score) {
    OZ_REQUIRE(t && B >= 1 && B <= t->Bmax, "oz_trainer_aux_outputs: bad argument");
    T_LOCK(t);
    if (int rc = t_need_aux(t, "oz_trainer_aux_outputs")) return rc;
    if (int rc = t_need_step(t, "oz_trainer_aux_outputs")) return rc;
    if (own) if (int rc = t_read(t, t->ao, own, (int64_t)B * t->n * t->n)) return rc;
    if (score) if (int rc = t_read(t, t->as, score, B)) return rc;
    return OZ_OK;
}
OZ_API int oz_trainer_get_aux_losses(oz_trainer* t, float* step2, double* epoch2) {
    OZ_REQUIRE(t, "oz_trainer_get_aux_losses: NULL");
    T_LOCK(t);
    if (int rc = t_need_aux(t, "oz_trainer_get_aux_losses")) return rc;
    if (step2) {
        if (int rc = t_need_step(t, "oz_trainer_get_aux_losses")) return rc;
        if (int rc = t_read(t, t->aux_losses, step2, 2)) return rc;
    }
    if (epoch2) { epoch2[0] = t->epoch_aux[0]; epoch2[1] = t->epoch_aux[1]; }
    return OZ_OK;
}
OZ_API int oz_trainer_get_aux_head_grads(oz_trainer* t, int B, float* dopre, float* dspre, float* df2_before) {
    OZ_REQUIRE(t && dopre && dspre && B >= 1 && B <= t->Bmax, "oz_trainer_get_aux_head_grads: bad argument");
    T_LOCK(t);
    if (int rc = t_need_aux(t, "oz_trainer_get_aux_head_grads")) return rc;
    if (int rc = t_need_step(t, "oz_trainer_get_aux_head_grads")) return rc;
    if (int rc = t_read(t, t->dopre, dopre, (int64_t)B * t->n * t->n)) return rc;
    if (int rc = t_read(t, t->dspre, dspre, B)) return rc;
    if (!df2_before) return OZ_OK;
    if (!t->capture || !t->cap_valid || !(t->w_own > 0.f || t->w_sc > 0.f)) {
        oz_set_error("oz_trainer_get_aux_head_grads: no captured step with an auxiliary weight on (oz_trainer_set_capture(t, 1), then a step)");
        return OZ_ERR_STATE;
    }
    return t_read(t, t->cap_f2, df2_before, (int64_t)B * 512);
}
OZ_API int oz_trainer_get_plan(oz_trainer* t, int* plan, int n) {
    OZ_REQUIRE(t && plan && n == OZ_TRAINER_PLAN_ROWS * OZ_TRAINER_PLAN_FIELDS, "oz_trainer_get_plan: plan holds OZ_TRAINER_PLAN_ROWS x OZ_TRAINER_PLAN_FIELDS ints");
    T_LOCK(t);
    memcpy(plan, t->plan, sizeof t->plan);
    return OZ_OK;
}
OZ_API int oz_trainer_get_bn_stats(oz_trainer* t, int layer, float* mean, float* rstd) {
    OZ_REQUIRE(t && mean && rstd && layer >= 0 && layer < 6, "oz_trainer_get_bn_stats: bad argument");
    T_LOCK(t);
    if (int rc = t_need_step(t, "oz_trainer_get_bn_stats")) return rc;
    if (int rc = t_read(t, t->mean[layer], mean, t->L[layer].Co)) return rc;
    return t_read(t, t->rstd[layer], rstd, t->L[layer].Co);
}
OZ_API int oz_trainer_get_adam_state(oz_trainer* t, int index, float* m, float* v) {
    OZ_REQUIRE(t && m && v && index >= 0 && index < t->nw, "oz_trainer_get_adam_state: bad argument");
    T_LOCK(t);
    OZ_REQUIRE(t->toff[index] >= 0, "oz_trainer_get_adam_state: array %d is a moving statistic, it has no moments", index);
    if (int rc = t_read(t, t->M1 + t->toff[index], m, t->size[index])) return rc;
    return t_read(t, t->V2 + t->toff[index], v, t->size[index]);
}
