// oz_rules.hip -- library core (errors, device selection), batched rule kernels (K1-K3) and the
// dihedral symmetry expansion of training examples (K8).  HBM-bound integer/byte work: one thread
// per position / per output example, SoA inputs, coalesced loads and stores.  Plus the batch entry of
// the fixed-depth minimax (one wavefront per position, oz_minimax.h) and of the exact endgame solver (oz_solve.h).
#include <stdarg.h>
#include <string.h>

#include "oz_internal.h"
#include "oz_minimax.h"
#include "oz_openings.h"
#include "oz_solve.h"

// ---------------------------------------------------------------- errors / device
static thread_local char g_err[512] = "";
static thread_local int g_device = -1;

void oz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
OZ_API const char* oz_last_error(void) { return g_err; }
OZ_API int oz_version(void) { return 230; }     // 201: visit-count policy targets; 210: leaf-parallel search (leaves_per_step); 220: root noise; 230: move sampling
                                                // 200 (round 4): edge_cap left oz_mcts_create / oz_arena_create / oz_selfplay_config
OZ_API int oz_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}
OZ_API int oz_set_device(int device) {
    OZ_HIP(hipSetDevice(device));
    g_device = device;
    return OZ_OK;
}
// The device a new object is created on / a batch call runs on: the one oz_set_device chose for this thread, else whatever
// the HIP runtime's current device is RIGHT NOW (e.g. torch.cuda.set_device(local_rank) in a one-process-per-GPU job) --
// never a value cached from an earlier call, and never overriding a device the caller selected.
int oz_current_device() {
    if (g_device >= 0) { hipSetDevice(g_device); return g_device; }
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    return d;
}

// small RAII device buffer for the batch entry points
template <typename T> struct DevBuf {
    T* p = nullptr;
    hipError_t alloc(size_t count) { return hipMalloc((void**)&p, sizeof(T) * (count ? count : 1)); }
    ~DevBuf() { if (p) hipFree(p); }
};

// Persistent staging of the oz_rules_* entry points (one per device, process lifetime): the drop-in OthelloGame asks about
// ONE position per call, so a call must not pay hipMalloc / hipFree (device-wide syncs) nor one blocking copy per array.
// A call packs its inputs into the pinned host image, does ONE upload, the kernel, ONE download on a private stream.
struct RulesStage {
    std::mutex mu;
    hipStream_t stream = nullptr;
    unsigned char *dev = nullptr, *host = nullptr;       // host = pinned (hipHostMalloc)
    size_t cap = 0;
    bool profile = false;                                // oz_rules_profile: HIP events around the kernel of every call
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms_total = 0.0;
    long long launches = 0;
    int reserve(size_t bytes) {
        if (!stream) OZ_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (bytes <= cap) return OZ_OK;
        size_t want = cap ? cap : 4096;
        while (want < bytes) want *= 2;
        if (dev) { hipFree(dev); hipHostFree(host); dev = host = nullptr; cap = 0; }
        OZ_HIP(hipMalloc((void**)&dev, want));
        OZ_HIP(hipHostMalloc((void**)&host, want, hipHostMallocDefault));
        cap = want;
        return OZ_OK;
    }
};
static RulesStage g_stage[16];
static inline size_t pad8(size_t x) { return (x + 7) & ~(size_t)7; }

// ---------------------------------------------------------------- rule kernels
__global__ void k_legal(const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp, int count, uint64_t valid,
                        uint64_t* __restrict__ legal) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) legal[i] = oz_legal(own[i], opp[i], valid);
}
__global__ void k_apply(const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp, const uint8_t* __restrict__ sq,
                        int count, uint64_t* __restrict__ own_out, uint64_t* __restrict__ opp_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t a = own[i], b = opp[i];
    oz_apply(a, b, sq[i]);
    own_out[i] = a; opp_out[i] = b;
}
__global__ void k_status(const uint64_t* __restrict__ c0, const uint64_t* __restrict__ c1, int count, uint64_t valid,
                         uint8_t* __restrict__ finished, int32_t* __restrict__ p0, int32_t* __restrict__ p1,
                         int8_t* __restrict__ winner) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t a = c0[i], b = c1[i];
    finished[i] = (oz_legal(a, b, valid) == 0 && oz_legal(b, a, valid) == 0) ? 1 : 0;
    int x = oz_popc(a), y = oz_popc(b);
    p0[i] = x; p1[i] = y;
    winner[i] = x >= y ? 1 : -1;          // max() over {BLACK, WHITE} keeps the first maximum
}
__global__ void k_play(const uint64_t* __restrict__ black, const uint64_t* __restrict__ white, const int8_t* __restrict__ player,
                       const uint8_t* __restrict__ sq, int count, uint64_t valid, uint64_t* __restrict__ bo,
                       uint64_t* __restrict__ wo, int8_t* __restrict__ po, uint8_t* __restrict__ fo) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t b = black[i], w = white[i];
    int p = player[i], f = 0;
    oz_game_play(b, w, p, f, sq[i], valid);
    bo[i] = b; wo[i] = w; po[i] = (int8_t)p; fo[i] = (uint8_t)f;
}

static inline int grid_for(int count) { return (count + 255) / 256; }
static int check_n(int n) {
    OZ_REQUIRE(n == 4 || n == 6 || n == 8, "board size must be 4, 6 or 8 (got %d)", n);
    return OZ_OK;
}

// run `launch(dev_in, dev_out, stream)` between one upload of in_bytes and one download of out_bytes
template <typename Pack, typename Launch, typename Unpack>
static int rules_call(size_t in_bytes, size_t out_bytes, Pack pack, Launch launch, Unpack unpack) {
    const int dev = oz_current_device();
    OZ_REQUIRE(dev >= 0 && dev < 16, "device index %d out of range", dev);
    RulesStage& st = g_stage[dev];
    std::lock_guard<std::mutex> lk(st.mu);
    const size_t in_p = pad8(in_bytes);
    if (int rc = st.reserve(in_p + pad8(out_bytes))) return rc;
    pack(st.host);
    OZ_HIP(hipMemcpyAsync(st.dev, st.host, in_bytes, hipMemcpyHostToDevice, st.stream));
    if (st.profile) OZ_HIP(hipEventRecord(st.ev0, st.stream));
    launch(st.dev, st.dev + in_p, st.stream);
    OZ_HIP(hipGetLastError());
    if (st.profile) OZ_HIP(hipEventRecord(st.ev1, st.stream));
    OZ_HIP(hipMemcpyAsync(st.host + in_p, st.dev + in_p, out_bytes, hipMemcpyDeviceToHost, st.stream));
    OZ_HIP(hipStreamSynchronize(st.stream));
    if (st.profile) {
        float ms = 0.f;
        OZ_HIP(hipEventElapsedTime(&ms, st.ev0, st.ev1));
        st.ms_total += ms; st.launches += 1;
    }
    unpack(st.host + in_p);
    return OZ_OK;
}

// HIP-event timing of the kernels behind the oz_rules_* batch entries on the current device (tools/solve_bench.py); off, a call records nothing
OZ_API int oz_rules_profile(int enable) {
    const int dev = oz_current_device();
    OZ_REQUIRE(dev >= 0 && dev < 16, "device index %d out of range", dev);
    RulesStage& st = g_stage[dev];
    std::lock_guard<std::mutex> lk(st.mu);
    if (enable && !st.ev0) { OZ_HIP(hipEventCreate(&st.ev0)); OZ_HIP(hipEventCreate(&st.ev1)); }
    st.profile = enable != 0;
    return OZ_OK;
}
OZ_API int oz_rules_profile_read(double* ms_total, int64_t* launches, int reset) {
    const int dev = oz_current_device();
    OZ_REQUIRE(dev >= 0 && dev < 16, "device index %d out of range", dev);
    RulesStage& st = g_stage[dev];
    std::lock_guard<std::mutex> lk(st.mu);
    if (ms_total) *ms_total = st.ms_total;
    if (launches) *launches = st.launches;
    if (reset) { st.ms_total = 0.0; st.launches = 0; }
    return OZ_OK;
}

OZ_API int oz_rules_legal_moves(const uint64_t* own, const uint64_t* opp, int n, int count, uint64_t* legal) {
    if (int rc = check_n(n)) return rc;
    if (count <= 0) return OZ_OK;
    const size_t c8 = 8ull * count;
    return rules_call(2 * c8, c8,
        [&](unsigned char* h) { memcpy(h, own, c8); memcpy(h + c8, opp, c8); },
        [&](unsigned char* di, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_legal, dim3(grid_for(count)), dim3(256), 0, s, (const uint64_t*)di, (const uint64_t*)(di + c8), count,
                               oz_valid_mask(n), (uint64_t*)dout);
        },
        [&](const unsigned char* h) { memcpy(legal, h, c8); });
}

OZ_API int oz_rules_apply_moves(const uint64_t* own, const uint64_t* opp, const uint8_t* sq, int n, int count,
                                uint64_t* own_out, uint64_t* opp_out) {
    if (int rc = check_n(n)) return rc;
    if (count <= 0) return OZ_OK;
    for (int i = 0; i < count; ++i) OZ_REQUIRE((sq[i] >> 3) < n && (sq[i] & 7) < n, "square %d outside the %dx%d board", sq[i], n, n);
    const size_t c8 = 8ull * count;
    return rules_call(2 * c8 + count, 2 * c8,
        [&](unsigned char* h) { memcpy(h, own, c8); memcpy(h + c8, opp, c8); memcpy(h + 2 * c8, sq, count); },
        [&](unsigned char* di, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_apply, dim3(grid_for(count)), dim3(256), 0, s, (const uint64_t*)di, (const uint64_t*)(di + c8),
                               (const uint8_t*)(di + 2 * c8), count, (uint64_t*)dout, (uint64_t*)(dout + c8));
        },
        [&](const unsigned char* h) { memcpy(own_out, h, c8); memcpy(opp_out, h + c8, c8); });
}

OZ_API int oz_rules_status(const uint64_t* ch0, const uint64_t* ch1, int n, int count, uint8_t* finished,
                           int32_t* pts0, int32_t* pts1, int8_t* winner) {
    if (int rc = check_n(n)) return rc;
    if (count <= 0) return OZ_OK;
    const size_t c8 = 8ull * count, c4 = 4ull * count, c1 = pad8(count);
    // output image: pts0 | pts1 | finished | winner (each 8-byte aligned)
    return rules_call(2 * c8, 2 * pad8(c4) + 2 * c1,
        [&](unsigned char* h) { memcpy(h, ch0, c8); memcpy(h + c8, ch1, c8); },
        [&](unsigned char* di, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_status, dim3(grid_for(count)), dim3(256), 0, s, (const uint64_t*)di, (const uint64_t*)(di + c8), count,
                               oz_valid_mask(n), (uint8_t*)(dout + 2 * pad8(c4)), (int32_t*)dout, (int32_t*)(dout + pad8(c4)),
                               (int8_t*)(dout + 2 * pad8(c4) + c1));
        },
        [&](const unsigned char* h) {
            memcpy(pts0, h, c4); memcpy(pts1, h + pad8(c4), c4);
            memcpy(finished, h + 2 * pad8(c4), count); memcpy(winner, h + 2 * pad8(c4) + c1, count);
        });
}

OZ_API int oz_rules_play(const uint64_t* black, const uint64_t* white, const int8_t* player, const uint8_t* sq, int n,
                         int count, uint64_t* black_out, uint64_t* white_out, int8_t* player_out, uint8_t* finished_out) {
    if (int rc = check_n(n)) return rc;
    if (count <= 0) return OZ_OK;
    for (int i = 0; i < count; ++i) {
        OZ_REQUIRE((sq[i] >> 3) < n && (sq[i] & 7) < n, "square %d outside the %dx%d board", sq[i], n, n);
        OZ_REQUIRE(player[i] == 1 || player[i] == -1, "player must be +1 or -1");
    }
    const size_t c8 = 8ull * count, c1 = pad8(count);
    return rules_call(2 * c8 + 2 * c1, 2 * c8 + 2 * c1,
        [&](unsigned char* h) { memcpy(h, black, c8); memcpy(h + c8, white, c8); memcpy(h + 2 * c8, player, count); memcpy(h + 2 * c8 + c1, sq, count); },
        [&](unsigned char* di, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_play, dim3(grid_for(count)), dim3(256), 0, s, (const uint64_t*)di, (const uint64_t*)(di + c8),
                               (const int8_t*)(di + 2 * c8), (const uint8_t*)(di + 2 * c8 + c1), count, oz_valid_mask(n), (uint64_t*)dout,
                               (uint64_t*)(dout + c8), (int8_t*)(dout + 2 * c8), (uint8_t*)(dout + 2 * c8 + c1));
        },
        [&](const unsigned char* h) {
            memcpy(black_out, h, c8); memcpy(white_out, h + c8, c8); memcpy(player_out, h + 2 * c8, count); memcpy(finished_out, h + 2 * c8 + c1, count);
        });
}

// ---------------------------------------------------------------- minimax (agents.py:27-41, the greedy agent's intent, made deeper by one integer)
// one 64-lane block per position (oz_minimax.h): values[i][sq] = exact root value of the move on sq, bests[i] = the maximal moves
__global__ __launch_bounds__(64) void k_minimax(const uint64_t* __restrict__ black, const uint64_t* __restrict__ white, const int8_t* __restrict__ player,
                                                uint64_t valid, int depth, MinimaxEval ev, int32_t* __restrict__ values, uint64_t* __restrict__ bests) {
    __shared__ MinimaxLds L;
    const int i = blockIdx.x, lane = threadIdx.x;
    uint64_t b = 0;
    const int v = mm_root(L, ev, valid, lane, black[i], white[i], player[i], depth, &b);
    values[(size_t)i * 64 + lane] = v;
    if (lane == 0) bests[i] = b;
}

OZ_API int oz_rules_minimax(const uint64_t* black, const uint64_t* white, const int8_t* player, int n, int count, int depth, int eval,
                            int32_t* values, uint64_t* bests) {
    if (int rc = check_n(n)) return rc;
    OZ_REQUIRE(depth >= 1 && depth <= OZ_MINIMAX_MAX_DEPTH, "oz_rules_minimax: depth %d outside 1..%d", depth, OZ_MINIMAX_MAX_DEPTH);
    OZ_REQUIRE(eval == OZ_MINIMAX_EVAL_DISCS || eval == OZ_MINIMAX_EVAL_WEIGHTED, "oz_rules_minimax: unknown evaluation %d", eval);
    if (count <= 0) return OZ_OK;
    OZ_REQUIRE(black && white && player, "null argument");
    for (int i = 0; i < count; ++i) OZ_REQUIRE(player[i] == 1 || player[i] == -1, "player must be +1 or -1");
    const size_t c8 = 8ull * count, c1 = pad8(count), cv = 256ull * count;
    const MinimaxEval ev = oz_minimax_eval_make(n, eval);
    // output image: values | bests
    return rules_call(2 * c8 + c1, cv + c8,
        [&](unsigned char* h) { memcpy(h, black, c8); memcpy(h + c8, white, c8); memcpy(h + 2 * c8, player, count); },
        [&](unsigned char* di, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_minimax, dim3(count), dim3(64), 0, s, (const uint64_t*)di, (const uint64_t*)(di + c8), (const int8_t*)(di + 2 * c8),
                               oz_valid_mask(n), depth, ev, (int32_t*)dout, (uint64_t*)(dout + cv));
        },
        [&](const unsigned char* h) {
            if (values) memcpy(values, h, cv);
            if (bests) memcpy(bests, h + cv, c8);
        });
}

// ---------------------------------------------------------------- exact endgame solver (oz_solve.h; the reference has none)
// one 64-lane block per position: values[i][sq] = S after the move on sq, bests[i] = the maximal moves, value[i] = S of the position;
// a position with more than max_empties empties is left alone (solved[i] = 0)
__global__ __launch_bounds__(64) void k_solve(const uint64_t* __restrict__ black, const uint64_t* __restrict__ white, const int8_t* __restrict__ player,
                                              uint64_t valid, uint64_t corners, int n2, int max_empties, int32_t* __restrict__ values,
                                              uint64_t* __restrict__ bests, int32_t* __restrict__ value, uint8_t* __restrict__ solved) {
    __shared__ SolveLds L;
    const int i = blockIdx.x, lane = threadIdx.x;
    const uint64_t b = black[i], w = white[i];
    const int empties = n2 - oz_popc(b | w);
    uint64_t best = 0;
    int v = OZ_MINIMAX_NONE, root = 0;
    if (empties <= max_empties) v = sv_position(L, valid, corners, lane, b, w, player[i], empties, &best, &root);
    values[(size_t)i * 64 + lane] = v;
    if (lane == 0) { bests[i] = best; value[i] = root; solved[i] = empties <= max_empties ? 1 : 0; }
}

OZ_API int oz_rules_solve(const uint64_t* black, const uint64_t* white, const int8_t* player, int n, int count, int max_empties,
                          int32_t* values, uint64_t* bests, int32_t* value, uint8_t* solved) {
    if (int rc = check_n(n)) return rc;
    OZ_REQUIRE(max_empties >= 0 && max_empties <= OZ_SOLVE_MAX_EMPTIES, "oz_rules_solve: max_empties %d outside 0..%d", max_empties, OZ_SOLVE_MAX_EMPTIES);
    if (count <= 0) return OZ_OK;
    OZ_REQUIRE(black && white && player, "null argument");
    const uint64_t valid = oz_valid_mask(n);
    for (int i = 0; i < count; ++i) {
        OZ_REQUIRE(player[i] == 1 || player[i] == -1, "player must be +1 or -1");
        OZ_REQUIRE(((black[i] | white[i]) & ~valid) == 0 && (black[i] & white[i]) == 0, "oz_rules_solve: position %d is no %dx%d board", i, n, n);
    }
    const size_t c8 = 8ull * count, c4 = pad8(4ull * count), c1 = pad8(count), cv = 256ull * count;
    // output image: values | bests | value | solved
    return rules_call(2 * c8 + c1, cv + c8 + c4 + c1,
        [&](unsigned char* h) { memcpy(h, black, c8); memcpy(h + c8, white, c8); memcpy(h + 2 * c8, player, count); },
        [&](unsigned char* di, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_solve, dim3(count), dim3(64), 0, s, (const uint64_t*)di, (const uint64_t*)(di + c8), (const int8_t*)(di + 2 * c8),
                               valid, oz_solve_corners(n), n * n, max_empties, (int32_t*)dout, (uint64_t*)(dout + cv), (int32_t*)(dout + cv + c8),
                               (uint8_t*)(dout + cv + c8 + c4));
        },
        [&](const unsigned char* h) {
            if (values) memcpy(values, h, cv);
            if (bests) memcpy(bests, h + cv, c8);
            if (value) memcpy(value, h + cv + c8, 4ull * count);
            if (solved) memcpy(solved, h + cv + c8 + c4, count);
        });
}

// the sign of S only: sv_root under the root window (-1, +1) (oz_solve.h), what a search leaf needs (k_solve_leaves, oz_search.hip)
__global__ __launch_bounds__(64) void k_solve_sign(const uint64_t* __restrict__ black, const uint64_t* __restrict__ white, const int8_t* __restrict__ player,
                                                   uint64_t valid, uint64_t corners, int n2, int max_empties, int8_t* __restrict__ sign,
                                                   uint8_t* __restrict__ solved) {
    __shared__ SolveLdsW L;
    const int i = blockIdx.x, lane = threadIdx.x;
    const uint64_t b = black[i], w = white[i];
    const int empties = n2 - oz_popc(b | w);
    int sg = 0;
    if (empties <= max_empties) sg = player[i] == 1 ? sv_sign(L, valid, corners, lane, b, w, empties) : sv_sign(L, valid, corners, lane, w, b, empties);
    if (lane == 0) { sign[i] = (int8_t)sg; solved[i] = empties <= max_empties ? 1 : 0; }
}

OZ_API int oz_rules_solve_sign(const uint64_t* black, const uint64_t* white, const int8_t* player, int n, int count, int max_empties,
                               int8_t* sign, uint8_t* solved) {
    if (int rc = check_n(n)) return rc;
    OZ_REQUIRE(max_empties >= 0 && max_empties <= OZ_SOLVE_MAX_EMPTIES, "oz_rules_solve_sign: max_empties %d outside 0..%d", max_empties, OZ_SOLVE_MAX_EMPTIES);
    if (count <= 0) return OZ_OK;
    OZ_REQUIRE(black && white && player, "null argument");
    const uint64_t valid = oz_valid_mask(n);
    for (int i = 0; i < count; ++i) {
        OZ_REQUIRE(player[i] == 1 || player[i] == -1, "player must be +1 or -1");
        OZ_REQUIRE(((black[i] | white[i]) & ~valid) == 0 && (black[i] & white[i]) == 0, "oz_rules_solve_sign: position %d is no %dx%d board", i, n, n);
    }
    const size_t c8 = 8ull * count, c1 = pad8(count);
    // output image: sign | solved
    return rules_call(2 * c8 + c1, 2 * c1,
        [&](unsigned char* h) { memcpy(h, black, c8); memcpy(h + c8, white, c8); memcpy(h + 2 * c8, player, count); },
        [&](unsigned char* di, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_solve_sign, dim3(count), dim3(64), 0, s, (const uint64_t*)di, (const uint64_t*)(di + c8), (const int8_t*)(di + 2 * c8),
                               valid, oz_solve_corners(n), n * n, max_empties, (int8_t*)dout, (uint8_t*)(dout + c1));
        },
        [&](const unsigned char* h) {
            if (sign) memcpy(sign, h, count);
            if (solved) memcpy(solved, h + c1, count);
        });
}

// ---------------------------------------------------------------- random openings (oz_openings.h; the reference has none)
// one thread per opening: the position it reaches and the squares it played (0 beyond n_plies)
__global__ void k_random_openings(int n, uint64_t valid, int count, int plies, uint64_t seed, uint64_t first_id, uint64_t* __restrict__ black,
                                  uint64_t* __restrict__ white, int32_t* __restrict__ n_plies, int8_t* __restrict__ player,
                                  uint8_t* __restrict__ finished, uint8_t* __restrict__ actions) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t b, w;
    int p, f;
    uint8_t* row = actions + (size_t)i * OZ_OPENING_MAX_PLIES;
    const int played = oz_opening_play(n, valid, plies, nullptr, seed, first_id + (uint64_t)i, b, w, p, f,
                                       [&](int ply, uint64_t, uint64_t, int, int action) { row[ply] = (uint8_t)action; });
    for (int k = played; k < OZ_OPENING_MAX_PLIES; ++k) row[k] = 0;
    black[i] = b; white[i] = w; n_plies[i] = played; player[i] = (int8_t)p; finished[i] = (uint8_t)f;
}

OZ_API int oz_rules_random_openings(int n, int64_t count64, int plies, uint64_t opening_seed, uint64_t first_opening_id, uint64_t* black,
                                    uint64_t* white, int8_t* player, uint8_t* finished, uint8_t* actions, int32_t* n_plies) {
    if (int rc = check_n(n)) return rc;
    OZ_REQUIRE(plies >= 0 && plies <= OZ_OPENING_MAX_PLIES, "oz_rules_random_openings: plies %d outside 0..%d", plies, OZ_OPENING_MAX_PLIES);
    OZ_REQUIRE(count64 >= 0 && count64 <= (1LL << 22), "oz_rules_random_openings: count %lld outside 0..2^22", (long long)count64);
    if (count64 == 0) return OZ_OK;
    const int count = (int)count64;
    const size_t c8 = 8ull * count, c4 = pad8(4ull * count), c1 = pad8(count), ca = (size_t)count * OZ_OPENING_MAX_PLIES;
    // no input but the scalars (eight bytes go up so that the one upload of rules_call has something to carry); output image:
    // black | white | n_plies | player | finished | actions
    return rules_call(8, 2 * c8 + c4 + 2 * c1 + ca,
        [&](unsigned char* h) { memset(h, 0, 8); },
        [&](unsigned char*, unsigned char* dout, hipStream_t s) {
            hipLaunchKernelGGL(k_random_openings, dim3(grid_for(count)), dim3(256), 0, s, n, oz_valid_mask(n), count, plies, opening_seed,
                               first_opening_id, (uint64_t*)dout, (uint64_t*)(dout + c8), (int32_t*)(dout + 2 * c8), (int8_t*)(dout + 2 * c8 + c4),
                               (uint8_t*)(dout + 2 * c8 + c4 + c1), (uint8_t*)(dout + 2 * c8 + c4 + 2 * c1));
        },
        [&](const unsigned char* h) {
            if (black) memcpy(black, h, c8);
            if (white) memcpy(white, h + c8, c8);
            if (n_plies) memcpy(n_plies, h + 2 * c8, 4ull * count);
            if (player) memcpy(player, h + 2 * c8 + c4, count);
            if (finished) memcpy(finished, h + 2 * c8 + c4 + c1, count);
            if (actions) memcpy(actions, h + 2 * c8 + c4 + 2 * c1, ca);
        });
}

// ---------------------------------------------------------------- symmetries (K8)
// (oz_sym_src, the source cell of an output cell under symmetry t, lives in oz_common.h: the replay buffer's append kernel shares it)

OZ_API int oz_symmetry_table(int n, int32_t* perm) {
    if (int rc = check_n(n)) return rc;
    for (int t = 0; t < 8; ++t)
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) perm[(t * n + r) * n + c] = oz_sym_src(t, n, r, c);
    return OZ_OK;
}

// one thread per output cell pair: boards[(rec*8+t)][r][c][0..1]; the policy index / z by the cell-0 thread
__global__ void k_expand(const oz_record* __restrict__ recs, int64_t count, int n, int alias_final,
                         uint8_t* __restrict__ boards, int32_t* __restrict__ pol, int8_t* __restrict__ z) {
    const int n2 = n * n;
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count * 8 * n2) return;
    const int cell = (int)(idx % n2);
    const int64_t ex = idx / n2;
    const int t = (int)(ex & 7);
    const oz_record rec = recs[ex >> 3];
    const int r = cell / n, c = cell % n;
    const int src = oz_sym_src(t, n, r, c), sr = src / n, sc = src % n;
    const uint64_t b = alias_final ? rec.final_black : rec.black, w = alias_final ? rec.final_white : rec.white;
    uchar2 o;
    o.x = (uint8_t)((b >> (sr * 8 + sc)) & 1); o.y = (uint8_t)((w >> (sr * 8 + sc)) & 1);
    reinterpret_cast<uchar2*>(boards)[idx] = o;
    const int a = (rec.action >> 3) * n + (rec.action & 7);
    if (src == a) pol[ex] = cell;             // the one-hot lands where its source cell is the action
    if (cell == 0) z[ex] = rec.z;
}

OZ_API int oz_examples_expand(const oz_record* records, int64_t count, int n, int alias_final, uint8_t* boards,
                              int32_t* policy_index, int8_t* z) {
    if (int rc = check_n(n)) return rc;
    if (count <= 0) return OZ_OK;
    oz_current_device();
    const int64_t nex = count * 8, cells = nex * n * n;
    DevBuf<oz_record> r; DevBuf<uint8_t> b; DevBuf<int32_t> p; DevBuf<int8_t> zz;
    OZ_HIP(r.alloc(count)); OZ_HIP(b.alloc(cells * 2)); OZ_HIP(p.alloc(nex)); OZ_HIP(zz.alloc(nex));
    OZ_HIP(hipMemcpy(r.p, records, sizeof(oz_record) * count, hipMemcpyHostToDevice));
    const int64_t blocks = (cells + 255) / 256;
    OZ_REQUIRE(blocks < (1ll << 31), "too many examples in one call");
    hipLaunchKernelGGL(k_expand, dim3((unsigned)blocks), dim3(256), 0, 0, r.p, count, n, alias_final, b.p, p.p, zz.p);
    OZ_HIP(hipGetLastError());
    OZ_HIP(hipMemcpy(boards, b.p, cells * 2, hipMemcpyDeviceToHost));
    OZ_HIP(hipMemcpy(policy_index, p.p, 4 * nex, hipMemcpyDeviceToHost));
    OZ_HIP(hipMemcpy(z, zz.p, nex, hipMemcpyDeviceToHost));
    return OZ_OK;
}

// (oz_count_pow, N ** (1 / T) of a visit count, lives in oz_common.h)
// one 64-lane block per record, lane = cell r*n+c of the record's own (n, n) view: pi of the root (pairwise np.sum by lane 0, as on the
// host), then for each of the 8 symmetries the output cell `lane` takes its source cell's value -- boards, pi and z of the 8 examples
__global__ __launch_bounds__(64) void k_expand_visits(const oz_record* __restrict__ recs, const int32_t* __restrict__ counts, int n, int alias_final,
                                                      double inv, int k, uint8_t* __restrict__ boards, double* __restrict__ pi, int8_t* __restrict__ z) {
    __shared__ double arr[64];
    __shared__ double divisor;
    const int64_t rix = blockIdx.x;
    const int lane = threadIdx.x, n2 = n * n;
    const int r = lane / n, c = lane % n;
    arr[lane] = lane < n2 ? oz_count_pow(counts[rix * 64 + r * 8 + c], inv, k) : 0.0;     // counts are 0 off the legal set
    __syncthreads();
    if (lane == 0) {
        const double sum = pairwise_sum(arr, n2);
        divisor = sum == 0 ? 1.0 : sum;
    }
    __syncthreads();
    const double q = arr[lane] / divisor;
    __syncthreads();
    arr[lane] = q;
    __syncthreads();
    if (lane >= n2) return;
    const oz_record rec = recs[rix];
    const uint64_t b = alias_final ? rec.final_black : rec.black, w = alias_final ? rec.final_white : rec.white;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int64_t ex = rix * 8 + t;
        const int src = oz_sym_src(t, n, r, c), sq = (src / n) * 8 + src % n;
        pi[ex * n2 + lane] = arr[src];
        uchar2 o;
        o.x = (uint8_t)((b >> sq) & 1); o.y = (uint8_t)((w >> sq) & 1);
        reinterpret_cast<uchar2*>(boards)[ex * n2 + lane] = o;
        if (lane == 0) z[ex] = rec.z;
    }
}

OZ_API int oz_examples_expand_visits(const oz_record* records, const int32_t* counts, int64_t count, int n, int alias_final, double temperature,
                                     uint8_t* boards, double* pi, int8_t* z) {
    if (int rc = check_n(n)) return rc;
    OZ_REQUIRE(temperature > 0, "oz_examples_expand_visits: temperature %g (the visit distribution needs T > 0)", temperature);
    if (count <= 0) return OZ_OK;
    OZ_REQUIRE(records && counts && boards && pi && z, "null argument");
    OZ_REQUIRE(count < (1ll << 31), "too many records in one call");
    oz_current_device();
    const int64_t nex = count * 8, cells = nex * n * n;
    DevBuf<oz_record> r; DevBuf<int32_t> cn; DevBuf<uint8_t> b; DevBuf<double> p; DevBuf<int8_t> zz;
    OZ_HIP(r.alloc(count)); OZ_HIP(cn.alloc(count * 64)); OZ_HIP(b.alloc(cells * 2)); OZ_HIP(p.alloc(cells)); OZ_HIP(zz.alloc(nex));
    OZ_HIP(hipMemcpy(r.p, records, sizeof(oz_record) * count, hipMemcpyHostToDevice));
    OZ_HIP(hipMemcpy(cn.p, counts, sizeof(int32_t) * 64 * count, hipMemcpyHostToDevice));
    const double inv = 1.0 / temperature;
    const int k = oz_count_pow_k(inv);
    hipLaunchKernelGGL(k_expand_visits, dim3((unsigned)count), dim3(64), 0, 0, r.p, cn.p, n, alias_final, inv, k, b.p, p.p, zz.p);
    OZ_HIP(hipGetLastError());
    OZ_HIP(hipMemcpy(boards, b.p, cells * 2, hipMemcpyDeviceToHost));
    OZ_HIP(hipMemcpy(pi, p.p, sizeof(double) * cells, hipMemcpyDeviceToHost));
    OZ_HIP(hipMemcpy(z, zz.p, nex, hipMemcpyDeviceToHost));
    return OZ_OK;
}

// the 8 symmetric examples of every record with a float32 policy row by square (rows[count][64], the improved policy of a Gumbel search): on the
// host, no device needed.  Example 8 i + t: boards and z as oz_examples_expand, pi[(8 i + t)][r][c] = the row's value at the source cell of (r, c)
// under symmetry t -- values are copied, never recomputed, so the rows are the record's bit for bit.
OZ_API int oz_examples_expand_policy(const oz_record* records, const float* rows, int64_t count, int n, int alias_final, uint8_t* boards, float* pi,
                                     int8_t* z) {
    if (int rc = check_n(n)) return rc;
    if (count <= 0) return OZ_OK;
    OZ_REQUIRE(records && rows && boards && pi && z, "null argument");
    const int n2 = n * n;
    for (int64_t i = 0; i < count; ++i) {
        const oz_record& rec = records[i];
        const uint64_t b = alias_final ? rec.final_black : rec.black, w = alias_final ? rec.final_white : rec.white;
        for (int t = 0; t < 8; ++t) {
            const int64_t ex = i * 8 + t;
            for (int cell = 0; cell < n2; ++cell) {
                const int src = oz_sym_src(t, n, cell / n, cell % n), sq = (src / n) * 8 + src % n;
                pi[ex * n2 + cell] = rows[i * 64 + sq];
                boards[(ex * n2 + cell) * 2] = (uint8_t)((b >> sq) & 1);
                boards[(ex * n2 + cell) * 2 + 1] = (uint8_t)((w >> sq) & 1);
            }
            z[ex] = rec.z;
        }
    }
    return OZ_OK;
}

// the auxiliary targets of `R` records (oz_aux_target, oz_common.h: the definition the replay buffer's append kernels evaluate): on the host,
// no device needed
OZ_API int oz_aux_targets(const oz_record* records, int64_t R, uint64_t* fin_own, uint64_t* fin_opp) {
    OZ_REQUIRE(R >= 0 && (R == 0 || (records && fin_own && fin_opp)), "oz_aux_targets: null argument or negative count");
    for (int64_t i = 0; i < R; ++i) oz_aux_target(records[i], fin_own[i], fin_opp[i]);
    return OZ_OK;
}
