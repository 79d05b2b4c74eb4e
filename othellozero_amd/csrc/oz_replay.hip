// oz_replay.hip -- the device-resident replay buffer (oz_replay_*): finished training examples in HBM, in the layout of the trainer's
// resident data set, appended device to device from a self-play engine's records (or from records / examples the host hands in) and read
// in place by oz_trainer_fit_epoch_replay (oz_train.hip).  What replaces, for callers that opt in, the host's list of example tuples
// (main.py:21-53 CircularArray + training.py:58-72) between the engines and the trainer.
#include <algorithm>
#include <numeric>

#include "oz_internal.h"

// ---------------------------------------------------------------- the append kernel
// One wavefront per record, fetched through `perm` (the (game_id, ply) order).  The record's 8 examples (symmetry t of oz_sym_src, the
// identity last) have the running indices base + 8 i + t; example e of the launch is dropped when e < skip (an append larger than the
// buffer keeps its last `capacity` examples) and otherwise lands in slot (base + e) % capacity: the kept ones are at most `capacity`
// consecutive running indices, so no two of a launch share a slot.
// Boards: lane = square row*8+col, so the transformed bitboard of a symmetry is ONE ballot of "my source square holds a disc".
// pi:     lane = cell row*n+col.  VISITS: the float64 row of k_expand_visits (oz_count_pow, lane 0's pairwise_sum, one division), rounded
//         once to float32, then every symmetry's output cell takes its source cell's value by a cross-lane read; ONEHOT: 1.0f where the
//         source cell is the action.  Stores of a row are contiguous over the lanes.
//         POLICY (the improved policy of a Gumbel search): `counts` holds the records' float32 rows by square, bit for bit in the int32 words;
//         every symmetry's output cell takes its source cell's value: a copy, no arithmetic.
// own / opp / z of example t are written by lane t: one 8-lane store each per record.  z = the record's z, or with zt (the records' value
// targets, indexed like recs) the record's float32 target.
// No atomics, no scratch, fixed order.
// AUX (a buffer of oz_replay_create_aux): the record's final pair (oz_aux_target: the final board from the mover's side, 0 / 0 without one) goes
// through the same ballots as the boards, and lane t stores example t's pair into fo / fp.  The other instantiations never touch fo / fp.
template <int N, bool VISITS, bool POLICY = false, bool AUX = false>
__global__ __launch_bounds__(64) void k_replay_append(const oz_record* __restrict__ recs, const int32_t* __restrict__ counts,
                                                      const int32_t* __restrict__ perm, int alias_final, double inv, int k, long long base,
                                                      long long skip, long long capacity, uint64_t* __restrict__ own,
                                                      uint64_t* __restrict__ opp, float* __restrict__ pi, float* __restrict__ z,
                                                      const float* __restrict__ zt, uint64_t* __restrict__ fo, uint64_t* __restrict__ fp) {
    constexpr int N2 = N * N;
    __shared__ double arr[64];
    __shared__ double divisor;
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    const int rix = perm[i];
    const oz_record rec = recs[rix];
    const uint64_t b = alias_final ? rec.final_black : rec.black, w = alias_final ? rec.final_white : rec.white;
    const int r8 = lane >> 3, c8 = lane & 7;                 // this lane as a square
    const bool on_board = r8 < N && c8 < N;
    const int rn = lane / N, cn = lane % N;                  // this lane as a cell of the (n, n) view
    const bool is_cell = lane < N2;
    float q32 = 0.f;
    if constexpr (VISITS) {
        arr[lane] = is_cell ? oz_count_pow(counts[(long long)rix * 64 + rn * 8 + cn], inv, k) : 0.0;     // counts are 0 off the legal set
        __syncthreads();
        if (lane == 0) {
            const double sum = pairwise_sum(arr, N2);
            divisor = sum == 0 ? 1.0 : sum;
        }
        __syncthreads();
        q32 = (float)(arr[lane] / divisor);
    }
    if constexpr (POLICY) q32 = is_cell ? __int_as_float(counts[(long long)rix * 64 + rn * 8 + cn]) : 0.f;
    const int action = (rec.action >> 3) * N + (rec.action & 7);
    uint64_t my_own = 0, my_opp = 0, fin_o = 0, fin_p = 0, my_fo = 0, my_fp = 0;
    if constexpr (AUX) oz_aux_target(rec, fin_o, fin_p);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int s8 = on_board ? oz_sym_src(t, N, r8, c8) : 0;
        const int sq = (s8 / N) * 8 + s8 % N;
        const uint64_t bo = __ballot(on_board && ((b >> sq) & 1)), bw = __ballot(on_board && ((w >> sq) & 1));
        if (lane == t) { my_own = bo; my_opp = bw; }
        if constexpr (AUX) {
            const uint64_t ao = __ballot(on_board && ((fin_o >> sq) & 1)), aw = __ballot(on_board && ((fin_p >> sq) & 1));
            if (lane == t) { my_fo = ao; my_fp = aw; }
        }
        const int src = is_cell ? oz_sym_src(t, N, rn, cn) : 0;
        float p;
        if constexpr (VISITS || POLICY) p = __shfl(q32, src);
        else p = src == action ? 1.0f : 0.0f;
        const long long e = i * 8 + t;
        if (is_cell && e >= skip) pi[((base + e) % capacity) * N2 + lane] = p;
    }
    const long long e = i * 8 + lane;
    if (lane < 8 && e >= skip) {
        const long long slot = (base + e) % capacity;
        own[slot] = my_own; opp[slot] = my_opp; z[slot] = zt ? zt[rix] : (float)rec.z;
        if constexpr (AUX) { fo[slot] = my_fo; fp[slot] = my_fp; }
    }
}

// The weighted append ("policy surprise weighting" in the header): record i of the permutation becomes copies[rix] examples instead of 8;
// example k of them is symmetry (first_sym[rix] + k) & 7 and has the running index base + off[i] + k, off = the exclusive prefix sum of the
// copy counts over the permutation.  The eight boards are made once, as above, and kept in LDS; the row of example k is computed for its
// symmetry (copies beyond 8 repeat symmetries).  skip / capacity as above; the kept examples of a launch are at most `capacity` consecutive
// running indices.  A record with no copy writes nothing.  One wavefront per record, no atomics, no scratch, fixed order.  AUX: as above, the
// eight final pairs kept in LDS beside the boards.
template <int N, bool VISITS, bool POLICY = false, bool AUX = false>
__global__ __launch_bounds__(64) void k_replay_append_w(const oz_record* __restrict__ recs, const int32_t* __restrict__ counts,
                                                        const int32_t* __restrict__ perm, int alias_final, double inv, int k, long long base,
                                                        long long skip, long long capacity, uint64_t* __restrict__ own,
                                                        uint64_t* __restrict__ opp, float* __restrict__ pi, float* __restrict__ z,
                                                        const float* __restrict__ zt, const int32_t* __restrict__ copies,
                                                        const uint8_t* __restrict__ first_sym, const long long* __restrict__ off,
                                                        uint64_t* __restrict__ fo, uint64_t* __restrict__ fp) {
    constexpr int N2 = N * N;
    __shared__ double arr[64];
    __shared__ double divisor;
    __shared__ uint64_t s_own[8], s_opp[8];
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    const int rix = perm[i];
    const int c = copies[rix], t0 = first_sym[rix] & 7;
    if (c <= 0) return;                                      // (the same for every lane)
    const long long e0 = off[i];
    const oz_record rec = recs[rix];
    const uint64_t b = alias_final ? rec.final_black : rec.black, w = alias_final ? rec.final_white : rec.white;
    const int r8 = lane >> 3, c8 = lane & 7;                 // this lane as a square
    const bool on_board = r8 < N && c8 < N;
    const int rn = lane / N, cn = lane % N;                  // this lane as a cell of the (n, n) view
    const bool is_cell = lane < N2;
    float q32 = 0.f;
    if constexpr (VISITS) {
        arr[lane] = is_cell ? oz_count_pow(counts[(long long)rix * 64 + rn * 8 + cn], inv, k) : 0.0;     // counts are 0 off the legal set
        __syncthreads();
        if (lane == 0) {
            const double sum = pairwise_sum(arr, N2);
            divisor = sum == 0 ? 1.0 : sum;
        }
        __syncthreads();
        q32 = (float)(arr[lane] / divisor);
    }
    if constexpr (POLICY) q32 = is_cell ? __int_as_float(counts[(long long)rix * 64 + rn * 8 + cn]) : 0.f;
    const int action = (rec.action >> 3) * N + (rec.action & 7);
    uint64_t* s_fin = nullptr;                               // AUX: [0 .. 7] fin_own, [8 .. 15] fin_opp of the eight symmetries
    uint64_t fin_o = 0, fin_p = 0;
    if constexpr (AUX) {
        __shared__ uint64_t s_fin_buf[16];
        s_fin = s_fin_buf;
        oz_aux_target(rec, fin_o, fin_p);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int s8 = on_board ? oz_sym_src(t, N, r8, c8) : 0;
        const int sq = (s8 / N) * 8 + s8 % N;
        const uint64_t bo = __ballot(on_board && ((b >> sq) & 1)), bw = __ballot(on_board && ((w >> sq) & 1));
        if (lane == t) { s_own[t] = bo; s_opp[t] = bw; }
        if constexpr (AUX) {
            const uint64_t ao = __ballot(on_board && ((fin_o >> sq) & 1)), aw = __ballot(on_board && ((fin_p >> sq) & 1));
            if (lane == t) { s_fin[t] = ao; s_fin[8 + t] = aw; }
        }
    }
    __syncthreads();
    for (int kk = 0; kk < c; ++kk) {
        const int t = (t0 + kk) & 7;
        const int src = is_cell ? oz_sym_src(t, N, rn, cn) : 0;
        float p;
        if constexpr (VISITS || POLICY) p = __shfl(q32, src);
        else p = src == action ? 1.0f : 0.0f;
        const long long e = e0 + kk;
        if (is_cell && e >= skip) pi[((base + e) % capacity) * N2 + lane] = p;
    }
    const float zv = zt ? zt[rix] : (float)rec.z;
    for (int kk = lane; kk < c; kk += 64) {
        const long long e = e0 + kk;
        if (e >= skip) {
            const int t = (t0 + kk) & 7;
            const long long slot = (base + e) % capacity;
            own[slot] = s_own[t]; opp[slot] = s_opp[t]; z[slot] = zv;
            if constexpr (AUX) { fo[slot] = s_fin[t]; fp[slot] = s_fin[8 + t]; }
        }
    }
}

// ---------------------------------------------------------------- the object
#define R_LOCK(r) std::lock_guard<std::mutex> rlock__((r)->mu)

static int replay_create(oz_replay** out, int n, int64_t capacity, bool aux) {
    OZ_REQUIRE(out, "oz_replay_create: null argument");
    OZ_REQUIRE(n == 4 || n == 6 || n == 8, "oz_replay_create: board size must be 4, 6 or 8 (got %d)", n);
    OZ_REQUIRE(capacity >= 1 && capacity < (1ll << 31), "oz_replay_create: capacity %lld outside [1, 2^31 - 1] examples", (long long)capacity);
    oz_replay* r = new oz_replay();
    r->n = n; r->capacity = capacity; r->device = oz_current_device();
    auto fail = [&](hipError_t e) {
        oz_set_error("oz_replay_create: %s (%lld examples of %d bytes)", hipGetErrorString(e), (long long)capacity, 24 + 4 * n * n);
        oz_replay_destroy(r);
        return OZ_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(r->device)) != hipSuccess) return fail(e);
    if ((e = hipStreamCreateWithFlags(&r->s, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&r->own, sizeof(uint64_t) * capacity)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&r->opp, sizeof(uint64_t) * capacity)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&r->pi, sizeof(float) * capacity * n * n)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&r->z, sizeof(float) * capacity)) != hipSuccess) return fail(e);
    if (aux) {
        if ((e = hipMalloc((void**)&r->fo, sizeof(uint64_t) * capacity)) != hipSuccess) return fail(e);
        if ((e = hipMalloc((void**)&r->fp, sizeof(uint64_t) * capacity)) != hipSuccess) return fail(e);
    }
    *out = r;
    return OZ_OK;
}
OZ_API int oz_replay_create(oz_replay** out, int n, int64_t capacity) { return replay_create(out, n, capacity, false); }
OZ_API int oz_replay_create_aux(oz_replay** out, int n, int64_t capacity) { return replay_create(out, n, capacity, true); }
OZ_API int oz_replay_has_aux(oz_replay* r, int* aux) {
    OZ_REQUIRE(r && aux, "oz_replay_has_aux: null argument");
    *aux = r->fo ? 1 : 0;
    return OZ_OK;
}

OZ_API int oz_replay_destroy(oz_replay* r) {
    if (!r) return OZ_OK;
    hipSetDevice(r->device);
    if (r->s) hipStreamSynchronize(r->s);
    for (void* q : {(void*)r->own, (void*)r->opp, (void*)r->pi, (void*)r->z, (void*)r->fo, (void*)r->fp, (void*)r->st_rec, (void*)r->st_cnt, (void*)r->st_perm, (void*)r->st_tgt, (void*)r->st_cpy, (void*)r->st_sym, (void*)r->st_off}) if (q) hipFree(q);
    if (r->s) hipStreamDestroy(r->s);
    delete r;
    return OZ_OK;
}

OZ_API int oz_replay_clear(oz_replay* r) {
    OZ_REQUIRE(r, "oz_replay_clear: null replay buffer");
    R_LOCK(r);
    r->total = 0;
    return OZ_OK;
}

OZ_API int oz_replay_info(oz_replay* r, int64_t* held, int64_t* capacity, int64_t* total) {
    OZ_REQUIRE(r, "oz_replay_info: null replay buffer");
    R_LOCK(r);
    if (held) *held = r->held();
    if (capacity) *capacity = r->capacity;
    if (total) *total = r->total;
    return OZ_OK;
}

// room for `records` staged records (+ their permutation) and `count_rows` visit-count rows
static int replay_reserve(oz_replay* r, int64_t records, int64_t count_rows, int64_t target_rows = 0) {
    if (target_rows > r->st_tgt_cap) {
        if (r->st_tgt) hipFree(r->st_tgt);
        r->st_tgt = nullptr; r->st_tgt_cap = 0;
        OZ_HIP(hipMalloc((void**)&r->st_tgt, sizeof(float) * target_rows));
        r->st_tgt_cap = target_rows;
    }
    if (records > r->st_rec_cap) {
        if (r->st_rec) { hipFree(r->st_rec); hipFree(r->st_perm); }
        r->st_rec = nullptr; r->st_perm = nullptr; r->st_rec_cap = 0;
        OZ_HIP(hipMalloc((void**)&r->st_rec, sizeof(oz_record) * records));
        OZ_HIP(hipMalloc((void**)&r->st_perm, sizeof(int32_t) * records));
        r->st_rec_cap = records;
    }
    if (count_rows > r->st_cnt_cap) {
        if (r->st_cnt) hipFree(r->st_cnt);
        r->st_cnt = nullptr; r->st_cnt_cap = 0;
        OZ_HIP(hipMalloc((void**)&r->st_cnt, sizeof(int32_t) * 64 * count_rows));
        r->st_cnt_cap = count_rows;
    }
    return OZ_OK;
}

// room for the copy counts, first symmetries and example offsets of `records` staged records (the weighted append)
static int replay_reserve_weighted(oz_replay* r, int64_t records) {
    if (records <= r->st_w_cap) return OZ_OK;
    for (void* q : {(void*)r->st_cpy, (void*)r->st_sym, (void*)r->st_off}) if (q) hipFree(q);
    r->st_cpy = nullptr; r->st_sym = nullptr; r->st_off = nullptr; r->st_w_cap = 0;
    OZ_HIP(hipMalloc((void**)&r->st_cpy, sizeof(int32_t) * records));
    OZ_HIP(hipMalloc((void**)&r->st_sym, (size_t)records));
    OZ_HIP(hipMalloc((void**)&r->st_off, sizeof(long long) * records));
    r->st_w_cap = records;
    return OZ_OK;
}

static int replay_check_target(const char* who, int alias_final, int target, double temperature, bool engine = false) {
    OZ_REQUIRE(alias_final == 0 || alias_final == 1, "%s: alias_final = %d (0 or 1)", who, alias_final);
    OZ_REQUIRE(target != OZ_REPLAY_TARGET_POLICY || engine, "%s: OZ_REPLAY_TARGET_POLICY is offered for an engine's records only (oz_replay_append_selfplay)", who);
    OZ_REQUIRE(target == OZ_REPLAY_TARGET_ONEHOT || target == OZ_REPLAY_TARGET_VISITS || target == OZ_REPLAY_TARGET_POLICY,
               "%s: target = %d (OZ_REPLAY_TARGET_ONEHOT, OZ_REPLAY_TARGET_VISITS or OZ_REPLAY_TARGET_POLICY)", who, target);
    OZ_REQUIRE(target != OZ_REPLAY_TARGET_VISITS || temperature > 0, "%s: temperature %g (the visit distribution needs T > 0)", who, temperature);
    return OZ_OK;
}

template <int N, bool AUX> static void replay_launch(oz_replay* r, int64_t count, int alias_final, int target, double inv, int k, long long skip, const float* zt) {
    const dim3 grid((unsigned)count), block(64);
    if (target == OZ_REPLAY_TARGET_POLICY)
        hipLaunchKernelGGL((k_replay_append<N, false, true, AUX>), grid, block, 0, r->s, r->st_rec, r->st_cnt, r->st_perm, alias_final, inv, k, (long long)r->total, skip,
                           (long long)r->capacity, r->own, r->opp, r->pi, r->z, zt, r->fo, r->fp);
    else if (target == OZ_REPLAY_TARGET_VISITS)
        hipLaunchKernelGGL((k_replay_append<N, true, false, AUX>), grid, block, 0, r->s, r->st_rec, r->st_cnt, r->st_perm, alias_final, inv, k, (long long)r->total, skip,
                           (long long)r->capacity, r->own, r->opp, r->pi, r->z, zt, r->fo, r->fp);
    else
        hipLaunchKernelGGL((k_replay_append<N, false, false, AUX>), grid, block, 0, r->s, r->st_rec, (const int32_t*)nullptr, r->st_perm, alias_final, inv, k,
                           (long long)r->total, skip, (long long)r->capacity, r->own, r->opp, r->pi, r->z, zt, r->fo, r->fp);
}

template <int N, bool AUX> static void replay_launch_w(oz_replay* r, int64_t count, int alias_final, int target, double inv, int k, long long skip, const float* zt) {
    const dim3 grid((unsigned)count), block(64);
    if (target == OZ_REPLAY_TARGET_POLICY)
        hipLaunchKernelGGL((k_replay_append_w<N, false, true, AUX>), grid, block, 0, r->s, r->st_rec, r->st_cnt, r->st_perm, alias_final, inv, k, (long long)r->total, skip,
                           (long long)r->capacity, r->own, r->opp, r->pi, r->z, zt, r->st_cpy, r->st_sym, r->st_off, r->fo, r->fp);
    else if (target == OZ_REPLAY_TARGET_VISITS)
        hipLaunchKernelGGL((k_replay_append_w<N, true, false, AUX>), grid, block, 0, r->s, r->st_rec, r->st_cnt, r->st_perm, alias_final, inv, k, (long long)r->total, skip,
                           (long long)r->capacity, r->own, r->opp, r->pi, r->z, zt, r->st_cpy, r->st_sym, r->st_off, r->fo, r->fp);
    else
        hipLaunchKernelGGL((k_replay_append_w<N, false, false, AUX>), grid, block, 0, r->s, r->st_rec, (const int32_t*)nullptr, r->st_perm, alias_final, inv, k,
                           (long long)r->total, skip, (long long)r->capacity, r->own, r->opp, r->pi, r->z, zt, r->st_cpy, r->st_sym, r->st_off, r->fo, r->fp);
}

// the staged records [first, first + count) of r->st_rec (host copy: h[0 .. count)) -> 8 examples each, in ascending (game_id, ply).  The fast
// records of a playout cap (pad[0] != 0) are no training examples: they stay out of the permutation, so the kernel never sees them;
// *kept = the records appended.
static int replay_append_staged(oz_replay* r, const oz_record* h, int64_t first, int64_t staged, int alias_final, int target, double temperature,
                                int64_t* kept, const float* zt = nullptr, const int32_t* hc = nullptr, int64_t* examples = nullptr) {
    // hc (the weighted append): the staged records' copy counts on the host, hc[0 .. staged), their device copy in r->st_cpy / r->st_sym
    std::vector<int32_t> perm;
    perm.reserve((size_t)staged);
    for (int64_t i = 0; i < staged; ++i)
        if (h[i].pad[0] == 0) perm.push_back((int32_t)i);
    const int64_t count = (int64_t)perm.size();
    *kept = count;
    if (count == 0) return OZ_OK;
    std::stable_sort(perm.begin(), perm.end(), [h](int32_t a, int32_t b) {
        return h[a].game_id != h[b].game_id ? h[a].game_id < h[b].game_id : h[a].ply < h[b].ply;
    });
    for (int32_t& p : perm) p += (int32_t)first;
    const double inv = target == OZ_REPLAY_TARGET_VISITS ? 1.0 / temperature : 1.0;
    const int k = oz_count_pow_k(inv);
    std::vector<long long> off;
    long long E = 8 * (long long)count;
    if (hc) {                                                  // the exclusive prefix sum of the copy counts over the permutation
        off.resize((size_t)count);
        E = 0;
        for (int64_t i = 0; i < count; ++i) { off[(size_t)i] = E; E += hc[perm[(size_t)i] - first] > 0 ? hc[perm[(size_t)i] - first] : 0; }
    }
    if (examples) *examples = E;
    const long long skip = E > r->capacity ? E - r->capacity : 0;
    hipError_t e = hipMemcpyAsync(r->st_perm, perm.data(), sizeof(int32_t) * count, hipMemcpyHostToDevice, r->s);
    if (e == hipSuccess && hc) e = hipMemcpyAsync(r->st_off, off.data(), sizeof(long long) * count, hipMemcpyHostToDevice, r->s);
    if (e == hipSuccess && hc) {
        switch (r->n * 2 + (r->fo ? 1 : 0)) {
        case 8: replay_launch_w<4, false>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 9: replay_launch_w<4, true>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 12: replay_launch_w<6, false>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 13: replay_launch_w<6, true>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 16: replay_launch_w<8, false>(r, count, alias_final, target, inv, k, skip, zt); break;
        default: replay_launch_w<8, true>(r, count, alias_final, target, inv, k, skip, zt);
        }
        e = hipGetLastError();
    } else if (e == hipSuccess) {
        switch (r->n * 2 + (r->fo ? 1 : 0)) {
        case 8: replay_launch<4, false>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 9: replay_launch<4, true>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 12: replay_launch<6, false>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 13: replay_launch<6, true>(r, count, alias_final, target, inv, k, skip, zt); break;
        case 16: replay_launch<8, false>(r, count, alias_final, target, inv, k, skip, zt); break;
        default: replay_launch<8, true>(r, count, alias_final, target, inv, k, skip, zt);
        }
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(r->s);          // whatever happened: `perm` and the caller's arrays may go away
    OZ_HIP(e);
    OZ_HIP(es);
    r->total += E;
    return OZ_OK;
}

static int replay_append_selfplay(oz_replay* r, oz_selfplay* sp, int64_t first_record, int alias_final, int target, double temperature,
                                  int64_t* appended_records, bool targets, bool weighted = false, int64_t* appended_examples = nullptr) {
    OZ_REQUIRE(r && sp, "oz_replay_append_selfplay: null argument");
    if (int rc = replay_check_target("oz_replay_append_selfplay", alias_final, target, temperature, true)) return rc;
    OZ_REQUIRE(first_record >= 0, "oz_replay_append_selfplay: first_record %lld", (long long)first_record);
    R_LOCK(r);
    int n = 0, device = 0, record_visits = 0;
    int64_t completed = 0;
    if (int rc = oz_selfplay_replay_facts(sp, &n, &device, &record_visits, &completed)) return rc;       // waits for the engine's stream
    OZ_REQUIRE(n == r->n, "oz_replay_append_selfplay: the engine plays %d x %d, the replay buffer holds %d x %d examples", n, n, r->n, r->n);
    OZ_REQUIRE(device == r->device, "oz_replay_append_selfplay: the engine lives on device %d, the replay buffer on device %d", device, r->device);
    const bool visits = target == OZ_REPLAY_TARGET_VISITS, policy = target == OZ_REPLAY_TARGET_POLICY;
    OZ_REQUIRE(!visits || record_visits, "oz_replay_append_selfplay: this engine does not record visit counts: create it with oz_selfplay_config.record_visits = 1");
    OZ_REQUIRE(!policy || oz_selfplay_has_gumbel(sp), "oz_replay_append_selfplay: target OZ_REPLAY_TARGET_POLICY needs an engine with the Gumbel search (oz_selfplay_set_gumbel)");
    if (appended_records) *appended_records = 0;
    if (appended_examples) *appended_examples = 0;
    if (completed <= first_record) return OZ_OK;
    OZ_HIP(hipSetDevice(r->device));
    if (int rc = replay_reserve(r, completed, visits || policy ? completed : 0, targets ? completed : 0)) return rc;
    if (weighted) { if (int rc = replay_reserve_weighted(r, completed)) return rc; }
    int64_t got = 0, got_rows = 0;
    if (int rc = oz_selfplay_records_device(sp, r->st_rec, completed, &got)) return rc;
    if (visits) {
        if (int rc = oz_selfplay_visits_device(sp, r->st_cnt, got, &got_rows)) return rc;
        if (got_rows < got) got = got_rows;
    }
    if (policy) {                                // the float32 rows into the staging of the int32 count rows: 256 B each, either way
        if (int rc = oz_selfplay_policies_device(sp, r->st_cnt, got, &got_rows)) return rc;
        if (got_rows < got) got = got_rows;
    }
    if (targets) {
        if (int rc = oz_selfplay_targets_device(sp, r->st_tgt, got, &got_rows)) return rc;
        if (got_rows < got) got = got_rows;
    }
    if (weighted) {
        if (int rc = oz_selfplay_copies_device(sp, r->st_cpy, r->st_sym, got, &got_rows)) return rc;
        if (got_rows < got) got = got_rows;
    }
    OZ_HIP(hipStreamSynchronize(nullptr));       // the engine's device-to-device copies ran on the null stream
    const int64_t count = got - first_record;
    if (count <= 0) return OZ_OK;
    std::vector<oz_record> h((size_t)count);     // 48 B per record: 2 % of the example bytes; the examples never leave the device
    OZ_HIP(hipMemcpyAsync(h.data(), r->st_rec + first_record, sizeof(oz_record) * count, hipMemcpyDeviceToHost, r->s));
    std::vector<int32_t> hc;                     // ... and, weighted, 4 B more: their copy counts, for the offsets
    if (weighted) {
        hc.resize((size_t)count);
        OZ_HIP(hipMemcpyAsync(hc.data(), r->st_cpy + first_record, sizeof(int32_t) * count, hipMemcpyDeviceToHost, r->s));
    }
    OZ_HIP(hipStreamSynchronize(r->s));
    int64_t kept = 0;
    if (int rc = replay_append_staged(r, h.data(), first_record, count, alias_final, target, temperature, &kept, targets ? r->st_tgt : nullptr,
                                      weighted ? hc.data() : nullptr, appended_examples)) return rc;
    if (appended_records) *appended_records = kept;
    return OZ_OK;
}
OZ_API int oz_replay_append_selfplay_weighted(oz_replay* r, oz_selfplay* sp, int64_t first_record, int alias_final, int target, double temperature,
                                              int value_targets, int64_t* appended_records, int64_t* appended_examples) {
    OZ_REQUIRE(value_targets == 0 || value_targets == 1, "oz_replay_append_selfplay_weighted: value_targets = %d (0 or 1)", value_targets);
    return replay_append_selfplay(r, sp, first_record, alias_final, target, temperature, appended_records, value_targets != 0, true, appended_examples);
}
OZ_API int oz_replay_append_selfplay(oz_replay* r, oz_selfplay* sp, int64_t first_record, int alias_final, int target, double temperature,
                                     int64_t* appended_records) {
    return replay_append_selfplay(r, sp, first_record, alias_final, target, temperature, appended_records, false);
}
OZ_API int oz_replay_append_selfplay_targets(oz_replay* r, oz_selfplay* sp, int64_t first_record, int alias_final, int target, double temperature,
                                             int64_t* appended_records) {
    return replay_append_selfplay(r, sp, first_record, alias_final, target, temperature, appended_records, true);
}

static int replay_append_records(oz_replay* r, const oz_record* records, const int32_t* counts, const float* values, int64_t count, int alias_final,
                                 int target, double temperature) {
    OZ_REQUIRE(r, "oz_replay_append_records: null replay buffer");
    if (int rc = replay_check_target("oz_replay_append_records", alias_final, target, temperature)) return rc;
    const bool visits = target == OZ_REPLAY_TARGET_VISITS;
    OZ_REQUIRE(count >= 0 && count < (1ll << 28), "oz_replay_append_records: %lld records in one call", (long long)count);
    OZ_REQUIRE(!visits || counts || count == 0, "oz_replay_append_records: OZ_REPLAY_TARGET_VISITS needs the records' visit counts (counts == NULL)");
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(records, "oz_replay_append_records: null records");
    R_LOCK(r);
    OZ_HIP(hipSetDevice(r->device));
    if (int rc = replay_reserve(r, count, visits ? count : 0, values ? count : 0)) return rc;
    OZ_HIP(hipMemcpyAsync(r->st_rec, records, sizeof(oz_record) * count, hipMemcpyHostToDevice, r->s));
    if (values) OZ_HIP(hipMemcpyAsync(r->st_tgt, values, sizeof(float) * count, hipMemcpyHostToDevice, r->s));
    if (visits) OZ_HIP(hipMemcpyAsync(r->st_cnt, counts, sizeof(int32_t) * 64 * count, hipMemcpyHostToDevice, r->s));
    int64_t kept = 0;
    const int rc = replay_append_staged(r, records, 0, count, alias_final, target, temperature, &kept, values ? r->st_tgt : nullptr);
    const hipError_t es = hipStreamSynchronize(r->s);          // (nothing kept: no launch waited for the uploads, and the caller's arrays may go away)
    if (rc) return rc;
    OZ_HIP(es);
    return OZ_OK;
}
OZ_API int oz_replay_append_records(oz_replay* r, const oz_record* records, const int32_t* counts, int64_t count, int alias_final, int target,
                                    double temperature) {
    return replay_append_records(r, records, counts, nullptr, count, alias_final, target, temperature);
}
OZ_API int oz_replay_append_records_values(oz_replay* r, const oz_record* records, const int32_t* counts, const float* values, int64_t count,
                                           int alias_final, int target, double temperature) {
    OZ_REQUIRE(values || count == 0, "oz_replay_append_records_values: null values");
    return replay_append_records(r, records, counts, values, count, alias_final, target, temperature);
}

// `count` rows of `width` bytes from the host into the ring at running index `k0` (count <= capacity): at most two pieces
static int replay_ring_upload(oz_replay* r, void* dst, const void* src, size_t width, int64_t k0, int64_t count) {
    const int64_t s0 = k0 % r->capacity, head = std::min(count, r->capacity - s0);
    OZ_HIP(hipMemcpyAsync((char*)dst + width * s0, src, width * head, hipMemcpyHostToDevice, r->s));
    if (count > head) OZ_HIP(hipMemcpyAsync(dst, (const char*)src + width * head, width * (count - head), hipMemcpyHostToDevice, r->s));
    return OZ_OK;
}

// `count` rows of `width` zero bytes into the ring at running index `k0` (count <= capacity)
static int replay_ring_zero(oz_replay* r, void* dst, size_t width, int64_t k0, int64_t count) {
    const int64_t s0 = k0 % r->capacity, head = std::min(count, r->capacity - s0);
    OZ_HIP(hipMemsetAsync((char*)dst + width * s0, 0, width * head, r->s));
    if (count > head) OZ_HIP(hipMemsetAsync(dst, 0, width * (count - head), r->s));
    return OZ_OK;
}

// fin_own / fin_opp: the examples' final pairs for a buffer that keeps them (NULL: zero pairs, "no auxiliary target"); a plain buffer ignores them
static int replay_append_examples_locked(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, int64_t count,
                                         const uint64_t* fin_own = nullptr, const uint64_t* fin_opp = nullptr) {
    OZ_HIP(hipSetDevice(r->device));
    const int64_t skip = count > r->capacity ? count - r->capacity : 0, kept = count - skip, k0 = r->total + skip;
    const size_t A = (size_t)r->n * r->n;
    int rc = replay_ring_upload(r, r->own, own + skip, sizeof(uint64_t), k0, kept);
    if (!rc) rc = replay_ring_upload(r, r->opp, opp + skip, sizeof(uint64_t), k0, kept);
    if (!rc) rc = replay_ring_upload(r, r->pi, pi + skip * A, sizeof(float) * A, k0, kept);
    if (!rc) rc = replay_ring_upload(r, r->z, z + skip, sizeof(float), k0, kept);
    if (!rc && r->fo && fin_own) {
        rc = replay_ring_upload(r, r->fo, fin_own + skip, sizeof(uint64_t), k0, kept);
        if (!rc) rc = replay_ring_upload(r, r->fp, fin_opp + skip, sizeof(uint64_t), k0, kept);
    } else if (!rc && r->fo) {
        rc = replay_ring_zero(r, r->fo, sizeof(uint64_t), k0, kept);
        if (!rc) rc = replay_ring_zero(r, r->fp, sizeof(uint64_t), k0, kept);
    }
    hipError_t e = hipStreamSynchronize(r->s);   // the host arrays may go away, whatever happened
    if (rc) return rc;
    OZ_HIP(e);
    r->total += count;
    return OZ_OK;
}

OZ_API int oz_replay_append_examples(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, int64_t count) {
    OZ_REQUIRE(r, "oz_replay_append_examples: null replay buffer");
    OZ_REQUIRE(count >= 0, "oz_replay_append_examples: count %lld", (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(own && opp && pi && z, "oz_replay_append_examples: null argument");
    R_LOCK(r);
    return replay_append_examples_locked(r, own, opp, pi, z, count);
}

OZ_API int oz_replay_append_examples_aux(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z,
                                         const uint64_t* fin_own, const uint64_t* fin_opp, int64_t count) {
    OZ_REQUIRE(r, "oz_replay_append_examples_aux: null replay buffer");
    OZ_REQUIRE(count >= 0, "oz_replay_append_examples_aux: count %lld", (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(own && opp && pi && z && fin_own && fin_opp, "oz_replay_append_examples_aux: null argument");
    R_LOCK(r);
    return replay_append_examples_locked(r, own, opp, pi, z, count, fin_own, fin_opp);
}

static int replay_restore(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, const uint64_t* fin_own,
                          const uint64_t* fin_opp, int64_t count, int64_t total) {
    OZ_REQUIRE(r, "oz_replay_restore: null replay buffer");
    R_LOCK(r);
    OZ_REQUIRE(total >= 0 && count == (total < r->capacity ? total : r->capacity),
               "oz_replay_restore: %lld examples for a running index of %lld in a buffer of %lld (wanted: min(total, capacity))", (long long)count,
               (long long)total, (long long)r->capacity);
    OZ_REQUIRE(count == 0 || (own && opp && pi && z), "oz_replay_restore: null argument");
    r->total = total - count;
    if (count == 0) return OZ_OK;
    if (int rc = replay_append_examples_locked(r, own, opp, pi, z, count, fin_own, fin_opp)) { r->total = 0; return rc; }
    return OZ_OK;
}
OZ_API int oz_replay_restore(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, int64_t count, int64_t total) {
    return replay_restore(r, own, opp, pi, z, nullptr, nullptr, count, total);
}
OZ_API int oz_replay_restore_aux(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, const uint64_t* fin_own,
                                 const uint64_t* fin_opp, int64_t count, int64_t total) {
    OZ_REQUIRE(count == 0 || (fin_own && fin_opp), "oz_replay_restore_aux: null argument");
    return replay_restore(r, own, opp, pi, z, fin_own, fin_opp, count, total);
}

OZ_API int oz_replay_read(oz_replay* r, int64_t first_slot, int64_t count, uint64_t* own, uint64_t* opp, float* pi, float* z) {
    OZ_REQUIRE(r, "oz_replay_read: null replay buffer");
    R_LOCK(r);
    OZ_REQUIRE(first_slot >= 0 && count >= 0 && first_slot + count <= r->held(), "oz_replay_read: slots [%lld, %lld) but the buffer holds %lld examples",
               (long long)first_slot, (long long)(first_slot + count), (long long)r->held());
    if (count == 0) return OZ_OK;
    OZ_HIP(hipSetDevice(r->device));
    const size_t A = (size_t)r->n * r->n;
    if (own) OZ_HIP(hipMemcpyAsync(own, r->own + first_slot, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, r->s));
    if (opp) OZ_HIP(hipMemcpyAsync(opp, r->opp + first_slot, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, r->s));
    if (pi) OZ_HIP(hipMemcpyAsync(pi, r->pi + first_slot * A, sizeof(float) * A * count, hipMemcpyDeviceToHost, r->s));
    if (z) OZ_HIP(hipMemcpyAsync(z, r->z + first_slot, sizeof(float) * count, hipMemcpyDeviceToHost, r->s));
    OZ_HIP(hipStreamSynchronize(r->s));
    return OZ_OK;
}

// the final pairs of `count` slots from `first_slot` on, of a buffer that keeps them (oz_replay_create_aux; OZ_ERR_STATE otherwise)
OZ_API int oz_replay_read_aux(oz_replay* r, int64_t first_slot, int64_t count, uint64_t* fin_own, uint64_t* fin_opp) {
    OZ_REQUIRE(r, "oz_replay_read_aux: null replay buffer");
    R_LOCK(r);
    if (!r->fo) { oz_set_error("oz_replay_read_aux: this replay buffer keeps no final pairs (oz_replay_create_aux)"); return OZ_ERR_STATE; }
    OZ_REQUIRE(first_slot >= 0 && count >= 0 && first_slot + count <= r->held(), "oz_replay_read_aux: slots [%lld, %lld) but the buffer holds %lld examples",
               (long long)first_slot, (long long)(first_slot + count), (long long)r->held());
    if (count == 0) return OZ_OK;
    OZ_HIP(hipSetDevice(r->device));
    if (fin_own) OZ_HIP(hipMemcpyAsync(fin_own, r->fo + first_slot, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, r->s));
    if (fin_opp) OZ_HIP(hipMemcpyAsync(fin_opp, r->fp + first_slot, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, r->s));
    OZ_HIP(hipStreamSynchronize(r->s));
    return OZ_OK;
}
