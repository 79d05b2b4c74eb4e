// oz_search.hip -- PUCT search (K4-K7, K13), self-play and arena drivers for gfx950.
//
// Replaces MCTS/__init__.py:19-187 + othelo_mcts.py:9-88 (search) and training.py:26-72,
// agents.py:44-84 (drivers).  Design (MI355X-first, not a translation):
//   * every game owns one OthelloMCTS instance = one open-addressing table keyed by the exact
//     128-bit (own, opp) pair (replaces sha1, MCTS/__init__.py:7-16) plus a pool of fixed-stride node
//     records (header + visit / Q / P rows, see "tree storage"), all resident in HBM; nothing is rebuilt
//     between moves (sub-tree / transposition reuse);
//   * ONE WAVEFRONT PER GAME: lane == board square.  PUCT argmax (MCTS/__init__.py:65,168-170)
//     is a 64-lane max-reduction + ballot, lowest lane wins ties (== Python's first maximum in
//     ascending square order); a node record reaches LDS in one wave-wide load and the descent's
//     frontier stays in LDS; table probes are 64-wide ballots; the backup walks all path levels in
//     parallel (one lane per level);
//   * lock step: every active game advances exactly one simulation per step (simulations of one
//     game are sequential in the reference; no virtual loss), leaves that need the network are
//     compacted by ballot + prefix sum into one dense batch (deterministic slot order), evaluated
//     by one NN launch sequence, then expanded / backed up; opt-in (oz_mcts_set_leaves_per_step): K descents per game and step under a
//     virtual loss, the k_wide_* kernels below -- the default and every golden fixture stay on one descent per step;
//   * float semantics that decide discrete outcomes are restated exactly (SURVEY.md R-FP):
//     U in float64 evaluated left to right with no FMA contraction, P normalised with NumPy's
//     pairwise order, Q accumulated in the dynamic type NumPy would use (q_mode).
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include "oz_internal.h"
#include "oz_minimax.h"
#include "oz_openings.h"
#include "oz_solve.h"

enum { VT_INT = 0, VT_F32 = 1, VT_F64 = 2 };
#define OZ_MAX_DEPTH 64
#define OZ_TAG_F32 0x80000000u
#define OZ_NSTAT 5
enum { ST_SIMS = 0, ST_VISITS = 1, ST_EXPAND = 2, ST_TERMINAL = 3, ST_FALLBACK = 4 };
enum { EF_NODES = 1, EF_EDGES = 2, EF_DEPTH = 4, EF_NOMOVE = 8, EF_RECORDS = 16, EF_ROOT = 32, EF_CORRUPT = 64 };

// ---------------------------------------------------------------- tree storage (per game: one OthelloMCTS instance)
// One fixed-stride RECORD per node, addressed by the node index alone:
//     [ header 32 B: own u64 | opp u64 | Ns i32 | cnt i32 | pad ][ cnt edges x 24 B: N|tag u32, child i32, Q f64, P f64 ]
// edges in ascending square order of the legal set (rank = popcount of the legal bits below the square).  rec_bytes is a
// multiple of 64 and at most 1024, so ONE wave-wide 16-byte load (a lane per chunk) brings a whole node -- header and its
// visit / Q / P table -- into LDS in a single memory round trip, from where every lane (= board square) picks its edge.
// `child` caches the record index of the state the edge leads to (-1 = not expanded yet), so a descent follows indices and
// probes the hash table only where it leaves the known tree (the leaf) -- not at every level.  The record stride trades HBM
// capacity (22.6 GB of 288 for 4096 games x 6164 nodes; only the touched 64-byte sectors ever move) for one dependent
// memory round trip per tree level instead of four (table window, key compare, node header, edge rows).
// Hash table: 32-bit entries [tag 12 | index+1 20], 0 = empty; a 64-wide window is one 256-byte read and only tag matches
// (1 in 4096 false positives) go on to compare the 128-bit key in the record header.
struct OzEdge { uint32_t n_tag; int32_t child; double q; double p; };
#define OZ_REC_HDR 32
#define OZ_EDGE_BYTES 24
#define OZ_HT_IDX_BITS 20
#define OZ_HT_IDX_MASK ((1u << OZ_HT_IDX_BITS) - 1u)
static_assert(sizeof(OzEdge) == OZ_EDGE_BYTES, "edge layout");

// proofs ("proofs" in oz_common.h): what the OZ_VSIGNS_PROVEN instantiations of the tree kernels get beside the records
enum { PS_EDGES = 0, PS_EDGE_STOPS = 1, PS_NODE_STOPS = 2, PS_ROOTS = 3, OZ_NPSTAT = 4 };
struct ProofDev {
    OzProof* entry;            // [G][node_cap] one entry per node record, written whole at expansion
    unsigned long long* stat;  // [G][OZ_NPSTAT] edges proven, descents ended on a proven edge / on a proven node, roots whose value became known
    int E;                     // the object's solve_leaves: a leaf expanded with <= E empties carries the exact sign in v (0: none does)
};
struct MctsDev {
    int G, n, n2, node_cap, row_cap, rec_bytes, ht_cap;
    uint64_t valid;
    double c;
    int qmode;
    unsigned char* recs;       // [G][node_cap][rec_bytes]
    int* node_count;           // [G]
    uint32_t* ht;              // [G][ht_cap]
    int* root_node;            // [G] record index of the current root (-1: not looked up yet / not expanded)
    uint64_t *root_own, *root_opp;
    uint8_t* active;
    int* leaf_status;
    uint64_t *leaf_own, *leaf_opp, *leaf_legal;
    int *depth, *term_value, *leaf_slot, *leaf_fs;
    int2* path;                // [G][OZ_MAX_DEPTH] (node index, edge rank)
    uint64_t *batch_own, *batch_opp;
    int* batch_count;
    float *pi, *v;
    double* last_value;
    int* last_vtype;
    unsigned long long* stat;  // [G][OZ_NSTAT]
    int* error_flag;
    unsigned long long* eval_leaves;    // positions handed to the network so far (after cross-game de-duplication)
    int dedup;                 // k_compact: evaluate a board reached by several games in the same step once
    int batch_cap, batch_rot;  // k_compact (free-running driver): at most batch_cap slots (0: no cap), handed out in game order starting at game batch_rot
    EvalCacheDev ec;           // the network's persistent evaluation cache (buckets == 0: none)
    int* hit_count;            // leaves of this batch served from the cache: they take the pi / v rows G-1, G-2, ... (never the network's rows 0 ..)
    int* hit_entry;            // [G] cache entry of hit h
    unsigned batch_stamp;      // k_cache_insert: number of this batch (two inserts into one entry within a batch: the first wins)
    // Dirichlet root noise ("root noise" below): null / 0 until an object arms it for the first time
    double* noise_eta;         // [G][64] eta by square, 0 off the legal set of the root it was drawn for
    uint8_t* noise_armed;      // [G] the slot's CURRENT root carries noise
    double noise_eps;          // the mixing weight (0: off)
    double forced_k;           // forced playouts ("forced playouts" below): the forcing constant k (0: off); needs noise, so the TV_NOISE kernels alone read it
    ProofDev pf;               // proofs ("proofs" below): null / 0 until oz_*_set_proofs; the OZ_VSIGNS_PROVEN instantiations alone read it
    OzSelection sel;           // selection ("selection" in oz_common.h): flags == 0 until oz_*_set_selection; the TV_SEL kernels alone read it
};
// the frontier entries (node, edge rank): the rank is below 64; in the sound instantiations (VS, "value signs" in oz_common.h) bit 30 of .y keeps
// sigma of the level -- the descent swapped sides after the edge.  The reference instantiations never set the bit and read .y as it is.
#define OZ_PATH_SWAP (1 << 30)
template <int VS> __device__ __forceinline__ int path_rank(int y) { return VS != OZ_VSIGNS_REFERENCE ? y & (OZ_PATH_SWAP - 1) : y; }

// Gumbel search ("Gumbel search" below): what the tree kernels get beside MctsDev; the TV_GUMBEL ones alone read it.  An object without the option never fills it.
struct GumbelDev {
    double* g;                 // [G][64] the Gumbel draw by square, 0 off the legal set of the root it was drawn for
    int* n0;                   // [G][64] the root's stored N when the slot was armed (0: the root was not in the table)
    uint8_t* armed;            // [G] the slot's CURRENT root is a Gumbel root
    const int* table;          // [max_considered][budget] considered_visits(m, budget), m = 1 .. max_considered
    int max_considered, budget;
    double c_visit, c_scale;
};

__device__ __forceinline__ unsigned char* rec_ptr(const MctsDev& t, int g, int node) {
    return t.recs + ((size_t)g * t.node_cap + (size_t)node) * (size_t)t.rec_bytes;
}
__device__ __forceinline__ OzEdge* rec_edge(const MctsDev& t, int g, int node, int rank) {
    return reinterpret_cast<OzEdge*>(rec_ptr(t, g, node) + OZ_REC_HDR) + rank;
}
__device__ __forceinline__ int* rec_Ns(const MctsDev& t, int g, int node) {
    return reinterpret_cast<int*>(rec_ptr(t, g, node) + 16);
}
// a record holds one edge per legal square, in square order: the rank of square sq under `legal`, and this lane's edge of `node` (lane = square)
__device__ __forceinline__ int edge_rank(uint64_t legal, int sq) { return oz_popc(legal & ((1ULL << sq) - 1ULL)); }
__device__ __forceinline__ OzEdge* lane_edge(const MctsDev& t, int g, int node, uint64_t legal, int lane) {
    return rec_edge(t, g, node, edge_rank(legal, lane));
}

// per-wavefront LDS working set of the tree kernels (one wave = one game = one block of 64)
struct TreeLds {
    uint4 rec[64];             // the staged node record: header + visit / Q / P rows (<= 1024 B)
    int2 path[OZ_MAX_DEPTH];   // the frontier of this descent: (node, edge rank) per level
    double arr[64];            // expand: masked policy row for the pairwise sum
};

// ---------------------------------------------------------------- wave helpers (wave = 64 lanes)
__device__ __forceinline__ double wave_max_f64(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        double y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}
// the balanced binary tree sum over the lanes 0 .. 63 (oz_tree_sum64, oz_common.h): round r adds the partner lane ^ (1 << r); addition
// commutes, so every lane ends with the same bits
__device__ __forceinline__ double wave_tree_sum_f64(double x) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ int wave_max_i32(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        int y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}
// Wave-uniform values (the position a wave stands on, node indices, the chosen square) belong in SGPRs: the bitboard
// arithmetic of the rules (legal set, flips: ~300 64-bit shift / and / or per tree level) then runs on the scalar unit --
// one instruction per 64-bit op per WAVE instead of two vector instructions per op per 16 lanes.  Loads through a pointer
// come back in vector registers, so the uniformity has to be stated.
// (the builtin returns a signed int: every half is cast to uint32_t before it is widened)
__device__ __forceinline__ uint32_t uni32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ int unii(int x) { return (int)__builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) {
    const uint32_t lo = uni32((uint32_t)x), hi = uni32((uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | (uint64_t)lo;
}
__device__ __forceinline__ int lane_get(int x, int lane) { return (int)__builtin_amdgcn_readlane(x, lane); }   // lane must be uniform

// one wave = one game: stores of one lane must have completed (and may not be reordered by the compiler) before the
// other lanes load the same locations in the next phase
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t key_hash64(uint64_t own, uint64_t opp) {
    return oz_sm64(own * 0x2545F4914F6CDD1DULL ^ oz_sm64(opp));
}

// 64-wide linear probe.  Returns the node index or -1; *free_slot = first empty slot of the probe
// sequence (where an insert must go).  All lanes get the same results.
__device__ int ht_find(const MctsDev& t, int g, uint64_t own, uint64_t opp, int lane, int* free_slot) {
    const uint32_t* __restrict__ ht = t.ht + (size_t)g * t.ht_cap;
    const int cap = t.ht_cap, mask = cap - 1;
    const uint64_t hh = key_hash64(own, opp);
    int base = (int)((uint32_t)(hh >> 17) & (uint32_t)mask);
    const uint32_t tag = (uint32_t)(hh >> 52);
    for (int probed = 0; probed < cap; probed += 64, base = (base + 64) & mask) {
        const uint32_t e = ht[(base + lane) & mask];
        const bool empty = e == 0;
        const int idx = (int)(e & OZ_HT_IDX_MASK) - 1;
        bool match = false;
        if (!empty && (e >> OZ_HT_IDX_BITS) == tag && idx < t.node_cap) {
            const uint64_t* h = reinterpret_cast<const uint64_t*>(rec_ptr(t, g, idx));
            match = h[0] == own && h[1] == opp;
        }
        const uint64_t mb = __ballot(match), eb = __ballot(empty);
        if (mb) {
            const int ml = oz_ctz(mb);
            if (!eb || ml < oz_ctz(eb)) return lane_get(idx, ml);
        }
        if (eb) {
            *free_slot = (base + oz_ctz(eb)) & mask;
            return -1;
        }
    }
    *free_slot = -1;
    return -1;
}
__device__ __forceinline__ uint32_t ht_entry(uint64_t own, uint64_t opp, int node) {
    return ((uint32_t)(key_hash64(own, opp) >> 52) << OZ_HT_IDX_BITS) | (uint32_t)(node + 1);
}

// ---------------------------------------------------------------- root noise: Dirichlet noise on the root prior (opt-in, AlphaZero's exploration)
// (the semantics are stated in include/othellozero_amd.h, "root noise"; the restatement the tests hold this against is tests/root_noise_ref.py.)
//   * STORED PRIORS ARE NEVER MODIFIED: the node tables are transposition tables that outlive a move, so the noise is a view taken at selection
//     time, at depth 0 of a descent only, of the root it was drawn for (a position cannot recur below itself: every move adds a disc, so
//     "depth 0" and "is the root" coincide).  On an armed slot, for a legal square: Pn = (1.0 - eps) * P + eps * eta[sq] in float64, two products
//     and one sum as written, and U = Q + (c * Pn) * (sqrt(Ns) / (1 + N)) -- under leaf-parallel search with the virtual-loss view of Ns, N, Q.
//     Deeper levels, unarmed slots and eps == 0 read the stored P.  First-maximum tie break and the Ns == 0 quirk are untouched.
//   * the noise belongs to ONE root board of ONE slot: noise_armed[g] says that eta[g] is that of the slot's current root; whatever gives a slot
//     another board clears it (oz_mcts_set_roots, k_sp_roots / k_sp_roots_stagger, the move inside the free-running advance) or draws anew.
//   * a compile-time variant: the bodies below take template <bool NOISE>; an object that never armed noise launches the NOISE = false kernels,
//     which are the code they were before this section existed.  The host picks per launch (oz_mcts::noise_ever).
// The sampler: one lane per square, counter based, no state.  u(sq, i) = oz_rng_unit(oz_rng(seed, game id, ply, OZ_RNG_NOISE + 256 sq + 65536 i)),
// w = 1 - u in (0, 1].  Gamma(alpha) by Marsaglia-Tsang (with the alpha < 1 boost g *= w^(1 / alpha)), at most 16 attempts of three draws each
// (draws 3t, 3t + 1, 3t + 2; the boost takes draw 48) -- all float64; eta = g / S, S = NumPy's pairwise sum of g over the (n, n) array with zeros
// off the legal set; S == 0 or not finite: uniform over the legal squares.  A root with one legal move gets g / g = 1.0 exactly.
__device__ __forceinline__ double noise_unit(uint64_t seed, uint64_t gid, uint64_t ply, int sq, int i) {
    return oz_rng_unit(oz_rng(seed, gid, ply, (uint64_t)OZ_RNG_NOISE + 256ull * (uint64_t)sq + 65536ull * (uint64_t)i));
}
__device__ __forceinline__ double noise_gamma(double alpha, uint64_t seed, uint64_t gid, uint64_t ply, int sq) {
    const double a = alpha < 1.0 ? alpha + 1.0 : alpha;
    const double d = a - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * d);
    double g = d;                                                               // (16 rejections in a row: never seen; the mean of the law)
    for (int t = 0; t < 16; ++t) {
        const double w0 = 1.0 - noise_unit(seed, gid, ply, sq, 3 * t), u1 = noise_unit(seed, gid, ply, sq, 3 * t + 1);
        const double x = sqrt(-2.0 * log(w0)) * cos(2.0 * 3.14159265358979323846 * u1);          // Box-Muller
        double v = 1.0 + cc * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double w2 = 1.0 - noise_unit(seed, gid, ply, sq, 3 * t + 2);
        if (log(w2) < 0.5 * x * x + d - d * v + d * log(v)) { g = d * v; break; }
    }
    if (alpha < 1.0) g *= pow(1.0 - noise_unit(seed, gid, ply, sq, 48), 1.0 / alpha);
    return g;
}
// one wave = one game: draws eta for the root (own, opp) of slot g and arms the slot.  arr = 64 doubles of LDS (free on entry, free on return).
__device__ __forceinline__ void root_noise_body(const MctsDev& t, double* arr, int g, int lane, uint64_t own, uint64_t opp, double alpha,
                                                uint64_t seed, uint64_t gid, int ply) {
    const uint64_t legal = oz_legal(own, opp, t.valid);
    const int r = lane >> 3, c = lane & 7, n = t.n;
    const bool inb = r < n && c < n, is_legal = (legal >> lane) & 1;
    const double gm = is_legal ? noise_gamma(alpha, seed, gid, (uint64_t)ply, lane) : 0.0;
    __syncthreads();
    if (inb) arr[r * n + c] = gm;
    __syncthreads();
    const double S = pairwise_sum(arr, t.n2);
    double eta = 0.0;
    if (is_legal) eta = (S > 0.0 && S < INFINITY) ? gm / S : 1.0 / (double)oz_popc(legal);
    t.noise_eta[(size_t)g * 64 + lane] = eta;
    if (lane == 0) t.noise_armed[g] = legal != 0 ? 1 : 0;
    __syncthreads();
}
// the noise of the CURRENT roots of the active slots, keyed (seed, game_ids[g], plies[g]); an idle slot is disarmed
__global__ __launch_bounds__(64) void k_root_noise(MctsDev t, double alpha, uint64_t seed, const uint64_t* __restrict__ game_ids,
                                                   const int* __restrict__ plies) {
    __shared__ double arr[64];
    const int g = blockIdx.x, lane = threadIdx.x;
    if (!t.active[g]) {
        if (lane == 0) t.noise_armed[g] = 0;
        return;
    }
    root_noise_body(t, arr, g, lane, uni64(t.root_own[g]), uni64(t.root_opp[g]), alpha, seed, uni64(game_ids[g]), unii(plies[g]));
}
// armed = active (oz_mcts_set_root_noise with a null `armed`)
__global__ void k_noise_arm_active(MctsDev t) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < t.G) t.noise_armed[g] = t.active[g] ? 1 : 0;
}
// what a descent of slot g mixes into its root's priors: true and *eta = this lane's share if the slot is armed
template <bool NOISE> __device__ __forceinline__ bool noise_of_slot(const MctsDev& t, int g, int lane, double* eta) {
    if constexpr (NOISE) {
        if (t.noise_eps > 0.0 && unii((int)t.noise_armed[g]) != 0) {
            *eta = t.noise_eta[(size_t)g * 64 + lane];                          // one coalesced 512-byte load per descent
            return true;
        }
    }
    return false;
}

// ---------------------------------------------------------------- move sampling: a ~ N(root, a)^(1/T) for the opening plies (opt-in, AlphaZero's move rule)
// (the definition is stated in include/othellozero_amd.h, "move sampling"; the restatement the tests hold this against is tests/move_sampling_ref.py.)
// One wave = one game, lane = square.  cnt = the root's visit count of this lane's square, mx = their maximum (>= 1), legal uniform, u = the unit
// draw of stream (seed, game id, ply, OZ_RNG_SAMPLE).  All float64, no contraction:
//     w[sq] = N[sq] == 0 ? 0.0 : pow((double)N[sq] / (double)mx, 1.0 / T)     legal squares only; in (0, 1] for every T, exactly 1.0 at the maximum
//     cum[sq] = the running sum of w over the legal squares in ascending sq, ONE ADDITION AFTER THE OTHER (c = c + w[sq]): the order is part of the
//     definition, so this is a 64-step lane loop and not a tree scan (nothing next to the `sims` simulations of a move)
//     r = u * c_total;  action = the first legal square with cum[sq] > r, else (u * c rounded up to c) the last legal square with w > 0
// A square with N == 0 adds 0.0 and its cum equals its predecessor's: never chosen.  -1: no visited legal square (the callers exclude it).
struct MoveSampling { double temperature; int plies; };    // plies == 0: off
// ---------------------------------------------------------------- playout cap: most self-play moves on a small budget, a random share on the full one (opt-in, KataGo's)
// (the definition is stated in include/othellozero_amd.h, "playout cap"; the restatement the tests hold this against is tests/playout_cap_ref.py.)
// The budget of the searched move of (game id, ply) is oz_playout_budget (oz_common.h): a function of the key alone, so every kernel that needs
// it -- the budget, the noise decision, the flag of the move -- evaluates it again (two integer mixes and one compare per wave) instead of
// carrying a per-slot state.  A fast move draws no root noise, and its record carries flag 1 in the first spare byte.
struct PlayoutCap {
    int fast_sims;                  // 0: off
    double full_prob;
    uint8_t* log_fast;              // [G][64] the flag of every ply of the game in progress, next to GamesDev.log_greedy
    unsigned long long* moves;      // [0] full moves [1] fast moves played under the cap
};
__device__ __forceinline__ double lane_get_f64(double x, int lane) {      // lane must be uniform
    const long long b = __double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | (uint64_t)lo));
}
__device__ __forceinline__ int sample_move(int cnt, uint64_t legal, int mx, double temperature, double u, int lane) {
    const bool is_legal = (legal >> lane) & 1;
    const double inv = 1.0 / temperature;
    const double w = (is_legal && cnt != 0) ? pow((double)cnt / (double)mx, inv) : 0.0;
    double c = 0.0, cum = 0.0;
    for (int sq = 0; sq < 64; ++sq) {
        if (!((legal >> sq) & 1)) continue;
        c = c + lane_get_f64(w, sq);
        if (lane == sq) cum = c;
    }
    const double r = u * c;
    const uint64_t over = __ballot(is_legal && cum > r);
    if (over) return oz_ctz(over);
    const uint64_t visited = __ballot(is_legal && w > 0.0);
    return visited ? 63 - __builtin_clzll(visited) : -1;
}

// ---------------------------------------------------------------- forced playouts and policy target pruning (opt-in, KataGo's; needs root noise)
// (the definition is stated in include/othellozero_amd.h, "forced playouts"; the restatement the tests hold this against is tests/forced_playouts_ref.py.)
//   * forcing lives in descend_one<true>, at depth 0 of a descent from an armed root: a child tried at least once whose count (in-flight descents
//     included) is below sqrt((k * Pn) * Ns) gets U = +inf.  MctsDev.forced_k is uniform, and so are `noisy` and `depth`: the wave takes one
//     branch, only the compare is per lane.  k == 0 leaves the expression the noise kernels evaluated before.
//   * pruning lives in the move (sp_move_body<.., FORCE>) and in k_root_read<RO_PRUNED>: one lane per square computes oz_forced_prune (oz_common.h) of
//     its own (N, Q, P, eta) and of star's, fetched with lane_get.  Only the row that becomes the policy target is pruned; last_counts, the
//     arg-max, the tie rule, sample_move and the e-greedy branch read the raw counts.
struct ForcedPlayouts {
    double k;                       // 0: off
    unsigned long long* stat;       // [0] moves whose recorded row differs from the raw one [1] visits of the rows pruning ran on [2] visits kept of them
};
__device__ __forceinline__ int wave_sum_i32(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
// the pruned count of this lane's square at the root record `node` of slot g (its noise armed, eta[g] that of this root); cnt = the lane's raw
// count (0 off the legal set), mx = the largest
__device__ __forceinline__ int forced_prune_lane(const MctsDev& t, int g, int node, int lane, uint64_t legal, int cnt, int mx, double k) {
    const bool is_legal = (legal >> lane) & 1;
    double Q = 0.0, P = 0.0;
    if (is_legal) {
        const OzEdge* e = lane_edge(t, g, node, legal, lane);
        Q = e->q; P = e->p;
    }
    const double eta = t.noise_eta[(size_t)g * 64 + lane];
    const int Ns = unii(*rec_Ns(t, g, node));
    const uint64_t top = __ballot(is_legal && cnt == mx);
    if (top == 0) return cnt;                                               // no legal move: nothing to prune
    const int star = oz_ctz(top);
    const int Nstar = lane_get(cnt, star);
    const double Qstar = lane_get_f64(Q, star), Pstar = lane_get_f64(P, star), etastar = lane_get_f64(eta, star);
    return is_legal ? oz_forced_prune(cnt, Q, P, eta, Nstar, Qstar, Pstar, etastar, lane == star ? 1 : 0, Ns, t.c, t.noise_eps, k) : 0;
}

// ---------------------------------------------------------------- K4: select / descend
// MCTS.simulate down to the first terminal or unexpanded state (MCTS/__init__.py:39-44,58-67),
// get_next_state (othelo_mcts.py:43-49).  One wave per game; per level ONE wave-wide load stages the node's record in LDS.
// One descent from a root down to the first terminal or unknown state; shared by the one-descent-per-step search (select_body) and the
// leaf-parallel one (wide_select_body).  `rec` / `path` = the LDS record stage and this descent's frontier (OZ_MAX_DEPTH entries);
// `rootn` = the caller's cached record index of the root, kept up to date; noisy / eta = the slot's root-noise view (noise_of_slot).
// The statistics are seen through the step's descents already in flight ("leaf-parallel search" below): descents 0 .. fl.n-1 with their
// frontiers and depths.  With none in flight (select_body passes a literal 0: the loop compiles away) the view is the identity.
struct InFlight { const int2 (*path)[OZ_MAX_DEPTH]; const int* depth; int n; };
struct Descent {
    uint64_t own, opp, legal;  // where it ended, and the mover's legal set there
    int depth, status, tval;
    int fs;                    // free table slot of the probe that left the known tree (-1: none)
    int err;                   // EF_* bit of an error exit (status is then OZ_LEAF_IDLE), 0: none
};
// GUMBEL (the TV_GUMBEL kernels): gr = the slot's Gumbel view (gumbel_of_slot); on an armed root, depth 0 picks by the Gumbel rule instead of PUCT.
struct GumbelRoot { bool armed; double g; int n0; const GumbelDev* gd; };
// VS: the value signs the tree holds (oz_common.h), a template argument of every tree kernel: the default's code is the reference rule alone
// SEL (the TV_SEL kernels): U by the selection rule of oz_common.h ("selection"); t.sel is uniform: one branch per part and wave
template <bool NOISE, bool GUMBEL = false, int VS = OZ_VSIGNS_REFERENCE, bool SEL = false>
__device__ __forceinline__ Descent descend_one(const MctsDev& t, uint4* rec, int2* path, int g, int lane, uint64_t own, uint64_t opp, uint64_t legal,
                                               int& rootn, bool noisy, double eta, const InFlight fl, const GumbelRoot gr = GumbelRoot{false, 0.0, 0, nullptr}) {
    int depth = 0, status, tval = 0, err = 0, fs = -1;
    int node = rootn;                                           // record index of the state we stand on, -1 = unknown
    int pnode = -1, prank = 0;                                  // the edge we arrived through (to cache the child index)
    for (;;) {
        // `legal` = the mover's legal set of the state we stand on (of the root above; below, the move that led here computed it)
        if (legal == 0 && oz_legal(opp, own, t.valid) == 0) {       // is_terminal_state, othelo_mcts.py:28-29
            // get_state_reward: winner of the ch0 view, draw -> ch0 (simulate returns -reward: the backup's reference rule); sound: the sign, a draw is 0
            tval = oz_terminal_value(oz_vsigns_rule(VS), own, opp);
            status = OZ_LEAF_TERMINAL;
            break;
        }
        if (node < 0) {                                             // leaving the known tree: is the state in the table (transposition)?
            node = ht_find(t, g, own, opp, lane, &fs);
            if (node < 0) { status = OZ_LEAF_EVAL; break; }
            if (pnode < 0) rootn = node;
            if (lane == 0) {
                if (pnode >= 0) rec_edge(t, g, pnode, prank)->child = node;
                else t.root_node[g] = node;
            }
        }
        if (legal == 0) { err = EF_NOMOVE; status = OZ_LEAF_IDLE; break; }   // reference: max() of empty list
        if (depth >= OZ_MAX_DEPTH) { err = EF_DEPTH; status = OZ_LEAF_IDLE; break; }
        if (node >= t.node_cap) { err = EF_CORRUPT; status = OZ_LEAF_IDLE; break; }   // never dereference an index outside the pool
        // stage the record: header + cnt edges, 16 bytes per lane
        const int cnt = oz_popc(legal);
        const int chunks = (OZ_REC_HDR + cnt * OZ_EDGE_BYTES + 15) >> 4;
        // proofs: the node's entry, its address a function of the node index like the record's -- both loads are in flight together
        uint64_t plo = 0, phi = 0, pcand = legal;
        int pown = OZ_PROOF_NONE;
        if constexpr (VS == OZ_VSIGNS_PROVEN) {
            const OzProof* pp = t.pf.entry + (size_t)g * t.node_cap + node;
            plo = pp->lo; phi = pp->hi; pown = pp->own;
        }
        __syncthreads();                                            // the previous level's LDS reads are done
        if (lane < chunks) rec[lane] = reinterpret_cast<const uint4*>(rec_ptr(t, g, node))[lane];
        __syncthreads();
        if constexpr (VS == OZ_VSIGNS_PROVEN) {
            plo = uni64(plo); phi = uni64(phi); pown = unii(pown);
            const int val = oz_proof_value(legal, plo, phi, pown);
            if (depth > 0 && val != OZ_PROOF_NONE) {                // a proven position is not searched again (the root always is: a move needs visits)
                tval = val;
                status = OZ_LEAF_TERMINAL;
                if (lane == 0) t.pf.stat[(size_t)g * OZ_NPSTAT + PS_NODE_STOPS] += 1;
                break;
            }
            int bad;
            pcand = oz_proof_candidates(legal, plo, phi, val, &bad);
            if (bad && lane == 0) atomicOr(t.error_flag, EF_CORRUPT);
        }
        const uint64_t* w = reinterpret_cast<const uint64_t*>(rec);
        const int Ns = unii((int)(uint32_t)w[2]);
        const bool is_legal = (legal >> lane) & 1;
        const int rank = edge_rank(legal, lane);
        // the in-flight descents of this step that stand on this node at this level, and those that took this lane's edge from it
        int ks = 0, ke = 0;
        for (int i = 0; i < fl.n; ++i)
            if (fl.depth[i] > depth) {
                const int2 pe = fl.path[i][depth];
                if (pe.x == node) { ++ks; ke += path_rank<VS>(pe.y) == rank ? 1 : 0; }
            }
        double U = -INFINITY;
        int child = -1;
        if (is_legal) {
            const uint64_t w0 = w[4 + 3 * rank];
            int N = (int)((uint32_t)w0 & ~OZ_TAG_F32);
            child = (int)(w0 >> 32);
            double Q = __longlong_as_double((long long)w[5 + 3 * rank]);
            const double P = __longlong_as_double((long long)w[6 + 3 * rank]);
            if (ke) {                                                       // ke == 0 reads the stored bits: (N * Q) / N is not Q
                Q = ((double)N * Q - (double)ke) / (double)(N + ke);
                N += ke;
            }
            if constexpr (VS == OZ_VSIGNS_PROVEN) {                         // a proven edge is worth its proof, whatever was averaged into Q
                const int e = oz_proof_edge(plo, phi, lane);
                if (e != OZ_PROOF_NONE) Q = (double)e;
            }
            const double bound = sqrt((double)(Ns + ks)) / (double)(1 + N);    // MCTS/__init__.py:169
            U = Q + (t.c * P) * bound;                                     // :170, left to right
            if constexpr (NOISE) {
                if (noisy && depth == 0) {                                  // (uniform: one branch per wave, only the forcing compare is per lane)
                    const double Pn = (1.0 - t.noise_eps) * P + t.noise_eps * eta;          // the root's noisy view of P
                    U = Q + (t.c * Pn) * bound;
                    // forced playouts: a tried child of the noisy root below its quota is selected before any PUCT value (the first such square)
                    if (t.forced_k > 0.0 && N > 0 && (double)N < sqrt((t.forced_k * Pn) * (double)(Ns + ks))) U = INFINITY;
                }
            }
        }
        if constexpr (SEL) {
            int N = 0;
            double Q = 0.0, P = 0.0;
            if (is_legal) {
                N = (int)((uint32_t)w[4 + 3 * rank] & ~OZ_TAG_F32);
                Q = __longlong_as_double((long long)w[5 + 3 * rank]);
                P = __longlong_as_double((long long)w[6 + 3 * rank]);
                if (ke) {
                    Q = ((double)N * Q - (double)ke) / (double)(N + ke);
                    N += ke;
                }
                if constexpr (NOISE) {
                    if (noisy && depth == 0) P = (1.0 - t.noise_eps) * P + t.noise_eps * eta;
                }
            }
            const int nv = Ns + ks;
            const double cS = (t.sel.flags & OZ_SEL_GROWTH) ? oz_select_c(t.c, t.sel.base, t.sel.factor, nv) : t.c;
            const double r = oz_select_r(t.sel.flags & OZ_SEL_PRIOR_FIRST, nv);
            if (t.sel.flags & OZ_SEL_FPU) {
                const bool vis = is_legal && N > 0;
                const int SN = wave_sum_i32(is_legal ? N : 0);
                const double SQ = wave_tree_sum_f64(vis ? oz_select_fpu_q(N, Q) : 0.0);
                const double SP = wave_tree_sum_f64(vis ? P : 0.0);
                double V;
                const double F = oz_select_fpu(__longlong_as_double((long long)w[3]), SQ, SP, SN, depth == 0 ? t.sel.fpu_root : t.sel.fpu, &V);
                if (!vis) Q = F;
            }
            if (is_legal) {
                if constexpr (VS == OZ_VSIGNS_PROVEN) {
                    const int e = oz_proof_edge(plo, phi, lane);
                    if (e != OZ_PROOF_NONE) Q = (double)e;
                }
                U = oz_select_u(Q, cS, P, r, N);
            }
        }
        bool cand = is_legal;
        if constexpr (VS == OZ_VSIGNS_PROVEN) {
            cand = (pcand >> lane) & 1;
            if (!cand) U = -INFINITY;
        }
        if constexpr (GUMBEL) {
            if (gr.armed && depth == 0) {                                   // (uniform: one branch per wave)
                const GumbelDev& gd = *gr.gd;
                int N = 0;
                double Q = 0.0, P = 0.0;
                if (is_legal) {
                    N = (int)((uint32_t)w[4 + 3 * rank] & ~OZ_TAG_F32);
                    Q = __longlong_as_double((long long)w[5 + 3 * rank]);
                    P = __longlong_as_double((long long)w[6 + 3 * rank]);
                }
                const int nv = is_legal ? N - gr.n0 : 0;                    // this search's visits of the lane's move
                const int tv = wave_sum_i32(nv), maxn = wave_max_i32(nv);
                OzGumbelSums sm{0, 0, 0.0, 0.0};                            // the float sums are sequential in square order: every lane walks the staged edges
                for (int r = 0; r < cnt; ++r)
                    oz_gumbel_acc(sm, (int)((uint32_t)w[4 + 3 * r] & ~OZ_TAG_F32), __longlong_as_double((long long)w[5 + 3 * r]),
                                  __longlong_as_double((long long)w[6 + 3 * r]));
                const double vmix = oz_gumbel_vmix(sm, __longlong_as_double((long long)w[3]));
                const int m_eff = gd.max_considered < cnt ? gd.max_considered : cnt;
                const int cv = tv >= 0 && tv < gd.budget ? gd.table[(size_t)(m_eff - 1) * gd.budget + tv] : maxn;
                const bool match = is_legal && nv == cv;
                cand = __ballot(match) ? match : is_legal;
                U = cand ? oz_gumbel_score(gr.g, P, oz_gumbel_sigma(N, Q, vmix, sm.maxN, gd.c_visit, gd.c_scale)) : -INFINITY;
            }
        }
        const double m = wave_max_f64(U);
        const int best = oz_ctz(__ballot(cand && U == m));                 // first maximum
        const int brank = edge_rank(legal, best);
        if constexpr (VS == OZ_VSIGNS_REFERENCE) { if (lane == 0) path[depth] = make_int2(node, brank); }
        ++depth;
        pnode = node; prank = brank;
        node = lane_get(child, best);
        oz_apply(own, opp, best);
        // swap only if the opponent can move (othelo_mcts.py:43-49); its legal set IS the next state's -- one flood per level, not two
        const uint64_t theirs = oz_legal(opp, own, t.valid);
        if constexpr (VS != OZ_VSIGNS_REFERENCE) { if (lane == 0) path[depth - 1] = make_int2(pnode, brank | (theirs != 0 ? OZ_PATH_SWAP : 0)); }   // sigma rides along
        if (theirs != 0) { uint64_t s = own; own = opp; opp = s; legal = theirs; }
        else legal = oz_legal(own, opp, t.valid);                   // pass (or the game is over): the same side is to move again
        if constexpr (VS == OZ_VSIGNS_PROVEN) {
            const int e = oz_proof_edge(plo, phi, best);
            if (e != OZ_PROOF_NONE) {                               // the edge is proven: its value for the side to move after it, no look at the child
                tval = theirs != 0 ? -e : e;
                status = OZ_LEAF_TERMINAL;
                if (lane == 0) t.pf.stat[(size_t)g * OZ_NPSTAT + PS_EDGE_STOPS] += 1;
                break;
            }
        }
    }
    return Descent{own, opp, legal, depth, status, tval, fs, err};
}
// (body shared by k_select and the free-running k_advance; returns the status it stored in leaf_status[g].  A descent that ends in an error
// is stored like any other, with status OZ_LEAF_IDLE.)
// the slot's Gumbel view: armed, and then this lane's draw and snapshot (one coalesced 512-byte and one 256-byte load per descent)
__device__ __forceinline__ GumbelRoot gumbel_of_slot(const GumbelDev& gd, int g, int lane) {
    GumbelRoot gr{false, 0.0, 0, &gd};
    if (unii((int)gd.armed[g]) != 0) {
        gr.armed = true;
        gr.g = gd.g[(size_t)g * 64 + lane];
        gr.n0 = gd.n0[(size_t)g * 64 + lane];
    }
    return gr;
}
template <bool NOISE = false, bool GUMBEL = false, int VS = OZ_VSIGNS_REFERENCE, bool SEL = false>
__device__ __forceinline__ int select_body(const MctsDev& t, TreeLds& L, int g, int lane, const GumbelDev* gd = nullptr) {
    if (!t.active[g]) {
        if (lane == 0) t.leaf_status[g] = OZ_LEAF_IDLE;
        return OZ_LEAF_IDLE;
    }
    double eta = 0.0;
    const bool noisy = noise_of_slot<NOISE>(t, g, lane, &eta);
    const uint64_t own = uni64(t.root_own[g]), opp = uni64(t.root_opp[g]);
    int rootn = unii(t.root_node[g]);
    GumbelRoot gr{false, 0.0, 0, nullptr};
    if constexpr (GUMBEL) gr = gumbel_of_slot(*gd, g, lane);
    const Descent e = descend_one<NOISE, GUMBEL, VS, SEL>(t, L.rec, L.path, g, lane, own, opp, oz_legal(own, opp, t.valid), rootn, noisy, eta, InFlight{nullptr, nullptr, 0}, gr);
    __syncthreads();
    if (lane < e.depth) t.path[(size_t)g * OZ_MAX_DEPTH + lane] = L.path[lane];          // the frontier, one coalesced store
    if (lane == 0) {
        t.leaf_status[g] = e.status;
        t.leaf_own[g] = e.own; t.leaf_opp[g] = e.opp; t.leaf_legal[g] = e.legal; t.leaf_fs[g] = e.fs;
        t.depth[g] = e.depth; t.term_value[g] = e.tval;
        unsigned long long* st = t.stat + (size_t)g * OZ_NSTAT;
        st[ST_SIMS] += 1; st[ST_VISITS] += (unsigned long long)(e.depth + 1);
        if (e.status == OZ_LEAF_TERMINAL) st[ST_TERMINAL] += 1;
        if (e.err) atomicOr(t.error_flag, e.err);
    }
    return e.status;
}

// ---------------------------------------------------------------- K13: leaf compaction
// ballot + prefix sum over the games; slot order = game order (deterministic).
// Leaves are also de-duplicated ACROSS games (G <= OZ_DEDUP_MAX_G): a board that several games reach in the same step
// is evaluated once and every one of those games reads the same (pi, v) row.  The network's output for a position does
// not depend on its slot or on the batch (oz_net.hip), so results are bit-identical with or without this; it removes the
// evaluations of the opening plies, where thousands of concurrent games still walk the same few positions.
// The table (LDS, open addressing) holds the LOWEST game index with a given board: slots are the first occurrences in game order.
// ---- the network's persistent evaluation cache (EvalCacheDev, oz_internal.h)
__device__ __forceinline__ unsigned ec_bucket(const EvalCacheDev& c, uint64_t own, uint64_t opp, unsigned* way_pick) {
    const uint64_t h = key_hash64(own ^ 0x6A09E667F3BCC909ULL, opp);
    *way_pick = (unsigned)(h >> 40) & (OZ_EC_WAYS - 1);
    return (unsigned)(h >> 8) & (c.buckets - 1);
}
// entry index of (own, opp), or -1 (one 64-byte line read)
__device__ __forceinline__ int ec_find(const EvalCacheDev& c, uint64_t own, uint64_t opp) {
    unsigned pick;
    const unsigned b = ec_bucket(c, own, opp, &pick);
    const ulonglong2* k = reinterpret_cast<const ulonglong2*>(c.keys) + (size_t)b * OZ_EC_WAYS;
#pragma unroll
    for (int w = 0; w < OZ_EC_WAYS; ++w) {
        const ulonglong2 e = k[w];
        if (e.x == own && e.y == opp) return (int)(b * OZ_EC_WAYS + w);
    }
    return -1;
}
// the (pi, v) rows of this batch's cache hits: hit h -> row G-1-h of the engine's pi / v arrays.  One thread per (hit, policy entry).
__global__ __launch_bounds__(256) void k_cache_copy(MctsDev t) {
    const int idx = blockIdx.x * 256 + threadIdx.x, h = idx >> 6, a = idx & 63;
    if (h >= *t.hit_count) return;
    const int e = t.hit_entry[h], row = t.G - 1 - h;
    if (a < t.n2) t.pi[(size_t)row * t.n2 + a] = t.ec.pi[(size_t)e * t.n2 + a];
    if (a == 0) t.v[row] = t.ec.v[e];
}
// after the network: every evaluated position (rows 0 .. batch_count-1) goes into the cache.  One wave per position.
__global__ __launch_bounds__(256) void k_cache_insert(MctsDev t) {
    const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= *t.batch_count) return;
    const uint64_t own = t.batch_own[slot], opp = t.batch_opp[slot];
    unsigned pick;
    const unsigned b = ec_bucket(t.ec, own, opp, &pick);
    const ulonglong2* k = reinterpret_cast<const ulonglong2*>(t.ec.keys) + (size_t)b * OZ_EC_WAYS;
    ulonglong2 e = make_ulonglong2(1, 1);
    if (lane < OZ_EC_WAYS) e = k[lane];
    const uint64_t present = __ballot(lane < OZ_EC_WAYS && e.x == own && e.y == opp);
    if (present) return;                                             // (two games evaluated the same board in one batch and the other one won)
    const uint64_t empty = __ballot(lane < OZ_EC_WAYS && e.x == 0 && e.y == 0);
    // candidate ways: the empty ones in order, else the way the hash picks; an entry takes ONE insert per batch (another position of this
    // batch may be claiming the same way right now: the stamp arbitrates, the loser tries the next candidate or stays uncached)
    uint64_t cand = empty ? empty : (1ULL << pick);
    size_t entry = 0;
    int mine = 0;
    while (cand && !mine) {
        entry = (size_t)b * OZ_EC_WAYS + (unsigned)oz_ctz(cand);
        cand &= cand - 1;
        if (lane == 0) mine = atomicExch(&t.ec.stamp[entry], t.batch_stamp) != t.batch_stamp;
        mine = __shfl(mine, 0, 64);
    }
    if (!mine) return;
    // the key goes LAST, behind a fence: a lookup of another stream that sees the key sees the whole (pi, v) of THIS insert.  (That covers an
    // entry being filled; an entry being REPLACED while another engine's k_cache_copy reads it is not covered -- engines that share a cached
    // network must not run concurrently, see oz_net_set_eval_cache in the header.)
    if (lane == 0) { t.ec.keys[entry * 2] = 0; t.ec.keys[entry * 2 + 1] = 0; }
    __threadfence();
    if (lane < t.n2) t.ec.pi[entry * t.n2 + lane] = t.pi[(size_t)slot * t.n2 + lane];
    if (lane == 0) t.ec.v[entry] = t.v[slot];
    __threadfence();
    if (lane == 0) {
        t.ec.keys[entry * 2] = own; t.ec.keys[entry * 2 + 1] = opp;
        atomicAdd(&t.ec.counters[2], 1ULL);
    }
}

#define OZ_DEDUP_MAX_G 8192
#define OZ_DEDUP_SLOTS 16384
__device__ __forceinline__ unsigned dedup_hash(uint64_t own, uint64_t opp) {
    return (unsigned)(((own * 0x9E3779B97F4A7C15ull) ^ (opp * 0xC2B2AE3D27D4EB4Full)) >> 40) & (OZ_DEDUP_SLOTS - 1);
}
__global__ __launch_bounds__(1024) void k_compact(MctsDev t) {
    __shared__ int wtot[16], whit[16];
    __shared__ int base_s, hit_s;
    __shared__ int tab[OZ_DEDUP_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool dedup = t.dedup && t.G <= OZ_DEDUP_MAX_G;
    const bool cached = t.ec.buckets != 0;
    if (tid == 0) { base_s = 0; hit_s = 0; }
    if (dedup) {
        for (int i = tid; i < OZ_DEDUP_SLOTS; i += 1024) tab[i] = -1;
        __syncthreads();
        for (int g = tid; g < t.G; g += 1024) {
            if (t.leaf_status[g] != OZ_LEAF_EVAL) continue;
            const uint64_t own = t.leaf_own[g], opp = t.leaf_opp[g];
            unsigned h = dedup_hash(own, opp);
            for (;;) {
                int cur = atomicCAS(&tab[h], -1, g);
                if (cur == -1) break;                                      // claimed an empty slot
                if (t.leaf_own[cur] == own && t.leaf_opp[cur] == opp) {    // same board: keep the lowest game index
                    atomicMin(&tab[h], g);
                    break;
                }
                h = (h + 1) & (OZ_DEDUP_SLOTS - 1);
            }
        }
    }
    __syncthreads();
    const int cap = t.batch_cap > 0 ? t.batch_cap : t.G;
    for (int start = 0; start < t.G; start += 1024) {
        // game order, starting at game batch_rot (the start rotates from batch to batch when a cap defers leaves: every game gets served)
        const int seq = start + tid;
        int g = seq + t.batch_rot;
        if (g >= t.G) g -= t.G;
        const bool leaf = seq < t.G && t.leaf_status[g] == OZ_LEAF_EVAL;
        int first = g;
        if (leaf && dedup) {
            const uint64_t own = t.leaf_own[g], opp = t.leaf_opp[g];
            unsigned h = dedup_hash(own, opp);
            for (;;) {
                first = tab[h];
                if (t.leaf_own[first] == own && t.leaf_opp[first] == opp) break;
                h = (h + 1) & (OZ_DEDUP_SLOTS - 1);
            }
        }
        // first occurrence: gets a row -- a network slot, or (the board is in the network's evaluation cache) one of the hit rows G-1, G-2, ...
        int entry = -1;
        if (cached && leaf && first == g) entry = ec_find(t.ec, t.leaf_own[g], t.leaf_opp[g]);
        const bool hit = entry >= 0;
        const bool flag = leaf && first == g && !hit;
        const uint64_t b = __ballot(flag), bh = __ballot(hit);
        const int pre = oz_popc(b & ((1ULL << lane) - 1ULL)), preh = oz_popc(bh & ((1ULL << lane) - 1ULL));
        if (lane == 0) { wtot[w] = oz_popc(b); whit[w] = oz_popc(bh); }
        __syncthreads();
        int woff = 0, total = 0, hoff = 0, htotal = 0;
        for (int i = 0; i < 16; ++i) { int x = wtot[i], y = whit[i]; if (i < w) { woff += x; hoff += y; } total += x; htotal += y; }
        const int base = base_s, hbase = hit_s;
        if (hit) {
            const int h = hbase + hoff + preh;
            t.leaf_slot[g] = t.G - 1 - h;
            t.hit_entry[h] = entry;
        }
        if (flag) {
            const int slot = base + woff + pre;
            if (slot < cap) {
                t.leaf_slot[g] = slot;
                t.batch_own[slot] = t.leaf_own[g];
                t.batch_opp[slot] = t.leaf_opp[g];
            } else {
                t.leaf_slot[g] = 0;
                t.leaf_status[g] = OZ_LEAF_WAIT;                            // no slot in this batch: the leaf is offered again in the next one
            }
        } else if (leaf && !hit) {
            t.leaf_slot[g] = -1 - first;                                   // resolved below (the first occurrence may sit in a later chunk)
        }
        __syncthreads();
        if (tid == 0) { base_s = base + total; hit_s = hbase + htotal; }
        __syncthreads();
    }
    if (dedup) {
        __threadfence_block();
        __syncthreads();
        for (int g = tid; g < t.G; g += 1024)
            if (t.leaf_status[g] == OZ_LEAF_EVAL && t.leaf_slot[g] < 0) {
                const int first = -1 - t.leaf_slot[g];
                if (t.leaf_status[first] == OZ_LEAF_WAIT) { t.leaf_slot[g] = 0; t.leaf_status[g] = OZ_LEAF_WAIT; }     // shares the deferred board: waits with it
                else t.leaf_slot[g] = t.leaf_slot[first];
            }
    }
    if (tid == 0) {
        const int used = base_s < cap ? base_s : cap;
        *t.batch_count = used; *t.eval_leaves += (unsigned long long)used;
        *t.hit_count = hit_s;
        if (cached) { atomicAdd(&t.ec.counters[0], (unsigned long long)(base_s + hit_s)); atomicAdd(&t.ec.counters[1], (unsigned long long)hit_s); }
    }
}

// ---------------------------------------------------------------- solved leaves (opt-in: oz_mcts_set_solve_leaves; the reference's search has none)
// After the evaluator (and after k_cache_insert: the network's cache keeps the NETWORK's v, other engines share it), before expand + backup: a
// row of this step whose board has at most E empties gets v = (float)sign(S), S its exact value for the side to move (oz_solve.h under the root
// window (-1, +1)); pi stays the network's.  A draw is 0.0f.  One wave per row that some game reads this step: blocks [0, cap) are the network's
// rows (the board is the batch's), blocks cap + g (launched where the search looks leaves up in the evaluation cache) the games, for the
// rows G-1-h of the cache hits.  A hit row's board is the leaf of a game that reads it -- not the key of cache entry hit_entry[h], which
// k_cache_insert may have given to another position of this very batch by now -- and the first game to put the launch's stamp on the row
// solves it, so a row shared by de-duplicated games is solved once.  A search leaf always has a legal move (descend_one ends on a finished
// board as TERMINAL), sv_sign covers the other cases all the same.
struct SolveLeavesDev {
    int E, cap, hits;                                     // rows with <= E empties; the network's rows are [0, min(cap, *batch_count)); hits: the game blocks are there
    uint64_t corners;
    unsigned stamp;                                       // of this launch, never 0
    unsigned* claim;                                      // [G] the stamp of the launch that solved the row last
    unsigned long long* rows;                             // rows solved so far
};
__global__ __launch_bounds__(64) void k_solve_leaves(MctsDev t, SolveLeavesDev sl) {
    __shared__ SolveLdsW L;
    const int lane = threadIdx.x;
    int row = blockIdx.x;
    uint64_t own, opp;
    if (row < sl.cap) {
        if (row >= *t.batch_count) return;
        own = t.batch_own[row]; opp = t.batch_opp[row];
    } else {
        const int g = row - sl.cap;
        if (g >= t.G || t.leaf_status[g] != OZ_LEAF_EVAL) return;
        row = t.leaf_slot[g];
        if (row < t.G - *t.hit_count || row >= t.G) return;              // the network's row: solved above
        own = t.leaf_own[g]; opp = t.leaf_opp[g];
    }
    const int empties = t.n2 - oz_popc(own | opp);
    if (empties > sl.E) return;
    if (blockIdx.x >= (unsigned)sl.cap) {
        int mine = 0;
        if (lane == 0) mine = atomicExch(&sl.claim[row], sl.stamp) != sl.stamp;
        if (!__shfl(mine, 0, 64)) return;
    }
    const int sg = sv_sign(L, t.valid, sl.corners, lane, own, opp, empties);
    if (lane == 0) { t.v[row] = (float)sg; atomicAdd(sl.rows, 1ULL); }
}

// ---------------------------------------------------------------- K5 + K6: expand and backup
__device__ __forceinline__ void q_update(const MctsDev& t, OzEdge* e, double val, int vt) {
    const uint32_t nt = e->n_tag;
    const int N = (int)(nt & ~OZ_TAG_F32);
    const bool q32 = (nt & OZ_TAG_F32) != 0;
    const double Q = e->q;
    uint32_t tag = 0;
    double q;
    if (t.qmode == OZ_QMODE_F64 || (!q32 && vt != VT_F32)) {
        q = ((double)N * Q + val) / (double)(N + 1);                 // MCTS/__init__.py:68 in float64
    } else {                                                          // NumPy >= 2 weak-scalar promotion
        const float prod = q32 ? (float)N * (float)Q : (float)((double)N * Q);
        const float s = prod + (float)val;
        q = (double)(s / (float)(N + 1));
        tag = OZ_TAG_F32;
    }
    e->q = q;
    e->n_tag = (uint32_t)(N + 1) | tag;
}

// one descent's end as the expand + backup sees it: the one-descent-per-step kernels fill it from the per-game arrays (leaf_*[g], depth[g], path[g]),
// the leaf-parallel ones from the per-(game, j) arrays
struct LeafRef {
    int status;
    uint64_t own, opp, legal;
    int slot;                  // row of pi / v
    int fs;                    // free table slot for the new node
    int depth, tval;
    const int2* path;          // [depth]
};
// backup (MCTS/__init__.py:68-71): the level-d caller sees the leaf value negated (depth-1-d) times; all levels in
// parallel, one lane per level (a path never visits a node twice: every move adds a disc)
// `value` = the leaf's value for the side to move there; what each level stores of it is oz_backup_value (oz_common.h) under VS: the
// reference's one negation per level, or -- sound -- one per level at which the descent swapped sides (the sigma bits of the frontier)
// proofs: the loop of the backup, after the Q update (lane 0; one entry per level, and it usually ends after one or two).  leaf = V_L, exact.
__device__ __forceinline__ void proof_backup(const MctsDev& t, int g, int depth, const int2* __restrict__ path, int leaf) {
    unsigned long long* st = t.pf.stat + (size_t)g * OZ_NPSTAT;
    int x = leaf;
    for (int d = depth - 1; d >= 0; --d) {
        const int2 pe = path[d];
        if ((unsigned)pe.x >= (unsigned)t.node_cap) return;         // (backup_one has raised EF_CORRUPT)
        OzProof* pp = t.pf.entry + (size_t)g * t.node_cap + pe.x;
        OzProof p = *pp;
        const int rank = pe.y & (OZ_PATH_SWAP - 1);
        uint64_t rest = p.legal;                                    // the square of the edge: the rank-th legal one
        for (int i = 0; i < rank; ++i) rest &= rest - 1;
        if (rest == 0) { atomicOr(t.error_flag, EF_CORRUPT); return; }
        x = (pe.y & OZ_PATH_SWAP) ? -x : x;
        const int before = oz_proof_value(p.legal, p.lo, p.hi, p.own);
        const int r = oz_proof_mark(&p.lo, &p.hi, oz_ctz(rest), x);
        if (r < 0) atomicOr(t.error_flag, EF_CORRUPT);
        if (r > 0) { pp->lo = p.lo; pp->hi = p.hi; st[PS_EDGES] += 1; }
        const int v = oz_proof_value(p.legal, p.lo, p.hi, p.own);
        if (v == OZ_PROOF_NONE) return;
        if (d == 0 && before == OZ_PROOF_NONE) st[PS_ROOTS] += 1;
        x = v;
    }
}
template <int VS>
__device__ __forceinline__ void backup_one(const MctsDev& t, int g, int lane, int depth, const int2* __restrict__ path, double value, int vt, bool exact = false) {
    int2 pe = make_int2(0, 0);
    if (lane < depth) pe = path[lane];
    const uint64_t swaps = VS != OZ_VSIGNS_REFERENCE ? __ballot((pe.y & OZ_PATH_SWAP) != 0) : 0;          // (lanes at or above depth hold 0)
    if (lane < depth) {
        const int rank = path_rank<VS>(pe.y);
        const double val = oz_backup_value(oz_vsigns_rule(VS), swaps, depth, lane, value);
        if ((unsigned)pe.x < (unsigned)t.node_cap && (unsigned)rank < (unsigned)t.row_cap) {
            q_update(t, rec_edge(t, g, pe.x, rank), val, vt);
            *rec_Ns(t, g, pe.x) += 1;
        } else atomicOr(t.error_flag, EF_CORRUPT);
    }
    if (lane == 0) {
        t.last_value[g] = oz_backup_last(oz_vsigns_rule(VS), swaps, depth, value);
        t.last_vtype[g] = vt;
    }
    if constexpr (VS == OZ_VSIGNS_PROVEN) {
        if (exact && lane == 0) proof_backup(t, g, depth, path, (int)value);
    }
}
// expand the leaf if it needs it, then back its value up along its path.  GUMBEL: the new node's header keeps the value the expansion backs
// up, before negation (the network's v, or the exact one where solve_leaves replaced it) -- vhat of the completed-Q formula, in header word 3.
// SEL: the same word, vhat of the selection rule's FPU
template <bool GUMBEL = false, int VS = OZ_VSIGNS_REFERENCE, bool SEL = false>
__device__ __forceinline__ void expand_backup_one(const MctsDev& t, TreeLds& L, int g, int lane, const LeafRef& lf) {
    const int status = lf.status;
    if (status == OZ_LEAF_IDLE || status == OZ_LEAF_WAIT) return;           // (WAIT: the leaf was not in the batch, nothing to expand yet)
    double value;
    int vt;
    bool exact = false;
    if (status == OZ_LEAF_EVAL) {
        // first visit (MCTS/__init__.py:44-57): P = pi * mask, normalised; uniform over legal if the sum is 0
        const uint64_t own = lf.own, opp = lf.opp, legal = lf.legal;
        const int slot = lf.slot;
        const int r = lane >> 3, c = lane & 7, n = t.n;
        const bool inb = r < n && c < n, is_legal = (legal >> lane) & 1;
        const int a = r * n + c;
        double p = is_legal ? (double)t.pi[(size_t)slot * t.n2 + a] : 0.0;     // float32 * float64 mask
        if (inb) L.arr[a] = p;
        __syncthreads();
        const double sum = pairwise_sum(L.arr, t.n2);
        const int cnt = oz_popc(legal);
        if (sum > 0) p = p / sum;
        else p = is_legal ? 1.0 / (double)cnt : 0.0;                           // mask / np.sum(mask)
        const int node = unii(t.node_count[g]), fs = lf.fs, depth = lf.depth;
        const bool ok = node < t.node_cap && cnt <= t.row_cap && fs >= 0;
        if (ok) {
            // build the record in LDS (header + one edge per legal square, N = 0, Q = 0, child unknown), store it with one
            // wave-wide 16-byte store, link it into the table and into the edge we came through
            uint64_t* w = reinterpret_cast<uint64_t*>(L.rec);
            if (lane == 0) {
                w[0] = own; w[1] = opp; w[2] = (uint64_t)(uint32_t)cnt << 32; w[3] = 0;
                if constexpr (GUMBEL || SEL) w[3] = (uint64_t)__double_as_longlong((double)t.v[slot]);
            }
            if (is_legal) {
                const int rank = edge_rank(legal, lane);
                w[4 + 3 * rank] = 0xFFFFFFFF00000000ULL;                       // N|tag = 0, child = -1
                w[5 + 3 * rank] = 0;                                           // Q = 0.0
                w[6 + 3 * rank] = (uint64_t)__double_as_longlong(p);
            }
            if (lane == 63 && (cnt * 3) % 2) w[4 + 3 * cnt] = 0;               // the last 16-byte chunk is half used: no stale bytes
            __syncthreads();
            const int chunks = (OZ_REC_HDR + cnt * OZ_EDGE_BYTES + 15) >> 4;
            if (lane < chunks) reinterpret_cast<uint4*>(rec_ptr(t, g, node))[lane] = L.rec[lane];
            if constexpr (VS == OZ_VSIGNS_PROVEN) {
                // the node's proof entry, whole (a reused pool slot inherits nothing); a solved leaf's v is its exact sign: the node's own value
                int ownv = OZ_PROOF_NONE;
                if (t.pf.E > 0 && t.n2 - oz_popc(own | opp) <= t.pf.E) ownv = (int)t.v[slot];
                exact = ownv != OZ_PROOF_NONE;
                if (lane == 0) {
                    t.pf.entry[(size_t)g * t.node_cap + node] = OzProof{0, 0, legal, ownv, 0};
                    if (exact && depth == 0) t.pf.stat[(size_t)g * OZ_NPSTAT + PS_ROOTS] += 1;
                }
            }
            if (lane == 0) {
                t.node_count[g] = node + 1;
                t.ht[(size_t)g * t.ht_cap + fs] = ht_entry(own, opp, node);
                if (depth > 0) {
                    const int2 pe = lf.path[depth - 1];
                    rec_edge(t, g, pe.x, path_rank<VS>(pe.y))->child = node;
                } else t.root_node[g] = node;
            }
        }
        if (lane == 0) {
            unsigned long long* st = t.stat + (size_t)g * OZ_NSTAT;
            st[ST_EXPAND] += 1;
            if (!(sum > 0)) st[ST_FALLBACK] += 1;
            if (!ok) atomicOr(t.error_flag, node >= t.node_cap || fs < 0 ? EF_NODES : EF_EDGES);
        }
        value = (double)t.v[slot];                                             // v for the leaf's mover (return -v, :57: the negation is the backup rule's)
        vt = t.qmode == OZ_QMODE_F64 ? VT_F64 : VT_F32;
    } else {
        value = (double)lf.tval;
        vt = VT_INT;
        exact = true;
    }
    backup_one<VS>(t, g, lane, lf.depth, lf.path, value, vt, exact);
}
// ... of the descent select_body stored in the per-game arrays.  slot_is_game != 0: pi / v are indexed by game (host evaluator path); else
// by compacted slot.
template <int VS>
__device__ __forceinline__ void backup_body(const MctsDev& t, int g, int lane, double value, int vt) {
    backup_one<VS>(t, g, lane, t.depth[g], t.path + (size_t)g * OZ_MAX_DEPTH, value, vt);
}
template <bool GUMBEL = false, int VS = OZ_VSIGNS_REFERENCE, bool SEL = false>
__device__ __forceinline__ void expand_backup_body(const MctsDev& t, TreeLds& L, int g, int lane, int slot_is_game) {
    LeafRef lf;
    lf.status = unii(t.leaf_status[g]);
    lf.own = uni64(t.leaf_own[g]); lf.opp = uni64(t.leaf_opp[g]); lf.legal = uni64(t.leaf_legal[g]);
    lf.slot = slot_is_game ? g : unii(t.leaf_slot[g]);
    lf.fs = unii(t.leaf_fs[g]);
    lf.depth = unii(t.depth[g]); lf.tval = unii(t.term_value[g]);
    lf.path = t.path + (size_t)g * OZ_MAX_DEPTH;
    expand_backup_one<GUMBEL, VS, SEL>(t, L, g, lane, lf);
}
// ---- the tree kernels: one template per phase, instantiated per variant.  V is a mask of TV_* flags; tree_kernels() (host side) computes it
// from the object's state and is the one place that says which masks have a kernel.  An object without an option launches the instantiations
// without its flag, which are the code they were before the option existed, register for register.
//   flag        option (what sets it)                                   what the bodies do with it
//   TV_SIGNS    the low two bits ARE the OZ_VSIGNS_* value:             VS of every body: the backup's signs, sigma riding in the path entries;
//               value signs (oz_*_set_value_signs: SOUND), proofs       PROVEN also keeps, backs up and descends by the proof entries (t.pf)
//               (oz_*_set_proofs: PROVEN); 0 = the reference's rule
//   TV_NOISE    root noise, from the object's first arming on           NOISE of the descent: an armed slot's depth 0 sees (1 - eps) P + eps eta;
//               (oz_mcts::noise_ever)                                   the expansion and the backup never look at it (k_*expand_backup: never set)
//   TV_SEL      selection (oz_*_set_selection, t.sel.flags != 0)        SEL: U by the selection rule of oz_common.h; a new node keeps vhat for its FPU
//   TV_GUMBEL   the Gumbel search, from its first setting on            GUMBEL: an armed root picks by the Gumbel rule (reads gd; nobody else does);
//               (oz_mcts::gumbel_ever); one descent per step only       a new node keeps vhat for the completed Q
enum : unsigned { TV_SIGNS = 3, TV_NOISE = 4, TV_SEL = 8, TV_GUMBEL = 16 };
constexpr bool has(unsigned v, unsigned flag) { return (v & flag) != 0; }
// between the expand + backup of one step and what the same wave does next in the same launch: the wave's own stores (records, child indices,
// table entry, root index) before its loads, and the LDS stage free again
__device__ __forceinline__ void backup_fence() {
    wave_sync();
    __syncthreads();
}
template <unsigned V>
__global__ __launch_bounds__(64) void k_select(MctsDev t, GumbelDev gd) {
    __shared__ TreeLds L;
    select_body<has(V, TV_NOISE), has(V, TV_GUMBEL), int(V & TV_SIGNS), has(V, TV_SEL)>(t, L, blockIdx.x, threadIdx.x, &gd);
}
template <unsigned V>
__global__ __launch_bounds__(64) void k_expand_backup(MctsDev t, int slot_is_game) {
    static_assert(!has(V, TV_NOISE), "root noise is the descent's alone: one expand + backup for both");
    __shared__ TreeLds L;
    expand_backup_body<has(V, TV_GUMBEL), int(V & TV_SIGNS), has(V, TV_SEL)>(t, L, blockIdx.x, threadIdx.x, slot_is_game);
}
// expand + backup of simulation s-1 and the descent of simulation s in ONE launch (same wave, same game): one kernel boundary
// less per simulation step, and the records the backup has just written are re-read by the descent while still in the CU's cache
template <unsigned V>
__global__ __launch_bounds__(64) void k_backup_select(MctsDev t, GumbelDev gd) {
    __shared__ TreeLds L;
    expand_backup_body<has(V, TV_GUMBEL), int(V & TV_SIGNS), has(V, TV_SEL)>(t, L, blockIdx.x, threadIdx.x, 0);
    backup_fence();
    select_body<has(V, TV_NOISE), has(V, TV_GUMBEL), int(V & TV_SIGNS), has(V, TV_SEL)>(t, L, blockIdx.x, threadIdx.x, &gd);
}


// ---------------------------------------------------------------- leaf-parallel search: K leaves per game and step under virtual loss
// (opt-in: oz_mcts_set_leaves_per_step; the kernels above stay the default and are what K = 1 runs.  Both sets of kernels walk the tree with
// the one descend_one and expand and back up with the one expand_backup_one: the k_wide_* bodies below add the loop over the step's descents
// and the per-(game, j) arrays.)  For ONE game and ONE step, with `left` = simulations of the current simulate call still to run:
//   1. for j = 0 .. min(K, left) - 1, one after the other, the game's wave descends from the root (descend_one), where
//      at a node s at depth d the statistics are seen through the descents of this step already in flight: k(s, a) = the number of them
//      whose level d is (s, a), k(s) = the number whose level d is at s (a state sits at one depth only, so level d is all there is to
//      compare: <= K - 1 compares per level).  k(s, a) == 0: N' = N, Q' = Q, the stored bits.  Otherwise N' = N + k and
//      Q' = ((double)N * Q - (double)k) / (double)(N + k) in float64 (every in-flight descent counts as one visit that returned -1 to the
//      chooser; a view, nothing is stored and the Q type tag is not touched).  U = Q' + (c * P) * (sqrt((double)(Ns + k(s))) / (double)(1 + N')).
//   2. a descent that ends on a finished board joins the in-flight set with its integer value; one that ends on a state not in the table
//      joins it as a leaf -- unless an earlier leaf of this step is the same board (its child edge is still -1, the table does not know it:
//      the boards are compared), then it is DISCARDED (no simulation, counted in the collision counter only) and the step closes for the game.
//   3. all leaves of all games form one batch in (game, j) order (k_wide_compact); EVERY leaf is evaluated: no cross-game de-duplication
//      and no evaluation cache here (results would be identical), so leaves_evaluated == expansions for K > 1.
//   4. per game, j ascending: expand leaf j (the table is probed again for the free slot: two pending leaves of one step may have been
//      shown the same one), back its value up along path j with q_update; a terminal descent in its place in that order.
//   5. left -= the descents of the step.  A simulate call runs steps until every game has done exactly nsims simulations.
// At K = 1 this is the search above (oz_mcts_use_wide_kernels runs it through these kernels: the reference's traces hold them bit for bit in
// both Q regimes).  At K > 1 the float64 regime is held against a restatement (tests/wide_search_ref.py); OZ_QMODE_NEP50 has no replay of its
// own at K > 1: the view above is float64 in both regimes and everything stored goes through the one q_update, so it holds by construction.
struct WideDev {
    int K;                                       // descents per game and step
    int *status, *depth, *term_value, *slot;     // [G][OZ_MCTS_MAX_LEAVES_PER_STEP]
    uint64_t *own, *opp, *legal;                 // [G][OZ_MCTS_MAX_LEAVES_PER_STEP]
    int2* path;                                  // [G][OZ_MCTS_MAX_LEAVES_PER_STEP][OZ_MAX_DEPTH]
    int* count;                                  // [G] descents in flight (between a wide descent and its expand + backup)
    int* left;                                   // [G] simulations of the current simulate call still to run
    int* max_left;                               // [1] the largest `left` (k_wide_left)
    unsigned long long* stat;                    // [G][3] steps, descents discarded on a collision, leaves handed to the network
};
#define OZ_WK OZ_MCTS_MAX_LEAVES_PER_STEP
struct WideLds {
    TreeLds t;
    int2 path[OZ_WK][OZ_MAX_DEPTH];              // the frontiers of the step's descents
    uint64_t own[OZ_WK], opp[OZ_WK];             // where they ended
    int depth[OZ_WK], status[OZ_WK];
};

template <bool NOISE = false, int VS = OZ_VSIGNS_REFERENCE, bool SEL = false>
__device__ __forceinline__ void wide_select_body(const MctsDev& t, const WideDev& w, WideLds& L, int g, int lane) {
    const int left = t.active[g] ? unii(w.left[g]) : 0;
    const int nd = left < w.K ? left : w.K;
    if (nd <= 0) {
        if (lane == 0) w.count[g] = 0;
        return;
    }
    double eta = 0.0;
    const bool noisy = noise_of_slot<NOISE>(t, g, lane, &eta);
    const uint64_t rown = uni64(t.root_own[g]), ropp = uni64(t.root_opp[g]);
    const uint64_t rlegal = oz_legal(rown, ropp, t.valid);
    int rootn = unii(t.root_node[g]);
    int count = 0, coll = 0, leaves = 0, nterm = 0, visits = 0, err = 0;
    const size_t gb = (size_t)g * OZ_WK;
    for (int j = 0; j < nd; ++j) {
        const Descent e = descend_one<NOISE, false, VS, SEL>(t, L.t.rec, L.path[j], g, lane, rown, ropp, rlegal, rootn, noisy, eta, InFlight{L.path, L.depth, j});
        if (e.err) { err = e.err; break; }                                      // the step stops here for this game (nothing of this descent is stored)
        if (e.status == OZ_LEAF_EVAL) {
            bool same = false;
            for (int i = 0; i < j; ++i) same = same || (L.status[i] == OZ_LEAF_EVAL && L.own[i] == e.own && L.opp[i] == e.opp);
            if (same) { coll = 1; break; }                                      // discarded: the step's collection closes for this game
            ++leaves;
        } else ++nterm;
        if (lane == 0) {
            L.own[j] = e.own; L.opp[j] = e.opp; L.depth[j] = e.depth; L.status[j] = e.status;
            w.status[gb + j] = e.status; w.own[gb + j] = e.own; w.opp[gb + j] = e.opp; w.legal[gb + j] = e.legal;
            w.depth[gb + j] = e.depth; w.term_value[gb + j] = e.tval;
        }
        ++count;
        visits += e.depth + 1;
        wave_sync();                                                            // lane 0's frontier / child-index stores before the next descent's loads
    }
    wave_sync();
    for (int i = 0; i < count; ++i)
        if (lane < L.depth[i]) w.path[(gb + i) * OZ_MAX_DEPTH + lane] = L.path[i][lane];
    if (lane == 0) {
        w.count[g] = count;
        unsigned long long* st = t.stat + (size_t)g * OZ_NSTAT;
        st[ST_SIMS] += (unsigned long long)count; st[ST_VISITS] += (unsigned long long)visits; st[ST_TERMINAL] += (unsigned long long)nterm;
        unsigned long long* ws = w.stat + (size_t)g * 3;
        ws[0] += 1; ws[1] += (unsigned long long)coll; ws[2] += (unsigned long long)leaves;
        if (err) {
            atomicOr(t.error_flag, err);
            w.left[g] = count;                                                  // nothing more for this game: the host's loop ends, the caller gets the error
        }
    }
}

// per game, j ascending: expand leaf j / take the terminal value, back it up along path j
template <int VS = OZ_VSIGNS_REFERENCE, bool SEL = false>
__device__ __forceinline__ void wide_expand_backup_body(const MctsDev& t, const WideDev& w, WideLds& L, int g, int lane) {
    const int count = unii(w.count[g]);
    if (count <= 0) return;
    const size_t gb = (size_t)g * OZ_WK;
    int depth = 0;
    for (int j = 0; j < count; ++j) {
        LeafRef lf;
        lf.status = unii(w.status[gb + j]);
        lf.own = uni64(w.own[gb + j]); lf.opp = uni64(w.opp[gb + j]); lf.legal = uni64(w.legal[gb + j]);
        lf.slot = unii(w.slot[gb + j]);
        lf.depth = depth = unii(w.depth[gb + j]); lf.tval = unii(w.term_value[gb + j]);
        lf.path = w.path + (gb + j) * OZ_MAX_DEPTH;
        lf.fs = -1;
        if (lf.status == OZ_LEAF_EVAL) {                                        // the free slot NOW: the earlier leaves of the step are in
            int fs = -1;
            if (ht_find(t, g, lf.own, lf.opp, lane, &fs) >= 0) fs = -1;          // (cannot be in the table: the step holds a board once)
            lf.fs = fs;
        }
        expand_backup_one<false, VS, SEL>(t, L.t, g, lane, lf);
        wave_sync();                                                            // records, table entry, Q / N of this descent before the next one's loads
        __syncthreads();
    }
    if (lane == 0) {
        w.left[g] -= count;
        w.count[g] = 0;
        t.depth[g] = depth;                                                     // oz_mcts_last_value: of the last simulation backed up
    }
}
// the leaf-parallel tree kernels: V as above (no TV_GUMBEL: the Gumbel search runs one descent per step)
template <unsigned V>
__global__ __launch_bounds__(64) void k_wide_select(MctsDev t, WideDev w) {
    static_assert(!has(V, TV_GUMBEL), "the Gumbel search has no leaf-parallel kernels");
    __shared__ WideLds L;
    wide_select_body<has(V, TV_NOISE), int(V & TV_SIGNS), has(V, TV_SEL)>(t, w, L, blockIdx.x, threadIdx.x);
}
template <unsigned V>
__global__ __launch_bounds__(64) void k_wide_expand_backup(MctsDev t, WideDev w) {
    static_assert(!has(V, TV_GUMBEL), "the Gumbel search has no leaf-parallel kernels");
    static_assert(!has(V, TV_NOISE), "root noise is the descent's alone: one expand + backup for both");
    __shared__ WideLds L;
    wide_expand_backup_body<int(V & TV_SIGNS), has(V, TV_SEL)>(t, w, L, blockIdx.x, threadIdx.x);
}
// expand + backup of step s-1 and the descents of step s in ONE launch (the wide counterpart of k_backup_select)
template <unsigned V>
__global__ __launch_bounds__(64) void k_wide_backup_select(MctsDev t, WideDev w) {
    static_assert(!has(V, TV_GUMBEL), "the Gumbel search has no leaf-parallel kernels");
    __shared__ WideLds L;
    wide_expand_backup_body<int(V & TV_SIGNS), has(V, TV_SEL)>(t, w, L, blockIdx.x, threadIdx.x);
    backup_fence();
    wide_select_body<has(V, TV_NOISE), int(V & TV_SIGNS), has(V, TV_SEL)>(t, w, L, blockIdx.x, threadIdx.x);
}
// dense batch in (game, j) order: prefix sum over the per-game leaf counts
__global__ __launch_bounds__(1024) void k_wide_compact(MctsDev t, WideDev w) {
    __shared__ int wtot[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int start = 0; start < t.G; start += 1024) {
        const int g = start + tid;
        const size_t gb = (size_t)g * OZ_WK;
        int cnt = 0, n = 0;
        if (g < t.G) {
            cnt = w.count[g];
            for (int j = 0; j < cnt; ++j) n += w.status[gb + j] == OZ_LEAF_EVAL ? 1 : 0;
        }
        int x = n;                                                              // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) wtot[wv] = x;
        __syncthreads();
        int woff = 0, total = 0;
        for (int i = 0; i < 16; ++i) { const int y = wtot[i]; if (i < wv) woff += y; total += y; }
        int pos = base_s + woff + x - n;
        for (int j = 0; j < cnt; ++j)
            if (w.status[gb + j] == OZ_LEAF_EVAL) {
                w.slot[gb + j] = pos;
                t.batch_own[pos] = w.own[gb + j];
                t.batch_opp[pos] = w.opp[gb + j];
                ++pos;
            }
        __syncthreads();
        if (tid == 0) base_s += total;
        __syncthreads();
    }
    if (tid == 0) { *t.batch_count = base_s; *t.eval_leaves += (unsigned long long)base_s; }
}
__global__ void k_wide_begin(MctsDev t, WideDev w, int nsims) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G) return;
    w.left[g] = t.active[g] ? nsims : 0;
    w.count[g] = 0;
}
// the keys a lock-step round under a playout cap evaluates oz_playout_budget with: the slots' (game id, ply) and the engine's seed
struct CapKeys { PlayoutCap pc; uint64_t seed; const uint64_t* game_id; const int* ply; };
__device__ __forceinline__ int cap_budget(const CapKeys& ck, int g, int nsims, int* fast) {
    return oz_playout_budget(ck.seed, ck.game_id[g], (uint64_t)ck.ply[g], nsims, ck.pc.fast_sims, ck.pc.full_prob, fast);
}
// k_wide_begin under a playout cap: every game's own budget (mcts_wide_steps runs until the largest remaining one is zero)
__global__ void k_wide_begin_c(MctsDev t, WideDev w, int nsims, CapKeys ck) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G) return;
    int fast;
    w.left[g] = t.active[g] ? cap_budget(ck, g, nsims, &fast) : 0;
    w.count[g] = 0;
}
// one-descent-per-step rounds under a playout cap: after the first fast_sims simulations the slots whose move is fast sit out the rest (an
// inactive slot descends nowhere and backs nothing up, as in a staggered round); k_cap_resume brings them back for the move (a round under
// the cap is never a staggered one: every live game takes part, so "live" is "active")
__global__ void k_cap_park(MctsDev t, CapKeys ck) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G || !t.active[g]) return;
    int fast;
    cap_budget(ck, g, 0, &fast);
    if (fast) t.active[g] = 0;
}
__global__ void k_cap_resume(MctsDev t, const uint8_t* __restrict__ finished) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < t.G) t.active[g] = finished[g] ? 0 : 1;
}
// k_root_noise under a playout cap: the full moves draw, a fast move's slot stays disarmed (its descents read the stored priors)
__global__ __launch_bounds__(64) void k_root_noise_c(MctsDev t, double alpha, CapKeys ck) {
    __shared__ double arr[64];
    const int g = blockIdx.x, lane = threadIdx.x;
    int fast = 0;
    if (t.active[g]) cap_budget(ck, g, 0, &fast);
    if (!t.active[g] || unii(fast)) {
        if (lane == 0) t.noise_armed[g] = 0;
        return;
    }
    root_noise_body(t, arr, g, lane, uni64(t.root_own[g]), uni64(t.root_opp[g]), alpha, ck.seed, uni64(ck.game_id[g]), unii(ck.ply[g]));
}
__global__ void k_wide_left(MctsDev t, WideDev w) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int left = g < t.G ? w.left[g] : 0;
    const int m = wave_max_i32(left);
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(w.max_left, m);
}

// tree collection ("tree collection" below): what k_tree_collect gets beside MctsDev.  An object that never arms it allocates and passes nothing.
enum { GC_COLLECTIONS = 0, GC_BEFORE = 1, GC_KEPT = 2, GC_PEAK_NODES = 3, GC_PEAK_KEPT = 4, OZ_NGCSTAT = 5 };
struct TreeGcDev {
    int* map;                  // [G][node_cap] old index -> new index, -1 where dropped (scratch of one launch)
    long long* stat;           // [G][OZ_NGCSTAT] per game, no atomics: summed / maximised at the read
    long long* last;           // [G][2] nodes before, nodes kept of the LAST launch (0, 0 where the slot was not collected)
    int mode;                  // OZ_TREE_GC_ON_DEMAND: only where node_count + sims > node_cap; OZ_TREE_GC_EVERY_MOVE: every active slot
    int sims;
};

// ---------------------------------------------------------------- host object
struct oz_mcts {
    MctsDev d;
    hipStream_t stream = nullptr;
    int device = 0;
    std::mutex mu;
    bool selected = false;
    std::vector<void*> allocs;
    // HIP-event timing on the launch stream: slot TS_NN (the evaluator's launches) whenever a driver asks for it,
    // the tree kernels too when `profile` is on (oz_selfplay_profile)
    OzTimer timer{OZ_TREE_KERNELS};
    bool profile = false;
    unsigned batch_no = 0;           // batches evaluated (stamp of the evaluation-cache inserts)
    // staging of oz_mcts_root_counts (called once per move by the drop-in agents): lives with the object
    int32_t* rc_counts = nullptr; uint64_t* rc_legal = nullptr; int32_t* rc_rc = nullptr;
    // leaf-parallel search (oz_mcts_set_leaves_per_step): w.status == nullptr until it is asked for
    WideDev w{};
    int leaves_per_step = 1;
    bool use_wide = false;           // oz_mcts_use_wide_kernels: K = 1 through the wide kernels
    bool wide() const { return leaves_per_step > 1 || use_wide; }
    // root noise: true from the first arming on (d.noise_eta / d.noise_armed are then allocated): the descents run on the TV_NOISE kernels
    bool noise_ever = false;
    uint64_t* noise_ids = nullptr; int32_t* noise_plies = nullptr;      // staging of the keys of oz_mcts_sample_root_noise / oz_mcts_sample_moves, [G] each
    // Gumbel search: true from the first oz_mcts_set_gumbel / oz_mcts_sample_gumbel on (gd's arrays are then allocated): the object runs on the TV_GUMBEL kernels
    bool gumbel_ever = false;
    GumbelDev gd{};
    int* gumbel_table = nullptr; size_t gumbel_table_len = 0;           // the device copy of the schedule gd.table points to
    uint8_t* gumbel_want = nullptr;                                     // [G] staging of the host's `armed`
    float* gumbel_pi = nullptr; double* gumbel_score = nullptr;         // [G][64] each: what k_gumbel_policy wrote last
    // solved leaves (oz_mcts_set_solve_leaves): 0 = off, nothing allocated and nothing launched
    int solve_leaves = 0;
    // value signs of the backup (oz_mcts_set_value_signs): which instantiation of the tree kernels the object launches
    int vsigns = OZ_VSIGNS_REFERENCE;
    // proofs (oz_mcts_set_proofs): on top of sound signs, the OZ_VSIGNS_PROVEN instantiations (d.pf's arrays are allocated at the first setting)
    bool proofs = false;
    unsigned solve_stamp = 0;
    unsigned* solve_claim = nullptr; unsigned long long* solve_rows = nullptr;
    bool solve_profile = false;      // oz_mcts_solve_leaves_profile: HIP events around k_solve_leaves
    OzTimer solve_timer{1};
    // tree collection (oz_mcts_collect, oz_*_set_tree_gc): gc.map == nullptr until the object's first arming
    TreeGcDev gc{};
    bool gc_profile = false;         // oz_selfplay_tree_gc_profile: HIP events around k_tree_collect
    OzTimer gc_timer{1};

    template <typename T> int alloc(T** p, size_t count) {
        OZ_HIP(hipMalloc((void**)p, sizeof(T) * (count ? count : 1)));
        allocs.push_back(*p);
        return OZ_OK;
    }
};

static int next_pow2(int x) { int p = 64; while (p < x) p <<= 1; return p; }

static int mcts_reset_locked(oz_mcts* m, int game) {
    MctsDev& d = m->d;
    if (game < 0) {
        OZ_HIP(hipMemsetAsync(d.node_count, 0, sizeof(int) * d.G, m->stream));
        OZ_HIP(hipMemsetAsync(d.root_node, 0xFF, sizeof(int) * d.G, m->stream));
        OZ_HIP(hipMemsetAsync(d.ht, 0, sizeof(uint32_t) * (size_t)d.G * d.ht_cap, m->stream));
    } else {
        OZ_REQUIRE(game < d.G, "game index %d out of range", game);
        OZ_HIP(hipMemsetAsync(d.node_count + game, 0, sizeof(int), m->stream));
        OZ_HIP(hipMemsetAsync(d.root_node + game, 0xFF, sizeof(int), m->stream));
        OZ_HIP(hipMemsetAsync(d.ht + (size_t)game * d.ht_cap, 0, sizeof(uint32_t) * (size_t)d.ht_cap, m->stream));
    }
    return OZ_OK;
}

// row capacity of a node record: the largest legal-move count the board can show (n*n - 4 empty squares at most), capped
// so that a record fits one wave-wide 16-byte load (1024 B = header + 41 edges; 33 is the known maximum mobility of 8x8
// Othello positions).  A position with more legal moves raises OZ_ERR_CAPACITY, never a silent truncation.
static int row_cap_for(int n) { const int e = n * n - 4; return e < 41 ? e : 41; }

static int mcts_create(oz_mcts** out, int n, int G, int node_cap, double c, int q_mode) {
    OZ_REQUIRE(n == 4 || n == 6 || n == 8, "board size must be 4, 6 or 8 (got %d)", n);
    OZ_REQUIRE(G > 0 && node_cap > 0, "num_games and node_cap must be positive");
    OZ_REQUIRE(node_cap < (int)OZ_HT_IDX_MASK, "node_cap %d too large (max %u)", node_cap, OZ_HT_IDX_MASK - 1);
    OZ_REQUIRE(q_mode == OZ_QMODE_NEP50 || q_mode == OZ_QMODE_F64, "unknown q_mode %d", q_mode);
    oz_mcts* m = new oz_mcts();
    m->device = oz_current_device();
    MctsDev& d = m->d;
    memset(&d, 0, sizeof d);
    d.G = G; d.n = n; d.n2 = n * n; d.node_cap = node_cap;
    d.row_cap = row_cap_for(n);
    d.rec_bytes = (OZ_REC_HDR + d.row_cap * OZ_EDGE_BYTES + 63) & ~63;
    d.ht_cap = next_pow2(2 * node_cap);
    d.valid = oz_valid_mask(n); d.c = c; d.qmode = q_mode;
    int rc = OZ_OK;
#define A(ptr, cnt) if (!rc) rc = m->alloc(&d.ptr, cnt)
    A(recs, (size_t)G * node_cap * d.rec_bytes);
    A(node_count, G); A(root_node, G);
    A(ht, (size_t)G * d.ht_cap);
    A(root_own, G); A(root_opp, G); A(active, G);
    A(leaf_status, G); A(leaf_own, G); A(leaf_opp, G); A(leaf_legal, G);
    A(depth, G); A(term_value, G); A(leaf_slot, G); A(leaf_fs, G); A(path, (size_t)G * OZ_MAX_DEPTH);
    A(batch_own, G); A(batch_opp, G); A(batch_count, 1);
    A(pi, (size_t)G * d.n2); A(v, G);
    A(last_value, G); A(last_vtype, G);
    A(stat, (size_t)G * OZ_NSTAT); A(error_flag, 1); A(eval_leaves, 1);
    A(hit_count, 1); A(hit_entry, G);
#undef A
    if (!rc) rc = m->alloc(&m->rc_counts, (size_t)G * 64);
    if (!rc) rc = m->alloc(&m->rc_legal, (size_t)G);
    if (!rc) rc = m->alloc(&m->rc_rc, (size_t)G);
    d.batch_cap = 0; d.batch_rot = 0;
    d.dedup = 1;               // cross-game leaf de-duplication (oz_mcts_set_dedup / oz_selfplay_config.dedup switch it off)
    if (!rc && hipStreamCreate(&m->stream) != hipSuccess) { oz_set_error("hipStreamCreate failed"); rc = OZ_ERR_HIP; }
    if (!rc) {
        hipMemsetAsync(d.stat, 0, sizeof(unsigned long long) * (size_t)G * OZ_NSTAT, m->stream);
        hipMemsetAsync(d.error_flag, 0, sizeof(int), m->stream);
        hipMemsetAsync(d.eval_leaves, 0, sizeof(unsigned long long), m->stream);
        hipMemsetAsync(d.hit_count, 0, sizeof(int), m->stream);
        hipMemsetAsync(d.active, 0, G, m->stream);
        hipMemsetAsync(d.leaf_status, 0, sizeof(int) * G, m->stream);
        hipMemsetAsync(d.batch_count, 0, sizeof(int), m->stream);
        hipMemsetAsync(d.last_value, 0, sizeof(double) * G, m->stream);
        hipMemsetAsync(d.last_vtype, 0, sizeof(int) * G, m->stream);
        hipMemsetAsync(d.depth, 0, sizeof(int) * G, m->stream);
        rc = mcts_reset_locked(m, -1);
        if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) { oz_set_error("stream sync failed"); rc = OZ_ERR_HIP; }
    }
    if (rc) {
        for (void* p : m->allocs) hipFree(p);
        if (m->stream) hipStreamDestroy(m->stream);
        delete m;
        return rc;
    }
    *out = m;
    return OZ_OK;
}

static void mcts_destroy(oz_mcts* m) {
    if (!m) return;
    hipSetDevice(m->device);
    hipStreamSynchronize(m->stream);
    m->timer.destroy();
    m->solve_timer.destroy();
    m->gc_timer.destroy();
    for (void* p : m->allocs) hipFree(p);
    hipStreamDestroy(m->stream);
    delete m;
}

static int check_error_flag(oz_mcts* m) {
    int ef = 0;
    OZ_HIP(hipMemcpyAsync(&ef, m->d.error_flag, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    if (ef & (EF_NODES | EF_EDGES)) {
        if (ef & EF_NODES) oz_set_error("per-game node table overflow (node_cap=%d): raise the capacity", m->d.node_cap);
        else oz_set_error("a position has more than %d legal moves (the row capacity of a node record)", m->d.row_cap);
        return OZ_ERR_CAPACITY;
    }
    if (ef & EF_RECORDS) { oz_set_error("move-record buffer overflow: raise record_cap or drain records more often"); return OZ_ERR_CAPACITY; }
    if (ef & EF_DEPTH) { oz_set_error("search path deeper than %d", OZ_MAX_DEPTH); return OZ_ERR_CAPACITY; }
    if (ef & EF_NOMOVE) { oz_set_error("a revisited state has no legal action (the reference raises ValueError: max() arg is an empty sequence)"); return OZ_ERR_STATE; }
    if (ef & EF_ROOT) { oz_set_error("root state missing from the search table after the simulations"); return OZ_ERR_KEY; }
    if (ef & EF_CORRUPT) { oz_set_error("search table corrupt: a node index outside the pool was met (internal error)"); return OZ_ERR_STATE; }
    return OZ_OK;
}

// the tree kernels of one variant: a call's first descents, every further step's (the step before backed up in the same launch), the closing
// expand + backup; one descent per game and step, and K of them (null where the variant has none)
struct TreeKernels {
    void (*select)(MctsDev, GumbelDev);
    void (*backup_select)(MctsDev, GumbelDev);
    void (*expand_backup)(MctsDev, int);
    void (*wide_select)(MctsDev, WideDev);
    void (*wide_backup_select)(MctsDev, WideDev);
    void (*wide_expand_backup)(MctsDev, WideDev);
};
template <unsigned V> static TreeKernels tree_kernels_of() {
    constexpr unsigned B = V & ~TV_NOISE;                    // root noise is the descent's alone
    if constexpr (has(V, TV_GUMBEL)) return {k_select<V>, k_backup_select<V>, k_expand_backup<B>, nullptr, nullptr, nullptr};
    else return {k_select<V>, k_backup_select<V>, k_expand_backup<B>, k_wide_select<V>, k_wide_backup_select<V>, k_wide_expand_backup<B>};
}
// the tree kernels of the object as it is now.  THE list of the variants that exist: every value signs with and without root noise and the
// selection rule, and the Gumbel search under the reference's and the sound signs alone, one descent per step (the setters refuse the rest)
static int tree_kernels(const oz_mcts* m, TreeKernels* k) {
    const unsigned v = (m->proofs ? OZ_VSIGNS_PROVEN : m->vsigns != OZ_VSIGNS_REFERENCE ? OZ_VSIGNS_SOUND : OZ_VSIGNS_REFERENCE) | (m->noise_ever ? TV_NOISE : 0) |
                       (m->d.sel.flags ? TV_SEL : 0) | (m->gumbel_ever ? TV_GUMBEL : 0);
    switch (v) {
#define OZ_V(...) case (__VA_ARGS__): *k = tree_kernels_of<(__VA_ARGS__)>(); break
        OZ_V(OZ_VSIGNS_REFERENCE); OZ_V(OZ_VSIGNS_REFERENCE | TV_NOISE); OZ_V(OZ_VSIGNS_REFERENCE | TV_SEL); OZ_V(OZ_VSIGNS_REFERENCE | TV_NOISE | TV_SEL);
        OZ_V(OZ_VSIGNS_SOUND); OZ_V(OZ_VSIGNS_SOUND | TV_NOISE); OZ_V(OZ_VSIGNS_SOUND | TV_SEL); OZ_V(OZ_VSIGNS_SOUND | TV_NOISE | TV_SEL);
        OZ_V(OZ_VSIGNS_PROVEN); OZ_V(OZ_VSIGNS_PROVEN | TV_NOISE); OZ_V(OZ_VSIGNS_PROVEN | TV_SEL); OZ_V(OZ_VSIGNS_PROVEN | TV_NOISE | TV_SEL);
        OZ_V(OZ_VSIGNS_REFERENCE | TV_GUMBEL); OZ_V(OZ_VSIGNS_SOUND | TV_GUMBEL);
#undef OZ_V
        default:
            oz_set_error("the search has no tree kernels for value signs %u%s%s%s", v & TV_SIGNS, has(v, TV_NOISE) ? " + root noise" : "",
                         has(v, TV_SEL) ? " + selection" : "", has(v, TV_GUMBEL) ? " + the Gumbel search" : "");
            return OZ_ERR_STATE;
    }
    if (m->wide() && !k->wide_select) { oz_set_error("the Gumbel search runs one leaf per game and step: it has no leaf-parallel kernels"); return OZ_ERR_STATE; }
    return OZ_OK;
}
enum { TS_SELECT = 0, TS_COMPACT = 1, TS_NN = 2, TS_BACKUP = 3, TS_MOVE = 4 };
// the step's solved rows (k_solve_leaves): after the evaluator of EITHER kind of step has written the rows [0, cap) (and the cache has taken
// them), before their expand + backup.  hits: the step may have rows served from the evaluation cache.  Off (the default), nothing is launched.
static void solve_leaves_async(oz_mcts* m, int cap, bool hits) {
    if (m->solve_leaves <= 0) return;
    const MctsDev& d = m->d;
    m->solve_stamp += 1;
    if (m->solve_stamp == 0) m->solve_stamp = 1;             // 0 = "never solved"
    const SolveLeavesDev sl{m->solve_leaves, cap, hits ? 1 : 0, oz_solve_corners(d.n), m->solve_stamp, m->solve_claim, m->solve_rows};
    const long long ti = m->solve_profile ? m->solve_timer.begin(0, m->stream) : -1;
    hipLaunchKernelGGL(k_solve_leaves, dim3((unsigned)(cap + (hits ? d.G : 0))), dim3(64), 0, m->stream, d, sl);
    m->solve_timer.end(ti, m->stream);
    if (m->solve_profile && m->solve_timer.backlog() > 4096) m->solve_timer.drain();
}
// the evaluator's part of a batch: the rows of the leaves k_compact found in the network's evaluation cache (if the search uses one),
// the network on the compacted batch (launched for up to max_count leaves), the evaluated positions into the cache
static int eval_batch_async(oz_mcts* m, oz_net* net, int max_count, bool timed) {
    MctsDev& d = m->d;
    hipStream_t s = m->stream;
    if (d.ec.buckets) hipLaunchKernelGGL(k_cache_copy, dim3((unsigned)(((long long)d.G * 64 + 255) / 256)), dim3(256), 0, s, d);
    const long long ti = timed ? m->timer.begin(TS_NN, s) : -1;
    if (int rc = oz_net_forward_device(net, d.batch_own, d.batch_opp, d.batch_count, max_count, d.pi, d.v, s)) { m->timer.cancel(ti); return rc; }
    m->timer.end(ti, s);
    if (d.ec.buckets) {
        m->batch_no += 1;
        if (m->batch_no == 0) m->batch_no = 1;               // 0 = "never written"
        d.batch_stamp = m->batch_no;
        hipLaunchKernelGGL(k_cache_insert, dim3((unsigned)((max_count + 3) / 4)), dim3(256), 0, s, d);
    }
    solve_leaves_async(m, max_count, d.ec.buckets != 0);
    return OZ_OK;
}

// `launch` on m->stream, between a pair of timing events of slot `slot` if `on`
template <typename F> static void timed(oz_mcts* m, int slot, bool on, F&& launch) {
    const long long i = on ? m->timer.begin(slot, m->stream) : -1;
    launch();
    m->timer.end(i, m->stream);
}

// ---- leaf-parallel search: host side
// the per-(game, j) arrays, and batch / (pi, v) arrays for G * OZ_WK leaves in place of the G-leaf ones (which stay allocated until destroy)
static int wide_alloc(oz_mcts* m) {
    if (m->w.status) return OZ_OK;
    MctsDev& d = m->d;
    WideDev& w = m->w;
    const size_t GK = (size_t)d.G * OZ_WK;
    const size_t held = m->allocs.size();
    int rc = OZ_OK;
#define A(ptr, cnt) if (!rc) rc = m->alloc(&ptr, cnt)
    A(w.depth, GK); A(w.term_value, GK); A(w.slot, GK);
    A(w.own, GK); A(w.opp, GK); A(w.legal, GK); A(w.path, GK * OZ_MAX_DEPTH);
    A(w.count, d.G); A(w.left, d.G); A(w.max_left, 1); A(w.stat, (size_t)d.G * 3);
    uint64_t *bo = nullptr, *bp = nullptr; float *pi = nullptr, *v = nullptr;
    A(bo, GK); A(bp, GK); A(pi, GK * d.n2); A(v, GK);
    A(w.status, GK);
#undef A
    if (rc) {                                                   // all or nothing: give back what this call allocated
        for (size_t i = held; i < m->allocs.size(); ++i) hipFree(m->allocs[i]);
        m->allocs.resize(held);
        w = WideDev{};
        return rc;
    }
    d.batch_own = bo; d.batch_opp = bp; d.pi = pi; d.v = v;
    OZ_HIP(hipMemsetAsync(w.count, 0, sizeof(int) * d.G, m->stream));
    OZ_HIP(hipMemsetAsync(w.left, 0, sizeof(int) * d.G, m->stream));
    OZ_HIP(hipMemsetAsync(w.stat, 0, sizeof(unsigned long long) * 3 * d.G, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
static int wide_check_k(int k) {
    OZ_REQUIRE(k >= 1 && k <= OZ_MCTS_MAX_LEAVES_PER_STEP, "leaves_per_step %d outside 1 .. %d", k, OZ_MCTS_MAX_LEAVES_PER_STEP);
    return OZ_OK;
}
static int wide_set_k(oz_mcts* m, int k) {
    if (k > 1 && m->gumbel_ever) { oz_set_error("leaves_per_step %d: the Gumbel search runs one leaf per game and step", k); return OZ_ERR_STATE; }
    if (k > 1) if (int rc = wide_alloc(m)) return rc;
    m->leaves_per_step = k;
    return OZ_OK;
}

// `nsims` simulations for every active game, K = leaves_per_step descents per game and step: ceil(nsims / K) steps are enqueued without a
// host round trip (descents | compaction | evaluator, the previous step's expand + backup fused with the next step's descents, one closing
// expand + backup), then the largest remaining budget is read back (4 bytes) and further steps follow until it is zero (steps cut short by
// a collision leave a remainder).  max_games = an upper bound of the active games: the evaluator is launched for max_games * K leaves.
static int mcts_wide_steps(oz_mcts* m, oz_net* net, int nsims, int max_games, bool time_eval, const CapKeys* ck = nullptr) {
    MctsDev& d = m->d;
    if (int rc = wide_alloc(m)) return rc;
    TreeKernels tk;
    if (int rc = tree_kernels(m, &tk)) return rc;
    WideDev w = m->w;
    w.K = m->leaves_per_step;
    hipStream_t s = m->stream;
    const bool all = m->profile;
    const int cap = max_games * w.K;
    const dim3 gg((unsigned)((d.G + 255) / 256));
    if (ck) hipLaunchKernelGGL(k_wide_begin_c, gg, dim3(256), 0, s, d, w, nsims, *ck);       // a playout cap: every game's own budget (<= nsims)
    else hipLaunchKernelGGL(k_wide_begin, gg, dim3(256), 0, s, d, w, nsims);
    int steps = (nsims + w.K - 1) / w.K;
    long long enqueued = 0;                                     // every step runs >= 1 simulation of every game with budget left: <= nsims steps in all
    while (steps > 0) {
        enqueued += steps;
        if (enqueued > (long long)nsims) { oz_set_error("leaf-parallel search: the simulation budget did not run out after %d steps (internal error)", nsims); return OZ_ERR_STATE; }
        for (int k = 0; k < steps; ++k) {
            timed(m, TS_SELECT, all, [&] { hipLaunchKernelGGL(k == 0 ? tk.wide_select : tk.wide_backup_select, dim3(d.G), dim3(64), 0, s, d, w); });
            timed(m, TS_COMPACT, all, [&] { hipLaunchKernelGGL(k_wide_compact, dim3(1), dim3(1024), 0, s, d, w); });
            const long long i = (time_eval || all) ? m->timer.begin(TS_NN, s) : -1;
            if (int rc = oz_net_forward_device(net, d.batch_own, d.batch_opp, d.batch_count, cap, d.pi, d.v, s)) { m->timer.cancel(i); return rc; }
            m->timer.end(i, s);
            solve_leaves_async(m, cap, false);              // (no evaluation cache here: every leaf has a row of its own)
        }
        timed(m, TS_BACKUP, all, [&] { hipLaunchKernelGGL(tk.wide_expand_backup, dim3(d.G), dim3(64), 0, s, d, w); });
        OZ_HIP(hipGetLastError());
        int max_left = 0;
        OZ_HIP(hipMemsetAsync(w.max_left, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_wide_left, gg, dim3(256), 0, s, d, w);
        OZ_HIP(hipMemcpyAsync(&max_left, w.max_left, sizeof(int), hipMemcpyDeviceToHost, s));
        OZ_HIP(hipStreamSynchronize(s));
        steps = (max_left + w.K - 1) / w.K;
        if (m->timer.backlog() > 4096) m->timer.drain();
    }
    return OZ_OK;
}

static int mcts_collect_eval_time(oz_mcts* m) {
    if (m->timer.collect() != OZ_OK) { oz_set_error("HIP event timing failed"); return OZ_ERR_HIP; }
    return OZ_OK;
}

// `nsims` simulations for every active game (all on m->stream), leaves evaluated by `net`.  max_games = an upper bound of the active games (<= G):
// the evaluator's launches are made for max_games x leaves_per_step leaves.  One descent per game and step: descent | compaction | evaluator,
// then per further simulation the previous one's expand + backup fused with the next descent (k_backup_select), and one closing expand +
// backup: nsims + 1 tree launches instead of 2 nsims (results are identical to the unfused sequence, which oz_mcts_select / oz_mcts_backup
// still run).  nsims <= 0 launches nothing: the closing expand + backup would run over the leaf_status of an earlier call.
static int mcts_steps_async(oz_mcts* m, oz_net* net, int nsims, int max_games, bool time_eval, const CapKeys* ck = nullptr) {
    if (m->wide()) return mcts_wide_steps(m, net, nsims, max_games, time_eval, ck);
    if (nsims <= 0) return OZ_OK;
    TreeKernels tk;
    if (int rc = tree_kernels(m, &tk)) return rc;
    MctsDev& d = m->d;
    hipStream_t s = m->stream;
    const bool all = m->profile;
    for (int k = 0; k < nsims; ++k) {
        timed(m, TS_SELECT, all, [&] { hipLaunchKernelGGL(k == 0 ? tk.select : tk.backup_select, dim3(d.G), dim3(64), 0, s, d, m->gd); });
        timed(m, TS_COMPACT, all, [&] { hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, s, d); });
        if (int rc = eval_batch_async(m, net, max_games, time_eval || all)) return rc;
    }
    timed(m, TS_BACKUP, all, [&] { hipLaunchKernelGGL(tk.expand_backup, dim3(d.G), dim3(64), 0, s, d, 0); });
    OZ_HIP(hipGetLastError());
    return OZ_OK;
}

OZ_API int oz_mcts_create(oz_mcts** out, int n, int num_games, int node_cap, double c, int q_mode) {
    OZ_REQUIRE(out, "null out pointer");
    return mcts_create(out, n, num_games, node_cap, c, q_mode);
}
OZ_API int oz_mcts_destroy(oz_mcts* m) { mcts_destroy(m); return OZ_OK; }

OZ_API int oz_mcts_set_dedup(oz_mcts* m, int enable) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    m->d.dedup = enable ? 1 : 0;                          // takes effect at the next leaf compaction (kernels get the struct by value)
    return OZ_OK;
}

OZ_API int oz_mcts_reset(oz_mcts* m, int game) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    if (int rc = mcts_reset_locked(m, game)) return rc;
    OZ_HIP(hipStreamSynchronize(m->stream));
    m->selected = false;
    return OZ_OK;
}

OZ_API int oz_mcts_set_roots(oz_mcts* m, const uint64_t* own, const uint64_t* opp, const uint8_t* active) {
    OZ_REQUIRE(m && own && opp, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    const int G = m->d.G;
    for (int i = 0; i < G; ++i)
        OZ_REQUIRE((own[i] & opp[i]) == 0 && ((own[i] | opp[i]) & ~m->d.valid) == 0, "root %d is not a valid %dx%d board", i, m->d.n, m->d.n);
    auto disarm_moved = [&](uint8_t* armed_dev) -> int {  // what was armed for one board: a slot that gets another one loses it
        std::vector<uint64_t> o(G), p(G);
        std::vector<uint8_t> armed(G);
        OZ_HIP(hipMemcpyAsync(o.data(), m->d.root_own, 8ull * G, hipMemcpyDeviceToHost, m->stream));
        OZ_HIP(hipMemcpyAsync(p.data(), m->d.root_opp, 8ull * G, hipMemcpyDeviceToHost, m->stream));
        OZ_HIP(hipMemcpyAsync(armed.data(), armed_dev, G, hipMemcpyDeviceToHost, m->stream));
        OZ_HIP(hipStreamSynchronize(m->stream));
        for (int i = 0; i < G; ++i)
            if (o[i] != own[i] || p[i] != opp[i]) armed[i] = 0;
        OZ_HIP(hipMemcpyAsync(armed_dev, armed.data(), G, hipMemcpyHostToDevice, m->stream));
        OZ_HIP(hipStreamSynchronize(m->stream));           // (`armed` is a local: the copy must be done before it goes)
        return OZ_OK;
    };
    if (m->noise_ever)                                     // root noise ...
        if (int rc = disarm_moved(m->d.noise_armed)) return rc;
    if (m->gumbel_ever)                                    // ... and the Gumbel draw with its snapshot of the root's counts
        if (int rc = disarm_moved(m->gd.armed)) return rc;
    OZ_HIP(hipMemcpyAsync(m->d.root_own, own, 8ull * G, hipMemcpyHostToDevice, m->stream));
    OZ_HIP(hipMemcpyAsync(m->d.root_opp, opp, 8ull * G, hipMemcpyHostToDevice, m->stream));
    if (active) OZ_HIP(hipMemcpyAsync(m->d.active, active, G, hipMemcpyHostToDevice, m->stream));
    else OZ_HIP(hipMemsetAsync(m->d.active, 1, G, m->stream));
    OZ_HIP(hipMemsetAsync(m->d.root_node, 0xFF, sizeof(int) * G, m->stream));       // new roots: look them up again
    OZ_HIP(hipStreamSynchronize(m->stream));
    m->selected = false;
    return OZ_OK;
}

OZ_API int oz_mcts_simulate(oz_mcts* m, oz_net* net, int nsims) {
    OZ_REQUIRE(m && net, "null argument");
    OZ_REQUIRE(net->n == m->d.n, "network board size %d != search board size %d", net->n, m->d.n);
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REQUIRE(net->max_batch >= m->d.G * m->leaves_per_step, "network max_batch %d < num_games %d x leaves_per_step %d", net->max_batch, m->d.G,
               m->leaves_per_step);
    if (m->wide() && m->selected) { oz_set_error("oz_mcts_simulate: a host-evaluated step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkn(net->mu);
    hipSetDevice(m->device);
    if (int rc = mcts_steps_async(m, net, nsims, m->d.G, false)) return rc;
    m->selected = false;
    return check_error_flag(m);
}

#define OZ_REFUSE_WIDE(m, fn) \
    do { if ((m)->leaves_per_step > 1) { oz_set_error(fn ": the host-evaluator split runs one leaf per game and step (leaves_per_step is %d: set it to 1)", (m)->leaves_per_step); return OZ_ERR_STATE; } } while (0)

// ---- solved leaves: the option
static int solve_leaves_check(const char* fn, int e) {
    OZ_REQUIRE(e >= 0 && e <= OZ_SOLVE_LEAVES_MAX_EMPTIES, "%s: max_empties %d outside 0 .. %d", fn, e, OZ_SOLVE_LEAVES_MAX_EMPTIES);
    return OZ_OK;
}
static int solve_leaves_set_locked(oz_mcts* m, int e) {
    if (e > 0 && !m->solve_rows) {
        hipSetDevice(m->device);
        const size_t held = m->allocs.size();
        int rc = m->alloc(&m->solve_claim, (size_t)m->d.G);
        if (!rc) rc = m->alloc(&m->solve_rows, 1);
        if (rc) {
            for (size_t i = held; i < m->allocs.size(); ++i) hipFree(m->allocs[i]);
            m->allocs.resize(held);
            m->solve_claim = nullptr; m->solve_rows = nullptr;
            return rc;
        }
        OZ_HIP(hipMemsetAsync(m->solve_claim, 0, sizeof(unsigned) * (size_t)m->d.G, m->stream));
        OZ_HIP(hipMemsetAsync(m->solve_rows, 0, sizeof(unsigned long long), m->stream));
    }
    m->solve_leaves = e;
    m->d.pf.E = e;                                         // (proofs: a leaf expanded with <= e empties carries its exact sign)
    return OZ_OK;
}
static int solve_leaves_rows_locked(oz_mcts* m, int64_t* rows) {
    unsigned long long r = 0;
    if (m->solve_rows) {
        hipSetDevice(m->device);
        OZ_HIP(hipMemcpyAsync(&r, m->solve_rows, sizeof r, hipMemcpyDeviceToHost, m->stream));
        OZ_HIP(hipStreamSynchronize(m->stream));
    }
    *rows = (int64_t)r;
    return OZ_OK;
}
OZ_API int oz_mcts_set_solve_leaves(oz_mcts* m, int max_empties) {
    OZ_REQUIRE(m, "null mcts");
    if (int rc = solve_leaves_check("oz_mcts_set_solve_leaves", max_empties)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    return solve_leaves_set_locked(m, max_empties);
}
OZ_API int oz_mcts_get_solve_leaves(oz_mcts* m, int* max_empties, int64_t* rows_solved) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    if (max_empties) *max_empties = m->solve_leaves;
    if (rows_solved) return solve_leaves_rows_locked(m, rows_solved);
    return OZ_OK;
}
// HIP-event timing of k_solve_leaves (tools/solve_leaves_bench.py); off, nothing is recorded
OZ_API int oz_mcts_solve_leaves_profile(oz_mcts* m, int enable) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    m->solve_profile = enable != 0;
    return OZ_OK;
}
OZ_API int oz_mcts_solve_leaves_profile_read(oz_mcts* m, double* ms_total, int64_t* launches, int reset) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    if (m->solve_timer.collect() != OZ_OK) { oz_set_error("HIP event timing failed"); return OZ_ERR_HIP; }
    if (ms_total) *ms_total = m->solve_timer.ms[0];
    if (launches) *launches = m->solve_timer.count[0];
    if (reset) m->solve_timer.reset();
    return OZ_OK;
}

// ---- value signs: the option (a tree holds values of one rule only, so the mode changes on an empty tree alone)
static_assert(OZ_VALUE_SIGNS_REFERENCE == OZ_VSIGNS_REFERENCE && OZ_VALUE_SIGNS_SOUND == OZ_VSIGNS_SOUND, "value signs: one numbering");
static int value_signs_check(const char* fn, int mode) {
    OZ_REQUIRE(mode == OZ_VALUE_SIGNS_REFERENCE || mode == OZ_VALUE_SIGNS_SOUND, "%s: unknown mode %d", fn, mode);
    return OZ_OK;
}
static int value_signs_set_locked(oz_mcts* m, const char* fn, int mode) {
    if (m->selected) { oz_set_error("%s: a step is pending (oz_mcts_select without oz_mcts_backup)", fn); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    std::vector<int> nodes((size_t)m->d.G);
    OZ_HIP(hipMemcpyAsync(nodes.data(), m->d.node_count, sizeof(int) * nodes.size(), hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    for (int n : nodes)
        if (n != 0) { oz_set_error("%s: the tree holds nodes already (set the mode right after create or after oz_mcts_reset(-1))", fn); return OZ_ERR_STATE; }
    if (m->proofs && mode != OZ_VSIGNS_SOUND) { oz_set_error("%s: proofs are on and need the sound signs (switch them off first)", fn); return OZ_ERR_STATE; }
    m->vsigns = mode;
    return OZ_OK;
}
OZ_API int oz_mcts_set_value_signs(oz_mcts* m, int mode) {
    OZ_REQUIRE(m, "null mcts");
    if (int rc = value_signs_check("oz_mcts_set_value_signs", mode)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    return value_signs_set_locked(m, "oz_mcts_set_value_signs", mode);
}
OZ_API int oz_mcts_get_value_signs(oz_mcts* m, int* mode) {
    OZ_REQUIRE(m && mode, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    *mode = m->vsigns;
    return OZ_OK;
}
// the definition on the host (oz_common.h), for tests and tools without a device
OZ_API int oz_search_backup_values(int mode, uint64_t swap_bits, int depth, double leaf_value, double* out, double* last_value) {
    if (int rc = value_signs_check("oz_search_backup_values", mode)) return rc;
    OZ_REQUIRE(depth >= 0 && depth <= OZ_MAX_DEPTH, "oz_search_backup_values: depth %d outside 0 .. %d", depth, OZ_MAX_DEPTH);
    OZ_REQUIRE(depth == 0 || out, "oz_search_backup_values: null argument");
    if (depth < 64) swap_bits &= (1ULL << depth) - 1ULL;
    for (int d = 0; d < depth; ++d) out[d] = oz_backup_value(mode, swap_bits, depth, d, leaf_value);
    if (last_value) *last_value = oz_backup_last(mode, swap_bits, depth, leaf_value);
    return OZ_OK;
}
OZ_API int oz_search_terminal_value(int mode, uint64_t own, uint64_t opp, int* value) {
    if (int rc = value_signs_check("oz_search_terminal_value", mode)) return rc;
    OZ_REQUIRE(value, "oz_search_terminal_value: null argument");
    *value = oz_terminal_value(mode, own, opp);
    return OZ_OK;
}

// ---- proofs: the option (include/othellozero_amd.h, "proofs").  Like the value signs it changes on an empty tree alone; it needs the sound
// signs (the reference's finished boards carry the wrong sign) and refuses the kernel families without a proven instantiation.
static_assert(OZ_PROOF_UNKNOWN == OZ_PROOF_NONE, "proofs: one numbering");
static int proofs_set_locked(oz_mcts* m, const char* fn, int enable) {
    if (m->selected) { oz_set_error("%s: a step is pending (oz_mcts_select without oz_mcts_backup)", fn); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    MctsDev& d = m->d;
    std::vector<int> nodes((size_t)d.G);
    OZ_HIP(hipMemcpyAsync(nodes.data(), d.node_count, sizeof(int) * nodes.size(), hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    for (int n : nodes)
        if (n != 0) { oz_set_error("%s: the tree holds nodes already (set the option right after create or after oz_mcts_reset(-1))", fn); return OZ_ERR_STATE; }
    if (!enable) { m->proofs = false; return OZ_OK; }
    if (m->vsigns != OZ_VSIGNS_SOUND) { oz_set_error("%s: proofs need value signs \"sound\" (a proof built on the reference's finished boards is wrong)", fn); return OZ_ERR_STATE; }
    if (m->gumbel_ever) { oz_set_error("%s: not with the Gumbel search (its kernels have no proven instantiation)", fn); return OZ_ERR_STATE; }
    if (d.forced_k > 0.0) { oz_set_error("%s: not with forced playouts (set k to 0 first)", fn); return OZ_ERR_STATE; }
    if (!d.pf.entry) {
        const size_t held = m->allocs.size();
        int rc = m->alloc(&d.pf.entry, (size_t)d.G * d.node_cap);
        if (!rc) rc = m->alloc(&d.pf.stat, (size_t)d.G * OZ_NPSTAT);
        if (!rc && (hipMemsetAsync(d.pf.stat, 0, sizeof(unsigned long long) * OZ_NPSTAT * (size_t)d.G, m->stream) != hipSuccess ||
                    hipStreamSynchronize(m->stream) != hipSuccess)) {
            oz_set_error("%s: clearing the counters failed", fn);
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < m->allocs.size(); ++i) hipFree(m->allocs[i]);
            m->allocs.resize(held);
            d.pf.entry = nullptr; d.pf.stat = nullptr;
            return rc;
        }
    }
    d.pf.E = m->solve_leaves;
    m->proofs = true;
    return OZ_OK;
}
OZ_API int oz_mcts_set_proofs(oz_mcts* m, int enable) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    return proofs_set_locked(m, "oz_mcts_set_proofs", enable);
}
OZ_API int oz_mcts_get_proofs(oz_mcts* m, int* enabled) {
    OZ_REQUIRE(m && enabled, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    *enabled = m->proofs ? 1 : 0;
    return OZ_OK;
}
// ---- selection: the option (include/othellozero_amd.h, "selection").  Every node of such a tree keeps vhat in header word 3, so like the value
// signs it changes on an empty tree alone; it refuses the kernel families without a selection instantiation and forced playouts.
static_assert(OZ_SELECT_FPU == OZ_SEL_FPU && OZ_SELECT_GROWTH == OZ_SEL_GROWTH && OZ_SELECT_PRIOR_FIRST == OZ_SEL_PRIOR_FIRST, "selection: one numbering");
static int selection_check(const char* fn, int flags, double fpu, double fpu_root, double base, double factor) {
    OZ_REQUIRE((flags & ~(OZ_SEL_FPU | OZ_SEL_GROWTH | OZ_SEL_PRIOR_FIRST)) == 0, "%s: unknown flag bits %d", fn, flags);
    if (flags & OZ_SEL_FPU) {                                                                                  // (NaN fails both compares)
        OZ_REQUIRE(fpu >= 0.0 && fpu <= 4.0, "%s: fpu_reduction %g outside [0, 4]", fn, fpu);
        OZ_REQUIRE(fpu_root >= 0.0 && fpu_root <= 4.0, "%s: fpu_root_reduction %g outside [0, 4]", fn, fpu_root);
    }
    if (flags & OZ_SEL_GROWTH) {
        OZ_REQUIRE(base > 0.0 && base < INFINITY, "%s: cpuct_base %g must be positive and finite", fn, base);
        OZ_REQUIRE(factor >= 0.0 && factor < INFINITY, "%s: cpuct_factor %g must be >= 0 and finite", fn, factor);
    }
    return OZ_OK;
}
// a part that is off keeps no parameters: what the getter reports is what the kernels read
static OzSelection selection_of(int flags, double fpu, double fpu_root, double base, double factor) {
    OzSelection s{flags, 0.0, 0.0, 0.0, 0.0};
    if (flags & OZ_SEL_FPU) { s.fpu = fpu; s.fpu_root = fpu_root; }
    if (flags & OZ_SEL_GROWTH) { s.base = base; s.factor = factor; }
    return s;
}
static int selection_set_locked(oz_mcts* m, const char* fn, const OzSelection& sel) {
    if (m->selected) { oz_set_error("%s: a step is pending (oz_mcts_select without oz_mcts_backup)", fn); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    MctsDev& d = m->d;
    std::vector<int> nodes((size_t)d.G);
    OZ_HIP(hipMemcpyAsync(nodes.data(), d.node_count, sizeof(int) * nodes.size(), hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    for (int n : nodes)
        if (n != 0) { oz_set_error("%s: the tree holds nodes already (set the option right after create or after oz_mcts_reset(-1))", fn); return OZ_ERR_STATE; }
    if (sel.flags) {
        if (m->gumbel_ever) { oz_set_error("%s: not with the Gumbel search (its kernels have no selection instantiation)", fn); return OZ_ERR_STATE; }
        if (d.forced_k > 0.0) { oz_set_error("%s: not with forced playouts (their quota and pruning restate PUCT with the constant c; set k to 0 first)", fn); return OZ_ERR_STATE; }
    }
    d.sel = sel;
    return OZ_OK;
}
OZ_API int oz_mcts_set_selection(oz_mcts* m, int flags, double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor) {
    OZ_REQUIRE(m, "null mcts");
    if (int rc = selection_check("oz_mcts_set_selection", flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    return selection_set_locked(m, "oz_mcts_set_selection", selection_of(flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor));
}
OZ_API int oz_mcts_get_selection(oz_mcts* m, int* flags, double* fpu_reduction, double* fpu_root_reduction, double* cpuct_base, double* cpuct_factor) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    const OzSelection& s = m->d.sel;
    if (flags) *flags = s.flags;
    if (fpu_reduction) *fpu_reduction = s.fpu;
    if (fpu_root_reduction) *fpu_root_reduction = s.fpu_root;
    if (cpuct_base) *cpuct_base = s.base;
    if (cpuct_factor) *cpuct_factor = s.factor;
    return OZ_OK;
}
// the definition on the host (oz_common.h), for tests and tools without a device
OZ_API int oz_search_select_c(double c, double base, double factor, int n, double* out) {
    OZ_REQUIRE(out, "oz_search_select_c: null argument");
    if (int rc = selection_check("oz_search_select_c", OZ_SEL_GROWTH, 0.0, 0.0, base, factor)) return rc;
    OZ_REQUIRE(n >= 0, "oz_search_select_c: n %d", n);
    *out = oz_select_c(c, base, factor, n);
    return OZ_OK;
}
OZ_API int oz_search_select_scores(const int32_t* N, const double* Q, const double* P, uint64_t legal, int Ns, double vhat, int level, double c, int flags,
                                   double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor, double* U, double* F,
                                   double* V, double* c_S, int32_t* pick) {
    OZ_REQUIRE(N && Q && P && U, "oz_search_select_scores: null argument");
    if (int rc = selection_check("oz_search_select_scores", flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor)) return rc;
    OZ_REQUIRE(Ns >= 0 && level >= 0, "oz_search_select_scores: Ns %d, level %d", Ns, level);
    for (int sq = 0; sq < 64; ++sq) OZ_REQUIRE(!((legal >> sq) & 1) || N[sq] >= 0, "oz_search_select_scores: N[%d] = %d", sq, N[sq]);
    const OzSelection s = selection_of(flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor);
    const double cS = (s.flags & OZ_SEL_GROWTH) ? oz_select_c(c, s.base, s.factor, Ns) : c;
    const double r = oz_select_r(s.flags & OZ_SEL_PRIOR_FIRST, Ns);
    double f = 0.0, v = 0.0;
    if (s.flags & OZ_SEL_FPU) {
        double aq[64], ap[64];
        int SN = 0;
        for (int sq = 0; sq < 64; ++sq) {
            const bool vis = ((legal >> sq) & 1) && N[sq] > 0;
            if ((legal >> sq) & 1) SN += N[sq];
            aq[sq] = vis ? oz_select_fpu_q(N[sq], Q[sq]) : 0.0;
            ap[sq] = vis ? P[sq] : 0.0;
        }
        f = oz_select_fpu(vhat, oz_tree_sum64(aq), oz_tree_sum64(ap), SN, level == 0 ? s.fpu_root : s.fpu, &v);
    }
    int best = -1;
    for (int sq = 0; sq < 64; ++sq) {
        U[sq] = -INFINITY;
        if (!((legal >> sq) & 1)) continue;
        const double q = (s.flags & OZ_SEL_FPU) && N[sq] == 0 ? f : Q[sq];
        U[sq] = oz_select_u(q, cS, P[sq], r, N[sq]);
        if (best < 0 || U[sq] > U[best]) best = sq;                        // the first maximum
    }
    if (F) *F = f;
    if (V) *V = v;
    if (c_S) *c_S = cS;
    if (pick) *pick = best;
    return OZ_OK;
}
static int proof_stats_locked(oz_mcts* m, int64_t* out4) {
    for (int k = 0; k < OZ_NPSTAT; ++k) out4[k] = 0;
    if (!m->d.pf.stat) return OZ_OK;
    const size_t cnt = (size_t)m->d.G * OZ_NPSTAT;
    std::vector<unsigned long long> h(cnt);
    hipSetDevice(m->device);
    OZ_HIP(hipMemcpyAsync(h.data(), m->d.pf.stat, 8 * cnt, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    for (size_t i = 0; i < cnt; ++i) out4[i % OZ_NPSTAT] += (int64_t)h[i];
    return OZ_OK;
}
OZ_API int oz_mcts_proof_stats(oz_mcts* m, int64_t* out4) {
    OZ_REQUIRE(m && out4, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    return proof_stats_locked(m, out4);
}
// the proof entry of node `index` of game `game` (indices as oz_mcts_dump_node) on the host; false: the object keeps none
static int proof_entry_locked(oz_mcts* m, int game, int index, OzProof* p) {
    MctsDev& d = m->d;
    OZ_REQUIRE(game >= 0 && game < d.G, "game index out of range");
    hipSetDevice(m->device);
    OZ_HIP(hipStreamSynchronize(m->stream));
    int nn = 0;
    OZ_HIP(hipMemcpy(&nn, d.node_count + game, 4, hipMemcpyDeviceToHost));
    OZ_REQUIRE(index >= 0 && index < nn, "node index %d out of range (%d nodes)", index, nn);
    OZ_HIP(hipMemcpy(p, d.pf.entry + (size_t)game * d.node_cap + index, sizeof(OzProof), hipMemcpyDeviceToHost));
    return OZ_OK;
}
static void proof_edges(const OzProof& p, int8_t* edge) {
    for (int s = 0; s < 64; ++s) edge[s] = (int8_t)(((p.legal >> s) & 1) ? oz_proof_edge(p.lo, p.hi, s) : OZ_PROOF_NONE);
}
OZ_API int oz_mcts_dump_proofs(oz_mcts* m, int game, int index, int8_t* edge, int8_t* node_value, int8_t* node_val) {
    OZ_REQUIRE(m && edge && node_value && node_val, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->proofs) { oz_set_error("oz_mcts_dump_proofs: the object keeps no proofs (oz_mcts_set_proofs)"); return OZ_ERR_STATE; }
    OzProof p;
    if (int rc = proof_entry_locked(m, game, index, &p)) return rc;
    proof_edges(p, edge);
    *node_value = (int8_t)p.own;
    *node_val = (int8_t)oz_proof_value(p.legal, p.lo, p.hi, p.own);
    return OZ_OK;
}
// the proofs of the current roots: rc[g] = 0, or 1 where game g is idle or its root is not in the table (edge / val are then unknown)
OZ_API int oz_mcts_root_proofs(oz_mcts* m, int8_t* edge, int8_t* val, int32_t* rc) {
    OZ_REQUIRE(m && edge && val && rc, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->proofs) { oz_set_error("oz_mcts_root_proofs: the object keeps no proofs (oz_mcts_set_proofs)"); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    MctsDev& d = m->d;
    const int G = d.G;
    std::vector<uint64_t> o(G), q(G);
    std::vector<uint8_t> act(G);
    std::vector<int> nn(G);
    OZ_HIP(hipMemcpyAsync(o.data(), d.root_own, 8ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(q.data(), d.root_opp, 8ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(act.data(), d.active, G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(nn.data(), d.node_count, 4ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    std::vector<uint64_t> keys;
    std::vector<OzProof> pr;
    for (int g = 0; g < G; ++g) {
        for (int s = 0; s < 64; ++s) edge[(size_t)g * 64 + s] = OZ_PROOF_NONE;
        val[g] = OZ_PROOF_NONE; rc[g] = 1;
        if (!act[g] || nn[g] <= 0) continue;
        // (the host has no view of the hash table: the node headers are searched -- a call per move on small trees, for tests and tools)
        keys.resize((size_t)nn[g] * 2);
        OZ_HIP(hipMemcpy2D(keys.data(), 16, d.recs + (size_t)g * d.node_cap * (size_t)d.rec_bytes, (size_t)d.rec_bytes, 16, (size_t)nn[g], hipMemcpyDeviceToHost));
        for (int i = 0; i < nn[g]; ++i)
            if (keys[2 * (size_t)i] == o[g] && keys[2 * (size_t)i + 1] == q[g]) {
                OzProof p;
                OZ_HIP(hipMemcpy(&p, d.pf.entry + (size_t)g * d.node_cap + i, sizeof(OzProof), hipMemcpyDeviceToHost));
                proof_edges(p, edge + (size_t)g * 64);
                val[g] = (int8_t)oz_proof_value(p.legal, p.lo, p.hi, p.own);
                rc[g] = 0;
                break;
            }
    }
    return OZ_OK;
}
// the rule on the host (oz_common.h), for tests and tools without a device.  Values are -1 / 0 / +1 or OZ_PROOF_UNKNOWN.
static bool proof_is_value(int v) { return v == OZ_PROOF_NONE || (v >= -1 && v <= 1); }
OZ_API int oz_search_proof_value(uint64_t legal, uint64_t lo, uint64_t hi, int own_value, int* value) {
    OZ_REQUIRE(value, "oz_search_proof_value: null argument");
    OZ_REQUIRE(proof_is_value(own_value), "oz_search_proof_value: own_value %d", own_value);
    *value = oz_proof_value(legal, lo, hi, own_value);
    return OZ_OK;
}
OZ_API int oz_search_proof_candidates(uint64_t legal, uint64_t lo, uint64_t hi, int node_val, uint64_t* candidates, int* inconsistent) {
    OZ_REQUIRE(candidates && inconsistent, "oz_search_proof_candidates: null argument");
    OZ_REQUIRE(proof_is_value(node_val), "oz_search_proof_candidates: node_val %d", node_val);
    *candidates = oz_proof_candidates(legal, lo, hi, node_val, inconsistent);
    return OZ_OK;
}
// the proof loop over a path: level d's node has (legal[d], lo[d], hi[d], own_value[d]) and the descent took its square[d] with swap bit
// sigma[d]; lo / hi are updated in place.  out3 = levels marked, edges newly proven, 1 where the root's value became known;
// *conflict = 1 where a known edge differed.
OZ_API int oz_search_proof_backup(const uint8_t* sigma, const int32_t* square, int depth, int leaf_value, const uint64_t* legal, uint64_t* lo, uint64_t* hi,
                                  const int8_t* own_value, int32_t* out3, int* conflict) {
    OZ_REQUIRE(depth >= 0 && depth <= OZ_MAX_DEPTH, "oz_search_proof_backup: depth %d outside 0 .. %d", depth, OZ_MAX_DEPTH);
    OZ_REQUIRE(leaf_value >= -1 && leaf_value <= 1, "oz_search_proof_backup: leaf_value %d", leaf_value);
    OZ_REQUIRE(out3 && conflict && (depth == 0 || (sigma && square && legal && lo && hi && own_value)), "oz_search_proof_backup: null argument");
    OzProof pr[OZ_MAX_DEPTH];
    OzProof* pp[OZ_MAX_DEPTH];
    int sq[OZ_MAX_DEPTH];
    for (int d = 0; d < depth; ++d) {
        OZ_REQUIRE(square[d] >= 0 && square[d] < 64 && ((legal[d] >> square[d]) & 1), "oz_search_proof_backup: square[%d] = %d is not legal", d, square[d]);
        OZ_REQUIRE(proof_is_value(own_value[d]), "oz_search_proof_backup: own_value[%d] = %d", d, own_value[d]);
        pr[d] = OzProof{lo[d], hi[d], legal[d], own_value[d], 0};
        pp[d] = &pr[d]; sq[d] = square[d];
    }
    int fresh = 0, root = 0;
    out3[0] = oz_proof_backup(pp, sq, sigma, depth, leaf_value, &fresh, conflict, &root);
    out3[1] = fresh; out3[2] = root;
    for (int d = 0; d < depth; ++d) { lo[d] = pr[d].lo; hi[d] = pr[d].hi; }
    return OZ_OK;
}

#define OZ_REFUSE_SOLVED(m, fn) \
    do { if ((m)->solve_leaves > 0) { oz_set_error(fn ": the host-evaluator split takes the caller's (pi, v) as they are (solve_leaves is %d: set it to 0)", (m)->solve_leaves); return OZ_ERR_STATE; } } while (0)

OZ_API int oz_mcts_set_leaves_per_step(oz_mcts* m, int k) {
    OZ_REQUIRE(m, "null mcts");
    if (int rc = wide_check_k(k)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->selected) { oz_set_error("oz_mcts_set_leaves_per_step: a step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    return wide_set_k(m, k);
}
OZ_API int oz_mcts_get_leaves_per_step(oz_mcts* m, int* k) {
    OZ_REQUIRE(m && k, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    *k = m->leaves_per_step;
    return OZ_OK;
}
// diagnostic: leaves_per_step = 1 through the wide kernels (the reference's fixtures then hold the wide kernels)
OZ_API int oz_mcts_use_wide_kernels(oz_mcts* m, int enable) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->selected) { oz_set_error("oz_mcts_use_wide_kernels: a step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    if (enable && m->gumbel_ever) { oz_set_error("oz_mcts_use_wide_kernels: the Gumbel search runs on the one-descent kernels"); return OZ_ERR_STATE; }
    if (enable) if (int rc = wide_alloc(m)) return rc;
    m->use_wide = enable != 0;
    return OZ_OK;
}
static int wide_stats_locked(oz_mcts* m, int64_t* out3) {
    out3[0] = out3[1] = out3[2] = 0;
    if (!m->w.status) return OZ_OK;
    const size_t cnt = (size_t)m->d.G * 3;
    std::vector<unsigned long long> h(cnt);
    OZ_HIP(hipMemcpyAsync(h.data(), m->w.stat, 8 * cnt, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    for (size_t i = 0; i < cnt; ++i) out3[i % 3] += (int64_t)h[i];
    return OZ_OK;
}
OZ_API int oz_mcts_wide_stats(oz_mcts* m, int64_t* out3) {
    OZ_REQUIRE(m && out3, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    return wide_stats_locked(m, out3);
}

// ---- root noise: host side
static int noise_check(const char* fn, double alpha, double eps, bool with_alpha) {
    OZ_REQUIRE(!with_alpha || (alpha >= 0.01 && alpha <= 100.0), "%s: alpha %g outside [0.01, 100]", fn, alpha);       // (NaN fails both compares)
    OZ_REQUIRE(eps >= 0.0 && eps <= 1.0, "%s: eps %g outside [0, 1]", fn, eps);
    return OZ_OK;
}
// eta and the armed flags, at the first arming: 513 B per game
static int noise_alloc(oz_mcts* m) {
    if (m->noise_ever) return OZ_OK;
    MctsDev& d = m->d;
    const size_t held = m->allocs.size();
    double* eta = nullptr; uint8_t* armed = nullptr;
    int rc = m->alloc(&eta, (size_t)d.G * 64);
    if (!rc) rc = m->alloc(&armed, (size_t)d.G);
    if (!rc && (hipMemsetAsync(eta, 0, sizeof(double) * 64 * (size_t)d.G, m->stream) != hipSuccess ||
                hipMemsetAsync(armed, 0, (size_t)d.G, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)) {
        oz_set_error("root noise: clearing the buffers failed");
        rc = OZ_ERR_HIP;
    }
    if (rc) {
        for (size_t i = held; i < m->allocs.size(); ++i) hipFree(m->allocs[i]);
        m->allocs.resize(held);
        return rc;
    }
    d.noise_eta = eta; d.noise_armed = armed;
    m->noise_ever = true;
    return OZ_OK;
}
// every slot disarmed, nothing allocated
static int noise_disarm(oz_mcts* m) {
    m->d.noise_eps = 0.0;
    if (m->noise_ever) {
        OZ_HIP(hipMemsetAsync(m->d.noise_armed, 0, (size_t)m->d.G, m->stream));
        OZ_HIP(hipStreamSynchronize(m->stream));
    }
    return OZ_OK;
}
#define OZ_REFUSE_GUMBEL(m, fn, what) \
    do { if ((m)->gumbel_ever) { oz_set_error("%s: the Gumbel search replaces " what " (the object has it switched on)", fn); return OZ_ERR_STATE; } } while (0)
#define OZ_REFUSE_PENDING(m, fn) \
    do { if ((m)->selected) { oz_set_error(fn ": a step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; } } while (0)

OZ_API int oz_mcts_set_root_noise(oz_mcts* m, double eps, const double* eta, const uint8_t* armed) {
    OZ_REQUIRE(m, "null mcts");
    if (int rc = noise_check("oz_mcts_set_root_noise", 1.0, eps, false)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_PENDING(m, "oz_mcts_set_root_noise");
    if (eta && eps != 0.0) OZ_REFUSE_GUMBEL(m, "oz_mcts_set_root_noise", "root noise");
    hipSetDevice(m->device);
    if (!eta || eps == 0.0) return noise_disarm(m);
    const int G = m->d.G;
    for (size_t i = 0; i < (size_t)G * 64; ++i) OZ_REQUIRE(eta[i] >= 0.0 && eta[i] <= 1.0, "oz_mcts_set_root_noise: eta[%zu][%zu] = %g outside [0, 1]", i / 64, i % 64, eta[i]);
    if (int rc = noise_alloc(m)) return rc;
    OZ_HIP(hipMemcpyAsync(m->d.noise_eta, eta, sizeof(double) * 64 * (size_t)G, hipMemcpyHostToDevice, m->stream));
    std::vector<uint8_t> a;
    if (armed) {
        a.resize(G);
        for (int i = 0; i < G; ++i) a[i] = armed[i] ? 1 : 0;
        OZ_HIP(hipMemcpyAsync(m->d.noise_armed, a.data(), G, hipMemcpyHostToDevice, m->stream));
    } else hipLaunchKernelGGL(k_noise_arm_active, dim3((G + 255) / 256), dim3(256), 0, m->stream, m->d);
    OZ_HIP(hipGetLastError());
    OZ_HIP(hipStreamSynchronize(m->stream));
    m->d.noise_eps = eps;
    return OZ_OK;
}
// the (game id, ply) keys of oz_mcts_sample_root_noise / oz_mcts_sample_moves, on the device (allocated at the first use)
static int stage_keys(oz_mcts* m, const uint64_t* game_ids, const int32_t* plies) {
    const int G = m->d.G;
    if (!m->noise_ids) {
        if (int rc = m->alloc(&m->noise_ids, (size_t)G)) return rc;
        if (int rc = m->alloc(&m->noise_plies, (size_t)G)) return rc;
    }
    OZ_HIP(hipMemcpyAsync(m->noise_ids, game_ids, 8ull * G, hipMemcpyHostToDevice, m->stream));
    OZ_HIP(hipMemcpyAsync(m->noise_plies, plies, 4ull * G, hipMemcpyHostToDevice, m->stream));
    return OZ_OK;
}
OZ_API int oz_mcts_sample_root_noise(oz_mcts* m, double alpha, double eps, uint64_t seed, const uint64_t* game_ids, const int32_t* plies) {
    OZ_REQUIRE(m && game_ids && plies, "null argument");
    if (int rc = noise_check("oz_mcts_sample_root_noise", alpha, eps, true)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_PENDING(m, "oz_mcts_sample_root_noise");
    if (eps != 0.0) OZ_REFUSE_GUMBEL(m, "oz_mcts_sample_root_noise", "root noise");
    hipSetDevice(m->device);
    if (eps == 0.0) return noise_disarm(m);
    const int G = m->d.G;
    for (int i = 0; i < G; ++i) OZ_REQUIRE(plies[i] >= 0, "oz_mcts_sample_root_noise: plies[%d] = %d", i, plies[i]);
    if (int rc = noise_alloc(m)) return rc;
    if (int rc = stage_keys(m, game_ids, plies)) return rc;
    hipLaunchKernelGGL(k_root_noise, dim3(G), dim3(64), 0, m->stream, m->d, alpha, seed, (const uint64_t*)m->noise_ids, (const int*)m->noise_plies);
    OZ_HIP(hipGetLastError());
    OZ_HIP(hipStreamSynchronize(m->stream));
    m->d.noise_eps = eps;
    return OZ_OK;
}
static int noise_read_locked(oz_mcts* m, double* eta, uint8_t* armed) {
    const int G = m->d.G;
    if (!m->noise_ever) {
        if (eta) memset(eta, 0, sizeof(double) * 64 * (size_t)G);
        if (armed) memset(armed, 0, (size_t)G);
        return OZ_OK;
    }
    if (eta) OZ_HIP(hipMemcpyAsync(eta, m->d.noise_eta, sizeof(double) * 64 * (size_t)G, hipMemcpyDeviceToHost, m->stream));
    if (armed) OZ_HIP(hipMemcpyAsync(armed, m->d.noise_armed, (size_t)G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
OZ_API int oz_mcts_get_root_noise(oz_mcts* m, double* eta, uint8_t* armed, double* eps) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    if (eps) *eps = m->d.noise_eps;
    return noise_read_locked(m, eta, armed);
}

OZ_API int oz_mcts_select(oz_mcts* m) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_WIDE(m, "oz_mcts_select");
    OZ_REFUSE_SOLVED(m, "oz_mcts_select");
    TreeKernels tk;
    if (int rc = tree_kernels(m, &tk)) return rc;
    hipSetDevice(m->device);
    hipLaunchKernelGGL(tk.select, dim3(m->d.G), dim3(64), 0, m->stream, m->d, m->gd);
    OZ_HIP(hipGetLastError());
    m->selected = true;
    return check_error_flag(m);
}

OZ_API int oz_mcts_leaves(oz_mcts* m, int32_t* status, uint64_t* own, uint64_t* opp) {
    OZ_REQUIRE(m && status && own && opp, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_WIDE(m, "oz_mcts_leaves");
    OZ_REQUIRE(m->selected, "oz_mcts_leaves: call oz_mcts_select first");
    hipSetDevice(m->device);
    const int G = m->d.G;
    OZ_HIP(hipMemcpyAsync(status, m->d.leaf_status, 4ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(own, m->d.leaf_own, 8ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(opp, m->d.leaf_opp, 8ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}

OZ_API int oz_mcts_backup(oz_mcts* m, const float* pi, const float* v) {
    OZ_REQUIRE(m && pi && v, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_WIDE(m, "oz_mcts_backup");
    OZ_REFUSE_SOLVED(m, "oz_mcts_backup");
    if (!m->selected) { oz_set_error("oz_mcts_backup: call oz_mcts_select first"); return OZ_ERR_STATE; }
    TreeKernels tk;
    if (int rc = tree_kernels(m, &tk)) return rc;
    hipSetDevice(m->device);
    const int G = m->d.G;
    OZ_HIP(hipMemcpyAsync(m->d.pi, pi, 4ull * G * m->d.n2, hipMemcpyHostToDevice, m->stream));
    OZ_HIP(hipMemcpyAsync(m->d.v, v, 4ull * G, hipMemcpyHostToDevice, m->stream));
    hipLaunchKernelGGL(tk.expand_backup, dim3(G), dim3(64), 0, m->stream, m->d, 1);
    OZ_HIP(hipGetLastError());
    m->selected = false;
    return check_error_flag(m);
}

OZ_API int oz_mcts_last_value(oz_mcts* m, double* value, int32_t* vtype, int32_t* depth) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    const int G = m->d.G;
    if (value) OZ_HIP(hipMemcpyAsync(value, m->d.last_value, 8ull * G, hipMemcpyDeviceToHost, m->stream));
    if (vtype) OZ_HIP(hipMemcpyAsync(vtype, m->d.last_vtype, 4ull * G, hipMemcpyDeviceToHost, m->stream));
    if (depth) OZ_HIP(hipMemcpyAsync(depth, m->d.depth, 4ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}

// ---------------------------------------------------------------- root read-outs: what the search knows of the root of every slot
// record index of the root of slot g (cached by the descent, else looked up); -1 = not in the table
__device__ __forceinline__ int root_lookup(const MctsDev& t, int g, uint64_t own, uint64_t opp, int lane) {
    int node = unii(t.root_node[g]);
    if (node < 0) { int fs; node = ht_find(t, g, own, opp, lane, &fs); }
    return node;
}
// the root's row, N(state, action) of MCTS/__init__.py:73-84,172-175: one wave per slot, lane = square.  rc (wave-uniform): 0; 1 = the root is not
// in the table; 2 = it is and was never selected from (_Nsa[hash] still empty -> KeyError in the reference).  cnt = this lane's raw count and,
// with Q, q = its stored Q: 0 off the legal set and where rc != 0
struct RootRow { uint64_t legal; int node, rc, cnt; double q; };
template <bool Q = false>
__device__ __forceinline__ RootRow root_row(const MctsDev& t, int g, int lane) {
    const uint64_t own = uni64(t.root_own[g]), opp = uni64(t.root_opp[g]);
    RootRow r{oz_legal(own, opp, t.valid), root_lookup(t, g, own, opp, lane), 0, 0, 0.0};
    if (r.node < 0) r.rc = 1;
    else if (*rec_Ns(t, g, r.node) == 0) r.rc = 2;
    else if ((r.legal >> lane) & 1) {
        const OzEdge* e = lane_edge(t, g, r.node, r.legal, lane);
        r.cnt = (int)(e->n_tag & ~OZ_TAG_F32);
        if constexpr (Q) r.q = e->q;
    }
    r.rc = unii(r.rc);
    return r;
}
// proof play of the root record `node` ("proof play" in the header): its proof entry -- one 32-byte wave-uniform load -- and what oz_proof_play
// (oz_common.h) keeps of the raw counts cnt.  The rule's row is cnt on the squares of `keep` and 0 elsewhere; every member is wave-uniform
struct ProofRow { uint64_t keep; int val, fall; };
__device__ __forceinline__ ProofRow proof_row(const MctsDev& t, int g, int node, int cnt) {
    const OzProof* pe = t.pf.entry + (size_t)g * t.node_cap + node;
    ProofRow p;
    int bad;
    p.val = oz_proof_play(uni64(pe->legal), uni64(pe->lo), uni64(pe->hi), unii(pe->own), __ballot(cnt > 0), &p.keep, &p.fall, &bad);
    return p;
}
// the root value of a search ("value targets" in the header): the visit-weighted mean of the stored Q over the raw counts.  terms = 64 doubles
// of LDS: terms[lane] = oz_root_term of the lane's edge, the wave sums N, oz_root_mean divides (rc 2: no visit at all)
struct RootValue { double v; int rc; };
__device__ __forceinline__ RootValue root_value(double* terms, int cnt, double q, int lane) {
    terms[lane] = oz_root_term(cnt, q);
    const int total = wave_sum_i32(cnt);
    wave_sync();
    RootValue r;
    r.v = oz_root_mean(terms, (long long)total, &r.rc);
    return r;
}
// ---- the read-out kernel of the bare search: one template, instantiated per entry.  R is a mask of RO_* flags: which row, and what is written
// into the staging (ReadArgs).  Neither RO_VALUE nor RO_SAMPLE: the [G][64] row, the legal sets and rc.
//   flag          what it does                                                                                    entries (oz_mcts_*)
//   (none)        the raw row                                                                                     root_counts
//   RO_PRUNED     the policy target's row: pruned where the slot's noise is armed (and k > 0), raw elsewhere      pruned_counts
//   RO_PROVEN     the rule's row: the raw count on the squares proof play keeps, 0 elsewhere                      proven_counts
//   RO_VALUE      writes the root value of the RAW row; with RO_PROVEN the exact one where the proofs know it     root_values, proven_root_values
//   RO_SAMPLE     writes the move sampled from the row and its maximum (the engine's sample_move, the same        sample_moves, proven_sample_moves
//                 keys); -1 where rc != 0 and on an idle slot
enum : unsigned { RO_PRUNED = 1, RO_PROVEN = 2, RO_VALUE = 4, RO_SAMPLE = 8 };
// the staging by what lies there: row = [G][64] counts (RO_SAMPLE: [G] actions), word = [G] 8-byte words (legal sets; RO_VALUE: the values'
// bits), code = [G] rc.  The keys are the samplers' alone.
struct ReadArgs {
    int32_t* row; uint64_t* word; int32_t* code;
    double temperature; uint64_t seed; const uint64_t* game_ids; const int* plies;
};
template <unsigned R>
__global__ __launch_bounds__(64) void k_root_read(MctsDev t, ReadArgs a) {
    static_assert(R < 16 && !(has(R, RO_PRUNED) && R != RO_PRUNED) && !(has(R, RO_VALUE) && has(R, RO_SAMPLE)), "no entry reads this out");
    const int g = blockIdx.x, lane = threadIdx.x;
    const RootRow r = root_row<has(R, RO_VALUE)>(t, g, lane);
    int cnt = r.cnt, pval = OZ_PROOF_NONE;
    if constexpr (has(R, RO_PROVEN)) {
        if (r.rc == 0) {
            const ProofRow p = proof_row(t, g, r.node, cnt);
            pval = p.val;
            if (!has(R, RO_VALUE) && !((p.keep >> lane) & 1)) cnt = 0;
        }
    }
    if constexpr (has(R, RO_PRUNED)) {
        if (r.rc == 0 && t.forced_k > 0.0 && t.noise_eps > 0.0 && t.noise_armed && unii((int)t.noise_armed[g]) != 0)
            cnt = forced_prune_lane(t, g, r.node, lane, r.legal, cnt, unii(wave_max_i32(cnt)), t.forced_k);
    }
    if constexpr (has(R, RO_VALUE)) {
        __shared__ double terms[64];
        RootValue v = root_value(terms, cnt, r.q, lane);
        if (pval != OZ_PROOF_NONE) v = RootValue{(double)pval, 0};
        if (lane == 0) { a.word[g] = (uint64_t)__double_as_longlong(r.rc == 0 ? v.v : 0.0); a.code[g] = r.rc == 0 ? v.rc : r.rc; }
    } else if constexpr (has(R, RO_SAMPLE)) {
        const int mx = unii(wave_max_i32(cnt));
        int action = -1;
        if (r.rc == 0 && mx >= 1 && t.active[g])
            action = sample_move(cnt, r.legal, mx, a.temperature, oz_rng_unit(oz_rng(a.seed, uni64(a.game_ids[g]), (uint64_t)unii(a.plies[g]), OZ_RNG_SAMPLE)), lane);
        if (lane == 0) { a.row[g] = action; a.code[g] = r.rc; }
    } else {
        a.row[(size_t)g * 64 + lane] = cnt;
        if (lane == 0) { a.word[g] = r.legal; a.code[g] = r.rc; }
    }
}
static int sample_check(const char* fn, double temperature) {
    OZ_REQUIRE(temperature >= 0.01 && temperature <= 100.0, "%s: temperature %g outside [0.01, 100]", fn, temperature);     // (NaN fails both compares)
    return OZ_OK;
}
// one read-out, from the lock to the synchronised copies: `out` = the rows, the values or the actions (what k_root_read<R> writes), legal =
// the rows' legal sets.  The samplers bring their keys; RO_PROVEN needs an object that keeps proofs, the raw sampler one without the Gumbel search.
struct ReadKeys { double temperature; uint64_t seed; const uint64_t* game_ids; const int32_t* plies; };
template <unsigned R>
static int root_read(oz_mcts* m, const char* fn, void* out, uint64_t* legal, int32_t* rc, ReadKeys k = ReadKeys{}) {
    constexpr bool rows = !has(R, RO_VALUE | RO_SAMPLE);
    std::lock_guard<std::mutex> lk(m->mu);
    if (has(R, RO_PROVEN) && !m->proofs) { oz_set_error("%s: the object keeps no proofs (oz_mcts_set_proofs)", fn); return OZ_ERR_STATE; }
    if (R == RO_SAMPLE) OZ_REFUSE_GUMBEL(m, fn, "move sampling");
    hipSetDevice(m->device);
    const int G = m->d.G;
    ReadArgs a{m->rc_counts, m->rc_legal, m->rc_rc, k.temperature, k.seed, nullptr, nullptr};
    if (has(R, RO_SAMPLE)) {
        for (int i = 0; i < G; ++i) OZ_REQUIRE(k.plies[i] >= 0, "%s: plies[%d] = %d", fn, i, k.plies[i]);
        if (int r = stage_keys(m, k.game_ids, k.plies)) return r;
        a.game_ids = (const uint64_t*)m->noise_ids; a.plies = (const int*)m->noise_plies;
    }
    hipLaunchKernelGGL(k_root_read<R>, dim3(G), dim3(64), 0, m->stream, m->d, a);
    OZ_HIP(hipGetLastError());
    if (has(R, RO_VALUE)) OZ_HIP(hipMemcpyAsync(out, a.word, 8ull * G, hipMemcpyDeviceToHost, m->stream));
    else OZ_HIP(hipMemcpyAsync(out, a.row, 4ull * G * (rows ? 64 : 1), hipMemcpyDeviceToHost, m->stream));
    if (rows) OZ_HIP(hipMemcpyAsync(legal, a.word, 8ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(rc, a.code, 4ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
OZ_API int oz_mcts_root_counts(oz_mcts* m, int32_t* counts, uint64_t* legal, int32_t* rc) {
    OZ_REQUIRE(m && counts && legal && rc, "null argument");
    return root_read<0>(m, "oz_mcts_root_counts", counts, legal, rc);
}
OZ_API int oz_mcts_pruned_counts(oz_mcts* m, int32_t* counts, uint64_t* legal, int32_t* rc) {
    OZ_REQUIRE(m && counts && legal && rc, "null argument");
    return root_read<RO_PRUNED>(m, "oz_mcts_pruned_counts", counts, legal, rc);
}
OZ_API int oz_mcts_proven_counts(oz_mcts* m, int32_t* counts, uint64_t* legal, int32_t* rc) {
    OZ_REQUIRE(m && counts && legal && rc, "null argument");
    return root_read<RO_PROVEN>(m, "oz_mcts_proven_counts", counts, legal, rc);
}
OZ_API int oz_mcts_root_values(oz_mcts* m, double* value, int32_t* rc) {
    OZ_REQUIRE(m && value && rc, "null argument");
    return root_read<RO_VALUE>(m, "oz_mcts_root_values", value, nullptr, rc);
}
OZ_API int oz_mcts_proven_root_values(oz_mcts* m, double* value, int32_t* rc) {
    OZ_REQUIRE(m && value && rc, "null argument");
    return root_read<RO_PROVEN | RO_VALUE>(m, "oz_mcts_proven_root_values", value, nullptr, rc);
}
// move sampling on the current roots of the active slots: the drop-in path's move rule, under proof play over the rule's row
OZ_API int oz_mcts_sample_moves(oz_mcts* m, double temperature, uint64_t seed, const uint64_t* game_ids, const int32_t* plies, int32_t* action, int32_t* rc) {
    OZ_REQUIRE(m && game_ids && plies && action && rc, "null argument");
    if (int r = sample_check("oz_mcts_sample_moves", temperature)) return r;
    return root_read<RO_SAMPLE>(m, "oz_mcts_sample_moves", action, nullptr, rc, ReadKeys{temperature, seed, game_ids, plies});
}
OZ_API int oz_mcts_proven_sample_moves(oz_mcts* m, double temperature, uint64_t seed, const uint64_t* game_ids, const int32_t* plies, int32_t* action, int32_t* rc) {
    OZ_REQUIRE(m && game_ids && plies && action && rc, "null argument");
    if (int r = sample_check("oz_mcts_proven_sample_moves", temperature)) return r;
    return root_read<RO_PROVEN | RO_SAMPLE>(m, "oz_mcts_proven_sample_moves", action, nullptr, rc, ReadKeys{temperature, seed, game_ids, plies});
}
// oz_root_value over `count` rows, on the host: needs no device
OZ_API int oz_root_values(const int32_t* N, const double* Q, int64_t count, double* out) {
    OZ_REQUIRE(count >= 0, "oz_root_values: count %lld", (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(N && Q && out, "oz_root_values: null argument");
    for (int64_t i = 0; i < count * 64; ++i) OZ_REQUIRE(N[i] >= 0, "oz_root_values: N[%lld][%d] = %d", (long long)(i / 64), (int)(i % 64), N[i]);
    for (int64_t i = 0; i < count; ++i) {
        int rc;
        out[i] = oz_root_value(N + i * 64, Q + i * 64, &rc);
    }
    return OZ_OK;
}

// ---------------------------------------------------------------- Gumbel search: the root rule of Gumbel AlphaZero (opt-in)
// (the semantics are stated in include/othellozero_amd.h, "Gumbel search"; the restatement the tests hold this against is tests/gumbel_ref.py.)
//   * a view at depth 0, like root noise: the stored statistics are what PUCT stores, the Gumbel rule only decides which root edge a descent takes
//     (descend_one<.., GUMBEL>), on the root the slot was armed for; deeper levels and unarmed roots are PUCT;
//   * the one thing stored differently: the TV_GUMBEL expansion keeps the node's own value in header word 3 (expand_backup_one<GUMBEL>), which the
//     completed-Q formula needs at the root -- so the option is switched on over an empty tree only;
//   * a compile-time variant: an object that never switched it on launches the kernels it launched before this section existed.
// arm the CURRENT roots: one wave per slot, one lane per square.  draw != 0: g from the streams (seed, ids[g], plies[g]); else g is the host's, already
// in place.  want: null = every active slot, else the slots with want[g] != 0.  N0 = the root record's counts now (0: the root is not in the table).
__global__ __launch_bounds__(64) void k_gumbel_arm(MctsDev t, GumbelDev gd, int draw, uint64_t seed, const uint64_t* __restrict__ ids,
                                                   const int* __restrict__ plies, const uint8_t* __restrict__ want) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const uint64_t own = uni64(t.root_own[g]), opp = uni64(t.root_opp[g]);
    const uint64_t legal = oz_legal(own, opp, t.valid);
    const bool on = unii((int)t.active[g]) != 0 && legal != 0 && (want == nullptr || unii((int)want[g]) != 0);
    if (!on) {
        if (lane == 0) gd.armed[g] = 0;
        return;
    }
    const bool is_legal = (legal >> lane) & 1;
    if (draw) gd.g[(size_t)g * 64 + lane] = is_legal ? oz_gumbel_draw(seed, uni64(ids[g]), (uint64_t)unii(plies[g]), lane) : 0.0;
    const int node = root_lookup(t, g, own, opp, lane);
    int n0 = 0;
    if (node >= 0 && node < t.node_cap && is_legal) n0 = (int)(lane_edge(t, g, node, legal, lane)->n_tag & ~OZ_TAG_F32);
    gd.n0[(size_t)g * 64 + lane] = n0;
    if (lane == 0) gd.armed[g] = 1;
}
// the improved policy, the move and this lane's score at the root record `node` of an armed slot: one wave, one lane per square.  arr = 64 doubles
// of LDS.  Shared by k_gumbel_policy and the engine's move (sp_move_body<.., GUMBEL>).
struct GumbelPick { float p; double score; int move; };
__device__ __forceinline__ GumbelPick gumbel_policy_lane(const MctsDev& t, const GumbelDev& gd, double* arr, int g, int node, int lane, uint64_t legal) {
    const bool is_legal = (legal >> lane) & 1;
    const int cnt = oz_popc(legal);
    int N = 0;
    double Q = 0.0, P = 0.0;
    if (is_legal) {
        const OzEdge* e = lane_edge(t, g, node, legal, lane);
        N = (int)(e->n_tag & ~OZ_TAG_F32); Q = e->q; P = e->p;
    }
    const int nv = is_legal ? N - gd.n0[(size_t)g * 64 + lane] : 0;
    const int maxn = wave_max_i32(is_legal ? nv : -2147483647 - 1);
    OzGumbelSums sm{0, 0, 0.0, 0.0};
    for (int r = 0; r < cnt && r < t.row_cap; ++r) {                    // sequential, in square order (every lane reads the same edge: one broadcast load)
        const OzEdge* e = rec_edge(t, g, node, r);
        oz_gumbel_acc(sm, (int)(e->n_tag & ~OZ_TAG_F32), e->q, e->p);
    }
    const double vhat = *reinterpret_cast<const double*>(rec_ptr(t, g, node) + 24);
    const double vmix = oz_gumbel_vmix(sm, vhat);
    double x = -INFINITY, sc = -INFINITY;
    if (is_legal) {
        const double sg = oz_gumbel_sigma(N, Q, vmix, sm.maxN, gd.c_visit, gd.c_scale);
        x = oz_gumbel_x(P, sg);
        sc = oz_gumbel_score(gd.g[(size_t)g * 64 + lane], P, sg);
    }
    const bool cand = is_legal && nv == maxn;
    const double ms = wave_max_f64(cand ? sc : -INFINITY);
    const int best = oz_ctz(__ballot(cand && sc == ms));
    const double mx = wave_max_f64(x);
    float p;
    if (mx == -INFINITY) p = is_legal ? (float)(1.0 / (double)cnt) : 0.0f;
    else {
        const double e = is_legal ? exp(x - mx) : 0.0;
        __syncthreads();                                                // (arr may still be read by the caller's previous use)
        arr[lane] = e;
        __syncthreads();
        double sum = 0.0;
        for (int sq = 0; sq < 64; ++sq) sum = sum + arr[sq];
        p = (float)(e / sum);
    }
    return GumbelPick{p, sc, best};
}
// the improved policy row, the move and the scores of every armed slot's root: one wave per slot, one lane per square.
// rc: 0 = ok, 1 = the root is not in the table, 3 = the slot is idle or not armed (rows of zeros, scores -inf, action -1)
__global__ __launch_bounds__(64) void k_gumbel_policy(MctsDev t, GumbelDev gd, float* __restrict__ pi_out, int* __restrict__ action_out,
                                                      int* __restrict__ rc_out, double* __restrict__ score_out) {
    __shared__ double arr[64];
    const int g = blockIdx.x, lane = threadIdx.x;
    const uint64_t own = uni64(t.root_own[g]), opp = uni64(t.root_opp[g]);
    const uint64_t legal = oz_legal(own, opp, t.valid);
    const bool armed = unii((int)t.active[g]) != 0 && unii((int)gd.armed[g]) != 0 && legal != 0;
    int node = -1;
    if (armed) node = root_lookup(t, g, own, opp, lane);
    if (node < 0 || node >= t.node_cap) {
        pi_out[(size_t)g * 64 + lane] = 0.0f;
        score_out[(size_t)g * 64 + lane] = -INFINITY;
        if (lane == 0) { action_out[g] = -1; rc_out[g] = armed ? 1 : 3; }
        return;
    }
    const GumbelPick pk = gumbel_policy_lane(t, gd, arr, g, node, lane, legal);
    pi_out[(size_t)g * 64 + lane] = pk.p;
    score_out[(size_t)g * 64 + lane] = pk.score;
    if (lane == 0) { action_out[g] = pk.move; rc_out[g] = 0; }
}

static int gumbel_check(const char* fn, int max_considered, double c_visit, double c_scale, int budget) {
    OZ_REQUIRE(max_considered >= 1 && max_considered <= 64, "%s: max_considered %d outside [1, 64]", fn, max_considered);
    OZ_REQUIRE(c_visit >= 0.0 && c_visit <= 1e9, "%s: c_visit %g outside [0, 1e9]", fn, c_visit);                  // (NaN fails both compares)
    OZ_REQUIRE(c_scale > 0.0 && c_scale <= 1e9, "%s: c_scale %g outside (0, 1e9]", fn, c_scale);
    OZ_REQUIRE(budget >= 1 && budget <= OZ_GUMBEL_MAX_BUDGET, "%s: budget %d outside [1, %d]", fn, budget, OZ_GUMBEL_MAX_BUDGET);
    return OZ_OK;
}
// the schedule of every m = 1 .. max_considered at the budget, [max_considered][budget]
static std::vector<int> gumbel_tables(int max_considered, int budget) {
    std::vector<int> tab((size_t)max_considered * budget);
    for (int mm = 1; mm <= max_considered; ++mm) oz_gumbel_schedule(mm, budget, tab.data() + (size_t)(mm - 1) * budget);
    return tab;
}
// switch the option on (the first call: the arrays, 772 B per game + the table) and set its parameters
static int gumbel_enable(oz_mcts* m, const char* fn, int max_considered, double c_visit, double c_scale, int budget) {
    MctsDev& d = m->d;
    const int G = d.G;
    if (!m->gumbel_ever) {
        if (m->proofs) { oz_set_error("%s: not with proofs (the Gumbel kernels have no proven instantiation)", fn); return OZ_ERR_STATE; }
        if (m->d.sel.flags) { oz_set_error("%s: not with the selection option (the Gumbel kernels have no selection instantiation)", fn); return OZ_ERR_STATE; }
        if (m->noise_ever) { oz_set_error("%s: the Gumbel search replaces root noise and forced playouts (the object has armed root noise)", fn); return OZ_ERR_STATE; }
        if (m->wide()) { oz_set_error("%s: the Gumbel search runs one leaf per game and step (leaves_per_step is %d)", fn, m->leaves_per_step); return OZ_ERR_STATE; }
        std::vector<int> nn(G);
        OZ_HIP(hipMemcpyAsync(nn.data(), d.node_count, 4ull * G, hipMemcpyDeviceToHost, m->stream));
        OZ_HIP(hipStreamSynchronize(m->stream));
        for (int i = 0; i < G; ++i)
            if (nn[i] != 0) {
                oz_set_error("%s: the tree of game %d holds %d nodes expanded without the option (switch it on at creation or after oz_mcts_reset(-1))", fn, i, nn[i]);
                return OZ_ERR_STATE;
            }
        const size_t held = m->allocs.size();
        GumbelDev gd{};
        int rc = m->alloc(&gd.g, (size_t)G * 64);
        if (!rc) rc = m->alloc(&gd.n0, (size_t)G * 64);
        if (!rc) rc = m->alloc(&gd.armed, (size_t)G);
        if (!rc) rc = m->alloc(&m->gumbel_want, (size_t)G);
        if (!rc) rc = m->alloc(&m->gumbel_pi, (size_t)G * 64);
        if (!rc) rc = m->alloc(&m->gumbel_score, (size_t)G * 64);
        if (!rc && (hipMemsetAsync(gd.g, 0, sizeof(double) * 64 * (size_t)G, m->stream) != hipSuccess ||
                    hipMemsetAsync(gd.n0, 0, sizeof(int) * 64 * (size_t)G, m->stream) != hipSuccess ||
                    hipMemsetAsync(gd.armed, 0, (size_t)G, m->stream) != hipSuccess ||
                    hipMemsetAsync(m->gumbel_score, 0, sizeof(double) * 64 * (size_t)G, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)) {
            oz_set_error("Gumbel search: clearing the buffers failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < m->allocs.size(); ++i) hipFree(m->allocs[i]);
            m->allocs.resize(held);
            m->gumbel_want = nullptr; m->gumbel_pi = nullptr; m->gumbel_score = nullptr;
            return rc;
        }
        m->gd = gd;
        m->gumbel_ever = true;
    }
    GumbelDev& gd = m->gd;
    if (!gd.table || gd.max_considered != max_considered || gd.budget != budget) {
        const std::vector<int> tab = gumbel_tables(max_considered, budget);
        if (tab.size() > m->gumbel_table_len) {
            if (int rc = m->alloc(&m->gumbel_table, tab.size())) return rc;       // (the smaller one stays in allocs until destroy)
            m->gumbel_table_len = tab.size();
        }
        OZ_HIP(hipStreamSynchronize(m->stream));                                  // no launch still reads the table
        OZ_HIP(hipMemcpy(m->gumbel_table, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
        gd.table = m->gumbel_table;
    }
    gd.max_considered = max_considered; gd.budget = budget; gd.c_visit = c_visit; gd.c_scale = c_scale;
    return OZ_OK;
}
OZ_API int oz_mcts_set_gumbel(oz_mcts* m, int max_considered, double c_visit, double c_scale, int budget, const double* g, const uint8_t* armed) {
    OZ_REQUIRE(m, "null mcts");
    if (int rc = gumbel_check("oz_mcts_set_gumbel", max_considered, c_visit, c_scale, budget)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_PENDING(m, "oz_mcts_set_gumbel");
    hipSetDevice(m->device);
    const int G = m->d.G;
    if (g) for (size_t i = 0; i < (size_t)G * 64; ++i) OZ_REQUIRE(g[i] == g[i] && g[i] > -INFINITY && g[i] < INFINITY, "oz_mcts_set_gumbel: g[%zu][%zu] is not finite", i / 64, i % 64);
    if (int rc = gumbel_enable(m, "oz_mcts_set_gumbel", max_considered, c_visit, c_scale, budget)) return rc;
    if (!g) {                                              // the parameters only: every slot disarmed
        OZ_HIP(hipMemsetAsync(m->gd.armed, 0, (size_t)G, m->stream));
        OZ_HIP(hipStreamSynchronize(m->stream));
        return OZ_OK;
    }
    OZ_HIP(hipMemcpyAsync(m->gd.g, g, sizeof(double) * 64 * (size_t)G, hipMemcpyHostToDevice, m->stream));
    std::vector<uint8_t> a;
    if (armed) {
        a.assign(armed, armed + G);
        OZ_HIP(hipMemcpyAsync(m->gumbel_want, a.data(), G, hipMemcpyHostToDevice, m->stream));
    }
    hipLaunchKernelGGL(k_gumbel_arm, dim3(G), dim3(64), 0, m->stream, m->d, m->gd, 0, 0ull, (const uint64_t*)nullptr, (const int*)nullptr,
                       armed ? (const uint8_t*)m->gumbel_want : (const uint8_t*)nullptr);
    OZ_HIP(hipGetLastError());
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
OZ_API int oz_mcts_sample_gumbel(oz_mcts* m, int max_considered, double c_visit, double c_scale, int budget, uint64_t seed, const uint64_t* game_ids,
                                 const int32_t* plies) {
    OZ_REQUIRE(m && game_ids && plies, "null argument");
    if (int rc = gumbel_check("oz_mcts_sample_gumbel", max_considered, c_visit, c_scale, budget)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_PENDING(m, "oz_mcts_sample_gumbel");
    hipSetDevice(m->device);
    const int G = m->d.G;
    for (int i = 0; i < G; ++i) OZ_REQUIRE(plies[i] >= 0, "oz_mcts_sample_gumbel: plies[%d] = %d", i, plies[i]);
    if (int rc = gumbel_enable(m, "oz_mcts_sample_gumbel", max_considered, c_visit, c_scale, budget)) return rc;
    if (int rc = stage_keys(m, game_ids, plies)) return rc;
    hipLaunchKernelGGL(k_gumbel_arm, dim3(G), dim3(64), 0, m->stream, m->d, m->gd, 1, seed, (const uint64_t*)m->noise_ids, (const int*)m->noise_plies,
                       (const uint8_t*)nullptr);
    OZ_HIP(hipGetLastError());
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
OZ_API int oz_mcts_get_gumbel(oz_mcts* m, double* g, uint8_t* armed, int32_t* N0, int32_t* max_considered, double* c_visit, double* c_scale, int32_t* budget) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    const int G = m->d.G;
    if (max_considered) *max_considered = m->gd.max_considered;         // (0 on an object without the option)
    if (c_visit) *c_visit = m->gd.c_visit;
    if (c_scale) *c_scale = m->gd.c_scale;
    if (budget) *budget = m->gd.budget;
    if (!m->gumbel_ever) {
        if (g) memset(g, 0, sizeof(double) * 64 * (size_t)G);
        if (armed) memset(armed, 0, (size_t)G);
        if (N0) memset(N0, 0, sizeof(int32_t) * 64 * (size_t)G);
        return OZ_OK;
    }
    if (g) OZ_HIP(hipMemcpyAsync(g, m->gd.g, sizeof(double) * 64 * (size_t)G, hipMemcpyDeviceToHost, m->stream));
    if (armed) OZ_HIP(hipMemcpyAsync(armed, m->gd.armed, (size_t)G, hipMemcpyDeviceToHost, m->stream));
    if (N0) OZ_HIP(hipMemcpyAsync(N0, m->gd.n0, sizeof(int32_t) * 64 * (size_t)G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
OZ_API int oz_mcts_gumbel_policy(oz_mcts* m, float* pi, int32_t* action, int32_t* rc) {
    OZ_REQUIRE(m && pi && action && rc, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->gumbel_ever) { oz_set_error("oz_mcts_gumbel_policy: the object has no Gumbel search (oz_mcts_set_gumbel / oz_mcts_sample_gumbel first)"); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    const int G = m->d.G;
    int32_t* da = m->rc_counts; int32_t* dr = m->rc_rc;           // (the staging of oz_mcts_root_counts: [G][64] and [G])
    hipLaunchKernelGGL(k_gumbel_policy, dim3(G), dim3(64), 0, m->stream, m->d, m->gd, m->gumbel_pi, da, dr, m->gumbel_score);
    OZ_HIP(hipGetLastError());
    OZ_HIP(hipMemcpyAsync(pi, m->gumbel_pi, 4ull * G * 64, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(action, da, 4ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipMemcpyAsync(rc, dr, 4ull * G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
// the scores g + logit + sigma the last oz_mcts_gumbel_policy evaluated, [num_games][64] by square, -inf off the legal set (for inspection)
OZ_API int oz_mcts_gumbel_scores(oz_mcts* m, double* score) {
    OZ_REQUIRE(m && score, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->gumbel_ever) { oz_set_error("oz_mcts_gumbel_scores: the object has no Gumbel search"); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    OZ_HIP(hipMemcpyAsync(score, m->gumbel_score, 8ull * m->d.G * 64, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}
// header word 3 of node `index` of game `game`: the node's own value (vhat) where it was expanded under the Gumbel search or under the
// selection option, 0.0 elsewhere
OZ_API int oz_mcts_node_value(oz_mcts* m, int game, int index, double* value) {
    OZ_REQUIRE(m && value, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    MctsDev& d = m->d;
    OZ_REQUIRE(game >= 0 && game < d.G, "game index out of range");
    OZ_HIP(hipStreamSynchronize(m->stream));
    int nn = 0;
    OZ_HIP(hipMemcpy(&nn, d.node_count + game, 4, hipMemcpyDeviceToHost));
    OZ_REQUIRE(index >= 0 && index < nn, "node index %d out of range (%d nodes)", index, nn);
    OZ_HIP(hipMemcpy(value, d.recs + ((size_t)game * d.node_cap + index) * (size_t)d.rec_bytes + 24, sizeof(double), hipMemcpyDeviceToHost));
    return OZ_OK;
}
// ---- the host-only twins (no device needed)
OZ_API int oz_gumbel_considered_visits(int m, int n, int32_t* out) {
    OZ_REQUIRE(m >= 1 && m <= 64, "oz_gumbel_considered_visits: m %d outside [1, 64]", m);
    OZ_REQUIRE(n >= 1 && n <= OZ_GUMBEL_MAX_BUDGET, "oz_gumbel_considered_visits: n %d outside [1, %d]", n, OZ_GUMBEL_MAX_BUDGET);
    OZ_REQUIRE(out, "oz_gumbel_considered_visits: null argument");
    oz_gumbel_schedule(m, n, out);
    return OZ_OK;
}
OZ_API int oz_gumbel_draws(uint64_t seed, const uint64_t* game_ids, const int32_t* plies, const uint64_t* legal, int64_t count, double* g) {
    OZ_REQUIRE(count >= 0, "oz_gumbel_draws: count %lld", (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(game_ids && plies && legal && g, "oz_gumbel_draws: null argument");
    for (int64_t i = 0; i < count; ++i) OZ_REQUIRE(plies[i] >= 0, "oz_gumbel_draws: plies[%lld] = %d", (long long)i, plies[i]);
    for (int64_t i = 0; i < count; ++i)
        for (int sq = 0; sq < 64; ++sq) g[i * 64 + sq] = ((legal[i] >> sq) & 1) ? oz_gumbel_draw(seed, game_ids[i], (uint64_t)plies[i], sq) : 0.0;
    return OZ_OK;
}
OZ_API int oz_gumbel_from_units(const double* u, int64_t count, double* g) {
    OZ_REQUIRE(count >= 0, "oz_gumbel_from_units: count %lld", (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(u && g, "oz_gumbel_from_units: null argument");
    for (int64_t i = 0; i < count; ++i) OZ_REQUIRE(u[i] >= 0.0 && u[i] < 1.0, "oz_gumbel_from_units: u[%lld] = %g outside [0, 1)", (long long)i, u[i]);
    for (int64_t i = 0; i < count; ++i) g[i] = oz_gumbel_value(u[i]);
    return OZ_OK;
}
OZ_API int oz_gumbel_root(const int32_t* N, const int32_t* N0, const double* Q, const double* P, const double* g, const uint64_t* legal, const double* vhat,
                          int64_t count, int max_considered, double c_visit, double c_scale, int budget, int32_t* pick, int32_t* move, float* pi,
                          double* score, double* gaps) {
    if (int rc = gumbel_check("oz_gumbel_root", max_considered, c_visit, c_scale, budget)) return rc;
    OZ_REQUIRE(count >= 0, "oz_gumbel_root: count %lld", (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(N && N0 && Q && P && g && legal && vhat && pick && move && pi, "oz_gumbel_root: null argument");
    for (int64_t i = 0; i < count * 64; ++i)
        OZ_REQUIRE(N[i] >= 0 && N0[i] >= 0 && N0[i] <= N[i], "oz_gumbel_root: N[%lld][%d] = %d, N0 = %d", (long long)(i / 64), (int)(i % 64), N[i], N0[i]);
    const std::vector<int> tab = gumbel_tables(max_considered, budget);
    for (int64_t i = 0; i < count; ++i) {
        int pk, mv;
        oz_gumbel_root_row(N + i * 64, N0 + i * 64, Q + i * 64, P + i * 64, g + i * 64, legal[i], vhat[i], max_considered, c_visit, c_scale, budget, tab.data(),
                           &pk, &mv, pi + i * 64, score ? score + i * 64 : nullptr, gaps ? gaps + 2 * i : nullptr, gaps ? gaps + 2 * i + 1 : nullptr);
        pick[i] = pk; move[i] = mv;
    }
    return OZ_OK;
}

// ---- forced playouts: host side
static int forced_check(const char* fn, double k) {
    OZ_REQUIRE(k >= 0.0 && k <= 16.0, "%s: k %g outside [0, 16] (0 = off)", fn, k);          // (NaN fails both compares)
    return OZ_OK;
}
// k > 0 needs root noise armed on the object (forcing is a rule of the noisy root); k == 0 switches off
static int forced_set_locked(oz_mcts* m, const char* fn, double k) {
    if (k > 0.0 && m->proofs) { oz_set_error("%s: not with proofs (forcing a proven loss would undo them)", fn); return OZ_ERR_STATE; }
    if (k > 0.0 && m->d.sel.flags) { oz_set_error("%s: not with the selection option (the quota and the pruning restate PUCT with the constant c)", fn); return OZ_ERR_STATE; }
    if (k > 0.0 && !(m->noise_ever && m->d.noise_eps > 0.0)) {
        oz_set_error("%s: forced playouts need root noise (arm it first)", fn);
        return OZ_ERR_STATE;
    }
    m->d.forced_k = k;                                     // takes effect at the next launch (kernels get the struct by value)
    return OZ_OK;
}
OZ_API int oz_mcts_set_forced_playouts(oz_mcts* m, double k) {
    OZ_REQUIRE(m, "null mcts");
    if (int rc = forced_check("oz_mcts_set_forced_playouts", k)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    OZ_REFUSE_PENDING(m, "oz_mcts_set_forced_playouts");
    return forced_set_locked(m, "oz_mcts_set_forced_playouts", k);
}
OZ_API int oz_mcts_get_forced_playouts(oz_mcts* m, double* k) {
    OZ_REQUIRE(m && k, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    *k = m->d.forced_k;
    return OZ_OK;
}
// oz_proof_play of one root, on the host: needs no device.  edge[sq] = -1 / 0 / +1 or OZ_PROOF_UNKNOWN as oz_mcts_root_proofs gives them
// (read on the legal squares), own_value likewise; counts = the root's 64 raw counts.
OZ_API int oz_search_proof_play(uint64_t legal, const int8_t* edge, int own_value, const int32_t* counts, int8_t* val, uint64_t* keep, int32_t* row,
                                int* fallback, int* inconsistent) {
    OZ_REQUIRE(edge && counts, "oz_search_proof_play: null argument");
    OZ_REQUIRE(own_value == OZ_PROOF_NONE || (own_value >= -1 && own_value <= 1), "oz_search_proof_play: own_value = %d", own_value);
    uint64_t lo = 0, hi = 0, visited = 0;
    for (int sq = 0; sq < 64; ++sq) {
        OZ_REQUIRE(counts[sq] >= 0, "oz_search_proof_play: counts[%d] = %d", sq, counts[sq]);
        if (counts[sq] > 0) visited |= 1ULL << sq;
        if (!((legal >> sq) & 1) || edge[sq] == OZ_PROOF_NONE) continue;
        OZ_REQUIRE(edge[sq] >= -1 && edge[sq] <= 1, "oz_search_proof_play: edge[%d] = %d", sq, (int)edge[sq]);
        oz_proof_mark(&lo, &hi, sq, edge[sq]);
    }
    OZ_REQUIRE((visited & ~legal) == 0, "oz_search_proof_play: a count off the legal set");
    uint64_t k;
    int f, bad;
    const int v = oz_proof_play(legal, lo, hi, own_value, visited, &k, &f, &bad);
    if (val) *val = (int8_t)v;
    if (keep) *keep = k;
    if (fallback) *fallback = f;
    if (inconsistent) *inconsistent = bad;
    if (row) for (int sq = 0; sq < 64; ++sq) row[sq] = ((k >> sq) & 1) ? counts[sq] : 0;
    return OZ_OK;
}

// oz_forced_prune over `count` rows, on the host: needs no device
OZ_API int oz_forced_playouts_prune(const int32_t* N, const double* Q, const double* P, const double* eta, const uint64_t* legal, const int32_t* Ns,
                                    int64_t count, double c, double eps, double k, int32_t* pruned) {
    OZ_REQUIRE(count >= 0, "oz_forced_playouts_prune: count %lld", (long long)count);
    if (int rc = forced_check("oz_forced_playouts_prune", k)) return rc;
    OZ_REQUIRE(eps >= 0.0 && eps <= 1.0, "oz_forced_playouts_prune: eps %g outside [0, 1]", eps);
    OZ_REQUIRE(c == c, "oz_forced_playouts_prune: c is NaN");
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(N && Q && P && eta && legal && Ns && pruned, "oz_forced_playouts_prune: null argument");
    for (int64_t i = 0; i < count; ++i) {
        OZ_REQUIRE(Ns[i] >= 0, "oz_forced_playouts_prune: Ns[%lld] = %d", (long long)i, Ns[i]);
        for (int sq = 0; sq < 64; ++sq)
            OZ_REQUIRE(N[i * 64 + sq] >= 0, "oz_forced_playouts_prune: N[%lld][%d] = %d", (long long)i, sq, N[i * 64 + sq]);
    }
    for (int64_t i = 0; i < count; ++i) {
        const int32_t* n = N + i * 64;
        const double *q = Q + i * 64, *p = P + i * 64, *e = eta + i * 64;
        int32_t* out = pruned + i * 64;
        int star = -1;
        for (int sq = 0; sq < 64; ++sq)
            if (((legal[i] >> sq) & 1) && (star < 0 || n[sq] > n[star])) star = sq;          // the first legal square with the largest N
        for (int sq = 0; sq < 64; ++sq)
            out[sq] = ((legal[i] >> sq) & 1) ? oz_forced_prune(n[sq], q[sq], p[sq], e[sq], n[star], q[star], p[star], e[star], sq == star, Ns[i], c, eps, k) : 0;
    }
    return OZ_OK;
}

// OthelloMCTS.get_policy_action_probabilities (othelo_mcts.py:51-67) of every game's current root: float64 (n, n) row-major rows.
//   temperature != 0: N ** (1 / T) on the legal squares, divided by np.sum of the (n, n) array (NumPy's pairwise order) -- or by 1 if that is 0;
//   temperature == 0: one-hot of a best square: of the squares whose count equals the maximum of the (n, n) array, in row-major order (np.argwhere),
//                     the one `tie_draws[g] % (how many)` picks -- random.choice(bests) in the reference; null tie_draws: the first.
// rc[g] as oz_mcts_root_counts reports it; a root that was expanded but never selected from (rc 2: KeyError in the reference) gets a zero row.
OZ_API int oz_mcts_policy(oz_mcts* m, double temperature, const uint64_t* tie_draws, double* policy, int32_t* rc) {
    OZ_REQUIRE(m && policy && rc, "null argument");
    const int G = m->d.G, n = m->d.n, n2 = n * n;
    std::vector<int32_t> counts((size_t)G * 64);
    std::vector<uint64_t> legal((size_t)G);
    if (int r = oz_mcts_root_counts(m, counts.data(), legal.data(), rc)) return r;
    for (int g = 0; g < G; ++g) {
        double* out = policy + (size_t)g * n2;
        double arr[64];
        for (int i = 0; i < n2; ++i) arr[i] = 0.0;
        for (int i = 0; i < n2; ++i) out[i] = 0.0;
        if (rc[g] == 2) continue;
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c)
                if ((legal[g] >> (r * 8 + c)) & 1) {
                    const int cnt = counts[(size_t)g * 64 + r * 8 + c];
                    arr[r * n + c] = temperature == 0 ? (double)cnt : pow((double)cnt, 1.0 / temperature);
                }
        if (temperature == 0) {
            double mx = arr[0];
            for (int i = 1; i < n2; ++i) mx = arr[i] > mx ? arr[i] : mx;
            int nb = 0;
            for (int i = 0; i < n2; ++i) nb += arr[i] == mx;
            int pick = tie_draws ? (int)(tie_draws[g] % (uint64_t)nb) : 0;
            for (int i = 0; i < n2; ++i)
                if (arr[i] == mx && pick-- == 0) { out[i] = 1.0; break; }
        } else {
            double sum = n2 >= 8 ? pairwise_sum(arr, n2) : 0.0;
            if (n2 < 8) for (int i = 0; i < n2; ++i) sum += arr[i];
            if (sum == 0) sum = 1.0;
            for (int i = 0; i < n2; ++i) out[i] = arr[i] / sum;
        }
    }
    return OZ_OK;
}

OZ_API int oz_mcts_num_nodes(oz_mcts* m, int32_t* num_nodes) {
    OZ_REQUIRE(m && num_nodes, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    OZ_HIP(hipMemcpyAsync(num_nodes, m->d.node_count, 4ull * m->d.G, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    return OZ_OK;
}

OZ_API int oz_mcts_dump_node(oz_mcts* m, int game, int index, uint64_t* own, uint64_t* opp, int32_t* Ns, uint64_t* legal,
                             int32_t* N, double* Q, uint8_t* qtag, double* P) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    MctsDev& d = m->d;
    OZ_REQUIRE(game >= 0 && game < d.G, "game index out of range");
    OZ_HIP(hipStreamSynchronize(m->stream));
    int nn = 0;
    OZ_HIP(hipMemcpy(&nn, d.node_count + game, 4, hipMemcpyDeviceToHost));
    OZ_REQUIRE(index >= 0 && index < nn, "node index %d out of range (%d nodes)", index, nn);
    std::vector<unsigned char> rec((size_t)d.rec_bytes);
    OZ_HIP(hipMemcpy(rec.data(), d.recs + ((size_t)game * d.node_cap + index) * (size_t)d.rec_bytes, rec.size(), hipMemcpyDeviceToHost));
    const uint64_t* h = reinterpret_cast<const uint64_t*>(rec.data());
    *own = h[0]; *opp = h[1];
    *Ns = (int32_t)(uint32_t)h[2];
    *legal = oz_legal(h[0], h[1], d.valid);                 // the legal set is a function of the key (recomputed, not stored)
    const OzEdge* e = reinterpret_cast<const OzEdge*>(rec.data() + OZ_REC_HDR);
    for (int s = 0; s < 64; ++s) { N[s] = 0; Q[s] = 0; qtag[s] = 0; P[s] = 0; }
    int k = 0;
    for (int s = 0; s < 64; ++s)
        if ((*legal >> s) & 1) { N[s] = (int)(e[k].n_tag & ~OZ_TAG_F32); qtag[s] = (e[k].n_tag & OZ_TAG_F32) ? 1 : 0; Q[s] = e[k].q; P[s] = e[k].p; ++k; }
    return OZ_OK;
}

static int mcts_stats_locked(oz_mcts* m, int64_t* out5) {
    const size_t cnt = (size_t)m->d.G * OZ_NSTAT;
    std::vector<unsigned long long> h(cnt);
    OZ_HIP(hipMemcpyAsync(h.data(), m->d.stat, 8 * cnt, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    for (int k = 0; k < OZ_NSTAT; ++k) out5[k] = 0;
    for (size_t i = 0; i < cnt; ++i) out5[i % OZ_NSTAT] += (int64_t)h[i];
    return OZ_OK;
}
OZ_API int oz_mcts_stats(oz_mcts* m, int64_t* out5) {
    OZ_REQUIRE(m && out5, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    hipSetDevice(m->device);
    return mcts_stats_locked(m, out5);
}

// ---------------------------------------------------------------- tree collection: drop the nodes a slot's game has passed (opt-in)
// (the semantics are stated in include/othellozero_amd.h, "tree collection"; the rule is oz_tree_keep, oz_common.h.)
// One wave per game, active slots only, against the slot's current root.  What holds a record index across move rounds, and what becomes of it:
//   * every edge's `child`: -1 stays, anything else becomes map[child] (a kept node's child holds more discs than the root: kept too);
//   * root_node[g]: set to -1, whoever needs the root looks it up again (the descents, root_lookup);
//   * the OzProof entry of a node (an array parallel to the records): moves with its record;
//   * the hash table: zeroed and refilled from the kept records.
// path / the per-(game, j) arrays of the leaf-parallel search / leaf_* / hit_entry live inside a step and no step is pending here; Gumbel's n0,
// the noise eta are by square; vhat (header word 3) travels inside the record.  An expansion writes every byte of a record (and of its proof
// entry) that any reader reads -- the header whole, popcount(legal) edges, the unused half of the last 16-byte chunk -- so the freed tail is
// left as it is: the next expansion into a freed index overwrites what will be read of it.
// A kernel of its own with arguments of its own (MctsDev is untouched): an object that never arms the option launches and allocates nothing.
__global__ __launch_bounds__(64) void k_tree_collect(MctsDev t, TreeGcDev gc) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) { gc.last[(size_t)g * 2] = 0; gc.last[(size_t)g * 2 + 1] = 0; }
    if (!unii((int)t.active[g])) return;
    const int nc = unii(t.node_count[g]);
    long long* st = gc.stat + (size_t)g * OZ_NGCSTAT;
    if (lane == 0 && (long long)nc > st[GC_PEAK_NODES]) st[GC_PEAK_NODES] = nc;
    if (nc < 0 || nc > t.node_cap) { if (lane == 0) atomicOr(t.error_flag, EF_CORRUPT); return; }
    if (gc.mode == OZ_TREE_GC_ON_DEMAND && (long long)nc + (long long)gc.sims <= (long long)t.node_cap) return;     // (uniform: a simulation expands at most one node)
    const uint64_t ro = uni64(t.root_own[g]), rp = uni64(t.root_opp[g]);
    int* __restrict__ map = gc.map + (size_t)g * t.node_cap;
    // pass 1, the plan: a lane per record header, ballot + prefix popcount per 64 = the stable old -> new map
    int kept = 0;
    for (int base = 0; base < nc; base += 64) {
        const int i = base + lane;
        bool keep = false;
        if (i < nc) {
            const uint64_t* h = reinterpret_cast<const uint64_t*>(rec_ptr(t, g, i));
            keep = oz_tree_keep(ro, rp, h[0], h[1]);
        }
        const uint64_t kb = __ballot(keep);
        if (i < nc) map[i] = keep ? kept + oz_popc(kb & ((1ULL << lane) - 1ULL)) : -1;
        kept += oz_popc(kb);
    }
    __threadfence();
    __syncthreads();
    // pass 2, the move: kept records to their new index in ascending order, in place (dst <= src and records are disjoint strides: a forward
    // sweep never overwrites a record it has yet to read).  One wave-wide 16-byte load per record, as the descent's; every byte as it was
    // except the edges' child words.
    const int rec_chunks = t.rec_bytes >> 4;                       // <= 64
    bool bad = false;
    for (int base = 0; base < nc; base += 64) {
        const int mi = base + lane < nc ? map[base + lane] : -1;
        uint64_t kb = __ballot(mi >= 0);
        while (kb) {
            const int l = oz_ctz(kb);
            kb &= kb - 1;
            const int src = base + l, dst = lane_get(mi, l);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (lane < rec_chunks) v = reinterpret_cast<const uint4*>(rec_ptr(t, g, src))[lane];
            int cnt = lane_get((int)v.y, 1);                       // header word 2 = Ns | cnt << 32: the high half is lane 1's .y
            if (cnt < 0 || cnt > t.row_cap) { bad = true; cnt = 0; }
            const int chunks = (OZ_REC_HDR + cnt * OZ_EDGE_BYTES + 15) >> 4;
            uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int w = 4 * lane + j - 9;                    // the child of edge r is 32-bit word 9 + 6 r of the record
                if (w >= 0 && w % 6 == 0 && w / 6 < cnt && (int)x[j] != -1) {
                    const int c = (int)x[j];
                    int nm = -1;
                    if ((unsigned)c < (unsigned)nc) nm = map[c];
                    if (nm < 0) bad = true;                        // never a dangling index: the edge forgets its child (and the error is raised)
                    x[j] = (uint32_t)nm;
                }
            }
            if (lane < chunks) reinterpret_cast<uint4*>(rec_ptr(t, g, dst))[lane] = make_uint4(x[0], x[1], x[2], x[3]);
            if (t.pf.entry != nullptr && dst != src) {
                uint4 pv = make_uint4(0, 0, 0, 0);
                if (lane < 2) pv = reinterpret_cast<const uint4*>(t.pf.entry + (size_t)g * t.node_cap + src)[lane];
                if (lane < 2) reinterpret_cast<uint4*>(t.pf.entry + (size_t)g * t.node_cap + dst)[lane] = pv;
            }
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(t.error_flag, EF_CORRUPT);
    // pass 3, the hash table: empty the game's window, then the kept nodes 64 at a time, each by linear probing from its key's base slot --
    // a slot only ever goes from empty to taken, so every slot between a key's base and its entry is taken: what ht_find relies on
    uint32_t* ht = t.ht + (size_t)g * t.ht_cap;
    const int mask = t.ht_cap - 1;
    for (int i = lane; i < t.ht_cap; i += 64) ht[i] = 0;
    __threadfence();
    __syncthreads();
    for (int base = 0; base < kept; base += 64) {
        const int i = base + lane;
        if (i < kept) {
            const uint64_t* h = reinterpret_cast<const uint64_t*>(rec_ptr(t, g, i));
            const uint64_t own = h[0], opp = h[1];
            const uint32_t e = ht_entry(own, opp, i);
            int slot = (int)((uint32_t)(key_hash64(own, opp) >> 17) & (uint32_t)mask);
            for (int probed = 0; probed < t.ht_cap; ++probed, slot = (slot + 1) & mask)     // (ht_cap >= 2 node_cap: a free slot exists)
                if (atomicCAS(&ht[slot], 0u, e) == 0u) break;
        }
    }
    // pass 4, the counters
    if (lane == 0) {
        t.node_count[g] = kept;
        t.root_node[g] = -1;
        st[GC_COLLECTIONS] += 1; st[GC_BEFORE] += nc; st[GC_KEPT] += kept;
        if ((long long)kept > st[GC_PEAK_KEPT]) st[GC_PEAK_KEPT] = kept;
        gc.last[(size_t)g * 2] = nc; gc.last[(size_t)g * 2 + 1] = kept;
    }
}

static int tree_gc_check(const char* fn, int mode) {
    OZ_REQUIRE(mode == OZ_TREE_GC_OFF || mode == OZ_TREE_GC_ON_DEMAND || mode == OZ_TREE_GC_EVERY_MOVE, "%s: unknown tree_gc mode %d", fn, mode);
    return OZ_OK;
}
// the scratch map and the counters, at the object's first arming
static int tree_gc_alloc(oz_mcts* m) {
    if (m->gc.map) return OZ_OK;
    hipSetDevice(m->device);
    const MctsDev& d = m->d;
    const size_t held = m->allocs.size();
    TreeGcDev gc{};
    int rc = m->alloc(&gc.map, (size_t)d.G * d.node_cap);
    if (!rc) rc = m->alloc(&gc.stat, (size_t)d.G * OZ_NGCSTAT);
    if (!rc) rc = m->alloc(&gc.last, (size_t)d.G * 2);
    if (rc) {
        for (size_t i = held; i < m->allocs.size(); ++i) hipFree(m->allocs[i]);
        m->allocs.resize(held);
        return rc;
    }
    OZ_HIP(hipMemsetAsync(gc.stat, 0, sizeof(long long) * (size_t)d.G * OZ_NGCSTAT, m->stream));
    OZ_HIP(hipMemsetAsync(gc.last, 0, sizeof(long long) * (size_t)d.G * 2, m->stream));
    m->gc = gc;
    return OZ_OK;
}
// one launch on m->stream (the object is armed: tree_gc_alloc has run); sims = the budget ON_DEMAND makes room for
static void tree_collect_async(oz_mcts* m, int mode, int sims) {
    TreeGcDev gc = m->gc;
    gc.mode = mode; gc.sims = sims;
    const long long ti = m->gc_profile ? m->gc_timer.begin(0, m->stream) : -1;
    hipLaunchKernelGGL(k_tree_collect, dim3(m->d.G), dim3(64), 0, m->stream, m->d, gc);
    m->gc_timer.end(ti, m->stream);
    if (m->gc_profile && m->gc_timer.backlog() > 4096) m->gc_timer.drain();
}
static int tree_gc_stats_locked(oz_mcts* m, oz_tree_gc_stats* out) {
    memset(out, 0, sizeof *out);
    if (!m->gc.stat) return OZ_OK;
    hipSetDevice(m->device);
    const size_t cnt = (size_t)m->d.G * OZ_NGCSTAT;
    std::vector<long long> h(cnt);
    OZ_HIP(hipMemcpyAsync(h.data(), m->gc.stat, sizeof(long long) * cnt, hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    for (int g = 0; g < m->d.G; ++g) {
        const long long* s = h.data() + (size_t)g * OZ_NGCSTAT;
        out->collections += s[GC_COLLECTIONS]; out->nodes_before_sum += s[GC_BEFORE]; out->nodes_kept_sum += s[GC_KEPT];
        if (s[GC_PEAK_NODES] > out->peak_nodes) out->peak_nodes = s[GC_PEAK_NODES];
        if (s[GC_PEAK_KEPT] > out->peak_kept) out->peak_kept = s[GC_PEAK_KEPT];
    }
    return OZ_OK;
}
static int tree_gc_profile_read_locked(oz_mcts* m, double* ms_total, int64_t* launches, int reset) {
    hipSetDevice(m->device);
    if (m->gc_timer.collect() != OZ_OK) { oz_set_error("HIP event timing failed"); return OZ_ERR_HIP; }
    if (ms_total) *ms_total = m->gc_timer.ms[0];
    if (launches) *launches = m->gc_timer.count[0];
    if (reset) m->gc_timer.reset();
    return OZ_OK;
}

OZ_API int oz_mcts_collect(oz_mcts* m, int64_t* out2) {
    OZ_REQUIRE(m, "null mcts");
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->selected) { oz_set_error("oz_mcts_collect: a host-evaluated step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; }
    hipSetDevice(m->device);
    if (int rc = tree_gc_alloc(m)) return rc;
    tree_collect_async(m, OZ_TREE_GC_EVERY_MOVE, 0);
    OZ_HIP(hipGetLastError());
    std::vector<long long> last((size_t)m->d.G * 2);
    OZ_HIP(hipMemcpyAsync(last.data(), m->gc.last, sizeof(long long) * last.size(), hipMemcpyDeviceToHost, m->stream));
    OZ_HIP(hipStreamSynchronize(m->stream));
    if (out2) {
        out2[0] = out2[1] = 0;
        for (int g = 0; g < m->d.G; ++g) { out2[0] += last[(size_t)g * 2]; out2[1] += last[(size_t)g * 2 + 1]; }
    }
    return check_error_flag(m);
}
OZ_API int oz_mcts_tree_gc_stats(oz_mcts* m, oz_tree_gc_stats* stats) {
    OZ_REQUIRE(m && stats, "null argument");
    std::lock_guard<std::mutex> lk(m->mu);
    return tree_gc_stats_locked(m, stats);
}
// the rule on the host, no device needed
OZ_API int oz_search_tree_keep(uint64_t root_own, uint64_t root_opp, const uint64_t* own, const uint64_t* opp, int64_t count, uint8_t* keep,
                               int32_t* new_index, int64_t* kept) {
    OZ_REQUIRE(count >= 0 && (count == 0 || (own && opp && keep && new_index)) && kept, "oz_search_tree_keep: null argument or count %lld < 0", (long long)count);
    OZ_REQUIRE(count <= 0x7FFFFFFFLL, "oz_search_tree_keep: count %lld does not fit a node index", (long long)count);
    int64_t k = 0;
    for (int64_t i = 0; i < count; ++i) {
        const bool kp = oz_tree_keep(root_own, root_opp, own[i], opp[i]);
        keep[i] = kp ? 1 : 0;
        new_index[i] = kp ? (int32_t)k : -1;
        k += kp ? 1 : 0;
    }
    *kept = k;
    return OZ_OK;
}

// ================================================================ self-play driver
struct GamesDev {
    int G, n;
    uint64_t valid;
    uint64_t *black, *white, *game_id;
    int8_t* player;
    uint8_t* finished;
    int* ply;
    // per-slot move log of the game in progress
    uint64_t *log_black, *log_white;      // [G][64]
    uint8_t *log_action, *log_greedy;     // [G][64]
    int8_t* log_player;                   // [G][64]
    int32_t* last_counts;                 // [G][64]
    oz_record* records;
    // oz_selfplay_config.record_visits: root visit counts of every move of the game in progress, and of every record (same ring index)
    int32_t* log_counts;                  // [G][64 plies][64 squares], or null
    int32_t* visits;                      // [record_cap][64], or null
    // oz_selfplay_set_record_values: the root value of every move of the game in progress, and of every record (same ring index)
    double* log_values;                   // [G][64 plies], or null
    double* values;                       // [record_cap], or null
    unsigned long long* counters;         // [0] records [1] games completed [2] moves
    long long record_cap;
    int record_visits;
    uint64_t seed, id_stride;
    double temperature, e_greedy;
    int refill, init_black_set;
    uint64_t init_black, init_white;
};

__global__ void k_sp_roots(GamesDev gm, MctsDev t, int mover_filter /* 0 all, +1 / -1: only games with that mover */) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= gm.G) return;
    const int p = gm.player[g];
    const bool act = !gm.finished[g] && (mover_filter == 0 || mover_filter == p);
    t.active[g] = act ? 1 : 0;
    if (t.noise_armed) t.noise_armed[g] = 0;              // root noise belongs to the old root (k_root_noise follows where the engine draws it)
    if (act) {
        t.root_node[g] = -1;
        t.root_own[g] = p == 1 ? gm.black[g] : gm.white[g];
        t.root_opp[g] = p == 1 ? gm.white[g] : gm.black[g];
    }
}

// oz_selfplay_stagger: in round r only the slots whose start offset is still ahead of r search and move
__global__ void k_sp_roots_stagger(GamesDev gm, MctsDev t, int round, int period) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= gm.G) return;
    const int offset = (int)(((long long)g * period) / gm.G);
    const int p = gm.player[g];
    const bool act = !gm.finished[g] && offset > round;
    t.active[g] = act ? 1 : 0;
    if (t.noise_armed) t.noise_armed[g] = 0;              // root noise belongs to the old root (k_root_noise follows where the engine draws it)
    if (act) {
        t.root_node[g] = -1;
        t.root_own[g] = p == 1 ? gm.black[g] : gm.white[g];
        t.root_opp[g] = p == 1 ? gm.white[g] : gm.black[g];
    }
}

// K7: root policy extraction + action choice + OthelloGame.play + example recording
// (othelo_mcts.py:51-67, training.py:45-67 / agents.py:52-68).  One wave per game.
//   arena != 0: agents.py semantics (temperature 0, argmax over valid actions of the one-hot).
// NOISE (the free-running advance of an engine with root noise): the move takes the slot to another root -- its noise is dropped, the advance
// draws the next root's.  The lock-step k_sp_move leaves root and noise as they are until the next round's roots kernel (oz_selfplay_root_noise
// reads them in between).  (noise_armed is null on an engine whose only extra is move sampling.)
// SAMPLE (an engine with move sampling, oz_selfplay_set_move_sampling): where the coin falls on the greedy branch and ply < ms.plies, the move is
// drawn by sample_move, keyed (seed, game id, ply), instead of taken as the arg-max; greedy = 2 in its record.  Never in the arena.
// CAP (an engine with a playout cap, oz_selfplay_set_playout_cap; pc.fast_sims > 0 where it is on): the move's full / fast bit, oz_playout_budget
// of (seed, game id, ply), goes into the move log next to `greedy` and from there into byte pad[0] of the game's records; one of two counters
// counts the move.  The move rule itself does not look at the bit.  Never in the arena, never in a staggered round.
// FORCE (an engine with forced playouts, oz_selfplay_set_forced_playouts; fp.k > 0 where it is on): on a root whose noise is armed -- read before
// NOISE clears the flag -- the row that goes to log_counts / visits is the pruned one (forced_prune_lane) and three counters count it.  Everything
// that chooses the move keeps reading the raw counts.  A fast move of a playout cap is unarmed: never pruned.  Never in the arena.
// VALUES (an engine that records root values, oz_selfplay_set_record_values; gm.log_values != null where it is on): the visit-weighted mean of
// the root's Q over the raw counts goes into the move log next to the counts and from there beside the game's records.  Such an engine launches
// instantiations of its own (MV_FULL in a lock-step round; the AV_EXTRAS advance or, with no other option, AV_VALUES alone), so the kernels of an
// engine without it stay the code they were, register for register.  Never in the arena.
// GUMBEL (an engine with the Gumbel search, oz_selfplay_set_gumbel; lock-step rounds only): the round's roots kernel is followed by k_gumbel_arm,
// so the root of every active slot with a legal move is armed.  Where the coin falls on its greedy branch the move is the Gumbel root's
// (gumbel_policy_lane), greedy = 3 in its record; the explore branch is unchanged.  The float32 improved-policy row of the search goes into the
// move log and from there beside the game's records, as the visit-count rows do.  Never in the arena.
struct GumbelPlay {
    GumbelDev gd;
    float* log_pi;                         // [G][64 plies][64 squares]
    float* policies;                       // [record_cap][64]
    unsigned long long* moves;             // [1] moves picked by the Gumbel rule
};
// SURPRISE (an engine that records policy surprise, oz_selfplay_set_record_surprise; "policy surprise weighting" in the header): s = KL(q || p)
// of the move's search, q the row that becomes the policy target (the pruned count row at T = 1, normalised as k_expand_visits does; under GUMBEL
// the float32 improved-policy row) and p the root's stored priors, goes into the move log and from there beside the game's records, as the
// root value does.  Instantiations of its own (MV_SURPRISE, AV_SURPRISE): every other kernel stays the code it was.
// Never in the arena.
struct SurprisePlay {
    double* log;                           // [G][64 plies]
    double* rec;                           // [record_cap]
};
// RESIGN (an engine with resignation, oz_selfplay_set_resign; "resignation" in the header; lock-step rounds only; rs.r > 0 where it is on): the
// slot's (side, streak) take the move's root value -- the VALUES rootv, no second routine -- through oz_resign_step (oz_common.h).  At the first
// trigger of a game that is not exempt, where the move does not end the game by itself, the game ends through the `fin` branch with the winner
// overridden and pad[1] = 1 in its records; an exempt game remembers its first trigger and is counted at its natural end.  Lane 0 resets the
// slot's state where the game ends.  Instantiations of its own (MV_RESIGN): every other kernel stays the code it was.  Never
// in the arena.
struct ResignPlay {
    double v, keep_prob;
    int r, min_ply;                        // r > 0 = on
    int8_t* side;                          // [G] whose win the last root values called (+1 BLACK, -1 WHITE, 0 nobody's)
    uint8_t* streak;                       // [G] for how many searched moves in a row
    int8_t* ex_side;                       // [G] exempt game: the side of its first trigger, 0 = none yet
    uint8_t* ex_ply;                       // [G] ... and its ply
    unsigned long long* stat;              // [6] oz_resign_stats in its order
};
// (calls, not inlined code: a 64-term pairwise_sum of constant length is unrolled into 64 loads in flight, 128 VGPRs; inlined into the move
// they cost the free-running advance a wave of occupancy for all of its simulations, and the sums run once per move)
__device__ __noinline__ double surprise_row_sum(const double* a) { return pairwise_sum(a, 64); }
// PROVEN (an engine or an arena agent with proof play, oz_selfplay_set_proof_play / oz_arena_set_proof_play; "proof play" in the header; on top
// of proofs, lock-step rounds only): the move loads the root's proof entry -- one 32-byte wave-uniform load -- and applies oz_proof_play
// (oz_common.h): `row` is the raw count on the kept squares, and everything that reads `row` -- log_counts / visits, SURPRISE, and here every
// branch of the move that reads counts -- reads it and its maximum; rootv is the exact value where it is known (VALUES logs it, RESIGN reads it);
// the proof code goes into the move log and from there into byte pad[2] of the game's records.  The explore branch of the coin stays uniform
// over the legal set and last_counts stays raw.  Instantiations of its own (MV_PROVEN): every other kernel stays the code it was.
struct ProofPlay {
    uint8_t* log;                          // [G][64 plies] the proof code of every ply of the game in progress; null in the arena
    unsigned long long* stat;              // [4] proven roots, rows changed, moves changed, fallbacks; null in the arena
};
__device__ __noinline__ double surprise_sum(const double* term) { return oz_surprise_sum(term); }
template <bool NOISE = false, bool SAMPLE = false, bool CAP = false, bool FORCE = false, bool VALUES = false, bool GUMBEL = false, bool SURPRISE = false,
          bool RESIGN = false, bool PROVEN = false>
__device__ __forceinline__ void sp_move_body(const GamesDev& gm, const MctsDev& t, int g, int lane, int arena, MoveSampling ms = MoveSampling{},
                                             PlayoutCap pc = PlayoutCap{}, ForcedPlayouts fp = ForcedPlayouts{}, GumbelPlay gp = GumbelPlay{},
                                             SurprisePlay su = SurprisePlay{}, ResignPlay rs = ResignPlay{}, ProofPlay pp = ProofPlay{}) {
    static_assert(!RESIGN || VALUES, "resignation reads the root value the VALUES move computes");
    static_assert(!PROVEN || !GUMBEL, "proofs and the Gumbel search exclude each other");
    if (!t.active[g]) return;
    bool prune = false;
    (void)prune;
    if constexpr (FORCE) prune = fp.k > 0.0 && t.noise_eps > 0.0 && t.noise_armed && unii((int)t.noise_armed[g]) != 0;
    if constexpr (NOISE) { if (lane == 0 && t.noise_armed) t.noise_armed[g] = 0; }
    const uint64_t own = uni64(t.root_own[g]), opp = uni64(t.root_opp[g]);
    const uint64_t legal = oz_legal(own, opp, t.valid);
    const int node = root_lookup(t, g, own, opp, lane);
    if (node < 0 || *rec_Ns(t, g, node) == 0) {           // KeyError path of the reference (sims < 2)
        if (lane == 0) atomicOr(t.error_flag, EF_ROOT);
        return;
    }
    const bool is_legal = (legal >> lane) & 1;
    int cnt = 0;
    if (is_legal) cnt = (int)(lane_edge(t, g, node, legal, lane)->n_tag & ~OZ_TAG_F32);
    gm.last_counts[(size_t)g * 64 + lane] = cnt;
    // proof play: what the root's proof entry keeps of the counts (proof_row); every value is wave-uniform
    int pval = OZ_PROOF_NONE, pfall = 0;
    uint64_t pkeep = legal;
    (void)pval; (void)pfall; (void)pkeep;
    if constexpr (PROVEN) {
        const ProofRow p = proof_row(t, g, node, cnt);
        pval = p.val; pkeep = p.keep; pfall = p.fall;
    }
    // record_values: the root value of this search from the RAW counts and the stored Q (root_value)
    double rootv = 0.0;
    (void)rootv;
    if constexpr (VALUES) {
        if (gm.log_values) {
            __shared__ double terms[64];
            rootv = root_value(terms, cnt, is_legal ? lane_edge(t, g, node, legal, lane)->q : 0.0, lane).v;
            wave_sync();                                         // the next move of this wave (free-running loop) writes terms[] again
            if constexpr (PROVEN) { if (pval != OZ_PROOF_NONE) rootv = (double)pval; }
        }
    }
    const int ply = unii(gm.ply[g]);
    const size_t lb = (size_t)g * 64;
    const uint64_t gid = uni64(gm.game_id[g]);
    const int mx = unii(wave_max_i32(cnt));                      // >= 1 once the root has been selected from
    int row = cnt;                                               // what the policy target keeps of cnt
    if constexpr (FORCE) {
        if (prune) {
            row = forced_prune_lane(t, g, node, lane, legal, cnt, mx, fp.k);
            const int raw = wave_sum_i32(cnt), kept = wave_sum_i32(row);
            if (lane == 0) {
                if (kept != raw) atomicAdd(&fp.stat[0], 1ULL);
                atomicAdd(&fp.stat[1], (unsigned long long)raw);
                atomicAdd(&fp.stat[2], (unsigned long long)kept);
            }
        }
    }
    int mcnt = cnt, mmx = mx;                                    // what the move reads: the raw counts, or under PROVEN the row and its maximum
    if constexpr (PROVEN) {
        row = ((pkeep >> lane) & 1) ? cnt : 0;
        mcnt = row; mmx = unii(wave_max_i32(row));
    }
    float gpi = 0.0f;                                            // this lane's entry of the improved policy row
    int gmove = -1;
    (void)gpi; (void)gmove;
    if constexpr (GUMBEL) {
        if (unii((int)gp.gd.armed[g]) != 0) {
            __shared__ double garr[64];
            const GumbelPick pk = gumbel_policy_lane(t, gp.gd, garr, g, node, lane, legal);
            gpi = pk.p; gmove = pk.move;
        }
    }
    // record_surprise: KL(target row || stored priors) of this search (oz_surprise_term / oz_surprise_sum, oz_common.h)
    double surp = 0.0;
    (void)surp;
    if constexpr (SURPRISE) {
        __shared__ double sterm[64];
        double q;
        if constexpr (GUMBEL) q = (double)gpi;
        else {
            sterm[lane] = (double)row;                            // oz_count_pow at T = 1 (k = 1: the count itself), then the sum and the one division of
                                                                  // k_expand_visits / k_replay_append<VISITS>; spelled out: the call would compile pow() in
            wave_sync();
            const double sum = surprise_row_sum(sterm);
            wave_sync();
            q = sterm[lane] / (sum == 0 ? 1.0 : sum);
            wave_sync();
        }
        sterm[lane] = oz_surprise_term(q, is_legal ? lane_edge(t, g, node, legal, lane)->p : 0.0);
        wave_sync();
        surp = surprise_sum(sterm);
        wave_sync();                                             // the next move of this wave (free-running loop) writes sterm[] again
    }
    int action, greedy = 1;
    if (arena || gm.temperature == 0.0) {
        // bests = argwhere(p == p.max()) over the whole board; random.choice(bests) -> RNG_TIE stream
        const uint64_t bests = __ballot(is_legal && mcnt == mmx);
        const int nbests = oz_popc(bests);
        action = oz_kth_bit(bests, (int)(oz_rng(gm.seed, gid, (uint64_t)ply, OZ_RNG_TIE) % (uint64_t)nbests));
    } else {
        // N**(1/T) / sum is monotone in N: argwhere(policy == policy.max())[0] = first max-visit square
        action = oz_ctz(__ballot(is_legal && mcnt == mmx));
    }
    if constexpr (GUMBEL) {
        if (gmove >= 0) { action = gmove; greedy = 3; }
    }
    if (!arena) {
        const double coin = oz_rng_unit(oz_rng(gm.seed, gid, (uint64_t)ply, OZ_RNG_COIN));
        if (!(coin <= gm.e_greedy)) {                      // training.py:53-56
            greedy = 0;
            action = oz_kth_bit(legal, (int)(oz_rng(gm.seed, gid, (uint64_t)ply, OZ_RNG_EXPLORE) % (uint64_t)oz_popc(legal)));
        } else if constexpr (SAMPLE) {
            if (ply < ms.plies) {
                greedy = 2;
                action = sample_move(mcnt, legal, mmx, ms.temperature, oz_rng_unit(oz_rng(gm.seed, gid, (uint64_t)ply, OZ_RNG_SAMPLE)), lane);
            }
        }
    }
    // proof play: the proof code of the move, and the counters -- the move the raw counts give is evaluated beside the one played
    int pcode = 0;
    (void)pcode;
    if constexpr (PROVEN) {
        pcode = oz_proof_code(pval);
        const bool row_changed = __ballot(row != cnt) != 0;
        bool move_changed = false;
        if (row_changed && greedy != 0) {
            int raw;
            if (greedy == 2) raw = sample_move(cnt, legal, mx, ms.temperature, oz_rng_unit(oz_rng(gm.seed, gid, (uint64_t)ply, OZ_RNG_SAMPLE)), lane);
            else if (arena || gm.temperature == 0.0) {
                const uint64_t bests = __ballot(is_legal && cnt == mx);
                raw = oz_kth_bit(bests, (int)(oz_rng(gm.seed, gid, (uint64_t)ply, OZ_RNG_TIE) % (uint64_t)oz_popc(bests)));
            } else raw = oz_ctz(__ballot(is_legal && cnt == mx));
            move_changed = raw != action;
        }
        if (lane == 0 && pp.stat) {
            if (pcode) atomicAdd(&pp.stat[0], 1ULL);
            if (row_changed) atomicAdd(&pp.stat[1], 1ULL);
            if (move_changed) atomicAdd(&pp.stat[2], 1ULL);
            if (pfall) atomicAdd(&pp.stat[3], 1ULL);
        }
    }
    uint64_t black = uni64(gm.black[g]), white = uni64(gm.white[g]);
    int player = unii(gm.player[g]), fin = 0;
    if (lane == 0 && ply < 64) {
        gm.log_black[lb + ply] = black; gm.log_white[lb + ply] = white;
        gm.log_action[lb + ply] = (uint8_t)action; gm.log_player[lb + ply] = (int8_t)player;
        gm.log_greedy[lb + ply] = (uint8_t)greedy;
        if constexpr (PROVEN) { if (pp.log) pp.log[lb + ply] = (uint8_t)pcode; }
    }
    int fast = 0;
    (void)fast;
    if constexpr (CAP) {
        if (pc.fast_sims > 0) {
            oz_playout_budget(gm.seed, gid, (uint64_t)ply, 0, pc.fast_sims, pc.full_prob, &fast);
            if (lane == 0) {
                if (ply < 64) pc.log_fast[lb + ply] = (uint8_t)fast;
                atomicAdd(&pc.moves[fast], 1ULL);
            }
        }
    }
    // resignation: the slot's state takes this move's root value (oz_resign_step, oz_common.h); every value below is wave-uniform
    OzResign rst{0, 0};
    bool rtrig = false, rexempt = false, adjudicated = false;
    int rex_side = 0, rex_ply = 0;
    (void)rst; (void)rtrig; (void)rexempt; (void)adjudicated; (void)rex_side; (void)rex_ply;
    if constexpr (RESIGN) {
        if (rs.r > 0) {
            rst = OzResign{unii((int)rs.side[g]), unii((int)rs.streak[g])};
            rtrig = oz_resign_step(rst, player, rootv, rs.v, rs.r, rs.min_ply, ply);
            rexempt = oz_resign_is_exempt(gm.seed, gid, rs.keep_prob);
            rex_side = unii((int)rs.ex_side[g]); rex_ply = unii((int)rs.ex_ply[g]);
            if (rtrig && rexempt && rex_side == 0) { rex_side = rst.side; rex_ply = ply; }       // the first trigger of an exempt game
        }
    }
    oz_game_play(black, white, player, fin, action, gm.valid);
    const int nply = ply + 1;
    if constexpr (RESIGN) {
        if (rtrig && !rexempt && !fin) { adjudicated = true; fin = 1; }       // the move was played as ever; the game stops here
    }
    if (fin) {
        // get_winning_player: draw -> BLACK; z = +1 if winner == mover else -1 (training.py:69-72)
        int winner = oz_popc(black) >= oz_popc(white) ? 1 : -1;
        if constexpr (RESIGN) {
            if (rs.r > 0 && lane == 0) {
                if (adjudicated) {
                    atomicAdd(&rs.stat[0], 1ULL);
                    atomicAdd(&rs.stat[1], (unsigned long long)nply);
                } else if (rexempt) {
                    atomicAdd(&rs.stat[2], 1ULL);
                    if (rex_side != 0) {
                        atomicAdd(&rs.stat[3], 1ULL);
                        if (winner != rex_side) atomicAdd(&rs.stat[4], 1ULL);
                        atomicAdd(&rs.stat[5], (unsigned long long)rex_ply);
                    }
                }
            }
            if (adjudicated) winner = rst.side;
        }
        unsigned long long base = 0;
        if (lane == 0) {
            base = atomicAdd(&gm.counters[0], (unsigned long long)nply);
            atomicAdd(&gm.counters[1], 1ULL);
        }
        base = __shfl(base, 0, 64);
        if (lane < nply) {                                 // lane i writes the record of ply i
            if ((long long)(base + lane) < gm.record_cap) {
                oz_record r;
                const bool cur = lane == ply;              // this ply's log entry is still in registers
                r.black = cur ? gm.black[g] : gm.log_black[lb + lane];
                r.white = cur ? gm.white[g] : gm.log_white[lb + lane];
                r.final_black = black; r.final_white = white; r.game_id = gid;
                r.ply = (uint8_t)lane; r.action = cur ? (uint8_t)action : gm.log_action[lb + lane];
                r.player = cur ? gm.player[g] : gm.log_player[lb + lane];
                r.z = (int8_t)(winner == r.player ? 1 : -1);
                r.greedy = cur ? (uint8_t)greedy : gm.log_greedy[lb + lane];
                r.pad[0] = r.pad[1] = r.pad[2] = 0;
                if constexpr (CAP) { if (pc.fast_sims > 0) r.pad[0] = cur ? (uint8_t)fast : pc.log_fast[lb + lane]; }
                if constexpr (RESIGN) { if (adjudicated) r.pad[1] = 1; }
                if constexpr (PROVEN) { if (pp.log) r.pad[2] = cur ? (uint8_t)pcode : pp.log[lb + lane]; }
                gm.records[base + lane] = r;
            } else atomicOr(t.error_flag, EF_RECORDS);
        }
        if (gm.record_visits) {
            // row i of the game's counts next to record i, one coalesced 256-byte row per ply; a row is written where its record is
            // (the loop above has flagged EF_RECORDS for the rest).  This ply's row is still in registers.
            const long long room = gm.record_cap - (long long)base;
            for (int i = 0; i < nply && i < room; ++i)
                gm.visits[(size_t)(base + i) * 64 + lane] = i == ply ? row : gm.log_counts[(lb + i) * 64 + lane];
        }
        if constexpr (GUMBEL) {                               // the improved-policy rows next to the records, as the visit-count rows above
            const long long room = gm.record_cap - (long long)base;
            for (int i = 0; i < nply && i < room; ++i)
                gp.policies[(size_t)(base + i) * 64 + lane] = i == ply ? gpi : gp.log_pi[(lb + i) * 64 + lane];
        }
        // the game's root values next to its records, lane i the value of ply i; this ply's is still in registers
        if constexpr (VALUES) {
            if (gm.log_values && lane < nply && (long long)(base + lane) < gm.record_cap)
                gm.values[base + lane] = lane == ply ? rootv : gm.log_values[lb + lane];
        }
        if constexpr (SURPRISE) {                             // ... and its surprises, the same way
            if (lane < nply && (long long)(base + lane) < gm.record_cap) su.rec[base + lane] = lane == ply ? surp : su.log[lb + lane];
        }
    } else {
        if (gm.record_visits && ply < 64) gm.log_counts[(lb + ply) * 64 + lane] = row;
        if constexpr (VALUES) { if (gm.log_values && lane == 0 && ply < 64) gm.log_values[lb + ply] = rootv; }
        if constexpr (GUMBEL) { if (ply < 64) gp.log_pi[(lb + ply) * 64 + lane] = gpi; }
        if constexpr (SURPRISE) { if (lane == 0 && ply < 64) su.log[lb + ply] = surp; }
    }
    if constexpr (GUMBEL) { if (lane == 0 && greedy == 3) atomicAdd(gp.moves, 1ULL); }
    if (lane == 0) atomicAdd(&gm.counters[2], 1ULL);
    if constexpr (RESIGN) {                                // the slot's state: that of the game in progress, zero for the next game where this one ended
        if (rs.r > 0 && lane == 0) {
            rs.side[g] = (int8_t)(fin ? 0 : rst.side); rs.streak[g] = (uint8_t)(fin ? 0 : rst.streak);
            rs.ex_side[g] = (int8_t)(fin ? 0 : rex_side); rs.ex_ply[g] = (uint8_t)(fin ? 0 : rex_ply);
        }
    }
    if (fin && gm.refill) {
        // a fresh OthelloGame + a fresh OthelloMCTS in the same slot (training.py:30-32)
        for (int i = lane; i < t.ht_cap; i += 64) t.ht[(size_t)g * t.ht_cap + i] = 0;
        if (lane == 0) {
            t.node_count[g] = 0; t.root_node[g] = -1;
            gm.black[g] = gm.init_black; gm.white[g] = gm.init_white; gm.player[g] = 1;
            gm.finished[g] = 0; gm.ply[g] = 0; gm.game_id[g] = gid + gm.id_stride;
        }
    } else if (lane == 0) {
        gm.black[g] = black; gm.white[g] = white; gm.player[g] = (int8_t)player;
        gm.finished[g] = (uint8_t)fin; gm.ply[g] = nply;
        t.root_node[g] = -1;                               // the position changed: the next descent looks its root up again
    }
}
// ---- the move kernel of the lock-step rounds and the arena: one template, instantiated per variant.  M is a mask of MV_* flags; move_kernel()
// (host side) computes it from the engine's state, fills the arguments and is the one place that says which masks have a kernel.
//   flag          option (what sets it)                                              template argument of sp_move_body (described above it)
//   MV_SAMPLE     move sampling (oz_selfplay_set_move_sampling); a.ms.plies == 0: off     SAMPLE
//   MV_CAP        a playout cap (oz_selfplay_set_playout_cap); a.pc.fast_sims == 0: off   CAP     (a staggered round passes a cap that is off)
//   MV_FORCE      forced playouts (oz_selfplay_set_forced_playouts); a.fp.k == 0: off     FORCE
//   MV_VALUES     recorded root values (oz_selfplay_set_record_values); gm.log_values     VALUES
//   MV_GUMBEL     the Gumbel search (oz_selfplay_set_gumbel): a.gp                        GUMBEL
//   MV_SURPRISE   recorded policy surprise (oz_selfplay_set_record_surprise): a.su        SURPRISE
//   MV_RESIGN     resignation (oz_selfplay_set_resign): a.rs                              RESIGN  (reads the VALUES root value)
//   MV_PROVEN     proof play (oz_selfplay_set_proof_play / oz_arena_set_proof_play): a.pp PROVEN  (a.pp is null in the arena)
// MV_FULL is what every self-play engine with forced playouts, recorded values, recorded surprise, resignation or proof play launches: those
// options are looked at when the move runs, so their combinations need no kernels of their own.  NOISE is the free-running advance's alone.
enum : unsigned { MV_SAMPLE = 1, MV_CAP = 2, MV_FORCE = 4, MV_VALUES = 8, MV_GUMBEL = 16, MV_SURPRISE = 32, MV_RESIGN = 64, MV_PROVEN = 128,
                  MV_FULL = MV_SAMPLE | MV_CAP | MV_FORCE | MV_VALUES };
// a default-constructed member is an option that is off.  (What MV_FULL and its combinations read comes first and packed, as those kernels
// always took it, the Gumbel state behind: the order at which every instantiation keeps the registers of the kernel it replaced.)
struct MoveArgs {
    MoveSampling ms; PlayoutCap pc; ForcedPlayouts fp; SurprisePlay su; ResignPlay rs; ProofPlay pp; GumbelPlay gp;
    int arena;                             // != 0: agents.py semantics
};
template <unsigned M>
__global__ __launch_bounds__(64) void k_sp_move(GamesDev gm, MctsDev t, MoveArgs a) {
    // (the plain move alone serves self-play and the arena; MV_PROVEN by itself is the arena's, everything else self-play's: the flag folds away)
    const int arena = M == 0 ? a.arena : M == MV_PROVEN ? 1 : 0;
    sp_move_body<false, has(M, MV_SAMPLE), has(M, MV_CAP), has(M, MV_FORCE), has(M, MV_VALUES), has(M, MV_GUMBEL), has(M, MV_SURPRISE), has(M, MV_RESIGN),
                 has(M, MV_PROVEN)>(gm, t, blockIdx.x, threadIdx.x, arena, a.ms, a.pc, a.fp, a.gp, a.su, a.rs, a.pp);
}

// ---------------------------------------------------------------- free-running self-play step
// The lock-step driver gives every game one simulation per step; simulations that end on a finished board need no
// network evaluation, so ~8 % of the slots of a leaf batch stay empty and a move round always costs `sims` network passes.
// k_advance lets every game run on by itself until its next simulation needs the network: it counts the simulation the
// previous step completed, plays the move once `sims` of them are done (k_sp_move's body: action choice, play, records,
// refill), walks further simulations that end on finished boards (k_select's body + the backup), and stops at the first
// first-visit leaf -- so (almost) every game contributes one leaf to every batch.  A game's own sequence of simulations,
// moves and random draws is exactly the lock-step one (games are independent, streams are keyed by game id and ply, a
// position's (pi, v) does not depend on the batch it sits in), so records are identical; only the interleaving of the
// games changes.  OZ_ADVANCE_CAP bounds the work of one call (late-game positions whose whole remaining tree is known
// can run many network-free simulations); a game that hits the cap simply contributes no leaf to this batch.  The launch lasts
// as long as its slowest wave, so the cap trades batch fill for launch time -- measured at 4096 games x 100 simulations
// (bench.py --driver free): cap 24 -> 4081 leaves per batch but 367 us per launch, 1.40 M expansions/s; cap 8 -> 1.56 M;
// cap 4 -> 1.585 M; cap 2 -> 3908 leaves per batch, 1.59 M (1.60 M with k_backup_advance; the lock-step driver: 1.56-1.58 M).
#define OZ_ADVANCE_CAP 2
// EXTRAS: the one instantiation for engines with root noise, move sampling, a playout cap or any of them together; which of them is on is looked
// at when it runs (t.noise_eps > 0, xt.sample.plies > 0, xt.cap.fast_sims > 0).  An engine with none launches the EXTRAS = false kernels, which
// are the code they were before.  VALUES: the move records root values where gm.log_values is set (sp_move_body<.., VALUES>); part of EXTRAS,
// and on its own the instantiation of an engine whose only option it is (AV_VALUES alone: the plain kernels plus the move's value, not the
// registers of every extra).
//   playout cap: the move is played once `done` reaches the budget of the slot's current (game id, ply) instead of `sims`; a fast root draws no
//   noise.  Both are oz_playout_budget of the key, evaluated again at every pass of the loop: noise_armed[g] == 0 keeps meaning "no noise on this
//   root" and needs no third state for "decided: none", and a fast root stays unarmed for oz_selfplay_root_noise to report.
//   root noise: the noise of a game's root is drawn here, before the first descent from it (noise_armed[g] == 0: a fresh engine, or the move above
//   has just changed the root), keyed (seed, game id, ply) like k_root_noise in the lock-step round: the records stay those of oz_selfplay_run.
//   move sampling: sp_move_body<.., SAMPLE> is a function of the root's counts and (seed, game id, ply): the same records again.
//   forced playouts: the descents force through t.forced_k, the move prunes its row while the root's noise is still armed (sp_move_body<.., FORCE>
//   reads the flag before it clears it): a function of the root record and eta, the same rows again.
struct SelfplayExtras { double alpha; uint64_t seed; MoveSampling sample; PlayoutCap cap; ForcedPlayouts forced; };
template <bool EXTRAS = false, bool VALUES = EXTRAS, bool SURPRISE = false, int VS = OZ_VSIGNS_REFERENCE>
__device__ __forceinline__ void advance_body(const GamesDev& gm, const MctsDev& t, TreeLds& L, int g, int lane, int sims, int* __restrict__ sims_done, int cap,
                                             SelfplayExtras xt = SelfplayExtras{}, SurprisePlay su = SurprisePlay{}) {
    if (unii(t.leaf_status[g]) == OZ_LEAF_WAIT) {          // batch cap: the leaf of the simulation in progress found no slot -- offer it again, unchanged
        if (lane == 0) t.leaf_status[g] = OZ_LEAF_EVAL;
        return;
    }
    int done = sims_done[g];
    if (t.leaf_status[g] == OZ_LEAF_EVAL) ++done;          // the simulation whose leaf the previous step evaluated and backed up
    int status = OZ_LEAF_IDLE;
    for (int it = 0; it < cap; ++it) {
        if (gm.finished[g]) { if (lane == 0) { t.active[g] = 0; t.leaf_status[g] = OZ_LEAF_IDLE; } status = OZ_LEAF_IDLE; break; }
        // roots of the position to move in (k_sp_roots)
        const int p = gm.player[g];
        if (lane == 0) {
            t.active[g] = 1;
            t.root_own[g] = p == 1 ? gm.black[g] : gm.white[g];
            t.root_opp[g] = p == 1 ? gm.white[g] : gm.black[g];
        }
        wave_sync();                                       // lane 0's stores are visible to the wave's next loads
        int budget = sims, fast = 0;
        if constexpr (EXTRAS) {
            if (xt.cap.fast_sims > 0)
                budget = oz_playout_budget(gm.seed, uni64(gm.game_id[g]), (uint64_t)unii(gm.ply[g]), sims, xt.cap.fast_sims, xt.cap.full_prob, &fast);
        }
        if (done >= budget) {                              // training.py:42-67: the move after num_simulations simulations
            sp_move_body<EXTRAS, EXTRAS, EXTRAS, EXTRAS, VALUES, false, SURPRISE>(gm, t, g, lane, 0, xt.sample, xt.cap, xt.forced, GumbelPlay{}, su);
            done = 0;
            if (lane == 0) t.leaf_status[g] = OZ_LEAF_IDLE;    // the evaluated leaf is consumed: nothing pending if the cap ends the loop here
            wave_sync();
            continue;                                      // (a finished game is refilled by the move, or goes idle above)
        }
        if constexpr (EXTRAS) {
            if (t.noise_eps > 0.0 && !fast && unii((int)t.noise_armed[g]) == 0) {
                root_noise_body(t, L.arr, g, lane, uni64(t.root_own[g]), uni64(t.root_opp[g]), xt.alpha, xt.seed, uni64(gm.game_id[g]), unii(gm.ply[g]));
                wave_sync();
            }
        }
        status = select_body<EXTRAS, false, VS>(t, L, g, lane);
        if (status != OZ_LEAF_TERMINAL) break;             // EVAL: wait for the network; IDLE: error path
        wave_sync();
        backup_body<VS>(t, g, lane, (double)t.term_value[g], VT_INT);
        ++done;
        status = OZ_LEAF_IDLE;
        if (lane == 0) t.leaf_status[g] = OZ_LEAF_IDLE;    // nothing pending if the cap ends the loop here
        wave_sync();
    }
    if (lane == 0) sims_done[g] = done;
}
// ---- the free-running kernels: one template per phase, instantiated per variant.  A is a mask of AV_* flags; advance_kernels() (host side)
// computes it from the engine's state, fills the arguments and is the one place that says which masks have a kernel.
//   flag          option (what sets it)                                                    template argument of advance_body (described above it)
//   AV_SIGNS      the low two bits ARE the OZ_VSIGNS_* value (REFERENCE or SOUND: no proofs)   VS
//   AV_EXTRAS     root noise, move sampling, a playout cap, recorded surprise: any of them     EXTRAS (each is looked at when it runs: a.xt)
//   AV_VALUES     recorded root values; every AV_EXTRAS kernel has it                          VALUES (gm.log_values says whether it records)
//   AV_SURPRISE   recorded policy surprise; on top of AV_EXTRAS                                SURPRISE (a.su)
enum : unsigned { AV_SIGNS = 3, AV_EXTRAS = 4, AV_VALUES = 8, AV_SURPRISE = 16 };
// a default-constructed xt / su is an option that is off
struct AdvanceArgs { SelfplayExtras xt; SurprisePlay su; };
template <unsigned A>
__global__ __launch_bounds__(64) void k_advance(GamesDev gm, MctsDev t, int sims, int* __restrict__ sims_done, int cap, AdvanceArgs a) {
    __shared__ TreeLds L;
    advance_body<has(A, AV_EXTRAS), has(A, AV_VALUES), has(A, AV_SURPRISE), int(A & AV_SIGNS)>(gm, t, L, blockIdx.x, threadIdx.x, sims, sims_done, cap, a.xt, a.su);
}
// expand + backup of the leaves the previous batch evaluated and the advance to the next batch's leaves in ONE launch (the free-running
// counterpart of k_backup_select: one kernel boundary less per batch, the records just written are re-read from the CU's cache)
template <unsigned A>
__global__ __launch_bounds__(64) void k_backup_advance(GamesDev gm, MctsDev t, int sims, int* __restrict__ sims_done, int cap, AdvanceArgs a) {
    __shared__ TreeLds L;
    expand_backup_body<false, int(A & AV_SIGNS)>(t, L, blockIdx.x, threadIdx.x, 0);
    backup_fence();
    advance_body<has(A, AV_EXTRAS), has(A, AV_VALUES), has(A, AV_SURPRISE), int(A & AV_SIGNS)>(gm, t, L, blockIdx.x, threadIdx.x, sims, sims_done, cap, a.xt, a.su);
}

// RandomOthelloAgent.play (agents.py:20-24) for every live game whose mover is `side`: random.choice over the valid
// actions in ascending row-major order -> the RNG_TIE stream (the fixture generator patches random.choice to it)
__global__ void k_arena_random_move(GamesDev gm, int side) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= gm.G || gm.finished[g] || gm.player[g] != side) return;
    uint64_t black = gm.black[g], white = gm.white[g];
    int player = side, fin = 0;
    const uint64_t legal = oz_legal(side == 1 ? black : white, side == 1 ? white : black, gm.valid);
    const int ply = gm.ply[g];
    const int action = oz_kth_bit(legal, (int)(oz_rng(gm.seed, gm.game_id[g], (uint64_t)ply, OZ_RNG_TIE) % (uint64_t)oz_popc(legal)));
    const size_t lb = (size_t)g * 64;
    if (ply < 64) {
        gm.log_black[lb + ply] = black; gm.log_white[lb + ply] = white;
        gm.log_action[lb + ply] = (uint8_t)action; gm.log_player[lb + ply] = (int8_t)player; gm.log_greedy[lb + ply] = 0;
    }
    oz_game_play(black, white, player, fin, action, gm.valid);
    gm.black[g] = black; gm.white[g] = white; gm.player[g] = (int8_t)player;
    gm.finished[g] = (uint8_t)fin; gm.ply[g] = ply + 1;
    atomicAdd(&gm.counters[2], 1ULL);
}

// The minimax opponent (agents.py:27-41, oz_minimax.h) in k_arena_random_move's place: one wave per game, the move = the RNG_TIE choice among the
// moves of maximal root value; the same move log, oz_game_play, ply and move counter.
__global__ __launch_bounds__(64) void k_arena_minimax_move(GamesDev gm, int side, int depth, MinimaxEval ev) {
    __shared__ MinimaxLds L;
    const int g = blockIdx.x, lane = threadIdx.x;
    if (gm.finished[g] || gm.player[g] != side) return;                 // block-uniform
    uint64_t black = gm.black[g], white = gm.white[g], bests = 0;
    mm_root(L, ev, gm.valid, lane, black, white, side, depth, &bests);
    if (lane != 0 || bests == 0) return;                                // (a live game's mover always has a move)
    int player = side, fin = 0;
    const int ply = gm.ply[g];
    const int action = oz_kth_bit(bests, (int)(oz_rng(gm.seed, gm.game_id[g], (uint64_t)ply, OZ_RNG_TIE) % (uint64_t)oz_popc(bests)));
    const size_t lb = (size_t)g * 64;
    if (ply < 64) {
        gm.log_black[lb + ply] = black; gm.log_white[lb + ply] = white;
        gm.log_action[lb + ply] = (uint8_t)action; gm.log_player[lb + ply] = (int8_t)player; gm.log_greedy[lb + ply] = 0;
    }
    oz_game_play(black, white, player, fin, action, gm.valid);
    gm.black[g] = black; gm.white[g] = white; gm.player[g] = (int8_t)player;
    gm.finished[g] = (uint8_t)fin; gm.ply[g] = ply + 1;
    atomicAdd(&gm.counters[2], 1ULL);
}

// The opening of every arena game (oz_openings.h; oz_arena_set_openings / oz_arena_set_opening_moves), once, before the first round: one thread
// per game plays the opening with id first_id + g -- NOT the game's id -- from the standard position the slot holds, logs its plies like any other
// move (greedy 0) and leaves board, mover, finished flag and ply where the first searched round takes over.  At most 16 plies: the log has room.
__global__ void k_arena_openings(GamesDev gm, OpeningsDev op) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= gm.G) return;
    uint64_t black, white;
    int player, fin;
    const size_t lb = (size_t)g * 64;
    const int played = oz_opening_play(gm.n, gm.valid, op.moves ? op.n_plies[g] : op.plies, op.moves ? op.moves + (size_t)g * OZ_OPENING_MAX_PLIES : nullptr,
                                       op.seed, op.first_id + (uint64_t)g, black, white, player, fin,
                                       [&](int ply, uint64_t b, uint64_t w, int p, int action) {
                                           gm.log_black[lb + ply] = b; gm.log_white[lb + ply] = w;
                                           gm.log_action[lb + ply] = (uint8_t)action; gm.log_player[lb + ply] = (int8_t)p; gm.log_greedy[lb + ply] = 0;
                                       });
    gm.black[g] = black; gm.white[g] = white; gm.player[g] = (int8_t)player;
    gm.finished[g] = (uint8_t)fin; gm.ply[g] = played;
    op.opening_plies[g] = played;
    if (played) atomicAdd(&gm.counters[2], (unsigned long long)played);
}

static void initial_board(int n, uint64_t* black, uint64_t* white) { oz_initial_board(n, *black, *white); }

struct oz_selfplay {
    oz_selfplay_config cfg;
    oz_mcts* m = nullptr;
    oz_net* net = nullptr;
    GamesDev gm;
    int* d_sims_done = nullptr;      // free-running mode: simulations completed for the move in progress, per game
    int mode = 0;                    // 0 fresh, 1 driven by oz_selfplay_run (lock step), 2 by oz_selfplay_run_steps (free-running)
    int batch_cap = 0;               // free-running driver: leaves per network batch (0: up to G)
    long long batch_no = 0;          // batches launched by the free-running driver (rotation of the slot order under a cap)
    int stagger_period = 0;
    bool noise_on = false;           // oz_selfplay_set_root_noise: every searched move draws Dir(noise_alpha) at its root
    double noise_alpha = 0.0;
    MoveSampling sample{0.0, 0};     // oz_selfplay_set_move_sampling: plies > 0 = on
    PlayoutCap cap{0, 0.0, nullptr, nullptr};      // oz_selfplay_set_playout_cap: fast_sims > 0 = on (the buffers stay once allocated)
    ForcedPlayouts forced{0.0, nullptr};           // oz_selfplay_set_forced_playouts: k > 0 = on (the counters stay once allocated); m->d.forced_k holds the same k
    bool gumbel_on = false;          // oz_selfplay_set_gumbel: every searched move of a lock-step round is a Gumbel root search
    float *gumbel_log = nullptr, *gumbel_rows = nullptr;       // its improved-policy rows: the move log and the rows beside the records
    unsigned long long* gumbel_moves = nullptr;
    std::vector<void*> allocs;
    std::mutex mu;
    long long records_read = 0;
    long long* d_endgame = nullptr;  // oz_selfplay_solve_records: its six counters (allocated by the first call)
    // oz_selfplay_set_record_values: the buffers stay once allocated; gm.log_values / gm.values point at them while the option is on
    double *val_log = nullptr, *val_rec = nullptr;
    float* targets = nullptr;        // oz_selfplay_value_targets: [record_cap], allocated by the first call
    long long* d_vt = nullptr;       // ... and its three counters
    // oz_selfplay_set_record_surprise: the buffers stay once allocated; su points at them while the option is on
    double *sur_log = nullptr, *sur_rec = nullptr;
    SurprisePlay su{nullptr, nullptr};
    float* weights = nullptr;        // oz_selfplay_surprise_weights: [record_cap] each, allocated by the first call
    int32_t* copies = nullptr;
    uint8_t* first_sym = nullptr;
    long long* d_sw = nullptr;       // ... and its five counters
    ResignPlay resign{0.0, 0.0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};      // oz_selfplay_set_resign: r > 0 = on (the buffers stay once allocated)
    // oz_selfplay_set_proof_play (the arena: oz_arena_set_proof_play, [0] BLACK's agent, [1] WHITE's): the buffers stay once allocated
    bool proof_play = false, arena_proof_play[2] = {false, false};
    ProofPlay pplay{nullptr, nullptr};
    long long* d_pt = nullptr;       // oz_selfplay_proof_targets: its three counters (allocated by the first call)
    // oz_selfplay_set_tree_gc (the arena: oz_arena_set_tree_gc, [0] BLACK's agent, [1] WHITE's): k_tree_collect after the round's roots kernel
    int tree_gc = OZ_TREE_GC_OFF, arena_tree_gc[2] = {OZ_TREE_GC_OFF, OZ_TREE_GC_OFF};
    template <typename T> int alloc(T** p, size_t count) {
        OZ_HIP(hipMalloc((void**)p, sizeof(T) * (count ? count : 1)));
        allocs.push_back(*p);
        return OZ_OK;
    }
};

static int games_alloc(oz_selfplay* sp, int G, int n, long long record_cap, int record_visits) {
    GamesDev& gm = sp->gm;
    memset(&gm, 0, sizeof gm);
    gm.G = G; gm.n = n; gm.valid = oz_valid_mask(n); gm.record_cap = record_cap; gm.record_visits = record_visits;
    int rc = OZ_OK;
#define A(ptr, cnt) if (!rc) rc = sp->alloc(&gm.ptr, cnt)
    A(black, G); A(white, G); A(game_id, G); A(player, G); A(finished, G); A(ply, G);
    A(log_black, (size_t)G * 64); A(log_white, (size_t)G * 64); A(log_action, (size_t)G * 64);
    A(log_greedy, (size_t)G * 64); A(log_player, (size_t)G * 64); A(last_counts, (size_t)G * 64);
    A(records, (size_t)record_cap); A(counters, 4);
    if (record_visits) { A(log_counts, (size_t)G * 64 * 64); A(visits, (size_t)record_cap * 64); }      // 16 KB per slot, 256 B per record
#undef A
    return rc;
}

static int games_init(oz_selfplay* sp, uint64_t first_id, hipStream_t s) {
    GamesDev& gm = sp->gm;
    const int G = gm.G;
    uint64_t b, w;
    initial_board(gm.n, &b, &w);
    gm.init_black = b; gm.init_white = w;
    std::vector<uint64_t> hb(G, b), hw(G, w), ids(G);
    for (int i = 0; i < G; ++i) ids[i] = first_id + (uint64_t)i;
    std::vector<int8_t> pl(G, 1);
    OZ_HIP(hipMemcpyAsync(gm.black, hb.data(), 8ull * G, hipMemcpyHostToDevice, s));
    OZ_HIP(hipMemcpyAsync(gm.white, hw.data(), 8ull * G, hipMemcpyHostToDevice, s));
    OZ_HIP(hipMemcpyAsync(gm.game_id, ids.data(), 8ull * G, hipMemcpyHostToDevice, s));
    OZ_HIP(hipMemcpyAsync(gm.player, pl.data(), G, hipMemcpyHostToDevice, s));
    OZ_HIP(hipMemsetAsync(gm.finished, 0, G, s));
    OZ_HIP(hipMemsetAsync(gm.ply, 0, 4ull * G, s));
    OZ_HIP(hipMemsetAsync(gm.counters, 0, 8 * 4, s));
    OZ_HIP(hipMemsetAsync(gm.last_counts, 0, 4ull * G * 64, s));
    OZ_HIP(hipStreamSynchronize(s));
    return OZ_OK;
}

OZ_API int oz_selfplay_create(oz_selfplay** out, const oz_selfplay_config* cfg, oz_net* net) {
    OZ_REQUIRE(out && cfg && net, "null argument");
    OZ_REQUIRE(cfg->sims >= 2, "num_simulations must be >= 2 (with 1 the reference raises KeyError at othelo_mcts.py:66)");
    OZ_REQUIRE(cfg->num_games > 0, "num_games must be positive");
    OZ_REQUIRE(net->n == cfg->n, "network board size %d != %d", net->n, cfg->n);
    OZ_REQUIRE(net->max_batch >= cfg->num_games, "network max_batch %d < num_games %d", net->max_batch, cfg->num_games);
    OZ_REQUIRE(cfg->dedup == OZ_DEDUP_DEFAULT || cfg->dedup == OZ_DEDUP_ON || cfg->dedup == OZ_DEDUP_OFF, "oz_selfplay_config.dedup = %d", cfg->dedup);
    OZ_REQUIRE(cfg->eval_cache == 0 || cfg->eval_cache == 1, "oz_selfplay_config.eval_cache = %d", cfg->eval_cache);
    OZ_REQUIRE(cfg->batch_cap == 0 || cfg->batch_cap >= 8, "oz_selfplay_config.batch_cap = %d (0 = none, else >= 8 leaves)", cfg->batch_cap);
    OZ_REQUIRE(cfg->record_visits == 0 || cfg->record_visits == 1, "oz_selfplay_config.record_visits = %d", cfg->record_visits);
    oz_selfplay* sp = new oz_selfplay();
    sp->cfg = *cfg; sp->net = net;
    const int max_plies = cfg->n * cfg->n - 4;
    const int node_cap = cfg->node_cap > 0 ? cfg->node_cap : cfg->sims * (max_plies + 1) + 64;
    const long long rcap = cfg->record_cap > 0 ? cfg->record_cap : (long long)cfg->num_games * 64 * 4;
    int rc = mcts_create(&sp->m, cfg->n, cfg->num_games, node_cap, cfg->c, cfg->q_mode);
    if (!rc) rc = games_alloc(sp, cfg->num_games, cfg->n, rcap, cfg->record_visits);
    if (!rc) sp->m->d.dedup = cfg->dedup == OZ_DEDUP_OFF ? 0 : 1;
    if (!rc) sp->batch_cap = cfg->batch_cap;
    if (!rc) rc = sp->alloc(&sp->d_sims_done, cfg->num_games);
    if (!rc && hipMemset(sp->d_sims_done, 0, sizeof(int) * cfg->num_games) != hipSuccess) rc = OZ_ERR_HIP;
    if (!rc) {
        sp->gm.seed = cfg->seed; sp->gm.id_stride = cfg->game_id_stride ? cfg->game_id_stride : (uint64_t)cfg->num_games;
        sp->gm.temperature = cfg->temperature; sp->gm.e_greedy = cfg->e_greedy; sp->gm.refill = cfg->refill;
        rc = games_init(sp, cfg->first_game_id, sp->m->stream);
    }
    if (rc) {
        for (void* p : sp->allocs) hipFree(p);
        mcts_destroy(sp->m);
        delete sp;
        return rc;
    }
    *out = sp;
    return OZ_OK;
}

OZ_API int oz_selfplay_destroy(oz_selfplay* sp) {
    if (!sp) return OZ_OK;
    hipSetDevice(sp->m->device);
    hipStreamSynchronize(sp->m->stream);
    for (void* p : sp->allocs) hipFree(p);
    mcts_destroy(sp->m);
    delete sp;
    return OZ_OK;
}

// cfg.eval_cache: the engine's leaves go through the network's evaluation cache as it is NOW (oz_net_set_eval_cache may have been called,
// or called again, since the engine was created)
static void selfplay_attach_cache(oz_selfplay* sp) {
    sp->m->d.ec = (sp->cfg.eval_cache && sp->net->ec.buckets && sp->net->ec.n2 == sp->m->d.n2) ? sp->net->ec : EvalCacheDev();
}

// the move kernel of the engine as it is now, with its arguments.  agent < 0: a self-play round (capped: under the engine's playout cap; a
// staggered round is not); agent 0 / 1: that agent's move in the arena (agents.py semantics, no option but proof play).  THE list of the
// variants that exist.
typedef void (*MoveKernel)(GamesDev, MctsDev, MoveArgs);
static int move_kernel(const oz_selfplay* sp, const oz_mcts* m, int agent, bool capped, MoveKernel* k, MoveArgs* a) {
    unsigned v = 0;
    *a = MoveArgs{};
    if (agent >= 0) {
        a->arena = 1;
        v = sp->arena_proof_play[agent] ? MV_PROVEN : 0;
    } else {
        a->ms = sp->sample; a->pc = capped ? sp->cap : PlayoutCap{}; a->fp = sp->forced; a->su = sp->su; a->rs = sp->resign; a->pp = sp->pplay;
        if (sp->gumbel_on) a->gp = GumbelPlay{m->gd, sp->gumbel_log, sp->gumbel_rows, sp->gumbel_moves};
        v = (sp->proof_play && m->proofs ? MV_PROVEN : 0) | (sp->resign.r > 0 ? MV_RESIGN : 0) | (sp->su.log ? MV_SURPRISE : 0);
        if (sp->gumbel_on) v |= MV_VALUES | MV_GUMBEL;                                  // (it replaces move sampling, forced playouts and the cap)
        else if (v || sp->forced.k > 0.0 || sp->gm.log_values) v |= MV_FULL;
        else if (capped) v = MV_SAMPLE | MV_CAP;                                        // (with or without move sampling: ms.plies says)
        else if (sp->sample.plies > 0) v = MV_SAMPLE;
    }
    switch (v) {
#define OZ_M(...) case (__VA_ARGS__): *k = k_sp_move<(__VA_ARGS__)>; return OZ_OK
        OZ_M(0); OZ_M(MV_SAMPLE); OZ_M(MV_SAMPLE | MV_CAP); OZ_M(MV_FULL);
        OZ_M(MV_FULL | MV_SURPRISE); OZ_M(MV_FULL | MV_RESIGN); OZ_M(MV_FULL | MV_SURPRISE | MV_RESIGN);
        OZ_M(MV_FULL | MV_PROVEN); OZ_M(MV_FULL | MV_SURPRISE | MV_PROVEN); OZ_M(MV_FULL | MV_RESIGN | MV_PROVEN); OZ_M(MV_FULL | MV_SURPRISE | MV_RESIGN | MV_PROVEN);
        OZ_M(MV_VALUES | MV_GUMBEL); OZ_M(MV_VALUES | MV_GUMBEL | MV_SURPRISE);
        OZ_M(MV_PROVEN);                                                                // (the arena's)
#undef OZ_M
    }
    oz_set_error("no move kernel for this combination of options (variant 0x%x)", v);
    return OZ_ERR_STATE;
}

// one move round on m->stream: roots, `sims` lock-step simulations, move.  stagger_round >= 0: only slots whose start
// offset (oz_selfplay_stagger) is still ahead of that round take part.  With leaves_per_step > 1 the round synchronises the stream once (the
// 4-byte budget read-back of mcts_wide_steps): the lock-step drivers are then no longer asynchronous.
static int selfplay_round_async(oz_selfplay* sp, int sims, int stagger_round) {
    oz_mcts* m = sp->m;
    const int G = sp->gm.G;
    hipStream_t s = m->stream;
    // a playout cap holds for the rounds of oz_selfplay_run; a staggered round plays every slot at `sims`, flag 0, through the kernels it always ran
    const bool capped = sp->cap.fast_sims > 0 && stagger_round < 0;
    const CapKeys ck{sp->cap, sp->gm.seed, (const uint64_t*)sp->gm.game_id, (const int*)sp->gm.ply};
    const dim3 gg((unsigned)((G + 255) / 256));
    timed(m, TS_MOVE, m->profile, [&] {
        if (stagger_round >= 0) hipLaunchKernelGGL(k_sp_roots_stagger, gg, dim3(256), 0, s, sp->gm, m->d, stagger_round, sp->stagger_period);
        else hipLaunchKernelGGL(k_sp_roots, gg, dim3(256), 0, s, sp->gm, m->d, 0);
        if (sp->tree_gc != OZ_TREE_GC_OFF) tree_collect_async(m, sp->tree_gc, sims);      // before whoever looks the new roots up (Gumbel arming, the descents)
        if (sp->gumbel_on) hipLaunchKernelGGL(k_gumbel_arm, dim3(G), dim3(64), 0, s, m->d, m->gd, 1, sp->gm.seed, (const uint64_t*)sp->gm.game_id, (const int*)sp->gm.ply, (const uint8_t*)nullptr);
        if (sp->noise_on && capped) hipLaunchKernelGGL(k_root_noise_c, dim3(G), dim3(64), 0, s, m->d, sp->noise_alpha, ck);
        else if (sp->noise_on) hipLaunchKernelGGL(k_root_noise, dim3(G), dim3(64), 0, s, m->d, sp->noise_alpha, sp->gm.seed, (const uint64_t*)sp->gm.game_id, (const int*)sp->gm.ply);
    });
    if (capped && !m->wide()) {
        // one descent per step: the first fast_sims simulations for every game, the rest for the games whose move is full.  A game's own
        // sequence of simulations does not depend on where the call is split, nor on who else is active.
        const int fs = sp->cap.fast_sims;
        if (int rc = mcts_steps_async(m, sp->net, fs, G, true)) return rc;
        if (sims > fs) {
            hipLaunchKernelGGL(k_cap_park, gg, dim3(256), 0, s, m->d, ck);
            if (int rc = mcts_steps_async(m, sp->net, sims - fs, G, true)) return rc;
            hipLaunchKernelGGL(k_cap_resume, gg, dim3(256), 0, s, m->d, (const uint8_t*)sp->gm.finished);
        }
    } else if (int rc = mcts_steps_async(m, sp->net, sims, G, true, capped ? &ck : nullptr)) return rc;
    MoveKernel move;
    MoveArgs margs;
    if (int rc = move_kernel(sp, m, -1, capped, &move, &margs)) return rc;
    timed(m, TS_MOVE, m->profile, [&] { hipLaunchKernelGGL(move, dim3(G), dim3(64), 0, s, sp->gm, m->d, margs); });
    OZ_HIP(hipGetLastError());
    if (m->timer.backlog() > 4096) m->timer.drain();      // completed pairs only: never a host stall inside the enqueue loop
    return OZ_OK;
}

OZ_API int oz_selfplay_run(oz_selfplay* sp, int rounds) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkn(sp->net->mu);
    hipSetDevice(sp->m->device);
    OZ_REQUIRE(sp->mode != 2, "oz_selfplay_run after oz_selfplay_run_steps: moves are in progress (use one driver per engine)");
    sp->mode = 1;
    selfplay_attach_cache(sp);
    for (int r = 0; r < rounds; ++r)
        if (int rc = selfplay_round_async(sp, sp->cfg.sims, -1)) return rc;
    return OZ_OK;
}

// Spread the slots of a continuous self-play engine over the plies of a game BEFORE measuring it: a service that has been
// running for a while holds games at every stage, whereas a fresh engine holds num_games openings that would all finish in
// the same move round.  Slot g gets the start offset (g * period) / num_games, period = the longest game (n*n - 4 plies):
// in round r (r = 0 .. period-2) the slots whose offset is > r play one move with `sims_pre` simulations -- real searched
// self-play moves by the same kernels and RNG streams, recorded like any other -- the others wait.  Afterwards slot g is
// offset(g) plies into its first game, and the refills keep the spread.  Asynchronous, like oz_selfplay_run (both synchronise
// once per round when leaves_per_step > 1).
OZ_API int oz_selfplay_stagger(oz_selfplay* sp, int sims_pre) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE(sims_pre >= 2, "sims_pre must be >= 2 (the reference raises KeyError with one simulation)");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkn(sp->net->mu);
    hipSetDevice(sp->m->device);
    OZ_REQUIRE(sp->mode == 0, "oz_selfplay_stagger must be the first driver call on an engine");
    if (sp->m->proofs) { oz_set_error("oz_selfplay_stagger: not with proofs (use oz_selfplay_run)"); return OZ_ERR_STATE; }
    if (sp->m->d.sel.flags) { oz_set_error("oz_selfplay_stagger: not with the selection option (it continues on the free-running kernels; use oz_selfplay_run)"); return OZ_ERR_STATE; }
    if (sp->gumbel_on) { oz_set_error("oz_selfplay_stagger: not with the Gumbel search (its budget is num_simulations; use oz_selfplay_run)"); return OZ_ERR_STATE; }
    if (sp->resign.r > 0) { oz_set_error("oz_selfplay_stagger: not with resignation (its rounds search at sims_pre; use oz_selfplay_run)"); return OZ_ERR_STATE; }
    if (sp->tree_gc != OZ_TREE_GC_OFF) { oz_set_error("oz_selfplay_stagger: not with tree collection (it continues on the free-running kernels; use oz_selfplay_run)"); return OZ_ERR_STATE; }
    OZ_REQUIRE(sp->cfg.refill, "oz_selfplay_stagger is for continuous self-play (cfg.refill = 1)");
    sp->mode = 1;
    selfplay_attach_cache(sp);
    sp->stagger_period = sp->cfg.n * sp->cfg.n - 4;
    for (int r = 0; r + 1 < sp->stagger_period; ++r)
        if (int rc = selfplay_round_async(sp, sims_pre, r)) return rc;
    return OZ_OK;
}

OZ_API int oz_selfplay_profile(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    sp->m->profile = enable != 0;
    return OZ_OK;
}

OZ_API int oz_selfplay_profile_read(oz_selfplay* sp, double* ms_total, int64_t* launches, int reset) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    if (int rc = mcts_collect_eval_time(sp->m)) return rc;
    for (int i = 0; i < OZ_TREE_KERNELS; ++i) {
        if (ms_total) ms_total[i] = sp->m->timer.ms[i];
        if (launches) launches[i] = sp->m->timer.count[i];
    }
    if (reset) sp->m->timer.reset();
    return OZ_OK;
}

// leaf-parallel search for the lock-step drivers (oz_selfplay_run, oz_selfplay_stagger); before the first driver call
OZ_API int oz_selfplay_set_leaves_per_step(oz_selfplay* sp, int k) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = wide_check_k(k)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_leaves_per_step: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (sp->gumbel_on && k > 1) { oz_set_error("oz_selfplay_set_leaves_per_step: the Gumbel search runs one leaf per game and step"); return OZ_ERR_STATE; }
    OZ_REQUIRE(sp->net->max_batch >= sp->gm.G * k, "network max_batch %d < num_games %d x leaves_per_step %d", sp->net->max_batch, sp->gm.G, k);
    hipSetDevice(sp->m->device);
    return wide_set_k(sp->m, k);
}

// solved leaves for every search of the engine (lock-step rounds at any leaves_per_step, oz_selfplay_stagger, the free-running driver); takes
// effect at the next step
OZ_API int oz_selfplay_set_solve_leaves(oz_selfplay* sp, int max_empties) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = solve_leaves_check("oz_selfplay_set_solve_leaves", max_empties)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    return solve_leaves_set_locked(sp->m, max_empties);
}
OZ_API int oz_selfplay_get_solve_leaves(oz_selfplay* sp, int* max_empties, int64_t* rows_solved) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    return oz_mcts_get_solve_leaves(sp->m, max_empties, rows_solved);
}
// value signs of the engine's search (see oz_mcts_set_value_signs), for every driver; before the first driver call
OZ_API int oz_selfplay_set_value_signs(oz_selfplay* sp, int mode) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = value_signs_check("oz_selfplay_set_value_signs", mode)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_value_signs: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    return value_signs_set_locked(sp->m, "oz_selfplay_set_value_signs", mode);
}
// the selection rule of the engine's search (see oz_mcts_set_selection), for oz_selfplay_run; before the first driver call
OZ_API int oz_selfplay_set_selection(oz_selfplay* sp, int flags, double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = selection_check("oz_selfplay_set_selection", flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_selection: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    return selection_set_locked(sp->m, "oz_selfplay_set_selection", selection_of(flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor));
}
OZ_API int oz_selfplay_get_selection(oz_selfplay* sp, int* flags, double* fpu_reduction, double* fpu_root_reduction, double* cpuct_base, double* cpuct_factor) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    return oz_mcts_get_selection(sp->m, flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor);
}
// proofs of the engine's search (see oz_mcts_set_proofs), for oz_selfplay_run; before the first driver call
OZ_API int oz_selfplay_set_proofs(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_proofs: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (!enable && sp->proof_play) { oz_set_error("oz_selfplay_set_proofs: proof play is on and reads the proofs (oz_selfplay_set_proof_play(sp, 0) first)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    return proofs_set_locked(sp->m, "oz_selfplay_set_proofs", enable);
}
OZ_API int oz_selfplay_proof_stats(oz_selfplay* sp, int64_t* out4) {
    OZ_REQUIRE(sp && out4, "null argument");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    return proof_stats_locked(sp->m, out4);
}
// proof play of the engine's moves ("proof play" in the header), for oz_selfplay_run; on top of proofs; before the first driver call
OZ_API int oz_selfplay_set_proof_play(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE(enable == 0 || enable == 1, "oz_selfplay_set_proof_play: enable = %d (0 or 1)", enable);
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_proof_play: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (!enable) { sp->proof_play = false; return OZ_OK; }
    if (!sp->m->proofs) { oz_set_error("oz_selfplay_set_proof_play: the engine keeps no proofs (oz_selfplay_set_proofs first)"); return OZ_ERR_STATE; }
    if (!sp->pplay.stat) {
        hipSetDevice(sp->m->device);
        const size_t held = sp->allocs.size(), G = (size_t)sp->gm.G;
        uint8_t* log = nullptr; unsigned long long* stat = nullptr;
        int rc = sp->alloc(&log, G * 64);
        if (!rc) rc = sp->alloc(&stat, 4);
        if (!rc && (hipMemset(log, 0, G * 64) != hipSuccess || hipMemset(stat, 0, 4 * sizeof(unsigned long long)) != hipSuccess)) {
            oz_set_error("oz_selfplay_set_proof_play: clearing the buffers failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < sp->allocs.size(); ++i) hipFree(sp->allocs[i]);
            sp->allocs.resize(held);
            return rc;
        }
        sp->pplay.log = log; sp->pplay.stat = stat;
    }
    sp->proof_play = true;
    return OZ_OK;
}
// out4: searched moves on a proven root, moves whose row differs from the raw counts, moves whose action does, fallbacks
OZ_API int oz_selfplay_proof_play_stats(oz_selfplay* sp, int64_t* out4) {
    OZ_REQUIRE(sp && out4, "null argument");
    std::lock_guard<std::mutex> lk(sp->mu);
    unsigned long long c[4] = {0, 0, 0, 0};
    if (sp->pplay.stat) {
        hipSetDevice(sp->m->device);
        OZ_HIP(hipStreamSynchronize(sp->m->stream));
        OZ_HIP(hipMemcpy(c, sp->pplay.stat, sizeof c, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < 4; ++i) out4[i] = (int64_t)c[i];
    return OZ_OK;
}
OZ_API int oz_selfplay_get_value_signs(oz_selfplay* sp, int* mode) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    return oz_mcts_get_value_signs(sp->m, mode);
}
// HIP-event timing of the engine's k_solve_leaves launches (oz_mcts_solve_leaves_profile on the engine's search)
OZ_API int oz_selfplay_solve_leaves_profile(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    return oz_mcts_solve_leaves_profile(sp->m, enable);
}
OZ_API int oz_selfplay_solve_leaves_profile_read(oz_selfplay* sp, double* ms_total, int64_t* launches, int reset) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    return oz_mcts_solve_leaves_profile_read(sp->m, ms_total, launches, reset);
}

// tree collection for the rounds of oz_selfplay_run (see oz_mcts_collect); before the first driver call.  The free-running k_advance* family
// moves inside the kernel and would need the collection as a device call there: oz_selfplay_run_steps / oz_selfplay_stagger refuse the option.
OZ_API int oz_selfplay_set_tree_gc(oz_selfplay* sp, int mode) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = tree_gc_check("oz_selfplay_set_tree_gc", mode)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_tree_gc: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    if (mode != OZ_TREE_GC_OFF) if (int rc = tree_gc_alloc(sp->m)) return rc;
    sp->tree_gc = mode;
    return OZ_OK;
}
OZ_API int oz_selfplay_get_tree_gc(oz_selfplay* sp, int* mode, oz_tree_gc_stats* stats) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    if (mode) *mode = sp->tree_gc;
    if (stats) return tree_gc_stats_locked(sp->m, stats);
    return OZ_OK;
}
// HIP-event timing of the engine's collection launches; off, nothing is recorded
OZ_API int oz_selfplay_tree_gc_profile(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    sp->m->gc_profile = enable != 0;
    return OZ_OK;
}
OZ_API int oz_selfplay_tree_gc_profile_read(oz_selfplay* sp, double* ms_total, int64_t* launches, int reset) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    return tree_gc_profile_read_locked(sp->m, ms_total, launches, reset);
}

// root noise for every searched move of the engine (the lock-step rounds, oz_selfplay_stagger's included, and the free-running driver); before
// the first driver call
OZ_API int oz_selfplay_set_root_noise(oz_selfplay* sp, double alpha, double eps) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = noise_check("oz_selfplay_set_root_noise", alpha, eps, true)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_root_noise: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (sp->gumbel_on) { oz_set_error("oz_selfplay_set_root_noise: the Gumbel search replaces root noise (the engine has it switched on)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    hipSetDevice(sp->m->device);
    if (eps == 0.0) { sp->noise_on = false; sp->forced.k = 0.0; sp->m->d.forced_k = 0.0; return noise_disarm(sp->m); }       // (forced playouts go with the noise)
    if (int rc = noise_alloc(sp->m)) return rc;
    sp->m->d.noise_eps = eps;
    sp->noise_alpha = alpha; sp->noise_on = true;
    return OZ_OK;
}
// move sampling for the self-play moves of the engine (lock-step rounds, oz_selfplay_stagger's included, at any leaves_per_step, and the
// free-running driver); before the first driver call.  plies == 0 disarms; nothing is allocated either way.
OZ_API int oz_selfplay_set_move_sampling(oz_selfplay* sp, double temperature, int plies) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = sample_check("oz_selfplay_set_move_sampling", temperature)) return rc;
    OZ_REQUIRE(plies >= 0 && plies <= 64, "oz_selfplay_set_move_sampling: plies %d outside [0, 64]", plies);
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_move_sampling: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (sp->gumbel_on) { oz_set_error("oz_selfplay_set_move_sampling: the Gumbel search replaces move sampling (the engine has it switched on)"); return OZ_ERR_STATE; }
    sp->sample = MoveSampling{plies > 0 ? temperature : 0.0, plies};
    return OZ_OK;
}
// playout cap for the self-play moves of the engine (oz_selfplay_run at any leaves_per_step and the free-running driver; oz_selfplay_stagger's
// rounds stay at sims_pre, flag 0); before the first driver call.  fast_sims == 0 disarms.  64 B per slot at the first arming.
OZ_API int oz_selfplay_set_playout_cap(oz_selfplay* sp, int fast_sims, double full_prob) {
    OZ_REQUIRE(sp, "null selfplay");
    if (fast_sims != 0) {
        OZ_REQUIRE(fast_sims >= 2 && fast_sims <= sp->cfg.sims, "oz_selfplay_set_playout_cap: fast_sims %d outside [2, num_simulations = %d] (0 = off)", fast_sims,
                   sp->cfg.sims);
        OZ_REQUIRE(full_prob > 0.0 && full_prob <= 1.0, "oz_selfplay_set_playout_cap: full_prob %g outside (0, 1]", full_prob);       // (NaN fails both compares)
    }
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_playout_cap: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (sp->gumbel_on && fast_sims != 0) { oz_set_error("oz_selfplay_set_playout_cap: not with the Gumbel search (a cap needs two budgets and two schedules)"); return OZ_ERR_STATE; }
    if (fast_sims == 0) { sp->cap.fast_sims = 0; sp->cap.full_prob = 0.0; return OZ_OK; }
    if (!sp->cap.log_fast) {
        hipSetDevice(sp->m->device);
        const size_t held = sp->allocs.size(), G = (size_t)sp->gm.G;
        uint8_t* log_fast = nullptr; unsigned long long* moves = nullptr;
        int rc = sp->alloc(&log_fast, G * 64);
        if (!rc) rc = sp->alloc(&moves, 2);
        if (!rc && (hipMemset(log_fast, 0, G * 64) != hipSuccess || hipMemset(moves, 0, 2 * sizeof(unsigned long long)) != hipSuccess)) {
            oz_set_error("oz_selfplay_set_playout_cap: clearing the buffers failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < sp->allocs.size(); ++i) hipFree(sp->allocs[i]);
            sp->allocs.resize(held);
            return rc;
        }
        sp->cap.log_fast = log_fast; sp->cap.moves = moves;
    }
    sp->cap.fast_sims = fast_sims; sp->cap.full_prob = full_prob;
    return OZ_OK;
}
OZ_API int oz_selfplay_get_playout_cap(oz_selfplay* sp, int* fast_sims, double* full_prob, int64_t* full_moves, int64_t* fast_moves) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    if (fast_sims) *fast_sims = sp->cap.fast_sims;
    if (full_prob) *full_prob = sp->cap.full_prob;
    unsigned long long c[2] = {0, 0};
    if ((full_moves || fast_moves) && sp->cap.moves) {
        hipSetDevice(sp->m->device);
        OZ_HIP(hipStreamSynchronize(sp->m->stream));
        OZ_HIP(hipMemcpy(c, sp->cap.moves, sizeof c, hipMemcpyDeviceToHost));
    }
    if (full_moves) *full_moves = (int64_t)c[0];
    if (fast_moves) *fast_moves = (int64_t)c[1];
    return OZ_OK;
}
// forced playouts for every searched move whose root draws noise (lock-step rounds at any leaves_per_step, oz_selfplay_stagger's included, and the
// free-running driver); after oz_selfplay_set_root_noise, before the first driver call.  k == 0 switches off.  24 B at the first arming.
OZ_API int oz_selfplay_set_forced_playouts(oz_selfplay* sp, double k) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = forced_check("oz_selfplay_set_forced_playouts", k)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_forced_playouts: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (sp->gumbel_on) { oz_set_error("oz_selfplay_set_forced_playouts: the Gumbel search replaces forced playouts (the engine has it switched on)"); return OZ_ERR_STATE; }
    if (k > 0.0 && !sp->noise_on) { oz_set_error("oz_selfplay_set_forced_playouts: forced playouts need root noise (oz_selfplay_set_root_noise first)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    if (k > 0.0 && !sp->forced.stat) {
        hipSetDevice(sp->m->device);
        const size_t held = sp->allocs.size();
        unsigned long long* stat = nullptr;
        int rc = sp->alloc(&stat, 3);
        if (!rc && hipMemset(stat, 0, 3 * sizeof(unsigned long long)) != hipSuccess) {
            oz_set_error("oz_selfplay_set_forced_playouts: clearing the counters failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < sp->allocs.size(); ++i) hipFree(sp->allocs[i]);
            sp->allocs.resize(held);
            return rc;
        }
        sp->forced.stat = stat;
    }
    if (int rc = forced_set_locked(sp->m, "oz_selfplay_set_forced_playouts", k)) return rc;
    sp->forced.k = k;
    return OZ_OK;
}
OZ_API int oz_selfplay_get_forced_playouts(oz_selfplay* sp, double* k, int64_t* moves_pruned, int64_t* visits_raw, int64_t* visits_kept) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    if (k) *k = sp->forced.k;
    unsigned long long c[3] = {0, 0, 0};
    if ((moves_pruned || visits_raw || visits_kept) && sp->forced.stat) {
        hipSetDevice(sp->m->device);
        OZ_HIP(hipStreamSynchronize(sp->m->stream));
        OZ_HIP(hipMemcpy(c, sp->forced.stat, sizeof c, hipMemcpyDeviceToHost));
    }
    if (moves_pruned) *moves_pruned = (int64_t)c[0];
    if (visits_raw) *visits_raw = (int64_t)c[1];
    if (visits_kept) *visits_kept = (int64_t)c[2];
    return OZ_OK;
}
// oz_playout_budget over a batch, on the host: needs no device
OZ_API int oz_playout_budgets(uint64_t seed, const uint64_t* game_ids, const int32_t* plies, int64_t count, int sims, int fast_sims, double full_prob,
                              int32_t* out) {
    OZ_REQUIRE(count >= 0, "oz_playout_budgets: count %lld", (long long)count);
    OZ_REQUIRE(sims >= 2, "oz_playout_budgets: num_simulations %d (>= 2)", sims);
    if (fast_sims != 0) {
        OZ_REQUIRE(fast_sims >= 2 && fast_sims <= sims, "oz_playout_budgets: fast_sims %d outside [2, num_simulations = %d] (0 = off)", fast_sims, sims);
        OZ_REQUIRE(full_prob > 0.0 && full_prob <= 1.0, "oz_playout_budgets: full_prob %g outside (0, 1]", full_prob);
    }
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(game_ids && plies && out, "oz_playout_budgets: null argument");
    for (int64_t i = 0; i < count; ++i) {
        OZ_REQUIRE(plies[i] >= 0, "oz_playout_budgets: plies[%lld] = %d", (long long)i, plies[i]);
        int fast;
        out[i] = oz_playout_budget(seed, game_ids[i], (uint64_t)plies[i], sims, fast_sims, full_prob, &fast);
    }
    return OZ_OK;
}
// resignation for the self-play games of the engine (oz_selfplay_run at any leaves_per_step); after oz_selfplay_set_record_values(sp, 1), before
// the first driver call.  r == 0 disarms.  4 B per slot + 48 B at the first arming.
static int resign_check(const char* fn, double v, int r, int min_ply) {
    OZ_REQUIRE(v > 0.0 && v <= 1.0, "%s: v %g outside (0, 1]", fn, v);                              // (NaN fails both compares)
    OZ_REQUIRE(r >= 1 && r <= 8, "%s: r %d outside [1, 8]", fn, r);
    OZ_REQUIRE(min_ply >= 0 && min_ply <= 64, "%s: min_ply %d outside [0, 64]", fn, min_ply);
    return OZ_OK;
}
OZ_API int oz_selfplay_set_resign(oz_selfplay* sp, double v, int r, int min_ply, double keep_prob) {
    OZ_REQUIRE(sp, "null selfplay");
    if (r != 0) {
        if (int rc = resign_check("oz_selfplay_set_resign", v, r, min_ply)) return rc;
        OZ_REQUIRE(keep_prob >= 0.0 && keep_prob <= 1.0, "oz_selfplay_set_resign: keep_prob %g outside [0, 1]", keep_prob);
    }
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_resign: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (r == 0) { sp->resign.r = 0; return OZ_OK; }
    if (sp->gumbel_on) { oz_set_error("oz_selfplay_set_resign: not with the Gumbel search (the engine has it switched on)"); return OZ_ERR_STATE; }
    if (!sp->gm.log_values) { oz_set_error("oz_selfplay_set_resign: the rule reads recorded root values (oz_selfplay_set_record_values(sp, 1) first)"); return OZ_ERR_STATE; }
    if (!sp->resign.stat) {
        hipSetDevice(sp->m->device);
        const size_t held = sp->allocs.size(), G = (size_t)sp->gm.G;
        uint8_t* state = nullptr; unsigned long long* stat = nullptr;
        int rc = sp->alloc(&state, 4 * G);
        if (!rc) rc = sp->alloc(&stat, 6);
        if (!rc && (hipMemset(state, 0, 4 * G) != hipSuccess || hipMemset(stat, 0, 6 * sizeof(unsigned long long)) != hipSuccess)) {
            oz_set_error("oz_selfplay_set_resign: clearing the buffers failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < sp->allocs.size(); ++i) hipFree(sp->allocs[i]);
            sp->allocs.resize(held);
            return rc;
        }
        sp->resign.side = (int8_t*)state; sp->resign.streak = state + G;
        sp->resign.ex_side = (int8_t*)(state + 2 * G); sp->resign.ex_ply = state + 3 * G;
        sp->resign.stat = stat;
    }
    sp->resign.v = v; sp->resign.r = r; sp->resign.min_ply = min_ply; sp->resign.keep_prob = keep_prob;
    return OZ_OK;
}
OZ_API int oz_selfplay_get_resign(oz_selfplay* sp, double* v, int* r, int* min_ply, double* keep_prob, oz_resign_stats* stats) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    const bool on = sp->resign.r > 0;
    if (v) *v = on ? sp->resign.v : 0.0;
    if (r) *r = sp->resign.r;
    if (min_ply) *min_ply = on ? sp->resign.min_ply : 0;
    if (keep_prob) *keep_prob = on ? sp->resign.keep_prob : 0.0;
    if (stats) {
        unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
        if (sp->resign.stat) {
            hipSetDevice(sp->m->device);
            OZ_HIP(hipStreamSynchronize(sp->m->stream));
            OZ_HIP(hipMemcpy(c, sp->resign.stat, sizeof c, hipMemcpyDeviceToHost));
        }
        stats->games_adjudicated = (int64_t)c[0]; stats->adjudicated_plies_sum = (int64_t)c[1]; stats->games_exempt = (int64_t)c[2];
        stats->exempt_triggered = (int64_t)c[3]; stats->exempt_wrong = (int64_t)c[4]; stats->exempt_trigger_ply_sum = (int64_t)c[5];
    }
    return OZ_OK;
}
// oz_resign_step over whole sequences, on the host: needs no device
OZ_API int oz_resign_scan(const int8_t* players, const double* values, const int32_t* plies_per_game, int64_t games, double v, int r, int min_ply,
                          int32_t* trigger_ply, int8_t* trigger_side) {
    if (int rc = resign_check("oz_resign_scan", v, r, min_ply)) return rc;
    OZ_REQUIRE(games >= 0, "oz_resign_scan: games %lld", (long long)games);
    if (games == 0) return OZ_OK;
    OZ_REQUIRE(plies_per_game && trigger_ply && trigger_side, "oz_resign_scan: null argument");
    int64_t total = 0;
    for (int64_t g = 0; g < games; ++g) {
        OZ_REQUIRE(plies_per_game[g] >= 0, "oz_resign_scan: plies_per_game[%lld] = %d", (long long)g, plies_per_game[g]);
        total += plies_per_game[g];
    }
    OZ_REQUIRE(total == 0 || (players && values), "oz_resign_scan: null argument");
    for (int64_t i = 0; i < total; ++i) OZ_REQUIRE(players[i] == 1 || players[i] == -1, "oz_resign_scan: players[%lld] = %d", (long long)i, (int)players[i]);
    int64_t at = 0;
    for (int64_t g = 0; g < games; ++g) {
        OzResign st{0, 0};
        trigger_ply[g] = -1; trigger_side[g] = 0;
        for (int i = 0; i < plies_per_game[g]; ++i) {
            const bool trig = oz_resign_step(st, players[at + i], values[at + i], v, r, min_ply, i);
            if (trig && trigger_ply[g] < 0) { trigger_ply[g] = i; trigger_side[g] = (int8_t)st.side; }
        }
        at += plies_per_game[g];
    }
    return OZ_OK;
}
OZ_API int oz_resign_exempt(uint64_t seed, const uint64_t* game_ids, int64_t count, double keep_prob, uint8_t* out) {
    OZ_REQUIRE(keep_prob >= 0.0 && keep_prob <= 1.0, "oz_resign_exempt: keep_prob %g outside [0, 1]", keep_prob);
    OZ_REQUIRE(count >= 0, "oz_resign_exempt: count %lld", (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE(game_ids && out, "oz_resign_exempt: null argument");
    for (int64_t i = 0; i < count; ++i) out[i] = oz_resign_is_exempt(seed, game_ids[i], keep_prob) ? 1 : 0;
    return OZ_OK;
}
// the Gumbel search for every searched move of the lock-step rounds of oz_selfplay_run; before the first driver call.  The budget is the
// engine's num_simulations, the seed the engine's.  16 KB per slot + 256 B per record for the improved-policy rows at the first call.
OZ_API int oz_selfplay_set_gumbel(oz_selfplay* sp, int max_considered, double c_visit, double c_scale) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = gumbel_check("oz_selfplay_set_gumbel", max_considered, c_visit, c_scale, sp->cfg.sims)) return rc;
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_gumbel: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (sp->noise_on || sp->forced.k > 0.0) { oz_set_error("oz_selfplay_set_gumbel: the Gumbel search replaces root noise and forced playouts (the engine has them switched on)"); return OZ_ERR_STATE; }
    if (sp->sample.plies > 0) { oz_set_error("oz_selfplay_set_gumbel: the Gumbel search replaces move sampling (the engine has it switched on)"); return OZ_ERR_STATE; }
    if (sp->cap.fast_sims > 0) { oz_set_error("oz_selfplay_set_gumbel: not with a playout cap (it needs two budgets and two schedules)"); return OZ_ERR_STATE; }
    if (sp->resign.r > 0) { oz_set_error("oz_selfplay_set_gumbel: not with resignation (the engine has it armed)"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    hipSetDevice(sp->m->device);
    if (!sp->gumbel_log) {
        const size_t held = sp->allocs.size(), G = (size_t)sp->gm.G;
        float *lg = nullptr, *rows = nullptr; unsigned long long* moves = nullptr;
        int rc = sp->alloc(&lg, G * 64 * 64);
        if (!rc) rc = sp->alloc(&rows, (size_t)sp->gm.record_cap * 64);
        if (!rc) rc = sp->alloc(&moves, 1);
        if (!rc && (hipMemset(lg, 0, sizeof(float) * G * 64 * 64) != hipSuccess || hipMemset(moves, 0, sizeof(unsigned long long)) != hipSuccess)) {
            oz_set_error("oz_selfplay_set_gumbel: clearing the buffers failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < sp->allocs.size(); ++i) hipFree(sp->allocs[i]);
            sp->allocs.resize(held);
            return rc;
        }
        sp->gumbel_log = lg; sp->gumbel_rows = rows; sp->gumbel_moves = moves;
    }
    if (int rc = gumbel_enable(sp->m, "oz_selfplay_set_gumbel", max_considered, c_visit, c_scale, sp->cfg.sims)) return rc;
    sp->gumbel_on = true;
    return OZ_OK;
}
OZ_API int oz_selfplay_get_gumbel(oz_selfplay* sp, int32_t* max_considered, double* c_visit, double* c_scale, int64_t* moves) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    if (max_considered) *max_considered = sp->gumbel_on ? sp->m->gd.max_considered : 0;
    if (c_visit) *c_visit = sp->gumbel_on ? sp->m->gd.c_visit : 0.0;
    if (c_scale) *c_scale = sp->gumbel_on ? sp->m->gd.c_scale : 0.0;
    unsigned long long c = 0;
    if (moves && sp->gumbel_moves) {
        hipSetDevice(sp->m->device);
        OZ_HIP(hipStreamSynchronize(sp->m->stream));
        OZ_HIP(hipMemcpy(&c, sp->gumbel_moves, sizeof c, hipMemcpyDeviceToHost));
    }
    if (moves) *moves = (int64_t)c;
    return OZ_OK;
}
// what the last round's searches ran on: g, armed, N0 as oz_mcts_get_gumbel (zeros on an engine without the option)
OZ_API int oz_selfplay_gumbel(oz_selfplay* sp, double* g, uint8_t* armed, int32_t* N0) {
    OZ_REQUIRE(sp, "null selfplay");
    { std::lock_guard<std::mutex> lk(sp->mu); hipSetDevice(sp->m->device); OZ_HIP(hipStreamSynchronize(sp->m->stream)); }
    return oz_mcts_get_gumbel(sp->m, g, armed, N0, nullptr, nullptr, nullptr, nullptr);
}
OZ_API int oz_selfplay_root_noise(oz_selfplay* sp, double* eta, uint8_t* armed) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkm(sp->m->mu);
    hipSetDevice(sp->m->device);
    OZ_HIP(hipStreamSynchronize(sp->m->stream));
    return noise_read_locked(sp->m, eta, armed);
}

// the free-running kernels of the engine as it is now -- a call's first advance, every further batch's (the batch before backed up in the same
// launch), the closing expand + backup -- with the arguments that do not change from batch to batch.  THE list of the variants that exist:
// plain, recorded values alone, the extras, the extras with recorded surprise, each under the reference's and the sound signs; what the
// free-running driver does not run at all, oz_selfplay_run_steps refuses by name before it gets here.
struct AdvanceKernels {
    void (*advance)(GamesDev, MctsDev, int, int*, int, AdvanceArgs);
    void (*backup_advance)(GamesDev, MctsDev, int, int*, int, AdvanceArgs);
    void (*expand_backup)(MctsDev, int);
};
static int advance_kernels(const oz_selfplay* sp, AdvanceKernels* k, AdvanceArgs* a) {
    const oz_mcts* m = sp->m;
    const bool surprise = sp->su.log != nullptr;
    const bool extras = surprise || m->noise_ever || sp->sample.plies > 0 || sp->cap.fast_sims > 0;
    *a = AdvanceArgs{};
    if (extras) a->xt = SelfplayExtras{sp->noise_alpha, sp->gm.seed, sp->sample, sp->cap, sp->forced};
    if (surprise) a->su = sp->su;
    const unsigned signs = m->proofs ? OZ_VSIGNS_PROVEN : m->vsigns != OZ_VSIGNS_REFERENCE ? OZ_VSIGNS_SOUND : OZ_VSIGNS_REFERENCE;
    const unsigned v = signs | (extras ? AV_EXTRAS : 0) | (extras || sp->gm.log_values ? AV_VALUES : 0) | (surprise ? AV_SURPRISE : 0);
    switch (v) {
#define OZ_A(...) \
    case (__VA_ARGS__): *k = AdvanceKernels{k_advance<(__VA_ARGS__)>, k_backup_advance<(__VA_ARGS__)>, k_expand_backup<(__VA_ARGS__) & AV_SIGNS>}; return OZ_OK
        OZ_A(OZ_VSIGNS_REFERENCE); OZ_A(OZ_VSIGNS_REFERENCE | AV_VALUES); OZ_A(OZ_VSIGNS_REFERENCE | AV_EXTRAS | AV_VALUES);
        OZ_A(OZ_VSIGNS_REFERENCE | AV_EXTRAS | AV_VALUES | AV_SURPRISE);
        OZ_A(OZ_VSIGNS_SOUND); OZ_A(OZ_VSIGNS_SOUND | AV_VALUES); OZ_A(OZ_VSIGNS_SOUND | AV_EXTRAS | AV_VALUES);
        OZ_A(OZ_VSIGNS_SOUND | AV_EXTRAS | AV_VALUES | AV_SURPRISE);
#undef OZ_A
    }
    oz_set_error("oz_selfplay_run_steps: the free-running driver has no kernels for this combination of options (variant 0x%x); use oz_selfplay_run", v);
    return OZ_ERR_STATE;
}

OZ_API int oz_selfplay_run_steps(oz_selfplay* sp, int steps) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->m->leaves_per_step > 1) {
        oz_set_error("oz_selfplay_run_steps: the free-running driver runs one leaf per game and batch (leaves_per_step is %d); use oz_selfplay_run", sp->m->leaves_per_step);
        return OZ_ERR_STATE;
    }
    if (sp->gumbel_on) { oz_set_error("oz_selfplay_run_steps: the free-running driver does not run the Gumbel search; use oz_selfplay_run"); return OZ_ERR_STATE; }
    if (sp->m->proofs) { oz_set_error("oz_selfplay_run_steps: the free-running driver keeps no proofs; use oz_selfplay_run"); return OZ_ERR_STATE; }
    if (sp->m->d.sel.flags) { oz_set_error("oz_selfplay_run_steps: the free-running kernels have no selection instantiation; use oz_selfplay_run"); return OZ_ERR_STATE; }
    if (sp->resign.r > 0) { oz_set_error("oz_selfplay_run_steps: the free-running driver does not resign games; use oz_selfplay_run"); return OZ_ERR_STATE; }
    if (sp->tree_gc != OZ_TREE_GC_OFF) { oz_set_error("oz_selfplay_run_steps: the free-running driver moves inside its kernels and does not collect the tree; use oz_selfplay_run"); return OZ_ERR_STATE; }
    std::lock_guard<std::mutex> lkn(sp->net->mu);
    oz_mcts* m = sp->m;
    hipSetDevice(m->device);
    MctsDev& d = m->d;
    if (sp->mode == 1) OZ_HIP(hipMemsetAsync(d.leaf_status, 0, sizeof(int) * d.G, m->stream));    // no simulation is pending after whole rounds
    if (sp->mode == 1 && m->noise_ever) OZ_HIP(hipMemsetAsync(d.noise_armed, 0, (size_t)d.G, m->stream));     // ... and the last round's noise is that of the roots before its moves
    sp->mode = 2;
    selfplay_attach_cache(sp);
    AdvanceKernels ak;
    AdvanceArgs aargs;
    if (int rc = advance_kernels(sp, &ak, &aargs)) return rc;
    for (int i = 0; i < steps; ++i) {
        const bool all = m->profile;
        hipStream_t s = m->stream;
        // under a batch cap the leaves on offer exceed the slots anyway (waiting games re-offer theirs), so one descent per game and call is
        // enough to keep the batches full and the launch is as short as the lock-step one (measured: +1.2 % expansions/s, +3 % games/s over 2)
        const int adv_cap = (sp->batch_cap > 0 && sp->batch_cap < d.G ? 1 : OZ_ADVANCE_CAP);
        // (from the second batch of a call on, the previous batch's expand + backup rides in the same launch; one closing k_expand_backup per call)
        timed(m, TS_SELECT, all, [&] { hipLaunchKernelGGL(i == 0 ? ak.advance : ak.backup_advance, dim3(d.G), dim3(64), 0, s, sp->gm, d, sp->cfg.sims, sp->d_sims_done, adv_cap, aargs); });
        MctsDev dc = d;                                    // this batch's cap and slot order (the kernels take the struct by value)
        const int cap = sp->batch_cap > 0 && sp->batch_cap < d.G ? sp->batch_cap : 0;
        dc.batch_cap = cap;
        dc.batch_rot = cap ? (int)((sp->batch_no * (long long)cap) % d.G) : 0;
        sp->batch_no += 1;
        timed(m, TS_COMPACT, all, [&] { hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, s, dc); });
        // (the network's launches are sized for the cap: it picks its tile shapes from the batch it is asked to hold)
        if (int rc = eval_batch_async(m, sp->net, cap ? cap : d.G, true)) return rc;
        if (i == steps - 1) timed(m, TS_BACKUP, all, [&] { hipLaunchKernelGGL(ak.expand_backup, dim3(d.G), dim3(64), 0, s, d, 0); });
        OZ_HIP(hipGetLastError());
        if (m->timer.backlog() > 4096) m->timer.drain();      // completed pairs only: never a host stall inside the enqueue loop
    }
    return OZ_OK;
}

OZ_API int oz_selfplay_set_batch_cap(oz_selfplay* sp, int cap) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    OZ_REQUIRE(cap >= 0, "oz_selfplay_set_batch_cap: cap %d", cap);
    OZ_REQUIRE(cap == 0 || cap >= 8, "oz_selfplay_set_batch_cap: a cap below 8 leaves (got %d)", cap);
    sp->batch_cap = cap;
    return OZ_OK;
}

OZ_API int oz_selfplay_set_dedup(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    sp->m->d.dedup = enable ? 1 : 0;
    return OZ_OK;
}

OZ_API int oz_selfplay_sync(oz_selfplay* sp) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    if (int rc = check_error_flag(sp->m)) return rc;
    if (int rc = mcts_collect_eval_time(sp->m)) return rc;
    std::lock_guard<std::mutex> lkn(sp->net->mu);
    return sp->net->check();
}

OZ_API int oz_selfplay_get_stats(oz_selfplay* sp, oz_selfplay_stats* out) {
    OZ_REQUIRE(sp && out, "null argument");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    int64_t s5[OZ_NSTAT];
    if (int rc = mcts_stats_locked(sp->m, s5)) return rc;
    unsigned long long c[4];
    OZ_HIP(hipMemcpy(c, sp->gm.counters, sizeof c, hipMemcpyDeviceToHost));
    std::vector<uint8_t> fin(sp->gm.G);
    OZ_HIP(hipMemcpy(fin.data(), sp->gm.finished, sp->gm.G, hipMemcpyDeviceToHost));
    int ef = 0;
    OZ_HIP(hipMemcpy(&ef, sp->m->d.error_flag, 4, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->simulations = s5[ST_SIMS]; out->node_visits = s5[ST_VISITS]; out->expansions = s5[ST_EXPAND];
    out->terminal_hits = s5[ST_TERMINAL]; out->fallbacks = s5[ST_FALLBACK];
    out->records = (int64_t)c[0]; out->games_completed = (int64_t)c[1]; out->moves = (int64_t)c[2];
    int live = 0;
    for (uint8_t f : fin) live += f ? 0 : 1;
    out->live_games = live; out->overflow = ef;
    unsigned long long ev = 0;
    OZ_HIP(hipMemcpy(&ev, sp->m->d.eval_leaves, sizeof ev, hipMemcpyDeviceToHost));
    out->leaves_evaluated = (int64_t)ev;
    return OZ_OK;
}

OZ_API int oz_selfplay_state(oz_selfplay* sp, uint64_t* black, uint64_t* white, int8_t* player, uint8_t* finished,
                             int32_t* ply, uint64_t* game_id) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    OZ_HIP(hipStreamSynchronize(sp->m->stream));
    const int G = sp->gm.G;
    if (black) OZ_HIP(hipMemcpy(black, sp->gm.black, 8ull * G, hipMemcpyDeviceToHost));
    if (white) OZ_HIP(hipMemcpy(white, sp->gm.white, 8ull * G, hipMemcpyDeviceToHost));
    if (player) OZ_HIP(hipMemcpy(player, sp->gm.player, G, hipMemcpyDeviceToHost));
    if (finished) OZ_HIP(hipMemcpy(finished, sp->gm.finished, G, hipMemcpyDeviceToHost));
    if (ply) OZ_HIP(hipMemcpy(ply, sp->gm.ply, 4ull * G, hipMemcpyDeviceToHost));
    if (game_id) OZ_HIP(hipMemcpy(game_id, sp->gm.game_id, 8ull * G, hipMemcpyDeviceToHost));
    return OZ_OK;
}

// rows of `src` (`width` bytes each, ring index = record index): the records or the visit-count rows
static int selfplay_rows(oz_selfplay* sp, const void* src, size_t width, void* dst, int64_t max_records, int64_t* written, hipMemcpyKind kind) {
    OZ_REQUIRE(sp && written, "null argument");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    OZ_HIP(hipStreamSynchronize(sp->m->stream));
    unsigned long long total = 0;
    OZ_HIP(hipMemcpy(&total, sp->gm.counters, 8, hipMemcpyDeviceToHost));
    long long n = (long long)total;
    if (n > sp->gm.record_cap) n = sp->gm.record_cap;
    if (n > max_records) n = max_records;
    if (n > 0) {
        OZ_REQUIRE(dst, "null destination");
        OZ_HIP(hipMemcpy(dst, src, width * (size_t)n, kind));
    }
    *written = n;
    return OZ_OK;
}
OZ_API int oz_selfplay_records(oz_selfplay* sp, oz_record* out, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    return selfplay_rows(sp, sp->gm.records, sizeof(oz_record), out, max_records, written, hipMemcpyDeviceToHost);
}
OZ_API int oz_selfplay_records_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    return selfplay_rows(sp, sp->gm.records, sizeof(oz_record), dst_device, max_records, written, hipMemcpyDeviceToDevice);
}
int oz_selfplay_replay_facts(oz_selfplay* sp, int* n, int* device, int* record_visits, int64_t* completed) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    OZ_HIP(hipStreamSynchronize(sp->m->stream));
    unsigned long long total = 0;
    OZ_HIP(hipMemcpy(&total, sp->gm.counters, 8, hipMemcpyDeviceToHost));
    *n = sp->gm.n; *device = sp->m->device; *record_visits = sp->gm.record_visits;
    *completed = (long long)total > sp->gm.record_cap ? sp->gm.record_cap : (int64_t)total;
    return OZ_OK;
}
int oz_selfplay_has_gumbel(oz_selfplay* sp) { std::lock_guard<std::mutex> lk(sp->mu); return sp->gumbel_on ? 1 : 0; }
#define OZ_REQUIRE_GUMBEL(sp) OZ_REQUIRE((sp)->gumbel_on, "this engine does not run the Gumbel search: oz_selfplay_set_gumbel before the first driver call")
// the float32 improved-policy row of every recorded move, by square: row i belongs to record i of oz_selfplay_records, the same ring order
OZ_API int oz_selfplay_policies(oz_selfplay* sp, float* out, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_GUMBEL(sp);
    return selfplay_rows(sp, sp->gumbel_rows, 64 * sizeof(float), out, max_records, written, hipMemcpyDeviceToHost);
}
OZ_API int oz_selfplay_policies_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_GUMBEL(sp);
    return selfplay_rows(sp, sp->gumbel_rows, 64 * sizeof(float), dst_device, max_records, written, hipMemcpyDeviceToDevice);
}
#define OZ_REQUIRE_VISITS(sp) OZ_REQUIRE((sp)->gm.record_visits, "this engine does not record visit counts: create it with oz_selfplay_config.record_visits = 1")
OZ_API int oz_selfplay_visits(oz_selfplay* sp, int32_t* out, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_VISITS(sp);
    return selfplay_rows(sp, sp->gm.visits, 64 * sizeof(int32_t), out, max_records, written, hipMemcpyDeviceToHost);
}
OZ_API int oz_selfplay_visits_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_VISITS(sp);
    return selfplay_rows(sp, sp->gm.visits, 64 * sizeof(int32_t), dst_device, max_records, written, hipMemcpyDeviceToDevice);
}

// ---------------------------------------------------------------- exact value targets for the endgame records (oz_solve.h)
// one 64-lane block per record: S of the board BEFORE the move; z = the sign of S for the mover (0 -> BLACK wins, as oz_record.z has it);
// acc: [0] records seen [1] solved [2] z changed [3] moves of maximal value [4] sum of S - values[action] [5] its maximum
__global__ __launch_bounds__(64) void k_solve_records(oz_record* __restrict__ recs, uint64_t valid, uint64_t corners, int n2, int max_empties,
                                                      long long* __restrict__ acc) {
    __shared__ SolveLds L;
    oz_record* rec = recs + blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t b = rec->black, w = rec->white;
    const int player = rec->player, action = rec->action, z_old = rec->z;
    const int empties = n2 - oz_popc(b | w);
    if (empties > max_empties) {
        if (lane == 0) atomicAdd((unsigned long long*)&acc[0], 1ULL);
        return;
    }
    uint64_t bests = 0;
    int S = 0;
    const int v = sv_position(L, valid, corners, lane, b, w, player, empties, &bests, &S);
    const int played = __shfl(v, action & 63, 64);
    if (lane != 0) return;
    const int z = S > 0 ? 1 : S < 0 ? -1 : player == 1 ? 1 : -1;
    if (z != z_old) rec->z = (int8_t)z;
    const int loss = played == OZ_MINIMAX_NONE ? 0 : S - played;
    atomicAdd((unsigned long long*)&acc[0], 1ULL);
    atomicAdd((unsigned long long*)&acc[1], 1ULL);
    if (z != z_old) atomicAdd((unsigned long long*)&acc[2], 1ULL);
    if (loss == 0) atomicAdd((unsigned long long*)&acc[3], 1ULL);
    else { atomicAdd((unsigned long long*)&acc[4], (unsigned long long)loss); atomicMax(&acc[5], (long long)loss); }
}

OZ_API int oz_selfplay_solve_records(oz_selfplay* sp, int64_t first_record, int max_empties, oz_endgame_stats* stats) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE(max_empties >= 1 && max_empties <= OZ_SOLVE_MAX_EMPTIES, "oz_selfplay_solve_records: max_empties %d outside 1..%d", max_empties, OZ_SOLVE_MAX_EMPTIES);
    OZ_REQUIRE(first_record >= 0, "oz_selfplay_solve_records: first_record %lld", (long long)first_record);
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->m->selected) { oz_set_error("oz_selfplay_solve_records: a step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; }
    hipSetDevice(sp->m->device);
    hipStream_t s = sp->m->stream;
    OZ_HIP(hipStreamSynchronize(s));
    unsigned long long total = 0;
    OZ_HIP(hipMemcpy(&total, sp->gm.counters, 8, hipMemcpyDeviceToHost));
    long long have = (long long)total > sp->gm.record_cap ? sp->gm.record_cap : (long long)total;
    const long long count = have > first_record ? have - first_record : 0;
    OZ_REQUIRE(count < (1ll << 31), "too many records in one call");
    long long acc[6] = {0, 0, 0, 0, 0, 0};
    if (count > 0) {
        if (!sp->d_endgame) { if (int rc = sp->alloc(&sp->d_endgame, 6)) return rc; }
        OZ_HIP(hipMemsetAsync(sp->d_endgame, 0, sizeof acc, s));
        const int n = sp->gm.n;
        hipLaunchKernelGGL(k_solve_records, dim3((unsigned)count), dim3(64), 0, s, sp->gm.records + first_record, sp->gm.valid, oz_solve_corners(n),
                           n * n, max_empties, sp->d_endgame);
        OZ_HIP(hipGetLastError());
        OZ_HIP(hipMemcpyAsync(acc, sp->d_endgame, sizeof acc, hipMemcpyDeviceToHost, s));
        OZ_HIP(hipStreamSynchronize(s));
    }
    if (stats) {
        stats->records = acc[0]; stats->solved = acc[1]; stats->z_changed = acc[2]; stats->optimal_moves = acc[3];
        stats->disc_loss_sum = acc[4]; stats->disc_loss_max = (int32_t)acc[5]; stats->pad = 0;
    }
    return OZ_OK;
}

// ---------------------------------------------------------------- value targets from the search ("value targets" in the header)
// root values of the engine's searched moves: [G][64 plies] of the games in progress and one double per record.  Before the first driver call.
OZ_API int oz_selfplay_set_record_values(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE(enable == 0 || enable == 1, "oz_selfplay_set_record_values: enable = %d (0 or 1)", enable);
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_record_values: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    if (!enable && sp->resign.r > 0) { oz_set_error("oz_selfplay_set_record_values: resignation is armed and reads the root values (disarm it first)"); return OZ_ERR_STATE; }
    if (enable && !sp->val_log) {
        hipSetDevice(sp->m->device);
        const size_t held = sp->allocs.size(), G = (size_t)sp->gm.G, cap = (size_t)sp->gm.record_cap;
        double *val_log = nullptr, *val_rec = nullptr;
        int rc = sp->alloc(&val_log, G * 64);
        if (!rc) rc = sp->alloc(&val_rec, cap);
        if (!rc && (hipMemset(val_log, 0, 8 * G * 64) != hipSuccess || hipMemset(val_rec, 0, 8 * (cap ? cap : 1)) != hipSuccess)) {
            oz_set_error("oz_selfplay_set_record_values: clearing the buffers failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < sp->allocs.size(); ++i) hipFree(sp->allocs[i]);
            sp->allocs.resize(held);
            return rc;
        }
        sp->val_log = val_log; sp->val_rec = val_rec;
    }
    sp->gm.log_values = enable ? sp->val_log : nullptr;
    sp->gm.values = enable ? sp->val_rec : nullptr;
    return OZ_OK;
}
#define OZ_REQUIRE_VALUES(sp) OZ_REQUIRE((sp)->gm.values, "this engine does not record root values: call oz_selfplay_set_record_values(sp, 1) before the first driver call")
OZ_API int oz_selfplay_values(oz_selfplay* sp, double* out, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_VALUES(sp);
    return selfplay_rows(sp, sp->gm.values, sizeof(double), out, max_records, written, hipMemcpyDeviceToHost);
}
OZ_API int oz_selfplay_values_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_VALUES(sp);
    return selfplay_rows(sp, sp->gm.values, sizeof(double), dst_device, max_records, written, hipMemcpyDeviceToDevice);
}

// One wavefront per record i of [first, have).  Lane l loads record i + l: a game's records are contiguous and ascending in ply, so the
// game ends before the first lane l >= 1 whose record has ply 0 or another game id, or lies past the range (a game has at most 60 plies:
// the end is always inside the wave).  TD: the recurrence runs backwards from there over the lanes' (p z, p q, exact), every lane the
// same steps (oz_value_target_td_step); lane 0 stores.  acc: [0] records [1] exact [2] sign(t) != z.  exact_proven: a record with a proof
// code (pad[2] != 0, "proof play" in the header) is exact too -- its z is the proven sign once oz_selfplay_proof_targets has run.
__global__ __launch_bounds__(64) void k_value_targets(const oz_record* __restrict__ recs, const double* __restrict__ values, long long first, long long have,
                                                      int n2, int mode, double om, double param, int exact_empties, int exact_proven,
                                                      float* __restrict__ targets, long long* __restrict__ acc) {
    const int lane = threadIdx.x;
    const long long i = first + blockIdx.x, j = i + lane;
    const bool in = j < have;
    uint64_t gid = 0, black = 0, white = 0;
    int ply = 0, p = 1, z = 1, code = 0;
    double q = 0.0;
    if (in) {
        const oz_record* r = recs + j;
        gid = r->game_id; black = r->black; white = r->white; ply = r->ply; p = r->player; z = r->z; code = r->pad[2];
        q = values[j];
    }
    const uint64_t gid0 = uni64(gid);
    const uint64_t stop = __ballot(lane >= 1 && (!in || ply == 0 || gid != gid0));
    const int T = stop ? oz_ctz(stop) : 64;                       // records from i to the end of its game
    const bool exact = oz_value_target_exact(black, white, n2, exact_empties) || (exact_proven && code != 0);
    const double pz = (double)(p * z), pq = (double)p * q;
    double t;
    if (mode == OZ_VALUE_TARGET_TD) {
        double B = __shfl(pz, T - 1, 64);
        for (int k = T - 1; k >= 0; --k) {
            const double kpz = __shfl(pz, k, 64), kpq = __shfl(pq, k, 64);
            const int kex = __shfl((int)exact, k, 64);
            B = kex ? kpz : oz_value_target_td_step(kpq, B, om, param);
        }
        t = (double)p * B;
    } else if (mode == OZ_VALUE_TARGET_BLEND) {
        t = exact ? (double)z : oz_value_target_blend((double)z, q, om, param);
    } else t = (double)z;
    if (lane != 0) return;
    const float t32 = (float)t;
    targets[i] = t32;
    const int sgn = t32 > 0.f ? 1 : t32 < 0.f ? -1 : 0;
    atomicAdd((unsigned long long*)&acc[0], 1ULL);
    if (exact) atomicAdd((unsigned long long*)&acc[1], 1ULL);
    if (sgn != z) atomicAdd((unsigned long long*)&acc[2], 1ULL);
}

static int value_target_check(const char* fn, int mode, double param, int exact_empties) {
    OZ_REQUIRE(mode == OZ_VALUE_TARGET_OUTCOME || mode == OZ_VALUE_TARGET_BLEND || mode == OZ_VALUE_TARGET_TD, "%s: mode = %d (OZ_VALUE_TARGET_*)", fn, mode);
    OZ_REQUIRE(mode == OZ_VALUE_TARGET_OUTCOME || (param >= 0.0 && param <= 1.0), "%s: parameter %g outside [0, 1]", fn, param);      // (NaN fails both compares)
    OZ_REQUIRE(exact_empties >= 0 && exact_empties <= OZ_SOLVE_MAX_EMPTIES, "%s: exact_empties %d outside 0..%d", fn, exact_empties, OZ_SOLVE_MAX_EMPTIES);
    return OZ_OK;
}

static int selfplay_value_targets(const char* fn, oz_selfplay* sp, int64_t first_record, int mode, double param, int exact_empties, int exact_proven,
                                  oz_value_target_stats* stats) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = value_target_check(fn, mode, param, exact_empties)) return rc;
    OZ_REQUIRE(exact_proven == 0 || exact_proven == 1, "%s: exact_proven = %d (0 or 1)", fn, exact_proven);
    OZ_REQUIRE(first_record >= 0, "%s: first_record %lld", fn, (long long)first_record);
    std::lock_guard<std::mutex> lk(sp->mu);
    OZ_REQUIRE_VALUES(sp);
    if (sp->m->selected) { oz_set_error("%s: a step is pending (oz_mcts_select without oz_mcts_backup)", fn); return OZ_ERR_STATE; }
    hipSetDevice(sp->m->device);
    hipStream_t s = sp->m->stream;
    OZ_HIP(hipStreamSynchronize(s));
    unsigned long long total = 0;
    OZ_HIP(hipMemcpy(&total, sp->gm.counters, 8, hipMemcpyDeviceToHost));
    const long long have = (long long)total > sp->gm.record_cap ? sp->gm.record_cap : (long long)total;
    const long long count = have > first_record ? have - first_record : 0;
    OZ_REQUIRE(count < (1ll << 31), "too many records in one call");
    if (!sp->targets) {
        if (int rc = sp->alloc(&sp->targets, (size_t)sp->gm.record_cap)) return rc;
        OZ_HIP(hipMemsetAsync(sp->targets, 0, sizeof(float) * (size_t)(sp->gm.record_cap ? sp->gm.record_cap : 1), s));
    }
    long long acc[3] = {0, 0, 0};
    if (count > 0) {
        if (!sp->d_vt) { if (int rc = sp->alloc(&sp->d_vt, 3)) return rc; }
        OZ_HIP(hipMemsetAsync(sp->d_vt, 0, sizeof acc, s));
        const int n = sp->gm.n;
        const double om = 1.0 - param;
        hipLaunchKernelGGL(k_value_targets, dim3((unsigned)count), dim3(64), 0, s, sp->gm.records, sp->gm.values, (long long)first_record, have, n * n, mode, om,
                           param, exact_empties, exact_proven, sp->targets, sp->d_vt);
        OZ_HIP(hipGetLastError());
        OZ_HIP(hipMemcpyAsync(acc, sp->d_vt, sizeof acc, hipMemcpyDeviceToHost, s));
    }
    OZ_HIP(hipStreamSynchronize(s));
    if (stats) { stats->records = acc[0]; stats->exact = acc[1]; stats->sign_changed = acc[2]; }
    return OZ_OK;
}
OZ_API int oz_selfplay_value_targets(oz_selfplay* sp, int64_t first_record, int mode, double param, int exact_empties, oz_value_target_stats* stats) {
    return selfplay_value_targets("oz_selfplay_value_targets", sp, first_record, mode, param, exact_empties, 0, stats);
}
// ... with exact_proven = 1 a record that carries a proof code is exact as well (run oz_selfplay_proof_targets first: z is then the proven sign)
OZ_API int oz_selfplay_value_targets_x(oz_selfplay* sp, int64_t first_record, int mode, double param, int exact_empties, int exact_proven,
                                       oz_value_target_stats* stats) {
    return selfplay_value_targets("oz_selfplay_value_targets_x", sp, first_record, mode, param, exact_empties, exact_proven, stats);
}
#define OZ_REQUIRE_TARGETS(sp) OZ_REQUIRE((sp)->targets, "this engine holds no value targets: call oz_selfplay_value_targets first")
OZ_API int oz_selfplay_targets(oz_selfplay* sp, float* out, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_TARGETS(sp);
    return selfplay_rows(sp, sp->targets, sizeof(float), out, max_records, written, hipMemcpyDeviceToHost);
}
OZ_API int oz_selfplay_targets_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_TARGETS(sp);
    return selfplay_rows(sp, sp->targets, sizeof(float), dst_device, max_records, written, hipMemcpyDeviceToDevice);
}
// the same targets on the host (no device needed): records in any order, grouped by game id and sorted by ply
static int host_value_targets(const char* fn, const oz_record* records, const double* values, int64_t R, int n, int mode, double param, int exact_empties,
                              int exact_proven, float* out) {
    if (int rc = value_target_check(fn, mode, param, exact_empties)) return rc;
    OZ_REQUIRE(exact_proven == 0 || exact_proven == 1, "%s: exact_proven = %d (0 or 1)", fn, exact_proven);
    OZ_REQUIRE(n == 4 || n == 6 || n == 8, "%s: board size must be 4, 6 or 8 (got %d)", fn, n);
    OZ_REQUIRE(R >= 0, "%s: R %lld", fn, (long long)R);
    if (R == 0) return OZ_OK;
    OZ_REQUIRE(records && values && out, "%s: null argument", fn);
    std::vector<int64_t> order((size_t)R);
    for (int64_t i = 0; i < R; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [records](int64_t a, int64_t b) {
        return records[a].game_id != records[b].game_id ? records[a].game_id < records[b].game_id : records[a].ply < records[b].ply;
    });
    const double om = 1.0 - param;
    const int n2 = n * n;
    for (int64_t lo = 0; lo < R;) {
        int64_t hi = lo + 1;
        while (hi < R && records[order[(size_t)hi]].game_id == records[order[(size_t)lo]].game_id) ++hi;
        const oz_record& last = records[order[(size_t)hi - 1]];
        double B = (double)(last.player * last.z);
        for (int64_t k = hi - 1; k >= lo; --k) {
            const int64_t ix = order[(size_t)k];
            const oz_record& r = records[ix];
            const bool exact = oz_value_target_exact(r.black, r.white, n2, exact_empties) || (exact_proven && r.pad[2] != 0);
            const double z = (double)r.z, p = (double)r.player, q = values[ix];
            double t = z;
            if (mode == OZ_VALUE_TARGET_TD) {
                B = exact ? (double)(r.player * r.z) : oz_value_target_td_step(p * q, B, om, param);
                t = p * B;
            } else if (mode == OZ_VALUE_TARGET_BLEND && !exact) t = oz_value_target_blend(z, q, om, param);
            out[ix] = (float)t;
        }
        lo = hi;
    }
    return OZ_OK;
}
OZ_API int oz_value_targets(const oz_record* records, const double* values, int64_t R, int n, int mode, double param, int exact_empties, float* out) {
    return host_value_targets("oz_value_targets", records, values, R, n, mode, param, exact_empties, 0, out);
}
OZ_API int oz_value_targets_x(const oz_record* records, const double* values, int64_t R, int n, int mode, double param, int exact_empties,
                              int exact_proven, float* out) {
    return host_value_targets("oz_value_targets_x", records, values, R, n, mode, param, exact_empties, exact_proven, out);
}

// ---------------------------------------------------------------- proof targets ("proof play" in the header)
// one 64-lane block per record, in place, like k_solve_records: a record with a proof code gets z = the proven sign for its mover (a draw: BLACK's
// win, as oz_record.z has it).  Idempotent.  acc: [0] records seen [1] proven [2] z changed
__global__ __launch_bounds__(64) void k_proof_targets(oz_record* __restrict__ recs, long long* __restrict__ acc) {
    if (threadIdx.x != 0) return;
    oz_record* rec = recs + blockIdx.x;
    const int code = rec->pad[2], player = rec->player, z_old = rec->z;
    atomicAdd((unsigned long long*)&acc[0], 1ULL);
    if (code == 0) return;
    const int z = oz_proof_code_z(code, player);
    if (z != z_old) rec->z = (int8_t)z;
    atomicAdd((unsigned long long*)&acc[1], 1ULL);
    if (z != z_old) atomicAdd((unsigned long long*)&acc[2], 1ULL);
}
OZ_API int oz_selfplay_proof_targets(oz_selfplay* sp, int64_t first_record, oz_proof_target_stats* stats) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE(first_record >= 0, "oz_selfplay_proof_targets: first_record %lld", (long long)first_record);
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->m->selected) { oz_set_error("oz_selfplay_proof_targets: a step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; }
    hipSetDevice(sp->m->device);
    hipStream_t s = sp->m->stream;
    OZ_HIP(hipStreamSynchronize(s));
    unsigned long long total = 0;
    OZ_HIP(hipMemcpy(&total, sp->gm.counters, 8, hipMemcpyDeviceToHost));
    const long long have = (long long)total > sp->gm.record_cap ? sp->gm.record_cap : (long long)total;
    const long long count = have > first_record ? have - first_record : 0;
    OZ_REQUIRE(count < (1ll << 31), "too many records in one call");
    long long acc[3] = {0, 0, 0};
    if (count > 0) {
        if (!sp->d_pt) { if (int rc = sp->alloc(&sp->d_pt, 3)) return rc; }
        OZ_HIP(hipMemsetAsync(sp->d_pt, 0, sizeof acc, s));
        hipLaunchKernelGGL(k_proof_targets, dim3((unsigned)count), dim3(64), 0, s, sp->gm.records + first_record, sp->d_pt);
        OZ_HIP(hipGetLastError());
        OZ_HIP(hipMemcpyAsync(acc, sp->d_pt, sizeof acc, hipMemcpyDeviceToHost, s));
        OZ_HIP(hipStreamSynchronize(s));
    }
    if (stats) { stats->records = acc[0]; stats->proven = acc[1]; stats->z_changed = acc[2]; }
    return OZ_OK;
}
// the same pass on the host (no device needed), in place -> stats
OZ_API int oz_proof_targets(oz_record* records, int64_t R, oz_proof_target_stats* stats) {
    OZ_REQUIRE(R >= 0, "oz_proof_targets: R %lld", (long long)R);
    OZ_REQUIRE(R == 0 || records, "oz_proof_targets: null argument");
    oz_proof_target_stats st = {0, 0, 0};
    for (int64_t i = 0; i < R; ++i) {
        oz_record& r = records[i];
        st.records += 1;
        if (r.pad[2] == 0) continue;
        OZ_REQUIRE(r.pad[2] <= 3, "oz_proof_targets: record %lld has proof code %d", (long long)i, (int)r.pad[2]);
        const int z = oz_proof_code_z(r.pad[2], r.player);
        st.proven += 1;
        if (z != r.z) { r.z = (int8_t)z; st.z_changed += 1; }
    }
    if (stats) *stats = st;
    return OZ_OK;
}

// ---------------------------------------------------------------- policy surprise weighting ("policy surprise weighting" in the header)
// surprises of the engine's searched moves: [G][64 plies] of the games in progress and one double per record.  Before the first driver call.
OZ_API int oz_selfplay_set_record_surprise(oz_selfplay* sp, int enable) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE(enable == 0 || enable == 1, "oz_selfplay_set_record_surprise: enable = %d (0 or 1)", enable);
    std::lock_guard<std::mutex> lk(sp->mu);
    if (sp->mode != 0) { oz_set_error("oz_selfplay_set_record_surprise: the engine has been driven already (set it before the first driver call)"); return OZ_ERR_STATE; }
    OZ_REQUIRE(!enable || sp->gm.record_visits || sp->gumbel_on,
               "oz_selfplay_set_record_surprise: the surprise is that of a recorded policy target: create the engine with oz_selfplay_config.record_visits = 1 or "
               "switch the Gumbel search on first (oz_selfplay_set_gumbel)");
    if (enable && !sp->sur_log) {
        hipSetDevice(sp->m->device);
        const size_t held = sp->allocs.size(), G = (size_t)sp->gm.G, cap = (size_t)sp->gm.record_cap;
        double *sur_log = nullptr, *sur_rec = nullptr;
        int rc = sp->alloc(&sur_log, G * 64);
        if (!rc) rc = sp->alloc(&sur_rec, cap);
        if (!rc && (hipMemset(sur_log, 0, 8 * G * 64) != hipSuccess || hipMemset(sur_rec, 0, 8 * (cap ? cap : 1)) != hipSuccess)) {
            oz_set_error("oz_selfplay_set_record_surprise: clearing the buffers failed");
            rc = OZ_ERR_HIP;
        }
        if (rc) {
            for (size_t i = held; i < sp->allocs.size(); ++i) hipFree(sp->allocs[i]);
            sp->allocs.resize(held);
            return rc;
        }
        sp->sur_log = sur_log; sp->sur_rec = sur_rec;
    }
    sp->su = enable ? SurprisePlay{sp->sur_log, sp->sur_rec} : SurprisePlay{nullptr, nullptr};
    return OZ_OK;
}
#define OZ_REQUIRE_SURPRISE(sp) OZ_REQUIRE((sp)->su.rec, "this engine does not record policy surprise: call oz_selfplay_set_record_surprise(sp, 1) before the first driver call")
OZ_API int oz_selfplay_surprises(oz_selfplay* sp, double* out, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_SURPRISE(sp);
    return selfplay_rows(sp, sp->su.rec, sizeof(double), out, max_records, written, hipMemcpyDeviceToHost);
}
OZ_API int oz_selfplay_surprises_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_SURPRISE(sp);
    return selfplay_rows(sp, sp->su.rec, sizeof(double), dst_device, max_records, written, hipMemcpyDeviceToDevice);
}
// the same surprises on the host (no device needed): the count rows are normalised at T = 1 as the move does, the float32 rows are widened
static int policy_surprises(const char* fn, const int32_t* N, const float* q32, const double* P, int64_t count, double* out) {
    OZ_REQUIRE(count >= 0, "%s: count %lld", fn, (long long)count);
    if (count == 0) return OZ_OK;
    OZ_REQUIRE((N || q32) && P && out, "%s: null argument", fn);
    if (N) for (int64_t i = 0; i < count * 64; ++i) OZ_REQUIRE(N[i] >= 0, "%s: N[%lld][%d] = %d", fn, (long long)(i / 64), (int)(i % 64), N[i]);
    for (int64_t i = 0; i < count; ++i) {
        double q[64], term[64];
        if (N) {
            for (int sq = 0; sq < 64; ++sq) q[sq] = (double)N[i * 64 + sq];
            const double sum = pairwise_sum(q, 64), divisor = sum == 0 ? 1.0 : sum;
            for (int sq = 0; sq < 64; ++sq) q[sq] = q[sq] / divisor;
        } else
            for (int sq = 0; sq < 64; ++sq) q[sq] = (double)q32[i * 64 + sq];
        for (int sq = 0; sq < 64; ++sq) term[sq] = oz_surprise_term(q[sq], P[i * 64 + sq]);
        out[i] = oz_surprise_sum(term);
    }
    return OZ_OK;
}
OZ_API int oz_policy_surprises(const int32_t* N, const double* P, int64_t count, double* out) {
    return policy_surprises("oz_policy_surprises", N, nullptr, P, count, out);
}
OZ_API int oz_policy_surprises_f32(const float* q, const double* P, int64_t count, double* out) {
    return policy_surprises("oz_policy_surprises_f32", nullptr, q, P, count, out);
}

// One wavefront per record i of [first, have).  The record's ply says where its game starts (a game's records are contiguous and ascending
// in ply): lane l loads record i - ply + l and belongs to the game while its game id and ply fit (a game has at most 60 plies: all of it is
// inside the wave; one cut off by record_cap ends there).  K = the game's fully searched records (pad[0] == 0), S = pairwise_sum of their
// surprises by lane = ply, zeros elsewhere; the record's weight, copy count and first symmetry: oz_surprise_weight / oz_surprise_copies
// (oz_common.h).  Lane ply stores.  acc: [0] records [1] fully searched [2] examples [3] fully searched with no copy [4] the largest count
__global__ __launch_bounds__(64) void k_surprise_weights(const oz_record* __restrict__ recs, const double* __restrict__ surprises, long long first,
                                                         long long have, double om, double frac, uint64_t weight_seed, float* __restrict__ weights,
                                                         int32_t* __restrict__ copies, uint8_t* __restrict__ first_sym, long long* __restrict__ acc) {
    __shared__ double arr[64];
    const int lane = threadIdx.x;
    const long long i = first + blockIdx.x;
    const int ply0 = unii((int)recs[i].ply);
    const uint64_t gid0 = uni64(recs[i].game_id);
    const long long j = i - ply0 + lane;
    bool in = j >= 0 && j < have, full = false;
    double s = 0.0;
    if (in) {
        const oz_record* r = recs + j;
        in = r->game_id == gid0 && (int)r->ply == lane;
        full = in && r->pad[0] == 0;
        if (full) s = surprises[j];
    }
    const int K = oz_popc(__ballot(full));
    arr[lane] = s;
    __syncthreads();
    const double S = pairwise_sum(arr, 64);
    if (lane != ply0) return;
    const uint64_t d = oz_rng(weight_seed, gid0, (uint64_t)ply0, OZ_RNG_SURPRISE);
    const float w = full ? oz_surprise_weight(s, K, S, om, frac) : 0.0f;
    const int c = full ? oz_surprise_copies(w, d) : 0;
    weights[i] = w; copies[i] = c; first_sym[i] = (uint8_t)(d & 7);
    atomicAdd((unsigned long long*)&acc[0], 1ULL);
    if (full) {
        atomicAdd((unsigned long long*)&acc[1], 1ULL);
        atomicAdd((unsigned long long*)&acc[2], (unsigned long long)c);
        if (c == 0) atomicAdd((unsigned long long*)&acc[3], 1ULL);
        atomicMax((unsigned long long*)&acc[4], (unsigned long long)c);
    }
}

static int surprise_frac_check(const char* fn, double frac) {
    OZ_REQUIRE(frac > 0.0 && frac <= 1.0, "%s: frac %g outside (0, 1]", fn, frac);          // (NaN fails both compares)
    return OZ_OK;
}

OZ_API int oz_selfplay_surprise_weights(oz_selfplay* sp, int64_t first_record, double frac, uint64_t weight_seed, oz_surprise_weight_stats* stats) {
    OZ_REQUIRE(sp, "null selfplay");
    if (int rc = surprise_frac_check("oz_selfplay_surprise_weights", frac)) return rc;
    OZ_REQUIRE(first_record >= 0, "oz_selfplay_surprise_weights: first_record %lld", (long long)first_record);
    std::lock_guard<std::mutex> lk(sp->mu);
    OZ_REQUIRE_SURPRISE(sp);
    if (sp->m->selected) { oz_set_error("oz_selfplay_surprise_weights: a step is pending (oz_mcts_select without oz_mcts_backup)"); return OZ_ERR_STATE; }
    hipSetDevice(sp->m->device);
    hipStream_t s = sp->m->stream;
    OZ_HIP(hipStreamSynchronize(s));
    unsigned long long total = 0;
    OZ_HIP(hipMemcpy(&total, sp->gm.counters, 8, hipMemcpyDeviceToHost));
    const long long have = (long long)total > sp->gm.record_cap ? sp->gm.record_cap : (long long)total;
    const long long count = have > first_record ? have - first_record : 0;
    OZ_REQUIRE(count < (1ll << 31), "too many records in one call");
    if (!sp->first_sym) {
        const size_t cap = (size_t)(sp->gm.record_cap ? sp->gm.record_cap : 1);
        if (!sp->weights) { if (int rc = sp->alloc(&sp->weights, cap)) return rc; }
        if (!sp->copies) { if (int rc = sp->alloc(&sp->copies, cap)) return rc; }
        if (int rc = sp->alloc(&sp->first_sym, cap)) return rc;
        OZ_HIP(hipMemsetAsync(sp->weights, 0, sizeof(float) * cap, s));
        OZ_HIP(hipMemsetAsync(sp->copies, 0, sizeof(int32_t) * cap, s));
        OZ_HIP(hipMemsetAsync(sp->first_sym, 0, cap, s));
    }
    long long acc[5] = {0, 0, 0, 0, 0};
    if (count > 0) {
        if (!sp->d_sw) { if (int rc = sp->alloc(&sp->d_sw, 5)) return rc; }
        OZ_HIP(hipMemsetAsync(sp->d_sw, 0, sizeof acc, s));
        const double om = 1.0 - frac;
        hipLaunchKernelGGL(k_surprise_weights, dim3((unsigned)count), dim3(64), 0, s, sp->gm.records, sp->su.rec, (long long)first_record, have, om, frac,
                           weight_seed, sp->weights, sp->copies, sp->first_sym, sp->d_sw);
        OZ_HIP(hipGetLastError());
        OZ_HIP(hipMemcpyAsync(acc, sp->d_sw, sizeof acc, hipMemcpyDeviceToHost, s));
    }
    OZ_HIP(hipStreamSynchronize(s));
    if (stats) { stats->records = acc[0]; stats->full_records = acc[1]; stats->examples = acc[2]; stats->zero_copies = acc[3]; stats->max_copies = acc[4]; }
    return OZ_OK;
}
#define OZ_REQUIRE_WEIGHTS(sp) OZ_REQUIRE((sp)->first_sym, "this engine holds no surprise weights: call oz_selfplay_surprise_weights first")
OZ_API int oz_selfplay_weights(oz_selfplay* sp, float* weights, int32_t* copies, uint8_t* first_sym, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_WEIGHTS(sp);
    OZ_REQUIRE(weights && copies && first_sym, "oz_selfplay_weights: null argument");
    if (int rc = selfplay_rows(sp, sp->weights, sizeof(float), weights, max_records, written, hipMemcpyDeviceToHost)) return rc;
    if (int rc = selfplay_rows(sp, sp->copies, sizeof(int32_t), copies, max_records, written, hipMemcpyDeviceToHost)) return rc;
    return selfplay_rows(sp, sp->first_sym, 1, first_sym, max_records, written, hipMemcpyDeviceToHost);
}
// (for the replay buffer's weighted append: the copy counts and first symmetries, device to device)
int oz_selfplay_copies_device(oz_selfplay* sp, void* copies_device, void* first_sym_device, int64_t max_records, int64_t* written) {
    OZ_REQUIRE(sp, "null selfplay");
    OZ_REQUIRE_WEIGHTS(sp);
    if (int rc = selfplay_rows(sp, sp->copies, sizeof(int32_t), copies_device, max_records, written, hipMemcpyDeviceToDevice)) return rc;
    return selfplay_rows(sp, sp->first_sym, 1, first_sym_device, max_records, written, hipMemcpyDeviceToDevice);
}
// the same weights on the host (no device needed): records in any order, grouped by game id and sorted by ply
static void surprise_order(const oz_record* records, int64_t R, std::vector<int64_t>& order) {
    order.resize((size_t)R);
    for (int64_t i = 0; i < R; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [records](int64_t a, int64_t b) {
        return records[a].game_id != records[b].game_id ? records[a].game_id < records[b].game_id : records[a].ply < records[b].ply;
    });
}
OZ_API int oz_surprise_weights(const oz_record* records, const double* surprises, int64_t R, double frac, float* w) {
    if (int rc = surprise_frac_check("oz_surprise_weights", frac)) return rc;
    OZ_REQUIRE(R >= 0, "oz_surprise_weights: R %lld", (long long)R);
    if (R == 0) return OZ_OK;
    OZ_REQUIRE(records && surprises && w, "oz_surprise_weights: null argument");
    for (int64_t i = 0; i < R; ++i) OZ_REQUIRE(records[i].ply < 64, "oz_surprise_weights: records[%lld].ply = %d", (long long)i, (int)records[i].ply);
    std::vector<int64_t> order;
    surprise_order(records, R, order);
    const double om = 1.0 - frac;
    for (int64_t lo = 0; lo < R;) {
        int64_t hi = lo + 1;
        while (hi < R && records[order[(size_t)hi]].game_id == records[order[(size_t)lo]].game_id) ++hi;
        double arr[64];
        for (int l = 0; l < 64; ++l) arr[l] = 0.0;
        int K = 0;
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t ix = order[(size_t)k];
            if (records[ix].pad[0] == 0) { ++K; arr[records[ix].ply] = surprises[ix]; }
        }
        const double S = pairwise_sum(arr, 64);
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t ix = order[(size_t)k];
            w[ix] = records[ix].pad[0] == 0 ? oz_surprise_weight(surprises[ix], K, S, om, frac) : 0.0f;
        }
        lo = hi;
    }
    return OZ_OK;
}
OZ_API int oz_surprise_copies(const oz_record* records, const float* w, int64_t R, uint64_t weight_seed, int32_t* copies, uint8_t* first_sym) {
    OZ_REQUIRE(R >= 0, "oz_surprise_copies: R %lld", (long long)R);
    if (R == 0) return OZ_OK;
    OZ_REQUIRE(records && w && copies && first_sym, "oz_surprise_copies: null argument");
    for (int64_t i = 0; i < R; ++i) {
        OZ_REQUIRE(w[i] >= 0.0f && w[i] <= 64.0f, "oz_surprise_copies: w[%lld] = %g outside [0, 64]", (long long)i, (double)w[i]);
        const uint64_t d = oz_rng(weight_seed, records[i].game_id, (uint64_t)records[i].ply, OZ_RNG_SURPRISE);
        copies[i] = oz_surprise_copies(w[i], d);
        first_sym[i] = (uint8_t)(d & 7);
    }
    return OZ_OK;
}

OZ_API int oz_selfplay_last_counts(oz_selfplay* sp, int32_t* counts) {
    OZ_REQUIRE(sp && counts, "null argument");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    OZ_HIP(hipStreamSynchronize(sp->m->stream));
    OZ_HIP(hipMemcpy(counts, sp->gm.last_counts, 4ull * sp->gm.G * 64, hipMemcpyDeviceToHost));
    return OZ_OK;
}

OZ_API int oz_selfplay_eval_time(oz_selfplay* sp, double* ms_total, int64_t* launches, int64_t* leaves) {
    OZ_REQUIRE(sp, "null selfplay");
    std::lock_guard<std::mutex> lk(sp->mu);
    hipSetDevice(sp->m->device);
    if (int rc = mcts_collect_eval_time(sp->m)) return rc;
    if (ms_total) *ms_total = sp->m->timer.ms[TS_NN];
    if (launches) *launches = sp->m->timer.count[TS_NN];
    if (leaves) {
        int64_t s5[OZ_NSTAT];
        if (int rc = mcts_stats_locked(sp->m, s5)) return rc;
        *leaves = s5[ST_EXPAND];
    }
    return OZ_OK;
}

// ================================================================ arena
struct oz_arena {
    oz_selfplay games;           // reuses the game-state arrays (games.m = agent A's search)
    oz_mcts* mb = nullptr;       // agent B's search
    oz_net *na = nullptr, *nb = nullptr;
    int sims = 0;
    std::mutex mu;
    // full move lists (arena games are not refilled): [G][128]
    uint8_t* d_actions = nullptr; int8_t* d_players = nullptr;
    int* d_nmoves = nullptr;
    int* d_movers = nullptr;     // [2] live games with BLACK / WHITE to move (k_arena_movers)
    bool started = false;        // oz_arena_run / oz_arena_run_rounds has been called
    int eval_cache = 0;          // oz_arena_set_eval_cache: the two searches look their leaves up in (and insert them into) their networks' evaluation caches
    // oz_arena_set_opponent: who moves for the colour without a network ([0] BLACK, [1] WHITE)
    int opp_kind[2] = {OZ_AGENT_RANDOM, OZ_AGENT_RANDOM}, opp_depth[2] = {1, 1}, opp_eval[2] = {OZ_MINIMAX_EVAL_DISCS, OZ_MINIMAX_EVAL_DISCS};
    OzTimer opp_timer{1};        // k_arena_minimax_move, with oz_arena_profile on
    // oz_arena_set_openings / oz_arena_set_opening_moves (the later call counts): 0 off, 1 random, 2 lists; the buffers are allocated by the setters
    int open_mode = 0, open_plies = 0;
    uint64_t open_seed = 0, open_first_id = 0;
    uint8_t* d_open_moves = nullptr;      // [G][OZ_OPENING_MAX_PLIES], list mode
    int32_t* d_open_n = nullptr;          // [G], list mode
    int32_t* d_open_plies = nullptr;      // [G] plies the opening kernel played
};

// live games per mover: counts[0] = BLACK to move, counts[1] = WHITE to move (an agent with nothing to move this round is not launched)
__global__ void k_arena_movers(GamesDev gm, int* counts) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < gm.G && !gm.finished[g];
    const uint64_t b = __ballot(live && gm.player[g] == 1), w = __ballot(live && gm.player[g] == -1);
    if ((threadIdx.x & 63) == 0) {
        if (b) atomicAdd(&counts[0], oz_popc(b));
        if (w) atomicAdd(&counts[1], oz_popc(w));
    }
}

// copies the slot's move log into the arena move list before k_sp_move overwrites nothing (log is per ply)
__global__ void k_arena_collect(GamesDev gm, uint8_t* actions, int8_t* players, int* nmoves) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= gm.G) return;
    const int k = gm.ply[g];
    nmoves[g] = k;
    for (int i = 0; i < k && i < 64; ++i) {
        actions[(size_t)g * 128 + i] = gm.log_action[(size_t)g * 64 + i];
        players[(size_t)g * 128 + i] = gm.log_player[(size_t)g * 64 + i];
    }
}

OZ_API int oz_arena_create(oz_arena** out, int n, int num_games, int sims, double c, int q_mode, uint64_t seed,
                           uint64_t first_game_id, oz_net* net_a, oz_net* net_b, int node_cap) {
    OZ_REQUIRE(out, "null argument");            // a NULL network = that colour is played by RandomOthelloAgent or by oz_arena_set_opponent's choice
    OZ_REQUIRE(sims >= 2, "num_simulations must be >= 2");
    OZ_REQUIRE((!net_a || net_a->n == n) && (!net_b || net_b->n == n), "network board size mismatch");
    OZ_REQUIRE((!net_a || net_a->max_batch >= num_games) && (!net_b || net_b->max_batch >= num_games), "network max_batch < num_games");
    oz_arena* a = new oz_arena();
    a->na = net_a; a->nb = net_b; a->sims = sims;
    const int max_plies = n * n - 4;
    // each agent searches only on its own turns: about half the plies
    const int ncap = node_cap > 0 ? node_cap : sims * (max_plies / 2 + 2) + 64;
    oz_selfplay* sp = &a->games;
    memset(&sp->cfg, 0, sizeof sp->cfg);
    sp->cfg.n = n; sp->cfg.num_games = num_games; sp->cfg.sims = sims; sp->cfg.c = c; sp->cfg.q_mode = q_mode; sp->cfg.seed = seed;
    int rc = mcts_create(&sp->m, n, num_games, ncap, c, q_mode);
    if (!rc) rc = mcts_create(&a->mb, n, num_games, ncap, c, q_mode);
    if (!rc) rc = games_alloc(sp, num_games, n, (long long)num_games * 64, 0);      // the arena keeps no visit counts
    if (!rc) {
        sp->gm.seed = seed; sp->gm.id_stride = 0; sp->gm.temperature = 0; sp->gm.e_greedy = 1.0; sp->gm.refill = 0;
        rc = games_init(sp, first_game_id, sp->m->stream);
    }
    if (!rc && hipMalloc((void**)&a->d_actions, (size_t)num_games * 128) != hipSuccess) rc = OZ_ERR_HIP;
    if (!rc && hipMalloc((void**)&a->d_players, (size_t)num_games * 128) != hipSuccess) rc = OZ_ERR_HIP;
    if (!rc && hipMalloc((void**)&a->d_nmoves, 4ull * num_games) != hipSuccess) rc = OZ_ERR_HIP;
    if (!rc && hipMalloc((void**)&a->d_movers, 8) != hipSuccess) rc = OZ_ERR_HIP;
    if (!rc && (hipMemset(a->d_actions, 0, (size_t)num_games * 128) != hipSuccess || hipMemset(a->d_players, 0, (size_t)num_games * 128) != hipSuccess)) rc = OZ_ERR_HIP;   // entries beyond n_moves read 0
    if (rc) {
        for (void* p : sp->allocs) hipFree(p);
        mcts_destroy(sp->m); mcts_destroy(a->mb);
        if (a->d_actions) hipFree(a->d_actions);
        if (a->d_players) hipFree(a->d_players);
        if (a->d_nmoves) hipFree(a->d_nmoves);
        if (a->d_movers) hipFree(a->d_movers);
        delete a;
        if (rc == OZ_ERR_HIP) oz_set_error("arena allocation failed");
        return rc;
    }
    *out = a;
    return OZ_OK;
}

OZ_API int oz_arena_destroy(oz_arena* a) {
    if (!a) return OZ_OK;
    hipSetDevice(a->games.m->device);
    hipStreamSynchronize(a->games.m->stream);
    hipStreamSynchronize(a->mb->stream);
    for (void* p : a->games.allocs) hipFree(p);
    mcts_destroy(a->games.m); mcts_destroy(a->mb);
    hipFree(a->d_actions); hipFree(a->d_players); hipFree(a->d_nmoves); hipFree(a->d_movers);
    if (a->d_open_moves) hipFree(a->d_open_moves);
    if (a->d_open_n) hipFree(a->d_open_n);
    if (a->d_open_plies) hipFree(a->d_open_plies);
    a->opp_timer.destroy();
    delete a;
    return OZ_OK;
}

OZ_API int oz_arena_run(oz_arena* a) { return oz_arena_run_rounds(a, 0); }

// counters of the two agents' searches since creation (layout of oz_mcts_stats); a RandomOthelloAgent side reads zeros
OZ_API int oz_arena_stats(oz_arena* a, int64_t* black5, int64_t* white5) {
    OZ_REQUIRE(a && black5 && white5, "null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    hipSetDevice(a->games.m->device);
    if (int rc = mcts_stats_locked(a->games.m, black5)) return rc;
    return mcts_stats_locked(a->mb, white5);
}

// cross-game leaf de-duplication of both agents' searches (default on, as everywhere in the library; results are identical either way)
OZ_API int oz_arena_set_dedup(oz_arena* a, int enable) {
    OZ_REQUIRE(a, "null arena");
    std::lock_guard<std::mutex> lk(a->mu);
    a->games.m->d.dedup = enable ? 1 : 0;
    a->mb->d.dedup = enable ? 1 : 0;
    return OZ_OK;
}
// HIP-event timing of both agents' tree kernels (slots of oz_selfplay_profile; the sums of the two searches)
OZ_API int oz_arena_profile(oz_arena* a, int enable) {
    OZ_REQUIRE(a, "null arena");
    std::lock_guard<std::mutex> lk(a->mu);
    a->games.m->profile = enable != 0;
    a->mb->profile = enable != 0;
    return OZ_OK;
}
OZ_API int oz_arena_profile_read(oz_arena* a, double* ms_total, int64_t* launches, int reset) {
    OZ_REQUIRE(a, "null arena");
    std::lock_guard<std::mutex> lk(a->mu);
    hipSetDevice(a->games.m->device);
    oz_mcts* both[2] = {a->games.m, a->mb};
    for (oz_mcts* m : both) if (int rc = mcts_collect_eval_time(m)) return rc;
    for (int i = 0; i < OZ_TREE_KERNELS; ++i) {
        if (ms_total) ms_total[i] = both[0]->timer.ms[i] + both[1]->timer.ms[i];
        if (launches) launches[i] = both[0]->timer.count[i] + both[1]->timer.count[i];
    }
    if (reset) for (oz_mcts* m : both) m->timer.reset();
    return OZ_OK;
}
// positions the two agents' networks have evaluated so far (<= expansions when boards are shared between games)
OZ_API int oz_arena_leaves_evaluated(oz_arena* a, int64_t* black, int64_t* white) {
    OZ_REQUIRE(a && black && white, "null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    hipSetDevice(a->games.m->device);
    OZ_HIP(hipStreamSynchronize(a->games.m->stream));
    unsigned long long eb = 0, ew = 0;
    OZ_HIP(hipMemcpy(&eb, a->games.m->d.eval_leaves, sizeof eb, hipMemcpyDeviceToHost));
    OZ_HIP(hipMemcpy(&ew, a->mb->d.eval_leaves, sizeof ew, hipMemcpyDeviceToHost));
    *black = (int64_t)eb; *white = (int64_t)ew;
    return OZ_OK;
}

// the persistent evaluation caches of the two networks (oz_net_set_eval_cache) serve the arena's searches too: arena games start from ONE opening
// and play deterministically, so across games, plies and steps most boards recur -- the reference's own per-search _predict_cache
// (othelo_mcts.py:13,82-88) generalised to everything that uses the network.  A hit changes no bit (a position's (pi, v) does not depend on the
// batch it is evaluated in): moves, boards and results are those of the uncached arena.  Default off, like oz_selfplay_config.eval_cache.
OZ_API int oz_arena_set_eval_cache(oz_arena* a, int enable) {
    OZ_REQUIRE(a, "null arena");
    std::lock_guard<std::mutex> lk(a->mu);
    a->eval_cache = enable ? 1 : 0;
    return OZ_OK;
}

// leaf-parallel search per agent (k_black for net_a's search, k_white for net_b's); before the first run
OZ_API int oz_arena_set_leaves_per_step(oz_arena* a, int k_black, int k_white) {
    OZ_REQUIRE(a, "null arena");
    if (int rc = wide_check_k(k_black)) return rc;
    if (int rc = wide_check_k(k_white)) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_leaves_per_step: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    const int G = a->games.gm.G;
    OZ_REQUIRE(!a->na || a->na->max_batch >= G * k_black, "BLACK network max_batch %d < num_games %d x leaves_per_step %d", a->na->max_batch, G, k_black);
    OZ_REQUIRE(!a->nb || a->nb->max_batch >= G * k_white, "WHITE network max_batch %d < num_games %d x leaves_per_step %d", a->nb->max_batch, G, k_white);
    hipSetDevice(a->games.m->device);
    if (int rc = wide_set_k(a->games.m, k_black)) return rc;
    return wide_set_k(a->mb, k_white);
}

// solved leaves per agent (black for net_a's search, white for net_b's; a colour without a network searches nothing); before the first run
OZ_API int oz_arena_set_solve_leaves(oz_arena* a, int black, int white) {
    OZ_REQUIRE(a, "null arena");
    if (int rc = solve_leaves_check("oz_arena_set_solve_leaves", black)) return rc;
    if (int rc = solve_leaves_check("oz_arena_set_solve_leaves", white)) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_solve_leaves: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    if (int rc = solve_leaves_set_locked(a->games.m, black)) return rc;
    return solve_leaves_set_locked(a->mb, white);
}
// value signs per agent (black for net_a's search, white for net_b's); before the first run
OZ_API int oz_arena_set_value_signs(oz_arena* a, int black, int white) {
    OZ_REQUIRE(a, "null arena");
    if (int rc = value_signs_check("oz_arena_set_value_signs", black)) return rc;
    if (int rc = value_signs_check("oz_arena_set_value_signs", white)) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_value_signs: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    if (int rc = value_signs_set_locked(a->games.m, "oz_arena_set_value_signs", black)) return rc;
    return value_signs_set_locked(a->mb, "oz_arena_set_value_signs", white);
}
// the selection rule of one agent's search (agent +1: BLACK, net_a's; -1: WHITE, net_b's); before the first run
OZ_API int oz_arena_set_selection(oz_arena* a, int agent, int flags, double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor) {
    OZ_REQUIRE(a, "null arena");
    OZ_REQUIRE(agent == 1 || agent == -1, "oz_arena_set_selection: agent must be +1 (BLACK) or -1 (WHITE), got %d", agent);
    if (int rc = selection_check("oz_arena_set_selection", flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor)) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_selection: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    oz_mcts* m = agent == 1 ? a->games.m : a->mb;
    std::lock_guard<std::mutex> lkm(m->mu);
    return selection_set_locked(m, "oz_arena_set_selection", selection_of(flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor));
}
// proofs per agent (black for net_a's search, white for net_b's), each on top of sound signs; before the first run
OZ_API int oz_arena_set_proofs(oz_arena* a, int black, int white) {
    OZ_REQUIRE(a, "null arena");
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_proofs: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    if ((!black && a->games.arena_proof_play[0]) || (!white && a->games.arena_proof_play[1])) {
        oz_set_error("oz_arena_set_proofs: proof play is on for that agent and reads the proofs (oz_arena_set_proof_play first)");
        return OZ_ERR_STATE;
    }
    if (int rc = proofs_set_locked(a->games.m, "oz_arena_set_proofs", black)) return rc;
    return proofs_set_locked(a->mb, "oz_arena_set_proofs", white);
}
// proof play per agent ("proof play" in the header): the agent's move is the arg-max of the row its root's proofs keep; needs that agent's
// proofs; before the first run
OZ_API int oz_arena_set_proof_play(oz_arena* a, int black, int white) {
    OZ_REQUIRE(a, "null arena");
    OZ_REQUIRE((black == 0 || black == 1) && (white == 0 || white == 1), "oz_arena_set_proof_play: black = %d, white = %d (0 or 1)", black, white);
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_proof_play: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    if ((black && !a->games.m->proofs) || (white && !a->mb->proofs)) {
        oz_set_error("oz_arena_set_proof_play: the agent keeps no proofs (oz_arena_set_proofs first)");
        return OZ_ERR_STATE;
    }
    a->games.arena_proof_play[0] = black != 0; a->games.arena_proof_play[1] = white != 0;
    return OZ_OK;
}
// tree collection of one agent's search (see oz_mcts_collect): agent +1 = BLACK (net_a), -1 = WHITE (net_b); before the first run
OZ_API int oz_arena_set_tree_gc(oz_arena* a, int agent, int mode) {
    OZ_REQUIRE(a, "null arena");
    OZ_REQUIRE(agent == 1 || agent == -1, "oz_arena_set_tree_gc: agent %d (+1 BLACK, -1 WHITE)", agent);
    if (int rc = tree_gc_check("oz_arena_set_tree_gc", mode)) return rc;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_tree_gc: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    oz_mcts* m = agent == 1 ? a->games.m : a->mb;
    std::lock_guard<std::mutex> lkm(m->mu);
    if (mode != OZ_TREE_GC_OFF) if (int rc = tree_gc_alloc(m)) return rc;
    a->games.arena_tree_gc[agent == 1 ? 0 : 1] = mode;
    return OZ_OK;
}
OZ_API int oz_arena_get_tree_gc(oz_arena* a, int agent, int* mode, oz_tree_gc_stats* stats) {
    OZ_REQUIRE(a, "null arena");
    OZ_REQUIRE(agent == 1 || agent == -1, "oz_arena_get_tree_gc: agent %d (+1 BLACK, -1 WHITE)", agent);
    std::lock_guard<std::mutex> lk(a->mu);
    oz_mcts* m = agent == 1 ? a->games.m : a->mb;
    std::lock_guard<std::mutex> lkm(m->mu);
    if (mode) *mode = a->games.arena_tree_gc[agent == 1 ? 0 : 1];
    if (stats) return tree_gc_stats_locked(m, stats);
    return OZ_OK;
}
OZ_API int oz_arena_get_solve_leaves(oz_arena* a, int64_t* rows_black, int64_t* rows_white) {
    OZ_REQUIRE(a && rows_black && rows_white, "null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    if (int rc = solve_leaves_rows_locked(a->games.m, rows_black)) return rc;
    return solve_leaves_rows_locked(a->mb, rows_white);
}

// the mover of a colour without a network (default OZ_AGENT_RANDOM = RandomOthelloAgent); before the first run
OZ_API int oz_arena_set_opponent(oz_arena* a, int side, int kind, int depth, int eval) {
    OZ_REQUIRE(a, "null arena");
    OZ_REQUIRE(side == 1 || side == -1, "oz_arena_set_opponent: side must be +1 (BLACK) or -1 (WHITE), got %d", side);
    OZ_REQUIRE(kind == OZ_AGENT_RANDOM || kind == OZ_AGENT_MINIMAX, "oz_arena_set_opponent: unknown agent kind %d", kind);
    OZ_REQUIRE(!(side == 1 ? a->na : a->nb), "oz_arena_set_opponent: %s is played by a network", side == 1 ? "BLACK" : "WHITE");
    if (kind == OZ_AGENT_MINIMAX) {
        OZ_REQUIRE(depth >= 1 && depth <= OZ_MINIMAX_MAX_DEPTH, "oz_arena_set_opponent: depth %d outside 1..%d", depth, OZ_MINIMAX_MAX_DEPTH);
        OZ_REQUIRE(eval == OZ_MINIMAX_EVAL_DISCS || eval == OZ_MINIMAX_EVAL_WEIGHTED, "oz_arena_set_opponent: unknown evaluation %d", eval);
    }
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_opponent: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    const int i = side == 1 ? 0 : 1;
    a->opp_kind[i] = kind;
    if (kind == OZ_AGENT_MINIMAX) { a->opp_depth[i] = depth; a->opp_eval[i] = eval; }
    return OZ_OK;
}
OZ_API int oz_arena_opponent_time(oz_arena* a, double* ms_total, int64_t* launches) {
    OZ_REQUIRE(a, "null arena");
    std::lock_guard<std::mutex> lk(a->mu);
    hipSetDevice(a->games.m->device);
    if (a->opp_timer.collect()) { oz_set_error("oz_arena_opponent_time: event timing failed"); return OZ_ERR_HIP; }
    if (ms_total) *ms_total = a->opp_timer.ms[0];
    if (launches) *launches = a->opp_timer.count[0];
    return OZ_OK;
}

// Openings (oz_openings.h): before the first run; plies == 0 / every n_plies == 0 plays nothing.  Random mode keeps three numbers; list mode
// replays every list on the host through the same rules the kernel runs (they are OZ_HD) and refuses what is not a game, so the kernel has no
// error path.
static int arena_openings_buffers(oz_arena* a, bool lists) {
    const int G = a->games.gm.G;
    hipSetDevice(a->games.m->device);
    if (!a->d_open_plies) {
        OZ_HIP(hipMalloc((void**)&a->d_open_plies, 4ull * G));
        OZ_HIP(hipMemset(a->d_open_plies, 0, 4ull * G));
    }
    if (lists && !a->d_open_moves) {
        OZ_HIP(hipMalloc((void**)&a->d_open_moves, (size_t)G * OZ_OPENING_MAX_PLIES));
        OZ_HIP(hipMalloc((void**)&a->d_open_n, 4ull * G));
    }
    return OZ_OK;
}
OZ_API int oz_arena_set_openings(oz_arena* a, int plies, uint64_t opening_seed, uint64_t first_opening_id) {
    OZ_REQUIRE(a, "null arena");
    OZ_REQUIRE(plies >= 0 && plies <= OZ_OPENING_MAX_PLIES, "oz_arena_set_openings: plies %d outside 0..%d", plies, OZ_OPENING_MAX_PLIES);
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_openings: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    if (plies > 0) if (int rc = arena_openings_buffers(a, false)) return rc;
    a->open_mode = plies > 0 ? 1 : 0;
    a->open_plies = plies; a->open_seed = opening_seed; a->open_first_id = first_opening_id;
    return OZ_OK;
}
OZ_API int oz_arena_set_opening_moves(oz_arena* a, const uint8_t* moves, const int32_t* n_plies) {
    OZ_REQUIRE(a && moves && n_plies, "null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->started) { oz_set_error("oz_arena_set_opening_moves: the arena has run already (set it before the first run)"); return OZ_ERR_STATE; }
    const GamesDev& gm = a->games.gm;
    const int G = gm.G;
    for (int g = 0; g < G; ++g) {
        OZ_REQUIRE(n_plies[g] >= 0 && n_plies[g] <= OZ_OPENING_MAX_PLIES, "oz_arena_set_opening_moves: game %d: n_plies %d outside 0..%d", g, n_plies[g],
                   OZ_OPENING_MAX_PLIES);
        uint64_t black, white;
        int player = 1, fin = 0;
        oz_initial_board(gm.n, black, white);
        for (int ply = 0; ply < n_plies[g]; ++ply) {
            const int sq = moves[(size_t)g * OZ_OPENING_MAX_PLIES + ply];
            OZ_REQUIRE(!fin, "oz_arena_set_opening_moves: game %d, ply %d: the game has ended before this move", g, ply);
            const uint64_t legal = oz_legal(player == 1 ? black : white, player == 1 ? white : black, gm.valid);
            OZ_REQUIRE(sq < 64 && ((legal >> sq) & 1), "oz_arena_set_opening_moves: game %d, ply %d: square %d is no legal move of %s", g, ply, sq,
                       player == 1 ? "BLACK" : "WHITE");
            oz_game_play(black, white, player, fin, sq, gm.valid);
        }
    }
    if (int rc = arena_openings_buffers(a, true)) return rc;
    OZ_HIP(hipMemcpy(a->d_open_moves, moves, (size_t)G * OZ_OPENING_MAX_PLIES, hipMemcpyHostToDevice));
    OZ_HIP(hipMemcpy(a->d_open_n, n_plies, 4ull * G, hipMemcpyHostToDevice));
    a->open_mode = 2;
    return OZ_OK;
}
// plies the opening of every game played (zeros with openings off, and before the first run)
OZ_API int oz_arena_opening_plies(oz_arena* a, int32_t* out) {
    OZ_REQUIRE(a && out, "null argument");
    std::lock_guard<std::mutex> lk(a->mu);
    const int G = a->games.gm.G;
    if (!a->d_open_plies) { memset(out, 0, 4ull * G); return OZ_OK; }
    hipSetDevice(a->games.m->device);
    OZ_HIP(hipStreamSynchronize(a->games.m->stream));
    OZ_HIP(hipMemcpy(out, a->d_open_plies, 4ull * G, hipMemcpyDeviceToHost));
    return OZ_OK;
}

// the move of the colour `side` that has no network: RandomOthelloAgent, or the minimax opponent oz_arena_set_opponent chose
static void arena_opponent_move(oz_arena* a, int side, hipStream_t s) {
    const GamesDev& gm = a->games.gm;
    const int i = side == 1 ? 0 : 1;
    if (a->opp_kind[i] == OZ_AGENT_RANDOM) {
        hipLaunchKernelGGL(k_arena_random_move, dim3((gm.G + 255) / 256), dim3(256), 0, s, gm, side);
        return;
    }
    const long long h = a->games.m->profile ? a->opp_timer.begin(0, s) : -1;
    hipLaunchKernelGGL(k_arena_minimax_move, dim3(gm.G), dim3(64), 0, s, gm, side, a->opp_depth[i], oz_minimax_eval_make(gm.n, a->opp_eval[i]));
    a->opp_timer.end(h, s);
}

OZ_API int oz_arena_run_rounds(oz_arena* a, int max_rounds_arg) {
    OZ_REQUIRE(a, "null arena");
    OZ_REQUIRE(max_rounds_arg >= 0, "oz_arena_run_rounds: max_rounds %d", max_rounds_arg);
    std::lock_guard<std::mutex> lk(a->mu);
    const bool first_run = !a->started;
    a->started = true;
    oz_selfplay* sp = &a->games;
    oz_mcts *ma = sp->m, *mb = a->mb;
    hipSetDevice(ma->device);
    if (first_run && a->open_mode) {     // the openings, once, ahead of the first round on the stream the rounds run on
        const OpeningsDev op = {a->open_mode == 1 ? a->open_plies : 0, a->open_seed, a->open_first_id, a->open_mode == 2 ? a->d_open_moves : nullptr,
                                a->d_open_n, a->d_open_plies};
        hipLaunchKernelGGL(k_arena_openings, dim3((sp->gm.G + 255) / 256), dim3(256), 0, ma->stream, sp->gm, op);
    }
    // (the caches as they are NOW: oz_net_set_eval_cache may have been called since the arena was created.  The two searches run one after
    //  the other on one stream, so even ONE network playing itself never has two users of its cache at a time.)
    ma->d.ec = (a->eval_cache && a->na && a->na->ec.buckets && a->na->ec.n2 == ma->d.n2) ? a->na->ec : EvalCacheDev();
    mb->d.ec = (a->eval_cache && a->nb && a->nb->ec.buckets && a->nb->ec.n2 == mb->d.n2) ? a->nb->ec : EvalCacheDev();
    const int G = sp->gm.G;
    hipStream_t s = ma->stream;          // both searches are driven on agent A's stream (they share game state)
    hipStream_t sb_saved = mb->stream;
    mb->stream = s;
    int rc = OZ_OK;
    // every round plays one ply in every live game (two where a RandomOthelloAgent side moves first); n*n rounds end every game
    const int max_rounds = max_rounds_arg > 0 && max_rounds_arg < sp->gm.n * sp->gm.n ? max_rounds_arg : sp->gm.n * sp->gm.n;
    std::vector<uint8_t> fin(G);
    for (int round = 0; round < max_rounds && !rc; ++round) {
        // BLACK movers search in agent A's tables with net A, WHITE movers in agent B's with net B
        // a NULL network = RandomOthelloAgent on that colour: it moves first in the round (a game may then play two plies
        // in one round, which changes nothing: games are independent and every ply is keyed by (game id, ply))
        if (!a->na) arena_opponent_move(a, 1, s);
        if (!a->nb) arena_opponent_move(a, -1, s);
        // who has to move?  Without passes every game of a round has the same mover, so one of the two agents has nothing to search: its
        // a->sims steps (11 launches each over zero leaves) are skipped -- one 8-byte read-back per round buys ~10 % at 800 sims per move.
        // (Round 5, measured and removed: BOTH agents in every round -- the odd slots held back one ply, agent A's and agent B's chains on two
        //  streams, k-splits sized for half batches -- 350.6 against 348.7 ms per ply of 512 games in an A/B on one device: the second chain's
        //  kernels run beside the first one's and slow them by what they gain, the chip is power limited)
        int movers[2] = {0, 0};
        hipMemsetAsync(a->d_movers, 0, sizeof movers, s);
        hipLaunchKernelGGL(k_arena_movers, dim3((G + 255) / 256), dim3(256), 0, s, sp->gm, a->d_movers);
        hipMemcpyAsync(movers, a->d_movers, sizeof movers, hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess) { oz_set_error("arena: stream failed"); rc = OZ_ERR_HIP; break; }
        if (movers[0] + movers[1] == 0) break;               // every game is over
        const bool run_a = a->na && movers[0] > 0, run_b = a->nb && movers[1] > 0;
        if (run_a) hipLaunchKernelGGL(k_sp_roots, dim3((G + 255) / 256), dim3(256), 0, s, sp->gm, ma->d, 1);
        if (run_a && sp->arena_tree_gc[0] != OZ_TREE_GC_OFF) tree_collect_async(ma, sp->arena_tree_gc[0], a->sims);
        if (run_b) hipLaunchKernelGGL(k_sp_roots, dim3((G + 255) / 256), dim3(256), 0, s, sp->gm, mb->d, -1);
        if (run_b && sp->arena_tree_gc[1] != OZ_TREE_GC_OFF) tree_collect_async(mb, sp->arena_tree_gc[1], a->sims);
        // the evaluator's launches are made for the movers of the round (an upper bound of the leaves a batch can hold), not for all G slots
        if (run_a) {
            std::lock_guard<std::mutex> la(a->na->mu);
            rc = mcts_steps_async(ma, a->na, a->sims, movers[0], false);
        }
        if (!rc && run_b) {
            std::lock_guard<std::mutex> lb(a->nb->mu);
            rc = mcts_steps_async(mb, a->nb, a->sims, movers[1], false);
        }
        if (rc) break;
        oz_mcts* const movers_m[2] = {run_a ? ma : nullptr, run_b ? mb : nullptr};
        for (int agent = 0; agent < 2 && !rc; ++agent) {
            oz_mcts* mm = movers_m[agent];
            MoveKernel move;
            MoveArgs margs;
            if (!mm || (rc = move_kernel(sp, mm, agent, false, &move, &margs))) continue;
            timed(mm, TS_MOVE, mm->profile, [&] { hipLaunchKernelGGL(move, dim3(G), dim3(64), 0, s, sp->gm, mm->d, margs); });
        }
        if (rc) break;
        if (hipGetLastError() != hipSuccess) { oz_set_error("arena kernel launch failed"); rc = OZ_ERR_HIP; break; }
        if ((round & 3) == 3 || round + 1 == max_rounds) {
            if ((rc = check_error_flag(ma))) break;
            if ((rc = check_error_flag(mb))) break;
            if (hipMemcpy(fin.data(), sp->gm.finished, G, hipMemcpyDeviceToHost) != hipSuccess) { oz_set_error("memcpy failed"); rc = OZ_ERR_HIP; break; }
            bool all = true;
            for (uint8_t f : fin) all = all && f;
            if (all) break;
        }
    }
    if (!rc) rc = check_error_flag(ma);
    if (!rc) rc = check_error_flag(mb);
    mb->stream = sb_saved;
    if (rc) return rc;
    OZ_HIP(hipStreamSynchronize(s));
    return OZ_OK;
}

OZ_API int oz_arena_results(oz_arena* a, int8_t* winner, int32_t* points, int32_t* n_moves, uint8_t* actions,
                            int8_t* players, uint64_t* final_black, uint64_t* final_white) {
    OZ_REQUIRE(a, "null arena");
    std::lock_guard<std::mutex> lk(a->mu);
    oz_selfplay* sp = &a->games;
    hipSetDevice(sp->m->device);
    const int G = sp->gm.G;
    hipLaunchKernelGGL(k_arena_collect, dim3((G + 255) / 256), dim3(256), 0, sp->m->stream, sp->gm, a->d_actions, a->d_players, a->d_nmoves);
    OZ_HIP(hipStreamSynchronize(sp->m->stream));
    std::vector<uint64_t> b(G), w(G);
    OZ_HIP(hipMemcpy(b.data(), sp->gm.black, 8ull * G, hipMemcpyDeviceToHost));
    OZ_HIP(hipMemcpy(w.data(), sp->gm.white, 8ull * G, hipMemcpyDeviceToHost));
    for (int g = 0; g < G; ++g) {
        const int pb = __builtin_popcountll(b[g]), pw = __builtin_popcountll(w[g]);
        if (winner) winner[g] = pb >= pw ? 1 : -1;               // draw -> BLACK agent (agents.py:83-84)
        if (points) points[g] = pb >= pw ? pb : pw;
        if (final_black) final_black[g] = b[g];
        if (final_white) final_white[g] = w[g];
    }
    if (n_moves) OZ_HIP(hipMemcpy(n_moves, a->d_nmoves, 4ull * G, hipMemcpyDeviceToHost));
    if (actions) OZ_HIP(hipMemcpy(actions, a->d_actions, (size_t)G * 128, hipMemcpyDeviceToHost));
    if (players) OZ_HIP(hipMemcpy(players, a->d_players, (size_t)G * 128, hipMemcpyDeviceToHost));
    return OZ_OK;
}

// ================================================================ exchange step over RCCL (SURVEY.md 8(b) gather_examples(comm), 8(e))
// The path's ONE collective -- the all-gather of the move records of the games a self-play batch completed -- behind the C ABI, for
// hosts that are not Python (othellozero_amd/distributed.py does the same through torch.distributed).  RCCL is bound at run time
// (dlopen of librccl.so.1: a process that already carries an RCCL -- PyTorch ships its own -- keeps using that one; no link-time
// dependency for single-GPU users).  Replaces WorkerManager.get_results' list concatenation (workers.py:180-184) and the ssh / pickle
// return path (workers.py:147-159).
#include <dlfcn.h>
namespace {
struct Rccl {
    struct Id { char b[OZ_COMM_ID_BYTES]; };                 // ncclUniqueId: 128 bytes, passed BY VALUE to ncclCommInitRank
    void* h = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
std::mutex g_rccl_mu;
int rccl_load() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.h) return OZ_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* nm : names) if ((h = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) { oz_set_error("RCCL not available: %s", dlerror()); return OZ_ERR_STATE; }
    Rccl r;
    r.h = h;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.GetErrorString) {
        oz_set_error("the RCCL library lacks an expected symbol");
        dlclose(h);
        return OZ_ERR_STATE;
    }
    g_rccl = r;
    return OZ_OK;
}
}  // namespace
#define OZ_NCCL(call) do { int rc__ = (call); if (rc__ != 0) { oz_set_error("RCCL: %s (%s)", g_rccl.GetErrorString(rc__), #call); return OZ_ERR_HIP; } } while (0)
enum { OZ_NCCL_UINT8 = 1, OZ_NCCL_INT64 = 4 };              // ncclDataType_t (rccl.h)

struct oz_comm {
    void* comm = nullptr;
    int rank = 0, world = 1, device = 0;
    hipStream_t stream = nullptr;
    long long* d_counts = nullptr;        // [2 + 2 * world]: this rank's (count, room), then every rank's pair
    unsigned char *d_send = nullptr, *d_recv = nullptr;
    long long cap = 0;                    // bytes per rank the two buffers hold
    std::mutex mu;
};

OZ_API int oz_comm_unique_id(uint8_t* id) {
    OZ_REQUIRE(id, "null id");
    if (int rc = rccl_load()) return rc;
    oz_current_device();
    OZ_NCCL(g_rccl.GetUniqueId(id));
    return OZ_OK;
}

OZ_API int oz_comm_create(oz_comm** out, const uint8_t* id, int rank, int world) {
    OZ_REQUIRE(out && id, "null argument");
    OZ_REQUIRE(world >= 1 && rank >= 0 && rank < world, "oz_comm_create: rank %d of %d", rank, world);
    if (int rc = rccl_load()) return rc;
    oz_comm* c = new oz_comm();
    c->rank = rank; c->world = world; c->device = oz_current_device();
    Rccl::Id uid;
    memcpy(uid.b, id, OZ_COMM_ID_BYTES);
    int nrc = g_rccl.CommInitRank(&c->comm, world, uid, rank);
    if (nrc != 0) { oz_set_error("RCCL: %s (ncclCommInitRank, rank %d of %d)", g_rccl.GetErrorString(nrc), rank, world); delete c; return OZ_ERR_HIP; }
    if (hipStreamCreate(&c->stream) != hipSuccess || hipMalloc((void**)&c->d_counts, sizeof(long long) * (2 * world + 2)) != hipSuccess) {
        oz_set_error("oz_comm_create: stream / buffer allocation failed");
        g_rccl.CommDestroy(c->comm);
        delete c;
        return OZ_ERR_HIP;
    }
    *out = c;
    return OZ_OK;
}

OZ_API int oz_comm_destroy(oz_comm* c) {
    if (!c) return OZ_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->comm) g_rccl.CommDestroy(c->comm);
    hipFree(c->d_counts); hipFree(c->d_send); hipFree(c->d_recv);
    hipStreamDestroy(c->stream);
    delete c;
    return OZ_OK;
}

// COLLECTIVE: every rank of `comm` calls it with its own engine.  The records [first_record, records completed so far) of every rank's
// engine, concatenated in rank order, into `out` (host, caller-owned, max_records long; per_rank[world] gets every rank's count).
// A (count, room) pair all-gather (16 bytes per rank) + ONE padded all-gather of the rows, device to device out of the engines' HBM
// buffers.  Every decision that could end the call on one rank is taken from the GATHERED pairs, i.e. identically on every rank (a
// rank-local capacity check let one rank leave while its peers entered the payload all-gather; ADVICE r4: so did a rank-local argument or HIP
// error BEFORE the first all-gather): a rank whose own arguments are bad (first_record < 0, a null buffer with room, the communicator on
// another device) or whose record counter cannot be read joins the pair all-gather with room = -2, "cannot take part", and EVERY rank fails
// together -- that rank with its own message, the others naming it; too little room on ANY rank fails the call on EVERY rank before the payload
// moves; a failed buffer allocation is agreed on by one more 8-byte all-gather.  What stays rank-local: null sp / comm / written (there is no
// communicator to say so with) and an RCCL / HIP failure of the collectives themselves (the communicator is then broken for everybody).
// out == NULL with max_records == 0 on every rank = the counts only (*written = the pooled number, per_rank filled): size the buffer, call again.
// The protocol is the same for any per-record payload: gather_rows moves `width`-byte rows of the engine buffer `src` (ring index = record
// index), so the records and the visit-count rows of oz_selfplay_gather_visits come back in the same order for the same first_record.
// visits != 0: the rows are the visit counts, which an engine without record_visits does not have -- a local argument error like the others.
static int gather_rows(oz_selfplay* sp, oz_comm* c, int visits, int64_t first_record, void* out_, int64_t max_records, int64_t* written,
                       int64_t* per_rank, const char* fn) {
    OZ_REQUIRE(sp && c && written, "null argument");
    std::lock_guard<std::mutex> lk(sp->mu);
    std::lock_guard<std::mutex> lkc(c->mu);
    hipSetDevice(c->device);
    unsigned char* out = (unsigned char*)out_;
    const size_t width = visits ? 64 * sizeof(int32_t) : sizeof(oz_record);
    const unsigned char* src = visits ? (const unsigned char*)sp->gm.visits : (const unsigned char*)sp->gm.records;
    char local_bad[256] = "";
    if (visits && !sp->gm.record_visits) snprintf(local_bad, sizeof local_bad, "the engine does not record visit counts (oz_selfplay_config.record_visits = 0)");
    else if (first_record < 0) snprintf(local_bad, sizeof local_bad, "first_record %lld", (long long)first_record);
    else if (!out && max_records != 0) snprintf(local_bad, sizeof local_bad, "null output buffer with room for %lld records", (long long)max_records);
    else if (c->device != sp->m->device) snprintf(local_bad, sizeof local_bad, "the communicator lives on device %d, the engine on device %d", c->device, sp->m->device);
    unsigned long long total = 0;
    if (!local_bad[0]) {
        hipError_t e = hipStreamSynchronize(sp->m->stream);
        if (e == hipSuccess) e = hipMemcpy(&total, sp->gm.counters, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { snprintf(local_bad, sizeof local_bad, "reading the engine's record counter failed: %s", hipGetErrorString(e)); (void)hipGetLastError(); }
    }
    long long have = (long long)total < sp->gm.record_cap ? (long long)total : sp->gm.record_cap;
    const int W = c->world;
    // room: >= 0 = records `out` holds, -1 = "counts only", -2 = "this rank cannot take part"
    long long pair[2] = {have > first_record ? have - first_record : 0, out ? (long long)max_records : -1};
    if (local_bad[0]) { pair[0] = 0; pair[1] = -2; }
    const long long mine = pair[0];
    OZ_HIP(hipMemcpyAsync(c->d_counts, pair, sizeof pair, hipMemcpyHostToDevice, c->stream));
    OZ_NCCL(g_rccl.AllGather(c->d_counts, c->d_counts + 2, 2, OZ_NCCL_INT64, c->comm, c->stream));
    std::vector<long long> pairs((size_t)2 * W);
    OZ_HIP(hipMemcpyAsync(pairs.data(), c->d_counts + 2, sizeof(long long) * 2 * W, hipMemcpyDeviceToHost, c->stream));
    OZ_HIP(hipStreamSynchronize(c->stream));
    *written = 0;
    if (local_bad[0]) { oz_set_error("%s: %s (every rank fails together)", fn, local_bad); return OZ_ERR_ARG; }
    for (int r = 0; r < W; ++r)
        if (pairs[2 * r + 1] == -2) { oz_set_error("%s: rank %d could not take part (bad arguments or a local error there): every rank fails together", fn, r); return OZ_ERR_STATE; }
    long long mx = 0, sum = 0;
    int counts_only = 0, short_rank = -1;
    for (int r = 0; r < W; ++r) {
        const long long cnt = pairs[2 * r];
        mx = cnt > mx ? cnt : mx; sum += cnt;
        if (per_rank) per_rank[r] = cnt;
        if (pairs[2 * r + 1] < 0) ++counts_only;
    }
    for (int r = 0; r < W && short_rank < 0; ++r) if (pairs[2 * r + 1] >= 0 && pairs[2 * r + 1] < sum) short_rank = r;
    if (counts_only == W) { *written = sum; return OZ_OK; }
    OZ_REQUIRE(counts_only == 0, "%s: %d of %d ranks asked for the counts only (out == NULL), the others for the rows", fn, counts_only, W);
    OZ_REQUIRE(short_rank < 0, "%s: %lld pooled records, rank %d has room for %lld (every rank fails together)", fn, sum, short_rank,
               pairs[2 * short_rank + 1]);
    if (mx == 0) return OZ_OK;
    if (mx * (long long)width > c->cap) {                     // grow the padded send / receive buffers (kept with the communicator); every rank's cap
        hipFree(c->d_send); hipFree(c->d_recv);               // has followed the same (mx, width) history, so all of them are here together
        c->d_send = c->d_recv = nullptr; c->cap = 0;
        const long long cap = (mx + mx / 4 + 1024) * (long long)width;
        long long failed = hipMalloc((void**)&c->d_send, (size_t)cap) != hipSuccess ||
                           hipMalloc((void**)&c->d_recv, (size_t)cap * W) != hipSuccess;
        if (!failed) c->cap = cap;
        else { hipFree(c->d_send); hipFree(c->d_recv); c->d_send = c->d_recv = nullptr; (void)hipGetLastError(); }
        OZ_HIP(hipMemcpyAsync(c->d_counts, &failed, sizeof failed, hipMemcpyHostToDevice, c->stream));
        OZ_NCCL(g_rccl.AllGather(c->d_counts, c->d_counts + 2, 1, OZ_NCCL_INT64, c->comm, c->stream));
        std::vector<long long> st((size_t)W);
        OZ_HIP(hipMemcpyAsync(st.data(), c->d_counts + 2, sizeof(long long) * W, hipMemcpyDeviceToHost, c->stream));
        OZ_HIP(hipStreamSynchronize(c->stream));
        for (int r = 0; r < W; ++r)
            if (st[r]) { oz_set_error("%s: rank %d could not allocate its exchange buffers (%lld bytes x %d ranks)", fn, r, cap, W); return OZ_ERR_HIP; }
    }
    if (mine) OZ_HIP(hipMemcpyAsync(c->d_send, src + (size_t)first_record * width, (size_t)mine * width, hipMemcpyDeviceToDevice, c->stream));
    if (mine < mx) OZ_HIP(hipMemsetAsync(c->d_send + (size_t)mine * width, 0, (size_t)(mx - mine) * width, c->stream));
    OZ_NCCL(g_rccl.AllGather(c->d_send, c->d_recv, (size_t)mx * width, OZ_NCCL_UINT8, c->comm, c->stream));
    long long pos = 0;
    for (int r = 0; r < W; ++r) {
        const long long cnt = pairs[2 * r];
        if (cnt) OZ_HIP(hipMemcpyAsync(out + (size_t)pos * width, c->d_recv + (size_t)r * mx * width, (size_t)cnt * width,
                                       hipMemcpyDeviceToHost, c->stream));
        pos += cnt;
    }
    OZ_HIP(hipStreamSynchronize(c->stream));
    *written = sum;
    return OZ_OK;
}
OZ_API int oz_selfplay_gather_records(oz_selfplay* sp, oz_comm* c, int64_t first_record, oz_record* out, int64_t max_records, int64_t* written,
                                      int64_t* per_rank) {
    return gather_rows(sp, c, 0, first_record, out, max_records, written, per_rank, "oz_selfplay_gather_records");
}
OZ_API int oz_selfplay_gather_visits(oz_selfplay* sp, oz_comm* c, int64_t first_record, int32_t* out, int64_t max_records, int64_t* written,
                                     int64_t* per_rank) {
    return gather_rows(sp, c, 1, first_record, out, max_records, written, per_rank, "oz_selfplay_gather_visits");
}

// ================================================================ diagnostics
// Device arithmetic used by the PUCT / backup formulas, exposed so the parity tests can compare it with the
// host libm / IEEE results bit for bit: sqrt (float64), division (float64, float32), float32 multiply-add chain.
__global__ void k_selftest_arith(const double* a, const double* b, int count, double* sq, double* dv, float* fdv, float* fq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    sq[i] = sqrt(a[i]);
    dv[i] = a[i] / b[i];
    const float x = (float)a[i], y = (float)b[i];
    fdv[i] = x / y;
    fq[i] = (x * y + x) / y;       // must stay mul, add, div (no FMA contraction)
}
OZ_API int oz_selftest_arith(const double* a, const double* b, int count, double* sqrt_a, double* div_ab, float* fdiv_ab,
                             float* fchain) {
    OZ_REQUIRE(a && b && sqrt_a && div_ab && fdiv_ab && fchain && count > 0, "bad argument");
    oz_current_device();
    double *da, *db, *ds, *dd; float *df, *dq;
    OZ_HIP(hipMalloc((void**)&da, 8ull * count)); OZ_HIP(hipMalloc((void**)&db, 8ull * count));
    OZ_HIP(hipMalloc((void**)&ds, 8ull * count)); OZ_HIP(hipMalloc((void**)&dd, 8ull * count));
    OZ_HIP(hipMalloc((void**)&df, 4ull * count)); OZ_HIP(hipMalloc((void**)&dq, 4ull * count));
    hipMemcpy(da, a, 8ull * count, hipMemcpyHostToDevice); hipMemcpy(db, b, 8ull * count, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_selftest_arith, dim3((count + 255) / 256), dim3(256), 0, 0, da, db, count, ds, dd, df, dq);
    hipError_t e = hipDeviceSynchronize();
    hipMemcpy(sqrt_a, ds, 8ull * count, hipMemcpyDeviceToHost); hipMemcpy(div_ab, dd, 8ull * count, hipMemcpyDeviceToHost);
    hipMemcpy(fdiv_ab, df, 4ull * count, hipMemcpyDeviceToHost); hipMemcpy(fchain, dq, 4ull * count, hipMemcpyDeviceToHost);
    hipFree(da); hipFree(db); hipFree(ds); hipFree(dd); hipFree(df); hipFree(dq);
    OZ_HIP(e);
    return OZ_OK;
}

// Sustained matrix-pipe rate of THIS device, right now: a pure-MFMA loop (no LDS, no loads, no barriers; one block per CU, one wave per SIMD,
// four independent accumulators back to back -- the issue pattern of the GEMM kernels' clusters) for about `target_ms`.  kind 0 =
// v_mfma_f32_32x32x2_f32 (what k_gemm_f32 runs on), kind 1 = v_mfma_f32_16x16x32_f16 on operands with every mantissa bit busy (what k_gemm_h2
// runs on; the sustained clock of that pipe follows the operand bits, docs/HISTORY.md section 4).  bench.py puts both numbers into its line as
// `device_calibration`, so that a reader can tell a slow box (or a power-capped one) from a regression: the GEMM kernels' own rate moves
// with this one.  tflops = FLOP of the issued MFMAs / HIP-event time; clock_ghz = the clock at which back-to-back issue (64 / 16 cycles per
// MFMA and SIMD) gives that rate.
__global__ __launch_bounds__(256) void k_diag_mfma_f32(float* out, int iters, float a0, float b0) {
    f32x16 acc[4];
    for (int i = 0; i < 4; ++i) for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const float a = a0 + threadIdx.x * 1.0009765625e-3f, b = b0 + threadIdx.x * 2.001953125e-3f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
    }
    float s = 0.f;
    for (int i = 0; i < 4; ++i) for (int r = 0; r < 16; ++r) s += acc[i][r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_diag_mfma_f16(float* out, int iters, unsigned seed) {
    f32x4 acc[4];
    for (int i = 0; i < 4; ++i) for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;
    f16x8 a, b;
    uint64_t r = oz_sm64(seed + 977u * (blockIdx.x * blockDim.x + threadIdx.x));
    for (int j = 0; j < 8; ++j) {                            // values in [2^-3, 2^-2) with random mantissas and signs: the window the network's tensors sit in
        r = oz_sm64(r);
        const unsigned short ha = (unsigned short)(0x3000u | (r & 0x3FFu) | ((r >> 10) & 1u) << 15);
        const unsigned short hb = (unsigned short)(0x3000u | ((r >> 16) & 0x3FFu) | ((r >> 26) & 1u) << 15);
        a[j] = __builtin_bit_cast(_Float16, ha); b[j] = __builtin_bit_cast(_Float16, hb);
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[i], 0, 0, 0);
    }
    float s = 0.f;
    for (int i = 0; i < 4; ++i) for (int r2 = 0; r2 < 4; ++r2) s += acc[i][r2];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_diag_mfma_bf16(float* out, int iters, unsigned seed) {
    f32x4 acc[4];
    for (int i = 0; i < 4; ++i) for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;
    bf16x8 a, b;
    uint64_t r = oz_sm64(seed + 977u * (blockIdx.x * blockDim.x + threadIdx.x));
    for (int j = 0; j < 8; ++j) {                            // values in [2^-3, 2^-2) with random 7-bit mantissas and signs: what the planes of precision bf16x3 hold
        r = oz_sm64(r);
        const unsigned short ha = (unsigned short)(0x3E00u | (r & 0x7Fu) | ((r >> 10) & 1u) << 15);
        const unsigned short hb = (unsigned short)(0x3E00u | ((r >> 16) & 0x7Fu) | ((r >> 26) & 1u) << 15);
        a[j] = __builtin_bit_cast(__bf16, ha); b[j] = __builtin_bit_cast(__bf16, hb);
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
    }
    float s = 0.f;
    for (int i = 0; i < 4; ++i) for (int r2 = 0; r2 < 4; ++r2) s += acc[i][r2];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
OZ_API int oz_selftest_mfma_rate(int kind, double target_ms, double* tflops, double* clock_ghz, double* ms_measured) {
    OZ_REQUIRE((kind == 0 || kind == 1 || kind == 2) && tflops, "oz_selftest_mfma_rate: kind must be 0 (f32), 1 (f16) or 2 (bf16), tflops non-null");
    OZ_REQUIRE(target_ms > 0 && target_ms <= 2000, "oz_selftest_mfma_rate: target_ms %.1f outside (0, 2000]", target_ms);
    const int dev = oz_current_device();
    hipDeviceProp_t prop;
    OZ_HIP(hipGetDeviceProperties(&prop, dev));
    const int cus = prop.multiProcessorCount;
    float* out = nullptr;
    OZ_HIP(hipMalloc((void**)&out, sizeof(float) * 256 * (size_t)cus));
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const double flop_per_mfma = kind == 0 ? 32.0 * 32 * 2 * 2 : 16.0 * 16 * 32 * 2;
    const double cycles_per_mfma = kind == 0 ? 64.0 : 16.0;  // back-to-back issue on one SIMD
    auto launch = [&](int iters) {
        if (kind == 0) hipLaunchKernelGGL(k_diag_mfma_f32, dim3(cus), dim3(256), 0, 0, out, iters, 0.5f, 0.25f);
        else if (kind == 1) hipLaunchKernelGGL(k_diag_mfma_f16, dim3(cus), dim3(256), 0, 0, out, iters, 12345u);
        else hipLaunchKernelGGL(k_diag_mfma_bf16, dim3(cus), dim3(256), 0, 0, out, iters, 12345u);
    };
    // a short run sizes the long one (and warms the clocks up)
    int iters = kind == 0 ? 400 : 1600;
    float ms = 0.f;
    hipError_t err = hipSuccess;
    for (int pass = 0; pass < 2 && err == hipSuccess; ++pass) {
        hipEventRecord(e0, 0);
        launch(iters);
        hipEventRecord(e1, 0);
        err = hipEventSynchronize(e1);
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
        if (pass == 0 && err == hipSuccess) {
            const double scale = target_ms / (ms > 1e-3f ? ms : 1e-3f);
            const double want = iters * scale;
            iters = (int)(want < 1 ? 1 : want > 2.0e8 ? 2.0e8 : want);
        }
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(out);
    OZ_HIP(err);
    const double mfmas = (double)cus * 4 /* waves = SIMDs */ * iters * 64.0;
    const double rate = mfmas * flop_per_mfma / (ms * 1e-3);
    *tflops = rate / 1e12;
    if (clock_ghz) *clock_ghz = mfmas / ((double)cus * 4) * cycles_per_mfma / (ms * 1e-3) / 1e9;
    if (ms_measured) *ms_measured = ms;
    return OZ_OK;
}
