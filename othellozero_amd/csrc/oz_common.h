// oz_common.h -- shared host/device helpers of libothellozero_amd (gfx950).
//
// Board representation everywhere in the library: two uint64 bitboards per
// position, bit index = row*8 + col for EVERY board size n in {4,6,8}; the
// n x n board occupies the top-left corner of the 8x8 grid, squares outside it
// are never occupied and never playable.  "own"/"opp" = reference channel 0 /
// channel 1 of a mover-canonical state (othelo_mcts.py:22-26,43-49);
// "black"/"white" = absolute colours of a game (Othello/__init__.py:22-25).
// NN action index = row*n + col (Net/NNet.py:86 reshape order).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define OZ_HD __host__ __device__ __forceinline__

// ---------------------------------------------------------------- integer mixers
// (identical formulas in oracle/oz_oracle.c and tests/golden/gen_golden.py)
OZ_HD uint64_t oz_sm64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
OZ_HD uint64_t oz_rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

enum { OZ_RNG_COIN = 0, OZ_RNG_EXPLORE = 1, OZ_RNG_TIE = 2, OZ_RNG_NOISE = 3, OZ_RNG_SAMPLE = 4, OZ_RNG_OPENING = 5, OZ_RNG_PLAYOUT = 6, OZ_RNG_GUMBEL = 7, OZ_RNG_SURPRISE = 8, OZ_RNG_RESIGN = 9 };
// GUMBEL: stream 7 + 256 * square, the Gumbel draw of a root's square (Gumbel search below).  7 + 256 sq is none of 0 .. 6 for sq >= 1 and is 7 for
// sq == 0; it is none of 3 + 256 sq' + 65536 i either: that would need 4 == 256 (sq' - sq) + 65536 i, and the right side is a multiple of 256.
// NOISE: stream 3 + 256 * square + 65536 * draw (root noise, oz_search.hip); SAMPLE: the one unit draw of a sampled move (move sampling,
// oz_search.hip) -- 4 is none of 3 + 256 sq + 65536 i; OPENING: the move of an opening ply, keyed (opening seed, opening id, ply)
// (oz_openings.h) -- nor is 5; PLAYOUT: the full / fast draw of a self-play move (playout cap, oz_playout_budget below) -- nor is 6
// SURPRISE: the draw of a record's copy count and first symmetry (policy surprise weighting below), keyed (weight seed, game id, ply) -- 8 is
// none of 3 + 256 sq + 65536 i, and 7 + 256 sq == 8 has no solution
// RESIGN: the one unit draw that exempts a game from resignation (resignation below), keyed (seed, game id, 0) -- 9 is none of 0 .. 8; it is none
// of 3 + 256 sq + 65536 i (6 is no multiple of 256) and none of 7 + 256 sq (nor is 2)
static_assert(OZ_RNG_RESIGN > OZ_RNG_SURPRISE && (OZ_RNG_RESIGN - OZ_RNG_NOISE) % 256 != 0 && (OZ_RNG_RESIGN - OZ_RNG_GUMBEL) % 256 != 0,
              "OZ_RNG_RESIGN collides with another stream");
// counter-based stream replacing random.random / np.random.choice / random.choice
// (training.py:51,56; othelo_mcts.py:59): keyed (seed, global game id, ply, purpose)
OZ_HD uint64_t oz_rng(uint64_t seed, uint64_t game, uint64_t move, uint64_t stream) {
    uint64_t a = oz_sm64(seed + 0x632BE59BD9B4E019ULL * game);
    return oz_sm64(a ^ (move * 0x9E3779B97F4A7C15ULL) ^ (stream * 0xD1B54A32D192ED03ULL));
}
OZ_HD double oz_rng_unit(uint64_t u) { return (double)(u >> 11) * (1.0 / 9007199254740992.0); }

// playout cap (include/othellozero_amd.h, "playout cap"): the simulation budget of the searched self-play move of game `game` at ply `ply`.
// The move is FULL iff u < full_prob, u = the unit draw of stream (seed, game, ply, OZ_RNG_PLAYOUT): `sims` simulations, *fast = 0; otherwise
// `fast_sims` simulations, *fast = 1.  fast_sims == 0 is the option switched off: every move is full.  The one definition the kernels
// (oz_search.hip) and the host's oz_playout_budgets share.
OZ_HD int oz_playout_budget(uint64_t seed, uint64_t game, uint64_t ply, int sims, int fast_sims, double full_prob, int* fast) {
    const int f = fast_sims > 0 && !(oz_rng_unit(oz_rng(seed, game, ply, OZ_RNG_PLAYOUT)) < full_prob) ? 1 : 0;
    *fast = f;
    return f ? fast_sims : sims;
}

// forced playouts (include/othellozero_amd.h, "forced playouts"): the count of one legal square of an armed root's row as the policy target
// keeps it.  N, Q, P, eta = the square's stored statistics and its share of the noise; the *s operands = those of `star`, the first legal
// square with the largest N (is_star != 0: this square is star and keeps its count); Ns, c, eps, k = the root's visits, the exploration
// constant, the noise's mixing weight and the forcing constant.  float64, no contraction, every
// expression as the header writes it.  The one definition the kernels (oz_search.hip) and the host's oz_forced_playouts_prune share.
OZ_HD int oz_forced_prune(int N, double Q, double P, double eta, int Nstar, double Qstar, double Pstar, double etastar, int is_star, int Ns, double c,
                          double eps, double k) {
#pragma clang fp contract(off)
    if (is_star || N <= 0 || !(k > 0.0)) return N;
    const double root = sqrt((double)Ns);
    const double Pn = (1.0 - eps) * P + eps * eta, Pns = (1.0 - eps) * Pstar + eps * etastar;
    const double Ustar = Qstar + (c * Pns) * (root / (double)(1 + Nstar));
    const double f = ceil(sqrt((k * Pn) * (double)Ns));
    const int F = f < 2147483647.0 ? (int)f : 2147483647;          // the most forcing can have added (NaN: everything, the PUCT bound below decides alone)
    const double gap = Ustar - Q;
    int Np = N;
    if (gap > 0.0) {                                                // else its Q alone reaches Ustar: keep
        const double need = ((c * Pn) * root) / gap - 1.0;
        const int m = need < (double)N ? (need > 0.0 ? (int)ceil(need) : 0) : N;          // NaN / inf: keep
        const int lo = N - F > m ? N - F : m;
        Np = N < lo ? N : lo;
    }
    if (Np < N && Np <= 1) Np = 0;                                  // a child cut down to one visit is dropped
    return Np;
}

// Gumbel search (include/othellozero_amd.h, "Gumbel search"): the root rule of Gumbel AlphaZero.  float64, no contraction, squares in ascending
// sq = row*8 + col, the first maximum wins.  The kernels (oz_search.hip) and the host's oz_gumbel_* evaluate the functions below.
// The Gumbel draw of a legal square from its unit draw u in [0, 1) (a multiple of 2^-53): g = -log(-log(w)), w = u except that the one endpoint
// the stream can give, u == 0, maps to w = 2^-54 (half the smallest draw above it).  w lies in [2^-54, 1 - 2^-53], so -log(w) lies in
// [1.1e-16, 37.5] and g in [-3.63, 36.8]: always finite.
// g is ill-conditioned where -log(w) is near 1 (g near 0): one ulp of the inner logarithm is then many ulps of g, so the inner logarithm has to be
// the correctly rounded one.  The host's libm log is (in all but 1 of 1 400 arguments); the device's is a 1-ulp function, so the device evaluates
// both logarithms with oz_log_cr below: double-double arithmetic (error below 2^-85, correctly rounded in practice), IEEE operations only.
struct OzDD { double hi, lo; };
OZ_HD OzDD oz_dd_two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return OzDD{s, (a - (s - bb)) + (b - bb)};
}
OZ_HD OzDD oz_dd_norm(double a, double b) {                         // |a| >= |b|
#pragma clang fp contract(off)
    const double s = a + b;
    return OzDD{s, b - (s - a)};
}
OZ_HD OzDD oz_dd_add(OzDD a, OzDD b) {
#pragma clang fp contract(off)
    OzDD s = oz_dd_two_sum(a.hi, b.hi);
    const double l = (a.lo + b.lo) + s.lo;
    return oz_dd_norm(s.hi, l);
}
OZ_HD OzDD oz_dd_mul(OzDD a, OzDD b) {
#pragma clang fp contract(off)
    const double p = a.hi * b.hi;
    const double e = __builtin_fma(a.hi, b.hi, -p);                 // the exact error of the product
    const double c = a.hi * b.lo + a.lo * b.hi;
    return oz_dd_norm(p, e + c);
}
OZ_HD OzDD oz_dd_div(OzDD a, OzDD b) {
#pragma clang fp contract(off)
    const double q1 = a.hi / b.hi;
    const OzDD p = oz_dd_mul(b, OzDD{q1, 0.0});
    const OzDD r = oz_dd_add(a, OzDD{-p.hi, -p.lo});
    const double q2 = r.hi / b.hi;
    return oz_dd_norm(q1, q2);
}
// log(x) of a positive normal x: x = 2^e m, m in [0.75, 1.5); s = (m - 1) / (m + 1), |s| <= 0.2; log(m) = 2 s (1 + z/3 + z^2/5 + ..), z = s^2, the
// terms up to z^4 / 9 in double-double, z^5 / 11 .. z^17 / 35 in double (below 2^-79 of the sum); the next term is below 2^-88
OZ_HD double oz_log_cr(double x) {
#pragma clang fp contract(off)
    union { double d; uint64_t u; } b;
    b.d = x;
    int e = (int)((b.u >> 52) & 0x7FF) - 1023;
    b.u = (b.u & 0x000FFFFFFFFFFFFFULL) | 0x3FF0000000000000ULL;
    double m = b.d;
    if (m >= 1.5) { m *= 0.5; e += 1; }
    const OzDD s = oz_dd_div(OzDD{m - 1.0, 0.0}, oz_dd_two_sum(m, 1.0));
    const OzDD z = oz_dd_mul(s, s);
    double t = 1.0 / 35.0;
    for (int c = 33; c >= 11; c -= 2) t = t * z.hi + 1.0 / (double)c;
    OzDD h{t, 0.0};
    for (int c = 9; c >= 1; c -= 2) h = oz_dd_add(oz_dd_mul(h, z), oz_dd_div(OzDD{1.0, 0.0}, OzDD{(double)c, 0.0}));
    OzDD r = oz_dd_mul(s, h);
    r.hi *= 2.0; r.lo *= 2.0;
    const OzDD ln2{0x1.62e42fefa39efp-1, 0x1.abc9e3b39803fp-56};
    const OzDD k = oz_dd_mul(ln2, OzDD{(double)e, 0.0});
    r = oz_dd_add(k, r);
    return r.hi + r.lo;
}
OZ_HD double oz_gumbel_value(double u) {
#pragma clang fp contract(off)
    const double w = u > 0.0 ? u : 5.5511151231257827e-17;
#if defined(__HIP_DEVICE_COMPILE__)
    return -oz_log_cr(-oz_log_cr(w));
#else
    return -log(-log(w));
#endif
}
OZ_HD double oz_gumbel_draw(uint64_t seed, uint64_t game, uint64_t ply, int sq) {
    return oz_gumbel_value(oz_rng_unit(oz_rng(seed, game, ply, (uint64_t)OZ_RNG_GUMBEL + 256ull * (uint64_t)sq)));
}
// considered_visits(m, n): the visit count a root's pick must match at each of the n simulations of a search that considers m moves
// (sequential halving).  out[n].  m <= 1: 0, 1, .., n-1.
inline void oz_gumbel_schedule(int m, int n, int* out) {
    if (m <= 1) { for (int i = 0; i < n; ++i) out[i] = i; return; }
    int L = 0;
    while ((1 << L) < m) ++L;                                      // ceil(log2 m)
    int visits[64];
    for (int i = 0; i < 64; ++i) visits[i] = 0;
    int k = m, len = 0;
    while (len < n) {
        int extra = n / (L * k);
        if (extra < 1) extra = 1;
        for (int e = 0; e < extra && len < n; ++e)
            for (int i = 0; i < k; ++i) {
                if (len < n) out[len++] = visits[i];
                visits[i] += 1;
            }
        k = k / 2 > 2 ? k / 2 : 2;
    }
}
// The root's sums, one legal square after the other in ascending order: sumN, maxN over the stored N; Pvis, PQ over the squares with N > 0.
struct OzGumbelSums { long long sumN; int maxN; double Pvis, PQ; };
OZ_HD void oz_gumbel_acc(OzGumbelSums& s, int N, double Q, double P) {
#pragma clang fp contract(off)
    s.sumN += N;
    if (N > s.maxN) s.maxN = N;
    if (N > 0) {
        const double pq = P * Q;
        s.Pvis = s.Pvis + P;
        s.PQ = s.PQ + pq;
    }
}
// the value every unvisited move is completed with
OZ_HD double oz_gumbel_vmix(const OzGumbelSums& s, double vhat) {
#pragma clang fp contract(off)
    if (s.sumN == 0) return vhat;
    const double r = (double)s.sumN / s.Pvis;
    const double a = s.Pvis > 0.0 ? r * s.PQ : 0.0;              // (only zero-prior squares visited: no prior-weighted mean, the term is 0)
    return (vhat + a) / (1.0 + (double)s.sumN);
}
// x = logit + sigma of a legal square (the improved policy is its softmax, the score adds g in front)
OZ_HD double oz_gumbel_sigma(int N, double Q, double vmix, int maxN, double c_visit, double c_scale) {
#pragma clang fp contract(off)
    const double qhat = N > 0 ? Q : vmix;
    const double h = (qhat + 1.0) * 0.5;
    const double s = (c_visit + (double)maxN) * c_scale;
    return s * h;
}
OZ_HD double oz_gumbel_x(double P, double sigma) {
#pragma clang fp contract(off)
    return log(P) + sigma;                                         // log(0) = -inf: such a square wins only where nothing else is legal
}
OZ_HD double oz_gumbel_score(double g, double P, double sigma) {
#pragma clang fp contract(off)
    const double a = g + log(P);
    return a + sigma;
}
// One root on the host, from its rows by square: the pick of the next descent, the move, the improved policy row (float32 [64]) and the
// scores (float64 [64], -inf off the legal set; may be null).  tables[max_considered][budget] = oz_gumbel_schedule(m, budget) for m = 1 .. max_considered.  *gap_pick / *gap_move (may be null) = the
// distance between the best and the second-best score among the candidates of the decision (inf with one candidate).
inline void oz_gumbel_root_row(const int32_t* N, const int32_t* N0, const double* Q, const double* P, const double* g, uint64_t legal, double vhat,
                               int max_considered, double c_visit, double c_scale, int budget, const int* tables, int* pick, int* move, float* pi, double* score,
                               double* gap_pick, double* gap_move) {
#pragma clang fp contract(off)
    OzGumbelSums s{0, 0, 0.0, 0.0};
    long long t = 0;
    int maxn = 0;
    for (int sq = 0; sq < 64; ++sq)
        if ((legal >> sq) & 1) {
            oz_gumbel_acc(s, N[sq], Q[sq], P[sq]);
            const int n = N[sq] - N0[sq];
            t += n;
            if (n > maxn) maxn = n;
        }
    const double vmix = oz_gumbel_vmix(s, vhat);
    double x[64], sc[64], mx = -INFINITY;
    for (int sq = 0; sq < 64; ++sq) {
        x[sq] = sc[sq] = -INFINITY;
        pi[sq] = 0.0f;
        if ((legal >> sq) & 1) {
            const double sg = oz_gumbel_sigma(N[sq], Q[sq], vmix, s.maxN, c_visit, c_scale);
            x[sq] = oz_gumbel_x(P[sq], sg);
            sc[sq] = oz_gumbel_score(g[sq], P[sq], sg);
            if (x[sq] > mx) mx = x[sq];
        }
        if (score) score[sq] = sc[sq];
    }
    const int cnt = __builtin_popcountll(legal);
    *pick = -1; *move = -1;
    if (gap_pick) *gap_pick = INFINITY;
    if (gap_move) *gap_move = INFINITY;
    if (cnt == 0) return;
    const int m_eff = max_considered < cnt ? max_considered : cnt;
    const int cv = t >= 0 && t < budget ? tables[(size_t)(m_eff - 1) * budget + t] : maxn;
    for (int which = 0; which < 2; ++which) {
        const int want = which ? maxn : cv;
        bool any = false;
        for (int sq = 0; sq < 64; ++sq) any = any || (((legal >> sq) & 1) && N[sq] - N0[sq] == want);
        int best = -1;
        double bs = 0.0, second = -INFINITY;
        for (int sq = 0; sq < 64; ++sq) {
            if (!((legal >> sq) & 1) || (any && N[sq] - N0[sq] != want)) continue;
            if (best < 0) { best = sq; bs = sc[sq]; }
            else if (sc[sq] > bs) { second = bs; best = sq; bs = sc[sq]; }
            else if (sc[sq] > second) second = sc[sq];
        }
        const double gap = second == -INFINITY ? INFINITY : bs - second;
        if (which) { *move = best; if (gap_move) *gap_move = gap; }
        else { *pick = best; if (gap_pick) *gap_pick = gap; }
    }
    // the improved policy: softmax of x over the legal squares, the sum in ascending order, one rounding to float32 per element
    if (mx == -INFINITY) { for (int sq = 0; sq < 64; ++sq) if ((legal >> sq) & 1) pi[sq] = (float)(1.0 / (double)cnt); return; }
    double e[64], sum = 0.0;
    for (int sq = 0; sq < 64; ++sq) {
        e[sq] = ((legal >> sq) & 1) ? exp(x[sq] - mx) : 0.0;
        sum = sum + e[sq];
    }
    for (int sq = 0; sq < 64; ++sq) pi[sq] = (float)(e[sq] / sum);
}

OZ_HD uint64_t oz_stub_h(uint64_t own, uint64_t opp, uint64_t salt, uint64_t i) {
    return oz_sm64(oz_sm64(own ^ salt) ^ oz_rotl64(opp, 29) ^ ((i + 1) * 0xD6E8FEB86659FD93ULL));
}

// ---------------------------------------------------------------- bitboard rules
OZ_HD uint64_t oz_valid_mask(int n) {
    uint64_t row = (1ULL << n) - 1ULL, m = 0;
    for (int r = 0; r < n; ++r) m |= row << (8 * r);
    return m;
}

#define OZ_NOT_COL0 0xFEFEFEFEFEFEFEFEULL
#define OZ_NOT_COL7 0x7F7F7F7F7F7F7F7FULL

// one step along direction D (0..7); rows grow with bit index (south = +8), cols east = +1
template <int D> OZ_HD uint64_t oz_shift(uint64_t x) {
    if (D == 0) return x << 8;                       // S  (+1, 0)
    if (D == 1) return x >> 8;                       // N  (-1, 0)
    if (D == 2) return (x << 1) & OZ_NOT_COL0;       // E  ( 0,+1)
    if (D == 3) return (x >> 1) & OZ_NOT_COL7;       // W  ( 0,-1)
    if (D == 4) return (x << 9) & OZ_NOT_COL0;       // SE (+1,+1)
    if (D == 5) return (x >> 9) & OZ_NOT_COL7;       // NW (-1,-1)
    if (D == 6) return (x << 7) & OZ_NOT_COL7;       // SW (+1,-1)
    return (x >> 7) & OZ_NOT_COL0;                   // NE (-1,+1)
}

template <int D> OZ_HD uint64_t oz_legal_dir(uint64_t own, uint64_t opp) {
    uint64_t t = oz_shift<D>(own) & opp;
    t |= oz_shift<D>(t) & opp; t |= oz_shift<D>(t) & opp; t |= oz_shift<D>(t) & opp;
    t |= oz_shift<D>(t) & opp; t |= oz_shift<D>(t) & opp;
    return oz_shift<D>(t);
}

// R4 (Othello/__init__.py:208-214): legal-move set of the side holding `own`.
// Legality is identical to standard Othello, so the standard flood works.
OZ_HD uint64_t oz_legal(uint64_t own, uint64_t opp, uint64_t valid) {
    uint64_t m = oz_legal_dir<0>(own, opp) | oz_legal_dir<1>(own, opp) | oz_legal_dir<2>(own, opp) |
                 oz_legal_dir<3>(own, opp) | oz_legal_dir<4>(own, opp) | oz_legal_dir<5>(own, opp) |
                 oz_legal_dir<6>(own, opp) | oz_legal_dir<7>(own, opp);
    return m & ~(own | opp) & valid;
}

// R3 (Othello/__init__.py:216-235) along one ray, INCLUDING the reference's
// "flip-through": every opponent disc that lies before the LAST own disc of the
// contiguous occupied run starting at the neighbour is flipped.
//   D = walking direction, B = its opposite.
template <int D, int B> OZ_HD uint64_t oz_flips_dir(uint64_t bit, uint64_t own, uint64_t opp) {
    uint64_t x = oz_shift<D>(bit) & opp;              // first neighbour must be an opponent disc
    if (!x) return 0;
    const uint64_t occ = own | opp;
    uint64_t seg = x;                                 // contiguous occupied run from the neighbour
    seg |= oz_shift<D>(seg) & occ; seg |= oz_shift<D>(seg) & occ; seg |= oz_shift<D>(seg) & occ;
    seg |= oz_shift<D>(seg) & occ; seg |= oz_shift<D>(seg) & occ; seg |= oz_shift<D>(seg) & occ;
    uint64_t back = seg & own;                        // own discs inside the run ...
    back |= oz_shift<B>(back) & seg; back |= oz_shift<B>(back) & seg; back |= oz_shift<B>(back) & seg;
    back |= oz_shift<B>(back) & seg; back |= oz_shift<B>(back) & seg; back |= oz_shift<B>(back) & seg;
    return back & opp;                                // ... and every opponent disc before one of them
}

// flips of placing a disc of `own` on square sq (sq must be empty; no legality check, R5)
OZ_HD uint64_t oz_flips(uint64_t own, uint64_t opp, int sq) {
    const uint64_t bit = 1ULL << sq;
    return oz_flips_dir<0, 1>(bit, own, opp) | oz_flips_dir<1, 0>(bit, own, opp) |
           oz_flips_dir<2, 3>(bit, own, opp) | oz_flips_dir<3, 2>(bit, own, opp) |
           oz_flips_dir<4, 5>(bit, own, opp) | oz_flips_dir<5, 4>(bit, own, opp) |
           oz_flips_dir<6, 7>(bit, own, opp) | oz_flips_dir<7, 6>(bit, own, opp);
}

// R5 flip_board_squares (Othello/__init__.py:237-247)
OZ_HD void oz_apply(uint64_t& own, uint64_t& opp, int sq) {
    const uint64_t f = oz_flips(own, opp, sq);
    own |= f | (1ULL << sq);
    opp &= ~(f | (1ULL << sq));
}

// OthelloGame.play, Othello/__init__.py:136-159: flip, switch player; if the new mover has no move,
// either the game is over (nobody can move) or the turn passes back.  player: +1 BLACK, -1 WHITE.
OZ_HD void oz_game_play(uint64_t& black, uint64_t& white, int& player, int& finished, int sq, uint64_t valid) {
    if (player == 1) oz_apply(black, white, sq); else oz_apply(white, black, sq);
    player = -player;
    uint64_t mine = player == 1 ? black : white, theirs = player == 1 ? white : black;
    if (oz_legal(mine, theirs, valid) == 0) {
        if (oz_legal(theirs, mine, valid) == 0) finished = 1;
        else player = -player;
    }
}

OZ_HD int oz_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}
OZ_HD int oz_ctz(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)x) - 1;
#else
    return __builtin_ctzll(x);
#endif
}
// index of the k-th (0-based) set bit
OZ_HD int oz_kth_bit(uint64_t m, int k) {
    for (int i = 0; i < k; ++i) m &= m - 1;
    return oz_ctz(m);
}

// NumPy pairwise sum of a contiguous float64 vector, 8 <= len <= 128 (np.sum at MCTS/__init__.py:49-51)
__host__ __device__ inline double pairwise_sum(const double* a, int len) {
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < len - (len % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < len; ++i) res += a[i];
    return res;
}

// ---------------------------------------------------------------- value signs of the backup
// (include/othellozero_amd.h, "value signs").  A descent took the edges 0 .. depth-1; bit d of `swaps` is sigma_d: 1 where the turn went to the
// opponent after edge d (the descent swapped own and opp), 0 where the same side moves again (a pass, or the game is over).  `leaf` is the
// leaf's value for the side to move there -- `own` as the descent leaves it: the network's v, the solved sign, or oz_terminal_value.
//   sound:     edge d gets leaf * (-1)^(sigma_d + .. + sigma_{depth-1}): the leaf as the side that played edge d sees it.
//   reference: edge d gets leaf * (-1)^(depth - d) (MCTS/__init__.py:68-71: one negation per level, whoever moves), and a finished board is
//              worth +1 to `own` unless it has fewer discs (:39-40: a draw is own's win) -- so a move that ends the game in the mover's favour
//              stores -1.  The sigma bits are not read.
// Negations only: the values are exact in both modes.  oz_backup_last is what oz_mcts_last_value reports: minus what edge 0 got (at depth 0,
// -leaf).  The one definition the tree kernels (descend_one / backup_one, oz_search.hip) and the host's oz_search_backup_values share.
#define OZ_VSIGNS_REFERENCE 0
#define OZ_VSIGNS_SOUND 1
OZ_HD int oz_terminal_value(int mode, uint64_t own, uint64_t opp) {
    const int a = oz_popc(own), b = oz_popc(opp);
    if (mode == OZ_VSIGNS_SOUND) return (a > b) - (a < b);
    return a >= b ? 1 : -1;
}
OZ_HD double oz_backup_value(int mode, uint64_t swaps, int depth, int d, double leaf) {
    const int flips = mode == OZ_VSIGNS_SOUND ? oz_popc(swaps >> d) : depth - d;
    return (flips & 1) ? -leaf : leaf;
}
OZ_HD double oz_backup_last(int mode, uint64_t swaps, int depth, double leaf) {
    return -oz_backup_value(mode, depth > 0 ? swaps : 0, depth, 0, leaf);
}

// ---------------------------------------------------------------- proofs: exact values kept and backed up the tree
// (include/othellozero_amd.h, "proofs").  OZ_VSIGNS_PROVEN is the third, internal value of the tree kernels' VS argument: the sound rule plus
// proofs (every `mode == OZ_VSIGNS_SOUND` test above reads it through oz_vsigns_rule).  A proof is -1 / 0 / +1 for the side to move at the
// node, or OZ_PROOF_NONE.  One 32-byte entry per node beside its record: two masks by square (state of square sq = 2 * hi + lo: 0 unknown,
// 1 loss, 2 draw, 3 win -- e = state - 2), the node's legal set and its own value (set where it was expanded from a solved leaf).
#define OZ_VSIGNS_PROVEN 2
#define OZ_PROOF_NONE (-128)
struct OzProof { uint64_t lo, hi, legal; int32_t own, pad; };
OZ_HD int oz_vsigns_rule(int vs) { return vs == OZ_VSIGNS_PROVEN ? OZ_VSIGNS_SOUND : vs; }
OZ_HD int oz_proof_edge(uint64_t lo, uint64_t hi, int sq) {
    const int st = (int)((hi >> sq) & 1) * 2 + (int)((lo >> sq) & 1);
    return st ? st - 2 : OZ_PROOF_NONE;
}
// val(S): the own value if set; else +1 if a legal edge wins; else the maximum if every legal edge is known; else unknown
OZ_HD int oz_proof_value(uint64_t legal, uint64_t lo, uint64_t hi, int own) {
    if (own != OZ_PROOF_NONE) return own;
    if (legal & lo & hi) return 1;
    if (legal == 0 || (legal & ~(lo | hi)) != 0) return OZ_PROOF_NONE;
    return (legal & hi) ? 0 : -1;
}
// the edges a descent may take at a node of value `val` (OZ_PROOF_NONE below the root, where a known node is never descended): those whose
// proof equals a known val; else -- and where there is none -- those not proven lost; none of those either: the legal set, *inconsistent = 1
OZ_HD uint64_t oz_proof_candidates(uint64_t legal, uint64_t lo, uint64_t hi, int val, int* inconsistent) {
    *inconsistent = 0;
    uint64_t c = 0;
    if (val == 1) c = legal & lo & hi;
    else if (val == 0) c = legal & hi & ~lo;
    else if (val == -1) c = legal & lo & ~hi;
    if (c) return c;
    c = legal & ~(lo & ~hi);
    if (c) return c;
    *inconsistent = 1;
    return legal;
}
// e(S, sq) = x: 1 newly proven, 0 known and equal, -1 known and different (the masks are left alone)
OZ_HD int oz_proof_mark(uint64_t* lo, uint64_t* hi, int sq, int x) {
    const int e = oz_proof_edge(*lo, *hi, sq);
    if (e != OZ_PROOF_NONE) return e == x ? 0 : -1;
    const int st = x + 2;
    *lo |= (uint64_t)(st & 1) << sq;
    *hi |= (uint64_t)(st >> 1) << sq;
    return 1;
}
// the proof loop of the backup over the entries of a path (pr[d] = the entry of the node of level d, sq[d] / sigma[d] its edge and swap bit):
// from the bottom, x = V_L; per level x = sigma_d ? -x : x, e(path[d]) = x, and on while the node's value is known with x = that value.
// -> levels marked (counted from the bottom); *fresh = edges newly proven, *conflict = 1 where a known edge differed, *root = 1 where the
// value of level 0's node went from unknown to known
OZ_HD int oz_proof_backup(OzProof* const* pr, const int* sq, const unsigned char* sigma, int depth, int leaf, int* fresh, int* conflict, int* root) {
    int x = leaf, levels = 0;
    *fresh = 0; *conflict = 0; *root = 0;
    for (int d = depth - 1; d >= 0; --d) {
        OzProof* p = pr[d];
        x = sigma[d] ? -x : x;
        const int before = oz_proof_value(p->legal, p->lo, p->hi, p->own);
        const int r = oz_proof_mark(&p->lo, &p->hi, sq[d], x);
        ++levels;
        if (r > 0) *fresh += 1;
        if (r < 0) *conflict = 1;
        const int v = oz_proof_value(p->legal, p->lo, p->hi, p->own);
        if (v == OZ_PROOF_NONE) break;
        if (d == 0 && before == OZ_PROOF_NONE) *root = 1;
        x = v;
    }
    return levels;
}
// proof play (include/othellozero_amd.h, "proof play"): what a root's proofs leave of its raw counts for the move, the policy row and the root
// value.  `visited` = the squares with a raw count > 0.  -> val = oz_proof_value of the entry; *keep = the candidates the descent picks from at
// the root (oz_proof_candidates of val) where one of them was visited, else the legal set with *fallback = 1.  The row is the raw count on
// *keep and 0 elsewhere; the root value is (double)val where val is known; the proof code of the move is oz_proof_code(val).  A root proven
// a loss keeps its whole row: every edge is a candidate.
OZ_HD int oz_proof_play(uint64_t legal, uint64_t lo, uint64_t hi, int own, uint64_t visited, uint64_t* keep, int* fallback, int* inconsistent) {
    const int val = oz_proof_value(legal, lo, hi, own);
    const uint64_t c = oz_proof_candidates(legal, lo, hi, val, inconsistent);
    *fallback = (c & visited) == 0;
    *keep = *fallback ? legal : c;
    return val;
}
OZ_HD int oz_proof_code(int val) { return val == OZ_PROOF_NONE ? 0 : val + 2; }       // 0 unknown, 1 loss, 2 draw, 3 win: for the mover
// the sign a proof code gives oz_record.z (a draw follows z's convention: BLACK's win); code != 0
OZ_HD int oz_proof_code_z(int code, int player) { return code == 3 ? 1 : code == 1 ? -1 : player == 1 ? 1 : -1; }

// ---------------------------------------------------------------- selection: FPU reduction, visit-scaled c_puct, prior-first (opt-in)
// (include/othellozero_amd.h, "selection").  At a node S at level d of a descent, for a legal square a: N', Q' = the statistics as selection sees
// them (stored, or the virtual-loss view), n = Ns + k(S) the node's visits in that view, P the prior selection uses (the noisy one at an armed
// root), vhat the value the node's expansion backed up (header word 3).  float64, no contraction, every product, sum and quotient rounded on
// its own in the order written:
//     growth:      c_S = c + factor * oz_log_cr(((1.0 + (double)n) + base) / base)                     off: c_S = c
//     prior-first: r = n > 0 ? sqrt((double)n) : 1.0                                                    off: r = sqrt((double)n)
//     FPU:         f = d == 0 ? root_reduction : reduction;  visited(a) := N'_a > 0;  SN = the integer sum of N'_a,
//                  SQ = tree-sum of (visited ? (double)N'_a * Q'_a : 0.0),  SP = tree-sum of (visited ? P_a : 0.0),
//                  V = (vhat + SQ) / (1.0 + (double)SN),  F = V - f * sqrt(SP), and F = -1.0 where F < -1.0;
//                  a legal edge with N'_a == 0 takes Q'_a := F
//     U_a = Q'_a + (c_S * P_a) * (r / (double)(1 + N'_a))
// tree-sum: the balanced binary tree over the squares 0 .. 63 (x_i <- x_{2i} + x_{2i+1}, six rounds), zeros off the legal set -- one xor
// butterfly of the wave (wave_tree_sum_f64, oz_search.hip; addition commutes, so every lane ends with the same bits), oz_tree_sum64 on the host.
// The one definition the SEL instantiations of descend_one and the host's oz_search_select_c / oz_search_select_scores share.
#define OZ_SEL_FPU 1
#define OZ_SEL_GROWTH 2
#define OZ_SEL_PRIOR_FIRST 4
struct OzSelection { int flags; double fpu, fpu_root, base, factor; };    // flags == 0: off
OZ_HD double oz_select_c(double c, double base, double factor, int n) {
#pragma clang fp contract(off)
    return c + factor * oz_log_cr(((1.0 + (double)n) + base) / base);
}
OZ_HD double oz_select_r(int prior_first, int n) {
#pragma clang fp contract(off)
    return prior_first && n <= 0 ? 1.0 : sqrt((double)n);
}
OZ_HD double oz_select_fpu_q(int N, double Q) {
#pragma clang fp contract(off)
    return N > 0 ? (double)N * Q : 0.0;
}
OZ_HD double oz_select_fpu(double vhat, double SQ, double SP, int SN, double f, double* V) {
#pragma clang fp contract(off)
    *V = (vhat + SQ) / (1.0 + (double)SN);
    const double F = *V - f * sqrt(SP);
    return F < -1.0 ? -1.0 : F;
}
OZ_HD double oz_select_u(double Q, double cS, double P, double r, int N) {
#pragma clang fp contract(off)
    return Q + (cS * P) * (r / (double)(1 + N));
}
__host__ __device__ inline double oz_tree_sum64(const double* x /* [64] */) {
#pragma clang fp contract(off)
    double s[64];
    for (int i = 0; i < 64; ++i) s[i] = x[i];
    for (int w = 32; w >= 1; w >>= 1)
        for (int i = 0; i < w; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}

// ---------------------------------------------------------------- tree collection: which stored nodes a slot can still look up
// (include/othellozero_amd.h, "tree collection").  Every move adds exactly one disc and a pass creates no node (the child is stored as
// OthelloGame.play leaves it), so a descent from a root with D discs looks up the root itself and positions with more than D discs, nothing
// else: a stored node that is not the root and holds <= D discs is dead, every other node keeps its statistics.  (Reachability through the
// `child` indices would be the wrong rule: a transposed child that IS in the table reads -1 on an edge until that edge is descended.)
// The one definition k_tree_collect (oz_search.hip) and the host's oz_search_tree_keep share.
OZ_HD bool oz_tree_keep(uint64_t root_own, uint64_t root_opp, uint64_t own, uint64_t opp) {
    return (own == root_own && opp == root_opp) || oz_popc(own | opp) > oz_popc(root_own | root_opp);
}

// ---------------------------------------------------------------- root value and value targets
// (include/othellozero_amd.h, "value targets").  The root value of a search: the visit-weighted mean of the root's Q, for the player to
// move.  a[sq] = oz_root_term: (double)N * Q where N > 0, else 0 (counts are 0 off the legal set); oz_root_mean = pairwise_sum(a, 64) /
// (double)sum N, or 0 with *rc = 2 where nothing was visited.  float64, no contraction.  The kernels (oz_search.hip: one lane per square
// computes its term into a[], the wave sums N) and the host's oz_root_values (oz_root_value below) evaluate these two functions.
OZ_HD double oz_root_term(int32_t N, double Q) {
#pragma clang fp contract(off)
    return N > 0 ? (double)N * Q : 0.0;
}
__host__ __device__ inline double oz_root_mean(const double* a /* [64] */, long long total, int* rc) {
    if (total <= 0) { *rc = 2; return 0.0; }
    *rc = 0;
    return pairwise_sum(a, 64) / (double)total;
}
__host__ __device__ inline double oz_root_value(const int32_t* N /* [64] */, const double* Q /* [64] */, int* rc) {
    double a[64];
    long long total = 0;
    for (int sq = 0; sq < 64; ++sq) {
        a[sq] = oz_root_term(N[sq], Q[sq]);
        if (N[sq] > 0) total += N[sq];
    }
    return oz_root_mean(a, total, rc);
}
// The value target of a record from the game outcome z, the root value q and the targets of the plies after it.  exact: the record's z
// is an exact endgame value (oz_selfplay_solve_records with max_empties = E) and stays; blend: (1 - w) z + w q; td_step: one step of
// the TD(lambda) recurrence from BLACK's side, B_i = (1 - lam) (p_i q_i) + lam B_{i+1}.  om = 1 - w / 1 - lam, computed once by the
// caller.  float64, every product and the sum rounded on their own.  The one definition k_value_targets and the host's oz_value_targets share.
OZ_HD bool oz_value_target_exact(uint64_t black, uint64_t white, int n2, int exact_empties) {
    return exact_empties > 0 && n2 - oz_popc(black | white) <= exact_empties;
}
OZ_HD double oz_value_target_blend(double z, double q, double om, double w) {
#pragma clang fp contract(off)
    const double a = om * z, b = w * q;
    return a + b;
}
OZ_HD double oz_value_target_td_step(double pq, double b_next, double om, double lam) {
#pragma clang fp contract(off)
    const double a = om * pq, b = lam * b_next;
    return a + b;
}

// ---------------------------------------------------------------- resignation
// (include/othellozero_amd.h, "resignation").  The state of one game: side = whose win the last root values called (+1 BLACK, -1 WHITE, 0
// nobody's), streak = how many searched moves in a row called it (saturating at 255).  oz_resign_step takes the state over the searched move of
// ply `ply` with mover p = +-1 and root value q (oz_root_mean of the RAW counts, for the mover) and says whether the rule triggers there:
// b = p q is the value from BLACK's side; c = +1 where b >= v, -1 where b <= -v, else 0 (NaN fails both compares: 0).  float64, no contraction.
// oz_resign_is_exempt: the game is played out regardless (the audit share).  The one definition the move (oz_search.hip) and the host's
// oz_resign_scan / oz_resign_exempt share.
struct OzResign { int side, streak; };
OZ_HD bool oz_resign_step(OzResign& st, int p, double q, double v, int r, int min_ply, int ply) {
#pragma clang fp contract(off)
    const double b = (double)p * q;
    const int c = b >= v ? 1 : b <= -v ? -1 : 0;
    if (c == 0) { st.side = 0; st.streak = 0; }
    else if (c == st.side) st.streak = st.streak + 1 < 255 ? st.streak + 1 : 255;
    else { st.side = c; st.streak = 1; }
    return st.streak >= r && ply >= min_ply;
}
OZ_HD bool oz_resign_is_exempt(uint64_t seed, uint64_t game, double keep_prob) { return oz_rng_unit(oz_rng(seed, game, 0, OZ_RNG_RESIGN)) < keep_prob; }

// ---------------------------------------------------------------- policy surprise weighting
// (include/othellozero_amd.h, "policy surprise weighting").  The surprise of a searched move: s = KL(q || p), q the policy target row of the
// search and p the root's stored priors, by square.  oz_surprise_term: one square's q (log q - log max(p, DBL_MIN)), 0 where q is not positive;
// both logarithms are oz_log_cr (IEEE operations only: the same bits on host and device).  oz_surprise_sum: pairwise_sum of the 64 terms,
// clamped at 0 (rounding can leave a tiny negative sum where q == p).  float64, no contraction.  The move (oz_search.hip: one lane per
// square computes its term, the sum is taken over the wave's 64 terms) and the host's oz_policy_surprises evaluate these two functions.
OZ_HD double oz_surprise_term(double q, double p) {
#pragma clang fp contract(off)
    if (!(q > 0.0)) return 0.0;
    const double pp = p > 2.2250738585072014e-308 ? p : 2.2250738585072014e-308;
    const double d = oz_log_cr(q) - oz_log_cr(pp);
    return q * d;
}
__host__ __device__ inline double oz_surprise_sum(const double* term /* [64] */) {
    const double s = pairwise_sum(term, 64);
    return s > 0.0 ? s : 0.0;
}
// The weight of a fully searched record of a game with K such records whose surprises sum to S (pairwise, by ply): (1 - frac) + frac s K / S,
// rounded once to float32; 1 where S == 0.  om = 1 - frac, computed once by the caller.  Its copy count: floor(8 w + u), u the unit draw of
// d = oz_rng(weight seed, game id, ply, OZ_RNG_SURPRISE); its first symmetry: d & 7 (oz_rng_unit reads d >> 11: independent bits).
// The one definition k_surprise_weights and the host's oz_surprise_weights / oz_surprise_copies share.
OZ_HD float oz_surprise_weight(double s, int K, double S, double om, double frac) {
#pragma clang fp contract(off)
    if (S == 0.0) return 1.0f;
    const double a = s * (double)K;
    const double b = a / S;
    const double c = frac * b;
    return (float)(om + c);
}
OZ_HD int oz_surprise_copies(float w, uint64_t d) {
#pragma clang fp contract(off)
    const double a = 8.0 * (double)w;
    return (int)floor(a + oz_rng_unit(d));
}

// ---------------------------------------------------------------- training examples
// training_example_symmetries, training.py:13-23: outputs in the order rot90 k=1..4 (CCW), each
// first with fliplr then without.  src(t, r, c) = source cell of output cell (r, c).
OZ_HD int oz_sym_src(int t, int n, int r, int c) {
    const int k = (t >> 1) + 1, flip = !(t & 1);
    int rr = r, cc = flip ? (n - 1 - c) : c;
    for (int q = 0; q < (k & 3); ++q) { int ti = cc, tj = n - 1 - rr; rr = ti; cc = tj; }
    return rr * n + cc;
}

// ---------------------------------------------------------------- evaluation symmetry
// (include/othellozero_amd.h, "evaluation symmetry").  The orientation a position is evaluated in: a pure function of the position and a
// seed, so that a network with the option on is still a deterministic function of the board.  The one definition the kernels (oz_net.hip)
// and the host's oz_eval_symmetries share.
OZ_HD int oz_eval_symmetry(uint64_t seed, uint64_t own, uint64_t opp) { return (int)(oz_sm64(oz_sm64(seed ^ own) + opp) >> 61); }
// the bitboard b in orientation t (the numbering of oz_sym_src; t = 7 is the identity): bit r*8+c of the result, r, c < n, is the bit of b at
// the cell oz_sym_src(t, n, r, c); bits outside the n x n corner are 0.  Shared with the host's oz_sym_boards.
OZ_HD uint64_t oz_sym_board(int t, int n, uint64_t b) {
    uint64_t out = 0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            const int src = oz_sym_src(t, n, r, c);
            out |= ((b >> ((src / n) * 8 + src % n)) & 1ULL) << (r * 8 + c);
        }
    return out;
}

// ---------------------------------------------------------------- auxiliary targets (include/othellozero_amd.h, "auxiliary heads")
// The final board of a record's game from the mover's side: (final_black, final_white) for BLACK to move, swapped for WHITE.  Both words are 0
// ("no auxiliary target") for a record of an adjudicated game (pad[1] == 1: the board at the stop is no final board) and for the fast record
// of a playout cap (pad[0] == 1).  A real final board is never empty, so fin_own | fin_opp == 0 IS the mask.  The one definition the append
// kernels (oz_replay.hip) and the host's oz_aux_targets share; Rec = oz_record.
template <typename Rec> OZ_HD void oz_aux_target(const Rec& rec, uint64_t& fin_own, uint64_t& fin_opp) {
    const bool none = rec.pad[0] == 1 || rec.pad[1] == 1, black = rec.player == 1;
    fin_own = none ? 0 : black ? rec.final_black : rec.final_white;
    fin_opp = none ? 0 : black ? rec.final_white : rec.final_black;
}
// the ownership target of square sq = row*8+col: +1 / -1 / 0 for a square of fin_own / of fin_opp / empty
OZ_HD float oz_aux_own_target(uint64_t fin_own, uint64_t fin_opp, int sq) { return (float)((fin_own >> sq) & 1) - (float)((fin_opp >> sq) & 1); }
// the score target: the final disc margin for the mover over the A = n*n squares (both counts are exact in float32, one division)
OZ_HD float oz_aux_score_target(uint64_t fin_own, uint64_t fin_opp, int A) { return (float)(oz_popc(fin_own) - oz_popc(fin_opp)) / (float)A; }

// N ** (1 / T) of get_policy_action_probabilities (othelo_mcts.py:59-60) for a visit count.  k = 1 / T where that is an integer (else 0):
// the product of k factors is exact while it stays <= 2^53 (every partial product is then an integer below it), so it equals the
// correctly rounded power the host computes; beyond that, and for any other exponent, the device's pow.
__device__ __forceinline__ double oz_count_pow(int cnt, double inv, int k) {
    const double x = (double)cnt;
    if (k > 0) {
        double r = x;
        for (int i = 1; i < k; ++i) r *= x;
        if (r <= 9007199254740992.0) return r;
    }
    return pow(x, inv);
}
// the k of oz_count_pow for inv = 1 / T
inline int oz_count_pow_k(double inv) { return (inv == floor(inv) && inv <= 64.0) ? (int)inv : 0; }

// ---------------------------------------------------------------- error plumbing (host)
#include <stdio.h>
void oz_set_error(const char* fmt, ...);
// error codes: include/othellozero_amd.h (include it before this header)
#define OZ_HIP(call)                                                                     \
    do {                                                                                  \
        hipError_t e__ = (call);                                                          \
        if (e__ != hipSuccess) {                                                          \
            oz_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            return OZ_ERR_HIP;                                                            \
        }                                                                                 \
    } while (0)
#define OZ_REQUIRE(cond, ...)                                                             \
    do {                                                                                  \
        if (!(cond)) { oz_set_error(__VA_ARGS__); return OZ_ERR_ARG; }                    \
    } while (0)

// ---------------------------------------------------------------- device vector types
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));           // one 16-byte store
typedef const __attribute__((address_space(1))) void* oz_gptr;        // global source of an LDS-DMA (global_load_lds)
typedef __attribute__((address_space(3))) void* oz_lptr;              // its LDS destination

// ---------------------------------------------------------------- split-plane operand formats
// An fp32 value as the sum of two fp16 planes (precision f16x2, oz_net_h2.h header) or of three bf16 planes (precision bf16x3, oz_net_b3.h header).
__device__ __forceinline__ void h2_split(float x, _Float16& h1, _Float16& h2) {
    h1 = (_Float16)x;
    h2 = (_Float16)(x - (float)h1);
}
// x = b1 + b2 + b3 exactly for 2^-100 <= |x| <= FLT_MAX (round to nearest: |x - b1| <= 2^-8 |x|, |x - b1 - b2| <= 2^-17 |x|, and the third residual
// has at most 8 significant bits); below 2^-100 the last residual can fall under bf16's subnormal step: absolute error < 2^-120.  Inf and NaN give
// NaN planes.
__device__ __forceinline__ void b3_split(float x, __bf16& b1, __bf16& b2, __bf16& b3) {
    b1 = (__bf16)x;
    // the top 0.4 % of fp32's range (|x| > 0x7F7F8000 = bf16's largest value + half an ulp) would ROUND to infinity: take bf16's largest value instead --
    // the residual (< 2^120) still fits the other two planes exactly
    if (__builtin_isinf((float)b1) && !__builtin_isinf(x)) b1 = __builtin_bit_cast(__bf16, (unsigned short)(x < 0.f ? 0xFF7Fu : 0x7F7Fu));
    const float r1 = x - (float)b1;               // exact
    b2 = (__bf16)r1;
    b3 = (__bf16)(r1 - (float)b2);                // exact difference, at most 8 significant bits: the cast is exact
}
// Eight values split into PLANES planes (2: h2_split, 3: b3_split), plane p stored as one 16-byte chunk at dst[p * pstride];
// NT = non-temporal stores (an output that would otherwise evict data the kernel re-reads from L2).
template <bool NT> __device__ __forceinline__ void oz_store16(uint4* dst, u32x4 v) {
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst));
    else *reinterpret_cast<u32x4*>(dst) = v;
}
template <int PLANES, bool NT = false>
__device__ __forceinline__ void oz_split8_store(uint4* dst, size_t pstride, const float (&v)[8]) {
    static_assert(PLANES == 2 || PLANES == 3, "f16x2 or bf16x3");
    if constexpr (PLANES == 2) {
        f16x8 h1, h2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            _Float16 a, b;
            h2_split(v[j], a, b);
            h1[j] = a; h2[j] = b;
        }
        oz_store16<NT>(dst, __builtin_bit_cast(u32x4, h1));
        oz_store16<NT>(dst + pstride, __builtin_bit_cast(u32x4, h2));
    } else {
        bf16x8 p0, p1, p2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 a, b, c;
            b3_split(v[j], a, b, c);
            p0[j] = a; p1[j] = b; p2[j] = c;
        }
        oz_store16<NT>(dst, __builtin_bit_cast(u32x4, p0));
        oz_store16<NT>(dst + pstride, __builtin_bit_cast(u32x4, p1));
        oz_store16<NT>(dst + 2 * pstride, __builtin_bit_cast(u32x4, p2));
    }
}
// The h2 layout: a row of K values (a pixel's channels or a weight row's k) is K / 8 groups of 32 bytes, group g = [h1 x 8][h2 x 8] at chunks
// 2 g, 2 g + 1 of the row; rows follow each other.  Stores the group of k .. k + 7 (k % 8 == 0) of row `row`.
OZ_HD size_t h2_group_chunk(size_t row, int K, int k) { return (row * (size_t)(K >> 3) + (k >> 3)) * 2; }      // the h1 chunk; h2 follows it
template <bool NT = false>
__device__ __forceinline__ void h2_store8(uint4* out, size_t row, int K, int k, const float (&v)[8]) {
    oz_split8_store<2, NT>(out + h2_group_chunk(row, K, k), 1, v);
}
// The b3 layout: a row of K values is K / 32 k-tiles of 192 bytes = 12 chunks [plane 0: 32 bf16][plane 1: 32 bf16][plane 2: 32 bf16]; the chunk
// of plane p and 8-group kg = (k / 8) % 4 of k-tile k / 32 sits at 12 (k / 32) + 4 p + kg of the row; rows follow each other.  Stores the group of
// k .. k + 7 (k % 8 == 0) of row `row`.
OZ_HD size_t b3_group_chunk(size_t row, int K, int k) { return row * (size_t)(K / 32 * 12) + (k >> 5) * 12 + ((k >> 3) & 3); }   // plane 0; plane p 4 p chunks on
template <bool NT = false>
__device__ __forceinline__ void b3_store8(uint4* out, size_t row, int K, int k, const float (&v)[8]) {
    oz_split8_store<3, NT>(out + b3_group_chunk(row, K, k), 4, v);
}
// The way back (diagnostics: oz_net_get_activation): the eight values of the group at `src` (h2_group_chunk / b3_group_chunk) as the exact sum of
// their PLANES planes, plane p one 16-byte chunk at src[p * pstride] -- what a kernel that consumes the layout multiplies, in float64.
template <int PLANES>
__device__ __forceinline__ void oz_split8_load(const uint4* src, size_t pstride, double (&v)[8]) {
    static_assert(PLANES == 2 || PLANES == 3, "f16x2 or bf16x3");
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0;
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(src + p * pstride);
        if constexpr (PLANES == 2) {
            const f16x8 h = __builtin_bit_cast(f16x8, raw);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (double)(float)h[j];
        } else {
            const bf16x8 b = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (double)(float)b[j];
        }
    }
}
