// oz_minimax.h -- fixed-depth minimax on bitboards, one wavefront per position (gfx950).  The opponent the reference's author wanted next to
// RandomOthelloAgent: agents.py:27-41 (GreedyOthelloAgent, dead code) is "play the move that gains the most discs" = depth 1 on the disc count.
// Shared by the batch entry oz_rules_minimax (oz_rules.hip) and the arena's k_arena_minimax_move (oz_search.hip).  Integer arithmetic only.
//
// V(P, d), from the viewpoint of P's mover: T(P) if P is finished, else E(P) if d == 0, else max over legal a of s * V(child(P, a), d - 1), the child
// as oz_game_play leaves it: s = +1 where the turn passed back (same mover again), -1 otherwise.  E and T are antisymmetric in the mover, so the
// search works on (own, opp) = (mover's discs, the other's) and a finished child needs no mover at all: its T is taken for the side that moved.
// Depth counts moves made; passes are free.
//
// Work split: the root moves sit on the lanes by square (lane = row * 8 + col, the layout of values[64]); for depth >= 2 the wave then runs over
// the (root move, reply) PAIRS, 64 at a time -- an 8x8 midgame has ~10 root moves but ~100 pairs -- each lane searching its pair's subtree with a
// FULL window, and every root lane folds the exact values of its own replies afterwards (plain max over LDS, no atomics).  Inside a lane's subtree:
// iterative fail-hard alpha-beta, the lane's frame stack in LDS (32 bytes a frame, lane-contiguous arrays: no bank conflict, no scratch).
#pragma once
#include "oz_common.h"

#define OZ_MM_INF (1 << 20)                              // above every |T| (64000) and |E| (576); beta * 2 + pass still fits an int
#define OZ_MM_FRAMES (OZ_MINIMAX_MAX_DEPTH - 3)          // a pair's subtree has depth - 2 plies; a search of d plies stacks d - 1 frames
static_assert(OZ_MM_FRAMES >= 1, "the frame stack needs a level");

// the evaluation as data: the six weight classes of the n x n board as square masks (weights 100, -20, -50, 10, -2, 1 in this order)
struct MinimaxEval {
    uint64_t cls[6];
    int eval;
};
// class of square (r, c): dr = min(r, n-1-r), dc = min(c, n-1-c), (a, b) = (min(min(dr,dc), 2), min(max(dr,dc), 2)) ->
// (0,0) 100 | (0,1) -20 | (1,1) -50 | (0,2) 10 | (1,2) -2 | (2,2) 1
inline MinimaxEval oz_minimax_eval_make(int n, int eval) {
    MinimaxEval e = {};
    e.eval = eval;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            const int dr = r < n - 1 - r ? r : n - 1 - r, dc = c < n - 1 - c ? c : n - 1 - c;
            int a = dr < dc ? dr : dc, b = dr < dc ? dc : dr;
            a = a < 2 ? a : 2; b = b < 2 ? b : 2;
            const int k = a == 0 ? (b == 0 ? 0 : b == 1 ? 1 : 3) : a == 1 ? (b == 1 ? 2 : 4) : 5;
            e.cls[k] |= 1ULL << (r * 8 + c);
        }
    return e;
}

// E: the static value for the side holding `own`
__device__ __forceinline__ int mm_static(const MinimaxEval& e, uint64_t own, uint64_t opp) {
    if (e.eval == OZ_MINIMAX_EVAL_DISCS) return oz_popc(own) - oz_popc(opp);
    return 100 * (oz_popc(own & e.cls[0]) - oz_popc(opp & e.cls[0])) - 20 * (oz_popc(own & e.cls[1]) - oz_popc(opp & e.cls[1])) -
           50 * (oz_popc(own & e.cls[2]) - oz_popc(opp & e.cls[2])) + 10 * (oz_popc(own & e.cls[3]) - oz_popc(opp & e.cls[3])) -
           2 * (oz_popc(own & e.cls[4]) - oz_popc(opp & e.cls[4])) + (oz_popc(own & e.cls[5]) - oz_popc(opp & e.cls[5]));
}
// T: the value of a finished board for the side holding `own`
__device__ __forceinline__ int mm_terminal(const MinimaxEval& e, uint64_t own, uint64_t opp) {
    const int d = oz_popc(own) - oz_popc(opp);
    return e.eval == OZ_MINIMAX_EVAL_DISCS ? d : 1000 * d;
}

struct MinimaxLds {
    // frame stacks: [level][lane]; bs = beta * 2 + (1 where the frame's node was reached by a pass: its value goes up with s = +1)
    uint64_t own[OZ_MM_FRAMES][64], opp[OZ_MM_FRAMES][64], moves[OZ_MM_FRAMES][64];
    int alpha[OZ_MM_FRAMES][64], bs[OZ_MM_FRAMES][64];
    // root stage: the child of root move `lane` (mover first), its legal replies, the running pair offsets and one chunk of pair values
    uint64_t c_own[64], c_opp[64], c_replies[64];
    int off[65], val[64];
};

// after the side holding `own` has moved: the next node.  -> 0 finished; -1 the other side moves (own / opp swapped); +1 the turn passed back
__device__ __forceinline__ int mm_next(uint64_t& own, uint64_t& opp, uint64_t& moves, uint64_t valid) {
    const uint64_t l1 = oz_legal(opp, own, valid);
    if (l1) { const uint64_t t = own; own = opp; opp = t; moves = l1; return -1; }
    moves = oz_legal(own, opp, valid);
    return moves ? 1 : 0;
}

// exact V of the node (own to move, moves = its legal set, not empty) with d >= 1 plies left (d - 1 <= OZ_MM_FRAMES): full window at the top,
// fail-hard alpha-beta below.  Every lane runs its own tree; the loop does one move per turn and folds finished nodes before it.
__device__ __forceinline__ int mm_search(MinimaxLds& L, const MinimaxEval& e, uint64_t valid, int lane, uint64_t own, uint64_t opp, uint64_t moves, int d) {
    int level = 0, alpha = -OZ_MM_INF, beta = OZ_MM_INF, pass = 0;
    for (;;) {
        while (moves == 0 || alpha >= beta) {               // this node is done: its value (alpha) goes to the parent's frame
            if (level == 0) return alpha;
            const int v = pass ? alpha : -alpha;
            --level;
            own = L.own[level][lane]; opp = L.opp[level][lane]; moves = L.moves[level][lane];
            alpha = L.alpha[level][lane];
            const int bs = L.bs[level][lane];
            beta = bs >> 1; pass = bs & 1;
            if (v > alpha) alpha = v;
        }
        const int sq = oz_ctz(moves);
        moves &= moves - 1;
        uint64_t o2 = own, p2 = opp, m2;
        oz_apply(o2, p2, sq);
        const uint64_t mine = o2, theirs = p2;              // the board for the side that just moved
        const int s = mm_next(o2, p2, m2, valid);
        int v;
        if (s == 0) v = mm_terminal(e, mine, theirs);
        else if (d - level == 1) v = mm_static(e, mine, theirs);
        else {                                              // descend (level <= d - 2 < OZ_MM_FRAMES)
            L.own[level][lane] = own; L.opp[level][lane] = opp; L.moves[level][lane] = moves;
            L.alpha[level][lane] = alpha; L.bs[level][lane] = beta * 2 + pass;
            ++level;
            own = o2; opp = p2; moves = m2;
            if (s < 0) { const int a = -beta; beta = -alpha; alpha = a; pass = 0; }
            else pass = 1;
            continue;
        }
        if (v > alpha) alpha = v;
    }
}

// One wave (a block of 64 lanes) on one position: -> the exact root value of the move on square `lane` (OZ_MINIMAX_NONE off the legal set);
// *bests = the legal moves of maximal value (0: the mover has no move or the board is finished), the same in every lane.
// Every lane of the block must call it (block-wide barriers inside).
__device__ __forceinline__ int mm_root(MinimaxLds& L, const MinimaxEval& e, uint64_t valid, int lane, uint64_t black, uint64_t white, int player,
                                       int depth, uint64_t* bests) {
    depth = depth < 1 ? 1 : depth > OZ_MINIMAX_MAX_DEPTH ? OZ_MINIMAX_MAX_DEPTH : depth;
    const uint64_t own = player == 1 ? black : white, opp = player == 1 ? white : black;
    const uint64_t legal = oz_legal(own, opp, valid);
    const bool is_root = (legal >> lane) & 1;
    int value = OZ_MINIMAX_NONE, cs = 0;
    uint64_t co = 0, cp = 0, replies = 0;
    if (is_root) {
        co = own; cp = opp;
        oz_apply(co, cp, lane);
        const uint64_t mine = co, theirs = cp;
        cs = mm_next(co, cp, replies, valid);
        if (cs == 0) { value = mm_terminal(e, mine, theirs); replies = 0; }
        else if (depth == 1) { value = mm_static(e, mine, theirs); replies = 0; }
    }
    L.c_own[lane] = co; L.c_opp[lane] = cp; L.c_replies[lane] = replies;
    int inc = oz_popc(replies);                              // inclusive scan over the lanes: pair offsets
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    L.off[lane + 1] = inc;
    if (lane == 0) L.off[0] = 0;
    __syncthreads();
    const int total = L.off[64], first = L.off[lane], last = L.off[lane + 1];
    int best = -OZ_MM_INF;
    for (int c0 = 0; c0 < total; c0 += 64) {                 // pairs c0 .. c0 + 63, pair t on lane t - c0
        const int t = c0 + lane;
        int v = -OZ_MM_INF, s2 = 0;
        uint64_t go = 0, gp = 0, gm = 0;
        if (t < total) {
            int lo = 0, hi = 64;                             // the root r with off[r] <= t < off[r + 1]
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int mid = (lo + hi) >> 1;
                if (L.off[mid] <= t) lo = mid; else hi = mid;
            }
            go = L.c_own[lo]; gp = L.c_opp[lo];
            oz_apply(go, gp, oz_kth_bit(L.c_replies[lo], t - L.off[lo]));
            const uint64_t mine = go, theirs = gp;
            s2 = mm_next(go, gp, gm, valid);
            if (s2 == 0) v = mm_terminal(e, mine, theirs);
            else if (depth == 2) { v = mm_static(e, mine, theirs); s2 = 0; }
        }
        if (s2 != 0) v = s2 * mm_search(L, e, valid, lane, go, gp, gm, depth - 2);
        L.val[lane] = v;
        __syncthreads();
        const int b = first > c0 ? first : c0, en = last < c0 + 64 ? last : c0 + 64;
        for (int i = b; i < en; ++i) {
            const int x = L.val[i - c0];
            best = x > best ? x : best;
        }
        __syncthreads();
    }
    if (replies) value = cs * best;
    int mx = value;                                          // OZ_MINIMAX_NONE = INT32_MIN is below every value
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int y = __shfl_xor(mx, o, 64);
        mx = y > mx ? y : mx;
    }
    *bests = __ballot(is_root && value == mx);
    return value;
}
