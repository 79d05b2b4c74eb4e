// oz_solve.h -- exact endgame solver on bitboards, one wavefront per position (gfx950).  The reference has no solver (it trains on played
// outcomes only); this is oz_minimax.h's machinery with the horizon taken away.  Shared by the batch entry oz_rules_solve (oz_rules.hip) and by
// oz_selfplay_solve_records (oz_search.hip).  Integer arithmetic only.
//
// S(P), from the viewpoint of P's mover: own discs - opponent discs if P is finished, else max over legal a of s * S(child(P, a)), the child as
// oz_game_play leaves it: s = +1 where the turn passed back, -1 otherwise.  Empties are not awarded.  |S| <= 64.
//
// Work split.  The top of the tree is expanded breadth first into a node list in LDS (root children, their replies, ...) until a level holds
// OZ_SV_ITEMS nodes, the list is full, or the level's positions have OZ_SV_MIN_EMPTIES empties or fewer.  The last level's nodes are the ITEMS: a
// lane takes the next one from an LDS counter whenever it has finished one, so a lane with a small subtree does not wait for one with a large one.
// Every node keeps `best`, the largest value a completed child has returned (its own viewpoint), and `pend`, its children still out.  An item's
// window is read off its ancestors' `best` at the moment it starts: walking up, an ancestor of the same orientation raises the item's alpha to its
// best, one of the opposite orientation lowers the item's beta to minus its best -- plain alpha-beta with whatever bounds exist by then.  Root
// children have no parent, hence the window (-inf, +inf): EVERY ROOT MOVE'S VALUE IS EXACT.  The item's fail-hard result goes to its parent by an
// LDS max; the lane that brings a node's `pend` to zero carries that node's best one level further up.  Windows only ever tighten, so a result
// computed under an earlier, wider window is still a valid fail-hard result under the final one, and max is order-free: the outputs do not depend
// on which lane finished when.  A node whose window is already empty is skipped (its value cannot matter to its parent any more).
// No lane waits for another: every loop is bounded by the tree, the only synchronisation is the block barrier between expansion levels.
//
// Root window (compile time: sv_root<RA, RB>, the default is the full window above and compiles to what it was).  Where only the fail-hard value of
// the ROOT in (RA, RB) is wanted -- (-1, +1) gives sign(S), what a search leaf needs -- the root is one more ancestor: its `best` (L.root, in
// SolveLdsW) starts at RA, a completed root child raises it by the same LDS max, and the ancestor walk of an item ends there: an item of the root's
// orientation gets alpha >= root best and beta <= RB, one of the other orientation beta <= -root best and alpha >= -RB.  Once root best >= RB
// every window that is read is empty and nothing more starts.  The argument above carries over unchanged: the root's best only grows, so the
// bound an item read is never tighter than the final one and its fail-hard result stays valid under it; a result at or beyond the bound it was
// cut at reaches the root as a value <= root best (no effect on the max) or >= RB (clamped to RB at the end); and the root's value is a max,
// order-free.  The output min(root best, RB) therefore does not depend on which lane finished when -- only the amount of work does.  The per-move
// values and *bests of a windowed root are NOT exact and are not returned.
//
// Inside an item: iterative fail-hard alpha-beta, the lane's frame stack in LDS (20 bytes a frame -- the moves left, the discs the move changed, so
// that the parent's board is the child's with the move undone -- in lane-contiguous arrays: consecutive lanes hit consecutive banks, no scratch),
// corners first, the last empty counted by its flips without a frame or a legal-move flood.
#pragma once
#include "oz_minimax.h"

#define OZ_SV_INF 127                                     // above every |S| (64); alpha + 128 and beta + 128 fit a byte each
#define OZ_SV_FRAMES (OZ_SOLVE_MAX_EMPTIES - 3)           // an item has <= MAX - 1 empties; a search over e empties stacks e - 2 frames
#define OZ_SV_NODES 512                                   // expanded top of the tree
#define OZ_SV_ITEMS 160                                   // a level of this many nodes is not expanded further
#define OZ_SV_MIN_EMPTIES 4                               // nor one whose positions have this many empties or fewer
static_assert(OZ_SV_FRAMES >= 1, "the frame stack needs a level");

struct SolveLds {
    // frame stacks: [level][lane]; moves = the frame's moves not tried yet, undo = the square of the move in progress and the discs it flipped,
    // ab = (alpha + 128) | (beta + 128) << 8 | (1 << 16 where the frame's node was reached by a pass) | that square << 17
    uint64_t moves[OZ_SV_FRAMES][64], undo[OZ_SV_FRAMES][64];
    int ab[OZ_SV_FRAMES][64];
    // the expanded top: the position of node k (its mover first)
    uint64_t n_own[OZ_SV_NODES], n_opp[OZ_SV_NODES];
    int best[OZ_SV_NODES], pend[OZ_SV_NODES];
    // (parent + 1) << 2 | (2 for a dead node: a finished board, nothing to search) | (1 where the node's value goes up with s = +1); root
    // children: parent = -1
    int link[OZ_SV_NODES];
    int next;                                             // the item counter
};
struct SolveLdsW : SolveLds { int root; };                // a windowed root's best (sv_root<RA, RB>); the full-window kernels keep SolveLds

// one empty square x, `own` to move: exact disc difference for own at the end (a square is playable iff it flips something)
__device__ __forceinline__ int sv_last1(uint64_t own, uint64_t opp, int x) {
    const int d = oz_popc(own) - oz_popc(opp);
    const int f = oz_popc(oz_flips(own, opp, x));
    if (f) return d + 1 + 2 * f;
    const int g = oz_popc(oz_flips(opp, own, x));
    return g ? d - 1 - 2 * g : d;
}

// fail-hard value of the node (own to move, moves = its legal set, not empty, e >= 1 empties, e - 2 <= OZ_SV_FRAMES) in the window (alpha, beta):
// exact inside it, <= alpha below, >= beta above
__device__ __forceinline__ int sv_search(SolveLds& L, uint64_t valid, uint64_t corners, int lane, uint64_t own, uint64_t opp, uint64_t moves, int e,
                                         int alpha, int beta) {
    if (e == 1) return sv_last1(own, opp, oz_ctz(moves));
    int level = 0, pass = 0;
    for (;;) {
        while (moves == 0 || alpha >= beta) {               // this node is done: its value (alpha) goes to the parent's frame
            if (level == 0) return alpha;
            const int v = pass ? alpha : -alpha;
            --level;
            const int ab = L.ab[level][lane];
            const uint64_t changed = L.undo[level][lane], after_own = pass ? own : opp, after_opp = pass ? opp : own;
            own = after_own & ~changed; opp = (after_opp | changed) & ~(1ULL << (ab >> 17));
            moves = L.moves[level][lane];
            alpha = (ab & 255) - 128; beta = ((ab >> 8) & 255) - 128; pass = (ab >> 16) & 1;
            if (v > alpha) alpha = v;
        }
        const uint64_t first = moves & corners;
        const int sq = oz_ctz(first ? first : moves);
        const uint64_t bit = 1ULL << sq;
        moves &= ~bit;
        const uint64_t f = oz_flips(own, opp, sq);
        uint64_t o2 = own | f | bit, p2 = opp & ~f, m2;
        int v;
        if (e - level == 2) v = -sv_last1(p2, o2, oz_ctz(valid & ~(o2 | p2)));      // the child has one empty: the other side moves, or passes
        else {
            const uint64_t mine = o2, theirs = p2;
            const int s = mm_next(o2, p2, m2, valid);
            if (s != 0) {                                   // descend (level <= e - 3 < OZ_SV_FRAMES)
                L.moves[level][lane] = moves; L.undo[level][lane] = f | bit;
                L.ab[level][lane] = (alpha + 128) | (beta + 128) << 8 | pass << 16 | sq << 17;
                ++level;
                own = o2; opp = p2; moves = m2;
                if (s < 0) { const int a = -beta; beta = -alpha; alpha = a; pass = 0; }
                else pass = 1;
                continue;
            }
            v = oz_popc(mine) - oz_popc(theirs);
        }
        if (v > alpha) alpha = v;
    }
}

// node i is complete: its best goes to its parent; whoever completes the parent's last child carries on from there.  WIN: a root child's goes
// to the root's best
template <bool WIN, class LDS> __device__ __forceinline__ void sv_complete(LDS& L, int i) {
    for (;;) {
        const int lk = L.link[i], p = (lk >> 2) - 1;
        const int v = L.best[i];
        if (p < 0) {
            if constexpr (WIN) if (v != -OZ_SV_INF) atomicMax(&L.root, (lk & 1) ? v : -v);
            return;
        }
        if (v != -OZ_SV_INF) atomicMax(&L.best[p], (lk & 1) ? v : -v);      // (-inf: every child was skipped, the node has nothing to say)
        __threadfence_block();
        if (atomicSub(&L.pend[p], 1) != 1) return;
        __threadfence_block();
        i = p;
    }
}

// One wave (a block of 64 lanes) on one position whose mover (own) has the legal moves `legal` (not empty) and `empties` <= OZ_SOLVE_MAX_EMPTIES
// empty squares: -> the exact value of the move on square `lane` (OZ_MINIMAX_NONE off the legal set); *bests = the moves of maximal value,
// *value = that maximum = S of the position, the same in every lane.  Every lane of the block must call it (block-wide barriers inside).
// With a root window (RA, RB) inside (-inf, +inf) (LDS = SolveLdsW): *value = the fail-hard value of the position in that window, RA <= *value <=
// RB, the same in every lane; *bests = 0 and the return value is OZ_MINIMAX_NONE (see the header: the moves' values are not exact then).
template <int RA = -OZ_SV_INF, int RB = OZ_SV_INF, class LDS = SolveLds>
__device__ __forceinline__ int sv_root(LDS& L, uint64_t valid, uint64_t corners, int lane, uint64_t own, uint64_t opp, uint64_t legal,
                                       int empties, uint64_t* bests, int* value) {
    constexpr bool WIN = RA > -OZ_SV_INF || RB < OZ_SV_INF;
    static_assert(RA < RB, "an empty root window");
    const bool is_root = (legal >> lane) & 1;
    const int idx = oz_popc(legal & ((1ULL << lane) - 1ULL));
    __syncthreads();                                        // (a caller may run several positions through one SolveLds)
    if (lane == 0) {
        L.next = 0;
        if constexpr (WIN) L.root = RA;
    }
    if (is_root) {
        uint64_t co = own, cp = opp, m;
        oz_apply(co, cp, lane);
        const uint64_t mine = co, theirs = cp;
        const int s = mm_next(co, cp, m, valid);
        L.n_own[idx] = co; L.n_opp[idx] = cp;
        L.best[idx] = s ? -OZ_SV_INF : oz_popc(mine) - oz_popc(theirs);     // a finished child: its value for the side that moved, s = +1
        L.pend[idx] = 0;
        L.link[idx] = s > 0 ? 1 : s == 0 ? 3 : 0;
    }
    __syncthreads();
    if constexpr (WIN) {                                    // a root child that ends the game is complete already
        if (is_root && (L.link[idx] & 2)) atomicMax(&L.root, L.best[idx]);
        __syncthreads();
    }
    int lo = 0, hi = oz_popc(legal), e = empties - 1;       // the current level [lo, hi), its positions' empties
    while (e > OZ_SV_MIN_EMPTIES && hi - lo < OZ_SV_ITEMS) {
        int total = 0;
        for (int c0 = lo; c0 < hi; c0 += 64)               // (the legal sets are not kept: 4 KB of LDS against two floods per node)
            total += c0 + lane < hi && !(L.link[c0 + lane] & 2) ? oz_popc(oz_legal(L.n_own[c0 + lane], L.n_opp[c0 + lane], valid)) : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
        if (total == 0 || hi + total > OZ_SV_NODES) break;
        int base = hi;
        for (int c0 = lo; c0 < hi; c0 += 64) {              // node c0 + lane writes its children, a finished one as a dead node
            const int i = c0 + lane;
            uint64_t mv = i < hi && !(L.link[i] & 2) ? oz_legal(L.n_own[i], L.n_opp[i], valid) : 0;
            int inc = oz_popc(mv);
            const int cnt = inc;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(inc, o, 64);
                if (lane >= o) inc += y;
            }
            int k = base + inc - cnt;
            base += __shfl(inc, 63, 64);
            if (cnt) {
                const uint64_t o0 = L.n_own[i], p0 = L.n_opp[i];
                int live = 0, b = -OZ_SV_INF;
                for (; mv; mv &= mv - 1, ++k) {
                    uint64_t co = o0, cp = p0, m;
                    oz_apply(co, cp, oz_ctz(mv));
                    const uint64_t mine = co, theirs = cp;
                    const int s = mm_next(co, cp, m, valid);
                    L.n_own[k] = co; L.n_opp[k] = cp;
                    L.best[k] = -OZ_SV_INF; L.pend[k] = 0;
                    L.link[k] = (i + 1) << 2 | (s > 0 ? 1 : s == 0 ? 3 : 0);
                    if (s == 0) { const int t = oz_popc(mine) - oz_popc(theirs); b = t > b ? t : b; }
                    else ++live;
                }
                L.best[i] = b; L.pend[i] = live;
            }
        }
        __syncthreads();
        for (int c0 = lo; c0 < hi; c0 += 64)                // a node all of whose children are finished boards is complete already
            if (c0 + lane < hi && !(L.link[c0 + lane] & 2) && L.pend[c0 + lane] == 0) sv_complete<WIN>(L, c0 + lane);
        __syncthreads();
        lo = hi; hi = base; --e;
    }
    for (;;) {                                              // the items: the live nodes of the last level
        const int i = lo + atomicAdd(&L.next, 1);
        if (i >= hi) break;
        int alpha = -OZ_SV_INF, beta = OZ_SV_INF, lk = L.link[i];
        if (lk & 2) continue;
        bool same = lk & 1;                                 // does the ancestor's viewpoint equal the item's?
        for (int p = (lk >> 2) - 1; p >= 0; p = (lk >> 2) - 1) {
            const int b = L.best[p];
            if (same) alpha = b > alpha ? b : alpha;
            else beta = -b < beta ? -b : beta;
            lk = L.link[p];
            same = same == (bool)(lk & 1);
        }
        if constexpr (WIN) {                                // ... and ends at the root (`same`: the root's viewpoint equals the item's)
            const int b = L.root;
            if (same) { alpha = b > alpha ? b : alpha; beta = RB < beta ? RB : beta; }
            else { beta = -b < beta ? -b : beta; alpha = -RB > alpha ? -RB : alpha; }
        }
        if (alpha < beta) {
            const uint64_t io = L.n_own[i], ip = L.n_opp[i];
            L.best[i] = sv_search(L, valid, corners, lane, io, ip, oz_legal(io, ip, valid), e, alpha, beta);
        }
        __threadfence_block();
        sv_complete<WIN>(L, i);
    }
    __syncthreads();
    if constexpr (WIN) {
        const int b = L.root;
        *bests = 0;
        *value = b < RB ? b : RB;
        return OZ_MINIMAX_NONE;
    }
    int v = OZ_MINIMAX_NONE;
    if (is_root) {
        const int b = L.best[idx];
        v = (L.link[idx] & 1) ? b : -b;
    }
    int mx = v;                                             // OZ_MINIMAX_NONE = INT32_MIN is below every value
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int y = __shfl_xor(mx, o, 64);
        mx = y > mx ? y : mx;
    }
    *bests = __ballot(is_root && v == mx);
    *value = mx;
    return v;
}

// Any position: -> the value of the move on square `lane` (OZ_MINIMAX_NONE off the legal set, and everywhere when there is nothing to play);
// *bests as sv_root, 0 for a finished board or a mover without a move; *value = S of the position (after the pass where the mover has none)
__device__ __forceinline__ int sv_position(SolveLds& L, uint64_t valid, uint64_t corners, int lane, uint64_t black, uint64_t white, int player,
                                           int empties, uint64_t* bests, int* value) {
    const uint64_t own = player == 1 ? black : white, opp = player == 1 ? white : black;
    const uint64_t legal = oz_legal(own, opp, valid);
    if (legal) return sv_root(L, valid, corners, lane, own, opp, legal, empties, bests, value);
    *bests = 0;
    const uint64_t theirs = oz_legal(opp, own, valid);
    if (theirs == 0) { *value = oz_popc(own) - oz_popc(opp); return OZ_MINIMAX_NONE; }
    uint64_t b2;
    int v2;
    sv_root(L, valid, corners, lane, opp, own, theirs, empties, &b2, &v2);
    *value = -v2;
    return OZ_MINIMAX_NONE;
}

// the four corners of the n x n board
inline uint64_t oz_solve_corners(int n) { return 1ULL | 1ULL << (n - 1) | 1ULL << (8 * (n - 1)) | 1ULL << (8 * (n - 1) + n - 1); }

// sign of S for `own` to move (after the pass where own has no move): -1 / 0 / +1, the same in every lane.  The root window (-1, +1) is symmetric,
// so the passed position's sign is minus the opponent's.  Every lane of the block must call it.
__device__ __forceinline__ int sv_sign(SolveLdsW& L, uint64_t valid, uint64_t corners, int lane, uint64_t own, uint64_t opp, int empties) {
    uint64_t b;
    int v;
    const uint64_t legal = oz_legal(own, opp, valid);
    if (legal) { sv_root<-1, 1>(L, valid, corners, lane, own, opp, legal, empties, &b, &v); return v; }
    const uint64_t theirs = oz_legal(opp, own, valid);
    if (theirs == 0) { const int d = oz_popc(own) - oz_popc(opp); return (d > 0) - (d < 0); }
    sv_root<-1, 1>(L, valid, corners, lane, opp, own, theirs, empties, &b, &v);
    return -v;
}
