/*
 * othellozero_amd.h -- C ABI of libothellozero_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for the self-play hot path of Galtvam/OthelloZero.  The
 * reference has no FFI layer (its boundary is Python duck typing), so each entry
 * point below cites the reference interface it replaces (file:line under the
 * reference tree); the othellozero_amd Python package binds them with ctypes and re-creates
 * the reference's Python surfaces on top.
 *
 * Conventions: plain pointers and sizes, caller-owned output buffers, int status
 * return (0 = OZ_OK) + oz_last_error() (thread-local string); no exceptions
 * cross the ABI.  Unless a parameter says "device pointer" every pointer is a
 * host pointer.  Boards: two uint64 bitboards, bit = row*8 + col for every board
 * size n in {4,6,8} (n x n corner of an 8x8 grid).  own/opp = channel 0/1 of a
 * mover-canonical state; black/white = absolute colours.  Squares are reported
 * as sq = row*8 + col; NN policy vectors are indexed row*n + col.
 * All objects are internally serialised (a mutex per object): concurrent calls
 * from ThreadWorker-style Python threads (workers.py:33-37,82-90) are safe.
 */
#ifndef OTHELLOZERO_AMD_H
#define OTHELLOZERO_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define OZ_OK 0
#define OZ_ERR_HIP 1       /* a HIP runtime call failed                         */
#define OZ_ERR_ARG 2       /* bad argument                                      */
#define OZ_ERR_CAPACITY 3  /* a per-game node table / record buffer overflowed      */
#define OZ_ERR_KEY 4       /* the reference would raise KeyError here           */
#define OZ_ERR_STATE 5     /* call sequence error                               */

/* Q accumulation regime (SURVEY.md R-FP): what `N*Q + value` promotes to */
#define OZ_QMODE_NEP50 0   /* NumPy >= 2: float32 once a float32 value arrives  */
#define OZ_QMODE_F64 1     /* NumPy 1.18.5 (requirements.txt:19): float64       */

/* per-game status after a select pass */
#define OZ_LEAF_IDLE 0       /* game slot not searching                          */
#define OZ_LEAF_TERMINAL 1   /* simulation ended on a finished board (MCTS/__init__.py:39-40) */
#define OZ_LEAF_EVAL 2       /* first visit: needs NN evaluation (MCTS/__init__.py:44-57)     */
#define OZ_LEAF_WAIT 3       /* free-running driver with a batch cap: the leaf is chosen and waits for a slot of a later batch */

const char* oz_last_error(void);
int oz_version(void);                 /* 230 */
int oz_device_count(void);
int oz_set_device(int device);       /* device used by objects created afterwards on this thread */

/* ------------------------------------------------------------------ rules
 * Batched Othello/__init__.py static board functions, one HIP thread per position. */
/* get_player_valid_actions (:208-214): legal[i] = bit mask of legal squares for the side holding own[i] */
int oz_rules_legal_moves(const uint64_t* own, const uint64_t* opp, int n, int count, uint64_t* legal);
/* flip_board_squares (:237-247) as the side holding own[i] on sq[i] (no legality check) */
int oz_rules_apply_moves(const uint64_t* own, const uint64_t* opp, const uint8_t* sq, int n, int count,
                         uint64_t* own_out, uint64_t* opp_out);
/* has_board_finished (:249-252), get_board_players_points / get_board_winning_player (:254-260; draw -> ch0) */
int oz_rules_status(const uint64_t* ch0, const uint64_t* ch1, int n, int count, uint8_t* finished,
                    int32_t* pts0, int32_t* pts1, int8_t* winner /* +1 ch0, -1 ch1 */);
/* OthelloGame.play (:136-159): flip, switch player, pass / finish logic. player: +1 BLACK, -1 WHITE */
int oz_rules_play(const uint64_t* black, const uint64_t* white, const int8_t* player, const uint8_t* sq, int n,
                  int count, uint64_t* black_out, uint64_t* white_out, int8_t* player_out, uint8_t* finished_out);

/* fixed-depth minimax (agents.py:27-41: GreedyOthelloAgent, dead code in the reference -- "play the move that gains the most discs" is depth 1 on
 * the disc count).  V(P, d), from the viewpoint of P's mover: T(P) if P is finished, else E(P) if d == 0, else max over legal a of
 * s * V(child(P, a), d - 1), the child as OthelloGame.play leaves it (s = +1 where the turn passed back, -1 otherwise; a finished child's T is taken
 * from its stored player, with the same s).  Depth counts moves made, passes are free.  int32 throughout, antisymmetric in the mover:
 *   OZ_MINIMAX_EVAL_DISCS     E = T = own discs - opponent discs
 *   OZ_MINIMAX_EVAL_WEIGHTED  E = sum of w(sq) over own - sum over opponent, T = 1000 * (own - opponent); w by (a, b) = (min(min(dr, dc), 2),
 *                             min(max(dr, dc), 2)), dr = min(r, n-1-r), dc = min(c, n-1-c): (0,0) 100, (0,1) -20, (1,1) -50, (0,2) 10, (1,2) -2,
 *                             (2,2) 1; |E| <= 576 < 1000 on 8x8, so a decided game outranks every static value
 * One wavefront per position, exact root values (every root move searched with a full window). */
#define OZ_MINIMAX_EVAL_DISCS 0
#define OZ_MINIMAX_EVAL_WEIGHTED 1
#define OZ_MINIMAX_MAX_DEPTH 6       /* a condition, not a knob: one launch must stay short */
#define OZ_MINIMAX_NONE INT32_MIN
/* batch entry (agents.py:27-41): the exact root value of every legal move of `count` positions; values[count][64] by square row*8+col
 * (OZ_MINIMAX_NONE off the legal set), bests[count] = mask of the maximal moves (0 when the mover has no move or the board is finished); any
 * output may be NULL */
int oz_rules_minimax(const uint64_t* black, const uint64_t* white, const int8_t* player, int n, int count, int depth, int eval,
                     int32_t* values, uint64_t* bests);

/* exact endgame solver (the reference has none: it trains on played outcomes only).  S(P), from the viewpoint of P's mover: own discs - opponent
 * discs if P is finished, else max over legal a of s * S(child(P, a)), the child as OthelloGame.play leaves it (s = +1 where the turn passed back,
 * -1 otherwise): oz_rules_minimax on OZ_MINIMAX_EVAL_DISCS without a horizon, on the library's own rules (flip-through and pass logic included);
 * empties are not awarded to the winner.  One wavefront per position; every root move's value is exact, not a bound. */
#define OZ_SOLVE_MAX_EMPTIES 12      /* a condition, not a knob: a whole 4x4 game, a 12-ply 8x8 endgame; the frame stack in LDS is sized by it */
/* batch entry: values[count][64] = S after the move on each legal square (OZ_MINIMAX_NONE elsewhere), bests[count] = mask of the maximal moves,
 * value[count] = S of the position, solved[count] = 1.  A position with more than max_empties empties (n*n - popcount(black | white)) is
 * skipped, not refused: solved 0, values all OZ_MINIMAX_NONE, bests 0, value 0.  A finished board or a mover without a move is solved with
 * bests 0 and no move value; its value is that of the finished board, or of the position after the pass.  Any output may be NULL.
 * OZ_ERR_ARG: max_empties outside 0..OZ_SOLVE_MAX_EMPTIES, a player that is not +1 / -1, discs off the n x n board or on one square twice. */
int oz_rules_solve(const uint64_t* black, const uint64_t* white, const int8_t* player, int n, int count, int max_empties,
                   int32_t* values /* [count][64] */, uint64_t* bests /* [count] */, int32_t* value /* [count] */, uint8_t* solved /* [count] */);
/* sign of S for the mover (after the pass where the mover has none): -1 / 0 / +1; positions above max_empties: solved 0, sign 0.
 * The same solver under the root window (-1, +1): the root's own best tightens every subtree's window and nothing more starts once a win is
 * found, so it costs a fraction of oz_rules_solve -- and says nothing about the moves.  What a search leaf needs (oz_mcts_set_solve_leaves).
 * Same argument checks and errors as oz_rules_solve. */
int oz_rules_solve_sign(const uint64_t* black, const uint64_t* white, const int8_t* player, int n, int count, int max_empties,
                        int8_t* sign /* [count] */, uint8_t* solved /* [count] */);
/* random openings (the reference has none: every game of a match starts from the one standard position, agents.py:71-84).  Opening `id` of
 * (plies, opening_seed): from the standard position with BLACK to move, while ply < plies and the game is not over, the mover OthelloGame.play left
 * plays oz_kth_bit(legal, oz_rng(opening_seed, id, ply, OZ_RNG_OPENING = 5) % popcount(legal)) -- RandomOthelloAgent's random.choice on a stream
 * of its own; a pass lets one side move twice in a row, a game that ends inside its opening stays ended with n_plies < plies.
 * Batch entry: the openings first_opening_id .. first_opening_id + count - 1 (count <= 2^22): the position each one reaches, who is to move, whether
 * the game is over, the squares played (row*8+col, 0 beyond n_plies) and their number.  Any output may be NULL.  What oz_arena_set_openings
 * plays, obtainable without an arena -- and handed back to one as lists through oz_arena_set_opening_moves.
 * OZ_ERR_ARG: plies outside 0..OZ_OPENING_MAX_PLIES, count outside 0..2^22. */
#define OZ_OPENING_MAX_PLIES 16
int oz_rules_random_openings(int n, int64_t count, int plies, uint64_t opening_seed, uint64_t first_opening_id,
                             uint64_t* black, uint64_t* white, int8_t* player, uint8_t* finished,
                             uint8_t* actions /* [count][OZ_OPENING_MAX_PLIES], 0 beyond n_plies */, int32_t* n_plies);
/* HIP-event timing of the kernel of every oz_rules_* batch call on the current device (default off: nothing is recorded); the read returns
 * the total since creation / the last reset and the number of launches (each may be NULL) */
int oz_rules_profile(int enable);
int oz_rules_profile_read(double* ms_total, int64_t* launches, int reset);

/* ------------------------------------------------------------------ network
 * NNetWrapper (Net/NNet.py:22-101) inference side; OthelloNN graph (Net/OthelloNN.py:42-56). */
typedef struct oz_net oz_net;
/* ONN with `channels` conv filters (reference: 512), for boards n x n, batches up to max_batch */
int oz_net_create(oz_net** out, int n, int channels, int max_batch);
/* BaseNN (Net/BaseNN.py:41-56): same trunk on ONE input plane (+1 mover, -1 opponent); 40 weight arrays, conv1 kernel (3,3,1,C) */
int oz_net_create_bnn(oz_net** out, int n, int channels, int max_batch);
/* deterministic integer-hash stand-in for predict() (test nets; formula in oracle/oz_oracle.c orc_stub_predict) */
int oz_net_create_stub(oz_net** out, int n, uint64_t salt, uint64_t keep_mask, int max_batch);
int oz_net_destroy(oz_net* net);
/* weights in keras Model.get_weights() order: 40 arrays for ONN (model.set_weights / get_weights, Net/NNet.py:98-101) */
int oz_net_num_weights(const oz_net* net);
int oz_net_weight_size(const oz_net* net, int index, int64_t* nelem);
int oz_net_set_weight(oz_net* net, int index, const float* data, int64_t nelem);
int oz_net_get_weight(const oz_net* net, int index, float* data, int64_t nelem);
/* a fresh OthelloNN as Keras initialises it (Net/OthelloNN.py:42-56: glorot_uniform kernels, zero biases, identity BatchNormalization) from a
 * deterministic stream keyed by `seed`; follow with oz_net_commit.  Not NumPy's numbers for that seed: read them back with oz_net_get_weight. */
int oz_net_init_random(oz_net* net, uint64_t seed);
/* arithmetic of the 3x3 convolutions and dense layers: 0 = exact fp32 matrix cores (v_mfma_f32_32x32x2_f32);
 * 1 = "f32 via 2 x fp16 split" (fp32-EQUIVALENT, not fp32): x = h1 + h2, products a1*b1 + a1*b2 + a2*b1 on v_mfma_f32_16x16x32_f16 with
 * fp32 accumulation.  An element is carried with an error of max(2^-24 |x|, 2^-25) inside the fp16 range, and oz_net_commit places every
 * tensor: each activation channel and each weight column gets an exact power-of-two scale -- activations from the maxima of |BN output| over
 * a fixed calibration set of positions -- so that its maximum lands in [2^-3, 2^-2): every element then has an absolute error <= 2^-23 of
 * its channel's (column's) calibration maximum, fp32's own relative precision where a dot product's large terms are (the scales are folded
 * into the BN scale / shift and the next layer's weights: the network function is unchanged; oz_net_get_scaling reads the exponents).
 * Guards, sticky, reported as OZ_ERR_STATE by oz_net_check / predict / selfplay_sync: an activation above 65504, or a pixel row whose
 * largest activation is non-zero and 2^15 or more below its channels' calibration maxima.  oz_net_commit also runs the self-check of
 * OZ_NET_OPT_SELF_CHECK.  Needs channels % 256 == 0 and channels <= 2048.
 * 2 = "f32 via 3 x bf16 split" (fp32-class): x = b1 + b2 + b3 with b1 = bf16(x), b2 = bf16(x - b1), b3 = bf16(x - b1 - b2) -- bf16 has fp32's
 * exponent range and 8 significand bits, so the three planes hold x exactly for 2^-100 <= |x| <= FLT_MAX (the bounds below that: b3_split in
 * othellozero_amd/csrc/oz_common.h): no scaling, no calibration, no guards, no refusal path.  A product keeps six of the nine cross terms (a3 b1, a1 b3, a2 b2, a2 b1, a1 b2, a1 b1 on v_mfma_f32_16x16x32_bf16, fp32
 * accumulation, small terms first); the dropped ones are <= 2^-25 of the product each, within fp32's own rounding of it.  conv3, conv4, fc1 and
 * fc2 run this way on k_gemm_b3 (oz_net_b3.h), conv1 + conv2 from the exact-fp32 pattern tables, the heads in fp32; networks with max_batch < 128
 * (the latency path: weight streams and split-K launches, not matrix rate) run precision 0's kernels unchanged.  Needs channels % 256 == 0.
 * Cost 6 MFMAs at 16x the fp32 rate: 2.67x the fp32 matrix roof.
 * Takes effect at the next oz_net_commit. */
int oz_net_set_precision(oz_net* net, int mode);
int oz_net_get_precision(const oz_net* net);
int oz_net_check(oz_net* net);
/* fold BN (epsilon 1e-3, moving statistics) + re-layout for the kernels; call after the last set_weight */
int oz_net_commit(oz_net* net);
/* NNetWrapper.predict (Net/NNet.py:70-87) for `count` canonical boards: pi[count][n*n] float32, v[count] float32 */
int oz_net_predict(oz_net* net, const uint64_t* own, const uint64_t* opp, int count, float* pi, float* v);
/* the same on boards in the reference's layout (Net/NNet.py:80-84): count x (n, n, 2) bytes NHWC, channel 0 = the mover, non-zero = a disc */
int oz_net_predict_boards(oz_net* net, const uint8_t* boards_nhwc, int count, float* pi, float* v);
/* Test entry: one forward launched the way the searches launch it -- grid and launch plan of `launch` positions, `count` of them live.  own / opp
 * hold `launch` boards; pi[launch][n*n] and v[launch] are in/out: uploaded before the forward, all `launch` rows downloaded after it (rows from
 * `count` on come back as they went in).  0 <= count <= launch, 1 <= launch <= max_batch (evaluation symmetry "mean": 8 * launch <= max_batch), else
 * OZ_ERR_ARG with nothing launched; count == 0 runs the launch.  Rows [0, count) equal oz_net_predict's bit for bit; the guard flag is reported as
 * oz_net_predict reports it.  Works for the stub network too. */
int oz_net_forward_launched(oz_net* net, const uint64_t* own, const uint64_t* opp, int count, int launch, float* pi, float* v);
/* timing hook for bench.py: run the forward `iters` times on `count` resident boards, return avg ms per forward (HIP events) */
int oz_net_time_forward(oz_net* net, int count, int iters, float* ms_avg);
/* HIP-event timing of the dominant launch on the stream it is launched on: the conv3 implicit GEMM when conv1 + conv2
 * run as a table gather-sum (the default), else the conv2 implicit GEMM; oz_net_profiled_layer says which (3 / 2) */
int oz_net_profile(oz_net* net, int enable /* 0 off, 1 the dominant launch only, 2 every kernel of the forward */);
int oz_net_profile_read(oz_net* net, double* conv2_ms_total, int64_t* conv2_launches);
/* per-kernel totals since creation (or the last reset), slots: 0 input (k_lut_ids, or the conv1 kernel) 1 conv2 (table
 * gather-sum or GEMM) 2 conv3 3 conv4 4 fc1 (+ split-K reduce) 5 fc2 6 heads; only slots enabled by the profile mode advance */
#define OZ_NET_KERNELS 7
int oz_net_profile_kernels(oz_net* net, double* ms_total /* [OZ_NET_KERNELS] */, int64_t* launches /* [OZ_NET_KERNELS] */, int reset);
int oz_net_profiled_layer(oz_net* net, int* layer);
/* how conv1 / conv2 are evaluated.  2 (default): both from tables over the 3^9 neighbourhood patterns of the discrete
 * input planes (no GEMM for conv2; tables rebuilt by oz_net_commit); 1 (precision f16x2, max_batch > 32): conv1 from its table
 * inside conv2's operand gather, conv2 an MFMA GEMM (bit-identical to 0); 0: conv1 kernel + conv2 MFMA GEMM; -1: back to the
 * default.  Takes effect at the next forward. */
int oz_net_set_tables(oz_net* net, int mode);
/* Persistent exact-key evaluation cache of this network: (own, opp) -> (pi, v) for up to ~`entries` positions in HBM (rounded up to a
 * power of two of 4-way buckets; n*n + 6 words per entry; 0 frees it).  The generalisation of the reference's per-search
 * `_predict_cache` (othelo_mcts.py:13,82-88: one dict per OthelloMCTS instance) to every self-play engine that is created with
 * oz_selfplay_config.eval_cache = 1 on this network -- across batches, games and refilled slots.  A hit changes no bit of any result
 * (a position's (pi, v) is independent of the batch it is evaluated in); the cache is emptied by oz_net_commit (new weights) and by an
 * oz_net_set_tables that changes the form of conv1 / conv2 (the table form adds conv2's products in another order than the GEMM forms).
 * Engines that share a cached network may run one after the other (a second engine starts warm) but NOT concurrently: their enqueues are
 * serialised by the network's mutex, their streams are not, and an entry one engine replaces could be read half-written by the other. */
int oz_net_set_eval_cache(oz_net* net, int64_t entries);
int oz_net_eval_cache_stats(oz_net* net, int64_t* entries, int64_t* lookups, int64_t* hits, int64_t* inserts);
/* ---- evaluation symmetry: evaluate a position in a dihedral symmetry of the board (opt-in; off, every forward issues exactly the launches it
 * issued before; the reference has none).  AlphaZero and KataGo evaluate every leaf in a randomly chosen orientation, so that a network that is
 * only approximately equivariant does not show the search the same orientation bias in every game.  Here the orientation is no draw per call:
 *     f_sym(own, opp) = S_t^-1( f( S_t(own), S_t(opp) ) ),   t = oz_eval_symmetry(seed, own, opp) = sm64(sm64(seed ^ own) + opp) >> 61
 * (csrc/oz_common.h), a pure function of the position and a seed that lives in the NETWORK.  The network stays a deterministic function of the
 * board, so batch-position bit-identity, the searches' de-duplication, the evaluation cache and the transposition tables hold unchanged; a
 * search evaluates a position once, so "random per position" differs from "random per evaluation" only across searches -- give every iteration
 * a new seed.  Orientations are numbered as the training symmetries (oz_symmetry_table; 7 = the identity): cell (r, c) of the board in
 * orientation t is cell src_t(r, c) of the original, and pi[src_t(r, c)] = pi_t[r * n + c].
 * OZ_EVAL_SYM_RANDOM: one orientation per position, two small launches around the forward.  OZ_EVAL_SYM_MEAN: all eight, pi and v their float32 mean
 * 0.125f * (((x_0 + x_1) + x_2) + ... + x_7) with x_t mapped back to the original cells -- the smoother evaluator for matches and measurements at 8x
 * the network work; a call of `count` positions then needs 8 * count <= max_batch (OZ_ERR_ARG otherwise), so a search needs a network with
 * max_batch >= 8 * games * leaves_per_step.
 * oz_net_set_eval_symmetry takes the network's mutex, synchronises the device, allocates the scratch boards (and outputs) on first use and empties
 * the evaluation cache; modes other than the three are refused.  The setting is part of the network: it survives oz_net_set_weight and
 * oz_net_commit, and every caller of the network sees it -- the searches, the self-play drivers, the arenas, oz_net_predict / _predict_boards and
 * oz_net_time_forward (which then times the transform kernels too).  oz_net_get_activation and oz_net_get_info then describe the TRANSFORMED batch
 * (RANDOM: the boards in their orientations, in call order; MEAN: rows 8 i + t = position i in orientation t).  Commit-time calibration, the f16x2
 * self-check and the table builds never see the option.  Engines that share a network must not run concurrently (as with the evaluation cache). */
enum { OZ_EVAL_SYM_OFF = 0, OZ_EVAL_SYM_RANDOM = 1, OZ_EVAL_SYM_MEAN = 2 };
int oz_net_set_eval_symmetry(oz_net* net, int mode, uint64_t seed);
int oz_net_get_eval_symmetry(oz_net* net, int* mode, uint64_t* seed);
/* HIP-event timing of the two kernels of the option on the stream they are launched on: enable != 0 switches it on for the forwards that follow;
 * ms_total[2] / launches[2] (either may be null) receive the totals so far, slot 0 = k_sym_boards, 1 = k_sym_policy; reset != 0 zeroes them. */
int oz_net_eval_symmetry_profile(oz_net* net, int enable, double* ms_total /* [2] */, int64_t* launches /* [2] */, int reset);
/* host only, no GPU needed: the two functions above as the kernels evaluate them.  t_out[i] = oz_eval_symmetry(seed, own[i], opp[i]);
 * out[i] = boards[i] in orientation t[i] on an n x n board (bits outside the n x n corner are 0; t outside 0 .. 7 is refused). */
int oz_eval_symmetries(uint64_t seed, const uint64_t* own, const uint64_t* opp, int64_t count, int32_t* t_out);
int oz_sym_boards(const int32_t* t, int n, const uint64_t* boards, int64_t count, uint64_t* out);
/* diagnostics switch, per network (default 0): the 3x3 convolutions of precision f16x2 on the one-barrier-per-k-tile main loop instead of
 * the ping-pong loops (4-phase on the 256-row tile, 2-phase on the 192- and 128-row tiles).  Same accumulation order, bit-identical results: the reference form the LDS-DMA race screen
 * (tools/pp_race_check.py, test_pingpong_conv_loop_bit_identical_to_simple_loop) compares the ping-pong schedule against. */
#define OZ_NET_OPT_SIMPLE_LOOP 1
/* precision f16x2, all take effect at the next oz_net_commit: the powers of two the per-channel calibration maxima (ACT, default -2) and the
 * per-column weight maxima (W, default -2) are moved below -- the defaults are the measured optimum of tools/target_probe.py, other values
 * are test hooks and experiments -- and log2 of the low-side guard's row threshold (default -17; <= -100 switches the guard off) */
#define OZ_NET_OPT_ACT_TARGET_LOG2 2
#define OZ_NET_OPT_LOW_GUARD_LOG2 3
/* precision f16x2, default 1: oz_net_commit runs its calibration positions through the f16x2 kernels and through the exact-fp32 kernels and
 * fails with OZ_ERR_STATE when max |d pi| or max |d v| exceeds 8e-6 (a network that amplifies rounding beyond what 22 of fp32's 24 bits hold
 * within 1e-5: a conditioning problem no range guard can see; healthy networks measure <= 4e-6, of which up to 3e-6 is the fp32 kernels' own
 * rounding); 0 = off, 2 = measure only; oz_net_self_check reads what the last commit measured */
#define OZ_NET_OPT_SELF_CHECK 4
#define OZ_NET_OPT_W_TARGET_LOG2 5
/* diagnostics switch, per network (default 0), precision f32: the 3x3 convolutions of large batches never take the 256 x 256 tile (GmBig) and run
 * on the 128 x 128 one (GmStd) like every other layer.  Both tiles add every output element's products in the same order: bit-identical
 * results -- the screen test_f32_big_tile_bit_identical_to_the_standard_tile compares them.  Takes effect at the next forward. */
#define OZ_NET_OPT_F32_STD_TILE 6
/* precision f16x2, medium networks (32 < max_batch < ~1000), default 0: 1 = the k-splits of the 3x3 convolutions are chosen for LATENCY (a cost
 * model of grid rounds x k-tiles per block + reduce slabs) instead of "the fewest slices that fill 192 blocks".  For callers whose batches are
 * usually far smaller than max_batch -- an arena with the library's de-duplication and evaluation cache evaluates ~15 leaves per step, and a
 * launch of one-slice 144-k-tile blocks takes 205 us whatever it holds: bench.py's config5, 31 -> 45 games/s -- at a price for full batches
 * (407 -> 430 us per 512-leaf step).  A per-network constant: a position's (pi, v) does not depend on the size of the call; two networks with
 * different settings agree to rounding.  Takes effect at the next oz_net_commit. */
#define OZ_NET_OPT_LATENCY_SPLITS 7
/* diagnostics switch, per network (default 0), precision f16x2, max_batch > 32: conv3 runs on the row tile of this height (128, 192 or 256)
 * instead of the one the forward picks for the call (fewest grid rounds x tile height).  All three add every output element's products in the
 * same order: bit-identical results -- test_conv3_tiles_bit_identical compares them.  Takes effect at the next forward. */
#define OZ_NET_OPT_CONV3_TILE 8
/* diagnostics switch, per network (default 1), precision f16x2: main loop of the 128 x 256 tile (conv3 of calls of <= 455 leaves, conv4 and fc1 of
 * medium networks): 1 = one phase per k-tile on three LDS stages (round 6), 2 = the 2-phase loop on two stages (round 5).  Bit-identical results. */
#define OZ_NET_OPT_LOW_LOOP_PHASES 9
/* diagnostics switch, per network (default 0), precision bf16x3: the tile of conv3 / conv4 -- 0 = the launcher picks (256 x 256 where the network's
 * capacity fills the chip on it, else 128 x 256), 128 / 256 = that tile.  Bit-identical results: the screen of the two tiles. */
#define OZ_NET_OPT_B3_TILE 10
/* diagnostics switch, per network (default 0), precision bf16x3: the mixed plan of conv3 / conv4 -- the layer's leading rows on 256 x 256 tiles, the rows
 * behind them on 128 x 256 tiles, two launches.  0 = the launcher picks (from the network's capacity: the big tile for whole rounds of the 256 CUs, the small
 * one for what is left, where that is at least one big round plus at most one small round and prices below either tile alone -- an 8x8 network of 4096
 * boards: conv3's first 131072 rows), negative = never mix, a positive multiple of 256 = that many leading rows of conv3 and conv4 on the big tile whatever
 * the pricing and the k split say (ignored where it does not lie inside the layer's capacity rows) -- lets a small network put the boundary anywhere.
 * OZ_NET_OPT_B3_TILE 128 / 256 overrides it: that tile for the whole launch.  Bit-identical results.  Takes effect at the next forward. */
#define OZ_NET_OPT_B3_MIX_ROWS 11
int oz_net_set_option(oz_net* net, int option, int value);
int oz_net_self_check(oz_net* net, double* max_dpi, double* max_dv, int* positions);
/* precision f16x2: the exponents chosen at the last commit.  which = 0 .. 4: per-channel activation exponents of the conv1, conv2, conv3,
 * conv4 (channels each) and fc1 (1024) outputs; which = 5 .. 9: per-column weight exponents of conv2, conv3, conv4 (channels), fc1 (1024), fc2 (512) */
int oz_net_get_scaling(oz_net* net, int which, int32_t* out, int64_t nelem);
/* launch facts of the last forward: OZ_NET_INFO_CONV3_TILE_ROWS = the row-tile height conv3 ran on.  Precision f16x2: 256 / 192 / 128, chosen per call
 * from the capacity the caller launches with (256 at bench.py's batch cap of 3640 leaves; 128 when the call fits one grid round on that tile, e.g.
 * an arena's ~430-leaf batches), 128 x 128 tiles on the latency path (max_batch <= 32).
 * Precision bf16x3: 256 where the whole layer ran on the 256 x 256 tile, else 128 -- a layer on the mixed plan (OZ_NET_KERNEL_B3_MIXED) reports the SMALLEST
 * row tile of the plan that ran, 128; how many of its rows went to the 256-row tile is OZ_NET_INFO_LAYER_BIG_ROWS.
 * Precision f32: what oz_gemm_f32_launch really launched -- 256 (GmBig: a 3x3 convolution whose 256 x 256 tiles fill the chip, e.g. every call
 * of a max_batch = 4096 network), 128 (GmStd: smaller networks, or OZ_NET_OPT_F32_STD_TILE), 64 (the weight-stream kernel of layers with at
 * most 64 rows: one-position networks). */
#define OZ_NET_INFO_CONV3_TILE_ROWS 1
/* precision f16x2: the guard bits (1 = an activation above the fp16 range, 4 = a low row) raised ON THE CALIBRATION POSITIONS by the self-check of the
 * last oz_net_commit -- 0 for a healthy network.  With OZ_NET_OPT_SELF_CHECK = 1 such a commit fails; with 2 (measure only) it succeeds and this
 * says what happened.  The device flag is cleared by the commit that reported it. */
#define OZ_NET_INFO_SELF_CHECK_GUARD 2
/* the arithmetic the network's GEMM layers really run in: the precision mode, except that a precision-2 (bf16x3) network of max_batch < 128 reports 0 --
 * its layers are the exact-fp32 latency kernels (see oz_net_set_precision) */
#define OZ_NET_INFO_ARITHMETIC 3
/* the launch plan of the last forward, per layer l = 1 .. 5 (conv2, conv3, conv4, fc1, fc2): the row-tile height of the kernel that ran the layer
 * (64 / 128 / 192 / 256; 0 = no row tiles: the table gather), the number of k-slices its k loop was cut into (1 = unsplit; slices of layers
 * 1 .. 4 are added by the precision's fixed-order reduce kernel, those of fc2 by the heads kernel), and which kernel / main loop it was
 * (OZ_NET_KERNEL_*).  What a test matrix needs to show that it ran the configuration it names.  OZ_NET_INFO_LAYER_BIG_ROWS: precision bf16x3, how
 * many leading rows of the layer's capacity belong to 256-row tiles -- 0 for OZ_NET_KERNEL_B3, every row for OZ_NET_KERNEL_B3_BIG, the boundary of the two
 * launches for OZ_NET_KERNEL_B3_MIXED (whose OZ_NET_INFO_LAYER_TILE_ROWS is 128, the smaller tile); 0 in the other precisions. */
#define OZ_NET_INFO_LAYER_TILE_ROWS(l) (16 + (l))
#define OZ_NET_INFO_LAYER_KSLICES(l) (32 + (l))
#define OZ_NET_INFO_LAYER_KERNEL(l) (48 + (l))
#define OZ_NET_INFO_LAYER_BIG_ROWS(l) (64 + (l))
enum {
    OZ_NET_KERNEL_NONE = 0,
    OZ_NET_KERNEL_F32_SKINNY = 1,        /* k_gemm_f32_skinny: the weight stream of layers with at most 64 rows */
    OZ_NET_KERNEL_F32_STD = 2,           /* k_gemm_f32<GmStd>, board-major row tiles */
    OZ_NET_KERNEL_F32_STD_PIXMAJOR = 3,  /* k_gemm_f32<GmStd>, pixel-major row tiles (conv2 as a GEMM) */
    OZ_NET_KERNEL_F32_BIG = 4,           /* k_gemm_f32<GmBig> */
    OZ_NET_KERNEL_LUT = 5,               /* conv1 + conv2 as the table gather, one thread per (pixel, 8 channels) */
    OZ_NET_KERNEL_LUT_XCD = 6,           /* ... one table slice per XCD (512 filters) */
    OZ_NET_KERNEL_LUT_XCD_INLINE = 7,    /* ... with the pattern ids computed inside the gather (precision f32, max_batch <= 32) */
    OZ_NET_KERNEL_H2_SMALL2 = 10, OZ_NET_KERNEL_H2_SMALL = 11, OZ_NET_KERNEL_H2_BIGPP = 12, OZ_NET_KERNEL_H2_BIGPP_LUT = 13,
    OZ_NET_KERNEL_H2_MIDPP = 14, OZ_NET_KERNEL_H2_LOWPP1 = 15, OZ_NET_KERNEL_H2_LOWPP = 16, OZ_NET_KERNEL_H2_BIG = 17, OZ_NET_KERNEL_H2_MID = 18,
    OZ_NET_KERNEL_H2_THIN2 = 19, OZ_NET_KERNEL_H2_THIN = 20, OZ_NET_KERNEL_H2_THIN4W = 21,     /* k_gemm_h2 on the tile configuration of that name */
    OZ_NET_KERNEL_B3 = 30,               /* k_gemm_b3 (128 x 256) */
    OZ_NET_KERNEL_B3_BIG = 31,           /* k_gemm_b3_big (256 x 256) */
    OZ_NET_KERNEL_B3_MIXED = 32          /* k_gemm_b3_big over the layer's leading rows, then k_gemm_b3 over the rest (OZ_NET_OPT_B3_MIX_ROWS) */
};
int oz_net_get_info(oz_net* net, int what, int* value);
/* host only, no GPU needed: the plan a precision-bf16x3 network of board size n (6 / 8), `channels` filters and capacity max_batch makes for its layer
 * 1 .. 5 (conv2 .. fc2) when the layer's k loop has `kslices` slices, under OZ_NET_OPT_B3_TILE = tile_opt and OZ_NET_OPT_B3_MIX_ROWS = mix_rows_opt: *kernel =
 * OZ_NET_KERNEL_B3 / _B3_BIG / _B3_MIXED, *big_rows as OZ_NET_INFO_LAYER_BIG_ROWS reports them, *small_tiles = the 128-row tiles of the capacity's remaining
 * rows.  The function the forward itself asks. */
int oz_net_b3_plan(int n, int channels, int max_batch, int layer, int kslices, int tile_opt, int mix_rows_opt, int* kernel, int64_t* big_rows, int64_t* small_tiles);
/* Diagnostics: a read-only view of the last forward (the inference side's counterpart of oz_trainer_get_activation).  layer 0 .. 3 = the outputs
 * of conv1 .. conv4, 4 / 5 = fc1 / fc2 (the trainer's numbering); a row is a (board, pixel) index of the last forward -- oz_net_predict's boards in
 * call order -- and out[rows][channels] receives rows first_row .. first_row + rows - 1 as float64: EXACTLY the numbers the consuming kernel
 * multiplies.  fp32 rows as they are; rows in the h2 layout as (h1 + h2) x 2^-aexp[channel] (the exact inverse of the channel's power of two);
 * rows in the b3 layout as b1 + b2 + b3.  fc2 of a forward that left its k-slices to the heads kernel: what that kernel forms -- the slices added
 * in slice order in fp32, then scale, shift and ReLU.  OZ_ERR_STATE (with a message) for a layer the forward never materialises -- conv1 when it is
 * folded into a table -- and before the first forward after a commit; OZ_ERR_ARG for rows outside the last forward and for a stub network.
 * Takes the network's mutex; changes no state. */
int oz_net_get_activation(oz_net* net, int layer, int64_t first_row, int64_t rows, double* out /* [rows][channels] */);

/* ------------------------------------------------------------------ search
 * OthelloMCTS / MCTS (othelo_mcts.py:9-88, MCTS/__init__.py:19-187): num_games independent
 * instances, one wavefront per instance, tables resident in HBM. */
typedef struct oz_mcts oz_mcts;
/* node_cap: states per instance (each a fixed-stride record: header + one 24-byte edge per legal move, 1024 B on 8x8).
 * (oz_version 200: the `edge_cap` arguments / field of version 100 are gone -- the edges live inside the node records since round 2) */
int oz_mcts_create(oz_mcts** out, int n, int num_games, int node_cap, double c, int q_mode);
int oz_mcts_destroy(oz_mcts* m);
int oz_mcts_reset(oz_mcts* m, int game /* -1 = all */);                 /* fresh OthelloMCTS() */
/* cross-game leaf de-duplication of oz_mcts_simulate's batches (default on; results are identical either way) */
int oz_mcts_set_dedup(oz_mcts* m, int enable);
/* roots of the next simulations: canonical boards (othelo_mcts.py:22-26); active[i]=0 leaves slot i idle */
int oz_mcts_set_roots(oz_mcts* m, const uint64_t* own, const uint64_t* opp, const uint8_t* active);
/* OthelloMCTS.simulate x nsims for every active slot, leaves evaluated in one batch per step by `net` */
int oz_mcts_simulate(oz_mcts* m, oz_net* net, int nsims);
/* the same split for a host-side evaluator (any Python object with .predict):
 *   select -> leaves -> [caller evaluates OZ_LEAF_EVAL slots] -> backup */
int oz_mcts_select(oz_mcts* m);
int oz_mcts_leaves(oz_mcts* m, int32_t* status, uint64_t* own, uint64_t* opp);
int oz_mcts_backup(oz_mcts* m, const float* pi /* [num_games][n*n] */, const float* v /* [num_games] */);
/* value returned by the last simulate() of each slot and its dynamic type (0 int, 1 float32, 2 float64) */
int oz_mcts_last_value(oz_mcts* m, double* value, int32_t* vtype, int32_t* depth);
/* N(state, action) of the current root for every square (MCTS/__init__.py:73-84): counts[g][64];
 * rc[g]: 0 ok, 1 root unknown (all zero), 2 KeyError (root never selected from) */
int oz_mcts_root_counts(oz_mcts* m, int32_t* counts, uint64_t* legal, int32_t* rc);
/* get_policy_action_probabilities (othelo_mcts.py:51-67) of every game's current root: policy[g] = float64 (n, n) row-major.
 * temperature != 0: N ** (1 / T) on the legal squares over their np.sum (NumPy's summation order; or 1 if it is 0); temperature == 0: one-hot of
 * a best square, of the max-count squares in row-major order the one tie_draws[g] % (how many) picks (random.choice in the reference; null: the
 * first).  rc[g] as in oz_mcts_root_counts; rc 2 (KeyError in the reference) leaves a zero row. */
int oz_mcts_policy(oz_mcts* m, double temperature, const uint64_t* tie_draws, double* policy, int32_t* rc);
/* table inspection (parity tests): nodes of slot `game` in expansion order */
int oz_mcts_num_nodes(oz_mcts* m, int32_t* num_nodes /* [num_games] */);
int oz_mcts_dump_node(oz_mcts* m, int game, int index, uint64_t* own, uint64_t* opp, int32_t* Ns, uint64_t* legal,
                      int32_t* N /*64*/, double* Q /*64*/, uint8_t* qtag /*64: 1 = float32-typed*/, double* P /*64*/);
/* counters since creation: [0] simulations [1] node visits [2] expansions [3] terminal hits [4] uniform-prior fallbacks */
int oz_mcts_stats(oz_mcts* m, int64_t* out5);

/* ---- leaf-parallel search: K = leaves_per_step descents per game and step under virtual loss (opt-in; the default 1 is the search above, bit for bit)
 * For one game and one step, `left` = simulations of the simulate call still to run: min(K, left) descents, one after the other, each exactly
 * the descent above except that an edge (s, a) which k > 0 earlier descents of this step took is seen as N' = N + k,
 * Q' = ((double)N * Q - (double)k) / (double)(N + k) (float64; every in-flight descent counts as one visit that returned -1; k == 0 reads
 * the stored bits) and the node as Ns + k(s) visits: U = Q' + (c * P) * (sqrt(Ns + k(s)) / (1 + N')).  A descent that ends on a finished
 * board takes its place with the integer value; one that ends on an unknown state is a leaf, unless an earlier leaf of the step is the same
 * board: then it is discarded (no simulation; counted as a collision) and the step closes for that game.  All leaves of all games form ONE
 * network batch in (game, j) order; then per game, j ascending, leaf j is expanded and its value backed up along path j.  A simulate call
 * runs steps until every active game has done exactly nsims simulations; a game's result depends on its own state only.
 * K > 1 evaluates every leaf: no cross-game de-duplication and no evaluation cache (results would be identical), so
 * leaves_evaluated == expansions.  OZ_QMODE_NEP50 at K > 1: the view is float64 in both regimes and every stored value goes through the
 * same update as at K = 1, which the reference's traces hold through these kernels (oz_mcts_use_wide_kernels); it has no replay of its own.
 * OZ_ERR_ARG: k outside 1 .. OZ_MCTS_MAX_LEAVES_PER_STEP, a network whose max_batch < num_games * k (here for the drivers, in
 * oz_mcts_simulate for a bare search).  OZ_ERR_STATE: a change while a step is pending / after the first driver call, and for k > 1 the
 * host-evaluator split (oz_mcts_select / leaves / backup) and the free-running driver oz_selfplay_run_steps (its batches are full already). */
#define OZ_MCTS_MAX_LEAVES_PER_STEP 16
/* the first k > 1 (or oz_mcts_use_wide_kernels) allocates the per-(game, j) arrays, sized for OZ_MCTS_MAX_LEAVES_PER_STEP whatever k is:
 * 8.9 KB per game (the paths are 8 KB of it: 36 MB at 4 096 games) plus the batch and (pi, v) rows for num_games x 16 leaves */
int oz_mcts_set_leaves_per_step(oz_mcts* m, int k);
int oz_mcts_get_leaves_per_step(oz_mcts* m, int* k);
/* diagnostic: run k = 1 through the leaf-parallel kernels */
int oz_mcts_use_wide_kernels(oz_mcts* m, int enable);
/* out[0] game-steps run by the leaf-parallel kernels, out[1] descents discarded on a collision, out[2] leaves handed to the network */
int oz_mcts_wide_stats(oz_mcts* m, int64_t* out3);

/* ---- solved leaves: exact values for leaves with few empties (opt-in; 0 = off is the search above, launch for launch; the reference has none)
 * In every step, after the evaluator has written the step's (pi, v) rows and the evaluation cache has taken them (the cache keeps the NETWORK's
 * v: engines that share it may run without this option), a row whose board has at most max_empties empties gets v = (float)sign(S), S the
 * exact value of the position for the side to move (oz_rules_solve_sign); pi stays the network's.  A DRAW IS 0.0f -- the search's own terminal
 * rule, which gives a drawn final board to whichever side is channel 0 there, is not reproduced.  The value is backed up like any network value
 * (its type follows q_mode).  Every distinct row is solved once per step: de-duplicated games share it as they share the network's.  Works at
 * any leaves_per_step, with root noise, move sampling, the evaluation cache and every driver.
 * OZ_SOLVE_LEAVES_MAX_EMPTIES is below OZ_SOLVE_MAX_EMPTIES on purpose: a step waits for its slowest row, and it may hold hundreds.
 * OZ_ERR_ARG: max_empties outside 0 .. OZ_SOLVE_LEAVES_MAX_EMPTIES (the object stays as it was).  OZ_ERR_STATE: oz_mcts_select / oz_mcts_backup
 * while the option is on (the host-evaluator split takes the caller's (pi, v) as they are). */
#define OZ_SOLVE_LEAVES_MAX_EMPTIES 10
int oz_mcts_set_solve_leaves(oz_mcts* m, int max_empties);        /* 0 = off (default) .. OZ_SOLVE_LEAVES_MAX_EMPTIES; takes effect at the next step */
int oz_mcts_get_solve_leaves(oz_mcts* m, int* max_empties, int64_t* rows_solved /* since create */);      /* either may be NULL */
/* HIP-event timing of the solving kernel (default off); the read returns the total and the launches since creation / the last reset */
int oz_mcts_solve_leaves_profile(oz_mcts* m, int enable);
int oz_mcts_solve_leaves_profile_read(oz_mcts* m, double* ms_total, int64_t* launches, int reset);

/* ---- value signs: a backup whose signs are right across passes and finished boards (opt-in; OZ_VALUE_SIGNS_REFERENCE, the default, is the
 * search above bit for bit).  The reference's rule (MCTS/__init__.py:39-40,68-71) negates the value once per level on the way up, and returns
 * -reward of a finished board seen from channel 0.  Two things differ from a sound negamax: a finished child is not
 * colour-swapped, so a move that wins the game on the spot stores Q = -1 in its parent (and a draw counts as channel 0's win); and after a
 * pass the same side moves again, yet the value is negated there too, so every value that crosses a pass arrives above it with the wrong sign.
 * With OZ_VALUE_SIGNS_SOUND, for a descent along the edges 0 .. depth-1, sigma_d = 1 where the sides swapped after edge d and 0 where the
 * same side moves again (a pass, or the game is over), and V_L the leaf's value for the side to move at the leaf (the network's v, the solved
 * sign, or sign(discs own - discs opp) in {-1, 0, +1} on a finished board, an integer value like the reference's):
 *     edge d gets  V_L * (-1)^(sigma_d + .. + sigma_{depth-1}),   oz_mcts_last_value reports minus what edge 0 got (at depth 0: -V_L).
 * Nothing else changes: the Q update and its type rule, N, Ns, PUCT, the tie rule, the virtual loss of the leaf-parallel search, the tables,
 * de-duplication, the caches and the random streams.  It combines with every other option; root values, value targets, recorded surprise,
 * the resign rule and Gumbel's completed Q read what the search stores.  One mismatch stays: a drawn game is 0 here and +-1 (draw -> BLACK)
 * in the records' z.  OZ_ERR_STATE: the tree holds nodes (a tree mixes neither rule: right after create or after oz_mcts_reset(-1) only). */
#define OZ_VALUE_SIGNS_REFERENCE 0
#define OZ_VALUE_SIGNS_SOUND 1
int oz_mcts_set_value_signs(oz_mcts* m, int mode);
int oz_mcts_get_value_signs(oz_mcts* m, int* mode);
/* the definition on the host, no device needed: out[d] = what edge d stores, d = 0 .. depth-1 (depth <= 64; bit d of swap_bits = sigma_d, read
 * in sound mode only); *last_value (may be NULL) = what oz_mcts_last_value reports.  leaf_value = V_L above in BOTH modes: the reference's
 * -v / -reward at the leaf is part of its rule. */
int oz_search_backup_values(int mode, uint64_t swap_bits, int depth, double leaf_value, double* out, double* last_value);
/* V_L of a finished board for `own`, the side the descent leaves to move: sound sign(discs own - discs opp); reference +1 unless own has fewer
 * discs, -1 then (MCTS/__init__.py:39-40 returns its negation) */
int oz_search_terminal_value(int mode, uint64_t own, uint64_t opp, int* value);

/* ---- proofs: exact values kept as proofs and backed up the tree (opt-in, on top of OZ_VALUE_SIGNS_SOUND; off, every result stays bit for
 * bit).  The MCTS-Solver step (Winands et al. 2008; "certainty propagation").  Values are -1 / 0 / +1 or unknown (OZ_PROOF_UNKNOWN).
 * States: an edge (S, a) may carry a proven value e(S, a) for the side to move at S; a node may carry an own proven value (set only where it
 *   was expanded from a solved leaf).  val(S) = the own value if set; else +1 if any legal edge has e = +1; else max e if every legal edge is
 *   known; else unknown.
 * Exact results of a descent (V_L = the value for the side to move where the descent ends, as in "value signs"): (1) it ends on a finished
 *   board; (2) it stops on a proof (below); (3) the leaf is expanded while solve_leaves = E > 0 and has <= E empties: v is the exact sign, and
 *   the new node's own value is set to it.  Every other leaf proves nothing.
 * Descent, at the node S at level d: the finished-board check and the table lookup come first.  If d > 0 and val(S) is known the descent ends
 *   here like a finished board with V_L = val(S), no edge of S visited (the root never stops: a move must receive visits).  Candidates: the
 *   legal edges with e == val(S) if that is known (the root only); else, and where that set is empty, the legal edges with e != -1; none of
 *   those either: the legal set, and the search reports a corrupt table.  U is the search's formula (in-flight view, root noise, float64 left
 *   to right) with Q = (double)e in place of the (adjusted) Q where e is known; the first maximum among the candidates is taken.  If the taken
 *   edge's e is known the descent ends right after the move (depth d + 1, like a finished board) with V_L = sigma_d ? -e : e; the child is
 *   not looked up.
 * Backup: Q / N / Ns of every level exactly as in sound mode.  Then, for an exact result, from the bottom with x = V_L, for d = depth-1 .. 0:
 *   x = sigma_d ? -x : x; e(path[d]) = x (a known, different value reports a corrupt table); stop if val(path[d].node) is unknown, else
 *   x = that value.  With leaves_per_step = K the K backups of a step run in their order; proofs are read in selection, written in backup.
 * Stored Q stays the running mean and oz_mcts_root_values / oz_mcts_root_counts / the move read the raw statistics as before.  Proofs live in
 * 32 bytes per node beside the records, persist with the tree and go with oz_mcts_reset.  Supported: oz_mcts_simulate, oz_selfplay_run,
 * the arena, any leaves_per_step, root noise, move sampling, playout cap, solve_leaves, the recorded rows and targets, resignation.
 * OZ_ERR_STATE: the tree holds nodes; the signs are OZ_VALUE_SIGNS_REFERENCE; the Gumbel search or forced playouts are on (and those refuse
 * an object with proofs); oz_selfplay_run_steps and oz_selfplay_stagger refuse an engine with proofs. */
#define OZ_PROOF_UNKNOWN (-128)
int oz_mcts_set_proofs(oz_mcts* m, int enable);
int oz_mcts_get_proofs(oz_mcts* m, int* enabled);
/* node `index` of game `game` (indices as oz_mcts_dump_node): edge[64] by square (OZ_PROOF_UNKNOWN off the legal set), *node_value the own
 * value, *node_val val(S).  OZ_ERR_STATE on an object without the option. */
int oz_mcts_dump_proofs(oz_mcts* m, int game, int index, int8_t* edge, int8_t* node_value, int8_t* node_val);
/* the current roots: edge [G][64], val [G], rc [G] (0, or 1 where the game is idle or its root is not in the table) */
int oz_mcts_root_proofs(oz_mcts* m, int8_t* edge, int8_t* val, int32_t* rc);
/* summed over the games: [0] edges proven [1] descents ended on a proven edge [2] descents ended on a proven node [3] roots whose value became
 * known (zeros on an object without the option) */
int oz_mcts_proof_stats(oz_mcts* m, int64_t* out4);
/* the rule on the host, no device needed.  A node's edge proofs are two masks by square: state = 2 * hi bit + lo bit, 0 unknown, 1 loss,
 * 2 draw, 3 win.  oz_search_proof_value: val(S).  oz_search_proof_candidates: the candidate set of a node of value node_val (pass
 * OZ_PROOF_UNKNOWN below the root), *inconsistent = 1 where it fell back to the legal set.  oz_search_proof_backup: the loop of the backup
 * over a path of `depth` levels (level d: the node's legal[d], lo[d], hi[d], own_value[d], the square taken and sigma[d]); lo / hi are
 * updated in place, out3 = levels marked, edges newly proven, 1 where level 0's value became known; *conflict = 1 where a known edge differed. */
int oz_search_proof_value(uint64_t legal, uint64_t lo, uint64_t hi, int own_value, int* value);
int oz_search_proof_candidates(uint64_t legal, uint64_t lo, uint64_t hi, int node_val, uint64_t* candidates, int* inconsistent);
int oz_search_proof_backup(const uint8_t* sigma, const int32_t* square, int depth, int leaf_value, const uint64_t* legal, uint64_t* lo, uint64_t* hi,
                           const int8_t* own_value, int32_t* out3, int* conflict);

/* ---- selection: first-play urgency (FPU) reduction, a visit-scaled exploration constant and a prior-first first visit (opt-in; with every
 * part off, the default, every kernel, table, record and launch is the search above).  The reference's rule U = Q + c P sqrt(Ns) / (1 + N)
 * values an unvisited move at Q = 0, keeps c constant, and sends the first visit of a fresh node (sqrt(0) = 0: all U equal) to the first legal
 * square.  Three parts, each switchable on its own (KataGo / Leela Chess Zero's FPU; AlphaZero's and Lc0's c(s)).
 * At a node S at level d of a descent, for a legal square a:
 *   N'_a, Q'_a = the statistics as selection sees them today: the stored bits where no descent of this step is in flight on the edge, else
 *     the virtual-loss view N + k, ((double)N * Q - (double)k) / (double)(N + k);  n = Ns + k(S), the node's visits in the same view;
 *   P_a = the prior selection uses today: the stored P, or Pn = (1 - eps) * P + eps * eta at depth 0 of an armed noisy root;
 *   vhat(S) = the value the node's expansion backed up, for the side to move at S: the network's v, or the solved sign under solve_leaves
 *     (header word 3 of the node, what the Gumbel kernels keep there; oz_mcts_node_value reads it).
 * float64, no contraction, every product, sum and quotient rounded on its own in the order written:
 *   OZ_SELECT_GROWTH (cpuct_base > 0, cpuct_factor >= 0):  c_S = c + cpuct_factor * log(((1.0 + (double)n) + cpuct_base) / cpuct_base), the
 *     logarithm the library's correctly rounded one (error below 2^-85);  off: c_S = c.  AlphaZero: (19652, 1); Lc0 about (38739, 3.9).
 *   OZ_SELECT_PRIOR_FIRST:  r = n > 0 ? sqrt((double)n) : 1.0;  off: r = sqrt((double)n).  A fresh node's first visit then goes to the first
 *     maximum of c_S * P_a (of F + c_S * P_a under FPU; F is the same for all squares).
 *   OZ_SELECT_FPU (both reductions in [0, 4]):  f = fpu_root_reduction at d == 0, else fpu_reduction (KataGo: 0.2, and 0.1 or 0 at the
 *     root).  With visited(a) := N'_a > 0:  SN = the integer sum of N'_a;  SQ = tree-sum over the 64 squares of
 *     (visited ? (double)N'_a * Q'_a : 0.0);  SP = tree-sum of (visited ? P_a : 0.0);  V = (vhat + SQ) / (1.0 + (double)SN);
 *     F = V - f * sqrt(SP), then F = -1.0 where F < -1.0.  Every legal edge with N'_a == 0 takes Q'_a := F; edges with visits keep theirs.
 *     tree-sum = the balanced binary tree over the squares 0 .. 63 (zeros off the legal set): x_i <- x_{2i} + x_{2i+1}, six rounds.
 *   U_a = Q'_a + (c_S * P_a) * (r / (double)(1 + N'_a)).
 * Under proofs a known edge value replaces Q'_a after the FPU step, as before.  First-maximum tie break, the candidate sets of the proofs,
 * the in-flight view, the stored Q / N / Ns, the backup and the move rules do not change.
 * Supported: oz_mcts_simulate at any leaves_per_step, oz_mcts_select / leaves / backup, oz_selfplay_run, the arena, both value signs, proofs
 * and proof play, root noise, move sampling, playout cap, solve_leaves, every recorded row and target, resignation.
 * OZ_ERR_ARG: a value outside the ranges above (NaN included) of a part that is on, unknown flag bits.  OZ_ERR_STATE: the tree holds nodes
 * (every node of such a tree keeps vhat: right after create or after oz_mcts_reset(-1) only) or a step is pending; the Gumbel search or
 * forced playouts are on (their quota and pruning restate PUCT with the constant c) -- and those refuse an object with the option, whichever
 * is set second; oz_selfplay_run_steps and oz_selfplay_stagger refuse an engine with it (the free-running kernels stay as they are).
 * flags == 0 switches the option off; a part that is off keeps no parameters (the getter reports 0 for them). */
#define OZ_SELECT_FPU 1
#define OZ_SELECT_GROWTH 2
#define OZ_SELECT_PRIOR_FIRST 4
int oz_mcts_set_selection(oz_mcts* m, int flags, double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor);
int oz_mcts_get_selection(oz_mcts* m, int* flags, double* fpu_reduction, double* fpu_root_reduction, double* cpuct_base, double* cpuct_factor);
/* the rule on the host, no device needed.  oz_search_select_c: c_S of a node with n visits.  oz_search_select_scores: one node from its rows by
 * square -- N, Q = N', Q' above (the caller's view), P = the prior in use, Ns = n, level = d -> U[64] (-inf off the legal set); F, V (0 with
 * FPU off), c_S and pick (the first maximum; -1 without a legal square) may be NULL. */
int oz_search_select_c(double c, double cpuct_base, double cpuct_factor, int n, double* out);
int oz_search_select_scores(const int32_t* N, const double* Q, const double* P, uint64_t legal, int Ns, double vhat, int level, double c, int flags,
                            double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor, double* U, double* F, double* V,
                            double* c_S, int32_t* pick);

/* ---- root noise: Dirichlet noise on the root prior, AlphaZero's exploration inside the search (opt-in; off, every result stays bit for bit)
 * P'(root, a) = (1 - eps) P(root, a) + eps eta_a, eta ~ Dir(alpha) over the root's legal moves, fresh for every searched move.
 * STORED PRIORS ARE NEVER MODIFIED: the node tables are transposition tables that persist across the moves of a game, so the noise is applied
 * at selection time only, at depth 0 of a descent, to the root it was drawn for (an Othello position cannot recur below itself, so "depth 0"
 * and "is the root" coincide).  In float64, no contraction, on an armed root and a legal square sq:
 *     Pn = (1.0 - eps) * P + eps * eta[sq]          two products, one sum, as written
 *     U  = Q + (c * Pn) * (sqrt(Ns) / (1 + N))      the shape of the search above; at leaves_per_step > 1 with the virtual-loss view of Ns, N, Q
 * Deeper levels, unarmed roots and eps == 0 use the stored P; the first maximum still wins ties and the reference's Ns == 0 quirk (all U equal:
 * the first legal square) is unchanged.  The host-evaluator split (oz_mcts_select / leaves / backup) honours the noise too.
 * Lifetime: noise belongs to ONE root board of ONE slot.  Giving the slot a different board drops it (oz_mcts_set_roots with another board, the
 * engines' root kernels, the move of the free-running driver); arming again replaces it.  The arena and the evaluation games never use noise.
 * The sampler (device side, one lane per square, counter based, no state): with u(sq, i) = the unit draw of the library's stream
 * (seed, game id, ply, 3 + 256 sq + 65536 i) and w(sq, i) = 1.0 - u(sq, i) in (0, 1], Gamma(alpha) of a legal square is Marsaglia-Tsang with the
 * alpha < 1 boost, all float64:
 *     a = alpha < 1 ? alpha + 1 : alpha;  d = a - 1.0/3.0;  cc = 1.0 / sqrt(9.0 * d);  g = d
 *     for t in 0 .. 15:  x = sqrt(-2.0 * log(w(sq, 3t))) * cos(2.0 * pi * u(sq, 3t + 1));  v = 1.0 + cc * x;  if v <= 0: continue;  v = v * v * v
 *                        if log(w(sq, 3t + 2)) < 0.5 * x * x + d - d * v + d * log(v): g = d * v; break
 *     if alpha < 1: g *= pow(w(sq, 48), 1.0 / alpha)
 * eta[sq] = g / S, S = the sum of g over the (n, n) array in NumPy's pairwise order (zeros off the legal set); S == 0 or not finite: 1 / count
 * on the legal squares.  Squares off the legal set are exactly 0; a root with one legal move gets exactly 1.0.
 * OZ_ERR_ARG: alpha not in [0.01, 100], eps not in [0, 1] (NaN included), an eta outside [0, 1].  OZ_ERR_STATE: a change while a step is pending
 * (oz_mcts_select without oz_mcts_backup) / after an engine's first driver call.  eps == 0 disarms and allocates nothing; the first arming
 * allocates 513 B per game (2 MB at 4 096 games) and moves the object's descents to the noise-aware instantiation of the kernels. */
/* host-supplied noise for a bare search: eta[num_games][64] by square (row*8+col), 0 off the legal set; armed[g] != 0 arms slot g for its
 * CURRENT root (null: every active slot); eta == NULL or eps == 0 disarms all */
int oz_mcts_set_root_noise(oz_mcts* m, double eps, const double* eta, const uint8_t* armed);
/* device-drawn noise for the current roots of the active slots, keyed (seed, game_ids[g], plies[g]) */
int oz_mcts_sample_root_noise(oz_mcts* m, double alpha, double eps, uint64_t seed, const uint64_t* game_ids, const int32_t* plies);
/* what is set: eta[num_games][64], armed[num_games], *eps (each may be NULL); an object that never armed noise reads zeros */
int oz_mcts_get_root_noise(oz_mcts* m, double* eta /* [num_games][64] */, uint8_t* armed /* [num_games] */, double* eps);

/* ---- move sampling: a ~ N(root, a)^(1/T) for the opening plies, AlphaZero's move rule (opt-in; off, every record stays bit for bit)
 * The reference plays the arg-max of the root's visit counts, or (coin > e_greedy) a uniformly random legal move.  With move sampling the
 * greedy branch of the coin draws the move of a game whose ply < plies in proportion to N^(1/T) instead; later plies and the explore branch
 * are unchanged (pure AlphaZero: e_greedy = 1).  One definition for the engines and for the bare search, on the device, one wave per game,
 * one lane per square.  With N[sq] the root's visit counts, mx = max N (>= 1), T the temperature and ONE unit draw
 * u = the library's stream (seed, game id, ply, 4) -- stream 4 is none of the root-noise streams 3 + 256 sq + 65536 i -- in float64, no
 * contraction, squares in ascending sq = row*8 + col:
 *     inv     = 1.0 / T
 *     w[sq]   = N[sq] == 0 ? 0.0 : pow((double)N[sq] / (double)mx, inv)      legal squares only; a max-count square gets exactly 1.0
 *     cum[sq] = the running sum of w, added one square after the other in ascending order (c = c + w[sq]); the order is part of the definition
 *     r       = u * c_total                                                  c_total = cum of the last legal square
 *     action  = the first legal square with cum[sq] > r; if there is none (u * c rounded up to c), the last legal square with w > 0
 * Dividing by mx keeps pow in (0, 1] for every T.  A square with N == 0 is never chosen; a root with one visited move always plays it.
 * OZ_ERR_ARG: temperature not in [0.01, 100] (NaN included), plies not in [0, 64]. */
/* the sampled move of the current roots of the active slots, keyed (seed, game_ids[g], plies[g]): action[g] = the square, or -1 where rc[g] != 0
 * (rc as oz_mcts_root_counts: 1 unknown root, 2 expanded but never selected from) and on an idle slot */
int oz_mcts_sample_moves(oz_mcts* m, double temperature, uint64_t seed, const uint64_t* game_ids, const int32_t* plies,
                         int32_t* action /* [num_games], sq or -1 */, int32_t* rc /* [num_games] */);

/* ---- playout cap: most self-play moves on a small simulation budget, a random share on the full one (opt-in, KataGo's playout cap
 * randomization; off, every record stays bit for bit).  Most moves of a self-play game exist only to carry the game forward; only a fully
 * searched move is worth a training example.  With the cap (fast_sims, full_prob), 2 <= fast_sims <= num_simulations, 0 < full_prob <= 1:
 *     u      = the unit draw of the library's stream (seed, game id, ply, OZ_RNG_PLAYOUT = 6) -- stream 6 is none of 0 .. 5 and none of
 *              the root-noise streams 3 + 256 sq + 65536 i
 *     the searched self-play move of (game id, ply) is FULL iff u < full_prob; its budget is num_simulations when full, fast_sims otherwise
 * The budget counts NEW simulations of that move, as num_simulations always did; the node tables persist across the moves of a game,
 * unchanged.  ONE function, oz_playout_budget (csrc/oz_common.h), is what the kernels and oz_playout_budgets evaluate.
 *   * the record of a fast move has pad[0] == 1, of a full move 0 (the first spare byte of oz_record; the layout does not change).  A fast
 *     record is not a training example: oz_replay_append_selfplay / oz_replay_append_records leave it out, and so do the Python consumers.
 *   * a fast move draws no root noise: its descents read the stored priors and oz_selfplay_root_noise reports its slot unarmed (noise
 *     widens a policy target, and a fast move has none).  The e-greedy coin, the explore branch and move sampling are untouched, keyed by
 *     ply as ever.
 *   * full_prob == 1: every move is full and every flag 0 -- the bytes of the engine without the option.
 *   * never touched: the arena, matches and evaluations, the bare oz_mcts, and the rounds of oz_selfplay_stagger (every slot plays at
 *     sims_pre, flag 0, and is counted neither full nor fast). */
/* the budgets of `count` (game id, ply) pairs, on the host (no device needed): out[i] = sims or fast_sims.  fast_sims == 0: off, every
 * out[i] = sims.  OZ_ERR_ARG: sims < 2, fast_sims not 0 and outside [2, sims], full_prob outside (0, 1] (NaN included), a negative ply. */
int oz_playout_budgets(uint64_t seed, const uint64_t* game_ids, const int32_t* plies, int64_t count, int sims, int fast_sims,
                       double full_prob, int32_t* out /* [count] */);

/* ---- resignation: stop a decided self-play game early, play a fixed share out regardless as an audit (opt-in, AlphaGo Zero's and KataGo's;
 * off, every launch, record and row stays bit for bit).  A decided game otherwise keeps running full searches until the last disc is placed,
 * and its last records carry the outcome of noise played after the game was decided.  With (v, r, min_ply, keep_prob), 0 < v <= 1,
 * 1 <= r <= 8, 0 <= min_ply <= 64, 0 <= keep_prob <= 1, every game holds side in {-1, 0, +1} and streak, both 0 at its start.  After the
 * search of the self-play move of (game id, ply i), mover p_i = +-1, root value q_i (oz_root_term / oz_root_mean over the RAW counts, "value
 * targets" below), all in float64:
 *     b = p_i * q_i                                                   the root value from BLACK's side
 *     c = b >= v ? +1 : b <= -v ? -1 : 0                               NaN: 0
 *     c == 0:    side = 0, streak = 0;   c == side:  streak = min(streak + 1, 255);   otherwise:  side = c, streak = 1
 *     trigger_i = streak >= r && i >= min_ply
 * ONE function, oz_resign_step (csrc/oz_common.h), is what the move kernels and oz_resign_scan evaluate.  Every searched self-play move
 * updates the state: the fast moves of a playout cap and the moves of the explore branch too.
 * A game is EXEMPT iff the unit draw of the library's stream (seed, game id, 0, OZ_RNG_RESIGN = 9) is < keep_prob -- stream 9 is none of
 * 0 .. 8, none of the root-noise streams 3 + 256 sq + 65536 i and none of the Gumbel streams 7 + 256 sq (oz_resign_exempt).
 *   * a game that is not exempt, at its first trigger, where move i does not end the game by itself: move i is chosen, logged and played as
 *     ever, then the game ends as ADJUDICATED: winner = side, final_black / final_white = the board after move i, every record of the game
 *     has z = +1 iff winner == player and pad[1] == 1 (the second spare byte of oz_record; the layout does not change).  games_completed,
 *     moves, records, the visit, value, policy and surprise rows and the refill behave exactly as at a natural end.
 *   * where move i ends the game by itself the natural result stands, pad[1] == 0, and the game is not counted as adjudicated.
 *   * an exempt game remembers its first trigger (ply and side; one at the game's last move counts) and plays on; its records have
 *     pad[1] == 0.  At its end it is counted in games_exempt, and where it triggered in exempt_triggered, its remembered ply added to
 *     exempt_trigger_ply_sum, and in exempt_wrong iff the natural winner (a draw goes to BLACK, as in oz_record.z) is not the remembered
 *     side: exempt_wrong / exempt_triggered is the rule's false-positive rate, the number v is tuned by.
 *   * keep_prob == 1: every game is exempt -- the bytes of the engine without the option, and the counters still measure the rule.
 *   * never touched: the arena, matches and evaluations, the bare oz_mcts.  pad[2] stays 0 (it is proof play's). */
typedef struct {
    int64_t games_adjudicated;      /* games ended by the rule */
    int64_t adjudicated_plies_sum;  /* the plies those games were played for (their records) */
    int64_t games_exempt;           /* exempt games completed */
    int64_t exempt_triggered;       /* of them, games in which the rule triggered */
    int64_t exempt_wrong;           /* of them, games whose natural winner is not the side the first trigger called */
    int64_t exempt_trigger_ply_sum; /* the plies of those first triggers, summed over exempt_triggered */
} oz_resign_stats;
/* the first trigger of `games` sequences on the host (no device needed): game g is the next plies_per_game[g] entries of players (+-1) and
 * values, ply 0 first; trigger_ply[g] = the ply, trigger_side[g] = the side it calls the game for, or -1 and 0 where the rule never
 * triggers.  OZ_ERR_ARG: v outside (0, 1], r outside [1, 8], min_ply outside [0, 64] (NaN included), a negative length, a player not +-1. */
int oz_resign_scan(const int8_t* players, const double* values, const int32_t* plies_per_game, int64_t games, double v, int r, int min_ply,
                   int32_t* trigger_ply /* [games] */, int8_t* trigger_side /* [games] */);
/* out[i] = 1 where the game with id game_ids[i] is exempt under (seed, keep_prob), else 0; on the host (no device needed).  OZ_ERR_ARG:
 * keep_prob outside [0, 1] (NaN included). */
int oz_resign_exempt(uint64_t seed, const uint64_t* game_ids, int64_t count, double keep_prob, uint8_t* out /* [count] */);

/* ---- forced playouts: forced playouts and policy target pruning for the noisy root (opt-in, KataGo's; off, every launch, record and row stays
 * bit for bit).  At ~100 simulations a move the noise favours but the prior dismisses gets a visit or two and is dropped: if it is good the
 * search never finds out, if it is bad its visits stay in the row policy_target="visits" trains on.  With the forcing constant k (KataGo: 2.0;
 * accepted: [0, 16], 0 = off), all in float64, no contraction, as written; Pn(sq) = (1.0 - eps) * P + eps * eta[sq] is the root noise's view:
 * FORCING -- only at depth 0 of a descent from a root whose noise is armed (where the descent already reads Pn).  With the descent's view
 * Ns + ks, N', Q' (virtual loss included) and U computed for a legal square as ever:
 *     nf = sqrt((k * Pn) * (double)(Ns + ks))
 *     if (N' > 0 && (double)N' < nf) U = +INFINITY
 * The first maximum in ascending square order still wins, among several infinities too.  A child with N' == 0 is never forced; the Ns == 0 quirk
 * gives nf == 0 and stays.  Deeper levels, unarmed roots, the fast moves of a playout cap (they draw no noise), arenas, matches and evaluations
 * are never forced.  At leaves_per_step > 1 the in-flight descents count in N', so forcing spreads over them.  The host-evaluator split
 * (oz_mcts_select / leaves / backup) honours forcing as it honours noise.
 * PRUNING -- of a root's count row, when the move is chosen, on a root whose noise is armed, k > 0.  From the stored N[sq], Q[sq], P[sq], Ns of the
 * root record (no virtual loss exists then), eta, eps and c:
 *     root  = sqrt((double)Ns)
 *     star  = the first legal square, ascending, with N == max N
 *     Ustar = Q[star] + (c * Pn[star]) * (root / (double)(1 + N[star]))
 *     for every other legal sq with N[sq] > 0:
 *         F    = (int)ceil(sqrt((k * Pn[sq]) * (double)Ns))                     the most forcing can have added
 *         gap  = Ustar - Q[sq]
 *         if !(gap > 0.0):  Np = N[sq]                                          its Q alone reaches Ustar: keep
 *         else:
 *             need = ((c * Pn[sq]) * root) / gap - 1.0
 *             m    = need < (double)N[sq] ? max(0, (int)ceil(need)) : N[sq]     NaN / inf: keep
 *             Np   = min(N[sq], max(N[sq] - F, m))
 *         if (Np < N[sq] && Np <= 1) Np = 0                                     a child cut down to one visit is dropped
 *     pruned[star] = N[star];  pruned[sq] = N[sq] where N[sq] == 0;  pruned[sq] = 0 off the legal set
 * star keeps its count, so a pruned row is never all zero.  ONE function, oz_forced_prune (csrc/oz_common.h), is what the kernels and
 * oz_forced_playouts_prune evaluate.
 * MOVE CHOICE IS EXPLORATION, THE TARGET IS WHAT IS LEARNED: only the row that becomes the policy target (the engine's visit rows with
 * record_visits = 1, oz_mcts_pruned_counts) is pruned.  oz_selfplay_last_counts, oz_mcts_root_counts, the arg-max, the tie rule, move sampling
 * and the e-greedy branch read the raw counts: the games change through forcing alone.
 * OZ_ERR_ARG: k outside [0, 16] (NaN included).  OZ_ERR_STATE: k > 0 on an object without root noise, a change while a step is pending / after
 * an engine's first driver call.  A refused call leaves the object as it was. */
/* oz_forced_prune over `count` rows, on the host (no device needed): N, Q, P, eta, pruned are [count][64] by square, legal and Ns [count].
 * OZ_ERR_ARG also for eps outside [0, 1], a NaN c, a negative N or Ns. */
int oz_forced_playouts_prune(const int32_t* N, const double* Q, const double* P, const double* eta, const uint64_t* legal, const int32_t* Ns,
                             int64_t count, double c, double eps, double k, int32_t* pruned /* [count][64] */);
/* the forcing constant of a bare search: needs root noise armed before (oz_mcts_set_root_noise / oz_mcts_sample_root_noise with eps > 0) */
int oz_mcts_set_forced_playouts(oz_mcts* m, double k);
int oz_mcts_get_forced_playouts(oz_mcts* m, double* k);
/* oz_mcts_root_counts with the policy target's rows: pruned on the slots whose noise is armed (k > 0), raw on the others */
int oz_mcts_pruned_counts(oz_mcts* m, int32_t* counts, uint64_t* legal, int32_t* rc);

/* ---- Gumbel search: the root rule of Gumbel AlphaZero (Danihelka et al., ICLR 2022) for a bare search (opt-in; off, every launch and every result
 * stays bit for bit).  At 16 .. 100 simulations over up to 33 legal moves a visit-count row is mostly "where PUCT happened to look".  The Gumbel
 * root samples max_considered moves without replacement (Gumbel-top-k of g + logit), spends the budget on them by sequential halving, and yields
 * pi' = softmax(logit + sigma(completed Q)), a policy target that improves on the prior at any budget.  It replaces root noise, forced playouts
 * and move sampling.  All arithmetic is float64, no contraction, squares in ascending sq = row*8 + col, the first maximum wins; ONE set of
 * functions (csrc/oz_common.h: oz_gumbel_value, oz_gumbel_schedule, oz_gumbel_acc / _vmix / _sigma / _x / _score) is what the kernels and the
 * host-only twins below evaluate.
 * DRAW       g[sq] = -log(-log(w)) on the legal squares, 0 elsewhere; w = u, the unit draw of the library's stream (seed, game id, ply,
 *            OZ_RNG_GUMBEL + 256 sq), OZ_RNG_GUMBEL = 7 -- none of the streams 0 .. 6 and none of the root-noise streams 3 + 256 sq + 65536 i.
 *            u is a multiple of 2^-53 in [0, 1): its one endpoint u == 0 maps to w = 2^-54, so w lies in [2^-54, 1 - 2^-53] and g in
 *            [-3.63, 36.8], always finite.
 * SCHEDULE   considered_visits(m, n), a list of length n: for m <= 1 it is 0, 1, .., n-1; else L = ceil(log2 m), visits = [0] * m, k = m, and
 *            while the list is short: extra = max(1, n / (L k)) times append visits[0 .. k-1] and increment those k entries, then k = max(2, k / 2);
 *            truncated to n.  m = 4, n = 16: 0 0 0 0 1 1 1 1 2 2 3 3 4 4 5 5.  The host builds the tables of m = 1 .. max_considered at the budget
 *            and uploads them once.
 * ROOT       at an armed root with stored priors P, edge statistics N (type tag masked) and Q, N0 = the snapshot of N taken at arming (0 for a
 *            root not yet in the table) and vhat = the root's own value (header word 3 of its record, below):
 *                n(a)     = N(a) - N0(a)        this search's visits: a position cannot recur below itself, so only root picks change root edges
 *                sumN     = sum N;  maxN = max N;  Pvis = sum over N > 0 of P;  PQ = sum over N > 0 of P * Q        one legal square after the other
 *                vmix     = sumN == 0 ? vhat : (vhat + (sumN / Pvis) * PQ) / (1 + sumN)        Pvis == 0 (only zero-prior squares visited): that term is 0
 *                qhat(a)  = N(a) > 0 ? Q(a) : vmix
 *                sigma(a) = ((c_visit + maxN) * c_scale) * ((qhat(a) + 1.0) * 0.5)
 *                score(a) = (g[a] + log(P(a))) + sigma(a)                log(0) = -inf: such a square wins only where nothing else is legal
 * PICK       at depth 0 of a descent from an armed root: t = sum n(a), m_eff = min(max_considered, number of legal moves),
 *            cv = t < budget ? considered_visits(m_eff, budget)[t] : max n(a); the first maximum of score over the legal a with n(a) == cv, or over
 *            all legal squares if none matches.  Deeper levels and unarmed roots are PUCT exactly as without the option.
 * MOVE       the first maximum of score over the legal a with n(a) == max n.
 * POLICY     pi'[a] = exp(x[a] - max x) / sum exp(..), x = log(P) + sigma over the legal squares, the sum in ascending order, each element rounded
 *            once to float32, 0 off the legal set (every x == -inf: 1 / count).
 * STORAGE    a search with the option on keeps, in header word 3 of every node it expands (8 bytes that are 0 otherwise), the value the expansion
 *            backs up before negation: the network's v of the node, or the exact one where solve_leaves replaced it.  Hence the option is switched
 *            on over an EMPTY tree only: at creation, or after oz_mcts_reset(-1); OZ_ERR_STATE otherwise.  Once on, the object stays on the
 *            Gumbel-aware kernels (772 B per game plus the tables, at the first call); an object that never switched it on allocates nothing and
 *            launches the kernels it always launched.
 * Lifetime: as root noise -- the draw and the snapshot belong to ONE root board of ONE slot; oz_mcts_set_roots with another board disarms the
 * slot, arming again replaces them.  The host-evaluator split (oz_mcts_select / leaves / backup) honours the option.
 * OZ_ERR_ARG: max_considered outside [1, 64], c_visit < 0, c_scale <= 0 (NaN included; both at most 1e9), budget outside
 * [1, OZ_GUMBEL_MAX_BUDGET], a g that is not finite.  OZ_ERR_STATE: a non-empty tree at the first call, a step pending, an object that has armed
 * root noise or runs leaves_per_step > 1 / the wide kernels -- and, once the option is on, oz_mcts_set_root_noise / oz_mcts_sample_root_noise
 * with eps > 0, oz_mcts_sample_moves, oz_mcts_set_leaves_per_step(k > 1) and oz_mcts_use_wide_kernels(1).  A refused call leaves the object as
 * it was. */
#define OZ_GUMBEL_MAX_BUDGET 65536
/* host-supplied draws: g[num_games][64] by square; armed[g] != 0 arms slot g for its CURRENT root and snapshots N0 (null: every active slot);
 * g == NULL sets the parameters and disarms every slot */
int oz_mcts_set_gumbel(oz_mcts* m, int max_considered, double c_visit, double c_scale, int budget, const double* g /* [num_games][64] or NULL */,
                       const uint8_t* armed);
/* device-drawn g for the current roots of the active slots, keyed (seed, game_ids[g], plies[g]) */
int oz_mcts_sample_gumbel(oz_mcts* m, int max_considered, double c_visit, double c_scale, int budget, uint64_t seed, const uint64_t* game_ids,
                          const int32_t* plies);
/* what is set (each pointer may be NULL); an object without the option reads zeros */
int oz_mcts_get_gumbel(oz_mcts* m, double* g /* [num_games][64] */, uint8_t* armed /* [num_games] */, int32_t* N0 /* [num_games][64] */,
                       int32_t* max_considered, double* c_visit, double* c_scale, int32_t* budget);
/* the improved policy rows and the moves of the current roots: rc[g] 0 = ok; 1 = the root is not in the table; 3 = the slot is idle or not armed
 * (then a zero row and action -1) */
int oz_mcts_gumbel_policy(oz_mcts* m, float* pi /* [num_games][64] */, int32_t* action /* [num_games] */, int32_t* rc /* [num_games] */);
/* the scores the last oz_mcts_gumbel_policy evaluated, -inf off the legal set (inspection) */
int oz_mcts_gumbel_scores(oz_mcts* m, double* score /* [num_games][64] */);
/* header word 3 of a node (indices as oz_mcts_dump_node): its own value where it was expanded under the option -- or under the selection
 * option ("selection": vhat) --, 0.0 elsewhere */
int oz_mcts_node_value(oz_mcts* m, int game, int index, double* value);
/* the host-only twins (no device needed).  oz_gumbel_considered_visits: out[n], m in [1, 64].  oz_gumbel_draws: g[count][64] of `count` roots from
 * their keys and legal sets.  oz_gumbel_from_units: g of given unit draws u in [0, 1) (the endpoint mapping above).  oz_gumbel_root: pick, move and
 * pi'[count][64] of `count` roots from their rows by square; score[count][64] and gaps[count][2] may be NULL -- gaps = the distance between the
 * best and the second-best score among the candidates of the pick and of the move (inf with one candidate). */
int oz_gumbel_considered_visits(int m, int n, int32_t* out /* [n] */);
int oz_gumbel_draws(uint64_t seed, const uint64_t* game_ids, const int32_t* plies, const uint64_t* legal, int64_t count, double* g /* [count][64] */);
int oz_gumbel_from_units(const double* u, int64_t count, double* g);
int oz_gumbel_root(const int32_t* N, const int32_t* N0, const double* Q, const double* P, const double* g, const uint64_t* legal, const double* vhat,
                   int64_t count, int max_considered, double c_visit, double c_scale, int budget, int32_t* pick, int32_t* move, float* pi,
                   double* score, double* gaps);

/* ------------------------------------------------------------------ self-play
 * execute_episode (training.py:26-72) for num_games concurrent games in lock step. */
typedef struct oz_selfplay oz_selfplay;
typedef struct {
    int32_t n;              /* board size 4/6/8 */
    int32_t num_games;      /* concurrent game slots */
    int32_t sims;           /* num_simulations per move (>= 2) */
    int32_t q_mode;         /* OZ_QMODE_* */
    double c;               /* degree_exploration */
    double temperature;     /* policy_temperature: 0 -> max-visit with stream tie-break, else first max of N */
    double e_greedy;        /* coin <= e_greedy -> greedy */
    uint64_t seed;          /* RNG streams keyed (seed, global game id, ply) */
    uint64_t first_game_id; /* global id of slot 0 (multi-GPU sharding: rank*num_games) */
    uint64_t game_id_stride;/* id step when a slot is refilled (world_size*num_games) */
    int32_t refill;         /* 1: a finished slot immediately starts a new game */
    int32_t node_cap;       /* per-game node table capacity (0 = sims*61+64) */
    int32_t reserved0;      /* 0 */
    int32_t record_cap;     /* move records kept for export (0 = num_games*64*4) */
    int32_t dedup;          /* OZ_DEDUP_*: cross-game leaf de-duplication -- a board that several games reach in the same batch is evaluated
                             * once and every one of them reads the same (pi, v) row; changes no record, count or statistic, only leaves_evaluated */
    int32_t batch_cap;      /* free-running driver: leaves per network batch (0 = none), see oz_selfplay_set_batch_cap */
    int32_t eval_cache;     /* 1: leaves whose board is in the network's evaluation cache (oz_net_set_eval_cache) take their (pi, v) from it and
                             * need no batch slot; evaluated leaves are inserted.  0 (default): every leaf is evaluated by the network */
    int32_t record_visits;  /* 1: keep every move's root visit counts N(s, a) next to its record (oz_selfplay_visits) -- the search's
                             * visit distribution pi, the AlphaZero policy target; 16 KB per slot + 256 B per record of device memory.
                             * 0 (default): nothing is kept or allocated */
} oz_selfplay_config;
#define OZ_DEDUP_DEFAULT 0  /* = on */
#define OZ_DEDUP_ON 1
#define OZ_DEDUP_OFF 2

/* one move of one game; 8-fold symmetry expansion (training.py:13-23) happens in oz_examples_expand */
typedef struct {
    uint64_t black, white;  /* absolute board BEFORE the move (per-move snapshot) */
    uint64_t final_black, final_white; /* board at the end of that game (the reference's aliased view, T2) */
    uint64_t game_id;
    uint8_t ply;
    uint8_t action;         /* sq = row*8+col */
    int8_t player;          /* mover: +1 BLACK, -1 WHITE */
    int8_t z;               /* +1 if winner == mover else -1 (draw -> BLACK wins) */
    uint8_t greedy;         /* 1 = greedy branch of the coin (arg-max), 0 = explore branch (uniform legal move), 2 = greedy branch, move
                             * drawn by move sampling (oz_selfplay_set_move_sampling; ply < plies) */
    uint8_t pad[3];         /* pad[0]: 0 = the move was searched on the full budget, 1 = on the fast one ("playout cap" above: not a training
                             * example); always 0 without the option.  pad[1]: 1 = the game was adjudicated ("resignation" above: z and the final board are those
                             * of the stop), else 0.  pad[2]: the proof code of the move's root ("proof play" below: 1 loss, 2 draw, 3 win, for
                             * the mover), 0 = unknown; always 0 without the option */
} oz_record;

typedef struct {
    int64_t simulations, node_visits, expansions, terminal_hits, fallbacks;
    int64_t moves, games_completed, records;
    int32_t live_games, overflow;
    int64_t leaves_evaluated;   /* positions handed to the network: <= expansions, because a board that several games reach in
                                 * the same step is evaluated once (results are identical either way; oz_selfplay_config.dedup = OZ_DEDUP_OFF disables) */
} oz_selfplay_stats;

int oz_selfplay_create(oz_selfplay** out, const oz_selfplay_config* cfg, oz_net* net);
int oz_selfplay_destroy(oz_selfplay* sp);
/* `rounds` move rounds: every live game runs cfg.sims simulations, chooses, records and plays one move.
 * Asynchronous (stream ordered); oz_selfplay_sync waits. */
int oz_selfplay_run(oz_selfplay* sp, int rounds);
/* free-running form of oz_selfplay_run: `steps` network batches; in each of them every live game first plays its move if the
 * simulations of the move are complete, runs the simulations that need no network (finished boards) and contributes the
 * leaf of its next first-visit simulation -- batches stay full instead of ~92 % full, moves are no longer aligned across
 * games, every game's simulations / moves / records are exactly those of oz_selfplay_run (training.py:39-67). */
int oz_selfplay_run_steps(oz_selfplay* sp, int steps);
/* batch cap of the free-running driver (0 = none, the default): a network batch holds at most `cap` leaves; a game whose leaf finds no
 * slot keeps it (OZ_LEAF_WAIT) and offers it again in the next batch -- slots are handed out in game order from a start that rotates by
 * `cap` games per batch, so every game is served.  A game's simulations / moves / records do not change; what changes is the size of the
 * launches: the convolution grids are a whole number of rounds of the chip at the right cap (4096 8x8 games on the 512-filter network:
 * cap 3640 = 1024 conv3 tiles of 256 x 256 = 4.0 rounds of 256 CUs, against 5.5 rounds paid as 6 without it). */
int oz_selfplay_set_batch_cap(oz_selfplay* sp, int cap);
/* cross-game leaf de-duplication on / off from the next batch on (oz_selfplay_config.dedup sets the initial state) */
int oz_selfplay_set_dedup(oz_selfplay* sp, int enable);
/* leaves_per_step of the engine's search for the lock-step drivers oz_selfplay_run / oz_selfplay_stagger (see oz_mcts_set_leaves_per_step);
 * before the first driver call.  With k > 1 the drivers read 4 bytes back per move round (the largest remaining budget), i.e. they synchronise
 * the stream once per round and are no longer asynchronous; every leaf goes to the network: oz_selfplay_config.dedup and .eval_cache have no
 * effect (records would be identical either way), leaves_evaluated == expansions. */
int oz_selfplay_set_leaves_per_step(oz_selfplay* sp, int k);
/* solved leaves of the engine's search (see oz_mcts_set_solve_leaves), for every driver; takes effect at the next step */
int oz_selfplay_set_solve_leaves(oz_selfplay* sp, int max_empties);
int oz_selfplay_get_solve_leaves(oz_selfplay* sp, int* max_empties, int64_t* rows_solved);
/* value signs of the engine's search, for every driver (see oz_mcts_set_value_signs; the reference's rule, MCTS/__init__.py:39-40,68-71, is
 * the default: sound mode differs on finished boards and across passes); OZ_ERR_STATE after the first driver call */
int oz_selfplay_set_value_signs(oz_selfplay* sp, int mode);
int oz_selfplay_get_value_signs(oz_selfplay* sp, int* mode);
/* the selection rule of the engine's search (see oz_mcts_set_selection), for oz_selfplay_run; OZ_ERR_STATE after the first driver call */
int oz_selfplay_set_selection(oz_selfplay* sp, int flags, double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor);
int oz_selfplay_get_selection(oz_selfplay* sp, int* flags, double* fpu_reduction, double* fpu_root_reduction, double* cpuct_base, double* cpuct_factor);
/* proofs of the engine's search (see oz_mcts_set_proofs; after oz_selfplay_set_value_signs(sp, OZ_VALUE_SIGNS_SOUND)), for oz_selfplay_run;
 * OZ_ERR_STATE after the first driver call.  oz_selfplay_proof_stats: as oz_mcts_proof_stats, over the engine's games so far. */
int oz_selfplay_set_proofs(oz_selfplay* sp, int enable);
int oz_selfplay_proof_stats(oz_selfplay* sp, int64_t* out4);
/* HIP-event timing of the engine's solving kernel (oz_mcts_solve_leaves_profile / _read on the engine's search) */
int oz_selfplay_solve_leaves_profile(oz_selfplay* sp, int enable);
int oz_selfplay_solve_leaves_profile_read(oz_selfplay* sp, double* ms_total, int64_t* launches, int reset);
/* self-play with root noise: every searched move of every game (oz_selfplay_stagger's included) draws Dir(alpha) at its root, keyed
 * (cfg.seed, game id, ply) -- in a kernel of its own behind the roots kernel of a lock-step round, inside the advance kernel of the
 * free-running driver (whose records stay exactly those of oz_selfplay_run).  Before the first driver call. */
int oz_selfplay_set_root_noise(oz_selfplay* sp, double alpha, double eps);
/* the noise of the searches of the last move round of oz_selfplay_run (tests; eta[num_games][64], armed[num_games]) */
int oz_selfplay_root_noise(oz_selfplay* sp, double* eta, uint8_t* armed);
/* self-play with move sampling ("move sampling" above): the coin is drawn as ever; where it falls on the greedy branch, the move of a game
 * whose ply < plies is sampled, keyed (cfg.seed, game id, ply), and its record has greedy = 2.  Holds for oz_selfplay_run, the free-running
 * oz_selfplay_run_steps (whose records stay exactly those of oz_selfplay_run), oz_selfplay_stagger and leaves_per_step > 1; the arena and the
 * evaluation games never sample.  Before the first driver call (OZ_ERR_STATE afterwards).  plies == 0 disarms; nothing is allocated. */
int oz_selfplay_set_move_sampling(oz_selfplay* sp, double temperature, int plies);
/* self-play under a playout cap ("playout cap" above), keyed (cfg.seed, game id, ply).  Holds for oz_selfplay_run at any leaves_per_step and
 * for the free-running oz_selfplay_run_steps, whose records stay exactly those of oz_selfplay_run; oz_selfplay_stagger's rounds are not
 * capped.  Before the first driver call (OZ_ERR_STATE afterwards).  fast_sims == 0 disarms (full_prob is then not looked at).  OZ_ERR_ARG:
 * fast_sims not 0 and outside [2, cfg.sims], full_prob outside (0, 1] (NaN included).  The engine stays usable after a refusal.
 * 64 B per slot of device memory at the first arming. */
int oz_selfplay_set_playout_cap(oz_selfplay* sp, int fast_sims, double full_prob);
/* what is set (fast_sims 0 = off) and the moves played under the cap so far: full_moves + fast_moves = the moves of oz_selfplay_run /
 * oz_selfplay_run_steps since the cap was armed.  Every pointer may be NULL; reading a counter waits for the engine's stream. */
int oz_selfplay_get_playout_cap(oz_selfplay* sp, int* fast_sims, double* full_prob, int64_t* full_moves, int64_t* fast_moves);
/* self-play with forced playouts ("forced playouts" above): every searched move whose root draws noise is forced, and its visit row
 * (record_visits = 1) is the pruned one.  Holds for oz_selfplay_run at any leaves_per_step, for oz_selfplay_stagger (its rounds draw noise) and
 * for the free-running oz_selfplay_run_steps, whose records and rows stay exactly those of oz_selfplay_run; the fast moves of a playout cap are
 * neither forced nor pruned.  After oz_selfplay_set_root_noise, before the first driver call (OZ_ERR_STATE otherwise); k == 0 switches off. */
int oz_selfplay_set_forced_playouts(oz_selfplay* sp, double k);
/* what is set and, since it was armed: the moves whose recorded row differs from the raw counts, and the visits before / after pruning summed
 * over every move pruning ran on (the moves with an armed root).  Every pointer may be NULL; reading a counter waits for the engine's stream. */
int oz_selfplay_get_forced_playouts(oz_selfplay* sp, double* k, int64_t* moves_pruned, int64_t* visits_raw, int64_t* visits_kept);
/* self-play with resignation ("resignation" above), keyed (cfg.seed, game id).  Holds for oz_selfplay_run at any leaves_per_step, with root
 * noise, move sampling, a playout cap, forced playouts, record_visits, recorded surprise, solved leaves, oz_selfplay_solve_records and the
 * value targets (the TD chain then ends in the adjudicated z).  Needs oz_selfplay_set_record_values(sp, 1) first -- the rule reads the root
 * value the move computes for it -- and comes before the first driver call (OZ_ERR_STATE otherwise).  OZ_ERR_STATE also: together with
 * the Gumbel search (whichever comes second is refused), and, once it is armed, oz_selfplay_run_steps, oz_selfplay_stagger and
 * oz_selfplay_set_record_values(sp, 0).  r == 0 disarms (the other arguments are then not looked at).  OZ_ERR_ARG: v outside (0, 1], r
 * outside [0, 8], min_ply outside [0, 64], keep_prob outside [0, 1] (NaN included).  The engine stays usable after a refusal.  4 B per slot
 * + 48 B of device memory at the first arming. */
int oz_selfplay_set_resign(oz_selfplay* sp, double v, int r, int min_ply, double keep_prob);
/* what is set (r 0 = off) and the counters since the arming.  Every pointer may be NULL; reading the counters waits for the engine's stream. */
int oz_selfplay_get_resign(oz_selfplay* sp, double* v, int* r, int* min_ply, double* keep_prob, oz_resign_stats* stats);
int oz_selfplay_sync(oz_selfplay* sp);
/* continuous self-play (cfg.refill): bring a fresh engine to the steady state of a long-running one before measuring it --
 * slot g is advanced (g * P) / num_games plies into its first game, P = n*n - 4, by searched self-play moves at `sims_pre`
 * simulations each (same kernels, same RNG streams, recorded like any move), so that every later move round completes
 * about num_games / P games instead of none for P - 1 rounds and all of them in one.  First driver call only; asynchronous. */
int oz_selfplay_stagger(oz_selfplay* sp, int sims_pre);
/* HIP-event timing of the tree kernels on the launch stream: slots 0 select 1 leaf compaction 2 evaluator (all network
 * launches) 3 expand + backup 4 roots + move; slot 2 is always timed (oz_selfplay_eval_time), the others while enabled */
#define OZ_TREE_KERNELS 5
int oz_selfplay_profile(oz_selfplay* sp, int enable);
int oz_selfplay_profile_read(oz_selfplay* sp, double* ms_total /* [OZ_TREE_KERNELS] */, int64_t* launches /* [OZ_TREE_KERNELS] */, int reset);
int oz_selfplay_get_stats(oz_selfplay* sp, oz_selfplay_stats* out);
/* per-slot view: boards, player to move, finished flag, plies played, global game id */
int oz_selfplay_state(oz_selfplay* sp, uint64_t* black, uint64_t* white, int8_t* player, uint8_t* finished,
                      int32_t* ply, uint64_t* game_id);
/* records of COMPLETED games, in completion order; returns how many were written */
int oz_selfplay_records(oz_selfplay* sp, oz_record* out, int64_t max_records, int64_t* written);
/* same, device to device, for the RCCL all-gather (dst = device pointer, e.g. a torch tensor) */
int oz_selfplay_records_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written);
/* self-play with the Gumbel search ("Gumbel search" above): every searched move of the lock-step rounds of oz_selfplay_run arms its root in the
 * round's roots step -- g drawn on the device, keyed (seed, game id, ply) with the engine's seed, N0 snapshot from the game's persistent tree, the
 * budget = num_simulations -- and its descents pick by the Gumbel rule at depth 0.  Where the e-greedy coin falls on its greedy branch the move is
 * the Gumbel root's MOVE and the record's `greedy` byte is 3; the explore branch is unchanged (pure Gumbel: e_greedy = 1).  The engine keeps the
 * float32 improved-policy row of every searched move beside its record (256 B each; storage, flush and refill as the visit-count rows).
 * Before the first driver call (OZ_ERR_STATE afterwards).  OZ_ERR_STATE also: together with root noise, forced playouts, move sampling, a playout
 * cap or leaves_per_step > 1 (whichever comes second is refused), and, once it is on, oz_selfplay_run_steps and oz_selfplay_stagger.  Arenas,
 * matches and evaluations never use it; solved leaves, recorded values and value targets, de-duplication and the evaluation cache combine with
 * it unchanged. */
int oz_selfplay_set_gumbel(oz_selfplay* sp, int max_considered, double c_visit, double c_scale);
/* what is set (max_considered 0 = off) and the moves picked by the Gumbel rule so far (each may be NULL) */
int oz_selfplay_get_gumbel(oz_selfplay* sp, int32_t* max_considered, double* c_visit, double* c_scale, int64_t* moves);
/* g, armed and N0 of the searches of the last move round, as oz_mcts_get_gumbel */
int oz_selfplay_gumbel(oz_selfplay* sp, double* g /* [num_games][64] */, uint8_t* armed /* [num_games] */, int32_t* N0 /* [num_games][64] */);
/* the improved-policy rows: row i (float32 [64] by square) belongs to record i of oz_selfplay_records, the same ring order (OZ_ERR_ARG on an
 * engine without the option) */
int oz_selfplay_policies(oz_selfplay* sp, float* out /* [max_records][64] */, int64_t max_records, int64_t* written);
int oz_selfplay_policies_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written);
/* root visit counts of every recorded move (oz_selfplay_config.record_visits = 1; OZ_ERR_ARG otherwise): row i belongs to record i of
 * oz_selfplay_records -- the same ring order, so one permutation sorts both.  A row holds the N(state, action) the move's search left at
 * its root, visits earlier moves' searches left in the same tree included, at square row*8+col, 0 off the legal set: exactly what
 * get_policy_action_probabilities (othelo_mcts.py:51-67) reads.  int32, exact.  A row is kept where its record is (record_cap). */
int oz_selfplay_visits(oz_selfplay* sp, int32_t* out /* [max_records][64] */, int64_t max_records, int64_t* written);
/* same, device to device */
int oz_selfplay_visits_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written);
/* exact value targets for the endgame records (opt-in; never called, every record stays bit for bit): the completed records
 * [first_record, completed so far) of the engine, in place on the device, one wavefront per record.  The position solved is the board BEFORE
 * the move (black, white, player), never the aliased final board.  A record with at most max_empties empties gets z = +1 if S > 0, -1 if
 * S < 0, and for S == 0 z = +1 if the mover is BLACK, else -1 (the draw -> BLACK convention of oz_record.z); its disc loss is
 * S - values[action] >= 0.  No other byte of a record, no visit-count row and no record above the cap changes; a second call finds
 * z_changed == 0.  Waits for the engine's stream like oz_selfplay_records.  OZ_ERR_ARG: max_empties outside 1..OZ_SOLVE_MAX_EMPTIES,
 * first_record < 0; OZ_ERR_STATE: a step is pending. */
typedef struct {
    int64_t records;        /* records looked at */
    int64_t solved;         /* of them, at or below max_empties */
    int64_t z_changed;      /* solved records whose z was rewritten */
    int64_t optimal_moves;  /* solved records whose move has the maximal value (disc loss 0) */
    int64_t disc_loss_sum;  /* sum of S - values[action] over the solved records */
    int32_t disc_loss_max, pad;
} oz_endgame_stats;
int oz_selfplay_solve_records(oz_selfplay* sp, int64_t first_record, int max_empties, oz_endgame_stats* stats /* optional */);
/* ------------------------------------------------------------------ value targets (opt-in; with nothing of it called every record, launch and
 * result is bit for bit what it was).  A record's z is the outcome of one noisy game.  The search knows more about the position it moved from:
 * its ROOT VALUE, the visit-weighted mean of the root's Q,
 *     a[sq]  = N[sq] > 0 ? (double)N[sq] * Q[sq] : 0.0          sq = 0 .. 63; N is 0 off the legal set
 *     value  = pairwise_sum(a, 64) / (double)sum(N)              NumPy's pairwise sum (np.sum of 64 float64); sum(N) == 0: value 0, rc 2
 * in float64 without contraction, N the RAW root counts (never the pruned row of forced playouts) and Q the stored edge value read as a
 * double whatever its q_mode tag: the root's value for the player to move (MCTS/__init__.py:68 keeps Q(s, a) for the mover at s).  ONE
 * definition, oz_root_term / oz_root_mean (csrc/oz_common.h), is what the kernels and oz_root_values evaluate.
 * A VALUE TARGET combines z with the root values.  Take one game's records i = 0 .. T-1 in ply order, mover p_i = +-1, z_i as stored at the
 * time of the call (after oz_selfplay_solve_records if that ran), root value q_i, exact_i = (E > 0 and empties_i <= E), E = exact_empties:
 *     OZ_VALUE_TARGET_OUTCOME   t_i = z_i
 *     OZ_VALUE_TARGET_BLEND     t_i = exact_i ? z_i : (1 - w) * z_i + w * q_i                                   param = w in [0, 1]
 *     OZ_VALUE_TARGET_TD        from BLACK's side: B_T = p_{T-1} * z_{T-1};  for i = T-1 .. 0:                   param = lam in [0, 1]
 *                               B_i = exact_i ? p_i * z_i : (1 - lam) * (p_i * q_i) + lam * B_{i+1};  t_i = p_i * B_i
 * float64, every product and every sum rounded on its own, 1 - w / 1 - lam computed once, the result rounded once to float32.  A solved
 * record restarts the chain: earlier plies bootstrap from the exact value.  After a pass the movers do not alternate: the sign always comes
 * from `player`.  The fast records of a playout cap take part in the chain (they are dropped as examples, as ever).  ONE definition,
 * oz_value_target_* (csrc/oz_common.h), is what k_value_targets and oz_value_targets evaluate.  lam = 1 and w = 0 are the outcome,
 * lam = 0 and (off the exact records) w = 1 the root value itself. */
#define OZ_VALUE_TARGET_OUTCOME 0
#define OZ_VALUE_TARGET_BLEND 1
#define OZ_VALUE_TARGET_TD 2
typedef struct {
    int64_t records;        /* records given a target */
    int64_t exact;          /* of them, exact_i */
    int64_t sign_changed;   /* of them, sign(t_i) != z_i (t_i == 0 counts) */
} oz_value_target_stats;
/* the root value of `count` rows N[count][64], Q[count][64] by square, on the host (no device needed).  OZ_ERR_ARG: a negative N. */
int oz_root_values(const int32_t* N, const double* Q, int64_t count, double* out /* [count] */);
/* the root value of every slot's current root: value[num_games], rc[num_games] as oz_mcts_root_counts (0 ok, 1 unknown state, 2 never
 * selected from; value 0 where rc != 0) */
int oz_mcts_root_values(oz_mcts* m, double* value, int32_t* rc);
/* the engine keeps the root value of every searched move next to its record: lock-step rounds at any leaves_per_step, oz_selfplay_stagger
 * and the free-running driver alike, whose values stay exactly those of oz_selfplay_run; no record and no statistic changes.  Before the
 * first driver call (OZ_ERR_STATE afterwards).  512 B per slot + 8 B per record of device memory at the first enabling. */
int oz_selfplay_set_record_values(oz_selfplay* sp, int enable);
/* value i belongs to record i of oz_selfplay_records, the same ring order (OZ_ERR_ARG on an engine that does not record values) */
int oz_selfplay_values(oz_selfplay* sp, double* out /* [max_records] */, int64_t max_records, int64_t* written);
int oz_selfplay_values_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written);
/* the value targets of the completed records [first_record, completed so far) into the engine's float32 targets[record_cap] on the device,
 * one wavefront per record; a first_record inside a game still reads that game to its end.  Needs oz_selfplay_set_record_values.  Records
 * are not touched.  OZ_ERR_ARG: an unknown mode, param outside [0, 1] (NaN included; not looked at for OUTCOME), exact_empties outside
 * 0..OZ_SOLVE_MAX_EMPTIES, first_record < 0; OZ_ERR_STATE: a step is pending. */
int oz_selfplay_value_targets(oz_selfplay* sp, int64_t first_record, int mode, double param, int exact_empties,
                              oz_value_target_stats* stats /* optional */);
/* target i belongs to record i (OZ_ERR_ARG before the first oz_selfplay_value_targets; targets below its first_record are 0 or stale) */
int oz_selfplay_targets(oz_selfplay* sp, float* out /* [max_records] */, int64_t max_records, int64_t* written);
int oz_selfplay_targets_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written);
/* the same targets on the host (no device needed): R records in any order with their root values; records of one game_id are one game,
 * taken in ply order.  out[i] belongs to records[i]. */
int oz_value_targets(const oz_record* records, const double* values, int64_t R, int n, int mode, double param, int exact_empties,
                     float* out /* [R] */);

/* ------------------------------------------------------------------ policy surprise weighting (opt-in; with nothing of it called every kernel,
 * record, file and launch is what it was).  In most self-play positions the search confirms the network's prior; in a few it overturns it.
 * Every record becomes 8 examples, so the informative ones are diluted.  KataGo's remedy: a record's share of the training data is
 * proportional to how far its policy target moved from the prior.
 * The SURPRISE of a searched move, float64 without contraction, by square sq = 0 .. 63:
 *     q      = the row that becomes the policy target: the recorded count row (the pruned one under forced playouts) at T = 1, (double)N[sq] /
 *              pairwise_sum((double)N, 64), as k_expand_visits normalises it; with the Gumbel search the float32 improved-policy row, widened
 *     p      = the root's STORED prior of the square (never the noised one), 0 off the legal set
 *     term   = q > 0 ? q * (oz_log_cr(q) - oz_log_cr(max(p, DBL_MIN))) : 0          oz_log_cr: the same bits on host and device
 *     s      = max(0, pairwise_sum(term, 64))                                         = KL(q || p)
 * ONE definition, oz_surprise_term / oz_surprise_sum (csrc/oz_common.h), is what the move kernels and oz_policy_surprises evaluate.
 * WEIGHTS: take one game's records; K = those with pad[0] == 0 (fully searched), S = pairwise_sum of their s by ply (zeros elsewhere, 64 terms):
 *     w_i    = (float)((1 - frac) + frac * (s_i * (double)K / S))      fully searched;  1.0f where S == 0;  0 for a fast record
 * so a game's weights sum to K: the amount of data is preserved.  frac in (0, 1]; KataGo uses 0.5.
 * COPIES: d = oz_rng(weight_seed, game_id, ply, OZ_RNG_SURPRISE = 8);  c_i = (int)floor(8.0 * (double)w_i + oz_rng_unit(d)): the record becomes
 * c_i examples instead of 8, E[c_i] = 8 w_i; the first of them is symmetry t0_i = d & 7 (oz_rng_unit reads d >> 11: independent bits), example
 * k is symmetry (t0_i + k) & 7 of oz_sym_src.  ONE definition, oz_surprise_weight / oz_surprise_copies (csrc/oz_common.h), is what
 * k_surprise_weights and the host functions evaluate.  KataGo's extra weight for surprising FAST moves is not built: a fast record gets 0. */
typedef struct {
    int64_t records;        /* records given a weight */
    int64_t full_records;   /* of them, fully searched (pad[0] == 0) */
    int64_t examples;       /* sum of c_i */
    int64_t zero_copies;    /* fully searched records with c_i == 0 */
    int64_t max_copies;     /* the largest c_i */
} oz_surprise_weight_stats;
/* the engine keeps the surprise of every searched move next to its record: lock-step rounds at any leaves_per_step, oz_selfplay_stagger and
 * the free-running driver alike, with root noise, move sampling, forced playouts, a playout cap, recorded values and the Gumbel search; no
 * record, no row and no statistic changes.  The surprise of a fast move is recorded and never used.  Before the first driver call (OZ_ERR_STATE
 * afterwards).  Needs an engine that records a policy target: record_visits = 1 or oz_selfplay_set_gumbel before it (OZ_ERR_ARG).  512 B per
 * slot + 8 B per record of device memory at the first enabling. */
int oz_selfplay_set_record_surprise(oz_selfplay* sp, int enable);
/* surprise i belongs to record i of oz_selfplay_records, the same ring order (OZ_ERR_ARG on an engine that does not record surprise) */
int oz_selfplay_surprises(oz_selfplay* sp, double* out /* [max_records] */, int64_t max_records, int64_t* written);
int oz_selfplay_surprises_device(oz_selfplay* sp, void* dst_device, int64_t max_records, int64_t* written);
/* the surprise of `count` rows by square on the host (no device needed): N[count][64] int32 count rows (OZ_ERR_ARG: a negative count), or
 * q[count][64] float32 policy rows; P[count][64] the priors. */
int oz_policy_surprises(const int32_t* N, const double* P, int64_t count, double* out /* [count] */);
int oz_policy_surprises_f32(const float* q, const double* P, int64_t count, double* out /* [count] */);
/* weights, copy counts and first symmetries of the completed records [first_record, completed so far) into the engine's float32 weights,
 * int32 copies and uint8 first_sym [record_cap] on the device (allocated by the first call), one wavefront per record; a game that lies
 * partly before first_record is still normalised over all of its records.  Needs oz_selfplay_set_record_surprise.  Records are not touched.
 * OZ_ERR_ARG: frac outside (0, 1] (NaN included), first_record < 0; OZ_ERR_STATE: a step is pending. */
int oz_selfplay_surprise_weights(oz_selfplay* sp, int64_t first_record, double frac, uint64_t weight_seed,
                                 oz_surprise_weight_stats* stats /* optional */);
/* entry i belongs to record i (OZ_ERR_ARG before the first oz_selfplay_surprise_weights; entries below its first_record are 0 or stale) */
int oz_selfplay_weights(oz_selfplay* sp, float* weights, int32_t* copies, uint8_t* first_sym /* [max_records] each */, int64_t max_records,
                        int64_t* written);
/* the same on the host (no device needed): R records in any order; records of one game_id are one game, taken in ply order (ply < 64).
 * w[i], copies[i], first_sym[i] belong to records[i].  oz_surprise_copies: w in [0, 64] (the weights of oz_surprise_weights). */
int oz_surprise_weights(const oz_record* records, const double* surprises, int64_t R, double frac, float* w /* [R] */);
int oz_surprise_copies(const oz_record* records, const float* w, int64_t R, uint64_t weight_seed, int32_t* copies /* [R] */,
                       uint8_t* first_sym /* [R] */);

/* root visit counts of the last move round, counts[num_games][64] (parity tests) */
int oz_selfplay_last_counts(oz_selfplay* sp, int32_t* counts);
/* HIP-event time of the evaluator (NN) launches since creation, and their count */
int oz_selfplay_eval_time(oz_selfplay* sp, double* ms_total, int64_t* launches, int64_t* leaves);

/* ------------------------------------------------------------------ exchange step (multi-GPU; SURVEY.md 8(b) gather_examples(comm), 8(e))
 * One process per GPU, games sharded by global id (first_game_id / game_id_stride), weights replicated; the path's ONE collective is
 * the all-gather of the 48-byte move records of completed games -- RCCL over xGMI, bound at run time (librccl.so.1).  Replaces
 * WorkerManager.get_results' list concatenation and the ssh / pickle return path (workers.py:147-159,180-184).
 * Rank 0 makes an id (oz_comm_unique_id), the host hands its 128 bytes to every rank, every rank calls oz_comm_create on ITS device
 * (oz_set_device first), then oz_selfplay_gather_records collectively. */
typedef struct oz_comm oz_comm;
#define OZ_COMM_ID_BYTES 128
int oz_comm_unique_id(uint8_t* id /* [OZ_COMM_ID_BYTES] */);
int oz_comm_create(oz_comm** out, const uint8_t* id, int rank, int world);
int oz_comm_destroy(oz_comm* comm);
/* COLLECTIVE over `comm`: the records [first_record, completed so far) of every rank's engine, concatenated in rank order, into `out`
 * (host buffer of max_records); *written = their number, per_rank[world] (optional) = what each rank contributed.  Room is checked against
 * the pooled count on EVERY rank's behalf before the payload moves: too little room on any rank fails the call on all of them together
 * (OZ_ERR_ARG), never on one rank alone.  out == NULL and max_records == 0 on every rank: the counts only (*written = the pooled number). */
int oz_selfplay_gather_records(oz_selfplay* sp, oz_comm* comm, int64_t first_record, oz_record* out, int64_t max_records, int64_t* written,
                               int64_t* per_rank);
/* COLLECTIVE, the same protocol for the visit-count rows of oz_selfplay_visits (every engine created with record_visits = 1; a rank
 * without them fails the call on every rank together): the rows come back in the order oz_selfplay_gather_records returns the records
 * for the same first_record. */
int oz_selfplay_gather_visits(oz_selfplay* sp, oz_comm* comm, int64_t first_record, int32_t* out /* [max_records][64] */, int64_t max_records,
                              int64_t* written, int64_t* per_rank);

/* ------------------------------------------------------------------ arena
 * duel_between_agents with two NeuralNetworkOthelloAgent (agents.py:44-84): net_a = BLACK, net_b = WHITE,
 * one OthelloMCTS per agent per game, temperature 0, ties broken by the RNG_TIE stream.
 * One of net_a / net_b may be NULL: that colour is played by RandomOthelloAgent (agents.py:20-24; the evaluation games of
 * main.py:163-233), its random.choice drawn from the RNG_TIE stream at that ply.  Both may be NULL (no search at all): the opponents of
 * oz_arena_set_opponent against each other. */
typedef struct oz_arena oz_arena;
int oz_arena_create(oz_arena** out, int n, int num_games, int sims, double c, int q_mode, uint64_t seed,
                    uint64_t first_game_id, oz_net* net_a, oz_net* net_b, int node_cap);
int oz_arena_destroy(oz_arena* a);
int oz_arena_run(oz_arena* a);       /* plays all games to the end (synchronous) */
/* the same, stopping after `max_rounds` further rounds (0 = to the end): a round = one searched ply in every live game.  Synchronous; may
 * be called again to play on.  bench.py's config-5 leg times a bounded number of plies at 800 sims with two real networks. */
int oz_arena_run_rounds(oz_arena* a, int max_rounds);
/* search counters of the BLACK / WHITE agent since creation, layout of oz_mcts_stats */
int oz_arena_stats(oz_arena* a, int64_t* black5, int64_t* white5);
/* cross-game leaf de-duplication of both agents' searches (default on; identical results either way) and the positions the two
 * networks have evaluated so far (<= expansions when concurrent games share boards -- arena games start from one opening) */
int oz_arena_set_dedup(oz_arena* a, int enable);
int oz_arena_leaves_evaluated(oz_arena* a, int64_t* black, int64_t* white);
/* the two agents' leaves go through their networks' persistent evaluation caches (oz_net_set_eval_cache; default 0 = every leaf is evaluated):
 * identical moves, boards and results -- the reference's per-search _predict_cache (othelo_mcts.py:13,82-88) across games, plies and steps */
int oz_arena_set_eval_cache(oz_arena* a, int enable);
/* leaves_per_step of the BLACK (net_a) and WHITE (net_b) agent's search; before the first run.  The networks want max_batch >= num_games * k.
 * With k > 1 an agent's leaves bypass the evaluation cache. */
int oz_arena_set_leaves_per_step(oz_arena* a, int k_black, int k_white);
/* solved leaves of the BLACK (net_a) and WHITE (net_b) agent's search (see oz_mcts_set_solve_leaves); before the first run, like
 * oz_arena_set_leaves_per_step.  The read returns the rows each search has solved so far. */
int oz_arena_set_solve_leaves(oz_arena* a, int black, int white); /* per agent, before the first run, like oz_arena_set_leaves_per_step */
int oz_arena_get_solve_leaves(oz_arena* a, int64_t* rows_black, int64_t* rows_white);
/* value signs of the BLACK (net_a) and WHITE (net_b) agent's search (see oz_mcts_set_value_signs; the reference's rule, MCTS/__init__.py:39-40,
 * 68-71, is the default: sound mode differs on finished boards and across passes); per agent, before the first run */
int oz_arena_set_value_signs(oz_arena* a, int black, int white);
/* proofs of the BLACK (net_a) and WHITE (net_b) agent's search (see oz_mcts_set_proofs; an agent with proofs needs sound signs); before the
 * first run */
int oz_arena_set_proofs(oz_arena* a, int black, int white);

/* ------------------------------------------------------------------ proof play: play and record what a proven root knows (opt-in, on top of
 * proofs; with nothing of it called every kernel, record, file and launch is what it was).  The search proves wins, draws and losses; without
 * this option the move, the visit row and the root value still read the raw counts and the stored Q -- a move proven lost after it took most
 * of the visits is played, trained towards and averaged in.  The rule, one definition for host and device (oz_proof_play, csrc/oz_common.h),
 * over the root's proof entry (legal, lo, hi, own) and its raw counts cnt[64]:
 *   val  = val(root) ("proofs" above); C = the candidates the descent picks from at the root: the edges that prove a known val, else the
 *          edges not proven lost, else the legal set.
 *   keep = C where a square of C has cnt > 0; else the legal set, counted as a fallback.  A root proven a loss keeps its whole row.
 *   row[a] = cnt[a] on keep, 0 elsewhere: the recorded visit row, and what record_surprise measures.
 *   move:  every branch that reads counts -- the arena's and temperature 0's arg-max with its tie draw, the first maximum, move sampling --
 *          reads row and its maximum.  The explore branch of the e-greedy coin stays uniform over the legal set.
 *   root value = (double)val where val is known, else the raw visit-weighted mean: what record_values logs and resignation reads.
 *   proof code of a searched move = val + 2 (1 loss, 2 draw, 3 win, for the mover), 0 where unknown: byte pad[2] of the move's record.
 * oz_selfplay_last_counts stays raw.  The option inherits the support matrix and the refusals of proofs and adds none but this: it needs
 * proofs (OZ_ERR_STATE without them; switching proofs off under it is refused too). */
/* the engine's moves, for oz_selfplay_run; before the first driver call (OZ_ERR_STATE afterwards) */
int oz_selfplay_set_proof_play(oz_selfplay* sp, int enable);
/* [0] searched moves on a proven root [1] moves whose row differs from the raw counts [2] moves whose action differs from the one the raw
 * counts give (greedy and sampled moves; both are evaluated) [3] fallbacks.  Zeros on an engine without the option. */
int oz_selfplay_proof_play_stats(oz_selfplay* sp, int64_t* out4);
/* per agent (black for net_a's search, white for net_b's); needs that agent's proofs; before the first run */
int oz_arena_set_proof_play(oz_arena* a, int black, int white);
/* the selection rule of one agent's search (see oz_mcts_set_selection): agent +1 = BLACK (net_a), -1 = WHITE (net_b); before the first run */
int oz_arena_set_selection(oz_arena* a, int agent, int flags, double fpu_reduction, double fpu_root_reduction, double cpuct_base, double cpuct_factor);

/* ---- tree collection: drop the stored nodes a slot's game has passed (opt-in; off, every kernel, table, record and launch is what it was)
 * A slot's node table only grows until the slot is refilled or reset, so node_cap has to hold a whole game.  Every move adds exactly one disc
 * and a pass creates no node, so once a slot's root holds D discs a stored node that is not the root and holds <= D discs can never be looked
 * up again; every node with more than D discs keeps its statistics.  A collection drops exactly those dead nodes: the kept records move to
 * the front of the slot's pool in expansion order (stable), every edge's cached child index is renumbered, the node's proof entry moves with
 * it, the slot's hash table is rebuilt.  No result bit changes -- counts, values, moves, records, rows are those of the object without the
 * option -- only records are freed, so a smaller node_cap suffices.  node_cap keeps its meaning and its defaults; overflow after a
 * collection is OZ_ERR_CAPACITY as ever.
 * The identity holds while a slot's roots never lose discs: a root set to an EARLIER position finds its dropped nodes gone and expands them
 * afresh (a loss of statistics, never an error).
 * oz_search_tree_keep: the rule on the host, no device needed.  keep[i] = node i stays under the root (root_own, root_opp): it IS the root, or
 * popcount(own | opp) > popcount(root_own | root_opp); new_index[i] = the number of kept j < i, -1 where dropped; *kept = their number.
 * oz_mcts_collect: collects the active slots against their current roots (inactive slots are untouched byte for byte; nothing happens on an
 * object whose roots were never set).  out2 (may be NULL) = nodes before, nodes kept, summed over the active slots.  OZ_ERR_STATE while a step
 * is pending (oz_mcts_select without oz_mcts_backup).  The first call allocates the scratch map, 4 B per node of capacity.
 * Engine and arena: k_tree_collect runs behind the round's roots kernel, before anything looks the new roots up.
 *   OZ_TREE_GC_ON_DEMAND   decided per game on the device: collect iff node_count + num_simulations > node_cap (a simulation expands at most
 *                          one node, at any leaves_per_step)
 *   OZ_TREE_GC_EVERY_MOVE  every active slot every round (the diagnostic mode: small tests exercise the kernel on every move)
 * Before the first driver call / the first run (OZ_ERR_STATE afterwards); OZ_ERR_ARG for an unknown mode.  It combines with every option of
 * oz_selfplay_run and the arena.  oz_selfplay_run_steps and oz_selfplay_stagger refuse an engine with the option (OZ_ERR_STATE): the
 * free-running kernels move inside the kernel and would need the collection as a device call there.
 * oz_tree_gc_stats, per-game counters reduced at the read: collections, the node counts before and after them summed, peak_nodes = the largest
 * node count a slot had at the start of a round since arming, peak_kept = the largest count after a collection -- peak_kept + num_simulations
 * is the node_cap a game of that kind needs under OZ_TREE_GC_ON_DEMAND.  Zeros on an object that never armed the option. */
#define OZ_TREE_GC_OFF 0
#define OZ_TREE_GC_ON_DEMAND 1
#define OZ_TREE_GC_EVERY_MOVE 2
typedef struct oz_tree_gc_stats {
    int64_t collections, nodes_before_sum, nodes_kept_sum, peak_nodes, peak_kept;
} oz_tree_gc_stats;
int oz_search_tree_keep(uint64_t root_own, uint64_t root_opp, const uint64_t* own, const uint64_t* opp, int64_t count,
                        uint8_t* keep /* [count] */, int32_t* new_index /* [count], -1 where dropped */, int64_t* kept);
int oz_mcts_collect(oz_mcts* m, int64_t* out2);
int oz_mcts_tree_gc_stats(oz_mcts* m, oz_tree_gc_stats* stats);
int oz_selfplay_set_tree_gc(oz_selfplay* sp, int mode);
int oz_selfplay_get_tree_gc(oz_selfplay* sp, int* mode, oz_tree_gc_stats* stats);
/* HIP-event timing of the engine's collection launches (one pair per launch); off, nothing is recorded */
int oz_selfplay_tree_gc_profile(oz_selfplay* sp, int enable);
int oz_selfplay_tree_gc_profile_read(oz_selfplay* sp, double* ms_total, int64_t* launches, int reset);
/* per agent: agent +1 = BLACK (net_a), -1 = WHITE (net_b); before the first run */
int oz_arena_set_tree_gc(oz_arena* a, int agent, int mode);
int oz_arena_get_tree_gc(oz_arena* a, int agent, int* mode, oz_tree_gc_stats* stats);
/* the bare search: oz_mcts_root_counts / oz_mcts_root_values with the rule's row and value (same shapes and rc); OZ_ERR_STATE on an object
 * without proofs.  oz_mcts_root_counts and oz_mcts_root_values stay the raw ones. */
int oz_mcts_proven_counts(oz_mcts* m, int32_t* counts /* [G][64] */, uint64_t* legal /* [G] */, int32_t* rc /* [G] */);
int oz_mcts_proven_root_values(oz_mcts* m, double* value /* [G] */, int32_t* rc /* [G] */);
/* oz_mcts_sample_moves over the rule's row and its maximum (same arguments, keys and rc) */
int oz_mcts_proven_sample_moves(oz_mcts* m, double temperature, uint64_t seed, const uint64_t* game_ids, const int32_t* plies, int32_t* action,
                                int32_t* rc);
/* proof targets: the completed records [first_record, completed so far), in place, one wavefront per record: a record with pad[2] != 0 gets
 * z = the proven sign for its mover; a proven draw follows z's convention (BLACK's win).  Idempotent.  Run it before
 * oz_selfplay_solve_records, the value targets and the replay appends.  oz_proof_targets: the same pass over R records on the host. */
typedef struct {
    int64_t records;        /* records looked at */
    int64_t proven;         /* of them, with a proof code */
    int64_t z_changed;      /* of those, whose z was another sign */
} oz_proof_target_stats;
int oz_selfplay_proof_targets(oz_selfplay* sp, int64_t first_record, oz_proof_target_stats* stats /* optional */);
int oz_proof_targets(oz_record* records, int64_t R, oz_proof_target_stats* stats /* optional */);
/* oz_selfplay_value_targets / oz_value_targets with one more flag: exact_proven = 1 makes a record with a proof code exact like one with
 * <= exact_empties empties (it restarts the TD chain; BLEND keeps its z).  The entries without the flag are these with 0, the same code. */
int oz_selfplay_value_targets_x(oz_selfplay* sp, int64_t first_record, int mode, double param, int exact_empties, int exact_proven,
                                oz_value_target_stats* stats /* optional */);
int oz_value_targets_x(const oz_record* records, const double* values, int64_t R, int n, int mode, double param, int exact_empties,
                       int exact_proven, float* out /* [R] */);
/* the rule on the host, no device needed: edge[64] and own_value as oz_mcts_root_proofs / oz_mcts_dump_proofs give them (read on the legal
 * squares; OZ_PROOF_UNKNOWN = none), counts[64] the raw counts (0 off the legal set).  Every output may be NULL. */
int oz_search_proof_play(uint64_t legal, const int8_t* edge, int own_value, const int32_t* counts, int8_t* val, uint64_t* keep,
                         int32_t* row /* [64] */, int* fallback, int* inconsistent);

/* HIP-event timing of the two agents' tree kernels on the launch stream, slots of oz_selfplay_profile (0 select 1 leaf compaction 2 evaluator = all
 * network launches 3 expand + backup 4 move), summed over both searches; the networks' own kernels: oz_net_profile on net_a / net_b */
int oz_arena_profile(oz_arena* a, int enable);
int oz_arena_profile_read(oz_arena* a, double* ms_total /* [OZ_TREE_KERNELS] */, int64_t* launches /* [OZ_TREE_KERNELS] */, int reset);
#define OZ_AGENT_RANDOM 0
#define OZ_AGENT_MINIMAX 1
/* who moves for a colour whose network is NULL (agents.py:27-41; default OZ_AGENT_RANDOM, unchanged): OZ_AGENT_MINIMAX plays
 * oz_kth_bit(bests, RNG_TIE draw of (seed, game id, ply) % popcount(bests)) with bests as oz_rules_minimax defines it -- the stream and the
 * random.choice shape of the random mover.  Before the first run, OZ_ERR_STATE afterwards; OZ_ERR_ARG for a colour that has a network, a depth
 * outside 1..OZ_MINIMAX_MAX_DEPTH or an unknown eval (depth and eval are not read for OZ_AGENT_RANDOM) */
int oz_arena_set_opponent(oz_arena* a, int side /* +1 BLACK, -1 WHITE */, int kind, int depth, int eval);
/* with oz_arena_profile on: HIP-event time and launches of the network-free colour's move kernel under OZ_AGENT_MINIMAX (agents.py:27-41;
 * zeros for OZ_AGENT_RANDOM, whose launches are not timed) */
int oz_arena_opponent_time(oz_arena* a, double* ms_total, int64_t* launches);
/* Openings: every game plays its first plies without any search, once, at the head of the first oz_arena_run / oz_arena_run_rounds (whose
 * max_rounds counts the searched rounds after them), then the agents take over from the position reached.  Default off: every game starts
 * from the standard position, as in the reference.  The opening plies are ordinary logged moves (actions / players / n_moves of
 * oz_arena_results include them, so `actions` still replays a game from the standard position).  The opening id of game slot g is
 * first_opening_id + g and does NOT depend on seed or first_game_id: two arenas given the same (opening_seed, first_opening_id) play the same
 * openings -- new against old and old against new, or two candidates against one suite; every later ply stays keyed (seed, game id, true ply).
 * A game that ends inside its opening stays ended and its result stands.  Independent of leaves_per_step, solve_leaves, the evaluation
 * cache, de-duplication and oz_arena_set_opponent.
 * oz_arena_set_openings: random openings of `plies` plies as oz_rules_random_openings defines them; plies == 0 switches openings off.
 * oz_arena_set_opening_moves: game g plays moves[g][0 .. n_plies[g] - 1] (squares row*8+col).  Every list is replayed on the host first:
 * OZ_ERR_ARG, naming the game and the ply, for a move that is not legal, a move after the game has ended or an n_plies outside
 * 0..OZ_OPENING_MAX_PLIES (and nothing is changed).
 * Both only before the first run (OZ_ERR_STATE afterwards); the later call counts.  oz_arena_set_openings: OZ_ERR_ARG for plies outside
 * 0..OZ_OPENING_MAX_PLIES.  oz_arena_opening_plies: the plies each game's opening played (zeros with openings off and before the first run). */
int oz_arena_set_openings(oz_arena* a, int plies, uint64_t opening_seed, uint64_t first_opening_id);
int oz_arena_set_opening_moves(oz_arena* a, const uint8_t* moves /* [num_games][OZ_OPENING_MAX_PLIES] */, const int32_t* n_plies /* [num_games] */);
int oz_arena_opening_plies(oz_arena* a, int32_t* out /* [num_games] */);
int oz_arena_results(oz_arena* a, int8_t* winner /* +1 net_a */, int32_t* points, int32_t* n_moves,
                     uint8_t* actions /* [num_games][128] */, int8_t* players /* [num_games][128] */,
                     uint64_t* final_black, uint64_t* final_white);

/* ------------------------------------------------------------------ examples
 * training_example_symmetries (training.py:13-23) + the returned tuple layout of execute_episode (:58-72):
 * for each record 8 examples in the reference's order; boards[count*8][n][n][2] uint8 {0,1},
 * policy_index[count*8] (one-hot position row*n+col), z[count*8].
 * alias_final != 0 reproduces the reference's aliasing quirk (boards show the final position). */
int oz_examples_expand(const oz_record* records, int64_t count, int n, int alias_final, uint8_t* boards,
                       int32_t* policy_index, int8_t* z);
int oz_symmetry_table(int n, int32_t* perm /* [8][n*n] source index of every output cell */);
/* the same expansion with the search's visit distribution as the policy target (the AlphaZero pi) instead of the one-hot of the move:
 * counts[count][64] = the rows of oz_selfplay_visits.  pi[count*8][n*n] float64 = get_policy_action_probabilities(root, temperature)
 * (othelo_mcts.py:51-67) of the record's root, then the record's 8 symmetries in training_example_symmetries' order (the identity is
 * example 7): N ** (1 / temperature) on the legal squares divided by np.sum of the (n, n) array in NumPy's pairwise order, or by 1 if
 * that is 0.  Bit-exact against that formula on the host whenever 1 / temperature is an integer; otherwise within 1 ulp of the
 * device's pow per element.  temperature <= 0: OZ_ERR_ARG.  boards and z as in oz_examples_expand. */
int oz_examples_expand_visits(const oz_record* records, const int32_t* counts, int64_t count, int n, int alias_final, double temperature,
                              uint8_t* boards, double* pi, int8_t* z);
/* the same with a float32 policy row by square per record (rows[count][64], e.g. the improved policy of a Gumbel search), on the host (no
 * device needed): pi[8 * count][n][n] float32, every value copied from its source cell, bit for bit */
int oz_examples_expand_policy(const oz_record* records, const float* rows, int64_t count, int n, int alias_final, uint8_t* boards, float* pi,
                              int8_t* z);

/* ------------------------------------------------------------------ training step
 * NNetWrapper.train (Net/NNet.py:53-68) = keras Model.fit on Net/OthelloNN.py:42-56 / Net/BaseNN.py:41-57:
 * losses categorical_crossentropy (on the (n, n)-reshaped policy: per-row renormalisation, see oz_train.hip) +
 * mean_squared_error, Adam(lr, clipvalue) in tf.keras' formulation, BatchNormalization in training mode
 * (momentum bn_momentum, eps 1e-3), inverted Dropout with a counter-based mask keyed (seed, step, layer, element).
 * Weights use the same 40-array get_weights() indexing as oz_net_set_weight.  One optimiser step =
 * oz_trainer_forward_backward (gradients of the batch-mean loss into the gradient arena) + oz_trainer_apply; a
 * data-parallel job all-reduces (averages) the arena between the two calls.  `external_grads` may point to a caller-
 * owned device buffer of oz_trainer_arena_size floats (e.g. a torch tensor handed to RCCL); NULL = library-owned. */
typedef struct oz_trainer oz_trainer;
int oz_trainer_arena_size(int n, int channels, int in_channels, int64_t* nelem);
int oz_trainer_create(oz_trainer** out, int n, int channels, int in_channels, int max_batch, float lr, float clipvalue /* <= 0: none */,
                      float dropout, float bn_momentum, uint64_t seed, float* external_grads);
int oz_trainer_destroy(oz_trainer* t);
/* arithmetic of the 3x3 layers (conv2..conv4): 0 = fp32 matrix cores (default); 1 = f16x2 -- forward and data-gradient GEMMs with every
 * fp32 value as two fp16 planes, 3 fp16 MFMA products per fp32 product with fp32 accumulation (the inference kernels of precision f16x2;
 * tensors are moved into the fp16 range by exact powers of two taken from their own maxima on the device, per step), an activation above
 * 65504 raises OZ_ERR_STATE at the next synchronising call (forward_backward, fit_epoch); 2 = bf16x3 -- forward, data gradient AND weight
 * gradient with every fp32 value exactly as three bf16 planes, 6 bf16 MFMA products per fp32 product with fp32 accumulation, no scaling,
 * no range flag, nothing to refuse.  conv1, the dense layers, BN, losses and Adam stay fp32.  Modes 1 and 2 need channels % 256 == 0 and
 * allocate their buffers at first use; a trainer may switch among the modes between steps. */
int oz_trainer_set_precision(oz_trainer* t, int mode);
/* the policy loss.  OZ_POLICY_LOSS_ROWS (default): the reference's categorical_crossentropy on the (n, n)-reshaped softmax, i.e. every
 * board row renormalised on its own and the loss averaged over rows -- trains only ratios within a row.  OZ_POLICY_LOSS_FLAT: keras'
 * categorical_crossentropy on the (B, n*n) softmax -- q = p / sum(p), clipped to [1e-7, 1 - 1e-7], -sum_i t_i log q_i, batch mean: the
 * loss for dense visit-distribution targets (oz_examples_expand_visits).  Every precision, the step-wise and the resident paths;
 * losses3[1] reports the loss of the mode. */
#define OZ_POLICY_LOSS_ROWS 0
#define OZ_POLICY_LOSS_FLAT 1
int oz_trainer_set_policy_loss(oz_trainer* t, int mode);
int oz_trainer_set_weight(oz_trainer* t, int index, const float* data, int64_t nelem);
int oz_trainer_get_weight(oz_trainer* t, int index, float* data, int64_t nelem);
int oz_trainer_get_grad(oz_trainer* t, int index, float* data, int64_t nelem);      /* trainable arrays only */
int oz_trainer_grad_arena(oz_trainer* t, void** device_ptr, int64_t* nelem);
/* boards as bitboards: own = channel 0, opp = channel 1 of the example board (BaseNN: +1 / -1 squares);
 * pi_target [B][n*n], z_target [B]; losses3 = {total, policy, value} batch means.  Synchronous. */
int oz_trainer_forward_backward(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target,
                                const float* z_target, int B, float* losses3);
int oz_trainer_apply(oz_trainer* t);                         /* Adam step + BN moving-statistics commit (stream-ordered) */
/* keras Model.fit as the reference drives it (Net/NNet.py:67) with the examples RESIDENT on the device: one upload per fit
 * (set_dataset: own / opp / pi_target [N][n*n] / z_target [N]), then per epoch ONE call that runs the optimiser steps of the
 * shuffled order (`order`: `count` example indices, batches of `batch`, the last one may be short) back to back on the
 * stream -- per-step batch gather on the device, no host copy or synchronisation per step -- and returns the
 * sample-weighted mean losses of the epoch {total, policy, value}.  Single-process training; a data-parallel job keeps
 * the step-wise calls (its all-reduce sits between backward and apply). */
int oz_trainer_set_dataset(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target, int64_t N);
int oz_trainer_fit_epoch(oz_trainer* t, const int32_t* order, int64_t count, int batch, float* losses3);
int oz_trainer_outputs(oz_trainer* t, int B, float* p /* [B][n*n] */, float* v /* [B] */);   /* of the last forward pass */
/* Held-out evaluation in INFERENCE mode (keras Model.evaluate / validation_data): the network that will play -- the BN layers on their CURRENT
 * moving statistics, no dropout -- on examples that are not trained on by the call.  The weights evaluated are the raw iterate (the trainer's
 * parameters); the weight average of oz_optimizer.average_decay is NOT evaluated (it would need a second set of derived GEMM operands).
 * The forward is the step's own: the same conv1 kernel and GEMM launches in the trainer's precision, the loss of the trainer's policy-loss mode.
 * out[OZ_EVAL_FIELDS] float64:
 *   out[0..2] = mean loss, policy loss, value loss (the definitions of losses3, in inference mode), float64 sums of the per-example float32 values;
 *   out[3] = share of examples whose policy arg-max equals the target's (the lowest index among equal maxima on both sides);
 *   out[4] = share of the examples with z != 0 whose v has z's sign (0 when there are none);
 *   out[5] = examples; out[6] = examples with z != 0; out[7] = 0 (reserved).
 * Batches of `batch` in [1, max_batch] in the given order, the last one may be short; the sums are added in an order that depends on the
 * batch sizes alone (no atomics), so a repeated call returns the same doubles.
 * oz_trainer_evaluate: N host examples, uploaded to arrays of the evaluation's own -- the resident data set of oz_trainer_set_dataset stays.
 * oz_trainer_evaluate_dataset: `count` indices into the resident data set (any count >= 1; OZ_ERR_ARG while it is empty).
 * oz_trainer_evaluate_replay (declared with the replay buffer below): `count` slot indices in [0, held).
 * Left untouched: the weights, Adam moments, the weight average, the step count, the moving statistics and the ones a pending
 * forward_backward has staged, the gradient arena, the losses of the last step, the resident data set and its order -- a forward_backward,
 * an evaluation, then apply gives the weights it gives without the evaluation, bit for bit.  Overwritten: the pre-activations, activations,
 * p / v and the staged batch, so oz_trainer_outputs / _get_activation (and get_preact) afterwards show the evaluation's LAST batch, and the
 * plan rows' forward GEMM fields.  Errors: OZ_ERR_ARG for a batch outside [1, max_batch], an index out of range, another board size or
 * device; in precision f16x2 the range guard acts as in a step (OZ_ERR_STATE, reported once).  Synchronous. */
#define OZ_EVAL_FIELDS 8
int oz_trainer_evaluate(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target, int64_t N,
                        int batch, double* out);
int oz_trainer_evaluate_dataset(oz_trainer* t, const int32_t* order, int64_t count, int batch, double* out);
/* post-activation output of block `layer` (0-3 conv, 4-5 dense; [B][pixels][channels]) of the last forward pass -- inspection */
int oz_trainer_get_activation(oz_trainer* t, int layer, int B, float* data, int64_t nelem);
/* Diagnostics: read-only views of the last step, for judging every GEMM of the trainer on its own (no kernel is changed by them).
 * get_preact: z[layer], the GEMM output plus bias BEFORE the BN, [B][Hout][Hout][Co], layer 0 .. 5.
 * get_dz:     the WHOLE buffer of the gradient wrt z[layer], [B][Hz][Hz][Co]: conv3 / conv4 ('valid') keep it zero-bordered (Hz = Hout + 4, interior at
 *             offset 2), every other layer has Hz = Hout (dense layers 1).
 * set_capture (off by default): while on, every data-gradient launch (and the heads' backward) is followed by a device-to-device copy on the main
 *             stream of the live rows of its output into a per-layer buffer (allocated at the first `on`) -- the data gradients live in two
 *             ping-pong buffers that are overwritten two layers later.  With capture off the launch sequence of a step is unchanged.
 * get_dgrad:  the captured gradient wrt a[layer] (layer 0 .. 5; [B][Hout][Hout][Co]): the raw GEMM output, before the ReLU mask of the BN backward.
 *             OZ_ERR_STATE when capture is off or no step ran since it was switched on.
 * get_head_grads: the gradients wrt the policy logits and the value head's pre-activation, the two operands of the heads' data gradient.
 * get_preact, get_dz and get_head_grads return OZ_ERR_STATE before the first step of the trainer.
 * get_bn_stats: the batch mean and rstd = 1 / sqrt(biased variance + 1e-3) that the BN forward of `layer` (0 .. 5) left, Co floats each.
 * get_adam_state: the two Adam moments of trainable array `index` (get_weights() order; a moving statistic is refused), as many floats each as the array holds.
 * get_plan:   the launch plan of the last step, as the launchers themselves reported it (oz_net_get_info's counterpart): for layer l = 1 .. 5
 *             (conv2 .. fc2) the OZ_TRAINER_PLAN_FIELDS ints at plan[(l - 1) * OZ_TRAINER_PLAN_FIELDS], then a sixth row for conv1 (layer 0), which
 *             has no GEMM: only its OZ_TRAINER_PLAN_BN_* and OZ_TRAINER_PLAN_CONV1_* fields are set; n = 6 * OZ_TRAINER_PLAN_FIELDS. */
#define OZ_TRAINER_PLAN_ROWS 6               /* rows 0 .. 4: layers 1 .. 5; row 5: layer 0 (conv1) */
#define OZ_TRAINER_PLAN_FIELDS 12            /* ints per layer; [7] is reserved (0) */
#define OZ_TRAINER_PLAN_FWD_KSLICES 0        /* forward GEMM: k-slices, then the kernel (OZ_NET_KERNEL_*: names the tile) */
#define OZ_TRAINER_PLAN_FWD_KERNEL 1
#define OZ_TRAINER_PLAN_DGRAD_KSLICES 2      /* data-gradient GEMM likewise */
#define OZ_TRAINER_PLAN_DGRAD_KERNEL 3
#define OZ_TRAINER_PLAN_DGRAD_TAP_SKIP 4     /* 1: the data gradient ran on pixel-major row tiles (OZ_NET_KERNEL_F32_STD_PIXMAJOR), the form of k_gemm_f32
                                              * that skips the k-tiles of taps reading only zeros; derived from the kernel the launcher reports */
#define OZ_TRAINER_PLAN_WGRAD_KERNEL 5       /* OZ_TRAINER_WGRAD_* */
#define OZ_TRAINER_PLAN_WGRAD_MSPLIT 6       /* row splits of the weight gradient (> 1: raw slabs + the fixed-order sum) */
#define OZ_TRAINER_PLAN_BN_FWD 8             /* OZ_TRAINER_BN_FWD_*: the regime t_bn_forward took for the layer's BN */
#define OZ_TRAINER_PLAN_BN_BWD 9             /* OZ_TRAINER_BN_BWD_* (t_bn_backward) */
#define OZ_TRAINER_PLAN_BN_BWD_RS 10         /* row splits of the split BN backward (1 on the fused path) */
#define OZ_TRAINER_PLAN_CONV1_S1 11          /* conv1's row only: row splits of k_t_conv1_wgrad */
enum {
    OZ_TRAINER_BN_FWD_FUSED32 = 1,           /* k_t_bn_fwd_fused<32>: up to 2048 rows */
    OZ_TRAINER_BN_FWD_FUSED64 = 2,           /* k_t_bn_fwd_fused<64>: up to OZ_BN_FUSED_MAX_ROWS rows */
    OZ_TRAINER_BN_FWD_STREAM = 3,            /* k_t_colreduce<0 / 1> + k_t_fin_mean / k_t_fin_var + k_t_bn_fwd */
    OZ_TRAINER_BN_BWD_FUSED = 1,             /* k_t_bn_bwd_fused (float64 sums) */
    OZ_TRAINER_BN_BWD_SPLIT = 2              /* k_t_colreduce<2> + k_t_bnb_apply + k_t_sum_partials */
};
enum {
    OZ_TRAINER_WGRAD_TAPS_F32 = 1,           /* k_wgrad_f32, one tap per block */
    OZ_TRAINER_WGRAD_BOARDS_F32 = 2,         /* k_wgrad_conv, board-resident */
    OZ_TRAINER_WGRAD_OCT_H2 = 3,             /* k_wgrad_h2 on the octet images */
    OZ_TRAINER_WGRAD_OCT_B3 = 4              /* k_wgrad_b3 on the octet images */
};
int oz_trainer_get_preact(oz_trainer* t, int layer, int B, float* data, int64_t nelem);
int oz_trainer_get_dz(oz_trainer* t, int layer, int B, float* data, int64_t nelem);
int oz_trainer_set_capture(oz_trainer* t, int on);
int oz_trainer_get_dgrad(oz_trainer* t, int layer, int B, float* data, int64_t nelem);
int oz_trainer_get_head_grads(oz_trainer* t, int B, float* dlogit /* [B][n*n] */, float* dvpre /* [B] */);
int oz_trainer_get_plan(oz_trainer* t, int* plan, int n);
int oz_trainer_get_bn_stats(oz_trainer* t, int layer, float* mean /* [Co] */, float* rstd /* [Co] */);
int oz_trainer_get_adam_state(oz_trainer* t, int index, float* m, float* v);
int oz_trainer_sync(oz_trainer* t);
int oz_trainer_step_count(oz_trainer* t, int64_t* step);

/* ---- optimiser options (opt-in; with none set oz_trainer_apply launches k_t_adam as before and every weight, moment, loss and file is unchanged)
 * What AlphaZero's objective (z - v)^2 - pi^T log p + c |theta|^2 and KataGo's training add to plain Adam with clipvalue: an L2 term or a
 * decoupled weight decay, a learning-rate schedule, a clip of the gradient's global norm and an exponential moving average of the weights.  They
 * live here, behind oz_trainer_apply, because oz_trainer_fit_epoch / _replay run every optimiser step of an epoch back to back on the device:
 * there is no host hook between two steps.
 *
 * ONE STEP, PER ELEMENT, IN THIS ORDER (the definition; G = the gradient arena as backward -- or a data-parallel job's all-reduce -- left it):
 *   1. g = G * s                            s = min(1, global_clipnorm / |G|_2), as float32; 1 with the clip off
 *   2. g += 2 c w                           decayed arrays only (l2 = c; the factor enters as the float32 rounding of 2 c)
 *   3. g = clip(g, -clipvalue, clipvalue)   oz_trainer_create's clipvalue
 *   4. m = 0.9 m + 0.1 g, v = 0.999 v + 0.001 g g            as before
 *   5. w_new = (w - lr_t m / (sqrt(v) + 1e-7)) - (lr_s lambda) w      the last term on decayed arrays only (weight_decay = lambda; the product
 *                                           lr_s lambda is formed in double and enters as its float32 rounding)
 *   6. E = d E + (1 - d) w_new              average_decay = d; d and 1 - d (formed in double) enter as their float32 roundings
 * |G|_2 is taken over every trainable element of the arena, the padding between arrays excluded.  THE L2 TERM IS NOT PART OF THE CLIPPED NORM:
 * the norm pass reads G alone (one streaming read), and the clip bounds the data gradient, not the regulariser.  The norm is GLOBAL, one
 * number per step (Keras' clipnorm is per variable; its global_clipnorm is this one).  It is a two-stage sum in float64 whose partial sums are
 * combined in a fixed order, without floating-point atomics: a step is bit-reproducible from run to run.
 * The rate of step s (1-based count of the step being applied) is lr_s = lr * f(s), in double on the host (oz_lr_schedule_at is the one
 * definition; oz_trainer_apply calls it):  s <= warmup_steps: f = s / warmup_steps;  otherwise q = min(1, (s - warmup_steps) /
 * max(1, total_steps - warmup_steps)) and  OZ_LR_CONSTANT: f = 1;  OZ_LR_LINEAR: f = 1 - (1 - r) q;  OZ_LR_COSINE: f = r + (1 - r) (1 + cos(pi q)) / 2,
 * r = final_ratio.  lr_t = lr_s sqrt(1 - 0.999^s) / (1 - 0.9^s) is then formed and rounded to float32 as before.
 * decay_mask: bit i selects get_weights() index i; 0 = the default, the eight kernels (indices 0, 6, .., 30, 36, 38: no bias, gamma or beta).
 * The average E (+ one arena, 64 MB at 512 filters) is allocated only when average_decay is on, seeded with the weights when it is switched on,
 * and re-seeded by oz_trainer_set_weight for the trainable array that call writes.  The BN moving statistics are not averaged.
 * Refused with OZ_ERR_ARG: a negative or NaN l2 / weight_decay / global_clipnorm, l2 and weight_decay both positive, average_decay outside [0, 1)
 * (0 = off), an unknown schedule, final_ratio outside [0, 1], negative warmup_steps / total_steps, warmup_steps > total_steps for a LINEAR or
 * COSINE schedule (CONSTANT does not look at total_steps), a mask bit >= 40 or on a moving statistic (6 l + 4, 6 l + 5). */
#define OZ_LR_CONSTANT 0
#define OZ_LR_LINEAR 1
#define OZ_LR_COSINE 2
typedef struct {
    double l2;                 /* c >= 0; 0 = off */
    double weight_decay;       /* lambda >= 0, decoupled (AdamW); 0 = off */
    uint64_t decay_mask;       /* 0 = the default mask */
    double global_clipnorm;    /* > 0 switches the global-norm clip on */
    double average_decay;      /* d in (0, 1) switches the weight average on */
    int32_t schedule;          /* OZ_LR_* */
    int32_t reserved;          /* 0 */
    int64_t warmup_steps, total_steps;
    double final_ratio;        /* r in [0, 1] */
} oz_optimizer;
/* opt == NULL: everything off (what a trainer starts with).  Takes effect at the next apply; the step count is not touched. */
int oz_trainer_set_optimizer(oz_trainer* t, const oz_optimizer* opt);
int oz_trainer_get_optimizer(oz_trainer* t, oz_optimizer* opt);
int oz_trainer_set_lr(oz_trainer* t, float lr);              /* the base rate `lr`, from the next apply on */
/* *out = lr_s of step `step` (>= 1) under `opt` (NULL: lr).  Pure host function, no GPU needed; validates the whole struct (list above). */
int oz_lr_schedule_at(const oz_optimizer* opt, float lr, int64_t step, double* out);
/* the last applied step: its lr_s, and -- valid with global_clipnorm on, else 0 and 1 -- |G|_2 and s (the double the float32 factor was rounded
 * from).  Waits for the stream.  OZ_ERR_STATE before the first apply. */
int oz_trainer_get_step_info(oz_trainer* t, double* lr_s, double* grad_norm, double* clip_scale);
/* E of a trainable array; the current value of a moving statistic.  OZ_ERR_STATE with the average off. */
int oz_trainer_get_weight_average(oz_trainer* t, int index, float* data, int64_t nelem);
/* on demand, the same reduction kernels: the sum of squares of the gradient arena's array elements (OZ_SQSUM_GRADIENTS) or of the decayed
 * arrays' weights (OZ_SQSUM_DECAYED_WEIGHTS, under the current or default mask: c * this is the L2 term of the objective).  Waits for the stream.
 * The three loss numbers of a step or an epoch stay the data losses. */
#define OZ_SQSUM_GRADIENTS 0
#define OZ_SQSUM_DECAYED_WEIGHTS 1
int oz_trainer_sqsum(oz_trainer* t, int what, double* out);
/* Benchmark hook: mean HIP-event milliseconds of `iters` back-to-back launches of the step's optimiser kernel (ms3[0]: k_t_adam with the options
 * off, k_t_adam_x otherwise) and of the norm's two kernels (ms3[1]; 0 with global_clipnorm off); ms3[2] is reserved (0).  The launches are real:
 * weights, moments and average move as under `iters` steps on the arena as it stands (the step count does not) -- for a scratch trainer. */
int oz_trainer_time_optimizer(oz_trainer* t, int iters, double* ms3);

/* ---- auxiliary heads (opt-in; without them every kernel, launch, arena size, file and result is unchanged)
 * KataGo's auxiliary targets from the END of the game: an ownership head and a score head on f2 (the 512 post-dropout features the policy and
 * value heads read), trained with the trunk and then thrown away -- the search, predict and the inference network never see them.
 * The target, one definition (oz_aux_target, csrc/oz_common.h; on the host oz_aux_targets): a record's final board from the mover's side,
 * (fin_own, fin_opp) = (final_black, final_white) for player == +1, swapped otherwise; both words 0 = "no auxiliary target" for a record of
 * an adjudicated game (pad[1] == 1: its board at the stop is no final board) and for the fast record of a playout cap (pad[0] == 1).  A real
 * final board is never empty: fin_own | fin_opp == 0 is the mask m = 0.  With A = n*n: ownership target t_a = +1 / -1 / 0 for a square of
 * fin_own / of fin_opp / empty, score target s* = (popcount(fin_own) - popcount(fin_opp)) / A.  A symmetry acts on the pair as on the boards.
 * Heads and losses (fp32 in every trainer precision):  o_a = tanh(f2 . Wown[:, a] + bown[a]),  s = tanh(f2 . Wsc + bsc),
 *   L_own = (1/B) sum_b m_b (1/A) sum_a (o_a - t_a)^2,   L_sc = (1/B) sum_b m_b (s - s*)^2      (B = the batch, as the value loss divides)
 *   total loss = policy + value + w_own L_own + w_score L_sc   (losses[0]; the policy and value numbers stay what they were).
 * Weights: four arrays behind the forty -- 40 Wown [512][A], 41 bown [A], 42 Wsc [512], 43 bsc [1] -- at the end of the parameter, gradient
 * and Adam arenas (the forty keep their offsets; the arena then ends with bsc, without padding: oz_trainer_arena_size_aux =
 * oz_trainer_arena_size + 512 A + A + 512 + 1).  oz_trainer_set_weight / get_weight / get_grad / get_adam_state / get_weight_average take the
 * indices 40 .. 43; the optimiser options and the weight average act on the larger arena (the default decay mask gains
 * the two kernels 40 and 42; an explicit decay_mask names arrays 0 .. 39 only).  A fresh head is Glorot-uniform from the trainer's seed, biases 0.
 * oz_trainer_set_aux_heads: before the first step (OZ_ERR_STATE later); OZ_ERR_ARG for a negative or non-finite weight; again before the first
 * step it only replaces the two weights.  OZ_ERR_ARG for a trainer created on an external gradient arena (a data-parallel fit): the library
 * cannot see the size of a caller's arena, one sized for the forty arrays would be written past its end, and the final pairs do not travel
 * through the pooled rows anyway; the heads' arenas are always library-owned (oz_trainer_arena_size_aux says how large they are).
 * Both weights 0: the heads' forward and losses run, no backward kernel is launched, and the forty gradients and three losses are those of a
 * trainer without the heads, bit for bit.
 * Data: _forward_backward_aux / _set_dataset_aux take the examples' pairs; the entry points without them feed every mask 0.  An epoch from a
 * replay buffer needs one that keeps the pairs (oz_replay_create_aux; OZ_ERR_ARG otherwise).  losses5 = {total, policy, value, L_own, L_sc}.
 * oz_trainer_evaluate* do not run the heads. */
int oz_aux_targets(const oz_record* records, int64_t R, uint64_t* fin_own /* [R] */, uint64_t* fin_opp /* [R] */);      /* host only, no GPU needed */
int oz_trainer_arena_size_aux(int n, int channels, int in_channels, int64_t* nelem);
int oz_trainer_set_aux_heads(oz_trainer* t, float w_own, float w_score);
int oz_trainer_get_aux_heads(oz_trainer* t, int* on, float* w_own, float* w_score);
int oz_trainer_forward_backward_aux(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target,
                                    const uint64_t* fin_own, const uint64_t* fin_opp, int B, float* losses5);
int oz_trainer_set_dataset_aux(oz_trainer* t, const uint64_t* own, const uint64_t* opp, const float* pi_target, const float* z_target,
                               const uint64_t* fin_own, const uint64_t* fin_opp, int64_t N);
/* of the last forward pass: o [B][A], s [B] (each may be NULL) */
int oz_trainer_aux_outputs(oz_trainer* t, int B, float* own, float* score);
/* step2 (optional): the last step's {L_own, L_sc}; epoch2 (optional): the sample-weighted float64 means of the last oz_trainer_fit_epoch /
 * _replay call, accumulated on the device in step order like its three losses */
int oz_trainer_get_aux_losses(oz_trainer* t, float* step2, double* epoch2);
/* diagnostics: the last step's gradients wrt the two pre-activations, the loss weights included (dopre [B][A], dspre [B]); df2_before
 * (optional, [B][512]): the gradient wrt f2 as the policy and value heads left it, before the auxiliary term was added -- needs
 * oz_trainer_set_capture and a weight on (OZ_ERR_STATE otherwise); oz_trainer_get_dgrad(5) then shows the sum */
int oz_trainer_get_aux_head_grads(oz_trainer* t, int B, float* dopre, float* dspre, float* df2_before);

/* ------------------------------------------------------------------ replay buffer (opt-in; without it every result, record and file is unchanged)
 * Finished training examples RESIDENT on the device, between the self-play engines that produce them and the trainer that consumes them:
 * the replacement, for callers that ask for it, of the host's list of example tuples (main.py:21-53 CircularArray, training.py:58-72).
 * Storage: slot s holds exactly what the trainer's resident data set holds for an example -- own[s], opp[s] uint64 (own = channel 0 of the
 * example board = the record's BLACK board, opp = channel 1 = its WHITE board: absolute colours; bit row*8+col), pi[s][n*n] float32 indexed
 * row*n+col, z[s] float32.  276 B per 8x8 example.
 * The 8 examples of a record: example 8i+t is symmetry t of training_example_symmetries' order (oz_symmetry_table; the identity is example 7):
 * output bit (r, c) of the board is the source bit perm[t][r][c] of the board at the move -- of the game's final board (final_black /
 * final_white) when alias_final != 0; z = (float)record.z.  OZ_REPLAY_TARGET_ONEHOT: pi is 1.0f at the output cell whose source cell is the
 * action, 0 elsewhere.  OZ_REPLAY_TARGET_VISITS: the float64 row of oz_examples_expand_visits at `temperature` (the same device code: N ** (1 / T)
 * on the legal squares over their np.sum in NumPy's pairwise order, or over 1 if that is 0), each element rounded once to float32 (round to
 * nearest), then the 8 symmetries.  A slot so equals, bit for bit, what trainer.pack_examples(loop.examples_from_records(...)) yields.
 * Order: the records of ONE append are appended in ascending (game_id, ply), whatever order the engine's buffer or the caller's array holds
 * them in (games that finish in the same kernel reserve their blocks of the engine's buffer in a race): contents never depend on it.
 * Ring: the example with running index k (counted from creation or the last clear) lives in slot k % capacity -- the oldest example is
 * overwritten.  (NOT the reference's CircularArray + in-place random.shuffle, which overwrites random survivors; the host path keeps that.)
 * capacity need not be a multiple of 8: a record's examples may straddle the wrap.  An append of more than `capacity` examples keeps its last
 * `capacity`.
 * Fast records: a record with pad[0] != 0 (a move searched on the fast budget of a playout cap) is not a training example and is left out of
 * an append -- out of the order the host builds anyway; *appended_records, `total` and the kept-last-`capacity` rule count the kept records.
 * Errors, all OZ_ERR_ARG: a board size of the engine / trainer that differs from the buffer's; an object on another device; VISITS with
 * temperature <= 0, from an engine created without record_visits, or with counts == NULL; first_record < 0; an order index outside [0, held);
 * batch outside [1, max_batch]; alias_final not 0 / 1; an unknown target; capacity outside [1, 2^31 - 1]; a read beyond `held`.
 * Synchronisation: every call is synchronous; the appends wait for the engine's stream first (like oz_selfplay_records).  One mutex per
 * object; oz_trainer_fit_epoch_replay locks the trainer, then the buffer, and runs on the trainer's stream like oz_trainer_fit_epoch. */
typedef struct oz_replay oz_replay;
#define OZ_REPLAY_TARGET_ONEHOT 0   /* pi = one-hot of the move played (oz_examples_expand) */
#define OZ_REPLAY_TARGET_VISITS 1   /* pi = the visit distribution at `temperature` (oz_examples_expand_visits) */
#define OZ_REPLAY_TARGET_POLICY 2   /* pi = the record's improved-policy row of a Gumbel search (oz_examples_expand_policy), bit for bit; an engine
                                     * with oz_selfplay_set_gumbel, oz_replay_append_selfplay / _targets only (OZ_ERR_ARG elsewhere) */
int oz_replay_create(oz_replay** out, int n, int64_t capacity /* examples, 1 .. 2^31-1 */);
int oz_replay_destroy(oz_replay* r);
int oz_replay_clear(oz_replay* r);
/* held = min(total, capacity); total = examples appended since creation / clear (each may be NULL) */
int oz_replay_info(oz_replay* r, int64_t* held, int64_t* capacity, int64_t* total);
/* records [first_record, completed so far) of the engine -> 8 examples each, device to device (the 48-byte records alone visit the host, to be
 * ordered; the examples never leave the device); *appended_records (optional) says how many */
int oz_replay_append_selfplay(oz_replay* r, oz_selfplay* sp, int64_t first_record, int alias_final, int target, double temperature,
                              int64_t* appended_records);
/* the same from host records (+ counts[count][64], the rows of oz_selfplay_visits, for OZ_REPLAY_TARGET_VISITS, else NULL): the pooled records
 * of a multi-GPU run, saved games.  count < 2^28. */
int oz_replay_append_records(oz_replay* r, const oz_record* records, const int32_t* counts, int64_t count, int alias_final,
                             int target, double temperature);
/* the two appends with VALUE TARGETS ("value targets" above) in place of the records' z: example z = the float32 target of its record, 8 per
 * record.  _targets: the engine's targets as the last oz_selfplay_value_targets left them (OZ_ERR_ARG before the first; the caller computes them
 * for first_record or earlier), staged device to device beside the records and the counts.  _values: values[count] float32, one per record. */
int oz_replay_append_selfplay_targets(oz_replay* r, oz_selfplay* sp, int64_t first_record, int alias_final, int target, double temperature,
                                      int64_t* appended_records);
int oz_replay_append_records_values(oz_replay* r, const oz_record* records, const int32_t* counts, const float* values, int64_t count,
                                    int alias_final, int target, double temperature);
/* the engine append under POLICY SURPRISE WEIGHTING ("policy surprise weighting" above): record i becomes c_i examples instead of 8, the copy
 * counts and first symmetries as the last oz_selfplay_surprise_weights left them (OZ_ERR_ARG before the first; the caller computes them for
 * first_record or earlier).  Records in ascending (game_id, ply) as ever; example k < c_i of record i is symmetry (t0_i + k) & 7 and has the
 * running index total + off_i + k, off = the exclusive prefix sum of c over that order (built on the host from 4 B per record; the example
 * bytes stay on the device).  E = sum c_i examples: total advances by E, an append larger than the buffer keeps its last `capacity`.  A record
 * with c_i == 0 writes nothing.  value_targets != 0: example z = the record's float32 value target, as oz_replay_append_selfplay_targets.
 * *appended_records = the non-fast records considered, *appended_examples = E (both optional).  One wavefront per record, no atomics. */
int oz_replay_append_selfplay_weighted(oz_replay* r, oz_selfplay* sp, int64_t first_record, int alias_final, int target, double temperature,
                                       int value_targets, int64_t* appended_records, int64_t* appended_examples);
/* finished examples from the host, in the given order (restoring a saved buffer, hand-made data) */
int oz_replay_append_examples(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi /* [count][n*n] */,
                              const float* z, int64_t count);
/* a saved buffer back: clears, then places the `count` = min(total, capacity) newest examples, oldest first, at the running indices
 * [total - count, total) -- the slots they had when they were appended -- and leaves the running index at `total` */
int oz_replay_restore(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, int64_t count, int64_t total);
/* slots [first_slot, first_slot + count) to the host (tests, saving; each array may be NULL) */
int oz_replay_read(oz_replay* r, int64_t first_slot, int64_t count, uint64_t* own, uint64_t* opp, float* pi, float* z);
/* oz_trainer_fit_epoch with the replay buffer as the resident data set: order[i] = a slot index in [0, held); the same launches, steps and
 * losses as oz_trainer_fit_epoch on a data set with the slots' contents */
int oz_trainer_fit_epoch_replay(oz_trainer* t, oz_replay* r, const int32_t* order, int64_t count, int batch, float* losses3);
/* oz_trainer_evaluate_dataset with the replay buffer's slots as the data set (order[i] in [0, held)); locks the trainer, then the buffer */
int oz_trainer_evaluate_replay(oz_trainer* t, oz_replay* r, const int32_t* order, int64_t count, int batch, double* out);
/* A buffer that also keeps every slot's FINAL PAIR for the trainer's auxiliary heads ("auxiliary heads" above): two more uint64 per slot,
 * fin_own[s], fin_opp[s] = oz_aux_target of the example's record under the example's symmetry (0 / 0: no auxiliary target).  Every append
 * fills them: the record appends (plain, with value targets, weighted) through AUX instantiations of the two append kernels -- the same
 * ballots as the boards, lane t stores example t's pair, no atomics -- and the example appends through the _aux entry points below; the
 * entry points without the pair write zeros into such a buffer.  own / opp / pi / z of a slot are what a plain buffer holds for the same
 * appends.  The _aux example entry points on a plain buffer ignore the pair; oz_replay_read_aux on one is OZ_ERR_STATE. */
int oz_replay_create_aux(oz_replay** out, int n, int64_t capacity);
int oz_replay_has_aux(oz_replay* r, int* aux);
int oz_replay_append_examples_aux(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, const uint64_t* fin_own,
                                  const uint64_t* fin_opp, int64_t count);
int oz_replay_restore_aux(oz_replay* r, const uint64_t* own, const uint64_t* opp, const float* pi, const float* z, const uint64_t* fin_own,
                          const uint64_t* fin_opp, int64_t count, int64_t total);
int oz_replay_read_aux(oz_replay* r, int64_t first_slot, int64_t count, uint64_t* fin_own, uint64_t* fin_opp);

/* ------------------------------------------------------------------ diagnostics
 * device arithmetic behind the PUCT / backup formulas (MCTS/__init__.py:68,168-170), for bit-exact
 * comparison with the host: sqrt(a), a/b in float64; a/b and (a*b+a)/b in float32 (no FMA contraction). */
int oz_selftest_arith(const double* a, const double* b, int count, double* sqrt_a, double* div_ab, float* fdiv_ab,
                      float* fchain);
/* what the matrix pipe of the current device sustains right now: a pure-MFMA loop (no LDS, no loads, no barriers, one wave per SIMD) for
 * about target_ms milliseconds.  kind 0 = v_mfma_f32_32x32x2_f32 (precision f32's instruction), 1 = v_mfma_f32_16x16x32_f16 on operands with
 * busy mantissas (precision f16x2's), 2 = v_mfma_f32_16x16x32_bf16 on operands with random 7-bit mantissas (precision bf16x3's planes).  tflops = issued FLOP / HIP-event time; clock_ghz (optional) = the clock at which back-to-back issue
 * gives that rate; ms_measured (optional).  bench.py reports both kinds as `device_calibration`: the number that separates a slow or
 * power-capped box from a regression of the kernels. */
int oz_selftest_mfma_rate(int kind, double target_ms, double* tflops, double* clock_ghz, double* ms_measured);
/* the three-plane split of precision bf16x3 as the device evaluates it (oz_net_b3.h, b3_split): for x[i], planes[3 i .. 3 i + 2] (optional) = (b1, b2, b3)
 * widened to fp32 and sum[i] = (b1 + b2) + b3 in fp32 -- equal to x[i] bit for bit for every finite x with |x| >= 2^-100 (the claim the mode rests on;
 * tests/test_gpu_parity.py::test_bf16x3_split_is_exact).  Host buffers; count <= 2^28. */
int oz_selftest_b3_split(const float* x, int64_t count, float* planes, float* sum);

#ifdef __cplusplus
}
#endif
#endif
