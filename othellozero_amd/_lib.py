"""ctypes binding of libothellozero_amd.so (include/othellozero_amd.h).

There is NO fallback: if the HIP library cannot be loaded, importing anything that
computes raises `OzLibraryError`.  The library is built in-tree by
`python -m othellozero_amd.build` (hipcc --offload-arch=gfx950).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OZ_LIB_PATH") or os.path.join(_HERE, "lib", "libothellozero_amd.so")

OZ_OK, OZ_ERR_HIP, OZ_ERR_ARG, OZ_ERR_CAPACITY, OZ_ERR_KEY, OZ_ERR_STATE = range(6)
QMODE_NEP50, QMODE_F64 = 0, 1
DEDUP_DEFAULT, DEDUP_ON, DEDUP_OFF = 0, 1, 2                                          # oz_selfplay_config.dedup
NET_OPT_SIMPLE_LOOP, NET_OPT_ACT_TARGET_LOG2, NET_OPT_LOW_GUARD_LOG2, NET_OPT_SELF_CHECK, NET_OPT_W_TARGET_LOG2, NET_OPT_F32_STD_TILE, NET_OPT_LATENCY_SPLITS = 1, 2, 3, 4, 5, 6, 7      # oz_net_set_option
NET_OPT_CONV3_TILE = 8
NET_OPT_LOW_LOOP_PHASES = 9
NET_OPT_B3_TILE = 10
NET_OPT_B3_MIX_ROWS = 11
NET_INFO_CONV3_TILE_ROWS, NET_INFO_SELF_CHECK_GUARD, NET_INFO_ARITHMETIC = 1, 2, 3                                                          # oz_net_get_info
NET_INFO_LAYER_BIG_ROWS = 64       # + layer: bf16x3, the leading rows on 256-row tiles
NET_INFO_LAYER_TILE_ROWS, NET_INFO_LAYER_KSLICES, NET_INFO_LAYER_KERNEL = 16, 32, 48      # + layer 1 .. 5 (conv2 .. fc2): the launch plan of the last forward
NET_KERNEL_NAMES = {0: "none", 1: "f32_skinny", 2: "f32_std", 3: "f32_std_pixmajor", 4: "f32_big", 5: "lut", 6: "lut_xcd", 7: "lut_xcd_inline",
                    10: "h2_small2", 11: "h2_small", 12: "h2_bigpp", 13: "h2_bigpp_lut", 14: "h2_midpp", 15: "h2_lowpp1", 16: "h2_lowpp", 17: "h2_big",
                    18: "h2_mid", 19: "h2_thin2", 20: "h2_thin", 21: "h2_thin4w", 30: "b3", 31: "b3_big", 32: "b3_mixed"}      # OZ_NET_KERNEL_* of the header
LEAF_IDLE, LEAF_TERMINAL, LEAF_EVAL = 0, 1, 2
VT_INT, VT_F32, VT_F64 = 0, 1, 2
MAX_LEAVES_PER_STEP = 16                                                             # OZ_MCTS_MAX_LEAVES_PER_STEP
POLICY_LOSS_ROWS, POLICY_LOSS_FLAT = 0, 1                                            # oz_trainer_set_policy_loss
TRAINER_PLAN_FIELDS, TRAINER_PLAN_ROWS = 12, 6                                       # OZ_TRAINER_PLAN_*: rows for layers 1 .. 5, then conv1's, of oz_trainer_get_plan
TRAINER_BN_FWD_NAMES = {0: "none", 1: "fused32", 2: "fused64", 3: "stream"}          # OZ_TRAINER_BN_FWD_*
TRAINER_BN_BWD_NAMES = {0: "none", 1: "fused", 2: "split"}                           # OZ_TRAINER_BN_BWD_*
TRAINER_WGRAD_NAMES = {0: "none", 1: "taps_f32", 2: "boards_f32", 3: "oct_h2", 4: "oct_b3"}      # OZ_TRAINER_WGRAD_*
MINIMAX_EVAL_DISCS, MINIMAX_EVAL_WEIGHTED, MINIMAX_MAX_DEPTH, MINIMAX_NONE = 0, 1, 6, -2 ** 31    # OZ_MINIMAX_*
MINIMAX_EVALS = {"discs": MINIMAX_EVAL_DISCS, "weighted": MINIMAX_EVAL_WEIGHTED}
SOLVE_MAX_EMPTIES = 12                                                               # OZ_SOLVE_MAX_EMPTIES
SOLVE_LEAVES_MAX_EMPTIES = 10                                                        # OZ_SOLVE_LEAVES_MAX_EMPTIES
AGENT_RANDOM, AGENT_MINIMAX = 0, 1                                                   # oz_arena_set_opponent
OPENING_MAX_PLIES = 16                                                               # OZ_OPENING_MAX_PLIES
REPLAY_TARGET_ONEHOT, REPLAY_TARGET_VISITS, REPLAY_TARGET_POLICY = 0, 1, 2                                    # oz_replay_append_*
VALUE_TARGET_OUTCOME, VALUE_TARGET_BLEND, VALUE_TARGET_TD = 0, 1, 2                  # OZ_VALUE_TARGET_*
VALUE_TARGET_MODES = {"outcome": VALUE_TARGET_OUTCOME, "blend": VALUE_TARGET_BLEND, "td": VALUE_TARGET_TD}
NET_KERNELS = ("input", "conv2", "conv3", "conv4", "fc1", "fc2", "heads")           # OZ_NET_KERNELS slots
TREE_KERNELS = ("select", "compact", "network", "expand_backup", "roots_move")       # OZ_TREE_KERNELS slots


class OzLibraryError(RuntimeError):
    pass


class OzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[oz error {code}] {msg}")
        self.code = code


class SelfplayConfig(C.Structure):
    _fields_ = [
        ("n", C.c_int32), ("num_games", C.c_int32), ("sims", C.c_int32), ("q_mode", C.c_int32),
        ("c", C.c_double), ("temperature", C.c_double), ("e_greedy", C.c_double),
        ("seed", C.c_uint64), ("first_game_id", C.c_uint64), ("game_id_stride", C.c_uint64),
        ("refill", C.c_int32), ("node_cap", C.c_int32), ("reserved0", C.c_int32), ("record_cap", C.c_int32),
        ("dedup", C.c_int32), ("batch_cap", C.c_int32), ("eval_cache", C.c_int32), ("record_visits", C.c_int32),
    ]


class SelfplayStats(C.Structure):
    _fields_ = [
        ("simulations", C.c_int64), ("node_visits", C.c_int64), ("expansions", C.c_int64),
        ("terminal_hits", C.c_int64), ("fallbacks", C.c_int64),
        ("moves", C.c_int64), ("games_completed", C.c_int64), ("records", C.c_int64),
        ("live_games", C.c_int32), ("overflow", C.c_int32),
        ("leaves_evaluated", C.c_int64),
    ]


class EndgameStats(C.Structure):                                                     # oz_endgame_stats
    _fields_ = [
        ("records", C.c_int64), ("solved", C.c_int64), ("z_changed", C.c_int64), ("optimal_moves", C.c_int64), ("disc_loss_sum", C.c_int64),
        ("disc_loss_max", C.c_int32), ("pad", C.c_int32),
    ]


class SurpriseWeightStats(C.Structure):                                              # oz_surprise_weight_stats
    _fields_ = [("records", C.c_int64), ("full_records", C.c_int64), ("examples", C.c_int64), ("zero_copies", C.c_int64),
                ("max_copies", C.c_int64)]


class ResignStats(C.Structure):                                                      # oz_resign_stats
    _fields_ = [("games_adjudicated", C.c_int64), ("adjudicated_plies_sum", C.c_int64), ("games_exempt", C.c_int64),
                ("exempt_triggered", C.c_int64), ("exempt_wrong", C.c_int64), ("exempt_trigger_ply_sum", C.c_int64)]


class ValueTargetStats(C.Structure):                                                 # oz_value_target_stats
    _fields_ = [("records", C.c_int64), ("exact", C.c_int64), ("sign_changed", C.c_int64)]


class ProofTargetStats(C.Structure):                                                 # oz_proof_target_stats
    _fields_ = [("records", C.c_int64), ("proven", C.c_int64), ("z_changed", C.c_int64)]


class TreeGcStats(C.Structure):                                                      # oz_tree_gc_stats
    _fields_ = [("collections", C.c_int64), ("nodes_before_sum", C.c_int64), ("nodes_kept_sum", C.c_int64), ("peak_nodes", C.c_int64),
                ("peak_kept", C.c_int64)]


class Optimizer(C.Structure):                                                       # oz_optimizer
    _fields_ = [
        ("l2", C.c_double), ("weight_decay", C.c_double), ("decay_mask", C.c_uint64), ("global_clipnorm", C.c_double),
        ("average_decay", C.c_double), ("schedule", C.c_int32), ("reserved", C.c_int32), ("warmup_steps", C.c_int64),
        ("total_steps", C.c_int64), ("final_ratio", C.c_double),
    ]


LR_SCHEDULES = {"constant": 0, "linear": 1, "cosine": 2}                             # OZ_LR_*
EVAL_FIELDS = 8                                                                      # OZ_EVAL_FIELDS
SQSUM_KINDS = {"gradients": 0, "weights": 1}                                         # OZ_SQSUM_GRADIENTS / OZ_SQSUM_DECAYED_WEIGHTS


# numpy view of oz_record (48 bytes)
RECORD_DTYPE = np.dtype([
    ("black", "<u8"), ("white", "<u8"), ("final_black", "<u8"), ("final_white", "<u8"), ("game_id", "<u8"),
    ("ply", "u1"), ("action", "u1"), ("player", "i1"), ("z", "i1"), ("greedy", "u1"), ("pad", "u1", (3,)),
])
assert RECORD_DTYPE.itemsize == 48
RNG_PLAYOUT = 6                                                                      # OZ_RNG_PLAYOUT
RNG_RESIGN = 9                                                                       # OZ_RNG_RESIGN


def record_fast(records):
    """the playout-cap flag of move records (RECORD_DTYPE): uint8, 1 = the move was searched on the fast budget (no training example),
    0 = on the full one; the first spare byte of oz_record, always 0 without the option"""
    return np.asarray(records)["pad"][..., 0]


def record_adjudicated(records):
    """the resignation flag of move records (RECORD_DTYPE): uint8, 1 = the record's game was adjudicated (stopped by the resignation rule: z
    and the final board are those of the stop), 0 = it was played to its end; the second spare byte of oz_record, always 0 without the option"""
    return np.asarray(records)["pad"][..., 1]


def full_records(records, visits=None):
    """the filter of the record consumers: (records, visits) without the fast records of a playout cap and their visit-count rows, order
    kept; with no flag set the arguments come back as they are"""
    rec = np.asarray(records)
    keep = record_fast(rec) == 0
    if keep.all():
        return records, visits
    if visits is not None:
        cnt = np.asarray(visits).reshape(-1, 64)
        assert cnt.shape[0] == rec.size, f"{cnt.shape[0]} visit-count rows for {rec.size} records"
        visits = cnt[keep]
    return rec[keep], visits

_u64p, _i32p, _f32p, _f64p = (C.POINTER(t) for t in (C.c_uint64, C.c_int32, C.c_float, C.c_double))
_u8p, _i8p, _i64p, _vp = C.POINTER(C.c_uint8), C.POINTER(C.c_int8), C.POINTER(C.c_int64), C.c_void_p

# name -> argtypes: every symbol include/othellozero_amd.h declares (tests check the export list)
SIGNATURES = {
    "oz_version": [], "oz_device_count": [], "oz_set_device": [C.c_int],
    "oz_rules_legal_moves": [_u64p, _u64p, C.c_int, C.c_int, _u64p],
    "oz_rules_apply_moves": [_u64p, _u64p, _u8p, C.c_int, C.c_int, _u64p, _u64p],
    "oz_rules_status": [_u64p, _u64p, C.c_int, C.c_int, _u8p, _i32p, _i32p, _i8p],
    "oz_rules_play": [_u64p, _u64p, _i8p, _u8p, C.c_int, C.c_int, _u64p, _u64p, _i8p, _u8p],
    "oz_rules_minimax": [_u64p, _u64p, _i8p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _u64p],      # agents.py:27-41
    "oz_rules_solve": [_u64p, _u64p, _i8p, C.c_int, C.c_int, C.c_int, _i32p, _u64p, _i32p, _u8p],
    "oz_rules_solve_sign": [_u64p, _u64p, _i8p, C.c_int, C.c_int, C.c_int, _i8p, _u8p],
    "oz_rules_random_openings": [C.c_int, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, _u64p, _u64p, _i8p, _u8p, _u8p, _i32p],
    "oz_rules_profile": [C.c_int], "oz_rules_profile_read": [_f64p, _i64p, C.c_int],
    "oz_selfplay_solve_records": [_vp, C.c_int64, C.c_int, C.POINTER(EndgameStats)],
    "oz_net_create": [C.POINTER(_vp), C.c_int, C.c_int, C.c_int],
    "oz_net_create_bnn": [C.POINTER(_vp), C.c_int, C.c_int, C.c_int],
    "oz_net_create_stub": [C.POINTER(_vp), C.c_int, C.c_uint64, C.c_uint64, C.c_int],
    "oz_net_destroy": [_vp], "oz_net_num_weights": [_vp],
    "oz_net_weight_size": [_vp, C.c_int, _i64p],
    "oz_net_set_weight": [_vp, C.c_int, _f32p, C.c_int64],
    "oz_net_get_weight": [_vp, C.c_int, _f32p, C.c_int64],
    "oz_net_commit": [_vp],
    "oz_net_set_precision": [_vp, C.c_int], "oz_net_get_precision": [_vp], "oz_net_check": [_vp],
    "oz_net_init_random": [_vp, C.c_uint64],
    "oz_net_predict": [_vp, _u64p, _u64p, C.c_int, _f32p, _f32p],
    "oz_net_predict_boards": [_vp, _u8p, C.c_int, _f32p, _f32p],
    "oz_net_forward_launched": [_vp, _u64p, _u64p, C.c_int, C.c_int, _f32p, _f32p],
    "oz_net_time_forward": [_vp, C.c_int, C.c_int, _f32p],
    "oz_net_profile": [_vp, C.c_int], "oz_net_profile_read": [_vp, _f64p, _i64p],
    "oz_net_profiled_layer": [_vp, C.POINTER(C.c_int)], "oz_net_set_tables": [_vp, C.c_int],
    "oz_net_profile_kernels": [_vp, _f64p, _i64p, C.c_int],
    "oz_net_set_eval_cache": [_vp, C.c_int64], "oz_net_eval_cache_stats": [_vp, _i64p, _i64p, _i64p, _i64p],
    "oz_net_set_eval_symmetry": [_vp, C.c_int, C.c_uint64], "oz_net_get_eval_symmetry": [_vp, C.POINTER(C.c_int), _u64p],
    "oz_net_eval_symmetry_profile": [_vp, C.c_int, _f64p, _i64p, C.c_int],
    "oz_eval_symmetries": [C.c_uint64, _u64p, _u64p, C.c_int64, _i32p], "oz_sym_boards": [_i32p, C.c_int, _u64p, C.c_int64, _u64p],
    "oz_net_set_option": [_vp, C.c_int, C.c_int], "oz_net_get_info": [_vp, C.c_int, C.POINTER(C.c_int)],
    "oz_net_get_scaling": [_vp, C.c_int, _i32p, C.c_int64],
    "oz_net_b3_plan": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _i64p, _i64p],
    "oz_net_get_activation": [_vp, C.c_int, C.c_int64, C.c_int64, _f64p],
    "oz_net_self_check": [_vp, _f64p, _f64p, C.POINTER(C.c_int)],
    "oz_mcts_create": [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int],
    "oz_mcts_destroy": [_vp], "oz_mcts_reset": [_vp, C.c_int], "oz_mcts_set_dedup": [_vp, C.c_int],
    "oz_mcts_set_roots": [_vp, _u64p, _u64p, _u8p],
    "oz_mcts_simulate": [_vp, _vp, C.c_int], "oz_mcts_select": [_vp],
    "oz_mcts_leaves": [_vp, _i32p, _u64p, _u64p],
    "oz_mcts_backup": [_vp, _f32p, _f32p],
    "oz_mcts_last_value": [_vp, _f64p, _i32p, _i32p],
    "oz_mcts_root_counts": [_vp, _i32p, _u64p, _i32p],
    "oz_mcts_policy": [_vp, C.c_double, _u64p, C.POINTER(C.c_double), _i32p],
    "oz_mcts_num_nodes": [_vp, _i32p],
    "oz_mcts_dump_node": [_vp, C.c_int, C.c_int, _u64p, _u64p, _i32p, _u64p, _i32p, _f64p, _u8p, _f64p],
    "oz_mcts_stats": [_vp, _i64p],
    "oz_mcts_set_leaves_per_step": [_vp, C.c_int], "oz_mcts_get_leaves_per_step": [_vp, C.POINTER(C.c_int)],
    "oz_mcts_use_wide_kernels": [_vp, C.c_int], "oz_mcts_wide_stats": [_vp, _i64p],
    "oz_selfplay_set_leaves_per_step": [_vp, C.c_int], "oz_arena_set_leaves_per_step": [_vp, C.c_int, C.c_int],
    "oz_mcts_set_solve_leaves": [_vp, C.c_int], "oz_mcts_get_solve_leaves": [_vp, C.POINTER(C.c_int), _i64p],
    "oz_mcts_solve_leaves_profile": [_vp, C.c_int], "oz_mcts_solve_leaves_profile_read": [_vp, _f64p, _i64p, C.c_int],
    "oz_selfplay_set_solve_leaves": [_vp, C.c_int], "oz_selfplay_get_solve_leaves": [_vp, C.POINTER(C.c_int), _i64p],
    "oz_selfplay_solve_leaves_profile": [_vp, C.c_int], "oz_selfplay_solve_leaves_profile_read": [_vp, _f64p, _i64p, C.c_int],
    "oz_arena_set_solve_leaves": [_vp, C.c_int, C.c_int], "oz_arena_get_solve_leaves": [_vp, _i64p, _i64p],
    "oz_mcts_set_value_signs": [_vp, C.c_int], "oz_mcts_get_value_signs": [_vp, C.POINTER(C.c_int)],
    "oz_selfplay_set_value_signs": [_vp, C.c_int], "oz_selfplay_get_value_signs": [_vp, C.POINTER(C.c_int)],
    "oz_arena_set_value_signs": [_vp, C.c_int, C.c_int],
    "oz_search_backup_values": [C.c_int, C.c_uint64, C.c_int, C.c_double, _f64p, _f64p],
    "oz_search_terminal_value": [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_int)],
    "oz_mcts_set_selection": [_vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double],
    "oz_mcts_get_selection": [_vp, C.POINTER(C.c_int), _f64p, _f64p, _f64p, _f64p],
    "oz_selfplay_set_selection": [_vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double],
    "oz_selfplay_get_selection": [_vp, C.POINTER(C.c_int), _f64p, _f64p, _f64p, _f64p],
    "oz_arena_set_selection": [_vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double],
    "oz_search_select_c": [C.c_double, C.c_double, C.c_double, C.c_int, _f64p],
    "oz_search_select_scores": [_i32p, _f64p, _f64p, C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                C.c_double, _f64p, _f64p, _f64p, _f64p, _i32p],
    "oz_search_tree_keep": [C.c_uint64, C.c_uint64, _u64p, _u64p, C.c_int64, _u8p, _i32p, _i64p],
    "oz_mcts_collect": [_vp, _i64p], "oz_mcts_tree_gc_stats": [_vp, C.POINTER(TreeGcStats)],
    "oz_selfplay_set_tree_gc": [_vp, C.c_int], "oz_selfplay_get_tree_gc": [_vp, C.POINTER(C.c_int), C.POINTER(TreeGcStats)],
    "oz_selfplay_tree_gc_profile": [_vp, C.c_int], "oz_selfplay_tree_gc_profile_read": [_vp, _f64p, _i64p, C.c_int],
    "oz_arena_set_tree_gc": [_vp, C.c_int, C.c_int], "oz_arena_get_tree_gc": [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(TreeGcStats)],
    "oz_mcts_set_proofs": [_vp, C.c_int], "oz_mcts_get_proofs": [_vp, C.POINTER(C.c_int)],
    "oz_mcts_dump_proofs": [_vp, C.c_int, C.c_int, _i8p, _i8p, _i8p], "oz_mcts_root_proofs": [_vp, _i8p, _i8p, _i32p],
    "oz_mcts_proof_stats": [_vp, _i64p], "oz_selfplay_set_proofs": [_vp, C.c_int], "oz_selfplay_proof_stats": [_vp, _i64p],
    "oz_arena_set_proofs": [_vp, C.c_int, C.c_int],
    "oz_selfplay_set_proof_play": [_vp, C.c_int], "oz_selfplay_proof_play_stats": [_vp, _i64p],
    "oz_selfplay_proof_targets": [_vp, C.c_int64, C.POINTER(ProofTargetStats)], "oz_proof_targets": [_vp, C.c_int64, C.POINTER(ProofTargetStats)],
    "oz_arena_set_proof_play": [_vp, C.c_int, C.c_int],
    "oz_mcts_proven_sample_moves": [_vp, C.c_double, C.c_uint64, _u64p, _i32p, _i32p, _i32p],
    "oz_mcts_proven_counts": [_vp, _i32p, _u64p, _i32p],"oz_mcts_proven_root_values": [_vp, _f64p, _i32p],
    "oz_selfplay_value_targets_x": [_vp, C.c_int64, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(ValueTargetStats)],
    "oz_value_targets_x": [_vp, _f64p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _f32p],
    "oz_search_proof_play": [C.c_uint64, _i8p, C.c_int, _i32p, _i8p, _u64p, _i32p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "oz_search_proof_value": [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int)],
    "oz_search_proof_candidates": [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _u64p, C.POINTER(C.c_int)],
    "oz_search_proof_backup": [_u8p, _i32p, C.c_int, C.c_int, _u64p, _u64p, _u64p, _i8p, _i32p, C.POINTER(C.c_int)],
    "oz_mcts_set_root_noise": [_vp, C.c_double, _f64p, _u8p],
    "oz_mcts_sample_root_noise": [_vp, C.c_double, C.c_double, C.c_uint64, _u64p, _i32p],
    "oz_mcts_get_root_noise": [_vp, _f64p, _u8p, _f64p],
    "oz_selfplay_set_root_noise": [_vp, C.c_double, C.c_double], "oz_selfplay_root_noise": [_vp, _f64p, _u8p],
    "oz_mcts_sample_moves": [_vp, C.c_double, C.c_uint64, _u64p, _i32p, _i32p, _i32p],
    "oz_selfplay_set_move_sampling": [_vp, C.c_double, C.c_int],
    "oz_selfplay_set_playout_cap": [_vp, C.c_int, C.c_double],
    "oz_selfplay_get_playout_cap": [_vp, C.POINTER(C.c_int), _f64p, _i64p, _i64p],
    "oz_forced_playouts_prune": [_i32p, _f64p, _f64p, _f64p, _u64p, _i32p, C.c_int64, C.c_double, C.c_double, C.c_double, _i32p],
    "oz_mcts_set_forced_playouts": [_vp, C.c_double], "oz_mcts_get_forced_playouts": [_vp, _f64p],
    "oz_mcts_pruned_counts": [_vp, _i32p, _u64p, _i32p],
    "oz_selfplay_set_forced_playouts": [_vp, C.c_double],
    "oz_selfplay_get_forced_playouts": [_vp, _f64p, _i64p, _i64p, _i64p],
    "oz_playout_budgets": [C.c_uint64, _u64p, _i32p, C.c_int64, C.c_int, C.c_int, C.c_double, _i32p],
    "oz_selfplay_set_resign": [_vp, C.c_double, C.c_int, C.c_int, C.c_double],
    "oz_selfplay_get_resign": [_vp, _f64p, C.POINTER(C.c_int), C.POINTER(C.c_int), _f64p, C.POINTER(ResignStats)],
    "oz_resign_scan": [_i8p, _f64p, _i32p, C.c_int64, C.c_double, C.c_int, C.c_int, _i32p, _i8p],
    "oz_resign_exempt": [C.c_uint64, _u64p, C.c_int64, C.c_double, _u8p],
    "oz_mcts_set_gumbel": [_vp, C.c_int, C.c_double, C.c_double, C.c_int, _f64p, _u8p],
    "oz_mcts_sample_gumbel": [_vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_uint64, _u64p, _i32p],
    "oz_mcts_get_gumbel": [_vp, _f64p, _u8p, _i32p, _i32p, _f64p, _f64p, _i32p],
    "oz_mcts_gumbel_policy": [_vp, _f32p, _i32p, _i32p], "oz_mcts_gumbel_scores": [_vp, _f64p],
    "oz_mcts_node_value": [_vp, C.c_int, C.c_int, _f64p],
    "oz_selfplay_set_gumbel": [_vp, C.c_int, C.c_double, C.c_double], "oz_selfplay_get_gumbel": [_vp, _i32p, _f64p, _f64p, _i64p],
    "oz_selfplay_gumbel": [_vp, _f64p, _u8p, _i32p],
    "oz_selfplay_policies": [_vp, _f32p, C.c_int64, _i64p], "oz_selfplay_policies_device": [_vp, _vp, C.c_int64, _i64p],
    "oz_gumbel_considered_visits": [C.c_int, C.c_int, _i32p],
    "oz_gumbel_draws": [C.c_uint64, _u64p, _i32p, _u64p, C.c_int64, _f64p], "oz_gumbel_from_units": [_f64p, C.c_int64, _f64p],
    "oz_gumbel_root": [_i32p, _i32p, _f64p, _f64p, _f64p, _u64p, _f64p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_int, _i32p, _i32p, _f32p,
                       _f64p, _f64p],
    "oz_selfplay_create": [C.POINTER(_vp), C.POINTER(SelfplayConfig), _vp],
    "oz_selfplay_destroy": [_vp], "oz_selfplay_run": [_vp, C.c_int], "oz_selfplay_run_steps": [_vp, C.c_int], "oz_selfplay_sync": [_vp],
    "oz_selfplay_stagger": [_vp, C.c_int], "oz_selfplay_profile": [_vp, C.c_int], "oz_selfplay_set_batch_cap": [_vp, C.c_int], "oz_selfplay_set_dedup": [_vp, C.c_int],
    "oz_selfplay_profile_read": [_vp, _f64p, _i64p, C.c_int],
    "oz_selfplay_get_stats": [_vp, C.POINTER(SelfplayStats)],
    "oz_selfplay_state": [_vp, _u64p, _u64p, _i8p, _u8p, _i32p, _u64p],
    "oz_selfplay_records": [_vp, _vp, C.c_int64, _i64p],
    "oz_selfplay_records_device": [_vp, _vp, C.c_int64, _i64p],
    "oz_selfplay_visits": [_vp, _i32p, C.c_int64, _i64p],
    "oz_selfplay_visits_device": [_vp, _vp, C.c_int64, _i64p],
    "oz_selfplay_last_counts": [_vp, _i32p],
    "oz_root_values": [_i32p, _f64p, C.c_int64, _f64p], "oz_mcts_root_values": [_vp, _f64p, _i32p],
    "oz_selfplay_set_record_values": [_vp, C.c_int],
    "oz_selfplay_values": [_vp, _f64p, C.c_int64, _i64p], "oz_selfplay_values_device": [_vp, _vp, C.c_int64, _i64p],
    "oz_selfplay_value_targets": [_vp, C.c_int64, C.c_int, C.c_double, C.c_int, C.POINTER(ValueTargetStats)],
    "oz_selfplay_targets": [_vp, _f32p, C.c_int64, _i64p], "oz_selfplay_targets_device": [_vp, _vp, C.c_int64, _i64p],
    "oz_value_targets": [_vp, _f64p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, _f32p],
    "oz_selfplay_set_record_surprise": [_vp, C.c_int],
    "oz_selfplay_surprises": [_vp, _f64p, C.c_int64, _i64p], "oz_selfplay_surprises_device": [_vp, _vp, C.c_int64, _i64p],
    "oz_policy_surprises": [_i32p, _f64p, C.c_int64, _f64p], "oz_policy_surprises_f32": [_f32p, _f64p, C.c_int64, _f64p],
    "oz_selfplay_surprise_weights": [_vp, C.c_int64, C.c_double, C.c_uint64, C.POINTER(SurpriseWeightStats)],
    "oz_selfplay_weights": [_vp, _f32p, _i32p, _u8p, C.c_int64, _i64p],
    "oz_surprise_weights": [_vp, _f64p, C.c_int64, C.c_double, _f32p],
    "oz_surprise_copies": [_vp, _f32p, C.c_int64, C.c_uint64, _i32p, _u8p],
    "oz_selfplay_eval_time": [_vp, _f64p, _i64p, _i64p],
    "oz_comm_unique_id": [_u8p], "oz_comm_create": [C.POINTER(_vp), _u8p, C.c_int, C.c_int], "oz_comm_destroy": [_vp],
    "oz_selfplay_gather_records": [_vp, _vp, C.c_int64, _vp, C.c_int64, _i64p, _i64p],
    "oz_selfplay_gather_visits": [_vp, _vp, C.c_int64, _i32p, C.c_int64, _i64p, _i64p],
    "oz_arena_create": [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_uint64, _vp, _vp, C.c_int],
    "oz_arena_destroy": [_vp], "oz_arena_run": [_vp], "oz_arena_run_rounds": [_vp, C.c_int], "oz_arena_stats": [_vp, _i64p, _i64p],
    "oz_arena_set_dedup": [_vp, C.c_int], "oz_arena_set_eval_cache": [_vp, C.c_int], "oz_arena_profile": [_vp, C.c_int], "oz_arena_profile_read": [_vp, _f64p, _i64p, C.c_int], "oz_arena_leaves_evaluated": [_vp, _i64p, _i64p],
    "oz_arena_set_opponent": [_vp, C.c_int, C.c_int, C.c_int, C.c_int], "oz_arena_opponent_time": [_vp, _f64p, _i64p],      # agents.py:27-41
    "oz_arena_set_openings": [_vp, C.c_int, C.c_uint64, C.c_uint64], "oz_arena_set_opening_moves": [_vp, _u8p, _i32p],
    "oz_arena_opening_plies": [_vp, _i32p],
    "oz_arena_results": [_vp, _i8p, _i32p, _i32p, _u8p, _i8p, _u64p, _u64p],
    "oz_examples_expand": [_vp, C.c_int64, C.c_int, C.c_int, _u8p, _i32p, _i8p],
    "oz_examples_expand_visits": [_vp, _i32p, C.c_int64, C.c_int, C.c_int, C.c_double, _u8p, _f64p, _i8p],
    "oz_examples_expand_policy": [_vp, _f32p, C.c_int64, C.c_int, C.c_int, _u8p, _f32p, _i8p],
    "oz_symmetry_table": [C.c_int, _i32p],
    "oz_selftest_arith": [_f64p, _f64p, C.c_int, _f64p, _f64p, _f32p, _f32p],
    "oz_selftest_mfma_rate": [C.c_int, C.c_double, _f64p, _f64p, _f64p],
    "oz_selftest_b3_split": [_f32p, C.c_int64, _f32p, _f32p],
    "oz_trainer_arena_size": [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)],
    "oz_trainer_create": [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                          C.c_uint64, _vp],
    "oz_trainer_destroy": [_vp],
    "oz_trainer_set_weight": [_vp, C.c_int, _f32p, C.c_int64],
    "oz_trainer_get_weight": [_vp, C.c_int, _f32p, C.c_int64],
    "oz_trainer_get_grad": [_vp, C.c_int, _f32p, C.c_int64],
    "oz_trainer_grad_arena": [_vp, C.POINTER(_vp), C.POINTER(C.c_int64)],
    "oz_trainer_forward_backward": [_vp, _u64p, _u64p, _f32p, _f32p, C.c_int, _f32p],
    "oz_trainer_apply": [_vp],
    "oz_trainer_set_dataset": [_vp, _u64p, _u64p, _f32p, _f32p, C.c_int64],
    "oz_trainer_fit_epoch": [_vp, _i32p, C.c_int64, C.c_int, _f32p],
    "oz_trainer_evaluate": [_vp, _u64p, _u64p, _f32p, _f32p, C.c_int64, C.c_int, _f64p],
    "oz_trainer_evaluate_dataset": [_vp, _i32p, C.c_int64, C.c_int, _f64p],
    "oz_trainer_outputs": [_vp, C.c_int, _f32p, _f32p],
    "oz_trainer_get_activation": [_vp, C.c_int, C.c_int, _f32p, C.c_int64],
    "oz_trainer_get_preact": [_vp, C.c_int, C.c_int, _f32p, C.c_int64], "oz_trainer_get_dz": [_vp, C.c_int, C.c_int, _f32p, C.c_int64],
    "oz_trainer_set_capture": [_vp, C.c_int], "oz_trainer_get_dgrad": [_vp, C.c_int, C.c_int, _f32p, C.c_int64],
    "oz_trainer_get_plan": [_vp, _i32p, C.c_int],
    "oz_trainer_get_bn_stats": [_vp, C.c_int, _f32p, _f32p], "oz_trainer_get_adam_state": [_vp, C.c_int, _f32p, _f32p],
    "oz_trainer_get_head_grads": [_vp, C.c_int, _f32p, _f32p],
    "oz_trainer_sync": [_vp],
    "oz_trainer_set_precision": [_vp, C.c_int],
    "oz_trainer_set_policy_loss": [_vp, C.c_int],
    "oz_trainer_step_count": [_vp, C.POINTER(C.c_int64)],
    "oz_trainer_set_optimizer": [_vp, C.POINTER(Optimizer)], "oz_trainer_get_optimizer": [_vp, C.POINTER(Optimizer)],
    "oz_trainer_set_lr": [_vp, C.c_float],
    "oz_lr_schedule_at": [C.POINTER(Optimizer), C.c_float, C.c_int64, C.POINTER(C.c_double)],
    "oz_trainer_get_step_info": [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "oz_trainer_get_weight_average": [_vp, C.c_int, _f32p, C.c_int64],
    "oz_trainer_sqsum": [_vp, C.c_int, C.POINTER(C.c_double)],
    "oz_trainer_time_optimizer": [_vp, C.c_int, _f64p],
    "oz_replay_create": [C.POINTER(_vp), C.c_int, C.c_int64], "oz_replay_destroy": [_vp], "oz_replay_clear": [_vp],
    "oz_replay_info": [_vp, _i64p, _i64p, _i64p],
    "oz_replay_append_selfplay": [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_double, _i64p],
    "oz_replay_append_records": [_vp, _vp, _i32p, C.c_int64, C.c_int, C.c_int, C.c_double],
    "oz_replay_append_selfplay_targets": [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_double, _i64p],
    "oz_replay_append_selfplay_weighted": [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, _i64p, _i64p],
    "oz_replay_append_records_values": [_vp, _vp, _i32p, _f32p, C.c_int64, C.c_int, C.c_int, C.c_double],
    "oz_replay_append_examples": [_vp, _u64p, _u64p, _f32p, _f32p, C.c_int64],
    "oz_replay_restore": [_vp, _u64p, _u64p, _f32p, _f32p, C.c_int64, C.c_int64],
    "oz_replay_read": [_vp, C.c_int64, C.c_int64, _u64p, _u64p, _f32p, _f32p],
    "oz_trainer_fit_epoch_replay": [_vp, _vp, _i32p, C.c_int64, C.c_int, _f32p],
    "oz_trainer_evaluate_replay": [_vp, _vp, _i32p, C.c_int64, C.c_int, _f64p],
    # auxiliary heads
    "oz_aux_targets": [_vp, C.c_int64, _u64p, _u64p],
    "oz_trainer_arena_size_aux": [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)],
    "oz_trainer_set_aux_heads": [_vp, C.c_float, C.c_float],
    "oz_trainer_get_aux_heads": [_vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "oz_trainer_forward_backward_aux": [_vp, _u64p, _u64p, _f32p, _f32p, _u64p, _u64p, C.c_int, _f32p],
    "oz_trainer_set_dataset_aux": [_vp, _u64p, _u64p, _f32p, _f32p, _u64p, _u64p, C.c_int64],
    "oz_trainer_aux_outputs": [_vp, C.c_int, _f32p, _f32p],
    "oz_trainer_get_aux_losses": [_vp, _f32p, _f64p],
    "oz_trainer_get_aux_head_grads": [_vp, C.c_int, _f32p, _f32p, _f32p],
    "oz_replay_create_aux": [C.POINTER(_vp), C.c_int, C.c_int64], "oz_replay_has_aux": [_vp, C.POINTER(C.c_int)],
    "oz_replay_append_examples_aux": [_vp, _u64p, _u64p, _f32p, _f32p, _u64p, _u64p, C.c_int64],
    "oz_replay_restore_aux": [_vp, _u64p, _u64p, _f32p, _f32p, _u64p, _u64p, C.c_int64, C.c_int64],
    "oz_replay_read_aux": [_vp, C.c_int64, C.c_int64, _u64p, _u64p],
}

_LIB = None
PRELOAD_TORCH_HIP = True          # set to False before the first load() to bind the library to the system ROCm runtime even where PyTorch is installed


HIP_RUNTIME_BOUND = None          # after load(): "torch:<path>" (PyTorch's bundled runtime was preloaded) or "system"


def _elf_dynamic_strings(path):
    """(DT_SONAME or None, [DT_NEEDED ...]) of a little-endian ELF64 shared object, read without external tools"""
    import struct
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise ValueError("not a little-endian ELF64 file")
    phoff, = struct.unpack_from("<Q", data, 0x20)
    phentsize, phnum = struct.unpack_from("<HH", data, 0x36)
    loads, dyn = [], None
    for k in range(phnum):
        p_type, _flags, p_offset, p_vaddr, _paddr, p_filesz = struct.unpack_from("<IIQQQQ", data, phoff + k * phentsize)
        if p_type == 1:
            loads.append((p_vaddr, p_offset, p_filesz))
        elif p_type == 2:
            dyn = (p_offset, p_filesz)
    if dyn is None:
        return None, []
    entries = [struct.unpack_from("<qQ", data, dyn[0] + 16 * k) for k in range(dyn[1] // 16)]
    strtab = next((v for t, v in entries if t == 5), None)
    if strtab is None:
        return None, []
    off = next((strtab - va + fo for va, fo, sz in loads if va <= strtab < va + sz), strtab)

    def name(idx):
        end = data.index(b"\0", off + idx)
        return data[off + idx:end].decode()
    soname = next((name(v) for t, v in entries if t == 14), None)
    return soname, [name(v) for t, v in entries if t == 1]


def _one_hip_runtime(lib_path):
    """PyTorch wheels bundle their own HIP runtime (torch/lib/libamdhip64.so) and load it by path.  If this library is loaded first it
    binds to the system runtime, a later `import torch` brings the bundled one in as well, and the process holds TWO HIP / HSA runtimes:
    streams and device pointers of one are invalid handles in the other (torch tensors handed to the library, the library's RCCL
    exchange step on torch's RCCL -- `ncclCommInitRank: unhandled cuda error`).  So where PyTorch is installed but not imported yet, its
    runtime is loaded first and the library's DT_NEEDED entry resolves to it -- ONLY when that is the runtime the library was linked
    against: the bundled file's SONAME must equal the library's DT_NEEDED name (libamdhip64.so.<major>); otherwise the system runtime is
    used and a warning says so (a silent major-version mix fails, or loads two runtimes anyway, with no message).  Where
    PyTorch is absent (a C host, examples/selfplay_host.c) the system runtime and the system RCCL are used together.
    `othellozero_amd._lib.HIP_RUNTIME_BOUND` records what happened; PRELOAD_TORCH_HIP = False (before the first load) opts out."""
    global HIP_RUNTIME_BOUND
    import importlib.util
    import sys
    import warnings
    HIP_RUNTIME_BOUND = "system"
    if not PRELOAD_TORCH_HIP:
        return
    try:
        spec = importlib.util.find_spec("torch")
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else None
    except Exception:            # no PyTorch, or an unusual layout: the system runtime it is
        return
    if not cand or not os.path.exists(cand):
        return
    try:
        bundled_soname, _ = _elf_dynamic_strings(cand)
        _, needed = _elf_dynamic_strings(lib_path)
        wanted = next((x for x in needed if x.startswith("libamdhip64.so")), None)
    except Exception as e:
        warnings.warn(f"othellozero_amd: could not compare PyTorch's bundled HIP runtime with the library's ({e}); using the system runtime")
        return
    if "torch" in sys.modules:
        HIP_RUNTIME_BOUND = "torch:" + cand          # already in the process (loaded by path): DT_NEEDED resolves to it by SONAME, or not at all
        if wanted and bundled_soname != wanted:
            warnings.warn(f"othellozero_amd: PyTorch's HIP runtime ({bundled_soname}) is not the one this library was linked against ({wanted}): "
                          "two HIP runtimes in one process; do not hand torch device pointers or streams to the library")
            HIP_RUNTIME_BOUND = "system"
        return
    if wanted and bundled_soname == wanted:
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        HIP_RUNTIME_BOUND = "torch:" + cand
    else:
        warnings.warn(f"othellozero_amd: PyTorch bundles HIP runtime {bundled_soname}, the library was linked against {wanted}: not preloading it; "
                      "a later `import torch` will put two HIP runtimes in this process (keep torch device pointers away from the library)")


def load(path=None):
    """Load the HIP library (no compute).  Raises OzLibraryError if it is missing or unloadable."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OzLibraryError(
            f"{p} not found: the HIP extension is required (no CPU fallback). Build it with "
            "`python -m othellozero_amd.build` (hipcc --offload-arch=gfx950).")
    _one_hip_runtime(p)
    try:
        lib = C.CDLL(p)
    except OSError as e:
        raise OzLibraryError(f"cannot load {p}: {e}") from e
    lib.oz_last_error.restype = C.c_char_p
    lib.oz_last_error.argtypes = []
    for name, args in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise OzLibraryError(f"{p} does not export {name}") from e
        fn.argtypes = args
        fn.restype = C.c_int
    if path is None:
        _LIB = lib
    return lib


def check_root_noise(root_noise):
    """root_noise = None or (alpha, epsilon): Dirichlet noise on the root prior of every searched self-play move.  Returns None or the pair
    as floats; ValueError for anything the library would refuse (alpha in [0.01, 100], epsilon in [0, 1])."""
    if root_noise is None:
        return None
    try:
        alpha, eps = (float(x) for x in root_noise)
    except (TypeError, ValueError):
        raise ValueError(f"root_noise must be None or (alpha, epsilon), got {root_noise!r}") from None
    if not 0.01 <= alpha <= 100.0:
        raise ValueError(f"root_noise: alpha must be in [0.01, 100] (got {alpha})")
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"root_noise: epsilon must be in [0, 1] (got {eps})")
    return alpha, eps


def check_forced_playouts(forced_playouts, root_noise=None, need_noise=True):
    """forced_playouts = None or k: KataGo's forced playouts and policy target pruning on every searched self-play move whose root draws
    noise (include/othellozero_amd.h, "forced playouts").  Returns 0.0 (off: None or 0) or k as a float; ValueError for anything the library
    would refuse: k a number in [0, 16], and -- forcing is a rule of the noisy root -- k > 0 without root_noise (an epsilon of 0 is none)
    where need_noise is set."""
    if forced_playouts is None:
        return 0.0
    if isinstance(forced_playouts, (bool, str, bytes)):
        raise ValueError(f"forced_playouts must be None or a number k in [0, 16], got {forced_playouts!r}")
    try:
        k = float(forced_playouts)
    except (TypeError, ValueError):
        raise ValueError(f"forced_playouts must be None or a number k in [0, 16], got {forced_playouts!r}") from None
    if not 0.0 <= k <= 16.0:
        raise ValueError(f"forced_playouts: k must be in [0, 16] (got {k})")
    if k > 0.0 and need_noise and (root_noise is None or not root_noise[1] > 0.0):
        raise ValueError("forced_playouts needs root_noise=(alpha, epsilon > 0): forcing and pruning are rules of the noisy root")
    return k


EVAL_SYM_OFF, EVAL_SYM_RANDOM, EVAL_SYM_MEAN = 0, 1, 2       # oz_net_set_eval_symmetry
EVAL_SYM_MODES = {"off": EVAL_SYM_OFF, "random": EVAL_SYM_RANDOM, "mean": EVAL_SYM_MEAN}
EVAL_SYM_NAMES = {v: k for k, v in EVAL_SYM_MODES.items()}


GUMBEL_DEFAULT = (16, 50.0, 1.0)


def check_gumbel(gumbel):
    """gumbel = None, True (= GUMBEL_DEFAULT) or (max_considered, c_visit, c_scale): the Gumbel root search of include/othellozero_amd.h,
    "Gumbel search".  Returns None or the triple (int, float, float); ValueError for what the library would refuse: max_considered an integer in
    [1, 64], c_visit in [0, 1e9], c_scale in (0, 1e9]."""
    if gumbel is None or gumbel is False:
        return None
    if gumbel is True:
        return GUMBEL_DEFAULT
    try:
        m, c_visit, c_scale = gumbel
        if isinstance(m, bool) or int(m) != m:
            raise TypeError
        m, c_visit, c_scale = int(m), float(c_visit), float(c_scale)
    except (TypeError, ValueError):
        raise ValueError(f"gumbel must be None, True or (max_considered, c_visit, c_scale), got {gumbel!r}") from None
    if not 1 <= m <= 64:
        raise ValueError(f"gumbel: max_considered must be in [1, 64] (got {m})")
    if not 0.0 <= c_visit <= 1e9:
        raise ValueError(f"gumbel: c_visit must be in [0, 1e9] (got {c_visit})")
    if not 0.0 < c_scale <= 1e9:
        raise ValueError(f"gumbel: c_scale must be in (0, 1e9] (got {c_scale})")
    return m, c_visit, c_scale


def check_gumbel_options(gumbel, root_noise=None, forced_playouts=None, sample_moves=None, playout_cap=None, leaves_per_step=1,
                         free_running=False, distributed=False):
    """check_gumbel plus what the Gumbel search does not combine with -- a ValueError before any library call: root_noise, forced_playouts
    and sample_moves (it replaces them), playout_cap (two budgets and two schedules), leaves_per_step > 1, the free-running driver and
    distributed self-play."""
    gumbel = check_gumbel(gumbel)
    if gumbel is None:
        return None
    if root_noise is not None or (forced_playouts is not None and forced_playouts != 0) or sample_moves is not None:
        raise ValueError("gumbel replaces root_noise, forced_playouts and sample_moves: leave them off")
    if playout_cap is not None:
        raise ValueError("gumbel does not combine with playout_cap (a cap needs two budgets and two schedules)")
    if int(leaves_per_step) != 1:
        raise ValueError(f"gumbel runs one leaf per game and step (leaves_per_step is {leaves_per_step})")
    if free_running:
        raise ValueError("gumbel runs in the lock-step rounds only (not the free-running driver, not stagger)")
    if distributed:
        raise ValueError("gumbel is not offered with distributed=True")
    return gumbel


def check_eval_symmetry(mode, seed=0):
    """mode = None, "off", "random" or "mean", seed a whole number in [0, 2^64): the orientation a network evaluates a position in
    (include/othellozero_amd.h, "evaluation symmetry").  Returns (OZ_EVAL_SYM_* code, seed); ValueError for anything else."""
    if mode is None:
        mode = "off"
    if not isinstance(mode, str) or mode not in EVAL_SYM_MODES:
        raise ValueError(f'eval_symmetry: mode must be None, "off", "random" or "mean" (got {mode!r})')
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"eval_symmetry: seed must be a whole number in [0, 2^64) (got {seed!r})")
    return EVAL_SYM_MODES[mode], int(seed)


def check_sample_moves(sample_moves):
    """sample_moves = None or (temperature, plies): the greedy branch of the self-play coin draws the move of the first `plies` plies in
    proportion to N ** (1 / temperature) instead of taking the arg-max.  Returns None or (float, int); ValueError for anything the library
    would refuse (temperature in [0.01, 100], plies a whole number in [0, 64])."""
    if sample_moves is None:
        return None
    try:
        temperature, plies = sample_moves
        temperature = float(temperature)
        if isinstance(plies, bool) or int(plies) != plies:
            raise ValueError
        plies = int(plies)
    except (TypeError, ValueError):
        raise ValueError(f"sample_moves must be None or (temperature, plies), got {sample_moves!r}") from None
    if not 0.01 <= temperature <= 100.0:
        raise ValueError(f"sample_moves: temperature must be in [0.01, 100] (got {temperature})")
    if not 0 <= plies <= 64:
        raise ValueError(f"sample_moves: plies must be in [0, 64] (got {plies})")
    return temperature, plies


def check_playout_cap(playout_cap, num_simulations=None):
    """playout_cap = None or (fast_sims, full_prob): a searched self-play move runs num_simulations simulations with probability full_prob and
    fast_sims otherwise, and only the fully searched moves become training examples (oz_selfplay_set_playout_cap).  Returns None or
    (int, float); ValueError for anything the library would refuse: fast_sims a whole number in [2, num_simulations] (the upper bound is
    checked where num_simulations is given), full_prob in (0, 1]."""
    if playout_cap is None:
        return None
    try:
        fast_sims, full_prob = playout_cap
        if isinstance(fast_sims, bool) or int(fast_sims) != fast_sims:
            raise ValueError
        fast_sims, full_prob = int(fast_sims), float(full_prob)
    except (TypeError, ValueError):
        raise ValueError(f"playout_cap must be None or (fast_sims, full_prob), got {playout_cap!r}") from None
    if fast_sims < 2 or (num_simulations is not None and fast_sims > num_simulations):
        raise ValueError(f"playout_cap: fast_sims must be in [2, num_simulations{'' if num_simulations is None else ' = %d' % num_simulations}] "
                         f"(got {fast_sims})")
    if not 0.0 < full_prob <= 1.0:
        raise ValueError(f"playout_cap: full_prob must be in (0, 1] (got {full_prob})")
    return fast_sims, full_prob


def check_resign(resign, gumbel=None, free_running=False):
    """resign = None or (v, r, min_ply, keep_prob): resignation of decided self-play games with a played-out audit share
    (include/othellozero_amd.h, "resignation").  A game whose root values, seen from BLACK, stayed at or beyond +-v for r searched moves in
    a row is stopped from ply min_ply on and given to that side; a share keep_prob of the games, drawn per (seed, game id), is played out
    regardless and measures the rule.  Returns None or (float, int, int, float); ValueError for anything the library would refuse: v in
    (0, 1], r a whole number in [1, 8], min_ply a whole number in [0, 64], keep_prob in [0, 1] (NaN refused), and together with gumbel or the
    free-running driver."""
    if resign is None:
        return None
    bad = f"resign must be None or (v, r, min_ply, keep_prob), got {resign!r}"
    try:
        v, r, min_ply, keep_prob = resign
        if any(isinstance(x, (bool, str, bytes)) for x in (v, r, min_ply, keep_prob)) or int(r) != r or int(min_ply) != min_ply:
            raise ValueError
        v, r, min_ply, keep_prob = float(v), int(r), int(min_ply), float(keep_prob)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(bad) from None
    if not 0.0 < v <= 1.0:
        raise ValueError(f"resign: v must be in (0, 1] (got {v})")
    if not 1 <= r <= 8:
        raise ValueError(f"resign: r must be in [1, 8] (got {r})")
    if not 0 <= min_ply <= 64:
        raise ValueError(f"resign: min_ply must be in [0, 64] (got {min_ply})")
    if not 0.0 <= keep_prob <= 1.0:
        raise ValueError(f"resign: keep_prob must be in [0, 1] (got {keep_prob})")
    if gumbel is not None and gumbel is not False:
        raise ValueError("resign does not combine with gumbel")
    if free_running:
        raise ValueError("resign holds for the lock-step rounds only (not the free-running driver, not stagger)")
    return v, r, min_ply, keep_prob


def playout_budgets(seed, game_ids, plies, num_simulations, playout_cap):
    """oz_playout_budgets: the simulation budgets (int32) of the searched self-play moves (game_ids[i], plies[i]) under playout_cap --
    num_simulations for a full move, fast_sims for a fast one; the function the kernels evaluate, run on the host (no GPU needed)"""
    cap = check_playout_cap(playout_cap, num_simulations) or (0, 1.0)
    ids = np.ascontiguousarray(game_ids, dtype=np.uint64).ravel()
    ply = np.ascontiguousarray(plies, dtype=np.int32).ravel()
    assert ids.size == ply.size, (ids.size, ply.size)
    out = np.zeros(ids.size, np.int32)
    check(load().oz_playout_budgets(int(seed), p_u64(ids), p_i32(ply), ids.size, int(num_simulations), cap[0], cap[1], p_i32(out)))
    return out


def check_minimax(depth, evaluation):
    """depth and evaluation of a minimax opponent -> (int depth, OZ_MINIMAX_EVAL_* code); ValueError for anything the library would refuse
    (depth a whole number in 1..OZ_MINIMAX_MAX_DEPTH, evaluation "discs" or "weighted")."""
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= depth <= MINIMAX_MAX_DEPTH:
        raise ValueError(f"minimax: depth must be a whole number in 1..{MINIMAX_MAX_DEPTH} (got {depth!r})")
    if not isinstance(evaluation, str) or evaluation not in MINIMAX_EVALS:
        raise ValueError(f"minimax: evaluation must be 'discs' or 'weighted' (got {evaluation!r})")
    return int(depth), MINIMAX_EVALS[evaluation]


def check_solve_empties(empties, least=0, what="max_empties"):
    """the empties bound of the exact endgame solver -> int; ValueError for anything the library would refuse (a whole number in
    least..OZ_SOLVE_MAX_EMPTIES; least is 0 where 0 means "off" or "finished boards only", 1 for oz_selfplay_solve_records)."""
    if isinstance(empties, bool) or not isinstance(empties, (int, np.integer)) or not least <= empties <= SOLVE_MAX_EMPTIES:
        raise ValueError(f"endgame solver: {what} must be a whole number in {least}..{SOLVE_MAX_EMPTIES} (got {empties!r})")
    return int(empties)


def check_solve_leaves(solve_leaves, what="solve_leaves"):
    """solve_leaves=E of the searches (oz_mcts_set_solve_leaves) -> int E; 0 is off.  ValueError for anything the library would refuse: a
    whole number in 0..OZ_SOLVE_LEAVES_MAX_EMPTIES, which is below the solver's own bound (a search step waits for its slowest row)."""
    if (isinstance(solve_leaves, bool) or not isinstance(solve_leaves, (int, np.integer))
            or not 0 <= solve_leaves <= SOLVE_LEAVES_MAX_EMPTIES):
        raise ValueError(f"{what} must be a whole number in 0..{SOLVE_LEAVES_MAX_EMPTIES} (got {solve_leaves!r})")
    return int(solve_leaves)


def check_solve_leaves_pair(solve_leaves):
    """arena_batch(solve_leaves=E or (E_black, E_white)) -> (int, int)"""
    if isinstance(solve_leaves, (tuple, list)):
        if len(solve_leaves) != 2:
            raise ValueError(f"solve_leaves must be E or (E_black, E_white) (got {solve_leaves!r})")
        return check_solve_leaves(solve_leaves[0], "solve_leaves[black]"), check_solve_leaves(solve_leaves[1], "solve_leaves[white]")
    e = check_solve_leaves(solve_leaves)
    return e, e


VALUE_SIGNS = {"reference": 0, "sound": 1}     # OZ_VALUE_SIGNS_*


def check_value_signs(value_signs, what="value_signs"):
    """value_signs="reference" | "sound" of the searches (oz_mcts_set_value_signs) -> the library's mode number; ValueError otherwise"""
    if not isinstance(value_signs, str) or value_signs not in VALUE_SIGNS:
        raise ValueError(f"{what} must be 'reference' or 'sound' (got {value_signs!r})")
    return VALUE_SIGNS[value_signs]


def check_value_signs_pair(value_signs):
    """arena_batch(value_signs=mode or (mode_black, mode_white)) -> (int, int)"""
    if isinstance(value_signs, (tuple, list)):
        if len(value_signs) != 2:
            raise ValueError(f"value_signs must be one mode or (black, white) (got {value_signs!r})")
        return check_value_signs(value_signs[0], "value_signs[black]"), check_value_signs(value_signs[1], "value_signs[white]")
    m = check_value_signs(value_signs)
    return m, m


SELECT_FPU, SELECT_GROWTH, SELECT_PRIOR_FIRST = 1, 2, 4     # OZ_SELECT_*
SELECTION_KEYS = ("fpu", "cpuct_growth", "prior_first")


def _selection_pair(value, what, lo_open, hi):
    """two finite floats; the first in (0, inf) where lo_open, else both in [0, hi]"""
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__") or len(value) != 2:
        raise ValueError(f"{what} must be a pair of numbers (got {value!r})")
    out = []
    for i, x in enumerate(value):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what}[{i}] must be a number (got {x!r})")
        x = float(x)
        low_ok = x > 0.0 if (lo_open and i == 0) else x >= 0.0
        if not (low_ok and x <= hi and x != float("inf")):              # (NaN fails the compares)
            raise ValueError(f"{what}[{i}] = {x!r} outside the range the library takes")
        out.append(x)
    return tuple(out)


def check_selection(selection, what="selection", gumbel=None, forced_playouts=None):
    """selection=None | dict(fpu=(reduction, root_reduction), cpuct_growth=(base, factor), prior_first=bool) of the searches
    (oz_mcts_set_selection; include/othellozero_amd.h, "selection") -> (flags, fpu_reduction, fpu_root_reduction, cpuct_base, cpuct_factor),
    flags == 0 where every part is off.  ValueError for anything the library would refuse -- both reductions in [0, 4], base > 0, factor >= 0,
    all finite -- and for the Gumbel search or forced playouts beside it, before the library is touched."""
    if selection is None:
        return (0, 0.0, 0.0, 0.0, 0.0)
    if not isinstance(selection, dict):
        raise ValueError(f"{what} must be None or a dict with the keys {SELECTION_KEYS} (got {selection!r})")
    unknown = [k for k in selection if k not in SELECTION_KEYS]
    if unknown:
        raise ValueError(f"{what}: unknown key(s) {unknown!r} (known: {SELECTION_KEYS})")
    flags, fpu, growth = 0, (0.0, 0.0), (0.0, 0.0)
    if selection.get("fpu") is not None:
        fpu = _selection_pair(selection["fpu"], f"{what}['fpu']", False, 4.0)
        flags |= SELECT_FPU
    if selection.get("cpuct_growth") is not None:
        growth = _selection_pair(selection["cpuct_growth"], f"{what}['cpuct_growth']", True, float("inf"))
        flags |= SELECT_GROWTH
    pf = selection.get("prior_first", False)
    if not isinstance(pf, (bool, np.bool_)):
        raise ValueError(f"{what}['prior_first'] must be True or False (got {pf!r})")
    if pf:
        flags |= SELECT_PRIOR_FIRST
    if flags and gumbel is not None:
        raise ValueError(f"{what} does not combine with the Gumbel search (its root rule is not PUCT)")
    if flags and forced_playouts:
        raise ValueError(f"{what} does not combine with forced playouts (their quota and pruning restate PUCT with the constant c)")
    return (flags, fpu[0], fpu[1], growth[0], growth[1])


def check_selection_pair(selection):
    """arena_batch(selection=one value or (black, white)) -> (checked, checked)"""
    if isinstance(selection, (tuple, list)):
        if len(selection) != 2:
            raise ValueError(f"selection must be one value or (black, white) (got {selection!r})")
        return check_selection(selection[0], "selection[black]"), check_selection(selection[1], "selection[white]")
    s = check_selection(selection)
    return s, s


def selection_dict(checked):
    """the keyword's form of a checked selection (what OthelloMCTS.selection reads back): None where the option is off"""
    flags, f, fr, b, k = checked
    if not flags:
        return None
    return dict(fpu=(f, fr) if flags & SELECT_FPU else None, cpuct_growth=(b, k) if flags & SELECT_GROWTH else None,
                prior_first=bool(flags & SELECT_PRIOR_FIRST))


TREE_GC = {"off": 0, "demand": 1, "every": 2}   # OZ_TREE_GC_*
TREE_GC_STATS = ("collections", "nodes_before_sum", "nodes_kept_sum", "peak_nodes", "peak_kept")     # oz_tree_gc_stats


def check_tree_gc(tree_gc, what="tree_gc"):
    """tree_gc="off" | "demand" | "every" of the searches (include/othellozero_amd.h, "tree collection") -> the library's mode number;
    ValueError otherwise, before the library is touched"""
    if not isinstance(tree_gc, str) or tree_gc not in TREE_GC:
        raise ValueError(f"{what} must be 'off', 'demand' or 'every' (got {tree_gc!r})")
    return TREE_GC[tree_gc]


def check_tree_gc_pair(tree_gc):
    """arena_batch(tree_gc=mode or (mode_black, mode_white)) -> (int, int)"""
    if isinstance(tree_gc, (tuple, list)):
        if len(tree_gc) != 2:
            raise ValueError(f"tree_gc must be one mode or (black, white) (got {tree_gc!r})")
        return check_tree_gc(tree_gc[0], "tree_gc[black]"), check_tree_gc(tree_gc[1], "tree_gc[white]")
    m = check_tree_gc(tree_gc)
    return m, m


def tree_gc_stats_dict(st):
    return {k: int(getattr(st, k)) for k in TREE_GC_STATS}


def search_tree_keep(root_own, root_opp, own, opp):
    """oz_search_tree_keep on the host: (keep uint8[count], new_index int32[count], kept)"""
    own = np.ascontiguousarray(own, dtype=np.uint64).ravel()
    opp = np.ascontiguousarray(opp, dtype=np.uint64).ravel()
    if own.size != opp.size:
        raise ValueError("own and opp must have the same length")
    keep = np.zeros(own.size, dtype=np.uint8)
    new_index = np.zeros(own.size, dtype=np.int32)
    kept = C.c_int64(0)
    check(load().oz_search_tree_keep(int(root_own), int(root_opp), own.ctypes.data_as(_u64p), opp.ctypes.data_as(_u64p), own.size,
                                     keep.ctypes.data_as(_u8p), new_index.ctypes.data_as(_i32p), C.byref(kept)))
    return keep, new_index, int(kept.value)


PROOF_UNKNOWN = -128                            # OZ_PROOF_UNKNOWN
PROOF_STATS = ("edges_proven", "edge_stops", "node_stops", "roots_proven")     # oz_mcts_proof_stats


def check_proofs(proofs, value_signs, what="proofs", gumbel=None, forced_playouts=None):
    """proofs=True | False of the searches (oz_mcts_set_proofs) -> bool; on needs value_signs="sound" and neither the Gumbel search nor
    forced playouts: ValueError otherwise, before the library is touched"""
    if not isinstance(proofs, (bool, int, np.bool_)) or proofs not in (0, 1):
        raise ValueError(f"{what} must be True or False (got {proofs!r})")
    if proofs and value_signs != "sound":
        raise ValueError(f"{what}=True needs value_signs='sound' (got {value_signs!r}): a proof built on the reference's finished boards is wrong")
    if proofs and gumbel is not None:
        raise ValueError(f"{what}=True does not combine with the Gumbel search")
    if proofs and forced_playouts:
        raise ValueError(f"{what}=True does not combine with forced playouts")
    return bool(proofs)


def check_proofs_pair(proofs, value_signs):
    """arena_batch(proofs=flag or (black, white)) with value_signs=mode or (black, white) -> (bool, bool)"""
    vs = tuple(value_signs) if isinstance(value_signs, (tuple, list)) else (value_signs, value_signs)
    if isinstance(proofs, (tuple, list)):
        if len(proofs) != 2:
            raise ValueError(f"proofs must be one flag or (black, white) (got {proofs!r})")
        return check_proofs(proofs[0], vs[0], "proofs[black]"), check_proofs(proofs[1], vs[1], "proofs[white]")
    if proofs and vs[0] != vs[1]:
        raise ValueError("proofs=True with two value_signs: give proofs=(black, white)")
    p = check_proofs(proofs, vs[0])
    return p, p


PROOF_PLAY_STATS = ("proven_roots", "rows_changed", "moves_changed", "fallbacks")     # oz_selfplay_proof_play_stats


def check_proof_play(proof_play, proofs, what="proof_play"):
    """proof_play=True | False (include/othellozero_amd.h, "proof play") -> bool; on needs proofs=True: ValueError otherwise, before the
    library is touched"""
    if not isinstance(proof_play, (bool, int, np.bool_)) or proof_play not in (0, 1):
        raise ValueError(f"{what} must be True or False (got {proof_play!r})")
    if proof_play and not proofs:
        raise ValueError(f"{what}=True needs proofs=True: it plays and records what the proofs know")
    return bool(proof_play)


def check_proof_play_pair(proof_play, proofs):
    """arena_batch(proof_play=flag or (black, white)) with proofs = the checked (black, white) pair -> (bool, bool)"""
    if isinstance(proof_play, (tuple, list)):
        if len(proof_play) != 2:
            raise ValueError(f"proof_play must be one flag or (black, white) (got {proof_play!r})")
        return check_proof_play(proof_play[0], proofs[0], "proof_play[black]"), check_proof_play(proof_play[1], proofs[1], "proof_play[white]")
    if proof_play and proofs[0] != proofs[1]:
        raise ValueError("proof_play=True with proofs on one agent: give proof_play=(black, white)")
    p = check_proof_play(proof_play, proofs[0])
    return p, p


def check_proof_targets(proof_targets, proof_play):
    """proof_targets=True | False -> bool; on needs proof_play=True (the records carry no proof code without it)"""
    if not isinstance(proof_targets, (bool, int, np.bool_)) or proof_targets not in (0, 1):
        raise ValueError(f"proof_targets must be True or False (got {proof_targets!r})")
    if proof_targets and not proof_play:
        raise ValueError("proof_targets=True needs proof_play=True: the records carry no proof code without it")
    return bool(proof_targets)


def record_proven(records):
    """the proven value of move records (RECORD_DTYPE) for the mover: int8 -1 / 0 / +1, PROOF_UNKNOWN where the record carries no proof
    code (pad[2] == 0: the third spare byte of oz_record, always 0 without proof play)"""
    code = np.asarray(records)["pad"][..., 2].astype(np.int16)
    return np.where(code == 0, PROOF_UNKNOWN, code - 2).astype(np.int8)


def proof_targets(records):
    """oz_proof_targets on the host, in place: z of every record with a proof code becomes the proven sign -> dict(records, proven, z_changed)"""
    records = np.asarray(records)
    if records.dtype != RECORD_DTYPE or not records.flags.c_contiguous or not records.flags.writeable:
        raise ValueError("proof_targets: a writeable contiguous RECORD_DTYPE array")
    st = ProofTargetStats()
    check(load().oz_proof_targets(records.ctypes.data_as(_vp), int(records.size), C.byref(st)))
    return {"records": st.records, "proven": st.proven, "z_changed": st.z_changed}


def check_endgame_targets(endgame_targets, alias_final_boards):
    """training(endgame_targets=E) -> int E; 0 is off.  E > 0 needs alias_final_boards=False: an exact value belongs to the position of the move."""
    e = check_solve_empties(endgame_targets, 0, "endgame_targets")
    if e > 0 and alias_final_boards:
        raise ValueError("endgame_targets needs alias_final_boards=False: an exact value belongs to the position of its move, not to the "
                         "game's final position")
    return e


def check_value_target(value_target, alias_final_boards=False):
    """value_target = None / "outcome" (the records' z), ("blend", w) or ("td", lam), both parameters in [0, 1]: the value target of the
    training examples (include/othellozero_amd.h, "value targets").  Returns (OZ_VALUE_TARGET_* code, parameter) -- (VALUE_TARGET_OUTCOME,
    0.0) is the option off; ValueError for anything else, and for a search-value target with alias_final_boards: a search value belongs to
    the position of its move, not to the game's final position."""
    if value_target is None or (isinstance(value_target, str) and value_target == "outcome"):
        return VALUE_TARGET_OUTCOME, 0.0
    bad = f'value_target must be None, "outcome", ("blend", w) or ("td", lam), got {value_target!r}'
    if not isinstance(value_target, (tuple, list)) or len(value_target) != 2 or not isinstance(value_target[0], str) \
            or value_target[0] not in ("blend", "td"):
        raise ValueError(bad)
    if isinstance(value_target[1], (bool, str, bytes)):
        raise ValueError(bad)
    try:
        param = float(value_target[1])
    except (TypeError, ValueError):
        raise ValueError(bad) from None
    if not 0.0 <= param <= 1.0:
        raise ValueError(f"value_target: the parameter of {value_target[0]!r} must be in [0, 1] (got {param})")
    if alias_final_boards:
        raise ValueError("value_target needs alias_final_boards=False: a search value belongs to the position of its move, not to the game's "
                         "final position")
    return VALUE_TARGET_MODES[value_target[0]], param


def check_aux_heads(aux_heads, what="aux_heads"):
    """aux_heads = None / False (off) or dict(ownership=w, score=w): the loss weights of the trainer's auxiliary heads (include/othellozero_amd.h,
    "auxiliary heads"), finite and >= 0, a missing key 0.  -> None or (w_own, w_score); ValueError for anything else.  The one check of the
    option: Trainer, NNetWrapper and loop.training call it; no GPU needed"""
    if aux_heads is None or aux_heads is False:
        return None
    bad = f"{what} must be None or dict(ownership=weight, score=weight) with finite weights >= 0, got {aux_heads!r}"
    if not isinstance(aux_heads, dict) or set(aux_heads) - {"ownership", "score"}:
        raise ValueError(bad)
    w = []
    for key in ("ownership", "score"):
        x = aux_heads.get(key, 0.0)
        if isinstance(x, (bool, str, bytes)):
            raise ValueError(bad)
        try:
            x = float(x)
        except (TypeError, ValueError):
            raise ValueError(bad) from None
        if not (x >= 0.0 and x < float("inf")):
            raise ValueError(bad)
        w.append(x)
    return tuple(w)


def check_aux_heads_loop(aux_heads, replay="host", distributed=False, alias_final_boards=False, in_channels=2):
    """training(aux_heads=...) -> None (off) or the dict to hand to the network.  The final pairs travel in the slots of the device replay buffer
    alone: replay="host" and distributed=True are refused (the host example tuples and the pooled rows do not carry them).  With
    alias_final_boards=True a two-plane network's examples SHOW the final board (the reference's aliased view): the ownership target would be
    the input itself, so that is refused too; a one-plane network's examples are the positions at the move whatever alias_final_boards says
    (examples_from_records), and pass."""
    w = check_aux_heads(aux_heads)
    if w is None:
        return None
    if distributed:
        raise ValueError("aux_heads is not offered with distributed=True: the pooled rows of the all-gather do not carry the final pairs, and the "
                         "device replay buffer that does is single-process")
    if replay != "device":
        raise ValueError("aux_heads needs replay='device': the final pairs are slots of the device replay buffer (ReplayBuffer(aux=True)); the "
                         "host example tuples do not carry them")
    if alias_final_boards and in_channels == 2:
        raise ValueError("aux_heads needs alias_final_boards=False for a two-plane network: the aliased view shows every example as the game's "
                         "final board, which is the ownership target itself")
    return dict(ownership=w[0], score=w[1])


def check_surprise_frac(frac, what="surprise_weight"):
    """the frac of policy surprise weighting (include/othellozero_amd.h, "policy surprise weighting"): a number in (0, 1] -> float;
    ValueError for anything else (NaN included)"""
    if isinstance(frac, (bool, str, bytes)):
        raise ValueError(f"{what}: frac must be a number in (0, 1], got {frac!r}")
    try:
        f = float(frac)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: frac must be a number in (0, 1], got {frac!r}") from None
    if not 0.0 < f <= 1.0:
        raise ValueError(f"{what}: frac must be in (0, 1] (got {f})")
    return f


def check_search_options(solve_leaves=0, value_signs="reference", proofs=False, proof_play=False, selection=None, tree_gc="off", gumbel=None,
                         forced_playouts=None, pairs=False):
    """The six options every batched search takes -- engines, arenas and the wrappers above them -- checked once, rules between them
    included (proofs need sound signs, proof play needs proofs; selection and proofs stand beside neither `gumbel` nor `forced_playouts`,
    which a self-play caller passes along).  pairs=True: each may also be a (black, white) pair, as arena_batch takes them.  -> the dict of
    the six in the form a keyword carries them (solve_leaves an int, proofs and proof_play bools where they are not pairs); it is its own
    valid input.  ValueError for anything else, in the order SelfPlayEngine has always looked."""
    if pairs:
        check_tree_gc_pair(tree_gc)
        check_selection_pair(selection)
        check_value_signs_pair(value_signs)
        check_proof_play_pair(proof_play, check_proofs_pair(proofs, value_signs))
        check_solve_leaves_pair(solve_leaves)
    else:
        check_tree_gc(tree_gc)
        check_selection(selection, gumbel=gumbel, forced_playouts=forced_playouts)
        check_value_signs(value_signs)
        proofs = check_proofs(proofs, value_signs, gumbel=gumbel, forced_playouts=forced_playouts)
        proof_play = check_proof_play(proof_play, proofs)
        solve_leaves = check_solve_leaves(solve_leaves)
    return dict(solve_leaves=solve_leaves, value_signs=value_signs, proofs=proofs, proof_play=proof_play, selection=selection, tree_gc=tree_gc)


def check_selfplay_options(num_simulations, record_visits=False, leaves_per_step=1, root_noise=None, sample_moves=None, solve_leaves=0,
                           playout_cap=None, forced_playouts=None, record_values=False, gumbel=None, record_surprise=False, resign=None,
                           value_signs="reference", proofs=False, proof_play=False, selection=None, tree_gc="off"):
    """Everything SelfPlayEngine takes beyond its plain configuration, checked once and in the engine's order: check_search_options, then
    resign (not with gumbel), recorded surprise (needs visit rows or gumbel), gumbel (replaces noise, forcing and sampling; no cap, one
    leaf per step), the playout cap against num_simulations, solve_leaves, root noise, forced playouts (need noise) and move sampling.
    -> the dict of all sixteen with the checked values; it is its own valid input, so a wrapper hands its result on.  ValueError otherwise,
    before the network or the library is touched."""
    o = check_search_options(0, value_signs, proofs, proof_play, selection, tree_gc, gumbel=gumbel, forced_playouts=forced_playouts)
    resign = check_resign(resign, gumbel=gumbel)
    if record_surprise and not (record_visits or gumbel):
        raise ValueError("record_surprise needs record_visits=True or gumbel=...: the surprise is that of a recorded policy target")
    gumbel = check_gumbel_options(gumbel, root_noise=root_noise, forced_playouts=forced_playouts, sample_moves=sample_moves,
                                  playout_cap=playout_cap, leaves_per_step=leaves_per_step)
    playout_cap = check_playout_cap(playout_cap, num_simulations)
    o["solve_leaves"] = check_solve_leaves(solve_leaves)                # (here, not above: where the engine has always checked it)
    root_noise = check_root_noise(root_noise)
    return dict(o, record_visits=record_visits, leaves_per_step=leaves_per_step, root_noise=root_noise, sample_moves=check_sample_moves(sample_moves),
                playout_cap=playout_cap, forced_playouts=check_forced_playouts(forced_playouts, root_noise), record_values=bool(record_values),
                gumbel=gumbel, record_surprise=bool(record_surprise), resign=resign)


def _given(value):
    return value is not None


_SEARCH_ON = dict(solve_leaves=lambda e: e != 0, value_signs=lambda mode: mode != "reference", proofs=bool, proof_play=bool,
                  selection=lambda s: check_selection(s)[0] != 0, tree_gc=lambda mode: mode != "off")
_ENGINE_ON = dict(_SEARCH_ON, record_visits=bool, leaves_per_step=lambda k: int(k) != 1, root_noise=_given, sample_moves=_given,
                  playout_cap=_given, forced_playouts=bool, record_values=bool, gumbel=_given, record_surprise=bool, resign=_given)


def search_kw(checked):
    """the keywords to pass on from check_search_options' dict (or the six of them in check_selfplay_options'): those of the options that
    are on (for a pair: on for either colour), with the caller's value -- nothing for an option that is off, so that callers without it
    see the calls they always saw"""
    return {k: v for k, v in checked.items() if k in _SEARCH_ON and any(_SEARCH_ON[k](x) for x in (v if isinstance(v, (tuple, list)) else (v,)))}


def engine_kw(checked, always=()):
    """search_kw for check_selfplay_options' dict; the names in `always` are passed on whatever their value"""
    return {k: v for k, v in checked.items() if k in always or _ENGINE_ON[k](v)}


def check_opponent(opponent):
    """opponent = None / "random" (RandomOthelloAgent), or ("minimax", depth) / ("minimax", depth, "discs" | "weighted"): who plays the colour that
    has no network in an arena or an evaluation.  Returns None for the random mover, else (depth, OZ_MINIMAX_EVAL_* code) -- the evaluation defaults
    to "weighted"; ValueError for anything else."""
    if opponent is None or (isinstance(opponent, str) and opponent == "random"):
        return None
    if isinstance(opponent, (tuple, list)) and len(opponent) in (2, 3) and isinstance(opponent[0], str) and opponent[0] == "minimax":
        return check_minimax(opponent[1], opponent[2] if len(opponent) == 3 else "weighted")
    raise ValueError(f"opponent must be None, 'random', ('minimax', depth) or ('minimax', depth, 'discs' | 'weighted'), got {opponent!r}")


def check_opponents(opponent, black_free, white_free):
    """the `opponent` argument of an arena whose BLACK / WHITE colour has no network (black_free / white_free) -> (BLACK's, WHITE's) checked
    opponent, each None (random mover, or a colour a network plays) or (depth, evaluation code).  One colour free: `opponent` is check_opponent's
    argument.  Both free: None (random against random) or a dict with the keys "black" / "white", each a check_opponent argument."""
    if isinstance(opponent, dict):
        if set(opponent) - {"black", "white"}:
            raise ValueError(f"opponent: a dict takes the keys 'black' and 'white' (got {sorted(map(str, opponent))})")
        black, white = check_opponent(opponent.get("black")), check_opponent(opponent.get("white"))
        if (black is not None and not black_free) or (white is not None and not white_free):
            raise ValueError("opponent: a colour that has a network cannot be given a minimax opponent")
        return black, white
    spec = check_opponent(opponent)
    if spec is None:
        return None, None
    if black_free and white_free:
        raise ValueError("opponent: neither colour has a network; say who plays which as {'black': ..., 'white': ...}")
    if not black_free and not white_free:
        raise ValueError("opponent: both colours have a network, there is no colour for the minimax opponent to play")
    return (spec, None) if black_free else (None, spec)


def _whole(x, lo, hi):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer)) and lo <= x <= hi


def check_opening_plies(plies, what="openings"):
    """the plies of a random opening -> int; ValueError for anything but a whole number in 0..OZ_OPENING_MAX_PLIES"""
    if not _whole(plies, 0, OPENING_MAX_PLIES):
        raise ValueError(f"{what}: plies must be a whole number in 0..{OPENING_MAX_PLIES} (got {plies!r})")
    return int(plies)


def check_openings(openings=None, first_opening_id=0, opening_moves=None, num_games=None):
    """The opening options of an arena.  openings = None or (plies, opening_seed): random openings (oz_arena_set_openings), game slot g playing
    opening first_opening_id + g.  opening_moves = None or (moves, n_plies): game g plays moves[g][:n_plies[g]] (oz_arena_set_opening_moves);
    moves an unsigned 8-bit integer array of shape (num_games, OZ_OPENING_MAX_PLIES), n_plies a 32-bit integer array of shape (num_games,).
    Returns None (off), ("random", plies, seed, first_opening_id) or ("moves", moves, n_plies) with contiguous arrays; ValueError for anything
    the library would refuse or could not read: both options at once, a wrong tuple shape, a plies that is no whole number (or a bool) or lies
    outside 0..OZ_OPENING_MAX_PLIES, a seed or id that is no whole number in 0..2^64 - 1, arrays of another shape or dtype, an n_plies entry
    out of range.  (Whether a listed move is legal is the library's check: it replays the lists.)"""
    if not _whole(first_opening_id, 0, 2 ** 64 - 1):
        raise ValueError(f"first_opening_id must be a whole number in 0..2^64 - 1 (got {first_opening_id!r})")
    if openings is not None and opening_moves is not None:
        raise ValueError("openings and opening_moves are two ways to say how the games start: give one of them")
    if openings is not None:
        if not isinstance(openings, (tuple, list)) or len(openings) != 2:
            raise ValueError(f"openings must be None or (plies, opening_seed), got {openings!r}")
        plies = check_opening_plies(openings[0])
        if not _whole(openings[1], 0, 2 ** 64 - 1):
            raise ValueError(f"openings: opening_seed must be a whole number in 0..2^64 - 1 (got {openings[1]!r})")
        return "random", plies, int(openings[1]), int(first_opening_id)
    if opening_moves is not None:
        if not isinstance(opening_moves, (tuple, list)) or len(opening_moves) != 2:
            raise ValueError(f"opening_moves must be None or (moves, n_plies), got {opening_moves!r}")
        moves, n_plies = opening_moves
        if not isinstance(moves, np.ndarray) or moves.dtype != np.uint8 or moves.ndim != 2 or moves.shape[1] != OPENING_MAX_PLIES:
            raise ValueError(f"opening_moves: moves must be a uint8 array of shape (num_games, {OPENING_MAX_PLIES})")
        if not isinstance(n_plies, np.ndarray) or n_plies.dtype != np.int32 or n_plies.shape != (moves.shape[0],):
            raise ValueError("opening_moves: n_plies must be an int32 array of shape (num_games,)")
        if num_games is not None and moves.shape[0] != num_games:
            raise ValueError(f"opening_moves: {moves.shape[0]} move lists for {num_games} games")
        if n_plies.size and (n_plies.min() < 0 or n_plies.max() > OPENING_MAX_PLIES):
            raise ValueError(f"opening_moves: every n_plies must be in 0..{OPENING_MAX_PLIES}")
        return "moves", np.ascontiguousarray(moves), np.ascontiguousarray(n_plies)
    return None


def check(rc):
    if rc != OZ_OK:
        msg = load().oz_last_error().decode("utf-8", "replace")
        if rc == OZ_ERR_KEY:
            raise KeyError(msg)
        raise OzError(rc, msg)


def require_gpu():
    lib = load()
    if lib.oz_device_count() <= 0:
        raise OzLibraryError("no HIP device visible: othellozero_amd computes on an MI355X only (no CPU fallback)")
    return lib


def mfma_rate(kind, target_ms=50.0):
    """oz_selftest_mfma_rate: {"tflops", "clock_ghz", "ms"} of a pure-MFMA loop on the current device; kind "f32" / "f16" / "bf16" """
    t, g, m = C.c_double(), C.c_double(), C.c_double()
    check(require_gpu().oz_selftest_mfma_rate({"f32": 0, "f16": 1, "bf16": 2}[kind], float(target_ms), C.byref(t), C.byref(g), C.byref(m)))
    return {"tflops": t.value, "clock_ghz": g.value, "ms": m.value}


# numpy -> pointer helpers
def p_u64(a): return a.ctypes.data_as(_u64p)
def p_i32(a): return a.ctypes.data_as(_i32p)
def p_f32(a): return a.ctypes.data_as(_f32p)
def p_f64(a): return a.ctypes.data_as(_f64p)
def p_u8(a): return a.ctypes.data_as(_u8p)
def p_i8(a): return a.ctypes.data_as(_i8p)
def p_i64(a): return a.ctypes.data_as(_i64p)


def pack_board(board):
    """(n,n,2) array-like (channel 0, channel 1) -> two python ints, bit = row*8 + col."""
    b = np.asarray(board).astype(bool)
    n = b.shape[0]
    w = (np.uint64(1) << (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(8) + np.arange(n, dtype=np.uint64)[None, :]))
    return int(w[b[:, :, 0]].sum(dtype=np.uint64)), int(w[b[:, :, 1]].sum(dtype=np.uint64))


def unpack_board(c0, c1, n):
    sq = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(8) + np.arange(n, dtype=np.uint64)[None, :])
    out = np.zeros((n, n, 2), dtype=bool)
    out[:, :, 0] = (np.uint64(c0) >> sq) & np.uint64(1)
    out[:, :, 1] = (np.uint64(c1) >> sq) & np.uint64(1)
    return out
