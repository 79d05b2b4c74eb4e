"""What the option wrappers hand on, recorded without a GPU: stand-ins for SelfPlayEngine, arena_batch and the device replay buffer, the
case list, and `run_case`, which turns one case into a JSON-able trace.  tests/golden/gen_option_calls.py wrote the traces of the commit
before the wrappers were folded into one check, one pass-on and one statistics path; tests/test_option_calls_cpu.py replays the cases.

A trace holds: the positional arguments and the exact keyword set and values SelfPlayEngine / arena_batch receive; the engine's and the
buffer's later calls in order, arguments bound against the real methods' signatures with the defaults applied; the shape of what comes
back (types, lengths, dtypes, which canned array sits where); the function attributes after a call that returns; for a refusal the
exception's type and text.  Reads of statistics (rows_solved(), resign_stats(), ...) change nothing and are left out of the sequence:
what they returned is compared where it ends up, in the function attributes.

The real SelfPlayEngine is traced too, over a stand-in for the library that records every oz_* call: the order and the arguments of
the oz_selfplay_set_* calls of a constructor, and what records() asks the library for and hands back with every flag set.

The engine stand-in runs the real constructor's checks (the real __init__ up to its first step towards the library, which a private
exception ends) and the real play_to_end over recorded primitives, so a refusal of the real engine is one of the stand-in too.
"""
import contextlib
import ctypes
import inspect

import numpy as np

from othellozero_amd import _lib, loop, replay, training

REAL_ENGINE, REAL_APPEND = training.SelfPlayEngine, replay.ReplayBuffer.append_engine
R = 3                                                   # canned records per engine
NET, OLD = "<net>", "<old net>"
STAT_READS = ("rows_solved", "playout_stats", "forced_playout_stats", "resign_stats", "gumbel_stats", "proof_stats", "proof_play_stats",
              "tree_gc_stats")
ENGINE_STEPS = ("run", "stats", "proof_targets", "solve_records", "value_targets", "surprise_weights", "records")
BATCH_ATTRS = ("rows_solved", "endgame_stats", "value_target_stats", "playout_stats", "forced_playout_stats", "gumbel_stats", "resign_stats",
               "surprise_stats", "proof_stats", "proof_play_stats", "proof_target_stats", "tree_gc_stats")
TRAINING_ATTRS = ("rows_solved", "resign_history", "surprise_history", "validation_history", "match_history", "proof_history",
                  "proof_play_history", "endgame_history")


class _Reached(Exception):
    """the real constructor got past its checks"""


class _Stop(Exception):
    """the loop got as far as the case follows it"""


def plain(x):
    """x as JSON holds it: networks by name, arrays by (dtype, shape, first entry), tuples told from lists"""
    if isinstance(x, StubNet):
        return x.name
    if isinstance(x, FakeEngine):
        return "<engine>"
    if isinstance(x, np.ndarray):
        if x.dtype.names:
            return {"records": list(x.shape)}
        return {"array": str(x.dtype), "shape": list(x.shape), "first": float(x.flat[0]) if x.size else None}
    if isinstance(x, tuple):
        return {"tuple": [plain(e) for e in x]}
    if isinstance(x, list):
        return [plain(e) for e in x]
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (np.integer, np.floating, np.bool_)):
        return x.item()
    assert x is None or isinstance(x, (bool, int, float, str)), repr(x)
    return x


def bound(real, args, kwargs):
    """the arguments of a call as the real function would name them, defaults applied, without self"""
    ba = inspect.signature(real).bind(None, *args, **kwargs)
    ba.apply_defaults()
    return {k: plain(v) for k, v in list(ba.arguments.items())[1:]}


class StubNet:
    """what loop.training reads of a network before its first fit"""
    policy_loss, in_channels = "flat", 2

    def __init__(self, log, name=NET):
        self.log, self.name = log, name

    def copy(self):
        return StubNet(self.log, OLD)

    def eval_symmetry(self):
        return ("off", 0)

    def set_eval_symmetry(self, *a):
        self.log.append(["net.set_eval_symmetry", plain(list(a))])

    def evaluate(self, *a, **k):
        raise _Stop

    def train(self, data, **kw):
        self.log.append(["net.train", "<replay>" if isinstance(data, FakeReplay) else type(data).__name__, plain(kw)])
        raise _Stop


class FakeEngine:
    log = None

    def __init__(self, *args, **kwargs):
        self.log.append(["SelfPlayEngine", plain(list(args)), plain(kwargs)])
        try:
            REAL_ENGINE.__init__(self, *args, **kwargs)
        except _Reached:
            pass
        ba = inspect.signature(REAL_ENGINE.__init__).bind(self, *args, **kwargs)
        ba.apply_defaults()
        a = ba.arguments
        self.n, self.num_games = a["board_size"], a["num_games"]
        self.solve_leaves, self.playout_cap, self.forced_playouts = a["solve_leaves"], a["playout_cap"], float(a["forced_playouts"] or 0.0)
        self.resign, self.gumbel, self.value_signs, self.tree_gc = a["resign"], a["gumbel"] or None, a["value_signs"], a["tree_gc"]
        self.proofs, self.proof_play, self.record_surprise = bool(a["proofs"]), bool(a["proof_play"]), bool(a["record_surprise"])
        self.record_values = bool(a["record_values"]) or self.resign is not None
        self.endgame_stats = self.value_target_stats = self.proof_target_stats = None

    def _step(self, name, args, kwargs):
        self.log.append(["engine." + name, bound(getattr(REAL_ENGINE, name), args, kwargs)])

    def run(self, *a, **k):
        self._step("run", a, k)

    def stats(self):
        self._step("stats", (), {})
        return dict(records=R, live_games=0, games_completed=self.num_games)

    def proof_targets(self, *a, **k):
        self._step("proof_targets", a, k)
        return dict(records=R, proven=2, z_changed=1)

    def solve_records(self, *a, **k):
        self._step("solve_records", a, k)
        return dict(records=R, solved=2, z_changed=1, optimal_moves=1, disc_loss_sum=4, disc_loss_max=4, mean_disc_loss=2.0)

    def value_targets(self, *a, **k):
        self._step("value_targets", a, k)
        return dict(records=R, exact=1, sign_changed=0)

    def surprise_weights(self, *a, **k):
        self._step("surprise_weights", a, k)
        return dict(records=R, full_records=R, examples=20, zero_copies=0, max_copies=9)

    def records(self, *a, **k):
        self._step("records", a, k)
        ba = inspect.signature(REAL_ENGINE.records).bind(self, *a, **k)
        ba.apply_defaults()
        f = ba.arguments
        rec = np.zeros(R, _lib.RECORD_DTYPE)
        rec["ply"] = np.arange(R)
        ret = [rec]
        for flag, dtype, shape, tag in (("with_visits", np.int32, (R, 64), 1), ("with_values", np.float64, (R,), 2),
                                        ("with_targets", np.float32, (R,), 3), ("with_policies", np.float32, (R, 64), 4),
                                        ("with_surprise", np.float64, (R,), 5)):
            if f[flag]:
                ret.append(np.full(shape, tag, dtype))
        if f["with_weights"]:
            ret.append((np.full(R, 6, np.float32), np.full(R, 7, np.int32), np.full(R, 8, np.uint8)))
        return rec if len(ret) == 1 else tuple(ret)

    play_to_end = REAL_ENGINE.play_to_end
    if hasattr(REAL_ENGINE, "option_stats"):
        option_stats = REAL_ENGINE.option_stats


CANNED_READS = dict(
    rows_solved=17, playout_stats=dict(fast_sims=4, full_prob=0.25, full_moves=5, fast_moves=6),
    forced_playout_stats=dict(k=2.0, moves_pruned=1, visits_raw=2, visits_kept=3),
    resign_stats=dict(v=0.9, r=2, min_ply=10, keep_prob=0.1, games_adjudicated=2, adjudicated_plies_sum=30, games_exempt=1, exempt_triggered=1,
                      exempt_wrong=0, exempt_trigger_ply_sum=12),
    gumbel_stats=dict(max_considered=16, c_visit=50.0, c_scale=1.0, moves=9), proof_stats=dict(zip(_lib.PROOF_STATS, (1, 2, 3, 4))),
    proof_play_stats=dict(zip(_lib.PROOF_PLAY_STATS, (5, 6, 7, 8))), tree_gc_stats=dict(mode="demand", **dict.fromkeys(_lib.TREE_GC_STATS, 9)))
for _name in STAT_READS:
    setattr(FakeEngine, _name, (lambda name: lambda self: CANNED_READS[name])(_name))


class FakeLibrary:
    """every oz_* entry: logs its name and its plain arguments (a pointer by its type's name), returns OZ_OK, and answers the two kinds of
    call records() reads from: the statistics, and a row count written behind the last argument"""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def entry(*args):
            self.log.append([name, [a if isinstance(a, (int, float)) else type(getattr(a, "_obj", a)).__name__ for a in args]])
            last = getattr(args[-1], "_obj", None) if args else None
            if name == "oz_selfplay_get_stats":
                last.records = R
            elif isinstance(last, ctypes.c_int64):
                last.value = args[-2]
            return _lib.OZ_OK
        return entry


class FakeReplay:
    log = None
    total = 0
    last_weight_stats = dict(records=R, full_records=R, examples=20, zero_copies=0, max_copies=9)

    def __init__(self, *a, **k):
        self.log.append(["ReplayBuffer", plain(list(a)), plain(k)])

    def append_engine(self, eng, *a, **k):
        self.log.append(["replay.append_engine", bound(REAL_APPEND, (eng,) + a, k)])
        return R

    def info(self):
        return (8 * R, 64, 8 * R)

    def __len__(self):
        return 8 * R


@contextlib.contextmanager
def stand_ins(log):
    """the package with the stand-ins in place; everything is put back on the way out"""
    def reached(*a, **k):
        raise _Reached

    def fake_arena(net_a, net_b, *a, **k):
        log.append(["arena_batch", plain([net_a, net_b] + list(a)), plain(k)])
        g = a[1]
        return dict(winner=np.array([1, -1] * g, np.int8)[:g], final_black=np.full(g, 7, np.uint64), final_white=np.full(g, 3, np.uint64),
                    opening_plies=np.full(g, 4, np.int32))

    def fake_expand(*a, **k):
        log.append(["expand_examples", bound(lambda self, records, board_size, alias_final=False, visits=None, target_temperature=1.0,
                                             values=None: None, a, k)])
        return ("boards", "policies", "z")

    def fake_examples(*a, **k):
        log.append(["examples_from_records", bound(lambda self, records, board_size, alias_final=True, in_channels=2, visits=None,
                                                   target_temperature=1.0, values=None, policies=None: None, a, k)])
        return []
    FakeEngine.log = FakeReplay.log = log
    saved = [(training, "SelfPlayEngine", FakeEngine), (training, "expand_examples", fake_expand), (loop, "arena_batch", fake_arena),
             (loop, "examples_from_records", fake_examples), (replay, "ReplayBuffer", FakeReplay), (_lib, "require_gpu", reached),
             (_lib, "load", reached)]
    saved = [(mod, name, getattr(mod, name), new) for mod, name, new in saved]
    attrs = [(fn, dict(vars(fn))) for fn in (training.selfplay_batch, loop.training, loop.self_play_match)]
    try:
        for mod, name, _old, new in saved:
            setattr(mod, name, new)
        yield
    finally:
        for mod, name, old, _new in saved:
            setattr(mod, name, old)
        for fn, had in attrs:
            vars(fn).clear()
            vars(fn).update(had)


LOOP_KW = dict(board_size=6, num_iterations=1, num_episodes=8, num_simulations=12, degree_exploration=1, temperature=1, e_greedy=0.9,
               evaluation_interval=1, evaluation_iterations=2, temperature_threshold=0, self_play_training=True, self_play_interval=1,
               self_play_total_games=2, self_play_threshold=1, checkpoint_filepath="unused.npz", training_buffer_size=64,
               alias_final_boards=False)
SOUND = dict(value_signs="sound")
PROOFS = dict(SOUND, proofs=True)
PLAY = dict(PROOFS, proof_play=True)
NOISE = dict(root_noise=(0.3, 0.25))
RESIGN = dict(resign=(0.9, 2, 10, 0.1))
FPU = dict(fpu=(0.2, 0.1))

# the options of selfplay_batch and _selfplay_into_replay: each alone, each at its off value spelled out, the documented combinations
ENGINE_OPTIONS = {
    "none": {},
    "root_noise": NOISE,
    "sample_moves": dict(sample_moves=(1.0, 8)),
    "solve_leaves": dict(solve_leaves=6),
    "playout_cap": dict(playout_cap=(4, 0.25)),
    "forced_playouts": dict(NOISE, forced_playouts=2.0),
    "gumbel_true": dict(gumbel=True),
    "gumbel_triple": dict(gumbel=(8, 50.0, 1.0)),
    "resign": RESIGN,
    "value_signs": SOUND,
    "proofs": PROOFS,
    "proof_play": PLAY,
    "proof_targets": dict(PLAY, proof_targets=True),
    "selection": dict(selection=FPU),
    "selection_all": dict(selection=dict(fpu=(0.2, 0.1), cpuct_growth=(19652.0, 1.0), prior_first=True)),
    "tree_gc_demand": dict(tree_gc="demand"),
    "tree_gc_every": dict(tree_gc="every"),
    "leaves_per_step": dict(leaves_per_step=4),
    "value_target_td": dict(value_target=("td", 0.8)),
    "value_target_blend": dict(value_target=("blend", 0.5)),
    "endgame_targets": dict(endgame_targets=8),
    "off_tree_gc": dict(tree_gc="off"),
    "off_selection": dict(selection={}),
    "off_selection_none": dict(selection=None),
    "off_proofs": dict(proofs=False, proof_play=False, proof_targets=False),
    "off_forced_none": dict(forced_playouts=None),
    "off_forced_zero": dict(forced_playouts=0),
    "off_forced_zero_noise": dict(NOISE, forced_playouts=0),
    "off_playout_cap": dict(playout_cap=None),
    "off_resign": dict(resign=None),
    "off_value_signs": dict(value_signs="reference"),
    "off_gumbel": dict(gumbel=None),
    "off_value_target": dict(value_target="outcome"),
    "off_endgame_solve": dict(endgame_targets=0, solve_leaves=0),
    "noise_forcing": dict(NOISE, forced_playouts=2.0, sample_moves=(1.0, 8)),
    "gumbel_value_target": dict(gumbel=True, value_target=("td", 0.8)),
    "proofs_all_targets": dict(PLAY, proof_targets=True, value_target=("td", 0.8), endgame_targets=8, solve_leaves=6),
    "cap_resign_solved": dict(RESIGN, playout_cap=(4, 0.25), solve_leaves=6),
    "everything_puct": dict(PLAY, **NOISE, **RESIGN, proof_targets=True, playout_cap=(4, 0.25), solve_leaves=6, sample_moves=(1.0, 8),
                            tree_gc="demand", leaves_per_step=2, value_target=("blend", 0.5), endgame_targets=8),
}
REFUSALS = {
    "forced_without_noise": dict(forced_playouts=2.0),
    "forced_zero_epsilon": dict(root_noise=(0.3, 0.0), forced_playouts=2.0),
    "forced_range": dict(NOISE, forced_playouts=17),
    "root_noise_alpha": dict(root_noise=(0.001, 0.25)),
    "root_noise_shape": dict(root_noise=0.3),
    "sample_moves_plies": dict(sample_moves=(1.0, 65)),
    "solve_leaves_range": dict(solve_leaves=11),
    "solve_leaves_bool": dict(solve_leaves=True),
    "playout_cap_sims": dict(playout_cap=(13, 0.25)),
    "playout_cap_prob": dict(playout_cap=(4, 0.0)),
    "gumbel_shape": dict(gumbel=(8, 50.0)),
    "gumbel_noise": dict(NOISE, gumbel=True),
    "gumbel_sample": dict(gumbel=True, sample_moves=(1.0, 8)),
    "gumbel_cap": dict(gumbel=True, playout_cap=(4, 0.25)),
    "gumbel_leaves": dict(gumbel=True, leaves_per_step=2),
    "resign_gumbel": dict(RESIGN, gumbel=True),
    "resign_range": dict(resign=(1.5, 2, 10, 0.1)),
    "resign_shape": dict(resign=(0.9, 2, 10)),
    "value_signs_name": dict(value_signs="right"),
    "proofs_reference": dict(proofs=True),
    "proofs_gumbel": dict(PROOFS, gumbel=True),
    "proofs_forced": dict(PROOFS, **NOISE, forced_playouts=2.0),
    "proofs_type": dict(SOUND, proofs="yes"),
    "proof_play_without_proofs": dict(SOUND, proof_play=True),
    "proof_targets_without_play": dict(PROOFS, proof_targets=True),
    "selection_gumbel": dict(selection=FPU, gumbel=True),
    "selection_forced": dict(NOISE, selection=FPU, forced_playouts=2.0),
    "selection_key": dict(selection=dict(fpv=(0.2, 0.1))),
    "selection_range": dict(selection=dict(fpu=(5.0, 0.1))),
    "tree_gc_name": dict(tree_gc="always"),
    "value_target_name": dict(value_target=("mean", 0.5)),
    "value_target_range": dict(value_target=("td", 1.5)),
    "endgame_targets_range": dict(endgame_targets=13),
}
BATCH_ONLY = {                                          # selfplay_batch's own arguments
    "record_visits": dict(record_visits=True),
    "noise_forcing_visits": dict(NOISE, forced_playouts=2.0, record_visits=True),
    "gumbel_visits_value_target": dict(gumbel=True, record_visits=True, value_target=("td", 0.8)),
    "visits_value_target": dict(record_visits=True, value_target=("blend", 0.5)),
    "surprise_visits": dict(record_visits=True, surprise_weight=(0.5, 7)),
    "surprise_gumbel": dict(gumbel=True, surprise_weight=(0.5, 7)),
    "surprise_visits_value_target": dict(record_visits=True, surprise_weight=(0.5, 7), value_target=("td", 0.8)),
    "off_surprise": dict(surprise_weight=None),
    "node_cap": dict(tree_gc="demand", node_cap=500),
    "expand": dict(expand=True),
    "expand_alias": dict(expand=True, alias_final=True),
    "expand_visits": dict(expand=True, record_visits=True, target_temperature=0.5),
    "expand_value_target": dict(expand=True, value_target=("td", 0.8)),
    "expand_visits_value_target": dict(expand=True, record_visits=True, value_target=("td", 0.8)),
    "expand_endgame_cap": dict(expand=True, endgame_targets=8, playout_cap=(4, 0.25)),
    "expand_proof_targets": dict(PLAY, expand=True, proof_targets=True),
}
BATCH_REFUSALS = {
    "gumbel_expand": dict(gumbel=True, expand=True),
    "surprise_expand": dict(record_visits=True, surprise_weight=(0.5, 7), expand=True),
    "surprise_without_target": dict(surprise_weight=(0.5, 7)),
    "surprise_shape": dict(record_visits=True, surprise_weight=0.5),
    "surprise_frac": dict(record_visits=True, surprise_weight=(1.5, 7)),
    "value_target_alias": dict(expand=True, alias_final=True, value_target=("td", 0.8)),
    "endgame_targets_alias": dict(expand=True, alias_final=True, endgame_targets=8),
}
# the six options the matches share: a scalar, a (black, white) pair, an off pair
SEARCH_OPTIONS = {
    "none": {},
    "solve_leaves": dict(solve_leaves=6), "solve_leaves_pair": dict(solve_leaves=(6, 0)), "solve_leaves_off_pair": dict(solve_leaves=(0, 0)),
    "value_signs": SOUND, "value_signs_pair": dict(value_signs=("sound", "reference")),
    "value_signs_off_pair": dict(value_signs=("reference", "reference")),
    "proofs": PROOFS, "proofs_pair": dict(SOUND, proofs=(True, False)),
    "proofs_off_pair": dict(proofs=(False, False)),
    "proof_play": PLAY, "proof_play_pair": dict(PROOFS, proof_play=(True, False)), "proof_play_off_pair": dict(proof_play=(False, False)),
    "selection": dict(selection=FPU), "selection_pair": dict(selection=(FPU, None)), "selection_off_pair": dict(selection=(None, None)),
    "selection_off": dict(selection={}),
    "tree_gc": dict(tree_gc="demand"), "tree_gc_pair": dict(tree_gc=("demand", "off")), "tree_gc_off_pair": dict(tree_gc=("off", "off")),
    "all": dict(PLAY, solve_leaves=6, selection=FPU, tree_gc="every"),
    "all_off": dict(solve_leaves=0, value_signs="reference", proofs=False, proof_play=False, selection=None, tree_gc="off"),
    "proofs_reference": dict(proofs=True), "proof_play_without_proofs": dict(SOUND, proof_play=True), "tree_gc_name": dict(tree_gc="always"),
    "solve_leaves_range": dict(solve_leaves=11), "value_signs_name": dict(value_signs="right"), "selection_key": dict(selection=dict(fpv=1)),
}
MATCH_ONLY = {
    "openings": dict(openings=(4, 11)), "openings_all": dict(PLAY, openings=(4, 11), solve_leaves=6, selection=FPU, tree_gc="demand"),
    "leaves_per_step": dict(leaves_per_step=4, seed=5),
}
TRAINING_OPTIONS = dict(
    {k: v for k, v in ENGINE_OPTIONS.items() if not k.startswith(("value_target", "endgame", "gumbel_value", "proofs_all", "everything"))},
    value_target_td=dict(value_target=("td", 0.8)), endgame_targets=dict(endgame_targets=8),
    visits=dict(policy_target="visits"), visits_forcing=dict(NOISE, policy_target="visits", forced_playouts=2.0),
    gumbel_improved=dict(gumbel=True, policy_target="improved", value_target=("td", 0.8)),
    proofs_all_targets=dict(PLAY, proof_targets=True, value_target=("td", 0.8), endgame_targets=8, solve_leaves=6, policy_target="visits"),
    cap_resign_solved=dict(RESIGN, playout_cap=(4, 0.25), solve_leaves=6), eval_symmetry=dict(eval_symmetry=("random", 3)),
    openings=dict(match_openings=(4, 11), evaluation_openings=(4, 12), batched_evaluation=True),
    minimax=dict(evaluation_opponent=("minimax", 2), batched_evaluation=True))
TRAINING_DEVICE_ONLY = dict(surprise_visits=dict(policy_target="visits", surprise_weight=0.5),
                            surprise_gumbel=dict(gumbel=True, policy_target="improved", surprise_weight=0.5),
                            validation=dict(validation_share=0.25))
TRAINING_REFUSALS = dict(
    {k: v for k, v in REFUSALS.items() if k != "endgame_targets_range"},
    surprise_host=dict(policy_target="visits", surprise_weight=0.5), surprise_onehot=dict(replay="device", surprise_weight=0.5),
    validation_host=dict(validation_share=0.25), improved_without_gumbel=dict(policy_target="improved"),
    visits_alias=dict(policy_target="visits", alias_final_boards=True), value_target_alias=dict(value_target=("td", 0.8), alias_final_boards=True),
    endgame_alias=dict(endgame_targets=8, alias_final_boards=True), eval_symmetry_mean=dict(eval_symmetry="mean"),
    evaluation_openings_host=dict(evaluation_openings=(4, 12)), match_openings_odd=dict(match_openings=(4, 11), self_play_total_games=3),
    replay_name=dict(replay="disk"), device_dump=dict(replay="device", dump_examples=True), gumbel_distributed=dict(gumbel=True, distributed=True),
    policy_target_name=dict(policy_target="soft"))


def cases():
    """[(case id, target, keyword arguments)]"""
    out = []
    for target in ("selfplay_batch", "into_replay"):
        for group in (ENGINE_OPTIONS, REFUSALS) + ((BATCH_ONLY, BATCH_REFUSALS) if target == "selfplay_batch" else ()):
            out += [(f"{target}-{name}", target, kw) for name, kw in group.items()]
    out += [("into_replay-visits", "into_replay", dict(visits=True, policy_target="visits", target_temperature=0.5)),
            ("into_replay-surprise", "into_replay", dict(visits=True, policy_target="visits", surprise_weight=(0.5, 7))),
            ("into_replay-surprise_value_target", "into_replay", dict(PLAY, visits=True, policy_target="visits", surprise_weight=(0.5, 7),
                                                                        value_target=("td", 0.8), proof_targets=True, endgame_targets=8)),
            ("into_replay-gumbel_improved", "into_replay", dict(gumbel=True, policy_target="improved", surprise_weight=(0.5, 7))),
            ("into_replay-alias", "into_replay", dict(alias_final_boards=True))]
    engine_args = set(inspect.signature(REAL_ENGINE.__init__).parameters)
    for group in (ENGINE_OPTIONS, REFUSALS):
        out += [(f"engine-{name}", "engine", kw) for name, kw in group.items() if set(kw) <= engine_args]
    out += [("engine-records", "engine", dict(record_visits=True, record_values=True, record_surprise=True)),
            ("engine-surprise_without_target", "engine", dict(record_surprise=True)),
            ("engine-everything", "engine", dict(PLAY, **NOISE, **RESIGN, playout_cap=(4, 0.25), solve_leaves=6, sample_moves=(1.0, 8), tree_gc="every",
                                                 leaves_per_step=2, selection=dict(FPU, prior_first=True), record_visits=True, record_surprise=True)),
            ("engine-forcing_visits", "engine", dict(NOISE, forced_playouts=2, record_visits=True, record_values=True)),
            ("engine-gumbel_surprise", "engine", dict(gumbel=(8, 50.0, 1.0), record_surprise=True, record_values=True, value_signs="sound"))]
    for target in ("evaluate_against_random_batch", "evaluate_against_opponent_batch", "paired_match", "self_play_match"):
        out += [(f"{target}-{name}", target, kw) for name, kw in SEARCH_OPTIONS.items()]
        out += [(f"{target}-{name}", target, kw) for name, kw in MATCH_ONLY.items() if not (target == "paired_match" and "openings" in kw)]
    out += [("evaluate_against_random_batch-minimax", "evaluate_against_random_batch", dict(opponent=("minimax", 2), games=5)),
            ("self_play_match-odd", "self_play_match", dict(total_games=5)),
            ("self_play_match-openings_odd", "self_play_match", dict(total_games=5, openings=(4, 11))),
            ("paired_match-without_openings", "paired_match", dict(openings=None))]
    for name, kw in TRAINING_OPTIONS.items():
        out += [(f"training_host-{name}", "training", kw), (f"training_device-{name}", "training", dict(kw, replay="device"))]
    out += [(f"training_device-{name}", "training", dict(kw, replay="device")) for name, kw in TRAINING_DEVICE_ONLY.items()]
    out += [(f"training-{name}", "training", kw) for name, kw in TRAINING_REFUSALS.items()]
    assert len({c[0] for c in out}) == len(out)
    # _selfplay_into_replay is the loop's own: what reaches it has been through the loop's check, so gumbel=True arrives as its triple
    return [(case, target, dict(kw, gumbel=_lib.GUMBEL_DEFAULT) if target == "into_replay" and kw.get("gumbel") is True else kw)
            for case, target, kw in out]


def _call(target, kw, log):
    net = StubNet(log)
    if target == "engine":                                  # the real class over a recording library
        library = FakeLibrary(log)
        _lib.require_gpu = _lib.load = lambda *a: library
        net._h = ctypes.c_void_p(1)
        eng = REAL_ENGINE(net, 6, 8, 12, **kw)
        return eng.records(True, True, True, bool(eng.gumbel), eng.record_surprise, True)
    if target == "selfplay_batch":
        return training.selfplay_batch(net, 6, 8, 12, **kw)
    if target == "into_replay":
        kw = dict(kw)
        head = [kw.pop(k, d) for k, d in (("visits", False), ("leaves_per_step", 1), ("root_noise", None), ("sample_moves", None),
                                          ("alias_final_boards", False), ("policy_target", "onehot"), ("target_temperature", 1.0))]
        loop.training.rows_solved = 0
        return loop._selfplay_into_replay(FakeReplay(), net, 6, 8, 12, 1.0, 1.0, 0.9, 1234, 16, _lib.QMODE_F64, *head, **kw)
    if target == "evaluate_against_random_batch":
        kw = dict(kw)
        return loop.evaluate_against_random_batch(6, net, kw.pop("games", 4), 12, 1.0, **kw)
    if target == "evaluate_against_opponent_batch":
        return loop.evaluate_against_opponent_batch(6, net, 4, 12, 1.0, ("minimax", 1, "discs"), **kw)
    if target == "paired_match":
        kw = dict(kw)
        return loop.paired_match(6, net, net.copy(), 3, 12, 1.0, kw.pop("openings", (4, 11)), **kw)
    if target == "self_play_match":
        kw = dict(kw)
        return loop.self_play_match(6, net, net.copy(), kw.pop("total_games", 4), 12, 1.0, **kw)
    assert target == "training", target
    return loop.training(neural_network=net, **dict(LOOP_KW, **kw))


def run_case(target, kw):
    """one case -> its trace"""
    log = []
    trace = dict(calls=log)
    with stand_ins(log):
        try:
            returned = _call(target, kw, log)
            if target != "into_replay":                     # (its return value is the loop's own business)
                trace["returned"] = plain(returned)
        except (_Stop, _Reached):
            trace["stopped"] = "at the first fit"
        except Exception as e:                              # a refusal, or anything else the parent did: it is the record either way
            trace["raised"] = [type(e).__name__, str(e)]
        if "raised" not in trace:
            if target == "selfplay_batch":
                trace["attributes"] = {k: plain(getattr(training.selfplay_batch, k, "<unset>")) for k in BATCH_ATTRS}
            if target == "self_play_match":
                trace["attributes"] = {"stats": plain(loop.self_play_match.stats)}
            if target == "training":
                trace["attributes"] = {k: plain(getattr(loop.training, k, "<unset>")) for k in TRAINING_ATTRS}
    if "raised" in trace:
        del log[:]                                          # a refusal is its exception alone, wherever it came from
    return trace
