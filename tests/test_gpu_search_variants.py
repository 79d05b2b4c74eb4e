"""Every instantiation of the search's kernel families, bit for bit against a run recorded before the families were folded (pytest -m gpu).

The tree kernels (k_select, k_backup_select, k_expand_backup and their k_wide_* counterparts), the free-running k_advance / k_backup_advance
and the move kernel k_sp_move are one template per family, instantiated per option combination; the host resolves the combination from the
object's state.  SETTINGS lists small engines whose combinations reach every instantiation; tests/golden/search_variants.npz holds what each
of them produced on the commit named in the file's `parent` entry: the record array as it is, SHA-256 digests of the per-record arrays
(visit rows, root values, improved policies, surprises), oz_selfplay_stats and the options' own counters.  The test asserts every entry is
identical.  Stub network, q_mode F64, 6x6, 8 games, 12 simulations per move.

    python tests/test_gpu_search_variants.py PARENT_COMMIT     # on an MI355X, from a checkout of that commit with this module copied in

writes the file, and refuses where a setting ends no game or an option's counter stays 0 (the test would pass vacuously)."""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_variants.npz")
N, G, SIMS, SALT, SEED, FIRST, EG = 6, 8, 12, 21, 77, 300, 0.8          # the engine setting of tests/test_gpu_proofs.py
NOISE = dict(root_noise=(0.5, 0.25))
SEL = dict(selection=dict(fpu=(0.2, 0.1), cpuct_growth=(20.0, 2.0), prior_first=True))
SIGNS = {"ref": dict(value_signs="reference"), "sound": dict(value_signs="sound"), "proven": dict(value_signs="sound", proofs=True)}
VISITS = dict(record_visits=True)
SURPRISE = dict(record_visits=True, record_surprise=True)
RESIGN = dict(resign=(0.3, 2, 8, 0.0))
PLAY = dict(proof_play=True, record_visits=True, record_values=True)
GUMBEL = dict(gumbel=(4, 50.0, 1.0))
# (signs, tree options) -> the move options that ride along at K = 1: together the thirteen self-play moves (the plain move: every K = 4 run)
MOVES = {
    ("ref", "plain"): dict(sample_moves=(1.0, 6)),                                  # move sampling
    ("ref", "noise"): dict(forced_playouts=2.0, **VISITS),                          # forced playouts
    ("ref", "sel"): dict(playout_cap=(4, 0.5)),                                     # playout cap
    ("ref", "noise_sel"): dict(record_values=True),                                 # recorded values
    ("sound", "plain"): SURPRISE,                                                   # ... with recorded surprise
    ("sound", "noise"): RESIGN,                                                     # resignation
    ("sound", "sel"): dict(**RESIGN, **SURPRISE),                                   # ... with recorded surprise
    ("sound", "noise_sel"): dict(playout_cap=(4, 0.5), sample_moves=(1.0, 6)),
    ("proven", "plain"): PLAY,                                                      # the four proof-play moves
    ("proven", "noise"): dict(**PLAY, record_surprise=True),
    ("proven", "sel"): dict(**PLAY, **RESIGN),
    ("proven", "noise_sel"): dict(**PLAY, **RESIGN, record_surprise=True),
}
TREE = {"plain": {}, "noise": NOISE, "sel": SEL, "noise_sel": dict(**NOISE, **SEL)}


def _settings():
    out = []
    for K in (1, 4):
        for signs in SIGNS:
            for tree in TREE:
                kw = dict(SIGNS[signs], **TREE[tree], leaves_per_step=K)
                if K == 1:
                    kw.update(MOVES[(signs, tree)])
                out.append((f"run_k{K}_{signs}_{tree}", "run", kw))
    out.append(("run_gumbel_ref", "run", dict(GUMBEL)))
    out.append(("run_gumbel_sound", "run", dict(GUMBEL, value_signs="sound", record_surprise=True)))
    for signs in ("ref", "sound"):
        for name, kw in (("plain", {}), ("values", dict(record_values=True)), ("noise", NOISE), ("surprise", SURPRISE)):
            out.append((f"steps_{signs}_{name}", "steps", dict(SIGNS[signs], **kw)))
    out.append(("arena_proof_play_black", "arena", {}))
    return out


SETTINGS = _settings()
# the counters that must not be 0 in the recorded run of a setting with the option: option key -> (entry of the result, index or None)
COUNTERS = {"proofs": ("proof_stats", 3), "proof_play": ("proof_play_stats", 1), "resign": ("resign_stats", 0), "forced_playouts": ("forced_stats", 0),
            "playout_cap": ("playout_stats", 1), "gumbel": ("gumbel_moves", 0), "sample_moves": ("sampled_moves", 0)}


def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _run(oz, kind, kw):
    """one setting to the end of its games -> {entry: array}"""
    from othellozero_amd.NNet import StubNetWrapper
    if kind == "arena":
        from othellozero_amd.agents import arena_batch
        na, nb = StubNetWrapper((N, N), 41, 0, max_batch=G), StubNetWrapper((N, N), 42, 0, max_batch=G)
        r = arena_batch(na, nb, N, G, SIMS, 1.0, seed=7, first_game_id=900, q_mode=oz.QMODE_F64, value_signs="sound", proofs=(True, False),
                        proof_play=(True, False))
        out = {k: np.asarray(r[k]) for k in ("winner", "points", "n_moves", "actions", "players", "final_black", "final_white")}
        out["stats"] = np.concatenate([np.asarray(r["stats_black"], np.int64), np.asarray(r["stats_white"], np.int64)])
        out["games_ended"] = np.array([int(np.count_nonzero(out["n_moves"]))], np.int64)
        return out
    from othellozero_amd.training import SelfPlayEngine
    K = kw.get("leaves_per_step", 1)
    eng = SelfPlayEngine(StubNetWrapper((N, N), SALT, 0, max_batch=G * K), N, G, SIMS, 1.0, 1.0, EG, seed=SEED, first_game_id=FIRST, **kw)
    for _ in range(200):
        if kind == "run":
            eng.run(4)
        else:
            eng.run_steps(32)
        if eng.stats()["live_games"] == 0:
            break
    st = eng.stats()
    assert st["live_games"] == 0 and st["overflow"] == 0, st
    with_visits, with_values = bool(kw.get("record_visits")), bool(kw.get("record_values") or kw.get("resign"))
    with_policies, with_surprise = "gumbel" in kw, bool(kw.get("record_surprise"))
    got = eng.records(with_visits=with_visits, with_values=with_values, with_policies=with_policies, with_surprise=with_surprise)
    got = list(got) if isinstance(got, tuple) else [got]
    out = {"records": got.pop(0)}
    for flag, name in ((with_visits, "visits"), (with_values, "values"), (with_policies, "policies"), (with_surprise, "surprises")):
        if flag:
            out[name + "_sha256"] = _digest(got.pop(0))
    out["proof_codes_sha256"] = _digest(out["records"]["pad"][:, 2])
    out["stats"] = np.array([int(st[k]) for k in sorted(st)], np.int64)
    out["games_ended"] = np.array([st["games_completed"]], np.int64)
    out["proof_stats"] = np.array(list(eng.proof_stats().values()), np.int64)
    out["proof_play_stats"] = np.array(list(eng.proof_play_stats().values()), np.int64)
    rs, fp, pc = eng.resign_stats(), eng.forced_playout_stats(), eng.playout_stats()
    out["resign_stats"] = np.array([rs[k] for k in ("games_adjudicated", "adjudicated_plies_sum", "games_exempt", "exempt_triggered", "exempt_wrong",
                                                    "exempt_trigger_ply_sum")], np.int64)
    out["forced_stats"] = np.array([fp[k] for k in ("moves_pruned", "visits_raw", "visits_kept")], np.int64)
    out["playout_stats"] = np.array([pc["full_moves"], pc["fast_moves"]], np.int64)
    out["gumbel_moves"] = np.array([eng.gumbel_stats()["moves"]], np.int64)
    out["sampled_moves"] = np.array([int(np.count_nonzero(out["records"]["greedy"] == 2))], np.int64)
    return out


@pytest.fixture(scope="module")
def oz():
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_file_holds_every_setting_and_names_its_commit(golden):
    assert len(str(golden["parent"])) == 40
    names = {k.split("/")[0] for k in golden.files if "/" in k}
    assert names == {name for name, _, _ in SETTINGS}
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "mcts.npz"))


@pytest.mark.parametrize("name,kind,kw", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_variant_is_bit_identical_to_the_recorded_run(oz, golden, name, kind, kw):
    got = _run(oz, kind, kw)
    want = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(name + "/")}
    assert set(got) == set(want) and want["games_ended"][0] >= 1, (name, sorted(got), sorted(want))
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (name, k)


def _generate(parent):
    import othellozero_amd  # noqa: F401
    from othellozero_amd import _lib
    _lib.require_gpu()
    assert len(parent) == 40, "the full hash of the commit the run is recorded on"
    out, vacuous = {"parent": np.array(parent)}, []
    for name, kind, kw in SETTINGS:
        got = _run(_lib, kind, kw)
        if got["games_ended"][0] < 1:
            vacuous.append((name, "no game ended"))
        for opt, (entry, i) in COUNTERS.items():
            if kw.get(opt) and got[entry][i] == 0:
                vacuous.append((name, opt, entry, got[entry].tolist()))
        print(name, "records" in got and got["records"].size, {k: got[k].tolist() for k in got if k.endswith("stats") or k.endswith("moves")}, flush=True)
        out.update({f"{name}/{k}": v for k, v in got.items()})
    assert not vacuous, vacuous
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes;", len(SETTINGS), "settings")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _generate(sys.argv[1])
