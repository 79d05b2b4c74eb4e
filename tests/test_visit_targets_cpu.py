"""CPU-only checks of the visit-count policy targets: the C ABI's new symbols and layout, the loop's refusals, and the pooling of
record || visit-count rows over gloo with world_size 2 (ragged and empty ranks)."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selfplay_config_layout_is_unchanged_and_carries_record_visits():
    """record_visits takes the place of the trailing reserved word: size and every offset stay, so C callers that zero the struct get
    today's engine"""
    from othellozero_amd import _lib
    cfg = _lib.SelfplayConfig
    assert C.sizeof(cfg) == 96
    offsets = {name: getattr(cfg, name).offset for name, _ in cfg._fields_}
    assert offsets == {"n": 0, "num_games": 4, "sims": 8, "q_mode": 12, "c": 16, "temperature": 24, "e_greedy": 32, "seed": 40,
                       "first_game_id": 48, "game_id_stride": 56, "refill": 64, "node_cap": 68, "reserved0": 72, "record_cap": 76,
                       "dedup": 80, "batch_cap": 84, "eval_cache": 88, "record_visits": 92}
    assert cfg().record_visits == 0


def test_visit_entry_points_are_declared_and_exported():
    from othellozero_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "othellozero_amd.h")).read()
    for name in ("oz_selfplay_visits", "oz_selfplay_visits_device", "oz_selfplay_gather_visits", "oz_examples_expand_visits",
                 "oz_trainer_set_policy_loss"):
        assert re.search(rf"^int {name}\(", hdr, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "int32_t record_visits;" in hdr and "#define OZ_POLICY_LOSS_FLAT 1" in hdr
    assert lib.oz_version() >= 201


def test_expand_visits_refuses_a_non_positive_temperature_before_any_device_work():
    from othellozero_amd import _lib
    lib = _lib.load()
    rec = np.zeros(1, _lib.RECORD_DTYPE)
    cnt = np.zeros((1, 64), np.int32)
    boards, pi, z = np.zeros((8, 6, 6, 2), np.uint8), np.zeros((8, 36)), np.zeros(8, np.int8)
    for T in (0.0, -0.5):
        rc = lib.oz_examples_expand_visits(rec.ctypes.data_as(C.c_void_p), _lib.p_i32(cnt), 1, 6, 0, T, _lib.p_u8(boards),
                                           _lib.p_f64(pi), _lib.p_i8(z))
        assert rc == _lib.OZ_ERR_ARG and b"temperature" in lib.oz_last_error()


class _Net:
    def __init__(self, policy_loss):
        self.policy_loss = policy_loss


@pytest.mark.parametrize("kw,match", [(dict(policy_target="visits", alias_final_boards=True, net="flat"), "alias_final_boards=False"),
                                      (dict(policy_target="visits", alias_final_boards=False, net="rows"), "policy_loss='flat'"),
                                      (dict(policy_target="pi", alias_final_boards=False, net="flat"), "policy_target")])
def test_loop_refuses_visit_targets_it_cannot_train_on(kw, match):
    """both refusals happen before any self-play and name the fix"""
    from othellozero_amd.loop import training
    net = _Net(kw.pop("net"))
    with pytest.raises(ValueError, match=re.escape(match)):
        training(board_size=6, num_iterations=1, num_episodes=2, num_simulations=4, degree_exploration=1, temperature=1,
                 neural_network=net, e_greedy=0.9, evaluation_interval=1, evaluation_iterations=1, temperature_threshold=0,
                 self_play_training=False, self_play_interval=1, self_play_total_games=2, self_play_threshold=1,
                 checkpoint_filepath="unused.h5", training_buffer_size=16, **kw)


GLOO_VISITS_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from othellozero_amd._lib import RECORD_DTYPE
from othellozero_amd.distributed import RECORD_BYTES, VISITS_BYTES, gather_records, records_to_tensor, split_record_rows
rank, world = int(os.environ["RANK"]), 2
dist.init_process_group("gloo", rank=rank, world_size=world)
def rows_of(r, count):
    rec = np.zeros(count, dtype=RECORD_DTYPE)
    rec["game_id"] = 2 * (np.arange(count)[::-1] // 4) + r          # the ranks' games interleave, each rank's rows out of order
    rec["ply"] = np.arange(count) % 4
    rec["black"] = 1000 * r + np.arange(count)
    cnt = (np.arange(count * 64, dtype=np.int64).reshape(count, 64) * (r + 3) + 70000).astype(np.int32)   # values past uint16
    return rec, cnt
def pool(count):
    rec, cnt = rows_of(rank, count)
    local = torch.cat([records_to_tensor(rec), torch.from_numpy(cnt.view(np.uint8).reshape(count, VISITS_BYTES).copy())], dim=1)
    assert local.shape == (count, RECORD_BYTES + VISITS_BYTES) == (count, 304)
    return split_record_rows(gather_records(local))
for counts in ((13, 40), (0, 9), (0, 0)):
    got_rec, got_cnt = pool(counts[rank])
    parts = [rows_of(r, counts[r]) for r in range(world)]
    want_rec = np.concatenate([p[0] for p in parts]); want_cnt = np.concatenate([p[1] for p in parts]).reshape(-1, 64)
    order = np.lexsort((want_rec["ply"], want_rec["game_id"]))
    assert got_rec.tobytes() == want_rec[order].tobytes() and np.array_equal(got_cnt, want_cnt[order]), (rank, counts)
    assert got_cnt.dtype == np.int32 and got_cnt.shape == (sum(counts), 64)
dist.barrier()
print("RANK_OK", rank)
"""


def test_gloo_world_size_2_pools_records_with_visit_counts(tmp_path):
    """[R, 48 + 256] rows (record || int32 counts) through distributed.gather_records over gloo: ragged ranks, an empty rank, every
    rank empty -- split after the sort, every record keeps its own counts row"""
    script = tmp_path / "gloo_visits_worker.py"
    script.write_text(GLOO_VISITS_WORKER)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=180)[0] for p in procs]
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"RANK_OK {rank}" in out, out
