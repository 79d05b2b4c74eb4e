"""Held-out evaluation without a GPU: the validation split of a replay buffer (trainer.holdout_slots), the History keys, the refusals of
loop.training(validation_share=...), the new symbols in header, bindings and library, and the GPU tests' data: the float64 oracle alone
has no near-tie on it (tests/evaluate_ref.py)."""
import os
import re

import numpy as np
import pytest

import evaluate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_trainer_evaluate", "oz_trainer_evaluate_dataset", "oz_trainer_evaluate_replay"]


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"^#define OZ_EVAL_FIELDS 8\b", header, flags=re.M) and _lib.EVAL_FIELDS == 8


def _ring_slots(capacity, total):
    """slot -> running index of the example it holds (the ring rule: index k lives in slot k % capacity)"""
    held = min(total, capacity)
    idx = np.full(held, -1, np.int64)
    for k in range(total - held, total):
        idx[k % capacity] = k
    return idx


@pytest.mark.parametrize("capacity,total,new", [(100, 40, 16), (100, 100, 30), (100, 100, 100), (64, 150, 24), (64, 70, 24), (10, 1000, 10),
                                                (64, 150, 500)])
@pytest.mark.parametrize("share", [0.25, 0.5, 0.1])
def test_holdout_slots_are_the_newest_and_disjoint(capacity, total, new, share):
    """unwrapped, exactly full and wrapped buffers: the two sets are disjoint, their union is arange(held), and the validation slots hold
    the V = floor(share * min(new, held)) newest examples, oldest first"""
    from othellozero_amd.trainer import holdout_slots
    held = min(total, capacity)
    train, val = holdout_slots(held, capacity, total, new, share)
    V = int(np.floor(share * min(new, held)))
    assert train.dtype == val.dtype == np.int32 and len(val) == V and len(train) == held - V
    assert not set(train) & set(val) and np.array_equal(np.sort(np.concatenate([train, val])), np.arange(held))
    assert np.array_equal(train, np.sort(train))
    age = _ring_slots(capacity, total)
    assert np.array_equal(age[val], np.arange(total - V, total))
    assert V == 0 or age[train].max() < total - V


def test_holdout_slots_small_appends_and_bad_shares():
    from othellozero_amd.trainer import holdout_slots
    train, val = holdout_slots(50, 100, 50, 3, 0.25)                # floor(0.75) = 0: nothing is held out
    assert len(val) == 0 and val.dtype == np.int32 and np.array_equal(train, np.arange(50))
    train, val = holdout_slots(0, 100, 0, 0, 0.5)
    assert len(val) == 0 and len(train) == 0
    for share in (0, 0.0, -0.1, 0.51, 1, float("nan")):
        with pytest.raises(ValueError, match="share"):
            holdout_slots(50, 100, 50, 16, share)


def test_history_without_validation_has_todays_keys():
    from othellozero_amd import trainer as T
    h = T.History()
    assert list(h.history) == ["loss", "pi-reshaped_loss", "v_loss"]
    T._record_epoch(h, 0, 1, (3.0, 2.0, 1.0), None)
    assert h.history == {"loss": [3.0], "pi-reshaped_loss": [2.0], "v_loss": [1.0]} and h.epoch == [0]
    val = dict(zip(T.VAL_KEYS, (0.5, 0.25, 0.25, 0.75, 1.0)), examples=4, decided=3)
    T._record_epoch(h, 1, 2, (3.0, 2.0, 1.0), None, val=val)
    assert set(h.history) == {"loss", "pi-reshaped_loss", "v_loss", "val_loss", "val_pi-reshaped_loss", "val_v_loss", "val_policy_top1",
                              "val_value_sign"}
    assert h.history["val_policy_top1"] == [0.75] and h.history["val_loss"] == [0.5]


def test_verbose_line_names_the_validation_numbers(capsys):
    from othellozero_amd import trainer as T
    h = T.History()
    T._record_epoch(h, 0, 1, (3.0, 2.0, 1.0), 1, val=dict(zip(T.VAL_KEYS, (0.5, 0.25, 0.25, 0.75, 1.0))))
    line = capsys.readouterr().out
    assert "val_loss: 0.5000" in line and "val_policy_top1: 0.7500" in line and "val_value_sign: 1.0000" in line


def _loop_kw():
    return dict(board_size=6, num_iterations=1, num_episodes=2, num_simulations=2, degree_exploration=1, temperature=1, neural_network=None,
                e_greedy=0.9, evaluation_interval=2, evaluation_iterations=2, temperature_threshold=0, self_play_training=False,
                self_play_interval=1, self_play_total_games=2, self_play_threshold=1, checkpoint_filepath="unused.npz", training_buffer_size=64)


def test_loop_refusals_need_no_gpu():
    from othellozero_amd import loop
    with pytest.raises(ValueError, match="validation_share needs replay='device'"):
        loop.training(validation_share=0.25, **_loop_kw())
    with pytest.raises(ValueError, match="validation_share needs replay='device'"):
        loop.training(validation_share=0.25, replay="host", **_loop_kw())
    with pytest.raises(ValueError, match="validation_share is not offered with distributed=True"):
        loop.training(validation_share=0.25, replay="device", distributed=True, **_loop_kw())
    for bad in (0, 0.0, -0.25, 0.6, 1, float("nan"), "0.25", True):
        with pytest.raises(ValueError, match="validation_share must be"):
            loop.training(validation_share=bad, replay="device", **_loop_kw())


def test_wrapper_refuses_mixed_validation_arguments():
    """(the checks precede every use of the device)"""
    from othellozero_amd.NNet import NNetWrapper
    net = object.__new__(NNetWrapper)
    with pytest.raises(ValueError, match="validation_slots= names slots of a ReplayBuffer"):
        NNetWrapper.train(net, [("board", "pi", 1.0)], validation_slots=np.arange(3))


@pytest.mark.parametrize("n,C", [(6, 128), (8, 128), (8, 256), (6, 256)])
def test_the_gpu_tests_data_has_no_near_tie_in_the_oracle(n, C):
    """the float64 oracle alone: no example with its top two p within 4e-5 or a decided example with |v| < 2e-5 (the cap of the GPU test is 2
    of 70), top-two gaps far above the 1e-6 the metrics test asserts on the device's p, and targets that exercise the tie rule: rows with
    several equal maxima where the lowest index makes the network's move a hit, and rows where it makes it a miss"""
    own, opp, pi, z = R.examples(n, C)
    p, v = R.oracle_outputs(n, C)
    assert len(z) == 70 and (z == 0).sum() >= 5 and (z != 0).sum() >= 40
    assert R.top2_gap(p).min() > 1e-4 and np.abs(v).min() > 1e-3
    m = R.metrics(p, v, pi, z, n, "flat")
    tied = np.array([np.sort(r)[-1] == np.sort(r)[-2] for r in pi])
    best_is_a_max = pi[np.arange(70), p.argmax(axis=1)] == pi.max(axis=1)
    assert (m["top1"] & tied).sum() >= 2 and (~m["top1"] & tied & best_is_a_max).sum() >= 5
    assert 0.2 < R.summary(m)["policy_top1"] < 0.8 and 0.2 < R.summary(m)["value_sign"] < 0.8
