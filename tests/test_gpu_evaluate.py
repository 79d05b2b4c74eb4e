"""Held-out evaluation in inference mode on the device (oz_trainer_evaluate / _dataset / _replay, Trainer.evaluate*, fit(validation=...),
fit_replay(validation_slots=...), NNetWrapper.evaluate, loop.training(validation_share=...)).

Data and references: tests/evaluate_ref.py (70 examples = two batches of 32 and a short one of 6, targets with equal maxima, some z == 0,
weights whose moving statistics fit the examples; the float64 oracle's outputs are computed once per (board, filters) and shared).
Tolerances: outputs and losses 2e-5, the tolerance tests/test_gpu_train.py holds the trainer's outputs and training losses to; the two
counts are integers and compared exactly against the device's own p and v.
"""
import random

import numpy as np
import pytest

import evaluate_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5
CASES = [pytest.param(6, 128, "f32", "rows", id="6x6-128-f32-rows"), pytest.param(8, 128, "f32", "flat", id="8x8-128-f32-flat"),
         pytest.param(8, 256, "f16x2", "flat", id="8x8-256-f16x2-flat"), pytest.param(6, 256, "bf16x3", "rows", id="6x6-256-bf16x3-rows")]


@pytest.fixture(scope="module")
def oz():
    from othellozero_amd import _lib
    _lib.require_gpu()
    return _lib


def _trainer(n, C, precision="f32", policy_loss="rows", max_batch=32, dropout=0.3, optimizer=None, momentum=0.99, weights=None):
    from othellozero_amd.trainer import Trainer
    t = Trainer(n, C, 2, max_batch=max_batch, lr=1e-3, clipvalue=0.5, dropout=dropout, bn_momentum=momentum, seed=21, precision=precision,
                policy_loss=policy_loss, optimizer=optimizer)
    t.set_weights(R.calibrated_weights(n, C) if weights is None else weights)
    return t


def _close(got, want):
    return all(np.isclose(got[k], want[k], atol=TOL, rtol=TOL) for k in ("loss", "pi-reshaped_loss", "v_loss"))


# ------------------------------------------------------------------ 1. the forward is the inference network
@pytest.mark.parametrize("n,C,precision,policy_loss", CASES)
def test_forward_is_the_inference_network(oz, n, C, precision, policy_loss):
    """after an evaluation, outputs() of its last batch (the short one of 6, then a batch of one) are the float64 inference network's and
    NNetWrapper.predict_batch's within 2e-5, and differ from the training-mode outputs of forward_backward on the same batch by more"""
    from othellozero_amd.NNet import NNetWrapper
    own, opp, pi, z = R.examples(n, C)
    po, vo = R.oracle_outputs(n, C)
    t = _trainer(n, C, precision, policy_loss)
    net = NNetWrapper((n, n), num_channels_1=C, max_batch=8, weights=t.get_weights())
    for first, B in ((64, 6), (0, 1)):                              # 70 examples at batch 32: the last batch holds 64 .. 69
        N = first + B
        res = t.evaluate(own[:N], opp[:N], pi[:N], z[:N], batch_size=32)
        assert res["examples"] == N
        p, v = t.outputs(B)
        ep, ev = np.abs(p - po[first:N]).max(), np.abs(v - vo[first:N]).max()
        pn, vn = net.predict_batch(own[first:N], opp[first:N])
        en, evn = np.abs(p - pn.reshape(B, n * n)).max(), np.abs(v - vn).max()
        print(f"B={B}: vs float64 oracle p {ep:.2e} v {ev:.2e} / vs predict_batch p {en:.2e} v {evn:.2e}")
        assert ep <= TOL and ev <= TOL and en <= TOL and evn <= TOL
    t.forward_backward(own[64:], opp[64:], pi[64:], z[64:])           # training mode: batch statistics of six boards, dropout 0.3
    pt, vt = t.outputs(6)
    dp, dv = np.abs(pt - po[64:]).max(), np.abs(vt - vo[64:]).max()
    print(f"training mode vs the inference oracle: p {dp:.2e} v {dv:.2e}")
    assert dp > TOL and dv > TOL


# ------------------------------------------------------------------ 2. the metrics, from the device's own outputs
@pytest.mark.parametrize("n,C,precision,policy_loss", CASES)
def test_metrics_follow_from_the_devices_outputs(oz, n, C, precision, policy_loss):
    """one batch of N = 32, 5 and 1: the float64 restatement of the losses on the p and v the device reports agrees within 2e-5 and the
    counts agree exactly (no example has two p maxima within 1e-6: asserted)"""
    t = _trainer(n, C, precision, policy_loss)
    for N in (32, 5, 1):
        own, opp, pi, z = (a[70 - N:] for a in R.examples(n, C))
        got = t.evaluate(own, opp, pi, z, batch_size=32)
        p, v = t.outputs(N)
        assert R.top2_gap(p).min() > 1e-6
        want = R.summary(R.metrics(p, v, pi, z, n, policy_loss))
        print(N, got, want)
        assert _close(got, want)
        assert got["examples"] == want["examples"] == N and got["decided"] == want["decided"]
        assert round(got["policy_top1"] * N) == round(want["policy_top1"] * N) and got["policy_top1"] == want["policy_top1"]
        assert got["value_sign"] == want["value_sign"]
        assert got["loss"] == got["pi-reshaped_loss"] + got["v_loss"]


def test_metrics_with_no_decided_example(oz):
    """every z == 0: value_sign is 0 and decided 0"""
    n, C = 6, 128
    own, opp, pi, z = (a[:5] for a in R.examples(n, C))
    got = _trainer(n, C).evaluate(own, opp, pi, np.zeros(5, np.float32))
    assert got["decided"] == 0 and got["value_sign"] == 0.0 and got["examples"] == 5


# ------------------------------------------------------------------ 3. against the float64 oracle end to end
@pytest.mark.parametrize("n,C,precision,policy_loss", CASES)
def test_against_the_float64_oracle(oz, n, C, precision, policy_loss):
    """70 examples at batch 32: losses within 2e-5; the counts may differ from the oracle's only by examples whose oracle top two p lie
    within 4e-5 (twice the output tolerance) or whose |v| < 2e-5 -- at most 2 of 70 such examples (the data has none: test_evaluate_host.py)"""
    own, opp, pi, z = R.examples(n, C)
    po, vo = R.oracle_outputs(n, C)
    m = R.metrics(po, vo, pi, z, n, policy_loss)
    want = R.summary(m)
    amb_p, amb_v = R.top2_gap(po) < 2 * TOL, (np.abs(vo) < TOL) & m["decided"]
    ambiguous = int((amb_p | amb_v).sum())
    assert ambiguous <= 2
    got = _trainer(n, C, precision, policy_loss).evaluate(own, opp, pi, z, batch_size=32)
    print(got, want, "ambiguous examples:", ambiguous)
    assert _close(got, want)
    assert got["examples"] == 70 and got["decided"] == want["decided"]
    assert abs(round(got["policy_top1"] * 70) - round(want["policy_top1"] * 70)) <= int(amb_p.sum())
    assert abs(round(got["value_sign"] * got["decided"]) - round(want["value_sign"] * want["decided"])) <= int(amb_v.sum())


# ------------------------------------------------------------------ 4. an evaluation leaves the trainer alone
def _state(t):
    from othellozero_amd.trainer import TRAINABLE
    return dict(weights=t.get_weights(), adam=[t.adam_state(i) for i in TRAINABLE], step=t.step, info=t.step_info())


def _same_state(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a["weights"], b["weights"])) and a["step"] == b["step"] and a["info"] == b["info"]
            and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a["adam"], b["adam"])))


@pytest.mark.parametrize("n,C,precision,optimizer", [
    pytest.param(6, 128, "f32", None, id="f32"),
    pytest.param(6, 128, "f32", dict(global_clipnorm=1.0, average_decay=0.9), id="f32-options"),
    pytest.param(8, 256, "f16x2", dict(global_clipnorm=1.0, average_decay=0.9), id="f16x2-options"),
    pytest.param(6, 256, "bf16x3", dict(global_clipnorm=1.0, average_decay=0.9), id="bf16x3-options")])
def test_an_evaluation_leaves_the_trainer_alone(oz, n, C, precision, optimizer):
    """three steps and a resident epoch with an evaluate (between forward_backward and apply), an evaluate_dataset and an evaluate_replay
    after every step, against the same without: weights, moving statistics, Adam moments, step, step_info, the weight average and the
    epoch's losses are bit-identical; a repeated evaluation returns identical doubles"""
    from othellozero_amd.replay import ReplayBuffer
    own, opp, pi, z = R.examples(n, C)
    buf = ReplayBuffer(n, 70)
    buf.append_examples(own, opp, pi, z)
    runs = []
    for with_eval in (False, True):
        t = _trainer(n, C, precision, "flat", optimizer=optimizer, momentum=0.9)
        t.set_dataset(own, opp, pi, z)
        evals = []
        for k in range(3):
            sl = slice(8 * k, 8 * k + (32, 17, 5)[k])
            t.forward_backward(own[sl], opp[sl], pi[sl], z[sl])
            if with_eval:
                evals.append(t.evaluate(own[40:], opp[40:], pi[40:], z[40:], batch_size=7))
            t.apply()
            if with_eval:
                evals.append(t.evaluate_dataset(np.arange(69, -1, -1), 32))
                evals.append(t.evaluate_replay(buf, np.arange(3, 50), 16))
                assert t.evaluate_replay(buf, np.arange(3, 50), 16) == evals[-1]
        state = _state(t)
        if optimizer:
            state["weights"] += t.get_weights(average=True)
        losses = t.fit_epoch(np.random.RandomState(2).permutation(70), 32)
        runs.append((state, losses, _state(t)))
        if with_eval:
            assert all(np.isfinite(list(e.values())).all() for e in evals) and len(evals) == 9
    (s0, l0, e0), (s1, l1, e1) = runs
    assert _same_state(s0, s1) and np.array_equal(l0, l1) and _same_state(e0, e1) and s0["step"] == 3 and e0["step"] == 6


# ------------------------------------------------------------------ 5. the three views agree
@pytest.mark.parametrize("n,C,precision,policy_loss", [CASES[0], CASES[3]])
def test_views_agree(oz, n, C, precision, policy_loss):
    """the same 70 examples as host arrays, as the resident data set with an order and as a ReplayBuffer's slots: identical doubles at one
    batch size; a permuted order: the same counts exactly, the means within 1e-6 relative.  The host-array call leaves the resident data set"""
    from othellozero_amd.replay import ReplayBuffer
    own, opp, pi, z = R.examples(n, C)
    t = _trainer(n, C, precision, policy_loss)
    half = np.arange(35)
    t.set_dataset(own[::-1], opp[::-1], pi[::-1], z[::-1])                # the resident data set holds the examples REVERSED
    before = t.evaluate_dataset(half, 32)
    host = t.evaluate(own, opp, pi, z, batch_size=32)
    assert t.evaluate_dataset(half, 32) == before                       # evaluate() on host arrays did not replace it
    resident = t.evaluate_dataset(np.arange(69, -1, -1), 32)
    buf = ReplayBuffer(n, 100)
    buf.append_examples(own, opp, pi, z)
    slots = t.evaluate_replay(buf, np.arange(70), 32)
    assert host == resident == slots and host["examples"] == 70
    perm = t.evaluate_replay(buf, np.random.RandomState(4).permutation(70), 32)
    for k in ("examples", "decided", "policy_top1", "value_sign"):
        assert perm[k] == host[k], k
    for k in ("loss", "pi-reshaped_loss", "v_loss"):
        assert abs(perm[k] - host[k]) <= 1e-6 * abs(host[k]), k


# ------------------------------------------------------------------ 6. errors
def test_refusals(oz):
    """a bad batch, an index out of range, another board size and an empty resident data set: OZ_ERR_ARG, the message names the function"""
    from othellozero_amd.replay import ReplayBuffer
    n, C = 6, 128
    own, opp, pi, z = R.examples(n, C)
    t = _trainer(n, C)

    def refused(call, name):
        with pytest.raises(oz.OzError) as e:
            call()
        assert e.value.code == oz.OZ_ERR_ARG and name in str(e.value), str(e.value)
    refused(lambda: t.evaluate_dataset(np.arange(4), 8), "oz_trainer_evaluate_dataset")              # no resident data set yet
    t.set_dataset(own, opp, pi, z)
    buf, other = ReplayBuffer(n, 80), ReplayBuffer(8, 80)
    buf.append_examples(own, opp, pi, z)
    other.append_examples(*R.examples(8, 128))
    for bad in (0, 33):
        refused(lambda: t.evaluate(own, opp, pi, z, batch_size=bad), "oz_trainer_evaluate:")
        refused(lambda: t.evaluate_dataset(np.arange(4), bad), "oz_trainer_evaluate_dataset")
        refused(lambda: t.evaluate_replay(buf, np.arange(4), bad), "oz_trainer_evaluate_replay")
    for idx in ([0, 70], [-1]):
        refused(lambda: t.evaluate_dataset(np.array(idx), 8), "oz_trainer_evaluate_dataset")
        refused(lambda: t.evaluate_replay(buf, np.array(idx), 8), "oz_trainer_evaluate_replay")
    refused(lambda: t.evaluate_replay(other, np.arange(4), 8), "oz_trainer_evaluate_replay")
    refused(lambda: t.evaluate_dataset(np.zeros(0, np.int32), 8), "oz_trainer_evaluate_dataset")
    assert t.evaluate_dataset(np.arange(70), 32)["examples"] == 70                                   # and the trainer is usable


def test_f16x2_range_error_is_reported_once_and_the_trainer_recovers(oz):
    """moving statistics that do not fit the data -- tiny variances and a mean 3000 below conv1's outputs: activations near 1e5, beyond the
    fp16 range -- make ONE f16x2 evaluation fail with OZ_ERR_STATE; the flag is cleared when reported: with good weights back, the same
    trainer evaluates and takes a step like a fresh one, bit for bit"""
    n, C = 6, 256
    own, opp, pi, z = (a[:16] for a in R.examples(n, C))
    w = R.calibrated_weights(n, C)
    good = _trainer(n, C, "f16x2", max_batch=16, dropout=0.0)
    want_eval = good.evaluate(own, opp, pi, z)
    want_step = good.forward_backward(own, opp, pi, z)
    bad = [a.copy() for a in w]
    bad[4] = bad[4] - 3000.0                                           # moving mean of conv1's BN
    bad[5] = np.full_like(bad[5], 1e-12)                               # its moving variance: rstd = 1 / sqrt(1e-3) = 31.6
    t = _trainer(n, C, "f16x2", max_batch=16, dropout=0.0, weights=bad)
    with pytest.raises(oz.OzError) as e:
        t.evaluate(own, opp, pi, z)
    assert e.value.code == oz.OZ_ERR_STATE and "fp16 range" in str(e.value)
    t.set_weights(w)
    assert t.evaluate(own, opp, pi, z) == want_eval                    # reported once
    assert t.forward_backward(own, opp, pi, z) == want_step


# ------------------------------------------------------------------ 7. the fits, the wrapper, the loop
def test_fit_with_validation(oz):
    """fit(validation=...): val_* lists of one entry per epoch, each the direct evaluate() after that epoch in a twin; the training side
    (history, weights) is bit-identical to the fit without validation, whose history has exactly the three loss keys"""
    from othellozero_amd.trainer import VAL_KEYS, fit
    n, C, bs, epochs = 6, 128, 32, 2
    own, opp, pi, z = R.examples(n, C)
    tr, va = slice(0, 50), slice(50, 70)
    val = (own[va], opp[va], pi[va], z[va])
    a, b, twin = (_trainer(n, C, momentum=0.9) for _ in range(3))
    ha = fit(a, own[tr], opp[tr], pi[tr], z[tr], batch_size=bs, epochs=epochs, shuffle_seed=3, validation=val)
    hb = fit(b, own[tr], opp[tr], pi[tr], z[tr], batch_size=bs, epochs=epochs, shuffle_seed=3)
    assert set(hb.history) == {"loss", "pi-reshaped_loss", "v_loss"}
    assert set(ha.history) == set(hb.history) | {"val_" + k for k in VAL_KEYS}
    assert all(ha.history[k] == hb.history[k] for k in hb.history) and ha.lr == hb.lr
    assert all(np.array_equal(x, y) for x, y in zip(a.get_weights(), b.get_weights()))
    twin.set_dataset(own[tr], opp[tr], pi[tr], z[tr])
    for ep in range(epochs):
        twin.fit_epoch(np.random.RandomState(3 + ep).permutation(50), bs)
        direct = twin.evaluate(*val, batch_size=bs)
        assert all(ha.history["val_" + k][ep] == direct[k] for k in VAL_KEYS), (ep, direct)
    assert all(len(ha.history["val_" + k]) == epochs for k in VAL_KEYS)


def test_fit_replay_with_validation_slots(oz):
    """fit_replay(validation_slots=...) on a wrapped buffer: val_* per epoch equal a twin's direct evaluate_replay; history and weights are
    those of fit_replay on a buffer that holds only the training slots, in that order"""
    from othellozero_amd.replay import ReplayBuffer
    from othellozero_amd.trainer import VAL_KEYS, fit_replay, holdout_slots
    n, C, bs, epochs = 6, 128, 16, 2
    own, opp, pi, z = R.examples(n, C)
    buf = ReplayBuffer(n, 60)
    buf.append_examples(own, opp, pi, z)                               # 70 into 60 slots: wrapped, the newest 10 live in slots 0 .. 9
    train_slots, val_slots = holdout_slots(*buf.info(), new_examples=30, share=0.4)
    assert list(val_slots) == [58, 59] + list(range(10)) and len(train_slots) == 48
    a, twin, c = (_trainer(n, C, momentum=0.9) for _ in range(3))
    ha = fit_replay(a, buf, batch_size=bs, epochs=epochs, shuffle_seed=8, validation_slots=val_slots)
    for ep in range(epochs):
        twin.fit_epoch_replay(buf, train_slots[np.random.RandomState(8 + ep).permutation(48)], bs)
        direct = twin.evaluate_replay(buf, val_slots, bs)
        assert all(ha.history["val_" + k][ep] == direct[k] for k in VAL_KEYS), (ep, direct)
    only = ReplayBuffer(n, 48)
    held = buf.read()
    only.append_examples(*(x[train_slots] for x in held))
    hc = fit_replay(c, only, batch_size=bs, epochs=epochs, shuffle_seed=8)
    assert set(hc.history) == {"loss", "pi-reshaped_loss", "v_loss"} and all(ha.history[k] == hc.history[k] for k in hc.history)
    assert all(np.array_equal(x, y) for x, y in zip(a.get_weights(), c.get_weights()))


def _tuples(n, own, opp, pi, z):
    from oracle import nn_numpy as O
    x = O.planes(own, opp, n, dtype=np.float32)
    return [(x[i], pi[i].reshape(n, n), float(z[i])) for i in range(len(z))]


def test_wrapper_evaluate_and_train_with_validation(oz):
    """NNetWrapper.evaluate on a fresh wrapper, before any train: the float64 oracle's numbers, and it changes nothing (weights, version);
    train(validation=...) reports the val_* lists; evaluate(ReplayBuffer, slots) reads the buffer"""
    from othellozero_amd.NNet import NNetWrapper
    from othellozero_amd.replay import ReplayBuffer
    n, C = 6, 128
    own, opp, pi, z = R.examples(n, C)
    w = R.calibrated_weights(n, C)
    net = NNetWrapper((n, n), num_channels_1=C, batch_size=32, epochs=1, max_batch=8, weights=w, policy_loss="flat")
    version = net._weights_version
    ex = _tuples(n, own, opp, pi, z)
    got = net.evaluate(ex[50:])
    want = R.summary(R.metrics(*(a[50:] for a in R.oracle_outputs(n, C)), pi[50:], z[50:], n, "flat"))
    assert _close(got, want) and got["examples"] == 20 and got["decided"] == want["decided"]
    assert net._weights_version == version and net._trainer.step == 0 and all(np.array_equal(x, y) for x, y in zip(net.get_weights(), w))
    buf = ReplayBuffer(n, 70)
    buf.append_examples(own, opp, pi, z)
    assert net.evaluate(buf, np.arange(50, 70)) == got
    hist = net.train(ex[:50], validation=ex[50:])
    assert len(hist.history["val_loss"]) == 1 and np.isfinite(hist.history["val_loss"][0]) and len(hist.history["loss"]) == 1
    assert net.evaluate(ex[50:])["loss"] == hist.history["val_loss"][0]            # the trainer kept the trained weights


def test_loop_with_a_validation_share(oz, tmp_path, monkeypatch, caplog):
    """two iterations of training(replay="device", validation_share=0.25) on 6 x 6 / 128 filters: finite validation numbers, one log line
    per iteration, the held-out slots are the newest quarter of each append; validation_share=None is the run without the keyword"""
    import logging
    from othellozero_amd import loop
    from othellozero_amd.NNet import NNetWrapper
    monkeypatch.chdir(tmp_path)
    n = 6
    kw = dict(board_size=n, num_iterations=2, num_episodes=4, num_simulations=4, degree_exploration=1, temperature=1, e_greedy=0.9,
              evaluation_interval=4, evaluation_iterations=2, temperature_threshold=0, self_play_training=False, self_play_interval=1,
              self_play_total_games=2, self_play_threshold=1, training_buffer_size=8 * 40 * 4, seed=13, replay="device")

    def run(name, **extra):
        random.seed(5)
        np.random.seed(5)
        NNetWrapper._models_built = 100                            # (the trainer's seeds derive from the per-process model index)
        net = NNetWrapper((n, n), num_channels_1=128, batch_size=32, epochs=2, max_batch=8)
        loop.training(neural_network=net, checkpoint_filepath=str(tmp_path / name), **kw, **extra)
        return loop.training.last_network.get_weights()
    built = NNetWrapper._models_built
    try:
        with caplog.at_level(logging.INFO):
            run("val.npz", validation_share=0.25)
        vh = loop.training.validation_history
        assert len(vh) == 2 and sum("held-out evaluation" in r.getMessage() for r in caplog.records) == 2
        for st in vh:
            assert st["examples"] > 0 and len(st["epochs"]) == 2
            assert all(np.isfinite(list(d.values())).all() for d in [st["before"]] + st["epochs"])
            assert st["before"]["examples"] == st["examples"] and 0 <= st["before"]["policy_top1"] <= 1
        plain = run("plain.npz")
        assert loop.training.validation_history == []
        none = run("none.npz", validation_share=None)
        assert all(np.array_equal(x, y) for x, y in zip(plain, none))
    finally:
        NNetWrapper._models_built = built
