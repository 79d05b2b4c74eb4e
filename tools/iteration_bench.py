"""Wall time of ONE iteration of the reference's training loop at main.py's default settings (board 6, 100 episodes x 25
simulations, buffer 76 800, 10 epochs at batch 32, 10 new-vs-old games, 12 + 12 evaluation games against the random agent),
run through othellozero_amd.loop.training on one GPU.  Prints one JSON line with the phase times.
--leaves-per-step K: the batched engines run K descents per game and network batch under virtual loss.

--replay device: the replay-buffer comparison instead -- iterations of loop.training with replay="host" and replay="device" alternating in
this one process on one device (--reps R of each, default 2), self-play + buffer + fit only (no arena, no evaluation: the feature does not
touch them), one JSON line with per-phase seconds of every run.  Host phases: "records -> example tuples", "random.shuffle of the tuples",
"tuples -> data set arrays (pack_examples)", "data set upload"; device phase: "append (device to device)".
--games G --board N --sims S override main.py's 100 / 6 / 25 there; --channels C --batch B --epochs E the network and the fit
(default 512 / 32 / 10); --out FILE also writes the line to FILE."""
import json, logging, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from othellozero_amd import loop
from othellozero_amd.NNet import NNetWrapper


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def replay_comparison():
    import random
    import types
    from othellozero_amd import trainer as T
    from othellozero_amd.replay import ReplayBuffer
    games, n, sims = _arg("--games", 100), _arg("--board", 6), _arg("--sims", 25)
    channels, batch, epochs, reps = _arg("--channels", 512), _arg("--batch", 32), _arg("--epochs", 10), _arg("--reps", 2)
    precision = "f16x2" if channels % 256 == 0 and "--f32" not in sys.argv else "f32"
    marks = []

    def timed(name, fn):
        def w(*a, **k):
            t = time.perf_counter(); r = fn(*a, **k); marks.append((name, time.perf_counter() - t)); return r
        return w
    loop.selfplay_batch = timed("self-play + records to the host", loop.selfplay_batch)
    loop._selfplay_into_replay = timed("self-play + append", loop._selfplay_into_replay)
    loop.examples_from_records = timed("records -> example tuples", loop.examples_from_records)
    loop.random = types.SimpleNamespace(shuffle=timed("random.shuffle of the tuples", random.shuffle), seed=random.seed)
    T.pack_examples = timed("tuples -> data set arrays (pack_examples)", T.pack_examples)
    T.Trainer.set_dataset = timed("data set upload", T.Trainer.set_dataset)
    ReplayBuffer.append_engine = timed("append (device to device)", ReplayBuffer.append_engine)
    out_path = os.path.abspath(_arg("--out", "", str)) if "--out" in sys.argv else None
    os.chdir(tempfile.mkdtemp())
    first = NNetWrapper((n, n), num_channels_1=channels, batch_size=batch, epochs=epochs, max_batch=max(128, games), precision=precision)
    runs = []
    for rep in range(reps):
        for mode in ("host", "device"):
            net = first.copy()
            net.batch_size, net.epochs = batch, epochs
            net.train = timed("fit", net.train)
            del marks[:]
            t0 = time.perf_counter()
            loop.training(board_size=n, num_iterations=1, num_episodes=games, num_simulations=sims, degree_exploration=1, temperature=1,
                          neural_network=net, e_greedy=0.9, evaluation_interval=2, evaluation_iterations=12, temperature_threshold=25,
                          self_play_training=False, self_play_interval=1, self_play_total_games=10, self_play_threshold=6,
                          checkpoint_filepath="./w.npz", training_buffer_size=8 * (n * n - 4) * games, seed=1 + rep, replay=mode)
            run = {"replay": mode, "rep": rep, "seconds": round(time.perf_counter() - t0, 3), "phases": {}}
            for name, dt in marks:
                run["phases"][name] = round(run["phases"].get(name, 0.0) + dt, 4)
            ph = run["phases"]
            if mode == "host":
                run["records_to_dataset_seconds"] = round(sum(ph.get(k, 0.0) for k in ("records -> example tuples", "random.shuffle of the tuples",
                                                                                      "tuples -> data set arrays (pack_examples)", "data set upload")), 4)
            else:
                run["records_to_dataset_seconds"] = ph.get("append (device to device)", 0.0)
                ph["self-play alone"] = round(ph["self-play + append"] - ph["append (device to device)"], 4)
            runs.append(run)
            del net
    out = {"metric": "replay_records_to_dataset_seconds", "settings": {"games": games, "board": n, "sims": sims, "channels": channels, "batch": batch,
                                                                        "epochs": epochs, "precision": precision}, "runs": runs}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if "--replay" in sys.argv:
    if _arg("--replay", "host", str) != "device":
        sys.exit("--replay device runs the comparison of both replay modes; without the flag the tool times the default iteration")
    replay_comparison()
    sys.exit(0)

marks = []
def timed(name, fn):
    def w(*a, **k):
        t = time.perf_counter(); r = fn(*a, **k); marks.append((name, time.perf_counter() - t)); return r
    return w
loop.selfplay_batch = timed("episodes (100 games x 25 sims, lock step)", loop.selfplay_batch)
loop.examples_from_records = timed("records -> example tuples", loop.examples_from_records)
loop.self_play_match = timed("new-vs-old arena (10 games)", loop.self_play_match)
loop.evaluate_against_random = timed("evaluation vs random, sequential drop-in agents (12 games)", loop.evaluate_against_random)
loop.evaluate_against_random_batch = timed("evaluation vs random, lock-step arena (12 games)", loop.evaluate_against_random_batch)

batched = "--batched-eval" in sys.argv
n = 6
lps = int(sys.argv[sys.argv.index("--leaves-per-step") + 1]) if "--leaves-per-step" in sys.argv else 1
precision = "f32" if "--f32" in sys.argv else "f16x2"        # inference AND training arithmetic of the wrapper
net = NNetWrapper((n, n), num_channels_1=512, batch_size=32, epochs=10, max_batch=max(128, 100 * lps), precision=precision)
net.train = timed("fit (10 epochs, batch 32)", net.train)
os.chdir(tempfile.mkdtemp())
t0 = time.perf_counter()
hist = loop.training(board_size=n, num_iterations=1, num_episodes=100, num_simulations=25, degree_exploration=1, temperature=1,
                     neural_network=net, e_greedy=0.9, evaluation_interval=1, evaluation_iterations=12, temperature_threshold=25,
                     self_play_training=True, self_play_interval=1, self_play_total_games=10, self_play_threshold=6,
                     checkpoint_filepath="./othelo_model_weights.h5", training_buffer_size=8 * 32 * 100 * 3, seed=1,
                     batched_evaluation=batched, leaves_per_step=lps)
total = time.perf_counter() - t0
out = {"metric": "seconds_per_training_iteration", "value": total, "settings": "main.py defaults (board 6)", "batched_eval": batched, "precision": precision, "leaves_per_step": lps,
       "phases": {}, "historic": hist}
for name, dt in marks:
    out["phases"][name] = round(out["phases"].get(name, 0.0) + dt, 3)
print(json.dumps(out))
