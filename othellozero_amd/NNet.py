"""NNetWrapper -- drop-in for Net/NNet.py:22-101 (inference side) on the HIP library.

Same constructor arguments, `.network_type`, `.predict(board) -> (pi (n,n) float32, v float32)`,
`.copy()`, `.save_checkpoint(path)`, `.load_checkpoint(path)`.  Added: `.predict_batch`,
`.get_weights()/.set_weights()` (keras Model.get_weights() order), `StubNetWrapper`.
Checkpoints are Keras HDF5 weight files (keras_h5.py).  `.train` (Net/NNet.py:53-68) runs the optimiser steps on the GPU
(oz_trainer_*, trainer.py).
"""
import ctypes as C
from enum import Enum, auto

import numpy as np

from . import _lib, keras_h5
from .weights import init_weights, onn_shapes


class NeuralNets(Enum):          # Net/NNet.py:14-16
    ONN = auto()
    BNN = auto()


class _NetHandle:
    def __init__(self):
        self._h = C.c_void_p()

    def __del__(self):
        try:
            if self._h:
                _lib.load().oz_net_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


PRECISION_MODES = {"f32": 0, "f16x2": 1, "bf16x3": 2}      # oz_net_set_precision


def b3_plan(n, channels, max_batch, layer, kslices=1, tile=0, mix_rows=0):
    """host only, no GPU: the plan a precision-bf16x3 network of that shape and capacity makes for `layer` (1 .. 5 = conv2 .. fc2) with `kslices`
    k-slices under NET_OPT_B3_TILE = tile and NET_OPT_B3_MIX_ROWS = mix_rows -- dict(kernel="b3" / "b3_big" / "b3_mixed", big_rows=the layer's
    leading rows on 256-row tiles, small_tiles=the 128-row tiles of the capacity's other rows) (oz_net_b3_plan: the function the forward asks)"""
    kernel, big_rows, small_tiles = C.c_int(), C.c_int64(), C.c_int64()
    _lib.check(_lib.load().oz_net_b3_plan(int(n), int(channels), int(max_batch), int(layer), int(kslices), int(tile), int(mix_rows),
                                          C.byref(kernel), C.byref(big_rows), C.byref(small_tiles)))
    return dict(kernel=_lib.NET_KERNEL_NAMES[kernel.value], big_rows=big_rows.value, small_tiles=small_tiles.value)


class NNetWrapper(_NetHandle):
    _models_built = 0          # Keras numbers layer names per process (conv2d, ..., conv2d_4, ...); checkpoints keep that

    def __init__(self, board_size=(8, 8), batch_size=32, epochs=10, num_channels_1=512, num_channels_2=256,
                 lr=0.001, dropout=0.3, network=NeuralNets.ONN, max_batch=1, seed=0, weights=None, precision="f32", train_precision=None,
                 policy_loss="rows", optimizer=None, aux_heads=None):
        super().__init__()
        self._model_index = NNetWrapper._models_built
        NNetWrapper._models_built += 1
        self.board_size_x, self.board_size_y = board_size
        assert self.board_size_x == self.board_size_y, "square boards only"
        self.action_size = self.board_size_x * self.board_size_y
        self.batch_size, self.epochs, self.lr, self.dropout = batch_size, epochs, lr, dropout
        self.network_type = network
        self.num_channels = num_channels_1          # num_channels_2 is accepted but unused (OthelloNN.py:39)
        self.max_batch = int(max_batch)
        if network not in (NeuralNets.ONN, NeuralNets.BNN):
            raise Exception('Invalid Network Type.')
        # BNN (Net/BaseNN.py): the same trunk on the one-channel board (+1 BLACK / -1 WHITE, mover-canonical in the search)
        self.in_channels = 2 if network is NeuralNets.ONN else 1
        lib = _lib.require_gpu()
        create = lib.oz_net_create if network is NeuralNets.ONN else lib.oz_net_create_bnn
        _lib.check(create(C.byref(self._h), self.board_size_x, self.num_channels, self.max_batch))
        # precision: "f32" = exact fp32 matrix cores; "f16x2" = f32 via 2 x fp16 split on the 16-bit matrix cores
        # (fp32-equivalent: same <= 1e-5 tolerance, ~4x faster; needs channels % 256 == 0; every activation channel / weight column is moved into the
        #  fp16 window by an exact power of two at commit, a commit-time self-check against the exact-fp32 kernels refuses networks that amplify
        #  rounding, and a position whose activations leave the calibrated range raises OzError(OZ_ERR_STATE) instead of returning a degraded answer)
        self.precision = precision
        # train_precision: the trainer's arithmetic for the 3x3 layers ("f32", "f16x2", "bf16x3"); None = f16x2 for an f16x2 network whose
        # num_channels_1 % 256 == 0, else f32
        assert train_precision in (None, "f32", "f16x2", "bf16x3"), train_precision
        self.train_precision = train_precision
        # policy_loss: "rows" = the reference's cross entropy on the (n, n)-reshaped policy (rows renormalised one by one); "flat" = on the
        # whole n*n softmax, what dense visit-distribution targets need (loop.training(policy_target="visits"))
        assert policy_loss in ("rows", "flat"), policy_loss
        self.policy_loss = policy_loss
        # optimizer: None or a dict of Trainer.set_optimizer's options (l2, weight_decay, decay_mask, global_clipnorm, average_decay, schedule) plus
        # use_average -- train() then commits the trainer's weight AVERAGE to this network (self-play, matches and checkpoints run on it) while the
        # trainer keeps its raw iterate.  Part of the network object: copy() carries the settings (not the optimiser's state), and
        # loop.training needs no parameter for them
        self.optimizer = dict(optimizer) if optimizer else None
        if self.optimizer:
            from .trainer import OPTIMIZER_KEYS
            unknown = set(self.optimizer) - set(OPTIMIZER_KEYS) - {"use_average"}
            assert not unknown, f"optimizer: unknown option(s) {sorted(unknown)}"
            assert not self.optimizer.get("use_average") or self.optimizer.get("average_decay", 0) > 0, "use_average needs average_decay in (0, 1)"
        # aux_heads: None or dict(ownership=w, score=w) -- train() then also trains an ownership and a score head on the games' final boards
        # (Trainer(aux_heads=...): fed by a ReplayBuffer(aux=True)).  The four arrays live with the trainer and in checkpoints; the inference
        # network, predict and the search never see them
        self.aux_heads = dict(aux_heads) if _lib.check_aux_heads(aux_heads) is not None else None
        self._aux_weights = None                      # the heads' four arrays as the last fit / load_checkpoint left them (None: the trainer's fresh ones)
        self._weights_version = 0                     # counts set_weights / init_random: train() re-seeds its trainer when somebody else set the weights
        self._exported_version = None                 # the version train() itself left behind
        self.requested_precision = precision          # what the caller asked for: a refused f16x2 commit falls back for THAT set of weights only
        self.f16x2_refusals = 0                       # commits precision f16x2 refused so far (train() reports it in its history)
        _lib.check(lib.oz_net_set_precision(self._h, PRECISION_MODES[precision]))
        self.set_weights(weights if weights is not None else
                         init_weights(self.board_size_x, seed, self.num_channels, in_channels=self.in_channels))

    # ---- weights (model.get_weights / set_weights, Net/NNet.py:98-101)
    def set_weights(self, weights, on_refusal="raise"):
        """model.set_weights + oz_net_commit.  Precision f16x2 may REFUSE a network at commit (OZ_ERR_STATE: a guard fired on the calibration
        positions, or the self-check against the exact-fp32 kernels measured more than 8e-6).  on_refusal="raise" (default): the OzError
        propagates -- callers that load arbitrary weights decide themselves.  on_refusal="f32": the wrapper warns, switches THIS network to
        precision f32 (exact fp32 kernels on the GPU, always valid) and commits again -- what train() uses, so that a long f16x2 run is not
        ended by the weights of one iteration."""
        lib = _lib.load()
        self._weights_version += 1
        if self.precision != self.requested_precision:        # an earlier set of weights was refused: THIS one gets the requested arithmetic again
            _lib.check(lib.oz_net_set_precision(self._h, PRECISION_MODES[self.requested_precision]))
            self.precision = self.requested_precision
        shapes = onn_shapes(self.board_size_x, self.num_channels, self.in_channels)
        assert len(weights) == len(shapes), f"expected {len(shapes)} arrays"
        for i, (w, shp) in enumerate(zip(weights, shapes)):
            a = np.ascontiguousarray(w, dtype=np.float32)
            assert a.shape == tuple(shp), f"weight {i}: shape {a.shape} != {shp}"
            _lib.check(lib.oz_net_set_weight(self._h, i, _lib.p_f32(a), a.size))
        try:
            _lib.check(lib.oz_net_commit(self._h))
        except _lib.OzError as e:
            if not (on_refusal == "f32" and e.code == _lib.OZ_ERR_STATE and self.precision == "f16x2"):
                raise
            import warnings
            self.f16x2_refusals += 1
            warnings.warn(f"othellozero_amd: precision f16x2 refused these weights at commit ({e}); THESE weights run in precision f32 "
                          f"(refusal {self.f16x2_refusals}; the next set_weights tries f16x2 again)")
            _lib.check(lib.oz_net_set_precision(self._h, 0))
            self.precision = "f32"
            _lib.check(lib.oz_net_commit(self._h))

    def init_random(self, seed):
        """a fresh network as Keras initialises it (glorot_uniform kernels, zero biases, identity BatchNormalization) from the LIBRARY's own
        deterministic stream (oz_net_init_random: what a C host gets; not NumPy's numbers for that seed), committed"""
        lib = _lib.load()
        self._weights_version += 1
        _lib.check(lib.oz_net_init_random(self._h, int(seed)))
        _lib.check(lib.oz_net_commit(self._h))

    def get_weights(self):
        lib = _lib.load()
        out = []
        for i, shp in enumerate(onn_shapes(self.board_size_x, self.num_channels, self.in_channels)):
            a = np.zeros(shp, dtype=np.float32)
            _lib.check(lib.oz_net_get_weight(self._h, i, _lib.p_f32(a), a.size))
            out.append(a)
        return out

    # ---- inference
    def predict_batch(self, own, opp):
        """canonical bitboards (uint64 arrays) -> pi (B, n, n) float32, v (B,) float32"""
        own = np.ascontiguousarray(own, dtype=np.uint64).ravel()
        opp = np.ascontiguousarray(opp, dtype=np.uint64).ravel()
        B, n = own.size, self.board_size_x
        pi = np.zeros((B, n, n), dtype=np.float32)
        v = np.zeros(B, dtype=np.float32)
        lib = _lib.load()
        for s in range(0, B, self.max_batch):
            e = min(B, s + self.max_batch)
            self._last_call_boards = e - s
            _lib.check(lib.oz_net_predict(self._h, _lib.p_u64(own[s:e]), _lib.p_u64(opp[s:e]), e - s,
                                          _lib.p_f32(pi[s:e]), _lib.p_f32(v[s:e])))
        return pi, v

    def forward_launched(self, own, opp, count, pi=None, v=None):
        """test entry (oz_net_forward_launched): ONE forward launched for len(own) positions -- their grid, their launch plan -- of which the first
        `count` are live, the way a search calls the network.  pi (launch, n, n) / v (launch,) float32 are uploaded before the forward (zeros when
        None) and come back whole: rows [0, count) as predict_batch gives them, rows from `count` on as they went in.  activation() and
        layer_plan() then describe this forward (rows of boards beyond `count` are whatever the buffers held)."""
        own = np.ascontiguousarray(own, dtype=np.uint64).ravel()
        opp = np.ascontiguousarray(opp, dtype=np.uint64).ravel()
        launch, n = own.size, self.board_size_x
        assert opp.size == launch
        pi = np.zeros((launch, n, n), np.float32) if pi is None else np.array(pi, dtype=np.float32, order="C").reshape(launch, n, n)
        v = np.zeros(launch, np.float32) if v is None else np.array(v, dtype=np.float32, order="C").reshape(launch)
        rc = _lib.load().oz_net_forward_launched(self._h, _lib.p_u64(own), _lib.p_u64(opp), int(count), launch, _lib.p_f32(pi), _lib.p_f32(v))
        if rc != _lib.OZ_ERR_ARG:
            self._last_call_boards = launch
        _lib.check(rc)
        return pi, v

    def predict(self, board):
        """Net/NNet.py:70-87: board (n,n,2) [ONN] or one-channel (n,n) with +1 / -1 [BNN] -> (pi.reshape(n,n), v[0][0])"""
        if self.in_channels == 1:
            b = np.asarray(board)
            board = np.stack([b == 1, b == -1], axis=2)
        own, opp = _lib.pack_board(board)
        pi, v = self.predict_batch(np.array([own], np.uint64), np.array([opp], np.uint64))
        return pi[0], v[0]

    def _train_arithmetic(self):
        if self.train_precision is not None:
            return self.train_precision
        return "f16x2" if self.precision == "f16x2" and self.num_channels % 256 == 0 else "f32"

    def train(self, examples, verbose=None, seed=None, allreduce=None, validation=None, validation_slots=None):
        """Net/NNet.py:53-68: model.fit(x=boards, y=[pis, vs], batch_size=self.batch_size, epochs=self.epochs) on the GPU
        (oz_trainer_*: MFMA forward / backward in the wrapper's precision -- "f16x2" runs the 3x3 layers' forward and data
        gradient on the fp16 matrix cores like the inference kernels (needs num_channels % 256 == 0, else fp32); train_precision="bf16x3"
        runs their forward and both gradients as three bf16 planes per fp32 value (fp32-class, no scaling, no guard) -- Adam
        lr=self.lr with clipvalue 0.5 for ONN / none for BNN, Dropout self.dropout, BN momentum 0.99; the wrapper's `optimizer` options act inside
        every step; with use_average the network receives the weight average after the fit).  Returns a History-like object (`.history['loss']`, ...).  The TensorBoard
        callback of the reference is not reproduced.  Optimiser state persists across calls like the compiled Keras model's.
        validation (example tuples) / validation_slots (slots of the ReplayBuffer passed as `examples`, held out of the fit: trainer.holdout_slots):
        held-out examples evaluated in inference mode after every epoch, History.history gains the val_* lists (trainer.fit / fit_replay)."""
        from . import trainer as T
        from .replay import ReplayBuffer
        if getattr(self, "aux_heads", None) and allreduce is not None:
            raise ValueError("a network with aux_heads does not train data-parallel: the all-reduce's gradient arena is sized for the forty arrays "
                             "and the host example tuples carry no final pairs (train from a ReplayBuffer(aux=True), single-process)")
        replay = examples if isinstance(examples, ReplayBuffer) else None
        if replay is not None:
            # a device-resident replay buffer in place of the tuple list: the fit reads its slots in place (trainer.fit_replay)
            if allreduce is not None:
                raise ValueError("training from a ReplayBuffer is single-process: a data-parallel fit keeps the step-wise path (pass example tuples)")
            if replay.n != self.board_size_x:
                raise ValueError(f"the ReplayBuffer holds {replay.n} x {replay.n} examples, this network plays {self.board_size_x} x {self.board_size_x}")
            if validation is not None:
                raise ValueError("a fit from a ReplayBuffer takes validation_slots= (slots of that buffer), not validation= example tuples")
            if len(replay) == 0:
                return T.History()
        elif validation_slots is not None:
            raise ValueError("validation_slots= names slots of a ReplayBuffer: pass validation= example tuples with example tuples")
        elif not examples:
            return T.History()
        else:
            own, opp, pi, z = T.pack_examples(examples, self.board_size_x, self.in_channels)
        self._sync_trainer(seed, allreduce)
        shuffle_seed = 1000003 * self._fit_calls + (self._model_index if seed is None else seed)
        if replay is not None:
            hist = T.fit_replay(self._trainer, replay, batch_size=self.batch_size, epochs=self.epochs, shuffle_seed=shuffle_seed, verbose=verbose,
                                validation_slots=validation_slots)
        else:
            val = T.pack_examples(validation, self.board_size_x, self.in_channels) if validation else None
            hist = T.fit(self._trainer, own, opp, pi, z, batch_size=self.batch_size, epochs=self.epochs, shuffle_seed=shuffle_seed,
                         allreduce=allreduce, verbose=verbose, validation=val)
        return self._finish_fit(hist, allreduce)

    def evaluate(self, examples_or_replay, slots=None):
        """keras Model.evaluate on held-out examples, in inference mode on the device (trainer.Trainer.evaluate: moving BN statistics, no dropout, the
        trainer's arithmetic and policy loss): example tuples, or a ReplayBuffer with `slots` (None: every held slot).  -> dict(loss,
        pi-reshaped_loss, v_loss, policy_top1, value_sign, examples, decided).  The trainer is created as train() creates it and receives the
        network's weights only when somebody else has set them since the trainer last exported (the weights version differs); nothing else
        changes -- no step, no optimiser state, no commit.  What is evaluated is the trainer's raw iterate: with use_average the network plays the
        weight average, which this does not measure."""
        from . import trainer as T
        from .replay import ReplayBuffer
        self._sync_trainer(None, None, only_if_changed=True)
        if isinstance(examples_or_replay, ReplayBuffer):
            replay = examples_or_replay
            if replay.n != self.board_size_x:
                raise ValueError(f"the ReplayBuffer holds {replay.n} x {replay.n} examples, this network plays {self.board_size_x} x {self.board_size_x}")
            slots = np.arange(len(replay), dtype=np.int32) if slots is None else np.ascontiguousarray(slots, dtype=np.int32)
            return self._trainer.evaluate_replay(replay, slots, self.batch_size)
        if slots is not None:
            raise ValueError("slots= names slots of a ReplayBuffer")
        own, opp, pi, z = T.pack_examples(examples_or_replay, self.board_size_x, self.in_channels)
        return self._trainer.evaluate(own, opp, pi, z, batch_size=self.batch_size)

    def _sync_trainer(self, seed, allreduce, only_if_changed=False):
        """the trainer of train() / evaluate(): created at the first use, then given the network's weights where they are not its own"""
        from . import trainer as T
        if getattr(self, "aux_heads", None) and allreduce is not None:
            raise ValueError("a network with aux_heads does not train data-parallel (its gradient arena is the library's own)")
        if getattr(self, "_trainer", None) is None:
            assert self.num_channels % 128 == 0, "the training kernels need num_channels % 128 == 0"
            # a GradientAllReduce owns the gradient arena (a torch tensor RCCL can reduce in place): the library writes into it
            self._trainer = T.Trainer(self.board_size_x, self.num_channels, self.in_channels, max_batch=self.batch_size, lr=self.lr,
                                      clipvalue=0.5 if self.network_type is NeuralNets.ONN else 0.0, dropout=self.dropout,
                                      seed=self._model_index if seed is None else seed,
                                      external_grads_ptr=getattr(allreduce, "ptr", None),
                                      precision=self._train_arithmetic(), policy_loss=self.policy_loss,
                                      optimizer={k: v for k, v in (self.optimizer or {}).items() if k != "use_average"},
                                      aux_heads=self.aux_heads)
            self._push_aux_weights()
            self._trainer_arena = getattr(allreduce, "ptr", None)
            self._fit_calls = 0
            self._exported_version = None
        if only_if_changed:              # evaluate(): the weights go in only when the version differs, and the trainer then holds this version
            if self._exported_version != self._weights_version:
                self._trainer.set_weights(self.get_weights())
                self._exported_version = self._weights_version
            return
        assert getattr(allreduce, "ptr", None) == self._trainer_arena, "train() must keep using the GradientAllReduce it started with"
        if not self.optimizer or self._exported_version != self._weights_version:
            # (without options: as ever.)  Somebody else set the network's weights: the trainer (and its average) starts from them
            self._trainer.set_weights(self.get_weights())
        elif allreduce is not None:
            # nobody has: the trainer keeps its raw iterate, moments and average; only the moving statistics the ranks averaged go back in
            mine = self.get_weights()
            for i in range(36):
                if i % 6 in (4, 5):
                    _lib.check(_lib.load().oz_trainer_set_weight(self._trainer._h, i, _lib.p_f32(mine[i]), mine[i].size))

    def _push_aux_weights(self):
        """the auxiliary heads' arrays a checkpoint brought go to the trainer, if there is one (else they wait for it)"""
        if self.aux_heads and self._aux_weights is not None and getattr(self, "_trainer", None) is not None:
            for i, a in zip(range(40, 44), self._aux_weights):
                a = np.ascontiguousarray(a, dtype=np.float32)
                _lib.check(_lib.load().oz_trainer_set_weight(self._trainer._h, i, _lib.p_f32(a), a.size))

    def set_aux_heads(self, aux_heads):
        """switch the auxiliary heads on (or change their weights) before the first train() / evaluate(): the trainer is created with them"""
        new = dict(aux_heads) if _lib.check_aux_heads(aux_heads) is not None else None
        if _lib.check_aux_heads(new) != _lib.check_aux_heads(self.aux_heads) and getattr(self, "_trainer", None) is not None:
            raise ValueError("aux_heads: this network's trainer exists already (the heads are switched on before the first step); create the "
                             "network with NNetWrapper(..., aux_heads=...)")
        self.aux_heads = new

    def aux_weights(self):
        """the four arrays of the auxiliary heads (Wown (512, n*n), bown, Wsc (512, 1), bsc): always the trainer's RAW iterate, with
        use_average too -- the trainer's own (created as train() creates it, if need be), or before there is one what the last fit, a copy() or
        a loaded checkpoint left; checkpoints store these.  None without aux_heads"""
        if not self.aux_heads:
            return None
        if getattr(self, "_trainer", None) is None and self._aux_weights is not None:      # (a copy(), a loaded checkpoint: no trainer needed to know them)
            return [np.array(a, dtype=np.float32) for a in self._aux_weights]
        self._sync_trainer(None, None, only_if_changed=True)
        return self._trainer.get_weights()[40:]

    def _finish_fit(self, hist, allreduce):
        """the end of train(): the trained weights go to the network"""
        self._fit_calls += 1
        use_average = bool(self.optimizer and self.optimizer.get("use_average"))
        weights = self._trainer.get_weights(average=use_average)
        if self.aux_heads:                              # the auxiliary heads stay with the trainer; a copy() of this network starts its own from them:
            # always the RAW iterate, what aux_weights() reports (use_average concerns the network that plays, which has no such heads)
            self._aux_weights = self._trainer.get_weights()[40:] if use_average else weights[40:]
        weights = weights[:40]
        if allreduce is not None:                       # BN moving statistics are per replica: average them
            from .distributed import average_moving_statistics
            weights = average_moving_statistics(weights, getattr(allreduce, "group", None))
        self.set_weights(weights, on_refusal="f32")
        if allreduce is not None:
            # the replicas hold the same weights, so a refusal is the same decision everywhere; should one rank's commit still be refused alone
            # (another calibration outcome on its device, say), EVERY rank evaluates these weights in precision f32 -- no rank decides by itself
            from .distributed import any_rank
            refused = self.precision != self.requested_precision
            if any_rank(refused, getattr(allreduce, "group", None)) and not refused:
                lib = _lib.load()
                _lib.check(lib.oz_net_set_precision(self._h, PRECISION_MODES["f32"]))
                self.precision = "f32"
                _lib.check(lib.oz_net_commit(self._h))
        self._exported_version = self._weights_version
        hist.precision = self.precision                     # the arithmetic these weights are evaluated in until the next set_weights
        hist.train_precision = self._trainer.precision      # the arithmetic the trainer's 3x3 layers ran in
        hist.f16x2_refusals = self.f16x2_refusals           # (attributes, not history entries: Keras' history holds per-epoch number lists only)
        return hist

    # ---- checkpoints (Net/NNet.py:90-96): Keras HDF5 weight files, read and written by keras_h5.py (no h5py needed);
    # files saved by the reference load here and the other way round.  A path ending in .npz selects a plain
    # NumPy archive of the same 40 arrays instead (an extension of this build).
    def save_checkpoint(self, filepath):
        """model.save_weights(filepath, save_format='h5')"""
        aux = self.aux_weights()          # with aux_heads: two more Dense layers, `ownership` and `score` (arrays 40 .. 43)
        if filepath.endswith(".npz"):
            np.savez(filepath, *(self.get_weights() + (aux or [])))
            return
        layers = keras_h5.keras_layer_table(self.get_weights(), self._model_index, self.network_type.name, aux=aux)
        keras_h5.save_keras_weights(filepath, layers)

    def _load_aux(self, arrays):
        """the auxiliary heads' four arrays of a checkpoint: restored into a network with aux_heads, ignored by any other"""
        if not self.aux_heads:
            return
        from .trainer import aux_shapes
        for i, (a, shp) in enumerate(zip(arrays, aux_shapes(self.board_size_x))):
            if tuple(np.shape(a)) != tuple(shp):
                raise ValueError(f"weight {40 + i} of the file has shape {tuple(np.shape(a))}, the auxiliary heads expect {tuple(shp)}")
        self._aux_weights = [np.array(a, dtype=np.float32) for a in arrays]
        self._push_aux_weights()

    def load_checkpoint(self, filepath):
        """model.load_weights(filepath): layers with weights are matched BY ORDER, as Keras does; a file whose
        weighted-layer count or shapes differ from this network raises ValueError."""
        if filepath.endswith(".npz"):
            with np.load(filepath) as z:
                arrays = [z[f"arr_{i}"] for i in range(len(z.files))]
            self.set_weights(arrays[:40] if len(arrays) == 44 else arrays)
            if len(arrays) == 44:
                self._load_aux(arrays[40:])
            return
        assert filepath.endswith('.h5'), 'Expecting a file with .h5 as extension'
        layers = [(name, ws) for name, ws in keras_h5.load_keras_weights(filepath) if ws]
        aux = None
        if len(layers) == 16 and tuple(name for name, _ in layers[14:]) == keras_h5.AUX_LAYERS:      # a file with the auxiliary heads' two layers
            aux, layers = keras_h5.flat_weights(layers[14:]), layers[:14]
        if len(layers) != 14:
            raise ValueError(f"You are trying to load a weight file containing {len(layers)} layers into a model with 14 layers.")
        flat = keras_h5.flat_weights(layers)
        shapes = onn_shapes(self.board_size_x, self.num_channels, self.in_channels)
        if len(flat) != len(shapes):
            raise ValueError(f"the file holds {len(flat)} weight arrays, this network has {len(shapes)}")
        for i, (a, shp) in enumerate(zip(flat, shapes)):
            if tuple(a.shape) != tuple(shp):
                raise ValueError(f"weight {i} of the file has shape {tuple(a.shape)}, this network expects {tuple(shp)}")
        self.set_weights(flat)
        if aux is not None:
            self._load_aux(aux)

    def copy(self):
        net = NNetWrapper((self.board_size_x, self.board_size_y), network=self.network_type,
                          num_channels_1=self.num_channels, max_batch=self.max_batch, weights=self.get_weights(),
                          precision=self.precision, train_precision=self.train_precision, policy_loss=self.policy_loss,
                          optimizer=self.optimizer, aux_heads=self.aux_heads)
        net._aux_weights = self._aux_weights
        mode, seed = self.eval_symmetry()
        if mode != "off" or seed:
            net.set_eval_symmetry(mode, seed)          # the evaluation symmetry is part of the network
        return net

    # ---- profiling hooks used by bench.py
    def time_forward(self, count, iters=3):
        ms = C.c_float()
        _lib.check(_lib.load().oz_net_time_forward(self._h, count, iters, C.byref(ms)))
        return ms.value

    def profile(self, enable=True):
        """HIP-event timing on the launch stream: True / 1 = the dominant launch only, 2 = every kernel of the forward, False / 0 = off"""
        _lib.check(_lib.load().oz_net_profile(self._h, int(enable)))

    def profile_kernels(self, reset=False):
        """{kernel: (ms_total, launches)} for _lib.NET_KERNELS (slots the profile mode did not time stay at their last value)"""
        k = len(_lib.NET_KERNELS)
        ms, cnt = np.zeros(k, np.float64), np.zeros(k, np.int64)
        _lib.check(_lib.load().oz_net_profile_kernels(self._h, _lib.p_f64(ms), _lib.p_i64(cnt), 1 if reset else 0))
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(_lib.NET_KERNELS)}

    def profile_read(self):
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(_lib.load().oz_net_profile_read(self._h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def set_tables(self, mode):
        """f16x2: 2 = conv1 + conv2 from pattern tables (default), 1 = conv1 table + conv2 GEMM, 0 = conv1 kernel + conv2 GEMM"""
        _lib.check(_lib.load().oz_net_set_tables(self._h, int(mode)))

    def set_eval_cache(self, entries):
        """persistent exact-key evaluation cache of this network for up to ~`entries` positions (0 frees it); used by engines created with
        eval_cache=True, emptied whenever the weights change"""
        _lib.check(_lib.load().oz_net_set_eval_cache(self._h, int(entries)))

    def set_eval_symmetry(self, mode, seed=0):
        """the orientation this network evaluates a position in (oz_net_set_eval_symmetry): None / "off" = as given; "random" = the dihedral
        symmetry oz_eval_symmetry(seed, own, opp) of the board, a pure function of the position and the seed -- what AlphaZero and KataGo draw
        per evaluation, here without giving up a deterministic network; "mean" = all eight and the float32 mean of (pi, v), for matches and
        measurements (8x the network work; a call of k positions needs 8 k <= max_batch).  Part of the network: every search, engine, arena
        and predict call that uses it sees the setting; it survives set_weights / train and travels with copy().  Empties the evaluation cache."""
        code, seed = _lib.check_eval_symmetry(mode, seed)
        _lib.check(_lib.load().oz_net_set_eval_symmetry(self._h, code, seed))

    def eval_symmetry(self):
        """(mode, seed) as set_eval_symmetry takes them; ("off", 0) for a network whose option was never touched"""
        m, s = C.c_int(), C.c_uint64()
        _lib.check(_lib.load().oz_net_get_eval_symmetry(self._h, C.byref(m), C.byref(s)))
        return _lib.EVAL_SYM_NAMES[m.value], int(s.value)

    def eval_symmetry_profile(self, enable=True, reset=False):
        """HIP-event timing of the option's two kernels: switches it on / off for the forwards that follow and returns what was timed so far,
        {"k_sym_boards": (ms_total, launches), "k_sym_policy": (ms_total, launches)}"""
        ms, cnt = np.zeros(2, np.float64), np.zeros(2, np.int64)
        _lib.check(_lib.load().oz_net_eval_symmetry_profile(self._h, 1 if enable else 0, _lib.p_f64(ms), _lib.p_i64(cnt), 1 if reset else 0))
        return {"k_sym_boards": (float(ms[0]), int(cnt[0])), "k_sym_policy": (float(ms[1]), int(cnt[1]))}

    def eval_cache_stats(self):
        e, l, h, i = (C.c_int64() for _ in range(4))
        _lib.check(_lib.load().oz_net_eval_cache_stats(self._h, C.byref(e), C.byref(l), C.byref(h), C.byref(i)))
        return dict(entries=e.value, lookups=l.value, hits=h.value, inserts=i.value)

    def set_option(self, option, value):
        """switches (_lib.NET_OPT_*): NET_OPT_SIMPLE_LOOP = the one-barrier conv loop the race screen compares against; precision f16x2, effective
        at the next commit(): NET_OPT_ACT_TARGET_LOG2 / NET_OPT_W_TARGET_LOG2 (calibration / column maxima land below 2^value, default -2),
        NET_OPT_LOW_GUARD_LOG2 (row threshold of the low-side guard, default -17; <= -100 = off), NET_OPT_SELF_CHECK (0 off, 1 enforce, 2 measure);
        precision f32: NET_OPT_F32_STD_TILE = the 3x3 convolutions on the 128 x 128 tile even where the 256 x 256 one would be picked (bit-identical)"""
        _lib.check(_lib.load().oz_net_set_option(self._h, int(option), int(value)))

    def commit(self):
        """oz_net_commit again (options that take effect at commit: NET_OPT_ACT_TARGET_LOG2, NET_OPT_LOW_GUARD_LOG2)"""
        _lib.check(_lib.load().oz_net_commit(self._h))

    def scaling(self, which):
        """precision f16x2: the power-of-two exponents of the last commit -- which 0 .. 4 = per-channel activation exponents of the conv1 .. conv4,
        fc1 outputs, 5 .. 9 = per-column weight exponents of conv2 .. fc2 (oz_net_get_scaling)"""
        C_ = self.num_channels
        size = [C_, C_, C_, C_, 1024, C_, C_, C_, 1024, 512][which]
        out = np.zeros(size, np.int32)
        _lib.check(_lib.load().oz_net_get_scaling(self._h, int(which), _lib.p_i32(out), size))
        return out

    def self_check(self):
        """precision f16x2: what the last commit's self-check measured -- (max |d pi|, max |d v|, positions) between the f16x2 and the
        exact-fp32 kernels on the calibration positions (negative: it did not run); a commit above 8e-6 raises OzError(OZ_ERR_STATE)"""
        a, b, k = C.c_double(), C.c_double(), C.c_int()
        _lib.check(_lib.load().oz_net_self_check(self._h, C.byref(a), C.byref(b), C.byref(k)))
        return a.value, b.value, k.value

    def self_check_guard(self):
        """precision f16x2: the guard bits (1 = above the fp16 range, 4 = a low row) the last commit's self-check saw on the calibration positions
        (0 = none; with NET_OPT_SELF_CHECK = 2 the commit succeeds and this is how a caller learns of them)"""
        v = C.c_int()
        _lib.check(_lib.load().oz_net_get_info(self._h, _lib.NET_INFO_SELF_CHECK_GUARD, C.byref(v)))
        return v.value

    def conv3_tile_rows(self):
        """row-tile height the LAST forward ran conv3 on (f16x2: 256 at bench.py's batch cap, 192 for full 4096-leaf launches, 128 on the latency path;
        f32: 256 = the 256 x 256 tile of large batches, 128 = the standard tile, 64 = the weight-stream kernel of one-position networks; bf16x3: 256 where every row ran on the 256 x 256 tile, else 128 --
        the smallest row tile of the plan, so 128 too for layer_plan()'s "b3_mixed")"""
        v = C.c_int()
        _lib.check(_lib.load().oz_net_get_info(self._h, _lib.NET_INFO_CONV3_TILE_ROWS, C.byref(v)))
        return v.value

    def arithmetic(self):
        """the arithmetic the GEMM layers really run in: self.precision, except "f32" for a bf16x3 network of max_batch < 128 (latency kernels)"""
        v = C.c_int()
        _lib.check(_lib.load().oz_net_get_info(self._h, _lib.NET_INFO_ARITHMETIC, C.byref(v)))
        return {0: "f32", 1: "f16x2", 2: "bf16x3"}[v.value]

    def layer_plan(self):
        """the launch plan of the LAST forward: {layer 1 .. 5 (conv2, conv3, conv4, fc1, fc2): dict(tile_rows=row-tile height (0: the table gather),
        kslices=k-slices of the layer's k loop, kernel=_lib.NET_KERNEL_NAMES name of the kernel / main loop, big_rows=precision bf16x3: the layer's
        leading rows on 256-row tiles -- for kernel "b3_mixed" the boundary between its two launches, with tile_rows = 128)} -- what a test reads to
        show that it ran the configuration it names (oz_net_get_info, OZ_NET_INFO_LAYER_*)"""
        lib, v, plan = _lib.load(), C.c_int(), {}
        for layer in range(1, 6):
            row = []
            for base in (_lib.NET_INFO_LAYER_TILE_ROWS, _lib.NET_INFO_LAYER_KSLICES, _lib.NET_INFO_LAYER_KERNEL, _lib.NET_INFO_LAYER_BIG_ROWS):
                _lib.check(lib.oz_net_get_info(self._h, base + layer, C.byref(v)))
                row.append(v.value)
            plan[layer] = dict(tile_rows=row[0], kslices=row[1], kernel=_lib.NET_KERNEL_NAMES[row[2]], big_rows=row[3])
        return plan

    def activation(self, layer, first_row=0, rows=None):
        """diagnostics: rows [first_row, first_row + rows) of the output of `layer` (0 .. 3 = conv1 .. conv4, 4 / 5 = fc1 / fc2) in the LAST
        oz_net_predict call (predict_batch cuts its boards into calls of max_batch), as float64 (rows, channels) -- exactly what the consuming
        kernel multiplies (oz_net_get_activation).  A row is a (board, pixel) index, boards in call order; rows=None reads to the end of the call.
        OzError(OZ_ERR_STATE) for a layer the forward does not materialise (conv1 in the table modes)."""
        n, C_ = self.board_size_x, self.num_channels
        pixels = [n * n, n * n, (n - 2) ** 2, (n - 4) ** 2, 1, 1][layer]
        channels = [C_, C_, C_, C_, 1024, 512][layer]
        if rows is None:
            rows = getattr(self, "_last_call_boards", 0) * pixels - first_row
        out = np.zeros((int(rows), channels), np.float64)
        _lib.check(_lib.load().oz_net_get_activation(self._h, int(layer), int(first_row), int(rows), _lib.p_f64(out)))
        return out

    def profiled_layer(self):
        """which launch profile_read() timed: 2 = the conv2 GEMM, 3 = the conv3 GEMM (f16x2: conv1 + conv2 are a table gather-sum)"""
        layer = C.c_int()
        _lib.check(_lib.load().oz_net_profiled_layer(self._h, C.byref(layer)))
        return layer.value


class StubNetWrapper(_NetHandle):
    """Device-side deterministic test network (integer hash of the board; formula: oracle/oz_oracle.c
    orc_stub_predict).  Duck-types NNetWrapper for the search / self-play engines."""

    def __init__(self, board_size=(8, 8), salt=0, keep_mask=0, max_batch=1):
        super().__init__()
        self.board_size_x, self.board_size_y = board_size
        self.action_size = self.board_size_x * self.board_size_y
        self.network_type = NeuralNets.ONN
        self.max_batch = int(max_batch)
        self.salt, self.keep_mask = salt, keep_mask
        lib = _lib.require_gpu()
        _lib.check(lib.oz_net_create_stub(C.byref(self._h), self.board_size_x, salt, keep_mask, self.max_batch))

    predict_batch = NNetWrapper.predict_batch
    predict = NNetWrapper.predict
    forward_launched = NNetWrapper.forward_launched
    set_eval_cache = NNetWrapper.set_eval_cache
    eval_cache_stats = NNetWrapper.eval_cache_stats
    set_eval_symmetry = NNetWrapper.set_eval_symmetry
    eval_symmetry = NNetWrapper.eval_symmetry
    eval_symmetry_profile = NNetWrapper.eval_symmetry_profile
