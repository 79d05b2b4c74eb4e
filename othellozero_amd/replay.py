"""Device-resident replay buffer -- C ABI: oz_replay_*.

`ReplayBuffer(board_size, capacity, aux=False)` holds finished training examples in HBM, in the layout of the trainer's resident data set
(own / opp bitboards, one float32 pi row, one float32 z per slot).  It is filled device to device from a `SelfPlayEngine`
(`append_engine`), from move records the host holds (`append_records`: pooled records of a multi-GPU run, saved games) or from finished
examples (`append_examples`), and `trainer.fit_replay` / `NNetWrapper.train(replay)` train from it in place: no example tuples, no
host arrays of examples.  The opt-in counterpart of `loop.CircularArray` for large engines; `loop.training(..., replay="device")` uses it.

Ring rule: the example with running index k (counted from creation or `clear()`) lives in slot k % capacity, the oldest example is
overwritten -- deliberately not the reference's CircularArray + in-place random.shuffle, which overwrites random survivors.
"""
import ctypes as C

import numpy as np

from . import _lib

POLICY_TARGETS = {"onehot": _lib.REPLAY_TARGET_ONEHOT, "visits": _lib.REPLAY_TARGET_VISITS}


def _target(policy_target, target_temperature, engine=False):
    if engine and policy_target == "improved":
        return _lib.REPLAY_TARGET_POLICY, float(target_temperature)
    if policy_target == "improved":
        raise ValueError("policy_target 'improved' is offered for an engine's records only (append_engine)")
    if policy_target not in POLICY_TARGETS:
        raise ValueError(f"policy_target must be 'onehot' or 'visits' (got {policy_target!r})")
    return POLICY_TARGETS[policy_target], float(target_temperature)


class ReplayBuffer:
    def __init__(self, board_size, capacity, aux=False):
        """room for `capacity` examples (1 .. 2^31 - 1) of board_size x board_size boards on the current device: 24 + 4 n^2 bytes each.
        aux=True: every slot also keeps its FINAL PAIR (fin_own, fin_opp: the game's final board from the mover's side under the example's
        symmetry, 0 / 0 for "no auxiliary target"; 16 bytes more), the targets of a Trainer(..., aux_heads=...).  Every append fills it; the
        four arrays of read() are what a plain buffer holds"""
        lib = _lib.require_gpu()
        self.n, self.aux = int(board_size), bool(aux)
        self._h = C.c_void_p()
        _lib.check((lib.oz_replay_create_aux if self.aux else lib.oz_replay_create)(C.byref(self._h), self.n, int(capacity)))

    def __del__(self):
        try:
            if self._h:
                _lib.load().oz_replay_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def info(self):
        """(held, capacity, total): held = min(total, capacity), total = examples appended since creation / clear()"""
        held, cap, total = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.load().oz_replay_info(self._h, C.byref(held), C.byref(cap), C.byref(total)))
        return held.value, cap.value, total.value

    def __len__(self):
        return self.info()[0]

    @property
    def capacity(self):
        return self.info()[1]

    @property
    def total(self):
        return self.info()[2]

    def clear(self):
        _lib.check(_lib.load().oz_replay_clear(self._h))

    def append_engine(self, eng, first_record=0, alias_final=False, policy_target="onehot", target_temperature=1.0, value_target="outcome",
                      exact_empties=0, target=None, surprise_weight=None, exact_proven=False):
        """the records [first_record, completed so far) of a SelfPlayEngine -> 8 examples each, in ascending (game_id, ply), device to
        device; returns the number of records appended.  policy_target="visits" needs an engine created with record_visits=True.
        policy_target="improved" (or target="improved") needs an engine created with gumbel=...: every example's pi is its record's float32
        improved-policy row under the example's symmetry, staged device to device, bit for bit.
        The fast records of a playout cap (_lib.record_fast) are left out and not counted.
        The records of an adjudicated game (_lib.record_adjudicated, an engine created with resign=...) are appended like any other: z is
        the adjudicated one, and with alias_final=True the "final board" of such a game is the board at the stop.
        value_target=("blend", w) / ("td", lam) (an engine created with record_values=True; alias_final=False): the engine computes the
        value targets of those records (SelfPlayEngine.value_targets(value_target, exact_empties, first_record)) and every example's z is
        its record's float32 target instead of the game outcome; "outcome" is the call without it.  exact_proven=True (after
        SelfPlayEngine.proof_targets()): a record with a proof code is exact for those targets, like one within exact_empties.
        surprise_weight=(frac, seed) (an engine created with record_surprise=True): policy surprise weighting.  The engine computes the
        records' weights (SelfPlayEngine.surprise_weights(frac, seed, first_record)) and record i becomes c_i = floor(8 w_i + u_i) examples
        instead of 8, the symmetries (t0_i + k) & 7; `total` advances by the sum of c_i, which self.last_examples then holds.  The return
        value stays the number of non-fast records considered.  Combines with every policy and value target and with alias_final."""
        target, T = _target(policy_target if target is None else target, target_temperature, engine=True)
        mode, _ = _lib.check_value_target(value_target, alias_final)
        xp = {"exact_proven": True} if exact_proven else {}
        done = C.c_int64()
        if surprise_weight is not None:
            try:
                frac, seed = surprise_weight
            except (TypeError, ValueError):
                raise ValueError(f"surprise_weight must be (frac, seed), got {surprise_weight!r}") from None
            frac = _lib.check_surprise_frac(frac)
            vt = mode != _lib.VALUE_TARGET_OUTCOME
            if vt:
                eng.value_targets(value_target, exact_empties=exact_empties, first_record=first_record, **xp)
            self.last_weight_stats = eng.surprise_weights(frac, seed, first_record=first_record)
            examples = C.c_int64()
            _lib.check(_lib.load().oz_replay_append_selfplay_weighted(self._h, eng._h, int(first_record), 1 if alias_final else 0, target, T,
                                                                      1 if vt else 0, C.byref(done), C.byref(examples)))
            self.last_examples = examples.value
            return done.value
        if mode != _lib.VALUE_TARGET_OUTCOME:
            eng.value_targets(value_target, exact_empties=exact_empties, first_record=first_record, **xp)
            _lib.check(_lib.load().oz_replay_append_selfplay_targets(self._h, eng._h, int(first_record), 0, target, T, C.byref(done)))
            return done.value
        _lib.check(_lib.load().oz_replay_append_selfplay(self._h, eng._h, int(first_record), 1 if alias_final else 0, target, T, C.byref(done)))
        return done.value

    def append_records(self, records, visits=None, alias_final=False, policy_target="onehot", target_temperature=1.0, values=None):
        """the same from records on the host (_lib.RECORD_DTYPE; visits = their int32 (R, 64) root visit counts for policy_target="visits"),
        in any order: they are appended in ascending (game_id, ply); returns the number of records appended -- the fast records of a
        playout cap (_lib.record_fast) are left out and not counted.
        values = the records' value targets, float32 (R,) (agents.rules_value_targets, SelfPlayEngine.records(with_targets=True)): every
        example's z is its record's target instead of the records' z"""
        target, T = _target(policy_target, target_temperature)
        rec = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE)
        if values is not None:
            val = np.ascontiguousarray(values, dtype=np.float32).ravel()
            assert val.size == rec.size, f"{val.size} value targets for {rec.size} records"
            cnt = None
            if visits is not None:
                cnt = np.ascontiguousarray(visits, dtype=np.int32).reshape(-1, 64)
                assert cnt.shape[0] == rec.size, f"{cnt.shape[0]} visit-count rows for {rec.size} records"
            _lib.check(_lib.load().oz_replay_append_records_values(self._h, rec.ctypes.data_as(C.c_void_p), None if cnt is None else _lib.p_i32(cnt),
                                                                   _lib.p_f32(val), rec.size, 1 if alias_final else 0, target, T))
            return int((_lib.record_fast(rec) == 0).sum())
        cnt = None
        if visits is not None:
            cnt = np.ascontiguousarray(visits, dtype=np.int32).reshape(-1, 64)
            assert cnt.shape[0] == rec.size, f"{cnt.shape[0]} visit-count rows for {rec.size} records"
        _lib.check(_lib.load().oz_replay_append_records(self._h, rec.ctypes.data_as(C.c_void_p), None if cnt is None else _lib.p_i32(cnt),
                                                        rec.size, 1 if alias_final else 0, target, T))
        return int((_lib.record_fast(rec) == 0).sum())

    def append_examples(self, own, opp, pi, z, fin_own=None, fin_opp=None):
        """finished examples in the given order: own / opp uint64 (N,), pi float32 (N, n*n), z float32 (N,) -- what read() returns.
        fin_own / fin_opp uint64 (N,): their final pairs (read_aux()); without them a buffer with aux=True stores zero pairs, and a plain
        buffer ignores them"""
        own = np.ascontiguousarray(own, dtype=np.uint64).ravel()
        opp = np.ascontiguousarray(opp, dtype=np.uint64).ravel()
        N = own.size
        pi = np.ascontiguousarray(pi, dtype=np.float32).reshape(N, self.n * self.n)
        z = np.ascontiguousarray(z, dtype=np.float32).reshape(N)
        assert opp.size == N, (opp.size, N)
        if fin_own is not None:
            fo = np.ascontiguousarray(fin_own, dtype=np.uint64).ravel()
            fp = np.ascontiguousarray(fin_opp, dtype=np.uint64).ravel()
            assert fo.size == N and fp.size == N, (fo.size, fp.size, N)
            _lib.check(_lib.load().oz_replay_append_examples_aux(self._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z),
                                                                 _lib.p_u64(fo), _lib.p_u64(fp), N))
            return
        _lib.check(_lib.load().oz_replay_append_examples(self._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z), N))

    def read(self, first=0, count=None):
        """slots [first, first + count) (default: every held slot from `first` on) -> (own, opp, pi (count, n*n), z)"""
        first = int(first)
        count = len(self) - first if count is None else int(count)
        k = max(count, 0)
        own, opp = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        pi, z = np.zeros((k, self.n * self.n), np.float32), np.zeros(k, np.float32)
        _lib.check(_lib.load().oz_replay_read(self._h, first, count, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z)))
        return own, opp, pi, z

    def read_aux(self, first=0, count=None):
        """the final pairs of slots [first, first + count) (default: every held slot from `first` on) -> (fin_own, fin_opp) uint64; a buffer
        with aux=True only (OzError OZ_ERR_STATE otherwise)"""
        first = int(first)
        count = len(self) - first if count is None else int(count)
        k = max(count, 0)
        fo, fp = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        _lib.check(_lib.load().oz_replay_read_aux(self._h, first, count, _lib.p_u64(fo), _lib.p_u64(fp)))
        return fo, fp

    def save(self, path):
        """one .npz: the held examples in AGE order (oldest first) plus board size, capacity and total; a buffer with aux=True adds the
        arrays fin_own / fin_opp"""
        held, cap, total = self.info()
        own, opp, pi, z = self.read(0, held)
        age = (np.arange(total - held, total) % cap).astype(np.int64)          # slot of the i-th oldest held example
        extra = {}
        if self.aux:
            fo, fp = self.read_aux(0, held)
            extra = dict(fin_own=fo[age], fin_opp=fp[age])
        with open(path, "wb") as f:
            np.savez(f, own=own[age], opp=opp[age], pi=pi[age], z=z[age], board_size=np.int64(self.n), capacity=np.int64(cap),
                     total=np.int64(total), **extra)

    @classmethod
    def load(cls, path, capacity=None, aux=False):
        """a buffer with the slot layout, contents and `total` of the saved one.  capacity: the saved one's unless given -- a smaller one
        keeps the newest examples; a larger one than a buffer that had already wrapped restarts the running index at the number kept
        (the overwritten examples are gone).  aux=True: a buffer that keeps the final pairs -- the file's, or zero pairs for a file saved
        without them; aux=False ignores the file's pairs"""
        with np.load(path, allow_pickle=False) as f:
            own, opp, pi, z = (np.ascontiguousarray(f[k]) for k in ("own", "opp", "pi", "z"))
            n, cap, total = int(f["board_size"]), int(f["capacity"]), int(f["total"])
            fin = (np.ascontiguousarray(f["fin_own"]), np.ascontiguousarray(f["fin_opp"])) if aux and "fin_own" in f.files else None
        buf = cls(n, cap if capacity is None else capacity, aux=True) if aux else cls(n, cap if capacity is None else capacity)
        keep = min(own.size, buf.capacity)
        if keep < min(total, buf.capacity):
            total = keep
        first = own.size - keep
        own = np.ascontiguousarray(own[first:], dtype=np.uint64)
        opp = np.ascontiguousarray(opp[first:], dtype=np.uint64)
        pi = np.ascontiguousarray(pi.reshape(-1, n * n)[first:], dtype=np.float32)
        z = np.ascontiguousarray(z[first:], dtype=np.float32)
        if fin is not None:
            fo = np.ascontiguousarray(fin[0][first:], dtype=np.uint64)
            fp = np.ascontiguousarray(fin[1][first:], dtype=np.uint64)
            _lib.check(_lib.load().oz_replay_restore_aux(buf._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z), _lib.p_u64(fo),
                                                         _lib.p_u64(fp), keep, total))
            return buf
        _lib.check(_lib.load().oz_replay_restore(buf._h, _lib.p_u64(own), _lib.p_u64(opp), _lib.p_f32(pi), _lib.p_f32(z), keep, total))
        return buf
