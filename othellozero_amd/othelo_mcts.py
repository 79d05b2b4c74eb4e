"""OthelloMCTS -- drop-in for othelo_mcts.py:9-88 + MCTS/__init__.py:19-187 on the HIP search kernels.

One instance = one per-game search table on the GPU (`oz_mcts` with a single slot).  `simulate(state,
player)` runs ONE simulation like the reference; when the network is a native `NNetWrapper` /
`StubNetWrapper` the leaf is evaluated on the device, otherwise (any duck-typed object with `.predict`)
the leaf board is handed to `neural_network.predict` on the host and its (pi, v) go back to the expand /
backup kernel -- the tree never leaves the GPU either way.
"""
import ctypes as C
import random

import numpy as np

from . import _lib
from .NNet import NeuralNets
from .Othello import OthelloGame, OthelloPlayer


class OthelloMCTS:
    def __init__(self, board_size, neural_network, degree_exploration, q_mode=_lib.QMODE_F64,
                 node_cap=8192, leaves_per_step=1, solve_leaves=0, forced_playouts=None, gumbel=None, value_signs="reference", proofs=False,
                 proof_play=False, selection=None, tree_gc="off"):
        """q_mode: OZ_QMODE_F64 = the NumPy 1.18.5 promotion the reference pins (requirements.txt:19),
        OZ_QMODE_NEP50 = what NumPy >= 2 computes (SURVEY.md R-FP).
        leaves_per_step > 1 (native networks only, created with max_batch >= leaves_per_step): that many descents of the tree per
        network batch, kept apart by a virtual loss (oz_mcts_set_leaves_per_step); not the reference's search order.
        solve_leaves=E > 0 (native networks only): a leaf with at most E empties takes its exact win / draw / loss (+1 / 0 / -1 for the side
        to move, oz_mcts_set_solve_leaves) in place of the network's value; the priors stay the network's.  Not the reference's search.
        forced_playouts=k > 0: KataGo's forced playouts on every root that carries noise (set_root_noise / sample_root_noise; without noise
        the search is unchanged), and pruned_counts / get_policy_action_probabilities(..., pruned=True) give the pruned policy target
        (oz_mcts_set_forced_playouts).  Not the reference's search.
        gumbel=(max_considered, c_visit, c_scale) or True: the search keeps every node's own value and is ready for the Gumbel root rule
        (include/othellozero_amd.h, "Gumbel search"): sample_gumbel / set_gumbel arm a root before its simulations, gumbel_policy gives the
        move and the improved policy afterwards.  It replaces root noise, forced playouts and move sampling; not with leaves_per_step > 1.
        Not the reference's search.
        value_signs="sound": the backup negates a value once per change of the side to move, not once per level, and a finished board is worth
        the sign of its disc difference to the side to move there, a draw 0 (oz_mcts_set_value_signs; include/othellozero_amd.h, "value
        signs").  "reference" (the default) is the reference's rule, which stores the wrong sign for a move that ends the game and across every
        pass.  Not the reference's search.
        proofs=True (needs value_signs="sound"; native networks only): exact values -- finished boards, solved leaves -- are kept as proofs
        and backed up the tree; the descent never picks a proven loss while something else is left, takes the exact value in place of the
        averaged Q and stops at a proven position (oz_mcts_set_proofs; include/othellozero_amd.h, "proofs").  root_proof / dump_proofs /
        proof_stats read them.  Not with gumbel or forced_playouts.
        proof_play=True (needs proofs=True): proven_counts / get_policy_action_probabilities(..., proven=True) / root_value(..., proven=True) /
        sample_action(..., proven=True) give the row, the policy, the value and the sampled move the root's proofs leave
        (include/othellozero_amd.h, "proof play"); the flag itself changes no call -- callers (execute_episode, the agents) read it.
        selection=dict(fpu=(reduction, root_reduction), cpuct_growth=(base, factor), prior_first=bool), every key optional: the descent's
        U = Q + c P sqrt(Ns) / (1 + N) with an unvisited move valued at the node's running value minus a reduction (first-play urgency)
        in place of 0, an exploration constant that grows with the node's visits, and a first visit that follows the prior
        (oz_mcts_set_selection; include/othellozero_amd.h, "selection").  None, or every part off, is the search as it was.  Every node then
        keeps the value its expansion backed up (node_values).  Not with gumbel or forced_playouts.  Not the reference's search.
        tree_gc="demand" | "every" ("off" is the default): collect() on the wrapper's own account (include/othellozero_amd.h, "tree
        collection") -- "every": before a simulate / simulate_n call whose root differs from the previous call's; "demand": when the node
        count at the last read plus the simulations since says the call may not fit node_cap (no read-back per simulation).  Counts, values
        and policies are those of the object without the option as long as the roots' disc counts never decrease: a root set to an EARLIER
        position finds its dropped nodes gone and expands them afresh -- a loss of statistics, never an error.  node_cap keeps its meaning
        and default; the option makes a smaller one sufficient."""
        self._gc_mode = _lib.check_tree_gc(tree_gc)
        self.tree_gc = tree_gc
        self._sim_root, self._gc_bound = None, 0
        self._selection = _lib.check_selection(selection, gumbel=gumbel, forced_playouts=forced_playouts)
        self.value_signs = value_signs
        vs_mode = _lib.check_value_signs(value_signs)
        self.proofs = _lib.check_proofs(proofs, value_signs, gumbel=gumbel, forced_playouts=forced_playouts)
        self.proof_play = _lib.check_proof_play(proof_play, self.proofs)
        self.gumbel = _lib.check_gumbel_options(gumbel, forced_playouts=forced_playouts, leaves_per_step=leaves_per_step)
        self.forced_playouts = _lib.check_forced_playouts(forced_playouts, need_noise=False)
        self._forced_set = False
        self.solve_leaves = _lib.check_solve_leaves(solve_leaves)
        self._board_size = board_size
        self._neural_network = neural_network
        # othelo_mcts.py:15-18: ONN nets see the two-channel board, BNN nets the one-channel (+1 / -1) view
        self._one_channel = getattr(neural_network.network_type, "name", "") == "BNN"
        self.degree_explorarion = degree_exploration
        self._q_mode = q_mode
        self._node_cap = node_cap
        self._h = C.c_void_p()
        self._native = getattr(neural_network, "_h", None) is not None
        self.leaves_per_step = int(leaves_per_step)
        if not 1 <= self.leaves_per_step <= _lib.MAX_LEAVES_PER_STEP:
            raise ValueError(f"leaves_per_step must be 1 .. {_lib.MAX_LEAVES_PER_STEP} (got {leaves_per_step})")
        if self.leaves_per_step != 1 and not self._native:
            raise ValueError("leaves_per_step > 1 needs a native NNetWrapper / StubNetWrapper (the leaves are evaluated on the device)")
        if self.proofs and not self._native:
            raise ValueError("proofs=True needs a native NNetWrapper / StubNetWrapper (the leaves are evaluated on the device)")
        if self.solve_leaves and not self._native:
            raise ValueError("solve_leaves > 0 needs a native NNetWrapper / StubNetWrapper (the leaves are evaluated and solved on the device)")
        lib = _lib.require_gpu()
        _lib.check(lib.oz_mcts_create(C.byref(self._h), board_size, 1, node_cap, float(degree_exploration), q_mode))
        self._root = None
        if vs_mode:
            _lib.check(lib.oz_mcts_set_value_signs(self._h, vs_mode))
        if self.proofs:
            _lib.check(lib.oz_mcts_set_proofs(self._h, 1))
        if self._selection[0]:
            _lib.check(lib.oz_mcts_set_selection(self._h, *self._selection))
        if self.leaves_per_step != 1:
            _lib.check(lib.oz_mcts_set_leaves_per_step(self._h, self.leaves_per_step))
        if self.solve_leaves:
            _lib.check(lib.oz_mcts_set_solve_leaves(self._h, self.solve_leaves))
        if self.gumbel is not None:                        # over the empty tree: the parameters, no root armed yet (the budget comes with the arming)
            _lib.check(lib.oz_mcts_set_gumbel(self._h, self.gumbel[0], self.gumbel[1], self.gumbel[2], 1, None, None))

    # ---- tree collection (include/othellozero_amd.h, "tree collection")
    def collect(self):
        """drop the stored nodes the current root has passed (oz_mcts_collect): those that are not the root and hold no more discs than it.
        -> (nodes before, nodes kept); (0, 0) before the first root is set.  No statistic of a kept node changes."""
        out = np.zeros(2, np.int64)
        _lib.check(_lib.load().oz_mcts_collect(self._h, _lib.p_i64(out)))
        if self._root is not None:
            self._gc_bound = int(out[1])
        return int(out[0]), int(out[1])

    # ---- selection (include/othellozero_amd.h, "selection")
    @property
    def selection(self):
        """the selection rule the library runs, as the keyword takes it (None: the default rule)"""
        flags, vals = C.c_int(), [C.c_double() for _ in range(4)]
        _lib.check(_lib.load().oz_mcts_get_selection(self._h, C.byref(flags), *(C.byref(v) for v in vals)))
        return _lib.selection_dict((flags.value, *(v.value for v in vals)))

    def node_values(self):
        """per node, in dump()'s order: the value its expansion backed up (vhat; kept under selection= and gumbel=, 0.0 otherwise)"""
        lib = _lib.load()
        nn = np.zeros(1, np.int32)
        _lib.check(lib.oz_mcts_num_nodes(self._h, _lib.p_i32(nn)))
        out, v = [], C.c_double()
        for i in range(int(nn[0])):
            _lib.check(lib.oz_mcts_node_value(self._h, 0, i, C.byref(v)))
            out.append(v.value)
        return out

    # ---- Gumbel search (include/othellozero_amd.h, "Gumbel search")
    def _need_gumbel(self):
        if self.gumbel is None:
            raise ValueError("this search was created without gumbel=(max_considered, c_visit, c_scale)")

    def sample_gumbel(self, budget, seed, game_id, ply, state=None, player=None):
        """arm the current root (or `state` seen by `player`, which becomes the root) for a search of `budget` simulations: g drawn on the
        device, keyed (seed, game_id, ply), N0 = the root's counts now"""
        self._need_gumbel()
        if state is not None:
            self._set_root(*self._canonical(state, player))
        gid, pl = np.array([int(game_id)], np.uint64), np.array([int(ply)], np.int32)
        _lib.check(_lib.load().oz_mcts_sample_gumbel(self._h, self.gumbel[0], self.gumbel[1], self.gumbel[2], int(budget), int(seed),
                                                     _lib.p_u64(gid), _lib.p_i32(pl)))

    def set_gumbel(self, g, budget, state=None, player=None):
        """the same with host-supplied draws: g = (n, n) or (64,) by square row*8+col; None disarms"""
        self._need_gumbel()
        if state is not None:
            self._set_root(*self._canonical(state, player))
        row = None
        if g is not None:
            e = np.asarray(g, dtype=np.float64)
            n = self._board_size
            row = np.zeros((1, 64), np.float64)
            if e.shape == (n, n):
                row.reshape(8, 8)[:n, :n] = e
            elif e.size == 64:
                row[0] = e.ravel()
            else:
                raise ValueError(f"g must be ({n}, {n}) or 64 values (got shape {e.shape})")
        _lib.check(_lib.load().oz_mcts_set_gumbel(self._h, self.gumbel[0], self.gumbel[1], self.gumbel[2], int(budget),
                                                  None if row is None else _lib.p_f64(row), None))

    def gumbel_root(self):
        """(g (64,) float64 by square, armed bool, N0 (64,) int32) of the current root"""
        g, armed, n0 = np.zeros((1, 64), np.float64), np.zeros(1, np.uint8), np.zeros((1, 64), np.int32)
        _lib.check(_lib.load().oz_mcts_get_gumbel(self._h, _lib.p_f64(g), _lib.p_u8(armed), _lib.p_i32(n0), None, None, None, None))
        return g[0], bool(armed[0]), n0[0]

    def gumbel_policy(self, state):
        """after the simulations of an armed root, for the mover-canonical `state` (as get_policy_action_probabilities takes it):
        ((row, col) = the Gumbel root's move, pi float32 (n, n) = the improved policy softmax(logit + sigma(completed Q))).  KeyError if the
        state is unknown or its root is not armed."""
        self._need_gumbel()
        own, opp = _lib.pack_board(state)
        self._set_root(own, opp)
        pi, action, rc = np.zeros((1, 64), np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        _lib.check(_lib.load().oz_mcts_gumbel_policy(self._h, _lib.p_f32(pi), _lib.p_i32(action), _lib.p_i32(rc)))
        if rc[0] != 0 or action[0] < 0:
            raise KeyError("state is unknown to the search or its root is not armed (sample_gumbel / set_gumbel before the simulations)")
        n = self._board_size
        return (int(action[0]) >> 3, int(action[0]) & 7), pi.reshape(8, 8)[:n, :n].copy()

    def rows_solved(self):
        """leaves this search has given their exact value so far (0 without solve_leaves)"""
        e, rows = C.c_int(), C.c_int64()
        _lib.check(_lib.load().oz_mcts_get_solve_leaves(self._h, C.byref(e), C.byref(rows)))
        return rows.value

    def __del__(self):
        try:
            if self._h:
                _lib.load().oz_mcts_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ---- helpers
    def _set_root(self, own, opp):
        if self._root != (own, opp):
            a, b = np.array([own], np.uint64), np.array([opp], np.uint64)
            _lib.check(_lib.load().oz_mcts_set_roots(self._h, _lib.p_u64(a), _lib.p_u64(b), None))
            self._root = (own, opp)

    def _last_value(self):
        val, vt = np.zeros(1, np.float64), np.zeros(1, np.int32)
        _lib.check(_lib.load().oz_mcts_last_value(self._h, _lib.p_f64(val), _lib.p_i32(vt), None))
        if vt[0] == _lib.VT_INT:
            return int(val[0])
        if vt[0] == _lib.VT_F32:
            return np.float32(val[0])
        return float(val[0])

    def _canonical(self, state, player):
        c0, c1 = _lib.pack_board(state)
        return (c1, c0) if player is OthelloPlayer.WHITE or getattr(player, "value", 1) == -1 else (c0, c1)

    # ---- root noise (include/othellozero_amd.h, "root noise"): applied at selection time to the root it is set for; stored priors never change
    def set_root_noise(self, eta, epsilon, state=None, player=None):
        """host-supplied noise for the current root (or for `state` seen by `player`, which becomes the root): eta = (n, n) or (64,) by square
        row*8+col, 0 off the legal set.  eta None or epsilon 0 disarms."""
        epsilon = float(epsilon)
        if not 0.0 <= epsilon <= 1.0:
            raise ValueError(f"epsilon must be in [0, 1] (got {epsilon})")
        if state is not None:
            self._set_root(*self._canonical(state, player))
        row = None
        if eta is not None:
            e = np.asarray(eta, dtype=np.float64)
            n = self._board_size
            row = np.zeros((1, 64), np.float64)
            if e.shape == (n, n):
                row.reshape(8, 8)[:n, :n] = e
            elif e.size == 64:
                row[0] = e.ravel()
            else:
                raise ValueError(f"eta must be ({n}, {n}) or 64 values (got shape {e.shape})")
            if not (np.isfinite(row).all() and (row >= 0).all() and (row <= 1).all()):
                raise ValueError("eta must lie in [0, 1]")
        _lib.check(_lib.load().oz_mcts_set_root_noise(self._h, epsilon, None if row is None else _lib.p_f64(row), None))
        self._arm_forced(row is not None and epsilon > 0.0)

    def sample_root_noise(self, alpha, epsilon, seed, game_id, ply, state=None, player=None):
        """device-drawn Dirichlet(alpha) noise over the legal moves of the current root (or of `state` seen by `player`, which becomes the
        root), keyed (seed, game_id, ply)"""
        alpha, epsilon = _lib.check_root_noise((alpha, epsilon))
        if state is not None:
            self._set_root(*self._canonical(state, player))
        gid, pl = np.array([int(game_id)], np.uint64), np.array([int(ply)], np.int32)
        _lib.check(_lib.load().oz_mcts_sample_root_noise(self._h, alpha, epsilon, int(seed), _lib.p_u64(gid), _lib.p_i32(pl)))
        self._arm_forced(epsilon > 0.0)

    def _arm_forced(self, noisy):
        """the library takes the forcing constant once noise is armed: hand it over at the first arming"""
        if self.forced_playouts > 0.0 and noisy and not self._forced_set:
            _lib.check(_lib.load().oz_mcts_set_forced_playouts(self._h, self.forced_playouts))
            self._forced_set = True

    def root_noise(self):
        """(eta (64,) float64 by square, armed bool, epsilon) of the current root"""
        eta, armed, eps = np.zeros((1, 64), np.float64), np.zeros(1, np.uint8), C.c_double()
        _lib.check(_lib.load().oz_mcts_get_root_noise(self._h, _lib.p_f64(eta), _lib.p_u8(armed), C.byref(eps)))
        return eta[0], bool(armed[0]), eps.value

    # ---- move sampling (include/othellozero_amd.h, "move sampling"): the engines' move rule for the opening plies, on the bare search
    def sample_action(self, state, temperature, seed, game_id, ply, proven=False):
        """the move drawn in proportion to N ** (1 / temperature) over the visit counts of the mover-canonical `state` (as
        get_policy_action_probabilities takes it), keyed (seed, game_id, ply): (row, col).  KeyError if the state is unknown or was never
        selected from.  proven=True (proofs=True): over proven_counts(state)."""
        temperature, _ = _lib.check_sample_moves((temperature, 0))
        own, opp = _lib.pack_board(state)
        self._set_root(own, opp)
        gid, pl = np.array([int(game_id)], np.uint64), np.array([int(ply)], np.int32)
        action, rc = np.zeros(1, np.int32), np.zeros(1, np.int32)
        fn = _lib.load().oz_mcts_proven_sample_moves if proven else _lib.load().oz_mcts_sample_moves
        _lib.check(fn(self._h, temperature, int(seed), _lib.p_u64(gid), _lib.p_i32(pl), _lib.p_i32(action),
              _lib.p_i32(rc)))
        if rc[0] != 0 or action[0] < 0:
            raise KeyError("state is unknown to the search or was never selected from")
        return int(action[0]) >> 3, int(action[0]) & 7

    # ---- reference surface
    def simulate(self, state, player):
        """othelo_mcts.py:22-26 + MCTS/__init__.py:30-71; `state` is not mutated."""
        return self.simulate_n(state, player, 1)

    def simulate_n(self, state, player, count):
        """`count` consecutive simulate(state, player) calls; returns the value of the last one."""
        lib = _lib.load()
        own, opp = self._canonical(state, player)
        self._set_root(own, opp)
        if self._gc_mode == _lib.TREE_GC["every"] and self._sim_root not in (None, (own, opp)):
            self.collect()
        elif self._gc_mode == _lib.TREE_GC["demand"] and self._gc_bound + int(count) > self._node_cap:
            self.collect()
        self._sim_root = (own, opp)
        self._gc_bound += int(count)                       # a simulation expands at most one node
        n = self._board_size
        if self._native:
            _lib.check(lib.oz_mcts_simulate(self._h, self._neural_network._h, int(count)))
            return self._last_value()
        status, lo, lp = np.zeros(1, np.int32), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        pi, v = np.zeros((1, n * n), np.float32), np.zeros(1, np.float32)
        for _ in range(int(count)):
            _lib.check(lib.oz_mcts_select(self._h))
            _lib.check(lib.oz_mcts_leaves(self._h, _lib.p_i32(status), _lib.p_u64(lo), _lib.p_u64(lp)))
            if status[0] == _lib.LEAF_EVAL:
                leaf = _lib.unpack_board(int(lo[0]), int(lp[0]), n)
                if self._one_channel:                      # othelo_mcts.py:85-86
                    leaf = OthelloGame.convert_to_one_channel_board(leaf)
                p, val = self._neural_network.predict(leaf)
                pi[0] = np.asarray(p, dtype=np.float32).reshape(-1)
                v[0] = val
            _lib.check(lib.oz_mcts_backup(self._h, _lib.p_f32(pi), _lib.p_f32(v)))
        return self._last_value()

    def _counts(self, state, pruned=False, proven=False):
        """visit counts of a mover-canonical state: (rc, counts[64], legal mask); pruned: the policy target's row (oz_mcts_pruned_counts);
        proven: the row the root's proofs keep (oz_mcts_proven_counts)"""
        own, opp = _lib.pack_board(state)
        self._set_root(own, opp)
        cnt, legal, rc = np.zeros(64, np.int32), np.zeros(1, np.uint64), np.zeros(1, np.int32)
        fn = _lib.load().oz_mcts_proven_counts if proven else _lib.load().oz_mcts_pruned_counts if pruned else _lib.load().oz_mcts_root_counts
        _lib.check(fn(self._h, _lib.p_i32(cnt), _lib.p_u64(legal), _lib.p_i32(rc)))
        return int(rc[0]), cnt, int(legal[0])

    def pruned_counts(self, state):
        """int32 (64,) by square: the visit counts of the mover-canonical `state` as the policy target keeps them -- pruned
        (include/othellozero_amd.h, "forced playouts") while the state is the root and carries noise and forced_playouts is on, the raw counts
        otherwise.  KeyError if the state is unknown or was never selected from."""
        rc, cnt, _ = self._counts(state, pruned=True)
        if rc != 0:
            raise KeyError("state is unknown to the search or was never selected from")
        return cnt

    def proven_counts(self, state):
        """int32 (64,) by square: the visit counts of the mover-canonical `state` as its proofs keep them (include/othellozero_amd.h, "proof
        play"): the raw counts of the moves the descent would still pick at the root, 0 elsewhere.  Needs proofs=True.  KeyError if the
        state is unknown or was never selected from."""
        rc, cnt, _ = self._counts(state, proven=True)
        if rc != 0:
            raise KeyError("state is unknown to the search or was never selected from")
        return cnt

    def root_value(self, state, proven=False):
        """the search's value of the mover-canonical `state` for the player to move: the visit-weighted mean of its edges' Q over the raw
        visit counts (include/othellozero_amd.h, "value targets"; agents.rules_root_values of the node's dump).  KeyError if the state is
        unknown or was never selected from.  proven=True (proofs=True): the exact value where the state's value is proven."""
        own, opp = _lib.pack_board(state)
        self._set_root(own, opp)
        val, rc = np.zeros(1, np.float64), np.zeros(1, np.int32)
        fn = _lib.load().oz_mcts_proven_root_values if proven else _lib.load().oz_mcts_root_values
        _lib.check(fn(self._h, _lib.p_f64(val), _lib.p_i32(rc)))
        if rc[0] != 0:
            raise KeyError("state is unknown to the search or was never selected from")
        return float(val[0])

    def N(self, state, action=None):
        """MCTS/__init__.py:73-84,172-175: 0 for an unknown state, Ns without an action, Nsa[action] otherwise
        (KeyError if the state was never selected from)."""
        rc, cnt, legal = self._counts(state)
        if rc == 1:
            return 0
        if action is None:
            return int(cnt.sum())                     # Ns == sum of Nsa (both are incremented together)
        sq = int(action[0]) * 8 + int(action[1])
        if rc == 2 or not (legal >> sq) & 1:
            raise KeyError(tuple(action))
        return int(cnt[sq])

    def get_state_actions(self, state):
        """othelo_mcts.py:40-41: legal actions of BLACK (= channel 0) as tuples, ascending row-major."""
        return [tuple(int(x) for x in a) for a in OthelloGame.get_player_valid_actions(state, OthelloPlayer.BLACK)]

    def get_policy_action_probabilities(self, state, temperature, pruned=False, proven=False):
        """othelo_mcts.py:51-67, evaluated with the same NumPy / random calls as the reference.  pruned=True: over pruned_counts(state), the
        policy target of a search with forced playouts.  proven=True: over proven_counts(state)."""
        n = self._board_size
        rc, cnt, legal = self._counts(state, pruned, proven)
        if rc == 2:
            raise KeyError("state was expanded but never selected from (num_simulations < 2)")
        probabilities = np.zeros((n, n))
        actions = [(s >> 3, s & 7) for s in range(64) if (legal >> s) & 1]
        if temperature == 0:
            for row, col in actions:
                probabilities[row, col] = int(cnt[row * 8 + col])
            bests = np.argwhere(probabilities == probabilities.max())
            row, col = random.choice(bests)
            probabilities = np.zeros((n, n))
            probabilities[row, col] = 1
            return probabilities
        for row, col in actions:
            probabilities[row, col] = int(cnt[row * 8 + col]) ** (1 / temperature)
        return probabilities / (np.sum(probabilities) or 1)

    # ---- the game hooks MCTS/__init__.py:86-166 declares abstract and othelo_mcts.py:28-49,69-88 fills in.  The search never calls
    # them here (the kernels carry the rules); callers that use them directly get the LIBRARY's rules kernels through the C ABI
    # (oz_rules_status / oz_rules_apply_moves / oz_rules_legal_moves on the packed board), i.e. the same bit-parallel code the search runs.
    # (no CPU fallback by design: without a GPU / the built library they raise OzLibraryError through require_gpu, like every compute call)
    def _rules_status(self, state):
        _lib.require_gpu()
        c0, c1 = (np.array([x], np.uint64) for x in _lib.pack_board(state))
        fin, p0, p1, win = np.zeros(1, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int8)
        _lib.check(_lib.load().oz_rules_status(_lib.p_u64(c0), _lib.p_u64(c1), self._board_size, 1, _lib.p_u8(fin), _lib.p_i32(p0),
                                               _lib.p_i32(p1), _lib.p_i8(win)))
        return bool(fin[0]), int(win[0])

    def _legal_mask(self, own, opp):
        _lib.require_gpu()
        legal = np.zeros(1, np.uint64)
        _lib.check(_lib.load().oz_rules_legal_moves(_lib.p_u64(np.array([own], np.uint64)), _lib.p_u64(np.array([opp], np.uint64)),
                                                    self._board_size, 1, _lib.p_u64(legal)))
        return int(legal[0])

    def is_terminal_state(self, state):
        return self._rules_status(state)[0]

    def get_state_reward(self, state):
        return self._rules_status(state)[1]                    # +1: channel 0 holds at least as many discs (a draw counts for it), else -1

    def get_next_state(self, state, action):
        own, opp = _lib.pack_board(state)
        sq = np.array([int(action[0]) * 8 + int(action[1])], np.uint8)
        o2, p2 = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        _lib.check(_lib.load().oz_rules_apply_moves(_lib.p_u64(np.array([own], np.uint64)), _lib.p_u64(np.array([opp], np.uint64)), _lib.p_u8(sq),
                                                    self._board_size, 1, _lib.p_u64(o2), _lib.p_u64(p2)))
        own, opp = int(o2[0]), int(p2[0])
        if self._legal_mask(opp, own):                         # the opponent can answer: it becomes the mover (channel 0); a pass keeps the orientation
            own, opp = opp, own
        nxt = _lib.unpack_board(own, opp, self._board_size)
        return nxt.astype(state.dtype) if isinstance(state, np.ndarray) and nxt.dtype != state.dtype else nxt      # the reference returns the input's dtype (np.copy + in-place flips)

    def _neural_network_predict(self, state):
        """one evaluation per distinct board of this search (the reference's per-instance dict, keyed by the exact board)"""
        seen = self.__dict__.setdefault("_predict_cache", {})
        key = _lib.pack_board(state)
        hit = seen.get(key)
        if hit is None:
            hit = seen[key] = self._neural_network.predict(OthelloGame.convert_to_one_channel_board(state) if self._one_channel else state)
        return hit

    def get_state_value(self, state):
        return self._neural_network_predict(state)[1]

    def get_state_actions_propabilities(self, state):          # (sic: the reference's spelling)
        return self._neural_network_predict(state)[0]

    def _mask_valid_moves(self, state):
        n = self._board_size
        legal = self._legal_mask(*_lib.pack_board(state))
        return np.array([[(legal >> (r * 8 + c)) & 1 for c in range(n)] for r in range(n)], dtype=np.float64)

    def moves_scaled_by_valid_moves(self, state):
        return self.get_state_actions_propabilities(state) * self._mask_valid_moves(state)

    # ---- inspection (parity tests)
    def dump(self):
        lib = _lib.load()
        nn = np.zeros(1, np.int32)
        _lib.check(lib.oz_mcts_num_nodes(self._h, _lib.p_i32(nn)))
        out = []
        for i in range(int(nn[0])):
            own, opp, legal, Ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
            N, Q, qt, P = np.zeros(64, np.int32), np.zeros(64, np.float64), np.zeros(64, np.uint8), np.zeros(64, np.float64)
            _lib.check(lib.oz_mcts_dump_node(self._h, 0, i, C.byref(own), C.byref(opp), C.byref(Ns), C.byref(legal),
                                             _lib.p_i32(N), _lib.p_f64(Q), _lib.p_u8(qt), _lib.p_f64(P)))
            out.append(dict(k0=own.value, k1=opp.value, Ns=Ns.value, legal=legal.value, N=N, Q=Q, qtag=qt, P=P))
        if self.proofs:
            for node, pr in zip(out, self.dump_proofs()):
                node["proofs"] = pr
        return out

    # ---- proofs (include/othellozero_amd.h, "proofs")
    def _need_proofs(self):
        if not self.proofs:
            raise ValueError("this search was created without proofs=True")

    def root_proof(self, state):
        """(val, edge) of the mover-canonical `state`: val = its proven value -1 / 0 / +1 for the player to move or None, edge = int8 (64,) by
        square with _lib.PROOF_UNKNOWN where nothing is proven.  KeyError if the state is unknown to the search."""
        self._need_proofs()
        own, opp = _lib.pack_board(state)
        self._set_root(own, opp)
        edge, val, rc = np.zeros((1, 64), np.int8), np.zeros(1, np.int8), np.zeros(1, np.int32)
        _lib.check(_lib.load().oz_mcts_root_proofs(self._h, _lib.p_i8(edge), _lib.p_i8(val), _lib.p_i32(rc)))
        if rc[0] != 0:
            raise KeyError("state is unknown to the search")
        return (None if val[0] == _lib.PROOF_UNKNOWN else int(val[0])), edge[0]

    def dump_proofs(self):
        """per node, in dump()'s order: dict(edge int8 (64,), value = the node's own value, val = val(S); _lib.PROOF_UNKNOWN = unknown)"""
        self._need_proofs()
        lib = _lib.load()
        nn = np.zeros(1, np.int32)
        _lib.check(lib.oz_mcts_num_nodes(self._h, _lib.p_i32(nn)))
        out = []
        for i in range(int(nn[0])):
            edge, value, val = np.zeros(64, np.int8), C.c_int8(), C.c_int8()
            _lib.check(lib.oz_mcts_dump_proofs(self._h, 0, i, _lib.p_i8(edge), C.byref(value), C.byref(val)))
            out.append(dict(edge=edge, value=value.value, val=val.value))
        return out

    def proof_stats(self):
        s = np.zeros(4, np.int64)
        _lib.check(_lib.load().oz_mcts_proof_stats(self._h, _lib.p_i64(s)))
        return dict(zip(_lib.PROOF_STATS, (int(x) for x in s)))

    def wide_stats(self):
        s = np.zeros(3, np.int64)
        _lib.check(_lib.load().oz_mcts_wide_stats(self._h, _lib.p_i64(s)))
        return dict(steps=int(s[0]), collisions=int(s[1]), leaves=int(s[2]))

    def stats(self):
        s = np.zeros(5, np.int64)
        _lib.check(_lib.load().oz_mcts_stats(self._h, _lib.p_i64(s)))
        return dict(simulations=int(s[0]), visits=int(s[1]), expansions=int(s[2]), terminal=int(s[3]), fallback=int(s[4]))
