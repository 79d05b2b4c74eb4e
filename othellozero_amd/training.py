"""Self-play drivers -- drop-in for training.py:13-72 plus the batched engine the reference lacks.

`execute_episode(...)` keeps the reference's signature, return layout and host-side random draws
(`random.random`, `np.random.choice`, `random.choice`) so existing callers (workers.py:83-84,
pickle_training.py:26-27) see the same behaviour; all rule / search / network work runs on the GPU.
`selfplay_batch(...)` is the MI355X-native path: thousands of games in lock step, resident in HBM,
counter-based RNG streams, one batched network evaluation per simulation step.
"""
import ctypes as C
import logging
import random

import numpy as np

from . import _lib
from .NNet import NeuralNets
from .Othello import BoardView, OthelloGame, OthelloPlayer
from .othelo_mcts import OthelloMCTS


def training_example_symmetries(board, policy):
    """training.py:13-23: 8 (board, policy) pairs, rot90 k=1..4 (CCW) each with fliplr first, then without."""
    symetric_examples = []
    for rotation in range(1, 5):
        for flip in (True, False):
            b, p = np.rot90(board, k=rotation), np.rot90(policy, k=rotation)
            if flip:
                b, p = np.fliplr(b), np.fliplr(p)
            symetric_examples.append((b, p))
    return symetric_examples


def execute_episode(board_size, neural_network, degree_exploration, num_simulations, policy_temperature, e_greedy,
                    q_mode=_lib.QMODE_F64, snapshot_boards=False, policy_target="onehot", target_temperature=1.0,
                    leaves_per_step=1, root_noise=None, noise_seed=0, sample_moves=None, sample_seed=0, solve_leaves=0,
                    forced_playouts=None, value_target="outcome", gumbel=None, gumbel_seed=0, value_signs="reference", proofs=False,
                    proof_play=False, selection=None, tree_gc="off", node_cap=0):
    """training.py:26-72.  Returns [(board (n,n,2) bool, one-hot policy (n,n) float64, z int), ...], 8 per move.

    gumbel=(max_considered, c_visit, c_scale) or True: every move's search is a Gumbel root search of num_simulations simulations
    (OthelloMCTS.sample_gumbel before them, keyed (gumbel_seed, 0, ply) with ply = the moves played so far), and the greedy branch of the coin
    plays the Gumbel root's move; the explore branch is unchanged.  policy_target="improved" (needs gumbel and snapshot_boards=True) stores the
    search's float32 improved policy (OthelloMCTS.gumbel_policy).  It replaces root_noise, forced_playouts and sample_moves; not with
    leaves_per_step > 1.  None is the function without it.

    snapshot_boards=False reproduces the reference exactly, including its aliasing quirk: the
    returned boards are views of the live game array, so every example shows the FINAL position.  Pass
    snapshot_boards=True to store the position at the time of the move instead (what training wants).

    policy_target="visits" stores the search's visit distribution instead of the one-hot of the move played (the AlphaZero
    pi): mcts.get_policy_action_probabilities(state, target_temperature) at every move.  With target_temperature > 0 that
    call draws no random number, so moves and random streams are those of the default "onehot".

    leaves_per_step > 1: that many descents per network batch under virtual loss (OthelloMCTS); a native network only.

    root_noise=(alpha, epsilon): Dirichlet noise on the root prior, drawn on the device once per move before that move's simulations, keyed
    (noise_seed, 0, ply) with ply = the moves played so far; None is the function without it.

    sample_moves=(temperature, plies): where the coin falls on the greedy branch, the move of a ply < plies is drawn on the device in proportion
    to N ** (1 / temperature) (OthelloMCTS.sample_action), keyed (sample_seed, 0, ply), instead of taken as the arg-max; None is the function
    without it.

    solve_leaves=E > 0: the search takes the exact win / draw / loss of a leaf with at most E empties in place of the network's value
    (OthelloMCTS); a native network only.

    forced_playouts=k > 0 (needs root_noise): KataGo's forced playouts in every move's search, and with policy_target="visits" the stored
    distribution is that of the pruned counts (OthelloMCTS.pruned_counts); the move is still chosen from the raw counts.

    value_target=("blend", w) / ("td", lam): every move's root value (OthelloMCTS.root_value) is recorded and z is the float value target of the
    move (agents.rules_value_targets) instead of the int outcome; needs snapshot_boards=True (a search value belongs to the position of its
    move).  "outcome" is the function without it.

    value_signs="sound": the search backs its values up with the signs right across passes and finished boards (OthelloMCTS); "reference" is
    the function without it.

    proofs=True (needs value_signs="sound"): the search keeps exact values as proofs and backs them up the tree (OthelloMCTS); not with
    gumbel or forced_playouts.

    proof_play=True (needs proofs=True): the policy the move is taken from, the sampled move, the "visits" target and the recorded root
    value are those the root's proofs leave (OthelloMCTS.proven_counts / root_value(proven=True)); the explore branch is unchanged.

    selection=dict(fpu=, cpuct_growth=, prior_first=): the selection rule of the search (OthelloMCTS); not with gumbel or forced_playouts.

    tree_gc="demand" | "every": the search drops the nodes the game has passed (OthelloMCTS); the examples are those of "off".  node_cap > 0:
    the search's node capacity in place of a whole game's nodes -- what the option makes sufficient."""
    _lib.check_tree_gc(tree_gc)
    _lib.check_selection(selection, gumbel=gumbel, forced_playouts=forced_playouts)
    _lib.check_value_signs(value_signs)
    _lib.check_proofs(proofs, value_signs, gumbel=gumbel, forced_playouts=forced_playouts)
    proof_play = _lib.check_proof_play(proof_play, proofs)
    pp = {"proven": True} if proof_play else {}
    vt_mode, _ = _lib.check_value_target(value_target, not snapshot_boards)
    root_values, movers, positions = [], [], []
    solve_leaves = _lib.check_solve_leaves(solve_leaves)
    root_noise = _lib.check_root_noise(root_noise)
    forced_playouts = _lib.check_forced_playouts(forced_playouts, root_noise)
    sample_moves = _lib.check_sample_moves(sample_moves)
    gumbel = _lib.check_gumbel_options(gumbel, root_noise=root_noise, forced_playouts=forced_playouts, sample_moves=sample_moves,
                                       leaves_per_step=leaves_per_step)
    assert policy_target in ("onehot", "visits", "improved"), policy_target
    if policy_target == "improved" and gumbel is None:
        raise ValueError("policy_target='improved' needs gumbel=(max_considered, c_visit, c_scale)")
    if policy_target == "improved" and not snapshot_boards:
        raise ValueError("policy_target='improved' needs snapshot_boards=True: an improved policy belongs to the position of its move")
    if policy_target == "visits" and not target_temperature > 0:
        raise ValueError(f"target_temperature must be > 0 for visit-count targets (got {target_temperature})")
    examples = []
    game = OthelloGame(board_size)
    mcts = OthelloMCTS(board_size, neural_network, degree_exploration, q_mode=q_mode,
                       node_cap=int(node_cap) if node_cap else num_simulations * (board_size * board_size - 3) + 64, leaves_per_step=leaves_per_step,
                       solve_leaves=solve_leaves, forced_playouts=forced_playouts, **({"gumbel": gumbel} if gumbel is not None else {}),
                       **_lib.search_kw(dict(value_signs=value_signs, proofs=proofs, proof_play=proof_play, selection=selection, tree_gc=tree_gc)))
    # training.py:34-37 (BNN examples are one-channel boards, a fresh array per round: no aliasing for them)
    board_view_type = BoardView.ONE_CHANNEL if getattr(neural_network.network_type, "name", "") == "BNN" else BoardView.TWO_CHANNELS

    while not game.has_finished():
        state = game.board(BoardView.TWO_CHANNELS)
        if root_noise is not None:
            mcts.sample_root_noise(root_noise[0], root_noise[1], noise_seed, 0, len(examples) // 8, state=state, player=game.current_player)
        if gumbel is not None:
            mcts.sample_gumbel(num_simulations, gumbel_seed, 0, len(examples) // 8, state=state, player=game.current_player)
        mcts.simulate_n(state, game.current_player, num_simulations)
        if game.current_player == OthelloPlayer.WHITE:
            state = OthelloGame.invert_board(state)
        policy = mcts.get_policy_action_probabilities(state, policy_temperature, **pp)
        if vt_mode != _lib.VALUE_TARGET_OUTCOME:
            root_values.append(mcts.root_value(state, **pp))
            movers.append(game.current_player.value)
            positions.append(_lib.pack_board(game.board(BoardView.TWO_CHANNELS)))

        coin = random.random()                      # e-greedy, training.py:51-56
        if coin <= e_greedy:
            action = np.argwhere(policy == policy.max())[0]
            if gumbel is not None:
                action = mcts.gumbel_policy(state)[0]
            if sample_moves is not None and len(examples) // 8 < sample_moves[1]:
                action = mcts.sample_action(state, sample_moves[0], sample_seed, 0, len(examples) // 8, **pp)
        else:
            actions = mcts.get_state_actions(state)
            action = actions[np.random.choice(len(actions))]

        action_choosed = np.zeros((board_size, board_size))
        action_choosed[action[0]][action[1]] = 1
        if policy_target == "improved":
            action_choosed = mcts.gumbel_policy(state)[1]
        if policy_target == "visits":
            action_choosed = mcts.get_policy_action_probabilities(state, target_temperature, pruned=forced_playouts > 0.0, **pp)
        board_now = game.board(board_view_type)
        if snapshot_boards:
            board_now = np.copy(board_now)
        for board_example, policy_example in training_example_symmetries(board_now, action_choosed):
            examples.append((board_example, policy_example, game.current_player))
        game.play(*action)

    winner, winner_points = game.get_winning_player()
    logging.info(f'Episode finished: The winner obtained {winner_points} points.')
    if vt_mode != _lib.VALUE_TARGET_OUTCOME:
        from .agents import rules_value_targets
        rec = np.zeros(len(movers), _lib.RECORD_DTYPE)
        rec["ply"] = np.arange(len(movers))
        rec["player"] = movers
        rec["z"] = [1 if winner.value == p else -1 for p in movers]
        rec["black"], rec["white"] = [b for b, _ in positions], [w for _, w in positions]
        targets = rules_value_targets(rec, root_values, board_size, value_target)
        return [(state, policy, float(targets[i // 8])) for i, (state, policy, _player) in enumerate(examples)]
    return [(state, policy, 1 if winner == player else -1) for state, policy, player in examples]


def duel_between_neural_networks(board_size, neural_network_1, neural_network_2, degree_exploration, num_simulations,
                                 fixed=False):
    """One game, neural_network_1 as BLACK against neural_network_2 (the name workers.py:14-15 and pickle_training.py:36 import;
    reference body: training.py:75-88).  What the reference really does is play the game and then fail: it looks the whole
    `(agent, points)` result of duel_between_agents up in a dict keyed by agent, i.e. KeyError -- recorded from a run of the
    reference in tests/golden/drivers_misc.json and reproduced here.  fixed=True returns what was meant: 0 if the first
    network won, 1 otherwise."""
    from .agents import NeuralNetworkOthelloAgent, duel_between_agents
    board = OthelloGame(board_size)
    black, white = (NeuralNetworkOthelloAgent(board, net, num_simulations, degree_exploration)
                    for net in (neural_network_1, neural_network_2))
    outcome = duel_between_agents(board, black, white)          # (winning agent, its points)
    if not fixed:
        raise KeyError(outcome)
    return 0 if outcome[0] is black else 1


def evaluate_neural_network(board_size, total_iterations, neural_network, num_simulations, degree_exploration,
                            agent_class, agent_arguments, fixed=False):
    """`total_iterations` games of the network's search agent against agent_class(game, *agent_arguments); returns the number
    of games counted as won (reference body: training.py:91-118, imported by workers.py:14-15).  Colours come from one
    random.shuffle of [opponent, network] per game, as there.  The reference compares the `(agent, points)` result with
    the agent itself, so it never counts a win and returns 0 (tests/golden/drivers_misc.json); fixed=True compares the agent."""
    from .agents import NeuralNetworkOthelloAgent, duel_between_agents
    wins = 0
    for _ in range(total_iterations):
        board = OthelloGame(board_size)
        ours = NeuralNetworkOthelloAgent(board, neural_network, num_simulations, degree_exploration)
        seats = [agent_class(board, *agent_arguments), ours]
        random.shuffle(seats)
        victor, _points = duel_between_agents(board, *seats)
        wins += int(fixed and victor is ours)
    logging.info(f'Neural Network Evaluation: {wins} of {total_iterations} games counted as won')
    return wins


# ---------------------------------------------------------------- batched engine
# SelfPlayEngine.records(): flag, C entry, dtype of each array the entry fills, shape of a row -- the weights are the one entry that fills
# three arrays, which come back as one tuple
_RECORD_ROWS = (("with_visits", "oz_selfplay_visits", (np.int32,), (64,)), ("with_values", "oz_selfplay_values", (np.float64,), ()),
                ("with_targets", "oz_selfplay_targets", (np.float32,), ()), ("with_policies", "oz_selfplay_policies", (np.float32,), (64,)),
                ("with_surprise", "oz_selfplay_surprises", (np.float64,), ()),
                ("with_weights", "oz_selfplay_weights", (np.float32, np.int32, np.uint8), ()))
_POINTER = {np.int32: _lib.p_i32, np.float32: _lib.p_f32, np.float64: _lib.p_f64, np.uint8: _lib.p_u8}


class SelfPlayEngine:
    """num_games concurrent execute_episode instances on one GPU (C ABI: oz_selfplay_*)."""

    def __init__(self, neural_network, board_size=8, num_games=4096, num_simulations=100, degree_exploration=1.0,
                 policy_temperature=1.0, e_greedy=0.9, seed=1234, first_game_id=0, game_id_stride=0,
                 q_mode=_lib.QMODE_F64, refill=False, node_cap=0, record_cap=0, dedup=True, batch_cap=0, eval_cache=False,
                 record_visits=False, leaves_per_step=1, root_noise=None, sample_moves=None, solve_leaves=0, playout_cap=None,
                 forced_playouts=None, record_values=False, gumbel=None, record_surprise=False, resign=None, value_signs="reference", proofs=False,
                 proof_play=False, selection=None, tree_gc="off"):
        """dedup: cross-game leaf de-duplication (a board several games reach in one batch is evaluated once; no record changes);
        batch_cap: leaves per network batch of the free-running driver (0 = none; see preferred_batch_cap);
        eval_cache: take (pi, v) of boards the network has evaluated before from its persistent cache (NNetWrapper.set_eval_cache) --
        the reference's per-search _predict_cache (othelo_mcts.py:82-88) across batches, games and refilled slots; no record changes;
        record_visits: keep every recorded move's root visit counts (records(with_visits=True)) -- the policy targets of
        expand_examples(visits=...); 16 KB per slot + 256 B per record of device memory, no record changes;
        leaves_per_step > 1: that many descents per game and network batch under virtual loss (oz_mcts_set_leaves_per_step) for run() /
        stagger(); the network needs max_batch >= num_games * leaves_per_step; run_steps() then raises; dedup and eval_cache then have no
        effect (every leaf is evaluated) and run(sync=False) still waits once per move round.  Not the reference's search order.
        root_noise=(alpha, epsilon): every searched move draws Dirichlet(alpha) noise over its root's legal moves on the device, keyed
        (seed, game id, ply), and its descents see (1 - epsilon) P + epsilon eta at the root (oz_selfplay_set_root_noise); stored priors and
        the records' layout do not change.
        sample_moves=(temperature, plies): where the coin falls on the greedy branch, the move of a game whose ply < plies is drawn in
        proportion to N ** (1 / temperature), keyed (seed, game id, ply), instead of taken as the arg-max (oz_selfplay_set_move_sampling);
        such a record has greedy == 2.  run(), run_steps() and stagger() alike; later plies and the explore branch are unchanged.
        solve_leaves=E > 0: in every search a leaf with at most E empties takes its exact win / draw / loss (+1 / 0 / -1 for the side to
        move) in place of the network's value, solved on the device right after the network's batch (oz_selfplay_set_solve_leaves); the
        priors stay the network's and its evaluation cache keeps the network's value.  Every driver, any leaves_per_step.  rows_solved()
        counts them.  Not the reference's search.
        playout_cap=(fast_sims, full_prob): KataGo's playout cap randomization (oz_selfplay_set_playout_cap).  A searched move runs
        num_simulations simulations with probability full_prob and fast_sims (2 .. num_simulations) otherwise, drawn per (seed, game id, ply);
        a fast move draws no root noise, and its record carries the flag _lib.record_fast reads: the record consumers (expand_examples,
        loop.examples_from_records, ReplayBuffer.append_*) train on the fully searched moves only, while every game still ends in an outcome
        for them.  run() at any leaves_per_step and run_steps() alike; stagger()'s rounds are not capped; playout_stats() counts the moves.
        full_prob = 1 plays the games of the engine without the option.  Measured at (20, 0.25), 4 096 games of 8x8 at 100 simulations:
        1.89 times the finished games per second, 0.51 times the fully searched records per second ("Playout cap").
        forced_playouts=k > 0 (None or 0 = off; needs root_noise): KataGo's forced playouts and policy target pruning
        (oz_selfplay_set_forced_playouts).  At the noisy root a child tried once is searched until it has sqrt(k * Pn * Ns) visits, and with
        record_visits the rows of records(with_visits=True) hold the PRUNED counts -- the visits PUCT would not have granted are taken out, a
        child cut down to one visit is dropped -- so everything downstream (expand_examples, the replay buffers) trains on what the search
        concluded.  last_counts() and the moves stay on the raw counts.  run(), run_steps() and stagger() alike; the fast moves of a playout
        cap are neither forced nor pruned.  forced_playout_stats() counts ("Forced playouts").
        record_values=True: keep every recorded move's root value -- the visit-weighted mean of the root's Q over the raw counts, for the player
        to move (oz_selfplay_set_record_values) -- for records(with_values=True) and value_targets(); 512 B per slot + 8 B per record of device
        memory, no record changes.  Every driver ("Value targets").
        gumbel=(max_considered, c_visit, c_scale) or True (= (16, 50.0, 1.0)): the root search of Gumbel AlphaZero for every searched move of
        run() (oz_selfplay_set_gumbel): the root samples max_considered moves without replacement with Gumbel noise drawn on the device, keyed
        (seed, game id, ply), spends num_simulations on them by sequential halving, and the greedy branch of the coin plays the root's move
        (greedy == 3 in its record; pure Gumbel: e_greedy = 1).  The engine keeps the float32 improved-policy row softmax(logit + sigma(completed
        Q)) of every searched move: records(with_policies=True), the targets of loop.examples_from_records(policies=...).  16 KB per slot +
        256 B per record.  It replaces root_noise, forced_playouts and sample_moves, and does not combine with playout_cap or
        leaves_per_step > 1 (ValueError); run_steps() and stagger() then raise.  gumbel_stats() counts ("Gumbel search").
        record_surprise=True (needs record_visits=True or gumbel=...): keep every recorded move's policy surprise KL(q || p), q the row that
        becomes its policy target and p the root's stored priors (oz_selfplay_set_record_surprise), for records(with_surprise=True) and
        surprise_weights(); 512 B per slot + 8 B per record, no record changes.  Every driver ("Policy surprise weighting").
        resign=(v, r, min_ply, keep_prob): resignation with a played-out audit share (oz_selfplay_set_resign); switches record_values on.
        After every searched move the root value, seen from BLACK, is held against +-v; once it has stayed at or beyond the same bound for r
        moves in a row and the ply is at least min_ply, the game stops after that move and goes to that side: its records carry z for that
        winner, the board at the stop as their final board and the flag _lib.record_adjudicated reads; a refilled slot starts its next game
        at once.  A share keep_prob of the games, drawn per (seed, game id), is played out regardless: resign_stats() counts how often the
        rule triggered in them and how often it was wrong.  The record consumers take an adjudicated record as any other (with
        alias_final=True the "final board" of such a game is the board at the stop).  run() at any leaves_per_step, with every option but
        gumbel (ValueError); run_steps() and stagger() then raise.  keep_prob = 1 plays the games of the engine without the option
        ("Resignation").
        value_signs="sound": every search of the engine backs its values up with the signs right across passes and finished boards -- one
        negation per change of the side to move, a finished board worth the sign of its disc difference to the side to move there, a draw 0
        (oz_selfplay_set_value_signs).  "reference" (the default) is the reference's rule.  Every driver and every option; the root values,
        value targets, recorded surprise and the resign rule read what the search stores.  A drawn game stays +-1 (draw -> BLACK) in the
        records' z ("Value signs").
        proofs=True (needs value_signs="sound"): every search keeps exact values -- finished boards, solved leaves, what was proven from
        them -- as proofs and backs them up the tree; a descent never picks a proven loss while something else is left, takes the exact
        value in place of the averaged Q and stops at a proven position (oz_selfplay_set_proofs).  run() / play_to_end() at any
        leaves_per_step with every option but gumbel and forced_playouts (ValueError); run_steps() and stagger() then raise.  The moves, the
        visit rows and the root values read the raw statistics as before.  proof_stats() counts ("Proofs").
        proof_play=True (needs proofs=True): the move, the recorded visit row and the recorded root value take what the root's proofs know
        (oz_selfplay_set_proof_play): the row keeps the raw counts of the moves the descent would still pick at the root -- those that prove
        a known value, else those not proven lost -- and every move rule that reads counts reads that row; the root value is the exact one
        where it is known; the record carries the proof code _lib.record_proven reads.  The explore branch of the coin and last_counts()
        stay as they are.  proof_play_stats() counts; proof_targets() makes z of the proven records exact ("Proof play").
        selection=dict(fpu=(reduction, root_reduction), cpuct_growth=(base, factor), prior_first=bool), every key optional: every search
        of the engine values an unvisited move at the node's running value minus a reduction in place of 0, lets the exploration constant
        grow with the node's visits and sends a fresh node's first visit where the prior points (oz_selfplay_set_selection;
        include/othellozero_amd.h, "selection").  run() / play_to_end() at any leaves_per_step with every option but gumbel and
        forced_playouts (ValueError); run_steps() and stagger() then raise.  Records, rows and targets read what the search stores
        ("Selection").
        tree_gc="demand" | "every" ("off" is the default): drop the stored nodes a slot's game has passed -- those that are not the root and
        hold no more discs than it, which no descent can reach again -- right after the round's roots are set (oz_selfplay_set_tree_gc;
        include/othellozero_amd.h, "tree collection").  No record, row or counter changes; node_cap can be far below a whole game's nodes.
        "demand" collects a slot only when num_simulations more nodes might not fit, "every" every slot every round (diagnostic).  run() /
        play_to_end() with every option; run_steps() and stagger() then raise.  tree_gc_stats() counts ("Tree collection")."""
        o = _lib.check_selfplay_options(num_simulations, record_visits, leaves_per_step, root_noise, sample_moves, solve_leaves, playout_cap,
                                        forced_playouts, record_values, gumbel, record_surprise, resign, value_signs, proofs, proof_play, selection,
                                        tree_gc)
        lib = _lib.require_gpu()
        assert getattr(neural_network, "_h", None) is not None, "SelfPlayEngine needs a native NNetWrapper / StubNetWrapper"
        self.net = neural_network
        self.cfg = _lib.SelfplayConfig(
            n=board_size, num_games=num_games, sims=num_simulations, q_mode=q_mode, c=float(degree_exploration),
            temperature=float(policy_temperature), e_greedy=float(e_greedy), seed=seed, first_game_id=first_game_id,
            game_id_stride=game_id_stride, refill=1 if refill else 0, node_cap=node_cap,
            record_cap=record_cap, dedup=_lib.DEDUP_ON if dedup else _lib.DEDUP_OFF, batch_cap=int(batch_cap),
            eval_cache=1 if eval_cache else 0, record_visits=1 if record_visits else 0)
        self._h = C.c_void_p()
        _lib.check(lib.oz_selfplay_create(C.byref(self._h), C.byref(self.cfg), neural_network._h))
        self.n, self.num_games = board_size, num_games
        self.value_signs, self.proofs, self.proof_play, self.tree_gc = o["value_signs"], o["proofs"], o["proof_play"], o["tree_gc"]
        selection = _lib.check_selection(o["selection"])                  # (the library's form of it: flags and four numbers)
        self.selection = _lib.selection_dict(selection)
        self.leaves_per_step = int(leaves_per_step)
        self.root_noise, self.sample_moves, self.solve_leaves, self.playout_cap = o["root_noise"], o["sample_moves"], o["solve_leaves"], o["playout_cap"]
        self.forced_playouts, self.gumbel, self.resign = o["forced_playouts"], o["gumbel"], o["resign"]
        self.record_values = o["record_values"] or self.resign is not None
        self.record_surprise = o["record_surprise"]
        self.endgame_stats = self.value_target_stats = self.proof_target_stats = None       # play_to_end's, where it ran them
        for armed, setter, args in (                                      # (the library sees the options in this order)
                (self.value_signs != "reference", lib.oz_selfplay_set_value_signs, (_lib.VALUE_SIGNS[self.value_signs],)),
                (self.proofs, lib.oz_selfplay_set_proofs, (1,)),
                (self.proof_play, lib.oz_selfplay_set_proof_play, (1,)),
                (selection[0], lib.oz_selfplay_set_selection, selection),
                (self.leaves_per_step != 1, lib.oz_selfplay_set_leaves_per_step, (self.leaves_per_step,)),
                (self.root_noise is not None, lib.oz_selfplay_set_root_noise, self.root_noise),
                (self.sample_moves is not None, lib.oz_selfplay_set_move_sampling, self.sample_moves),
                (self.solve_leaves, lib.oz_selfplay_set_solve_leaves, (self.solve_leaves,)),
                (self.playout_cap is not None, lib.oz_selfplay_set_playout_cap, self.playout_cap),
                (self.forced_playouts > 0.0, lib.oz_selfplay_set_forced_playouts, (self.forced_playouts,)),
                (self.record_values, lib.oz_selfplay_set_record_values, (1,)),
                (self.gumbel is not None, lib.oz_selfplay_set_gumbel, self.gumbel),
                (self.record_surprise, lib.oz_selfplay_set_record_surprise, (1,)),
                (self.resign is not None, lib.oz_selfplay_set_resign, self.resign),
                (self.tree_gc != "off", lib.oz_selfplay_set_tree_gc, (_lib.TREE_GC[self.tree_gc],))):
            if armed:
                _lib.check(setter(self._h, *args))

    def option_stats(self):
        """The statistics of the options this engine was created with, under the names selfplay_batch and loop.training publish them by:
        rows_solved, playout_stats, forced_playout_stats, resign_stats, gumbel_stats, proof_stats, proof_play_stats and tree_gc_stats are
        what the methods of those names return now; endgame_stats, value_target_stats and proof_target_stats what play_to_end's
        solve_records(), value_targets() and proof_targets() returned.  None for an option that is off."""
        on = dict(rows_solved=self.solve_leaves, playout_stats=self.playout_cap is not None, forced_playout_stats=self.forced_playouts > 0.0,
                  resign_stats=self.resign is not None, gumbel_stats=self.gumbel is not None, proof_stats=self.proofs,
                  proof_play_stats=self.proof_play, tree_gc_stats=self.tree_gc != "off")
        return dict({name: getattr(self, name)() if armed else None for name, armed in on.items()}, endgame_stats=self.endgame_stats,
                    value_target_stats=self.value_target_stats, proof_target_stats=self.proof_target_stats)

    def tree_gc_stats(self):
        """dict(mode, collections, nodes_before_sum, nodes_kept_sum, peak_nodes, peak_kept): the tree collection that is set and, since it was
        armed, the collections run, the node counts before and after them in sum, the largest node count a slot had at the start of a
        round and the largest it had after a collection -- peak_kept + num_simulations is the node_cap these games need under "demand"
        (zeros without tree_gc)"""
        mode, st = C.c_int(), _lib.TreeGcStats()
        _lib.check(_lib.load().oz_selfplay_get_tree_gc(self._h, C.byref(mode), C.byref(st)))
        return dict(mode={v: k for k, v in _lib.TREE_GC.items()}[mode.value], **_lib.tree_gc_stats_dict(st))

    def tree_gc_profile(self, enable=True):
        """HIP-event timing of the collection launches on / off (tree_gc_profile_read)"""
        _lib.check(_lib.load().oz_selfplay_tree_gc_profile(self._h, 1 if enable else 0))

    def tree_gc_profile_read(self, reset=False):
        """(milliseconds in total, launches) of the collection launches timed so far; waits for the stream"""
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(_lib.load().oz_selfplay_tree_gc_profile_read(self._h, C.byref(ms), C.byref(cnt), 1 if reset else 0))
        return ms.value, cnt.value

    def proof_stats(self):
        """dict(edges_proven, edge_stops, node_stops, roots_proven) over the engine's games so far: edges given a proof, descents ended on a
        proven edge / on a proven node, roots whose value became known (zeros without proofs=True)"""
        s = np.zeros(4, np.int64)
        _lib.check(_lib.load().oz_selfplay_proof_stats(self._h, _lib.p_i64(s)))
        return dict(zip(_lib.PROOF_STATS, (int(x) for x in s)))

    def proof_play_stats(self):
        """dict(proven_roots, rows_changed, moves_changed, fallbacks) over the engine's searched moves so far: those on a root whose value
        is known, those whose recorded row differs from the raw counts, those whose greedy or sampled action differs from the one the raw
        counts give, and those whose candidates were all unvisited (zeros without proof_play=True)"""
        s = np.zeros(4, np.int64)
        _lib.check(_lib.load().oz_selfplay_proof_play_stats(self._h, _lib.p_i64(s)))
        return dict(zip(_lib.PROOF_PLAY_STATS, (int(x) for x in s)))

    def proof_targets(self, first_record=0):
        """oz_selfplay_proof_targets: the completed records from `first_record` on that carry a proof code get z = the proven sign for their
        mover (a proven draw follows z's convention: BLACK's win), in place on the device; idempotent.  Run it before solve_records(),
        value_targets() and the replay appends.  -> dict(records, proven, z_changed)."""
        s = _lib.ProofTargetStats()
        _lib.check(_lib.load().oz_selfplay_proof_targets(self._h, int(first_record), C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    def resign_stats(self):
        """dict(v, r, min_ply, keep_prob, games_adjudicated, adjudicated_plies_sum, games_exempt, exempt_triggered, exempt_wrong,
        exempt_trigger_ply_sum): the resignation rule that is set (r 0 = off) and, since it was armed, the games it ended and the plies they
        were played for, and of the exempt games completed how many triggered the rule, how many of those the natural winner proved wrong,
        and the plies of their first triggers in sum.  exempt_wrong / exempt_triggered is the rule's false-positive rate."""
        v, r, m, kp, s = C.c_double(), C.c_int(), C.c_int(), C.c_double(), _lib.ResignStats()
        _lib.check(_lib.load().oz_selfplay_get_resign(self._h, C.byref(v), C.byref(r), C.byref(m), C.byref(kp), C.byref(s)))
        return dict(v=v.value, r=r.value, min_ply=m.value, keep_prob=kp.value, **{k: int(getattr(s, k)) for k, _ in s._fields_})

    def surprise_weights(self, frac, seed, first_record=0):
        """oz_selfplay_surprise_weights: weights, copy counts and first symmetries of the completed records from `first_record` on, computed
        on the device (records(with_weights=True), ReplayBuffer.append_engine(surprise_weight=...)); the records are not touched.  A fully
        searched record of a game with K of them gets w = (1 - frac) + frac s K / S, a fast record 0; it becomes floor(8 w + u) examples,
        u and the first symmetry drawn per (seed, game id, ply).  frac in (0, 1] (KataGo: 0.5).  Needs record_surprise=True.
        -> dict(records, full_records, examples, zero_copies, max_copies)."""
        frac = _lib.check_surprise_frac(frac, "surprise_weights")
        s = _lib.SurpriseWeightStats()
        _lib.check(_lib.load().oz_selfplay_surprise_weights(self._h, int(first_record), frac, int(seed) & (2 ** 64 - 1), C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    def gumbel_stats(self):
        """dict(max_considered, c_visit, c_scale, moves): the Gumbel search that is set (max_considered 0 = off) and the moves the Gumbel rule
        has picked so far (the records with greedy == 3, those of games still in progress included)"""
        m, cv, cs, moves = C.c_int32(), C.c_double(), C.c_double(), C.c_int64()
        _lib.check(_lib.load().oz_selfplay_get_gumbel(self._h, C.byref(m), C.byref(cv), C.byref(cs), C.byref(moves)))
        return dict(max_considered=m.value, c_visit=cv.value, c_scale=cs.value, moves=moves.value)

    def last_gumbel(self):
        """(g float64 (num_games, 64) by square, armed uint8 (num_games,), N0 int32 (num_games, 64)) of the searches of the last move round"""
        G = self.num_games
        g, armed, n0 = np.zeros((G, 64), np.float64), np.zeros(G, np.uint8), np.zeros((G, 64), np.int32)
        _lib.check(_lib.load().oz_selfplay_gumbel(self._h, _lib.p_f64(g), _lib.p_u8(armed), _lib.p_i32(n0)))
        return g, armed, n0

    def value_targets(self, value_target, exact_empties=0, first_record=0, exact_proven=False):
        """oz_selfplay_value_targets: the value targets of the completed records from `first_record` on, computed on the device into the
        engine's float32 targets (records(with_targets=True), ReplayBuffer.append_engine(value_target=...)); the records are not touched.
        value_target = "outcome", ("blend", w): (1 - w) z + w q, or ("td", lam): TD(lam) over the root values of the following plies, ending
        in the outcome.  exact_empties=E > 0 (after solve_records(E)): a record with at most E empties keeps its exact z and restarts the
        chain.  exact_proven=True (after proof_targets()): a record with a proof code does the same (oz_selfplay_value_targets_x).  Needs
        record_values=True.  -> dict(records, exact, sign_changed)."""
        mode, param = _lib.check_value_target(value_target)
        exact_empties = _lib.check_solve_empties(exact_empties, 0, "exact_empties")
        s = _lib.ValueTargetStats()
        if exact_proven:
            _lib.check(_lib.load().oz_selfplay_value_targets_x(self._h, int(first_record), mode, param, exact_empties, 1, C.byref(s)))
        else:
            _lib.check(_lib.load().oz_selfplay_value_targets(self._h, int(first_record), mode, param, exact_empties, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    def forced_playout_stats(self):
        """dict(k, moves_pruned, visits_raw, visits_kept): the forcing constant that is set (0 = off), the moves whose recorded row differs
        from their raw counts, and the visits before / after pruning summed over every move pruning ran on (the moves with a noisy root)"""
        k, moves, raw, kept = C.c_double(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.load().oz_selfplay_get_forced_playouts(self._h, C.byref(k), C.byref(moves), C.byref(raw), C.byref(kept)))
        return dict(k=k.value, moves_pruned=moves.value, visits_raw=raw.value, visits_kept=kept.value)

    def playout_stats(self):
        """dict(fast_sims, full_prob, full_moves, fast_moves): the playout cap that is set (fast_sims 0 = none) and the moves run() /
        run_steps() have played under it so far"""
        fs, p, full, fast = C.c_int(), C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(_lib.load().oz_selfplay_get_playout_cap(self._h, C.byref(fs), C.byref(p), C.byref(full), C.byref(fast)))
        return dict(fast_sims=fs.value, full_prob=p.value, full_moves=full.value, fast_moves=fast.value)

    def set_solve_leaves(self, max_empties):
        """solved leaves on (E > 0) / off (0) from the next search step on"""
        max_empties = _lib.check_solve_leaves(max_empties)
        _lib.check(_lib.load().oz_selfplay_set_solve_leaves(self._h, max_empties))
        self.solve_leaves = max_empties

    def solve_leaves_profile(self, enable=True):
        """HIP-event timing of the solving kernel on the launch stream (tools/solve_leaves_bench.py)"""
        _lib.check(_lib.load().oz_selfplay_solve_leaves_profile(self._h, 1 if enable else 0))

    def solve_leaves_profile_read(self, reset=False):
        """(ms_total, launches) of the solving kernel since the last reset"""
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(_lib.load().oz_selfplay_solve_leaves_profile_read(self._h, C.byref(ms), C.byref(cnt), 1 if reset else 0))
        return ms.value, cnt.value

    def rows_solved(self):
        """leaves the engine's searches have given their exact value so far"""
        e, rows = C.c_int(), C.c_int64()
        _lib.check(_lib.load().oz_selfplay_get_solve_leaves(self._h, C.byref(e), C.byref(rows)))
        return rows.value

    def __del__(self):
        try:
            if self._h:
                _lib.load().oz_selfplay_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def run(self, rounds=1, sync=True):
        """`rounds` move rounds: every live game runs num_simulations simulations and plays one move."""
        _lib.check(_lib.load().oz_selfplay_run(self._h, int(rounds)))
        if sync:
            self.sync()

    def run_steps(self, steps, sync=True):
        """free-running form of run(): `steps` network batches; every live game plays on by itself (its move when the
        simulations of the move are complete, simulations that need no network, the next first-visit leaf), so batches stay
        full; per game the simulations / moves / records are exactly those of run()"""
        _lib.check(_lib.load().oz_selfplay_run_steps(self._h, int(steps)))
        if sync:
            self.sync()

    def set_batch_cap(self, cap):
        """free-running driver: at most `cap` leaves per network batch (0 = no cap); a leaf that finds no slot waits for the next batch,
        the slot order rotates so that every game is served.  Records do not change; the launches become whole grid rounds at the right
        cap (see `preferred_batch_cap`)"""
        _lib.check(_lib.load().oz_selfplay_set_batch_cap(self._h, int(cap)))

    def set_dedup(self, enable):
        """cross-game leaf de-duplication on / off from the next batch on"""
        _lib.check(_lib.load().oz_selfplay_set_dedup(self._h, 1 if enable else 0))

    def stagger(self, sims_pre=None, sync=True):
        """continuous self-play (refill=True), first call only: advance slot g (g * P) // num_games plies into its first game
        (P = n*n - 4) by searched moves at `sims_pre` simulations each (default: num_simulations), so that the engine holds
        games at every stage like a long-running service and every later move round completes about num_games / P games"""
        _lib.check(_lib.load().oz_selfplay_stagger(self._h, int(sims_pre or self.cfg.sims)))
        if sync:
            self.sync()

    def profile(self, enable=True):
        """HIP-event timing of the tree kernels on the launch stream (the evaluator's launches are always timed)"""
        _lib.check(_lib.load().oz_selfplay_profile(self._h, 1 if enable else 0))

    def profile_read(self, reset=False):
        """{kernel: (ms_total, launches)} for _lib.TREE_KERNELS"""
        k = len(_lib.TREE_KERNELS)
        ms, cnt = np.zeros(k, np.float64), np.zeros(k, np.int64)
        _lib.check(_lib.load().oz_selfplay_profile_read(self._h, _lib.p_f64(ms), _lib.p_i64(cnt), 1 if reset else 0))
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(_lib.TREE_KERNELS)}

    def sync(self):
        _lib.check(_lib.load().oz_selfplay_sync(self._h))

    def stats(self):
        s = _lib.SelfplayStats()
        _lib.check(_lib.load().oz_selfplay_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def state(self):
        G = self.num_games
        b, w, gid = np.zeros(G, np.uint64), np.zeros(G, np.uint64), np.zeros(G, np.uint64)
        p, f, ply = np.zeros(G, np.int8), np.zeros(G, np.uint8), np.zeros(G, np.int32)
        _lib.check(_lib.load().oz_selfplay_state(self._h, _lib.p_u64(b), _lib.p_u64(w), _lib.p_i8(p), _lib.p_u8(f),
                                                 _lib.p_i32(ply), _lib.p_u64(gid)))
        return dict(black=b, white=w, player=p, finished=f, ply=ply, game_id=gid)

    def last_root_noise(self):
        """(eta float64 (num_games, 64) by square, armed uint8 (num_games,)) of the searches of the last move round of run()"""
        eta, armed = np.zeros((self.num_games, 64), np.float64), np.zeros(self.num_games, np.uint8)
        _lib.check(_lib.load().oz_selfplay_root_noise(self._h, _lib.p_f64(eta), _lib.p_u8(armed)))
        return eta, armed

    def last_counts(self):
        c = np.zeros((self.num_games, 64), np.int32)
        _lib.check(_lib.load().oz_selfplay_last_counts(self._h, _lib.p_i32(c)))
        return c

    def records(self, with_visits=False, with_values=False, with_targets=False, with_policies=False, with_surprise=False, with_weights=False):
        """move records of the games completed so far (numpy structured array, _lib.RECORD_DTYPE),
        sorted by (game_id, ply).  with_visits=True (engine created with record_visits=True): (records, counts), counts =
        int32 (R, 64) root visit counts of each record's move by square row*8+col, in the same order.
        with_values=True (record_values=True): (records, [counts,] values), values = float64 (R,) root value of each record's search.
        with_targets=True (after value_targets()): the float32 (R,) value targets follow, (records, [counts,] [values,] targets).
        with_policies=True (gumbel=...): the float32 (R, 64) improved-policy rows by square follow.
        with_surprise=True (record_surprise=True): the float64 (R,) policy surprises follow.
        with_weights=True (after surprise_weights()): the tuple (w float32 (R,), copies int32 (R,), first_sym uint8 (R,)) comes last."""
        total = self.stats()["records"]
        out = np.zeros(max(total, 1), dtype=_lib.RECORD_DTYPE)
        written = C.c_int64()
        _lib.check(_lib.load().oz_selfplay_records(self._h, out.ctypes.data_as(C.c_void_p), total, C.byref(written)))
        out = out[:written.value]
        order = np.lexsort((out["ply"], out["game_id"]))
        if with_surprise and not self.record_surprise:
            raise ValueError("records(with_surprise=True) needs an engine created with record_surprise=True")
        want = dict(with_visits=with_visits, with_values=with_values, with_targets=with_targets, with_policies=with_policies,
                    with_surprise=with_surprise, with_weights=with_weights)
        ret, got, rows = [out[order]], C.c_int64(), max(out.size, 1)
        for flag, entry, dtypes, row in _RECORD_ROWS:
            if want[flag]:
                arrays = [np.zeros((rows,) + row, dtype) for dtype in dtypes]
                _lib.check(getattr(_lib.load(), entry)(self._h, *(_POINTER[a.dtype.type](a) for a in arrays), out.size, C.byref(got)))
                assert got.value == out.size, (got.value, out.size)
                arrays = [a[:out.size][order] for a in arrays]
                ret.append(arrays[0] if len(arrays) == 1 else tuple(arrays))
        return tuple(ret) if len(ret) > 1 else ret[0]

    def solve_records(self, max_empties, first_record=0):
        """oz_selfplay_solve_records: the completed records from `first_record` on whose position has at most max_empties empties get the
        exact solver's value target in place on the device (z = the sign of the final disc difference under perfect play, for the mover; a
        draw goes to BLACK) -- nothing else of a record changes.  -> dict(records, solved, z_changed, optimal_moves, disc_loss_sum,
        disc_loss_max, mean_disc_loss): the discs the moves played gave away against perfect play, over the solved records.
        Under a playout cap it works on ALL records, the fast ones included: mean_disc_loss then measures the moves actually played, most of
        them searched on the fast budget, not the training examples alone."""
        max_empties = _lib.check_solve_empties(max_empties, 1)
        s = _lib.EndgameStats()
        _lib.check(_lib.load().oz_selfplay_solve_records(self._h, int(first_record), max_empties, C.byref(s)))
        out = {k: int(getattr(s, k)) for k, _ in s._fields_ if k != "pad"}
        out["mean_disc_loss"] = out["disc_loss_sum"] / out["solved"] if out["solved"] else 0.0
        return out

    def records_to_device(self, device_ptr, max_records):
        written = C.c_int64()
        _lib.check(_lib.load().oz_selfplay_records_device(self._h, C.c_void_p(device_ptr), max_records, C.byref(written)))
        return written.value

    def visits_to_device(self, device_ptr, max_records):
        """the visit-count rows (int32 [max_records][64]) in the ring order of records_to_device, device to device"""
        written = C.c_int64()
        _lib.check(_lib.load().oz_selfplay_visits_device(self._h, C.c_void_p(device_ptr), max_records, C.byref(written)))
        return written.value

    def policies_to_device(self, device_ptr, max_records):
        """the improved-policy rows (float32 [max_records][64], gumbel=...) in the ring order of records_to_device, device to device"""
        written = C.c_int64()
        _lib.check(_lib.load().oz_selfplay_policies_device(self._h, C.c_void_p(device_ptr), max_records, C.byref(written)))
        return written.value

    def targets_to_device(self, device_ptr, max_records):
        """the value targets (float32 [max_records], after value_targets()) in the ring order of records_to_device, device to device"""
        written = C.c_int64()
        _lib.check(_lib.load().oz_selfplay_targets_device(self._h, C.c_void_p(device_ptr), max_records, C.byref(written)))
        return written.value

    def eval_time(self):
        ms, launches, leaves = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(_lib.load().oz_selfplay_eval_time(self._h, C.byref(ms), C.byref(launches), C.byref(leaves)))
        return dict(ms=ms.value, launches=launches.value, leaves=leaves.value)

    def play_to_end(self, max_rounds=None, with_visits=False, endgame_targets=0, value_target="outcome", with_policies=False,
                    proof_targets=False):
        """endgame_targets=E > 0: solve_records(E) once the games are over, before the records are read (its stats: self.endgame_stats).
        value_target other than "outcome": value_targets(value_target, exact_empties=endgame_targets) after that (its stats:
        self.value_target_stats), and the targets come back too: (records, [counts,] targets).  with_policies=True (gumbel=...): the
        improved-policy rows come last.  proof_targets=True (proof_play=True): proof_targets() before all of that (its stats:
        self.proof_target_stats), and the value targets take a proven record as exact"""
        proof_targets = _lib.check_proof_targets(proof_targets, self.proof_play)
        max_rounds = max_rounds or self.n * self.n
        for _ in range(max_rounds):
            self.run(4)
            if self.stats()["live_games"] == 0:
                break
        if proof_targets:
            self.proof_target_stats = self.proof_targets()
        if endgame_targets:
            self.endgame_stats = self.solve_records(endgame_targets)
        if _lib.check_value_target(value_target)[0] != _lib.VALUE_TARGET_OUTCOME:
            self.value_target_stats = self.value_targets(value_target, exact_empties=endgame_targets, exact_proven=proof_targets)
            return self.records(with_visits=with_visits, with_targets=True, with_policies=with_policies)
        return self.records(with_visits=with_visits, with_policies=with_policies)


def preferred_batch_cap(board_size, num_games, channels=512, precision="f16x2"):
    """the batch cap at which conv3 -- the dominant launch -- is a whole number of rounds of 256 x 256 tiles on the chip's 256 CUs:
    the largest L <= num_games with ceil((n-2)^2 * L / 256) * (channels / 256) = 256 * r; 0 (no cap) when that is num_games itself or the
    network does not use those tiles (4096 8x8 games, 512 filters: 3640 = 4.0 rounds; 6x6: no cap).
    precision "bf16x3": no cap -- k_gemm_b3's one tile is 128 x 256, on which 4096 leaves are 9.0 rounds of conv3 AND 4.0 of conv4 (3640: 8.0 and
    3.55, paid as 4); measured 898 k against 886 k expansions/s with the cap (the free-running batches hold ~3900 leaves)"""
    if channels % 256 or num_games < 1024 or precision == "bf16x3":
        return 0
    P, cols = (board_size - 2) ** 2, channels // 256
    rounds = (num_games * P // 256) * cols // 256
    if rounds < 1:
        return 0
    cap = (256 * rounds // cols) * 256 // P
    return 0 if cap >= num_games else int(cap)


def expand_examples(records, board_size, alias_final=False, visits=None, target_temperature=1.0, values=None):
    """8-fold symmetry expansion of move records on the GPU (training.py:13-23,58-65).
    Returns boards (R*8, n, n, 2) uint8, policy_index (R*8,) int32 (position of the one-hot), z (R*8,) int8.

    visits = the records' root visit counts (int32 (R, 64), SelfPlayEngine.records(with_visits=True)): the policy is the search's
    visit distribution get_policy_action_probabilities(root, target_temperature) (othelo_mcts.py:51-67) in place of the one-hot,
    and the second array returned is pi (R*8, n, n) float64 (target_temperature > 0).

    The fast records of a playout cap (_lib.record_fast) are no training examples: they and their visit-count rows are dropped first, so R
    counts the fully searched moves.  The records of an adjudicated game (_lib.record_adjudicated) are examples like any other; with
    alias_final=True the "final board" of such a game is the board at the stop.

    values = the records' value targets (float32 (R,), agents.rules_value_targets / SelfPlayEngine.records(with_targets=True)): each
    example takes its record's target, 8 per record, and z comes back as float32 (in that case only)."""
    if values is not None:
        rec_all = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE)
        val = np.ascontiguousarray(values, dtype=np.float32).ravel()
        assert val.size == rec_all.size, f"{val.size} value targets for {rec_all.size} records"
        boards, pol, _z = expand_examples(rec_all, board_size, alias_final, visits=visits, target_temperature=target_temperature)
        return boards, pol, np.repeat(val[_lib.record_fast(rec_all).ravel() == 0], 8)
    records, visits = _lib.full_records(np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE), visits)
    rec = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE)
    R, n = rec.size, board_size
    if visits is not None:
        cnt = np.ascontiguousarray(visits, dtype=np.int32).reshape(-1, 64)
        assert cnt.shape[0] == R, f"{cnt.shape[0]} visit-count rows for {R} records"
        if not target_temperature > 0:
            raise ValueError(f"target_temperature must be > 0 for visit-count targets (got {target_temperature})")
        boards, pi, z = np.zeros((R * 8, n, n, 2), np.uint8), np.zeros((R * 8, n, n), np.float64), np.zeros(R * 8, np.int8)
        if R:
            _lib.check(_lib.require_gpu().oz_examples_expand_visits(rec.ctypes.data_as(C.c_void_p), _lib.p_i32(cnt), R, n,
                                                                    1 if alias_final else 0, float(target_temperature),
                                                                    _lib.p_u8(boards), _lib.p_f64(pi), _lib.p_i8(z)))
        return boards, pi, z
    boards = np.zeros((R * 8, n, n, 2), np.uint8)
    pol, z = np.zeros(R * 8, np.int32), np.zeros(R * 8, np.int8)
    if R:
        _lib.check(_lib.require_gpu().oz_examples_expand(rec.ctypes.data_as(C.c_void_p), R, n, 1 if alias_final else 0,
                                                         _lib.p_u8(boards), _lib.p_i32(pol), _lib.p_i8(z)))
    return boards, pol, z


def selfplay_batch(neural_network, board_size=8, num_games=4096, num_simulations=100, degree_exploration=1.0,
                   policy_temperature=1.0, e_greedy=0.9, seed=1234, first_game_id=0, q_mode=_lib.QMODE_F64,
                   expand=False, alias_final=False, record_visits=False, target_temperature=1.0, leaves_per_step=1, root_noise=None,
                   sample_moves=None, endgame_targets=0, solve_leaves=0, playout_cap=None, forced_playouts=None, value_target="outcome", gumbel=None,
                   surprise_weight=None, resign=None, value_signs="reference", proofs=False, proof_play=False, proof_targets=False,
                   selection=None, tree_gc="off", node_cap=0):
    """Play num_games complete games; returns the move records (or the expanded examples).
    tree_gc="demand" | "every": drop the tree nodes a game has passed (SelfPlayEngine); no record changes, a smaller node_cap (0 = the
    default, a whole game's nodes) suffices; selfplay_batch.tree_gc_stats holds the last call's SelfPlayEngine.tree_gc_stats() (None when off).
    selection=dict(fpu=, cpuct_growth=, prior_first=): the selection rule of the searches (SelfPlayEngine); not with gumbel or forced_playouts.
    proof_play=True (needs proofs=True): moves, visit rows, root values and the records' proof codes take what the roots' proofs know
    (SelfPlayEngine); selfplay_batch.proof_play_stats holds the last call's SelfPlayEngine.proof_play_stats() (None when off).
    proof_targets=True (needs proof_play=True): z of every proven record becomes the proven sign (SelfPlayEngine.proof_targets) before the
    endgame targets, the value targets -- which then take a proven record as exact -- and the expansion; selfplay_batch.proof_target_stats
    holds the last call's statistics (None when off).
    proofs=True (needs value_signs="sound"): the searches keep exact values as proofs and back them up the tree (SelfPlayEngine);
    selfplay_batch.proof_stats holds the last call's SelfPlayEngine.proof_stats() (None when off).
    value_signs="sound": the searches back their values up with the signs right across passes and finished boards (SelfPlayEngine).
    resign=(v, r, min_ply, keep_prob): resignation with a played-out audit share (SelfPlayEngine): a decided game stops early, its records
    carry the adjudicated z, the board at the stop as their final board (what alias_final=True then shows) and the flag
    _lib.record_adjudicated reads; nothing else about what comes back changes.  Not with gumbel (ValueError).  selfplay_batch.resign_stats
    holds the last call's SelfPlayEngine.resign_stats() (None when off).
    surprise_weight=(frac, weight_seed): policy surprise weighting (SelfPlayEngine(record_surprise=True).surprise_weights; needs
    record_visits=True or gumbel).  Two more entries come back last of all -- (records, ..., surprises, (w, copies, first_sym)): the float64
    policy surprise of every record and its float32 weight, int32 copy count and uint8 first symmetry, for the device replay buffer's
    weighted append or a consumer of one's own; not with expand (ValueError: the host example path does not weight).
    selfplay_batch.surprise_stats holds the last call's SelfPlayEngine.surprise_weights() statistics (None when off).
    gumbel=(max_considered, c_visit, c_scale) or True: the Gumbel root search in every searched move (SelfPlayEngine).  The float32 (R, 64)
    improved-policy rows come back last -- (records, [counts,] [targets,] policies) -- for loop.examples_from_records(policies=...); not with
    expand (ValueError).  selfplay_batch.gumbel_stats holds the last call's SelfPlayEngine.gumbel_stats() (None when off).
    record_visits=True: (records, visit counts) -- or, with expand, the examples with visit-distribution targets at target_temperature.
    root_noise=(alpha, epsilon): Dirichlet root noise in every search (SelfPlayEngine).
    sample_moves=(temperature, plies): the opening plies' moves are sampled from the visit counts (SelfPlayEngine).
    endgame_targets=E > 0: records with E empties or fewer carry the exact solver's value target (SelfPlayEngine.solve_records); with expand it
    needs alias_final=False.  selfplay_batch.endgame_stats holds the last call's statistics (None when off).
    solve_leaves=E > 0: exact values for the searches' leaves with at most E empties (SelfPlayEngine); selfplay_batch.rows_solved holds the
    last call's count (None when off).
    playout_cap=(fast_sims, full_prob): a playout cap on the searched moves (SelfPlayEngine).  The records returned are ALL records, the fast
    ones flagged (_lib.record_fast); with expand, the examples of the fully searched moves only.  selfplay_batch.playout_stats holds the last
    call's SelfPlayEngine.playout_stats() (None when off).
    forced_playouts=k > 0 (needs root_noise): forced playouts and policy target pruning (SelfPlayEngine): with record_visits the counts
    returned, and the targets expanded from them, are the pruned ones.  selfplay_batch.forced_playout_stats holds the last call's
    SelfPlayEngine.forced_playout_stats() (None when off).
    value_target=("blend", w) / ("td", lam): value targets from the searches' root values (SelfPlayEngine.value_targets, after the endgame
    targets, exact_empties = endgame_targets).  The float32 targets come back last -- (records, [counts,] targets) -- or, with expand, as
    the examples' float32 z; with expand it needs alias_final=False.  selfplay_batch.value_target_stats holds the last call's statistics
    (None when off)."""
    vt_on = _lib.check_value_target(value_target, expand and alias_final)[0] != _lib.VALUE_TARGET_OUTCOME
    o = _lib.check_selfplay_options(num_simulations, record_visits, leaves_per_step, root_noise, sample_moves, solve_leaves, playout_cap,
                                    forced_playouts, vt_on, gumbel, False, resign, value_signs, proofs, proof_play, selection, tree_gc)
    proof_targets = _lib.check_proof_targets(proof_targets, o["proof_play"])
    if o["gumbel"] is not None and expand:
        raise ValueError("selfplay_batch: gumbel with expand=True is not offered; expand the rows with loop.examples_from_records(policies=...)")
    if surprise_weight is not None:
        try:
            sw_frac, sw_seed = surprise_weight
        except (TypeError, ValueError):
            raise ValueError(f"surprise_weight must be (frac, weight_seed), got {surprise_weight!r}") from None
        sw_frac = _lib.check_surprise_frac(sw_frac)
        if expand:
            raise ValueError("selfplay_batch: surprise_weight with expand=True is not offered: the host example path writes 8 examples per record")
        if not (record_visits or o["gumbel"] is not None):
            raise ValueError("selfplay_batch: surprise_weight needs record_visits=True or gumbel=...: the surprise is that of a recorded policy target")
        o["record_surprise"] = True                        # (past the engine's rule for it, in this function's words just above)
    endgame_targets = _lib.check_endgame_targets(endgame_targets, expand and alias_final)
    eng = SelfPlayEngine(neural_network, board_size, num_games, num_simulations, degree_exploration, policy_temperature,
                         e_greedy, seed, first_game_id, q_mode=q_mode,
                         **_lib.engine_kw(o, always=("record_visits", "leaves_per_step", "root_noise", "sample_moves", "solve_leaves", "playout_cap")),
                         **({"node_cap": int(node_cap)} if node_cap else {}))
    got = eng.play_to_end(with_visits=record_visits, endgame_targets=endgame_targets, value_target=value_target,
                          with_policies=o["gumbel"] is not None, proof_targets=proof_targets)
    got = got if isinstance(got, tuple) else (got,)        # records, [counts,] [targets,] [policies]
    selfplay_batch.surprise_stats = None
    if surprise_weight is not None:
        selfplay_batch.surprise_stats = eng.surprise_weights(sw_frac, sw_seed)
        got += eng.records(with_surprise=True, with_weights=True)[1:]
    for name, stats in eng.option_stats().items():
        setattr(selfplay_batch, name, stats)
    if expand:
        return expand_examples(got[0], board_size, alias_final, visits=got[1] if record_visits else None, target_temperature=target_temperature,
                               values=got[-1] if vt_on else None)
    return got if len(got) > 1 else got[0]
