"""Replay buffer, iteration loop and promotion rules -- the caller of the hot path (main.py:21-259), SURVEY.md 8(f) item 3.

`CircularArray` is a drop-in for main.py:21-53 (same ring arithmetic, including its quirks: the write index only starts
moving once the buffer is full, and `random.shuffle(buffer)` permutes the slots the ring later overwrites).
`training(...)` keeps main.py:56-259's structure and decision rules, with the reference's WorkerManager fan-out replaced by
the batched GPU engines:

  episodes            worker_manager.run(EXECUTE_EPISODE, ...)          -> training.selfplay_batch (lock-step games in HBM)
  new-vs-old matches  worker_manager.run(DUEL_BETWEEN_NEURAL_NETWORKS)  -> agents.arena_batch (half the games per colour)
  fit                 neural_network.train(examples)                    -> oz_trainer_* (NNet.py)
  evaluation          duel_between_agents vs RandomOthelloAgent         -> the same drop-in agents (agents.py), sequential

Decision rules kept verbatim: promote after self-play when `new_net_victories >= self_play_threshold` (main.py:138);
after an evaluation round keep the new network when `net_wins > old_net_wins * 1.1` (main.py:238), otherwise fall back to
the old one; temperature drops to 0 from iteration `temperature_threshold` on (main.py:74-77).

Deliberate differences (documented, switchable where it matters):
* `reference_aliasing=True` reproduces `old_neural_network = neural_network` (main.py:142,243): after the first promotion
  both names are ONE object, so later training also changes the "old" network.  False keeps a real copy.
* the reference's worker-side `duel_between_neural_networks` (training.py:75-88) cannot run (it indexes a dict with the
  tuple `duel_between_agents` returns); the intent -- `self_play_total_games` temperature-0 games, half per colour -- is what
  `arena_batch` plays.
* `examples-<n>.txt` (a str() dump of the whole buffer every iteration, main.py:252-253) is only written when asked.
"""
import ctypes as C
import logging
import random

import numpy as np

from . import _lib
from .agents import MinimaxOthelloAgent, NeuralNetworkOthelloAgent, RandomOthelloAgent, arena_batch, duel_between_agents
from .Othello import OthelloGame, OthelloPlayer
from .training import expand_examples, selfplay_batch


class CircularArray:
    """Ring buffer with the semantics of main.py:21-53, quirks included: it grows like a list up to `max_`; once full,
    item k overwrites slot `_index % len` and `_index` becomes that slot + 1 (so it runs 1..len and restarts at slot 0
    through the modulo).  Indexing, slicing, assignment, iteration, len, str and repr go to the underlying list."""

    def __init__(self, max_):
        self._list, self._max, self._index = [], max_, 0

    def append(self, item):
        held = len(self._list)
        if held < self._max:
            self._list.append(item)
            return
        slot = self._index % held
        self._list[slot] = item
        self._index = slot + 1

    def extend(self, items):
        for item in items:
            self.append(item)

    def __len__(self):
        return len(self._list)

    def __getitem__(self, key):
        return self._list[key]

    def __setitem__(self, key, value):
        self._list[key] = value

    def __iter__(self):
        return iter(self._list)

    def __str__(self):
        return str(self._list)

    def __repr__(self):
        return f'{type(self).__name__}({len(self._list)!r})'


def examples_from_records(records, board_size, alias_final=True, in_channels=2, visits=None, target_temperature=1.0, values=None, policies=None):
    """move records of finished games -> the reference's example tuples [(board, one-hot policy (n,n), z)], 8 per move in
    training.py:13-23's order.

    in_channels=2 (OthelloNN): board (n,n,2) bool; alias_final=True shows every board as the game's FINAL position, which is
    what execute_episode really returns (the examples are views of the live game array); False stores the
    position at the move.
    in_channels=1 (BaseNN): board (n,n) with +1 BLACK / -1 WHITE, the position AT THE MOVE whatever alias_final says -- the
    reference builds a fresh one-channel array per round for BNN (training.py:34-37, Othello/__init__.py:79-84,266-270), so
    those examples are never aliased.
    visits (int32 (R, 64), the records' root visit counts): the policy of every example is the search's visit distribution at
    target_temperature (expand_examples) instead of the one-hot of the move played.
    The fast records of a playout cap (_lib.record_fast) are no training examples: they and their visit-count rows are dropped first.
    The records of an adjudicated game (_lib.record_adjudicated, SelfPlayEngine(resign=...)) are examples like any other: z is the adjudicated
    one, and with alias_final=True the "final board" of such a game is the board at the stop.
    values (float32 (R,), the records' value targets): the z of every example is its record's target, a float, instead of the int outcome.
    policies (float32 (R, 64) by square, the records' improved-policy rows of a Gumbel search, SelfPlayEngine.records(with_policies=True)): the
    policy of every example is its record's row under the example's symmetry, float32 (n, n), bit for bit (oz_examples_expand_policy, on the
    host); not together with visits."""
    if policies is not None:
        if visits is not None:
            raise ValueError("examples_from_records: policies and visits are two policy targets; pass one")
        rec = np.ascontiguousarray(records, dtype=_lib.RECORD_DTYPE).ravel()
        rows = np.ascontiguousarray(policies, dtype=np.float32).reshape(-1, 64)
        if rows.shape[0] != rec.size:
            raise ValueError(f"{rows.shape[0]} policy rows for {rec.size} records")
        keep = _lib.record_fast(rec).ravel() == 0
        if values is not None:
            val = np.ascontiguousarray(values, dtype=np.float32).ravel()
            assert val.size == rec.size, f"{val.size} value targets for {rec.size} records"
            values = val[keep]
        rec, rows = np.ascontiguousarray(rec[keep]), np.ascontiguousarray(rows[keep])
        R, n, one_channel = rec.size, board_size, in_channels == 1
        boards, pi, z = np.zeros((R * 8, n, n, 2), np.uint8), np.zeros((R * 8, n, n), np.float32), np.zeros(R * 8, np.int8)
        if R:
            _lib.check(_lib.load().oz_examples_expand_policy(rec.ctypes.data_as(C.c_void_p), _lib.p_f32(rows), R, n,
                                                             1 if alias_final and not one_channel else 0, _lib.p_u8(boards), _lib.p_f32(pi), _lib.p_i8(z)))
        boards = boards[..., 0].astype(np.int64) - boards[..., 1].astype(np.int64) if one_channel else boards.astype(bool)
        zz = [float(t) for t in np.repeat(values, 8)] if values is not None else [int(t) for t in z]
        return list(zip(boards, pi, zz))
    if values is not None:
        val = np.ascontiguousarray(values, dtype=np.float32).ravel()
        assert val.size == np.asarray(records).size, f"{val.size} value targets for {np.asarray(records).size} records"
        values = val[_lib.record_fast(records).ravel() == 0]
    records, visits = _lib.full_records(records, visits)
    one_channel = in_channels == 1
    boards, pol, z = expand_examples(records, board_size, alias_final=alias_final and not one_channel, visits=visits,
                                     target_temperature=target_temperature)
    n = board_size
    if one_channel:
        boards = boards[..., 0].astype(np.int64) - boards[..., 1].astype(np.int64)      # convert_to_one_channel_board
    else:
        boards = boards.astype(bool)
    if values is not None:
        z = [float(t) for t in np.repeat(values, 8)]
    else:
        z = [int(zz) for zz in z]
    if visits is not None:
        return list(zip(boards, pol, z))
    out = []
    for b, p, zz in zip(boards, pol, z):
        policy = np.zeros((n, n))
        policy[p // n, p % n] = 1
        out.append((b, policy, zz))
    return out


def evaluate_against_random(board_size, neural_network, games, num_simulations, degree_exploration, label="Network", opponent=None):
    """main.py:163-192 / :197-233: `games` duels against RandomOthelloAgent, colours drawn by random.shuffle.
    opponent=("minimax", depth[, "discs" | "weighted"]): against MinimaxOthelloAgent instead (None / "random": the random agent).
    -> dict(wins, black_wins, black_games, white_wins, white_games)"""
    minimax = _lib.check_opponent(opponent)
    r = dict(wins=0, black_wins=0, black_games=0, white_wins=0, white_games=0)
    if getattr(neural_network, "max_batch", 1) > 32 and hasattr(neural_network, "get_weights"):
        # one position per call: a twin with max_batch 1 takes the library's latency path (k loops split over idle CUs)
        from .NNet import NNetWrapper
        neural_network = NNetWrapper((board_size, board_size), network=neural_network.network_type,
                                     num_channels_1=neural_network.num_channels, max_batch=1,
                                     weights=neural_network.get_weights(), precision=neural_network.precision)
    for k in range(games):
        game = OthelloGame(board_size, current_player=OthelloPlayer.BLACK)
        nn_agent = NeuralNetworkOthelloAgent(game, neural_network, num_simulations, degree_exploration)
        random_agent = (RandomOthelloAgent(game) if minimax is None else
                        MinimaxOthelloAgent(game, minimax[0], "discs" if minimax[1] == _lib.MINIMAX_EVAL_DISCS else "weighted"))
        agents = [nn_agent, random_agent]
        random.shuffle(agents)
        agent_winner, points = duel_between_agents(game, *agents)
        winner = OthelloPlayer.BLACK if agents[0] is agent_winner else OthelloPlayer.WHITE
        colour = "black" if winner == OthelloPlayer.BLACK else "white"
        r[colour + "_games"] += 1
        if agent_winner is nn_agent:
            r["wins"] += 1
            r[colour + "_wins"] += 1
        logging.info('%s: %d of %d won (%.2f); as black %d/%d, as white %d/%d', label, r["wins"], k + 1, r["wins"] / (k + 1),
                     r["black_wins"], r["black_games"], r["white_wins"], r["white_games"])
    return r


def evaluate_against_random_batch(board_size, neural_network, games, num_simulations, degree_exploration, seed=0, leaves_per_step=1,
                                  opponent=None, solve_leaves=0, openings=None, value_signs="reference", proofs=False,
                                  proof_play=False, selection=None, tree_gc="off"):
    """The same evaluation as `evaluate_against_random` played in lock step on the GPU (agents.arena_batch with a random
    mover): the network takes BLACK in the first games // 2 + games % 2 games and WHITE in the rest (the reference draws the
    colours with random.shuffle; the split here is fixed).  opponent: arena_batch's (None / "random", or ("minimax", depth[, evaluation])).
    solve_leaves=E > 0: the network's search takes exact values for leaves with at most E empties (arena_batch).
    value_signs="sound": the network's search backs its values up with the signs right across passes and finished boards (arena_batch).
    proofs=True (needs value_signs="sound"): the network's search keeps exact values as proofs and backs them up the tree (arena_batch).
    proof_play=True (needs proofs=True): the network's move is the arg-max of the row its root's proofs keep (arena_batch).
    openings=(plies, opening_seed): every game starts with a random opening (arena_batch); game k of the BLACK half and game k of the WHITE half
    play opening k, so the network meets every opening from both sides (with an odd `games` the BLACK half has one opening more).
    -> dict(wins, black_wins, black_games, white_wins, white_games)"""
    _lib.check_opponent(opponent)
    search = _lib.search_kw(_lib.check_search_options(solve_leaves, value_signs, proofs, proof_play, selection, tree_gc))
    _lib.check_openings(openings)
    kw = dict(search, seed=seed, leaves_per_step=leaves_per_step, opponent=opponent,
              **({"openings": openings, "first_opening_id": 0} if openings is not None else {}))
    as_black, as_white = games // 2 + games % 2, games // 2
    r = dict(wins=0, black_wins=0, black_games=0, white_wins=0, white_games=0)
    if as_black:
        res = arena_batch(neural_network, None, board_size, as_black, num_simulations, degree_exploration, **kw)
        r["black_wins"] = int((res["winner"] == 1).sum())
    if as_white:
        res = arena_batch(None, neural_network, board_size, as_white, num_simulations, degree_exploration, first_game_id=as_black, **kw)
        r["white_wins"] = int((res["winner"] == -1).sum())
        r["black_games"] = as_white - r["white_wins"]              # games BLACK (the random agent) won
    r["white_games"] = r["white_wins"] + (as_black - r["black_wins"])
    r["black_games"] += r["black_wins"]
    r["wins"] = r["black_wins"] + r["white_wins"]
    return r


def evaluate_against_opponent(board_size, neural_network, games, num_simulations, degree_exploration, opponent, label="Network"):
    """`evaluate_against_random` under the name that says what it does when the opponent is not the random agent"""
    return evaluate_against_random(board_size, neural_network, games, num_simulations, degree_exploration, label=label, opponent=opponent)


def evaluate_against_opponent_batch(board_size, neural_network, games, num_simulations, degree_exploration, opponent, seed=0, leaves_per_step=1,
                                    solve_leaves=0, openings=None, value_signs="reference", proofs=False, proof_play=False, selection=None, tree_gc="off"):
    """`evaluate_against_random_batch` under the name that says what it does when the opponent is not the random agent"""
    return evaluate_against_random_batch(board_size, neural_network, games, num_simulations, degree_exploration, seed=seed,
                                         leaves_per_step=leaves_per_step, opponent=opponent, solve_leaves=solve_leaves, openings=openings,
                                         value_signs=value_signs, proofs=proofs, proof_play=proof_play, selection=selection, tree_gc=tree_gc)


def _discs(boards):
    return np.array([int(x).bit_count() for x in np.asarray(boards, dtype=np.uint64).ravel()], dtype=np.int64)


def pair_statistics(new_black_final_black, new_black_final_white, old_black_final_black, old_black_final_white, opening_plies=None):
    """The arithmetic of paired_match, on final boards alone (uint64 bitboards, one entry per pair): pair i is game i of the arena where the new
    network was BLACK (first two arguments: its final black / white discs) and game i of the arena where the old one was BLACK (last two), both
    begun with the same opening.  -> dict(
      pairs,
      wins        games to the new network by the reference's rule, where a drawn board goes to BLACK (get_winning_player): what self_play_match
                  counts, so a draw is a win for whoever happened to hold BLACK;
      wins_true, draws, losses   the 2 * pairs games by disc count, a drawn board counted as a draw;
      margin      int64 (pairs, 2): the new network's discs minus the old one's, [:, 0] as BLACK, [:, 1] as WHITE;
      pair_margin int64 (pairs,) = their sum: the opening's own advantage for BLACK cancels in it;
      mean_margin, se   mean of pair_margin and its standard error over pairs, std(ddof=1) / sqrt(pairs) (nan with fewer than two pairs);
      split_pairs pairs in which each network won one game: there the opening decided the games, not the networks;
      opening_plies     as given (None if not).)"""
    ab, aw, bb, bw = _discs(new_black_final_black), _discs(new_black_final_white), _discs(old_black_final_black), _discs(old_black_final_white)
    if not ab.size == aw.size == bb.size == bw.size:
        raise ValueError("pair_statistics: the four arrays hold one entry per pair each")
    pairs = int(ab.size)
    margin = np.stack([ab - aw, bw - bb], axis=1).reshape(pairs, 2)
    pair_margin = margin.sum(axis=1)
    return dict(pairs=pairs, wins=int((ab >= aw).sum() + (bw > bb).sum()), wins_true=int((margin > 0).sum()), draws=int((margin == 0).sum()),
                losses=int((margin < 0).sum()), margin=margin, pair_margin=pair_margin,
                mean_margin=float(pair_margin.mean()) if pairs else float("nan"),
                se=float(pair_margin.std(ddof=1) / np.sqrt(pairs)) if pairs > 1 else float("nan"),
                split_pairs=int((margin[:, 0] * margin[:, 1] < 0).sum()), opening_plies=opening_plies)


def paired_match(board_size, neural_network, old_neural_network, pairs, num_simulations, degree_exploration, openings, seed=0, leaves_per_step=1,
                 solve_leaves=0, value_signs="reference", proofs=False, proof_play=False, selection=None, tree_gc="off"):
    """A match over an opening suite, every opening played twice with the colours swapped -- NOT the reference's match (main.py:110-134 starts
    every game from the standard position).  Two arenas of `pairs` games: the new network as BLACK against the old one, then the old one as
    BLACK against the new; both get openings=(plies, opening_seed) and first_opening_id=0, so game i of either starts with opening i.  Game ids
    are 0 .. pairs - 1 and pairs .. 2 pairs - 1, as in self_play_match.  -> pair_statistics' dict, plus games = the two arena_batch results."""
    search = _lib.search_kw(_lib.check_search_options(solve_leaves, value_signs, proofs, proof_play, selection, tree_gc))
    if openings is None:
        raise ValueError("paired_match needs openings=(plies, opening_seed): without them every pair is the same two games")
    _lib.check_openings(openings)
    if isinstance(pairs, bool) or not isinstance(pairs, (int, np.integer)) or pairs < 1:
        raise ValueError(f"paired_match: pairs must be a whole number >= 1 (got {pairs!r})")
    kw = dict(search, leaves_per_step=leaves_per_step, openings=openings, first_opening_id=0)
    a = arena_batch(neural_network, old_neural_network, board_size, int(pairs), num_simulations, degree_exploration, seed=seed, **kw)
    b = arena_batch(old_neural_network, neural_network, board_size, int(pairs), num_simulations, degree_exploration, seed=seed,
                    first_game_id=int(pairs), **kw)
    assert np.array_equal(a["opening_plies"], b["opening_plies"])
    return dict(pair_statistics(a["final_black"], a["final_white"], b["final_black"], b["final_white"], a["opening_plies"]), games=(a, b))


def self_play_match(board_size, neural_network, old_neural_network, total_games, num_simulations, degree_exploration, seed=0,
                    leaves_per_step=1, solve_leaves=0, openings=None, value_signs="reference", proofs=False, proof_play=False, selection=None, tree_gc="off"):
    """main.py:110-134: total_games // 2 games with the new network as BLACK, the rest with it as WHITE.
    -> number of games the new network won (a drawn game goes to BLACK, like get_winning_player).
    solve_leaves=E > 0: both networks' searches take exact values for leaves with at most E empties (arena_batch).
    value_signs="sound": both networks' searches back their values up with the signs right across passes and finished boards (arena_batch).
    proofs=True (needs value_signs="sound"): both searches keep exact values as proofs and back them up the tree (arena_batch).
    proof_play=True (needs proofs=True): both agents' moves are the arg-max of the row their root's proofs keep (arena_batch).
    openings=(plies, opening_seed): paired_match over total_games // 2 openings instead (total_games must be even: a pair is two games); the
    return value is its `wins`, counted by the same rule, and self_play_match.stats holds its dict (None after a match without openings)."""
    search = _lib.search_kw(_lib.check_search_options(solve_leaves, value_signs, proofs, proof_play, selection, tree_gc))
    self_play_match.stats = None
    if openings is not None:
        _lib.check_openings(openings)
        if total_games % 2 or total_games < 2:
            raise ValueError(f"self_play_match with openings plays pairs of games: total_games must be even and >= 2 (got {total_games})")
        stats = paired_match(board_size, neural_network, old_neural_network, total_games // 2, num_simulations, degree_exploration, openings,
                             seed=seed, leaves_per_step=leaves_per_step, **search)
        self_play_match.stats = {k: v for k, v in stats.items() if k != "games"}
        return stats["wins"]
    as_black, as_white = total_games // 2, total_games // 2 + total_games % 2
    kw = dict(search, seed=seed, leaves_per_step=leaves_per_step)
    wins = 0
    if as_black:
        res = arena_batch(neural_network, old_neural_network, board_size, as_black, num_simulations, degree_exploration, **kw)
        wins += int((res["winner"] == 1).sum())
    if as_white:
        res = arena_batch(old_neural_network, neural_network, board_size, as_white, num_simulations, degree_exploration, first_game_id=as_black, **kw)
        wins += int((res["winner"] == -1).sum())
    return wins


_ENGINE_ALWAYS = ("record_visits", "leaves_per_step", "root_noise", "sample_moves", "solve_leaves")    # the loop's engines get these, on or off
_STATS_PUBLISHED = ("resign_stats", "surprise_stats", "proof_stats", "proof_play_stats", "proof_target_stats")      # training.<name> of an iteration


def _selfplay_into_replay(replay, neural_network, board_size, num_episodes, num_simulations, degree_exploration, temperature, e_greedy, seed,
                          first_game_id, q_mode, visits, leaves_per_step, root_noise, sample_moves, alias_final_boards, policy_target,
                          target_temperature, endgame_targets=0, solve_leaves=0, playout_cap=None, forced_playouts=0.0, value_target="outcome",
                          gumbel=None, surprise_weight=None, resign=None, value_signs="reference", proofs=False, proof_play=False,
                          proof_targets=False, selection=None, tree_gc="off"):
    """one iteration's games on the engine selfplay_batch would create, played to the end without reading a record, and their examples
    appended to the device buffer; -> (records appended, the engine's option_stats() plus surprise_stats: what _publish_selfplay_stats
    takes).  One-channel (BaseNN) examples are never aliased (examples_from_records).  endgame_targets > 0: SelfPlayEngine.solve_records before the append.  playout_cap: the engine's; the
    append leaves the fast records out and counts the fully searched ones.  forced_playouts: the engine's; its visit rows, which the append
    reads, are then the pruned ones.  value_target: the engine records root values and the append computes the value targets (after the
    endgame solver, exact_empties = endgame_targets).  gumbel: the engine's; policy_target="improved" appends its improved-policy rows.
    surprise_weight=(frac, weight_seed): the engine records policy surprise and the append writes c_i examples per record
    (ReplayBuffer.append_engine(surprise_weight=...)); training.surprise_stats then holds the iteration's dict(records, examples,
    mean_copies, max_copies, mean_surprise).  resign: the engine's; an adjudicated record is appended like any other, and training.resign_stats
    then holds the engine's resign_stats().  proof_play: the engine's; training.proof_play_stats then holds its proof_play_stats().
    proof_targets: SelfPlayEngine.proof_targets before the endgame solver and the append, whose value targets then take a proven record as
    exact; training.proof_target_stats holds its statistics."""
    from .training import SelfPlayEngine
    vt_on = _lib.check_value_target(value_target)[0] != _lib.VALUE_TARGET_OUTCOME
    o = _lib.check_selfplay_options(num_simulations, visits, leaves_per_step, root_noise, sample_moves, solve_leaves, playout_cap, forced_playouts,
                                    vt_on, gumbel, surprise_weight is not None, resign, value_signs, proofs, proof_play, selection, tree_gc)
    eng = SelfPlayEngine(neural_network, board_size, num_episodes, num_simulations, degree_exploration, temperature, e_greedy, seed,
                         first_game_id, q_mode=q_mode, **_lib.engine_kw(o, always=_ENGINE_ALWAYS))
    for _ in range(board_size * board_size):
        eng.run(4)
        if eng.stats()["live_games"] == 0:
            break
    if proof_targets:
        eng.proof_target_stats = eng.proof_targets()
    if endgame_targets:
        eng.endgame_stats = eng.solve_records(endgame_targets)
    stats = dict(eng.option_stats(), surprise_stats=None)
    appended = replay.append_engine(eng, alias_final=alias_final_boards and getattr(neural_network, "in_channels", 2) == 2,
                                    policy_target=policy_target, target_temperature=target_temperature, surprise_weight=surprise_weight,
                                    **({"value_target": value_target, "exact_empties": endgame_targets, "exact_proven": bool(proof_targets)} if vt_on else {}))
    if surprise_weight is not None:
        st = replay.last_weight_stats
        rec, sur = eng.records(with_surprise=True)
        full = _lib.record_fast(rec) == 0
        stats["surprise_stats"] = dict(records=st["full_records"], examples=st["examples"], max_copies=st["max_copies"],
                                       mean_copies=st["examples"] / st["full_records"] if st["full_records"] else 0.0,
                                       mean_surprise=float(sur[full].mean()) if full.any() else 0.0)
    return appended, stats


def _publish_selfplay_stats(i, num_iterations, stats):
    """an iteration's self-play statistics (SelfPlayEngine.option_stats(), and surprise_stats where the device path weighted) -> the
    training.* attributes of their names, training.rows_solved, the histories and the log lines of the options that are on"""
    training.rows_solved += stats["rows_solved"] or 0
    for name in _STATS_PUBLISHED:
        setattr(training, name, stats.get(name))
    if stats["resign_stats"] is not None:
        training.resign_history.append(stats["resign_stats"])
        _log_resign(i, num_iterations, stats["resign_stats"])
    if stats["proof_stats"] is not None:
        training.proof_history.append(stats["proof_stats"])
        _log_proofs(i, num_iterations, stats["proof_stats"])
    if stats["proof_play_stats"] is not None:
        training.proof_play_history.append(dict(stats["proof_play_stats"], targets=stats["proof_target_stats"]))
        _log_proof_play(i, num_iterations, stats["proof_play_stats"], stats["proof_target_stats"])
    if stats.get("surprise_stats") is not None:
        st = stats["surprise_stats"]
        training.surprise_history.append(st)
        logging.info('[%d/%d] surprise weighting: %d examples from %d records / mean_copies %.3f / max_copies %d / mean_surprise %.4f', i,
                     num_iterations, st["examples"], st["records"], st["mean_copies"], st["max_copies"], st["mean_surprise"])
    if stats["endgame_stats"] is not None:
        training.endgame_history.append(stats["endgame_stats"])
        _log_endgame(i, num_iterations, stats["endgame_stats"])


def _log_resign(i, num_iterations, stats):
    logging.info('[%d/%d] resignation: %d games adjudicated after %.1f plies on average / audit: %d exempt games, %d triggered, %d wrongly '
                 '(false-positive rate %s)', i, num_iterations, stats["games_adjudicated"],
                 stats["adjudicated_plies_sum"] / stats["games_adjudicated"] if stats["games_adjudicated"] else 0.0, stats["games_exempt"],
                 stats["exempt_triggered"], stats["exempt_wrong"],
                 '%.3f' % (stats["exempt_wrong"] / stats["exempt_triggered"]) if stats["exempt_triggered"] else 'n/a')


def _log_proofs(i, num_iterations, stats):
    logging.info('[%d/%d] proofs: %d edges proven / descents ended on a proven edge %d, on a proven node %d / %d roots proven', i, num_iterations,
                 stats["edges_proven"], stats["edge_stops"], stats["node_stops"], stats["roots_proven"])


def _log_proof_play(i, num_iterations, stats, targets):
    logging.info('[%d/%d] proof play: %d moves on a proven root / %d rows changed, %d moves changed, %d fallbacks%s', i, num_iterations,
                 stats["proven_roots"], stats["rows_changed"], stats["moves_changed"], stats["fallbacks"],
                 '' if targets is None else ' / proof targets: %d of %d records proven, z changed in %d' % (
                     targets["proven"], targets["records"], targets["z_changed"]))


def _fit_with_holdout(i, num_iterations, neural_network, replay, total_before, share):
    """the device fit of an iteration with the newest floor(share * E) of the E examples its append wrote held out (trainer.holdout_slots):
    evaluated before the fit and after each epoch, logged, and recorded in training.validation_history"""
    from .trainer import VAL_KEYS, holdout_slots
    held, capacity, total = replay.info()
    _, val_slots = holdout_slots(held, capacity, total, total - total_before, share)
    before = neural_network.evaluate(replay, val_slots) if val_slots.size else None
    hist = neural_network.train(replay, verbose=2 if logging.root.level <= logging.DEBUG else None, validation_slots=val_slots)
    epochs = [{k: hist.history["val_" + k][ep] for k in VAL_KEYS} for ep in range(len(hist.history.get("val_loss", [])))]
    stats = dict(examples=int(val_slots.size), decided=before["decided"] if before else 0, before=before, epochs=epochs)
    training.validation_history.append(stats)
    _log_validation(i, num_iterations, stats)
    return hist


def _log_validation(i, num_iterations, stats):
    if not stats["epochs"]:
        logging.info('[%d/%d] held-out evaluation: %d examples held out, nothing to report', i, num_iterations, stats["examples"])
        return
    b, e = stats["before"], stats["epochs"][-1]
    logging.info('[%d/%d] held-out evaluation: %d newest examples (%d decided) / loss %.4f -> %.4f (pi %.4f -> %.4f, v %.4f -> %.4f) / '
                 'policy_top1 %.3f -> %.3f / value_sign %.3f -> %.3f (before the fit -> after its last epoch)', i, num_iterations,
                 stats["examples"], stats["decided"], b["loss"], e["loss"], b["pi-reshaped_loss"], e["pi-reshaped_loss"], b["v_loss"], e["v_loss"],
                 b["policy_top1"], e["policy_top1"], b["value_sign"], e["value_sign"])


def _log_endgame(i, num_iterations, stats):
    logging.info('[%d/%d] endgame targets: solved %d / z_changed %d / mean_disc_loss %.3f', i, num_iterations, stats["solved"],
                 stats["z_changed"], stats["mean_disc_loss"])


def training(board_size, num_iterations, num_episodes, num_simulations, degree_exploration, temperature, neural_network,
             e_greedy, evaluation_interval, evaluation_iterations, temperature_threshold, self_play_training,
             self_play_interval, self_play_total_games, self_play_threshold, checkpoint_filepath, training_buffer_size,
             seed=1234, reference_aliasing=True, alias_final_boards=True, dump_examples=False, q_mode=_lib.QMODE_F64,
             distributed=False, batched_evaluation=False, policy_target="onehot", target_temperature=1.0, leaves_per_step=1,
             root_noise=None, sample_moves=None, replay="host", evaluation_opponent="random", endgame_targets=0,
             solve_leaves=0, match_openings=None, evaluation_openings=None, playout_cap=None, forced_playouts=None, eval_symmetry=None,
             value_target="outcome", gumbel=None, surprise_weight=None, resign=None, validation_share=None, value_signs="reference", proofs=False,
             proof_play=False, proof_targets=False, selection=None, tree_gc="off", aux_heads=None):
    """main.py:56-259 on the GPU engines; returns `historic` = [(episodes done, win rate vs random), ...]

    aux_heads=dict(ownership=w, score=w) (None = off, the default: the loop is unchanged): KataGo's auxiliary targets from the end of the game.
    The trainer gains an ownership and a score head (Trainer(aux_heads=...): who owns each square on the game's final board, and the final disc
    margin, both for the mover; trained with the trunk, never used at play time), the device replay buffer keeps every example's final pair
    (ReplayBuffer(aux=True): zero for the records of adjudicated games and for fast records), and the two losses are logged per iteration;
    training.aux_history keeps them.  It needs replay="device", not distributed=True, and alias_final_boards=False for a two-plane network
    (ValueError otherwise: _lib.check_aux_heads_loop).  Playing strength is neither gated nor claimed ("Auxiliary heads").

    validation_share=f in (0, 0.5] (None = off, the default: the loop is unchanged): held-out evaluation of every iteration's fit.  After an
    iteration's append, the newest floor(f * E) of the E examples that append wrote (trainer.holdout_slots) are held out of THAT iteration's fit
    and evaluated in inference mode -- moving BN statistics, no dropout (NNetWrapper.evaluate) -- before the fit and after each of its epochs:
    one log line per iteration, and training.validation_history gains dict(examples, decided, before, epochs=[one dict per epoch]).  The
    examples stay in the ring and are ordinary training data from the next iteration on: validation is always on the newest games, never
    trained on at the time they are measured.  It needs replay="device" (ValueError otherwise).  Two known leaks: the cut may fall inside a
    game or between the symmetric copies of one position, so a held-out example may have a sibling in the training part; and opening
    positions recur in every game, so early-ply examples are in effect seen before.  The numbers bound nothing about playing strength, which is
    neither gated nor claimed ("Held-out evaluation").

    resign=(v, r, min_ply, keep_prob) (None = off, the default): resignation of decided SELF-PLAY games with a played-out audit share
    (SelfPlayEngine), in the host path, the distributed path (the flag travels inside the 48-byte records through the all-gather) and with
    replay="device" alike; matches and evaluations are never adjudicated.  A game whose root values, seen from BLACK, stayed at or beyond
    +-v for r searched moves in a row stops from ply min_ply on and goes to that side: its records carry that z and train like any other
    (with alias_final_boards=True the "final board" of such a game is the board at the stop), and the searches of a decided game's last
    plies are saved.  A share keep_prob of the games is played out regardless.  Logs the adjudicated games and the audit counters per
    iteration; training.resign_history keeps the engines' resign_stats() dicts (with distributed=True: this rank's), from which
    exempt_wrong / exempt_triggered is the rule's false-positive rate -- tune v until it is a few per cent (AlphaGo Zero: below 5 %).
    Not with gumbel (ValueError).  Playing strength is neither gated nor claimed ("Resignation").

    surprise_weight=frac in (0, 1] (None = off, the default; KataGo uses 0.5): policy surprise weighting of the SELF-PLAY records.  The engine
    keeps every searched move's surprise KL(policy target || root prior) (SelfPlayEngine(record_surprise=True)); a fully searched record of a
    game with K of them weighs (1 - frac) + frac s K / S and becomes floor(8 w + u) examples of the device buffer instead of 8, so the
    positions where the search overturned the prior take a larger share of the same amount of data.  The weight seed of iteration i is
    seed + i.  It needs replay="device" and policy_target "visits" or "improved" (ValueError otherwise: the host example path writes 8
    examples per record, distributed=True has no device buffer, and a one-hot target has no surprise to speak of).  Logs the examples
    written, the mean and maximum copies per record and the mean surprise per iteration; training.surprise_history keeps the dicts.
    Playing strength is neither gated nor claimed ("Policy surprise weighting").

    gumbel=(max_considered, c_visit, c_scale) or True (None = off, the default): the root search of Gumbel AlphaZero for every searched
    SELF-PLAY move (SelfPlayEngine), with replay="host" and replay="device" alike; matches and evaluations stay on PUCT.  It replaces
    root_noise, forced_playouts and sample_moves and does not combine with playout_cap, leaves_per_step > 1 or distributed=True
    (ValueError).  policy_target="improved" (needs gumbel, alias_final_boards=False and the flat policy loss) trains the policy on the
    searches' improved-policy rows softmax(logit + sigma(completed Q)); policy_target="visits" with gumbel keeps training on the raw counts.

    The optimiser's options (L2 term / decoupled weight decay, global-norm clip, learning-rate schedule, weight average) need no parameter
    here: the network object carries them -- NNetWrapper(..., optimizer=dict(...)); with use_average=True every train() commits the weight
    average, so self-play, matches, evaluations and checkpoints of the loop run on it, and copy() hands the settings to the promoted network.

    batched_evaluation=True plays the evaluation games against RandomOthelloAgent in lock step on the GPU
    (evaluate_against_random_batch) instead of one by one through the drop-in agents.

    distributed=True (torch.distributed initialised, one process per GPU): the episodes of an iteration are sharded over
    the ranks by global game id and pooled with one all-gather of move records, every rank then holds the same replay
    buffer (same `random` stream, seeded here), trains on its 1/world slice of it with one gradient all-reduce per step,
    and plays the (deterministic) matches / evaluations redundantly, so all ranks take the same promotion decisions
    without further communication; rank 0 writes the files.

    policy_target="visits" trains the policy on the search's visit distribution (the AlphaZero pi, from the root visit counts the
    engines record, at target_temperature) instead of the one-hot of the move played.  It needs alias_final_boards=False (pi belongs
    to the position of the move, not the game's final one) and a network whose policy_loss is "flat" (the reference's row-wise loss
    cannot learn how pi's mass splits between board rows).

    leaves_per_step > 1: the batched engines (self-play, matches, batched evaluation) run that many descents per game and network
    batch under virtual loss; the networks need max_batch >= games * leaves_per_step.  The drop-in evaluation agents keep 1.

    root_noise=(alpha, epsilon): Dirichlet noise on the root prior of every searched SELF-PLAY move (SelfPlayEngine), in the single-process and
    the distributed path alike; matches and evaluations stay noise-free.

    sample_moves=(temperature, plies): where the e_greedy coin falls on the greedy branch, the SELF-PLAY move of a game's first `plies`
    plies is drawn in proportion to N ** (1 / temperature) instead of taken as the arg-max (SelfPlayEngine), in both paths; matches and
    evaluations never sample.  Pure AlphaZero is e_greedy = 1.  temperature_threshold keeps its meaning.

    replay="device": the replay buffer is ONE replay.ReplayBuffer(board_size, training_buffer_size) in HBM for the run.  An iteration's
    engine plays to the end without its records being read, the buffer appends their examples device to device
    (ReplayBuffer.append_engine) and the network trains from the buffer in place (NNetWrapper.train(replay)): no example tuples, no
    random.shuffle of examples (the fit draws its own order per epoch).  The ring overwrites the OLDEST example, where the default "host"
    path keeps the reference's CircularArray + random.shuffle (which overwrites random survivors).  Matches, evaluation and promotion
    are unchanged.  Single-process, and there is no tuple list to dump: not with distributed=True or dump_examples=True.

    evaluation_opponent="random" (RandomOthelloAgent, the reference's yardstick) or ("minimax", depth) / ("minimax", depth, "discs" | "weighted"):
    who the evaluation games at `evaluation_interval` are played against, in the drop-in and the batched evaluation alike.  A network that
    wins 91 % of its games against the random agent can never be kept by the `new > old * 1.1` rule again; a fixed-depth minimax (depth 1 on
    "discs" is the reference's GreedyOthelloAgent, agents.py:27-41) is the harder opponent.  Matches between networks and self-play are untouched.

    endgame_targets=E (0 = off, the default; at most 12): once an iteration's games are over and before its records are read, the engine solves
    every record with E empties or fewer exactly on the device (SelfPlayEngine.solve_records) and rewrites its value target z to the sign of the
    final disc difference under perfect play -- in the host path, in the distributed path (each rank on its own records, before the all-gather)
    and with replay="device" (before the append).  The reference trains on played outcomes only.  Logs solved / z_changed / mean_disc_loss per
    iteration (the discs the moves played gave away against perfect play); training.endgame_history keeps the dicts.  It needs
    alias_final_boards=False.  Use 10, not the cap: on an MI355X the slowest of 64 random 8x8 positions takes 42 ms at 10 empties and 0.98 s at
    12, and relabelling 4 096 games at 10 costs 1 % of their self-play ("Endgame solver").

    solve_leaves=E (0 = off, the default; at most 10): inside every search of the batched engines -- self-play, matches and batched evaluation
    -- a leaf with E empties or fewer takes its exact win / draw / loss (+1 / 0 / -1 for the side to move, a draw is 0) in place of the
    network's value, solved on the device right after the network's batch; the priors stay the network's.  The visit counts that
    policy_target="visits" trains on and the moves that mean_disc_loss measures then come from exact values over the last plies.  The
    reference has nothing like it.  training.rows_solved counts the self-play leaves solved.  The drop-in evaluation agents stay without it.
    Use 6: on an MI355X at 4 096 games of 8x8 the solving kernel then takes 0.11 ms of a 3.8 ms network batch (174 leaves solved per batch), inside
    the run-to-run spread of the search without it; 8 costs 0.53 ms (a fifth more per batch), 10 costs 5.2 ms and more than doubles the batch
    ("Solved leaves"; tools/solve_leaves_bench.py, profiles/solve_leaves_bench.json).

    value_signs="sound" ("reference" = off, the default): every search of the batched engines -- self-play, matches and batched evaluation --
    backs its values up with the signs right across passes and finished boards: one negation per change of the side to move instead of one per
    level, and a finished board worth the sign of its disc difference to the side to move there, a draw 0.  The reference's rule stores -1 for
    a move that wins the game on the spot and flips every value that crosses a pass; the visit counts, root values, value
    targets, surprise and the resign rule all read those numbers.  Combines with every other option.  A drawn game stays +-1 in the records'
    z.  The drop-in evaluation agents stay without it ("Value signs"; tools/value_signs_bench.py).

    proofs=True (needs value_signs="sound"; False = off, the default): every search of the batched engines keeps the exact values it meets --
    finished boards, solved leaves -- as proofs, combines them at the parent (any winning move proves a win, all moves known proves their
    maximum) and backs them up the path; a descent never picks a proven loss while something else is left, takes the exact value in place of
    the averaged Q and stops at a proven position.  One setting serves self-play, the match and the batched evaluation.  The moves, visit rows
    and root values read the raw statistics as before.  Not with gumbel or forced_playouts (ValueError).  training.proof_history keeps the
    self-play engines' proof_stats() per iteration (with distributed=True: this rank's) ("Proofs"; tools/proofs_bench.py).

    selection=dict(fpu=(reduction, root_reduction), cpuct_growth=(base, factor), prior_first=bool) (None = off, the default): every search of
    the batched engines -- self-play, matches and batched evaluation -- selects with first-play urgency, a visit-scaled exploration constant
    and a prior-first first visit, each part on its own (OthelloMCTS, selection; include/othellozero_amd.h, "selection").  Not with gumbel or
    forced_playouts (ValueError).  The drop-in evaluation agents stay without it.  Playing strength is neither gated nor claimed (DESIGN.md,
    "Selection"; tools/selection_bench.py).
    tree_gc="demand" | "every" ("off" = the default): every search of the batched engines -- self-play, matches and batched evaluation --
    drops the stored nodes its games have passed (SelfPlayEngine, tree_gc; include/othellozero_amd.h, "tree collection").  No record, move
    or result changes: the option only lets a smaller node capacity suffice ("Tree collection").
    proof_play=True (needs proofs=True; False = off, the default): the searches' exact knowledge reaches the three hand-overs it stopped short
    of.  The recorded visit row keeps the raw counts of the moves the descent would still pick at the root -- those that prove a known
    value, else those not proven lost -- and every move rule that reads counts reads that row, so a move proven lost after it took most of
    the visits is neither played nor trained towards; the recorded root value (value targets, resignation) is the exact one where it is
    known; the record carries the proof code (_lib.record_proven).  The explore branch of the coin stays uniform.  One setting serves
    self-play, the match and the batched evaluation.  training.proof_play_history keeps the self-play engines' proof_play_stats() per
    iteration.  proof_targets=True (needs proof_play=True): before the endgame targets, the value targets and the appends, z of every
    proven record becomes the proven sign (SelfPlayEngine.proof_targets), and the value targets take such a record as exact.  Playing
    strength is neither gated nor claimed ("Proof play"; tools/proof_play_bench.py).

    match_openings=(plies, opening_seed) / evaluation_openings=(plies, opening_seed) (None = off, the default): the games of the new-vs-old
    match / of the batched evaluation start with random openings of `plies` plies instead of the one standard position, every opening played
    from both sides (self_play_match / evaluate_against_random_batch with openings=; DESIGN.md, "Openings").  At temperature 0 the reference's
    match is a handful of distinct games; this is not the reference's match.  The promotion rules are the same: the match still returns games
    won, counted the same way.  A match with openings also logs mean_margin +- se (discs per pair of games) and split_pairs, and
    training.match_history keeps its dicts (paired_match).  self_play_total_games must then be even; evaluation_openings needs
    batched_evaluation=True (the drop-in agents play one game at a time on the host, from the standard position).  With distributed=True every
    rank plays the whole match, as without openings.

    playout_cap=(fast_sims, full_prob) (None = off, the default): KataGo's playout cap randomization for the SELF-PLAY games (SelfPlayEngine).
    A searched move runs num_simulations simulations with probability full_prob and fast_sims otherwise; only the fully searched moves become
    training examples -- in the host path (examples_from_records drops the flagged records), in the distributed path (the flag travels inside
    the 48-byte records through the all-gather) and with replay="device" (the append leaves them out) -- while every game still ends in an
    outcome for them: more finished games per GPU-second for the value head, full-search visit distributions only for the policy head.  A
    fast move draws no root noise.  endgame_targets still relabels all records, so its mean_disc_loss measures the moves actually played, fast
    ones included.  Matches and evaluations are never capped.  The reference has nothing like it.  Use (20, 0.25) at 100 simulations, the
    one setting that has been measured: on an MI355X at 4 096 games of 8x8 it finishes 1.89 times as many games per second as the engine without
    it (2.03 times the moves at 40 simulations per move on average), while the fully searched records per second fall to 0.51 times -- a quarter
    of twice as many moves; expansions per second fall to 0.84 times because the capped games share fewer leaves for the cross-game
    de-duplication to take out ("Playout cap"; tools/playout_cap_bench.py, profiles/playout_cap_bench.json).

    forced_playouts=k (None or 0 = off, the default; KataGo uses 2; needs root_noise): forced playouts and policy target pruning for the
    SELF-PLAY searches (SelfPlayEngine), in the host path, the distributed path and with replay="device" alike.  At the noisy root every child
    tried once is searched until it has sqrt(k * Pn * Ns) visits, so a move the noise favours is examined instead of abandoned; when the move
    is played, the visits PUCT would not have granted are subtracted from the recorded row, so with policy_target="visits" the network trains
    on what the search concluded, not on how it explored.  The visit rows ARE the pruned counts then: examples_from_records, expand_examples
    and the device replay buffer read them unchanged.  The moves are still chosen from the raw counts; the fast moves of a playout cap,
    matches and evaluations are neither forced nor pruned.  The reference has nothing like it ("Forced playouts";
    tools/forced_playouts_bench.py, profiles/forced_playouts_bench.json).

    eval_symmetry=("random", s) (None = off, the default): the SELF-PLAY network of iteration i (1, 2, ...) evaluates every position in the
    dihedral symmetry oz_eval_symmetry(s + i, own, opp) of the board (NNetWrapper.set_eval_symmetry("random", s + i)), in the host path, the
    distributed path and with replay="device" alike: AlphaZero's and KataGo's random leaf symmetry as a pure function of the position, with a
    new seed per iteration, so that the orientation bias of a network that is only approximately equivariant does not repeat in every game
    and in the visit rows policy_target="visits" trains on.  The network's previous setting is back before the fit, matches and evaluation,
    which stay untouched like under every other self-play option.  "mean" (all eight orientations, 8x the network work) is for matches and
    measurements and is refused here: set it on the networks themselves with set_eval_symmetry("mean") ("Evaluation symmetry").

    value_target="outcome" (the default: z = the game's outcome, as ever), ("blend", w) or ("td", lam), w / lam in [0, 1]: the value head trains
    on targets built from the SELF-PLAY searches' root values -- the visit-weighted mean of the root's Q, which the engines then record per
    move (SelfPlayEngine(record_values=True)).  "blend": (1 - w) z + w q of the move's own search.  "td": KataGo-style short-term targets,
    TD(lam) backwards over the root values of the following plies, ending in the outcome (lam = 1 is the outcome, lam = 0 the root value).
    With endgame_targets=E the order is solve, then targets, then append: a solved record keeps its exact z and the plies before it bootstrap
    from it (exact_empties = E).  Host path, distributed path (each rank computes its own targets, 4 more bytes per row in the all-gather) and
    replay="device" (the append reads the engine's targets on the device) alike; the examples' z is then a float.  It needs
    alias_final_boards=False.  Playing strength is neither gated nor claimed ("Value targets")."""
    vt_on = _lib.check_value_target(value_target, alias_final_boards)[0] != _lib.VALUE_TARGET_OUTCOME
    training.resign_history = []
    training.surprise_history = []
    training.validation_history = []
    training.aux_history = []
    aux_heads = _lib.check_aux_heads_loop(aux_heads, replay, distributed, alias_final_boards, getattr(neural_network, "in_channels", 2))
    if aux_heads is not None:
        if not hasattr(neural_network, "set_aux_heads"):
            raise ValueError(f"aux_heads needs a network that trains auxiliary heads (NNetWrapper); {type(neural_network).__name__} has none")
        neural_network.set_aux_heads(aux_heads)
    if validation_share is not None:
        if isinstance(validation_share, bool) or not isinstance(validation_share, (int, float)) or not 0.0 < validation_share <= 0.5:
            raise ValueError(f"validation_share must be None or a share in (0, 0.5] of an iteration's new examples (got {validation_share!r})")
        if distributed:
            raise ValueError("validation_share is not offered with distributed=True: the held-out examples are slots of the device replay buffer, "
                             "which is single-process")
        if replay != "device":
            raise ValueError("validation_share needs replay='device': the held-out examples are the newest slots of the device replay buffer; the "
                             "host example path shuffles its buffer in place and has no newest part")
    if surprise_weight is not None:
        surprise_weight = _lib.check_surprise_frac(surprise_weight)
        if distributed:
            raise ValueError("surprise_weight is not offered with distributed=True: the weighted append writes into the device replay buffer, which "
                             "is single-process")
        if replay != "device":
            raise ValueError("surprise_weight needs replay='device': the weighted append writes a variable number of examples per record into the "
                             "device replay buffer; the host example path writes 8 per record")
        if policy_target not in ("visits", "improved"):
            raise ValueError("surprise_weight needs policy_target='visits' or 'improved': the surprise is that of the search's policy target, and "
                             "a one-hot target does not carry it")
    if eval_symmetry is not None:
        try:
            es_mode, es_seed = (eval_symmetry, 0) if isinstance(eval_symmetry, str) and eval_symmetry == "mean" else eval_symmetry
        except (TypeError, ValueError):
            raise ValueError(f'eval_symmetry must be None or ("random", seed), got {eval_symmetry!r}') from None
        if isinstance(es_mode, str) and es_mode == "mean":
            raise ValueError('eval_symmetry="mean" is not a self-play option (8x the network work per leaf): for matches and measurements set it on '
                             'the networks with NNetWrapper.set_eval_symmetry("mean")')
        if not isinstance(es_mode, str) or es_mode != "random":
            raise ValueError(f'eval_symmetry must be None or ("random", seed), got {eval_symmetry!r}')
        _lib.check_eval_symmetry(es_mode, es_seed)
        _lib.check_eval_symmetry(es_mode, es_seed + num_iterations)
        eval_symmetry = (es_mode, int(es_seed))
    _lib.check_opponent(evaluation_opponent)
    _lib.check_openings(match_openings)
    _lib.check_openings(evaluation_openings)
    if evaluation_openings is not None and not batched_evaluation:
        raise ValueError("evaluation_openings needs batched_evaluation=True: the drop-in evaluation agents play from the standard position")
    if match_openings is not None and self_play_training and (self_play_total_games % 2 or self_play_total_games < 2):
        raise ValueError(f"match_openings plays pairs of games: self_play_total_games must be even and >= 2 (got {self_play_total_games})")
    training.match_history = []
    training.proof_history = []
    training.proof_play_history = []
    training.rows_solved = 0
    endgame_targets = _lib.check_endgame_targets(endgame_targets, alias_final_boards)
    training.endgame_history = []
    if replay not in ("host", "device"):
        raise ValueError(f"replay must be 'host' or 'device' (got {replay!r})")
    if replay == "device" and distributed:
        raise ValueError("replay='device' is single-process: the data-parallel fit has no entry point that reads the device buffer yet "
                         "(use replay='host' with distributed=True)")
    if replay == "device" and dump_examples:
        raise ValueError("replay='device' keeps no example tuples to dump: use replay='host' with dump_examples=True, or ReplayBuffer.save")
    visits = policy_target == "visits"
    o = _lib.check_selfplay_options(num_simulations, visits, leaves_per_step, root_noise, sample_moves, solve_leaves, playout_cap, forced_playouts,
                                    vt_on, gumbel, False, resign, value_signs, proofs, proof_play, selection, tree_gc)
    o["record_surprise"] = surprise_weight is not None     # (past the engine's rule for it: the loop's own, above, say what it needs here)
    gumbel = _lib.check_gumbel_options(o["gumbel"], distributed=distributed)
    proof_targets = _lib.check_proof_targets(proof_targets, o["proof_play"])
    search = _lib.search_kw(o)                              # what the match and the batched evaluation share with self-play
    engine_options = {k: v for k, v in o.items() if not k.startswith("record_")}       # (the record_* flags: the two wrappers set them)
    if policy_target not in ("onehot", "visits", "improved"):
        raise ValueError(f"policy_target must be 'onehot', 'visits' or 'improved' (got {policy_target!r})")
    improved = policy_target == "improved"
    if improved and gumbel is None:
        raise ValueError("policy_target='improved' needs gumbel=(max_considered, c_visit, c_scale): the improved policy is the Gumbel search's")
    if improved and alias_final_boards:
        raise ValueError("policy_target='improved' needs alias_final_boards=False: an improved policy belongs to the position of its "
                         "move, not to the game's final position")
    if improved and getattr(neural_network, "policy_loss", "rows") != "flat":
        raise ValueError("policy_target='improved' needs a network trained with the flat policy loss: create it with "
                         "NNetWrapper(..., policy_loss='flat')")
    if visits and alias_final_boards:
        raise ValueError("policy_target='visits' needs alias_final_boards=False: a visit distribution belongs to the position of its "
                         "move, not to the game's final position")
    if visits and getattr(neural_network, "policy_loss", "rows") != "flat":
        raise ValueError("policy_target='visits' needs a network trained with the flat policy loss: create it with "
                         "NNetWrapper(..., policy_loss='flat') (the row-wise loss renormalises every board row on its own)")
    if visits and not target_temperature > 0:
        raise ValueError(f"target_temperature must be > 0 (got {target_temperature})")
    if self_play_training:
        assert self_play_threshold <= self_play_total_games, 'Self-play threshold must be less than self-play games'

    world, rank, allreduce = 1, 0, None
    if distributed:
        import torch
        import torch.distributed as dist
        from .distributed import GradientAllReduce, pooled_selfplay_records, shard_games
        from .training import SelfPlayEngine
        world, rank = dist.get_world_size(), dist.get_rank()
        assert num_episodes >= world, "fewer episodes than ranks"
        device = torch.device("cuda", torch.cuda.current_device())
        # pin the library to the device torch selected for this rank (objects created on this thread from here on)
        _lib.check(_lib.load().oz_set_device(torch.cuda.current_device()))
        allreduce = GradientAllReduce(board_size, neural_network.num_channels, neural_network.in_channels, device=device)
        random.seed(seed)

    def save(net):
        if rank == 0:
            net.save_checkpoint(checkpoint_filepath)

    historic = []
    total_episodes_done = 0
    training_examples = CircularArray(training_buffer_size)
    device_replay = None
    if replay == "device":
        from .replay import ReplayBuffer
        device_replay = ReplayBuffer(board_size, training_buffer_size, aux=True) if aux_heads is not None else ReplayBuffer(board_size, training_buffer_size)
    old_neural_network = neural_network.copy()
    for i in range(1, num_iterations + 1):
        logging.info('[%d/%d] begin', i, num_iterations)
        if temperature_threshold and i >= temperature_threshold:
            logging.info('[%d/%d] past the temperature threshold: moves are now the arg-max of the visit counts', i, num_iterations)
            temperature = 0

        logging.info('[%d/%d] self-play: %d games x %d simulations on the GPU', i, num_iterations, num_episodes, num_simulations)
        es_previous = None
        if eval_symmetry is not None:                      # this iteration's self-play only: restore_eval_symmetry() precedes every fit
            es_previous = neural_network.eval_symmetry()
            neural_network.set_eval_symmetry(eval_symmetry[0], eval_symmetry[1] + i)

        def restore_eval_symmetry(net=neural_network, previous=es_previous):
            if previous is not None:
                net.set_eval_symmetry(*previous)
        if device_replay is not None:
            total_before = device_replay.total if validation_share is not None else 0
            appended, stats = _selfplay_into_replay(device_replay, neural_network, board_size, num_episodes, num_simulations,
                                                    degree_exploration, temperature, e_greedy, seed, total_episodes_done, q_mode, visits,
                                                    alias_final_boards=alias_final_boards, policy_target=policy_target,
                                                    target_temperature=target_temperature, endgame_targets=endgame_targets,
                                                    value_target=value_target, proof_targets=proof_targets,
                                                    surprise_weight=None if surprise_weight is None else (surprise_weight, seed + i),
                                                    **engine_options)
            _publish_selfplay_stats(i, num_iterations, stats)
            total_episodes_done += num_episodes
            logging.info('[%d/%d] self-play done: %d records, device buffer holds %d examples', i, num_iterations, appended, len(device_replay))
            restore_eval_symmetry()
            logging.info('[%d/%d] fit on the device buffer', i, num_iterations)
            if validation_share is not None:
                hist = _fit_with_holdout(i, num_iterations, neural_network, device_replay, total_before, validation_share)
            else:
                hist = neural_network.train(device_replay, verbose=2 if logging.root.level <= logging.DEBUG else None)
            if aux_heads is not None and hist is not None and hist.history.get("ownership_loss"):
                training.aux_history.append({k: hist.history[k][-1] for k in ("ownership_loss", "score_loss")})
                logging.info('[%d/%d] auxiliary heads: ownership_loss %.4f score_loss %.4f', i, num_iterations,
                             hist.history["ownership_loss"][-1], hist.history["score_loss"][-1])
        else:
            if distributed:
                first, count = shard_games(num_episodes, rank, world)
                eng = SelfPlayEngine(neural_network, board_size, count, num_simulations, degree_exploration, temperature, e_greedy,
                                     seed=seed, first_game_id=total_episodes_done + first, q_mode=q_mode,
                                     **_lib.engine_kw(o, always=_ENGINE_ALWAYS))
                eng.play_to_end(endgame_targets=endgame_targets, value_target=value_target,      # each rank relabels its own records (and
                                proof_targets=proof_targets)                                       # computes its targets)
                stats = eng.option_stats()
                records = pooled_selfplay_records(eng, device, with_visits=visits, with_values=vt_on)   # the only exchange of the self-play phase
                del eng
            else:
                records = selfplay_batch(neural_network, board_size, num_games=num_episodes, num_simulations=num_simulations,
                                         degree_exploration=degree_exploration, policy_temperature=temperature, e_greedy=e_greedy,
                                         seed=seed, first_game_id=total_episodes_done, q_mode=q_mode, record_visits=visits,
                                         endgame_targets=endgame_targets, value_target=value_target, proof_targets=proof_targets, **engine_options)
                stats = {name: getattr(selfplay_batch, name, None) for name in ("rows_solved", "endgame_stats") + _STATS_PUBLISHED}
            restore_eval_symmetry()
            _publish_selfplay_stats(i, num_iterations, stats)
            counts = targets = policies = None
            if gumbel is not None:                             # the improved-policy rows come last
                policies, records = records[-1], (records[0] if len(records) == 2 else records[:-1])
            if vt_on:
                records, targets = (records[0], records[-1]) if not visits else ((records[0], records[1]), records[2])
            if visits:
                records, counts = records
            training_examples.extend(examples_from_records(records, board_size, alias_final=alias_final_boards,
                                                           in_channels=getattr(neural_network, "in_channels", 2), visits=counts,
                                                           target_temperature=target_temperature, **({"values": targets} if vt_on else {}),
                                                           **({"policies": policies} if improved else {})))
            total_episodes_done += num_episodes
            logging.info('[%d/%d] self-play done: %d records, buffer holds %d examples', i, num_iterations, len(records), len(training_examples))

            logging.info('[%d/%d] fit on the buffer', i, num_iterations)
            random.shuffle(training_examples)
            verbose = 2 if logging.root.level <= logging.DEBUG else None
            if distributed:
                usable = len(training_examples) - len(training_examples) % world     # equal step counts on every rank
                neural_network.train([training_examples[j] for j in range(rank, usable, world)], verbose=verbose, allreduce=allreduce)
            else:
                neural_network.train(training_examples, verbose=verbose)

        if self_play_training and i % self_play_interval == 0:
            logging.info('[%d/%d] arena: trained network against the previous one', i, num_iterations)
            new_net_victories = self_play_match(board_size, neural_network, old_neural_network, self_play_total_games,
                                                num_simulations, degree_exploration, seed=seed + i, leaves_per_step=leaves_per_step,
                                                **search, **({"openings": match_openings} if match_openings is not None else {}))
            if match_openings is not None:
                stats = self_play_match.stats
                training.match_history.append(stats)
                logging.info('[%d/%d] arena: mean_margin %+.2f +- %.2f discs per pair over %d openings, split_pairs %d', i, num_iterations,
                             stats["mean_margin"], stats["se"], stats["pairs"], stats["split_pairs"])
            logging.info('[%d/%d] arena: %d of %d games to the trained network', i, num_iterations, new_net_victories, self_play_total_games)
            if new_net_victories >= self_play_threshold:
                logging.info('[%d/%d] trained network promoted', i, num_iterations)
                save(neural_network)
                logging.info('[%d/%d] checkpoint -> %s', i, num_iterations, checkpoint_filepath)
                old_neural_network = neural_network if reference_aliasing else neural_network.copy()
            else:
                neural_network = old_neural_network if reference_aliasing else old_neural_network.copy()
                logging.info('[%d/%d] trained network rejected, previous one kept', i, num_iterations)
        else:
            save(neural_network)

        if i % evaluation_interval == 0:
            logging.info('[%d/%d] evaluation against %s: current network', i, num_iterations,
                         'the random agent' if _lib.check_opponent(evaluation_opponent) is None else f'{evaluation_opponent!r}')
            if batched_evaluation:
                new = evaluate_against_random_batch(board_size, neural_network, evaluation_iterations, num_simulations,
                                                    degree_exploration, seed=seed + 7919 * i, leaves_per_step=leaves_per_step,
                                                    opponent=evaluation_opponent, **search,
                                                    **({"openings": evaluation_openings} if evaluation_openings is not None else {}))
                old = evaluate_against_random_batch(board_size, old_neural_network, evaluation_iterations, num_simulations,
                                                    degree_exploration, seed=seed + 7919 * i + 1, leaves_per_step=leaves_per_step,
                                                    opponent=evaluation_opponent, **search,
                                                    **({"openings": evaluation_openings} if evaluation_openings is not None else {}))
            else:
                new = evaluate_against_random(board_size, neural_network, evaluation_iterations, num_simulations, degree_exploration,
                                              label=f'after {total_episodes_done} episodes, current network', opponent=evaluation_opponent)
                logging.info('[%d/%d] evaluation against the random agent: previous network', i, num_iterations)
                old = evaluate_against_random(board_size, old_neural_network, evaluation_iterations, num_simulations, degree_exploration,
                                              label=f'after {total_episodes_done} episodes, previous network', opponent=evaluation_opponent)
            if new["wins"] > (old["wins"] * 1.1):
                logging.info('[%d/%d] evaluation: current network kept (%d wins vs %d)', i, num_iterations, new['wins'], old['wins'])
                historic.append((total_episodes_done, (new["wins"] / evaluation_iterations)))
                save(neural_network)
                old_neural_network = neural_network if reference_aliasing else neural_network.copy()
            else:
                logging.info('[%d/%d] evaluation: back to the previous network (%d wins vs %d)', i, num_iterations, new['wins'], old['wins'])
                historic.append((total_episodes_done, (old["wins"] / evaluation_iterations)))
                save(old_neural_network)
                neural_network = old_neural_network if reference_aliasing else old_neural_network.copy()
            logging.info('history (episodes, win rate): %s', historic)

        logging.info('[%d/%d] end: %d episodes so far', i, num_iterations, total_episodes_done)
        if dump_examples and rank == 0:
            with open(f'examples-{board_size}.txt', 'w') as output:
                output.write(str(training_examples))
        if rank == 0:
            with open(f'historic-last-training-session-{board_size}.txt', 'w') as output:
                output.write(str(historic))

    training.last_network = neural_network
    return historic
