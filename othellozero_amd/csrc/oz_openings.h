// oz_openings.h -- openings for arena games: the first plies of a game played from the standard position before any search runs (gfx950).
// The reference has none: every duel_between_agents game starts from the one standard position (agents.py:71-84), and at temperature 0 the games
// of a match between two sharp networks are then one game per colour, played many times.  An opening suite -- every opening played twice, colours
// swapped -- is the standard remedy in engine testing.  Shared by the batch entry oz_rules_random_openings (oz_rules.hip), the arena's
// k_arena_openings (oz_search.hip) and, on the host, oz_arena_set_opening_moves' replay of the lists it is given.  Integer arithmetic only.
//
// An opening is keyed (opening_seed, opening id), NEVER by the game's seed or id: two arenas given the same (opening_seed, first_opening_id) face
// the same openings whoever plays them.  Random mode: the move of ply p is oz_kth_bit(legal, oz_rng(opening_seed, opening id, p, OZ_RNG_OPENING) %
// popcount(legal)) for whoever oz_game_play left to move -- k_arena_random_move's shape on a stream of its own.  List mode: the move of ply p is
// moves[p] (legality is the caller's business: the arena checks every list on the host before the kernel sees it).  oz_game_play handles passes
// (one side may move twice in a row); a game that ends inside its opening stays finished with fewer plies played than asked for.
#pragma once
#include "oz_common.h"

// what k_arena_openings needs besides the games: random mode (moves == nullptr: `plies` plies for every game) or list mode (moves[g][16], n_plies[g])
struct OpeningsDev {
    int plies;
    uint64_t seed, first_id;                   // the opening id of slot g is first_id + g
    const uint8_t* moves;                      // [G][OZ_OPENING_MAX_PLIES] squares row*8+col, or null
    const int32_t* n_plies;                    // [G], list mode
    int32_t* opening_plies;                    // [G] out: plies played (fewer than asked for where the game ended first)
};

OZ_HD void oz_initial_board(int n, uint64_t& black, uint64_t& white) {     // Othello/__init__.py:177-184
    const int h = n / 2;
    white = (1ULL << ((h - 1) * 8 + h - 1)) | (1ULL << (h * 8 + h));
    black = (1ULL << ((h - 1) * 8 + h)) | (1ULL << (h * 8 + h - 1));
}

// Plays the opening on a position held in registers: sets the standard position with BLACK to move, then moves while ply < plies and the game is
// not finished.  report(ply, black, white, player, action) is called for every ply BEFORE its move is made (the position and mover of the move,
// what a move log holds).  -> plies played.
template <typename Report>
OZ_HD int oz_opening_play(int n, uint64_t valid, int plies, const uint8_t* moves, uint64_t opening_seed, uint64_t opening_id,
                          uint64_t& black, uint64_t& white, int& player, int& finished, Report report) {
    oz_initial_board(n, black, white);
    player = 1; finished = 0;
    int ply = 0;
    while (ply < plies && !finished) {
        int action;
        if (moves) action = moves[ply];
        else {
            const uint64_t legal = oz_legal(player == 1 ? black : white, player == 1 ? white : black, valid);
            action = oz_kth_bit(legal, (int)(oz_rng(opening_seed, opening_id, (uint64_t)ply, OZ_RNG_OPENING) % (uint64_t)oz_popc(legal)));
        }
        report(ply, black, white, player, action);
        oz_game_play(black, white, player, finished, action, valid);
        ++ply;
    }
    return ply;
}
