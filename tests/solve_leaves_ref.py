"""Restatement of the solved leaves (include/othellozero_amd.h, "solved leaves"): an evaluator wrapper for the references that take one --
oracle.Mcts(evaluator=...), oracle.arena, Mcts.episode, wide_search_ref.WideSearch(evaluator=...).  A position with at most E empties
keeps the inner evaluator's pi and gets v = float(sign(S)), S the exact value for the side to move from tests/endgame_ref.py (a memoised
negamax without pruning); a draw is 0.0.  Every other position is the inner evaluator's."""
import numpy as np

import endgame_ref as eg
import oracle


def sign(x):
    return (x > 0) - (x < 0)


def exact_sign(own, opp, n):
    """sign of S for `own` to move (after the pass where own has no move)"""
    return sign(eg.value(own, opp, 1, n))


def stub(salt=0, keep_mask=0):
    """the oracle's stub network as an evaluator callable"""
    def inner(own, opp, n):
        return oracle.stub_predict(own, opp, n, salt, keep_mask)
    return inner


class evaluator:
    """evaluator(E, inner)(own, opp, n) -> (pi, v); .calls / .solved / .draws count the evaluations, the solved ones and the draws among them"""

    def __init__(self, E, inner):
        self.E, self.inner = int(E), inner
        self.calls = self.solved = self.draws = 0

    def __call__(self, own, opp, n):
        own, opp = int(own), int(opp)
        pi, v = self.inner(own, opp, n)
        self.calls += 1
        if n * n - eg.ref.popcount(own | opp) <= self.E:
            s = exact_sign(own, opp, n)
            self.solved += 1
            self.draws += s == 0
            v = np.float32(float(s))
        return pi, v
