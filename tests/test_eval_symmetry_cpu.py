"""The evaluation symmetry without a GPU: the new symbols in header, bindings and library; oz_sym_boards and oz_eval_symmetries (the
functions the kernels evaluate, run on the host) against the restatement in tests/eval_symmetry_ref.py, bit for bit; the properties of the
transform and of the selection; check_eval_symmetry; and that the searches and games the GPU test compares are not vacuous."""
import os
import re

import numpy as np
import pytest

import eval_symmetry_ref as ref
import minimax_ref as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["oz_net_set_eval_symmetry", "oz_net_get_eval_symmetry", "oz_net_eval_symmetry_profile", "oz_eval_symmetries", "oz_sym_boards"]
SEEDS = (0, 5, 0xDEADBEEFCAFEF00D)


def _boards(n):
    """every board of a few seeded playouts (both colours, the occupied set) and the single-bit boards of every cell"""
    out = []
    for own, opp in ref.positions(n):
        out += [own, opp, own | opp]
    return list(dict.fromkeys(out)) + [1 << (r * 8 + c) for r in range(n) for c in range(n)]


def _corner(n):
    return sum(1 << (r * 8 + c) for r in range(n) for c in range(n))


def test_new_symbols_in_header_bindings_and_library():
    from othellozero_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "othellozero_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "---- evaluation symmetry" in header
    assert re.search(r"OZ_EVAL_SYM_OFF = 0, OZ_EVAL_SYM_RANDOM = 1, OZ_EVAL_SYM_MEAN = 2", header)
    assert (_lib.EVAL_SYM_OFF, _lib.EVAL_SYM_RANDOM, _lib.EVAL_SYM_MEAN) == (0, 1, 2)
    with open(os.path.join(ROOT, "othellozero_amd", "csrc", "oz_common.h")) as f:
        common = f.read()
    assert re.search(r"\bint oz_eval_symmetry\(", common) and re.search(r"\buint64_t oz_sym_board\(", common)
    assert lib.oz_version() == 230


@pytest.mark.parametrize("n", [4, 6, 8])
def test_sym_boards_vs_restatement(n):
    from othellozero_amd.agents import rules_sym_boards
    boards = _boards(n)
    assert len(boards) >= 100 + n * n
    b = np.array(boards, np.uint64)
    corner = _corner(n)
    for t in range(8):
        got = rules_sym_boards(b, n, t)
        assert got.dtype == np.uint64 and got.shape == b.shape
        want = [ref.sym_board(t, n, x) for x in boards]
        assert got.tolist() == want, (n, t)
        assert all(int(x) & ~corner == 0 for x in got), (n, t)                 # nothing outside the n x n corner
        assert [mm.popcount(int(x)) for x in got] == [mm.popcount(x) for x in boards]
        back = rules_sym_boards(got, n, ref.inverse(t, n))                    # t, then its inverse
        assert np.array_equal(back, b), (n, t)
    assert np.array_equal(rules_sym_boards(b, n, ref.IDENTITY), b)            # t = 7 is the identity
    assert any(not np.array_equal(rules_sym_boards(b, n, t), b) for t in range(7))
    # one t per board, and bits outside the corner of the input are dropped
    ts = np.arange(b.size, dtype=np.int32) % 8
    assert rules_sym_boards(b, n, ts).tolist() == [ref.sym_board(int(t), n, x) for t, x in zip(ts, boards)]
    if n < 8:
        dirty = b | np.uint64(~corner & ref.M64)
        assert np.array_equal(rules_sym_boards(dirty, n, ts), rules_sym_boards(b, n, ts))


def test_sym_boards_is_the_training_symmetry_table():
    """the orientation numbering is oz_symmetry_table's: a single bit at cell perm[t][j] lands on cell j"""
    from othellozero_amd import _lib
    from othellozero_amd.agents import rules_sym_boards
    for n in (4, 6, 8):
        perm = np.zeros((8, n * n), np.int32)
        _lib.check(_lib.load().oz_symmetry_table(n, _lib.p_i32(perm)))
        assert perm.tolist() == [list(p) for p in ref.perms(n)]
        for t in range(8):
            src = np.array([1 << ((int(s) // n) * 8 + int(s) % n) for s in perm[t]], np.uint64)
            assert rules_sym_boards(src, n, t).tolist() == [1 << ((j // n) * 8 + j % n) for j in range(n * n)]


def test_sym_boards_refusals():
    from othellozero_amd import _lib
    lib = _lib.load()
    b, out = np.array([1, 2], np.uint64), np.zeros(2, np.uint64)
    for bad in (-1, 8, 100):
        t = np.array([7, bad], np.int32)
        assert lib.oz_sym_boards(_lib.p_i32(t), 6, _lib.p_u64(b), 2, _lib.p_u64(out)) == _lib.OZ_ERR_ARG
    t = np.array([7, 0], np.int32)
    for n in (3, 5, 7, 9):
        assert lib.oz_sym_boards(_lib.p_i32(t), n, _lib.p_u64(b), 2, _lib.p_u64(out)) == _lib.OZ_ERR_ARG
    assert lib.oz_sym_boards(_lib.p_i32(t), 6, _lib.p_u64(b), -1, _lib.p_u64(out)) == _lib.OZ_ERR_ARG
    assert lib.oz_sym_boards(None, 6, None, 0, None) == 0
    assert lib.oz_eval_symmetries(0, None, None, 0, None) == 0
    assert lib.oz_eval_symmetries(0, None, None, 1, None) == _lib.OZ_ERR_ARG


@pytest.mark.parametrize("n", [4, 6, 8])
def test_eval_symmetries_vs_restatement(n):
    from othellozero_amd.agents import rules_eval_symmetries
    pos = ref.positions(n)
    own, opp = [p[0] for p in pos], [p[1] for p in pos]
    for seed in SEEDS:
        got = rules_eval_symmetries(own, opp, seed)
        assert got.dtype == np.int32 and got.tolist() == [ref.symmetry(seed, o, p) for o, p in pos], (n, seed)


def _many_positions():
    pos = ref.positions(8, 99, 90)
    assert len(pos) >= 4000
    return pos


def test_selection_is_uniform_and_seeded():
    """over >= 4 000 distinct positions every orientation takes 10 % .. 15 % (the binomial sigma at 4 000 is 0.52 %: +-5 sigma around 12.5 %),
    for the restatement alone and for the library; two seeds disagree on more than half of the positions"""
    from othellozero_amd.agents import rules_eval_symmetries
    pos = _many_positions()
    own, opp = [p[0] for p in pos], [p[1] for p in pos]
    per_seed = []
    for seed in SEEDS:
        want = np.array([ref.symmetry(seed, o, p) for o, p in pos])
        share = np.bincount(want, minlength=8) / len(pos)
        assert share.min() >= 0.10 and share.max() <= 0.15, (seed, share)       # the restatement alone
        got = rules_eval_symmetries(own, opp, seed)
        assert np.array_equal(got, want), seed
        per_seed.append(got)
    for a in range(len(SEEDS)):
        for b in range(a + 1, len(SEEDS)):
            assert np.mean(per_seed[a] != per_seed[b]) > 0.5, (a, b)


def test_check_eval_symmetry():
    from othellozero_amd import _lib
    assert _lib.check_eval_symmetry(None) == (0, 0) and _lib.check_eval_symmetry("off", 3) == (0, 3)
    assert _lib.check_eval_symmetry("random", 5) == (1, 5) and _lib.check_eval_symmetry("mean") == (2, 0)
    assert _lib.check_eval_symmetry("random", np.int64(9)) == (1, 9) and _lib.check_eval_symmetry("random", 2 ** 64 - 1) == (1, 2 ** 64 - 1)
    for bad in ("Random", "", 1, 0, True, b"random", ("random", 1), 2.0):
        with pytest.raises(ValueError, match="mode"):
            _lib.check_eval_symmetry(bad)
    for bad in (-1, 2 ** 64, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="seed"):
            _lib.check_eval_symmetry("random", bad)


def test_wrapper_is_equivariant_where_the_inner_evaluator_is():
    """the restatement's own sanity: over an inner evaluator that IS equivariant, the wrapper changes nothing but rounding-free placement"""
    n = 6

    def inner(own, opp, nn):          # pi = the mover's discs as numbers, v = a symmetric function: equivariant under every orientation
        pi = np.array([(own >> ((j // nn) * 8 + j % nn)) & 1 for j in range(nn * nn)], np.float32)
        return pi.reshape(nn, nn), np.float32(mm.popcount(own) - mm.popcount(opp))
    for own, opp in ref.positions(n)[:40]:
        want = inner(own, opp, n)
        for mode in ("random", "mean"):
            pi, v = ref.evaluator(mode, 3, inner)(own, opp, n)
            assert np.array_equal(pi, want[0]) and v == want[1], mode


@pytest.mark.parametrize("name", list(ref.SEARCH_CASES))
def test_the_searches_of_the_gpu_test_are_not_vacuous(name):
    """under the wrapped stub evaluator every root's table differs from the plain stub's, and most positions were evaluated in another
    orientation than the identity"""
    n, mode, K, sims = ref.SEARCH_CASES[name]
    roots = ref.search_roots(name)
    assert len(roots) == 4 and len(set(roots)) == 4
    tables, ev = ref.search_reference(name)
    assert ev.calls >= 4 * sims // 2 and ev.moved >= ev.calls // 2, (ev.calls, ev.moved)
    for wrapped, plain in tables:
        if K == 1:
            assert not ref.same_tables(wrapped, plain)
        else:
            sig = [[(nd.own, nd.opp, nd.Ns, sorted(nd.N.items()), sorted(nd.Q.items()), sorted(nd.P.items())) for nd in w.nodes] for w in (wrapped, plain)]
            assert sig[0] != sig[1]


def test_the_games_of_the_gpu_test_are_not_vacuous():
    """the 64 self-play games over the wrapped stub: most differ from the games over the plain stub, and from those of a second seed"""
    import oracle
    E = ref.EP
    eps, ev = ref.episodes()
    assert ev.moved >= ev.calls // 2
    differ = 0
    for g, ep in enumerate(eps[:8]):
        twin = oracle.Mcts(E["n"], E["c"], 1, salt=E["salt"]).episode(E["sims"], E["T"], E["e_greedy"], E["seed"], E["first"] + g)
        differ += not (twin["n_moves"] == ep["n_moves"] and np.array_equal(twin["action"], ep["action"]))
    assert differ >= 6
