"""CPU-side checks of the whole-game beam solver (include/tpl_learn.h's rule, tpl_placement_solve in csrc/learn/solve.hip,
_learn_lib.placement_solve, solve.py's solve_configs and tighten_pool, ForwardGames(solver=...)):

  1. the mirror with a beam wide enough to keep everything finds a win at exactly the ply at which an exhaustive enumeration with
     the C oracle's moves first finds one;
  2. every solution the mirror reports wins, played through the C oracle, after exactly solution_len moves;
  3. a fixed carved set at L = 10 / M = 40 is solved whole by CLASSICAL_WEIGHTS at width 8, with solutions longer than a window;
  4. order and ties: under weights that make whole plies tie (all +0, all -0, one integer weight) the mirror is the rule as the
     header words it, stated plainly on the oracle's moves;
  5. the recorded mirror outputs that the GPU tests compare the kernel with are the mirror's as it stands (a slice of every case);
  6. tighten_pool's arithmetic, the Python refusals, ForwardGames' solver names, every refusal of the entry, its symbol and its
     kernel's resources -- none of which needs a GPU.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

import tetris_piclim as T


def _m():
    return T._learn_lib


CW = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)


def _placements(piece):
    m = _m()
    return np.flatnonzero(m.canonical_actions(int(piece) & 7, np.arange(40)) == np.arange(40)).tolist()


class Node:
    """One game on the C oracle that can be copied: board, counters and how many pieces were played."""

    def __init__(self, O, L, M, rows, pieces, lines=0, moves=0, state=0, played=0, path=()):
        self.O, self.L, self.M, self.pieces, self.played, self.path = O, L, M, pieces, played, path
        self.g = O.Game(L, M, rows=rows, pieces=pieces[played:], lines_cleared=lines, moves_used=moves, state=state)

    def child(self, b):
        g = self.g
        c = Node(self.O, self.L, self.M, g.rows, self.pieces, g.lines_cleared, g.moves_used, g.state, self.played, self.path + (b,))
        c.g.move(b // 10, b % 10)                              # plays pieces[played]
        c.played += 1
        return c

    running = property(lambda self: self.g.state == 0)
    won = property(lambda self: self.g.state == 1)


def _replay(O, L, M, rows, pieces, actions, length):
    g = O.Game(L, M, rows=rows, pieces=pieces)
    for j in range(length):
        assert g.state == 0, ("finished before the solution's end", j)
        g.move(int(actions[j]) // 10, int(actions[j]) % 10)
    return g.state, g.moves_used


def test_the_classical_weights_are_the_probes_row():
    assert T.CLASSICAL_WEIGHTS.dtype == np.float32 and T.CLASSICAL_WEIGHTS.shape == (12,)
    assert np.array_equal(T.CLASSICAL_WEIGHTS.view(np.uint32), CW.view(np.uint32))
    assert not T.CLASSICAL_WEIGHTS.flags.writeable
    probe = open(os.path.join(ROOT, "tools", "learner_probe.py")).read()
    assert "classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)" in probe


# ------------------------------------------------------------------------------------------------ 1. exhaustive search
def _first_winning_ply(O, L, M, rows, pieces):
    """Breadth first over the distinct placements: the first ply at which any sequence of moves wins, 0 if none does."""
    level = [Node(O, L, M, rows, pieces)]
    for ply in range(1, M + 1):
        nxt = []
        for node in level:
            for b in _placements(pieces[ply - 1]):
                c = node.child(b)
                if c.won:
                    return ply
                if c.running:
                    nxt.append(c)
        level = nxt
        if not level:
            return 0
    return 0


@pytest.mark.parametrize("L,M,game_L,count", [(1, 1, 1, 24), (1, 2, 1, 24), (2, 2, 1, 24), (2, 2, 2, 24), (2, 3, 2, 6), (2, 3, 1, 6)])
def test_a_beam_that_keeps_everything_is_the_exhaustive_search(oracle, L, M, game_L, count):
    """Boards carved for `game_L` lines, searched for L: with L > game_L many have no win within M moves."""
    m = _m()
    rows, pieces = T.generate_configs(game_L, M, count, seed=31 + M)
    width = 34 ** (M - 1)
    solved, length, actions, _ = m.placement_solve(rows, pieces, L, M, CW, width, max_width=width)
    want = np.array([_first_winning_ply(oracle, L, M, rows[i], pieces[i]) for i in range(count)])
    assert np.array_equal(length, want), (length.tolist(), want.tolist())
    assert np.array_equal(solved, (want > 0).astype(np.uint8))
    if L == game_L:
        assert solved.all()                                    # carved for this game: winnable by construction
    if (L, M, game_L) == (2, 2, 1):
        assert not solved.all()
    with pytest.raises(ValueError, match="width"):            # the wide beam is for this test: the rule's limit is 64
        m.placement_solve(rows, pieces, L, M, CW, 65)


# ------------------------------------------------------------------------------------------------ 2. solutions win
@pytest.mark.parametrize("L,M,width,synthetic", [(1, 1, 1, False), (2, 6, 3, False), (2, 6, 1, True), (3, 13, 4, True), (5, 20, 2, True)])
def test_every_solved_solution_wins_on_the_oracle_after_exactly_its_length(oracle, L, M, width, synthetic):
    m = _m()
    n = 32
    if synthetic:
        rows, pieces = oracle.synth_boards(5, 0, n, L), oracle.synth_pieces(5, 0, n, M)
    else:
        rows, pieces = T.generate_configs(L, M, n, seed=5)
    solved, length, actions, best = m.placement_solve(rows, pieces, L, M, CW, width)
    assert solved.dtype == np.uint8 and length.dtype == np.int32 and actions.dtype == np.uint8 and best.dtype == np.float32
    assert actions.shape == (n, M) and best.shape == (n, M) and actions.flags.c_contiguous and best.flags.c_contiguous
    assert solved.any()
    for i in range(n):
        if solved[i]:
            state, moves = _replay(oracle, L, M, rows[i], pieces[i], actions[i], length[i])
            assert state == 1 and moves == length[i] and 1 <= length[i] <= M, (i, state, moves, length[i])
            assert (actions[i, length[i]:] == 255).all() and (actions[i, :length[i]] < 40).all()
        else:
            assert length[i] == 0 and (actions[i] == 255).all()
    if (L, M, width) == (2, 6, 1):
        assert not solved.all()                                # the unsolved form is exercised


# ------------------------------------------------------------------------------------------------ 3. a fixed carved set
def test_the_classical_weights_at_width_8_solve_a_fixed_carved_set_past_the_window(oracle):
    """L = 10 / M = 40, 16 configurations of seed 7: chosen while the test was written; every one is solved and most solutions are
    longer than the twelve entries of a window, so the piece list is read past them and across the refill at ten moves."""
    m = _m()
    L, M, n = 10, 40, 16
    rows, pieces = T.generate_configs(L, M, n, seed=7)
    solved, length, actions, _ = m.placement_solve(rows, pieces, L, M, T.CLASSICAL_WEIGHTS, 8)
    assert solved.all()
    assert (length > 12).sum() >= n // 2 and length.max() <= M
    for i in range(n):
        assert _replay(oracle, L, M, rows[i], pieces[i], actions[i], length[i]) == (1, length[i])


# ------------------------------------------------------------------------------------------------ 4. order and ties
def _plain_solve(O, L, M, rows, pieces, w, width):
    """The rule as the header words it, one configuration, on the oracle's moves: candidates in order, the first won one in
    (value descending, index ascending; -0 = +0), else the `width` best kept in candidate order."""
    m = _m()

    def better(values, i, j):
        return values[i] > values[j] or (values[i] == values[j] and i < j)

    beam, best_value = [(Node(O, L, M, rows, pieces), np.float32(0.0))], []
    for ply in range(1, M + 1):
        cand = []
        for node, value in beam:
            if not node.running:
                cand.append((node, value))
                continue
            for b in _placements(pieces[ply - 1]):
                c = node.child(b)
                psi = np.concatenate([[c.g.lines_cleared, int(c.won), int(c.g.state >= 2)], m.board_features(c.g.rows)[0]])
                cand.append((c, m.placement_score(psi, w)))
        values = [float(v) for _, v in cand]
        order = []
        for i in range(len(cand)):                             # insertion sort under `better`
            at = 0
            while at < len(order) and better(values, order[at], i):
                at += 1
            order.insert(at, i)
        best_value.append(cand[order[0]][1])
        won = [i for i in order if cand[i][0].won]
        if won:
            return 1, ply, list(cand[won[0]][0].path), best_value
        beam = [cand[i] for i in sorted(order[:width])]
        if not any(node.running for node, _ in beam):
            break
    return 0, 0, [], best_value


def test_first_in_order_takes_the_lowest_index_among_equals_and_zeros_tie():
    first = _m()._first_in_order
    assert first(np.array([0.0, -0.0, 0.0], np.float32)) == 0
    assert first(np.array([-0.0, 0.0], np.float32)) == 0
    assert first(np.array([-1.0, -0.0, 0.0, -0.0], np.float32)) == 1
    assert first(np.array([2.0, 3.0, 3.0, 1.0], np.float32)) == 1


@pytest.mark.parametrize("name,w", [("all +0", np.zeros(12, np.float32)), ("all -0", np.full(12, -0.0, np.float32)),
                                    ("holes alone, the rest -0", np.array([-0.0] * 3 + [-1.0] + [-0.0] * 8, np.float32)),
                                    ("won counts against", np.array([0.0, -1.0] + [0.0] * 10, np.float32))])
@pytest.mark.parametrize("width", [1, 3, 40])
def test_whole_plies_that_tie_fall_by_candidate_index(oracle, name, w, width):
    m = _m()
    L, M, n = 2, 5, 6
    rows, pieces = T.generate_configs(L, M, n, seed=99)
    solved, length, actions, best = m.placement_solve(rows, pieces, L, M, w, width)
    for i in range(n):
        s, ln, path, values = _plain_solve(oracle, L, M, rows[i], pieces[i], w, width)
        assert (solved[i], length[i]) == (s, ln), (name, width, i)
        assert actions[i, :ln].tolist() == path and (actions[i, ln:] == 255).all(), (name, width, i)
        got = best[i].view(np.uint32)
        assert got[:len(values)].tolist() == [int(np.float32(v).view(np.uint32)) for v in values], (name, width, i)
        assert (got[len(values):] == 0).all()                  # +0 beyond the plies run
    if name == "all -0":
        plies = np.where(solved > 0, length, 0)
        assert all((best[i, :plies[i]].view(np.uint32) == 0x80000000).all() for i in range(n))      # a -0 keeps its bits
    if name == "all +0" and width == 1:
        # every value ties, so the beam is the lexicographically first path: placement 0 until a ply has a won candidate
        assert all((actions[i, :max(length[i] - 1, 0)] == 0).all() for i in range(n))


# ------------------------------------------------------------------------------------------------ 5. the recorded outputs
GOLDEN_CASES = ((1, 1), (2, 6), (3, 13), (5, 20))
GOLDEN_WIDTHS = (1, 3, 16, 64)


def test_the_recorded_mirror_outputs_are_the_mirrors(oracle):
    """tests/golden/solve_mirror.npz (make_golden_solve.py) against the mirror as it stands, on a slice of every case -- the mirror
    treats every configuration on its own -- and its inputs against the host generators."""
    m = _m()
    g = load_golden("solve_mirror.npz")
    for L, M in GOLDEN_CASES:
        rows, pieces = g[f"L{L}_M{M}_rows"], g[f"L{L}_M{M}_pieces"]
        assert rows.shape == (128, 20) and pieces.shape == (128, M + 1)
        c_rows, c_pieces = T.generate_configs(L, M, 64, seed=7)
        assert np.array_equal(rows[:64], c_rows) and np.array_equal(pieces[:64], c_pieces)
        assert np.array_equal(rows[64:], oracle.synth_boards(7, 0, 64, L)) and np.array_equal(pieces[64:], oracle.synth_pieces(7, 0, 64, M))
        for W in GOLDEN_WIDTHS:
            pick = np.array([0, 63, 64, 127] if W == 64 else [0, 1, 31, 63, 64, 65, 100, 127])
            got = m.placement_solve(rows[pick], pieces[pick], L, M, T.CLASSICAL_WEIGHTS, W)
            for name, x in zip(("solved", "solution_len", "actions", "best_value"), got):
                want = g[f"L{L}_M{M}_W{W}_{name}"][pick]
                assert x.dtype == want.dtype and np.array_equal(x.view(np.uint32) if name == "best_value" else x,
                                                                want.view(np.uint32) if name == "best_value" else want), (L, M, W, name)
    # what the recorded cases cover: both verdicts, and solutions of every length up to beyond a window
    assert any(not g[f"L{L}_M{M}_W{W}_solved"].all() for L, M in GOLDEN_CASES for W in GOLDEN_WIDTHS)
    assert g["L5_M20_W1_solution_len"].max() > 12
    assert g["long_L105_solved"].all() and g["long_L105_solution_len"].min() >= 240 and g["long_pieces"].shape == (4, 255)
    for i in range(4):                                         # the long solutions win on the oracle
        assert _replay(oracle, 105, 254, g["long_rows"][i], g["long_pieces"][i], g["long_L105_actions"][i],
                       int(g["long_L105_solution_len"][i])) == (1, int(g["long_L105_solution_len"][i]))
    assert not g["long_L112_solved"].any() and (g["long_L112_actions"] == 255).all()


# ------------------------------------------------------------------------------------------------ 6. arithmetic and arguments
def test_tighten_pool_keeps_the_solved_within_the_budget_and_cuts_the_piece_lists():
    import torch
    gen = np.random.default_rng(3)
    n, M = 50, 12
    rows = gen.integers(0, 1 << 10, (n, 20)).astype(np.uint16)
    pieces = gen.integers(0, 7, (n, M + 1)).astype(np.uint8)
    solved = gen.random(n) < 0.7
    length = np.where(solved, gen.integers(1, M + 1, n), 0).astype(np.int32)
    for M_new in (1, 5, 12):
        keep = solved & (length <= M_new)
        if not keep.any():
            continue
        r, p = T.tighten_pool(rows, pieces, solved, length, M_new)
        assert np.array_equal(r, rows[keep]) and np.array_equal(p, pieces[keep][:, :M_new + 1]) and p.flags.c_contiguous
        rt, pt = T.tighten_pool(torch.from_numpy(rows.view(np.int16)), torch.from_numpy(pieces), torch.from_numpy(solved),
                                torch.from_numpy(length), M_new)
        assert np.array_equal(rt.numpy().view(np.uint16), r) and np.array_equal(pt.numpy(), p) and pt.is_contiguous()
    # an unsolved entry has length 0, which is within every budget: `solved` decides
    r, _ = T.tighten_pool(rows, pieces, np.zeros(n, bool) | (np.arange(n) == 4), np.zeros(n, np.int32), 3)
    assert r.shape[0] == 1 and np.array_equal(r[0], rows[4])
    for bad in (0, 13, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="M_new"):
            T.tighten_pool(rows, pieces, solved, length, bad)
    with pytest.raises(ValueError, match="nothing is left"):
        T.tighten_pool(rows, pieces, np.zeros(n, bool), length, 5)
    with pytest.raises(ValueError, match="nothing is left"):
        T.tighten_pool(rows, pieces, np.ones(n, bool), np.full(n, 9, np.int32), 8)
    with pytest.raises(ValueError, match="solved and solution_len"):
        T.tighten_pool(rows, pieces, solved[:-1], length, 5)


def test_python_refusals_of_solve_configs_need_no_gpu():
    rows, pieces = np.zeros((4, 20), np.uint16), np.zeros((4, 7), np.uint8)
    ok = dict(rows=rows, pieces=pieces, L=2, M=6)
    for L in (0, 251, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="L must"):
            T.solve_configs(**dict(ok, L=L))
    for M in (0, 255, -1, 6.0, True):
        with pytest.raises(ValueError, match="M must"):
            T.solve_configs(**dict(ok, M=M))
    for width in (0, 65, -1, 1.5, 8.0, True, "8", None):
        with pytest.raises(ValueError, match="width"):
            T.solve_configs(**ok, width=width)
    for weights in (np.zeros(11), np.zeros((2, 12)), "classical", [None] * 12):
        with pytest.raises(ValueError, match="weights"):
            T.solve_configs(**ok, weights=weights)
    with pytest.raises(ValueError, match="finite"):
        T.solve_configs(**ok, weights=np.full(12, np.nan))
    for r, p in ((np.zeros((4, 19), np.uint16), pieces), (rows, np.zeros((4, 5), np.uint8)), (rows, np.zeros((4, 8), np.uint8)),
                 (rows, np.zeros((3, 7), np.uint8)), (np.zeros((4, 20, 9), bool), pieces), (rows, np.zeros(7, np.uint8))):
        with pytest.raises(ValueError, match="rows must be"):
            T.solve_configs(r, p, 2, 6)
    with pytest.raises(ValueError, match="at least one"):
        T.solve_configs(np.zeros((0, 20), np.uint16), np.zeros((0, 7), np.uint8), 2, 6)
    m = _m()
    for bad in (dict(L=0), dict(M=255), dict(width=0), dict(width=True)):
        with pytest.raises(ValueError):
            m.placement_solve(**{**dict(rows=rows, pieces=pieces, L=2, M=6, weights=CW, width=4), **bad})
    with pytest.raises(ValueError, match="pieces"):
        m.placement_solve(rows, pieces[:, :6], 2, 6, CW, 4)
    assert T.solve.solve_configs is T.solve_configs and T.solve.tighten_pool is T.tighten_pool


def test_forward_games_refuses_an_unknown_solver_before_it_touches_the_environment():
    assert T.ForwardGames.SOLVERS == ("reference", "beam")
    for bad in ("dfs", "Beam", "", None, 1):
        with pytest.raises(ValueError, match="solver"):
            T.ForwardGames(None, range(4), solver=bad)
    import inspect
    for cls in (T.ForwardGames, T.PoolRefresher):
        p = inspect.signature(cls.__init__).parameters
        assert (p["solver"].default, p["weights"].default, p["width"].default) == ("reference", None, 16), cls


def test_every_refusal_of_the_solve_entry_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    name = b"tpl_placement_solve"

    def solve(rows=fake, pieces=fake, n=4, L=2, M=6, weights=fake, width=4, solved=fake, length=fake, actions=fake, best=fake):
        return lib.tpl_placement_solve(rows, pieces, n, L, M, weights, width, solved, length, actions, best, None)

    for n in (0, -1, -(1 << 40)):
        assert solve(n=n) < 0 and b"positive" in err() and name in err(), n
    for n in (1 << 31, 1 << 40):
        assert solve(n=n) < 0 and b"2^31" in err() and name in err(), n
    for arg in ("rows", "pieces", "weights", "solved", "length", "actions"):
        assert solve(**{arg: None}) < 0 and b"null" in err() and name in err(), arg
    assert solve(weights=fake + 4) < 0 and b"weights must be 16-byte aligned" in err() and name in err()
    assert solve(length=fake + 2) < 0 and b"solution_len must be 4-byte aligned" in err() and name in err()
    assert solve(best=fake + 2) < 0 and b"best_value must be 4-byte aligned" in err() and name in err()
    assert solve(rows=fake + 1) < 0 and b"rows must be 2-byte aligned" in err() and name in err()
    for L, M in ((0, 6), (251, 6), (2, 0), (2, 255), (-1, 6), (2, 1 << 30)):
        assert solve(L=L, M=M) < 0 and b"L and M" in err() and name in err(), (L, M)
    for width in (0, 65, -1, 1 << 30, -(1 << 31)):
        assert solve(width=width) < 0 and b"width must be in [1, 64]" in err() and name in err(), width
    # the largest game is not refused for its size: a check that comes after L, M and the width speaks
    assert solve(L=250, M=254, width=64, rows=fake + 1) < 0 and b"aligned" in err() and b"L and M" not in err()
    # a bad width is refused with the optional output left out as well
    assert solve(width=0, best=None) < 0 and b"width" in err()


def test_the_header_declares_the_solve_entry_and_the_library_exports_it():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and "tpl_placement_solve" in declared
    proto = re.search(r"int tpl_placement_solve\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["rows", "pieces", "n", "L", "M", "weights", "width", "solved",
                                                                     "solution_len", "actions", "best_value", "stream"]
    assert "FOUND NO WIN" in raw and "DOES NOT MEAN" in raw    # what solved = 0 does and does not say
    assert "found no win" in T.solve_configs.__doc__ and "not that there is none" in T.solve_configs.__doc__
    assert hasattr(ctypes.CDLL(_m().build_library()), "tpl_placement_solve")
    units = [os.path.basename(p) for p in _m()._UNITS]
    assert "solve.hip" in units and any(p.endswith(os.path.join("learn", "solve.hip")) for p in _m()._sources())
    assert _m().SOLVE_MAX_MOVES == 254


def test_the_solve_kernel_uses_no_scratch_and_leaves_two_groups_a_cu_at_the_limits():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    mine = [r for r in rows if "placement_solve_kernel" in r[-1]]
    assert len(mine) == 1, [r[-1] for r in rows]
    assert mine[0][mine[0].index("scratch") - 1] == "0", mine
    assert int(mine[0][mine[0].index("vgpr") - 1]) <= 96, mine                   # five waves per SIMD, as the placement beam
    static = int(mine[0][mine[0].index("lds") - 1])
    tape = 2 * 64 * 254                                                          # the dynamic part at W = 64, M = 254
    assert static + tape <= 64 * 1024, mine                                      # launchable without an attribute
    assert 2 * (static + tape) <= 160 * 1024, mine                               # two groups to a CU's 160 KB
    assert 5 * (static + 2 * 64 * 40) <= 160 * 1024, mine                        # five at M = 40, whatever the width
    assert len([r for r in rows if "placement_beam_kernel" in r[-1]]) == 1
