"""CPU-side checks of the move bound and the bounded solver (include/tpl_learn.h's rule; _learn_lib.move_bound_cells, move_bound and
placement_solve(bound=True); solve.py's config_bound, solve_configs(bound=...), tighten_pool(bound=, slack=); BeamPolicy(bound=...)):

  1. the mirror of the bound is the definition, restated by brute force: random boards, boards with full rows, 1 .. 250 lines owed;
  2. on both carved fixtures the bound at the root EQUALS carving's sol_len, and no state of a recorded solution is dead even under
     a budget of sol_len moves;
  3. an exhaustive search on the C oracle never wins from a dead state and never before `bound`; the bounded mirror, wide enough to
     keep everything, reports the exhaustive search's first winning ply with complete = 1, and solved = 0 with complete = 1 where
     there is no win;
  4. the effect: 48 carved configurations at a budget of 14 moves, width 4: the bounded mirror solves strictly more than the plain one;
  5. the recorded outputs that the GPU tests compare the kernels with are the mirror's as it stands (a slice of every case);
  6. the Python refusals, every refusal of the six new entries, the header, the exports and the kernels' resources.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_solve_cpu import CW, Node, _first_winning_ply, _placements, _replay

import tetris_piclim as T

sys.path.insert(0, GOLDEN)
import make_golden_bound as G  # noqa: E402  -- the cases, the grouping by budget and the gathering of a case's outputs


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ 1. mirror against definition
def _cells_by_definition(rows, lines_left):
    """The rule as the header words it, one board: the costs of the twenty rows, as many 10s as asked for, the smallest summed."""
    cost = []
    for r in range(20):
        fill = bin(int(rows[r]) & 0x3FF).count("1")
        cost.append(10 - fill if fill < 10 else 10)
    cost = sorted(cost + [10] * lines_left)
    return sum(cost[:lines_left])


def test_the_mirror_of_the_bound_is_the_definition():
    m = _m()
    gen = np.random.default_rng(2)
    n = 600
    rows = np.zeros((n, 20), np.uint16)
    for i in range(n):
        height = int(gen.integers(0, 21))
        density = gen.random()
        cells = gen.random((height, 10)) < density
        rows[i, 20 - height:] = (cells.astype(np.uint16) << np.arange(10, dtype=np.uint16)).sum(axis=1)
    rows[::5, 19] = 0x3FF                                      # boards with full rows: they cost what a fresh row costs
    rows[::7, 10:15] = 0x3FF
    rows[3] = 0x3FF                                            # every row full
    rows[4] = 0
    left = gen.integers(1, 251, n)
    left[:250] = np.arange(1, 251)                             # every number of lines owed, past the twenty rows of a board
    got = m.move_bound_cells(rows, left)
    want = np.array([_cells_by_definition(rows[i], int(left[i])) for i in range(n)])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert got[3] == 10 * left[3] and got[4] == 10 * left[4] and (left > 20).sum() >= 200
    assert np.array_equal(m.move_bound_cells(rows, 0), np.zeros(n, np.int64))
    assert m.move_bound_cells(rows[0], 3) == _cells_by_definition(rows[0], 3)          # one board, one number
    # move_bound: a finished board owes and has nothing, a running board whose lines have reached L owes nothing
    state = gen.integers(0, 4, n)
    lines, moves = gen.integers(0, 12, n), gen.integers(0, 40, n)
    b = m.move_bound(rows, 10, 40, lines, moves, state)
    run = state == 0
    assert (b["cells"][~run] == 0).all() and (b["spare"][~run] == 0).all() and not b["dead"][~run].any()
    want = np.array([_cells_by_definition(rows[i], max(10 - int(lines[i]), 0)) for i in range(n)])
    assert np.array_equal(b["cells"][run], want[run]) and np.array_equal(b["spare"][run], (4 * (40 - moves) - want)[run])
    assert np.array_equal(b["need"], -(-b["cells"] // 4)) and np.array_equal(b["dead"], b["need"] > np.where(run, 40 - moves, 0))
    assert b["dead"].any() and (run & ~b["dead"]).any()
    with pytest.raises(ValueError, match="negative"):
        m.move_bound_cells(rows, -1)
    with pytest.raises(ValueError, match="rows must be"):
        m.move_bound_cells(rows[:, :19], 1)


# ------------------------------------------------------------------------------------------------ 2. the carved fixtures
@pytest.mark.parametrize("name", ["carved_L10_M40.npz", "carved_L5_M20.npz"])
def test_the_bound_at_the_root_is_carvings_solution_length_and_no_recorded_state_is_dead(name):
    m = _m()
    f = load_golden(name)
    L, M = int(f["L"]), int(f["M"])
    rows, sol_len = f["rows"], f["sol_len"].astype(np.int64)
    assert rows.shape == (256, 20)
    need = (m.move_bound_cells(rows, L) + 3) // 4
    assert np.array_equal(need, sol_len)                       # carving's solutions waste no cell: the bound proves them shortest
    assert (m.move_bound_cells(rows, L) <= 4 * sol_len).all()
    # every state of every recorded solution, under a budget of its own sol_len moves: cells <= 4 x (moves left)
    states = 0
    for t in range(M):
        at = np.flatnonzero(t < sol_len)                       # r_*[:, t] is the state after move t + 1 of the solution
        if at.size == 0:
            break
        moves = f["r_moves"][at, t].astype(np.int64)
        assert (moves == t + 1).all()
        cells = m.move_bound_cells(f["r_rows"][at, t], np.maximum(L - f["r_lines"][at, t].astype(np.int64), 0))
        won = f["r_state"][at, t] == 1
        assert (cells[~won] <= 4 * (sol_len[at] - moves)[~won]).all(), t
        assert np.array_equal(won, moves == sol_len[at])
        b = m.move_bound(f["r_rows"][at, t], L, M, f["r_lines"][at, t], moves, f["r_state"][at, t])
        assert not b["dead"].any()
        states += at.size
    assert states == sol_len.sum()


# ------------------------------------------------------------------------------------------------ 3. exhaustive search
def _exhaustive(O, L, M, rows, pieces):
    """Breadth first over ALL placements, dead states expanded too: (the first ply at which any sequence wins, 0 if none; whether a
    win was ever reached through a dead state)."""
    m = _m()
    level, first, through_dead = [(Node(O, L, M, rows, pieces), False)], 0, False
    for ply in range(1, M + 1):
        nxt, was = [], []
        for node, dead in level:
            for b in _placements(pieces[ply - 1]):
                c = node.child(b)
                if c.won:
                    first = first or ply
                    through_dead |= dead
                if c.running:
                    nxt.append(c)
                    was.append(dead)
        if not nxt:
            break
        now = m.move_bound(np.array([c.g.rows for c in nxt], np.uint16), L, M, [c.g.lines_cleared for c in nxt],
                           [c.g.moves_used for c in nxt], 0)["dead"]
        level = [(c, bool(a or d)) for c, a, d in zip(nxt, was, now)]
    return first, through_dead


@pytest.mark.parametrize("L,M,game_L,count", [(1, 1, 1, 24), (1, 2, 1, 24), (2, 2, 1, 24), (2, 2, 2, 24), (2, 3, 2, 6), (2, 3, 1, 6)])
def test_no_win_comes_from_a_dead_state_and_a_complete_bounded_search_is_the_exhaustive_one(oracle, L, M, game_L, count):
    """test_solve_cpu's boards: carved for `game_L` lines, searched for L; with L > game_L many have no win within M moves."""
    m = _m()
    rows, pieces = T.generate_configs(game_L, M, count, seed=31 + M)
    found = [_exhaustive(oracle, L, M, rows[i], pieces[i]) for i in range(count)]
    first = np.array([f[0] for f in found])
    assert not any(f[1] for f in found)                        # a dead state has no winning continuation
    assert np.array_equal(first, [_first_winning_ply(oracle, L, M, rows[i], pieces[i]) for i in range(count)])
    root_dead = m.move_bound(rows, L, M, 0, 0, 0)["dead"]
    assert (first[root_dead] == 0).all()
    width = 34 ** (M - 1)
    solved, length, actions, _, bound, complete = m.placement_solve(rows, pieces, L, M, CW, width, max_width=width, bound=True)
    assert bound.dtype == np.int32 and complete.dtype == np.uint8
    assert np.array_equal(bound, (m.move_bound_cells(rows, L) + 3) // 4)
    assert (first[first > 0] >= bound[first > 0]).all()        # the first winning ply is never below the bound
    assert complete.all()
    assert np.array_equal(length, first) and np.array_equal(solved, (first > 0).astype(np.uint8))
    for i in np.flatnonzero(solved):
        assert _replay(oracle, L, M, rows[i], pieces[i], actions[i], length[i]) == (1, length[i])
    if (L, M, game_L) in ((2, 2, 1), (2, 3, 1)):
        assert (solved == 0).any()                             # proved: no sequence of placements wins


# ------------------------------------------------------------------------------------------------ 4. the effect
def test_the_bounded_mirror_solves_strictly_more_of_a_tight_set_at_width_four(oracle):
    m = _m()
    f = load_golden("carved_L10_M40.npz")
    L, M, W = 10, 14, 4
    pick = np.flatnonzero((f["sol_len"] >= 12) & (f["sol_len"] <= 14))[:48]
    assert pick.size == 48
    rows, pieces = f["rows"][pick], f["pieces"][pick][:, :M + 1]
    plain = m.placement_solve(rows, pieces, L, M, T.CLASSICAL_WEIGHTS, W)
    pruned = m.placement_solve(rows, pieces, L, M, T.CLASSICAL_WEIGHTS, W, bound=True)
    scored = m.placement_solve(rows, pieces, L, M, T.CLASSICAL_WEIGHTS, W, bound=True, spare_weight=1.0)
    counts = [int(x[0].sum()) for x in (plain, pruned, scored)]
    print("solved of 48 at M = 14, width 4: plain, with the prune, with the prune and spare_weight = 1:", counts)
    assert counts[1] > counts[0] and counts[2] > counts[0]
    for solved, length, actions, _, bound, complete in (pruned, scored):
        assert np.array_equal(bound, f["sol_len"][pick])       # the bound is carving's own length here
        for i in np.flatnonzero(solved):
            assert _replay(oracle, L, M, rows[i], pieces[i], actions[i], length[i]) == (1, length[i])
            assert f["sol_len"][pick[i]] <= length[i] <= M     # no solution is shorter than carving's, which the bound proves shortest
        assert (length[solved == 0] == 0).all() and (actions[solved == 0] == 255).all()
        assert not complete.any() or (length[(solved == 1) & (complete == 1)] == bound[(solved == 1) & (complete == 1)]).all()
        print("of them as short as carving's, so provably shortest:", int(((solved == 1) & (length == bound)).sum()))


def test_the_defaults_of_the_mirror_are_the_unbounded_rule_and_spare_weight_needs_the_bound():
    m = _m()
    rows, pieces = T.generate_configs(2, 6, 12, seed=5)
    plain = m.placement_solve(rows, pieces, 2, 6, CW, 3)
    assert len(plain) == 4
    loose = m.placement_solve(rows, pieces, 2, 6, CW, 3, bound=False, spare_weight=0.0)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(plain, loose))
    with pytest.raises(ValueError, match="bound=True"):
        m.placement_solve(rows, pieces, 2, 6, CW, 3, spare_weight=0.5)
    for bad in (np.inf, np.nan, 1e39):
        with pytest.raises(ValueError, match="finite"):
            m.placement_solve(rows, pieces, 2, 6, CW, 3, bound=True, spare_weight=bad)
    with pytest.raises(ValueError, match="bound must"):
        m.placement_solve(rows, pieces, 2, 6, CW, 3, bound=1)


# ------------------------------------------------------------------------------------------------ 5. the recorded outputs
def _pinned(g, key, got):
    for name in G.NAMES:
        assert got[name].dtype == g[key + name].dtype, (key, name)
        assert np.array_equal(got[name].view(np.uint8), g[key + name].view(np.uint8)), (key, name)


def test_the_recorded_bounded_outputs_are_the_mirrors():
    """tests/golden/bound_mirror.npz (make_golden_bound.py) against the mirror as it stands, every configuration of what is recomputed:
    at widths 1, 3 and 16 one (slack, spare_weight) of every case and feature form in turn; at width 64, where a case takes the mirror
    up to half a minute, every combination at (2, 6) and one per feature form at (3, 13); and the inputs against the host generator.
    make_golden_bound.py says what is therefore trusted as recorded."""
    m = _m()
    g = load_golden("bound_mirror.npz")
    turn = 0
    for L, M in G.CASES:
        rows, pieces, sol_len = G.inputs(L, M)
        for name, x in (("rows", rows), ("pieces", pieces), ("sol_len", sol_len)):
            assert np.array_equal(g[f"L{L}_M{M}_{name}"], x), (L, M, name)
        assert np.array_equal(sol_len, (m.move_bound_cells(rows, L) + 3) // 4)     # the budgets are the bound and the bound + 1
        for F, w in G.weights().items():
            for W in (1, 3, 16):                               # width 64 takes the mirror half a minute a case
                slack, spare = G.SLACKS[turn % 2], G.SPARES[(turn // 2) % 2]
                turn += 1
                got = G.solve_case(m, rows, pieces, sol_len, L, M, slack, w, W, spare)
                key = f"L{L}_M{M}_F{F}_W{W}_s{slack}_p{int(spare * 100)}_"
                _pinned(g, key, got)
    for F, w in G.weights().items():                           # width 64
        for slack in G.SLACKS:
            for spare in G.SPARES:
                rows, pieces, sol_len = G.inputs(2, 6)
                _pinned(g, f"L2_M6_F{F}_W64_s{slack}_p{int(spare * 100)}_", G.solve_case(m, rows, pieces, sol_len, 2, 6, slack, w, 64, spare))
        rows, pieces, sol_len = G.inputs(3, 13)
        slack, spare = (0, 0.25) if F == 12 else (1, 0.0)
        _pinned(g, f"L3_M13_F{F}_W64_s{slack}_p{int(spare * 100)}_", G.solve_case(m, rows, pieces, sol_len, 3, 13, slack, w, 64, spare))
    # what the recorded cases cover: both verdicts, complete searches and cut ones, proofs of both kinds
    solved = np.concatenate([g[k] for k in g.files if k.endswith("_solved") and not k.startswith("long")])
    complete = np.concatenate([g[k] for k in g.files if k.endswith("_complete") and not k.startswith("long")])
    assert (solved == 0).sum() >= 50 and (solved == 1).sum() >= 1000 and (complete == 0).sum() >= 500 and (complete == 1).sum() >= 500
    assert ((solved == 0) & (complete == 1)).sum() == 0        # every configuration is winnable at its budget: no false proof
    assert g["long_L105_solved"].all() and g["long_L105_actions"].shape == (4, 254)


# ------------------------------------------------------------------------------------------------ 6. arithmetic and arguments
def test_tighten_pool_with_a_bound_keeps_what_is_provably_within_slack_of_the_least_budget():
    import torch
    gen = np.random.default_rng(8)
    n, M = 60, 12
    rows = gen.integers(0, 1 << 10, (n, 20)).astype(np.uint16)
    pieces = gen.integers(0, 7, (n, M + 1)).astype(np.uint8)
    solved = gen.random(n) < 0.8
    length = np.where(solved, gen.integers(4, M + 1, n), 0).astype(np.int32)
    bound = np.maximum(length - gen.integers(0, 4, n), 1).astype(np.int32)
    for M_new, slack in ((8, 0), (8, 1), (10, 2), (12, 0)):
        keep = solved & (length <= M_new) & (bound >= M_new - slack)
        if not keep.any():
            continue
        r, p = T.tighten_pool(rows, pieces, solved, length, M_new, bound=bound, slack=slack)
        assert np.array_equal(r, rows[keep]) and np.array_equal(p, pieces[keep][:, :M_new + 1])
        rt, pt = T.tighten_pool(torch.from_numpy(rows.view(np.int16)), torch.from_numpy(pieces), torch.from_numpy(solved),
                                torch.from_numpy(length), M_new, bound=torch.from_numpy(bound), slack=slack)
        assert np.array_equal(rt.numpy().view(np.uint16), r) and np.array_equal(pt.numpy(), p)
    plain = T.tighten_pool(rows, pieces, solved, length, 8)
    assert plain[0].shape[0] > T.tighten_pool(rows, pieces, solved, length, 8, bound=bound, slack=0)[0].shape[0]
    for kw in (dict(bound=bound), dict(slack=1)):
        with pytest.raises(ValueError, match="go together"):
            T.tighten_pool(rows, pieces, solved, length, 8, **kw)
    for bad in (-1, 1.0, True, "1"):
        with pytest.raises(ValueError, match="slack"):
            T.tighten_pool(rows, pieces, solved, length, 8, bound=bound, slack=bad)
    with pytest.raises(ValueError, match="bound must be"):
        T.tighten_pool(rows, pieces, solved, length, 8, bound=bound[:-1], slack=1)
    with pytest.raises(ValueError, match="nothing is left"):
        T.tighten_pool(rows, pieces, solved, length, 8, bound=np.zeros(n, np.int32), slack=0)


def test_python_refusals_of_the_bounded_interfaces_need_no_gpu():
    import inspect
    rows, pieces = np.zeros((4, 20), np.uint16), np.zeros((4, 7), np.uint8)
    ok = dict(rows=rows, pieces=pieces, L=2, M=6)
    with pytest.raises(ValueError, match="bound=True"):
        T.solve_configs(**ok, spare_weight=0.5)
    for bad in (np.inf, np.nan, 1e39, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            T.solve_configs(**ok, bound=True, spare_weight=bad)
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(ValueError, match="spare_weight must be a number"):
            T.solve_configs(**ok, bound=True, spare_weight=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="bound must be"):
            T.solve_configs(**ok, bound=bad)
    for L in (0, 251, 2.0, True):
        with pytest.raises(ValueError, match="L must"):
            T.config_bound(rows, L)
    for r in (np.zeros((4, 19), np.uint16), np.zeros((4, 20, 9), bool), np.zeros(20, np.uint16)):
        with pytest.raises(ValueError, match="rows must be"):
            T.config_bound(r, 2)
    with pytest.raises(ValueError, match="at least one"):
        T.config_bound(np.zeros((0, 20), np.uint16), 2)
    p = inspect.signature(T.solve_configs).parameters
    assert (p["bound"].default, p["spare_weight"].default) == (False, 0.0)
    p = inspect.signature(T.tighten_pool).parameters
    assert (p["bound"].default, p["slack"].default) == (None, None)
    for fn in (T.BeamPolicy.__init__, T.evaluate_heuristic, T.tune_heuristic):
        p = inspect.signature(fn).parameters
        assert (p["bound"].default, p["spare_weight"].default) == (False, 0.0), fn
    # the players: the bounded form is the beam's, so evaluate and tune refuse it without a width, before anything is built
    for fn, args in ((T.evaluate_heuristic, (None, CW, None, 4)), (T.tune_heuristic, (2, 6, None))):
        with pytest.raises(ValueError, match="give a width"):
            fn(*args, bound=True)
        with pytest.raises(ValueError, match="bound=True"):
            fn(*args, width=4, spare_weight=1.0)
        with pytest.raises(ValueError, match="finite"):
            fn(*args, width=4, bound=True, spare_weight=np.inf)
    with pytest.raises(ValueError, match="bound=True"):
        T.BeamPolicy(None, CW, 3, 4, spare_weight=0.25)
    with pytest.raises(ValueError, match="bound must be"):
        T.BeamPolicy(None, CW, 3, 4, bound="on")
    assert "IS a proof" in T.solve.__doc__ and "complete[i] set, solved[i] = False is a" in T.solve_configs.__doc__
    assert T.move_bound is T.heuristic.move_bound and T.config_bound is T.solve.config_bound
    assert {"move_bound", "config_bound"} <= set(T.__all__)


ENTRIES = ("tpl_move_bound", "tpl_move_bound_rows", "tpl_placement_solve_bound", "tpl_placement_solve_move_bound",
           "tpl_placement_beam_bound", "tpl_placement_beam_move_bound")
KERNELS = ("move_bound_kernel", "move_bound_rows_kernel", "placement_solve_bound_kernel", "placement_solve_move_bound_kernel",
           "placement_beam_bound_kernel", "placement_beam_move_bound_kernel")


def test_every_refusal_of_the_six_entries_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    # tpl_move_bound
    ok = [fake, fake, 8, 5, 20, fake, fake, None]
    for at, value, what in ((0, None, "null"), (1, None, "null"), (1, fake + 8, "16-byte"), (2, 0, "positive"), (2, -3, "positive"),
                            (2, (1 << 31) // 40 + 1, "too large"), (3, 0, "L and M"), (3, 251, "L and M"), (4, 0, "L and M"),
                            (4, 255, "L and M"), (5, None, "cells_out and spare_out"), (6, None, "cells_out and spare_out"),
                            (5, fake + 2, "4-byte"), (6, fake + 1, "4-byte")):
        args = list(ok)
        args[at] = value
        assert lib.tpl_move_bound(*args) < 0 and "tpl_move_bound:" in err() and what in err(), (at, value, err())
    # tpl_move_bound_rows
    ok = [fake, 8, 5, fake, None]
    for at, value, what in ((0, None, "null"), (3, None, "null"), (1, 0, "positive"), (1, -1, "positive"), (1, 1 << 31, "2^31"),
                            (2, 0, "L must"), (2, 251, "L must"), (0, fake + 1, "rows must be 2-byte"), (3, fake + 2, "cells_out must be 4-byte")):
        args = list(ok)
        args[at] = value
        assert lib.tpl_move_bound_rows(*args) < 0 and "tpl_move_bound_rows:" in err() and what in err(), (at, value, err())
    # the bounded solver: its twin's refusals and its own
    for name in ENTRIES[2:4]:
        fn = getattr(lib, name)
        ok = [fake, fake, 4, 2, 6, fake, 4, 0.25, fake, fake, fake, fake, fake, fake, None]
        for at, value, what in ((0, None, "null"), (1, None, "null"), (5, None, "null"), (8, None, "null"), (9, None, "null"),
                                (10, None, "null"), (12, None, "bound and complete"), (13, None, "bound and complete"),
                                (2, 0, "positive"), (2, 1 << 31, "2^31"), (3, 0, "L and M"), (3, 251, "L and M"), (4, 0, "L and M"),
                                (4, 255, "L and M"), (6, 0, "width must be in [1, 64]"), (6, 65, "width must be in [1, 64]"),
                                (0, fake + 1, "rows must be 2-byte"), (5, fake + 4, "weights must be 16-byte"),
                                (9, fake + 2, "solution_len must be 4-byte"), (11, fake + 2, "best_value must be 4-byte"),
                                (12, fake + 2, "bound must be 4-byte"), (7, float("inf"), "spare_weight must be finite"),
                                (7, float("nan"), "spare_weight must be finite")):
            args = list(ok)
            args[at] = value
            assert fn(*args) < 0 and name + ":" in err() and what in err(), (name, at, value, err())
        args = list(ok)
        args[11], args[6] = None, 0                            # a bad width is refused with the optional output left out as well
        assert fn(*args) < 0 and "width" in err()
    # the bounded beam
    for name in ENTRIES[4:]:
        fn = getattr(lib, name)
        ok = [fake, fake, 8, 5, 20, fake, 8, 2, 4, 0.0, fake, None, None, None]
        for at, value, what in ((0, None, "null"), (1, fake + 8, "16-byte"), (2, 0, "positive"), (2, (1 << 31) // 40 + 1, "too large"),
                                (3, 251, "L and M"), (4, 255, "L and M"), (5, None, "weights and action"), (10, None, "weights and action"),
                                (6, 0, "boards_per_member"), (5, fake + 8, "weights must be 16-byte"), (13, None, None),
                                (12, fake + 2, "score must be 4-byte"), (7, 0, "depth"), (7, 13, "depth"), (8, 0, "width"), (8, 65, "width"),
                                (9, float("inf"), "spare_weight must be finite"), (9, float("nan"), "spare_weight must be finite")):
            if what is None:
                continue
            args = list(ok)
            args[at] = value
            assert fn(*args) < 0 and name + ":" in err() and what in err(), (name, at, value, err())


def test_the_header_states_the_rule_and_the_library_exports_the_six_entries():
    m = _m()
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_\w+)\s*\(", text))
    assert declared == set(m.LEARN_SYMBOLS) and set(ENTRIES) <= declared
    lib = ctypes.CDLL(m.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    proto = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % n, text, flags=re.S).group(1).split(",")]
    for form in ("", "_move"):                                 # the twin's arguments, spare_weight behind the width, two outputs more
        twin = proto(f"tpl_placement_solve{form}")
        assert proto(f"tpl_placement_solve{form}_bound") == twin[:7] + ["spare_weight"] + twin[7:-1] + ["bound", "complete", "stream"]
        twin = proto(f"tpl_placement_beam{form}")
        assert proto(f"tpl_placement_beam{form}_bound") == twin[:9] + ["spare_weight"] + twin[9:]
    assert proto("tpl_move_bound") == ["plane_a", "plane_b", "n", "L", "M", "cells_out", "spare_out", "stream"]
    assert proto("tpl_move_bound_rows") == ["rows", "n", "L", "cells_out", "stream"]
    # the rule, its proof and what complete proves
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("a row is cleared only when all ten of its cells are filled", "Compaction keeps every surviving row's contents",
                  "Every move adds exactly four cells or tops out", "A DEAD BOARD HAS NO WINNING CONTINUATION", "THE BOUNDED FORM",
                  "one rounded multiply and one rounded add, made last", "UNDER complete = 1, solved = 0 PROVES"):
        assert words in flat, words
    # the body is shared, not copied: a bounded unit is its twin with the switch defined
    here = os.path.dirname(m._UNITS[-1])
    units = [os.path.basename(p) for p in m._UNITS]
    for unit, move in (("solve_bound", False), ("beam_bound", False), ("solve_move_bound", True), ("beam_move_bound", True)):
        code = [l for l in open(os.path.join(here, unit + ".hip")).read().splitlines() if l.strip() and not l.startswith("//")]
        want = (["#define TPL_PLACEMENT_MOVE_UNIT"] if move else []) + ["#define TPL_PLACEMENT_BOUND_UNIT",
                                                                          f'#include "{unit.split("_")[0]}.hip"']
        assert code == want and unit + ".hip" in units, unit
    assert "bound.hip" in units and units[-1] == "heuristic.hip"
    placement = open(os.path.join(here, "tpl_placement.h")).read()
    assert placement.count("move_bound_cells(") == 2            # defined, and used in the one place: move_bound
    assert placement.count("bounded_move(") == 1 and "kUnitBound" in placement


def test_the_six_kernels_use_no_scratch_and_the_bounded_twins_keep_four_groups_a_cu():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    num = lambda r, what: int(r[r.index(what) - 1])
    named = lambda kernel: [r for r in rows if f"{len(kernel)}{kernel}E" in r[-1]]      # the whole mangled name: no name within another
    for kernel in KERNELS:
        mine = named(kernel)
        assert len(mine) == 1, (kernel, [r[-1] for r in rows])
        assert num(mine[0], "scratch") == 0, mine
        if "placement" not in kernel:
            assert num(mine[0], "lds") == 0 and num(mine[0], "vgpr") <= 64, mine
            continue
        twin = named(kernel.replace("_bound", ""))
        assert len(twin) == 1, (kernel, [r[-1] for r in rows])
        waves = lambda r: min(8, 512 // (-(-num(r, "vgpr") // 8) * 8))             # waves a SIMD by the vector registers
        static = num(mine[0], "lds") + (2 * 64 * 40 if "solve" in kernel else 0)   # the solver's tape at M = 40
        groups = lambda r, lds: min(4 * waves(r) // 4, 160 * 1024 // lds)          # blocks of 256 threads
        assert groups(mine[0], static) >= 4, mine                                   # bound to four: the fifth would cost scratch
        assert num(mine[0], "lds") <= num(twin[0], "lds") + 16, (mine, twin)        # the beam in LDS did not grow
        if "solve" in kernel:
            tape = 2 * 64 * 254
            assert num(mine[0], "lds") + tape <= 64 * 1024 and 2 * (num(mine[0], "lds") + tape) <= 160 * 1024, mine
    assert all(num(r, "scratch") == 0 for r in rows)
