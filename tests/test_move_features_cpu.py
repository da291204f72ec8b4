"""CPU-side checks of the 14-feature form of the linear placement family (include/tpl_learn.h: features 12 landing_height and 13
eroded_cells; _learn_lib.host_move_features, placement_score, search_choice and placement_solve in the 14 form; heuristic.py and
solve.py's argument handling):

  1. the mirror's drop, cleared rows and features 12 and 13 against a brute force written here on 20 x 10 cell arrays, which takes
     its drop from the column tops and the shape query's patterns as the rule says: a few thousand random boards x all 40 actions
     x all 7 pieces, with top-outs, the right clamp, overhangs under which the piece would fit lower than the tops let it fall, and
     split clears;
  2. the hand cases of the rule;
  3. the C oracle's move leaves the same board and row count as the mirror on the same cases;
  4. with w12 = w13 = 0 the 14 form gives the 12 form's choices, plans and solutions exactly, and equal scores;
  5. the recorded two-ply choices that the GPU test compares the search kernel with on 2,048 states are the mirror's as it stands (a
     slice) on the states the generator makes;
  6. the argument handling, the names, DELLACHERIE_WEIGHTS, the header and the kernels' resources -- none of which needs a GPU.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

import learn_ref as R
import tetris_piclim as T

ARANGE = np.arange(40)


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ the boards
def _cells_to_rows(cells):
    return (cells.astype(np.int64) << np.arange(10)).sum(axis=-1).astype(np.uint16)


def _rows_to_cells(rows):
    return ((np.asarray(rows).astype(np.int64)[..., None] >> np.arange(10)) & 1).astype(bool)


def _random_boards(count, seed):
    """Stacks of every height up to the top (so that pieces top out), filled at densities that leave overhangs and holes at the
    low end and rows one or two cells short of full at the high end; no row is full."""
    rng = np.random.default_rng(seed)
    height = rng.integers(0, 21, size=(count, 1, 1))
    density = rng.choice([0.35, 0.6, 0.85, 0.95], size=(count, 1, 1))
    cells = (np.arange(20)[None, :, None] >= 20 - height) & (rng.random((count, 20, 10)) < density)
    gap = rng.integers(0, 10, size=(count, 20))                # a full row loses one cell
    full = cells.all(axis=2)
    cells[np.nonzero(full) + (gap[full],)] = False
    return cells


def _board(text):
    """A board from its bottom rows, top to bottom, '#' filled."""
    cells = np.zeros((20, 10), bool)
    lines = text.split()
    for k, line in enumerate(lines):
        assert len(line) == 10
        cells[20 - len(lines) + k] = [ch == "#" for ch in line]
    return cells


EDGE_BOARDS = {
    "empty": _board(".........."),
    # a four-deep well at column 0: a vertical I clears four rows
    "well4": _board(".######### .######### .######### .#########"),
    # rows 16, 17 and 19 lack column 0 only, row 18 lacks column 5 too: a vertical I clears a split set of three
    "split": _board(".######### .######### .####.#### .#########"),
    # one row lacks columns 0 and 1: a flat piece clears it with two of its cells
    "two_cells": _board("..########"),
    # an overhang: column 3 is filled at row 15 only, with room beneath it in which a piece would fit (a slide in from the side would
    # reach it) and which the column tops do not let it fall into
    "overhang": _board("...#...... .......... .......... .......... #.#.######"),
    # a roof over nearly everything
    "roof": _board("#########. .......... .......... .........."),
    # filled to the top row but one: everything but a flat I tops out
    "tall": np.concatenate([np.zeros((1, 10), bool), np.tile(np.array([[True] * 9 + [False]]), (19, 1))]),
    "full_height": np.tile(np.array([[True] * 9 + [False]]), (20, 1)),
}


def _edge_cells():
    return np.stack(list(EDGE_BOARDS.values()))


# ------------------------------------------------------------------------------------------------ the brute force
def _piece_cells(piece, r):
    """(h, w, [4, 4] bool cells with [i, c] = mask row i, mask column c) from the shape query."""
    h, w, masks, _ = T._lib.shape_info(piece, r)
    cell = np.zeros((4, 4), bool)
    for i in range(h):
        for c in range(w):
            cell[i, c] = (masks[i] >> c) & 1
    assert cell.sum() == 4
    return h, w, cell


def _brute(cells, piece, r, l):
    """The rule of include/tpl_learn.h on cell arrays [K, 20, 10]: drop from the column tops under the piece, the lock, the rows
    among the piece's that are full, features 12 and 13, and the board after the cleared rows are taken out."""
    k = cells.shape[0]
    at = np.arange(k)
    h, w, pc = _piece_cells(piece, r)
    loc = min(l, 10 - w)
    top = np.where(cells.any(axis=1), cells.argmax(axis=1), 20)                     # [K, 10]
    drop = np.full(k, 99)
    for c in range(w):
        lowest = max(i for i in range(4) if pc[i, c])                               # the piece's lowest cell in its column c
        drop = np.minimum(drop, top[:, loc + c] - 1 - lowest)
    ok = drop >= 0
    after = cells.copy()
    for i, c in zip(*np.nonzero(pc)):
        row = np.where(ok, drop + i, 0)
        assert not after[at[ok], row[ok], loc + c].any()                            # from the tops the piece never overlaps
        after[at[ok], row[ok], loc + c] = True
    # the lowest position at which the piece would FIT, wherever it came from: under an overhang it is below the drop
    fit = np.full(k, -1)
    for d in range(0, 21 - h):
        free = np.ones(k, bool)
        for i, c in zip(*np.nonzero(pc)):
            free &= ~cells[:, d + i, loc + c]
        fit = np.where(free, d, fit)
    rows = np.arange(20)[None, :]
    cleared = after.all(axis=2) & (rows >= drop[:, None]) & (rows < drop[:, None] + h) & ok[:, None]
    n = cleared.sum(axis=1)
    inside = np.zeros(k, np.int64)
    for i, c in zip(*np.nonzero(pc)):
        inside += cleared[at, np.where(ok, drop + i, 0)] & ok
    landing = np.where(ok, 39 - 2 * drop - h, 0)
    final = np.zeros_like(after)
    for b in range(k):                                                              # the kept rows sink, empty rows enter at the top
        kept = after[b][~cleared[b]]
        final[b, 20 - kept.shape[0]:] = kept
    return drop, cleared, landing, n * inside, n, final, ok, fit


@pytest.fixture(scope="module")
def boards():
    cells = np.concatenate([_edge_cells(), _random_boards(3000, 11)])
    return cells, _cells_to_rows(cells)


def test_the_mirror_is_the_brute_force_on_every_piece_and_action(boards):
    m = _m()
    cells, rows = boards
    k = rows.shape[0]
    seen = dict(topout=0, clamp=0, split=0, eroded=set(), fits_lower=0)
    for piece in range(7):
        for a in range(40):
            r, l = a // 10, a % 10
            drop, cleared, landing, eroded, n, final, ok, fit = _brute(cells, piece, r, l)
            assert (fit[ok] >= drop[ok]).all()                 # where it falls to it fits; a straight fall from above cannot pass a top
            seen["fits_lower"] += int((fit[ok] > drop[ok]).sum())
            got = m.host_moves_traced(rows, piece, r, l, 250, 254, 0, 0)
            g_drop, g_cleared, g_landing, g_eroded = got[5:]
            assert np.array_equal(g_drop >= 0, ok), (piece, a)
            assert np.array_equal(g_drop[ok], drop[ok]), (piece, a)
            assert np.array_equal(g_cleared, cleared), (piece, a)
            assert np.array_equal(g_landing, landing) and np.array_equal(g_eroded, eroded), (piece, a)
            assert np.array_equal(got[1], n) and np.array_equal(got[0], _cells_to_rows(final)), (piece, a)
            assert np.array_equal(got[4] == m.STATE_LOST_TOPOUT, ~ok)
            assert landing.min() >= 0 and landing.max() <= 38 and eroded.max() <= 16
            f = m.host_move_features(rows, piece, r, l, 250, 254, 0, 0)
            assert all(np.array_equal(x, y) for x, y in zip(f, got[5:]))
            seen["topout"] += int((~ok).sum())
            seen["clamp"] += int(l > 10 - T._lib.shape_info(piece, r)[1])
            first, last = cleared.argmax(axis=1), 19 - cleared[:, ::-1].argmax(axis=1)
            seen["split"] += int(((n > 0) & (last - first + 1 > n)).sum())
            seen["eroded"] |= set(np.unique(eroded).tolist())
    # the cases the issue names were all met
    assert seen["topout"] > 1000 and seen["clamp"] == 40 and seen["split"] > 0 and seen["fits_lower"] > 1000, seen
    assert {0, 1, 2, 9, 16} <= seen["eroded"], seen


def test_the_drop_is_from_the_column_tops_not_a_slide():
    """The drop is the straight fall from above, which the column tops give exactly (the piece's columns have no gaps, so the first
    contact is always a lowest cell on a top): an O at columns 2..3 rests on row 15's cell although the piece would fit in the open
    rows below it, where only a slide in from the side could take it.  The brute-force test counts such cases on the random boards."""
    m = _m()
    rows = _cells_to_rows(EDGE_BOARDS["overhang"][None])
    drop, _, landing, eroded = m.host_move_features(rows, 6, 0, 2, 250, 254, 0, 0)
    assert drop[0] == 13 and landing[0] == 39 - 26 - 2 and eroded[0] == 0           # rows 13 and 14, on top of (15, 3)
    drop, *_ = m.host_move_features(rows, 6, 0, 4, 250, 254, 0, 0)                   # beside it: down to the bottom row's top
    assert drop[0] == 17


def test_the_hand_cases_of_the_rule():
    m = _m()
    f = lambda name, piece, r, l, **kw: [int(x[0]) for x in m.host_move_features(
        _cells_to_rows(EDGE_BOARDS[name][None]), piece, r, l, kw.get("L", 250), kw.get("M", 254), 0, kw.get("moves", 0))[2:]]
    assert f("empty", 0, 0, 3) == [0, 0]                        # I flat on an empty floor
    assert f("empty", 6, 0, 4) == [1, 0]                        # O on an empty floor
    assert f("well4", 0, 1, 0) == [39 - 32 - 4, 16]             # a vertical I into the four-deep well: four rows, four cells
    assert f("split", 0, 1, 0) == [3, 9]                        # three rows of a split set, three cells
    assert f("two_cells", 6, 0, 0) == [1, 2]                    # an O clears one row with two of its cells in it
    assert f("two_cells", 1, 2, 0)[1] == 0 and f("two_cells", 0, 0, 0) == [2, 0]    # no clear: both rest a row up and leave a gap
    for piece in range(1, 7):                                   # top-outs: zeros
        assert f("full_height", piece, 0, 0) == [0, 0]
    assert f("tall", 0, 0, 0) == [38, 0]                        # the flat I still fits the top row: the highest landing
    # a finished board has no move: mirror_phi, the reference of the GPU features test, gives it fourteen zeros, which score 0
    rows = _cells_to_rows(EDGE_BOARDS["well4"][None].repeat(2, axis=0))
    phi, _ = mirror_phi(rows, np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64), np.array([True, False]), 250, 254)
    assert phi[0, 10, 13] == 16 and phi[0].any(axis=1).all() and not phi[1].any()
    assert m.placement_score(phi[1], np.arange(14, dtype=np.float32)).tolist() == [0.0] * 40


def test_the_c_oracle_leaves_the_same_board_and_row_count(oracle, boards):
    m = _m()
    cells, rows = boards
    pick = np.concatenate([np.arange(len(EDGE_BOARDS)), np.arange(len(EDGE_BOARDS), rows.shape[0], 61)])
    sub = rows[pick]
    for piece in range(7):
        for a in range(40):
            got = m.host_moves_traced(sub, piece, a // 10, a % 10, 250, 254, 0, 0)
            for i in range(sub.shape[0]):
                g = oracle.Game(250, 254, rows=sub[i], pieces=[piece, 0])
                g.move(a // 10, a % 10)
                assert np.array_equal(g.rows, got[0][i]) and g.lines_cleared == got[1][i], (piece, a, i)
                assert (g.state == 0) == (got[4][i] == 0) and g.moves_used == got[3][i], (piece, a, i)


# ------------------------------------------------------------------------------------------------ the mirror on packed states
def mirror_phi(rows, piece, lines, moves, running, L, M):
    """phi14 [K, 40, 14] by the mirror (zero for a board that does not run) and what every move leaves."""
    m = _m()
    k = rows.shape[0]
    phi = np.zeros((k, 40, 14), np.int64)
    left = dict(rows=np.zeros((k, 40, 20), np.uint16), lines=np.zeros((k, 40), np.int64), moves=np.zeros((k, 40), np.int64),
                state=np.zeros((k, 40), np.int64))
    for lo in range(0, k, 512):                                # 20 K moves at a time: the mirror holds a cell array per move
        hi = min(k, lo + 512)
        at = np.repeat(np.arange(lo, hi), 40)
        a = np.tile(ARANGE, hi - lo)
        r2, n, l2, m2, s2, _, _, land, erod = m.host_moves_traced(rows[at], piece[at], a // 10, a % 10, L, M, lines[at], moves[at])
        head = np.stack([n, s2 == m.STATE_WON, s2 >= m.STATE_LOST_LIMIT], axis=1).astype(np.int64)
        phi[lo:hi] = np.concatenate([head, m.board_features(r2), np.stack([land, erod], axis=1)], axis=1).reshape(hi - lo, 40, 14)
        for key, v in (("rows", r2), ("lines", l2), ("moves", m2), ("state", s2)):
            left[key][lo:hi] = v.reshape((hi - lo, 40) + v.shape[1:])
    phi[~running] = 0
    return phi, left


class MirrorStates:
    """Packed states (planes A, B uint32 [K, 4]) decoded, with the mirror's phi14 of all 40 actions of each."""

    def __init__(self, A, B, L, M):
        self.A, self.B, self.L, self.M, self.n = A, B, L, M, A.shape[0]
        f = R.decode_state(A, B)
        self.rows, self.cur, self.nxt = f["rows"], f["cur"].astype(np.int64), f["nxt"].astype(np.int64)
        self.lines, self.moves, self.state = (f[k].astype(np.int64) for k in ("lines", "moves", "state"))
        self.running = self.state == 0
        self.phi, self.left = mirror_phi(self.rows, self.cur, self.lines, self.moves, self.running, L, M)
        self.canonical = _m().canonical_actions(self.cur[:, None], ARANGE[None, :])
        self.distinct = self.canonical == ARANGE[None, :]


def mirror_search(s, idx, rows_w, chunk=64):
    """search_choice on the mirror's two-ply features of states idx of a MirrorStates, one weight row per state."""
    m = _m()
    action, second, score = [], [], []
    for lo in range(0, idx.size, chunk):
        sub, w = idx[lo:lo + chunk], rows_w[lo:lo + chunk]
        k = sub.size
        phi1, left = s.phi[sub], {key: v[sub] for key, v in s.left.items()}
        done1 = (left["state"] != 0) | ~s.running[sub][:, None]
        flat = lambda x: x.reshape((k * 40,) + x.shape[2:])
        phi2, _ = mirror_phi(flat(left["rows"]), np.repeat(s.nxt[sub], 40), flat(left["lines"]), flat(left["moves"]), ~flat(done1), s.L, s.M)
        phi2 = phi2.reshape(k, 40, 40, 14)
        phi2[..., 0] += phi1[:, :, None, 0]
        phi2[..., 12:] += phi1[:, :, None, 12:]
        distinct2 = m.canonical_actions(s.nxt[sub][:, None], ARANGE[None, :]) == ARANGE[None, :]
        a, b, v = m.search_choice(phi1, done1, s.distinct[sub], phi2, distinct2, w)
        action.append(np.where(s.running[sub], a, 0).astype(np.uint8)), second.append(b), score.append(v)
    return np.concatenate(action), np.concatenate(second), np.concatenate(score).astype(np.float32)


def population(n):
    """Three weight rows with a short last member: random, classical with the two move weights, non-zero only in 12 and 13."""
    gen = np.random.default_rng(n)
    per = -(-n // 3) + (1 if n > 5 else 0)
    members = -(-n // per)
    w = np.zeros((members, 14), np.float32)
    w[0] = gen.normal(size=14)
    if members > 1:
        w[1] = np.concatenate([np.array(T.CLASSICAL_WEIGHTS), np.array([-0.25, 0.5], np.float32)])
    if members > 2:
        w[2, 12:] = [-1.0, 2.0]
    return w, per


SEARCH_L, SEARCH_M, SEARCH_N = 10, 40, 2048


def search_states(count=SEARCH_N, seed=2048):
    """Mid-game states made on the host for the recorded two-ply reference: stacks of up to twelve rows (so that two pieces fit and
    rows are cleared), every piece id 0..7 in the window, lines and moves anywhere in the game, a tenth of the boards finished."""
    gen = np.random.default_rng(seed)
    cells = _random_boards(4 * count, seed)
    cells = cells[cells.any(axis=2).sum(axis=1) <= 12][:count]
    assert cells.shape[0] == count
    window = np.zeros(count, np.uint64)
    for j in range(12):
        window |= gen.integers(0, 8, count).astype(np.uint64) << np.uint64(3 * j)
    state = np.where(gen.random(count) < 0.1, gen.integers(1, 4, count), 0)
    return R.pack_state(_cells_to_rows(cells), gen.integers(0, SEARCH_L, count), gen.integers(0, SEARCH_M, count), state, 0, window)


def test_the_recorded_search_reference_is_the_generators_and_the_mirrors():
    g = load_golden("move_search_mirror.npz")
    A, B = search_states()
    assert np.array_equal(g["A"], A) and np.array_equal(g["B"], B)
    w, per = population(SEARCH_N)
    assert np.array_equal(g["weights"], w) and int(g["per"]) == per and g["action"].shape == (SEARCH_N,)
    idx = np.arange(5, SEARCH_N, 43)                           # 48 states, every member among them
    s = MirrorStates(A[idx], B[idx], SEARCH_L, SEARCH_M)
    action, second, score = mirror_search(s, np.arange(idx.size), w[idx // per])
    assert np.array_equal(g["action"][idx], action) and np.array_equal(g["second"][idx], second)
    assert np.array_equal(g["score"][idx].view(np.uint32), score.view(np.uint32))
    assert (g["second"] != 255).sum() > SEARCH_N // 2 and np.unique(g["action"]).size >= 30


# ------------------------------------------------------------------------------------------------ 4. the reduction
def _phi(rows, piece, L, M, lines, moves):
    """phi14 [K, 40, 14] of `piece` on K running boards, and what every move leaves."""
    m = _m()
    out, left = [], []
    for a in range(40):
        r2, n, l2, m2, s2, _, _, land, erod = m.host_moves_traced(rows, piece, a // 10, a % 10, L, M, lines, moves)
        head = np.stack([n, s2 == m.STATE_WON, s2 >= m.STATE_LOST_LIMIT], axis=1).astype(np.int64)
        phi = np.concatenate([head, m.board_features(r2), np.stack([land, erod], axis=1)], axis=1)
        phi[s2 == m.STATE_LOST_TOPOUT, 12:] = 0
        out.append(phi), left.append((r2, l2, m2, s2))
    return np.stack(out, axis=1), left


@pytest.fixture(scope="module")
def two_plies():
    m = _m()
    rng = np.random.default_rng(5)
    k, L, M = 24, 3, 6
    cells = _random_boards(400, 3)
    cells = cells[(cells.any(axis=2).sum(axis=1) < 14)][:k]                         # room for two pieces
    rows = _cells_to_rows(cells)
    cur, nxt = rng.integers(0, 7, k), rng.integers(0, 7, k)
    lines, moves = rng.integers(0, 3, k), rng.integers(0, 5, k)
    phi1, left = [], []
    phi1 = np.zeros((k, 40, 14), np.int64)
    phi2 = np.zeros((k, 40, 40, 14), np.int64)
    done1 = np.zeros((k, 40), bool)
    for p in range(7):
        sel = np.flatnonzero(cur == p)
        if not sel.size:
            continue
        f, after = _phi(rows[sel], p, L, M, lines[sel], moves[sel])
        phi1[sel] = f
        for a in range(40):
            r1, l1, m1, s1 = after[a]
            done1[sel, a] = s1 != 0
            for q in range(7):
                sub = np.flatnonzero(nxt[sel] == q)
                if not sub.size:
                    continue
                g, _ = _phi(r1[sub], q, L, M, l1[sub], m1[sub])
                g[:, :, 0] += f[sub, a, 0][:, None]                                 # cleared, landing and eroded add up
                g[:, :, 12:] += f[sub, a, 12:][:, None, :]
                phi2[sel[sub], a] = g
    at = np.arange(40)
    distinct1 = m.canonical_actions(cur[:, None], at[None, :]) == at[None, :]
    distinct2 = m.canonical_actions(nxt[:, None], at[None, :]) == at[None, :]
    return phi1, done1, distinct1, phi2, distinct2


def _weights14(seed, rows=None):
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 3, size=(14,) if rows is None else (rows, 14)).astype(np.float32)
    w[..., 1], w[..., 2] = 50, -50
    return w


def test_with_zero_move_weights_score_and_search_are_the_12_form(two_plies):
    m = _m()
    phi1, done1, distinct1, phi2, distinct2 = two_plies
    for seed in range(4):
        w = _weights14(seed)
        w[12:] = [0.0, -0.0][seed % 2]
        assert np.array_equal(m.placement_score(phi1, w), m.placement_score(phi1[..., :12], w[:12]))        # -0 == +0
        a14 = m.search_choice(phi1, done1, distinct1, phi2, distinct2, w)
        a12 = m.search_choice(phi1[..., :12], done1, distinct1, phi2[..., :12], distinct2, w[:12])
        assert np.array_equal(a14[0], a12[0]) and np.array_equal(a14[1], a12[1]) and np.array_equal(a14[2], a12[2])
    # and with them the choice moves: the features are not inert
    w = _weights14(9)
    w[3:12] = 0
    a14 = m.search_choice(phi1, done1, distinct1, phi2, distinct2, w)
    a12 = m.search_choice(phi1[..., :12], done1, distinct1, phi2[..., :12], distinct2, w[:12])
    assert not np.array_equal(a14[0], a12[0])
    # one row per board
    rows = _weights14(2, phi1.shape[0])
    per = m.search_choice(phi1, done1, distinct1, phi2, distinct2, rows)
    for i in (0, 7, phi1.shape[0] - 1):
        one = m.search_choice(phi1[i:i + 1], done1[i:i + 1], distinct1[i:i + 1], phi2[i:i + 1], distinct2[i:i + 1], rows[i])
        assert (per[0][i], per[1][i], per[2][i]) == (one[0][0], one[1][0], one[2][0])


def test_with_zero_move_weights_the_solver_is_the_12_form_and_its_14_form_wins(oracle):
    m = _m()
    g = load_golden("carved_L5_M20.npz")
    rows, pieces, L, M = g["rows"][:10], g["pieces"][:10], int(g["L"]), int(g["M"])
    classical = np.array(T.CLASSICAL_WEIGHTS)
    for width in (1, 4):
        w = np.concatenate([classical, np.zeros(2, np.float32)])
        s14 = m.placement_solve(rows, pieces, L, M, w, width)
        s12 = m.placement_solve(rows, pieces, L, M, classical, width)
        for x, y in zip(s14, s12):
            assert np.array_equal(x, y)
        assert s12[0].any()
    w = np.concatenate([classical, np.array([-0.25, 0.5], np.float32)])
    solved, length, actions, best = m.placement_solve(rows, pieces, L, M, w, 4)
    assert solved.any()
    for i in np.flatnonzero(solved):
        game = oracle.Game(L, M, rows=rows[i], pieces=pieces[i])
        for j in range(length[i]):
            assert game.state == 0
            game.move(int(actions[i, j]) // 10, int(actions[i, j]) % 10)
        assert game.state == 1 and game.moves_used == length[i]
    assert not np.array_equal(best, m.placement_solve(rows, pieces, L, M, classical, 4)[3])


# ------------------------------------------------------------------------------------------------ 6. arguments and names
class _Env:
    """What the heuristic module reads of an environment before it touches the device."""

    def __init__(self, n):
        import torch
        self.L, self.M, self.num_envs, self.reward_params, self.device = 5, 20, n, (0.0, 1.0, 0.0), torch.device("cpu")
        self.auto_reset = True


def test_weight_shapes_names_and_the_dellacherie_row():
    import torch
    h, m = T.heuristic, _m()
    env = _Env(8)
    for w, members in (np.zeros(14), 1), (np.zeros((2, 14)), 2), (torch.zeros(4, 14), 4), ([0] * 14, 1):
        for p in (h.HeuristicPolicy(env, w), h.HeuristicPolicy(env, w, depth=2), h.BeamPolicy(env, w, 3, 8)):
            assert p.members == members and p.features == 14 and tuple(p.weights.shape) == (members, 14)
            assert p.weights.dtype == torch.float32 and tuple(p._buffer.shape) == (members, 16)
    p12 = h.HeuristicPolicy(env, np.ones((2, 12)))
    assert p12.features == 12 and tuple(p12.weights.shape) == (2, 12) and p12.weights.is_contiguous()
    assert p12.weights.data_ptr() == p12._buffer.data_ptr() and tuple(p12._buffer.shape) == (2, 12)
    for shape in ((15,), (16,), (2, 13), (2, 15), (2, 16), (13,), (0, 14)):
        with pytest.raises(ValueError, match="shape"):
            h.HeuristicPolicy(env, np.zeros(shape, np.float32))
        with pytest.raises(ValueError, match="shape"):
            h.BeamPolicy(env, np.zeros(shape, np.float32), 2, 4)
    p = h.HeuristicPolicy(env, np.zeros((2, 14)))
    p.set_weights(np.arange(28).reshape(2, 14))
    assert np.array_equal(p.weights.numpy(), np.arange(28, dtype=np.float32).reshape(2, 14))
    assert np.array_equal(p._buffer.numpy()[:, 14:], np.zeros((2, 2), np.float32))   # entries 14 and 15 stay zero
    for other in (np.zeros((2, 12)), np.zeros(14), np.zeros((2, 16))):
        with pytest.raises(ValueError, match="shape"):
            p.set_weights(other)
    with pytest.raises(ValueError, match="keep their shape"):
        p12.set_weights(np.zeros((2, 14)))
    with pytest.raises(ValueError, match="finite"):
        p.set_weights(np.full((2, 14), np.inf))
    # tune_heuristic refuses before it builds an environment (config_pool None would fail there)
    for kw in (dict(features=14, init_mean=np.zeros(12)), dict(features=12, init_mean=np.zeros(14)), dict(init_mean=np.zeros(14)),
               dict(features=14, init_mean=np.zeros(16))):
        with pytest.raises(ValueError, match="init_mean"):
            h.tune_heuristic(2, 2, None, **kw)
    for features in (13, 16, 0, True, 14.5, "14"):
        with pytest.raises(ValueError, match="features"):
            h.tune_heuristic(2, 2, None, features=features)
    # solve_configs' weight row
    s = T.solve
    assert s._weight_row(np.zeros(14)).shape == (14,) and s._weight_row(np.zeros((1, 14))).shape == (14,)
    assert s._weight_row(None).shape == (12,)
    for shape in ((13,), (15,), (16,), (2, 14), (1, 16)):
        with pytest.raises(ValueError, match="one row"):
            s._weight_row(np.zeros(shape))
    with pytest.raises(ValueError, match="move"):
        h.placement_features(_Env(8), move=1)
    # the names and the named row
    assert T.MOVE_FEATURE_NAMES[:12] == T.FEATURE_NAMES and T.MOVE_FEATURE_NAMES[12:] == ("landing_height", "eroded_cells")
    assert len(T.FEATURE_NAMES) == 12 and T.MOVE_FEATURE_NAMES is m.MOVE_FEATURE_NAMES
    d = T.DELLACHERIE_WEIGHTS
    assert d.dtype == np.float32 and d.shape == (14,) and not d.flags.writeable
    with pytest.raises(ValueError):
        d[0] = 1.0
    want = dict(holes=-4, row_transitions=-1, column_transitions=-1, wells=-1, landing_height=-0.5, eroded_cells=1, won=100, lost=-100)
    assert {n: float(v) for n, v in zip(T.MOVE_FEATURE_NAMES, d)} == {n: float(want.get(n, 0)) for n in T.MOVE_FEATURE_NAMES}
    # the mirror's own refusals
    with pytest.raises(ValueError, match="12 or both in 14"):
        m.placement_score(np.zeros((3, 14)), np.zeros(12))
    with pytest.raises(ValueError, match="12 or both in 14"):
        m.placement_score(np.zeros((3, 13)), np.zeros(13))
    with pytest.raises(ValueError, match="12 or of 14"):
        m.placement_solve(np.zeros((1, 20), np.uint16), np.zeros((1, 3), np.uint8), 1, 2, np.zeros(16), 1)
    assert m.padded_weights(np.ones((2, 12), np.float32)).shape == (2, 12)
    assert np.array_equal(m.padded_weights(np.ones((2, 14), np.float32)), np.concatenate([np.ones((2, 14)), np.zeros((2, 2))], 1))


ENTRIES = ("tpl_placement_features_move", "tpl_placement_act_move", "tpl_placement_search_move", "tpl_placement_beam_move",
           "tpl_placement_solve_move")
KERNELS = ("placement_features_move_kernel", "placement_act_move_kernel", "placement_search_move_kernel",
           "placement_beam_move_kernel", "placement_solve_move_kernel")


def test_the_header_states_the_rule_and_declares_the_five_entries():
    import ctypes
    m = _m()
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_\w+)\s*\(", text))
    assert declared == set(m.LEARN_SYMBOLS) and set(ENTRIES) <= declared
    assert "#define TPL_NUM_MOVE_FEATURES 14" in raw and "#define TPL_MOVE_WEIGHT_STRIDE 16" in raw
    assert "left out on purpose" not in raw and "39 - 2 drop - h" in raw
    lib = ctypes.CDLL(m.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name), name
        twin = name[:-len("_move")]
        proto = lambda n: re.sub(r"\s+", " ", re.search(r"int %s\((.*?)\);" % n, text, flags=re.S).group(1))
        assert proto(name) == proto(twin), name                 # the same arguments as the 12-feature twin


def test_every_refusal_of_the_five_entries_comes_back_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error().decode()
    fake, E = 1 << 20, -1                                      # aligned, never dereferenced: every call is refused
    rc = lambda *a: a[0](*a[1:])
    F, A, S, B, V = (getattr(lib, n) for n in ENTRIES)
    # the planes, n, L and M: check_planes', under each entry's own name
    for fn, name, tail in ((F, ENTRIES[0], (fake, None, None)), (A, ENTRIES[1], (fake, 8, fake, None, None)),
                           (S, ENTRIES[2], (fake, 8, fake, None, None, None)), (B, ENTRIES[3], (fake, 8, 2, 4, fake, None, None, None))):
        for planes, n, L, M, what in (((None, fake), 8, 5, 20, "null"), ((fake, fake + 8), 8, 5, 20, "16-byte"), ((fake, fake), 0, 5, 20, "positive"),
                                      ((fake, fake), (1 << 31) // 40 + 1, 5, 20, "too large"), ((fake, fake), 8, 251, 20, "L and M"),
                                      ((fake, fake), 8, 5, 255, "L and M")):
            assert fn(*planes, n, L, M, *tail) < 0 and name in err() and what in err(), (name, what, err())
    assert F(fake, fake, 8, 5, 20, None, None, None) < 0 and "features is required" in err()
    assert F(fake, fake, 8, 5, 20, fake + 8, None, None) < 0 and "16-byte aligned" in err()        # 8 is the twin's alignment
    assert A(fake, fake, 8, 5, 20, None, 8, fake, None, None) < 0 and "weights and action" in err()
    assert A(fake, fake, 8, 5, 20, fake, 0, fake, None, None) < 0 and "boards_per_member" in err()
    assert A(fake, fake, 8, 5, 20, fake + 8, 8, fake, None, None) < 0 and "weights must be 16-byte" in err()
    assert S(fake, fake, 8, 5, 20, fake, 8, fake, None, fake + 2, None) < 0 and "score must be 4-byte" in err()
    for depth, width, what in ((0, 4, "depth"), (13, 4, "depth"), (2, 0, "width"), (2, 65, "width")):
        assert B(fake, fake, 8, 5, 20, fake, 8, depth, width, fake, None, None, None) < 0 and what in err()
    ok = (fake, fake, 8, 5, 20, fake, 4, fake, fake, fake, None, None)
    for at, value, what in ((0, None, "null"), (2, 0, "positive"), (3, 251, "L and M"), (4, 255, "L and M"), (5, fake + 4, "weights must be 16"),
                            (6, 65, "width"), (8, fake + 2, "solution_len"), (0, fake + 1, "rows must be 2-byte")):
        args = list(ok)
        args[at] = value
        assert V(*args) < 0 and ENTRIES[4] in err() and what in err(), (at, err())


def test_the_five_kernels_use_no_scratch_and_keep_their_twins_groups_a_cu():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    num = lambda r, what: int(r[r.index(what) - 1])
    for kernel in KERNELS:
        mine = [r for r in rows if kernel in r[-1]]
        twin = [r for r in rows if kernel.replace("_move", "") in r[-1]]
        assert len(mine) == 1 and len(twin) == 1, (kernel, [r[-1] for r in rows])
        assert num(mine[0], "scratch") == 0, mine
        waves = lambda r: min(8, 512 // (-(-num(r, "vgpr") // 8) * 8))             # waves a SIMD by the vector registers
        per_group = 5 if ("_act_" in kernel or "_search_" in kernel) else 4        # blocks of 320 and of 256 threads
        groups = lambda r: min(4 * waves(r) // per_group, 160 * 1024 // max(num(r, "lds"), 1))
        if "_beam_" in kernel:                                                      # bound to four: the fifth would cost scratch
            assert groups(twin[0]) == 5 and groups(mine[0]) == 4, (mine, twin)
        else:
            assert groups(mine[0]) == groups(twin[0]), (mine, twin)                 # workgroups a CU: the solver keeps its five
        assert num(mine[0], "lds") <= num(twin[0], "lds") + 128, (mine, twin)       # the beam in LDS did not grow: a weight row did
    assert all(num(r, "scratch") == 0 for r in rows)


def test_the_body_is_shared_not_copied():
    here = os.path.dirname(_m()._UNITS[-1])
    units = [os.path.basename(p) for p in _m()._UNITS]
    for unit in ("heuristic", "beam", "solve"):
        twin = open(os.path.join(here, unit + "_move.hip")).read()
        code = [l for l in twin.splitlines() if l.strip() and not l.startswith("//")]
        assert code == ["#define TPL_PLACEMENT_MOVE_UNIT", f'#include "{unit}.hip"'], unit
        assert unit + "_move.hip" in units
    placement = open(os.path.join(here, "tpl_placement.h")).read()
    assert placement.count("move_trace(") == 2                                     # defined, and used in the one place: placed_move
    for unit in ("heuristic.hip", "beam.hip", "solve.hip"):                        # the units move through placed_move / first_move
        assert "tpl::move_board" not in open(os.path.join(here, unit)).read(), unit
