"""CPU-side checks of the exact search from a node and of the proved move labels (include/tpl_learn.h's rules;
_learn_lib.placement_exact_nodes and placement_exact_labels; solve.py's prove_nodes, label_moves, label_states and blunders;
tpl_placement_exact_nodes[_move] and tpl_placement_exact_labels[_move] in csrc/learn/exact_nodes.hip).

The oracle is the SHIFTED GAME: a node (rows, lines, moves, entry) of the game (L, M) is the configuration (rows,
pieces[entry, moves:]) of the game (L - lines, M - moves), searched by the existing _learn_lib.placement_exact.

The nodes (node_sets below; the GPU tests use the same) come from the first 32 configurations of tests/golden/carved_L5_M20.npz: the
board after move k = sol_len - back of the recorded solution, in the game (5, sol_len + spare), grouped by M.  The lists of a group
are stored in reverse and named through `entry`, so that an entry is not a node's own index.

  1. the nodes mirror against placement_exact on each shifted configuration, one by one; the root searches in the game (5, 20);
  2. with lines = moves = 0 and entry = arange(n) the nodes mirror is placement_exact on test_solve_cpu's small games;
  3. the labels against moves made on the C oracle and the nodes mirror applied to every child; the counts of the three sets;
  4. every label 1 replays on the C oracle to a win after exactly `length` moves from the node; for every label 2 of the exact-budget
     set an exhaustive enumeration on the oracle finds no win; the solution's own move is labelled 1; best has the least length;
  5. the cap: max_nodes = 1 gives label 3 and never 2 wherever the running child's search needs a second node (it has no winning
     grandchild, and something is left to search); a search of one node is not cut short by it; a larger cap changes no 1 or 2;
  6. finished nodes; blunders; the Python refusals, every refusal of the four entries, the header against the exports, the resources.
"""
import ctypes
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_solve_cpu import CW, Node, _first_winning_ply, _placements

import tetris_piclim as T

COUNT, L5, CAP = 32, 5, 4096
SETS = {"back3": (3, 0), "back4": (4, 0), "back3_spare1": (3, 1)}          # name -> (back, spare moves)


def _m():
    return T._learn_lib


def weights_of(count):
    return CW if count == 12 else np.array(T.DELLACHERIE_WEIGHTS, np.float32)


@functools.lru_cache(maxsize=None)
def node_sets(key):
    """The groups of one input set, a dict each: M, idx (the configurations), rows [k, 20], lines, moves, entry [k], pieces
    [k, M + 1] (stored in reverse: entry = k - 1 - j), sol_move [k] (the recorded solution's move from the node, canonical)."""
    back, spare = SETS[key]
    g = load_golden("carved_L5_M20.npz")
    assert int(g["L"]) == L5
    sol_len = g["sol_len"][:COUNT].astype(np.int64)
    out = []
    for length in sorted(set(sol_len.tolist())):
        idx = np.flatnonzero(sol_len == length)
        M, k = length + spare, length - back
        assert k >= 1
        lists = np.ascontiguousarray(g["pieces"][idx, :M + 1][::-1])
        entry = (idx.size - 1 - np.arange(idx.size)).astype(np.uint32)
        moves = g["r_moves"][idx, k - 1]
        assert (moves == k).all() and (g["r_state"][idx, k - 1] == 0).all()
        sol = g["sol"][idx, k].astype(np.int64)
        sol_move = _m().canonical_actions(lists[entry, k], 10 * sol[:, 0] + sol[:, 1])
        out.append(dict(M=M, idx=idx, rows=g["r_rows"][idx, k - 1], lines=g["r_lines"][idx, k - 1], moves=moves, entry=entry,
                        pieces=lists, sol_move=sol_move))
    assert sum(grp["idx"].size for grp in out) == COUNT
    return out


def root_nodes(back):
    """The nodes `back` moves before the end of the recorded solutions, in the game (5, 20): one group, entry = the configuration."""
    g = load_golden("carved_L5_M20.npz")
    at = np.arange(COUNT)
    k = g["sol_len"][:COUNT].astype(np.int64) - back
    return dict(M=int(g["M"]), rows=g["r_rows"][at, k - 1], lines=g["r_lines"][at, k - 1], moves=g["r_moves"][at, k - 1],
                entry=at.astype(np.uint32), pieces=g["pieces"][:COUNT])


@functools.lru_cache(maxsize=None)
def mirror_nodes(key, count, cap=CAP, shortest=True):
    """The nodes mirror on every group of a set: a list of six-tuples.  Computed once; nobody writes to it."""
    return [_m().placement_exact_nodes(grp["rows"], grp["lines"], grp["moves"], grp["entry"], grp["pieces"], L5, grp["M"], weights_of(count),
                                       cap, shortest) for grp in node_sets(key)]


@functools.lru_cache(maxsize=None)
def mirror_labels(key, count, cap=CAP):
    """The labels mirror on every group of a set: a list of (label, length, nodes)."""
    return [_m().placement_exact_labels(grp["rows"], grp["lines"], grp["moves"], grp["entry"], grp["pieces"], L5, grp["M"],
                                        weights_of(count), cap) for grp in node_sets(key)]


def children_on_the_oracle(O, grp):
    """Every distinct placement of every node of a group, moved on the C oracle under (5, M) and judged by the move bound: a list of
    (node j, b, rows, lines, moves, state) with a dead child's state turned lost at the limit."""
    m, out = _m(), []
    for j in range(grp["idx"].size):
        lines, moves, lst = int(grp["lines"][j]), int(grp["moves"][j]), grp["pieces"][grp["entry"][j]]
        node = Node(O, L5, grp["M"], grp["rows"][j], lst, lines, moves, 0, moves)
        for b in _placements(lst[moves]):
            c = node.child(b).g
            state = c.state
            if state == 0 and m.move_bound(c.rows, L5, grp["M"], c.lines_cleared, c.moves_used, 0)["dead"][0]:
                state = 2
            out.append((j, b, c.rows, c.lines_cleared, c.moves_used, state))
    return out


# ------------------------------------------------------------------------------------------------ 1. the shifted game
@pytest.mark.parametrize("key", list(SETS))
def test_the_nodes_mirror_is_placement_exact_on_each_shifted_configuration(key):
    m = _m()
    for count in (12, 14):
        for grp, got in zip(node_sets(key), mirror_nodes(key, count)):
            M = grp["M"]
            assert [x.dtype for x in got] == [np.uint8, np.uint8, np.int32, np.uint8, np.int32, np.uint32]
            assert got[3].shape == (grp["idx"].size, M) and got[3].flags.c_contiguous
            for j in range(grp["idx"].size):
                lines, moves = int(grp["lines"][j]), int(grp["moves"][j])
                want = m.placement_exact(grp["rows"][j:j + 1], grp["pieces"][grp["entry"][j]][None, moves:], L5 - lines, M - moves,
                                         weights_of(count), CAP)
                for name, x, y in zip("solved proved length actions bound nodes".split(), got, want):
                    if name == "actions":
                        assert np.array_equal(x[j, :M - moves], y[0]) and (x[j, M - moves:] == 255).all(), (key, j)
                    else:
                        assert x[j] == y[0] and x.dtype == y.dtype, (key, name, j)
            back = SETS[key][0]
            assert got[0].all() and got[1].all() and (got[2] == back).all()          # the recorded solution is there, and no shorter one


def test_the_root_searches_near_the_end_take_a_few_nodes_and_find_the_recorded_length():
    for back, most in ((2, 2), (3, 6), (4, 17)):
        r = root_nodes(back)
        solved, proved, length, actions, bound, nodes = _m().placement_exact_nodes(r["rows"], r["lines"], r["moves"], r["entry"], r["pieces"],
                                                                                  L5, r["M"], CW, CAP)
        assert solved.all() and proved.all() and (length == back).all() and nodes.max() <= most and (bound <= back).all()
        assert (actions[:, back:] == 255).all() and (actions[:, :back] < 40).all()


# ------------------------------------------------------------------------------------------------ 2. a root is a node
@pytest.mark.parametrize("L,M,game_L,count", [(1, 1, 1, 24), (1, 2, 1, 24), (2, 2, 1, 24), (2, 2, 2, 24), (2, 3, 2, 6), (2, 3, 1, 6)])
def test_at_move_0_the_nodes_mirror_is_placement_exact_byte_for_byte(L, M, game_L, count):
    m = _m()
    rows, pieces = T.generate_configs(game_L, M, count, seed=31 + M)
    zero = np.zeros(count, np.uint8)
    for w in (CW, weights_of(14)):
        for shortest in (True, False):
            want = m.placement_exact(rows, pieces, L, M, w, 1 << 16, shortest)
            got = m.placement_exact_nodes(rows, zero, zero, np.arange(count), pieces, L, M, w, 1 << 16, shortest)
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ 3. the labels
COUNTS = {"back3": (33, 617, 6, 1), "back4": (35, 665, 12, 3), "back3_spare1": (79, 571, 199, 15)}     # wins, losses, largest, several wins


@pytest.mark.parametrize("key", list(SETS))
def test_the_labels_are_the_nodes_mirror_applied_to_the_children_made_on_the_oracle(oracle, key):
    m = _m()
    total = np.zeros(4, np.int64)
    largest = several = 0
    for grp, (label, length, nodes) in zip(node_sets(key), mirror_labels(key, 12)):
        k, M = grp["idx"].size, grp["M"]
        assert (label.dtype, length.dtype, nodes.dtype) == (np.uint8, np.int32, np.uint32) and label.shape == length.shape == nodes.shape == (k, 40)
        kids = children_on_the_oracle(oracle, grp)
        seen = np.zeros((k, 40), bool)
        run = [c for c in kids if c[5] == 0]
        for j, b, _, _, _, state in kids:
            seen[j, b] = True
            if state == 1:
                assert (label[j, b], length[j, b], nodes[j, b]) == (1, 1, 0)
            elif state != 0:
                assert (label[j, b], length[j, b], nodes[j, b]) == (2, 0, 0)
        assert (label[~seen] == 0).all() and (length[~seen] == 0).all() and (nodes[~seen] == 0).all() and (label[seen] != 0).all()
        if run:
            solved, proved, sol_len, _, _, count = m.placement_exact_nodes(
                np.array([c[2] for c in run]), np.array([c[3] for c in run]), np.array([c[4] for c in run]),
                np.array([grp["entry"][c[0]] for c in run]), grp["pieces"], L5, M, CW, CAP)
            for (j, b, *_), s, p, ln, cnt in zip(run, solved, proved, sol_len, count):
                want = (1, 1 + ln, cnt) if s else (2, 0, cnt) if p else (3, 0, cnt)
                assert (label[j, b], length[j, b], nodes[j, b]) == want, (key, j, b)
        for v in range(4):
            total[v] += (label == v).sum()
        largest, several = max(largest, int(nodes.max())), several + int(((label == 1).sum(axis=1) > 1).sum())
        # the recorded solution's own move is proved winning, in no more moves than the solution has left
        at = np.arange(k)
        assert (label[at, grp["sol_move"]] == 1).all() and (length[at, grp["sol_move"]] <= SETS[key][0]).all()
        # best: the least length among the proved-winning moves, the lowest placement among those
        best = m.best_labelled_move(label, length)
        torch = pytest.importorskip("torch")
        assert np.array_equal(best, T.solve._best_move(torch.from_numpy(label), torch.from_numpy(length)).numpy())
        for j in range(k):
            wins = np.flatnonzero(label[j] == 1)
            assert best[j] == wins[length[j, wins] == length[j, wins].min()][0]
    wins, losses, most, multi = COUNTS[key]
    assert (total[1], total[2], total[3], largest, several) == (wins, losses, 0, most, multi), (total.tolist(), largest, several)
    # the fourteen weights order the searches differently and prove the same
    for (label, length, _), (label14, length14, _) in zip(mirror_labels(key, 12), mirror_labels(key, 14)):
        assert np.array_equal(label, label14) and np.array_equal(length, length14)


# ------------------------------------------------------------------------------------------------ 4. checks outside the mirror
@pytest.mark.parametrize("key", list(SETS))
def test_every_proved_winning_move_replays_on_the_oracle_to_a_win_after_exactly_its_length(oracle, key):
    m = _m()
    for grp, (label, length, _) in zip(node_sets(key), mirror_labels(key, 12)):
        M = grp["M"]
        js, bs = np.nonzero(label == 1)
        kids = {(c[0], c[1]): c for c in children_on_the_oracle(oracle, grp)}
        deep = [(j, b) for j, b in zip(js, bs) if length[j, b] > 1]
        paths = {}
        if deep:
            got = m.placement_exact_nodes(np.array([kids[e][2] for e in deep]), np.array([kids[e][3] for e in deep]),
                                          np.array([kids[e][4] for e in deep]), np.array([grp["entry"][j] for j, _ in deep]),
                                          grp["pieces"], L5, M, CW, CAP)
            paths = {e: got[3][q] for q, e in enumerate(deep)}
        for j, b in zip(js, bs):
            moves, lst = int(grp["moves"][j]), grp["pieces"][grp["entry"][j]]
            g = oracle.Game(L5, M, rows=grp["rows"][j], pieces=lst[moves:], lines_cleared=int(grp["lines"][j]), moves_used=moves, state=0)
            for a in [int(b)] + [int(a) for a in paths.get((j, b), [])[:length[j, b] - 1]]:
                assert g.state == 0
                g.move(a // 10, a % 10)
            assert (g.state, g.moves_used) == (1, moves + length[j, b]), (key, j, b)


def test_no_proved_losing_move_of_the_exact_budget_set_has_a_win_on_the_oracle(oracle):
    """Two moves are left behind every move of this set, so the enumeration is 34 + 34^2 oracle moves a child at most."""
    checked = searched = 0
    for grp, (label, _, nodes) in zip(node_sets("back3"), mirror_labels("back3", 12)):
        for j, b, rows, lines, moves, _ in children_on_the_oracle(oracle, grp):
            if label[j, b] != 2 or moves != grp["moves"][j] + 1 or lines >= L5:
                continue                                       # a top-out made no move: nothing follows it
            lst = grp["pieces"][grp["entry"][j]]
            assert _first_winning_ply(oracle, L5 - lines, grp["M"] - moves, rows, lst[moves:]) == 0, (j, b)
            checked, searched = checked + 1, searched + int(nodes[j, b] > 0)
    assert searched == 81 and checked > searched               # the searched-out children and the dead ones


# ------------------------------------------------------------------------------------------------ 5. the cap
def test_a_cap_of_one_node_leaves_a_running_child_unproved_and_a_larger_cap_changes_no_proof():
    m = _m()
    opened = 0
    for grp, (label, length, nodes) in zip(node_sets("back3_spare1"), mirror_labels("back3_spare1", 12)):
        args = (grp["rows"], grp["lines"], grp["moves"], grp["entry"], grp["pieces"], L5, grp["M"], CW)
        runs = {cap: m.placement_exact_labels(*args, cap) for cap in (1, 8, 64)}
        runs[CAP] = (label, length, nodes)
        one = runs[1]
        searched = nodes > 0                                   # the child runs: its search expanded a node
        deeper = nodes > 1                                     # and needed a second one: no winning grandchild, and something left to search
        assert (one[0][deeper] == 3).all() and (one[1][deeper] == 0).all() and (one[2][searched] == 1).all()
        assert not ((one[0] == 2) & deeper).any()              # one node proves no loss where a second one was needed
        for x, y in zip(one, runs[CAP]):                       # a search of one node is not cut short by a cap of one
            assert np.array_equal(x[~deeper], y[~deeper])
        opened += int(deeper.sum())
        caps = sorted(runs)
        for lo, hi in zip(caps, caps[1:]):
            a, b = runs[lo], runs[hi]
            was = (a[0] == 1) | (a[0] == 2)
            for x, y in zip(a, b):
                assert np.array_equal(x[was], y[was]), (lo, hi)
            assert ((a[0] == 0) == (b[0] == 0)).all() and (b[2][b[0] == 3] == hi).all() and (b[2] <= hi).all()
    assert opened >= 32


# ------------------------------------------------------------------------------------------------ 6. edges, arguments, plumbing
def test_a_finished_node_is_proved_unsolved_without_a_node_and_has_no_labels():
    m = _m()
    grp = node_sets("back3")[1]
    k, M = grp["idx"].size, grp["M"]
    assert k >= 4
    lines, moves, entry = grp["lines"].copy(), grp["moves"].copy(), grp["entry"].astype(np.int64)
    lines[0], moves[1], entry[2] = L5, M, k
    got = m.placement_exact_nodes(grp["rows"], lines, moves, entry, grp["pieces"], L5, M, CW, CAP)
    ref = m.placement_exact_nodes(grp["rows"], grp["lines"], grp["moves"], grp["entry"], grp["pieces"], L5, M, CW, CAP)
    for x, y, dead in zip(got, ref, (0, 1, 0, 255, 0, 0)):
        assert (x[:3] == dead).all() and np.array_equal(x[3:], y[3:])
    label, length, nodes = m.placement_exact_labels(grp["rows"], lines, moves, entry, grp["pieces"], L5, M, CW, CAP)
    want = mirror_labels("back3", 12)[1]
    assert not label[:3].any() and not length[:3].any() and not nodes[:3].any()
    assert all(np.array_equal(x[3:], y[3:]) for x, y in zip((label, length, nodes), want))
    assert (m.best_labelled_move(label, length)[:3] == 255).all()
    # one move left: the label is the move's own verdict
    lines, moves = grp["lines"].copy(), np.full(k, M - 1, np.uint8)
    label, length, nodes = m.placement_exact_labels(grp["rows"], lines, moves, grp["entry"], grp["pieces"], L5, M, CW, 1)
    assert not (label == 3).any() and not nodes.any() and set(np.unique(length)) <= {0, 1}


def test_blunders_marks_a_proved_losing_move_taken_where_a_winning_one_was_proved():
    label = np.zeros((5, 40), np.uint8)
    label[0, [3, 4]] = 1, 2                                    # a win was there, the loss was taken
    label[1, [3, 4]] = 1, 3                                    # unproved is no proved blunder
    label[2, [3, 4]] = 2, 2                                    # nothing to throw away
    label[3, [3, 4]] = 1, 2                                    # the win was taken
    label[4, [3, 4]] = 1, 2                                    # an action the labels do not name
    action = np.array([4, 4, 4, 3, 255])
    assert T.blunders(label, action).tolist() == [1, 0, 0, 0, 0] and T.blunders(label, action).dtype == np.uint8
    torch = pytest.importorskip("torch")
    got = T.blunders(torch.from_numpy(label), torch.from_numpy(action))
    assert got.dtype == torch.uint8 and got.tolist() == [1, 0, 0, 0, 0]
    for bad in ((label[:, :39], action), (label, action[:4])):
        with pytest.raises(ValueError, match="label_before must be"):
            T.blunders(*bad)


def test_python_refusals_of_the_node_interface_and_of_the_mirrors_need_no_gpu():
    rows, pieces = np.zeros((4, 20), np.uint16), np.zeros((3, 7), np.uint8)
    z = np.zeros(4, np.uint8)
    ok = dict(rows=rows, lines=z, moves=z, entry=np.zeros(4, np.int64), pieces=pieces, L=2, M=6)
    for fn in (T.prove_nodes, T.label_moves):
        for L in (0, 251, 2.0, True, None):
            with pytest.raises(ValueError, match="L must"):
                fn(**dict(ok, L=L))
        for M in (0, 255, 6.0, True):
            with pytest.raises(ValueError, match="M must"):
                fn(**dict(ok, M=M))
        for bad in (0, (1 << 24) + 1, 1.5, True, None):
            with pytest.raises(ValueError, match="max_nodes"):
                fn(**ok, max_nodes=bad)
        for bad in (np.inf, np.nan, 1e39):
            with pytest.raises(ValueError, match="finite"):
                fn(**ok, spare_weight=bad)
        for weights in (np.zeros(11), np.zeros((2, 12)), "classical"):
            with pytest.raises(ValueError, match="weights"):
                fn(**ok, weights=weights)
        with pytest.raises(ValueError, match="rows must be"):
            fn(**dict(ok, rows=np.zeros((4, 19), np.uint16)))
        with pytest.raises(ValueError, match="at least one node"):
            fn(**dict(ok, rows=np.zeros((0, 20), np.uint16), lines=z[:0], moves=z[:0], entry=np.zeros(0, np.int64)))
        for p in (np.zeros((3, 5), np.uint8), np.zeros((0, 7), np.uint8), np.zeros(7, np.uint8)):
            with pytest.raises(ValueError, match="pieces must be"):
                fn(**dict(ok, pieces=p))
        for name in ("lines", "moves", "entry"):
            for bad in (z[:3], np.zeros(4, np.float32), np.zeros((4, 1), np.uint8)):
                with pytest.raises(ValueError, match=f"{name} must be 4 integers"):
                    fn(**dict(ok, **{name: bad}))
        for name in ("lines", "moves"):
            for bad in (np.array([0, 0, 0, 256]), np.array([0, -1, 0, 0])):
                with pytest.raises(ValueError, match=f"{name} must be in"):
                    fn(**dict(ok, **{name: bad}))
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="shortest must be"):
            T.prove_nodes(**ok, shortest=bad)
    p = inspect.signature(T.prove_nodes).parameters
    assert list(p) == ["rows", "lines", "moves", "entry", "pieces", "L", "M", "weights", "max_nodes", "shortest", "spare_weight", "device",
                       "validate"]
    assert (p["weights"].default, p["max_nodes"].default, p["shortest"].default, p["spare_weight"].default) == (None, 1 << 16, True, 0.0)
    p = inspect.signature(T.label_moves).parameters
    assert list(p) == ["rows", "lines", "moves", "entry", "pieces", "L", "M", "weights", "max_nodes", "spare_weight", "device", "validate"]
    assert (p["weights"].default, p["max_nodes"].default, p["spare_weight"].default) == (None, 1 << 12, 0.0)
    p = inspect.signature(T.label_states).parameters
    assert list(p) == ["env", "pieces", "weights", "max_nodes"] and (p["weights"].default, p["max_nodes"].default) == (None, 1 << 12)
    assert list(inspect.signature(T.blunders).parameters) == ["label_before", "action"]
    for name in ("prove_nodes", "label_moves", "label_states", "blunders"):
        assert getattr(T, name) is getattr(T.solve, name) and name in T.__all__ and name in T.solve.__all__
    assert "NOTHING is proved" in T.prove_nodes.__doc__ and "(L - lines[i], M - moves[i])" in T.prove_nodes.__doc__
    assert "Label 3 proves nothing" in T.label_moves.__doc__ and "Label 3 proves nothing" in T.label_states.__doc__

    class NoPool:
        L, M = 2, 6

        def pool_info(self):
            return dict(n_configs=0)

    class Pool(NoPool):
        def pool_info(self):
            return dict(n_configs=3)

    with pytest.raises(ValueError, match="needs an environment with a configuration pool"):
        T.label_states(NoPool(), pieces)
    for bad in (np.zeros((4, 7), np.uint8), np.zeros((3, 6), np.uint8), [[0] * 7] * 3):
        with pytest.raises(ValueError, match="pieces must be the loaded pool's lists"):
            T.label_states(Pool(), bad)
    # the mirrors
    m = _m()
    good = dict(rows=rows, lines=z, moves=z, entry=z, pieces=pieces, L=2, M=6, weights=CW, max_nodes=4)
    for fn in (m.placement_exact_nodes, m.placement_exact_labels):
        for bad in (dict(L=0), dict(M=255), dict(max_nodes=0), dict(max_nodes=True), dict(max_nodes=2.0), dict(spare_weight=np.inf),
                    dict(weights=np.zeros(13)), dict(pieces=pieces[:, :6]), dict(pieces=pieces[:0]), dict(lines=z[:3]),
                    dict(moves=np.zeros(4)), dict(entry=np.full(4, -1)), dict(lines=np.full(4, 256))):
            with pytest.raises(ValueError):
                fn(**{**good, **bad})
    with pytest.raises(ValueError):
        m.placement_exact_nodes(**good, shortest=1)
    assert list(inspect.signature(m.placement_exact_nodes).parameters) == ["rows", "lines", "moves", "entry", "pieces", "L", "M", "weights",
                                                                         "max_nodes", "shortest", "spare_weight"]
    assert list(inspect.signature(m.placement_exact_labels).parameters) == ["rows", "lines", "moves", "entry", "pieces", "L", "M", "weights",
                                                                          "max_nodes", "spare_weight"]
    assert (m.LABEL_NONE, m.LABEL_WIN, m.LABEL_LOSS, m.LABEL_OPEN) == (0, 1, 2, 3)


NODES = ("tpl_placement_exact_nodes", "tpl_placement_exact_nodes_move")
LABELS = ("tpl_placement_exact_labels", "tpl_placement_exact_labels_move")
KERNELS = ("placement_exact_nodes_kernel", "placement_exact_nodes_move_kernel", "placement_exact_labels_kernel",
           "placement_exact_labels_move_kernel")
HEAD = ["rows", "lines", "moves", "entry", "pieces", "n", "n_cfg", "L", "M", "weights", "spare_weight", "max_nodes"]
NODES_ARGS = HEAD + ["shortest", "solved", "proved", "solution_len", "actions", "bound", "nodes", "stream"]
LABELS_ARGS = HEAD + ["label", "length", "nodes", "stream"]


def test_every_refusal_of_the_four_entries_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    head = [fake, fake, fake, fake, fake, 4, 3, 2, 6, fake, 0.25, 100]
    for names, args, ok in ((NODES, NODES_ARGS, head + [1] + [fake] * 6 + [None]), (LABELS, LABELS_ARGS, head + [fake] * 3 + [None])):
        assert len(ok) == len(args)
        pointers = [a for a in args if a not in ("n", "n_cfg", "L", "M", "spare_weight", "max_nodes", "shortest", "stream")]
        cases = [(args.index(a), None, "null") for a in pointers]
        per_node = 1 if names is NODES else 40
        cases += [(5, 0, "positive"), (5, -3, "positive"), (5, -(-(1 << 31) // per_node), "2^31"), (5, 1 << 40, "2^31"),
                  (6, 0, "n_cfg must be in [1, 2^31)"), (6, -1, "n_cfg must be in"), (6, 1 << 31, "n_cfg must be in"),
                  (7, 0, "L and M"), (7, 251, "L and M"), (8, 0, "L and M"), (8, 255, "L and M"),
                  (0, fake + 1, "rows must be 2-byte"), (3, fake + 2, "entry must be 4-byte"), (9, fake + 4, "weights must be 16-byte"),
                  (10, float("inf"), "spare_weight must be finite"), (10, float("nan"), "spare_weight must be finite"),
                  (11, 0, "max_nodes must be in [1, 16777216]"), (11, (1 << 24) + 1, "max_nodes must be in"),
                  (args.index("nodes"), fake + 2, "nodes must be 4-byte")]
        if names is NODES:
            cases += [(12, 2, "shortest must be 0 or 1"), (12, -1, "shortest must be 0 or 1"),
                      (args.index("solution_len"), fake + 2, "solution_len must be 4-byte"), (args.index("bound"), fake + 2, "bound must be 4-byte")]
        else:
            cases += [(args.index("length"), fake + 2, "length must be 4-byte")]
        for name in names:
            fn = getattr(lib, name)
            for at, value, what in cases:
                call = list(ok)
                call[at] = value
                assert fn(*call) < 0 and name + ":" in err() and what in err(), (name, args[at], value, err())
            # the largest arguments are not refused for their size: a check that comes after them speaks
            call = list(ok)
            call[5], call[6], call[7], call[8], call[11], call[0] = -(-(1 << 31) // per_node) - 1, (1 << 31) - 1, 250, 254, 1 << 24, fake + 1
            assert fn(*call) < 0 and "rows must be 2-byte" in err()


def test_the_header_states_both_rules_and_the_library_exports_the_four_entries():
    m = _m()
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_\w+)\s*\(", text))
    assert declared == set(m.LEARN_SYMBOLS) and set(NODES + LABELS) <= declared
    lib = ctypes.CDLL(m.build_library())
    for names, args in ((NODES, NODES_ARGS), (LABELS, LABELS_ARGS)):
        for name in names:
            assert hasattr(lib, name), name
            proto = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S).group(1)
            assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == args, name
    for k, name in enumerate(("NONE", "WIN", "LOSS", "OPEN")):
        assert f"#define TPL_LABEL_{name} {k}\n" in raw
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("THE SHIFTED GAME", "the game (L - lines, M - moves)", "pieces[entry][moves + d] & 7",
                  "BYTE FOR BYTE, WHAT tpl_placement_exact WRITES FOR THE SHIFTED CONFIGURATION", "COUNTED FROM THE NODE",
                  "THE KERNEL TREATS IT AS FINISHED", "no index ever falls outside pieces", "LABEL 3 PROVES NOTHING", "PROVED WINNING",
                  "PROVED LOSING", "tpl_placement_exact_nodes applied to its children", "WITH proved = 0 NOTHING IS PROVED"):
        assert words in flat, words
    # the body is shared between the two forms, not copied, and the existing units are not part of it
    here = os.path.dirname(m._UNITS[0])
    units = [os.path.basename(p) for p in m._UNITS]
    assert "exact_nodes.hip" in units and "exact_nodes_move.hip" in units
    code = [l for l in open(os.path.join(here, "exact_nodes_move.hip")).read().splitlines() if l.strip() and not l.startswith("//")]
    assert code == ["#define TPL_PLACEMENT_MOVE_UNIT", "#define TPL_PLACEMENT_BOUND_UNIT", '#include "exact_nodes.hip"']
    body = open(os.path.join(here, "exact_nodes.hip")).read()
    assert "__syncthreads" not in body and '#include "exact.hip"' not in body and '#include "tpl_beam.h"' in body
    for doc in ("README.md", "DESIGN.md"):
        words = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "prove_nodes" in words and "label_moves" in words and "(L - lines, M - moves)" in words and "proves nothing" in words, doc


def test_the_node_kernels_use_no_scratch_and_fill_a_simd_with_waves():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    num = lambda r, what: int(r[r.index(what) - 1])
    for kernel in KERNELS:
        mine = [r for r in rows if f"{len(kernel)}{kernel}E" in r[-1]]       # the whole mangled name: no name within another
        assert len(mine) == 1, (kernel, [r[-1] for r in rows])
        r = mine[0]
        assert num(r, "scratch") == 0, r
        assert num(r, "vgpr") <= 64, r                                       # eight waves a SIMD by the vector registers
        static = num(r, "lds")
        assert static + 80 * 254 <= 64 * 1024, r                             # the deepest stack is launchable without an attribute
        assert 32 * (static + 80 * 40) <= 160 * 1024, r                      # M = 40: the 32 waves of a CU each have their stack
