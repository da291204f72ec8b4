"""CPU-side checks of the ranking update from proved move labels (include/tpl_learn.h's rule under tpl_ntuple_rank;
_learn_lib.ntuple_rank, ntuple_rank_step, ntuple_rank_fit; ntuple.py's NTupleRanker; csrc/learn/ntuple_rank.hip).  No GPU.

THE NODES (rank_nodes below; the GPU tests use the same): the 96 nodes of test_exact_nodes_cpu's three node sets -- the boards 3 and 4
moves before the end of the recorded solutions of the first 32 configurations of tests/golden/carved_L5_M20.npz --, each SHIFTED INTO
ONE GAME (5, 10): a node at move k of the game (5, M_g) is the node at move k + 10 - M_g of the game (5, 10) with its list moved up by
as much, which has the same moves left, the same pieces ahead and so the same labels.  They are labelled by
_learn_lib.placement_exact_labels at a cap of 256 nodes a child, which proves every child here.

  1. the nodes: the shift keeps the labels of the native games; every node is decided;
  2. the mirror on the nodes: greedy is the act rule's choice from an independent fold; with every distinct placement labelled 1 but
     one labelled 2, win is the best of the rest; the children are the C oracle's moves;
  3. hand-made rows: the zero table, empty W, empty X, a finished board, a won win child, a lost loss child, garbage bytes, the prune;
  4. ntuple_rank_step adds exactly +- rint(rate) on the two afterstates' entries and nothing elsewhere;
  5. fit from the zero table: fewer violations, more greedy moves labelled 1;
  6. the entry's refusals as statuses, the header, the four kernels' resources against their act twins, and the host code under
     ASan + UBSan in a stand-alone program (tests/c_abi/sanitize_ntuple_rank.cpp).
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
from test_exact_nodes_cpu import COUNT, L5, SETS, mirror_labels, node_sets
from test_solve_cpu import CW, Node, _placements

import tetris_piclim as T

M10, LABEL_CAP = 10, 256
REWARD, GAMMA = (1.0, 10.0, -1.0), 0.99
FIT = dict(epochs=4, batch=16, seed=3, rate=8.0)               # chosen on the CPU (test 5's docstring has the counts)
FIT_REWARD = (0.0, 0.0, 0.0)                                   # the table alone ranks: under the zero table every score ties


def _m():
    return T._learn_lib


def _labelled(rows, lines, moves, lists, native):
    """Nodes of the game (5, 10), each with its own list (entry = arange), labelled at LABEL_CAP; read-only arrays."""
    m = _m()
    rows, lines, moves, lists = np.array(rows, np.uint16), np.array(lines, np.int64), np.array(moves, np.int64), np.array(lists, np.uint8)
    n = rows.shape[0]
    label, _, _ = m.placement_exact_labels(rows, lines, moves, np.arange(n, dtype=np.uint32), lists, L5, M10, CW, LABEL_CAP)
    piece = np.stack([lists[np.arange(n), moves], lists[np.arange(n), moves + 1]], axis=1).astype(np.int64)
    out = dict(rows=rows, lines=lines, moves=moves, state=np.zeros(n, np.int64), piece=piece, pieces=lists, label=label, native=native)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rank_nodes():
    """The 96 nodes in the game (5, 10): rows uint16 [96, 20], lines, moves, state int64 [96], piece int64 [96, 2] (the falling piece and
    the next), pieces uint8 [96, 11] (each node's own list, entry = arange), label uint8 [96, 40], and `native`: (set, group, index)."""
    rows, lines, moves, lists, native = [], [], [], [], []
    for key in SETS:
        for q, grp in enumerate(node_sets(key)):
            shift = M10 - grp["M"]
            assert shift >= 0
            for j in range(grp["idx"].size):
                lst = np.zeros(M10 + 1, np.uint8)
                lst[shift:] = grp["pieces"][grp["entry"][j]]
                rows.append(grp["rows"][j]); lines.append(int(grp["lines"][j])); moves.append(int(grp["moves"][j]) + shift)
                lists.append(lst); native.append((key, q, j))
    return _labelled(rows, lines, moves, lists, native)


@functools.lru_cache(maxsize=None)
def end_nodes():
    """32 more nodes of the game (5, 10): the boards ONE move before the end of the same 32 recorded solutions.  The even ones have
    one move to spare (move 8): the recorded move wins at once, any other leaves a running board with one move left.  The odd ones
    have none (move 9): any other move ends the game lost at the limit."""
    g = load_golden("carved_L5_M20.npz")
    rows, lines, moves, lists, native = [], [], [], [], []
    for i in range(COUNT):
        k = int(g["sol_len"][i]) - 1
        spare = 1 - i % 2
        shift = M10 - (k + 1 + spare)
        assert k >= 1 and shift >= 0 and g["r_moves"][i, k - 1] == k and g["r_state"][i, k - 1] == 0
        lst = np.zeros(M10 + 1, np.uint8)
        lst[shift:] = g["pieces"][i, :k + 2 + spare]
        rows.append(g["r_rows"][i, k - 1]); lines.append(int(g["r_lines"][i, k - 1])); moves.append(k + shift)
        lists.append(lst); native.append(("end", 0, i))
    return _labelled(rows, lines, moves, lists, native)


@functools.lru_cache(maxsize=None)
def all_nodes():
    """rank_nodes and end_nodes in one set of 128."""
    a, b = rank_nodes(), end_nodes()
    out = {k: (a[k] + b[k] if k == "native" else np.concatenate([a[k], b[k]])) for k in a}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def rank_args(nodes, pick=slice(None)):
    """The state arguments of ntuple_rank for the nodes `pick`: (rows, piece, L, M, lines, moves, state)."""
    return nodes["rows"][pick], nodes["piece"][pick], L5, M10, nodes["lines"][pick], nodes["moves"][pick], nodes["state"][pick]


def small_table(form, seed, span=1 << 14):
    """Random small integers, so that scores tie now and then."""
    return np.random.default_rng(seed).integers(-span, span + 1, _m().ntuple_entries_of(form)).astype(np.int32)


def distinct_of(piece):
    acts = np.arange(40)
    return _m().canonical_actions(np.asarray(piece)[:, None], acts[None, :]) == acts[None, :]


# ------------------------------------------------------------------------------------------------ 1. the nodes
def test_the_shift_into_one_game_keeps_the_labels_and_every_node_is_decided():
    nodes = rank_nodes()
    assert nodes["label"].shape == (96, 40) and nodes["moves"].max() == M10 - 3 and nodes["moves"].min() >= 1
    for i, (key, q, j) in enumerate(nodes["native"]):
        if key == "back3_spare1":                              # the cached native labels of one set, at its own cap
            assert np.array_equal(nodes["label"][i], mirror_labels(key, 12, LABEL_CAP)[q][0][j]), (key, q, j)
    lab = nodes["label"]
    assert not (lab == 3).any() and set(np.unique(lab).tolist()) == {0, 1, 2}
    assert ((lab == 1).any(axis=1) & (lab == 2).any(axis=1)).all()
    assert ((lab != 0) == distinct_of(nodes["piece"][:, 0])).all()
    assert ((lab == 1).sum(axis=1) > 1).sum() >= 10            # several winning moves to choose among


# ------------------------------------------------------------------------------------------------ 2. the mirror on the nodes
def _scores(table, nodes, prune=False):
    """score [K, 40] of the act rule from an independent fold: every action moved on its own, the reward and V folded here."""
    m = _m()
    rows, piece, L, M, lines, moves, state = rank_args(nodes)
    k = rows.shape[0]
    a = np.tile(np.arange(40), k)
    node = np.repeat(np.arange(k), 40)
    r2, cleared, l2, m2, s2 = m.host_moves(rows[node], piece[node, 0], a // 10, a % 10, L, M, lines[node], moves[node])
    if prune:
        s2 = np.where(m.move_bound(r2, L, M, l2, m2, s2)["dead"], 2, s2)
    r = np.float32(REWARD[0]) * cleared.astype(np.float32)
    r = np.where(s2 == 1, r + np.float32(REWARD[1]), r)
    r = np.where(s2 >= 2, r + np.float32(REWARD[2]), r).astype(np.float32)
    v = m.ntuple_value(table, r2, piece[node, 1], L, M, l2, m2, s2)
    return np.where(s2 == 0, r + np.float32(GAMMA) * v, r).astype(np.float32).reshape(k, 40), s2.reshape(k, 40)


@pytest.mark.parametrize("form", ["2x4", "3x3", "feat", "feat+spare"])
def test_greedy_is_the_act_rules_choice_and_win_and_loss_are_the_best_of_their_sets(form):
    m, nodes = _m(), rank_nodes()
    table = small_table(form, 11)
    out = m.ntuple_rank(table, *rank_args(nodes), nodes["label"], GAMMA, REWARD, 0.0, False)
    assert list(out) == list(m.RANK_OUTPUTS)
    assert [out[k].dtype for k in m.RANK_OUTPUTS[:7]] == [np.uint8] * 4 + [np.float32] * 3
    score, _ = _scores(table, nodes)
    distinct = distinct_of(nodes["piece"][:, 0])
    best = lambda mask: np.argmax(np.where(mask, score, -np.inf) == np.where(mask, score, -np.inf).max(axis=1, keepdims=True), axis=1)
    assert np.array_equal(out["greedy"], best(distinct))
    assert np.array_equal(out["win"], best(nodes["label"] == 1)) and np.array_equal(out["loss"], best(nodes["label"] == 2))
    at = np.arange(96)
    assert np.array_equal(out["gap"].view(np.uint32), (score[at, out["win"]] - score[at, out["loss"]]).astype(np.float32).view(np.uint32))
    assert np.array_equal(out["violated"], (out["gap"] <= 0).astype(np.uint8)) and 0 < out["violated"].sum() < 96
    # every distinct placement labelled 1 but one labelled 2: win is the best of the rest, loss the one
    for loser in ("greedy", "lowest"):
        the_one = out["greedy"].astype(np.int64) if loser == "greedy" else np.argmax(distinct, axis=1)
        lab = distinct.astype(np.uint8)
        lab[at, the_one] = 2
        o = m.ntuple_rank(table, *rank_args(nodes), lab, GAMMA, REWARD, 0.0, False)
        rest = distinct.copy()
        rest[at, the_one] = False
        assert np.array_equal(o["loss"], the_one) and np.array_equal(o["win"], best(rest)) and np.array_equal(o["greedy"], out["greedy"])
        if loser == "greedy":                                  # the table's own choice is the loss: nothing beats it
            assert (o["gap"] <= 0).all() and o["violated"].all()


def test_the_afterstates_are_the_c_oracles_children(oracle):
    m, nodes = _m(), rank_nodes()
    out = m.ntuple_rank(small_table("feat+spare", 5), *rank_args(nodes), nodes["label"], GAMMA, REWARD, 0.0, True)
    for i in range(96):
        lst, moves = nodes["pieces"][i], int(nodes["moves"][i])
        node = Node(oracle, L5, M10, nodes["rows"][i], lst, int(nodes["lines"][i]), moves, 0, moves)
        assert out["win"][i] in _placements(lst[moves]) and out["loss"][i] in _placements(lst[moves])
        for side in ("win", "loss"):
            c = node.child(int(out[side][i])).g
            assert np.array_equal(out[side + "_rows"][i], np.asarray(c.rows, np.uint16)), (i, side)
            assert out[side + "_fields"][i].tolist() == [c.lines_cleared, c.moves_used, c.state], (i, side)


# ------------------------------------------------------------------------------------------------ 3. hand-made rows
def _zero(form="feat+spare"):
    return np.zeros(_m().ntuple_entries_of(form), np.int32)


def test_under_the_zero_table_every_score_ties_and_every_decided_node_teaches():
    m, nodes = _m(), rank_nodes()
    out = m.ntuple_rank(_zero(), *rank_args(nodes), nodes["label"], GAMMA, (0.0, 0.0, 0.0), 0.0, False)
    lab = nodes["label"]
    assert np.array_equal(out["win"], np.argmax(lab == 1, axis=1)) and np.array_equal(out["loss"], np.argmax(lab == 2, axis=1))
    assert np.array_equal(out["greedy"], np.argmax(lab != 0, axis=1))
    assert (out["gap"].view(np.uint32) == 0).all() and out["violated"].all()
    # a positive margin is violated too, a negative one is not
    assert m.ntuple_rank(_zero(), *rank_args(nodes), lab, GAMMA, (0.0, 0.0, 0.0), 0.5, False)["violated"].all()
    assert not m.ntuple_rank(_zero(), *rank_args(nodes), lab, GAMMA, (0.0, 0.0, 0.0), -0.5, False)["violated"].any()


def test_undecided_nodes_and_garbage_label_bytes():
    m, nodes = _m(), rank_nodes()
    pick = np.arange(12)
    rows, piece, L, M, lines, moves, state = rank_args(nodes, pick)
    lab = nodes["label"][pick].copy()
    table = small_table("feat", 7)
    base = m.ntuple_rank(table, rows, piece, L, M, lines, moves, state, lab, GAMMA, REWARD, 0.0, False)
    case = lab.copy()
    case[0][case[0] == 1] = 3                                  # empty W: label 3 proves nothing
    case[1][case[1] == 2] = 0                                  # empty X
    case[2] = 0                                                # no label at all
    st = state.copy()
    st[3:6] = (1, 2, 3)                                        # finished boards, their rows fully labelled
    out = m.ntuple_rank(table, rows, piece, L, M, lines, moves, st, case, GAMMA, REWARD, 0.0, False)
    und = np.arange(6)
    assert (out["win"][und] == 255).all() and (out["loss"][und] == 255).all() and (out["violated"][und] == 0).all()
    for k in ("gap", "err_win", "err_loss"):
        assert (out[k][und].view(np.uint32) == 0).all(), k
    for side in ("win", "loss"):                               # both afterstates are the state itself
        assert np.array_equal(out[side + "_rows"][und], rows[und])
        assert np.array_equal(out[side + "_fields"][und], np.stack([lines, moves, st], axis=1)[und])
    assert np.array_equal(out["greedy"][:3], base["greedy"][:3]) and (out["greedy"][3:6] == 0).all()
    for k in m.RANK_OUTPUTS:                                   # the other nodes do not notice
        assert np.array_equal(out[k][6:], base[k][6:]), k
    # garbage: bytes 4..255 anywhere, and labels 1 and 2 on the aliases, change nothing
    gen = np.random.default_rng(1)
    distinct = distinct_of(piece[:, 0])
    noisy = lab.copy()
    junk = gen.integers(4, 256, lab.shape).astype(np.uint8)
    hit = gen.random(lab.shape) < 0.3
    noisy[hit & (lab != 1) & (lab != 2)] = junk[hit & (lab != 1) & (lab != 2)]
    noisy[~distinct] = gen.integers(1, 3, (~distinct).sum()).astype(np.uint8)
    assert (noisy != lab).sum() > 50
    got = m.ntuple_rank(table, rows, piece, L, M, lines, moves, state, noisy, GAMMA, REWARD, 0.0, False)
    for k in m.RANK_OUTPUTS:
        assert np.array_equal(got[k], base[k]), k


def test_a_side_that_ends_the_game_teaches_nothing_and_the_prune_ends_a_dead_child():
    m, nodes = _m(), all_nodes()
    table = small_table("feat+spare", 9)
    args = rank_args(nodes)
    _, s2 = _scores(table, nodes)
    _, s2p = _scores(table, nodes, prune=True)
    distinct = distinct_of(nodes["piece"][:, 0])
    at = np.arange(128)
    won, lost, runs = distinct & (s2 == 1), distinct & (s2 >= 2), distinct & (s2 == 0)
    dead = distinct & (s2 == 0) & (s2p == 2)
    # a won win child against a running loss child: the node is violated by a huge margin, and only the loss is taught
    pick = np.flatnonzero(won.any(axis=1) & runs.any(axis=1))
    assert pick.size >= 8
    lab = np.zeros((128, 40), np.uint8)
    lab[pick, np.argmax(won, axis=1)[pick]] = 1
    lab[pick, np.argmax(runs, axis=1)[pick]] = 2
    out = m.ntuple_rank(table, *args, lab, GAMMA, REWARD, 1e6, False)
    assert out["violated"][pick].all() and (out["err_win"][pick] == 0).all() and (out["err_loss"][pick] == -1).all()
    assert (out["win_fields"][pick, 2] == 1).all() and (out["loss_fields"][pick, 2] == 0).all()
    assert (out["win"] == 255)[np.setdiff1d(at, pick)].all()
    # a lost loss child (here beside a won win child: at the last move nothing runs): neither side has a value to move, and the node
    # is still reported -- violated under a margin nothing reaches, not violated at margin 0, where the win's reward leads
    pick = np.flatnonzero(lost.any(axis=1) & won.any(axis=1))
    assert pick.size >= 8
    lab = np.zeros((128, 40), np.uint8)
    lab[pick, np.argmax(won, axis=1)[pick]] = 1
    lab[pick, np.argmax(lost, axis=1)[pick]] = 2
    out = m.ntuple_rank(table, *args, lab, GAMMA, REWARD, 1e6, False)
    assert out["violated"][pick].all() and (out["err_win"][pick] == 0).all() and (out["err_loss"][pick] == 0).all()
    assert (out["loss_fields"][pick, 2] >= 2).all() and (out["win_fields"][pick, 2] == 1).all()
    out = m.ntuple_rank(table, *args, lab, GAMMA, REWARD, 0.0, False)
    assert not out["violated"][pick].any() and (out["gap"][pick] > 0).all()
    # the prune: a dead running loss child is scored as lost at the limit -- r_lose and no gamma V -- and teaches nothing, while its
    # afterstate stays the true, running board
    pick = np.flatnonzero(dead.any(axis=1) & (runs & ~dead).any(axis=1))
    assert pick.size >= 8
    lab = np.zeros((128, 40), np.uint8)
    b_dead, b_live = np.argmax(dead, axis=1), np.argmax(runs & ~dead, axis=1)
    lab[pick, b_live[pick]] = 1
    lab[pick, b_dead[pick]] = 2
    off = m.ntuple_rank(table, *args, lab, GAMMA, REWARD, 1e6, False)
    on = m.ntuple_rank(table, *args, lab, GAMMA, REWARD, 1e6, True)
    assert (off["err_loss"][pick] == -1).all() and (on["err_loss"][pick] == 0).all() and (on["err_win"][pick] == 1).all()
    for k in ("win", "loss", "win_rows", "loss_rows", "win_fields", "loss_fields"):
        assert np.array_equal(on[k], off[k]), k
    assert (on["loss_fields"][pick, 2] == 0).all()
    score_on, _ = _scores(table, nodes, prune=True)
    assert np.array_equal(on["gap"][pick].view(np.uint32),
                          (score_on[pick, b_live[pick]] - score_on[pick, b_dead[pick]]).astype(np.float32).view(np.uint32))
    assert not np.array_equal(on["gap"][pick], off["gap"][pick])
    with pytest.raises(ValueError, match="prune"):
        m.ntuple_rank(small_table("feat", 1), *args, lab, GAMMA, REWARD, 0.0, True)


# ------------------------------------------------------------------------------------------------ 4. one step
@pytest.mark.parametrize("form,symmetric", [("2x4", False), ("3x3", True), ("feat", False), ("feat+spare", True)])
def test_a_step_adds_the_rounded_rate_on_the_two_afterstates_entries_and_nothing_elsewhere(form, symmetric):
    m, nodes = _m(), rank_nodes()
    pick = np.arange(0, 96, 4)
    args = rank_args(nodes, pick)
    L, M = args[2], args[3]
    start = small_table(form, 21)
    table = start.copy()
    rate = 37.4
    out = m.ntuple_rank_step(table, *args, nodes["label"][pick], GAMMA, REWARD, 0.0, form == "feat+spare", rate, symmetric)
    before = m.ntuple_rank(start, *args, nodes["label"][pick], GAMMA, REWARD, 0.0, form == "feat+spare")
    for k in m.RANK_OUTPUTS:                                   # the step reports the table before the adds
        assert np.array_equal(out[k], before[k]), k
    want = start.astype(np.int64)
    nxt = nodes["piece"][pick, 1]
    touched = 0
    for side, sign in (("win", 37), ("loss", -37)):
        f = out[side + "_fields"]
        index, used = m.ntuple_indices(out[side + "_rows"], nxt, L, M, f[:, 0], f[:, 1], form)
        taught = out["err_" + side] != 0
        assert np.array_equal(taught, (out["violated"] == 1) & (f[:, 2] == 0) if form != "feat+spare" else taught)
        np.add.at(want, index[used & taught[:, None]], sign)
        touched += int(taught.sum())
        if symmetric:
            mi, mu = m.ntuple_indices(m._reflected_rows(out[side + "_rows"]), np.array(m.PIECE_MIRROR)[nxt], L, M, f[:, 0], f[:, 1], form)
            mu = mu.copy()
            mu[:, m._counter_columns(form)] = False
            np.add.at(want, mi[mu & taught[:, None]], sign)
    assert touched >= 4 and np.array_equal(table.astype(np.int64), want) and not np.array_equal(table, start)


# ------------------------------------------------------------------------------------------------ 5. fit
def agreement(table, nodes, prune=True):
    """(violated, greedy labelled 1) over the nodes, all of which are decided."""
    out = _m().ntuple_rank(table, *rank_args(nodes), nodes["label"], GAMMA, FIT_REWARD, 0.0, prune)
    return int(out["violated"].sum()), int((nodes["label"][np.arange(96), out["greedy"]] == 1).sum())


@functools.lru_cache(maxsize=None)
def fitted():
    """The mirror of NTupleRanker.fit on the 96 nodes from the zero "feat+spare" table: (table, per-epoch violated counts)."""
    nodes = rank_nodes()
    table = _zero()
    counts = _m().ntuple_rank_fit(table, *rank_args(nodes), nodes["label"], GAMMA, FIT_REWARD, 0.0, True, FIT["rate"], False, FIT["epochs"],
                                  FIT["batch"], FIT["seed"])
    table.setflags(write=False)
    return table, counts


FIT_COUNTS = ((96, 5), [36, 6, 2, 2], (1, 95))                 # (violated, greedy labelled 1) before; violated per epoch; after


def test_fit_from_the_zero_table_lowers_the_violations_and_raises_the_agreement():
    """On the 96 nodes, all decided, from the zero "feat+spare" table with reward (0, 0, 0), gamma 0.99, margin 0, the prune on, rate 8,
    16 nodes a step, 4 epochs, seed 3, the mirror finds:
        before    96 nodes violated (every decided node: every score ties),  5 greedy moves labelled 1 (the lowest placement)
        epochs    36, 6, 2, 2 violated, each node counted when its minibatch was ranked
        after      1 node violated, 95 greedy moves labelled 1
    The GPU test holds NTupleRanker.fit to the same per-epoch counts."""
    nodes = rank_nodes()
    before = agreement(_zero(), nodes)
    table, counts = fitted()
    after = agreement(table, nodes)
    print("violated, greedy labelled 1: before", before, "per epoch", counts, "after", after)
    assert before[0] == 96                                     # every decided node, because every score ties
    assert len(counts) == FIT["epochs"] and all(0 <= c <= 96 for c in counts)
    assert after[0] < before[0]                                # strictly fewer violated nodes
    assert after[1] > before[1]                                # strictly more greedy moves that are proved wins
    assert (before, counts, after) == FIT_COUNTS


# ------------------------------------------------------------------------------------------------ 6. arguments and plumbing
ENTRY = "tpl_ntuple_rank"
KERNELS = {"ntuple_rank_kernel": "ntuple_act_kernel", "ntuple_rank3_kernel": "ntuple3_act_kernel",
           "ntuple_rank_feature_kernel": "ntuple_feature_act_kernel", "ntuple_rank_budget_kernel": "ntuple_budget_act_kernel"}
ARGS = ["plane_a", "plane_b", "n", "L", "M", "table", "entries", "label", "r_line", "r_win", "r_lose", "gamma", "margin", "prune", "win",
        "loss", "greedy", "violated", "gap", "err_win", "err_loss", "win_a", "win_b", "loss_a", "loss_b", "stream"]


def test_every_refusal_of_the_entry_comes_back_as_a_status_without_a_gpu():
    m = _m()
    lib = m.lib()
    fn = lib.tpl_ntuple_rank
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    counts = [m.ntuple_entries_of(form) for form in m.NTUPLE_RANK_FORMS]
    at = ARGS.index
    for entries in counts:
        ok = [fake, fake, 4, 5, 10, fake, entries, fake, 1.0, 10.0, -1.0, 0.99, 0.0, 0] + [fake] * 11 + [None]
        assert len(ok) == len(ARGS)
        cases = [(at(a), None, "null") for a in ("plane_a", "plane_b", "table", "label")]
        cases += [(at(a), None, "every output is required") for a in ARGS[14:25]]
        cases += [(2, 0, "positive"), (2, -3, "positive"), (2, (1 << 31) // 40 + 1, "40 n"), (2, 1 << 40, "40 n"), (3, 0, "L and M"),
                  (3, 251, "L and M"), (4, 0, "L and M"), (4, 255, "L and M"), (0, fake + 8, "planes must be 16-byte"),
                  (1, fake + 4, "planes must be 16-byte"), (5, fake + 4, "table must be 16-byte")]
        cases += [(at(a), fake + 8, "must be 16-byte aligned") for a in ("win_a", "win_b", "loss_a", "loss_b")]
        cases += [(at(a), fake + 2, "must be 4-byte aligned") for a in ("gap", "err_win", "err_loss")]
        for bad in (float("inf"), float("-inf"), float("nan")):
            cases += [(at("margin"), bad, "margin must be finite"), (at("gamma"), bad, "gamma must be finite")]
            cases += [(at(a), bad, "r_line, r_win and r_lose must be finite") for a in ("r_line", "r_win", "r_lose")]
        cases += [(at("prune"), 2, "prune must be 0 or 1"), (at("prune"), -1, "prune must be 0 or 1")]
        if entries != m.NTUPLE_ENTRIES_BUDGET:
            cases.append((at("prune"), 1, "budget table"))
        for where, value, what in cases:
            args = list(ok)
            args[where] = value
            assert fn(*args) < 0 and err().startswith(ENTRY + ":") and what in err(), (ARGS[where], value, err())
    # any other entry count is refused, first, with the four forms named: a sum table, a 3x3 + feature table, the staged tables
    others = [0, -1, 1, m.NTUPLE_ENTRIES_SUM, m.NTUPLE_ENTRIES_3X3_FEAT, 21505, 1 << 40] + \
        [m.ntuple_staged_entries_of(s) for s in ("2x4", "3x3", "2x4+3x3")]
    for entries in others:
        for args in ([fake, fake, 4, 5, 10, fake, entries, fake, 1.0, 10.0, -1.0, 0.99, 0.0, 0] + [fake] * 11 + [None],
                     [None, None, 0, 0, 0, None, entries, None, 1.0, 0.0, 0.0, float("nan"), float("nan"), 7] + [None] * 12):
            assert fn(*args) < 0 and ENTRY + ": entries must be" in err(), (entries, err())
            assert all(f'"{form}"' in err() for form in m.NTUPLE_RANK_FORMS) and all(str(c) in err() for c in counts), err()


def test_the_mirrors_refusals_and_the_python_surface():
    import torch
    m, nodes = _m(), rank_nodes()
    pick = np.arange(4)
    good = dict(zip(("rows", "piece", "L", "M", "lines", "moves", "state"), rank_args(nodes, pick)))
    good.update(table=_zero(), label=nodes["label"][pick], gamma=GAMMA, reward=REWARD, margin=0.0, prune=False)
    assert list(inspect.signature(m.ntuple_rank).parameters) == ["table", "rows", "piece", "L", "M", "lines", "moves", "state", "label",
                                                                  "gamma", "reward", "margin", "prune"]
    for bad in (dict(table=np.zeros(m.NTUPLE_ENTRIES_SUM, np.int32)), dict(table=np.zeros(m.ntuple_staged_entries_of("3x3"), np.int32)),
                dict(table=np.zeros(21504, np.int64)), dict(L=0), dict(M=255), dict(gamma=np.inf), dict(margin=np.nan), dict(margin=None),
                dict(reward=(1.0, 0.0)), dict(reward=(1.0, np.nan, 0.0)), dict(prune=1), dict(label=nodes["label"][pick].astype(np.int32)),
                dict(label=nodes["label"][:3]), dict(piece=nodes["piece"][pick, 0]), dict(table=_zero("feat"), prune=True)):
        with pytest.raises(ValueError):
            m.ntuple_rank(**{**good, **bad})
    with pytest.raises(ValueError, match="four plain forms"):
        m.ntuple_rank(**dict(good, table=np.zeros(m.NTUPLE_ENTRIES_SUM, np.int32)))
    # the order of a fit is a function of (count, epochs, seed): a permutation an epoch
    order = m.rank_fit_order(96, 3, 5)
    assert order.shape == (3, 96) and order.dtype == np.int64 and (np.sort(order, axis=1) == np.arange(96)).all()
    assert np.array_equal(order, m.rank_fit_order(96, 3, 5)) and not np.array_equal(order, m.rank_fit_order(96, 3, 6))
    assert not np.array_equal(order[0], order[1])
    # the ranker: the table's form, then the device
    for entries in (m.NTUPLE_ENTRIES_SUM, m.NTUPLE_ENTRIES_3X3_FEAT, m.ntuple_staged_entries_of("2x4"), 21505):
        with pytest.raises(ValueError, match="four plain forms") as e:
            T.NTupleRanker(torch.zeros(entries, dtype=torch.int32), 5, 10)
        assert all(form in str(e.value) for form in ("'2x4'", "'3x3'", "'feat'", "'feat+spare'"))
    for bad in (None, np.zeros(21504, np.int32), torch.zeros(21504, dtype=torch.float32), torch.zeros((2, 21504), dtype=torch.int32)):
        with pytest.raises(ValueError, match="table must be a contiguous int32 tensor"):
            T.NTupleRanker(bad, 5, 10)
    with pytest.raises(ValueError, match="on a GPU"):
        T.NTupleRanker(torch.zeros(21504, dtype=torch.int32), 5, 10)
    p = inspect.signature(T.NTupleRanker.__init__).parameters
    assert list(p) == ["self", "table", "L", "M", "gamma", "reward", "rate", "margin", "bound", "symmetric"]
    assert [p[k].default for k in ("gamma", "reward", "rate", "margin", "bound", "symmetric")] == [0.99, (1.0, 0.0, 0.0), 8.0, 0.0, False, False]
    assert list(inspect.signature(T.collect_labels).parameters) == ["env", "pieces", "policy", "steps", "max_nodes", "weights"]
    assert inspect.signature(T.collect_labels).parameters["max_nodes"].default == 1 << 12
    for name in ("NTupleRanker", "LabelSet", "collect_labels", "label_agreement"):
        assert name in T.__all__ and getattr(T, name) is not None
    assert T.NTupleRanker is T.ntuple.NTupleRanker and T.LabelSet is T.solve.LabelSet
    for doc in (T.NTupleRanker.__doc__, T.collect_labels.__doc__, T.label_agreement.__doc__):
        assert "proves nothing" in re.sub(r"\s+", " ", doc)
    # a LabelSet on the host: append, len, split by entry and by node
    s = T.LabelSet("cpu")
    assert len(s) == 0
    a = torch.arange(40, dtype=torch.int32).reshape(10, 4)
    s.append(a, a + 100, torch.ones((10, 40), dtype=torch.uint8), torch.tensor([5, 5, 2, 9, 2, 7, 7, 7, 9, 5]))
    assert len(s) == 10 and s.entry.dtype == torch.int32 and s.planes_a.is_contiguous()
    first, second = s.split(0.5)                               # entries 2, 5 | 7, 9
    assert sorted(first.entry.tolist()) == [2, 2, 5, 5, 5] and sorted(second.entry.tolist()) == [7, 7, 7, 9, 9]
    assert torch.equal(first.planes_b, first.planes_a + 100) and len(first) + len(second) == 10
    first, second = s.split(0.3, by="node")
    assert torch.equal(first.planes_a, a[:3]) and torch.equal(second.planes_a, a[3:])
    for bad in (dict(fraction=1.5), dict(fraction=True), dict(by="rows")):
        with pytest.raises(ValueError):
            s.split(**bad)
    with pytest.raises(ValueError):
        s.append(a, a, torch.ones((9, 40), dtype=torch.uint8))
    with pytest.raises(ValueError):
        s.append(a.to(torch.int64), a, torch.ones((10, 40), dtype=torch.uint8))


def test_the_header_states_the_rule_and_the_library_exports_the_entry():
    m = _m()
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_\w+)\s*\(", text))
    assert declared == set(m.LEARN_SYMBOLS) and ENTRY in declared
    lib = ctypes.CDLL(m.build_library())
    assert hasattr(lib, ENTRY)
    proto = re.search(r"int %s\((.*?)\);" % ENTRY, text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ARGS
    assert len(m.lib().tpl_ntuple_rank.argtypes) == len(ARGS)
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("THE TABLE IS READ ONLY", "LABEL 3 PROVES NOTHING AND TEACHES NOTHING", "is tpl_ntuple_act's score, bit for bit",
                  "A tie violates at margin 0", "A NaN gap does not violate", "win = loss = 255", "the row is not trusted to be well formed",
                  "slots = 1, head = 0, horizon = 1", "the same bytes in any order of arrival", "prune = 1 outside the budget form"):
        assert words in flat, words
    # a unit of its own in the act kernel's frame; ntuple.hip does not know it
    units = [os.path.basename(p) for p in m._UNITS]
    assert "ntuple_rank.hip" in units and "ntuple.hip" in units and units[-1] == "heuristic.hip"
    body = open(os.path.join(m._LEARN_CSRC, "ntuple_rank.hip")).read()
    assert "ntuple_value<S>" in body and "prune_dead<S>" in body and "first_move(" in body and "ordered_bits(" in body
    assert '#include "ntuple.hip"' not in body and "draw_hash" not in body and "atomicAdd" not in body
    assert "ntuple_rank" not in open(os.path.join(m._LEARN_CSRC, "ntuple.hip")).read()
    assert any(p.endswith(os.path.join("learn", "ntuple_rank.hip")) for p in m._sources())


def _waves(vgpr):
    """Waves a SIMD by the vector registers on gfx950: 512 a lane, handed out in blocks of 8, eight waves at the most."""
    return min(8, 512 // (8 * ((vgpr + 7) // 8)))


def test_the_four_kernels_use_no_scratch_and_keep_their_act_twins_waves():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    num = lambda r, what: int(r[r.index(what) - 1])

    def one(kernel):
        mine = [r for r in rows if f"{len(kernel)}{kernel}E" in r[-1]]       # the whole mangled name: no name within another
        assert len(mine) == 1, (kernel, [r[-1] for r in rows])
        return mine[0]

    for kernel, twin in KERNELS.items():
        r, t = one(kernel), one(twin)
        print(kernel, "vgpr", num(r, "vgpr"), "sgpr", num(r, "sgpr"), "lds", num(r, "lds"), "| twin vgpr", num(t, "vgpr"))
        assert num(r, "scratch") == 0, r
        assert _waves(num(r, "vgpr")) >= _waves(num(t, "vgpr")), (r, t)
        assert num(r, "lds") <= 1024, r                                      # the shape table, three maxima and the pair's scores


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_host_entry_code_under_address_and_ub_sanitizers(tmp_path):
    """The host side of csrc/learn/ntuple_rank.hip (the entry's argument checks) compiled host-only with -fsanitize=address,undefined
    and driven by a stand-alone program over every refusal path.  Nothing is loaded into Python."""
    flags = ["--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
             "-I", os.path.join(ROOT, "include")]
    exe = str(tmp_path / "sanitize_ntuple_rank")
    cmd = ["hipcc"] + flags + [os.path.join(_m()._LEARN_CSRC, "ntuple_rank.hip"),
                               os.path.join(ROOT, "tests", "c_abi", "sanitize_ntuple_rank.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "sanitizer run ok" in res.stdout, res.stdout + res.stderr
