"""The exact search from a node and the proved move labels on one MI355X (include/tpl_learn.h's rules;
tpl_placement_exact_nodes[_move] and tpl_placement_exact_labels[_move] in csrc/learn/exact_nodes.hip; T.prove_nodes, T.label_moves,
T.label_states).  THE KERNELS ARE THE MIRRORS, byte for byte, through guard-framed buffers filled with 0xCD; the mirrors are pinned
to the shifted game by tests/test_exact_nodes_cpu.py, whose node sets these tests share:

  1. both entries, both feature forms, on the three node sets (32 nodes a set, 1,280 waves for the labels);
  2. tpl_placement_exact_nodes at lines = moves = 0, entry = arange(n) against the existing T.prove_configs on the same 32 configurations
     at (5, 20): all six outputs;
  3. tpl_placement_exact_labels against T.prove_nodes called on the children;
  4. edge nodes in one launch -- a finished node, one move left, the last list, entries out of range --: every output written in full;
  5. M = 254 with the nodes at moves = 250: the largest stack, the piece index at the end of the list;
  6. T.label_states on 64 boards over the 32-entry pool, auto_reset=False, along the recorded solutions.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import load_golden
from test_exact_nodes_cpu import CAP, COUNT, L5, SETS, mirror_labels, mirror_nodes, node_sets, weights_of
from test_learn_range_gpu import Framed, _check, _stream
from test_learner_gpu import _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NODE_NAMES = ("solved", "proved", "solution_len", "actions", "bound", "nodes")
NODE_DTYPES = dict(solved=np.uint8, proved=np.uint8, solution_len=np.int32, actions=np.uint8, bound=np.int32, nodes=np.uint32)
LABEL_NAMES = ("label", "length", "nodes")
LABEL_DTYPES = dict(label=np.uint8, length=np.int32, nodes=np.uint32)


def _m():
    return T._learn_lib


def _weight_buffer(w):
    """A weight row as the entries read it: twelve floats, or sixteen with NaN in the two entries that are never read."""
    if w.shape[0] == 12:
        return np.array(w, np.float32)
    out = np.full(16, np.nan, np.float32)
    out[:14] = w
    return out


def _inputs(rows, lines, moves, entry, pieces, w):
    """The six inputs in guard-framed buffers."""
    wb = _weight_buffer(np.asarray(w, np.float32))
    host = (np.ascontiguousarray(rows, np.uint16), np.ascontiguousarray(lines, np.uint8), np.ascontiguousarray(moves, np.uint8),
            np.ascontiguousarray(entry, np.uint32), np.ascontiguousarray(pieces, np.uint8), wb)
    frames = []
    for seed, x in enumerate(host):
        f = Framed(x.nbytes, seed + 1)
        f.inner().copy_(torch.from_numpy(x.view(np.uint8).reshape(-1)))
        frames.append(f)
    return frames


def _launch(kind, rows, lines, moves, entry, pieces, L, M, w, max_nodes, shortest=True, spare_weight=0.0):
    """tpl_placement_exact_nodes[_move] (kind "nodes") or tpl_placement_exact_labels[_move] ("labels") through guard-framed buffers,
    every output filled with 0xCD first: the outputs on the host."""
    n, n_cfg = rows.shape[0], pieces.shape[0]
    assert pieces.shape == (n_cfg, M + 1)
    frames = _inputs(rows, lines, moves, entry, pieces, w)
    if kind == "nodes":
        names, dtypes, sizes = NODE_NAMES, NODE_DTYPES, dict(solved=n, proved=n, solution_len=4 * n, actions=n * M, bound=4 * n, nodes=4 * n)
    else:
        names, dtypes, sizes = LABEL_NAMES, LABEL_DTYPES, dict(label=40 * n, length=160 * n, nodes=160 * n)
    out = {k: Framed(sizes[k], 10 + j) for j, k in enumerate(names)}
    for f in out.values():
        f.inner().fill_(0xCD)
    head = [f.ptr() for f in frames[:5]] + [n, n_cfg, L, M, frames[5].ptr(), float(spare_weight), int(max_nodes)]
    if kind == "nodes":
        head.append(int(shortest))
    _check(_m().entry("exact_" + kind, len(w))(*head, *(out[k].ptr() for k in names), _stream()))
    for f in list(out.values()) + frames:
        f.assert_canary((kind, L, M, n))
    got = {k: out[k].host().view(dtypes[k]).copy() for k in names}
    if kind == "nodes":
        got["actions"] = got["actions"].reshape(n, M)
    else:
        got = {k: v.reshape(n, 40) for k, v in got.items()}
    return got


def _same(got, want, names, what):
    for name, ref in zip(names, want):
        assert got[name].dtype == ref.dtype and got[name].shape == ref.shape, (what, name, got[name].shape, ref.shape)
        bad = np.argwhere(got[name].view(np.uint8) != np.ascontiguousarray(ref).view(np.uint8))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())


def _args(grp):
    return grp["rows"], grp["lines"], grp["moves"], grp["entry"], grp["pieces"], L5, grp["M"]


# ------------------------------------------------------------------------------------------------ 1. the kernels are the mirrors
@pytest.mark.parametrize("count", (12, 14))
@pytest.mark.parametrize("key", list(SETS))
def test_both_entries_are_their_mirrors_byte_for_byte(key, count):
    w = weights_of(count)
    waves = 0
    for q, grp in enumerate(node_sets(key)):
        _same(_launch("nodes", *_args(grp), w, CAP), mirror_nodes(key, count)[q], NODE_NAMES, (key, count, q))
        got = _launch("labels", *_args(grp), w, CAP)
        _same(got, mirror_labels(key, count)[q], LABEL_NAMES, (key, count, q))
        assert not (got["label"] == 3).any()                   # nothing is capped in these sets
        waves += got["label"].size
    assert waves == 40 * COUNT
    if key == "back3_spare1" and count == 12:                  # the first win at the full budget, and a cap that binds
        for q, grp in enumerate(node_sets(key)):
            _same(_launch("nodes", *_args(grp), w, CAP, shortest=False), mirror_nodes(key, count, CAP, False)[q], NODE_NAMES, (key, "first", q))
            got = _launch("labels", *_args(grp), w, 8)
            _same(got, mirror_labels(key, count, 8)[q], LABEL_NAMES, (key, "cap 8", q))
            assert (got["nodes"][got["label"] == 3] == 8).all()


# ------------------------------------------------------------------------------------------------ 2. a root is a node
def test_at_move_0_the_nodes_entry_writes_what_prove_configs_writes():
    g = load_golden("carved_L5_M20.npz")
    rows, pieces, M = g["rows"][:COUNT], g["pieces"][:COUNT], int(g["M"])
    zero = np.zeros(COUNT, np.uint8)
    for w in (weights_of(12), weights_of(14)):
        for shortest in (True, False):
            want = T.prove_configs(rows, pieces, L5, M, weights=w, max_nodes=CAP, shortest=shortest, device=DEV)
            got = _launch("nodes", rows, zero, zero, np.arange(COUNT), pieces, L5, M, w, CAP, shortest=shortest)
            for name in NODE_NAMES:
                assert np.array_equal(got[name], _np(want[name]).astype(NODE_DTYPES[name])), (name, len(w), shortest)
            out = T.prove_nodes(rows, zero, zero, np.arange(COUNT), pieces, L5, M, weights=w, max_nodes=CAP, shortest=shortest, device=DEV)
            assert set(out) == set(want)
            for name in want:
                assert out[name].dtype == want[name].dtype and torch.equal(out[name], want[name]), name
    assert _np(want["proved"]).any()


# ------------------------------------------------------------------------------------------------ 3. the labels are the children's searches
@pytest.mark.parametrize("count", (12, 14))
def test_the_labels_are_prove_nodes_on_the_children(count):
    m, w = _m(), weights_of(count)
    for grp in node_sets("back3_spare1"):
        k, M = grp["idx"].size, grp["M"]
        out = T.label_moves(*_args(grp), weights=w, max_nodes=CAP, device=DEV)
        assert set(out) == {"label", "length", "nodes", "winning", "best"}
        kinds = dict(label=torch.uint8, length=torch.int32, nodes=torch.int32, winning=torch.bool, best=torch.uint8)
        for name, kind in kinds.items():
            assert out[name].dtype == kind and tuple(out[name].shape) == ((k,) if name == "best" else (k, 40)) and out[name].device.type == "cuda"
        label, length, nodes = (_np(out[name]) for name in LABEL_NAMES)
        # every distinct placement, moved and judged as the rule says, on the host
        cur = grp["pieces"][grp["entry"], grp["moves"]] & 7
        distinct = m.canonical_actions(cur[:, None], np.arange(40)[None, :]) == np.arange(40)[None, :]
        node, b = np.nonzero(distinct)
        r2, _, l2, m2, s2 = m.host_moves(grp["rows"][node], cur[node], b // 10, b % 10, L5, M, grp["lines"][node], grp["moves"][node])
        s2 = np.where(m.move_bound(r2, L5, M, l2, m2, s2)["dead"], 2, s2)
        assert not label[~distinct].any() and not length[~distinct].any() and not nodes[~distinct].any()
        assert (label[node, b][s2 == 1] == 1).all() and (length[node, b][s2 == 1] == 1).all() and (label[node, b][s2 >= 2] == 2).all()
        run = np.flatnonzero(s2 == 0)
        kids = T.prove_nodes(r2[run], l2[run], m2[run], grp["entry"][node[run]], grp["pieces"], L5, M, weights=w, max_nodes=CAP, device=DEV)
        solved, proved, sol_len, count_ = (_np(kids[name]) for name in ("solved", "proved", "solution_len", "nodes"))
        assert np.array_equal(label[node[run], b[run]], np.where(solved, 1, np.where(proved, 2, 3)))
        assert np.array_equal(length[node[run], b[run]], np.where(solved, 1 + sol_len, 0)) and np.array_equal(nodes[node[run], b[run]], count_)
        assert np.array_equal(_np(out["winning"]), label == 1) and np.array_equal(_np(out["best"]), m.best_labelled_move(label, length))
        at = np.arange(k)
        assert (label[at, grp["sol_move"]] == 1).all()


# ------------------------------------------------------------------------------------------------ 4. edge nodes
@pytest.mark.parametrize("count", (12, 14))
def test_edge_nodes_in_one_launch_write_every_output_in_full(count):
    m, w = _m(), weights_of(count)
    grp = node_sets("back3")[1]
    k, M = grp["idx"].size, grp["M"]
    assert k >= 6
    rows, lines, moves, entry = grp["rows"].copy(), grp["lines"].copy(), grp["moves"].copy(), grp["entry"].copy()
    lines[0] = L5                                              # finished: nothing is owed
    moves[1] = M - 1                                           # one move left: a stack of one record
    entry[2] = k - 1                                           # the last list
    entry[3] = k                                               # the first entry past the lists
    entry[4] = 0xFFFFFFFF                                      # config_index's UNKNOWN
    moves[5] = M                                               # no move left
    for kind, names, mirror in (("nodes", NODE_NAMES, m.placement_exact_nodes), ("labels", LABEL_NAMES, m.placement_exact_labels)):
        got = _launch(kind, rows, lines, moves, entry, grp["pieces"], L5, M, w, CAP)
        _same(got, mirror(rows, lines, moves, entry, grp["pieces"], L5, M, w, CAP), names, (kind, count))
        for name in names:                                     # nothing of the 0xCD fill is left: a flag, a label, a placement or 255
            assert not (got[name].view(np.uint8).reshape(k, -1) == 0xCD).all(axis=1).any(), (kind, name)
        if kind == "nodes":
            for j in (0, 3, 4, 5):
                assert [int(got[name][j]) for name in ("solved", "proved", "solution_len", "bound", "nodes")] == [0, 1, 0, 0, 0]
                assert (got["actions"][j] == 255).all()
        else:
            assert not got["label"][[0, 3, 4, 5]].any() and not got["nodes"][[0, 3, 4, 5]].any() and not (got["label"][1] == 3).any()
            assert got["label"][2].any() and not got["nodes"][1].any()


# ------------------------------------------------------------------------------------------------ 5. the largest stack
def test_nodes_at_move_250_of_a_game_of_254_moves_are_their_mirrors():
    """The back4 boards with their last five pieces at places 250 .. 254 of a list of 255: the shifted game is (5 - lines, 4)."""
    m, M = _m(), 254
    gen = np.random.default_rng(254)
    for grp in node_sets("back4")[:2]:
        k, at = grp["idx"].size, int(grp["moves"][0])
        lists = gen.integers(0, 7, (k, M + 1), dtype=np.uint8)
        lists[:, 250:] = grp["pieces"][:, at:at + 5]
        moves = np.full(k, 250, np.uint8)
        for count in (12, 14):
            w = weights_of(count)
            got = _launch("nodes", grp["rows"], grp["lines"], moves, grp["entry"], lists, L5, M, w, CAP)
            _same(got, m.placement_exact_nodes(grp["rows"], grp["lines"], moves, grp["entry"], lists, L5, M, w, CAP), NODE_NAMES, ("254", count))
            assert got["solved"].all() and (got["solution_len"] == 4).all() and (got["actions"][:, 4:] == 255).all()
            got = _launch("labels", grp["rows"], grp["lines"], moves, grp["entry"], lists, L5, M, w, CAP)
            _same(got, m.placement_exact_labels(grp["rows"], grp["lines"], moves, grp["entry"], lists, L5, M, w, CAP), LABEL_NAMES, ("254", count))
            assert (got["label"][np.arange(k), grp["sol_move"]] == 1).all()


# ------------------------------------------------------------------------------------------------ 6. an environment's boards
def test_label_states_labels_the_boards_of_an_environment_and_leaves_it_as_it_was():
    g = load_golden("carved_L5_M20.npz")
    rows, pieces, M, n = g["rows"][:COUNT], g["pieces"][:COUNT], int(g["M"]), 64
    sol_len = g["sol_len"][:COUNT].astype(np.int64)
    sol = 10 * g["sol"][:COUNT, :, 0].astype(np.int64) + g["sol"][:COUNT, :, 1]
    env = T.BatchedTetris(L5, M, n, device=DEV, seed=5, auto_reset=False)
    env.load_configs(rows, pieces)
    env.reset()
    dealt = _np(T.config_index(env)).astype(np.int64)
    assert ((dealt >= 0) & (dealt < COUNT)).all()
    board = np.arange(n)
    checked = {"first": 0, "second": 0, "late": 0, "finished": 0}
    for t in range(int(sol_len.max()) - 2):
        before = env.snapshot().data.clone()
        out = T.label_states(env, pieces)
        assert torch.equal(env.snapshot().data, before)        # read, never written
        state = {name: _np(v) for name, v in env.packed_state().items()}
        running = state["state"] == 0
        assert np.array_equal(_np(out["running"]), running) and np.array_equal(running, t < sol_len[dealt])
        entry = _np(T.config_index(env))
        assert np.array_equal(_np(out["entry"]), entry) and np.array_equal(entry[running], dealt[running]) and (entry[~running] == -1).all()
        assert (state["moves"][running] == t).all()
        # label_moves on the exported rows
        lines = np.where(running, state["lines"], L5).astype(np.uint8)
        same = T.label_moves(state["rows"], lines, state["moves"], np.where(running, dealt, COUNT), pieces, L5, M, device=DEV)
        for name in ("label", "length", "nodes", "winning", "best"):
            assert torch.equal(out[name], same[name]), (t, name)
        label, best = _np(out["label"]), _np(out["best"])
        assert not label[~running].any() and (best[~running] == 255).all()
        checked["finished"] += int((~running).sum())
        # the recorded next move is proved winning
        cur = pieces[dealt, np.minimum(t, M)] & 7
        move = _m().canonical_actions(cur, sol[dealt, np.minimum(t, M - 1)])
        where = running & ((t == 0) | (t == 1) | (t == sol_len[dealt] - 3))
        print("t", t, "boards", int(where.sum()), "labels of the recorded move", np.bincount(label[board[where], move[where]], minlength=4).tolist(),
              "unproved moves", int((label[running] == 3).sum()), "most nodes", int(_np(out["nodes"]).max()))
        assert (label[board[where], move[where]] == 1).all(), t
        assert (_np(out["length"])[board[where], move[where]] <= sol_len[dealt[where]] - t).all()
        checked["first" if t == 0 else "second" if t == 1 else "late"] += int(where.sum())
        action = np.where(running, sol[dealt, np.minimum(t, M - 1)], 0).astype(np.uint8)
        env.step(torch.from_numpy(action).to(DEV), observe=False)
    assert checked["first"] == n and checked["second"] == n and checked["late"] == n and checked["finished"] > 0
    assert (_np(env.state)[sol_len[dealt] <= int(sol_len.max()) - 2] == 1).all()       # the recorded solutions win
    env.terminate()
