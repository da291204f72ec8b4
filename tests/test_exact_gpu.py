"""The exact depth-first solver on one MI355X (include/tpl_learn.h's rule; tpl_placement_exact[_move] in csrc/learn/exact.hip;
T.prove_configs).  THE KERNEL IS THE MIRROR, byte for byte in solved, proved, solution_len, actions, bound and nodes, through
guard-framed buffers filled with 0xCD, against tests/golden/exact_mirror.npz (tests/test_exact_cpu.py pins the file to
_learn_lib.placement_exact; tests/golden/make_golden_exact.py lists the cases):

  1. the six small games of test_solve_cpu, both values of `shortest`, twelve weights and fourteen -- the fourteen in a row of
     sixteen with NaN in the two entries that are never read;
  2. generate_configs(3, 8, 64) and (5, 12, 32) at max_nodes 1, 7, 256 and 4,000 -- the cap in mid-descent and between two budgets --,
     spare_weight = 1, the fourteen weights at a cap, shortest = 0, n = 1 (a workgroup holds one configuration, so every n is
     a whole number of them), and the (3, 8) boards searched for four lines in six moves, where proofs that there is no win take
     a thousand nodes and more over several budgets;
  3. the 32 carved configurations at a budget of their own sol_len each, max_nodes = 4,000;
  4. games of 254 moves at max_nodes = 300, where the descent reaches the deepest records of the stack;
  5. T.prove_configs: the dict, its dtypes and shapes, optimal and unwinnable, tensors and arrays as input.
"""
import sys

import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import GOLDEN, load_golden
from test_learn_range_gpu import Framed, _check, _stream
from test_learner_gpu import _np

sys.path.insert(0, GOLDEN)
import make_golden_exact as G  # noqa: E402  -- the cases, their inputs and the grouping of the carved case by budget

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = dict(G.cases())
DTYPES = dict(solved=np.uint8, proved=np.uint8, solution_len=np.int32, actions=np.uint8, bound=np.int32, nodes=np.uint32)


def _m():
    return T._learn_lib


def _weight_buffer(w):
    """A weight row as the entries read it: twelve floats, or sixteen with NaN in the two entries that are never read."""
    if w.shape[0] == 12:
        return np.array(w, np.float32)
    out = np.full(16, np.nan, np.float32)
    out[:14] = w
    return out


def _exact(rows, pieces, L, M, w, max_nodes, shortest, spare_weight):
    """tpl_placement_exact[_move] through guard-framed buffers, every output filled with 0xCD first: the six arrays on the host."""
    n = rows.shape[0]
    wb = _weight_buffer(np.asarray(w, np.float32))
    rf, pf, wf = Framed(n * 40, 1), Framed(n * (M + 1), 2), Framed(wb.size * 4, 3)
    rf.inner().copy_(torch.from_numpy(np.ascontiguousarray(rows, np.uint16).view(np.uint8).reshape(-1)))
    pf.inner().copy_(torch.from_numpy(np.ascontiguousarray(pieces, np.uint8).reshape(-1)))
    wf.inner().copy_(torch.from_numpy(wb.view(np.uint8)))
    out = dict(solved=Framed(n, 4), proved=Framed(n, 5), solution_len=Framed(4 * n, 6), actions=Framed(n * M, 7), bound=Framed(4 * n, 8),
               nodes=Framed(4 * n, 9))
    for f in out.values():
        f.inner().fill_(0xCD)
    entry = _m().entry("exact", len(w))
    _check(entry(rf.ptr(), pf.ptr(), n, L, M, wf.ptr(), float(spare_weight), int(max_nodes), int(shortest),
                 *(out[k].ptr() for k in G.NAMES), _stream()))
    for name, f in list(out.items()) + [("rows", rf), ("pieces", pf), ("weights", wf)]:
        f.assert_canary((L, M, n, name))
    got = {k: out[k].host().view(DTYPES[k]).copy() for k in G.NAMES}
    got["actions"] = got["actions"].reshape(n, M)
    return got


def _same(got, g, key):
    for name in G.NAMES:
        want = g[f"{key}_{name}"]
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, (key, name, got[name].shape, want.shape)
        bad = np.argwhere(got[name].view(np.uint8) != want.view(np.uint8))
        assert bad.size == 0, (key, name, len(bad), bad[:4].tolist())


def _run(key):
    a = CASES[key]
    rows, pieces = G.inputs(a)
    return _exact(rows, pieces, a["L"], a["M"], G.weights()[a["F"]], a["max_nodes"], a["shortest"], a["spare_weight"])


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("small_")])
def test_the_small_games_are_the_mirror_byte_for_byte(key):
    got = _run(key)
    _same(got, load_golden("exact_mirror.npz"), key)
    assert got["proved"].all()                                 # the node budget is never reached


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("cfg_")])
def test_the_cap_in_mid_descent_and_between_budgets_is_the_mirrors(key):
    got = _run(key)
    _same(got, load_golden("exact_mirror.npz"), key)
    cap = CASES[key]["max_nodes"]
    assert (got["nodes"] <= cap).all() and (got["nodes"][got["proved"] == 0] == cap).all()
    assert (got["solved"] <= got["proved"]).all()


def test_the_carved_configurations_at_their_own_budgets_are_the_mirror_byte_for_byte():
    g = load_golden("exact_mirror.npz")
    rows, pieces, sol_len, L, M = G.carved_inputs()
    parts = []
    for budget, idx in G.carved_groups(sol_len):
        got = _exact(rows[idx], pieces[idx, :budget + 1], L, budget, T.CLASSICAL_WEIGHTS, G.CARVED_NODES, True, 0.0)
        parts.append((idx, budget, tuple(got[k] for k in G.NAMES)))
    got = G.carved_gather(parts, G.CARVED_COUNT, M)
    _same(got, g, "carved")
    proved = got["proved"] == 1
    assert proved.sum() >= 8 and (got["solved"][proved] == 1).all() and np.array_equal(got["solution_len"][proved], sol_len[proved])


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("long_")])
def test_a_game_of_254_moves_reaches_the_deepest_records_and_is_the_mirror(key):
    got = _run(key)
    _same(got, load_golden("exact_mirror.npz"), key)
    assert (got["nodes"] <= G.LONG_NODES).all()


def test_prove_configs_returns_the_mirrors_outputs_with_optimal_and_unwinnable():
    g = load_golden("exact_mirror.npz")
    key = "cfg_L3_M8_c256"
    a = CASES[key]
    rows, pieces = G.inputs(a)
    n, L, M = rows.shape[0], a["L"], a["M"]
    out = T.prove_configs(rows, pieces, L, M, max_nodes=a["max_nodes"], device=DEV)
    assert set(out) == {"solved", "proved", "solution_len", "actions", "solution", "bound", "nodes", "optimal", "unwinnable"}
    kinds = dict(solved=torch.bool, proved=torch.bool, solution_len=torch.int32, actions=torch.uint8, solution=torch.uint8,
                 bound=torch.int32, nodes=torch.int32, optimal=torch.bool, unwinnable=torch.bool)
    for name, kind in kinds.items():
        shape = (n, M) if name == "actions" else (n, M, 2) if name == "solution" else (n,)
        assert out[name].dtype == kind and tuple(out[name].shape) == shape and out[name].device.type == "cuda", name
    host = {k: _np(v) for k, v in out.items()}
    for name in G.NAMES:
        want = g[f"{key}_{name}"]
        assert np.array_equal(host[name].astype(want.dtype), want), name
    assert np.array_equal(host["optimal"], host["solved"]) and np.array_equal(host["unwinnable"], host["proved"] & ~host["solved"])
    played = host["actions"] != 255
    assert np.array_equal(host["solution"][..., 0][played], host["actions"][played] // 10)
    assert np.array_equal(host["solution"][..., 1][played], host["actions"][played] % 10) and (host["solution"][~played] == 0).all()
    # tensors as input, cells for rows, pieces without the piece behind the last move; shortest=False: nothing is called optimal
    cells = torch.from_numpy(((rows[:, :, None] >> np.arange(10)) & 1).astype(bool)).to(DEV)
    first = T.prove_configs(cells, torch.from_numpy(pieces[:, :M]).to(DEV), L, M, max_nodes=4000, shortest=False, device=DEV, validate=False)
    want = {name: g[f"cfg_L3_M8_c4000_first_{name}"] for name in G.NAMES}
    for name in G.NAMES:
        assert np.array_equal(_np(first[name]).astype(want[name].dtype), want[name]), name
    assert not _np(first["optimal"]).any()
    # a board that owes more than M moves can supply is proved unwinnable without a node: three rows of an empty board ask for thirty cells, eight moves
    empty = T.prove_configs(np.zeros((2, 20), np.uint16), np.zeros((2, 3), np.uint8), 3, 2, device=DEV)
    assert _np(empty["unwinnable"]).all() and (_np(empty["nodes"]) == 0).all() and (_np(empty["bound"]) == 8).all()
    # the fourteen weights select the other entry
    key = "cfg_L5_M12_c256_F14"
    a = CASES[key]
    rows, pieces = G.inputs(a)
    out = T.prove_configs(rows, pieces, a["L"], a["M"], weights=T.DELLACHERIE_WEIGHTS, max_nodes=256, device=DEV)
    for name in G.NAMES:
        assert np.array_equal(_np(out[name]).astype(g[f"{key}_{name}"].dtype), g[f"{key}_{name}"]), name
