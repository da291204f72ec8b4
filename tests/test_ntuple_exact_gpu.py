"""The table-ordered exact depth-first solver on one MI355X (include/tpl_learn.h's rule under tpl_ntuple_exact;
csrc/learn/ntuple_exact.hip; T.ntuple_prove_configs).  THE KERNEL IS THE MIRROR, byte for byte in solved, proved, solution_len, actions,
bound and nodes, through guard-framed buffers filled with 0xCD, against tests/golden/ntuple_exact_mirror.npz
(tests/test_ntuple_exact_cpu.py pins the file to _learn_lib.ntuple_exact; tests/golden/make_golden_ntuple_exact.py lists the cases and
makes the tables again from their hash):

  1. the six small games of test_solve_cpu, both values of `shortest`, the zero and the hashed "feat+spare" table;
  2. generate_configs(3, 8, 64) at max_nodes 1, 7, 256 and 4,000 and (5, 12, 32) at 7, 256 and 4,000 -- the cap in mid-descent and between
     two budgets -- and the (3, 8) boards searched for four lines in six moves, under "feat+spare" and "feat"; on (3, 8, 64): n = 1,
     shortest = 0, gamma 0.5 with reward (1, 10, -1), the zero table with reward (0, 0, 0), where every key ties and the order is b alone,
     the huge table, whose sums are rounded, and "3x3" and "2x4" at 256 nodes;
  3. the 32 carved configurations at a budget of their own sol_len each, max_nodes = 4,000;
  4. games of 254 moves at max_nodes = 300, where the descent reaches the deepest records of the stack and the spare row's last bin;
  5. T.ntuple_prove_configs: the dict, its dtypes and shapes, tensors and arrays as input, bound > M proved without a node.
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
import make_golden_ntuple_exact as N  # noqa: E402  -- the cases, their tables
import make_golden_exact as G  # noqa: E402  -- the inputs and the grouping of the carved case by budget

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = dict(N.cases())
DTYPES = dict(solved=np.uint8, proved=np.uint8, solution_len=np.int32, actions=np.uint8, bound=np.int32, nodes=np.uint32)
_device_tables = {}


def _m():
    return T._learn_lib


def _table(form, kind):
    """The table of a case in a guard-framed buffer of its own, uploaded once; every case checks its canaries."""
    if (form, kind) not in _device_tables:
        t = N.table(form, kind)
        f = Framed(t.size * 4, 3)
        f.inner().copy_(torch.from_numpy(t.view(np.uint8).copy()))
        _device_tables[(form, kind)] = (f, t.size)
    return _device_tables[(form, kind)]


def _exact(rows, pieces, L, M, form, kind, max_nodes, shortest, gamma, reward):
    """tpl_ntuple_exact through guard-framed buffers, every output filled with 0xCD first: the six arrays on the host."""
    n = rows.shape[0]
    rf, pf = Framed(n * 40, 1), Framed(n * (M + 1), 2)
    tf, entries = _table(form, kind)
    rf.inner().copy_(torch.from_numpy(np.ascontiguousarray(rows, np.uint16).view(np.uint8).reshape(-1)))
    pf.inner().copy_(torch.from_numpy(np.ascontiguousarray(pieces, np.uint8).reshape(-1)))
    out = dict(solved=Framed(n, 4), proved=Framed(n, 5), solution_len=Framed(4 * n, 6), actions=Framed(n * M, 7), bound=Framed(4 * n, 8),
               nodes=Framed(4 * n, 9))
    for f in out.values():
        f.inner().fill_(0xCD)
    _check(_m().lib().tpl_ntuple_exact(rf.ptr(), pf.ptr(), n, L, M, tf.ptr(), entries, *(float(r) for r in reward), float(gamma),
                                       int(max_nodes), int(shortest), *(out[k].ptr() for k in N.NAMES), _stream()))
    for name, f in list(out.items()) + [("rows", rf), ("pieces", pf), ("table", tf)]:
        f.assert_canary((L, M, n, name))
    assert np.array_equal(tf.host().view(np.int32), N.table(form, kind))      # nothing but the outputs is written
    got = {k: out[k].host().view(DTYPES[k]).copy() for k in N.NAMES}
    got["actions"] = got["actions"].reshape(n, M)
    return got


def _same(got, g, key):
    for name in N.NAMES:
        want = g[f"{key}_{name}"]
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, (key, name, got[name].shape, want.shape)
        bad = np.argwhere(got[name].view(np.uint8) != want.view(np.uint8))
        assert bad.size == 0, (key, name, len(bad), bad[:4].tolist())


def _run(key):
    a = CASES[key]
    rows, pieces = G.inputs(a)
    return _exact(rows, pieces, a["L"], a["M"], a["form"], a["kind"], a["max_nodes"], a["shortest"], a["gamma"], a["reward"])


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("small_")])
def test_the_small_games_are_the_mirror_byte_for_byte(key):
    got = _run(key)
    _same(got, load_golden("ntuple_exact_mirror.npz"), key)
    assert got["proved"].all()                                 # the node budget is never reached


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("cfg_")])
def test_the_cap_in_mid_descent_and_between_budgets_is_the_mirrors(key):
    got = _run(key)
    _same(got, load_golden("ntuple_exact_mirror.npz"), key)
    cap = CASES[key]["max_nodes"]
    assert (got["nodes"] <= cap).all() and (got["nodes"][got["proved"] == 0] == cap).all()
    assert (got["solved"] <= got["proved"]).all()


def test_the_carved_configurations_at_their_own_budgets_are_the_mirror_byte_for_byte():
    g = load_golden("ntuple_exact_mirror.npz")
    rows, pieces, sol_len, L, M = G.carved_inputs()
    parts = []
    for budget, idx in G.carved_groups(sol_len):
        got = _exact(rows[idx], pieces[idx, :budget + 1], L, budget, N.BUDGET, "hashed", N.CARVED_NODES, True, 1.0, (1.0, 0.0, 0.0))
        parts.append((idx, budget, tuple(got[k] for k in N.NAMES)))
    got = G.carved_gather(parts, G.CARVED_COUNT, M)
    _same(got, g, "carved")
    proved = got["proved"] == 1
    assert (got["solved"][proved] == 1).all() and np.array_equal(got["solution_len"][proved], sol_len[proved])


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("long_")])
def test_a_game_of_254_moves_reaches_the_deepest_records_and_is_the_mirror(key):
    got = _run(key)
    _same(got, load_golden("ntuple_exact_mirror.npz"), key)
    assert (got["nodes"] <= G.LONG_NODES).all()


def test_ntuple_prove_configs_returns_the_mirrors_outputs_with_optimal_and_unwinnable():
    g = load_golden("ntuple_exact_mirror.npz")
    key = "cfg_L3_M8_c256_budget"
    a = CASES[key]
    rows, pieces = G.inputs(a)
    n, L, M = rows.shape[0], a["L"], a["M"]
    table = torch.from_numpy(N.table(a["form"], a["kind"]).copy()).to(DEV)
    out = T.ntuple_prove_configs(rows, pieces, L, M, table, max_nodes=a["max_nodes"], device=DEV)
    assert set(out) == {"solved", "proved", "solution_len", "actions", "solution", "bound", "nodes", "optimal", "unwinnable"}
    kinds = dict(solved=torch.bool, proved=torch.bool, solution_len=torch.int32, actions=torch.uint8, solution=torch.uint8,
                 bound=torch.int32, nodes=torch.int32, optimal=torch.bool, unwinnable=torch.bool)
    for name, kind in kinds.items():
        shape = (n, M) if name == "actions" else (n, M, 2) if name == "solution" else (n,)
        assert out[name].dtype == kind and tuple(out[name].shape) == shape and out[name].device.type == "cuda", name
    host = {k: _np(v) for k, v in out.items()}
    for name in N.NAMES:
        want = g[f"{key}_{name}"]
        assert np.array_equal(host[name].astype(want.dtype), want), name
    assert np.array_equal(host["optimal"], host["solved"]) and np.array_equal(host["unwinnable"], host["proved"] & ~host["solved"])
    played = host["actions"] != 255
    assert np.array_equal(host["solution"][..., 0][played], host["actions"][played] // 10)
    assert np.array_equal(host["solution"][..., 1][played], host["actions"][played] % 10) and (host["solution"][~played] == 0).all()
    # what is solved feeds tighten_pool unchanged
    kept = T.tighten_pool(rows, pieces, host["solved"], host["solution_len"], M_new=4)
    assert kept[0].shape[0] == int((host["solved"] & (host["solution_len"] <= 4)).sum()) and kept[1].shape[1] == 5
    # tensors as input, cells for rows, pieces without the piece behind the last move, a table on the host; shortest=False: nothing
    # is called optimal.  gamma and the reward reach the kernel
    cells = torch.from_numpy(((rows[:, :, None] >> np.arange(10)) & 1).astype(bool)).to(DEV)
    first = T.ntuple_prove_configs(cells, torch.from_numpy(pieces).to(DEV), L, M, table.cpu(), max_nodes=256, shortest=False, device=DEV,
                                   validate=False)
    for name in N.NAMES:
        want = g[f"cfg_L3_M8_c256_first_{name}"]
        assert np.array_equal(_np(first[name]).astype(want.dtype), want), name
    assert not _np(first["optimal"]).any()
    other = T.ntuple_prove_configs(rows, pieces[:, :M], L, M, table, gamma=0.5, reward=(1.0, 10.0, -1.0), max_nodes=256, device=DEV)
    short = CASES["cfg_L3_M8_c256_gamma"]
    assert (short["gamma"], short["reward"]) == (0.5, (1.0, 10.0, -1.0))
    # pieces [n, M] are padded with piece 0 where the recorded case has the list's own last piece: V of a child at depth M - 1 is never
    # read, because a child that has made M moves does not run, so the outputs are the recorded ones
    for name in N.NAMES:
        want = g[f"cfg_L3_M8_c256_gamma_{name}"]
        assert np.array_equal(_np(other[name]).astype(want.dtype), want), name
    # a board that owes more than M moves can supply is proved unwinnable without a node: three rows of an empty board ask for thirty cells, eight moves
    empty = T.ntuple_prove_configs(np.zeros((2, 20), np.uint16), np.zeros((2, 3), np.uint8), 3, 2, table, device=DEV)
    assert _np(empty["unwinnable"]).all() and (_np(empty["nodes"]) == 0).all() and (_np(empty["bound"]) == 8).all()
    # the entry count selects the kernel: a "feat" table
    key = "cfg_L5_M12_c256_feat"
    a = CASES[key]
    rows, pieces = G.inputs(a)
    feat = torch.from_numpy(N.table(a["form"], a["kind"]).copy()).to(DEV)
    out = T.ntuple_prove_configs(rows, pieces, a["L"], a["M"], feat, max_nodes=256, device=DEV)
    for name in N.NAMES:
        assert np.array_equal(_np(out[name]).astype(g[f"{key}_{name}"].dtype), g[f"{key}_{name}"]), name
