"""CPU-side checks of the n-tuple beam search (include/tpl_learn.h's rule, tpl_ntuple_beam in csrc/learn/ntuple_beam.hip, the numpy
mirror in _learn_lib.py, ntuple.py's NTupleBeamPolicy and evaluate(width=)):

  1. the fold by hand on small paths: the leaf-inwards arithmetic against the forward accumulation it must not be, a path that ends
     the game, and a finished node carried through a ply unchanged;
  2. the mirror on random arrays: depth 1 is the arg-max of r + gamma V, depth 2 at full width is ntuple_search_choice's action and
     score with plan[1] <= second, a width of 1 is the greedy descent;
  3. the header declares the entry, the library exports it, the two kernels use no scratch and at most 128 VGPRs, and the counts the
     earlier tests pin are as they were;
  4. every refusal of the entry comes back as a status without a GPU;
  5. the Python refusals need no GPU.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tetris_piclim as T
from test_heuristic_cpu import _Env

f32 = np.float32
ARANGE = np.arange(40)


def _m():
    return T._learn_lib


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the fold by hand
def test_the_fold_goes_from_the_leaf_inwards_one_rounding_per_operation():
    m = _m()
    g = f32(0.99)
    # one ply: r + gamma * V, and r alone where the move ends the game (V is not read there)
    got = m.ntuple_beam_values([[0.5], [0.5]], [False, True], [3.0, np.nan], g)
    assert _bits(got).tolist() == _bits([f32(0.5) + g * f32(3.0), f32(0.5)]).tolist()
    # two plies: r1 + gamma * (r2 + gamma * v) is NOT (r1 + gamma * r2) + gamma * gamma * v -- a path where the last bit differs
    gen = np.random.default_rng(11)
    found = None
    for _ in range(2000):
        r1, r2, v = (f32(x) for x in gen.normal(size=3))
        inwards = f32(r1 + f32(g * f32(r2 + f32(g * v))))
        forwards = f32(f32(r1 + f32(g * r2)) + f32(f32(g * g) * v))
        if inwards != forwards:
            found = (r1, r2, v, inwards, forwards)
            break
    assert found is not None
    r1, r2, v, inwards, forwards = found
    got = m.ntuple_beam_values([[r1, r2]], [False], [v], g)
    assert _bits(got)[0] == _bits(inwards) and _bits(got)[0] != _bits(forwards)
    assert abs(int(_bits(inwards)) - int(_bits(forwards))) <= 4       # the last bits, not another quantity
    # three plies, the last move ends the game: r1 + g (r2 + g r3), V unread
    got = m.ntuple_beam_values([[1.0, 0.25, 10.0]], [True], [123.0], g)
    assert _bits(got)[0] == _bits(f32(1.0) + g * (f32(0.25) + g * f32(10.0)))
    # -0 stays -0: r = -0 and gamma * V = -0
    got = m.ntuple_beam_values([[-0.0]], [False], [-0.0], 1.0)
    assert _bits(got)[0] == 0x80000000
    with pytest.raises(ValueError, match="rewards"):
        m.ntuple_beam_values(np.zeros((3, 0), np.float32), [False] * 3, np.zeros(3), g)


def test_a_ply_lists_a_finished_node_once_and_carries_it_unchanged():
    m = _m()
    distinct = np.zeros(40, bool)
    distinct[[0, 3, 10, 13]] = True
    child = np.full((3, 40), 100.0, np.float32)                # what is not distinct must not be chosen
    child[0, [0, 3, 10, 13]] = (1.0, 4.0, 2.0, 4.0)
    child[2, [0, 3, 10, 13]] = (-0.0, 3.0, 5.0, 0.5)
    child[:, ~distinct] = 100.0
    # node 1 does not run: one candidate, value -0, path unchanged -- whatever child_value holds for it
    q, b, v = m.ntuple_beam_ply([9.0, -0.0, 9.0], [True, False, True], child, distinct, 64)
    assert q.tolist() == [0, 0, 0, 0, 1, 2, 2, 2, 2] and b.tolist() == [0, 3, 10, 13, 255, 0, 3, 10, 13]
    assert _bits(v).tolist() == _bits([1.0, 4.0, 2.0, 4.0, -0.0, -0.0, 3.0, 5.0, 0.5]).tolist()
    # width 3: 5.0, then the two 4.0 in candidate order; stored in candidate order
    q, b, v = m.ntuple_beam_ply([9.0, -0.0, 9.0], [True, False, True], child, distinct, 3)
    assert (q.tolist(), b.tolist(), v.tolist()) == ([0, 0, 2], [3, 13, 10], [4.0, 4.0, 5.0])
    # width 6: -0 of the carried node ties with -0 of (2, 0) and 0 is not there; the carried node comes first
    child[0, 0] = 0.75
    q, b, v = m.ntuple_beam_ply([9.0, -0.0, 9.0], [True, False, True], child, distinct, 8)
    assert (q.tolist(), b.tolist()) == ([0, 0, 0, 0, 1, 2, 2, 2], [0, 3, 10, 13, 255, 3, 10, 13])
    assert _bits(v)[4] == 0x80000000                           # with the bits it had
    # a beam of finished nodes only
    q, b, v = m.ntuple_beam_ply([2.0, 3.0], [False, False], np.zeros((2, 40), np.float32), distinct, 1)
    assert (q.tolist(), b.tolist(), v.tolist()) == ([1], [255], [3.0])


# ------------------------------------------------------------------------------------------------ 2. the mirror on random arrays
def _random_game(gen, K):
    """Two plies of made-up outcomes: ntuple_search_choice's arguments but gamma, and the one-ply values of every first move."""
    counts = (9, 17, 34)
    distinct1, distinct2 = np.zeros((K, 40), bool), np.zeros((K, 40), bool)
    for k in range(K):
        distinct1[k, np.sort(gen.choice(40, counts[k % 3], replace=False))] = True
        distinct2[k, np.sort(gen.choice(40, counts[(k // 3) % 3], replace=False))] = True
    small = lambda shape: (gen.integers(-2, 3, shape) * 0.25).astype(np.float32)       # many ties
    reward1 = np.where(gen.random((K, 40)) < 0.5, small((K, 40)), gen.normal(size=(K, 40))).astype(np.float32)
    reward2 = np.where(gen.random((K, 40, 40)) < 0.5, small((K, 40, 40)), gen.normal(size=(K, 40, 40))).astype(np.float32)
    value1 = gen.normal(size=(K, 40)).astype(np.float32) * f32(3)
    value2 = np.where(gen.random((K, 40, 40)) < 0.5, small((K, 40, 40)), gen.normal(size=(K, 40, 40)) * 3).astype(np.float32)
    done1, done2 = gen.random((K, 40)) < 0.2, gen.random((K, 40, 40)) < 0.2
    return reward1, done1, distinct1, reward2, done2, value2, distinct2, value1


def _children(game, k):
    reward1, done1, distinct1, reward2, done2, value2, distinct2, value1 = game

    def children(path):
        if len(path) == 0:
            return reward1[k], done1[k], value1[k], distinct1[k]
        a = path[0]
        assert len(path) == 1 and not done1[k, a]
        return reward2[k, a], done2[k, a], value2[k, a], distinct2[k]
    return children


def test_the_mirror_at_depth_one_two_and_width_one():
    m = _m()
    gen = np.random.default_rng(2176)
    K = 120
    game = _random_game(gen, K)
    reward1, done1, distinct1, reward2, done2, value2, distinct2, value1 = game
    differ = ended = 0
    for gamma in (0.99, 1.0, 0.0):
        g = f32(gamma)
        one = np.where(done1, reward1, reward1 + g * value1).astype(np.float32)
        action2, second2, score2, Q, _ = m.ntuple_search_choice(*game[:7], gamma)
        for k in range(K):
            children = _children(game, k)
            # depth 1, any width: the arg-max of r + gamma V over the distinct placements, the lowest index at the maximum
            masked = np.where(distinct1[k], one[k], -np.inf)
            want = int(np.argmax(masked == masked.max()))
            for width in (1, 5, 64):
                action, plan, score = m.ntuple_beam_choice(children, gamma, 1, width)
                assert (action, plan) == (want, [want]) and _bits(score) == _bits(one[k, want]), (k, width)
            # depth 2 at full width: the two-ply search's action and score; plan[1] <= second with equal folded values
            for width in (34, 64):
                action, plan, score = m.ntuple_beam_choice(children, gamma, 2, width)
                assert action == int(action2[k]) == plan[0] and _bits(score) == _bits(score2[k]), (k, gamma, width)
                if done1[k, action]:
                    assert plan[1] == 255 == int(second2[k])
                    ended += 1
                else:
                    assert plan[1] <= int(second2[k]) and distinct2[k, plan[1]]
                    fold = lambda b: m.ntuple_beam_values([[reward1[k, action], reward2[k, action, b]]], [done2[k, action, b]],
                                                          [value2[k, action, b]], gamma)[0]
                    assert fold(plan[1]) == fold(int(second2[k])) == score
                    differ += int(plan[1] != int(second2[k]))
            # width 1: the greedy descent -- the best first move by its one-ply value, then the best second move behind it
            action, plan, score = m.ntuple_beam_choice(children, gamma, 2, 1)
            assert action == want
            if done1[k, want]:
                assert plan == [want, 255] and _bits(score) == _bits(reward1[k, want])
            else:
                q = np.where(done2[k, want], reward2[k, want], reward2[k, want] + g * value2[k, want]).astype(np.float32)
                folded = np.where(distinct2[k], (reward1[k, want] + g * q).astype(np.float32), -np.inf)
                b = int(np.argmax(folded == folded.max()))
                assert plan == [want, b] and _bits(score) == _bits(folded[b]), (k, gamma)
        # a state that does not run
        assert m.ntuple_beam_choice(None, gamma, 3, 4, running=False) == (0, [255, 255, 255], f32(0.0))
    print(f"plan[1] below second on {differ} boards; the first move ended the game on {ended}")
    assert ended >= 10
    for depth in (0, 12, True, 1.5):
        with pytest.raises(ValueError, match="depth"):
            m.ntuple_beam_choice(None, 1.0, depth, 4)


# ------------------------------------------------------------------------------------------------ 3. symbols, resources
def test_the_header_declares_the_ntuple_beam_entry_and_the_library_exports_it():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and "tpl_ntuple_beam" in declared
    proto = re.search(r"int tpl_ntuple_beam\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == [
        "plane_a", "plane_b", "n", "L", "M", "r_line", "r_win", "r_lose", "gamma", "table", "depth", "width", "action", "plan", "score",
        "after_a", "after_b", "shape", "stream"]
    assert re.search(r"#define\s+TPL_NTUPLE_BEAM_MAX_DEPTH\s+11\b", text) and _m().NTUPLE_BEAM_MAX_DEPTH == 11
    for stated in ("min(D, 11 - moves(s) mod 10)", "tail_k = r_k + gamma * tail_{k+1}", "plan[1] <= second", "D = 1, any W"):
        assert stated in raw, stated
    lib = ctypes.CDLL(_m().build_library())
    assert hasattr(lib, "tpl_ntuple_beam")
    units = [os.path.basename(p) for p in _m()._UNITS]
    assert units[-1] == "heuristic.hip" and "ntuple_beam.hip" in units
    here = os.path.dirname(_m()._UNITS[-1])
    sources = [os.path.basename(p) for p in _m()._sources()]
    for shared in ("ntuple_beam.hip", "tpl_beam.h", "tpl_ntuple.h"):
        assert shared in sources, shared
    # shared, not copied: one definition of the table sum and of the selection rounds, both beam units on one frame
    text_of = lambda name: open(os.path.join(here, name)).read()
    assert "placement_beam_kernel" in text_of("beam.hip") and "ntuple_search_kernel" in text_of("ntuple.hip")
    for name in ("beam.hip", "ntuple.hip", "ntuple_beam.hip"):
        assert "long long ntuple_sum(" not in text_of(name) and "long long wave_max(" not in text_of(name), name
        assert "struct Shape2x4" not in text_of(name) and "select_keys(const" not in text_of(name), name
    assert "long long ntuple_sum(" in text_of("tpl_ntuple.h") and "struct Shape3x3" in text_of("tpl_ntuple.h")
    assert "long long wave_max(" in text_of("tpl_beam.h") and "select_keys(const" in text_of("tpl_beam.h")
    assert '#include "tpl_beam.h"' in text_of("beam.hip") and '#include "tpl_ntuple.h"' in text_of("ntuple.hip")
    assert '#include "tpl_beam.h"' in text_of("ntuple_beam.hip") and '#include "tpl_ntuple.h"' in text_of("ntuple_beam.hip")


def test_the_ntuple_beam_kernels_use_no_scratch_and_at_most_128_vgprs():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    for kernel in ("ntuple_beam_kernel", "ntuple_beam3_kernel"):
        mine = [r for r in rows if kernel in r[-1]]
        assert len(mine) == 1, (kernel, [r[-1] for r in rows])
        assert mine[0][mine[0].index("scratch") - 1] == "0", mine
        assert int(mine[0][mine[0].index("vgpr") - 1]) <= 128, mine
        assert int(mine[0][mine[0].index("lds") - 1]) <= 26 * 1024, mine            # six groups to a CU's 160 KB
    # what the earlier tests pin
    assert len([r for r in rows if "ntuple3_" in r[-1]]) == 9
    for kernel in ("ntuple_act_kernel", "ntuple_search_kernel", "ntuple_value_kernel", "placement_beam_kernel"):
        assert len([r for r in rows if kernel in r[-1]]) == 1, kernel
    assert len([r for r in rows if "ntuple_trace_kernel" in r[-1]]) == 2


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_every_refusal_of_the_ntuple_beam_entry_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    name = b"tpl_ntuple_beam"
    nan, inf = float("nan"), float("inf")

    def beam(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, depth=3, width=4, action=fake, plan=fake, score=fake,
             after_a=fake, after_b=fake, shape=0):
        return lib.tpl_ntuple_beam(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, depth, width, action, plan, score, after_a, after_b,
                                   shape, None)

    # the shape first, before any pointer is looked at
    for shape in (2, -1, 1 << 20):
        assert beam(a=None, b=None, table=None, action=None, plan=None, score=None, after_a=None, after_b=None, shape=shape,
                    depth=0, width=0) < 0 and b"shape must be" in err() and name in err(), shape
    for shape in (0, 1):
        for depth in (0, 12, -1, 1 << 30, -(1 << 31)):
            assert beam(depth=depth, shape=shape) < 0 and b"depth must be in [1, 11]" in err() and name in err(), depth
        for width in (0, 65, -1, 1 << 30, -(1 << 31)):
            assert beam(width=width, shape=shape) < 0 and b"width must be in [1, 64]" in err() and name in err(), width
        assert beam(after_a=None, shape=shape) < 0 and b"go together" in err() and name in err()
        assert beam(after_b=None, shape=shape) < 0 and b"go together" in err() and name in err()
    # the parent's checks under the new name: tpl_ntuple_act's
    limit = -(-(1 << 31) // 40)
    assert beam(a=None) < 0 and b"null" in err() and name in err()
    assert beam(b=None) < 0 and b"null" in err() and name in err()
    for n in (0, -1):
        assert beam(n=n) < 0 and b"positive" in err() and name in err(), n
    for n in (limit, 1 << 40):
        assert beam(n=n) < 0 and b"2^31" in err() and name in err(), n
    for plane in ("a", "b"):
        assert beam(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err(), plane
    for L, M in ((0, 2), (2, 256), (251, 2), (255, 2), (2, 255), (2, 0)):
        assert beam(L=L, M=M) < 0 and b"L and M" in err() and name in err(), (L, M)
    assert beam(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
    for off in (4, 8, 12):
        assert beam(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
    assert beam(action=None) < 0 and b"null" in err() and b"action" in err() and name in err()
    assert beam(after_a=fake + 8) < 0 and b"after_a and after_b must be 16-byte aligned" in err() and name in err()
    assert beam(after_b=fake + 4) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
    assert beam(score=fake + 2) < 0 and b"score must be 4-byte aligned" in err() and name in err()
    for gamma in (nan, inf, -inf):
        assert beam(gamma=gamma) < 0 and b"gamma must be finite" in err() and name in err(), gamma
    # depth and width are refused with every optional output left out as well; `plan` has no alignment requirement
    assert beam(depth=0, plan=None, score=None, after_a=None, after_b=None) < 0 and b"depth" in err()
    assert beam(plan=fake + 1, width=65) < 0 and b"width" in err()
    # the checks before depth and width speak first
    assert beam(depth=0, gamma=nan) < 0 and b"gamma" in err()


# ------------------------------------------------------------------------------------------------ 5. the Python surface
def test_python_refusals_of_the_ntuple_beam_need_no_gpu():
    import torch
    nt = T.ntuple
    assert T.NTupleBeamPolicy is nt.NTupleBeamPolicy and "NTupleBeamPolicy" in T.__all__ and "NTupleBeamPolicy" in nt.__all__
    env = _Env(8)
    env._own = lambda *args: T.BatchedTetris._own(env, *args)  # the environment's own check of a caller's buffer
    table = nt.ntuple_table("cpu")
    for depth in (0, 12, -1, 1.5, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="depth"):
            nt.NTupleBeamPolicy(env, table, depth, 4)
    for width in (0, 65, -1, 1.5, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="width"):
            nt.NTupleBeamPolicy(env, table, 3, width)
    for bad in (torch.zeros(nt.NTUPLE_ENTRIES + 1, dtype=torch.int32), torch.zeros(nt.NTUPLE_ENTRIES, dtype=torch.int64),
                torch.zeros(1024, dtype=torch.int32), None):
        with pytest.raises(ValueError, match="table"):
            nt.NTupleBeamPolicy(env, bad, 3, 4)
    with pytest.raises(ValueError, match="gamma"):
        nt.NTupleBeamPolicy(env, table, 3, 4, gamma=float("inf"))
    p = nt.NTupleBeamPolicy(env, table, 11, 64)
    assert (p.env, p.depth, p.width, p.gamma, p.shape) == (env, 11, 64, 0.99, "2x4")
    wide = nt.NTupleBeamPolicy(env, nt.ntuple_table("cpu", "3x3"), 1, 1, gamma=1.0)
    assert (wide.depth, wide.width, wide.gamma, wide.shape) == (1, 1, 1.0, "3x3")
    for kw, what in ((dict(plan=torch.zeros((8, 10), dtype=torch.uint8)), "plan"), (dict(plan=torch.zeros((8, 11), dtype=torch.int32)), "plan"),
                     (dict(score=torch.zeros(9)), "score"), (dict(out=torch.zeros(8, dtype=torch.int32)), "out"),
                     (dict(after=(torch.zeros((8, 4), dtype=torch.int32),)), "after"),
                     (dict(after=(torch.zeros((7, 4), dtype=torch.int32), torch.zeros((7, 4), dtype=torch.int32))), "after")):
        with pytest.raises(ValueError, match=what):
            p.act(**kw)
    learner = nt.NTupleLearner(env)
    with pytest.raises(ValueError, match="depth"):
        learner.evaluate(4, width=8)                           # a width without a depth
    for depth in (0, 12, True, "3"):
        with pytest.raises(ValueError, match="depth"):
            learner.evaluate(4, depth=depth, width=8)
    for width in (0, 65, True, 8.0):
        with pytest.raises(ValueError, match="width"):
            learner.evaluate(4, depth=3, width=width)
    with pytest.raises(ValueError, match="depth"):             # width=None is the interface as it was: depth 3 is refused
        learner.evaluate(4, depth=3)
