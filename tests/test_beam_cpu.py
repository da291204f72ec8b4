"""CPU-side checks of the beam search over the known piece window (include/tpl_learn.h's rule, tpl_placement_beam in
csrc/learn/beam.hip, _learn_lib.beam_select, heuristic.py's BeamPolicy and width=):

  * beam_select against a plain sort-based statement, with ties, +-0, count < W, W = 1 and count = W;
  * every refusal of tpl_placement_beam comes back as a status with the entry's name in the message, without a GPU;
  * the header declares the entry and the two limits, the library exports it, the unit is among the digested sources, and
    placement_beam_kernel is in tools/kernel_resources.sh's output exactly once, without scratch and within 128 VGPRs;
  * the Python refusals need no GPU.
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


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ 1. the selection
def _plain_select(values, width):
    """The rule as the header words it: order the candidates by (value descending, index ascending), -0 and +0 equal; keep the
    first min(width, count); list them by index."""
    def before(i, j):                                          # candidate i is better than candidate j
        return values[i] > values[j] or (values[i] == values[j] and i < j)
    order = []
    for i in range(len(values)):                               # insertion sort under `before`
        at = 0
        while at < len(order) and before(order[at], i):
            at += 1
        order.insert(at, i)
    return sorted(order[:width])


def test_beam_select_is_the_plain_statement_with_ties_zeros_and_short_lists():
    m = _m()
    gen = np.random.default_rng(64)
    cases = [(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], np.float32), w) for w in (1, 2, 3, 5, 6, 7, 64)]   # +-0 tie: index decides
    cases += [(np.array([3.0], np.float32), w) for w in (1, 64)]
    for count in (1, 2, 5, 34, 35, 300, 2176):
        for width in (1, 2, count - 1, count, count + 1, 64):
            if not 1 <= width <= 64:
                continue
            cases.append((gen.integers(-2, 3, count).astype(np.float32), width))               # many ties, at the W-th place too
            cases.append((gen.normal(size=count).astype(np.float32), width))
            z = gen.integers(-1, 2, count).astype(np.float32)
            z[z == 0] = np.where(gen.random(int((z == 0).sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
            cases.append((z, width))
    tied_at_the_edge = 0
    for values, width in cases:
        got = m.beam_select(values, width)
        want = _plain_select(values.tolist(), width)
        assert got.dtype == np.int64 and got.tolist() == want, (values[:10], width, got[:10], want[:10])
        assert len(want) == min(width, values.size) and (np.diff(got) > 0).all()
        if width < values.size:
            edge = np.sort(values)[::-1][width - 1]
            tied_at_the_edge += int((values == edge).sum() > (values[got] == edge).sum())
    assert tied_at_the_edge >= 20                              # a tie at the W-th place was cut by the index, many times
    assert m.beam_select(np.array([-0.0, 0.0], np.float32), 1).tolist() == [0]
    assert m.beam_select(np.array([0.0, -0.0], np.float32), 1).tolist() == [0]
    for bad in (0, 65, -1, True, 1.5):
        with pytest.raises(ValueError, match="width"):
            m.beam_select(np.zeros(4, np.float32), bad)
    with pytest.raises(ValueError, match="values"):
        m.beam_select(np.zeros((2, 2), np.float32), 1)
    with pytest.raises(ValueError, match="values"):
        m.beam_select(np.zeros(0, np.float32), 1)


# ------------------------------------------------------------------------------------------------ 2. arguments
def test_every_refusal_of_the_beam_entry_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    name = b"tpl_placement_beam"

    def beam(a=fake, b=fake, n=4, L=2, M=2, weights=fake, per=2, depth=3, width=4, action=fake, plan=fake, score=fake):
        return lib.tpl_placement_beam(a, b, n, L, M, weights, per, depth, width, action, plan, score, None)

    for depth in (0, 13, -1, 1 << 30, -(1 << 31)):
        assert beam(depth=depth) < 0 and b"depth must be in [1, 12]" in err() and name in err(), depth
    for width in (0, 65, -1, 1 << 30, -(1 << 31)):
        assert beam(width=width) < 0 and b"width must be in [1, 64]" in err() and name in err(), width
    # the inherited ones: tpl_placement_act's list
    limit = -(-(1 << 31) // 40)
    assert beam(a=None) < 0 and b"null" in err() and name in err()
    assert beam(b=None) < 0 and b"null" in err() and name in err()
    for n in (0, -1):
        assert beam(n=n) < 0 and b"positive" in err() and name in err(), n
    for n in (limit, 1 << 40):
        assert beam(n=n) < 0 and b"2^31" in err() and name in err(), n
    for plane in ("a", "b"):
        assert beam(**{plane: fake + 8}) < 0 and b"aligned" in err() and name in err(), plane
    for L, M in ((0, 2), (2, 256), (251, 2), (255, 2), (2, 255)):
        assert beam(L=L, M=M) < 0 and b"L and M" in err() and name in err(), (L, M)
    # the environment's largest game is not refused for its size: the alignment check, which comes after L and M, speaks
    assert beam(L=250, M=254, a=fake + 8) < 0 and b"aligned" in err() and b"L and M" not in err() and name in err()
    assert beam(weights=None) < 0 and b"null" in err() and name in err()
    assert beam(action=None) < 0 and b"null" in err() and name in err()
    assert beam(per=0) < 0 and b"boards_per_member" in err() and name in err()
    assert beam(weights=fake + 4) < 0 and b"weights must be 16-byte aligned" in err() and name in err()
    assert beam(score=fake + 2) < 0 and b"score must be 4-byte aligned" in err() and name in err()
    # a bad depth is refused with the optional outputs left out as well
    assert beam(depth=0, plan=None, score=None) < 0 and b"depth" in err()


# ------------------------------------------------------------------------------------------------ 3. symbols, resources
def test_the_header_declares_the_beam_entry_and_the_library_exports_it():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and "tpl_placement_beam" in declared
    proto = re.search(r"int tpl_placement_beam\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["plane_a", "plane_b", "n", "L", "M", "weights", "boards_per_member",
                                                                     "depth", "width", "action", "plan", "score", "stream"]
    assert re.search(r"#define\s+TPL_BEAM_MAX_DEPTH\s+12\b", text) and re.search(r"#define\s+TPL_BEAM_MAX_WIDTH\s+64\b", text)
    assert (_m().BEAM_MAX_DEPTH, _m().BEAM_MAX_WIDTH) == (12, 64)
    lib = ctypes.CDLL(_m().build_library())
    assert hasattr(lib, "tpl_placement_beam")
    units = [os.path.basename(p) for p in _m()._UNITS]
    assert units[-1] == "heuristic.hip" and "beam.hip" in units
    assert any(p.endswith(os.path.join("learn", "beam.hip")) for p in _m()._sources())
    assert "placement_beam_kernel" in open(os.path.join(os.path.dirname(_m()._UNITS[-1]), "beam.hip")).read()


def test_the_beam_kernel_uses_no_scratch_and_at_most_128_vgprs():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    mine = [r for r in rows if "placement_beam_kernel" in r[-1]]
    assert len(mine) == 1, [r[-1] for r in rows]
    assert mine[0][mine[0].index("scratch") - 1] == "0", mine
    assert int(mine[0][mine[0].index("vgpr") - 1]) <= 128, mine                  # four waves per SIMD
    assert int(mine[0][mine[0].index("lds") - 1]) <= 32 * 1024, mine             # five groups to a CU's 160 KB at the least
    for kernel in ("placement_features_kernel", "placement_act_kernel", "placement_search_kernel"):
        assert len([r for r in rows if kernel in r[-1]]) == 1, kernel             # none of them is part of the new name


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def test_python_refusals_of_depth_and_width_need_no_gpu():
    import torch
    h = T.heuristic
    assert T.BeamPolicy is h.BeamPolicy
    env = _Env(8)
    good = np.zeros(12, np.float32)
    for depth in (0, 13, -1, 1.5, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="depth"):
            h.BeamPolicy(env, good, depth, 4)
        with pytest.raises(ValueError, match="depth"):
            h.evaluate_heuristic(env, good, None, 4, depth=depth, width=4)
        with pytest.raises(ValueError, match="depth"):
            h.tune_heuristic(2, 2, None, depth=depth, width=4)
    for width in (0, 65, -1, 1.5, 8.0, True, "8"):
        with pytest.raises(ValueError, match="width"):
            h.BeamPolicy(env, good, 3, width)
        with pytest.raises(ValueError, match="width"):
            h.evaluate_heuristic(env, good, None, 4, depth=3, width=width)
        with pytest.raises(ValueError, match="width"):
            h.tune_heuristic(2, 2, None, depth=3, width=width)
    p = h.BeamPolicy(env, np.zeros((2, 12)), 12, 64)
    assert (p.env, p.members, p.boards_per_member, p.depth, p.width) == (env, 2, 4, 12, 64)
    assert p.weights.dtype == torch.float32 and tuple(p.weights.shape) == (2, 12)
    p = h.BeamPolicy(env, np.zeros((3, 12)), np.int64(1), np.int32(1), boards_per_member=3)
    assert (p.members, p.boards_per_member, p.depth, p.width) == (3, 3, 1, 1)
    p.set_weights(np.ones((3, 12)))
    assert float(p.weights.sum()) == 36.0
    with pytest.raises(ValueError, match="shape"):
        p.set_weights(np.ones(12))
    with pytest.raises(ValueError, match="finite"):
        h.BeamPolicy(env, np.full(12, np.inf), 3, 4)
    with pytest.raises(ValueError, match="weight rows|members"):
        h.BeamPolicy(env, np.zeros((3, 12)), 3, 4)
    # width=None is the interface as it was: depth 3 is refused, and a beam policy does not pass for a HeuristicPolicy
    with pytest.raises(ValueError, match="depth"):
        h.evaluate_heuristic(env, good, None, 4, depth=3)
    with pytest.raises(ValueError, match="depth"):
        h.tune_heuristic(2, 2, None, depth=3)
    beam, other_width, other_depth = h.BeamPolicy(env, good, 3, 8), h.BeamPolicy(env, good, 3, 4), h.BeamPolicy(env, good, 2, 8)
    plain = h.HeuristicPolicy(env, good, depth=2)
    with pytest.raises(ValueError, match="BeamPolicy"):
        h.evaluate_heuristic(env, good, None, 4, policy=other_depth, depth=2)
    with pytest.raises(ValueError, match="HeuristicPolicy"):
        h.evaluate_heuristic(env, good, None, 4, policy=plain, depth=2, width=8)
    with pytest.raises(ValueError, match="width 4"):
        h.evaluate_heuristic(env, good, None, 4, policy=other_width, depth=3, width=8)
    with pytest.raises(ValueError, match="depth 2"):
        h.evaluate_heuristic(env, good, None, 4, policy=other_depth, depth=3, width=8)
    with pytest.raises(ValueError, match="another environment"):
        h.evaluate_heuristic(_Env(8), good, None, 4, policy=beam, depth=3, width=8)
