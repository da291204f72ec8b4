"""CPU-side checks of the two-ply placement search (include/tpl_learn.h's rule, tpl_placement_search in csrc/learn/heuristic.hip,
_learn_lib.search_choice, heuristic.py's depth=2):

  * the numpy mirror against a plain Python double loop on random small-integer features and weights, where ties occur in both
    plies, and on a case where a fused multiply-add would change the last bit of the score;
  * every refusal of tpl_placement_search comes back as a status with the entry's name in the message, without a GPU;
  * the header declares the entry, the library exports it, and placement_search_kernel is in tools/kernel_resources.sh's output
    exactly once, without scratch and within 128 VGPRs;
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

f32 = np.float32


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ 1. the mirror
def _score(w, phi):
    """w . phi left to right in float32, every product and every sum rounded once, one scalar operation at a time."""
    acc = f32(f32(w[0]) * f32(phi[0]))
    for k in range(1, 12):
        acc = f32(acc + f32(f32(w[k]) * f32(phi[k])))
    return acc


def _double_loop(phi1, done1, distinct1, phi2, distinct2, w):
    """The rule as the header words it, for one board: (action, second, score)."""
    best = None
    for a in range(40):
        if not distinct1[a]:
            continue
        if done1[a]:
            value, second = _score(w, phi1[a]), 255
        else:
            value, second = None, None
            for b in range(40):
                if not distinct2[b]:
                    continue
                s = _score(w, phi2[a, b])
                if value is None or s > value:                 # strict: the lowest b stays; -0 > +0 is false
                    value, second = s, b
        if best is None or value > best[2]:
            best = (a, second, value)
    return best


def test_the_mirror_is_the_plain_double_loop_with_ties_in_both_plies():
    m = _m()
    gen = np.random.default_rng(21)
    K = 48
    phi1 = gen.integers(0, 3, (K, 40, 12))
    phi2 = gen.integers(0, 3, (K, 40, 40, 12))
    done1 = gen.random((K, 40)) < 0.3
    done1[:4] = True                                           # finished boards: every first move is "done", all features zero
    phi1[:4] = 0
    done1[4:6] = False
    distinct1 = gen.random((K, 40)) < 0.5
    distinct1[:, 0] = True
    distinct2 = gen.random((K, 40)) < 0.5
    distinct2[:, 0] = True
    w = (gen.integers(-1, 2, (K, 12)) * (gen.random((K, 12)) < 0.35)).astype(np.float32)       # few features: many ties
    w[6] = 0.0                                                 # every score is +0 or -0 ...
    w[7] = -0.0                                                # ... and here -0: they tie
    for weights, row in ((w, lambda i: w[i]), (w[9], lambda i: w[9])):                     # a row per board; one row for all
        act, sec, score = m.search_choice(phi1, done1, distinct1, phi2, distinct2, weights)
        assert act.dtype == np.uint8 and sec.dtype == np.uint8 and score.dtype == np.float32
        assert act.shape == sec.shape == score.shape == (K,)
        ties1 = ties2 = 0
        for i in range(K):
            a, b, s = _double_loop(phi1[i], done1[i], distinct1[i], phi2[i], distinct2[i], row(i))
            assert (int(act[i]), int(sec[i])) == (a, b), (i, act[i], sec[i], a, b)
            assert score[i] == s, (i, score[i], s)
            assert distinct1[i, a] and (b == 255) == bool(done1[i, a]) and (b == 255 or distinct2[i, b])
            # count the ties that the lowest-index rule decided
            if b != 255:
                s2 = [_score(row(i), phi2[i, a, bb]) for bb in range(40) if distinct2[i, bb]]
                ties2 += sum(1 for x in s2 if x == s) > 1
            v = []
            for aa in range(40):
                if distinct1[i, aa]:
                    one = np.zeros((1, 40), bool)
                    one[0, aa] = True
                    v.append(m.search_choice(phi1[i:i + 1], done1[i:i + 1], one, phi2[i:i + 1], distinct2[i:i + 1], row(i))[2][0])
            ties1 += sum(1 for x in v if x == s) > 1
        assert ties1 >= 10 and ties2 >= 10, (ties1, ties2)
    assert (m.search_choice(phi1, done1, distinct1, phi2, distinct2, w)[0][:4] == 0).all()
    assert (m.search_choice(phi1, done1, distinct1, phi2, distinct2, w)[1][:4] == 255).all()
    # distinct2 per (a, b) is accepted as well
    full = np.broadcast_to(distinct2[:, None, :], (K, 40, 40))
    for x, y in zip(m.search_choice(phi1, done1, distinct1, phi2, full, w), m.search_choice(phi1, done1, distinct1, phi2, distinct2, w)):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        m.search_choice(phi1, done1, distinct1, phi2[:, :39], distinct2, w)
    with pytest.raises(ValueError):
        m.search_choice(phi1, done1[:, :39], distinct1, phi2, distinct2, w)
    with pytest.raises(ValueError):
        m.search_choice(phi1, done1, distinct1, phi2, distinct2, w[:5])


def test_the_second_ply_score_rounds_every_product_and_every_sum_once():
    m = _m()
    # 1 + 0.1f * 9 in the second ply: the fused form ends in another bit (test_heuristic_cpu's case); the other placements
    # sit one unit in the last place above the fused and below the stepwise value, so a fused score would change the choice
    w = np.zeros(12, np.float32)
    w[0], w[1], w[3] = 1.0, 0.1, 1.0
    stepwise = f32(f32(1.0) + f32(f32(0.1) * f32(9.0)))
    fused = f32(np.float64(f32(0.1)) * 9.0 + 1.0)
    assert stepwise.view(np.uint32) != fused.view(np.uint32)
    phi1 = np.zeros((1, 40, 12), np.int64)
    phi2 = np.zeros((1, 40, 40, 12), np.int64)
    phi2[0, 5, 7, 0], phi2[0, 5, 7, 1] = 1, 9                  # psi(5, 7): the case; everything else scores 0
    done1 = np.zeros((1, 40), bool)
    ones = np.ones((1, 40), bool)
    act, sec, score = m.search_choice(phi1, done1, ones, phi2, ones, w)
    assert (int(act[0]), int(sec[0])) == (5, 7) and score[0].view(np.uint32) == stepwise.view(np.uint32)
    # a first move that ends the game takes its one-ply score, and the running sum of both plies' rows is feature 0
    done1[0, 3] = True
    phi1[0, 3, 0] = 4
    act, sec, score = m.search_choice(phi1, done1, ones, phi2, ones, w)
    assert (int(act[0]), int(sec[0]), float(score[0])) == (3, 255, 4.0)
    phi2[0, 2, 9, 0] = 8                                       # n1 + n2 = 8 converts exactly
    act, sec, score = m.search_choice(phi1, done1, ones, phi2, ones, w)
    assert (int(act[0]), int(sec[0]), float(score[0])) == (2, 9, 8.0)


# ------------------------------------------------------------------------------------------------ 2. arguments
def test_every_refusal_of_the_search_entry_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    name = b"tpl_placement_search"

    def search(a=fake, b=fake, n=4, L=2, M=2, weights=fake, per=2, action=fake, second=fake, score=fake):
        return lib.tpl_placement_search(a, b, n, L, M, weights, per, action, second, score, None)

    limit = -(-(1 << 31) // 40)                                # the first n with 40 n >= 2^31
    assert search(a=None) < 0 and b"null" in err() and name in err()
    assert search(b=None) < 0 and b"null" in err() and name in err()
    for n in (0, -1, -(1 << 40)):
        assert search(n=n) < 0 and b"positive" in err() and name in err(), n
    for n in (limit, limit + 1, 1 << 31, 1 << 40, (1 << 63) - 1):
        assert search(n=n) < 0 and b"2^31" in err() and name in err(), n
    for plane in ("a", "b"):
        for off in (4, 8, 1):
            assert search(**{plane: fake + off}) < 0 and b"aligned" in err() and name in err(), (plane, off)
    for L, M in ((0, 2), (256, 2), (2, 0), (2, 256), (-1, -1), (251, 2), (255, 2), (2, 255)):
        assert search(L=L, M=M) < 0 and b"L and M" in err() and name in err(), (L, M)
    # the environment's largest game is not refused for its size: the alignment check, which comes after L and M, speaks
    assert search(L=250, M=254, a=fake + 8) < 0 and b"aligned" in err() and b"L and M" not in err() and name in err()
    assert search(weights=None) < 0 and b"null" in err() and name in err()
    assert search(action=None) < 0 and b"null" in err() and name in err()
    for per in (0, -1, -(1 << 40)):
        assert search(per=per) < 0 and b"boards_per_member" in err() and name in err(), per
    for off in (1, 4, 8):
        assert search(weights=fake + off) < 0 and b"weights must be 16-byte aligned" in err() and name in err(), off
    for off in (1, 2):
        assert search(score=fake + off) < 0 and b"score must be 4-byte aligned" in err() and name in err(), off


# ------------------------------------------------------------------------------------------------ 3. symbols, resources
def test_the_header_declares_the_search_entry_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert "tpl_placement_search" in declared and "tpl_placement_search" in _m().LEARN_SYMBOLS
    proto = re.search(r"int tpl_placement_search\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["plane_a", "plane_b", "n", "L", "M", "weights",
                                                                     "boards_per_member", "action", "second", "score", "stream"]
    lib = ctypes.CDLL(_m().build_library())
    assert hasattr(lib, "tpl_placement_search")
    assert _m()._UNITS[-1].endswith("heuristic.hip")
    assert "placement_search_kernel" in open(_m()._UNITS[-1]).read()


def test_the_search_kernel_uses_no_scratch_and_at_most_128_vgprs():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    mine = [r for r in rows if "placement_search_kernel" in r[-1]]
    assert len(mine) == 1, [r[-1] for r in rows]
    assert mine[0][mine[0].index("scratch") - 1] == "0", mine
    assert int(mine[0][mine[0].index("vgpr") - 1]) <= 128, mine                  # four waves per SIMD
    for kernel in ("placement_features_kernel", "placement_act_kernel"):         # neither name is part of the new one
        assert len([r for r in rows if kernel in r[-1]]) == 1, kernel


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def test_python_refusals_of_the_depth_need_no_gpu():
    import torch
    h = T.heuristic
    env = _Env(8)
    good = np.zeros(12, np.float32)
    for depth in (0, 3, 1.5, True, -1, None, "2"):
        with pytest.raises(ValueError, match="depth"):
            h.HeuristicPolicy(env, good, depth=depth)
        with pytest.raises(ValueError, match="depth"):
            h.evaluate_heuristic(env, good, None, 4, depth=depth)
        with pytest.raises(ValueError, match="depth"):
            h.tune_heuristic(2, 2, None, depth=depth)
    one, two = h.HeuristicPolicy(env, good), h.HeuristicPolicy(env, good, None, 2)
    assert one.depth == 1 and two.depth == 2 and h.HeuristicPolicy(env, good, depth=1).depth == 1
    with pytest.raises(ValueError, match="second"):
        one.act(second=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="second"):
        one.act(out=torch.zeros(8, dtype=torch.uint8), second=torch.zeros(8, dtype=torch.uint8))
    # a policy of another depth
    with pytest.raises(ValueError, match="depth 2"):
        h.evaluate_heuristic(env, good, None, 4, policy=two)
    with pytest.raises(ValueError, match="depth 1"):
        h.evaluate_heuristic(env, good, None, 4, policy=one, depth=2)
    with pytest.raises(ValueError, match="depth 2"):
        h.evaluate_heuristic(env, good, None, 4, policy=two, depth=1)
