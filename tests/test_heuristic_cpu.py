"""CPU-side checks of the placement features and the linear placement policy (include/tpl_learn.h's rule, csrc/learn/heuristic.hip,
_learn_lib.board_features / placement_score, heuristic.py):

  * the numpy mirror on hand-written boards whose nine board features were worked out by hand, and its score rule on weights
    where a fused multiply-add would change the last bit;
  * every refusal of tpl_placement_features and tpl_placement_act comes back as a status with a message, without a GPU;
  * the header declares what LEARN_SYMBOLS lists and the library exports both entry points; both kernels are in
    tools/kernel_resources.sh's output without scratch, and the code object is gfx950 only;
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

FULL = 0x3FF
BOARD = ("holes", "aggregate_height", "max_height", "bumpiness", "row_transitions", "column_transitions", "wells",
         "rows_with_holes", "hole_depth")


def _m():
    return T._learn_lib


def _columns(heights):
    """Solid columns of the given heights as row masks."""
    rows = np.zeros(20, np.uint16)
    for x, h in enumerate(heights):
        for k in range(h):
            rows[19 - k] |= np.uint16(1 << x)
    return rows


# ------------------------------------------------------------------------------------------------ 1. the mirror
def _hand_written():
    empty = np.zeros(20, np.uint16)
    one_short = empty.copy()
    one_short[19] = FULL & ~(1 << 4)                           # the bottom row full but for column 4
    overhang = empty.copy()
    overhang[17] = 1 << 3                                      # one cell in column 3 with rows 18 and 19 empty below it
    wells = _columns([0, 3, 3, 3, 4, 0, 2, 2, 2, 2])           # an edge well of depth 3 (column 0), a centre well of depth 2 (5)
    two_holes = empty.copy()
    for r in (14, 16, 17, 19):                                 # column 2: filled, hole, filled, filled, hole, filled
        two_holes[r] = 1 << 2
    #                         holes  agg  max  bump  rowT  colT  wells  hole rows  depth
    return [("empty", empty, (0, 0, 0, 0, 40, 10, 0, 0, 0)),
            # nine columns of height 1 and a gap: two steps, the gap is a well of depth 1, every row still has two transitions
            ("one full-but-one row", one_short, (0, 9, 1, 2, 40, 10, 1, 0, 0)),
            # the cell's row has four transitions; its column: above / cell, cell / hole, and the empty bottom cell on the floor
            ("a single overhang", overhang, (2, 3, 3, 6, 42, 12, 0, 2, 1)),
            # edge well 3 (3 * 4 / 2 = 6) against the wall of height 20, centre well min(4, 2) = 2 (3); rows 16..19 have 4 each
            ("an edge well and a centre well", wells, (0, 21, 4, 10, 48, 10, 9, 0, 0)),
            # the column: 13/14, 14/15, 15/16, 17/18, 18/19 differ (5) + nine empty columns; one filled cell above the upper hole
            ("two separated holes", two_holes, (2, 6, 6, 12, 48, 14, 0, 2, 1))]


def test_the_mirror_on_hand_written_boards():
    m = _m()
    assert m.NUM_FEATURES == 12 and len(m.FEATURE_NAMES) == 12 and tuple(m.FEATURE_NAMES[3:]) == BOARD
    assert tuple(m.FEATURE_NAMES[:3]) == ("cleared", "won", "lost")
    cases = _hand_written()
    got = m.board_features(np.stack([rows for _, rows, _ in cases]))
    assert got.shape == (len(cases), 9)
    for (name, rows, want), g in zip(cases, got):
        assert tuple(g.tolist()) == want, (name, dict(zip(BOARD, g.tolist())))
        assert tuple(m.board_features(rows)[0].tolist()) == want               # a single board: [20]
    # the left-right mirror image has the same features (every one of them is symmetric)
    for name, rows, want in cases:
        flipped = np.array([sum(((int(v) >> x) & 1) << (9 - x) for x in range(10)) for v in rows], np.uint16)
        assert tuple(m.board_features(flipped)[0].tolist()) == want, name
    # a full-height alternating board: the bound of the largest feature
    comb = _columns([20, 0] * 5)
    f = dict(zip(BOARD, m.board_features(comb)[0].tolist()))
    assert f["wells"] == 5 * 210 and f["aggregate_height"] == 100 and f["max_height"] == 20 and f["bumpiness"] == 180
    assert max(f.values()) < 1 << 15
    with pytest.raises(ValueError):
        m.board_features(np.zeros((3, 19), np.uint16))


def test_the_score_rule_rounds_every_product_and_every_sum_once():
    m = _m()
    f32 = np.float32
    # 1 + 0.1f * 9: the product is not a float32, so the fused form (one rounding of the exact sum) ends in another bit
    w = np.zeros(12, np.float32)
    w[0], w[1] = 1.0, 0.1
    phi = np.zeros(12, np.int64)
    phi[0], phi[1], phi[4] = 1, 9, 3                            # phi_4 meets a zero weight: adding 0 changes nothing
    got = m.placement_score(phi, w)
    assert got.dtype == np.float32 and got.shape == ()
    stepwise = f32(f32(f32(1.0) * f32(1.0)) + f32(f32(0.1) * f32(9.0)))
    assert got.view(np.uint32) == stepwise.view(np.uint32)
    fused = f32(np.float64(f32(0.1)) * 9.0 + 1.0)              # fma(w1, phi1, s): exact in float64, rounded once
    assert fused.view(np.uint32) != got.view(np.uint32) and abs(float(fused) - float(got)) < 2e-7
    # left to right: the order of the sums is the index order
    w2 = np.zeros(12, np.float32)
    w2[0], w2[1], w2[2] = 1e8, -1e8, 1.0
    ones = np.ones(12, np.int64)
    assert m.placement_score(ones, w2) == f32(1.0)
    w2[0], w2[1], w2[2] = 1.0, 1e8, -1e8
    assert m.placement_score(ones, w2) == f32(0.0)
    # broadcasting: [K, 40, 12] features against [K, 1, 12] weights
    gen = np.random.default_rng(3)
    feats = gen.integers(0, 200, (5, 40, 12))
    ws = gen.normal(size=(5, 1, 12)).astype(np.float32)
    s = m.placement_score(feats, ws)
    assert s.shape == (5, 40) and s.dtype == np.float32
    for i in (0, 4):
        for a in (0, 39):
            acc = ws[i, 0, 0] * f32(feats[i, a, 0])
            for k in range(1, 12):
                acc = f32(acc + f32(ws[i, 0, k] * f32(feats[i, a, k])))
            assert s[i, a].view(np.uint32) == acc.view(np.uint32)
    # the reward weights: the score is the afterstate reward's two operations
    r = m.placement_score(np.array([3, 1, 0] + [7] * 9), np.array([0.1, 0.5, -0.25] + [0.0] * 9, np.float32))
    assert r.view(np.uint32) == f32(f32(f32(0.1) * f32(3.0)) + f32(0.5)).view(np.uint32)
    with pytest.raises(ValueError):
        m.placement_score(np.zeros(11), np.zeros(12))


# ------------------------------------------------------------------------------------------------ 2. arguments
def test_every_refusal_of_both_entry_points_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused

    def features(a=fake, b=fake, n=4, L=2, M=2, features=fake, canonical=fake):
        return lib.tpl_placement_features(a, b, n, L, M, features, canonical, None)

    def act(a=fake, b=fake, n=4, L=2, M=2, weights=fake, per=2, action=fake, score=fake):
        return lib.tpl_placement_act(a, b, n, L, M, weights, per, action, score, None)

    limit = -(-(1 << 31) // 40)                                # the first n with 40 n >= 2^31
    for call, name in ((features, b"tpl_placement_features"), (act, b"tpl_placement_act")):
        assert call(a=None) < 0 and b"null" in err() and name in err()
        assert call(b=None) < 0 and b"null" in err()
        for n in (0, -1, -(1 << 40)):
            assert call(n=n) < 0 and b"positive" in err(), n
        for n in (limit, limit + 1, 1 << 31, 1 << 40, (1 << 63) - 1):
            assert call(n=n) < 0 and b"2^31" in err(), n
        for plane in ("a", "b"):
            for off in (4, 8, 1):
                assert call(**{plane: fake + off}) < 0 and b"aligned" in err(), (plane, off)
        for L, M in ((0, 2), (256, 2), (2, 0), (2, 256), (-1, -1), (251, 2), (255, 2), (2, 255)):
            assert call(L=L, M=M) < 0 and b"L and M" in err() and name in err(), (L, M)
        # the environment's largest game is not refused for its size: the alignment check, which comes after L and M, speaks
        assert call(L=250, M=254, a=fake + 8) < 0 and b"aligned" in err() and b"L and M" not in err()
        assert name in err()
    assert features(features=None) < 0 and b"null" in err()
    for off in (1, 2, 4):
        assert features(features=fake + off) < 0 and b"8-byte aligned" in err(), off
    assert act(weights=None) < 0 and b"null" in err()
    assert act(action=None) < 0 and b"null" in err()
    for per in (0, -1, -(1 << 40)):
        assert act(per=per) < 0 and b"boards_per_member" in err(), per
    for off in (1, 4, 8):
        assert act(weights=fake + off) < 0 and b"weights must be 16-byte aligned" in err(), off
    for off in (1, 2):
        assert act(score=fake + off) < 0 and b"score must be 4-byte aligned" in err(), off


# ------------------------------------------------------------------------------------------------ 3. symbols, resources
def test_the_header_declares_the_two_entry_points_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    assert re.search(r"#define TPL_NUM_FEATURES 12\b", text)
    for name in _m().FEATURE_NAMES:                            # the table is stated where the rule is
        assert re.search(r"\b%s\b" % name, text), name
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text)))
    assert sorted(_m().LEARN_SYMBOLS) == declared
    assert "tpl_placement_features" in declared and "tpl_placement_act" in declared
    lib = ctypes.CDLL(_m().build_library())
    for name in ("tpl_placement_features", "tpl_placement_act"):
        assert hasattr(lib, name), name
    assert any(p.endswith(os.path.join("learn", "heuristic.hip")) for p in _m()._sources())
    assert _m()._UNITS[-1].endswith("heuristic.hip")


def test_the_two_kernels_use_no_scratch_and_target_gfx950_only():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    for kernel in ("placement_features_kernel", "placement_act_kernel"):
        mine = [r for r in rows if kernel in r[-1]]
        assert len(mine) == 1, [r[-1] for r in rows]
        assert mine[0][mine[0].index("scratch") - 1] == "0", mine
        assert int(mine[0][mine[0].index("vgpr") - 1]) <= 64, mine               # eight waves per SIMD
    blob = open(path, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx942", b"gfx90a", b"sm_"):
        assert other not in blob


# ------------------------------------------------------------------------------------------------ 4. the Python surface
class _Env:
    """What the heuristic module reads of an environment before it touches the device."""

    def __init__(self, n, reward=(0.0, 1.0, 0.0), auto_reset=True):
        import torch
        self.L, self.M, self.num_envs, self.reward_params, self.device = 5, 20, n, reward, torch.device("cpu")
        self.auto_reset = auto_reset


def test_python_refusals_need_no_gpu():
    import torch
    h = T.heuristic
    assert T.HeuristicPolicy is h.HeuristicPolicy and T.placement_features is h.placement_features
    assert T.evaluate_heuristic is h.evaluate_heuristic and T.tune_heuristic is h.tune_heuristic
    assert h.FEATURE_NAMES is _m().FEATURE_NAMES
    env = _Env(8)
    good = np.zeros(12, np.float32)
    for bad in (np.nan, np.inf, -np.inf, 1e39):                # 1e39 is finite in float64, not in float32
        w = good.astype(np.float64)
        w[5] = bad
        with pytest.raises(ValueError, match="finite"):
            h.HeuristicPolicy(env, w)
        with pytest.raises(ValueError, match="finite"):
            h.HeuristicPolicy(env, torch.from_numpy(np.stack([good.astype(np.float64), w])), 4)
    for shape in ((11,), (13,), (2, 11), (0, 12), (2, 2, 12), ()):
        with pytest.raises(ValueError, match="shape"):
            h.HeuristicPolicy(env, np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="numbers"):
        h.HeuristicPolicy(env, np.array(["a"] * 12))
    # rows against members
    with pytest.raises(ValueError, match="split evenly"):
        h.HeuristicPolicy(env, np.zeros((3, 12), np.float32))
    for per in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="positive integer"):
            h.HeuristicPolicy(env, np.zeros((2, 12), np.float32), per)
    for rows, per in ((2, 8), (2, 3), (3, 4), (1, 7)):         # ceil(8 / per) != rows
        with pytest.raises(ValueError, match="members"):
            h.HeuristicPolicy(env, np.zeros((rows, 12), np.float32), per)
    # what is accepted, on the host side: lists, integers, a short last member
    for w, per, members in ([0] * 12, None, 1), (np.zeros((3, 12)), 3, 3), (torch.zeros(4, 12), None, 4), (good, 8, 1):
        p = h.HeuristicPolicy(env, w, per)
        assert p.members == members and p.weights.dtype == torch.float32 and tuple(p.weights.shape) == (members, 12)
    assert h.HeuristicPolicy(env, np.zeros((3, 12)), 3).boards_per_member == 3
    p = h.HeuristicPolicy(env, np.zeros((2, 12)))
    with pytest.raises(ValueError, match="keep their shape"):
        p.set_weights(np.zeros(12))
    with pytest.raises(ValueError, match="finite"):
        p.set_weights(np.full((2, 12), np.nan))
    # evaluate_heuristic: the reward parameters that make the summed reward the win count
    for reward in ((1.0, 0.0, 0.0), (0.0, 1.0, -1.0), (0.1, 1.0, 0.0)):
        with pytest.raises(ValueError, match=r"\(0, 1, 0\)"):
            h.evaluate_heuristic(_Env(8, reward), good, None, 4)
    with pytest.raises(ValueError, match="auto-reset"):
        h.evaluate_heuristic(_Env(8, auto_reset=False), good, None, 4)
    for steps in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="steps"):
            h.evaluate_heuristic(env, good, None, steps)
    with pytest.raises(ValueError, match="finite"):
        h.evaluate_heuristic(env, np.full(12, np.inf), None, 4)
    # placement_features: the argument handling of afterstates()
    planes = torch.zeros((4, 4), dtype=torch.int32)
    for a, b in ((planes, None), (None, planes)):
        with pytest.raises(ValueError, match="go together"):
            h.placement_features(env, a, b)
    for t in (torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int64), np.zeros((4, 4), np.int32)):
        with pytest.raises(ValueError, match=r"int32 \[K, 4\]"):
            h.placement_features(env, t, planes)
    with pytest.raises(ValueError, match="equal shape"):
        h.placement_features(env, planes, torch.zeros((5, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="1 .."):
        h.placement_features(env, planes[:0], planes[:0])
    # tune_heuristic refuses before it builds an environment
    for kw in (dict(population=0), dict(boards_per_member=0), dict(generations=0), dict(elite_frac=0.0), dict(elite_frac=1.5),
               dict(init_std=0.0), dict(noise=-1.0), dict(init_std=float("nan"))):
        with pytest.raises(ValueError):
            h.tune_heuristic(2, 2, None, **kw)
