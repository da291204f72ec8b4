"""CPU-side checks of the n-tuple afterstate value function (include/tpl_learn.h's rule, csrc/learn/ntuple.hip, the numpy mirror
in _learn_lib and ntuple.py):

  * pinned hand cases of the mirror: the empty board, one cell in a corner, one cell in the middle, a finished state;
  * the header declares the three entries and the table size, the library exports them, the unit is among the digested sources,
    and each of the three kernels is in tools/kernel_resources.sh's output exactly once, without scratch and within 128 VGPRs;
  * every refusal of the three entries comes back as a status with the entry's name in the message, without a GPU, and the
    Python surface refuses a wrong table and an epsilon outside [0, 1];
  * the mirror's update does not depend on the order of its inputs, and the exploration index is uniform over the placements.
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

ENTRIES = 8 * 153 * 256 + 1024
COUNTER_BASE = 8 * 153 * 256


def _m():
    return T._learn_lib


def _random_table(gen, span=1 << 20):
    return gen.integers(-span, span + 1, ENTRIES).astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1. hand cases
def test_the_mirror_on_boards_small_enough_to_do_by_hand():
    m = _m()
    assert (m.NTUPLE_ENTRIES, m.NTUPLE_COUNTER_BASE) == (ENTRIES, COUNTER_BASE) == (314368, 313344)
    gen = np.random.default_rng(153)
    table = _random_table(gen)
    L, M = 10, 40
    empty = np.zeros(20, np.uint16)
    # an empty board has no tuple: V is the counter entry alone
    for piece, lines, moves, k in ((0, 0, 0, 64 * 10 + 40), (7, 3, 39, 64 * 7 + 1), (3, 10, 40, 0), (3, 12, 45, 0)):
        index, used = m.ntuple_indices(empty, piece, L, M, lines, moves)
        assert index.shape == (1, 154) and used.shape == (1, 154)
        assert not used[0, :153].any() and used[0, 153] and index[0, 153] == COUNTER_BASE + k
        v = m.ntuple_value(table, empty, piece, L, M, lines, moves, 0)
        assert v.dtype == np.float32 and v[0] == np.float32(table[COUNTER_BASE + k]) * np.float32(2.0 ** -16)
    # the counter's clamps: more than 15 lines or 63 moves left read the last entry of their axis
    index, _ = m.ntuple_indices(empty, 0, 250, 254, 0, 0)
    assert index[0, 153] == COUNTER_BASE + 64 * 15 + 63
    # one cell at row 19, column 0: tuple t = 16 (x = 0, y = 16) alone, bit 3 of its low nibble
    rows = empty.copy()
    rows[19] = 1
    index, used = m.ntuple_indices(rows, 2, L, M, 1, 2)
    assert np.flatnonzero(used[0, :153]).tolist() == [16] and index[0, 16] == (2 * 153 + 16) * 256 + 8
    want = int(table[(2 * 153 + 16) * 256 + 8]) + int(table[COUNTER_BASE + 64 * 9 + 38])
    assert m.ntuple_value(table, rows, 2, L, M, 1, 2, 0)[0] == np.float32(want) * np.float32(2.0 ** -16)
    # one cell at row 10, column 5: x = 4 sees it in its high nibble, x = 5 in its low one, each at y = 7..10
    rows = empty.copy()
    rows[10] = 1 << 5
    index, used = m.ntuple_indices(rows, 5, L, M, 0, 0)
    assert np.flatnonzero(used[0, :153]).tolist() == [17 * 4 + y for y in (7, 8, 9, 10)] + [17 * 5 + y for y in (7, 8, 9, 10)]
    for y in (7, 8, 9, 10):
        bit = 10 - y                                           # the cell's row within the window
        assert index[0, 17 * 4 + y] == (5 * 153 + 17 * 4 + y) * 256 + (1 << (4 + bit))
        assert index[0, 17 * 5 + y] == (5 * 153 + 17 * 5 + y) * 256 + (1 << bit)
    # a finished state is worth nothing, whatever is on it
    full = np.full(20, 0x3FF, np.uint16)
    for state in (1, 2, 3):
        assert m.ntuple_value(table, full, 1, L, M, 0, 0, state)[0] == 0.0
    assert m.ntuple_value(table, full, 1, L, M, 0, 0, 0)[0] != 0.0
    _, used = m.ntuple_indices(full, 1, L, M, 0, 0)
    assert used.all()
    # the sum is exact and rounded once: 154 entries of 2^30 + 1 are not a float32, and not what float32 additions give
    big = np.full(ENTRIES, (1 << 30) + 1, np.int32)
    assert m.ntuple_value(big, full, 1, L, M, 0, 0, 0)[0] == np.float32(154 * ((1 << 30) + 1)) * np.float32(2.0 ** -16)
    # several states at once, a refused piece, a refused table
    v = m.ntuple_value(table, np.stack([empty, rows, full]), [0, 5, 1], L, M, [0, 0, 0], 0, [0, 0, 2])
    assert v.shape == (3,) and v[2] == 0.0 and v[0] == np.float32(table[COUNTER_BASE + 64 * 10 + 40]) * np.float32(2.0 ** -16)
    with pytest.raises(ValueError, match="piece"):
        m.ntuple_indices(empty, 8, L, M, 0, 0)
    with pytest.raises(ValueError, match="rows"):
        m.ntuple_indices(np.zeros((2, 19), np.uint16), 0, L, M, 0, 0)
    for bad in (table.astype(np.int64), table[:-1], table.tolist()):
        with pytest.raises(ValueError, match="table"):
            m.ntuple_value(bad, empty, 0, L, M, 0, 0, 0)


def test_the_update_step_rounds_once_clamps_and_drops_a_nan():
    m = _m()
    e = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.4999, np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0], np.float32)
    assert m.ntuple_steps(e, 1.0).tolist() == [0, 2, 2, 0, -2, 0, 0, 1 << 24, -(1 << 24), 1 << 24, -(1 << 24), 0, 0]   # half to even
    assert m.ntuple_steps(np.array([np.inf, 1.0], np.float32), 0.0).tolist() == [0, 0]           # 0 * inf is a NaN
    # the product is a float32 product: 0.1f * 3 is not the float64 0.3
    assert m.ntuple_steps(np.array([3.0], np.float32), 0.1 * (1 << 24))[0] == int(np.rint(np.float32(0.1 * (1 << 24)) * np.float32(3.0)))


# ------------------------------------------------------------------------------------------------ 2. header and build
def test_the_header_declares_the_entries_and_the_library_exports_them():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and {"tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_update"} <= declared
    names = lambda entry: [a.split()[-1].lstrip("*") for a in re.search(rf"int {entry}\((.*?)\);", text, flags=re.S).group(1).split(",")]
    assert names("tpl_ntuple_value") == ["plane_a", "plane_b", "n", "L", "M", "table", "value", "stream"]
    assert names("tpl_ntuple_act") == ["plane_a", "plane_b", "n", "L", "M", "r_line", "r_win", "r_lose", "gamma", "table", "epsilon",
                                       "seed", "step", "action", "score", "after_a", "after_b", "value", "stream"]
    assert names("tpl_ntuple_update") == ["plane_a", "plane_b", "n", "L", "M", "table", "error", "rate", "stream"]
    assert re.search(r"#define\s+TPL_NTUPLE_ENTRIES\s+314368\b", text) and _m().NTUPLE_ENTRIES == 314368
    lib = ctypes.CDLL(_m().build_library())
    for entry in ("tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_update"):
        assert hasattr(lib, entry), entry
    units = [os.path.basename(p) for p in _m()._UNITS]
    assert units[-1] == "heuristic.hip" and "ntuple.hip" in units
    assert any(p.endswith(os.path.join("learn", "ntuple.hip")) for p in _m()._sources())
    assert T.NTuplePolicy is T.ntuple.NTuplePolicy and T.NTupleLearner is T.ntuple.NTupleLearner
    assert T.ntuple_table is T.ntuple.ntuple_table and T.ntuple_value is T.ntuple.ntuple_value


def test_the_three_kernels_use_no_scratch_and_at_most_128_vgprs():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    # tpl_ntuple_update launches ntuple_trace_kernel<false>: the one update kernel, at age 0 of a ring of one slot
    for kernel in ("ntuple_value_kernel", "ntuple_act_kernel", "ntuple_trace_kernelILb0"):
        mine = [r for r in rows if kernel in r[-1]]
        assert len(mine) == 1, (kernel, [r[-1] for r in rows])
        assert mine[0][mine[0].index("scratch") - 1] == "0", mine
        assert int(mine[0][mine[0].index("vgpr") - 1]) <= 128, mine


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_every_refusal_of_the_three_entries_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")

    def value(a=fake, b=fake, n=4, L=2, M=2, table=fake, value=fake):
        return lib.tpl_ntuple_value(a, b, n, L, M, table, value, None)

    def act(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, score=fake, after_a=fake, after_b=fake,
            value=fake):
        return lib.tpl_ntuple_act(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, score, after_a, after_b, value, None)

    def update(a=fake, b=fake, n=4, L=2, M=2, table=fake, error=fake, rate=1.0):
        return lib.tpl_ntuple_update(a, b, n, L, M, table, error, rate, None)

    limit = -(-(1 << 31) // 40)
    for entry, name in ((value, b"tpl_ntuple_value"), (act, b"tpl_ntuple_act"), (update, b"tpl_ntuple_update")):
        # check_planes' list, worded as the placement entries word it
        assert entry(a=None) < 0 and b"null" in err() and name in err()
        assert entry(b=None) < 0 and b"null" in err() and name in err()
        for n in (0, -1):
            assert entry(n=n) < 0 and b"positive" in err() and name in err(), n
        for n in (limit, 1 << 40):
            assert entry(n=n) < 0 and b"2^31" in err() and name in err(), n
        for plane in ("a", "b"):
            assert entry(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err(), plane
        for L, M in ((0, 2), (2, 256), (251, 2), (255, 2), (2, 255), (2, 0)):
            assert entry(L=L, M=M) < 0 and b"L and M" in err() and name in err(), (L, M)
        assert entry(L=250, M=254, a=fake + 8) < 0 and b"aligned" in err() and b"L and M" not in err() and name in err()
        # the table
        assert entry(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
        for off in (4, 8, 12):
            assert entry(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
    assert value(value=None) < 0 and b"null" in err() and b"value" in err()
    assert value(value=fake + 2) < 0 and b"value must be 4-byte aligned" in err()
    assert act(action=None) < 0 and b"null" in err() and b"action" in err()
    assert act(after_a=None) < 0 and b"go together" in err() and b"tpl_ntuple_act" in err()
    assert act(after_b=None) < 0 and b"go together" in err()
    assert act(after_a=fake + 8) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
    assert act(after_b=fake + 4) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
    assert act(score=fake + 2) < 0 and b"4-byte aligned" in err()
    assert act(value=fake + 1) < 0 and b"4-byte aligned" in err()
    for epsilon in (-0.001, 1.001, -1.0, 2.0, nan, inf, -inf):
        assert act(epsilon=epsilon) < 0 and b"epsilon must be in [0, 1]" in err() and b"tpl_ntuple_act" in err(), epsilon
    for gamma in (nan, inf, -inf):
        assert act(gamma=gamma) < 0 and b"gamma must be finite" in err(), gamma
    # a bad epsilon is refused with every optional output left out as well
    assert act(epsilon=2.0, score=None, after_a=None, after_b=None, value=None) < 0 and b"epsilon" in err()
    assert update(error=None) < 0 and b"null" in err() and b"error" in err()
    assert update(error=fake + 2) < 0 and b"error must be 4-byte aligned" in err()
    for rate in (nan, inf, -inf):
        assert update(rate=rate) < 0 and b"rate must be finite" in err() and b"tpl_ntuple_update" in err(), rate


def test_python_refusals_need_no_gpu():
    import torch
    nt = T.ntuple
    env = _Env(8)
    good = nt.ntuple_table("cpu")
    assert good.dtype == torch.int32 and tuple(good.shape) == (ENTRIES,) and int(good.abs().sum()) == 0
    p = nt.NTuplePolicy(env, good)
    assert (p.env, p.table, p.gamma, p.epsilon, p.seed, p.step) == (env, good, 0.99, 0.0, 0, 0) and p.table is good
    p = nt.NTuplePolicy(env, good, gamma=1, epsilon=1, seed=7)
    assert (p.gamma, p.epsilon, p.seed) == (1.0, 1.0, 7)
    wrong = (good.to(torch.int64), good.to(torch.float32), good[:-1], torch.zeros(ENTRIES + 1, dtype=torch.int32),
             good.view(8, -1), good.numpy(), torch.zeros(ENTRIES, dtype=torch.int32, device="meta"), None,
             torch.zeros(2 * ENTRIES, dtype=torch.int32)[::2])
    for table in wrong:
        with pytest.raises(ValueError, match="table"):
            nt.NTuplePolicy(env, table)
        with pytest.raises(ValueError, match="table"):
            nt.ntuple_value(env, table)
    planes = (torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 4), dtype=torch.int32))
    for table in wrong:
        with pytest.raises(ValueError, match="table"):
            nt.ntuple_value(planes, table, 5, 20)
    with pytest.raises(ValueError, match="L and M"):
        nt.ntuple_value(planes, good)
    with pytest.raises(ValueError, match="L and M"):
        nt.ntuple_value(env, good, L=5, M=20)
    for bad in ((planes[0],), (planes[0], planes[1][:2]), (planes[0].to(torch.int64), planes[1]), planes[0], (planes[0].view(-1), planes[1])):
        with pytest.raises(ValueError, match="source"):
            nt.ntuple_value(bad, good, 5, 20)
    for epsilon in (-0.1, 1.5, float("nan"), float("inf"), True, None, "0.1"):
        with pytest.raises(ValueError, match="epsilon"):
            nt.NTuplePolicy(env, good, epsilon=epsilon)
        with pytest.raises(ValueError, match="epsilon"):
            nt.NTupleLearner(env, epsilon=epsilon)
    for gamma in (float("nan"), float("inf"), None, True):
        with pytest.raises(ValueError, match="gamma"):
            nt.NTuplePolicy(env, good, gamma=gamma)
        with pytest.raises(ValueError, match="gamma"):
            nt.NTupleLearner(env, gamma=gamma)
    for rate in (float("nan"), float("-inf"), None):
        with pytest.raises(ValueError, match="rate"):
            nt.NTupleLearner(env, rate=rate)
    for seed in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            nt.NTuplePolicy(env, good, seed=seed)
    with pytest.raises(ValueError, match="auto-reset"):
        nt.NTupleLearner(_Env(8, auto_reset=False))
    with pytest.raises(ValueError, match="boards"):
        nt.NTuplePolicy(_Env(0), good)
    learner = nt.NTupleLearner(env, gamma=0.9, rate=4, epsilon=0.25, seed=3)
    assert learner.table.dtype == torch.int32 and tuple(learner.table.shape) == (ENTRIES,) and learner.steps == 0
    assert learner.policy.table is learner.table and learner.greedy.table is learner.table
    assert (learner.policy.epsilon, learner.greedy.epsilon, learner.policy.gamma, learner.rate) == (0.25, 0.0, 0.9, 4.0)
    # nothing is kept before the first step: the kept afterstates are finished states, which the update skips
    import learn_ref as R
    kept = R.decode_state(learner._kept[0].numpy(), learner._kept[1].numpy())
    assert (kept["state"] != 0).all() and kept["rows"].sum() == 0
    for steps in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            learner.train(steps)
    with pytest.raises(ValueError, match="steps"):
        learner.evaluate(0)


# ------------------------------------------------------------------------------------------------ 4. determinism, exploration
def test_the_mirror_update_does_not_depend_on_the_order_of_its_inputs():
    m = _m()
    gen = np.random.default_rng(17)
    k, L, M = 300, 10, 40
    rows = np.where(gen.random((k, 20, 1)) < 0.5, gen.integers(0, 1 << 10, (k, 20, 1)), 0).astype(np.uint16)[:, :, 0]
    rows[:40] = rows[0]                                        # forty copies of one board: every add of theirs collides
    piece, lines, moves = gen.integers(0, 8, k), gen.integers(0, 12, k), gen.integers(0, 45, k)
    piece[:40], lines[:40], moves[:40] = piece[0], lines[0], moves[0]
    state = np.where(gen.random(k) < 0.2, gen.integers(1, 4, k), 0)
    state[:40] = 0
    error = gen.normal(size=k).astype(np.float32)
    error[gen.integers(0, k, 10)] = np.nan
    start = gen.integers(-(1 << 31), 1 << 31, ENTRIES).astype(np.int32)          # the whole range: some adds wrap
    start[::3] = np.int32((1 << 31) - 1)
    first = m.ntuple_update(start.copy(), rows, piece, L, M, lines, moves, state, error, 2000.0)
    assert first is not start and (first != start).sum() > 1000
    for seed in range(3):
        o = np.random.default_rng(seed).permutation(k)
        again = m.ntuple_update(start.copy(), rows[o], piece[o], L, M, lines[o], moves[o], state[o], error[o], 2000.0)
        assert np.array_equal(again, first), seed
    # one state at a time is the same table, and the states that do not run, the NaNs and the empty pattern add nothing
    single = start.copy()
    for i in range(k):
        m.ntuple_update(single, rows[i], piece[i], L, M, lines[i], moves[i], state[i], error[i:i + 1], 2000.0)
    assert np.array_equal(single, first)
    live = (state == 0) & ~np.isnan(error)
    only = m.ntuple_update(start.copy(), rows[live], piece[live], L, M, lines[live], moves[live], 0, error[live], 2000.0)
    assert np.array_equal(only, first)
    empty_pattern = np.arange(COUNTER_BASE) % 256 == 0
    assert np.array_equal(first[:COUNTER_BASE][empty_pattern], start[:COUNTER_BASE][empty_pattern])
    # what the forty copies added is forty times one step, wrapped
    index, used = m.ntuple_indices(rows[0], piece[0], L, M, lines[0], moves[0])
    alone = m.ntuple_update(np.zeros(ENTRIES, np.int32), rows[:40], piece[:40], L, M, lines[:40], moves[:40], 0, error[:40], 2000.0)
    total = int(m.ntuple_steps(error[:40], 2000.0).sum())
    assert total != 0 and (alone[index[0][used[0]]] == total).all() and np.count_nonzero(alone) == used[0].sum()


def test_the_exploration_index_is_uniform_over_the_distinct_placements():
    m = _m()
    n = 1 << 16
    assert m.PIECE_PLACEMENTS == (17, 34, 34, 34, 17, 17, 9, 9)
    distinct = m.canonical_actions(np.arange(8)[:, None], np.arange(40)[None, :]) == np.arange(40)[None, :]
    assert distinct.sum(axis=1).tolist() == list(m.PIECE_PLACEMENTS)
    h = m._draw_hashes(5, 11, n)
    for s in (9, 17, 34):
        explores, j = m.ntuple_explore(5, 11, n, 1.0, s)
        assert explores.all() and j.min() == 0 and j.max() == s - 1
        assert np.array_equal(j, ((h & np.uint64(0xFFFFFFFF)).astype(object) * s >> 32).astype(np.int64))      # in exact integers
        # n draws into s bins: a bin's count is binomial(n, 1 / s); five standard deviations, over 60 bins in all, leave a
        # fair stream a chance of about 3e-5 to fail -- and the stream is fixed, so the test is deterministic
        count = np.bincount(j, minlength=s)
        bound = 5.0 * np.sqrt(n * (1.0 / s) * (1.0 - 1.0 / s))
        assert np.abs(count - n / s).max() <= bound, (s, count, bound)
    # the coin: (h >> 40) < (uint32)(epsilon * 2^24); never at 0, always at 1, a quarter of the boards at 0.25 within 5 sigma
    assert not m.ntuple_explore(5, 11, n, 0.0, 9)[0].any()
    quarter = m.ntuple_explore(5, 11, n, 0.25, 9)[0]
    assert np.array_equal(quarter, (h >> np.uint64(40)) < np.uint64(1 << 22))
    assert abs(int(quarter.sum()) - n / 4) <= 5.0 * np.sqrt(n * 0.25 * 0.75)
    # per board placements, and another step is another stream
    per = np.array(m.PIECE_PLACEMENTS)[np.arange(n) % 8]
    _, j = m.ntuple_explore(5, 11, n, 1.0, per)
    assert (j < per).all() and not np.array_equal(m.ntuple_explore(5, 12, n, 1.0, 34)[1], m.ntuple_explore(5, 11, n, 1.0, 34)[1])
