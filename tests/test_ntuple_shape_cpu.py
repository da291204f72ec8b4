"""The table shapes of the n-tuple value function without a GPU (include/tpl_learn.h's "Table shapes"; csrc/learn/ntuple.hip;
_learn_lib.py's numpy mirror; ntuple.py):

  1. the mirror's 3 x 3 indices by hand -- a cell in the interior, the two corner cells, full columns --, the constants, and the
     2 x 4 indices as they were when `shape` is left out;
  2. ntuple_mirror_permutation("3x3"): an involution without a fixed tuple entry that fixes the counters, equal to the rule's closed
     form, and the map from a board's indices to its reflection's;
  3. the numpy update, trace update and coherent update on a 3 x 3 table: independent of the order of their inputs, and a symmetric
     update leaves the table equal to its sigma-image;
  4. the header declares the six _shaped entries with the twin's argument names plus `shape`, the library exports them, and
     tpl_ntuple_entries answers;
  5. each 3 x 3 kernel is in tools/kernel_resources.sh's output the expected number of times, without scratch, within 128 VGPRs;
  6. every refusal of the new entries comes back as a status, and the Python refusals.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tetris_piclim as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, M = 10, 40
TUPLES, PATTERNS, COUNTER_BASE, ENTRIES = 144, 512, 589824, 590848
ENTRIES_2X4 = 314368
PI = np.array([0, 2, 1, 3, 5, 4, 6, 7])
TWINS = ("tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_search", "tpl_ntuple_update", "tpl_ntuple_update_trace",
         "tpl_ntuple_update_coherent")


def _m():
    return T._learn_lib


def _indices(rows, piece=0, lines=0, moves=0):
    return _m().ntuple_indices(rows, piece, L, M, lines, moves, shape="3x3")


# ------------------------------------------------------------------------------------------------ 1. the mirror by hand
def test_the_constants():
    m = _m()
    assert m.NTUPLE_SHAPES["3x3"] == (TUPLES, PATTERNS, ENTRIES) and m.NTUPLE_SHAPES["2x4"] == (153, 256, ENTRIES_2X4)
    assert (8 * TUPLES * PATTERNS, 8 * TUPLES * PATTERNS + 1024) == (COUNTER_BASE, ENTRIES)
    assert set(m.NTUPLE_SHAPES) == {"2x4", "3x3"} and m.NTUPLE_ENTRIES == ENTRIES_2X4
    assert T.NTUPLE_SHAPES is m.NTUPLE_SHAPES and T.ntuple_shape is T.ntuple.ntuple_shape


def test_single_cells_and_full_columns_by_hand():
    empty = np.zeros(20, np.uint16)
    index, used = _indices(empty, piece=3, lines=1, moves=2)
    assert index.shape == (1, TUPLES + 1) and used.shape == (1, TUPLES + 1)
    assert not used[0, :TUPLES].any() and used[0, TUPLES]                     # the all-empty pattern is skipped; the counter is not
    assert index[0, TUPLES] == COUNTER_BASE + 64 * 9 + 38
    assert np.array_equal(index[0, :TUPLES], (3 * TUPLES + np.arange(TUPLES)) * PATTERNS)
    # a cell in the interior, (row 10, column 5): the nine windows x = 3..5, y = 8..10, with the nine one-bit patterns
    rows = empty.copy()
    rows[10] = 1 << 5
    index, used = _indices(rows, piece=5)
    want = {18 * x + y: 1 << (3 * (5 - x) + (10 - y)) for x in (3, 4, 5) for y in (8, 9, 10)}
    assert sorted(np.flatnonzero(used[0, :TUPLES]).tolist()) == sorted(want)
    assert sorted(want.values()) == [1 << k for k in range(9)]
    for t, q in want.items():
        assert index[0, t] == ((5 * TUPLES + t) * PATTERNS) | q
    # the two corner cells lie in one window each: the first tuple's bit 0, the last tuple's bit 8
    rows = empty.copy()
    rows[0] = 1 << 0
    index, used = _indices(rows, piece=7)
    assert np.flatnonzero(used[0, :TUPLES]).tolist() == [0] and index[0, 0] == (7 * TUPLES * PATTERNS) | 1
    rows = empty.copy()
    rows[19] = 1 << 9
    index, used = _indices(rows, piece=1)
    assert np.flatnonzero(used[0, :TUPLES]).tolist() == [18 * 7 + 17] and 18 * 7 + 17 == TUPLES - 1
    assert index[0, TUPLES - 1] == ((1 * TUPLES + TUPLES - 1) * PATTERNS) | 256
    # a full column of 20 cells: 18 windows per window column that holds it, each with one full triplet
    for column, xs in ((0, (0,)), (1, (0, 1)), (4, (2, 3, 4)), (8, (6, 7)), (9, (7,))):
        rows = np.full(20, 1 << column, np.uint16)
        index, used = _indices(rows, piece=2)
        assert used[0, :TUPLES].sum() == 18 * len(xs)
        for x in range(8):
            for y in range(18):
                t = 18 * x + y
                assert used[0, t] == (x in xs)
                assert index[0, t] == ((2 * TUPLES + t) * PATTERNS) | ((7 << (3 * (column - x))) if x in xs else 0)
    # a full board: every pattern is 511
    index, used = _indices(np.full(20, 0x3FF, np.uint16), piece=6)
    assert used.all() and (index[0, :TUPLES] & 511 == 511).all()


def test_the_value_on_a_3x3_table_and_the_2x4_results_as_they_were():
    m = _m()
    gen = np.random.default_rng(33)
    rows = gen.integers(0, 1 << 10, (40, 20)).astype(np.uint16)
    piece, lines, moves = gen.integers(0, 8, 40), gen.integers(0, 12, 40), gen.integers(0, 45, 40)
    state = gen.integers(0, 2, 40)
    # 2 x 4 with `shape` left out: the rule restated here, cell by cell
    index, used = m.ntuple_indices(rows, piece, L, M, lines, moves)
    named, _ = m.ntuple_indices(rows, piece, L, M, lines, moves, shape="2x4")
    assert index.shape == (40, 154) and np.array_equal(index, named)
    for i in (0, 7, 39):
        for x in range(9):
            for y in range(17):
                q = sum((((int(rows[i, y + j]) >> x) & 1) << j) | (((int(rows[i, y + j]) >> (x + 1)) & 1) << (4 + j)) for j in range(4))
                assert index[i, 17 * x + y] == (piece[i] * 153 + 17 * x + y) * 256 + q and used[i, 17 * x + y] == (q != 0)
        assert index[i, 153] == 313344 + 64 * min(max(L - lines[i], 0), 15) + min(max(M - moves[i], 0), 63)
    # the value sizes itself by the table: exact sum, one rounding, 0 for a finished state
    for entries, shape in ((ENTRIES_2X4, "2x4"), (ENTRIES, "3x3")):
        table = gen.integers(-(1 << 30), 1 << 30, entries).astype(np.int32)
        index, used = m.ntuple_indices(rows, piece, L, M, lines, moves, shape=shape)
        total = np.array([sum(int(table[j]) for j in index[i][used[i]]) for i in range(40)])
        want = np.where(state == 0, total.astype(np.float32) * np.float32(2.0 ** -16), np.float32(0.0)).astype(np.float32)
        got = m.ntuple_value(table, rows, piece, L, M, lines, moves, state)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (got[state == 0] != 0).all()
    for bad in (np.zeros(ENTRIES + 1, np.int32), np.zeros(ENTRIES, np.int64), np.zeros((ENTRIES, 1), np.int32)):
        with pytest.raises(ValueError, match="table"):
            m.ntuple_value(bad, rows, piece, L, M, lines, moves, state)
    with pytest.raises(ValueError, match="shape"):
        m.ntuple_indices(rows, piece, L, M, lines, moves, shape="4x4")


# ------------------------------------------------------------------------------------------------ 2. the mirror permutation
def _closed_form():
    sigma = np.arange(ENTRIES, dtype=np.int64)
    p, x, y, q = np.meshgrid(np.arange(8), np.arange(8), np.arange(18), np.arange(PATTERNS), indexing="ij")
    swapped = (q >> 6) | (q & 0x38) | ((q & 7) << 6)
    sigma[:COUNTER_BASE] = (((PI[p] * TUPLES + 18 * (7 - x) + y) * PATTERNS) | swapped).reshape(-1)
    return sigma


def test_the_3x3_mirror_permutation():
    m = _m()
    sigma = m.ntuple_mirror_permutation("3x3")
    at = np.arange(ENTRIES)
    assert sigma.shape == (ENTRIES,) and np.array_equal(sigma[sigma], at)     # an involution
    assert (sigma[:COUNTER_BASE] != at[:COUNTER_BASE]).all()                  # eight window columns: no tuple is its own image
    assert np.array_equal(sigma[COUNTER_BASE:], at[COUNTER_BASE:])            # the counters stay
    assert np.array_equal(sigma, _closed_form())
    # 2 x 4 as it was: the closed form of the existing rule, which does have fixed tuple entries (x = 4)
    old = m.ntuple_mirror_permutation()
    p, x, y, q = np.meshgrid(np.arange(8), np.arange(9), np.arange(17), np.arange(256), indexing="ij")
    want = np.arange(ENTRIES_2X4)
    want[:313344] = ((PI[p] * 153 + 17 * (8 - x) + y) * 256 + ((q >> 4) | ((q & 15) << 4))).reshape(-1)
    assert np.array_equal(old, want) and np.array_equal(old, m.ntuple_mirror_permutation("2x4")) and (old[:313344] == want[:313344]).all()
    assert (old[:313344] == np.arange(313344)).any()
    with pytest.raises(ValueError, match="shape"):
        m.ntuple_mirror_permutation("3x4")
    # the indices of a board go to those of its reflection, tuple for tuple: (x, y) -> (7 - x, y)
    gen = np.random.default_rng(8)
    k = 320
    rows = (gen.integers(0, 1 << 10, (k, 20)) & gen.integers(0, 1 << 10, (k, 20))).astype(np.uint16)
    rows[:8] = 0
    piece = np.arange(k) % 8
    lines, moves = gen.integers(0, 12, k), gen.integers(0, 45, k)
    index, used = _indices(rows, piece, lines, moves)
    mirrored, mirrored_used = _indices(m._reflected_rows(rows), PI[piece], lines, moves)
    where = np.array([18 * (7 - x) + y for x in range(8) for y in range(18)] + [TUPLES])
    assert np.array_equal(sigma[index], mirrored[:, where]) and np.array_equal(used, mirrored_used[:, where])
    assert set(piece.tolist()) == set(range(8)) and used[:, :TUPLES].sum() > 100 * k


# ------------------------------------------------------------------------------------------------ 3. the numpy updates
def _ages(gen, k, horizon):
    ages = []
    for _ in range(horizon):
        rows = (gen.integers(0, 1 << 10, (k, 20)) & gen.integers(0, 1 << 10, (k, 20))).astype(np.uint16)
        ages.append((rows, gen.integers(0, 8, k), gen.integers(0, 12, k), gen.integers(0, 45, k), (gen.random(k) < 0.15).astype(np.int64)))
    return ages


def _permuted(ages, order):
    return [tuple(np.asarray(v)[order] for v in age) for age in ages]


def test_the_numpy_updates_on_a_3x3_table_do_not_depend_on_the_order_and_keep_symmetry():
    m = _m()
    gen = np.random.default_rng(12)
    k, horizon = 96, 3
    ages = _ages(gen, k, horizon)
    error = gen.normal(size=k).astype(np.float32)
    error[:3] = (np.nan, 1e30, 0.0)
    order = gen.permutation(k)
    sigma = m.ntuple_mirror_permutation("3x3")
    start = gen.integers(-(1 << 31), 1 << 31, ENTRIES).astype(np.int32)
    # the plain update
    rows, piece, lines, moves, state = ages[0]
    one = m.ntuple_update(start.copy(), rows, piece, L, M, lines, moves, state, error, 3000.0)
    r2, p2, l2, m2, s2 = _permuted(ages, order)[0]
    assert np.array_equal(one, m.ntuple_update(start.copy(), r2, p2, L, M, l2, m2, s2, error[order], 3000.0))
    changed = np.flatnonzero(one != start)
    assert changed.size > 1000 and (changed[changed < COUNTER_BASE] % PATTERNS != 0).all()       # never the all-empty pattern
    assert np.array_equal(one, m.ntuple_update_trace(start.copy(), ages[:1], L, M, error, 3000.0, 0.3, False))
    # the trace update, symmetric and not
    for symmetric in (False, True):
        got = m.ntuple_update_trace(start.copy(), ages, L, M, error, 3000.0, 0.7, symmetric)
        assert np.array_equal(got, m.ntuple_update_trace(start.copy(), _permuted(ages, order), L, M, error[order], 3000.0, 0.7, symmetric))
        assert (got != start).sum() > changed.size
    zero = np.zeros(ENTRIES, np.int32)
    sym = m.ntuple_update_trace(zero.copy(), ages, L, M, error, 3000.0, 0.7, True)
    plain = m.ntuple_update_trace(zero.copy(), ages, L, M, error, 3000.0, 0.7, False)
    assert np.array_equal(sym[sigma], sym) and not np.array_equal(plain[sigma], plain)
    both = (plain.view(np.uint32) + plain[sigma].view(np.uint32)).view(np.int32)                   # the update and its sigma-image
    both[COUNTER_BASE:] = plain[COUNTER_BASE:]                                                      # the counter once
    assert np.array_equal(sym, both)
    # the coherent update: both buffers, from a filled coherence buffer
    coherence = np.zeros((ENTRIES, 2), np.int64)
    m.ntuple_update_coherent(zero.copy(), coherence, ages, L, M, error, 3000.0, 0.7, True)
    assert np.array_equal(coherence[sigma], coherence) and (coherence[:, 1] > 0).sum() > 1000
    flipped = -error
    t1, c1 = m.ntuple_update_coherent(sym.copy(), coherence.copy(), ages, L, M, flipped, 2000.0, 0.7, True)
    t2, c2 = m.ntuple_update_coherent(sym.copy(), coherence.copy(), _permuted(ages, order), L, M, flipped[order], 2000.0, 0.7, True)
    assert np.array_equal(t1, t2) and np.array_equal(c1, c2)
    assert np.array_equal(t1[sigma], t1) and np.array_equal(c1[sigma], c1)
    alpha = m.ntuple_step_sizes(c1)
    assert alpha.shape == (ENTRIES,) and alpha.dtype == np.float32 and (alpha < 1.0).sum() > 1000 and (alpha == 1.0).sum() > 1000
    # a zeroed coherence buffer leaves the trace update's table
    t0, _ = m.ntuple_update_coherent(start.copy(), np.zeros((ENTRIES, 2), np.int64), ages, L, M, error, 3000.0, 0.7, False)
    assert np.array_equal(t0, m.ntuple_update_trace(start.copy(), ages, L, M, error, 3000.0, 0.7, False))
    # a coherence buffer of the other shape is refused
    with pytest.raises(ValueError, match="coherence"):
        m.ntuple_update_coherent(start.copy(), np.zeros((ENTRIES_2X4, 2), np.int64), ages, L, M, error, 1.0, 0.5, False)
    with pytest.raises(ValueError, match="coherence"):
        m.ntuple_step_sizes(np.zeros((ENTRIES + 1, 2), np.int64))


# ------------------------------------------------------------------------------------------------ 4. header and library
def test_the_header_declares_the_shaped_entries_and_the_library_exports_them():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS)
    names = lambda entry: [a.split()[-1].lstrip("*") for a in re.search(rf"int {entry}\((.*?)\);", text, flags=re.S).group(1).split(",")]
    for twin in TWINS:
        assert twin + "_shaped" in declared
        assert names(twin + "_shaped") == names(twin)[:-1] + ["shape", "stream"], twin
    assert re.search(r"#define\s+TPL_NTUPLE_ENTRIES_3X3\s+590848\b", text) and re.search(r"#define\s+TPL_NTUPLE_ENTRIES\s+314368\b", text)
    assert re.search(r"TPL_NTUPLE_SHAPE_2X4\s*=\s*0\b", text) and re.search(r"TPL_NTUPLE_SHAPE_3X3\s*=\s*1\b", text)
    assert "no wall and no floor bits" in raw                   # the rule says why the windows stay inside the board
    lib = ctypes.CDLL(_m().build_library())
    for twin in TWINS:
        assert hasattr(lib, twin + "_shaped"), twin
    lib.tpl_ntuple_entries.restype = ctypes.c_int64
    lib.tpl_ntuple_entries.argtypes = [ctypes.c_int32]
    assert [lib.tpl_ntuple_entries(s) for s in (0, 1, 2, -1, 1 << 20)] == [314368, 590848, -1, -1, -1]
    assert [os.path.basename(p) for p in _m()._UNITS][-1] == "heuristic.hip"


def test_the_3x3_kernels_use_no_scratch_and_at_most_128_vgprs():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    expected = {"ntuple3_value_kernel": 1, "ntuple3_act_kernel": 1, "ntuple3_search_kernel": 1, "ntuple3_trace_kernel": 2,
                "ntuple3_trace_kernelILb0": 1, "ntuple3_coherent_step_kernel": 2, "ntuple3_coherent_accumulate_kernel": 2}
    for kernel, count in expected.items():
        mine = [r for r in rows if kernel in r[-1]]
        assert len(mine) == count, (kernel, [r[-1] for r in rows])
        for r in mine:
            print(" ".join(r))
            assert r[r.index("scratch") - 1] == "0", r
            assert int(r[r.index("vgpr") - 1]) <= 128, r
    assert sum(1 for r in rows if "ntuple3_" in r[-1]) == 9
    # the coherent kernels' LDS is the 2 x 4 twins': the counter pre-sums do not depend on the shape
    lds = lambda name: sorted(r[r.index("lds") - 1] for r in rows if name in r[-1])
    for kernel in ("trace_kernel", "coherent_step_kernel", "coherent_accumulate_kernel"):
        assert lds("ntuple3_" + kernel) == lds("ntuple_" + kernel), kernel


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_every_refusal_of_the_shaped_entries_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")

    def value(shape=1, a=fake, b=fake, n=4, L=2, M=2, table=fake, value=fake):
        return lib.tpl_ntuple_value_shaped(a, b, n, L, M, table, value, shape, None)

    def act(shape=1, a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake,
            score=fake):
        return lib.tpl_ntuple_act_shaped(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, score, after_a, after_b,
                                         fake, shape, None)

    def search(shape=1, a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake,
               score=fake):
        return lib.tpl_ntuple_search_shaped(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, fake + 1, score,
                                            after_a, after_b, fake, shape, None)

    def update(shape=1, a=fake, b=fake, n=4, L=2, M=2, table=fake, error=fake, rate=1.0):
        return lib.tpl_ntuple_update_shaped(a, b, n, L, M, table, error, rate, shape, None)

    def trace(shape=1, a=fake, b=fake, n=4, L=2, M=2, table=fake, error=fake, rate=1.0, slots=3, head=0, horizon=2, decay=0.5):
        return lib.tpl_ntuple_update_trace_shaped(a, b, n, slots, head, horizon, L, M, table, error, rate, decay, 1, shape, None)

    def coherent(shape=1, a=fake, b=fake, n=4, L=2, M=2, table=fake, error=fake, rate=1.0, slots=3, head=0, horizon=2, decay=0.5,
                 coherence=fake):
        return lib.tpl_ntuple_update_coherent_shaped(a, b, n, slots, head, horizon, L, M, table, coherence, error, rate, decay, 0,
                                                     shape, None)

    entries = ((value, b"tpl_ntuple_value_shaped"), (act, b"tpl_ntuple_act_shaped"), (search, b"tpl_ntuple_search_shaped"),
               (update, b"tpl_ntuple_update_shaped"), (trace, b"tpl_ntuple_update_trace_shaped"),
               (coherent, b"tpl_ntuple_update_coherent_shaped"))
    limit = -(-(1 << 31) // 40)
    for entry, name in entries:
        # the shape, before anything else: every pointer null as well
        for shape in (-1, 2, 7, 1 << 30):
            assert entry(shape=shape) < 0 and b"shape" in err() and name in err(), (name, shape)
            assert entry(shape=shape, a=None, b=None, table=None) < 0 and b"shape" in err() and b"null" not in err(), (name, shape)
        # the twin's own refusals through the new entry, at both shapes
        for shape in (0, 1):
            assert entry(shape=shape, a=None) < 0 and b"null" in err() and name in err()
            assert entry(shape=shape, b=None) < 0 and b"null" in err() and name in err()
            for n in (0, -1):
                assert entry(shape=shape, n=n) < 0 and b"positive" in err() and name in err(), n
            for n in (limit, 1 << 40):
                assert entry(shape=shape, n=n) < 0 and b"2^31" in err() and name in err(), n
            for plane in ("a", "b"):
                assert entry(shape=shape, **{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err()
            for L_, M_ in ((0, 2), (2, 256), (251, 2), (2, 255), (2, 0)):
                assert entry(shape=shape, L=L_, M=M_) < 0 and b"L and M" in err() and name in err(), (L_, M_)
            assert entry(shape=shape, table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
            for off in (4, 8, 12):
                assert entry(shape=shape, table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
    assert value(value=None) < 0 and b"null" in err() and b"value" in err()
    assert value(value=fake + 2) < 0 and b"value must be 4-byte aligned" in err()
    for entry in (act, search):
        assert entry(action=None) < 0 and b"null" in err() and b"action" in err()
        assert entry(after_a=None) < 0 and b"go together" in err()
        assert entry(after_b=fake + 4) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
        assert entry(score=fake + 2) < 0 and b"4-byte aligned" in err()
        for epsilon in (-0.001, 1.001, nan, inf):
            assert entry(epsilon=epsilon) < 0 and b"epsilon must be in [0, 1]" in err(), epsilon
        for gamma in (nan, inf, -inf):
            assert entry(gamma=gamma) < 0 and b"gamma must be finite" in err(), gamma
    for entry in (update, trace, coherent):
        assert entry(error=None) < 0 and b"null" in err() and b"error" in err()
        assert entry(error=fake + 2) < 0 and b"error must be 4-byte aligned" in err()
        for rate in (nan, inf, -inf):
            assert entry(rate=rate) < 0 and b"rate must be finite" in err(), rate
    for entry in (trace, coherent):
        for slots in (0, -1, 18):
            assert entry(slots=slots, horizon=1) < 0 and b"slots must be in [1, 17]" in err(), slots
        for head in (-1, 3):
            assert entry(head=head) < 0 and b"head must be in [0, slots)" in err(), head
        for horizon in (0, 4):
            assert entry(horizon=horizon) < 0 and b"horizon must be in" in err(), horizon
        assert entry(slots=17, horizon=17) < 0 and b"horizon must be in" in err()
        assert entry(n=limit // 3 + 1) < 0 and b"40 * slots * n" in err()
        for decay in (-0.1, 1.1, nan):
            assert entry(decay=decay) < 0 and b"decay must be in [0, 1]" in err(), decay
    assert coherent(coherence=None) < 0 and b"null" in err() and b"coherence" in err()
    assert coherent(coherence=fake + 8) < 0 and b"coherence must be 16-byte aligned" in err()
    assert coherent(coherence=None, table=None) < 0 and b"table" in err()                          # after the table checks
    # the existing entries name themselves and not their twins
    assert lib.tpl_ntuple_value(None, fake, 4, 2, 2, fake, fake, None) < 0 and b"tpl_ntuple_value:" in err()


def test_the_python_refusals():
    N = T.ntuple
    assert N.ntuple_table("cpu").shape == (ENTRIES_2X4,) and N.ntuple_table("cpu", shape="3x3").shape == (ENTRIES,)
    assert N.ntuple_coherence("cpu", "3x3").shape == (ENTRIES, 2) and N.ntuple_coherence("cpu").shape == (ENTRIES_2X4, 2)
    assert N.ntuple_table("cpu", "3x3").dtype == torch.int32 and N.ntuple_coherence("cpu", "3x3").dtype == torch.int64
    assert N.ntuple_shape(N.ntuple_table("cpu")) == "2x4" and N.ntuple_shape(N.ntuple_table("cpu", "3x3")) == "3x3"
    for shape in ("4x4", "3X3", 1, None):
        with pytest.raises(ValueError, match="shape"):
            N.ntuple_table("cpu", shape=shape)
        with pytest.raises(ValueError, match="shape"):
            N.ntuple_coherence("cpu", shape=shape)
    third = torch.zeros(ENTRIES + 1024, dtype=torch.int32)
    for bad in (third, torch.zeros(0, dtype=torch.int32), [0] * 5, None):
        with pytest.raises(ValueError, match="table"):
            N.ntuple_shape(bad)
    with pytest.raises(ValueError, match="table"):
        N.ntuple_is_symmetric(third)
    with pytest.raises(ValueError, match="table"):
        N.ntuple_value((torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32)), third, L, M)
    with pytest.raises(ValueError, match="coherence"):
        N.ntuple_step_sizes(torch.zeros((ENTRIES + 1024, 2), dtype=torch.int64))
    # a coherence buffer of the other shape than the table's
    for table, buffer in (("3x3", "2x4"), ("2x4", "3x3")):
        with pytest.raises(ValueError, match="coherence"):
            N._coherence(N.ntuple_coherence("cpu", buffer), N.ntuple_table("cpu", table))
        assert N._coherence(N.ntuple_coherence("cpu", table), N.ntuple_table("cpu", table)) is not None
    # both sizes on the CPU: the symmetry test and the step sizes take the shape from what they are given
    for shape in ("2x4", "3x3"):
        assert N.ntuple_is_symmetric(N.ntuple_table("cpu", shape))
        one = N.ntuple_table("cpu", shape)
        one[5] = 1
        assert not N.ntuple_is_symmetric(one)
        assert (N.ntuple_step_sizes(N.ntuple_coherence("cpu", shape)) == 1.0).all()
