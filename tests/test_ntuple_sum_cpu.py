"""Two table shapes summed in one n-tuple value, without a GPU (include/tpl_learn.h's "Two shapes summed"; the _sum entries of
csrc/learn/ntuple.hip and ntuple_beam.hip; _learn_lib.py's numpy mirror; ntuple.py):

  1. the constants and the layout arithmetic: the second part of a sum table and of its coherence buffer starts 16-byte aligned;
  2. the sum indices are the two shapes' indices side by side, the second offset by where its part starts;
  3. the mirror value under full-range int32 tables is float32 of the Python-integer sum of BOTH parts, times 2^-16 -- one rounding
     -- and on at least a tenth of the running boards that is not float32(S_2x4) + float32(S_3x3);
  4. the mirror update, trace update and coherent update of a sum table are the existing mirror updates applied to the two parts;
  5. the mirror permutation is each part's, offset; ntuple_is_symmetric wants every part symmetric;
  6. the header declares the four _sum entries with their twins' arguments, the library exports them, tpl_ntuple_entries is as it was,
     and the four kernels use no scratch;
  7. every argument refusal of the four entries, with fake pointers, in the twin's order and under the entry's own name;
  8. the Python refusals and ntuple_parts.
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
ENTRIES_2X4, ENTRIES_3X3, ENTRIES_SUM = 314368, 590848, 905216
SUM = "2x4+3x3"


def _m():
    return T._learn_lib


def _boards(seed, k):
    """k boards as piled columns with holes (rows uint16 [k, 20], row 0 the top), with a piece, lines, moves and a state each; every
    fifth state is finished."""
    gen = np.random.default_rng(seed)
    height = gen.integers(0, 21, (k, 10))
    height[gen.integers(0, k, k // 8), gen.integers(0, 10, k // 8)] = 20           # full-height columns among them
    depth = 20 - np.arange(20)[None, :, None]                                        # row y is `20 - y` cells above the floor
    cell = (depth <= height[:, None, :]) & (gen.random((k, 20, 10)) < 0.85)
    rows = (cell.astype(np.int64) << np.arange(10)[None, None, :]).sum(axis=2).astype(np.uint16)
    state = np.where(np.arange(k) % 5 == 4, gen.integers(1, 4, k), 0)
    return dict(rows=rows, piece=gen.integers(0, 8, k), lines=gen.integers(0, 12, k), moves=gen.integers(0, 45, k), state=state)


def _full_range(seed, entries):
    return np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, entries).astype(np.int32)


def _args(b):
    return b["rows"], b["piece"], L, M, b["lines"], b["moves"]


# ------------------------------------------------------------------------------------------------ 1. constants and layout
def test_the_constants_and_the_layout():
    m = _m()
    assert m.NTUPLE_SUMS == {SUM: ("2x4", "3x3")} and m.NTUPLE_ENTRIES_SUM == ENTRIES_SUM == ENTRIES_2X4 + ENTRIES_3X3
    assert T.NTUPLE_SUMS is m.NTUPLE_SUMS and T.NTUPLE_ENTRIES_SUM == ENTRIES_SUM and T.ntuple_parts is T.ntuple.ntuple_parts
    assert set(m.NTUPLE_SHAPES) == {"2x4", "3x3"} and set(m.NTUPLE_SHAPE_IDS) == {"2x4", "3x3"}    # the sum is no third shape
    assert m.ntuple_shape_of(ENTRIES_SUM) == SUM and m.ntuple_shape_of(ENTRIES_2X4) == "2x4" and m.ntuple_shape_of(ENTRIES_3X3) == "3x3"
    assert m.ntuple_parts_of(SUM) == ("2x4", "3x3") and m.ntuple_parts_of("3x3") == ("3x3",) and m.ntuple_entries_of(SUM) == ENTRIES_SUM
    with pytest.raises(ValueError):
        m.ntuple_shape_of(ENTRIES_SUM + 1)
    # bytes: the table is 3,620,864 and its second part starts at 1,257,472; the coherence buffer's at 5,029,888 -- multiples of 16
    assert 4 * ENTRIES_SUM == 3620864 and 4 * ENTRIES_2X4 == 1257472 and (4 * ENTRIES_2X4) % 16 == 0
    assert 16 * ENTRIES_SUM == 14483456 and 16 * ENTRIES_2X4 == 5029888 and (16 * ENTRIES_2X4) % 16 == 0
    assert 4 * ENTRIES_SUM < 4 << 20                           # inside the 4 MiB L2 of an XCD, which a 4 x 3 window's table is not
    table, sums = T.ntuple_table("cpu", SUM), T.ntuple_coherence("cpu", SUM)
    assert tuple(table.shape) == (ENTRIES_SUM,) and table.dtype == torch.int32 and int(table.abs().sum()) == 0
    assert tuple(sums.shape) == (ENTRIES_SUM, 2) and sums.dtype == torch.int64
    for whole, unit in ((table, 4), (sums, 16)):
        parts = T.ntuple_parts(whole)
        assert [p.shape[0] for p in parts] == [ENTRIES_2X4, ENTRIES_3X3] and all(p.is_contiguous() for p in parts)
        assert [p.data_ptr() - whole.data_ptr() for p in parts] == [0, unit * ENTRIES_2X4]
        assert [T.ntuple_shape(p) for p in parts] == ["2x4", "3x3"]
        parts[1][7] = 5                                        # a view: written through to the whole
        assert int(whole[ENTRIES_2X4 + 7].reshape(-1)[0]) == 5
    for shape in ("2x4", "3x3"):
        one = T.ntuple_table("cpu", shape)
        parts = T.ntuple_parts(one)
        assert len(parts) == 1 and parts[0].data_ptr() == one.data_ptr() and parts[0].shape == one.shape


# ------------------------------------------------------------------------------------------------ 2. the indices
def test_the_sum_indices_are_the_two_shapes_indices_with_the_offset():
    m, b = _m(), _boards(1, 64)
    index, used = m.ntuple_indices(*_args(b), shape=SUM)
    i2, u2 = m.ntuple_indices(*_args(b), shape="2x4")
    i3, u3 = m.ntuple_indices(*_args(b), shape="3x3")
    assert index.shape == used.shape == (64, 154 + 145) and index.dtype == np.int64 and used.dtype == bool
    assert np.array_equal(index[:, :154], i2) and np.array_equal(index[:, 154:], i3 + ENTRIES_2X4)
    assert np.array_equal(used[:, :154], u2) and np.array_equal(used[:, 154:], u3)
    assert used[:, 153].all() and used[:, 298].all()           # both counters, the same k behind each part's own base
    assert np.array_equal(index[:, 153] - 313344, index[:, 298] - ENTRIES_2X4 - 589824)
    assert index[:, :154].max() < ENTRIES_2X4 <= index[:, 154:].min() and index.max() < ENTRIES_SUM
    assert m._counter_columns(SUM) == [153, 298] and m._counter_columns("2x4") == [153] and m._counter_columns("3x3") == [144]
    one, _ = m.ntuple_indices(b["rows"][0], 3, L, M, 1, 2, shape=SUM)
    assert one.shape == (1, 299)
    in_use = used[b["state"] == 0].sum(axis=1)
    print(f"entries in use per running board: mean {in_use.mean():.1f}, {in_use.min()} .. {in_use.max()}")


# ------------------------------------------------------------------------------------------------ 3. the value
def test_the_value_is_one_rounding_of_the_integer_sum_of_both_parts():
    m, b = _m(), _boards(2, 400)
    table = _full_range(3, ENTRIES_SUM)
    i2, u2 = m.ntuple_indices(*_args(b), shape="2x4")
    i3, u3 = m.ntuple_indices(*_args(b), shape="3x3")
    first, second = table[:ENTRIES_2X4], table[ENTRIES_2X4:]
    sa = [sum(int(first[j]) for j in i2[i][u2[i]]) for i in range(400)]                 # Python integers: exact
    sb = [sum(int(second[j]) for j in i3[i][u3[i]]) for i in range(400)]
    run = b["state"] == 0
    scale = np.float32(2.0 ** -16)
    want = np.array([np.float32(a + c) * scale if r else np.float32(0.0) for a, c, r in zip(sa, sb, run)], dtype=np.float32)
    got = m.ntuple_value(table, *_args(b), b["state"])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got.view(np.uint32)[~run] == 0).all() and (got[run] != 0).all() and (~run).sum() == 80
    # the sums are wider than float32's 24 bits, so where the rounding happens matters: rounding each part first gives another value
    twice = np.array([np.float32(a) + np.float32(c) for a, c in zip(sa, sb)], dtype=np.float32) * scale
    differ = (twice.view(np.uint32) != want.view(np.uint32)) & run
    widest = max(abs(a + c) for a, c, r in zip(sa, sb, run) if r)
    print(f"float32(Sa + Sb) != float32(Sa) + float32(Sb) on {differ.sum()} of {run.sum()} running boards; widest |S| 2^{np.log2(widest):.1f}")
    assert differ.sum() >= run.sum() / 10 and widest > 1 << 33
    # each part alone is a valid table of its shape: with the other part zero the sum table's value is the part's own
    for lo, hi, part in ((0, ENTRIES_2X4, first), (ENTRIES_2X4, ENTRIES_SUM, second)):
        only = np.zeros(ENTRIES_SUM, np.int32)
        only[lo:hi] = part
        alone = m.ntuple_value(np.ascontiguousarray(part), *_args(b), b["state"])
        assert np.array_equal(m.ntuple_value(only, *_args(b), b["state"]).view(np.uint32), alone.view(np.uint32))
    for bad in (np.zeros(ENTRIES_SUM + 1, np.int32), np.zeros(ENTRIES_SUM, np.int64)):
        with pytest.raises(ValueError, match="table"):
            m.ntuple_value(bad, *_args(b), b["state"])


# ------------------------------------------------------------------------------------------------ 4. the updates
def _ages(seed, k, horizon):
    return [tuple(_boards(seed + age, k)[f] for f in ("rows", "piece", "lines", "moves", "state")) for age in range(horizon)]


def _errors(seed, k):
    error = np.random.default_rng(seed).normal(size=k).astype(np.float32)
    error[:4] = np.array([0.0, np.nan, 1e9, -1e9], np.float32)
    return error


def test_the_update_of_a_sum_table_is_the_two_updates_of_its_parts():
    m, k = _m(), 96
    b, error = _boards(5, k), _errors(6, k)
    start = _full_range(7, ENTRIES_SUM)
    start[::5] = np.int32((1 << 31) - 1)                       # adds that wrap
    got = m.ntuple_update(start.copy(), *_args(b), b["state"], error, 3000.0)
    want = start.copy()
    for lo, hi in ((0, ENTRIES_2X4), (ENTRIES_2X4, ENTRIES_SUM)):
        want[lo:hi] = m.ntuple_update(start[lo:hi].copy(), *_args(b), b["state"], error, 3000.0)
    assert np.array_equal(got, want) and (got[:ENTRIES_2X4] != start[:ENTRIES_2X4]).any() and (got[ENTRIES_2X4:] != start[ENTRIES_2X4:]).any()
    assert (got != start)[[313344 + c for c in range(1024)]].any() and (got != start)[ENTRIES_2X4 + 589824:].any()    # both counters


@pytest.mark.parametrize("symmetric", [False, True])
def test_the_trace_and_coherent_updates_of_a_sum_table_are_those_of_its_parts(symmetric):
    m, k, horizon = _m(), 48, 3
    ages, error = _ages(11, k, horizon), _errors(12, k)
    start = _full_range(13, ENTRIES_SUM)
    cuts = ((0, ENTRIES_2X4), (ENTRIES_2X4, ENTRIES_SUM))
    got = m.ntuple_update_trace(start.copy(), ages, L, M, error, 3000.0, 0.7, symmetric)
    want = start.copy()
    for lo, hi in cuts:
        want[lo:hi] = m.ntuple_update_trace(start[lo:hi].copy(), ages, L, M, error, 3000.0, 0.7, symmetric)
    assert np.array_equal(got, want) and (got != start).any()
    # from the zero table a symmetric update leaves a table whose every part is symmetric
    left = m.ntuple_update_trace(np.zeros(ENTRIES_SUM, np.int32), ages, L, M, error, 3000.0, 0.7, symmetric)
    sigma = m.ntuple_mirror_permutation(SUM)
    assert np.array_equal(left[sigma], left) == symmetric
    # coherent, from a filled buffer: step sizes below 1 are in play
    filled = np.random.default_rng(14).integers(0, 1 << 20, (ENTRIES_SUM, 2)).astype(np.int64)
    filled[::3, 0] //= 3
    got_table, got_sums = m.ntuple_update_coherent(start.copy(), filled.copy(), ages, L, M, error, 3000.0, 0.7, symmetric)
    want_table, want_sums = start.copy(), filled.copy()
    for lo, hi in cuts:
        t, c = m.ntuple_update_coherent(start[lo:hi].copy(), filled[lo:hi].copy(), ages, L, M, error,
                                        3000.0, 0.7, symmetric)
        want_table[lo:hi], want_sums[lo:hi] = t, c
    assert np.array_equal(got_table, want_table) and np.array_equal(got_sums, want_sums)
    assert not np.array_equal(got_table, got) and (got_sums != filled).any()
    alpha = m.ntuple_step_sizes(filled)
    assert alpha.shape == (ENTRIES_SUM,) and np.array_equal(alpha[ENTRIES_2X4:], m.ntuple_step_sizes(np.ascontiguousarray(filled[ENTRIES_2X4:])))
    with pytest.raises(ValueError, match="coherence"):
        m.ntuple_update_coherent(start.copy(), np.zeros((ENTRIES_3X3, 2), np.int64), ages, L, M, error, 3000.0, 0.7, symmetric)


# ------------------------------------------------------------------------------------------------ 5. symmetry
def test_the_mirror_permutation_is_each_parts_and_symmetry_wants_every_part():
    m = _m()
    sigma = m.ntuple_mirror_permutation(SUM)
    assert sigma.shape == (ENTRIES_SUM,) and np.array_equal(sigma[:ENTRIES_2X4], m.ntuple_mirror_permutation("2x4"))
    assert np.array_equal(sigma[ENTRIES_2X4:], m.ntuple_mirror_permutation("3x3") + ENTRIES_2X4)
    assert np.array_equal(sigma[sigma], np.arange(ENTRIES_SUM))
    zero = T.ntuple_table("cpu", SUM)
    assert T.ntuple_is_symmetric(zero)
    gen = np.random.default_rng(21)
    parts = []
    for shape in ("2x4", "3x3"):                               # a symmetric table of each shape: t + t[sigma]
        t = gen.integers(-1000, 1000, m.NTUPLE_SHAPES[shape][2]).astype(np.int32)
        parts.append(torch.from_numpy(t + t[m.ntuple_mirror_permutation(shape)]))
        assert T.ntuple_is_symmetric(parts[-1])
    both = torch.cat(parts)
    assert T.ntuple_is_symmetric(both)
    for k, (lo, j) in enumerate(((0, 256 + 3), (ENTRIES_2X4, 512 + 3))):   # break one part: a tuple entry that is not its own image
        broken = both.clone()
        broken[lo + j] += 1
        views = T.ntuple_parts(broken)
        assert not T.ntuple_is_symmetric(broken)
        assert not T.ntuple_is_symmetric(views[k].contiguous()) and T.ntuple_is_symmetric(views[1 - k].contiguous())


# ------------------------------------------------------------------------------------------------ 6. header, library, kernels
SUM_ENTRIES = {"tpl_ntuple_value_sum": "tpl_ntuple_value", "tpl_ntuple_act_sum": "tpl_ntuple_act",
               "tpl_ntuple_search_sum": "tpl_ntuple_search", "tpl_ntuple_beam_sum": "tpl_ntuple_beam"}


def test_the_header_declares_the_sum_entries_and_the_library_exports_them():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and set(SUM_ENTRIES) <= declared
    names = lambda entry: [a.split()[-1].lstrip("*") for a in re.search(rf"int {entry}\((.*?)\);", text, flags=re.S).group(1).split(",")]
    for entry, twin in SUM_ENTRIES.items():
        assert names(entry) == [a for a in names(twin) if a != "shape"], entry
    assert re.search(r"#define\s+TPL_NTUPLE_ENTRIES_SUM\s+\(TPL_NTUPLE_ENTRIES \+ TPL_NTUPLE_ENTRIES_3X3\)", text)
    assert "added BEFORE the one rounding" in raw and "905,216" in raw and "1,257,472" in raw
    lib = ctypes.CDLL(_m().build_library())
    for entry in SUM_ENTRIES:
        assert hasattr(lib, entry), entry
    lib.tpl_ntuple_entries.restype = ctypes.c_int64
    lib.tpl_ntuple_entries.argtypes = [ctypes.c_int32]
    assert [lib.tpl_ntuple_entries(s) for s in (0, 1, 2, 3, -1)] == [ENTRIES_2X4, ENTRIES_3X3, -1, -1, -1]


def test_the_sum_kernels_use_no_scratch_and_the_frames_of_their_twins():
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _m().build_library()], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    field = lambda r, name: int(r[r.index(name) - 1])
    for kernel, twin in (("ntuple_sum_value_kernel", "ntuple3_value_kernel"), ("ntuple_sum_act_kernel", "ntuple3_act_kernel"),
                         ("ntuple_sum_search_kernel", "ntuple3_search_kernel"), ("ntuple_beam_sum_kernel", "ntuple_beam3_kernel")):
        mine, other = [r for r in rows if kernel in r[-1]], [r for r in rows if twin in r[-1]]
        assert len(mine) == 1 and len(other) == 1, kernel
        print(" ".join(mine[0]))
        assert field(mine[0], "scratch") == 0 and field(mine[0], "vgpr") <= 128
        assert field(mine[0], "lds") == field(other[0], "lds")                 # the beam: 24,904 bytes
    assert field([r for r in rows if "ntuple_beam_sum_kernel" in r[-1]][0], "lds") == 24904
    assert all(field(r, "scratch") == 0 for r in rows if "ntuple" in r[-1])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_every_refusal_of_the_sum_entries_comes_back_as_a_status_in_the_twins_order():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")

    def value(a=fake, b=fake, n=4, L=2, M=2, table=fake, value=fake):
        return lib.tpl_ntuple_value_sum(a, b, n, L, M, table, value, None)

    def act(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
            value=fake):
        return lib.tpl_ntuple_act_sum(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, score, after_a, after_b, value,
                                      None)

    def search(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
               value=fake):
        return lib.tpl_ntuple_search_sum(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, fake + 1, score, after_a,
                                         after_b, value, None)

    def beam(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, depth=3, width=8, action=fake, after_a=fake, after_b=fake,
             score=fake):
        return lib.tpl_ntuple_beam_sum(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, depth, width, action, fake + 1, score, after_a,
                                       after_b, None)

    entries = ((value, b"tpl_ntuple_value_sum:"), (act, b"tpl_ntuple_act_sum:"), (search, b"tpl_ntuple_search_sum:"),
               (beam, b"tpl_ntuple_beam_sum:"))
    limit = -(-(1 << 31) // 40)
    for entry, name in entries:
        assert entry(a=None) < 0 and b"null" in err() and name in err()
        assert entry(b=None) < 0 and b"null" in err() and name in err()
        for n in (0, -1):
            assert entry(n=n) < 0 and b"positive" in err() and name in err(), n
        for n in (limit, 1 << 40):
            assert entry(n=n) < 0 and b"2^31" in err() and name in err(), n
        for plane in ("a", "b"):
            assert entry(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err()
        for L_, M_ in ((0, 2), (2, 256), (251, 2), (2, 255), (2, 0)):
            assert entry(L=L_, M=M_) < 0 and b"L and M" in err() and name in err(), (L_, M_)
        assert entry(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
        for off in (4, 8, 12):
            assert entry(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
        # the order: planes before n before L and M before the table
        assert entry(a=None, n=0, L=0, table=None) < 0 and b"null" in err() and b"table" not in err()
        assert entry(n=0, L=0, table=None) < 0 and b"positive" in err()
        assert entry(L=0, table=None) < 0 and b"L and M" in err()
    assert value(value=None) < 0 and b"null" in err() and b"value" in err() and b"tpl_ntuple_value_sum:" in err()
    assert value(value=fake + 2) < 0 and b"value must be 4-byte aligned" in err()
    assert value(table=None, value=None) < 0 and b"table" in err()
    for entry, name in entries[1:]:
        assert entry(action=None) < 0 and b"null" in err() and b"action" in err() and name in err()
        assert entry(after_a=None) < 0 and b"go together" in err() and name in err()
        assert entry(after_b=fake + 4) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
        assert entry(score=fake + 2) < 0 and b"4-byte aligned" in err()
        for gamma in (nan, inf, -inf):
            assert entry(gamma=gamma) < 0 and b"gamma must be finite" in err() and name in err(), gamma
        # the order: table, action, after together, after aligned, score, (epsilon,) gamma
        assert entry(table=None, action=None) < 0 and b"table" in err()
        assert entry(action=None, after_a=None) < 0 and b"action" in err()
        assert entry(after_a=None, after_b=fake + 4) < 0 and b"go together" in err()
        assert entry(after_b=fake + 4, score=fake + 2) < 0 and b"16-byte aligned" in err()
        assert entry(score=fake + 2, gamma=nan) < 0 and b"4-byte aligned" in err()
    for entry in (act, search):
        assert entry(value=fake + 2) < 0 and b"score and value must be 4-byte aligned" in err()
        for epsilon in (-0.001, 1.001, nan, inf):
            assert entry(epsilon=epsilon) < 0 and b"epsilon must be in [0, 1]" in err(), epsilon
        assert entry(score=fake + 2, epsilon=2.0) < 0 and b"4-byte aligned" in err()
        assert entry(epsilon=2.0, gamma=nan) < 0 and b"epsilon" in err()
    for depth in (0, -1, 12):
        assert beam(depth=depth) < 0 and b"depth must be in [1, 11]" in err() and b"tpl_ntuple_beam_sum:" in err(), depth
    for width in (0, -1, 65):
        assert beam(width=width) < 0 and b"width must be in [1, 64]" in err(), width
    assert beam(gamma=nan, depth=0) < 0 and b"gamma" in err()
    assert beam(depth=0, width=0) < 0 and b"depth" in err()
    # the twins keep their own names, and the _shaped entries and the beam keep refusing a third shape
    assert lib.tpl_ntuple_value(None, fake, 4, 2, 2, fake, fake, None) < 0 and b"tpl_ntuple_value:" in err()
    assert lib.tpl_ntuple_value_shaped(fake, fake, 4, 2, 2, fake, fake, 2, None) < 0 and b"shape" in err()
    assert lib.tpl_ntuple_beam(fake, fake, 4, 2, 2, 0.0, 1.0, 0.0, 0.99, fake, 3, 8, fake, None, None, None, None, 2, None) < 0
    assert b"shape" in err() and b"tpl_ntuple_beam:" in err()


# ------------------------------------------------------------------------------------------------ 8. Python
def test_the_python_refusals():
    N = T.ntuple
    assert N.ntuple_shape(N.ntuple_table("cpu", SUM)) == SUM and N.ntuple_shape(N.ntuple_coherence("cpu", SUM)) == SUM
    for shape in ("3x3+2x4", "2x4 + 3x3", "2X4+3X3", "sum", 2, None, ("2x4", "3x3")):
        with pytest.raises(ValueError, match="shape"):
            N.ntuple_table("cpu", shape=shape)
        with pytest.raises(ValueError, match="shape"):
            N.ntuple_coherence("cpu", shape=shape)
        with pytest.raises(ValueError, match="shape"):
            _m().ntuple_indices(np.zeros(20, np.uint16), 0, L, M, 0, 0, shape=shape)
    off = torch.zeros(ENTRIES_SUM + 16, dtype=torch.int32)
    for bad in (off, torch.zeros(ENTRIES_SUM - 1024, dtype=torch.int32), None):
        with pytest.raises(ValueError, match="table"):
            N.ntuple_shape(bad)
        with pytest.raises(ValueError, match="table"):
            N.ntuple_parts(bad)
    planes = (torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32))
    for bad in (off, torch.zeros(ENTRIES_SUM, dtype=torch.int64), torch.zeros(2 * ENTRIES_SUM, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="table"):
            N.ntuple_value(planes, bad, L, M)
        with pytest.raises(ValueError, match="table"):
            N.ntuple_is_symmetric(bad)
    with pytest.raises(ValueError, match="coherence"):
        N.ntuple_step_sizes(torch.zeros((ENTRIES_SUM + 16, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="coherence"):
        N.ntuple_step_sizes(torch.zeros((ENTRIES_SUM, 2), dtype=torch.int32))
    # a coherence buffer goes with a table of its own size only
    for table, buffer in ((SUM, "2x4"), (SUM, "3x3"), ("3x3", SUM), ("2x4", SUM)):
        with pytest.raises(ValueError, match="coherence"):
            N._coherence(N.ntuple_coherence("cpu", buffer), N.ntuple_table("cpu", table))
    assert N._coherence(N.ntuple_coherence("cpu", SUM), N.ntuple_table("cpu", SUM)) is not None
    assert (N.ntuple_step_sizes(N.ntuple_coherence("cpu", SUM)) == 1.0).all()
    sums = N.ntuple_coherence("cpu", SUM)
    sums[ENTRIES_2X4 + 5] = torch.tensor([-3, 4])
    alpha = N.ntuple_step_sizes(sums)
    assert tuple(alpha.shape) == (ENTRIES_SUM,) and float(alpha[ENTRIES_2X4 + 5]) == 0.75 and int((alpha != 1.0).sum()) == 1
