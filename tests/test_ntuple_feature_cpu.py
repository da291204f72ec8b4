"""Feature tuples without a GPU (include/tpl_learn.h's "Feature tuples"; the _feature entries of csrc/learn/ntuple.hip and
ntuple_beam.hip; _learn_lib.py's numpy mirror; ntuple.py):

  1. LAYOUT: 19,456 and 610,304 entries, the header's constants, no collision with a plain or staged count, the pinned registries as
     they were, every declared symbol exported, no scratch in any n-tuple kernel;
  2. MIRROR: the feature columns are (p * 9 + j) * 256 + min(phi_j, 255) on the 8,192 boards of random_moves.npz; the comb board reads
     wells bin 255, the empty board bin 0 in seven features, 40 in row_transitions and 10 in column_transitions;
  3. SYMMETRY: the features are reflection-invariant on those boards; sigma moves only the piece; a symmetric trace update leaves
     table[sigma] == table, and then a board and its reflection under the mirrored piece have the same value bits; the sum form does
     the same with each part under its own sigma;
  4. SUM: one part zero gives the other part's bits; both filled is one rounding of the integer sum, with a seed searched for on which
     rounding each part first differs;
  5. REFUSALS: every argument refusal of the six entries as a status under the entry's own name, `form` first; the Python refusals.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden

import tetris_piclim as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, M = 10, 40
E3, EF, E3F = 590848, 19456, 610304
FEAT, BOTH = "feat", "3x3+feat"
PI = (0, 2, 1, 3, 5, 4, 6, 7)
ENTRIES = ("tpl_ntuple_value_feature", "tpl_ntuple_act_feature", "tpl_ntuple_search_feature", "tpl_ntuple_beam_feature",
           "tpl_ntuple_update_trace_feature", "tpl_ntuple_feature_bins")


def _m():
    return T._learn_lib


def _golden():
    """The 8,192 boards of random_moves.npz, inputs then outputs, with a piece, lines and moves each."""
    g = load_golden("random_moves.npz")
    rows = np.concatenate([g["rows"], g["o_rows"]]).astype(np.uint16)
    gen = np.random.default_rng(0)
    k = rows.shape[0]
    assert k == 8192
    return rows, gen.integers(0, 8, k), gen.integers(0, 12, k), gen.integers(0, 45, k)


def _comb():
    rows = np.zeros(20, np.uint16)
    rows[1:] = 0b0101010101
    return rows


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. layout
def test_the_layout_the_constants_and_the_registries():
    m = _m()
    assert m.NTUPLE_FEATURE_FORMS == {FEAT: 0, BOTH: 1} and T.NTUPLE_FEATURE_FORMS is m.NTUPLE_FEATURE_FORMS
    assert m.NTUPLE_FEATURES == 9 and m.NTUPLE_FEATURE_BINS == 256
    assert m.NTUPLE_ENTRIES_FEAT == EF == 8 * 9 * 256 + 1024 and m.NTUPLE_ENTRIES_3X3_FEAT == E3F == E3 + EF
    assert EF % 512 == 0 and E3F % 512 == 0 and (4 * E3) % 16 == 0
    assert m.ntuple_entries_of(FEAT) == EF and m.ntuple_entries_of(BOTH) == E3F
    assert m.ntuple_parts_of(FEAT) == (FEAT,) and m.ntuple_parts_of(BOTH) == ("3x3", FEAT)
    assert m.ntuple_shape_of(EF) == FEAT and m.ntuple_shape_of(E3F) == BOTH
    # the header's constants are the Python ones
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)\s", raw).group(1))
    assert define("TPL_NTUPLE_ENTRIES_FEAT") == EF and define("TPL_NTUPLE_ENTRIES_3X3_FEAT") == E3F
    assert define("TPL_NTUPLE_FEATURES") == 9 and define("TPL_NTUPLE_FEATURE_BINS") == 256
    assert define("TPL_NTUPLE_FEATURE_FORM_ALONE") == m.NTUPLE_FEATURE_FORMS[FEAT] == 0
    assert define("TPL_NTUPLE_FEATURE_FORM_3X3") == m.NTUPLE_FEATURE_FORMS[BOTH] == 1
    # the new counts collide with no plain, staged or coherence count, and the pinned registries are as they were
    assert not {EF, E3F} & (set(m._ntuple_counts()) | set(m._ntuple_staged_counts()))
    assert set(m.NTUPLE_SHAPES) == {"2x4", "3x3"} and m.NTUPLE_SHAPE_IDS == {"2x4": 0, "3x3": 1}
    assert m.NTUPLE_SUMS == {"2x4+3x3": ("2x4", "3x3")} and m.NTUPLE_FORM_IDS == {"2x4": 0, "3x3": 1, "2x4+3x3": 2}
    assert set(m._ntuple_counts()) == {314368, 590848, 905216}
    # the public functions by name and by entry count
    for name, entries in ((FEAT, EF), (BOTH, E3F)):
        table = T.ntuple_table("cpu", name)
        assert tuple(table.shape) == (entries,) and table.dtype == torch.int32 and int(table.abs().sum()) == 0
        assert T.ntuple_shape(table) == name and not T.ntuple_is_staged(table) and T.ntuple_is_symmetric(table)
    parts = T.ntuple_parts(T.ntuple_table("cpu", BOTH))
    assert [p.shape[0] for p in parts] == [E3, EF] and [T.ntuple_shape(p) for p in parts] == ["3x3", FEAT]
    assert parts[1].data_ptr() - parts[0].data_ptr() == 4 * E3 and len(T.ntuple_parts(T.ntuple_table("cpu", FEAT))) == 1


def test_every_declared_symbol_is_exported_and_no_ntuple_kernel_uses_scratch():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and set(ENTRIES) <= declared
    lib = ctypes.CDLL(_m().build_library())
    for name in _m().LEARN_SYMBOLS:
        assert hasattr(lib, name), name
    names = lambda entry: [a.split()[-1].lstrip("*") for a in re.search(rf"int {entry}\((.*?)\);", text, flags=re.S).group(1).split(",")]
    for entry, twin in (("tpl_ntuple_value_feature", "tpl_ntuple_value_shaped"), ("tpl_ntuple_act_feature", "tpl_ntuple_act_shaped"),
                        ("tpl_ntuple_search_feature", "tpl_ntuple_search_shaped"), ("tpl_ntuple_beam_feature", "tpl_ntuple_beam")):
        assert names(entry) == ["form" if a == "shape" else a for a in names(twin)], entry
    assert names("tpl_ntuple_update_trace_feature") == [a for a in names("tpl_ntuple_update_trace_shaped") if a != "shape"]
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _m().build_library()], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    field = lambda r, name: int(r[r.index(name) - 1])
    mine = [r for r in rows if "feature" in r[-1] and "ntuple" in r[-1]]
    for r in mine:
        print(" ".join(r))
    reads = [k for k in ("ntuple_feature_value_kernel", "ntuple_feature3_value_kernel", "ntuple_feature_act_kernel",
                         "ntuple_feature3_act_kernel", "ntuple_feature_search_kernel", "ntuple_feature3_search_kernel",
                         "ntuple_feature_beam_kernel", "ntuple_feature3_beam_kernel", "ntuple_feature_bins_kernel",
                         "ntuple_feature_trace_kernelILb0", "ntuple_feature_trace_kernelILb1")]
    for kernel in reads:
        assert sum(kernel in r[-1] for r in mine) == 1, kernel
    assert all(field(r, "scratch") == 0 for r in rows if "ntuple" in r[-1])


# ------------------------------------------------------------------------------------------------ 2. the mirror
def test_the_feature_columns_are_the_clamped_board_features_under_the_piece():
    m = _m()
    rows, piece, lines, moves = _golden()
    index, used = m.ntuple_indices(rows, piece, L, M, lines, moves, shape=FEAT)
    phi = m.board_features(rows)
    assert index.shape == used.shape == (8192, 10) and index.dtype == np.int64 and used.all()
    want = (piece[:, None] * 9 + np.arange(9)[None, :]) * 256 + np.minimum(phi, 255)
    assert np.array_equal(index[:, :9], want) and index[:, :9].max() < 18432
    assert np.array_equal(index[:, 9], 18432 + m.ntuple_counter_index(L, M, lines, moves))
    assert (phi.max(axis=0) > 0).all()                         # every feature takes part on this set
    both, used_both = m.ntuple_indices(rows, piece, L, M, lines, moves, shape=BOTH)
    i3, u3 = m.ntuple_indices(rows, piece, L, M, lines, moves, shape="3x3")
    assert both.shape == (8192, 145 + 10) and np.array_equal(both[:, :145], i3) and np.array_equal(both[:, 145:], index + E3)
    assert np.array_equal(used_both[:, :145], u3) and used_both[:, 145:].all()
    assert m._counter_columns(FEAT) == [9] and m._counter_columns(BOTH) == [144, 154]


def test_the_comb_board_reads_the_last_wells_bin_and_the_empty_board_the_wall_and_floor_terms():
    m = _m()
    phi = m.board_features(_comb())[0]
    assert phi[6] == 950                                       # wells: five wells of depth 19, 19 * 20 / 2 each
    for p in range(8):
        index, used = m.ntuple_indices(_comb(), p, L, M, 0, 0, shape=FEAT)
        assert used.all() and index[0, 6] == (p * 9 + 6) * 256 + 255
        assert np.array_equal(index[0, :9] % 256, np.minimum(phi, 255))
        # the empty board: 20 rows of two wall transitions each, ten columns of one floor transition each, nothing else
        empty, used = m.ntuple_indices(np.zeros(20, np.uint16), p, L, M, 0, 0, shape=FEAT)
        assert used.all() and (empty[0, :9] % 256).tolist() == [0, 0, 0, 0, 40, 10, 0, 0, 0]
        assert (empty[0, :9] // 256).tolist() == [p * 9 + j for j in range(9)]
    # a table that holds 1 at the clamped bin alone: the comb's value sees it, a wells count of 254 would not
    table = np.zeros(EF, np.int32)
    table[(3 * 9 + 6) * 256 + 255] = 1 << 16
    assert m.ntuple_value(table, _comb(), 3, L, M, 0, 0, 0)[0] == 1.0 and m.ntuple_value(table, _comb(), 2, L, M, 0, 0, 0)[0] == 0.0


# ------------------------------------------------------------------------------------------------ 3. symmetry
def test_the_features_are_invariant_under_reflection_and_sigma_moves_only_the_piece():
    m = _m()
    rows, piece, lines, moves = _golden()
    assert np.array_equal(m.board_features(m._reflected_rows(rows)), m.board_features(rows))
    assert (m._reflected_rows(rows) != rows).any(axis=1).mean() > 0.9
    sigma = m.ntuple_mirror_permutation(FEAT)
    assert sigma.shape == (EF,) and np.array_equal(sigma[sigma], np.arange(EF))
    assert np.array_equal(sigma[18432:], np.arange(18432, EF))
    j = np.arange(18432)
    assert np.array_equal(sigma[:18432], np.array(PI)[j // 2304] * 2304 + j % 2304)
    assert set((np.flatnonzero(sigma[:18432] == j) // 2304).tolist()) == {0, 3, 6, 7}
    both = m.ntuple_mirror_permutation(BOTH)
    assert np.array_equal(both[:E3], m.ntuple_mirror_permutation("3x3")) and np.array_equal(both[E3:], sigma + E3)
    assert np.array_equal(both[both], np.arange(E3F))


def _ages(seed, k, horizon):
    gen = np.random.default_rng(seed)
    rows, piece, lines, moves = _golden()
    out = []
    for _ in range(horizon):
        at = gen.integers(0, rows.shape[0], k)
        state = np.where(gen.random(k) < 0.2, gen.integers(1, 4, k), 0)
        out.append((rows[at], piece[at], lines[at], moves[at], state))
    return out


def _errors(seed, k):
    error = np.random.default_rng(seed).normal(size=k).astype(np.float32)
    error[:4] = np.array([0.0, np.nan, 1e9, -1e9], np.float32)
    return error


@pytest.mark.parametrize("shape", [FEAT, BOTH])
def test_a_symmetric_trace_update_leaves_a_symmetric_table_that_values_a_board_and_its_reflection_alike(shape):
    m, k = _m(), 200
    entries = m.ntuple_entries_of(shape)
    ages, error = _ages(3, k, 3), _errors(4, k)
    sigma = m.ntuple_mirror_permutation(shape)
    for symmetric in (False, True):
        table = m.ntuple_update_trace(np.zeros(entries, np.int32), ages, L, M, error, 3000.0, 0.7, symmetric)
        assert np.array_equal(table[sigma], table) == symmetric and np.count_nonzero(table[-EF:-1024]) > 100
        assert np.count_nonzero(table[-1024:]) > 0
    # the update of a sum form is the update of each part
    if shape == BOTH:
        want = np.zeros(entries, np.int32)
        want[:E3] = m.ntuple_update_trace(np.zeros(E3, np.int32), ages, L, M, error, 3000.0, 0.7, True)
        want[E3:] = m.ntuple_update_trace(np.zeros(EF, np.int32), ages, L, M, error, 3000.0, 0.7, True)
        assert np.array_equal(table, want)
    # every feature add is made twice under a self-mirror piece: a single state under O
    rows = _golden()[0][5000]
    one = [(rows[None], np.array([6]), np.array([1]), np.array([2]), np.array([0]))]
    once = m.ntuple_update_trace(np.zeros(EF, np.int32), one, L, M, np.array([1.0], np.float32), 8.0, 0.0, False)
    twice = m.ntuple_update_trace(np.zeros(EF, np.int32), one, L, M, np.array([1.0], np.float32), 8.0, 0.0, True)
    assert sorted(once[once != 0].tolist()) == [8] * 10 and sorted(twice[twice != 0].tolist()) == [8] + [16] * 9
    assert twice[-1024:].sum() == 8                            # the counter is added once
    # under the symmetric table a board and its reflection with the mirrored piece have the same value bits
    rows, piece, lines, moves = _golden()
    v = m.ntuple_value(table, rows, piece, L, M, lines, moves, 0)
    vm = m.ntuple_value(table, m._reflected_rows(rows), np.array(PI)[piece], L, M, lines, moves, 0)
    assert np.array_equal(_bits(v), _bits(vm)) and (v != 0).mean() > 0.5
    torch_table = torch.from_numpy(table)
    assert T.ntuple_is_symmetric(torch_table)
    broken = torch_table.clone()
    broken[entries - EF + 2304 + 5] += 1                        # piece 1 (L), whose image is piece 2 (J)
    assert not T.ntuple_is_symmetric(broken)


# ------------------------------------------------------------------------------------------------ 4. the sum
def test_the_value_of_the_sum_form_is_one_rounding_of_the_integer_sum():
    m = _m()
    rows, piece, lines, moves = _golden()
    rows, piece, lines, moves = rows[::16], piece[::16], lines[::16], moves[::16]
    k = rows.shape[0]
    state = np.where(np.arange(k) % 5 == 4, 2, 0)
    run = state == 0
    args = (rows, piece, L, M, lines, moves)
    scale = np.float32(2.0 ** -16)
    i3, u3 = m.ntuple_indices(*args, shape="3x3")
    jf, _ = m.ntuple_indices(*args, shape=FEAT)
    found = None
    for seed in range(20):                                     # a seed on which rounding each part first gives another value
        table = np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, E3F).astype(np.int32)
        first, second = table[:E3], table[E3:]
        sa = np.where(u3, first[i3].astype(np.int64), 0).sum(axis=1)
        sb = second[jf].astype(np.int64).sum(axis=1)
        want = np.where(run, (sa + sb).astype(np.float32) * scale, np.float32(0.0)).astype(np.float32)
        got = m.ntuple_value(table, *args, state)
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), seed
        exact = [np.float32(int(a) + int(b)) * scale for a, b in zip(sa.tolist(), sb.tolist())]          # Python integers
        assert np.array_equal(_bits(np.array(exact, np.float32)[run]), _bits(got[run]))
        twice = (sa.astype(np.float32) + sb.astype(np.float32)) * scale
        differ = (_bits(twice) != _bits(want)) & run
        if differ.any():
            found = (seed, int(differ.sum()))
            break
    print("rounding each part first differs on (seed, boards):", found)
    assert found is not None
    assert (_bits(got)[~run] == 0).all()
    # one part zero: the bits of the other part alone
    only3, onlyf = np.zeros(E3F, np.int32), np.zeros(E3F, np.int32)
    only3[:E3], onlyf[E3:] = first, second
    assert np.array_equal(_bits(m.ntuple_value(only3, *args, state)), _bits(m.ntuple_value(np.ascontiguousarray(first), *args, state)))
    assert np.array_equal(_bits(m.ntuple_value(onlyf, *args, state)), _bits(m.ntuple_value(np.ascontiguousarray(second), *args, state)))
    alone = m.ntuple_value(np.ascontiguousarray(second), *args, state)
    assert np.array_equal(_bits(alone[run]), _bits((sb.astype(np.float32) * scale)[run])) and (alone[run] != 0).all()
    # the plain update of a feature table: ten adds a running state, wrapping
    start = np.full(EF, (1 << 31) - 1, np.int32)
    left = m.ntuple_update(start.copy(), *args, state, np.full(k, 1.0, np.float32), 3.0)
    assert (left != start).sum() > 50 and (left[left != start] < 0).all()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_every_refusal_of_the_feature_entries_comes_back_as_a_status_with_the_form_first():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")

    def value(a=fake, b=fake, n=4, L=2, M=2, table=fake, value=fake, form=0):
        return lib.tpl_ntuple_value_feature(a, b, n, L, M, table, value, form, None)

    def act(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
            value=fake, form=1):
        return lib.tpl_ntuple_act_feature(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, score, after_a, after_b,
                                          value, form, None)

    def search(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
               value=fake, form=0):
        return lib.tpl_ntuple_search_feature(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, fake + 1, score,
                                             after_a, after_b, value, form, None)

    def beam(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, depth=3, width=8, action=fake, after_a=fake, after_b=fake,
             score=fake, form=1):
        return lib.tpl_ntuple_beam_feature(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, depth, width, action, fake + 1, score, after_a,
                                           after_b, form, None)

    def update(a=fake, b=fake, n=4, slots=5, head=2, horizon=4, L=2, M=2, table=fake, error=fake, rate=1.0, decay=0.5):
        return lib.tpl_ntuple_update_trace_feature(a, b, n, slots, head, horizon, L, M, table, error, rate, decay, 1, None)

    def bins(a=fake, b=fake, n=4, out=fake):
        return lib.tpl_ntuple_feature_bins(a, b, n, out, None)

    formed = ((value, b"tpl_ntuple_value_feature:"), (act, b"tpl_ntuple_act_feature:"), (search, b"tpl_ntuple_search_feature:"),
              (beam, b"tpl_ntuple_beam_feature:"))
    for entry, name in formed:                                 # the form first, before any pointer is looked at
        for form in (2, -1, 3, 1 << 20):
            assert entry(form=form) < 0 and b"form must be" in err() and name in err(), form
            assert entry(a=None, n=0, table=None, form=form) < 0 and b"form must be" in err()
        for form in (0, 1):
            assert entry(a=None, form=form) < 0 and b"null" in err() and b"form" not in err()
    limit = -(-(1 << 31) // 40)
    for entry, name in formed + ((update, b"tpl_ntuple_update_trace_feature:"), (bins, b"tpl_ntuple_feature_bins:")):
        assert entry(a=None) < 0 and b"null" in err() and name in err()
        assert entry(b=None) < 0 and b"null" in err() and name in err()
        for n in (0, -1):
            assert entry(n=n) < 0 and b"positive" in err() and name in err(), n
        for n in (limit, 1 << 40):
            assert entry(n=n) < 0 and b"2^31" in err() and name in err(), n
        for plane in ("a", "b"):
            assert entry(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err()
        if entry is bins:
            continue
        for L_, M_ in ((0, 2), (2, 256), (251, 2), (2, 255), (2, 0)):
            assert entry(L=L_, M=M_) < 0 and b"L and M" in err() and name in err(), (L_, M_)
        assert entry(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
        for off in (4, 8, 12):
            assert entry(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
        assert entry(a=None, n=0, L=0, table=None) < 0 and b"null" in err() and b"table" not in err()
        assert entry(n=0, L=0, table=None) < 0 and b"positive" in err()
        assert entry(L=0, table=None) < 0 and b"L and M" in err()
    assert bins(out=None) < 0 and b"null" in err() and b"bins" in err()
    assert value(value=None) < 0 and b"null" in err() and b"value" in err() and b"tpl_ntuple_value_feature:" in err()
    assert value(value=fake + 2) < 0 and b"value must be 4-byte aligned" in err()
    assert value(table=None, value=None) < 0 and b"table" in err()
    for entry, name in formed[1:]:
        assert entry(action=None) < 0 and b"null" in err() and b"action" in err() and name in err()
        assert entry(after_a=None) < 0 and b"go together" in err() and name in err()
        assert entry(after_b=fake + 4) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
        assert entry(score=fake + 2) < 0 and b"4-byte aligned" in err()
        for gamma in (nan, inf, -inf):
            assert entry(gamma=gamma) < 0 and b"gamma must be finite" in err() and name in err(), gamma
        assert entry(table=None, action=None) < 0 and b"table" in err()
        assert entry(action=None, after_a=None) < 0 and b"action" in err()
        assert entry(after_a=None, after_b=fake + 4) < 0 and b"go together" in err()
        assert entry(after_b=fake + 4, score=fake + 2) < 0 and b"16-byte aligned" in err()
        assert entry(score=fake + 2, gamma=nan) < 0 and b"4-byte aligned" in err()
    for entry in (act, search):
        assert entry(value=fake + 2) < 0 and b"score and value must be 4-byte aligned" in err()
        for epsilon in (-0.001, 1.001, nan, inf):
            assert entry(epsilon=epsilon) < 0 and b"epsilon must be in [0, 1]" in err(), epsilon
        assert entry(epsilon=2.0, gamma=nan) < 0 and b"epsilon" in err()
    for depth in (0, -1, 12):
        assert beam(depth=depth) < 0 and b"depth must be in [1, 11]" in err() and b"tpl_ntuple_beam_feature:" in err(), depth
    for width in (0, -1, 65):
        assert beam(width=width) < 0 and b"width must be in [1, 64]" in err(), width
    assert beam(gamma=nan, depth=0) < 0 and b"gamma" in err()
    assert beam(depth=0, width=0) < 0 and b"depth" in err()
    # the update: error, rate, then the ring
    assert update(error=None) < 0 and b"null" in err() and b"error" in err()
    assert update(error=fake + 2) < 0 and b"error must be 4-byte aligned" in err()
    for rate in (nan, inf, -inf):
        assert update(rate=rate) < 0 and b"rate must be finite" in err(), rate
    for slots in (0, -1, 18):
        assert update(slots=slots, head=0, horizon=1) < 0 and b"slots must be in [1, 17]" in err(), slots
    for head in (-1, 5):
        assert update(head=head) < 0 and b"head must be in [0, slots)" in err(), head
    for horizon in (0, 6):
        assert update(horizon=horizon) < 0 and b"horizon must be in" in err(), horizon
    assert update(slots=17, head=0, horizon=17) < 0 and b"horizon must be in" in err()
    assert update(n=limit // 4, slots=5) < 0 and b"40 * slots * n" in err()
    for decay in (-0.1, 1.1, nan):
        assert update(decay=decay) < 0 and b"decay must be in [0, 1]" in err(), decay
    assert update(table=None, error=None) < 0 and b"table" in err()
    assert update(error=None, rate=nan) < 0 and b"error" in err()
    assert update(rate=nan, slots=0) < 0 and b"rate" in err()
    # the existing entries keep refusing what they refused
    assert lib.tpl_ntuple_value_shaped(fake, fake, 4, 2, 2, fake, fake, 2, None) < 0 and b"shape" in err()
    assert lib.tpl_ntuple_value_staged(fake, fake, 4, 2, 2, fake, fake, 3, None) < 0 and b"form" in err()
    assert lib.tpl_ntuple_beam(fake, fake, 4, 2, 2, 0.0, 1.0, 0.0, 0.99, fake, 3, 8, fake, None, None, None, None, 2, None) < 0
    assert b"shape" in err() and b"tpl_ntuple_beam:" in err()


class _Env:
    """What NTupleLearner looks at before it allocates anything."""
    num_envs, auto_reset, L, M = 8, True, 2, 2
    device = torch.device("cpu")


def test_the_python_refusals():
    N = T.ntuple
    for shape in (FEAT, BOTH):
        with pytest.raises(ValueError, match="no staged form"):
            N.ntuple_table("cpu", shape, staged=True)
        with pytest.raises(ValueError, match="no coherence buffer"):
            N.ntuple_coherence("cpu", shape=shape)
        with pytest.raises(ValueError, match="no staged form"):
            N.ntuple_staged(N.ntuple_table("cpu", shape), N.ntuple_stage_map(10, 40))
        with pytest.raises(ValueError, match="coherent"):
            N.NTupleLearner(_Env(), shape=shape, coherent=True)
        with pytest.raises(ValueError, match="stage_map"):
            N.NTupleLearner(_Env(), shape=shape, stage_map=N.ntuple_stage_map(10, 40))
    for shape in ("feat+3x3", "features", "FEAT", 0, None):
        with pytest.raises(ValueError, match="shape"):
            N.ntuple_table("cpu", shape=shape)
        with pytest.raises(ValueError, match="shape"):
            _m().ntuple_indices(np.zeros(20, np.uint16), 0, L, M, 0, 0, shape=shape)
    planes = (torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32))
    for bad in (torch.zeros(EF + 16, dtype=torch.int32), torch.zeros(EF, dtype=torch.int64), torch.zeros(2 * E3F, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="table"):
            N.ntuple_value(planes, bad, L, M)
        with pytest.raises(ValueError, match="table"):
            N.ntuple_is_symmetric(bad)
    with pytest.raises(ValueError, match="table"):
        N.ntuple_shape(torch.zeros((EF, 2), dtype=torch.int64))                 # no coherence buffer has a feature form's count
    with pytest.raises(ValueError, match="source"):
        N.ntuple_feature_bins((torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64)))
