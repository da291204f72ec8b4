"""The budget table and the dead-board prune without a GPU (include/tpl_learn.h's "The budget table"; the _budget entries of
csrc/learn/ntuple.hip and ntuple_beam.hip; _learn_lib.py's numpy mirror; ntuple.py):

  1. THE FEATURE IS THERE: "feat+spare" has 21,504 entries by name and by count -- the first assertion, which the code before this form
     fails --, a registry of its own beside the pinned ones, the header's constants and the rule in the header's words;
  2. THE MIRROR IS THE DEFINITION: row 9 of ntuple_indices is sbin restated plainly, cell by cell in Python integers, on random boards
     under games up to L = 250 and M = 254, dead, live and clamped boards among them; columns 0 .. 8 are the feature table's, column
     10 the counter; the clamps of the issue: spare 380 -> bin 255, spare 200 -> bin 201 where the clamped counters would give 103;
  3. VALUE, SYMMETRY, PROMOTION: eleven entries, one rounding; spare is reflection-invariant, sigma moves only the piece, a symmetric
     update leaves table[sigma] == table; ntuple_budget(feat) has row 9 zero and the mirror values it as the source, bit for bit;
  4. REFUSALS: every argument refusal of the six entries as a status under the entry's own name; the Python refusals, bound=True on any
     other form among them, with a message that names "feat+spare";
  5. every declared symbol is exported, the six kernels are in the library and none uses scratch.
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
BUDGET, FEAT = "feat+spare", "feat"
EB, EF = 21504, 19456
PI = (0, 2, 1, 3, 5, 4, 6, 7)
ENTRIES = ("tpl_ntuple_value_budget", "tpl_ntuple_act_budget", "tpl_ntuple_search_budget", "tpl_ntuple_beam_budget",
           "tpl_ntuple_update_trace_budget", "tpl_ntuple_budget_bins")


def _m():
    return T._learn_lib


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the feature is there
def test_the_form_exists_by_name_and_by_count_and_the_header_states_the_rule():
    m = _m()
    assert m.ntuple_entries_of(BUDGET) == EB == 8 * 10 * 256 + 1024          # raises before this form existed
    table = T.ntuple_table("cpu", BUDGET)                                    # and so does this
    assert tuple(table.shape) == (EB,) and table.dtype == torch.int32 and int(table.abs().sum()) == 0
    assert T.ntuple_shape(table) == BUDGET and not T.ntuple_is_staged(table) and T.ntuple_is_symmetric(table)
    assert len(T.ntuple_parts(table)) == 1 and T.ntuple_parts(table)[0].data_ptr() == table.data_ptr()
    assert m.NTUPLE_BUDGET_FORMS == {BUDGET: 0} and T.NTUPLE_BUDGET_FORMS is m.NTUPLE_BUDGET_FORMS
    assert m.NTUPLE_BUDGET_ROWS == 10 and m.NTUPLE_ENTRIES_BUDGET == EB and 4 * EB == 86016
    assert m.ntuple_parts_of(BUDGET) == (BUDGET,) and m.ntuple_shape_of(EB) == BUDGET and m.ntuple_form_of(EB) == (BUDGET, False)
    assert m._counter_columns(BUDGET) == [10]
    # no other form has this count, and the pinned registries are as they were
    others = set(m._ntuple_counts()) | set(m._ntuple_staged_counts()) | set(m._ntuple_feature_counts())
    assert EB not in others and set(m._ntuple_budget_counts()) == {EB}
    assert set(m.NTUPLE_SHAPES) == {"2x4", "3x3"} and m.NTUPLE_SUMS == {"2x4+3x3": ("2x4", "3x3")}
    assert m.NTUPLE_FEATURE_FORMS == {FEAT: 0, "3x3+feat": 1} and set(m._ntuple_feature_counts()) == {EF, 610304}
    for name in ("NTUPLE_BUDGET_FORMS", "ntuple_budget", "ntuple_budget_bins"):
        assert name in T.__all__ and name in T.ntuple.__all__ and getattr(T, name) is getattr(T.ntuple, name)
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)\s", raw).group(1))
    assert define("TPL_NTUPLE_ENTRIES_BUDGET") == EB and define("TPL_NTUPLE_BUDGET_ROWS") == 10
    flat = " ".join(raw.split())
    for words in ("sbin = dead ? 0 : min(spare + 1, 255)", "spare = 4 (M - moves) - cells", "dead = spare < 0", "21,504",
                  "BOTH CLAMPS ARE * PART OF THE RULE", "never from the clamped counter index k", "THE PRUNE",
                  "after_a / after_b and `value` stay the true"):
        assert words in flat, words
    assert flat.index("Feature tuples: n-tuple tables") < flat.index("The budget table:")


# ------------------------------------------------------------------------------------------------ 2. the mirror is the definition
def _plain_sbin(rows, L, M, lines, moves):
    """sbin from the definition's words, a board at a time in Python integers."""
    out = []
    for board, l, mv in zip(rows.tolist(), lines.tolist(), moves.tolist()):
        cost = []
        for mask in board:
            fill = bin(mask & 0x3FF).count("1")
            cost.append(10 - fill if fill < 10 else 10)
        owed = max(L - l, 0)
        cost = sorted(cost) + [10] * max(owed - 20, 0)
        cells = sum(cost[:owed])
        spare = 4 * (M - mv) - cells
        out.append(0 if spare < 0 else min(spare + 1, 255))
    return np.array(out, np.int64)


def _random_boards(gen, k):
    """k boards in row form: a stack of random height, each row filled with its own density, some rows full and some nearly so."""
    height = gen.integers(0, 21, k)
    density = gen.random((k, 20)) ** 0.5
    cell = gen.random((k, 20, 10)) < density[:, :, None]
    cell[gen.random((k, 20)) < 0.08] = True                                   # full rows, which cost what a fresh row costs
    cell &= (np.arange(20)[None, :] >= 20 - height[:, None])[:, :, None]
    return (cell * (1 << np.arange(10))[None, None, :]).sum(axis=2).astype(np.uint16)


@pytest.mark.parametrize("L,M", [(1, 1), (2, 100), (5, 8), (10, 16), (10, 40), (20, 100), (37, 254), (250, 254), (250, 63), (16, 64)])
def test_row_nine_is_the_definition_restated_on_random_boards(L, M):
    m, k = _m(), 400
    gen = np.random.default_rng(1000 * L + M)
    rows = _random_boards(gen, k)
    piece, lines, moves = gen.integers(0, 8, k), gen.integers(0, L + 4, k), gen.integers(0, M, k)
    index, used = m.ntuple_indices(rows, piece, L, M, lines, moves, shape=BUDGET)
    assert index.shape == used.shape == (k, 11) and index.dtype == np.int64 and used.all()
    want = _plain_sbin(rows, L, M, lines, moves)
    assert np.array_equal(index[:, 9], (piece * 10 + 9) * 256 + want)
    assert np.array_equal(m.spare_bins(rows, L, M, lines, moves), want)
    phi = m.board_features(rows)
    assert np.array_equal(index[:, :9], (piece[:, None] * 10 + np.arange(9)[None, :]) * 256 + np.minimum(phi, 255))
    assert np.array_equal(index[:, 10], 20480 + m.ntuple_counter_index(L, M, lines, moves))
    assert index.min() >= 0 and index[:, :10].max() < 20480 and index[:, 10].max() < EB          # no state addresses outside
    # the feature columns are the feature table's under the other piece stride
    feat, _ = m.ntuple_indices(rows, piece, L, M, lines, moves, shape=FEAT)
    assert np.array_equal(index[:, :9] % 256, feat[:, :9] % 256) and np.array_equal(index[:, 10] - 20480, feat[:, 9] - 18432)
    # the bins of every state, running or not: a finished board has spare 0 and is not dead
    state = gen.integers(0, 4, k)
    bins = m.ntuple_budget_bins(rows, L, M, lines, moves, state)
    assert bins.shape == (k, 10) and bins.dtype == np.uint8
    assert np.array_equal(bins[:, 9], np.where(state == 0, want, 1)) and np.array_equal(bins[:, :9], np.minimum(phi, 255))
    print(f"L = {L}, M = {M}: dead {int((want == 0).sum())}, clamped {int((want == 255).sum())}, bins in use {np.unique(want).size}")


def test_dead_live_and_clamped_boards_are_all_met_and_the_clamps_are_the_issues():
    m = _m()
    seen = set()
    for L, M in ((5, 8), (10, 16), (2, 100), (250, 254)):
        gen = np.random.default_rng(L)
        rows = _random_boards(gen, 400)
        sbin = m.spare_bins(rows, L, M, gen.integers(0, L, 400), gen.integers(0, M, 400))
        seen |= {"dead"} if (sbin == 0).any() else set()
        seen |= {"live"} if ((sbin > 0) & (sbin < 255)).any() else set()
        seen |= {"clamped"} if (sbin == 255).any() else set()
    assert seen == {"dead", "live", "clamped"}
    empty = np.zeros(20, np.uint16)
    # fresh boards: spare = 4 M - 10 L.  (2, 100): 380, the last bin.  (20, 100): 200, bin 201 -- the clamped counters, 15 lines and 63
    # moves left, would give 4 * 63 - 150 = 102 and bin 103
    assert m.move_bound(empty, 2, 100, 0, 0, 0)["spare"][0] == 380 and m.spare_bins(empty, 2, 100, 0, 0)[0] == 255
    assert m.move_bound(empty, 20, 100, 0, 0, 0)["spare"][0] == 200 and m.spare_bins(empty, 20, 100, 0, 0)[0] == 201
    assert m.spare_bins(empty, 15, 63, 0, 0)[0] == 103
    index, _ = m.ntuple_indices(empty, 3, 20, 100, 0, 0, shape=BUDGET)
    assert index[0, 9] == (3 * 10 + 9) * 256 + 201 and index[0, 10] == 20480 + 64 * 15 + 63
    # spare 0 is live and reads bin 1; one cell short is dead and reads bin 0
    assert m.spare_bins(empty, 2, 5, 0, 0)[0] == 1 and m.spare_bins(empty, 2, 5, 0, 1)[0] == 0
    # a table that holds 1 at one spare bin alone sees exactly the boards of that bin
    table = np.zeros(EB, np.int32)
    table[(3 * 10 + 9) * 256 + 201] = 1 << 16
    assert m.ntuple_value(table, empty, 3, 20, 100, 0, 0, 0)[0] == 1.0 and m.ntuple_value(table, empty, 3, 20, 100, 0, 1, 0)[0] == 0.0
    assert m.ntuple_value(table, empty, 2, 20, 100, 0, 0, 0)[0] == 0.0 and m.ntuple_value(table, empty, 3, 20, 100, 0, 0, 2)[0] == 0.0


# ------------------------------------------------------------------------------------------------ 3. value, symmetry, promotion
def _golden():
    g = load_golden("random_moves.npz")
    rows = np.concatenate([g["rows"], g["o_rows"]]).astype(np.uint16)[::4]
    gen = np.random.default_rng(0)
    k = rows.shape[0]
    return rows, gen.integers(0, 8, k), gen.integers(0, 7, k), gen.integers(0, 16, k)


LG, MG = 5, 16                                                 # a game under which the golden boards are dead, live and in between


def test_the_value_is_one_rounding_of_eleven_entries_and_zero_for_a_finished_board():
    m = _m()
    rows, piece, lines, moves = _golden()
    k = rows.shape[0]
    state = np.where(np.arange(k) % 5 == 4, 2, 0)
    table = np.random.default_rng(3).integers(-(1 << 31), 1 << 31, EB).astype(np.int32)
    index, _ = m.ntuple_indices(rows, piece, LG, MG, lines, moves, shape=BUDGET)
    exact = [np.float32(sum(int(table[j]) for j in row)) * np.float32(2.0 ** -16) for row in index.tolist()]
    got = m.ntuple_value(table, rows, piece, LG, MG, lines, moves, state)
    run = state == 0
    assert got.dtype == np.float32 and np.array_equal(_bits(got[run]), _bits(np.array(exact, np.float32)[run]))
    assert (_bits(got)[~run] == 0).all() and (got[run] != 0).all()
    sbin = index[:, 9] % 256
    assert (sbin == 0).sum() > 50 and (sbin > 1).sum() > 50 and np.unique(sbin).size > 20
    # row 9 alone: V is row 9's entry at sbin plus the counter
    only = np.zeros(EB, np.int32)
    only.reshape(-1)[:20480].reshape(8, 10, 256)[:, 9] = table[:20480].reshape(8, 10, 256)[:, 9]
    only[20480:] = table[20480:]
    want = (only[index[:, 9]].astype(np.int64) + only[index[:, 10]]).astype(np.float32) * np.float32(2.0 ** -16)
    assert np.array_equal(_bits(m.ntuple_value(only, rows, piece, LG, MG, lines, moves, 0)), _bits(want))
    # the plain update: eleven adds a running state, wrapping
    start = np.full(EB, (1 << 31) - 1, np.int32)
    left = m.ntuple_update(start.copy(), rows, piece, LG, MG, lines, moves, state, np.full(k, 1.0, np.float32), 3.0)
    assert (left != start).sum() > 50 and (left[left != start] < 0).all()
    one = m.ntuple_update(np.zeros(EB, np.int32), rows[:1], piece[:1], LG, MG, lines[:1], moves[:1], 0, np.ones(1, np.float32), 8.0)
    assert sorted(one[one != 0].tolist()) == [8] * 11


def test_spare_is_reflection_invariant_sigma_moves_only_the_piece_and_a_symmetric_update_keeps_the_table_symmetric():
    m = _m()
    rows, piece, lines, moves = _golden()
    assert np.array_equal(m.spare_bins(m._reflected_rows(rows), LG, MG, lines, moves), m.spare_bins(rows, LG, MG, lines, moves))
    sigma = m.ntuple_mirror_permutation(BUDGET)
    assert sigma.shape == (EB,) and np.array_equal(sigma[sigma], np.arange(EB)) and np.array_equal(sigma[20480:], np.arange(20480, EB))
    j = np.arange(20480)
    assert np.array_equal(sigma[:20480], np.array(PI)[j // 2560] * 2560 + j % 2560)
    k = 300
    gen = np.random.default_rng(9)
    ages = []
    for _ in range(3):
        at = gen.integers(0, rows.shape[0], k)
        ages.append((rows[at], piece[at], lines[at], moves[at], np.where(gen.random(k) < 0.2, gen.integers(1, 4, k), 0)))
    error = gen.normal(size=k).astype(np.float32)
    error[:4] = np.array([0.0, np.nan, 1e9, -1e9], np.float32)
    for symmetric in (False, True):
        table = m.ntuple_update_trace(np.zeros(EB, np.int32), ages, LG, MG, error, 3000.0, 0.7, symmetric)
        assert np.array_equal(table[sigma], table) == symmetric
        spare_row = table[:20480].reshape(8, 10, 256)[:, 9]
        assert np.count_nonzero(spare_row) > 20 and np.count_nonzero(spare_row[:, 0]) > 0 and np.count_nonzero(table[20480:]) > 0
    v = m.ntuple_value(table, rows, piece, LG, MG, lines, moves, 0)
    vm = m.ntuple_value(table, m._reflected_rows(rows), np.array(PI)[piece], LG, MG, lines, moves, 0)
    assert np.array_equal(_bits(v), _bits(vm)) and (v != 0).mean() > 0.5
    torch_table = torch.from_numpy(table)
    assert T.ntuple_is_symmetric(torch_table)
    broken = torch_table.clone()
    broken[2560 + 9 * 256 + 1] += 1                            # piece 1 (L), row 9: its image is piece 2 (J)
    assert not T.ntuple_is_symmetric(broken)
    # a single state under O, symmetric: every row add is made twice, the counter once
    one = [(rows[:1], np.array([6]), np.array([1]), np.array([2]), np.array([0]))]
    twice = m.ntuple_update_trace(np.zeros(EB, np.int32), one, LG, MG, np.array([1.0], np.float32), 8.0, 0.0, True)
    assert sorted(twice[twice != 0].tolist()) == [8] + [16] * 10 and twice[20480:].sum() == 8


def test_a_promoted_feature_table_has_row_nine_zero_and_the_mirror_values_it_as_the_source():
    m = _m()
    rows, piece, lines, moves = _golden()
    feat = np.random.default_rng(4).integers(-(1 << 31), 1 << 31, EF).astype(np.int32)
    out = T.ntuple_budget(torch.from_numpy(feat))
    assert T.ntuple_shape(out) == BUDGET and out.dtype == torch.int32
    got = out.numpy()
    body = got[:20480].reshape(8, 10, 256)
    assert (body[:, 9] == 0).all() and np.array_equal(body[:, :9], feat[:18432].reshape(8, 9, 256)) and np.array_equal(got[20480:], feat[18432:])
    state = np.where(np.arange(rows.shape[0]) % 7 == 3, 1, 0)
    assert np.array_equal(_bits(m.ntuple_value(got, rows, piece, LG, MG, lines, moves, state)),
                          _bits(m.ntuple_value(feat, rows, piece, LG, MG, lines, moves, state)))
    for bad in (torch.zeros(EB, dtype=torch.int32), torch.zeros(EF, dtype=torch.int64), torch.zeros(590848, dtype=torch.int32), feat):
        with pytest.raises(ValueError, match="feat"):
            T.ntuple_budget(bad)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_every_refusal_of_the_budget_entries_comes_back_as_a_status():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")

    def value(a=fake, b=fake, n=4, L=2, M=2, table=fake, value=fake):
        return lib.tpl_ntuple_value_budget(a, b, n, L, M, table, value, None)

    def act(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
            value=fake, prune=1):
        return lib.tpl_ntuple_act_budget(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, score, after_a, after_b,
                                         value, prune, None)

    def search(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
               value=fake, prune=0):
        return lib.tpl_ntuple_search_budget(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, fake + 1, score,
                                            after_a, after_b, value, prune, None)

    def beam(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, depth=3, width=8, action=fake, after_a=fake, after_b=fake,
             score=fake, prune=1):
        return lib.tpl_ntuple_beam_budget(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, depth, width, action, fake + 1, score, after_a,
                                          after_b, prune, None)

    def update(a=fake, b=fake, n=4, slots=5, head=2, horizon=4, L=2, M=2, table=fake, error=fake, rate=1.0, decay=0.5):
        return lib.tpl_ntuple_update_trace_budget(a, b, n, slots, head, horizon, L, M, table, error, rate, decay, 1, None)

    def bins(a=fake, b=fake, n=4, L=2, M=2, out=fake):
        return lib.tpl_ntuple_budget_bins(a, b, n, L, M, out, None)

    reads = ((value, b"tpl_ntuple_value_budget:"), (act, b"tpl_ntuple_act_budget:"), (search, b"tpl_ntuple_search_budget:"),
             (beam, b"tpl_ntuple_beam_budget:"))
    limit = -(-(1 << 31) // 40)
    for entry, name in reads + ((update, b"tpl_ntuple_update_trace_budget:"), (bins, b"tpl_ntuple_budget_bins:")):
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
        assert entry(a=None, n=0, L=0) < 0 and b"null" in err()                 # the twins' order: planes, n, the game
        assert entry(n=0, L=0) < 0 and b"positive" in err()
        if entry is bins:
            continue
        assert entry(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
        for off in (4, 8, 12):
            assert entry(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
        assert entry(L=0, table=None) < 0 and b"L and M" in err()
    assert bins(out=None) < 0 and b"null" in err() and b"bins" in err() and b"tpl_ntuple_budget_bins:" in err()
    assert value(value=None) < 0 and b"null" in err() and b"value" in err() and b"tpl_ntuple_value_budget:" in err()
    assert value(value=fake + 2) < 0 and b"value must be 4-byte aligned" in err()
    assert value(table=None, value=None) < 0 and b"table" in err()
    for entry, name in reads[1:]:
        for prune in (0, 1, 7, -1):                            # the flag is any integer: nothing about it is refused
            assert entry(action=None, prune=prune) < 0 and b"null" in err() and b"action" in err() and name in err()
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
        assert beam(depth=depth) < 0 and b"depth must be in [1, 11]" in err() and b"tpl_ntuple_beam_budget:" in err(), depth
    for width in (0, -1, 65):
        assert beam(width=width) < 0 and b"width must be in [1, 64]" in err(), width
    assert beam(gamma=nan, depth=0) < 0 and b"gamma" in err()
    assert beam(depth=0, width=0) < 0 and b"depth" in err()
    # the update: error, rate, then the ring -- tpl_ntuple_update_trace_feature's, which still refuses them under its own name
    for entry, name in ((update, b"tpl_ntuple_update_trace_budget:"),
                        (lambda **kw: lib.tpl_ntuple_update_trace_feature(*[kw.get(k, v) for k, v in dict(
                            a=fake, b=fake, n=4, slots=5, head=2, horizon=4, L=2, M=2, table=fake, error=fake, rate=1.0, decay=0.5).items()],
                            1, None), b"tpl_ntuple_update_trace_feature:")):
        assert entry(error=None) < 0 and b"null" in err() and b"error" in err() and name in err()
        assert entry(error=fake + 2) < 0 and b"error must be 4-byte aligned" in err()
        for rate in (nan, inf, -inf):
            assert entry(rate=rate) < 0 and b"rate must be finite" in err(), rate
        for slots in (0, -1, 18):
            assert entry(slots=slots, head=0, horizon=1) < 0 and b"slots must be in [1, 17]" in err(), slots
        for head in (-1, 5):
            assert entry(head=head) < 0 and b"head must be in [0, slots)" in err(), head
        for horizon in (0, 6):
            assert entry(horizon=horizon) < 0 and b"horizon must be in" in err(), horizon
        assert entry(slots=17, head=0, horizon=17) < 0 and b"horizon must be in" in err()
        assert entry(n=limit // 4, slots=5) < 0 and b"40 * slots * n" in err() and name in err()
        for decay in (-0.1, 1.1, nan):
            assert entry(decay=decay) < 0 and b"decay must be in [0, 1]" in err(), decay
        assert entry(table=None, error=None) < 0 and b"table" in err()
        assert entry(error=None, rate=nan) < 0 and b"error" in err()
        assert entry(rate=nan, slots=0) < 0 and b"rate" in err()


class _Env:
    """What the policies and the learner look at before they allocate anything."""
    num_envs, auto_reset, L, M = 8, True, 2, 2
    device = torch.device("cpu")


def test_the_python_refusals():
    N = T.ntuple
    with pytest.raises(ValueError, match="no staged form"):
        N.ntuple_table("cpu", BUDGET, staged=True)
    with pytest.raises(ValueError, match="no coherence buffer"):
        N.ntuple_coherence("cpu", shape=BUDGET)
    with pytest.raises(ValueError, match="no staged form"):
        N.ntuple_staged(N.ntuple_table("cpu", BUDGET), N.ntuple_stage_map(10, 40))
    with pytest.raises(ValueError, match="coherent"):
        N.NTupleLearner(_Env(), shape=BUDGET, coherent=True)
    with pytest.raises(ValueError, match="stage_map"):
        N.NTupleLearner(_Env(), shape=BUDGET, stage_map=N.ntuple_stage_map(10, 40))
    # bound=True is the budget table's alone, and the message names the form to use
    named = re.escape('"feat+spare"')
    for shape in ("2x4", "3x3", "2x4+3x3", FEAT, "3x3+feat"):
        table = N.ntuple_table("cpu", shape)
        with pytest.raises(ValueError, match=named):
            N.NTuplePolicy(_Env(), table, bound=True)
        with pytest.raises(ValueError, match=named):
            N.NTupleBeamPolicy(_Env(), table, 3, 8, bound=True)
        with pytest.raises(ValueError, match=named):
            N.NTupleLearner(_Env(), shape=shape, bound=True)
        assert N.NTuplePolicy(_Env(), table).bound is False and N.NTupleBeamPolicy(_Env(), table, 3, 8).bound is False
    with pytest.raises(ValueError, match=named):
        N.NTuplePolicy(_Env(), N.ntuple_table("cpu", "2x4", staged=True), bound=True)
    budget = N.ntuple_table("cpu", BUDGET)
    assert N.NTuplePolicy(_Env(), budget, bound=True).bound is True and N.NTupleBeamPolicy(_Env(), budget, 3, 8, bound=True).bound is True
    assert N.NTuplePolicy(_Env(), budget).bound is False and N.NTuplePolicy(_Env(), budget, depth=2, bound=True).shape == BUDGET
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="bound"):
            N.NTuplePolicy(_Env(), budget, bound=bad)
        with pytest.raises(ValueError, match="bound"):
            N.NTupleBeamPolicy(_Env(), budget, 3, 8, bound=bad)
    for shape in ("spare+feat", "feat+spare ", "FEAT+SPARE", "spare"):
        with pytest.raises(ValueError, match="shape"):
            N.ntuple_table("cpu", shape=shape)
        with pytest.raises(ValueError, match="shape"):
            _m().ntuple_indices(np.zeros(20, np.uint16), 0, 5, 8, 0, 0, shape=shape)
    planes = (torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32))
    for bad in (torch.zeros(EB + 16, dtype=torch.int32), torch.zeros(EB, dtype=torch.int64), torch.zeros(2 * EB, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="table"):
            N.ntuple_value(planes, bad, 5, 8)
        with pytest.raises(ValueError, match="table"):
            N.ntuple_is_symmetric(bad)
    with pytest.raises(ValueError, match="table"):
        N.ntuple_shape(torch.zeros((EB, 2), dtype=torch.int64))                 # no coherence buffer has the budget table's count
    with pytest.raises(ValueError, match="source"):
        N.ntuple_budget_bins((torch.zeros((2, 4), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64)), 5, 8)
    with pytest.raises(ValueError, match="L and M"):
        N.ntuple_budget_bins(planes)


# ------------------------------------------------------------------------------------------------ 5. the library
def test_every_declared_symbol_is_exported_and_no_budget_kernel_uses_scratch():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and set(ENTRIES) <= declared
    lib = ctypes.CDLL(_m().build_library())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    names = lambda entry: [a.split()[-1].lstrip("*") for a in re.search(rf"int {entry}\((.*?)\);", text, flags=re.S).group(1).split(",")]
    assert names("tpl_ntuple_value_budget") == [a for a in names("tpl_ntuple_value_feature") if a != "form"]
    for entry in ("act", "search", "beam"):                    # the twin's arguments, `prune` where it has `form`
        assert names(f"tpl_ntuple_{entry}_budget") == ["prune" if a == "form" else a for a in names(f"tpl_ntuple_{entry}_feature")], entry
    assert names("tpl_ntuple_update_trace_budget") == names("tpl_ntuple_update_trace_feature")
    assert names("tpl_ntuple_budget_bins") == ["plane_a", "plane_b", "n", "L", "M", "bins", "stream"]
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _m().build_library()], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    field = lambda r, name: int(r[r.index(name) - 1])
    mine = [r for r in rows if "ntuple_budget" in r[-1]]
    for r in mine:
        print(" ".join(r))
    kernels = ("ntuple_budget_value_kernel", "ntuple_budget_act_kernel", "ntuple_budget_search_kernel", "ntuple_budget_beam_kernel",
               "ntuple_budget_bins_kernel", "ntuple_budget_trace_kernelILb0", "ntuple_budget_trace_kernelILb1")
    for kernel in kernels:
        assert sum(kernel in r[-1] for r in mine) == 1, kernel
    assert len(mine) == len(kernels) and all(field(r, "scratch") == 0 for r in mine)
    trace = [r for r in mine if "trace" in r[-1]]
    assert all(field(r, "lds") == 4 * EB for r in trace)       # the whole table's image: 86,016 bytes, one block a CU
    assert all(field(r, "vgpr") <= 128 for r in mine)
    assert all(field(r, "scratch") == 0 for r in rows if "ntuple" in r[-1])
