"""CPU-side checks of the n-tuple learner's temporal-coherence step sizes (include/tpl_learn.h's rule for tpl_ntuple_update_coherent,
the numpy mirror in _learn_lib, ntuple.py):

  * the mirror of the update against a second statement written here from rows, cells and plain Python integers -- the indices from
    the cells, the images through sigma's formula, the conversions by integer rounding, every float32 product as an exact double
    product rounded once; zero coherence gives ntuple_update_trace's table bytes; E takes d and A takes |d| at exactly the entries
    the table changed at (the counter once, 2 x at a self-image entry, nothing for a finished state or behind a cut); alpha is read
    before the call; a symmetric call keeps a symmetric pair symmetric;
  * ntuple_step_sizes over pairs chosen by class (COHERENCE_CLASSES), against exact rationals;
  * the toy case of 64 copies of one board at g = 3: the plain update diverges, the coherent one peaks at about four times its
    start and settles;
  * the header declares the entry, the library exports it, both new kernels are built in both forms without scratch;
  * every refusal of the entry comes back as a status with its name in the message, without a GPU, and NTupleLearner refuses a bad
    `coherent`.
"""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, load_golden

import tetris_piclim as T
from test_heuristic_cpu import _Env

ENTRIES = 8 * 153 * 256 + 1024
COUNTER_BASE = 8 * 153 * 256
PI = (0, 2, 1, 3, 5, 4, 6, 7)
L, M = 10, 40
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ the second statement
def _f32_of_int(n: int) -> int:
    """A non-negative integer rounded to the nearest float32, ties to even, as an integer (exact for n < 2^128)."""
    if n < (1 << 24):
        return n
    shift = n.bit_length() - 24
    q, r = divmod(n, 1 << shift)
    half = 1 << (shift - 1)
    if r > half or (r == half and q & 1):
        q += 1
    return q << shift


def _alpha(E: int, A: int) -> np.float32:
    """alpha of the pair (E, A) in plain integers.  The quotient of two float32 values taken in float64 and rounded to float32 is
    the float32 quotient rounded once (53 >= 2 * 24 + 2)."""
    if A <= 0:
        return np.float32(1.0)
    return min(np.float32(float(_f32_of_int(abs(E))) / float(_f32_of_int(A))), np.float32(1.0))


def _mul(a, b) -> np.float32:
    """A float32 product rounded once: the double product of two float32 values is exact."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.float64(np.float32(a)) * np.float64(np.float32(b)))


def _step(r, e) -> int:
    x = _mul(r, e)
    if np.isnan(x):
        return 0
    return int(np.rint(min(max(float(x), -float(1 << 24)), float(1 << 24))))


def _wrap(v: int, bits: int) -> int:
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _entries(rows, piece, lines, moves, symmetric):
    """The entries of one running state, in plain integers from the cells: the counter once, every tuple with a non-zero pattern and,
    with `symmetric`, its image through sigma's formula -- a list with repeats where the rule adds twice."""
    cell = lambda r, c: (int(rows[r]) >> c) & 1
    out = [COUNTER_BASE + 64 * min(max(L - int(lines), 0), 15) + min(max(M - int(moves), 0), 63)]
    for x in range(9):
        for y in range(17):
            q = sum((cell(y + j, x) << j) | (cell(y + j, x + 1) << (4 + j)) for j in range(4))
            if q:
                out.append((int(piece) * 153 + 17 * x + y) * 256 + q)
                if symmetric:
                    out.append((PI[int(piece)] * 153 + 17 * (8 - x) + y) * 256 + ((q >> 4) | ((q & 15) << 4)))
    return out


def _reference(table, coherence, ages, error, rate, decay, symmetric):
    """The rule of include/tpl_learn.h, board by board and entry by entry: (table, coherence) as new arrays."""
    tab = {}
    coh = {}
    k = len(error)
    for i in range(k):
        w = np.float32(1.0)
        for age, (rows, piece, lines, moves, state) in enumerate(ages):
            if age:
                w = _mul(w, decay)
            if int(state[i]) != 0:
                break
            r = _mul(rate, w)
            d = _step(r, error[i])
            if d == 0:
                continue
            for j in _entries(rows[i], piece[i], lines[i], moves[i], symmetric):
                alpha = _alpha(int(coherence[j, 0]), int(coherence[j, 1]))         # the buffer as it stood before the call
                tab[j] = tab.get(j, 0) + _step(_mul(r, alpha), error[i])
                dE, dA = coh.get(j, (0, 0))
                coh[j] = (dE + d, dA + abs(d))
    table, coherence = table.copy(), coherence.copy()
    for j, s in tab.items():
        table[j] = _wrap(int(table[j]) + s, 32)
    for j, (dE, dA) in coh.items():
        coherence[j] = (_wrap(int(coherence[j, 0]) + dE, 64), _wrap(int(coherence[j, 1]) + dA, 64))
    return table, coherence, set(coh)


# ------------------------------------------------------------------------------------------------ the classes of a pair
# (name, E, A) -- what ntuple_step_sizes and the kernel are tried on; coherence_by_class lays them over a buffer
COHERENCE_CLASSES = [
    ("A = 0", 5, 0), ("A = 0, E = 0", 0, 0), ("A < 0", 7, -3), ("A < 0, far", -9, I64_MIN),
    ("|E| > A", 10, 3), ("|E| > A, E < 0", -10, 3), ("E = A", 12345, 12345), ("E = -A", -12345, 12345),
    ("E = INT64_MIN", I64_MIN, 3 << 61), ("E = INT64_MIN, A at the top", I64_MIN, I64_MAX),
    ("above 2^24: a tie to even, down", (1 << 24) + 1, (1 << 25) + 2), ("above 2^24: a tie to even, up", (1 << 24) + 3, (1 << 26) + 12),
    ("above 2^24: E < 0", -((1 << 30) + 33), (1 << 31) + 65),
    ("above 2^53: a double would round twice", (1 << 53) + 1, (1 << 60) + (1 << 36) + 1),
    ("above 2^53: E < 0", -((1 << 57) + (1 << 33) + 1), (1 << 62) - 1),
    ("a small ratio: s rounds to 0", 1, 1 << 40), ("a small ratio, E < 0", -3, 1 << 50), ("E = 0", 0, 1000),
    ("half", 500, 1000), ("a third", -(1 << 20), 3 << 20), ("the next add wraps", I64_MAX - 5, I64_MAX - 5),
    ("the next add wraps, E < 0", I64_MIN + 5, I64_MAX - 3),
]


def coherence_by_class(seed):
    """A coherence buffer with the classes above laid over all its entries at random: (int64 [ENTRIES, 2], class index [ENTRIES])."""
    gen = np.random.default_rng(seed)
    which = gen.integers(0, len(COHERENCE_CLASSES), ENTRIES)
    pairs = np.array([(e, a) for _, e, a in COHERENCE_CLASSES], dtype=object)
    out = np.empty((ENTRIES, 2), np.int64)
    out[:, 0] = np.array([int(v) for v in pairs[:, 0]], np.int64)[which]
    out[:, 1] = np.array([int(v) for v in pairs[:, 1]], np.int64)[which]
    return out, which


def _states(gen, k, finished=0.2):
    """k random states as the mirror's fields (rows, piece, lines, moves, state)."""
    rows = np.where(gen.random((k, 20)) < 0.5, gen.integers(0, 1 << 10, (k, 20)), 0).astype(np.uint16)
    state = np.where(gen.random(k) < finished, gen.integers(1, 4, k), 0)
    return rows, gen.integers(0, 8, k), gen.integers(0, 12, k), gen.integers(0, 45, k), state


def _full_range_table(gen):
    start = gen.integers(-(1 << 31), 1 << 31, ENTRIES).astype(np.int32)
    start[::3] = np.int32((1 << 31) - 1)
    return start


# ------------------------------------------------------------------------------------------------ 1. the mirror of the update
@pytest.mark.parametrize("symmetric", [False, True])
def test_the_mirror_is_the_rule_written_from_cells_and_python_integers(symmetric):
    m = _m()
    gen = np.random.default_rng(11 + symmetric)
    k, horizon = 24, 3
    ages = [_states(gen, k) for _ in range(horizon)]
    ages[0][4][:20] = 0                                        # most boards run at age 0
    rate, decay = 3000.0, 0.9
    error = gen.normal(size=k).astype(np.float32)
    error[:6] = (np.nan, 1e9, -1e9, 0.52 / rate, -0.52 / rate, np.inf)
    table, (coherence, which) = _full_range_table(gen), coherence_by_class(5)
    want_t, want_c, touched = _reference(table, coherence, ages, error, rate, decay, symmetric)
    got_t, got_c = m.ntuple_update_coherent(table.copy(), coherence.copy(), ages, L, M, error, rate, decay, symmetric)
    assert got_t.dtype == np.int32 and got_c.dtype == np.int64
    assert np.array_equal(got_t, want_t) and np.array_equal(got_c, want_c)
    assert set(np.flatnonzero((got_c != coherence).any(axis=1)).tolist()) == touched and len(touched) > 1000
    assert set(which[sorted(touched)].tolist()) == set(range(len(COHERENCE_CLASSES)))             # every class was met
    assert set(np.flatnonzero(got_t != table).tolist()) <= touched
    assert (got_c[sorted(touched), 1] < coherence[sorted(touched), 1]).any()                      # an add wrapped in 64 bits
    # |s| <= |d|: a table entry one board alone touched moved by no more than its E did
    alone = [j for j in touched if abs(int(got_c[j, 1]) - int(coherence[j, 1])) < (1 << 24) and j < COUNTER_BASE]
    moved = np.abs(((got_t[alone].astype(np.int64) - table[alone]) + (1 << 31)) % (1 << 32) - (1 << 31))
    assert (moved <= np.abs(got_c[alone, 1] - coherence[alone, 1])).all() and len(alone) > 100


def test_zero_coherence_gives_the_table_bytes_of_ntuple_update_trace():
    m = _m()
    gen = np.random.default_rng(2)
    k, horizon = 120, 4
    ages = [_states(gen, k) for _ in range(horizon)]
    error = gen.normal(size=k).astype(np.float32)
    error[:5] = (np.nan, 1e9, -1e9, np.inf, -np.inf)
    start = _full_range_table(gen)
    for symmetric in (False, True):
        want = m.ntuple_update_trace(start.copy(), ages, L, M, error, 3000.0, 0.8, symmetric)
        got, coherence = m.ntuple_update_coherent(start.copy(), np.zeros((ENTRIES, 2), np.int64), ages, L, M, error, 3000.0, 0.8, symmetric)
        assert np.array_equal(got, want) and (got != start).sum() > 1000
        # the zero table, where nothing wraps: A is there exactly where the table could have changed
        flat = m.ntuple_update_trace(np.zeros(ENTRIES, np.int32), ages, L, M, np.abs(error), 3000.0, 0.8, symmetric)
        assert np.array_equal(coherence[:, 1] != 0, flat != 0)
        assert (np.abs(coherence[:, 0]) <= coherence[:, 1]).all()
    # a second call from that coherence is NOT the plain update: some entries have slowed down
    again, _ = m.ntuple_update_coherent(got.copy(), coherence.copy(), ages, L, M, -error, 3000.0, 0.8, True)
    assert not np.array_equal(again, m.ntuple_update_trace(got.copy(), ages, L, M, -error, 3000.0, 0.8, True))


def test_E_takes_d_and_A_takes_its_magnitude_at_exactly_the_entries_of_the_table():
    m = _m()
    rows = np.zeros(20, np.uint16)
    rows[16:] = (0b0000110000, 0b0001111000, 0b1100110011, 0b1111111111)         # its own reflection
    other = np.zeros(20, np.uint16)
    other[18:] = (0b0000000111, 0b1110001111)
    zero_t, zero_c = np.zeros(ENTRIES, np.int32), np.zeros((ENTRIES, 2), np.int64)
    sigma = m.ntuple_mirror_permutation()
    # one board under O (6), symmetric, error -1 at rate 7: d = -7
    t, c = m.ntuple_update_coherent(zero_t.copy(), zero_c.copy(), [(rows[None], [6], [0], [0], [0])], L, M, np.array([-1.0], np.float32),
                                    7.0, 0.5, True)
    index, used = m.ntuple_indices(rows, 6, L, M, 0, 0)
    own, counter = index[0][used[0]][:-1], index[0][-1]
    assert set(sigma[own].tolist()) == set(own.tolist())       # the board is its own reflection, and O its own image
    assert (t[own] == -14).all() and (c[own, 0] == -14).all() and (c[own, 1] == 14).all()          # 2 s, 2 d, 2 |d|
    middle = own[sigma[own] == own]
    assert middle.size >= 4
    assert t[counter] == -7 and tuple(c[counter]) == (-7, 7)                                       # the counter once
    assert np.count_nonzero(t) == own.size + 1 and np.count_nonzero(c[:, 1]) == own.size + 1
    # not symmetric: d once everywhere
    t, c = m.ntuple_update_coherent(zero_t.copy(), zero_c.copy(), [(rows[None], [6], [0], [0], [0])], L, M, np.array([-1.0], np.float32),
                                    7.0, 0.5, False)
    assert (t[own] == -7).all() and (c[own, 0] == -7).all() and (c[own, 1] == 7).all() and tuple(c[counter]) == (-7, 7)
    # two ages: a finished state at age 0 leaves everything alone, one at age 1 cuts the trace behind age 0; a NaN adds nothing
    for state, error, expect in (([1, 0], 1.0, 0), ([0, 2], 1.0, 1), ([0, 0], 1.0, 2), ([0, 0], np.nan, 0)):
        ages = [(rows[None], [6], [0], [0], state[:1]), (other[None], [1], [1], [3], state[1:])]
        t, c = m.ntuple_update_coherent(zero_t.copy(), zero_c.copy(), ages, L, M, np.array([error], np.float32), 8.0, 0.5, False)
        index1, used1 = m.ntuple_indices(other, 1, L, M, 1, 3)
        older = index1[0][used1[0]]
        assert np.count_nonzero(c[:, 1]) == (0, own.size + 1, own.size + 1 + older.size)[expect]
        assert np.array_equal(c[:, 0], t) and np.array_equal(c[:, 1], np.abs(t))                   # alpha 1, positive errors
        if expect == 2:
            assert (t[older] == 4).all() and (t[own] == 8).all()                                   # d_1 = rint(8 * 0.5 * 1)


def test_alpha_is_read_before_the_call_so_boards_that_share_an_entry_use_the_old_one():
    m = _m()
    rows = np.zeros(20, np.uint16)
    rows[18:] = (0b0000000111, 0b1110001111)
    index, used = m.ntuple_indices(rows, 2, L, M, 0, 0)
    own = index[0][used[0]]
    coherence = np.zeros((ENTRIES, 2), np.int64)
    coherence[own] = (500, 1000)                                                 # alpha = 0.5
    two = (np.stack([rows, rows]), [2, 2], [0, 0], [0, 0], [0, 0])
    error = np.array([1.0, -1.0], np.float32)                                    # d = +100 and -100: E stays, A grows by 200
    t, c = m.ntuple_update_coherent(np.zeros(ENTRIES, np.int32), coherence.copy(), [two], L, M, error, 100.0, 0.0, False)
    assert (t[own] == 0).all() and (c[own, 0] == 500).all() and (c[own, 1] == 1200).all()          # +50 and -50
    error = np.array([1.0, 1.0], np.float32)
    t, c = m.ntuple_update_coherent(np.zeros(ENTRIES, np.int32), coherence.copy(), [two], L, M, error, 100.0, 0.0, False)
    assert (t[own] == 100).all()                                                 # 50 + 50: the second board did not see 600 / 1100
    assert (c[own, 0] == 700).all() and (c[own, 1] == 1200).all()
    # board by board the second one would have used the new alpha, 600 / 1100
    one = (rows[None], [2], [0], [0], [0])
    t1, c1 = m.ntuple_update_coherent(np.zeros(ENTRIES, np.int32), coherence.copy(), [one], L, M, error[:1], 100.0, 0.0, False)
    t2, c2 = m.ntuple_update_coherent(t1, c1, [one], L, M, error[:1], 100.0, 0.0, False)
    assert (t2[own] == 50 + 55).all() and np.array_equal(c2, c)
    # the same board at two ages of one call: both ages read the old alpha as well
    t, c = m.ntuple_update_coherent(np.zeros(ENTRIES, np.int32), coherence.copy(), [one, one], L, M, error[:1], 100.0, 1.0, False)
    assert (t[own] == 100).all() and (c[own, 1] == 1200).all()


def test_a_symmetric_call_keeps_a_symmetric_pair_symmetric():
    m = _m()
    sigma = m.ntuple_mirror_permutation()
    gen = np.random.default_rng(5)
    k, horizon = 150, 3
    ages = [_states(gen, k) for _ in range(horizon)]
    error = gen.normal(size=k).astype(np.float32)
    lower = sigma < np.arange(ENTRIES)
    table = gen.integers(-(1 << 31), 1 << 31, ENTRIES).astype(np.int32)
    table = np.where(lower, table[sigma], table)
    coherence, _ = coherence_by_class(9)
    coherence = np.where(lower[:, None], coherence[sigma], coherence)
    assert np.array_equal(table[sigma], table) and np.array_equal(coherence[sigma], coherence)
    t, c = table.copy(), coherence.copy()
    for call in range(3):
        m.ntuple_update_coherent(t, c, ages, L, M, error * (1 - call), 2000.0, 0.9, True)
        assert np.array_equal(t[sigma], t) and np.array_equal(c[sigma], c), call
    assert (t != table).sum() > 1000 and (c != coherence).any(axis=1).sum() > 1000
    t, c = m.ntuple_update_coherent(table.copy(), coherence.copy(), ages, L, M, error, 2000.0, 0.9, False)
    assert not np.array_equal(t[sigma], t) and not np.array_equal(c[sigma], c)


# ------------------------------------------------------------------------------------------------ 2. the step sizes
def test_step_sizes_by_class_against_exact_rationals():
    m = _m()
    coherence = np.zeros((ENTRIES, 2), np.int64)
    for j, (_, e, a) in enumerate(COHERENCE_CLASSES):
        coherence[j] = (e, a)
    got = m.ntuple_step_sizes(coherence)
    assert got.dtype == np.float32 and got.shape == (ENTRIES,) and (got[len(COHERENCE_CLASSES):] == 1.0).all()
    for j, (name, e, a) in enumerate(COHERENCE_CLASSES):
        assert got[j].view(np.uint32) == np.float32(_alpha(e, a)).view(np.uint32), name
        assert 0.0 <= got[j] <= 1.0, name
    alpha = dict((name, float(got[j])) for j, (name, _, _) in enumerate(COHERENCE_CLASSES))
    for name in ("A = 0", "A = 0, E = 0", "A < 0", "A < 0, far", "|E| > A", "|E| > A, E < 0", "E = A", "E = -A",
                 "E = INT64_MIN", "E = INT64_MIN, A at the top", "the next add wraps"):
        assert alpha[name] == 1.0, name
    assert alpha["E = 0"] == 0.0 and alpha["half"] == 0.5 and alpha["a third"] == float(np.float32(1.0) / np.float32(3.0))
    # (E = INT64_MIN: the magnitude 2^63 is above every A, so alpha is 1 -- and negative where the magnitude was taken signed)
    # the conversions round to even: 2^24 + 1 -> 2^24 and 2^25 + 2 -> 2^25; 2^24 + 3 -> 2^24 + 4 and 2^26 + 12 -> 2^26 + 16
    assert alpha["above 2^24: a tie to even, down"] == 0.5
    assert _f32_of_int((1 << 24) + 3) == (1 << 24) + 4 and _f32_of_int((1 << 26) + 12) == (1 << 26) + 16
    assert Fraction(alpha["above 2^24: a tie to even, up"]) == Fraction(float(np.float32(((1 << 24) + 4) / ((1 << 26) + 16))))
    # 2^60 + 2^36 + 1 lies above the middle of two float32 values and rounds UP; through a double it would be a tie and round down
    assert _f32_of_int((1 << 60) + (1 << 36) + 1) == (1 << 60) + (1 << 37)
    assert got[13].view(np.uint32) == np.float32(np.float64(1 << 53) / np.float64((1 << 60) + (1 << 37))).view(np.uint32)
    # ratios so small that the step rounds to 0 where d does not
    for name in ("a small ratio: s rounds to 0", "a small ratio, E < 0"):
        j = [c[0] for c in COHERENCE_CLASSES].index(name)
        assert 0.0 < got[j] < 1e-11
        assert m.ntuple_steps(np.array([1.0], np.float32), 3000.0)[0] == 3000
        assert m.ntuple_coherent_steps(np.array([1.0], np.float32), 3000.0, got[j:j + 1])[0] == 0
    for bad in (coherence[:-1], coherence.astype(np.int32), coherence.reshape(-1), None):
        with pytest.raises(ValueError, match="coherence"):
            m.ntuple_step_sizes(bad)
    # the torch form, on the host: the same bits
    import torch
    assert T.ntuple_step_sizes is T.ntuple.ntuple_step_sizes and T.ntuple_coherence is T.ntuple.ntuple_coherence
    both, _ = coherence_by_class(3)
    for c in (coherence, both):
        mine = T.ntuple_step_sizes(torch.from_numpy(c))
        assert mine.dtype == torch.float32 and np.array_equal(mine.numpy().view(np.uint32), m.ntuple_step_sizes(c).view(np.uint32))
    fresh = T.ntuple_coherence("cpu")
    assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (ENTRIES, 2) and not fresh.any()
    for bad in (fresh[:-1], fresh.to(torch.int32), fresh.numpy(), None):
        with pytest.raises(ValueError, match="coherence"):
            T.ntuple_step_sizes(bad)


# ------------------------------------------------------------------------------------------------ 3. the toy case
def toy_board():
    """One carved start position from tests/golden/ as the mirror's fields for 64 copies, its entries in use and the rate at which
    g = n * m * rate * 2^-16 is 3."""
    rows = load_golden("carved_L10_M40.npz")["rows"].astype(np.uint16)
    rows = rows[(rows != 0).sum(axis=1) >= 4][0]
    n = 64
    _, used = _m().ntuple_indices(rows, 0, L, M, 0, 0)
    entries = int(used.sum())                                  # the tuples in use and the counter
    assert entries > 10
    state = (np.broadcast_to(rows, (n, 20)).copy(), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64),
             np.zeros(n, np.int64))
    return state, entries, 3.0 * 65536.0 / (n * entries)


def toy_assertions(plain, coherent, rate):
    """|e| of the two runs, step by step from the start (index 0) on; at least 60 steps each."""
    start = plain[0]
    assert coherent[0] == start and start > 0
    assert plain[40] > 1000.0 * start                          # g = 3: the error doubles every step until the clamp holds it
    assert rate * max(plain[:41]) >= float(1 << 24)            # ... which it reached
    peak = max(coherent)
    assert 2.0 * start < peak < 8.0 * start                    # the float simulation: 4 x the start, at the second step
    assert int(np.argmax(coherent)) <= 3
    assert all(e < start for e in coherent[40:]) and len(coherent) >= 60
    assert max(coherent[40:]) < 0.05 * start                   # ... and it settles near the rounding floor, far below the start


def test_the_toy_case_through_the_mirror_diverges_plain_and_settles_coherent():
    m = _m()
    state, entries, rate = toy_board()
    target = np.float32(10.0)
    runs = []
    for coherent in (False, True):
        table, coherence = np.zeros(ENTRIES, np.int32), np.zeros((ENTRIES, 2), np.int64)
        errors = []
        for step in range(61):
            error = (target - m.ntuple_value(table, state[0], state[1], L, M, state[2], state[3], state[4])).astype(np.float32)
            assert (error == error[0]).all()
            errors.append(abs(float(error[0])))
            if coherent:
                m.ntuple_update_coherent(table, coherence, [state], L, M, error, rate, 0.0, False)
            else:
                m.ntuple_update_trace(table, [state], L, M, error, rate, 0.0, False)
        runs.append(errors)
    print("plain", [f"{e:.3g}" for e in runs[0][:45]], "coherent", [f"{e:.3g}" for e in runs[1]])
    toy_assertions(*runs, rate)


# ------------------------------------------------------------------------------------------------ 4. header and build
def test_the_header_declares_the_entry_and_both_kernels_are_built_without_scratch():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    args = re.search(r"int tpl_ntuple_update_coherent\((.*?)\);", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ["ring_a", "ring_b", "n", "slots", "head", "horizon", "L", "M", "table",
                                                         "coherence", "error", "rate", "decay", "symmetric", "stream"]
    assert "tpl_ntuple_update_coherent" in _m().LEARN_SYMBOLS and "read before add" in raw.lower()
    path = _m().build_library()
    assert hasattr(ctypes.CDLL(path), "tpl_ntuple_update_coherent")
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    for kernel, lds in (("ntuple_coherent_step_kernel", "4096"), ("ntuple_coherent_accumulate_kernel", "16384")):
        mine = [r for r in rows if kernel in r[-1]]
        assert len(mine) == 2, (kernel, [r[-1] for r in rows])                  # symmetric and not
        for r in mine:
            assert r[r.index("scratch") - 1] == "0" and int(r[r.index("vgpr") - 1]) <= 128 and r[r.index("lds") - 1] == lds, r
            for taken in ("ntuple_trace_kernel", "ntuple_value_kernel", "ntuple_act_kernel"):
                assert taken not in r[-1]


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_every_refusal_of_the_entry_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")
    name = b"tpl_ntuple_update_coherent"

    def call(a=fake, b=fake, n=4, slots=3, head=1, horizon=2, L=2, M=2, table=fake, coherence=fake, error=fake, rate=1.0, decay=0.5,
             symmetric=0):
        return lib.tpl_ntuple_update_coherent(a, b, n, slots, head, horizon, L, M, table, coherence, error, rate, decay, symmetric, None)

    # tpl_ntuple_update_trace's list
    assert call(a=None) < 0 and b"null" in err() and name in err()
    assert call(b=None) < 0 and b"null" in err() and name in err()
    for n in (0, -1):
        assert call(n=n) < 0 and b"positive" in err() and name in err(), n
    limit = -(-(1 << 31) // 40)
    for n in (limit, 1 << 40):
        assert call(n=n, slots=1, head=0, horizon=1) < 0 and b"2^31" in err() and name in err(), n
    for plane in ("a", "b"):
        assert call(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err(), plane
    for L_, M_ in ((0, 2), (2, 256), (251, 2), (255, 2), (2, 255), (2, 0)):
        assert call(L=L_, M=M_) < 0 and b"L and M" in err() and name in err(), (L_, M_)
    assert call(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
    for off in (4, 8, 12):
        assert call(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
    # its own: the coherence buffer, after the table
    assert call(coherence=None) < 0 and b"null" in err() and b"coherence" in err() and name in err()
    for off in (1, 4, 8, 12):
        assert call(coherence=fake + off) < 0 and b"coherence must be 16-byte aligned" in err() and name in err(), off
    assert call(error=None) < 0 and b"null" in err() and b"error" in err() and name in err()
    assert call(error=fake + 2) < 0 and b"error must be 4-byte aligned" in err() and name in err()
    for rate in (nan, inf, -inf):
        assert call(rate=rate) < 0 and b"rate must be finite" in err() and name in err(), rate
    for slots in (0, -1, 18, 1 << 20):
        assert call(slots=slots, head=0, horizon=1) < 0 and b"slots must be in [1, 17]" in err() and name in err(), slots
    for slots, head in ((3, -1), (3, 3), (3, 4), (1, 1), (17, 17)):
        assert call(slots=slots, head=head, horizon=1) < 0 and b"head must be in [0, slots)" in err() and name in err(), (slots, head)
    for slots, horizon in ((3, 0), (3, -1), (3, 4), (1, 2), (17, 17), (16, 17), (17, 1 << 20)):
        assert call(slots=slots, head=0, horizon=horizon) < 0 and b"horizon must be in [1, min(slots, 16)]" in err() and name in err()
    for slots in (2, 17):
        n = -(-limit // slots)
        assert n < limit and call(n=n, slots=slots, head=0, horizon=1) < 0 and b"2^31" in err() and b"slots" in err() and name in err()
    for decay in (-0.001, 1.001, -1.0, 2.0, nan, inf, -inf):
        for symmetric in (0, 1):
            assert call(decay=decay, symmetric=symmetric) < 0 and b"decay must be in [0, 1]" in err() and name in err(), decay
    # the first thing wrong is the one reported, in tpl_ntuple_update_trace's order with the coherence buffer behind the table
    assert call(a=fake + 8, slots=99) < 0 and b"aligned" in err() and b"slots" not in err()
    assert call(slots=99, decay=2.0) < 0 and b"slots" in err() and b"decay" not in err()
    assert call(L=0, table=None) < 0 and b"L and M" in err()
    assert call(table=fake + 4, coherence=None) < 0 and b"table" in err() and b"coherence" not in err()
    assert call(coherence=fake + 8, error=None) < 0 and b"coherence" in err() and b"error" not in err()
    assert call(coherence=None, rate=nan) < 0 and b"coherence" in err() and b"rate" not in err()
    assert call(error=None, slots=0) < 0 and b"error" in err() and b"slots" not in err()
    assert call(rate=nan, head=9) < 0 and b"rate" in err() and b"head" not in err()
    assert call(head=9, horizon=0) < 0 and b"head" in err() and b"horizon" not in err()
    assert call(horizon=0, decay=nan) < 0 and b"horizon" in err() and b"decay" not in err()
    # and the two entries refuse alike, message for message, up to the name
    trace = lambda **kw: lib.tpl_ntuple_update_trace(*[kw.get(k, v) for k, v in (("a", fake), ("b", fake), ("n", 4), ("slots", 3), ("head", 1),
                                                     ("horizon", 2), ("L", 2), ("M", 2), ("table", fake), ("error", fake), ("rate", 1.0),
                                                     ("decay", 0.5), ("symmetric", 0))], None)
    for kw in (dict(a=None), dict(n=0), dict(L=0), dict(table=fake + 4), dict(error=None), dict(rate=inf), dict(slots=0), dict(head=5),
               dict(horizon=3, slots=2), dict(decay=nan), dict(a=fake + 8, table=None, decay=7.0)):
        assert trace(**kw) < 0
        theirs = err().replace(b"tpl_ntuple_update_trace", b"")
        assert call(**kw) < 0 and err().replace(name, b"") == theirs, kw


def test_the_learner_refuses_a_bad_coherent_and_owns_its_buffer():
    import torch
    nt = T.ntuple
    env = _Env(8)
    learner = nt.NTupleLearner(env)
    assert learner.coherent is False and learner.coherence is None
    learner = nt.NTupleLearner(env, gamma=0.5, rate=4, epsilon=0.25, seed=3, lam=0.8, horizon=4, symmetric=True, coherent=True)
    assert learner.coherent is True and learner.symmetric is True
    assert learner.coherence.dtype == torch.int64 and tuple(learner.coherence.shape) == (ENTRIES, 2) and not learner.coherence.any()
    learner.coherence[5] = torch.tensor([3, 4])
    learner.forget()                                           # the ring is cut; the coherence buffer is left alone
    assert learner.coherence[5].tolist() == [3, 4] and int(learner.coherence.abs().sum()) == 7
    assert float(T.ntuple_step_sizes(learner.coherence)[5]) == 0.75
    for coherent in (0, 1, None, "yes", 1.0):
        with pytest.raises(ValueError, match="coherent"):
            nt.NTupleLearner(env, coherent=coherent)
