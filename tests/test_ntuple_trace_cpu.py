"""CPU-side checks of the n-tuple learner's traces and mirror symmetry (include/tpl_learn.h's rule for tpl_ntuple_update_trace, the
numpy mirror in _learn_lib, ntuple.py):

  * sigma, the mirror permutation of the table's entries, is an involution that fixes the counters, keeps the empty pattern empty
    and is not the identity; on boards from tests/golden/ the entries of the reflected rows under pi(piece) are sigma of the
    board's own -- three statements of the reflection (sigma, the reflected rows, lib.mirror_states) that share nothing;
  * the mirror of the update with one age and symmetric=False is ntuple_update byte for byte, whatever the decay; a finished state
    at age j leaves the ages >= j out; a NaN adds nothing; decay 1 gives every running age the same step, decay 0 only age 0;
    the symmetric form keeps a symmetric table symmetric, adds the counter once and 2 d where an entry is its own image;
  * the header declares the entry, the library exports it, both forms of the kernel are built without scratch;
  * every refusal of the entry comes back as a status with its name in the message, without a GPU, and NTupleLearner refuses a bad
    lam, horizon and symmetric.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

import tetris_piclim as T
from test_heuristic_cpu import _Env

ENTRIES = 8 * 153 * 256 + 1024
COUNTER_BASE = 8 * 153 * 256
PI = (0, 2, 1, 3, 5, 4, 6, 7)
L, M = 10, 40


def _m():
    return T._learn_lib


def _swap(q):
    return (q >> 4) | ((q & 15) << 4)


def _golden_rows():
    """Boards that random moves left (random_moves.npz) and the carved start positions (carved_L10_M40.npz): uint16 [K, 20], each
    with cells on it."""
    rows = np.concatenate([load_golden("random_moves.npz")["o_rows"][::16], load_golden("carved_L10_M40.npz")["rows"][::4]])
    rows = np.unique(rows[(rows != 0).any(axis=1)].astype(np.uint16), axis=0)
    assert rows.shape[0] > 250
    return rows


def _states(gen, k, finished=0.2):
    """k random states as the mirror's fields (rows, piece, lines, moves, state)."""
    rows = np.where(gen.random((k, 20)) < 0.5, gen.integers(0, 1 << 10, (k, 20)), 0).astype(np.uint16)
    state = np.where(gen.random(k) < finished, gen.integers(1, 4, k), 0)
    return rows, gen.integers(0, 8, k), gen.integers(0, 12, k), gen.integers(0, 45, k), state


def _full_range_table(gen):
    start = gen.integers(-(1 << 31), 1 << 31, ENTRIES).astype(np.int32)
    start[::3] = np.int32((1 << 31) - 1)                       # entries at the top of the range: their adds wrap
    return start


# ------------------------------------------------------------------------------------------------ 1. sigma
def test_sigma_is_an_involution_that_fixes_the_counters_and_keeps_the_empty_pattern():
    sigma = _m().ntuple_mirror_permutation()
    assert sigma.dtype == np.int64 and sigma.shape == (ENTRIES,)
    assert np.array_equal(sigma[sigma], np.arange(ENTRIES))                                 # an involution, so a permutation
    assert np.array_equal(sigma[COUNTER_BASE:], np.arange(COUNTER_BASE, ENTRIES))           # fixes indices >= 313,344
    assert (sigma[:COUNTER_BASE] < COUNTER_BASE).all()
    empty = np.arange(COUNTER_BASE) % 256 == 0
    assert (sigma[:COUNTER_BASE][empty] % 256 == 0).all() and (sigma[:COUNTER_BASE][~empty] % 256 != 0).all()   # q = 0 <-> q = 0
    assert (sigma != np.arange(ENTRIES)).sum() > 300000                                      # far from the identity
    # by its definition, entry by entry, on a sample and on the corners
    gen = np.random.default_rng(0)
    cases = [(0, 0, 0, 1), (7, 8, 16, 255), (1, 4, 3, 0x12), (3, 4, 5, 0x33)] + [
        tuple(int(v) for v in (gen.integers(0, 8), gen.integers(0, 9), gen.integers(0, 17), gen.integers(0, 256))) for _ in range(500)]
    for p, x, y, q in cases:
        j = (p * 153 + 17 * x + y) * 256 + q
        assert sigma[j] == (PI[p] * 153 + 17 * (8 - x) + y) * 256 + _swap(q), (p, x, y, q)
    # its fixed points among the tuples: a self-mirror piece, the middle column pair, a palindromic pattern
    fixed = np.flatnonzero(sigma[:COUNTER_BASE] == np.arange(COUNTER_BASE))
    p, t, q = fixed // (153 * 256), fixed // 256 % 153, fixed % 256
    assert set(p.tolist()) == {0, 3, 6, 7} and (t // 17 == 4).all() and (q == _swap(q)).all() and fixed.size == 4 * 17 * 16


def test_the_reflected_rows_of_golden_boards_index_sigma_of_the_boards_own_entries():
    m = _m()
    sigma = m.ntuple_mirror_permutation()
    rows = _golden_rows()
    k = rows.shape[0]
    gen = np.random.default_rng(1)
    piece, lines, moves = np.arange(k) % 8, gen.integers(0, 12, k), gen.integers(0, 45, k)
    index, used = m.ntuple_indices(rows, piece, L, M, lines, moves)
    # the reflection through the packed state and lib's own mirror of it: a third statement, on the column words
    import learn_ref as R
    window = piece.astype(np.uint64) | (gen.integers(0, 1 << 33, k).astype(np.uint64) << np.uint64(3))
    A, B = R.pack_state(rows, lines, moves, 0, 0, window)
    mirrored = R.decode_state(*m.mirror_states(A, B))
    assert np.array_equal(mirrored["cur"], np.array(PI)[piece]) and np.array_equal(mirrored["rows"], m._reflected_rows(rows))
    assert not np.array_equal(mirrored["rows"], rows)
    mindex, mused = m.ntuple_indices(mirrored["rows"], mirrored["cur"].astype(np.int64), L, M, lines, moves)
    for i in range(k):
        own, image = index[i][used[i]], mindex[i][mused[i]]
        assert set(image.tolist()) == set(sigma[own].tolist()), i
        assert image[-1] == own[-1] >= COUNTER_BASE                                        # the counter stays where it is
    assert used[:, :153].sum() > 20 * k
    # so a symmetric table values a board and its reflection alike, bit for bit, and an asymmetric one does not
    table = gen.integers(-(1 << 20), 1 << 20, ENTRIES).astype(np.int32)
    sym = np.minimum(table, table[sigma])
    assert np.array_equal(sym[sigma], sym) and not np.array_equal(table[sigma], table)
    v = m.ntuple_value(sym, rows, piece, L, M, lines, moves, 0)
    vm = m.ntuple_value(sym, mirrored["rows"], mirrored["cur"].astype(np.int64), L, M, lines, moves, 0)
    assert np.array_equal(v.view(np.uint32), vm.view(np.uint32)) and (v != 0).all()
    w = m.ntuple_value(table, rows, piece, L, M, lines, moves, 0)
    wm = m.ntuple_value(table, mirrored["rows"], mirrored["cur"].astype(np.int64), L, M, lines, moves, 0)
    assert (w != wm).mean() > 0.9


# ------------------------------------------------------------------------------------------------ 2. the mirror of the update
def test_one_age_without_symmetry_is_ntuple_update_for_any_decay():
    m = _m()
    gen = np.random.default_rng(2)
    k = 200
    s = _states(gen, k)
    error = gen.normal(size=k).astype(np.float32)
    error[gen.integers(0, k, 8)] = np.nan
    error[:4] = (1e9, -1e9, np.inf, -np.inf)
    start = _full_range_table(gen)
    want = m.ntuple_update(start.copy(), s[0], s[1], L, M, s[2], s[3], s[4], error, 3000.0)
    assert (want != start).sum() > 1000
    for decay in (0.0, 0.5, 0.9, 1.0):
        got = m.ntuple_update_trace(start.copy(), [s], L, M, error, 3000.0, decay, False)
        assert got.dtype == np.int32 and np.array_equal(got, want), decay


def test_a_finished_state_cuts_the_trace_and_a_nan_adds_nothing():
    m = _m()
    gen = np.random.default_rng(3)
    k, horizon = 120, 5
    ages = [_states(gen, k, finished=0.0) for _ in range(horizon)]
    cut = np.arange(k) % (horizon + 1)                         # board i stops exactly at age cut[i]; cut == horizon runs through
    for j in range(horizon):
        ages[j][4][cut == j] = 1 + j % 3
    error = (gen.normal(size=k) + 3.0).astype(np.float32)
    error[7::16] = np.nan
    rate, decay = 500.0, 0.8
    start = _full_range_table(gen)
    got = m.ntuple_update_trace(start.copy(), ages, L, M, error, rate, decay, False)
    # age by age through ntuple_update: the states at age j of the boards that still run, at the rate the rule gives that age
    want, w = start.copy(), np.float32(1.0)
    for j in range(horizon):
        alive = cut > j
        r, p, l, mv, st = (x[alive] for x in ages[j])
        assert (st == 0).all()
        m.ntuple_update(want, r, p, L, M, l, mv, st, error[alive], np.float32(rate) * w)
        w = np.float32(w * np.float32(decay))
    assert np.array_equal(got, want) and (got != start).sum() > 1000
    # the states behind a cut do not matter, whatever they are, and neither do the boards with a NaN
    other = [tuple(x.copy() for x in age) for age in ages]
    for j in range(1, horizon):
        behind = cut < j
        other[j][0][behind] = 0x3FF
        other[j][1][behind] = 7
        other[j][4][behind] = 0                                # running again behind the cut: still not reached
    assert np.array_equal(m.ntuple_update_trace(start.copy(), other, L, M, error, rate, decay, False), got)
    quiet = [tuple(x[7::16] for x in age) for age in ages]
    assert np.array_equal(m.ntuple_update_trace(start.copy(), quiet, L, M, error[7::16], rate, decay, True), start)


def test_decay_one_gives_every_running_age_the_same_step_and_decay_zero_only_age_zero():
    m = _m()
    gen = np.random.default_rng(4)
    k, horizon = 40, 4
    ages = [_states(gen, k, finished=0.0) for _ in range(horizon)]
    error = gen.normal(size=k).astype(np.float32)
    zero = np.zeros(ENTRIES, np.int32)
    d = m.ntuple_steps(error, 1000.0)
    assert (d != 0).all()
    for i in (0, 17):                                          # one board at a time: every entry it touches holds its d, summed
        one = [tuple(x[i:i + 1] for x in age) for age in ages]
        got = m.ntuple_update_trace(zero.copy(), one, L, M, error[i:i + 1], 1000.0, 1.0, False)
        count = np.zeros(ENTRIES, np.int64)
        for r, p, l, mv, _ in one:
            index, used = m.ntuple_indices(r, p, L, M, l, mv)
            np.add.at(count, index[used], 1)
        assert np.array_equal(got.astype(np.int64), count * d[i]) and count.max() >= 1 and count.sum() > 4 * 20
    all_ = m.ntuple_update_trace(zero.copy(), ages, L, M, error, 1000.0, 0.0, False)
    first = m.ntuple_update(zero.copy(), ages[0][0], ages[0][1], L, M, ages[0][2], ages[0][3], 0, error, 1000.0)
    assert np.array_equal(all_, first)                         # decay 0: w_1 = 0, d_1 = rint(0 * e) = 0
    # the weights are float32 products, each rounded once: 0.9f * 0.9f * 0.9f, not the float64 0.729
    w = np.float32(np.float32(np.float32(0.9) * np.float32(0.9)) * np.float32(0.9))
    one = [tuple(x[:1] for x in age) for age in ages]
    big = np.array([1.0], np.float32)
    got = m.ntuple_update_trace(zero.copy(), one, L, M, big, float(1 << 23), 0.9, False)
    index, used = m.ntuple_indices(*one[3][:2], L, M, *one[3][2:4])
    only_age_3 = [j for j in index[0][used[0]] if all(j not in m.ntuple_indices(*a[:2], L, M, *a[2:4])[0][0] for a in one[:3])]
    assert only_age_3 and all(got[j] == int(np.rint(np.float32(1 << 23) * w)) for j in only_age_3)


def test_the_symmetric_update_keeps_the_table_symmetric_and_doubles_a_self_mirror_entry():
    m = _m()
    sigma = m.ntuple_mirror_permutation()
    gen = np.random.default_rng(5)
    k, horizon = 150, 3
    ages = [_states(gen, k) for _ in range(horizon)]
    error = gen.normal(size=k).astype(np.float32)
    table = gen.integers(-(1 << 31), 1 << 31, ENTRIES).astype(np.int32)
    start = np.where(sigma < np.arange(ENTRIES), table[sigma], table)                        # symmetric, over the whole range
    assert np.array_equal(start[sigma], start)
    plain = m.ntuple_update_trace(start.copy(), ages, L, M, error, 2000.0, 0.9, False)
    sym = m.ntuple_update_trace(start.copy(), ages, L, M, error, 2000.0, 0.9, True)
    assert np.array_equal(sym[sigma], sym) and not np.array_equal(plain[sigma], plain)
    # the symmetric update is the plain one plus its sigma-image on the tuples; the counters took their adds once
    delta = plain.view(np.uint32) - start.view(np.uint32)
    both = delta + delta[sigma]
    both[COUNTER_BASE:] = delta[COUNTER_BASE:]
    assert np.array_equal(sym.view(np.uint32) - start.view(np.uint32), both) and delta[COUNTER_BASE:].any()
    # a board that is its own reflection under piece O (6): the entries at x = 4 with a palindromic pattern take 2 d
    rows = np.zeros(20, np.uint16)
    rows[16:] = (0b0000110000, 0b0001111000, 0b1100110011, 0b1111111111)
    assert np.array_equal(m._reflected_rows(rows), rows)
    zero = np.zeros(ENTRIES, np.int32)
    got = m.ntuple_update_trace(zero.copy(), [(rows, 6, 0, 0, 0)], L, M, np.array([1.0], np.float32), 7.0, 0.5, True)
    index, used = m.ntuple_indices(rows, 6, L, M, 0, 0)
    own = index[0][used[0]][:-1]
    middle = own[own // 256 % 153 // 17 == 4]
    assert middle.size >= 4 and np.array_equal(sigma[middle], middle) and (got[middle] == 14).all()
    # the other entries take d of their own and d as the image of their partner at 8 - x, which the board has as well
    rest = np.setdiff1d(own, middle)
    assert rest.size > 10 and set(sigma[rest].tolist()) == set(rest.tolist()) and (got[rest] == 14).all()
    assert got[index[0][-1]] == 7 and np.count_nonzero(got) == own.size + 1              # the counter once; nothing else
    # the same board under L (1): its images lie in J's rows (2), so every entry takes d once
    got = m.ntuple_update_trace(zero.copy(), [(rows, 1, 0, 0, 0)], L, M, np.array([1.0], np.float32), 7.0, 0.5, True)
    index, used = m.ntuple_indices(rows, 1, L, M, 0, 0)
    own = index[0][used[0]][:-1]
    assert (sigma[own] // (153 * 256) == 2).all() and (got[own] == 7).all() and (got[sigma[own]] == 7).all()
    assert got[index[0][-1]] == 7 and np.count_nonzero(got) == 2 * own.size + 1


# ------------------------------------------------------------------------------------------------ 3. header and build
def test_the_header_declares_the_entry_and_both_forms_of_the_kernel_use_no_scratch():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    args = re.search(r"int tpl_ntuple_update_trace\((.*?)\);", text, flags=re.S).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ["ring_a", "ring_b", "n", "slots", "head", "horizon", "L", "M", "table", "error",
                                                         "rate", "decay", "symmetric", "stream"]
    assert "tpl_ntuple_update_trace" in _m().LEARN_SYMBOLS and "mirror-symmetric" in raw.lower()
    assert re.search(r"#define\s+TPL_NTUPLE_TRACE_MAX\s+16\b", text) and _m().NTUPLE_TRACE_MAX == 16
    path = _m().build_library()
    assert hasattr(ctypes.CDLL(path), "tpl_ntuple_update_trace")
    assert T.ntuple_is_symmetric is T.ntuple.ntuple_is_symmetric
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l and "ntuple_trace_kernel" in l]
    assert len(rows) == 2, rows                                # symmetric and not
    for r in rows:
        assert r[r.index("scratch") - 1] == "0" and int(r[r.index("vgpr") - 1]) <= 128 and r[r.index("lds") - 1] == "4096", r


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_every_refusal_of_the_entry_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")
    name = b"tpl_ntuple_update_trace"

    def trace(a=fake, b=fake, n=4, slots=3, head=1, horizon=2, L=2, M=2, table=fake, error=fake, rate=1.0, decay=0.5, symmetric=0):
        return lib.tpl_ntuple_update_trace(a, b, n, slots, head, horizon, L, M, table, error, rate, decay, symmetric, None)

    # tpl_ntuple_update's list
    assert trace(a=None) < 0 and b"null" in err() and name in err()
    assert trace(b=None) < 0 and b"null" in err() and name in err()
    for n in (0, -1):
        assert trace(n=n) < 0 and b"positive" in err() and name in err(), n
    limit = -(-(1 << 31) // 40)
    for n in (limit, 1 << 40):
        assert trace(n=n, slots=1, head=0, horizon=1) < 0 and b"2^31" in err() and name in err(), n
    for plane in ("a", "b"):
        assert trace(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err(), plane
    for L_, M_ in ((0, 2), (2, 256), (251, 2), (255, 2), (2, 255), (2, 0)):
        assert trace(L=L_, M=M_) < 0 and b"L and M" in err() and name in err(), (L_, M_)
    assert trace(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
    for off in (4, 8, 12):
        assert trace(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
    assert trace(error=None) < 0 and b"null" in err() and b"error" in err() and name in err()
    assert trace(error=fake + 2) < 0 and b"error must be 4-byte aligned" in err() and name in err()
    for rate in (nan, inf, -inf):
        assert trace(rate=rate) < 0 and b"rate must be finite" in err() and name in err(), rate
    # the ring
    for slots in (0, -1, 18, 1 << 20):
        assert trace(slots=slots, head=0, horizon=1) < 0 and b"slots must be in [1, 17]" in err() and name in err(), slots
    for slots, head in ((3, -1), (3, 3), (3, 4), (1, 1), (17, 17)):
        assert trace(slots=slots, head=head, horizon=1) < 0 and b"head must be in [0, slots)" in err() and name in err(), (slots, head)
    for slots, horizon in ((3, 0), (3, -1), (3, 4), (1, 2), (17, 17), (16, 17), (17, 1 << 20)):
        assert trace(slots=slots, head=0, horizon=horizon) < 0 and b"horizon must be in [1, min(slots, 16)]" in err() and name in err()
    # slots * n at 2^31 / 40, where n alone is not
    for slots in (2, 17):
        n = -(-limit // slots)
        assert n < limit and trace(n=n, slots=slots, head=0, horizon=1) < 0 and b"2^31" in err() and b"slots" in err() and name in err()
    for decay in (-0.001, 1.001, -1.0, 2.0, nan, inf, -inf):
        assert trace(decay=decay) < 0 and b"decay must be in [0, 1]" in err() and name in err(), decay
        assert trace(decay=decay, symmetric=1) < 0 and b"decay" in err()
    # the first thing wrong is the one reported: the planes before the ring, the ring before the decay
    assert trace(a=fake + 8, slots=99) < 0 and b"aligned" in err() and b"slots" not in err()
    assert trace(slots=99, decay=2.0) < 0 and b"slots" in err() and b"decay" not in err()


def test_python_refusals_of_the_learner_need_no_gpu():
    import torch
    nt = T.ntuple
    env = _Env(8)
    learner = nt.NTupleLearner(env)
    assert (learner.lam, learner.horizon, learner.symmetric, learner.decay, learner.slots) == (0.0, 1, False, 0.0, 2)
    learner = nt.NTupleLearner(env, gamma=0.5, rate=4, epsilon=0.25, seed=3, depth=2, lam=0.8, horizon=16, symmetric=True)
    assert (learner.lam, learner.horizon, learner.symmetric, learner.decay, learner.slots) == (0.8, 16, True, 0.4, 17)
    assert tuple(learner._ring[0].shape) == (17, 8, 4) and learner._ring[1].dtype == torch.int32 and learner._head == 0
    # nothing is kept before the first step: every slot holds finished states, which the update skips
    import learn_ref as R
    kept = R.decode_state(learner._ring[0].view(-1, 4).numpy(), learner._ring[1].view(-1, 4).numpy())
    assert (kept["state"] != 0).all() and kept["rows"].sum() == 0 and kept["state"].shape == (17 * 8,)
    assert learner._kept[0].data_ptr() == learner._ring[0][0].data_ptr() and learner._next[1].data_ptr() == learner._ring[1][1].data_ptr()
    for lam in (-0.1, 1.5, float("nan"), float("inf"), True, None, "0.5"):
        with pytest.raises(ValueError, match="lam"):
            nt.NTupleLearner(env, lam=lam)
    for horizon in (0, -1, 17, 1.0, 2.5, True, None, "4"):
        with pytest.raises(ValueError, match="horizon"):
            nt.NTupleLearner(env, horizon=horizon)
    for symmetric in (0, 1, None, "yes", 1.0):
        with pytest.raises(ValueError, match="symmetric"):
            nt.NTupleLearner(env, symmetric=symmetric)
    for gamma in (1.5, -0.5):                                  # a trace cannot grow or alternate: gamma * lam stays in [0, 1]
        with pytest.raises(ValueError, match="gamma \\* lam"):
            nt.NTupleLearner(env, gamma=gamma, lam=0.9, horizon=4)
    assert nt.NTupleLearner(env, gamma=1.5).decay == 0.0       # without traces any finite gamma goes, as before
    with pytest.raises(ValueError, match="boards"):
        nt.NTupleLearner(_Env(((1 << 31) - 1) // 40 // 4), horizon=4)
    # ntuple_is_symmetric: on the host as well, and it refuses what is no table
    sigma = torch.from_numpy(_m().ntuple_mirror_permutation())
    table = nt.ntuple_table("cpu")
    assert nt.ntuple_is_symmetric(table) is True
    table[5 * 256 + 0x21] = 3
    assert nt.ntuple_is_symmetric(table) is False
    table[int(sigma[5 * 256 + 0x21])] = 3
    assert nt.ntuple_is_symmetric(table) is True
    table[COUNTER_BASE + 7] = -1                               # the counters are their own images
    assert nt.ntuple_is_symmetric(table) is True
    for bad in (table[:-1], table.to(torch.int64), table.numpy(), None):
        with pytest.raises(ValueError, match="table"):
            nt.ntuple_is_symmetric(bad)
