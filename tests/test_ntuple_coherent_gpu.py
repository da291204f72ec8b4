"""Temporal-coherence step sizes of the n-tuple learner on one MI355X (include/tpl_learn.h's rule for tpl_ntuple_update_coherent;
ntuple_coherent_step_kernel and ntuple_coherent_accumulate_kernel in csrc/learn/ntuple.hip; ntuple.py):

  * KERNEL: one call leaves the numpy mirror's table AND coherence buffer byte for byte -- test_ntuple_trace_gpu.py's cases (rings
    picked from the 65,560 afterstates with finished ones cutting the traces, horizons 1 .. 16, the head at both ends and in a
    wrapping middle, n around a wave and a block, decays 0 .. 1, symmetric or not, its errors), the table over the whole int32
    range, the coherence buffer holding every class of test_ntuple_coherent_cpu.COHERENCE_CLASSES; every class is met by a running
    trace and some add wraps in 64 bits; two calls from one start give the same bytes; zero coherence gives
    tpl_ntuple_update_trace's table; 4,096 copies of one state at all 16 ages;
  * SYMMETRY: a symmetric pair stays symmetric over three calls, and the table values a state and its mirror alike;
  * the toy case of test_ntuple_coherent_cpu.py through tpl_ntuple_value and the entry;
  * LEARNER: coherent=True leaves the mirror's table and coherence after every step, is deterministic, the default leaves the
    bytes of coherent=False, T.ntuple_step_sizes is the mirror's bit for bit; and on the two-piece game it learns.
Canaries frame every buffer the kernels are handed.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_coherent_cpu import COHERENCE_CLASSES, coherence_by_class, toy_assertions, toy_board
from test_ntuple_gpu import ENTRIES, _fields, _framed, _full_range_table, after, pool  # noqa: F401  (fixtures)
from test_ntuple_trace_gpu import CASES, _age, _carved_env, _device_value, _errors, _picks, _ring, _trace, _two_piece_env, _weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTER_BASE = 313344


def _m():
    return T._learn_lib


def _coherent(A, B, head, horizon, table, coherence, error, rate, decay, symmetric, calls=1, game=(L, M)):
    """tpl_ntuple_update_coherent of a host ring (uint32 [slots, n, 4] each) through canary-framed buffers: (table, coherence)."""
    slots, n = A.shape[:2]
    a, b, t, c, e = _framed(A, 1), _framed(B, 2), _framed(table, 3), _framed(coherence, 5), _framed(error, 4)
    assert c.ptr() % 16 == 0 and t.ptr() % 16 == 0
    for _ in range(calls):
        _check(_lib().tpl_ntuple_update_coherent(a.ptr(), b.ptr(), n, slots, head, horizon, *game, t.ptr(), c.ptr(), e.ptr(), rate,
                                                 decay, int(symmetric), _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("coherence", c), ("error", e)):
        f.assert_canary((n, slots, head, horizon, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(e.host(), error.view(np.uint8))
    return t.host().view(np.int32).copy(), c.host().view(np.int64).reshape(ENTRIES, 2).copy()


# ------------------------------------------------------------------------------------------------ 1. KERNEL
@pytest.mark.parametrize("horizon,slots,head,n,decay,symmetric", CASES)
def test_kernels_leave_the_mirror_table_and_coherence_byte_for_byte(after, horizon, slots, head, n, decay, symmetric):
    f = after["fields"]
    gen = np.random.default_rng(1000 * horizon + 10 * slots + head + n)
    picks = _picks(gen, after, (slots, n))
    if n == 1:                                                 # the one board runs at age 0, or the call would add nothing
        picks[head, 0] = np.flatnonzero(f["state"] == 0)[313]
    A, B = _ring(after, picks)
    rate = 3000.0
    error = _errors(gen, n, rate)
    start = _full_range_table(horizon + n)
    coherence, which = coherence_by_class(horizon + n)
    slot_of = [(head - k) % slots for k in range(horizon)]
    ages = [_age(f, picks[s]) for s in slot_of]
    got_t, got_c = _coherent(A, B, head, horizon, start, coherence, error, rate, decay, symmetric)
    want_t, want_c = _m().ntuple_update_coherent(start.copy(), coherence.copy(), ages, L, M, error, rate, decay, bool(symmetric))
    assert np.array_equal(got_c, want_c)
    assert np.array_equal(got_t, want_t)
    touched = np.flatnonzero((got_c != coherence).any(axis=1))
    assert touched.size > 0 and (got_t != start).any()
    assert np.isin(np.flatnonzero(got_t != start), touched).all()
    assert not (touched[touched < COUNTER_BASE] % 256 == 0).any()                             # the all-empty pattern: never
    # the table is NOT the plain update's: step sizes below 1 were read
    plain = _m().ntuple_update_trace(start.copy(), ages, L, M, error, rate, decay, bool(symmetric))
    assert n == 1 or not np.array_equal(got_t, plain)
    # two calls from one start: the same bytes
    again_t, again_c = _coherent(A, B, head, horizon, start, coherence, error, rate, decay, symmetric)
    assert np.array_equal(again_t, got_t) and np.array_equal(again_c, got_c)
    if n < 321:
        return
    # the coverage: every class of a pair was met by a running trace, an add wrapped in 64 bits, a step rounded to 0 where d did not
    assert set(which[touched].tolist()) == set(range(len(COHERENCE_CLASSES)))
    names = [c[0] for c in COHERENCE_CLASSES]
    assert (got_c[touched, 1] < coherence[touched, 1]).any()                        # A only grows, unless it wraps
    top = touched[which[touched] == names.index("the next add wraps")]             # E six below the top of the range
    assert (got_c[top, 0] < 0).any()
    still = touched[which[touched] == names.index("E = 0")]                       # alpha 0: the table stays, E and A do not
    assert still.size > 0 and (got_t[still] == start[still]).all() and (plain[still] != start[still]).any()
    small = touched[which[touched] == names.index("a small ratio: s rounds to 0")]
    assert ((got_t[small] == start[small]) & (plain[small] != start[small])).any()
    d0 = _m().ntuple_steps(error, np.float32(rate))
    assert (np.abs(d0) == 1 << 24).sum() >= 2 and np.isnan(error).any()


def test_zero_coherence_gives_the_table_bytes_of_tpl_ntuple_update_trace(after):
    gen = np.random.default_rng(2)
    n, slots, head, horizon = 4096, 5, 1, 4
    f = after["fields"]
    picks = _picks(gen, after, (slots, n))
    A, B = _ring(after, picks)
    error = _errors(gen, n, 3000.0)
    start = _full_range_table(7)
    zero = np.zeros((ENTRIES, 2), np.int64)
    ages = [_age(f, picks[(head - k) % slots]) for k in range(horizon)]
    for symmetric in (0, 1):
        want = _trace(A, B, head, horizon, start, error, 3000.0, 0.9, symmetric)
        got_t, got_c = _coherent(A, B, head, horizon, start, zero, error, 3000.0, 0.9, symmetric)
        assert np.array_equal(got_t, want) and (want != start).sum() > 10000
        _, want_c = _m().ntuple_update_coherent(start.copy(), zero.copy(), ages, L, M, error, 3000.0, 0.9, bool(symmetric))
        assert np.array_equal(got_c, want_c) and (got_c[:, 1] > 0).sum() > 10000 and (np.abs(got_c[:, 0]) <= got_c[:, 1]).all()


@pytest.mark.parametrize("symmetric", [0, 1])
def test_4096_copies_of_one_state_at_all_16_ages_where_every_add_collides(pool, symmetric):
    n, horizon = 4096, 16
    i = int(np.flatnonzero(pool.running & ((pool.fields["rows"] != 0).sum(axis=1) > 8))[5])    # a running board with rows on it
    A = np.ascontiguousarray(np.broadcast_to(pool.A[i], (horizon, n, 4)))
    B = np.ascontiguousarray(np.broadcast_to(pool.B[i], (horizon, n, 4)))
    f = _fields(A[0], B[0])
    error = np.random.default_rng(4096).normal(size=n).astype(np.float32)
    error[:256], error[256:512] = 1e9, -1e9                    # two whole blocks at the clamp at every age: a block's counter sums
                                                               # are 2^32 and -2^32, which 32 bits would have lost
    start = _full_range_table(2)
    coherence, _ = coherence_by_class(4096)
    rate = 50000.0
    got_t, got_c = _coherent(A, B, 5, horizon, start, coherence, error, rate, 0.9, symmetric)
    want_t, want_c = _m().ntuple_update_coherent(start.copy(), coherence.copy(), [_age(f)] * horizon, L, M, error, rate, 0.9,
                                                 bool(symmetric))
    assert np.array_equal(got_c, want_c) and np.array_equal(got_t, want_t)
    index, used = _m().ntuple_indices(f["rows"][0], f["cur"][0], L, M, f["lines"][0], f["moves"][0])
    touched = index[0][used[0]]
    sigma = _m().ntuple_mirror_permutation()
    expect = np.union1d(touched, sigma[touched]) if symmetric else np.sort(touched)
    assert touched.size > 20 and np.array_equal(np.flatnonzero((got_c != coherence).any(axis=1)), expect)
    assert np.isin(np.flatnonzero(got_t != start), expect).all()                   # nothing outside the entries, nor their images
    # the counter, once, and in 64 bits: the sums are past 2^32, which a block's 32-bit sums would have lost
    d = [_m().ntuple_steps(error, np.float32(rate) * w) for w in _weights(0.9, horizon)]
    total, absolute = sum(int(x.sum()) for x in d), sum(int(np.abs(x).sum()) for x in d)
    counter = touched[-1]
    assert counter >= COUNTER_BASE and absolute > 1 << 32
    assert (int(got_c[counter, 0]) - int(coherence[counter, 0]) - total) % (1 << 64) == 0
    assert (int(got_c[counter, 1]) - int(coherence[counter, 1]) - absolute) % (1 << 64) == 0


# ------------------------------------------------------------------------------------------------ 2. SYMMETRY
def test_a_symmetric_pair_stays_symmetric_and_values_a_state_and_its_mirror_alike(pool, after):
    sigma = _m().ntuple_mirror_permutation()
    gen = np.random.default_rng(3)
    n, slots, head, horizon = 4096, 5, 2, 4
    picks = _picks(gen, after, (slots, n))
    A, B = _ring(after, picks)
    lower = sigma < np.arange(ENTRIES)
    raw = gen.integers(-(1 << 20), 1 << 20, ENTRIES).astype(np.int32)
    table = np.where(lower, raw[sigma], raw)
    coherence, _ = coherence_by_class(33)
    coherence = np.where(lower[:, None], coherence[sigma], coherence)
    assert np.array_equal(table[sigma], table) and np.array_equal(coherence[sigma], coherence)
    t, c = table, coherence
    for call in range(3):
        error = gen.normal(size=n).astype(np.float32)
        t, c = _coherent(A, B, head, horizon, t, c, error, 3000.0, 0.9, 1)
        assert np.array_equal(t[sigma], t) and np.array_equal(c[sigma], c), call
        assert T.ntuple_is_symmetric(torch.from_numpy(t).to(DEV)) is True
    assert (t != table).sum() > 10000 and (c != coherence).any(axis=1).sum() > 10000
    plain_t, plain_c = _coherent(A, B, head, horizon, table, coherence, error, 3000.0, 0.9, 0)
    assert not np.array_equal(plain_t[sigma], plain_t) and not np.array_equal(plain_c[sigma], plain_c)
    # the mirrors of the pool's states, from the device function the samplers use
    a, b = _framed(pool.A, 5), _framed(pool.B, 6)
    out_a, out_b = Framed(POOL * 16, 7), Framed(POOL * 16, 8)
    _check(_lib().tpl_mirror_states(POOL, a.ptr(), b.ptr(), out_a.ptr(), out_b.ptr(), None, None, _stream()))
    MA, MB = out_a.host().view(np.uint32).reshape(-1, 4).copy(), out_b.host().view(np.uint32).reshape(-1, 4).copy()
    v, vm = _device_value(pool.A, pool.B, t), _device_value(MA, MB, t)
    assert np.array_equal(v, vm) and (v != 0).sum() > 1000
    w, wm = _device_value(pool.A, pool.B, plain_t), _device_value(MA, MB, plain_t)
    assert (w != wm).sum() > 100


# ------------------------------------------------------------------------------------------------ 3. THE TOY CASE
def test_the_toy_case_on_the_device_diverges_plain_and_settles_coherent():
    import learn_ref as R
    state, entries, rate = toy_board()
    n = 64
    A, B = R.pack_state(state[0], state[2], state[3], state[4], 0, state[1].astype(np.uint64))
    a, b = _framed(A, 1), _framed(B, 2)
    target = 10.0
    runs = []
    for coherent in (False, True):
        table, coherence = Framed(4 * ENTRIES, 3), Framed(16 * ENTRIES, 4)
        value, error = Framed(4 * n, 5), Framed(4 * n, 6)
        errors = []
        for step in range(61):
            _check(_lib().tpl_ntuple_value(a.ptr(), b.ptr(), n, 10, 40, table.ptr(), value.ptr(), _stream()))
            e = target - value.inner().view(torch.float32)
            error.inner().view(torch.float32).copy_(e)
            errors.append(abs(float(e[0])))
            assert bool((e == e[0]).all())
            if coherent:
                _check(_lib().tpl_ntuple_update_coherent(a.ptr(), b.ptr(), n, 1, 0, 1, 10, 40, table.ptr(), coherence.ptr(), error.ptr(),
                                                         rate, 0.0, 0, _stream()))
            else:
                _check(_lib().tpl_ntuple_update_trace(a.ptr(), b.ptr(), n, 1, 0, 1, 10, 40, table.ptr(), error.ptr(), rate, 0.0, 0,
                                                      _stream()))
        for k, f in (("a", a), ("b", b), ("table", table), ("coherence", coherence), ("value", value), ("error", error)):
            f.assert_canary(k)
        runs.append(errors)
    print("plain", [f"{e:.3g}" for e in runs[0][:45]], "coherent", [f"{e:.3g}" for e in runs[1]])
    toy_assertions(*runs, rate)


# ------------------------------------------------------------------------------------------------ 4. LEARNER
@pytest.mark.parametrize("game", ["carved_L5_M20", "two_piece"])
def test_the_coherent_learner_leaves_the_mirror_table_and_coherence_after_every_step(game):
    n, steps, horizon = 64, 12, 4
    make = _carved_env if game == "carved_L5_M20" else _two_piece_env
    kw = dict(gamma=1.0, rate=16.0, epsilon=0.25, seed=5, lam=0.8, horizon=horizon, symmetric=True)
    # from the zeroed buffer, and -- the buffer is a plain tensor -- from a mirror-symmetric one that holds every class of a pair:
    # twelve steps from zero send most entries errors of one sign and leave every step size at 1
    sigma = _m().ntuple_mirror_permutation()
    classes, _ = coherence_by_class(12)
    classes = np.where((sigma < np.arange(ENTRIES))[:, None], classes[sigma], classes)
    zero = np.zeros((ENTRIES, 2), np.int64)

    def run(check, start=zero, **more):
        env = make(n)
        env.reset()
        learner = T.NTupleLearner(env, **kw, **more)
        table, coherence = np.zeros(ENTRIES, np.int32), start.copy()
        if learner.coherent:
            assert not bool(learner.coherence.any())
            learner.coherence.copy_(torch.from_numpy(start))
        slowed = 0
        for step in range(steps):
            learner.train(1)
            if not check:
                continue
            head = (learner._head - 1) % learner.slots         # the head the update was made with
            ring = [_np(r).view(np.uint32) for r in learner._ring]
            ages = [_fields(ring[0][(head - k) % learner.slots], ring[1][(head - k) % learner.slots]) for k in range(horizon)]
            _m().ntuple_update_coherent(table, coherence, [_age(f) for f in ages], env.L, env.M, _np(learner._error), 16.0,
                                        np.float32(0.8), True)
            assert np.array_equal(_np(learner.coherence), coherence), step
            assert np.array_equal(_np(learner.table), table), step
            alpha = _m().ntuple_step_sizes(coherence)
            assert np.array_equal(_np(T.ntuple_step_sizes(learner.coherence)).view(np.uint32), alpha.view(np.uint32)), step
            slowed += int((np.abs(table) < np.abs(coherence[:, 0] - start[:, 0])).sum())       # steps taken at less than the full rate
        if check:
            assert np.count_nonzero(table) > 100
            assert slowed > 0 or start is zero                 # step sizes below 1 were in play
            alpha = T.ntuple_step_sizes(learner.coherence)
            assert alpha.device == learner.coherence.device and alpha.dtype == torch.float32
            assert np.array_equal(_np(alpha).view(np.uint32), _m().ntuple_step_sizes(coherence).view(np.uint32))
            assert T.ntuple_is_symmetric(learner.table) is True
            assert np.array_equal(coherence[sigma], coherence)
            before = learner.coherence.clone()
            learner.forget()                                   # cuts the ring and leaves the coherence buffer alone
            assert torch.equal(learner.coherence, before)
        out = learner.table.clone(), (learner.coherence.clone() if learner.coherent else None)
        env.terminate()
        return out

    run(check=True, coherent=True)
    run(check=True, start=classes, coherent=True)
    a, b = run(check=False, start=classes, coherent=True), run(check=False, start=classes, coherent=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int((a[0] != 0).sum()) > 100    # one seed: the same bytes of both
    default, off = run(check=False), run(check=False, coherent=False)
    assert default[1] is None and torch.equal(default[0], off[0]) and not torch.equal(default[0], a[0])


def test_the_step_sizes_in_torch_are_the_mirror_bit_for_bit_on_every_class():
    coherence, _ = coherence_by_class(77)
    got = T.ntuple_step_sizes(torch.from_numpy(coherence).to(DEV))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (ENTRIES,)
    assert np.array_equal(_np(got).view(np.uint32), _m().ntuple_step_sizes(coherence).view(np.uint32))
    fresh = T.ntuple_coherence(DEV)
    assert fresh.is_cuda and fresh.dtype == torch.int64 and tuple(fresh.shape) == (ENTRIES, 2) and not bool(fresh.any())
    assert bool((T.ntuple_step_sizes(fresh) == 1.0).all())


def test_the_coherent_learner_beats_the_zero_table_on_the_two_piece_game():
    """The two-piece game of test_ntuple_gpu.py (4,096 boards, 64 carved configurations, reward (0, 1, 0), gamma 1, epsilon 0.25) at
    rate 8 with coherent=True, 300 steps.  Coherent steps are never larger than plain ones, and the plain learner at an eighth of
    this rate stands at 0.67 against the zero table's 0.1775 after 100 steps.  The criterion is that test's: more than five
    standard errors of the difference over the zero table."""
    TRAIN, EVAL = 300, 16
    n = 4096
    env = _two_piece_env(n)
    learner = T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.25, seed=5, coherent=True)
    before = learner.evaluate(EVAL)
    assert int(learner.table.abs().sum()) == 0 and int(learner.coherence.abs().sum()) == 0
    assert learner.train(TRAIN) == TRAIN
    trained = learner.evaluate(EVAL)
    alpha = T.ntuple_step_sizes(learner.coherence)[learner.coherence[:, 1] > 0]
    print(f"zero table: {before}; after {TRAIN} steps: {trained}; entries in use {int((learner.table != 0).sum())}, "
          f"largest {int(learner.table.abs().max())}; alpha over the {alpha.numel()} entries sent a step: mean {float(alpha.mean()):.3f}, "
          f"below 0.5: {int((alpha < 0.5).sum())}")
    p0, p1 = before["win_rate"], trained["win_rate"]
    stderr = np.sqrt(p0 * (1 - p0) / before["episodes"] + p1 * (1 - p1) / trained["episodes"])
    print(f"win rate {p0:.4f} -> {p1:.4f}: {(p1 - p0) / stderr:.1f} standard errors of the difference")
    assert before["episodes"] >= n * EVAL // 2 // 2 and trained["episodes"] >= n * EVAL // 2 // 2
    assert p1 - p0 > 5.0 * stderr
    assert int((learner.coherence[:, 1] > 0).sum()) > 1000
    env.terminate()
