"""TD(lambda) traces and mirror-symmetric updates of the n-tuple learner on one MI355X (include/tpl_learn.h's rule for
tpl_ntuple_update_trace; ntuple_trace_kernel in csrc/learn/ntuple.hip; ntuple.py):

  * KERNEL: one launch leaves the numpy mirror's table byte for byte from a table over the whole int32 range -- rings filled with
    picks from the 65,560 afterstates of the pool (finished ones cut the traces at every age), horizons 1 .. 16 in rings of
    horizon, horizon + 1 and 17 slots with the head at both ends and in a wrapping middle, n around a wave and a block, decays 0 ..
    1, symmetric or not, errors with NaNs, the clamp and steps that round to 0 at the older ages only; horizon 1 without symmetry
    is tpl_ntuple_update; 4,096 copies of one state at all 16 ages; two launches give the same bytes;
  * SYMMETRY: a symmetric update keeps a symmetric table symmetric (the other one does not), the symmetric table values every state
    and its tpl_mirror_states image alike bit for bit, and a self-mirror board takes 2 d on its middle entries;
  * LEARNER: with default arguments (and with horizon 1 whatever lam) the table bytes of a TD(0) loop written here from the four
    entries; with traces the mirror's table after every step, fed from the ring read back; deterministic; forget() cuts; and on
    the two-piece game it learns, and leaves a symmetric table.
Canaries frame every buffer the kernel is handed.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import load_golden
from test_afterstates_gpu import L, M, POOL
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_gpu import ENTRIES, _fields, _framed, _full_range_table, _update, after, pool  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTER_BASE = 313344


def _m():
    return T._learn_lib


def _age(f, idx=None):
    """The mirror's fields of one age out of decoded fields (optionally the states `idx` of them)."""
    pick = (lambda v: v) if idx is None else (lambda v: v[idx])
    return tuple(pick(f[k]) for k in ("rows", "cur", "lines", "moves", "state"))


def _trace(A, B, head, horizon, start, error, rate, decay, symmetric, launches=1, game=(L, M)):
    """tpl_ntuple_update_trace of a host ring (uint32 [slots, n, 4] each) through canary-framed buffers: the table it leaves."""
    slots, n = A.shape[:2]
    a, b, t, e = _framed(A, 1), _framed(B, 2), _framed(start, 3), _framed(error, 4)
    for _ in range(launches):
        _check(_lib().tpl_ntuple_update_trace(a.ptr(), b.ptr(), n, slots, head, horizon, *game, t.ptr(), e.ptr(), rate, decay,
                                              int(symmetric), _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("error", e)):
        f.assert_canary((n, slots, head, horizon, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(e.host(), error.view(np.uint8))
    return t.host().view(np.int32).copy()


def _picks(gen, after, shape, finished=0.1):
    """Picks from the 65,560 afterstates, int `shape`: a finished one with probability `finished` (a third of the afterstates are
    finished; drawn as they come, one board in 400 would run through 16 ages)."""
    state = after["fields"]["state"]
    done, live = np.flatnonzero(state != 0), np.flatnonzero(state == 0)
    assert done.size > 4000 and live.size > 40000
    return np.where(gen.random(shape) < finished, done[gen.integers(0, done.size, shape)], live[gen.integers(0, live.size, shape)])


def _ring(after, picks):
    """Ring planes of afterstate picks (int [slots, n])."""
    return np.ascontiguousarray(after["A"][picks]), np.ascontiguousarray(after["B"][picks])


def _errors(gen, n, rate):
    """Errors of order 1 with NaNs, the clamp on both sides and steps of 1 that the first decayed weight (0.9 or less) rounds to 0;
    a launch of fewer than 100 boards gets a third of its boards of them at the most."""
    error = gen.normal(size=n).astype(np.float32)
    special = [np.nan, 1e9, -1e9] * 4 + [0.52 / rate, -0.52 / rate] * 8
    at = gen.permutation(n)[:min(len(special), n // 3)]
    error[at] = np.array(special, np.float32)[:at.size]
    return error


# ------------------------------------------------------------------------------------------------ 1. KERNEL
# (horizon, slots, head, n, decay, symmetric): every horizon in rings of horizon, horizon + 1 and 17 slots, the head at 0, at
# slots - 1 and in a middle from which the ages wrap past slot 0; every n, every decay and both forms appear several times
CASES = [
    (1, 1, 0, 4096, 0.5, 0), (1, 2, 1, 1, 0.9, 1), (1, 17, 8, 63, 1.0, 1), (1, 2, 0, 65, 0.0, 0),
    (2, 2, 0, 321, 0.9, 1), (2, 3, 2, 4096, 0.5, 0), (2, 17, 0, 65, 1.0, 1), (2, 3, 1, 1, 0.5, 0),
    (5, 5, 2, 4096, 0.9, 0), (5, 6, 5, 321, 0.5, 1), (5, 17, 3, 63, 0.0, 1), (5, 6, 0, 65, 1.0, 0),
    (16, 16, 7, 321, 0.9, 1), (16, 17, 16, 4096, 0.5, 1), (16, 17, 0, 4096, 1.0, 0), (16, 16, 15, 63, 0.9, 0),
    (16, 17, 9, 4096, 0.0, 0),
]


def test_the_cases_cover_what_they_claim():
    h, s, head, n, decay, sym = (set(c[k] for c in CASES) for k in range(6))
    assert h == {1, 2, 5, 16} and n == {1, 63, 65, 321, 4096} and decay == {0.0, 0.5, 0.9, 1.0} and sym == {0, 1}
    for horizon in h:
        mine = [c for c in CASES if c[0] == horizon]
        assert {c[1] for c in mine} == {horizon, horizon + 1, 17}
        assert any(c[2] == 0 for c in mine) and any(c[2] == c[1] - 1 for c in mine)
        assert horizon == 1 or any(c[2] < c[0] - 1 for c in mine), horizon            # the older ages wrap past slot 0
        assert horizon < 5 or any(0 < c[2] < c[0] - 1 for c in mine), horizon         # ... from a head in the middle
        assert {c[5] for c in mine} == {0, 1}


@pytest.mark.parametrize("horizon,slots,head,n,decay,symmetric", CASES)
def test_kernel_leaves_the_mirror_table_byte_for_byte(after, horizon, slots, head, n, decay, symmetric):
    f = after["fields"]
    gen = np.random.default_rng(1000 * horizon + 10 * slots + head + n)
    picks = _picks(gen, after, (slots, n))
    if n == 1:                                                 # the one board runs at age 0, or the launch would add nothing
        picks[head, 0] = np.flatnonzero(f["state"] == 0)[313]
    A, B = _ring(after, picks)
    rate = 3000.0
    error = _errors(gen, n, rate)
    start = _full_range_table(horizon + n)
    slot_of = [(head - k) % slots for k in range(horizon)]
    ages = [_age(f, picks[s]) for s in slot_of]
    got = _trace(A, B, head, horizon, start, error, rate, decay, symmetric)
    want = _m().ntuple_update_trace(start.copy(), ages, L, M, error, rate, decay, bool(symmetric))
    assert np.array_equal(got, want)
    assert (got != start).any()
    assert not (got != start)[:COUNTER_BASE][np.arange(COUNTER_BASE) % 256 == 0].any()        # the all-empty pattern: never
    # two launches from one start: the same bytes
    assert np.array_equal(_trace(A, B, head, horizon, start, error, rate, decay, symmetric), got)
    if n < 321:
        return
    # the coverage: a board stops exactly at every age, boards run through all ages, a NaN and both clamps met a running trace,
    # and (where the weights decay) a step that is not 0 at age 0 is 0 at an older age that still runs
    running = np.stack([f["state"][picks[s]] == 0 for s in slot_of])              # [horizon, n]
    stop = np.where(running.all(axis=0), horizon, np.argmin(running, axis=0))
    assert set(stop.tolist()) == set(range(horizon + 1)), sorted(set(range(horizon + 1)) - set(stop.tolist()))
    for special in (np.isnan(error), error == np.float32(1e9), error == np.float32(-1e9)):
        assert (special & (stop > 0)).any()
    d = [_m().ntuple_steps(error, np.float32(rate) * w) for w in _weights(decay, horizon)]
    assert (np.abs(d[0]) == 1 << 24).sum() >= 2
    if horizon > 1 and decay < 1.0:
        assert any(((d[0] != 0) & (d[k] == 0) & (stop > k)).any() for k in range(1, horizon))
    if horizon > 1 and decay >= 0.9:                           # (0.5^15 leaves a step only to the clamped errors)
        assert ((d[horizon - 1] != 0) & (stop == horizon)).sum() > n // 20         # and the oldest age does get its adds


def _weights(decay, horizon):
    w = [np.float32(1.0)]
    for _ in range(horizon - 1):
        w.append(np.float32(w[-1] * np.float32(decay)))
    return w


def test_horizon_one_without_symmetry_leaves_the_bytes_of_tpl_ntuple_update(after):
    gen = np.random.default_rng(2)
    n, slots, head = 4096, 3, 1
    picks = _picks(gen, after, (slots, n))
    A, B = _ring(after, picks)
    error = _errors(gen, n, 3000.0)
    start = _full_range_table(7)
    want = _update(A[head], B[head], start, error, 3000.0)
    assert (want != start).sum() > 10000
    for decay in (0.0, 0.7, 1.0):
        assert np.array_equal(_trace(A, B, head, 1, start, error, 3000.0, decay, 0), want), decay
    assert not np.array_equal(_trace(A, B, head, 1, start, error, 3000.0, 0.7, 1), want)


@pytest.mark.parametrize("symmetric", [0, 1])
def test_4096_copies_of_one_state_at_all_16_ages_where_every_add_collides(pool, symmetric):
    n, horizon = 4096, 16
    i = int(np.flatnonzero(pool.running & ((pool.fields["rows"] != 0).sum(axis=1) > 8))[5])    # a running board with rows on it
    A = np.ascontiguousarray(np.broadcast_to(pool.A[i], (horizon, n, 4)))
    B = np.ascontiguousarray(np.broadcast_to(pool.B[i], (horizon, n, 4)))
    f = _fields(A[0], B[0])
    error = np.random.default_rng(4096).normal(size=n).astype(np.float32)
    start = _full_range_table(2)
    got = _trace(A, B, 5, horizon, start, error, 50000.0, 0.9, symmetric)
    want = _m().ntuple_update_trace(start.copy(), [_age(f)] * horizon, L, M, error, 50000.0, 0.9, bool(symmetric))
    assert np.array_equal(got, want)
    index, used = _m().ntuple_indices(f["rows"][0], f["cur"][0], L, M, f["lines"][0], f["moves"][0])
    touched = index[0][used[0]]
    sigma = _m().ntuple_mirror_permutation()
    expect = np.union1d(touched, sigma[touched]) if symmetric else np.sort(touched)
    assert touched.size > 20 and np.array_equal(np.flatnonzero(got != start), expect)
    total = sum(int(_m().ntuple_steps(error, np.float32(50000.0) * w).sum()) for w in _weights(0.9, horizon))
    assert ((got[touched[-1]].astype(np.int64) - start[touched[-1]].astype(np.int64) - total) % (1 << 32) == 0)    # the counter, once


# ------------------------------------------------------------------------------------------------ 2. SYMMETRY
def _device_value(A, B, table, L=L, M=M):
    n = A.shape[0]
    a, b, t, v = _framed(A, 1), _framed(B, 2), _framed(table, 3), Framed(4 * n, 4)
    _check(_lib().tpl_ntuple_value(a.ptr(), b.ptr(), n, L, M, t.ptr(), v.ptr(), _stream()))
    v.assert_canary("value")
    return v.host().view(np.uint32).copy()


def test_symmetric_updates_keep_the_table_symmetric_and_value_a_state_and_its_mirror_alike(pool, after):
    sigma = _m().ntuple_mirror_permutation()
    gen = np.random.default_rng(3)
    n, slots, head, horizon = 4096, 5, 2, 4
    picks = _picks(gen, after, (slots, n))
    A, B = _ring(after, picks)
    error = gen.normal(size=n).astype(np.float32)
    raw = gen.integers(-(1 << 20), 1 << 20, ENTRIES).astype(np.int32)
    symmetric_start = np.where(sigma < np.arange(ENTRIES), raw[sigma], raw)
    assert np.array_equal(symmetric_start[sigma], symmetric_start) and not np.array_equal(raw[sigma], raw)
    # the mirrors of the pool's states, from the device function the samplers use
    a, b = _framed(pool.A, 5), _framed(pool.B, 6)
    out_a, out_b = Framed(POOL * 16, 7), Framed(POOL * 16, 8)
    _check(_lib().tpl_mirror_states(POOL, a.ptr(), b.ptr(), out_a.ptr(), out_b.ptr(), None, None, _stream()))
    MA, MB = out_a.host().view(np.uint32).reshape(-1, 4).copy(), out_b.host().view(np.uint32).reshape(-1, 4).copy()
    assert not np.array_equal(MA, pool.A)
    for start in (np.zeros(ENTRIES, np.int32), symmetric_start):
        sym = _trace(A, B, head, horizon, start, error, 3000.0, 0.9, 1)
        plain = _trace(A, B, head, horizon, start, error, 3000.0, 0.9, 0)
        assert np.array_equal(sym[sigma], sym) and (sym != start).sum() > 10000
        assert not np.array_equal(plain[sigma], plain)
        assert T.ntuple_is_symmetric(torch.from_numpy(sym).to(DEV)) is True
        assert T.ntuple_is_symmetric(torch.from_numpy(plain).to(DEV)) is False
        v, vm = _device_value(pool.A, pool.B, sym), _device_value(MA, MB, sym)
        assert np.array_equal(v, vm) and (v != 0).sum() > 1000
        w, wm = _device_value(pool.A, pool.B, plain), _device_value(MA, MB, plain)
        assert (w != wm).sum() > 1000
    assert T.ntuple_is_symmetric(torch.from_numpy(raw).to(DEV)) is False


def test_a_self_mirror_board_under_O_takes_two_steps_on_its_middle_entries():
    import learn_ref as R
    sigma = _m().ntuple_mirror_permutation()
    rows = np.zeros(20, np.uint16)
    rows[16:] = (0b0000110000, 0b0001111000, 0b1100110011, 0b1111111111)
    n = 65
    A1, B1 = R.pack_state(rows[None], 0, 0, 0, 0, 6)
    A, B = np.ascontiguousarray(np.broadcast_to(A1, (2, n, 4))), np.ascontiguousarray(np.broadcast_to(B1, (2, n, 4)))
    error = np.zeros(n, np.float32)
    error[64] = 1.0                                            # one board adds: d = 7
    zero = np.zeros(ENTRIES, np.int32)
    got = _trace(A, B, 0, 1, zero, error, 7.0, 0.5, 1)
    index, used = _m().ntuple_indices(rows, 6, L, M, 0, 0)
    own = index[0][used[0]][:-1]
    middle = own[own // 256 % 153 // 17 == 4]
    assert middle.size >= 4 and np.array_equal(sigma[middle], middle) and (got[middle] == 14).all()
    assert got[index[0][-1]] == 7                              # the counter: once
    assert np.array_equal(got, _m().ntuple_update_trace(zero.copy(), [(rows, 6, 0, 0, 0)], L, M, error[64:], 7.0, 0.5, True))
    plain = _trace(A, B, 0, 1, zero, error, 7.0, 0.5, 0)
    assert (plain[own] == 7).all() and np.count_nonzero(plain) == own.size + 1


# ------------------------------------------------------------------------------------------------ 3. LEARNER
def _two_piece_env(n, seed=3):
    carved = T.generate_configs(2, 2, 64, seed=107)
    return T.BatchedTetris(2, 2, n, device=DEV, seed=seed, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)


def _carved_env(n, seed=3):
    f = load_golden("carved_L5_M20.npz")
    return T.BatchedTetris(int(f["L"]), int(f["M"]), n, device=DEV, seed=seed, auto_reset=True, reward=(1.0, 10.0, -1.0),
                           config_pool=(f["rows"], f["pieces"]))


def _td0_loop(env, steps, gamma, rate, epsilon, seed):
    """TD(0) on afterstates written from the four entries: the loop NTupleLearner ran before it had a ring."""
    n, lib = env.num_envs, _lib()
    table = T.ntuple_table(DEV)
    pa, pb = T.lookahead._state_ptrs(env)
    action, done = (torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(2))
    reward, score, value, error = (torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(4))
    kept = [torch.zeros((n, 4), dtype=torch.int32, device=DEV) for _ in range(2)]
    nxt = [torch.zeros((n, 4), dtype=torch.int32, device=DEV) for _ in range(2)]
    kept[1][:, 1] = 1 << 28                                    # finished states: nothing is kept before the first step
    for step in range(steps):
        _check(lib.tpl_ntuple_act(pa, pb, n, env.L, env.M, *env.reward_params, gamma, table.data_ptr(), epsilon, seed, step,
                                  action.data_ptr(), score.data_ptr(), nxt[0].data_ptr(), nxt[1].data_ptr(), None, _stream()))
        _check(lib.tpl_ntuple_value(kept[0].data_ptr(), kept[1].data_ptr(), n, env.L, env.M, table.data_ptr(), value.data_ptr(), _stream()))
        torch.sub(score, value, out=error)
        _check(lib.tpl_ntuple_update(kept[0].data_ptr(), kept[1].data_ptr(), n, env.L, env.M, table.data_ptr(), error.data_ptr(), rate,
                                     _stream()))
        env.step_into(action, reward, done)
        kept, nxt = nxt, kept
    return table


def test_the_learner_with_default_arguments_leaves_the_bytes_of_a_td0_loop_on_the_entries():
    kw = dict(gamma=0.95, rate=16.0, epsilon=0.25, seed=5)
    tables = []
    for make in (lambda env: _td0_loop(env, 20, **kw), lambda env: T.NTupleLearner(env, **kw),
                 lambda env: T.NTupleLearner(env, lam=0.9, horizon=1, **kw)):
        env = _carved_env(64)
        env.reset()
        got = make(env)
        if isinstance(got, T.NTupleLearner):
            assert got.train(20) == 20
            got = got.table
        tables.append(_np(got).copy())
        env.terminate()
    assert np.count_nonzero(tables[0]) > 100
    assert np.array_equal(tables[1], tables[0]) and np.array_equal(tables[2], tables[0])


@pytest.mark.parametrize("game", ["carved_L5_M20", "two_piece"])
def test_the_learner_with_traces_leaves_the_mirror_table_after_every_step(game):
    n, steps, horizon = 64, 12, 4
    make = _carved_env if game == "carved_L5_M20" else _two_piece_env
    kw = dict(gamma=1.0, rate=16.0, epsilon=0.25, seed=5, lam=0.8, horizon=horizon, symmetric=True)

    def run(check):
        env = make(n)
        env.reset()
        learner = T.NTupleLearner(env, **kw)
        assert learner.slots == horizon + 1 and np.float32(learner.decay) == np.float32(0.8)
        table = np.zeros(ENTRIES, np.int32)
        cuts = full = changed = 0
        for step in range(steps):
            learner.train(1)
            if not check:
                continue
            head = (learner._head - 1) % learner.slots         # the head the update was made with
            ring = [_np(r).view(np.uint32) for r in learner._ring]
            ages = [_fields(ring[0][(head - k) % learner.slots], ring[1][(head - k) % learner.slots]) for k in range(horizon)]
            cuts += int(sum((f["state"] != 0).sum() for f in ages[:min(step, horizon)]))
            full += int(np.all([f["state"] == 0 for f in ages], axis=0).sum())
            previous = table.copy()
            _m().ntuple_update_trace(table, [_age(f) for f in ages], env.L, env.M, _np(learner._error), 16.0, np.float32(0.8), True)
            assert np.array_equal(_np(learner.table), table), step
            changed += int(not np.array_equal(table, previous))
        if check:
            # on the two-piece game every second afterstate ends the episode and cuts the trace; on the other, traces reach all ages
            assert (cuts > 0 and full == 0) if game == "two_piece" else full > 0
            assert changed >= 3 and T.ntuple_is_symmetric(learner.table) is True
            # forget(), then one step: every slot but the one act writes is finished, so nothing is added at all -- the newest kept
            # afterstate is finished too, as on the very first step
            learner.forget()
            before = learner.table.clone()
            learner.train(1)
            assert torch.equal(learner.table, before)
            learner.train(1)                                   # the step after: age 0 alone is there to update
            ring = [_np(r).view(np.uint32) for r in learner._ring]
            head = (learner._head - 1) % learner.slots
            live = [int((_fields(ring[0][(head - k) % learner.slots], ring[1][(head - k) % learner.slots])["state"] == 0).sum())
                    for k in range(horizon)]
            assert live[0] > 0 and live[1:] == [0] * (horizon - 1)
            age0 = _fields(ring[0][head], ring[1][head])
            want = _m().ntuple_update_trace(_np(before).copy(), [_age(age0)], env.L, env.M, _np(learner._error), 16.0, 0.0, True)
            assert np.array_equal(_np(learner.table), want) and not torch.equal(learner.table, before)
        out = learner.table.clone()
        env.terminate()
        return out

    run(check=True)
    a, b = run(check=False), run(check=False)
    assert torch.equal(a, b) and int((a != 0).sum()) > 100     # two trainings with one seed: the same bytes


def test_td_lambda_with_symmetry_beats_the_zero_table_on_the_two_piece_game():
    """The two-piece game of test_ntuple_gpu.py (4,096 boards, 64 carved configurations, reward (0, 1, 0), gamma 1, epsilon 0.25)
    with horizon 2, lambda 0.8 and symmetric updates.  An episode has two moves, so a trace of two afterstates spans it.  The step
    of V is about (1 + 0.8) * 2 times TD(0)'s at the same rate; rate 4 keeps it inside the range that test's docstring found to
    work for TD(0) (rate 4 .. 32).  The criterion is that test's: more than five standard errors over the zero table."""
    TRAIN, EVAL = 300, 16
    n = 4096
    env = _two_piece_env(n)
    learner = T.NTupleLearner(env, gamma=1.0, rate=4.0, epsilon=0.25, seed=5, lam=0.8, horizon=2, symmetric=True)
    before = learner.evaluate(EVAL)
    assert int(learner.table.abs().sum()) == 0
    assert learner.train(TRAIN) == TRAIN
    trained = learner.evaluate(EVAL)
    print(f"zero table: {before}; after {TRAIN} steps: {trained}; entries in use {int((learner.table != 0).sum())}, "
          f"largest {int(learner.table.abs().max())}")
    p0, p1 = before["win_rate"], trained["win_rate"]
    stderr = np.sqrt(p0 * (1 - p0) / before["episodes"] + p1 * (1 - p1) / trained["episodes"])
    print(f"win rate {p0:.4f} -> {p1:.4f}: {(p1 - p0) / stderr:.1f} standard errors of the difference")
    assert before["episodes"] >= n * EVAL // 2 // 2 and trained["episodes"] >= n * EVAL // 2 // 2
    assert p1 - p0 > 5.0 * stderr
    assert T.ntuple_is_symmetric(learner.table) is True and int((learner.table != 0).sum()) > 1000
    env.terminate()
