"""The n-tuple afterstate value function on one MI355X (include/tpl_learn.h's rule; tpl_ntuple_value, tpl_ntuple_act,
tpl_ntuple_update in csrc/learn/ntuple.hip; ntuple.py):

  * VALUE: the kernel's V is the numpy mirror's bit for bit on the 1,639 states of the afterstate pool and on their 65,560
    afterstates, under a random table; finished states give exactly 0; n = 1, 63, 65, 321;
  * ACT: action, score, afterstate planes and value are the mirror's arg-max over the C oracle's afterstates, bit for bit -- a
    random table, a small-integer one (ties), the zero table (LookaheadPolicy without a network), epsilon = 1 and 0.25 with the
    predicted draws, each optional output left out once;
  * UPDATE: one launch leaves the mirror's table byte for byte -- 65,560 states, 4,096 copies of one state, n = 1, 63, 65 --, NaN
    errors and finished states add nothing, and two launches from one start give the same bytes;
  * LEARN: on the two-piece game the trained table's greedy win rate beats the zero table's by more than five standard errors,
    and two trainings with one seed give the same table.
Canaries frame every buffer the kernels are handed.
"""
import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, Pool, _resident
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENTRIES = 314368
PARAMS = (0.1, 0.5, -0.25)
GAMMA = 0.99


def _m():
    return T._learn_lib


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def _framed(host, seed):
    """The bytes of a host array in a canary-framed device buffer."""
    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    f = Framed(raw.size, seed)
    f.inner().copy_(torch.from_numpy(raw))
    return f


def _fields(A, B):
    d = R.decode_state(A, B)
    return {k: (v if k in ("rows", "window") else v.astype(np.int64)) for k, v in d.items()}


def _mirror_value(table, f, L=L, M=M):
    return _m().ntuple_value(table, f["rows"], f["cur"], L, M, f["lines"], f["moves"], f["state"])


@pytest.fixture(scope="module")
def after(pool):
    """The 40 afterstates of every pool state from tpl_afterstates: planes [POOL * 40, 4] and their decoded fields."""
    a, b = _framed(pool.A, 1), _framed(pool.B, 2)
    out_a, out_b = Framed(POOL * 640, 3), Framed(POOL * 640, 4)
    _check(_lib().tpl_afterstates(a.ptr(), b.ptr(), POOL, L, M, *PARAMS, out_a.ptr(), out_b.ptr(), None, None, None, None, _stream()))
    A, B = out_a.host().view(np.uint32).reshape(-1, 4).copy(), out_b.host().view(np.uint32).reshape(-1, 4).copy()
    return dict(A=A, B=B, fields=_fields(A, B))


def _random_table(seed, span=1 << 20):
    return np.random.default_rng(seed).integers(-span, span + 1, ENTRIES).astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1. VALUE
def _value(A, B, table, L=L, M=M):
    n = A.shape[0]
    a, b, t, v = _framed(A, 1), _framed(B, 2), _framed(table, 3), Framed(4 * n, 4)
    v.inner().fill_(0xCD)
    _check(_lib().tpl_ntuple_value(a.ptr(), b.ptr(), n, L, M, t.ptr(), v.ptr(), _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("value", v)):
        f.assert_canary((n, k))
    assert np.array_equal(t.host().view(np.int32), table) and np.array_equal(a.host(), A.view(np.uint8).reshape(-1))
    return v.host().view(np.float32).copy()


def test_value_is_the_mirror_bit_for_bit_on_the_pool_and_its_afterstates(pool, after):
    table = _random_table(153)
    f = _fields(pool.A, pool.B)
    got, want = _value(pool.A, pool.B, table), _mirror_value(table, f)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[f["state"] != 0] == 0).all() and (f["state"] != 0).sum() > 100 and (got[f["state"] == 0] != 0).all()
    fa = after["fields"]
    got, want = _value(after["A"], after["B"], table), _mirror_value(table, fa)
    assert got.shape == (POOL * 40,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    done = fa["state"] != 0
    assert (got[done].view(np.uint32) == 0).all() and done.sum() > 4000 and (~done).sum() > 40000
    # the next piece chooses the table rows: every id appears among the afterstates, 7 ("none") included
    assert set(fa["cur"][~done].tolist()) == set(range(8))


@pytest.mark.parametrize("n", [1, 63, 65, 321])
def test_value_at_sizes_around_a_wave_and_a_block(pool, after, n):
    table = _random_table(n, span=(1 << 31) - 1)              # the whole int32 range: sums of 37 bits
    idx = (np.arange(n) * 40 + 977 * n) % (POOL * 40)
    A, B = np.ascontiguousarray(after["A"][idx]), np.ascontiguousarray(after["B"][idx])
    got, want = _value(A, B, table), _mirror_value(table, _fields(A, B))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if n > 1:                                                  # the conversion rounded: these sums are no float32 values
        assert (np.abs(got) * 65536.0 > (1 << 24)).any()


# ------------------------------------------------------------------------------------------------ 2. ACT
class Expected:
    """What the rule says of tpl_ntuple_act on the pool's states, from the ORACLE's afterstates (Pool): per table, the score of
    every placement; per draw, the action played."""

    def __init__(self, pool, L=L, M=M):
        f = pool.fields
        self.pool, self.n, self._values = pool, pool.n, {}
        self.L, self.M = L, M
        self.cur = (f["window"] & np.uint64(7)).astype(np.int64)
        self.nxt = ((f["window"] >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
        self.distinct = _m().canonical_actions(self.cur[:, None], np.arange(40)[None, :]) == np.arange(40)[None, :]
        self.reward = pool.reward(np.arange(pool.n), PARAMS)
        # the afterstate planes the oracle's outcome packs to: the move's board and counters, top-outs as state 3, the window
        # popped by one entry, the slot and the spare bit carried over; a finished board as it is
        state = np.where(pool.topout, 3, pool.state)
        A, B = R.pack_state(pool.rows.reshape(-1, 20), pool.lines.reshape(-1), pool.moves.reshape(-1), state.reshape(-1),
                            np.repeat(np.asarray(f["slot"]), 40), np.repeat(f["window"] >> np.uint64(3), 40))
        B[:, 1] |= np.repeat(f["spare"], 40) << np.uint32(31)
        run = np.repeat(pool.running, 40)
        self.A = np.where(run[:, None], A, np.repeat(pool.A, 40, axis=0)).reshape(pool.n, 40, 4)
        self.B = np.where(run[:, None], B, np.repeat(pool.B, 40, axis=0)).reshape(pool.n, 40, 4)

    def values(self, table):
        """V of all 40 oracle afterstates of every state, float32 [POOL, 40]; kept per table: it is the slow part."""
        key = hash(table.tobytes())
        if key not in self._values:
            p = self.pool
            v = _m().ntuple_value(table, p.rows.reshape(-1, 20), np.repeat(self.nxt, 40), self.L, self.M, p.lines.reshape(-1),
                                  p.moves.reshape(-1), p.done.reshape(-1))
            self._values[key] = v.reshape(p.n, 40)
        return self._values[key]

    def choice(self, table, idx, gamma=GAMMA, epsilon=0.0, seed=0, step=0):
        """(action u8, score f32, after_a, after_b u32 [n, 4], value f32, explores bool) for the states `idx` as boards 0 .. n - 1."""
        p, n = self.pool, idx.size
        v = self.values(table)[idx]
        done, run = p.done[idx], p.running[idx]
        score = np.where(done, self.reward[idx], self.reward[idx] + np.float32(gamma) * v).astype(np.float32)
        score = np.where(run[:, None], score, np.float32(0.0))
        masked = np.where(self.distinct[idx], score, -np.inf)
        greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)     # the lowest index at the maximum; -0 == +0
        explores, j = _m().ntuple_explore(seed, step, n, epsilon, np.array(_m().PIECE_PLACEMENTS)[self.cur[idx]])
        explores &= run
        order = np.argsort(~self.distinct[idx], axis=1, kind="stable")             # the distinct placements first, ascending
        action = np.where(explores, order[np.arange(n), j], greedy)
        at = np.arange(n)
        value = np.where(done[at, action], np.float32(0.0), v[at, action]).astype(np.float32)
        return (action.astype(np.uint8), score[at, greedy], self.A[idx][at, action], self.B[idx][at, action], value, explores)


@pytest.fixture(scope="module")
def expected(pool):
    return Expected(pool)


def _act(A, B, table, gamma=GAMMA, epsilon=0.0, seed=0, step=0, skip=(), L=L, M=M, params=PARAMS):
    """tpl_ntuple_act of host planes through canary-framed buffers; `skip` names the outputs passed as NULL ("after" = both)."""
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    out = dict(action=Framed(n, 4), score=Framed(4 * n, 5), after_a=Framed(16 * n, 6), after_b=Framed(16 * n, 7), value=Framed(4 * n, 8))
    for f in out.values():
        f.inner().fill_(0xCD)
    given = {k: f for k, f in out.items() if k not in skip and not (k in ("after_a", "after_b") and "after" in skip)}
    p = lambda k: given[k].ptr() if k in given else None
    _check(_lib().tpl_ntuple_act(a.ptr(), b.ptr(), n, L, M, *params, gamma, t.ptr(), epsilon, seed, step, p("action"), p("score"),
                                 p("after_a"), p("after_b"), p("value"), _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((n, epsilon, skip, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(t.host().view(np.int32), table)
    for k, f in out.items():                                   # an output that was not given is not written
        if k not in given:
            assert (f.host() == 0xCD).all(), (skip, k)
    host = {k: f.host().copy() for k, f in given.items()}
    for k in ("after_a", "after_b"):
        if k in host:
            host[k] = host[k].view(np.uint32).reshape(n, 4)
    for k in ("score", "value"):
        if k in host:
            host[k] = host[k].view(np.float32)
    return host


def _assert_choice(got, want, what):
    action, score, after_a, after_b, value, _ = want
    assert np.array_equal(got["action"], action), what
    if "score" in got:
        assert np.array_equal(got["score"].view(np.uint32), score.view(np.uint32)), what
    if "after_a" in got:
        assert np.array_equal(got["after_a"], after_a) and np.array_equal(got["after_b"], after_b), what
    if "value" in got:
        assert np.array_equal(got["value"].view(np.uint32), value.view(np.uint32)), what


def test_act_is_the_mirror_arg_max_over_the_oracle_afterstates(pool, expected):
    all_ = np.arange(POOL)
    run = pool.running
    # a random table: scores all over the place; then every optional output left out once, and all of them
    table = _random_table(40)
    want = expected.choice(table, all_)
    full = _act(pool.A, pool.B, table)
    _assert_choice(full, want, "random table")
    assert (full["action"][~run] == 0).all() and (full["score"][~run].view(np.uint32) == 0).all() and (~run).sum() > 100
    assert np.array_equal(full["after_a"][~run], pool.A[~run]) and np.array_equal(full["after_b"][~run], pool.B[~run])
    assert (full["value"][~run].view(np.uint32) == 0).all()
    assert len(set(full["action"][run].tolist())) > 20 and set(expected.cur[run].tolist()) == set(range(7))
    ended = pool.done[all_, full["action"]] & run              # chosen moves that end the game: the score is the bare reward
    assert ended.sum() > 20 and (full["value"][ended] == 0).all()
    for skip in ("score", "after", "value"):
        got = _act(pool.A, pool.B, table, skip=(skip,))
        assert set(got) == set(full) - ({"after_a", "after_b"} if skip == "after" else {skip})
        for k, v in got.items():
            assert np.array_equal(v.view(np.uint8), full[k].view(np.uint8)), (skip, k)
    got = _act(pool.A, pool.B, table, skip=("score", "after", "value"))
    assert set(got) == {"action"} and np.array_equal(got["action"], full["action"])
    # the discount reaches the score
    other = _act(pool.A, pool.B, table, gamma=0.5)
    _assert_choice(other, expected.choice(table, all_, gamma=0.5), "gamma 0.5")
    assert not np.array_equal(other["score"], full["score"])
    # small integers: many placements tie, and the lowest wins
    gen = np.random.default_rng(41)
    small = np.where(gen.random(ENTRIES) < 0.1, gen.integers(-1, 2, ENTRIES), 0).astype(np.int32) << np.int32(12)
    want = expected.choice(small, all_)
    v = expected.values(small)
    score = np.where(pool.done, expected.reward, expected.reward + np.float32(GAMMA) * v)
    masked = np.where(expected.distinct, score, -np.inf)
    ties = ((masked == masked.max(axis=1, keepdims=True)).sum(axis=1) > 1) & run
    assert ties.sum() > 100, int(ties.sum())
    _assert_choice(_act(pool.A, pool.B, small), want, "small integers")


@pytest.mark.parametrize("n", [1, 7, 9, 63, 65])
def test_act_at_sizes_around_a_block_of_eight_boards(pool, expected, n):
    table = _random_table(n)
    idx = pool.take(n, 13 * n)
    got = _act(np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx]), table)
    _assert_choice(got, expected.choice(table, idx), n)


def test_act_with_the_zero_table_is_the_lookahead_without_a_network(pool, expected):
    zero = np.zeros(ENTRIES, np.int32)
    want = expected.choice(zero, np.arange(POOL))
    _assert_choice(_act(pool.A, pool.B, zero), want, "zero table")
    env, idx = _resident(pool, POOL, 0, PARAMS)
    assert np.array_equal(idx, np.arange(POOL))
    table = T.ntuple_table(DEV)
    policy = T.NTuplePolicy(env, table, gamma=GAMMA)
    action = policy.act()
    assert action.dtype == torch.uint8 and np.array_equal(_np(action), want[0])
    assert np.array_equal(_np(action), _np(T.LookaheadPolicy(env, None).act()))
    # the Python surface on a trained-looking table: outputs into given buffers, the value function on the environment and on planes
    host = _random_table(42)
    table.copy_(torch.from_numpy(host))
    want = expected.choice(host, np.arange(POOL), epsilon=0.25, seed=9, step=4)
    explorer = T.NTuplePolicy(env, table, gamma=GAMMA, epsilon=0.25, seed=9)
    out = torch.full((POOL,), 255, dtype=torch.uint8, device=DEV)
    score, value = torch.empty(POOL, device=DEV), torch.empty(POOL, device=DEV)
    planes = (torch.empty((POOL, 4), dtype=torch.int32, device=DEV), torch.empty((POOL, 4), dtype=torch.int32, device=DEV))
    assert explorer.act(out=out, score=score, after=planes, value=value, step=4) is out
    got = dict(action=_np(out), score=_np(score), value=_np(value), after_a=_np(planes[0]).view(np.uint32), after_b=_np(planes[1]).view(np.uint32))
    _assert_choice(got, want, "NTuplePolicy")
    explorer.step = 4
    assert np.array_equal(_np(explorer.act()), want[0]) and explorer.step == 5                  # the policy's own counter
    f = _fields(pool.A, pool.B)
    assert np.array_equal(_np(T.ntuple_value(env, table)).view(np.uint32), _mirror_value(host, f).view(np.uint32))
    v_after = T.ntuple_value(planes, table, L, M)
    assert np.array_equal(_np(v_after).view(np.uint32), want[4].view(np.uint32))                # V of `after` is `value`
    with pytest.raises(ValueError, match="after"):
        explorer.act(after=(planes[0][:-1], planes[1][:-1]))
    with pytest.raises(ValueError, match="score"):
        explorer.act(score=torch.empty(POOL, dtype=torch.float64, device=DEV))
    # act() is capturable: no allocation, no sync; the replay plays the captured step
    policy = T.NTuplePolicy(env, table, gamma=GAMMA, epsilon=0.25, seed=9)
    policy.act(out=out, score=score, step=4)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        policy.act(out=out, score=score, step=4)
    out.fill_(255)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np(out), want[0]) and np.array_equal(_np(score).view(np.uint32), want[1].view(np.uint32))
    env.terminate()


@pytest.mark.parametrize("epsilon", [1.0, 0.25])
def test_act_explores_uniformly_over_the_distinct_placements_on_the_predicted_draws(pool, expected, epsilon):
    table = _random_table(43)
    all_ = np.arange(POOL)
    run = pool.running
    greedy = expected.choice(table, all_)
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    want = expected.choice(table, all_, epsilon=epsilon, seed=seed, step=step)
    got = _act(pool.A, pool.B, table, epsilon=epsilon, seed=seed, step=step)
    _assert_choice(got, want, epsilon)
    explores = want[5]
    assert not explores[~run].any() and (got["action"][~run] == 0).all()
    if epsilon == 1.0:
        assert explores[run].all()
        # the predicted j-th distinct placement, from the hash alone
        h = _m()._draw_hashes(seed, step, POOL)
        s = np.array(_m().PIECE_PLACEMENTS, dtype=np.uint64)[expected.cur]
        j = (((h & np.uint64(0xFFFFFFFF)) * s) >> np.uint64(32)).astype(np.int64)
        nth = np.array([np.flatnonzero(expected.distinct[i])[j[i]] for i in range(POOL)])
        assert np.array_equal(got["action"][run], nth[run])
        assert len(set(got["action"][run].tolist())) >= 30     # all over the placements, not at the greedy few
    else:
        frac = explores[run].mean()
        assert abs(frac - 0.25) <= 5.0 * np.sqrt(0.25 * 0.75 / run.sum()), frac                  # binomial, five standard deviations
    # the score stays the greedy one -- it is the TD target -- while action, after and value follow the draw
    assert np.array_equal(got["score"].view(np.uint32), greedy[1].view(np.uint32))
    moved = got["action"] != greedy[0]
    assert moved.sum() > (0.5 if epsilon == 1.0 else 0.1) * run.sum() and not moved[~explores].any()
    assert (got["value"][moved] != greedy[4][moved]).any() and not np.array_equal(got["after_a"][moved], greedy[2][moved])
    assert expected.distinct[all_, got["action"]].all()
    # another step, another draw; the same step, the same draw
    again = _act(pool.A, pool.B, table, epsilon=epsilon, seed=seed, step=step, skip=("score", "after", "value"))
    other = _act(pool.A, pool.B, table, epsilon=epsilon, seed=seed, step=step + 1, skip=("score", "after", "value"))
    assert np.array_equal(again["action"], got["action"]) and not np.array_equal(other["action"], got["action"])


# ------------------------------------------------------------------------------------------------ 3. UPDATE
def _update(A, B, start, error, rate, launches=1, L=L, M=M):
    n = A.shape[0]
    a, b, t, e = _framed(A, 1), _framed(B, 2), _framed(start, 3), _framed(error, 4)
    for _ in range(launches):
        _check(_lib().tpl_ntuple_update(a.ptr(), b.ptr(), n, L, M, t.ptr(), e.ptr(), rate, _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("error", e)):
        f.assert_canary((n, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(e.host(), error.view(np.uint8))
    return t.host().view(np.int32).copy()


def _mirror_update(start, f, error, rate, L=L, M=M):
    return _m().ntuple_update(start.copy(), f["rows"], f["cur"], L, M, f["lines"], f["moves"], f["state"], error, rate)


def _full_range_table(seed):
    gen = np.random.default_rng(seed)
    start = gen.integers(-(1 << 31), 1 << 31, ENTRIES).astype(np.int32)
    start[::5] = np.int32((1 << 31) - 1)                       # entries at the top of the range: their adds wrap
    return start


def test_update_leaves_the_mirror_table_byte_for_byte_on_the_afterstates(after):
    gen = np.random.default_rng(65560)
    n, f = POOL * 40, after["fields"]
    error = gen.normal(size=n).astype(np.float32)
    error[gen.integers(0, n, 500)] = np.nan
    error[gen.integers(0, n, 50)] = np.inf
    error[gen.integers(0, n, 50)] = -np.inf
    error[gen.integers(0, n, 50)] = 1e30
    start, rate = _full_range_table(1), 3000.0
    got, want = _update(after["A"], after["B"], start, error, rate), _mirror_update(start, f, error, rate)
    assert np.array_equal(got, want)
    changed = got != start
    assert changed.sum() > 20000 and changed[313344:].sum() > 50
    assert not changed[:313344][np.arange(313344) % 256 == 0].any()                  # the all-empty pattern is never updated
    # two launches from the same start: the same bytes (integer adds in any order)
    assert np.array_equal(_update(after["A"], after["B"], start, error, rate), got)
    # NaN errors add nothing, and neither do the errors of finished states
    live = (f["state"] == 0) & ~np.isnan(error)
    assert (~live).sum() > 4000
    quiet = np.where(live, np.float32(0.0), error)
    quiet[f["state"] != 0] = np.float32(7.0)
    assert np.array_equal(_update(after["A"], after["B"], start, quiet, rate), start)
    # a second launch adds the same again: the kernel only adds
    zero = np.zeros(ENTRIES, np.int32)
    finite = np.where(np.isfinite(error), error, np.float32(0.0))
    once, twice = _update(after["A"], after["B"], zero, finite, 100.0), _update(after["A"], after["B"], zero, finite, 100.0, launches=2)
    assert np.array_equal(twice, 2 * once) and np.array_equal(once, _mirror_update(zero, f, finite, 100.0))


def test_update_of_4096_copies_of_one_state_where_every_add_collides(pool):
    n = 4096
    i = int(np.flatnonzero(pool.running & ((pool.fields["rows"] != 0).sum(axis=1) > 8))[5])        # a running board with rows on it
    A, B = np.repeat(pool.A[i:i + 1], n, axis=0), np.repeat(pool.B[i:i + 1], n, axis=0)
    f = _fields(A, B)
    error = np.random.default_rng(4096).normal(size=n).astype(np.float32)
    start = _full_range_table(2)
    got = _update(A, B, start, error, 50000.0)
    assert np.array_equal(got, _mirror_update(start, f, error, 50000.0))
    index, used = _m().ntuple_indices(f["rows"][0], f["cur"][0], L, M, f["lines"][0], f["moves"][0])
    touched = index[0][used[0]]
    assert touched.size > 20 and np.array_equal(np.flatnonzero(got != start), np.sort(touched))
    total = int(_m().ntuple_steps(error, 50000.0).sum())
    assert ((got[touched].astype(np.int64) - start[touched].astype(np.int64) - total) % (1 << 32) == 0).all()
    # the clamp: errors far beyond it add 2^24 apiece, and 4,096 of them wrap to zero
    huge = np.full(n, 1e30, np.float32)
    got = _update(A, B, start, huge, 1.0)
    assert np.array_equal(got, start)                          # 4,096 * 2^24 = 2^36 = 0 mod 2^32
    got = _update(A[:255], B[:255], start, huge[:255], 1.0)
    assert ((got[touched].astype(np.int64) - start[touched].astype(np.int64) - 255 * (1 << 24)) % (1 << 32) == 0).all()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_update_at_sizes_around_a_wave(after, n):
    idx = (np.arange(n) * 41 + 313 * n) % (POOL * 40)
    if n == 1:                                                 # the one state runs, or the launch would add nothing
        idx = np.flatnonzero(after["fields"]["state"] == 0)[313:314]
    A, B = np.ascontiguousarray(after["A"][idx]), np.ascontiguousarray(after["B"][idx])
    f = _fields(A, B)
    error = np.random.default_rng(n).normal(size=n).astype(np.float32)
    start = _full_range_table(n)
    got = _update(A, B, start, error, 1234.5)
    assert np.array_equal(got, _mirror_update(start, f, error, 1234.5)) and (got != start).any()


# ------------------------------------------------------------------------------------------------ 4. LEARN
def test_td_learning_beats_the_zero_table_on_the_two_piece_game_and_is_deterministic():
    """The two-piece game (L = 2, M = 2) over 64 carved configurations, reward (0, 1, 0), 4,096 boards.  The zero table plays the
    best immediate reward and wins about one episode in six (6,060 of 34,143; the two-ply search wins them all): TD(0) has to
    learn which first placements leave a board that the second piece can finish.

    gamma = 1: an episode has two moves.  epsilon = 0.25: the 64 boards that share a configuration try each of its at most 34
    first placements within a few episodes.  rate = 8: all 4,096 boards move in lockstep and add into shared entries, so the
    step of V is rate * 2^-16 times the boards that share an entry times the entries of a state; a sweep on an MI355X
    (profiles/learner/README.md) found every rate from 4 to 32 at 100 % after 100 steps, 1 and 2 slower (rint(rate * error) is
    0 for small errors), 0.5 learning nothing, and 64 and above diverging to entries of 2^31.  8 is the middle of the range
    that works, and 300 steps three times what it needed."""
    TRAIN, EVAL = 300, 16
    n = 4096
    carved = T.generate_configs(2, 2, 64, seed=107)

    def run():
        env = T.BatchedTetris(2, 2, n, device=DEV, seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)
        learner = T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.25, seed=5)
        before = learner.evaluate(EVAL)
        assert int(learner.table.abs().sum()) == 0
        # the zero table plays the best immediate reward: evaluate_heuristic's tallies with the reward weights, win for win
        same = T.evaluate_heuristic(env, [0.0, 1.0, 0.0] + [0.0] * 9, None, EVAL)
        assert (before["episodes"], before["wins"]) == (int(same["episodes"][0]), int(same["wins"][0]))
        assert learner.train(TRAIN) == TRAIN and learner.steps == TRAIN
        result = before, learner.evaluate(EVAL), learner.table.clone()
        env.terminate()
        return result

    before, trained, table = run()
    print(f"zero table: {before}; after {TRAIN} steps: {trained}; entries in use {int((table != 0).sum())}, "
          f"largest {int(table.abs().max())}")
    for r in (before, trained):
        assert r["episodes"] >= n * EVAL // 2 // 2 and r["win_rate"] == r["wins"] / r["episodes"]
    p0, p1 = before["win_rate"], trained["win_rate"]
    stderr = np.sqrt(p0 * (1 - p0) / before["episodes"] + p1 * (1 - p1) / trained["episodes"])
    print(f"win rate {p0:.4f} -> {p1:.4f}: {(p1 - p0) / stderr:.1f} standard errors of the difference")
    assert p1 - p0 > 5.0 * stderr
    _, again, table2 = run()
    assert again == trained and torch.equal(table, table2)     # the same seed, the same bytes
