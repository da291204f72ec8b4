"""The 3 x 3 table shape of the n-tuple value function on one MI355X (include/tpl_learn.h's "Table shapes"; the ntuple3_* kernels of
csrc/learn/ntuple.hip behind the six _shaped entries; ntuple.py).  Every kernel is held to the numpy mirror of _learn_lib.py bit
for bit -- floats compared as bits -- on the state set of the existing n-tuple tests: the 1,639 states of the afterstate pool and
their 65,560 afterstates, at n = 1, 7, 9, 257 and the whole set.

  * COVERAGE (on the host): the set has cells in rows 17..19 and columns 0 and 9 -- the last windows are at y = 17 and x = 7 --, a
    full-height column, every falling piece and finished states;
  * VALUE under a random table in +-2^20;
  * ACT and SEARCH: action, score, afterstate planes, value and `second` are the numpy rule's, composed as test_ntuple_search_gpu
    composes it, at epsilon 0 and 0.25;
  * UPDATE, and UPDATE_TRACE at horizon 1, 4 and 16 in a ring of 17 slots whose head wraps, symmetric and not, with errors 0, NaN
    and past the clamp: the mirror's table bytes; symmetric updates leave a symmetric table;
  * UPDATE_COHERENT: table and coherence bytes, from a zero buffer and a filled one, and the same bytes with the boards permuted;
  * SHAPE 0 through the new entries writes the bytes of the existing twin;
  * LEARNER: on the two-piece game a 3 x 3 learner is deterministic and gains at least half of what the 2 x 4 learner gains over the
    zero table in the same run; depth 2 and the coherent symmetric form run on it.
Canaries frame every buffer the kernels are handed.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL
from test_heuristic_gpu import _planes
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_gpu import GAMMA, PARAMS, Expected, _act, _assert_choice, _fields, _framed, _update, _value, after, pool  # noqa: F401
from test_ntuple_search_gpu import _same, _search
from test_ntuple_trace_gpu import _age, _picks, _ring, _trace

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TUPLES, PATTERNS, COUNTER_BASE, ENTRIES = 144, 512, 589824, 590848
ENTRIES_2X4 = 314368
SIZES = [1, 7, 9, 257]                                         # no multiple of an act block's 8 boards nor of 256
ARANGE = np.arange(40)
SLOTS, HEAD = 17, 2                                            # ages 0, 1, 2 in slots 2, 1, 0; age 3 wraps to slot 16


def _m():
    return T._learn_lib


def _table(seed, span=1 << 20, entries=ENTRIES):
    return np.random.default_rng(seed).integers(-span, span + 1, entries).astype(np.int32)


def _full_range(seed, entries=ENTRIES):
    start = np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, entries).astype(np.int32)
    start[::5] = np.int32((1 << 31) - 1)                       # entries at the top of the range: their adds wrap
    return start


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the entries, framed
def _value3(A, B, table, shape=1, L=L, M=M):
    n = A.shape[0]
    a, b, t, v = _framed(A, 1), _framed(B, 2), _framed(table, 3), Framed(4 * n, 4)
    v.inner().fill_(0xCD)
    _check(_lib().tpl_ntuple_value_shaped(a.ptr(), b.ptr(), n, L, M, t.ptr(), v.ptr(), shape, _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("value", v)):
        f.assert_canary((n, k))
    assert np.array_equal(t.host().view(np.int32), table) and np.array_equal(a.host(), A.view(np.uint8).reshape(-1))
    return v.host().view(np.float32).copy()


def _policy3(depth, A, B, table, gamma=GAMMA, epsilon=0.0, seed=0, step=0, shape=1, L=L, M=M):
    """tpl_ntuple_act_shaped (depth 1) or tpl_ntuple_search_shaped (depth 2) of host planes through canary-framed buffers."""
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, second=1, score=4, after_a=16, after_b=16, value=4)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    head = (a.ptr(), b.ptr(), n, L, M, *PARAMS, gamma, t.ptr(), epsilon, seed, step, p("action"))
    tail = (p("score"), p("after_a"), p("after_b"), p("value"), shape, _stream())
    if depth == 2:
        _check(_lib().tpl_ntuple_search_shaped(*head, p("second"), *tail))
    else:
        _check(_lib().tpl_ntuple_act_shaped(*head, *tail))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((depth, n, epsilon, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(t.host().view(np.int32), table)
    if depth == 1:
        assert (out.pop("second").host() == 0xCD).all()
    host = {k: f.host().copy() for k, f in out.items()}
    for k in ("after_a", "after_b"):
        host[k] = host[k].view(np.uint32).reshape(n, 4)
    for k in ("score", "value"):
        host[k] = host[k].view(np.float32)
    return host


def _trace3(A, B, head, horizon, start, error, rate, decay, symmetric, shape=1, coherence=None, planes=False, L=L, M=M):
    """tpl_ntuple_update_trace_shaped of a host ring (uint32 [slots, n, 4] each), tpl_ntuple_update_coherent_shaped where a
    coherence buffer is given, tpl_ntuple_update_shaped of planes [n, 4] with planes=True: the table (and the buffer) it leaves."""
    slots, n = (1, A.shape[0]) if planes else A.shape[:2]
    a, b, t, e = _framed(A, 1), _framed(B, 2), _framed(start, 3), _framed(error, 4)
    c = None if coherence is None else _framed(coherence, 5)
    if planes:
        _check(_lib().tpl_ntuple_update_shaped(a.ptr(), b.ptr(), n, L, M, t.ptr(), e.ptr(), rate, shape, _stream()))
    elif c is None:
        _check(_lib().tpl_ntuple_update_trace_shaped(a.ptr(), b.ptr(), n, slots, head, horizon, L, M, t.ptr(), e.ptr(), rate, decay,
                                                     int(symmetric), shape, _stream()))
    else:
        _check(_lib().tpl_ntuple_update_coherent_shaped(a.ptr(), b.ptr(), n, slots, head, horizon, L, M, t.ptr(), c.ptr(), e.ptr(),
                                                        rate, decay, int(symmetric), shape, _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("error", e)) + (() if c is None else (("coherence", c),)):
        f.assert_canary((n, slots, head, horizon, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(e.host(), error.view(np.uint8))
    table = t.host().view(np.int32).copy()
    return table if c is None else (table, c.host().view(np.int64).reshape(-1, 2).copy())


# ------------------------------------------------------------------------------------------------ COVERAGE
@pytest.fixture(scope="module")
def mirror(pool, after):
    """The 3 x 3 indices of the whole set, once: the pool's states and their afterstates."""
    out = {}
    for name, f in (("pool", _fields(pool.A, pool.B)), ("after", after["fields"])):
        index, used = _m().ntuple_indices(f["rows"], f["cur"], L, M, f["lines"], f["moves"], shape="3x3")
        out[name] = dict(fields=f, index=index, used=used)
    return out


def _mirror_value(table, part):
    f = part["fields"]
    total = np.where(part["used"], table[part["index"]].astype(np.int64), 0).sum(axis=1)
    return np.where(f["state"] == 0, total.astype(np.float32) * np.float32(2.0 ** -16), np.float32(0.0)).astype(np.float32)


def test_the_state_set_reaches_the_last_windows_every_piece_and_finished_states(mirror):
    """Counted on the host, on running states.  The pool of 1,639 states gives on its own: a non-empty window at y = 17 in 1,326
    states, at x = 7 in 1,302, at x = 0 in 1,325, the corner window (7, 17) in 1,301; cells in rows 17..19 in 1,326, in column 0 in
    1,226, in column 9 in 1,220; a full-height column in 18; at least 133 states a piece; 205 finished.  Each floor is half of
    that, and the afterstates' floors are half of what tpl_afterstates gives of them."""
    seen = {}
    for name, part in mirror.items():
        f, used = part["fields"], part["used"][:, :TUPLES].reshape(-1, 8, 18)
        run = f["state"] == 0
        cols = np.stack([(f["rows"].astype(np.int64) >> x) & 1 for x in range(10)], axis=2)        # [K, 20, 10]
        seen[name] = dict(
            last_row_window=int((used[:, :, 17].any(axis=1) & run).sum()), last_column_window=int((used[:, 7, :].any(axis=1) & run).sum()),
            first_column_window=int((used[:, 0, :].any(axis=1) & run).sum()), corner_window=int((used[:, 7, 17] & run).sum()),
            rows_17_to_19=int(((f["rows"][:, 17:] != 0).any(axis=1) & run).sum()),
            column_0=int((cols[:, :, 0].any(axis=1) & run).sum()), column_9=int((cols[:, :, 9].any(axis=1) & run).sum()),
            full_column=int(((cols.sum(axis=1) == 20).any(axis=1) & run).sum()), finished=int((~run).sum()),
            pieces=np.bincount(f["cur"][run], minlength=8).tolist())
        print(name, seen[name])
    p, a = seen["pool"], seen["after"]
    assert p["rows_17_to_19"] >= 663 and p["column_0"] >= 613 and p["column_9"] >= 610 and p["full_column"] >= 9 and p["finished"] >= 102
    assert p["last_row_window"] >= 663 and p["last_column_window"] >= 651 and p["first_column_window"] >= 662 and p["corner_window"] >= 650
    assert min(p["pieces"][:7]) >= 66
    # the 65,560 afterstates give 44,260 / 41,434 / 41,221 / 41,398 windows, 37,079 and 38,206 edge columns, 512 full columns, 21,048
    # finished states and at least 5,223 running states a piece, "none" among them
    assert a["last_row_window"] >= 22130 and a["last_column_window"] >= 20717 and a["first_column_window"] >= 20610
    assert a["corner_window"] >= 20699 and a["column_0"] >= 18539 and a["column_9"] >= 19103
    assert a["full_column"] >= 256 and a["finished"] >= 10524 and min(a["pieces"]) >= 2611


# ------------------------------------------------------------------------------------------------ VALUE
def test_value_is_the_mirror_bit_for_bit_on_the_whole_set(pool, after, mirror):
    table = _table(144)
    for name, (A, B) in (("pool", (pool.A, pool.B)), ("after", (after["A"], after["B"]))):
        got, want = _value3(A, B, table), _mirror_value(table, mirror[name])
        assert np.array_equal(_bits(got), _bits(want)), name
        done = mirror[name]["fields"]["state"] != 0
        assert (_bits(got)[done] == 0).all() and (got[~done] != 0).all()
    # the 2 x 4 kernel on the same planes gives another number: the shape is not ignored
    assert not np.array_equal(got, _value(after["A"], after["B"], _table(144, entries=ENTRIES_2X4)))


@pytest.mark.parametrize("n", SIZES)
def test_value_at_sizes_around_the_block_edges(after, mirror, n):
    table = _table(n, span=(1 << 31) - 1)                      # the whole int32 range: sums of 37 bits, rounded at the conversion
    idx = (np.arange(n) * 40 + 977 * n) % (POOL * 40)
    if n == 1:
        idx = np.flatnonzero(after["fields"]["state"] == 0)[977:978]
    A, B = np.ascontiguousarray(after["A"][idx]), np.ascontiguousarray(after["B"][idx])
    part = dict(fields={k: v[idx] for k, v in after["fields"].items()}, index=mirror["after"]["index"][idx], used=mirror["after"]["used"][idx])
    got = _value3(A, B, table)
    assert np.array_equal(_bits(got), _bits(_mirror_value(table, part))) and (got != 0).any()


# ------------------------------------------------------------------------------------------------ ACT and SEARCH
@pytest.fixture(scope="module")
def expected(pool):
    return Expected(pool)                                      # its values() take the shape from the table they are given


@pytest.fixture(scope="module")
def table3():
    return _table(40)


@pytest.mark.parametrize("n", SIZES + [POOL])
def test_act_is_the_mirror_arg_max_at_both_epsilons(pool, expected, table3, n):
    idx = pool.take(n, 0 if n == POOL else 13 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    for epsilon in (0.0, 0.25):
        want = expected.choice(table3, idx, epsilon=epsilon, seed=seed, step=step)
        got = _policy3(1, A, B, table3, epsilon=epsilon, seed=seed, step=step)
        _assert_choice(got, want, (n, epsilon))
    if n == POOL:
        run = pool.running
        greedy = expected.choice(table3, idx)
        assert want[5].sum() > 0.15 * run.sum() and (got["action"] != greedy[0]).sum() > 0.1 * run.sum()
        assert (got["action"][~run] == 0).all() and (_bits(got["score"])[~run] == 0).all() and (_bits(got["value"])[~run] == 0).all()
        assert np.array_equal(got["after_a"][~run], pool.A[~run]) and np.array_equal(got["after_b"][~run], pool.B[~run])
        assert len(set(greedy[0][run].tolist())) > 20
        # the 2 x 4 kernel under a 2 x 4 table does not play the same game
        other = _act(pool.A, pool.B, _table(40, entries=ENTRIES_2X4))
        assert (other["action"] != greedy[0]).sum() >= 100


class Composed:
    """tpl_ntuple_search's rule put together as test_ntuple_search_gpu.Composed does, from one-ply pieces over the 40 n afterstates
    of tpl_afterstates: Q(a) = r1 + gamma * score'(s_a) and second(a) = action'(s_a), (score', action') the 3 x 3 one-ply policy on
    the afterstate -- held to the numpy rule by the act tests above --, V(s_a) from the numpy mirror."""

    def __init__(self, A, B, table, gamma, L=L, M=M):
        n = self.n = A.shape[0]
        a, b = _planes(A, B)
        out_a, out_b = Framed(n * 640, 3), Framed(n * 640, 4)
        reward, done, canonical = Framed(n * 160, 5), Framed(n * 40, 6), Framed(n * 40, 7)
        _check(_lib().tpl_afterstates(a.ptr(), b.ptr(), n, L, M, *PARAMS, out_a.ptr(), out_b.ptr(), reward.ptr(), done.ptr(), None,
                                      canonical.ptr(), _stream()))
        self.A = out_a.host().view(np.uint32).reshape(-1, 4).copy()
        self.B = out_b.host().view(np.uint32).reshape(-1, 4).copy()
        r1 = reward.host().view(np.float32).reshape(n, 40).copy()
        self.done1 = done.host().reshape(n, 40) != 0
        self.distinct = canonical.host().reshape(n, 40) == ARANGE[None, :]
        ply = _policy3(1, self.A, self.B, table, gamma=gamma, L=L, M=M)
        f = _fields(self.A, self.B)
        self.value = _m().ntuple_value(table, f["rows"], f["cur"], L, M, f["lines"], f["moves"], f["state"]).reshape(n, 40)
        with np.errstate(invalid="ignore", over="ignore"):
            self.Q = np.where(self.done1, r1, r1 + np.float32(gamma) * ply["score"].reshape(n, 40)).astype(np.float32)
        self.second = np.where(self.done1, 255, ply["action"].reshape(n, 40)).astype(np.uint8)
        self.A, self.B = self.A.reshape(n, 40, 4), self.B.reshape(n, 40, 4)
        masked = np.where(self.distinct, self.Q, -np.inf)
        self.greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)       # the lowest index at the maximum

    def want(self, action=None):
        at = np.arange(self.n)
        action = self.greedy if action is None else action
        return dict(action=action.astype(np.uint8), second=self.second[at, action], score=self.Q[at, self.greedy],
                    after_a=self.A[at, action], after_b=self.B[at, action], value=self.value[at, action])


@pytest.mark.parametrize("n", SIZES + [POOL])
def test_search_is_the_one_ply_rule_composed_at_both_epsilons(pool, table3, n):
    idx = pool.take(n, 0 if n == POOL else 13 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    c = Composed(A, B, table3, GAMMA)
    run = pool.running[idx]
    cur = (pool.fields["window"][idx] & np.uint64(7)).astype(np.int64)
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    order = np.argsort(~c.distinct, axis=1, kind="stable")    # the distinct placements first, ascending
    for epsilon in (0.0, 0.25):
        explores, j = _m().ntuple_explore(seed, step, n, epsilon, np.array(_m().PIECE_PLACEMENTS)[cur])
        explores &= run
        action = np.where(explores, order[np.arange(n), j], c.greedy)
        got = _policy3(2, A, B, table3, epsilon=epsilon, seed=seed, step=step)
        _same(got, c.want(action), (n, epsilon))
        assert (got["action"][~run] == 0).all() and (got["second"][~run] == 255).all() and (_bits(got["score"])[~run] == 0).all()
        assert np.array_equal(got["after_a"][~run], A[~run]) and np.array_equal(got["after_b"][~run], B[~run])
    if n == POOL:
        assert explores.sum() > 0.15 * run.sum() and (got["action"] != c.greedy).sum() > 0.1 * run.sum()
        ended = c.done1[np.arange(n), got["action"]] & run
        assert ended.sum() >= 20 and (got["second"][ended] == 255).all() and (_bits(got["value"])[ended] == 0).all()
        assert (got["second"][run & ~ended] != 255).all() and (got["value"][run & ~ended] != 0).all()
        one = _policy3(1, A, B, table3, gamma=GAMMA)
        assert (one["action"] != c.want()["action"]).sum() >= 100                                  # two plies play another game


# ------------------------------------------------------------------------------------------------ UPDATE and UPDATE_TRACE
def _errors(gen, n):
    """Errors of order 1; from seven boards on, a 0, a NaN and one value past the clamp on either side."""
    error = gen.normal(size=n).astype(np.float32)
    if n >= 7:
        error[gen.permutation(n)[:4]] = np.array([0.0, np.nan, 1e9, -1e9], np.float32)
    return error


def _ring_case(after, seed, n):
    gen = np.random.default_rng(seed)
    picks = _picks(gen, after, (SLOTS, n))
    if n == 1:                                                 # the one board runs at age 0, or the launch would add nothing
        picks[HEAD, 0] = np.flatnonzero(after["fields"]["state"] == 0)[313]
    A, B = _ring(after, picks)
    return gen, picks, A, B


def test_update_leaves_the_mirror_table_on_the_whole_set(after, mirror):
    gen = np.random.default_rng(65560)
    n, f = POOL * 40, after["fields"]
    error = gen.normal(size=n).astype(np.float32)
    for value in (np.nan, np.inf, -np.inf, 1e30, 0.0):
        error[gen.integers(0, n, 100)] = value
    start, rate = _full_range(1), 3000.0
    got = _trace3(after["A"], after["B"], 0, 1, start, error, rate, 0.0, 0, planes=True)
    # the mirror's adds, from the indices computed once for the set
    index, used = mirror["after"]["index"], mirror["after"]["used"]
    d = np.where(f["state"] == 0, _m().ntuple_steps(error, rate), 0)
    live = used & (d != 0)[:, None]
    want = start.copy()
    np.add.at(want.view(np.uint32), index[live], np.broadcast_to(d[:, None], live.shape)[live].astype(np.uint32))
    assert np.array_equal(got, want)
    changed = got != start
    assert changed.sum() > 20000 and changed[COUNTER_BASE:].sum() > 50
    assert not changed[:COUNTER_BASE][np.arange(COUNTER_BASE) % PATTERNS == 0].any()   # the all-empty pattern is never updated
    assert (np.abs(d) == 1 << 24).sum() >= 100 and (np.isnan(error) & (f["state"] == 0)).sum() >= 20


@pytest.mark.parametrize("n", SIZES)
def test_update_at_sizes_around_the_block_edges(after, n):
    gen, picks, A, B = _ring_case(after, n, n)
    error, start = _errors(gen, n), _full_range(n)
    f = after["fields"]
    got = _trace3(A[HEAD], B[HEAD], 0, 1, start, error, 1234.5, 0.0, 0, planes=True)
    rows, cur, lines, moves, state = _age(f, picks[HEAD])
    want = _m().ntuple_update(start.copy(), rows, cur, L, M, lines, moves, state, error, 1234.5)
    assert np.array_equal(got, want) and (got != start).any()


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("horizon", [1, 4, 16])
@pytest.mark.parametrize("n", SIZES + [POOL])
def test_update_trace_leaves_the_mirror_table(after, n, horizon, symmetric):
    f = after["fields"]
    gen, picks, A, B = _ring_case(after, 1000 * horizon + n, n)
    rate, decay = 3000.0, 0.7
    error, start = _errors(gen, n), _full_range(horizon + n)
    ages = [_age(f, picks[(HEAD - k) % SLOTS]) for k in range(horizon)]
    assert horizon < 4 or (HEAD - (horizon - 1)) % SLOTS > HEAD                                   # the older ages wrap past slot 0
    got = _trace3(A, B, HEAD, horizon, start, error, rate, decay, symmetric)
    want = _m().ntuple_update_trace(start.copy(), ages, L, M, error, rate, decay, bool(symmetric))
    assert np.array_equal(got, want) and (got != start).any()
    assert not (got != start)[:COUNTER_BASE][np.arange(COUNTER_BASE) % PATTERNS == 0].any()
    if n < 257:
        return
    # from the zero table: a symmetric update leaves a symmetric table, the other one does not
    zero = np.zeros(ENTRIES, np.int32)
    left = _trace3(A, B, HEAD, horizon, zero, error, rate, decay, symmetric)
    assert np.array_equal(left, _m().ntuple_update_trace(zero.copy(), ages, L, M, error, rate, decay, bool(symmetric)))
    assert T.ntuple_is_symmetric(torch.from_numpy(left).to(DEV)) == bool(symmetric)
    if horizon > 1:                                            # boards stop at an older age, and boards run through all of them
        running = np.stack([f["state"][picks[(HEAD - k) % SLOTS]] == 0 for k in range(horizon)])
        stop = np.where(running.all(axis=0), horizon, np.argmin(running, axis=0))
        assert (stop == horizon).any() and ((stop > 0) & (stop < horizon)).any() and (stop == 0).any()


# ------------------------------------------------------------------------------------------------ UPDATE_COHERENT
@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("n", SIZES + [POOL])
def test_update_coherent_leaves_the_mirror_table_and_coherence(after, n, symmetric):
    f = after["fields"]
    horizon, rate, decay = 4, 3000.0, 0.7
    gen, picks, A, B = _ring_case(after, 77 + n, n)
    error, start = _errors(gen, n), _full_range(n + 3)
    ages = [_age(f, picks[(HEAD - k) % SLOTS]) for k in range(horizon)]
    zero = np.zeros((ENTRIES, 2), np.int64)
    # from a zero buffer: the trace update's table, and the first sums
    table1, sums1 = _trace3(A, B, HEAD, horizon, start, error, rate, decay, symmetric, coherence=zero)
    want_table, want_sums = _m().ntuple_update_coherent(start.copy(), zero.copy(), ages, L, M, error, rate, decay, bool(symmetric))
    assert np.array_equal(table1, want_table) and np.array_equal(sums1, want_sums)
    assert np.array_equal(table1, _m().ntuple_update_trace(start.copy(), ages, L, M, error, rate, decay, bool(symmetric)))
    assert (sums1[:, 1] > 0).any()
    # from a filled buffer, with other errors: step sizes below 1 come in
    filled = sums1.copy()
    filled[::3, 0] //= 3                                       # |E| below A on a third of the entries, whatever the errors do
    other = _errors(gen, n)
    table2, sums2 = _trace3(A, B, HEAD, horizon, table1, other, rate, decay, symmetric, coherence=filled)
    want_table, want_sums = _m().ntuple_update_coherent(table1.copy(), filled.copy(), ages, L, M, other, rate, decay, bool(symmetric))
    assert np.array_equal(table2, want_table) and np.array_equal(sums2, want_sums)
    if n >= 257:
        plain = _m().ntuple_update_trace(table1.copy(), ages, L, M, other, rate, decay, bool(symmetric))
        assert not np.array_equal(table2, plain)               # the step sizes did something
    # the boards in another order: the same bytes
    order = gen.permutation(n)
    table3_, sums3 = _trace3(np.ascontiguousarray(A[:, order]), np.ascontiguousarray(B[:, order]), HEAD, horizon, table1,
                             np.ascontiguousarray(other[order]), rate, decay, symmetric, coherence=filled)
    assert np.array_equal(table3_, table2) and np.array_equal(sums3, sums2)


# ------------------------------------------------------------------------------------------------ SHAPE 0 through the new entries
def test_every_shaped_entry_at_shape_0_writes_the_bytes_of_its_twin(pool, after):
    n = 257
    idx = pool.take(n, 500)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    table = _table(9, entries=ENTRIES_2X4)
    assert np.array_equal(_bits(_value3(A, B, table, shape=0)), _bits(_value(A, B, table)))
    kw = dict(epsilon=0.25, seed=11, step=5)
    one, twin = _policy3(1, A, B, table, shape=0, **kw), _act(A, B, table, **kw)
    for k, v in twin.items():
        assert np.array_equal(one[k].view(np.uint8), v.view(np.uint8)), k
    two, twin = _policy3(2, A, B, table, shape=0, **kw), _search(A, B, table, **kw)
    for k, v in twin.items():
        assert np.array_equal(two[k].view(np.uint8), v.view(np.uint8)), k
    gen, picks, RA, RB = _ring_case(after, 5, n)
    error, start = _errors(gen, n), _full_range(4, ENTRIES_2X4)
    assert np.array_equal(_trace3(RA[HEAD], RB[HEAD], 0, 1, start, error, 3000.0, 0.0, 0, shape=0, planes=True),
                          _update(RA[HEAD], RB[HEAD], start, error, 3000.0))
    for symmetric in (0, 1):
        want = _trace(RA, RB, HEAD, 4, start, error, 3000.0, 0.7, symmetric)
        assert np.array_equal(_trace3(RA, RB, HEAD, 4, start, error, 3000.0, 0.7, symmetric, shape=0), want) and (want != start).any()
        # the coherent twin, through its own entry
        filled = np.random.default_rng(6).integers(0, 1 << 20, (ENTRIES_2X4, 2)).astype(np.int64)
        a, b, t, e, c = _framed(RA, 1), _framed(RB, 2), _framed(start, 3), _framed(error, 4), _framed(filled, 5)
        _check(_lib().tpl_ntuple_update_coherent(a.ptr(), b.ptr(), n, SLOTS, HEAD, 4, L, M, t.ptr(), c.ptr(), e.ptr(), 3000.0, 0.7,
                                                 symmetric, _stream()))
        got_table, got_sums = _trace3(RA, RB, HEAD, 4, start, error, 3000.0, 0.7, symmetric, shape=0, coherence=filled)
        assert np.array_equal(got_table, t.host().view(np.int32)) and np.array_equal(got_sums.reshape(-1), c.host().view(np.int64))
        assert (got_table != start).any()


# ------------------------------------------------------------------------------------------------ LEARNER
def _two_piece_env(n):
    carved = T.generate_configs(2, 2, 64, seed=107)
    return T.BatchedTetris(2, 2, n, device=DEV, seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)


def test_a_3x3_learner_is_deterministic_and_gains_half_of_what_the_2x4_learner_gains():
    """The two-piece game of test_ntuple_gpu (L = 2, M = 2, 64 carved configurations, reward (0, 1, 0), 4,096 boards, gamma 1,
    epsilon 0.25, rate 8, 300 training steps, 16 evaluation steps).  The yardstick is the 2 x 4 learner of the same run: the 3 x 3
    win count must exceed the zero table's by at least half of the margin by which the 2 x 4 learner's does."""
    TRAIN, EVAL, n = 300, 16, 4096

    def run(shape):
        env = _two_piece_env(n)
        learner = T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.25, seed=5, shape=shape)
        assert learner.shape == shape and T.ntuple_shape(learner.table) == shape and learner.policy.shape == shape
        before = learner.evaluate(EVAL)
        assert int(learner.table.abs().sum()) == 0
        assert learner.train(TRAIN) == TRAIN
        result = before, learner.evaluate(EVAL), learner.table.clone()
        env.terminate()
        return result

    zero, narrow, _ = run("2x4")
    zero3, wide, table = run("3x3")
    print(f"wins of {zero['episodes']} episodes: zero table {zero['wins']}, 2x4 {narrow['wins']} of {narrow['episodes']}, "
          f"3x3 {wide['wins']} of {wide['episodes']}; 3x3 entries in use {int((table != 0).sum())}, largest {int(table.abs().max())}")
    assert zero3 == zero                                       # the zero table plays the same game in either shape
    assert tuple(table.shape) == (ENTRIES,) and narrow["wins"] > zero["wins"]
    assert wide["wins"] - zero["wins"] >= (narrow["wins"] - zero["wins"]) / 2
    _, again, table2 = run("3x3")
    assert again == wide and torch.equal(table, table2)        # the same seed, the same bytes


def test_depth_two_and_the_coherent_symmetric_form_run_on_a_3x3_learner():
    n = 4096
    env = _two_piece_env(n)
    learner = T.NTupleLearner(env, gamma=1.0, rate=2.0, epsilon=0.25, seed=5, coherent=True, symmetric=True, lam=0.8, horizon=4,
                              shape="3x3")
    assert tuple(learner.coherence.shape) == (ENTRIES, 2) and tuple(learner.table.shape) == (ENTRIES,)
    learner.train(60)
    assert int((learner.table != 0).sum()) > 0 and T.ntuple_is_symmetric(learner.table)
    sums = learner.coherence
    sigma = torch.from_numpy(_m().ntuple_mirror_permutation("3x3")).to(DEV)
    assert torch.equal(sums[sigma], sums) and int((sums[:, 1] > 0).sum()) > 0
    alpha = T.ntuple_step_sizes(sums)
    assert tuple(alpha.shape) == (ENTRIES,) and float(alpha.min()) >= 0.0 and float(alpha.max()) == 1.0
    one, two = learner.evaluate(16), learner.evaluate(16, depth=2)
    print(f"3x3 coherent symmetric: depth 1 {one}, depth 2 {two}")
    assert one["episodes"] > 0 and two["episodes"] > 0 and T.ntuple_is_symmetric(learner.table)
    # a coherence buffer of the other shape is refused before anything is launched
    learner.coherence = T.ntuple_coherence(DEV)
    with pytest.raises(ValueError, match="coherence"):
        learner.train(1)
    with pytest.raises(ValueError, match="shape"):
        T.NTupleLearner(env, shape="4x4")
    # a 3 x 3 table under a policy, and the value of the resident boards, by the table's shape
    policy = T.NTuplePolicy(env, learner.table, gamma=1.0, depth=2)
    assert policy.shape == "3x3" and tuple(policy.act().shape) == (n,)
    assert tuple(T.ntuple_value(env, learner.table).shape) == (n,)
    with pytest.raises(ValueError, match="table"):
        T.NTuplePolicy(env, torch.zeros(ENTRIES + 8, dtype=torch.int32, device=DEV))
    env.terminate()
