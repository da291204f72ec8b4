"""Two table shapes summed in one n-tuple value on one MI355X (include/tpl_learn.h's "Two shapes summed"; ntuple_sum_value_kernel,
ntuple_sum_act_kernel, ntuple_sum_search_kernel in csrc/learn/ntuple.hip, ntuple_beam_sum_kernel in csrc/learn/ntuple_beam.hip;
ntuple.py).  The state set is test_ntuple_shape_gpu's: the 1,639 states of the afterstate pool (L = 10, M = 40) and their 65,560
afterstates; sizes n = 1, 7, 9, 257 -- no multiple of an act block's 8 boards nor of 256 -- and the whole set.  Floats are compared as
bits, and canaries frame every buffer the kernels are handed.

  * VALUE: tpl_ntuple_value_sum is the numpy mirror bit for bit under full-range int32 tables, whose sums are 37 bits wide; finished
    states give +0; on more than a tenth of the running states float32(S_2x4 + S_3x3) is not float32(S_2x4) + float32(S_3x3);
  * REDUCTION: with one part zero, value_sum, act_sum (epsilon 0 and 1), search_sum and beam_sum write the bytes of the other part's
    entries run on that part alone; with both parts random they differ from both;
  * ACT is the mirror's arg-max -- tpl_afterstates' rewards, the mirror's V, the numpy choice rule -- at epsilon 0 and 1; SEARCH is the
    one-ply rule composed, as test_ntuple_shape_gpu composes it;
  * BEAM: D = 1 is act_sum at epsilon 0, D = 2 at W >= 34 gives search_sum's action and score, (3, 8) and (11, 64) are
    test_ntuple_beam_gpu's reference composed ply by ply, and the plan played move by move reaches the score;
  * LEARNER: every form of one train step leaves the mirror's bytes in table and coherence; one seed, the same bytes; on the
    two-piece game the sum learner gains at least half of what the 2 x 4 learner gains over the zero table in the same run.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, _resident
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_beam_gpu import compose
from test_ntuple_gpu import GAMMA, PARAMS, _fields, _framed, after, pool  # noqa: F401  (fixtures)
from test_ntuple_trace_gpu import _age, _carved_env, _two_piece_env

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SUM = "2x4+3x3"
E2, E3, ES = 314368, 590848, 905216
SIZES = [1, 7, 9, 257]                                         # no multiple of an act block's 8 boards nor of 256
ARANGE = np.arange(40)
PARTS = {0: slice(0, E2), 1: slice(E2, ES)}                    # the C shape of a part -> where it lies in a sum table


def _m():
    return T._learn_lib


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _random(seed, span=1 << 20, entries=ES):
    return np.random.default_rng(seed).integers(-span, span + 1, entries).astype(np.int32)


def _only(table, shape):
    """`table` with the part of the OTHER shape zeroed."""
    out = np.zeros_like(table)
    out[PARTS[shape]] = table[PARTS[shape]]
    return out


# ------------------------------------------------------------------------------------------------ the entries, framed
# form: "sum" -- the _sum entry on a sum table -- or a C shape id, 0 or 1: the _shaped entry (tpl_ntuple_beam) on a table of that shape
def _tail(form):
    return () if form == "sum" else (form,)


def _value(A, B, table, form="sum", L=L, M=M):
    n = A.shape[0]
    a, b, t, v = _framed(A, 1), _framed(B, 2), _framed(table, 3), Framed(4 * n, 4)
    v.inner().fill_(0xCD)
    entry = _lib().tpl_ntuple_value_sum if form == "sum" else _lib().tpl_ntuple_value_shaped
    _check(entry(a.ptr(), b.ptr(), n, L, M, t.ptr(), v.ptr(), *_tail(form), _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("value", v)):
        f.assert_canary((n, form, k))
    assert np.array_equal(t.host().view(np.int32), table) and np.array_equal(a.host(), A.view(np.uint8).reshape(-1))
    return v.host().view(np.float32).copy()


def _policy(depth, A, B, table, form="sum", gamma=GAMMA, epsilon=0.0, seed=0, step=0, L=L, M=M):
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, second=1, score=4, after_a=16, after_b=16, value=4)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    head = (a.ptr(), b.ptr(), n, L, M, *PARAMS, gamma, t.ptr(), epsilon, seed, step, p("action"))
    tail = (p("score"), p("after_a"), p("after_b"), p("value"), *_tail(form), _stream())
    name = ("tpl_ntuple_search" if depth == 2 else "tpl_ntuple_act") + ("_sum" if form == "sum" else "_shaped")
    _check(getattr(_lib(), name)(*head, p("second"), *tail) if depth == 2 else getattr(_lib(), name)(*head, *tail))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((depth, n, form, epsilon, k))
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


def _beam(A, B, table, depth, width, form="sum", gamma=GAMMA, L=L, M=M):
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, plan=depth, score=4, after_a=16, after_b=16)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    entry = _lib().tpl_ntuple_beam_sum if form == "sum" else _lib().tpl_ntuple_beam
    _check(entry(a.ptr(), b.ptr(), n, L, M, *PARAMS, gamma, t.ptr(), depth, width, p("action"), p("plan"), p("score"), p("after_a"),
                 p("after_b"), *_tail(form), _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((n, depth, width, form, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(t.host().view(np.int32), table)
    host = {k: f.host().copy() for k, f in out.items()}
    for k in ("after_a", "after_b"):
        host[k] = host[k].view(np.uint32).reshape(n, 4)
    host["plan"], host["score"] = host["plan"].reshape(n, depth), host["score"].view(np.float32)
    return host


def _same(got, want, what, keys=None):
    """Every output of `want` (or `keys` of them), byte for byte."""
    for k in (want if keys is None else keys):
        if len(got[k]) == 0 and len(want[k]) == 0:
            continue
        g, w = np.ascontiguousarray(got[k]).view(np.uint8).reshape(len(got[k]), -1), np.ascontiguousarray(want[k]).view(np.uint8).reshape(len(want[k]), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (what, k, bad.size, bad[:5].tolist(), got[k][bad[:5]].tolist(), want[k][bad[:5]].tolist())


def _differs(got, want, key):
    return not np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8))


# ------------------------------------------------------------------------------------------------ the mirror, once
@pytest.fixture(scope="module")
def mirror(pool, after):
    """The sum indices of the whole set, once: the pool's states and their afterstates."""
    out = {}
    for name, f in (("pool", _fields(pool.A, pool.B)), ("after", after["fields"])):
        index, used = _m().ntuple_indices(f["rows"], f["cur"], L, M, f["lines"], f["moves"], shape=SUM)
        out[name] = dict(fields=f, index=index, used=used)
    return out


def _part_sums(table, part):
    """(S_2x4, S_3x3) of every state, int64: the columns of each part of the sum indices."""
    entries = np.where(part["used"], table[part["index"]].astype(np.int64), 0)
    return entries[:, :154].sum(axis=1), entries[:, 154:].sum(axis=1)


def _mirror_value(table, part, idx=None):
    pick = (lambda v: v) if idx is None else (lambda v: v[idx])
    sa, sb = _part_sums(table, dict(index=pick(part["index"]), used=pick(part["used"])))
    state = pick(part["fields"]["state"])
    return np.where(state == 0, (sa + sb).astype(np.float32) * np.float32(2.0 ** -16), np.float32(0.0)).astype(np.float32)


@pytest.fixture(scope="module")
def ply(pool):
    """tpl_afterstates on the pool, once: the 40 afterstates of every state with their rewards, done flags and canonical actions,
    and the sum indices of the afterstates -- what the one-ply rule is put together from."""
    n = POOL
    a, b = _framed(pool.A, 1), _framed(pool.B, 2)
    out_a, out_b = Framed(n * 640, 3), Framed(n * 640, 4)
    reward, done, canonical = Framed(n * 160, 5), Framed(n * 40, 6), Framed(n * 40, 7)
    _check(_lib().tpl_afterstates(a.ptr(), b.ptr(), n, L, M, *PARAMS, out_a.ptr(), out_b.ptr(), reward.ptr(), done.ptr(), None,
                                  canonical.ptr(), _stream()))
    A, B = out_a.host().view(np.uint32).reshape(-1, 4).copy(), out_b.host().view(np.uint32).reshape(-1, 4).copy()
    f = _fields(A, B)
    index, used = _m().ntuple_indices(f["rows"], f["cur"], L, M, f["lines"], f["moves"], shape=SUM)
    return dict(A=A.reshape(n, 40, 4), B=B.reshape(n, 40, 4), reward=reward.host().view(np.float32).reshape(n, 40).copy(),
                done=done.host().reshape(n, 40) != 0, distinct=canonical.host().reshape(n, 40) == ARANGE[None, :],
                part=dict(fields=f, index=index, used=used))


def _choice(pool, ply, table, idx, gamma=GAMMA, epsilon=0.0, seed=0, step=0):
    """The rule of tpl_ntuple_act for the states `idx` as boards 0 .. n - 1 under a sum table: tpl_afterstates' rewards, the mirror's
    V of the afterstates, the lowest placement at the maximum, and the exploration draw."""
    n, at = idx.size, np.arange(idx.size)
    rows = (idx[:, None] * 40 + ARANGE[None, :]).reshape(-1)
    v = _mirror_value(table, ply["part"], rows).reshape(n, 40)
    done, run, distinct = ply["done"][idx], pool.running[idx], ply["distinct"][idx]
    score = np.where(done, ply["reward"][idx], ply["reward"][idx] + np.float32(gamma) * v).astype(np.float32)
    score = np.where(run[:, None], score, np.float32(0.0))
    masked = np.where(distinct, score, -np.inf)
    greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)
    cur = (pool.fields["window"][idx] & np.uint64(7)).astype(np.int64)
    explores, j = _m().ntuple_explore(seed, step, n, epsilon, np.array(_m().PIECE_PLACEMENTS)[cur])
    explores &= run
    order = np.argsort(~distinct, axis=1, kind="stable")
    action = np.where(explores, order[at, j], np.where(run, greedy, 0))
    value = np.where(done[at, action] | ~run, np.float32(0.0), v[at, action]).astype(np.float32)
    after_a = np.where(run[:, None], ply["A"][idx][at, action], pool.A[idx])
    after_b = np.where(run[:, None], ply["B"][idx][at, action], pool.B[idx])
    return dict(action=action.astype(np.uint8), score=score[at, greedy], after_a=after_a, after_b=after_b, value=value), explores


# ------------------------------------------------------------------------------------------------ VALUE
def test_value_sum_is_the_mirror_bit_for_bit_on_the_whole_set(pool, after, mirror):
    table = _random(299, span=(1 << 31) - 1)                   # the whole int32 range: sums of 37 bits, rounded at the conversion
    for name, (A, B) in (("pool", (pool.A, pool.B)), ("after", (after["A"], after["B"]))):
        got, want = _value(A, B, table), _mirror_value(table, mirror[name])
        assert np.array_equal(_bits(got), _bits(want)), name
        done = mirror[name]["fields"]["state"] != 0
        assert (_bits(got)[done] == 0).all() and (got[~done] != 0).all() and done.sum() > 100          # +0, not -0
        # where the rounding happens matters on this set: each part rounded first is another number
        sa, sb = _part_sums(table, mirror[name])
        twice = (sa.astype(np.float32) + sb.astype(np.float32)) * np.float32(2.0 ** -16)
        differ = (_bits(twice) != _bits(want)) & ~done
        print(f"{name}: float32(Sa + Sb) != float32(Sa) + float32(Sb) on {differ.sum()} of {(~done).sum()} running states")
        assert differ.sum() >= (~done).sum() / 10 and np.abs(sa + sb).max() > 1 << 33
        assert not np.array_equal(_bits(got)[differ], _bits(twice)[differ])


@pytest.mark.parametrize("n", SIZES)
def test_value_sum_at_sizes_around_the_block_edges(after, mirror, n):
    table = _random(n, span=(1 << 31) - 1)
    idx = (np.arange(n) * 40 + 977 * n) % (POOL * 40)
    if n == 1:
        idx = np.flatnonzero(after["fields"]["state"] == 0)[977:978]
    A, B = np.ascontiguousarray(after["A"][idx]), np.ascontiguousarray(after["B"][idx])
    got = _value(A, B, table)
    assert np.array_equal(_bits(got), _bits(_mirror_value(table, mirror["after"], idx))) and (got != 0).any()


# ------------------------------------------------------------------------------------------------ REDUCTION to the twins
@pytest.mark.parametrize("n", SIZES)
def test_with_one_part_zero_every_sum_entry_writes_the_bytes_of_the_other_parts_entry(pool, after, n):
    idx = pool.take(n, 13 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    pick = (np.arange(n) * 40 + 977 * n) % (POOL * 40)
    VA, VB = np.ascontiguousarray(after["A"][pick]), np.ascontiguousarray(after["B"][pick])
    table = _random(1000 + n)
    kw = dict(seed=0xDEADBEEFCAFEF00D, step=(1 << 40) + 3)
    calls = {"value": lambda t, form: dict(value=_value(VA, VB, t, form)),
             "act 0": lambda t, form: _policy(1, A, B, t, form, epsilon=0.0, **kw),
             "act 1": lambda t, form: _policy(1, A, B, t, form, epsilon=1.0, **kw),
             "search 0": lambda t, form: _policy(2, A, B, t, form, epsilon=0.0, **kw),
             "search 1": lambda t, form: _policy(2, A, B, t, form, epsilon=1.0, **kw),
             "beam 3 x 8": lambda t, form: _beam(A, B, t, 3, 8, form)}
    for what, call in calls.items():
        both = call(table, "sum")
        for shape in (0, 1):
            twin = call(np.ascontiguousarray(table[PARTS[shape]]), shape)
            _same(call(_only(table, shape), "sum"), twin, (what, shape, n))        # action, score, after, value, second, plan
            if n == 257:                                       # both parts random: another value, another game
                key = "value" if what == "value" else "score"
                assert _differs(both, twin, key), (what, shape)
                if what != "value" and not what.endswith(" 1"):
                    assert _differs(both, twin, "action"), (what, shape)


# ------------------------------------------------------------------------------------------------ ACT and SEARCH
@pytest.fixture(scope="module")
def table_sum():
    return _random(40)


@pytest.mark.parametrize("n", SIZES + [POOL])
def test_act_sum_is_the_mirror_arg_max_at_both_epsilons(pool, ply, table_sum, n):
    idx = pool.take(n, 0 if n == POOL else 13 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    for epsilon in (0.0, 1.0):
        want, explores = _choice(pool, ply, table_sum, idx, epsilon=epsilon, seed=seed, step=step)
        got = _policy(1, A, B, table_sum, epsilon=epsilon, seed=seed, step=step)
        _same(got, want, (n, epsilon))
        assert (explores == pool.running[idx]).all() if epsilon == 1.0 else not explores.any()
    if n == POOL:
        run = pool.running
        greedy, _ = _choice(pool, ply, table_sum, idx)
        assert (got["action"] != greedy["action"]).sum() > 0.5 * run.sum() and len(set(greedy["action"][run].tolist())) > 20
        assert (got["action"][~run] == 0).all() and (_bits(got["score"])[~run] == 0).all() and (_bits(got["value"])[~run] == 0).all()
        assert np.array_equal(got["after_a"][~run], pool.A[~run]) and np.array_equal(got["after_b"][~run], pool.B[~run])
        ended = ply["done"][np.arange(n), greedy["action"]] & run
        assert ended.sum() >= 20 and (greedy["value"][ended] == 0).all()


class Composed:
    """tpl_ntuple_search's rule put together as test_ntuple_shape_gpu.Composed does, from one-ply pieces over the 40 n afterstates of
    tpl_afterstates: Q(a) = r1 + gamma * score'(s_a) and second(a) = action'(s_a), (score', action') the one-ply sum policy on the
    afterstate -- held to the numpy rule by the act test above --, V(s_a) from the numpy mirror."""

    def __init__(self, ply, idx, table, gamma):
        n = self.n = idx.size
        self.A, self.B = ply["A"][idx], ply["B"][idx]
        r1, self.done1, self.distinct = ply["reward"][idx], ply["done"][idx], ply["distinct"][idx]
        one = _policy(1, np.ascontiguousarray(self.A.reshape(-1, 4)), np.ascontiguousarray(self.B.reshape(-1, 4)), table, gamma=gamma)
        rows = (idx[:, None] * 40 + ARANGE[None, :]).reshape(-1)
        self.value = _mirror_value(table, ply["part"], rows).reshape(n, 40)
        with np.errstate(invalid="ignore", over="ignore"):
            self.Q = np.where(self.done1, r1, r1 + np.float32(gamma) * one["score"].reshape(n, 40)).astype(np.float32)
        self.second = np.where(self.done1, 255, one["action"].reshape(n, 40)).astype(np.uint8)
        masked = np.where(self.distinct, self.Q, -np.inf)
        self.greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)

    def want(self, action=None):
        at = np.arange(self.n)
        action = self.greedy if action is None else action
        return dict(action=action.astype(np.uint8), second=self.second[at, action], score=self.Q[at, self.greedy],
                    after_a=self.A[at, action], after_b=self.B[at, action], value=self.value[at, action])


@pytest.mark.parametrize("n", SIZES)
def test_search_sum_is_the_one_ply_rule_composed_at_both_epsilons(pool, ply, table_sum, n):
    idx = pool.take(n, 13 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    c = Composed(ply, idx, table_sum, GAMMA)
    run = pool.running[idx]
    cur = (pool.fields["window"][idx] & np.uint64(7)).astype(np.int64)
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    order = np.argsort(~c.distinct, axis=1, kind="stable")
    for epsilon in (0.0, 0.25):
        explores, j = _m().ntuple_explore(seed, step, n, epsilon, np.array(_m().PIECE_PLACEMENTS)[cur])
        explores &= run
        action = np.where(explores, order[np.arange(n), j], c.greedy)
        got = _policy(2, A, B, table_sum, epsilon=epsilon, seed=seed, step=step)
        want = c.want(action)
        _same({k: v[run] for k, v in got.items()}, {k: v[run] for k, v in want.items()}, (n, epsilon))
        assert (got["action"][~run] == 0).all() and (got["second"][~run] == 255).all() and (_bits(got["score"])[~run] == 0).all()
        assert np.array_equal(got["after_a"][~run], A[~run]) and np.array_equal(got["after_b"][~run], B[~run])
    if n == 257:
        assert explores.sum() > 0.15 * run.sum()
        one = _policy(1, A, B, table_sum)
        assert (one["action"] != c.want()["action"]).sum() >= 20                                   # two plies play another game


# ------------------------------------------------------------------------------------------------ BEAM
@pytest.mark.parametrize("n", SIZES)
def test_beam_sum_at_depth_one_is_act_sum_and_at_depth_two_and_full_width_search_sum(pool, table_sum, n):
    idx = pool.take(n, 7 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    run = pool.running[idx]
    one = _policy(1, A, B, table_sum)
    for width in (1, 5, 64):
        got = _beam(A, B, table_sum, 1, width)
        _same(got, one, (n, 1, width), keys=("action", "score", "after_a", "after_b"))
        assert (got["plan"][:, 0] == np.where(run, one["action"], 255)).all()
    two = _policy(2, A, B, table_sum)
    for width in (34, 64):
        got = _beam(A, B, table_sum, 2, width)
        _same(got, two, (n, 2, width), keys=("action", "score", "after_a", "after_b"))
        assert (got["plan"][:, 1] <= two["second"]).all() and ((got["plan"][:, 1] == 255) == (two["second"] == 255)).all()
    assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all() and (_bits(got["score"][~run]) == 0).all()


@pytest.fixture(scope="module")
def env10():
    """Any L = 10 / M = 40 environment with the reward parameters: T.afterstates reads L, M and the rewards from it."""
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=9, reward=PARAMS)
    yield env
    env.terminate()


def _plies(pool, idx, depth):
    """The effective depth of every state: 0 where it is finished, else min(depth, 11 - moves mod 10)."""
    moves = _fields(pool.A[idx], pool.B[idx])["moves"]
    return np.where(pool.running[idx], np.minimum(depth, 11 - moves % 10), 0)


@pytest.mark.parametrize("depth,width", [(3, 8), (11, 64)])
def test_beam_sum_is_the_reference_composed_ply_by_ply(pool, env10, table_sum, depth, width):
    """test_ntuple_beam_gpu.compose: every ply T.afterstates, V of the children from T.ntuple_value -- tpl_ntuple_value_sum, held to
    the mirror above --, the numpy fold and ntuple_beam_ply."""
    n = 257
    idx = np.arange(n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    plies = _plies(pool, idx, depth)
    want = compose(env10, table_sum, A, B, plies, depth, width)
    got = _beam(A, B, table_sum, depth, width)
    _same(got, want, (depth, width), keys=("action", "plan", "score"))
    run = pool.running[idx]
    assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all()
    assert (got["plan"][run, 0] == got["action"][run]).all() and ((got["plan"] != 255).sum(axis=1) <= plies).all()
    assert (plies == depth).sum() >= 10 and (~run).sum() >= 10


def test_playing_the_plan_of_beam_sum_reaches_the_score(pool, table_sum):
    m, depth, width = _m(), 11, 8
    env, idx = _resident(pool, POOL, 0, PARAMS)
    table = torch.from_numpy(table_sum).to(DEV)
    policy = T.NTupleBeamPolicy(env, table, depth, width, gamma=GAMMA)
    assert policy.shape == SUM
    score = torch.empty(POOL, dtype=torch.float32, device=DEV)
    plan = torch.full((POOL, depth), 77, dtype=torch.uint8, device=DEV)
    action = policy.act(score=score, plan=plan)
    plan, score = _np(plan), _np(score)
    assert np.array_equal(_np(action), np.where(pool.running, plan[:, 0], 0))
    plies, length = _plies(pool, idx, depth), (plan != 255).sum(axis=1)
    assert (length <= plies).all() and (length[pool.running] >= 1).all()
    earned = np.zeros((POOL, depth), np.float32)
    final_v, final_state = np.zeros(POOL, np.float32), ((pool.B[:, 1] >> np.uint32(28)) & np.uint32(3)).astype(np.int64)
    for j in range(depth):
        step = np.where(plan[:, j] == 255, 0, plan[:, j]).astype(np.uint8)
        _, reward, _, _ = env.step(torch.from_numpy(step).to(DEV), observe=False)
        earned[:, j] = _np(reward)
        at = length == j + 1                                   # these boards have played their plan
        pa, pb = env.raw_planes()
        final_v[at] = _np(T.ntuple_value((pa, pb), table, L, M))[at]
        final_state[at] = ((_np(pb).view(np.uint32)[:, 1] >> np.uint32(28)) & np.uint32(3))[at]
    env.terminate()
    want = np.zeros(POOL, np.float32)
    for k in range(1, depth + 1):
        at = length == k
        if at.any():
            want[at] = m.ntuple_beam_values(earned[at, :k], final_state[at] != 0, final_v[at], GAMMA)
    bad = np.flatnonzero(_bits(want) != _bits(score))
    assert bad.size == 0, (bad[:5].tolist(), want[bad[:5]].tolist(), score[bad[:5]].tolist())
    assert ((length == plies) | (final_state != 0)).all() and (length == plies).sum() >= 100


# ------------------------------------------------------------------------------------------------ LEARNER
FORMS = {"plain": dict(), "trace 4 symmetric": dict(lam=0.8, horizon=4, symmetric=True),
         "coherent symmetric": dict(lam=0.8, horizon=4, symmetric=True, coherent=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_a_train_step_of_every_form_leaves_the_mirror_bytes(form):
    n, steps = 64, 12
    kw = dict(gamma=1.0, rate=16.0, epsilon=0.25, seed=5, shape=SUM, **FORMS[form])
    horizon, symmetric, coherent = kw.get("horizon", 1), kw.get("symmetric", False), kw.get("coherent", False)
    decay = np.float32(kw.get("lam", 0.0))

    def run(check):
        env = _carved_env(n)
        env.reset()
        learner = T.NTupleLearner(env, **kw)
        assert learner.shape == SUM and tuple(learner.table.shape) == (ES,) and learner.policy.shape == SUM
        assert (learner.coherence is None) != coherent and (not coherent or tuple(learner.coherence.shape) == (ES, 2))
        table, sums = np.zeros(ES, np.int32), np.zeros((ES, 2), np.int64)
        for step in range(steps):
            learner.train(1)
            if not check:
                continue
            head = (learner._head - 1) % learner.slots         # the head the update was made with
            ring = [_np(r).view(np.uint32) for r in learner._ring]
            ages = [_age(_fields(ring[0][(head - k) % learner.slots], ring[1][(head - k) % learner.slots])) for k in range(horizon)]
            if coherent:
                _m().ntuple_update_coherent(table, sums, ages, env.L, env.M, _np(learner._error), 16.0, decay, symmetric)
                assert np.array_equal(_np(learner.coherence), sums), step
            else:
                _m().ntuple_update_trace(table, ages, env.L, env.M, _np(learner._error), 16.0, decay, symmetric)
            assert np.array_equal(_np(learner.table), table), step
        if check:
            assert np.count_nonzero(table[:E2]) > 100 and np.count_nonzero(table[E2:]) > 100       # both parts learn
            assert np.count_nonzero(table[313344:E2]) > 0 and np.count_nonzero(table[E2 + 589824:]) > 0   # and both counters
            assert T.ntuple_is_symmetric(learner.table) is symmetric
            parts = T.ntuple_parts(learner.table)
            assert [T.ntuple_is_symmetric(p) for p in parts] == [symmetric, symmetric] and parts[1].data_ptr() == learner.table.data_ptr() + 4 * E2
            if coherent:
                assert np.count_nonzero(sums[:E2, 1]) > 100 and np.count_nonzero(sums[E2:, 1]) > 100
                alpha = T.ntuple_step_sizes(learner.coherence)
                assert np.array_equal(_bits(_np(alpha)), _bits(_m().ntuple_step_sizes(sums)))
        out = learner.table.clone(), (learner.coherence.clone() if coherent else None)
        if check and coherent:                                 # a coherence buffer of another size is refused before any launch
            before = learner.table.clone()
            for other in ("2x4", "3x3"):
                learner.coherence = T.ntuple_coherence(DEV, other)
                with pytest.raises(ValueError, match="coherence"):
                    learner.train(1)
            assert torch.equal(learner.table, before)
        env.terminate()
        return out

    checked, again = run(True), run(False)
    assert torch.equal(checked[0], again[0]) and (not coherent or torch.equal(checked[1], again[1]))   # one seed: the same bytes


def test_a_sum_learner_is_deterministic_and_gains_half_of_what_the_2x4_learner_gains():
    """The two-piece game of test_ntuple_gpu (L = 2, M = 2, 64 carved configurations, reward (0, 1, 0), 4,096 boards, gamma 1,
    epsilon 0.25, rate 8, 300 training steps, 16 evaluation steps).  The yardstick is the 2 x 4 learner of the same run, as for the
    3 x 3 learner: the sum learner's win count must exceed the zero table's by at least half of the margin by which the 2 x 4
    learner's does.  A state adds to both parts, so the step of V per unit of rate is about twice the 2 x 4 learner's; rates 4 to 32
    converge on this game, and a doubled step at rate 8 is inside that range."""
    TRAIN, EVAL, n = 300, 16, 4096

    def run(shape):
        env = _two_piece_env(n)
        learner = T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.25, seed=5, shape=shape)
        assert learner.shape == shape and T.ntuple_shape(learner.table) == shape and learner.policy.shape == shape
        before = learner.evaluate(EVAL)
        assert int(learner.table.abs().sum()) == 0
        assert learner.train(TRAIN) == TRAIN
        result = before, learner.evaluate(EVAL), learner.table.clone()
        if shape == SUM:                                       # the table plays at depth 2 and under the beam, by its size
            two, beam = learner.evaluate(EVAL, depth=2), learner.evaluate(EVAL, depth=3, width=8)
            print(f"sum table: depth 2 {two}, beam 3 x 8 {beam}")
            assert two["wins"] == two["episodes"] > 0          # an episode is two moves: two plies see its end, whatever V says
            assert beam["episodes"] > 0 and learner.evaluate(EVAL, depth=3, width=8) == beam
            assert torch.equal(learner.table, result[2])       # evaluation trains nothing
            assert tuple(T.ntuple_value(env, learner.table).shape) == (n,)
        env.terminate()
        return result

    zero, narrow, _ = run("2x4")
    zero_sum, summed, table = run(SUM)
    print(f"wins of {zero['episodes']} episodes: zero table {zero['wins']}, 2x4 {narrow['wins']} of {narrow['episodes']}, "
          f"2x4+3x3 {summed['wins']} of {summed['episodes']}; entries in use {[int((p != 0).sum()) for p in T.ntuple_parts(table)]}")
    assert zero_sum == zero                                    # the zero table plays the same game in any form
    assert tuple(table.shape) == (ES,) and narrow["wins"] > zero["wins"]
    assert summed["wins"] - zero["wins"] >= (narrow["wins"] - zero["wins"]) / 2
    assert all(int((p != 0).sum()) > 0 for p in T.ntuple_parts(table))
    _, again, table2 = run(SUM)
    assert again == summed and torch.equal(table, table2)      # the same seed, the same bytes
