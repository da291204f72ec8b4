"""Feature tuples on one MI355X (include/tpl_learn.h's "Feature tuples"; the ntuple_feature_* and ntuple_feature3_* kernels of
csrc/learn/ntuple.hip and ntuple_beam.hip; ntuple.py).  The state set is the other n-tuple GPU tests': the 1,639 states of the
afterstate pool (L = 10, M = 40) and their 65,560 afterstates, finished ones included, with the comb board and the empty board under
every falling piece added; sizes n = 1, 7, 9, 257 -- no multiple of an act block's 8 boards nor of 256 -- and the whole set.  Tables are
random in +-2^20, floats are compared as bits, and canaries frame every buffer the kernels are handed.

  * BINS: tpl_ntuple_feature_bins is the host mirror's min(board_features, 255) on the whole set;
  * VALUE: both forms are the numpy mirror; with one part zero the sum form gives tpl_ntuple_value_shaped's bits (3 x 3) and the
    "feat" kernel's;
  * ACT and SEARCH at epsilon 0 and 0.25, at the four sizes and on all 1,655 root states (the pool, the comb and the empty boards):
    tpl_afterstates' rewards, the mirror's V and ntuple_explore; for search two plies of afterstates and ntuple_search_choice --
    nothing of the kernels under test is in either reference;
  * BEAM: depth 1 is act and (2, 34) search at the same sizes and states; (3, 8) and (11, 64) are test_ntuple_beam_gpu's reference
    composed ply by ply on 48 pool states and the sixteen comb and empty boards;
  * UPDATE: horizons 1, 4 and 16 in a ring of 17 slots whose head wraps, symmetric and not, errors 0, NaN and past the clamp, from a
    table with entries at the top of the int32 range: the mirror's bytes; 4,096 states of 8 distinct boards with errors at the clamp,
    where every live entry takes thousands of adds and the totals pass 2^32, and the same bytes with the states permuted;
  * LEARNER on the two-piece game: train(3) is the loop composed by hand; one seed, the same bytes; symmetric stays symmetric;
    evaluate() at depth 1, 2 and (3, 8) runs; the win counts of 100 steps are printed beside the zero table's, not asserted.
"""
import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, _i32
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_beam_gpu import compose
from test_ntuple_gpu import GAMMA, PARAMS, _fields, _framed, after, pool  # noqa: F401  (fixtures)
from test_ntuple_trace_gpu import _age, _two_piece_env

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FEAT, BOTH = "feat", "3x3+feat"
E3, EF, E3F = 590848, 19456, 610304
FORMS = {FEAT: 0, BOTH: 1}
ENTRIES = {FEAT: EF, BOTH: E3F}
SIZES = [1, 7, 9, 257]
ARANGE = np.arange(40)


def _m():
    return T._learn_lib


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _random(seed, entries, span=1 << 20):
    return np.random.default_rng(seed).integers(-span, span + 1, entries).astype(np.int32)


def _extra():
    """The comb board (rows 1 .. 19 0b0101010101: wells 950, past the last bin) and the empty board under every falling piece."""
    comb = np.zeros(20, np.uint16)
    comb[1:] = 0b0101010101
    rows = np.stack([comb] * 8 + [np.zeros(20, np.uint16)] * 8)
    window = (np.arange(16, dtype=np.uint64) % np.uint64(8)) | (np.uint64(0o1234560123) << np.uint64(3))
    return R.pack_state(rows, 1, 3, 0, 0, window)


def _indices(f, form, L=L, M=M):
    return _m().ntuple_indices(f["rows"], f["cur"], L, M, f["lines"], f["moves"], shape=form)


def _value_of(table, part, idx=None):
    """The mirror's V from indices computed once."""
    pick = (lambda v: v) if idx is None else (lambda v: v[idx])
    total = np.where(pick(part["used"]), table[pick(part["index"])].astype(np.int64), 0).sum(axis=1)
    return np.where(pick(part["fields"]["state"]) == 0, total.astype(np.float32) * np.float32(2.0 ** -16), np.float32(0.0)).astype(np.float32)


@pytest.fixture(scope="module")
def whole(pool, after):
    """The whole set -- pool, afterstates, the comb and the empty boards -- with the indices of both forms, once."""
    XA, XB = _extra()
    A = np.ascontiguousarray(np.concatenate([pool.A, after["A"], XA]))
    B = np.ascontiguousarray(np.concatenate([pool.B, after["B"], XB]))
    f = _fields(A, B)
    out = dict(A=A, B=B, fields=f)
    for form in FORMS:
        index, used = _indices(f, form)
        out[form] = dict(fields=f, index=index, used=used)
    return out


# ------------------------------------------------------------------------------------------------ the entries, framed
def _value(A, B, table, form, L=L, M=M):
    """form: a feature form's name, or "3x3": tpl_ntuple_value_shaped with shape 1."""
    n = A.shape[0]
    a, b, t, v = _framed(A, 1), _framed(B, 2), _framed(table, 3), Framed(4 * n, 4)
    v.inner().fill_(0xCD)
    entry, tail = (_lib().tpl_ntuple_value_shaped, 1) if form == "3x3" else (_lib().tpl_ntuple_value_feature, FORMS[form])
    _check(entry(a.ptr(), b.ptr(), n, L, M, t.ptr(), v.ptr(), tail, _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("value", v)):
        f.assert_canary((n, form, k))
    assert np.array_equal(t.host().view(np.int32), table) and np.array_equal(a.host(), A.view(np.uint8).reshape(-1))
    return v.host().view(np.float32).copy()


def _policy(depth, A, B, table, form, gamma=GAMMA, epsilon=0.0, seed=0, step=0, L=L, M=M, params=PARAMS):
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, second=1, score=4, after_a=16, after_b=16, value=4)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    head = (a.ptr(), b.ptr(), n, L, M, *params, gamma, t.ptr(), epsilon, seed, step, p("action"))
    tail = (p("score"), p("after_a"), p("after_b"), p("value"), FORMS[form], _stream())
    _check(_lib().tpl_ntuple_search_feature(*head, p("second"), *tail) if depth == 2 else _lib().tpl_ntuple_act_feature(*head, *tail))
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


def _beam(A, B, table, depth, width, form, gamma=GAMMA, L=L, M=M, params=PARAMS):
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, plan=depth, score=4, after_a=16, after_b=16)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    _check(_lib().tpl_ntuple_beam_feature(a.ptr(), b.ptr(), n, L, M, *params, gamma, t.ptr(), depth, width, p("action"), p("plan"),
                                          p("score"), p("after_a"), p("after_b"), FORMS[form], _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((n, depth, width, form, k))
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
        g = np.ascontiguousarray(got[k]).view(np.uint8).reshape(len(got[k]), -1)
        w = np.ascontiguousarray(want[k]).view(np.uint8).reshape(len(want[k]), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (what, k, bad.size, bad[:5].tolist(), got[k][bad[:5]].tolist(), want[k][bad[:5]].tolist())


# ------------------------------------------------------------------------------------------------ BINS
def test_the_bins_are_the_host_mirrors_on_the_whole_set(whole):
    A, B = whole["A"], whole["B"]
    n = A.shape[0]
    assert n == POOL * 41 + 16
    a, b, out = _framed(A, 1), _framed(B, 2), Framed(9 * n, 3)
    out.inner().fill_(0xCD)
    _check(_lib().tpl_ntuple_feature_bins(a.ptr(), b.ptr(), n, out.ptr(), _stream()))
    for k, f in (("a", a), ("b", b), ("bins", out)):
        f.assert_canary(k)
    got = out.host().reshape(n, 9)
    phi = _m().board_features(whole["fields"]["rows"])
    assert np.array_equal(got, np.minimum(phi, 255).astype(np.uint8))
    assert (got[-16:-8, 6] == 255).all() and (phi[-16:-8, 6] == 950).all()                   # the comb: clamped
    assert (got[-8:] == np.array([0, 0, 0, 0, 40, 10, 0, 0, 0], np.uint8)).all()               # the empty board
    assert (whole["fields"]["state"] != 0).sum() > 4000        # finished states get their bins too
    for size in SIZES:                                         # the public function, at sizes around a block's edge
        planes = tuple(torch.from_numpy(x[5:5 + size].view(np.int32).copy()).to(DEV) for x in (A, B))
        assert np.array_equal(_np(T.ntuple_feature_bins(planes)), got[5:5 + size])


# ------------------------------------------------------------------------------------------------ VALUE
@pytest.mark.parametrize("form", list(FORMS))
def test_value_is_the_mirror_bit_for_bit_on_the_whole_set(whole, form):
    table = _random(17, ENTRIES[form])
    got, want = _value(whole["A"], whole["B"], table, form), _value_of(table, whole[form])
    assert np.array_equal(_bits(got), _bits(want))
    done = whole["fields"]["state"] != 0
    assert (_bits(got)[done] == 0).all() and (got[~done] != 0).mean() > 0.99 and done.sum() > 4000
    assert len(set(_bits(got[-16:]).tolist())) == 16           # the comb and the empty board differ under every piece
    full = _random(18, ENTRIES[form], span=(1 << 31) - 1)      # the whole int32 range: the sum is rounded at the conversion
    pick = np.arange(0, whole["A"].shape[0], 41)
    got = _value(np.ascontiguousarray(whole["A"][pick]), np.ascontiguousarray(whole["B"][pick]), full, form)
    assert np.array_equal(_bits(got), _bits(_value_of(full, whole[form], pick))) and (np.abs(got) * 65536.0 > (1 << 24)).any()


@pytest.mark.parametrize("n", SIZES)
def test_value_at_sizes_around_the_block_edges_and_with_one_part_zero(whole, n):
    idx = (np.arange(n) * 40 + 977 * n) % (POOL * 41)
    if n == 1:
        idx = np.flatnonzero(whole["fields"]["state"] == 0)[977:978]
    A, B = np.ascontiguousarray(whole["A"][idx]), np.ascontiguousarray(whole["B"][idx])
    table = _random(n, E3F)
    for form in FORMS:
        t = np.ascontiguousarray(table[-ENTRIES[form]:])
        got = _value(A, B, t, form)
        assert np.array_equal(_bits(got), _bits(_value_of(t, whole[form], idx))) and (got != 0).any()
    only3, onlyf = table.copy(), table.copy()
    only3[E3:], onlyf[:E3] = 0, 0
    assert np.array_equal(_bits(_value(A, B, only3, BOTH)), _bits(_value(A, B, np.ascontiguousarray(table[:E3]), "3x3")))
    assert np.array_equal(_bits(_value(A, B, onlyf, BOTH)), _bits(_value(A, B, np.ascontiguousarray(table[E3:]), FEAT)))


# ------------------------------------------------------------------------------------------------ ACT and SEARCH
ALL = POOL + 16                                                # the whole set of root states: the pool, then the comb and empty boards


@pytest.fixture(scope="module")
def roots(pool):
    """The root states of act, search and beam: the pool's 1,639, then the comb board and the empty board under every falling piece."""
    XA, XB = _extra()
    A, B = np.ascontiguousarray(np.concatenate([pool.A, XA])), np.ascontiguousarray(np.concatenate([pool.B, XB]))
    f = _fields(A, B)
    assert A.shape[0] == ALL and (f["state"][POOL:] == 0).all() and sorted(f["cur"][POOL:].tolist()) == sorted(list(range(8)) * 2)
    return dict(A=A, B=B, running=f["state"] == 0, cur=f["cur"].astype(np.int64))


def _take(n, offset):
    """n root states: the whole set (the sixteen extra boards included), or n of the pool's from `offset` on."""
    return np.arange(ALL) if n == ALL else (offset + np.arange(n)) % POOL


@pytest.fixture(scope="module")
def ply(roots):
    """tpl_afterstates on the root states, once: the 40 afterstates of every state with their rewards, done flags and canonical
    actions, and the indices of the afterstates under both forms."""
    n = ALL
    a, b = _framed(roots["A"], 1), _framed(roots["B"], 2)
    out_a, out_b = Framed(n * 640, 3), Framed(n * 640, 4)
    reward, done, canonical = Framed(n * 160, 5), Framed(n * 40, 6), Framed(n * 40, 7)
    _check(_lib().tpl_afterstates(a.ptr(), b.ptr(), n, L, M, *PARAMS, out_a.ptr(), out_b.ptr(), reward.ptr(), done.ptr(), None,
                                  canonical.ptr(), _stream()))
    A, B = out_a.host().view(np.uint32).reshape(-1, 4).copy(), out_b.host().view(np.uint32).reshape(-1, 4).copy()
    f = _fields(A, B)
    out = dict(A=A.reshape(n, 40, 4), B=B.reshape(n, 40, 4), reward=reward.host().view(np.float32).reshape(n, 40).copy(),
               done=done.host().reshape(n, 40) != 0, distinct=canonical.host().reshape(n, 40) == ARANGE[None, :])
    for form in FORMS:
        index, used = _indices(f, form)
        out[form] = dict(fields=f, index=index, used=used)
    return out


@pytest.fixture(scope="module")
def tables():
    return {form: _random(40 + FORMS[form], ENTRIES[form]) for form in FORMS}


def _explored(roots, ply, idx, greedy, epsilon, seed, step):
    """The action played: the greedy one, or where a running board explores the j-th of its distinct placements (ntuple_explore)."""
    n, run = idx.size, roots["running"][idx]
    explores, j = _m().ntuple_explore(seed, step, n, epsilon, np.array(_m().PIECE_PLACEMENTS)[roots["cur"][idx]])
    explores &= run
    order = np.argsort(~ply["distinct"][idx], axis=1, kind="stable")          # the distinct placements first, ascending
    return np.where(explores, order[np.arange(n), j], np.where(run, greedy, 0)), explores


def _outcome(roots, ply, v, idx, action):
    """What follows from the action played: its one-ply afterstate (the board itself where it is finished) and V of it."""
    at, run = np.arange(idx.size), roots["running"][idx]
    value = np.where(ply["done"][idx][at, action] | ~run, np.float32(0.0), v[at, action]).astype(np.float32)
    return dict(after_a=np.where(run[:, None], ply["A"][idx][at, action], roots["A"][idx]),
                after_b=np.where(run[:, None], ply["B"][idx][at, action], roots["B"][idx]), value=value)


def _choice(roots, ply, table, form, idx, gamma=GAMMA, epsilon=0.0, seed=0, step=0):
    """The rule of tpl_ntuple_act for the states `idx` as boards 0 .. n - 1: tpl_afterstates' rewards, the mirror's V of the
    afterstates, the lowest placement at the maximum, and the exploration draw."""
    n, at = idx.size, np.arange(idx.size)
    rows = (idx[:, None] * 40 + ARANGE[None, :]).reshape(-1)
    v = _value_of(table, ply[form], rows).reshape(n, 40)
    done, run, distinct = ply["done"][idx], roots["running"][idx], ply["distinct"][idx]
    score = np.where(done, ply["reward"][idx], ply["reward"][idx] + np.float32(gamma) * v).astype(np.float32)
    score = np.where(run[:, None], score, np.float32(0.0))
    masked = np.where(distinct, score, -np.inf)
    greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)
    action, explores = _explored(roots, ply, idx, greedy, epsilon, seed, step)
    return dict(action=action.astype(np.uint8), score=score[at, greedy], **_outcome(roots, ply, v, idx, action)), explores


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES + [ALL])
def test_act_is_the_mirror_arg_max_at_both_epsilons(roots, ply, tables, form, n):
    idx = _take(n, 13 * n)
    A, B = np.ascontiguousarray(roots["A"][idx]), np.ascontiguousarray(roots["B"][idx])
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    for epsilon in (0.0, 0.25):
        want, explores = _choice(roots, ply, tables[form], form, idx, epsilon=epsilon, seed=seed, step=step)
        got = _policy(1, A, B, tables[form], form, epsilon=epsilon, seed=seed, step=step)
        _same(got, want, (form, n, epsilon))
    if n == ALL:
        run = roots["running"]
        assert 0.15 * run.sum() < explores.sum() < 0.35 * run.sum()
        greedy, _ = _choice(roots, ply, tables[form], form, idx)
        assert len(set(greedy["action"][run].tolist())) > 20
        assert (got["action"][~run] == 0).all() and (_bits(got["score"])[~run] == 0).all() and (_bits(got["value"])[~run] == 0).all()
        assert np.array_equal(got["after_a"][~run], A[~run]) and np.array_equal(got["after_b"][~run], B[~run])
        ended = ply["done"][np.arange(n), greedy["action"]] & run
        assert ended.sum() >= 20 and (greedy["value"][ended] == 0).all()


@pytest.fixture(scope="module")
def env10():
    """Any L = 10 / M = 40 environment with the reward parameters: T.afterstates reads L, M and the rewards from it."""
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=9, reward=PARAMS)
    yield env
    env.terminate()


def _second_ply(env, dev_table, ply, idx, L=L, M=M):
    """The second ply of the states `idx`: T.afterstates on their 40 n first afterstates -- reward, done and distinct [n, 40, 40] --
    and V of the 1,600 n boards that leaves from T.ntuple_value, which the value tests hold to the mirror on the whole set."""
    n = idx.size
    sa = _i32(ply["A"][idx].reshape(-1, 4)).to(DEV)
    sb = _i32(ply["B"][idx].reshape(-1, 4)).to(DEV)
    two = T.afterstates(env, sa, sb)
    v = T.ntuple_value((two["states_a"].view(-1, 4), two["states_b"].view(-1, 4)), dev_table, L, M)
    shape = (n, 40, 40)
    return dict(reward=_np(two["reward"]).reshape(shape), done=_np(two["done"]).reshape(shape) != 0, value=_np(v).reshape(shape),
                distinct=_np(two["canonical"]).reshape(shape) == ARANGE)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES + [ALL])
def test_search_is_ntuple_search_choice_on_two_plies_of_afterstates_at_both_epsilons(roots, ply, env10, tables, form, n):
    """The numpy rule, with nothing of the kernels under test in it: the first ply from tpl_afterstates with the mirror's V, the second
    from T.afterstates with T.ntuple_value's V, ntuple_search_choice for Q, `second` and the greedy action, ntuple_explore for the draw."""
    idx = _take(n, 13 * n)
    at = np.arange(n)
    A, B = np.ascontiguousarray(roots["A"][idx]), np.ascontiguousarray(roots["B"][idx])
    run = roots["running"][idx]
    table = tables[form]
    dev_table = torch.from_numpy(table).to(DEV)
    rows = (idx[:, None] * 40 + ARANGE[None, :]).reshape(-1)
    v1 = _value_of(table, ply[form], rows).reshape(n, 40)
    held = _np(T.ntuple_value((_i32(ply["A"][idx].reshape(-1, 4)).to(DEV), _i32(ply["B"][idx].reshape(-1, 4)).to(DEV)), dev_table, L, M))
    assert np.array_equal(_bits(held), _bits(v1.reshape(-1)))   # T.ntuple_value is the mirror on these afterstates too
    two = _second_ply(env10, dev_table, ply, idx)
    greedy, _, score, Q, second = _m().ntuple_search_choice(ply["reward"][idx], ply["done"][idx], ply["distinct"][idx], two["reward"],
                                                            two["done"], two["value"], two["distinct"], GAMMA, running=run)
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    for epsilon in (0.0, 0.25):
        action, explores = _explored(roots, ply, idx, greedy.astype(np.int64), epsilon, seed, step)
        want = dict(action=action.astype(np.uint8), second=second[at, action], score=score, **_outcome(roots, ply, v1, idx, action))
        got = _policy(2, A, B, table, form, epsilon=epsilon, seed=seed, step=step)
        _same(got, want, (form, n, epsilon))
        assert (got["action"][~run] == 0).all() and (got["second"][~run] == 255).all() and (_bits(got["score"])[~run] == 0).all()
        assert np.array_equal(got["after_a"][~run], A[~run]) and np.array_equal(got["after_b"][~run], B[~run])
    if n == ALL:
        assert explores.sum() > 0.15 * run.sum() and (got["action"] != greedy).sum() > 0.1 * run.sum()
        ended = ply["done"][idx][at, got["action"]] & run
        assert ended.sum() >= 20 and (got["second"][ended] == 255).all() and (_bits(got["value"])[ended] == 0).all()
        assert (got["second"][run & ~ended] != 255).all() and (got["value"][run & ~ended] != 0).all()
        one = _policy(1, A, B, table, form)
        assert (one["action"] != greedy).sum() >= 100          # two plies play another game


# ------------------------------------------------------------------------------------------------ BEAM
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES + [ALL])
def test_beam_at_depth_one_is_act_and_at_depth_two_and_full_width_search(roots, tables, form, n):
    idx = _take(n, 7 * n)
    A, B = np.ascontiguousarray(roots["A"][idx]), np.ascontiguousarray(roots["B"][idx])
    run = roots["running"][idx]
    one = _policy(1, A, B, tables[form], form)
    got = _beam(A, B, tables[form], 1, 5, form)
    _same(got, one, (form, n, 1), keys=("action", "score", "after_a", "after_b"))
    assert (got["plan"][:, 0] == np.where(run, one["action"], 255)).all()
    two = _policy(2, A, B, tables[form], form)
    got = _beam(A, B, tables[form], 2, 34, form)
    _same(got, two, (form, n, 2), keys=("action", "score", "after_a", "after_b"))
    assert ((got["plan"][:, 1] == 255) == (two["second"] == 255)).all()
    assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all() and (_bits(got["score"][~run]) == 0).all()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("depth,width", [(3, 8), (11, 64)])
def test_beam_is_the_reference_composed_ply_by_ply(roots, env10, tables, form, depth, width):
    """test_ntuple_beam_gpu.compose: every ply T.afterstates, V of the children from T.ntuple_value -- tpl_ntuple_value_feature, held
    to the mirror above --, the numpy fold and ntuple_beam_ply.  48 states of the pool and the sixteen comb and empty boards."""
    idx = np.concatenate([100 + np.arange(48), POOL + np.arange(16)])
    A, B = np.ascontiguousarray(roots["A"][idx]), np.ascontiguousarray(roots["B"][idx])
    run = roots["running"][idx]
    moves = _fields(A, B)["moves"]
    plies = np.where(run, np.minimum(depth, 11 - moves % 10), 0)
    want = compose(env10, tables[form], A, B, plies, depth, width)
    got = _beam(A, B, tables[form], depth, width, form)
    _same(got, want, (form, depth, width), keys=("action", "plan", "score"))
    assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all()
    assert (got["plan"][run, 0] == got["action"][run]).all() and (plies >= min(depth, 3)).sum() >= 10


# ------------------------------------------------------------------------------------------------ UPDATE
def _update(A, B, head, horizon, start, error, rate, decay, symmetric, L=L, M=M):
    """tpl_ntuple_update_trace_feature of a host ring (uint32 [slots, n, 4] each) through canary-framed buffers: the table it leaves."""
    slots, n = A.shape[:2]
    a, b, t, e = _framed(A, 1), _framed(B, 2), _framed(start, 3), _framed(error, 4)
    _check(_lib().tpl_ntuple_update_trace_feature(a.ptr(), b.ptr(), n, slots, head, horizon, L, M, t.ptr(), e.ptr(), rate, decay,
                                                  int(symmetric), _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("error", e)):
        f.assert_canary((n, slots, head, horizon, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(e.host(), error.view(np.uint8))
    return t.host().view(np.int32).copy()


def _start(seed):
    start = np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, EF).astype(np.int32)
    start[::3] = np.int32((1 << 31) - 1)                       # entries at the top of the range: their adds wrap
    return start


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("horizon,head,n", [(1, 16, 257), (4, 2, 4096), (16, 9, 1000), (16, 3, 7)])
def test_the_update_leaves_the_mirror_bytes_in_a_ring_whose_head_wraps(whole, horizon, head, n, symmetric):
    slots = 17
    gen = np.random.default_rng(100 * horizon + head + symmetric)
    state = whole["fields"]["state"]
    done, live = np.flatnonzero(state != 0), np.flatnonzero(state == 0)
    picks = np.where(gen.random((slots, n)) < 0.1, done[gen.integers(0, done.size, (slots, n))], live[gen.integers(0, live.size, (slots, n))])
    picks[(head - gen.integers(0, horizon, 16)) % slots, gen.integers(0, n, 16)] = whole["A"].shape[0] - 16 + np.arange(16)   # comb, empty
    A, B = np.ascontiguousarray(whole["A"][picks]), np.ascontiguousarray(whole["B"][picks])
    rate = 3000.0
    error = gen.normal(size=n).astype(np.float32)
    special = np.array([0.0, np.nan, 1e9, -1e9, 0.52 / rate, -0.0, np.inf], np.float32)
    error[gen.permutation(n)[:min(special.size, n)]] = special[:min(special.size, n)]
    start = _start(horizon + n)
    ages = [_age(whole["fields"], picks[(head - k) % slots]) for k in range(horizon)]
    assert horizon == 1 or head < horizon - 1                  # the older ages wrap past slot 0
    got = _update(A, B, head, horizon, start, error, rate, 0.9, symmetric)
    want = _m().ntuple_update_trace(start.copy(), ages, L, M, error, rate, 0.9, bool(symmetric))
    assert np.array_equal(got, want) and (got != start).any()
    if n >= 1000:
        assert (got != start)[:18432].sum() > 500 and (got != start)[18432:].any()


def test_4096_states_of_8_boards_with_errors_at_the_clamp_and_the_same_bytes_with_the_states_permuted(whole):
    n, slots, head, horizon = 4096, 17, 1, 4
    gen = np.random.default_rng(8)
    live = np.flatnonzero(whole["fields"]["state"] == 0)
    eight = live[gen.integers(0, live.size, 8)]
    eight[0] = whole["A"].shape[0] - 13                        # a comb board among them: the clamped bin
    picks = np.broadcast_to(eight[gen.integers(0, 8, n)], (slots, n))
    error = np.where(gen.random(n) < 0.9, 1e9, -1e9).astype(np.float32)          # every step is +-2^24
    start = _start(5)
    for symmetric in (0, 1):
        A, B = np.ascontiguousarray(whole["A"][picks]), np.ascontiguousarray(whole["B"][picks])
        ages = [_age(whole["fields"], picks[0])] * horizon
        got = _update(A, B, head, horizon, start, error, 3000.0, 1.0, symmetric)
        want = _m().ntuple_update_trace(start.copy(), ages, L, M, error, 3000.0, 1.0, bool(symmetric))
        assert np.array_equal(got, want)
        changed = np.flatnonzero(got != start)
        assert 10 <= changed.size <= 8 * 19 + 8
        total = horizon * int(_m().ntuple_steps(error, 3000.0).sum())
        assert abs(total) > 1 << 32                            # the sum of all steps passes 2^32: the adds wrapped
        order = gen.permutation(n)
        again = _update(np.ascontiguousarray(A[:, order]), np.ascontiguousarray(B[:, order]), head, horizon, start,
                        np.ascontiguousarray(error[order]), 3000.0, 1.0, symmetric)
        assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------------ LEARNER
def _by_hand(env, form, steps, gamma, rate, epsilon, seed):
    """The learner's loop from the public pieces: NTuplePolicy.act, ntuple_value, the subtraction, the update entries part by part,
    the environment's step."""
    n, lib = env.num_envs, _lib()
    table = T.ntuple_table(DEV, form)
    policy = T.NTuplePolicy(env, table, gamma, epsilon, seed)
    action, done = (torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(2))
    reward, score, error = (torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(3))
    kept = [torch.zeros((n, 4), dtype=torch.int32, device=DEV) for _ in range(2)]
    nxt = [torch.zeros((n, 4), dtype=torch.int32, device=DEV) for _ in range(2)]
    kept[1][:, 1] = 1 << 28                                    # finished states: nothing is kept before the first step
    parts = T.ntuple_parts(table)
    for step in range(steps):
        policy.act(out=action, score=score, after=tuple(nxt), step=step)
        torch.sub(score, T.ntuple_value(tuple(kept), table, env.L, env.M), out=error)
        ring = (kept[0].data_ptr(), kept[1].data_ptr(), n, 1, 0, 1, env.L, env.M)
        if form == BOTH:
            _check(lib.tpl_ntuple_update_trace_shaped(*ring, parts[0].data_ptr(), error.data_ptr(), rate, 0.0, 0, 1, _stream()))
        _check(lib.tpl_ntuple_update_trace_feature(*ring, parts[-1].data_ptr(), error.data_ptr(), rate, 0.0, 0, _stream()))
        env.step_into(action, reward, done)
        kept, nxt = nxt, kept
    return table


@pytest.mark.parametrize("form", list(FORMS))
def test_three_train_steps_leave_the_bytes_of_the_loop_composed_by_hand(form):
    kw = dict(gamma=1.0, rate=64.0, epsilon=0.25, seed=5)
    env = _two_piece_env(4096)
    env.reset()
    want = _np(_by_hand(env, form, 3, **kw)).copy()
    env.terminate()
    env = _two_piece_env(4096)
    env.reset()
    learner = T.NTupleLearner(env, shape=form, **kw)
    assert learner.shape == form and learner.policy.shape == form and tuple(learner.table.shape) == (ENTRIES[form],)
    assert learner.train(3) == 3
    got = _np(learner.table).copy()
    env.terminate()
    assert np.array_equal(got, want) and np.count_nonzero(got[-EF:-1024]) > 10 and np.count_nonzero(got[-1024:]) > 0
    assert form == FEAT or np.count_nonzero(got[:E3]) > 10


def test_learners_are_deterministic_symmetric_ones_stay_symmetric_and_every_evaluation_runs():
    """The two-piece game (L = 2, M = 2, the 64-configuration pool, reward (0, 1, 0), 4,096 boards, gamma 1, epsilon 0.25).  A state
    adds to 10 entries of a feature table where it adds to about 107 of a 3 x 3 one, so "feat" alone runs at rate 64 where the window
    tables run at 8.  The win counts are printed, not asserted: nobody has measured what a feature table learns here."""
    TRAIN, EVAL, n = 100, 16, 4096

    def run(form, rate, **kw):
        env = _two_piece_env(n)
        learner = T.NTupleLearner(env, gamma=1.0, rate=rate, epsilon=0.25, seed=5, shape=form, **kw)
        zero = learner.evaluate(EVAL)
        assert int(learner.table.abs().sum()) == 0 and learner.train(TRAIN) == TRAIN
        played = dict(depth_1=learner.evaluate(EVAL), depth_2=learner.evaluate(EVAL, depth=2), beam_3x8=learner.evaluate(EVAL, depth=3, width=8))
        assert all(r["episodes"] > 0 for r in played.values()) and played["depth_2"]["wins"] == played["depth_2"]["episodes"]
        table = learner.table.clone()
        symmetric = T.ntuple_is_symmetric(learner.table)
        assert tuple(T.ntuple_value(env, learner.table).shape) == (n,)
        env.terminate()
        return zero, played, table, symmetric

    for form, rate in ((FEAT, 64.0), (BOTH, 8.0)):
        zero, played, table, symmetric = run(form, rate)
        _, again, table2, _ = run(form, rate)
        assert torch.equal(table, table2) and again == played  # one seed, the same bytes
        _, with_sigma, table3, symmetric = run(form, rate / 2, lam=0.8, horizon=2, symmetric=True)
        assert symmetric and int((table3 != 0).sum()) > 10
        print(f"{form}: zero table {zero['wins']} of {zero['episodes']}; after {TRAIN} steps at rate {rate}: "
              + ", ".join(f"{k} {v['wins']} of {v['episodes']}" for k, v in played.items())
              + f"; symmetric with traces at rate {rate / 2}: {with_sigma['depth_1']['wins']} of {with_sigma['depth_1']['episodes']}"
              + f"; entries in use {[int((p != 0).sum()) for p in T.ntuple_parts(table)]}")
