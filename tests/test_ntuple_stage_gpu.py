"""Stage-indexed n-tuple tables on one MI355X (include/tpl_learn.h's "Staged tables"; the ntuple_staged*_kernel of csrc/learn/ntuple.hip
and ntuple_beam.hip; ntuple.py).  The states are test_ntuple_gpu's: the 1,639 states of the afterstate pool (L = 10, M = 40) and their
65,560 afterstates; n = 1, 7, 8, 9 around an act block's eight boards, n = 255, 256, 257 around the 256 lanes of a value or update
block.  Floats are compared as bits, and canaries frame every buffer the kernels are handed.

  1. VALUE: the staged value is the numpy mirror bit for bit, for each form, under eight distinct random blocks and the map
     stage = moves left & 7 -- on states that fall in at least four stages;
  2. REPLICATION: a staged table of eight copies of a plain table writes the plain kernels' bytes for value, act, search (both epsilons)
     and beam, under the moves map and under a map of random 32-bit words;
  3. STAGES CROSSED: under the moves map, where every ply changes stage, and distinct blocks, act, search and beam are the reference
     composed ply by ply from T.afterstates, the staged T.ntuple_value and the numpy folds; a played beam plan reaches its score;
  4. UPDATE: one staged update leaves the mirror's bytes, the map and the blocks of unused stages untouched; under the all-zero map
     block 0 takes the plain update's bytes; shuffled boards, the same bytes;
  5. LEARNER: one seed, the same bytes; promoted from a plain table under the all-zero map, block 0 is the plain learner's table step
     for step and the other blocks stay; symmetric stays symmetric under four stages; evaluate at depth 1, 2 and beam (3, 8).
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, _i32, _resident
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_beam_gpu import compose
from test_ntuple_gpu import GAMMA, PARAMS, _fields, _framed, after, pool  # noqa: F401  (fixtures)
from test_ntuple_trace_gpu import _age, _carved_env, _errors, _picks, _ring

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SUM = "2x4+3x3"
FORMS = {"2x4": 314368, "3x3": 590848, SUM: 905216}
FORM_IDS = {"2x4": 0, "3x3": 1, SUM: 2}
PART_AT = {"2x4": ((0, 0),), "3x3": ((1, 0),), SUM: ((0, 0), (1, 314368))}        # (C shape, first entry) of a form's parts
BOARDS = [1, 7, 8, 9]                                          # around an act block's eight boards
LANES = [255, 256, 257]                                        # around a value or update block's 256 lanes
ARANGE = np.arange(40)
MOVES_MAP = (np.arange(1024) % 64 & 7).astype(np.int32)        # stage = moves left & 7: every move changes the stage
WILD_MAP = np.random.default_rng(77).integers(-(1 << 31), 1 << 31, 1024).astype(np.int32)


def _m():
    return T._learn_lib


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _blocks(seed, form, stage_map, span=1 << 20):
    """A staged table of eight DISTINCT random blocks."""
    body = np.random.default_rng(seed).integers(-span, span + 1, 8 * FORMS[form]).astype(np.int32)
    return np.concatenate([body, stage_map])


def _copies(plain, stage_map):
    """ntuple_staged on the host: eight copies of a plain table, then the map."""
    return np.concatenate([np.tile(plain, 8), stage_map])


def _entry(base, form, staged):
    """(the C entry, its trailing arguments before `stream`) that reads a table of `form`, staged or plain."""
    if staged:
        return getattr(_lib(), base + "_staged"), (FORM_IDS[form],)
    if form == SUM:
        return getattr(_lib(), base + "_sum"), ()
    return getattr(_lib(), base if base == "tpl_ntuple_beam" else base + "_shaped"), (FORM_IDS[form],)


# ------------------------------------------------------------------------------------------------ the entries, framed
def _value(A, B, table, form, staged=True, L=L, M=M):
    n = A.shape[0]
    a, b, t, v = _framed(A, 1), _framed(B, 2), _framed(table, 3), Framed(4 * n, 4)
    v.inner().fill_(0xCD)
    entry, tail = _entry("tpl_ntuple_value", form, staged)
    _check(entry(a.ptr(), b.ptr(), n, L, M, t.ptr(), v.ptr(), *tail, _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("value", v)):
        f.assert_canary((n, form, staged, k))
    assert np.array_equal(t.host().view(np.int32), table)
    return dict(value=v.host().view(np.float32).copy())


def _outputs(out, n, depth=None):
    host = {k: f.host().copy() for k, f in out.items()}
    for k in ("after_a", "after_b"):
        host[k] = host[k].view(np.uint32).reshape(n, 4)
    for k in ("score", "value"):
        if k in host:
            host[k] = host[k].view(np.float32)
    if "plan" in host:
        host["plan"] = host["plan"].reshape(n, depth)
    return host


def _policy(depth, A, B, table, form, staged=True, gamma=GAMMA, epsilon=0.0, seed=0, step=0, L=L, M=M, params=PARAMS):
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, second=1, score=4, after_a=16, after_b=16, value=4)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    entry, tail = _entry("tpl_ntuple_search" if depth == 2 else "tpl_ntuple_act", form, staged)
    head = (a.ptr(), b.ptr(), n, L, M, *params, gamma, t.ptr(), epsilon, seed, step, p("action"))
    rest = (p("score"), p("after_a"), p("after_b"), p("value"), *tail, _stream())
    _check(entry(*head, p("second"), *rest) if depth == 2 else entry(*head, *rest))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((depth, n, form, staged, epsilon, k))
    assert np.array_equal(t.host().view(np.int32), table)
    if depth == 1:
        assert (out.pop("second").host() == 0xCD).all()
    return _outputs(out, n)


def _beam(A, B, table, depth, width, form, staged=True, gamma=GAMMA, L=L, M=M, params=PARAMS):
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, plan=depth, score=4, after_a=16, after_b=16)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    entry, tail = _entry("tpl_ntuple_beam", form, staged)
    _check(entry(a.ptr(), b.ptr(), n, L, M, *params, gamma, t.ptr(), depth, width, p("action"), p("plan"), p("score"), p("after_a"),
                 p("after_b"), *tail, _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((n, depth, width, form, staged, k))
    assert np.array_equal(t.host().view(np.int32), table)
    return _outputs(out, n, depth)


def _same(got, want, what, keys=None):
    """Every output of `want` (or `keys` of them), byte for byte."""
    for k in (want if keys is None else keys):
        g = np.ascontiguousarray(got[k]).view(np.uint8).reshape(len(got[k]), -1)
        w = np.ascontiguousarray(want[k]).view(np.uint8).reshape(len(want[k]), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (what, k, bad.size, bad[:5].tolist(), got[k][bad[:5]].tolist(), want[k][bad[:5]].tolist())


def _states(pool, n, offset):
    idx = pool.take(n, offset)
    return idx, np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])


def _mirror_value(table, f, idx, L=L, M=M):
    return _m().ntuple_value(table, f["rows"][idx], f["cur"][idx], L, M, f["lines"][idx], f["moves"][idx], f["state"][idx])


@pytest.fixture(scope="module")
def env10():
    """Any L = 10 / M = 40 environment with the reward parameters: T.afterstates reads L, M and the rewards from it."""
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=9, reward=PARAMS)
    yield env
    env.terminate()


# ------------------------------------------------------------------------------------------------ 1. VALUE
@pytest.mark.parametrize("form", list(FORMS))
def test_the_staged_value_is_the_mirror_bit_for_bit_and_the_states_fall_in_many_stages(pool, after, form):
    table = _blocks(101, form, MOVES_MAP, span=(1 << 31) - 1)  # the whole int32 range: the rounding is at the conversion
    sets = [(n, after, (np.arange(n) * 40 + 977 * n) % (POOL * 40)) for n in LANES] + [(POOL, dict(A=pool.A, B=pool.B,
                                                                                                    fields=_fields(pool.A, pool.B)), np.arange(POOL))]
    for n, source, idx in sets:
        f = source["fields"]
        A, B = np.ascontiguousarray(source["A"][idx]), np.ascontiguousarray(source["B"][idx])
        got, want = _value(A, B, table, form)["value"], _mirror_value(table, f, idx)
        assert np.array_equal(_bits(got), _bits(want)), (form, n)
        run = f["state"][idx] == 0
        stages = _m().ntuple_stages_of(table, L, M, f["lines"][idx], f["moves"][idx])[run]
        assert len(set(stages.tolist())) >= 4, (n, sorted(set(stages.tolist())))      # a fixture collapsed to one stage cannot pass
        assert np.array_equal(stages, np.clip(M - f["moves"][idx][run], 0, 63) & 7)
        assert (_bits(got)[~run] == 0).all() and (got[run] != 0).all() and run.sum() >= n // 2
        # the stage decides: block 0 alone, read as a plain table, gives another value on most running states
        plain = _value(A, B, np.ascontiguousarray(table[:FORMS[form]]), form, staged=False)["value"]
        assert np.array_equal(_bits(plain)[run][stages == 0], _bits(got)[run][stages == 0])
        assert (_bits(plain)[run][stages != 0] != _bits(got)[run][stages != 0]).all()


# ------------------------------------------------------------------------------------------------ 2. REPLICATION
@pytest.mark.parametrize("stage_map", ["moves", "wild"])
@pytest.mark.parametrize("form", list(FORMS))
def test_eight_copies_of_a_plain_table_write_the_plain_kernels_bytes_whatever_the_map(pool, after, form, stage_map):
    plain = np.random.default_rng(200 + FORM_IDS[form]).integers(-(1 << 20), (1 << 20) + 1, FORMS[form]).astype(np.int32)
    staged = _copies(plain, MOVES_MAP if stage_map == "moves" else WILD_MAP)
    pick = (np.arange(257) * 40 + 977) % (POOL * 40)
    VA, VB = np.ascontiguousarray(after["A"][pick]), np.ascontiguousarray(after["B"][pick])
    _same(_value(VA, VB, staged, form), _value(VA, VB, plain, form, staged=False), (form, "value"))
    kw = dict(seed=0xDEADBEEFCAFEF00D, step=(1 << 40) + 3)
    for n in BOARDS:
        _, A, B = _states(pool, n, 13 * n)
        for depth in (1, 2):
            for epsilon in (0.0, 0.25):
                _same(_policy(depth, A, B, staged, form, epsilon=epsilon, **kw),
                      _policy(depth, A, B, plain, form, staged=False, epsilon=epsilon, **kw), (form, n, depth, epsilon))
        for depth, width in ((1, 1), (2, 34), (3, 8)):
            _same(_beam(A, B, staged, depth, width, form), _beam(A, B, plain, depth, width, form, staged=False), (form, n, depth, width))


# ------------------------------------------------------------------------------------------------ 3. STAGES CROSSED
def _state_of(B):
    return (B[..., 1] >> np.uint32(28)) & np.uint32(3)


def _one_ply(env, dev_table, A, B, L=L, M=M):
    """T.afterstates of the states and the staged T.ntuple_value of their afterstates -- each in the block of ITS lines and moves."""
    n = A.shape[0]
    after = T.afterstates(env, _i32(A).to(DEV), _i32(B).to(DEV))
    sa, sb = after["states_a"].view(-1, 4), after["states_b"].view(-1, 4)
    v = _np(T.ntuple_value((sa, sb), dev_table, L, M)).reshape(n, 40)
    return dict(A=_np(sa).view(np.uint32).reshape(n, 40, 4), B=_np(sb).view(np.uint32).reshape(n, 40, 4), value=v,
                reward=_np(after["reward"]).reshape(n, 40), done=_np(after["done"]).reshape(n, 40) != 0,
                distinct=_np(after["canonical"]).reshape(n, 40) == ARANGE)


def _outcome(A, B, one, action, run):
    at = np.arange(A.shape[0])
    value = np.where(one["done"][at, action] | ~run, np.float32(0.0), one["value"][at, action]).astype(np.float32)
    return dict(after_a=np.where(run[:, None], one["A"][at, action], A), after_b=np.where(run[:, None], one["B"][at, action], B),
                value=value)


@pytest.fixture(scope="module")
def crossed():
    """Per form: a staged table of distinct blocks under the moves map, on the host and on the device."""
    out = {}
    for form in FORMS:
        table = _blocks(300 + FORM_IDS[form], form, MOVES_MAP)
        out[form] = (table, torch.from_numpy(table).to(DEV))
    return out


@pytest.mark.parametrize("n", BOARDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_act_and_search_value_every_ply_in_its_own_stage(pool, env10, crossed, form, n):
    table, dev_table = crossed[form]
    _, A, B = _states(pool, n, 13 * n + 5)
    run = _state_of(B) == 0
    g = np.float32(GAMMA)
    one = _one_ply(env10, dev_table, A, B)
    # act: r + gamma V(afterstate), V in the afterstate's stage -- one move on from the root's
    score = np.where(run[:, None], np.where(one["done"], one["reward"], one["reward"] + g * one["value"]), np.float32(0.0)).astype(np.float32)
    masked = np.where(one["distinct"], score, -np.inf)
    action = np.where(run, np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1), 0)
    want = dict(action=action.astype(np.uint8), score=score[np.arange(n), action], **_outcome(A, B, one, action, run))
    got = _policy(1, A, B, table, form)
    _same(got, want, (form, n, "act"))
    # search: the second ply's boards are two moves on
    two = _one_ply(env10, dev_table, np.ascontiguousarray(one["A"].reshape(-1, 4)), np.ascontiguousarray(one["B"].reshape(-1, 4)))
    shape = (n, 40, 40)
    action, second, score, _, _ = _m().ntuple_search_choice(one["reward"], one["done"], one["distinct"], two["reward"].reshape(shape),
                                                            two["done"].reshape(shape), two["value"].reshape(shape),
                                                            two["distinct"].reshape(shape), GAMMA, running=run)
    want = dict(action=action, second=second, score=score, **_outcome(A, B, one, action.astype(np.int64), run))
    got2 = _policy(2, A, B, table, form)
    _same(got2, want, (form, n, "search"))
    if n == 9 and run.all():
        stage = lambda x: (np.clip(M - _fields(x["A"].reshape(-1, 4), x["B"].reshape(-1, 4))["moves"], 0, 63) & 7).reshape(n, -1)
        root = np.clip(M - _fields(A, B)["moves"], 0, 63) & 7
        going = ~one["done"]                                  # a finished afterstate is its own afterstate
        assert (stage(one) != root[:, None]).all() and (stage(two).reshape(n, 40, 40) != stage(one)[:, :, None])[going].all()


CASES = [(form, depth, width) for form in FORMS for depth, width in ((3, 8), (6, 16))] + [("2x4", 11, 64)]


def _plies(A, B, depth):
    """The effective depth of every state: 0 where it is finished, else min(depth, 11 - moves mod 10)."""
    return np.where(_state_of(B) == 0, np.minimum(depth, 11 - _fields(A, B)["moves"] % 10), 0)


@pytest.mark.parametrize("n", BOARDS)
@pytest.mark.parametrize("form,depth,width", CASES)
def test_the_beam_is_the_reference_composed_ply_by_ply_with_every_leaf_in_its_own_stage(pool, env10, crossed, form, depth, width, n):
    """test_ntuple_beam_gpu.compose: every ply T.afterstates, V of the children from the staged T.ntuple_value -- held to the mirror
    above --, the numpy fold and ntuple_beam_ply."""
    table, _ = crossed[form]
    _, A, B = _states(pool, n, 7 * n + 24)
    plies = _plies(A, B, depth)
    want = compose(env10, table, A, B, plies, depth, width)
    got = _beam(A, B, table, depth, width, form)
    _same(got, want, (form, depth, width, n), keys=("action", "plan", "score"))
    one = _policy(1, A, B, table, form)                        # `after` is the one-ply afterstate of the action, as act packs it
    run = _state_of(B) == 0
    assert (got["plan"][run, 0] == got["action"][run]).all() and (got["action"][~run] == 0).all()
    if depth == 3:
        same = got["action"] == one["action"]
        assert np.array_equal(got["after_a"][same], one["after_a"][same]) and np.array_equal(got["after_b"][same], one["after_b"][same])


@pytest.mark.parametrize("form", list(FORMS))
def test_playing_the_plan_of_a_staged_beam_reaches_its_score(pool, crossed, form):
    m, depth, width = _m(), 11, 8
    env, idx = _resident(pool, POOL, 0, PARAMS)
    table = crossed[form][1]
    policy = T.NTupleBeamPolicy(env, table, depth, width, gamma=GAMMA)
    assert policy.shape == form and policy.staged
    score = torch.empty(POOL, dtype=torch.float32, device=DEV)
    plan = torch.full((POOL, depth), 77, dtype=torch.uint8, device=DEV)
    action = policy.act(score=score, plan=plan)
    plan, score = _np(plan), _np(score)
    assert np.array_equal(_np(action), np.where(pool.running, plan[:, 0], 0))
    plies, length = _plies(pool.A, pool.B, depth), (plan != 255).sum(axis=1)
    assert (length <= plies).all() and (length[pool.running] >= 1).all()
    earned = np.zeros((POOL, depth), np.float32)
    final_v, final_state = np.zeros(POOL, np.float32), _state_of(pool.B).astype(np.int64)
    for j in range(depth):
        step = np.where(plan[:, j] == 255, 0, plan[:, j]).astype(np.uint8)
        _, reward, _, _ = env.step(torch.from_numpy(step).to(DEV), observe=False)
        earned[:, j] = _np(reward)
        at = length == j + 1                                   # these boards have played their plan
        pa, pb = env.raw_planes()
        final_v[at] = _np(T.ntuple_value((pa, pb), table, L, M))[at]
        final_state[at] = _state_of(_np(pb).view(np.uint32))[at]
    env.terminate()
    want = np.zeros(POOL, np.float32)
    for k in range(1, depth + 1):
        at = length == k
        if at.any():
            want[at] = m.ntuple_beam_values(earned[at, :k], final_state[at] != 0, final_v[at], GAMMA)
    bad = np.flatnonzero(_bits(want) != _bits(score))
    assert bad.size == 0, (bad[:5].tolist(), want[bad[:5]].tolist(), score[bad[:5]].tolist())
    assert (length == plies).sum() >= 100


# ------------------------------------------------------------------------------------------------ 4. UPDATE
def _trace(A, B, head, horizon, start, error, rate, decay, symmetric, form, staged=True, L=L, M=M):
    """The trace update of a host ring (uint32 [slots, n, 4] each) through canary-framed buffers: the table it leaves.  Staged: one
    tpl_ntuple_update_trace_staged; plain: tpl_ntuple_update_trace_shaped once per part."""
    slots, n = A.shape[:2]
    a, b, t, e = _framed(A, 1), _framed(B, 2), _framed(start, 3), _framed(error, 4)
    ring = (a.ptr(), b.ptr(), n, slots, head, horizon, L, M)
    tail = (e.ptr(), rate, decay, int(symmetric))
    if staged:
        _check(_lib().tpl_ntuple_update_trace_staged(*ring, t.ptr(), *tail, FORM_IDS[form], _stream()))
    else:
        for shape, at in PART_AT[form]:
            _check(_lib().tpl_ntuple_update_trace_shaped(*ring, t.ptr() + 4 * at, *tail, shape, _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("error", e)):
        f.assert_canary((n, slots, head, horizon, form, staged, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(e.host(), error.view(np.uint8))
    return t.host().view(np.int32).copy()


UPDATES = [(form, horizon, symmetric, LANES[(i + j + k) % 3]) for i, form in enumerate(FORMS) for j, horizon in enumerate((1, 4))
           for k, symmetric in enumerate((False, True))]
FOUR_MAP = (np.arange(1024) % 64 & 3).astype(np.int32) | np.int32(8)               # stage = moves left & 3, and a bit the mask drops


@pytest.mark.parametrize("form,horizon,symmetric,n", UPDATES)
def test_a_staged_update_leaves_the_mirror_bytes_the_map_and_the_unused_blocks(after, form, horizon, symmetric, n):
    assert {u[3] for u in UPDATES} == set(LANES)
    f, entries = after["fields"], FORMS[form]
    gen = np.random.default_rng(1000 * horizon + n + FORM_IDS[form])
    slots, head, rate, decay = horizon + 1, horizon // 2, 3000.0, 0.7
    picks = _picks(gen, after, (slots, n))
    A, B = _ring(after, picks)
    error = _errors(gen, n, rate)
    start = _blocks(400 + n, form, FOUR_MAP, span=(1 << 31) - 1)
    ages = [_age(f, picks[(head - k) % slots]) for k in range(horizon)]
    got = _trace(A, B, head, horizon, start, error, rate, decay, symmetric, form)
    want = _m().ntuple_update_trace(start.copy(), ages, L, M, error, rate, decay, symmetric)
    assert np.array_equal(got, want)
    assert np.array_equal(got[-1024:], FOUR_MAP)                                     # the map is read, never written
    changed = [bool((got[g * entries:(g + 1) * entries] != start[g * entries:(g + 1) * entries]).any()) for g in range(8)]
    assert changed == [True] * 4 + [False] * 4                                       # stages 4 .. 7: no state falls in them
    # the all-zero map: block 0 takes the bytes the plain update leaves on a plain table, the other blocks nothing
    zero = start.copy()
    zero[-1024:] = 0
    got0 = _trace(A, B, head, horizon, zero, error, rate, decay, symmetric, form)
    plain = _trace(A, B, head, horizon, np.ascontiguousarray(start[:entries]), error, rate, decay, symmetric, form, staged=False)
    assert np.array_equal(got0[:entries], plain) and np.array_equal(got0[entries:], zero[entries:]) and (plain != start[:entries]).any()
    # the boards in another order: the same bytes
    order = gen.permutation(n)
    assert np.array_equal(_trace(np.ascontiguousarray(A[:, order]), np.ascontiguousarray(B[:, order]), head, horizon, start,
                                 np.ascontiguousarray(error[order]), rate, decay, symmetric, form), got)


# ------------------------------------------------------------------------------------------------ 5. LEARNER
def _random_plain(form, seed, symmetric=False):
    t = np.random.default_rng(seed).integers(-(1 << 12), (1 << 12) + 1, FORMS[form]).astype(np.int32)
    return torch.from_numpy(t + t[_m().ntuple_mirror_permutation(form)] if symmetric else t).to(DEV)


@pytest.mark.parametrize("form", list(FORMS))
def test_promoted_under_the_all_zero_map_block_0_is_the_plain_learners_table(form):
    n, steps = 256, 40
    kw = dict(gamma=1.0, rate=16.0, epsilon=0.25, seed=5, shape=form, lam=0.8, horizon=4)
    start = _random_plain(form, 500)

    def run(**more):
        env = _carved_env(n)
        env.reset()
        learner = T.NTupleLearner(env, start=start, **kw, **more)
        assert learner.train(steps) == steps
        table = learner.table.clone()
        env.terminate()
        return table

    plain = run()
    staged = run(stage_map=torch.zeros(1024, dtype=torch.int32))
    assert tuple(plain.shape) == (FORMS[form],) and T.ntuple_is_staged(staged) and not torch.equal(plain, start)
    blocks = T.ntuple_stages(staged)
    assert torch.equal(blocks[0], plain) and all(torch.equal(b, start) for b in blocks[1:])
    assert int(T.ntuple_map(staged).abs().sum()) == 0


@pytest.mark.parametrize("form", list(FORMS))
def test_a_staged_learner_is_deterministic_stays_symmetric_and_evaluates_at_every_depth(form):
    n, steps = 256, 40

    def run():
        env = _carved_env(n)
        env.reset()
        four = T.ntuple_stage_map(env.L, env.M, moves=4)
        learner = T.NTupleLearner(env, gamma=1.0, rate=16.0, epsilon=0.25, seed=5, shape=form, lam=0.8, horizon=4, symmetric=True,
                                  stage_map=four, start=_random_plain(form, 600, symmetric=True))
        assert T.ntuple_is_symmetric(learner.table) and learner.policy.staged and learner.shape == form
        before = learner.table.clone()
        learner.train(steps)
        assert T.ntuple_is_symmetric(learner.table)            # every block, under four stages
        moved = [not torch.equal(x, y) for x, y in zip(T.ntuple_stages(learner.table), T.ntuple_stages(before))]
        assert moved == [True] * 4 + [False] * 4 and torch.equal(T.ntuple_map(learner.table).cpu(), four)
        table = learner.table.clone()
        results = [learner.evaluate(8), learner.evaluate(8, depth=2), learner.evaluate(8, depth=3, width=8)]
        assert all(r["episodes"] >= 0 and 0 <= r["wins"] <= max(r["episodes"], 1) for r in results)
        assert torch.equal(learner.table, table)               # evaluation trains nothing
        assert tuple(T.ntuple_value(env, learner.table).shape) == (n,)
        env.terminate()
        return table, results

    first, again = run(), run()
    assert torch.equal(first[0], again[0]) and first[1] == again[1]                   # one seed: the same bytes, the same games
