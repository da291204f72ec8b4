"""The two-ply n-tuple policy on one MI355X (include/tpl_learn.h's rule, tpl_ntuple_search in csrc/learn/ntuple.hip,
NTuplePolicy(depth=2), NTupleLearner(depth=2)), on test_afterstates_gpu's pool of 1,639 states at L = 10 / M = 40:

  1. ORACLE: on 200 evenly spread running states whose next piece is a real one, every distinct (a, b) is played as two moves of
     the C oracle (test_ntuple_search_cpu.TwoMoves); rewards and V(s2) come from the oracle's rows, lines, moves and the original
     window entry 2 through the numpy mirror; action, second and score are _learn_lib.ntuple_search_choice, bit for bit, for a
     random table and gamma = 1 and 0.99; the coverage conditions are asserted on the oracle's outcomes alone.
  2. PARENT KERNELS: on all 1,639 states (finished boards and next piece 7 among them) Q(a) = r1 + gamma * score' and second(a) =
     action' with r1 from tpl_afterstates and (score', action') from tpl_ntuple_act over the 40 n afterstates; after and value
     are tpl_afterstates' state of the action played and tpl_ntuple_value of it; n = 1, 7, 9, 63, 65 and the whole pool.
  3. ZERO TABLE: with reward (0, 1, 0), gamma = 1 and an all-zero table, action and second are tpl_placement_search's with
     win-only weights, and both scores are exactly `won`.
  4. EXPLORATION: epsilon = 1 and 0.25 play the predicted rank, on the boards tpl_ntuple_act explores at that (seed, step).
  5. STEP: after a non-auto-reset step with the action, the one-ply policy plays `second`.
  6. the policy object; 7. the solver property and the learner's determinism; 8. the argument refusals.
Canaries frame every buffer the kernel is handed.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, Pool, _resident
from test_heuristic_gpu import _planes
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_gpu import ENTRIES, GAMMA, PARAMS, _act, _framed, _random_table, _value
from test_ntuple_search_cpu import ARANGE, TwoMoves
from test_search_gpu import _search as _placement_search

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SUBSET = 200                                                   # of the 1,200-odd states the oracle can play two plies of
TPL_ERR_ARG = -1
OUTPUTS = dict(action=1, second=1, score=4, after_a=16, after_b=16, value=4)         # bytes per board


def _m():
    return T._learn_lib


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def _outputs(n):
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(OUTPUTS.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    return out


def _search(A, B, table, gamma=GAMMA, epsilon=0.0, seed=0, step=0, skip=(), params=PARAMS, L=L, M=M):
    """tpl_ntuple_search of host planes through canary-framed buffers; `skip` names the outputs passed as NULL ("after" = both)."""
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    out = _outputs(n)
    given = {k: f for k, f in out.items() if k not in skip and not (k in ("after_a", "after_b") and "after" in skip)}
    p = lambda k: given[k].ptr() if k in given else None
    _check(_lib().tpl_ntuple_search(a.ptr(), b.ptr(), n, L, M, *params, gamma, t.ptr(), epsilon, seed, step, p("action"), p("second"),
                                    p("score"), p("after_a"), p("after_b"), p("value"), _stream()))
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


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(got, want, what):
    for k, w in want.items():
        if k not in got:
            continue
        g, w = (_bits(got[k]), _bits(w)) if k in ("score", "value") else (got[k], w)
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, (what, k, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.fixture(scope="module")
def two(oracle, pool):
    f = pool.fields
    nxt = ((f["window"] >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
    idx = np.flatnonzero(pool.running & (nxt <= 6))            # the oracle has no piece 7
    assert idx.size >= 1000
    idx = idx[np.linspace(0, idx.size - 1, SUBSET).astype(np.int64)]
    t = TwoMoves(oracle, f["rows"][idx], np.asarray(f["lines"])[idx], np.asarray(f["moves"])[idx], f["window"][idx], L, M)
    t.idx = idx
    print(f"{SUBSET} states, {int(t.played.sum())} (a, b) pairs; the oracle's outcomes: {t.count}")
    # the coverage conditions, on the oracle's own outcomes (the whole pool gives at least 100 of each: test_search_gpu)
    assert set(t.nxt.tolist()) == set(range(7)) and set(t.third.tolist()) >= set(range(7))
    assert min(t.count.values()) >= 10, t.count
    return t


@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_the_search_is_two_oracle_moves_and_the_mirror_bit_for_bit(pool, two, gamma):
    table = _random_table(200)
    A, B = np.ascontiguousarray(pool.A[two.idx]), np.ascontiguousarray(pool.B[two.idx])
    action, second, score, Q, _ = _m().ntuple_search_choice(*two.inputs(table, PARAMS), gamma)
    got = _search(A, B, table, gamma=gamma)
    _same(got, dict(action=action, second=second, score=score), gamma)
    at = np.arange(SUBSET)
    went_on = second != 255
    assert two.distinct1[at, action].all() and np.array_equal(went_on, ~two.done1[at, action])
    assert two.distinct2[at[went_on], second[went_on]].all() and went_on.sum() >= 100 and (~went_on).any()
    assert len(set(action.tolist())) > 15 and len(set(second[went_on].tolist())) > 15
    if gamma == 1.0:                                           # each optional output left out once, and all of them
        for skip in ("second", "score", "after", "value"):
            other = _search(A, B, table, gamma=gamma, skip=(skip,))
            assert set(other) == set(got) - ({"after_a", "after_b"} if skip == "after" else {skip})
            for k, v in other.items():
                assert np.array_equal(v.view(np.uint8), got[k].view(np.uint8)), (skip, k)
        bare = _search(A, B, table, gamma=gamma, skip=("second", "score", "after", "value"))
        assert set(bare) == {"action"} and np.array_equal(bare["action"], action)
    else:                                                      # the discount reaches the score and, here and there, the choice
        other = _m().ntuple_search_choice(*two.inputs(table, PARAMS), 1.0)
        assert not np.array_equal(_bits(other[2]), _bits(score))


# ------------------------------------------------------------------------------------------------ 2. against the parent's kernels
class Composed:
    """The rule put together from the parent's kernels for the states (A, B): tpl_afterstates, then tpl_ntuple_act (epsilon = 0)
    and tpl_ntuple_value over the 40 n afterstates -- Q and second of every first placement, its afterstate and V of it."""

    def __init__(self, A, B, table, gamma, params=PARAMS, L=L, M=M):
        n = self.n = A.shape[0]
        a, b = _planes(A, B)
        out_a, out_b = Framed(n * 640, 3), Framed(n * 640, 4)
        reward, done, canonical = Framed(n * 160, 5), Framed(n * 40, 6), Framed(n * 40, 7)
        _check(_lib().tpl_afterstates(a.ptr(), b.ptr(), n, L, M, *params, out_a.ptr(), out_b.ptr(), reward.ptr(), done.ptr(), None,
                                      canonical.ptr(), _stream()))
        self.A = out_a.host().view(np.uint32).reshape(-1, 4).copy()
        self.B = out_b.host().view(np.uint32).reshape(-1, 4).copy()
        r1 = reward.host().view(np.float32).reshape(n, 40).copy()
        self.done1 = done.host().reshape(n, 40) != 0
        self.distinct = canonical.host().reshape(n, 40) == ARANGE[None, :]
        assert params == PARAMS                                # test_ntuple_gpu's _act plays with them
        ply = _act(self.A, self.B, table, gamma=gamma, skip=("after", "value"), L=L, M=M)
        self.value = _value(self.A, self.B, table, L=L, M=M).reshape(n, 40)
        self.running = ((B[:, 1] >> np.uint32(28)) & np.uint32(3)) == 0
        with np.errstate(invalid="ignore", over="ignore"):
            self.Q = np.where(self.done1, r1, r1 + np.float32(gamma) * ply["score"].reshape(n, 40)).astype(np.float32)
        self.second = np.where(self.done1, 255, ply["action"].reshape(n, 40)).astype(np.uint8)
        self.A, self.B = self.A.reshape(n, 40, 4), self.B.reshape(n, 40, 4)
        masked = np.where(self.distinct, self.Q, -np.inf)
        self.greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)       # the lowest index at the maximum

    def want(self, action=None):
        """The kernel's six outputs when `action` (default: the greedy one) is played."""
        at = np.arange(self.n)
        action = self.greedy if action is None else action
        return dict(action=action.astype(np.uint8), second=self.second[at, action], score=self.Q[at, self.greedy],
                    after_a=self.A[at, action], after_b=self.B[at, action], value=self.value[at, action])


@pytest.mark.parametrize("n", [1, 7, 9, 63, 65, POOL])
def test_the_search_is_the_one_ply_kernels_composed_on_every_state(pool, n):
    idx = pool.take(n, 0 if n == POOL else 13 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    table = _random_table(n)
    for gamma in (0.99, 1.0) if n == POOL else (0.99,):
        c = Composed(A, B, table, gamma)
        got = _search(A, B, table, gamma=gamma)
        _same(got, c.want(), (n, gamma))
        run = pool.running[idx]
        assert np.array_equal(c.running, run)
        assert (got["action"][~run] == 0).all() and (got["second"][~run] == 255).all() and (_bits(got["score"])[~run] == 0).all()
        assert np.array_equal(got["after_a"][~run], A[~run]) and np.array_equal(got["after_b"][~run], B[~run])
        assert (_bits(got["value"])[~run] == 0).all()
    if n == POOL:
        nxt = ((pool.fields["window"] >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
        assert (~run).sum() >= 100 and (run & (nxt == 7)).sum() >= 100
        ended = c.done1[np.arange(n), got["action"]] & run     # chosen first moves that end the game: no second, value 0
        assert ended.sum() >= 20 and (got["second"][ended] == 255).all() and (_bits(got["value"])[ended] == 0).all()
        assert (got["second"][run & ~ended] != 255).all() and (got["value"][run & ~ended] != 0).all()
        # two plies and one ply do not play the same game
        one = _act(A, B, table, gamma=1.0, skip=("after", "value"))
        assert (one["action"] != got["action"]).sum() >= 100


# ------------------------------------------------------------------------------------------------ 3. the zero table
def test_the_zero_table_with_a_win_only_reward_is_the_two_ply_heuristic_with_win_only_weights(pool):
    zero = np.zeros(ENTRIES, np.int32)
    got = _search(pool.A, pool.B, zero, gamma=1.0, params=(0.0, 1.0, 0.0))
    w = np.zeros(12, np.float32)
    w[1] = 1.0
    a, b = _planes(pool.A, pool.B)
    action, second, score = _placement_search(a, b, POOL, w, POOL)
    assert np.array_equal(got["action"], action) and np.array_equal(got["second"], second)
    assert np.array_equal(_bits(got["score"]), _bits(score))
    won = got["score"] == 1.0
    assert ((got["score"] == 0.0) | won).all() and won.sum() >= 50 and (~won).sum() >= 50
    assert (_bits(got["value"]) == 0).all()


# ------------------------------------------------------------------------------------------------ 4. exploration
@pytest.fixture(scope="module")
def composed(pool):
    table = _random_table(43)
    return table, Composed(pool.A, pool.B, table, GAMMA)


@pytest.mark.parametrize("epsilon", [1.0, 0.25])
def test_exploration_is_the_one_ply_draw_and_the_outputs_follow_the_move_played(pool, composed, epsilon):
    table, c = composed
    run = pool.running
    cur = (pool.fields["window"] & np.uint64(7)).astype(np.int64)
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    explores, j = _m().ntuple_explore(seed, step, POOL, epsilon, np.array(_m().PIECE_PLACEMENTS)[cur])
    explores &= run
    order = np.argsort(~c.distinct, axis=1, kind="stable")    # the distinct placements first, ascending
    action = np.where(explores, order[np.arange(POOL), j], c.greedy)
    got = _search(pool.A, pool.B, table, epsilon=epsilon, seed=seed, step=step)
    _same(got, c.want(action), epsilon)                        # score: the greedy maximum; second, after, value: the move played
    assert c.distinct[np.arange(POOL), got["action"]].all()
    moved = got["action"] != c.greedy
    assert moved.sum() > (0.5 if epsilon == 1.0 else 0.1) * run.sum() and not moved[~explores].any()
    greedy = c.want()
    assert (got["second"][moved] != greedy["second"][moved]).any() and (got["value"][moved] != greedy["value"][moved]).any()
    if epsilon == 1.0:
        assert explores[run].all() and len(set(got["action"][run].tolist())) >= 30
    else:
        frac = explores[run].mean()
        assert abs(frac - 0.25) <= 5.0 * np.sqrt(0.25 * 0.75 / run.sum()), frac
    # the same boards explore the same rank at both depths: tpl_ntuple_act at this (seed, step, epsilon)
    one = _act(pool.A, pool.B, table, epsilon=epsilon, seed=seed, step=step, skip=("score",))
    one_greedy = _act(pool.A, pool.B, table, skip=("score", "after", "value"))
    assert np.array_equal(one["action"][explores], got["action"][explores])
    assert np.array_equal(one["after_a"][explores], got["after_a"][explores])
    assert np.array_equal(one["after_b"][explores], got["after_b"][explores])
    assert np.array_equal(_bits(one["value"])[explores], _bits(got["value"])[explores])
    assert np.array_equal(one["action"][~explores], one_greedy["action"][~explores])
    # the same step, the same draw; another step, another draw
    again = _search(pool.A, pool.B, table, epsilon=epsilon, seed=seed, step=step, skip=("score", "after", "value"))
    other = _search(pool.A, pool.B, table, epsilon=epsilon, seed=seed, step=step + 1, skip=("score", "after", "value"))
    assert np.array_equal(again["action"], got["action"]) and np.array_equal(again["second"], got["second"])
    assert not np.array_equal(other["action"], got["action"])


# ------------------------------------------------------------------------------------------------ 5. against the step kernel
def _table_on_device(host):
    table = T.ntuple_table(DEV)
    table.copy_(torch.from_numpy(host))
    return table


def test_after_the_step_the_one_ply_policy_plays_second(pool):
    for gamma, seed in ((GAMMA, 50), (1.0, 51)):
        table = _table_on_device(_random_table(seed))
        env, idx = _resident(pool, POOL, 0, PARAMS)
        assert not env.auto_reset
        deep, shallow = T.NTuplePolicy(env, table, gamma=gamma, depth=2), T.NTuplePolicy(env, table, gamma=gamma, depth=1)
        second = torch.full((POOL,), 77, dtype=torch.uint8, device=DEV)
        action = deep.act(second=second)
        env.step(action, observe=False)
        _, b = env.raw_planes()
        running = ((_np(b).view(np.uint32)[:, 1] >> np.uint32(28)) & np.uint32(3)) == 0
        action1, second = _np(shallow.act()), _np(second)
        assert running.sum() >= 500 and (~running).sum() >= 200
        assert np.array_equal(action1[running], second[running]), gamma
        assert (second[~running] == 255).all(), gamma
        env.terminate()


# ------------------------------------------------------------------------------------------------ 6. the policy object
def test_the_policy_object_at_depth_two_and_depth_one_as_it_was(pool):
    n = 300
    env, idx = _resident(pool, n, 900, PARAMS)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    host = _random_table(6)
    table = _table_on_device(host)
    kw = dict(gamma=GAMMA, epsilon=0.25, seed=9)
    want = _search(A, B, host, epsilon=0.25, seed=9, step=4)
    policy = T.NTuplePolicy(env, table, depth=2, **kw)
    assert policy.depth == 2
    act = policy.act(step=4)
    assert act.dtype == torch.uint8 and tuple(act.shape) == (n,) and np.array_equal(_np(act), want["action"])
    policy.step = 4
    assert np.array_equal(_np(policy.act()), want["action"]) and policy.step == 5               # the policy's own counter
    out = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    second = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    score, value = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    planes = (torch.empty((n, 4), dtype=torch.int32, device=DEV), torch.empty((n, 4), dtype=torch.int32, device=DEV))

    def outputs():
        return dict(action=_np(out), second=_np(second), score=_np(score), value=_np(value),
                    after_a=_np(planes[0]).view(np.uint32), after_b=_np(planes[1]).view(np.uint32))

    assert policy.act(out=out, score=score, after=planes, value=value, step=4, second=second) is out
    _same(outputs(), want, "policy")
    with pytest.raises(ValueError, match="second"):
        policy.act(second=torch.empty(n + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="second"):
        policy.act(second=torch.empty(n, dtype=torch.int32, device=DEV))
    # captured into a graph: one launch, no allocation, no host sync; the table is read at every replay
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            policy.act(out=out, score=score, after=planes, value=value, step=4, second=second)
    other = _random_table(7)
    where = table.data_ptr()
    table.copy_(torch.from_numpy(other))                       # in place
    assert table.data_ptr() == where
    for t in (out, second):
        t.fill_(99)
    graph.replay()
    torch.cuda.synchronize()
    replayed = _search(A, B, other, epsilon=0.25, seed=9, step=4)
    _same(outputs(), replayed, "replayed")
    assert (replayed["action"] != want["action"]).any()
    pa, pb = env.raw_planes()                                  # act() leaves the environment's planes untouched
    assert np.array_equal(_np(pa).view(np.uint32), A) and np.array_equal(_np(pb).view(np.uint32), B)
    # depth 1: the default, and tpl_ntuple_act as it was
    one = _act(A, B, other, epsilon=0.25, seed=9, step=4)
    for shallow in (T.NTuplePolicy(env, table, **kw), T.NTuplePolicy(env, table, depth=1, **kw)):
        assert shallow.depth == 1
        assert shallow.act(out=out, score=score, after=planes, value=value, step=4) is out
        got = outputs()
        for k, v in one.items():
            assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), k
        with pytest.raises(ValueError, match="second"):
            shallow.act(second=second)
    env.terminate()


# ------------------------------------------------------------------------------------------------ 7. the solver and the learner
def test_two_plies_solve_the_two_piece_game_with_the_zero_table_and_training_is_deterministic():
    """L = 2 / M = 2 over 64 carved configurations, win-only reward: both pieces are visible at reset, so the zero table wins
    every episode at two plies; at one ply it plays the best immediate reward and wins about one in six (the recorded run:
    6,060 of 34,143)."""
    n, steps = 4096, 16
    carved = T.generate_configs(2, 2, 64, seed=107)

    def make(depth):
        env = T.BatchedTetris(2, 2, n, device=DEV, seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)
        return env, T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.25, seed=5, depth=depth)

    env, learner = make(1)
    deep, shallow = learner.evaluate(steps, depth=2), learner.evaluate(steps, depth=1)
    assert learner.evaluate(steps) == shallow and int(learner.table.abs().sum()) == 0
    env.terminate()
    print(f"the zero table at depth 2: {deep}; at depth 1: {shallow}")
    assert deep["episodes"] >= n * steps // 2 // 2 and deep["wins"] == deep["episodes"]
    assert shallow["episodes"] >= n * steps // 2 // 2 and shallow["wins"] < shallow["episodes"]
    tables = []
    for _ in range(2):
        env, learner = make(2)
        assert learner.depth == 2 and learner.policy.depth == 2 and learner.greedy.depth == 2
        assert learner.evaluate(steps) == deep                 # None: the learner's own depth
        assert learner.train(20) == 20
        tables.append(learner.table.clone())
        env.terminate()
    assert torch.equal(tables[0], tables[1]) and int((tables[0] != 0).sum()) > 0


# ------------------------------------------------------------------------------------------------ 8. the argument refusals
def test_every_refusal_is_a_status_and_leaves_the_outputs_untouched(pool):
    n = 16
    A, B = np.ascontiguousarray(pool.A[:n]), np.ascontiguousarray(pool.B[:n])
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(np.zeros(ENTRIES, np.int32), 3)
    out = _outputs(n)
    nan, inf = float("nan"), float("inf")
    limit = -(-(1 << 31) // 40)                                # the first n with 40 n >= 2^31

    def call(**kw):
        arg = dict(a=a.ptr(), b=b.ptr(), n=n, L=L, M=M, gamma=GAMMA, table=t.ptr(), epsilon=0.1, **{k: f.ptr() for k, f in out.items()})
        arg.update(kw)
        return _lib().tpl_ntuple_search(arg["a"], arg["b"], arg["n"], arg["L"], arg["M"], *PARAMS, arg["gamma"], arg["table"],
                                        arg["epsilon"], 1, 2, arg["action"], arg["second"], arg["score"], arg["after_a"],
                                        arg["after_b"], arg["value"], _stream())

    cases = [dict(action=None), dict(after_a=None), dict(after_b=None), dict(after_a=out["after_a"].ptr() + 8),
             dict(after_b=out["after_b"].ptr() + 4), dict(score=out["score"].ptr() + 2), dict(value=out["value"].ptr() + 1),
             dict(a=None), dict(b=a.ptr() + 8), dict(table=None), dict(table=t.ptr() + 4)]
    cases += [dict(epsilon=e) for e in (-0.001, 1.001, nan, inf, -inf)] + [dict(gamma=g) for g in (nan, inf, -inf)]
    cases += [dict(L=0), dict(L=251), dict(L=-1), dict(M=0), dict(M=255), dict(n=0), dict(n=-1), dict(n=limit), dict(n=1 << 40)]
    for kw in cases:
        assert call(**kw) == TPL_ERR_ARG, kw
        assert b"tpl_ntuple_search" in _lib().tpl_learn_last_error(), kw
    torch.cuda.synchronize()
    for k, f in out.items():
        f.assert_canary(k)
        assert (f.host() == 0xCD).all(), k
    # the same buffers are good for a call that is not refused; `second` may sit at any address
    odd = Framed(n + 1, 9)
    odd.inner().fill_(0xCD)
    _check(call(second=odd.ptr() + 1))
    torch.cuda.synchronize()
    odd.assert_canary("odd second")
    want = _search(A, B, np.zeros(ENTRIES, np.int32), epsilon=0.1, seed=1, step=2)
    assert np.array_equal(odd.host()[1:], want["second"]) and odd.host()[0] == 0xCD
    assert np.array_equal(out["action"].host(), want["action"]) and (out["second"].host() == 0xCD).all()
