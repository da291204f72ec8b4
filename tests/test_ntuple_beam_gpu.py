"""The n-tuple beam search on one MI355X (include/tpl_learn.h's rule, tpl_ntuple_beam in csrc/learn/ntuple_beam.hip,
NTupleBeamPolicy, NTupleLearner.evaluate(depth, width)).  The states are the 1,639 of test_afterstates_gpu's pool (L = 10, M = 40:
random windows with piece 7 among them, moves in {8, 9, 18, 19}, finished boards, boards near L and M); the table is random in
+-2^20 for each shape; gamma and the reward parameters are test_ntuple_gpu's.

  1. PARENT KERNELS, exact: depth 1 at any width is tpl_ntuple_act_shaped (action, score, after), depth 2 at width >= 34 is
     tpl_ntuple_search_shaped (action, score) with plan[1] <= second, through canary-framed buffers, each optional output left out
     once, the planes and the table untouched.
  2. REFERENCE BEAM, built without the kernel under test: every ply is T.afterstates on the current beam's planes, V from
     T.ntuple_value on the children (once from the numpy mirror), _learn_lib.ntuple_beam_values and ntuple_beam_ply; action, plan
     and score bit for bit.
  3. COVERAGE of the reference's own outcomes.
  4. THE PLAN IS PLAYABLE: stepping plan[:, j] on the environment earns rewards and reaches a board whose fold is `score`.
  5. the policy object, a captured graph, the two-piece game and evaluate(depth, width).
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, _i32, _resident
from test_beam_gpu import States
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_gpu import GAMMA, PARAMS, _fields, _framed, _mirror_value
from test_ntuple_shape_gpu import _policy3

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARANGE = np.arange(40)
SHAPES = ("2x4", "3x3")
OUTPUTS = dict(action=1, plan=None, score=4, after_a=16, after_b=16)             # bytes per board; plan: depth


def _m():
    return T._learn_lib


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def states():
    return States()


@pytest.fixture(scope="module")
def tables():
    gen = np.random.default_rng(2176)
    return {s: gen.integers(-(1 << 20), (1 << 20) + 1, _m().NTUPLE_SHAPES[s][2]).astype(np.int32) for s in SHAPES}


@pytest.fixture(scope="module")
def env10():
    """Any L = 10 / M = 40 environment with the reward parameters: T.afterstates reads L, M and the rewards from it."""
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=9, reward=PARAMS)
    yield env
    env.terminate()


def effective(states, idx, depth):
    """The effective depth of every state: 0 where it is finished, else min(depth, 11 - moves mod 10)."""
    return np.where(states.running[idx], np.minimum(depth, 11 - states.moves[idx] % 10), 0)


def _beam(A, B, table, depth, width, gamma=GAMMA, skip=(), params=PARAMS, L=L, M=M):
    """tpl_ntuple_beam of host planes through canary-framed buffers; `skip` names the outputs passed as NULL ("after" = both)."""
    n = A.shape[0]
    shape = _m().NTUPLE_SHAPE_IDS[_m().ntuple_shape_of(table.shape[0])]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    out = {k: Framed((depth if size is None else size) * n, 4 + j) for j, (k, size) in enumerate(OUTPUTS.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    given = {k: f for k, f in out.items() if k not in skip and not (k in ("after_a", "after_b") and "after" in skip)}
    p = lambda k: given[k].ptr() if k in given else None
    _check(_lib().tpl_ntuple_beam(a.ptr(), b.ptr(), n, L, M, *params, gamma, t.ptr(), depth, width, p("action"), p("plan"), p("score"),
                                  p("after_a"), p("after_b"), shape, _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((n, depth, width, skip, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(t.host().view(np.int32), table)      # the planes and the table are read only
    for k, f in out.items():                                   # an output that was not given is not written
        if k not in given:
            assert (f.host() == 0xCD).all(), (skip, k)
    host = {k: f.host().copy() for k, f in given.items()}
    for k in ("after_a", "after_b"):
        if k in host:
            host[k] = host[k].view(np.uint32).reshape(n, 4)
    if "plan" in host:
        host["plan"] = host["plan"].reshape(n, depth)
    if "score" in host:
        host["score"] = host["score"].view(np.float32)
    return host


def _same(got, want, what):
    for k, w in want.items():
        if k not in got:
            continue
        g, w = (_bits(got[k]), _bits(w)) if k == "score" else (got[k], np.asarray(w))
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, (what, k, bad.size, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


# ------------------------------------------------------------------------------------------------ 1. the parent's kernels
def _folded_second(env, table, A, B, action, b2, gamma, L=L, M=M):
    """r1 + gamma * (r2 + gamma * V) of first placement `action` and second placement `b2` for every state, by T.afterstates and
    T.ntuple_value: what the beam calls the folded value of the path (action, b2)."""
    n = A.shape[0]
    at = np.arange(n)
    first = T.afterstates(env, _i32(A).to(DEV), _i32(B).to(DEV))
    r1 = _np(first["reward"])[at, action]
    sa, sb = first["states_a"][at, action].contiguous(), first["states_b"][at, action].contiguous()
    second = T.afterstates(env, sa, sb)
    r2, done2 = _np(second["reward"])[at, b2], _np(second["done"])[at, b2] != 0
    ta, tb = second["states_a"][at, b2].contiguous(), second["states_b"][at, b2].contiguous()
    v = _np(T.ntuple_value((ta, tb), torch.from_numpy(table).to(DEV), L, M))
    return _m().ntuple_beam_values(np.stack([r1, r2], axis=1), done2, v, gamma)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 13, 257, POOL])
def test_depth_one_is_the_act_kernel_and_depth_two_at_full_width_is_the_search_kernel(states, tables, env10, n, shape):
    idx = states.take(n, 0 if n == POOL else 7 * n)
    A, B = np.ascontiguousarray(states.A[idx]), np.ascontiguousarray(states.B[idx])
    run = states.running[idx]
    table, sid = tables[shape], _m().NTUPLE_SHAPE_IDS[shape]
    one = _policy3(1, A, B, table, shape=sid)
    for width in (1, 5, 64):
        got = _beam(A, B, table, 1, width)
        _same(got, {k: one[k] for k in ("action", "score", "after_a", "after_b")}, (n, shape, 1, width))
        assert (got["plan"][:, 0] == np.where(run, one["action"], 255)).all()
    two = _policy3(2, A, B, table, shape=sid)
    for width in (34, 35, 64):
        got = _beam(A, B, table, 2, width)
        _same(got, {k: two[k] for k in ("action", "score", "after_a", "after_b")}, (n, shape, 2, width))
        assert (got["plan"][:, 0] == np.where(run, two["action"], 255)).all()
        # plan[1] is the lowest b whose folded value is the score, second the lowest b at the maximum of q: plan[1] <= second
        assert (got["plan"][:, 1] <= two["second"]).all() and ((got["plan"][:, 1] == 255) == (two["second"] == 255)).all()
    differ = np.flatnonzero(got["plan"][:, 1] != two["second"])
    print(f"n = {n}, {shape}: plan[1] differs from second on {differ.size} boards")
    if differ.size:                                            # two different q that round to one Q
        args = (env10, table, A[differ], B[differ], two["action"][differ])
        by_plan = _folded_second(*args, got["plan"][differ, 1], GAMMA)
        by_second = _folded_second(*args, two["second"][differ], GAMMA)
        assert np.array_equal(_bits(by_plan), _bits(got["score"][differ])) and np.array_equal(_bits(by_second), _bits(by_plan))
    assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all() and (_bits(got["score"][~run]) == 0).all()
    assert np.array_equal(got["after_a"][~run], A[~run]) and np.array_equal(got["after_b"][~run], B[~run])
    want = _beam(A, B, table, 2, 34)
    for skip in ("plan", "score", "after"):                    # each optional output left out once, and all of them
        other = _beam(A, B, table, 2, 34, skip=(skip,))
        assert set(other) == set(want) - ({"after_a", "after_b"} if skip == "after" else {skip})
        for k, v in other.items():
            assert np.array_equal(v.view(np.uint8), want[k].view(np.uint8)), (skip, k)
    bare = _beam(A, B, table, 2, 34, skip=("plan", "score", "after"))
    assert set(bare) == {"action"} and np.array_equal(bare["action"], want["action"])
    if n == POOL:
        assert (~run).sum() >= 100 and (two["action"] != one["action"]).any()


# ------------------------------------------------------------------------------------------------ 2. the reference beam
def _state_of(B):
    return (B[..., 1] >> np.uint32(28)) & np.uint32(3)


def compose(env, table, A, B, plies, depth, width, gamma=GAMMA, mirror_value=False, L=L, M=M):
    """The rule without the kernel under test: every ply is T.afterstates on the beam's planes, V of the children from
    T.ntuple_value (mirror_value: from _learn_lib.ntuple_value on the decoded children), the numpy fold and ntuple_beam_ply.
    A, B uint32 [n, 4], plies [n] the effective depth of every state.  Returns action, plan, score and what the coverage counts."""
    m = _m()
    n = A.shape[0]
    dev_table = torch.from_numpy(table).to(DEV)
    nodeA, nodeB = A[:, None, :].copy(), B[:, None, :].copy()
    value = np.zeros((n, 1), np.float32)
    rewards = np.zeros((n, 1, depth), np.float32)              # r_1 .. r_j of a node's path
    path = np.full((n, 1, depth), 255, np.uint8)
    size = np.ones(n, np.int64)                                # the nodes of a beam are a prefix
    edge_tie = np.zeros(n, bool)
    carried = np.zeros(n, bool)
    for j in range(int(plies.max(initial=0))):
        act = np.flatnonzero(plies > j)
        k, wc = act.size, nodeA.shape[1]
        pa, pb = (_i32(x[act].reshape(-1, 4)).to(DEV) for x in (nodeA, nodeB))
        after = T.afterstates(env, pa, pb)
        sa, sb = after["states_a"].view(-1, 4), after["states_b"].view(-1, 4)
        if mirror_value:
            v = _mirror_value(table, _fields(_np(sa).view(np.uint32), _np(sb).view(np.uint32)), L=L, M=M)
        else:
            v = _np(T.ntuple_value((sa, sb), dev_table, L, M))
        sa, sb = (_np(x).view(np.uint32).reshape(k, wc, 40, 4) for x in (sa, sb))
        reward = _np(after["reward"]).reshape(k, wc, 40)
        ended = _np(after["done"]).reshape(k, wc, 40) != 0
        distinct = _np(after["canonical"]).reshape(k, wc, 40) == ARANGE
        run = _state_of(nodeB[act]) == 0                       # [k, wc]
        before = np.broadcast_to(rewards[act][:, :, None, :j], (k, wc, 40, j))
        folded = m.ntuple_beam_values(np.concatenate([before, reward[..., None]], axis=3).reshape(-1, j + 1), ended.reshape(-1),
                                      v.reshape(-1), gamma).reshape(k, wc, 40)
        keep = []
        for t, s in enumerate(act):
            live = int(size[s])
            keep.append(m.ntuple_beam_ply(value[s, :live], run[t, :live], folded[t, :live], distinct[t, :live], width))
            cand = np.where(run[t, :live, None], distinct[t, :live], ARANGE == 0)
            listed = np.where(run[t, :live, None], folded[t, :live], value[s, :live, None])[cand]
            if listed.size > width:
                ranked = np.sort(listed + np.float32(0.0))[::-1]
                edge_tie[s] |= ranked[width - 1] == ranked[width]
        wn = max(wc, max(q.size for q, _, _ in keep))
        grown = lambda x, fill: np.concatenate([x, np.full((n, wn - wc) + x.shape[2:], fill, x.dtype)], axis=1)
        nodeA, nodeB, value, rewards, path = (grown(x, f) for x, f in ((nodeA, 0), (nodeB, 0), (value, 0), (rewards, 0), (path, 255)))
        for t, s in enumerate(act):
            q, b, val = keep[t]
            moved = b != 255
            carried[s] |= bool((~moved).any())
            b0 = np.where(moved, b, 0)
            new_path, new_rewards = path[s, q].copy(), rewards[s, q].copy()
            new_path[moved, j] = b[moved]
            new_rewards[moved, j] = reward[t, q, b0][moved]
            nodeA[s, :q.size], nodeB[s, :q.size] = sa[t, q, b0], sb[t, q, b0]          # a finished board's afterstate is itself
            value[s, :q.size], path[s, :q.size], rewards[s, :q.size] = val, new_path, new_rewards
            size[s] = q.size
    at = np.arange(n)
    best = np.array([m.beam_select(value[s, :size[s]], 1)[0] for s in range(n)], np.int64)
    end = _state_of(nodeB)
    live = np.arange(nodeA.shape[1])[None, :] < size[:, None]
    return dict(action=np.where(plies > 0, path[at, best, 0], 0).astype(np.uint8), plan=path[at, best], score=value[at, best],
                carried=carried, won=((end == 1) & live & (plies > 0)[:, None]).any(axis=1),
                lost=((end >= 2) & live & (plies > 0)[:, None]).any(axis=1), edge_tie=edge_tie)


class Reference:
    """compose() of the pool's first `n` states, once per (shape, depth, width, n)."""

    def __init__(self, states, env, tables):
        self.states, self.env, self.tables, self.memo = states, env, tables, {}

    def get(self, shape, depth, width, n=POOL):
        key = (shape, depth, width, n)
        if key not in self.memo:
            s = self.states
            idx = np.arange(n)
            self.memo[key] = compose(self.env, self.tables[shape], s.A[idx], s.B[idx], effective(s, idx, depth), depth, width)
        return self.memo[key]


@pytest.fixture(scope="module")
def reference(states, env10, tables):
    return Reference(states, env10, tables)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("depth,width,n", [(3, 1, POOL), (3, 8, POOL), (2, 5, POOL), (4, 16, 257), (6, 16, 257), (11, 64, 257)])
def test_the_beam_is_the_reference_composed_ply_by_ply(states, reference, tables, depth, width, n, shape):
    want = reference.get(shape, depth, width, n)
    A, B = np.ascontiguousarray(states.A[:n]), np.ascontiguousarray(states.B[:n])
    got = _beam(A, B, tables[shape], depth, width)
    _same(got, dict(action=want["action"], plan=want["plan"], score=want["score"]), (shape, depth, width))
    run = states.running[:n]
    plies = effective(states, np.arange(n), depth)
    assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all()
    assert (got["plan"][run, 0] == got["action"][run]).all() and (got["action"][run] < 40).all()
    assert ((got["plan"] != 255).sum(axis=1) <= plies).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_the_reference_with_the_value_from_the_numpy_mirror(states, env10, tables, shape):
    n = 13
    idx = states.take(n, 7 * n)
    A, B = np.ascontiguousarray(states.A[idx]), np.ascontiguousarray(states.B[idx])
    want = compose(env10, tables[shape], A, B, effective(states, idx, 3), 3, 8, mirror_value=True)
    _same(_beam(A, B, tables[shape], 3, 8), dict(action=want["action"], plan=want["plan"], score=want["score"]), shape)


# ------------------------------------------------------------------------------------------------ 3. coverage
def test_the_reference_covers_what_the_rule_distinguishes(states, reference):
    """Counted on the reference's own outcomes.  The floors: the pool holds every kind of state some 200 times (one kind in eight
    of 1,639), so an outcome that a kind of state brings about is asked for on at least one board, and the two the issue puts a
    number to -- a width and a depth that change the choice -- on at least 100."""
    narrow, wide, two, three = (reference.get("2x4", *key) for key in ((3, 1), (3, 8), (2, 5), (3, 5)))
    deep = reference.get("2x4", 11, 64, 257)
    run = states.running
    depths = effective(states, np.arange(POOL), 11)
    count = dict(depth_2=int((run & (depths == 2)).sum()), depth_3=int((run & (depths == 3)).sum()),
                 depth_11=int((run & (depths == 11)).sum()), depth_11_searched=int((effective(states, np.arange(257), 11) == 11).sum()),
                 carried=int(wide["carried"].sum() + deep["carried"].sum()),
                 won_inside=int(wide["won"].sum()), lost_inside=int(wide["lost"].sum()),
                 width_matters=int((narrow["action"] != wide["action"]).sum()),
                 depth_matters=int((three["action"] != two["action"]).sum()),
                 edge_ties=int(wide["edge_tie"].sum() + two["edge_tie"].sum()))
    print("coverage of the reference's outcomes:", count)
    assert min(count.values()) >= 1, count
    assert count["width_matters"] >= 100 and count["depth_matters"] >= 100, count


# ------------------------------------------------------------------------------------------------ 4. the plan is playable
@pytest.mark.parametrize("shape,depth,width", [("2x4", 3, 4), ("3x3", 11, 8)])
def test_playing_the_plan_earns_the_rewards_and_reaches_the_board_that_fold_to_the_score(states, tables, shape, depth, width):
    m = _m()
    env, idx = _resident(states, POOL, 0, PARAMS)
    assert not env.auto_reset and env.pool_info()["n_configs"] == 0              # no pool: no refill, the rule's pop
    table = torch.from_numpy(tables[shape]).to(DEV)
    policy = T.NTupleBeamPolicy(env, table, depth, width, gamma=GAMMA)
    score = torch.empty(POOL, dtype=torch.float32, device=DEV)
    plan = torch.full((POOL, depth), 77, dtype=torch.uint8, device=DEV)
    action = policy.act(score=score, plan=plan)
    plan, score = _np(plan), _np(score)
    assert np.array_equal(_np(action), np.where(states.running, plan[:, 0], 0))
    plies = effective(states, idx, depth)
    length = (plan != 255).sum(axis=1)
    assert (length <= plies).all() and (length[states.running] >= 1).all() and (plan[np.arange(depth)[None, :] >= length[:, None]] == 255).all()
    earned = np.zeros((POOL, depth), np.float32)
    final_v, final_state = np.zeros(POOL, np.float32), _state_of(states.B).astype(np.int64)
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
    assert bad.size == 0, (shape, depth, width, bad[:5].tolist(), want[bad[:5]].tolist(), score[bad[:5]].tolist())
    # a plan ends where the game ends or the known pieces do
    assert ((length == plies) | (final_state != 0)).all() and (length == plies).sum() >= 100 and (length < plies).sum() >= 1


# ------------------------------------------------------------------------------------------------ 5. the policy object
def test_the_policy_object_and_a_captured_graph(states, tables):
    n = 300
    env, idx = _resident(states, n, 900, PARAMS)
    A, B = np.ascontiguousarray(states.A[idx]), np.ascontiguousarray(states.B[idx])
    table = torch.from_numpy(tables["3x3"]).to(DEV)
    policy = T.NTupleBeamPolicy(env, table, 3, 4, gamma=GAMMA)
    assert (policy.depth, policy.width, policy.shape, policy.env) == (3, 4, "3x3", env)
    want = _beam(A, B, tables["3x3"], 3, 4)
    act = policy.act()
    assert act.dtype == torch.uint8 and tuple(act.shape) == (n,) and np.array_equal(_np(act), want["action"])
    out = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    plan = torch.full((n, 3), 77, dtype=torch.uint8, device=DEV)
    score = torch.empty(n, dtype=torch.float32, device=DEV)
    after = tuple(torch.empty((n, 4), dtype=torch.int32, device=DEV) for _ in range(2))

    def outputs():
        return dict(action=_np(out), plan=_np(plan), score=_np(score), after_a=_np(after[0]).view(np.uint32),
                    after_b=_np(after[1]).view(np.uint32))
    assert policy.act(out=out, score=score, plan=plan, after=after) is out
    _same(outputs(), want, "policy")
    with pytest.raises(ValueError, match="plan"):
        policy.act(plan=torch.empty((n, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="after"):
        policy.act(after=(after[0], after[1][:-1]))
    # captured into a graph: one launch, no allocation, no host sync; the table is read at every replay
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            policy.act(out=out, score=score, plan=plan, after=after)
    other = np.random.default_rng(5).integers(-(1 << 20), (1 << 20) + 1, tables["3x3"].shape[0]).astype(np.int32)
    table.copy_(torch.from_numpy(other).to(DEV))
    for t in (out, plan):
        t.fill_(99)
    graph.replay()
    torch.cuda.synchronize()
    _same(outputs(), _beam(A, B, other, 3, 4), "replayed")
    assert (_np(out) != want["action"]).any()
    pa, pb = env.raw_planes()                                  # act() leaves the environment's planes untouched
    assert np.array_equal(_np(pa).view(np.uint32), A) and np.array_equal(_np(pb).view(np.uint32), B)
    env.terminate()


def test_the_two_piece_game_is_solved_at_depth_three_and_a_trained_table_gains_from_the_beam():
    """test_ntuple_gpu's two-piece game (L = 2, M = 2, 64 carved configurations, reward (0, 1, 0), gamma 1): an episode is two
    moves, so a zero table under a search of two plies or more wins every episode; after 300 steps of training a beam of three
    plies wins at least what one ply of the same table wins."""
    n, EVAL = 4096, 16
    carved = T.generate_configs(2, 2, 64, seed=107)
    env = T.BatchedTetris(2, 2, n, device=DEV, seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)
    learner = T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.25, seed=5)
    beam, search = learner.evaluate(EVAL, depth=3, width=64), learner.evaluate(EVAL, depth=2)
    print("zero table: depth 3 x 64", beam, "depth 2", search)
    assert int(learner.table.abs().sum()) == 0
    assert beam["episodes"] >= n * EVAL // 2 // 2 and beam["wins"] == beam["episodes"]
    assert search["wins"] == search["episodes"] == beam["episodes"]
    learner.train(300)
    table = learner.table.clone()
    deep, again, one = learner.evaluate(EVAL, depth=3, width=8), learner.evaluate(EVAL, depth=3, width=8), learner.evaluate(EVAL, depth=1)
    print("after 300 steps: depth 3 x 8", deep, "depth 1", one)
    assert deep == again and torch.equal(table, learner.table)                   # deterministic, and evaluation trains nothing
    assert deep["episodes"] >= n * EVAL // 2 // 2 and deep["wins"] >= one["wins"]
    assert learner.evaluate(EVAL) == one                       # width=None is the interface as it was
    with pytest.raises(ValueError, match="depth"):
        learner.evaluate(EVAL, width=8)
    env.terminate()
