"""The beam search over the known piece window on one MI355X (include/tpl_learn.h's rule, tpl_placement_beam, BeamPolicy,
evaluate_heuristic / tune_heuristic with a width).  The states are the 1,639 of test_afterstates_gpu's pool (L = 10, M = 40:
random windows with piece 7 among them, moves in {8, 9, 18, 19}, finished boards, boards near L and M).

  1. PARENT KERNELS, exact: depth 1 at any width is tpl_placement_act, depth 2 at width >= 34 is tpl_placement_search, bit for
     bit, through canary-framed buffers, each optional output left out once, the planes untouched.
  2. REFERENCE BEAM composed from the parent's kernels: every ply is T.afterstates and T.placement_features on the current
     beam's planes, the cleared rows accumulated, placement_score and beam_select; action, plan and score bit for bit.
  3. ORACLE: the same reference with every move played by the C oracle and the features from _learn_lib.board_features.
  4. COVERAGE of the reference's own outcomes: clamped depths, finished nodes carried, wins inside the beam, widths and depths
     that change the choice, ties at the W-th place.
  5. THE PLAN IS PLAYABLE: stepping plan[:, j] on the environment reaches a board that scores `score`.
  6. the policy object, a captured graph, evaluate_heuristic and tune_heuristic with a width.
"""
import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from conftest import load_golden
from test_afterstates_gpu import L, M, POOL, REWARDS, _i32, _pool_fields, _resident
from test_heuristic_gpu import _act, _planes, _weight_sets
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_search_gpu import _search

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NF = 12
ARANGE = np.arange(40)
WEIGHT_SETS = _weight_sets()
RANDOM, SMALL, CLASSICAL = WEIGHT_SETS[0][1], WEIGHT_SETS[2][1], WEIGHT_SETS[4][1]
assert WEIGHT_SETS[2][0] == "small integers" and WEIGHT_SETS[4][0] == "the classical signs"


def _m():
    return T._learn_lib


class States:
    """The pool's states and planes (test_afterstates_gpu's generator and seed), without the oracle's outcomes."""

    def __init__(self, fields=None):
        f = self.fields = _pool_fields(np.random.default_rng(1639)) if fields is None else fields
        self.n = len(f["lines"])
        self.A, self.B = R.pack_state(f["rows"], f["lines"], f["moves"], f["state"], f["slot"], f["window"])
        self.B[:, 1] |= f["spare"] << np.uint32(31)
        self.running = np.asarray(f["state"]) == 0
        self.moves = np.asarray(f["moves"]).astype(np.int64)
        self.known = 12 - self.moves % 10                      # the true pieces a window holds

    def take(self, n, offset):
        return (offset + np.arange(n)) % self.n

    def plies(self, idx, depth):
        return np.where(self.running[idx], np.minimum(depth, self.known[idx]), 0)


@pytest.fixture(scope="module")
def states():
    return States()


@pytest.fixture(scope="module")
def env10():
    """Any L = 10 / M = 40 environment: T.afterstates and T.placement_features read L and M from it."""
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=9, reward=REWARDS[0])
    yield env
    env.terminate()


def _beam(a, b, n, weights, per, depth, width, skip=None, L=L, M=M):
    """tpl_placement_beam through canary-framed buffers; `skip` names the optional output passed as NULL."""
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, NF)
    wf = Framed(w.size * 4, 5)
    wf.inner().copy_(torch.from_numpy(w.view(np.uint8).reshape(-1)))
    action, plan, score = Framed(n, 6), Framed(n * depth, 7), Framed(n * 4, 8)
    for f in (action, plan, score):
        f.inner().fill_(0xCD)
    _check(_lib().tpl_placement_beam(a.ptr(), b.ptr(), n, L, M, wf.ptr(), per, depth, width, action.ptr(),
                                     None if skip == "plan" else plan.ptr(), None if skip == "score" else score.ptr(), _stream()))
    for name, f in (("action", action), ("plan", plan), ("score", score), ("weights", wf), ("a", a), ("b", b)):
        f.assert_canary((n, per, depth, width, skip, name))
    assert np.array_equal(wf.host(), w.view(np.uint8).reshape(-1))
    if skip == "plan":
        assert (plan.host() == 0xCD).all()                     # an output that was not given is not written
    if skip == "score":
        assert (score.host() == 0xCD).all()
    return action.host().copy(), plan.host().reshape(n, depth).copy(), score.host().view(np.float32).copy()


def _same(got, want, what, skip=None):
    for name, g, w in zip(("action", "plan", "score"), got, want):
        if name == skip:
            continue
        g, w = (g.view(np.uint32), w.view(np.uint32)) if name == "score" else (g, w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------ 1. the parent's kernels
@pytest.mark.parametrize("n", [1, 2, 13, POOL])
def test_depth_one_is_the_act_kernel_and_depth_two_at_full_width_is_the_search_kernel(states, n):
    idx = states.take(n, 0 if n == POOL else 7 * n)
    a, b = _planes(states.A[idx], states.B[idx])
    run = states.running[idx]
    for name, w in (("random", RANDOM), ("small integers", SMALL), ("classical", CLASSICAL)):
        act1, score1 = _act(a, b, n, w, n)
        for width in (1, 5, 64):
            got = _beam(a, b, n, w, n, 1, width)
            _same((got[0], got[2]), (act1, score1), (n, name, 1, width))
            assert (got[1][:, 0] == np.where(run, act1, 255)).all()
        act2, second, score2 = _search(a, b, n, w, n)
        for width in (34, 35, 64):
            got = _beam(a, b, n, w, n, 2, width)
            _same((got[0], got[1][:, 1], got[2]), (act2, second, score2), (n, name, 2, width))
            assert (got[1][:, 0] == np.where(run, act2, 255)).all()
        assert (got[0][~run] == 0).all() and (got[1][~run] == 255).all()
    want = _beam(a, b, n, w, n, 2, 34)
    for skip in ("plan", "score"):                             # each optional output left out once
        _same(_beam(a, b, n, w, n, 2, 34, skip=skip), want, (n, skip), skip=skip)
    _same(_beam(a, b, n, w, (1 << 40) + 3, 2, 34), want, "per above n")
    assert np.array_equal(a.host(), states.A[idx].view(np.uint8).reshape(-1))       # the states are read only
    assert np.array_equal(b.host(), states.B[idx].view(np.uint8).reshape(-1))
    if n == POOL:
        assert (~run).sum() >= 100 and (act2 != act1).any()


# ------------------------------------------------------------------------------------------------ 2. the reference beam
def _state_of(B):
    return (B[..., 1] >> np.uint32(28)) & np.uint32(3)


def _choose(value, valid):
    """The best valid node of every final beam under the rule's order: its index [n]."""
    best = np.zeros(value.shape[0], np.int64)
    for s in range(value.shape[0]):
        at = np.flatnonzero(valid[s])
        best[s] = at[_m().beam_select(value[s][at], 1)[0]]
    return best


def compose(env, A, B, plies, wrows, depth, width):
    """The rule with every ply made by the parent's kernels: T.afterstates and T.placement_features on the beam's planes, the
    cleared rows accumulated, placement_score, beam_select.  A, B uint32 [n, 4], plies [n] the effective depth of every state,
    wrows float32 [n, 12].  Returns action, plan, score and what the coverage test counts."""
    m = _m()
    n = A.shape[0]
    nodeA, nodeB = A[:, None, :].copy(), B[:, None, :].copy()
    cleared = np.zeros((n, 1), np.int64)
    value = m.placement_score(np.zeros(NF, np.int64), wrows)[:, None].copy()        # a finished root: the score of twelve zeros
    path = np.full((n, 1, depth), 255, np.uint8)
    valid = np.ones((n, 1), bool)
    edge_tie = np.zeros(n, bool)
    for j in range(int(plies.max(initial=0))):
        act = np.flatnonzero(plies > j)
        k, wc = act.size, nodeA.shape[1]
        pa, pb = (_i32(x[act].reshape(-1, 4)).to(DEV) for x in (nodeA, nodeB))
        after = T.afterstates(env, pa, pb)
        phi, canonical = T.placement_features(env, pa, pb)
        sa, sb = (_np(after[key]).view(np.uint32).reshape(k, wc, 40, 4) for key in ("states_a", "states_b"))
        rows = _np(after["cleared"]).reshape(k, wc, 40).astype(np.int64)
        psi = _np(phi).reshape(k, wc, 40, NF).astype(np.int32)
        run = _state_of(nodeB[act]) == 0                                              # [k, wc]
        assert np.array_equal(psi[..., 0][run], rows[run])
        psi[..., 0] = cleared[act][:, :, None] + rows
        score = np.where(run[:, :, None], m.placement_score(psi, wrows[act][:, None, None, :]), value[act][:, :, None])
        distinct = _np(canonical).reshape(k, wc, 40) == ARANGE
        cand = valid[act][:, :, None] & np.where(run[:, :, None], distinct, ARANGE == 0)
        keep = []
        for t in range(k):                                     # the candidates in order: node by node, ascending placement
            at = np.flatnonzero(cand[t].reshape(-1))
            v = score[t].reshape(-1)[at]
            keep.append(at[m.beam_select(v, width)])
            if at.size > width:
                ranked = np.sort(v)[::-1]
                edge_tie[act[t]] |= ranked[width - 1] == ranked[width]
        wn = max(wc, max(x.size for x in keep))
        grown = lambda x, fill: np.concatenate([x, np.full((n, wn - wc) + x.shape[2:], fill, x.dtype)], axis=1)
        nodeA, nodeB, cleared, value, path, valid = (grown(x, f) for x, f in ((nodeA, 0), (nodeB, 0), (cleared, 0), (value, 0),
                                                                                (path, 255), (valid, False)))
        for t, s in enumerate(act):
            q, b = keep[t] // 40, keep[t] % 40
            size = q.size
            moved = run[t][q]
            new_path = path[s, q].copy()
            new_path[moved, j] = b[moved]
            nodeA[s, :size], nodeB[s, :size] = sa[t, q, b], sb[t, q, b]              # a finished board's afterstate is itself
            cleared[s, :size] = cleared[s, q] + rows[t, q, b]
            value[s, :size] = score[t, q, b]
            path[s, :size] = new_path
            valid[s] = np.arange(wn) < size
    best = _choose(value, valid)
    at = np.arange(n)
    end = _state_of(nodeB)
    last = np.maximum(plies, 1) - 1
    carried = valid & (end != 0) & (path[at[:, None], np.arange(valid.shape[1])[None, :], last[:, None]] == 255) & (plies >= 2)[:, None]
    return dict(action=np.where(plies > 0, path[at, best, 0], 0).astype(np.uint8), plan=path[at, best], score=value[at, best],
                carried=carried.any(axis=1), wins=(end[at, best] == 1) & (plies > 0), edge_tie=edge_tie)


class Reference:
    """compose() of all 1,639 states, once per (weights, depth, width)."""

    def __init__(self, states, env):
        self.states, self.env, self.memo = states, env, {}

    def get(self, name, w, depth, width):
        key = (name, depth, width)
        if key not in self.memo:
            s = self.states
            rows = np.broadcast_to(np.asarray(w, np.float32), (POOL, NF))
            self.memo[key] = compose(self.env, s.A, s.B, s.plies(np.arange(POOL), depth), rows, depth, width)
        return self.memo[key]


@pytest.fixture(scope="module")
def reference(states, env10):
    return Reference(states, env10)


@pytest.fixture(scope="module")
def all_planes(states):
    return _planes(states.A, states.B)


SHAPES = [(2, 1), (2, 3), (2, 33), (3, 1), (3, 4), (3, 64), (4, 8), (12, 2)]


@pytest.mark.parametrize("depth,width", SHAPES)
def test_the_beam_is_the_parents_kernels_composed_ply_by_ply(states, reference, all_planes, depth, width):
    a, b = all_planes
    for name, w in (("classical", CLASSICAL), ("small integers", SMALL)):
        want = reference.get(name, w, depth, width)
        got = _beam(a, b, POOL, w, POOL, depth, width)
        _same(got, (want["action"], want["plan"], want["score"]), (name, depth, width))
        run = states.running
        assert (got[0][~run] == 0).all() and (got[1][~run] == 255).all()
        assert (got[1][run, 0] == got[0][run]).all() and (got[0][run] < 40).all()


def test_the_widest_and_deepest_beam_on_a_subset(states, env10):
    idx = states.take(64, 3)                                   # every kind of state, moves 8, 9, 18, 19 among them
    a, b = _planes(states.A[idx], states.B[idx])
    plies = states.plies(idx, 12)
    assert plies.max() == 12 and plies.min() == 0 and np.unique(plies).size >= 6
    for w in (CLASSICAL, SMALL):
        want = compose(env10, states.A[idx], states.B[idx], plies, np.broadcast_to(w, (64, NF)), 12, 64)
        _same(_beam(a, b, 64, w, 64, 12, 64), (want["action"], want["plan"], want["score"]), "12 x 64")
        assert ((want["plan"] != 255).sum(axis=1) <= plies).all()


@pytest.mark.parametrize("per", [1, 3, 1000])
def test_a_population_searches_with_one_weight_row_per_member(states, env10, all_planes, per):
    a, b = all_planes
    members = -(-POOL // per)
    gen = np.random.default_rng(per)
    w = gen.normal(size=(members, NF)).astype(np.float32)
    w[::3] = gen.integers(-2, 3, w[::3].shape)
    rows = w[np.arange(POOL) // per]
    want = compose(env10, states.A, states.B, states.plies(np.arange(POOL), 3), rows, 3, 4)
    _same(_beam(a, b, POOL, w, per, 3, 4), (want["action"], want["plan"], want["score"]), per)
    if members > 1:                                            # the rows matter
        one = compose(env10, states.A, states.B, states.plies(np.arange(POOL), 3), np.broadcast_to(w[0], (POOL, NF)), 3, 4)
        assert (one["action"] != want["action"]).any()


# ------------------------------------------------------------------------------------------------ 3. the oracle
def oracle_beam(O, f, i, plies, w, depth, width, L=L, M=M):
    """The rule on state i at the game (L, M) with every move played by the C oracle: (action, plan, score)."""
    m = _m()
    window = int(f["window"][i])
    pieces = [(window >> (3 * j)) & 7 for j in range(plies)]
    nodes = [dict(rows=f["rows"][i], lines=int(f["lines"][i]), moves=int(f["moves"][i]), state=0, cleared=0, value=None, path=[])]
    for j in range(plies):
        placements = np.flatnonzero(m.canonical_actions(pieces[j], ARANGE) == ARANGE)
        cands, fresh = [], []
        for node in nodes:
            if node["state"] != 0:
                cands.append(node)
                continue
            for b in placements:
                g = O.Game(L, M, rows=node["rows"], pieces=[pieces[j]], lines_cleared=node["lines"], moves_used=node["moves"])
                ret = g.move(int(b) // 10, int(b) % 10)
                child = dict(rows=g.rows.copy(), lines=g.lines_cleared, moves=g.moves_used, state=g.state,
                             cleared=node["cleared"] + max(ret, 0), value=None, path=node["path"] + [int(b)])
                cands.append(child)
                fresh.append(child)
        if fresh:                                              # none where every node of the beam is a finished game
            board = m.board_features(np.array([c["rows"] for c in fresh], np.uint16))
            head = np.array([(c["cleared"], c["state"] == 1, c["state"] == 2) for c in fresh], np.int64)
            for c, v in zip(fresh, m.placement_score(np.concatenate([head, board], axis=1), w)):
                c["value"] = v
        keep = m.beam_select(np.array([c["value"] for c in cands], np.float32), width)
        nodes = [cands[k] for k in keep]
    best = nodes[m.beam_select(np.array([c["value"] for c in nodes], np.float32), 1)[0]]
    return best["path"][0], best["path"] + [255] * (depth - len(best["path"])), best["value"]


@pytest.mark.parametrize("depth,width", [(3, 4), (4, 8)])
def test_the_beam_is_oracle_moves_and_the_host_features(oracle, states, depth, width):
    f = states.fields
    plies = states.plies(np.arange(POOL), depth)
    window = f["window"]
    real = np.ones(POOL, bool)
    for j in range(depth):                                     # the oracle has no piece 7
        real &= (j >= plies) | (((window >> np.uint64(3 * j)) & np.uint64(7)) <= 6)
    able = np.flatnonzero(states.running & real)
    idx = able[np.linspace(0, able.size - 1, 200).astype(np.int64)]
    assert np.unique(idx).size == 200 and {8, 9, 18, 19} <= set(states.moves[idx].tolist())
    a, b = _planes(states.A[idx], states.B[idx])
    for name, w in (("classical", CLASSICAL), ("small integers", SMALL)):
        got = _beam(a, b, 200, w, 200, depth, width)
        for t, i in enumerate(idx):
            action, plan, score = oracle_beam(oracle, f, i, int(plies[i]), w, depth, width)
            assert (int(got[0][t]), got[1][t].tolist()) == (action, plan), (name, i, got[1][t].tolist(), plan)
            assert got[2][t].view(np.uint32) == np.float32(score).view(np.uint32), (name, i, got[2][t], score)


# ------------------------------------------------------------------------------------------------ 4. coverage
# half of what the reference measures -- 498, 988, 142, 292, 406 and 1,194 -- as TwoPly's >= 100
COVERAGE_FLOOR = dict(clamped=249, carried=494, wins_inside=71, width_matters=146, depth_matters=203, edge_ties=597)


def test_the_reference_covers_what_the_rule_distinguishes(states, reference):
    deep = reference.get("classical", CLASSICAL, 12, 2)
    narrow, wide = reference.get("classical", CLASSICAL, 3, 4), reference.get("classical", CLASSICAL, 3, 64)
    two = reference.get("classical", CLASSICAL, 2, 33)
    small = reference.get("small integers", SMALL, 3, 4)
    run = states.running
    count = dict(clamped=int((run & (states.known < 12) & np.isin(states.moves % 10, (8, 9))).sum()),
                 carried=int(wide["carried"].sum() + deep["carried"].sum()),
                 wins_inside=int(wide["wins"].sum()),
                 width_matters=int((narrow["action"] != wide["action"]).sum()),
                 depth_matters=int((wide["action"] != two["action"]).sum()),
                 edge_ties=int(small["edge_tie"].sum()))
    print("coverage of the reference's outcomes:", count)
    assert min(count.values()) > 0, count
    for name, least in COVERAGE_FLOOR.items():
        assert count[name] >= least, (name, count)


# ------------------------------------------------------------------------------------------------ 5. the plan is playable
@pytest.mark.parametrize("depth,width", [(3, 4), (12, 8)])
def test_playing_the_plan_reaches_a_board_that_scores_the_score(states, depth, width):
    m = _m()
    for name, w in (("classical", CLASSICAL), ("random", RANDOM)):
        env, idx = _resident(states, POOL, 0, REWARDS[0])
        assert not env.auto_reset and env.pool_info()["n_configs"] == 0          # no pool: no refill, the rule's pop
        policy = T.BeamPolicy(env, w, depth, width)
        score = torch.empty(POOL, dtype=torch.float32, device=DEV)
        plan = torch.full((POOL, depth), 77, dtype=torch.uint8, device=DEV)
        action = policy.act(score=score, plan=plan)
        plan, score = _np(plan), _np(score)
        assert np.array_equal(_np(action), np.where(states.running, plan[:, 0], 0))
        plies = states.plies(idx, depth)
        # the planes after j steps, j = 0 .. depth; a board's end is after its own number of plies (a finished board stays)
        seen = [tuple(_np(x).view(np.uint32).copy() for x in env.raw_planes())]
        for j in range(depth):
            step = np.where(plan[:, j] == 255, 0, plan[:, j]).astype(np.uint8)
            env.step(torch.from_numpy(step).to(DEV), observe=False)
            seen.append(tuple(_np(x).view(np.uint32).copy() for x in env.raw_planes()))
        env.terminate()
        A = np.stack([seen[p][0][i] for i, p in enumerate(plies)])
        B = np.stack([seen[p][1][i] for i, p in enumerate(plies)])
        end, start = R.decode_state(A, B), R.decode_state(states.A, states.B)
        run = states.running
        psi = np.zeros((POOL, NF), np.int64)
        psi[:, 0] = end["lines"].astype(np.int64) - start["lines"].astype(np.int64)
        psi[:, 1] = end["state"] == 1
        psi[:, 2] = end["state"] >= 2
        psi[:, 3:] = m.board_features(end["rows"])
        psi[~run] = 0
        want = m.placement_score(psi, w)
        bad = np.flatnonzero(want.view(np.uint32) != score.view(np.uint32))
        assert bad.size == 0, (name, depth, width, bad[:5].tolist(), want[bad[:5]].tolist(), score[bad[:5]].tolist())
        # a plan ends where the game ends or the known pieces do
        length = (plan != 255).sum(axis=1)
        assert (length <= plies).all() and (length[run] >= 1).all() and ((length == plies) | (end["state"] != 0)).all()


# ------------------------------------------------------------------------------------------------ 6. the policy object
def test_the_policy_object_and_a_captured_graph(states):
    n = 300
    env, idx = _resident(states, n, 900, REWARDS[0])
    a, b = _planes(states.A[idx], states.B[idx])
    gen = np.random.default_rng(4)
    w = gen.normal(size=(3, NF)).astype(np.float32)
    policy = T.BeamPolicy(env, w.tolist(), 3, 4, boards_per_member=128)             # 128 + 128 + 44
    assert (policy.members, policy.boards_per_member, policy.depth, policy.width, policy.env) == (3, 128, 3, 4, env)
    want = _beam(a, b, n, w, 128, 3, 4)
    act = policy.act()
    assert act.dtype == torch.uint8 and tuple(act.shape) == (n,) and np.array_equal(_np(act), want[0])
    out = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    plan = torch.full((n, 3), 77, dtype=torch.uint8, device=DEV)
    score = torch.empty(n, dtype=torch.float32, device=DEV)
    assert policy.act(out=out, score=score, plan=plan) is out
    _same((_np(out), _np(plan), _np(score)), want, "policy")
    for bad in (torch.empty((n, 4), dtype=torch.uint8, device=DEV), torch.empty((n + 1, 3), dtype=torch.uint8, device=DEV),
                torch.empty((n, 3), dtype=torch.int32, device=DEV), torch.empty((n, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="plan"):
            policy.act(plan=bad)
    with pytest.raises(ValueError, match="score"):
        policy.act(score=torch.empty(n + 1, dtype=torch.float32, device=DEV))
    # captured into a graph: one launch, no allocation, no host sync; set_weights in place
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            policy.act(out=out, score=score, plan=plan)
    where = policy.weights.data_ptr()
    policy.set_weights(w[::-1].copy())
    assert policy.weights.data_ptr() == where
    for t in (out, plan):
        t.fill_(99)
    graph.replay()
    torch.cuda.synchronize()
    _same((_np(out), _np(plan), _np(score)), _beam(a, b, n, w[::-1].copy(), 128, 3, 4), "replayed")
    assert (_np(out) != want[0]).any()
    pa, pb = env.raw_planes()                                  # act() leaves the environment's planes untouched
    assert np.array_equal(_np(pa).view(np.uint32), states.A[idx]) and np.array_equal(_np(pb).view(np.uint32), states.B[idx])
    env.terminate()


def test_evaluate_with_a_width_is_deterministic_and_the_depth_reaches_the_players():
    f = load_golden("carved_L10_M40.npz")
    n, steps = 2048, 2 * M
    env = T.BatchedTetris(L, M, n, device=DEV, seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=(f["rows"], f["pieces"]))
    deep = T.evaluate_heuristic(env, CLASSICAL, None, steps, depth=3, width=8)
    again = T.evaluate_heuristic(env, CLASSICAL, None, steps, depth=3, width=8, policy=T.BeamPolicy(env, CLASSICAL, 3, 8))
    two = T.evaluate_heuristic(env, CLASSICAL, None, steps, depth=2)
    with pytest.raises(ValueError, match="BeamPolicy"):
        T.evaluate_heuristic(env, CLASSICAL, None, steps, depth=2, policy=T.BeamPolicy(env, CLASSICAL, 2, 8))
    with pytest.raises(ValueError, match="width 4"):
        T.evaluate_heuristic(env, CLASSICAL, None, steps, depth=3, width=8, policy=T.BeamPolicy(env, CLASSICAL, 3, 4))
    env.terminate()
    print("depth 3 x 8:", {k: v.tolist() for k, v in deep.items()}, "depth 2:", {k: v.tolist() for k, v in two.items()})
    assert deep["episodes"].tolist() == again["episodes"].tolist() and deep["wins"].tolist() == again["wins"].tolist()
    assert deep["episodes"][0] >= n and (deep["episodes"].tolist(), deep["wins"].tolist()) != (two["episodes"].tolist(), two["wins"].tolist())


def test_depth_two_at_full_width_solves_the_two_piece_game_and_the_tuner_is_deterministic():
    EVAL_L, EVAL_M = 2, 2
    carved = T.generate_configs(EVAL_L, EVAL_M, 64, seed=107)
    n, steps = 4096, 16
    w = np.zeros(NF, np.float32)
    w[1] = 1.0
    env = T.BatchedTetris(EVAL_L, EVAL_M, n, device=DEV, seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)
    beam = T.evaluate_heuristic(env, w, None, steps, depth=2, width=34)
    search = T.evaluate_heuristic(env, w, None, steps, depth=2)
    env.terminate()
    e, won = int(beam["episodes"][0]), int(beam["wins"][0])
    assert e >= n * steps // EVAL_M // 2 and won == e          # the identity with the two-ply search, which solves this game
    assert search["episodes"].tolist() == [e] and search["wins"].tolist() == [won]
    kw = dict(population=8, boards_per_member=256, steps=8, generations=2, seed=5, device=DEV, depth=3, width=4)
    first, second = T.tune_heuristic(EVAL_L, EVAL_M, carved, **kw), T.tune_heuristic(EVAL_L, EVAL_M, carved, **kw)
    assert np.array_equal(first["mean"], second["mean"]) and np.array_equal(first["best"], second["best"])
    assert first["best_fitness"] == second["best_fitness"] and first["history"] == second["history"] and len(first["history"]) == 2
    one = T.tune_heuristic(EVAL_L, EVAL_M, carved, **dict(kw, depth=1, width=None))
    assert one["history"] != first["history"]                  # the depth and the width reach the members
