"""The two-ply placement search on one MI355X (include/tpl_learn.h's rule, tpl_placement_search, HeuristicPolicy(depth=2)):

  * ORACLE: for every running state of test_afterstates_gpu's pool whose next piece is a real one, every distinct first placement
    and -- where the game goes on -- every distinct placement of the next piece is played as two moves of the C oracle; psi is
    built from the return values, the states and _learn_lib.board_features; the kernel's action, second and score are
    _learn_lib.search_choice on them, bit for bit, through canary-framed buffers, for every weight set of test_heuristic_gpu and
    for populations; the coverage conditions are asserted on the oracle's outcomes alone.
  * PARENT KERNELS: on all 1,639 states (finished boards and next piece 7 among them) the same with phi of both plies taken from
    tpl_placement_features and tpl_afterstates, for every size that crosses the 8-board block and the short last block.
  * STEP: after a non-auto-reset step with the chosen action, the one-ply policy chooses `second` with the same score.
  * the policy object (out / score / second, a captured graph after set_weights, the planes untouched, depth 1 as before);
  * SOLVER: on an L = 2 / M = 2 carved pool both pieces are visible at reset, so depth 2 with win-only weights wins every episode
    and depth 1 cannot.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, REWARDS, SIZES, Pool, _i32, _resident
from test_heuristic_gpu import Cases, _planes, _weight_sets
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NF = 12
WEIGHT_SETS = _weight_sets()
ARANGE = np.arange(40)


def _m():
    return T._learn_lib


class TwoPly:
    """test_heuristic_gpu's Cases and -- computed once -- psi(a, b) of every state the oracle can play two plies of."""

    def __init__(self, oracle, cases=None, L=L, M=M, most=None):
        """Without `cases`: test_heuristic_gpu's own at L = 10 / M = 40, and the coverage conditions; with them (Cases of another
        pool, played at its game (L, M)): at most `most` of its states, evenly spread, the coverage left to the caller."""
        own = cases is None
        c = self.cases = Cases(oracle) if own else cases
        p = self.pool = c.pool
        f = p.fields
        cur = (f["window"] & np.uint64(7)).astype(np.int64)
        nxt = ((f["window"] >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
        self.idx = np.flatnonzero(p.running & (nxt <= 6))      # the oracle has no piece 7
        if most is not None and self.idx.size > most:
            self.idx = self.idx[np.linspace(0, self.idx.size - 1, most).astype(np.int64)]
        K = self.idx.size
        self.done1 = p.done[self.idx]                          # [K, 40]: the first move ends the game
        self.distinct2 = _m().canonical_actions(nxt[self.idx][:, None], ARANGE[None, :]) == ARANGE[None, :]
        where, rows2, head = [], [], []                        # (k, a, b), the board after both moves, (n1 + n2, won2, lost2)
        count = dict(first_move_ends=0, win2=0, limit2=0, topout2=0, both_clear=0, cleared={k: 0 for k in range(5)})
        for k, i in enumerate(self.idx):
            pieces = [int(cur[i]), int(nxt[i])]
            for a in np.flatnonzero(c.distinct[i]):
                g1 = oracle.Game(L, M, rows=f["rows"][i], pieces=pieces, lines_cleared=int(f["lines"][i]), moves_used=int(f["moves"][i]))
                ret1 = g1.move(int(a) // 10, int(a) % 10)
                assert ret1 == p.ret[i, a] and g1.state == p.state[i, a]
                if g1.state != 0:
                    count["first_move_ends"] += 1
                    continue
                n1, rows1, lines1, moves1 = max(ret1, 0), g1.rows.tolist(), g1.lines_cleared, g1.moves_used
                assert g1.pieces == pieces[1:]
                for b in np.flatnonzero(self.distinct2[k]):
                    g = oracle.Game(L, M, rows=rows1, pieces=pieces[1:], lines_cleared=lines1, moves_used=moves1)
                    ret2 = g.move(int(b) // 10, int(b) % 10)   # the second move, from what the first one left
                    n2 = max(ret2, 0)
                    where.append((k, a, b))
                    rows2.append(g.rows)
                    head.append((n1 + n2, g.state == 1, g.state == 2))
                    count["win2"] += g.state == 1
                    count["topout2"] += ret2 < 0
                    count["limit2"] += g.state == 2 and ret2 >= 0
                    count["both_clear"] += n1 > 0 and n2 > 0
                    if n1 + n2 <= 4:
                        count["cleared"][n1 + n2] += 1
        self.pairs = len(where)
        self.phi2 = np.zeros((K, 40, 40, NF), np.int16)
        if self.pairs:                                         # none where every first move ends the game (M = 1)
            where, rows2, head = np.array(where), np.array(rows2, np.uint16), np.array(head, np.int64)
            board = np.concatenate([_m().board_features(rows2[at:at + 32768]) for at in range(0, self.pairs, 32768)])
            self.phi2[where[:, 0], where[:, 1], where[:, 2], :3] = head
            self.phi2[where[:, 0], where[:, 1], where[:, 2], 3:] = board
        self.phi1 = c.phi[self.idx]
        self.distinct1 = c.distinct[self.idx]
        print(f"{K} states, {self.pairs} (a, b) pairs; the oracle's outcomes: {count}")
        self.count = count
        if not own:
            return
        # the coverage conditions, on the oracle's own outcomes
        assert K >= 1000 and set(nxt[self.idx].tolist()) == set(range(7))
        for name in ("first_move_ends", "win2", "limit2", "topout2", "both_clear"):
            assert count[name] >= 100, (name, count)
        assert min(count["cleared"].values()) >= 100, count

    def want(self, sel, weights, per):
        """search_choice for the selection `sel` of the K states, board j of it under weight row j // per."""
        w = np.asarray(weights, np.float32).reshape(-1, NF)
        rows = w[np.arange(sel.size) // per]
        return _m().search_choice(self.phi1[sel], self.done1[sel], self.distinct1[sel], self.phi2[sel], self.distinct2[sel], rows)


@pytest.fixture(scope="module")
def twoply(oracle):
    return TwoPly(oracle)


def _search(a, b, n, weights, per, skip=None, L_=L, M_=M):
    """tpl_placement_search through canary-framed buffers; `skip` names the optional output passed as NULL."""
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, NF)
    wf = Framed(w.size * 4, 5)
    wf.inner().copy_(torch.from_numpy(w.view(np.uint8).reshape(-1)))
    action, second, score = Framed(n, 6), Framed(n, 7), Framed(n * 4, 8)
    for f in (action, second, score):
        f.inner().fill_(0xCD)
    _check(_lib().tpl_placement_search(a.ptr(), b.ptr(), n, L_, M_, wf.ptr(), per, action.ptr(),
                                       None if skip == "second" else second.ptr(), None if skip == "score" else score.ptr(),
                                       _stream()))
    for name, f in (("action", action), ("second", second), ("score", score), ("weights", wf), ("a", a), ("b", b)):
        f.assert_canary((n, per, skip, name))
    assert np.array_equal(wf.host(), w.view(np.uint8).reshape(-1))
    if skip == "second":
        assert (second.host() == 0xCD).all()                   # an output that was not given is not written
    if skip == "score":
        assert (score.host() == 0xCD).all()
    return action.host().copy(), second.host().copy(), score.host().view(np.float32).copy()


def _same(got, want, what, skip=None):
    for name, g, w in zip(("action", "second", "score"), got, want):
        if name == skip:
            continue
        g, w = (g.view(np.uint32), w.view(np.uint32)) if name == "score" else (g, w)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.fixture(scope="module")
def oracle_planes(twoply):
    p = twoply.pool
    return _planes(p.A[twoply.idx], p.B[twoply.idx])


@pytest.mark.parametrize("k", range(len(WEIGHT_SETS)), ids=[name for name, _ in WEIGHT_SETS])
def test_the_search_is_two_oracle_moves_and_the_mirror_bit_for_bit(twoply, oracle_planes, k):
    name, w = WEIGHT_SETS[k]
    a, b = oracle_planes
    n = twoply.idx.size
    sel = np.arange(n)
    want = twoply.want(sel, w, n)
    _same(_search(a, b, n, w, n), want, name)
    assert twoply.distinct1[sel, want[0]].all()
    went_on = want[1] != 255
    assert np.array_equal(went_on, ~twoply.done1[sel, want[0]]) and twoply.distinct2[sel[went_on], want[1][went_on]].all()
    if k == 0:                                                 # each optional output left out once
        for skip in ("second", "score"):
            _same(_search(a, b, n, w, n, skip=skip), want, (name, skip), skip=skip)
        _same(_search(a, b, n, w, (1 << 40) + 3), want, "per above n")
        assert went_on.sum() >= 100 and (~went_on).any()
    if name == "small integers":
        s2 = np.where(twoply.distinct2[:, None, :], _m().placement_score(twoply.phi2, w), -np.inf).max(axis=2)
        v = np.where(twoply.done1, _m().placement_score(twoply.phi1, w), s2)
        v = np.where(twoply.distinct1, v, -np.inf)
        ties = int(((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        print(f"small-integer weights: {ties} of {n} boards have more than one first placement at the maximum")
        assert ties >= 100


@pytest.mark.parametrize("per", [1, 3, 1000])
def test_a_population_searches_with_one_weight_row_per_member(twoply, oracle_planes, per):
    a, b = oracle_planes
    n = twoply.idx.size
    members = -(-n // per)
    gen = np.random.default_rng(per)
    w = gen.normal(size=(members, NF)).astype(np.float32)
    w[::3] = gen.integers(-2, 3, w[::3].shape)
    want = twoply.want(np.arange(n), w, per)
    _same(_search(a, b, n, w, per), want, per)
    if members > 1:                                            # the rows matter
        assert (twoply.want(np.arange(n), w[:1], n)[0] != want[0]).any()


# ------------------------------------------------------------------------------------------------ 2. against the parent's kernels
@pytest.mark.parametrize("n", SIZES)
def test_the_search_is_the_one_ply_kernels_composed_on_every_state(twoply, n):
    pool = twoply.pool
    env, idx = _resident(pool, n, 0 if n == POOL else 7 * n, REWARDS[0])
    phi1, canonical1 = T.placement_features(env)
    after = T.afterstates(env)
    phi2, canonical2 = T.placement_features(env, after["states_a"].view(-1, 4), after["states_b"].view(-1, 4))
    env.terminate()
    done1 = _np(after["done"]) != 0
    psi = _np(phi2).reshape(n, 40, 40, NF).copy()
    psi[..., 0] += _np(after["cleared"]).astype(np.int16)[:, :, None]              # n1 + n2
    distinct1 = _np(canonical1) == ARANGE[None, :]
    distinct2 = _np(canonical2).reshape(n, 40, 40) == ARANGE[None, None, :]
    a, b = _planes(pool.A[idx], pool.B[idx])
    run = pool.running[idx]
    nxt = ((pool.fields["window"][idx] >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
    for name, w in WEIGHT_SETS[0:5:2]:                         # random, small integers (ties), the classical signs
        want = _m().search_choice(_np(phi1), done1, distinct1, psi, distinct2, w)
        got = _search(a, b, n, w, n)
        _same(got, want, (n, name))
        assert (got[0][~run] == 0).all() and (got[1][~run] == 255).all()
        assert (got[2][~run].view(np.uint32) == _m().placement_score(np.zeros(NF, np.int64), w).view(np.uint32)).all()
    if n == POOL:
        assert (~run).sum() >= 100 and (run & (nxt == 7)).sum() >= 100
        assert np.array_equal(got[0][twoply.idx], twoply.want(np.arange(twoply.idx.size), w, POOL)[0])
    assert np.array_equal(a.host(), pool.A[idx].view(np.uint8).reshape(-1))         # the states are read only


# ------------------------------------------------------------------------------------------------ 3. against the step kernel
def test_after_the_step_the_one_ply_policy_plays_the_second_move_with_the_same_score(twoply):
    pool, n = twoply.pool, POOL
    for name, w in (WEIGHT_SETS[4], WEIGHT_SETS[0], WEIGHT_SETS[2]):
        w = w.copy()
        w[0] = 0.0                                             # the rows of the first move are in psi_0, not in phi_0 afterwards
        env, idx = _resident(pool, n, 0, REWARDS[0])
        assert not env.auto_reset
        deep, shallow = T.HeuristicPolicy(env, w, depth=2), T.HeuristicPolicy(env, w, depth=1)
        second = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
        score = torch.empty(n, dtype=torch.float32, device=DEV)
        action = deep.act(score=score, second=second)
        env.step(action, observe=False)
        _, b = env.raw_planes()
        running = ((_np(b).view(np.uint32)[:, 1] >> np.uint32(28)) & np.uint32(3)) == 0
        score1 = torch.empty(n, dtype=torch.float32, device=DEV)
        action1 = _np(shallow.act(score=score1))
        second, score, score1 = _np(second), _np(score), _np(score1)
        assert running.sum() >= 500 and (~running).sum() >= 200, name
        assert np.array_equal(action1[running], second[running]), name
        assert np.array_equal(score1[running].view(np.uint32), score[running].view(np.uint32)), name
        assert (second[~running] == 255).all(), name
        env.terminate()


# ------------------------------------------------------------------------------------------------ 4. the policy object
def test_the_policy_object_at_depth_two_and_depth_one_as_it_was(twoply):
    pool, n = twoply.pool, 300
    env, idx = _resident(pool, n, 900, REWARDS[0])
    a, b = _planes(pool.A[idx], pool.B[idx])
    gen = np.random.default_rng(4)
    w = gen.normal(size=(3, NF)).astype(np.float32)
    policy = T.HeuristicPolicy(env, w.tolist(), 128, depth=2)   # 128 + 128 + 44
    assert policy.members == 3 and policy.depth == 2
    want = _search(a, b, n, w, 128)
    act = policy.act()
    assert act.dtype == torch.uint8 and tuple(act.shape) == (n,) and np.array_equal(_np(act), want[0])
    out = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    second = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    score = torch.empty(n, dtype=torch.float32, device=DEV)
    assert policy.act(out=out, score=score, second=second) is out
    _same((_np(out), _np(second), _np(score)), want, "policy")
    with pytest.raises(ValueError, match="second"):
        policy.act(second=torch.empty(n + 1, dtype=torch.uint8, device=DEV))
    # captured into a graph: one launch, no allocation, no host sync; set_weights in place
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            policy.act(out=out, score=score, second=second)
    where = policy.weights.data_ptr()
    policy.set_weights(w[::-1].copy())
    assert policy.weights.data_ptr() == where
    for t in (out, second):
        t.fill_(99)
    graph.replay()
    torch.cuda.synchronize()
    _same((_np(out), _np(second), _np(score)), _search(a, b, n, w[::-1].copy(), 128), "replayed")
    assert (_np(out) != want[0]).any()
    pa, pb = env.raw_planes()                                  # act() leaves the environment's planes untouched
    assert np.array_equal(_np(pa).view(np.uint32), pool.A[idx]) and np.array_equal(_np(pb).view(np.uint32), pool.B[idx])
    # depth 1: the default, and byte for byte what it was
    for shallow in (T.HeuristicPolicy(env, w, 128), T.HeuristicPolicy(env, w, 128, depth=1)):
        assert shallow.depth == 1
        s1 = torch.empty(n, dtype=torch.float32, device=DEV)
        a1 = shallow.act(score=s1)
        want_act, want_score = twoply.cases.best(idx, w, 128)
        assert np.array_equal(_np(a1), want_act) and np.array_equal(_np(s1).view(np.uint32), want_score.view(np.uint32))
        with pytest.raises(ValueError, match="second"):
            shallow.act(second=second)
    env.terminate()


# ------------------------------------------------------------------------------------------------ 5. the solver property
EVAL_L, EVAL_M = 2, 2


def test_two_plies_with_win_only_weights_solve_the_two_piece_game_and_one_ply_cannot():
    carved = T.generate_configs(EVAL_L, EVAL_M, 64, seed=107)
    n, steps = 4096, 16
    w = np.zeros(NF, np.float32)
    w[1] = 1.0
    env = T.BatchedTetris(EVAL_L, EVAL_M, n, device=DEV, seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)
    deep = T.evaluate_heuristic(env, w, None, steps, depth=2)
    again = T.evaluate_heuristic(env, w, None, steps, policy=T.HeuristicPolicy(env, w, depth=2), depth=2)
    shallow = T.evaluate_heuristic(env, w, None, steps)
    with pytest.raises(ValueError, match="depth"):
        T.evaluate_heuristic(env, w, None, steps, policy=T.HeuristicPolicy(env, w, depth=2))
    env.terminate()
    e2, w2, e1, w1 = int(deep["episodes"][0]), int(deep["wins"][0]), int(shallow["episodes"][0]), int(shallow["wins"][0])
    print(f"depth 2: {w2} / {e2}; depth 1: {w1} / {e1}")
    assert e2 >= n * steps // EVAL_M // 2 and w2 == e2
    assert again["episodes"].tolist() == [e2] and again["wins"].tolist() == [w2]
    assert e1 >= n * steps // EVAL_M // 2 and w1 < e1
    kw = dict(population=8, boards_per_member=256, steps=8, generations=2, seed=5, device=DEV, depth=2)
    first, second = T.tune_heuristic(EVAL_L, EVAL_M, carved, **kw), T.tune_heuristic(EVAL_L, EVAL_M, carved, **kw)
    assert np.array_equal(first["mean"], second["mean"]) and np.array_equal(first["best"], second["best"])
    assert first["best_fitness"] == second["best_fitness"] and first["history"] == second["history"] and len(first["history"]) == 2
    one = T.tune_heuristic(EVAL_L, EVAL_M, carved, **dict(kw, depth=1))
    assert one["history"] != first["history"]                  # the depth reaches the members
