"""Placement features, the fused placement policy and its tuning on one MI355X (include/tpl_learn.h's rule, tpl_placement_features,
tpl_placement_act, heuristic.py):

  * FEATURES: for every board of test_afterstates_gpu's 1,639 states and all 40 actions, the twelve kernel values are the C
    oracle's move (return value and state -> features 0..2) and _learn_lib.board_features of the board it leaves (3..11);
    finished boards are all zero; canaries around both outputs, `canonical` left out once; the cases cover every feature.
  * ACT: action and best score are the numpy arg-max over the distinct placements of _learn_lib.placement_score, bit for bit,
    for random, small-integer (ties), one-hot and reward weights, one policy or a population with a short last member; with
    the reward weights the actions are LookaheadPolicy(env, None).act()'s.
  * EVALUATE / TUNE on an L = 2 / M = 2 carved pool: a population evaluated jointly is each member evaluated alone;
    tune_heuristic is deterministic and its best member beats the uniform random policy by more than five standard errors.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import L, M, POOL, REWARDS, SIZES, Pool, _i32, _resident
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NF = 12


def _m():
    return T._learn_lib


class Cases:
    """The pool and -- computed once -- phi of all 40 actions of every state as the oracle and the numpy mirror give it."""

    def __init__(self, oracle, pool=None):
        """Without `pool`: test_afterstates_gpu's own, and the coverage conditions of its 1,639 states; with one (a Pool of other
        states, played at its own game): phi of those, the coverage left to the caller."""
        p = self.pool = Pool(oracle) if pool is None else pool
        run = p.running[:, None]
        board = _m().board_features(p.rows.reshape(-1, 20)).reshape(p.n, 40, 9)
        phi = np.zeros((p.n, 40, NF), np.int64)
        phi[:, :, 0] = p.cleared
        phi[:, :, 1] = p.won
        phi[:, :, 2] = p.limit | p.topout
        phi[:, :, 3:] = board
        self.phi = np.where(run[:, :, None], phi, 0)
        cur = (p.fields["window"] & np.uint64(7)).astype(np.int64)
        self.canonical = _m().canonical_actions(cur[:, None], np.arange(40)[None, :])
        self.distinct = self.canonical == np.arange(40)[None, :]
        if pool is not None:
            return
        # the coverage conditions, on the oracle's own outcomes
        values = {name: np.unique(self.phi[:, :, k]).size for k, name in enumerate(_m().FEATURE_NAMES)}
        clearing, topouts = int((self.phi[:, :, 0] > 0).sum()), int(p.topout.sum())
        print(f"distinct values per feature over {POOL} x 40: {values}; {clearing} clearing pairs, {topouts} top-out pairs, "
              f"{int((~p.running).sum())} finished boards, largest value {int(self.phi.max())}")
        for name, count in values.items():
            assert count >= (2 if name in ("won", "lost") else 3), (name, count)
        assert clearing >= 100 and topouts >= 100 and (~p.running).any()
        assert self.phi.min() >= 0 and self.phi.max() < 1 << 15

    def best(self, idx, weights, per):
        """(action u8 [n], score f32 [n]): the lowest index at the float32 maximum of placement_score over the distinct
        placements, board i of the selection under weight row i // per."""
        w = np.asarray(weights, np.float32).reshape(-1, NF)
        member = np.arange(idx.size) // per
        score = _m().placement_score(self.phi[idx], w[member][:, None, :])
        masked = np.where(self.distinct[idx], score, -np.inf)
        act = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)
        return act.astype(np.uint8), score[np.arange(idx.size), act]


@pytest.fixture(scope="module")
def cases(oracle):
    return Cases(oracle)


def _planes(A, B):
    n = A.shape[0]
    a, b = Framed(n * 16, 1), Framed(n * 16, 2)
    a.inner().copy_(torch.from_numpy(np.ascontiguousarray(A).view(np.uint8).reshape(-1)))
    b.inner().copy_(torch.from_numpy(np.ascontiguousarray(B).view(np.uint8).reshape(-1)))
    return a, b


# ------------------------------------------------------------------------------------------------ 1. features
@pytest.mark.parametrize("n", SIZES)
def test_the_features_are_the_oracle_move_and_the_mirror_for_every_board_and_action(cases, n):
    pool = cases.pool
    idx = pool.take(n, 0 if n == POOL else 7 * n)
    a, b = _planes(pool.A[idx], pool.B[idx])
    feats, canon = Framed(n * 40 * NF * 2, 3), Framed(n * 40, 4)
    for with_canonical in (True, False):
        feats.inner().fill_(0xCD)
        canon.inner().fill_(0xCD)
        _check(_lib().tpl_placement_features(a.ptr(), b.ptr(), n, L, M, feats.ptr(), canon.ptr() if with_canonical else None,
                                             _stream()))
        for name, f in (("features", feats), ("canonical", canon), ("a", a), ("b", b)):
            f.assert_canary((n, with_canonical, name))
        got = feats.host().view(np.int16).reshape(n, 40, NF).astype(np.int64)
        wrong = np.argwhere(got != cases.phi[idx])
        assert wrong.size == 0, (n, wrong[:5].tolist(), got[tuple(wrong[0][:2])].tolist(), cases.phi[idx][tuple(wrong[0][:2])].tolist())
        if with_canonical:
            assert np.array_equal(canon.host().reshape(n, 40), cases.canonical[idx]), n
        else:
            assert (canon.host() == 0xCD).all(), n              # an output that was not given is not written
    run = pool.running[idx]
    assert (got[~run] == 0).all()
    if n == POOL:
        assert (~run).any() and (got[run].reshape(-1, NF).max(axis=0) > 0).all()
    assert np.array_equal(a.host(), pool.A[idx].view(np.uint8).reshape(-1))    # the states are read only


def test_placement_features_of_resident_boards_and_of_given_planes(cases):
    pool, n = cases.pool, 300
    env, idx = _resident(pool, n, 11, REWARDS[0])
    feats, canon = T.placement_features(env)
    assert feats.shape == (n, 40, NF) and feats.dtype == torch.int16 and canon.shape == (n, 40) and canon.dtype == torch.uint8
    assert np.array_equal(_np(feats).astype(np.int64), cases.phi[idx]) and np.array_equal(_np(canon), cases.canonical[idx])
    f2, c2 = T.placement_features(env, _i32(pool.A[idx]), _i32(pool.B[idx]))
    assert torch.equal(f2, feats) and torch.equal(c2, canon)
    a, b = env.raw_planes()
    assert np.array_equal(_np(a).view(np.uint32), pool.A[idx]) and np.array_equal(_np(b).view(np.uint32), pool.B[idx])
    env.terminate()


# ------------------------------------------------------------------------------------------------ 2. act
def _weight_sets():
    gen = np.random.default_rng(12)
    sets = [("random", gen.normal(size=NF).astype(np.float32)),
            ("random, wide", (gen.normal(size=NF) * 10.0 ** gen.integers(-3, 4, NF)).astype(np.float32)),
            ("small integers", gen.integers(-2, 3, NF).astype(np.float32)),
            ("all zero", np.zeros(NF, np.float32)),
            ("the classical signs", np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1))]
    for k in range(NF):
        for sign in (1.0, -1.0):
            w = np.zeros(NF, np.float32)
            w[k] = sign
            sets.append((f"one-hot {sign:+.0f} on {_m().FEATURE_NAMES[k]}", w))
    for params in REWARDS:
        sets.append((f"reward {params}", np.array(list(params) + [0.0] * 9, np.float32)))
    return sets


def _act(a, b, n, weights, per, with_score=True, L=L, M=M):
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, NF)
    wf = Framed(w.size * 4, 5)
    wf.inner().copy_(torch.from_numpy(w.view(np.uint8).reshape(-1)))
    action, score = Framed(n, 6), Framed(n * 4, 7)
    action.inner().fill_(0xCD)
    score.inner().fill_(0xCD)
    _check(_lib().tpl_placement_act(a.ptr(), b.ptr(), n, L, M, wf.ptr(), per, action.ptr(), score.ptr() if with_score else None,
                                    _stream()))
    for name, f in (("action", action), ("score", score), ("weights", wf), ("a", a), ("b", b)):
        f.assert_canary((n, per, name))
    assert np.array_equal(wf.host(), w.view(np.uint8).reshape(-1))
    if not with_score:
        assert (score.host() == 0xCD).all()
    return action.host().copy(), score.host().view(np.float32).copy()


@pytest.mark.parametrize("n", SIZES)
def test_action_and_best_score_are_the_numpy_arg_max_bit_for_bit(cases, n):
    pool = cases.pool
    idx = pool.take(n, 0 if n == POOL else 7 * n)
    a, b = _planes(pool.A[idx], pool.B[idx])
    ties = 0
    for name, w in _weight_sets():
        act, score = _act(a, b, n, w, n)
        want_act, want_score = cases.best(idx, w, n)
        assert np.array_equal(act, want_act), (n, name, np.flatnonzero(act != want_act)[:5])
        assert np.array_equal(score.view(np.uint32), want_score.view(np.uint32)), (n, name)
        assert cases.distinct[idx][np.arange(n), act].all()
        if name == "small integers":
            s = np.where(cases.distinct[idx], _m().placement_score(cases.phi[idx], w), -np.inf)
            ties = int(((s == s.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    act2, _ = _act(a, b, n, _weight_sets()[0][1], n, with_score=False)
    assert np.array_equal(act2, cases.best(idx, _weight_sets()[0][1], n)[0])
    run = pool.running[idx]
    assert (act2[~run] == 0).all()
    if n == POOL:
        print(f"small-integer weights: {ties} of {n} boards have more than one placement at the maximum")
        assert ties >= 100
    # a boards_per_member above n is the single-policy case
    act3, _ = _act(a, b, n, _weight_sets()[0][1], (1 << 40) + 3)
    assert np.array_equal(act3, act2)


@pytest.mark.parametrize("per", [1, 3, 64, 1000, POOL])
def test_a_population_plays_one_weight_row_per_member(cases, per):
    pool, n = cases.pool, POOL
    idx = pool.take(n, 0)
    a, b = _planes(pool.A, pool.B)
    members = -(-n // per)
    assert per in (1, n) or n % per != 0                       # a short last member
    gen = np.random.default_rng(per)
    w = gen.normal(size=(members, NF)).astype(np.float32)
    w[::3] = gen.integers(-2, 3, w[::3].shape)
    act, score = _act(a, b, n, w, per)
    want_act, want_score = cases.best(idx, w, per)
    assert np.array_equal(act, want_act) and np.array_equal(score.view(np.uint32), want_score.view(np.uint32))
    if members > 1:                                            # the rows matter: one row for everybody gives other actions
        assert (cases.best(idx, w[:1], n)[0] != want_act).any()


def test_the_policy_object_and_the_reward_weights(cases):
    pool, n = cases.pool, 300
    for params in REWARDS:
        env, idx = _resident(pool, n, 500, params)
        w = np.array(list(params) + [0.0] * 9, np.float32)
        policy = T.HeuristicPolicy(env, w)
        assert policy.members == 1 and policy.boards_per_member == n
        act = policy.act()
        assert act.dtype == torch.uint8 and tuple(act.shape) == (n,)
        look = T.LookaheadPolicy(env, image=None).act()
        assert torch.equal(act, look), params
        # and the best score is the best distinct afterstate reward, bit for bit (no reward here is -0)
        out = T.afterstates(env, with_states=False)
        reward = np.where(cases.distinct[idx], _np(out["reward"]), -np.inf)
        score = torch.empty(n, dtype=torch.float32, device=DEV)
        buf = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
        assert policy.act(out=buf, score=score) is buf and torch.equal(buf, act)
        assert np.array_equal(_np(score).view(np.uint32), reward.max(axis=1).astype(np.float32).view(np.uint32))
        a, b = env.raw_planes()                                # act() leaves the environment's planes untouched
        assert np.array_equal(_np(a).view(np.uint32), pool.A[idx]) and np.array_equal(_np(b).view(np.uint32), pool.B[idx])
        env.terminate()
    # a population through the object, lists accepted, set_weights in place
    env, idx = _resident(pool, n, 900, REWARDS[0])
    gen = np.random.default_rng(4)
    w = gen.normal(size=(3, NF)).astype(np.float32)
    policy = T.HeuristicPolicy(env, w.tolist(), 128)           # 128 + 128 + 44
    assert policy.members == 3
    assert np.array_equal(_np(policy.act()), cases.best(idx, w, 128)[0])
    where = policy.weights.data_ptr()
    policy.set_weights(w[::-1].copy())
    assert policy.weights.data_ptr() == where
    assert np.array_equal(_np(policy.act()), cases.best(idx, w[::-1], 128)[0])
    # captured into a graph: no allocation, no host sync
    out = torch.empty(n, dtype=torch.uint8, device=DEV)
    policy.act(out=out)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            policy.act(out=out)
    policy.set_weights(w)
    out.fill_(255)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np(out), cases.best(idx, w, 128)[0])
    env.terminate()


# ------------------------------------------------------------------------------------------------ 3. evaluate, tune
EVAL_L, EVAL_M, PER, STEPS = 2, 2, 256, 8


@pytest.fixture(scope="module")
def carved():
    return T.generate_configs(EVAL_L, EVAL_M, 64, seed=107)


def _eval_env(n, carved, offset=0, seed=3):
    return T.BatchedTetris(EVAL_L, EVAL_M, n, device=DEV, seed=seed, global_offset=offset, auto_reset=True,
                           reward=(0.0, 1.0, 0.0), config_pool=carved)


def test_a_population_evaluated_jointly_is_each_member_alone(carved):
    P = 4
    gen = np.random.default_rng(8)
    w = gen.normal(size=(P, NF)).astype(np.float32)
    w[0] = 0.0
    w[0, 1] = 1.0                                              # one member that plays for the win
    env = _eval_env(P * PER, carved)
    joint = T.evaluate_heuristic(env, w, PER, STEPS)
    assert env.step_clock() == STEPS
    assert T.evaluate_heuristic(env, w, PER, STEPS)["wins"].tolist() == joint["wins"].tolist()       # from a full reset
    env.terminate()
    for k in ("episodes", "wins"):
        assert joint[k].shape == (P,) and joint[k].dtype == np.int64
    print("joint:", {k: v.tolist() for k, v in joint.items()})
    assert (joint["episodes"] >= PER * STEPS // EVAL_M // 2).all() and (joint["wins"] <= joint["episodes"]).all()
    assert np.array_equal(joint["win_rate"], joint["wins"] / np.maximum(joint["episodes"], 1))
    assert joint["wins"][0] > 0 and len(set(joint["wins"].tolist())) > 1
    for p in range(P):
        alone_env = _eval_env(PER, carved, offset=PER * p)
        alone = T.evaluate_heuristic(alone_env, w[p], None, STEPS)
        alone_env.terminate()
        assert alone["episodes"].tolist() == [joint["episodes"][p]] and alone["wins"].tolist() == [joint["wins"][p]], p
    with pytest.raises(ValueError, match=r"\(0, 1, 0\)"):
        bad = T.BatchedTetris(EVAL_L, EVAL_M, PER, device=DEV, auto_reset=True, config_pool=carved)
        try:
            T.evaluate_heuristic(bad, w[0], None, STEPS)
        finally:
            bad.terminate()


def test_the_tuner_is_deterministic_and_its_best_member_beats_the_random_policy(carved):
    kw = dict(population=16, boards_per_member=PER, steps=STEPS, generations=3, seed=5, device=DEV)
    first = T.tune_heuristic(EVAL_L, EVAL_M, carved, **kw)
    again = T.tune_heuristic(EVAL_L, EVAL_M, carved, **kw)
    assert first["mean"].dtype == np.float32 and first["mean"].shape == (NF,) and first["best"].shape == (NF,)
    assert np.array_equal(first["mean"], again["mean"]) and np.array_equal(first["best"], again["best"])
    assert first["best_fitness"] == again["best_fitness"] and first["history"] == again["history"]
    assert len(first["history"]) == 3
    for h in first["history"]:
        assert set(h) == {"population_mean", "elite_mean", "best"} and all(type(v) is float for v in h.values())
        assert h["population_mean"] <= h["elite_mean"] + 1e-12 and h["elite_mean"] <= h["best"] + 1e-12 and h["best"] <= 1.0
    assert first["best_fitness"] == max(h["best"] for h in first["history"])
    other = T.tune_heuristic(EVAL_L, EVAL_M, carved, **dict(kw, seed=6))
    assert not np.array_equal(other["best"], first["best"])
    # the best member and the uniform random policy over the same number of fresh episodes
    n, steps = 4096, 16
    env = _eval_env(n, carved, seed=77)
    tuned = T.evaluate_heuristic(env, first["best"], None, steps)
    e1, w1 = int(tuned["episodes"][0]), int(tuned["wins"][0])
    env.reset()
    reward_sum, finished = env.rollout_random(steps, seed=1)
    e2, w2 = int(finished.sum()), int(round(float(reward_sum.sum())))
    env.terminate()
    E = min(e1, e2)                                            # the smaller count for both: the larger standard error
    p1, p2 = w1 / e1, w2 / e2
    se = (p1 * (1 - p1) / E + p2 * (1 - p2) / E) ** 0.5
    print(f"tuned {w1} / {e1} = {p1:.4f}, random {w2} / {e2} = {p2:.4f}, E = {E}, 5 standard errors = {5 * se:.4f}; "
          f"history {first['history']}")
    assert E >= n * steps // EVAL_M // 2
    assert p1 - p2 > 5 * se
