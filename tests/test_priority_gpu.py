"""Prioritized replay on one MI355X: the device sum tree equals the numpy mirror's bytes after pushes (wrapping) and write-backs
(duplicates, NaN, +-inf, 0, negatives), the prioritized draws and probabilities are the mirror's and every sampled field is the
recorded transition's, a rare high-priority needle is drawn at its share, the tree stays exact at 2^22 slots, PER updates
equal a plain-torch restatement, and the learner still learns the two small tasks with PER on."""
import copy

import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_learner_gpu import TASKS, THRESHOLDS, _env, _model, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mirror():
    return T._learn_lib


def _assert_tree(ring, tree, what=""):
    got = _np(ring.tree.view(torch.int64))
    want = tree.view(np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def _record(want, head, traj, after, cap):
    """What each slot of the ring holds after a push of `traj` at `head` (after = the resident planes after the chunk)."""
    sa, sb = _np(traj["states_a"]), _np(traj["states_b"])
    a, r, d = _np(traj["actions"]), _np(traj["rewards"]), _np(traj["dones"]).astype(np.uint8)
    steps, n = a.shape
    for t in range(steps):
        na = sa[t + 1] if t + 1 < steps else _np(after[0])
        nb = sb[t + 1] if t + 1 < steps else _np(after[1])
        slots = (head + t * n + np.arange(n)) % cap
        want["sa"][slots], want["sb"][slots], want["na"][slots], want["nb"][slots] = sa[t], sb[t], na, nb
        want["a"][slots], want["r"][slots], want["d"][slots] = a[t], r[t], d[t]


def _check_draws(env, ring, tree, want, batch, seed, update, dtype):
    next_env = T.BatchedTetris(env.L, env.M, batch, device=DEV, seed=5)
    got = ring.sample(batch, seed, update, next_env, obs_dtype=dtype)
    idx, prob = _mirror().prioritized_draws(tree, seed, update, batch)
    assert np.array_equal(_np(got["index"]), idx)
    assert np.array_equal(_np(got["prob"]).view(np.int32), prob.view(np.int32))
    ref = env.expand_states(torch.from_numpy(want["sa"][idx]).to(DEV), torch.from_numpy(want["sb"][idx]).to(DEV), dtype=dtype)
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert got["obs"].dtype == dtype and torch.equal(got["obs"].view(iv), ref.view(iv))
    na, nb = next_env.raw_planes()
    assert np.array_equal(_np(na), want["na"][idx]) and np.array_equal(_np(nb), want["nb"][idx])
    assert np.array_equal(_np(got["action"]), want["a"][idx])
    assert np.array_equal(_np(got["reward"]).view(np.uint32), want["r"][idx].view(np.uint32))
    assert np.array_equal(_np(got["done"]), want["d"][idx])
    next_env.terminate()
    return got


# ------------------------------------------------------------------------------------------------ 1 + 2. tree and draws
def test_tree_and_draws_equal_the_mirror_across_a_wrapped_ring():
    """Three pushes of 2 x 1000 transitions into a ring of 4500 (the third wraps), write-backs with duplicates and every edge
    value, a fourth push over updated slots: after each step the device tree's bytes are the mirror's, and the prioritized
    draws (slots, prob, every sampled field, obs bit for bit as env.expand_states) are too, for float32 and bf16 obs."""
    L, M, n, steps, cap = 5, 20, 1000, 2, 4500
    env = _env(L, M, n, seed=3)
    image = T.actor.policy_image(_model(0), env.device, f32="split")
    ring = T.PrioritizedReplayRing(cap, env.device)
    tree = _mirror().priority_tree_init(cap)
    _assert_tree(ring, tree, "init")
    want = dict(sa=np.zeros((cap, 4), np.int32), sb=np.zeros((cap, 4), np.int32), na=np.zeros((cap, 4), np.int32),
                nb=np.zeros((cap, 4), np.int32), a=np.zeros(cap, np.uint8), r=np.zeros(cap, np.float32), d=np.zeros(cap, np.uint8))
    gen = np.random.default_rng(0)
    for push in range(3):
        traj = env.actor_rollout(image, steps, epsilon=0.3, seed=11, step0=push * steps, record=True, record_states=True)
        head = ring.head
        ring.push(env, traj)
        _record(want, head, traj, env.raw_planes(), cap)
        _mirror().priority_tree_push(tree, head, steps * n)
        _assert_tree(ring, tree, f"push {push}")
        _check_draws(env, ring, tree, want, 777, 9, push, torch.float32)
        # a write-back with duplicates and every edge value
        index = gen.integers(0, ring.size, 300)
        index[:6] = index[6]                                              # one slot seven times
        pr = gen.random(300) * 10.0 ** gen.integers(-14, 4, 300)
        pr[[10, 11, 12, 13, 14, 15, 16]] = [np.nan, np.inf, -np.inf, 0.0, -2.5, -0.0, 1e300]
        ring.update_priorities(torch.from_numpy(index).to(DEV), torch.from_numpy(pr).to(DEV))
        _mirror().priority_tree_update(tree, index, pr)
        _assert_tree(ring, tree, f"update {push}")
    assert float(ring.max_priority()) == 1e30 == tree[0]
    assert torch.equal(ring.priorities().cpu(), torch.from_numpy(tree[16:16 + cap]))
    assert float(ring.total()) == tree[_mirror().priority_layout(cap)[0][-1]]
    for batch, dtype, update in ((4096, torch.bfloat16, 4), (64, torch.float32, 0), (4096, torch.float32, 5)):
        _check_draws(env, ring, tree, want, batch, 9, update, dtype)
    # a later push over updated slots gives them the running maximum
    traj = env.actor_rollout(image, steps, epsilon=0.3, seed=11, step0=6, record=True, record_states=True)
    head = ring.head
    ring.push(env, traj)
    _record(want, head, traj, env.raw_planes(), cap)
    _mirror().priority_tree_push(tree, head, steps * n)
    _assert_tree(ring, tree, "push over updated slots")
    slots = (head + np.arange(steps * n)) % cap
    assert (_np(ring.priorities())[slots] == 1e30).all()
    # the last sample came before this push: writing its priorities back would land on overwritten slots, so it is refused
    with pytest.raises(ValueError, match="pushed"):
        ring.update_priorities(torch.zeros(4, dtype=torch.int64, device=DEV), torch.ones(4, dtype=torch.float64, device=DEV))
    _assert_tree(ring, tree, "refused write-back")
    _check_draws(env, ring, tree, want, 4096, 3, 7, torch.bfloat16)
    env.terminate()


# ------------------------------------------------------------------------------------------------ 3. the needle
def test_needle_is_drawn_at_its_share():
    """A 2^20 ring, 64 slots at 2^14 times the base priority: half the mass.  16 minibatches of 65,536: the draws are the
    mirror's, and the needles' share is within 5 sigma of (64 * 2^14) / total."""
    cap, n, steps = 1 << 20, 1 << 16, 16
    env = _env(2, 2, n, seed=4)
    image = T.actor.policy_image(_model(1), env.device, f32="split")
    ring = T.PrioritizedReplayRing(cap, env.device)
    ring.push(env, env.actor_rollout(image, steps, epsilon=0.5, seed=2, record=True, record_states=True))
    tree = _mirror().priority_tree_push(_mirror().priority_tree_init(cap), 0, cap)
    needles = np.random.default_rng(1).choice(cap, 64, replace=False)
    next_env = T.BatchedTetris(2, 2, 65536, device=DEV, seed=5)
    ring.sample(65536, 0, 0, next_env)
    ring.update_priorities(torch.from_numpy(needles).to(DEV), torch.full((64,), 2.0 ** 14, dtype=torch.float64, device=DEV))
    _mirror().priority_tree_update(tree, needles, np.full(64, 2.0 ** 14))
    _assert_tree(ring, tree, "needles")
    share_want = 64 * 2.0 ** 14 / (cap - 64 + 64 * 2.0 ** 14)
    hits = total = 0
    for update in range(16):
        got = ring.sample(65536, 7, update, next_env)
        idx, prob = _mirror().prioritized_draws(tree, 7, update, 65536)
        assert np.array_equal(_np(got["index"]), idx) and np.array_equal(_np(got["prob"]), prob)
        hits += int(np.isin(idx, needles).sum())
        total += idx.size
    sigma = np.sqrt(share_want * (1 - share_want) / total)
    assert abs(hits / total - share_want) < 5 * sigma, (hits / total, share_want)
    next_env.terminate()
    env.terminate()


# ------------------------------------------------------------------------------------------------ 4. scale
def test_tree_is_exact_at_scale():
    """16 x 262,144 transitions pushed into a 2^22 ring, then a write-back of 65,536 with duplicates: the tree is the mirror's."""
    cap, n, steps = 1 << 22, 1 << 18, 16
    env = _env(10, 40, n, seed=6)
    image = T.actor.policy_image(_model(2), env.device, f32="split")
    ring = T.PrioritizedReplayRing(cap, env.device)
    ring.push(env, env.actor_rollout(image, steps, epsilon=0.5, seed=3, record=True, record_states=True))
    tree = _mirror().priority_tree_push(_mirror().priority_tree_init(cap), 0, steps * n)
    _assert_tree(ring, tree, "push")
    next_env = T.BatchedTetris(10, 40, 65536, device=DEV, seed=5)
    got = ring.sample(65536, 1, 0, next_env)
    idx, _ = _mirror().prioritized_draws(tree, 1, 0, 65536)
    assert np.array_equal(_np(got["index"]), idx)
    gen = np.random.default_rng(4)
    pr = np.abs(gen.standard_normal(65536)) ** 0.6 + 1e-6
    index = _np(got["index"]).copy()
    index[::17] = index[0]
    ring.update_priorities(torch.from_numpy(index).to(DEV), torch.from_numpy(pr).to(DEV))
    _mirror().priority_tree_update(tree, index, pr)
    _assert_tree(ring, tree, "update")
    next_env.terminate()
    env.terminate()


# ------------------------------------------------------------------------------------------------ 5. the learner
def test_prioritized_updates_equal_a_plain_torch_restatement():
    L, M, n = 5, 20, 1024
    env = _env(L, M, n, seed=6)
    tau, lr, alpha, beta, eps, seed = 0.005, 1e-4, 0.6, 0.4, 1e-6, 2
    learner = T.DQNLearner(env, model=_model(8), capacity=1 << 14, batch_size=128, tau=tau, lr=lr, seed=seed, prioritized=True,
                           alpha=alpha, beta=beta, beta_final=1.0, beta_updates=10, priority_eps=eps)
    assert isinstance(learner.ring, T.PrioritizedReplayRing)
    learner.collect(4)
    size = learner.ring.size
    tree = _mirror().priority_tree_push(_mirror().priority_tree_init(1 << 14), 0, size)
    _assert_tree(learner.ring, tree, "collect")
    policy_net = copy.deepcopy(learner.model)
    target_net = copy.deepcopy(learner.target)
    optimizer = torch.optim.AdamW(policy_net.parameters(), lr=lr, amsgrad=True)
    for k in range(3):
        beta_k = beta + (1.0 - beta) * min(1.0, k / 10)
        assert learner.beta() == beta_k
        learner.update(1)
        b = learner.last
        idx, prob = _mirror().prioritized_draws(tree, seed, k, 128)
        assert np.array_equal(_np(b["index"]), idx) and np.array_equal(_np(b["prob"]), prob)
        w = (size * prob.astype(np.float64)) ** -beta_k
        w = (w / w.max()).astype(np.float32)
        assert np.allclose(_np(b["weight"]), w, rtol=1e-6, atol=0)
        out = policy_net(b["obs"])
        a = b["action"].long().unsqueeze(1)
        q = (out.gather(1, a // 10) + out.gather(1, 4 + a % 10)).squeeze(1)
        loss = (torch.from_numpy(w).to(DEV) * torch.nn.functional.smooth_l1_loss(q, b["y"], reduction="none")).mean()
        optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(policy_net.parameters(), 100)
        optimizer.step()
        target_sd, policy_sd = target_net.state_dict(), policy_net.state_dict()
        for key in policy_sd:
            target_sd[key] = policy_sd[key] * tau + target_sd[key] * (1 - tau)
        target_net.load_state_dict(target_sd)
        for mine, ref in ((learner.model, policy_net), (learner.target, target_net)):
            for p, r in zip(mine.parameters(), ref.parameters()):
                assert torch.allclose(p, r, rtol=1e-6, atol=1e-8), k
        # the written-back priorities: (|q - y| + eps)^alpha of the update's own forward pass, clamped, largest of duplicates
        assert torch.allclose(b["q"], q.detach(), rtol=1e-5, atol=1e-6)
        written = _np((b["q"] - b["y"]).double().abs().add(eps).pow(alpha))
        _mirror().priority_tree_update(tree, idx, written)
        _assert_tree(learner.ring, tree, f"update {k}")
    # a write-back after a push is refused
    learner.collect(1)
    with pytest.raises(ValueError, match="pushed"):
        learner.ring.update_priorities(learner.last["index"], torch.ones(128, dtype=torch.float64, device=DEV))
    env.terminate()


def test_alpha_zero_is_uniform_with_unit_weights():
    env = _env(2, 2, 1000, seed=2)
    learner = T.DQNLearner(env, model=_model(1), capacity=3000, batch_size=256, seed=5, prioritized=True, alpha=0.0)
    learner.collect(3)
    for _ in range(3):
        learner.update(1)
        b = learner.last
        assert torch.equal(b["prob"], torch.full_like(b["prob"], np.float32(1.0 / learner.ring.size)))
        assert torch.equal(b["weight"], torch.ones_like(b["weight"]))
    assert torch.equal(learner.ring.priorities()[:3000], torch.ones(3000, dtype=torch.float64, device=DEV))
    env.terminate()


def test_uniform_learner_allocates_no_tree():
    env = _env(2, 2, 256, seed=1)
    learner = T.DQNLearner(env, capacity=1024, batch_size=64)
    assert type(learner.ring) is T.ReplayRing and not hasattr(learner.ring, "tree")
    learner.collect(1)
    learner.update(1)
    assert "weight" not in learner.last and "prob" not in learner.last
    env.terminate()


# ------------------------------------------------------------------------------------------------ 6. it learns with PER
def _train_per(task, seed, n=4096):
    L, M, reward, rounds, per_round = TASKS[task]
    rows, pieces = T.generate_configs(L, M, 64, seed=100 + seed)
    env = _env(L, M, n, seed=seed, pool=(rows, pieces), reward=reward)
    learner = T.DQNLearner(env, model=_model(seed), capacity=1 << 16, batch_size=1024, eps_start=1.0, eps_end=0.05,
                           eps_decay=10, tau=0.05, lr=1e-3, seed=seed, prioritized=True)
    random_rate = learner.evaluate(4 * M, epsilon=1.0)["win_rate"]
    for _ in range(rounds):
        learner.collect(1)
        if learner.ring.size >= learner.batch_size:
            learner.update(per_round)
    greedy = learner.evaluate(4 * M)
    env.terminate()
    return random_rate, greedy["win_rate"], greedy["episodes"]


@pytest.mark.parametrize("task", sorted(TASKS))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_it_learns_with_prioritized_replay(task, seed):
    """test_learner_gpu.test_it_learns's budget and floors, with prioritized=True (alpha 0.6, beta 0.4 -> 1)."""
    random_rate, greedy, episodes = _train_per(task, seed)
    factor, floor = THRESHOLDS[task]
    print(f"{task} seed {seed} PER: random {random_rate:.4f} greedy {greedy:.4f} over {episodes} episodes")
    assert episodes > 1000
    assert greedy >= floor and greedy >= factor * max(random_rate, 1e-3)
