"""The DQN learner on one MI355X: the replay ring's push and sample are exact (against the recorded trajectory and
env.expand_states), the device packers equal the host packers byte for byte, the target network's Q'(s') on the split kernel
is float32-grade, one update is the tutorial's optimize_model step, and the learner learns two small tasks."""
import copy

import numpy as np
import pytest
import torch

import tetris_piclim as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().numpy()


def _params_np(model):
    layers = [model.layer1, model.layer2, model.layer3, model.layer4, model.layer5]
    return [(_np(l.weight).astype(np.float32), _np(l.bias).astype(np.float32)) for l in layers]


def _model(seed, device=DEV):
    torch.manual_seed(seed)
    return T.PolicyMLP().to(device)


def _env(L, M, n, seed=1, pool=None, reward=(1.0, 0.0, 0.0)):
    env = T.BatchedTetris(L, M, n, device=DEV, seed=seed, auto_reset=True, reward=reward)
    if pool is None:
        rows, pieces = env.synthetic_configs(512)
    else:
        rows, pieces = pool
    env.load_configs(rows, pieces)
    env.reset()
    return env


# ------------------------------------------------------------------------------------------------ 1. push / sample
def test_push_and_sample_are_exact_across_a_wrapped_ring():
    """Three pushes of 2 x 1000 transitions into a ring of 4500: the third wraps.  Every drawn slot is the host mirror's,
    every sampled field equals what the recorded trajectory says that slot holds, obs bit for bit as env.expand_states."""
    L, M, n, steps, cap = 5, 20, 1000, 2, 4500
    env = _env(L, M, n, seed=3)
    image = T.actor.policy_image(_model(0), env.device, f32="split")
    ring = T.ReplayRing(cap, env.device)
    want = {k: [None] * cap for k in ("sa", "sb", "na", "nb", "a", "r", "d")}
    prev_after = None
    for push in range(3):
        traj = env.actor_rollout(image, steps, epsilon=0.3, seed=11, step0=push * steps, record=True, record_states=True)
        after_a, after_b = env.raw_planes()
        if prev_after is not None:          # the recorded planes and the resident planes are one layout
            assert torch.equal(traj["states_a"][0], prev_after[0]) and torch.equal(traj["states_b"][0], prev_after[1])
        prev_after = (after_a, after_b)
        head = ring.head
        ring.push(env, traj)
        sa, sb = _np(traj["states_a"]), _np(traj["states_b"])
        a, r, d = _np(traj["actions"]), _np(traj["rewards"]), _np(traj["dones"]).astype(np.uint8)
        for t in range(steps):
            na = sa[t + 1] if t + 1 < steps else _np(after_a)
            nb = sb[t + 1] if t + 1 < steps else _np(after_b)
            for i in range(n):
                slot = (head + t * n + i) % cap
                want["sa"][slot], want["sb"][slot], want["na"][slot], want["nb"][slot] = sa[t, i], sb[t, i], na[i], nb[i]
                want["a"][slot], want["r"][slot], want["d"][slot] = a[t, i], r[t, i], d[t, i]
        assert ring.head == (head + steps * n) % cap
    assert ring.size == cap and ring.head == 6000 % cap
    for batch, dtype, update in ((777, torch.float32, 3), (4096, torch.bfloat16, 4), (64, torch.float32, 0)):
        next_env = T.BatchedTetris(L, M, batch, device=DEV, seed=5)
        got = ring.sample(batch, 9, update, next_env, obs_dtype=dtype, with_index=True)
        idx = T._learn_lib.replay_indices(9, update, batch, cap)
        assert np.array_equal(_np(got["index"]), idx)
        sa = torch.from_numpy(np.stack([want["sa"][k] for k in idx])).to(DEV)
        sb = torch.from_numpy(np.stack([want["sb"][k] for k in idx])).to(DEV)
        ref = env.expand_states(sa, sb, dtype=dtype)
        assert got["obs"].dtype == dtype and torch.equal(got["obs"].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                                         ref.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
        na, nb = next_env.raw_planes()
        assert np.array_equal(_np(na), np.stack([want["na"][k] for k in idx]))
        assert np.array_equal(_np(nb), np.stack([want["nb"][k] for k in idx]))
        assert np.array_equal(_np(got["action"]), np.array([want["a"][k] for k in idx]))
        assert np.array_equal(_np(got["reward"]).view(np.uint32), np.array([want["r"][k] for k in idx]).view(np.uint32))
        assert np.array_equal(_np(got["done"]), np.array([want["d"][k] for k in idx]))
        next_env.terminate()
    # a draw is uniform over the filled part only: a fresh ring with one push of 2 x 1000 draws below 2000
    small = T.ReplayRing(cap, env.device)
    small.push(env, env.actor_rollout(image, steps, record=True, record_states=True))
    next_env = T.BatchedTetris(L, M, 4096, device=DEV, seed=5)
    assert int(small.sample(4096, 1, 0, next_env, with_index=True)["index"].max()) < steps * n
    env.terminate()


# ------------------------------------------------------------------------------------------------ 2. device packing
def _tie_weights(gen, shape):
    """float32 values whose bf16 rounding is an exact tie (low 16 bits 0x8000, both parities of bit 16), ties one piece
    further down (the split's second piece), random patterns, zeros of both signs and a few subnormals."""
    n = int(np.prod(shape))
    exp = gen.integers(100, 130, n).astype(np.uint32)
    mant = gen.integers(0, 1 << 23, n).astype(np.uint32)
    sign = gen.integers(0, 2, n).astype(np.uint32)
    kind = gen.integers(0, 5, n)
    mant = np.where(kind == 0, (mant & ~np.uint32(0xFFFF)) | np.uint32(0x8000), mant)
    mant = np.where(kind == 1, (mant & ~np.uint32(0xFF)) | np.uint32(0x80), mant)
    bits = (sign << np.uint32(31)) | (exp << np.uint32(23)) | mant
    bits = np.where(kind == 2, gen.integers(0, 1 << 23, n).astype(np.uint32) | (sign << np.uint32(31)), bits)   # subnormal
    bits[:4] = [0, 0x80000000, 1, 0x80000001]
    return bits.view(np.float32).reshape(shape)


@pytest.mark.parametrize("weights", ["random", "ties"])
def test_device_pack_equals_the_host_pack_byte_for_byte(weights):
    model = _model(7)
    if weights == "ties":
        gen = np.random.default_rng(5)
        with torch.no_grad():
            for p in model.parameters():
                p.copy_(torch.from_numpy(_tie_weights(gen, tuple(p.shape))))
    else:
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(torch.exp(torch.randn_like(p)))          # spread the exponents
    params = _params_np(model)
    tensors = T._learn_lib.policy_tensors(model)
    for kind, host_kind in (("bf16", False), ("f32", True), ("split", "split")):
        dev = T._learn_lib.pack_policy_device(tensors, kind)
        host = T.pack_policy(params, f32=host_kind)
        got = _np(dev)
        assert got.shape == host.shape, kind
        bad = np.flatnonzero(got != host)
        assert bad.size == 0, (kind, bad[:8], got[bad[:8]], host[bad[:8]])


# ------------------------------------------------------------------------------------------------ 3. target logits
def test_target_logits_are_float32_grade_and_y_is_the_formula():
    L, M, n = 2, 2, 2048                                    # M = 2: the minibatch holds finished episodes too
    env = _env(L, M, n, seed=2)
    learner = T.DQNLearner(env, model=_model(3), capacity=1 << 14, batch_size=1000, seed=4)
    with torch.no_grad():                                   # a target net that is not the online net
        for p in learner.target.parameters():
            p.add_(0.05 * torch.randn_like(p))
    T._learn_lib.pack_policy_device(T._learn_lib.policy_tensors(learner.target), "split", out=learner.target_image)
    learner.collect(3)
    mb = learner.minibatch()
    obs_next = learner.next_env.observe(torch.float32).double()
    target64 = copy.deepcopy(learner.target).double()
    with torch.no_grad():
        ref = target64(obs_next)
    tol = 2e-5 * (1 + float(ref.abs().max()))
    assert float((mb["next_q"].double() - ref).abs().max()) <= tol
    q = mb["next_q"].double()
    y64 = mb["reward"].double() + 0.99 * (1 - mb["done"].double()) * (q[:, :4].max(1).values + q[:, 4:].max(1).values)
    assert torch.allclose(mb["y"].double(), y64, rtol=1e-6, atol=1e-6)
    assert bool((mb["done"] == 1).any()) and bool((mb["done"] == 0).any())     # both branches of the formula were exercised
    env.terminate()


def test_learner_refuses_what_it_cannot_learn_from():
    env = T.BatchedTetris(2, 2, 256, device=DEV, seed=1, auto_reset=False)
    with pytest.raises(ValueError, match="auto_reset"):
        T.DQNLearner(env)
    env.terminate()
    env = _env(2, 2, 256)
    learner = T.DQNLearner(env, capacity=1000, batch_size=512)
    with pytest.raises(ValueError, match="capacity"):
        learner.collect(4)                                  # 4 x 256 > 1000
    learner.collect(1)
    with pytest.raises(ValueError, match="batch_size"):
        learner.update()                                    # 256 < 512 transitions
    learner.collect(2)
    learner.update()
    env.terminate()


# ------------------------------------------------------------------------------------------------ 4. one update
def test_updates_equal_the_tutorial_step():
    L, M, n = 5, 20, 1024
    env = _env(L, M, n, seed=6)
    tau, lr = 0.005, 1e-4
    learner = T.DQNLearner(env, model=_model(8), capacity=1 << 14, batch_size=128, tau=tau, lr=lr, seed=2)
    learner.collect(4)
    policy_net = copy.deepcopy(learner.model)
    target_net = copy.deepcopy(learner.target)
    optimizer = torch.optim.AdamW(policy_net.parameters(), lr=lr, amsgrad=True)
    criterion = torch.nn.SmoothL1Loss()
    for k in range(3):
        learner.update(1)
        b = learner.last
        out = policy_net(b["obs"])
        a = b["action"].long().unsqueeze(1)
        state_action_values = out.gather(1, a // 10) + out.gather(1, 4 + a % 10)
        loss = criterion(state_action_values, b["y"].unsqueeze(1))
        optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(policy_net.parameters(), 100)
        optimizer.step()
        target_sd, policy_sd = target_net.state_dict(), policy_net.state_dict()
        for key in policy_sd:
            target_sd[key] = policy_sd[key] * tau + target_sd[key] * (1 - tau)
        target_net.load_state_dict(target_sd)
        if k in (0, 2):
            for mine, ref in ((learner.model, policy_net), (learner.target, target_net)):
                for p, q in zip(mine.parameters(), ref.parameters()):
                    assert torch.allclose(p, q, rtol=1e-6, atol=1e-8), k
            # the target image is the split pack of the target parameters
            assert np.array_equal(_np(learner.target_image), T.pack_policy(_params_np(learner.target), f32="split"))
    env.terminate()


# ------------------------------------------------------------------------------------------------ 5. it learns
TASKS = {
    # (L, M, reward, rounds, updates per round): hyperparameters other than the reference's -- lr 1e-3, batch 1024, tau 0.05,
    # epsilon from 1.0 to 0.05 over ~10 lockstep iterations -- so that a few seconds of training show the effect
    "bandit": (1, 1, (1.0, 0.0, 0.0), 40, 10),
    "two_moves": (2, 2, (0.0, 1.0, 0.0), 60, 10),
}
# (factor over the random policy, absolute floor) for the greedy win rate after training.  Measured on an MI355X, seeds 0 / 1 / 2:
#   bandit     random (epsilon 1) 0.070 / 0.071 / 0.065   greedy 1.000 / 0.986 / 0.986
#   two_moves  random (epsilon 1) 0.026 / 0.022 / 0.028   greedy 0.771 / 0.766 / 0.836   (1.000 after 200 rounds of 20 updates)
# The thresholds sit about half-way between random and reached: floors 0.5 and 0.4, factors 5 and 10 (reached: 14 and 30).
THRESHOLDS = {"bandit": (5.0, 0.5), "two_moves": (10.0, 0.4)}


def train_task(task, seed, n=4096):
    L, M, reward, rounds, per_round = TASKS[task]
    rows, pieces = T.generate_configs(L, M, 64, seed=100 + seed)
    env = _env(L, M, n, seed=seed, pool=(rows, pieces), reward=reward)
    learner = T.DQNLearner(env, model=_model(seed), capacity=1 << 16, batch_size=1024, eps_start=1.0, eps_end=0.05,
                           eps_decay=10, tau=0.05, lr=1e-3, seed=seed)
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
def test_it_learns(task, seed):
    """Greedy win rate after a fixed budget against the random policy on the same pool of 64 carved configurations.

    bandit: L=1, M=1, a reward per line -- one move decides, s' is never used.  two_moves: L=2, M=2, reward only for a win --
    the first move earns nothing, its value reaches it only through gamma * max Q'(s').  4096 boards, 40 / 60 rounds of
    collect(1) + update(10), batch 1024, lr 1e-3, tau 0.05, epsilon 1.0 -> 0.05 with eps_decay 10 (not the reference's
    constants: chosen so that a few seconds of training show the effect).  Measured rates: THRESHOLDS above."""
    random_rate, greedy, episodes = train_task(task, seed)
    factor, floor = THRESHOLDS[task]
    print(f"{task} seed {seed}: random {random_rate:.4f} greedy {greedy:.4f} over {episodes} episodes")
    assert episodes > 1000
    assert greedy >= floor and greedy >= factor * max(random_rate, 1e-3)
