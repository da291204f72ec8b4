"""n-step returns on one MI355X (include/tpl_learn.h's rule, tpl_replay_sample_nstep, ReplayRing.sample(n_step=...),
DQNLearner(n_step=...)):

  * n_step = 1 through the new entry point is tpl_replay_sample / tpl_replay_sample_prioritized bit for bit;
  * on written rings (65,537 slots / stride 1,000 and 257 slots / stride 16) every output equals _learn_lib.nstep_targets
    bit for bit, canaries around every output intact, with each of the three endings drawn at least 20 times per batch;
  * on recorded rollouts the return, done, discount, steps and s' equal a restatement that walks the trajectories in time;
  * DQNLearner(n_step=3) updates equal a plain-torch restatement whose y comes from the mirror (uniform and prioritized,
    the written-back priorities included), and the learner still learns the two small tasks.
"""
import copy

import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from test_learn_range_gpu import DeviceTree, Framed, _check, _lib, _stream, _synthetic_ring
from test_learner_gpu import _env, _model, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = 0, 1
GAMMAS = [0.0, 0.5, 0.99, 1.0]
N_STEPS = [2, 3, 5, 16]
BATCH = 4099


def _mirror():
    return T._learn_lib


def _written_ring(cap, seed, M, p_done=0.2):
    """Records of _synthetic_ring (s at the ends of every field, random s' words and actions) with finite random rewards and
    dones at probability p_done."""
    gen = np.random.default_rng(seed)
    rec = _synthetic_ring(gen, cap, M)
    rec[:, 64:68] = (gen.standard_normal(cap) * 10).astype(np.float32).view(np.uint8).reshape(cap, 4)
    rec[:, 69] = (gen.random(cap) < p_done).astype(np.uint8)
    return rec


def _device_tree(cap, size, seed):
    """A tree whose first `size` leaves hold random priorities (device and mirror, checked against each other)."""
    tree = DeviceTree(cap)
    tree.push(0, size)
    gen = np.random.default_rng(seed)
    tree.update(np.arange(size), gen.random(size) * 10 + 0.1, "random priorities")
    return tree


def _sample_nstep(ring, tree, cap, size, head, stride, n_step, gamma, batch, seed, update, L, M, dtype):
    """tpl_replay_sample_nstep into canary-framed outputs; returns them as host arrays after checking every canary."""
    esize = 4 if dtype == F32 else 2
    out = dict(obs=Framed(batch * 217 * esize, 1), next_a=Framed(batch * 16, 2), next_b=Framed(batch * 16, 3),
               action=Framed(batch, 4), ret=Framed(batch * 4, 5), discount=Framed(batch * 4, 6), done=Framed(batch, 7),
               steps=Framed(batch, 8), index=Framed(batch * 8, 9))
    if tree is not None:
        out["prob"] = Framed(batch * 4, 10)
    _check(_lib().tpl_replay_sample_nstep(
        ring.data_ptr(), None if tree is None else tree.dev.ptr(), cap, size, head, stride, n_step, gamma, batch, seed, update,
        L, M, out["obs"].ptr(), dtype, out["next_a"].ptr(), out["next_b"].ptr(), out["action"].ptr(), out["ret"].ptr(),
        out["discount"].ptr(), out["done"].ptr(), out["steps"].ptr(), out["index"].ptr(),
        out["prob"].ptr() if tree is not None else None, _stream()))
    for k, o in out.items():
        o.assert_canary((k, n_step, gamma))
    host = {k: o.host() for k, o in out.items()}
    host["obs"] = host["obs"].view(np.uint32 if dtype == F32 else np.uint16).reshape(batch, 217)
    host["next_a"] = host["next_a"].view(np.uint32).reshape(batch, 4)
    host["next_b"] = host["next_b"].view(np.uint32).reshape(batch, 4)
    host["index"] = host["index"].view(np.int64)
    for k in ("ret", "discount", "prob"):
        if k in host:
            host[k] = host[k].view(np.float32)
    return host


def _obs_bits(obs64, dtype):
    if dtype == F32:
        return obs64.astype(np.float32).view(np.uint32)
    return torch.from_numpy(obs64).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------ 1. n_step = 1
@pytest.mark.parametrize("mode", ["uniform", "prioritized"])
def test_n_step_one_is_the_existing_sampler_bit_for_bit(mode):
    cap, L, M, stride, seed = 4500, 5, 20, 100, 21
    rec = _written_ring(cap, 3, M, p_done=0.5)
    ring = torch.from_numpy(rec.reshape(-1)).to(DEV)
    for size, head in ((cap, 1234), (2000, 2000)):
        tree = _device_tree(cap, size, size) if mode == "prioritized" else None
        for batch, dtype, update in ((4099, F32, 0), (777, BF16, 1), (64, F32, 2)):
            for gamma in (0.99, 0.5):
                esize = 4 if dtype == F32 else 2
                bufs = [dict(obs=torch.empty(batch * 217 * esize, dtype=torch.uint8, device=DEV),
                             next_a=torch.empty(batch * 16, dtype=torch.uint8, device=DEV),
                             next_b=torch.empty(batch * 16, dtype=torch.uint8, device=DEV),
                             action=torch.empty(batch, dtype=torch.uint8, device=DEV),
                             reward=torch.empty(batch * 4, dtype=torch.uint8, device=DEV),
                             done=torch.empty(batch, dtype=torch.uint8, device=DEV),
                             index=torch.empty(batch * 8, dtype=torch.uint8, device=DEV),
                             prob=torch.empty(batch * 4, dtype=torch.uint8, device=DEV)) for _ in range(2)]
                old, new = bufs
                for b in bufs:                                # different garbage in each, so nothing matches by accident
                    for t in b.values():
                        t.random_(0, 256)
                disc = torch.empty(batch, dtype=torch.float32, device=DEV)
                steps = torch.empty(batch, dtype=torch.uint8, device=DEV)
                p = lambda b, k: b[k].data_ptr()
                if tree is None:
                    _check(_lib().tpl_replay_sample(ring.data_ptr(), cap, size, batch, seed, update, L, M, p(old, "obs"), dtype,
                                                    p(old, "next_a"), p(old, "next_b"), p(old, "action"), p(old, "reward"),
                                                    p(old, "done"), p(old, "index"), _stream()))
                else:
                    _check(_lib().tpl_replay_sample_prioritized(
                        ring.data_ptr(), tree.dev.ptr(), cap, size, batch, seed, update, L, M, p(old, "obs"), dtype,
                        p(old, "next_a"), p(old, "next_b"), p(old, "action"), p(old, "reward"), p(old, "done"),
                        p(old, "index"), p(old, "prob"), _stream()))
                _check(_lib().tpl_replay_sample_nstep(
                    ring.data_ptr(), None if tree is None else tree.dev.ptr(), cap, size, head, stride, 1, gamma, batch, seed,
                    update, L, M, p(new, "obs"), dtype, p(new, "next_a"), p(new, "next_b"), p(new, "action"),
                    p(new, "reward"), disc.data_ptr(), p(new, "done"), steps.data_ptr(), p(new, "index"),
                    None if tree is None else p(new, "prob"), _stream()))
                torch.cuda.synchronize()
                what = (mode, size, batch, dtype, gamma)
                for k in old:
                    if k == "prob" and tree is None:
                        continue
                    assert torch.equal(old[k], new[k]), (what, k)
                d = _np(new["done"])
                want = np.where(d != 0, np.float32(0.0), np.float32(gamma)).astype(np.float32)
                assert np.array_equal(_np(disc).view(np.uint32), want.view(np.uint32)), what
                assert (_np(steps) == 1).all(), what
                assert (d == 0).any() and (d != 0).any(), what


# ------------------------------------------------------------------------------------------------ 2. written rings
RINGS = {"large": (65537, 1000, [(65537, 12345), (40000, 40000)]), "small": (257, 16, [(257, 100), (200, 200)])}


@pytest.mark.parametrize("mode", ["uniform", "prioritized"])
@pytest.mark.parametrize("which", sorted(RINGS))
def test_written_ring_equals_the_mirror(which, mode):
    cap, stride, shapes = RINGS[which]
    L, M, seed = 5, 20, 17
    rec = _written_ring(cap, 0, M)
    dec = R.decode_records(rec)
    obs_all = R.obs_from_fields(dec["s"], L, M)
    ring = torch.from_numpy(rec.reshape(-1)).to(DEV)
    calls = 0
    for size, head in shapes:
        tree = _device_tree(cap, size, size + 1) if mode == "prioritized" else None
        for n_step in N_STEPS:
            for gamma in GAMMAS:
                update, dtype = calls, (F32, BF16)[calls % 2]
                calls += 1
                got = _sample_nstep(ring, tree, cap, size, head, stride, n_step, gamma, BATCH, seed, update, L, M, dtype)
                if tree is None:
                    idx = _mirror().replay_indices(seed, update, BATCH, size)
                else:
                    idx, prob = _mirror().prioritized_draws(tree.mirror, seed, update, BATCH)
                    assert np.array_equal(got["prob"].view(np.uint32), prob.view(np.uint32))
                ret, disc, done, steps, src = _mirror().nstep_targets(rec, cap, size, head, stride, idx, n_step, gamma)
                what = (which, mode, size, head, n_step, gamma)
                assert np.array_equal(got["index"], idx), what
                assert np.array_equal(got["ret"].view(np.uint32), ret.view(np.uint32)), what
                assert np.array_equal(got["discount"].view(np.uint32), disc.view(np.uint32)), what
                assert np.array_equal(got["done"], done), what
                assert np.array_equal(got["steps"], steps), what
                assert np.array_equal(got["next_a"], dec["na"][src]), what
                assert np.array_equal(got["next_b"], dec["nb"][src]), what
                assert np.array_equal(got["action"], dec["action"][idx]), what
                assert np.array_equal(got["obs"], _obs_bits(obs_all[idx], dtype)), what
                if which == "large" and mode == "uniform":
                    full = int((steps == n_step).sum())
                    by_done = int(((steps < n_step) & (done != 0)).sum())
                    by_head = int(((steps < n_step) & (done == 0)).sum())
                    print(f"{what}: full {full} done {by_done} head {by_head}")
                    assert min(full, by_done, by_head) >= 20, (what, full, by_done, by_head)
                if which == "small" and mode == "uniform":
                    assert np.unique(idx).size == size, what                     # every slot drawn


# ------------------------------------------------------------------------------------------------ 3. recorded rollouts
@pytest.mark.parametrize("L,M", [(5, 20), (2, 2)])
def test_recorded_rollouts_equal_the_time_walk(L, M):
    """Three pushes of 2 x 1000 transitions into a ring of 4500 (the third wraps).  Each draw is followed in time: board i from
    step tau on, while the step was recorded, stopping after a done; s' is the state recorded at tau + K, or the resident
    planes after the last push."""
    n, steps_per, cap, n_step, gamma = 1000, 2, 4500, 3, 0.99
    env = _env(L, M, n, seed=3)
    image = T.actor.policy_image(_model(0), env.device, f32="split")
    ring = T.ReplayRing(cap, env.device)
    sa, sb, r, d, a = [], [], [], [], []
    for push in range(3):
        traj = env.actor_rollout(image, steps_per, epsilon=0.3, seed=11, step0=push * steps_per, record=True,
                                 record_states=True)
        ring.push(env, traj)
        sa += list(_np(traj["states_a"]))
        sb += list(_np(traj["states_b"]))
        r += list(_np(traj["rewards"]))
        d += list(_np(traj["dones"]).astype(np.uint8))
        a += list(_np(traj["actions"]))
    after = [_np(x) for x in env.raw_planes()]
    sa, sb = np.stack(sa + [after[0]]), np.stack(sb + [after[1]])             # [7, n, 4]: the state at every step tau
    r, d, a = np.stack(r), np.stack(d), np.stack(a)                            # [6, n]
    total = 6 * n
    assert ring.head == total % cap and ring.size == cap and ring.stride == n
    gam = np.float32(gamma)
    for batch, dtype, update in ((4096, torch.float32, 0), (777, torch.bfloat16, 1)):
        next_env = T.BatchedTetris(L, M, batch, device=DEV, seed=5)
        got = ring.sample(batch, 9, update, next_env, obs_dtype=dtype, with_index=True, n_step=n_step, gamma=gamma)
        idx = _np(got["index"])
        assert np.array_equal(idx, _mirror().replay_indices(9, update, batch, cap))
        want = dict(ret=[], disc=[], done=[], steps=[], tau=[], i=[], last=[])
        for j in idx:
            g = int(j) + cap * ((total - 1 - int(j)) // cap)
            tau, i = divmod(g, n)
            ret, gk, k_last = np.float32(r[tau, i]), np.float32(1.0), 0
            if not d[tau, i]:
                for k in range(1, n_step):
                    if tau + k > 5:                                            # step tau + k was not recorded yet
                        break
                    gk = np.float32(gk * gam)
                    ret = np.float32(ret + np.float32(gk * r[tau + k, i]))
                    k_last = k
                    if d[tau + k, i]:
                        break
            dn = d[tau + k_last, i]
            want["ret"].append(ret)
            want["done"].append(dn)
            want["disc"].append(np.float32(0.0) if dn else np.float32(gk * gam))
            want["steps"].append(k_last + 1)
            want["tau"].append(tau)
            want["i"].append(i)
        tau, i, K = np.array(want["tau"]), np.array(want["i"]), np.array(want["steps"])
        ref = env.expand_states(torch.from_numpy(sa[tau, i]).to(DEV), torch.from_numpy(sb[tau, i]).to(DEV), dtype=dtype)
        iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert torch.equal(got["obs"].view(iv), ref.view(iv))
        assert np.array_equal(_np(got["action"]), a[tau, i])
        assert np.array_equal(_np(got["reward"]).view(np.uint32), np.array(want["ret"], np.float32).view(np.uint32))
        assert np.array_equal(_np(got["discount"]).view(np.uint32), np.array(want["disc"], np.float32).view(np.uint32))
        assert np.array_equal(_np(got["done"]), np.array(want["done"], np.uint8))
        assert np.array_equal(_np(got["steps"]), K.astype(np.uint8))
        na, nb = next_env.raw_planes()
        assert np.array_equal(_np(na), sa[tau + K, i]) and np.array_equal(_np(nb), sb[tau + K, i])
        ended = np.array(want["done"]) != 0
        print(f"L={L} M={M} batch {batch}: K=3 {(K == 3).sum()}, ended by done {ended.sum()}, cut by the head "
              f"{((K < 3) & ~ended).sum()}")
        if M == 2:                         # a game of at most two moves: no return runs three, most end by done
            assert (K <= 2).all() and ended.mean() > 0.75
        else:
            assert (K == 3).any() and ended.any() and ((K < 3) & ~ended).any()
        next_env.terminate()
    # a push from a second environment leaves 1-step sampling alone and refuses n-step sampling
    other = _env(L, M, n, seed=4)
    ring.push(other, other.actor_rollout(image, 1, record=True, record_states=True))
    next_env = T.BatchedTetris(L, M, 64, device=DEV, seed=5)
    ring.sample(64, 1, 0, next_env)
    with pytest.raises(ValueError, match="one environment"):
        ring.sample(64, 1, 0, next_env, n_step=2, gamma=0.9)
    next_env.terminate()
    other.terminate()
    env.terminate()


# ------------------------------------------------------------------------------------------------ 4. the learner
@pytest.mark.parametrize("prioritized", [False, True])
def test_nstep_updates_equal_a_plain_torch_restatement(prioritized):
    L, M, n = 5, 20, 1024
    env = _env(L, M, n, seed=6)
    tau, lr, alpha, beta, eps, seed, gamma, n_step, cap, B = 0.005, 1e-4, 0.6, 0.4, 1e-6, 2, 0.99, 3, 1 << 14, 128
    learner = T.DQNLearner(env, model=_model(8), capacity=cap, batch_size=B, tau=tau, lr=lr, seed=seed, gamma=gamma,
                           prioritized=prioritized, alpha=alpha, beta=beta, beta_final=1.0, beta_updates=10,
                           priority_eps=eps, n_step=n_step)
    assert learner.n_step == n_step
    learner.collect(6)
    size, head = learner.ring.size, learner.ring.head
    records = _np(learner.ring.data).reshape(cap, 80)
    dec = R.decode_records(records)
    if prioritized:
        tree = _mirror().priority_tree_push(_mirror().priority_tree_init(cap), 0, size)
    policy_net = copy.deepcopy(learner.model)
    target_net = copy.deepcopy(learner.target)
    optimizer = torch.optim.AdamW(policy_net.parameters(), lr=lr, amsgrad=True)
    criterion = torch.nn.SmoothL1Loss()
    fmax = T.learn.factored_max
    for k in range(3):
        learner.update(1)
        b = learner.last
        if prioritized:
            idx, prob = _mirror().prioritized_draws(tree, seed, k, B)
            assert np.array_equal(_np(b["prob"]).view(np.uint32), prob.view(np.uint32))
        else:
            idx = _mirror().replay_indices(seed, k, B, size)
        assert np.array_equal(_np(b["index"]), idx)
        ret, disc, done, steps, src = _mirror().nstep_targets(records, cap, size, head, n, idx, n_step, gamma)
        assert np.array_equal(_np(b["reward"]).view(np.uint32), ret.view(np.uint32))
        assert np.array_equal(_np(b["discount"]).view(np.uint32), disc.view(np.uint32))
        assert np.array_equal(_np(b["done"]), done) and np.array_equal(_np(b["steps"]), steps)
        na, nb = learner.next_env.raw_planes()
        assert np.array_equal(_np(na).view(np.uint32), dec["na"][src]) and np.array_equal(_np(nb).view(np.uint32), dec["nb"][src])
        y = torch.from_numpy(ret).to(DEV) + torch.from_numpy(disc).to(DEV) * fmax(b["next_q"])
        assert torch.equal(b["y"], y), k
        out = policy_net(b["obs"])
        a = b["action"].long().unsqueeze(1)
        q = (out.gather(1, a // 10) + out.gather(1, 4 + a % 10)).squeeze(1)
        if prioritized:
            beta_k = beta + (1.0 - beta) * min(1.0, k / 10)
            w = (size * prob.astype(np.float64)) ** -beta_k
            w = (w / w.max()).astype(np.float32)
            assert np.allclose(_np(b["weight"]), w, rtol=1e-6, atol=0)
            loss = (torch.from_numpy(w).to(DEV) * torch.nn.functional.smooth_l1_loss(q, y, reduction="none")).mean()
        else:
            loss = criterion(q, y)
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
        if prioritized:                                       # written back: (|q - y| + eps)^alpha of the n-step y
            assert torch.allclose(b["q"], q.detach(), rtol=1e-5, atol=1e-6)
            written = _np((b["q"] - y).double().abs().add(eps).pow(alpha))
            _mirror().priority_tree_update(tree, idx, written)
            got = _np(learner.ring.tree.view(torch.int64))
            bad = np.flatnonzero(got != tree.view(np.int64))
            assert bad.size == 0, (k, bad[:8])
    assert (steps > 1).any() and (steps < n_step).any()
    env.terminate()


def test_the_learner_refuses_gamma_outside_the_unit_interval_with_n_steps():
    env = _env(2, 2, 256)
    with pytest.raises(ValueError, match="gamma"):
        T.DQNLearner(env, capacity=1000, batch_size=64, gamma=1.01, n_step=2)
    with pytest.raises(ValueError, match="n_step"):
        T.DQNLearner(env, capacity=1000, batch_size=64, n_step=17)
    learner = T.DQNLearner(env, capacity=1000, batch_size=64, gamma=1.01)      # n_step = 1: as before
    assert learner.n_step == 1
    env.terminate()


# ------------------------------------------------------------------------------------------------ 5. it learns
# Copied from tests/test_learner_gpu.py (TASKS, THRESHOLDS and train_task's budget, for test_it_learns): the same tasks, the
# same budget, the same thresholds.
TASKS = {
    "bandit": (1, 1, (1.0, 0.0, 0.0), 40, 10),
    "two_moves": (2, 2, (0.0, 1.0, 0.0), 60, 10),
}
THRESHOLDS = {"bandit": (5.0, 0.5), "two_moves": (10.0, 0.4)}


def train_task(task, seed, n_step, n=4096):
    L, M, reward, rounds, per_round = TASKS[task]
    rows, pieces = T.generate_configs(L, M, 64, seed=100 + seed)
    env = _env(L, M, n, seed=seed, pool=(rows, pieces), reward=reward)
    learner = T.DQNLearner(env, model=_model(seed), capacity=1 << 16, batch_size=1024, eps_start=1.0, eps_end=0.05,
                           eps_decay=10, tau=0.05, lr=1e-3, seed=seed, n_step=n_step)
    random_rate = learner.evaluate(4 * M, epsilon=1.0)["win_rate"]
    for _ in range(rounds):
        learner.collect(1)
        if learner.ring.size >= learner.batch_size:
            learner.update(per_round)
    greedy = learner.evaluate(4 * M)
    env.terminate()
    return random_rate, greedy["win_rate"], greedy["episodes"]


@pytest.mark.parametrize("n_step", [2, 3])
@pytest.mark.parametrize("task", sorted(TASKS))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_it_learns_with_n_step_returns(task, seed, n_step):
    random_rate, greedy, episodes = train_task(task, seed, n_step)
    factor, floor = THRESHOLDS[task]
    print(f"{task} n_step {n_step} seed {seed}: random {random_rate:.4f} greedy {greedy:.4f} over {episodes} episodes")
    assert episodes > 1000
    assert greedy >= floor and greedy >= factor * max(random_rate, 1e-3)
