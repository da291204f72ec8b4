"""Mirror-symmetry augmentation on one MI355X (include/tpl_learn.h's rule, tpl_replay_sample_mirror, tpl_mirror_states,
ReplayRing.sample(mirror=...), DQNLearner(mirror=True)):

  * mode 2, in each of the four draw forms, float32 and bf16, batches 1 .. 65,537: obs is the mode-0 obs permuted by
    MIRROR_OBS_PERM, the s' planes are mirror_states of the mode-0 planes, action is mirror_actions, every other output is
    identical, `mirrored` is all ones, canaries around every output intact;
  * mode 1: `mirrored` is mirror_coins, each draw equals its mode-0 or its mode-2 counterpart accordingly, index is the
    existing sampler's; mode 0 through the new entry is the existing entry byte for byte;
  * tpl_mirror_states is the numpy mirror, and the HIP step path commutes with it: a batch of states and their mirrors,
    stepped with actions and mirrored actions, give the same reward and done and mirrored boards;
  * DQNLearner(mirror=True) collects and updates: last["mirrored"] is that update's coins, obs, action and s' are the
    mirrored transition's, and next_q is the target network on the mirrored s'.
"""
import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from test_learn_range_gpu import DeviceTree, Framed, _check, _lib, _stream, _synthetic_ring
from test_learner_gpu import _env, _model, _np, _params_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = 0, 1
BATCHES = [1, 63, 64, 65, 128, 65537]
FORMS = {"uniform": (False, 0), "prioritized": (True, 0), "uniform_nstep": (False, 3), "prioritized_nstep": (True, 3)}
CAP, STRIDE, GAMMA, L, M, SEED = 4500, 100, 0.99, 5, 20, 23
SHAPE = (3000, 3000)                                       # (size, head): a ring that is not full, so n-step draws meet the head


def _m():
    return T._learn_lib


class Ring:
    """A written ring of CAP records (s at the ends of every field, random s' words -- all 256 bits -- random action bytes,
    finite rewards, dones at 0.2) on the device, decoded on the host, with a tree of random priorities."""

    def __init__(self, seed=3):
        gen = np.random.default_rng(seed)
        self.rec = _synthetic_ring(gen, CAP, M)
        self.rec[:, 64:68] = (gen.standard_normal(CAP) * 10).astype(np.float32).view(np.uint8).reshape(CAP, 4)
        self.rec[:, 69] = (gen.random(CAP) < 0.2).astype(np.uint8)
        self.dec = R.decode_records(self.rec)
        self.dev = torch.from_numpy(self.rec.reshape(-1)).to(DEV)
        self.size, self.head = SHAPE
        self.tree = DeviceTree(CAP)
        self.tree.push(0, self.size)
        self.tree.update(np.arange(self.size), gen.random(self.size) * 10 + 0.1, "random priorities")

    def draw(self, form, batch, update, dtype, mirror, entry="mirror"):
        """One minibatch into canary-framed outputs, as host arrays.  entry="mirror": tpl_replay_sample_mirror in mode `mirror`;
        entry="existing": the entry point that form had before (mirror is not passed)."""
        prioritized, n_step = FORMS[form]
        esize = 4 if dtype == F32 else 2
        out = dict(obs=Framed(batch * 217 * esize, 1), next_a=Framed(batch * 16, 2), next_b=Framed(batch * 16, 3),
                   action=Framed(batch, 4), ret=Framed(batch * 4, 5), done=Framed(batch, 7), index=Framed(batch * 8, 9))
        if n_step:
            out.update(discount=Framed(batch * 4, 6), steps=Framed(batch, 8))
        if prioritized:
            out["prob"] = Framed(batch * 4, 10)
        if entry == "mirror":
            out["mirrored"] = Framed(batch, 11, zero=False)
            out["mirrored"].inner().fill_(0xAB)
        p = lambda k: out[k].ptr() if k in out else None
        tree = self.tree.dev.ptr() if prioritized else None
        common = (batch, SEED, update, L, M, p("obs"), dtype, p("next_a"), p("next_b"), p("action"), p("ret"))
        if entry == "mirror":
            _check(_lib().tpl_replay_sample_mirror(self.dev.data_ptr(), tree, CAP, self.size, self.head, STRIDE, n_step, GAMMA,
                                                   *common, p("discount"), p("done"), p("steps"), p("index"), p("prob"), mirror,
                                                   p("mirrored"), _stream()))
        elif n_step:
            _check(_lib().tpl_replay_sample_nstep(self.dev.data_ptr(), tree, CAP, self.size, self.head, STRIDE, n_step, GAMMA,
                                                  *common, p("discount"), p("done"), p("steps"), p("index"), p("prob"), _stream()))
        elif prioritized:
            _check(_lib().tpl_replay_sample_prioritized(self.dev.data_ptr(), tree, CAP, self.size, *common, p("done"), p("index"),
                                                        p("prob"), _stream()))
        else:
            _check(_lib().tpl_replay_sample(self.dev.data_ptr(), CAP, self.size, *common, p("done"), p("index"), _stream()))
        for k, o in out.items():
            o.assert_canary((form, batch, dtype, mirror, entry, k))
        host = {k: o.host() for k, o in out.items()}
        host["obs"] = host["obs"].view(np.uint32 if dtype == F32 else np.uint16).reshape(batch, 217)
        host["next_a"] = host["next_a"].view(np.uint32).reshape(batch, 4)
        host["next_b"] = host["next_b"].view(np.uint32).reshape(batch, 4)
        host["index"] = host["index"].view(np.int64)
        return host

    def slots(self, form, batch, update):
        if FORMS[form][0]:
            return _m().prioritized_draws(self.tree.mirror, SEED, update, batch)[0]
        return _m().replay_indices(SEED, update, batch, self.size)


@pytest.fixture(scope="module")
def ring():
    return Ring()


def _assert_mirrored(ring, plain, got, rows, what):
    """Draws `rows` of `got` are the mirror of the same draws of the mode-0 minibatch `plain`."""
    idx = plain["index"][rows]
    assert np.array_equal(got["obs"][rows], plain["obs"][rows][:, _m().MIRROR_OBS_PERM]), what
    wa, wb = _m().mirror_states(plain["next_a"][rows], plain["next_b"][rows])
    assert np.array_equal(got["next_a"][rows], wa) and np.array_equal(got["next_b"][rows], wb), what
    want = _m().mirror_actions(plain["action"][rows], ring.dec["sa"][idx], ring.dec["sb"][idx])
    assert np.array_equal(got["action"][rows], want), what
    assert (got["action"][rows] < 40).all(), what


def _assert_same(plain, got, rows, keys, what):
    for k in keys:
        assert np.array_equal(got[k][rows], plain[k][rows]), (what, k)


# ------------------------------------------------------------------------------------------------ 6. mode 2
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_mode_two_is_the_mirror_of_every_draw(ring, form, dtype):
    for update, batch in enumerate(BATCHES):
        plain = ring.draw(form, batch, update, dtype, 0)
        got = ring.draw(form, batch, update, dtype, 2)
        what = (form, dtype, batch)
        every = np.arange(batch)
        assert np.array_equal(plain["index"], ring.slots(form, batch, update)), what
        _assert_mirrored(ring, plain, got, every, what)
        others = [k for k in plain if k not in ("obs", "next_a", "next_b", "action", "mirrored")]
        assert {"ret", "done", "index"} <= set(others) and ("steps" in others) == bool(FORMS[form][1])
        _assert_same(plain, got, every, others, what)
        assert (got["mirrored"] == 1).all() and (plain["mirrored"] == 0).all(), what
        if batch >= 128:                                   # the draw is not its own mirror
            assert (got["obs"] != plain["obs"]).any() and (got["next_a"] != plain["next_a"]).any()
            assert (got["action"] != plain["action"]).any()
    if FORMS[form][1]:                                     # the n-step draws took s' from successors, and met dones and the head
        assert (plain["steps"] == 3).any() and (plain["steps"] < 3).any()


# ------------------------------------------------------------------------------------------------ 7. mode 1
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_mode_one_follows_the_coin_and_mode_zero_is_the_existing_entry(ring, form, dtype):
    for update, batch in ((40, 65), (41, 4099), (42, 65537)):
        existing = ring.draw(form, batch, update, dtype, None, entry="existing")
        plain = ring.draw(form, batch, update, dtype, 0)
        coin = ring.draw(form, batch, update, dtype, 1)
        always = ring.draw(form, batch, update, dtype, 2)
        what = (form, dtype, batch)
        for k in existing:                                 # mode 0 through the new entry: the existing entry byte for byte
            assert np.array_equal(existing[k], plain[k]), (what, k)
        assert (plain["mirrored"] == 0).all()
        coins = _m().mirror_coins(SEED, update, batch)
        assert np.array_equal(coin["mirrored"], coins), what
        assert np.array_equal(coin["index"], existing["index"]) and np.array_equal(coin["index"], ring.slots(form, batch, update))
        keys = [k for k in plain if k != "mirrored"]
        heads, tails = np.flatnonzero(coins == 1), np.flatnonzero(coins == 0)
        assert heads.size and tails.size
        _assert_same(always, coin, heads, keys, what)
        _assert_same(plain, coin, tails, keys, what)
        _assert_mirrored(ring, plain, coin, heads, what)


# ------------------------------------------------------------------------------------------------ 8. the step path
def _device_mirror(A, B, action=None, in_place=False):
    """tpl_mirror_states on host arrays, through canary-framed device buffers."""
    n = A.shape[0]
    a, b, oa, ob = Framed(n * 16, 1), Framed(n * 16, 2), Framed(n * 16, 3), Framed(n * 16, 4)
    a.inner().copy_(torch.from_numpy(A.view(np.uint8).reshape(-1)))
    b.inner().copy_(torch.from_numpy(B.view(np.uint8).reshape(-1)))
    act = out_act = None
    if action is not None:
        act, out_act = Framed(n, 5), Framed(n, 6)
        act.inner().copy_(torch.from_numpy(action))
    if in_place:
        oa, ob, out_act = a, b, act
    _check(_lib().tpl_mirror_states(n, a.ptr(), b.ptr(), oa.ptr(), ob.ptr(), None if act is None else act.ptr(),
                                    None if act is None else out_act.ptr(), _stream()))
    for f in (a, b, oa, ob) + (() if act is None else (act, out_act)):
        f.assert_canary(("tpl_mirror_states", n, in_place))
    if not in_place:                                       # the inputs are left alone
        assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    return (oa.host().view(np.uint32).reshape(n, 4), ob.host().view(np.uint32).reshape(n, 4),
            None if act is None else out_act.host())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_standalone_entry_is_the_numpy_mirror(n):
    gen = np.random.default_rng(n)
    A, B = (np.ascontiguousarray(x[:n]) for x in R.pack_state(**R.random_fields(gen, n + 1)))     # (it makes two at least)
    B[:, 1] |= gen.integers(0, 2, n).astype(np.uint32) << np.uint32(31)          # the unused bit is carried over
    action = gen.integers(0, 256, n).astype(np.uint8)
    wa, wb = _m().mirror_states(A, B)
    want = _m().mirror_actions(action, A, B)
    for in_place in (False, True):
        ga, gb, gact = _device_mirror(A, B, action, in_place)
        assert np.array_equal(ga, wa) and np.array_equal(gb, wb) and np.array_equal(gact, want), (n, in_place)
    ga, gb, gact = _device_mirror(A, B)                    # without actions
    assert np.array_equal(ga, wa) and np.array_equal(gb, wb) and gact is None
    ba, bb, _ = _device_mirror(ga, gb)                     # an involution
    assert np.array_equal(ba, A) and np.array_equal(bb, B)


def _step_states(gen, n, L, M):
    """n running boards and an action each: ragged stacks, tall ones (top-outs), stacks of 1..4 full rows with a one-column
    well and the upright I over it (clears), with lines within four of L and moves within two of M for half of them."""
    rows = np.zeros((n, 20), np.uint16)
    window = gen.integers(0, 1 << 36, n, dtype=np.int64).astype(np.uint64)
    cur = gen.integers(0, 7, n)
    action = gen.integers(0, 40, n).astype(np.uint8)
    for i in range(n):
        kind = i % 3
        heights = gen.integers(0, 13, 10) if kind == 0 else gen.integers(14, 21, 10)
        if kind < 2:
            for x in range(10):
                for k in range(int(heights[x])):
                    if k == heights[x] - 1 or gen.random() > 0.2:
                        rows[i, 19 - k] |= np.uint16(1 << x)
        else:
            well, k = int(gen.integers(0, 10)), int(gen.integers(1, 5))
            rows[i, 20 - k:] = np.uint16(0x3FF & ~(1 << well))
            cur[i], action[i] = 0, 10 + well                # the upright I into the well
    window = (window & ~np.uint64(7)) | cur.astype(np.uint64)
    near = gen.random(n) < 0.5
    lines = np.where(near, L - 1 - gen.integers(0, 4, n), gen.integers(0, L, n))
    moves = np.where(near, M - 1 - gen.integers(0, 2, n), gen.integers(0, M, n))
    return R.pack_state(rows, lines, moves, 0, 0, window) + (action,)


@pytest.mark.parametrize("L,M", [(10, 40), (5, 20)])
def test_the_hip_step_path_commutes_with_the_mirror(L, M):
    n = 12288
    gen = np.random.default_rng(L)
    A, B, action = _step_states(gen, n, L, M)
    mA, mB, m_action = _device_mirror(A, B, action)
    envs = []
    for planes, act in (((A, B), action), ((mA, mB), m_action)):
        env = T.BatchedTetris(L, M, n, device=DEV, seed=3, auto_reset=False, reward=(1.0, 10.0, -3.0))
        env.load_configs(*env.synthetic_configs(256))
        env.reset()
        env.write_raw_planes(*[torch.from_numpy(p.view(np.int32)) for p in planes])
        _, reward, done, _ = env.step(torch.from_numpy(act).to(DEV), observe=False)
        a, b = env.raw_planes()
        envs.append(dict(reward=_np(reward), done=_np(done), a=_np(a).view(np.uint32), b=_np(b).view(np.uint32)))
        env.terminate()
    plain, mirrored = envs
    assert np.array_equal(plain["reward"].view(np.uint32), mirrored["reward"].view(np.uint32))
    assert np.array_equal(plain["done"], mirrored["done"])
    want = R.decode_state(*_m().mirror_states(plain["a"], plain["b"]))
    got = R.decode_state(mirrored["a"], mirrored["b"])
    for k in ("rows", "lines", "moves", "state"):           # the piece window after the move is pool data: not compared
        assert np.array_equal(got[k], want[k]), k
    before, after = R.decode_state(A, B), R.decode_state(plain["a"], plain["b"])
    cleared = after["lines"].astype(int) - before["lines"].astype(int)
    seen = {k: int((cleared == k).sum()) for k in range(1, 5)}
    ends = {s: int((after["state"] == s).sum()) for s in (0, 1, 2, 3)}
    print(f"L={L} M={M}: cleared {seen}, states after {ends}")
    assert min(seen.values()) >= 100 and min(ends.values()) >= 100
    assert (plain["a"] != mirrored["a"]).any()


# ------------------------------------------------------------------------------------------------ 9. the learner
@pytest.mark.parametrize("kind", ["uniform", "prioritized", "nstep"])
def test_the_learner_draws_with_the_coin(kind):
    L, M, n, B, cap, seed, gamma = 5, 20, 1024, 256, 1 << 14, 4, 0.99
    env = _env(L, M, n, seed=6)
    n_step = 3 if kind == "nstep" else 1
    learner = T.DQNLearner(env, model=_model(8), capacity=cap, batch_size=B, seed=seed, gamma=gamma,
                           prioritized=kind == "prioritized", n_step=n_step, mirror=True)
    assert learner.mirror is True and learner.n_step == n_step
    learner.collect(6)
    size, head = learner.ring.size, learner.ring.head
    records = _np(learner.ring.data).reshape(cap, 80)
    dec = R.decode_records(records)
    perm = _m().MIRROR_OBS_PERM
    for k in range(3):
        params = _params_np(learner.target)                 # the target network this update bootstraps from
        loss = learner.update(1)
        assert np.isfinite(loss)
        b = learner.last
        coins = _m().mirror_coins(seed, k, B)
        flip = coins == 1
        assert np.array_equal(_np(b["mirrored"]), coins) and flip.any() and (~flip).any()
        idx = _np(b["index"])
        if kind != "prioritized":
            assert np.array_equal(idx, _m().replay_indices(seed, k, B, size))
        src = idx
        if n_step > 1:
            ret, disc, done, steps, src = _m().nstep_targets(records, cap, size, head, n, idx, n_step, gamma)
            assert np.array_equal(_np(b["reward"]).view(np.uint32), ret.view(np.uint32))
            assert np.array_equal(_np(b["discount"]).view(np.uint32), disc.view(np.uint32))
            assert np.array_equal(_np(b["done"]), done) and np.array_equal(_np(b["steps"]), steps)
        else:
            assert np.array_equal(_np(b["reward"]).view(np.uint32), dec["reward_bits"][idx])
            assert np.array_equal(_np(b["done"]), dec["done"][idx])
        # s, a and s' are the mirrored transition's where the coin says so
        obs = R.obs_from_fields({key: v[idx] for key, v in dec["s"].items()}, L, M)
        obs = np.where(flip[:, None], obs[:, perm], obs).astype(np.float32)
        assert np.array_equal(_np(b["obs"]).view(np.uint32), obs.view(np.uint32)), k
        act = np.where(flip, _m().mirror_actions(dec["action"][idx], dec["sa"][idx], dec["sb"][idx]), dec["action"][idx])
        assert np.array_equal(_np(b["action"]), act), k
        ma, mb = _m().mirror_states(dec["na"][src], dec["nb"][src])
        wa, wb = np.where(flip[:, None], ma, dec["na"][src]), np.where(flip[:, None], mb, dec["nb"][src])
        na, nb = (_np(x).view(np.uint32) for x in learner.next_env.raw_planes())
        assert np.array_equal(na, wa) and np.array_equal(nb, wb), k
        # Q'(s') of the target image on the mirrored s', within the split kernel's documented bound
        ref = R.mlp64(R.obs_from_fields(R.decode_state(wa, wb), L, M), params)
        tol = 2e-5 * (1 + np.abs(ref).max())
        err = np.abs(_np(b["next_q"]).astype(np.float64) - ref).max()
        print(f"{kind} update {k}: {int(flip.sum())} of {B} mirrored, next_q error {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (k, err, tol)
        # and the mirrored s' is a different input: the plain s' does not give these values
        plain_q = R.mlp64(R.obs_from_fields(R.decode_state(dec["na"][src], dec["nb"][src]), L, M), params)
        assert np.abs(plain_q - ref)[flip].max() > 10 * tol
    # the ring's own surface: mirror="always" against mirror=False, which returns what it always did
    next_env = T.BatchedTetris(L, M, 64, device=DEV, seed=5)
    extra = dict(n_step=n_step, gamma=gamma) if n_step > 1 else {}
    if kind != "prioritized":
        extra["with_index"] = True
    plain = learner.ring.sample(64, 1, 0, next_env, **extra)
    plain_next = [_np(x).view(np.uint32) for x in next_env.raw_planes()]
    always = learner.ring.sample(64, 1, 0, next_env, mirror="always", **extra)
    always_next = [_np(x).view(np.uint32) for x in next_env.raw_planes()]
    assert "mirrored" not in plain and (_np(always["mirrored"]) == 1).all()
    assert set(always) == set(plain) | {"mirrored"}
    assert np.array_equal(_np(always["obs"]), _np(plain["obs"])[:, perm])
    for got, want in zip(always_next, _m().mirror_states(*plain_next)):
        assert np.array_equal(got, want)
    for key in set(plain) - {"obs", "action"}:
        assert torch.equal(always[key], plain[key]), key
    next_env.terminate()
    env.terminate()
