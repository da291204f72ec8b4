"""The learner's device code (csrc/learn/replay.hip, priority.hip, tpl_replay_draw.h) over its whole argument range, against
host references that do not go through the device (tests/learn_ref.py and _learn_lib's numpy tree mirror):

  * STATE: learn_ref.decode_state of the resident planes is tpl_get_state's export, on boards in every state and on planes
    written with every field at its limits.
  * PUSH: after every push the whole ring, every slot and all 80 bytes, is a numpy model built from the recorded
    trajectory (capacities 1 .. 65537, chunks of 1 .. 2049 boards x 1 .. 5 steps, heads 0 and capacity - 1), and a canary
    on each side of the ring is intact.
  * UNIFORM SAMPLE: records at the ends of every field, batches whose last wave holds 1 .. 64 draws, float32 and bf16,
    (L, M) from (1, 1) to (250, 254): every output equals the drawn record decoded on the host, and every canary byte
    around every output is intact.
  * SUM TREE: heights 1, 2, 3, 4, 5, 6, 7, 8 and 9 (2^28 + 1 slots): pushes with and without wrap, write-backs with
    ignored indices, duplicates and edge values, and draws, all bit for bit against the mirror; the descent's rounding
    fallback on the device.
  * LEARNER: minibatch obs and the TD target y at (L, M) = (1, 1) and (250, 254) against a float64 host reference.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from test_learn_range_cpu import FALLBACK, fallback_tree
from test_learner_gpu import _env, _model, _np, _params_np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 4096                                   # canary bytes on each side of a buffer (keeps 128-byte alignment)
F32, BF16 = 0, 1                             # tpl_obs_dtype codes (TPL_F32 / TPL_BF16)


def _lib():
    return T._learn_lib.lib()


def _check(status):
    T._learn_lib.check(status)


def _stream():
    return torch._C._cuda_getCurrentRawStream(0)


class Framed:
    """`nbytes` device bytes framed by PAD random canary bytes on each side."""

    def __init__(self, nbytes, seed=0, zero=True):
        self.nbytes = int(nbytes)
        gen = np.random.default_rng(seed)
        self.canary = torch.from_numpy(gen.integers(0, 256, 2 * PAD, dtype=np.uint8)).to(DEV)
        self.buf = torch.empty(self.nbytes + 2 * PAD, dtype=torch.uint8, device=DEV)
        self.buf[:PAD] = self.canary[:PAD]
        self.buf[PAD + self.nbytes:] = self.canary[PAD:]
        if zero:
            self.inner().zero_()

    def inner(self):
        return self.buf[PAD:PAD + self.nbytes]

    def ptr(self):
        return self.buf.data_ptr() + PAD

    def host(self):
        return _np(self.inner())

    def assert_canary(self, what=""):
        torch.cuda.synchronize()
        assert torch.equal(self.buf[:PAD], self.canary[:PAD]), ("canary before", what)
        assert torch.equal(self.buf[PAD + self.nbytes:], self.canary[PAD:]), ("canary after", what)


def _plane_ptrs(env):
    pa, pb = C.c_void_p(), C.c_void_p()
    T._lib.check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
    return pa.value, pb.value


# ------------------------------------------------------------------------------------------------ 1. the state decoder
def _assert_export(env, what):
    a, b = env.raw_planes()
    d = R.decode_state(_np(a), _np(b))
    got = {k: _np(v) for k, v in env.packed_state().items()}
    assert np.array_equal(got["rows"].view(np.uint16), d["rows"]), what
    for k in ("cur", "nxt", "lines", "moves"):
        assert np.array_equal(got[k], d[k]), (what, k)
    assert np.array_equal(got["state"], np.where(d["state"] == 3, 2, d["state"])), what
    return d


@pytest.mark.parametrize("L,M", [(1, 1), (1, 3), (5, 20), (250, 254)])
def test_decode_state_is_the_device_export_in_every_state(L, M):
    n = 2048
    env = T.BatchedTetris(L, M, n, device=DEV, seed=3, auto_reset=False)
    rows, pieces = env.synthetic_configs(256)
    env.load_configs(rows, pieces)
    env.reset()
    seen = set()
    for t in range(min(M + 2, 30)):
        env.step(env.synthetic_actions(t), observe=False)
        seen |= set(_assert_export(env, t)["state"].tolist())
    assert (1 in seen) if L == 1 else (3 in seen), seen                  # won boards at L = 1, top-outs elsewhere
    assert 2 in seen or M > 30, seen
    # planes written with every field at its limits (moves <= M, as the environment keeps them)
    f = R.random_fields(np.random.default_rng(L + M), n, M=M)
    A, B = R.pack_state(**f)
    env.write_raw_planes(torch.from_numpy(A.view(np.int32)), torch.from_numpy(B.view(np.int32)))
    d = _assert_export(env, "written")
    assert set(d["state"].tolist()) == {0, 1, 2, 3}
    # and the observation of those planes is the host's
    obs = env.expand_states(torch.from_numpy(A.view(np.int32)).to(DEV), torch.from_numpy(B.view(np.int32)).to(DEV))
    assert np.array_equal(_np(obs).view(np.uint32), R.obs_from_fields(d, L, M).astype(np.float32).view(np.uint32))
    env.terminate()


# ------------------------------------------------------------------------------------------------ 2. replay push
PUSH_CAPS = [1, 64, 4500, 65537]
PUSH_N = [1, 63, 64, 65, 257, 2049]
PUSH_T = [1, 2, 5]


def _records(traj, after, steps, n):
    """The [steps * n, 80] records of one chunk, from the recorded trajectory (s' = the next recorded state, or the
    resident planes after the chunk for the last step)."""
    sa = _np(traj["states_a"]).view(np.uint32).reshape(steps, n, 4)
    sb = _np(traj["states_b"]).view(np.uint32).reshape(steps, n, 4)
    na = np.concatenate([sa[1:], _np(after[0]).view(np.uint32)[None]], axis=0)
    nb = np.concatenate([sb[1:], _np(after[1]).view(np.uint32)[None]], axis=0)
    rec = np.zeros((steps * n, 80), np.uint8)
    for off, w in ((0, sa), (16, sb), (32, na), (48, nb)):
        rec[:, off:off + 16] = w.reshape(-1, 4).view(np.uint8).reshape(-1, 16)
    rec[:, 64:68] = _np(traj["rewards"]).reshape(-1).view(np.uint8).reshape(-1, 4)
    rec[:, 68] = _np(traj["actions"]).reshape(-1)
    rec[:, 69] = _np(traj["dones"]).reshape(-1).astype(np.uint8)
    return rec


@pytest.mark.parametrize("cap", PUSH_CAPS)
def test_push_writes_exactly_its_slots_and_nothing_else(cap):
    L, M = 2, 3                                                   # short games: most chunks hold done transitions
    image = T.actor.policy_image(_model(0), DEV, f32="split")
    ring = Framed(cap * 80, seed=cap)
    model = np.zeros((cap, 80), np.uint8)
    envs = {}
    step0, dones, pushes = 0, 0, 0
    plan = [(n, steps, head) for n in PUSH_N for steps in PUSH_T if steps * n <= cap for head in sorted({0, cap - 1})]
    if cap >= 64:
        plan.append((64, 1, 17))                                  # a head inside the ring; at capacity 64 a push of all of it
    for n, steps, head in plan:
        if n not in envs:
            envs[n] = _env(L, M, n, seed=n)
        env = envs[n]
        traj = env.actor_rollout(image, steps, epsilon=0.5, seed=5, step0=step0, record=True, record_states=True)
        step0 += steps
        after = env.raw_planes()
        pa, pb = _plane_ptrs(env)
        _check(_lib().tpl_replay_push(ring.ptr(), cap, head, steps, n, traj["actions"].data_ptr(), traj["rewards"].data_ptr(),
                                      traj["dones"].data_ptr(), traj["states_a"].data_ptr(), traj["states_b"].data_ptr(), pa, pb,
                                      _stream()))
        rec = _records(traj, after, steps, n)
        model[(head + np.arange(steps * n)) % cap] = rec
        got = ring.host().reshape(cap, 80)
        bad = np.flatnonzero((got != model).any(axis=1))
        assert bad.size == 0, (n, steps, head, bad[:8])
        ring.assert_canary((n, steps, head))
        # a done transition's s' is the freshly reset board
        d = rec[:, 69] != 0
        if d.any():
            nxt = R.decode_records(rec[d])
            s2 = R.decode_state(nxt["na"], nxt["nb"])
            assert (s2["moves"] == 0).all() and (s2["lines"] == 0).all() and (s2["state"] == 0).all()
        dones += int(d.sum())
        pushes += 1
    assert pushes == len(plan) and (dones > 0 or cap == 1)
    assert not R.decode_records(model)["tail"].any()
    for env in envs.values():
        env.terminate()


# ------------------------------------------------------------------------------------------------ 3. uniform sample
SAMPLE_BATCHES = [1, 7, 63, 64, 65, 255, 257, 4099]
GAMES = [(1, 1), (5, 20), (10, 40), (250, 254)]


def _synthetic_ring(gen, cap, M):
    """`cap` records with s at the ends of every field (moves <= M), random s' words, reward bits, actions and dones."""
    f = R.random_fields(gen, cap, M=M)
    A, B = R.pack_state(**f)
    rec = np.zeros((cap, 80), np.uint8)
    rec[:, 0:16], rec[:, 16:32] = A.view(np.uint8).reshape(cap, 16), B.view(np.uint8).reshape(cap, 16)
    rec[:, 32:64] = gen.integers(0, 256, (cap, 32), dtype=np.uint8)
    r = gen.standard_normal(cap).astype(np.float32) * np.float32(100)
    r[:4] = [0.0, -0.0, np.float32(1e-40), np.float32(3e38)]
    rec[:, 64:68] = r.view(np.uint8).reshape(cap, 4)
    rec[:, 68] = gen.integers(0, 256, cap)
    rec[:, 69] = gen.integers(0, 2, cap)
    return rec


@pytest.mark.parametrize("L,M", GAMES)
def test_uniform_sample_is_the_decoded_record_with_intact_canaries(L, M):
    cap, seed = 4500, 13
    gen = np.random.default_rng(L * 1000 + M)
    rec = _synthetic_ring(gen, cap, M)
    dec = R.decode_records(rec)
    ring = torch.from_numpy(rec.reshape(-1)).to(DEV)
    obs_all = R.obs_from_fields(dec["s"], L, M)
    calls = 0
    for size in (cap, 1234):
        for batch in SAMPLE_BATCHES:
            for dtype, esize in ((F32, 4), (BF16, 2)):
                update = calls
                calls += 1
                out = dict(obs=Framed(batch * 217 * esize, 1), next_a=Framed(batch * 16, 2), next_b=Framed(batch * 16, 3),
                           action=Framed(batch, 4), reward=Framed(batch * 4, 5), done=Framed(batch, 6), index=Framed(batch * 8, 7))
                _check(_lib().tpl_replay_sample(
                    ring.data_ptr(), cap, size, batch, seed, update, L, M, out["obs"].ptr(), dtype, out["next_a"].ptr(),
                    out["next_b"].ptr(), out["action"].ptr(), out["reward"].ptr(), out["done"].ptr(), out["index"].ptr(),
                    _stream()))
                what = (size, batch, dtype)
                for o in out.values():
                    o.assert_canary(what)
                idx = T._learn_lib.replay_indices(seed, update, batch, size)
                assert np.array_equal(out["index"].host().view(np.int64), idx), what
                want = obs_all[idx]
                if dtype == F32:
                    assert np.array_equal(out["obs"].host().view(np.uint32), want.astype(np.float32).view(np.uint32).reshape(-1)), what
                else:
                    wb = torch.from_numpy(want).to(torch.bfloat16).view(torch.int16).numpy().reshape(-1)
                    assert np.array_equal(out["obs"].host().view(np.int16), wb), what
                assert np.array_equal(out["next_a"].host().view(np.uint32).reshape(-1, 4), dec["na"][idx]), what
                assert np.array_equal(out["next_b"].host().view(np.uint32).reshape(-1, 4), dec["nb"][idx]), what
                assert np.array_equal(out["action"].host(), dec["action"][idx]), what
                assert np.array_equal(out["reward"].host().view(np.uint32), dec["reward_bits"][idx]), what
                assert np.array_equal(out["done"].host(), dec["done"][idx]), what
    # the features at their ends were drawn: negative lines left, and moves left 0 and M
    assert obs_all[:, 214].min() == L - 255 and obs_all[:, 215].min() == 0 and obs_all[:, 215].max() == M


# ------------------------------------------------------------------------------------------------ 4. the sum tree
TREE_CAPS = [1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65537, (1 << 24) + 1]
DRAW_BATCHES = [1, 65, 257, 4099]


class DeviceTree:
    """A device tree framed by canaries, next to its numpy mirror; every operation is checked against the mirror."""

    def __init__(self, cap):
        self.cap = cap
        self.m = T._learn_lib
        self.nbytes = _lib().tpl_priority_tree_bytes(cap)
        assert self.nbytes == 8 * self.m.priority_layout(cap)[2]
        self.dev = Framed(self.nbytes, seed=cap % 1000, zero=False)
        self.mirror = self.m.priority_tree_init(cap)
        _check(_lib().tpl_priority_init(self.dev.ptr(), cap, _stream()))
        self.check("init")

    def check(self, what):
        got = self.dev.host().view(np.int64)
        bad = np.flatnonzero(got != self.mirror.view(np.int64))
        assert bad.size == 0, (self.cap, what, bad[:8], got[bad[:8]].view(np.float64), self.mirror[bad[:8]])
        self.dev.assert_canary((self.cap, what))

    def push(self, head, count):
        _check(_lib().tpl_priority_push(self.dev.ptr(), self.cap, head, count, _stream()))
        self.m.priority_tree_push(self.mirror, head, count)
        self.check(("push", head, count))

    def update(self, index, priority, what):
        index, priority = np.asarray(index, np.int64), np.asarray(priority, np.float64)
        i_d, p_d = torch.from_numpy(index).to(DEV), torch.from_numpy(priority).to(DEV)
        _check(_lib().tpl_priority_update(self.dev.ptr(), self.cap, index.size, i_d.data_ptr(), p_d.data_ptr(), _stream()))
        self.m.priority_tree_update(self.mirror, index, priority)
        self.check(what)

    def draws(self, ring, batch, seed, update):
        out = dict(obs=torch.empty((batch, 217), dtype=torch.bfloat16, device=DEV),
                   na=torch.empty((batch, 4), dtype=torch.int32, device=DEV), nb=torch.empty((batch, 4), dtype=torch.int32, device=DEV),
                   action=torch.empty(batch, dtype=torch.uint8, device=DEV), reward=torch.empty(batch, dtype=torch.float32, device=DEV),
                   done=torch.empty(batch, dtype=torch.uint8, device=DEV))
        index, prob = Framed(batch * 8, 8), Framed(batch * 4, 9)
        _check(_lib().tpl_replay_sample_prioritized(
            ring.data_ptr(), self.dev.ptr(), self.cap, self.cap, batch, seed, update, 2, 3, out["obs"].data_ptr(), BF16,
            out["na"].data_ptr(), out["nb"].data_ptr(), out["action"].data_ptr(), out["reward"].data_ptr(), out["done"].data_ptr(),
            index.ptr(), prob.ptr(), _stream()))
        index.assert_canary("index")
        prob.assert_canary("prob")
        idx, p = self.m.prioritized_draws(self.mirror, seed, update, batch)
        got_i, got_p = index.host().view(np.int64), prob.host().view(np.uint32)
        assert np.array_equal(got_i, idx), (self.cap, batch, np.flatnonzero(got_i != idx)[:8])
        assert np.array_equal(got_p, p.view(np.uint32)), (self.cap, batch)
        leaves = self.mirror[16:16 + self.cap]
        assert (leaves[idx] > 0).all()
        return idx

    def levels_of(self, head, count):
        """Per level k >= 1 of a wrapping push: 'disjoint' when its two parent ranges stay apart, else 'merged'."""
        offsets, _, _ = self.m.priority_layout(self.cap)
        end1 = head + count - self.cap
        kinds = []
        for k in range(1, len(offsets)):
            lo0, hi1 = head >> (4 * k), ((end1 - 1) >> (4 * k)) + 1
            kinds.append("merged" if hi1 >= lo0 else "disjoint")
        return kinds


@pytest.mark.parametrize("cap", TREE_CAPS)
def test_sum_tree_is_the_mirror_at_every_height(cap):
    t = DeviceTree(cap)
    gen = np.random.default_rng(cap % 977)
    size = max(1, cap // 3)
    t.push(0, size)                                                             # no wrap
    t.update([size // 2], [3.5], "batch 1")
    # ignored indices with a priority above every other: neither a leaf nor the running maximum moves
    before = t.mirror[0]
    t.update([-1, -(1 << 62), cap, 1 << 62, 0], [1e25, 1e25, 1e25, 1e25, 2.0], "ignored indices")
    assert t.mirror[0] == max(before, 2.0) < 1e25
    t.update([-1, cap, -(1 << 62), 1 << 62], [7e20] * 4, "only ignored indices")
    assert t.mirror[0] == max(before, 2.0)
    # one slot named B times
    t.update(np.full(300, size - 1), gen.random(300) * 4.0, "one slot 300 times")
    if cap > size:
        t.update(gen.integers(size, cap, 97), gen.random(97) + 0.5, "slots past size")
    # wraps: one small, one large; at three or more levels their parent ranges stay apart low down and merge higher up
    if cap >= 2:
        for head, count in ((cap - min(7, cap - 1), min(10, cap)), (cap - cap // 4 - 1, cap // 4 + cap // 2 + 2)):
            if head + count <= cap or count > cap or head < 0:
                continue
            kinds = t.levels_of(head, count)
            assert kinds[-1] == "merged"
            if cap >= 255:
                assert "disjoint" in kinds, (cap, head, count, kinds)
            t.push(head, count)
        t.push(cap // 2 if cap > 2 else 1, cap)                                # count = capacity at head != 0
    t.push(cap - 1, 1)                                                          # count = 1 at the last slot
    # edge values at random filled slots
    index = gen.integers(0, cap, 16)
    pr = gen.random(16) * 10.0 ** gen.integers(-14, 4, 16)
    pr[:8] = [np.nan, np.inf, -np.inf, 0.0, -2.5, -0.0, 1e300, 1e-300]
    t.update(index, pr, "edge values")
    ring = torch.zeros(cap * 80, dtype=torch.uint8, device=DEV)
    for k, batch in enumerate(DRAW_BATCHES):
        t.draws(ring, batch, 21, k)


def test_device_descent_takes_the_rounding_fallback():
    cap = FALLBACK["capacity"]
    t = DeviceTree(cap)
    t.update(np.array(FALLBACK["slots"]), np.array(FALLBACK["leaves"]), "fallback leaves")
    assert np.array_equal(t.mirror, fallback_tree(T._learn_lib))
    ring = torch.zeros(cap * 80, dtype=torch.uint8, device=DEV)
    idx = t.draws(ring, FALLBACK["batch"], FALLBACK["seed"], FALLBACK["update"])
    assert idx[-1] == 4496 and set(np.unique(idx)) == set(FALLBACK["slots"])
    # sums that round (1e-12 + 3 + 1e30 + 0.1): no zero leaf is ever drawn
    t = DeviceTree(cap)
    t.update(np.array([0, 17, 4095, 4496]), np.array([1e-12, 3.0, 1e30, 0.1]), "rounding leaves")
    for update in range(4):
        idx = t.draws(ring, 65536, 5, update)
        assert set(np.unique(idx)) <= {0, 17, 4095, 4496}


def test_height_nine_tree_descends_through_every_level():
    cap = (1 << 28) + 1
    free, _ = torch.cuda.mem_get_info(0)
    if free < (32 << 30):
        pytest.skip(f"the 2^28 + 1 tree and its ring need about 24 GB of device memory; {free >> 30} GB free")
    t = DeviceTree(cap)
    assert len(T._learn_lib.priority_layout(cap)[0]) == 9
    t.push(cap - 5, 10)                                                         # slots 2^28 - 4 .. 2^28 and 0 .. 4
    assert t.levels_of(cap - 5, 10) == ["disjoint"] * 6 + ["merged"] * 2
    t.update([1 << 28, 3, 77, (1 << 27) + 5], [3.0, 0.25, 2.0, 1.5], "height 9 write-back")
    offsets, _, _ = T._learn_lib.priority_layout(cap)
    root_line = t.mirror[offsets[7]:offsets[7] + 2]
    assert (root_line > 0).all()                                                # mass under both children of the root
    ring = torch.zeros(cap * 80, dtype=torch.uint8, device=DEV)
    seen = np.zeros(0, np.int64)
    for k, batch in enumerate(DRAW_BATCHES):
        seen = np.union1d(seen, t.draws(ring, batch, 33, k))
    assert (1 << 28) in seen and (seen < (1 << 28)).any()
    del ring


# ------------------------------------------------------------------------------------------------ 5. the learner's target
@pytest.mark.parametrize("L,M", [(1, 1), (250, 254)])
def test_learner_obs_and_target_at_the_ends_of_the_game_range(L, M):
    env = _env(L, M, 2048, seed=7, reward=(1.0, 2.5, -1.5))
    learner = T.DQNLearner(env, model=_model(5), capacity=1 << 14, batch_size=1000, seed=3)
    with torch.no_grad():
        for p in learner.target.parameters():
            p.add_(0.05 * torch.randn_like(p))
    T._learn_lib.pack_policy_device(T._learn_lib.policy_tensors(learner.target), "split", out=learner.target_image)
    learner.collect(4)
    moves_left_max = 0
    for k in range(3):
        params = _params_np(learner.target)
        mb = learner.minibatch()
        idx = _np(mb["index"])
        rec = R.decode_records(_np(learner.ring.data))
        s = {key: v[idx] for key, v in rec["s"].items()}
        obs = R.obs_from_fields(s, L, M)
        assert np.array_equal(_np(mb["obs"]).view(np.uint32), obs.astype(np.float32).view(np.uint32)), k
        nxt = R.decode_state(rec["na"][idx], rec["nb"][idx])
        q64 = R.mlp64(R.obs_from_fields(nxt, L, M), params)
        r64 = rec["reward_bits"][idx].view(np.float32).astype(np.float64)
        done = rec["done"][idx].astype(np.float64)
        assert np.array_equal(_np(mb["reward"]).view(np.uint32), rec["reward_bits"][idx])
        assert np.array_equal(_np(mb["done"]), rec["done"][idx])
        y64 = r64 + learner.gamma * (1.0 - done) * (q64[:, :4].max(1) + q64[:, 4:].max(1))
        ulp = np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64)
        tol = learner.gamma * 2 * 2e-5 * (1 + np.abs(q64).max()) + 4 * ulp
        err = np.abs(_np(mb["y"]).astype(np.float64) - y64)
        assert (err <= tol).all(), (k, float(err.max()), float(tol.min()))
        if M == 1:
            assert (done == 1).all()
        moves_left_max = max(moves_left_max, int(obs[:, 215].max()))
        learner.update(1)
    assert moves_left_max >= (128 if M == 254 else 1)
    env.terminate()
