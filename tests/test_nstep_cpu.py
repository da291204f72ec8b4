"""CPU-side checks of n-step returns (include/tpl_learn.h's rule, _learn_lib.nstep_targets, tpl_replay_sample_nstep's argument
checks, the Python refusals): the slot-based mirror equals a restatement that walks each board's trajectory in time, the
entry point refuses every bad argument before any GPU work, and the Python surface refuses what the rule cannot serve."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tetris_piclim as T

GAMMAS = [0.0, 0.5, 0.99, 1.0]
N_STEPS = [1, 2, 3, 5, 16]
# (capacity, N, T, pushes): capacity a multiple of N and not wrapped / wrapped more than once; not a multiple of N wrapped once
# / more than once; capacity < n_step * N for every n_step > 2; a ring filled exactly (head back at 0)
SHAPES = [(64, 8, 2, 3), (64, 8, 3, 10), (100, 7, 2, 9), (50, 7, 3, 7), (20, 7, 2, 12), (13, 13, 1, 1)]


def _L():
    return T._learn_lib


def synthetic_pushes(gen, cap, n, steps, pushes):
    """[steps, n] pushes of random finite rewards and dones (p = 0.2) into a ring of `cap` 80-byte records.  Returns the
    record bytes, head, size and the per-transition rewards and dones in global order g = tau * n + i."""
    total = steps * n * pushes
    reward = (gen.standard_normal(total) * 10).astype(np.float32)
    done = (gen.random(total) < 0.2).astype(np.uint8)
    rec = np.zeros((cap, 80), np.uint8)
    head, pushed = 0, 0
    for _ in range(pushes):
        g = pushed + np.arange(steps * n)                     # transition (t, i) of this push is global pushed + t * n + i
        slot = (head + np.arange(steps * n)) % cap
        rec[slot, 64:68] = reward[g].view(np.uint8).reshape(-1, 4)
        rec[slot, 69] = done[g]
        rec[slot, 68] = (g % 40).astype(np.uint8)
        head = (head + steps * n) % cap
        pushed += steps * n
    return rec, head, min(pushed, cap), reward, done


def walk_in_time(reward, done, total, cap, n, slots, n_step, gamma):
    """The rule restated over time: slot j holds the newest global transition g = tau * n + i with g mod cap = j; follow board
    i through tau + 1, tau + 2, ... while that step was recorded (g + k * n < total), stopping after a done.  Slots appear
    only at the end, as the source of s'."""
    gam = np.float32(gamma)
    out = dict(ret=[], discount=[], done=[], steps=[], src=[])
    for j in slots:
        g = int(j) + cap * ((total - 1 - int(j)) // cap)
        ret, gk, last = np.float32(reward[g]), np.float32(1.0), g
        if not done[g]:
            for k in range(1, n_step):
                nxt = g + k * n
                if nxt >= total:
                    break
                gk = np.float32(gk * gam)
                ret = np.float32(ret + np.float32(gk * reward[nxt]))
                last = nxt
                if done[nxt]:
                    break
        out["ret"].append(ret)
        out["done"].append(done[last])
        out["discount"].append(np.float32(0.0) if done[last] else np.float32(gk * gam))
        out["steps"].append((last - g) // n + 1)
        out["src"].append(last % cap)
    return (np.array(out["ret"], np.float32), np.array(out["discount"], np.float32), np.array(out["done"], np.uint8),
            np.array(out["steps"], np.uint8), np.array(out["src"], np.int64))


@pytest.mark.parametrize("shape", SHAPES)
def test_mirror_is_the_time_walk_bit_for_bit(shape):
    cap, n, steps, pushes = shape
    gen = np.random.default_rng(cap * 100 + n)
    rec, head, size, reward, done = synthetic_pushes(gen, cap, n, steps, pushes)
    total = steps * n * pushes
    assert head == total % cap and size == min(total, cap)
    slots = np.concatenate([np.arange(size), _L().replay_indices(3, 1, 500, size)])
    for n_step in N_STEPS:
        for gamma in GAMMAS:
            got = _L().nstep_targets(rec, cap, size, head, n, slots, n_step, gamma)
            want = walk_in_time(reward, done, total, cap, n, slots, n_step, gamma)
            what = (shape, n_step, gamma)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what
            for a, b in zip(got[2:], want[2:]):
                assert a.dtype == b.dtype and np.array_equal(a, b), what
            if n_step == 3 and steps * pushes >= 3:           # all three endings occur: full length, a done, the head
                k, d = got[3], got[2]
                assert (k == 3).any() and ((k < 3) & (d != 0)).any() and ((k < 3) & (d == 0)).any(), what
            if n_step == 1:                                   # the 1-step sampler's outputs
                r = rec[slots, 64:68].copy().view(np.float32).reshape(-1)
                assert np.array_equal(got[0].view(np.uint32), r.view(np.uint32))
                assert np.array_equal(got[2], rec[slots, 69]) and np.array_equal(got[4], slots)
                assert np.array_equal(got[1], np.where(rec[slots, 69] != 0, np.float32(0), np.float32(gamma)).astype(np.float32))


def test_argument_errors_come_back_as_statuses_without_a_gpu():
    lib = _L().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                     # 128-byte aligned, never dereferenced: every call below is refused
    big = 1 << 32

    def sample(ring=fake, tree=None, cap=16, size=16, head=0, stride=4, n_step=3, gamma=0.99, batch=8, L=2, M=2, obs=fake,
               dtype=0, ret=fake, discount=fake, done=fake, steps=fake, index=None, prob=None):
        return lib.tpl_replay_sample_nstep(ring, tree, cap, size, head, stride, n_step, gamma, batch, 0, 0, L, M, obs, dtype,
                                           fake, fake, fake, ret, discount, done, steps, index, prob, None)

    # the two samplers' own checks
    assert sample(ring=None) < 0 and b"null" in err()
    assert sample(obs=None) < 0 and b"null" in err()
    for name in ("ret", "discount", "done", "steps"):
        assert sample(**{name: None}) < 0 and b"null" in err(), name
    assert sample(tree=fake, index=None, prob=fake) < 0 and b"null" in err()
    assert sample(tree=fake, index=fake, prob=None) < 0 and b"null" in err()
    assert sample(prob=fake) < 0 and b"prob" in err()                      # prob without a tree
    assert sample(cap=0, size=0) < 0 and b"capacity" in err()
    assert sample(cap=big, size=16) < 0 and b"capacity" in err()
    assert sample(size=0) < 0 and b"size" in err()
    assert sample(size=17) < 0 and b"size" in err()
    assert sample(batch=0) < 0 and b"batch" in err()
    assert sample(batch=1 << 30) < 0 and b"batch" in err()
    assert sample(L=0) < 0 and b"L and M" in err()
    assert sample(M=256) < 0 and b"L and M" in err()
    assert sample(dtype=7) < 0 and b"dtype" in err()
    assert sample(obs=fake + 4) < 0 and b"aligned" in err()
    assert sample(ring=fake + 8) < 0 and b"aligned" in err()
    assert sample(tree=fake + 16, index=fake, prob=fake) < 0 and b"aligned" in err()
    # the n-step rule's own
    for n_step in (0, -1, 17, 1 << 20):
        assert sample(n_step=n_step) < 0 and b"n_step" in err(), n_step
    for gamma in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert sample(gamma=gamma) < 0 and b"gamma" in err(), gamma
    for stride in (0, -4, 17):
        assert sample(stride=stride) < 0 and b"stride" in err(), stride
    for head in (-1, 16, 1 << 40):
        assert sample(head=head) < 0 and b"head" in err(), head
    assert sample(size=10, head=0) < 0 and b"head must equal size" in err()
    assert sample(size=10, head=11) < 0 and b"head must equal size" in err()
    assert sample(tree=fake, index=fake, prob=fake, size=10, head=9) < 0 and b"head must equal size" in err()
    # the mirror refuses what the library refuses
    rec = np.zeros((16, 80), np.uint8)
    for kw in (dict(n_step=0), dict(n_step=17), dict(gamma=1.5), dict(stride=0), dict(head=16), dict(size=10, head=3)):
        args = dict(capacity=16, size=16, head=0, stride=4, slots=[0], n_step=3, gamma=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            _L().nstep_targets(rec, **args)


def test_python_refusals_need_no_gpu():
    ring = T.ReplayRing(64, "cpu")
    with pytest.raises(ValueError, match="gamma"):
        ring.sample(8, 0, 0, None, n_step=3)
    for n_step in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="n_step"):
            ring.sample(8, 0, 0, None, n_step=n_step, gamma=0.9)
    with pytest.raises(ValueError, match="gamma"):
        ring.sample(8, 0, 0, None, n_step=3, gamma=1.5)

    class Env:                                         # stands in for a BatchedTetris: only its identity matters here
        pass

    a, b = Env(), Env()
    for second in ((b, 8), (a, 4)):                    # a second environment, or a second N
        ring = T.ReplayRing(64, "cpu")
        ring._track_push(a, 8)
        ring._track_push(a, 8)
        assert ring.stride == 8 and ring._one_source
        ring._track_push(*second)
        assert ring.stride == 8 and not ring._one_source
        with pytest.raises(ValueError, match="one environment"):
            ring.sample(8, 0, 0, None, n_step=2, gamma=0.9)
    for n_step in (0, 17, -3, 1.5):
        with pytest.raises(ValueError, match="n_step"):
            T.DQNLearner(None, n_step=n_step)
    with pytest.raises(ValueError, match="gamma"):
        T.DQNLearner(None, gamma=1.5, n_step=3)
    with pytest.raises(AttributeError):                # n_step = 1 leaves gamma alone: the environment check comes next
        T.DQNLearner(None, gamma=1.5, n_step=1)


def test_nstep_kernels_use_no_scratch():
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _L().build_library()],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    names = [r[-1] for r in rows]
    for kernel in ("replay_sample_kernel", "replay_sample_prioritized_kernel"):
        for dtype in ("f", "14__hip_bfloat16"):
            for kn in (0, 1, 4, 8, 16):
                want = f"{kernel}I{dtype}Li{kn}E"
                assert any(want in n for n in names), (want, names)
    for r in rows:
        assert r[r.index("scratch") - 1] == "0", r
    assert "tpl_replay_sample_nstep" in _L().LEARN_SYMBOLS
