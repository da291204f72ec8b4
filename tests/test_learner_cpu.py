"""CPU-side checks of the learner library (include/tpl_learn.h, csrc/learn/): it builds in-tree for gfx950 only, exports what
its header declares, uses no scratch; the host mirror of the sampling hash is the device's hash and is uniform; argument
errors come back as statuses before any GPU work; the factored Q's arg-max is the environment's action decode."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import tetris_piclim as T


def _learn():
    return T._learn_lib


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text)))


def test_learner_library_builds_in_tree_and_exports_every_declared_symbol():
    path = _learn().build_library()
    assert path == os.path.join(ROOT, "lib", "libtpl_learn.so") and os.path.exists(path)
    lib = ctypes.CDLL(path)
    declared = _declared_symbols()
    assert declared
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/tpl_learn.h but not exported"
    assert sorted(_learn().LEARN_SYMBOLS) == declared
    # the environment library's binding is untouched: none of the learner's entry points is in it
    assert not set(declared) & set(T.SYMBOLS)


def test_learner_digest_covers_the_environment_headers_it_includes():
    rel = {os.path.relpath(p, ROOT).split(os.sep, 1)[-1] for p in _learn()._sources()}
    for want in ("csrc/learn/replay.hip", "csrc/learn/pack.hip", "csrc/learn/tpl_learn_internal.h", "csrc/tpl_observe.h",
                 "csrc/tpl_device.h", "tpl_learn.h", "tetris_piclim.h"):
        assert any(r.endswith(want) for r in rel), want


def test_learner_code_object_targets_gfx950_only():
    blob = open(_learn().build_library(), "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx942", b"gfx90a", b"sm_"):
        assert other not in blob


def test_every_learner_kernel_uses_no_scratch():
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _learn().build_library()],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    names = [r[-1] for r in rows]
    for want in ("replay_push_kernel", "replay_sample_kernelIf", "replay_sample_kernelI14__hip_bfloat16", "pack_bf16_kernel",
                 "pack_f32_kernel", "pack_split_kernel"):
        assert any(want in n for n in names), (want, names)
    for r in rows:
        assert r[r.index("scratch") - 1] == "0", r


def test_host_mirror_of_the_sampling_hash_is_the_library_hash_and_stays_in_range():
    L, lib = _learn(), _learn().lib()
    for seed, update, size in ((0, 0, 1), (1, 0, 7), (12345, 3, 1000), ((1 << 64) - 1, (1 << 40) + 5, (1 << 32) - 1),
                               (7, 99, 1 << 24)):
        got = L.replay_indices(seed, update, 300, size)
        assert got.dtype == np.int64 and got.min() >= 0 and got.max() < size
        want = [lib.tpl_replay_index(seed, update, i, size) for i in range(300)]
        assert got.tolist() == want
    # the update number and the seed both change the draws
    assert not np.array_equal(L.replay_indices(0, 0, 64, 1 << 20), L.replay_indices(0, 1, 64, 1 << 20))
    assert not np.array_equal(L.replay_indices(0, 0, 64, 1 << 20), L.replay_indices(1, 0, 64, 1 << 20))
    assert lib.tpl_replay_index(0, 0, 0, 0) == -1 and lib.tpl_replay_index(0, 0, 0, 1 << 32) == -1
    with pytest.raises(ValueError):
        L.replay_indices(0, 0, 4, 0)


def test_sampling_hash_is_roughly_uniform():
    size, draws = 1000, 2_000_000
    idx = _learn().replay_indices(42, 7, draws, size)
    counts = np.bincount(idx, minlength=size)
    expected = draws / size
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    # 999 degrees of freedom: mean 999, sd ~45; 1200 is 4.5 sd out
    assert chi2 < 1200, chi2
    # and over a non-power-of-two ring near the 2^24 of the issue's ring: both halves equally often
    big = _learn().replay_indices(3, 0, 1_000_000, (1 << 24) - 3)
    assert abs(float((big < (1 << 23)).mean()) - 0.5) < 0.003


def test_argument_errors_come_back_as_statuses_without_a_gpu():
    lib = _learn().lib()
    err = lambda: lib.tpl_learn_last_error()
    assert lib.tpl_replay_record_bytes() == 80
    fake = 1 << 20                       # never dereferenced: every call below is refused before any HIP call
    ptrs = [fake] * 8
    # push: null pointers, capacity 0, a chunk larger than the ring, a head outside it
    assert lib.tpl_replay_push(None, 16, 0, 1, 4, *ptrs[:7], None) < 0 and b"null" in err()
    assert lib.tpl_replay_push(fake, 16, 0, 1, 4, None, *ptrs[:6], None) < 0 and b"null" in err()
    assert lib.tpl_replay_push(fake, 0, 0, 1, 4, *ptrs[:7], None) < 0 and b"capacity" in err()
    assert lib.tpl_replay_push(fake, 16, 0, 5, 4, *ptrs[:7], None) < 0 and b"exceeds" in err()
    assert lib.tpl_replay_push(fake, 16, 16, 1, 4, *ptrs[:7], None) < 0 and b"head" in err()
    assert lib.tpl_replay_push(fake, 16, 0, 0, 4, *ptrs[:7], None) < 0 and b"positive" in err()
    # sample: null pointers, capacity 0, an empty ring, batch 0, a bad dtype

    def sample(ring=fake, cap=16, size=16, batch=8, dtype=0, obs=fake, L=2, M=2):
        return lib.tpl_replay_sample(ring, cap, size, batch, 0, 0, L, M, obs, dtype, fake, fake, fake, fake, fake, None, None)

    assert sample(ring=None) < 0 and b"null" in err()
    assert sample(obs=None) < 0 and b"null" in err()
    assert sample(cap=0) < 0 and b"capacity" in err()
    assert sample(size=0) < 0 and b"size" in err()
    assert sample(size=17) < 0 and b"size" in err()
    assert sample(batch=0) < 0 and b"batch" in err()
    assert sample(dtype=7) < 0 and b"dtype" in err()
    assert sample(obs=fake + 4) < 0 and b"aligned" in err()
    assert sample(L=0) < 0 and b"L and M" in err()
    # pack: null pointers, unknown kind
    assert lib.tpl_learn_pack(2, *([None] * 11), None) < 0 and b"null" in err()
    assert lib.tpl_learn_pack(3, *([fake] * 11), None) < 0 and b"kind" in err()
    # the three image sizes are the environment library's
    env = T._lib.lib()
    assert lib.tpl_learn_image_bytes(0) == env.tpl_policy_image_bytes()
    assert lib.tpl_learn_image_bytes(1) == env.tpl_policy_image_bytes_f32()
    assert lib.tpl_learn_image_bytes(2) == env.tpl_policy_image_bytes_split()
    assert lib.tpl_learn_image_bytes(3) == 0


def test_factored_q_argmax_is_the_environment_decode():
    import torch
    factored_q, factored_max = T.learn.factored_q, T.learn.factored_max
    g = torch.Generator().manual_seed(0)
    out = torch.randn(4096, 14, generator=g)
    out[:7, :] = 0.0                                                 # ties: lowest index, as the decode
    q = torch.stack([factored_q(out, torch.full((4096,), a, dtype=torch.uint8)) for a in range(40)], dim=1)
    decode = out[:, :4].argmax(1) * 10 + out[:, 4:14].argmax(1)     # tpl_decode_actions (lowest index on ties)
    assert torch.equal(q.argmax(1), decode)
    assert torch.allclose(q.max(1).values, factored_max(out))


def test_importing_the_package_neither_builds_nor_loads_the_learner():
    code = ("import sys; sys.path.insert(0, %r); import tetris_piclim as T; T._lib.lib(); T.PolicyMLP; T.BatchedTetris; "
            "T.Actor; T.pool; T.sharding; "
            "print(int(any(m.endswith(('.learn', '._learn_lib')) for m in sys.modules)), int('libtpl_learn' in open('/proc/self/maps').read()))") % ROOT
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    assert res.stdout.split() == ["0", "0"]


def test_the_learner_never_reads_the_checker():
    for rel in ("learn.py", "_learn_lib.py", "csrc/learn/replay.hip", "csrc/learn/pack.hip", "csrc/learn/tpl_learn_internal.h"):
        text = open(os.path.join(os.path.dirname(T.__file__), rel)).read().lower()
        assert "oracle" not in text, rel
