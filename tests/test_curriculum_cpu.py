"""Per-configuration tallies and the resampled pool without a GPU (include/tpl_learn.h's "Per-configuration tallies and the resampled
pool"; csrc/learn/curriculum.hip; the numpy mirrors _learn_lib.assign_entries / pool_resample / curriculum_weights; curriculum.py):

  * the resample mirror: zero-weight entries are never drawn, a single non-zero weight takes every draw, counts 1 / 63 / 64 / 1,000,
    totals near 2^61, the records copied are the source's, and the 1 : 3 split over 4,096 draws is within five binomial standard
    deviations of 3,072 (a fixed hash: the count is pinned);
  * every refusal of resample_pool, curriculum_weights and the mirror comes before any device work;
  * curriculum_weights on hand-made tallies, numpy and torch forms alike;
  * the config-index mirror is the oracle's Env.assign over boards 0 .. 95, births 0 .. 50, both modes, two global offsets, three
    pool sizes;
  * the header declares what LEARN_SYMBOLS lists, the library exports the three entries, their kernels use no scratch, and the host
    entry code refuses every bad argument under ASan + UBSan in a stand-alone program (tests/c_abi/sanitize_curriculum.cpp).
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import tetris_piclim as T


def _m():
    return T._learn_lib


def _pool(n_cfg, M, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 1 << 10, (n_cfg, 20), dtype=np.uint16)
    pieces = rng.integers(0, 7, (n_cfg, M + 1), dtype=np.uint8)
    return rows, pieces


# ---------------------------------------------------------------------------------------------------------------- the resample mirror
@pytest.mark.parametrize("count", [1, 63, 64, 1000])
def test_resample_mirror_never_draws_a_zero_weight_and_copies_the_source_records(count):
    rows, pieces = _pool(37, 40, seed=count)
    weights = np.random.default_rng(1).integers(0, 5, 37).astype(np.int64)
    weights[[0, 5, 36]] = 0
    assert (weights > 0).any()
    r2, p2, source = _m().pool_resample(rows, pieces, weights, count, seed=3, round=2)
    assert source.dtype == np.int32 and source.shape == (count,) and r2.shape == (count, 20) and p2.shape == (count, 41)
    assert source.min() >= 0 and source.max() < 37 and (weights[source] > 0).all()
    assert np.array_equal(r2, rows[source]) and np.array_equal(p2, pieces[source])
    # the seed and the round both move the draws; the same arguments give the same pool
    again = _m().pool_resample(rows, pieces, weights, count, seed=3, round=2)[2]
    assert np.array_equal(source, again)
    if count >= 63:
        assert not np.array_equal(source, _m().pool_resample(rows, pieces, weights, count, seed=3, round=3)[2])
        assert not np.array_equal(source, _m().pool_resample(rows, pieces, weights, count, seed=4, round=2)[2])


@pytest.mark.parametrize("where", [0, 6, 12])
def test_resample_mirror_with_one_nonzero_weight_draws_only_that_entry(where):
    rows, pieces = _pool(13, 2)
    weights = np.zeros(13, np.int64)
    weights[where] = 9
    for count in (1, 63, 64, 1000):
        assert (_m().pool_resample(rows, pieces, weights, count)[2] == where).all()


def test_resample_mirror_with_totals_near_2_to_the_61():
    rows, pieces = _pool(5, 2)
    weights = np.array([(1 << 59) + 3, 0, (1 << 60) - 1, 1, (1 << 59)], np.int64)     # total = 2^61 + 3
    source = _m().pool_resample(rows, pieces, weights, 1000, seed=11)[2]
    counts = np.bincount(source, minlength=5)
    assert counts[1] == 0 and counts.sum() == 1000
    # shares 1/4, 1/2, ~0, 1/4: within five binomial standard deviations
    for k, share in ((0, 0.25), (2, 0.5), (4, 0.25)):
        assert abs(counts[k] - 1000 * share) < 5 * np.sqrt(1000 * share * (1 - share)), counts
    # each draw is the exact integer rule, in Python integers
    total = int(sum(int(w) for w in weights))
    prefix = np.cumsum(weights.astype(object))
    h = _m()._draw_hashes(11, 0, 1000)
    for j in range(0, 1000, 37):
        t = (int(h[j]) * total) >> 64
        assert source[j] == next(e for e in range(5) if prefix[e] > t)


def test_resample_mirror_one_to_three_split_is_binomial_and_pinned():
    rows, pieces = _pool(2, 2)
    source = _m().pool_resample(rows, pieces, np.array([1, 3], np.int64), 4096)[2]
    heavy = int((source == 1).sum())
    sd = np.sqrt(4096 * 0.75 * 0.25)                      # 27.7
    assert abs(heavy - 3072) < 5 * sd, heavy
    assert heavy == PINNED_HEAVY, heavy


PINNED_HEAVY = 3111   # what the fixed hash draws at seed 0, round 0: 1.4 standard deviations above 3,072


def test_mulhi64_mirror_is_exact():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 64, 500, dtype=np.uint64)
    b = rng.integers(0, 1 << 64, 500, dtype=np.uint64)
    a[:3] = [0, (1 << 64) - 1, (1 << 64) - 1]
    b[:3] = [(1 << 64) - 1, (1 << 64) - 1, 1]
    got = _m()._mulhi64(a, b)
    assert [int(x) for x in got] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_resample_refusals_come_before_any_device_work():
    rows, pieces = (torch.from_numpy(x) for x in (_pool(4, 2)[0].view(np.int16), _pool(4, 2)[1]))
    good = torch.tensor([1, 2, 0, 3], dtype=torch.int64)
    bad = [
        (dict(weights=torch.tensor([1, -1, 2, 3], dtype=torch.int64)), "negative"),
        (dict(weights=torch.zeros(4, dtype=torch.int64)), "total"),
        (dict(weights=torch.tensor([1 << 61, 1 << 61, 0, 0], dtype=torch.int64)), "total"),
        (dict(weights=torch.tensor([(1 << 62) - 1, 1, 0, 0], dtype=torch.int64)), "total"),
        (dict(weights=good[:3]), "weights"),
        (dict(weights=good.to(torch.int32)), "weights"),
        (dict(weights=good.to(torch.float64)), "weights"),
        (dict(weights=good.numpy()), "weights"),
        (dict(count=0), "count"),
        (dict(count=-3), "count"),
        (dict(count=2.0), "count"),
        (dict(count=True), "count"),
        (dict(count=1 << 31), "count"),
        (dict(rows=rows[:, :19]), "rows"),
        (dict(rows=rows.to(torch.int32)), "rows"),
        (dict(rows=rows.numpy()), "tensors"),
        (dict(pieces=pieces[:3]), "pieces"),
        (dict(pieces=pieces.to(torch.int16)), "pieces"),
        (dict(pieces=pieces[:, :1]), "pieces"),
    ]
    for change, word in bad:
        kwargs = dict(rows=rows, pieces=pieces, weights=good, count=8)
        kwargs.update(change)
        with pytest.raises(ValueError, match=word):
            T.resample_pool(**kwargs)
    # a total of exactly 2^62 - 1 passes the check of the weights (and is then refused for the device alone, on this CPU pool)
    with pytest.raises(ValueError, match="GPU"):
        T.resample_pool(rows, pieces, torch.tensor([(1 << 62) - 2, 1, 0, 0], dtype=torch.int64), 8)
    # the mirror refuses the same values
    r, p = _pool(4, 2)
    for w, word in (([1, -1, 2, 3], "negative"), ([0, 0, 0, 0], "total"), ([1 << 61, 1 << 61, 0, 0], "total")):
        with pytest.raises(ValueError, match=word):
            _m().pool_resample(r, p, np.array(w, np.int64), 8)
    for kwargs in (dict(weights=np.array([1, 2, 3], np.int64)), dict(weights=np.array([1, 2, 3, 4], np.int32)), dict(count=0),
                   dict(rows=r[:, :19]), dict(pieces=p.astype(np.int16))):
        full = dict(rows=r, pieces=p, weights=np.array([1, 2, 0, 3], np.int64), count=8)
        full.update(kwargs)
        with pytest.raises(ValueError):
            _m().pool_resample(**full)


def test_curriculum_weights_on_hand_made_tallies_and_its_refusals():
    episodes = np.array([0, 5, 5, 9, 1 << 20], np.int32)
    wins = np.array([0, 5, 0, 4, 1], np.int32)
    want = np.array([1, 1, 41, 41, 1 + 8 * ((1 << 20) - 1)], np.int64)
    got = _m().curriculum_weights(episodes, wins)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(_m().curriculum_weights(episodes, wins, floor=0, gain=1), [0, 0, 5, 5, (1 << 20) - 1])
    assert np.array_equal(_m().curriculum_weights(episodes, wins, floor=7, gain=0), [7] * 5)
    # the torch form: the same numbers, int64, from int32 or int64 tallies
    for dtype in (torch.int32, torch.int64):
        t = T.curriculum_weights(torch.from_numpy(episodes).to(dtype), torch.from_numpy(wins).to(dtype))
        assert t.dtype == torch.int64 and np.array_equal(t.numpy(), want)
    # no overflow where int32 arithmetic would: gain * losses above 2^31
    big = T.curriculum_weights(torch.tensor([1 << 30], dtype=torch.int32), torch.tensor([0], dtype=torch.int32), gain=1 << 20)
    assert int(big[0]) == 1 + (1 << 50)
    e, w = torch.from_numpy(episodes), torch.from_numpy(wins)
    for kwargs in (dict(floor=-1), dict(gain=-1), dict(floor=1.5), dict(gain=True)):
        with pytest.raises(ValueError):
            T.curriculum_weights(e, w, **kwargs)
        with pytest.raises(ValueError):
            _m().curriculum_weights(episodes, wins, **kwargs)
    with pytest.raises(ValueError):
        T.curriculum_weights(e, w[:4])
    with pytest.raises(ValueError):
        T.curriculum_weights(e.to(torch.float32), w)
    with pytest.raises(ValueError):
        T.curriculum_weights(episodes, wins)


# ---------------------------------------------------------------------------------------------------------------- the assignment
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("global_offset", [0, (1 << 33) + 5])
@pytest.mark.parametrize("n_cfg", [1, 7, 200])
def test_config_index_mirror_is_the_oracles_assignment(oracle, mode, global_offset, n_cfg):
    boards, births, seed, M = 96, 51, 12345, 3
    env = oracle.Env(boards, 2, M, global_offset, seed)
    rows, pieces = _pool(n_cfg, M)
    env.set_pool(rows, pieces)
    env.set_options(auto_reset=True, assign_mode=mode)
    b, t = np.meshgrid(np.arange(boards), np.arange(births), indexing="ij")
    got = _m().assign_entries(b, t, seed, global_offset, n_cfg, mode)
    want = np.array([[env.assign(i, k) for k in range(births)] for i in range(boards)])
    assert got.dtype == np.int64 and got.min() >= 0 and got.max() < n_cfg
    assert np.array_equal(got, want)
    # and at births past 2^32, where the hash reads the high word and the sequential mode only the low one
    high = np.array([(1 << 32) + 3, (1 << 40) + 7, (1 << 63) + 11], dtype=np.uint64)
    got = _m().assign_entries(np.arange(boards)[:, None], high[None, :], seed, global_offset, n_cfg, mode)
    want = np.array([[env.assign(i, int(k)) for k in high] for i in range(boards)])
    assert np.array_equal(got, want)
    env.close()


def test_config_index_mirror_refusals():
    for kwargs in (dict(mode=2), dict(n_cfg=0), dict(n_cfg=1 << 32), dict(global_offset=-1)):
        full = dict(boards=[0], births=[0], seed=0, global_offset=0, n_cfg=4, mode=0)
        full.update(kwargs)
        with pytest.raises(ValueError):
            _m().assign_entries(**full)


# ---------------------------------------------------------------------------------------------------------------- the library
ENTRIES = ("tpl_config_index", "tpl_pool_tally", "tpl_pool_resample")
KERNELS = ("config_index_kernel", "pool_tally_kernel", "pool_resample_kernel")


def test_header_symbols_and_kernels_agree():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and set(ENTRIES) <= declared
    lib = _m().lib()
    for name in ENTRIES:
        assert hasattr(lib, name)
    assert any(p.endswith(os.path.join("learn", "curriculum.hip")) for p in _m()._sources())
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _m().build_library()],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    for want in KERNELS:
        mine = [r for r in rows if want in r[-1]]
        assert mine, want
        for r in mine:
            assert r[r.index("scratch") - 1] == "0", r


def test_argument_errors_come_back_as_statuses_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                       # never dereferenced: every call below is refused before any HIP call
    assert lib.tpl_config_index(None, fake, fake, 4, 0, 0, 0, 7, 0, fake, fake, None) < 0 and b"null" in err()
    assert lib.tpl_config_index(fake, fake, fake, 4, 0, 0, 0, 0, 0, fake, fake, None) < 0 and b"no pool" in err()
    assert lib.tpl_config_index(fake, fake, fake, 4, 0, 0, 5, 7, 0, fake, fake, None) < 0 and b"assign_mode" in err()
    assert lib.tpl_pool_tally(fake, fake, fake, 4, 2, 3, fake, 0, 0, 0, 0, 7, 0, None, None, None, None, None) < 0 \
        and b"at least one" in err()
    assert lib.tpl_pool_tally(fake, fake, fake, 4, 2, 3, fake, 9, 0, 0, 0, 7, 0, fake, fake, None, None, None) < 0 and b"dtype" in err()
    assert lib.tpl_pool_resample(fake, fake, 4, 2, fake, 0, 0, 0, fake * 2, fake * 2, fake, None) < 0 and b"count" in err()
    assert lib.tpl_pool_resample(fake, fake, 4, 2, fake, 4, 0, 0, fake, fake * 2, fake, None) < 0 and b"must not be" in err()


def test_host_entry_code_under_address_and_ub_sanitizers(tmp_path):
    """The host side of csrc/learn/curriculum.hip (the three entries' argument checks) compiled host-only with
    -fsanitize=address,undefined and driven by a stand-alone program over every refusal path.  Nothing is loaded into Python."""
    flags = ["--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
             "-I", os.path.join(ROOT, "include")]
    exe = str(tmp_path / "sanitize_curriculum")
    cmd = ["hipcc"] + flags + [os.path.join(_m()._LEARN_CSRC, "curriculum.hip"),
                               os.path.join(ROOT, "tests", "c_abi", "sanitize_curriculum.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "sanitizer run ok" in res.stdout, res.stdout + res.stderr
