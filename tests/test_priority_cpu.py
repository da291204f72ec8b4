"""CPU-side checks of prioritized replay (include/tpl_learn.h, csrc/learn/priority.hip, _learn_lib's numpy mirror): the mirror's
descent is a search over exact prefix sums and never reaches a zero leaf, its stratified draws follow p / total, the clamp and
duplicate rules of the write-back, the tree's size, the host draw target against the library's, and every new entry point
refusing bad arguments before any GPU work."""
import os

import numpy as np
import pytest

from conftest import ROOT

import tetris_piclim as T


def _L():
    return T._learn_lib


def _tree_with_leaves(leaves):
    L = _L()
    tree = L.priority_tree_init(len(leaves))
    tree[L.PRIORITY_HEADER_WORDS:L.PRIORITY_HEADER_WORDS + len(leaves)] = leaves
    L.priority_tree_resum(tree)
    return tree


@pytest.mark.parametrize("capacity", [1, 15, 16, 17, 255, 256, 4500, (1 << 20) + 3])
def test_descent_is_a_search_over_exact_prefix_sums(capacity):
    """Integer priorities keep every sum and every u - prefix exact, so the descent must take the first slot whose prefix sum
    exceeds u (the last non-empty slot if rounding puts u at the total).  A third of the slots, the last one included, are 0."""
    L = _L()
    gen = np.random.default_rng(capacity)
    p = gen.integers(1, 1000, capacity).astype(np.float64)
    p[gen.random(capacity) < 1 / 3] = 0.0
    p[-1] = 0.0
    if not p.any():
        p[0] = 7.0
    tree = _tree_with_leaves(p)
    offsets, counts, _ = L.priority_layout(capacity)
    prefix = np.cumsum(p)
    assert tree[offsets[-1]] == prefix[-1] and counts[-1] == 1
    last_positive = int(np.flatnonzero(p)[-1])
    for seed, update, batch in ((0, 0, 1), (3, 1, 1000), ((1 << 64) - 1, 7, 4096)):
        idx, prob = L.prioritized_draws(tree, seed, update, batch)
        u = L.priority_targets(seed, update, batch, prefix[-1])
        want = np.minimum(np.searchsorted(prefix, u, side="right"), last_positive)
        assert np.array_equal(idx, want), (seed, update)
        assert (p[idx] > 0).all()                                          # zero leaves are never drawn
        assert np.array_equal(prob, (p[idx] / prefix[-1]).astype(np.float32))


def test_zero_leaves_are_never_drawn_even_when_rounding_leaves_u_at_the_total():
    L = _L()
    p = np.zeros(4500)
    p[[0, 17, 4095, 4496]] = [1e-12, 3.0, 1e30, 0.1]                       # sums that round
    tree = _tree_with_leaves(p)
    for update in range(8):
        idx, prob = L.prioritized_draws(tree, 5, update, 1 << 16)
        assert set(np.unique(idx)) <= {0, 17, 4095, 4496}
        assert (prob > 0).all()
    # a tree that was only pushed into draws only pushed slots
    tree = L.priority_tree_init(4500)
    L.priority_tree_push(tree, 4000, 700)                                  # wraps: slots 4000..4499 and 0..199
    idx, _ = L.prioritized_draws(tree, 1, 0, 1 << 16)
    assert ((idx >= 4000) | (idx < 200)).all()


def test_stratified_draw_frequencies_follow_p_over_total():
    L = _L()
    gen = np.random.default_rng(11)
    size = 1000
    p = gen.integers(1, 50, size).astype(np.float64) * gen.choice([1e-3, 1.0, 30.0], size)
    p[::97] = 0.0
    tree = _tree_with_leaves(p)
    counts = np.zeros(size)
    draws = 0
    for update in range(32):
        idx, _ = L.prioritized_draws(tree, 2, update, 65536)
        counts += np.bincount(idx, minlength=size)
        draws += idx.size
    assert counts[p == 0].sum() == 0
    live = p > 0
    expected = draws * p[live] / p.sum()
    chi2 = float(((counts[live] - expected) ** 2 / expected).sum())
    dof = int(live.sum()) - 1
    # stratification only lowers the spread below a multinomial draw's: mean dof, sd sqrt(2 dof); 5 sd out
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)


def test_write_back_clamps_and_takes_the_largest_of_duplicates():
    L = _L()
    tree = L.priority_tree_init(64)
    L.priority_tree_push(tree, 0, 64)
    leaves = tree[L.PRIORITY_HEADER_WORDS:L.PRIORITY_HEADER_WORDS + 64]
    assert (leaves == 1.0).all() and tree[0] == 1.0
    L.priority_tree_update(tree, [3, 4], [5.0, 0.25])
    assert leaves[3] == 5.0 and leaves[4] == 0.25 and tree[0] == 5.0
    # a slot's new priority replaces its old one even when smaller (the drawn leaves are zeroed first); duplicates take the
    # largest; NaN, -inf, 0, -0 and negatives become 1e-12, +inf 1e30; indices outside the ring are ignored
    L.priority_tree_update(tree, [3, 3, 3, 7, 8, 9, 10, 11, 12, 13, -1, 64],
                           [2.0, 3.0, 1.0, np.nan, np.inf, -np.inf, 0.0, -1.0, -0.0, 1e-300, 99.0, 99.0])
    assert leaves[3] == 3.0
    assert leaves[8] == 1e30
    assert (leaves[[7, 9, 10, 11, 12, 13]] == 1e-12).all()
    assert tree[0] == 1e30                                                  # the running maximum
    assert np.array_equal(L.clamp_priorities([np.nan, -np.inf, np.inf, 0.5]), [1e-12, 1e-12, 1e30, 0.5])
    # the rule is np.maximum.at after zeroing
    gen = np.random.default_rng(3)
    index = gen.integers(0, 64, 500)
    pr = gen.random(500) * 10
    t2 = tree.copy()
    L.priority_tree_update(t2, index, pr)
    want = leaves.copy()
    want[index] = 0.0
    np.maximum.at(want, index, pr)
    assert np.array_equal(t2[L.PRIORITY_HEADER_WORDS:L.PRIORITY_HEADER_WORDS + 64], want)
    # a later push gives the running maximum
    L.priority_tree_push(tree, 60, 8)
    assert (leaves[[60, 61, 62, 63, 0, 1, 2, 3]] == 1e30).all()


def test_tree_layout_and_size():
    L, lib = _L(), _L().lib()
    assert lib.tpl_priority_tree_bytes(0) == 0 and lib.tpl_priority_tree_bytes(1 << 32) == 0
    assert lib.tpl_priority_tree_bytes(-5) == 0
    caps = [1, 2, 15, 16, 17, 255, 256, 257, 4500, 65536, (1 << 20) + 3, 1 << 22, 1 << 24, (1 << 32) - 1]
    caps += list(np.random.default_rng(0).integers(1, 1 << 32, 50))
    for cap in caps:
        cap = int(cap)
        offsets, counts, words = L.priority_layout(cap)
        assert lib.tpl_priority_tree_bytes(cap) == 8 * words, cap
        assert 8 * words <= 8.6 * cap + 2048, cap
        assert offsets[0] == 16 and all(o % 16 == 0 for o in offsets)      # every level on a 128-byte line
        assert counts[-1] == 1 and len(offsets) <= 9
        assert all(counts[k] == -(-counts[k - 1] // 16) for k in range(1, len(counts)))
    # a draw reads ceil(log16 capacity) lines: 6 at 2^24
    assert len(L.priority_layout(1 << 24)[0]) - 1 == 6
    tree = L.priority_tree_init(4500)
    assert tree[0] == 1.0 and tree.view(np.int64)[1] == 4500 and tree.view(np.int64)[2] == 5
    assert not tree[3:].any()


def test_host_draw_target_is_the_library_target_bit_for_bit():
    L, lib = _L(), _L().lib()
    for seed, update, batch, total in ((0, 0, 1, 1.0), (1, 2, 1000, 4500.0), ((1 << 64) - 1, (1 << 40) + 5, 65536, 3e30 + 7),
                                       (12345, 3, 777, 0.1), (9, 0, 1 << 20, 2.0 ** 40 + 0.5)):
        want = L.priority_targets(seed, update, batch, total)
        picks = sorted({0, batch // 2, batch - 1} | set(np.random.default_rng(seed % 1000).integers(0, batch, 200).tolist()))
        got = np.array([lib.tpl_priority_target(seed, update, int(i), batch, total) for i in picks])
        assert np.array_equal(got.view(np.int64), want[picks].view(np.int64)), (seed, update)
        assert (want >= 0).all() and (want <= total).all()
    assert lib.tpl_priority_target(0, 0, 0, 0, 1.0) == -1.0
    assert lib.tpl_priority_target(0, 0, 5, 5, 1.0) == -1.0
    assert lib.tpl_priority_target(0, 0, -1, 5, 1.0) == -1.0


def test_every_priority_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _L().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                     # 128-byte aligned, never dereferenced: every call below is refused
    big = 1 << 32
    # init
    assert lib.tpl_priority_init(None, 16, None) < 0 and b"null" in err()
    assert lib.tpl_priority_init(fake, 0, None) < 0 and b"capacity" in err()
    assert lib.tpl_priority_init(fake, big, None) < 0 and b"capacity" in err()
    assert lib.tpl_priority_init(fake + 64, 16, None) < 0 and b"aligned" in err()
    # push
    assert lib.tpl_priority_push(None, 16, 0, 4, None) < 0 and b"null" in err()
    assert lib.tpl_priority_push(fake, 0, 0, 4, None) < 0 and b"capacity" in err()
    assert lib.tpl_priority_push(fake, big, 0, 4, None) < 0 and b"capacity" in err()
    assert lib.tpl_priority_push(fake, 16, 16, 4, None) < 0 and b"head" in err()
    assert lib.tpl_priority_push(fake, 16, -1, 4, None) < 0 and b"head" in err()
    assert lib.tpl_priority_push(fake, 16, 0, 0, None) < 0 and b"count" in err()
    assert lib.tpl_priority_push(fake, 16, 0, 17, None) < 0 and b"count" in err()
    assert lib.tpl_priority_push(fake + 8, 16, 0, 4, None) < 0 and b"aligned" in err()
    # update
    assert lib.tpl_priority_update(None, 16, 4, fake, fake, None) < 0 and b"null" in err()
    assert lib.tpl_priority_update(fake, 16, 4, None, fake, None) < 0 and b"null" in err()
    assert lib.tpl_priority_update(fake, 16, 4, fake, None, None) < 0 and b"null" in err()
    assert lib.tpl_priority_update(fake, 0, 4, fake, fake, None) < 0 and b"capacity" in err()
    assert lib.tpl_priority_update(fake, big, 4, fake, fake, None) < 0 and b"capacity" in err()
    assert lib.tpl_priority_update(fake, 16, 0, fake, fake, None) < 0 and b"batch" in err()
    assert lib.tpl_priority_update(fake + 16, 16, 4, fake, fake, None) < 0 and b"aligned" in err()
    assert lib.tpl_priority_update(fake, 16, 4, fake + 4, fake, None) < 0 and b"aligned" in err()

    # prioritized sample
    def sample(ring=fake, tree=fake, cap=16, size=16, batch=8, dtype=0, obs=fake, index=fake, prob=fake, L=2, M=2):
        return lib.tpl_replay_sample_prioritized(ring, tree, cap, size, batch, 0, 0, L, M, obs, dtype, fake, fake, fake, fake,
                                                 fake, index, prob, None)

    assert sample(ring=None) < 0 and b"null" in err()
    assert sample(tree=None) < 0 and b"null" in err()
    assert sample(index=None) < 0 and b"null" in err()
    assert sample(prob=None) < 0 and b"null" in err()
    assert sample(cap=0) < 0 and b"capacity" in err()
    assert sample(cap=big, size=16) < 0 and b"capacity" in err()
    assert sample(size=0) < 0 and b"size" in err()
    assert sample(size=17) < 0 and b"size" in err()
    assert sample(batch=0) < 0 and b"batch" in err()
    assert sample(dtype=7) < 0 and b"dtype" in err()
    assert sample(tree=fake + 16) < 0 and b"aligned" in err()
    assert sample(obs=fake + 4) < 0 and b"aligned" in err()
    assert sample(L=0) < 0 and b"L and M" in err()
    # the mirror refuses what the library refuses
    with pytest.raises(ValueError):
        _L().priority_layout(0)
    with pytest.raises(ValueError):
        _L().priority_tree_push(_L().priority_tree_init(16), 16, 1)


def test_priority_sources_are_in_the_digest_and_their_kernels_use_no_scratch():
    import subprocess
    rel = {os.path.relpath(p, ROOT).split(os.sep, 1)[-1] for p in _L()._sources()}
    for want in ("csrc/learn/priority.hip", "csrc/learn/tpl_replay_draw.h"):
        assert any(r.endswith(want) for r in rel), want
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _L().build_library()],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    names = [r[-1] for r in rows]
    for want in ("priority_init_kernel", "priority_push_kernel", "priority_resum_range_kernel", "priority_zero_kernel",
                 "priority_max_kernel", "priority_resum_index_kernel", "replay_sample_prioritized_kernelIf",
                 "replay_sample_prioritized_kernelI14__hip_bfloat16"):
        assert any(want in n for n in names), (want, names)
    for r in rows:
        assert r[r.index("scratch") - 1] == "0", r
    for rel in ("csrc/learn/priority.hip", "csrc/learn/tpl_replay_draw.h"):
        assert "oracle" not in open(os.path.join(os.path.dirname(T.__file__), rel)).read().lower(), rel


def test_the_prioritized_ring_is_exported_lazily():
    assert "PrioritizedReplayRing" in T.__all__
    assert T.PrioritizedReplayRing.__mro__[1] is T.ReplayRing
    import inspect
    params = list(inspect.signature(T.DQNLearner.__init__).parameters)
    assert params[-6:] == ["prioritized", "alpha", "beta", "beta_final", "beta_updates", "priority_eps"]
    assert params[:13] == ["self", "env", "model", "capacity", "batch_size", "gamma", "eps_start", "eps_end", "eps_decay",
                           "tau", "lr", "seed", "prioritized"]
