"""The step kernel across its geometries and output pointers (round 10).  Written for three candidates measured together -- a wave
that owns 64 * boards-per-lane ADJACENT boards with one clock load and one clock store, `done` leaving as whole dwords built from
the lanes' ballots where a wave's boards all lie inside the batch and the row is 4-byte aligned, and the block's tally of finished
episodes sent by the wave that counts itself in last instead of behind a barrier at the end (profiles/NOTES.md: the tally is what
the tree holds) -- and kept as what any new mapping of boards to lanes, any wider output store and any change to the tally has to
pass, as equality with the C oracle (integer work on both sides): a size on either side of every wave footprint (64, 128, 256
boards) and block footprint of every geometry, a `done` row at every alignment with the bytes around it guarded, a row of a
matrix whose rows are no multiple of four, `cleared` requested, wide actions, the statistics of every geometry, a snapshot, a
captured graph, and two shards of odd size.

The oracle plays each case ONCE (45 steps, the actions recorded); every geometry then replays the recorded actions on the device
and must give the recorded rewards, flags, rows cleared, final state and statistics.  Pool entries come in three kinds (entry
index mod 3, tests/test_step_requests_gpu.py): 0 an empty board dealt squares, played by the column script that lives through all
M moves (a refill at every tenth move, the end at the move limit); 1 an empty board with synthetic pieces and 2 a synthetic board,
both under the synthetic random policy (top-outs at every age).  The case's seed is the first for which the ORACLE's run shows a
finished episode (a reset with auto-reset), a window refill and an M-th move.
"""
import ctypes as C

import numpy as np
import pytest

from test_step_requests_gpu import O_COLUMNS, O_PIECE, _assert_state_equal, _np, _state

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 511, 512, 513, 1023, 1025, 1537, 2049]
GEOMETRIES = [(bpl, threads) for bpl in (1, 2, 4) for threads in (64, 256, 512)]
SHAPES = [(3, 10), (10, 40)]
STEPS = 45
POOL = 12
REWARD = (1.0, 0.5, -0.25)              # per line, win, loss: exact in binary
GUARD = 0xAB

_references = {}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import tetris_piclim
    return tetris_piclim


def make_pool(oracle, L, M, seed):
    rows = oracle.synth_boards(seed, 0, POOL, L).copy()
    pieces = oracle.synth_pieces(seed, 0, POOL, M).copy()
    rows[0::3] = 0
    rows[1::3] = 0
    pieces[0::3] = O_PIECE
    return rows, pieces


def _play(oracle, n, L, M, auto, seed, offset):
    """45 steps of the oracle alone; the actions it was given, what it answered, and what the run exercised."""
    pool = make_pool(oracle, L, M, seed + 1)
    cpu = oracle.Env(n, L, M, offset, seed)
    cpu.set_pool(*pool)
    cpu.set_options(auto_reset=auto, assign_mode=0, per_line=REWARD[0], win=REWARD[1], lose=REWARD[2])
    cpu.reset()
    kind = np.array([cpu.assign(b, 0) % 3 for b in range(n)])
    ref = dict(seed=seed, pool=pool, offset=offset, actions=np.empty((STEPS, n), np.uint8), reward=np.empty((STEPS, n), np.float32),
               done=np.empty((STEPS, n), np.uint8), cleared=np.empty((STEPS, n), np.uint8), states=[],
               finished=0, refills=0, mth_moves=0)
    for t in range(STEPS):
        before = cpu.get_state()
        a = oracle.synth_actions(seed, offset, n, t).copy()
        scripted = kind == 0
        a[scripted] = O_COLUMNS[before["moves"][scripted].astype(np.int64) % len(O_COLUMNS)]
        r, d, c = cpu.move(a // 10, a % 10)
        ref["actions"][t], ref["reward"][t], ref["done"][t], ref["cleared"][t] = a, r, d, c
        moving = before["state"] == 0
        move_no = before["moves"].astype(np.int64) + 1
        finished = moving & d.astype(bool)
        ref["finished"] += int(finished.sum())
        ref["refills"] += int((moving & (move_no % 10 == 0)).sum())
        ref["mth_moves"] += int((moving & (move_no == M)).sum())
        if auto:
            for b in np.flatnonzero(finished):
                kind[b] = cpu.assign(int(b), cpu.birth(int(b))) % 3
        ref["states"].append(cpu.get_state())
    ref["stats"] = cpu.stats()
    assert cpu.clock == STEPS
    cpu.close()
    return ref


def reference(oracle, n, L, M, auto, offset=0):
    key = (n, L, M, auto, offset)
    if key not in _references:
        for seed in range(1000 + n, 1060 + n):
            ref = _play(oracle, n, L, M, auto, seed, offset)
            if ref["finished"] and ref["refills"] and ref["mth_moves"]:
                break
        _references[key] = ref
    return _references[key]


def assert_exercised(ref, ctx):
    """A finished episode (with auto-reset that is a reset from the pool), a window refill and an M-th move all occurred."""
    assert ref["finished"] > 0 and ref["refills"] > 0 and ref["mth_moves"] > 0, f"{ctx}: {ref['finished']}, {ref['refills']}, {ref['mth_moves']}"


def make_env(T, ref, n, L, M, auto, offset=None):
    gpu = T.BatchedTetris(L, M, n, seed=ref["seed"], global_offset=ref["offset"] if offset is None else offset, auto_reset=auto,
                          reward=REWARD)
    gpu.load_configs(*ref["pool"])
    return gpu


def replay(gpu, actions, first=0, last=STEPS):
    """Steps first .. last - 1 with the recorded actions (a device tensor [STEPS, n] of any integer type); rewards and flags of
    those steps as numpy arrays."""
    import torch
    n = gpu.num_envs
    rewards = torch.empty((last - first, n), dtype=torch.float32, device=gpu.device)
    dones = torch.empty((last - first, n), dtype=torch.uint8, device=gpu.device)
    for t in range(first, last):
        gpu.step_into(actions[t], rewards[t - first], dones[t - first])
    return _np(rewards), _np(dones)


def assert_run_equal(gpu, got, ref, ctx, first=0, last=STEPS, lo=0, hi=None):
    rewards, dones = got
    assert np.array_equal(rewards, ref["reward"][first:last, lo:hi]), f"{ctx}: reward"
    assert np.array_equal(dones, ref["done"][first:last, lo:hi]), f"{ctx}: done"
    want = {k: v[lo:hi] for k, v in ref["states"][last - 1].items()}
    _assert_state_equal(_state(gpu), want, ctx)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("L,M", SHAPES)
def test_every_geometry_replays_the_oracles_run(T, oracle, L, M, auto, n):
    """Sizes around every wave footprint (64, 128, 256 boards) and block footprint (64 .. 2048) x nine geometries: rewards, flags,
    the final state, the statistics and the step clock.  One environment per case: a full reset puts it back to step 0, and the
    geometry changes under it (the clock words of the padding are written by whichever geometry ran last)."""
    import torch
    ref = reference(oracle, n, L, M, auto)
    assert_exercised(ref, f"L={L} M={M} n={n} auto={auto}")
    gpu = make_env(T, ref, n, L, M, auto)
    actions = torch.from_numpy(ref["actions"]).to(gpu.device)
    for bpl, threads in GEOMETRIES:
        ctx = f"L={L} M={M} n={n} auto={auto} bpl={bpl} threads={threads}"
        gpu.set_tuning(bpl, threads)
        gpu.reset()
        assert_run_equal(gpu, replay(gpu, actions), ref, ctx)
        assert gpu.stats() == ref["stats"], ctx
        assert gpu.step_clock() == STEPS, ctx
    gpu.terminate()


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("n", [65, 257, 1025])
@pytest.mark.parametrize("L,M", SHAPES)
def test_wide_actions(T, oracle, L, M, n, dtype):
    """The recorded actions as 4- and 8-byte integers (the uint8 form is what every other test here uses)."""
    import torch
    for auto in (True, False):
        ref = reference(oracle, n, L, M, auto)
        gpu = make_env(T, ref, n, L, M, auto)
        actions = torch.from_numpy(ref["actions"].astype(dtype)).to(gpu.device)
        for bpl, threads in GEOMETRIES:
            ctx = f"{dtype}: L={L} M={M} n={n} auto={auto} bpl={bpl} threads={threads}"
            gpu.set_tuning(bpl, threads)
            gpu.reset()
            assert_run_equal(gpu, replay(gpu, actions), ref, ctx)
            assert gpu.stats() == ref["stats"], ctx
        gpu.terminate()


def _guarded(torch, device, dtype, n, lead):
    """A buffer of n elements `lead` elements into an allocation filled with the guard byte; (whole allocation, the view)."""
    size = torch.empty((), dtype=dtype).element_size()
    whole = torch.full(((lead + n + 16) * size,), GUARD, dtype=torch.uint8, device=device).view(dtype)
    return whole, whole[lead:lead + n]


def _assert_guards(whole, lead, n, ctx):
    raw = _np(whole).view(np.uint8)
    size = whole.element_size()
    assert (raw[:lead * size] == GUARD).all(), f"{ctx}: bytes in front of the buffer were written"
    assert (raw[(lead + n) * size:] == GUARD).all(), f"{ctx}: bytes behind the buffer were written"


@pytest.mark.parametrize("skew", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [129, 257, 514])
@pytest.mark.parametrize("L,M", SHAPES)
def test_done_row_at_every_alignment_with_guard_bytes(T, oracle, L, M, n, skew):
    """`done` starting 0, 1, 2 and 3 bytes past a 4-byte boundary (only the first could leave as dwords), `reward` one float past a
    16-byte boundary: the values are the oracle's and the sixteen bytes on either side keep the guard pattern.  The sizes have
    full waves in front of a partial one at every geometry with more than one board per lane."""
    import torch
    ref = reference(oracle, n, L, M, True)
    gpu = make_env(T, ref, n, L, M, True)
    actions = torch.from_numpy(ref["actions"]).to(gpu.device)
    lead = 16 + skew
    for bpl, threads in GEOMETRIES:
        ctx = f"skew {skew}: L={L} M={M} n={n} bpl={bpl} threads={threads}"
        gpu.set_tuning(bpl, threads)
        gpu.reset()
        done_whole, done = _guarded(torch, gpu.device, torch.uint8, n, lead)
        reward_whole, reward = _guarded(torch, gpu.device, torch.float32, n, 1)
        assert done.data_ptr() % 4 == skew and reward.data_ptr() % 16 == 4
        for t in range(STEPS):
            done.fill_(GUARD)
            gpu.step_into(actions[t], reward, done)
            assert np.array_equal(_np(done), ref["done"][t]), f"{ctx}: done at step {t}"
            assert np.array_equal(_np(reward), ref["reward"][t]), f"{ctx}: reward at step {t}"
        _assert_guards(done_whole, lead, n, ctx)
        _assert_guards(reward_whole, 1, n, ctx)
        assert gpu.stats() == ref["stats"], ctx
    gpu.terminate()


@pytest.mark.parametrize("n", [129, 257, 514, 1025])
@pytest.mark.parametrize("L,M", SHAPES)
def test_done_as_a_row_of_a_matrix_whose_rows_are_no_multiple_of_four(T, oracle, L, M, n):
    """Step t writes row t of a [STEPS + 2, n] matrix of flags: consecutive rows start at every alignment in turn (n mod 4 is 1 or
    2), so a store wider than a byte would have to alternate with the byte form from step to step; the rows in front and behind and every row's neighbours
    show that no store crossed a row's end."""
    import torch
    assert n % 4 != 0
    ref = reference(oracle, n, L, M, True)
    gpu = make_env(T, ref, n, L, M, True)
    actions = torch.from_numpy(ref["actions"]).to(gpu.device)
    for bpl, threads in GEOMETRIES:
        ctx = f"rows: L={L} M={M} n={n} bpl={bpl} threads={threads}"
        gpu.set_tuning(bpl, threads)
        gpu.reset()
        dones = torch.full((STEPS + 2, n), GUARD, dtype=torch.uint8, device=gpu.device)
        rewards = torch.empty((STEPS, n), dtype=torch.float32, device=gpu.device)
        for t in range(STEPS):
            gpu.step_into(actions[t], rewards[t], dones[t + 1])
        got = _np(dones)
        assert (got[0] == GUARD).all() and (got[-1] == GUARD).all(), f"{ctx}: a guard row was written"
        assert np.array_equal(got[1:-1], ref["done"]), f"{ctx}: done"
        assert np.array_equal(_np(rewards), ref["reward"]), f"{ctx}: reward"
    gpu.terminate()


@pytest.mark.parametrize("n", [129, 257, 514])
@pytest.mark.parametrize("L,M", SHAPES)
def test_rows_cleared_beside_the_flags_with_guard_bytes(T, oracle, L, M, n):
    """The move form of the entry point with `cleared` requested (tpl_move: rotation and column apart), every output guarded."""
    import torch
    TPL_U8, check = T._lib.TPL_U8, T._lib.check
    ref = reference(oracle, n, L, M, True)
    gpu = make_env(T, ref, n, L, M, True)
    rot = torch.from_numpy(ref["actions"] // 10).to(gpu.device)
    loc = torch.from_numpy(ref["actions"] % 10).to(gpu.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for bpl, threads in GEOMETRIES:
        ctx = f"cleared: L={L} M={M} n={n} bpl={bpl} threads={threads}"
        gpu.set_tuning(bpl, threads)
        gpu.reset()
        done_whole, done = _guarded(torch, gpu.device, torch.uint8, n, 16)
        cleared_whole, cleared = _guarded(torch, gpu.device, torch.uint8, n, 19)
        reward_whole, reward = _guarded(torch, gpu.device, torch.float32, n, 1)
        for t in range(STEPS):
            check(gpu._lib.tpl_move(gpu._h, ptr(rot[t]), ptr(loc[t]), TPL_U8, ptr(reward), ptr(done), ptr(cleared), gpu._stream()))
            assert np.array_equal(_np(done), ref["done"][t]), f"{ctx}: done at step {t}"
            assert np.array_equal(_np(cleared), ref["cleared"][t]), f"{ctx}: cleared at step {t}"
            assert np.array_equal(_np(reward), ref["reward"][t]), f"{ctx}: reward at step {t}"
        _assert_guards(done_whole, 16, n, ctx)
        _assert_guards(cleared_whole, 19, n, ctx)
        _assert_guards(reward_whole, 1, n, ctx)
        _assert_state_equal(_state(gpu), ref["states"][-1], ctx)
        assert gpu.stats() == ref["stats"], ctx
    gpu.terminate()


@pytest.mark.parametrize("L,M", SHAPES)
def test_snapshot_and_restore_mid_run_reproduce_the_run(T, oracle, L, M):
    """A snapshot after 20 steps (boards, step clocks and statistics): the 25 steps behind it, played twice, are the oracle's
    both times, and so are the statistics."""
    import torch
    n, cut = 513, 20
    ref = reference(oracle, n, L, M, True)
    gpu = make_env(T, ref, n, L, M, True)
    actions = torch.from_numpy(ref["actions"]).to(gpu.device)
    for bpl, threads in GEOMETRIES:
        ctx = f"snapshot: L={L} M={M} bpl={bpl} threads={threads}"
        gpu.set_tuning(bpl, threads)
        gpu.reset()
        assert_run_equal(gpu, replay(gpu, actions, 0, cut), ref, ctx, 0, cut)
        saved = gpu.snapshot()
        for again in range(2):
            assert_run_equal(gpu, replay(gpu, actions, cut, STEPS), ref, f"{ctx} pass {again}", cut, STEPS)
            assert gpu.stats() == ref["stats"] and gpu.step_clock() == STEPS, f"{ctx} pass {again}"
            gpu.restore(saved)
        assert gpu.step_clock() == cut, ctx
    gpu.terminate()


@pytest.mark.parametrize("L,M", SHAPES)
def test_captured_graph_replayed_equals_eager(T, oracle, L, M):
    """Five steps in one HIP graph, replayed nine times with the recorded actions: what the eager launches give (the oracle's
    run)."""
    import torch
    n, K = 1025, 5
    ref = reference(oracle, n, L, M, True)
    gpu = make_env(T, ref, n, L, M, True)
    recorded = torch.from_numpy(ref["actions"]).to(gpu.device)
    for bpl, threads in GEOMETRIES:
        ctx = f"graph: L={L} M={M} bpl={bpl} threads={threads}"
        gpu.set_tuning(bpl, threads)
        gpu.reset()
        actions = torch.empty((K, n), dtype=torch.uint8, device=gpu.device)
        rewards = torch.empty((K, n), dtype=torch.float32, device=gpu.device)
        dones = torch.empty((K, n), dtype=torch.uint8, device=gpu.device)
        run = gpu.capture_steps(actions, rewards, dones)
        for block in range(STEPS // K):
            actions.copy_(recorded[K * block:K * block + K])
            run()
            assert np.array_equal(_np(rewards), ref["reward"][K * block:K * block + K]), f"{ctx}: reward in block {block}"
            assert np.array_equal(_np(dones), ref["done"][K * block:K * block + K]), f"{ctx}: done in block {block}"
        _assert_state_equal(_state(gpu), ref["states"][-1], ctx)
        assert gpu.stats() == ref["stats"], ctx
    gpu.terminate()


@pytest.mark.parametrize("L,M", SHAPES)
def test_two_shards_of_odd_size_equal_one_environment(T, oracle, L, M):
    """1,026 boards as one environment and as two of 513 with global offsets 0 and 513: the same boards, by the oracle's run of
    all 1,026 and by each other; the shards' statistics add up."""
    import torch
    n = 1026
    half = n // 2
    ref = reference(oracle, n, L, M, True)
    whole = make_env(T, ref, n, L, M, True)
    shards = [make_env(T, ref, half, L, M, True, offset=k * half) for k in range(2)]
    actions = torch.from_numpy(ref["actions"]).to(whole.device)
    parts = [actions[:, k * half:(k + 1) * half].contiguous() for k in range(2)]
    for bpl, threads in GEOMETRIES:
        ctx = f"shards: L={L} M={M} bpl={bpl} threads={threads}"
        whole.set_tuning(bpl, threads)
        whole.reset()
        got_whole = replay(whole, actions)
        assert_run_equal(whole, got_whole, ref, ctx)
        total = dict.fromkeys(ref["stats"], 0)
        for k, shard in enumerate(shards):
            shard.set_tuning(bpl, threads)
            shard.reset()
            got = replay(shard, parts[k])
            assert_run_equal(shard, got, ref, f"{ctx} shard {k}", lo=k * half, hi=(k + 1) * half)
            assert np.array_equal(got[0], got_whole[0][:, k * half:(k + 1) * half]), f"{ctx} shard {k}: reward against the whole"
            assert np.array_equal(got[1], got_whole[1][:, k * half:(k + 1) * half]), f"{ctx} shard {k}: done against the whole"
            for name, value in shard.stats().items():
                total[name] += value
        assert total == ref["stats"] == whole.stats(), ctx
    for env in [whole] + shards:
        env.terminate()
