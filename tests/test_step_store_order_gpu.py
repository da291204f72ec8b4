"""The end of the step kernel: which boards are stored as the move left them, which from a pool record, and when a block adds
its tally to the statistics.  Round 8 changed the last (one barrier and the block's episode count instead of
__syncthreads_or) and tried another order for the first two -- every board's 32 bytes stored ahead of the wait for the pool
records, the boards that finished stored a second time behind it -- which lost on the clock (profiles/NOTES.md) and is not
in the tree.  These are the cases that order was written against, and whoever tries it again has them to pass: a store from
the record that does not happen (the finished board stays on the board it lost), one that happens for a board that goes on,
a board's words lost beside a finished one, a block whose tally is skipped or added twice.  They put a wave wholly into the
reset region, keep whole waves and blocks out of it, mix the two in one wave across a pool swap, and follow the observation
of the fused form through a reset -- all as equality with the C oracle (integer work on both sides,
tests/test_step_requests_gpu.py), on the smallest sizes that have a lone lane, a full wave, a wave and one board, and more
than one block at every boards-per-lane geometry.
"""
import numpy as np
import pytest

from test_step_requests_gpu import O_COLUMNS, O_PIECE, _assert_state_equal, _np, _state, make_actions, make_pool

pytestmark = pytest.mark.gpu

SHAPES = [(3, 10), (5, 20), (10, 40)]
SIZES = [1, 64, 65, 513]


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import tetris_piclim
    return tetris_piclim


def _pair(T, oracle, L, M, n, bpl, auto, pool, seed):
    gpu = T.BatchedTetris(L, M, n, seed=seed, auto_reset=auto)
    gpu.set_tuning(bpl)
    cpu = oracle.Env(n, L, M, 0, seed)
    cpu.set_options(auto_reset=auto, assign_mode=0)
    gpu.load_configs(*pool)
    cpu.set_pool(*pool)
    gpu.reset()
    cpu.reset()
    return gpu, cpu


def _lockstep(gpu, cpu, steps, action_of, ctx, t0=0):
    """`steps` steps side by side: reward, done and the packed state at every step.  Returns done, [steps, n]."""
    dones = []
    for t in range(t0, t0 + steps):
        a = action_of(t, cpu.get_state())
        _, r_g, d_g, _ = gpu.step(a, observe=False)
        r_c, d_c = cpu.step(a)
        assert np.array_equal(_np(r_g), r_c), f"{ctx}: reward at step {t}"
        assert np.array_equal(_np(d_g).astype(np.uint8), d_c), f"{ctx}: done at step {t}"
        _assert_state_equal(_state(gpu), cpu.get_state(), f"{ctx} step {t}")
        dones.append(d_c.copy())
    return np.stack(dones)


def _finish(gpu, cpu, ctx):
    assert gpu.stats() == cpu.stats(), ctx
    gpu.terminate()
    cpu.close()


def _geometries():
    return [(bpl, auto) for bpl in (1, 2, 4) for auto in (True, False)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_every_board_finishes_in_the_same_step(T, oracle, L, M, n):
    """A one-entry pool and one action everywhere: all boards are the same board, so both boards of every lane of every wave
    are stored from their record in the same step (and none in the steps between); every block adds its tally at once."""
    rows, pieces = oracle.synth_boards(5, 0, 1, L).copy(), oracle.synth_pieces(5, 0, 1, M).copy()
    for bpl, auto in _geometries():
        ctx = f"all finish: L={L} M={M} n={n} bpl={bpl} auto={auto}"
        gpu, cpu = _pair(T, oracle, L, M, n, bpl, auto, (rows, pieces), seed=31 + n)
        done = _lockstep(gpu, cpu, 2 * M + 3, lambda t, s: np.full(n, 13, np.uint8), ctx)     # the piece turned once, column 3
        assert done.all(axis=1).any(), f"{ctx}: no step in which every board finished"
        if auto:
            assert cpu.stats()["episodes"] >= 2 * n, ctx                  # an episode lasts M moves at the most
        _finish(gpu, cpu, ctx)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_no_board_finishes_for_several_steps(T, oracle, L, M, n):
    """Empty boards dealt squares and played in the order of O_COLUMNS live through all M moves: whole waves skip the reset
    region step after step, no block has a tally to add, and the state is what the moves left."""
    rows = np.zeros((7, 20), np.uint16)
    pieces = np.full((7, M + 1), O_PIECE, np.uint8)
    for bpl, auto in _geometries():
        ctx = f"none finish: L={L} M={M} n={n} bpl={bpl} auto={auto}"
        gpu, cpu = _pair(T, oracle, L, M, n, bpl, auto, (rows, pieces), seed=57 + n)
        done = _lockstep(gpu, cpu, M + 9, lambda t, s: O_COLUMNS[s["moves"] % len(O_COLUMNS)], ctx)
        quiet = ~done.any(axis=1)
        assert quiet[:8].all(), f"{ctx}: a board finished within the first eight steps"
        assert done[M - 1].all(), f"{ctx}: the M-th move ends every episode"
        _finish(gpu, cpu, ctx)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_pool_swap_in_mid_episode(T, oracle, L, M, n):
    """A second pool loaded after a few steps: boards that finish reset from the new buffer while boards that go on in the
    same wave refill their piece window from the old one; a third pool is refused until every episode of the first has
    ended, M + 1 steps later."""
    seed = 200 + n
    pools = [make_pool(oracle, 9, L, M, seed + 1), make_pool(oracle, 12, L, M, seed + 2), make_pool(oracle, 5, L, M, seed + 3)]
    for bpl in (1, 2, 4):
        ctx = f"swap: L={L} M={M} n={n} bpl={bpl}"
        gpu, cpu = _pair(T, oracle, L, M, n, bpl, True, pools[0], seed)
        play = lambda t, s: make_actions(oracle, n, t, seed, s["moves"])
        _lockstep(gpu, cpu, 4, play, ctx)
        gpu.load_configs(*pools[1]); cpu.set_pool(*pools[1])
        assert gpu.pool_info()["steps_until_swap"] == M + 1
        with pytest.raises(T.TplError, match="may still be running"):
            gpu.load_configs(*pools[2])
        done = _lockstep(gpu, cpu, M + 1, play, ctx, t0=4)
        if n >= 64:
            assert done.any() and not done.all(), ctx
        assert gpu.pool_info()["steps_until_swap"] == 0
        gpu.load_configs(*pools[2]); cpu.set_pool(*pools[2])
        _lockstep(gpu, cpu, 6, play, ctx, t0=M + 5)
        _finish(gpu, cpu, ctx)


@pytest.mark.parametrize("bpl", [1, 2, 4])
def test_without_a_pool_nothing_moves(T, bpl):
    """No pool loaded, auto-reset on: there is no record for a finished board to reset from (nor a record 0 for a lane's
    other board to read and drop), and the kernel is never launched -- the step is refused on the host, in every form, and
    boards, step clock and statistics stay as they were."""
    import torch
    L, M, n = 5, 20, 65
    env = T.BatchedTetris(L, M, n, seed=3, auto_reset=True)
    env.set_tuning(bpl)
    before = _state(env)
    a = torch.zeros(n, dtype=torch.uint8, device=env.device)
    for _ in range(2):
        with pytest.raises(T.TplError, match="auto_reset needs tpl_load_configs first"):
            env.step(a, observe=False)
        with pytest.raises(T.TplError, match="auto_reset needs tpl_load_configs first"):
            env.step(a, observe=True)
        with pytest.raises(T.TplError, match="auto_reset needs tpl_load_configs first"):
            env.move(a, a)
    after = _state(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert env.step_clock() == 0 and env.stats()["episodes"] == 0
    env.terminate()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("auto", [True, False])
def test_step_observe_into_shows_the_boards_after_their_reset(T, oracle, dtype, auto):
    """The fused form expands the observation from the registers the state was stored from: in a step where boards reset it
    is the observation of the NEW boards -- what observe() gives after step_into() on a twin environment."""
    import torch
    L, M, n, seed = 5, 20, 65, 77
    dt = getattr(torch, dtype)
    pool = make_pool(oracle, 9, L, M, seed + 1)
    fused, cpu = _pair(T, oracle, L, M, n, 1, auto, pool, seed)
    twin, cpu2 = _pair(T, oracle, L, M, n, 2, auto, pool, seed)
    dev = fused.device
    r1, r2 = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    d1, d2 = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    obs = torch.empty((n, 217), dtype=dt, device=dev)
    resets = 0
    for t in range(M + 5):
        a = make_actions(oracle, n, t, seed, cpu.get_state()["moves"])
        a_dev = torch.from_numpy(a).to(dev)
        fused.step_observe_into(a_dev, r1, d1, obs)
        twin.step_into(a_dev, r2, d2)
        r_c, d_c = cpu.step(a)
        assert np.array_equal(_np(r1), r_c) and np.array_equal(_np(d1), d_c), t
        assert torch.equal(r1, r2) and torch.equal(d1, d2), t
        _assert_state_equal(_state(fused), cpu.get_state(), f"fused {dtype} auto={auto} step {t}")
        assert torch.equal(obs.view(torch.int16 if dt is torch.bfloat16 else torch.int32),
                           twin.observe(dt).view(torch.int16 if dt is torch.bfloat16 else torch.int32)), t
        if dt is torch.float32:
            assert np.array_equal(_np(obs), cpu.expand_obs()), t
        resets += int(d_c.any() and not d_c.all())
    assert resets > 0, "no step in which some boards finished beside boards that went on"
    assert fused.stats() == cpu.stats() == twin.stats()
    fused.terminate(); twin.terminate(); cpu.close(); cpu2.close()


@pytest.mark.parametrize("form", ["move", "int32", "int64"])
def test_move_form_and_wide_actions(T, oracle, form):
    """The kernel's other template forms: rotation and column apart, and actions as 4- and 8-byte integers."""
    import torch
    L, M, n, seed = 5, 20, 65, 91
    pool = make_pool(oracle, 9, L, M, seed + 1)
    for bpl, auto in _geometries():
        ctx = f"{form}: bpl={bpl} auto={auto}"
        gpu, cpu = _pair(T, oracle, L, M, n, bpl, auto, pool, seed)
        finished = 0
        for t in range(M + 5):
            a = make_actions(oracle, n, t, seed, cpu.get_state()["moves"])
            if form == "move":
                r_g, d_g, c_g = gpu.move(a // 10, a % 10)
                r_c, d_c, c_c = cpu.move(a // 10, a % 10)
                assert np.array_equal(_np(c_g), c_c), f"{ctx}: cleared at step {t}"
            else:
                _, r_g, d_g, _ = gpu.step(torch.from_numpy(a.astype(form)).to(gpu.device), observe=False)
                r_c, d_c = cpu.step(a)
            assert np.array_equal(_np(r_g), r_c) and np.array_equal(_np(d_g).astype(np.uint8), d_c), f"{ctx}: step {t}"
            _assert_state_equal(_state(gpu), cpu.get_state(), f"{ctx} step {t}")
            finished += int(d_c.sum())
        assert finished > 0, ctx
        _finish(gpu, cpu, ctx)
