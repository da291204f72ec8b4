"""The step kernel's memory requests -- the state planes, the action row (a streaming load since round 7), the window-refill
gathers, the pool records of finished boards, the step clocks (two boards of a lane in one store since round 7) -- in lockstep
with the C oracle where those paths branch: every refill point and the M-th move (where a window refill and the end of the
episode fall on one step), partial waves and blocks, a lane's second board past the end, every boards-per-lane geometry,
auto-reset on and off, a small and a board-sized pool.  Round 7 also tried dropping the refill gather of a board that makes its
M-th move under auto-reset (profiles/NOTES.md): whoever tries again has the frozen-board test below to pass.  Everything is
integer work (the reward is one rounded multiply and at most one rounded add on both sides): equality.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(3, 10), (5, 20), (10, 40)]
SIZES = [1, 63, 64, 65, 511, 512, 513, 1537]


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import tetris_piclim
    return tetris_piclim


def _np(t):
    return t.cpu().numpy()


def _state(env):
    s = {k: _np(v) for k, v in env.packed_state().items()}
    s["rows"] = s["rows"].view(np.uint16)
    return s


def _assert_state_equal(got, want, ctx):
    for k in ("rows", "cur", "nxt", "lines", "moves", "state", "pieces_left"):
        assert np.array_equal(got[k], want[k]), f"{ctx}: {k} differs at {np.argwhere(got[k] != want[k])[:5].tolist()}"


O_PIECE = 6                                   # the 2 x 2 square
O_COLUMNS = np.array([0, 2, 4, 6, 0, 2, 4, 6, 8], np.uint8)


def make_pool(oracle, count, L, M, seed):
    """Entries 0, 3, 6, ...: an empty board that is dealt squares only (played in the order of O_COLUMNS it lives through all M
    moves: every refill point and the M-th move); entries 1, 4, ...: an empty board with synthetic pieces; the others the
    synthetic boards and pieces."""
    rows = oracle.synth_boards(seed, 0, count, L).copy()
    pieces = oracle.synth_pieces(seed, 0, count, M).copy()
    rows[0::3] = 0
    rows[1::3] = 0
    pieces[0::3] = O_PIECE
    return rows, pieces


def make_actions(oracle, n, t, seed, moves):
    """One board in three drops its piece unrotated in the column O_COLUMNS gives for its move count (four squares side by side,
    twice, then the one that clears two rows); one stacks unrotated pieces side by side, column by the step; one plays the
    synthetic random policy (top-outs at every age)."""
    a = oracle.synth_actions(seed, 0, n, t).copy()
    i = np.arange(n)
    a[i % 3 == 1] = ((i[i % 3 == 1] + 4 * t) % 10).astype(np.uint8)
    a[i % 3 == 0] = O_COLUMNS[moves[i % 3 == 0] % len(O_COLUMNS)]
    return a


def run_lockstep(T, oracle, L, M, n, bpl, auto, pool, seed, every_step=None):
    """3 M + 5 steps of the HIP environment and the oracle side by side; reward and done compared at every step, the packed
    state at every step too, the statistics at the end.  Returns the oracle's state history flags: (boards seen at
    moves == M, refill points seen)."""
    gpu = T.BatchedTetris(L, M, n, seed=seed, auto_reset=auto)
    gpu.set_tuning(bpl)
    rows, pieces = make_pool(oracle, pool, L, M, seed + 1)
    gpu.load_configs(rows, pieces)
    gpu.reset()
    cpu = oracle.Env(n, L, M, 0, seed)
    cpu.set_pool(rows, pieces)
    cpu.set_options(auto_reset=auto, assign_mode=0)
    cpu.reset()
    ctx = f"L={L} M={M} n={n} bpl={bpl} auto={auto} pool={pool}"
    mth_moves, refill_points = 0, set()
    for t in range(3 * M + 5):
        before = cpu.get_state()
        a = make_actions(oracle, n, t, seed, before["moves"])
        _, r_g, d_g, _ = gpu.step(a, observe=False)
        r_c, d_c = cpu.step(a)
        assert np.array_equal(_np(r_g), r_c), f"{ctx}: reward at step {t}"
        assert np.array_equal(_np(d_g).astype(np.uint8), d_c), f"{ctx}: done at step {t}"
        want = cpu.get_state()
        _assert_state_equal(_state(gpu), want, f"{ctx} step {t}")
        moving = before["state"] == 0
        mth_moves += int((moving & (before["moves"] + 1 == M)).sum())
        refill_points |= set(np.unique((before["moves"][moving] + 1)[(before["moves"][moving] + 1) % 10 == 0]).tolist())
        if every_step is not None:
            every_step(t, before, want)
    assert gpu.stats() == cpu.stats(), ctx
    gpu.terminate()
    cpu.close()
    return mth_moves, refill_points


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_lockstep_with_the_oracle_over_refill_points_mth_moves_and_geometries(T, oracle, L, M, n):
    mth, points = 0, set()
    for bpl in (1, 2, 4):
        for auto in (True, False):
            for pool in (7, n):
                m, p = run_lockstep(T, oracle, L, M, n, bpl, auto, pool, seed=100 + n)
                mth += m
                points |= p
    if n >= 63:        # the cases were really there: boards made their M-th move, windows ran out at every multiple of ten
        assert mth > 0, "no board made its M-th move"
        assert points == set(range(10, M + 1, 10)), points


@pytest.mark.parametrize("L,M", SHAPES)
def test_a_board_frozen_by_its_mth_move_shows_the_oracles_pieces(T, oracle, L, M):
    """Auto-reset off: the board that makes its M-th move freezes as the move left it, and packed_state() shows its piece
    window -- refilled when M is a multiple of ten: that gather may be dropped under auto-reset, never here."""
    n = 513
    frozen_at_M = [0]

    def watch(t, before, after):
        made = (before["state"] == 0) & (before["moves"] + 1 == M) & (after["moves"] == M)
        frozen_at_M[0] += int(made.sum())
        assert (after["state"][made] != 0).all()

    for bpl in (1, 2, 4):
        run_lockstep(T, oracle, L, M, n, bpl, False, n, seed=7, every_step=watch)     # cur / nxt compared at every step
    assert frozen_at_M[0] > 0
