"""The step kernel's record region: a board whose piece window runs out fetches its piece word behind the move, in the region
where the boards that finished fetch their pool records -- one hash per board, the refill word or the reset record, never both
(round 9).  The cases that arrangement can get wrong, as equality with the C oracle at every step (integer work on both sides,
tests/test_step_requests_gpu.py): every board of a wave refilling in one step; a lane whose one board refills while its other
resets; a board that finishes on the very move that runs its window out -- by a win, by the move limit, by a top-out -- which takes
the record's window with auto-reset and keeps the oracle's refilled one without; a refill from the pool buffer a board carries
while resets come from the one loaded since; both assignment modes, a pool of one entry and of a size that is no power of two, a
global offset; the kernel's move form, wide actions and the fused observation; a captured graph replayed across a refill step.

Shapes: M = 9 never refills, M = 10 refills on the last allowed move, 12 / 25 / 40 refill at 10 / 20 / 30 / 40.  Sizes: a lone
lane, a wave less one, a wave and one board, two blocks and one board, and -- at four boards per lane -- a block and one board.

The pool entries come in four kinds (entry index mod 4) and every board is played by its kind's script, keyed by its move count:
  0  an empty board dealt squares, played so that it lives through all M moves (no line at all when L < 10, else two lines per
     nine moves): a refill at every tenth move, the end at the move limit;
  1  L rows filled but for the last column, dealt bars: bars down that column, flat bars in between, so that the L-th line is
     cleared by move 10 (a win on the refill move);
  2  an empty board dealt bars: four flat ones, five upright in the last column, and the tenth tops out (on the refill move);
  3  a synthetic board and pieces under the synthetic random policy (ends at every age).
"""
import numpy as np
import pytest

from test_step_requests_gpu import O_COLUMNS, O_PIECE, _assert_state_equal, _np, _state

pytestmark = pytest.mark.gpu

SHAPES = [(2, 9), (2, 10), (3, 12), (4, 25), (10, 40)]
SIZES = [1, 63, 65, 513, 1025]
LANE_STRIDE = 256                       # threads per block: a lane's boards are this far apart (set_tuning's default)
I_PIECE = 0
FLAT, UPRIGHT = 0, 19                   # the bar unrotated in column 0; turned once in column 9
NO_LINE_COLUMNS = np.array([0, 2, 4, 6], np.uint8)
REWARD = (1.0, 0.5, -0.25)              # per line, win, loss: exact in binary, and the reward's fraction says how a board finished


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import tetris_piclim
    return tetris_piclim


def make_pool(oracle, count, L, M, seed):
    rows = oracle.synth_boards(seed, 0, count, L).copy()
    pieces = oracle.synth_pieces(seed, 0, count, M).copy()
    kind = np.arange(count) % 4
    rows[kind != 3] = 0
    rows[kind == 1, 20 - L:] = 0x1FF                        # (row 19 is the floor)
    pieces[kind == 0] = O_PIECE
    pieces[(kind == 1) | (kind == 2)] = I_PIECE
    return rows, pieces


def scripted_actions(oracle, L, kind, moves, t, seed):
    """The action of every board for its next move (its move count is `moves`), by the kind of the pool entry it holds."""
    n = len(kind)
    a = oracle.synth_actions(seed, 0, n, t).copy()
    m = moves.astype(np.int64)
    columns = O_COLUMNS if L >= 10 else NO_LINE_COLUMNS
    a[kind == 0] = columns[m[kind == 0] % len(columns)]
    upright_first = (L + 3) // 4 - 1                        # four lines each, until at most four are left for move 10
    a[kind == 1] = np.where((m[kind == 1] < upright_first) | (m[kind == 1] == 9), UPRIGHT, FLAT)
    a[kind == 2] = np.where(m[kind == 2] < 4, FLAT, UPRIGHT)
    return a


class Twin:
    """The HIP environment and the oracle side by side, with the kind of the pool entry every board holds (entry mod 4: a new
    episode takes its entry from the current pool, at the step the oracle names)."""

    def __init__(self, T, oracle, L, M, n, bpl, auto, pool, seed, assign="hash", offset=0):
        self.oracle, self.L, self.M, self.n, self.seed = oracle, L, M, n, seed
        self.gpu = T.BatchedTetris(L, M, n, seed=seed, global_offset=offset, auto_reset=auto, assign=assign, reward=REWARD)
        self.gpu.set_tuning(bpl)
        self.cpu = oracle.Env(n, L, M, offset, seed)
        self.cpu.set_options(auto_reset=auto, assign_mode={"hash": 0, "sequential": 1}[assign], per_line=REWARD[0], win=REWARD[1],
                             lose=REWARD[2])
        self.gpu.load_configs(*pool)
        self.cpu.set_pool(*pool)
        self.gpu.reset()
        self.cpu.reset()
        self.auto = auto
        self.kind = np.array([self.cpu.assign(b, 0) % 4 for b in range(n)])
        self.t = 0
        self.seen = dict(refill_points=set(), all_refill=0, refill_and_finish=0, refill_beside_reset=0, wins_on_refill=0,
                         topouts_on_refill=0, limit_on_refill=0, carried_refills=0)
        self.swapped_at = None

    def swap(self, pool):
        self.gpu.load_configs(*pool)
        self.cpu.set_pool(*pool)
        self.swapped_at = self.t

    def next_actions(self):
        self.before = self.cpu.get_state()
        return scripted_actions(self.oracle, self.L, self.kind, self.before["moves"], self.t, self.seed)

    def oracle_step(self, a, move_form=False):
        """The oracle's step, and what the step exercised; returns what the HIP side has to show."""
        before = self.before
        born = np.array([self.cpu.birth(b) for b in range(self.n)]) if self.swapped_at is not None else None
        topouts_now = -self.cpu.stats()["topouts"]
        out = self.cpu.move(a // 10, a % 10) if move_form else self.cpu.step(a)
        topouts_now += self.cpu.stats()["topouts"]
        moving = before["state"] == 0
        done = out[1].astype(bool) & moving                             # finished in this step (a frozen board reports done too)
        move_no = before["moves"].astype(np.int64) + 1
        runs_out = moving & (move_no % 10 == 0)
        won = done & (out[0] % 1.0 == 0.5)
        lost = done & (out[0] % 1.0 == 0.75)
        seen = self.seen
        seen["refill_points"] |= set(np.unique(move_no[runs_out]).tolist())
        seen["all_refill"] += int(runs_out.all())
        seen["refill_and_finish"] += int((runs_out & done).sum())
        seen["wins_on_refill"] += int((runs_out & won).sum())
        # a loss is a top-out unless it is the M-th move; that one can be either, and the oracle's count of top-outs says which
        # (a board on its M-th move runs its window out exactly when M is a multiple of ten)
        topouts = int((runs_out & lost).sum()) if self.M % 10 else topouts_now - int((lost & ~runs_out).sum())
        seen["topouts_on_refill"] += topouts
        seen["limit_on_refill"] += int((runs_out & lost).sum()) - topouts
        goes_on = runs_out & ~done
        if self.n > LANE_STRIDE:
            seen["refill_beside_reset"] += int((goes_on[:-LANE_STRIDE] & done[LANE_STRIDE:]).sum() +
                                               (done[:-LANE_STRIDE] & goes_on[LANE_STRIDE:]).sum())
        if born is not None:
            seen["carried_refills"] += int((goes_on & (born < self.swapped_at)).sum())
        if self.auto:
            for b in np.flatnonzero(done):
                self.kind[b] = self.cpu.assign(int(b), self.cpu.birth(int(b))) % 4
        self.t += 1
        return out

    def check(self, got, want, ctx):
        for g, w, name in zip(got, want, ("reward", "done", "cleared")):
            assert np.array_equal(_np(g).astype(w.dtype), w), f"{ctx}: {name} at step {self.t - 1}"
        _assert_state_equal(_state(self.gpu), self.cpu.get_state(), f"{ctx} step {self.t - 1}")

    def lockstep(self, steps, ctx):
        for _ in range(steps):
            a = self.next_actions()
            _, r, d, _ = self.gpu.step(a, observe=False)
            self.check((r, d), self.oracle_step(a), ctx)

    def finish(self, ctx):
        assert self.gpu.stats() == self.cpu.stats(), ctx
        assert self.gpu.step_clock() == self.cpu.clock == self.t, ctx
        self.gpu.terminate()
        self.cpu.close()
        return self.seen


def _geometries():
    return [(bpl, auto) for bpl in (1, 2, 4) for auto in (True, False)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_every_board_refills_in_the_same_step(T, oracle, L, M, n):
    """A pool of one entry (kind 0) and one script: all boards are the same board, so both boards of every lane of every wave
    fetch a piece word in the same step, and when M is a multiple of ten all of them finish on a refill move, at the move
    limit: with auto-reset every lane's need turns from the word to the record, without it the word is kept."""
    pool = make_pool(oracle, 1, L, M, 5)
    for bpl, auto in _geometries():
        ctx = f"all refill: L={L} M={M} n={n} bpl={bpl} auto={auto}"
        twin = Twin(T, oracle, L, M, n, bpl, auto, pool, seed=31 + n)
        twin.lockstep(M + 12, ctx)
        seen = twin.finish(ctx)
        assert seen["refill_points"] == set(range(10, M + 1, 10)), f"{ctx}: {seen}"
        assert seen["all_refill"] >= M // 10, f"{ctx}: {seen}"
        if M % 10 == 0:
            assert seen["limit_on_refill"] >= n, f"{ctx}: {seen}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_refills_beside_resets_and_ends_on_the_refill_move(T, oracle, L, M, n):
    """The four kinds in one pool of twelve: at the tenth step boards that go on with a new window sit beside boards that win
    and boards that top out on that move -- in one wave, and in one lane where a lane has several boards."""
    pool = make_pool(oracle, 12, L, M, 9)
    for bpl, auto in _geometries():
        ctx = f"mixed: L={L} M={M} n={n} bpl={bpl} auto={auto}"
        twin = Twin(T, oracle, L, M, n, bpl, auto, pool, seed=100 + n)
        twin.lockstep(M + 12, ctx)
        seen = twin.finish(ctx)
        if M >= 10 and n >= 63:
            assert seen["wins_on_refill"] > 0 and seen["topouts_on_refill"] > 0, f"{ctx}: {seen}"
            assert seen["refill_points"] == set(range(10, M + 1, 10)), f"{ctx}: {seen}"
        if M > 10 and n > 2 * LANE_STRIDE:
            assert seen["refill_beside_reset"] > 0, f"{ctx}: {seen}"
        if M < 10:
            assert not seen["refill_points"], f"{ctx}: {seen}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_refill_from_the_carried_pool_after_a_swap(T, oracle, L, M, n):
    """A second pool, of another size, loaded after four steps: the boards that go on refill from the buffer they carry, with
    its size in their hash, while the boards that finish in the same step take records of the new one."""
    seed = 200 + n
    pools = [make_pool(oracle, 12, L, M, seed + 1), make_pool(oracle, 7, L, M, seed + 2)]
    for bpl in (1, 2, 4):
        ctx = f"swap: L={L} M={M} n={n} bpl={bpl}"
        twin = Twin(T, oracle, L, M, n, bpl, True, pools[0], seed)
        twin.lockstep(4, ctx)
        twin.swap(pools[1])
        twin.lockstep(M + 8, ctx)
        seen = twin.finish(ctx)
        if M > 10 and n >= 63:
            assert seen["carried_refills"] > 0, f"{ctx}: {seen}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_assignment_modes_pool_sizes_and_global_offset(T, oracle, L, M, n):
    """What goes into the one hash: sequential assignment, a pool of one entry, of five and of twelve, and a global offset beyond
    32 bits -- for the word (birth = clock - moves) and the record (birth = clock + 1) alike."""
    for assign, offset, count, auto in (("sequential", 0, 5, True), ("hash", (1 << 33) + 12345, 1, True),
                                        ("sequential", 77, 12, True), ("hash", 1000003, 7, False)):
        pool = make_pool(oracle, count, L, M, 17 + count)
        for bpl in (1, 2, 4):
            ctx = f"{assign} offset={offset} pool={count}: L={L} M={M} n={n} bpl={bpl} auto={auto}"
            twin = Twin(T, oracle, L, M, n, bpl, auto, pool, 300 + n, assign=assign, offset=offset)
            twin.lockstep(M + 12, ctx)
            seen = twin.finish(ctx)
            if n >= 63 or count == 1:                       # (a lone board shows what its one kind reaches)
                assert seen["refill_points"] == set(range(10, M + 1, 10)), f"{ctx}: {seen}"


@pytest.mark.parametrize("form", ["move", "int32", "int64"])
@pytest.mark.parametrize("L,M", SHAPES)
def test_move_form_and_wide_actions(T, oracle, L, M, form):
    """The kernel's other template forms: rotation and column apart (with the rows cleared), 4- and 8-byte actions."""
    import torch
    pool = make_pool(oracle, 12, L, M, 23)
    for n in (65, 1025):
        for bpl, auto in _geometries():
            ctx = f"{form}: L={L} M={M} n={n} bpl={bpl} auto={auto}"
            twin = Twin(T, oracle, L, M, n, bpl, auto, pool, seed=91 + n)
            for _ in range(M + 12):
                a = twin.next_actions()
                if form == "move":
                    got = twin.gpu.move(a // 10, a % 10)
                else:
                    _, r, d, _ = twin.gpu.step(torch.from_numpy(a.astype(form)).to(twin.gpu.device), observe=False)
                    got = (r, d)
                twin.check(got, twin.oracle_step(a, move_form=form == "move"), ctx)
            seen = twin.finish(ctx)
            assert seen["refill_points"] == set(range(10, M + 1, 10)), f"{ctx}: {seen}"
            if M >= 10:
                assert seen["refill_and_finish"] > 0, f"{ctx}: {seen}"


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("L,M", SHAPES)
def test_step_observe_into_shows_the_refilled_window(T, oracle, L, M, auto, dtype):
    """The fused form expands the observation from the registers the state is stored from, behind the record region: it shows the
    patched window of a board that refilled and the new board of one that reset -- what observe() gives after step_into() on
    a twin environment with two boards per lane, and the oracle's expansion."""
    import torch
    dt = getattr(torch, dtype)
    bits = torch.int16 if dt is torch.bfloat16 else torch.int32
    pool = make_pool(oracle, 12, L, M, 29)
    for n in (65, 513):
        ctx = f"fused {dtype}: L={L} M={M} n={n} auto={auto}"
        fused = Twin(T, oracle, L, M, n, 1, auto, pool, seed=77 + n)
        other = T.BatchedTetris(L, M, n, seed=77 + n, auto_reset=auto, reward=REWARD)
        other.load_configs(*pool)
        other.reset()
        dev = fused.gpu.device
        r1, r2 = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        d1, d2 = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
        obs = torch.empty((n, 217), dtype=dt, device=dev)
        for _ in range(M + 12):
            a = fused.next_actions()
            a_dev = torch.from_numpy(a).to(dev)
            fused.gpu.step_observe_into(a_dev, r1, d1, obs)
            other.step_into(a_dev, r2, d2)
            fused.check((r1, d1), fused.oracle_step(a), ctx)
            assert torch.equal(r1, r2) and torch.equal(d1, d2), f"{ctx}: step {fused.t - 1}"
            assert torch.equal(obs.view(bits), other.observe(dt).view(bits)), f"{ctx}: observation at step {fused.t - 1}"
            if dt is torch.float32:
                assert np.array_equal(_np(obs), fused.cpu.expand_obs()), f"{ctx}: observation at step {fused.t - 1}"
        assert other.stats() == fused.cpu.stats(), ctx
        other.terminate()
        seen = fused.finish(ctx)
        assert seen["refill_points"] == set(range(10, M + 1, 10)), f"{ctx}: {seen}"


@pytest.mark.parametrize("L,M", SHAPES)
def test_capture_steps_replays_across_refill_steps(T, oracle, L, M):
    """Four steps in one HIP graph, replayed until every refill point and the M-th move are behind: the tenth step sits inside
    the third replay, between steps that refill nothing."""
    import torch
    K = 4
    pool = make_pool(oracle, 12, L, M, 37)
    for n, bpl in ((65, 1), (513, 2), (1025, 4)):
        ctx = f"graph: L={L} M={M} n={n} bpl={bpl}"
        twin = Twin(T, oracle, L, M, n, bpl, True, pool, seed=41 + n)
        dev = twin.gpu.device
        actions = torch.empty((K, n), dtype=torch.uint8, device=dev)
        rewards = torch.empty((K, n), dtype=torch.float32, device=dev)
        dones = torch.empty((K, n), dtype=torch.uint8, device=dev)
        replay = twin.gpu.capture_steps(actions, rewards, dones)
        for block in range((M + 12 + K - 1) // K):
            want = []
            for k in range(K):                              # the scripts read the boards' move counts: the oracle goes first
                a = twin.next_actions()
                actions[k].copy_(torch.from_numpy(a))
                want.append(twin.oracle_step(a))
            replay()
            for k in range(K):
                assert np.array_equal(_np(rewards[k]), want[k][0]) and np.array_equal(_np(dones[k]), want[k][1]), f"{ctx}: step {K * block + k}"
            _assert_state_equal(_state(twin.gpu), twin.cpu.get_state(), f"{ctx} block {block}")
        seen = twin.finish(ctx)
        assert seen["refill_points"] == set(range(10, M + 1, 10)), f"{ctx}: {seen}"
        if M >= 10:
            assert seen["refill_and_finish"] > 0, f"{ctx}: {seen}"
