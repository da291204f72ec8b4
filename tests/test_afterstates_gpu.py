"""Afterstate enumeration and the one-ply lookahead policy on one MI355X (include/tpl_learn.h's rule, tpl_afterstates,
lookahead.afterstates / LookaheadPolicy, DQNLearner.evaluate(lookahead=True)):

  * the kernel against the C oracle: for every board and all 40 actions, oracle.Game.move on the decoded board is the decoded
    afterstate -- rows, lines, moves, state, cleared, done, the reward bit for bit, canonical, the window shifted by one entry,
    the slot and spare bits carried over -- over start positions, prepared wells (1- to 4-line and split clears), counters one
    short of L and M, tall boards, finished boards and dense random boards; canaries around all six outputs, each optional
    output left out once;
  * the kernel against the step kernel: the step of a non-auto-reset environment with a pool, action by action, leaves the
    enumeration's planes, reward and done, except window entries 2..11 on the refill move;
  * zero copy into a scratch environment, the policy without a network (the best distinct reward) and with one (the chosen
    action's float64 score is the best within the float32 roundings of the score);
  * the learner's evaluate(lookahead=True), and that the default evaluate() is untouched by it.
"""
import copy

import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from conftest import load_golden
from test_gpu_parity import _dense_boards
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _env, _model, _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, M = 10, 40
POOL = 1639
SIZES = [1, 2, 8, 13, 64, 65, 1639]
REWARDS = [(1.0, 0.0, 0.0), (0.1, 0.5, -0.25)]
FULL = 0x3FF


def _m():
    return T._learn_lib


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32))


# ------------------------------------------------------------------------------------------------ the boards
def _ragged(gen, lo, hi):
    rows = np.zeros(20, np.uint16)
    for x, h in enumerate(gen.integers(lo, hi, 10)):
        for k in range(int(h)):
            if k == int(h) - 1 or gen.random() > 0.2:
                rows[19 - k] |= np.uint16(1 << x)
    return rows


def _well(gen, k, split):
    """k rows (1..4) full but for one column at the bottom; split: one of the inner rows gets a second hole, so the upright I
    in the well clears rows that are not neighbours."""
    well = int(gen.integers(0, 10))
    rows = np.zeros(20, np.uint16)
    rows[20 - k:] = np.uint16(FULL & ~(1 << well))
    if split and k >= 3:
        rows[19 - int(gen.integers(1, k - 1))] &= np.uint16(~(1 << ((well + 1 + int(gen.integers(0, 9))) % 10)) & FULL)
    return rows, well


def _pool_fields(gen):
    """POOL states, kind by index mod 8: 0 the start positions of edges.npz, 1 prepared wells under the I, 2 counters one short
    of L and / or M (on wells and ragged boards), 3 moves in {8, 9, 18, 19}, 4 tall boards, 5 finished boards (states 1, 2, 3),
    6 and 7 dense random boards.  Every state has all 36 window bits random behind its current piece, a random slot bit and a
    random spare bit."""
    edges = load_golden("edges.npz")
    n_edges = int(edges["n"])
    dense = _dense_boards(gen, POOL)
    rows = np.zeros((POOL, 20), np.uint16)
    cur = gen.integers(0, 7, POOL)
    lines, moves, state = gen.integers(0, L - 1, POOL), gen.integers(0, M - 1, POOL), np.zeros(POOL, np.int64)
    for i in range(POOL):
        kind, k = i % 8, i // 8
        if kind == 0:
            c = k % n_edges
            rows[i] = edges[f"c{c}_rows0"]
            lines[i], moves[i] = min(int(edges[f"c{c}_lines0"]), L - 1), min(int(edges[f"c{c}_moves0"]), M - 1)
            if k < n_edges:
                cur[i] = int(edges[f"c{c}_pieces"][0])
        elif kind == 1:
            rows[i], _ = _well(gen, 1 + k % 4, split=k % 8 >= 4)
            cur[i] = 0
        elif kind == 2:
            if k % 2:
                rows[i], _ = _well(gen, 1 + (k // 2) % 4, split=False)
                cur[i] = 0
            else:
                rows[i] = _ragged(gen, 0, 10)
            lines[i], moves[i] = ((L - 1, 3), (2, M - 1), (L - 1, M - 1))[k % 3]
        elif kind == 3:
            rows[i] = _ragged(gen, 0, 13)
            moves[i] = (8, 9, 18, 19)[k % 4]
        elif kind == 4:
            rows[i] = _ragged(gen, 14 + k % 4, 21)
        elif kind == 5:
            rows[i] = dense[i]
            state[i] = 1 + k % 3
        else:
            rows[i] = dense[i]
        if i < 56:
            cur[i] = cur[i] if kind in (1, 2) else (i // 8) % 7
    window = (gen.integers(0, 1 << 36, POOL, dtype=np.int64).astype(np.uint64) & ~np.uint64(7)) | cur.astype(np.uint64)
    return dict(rows=rows, lines=lines, moves=moves, state=state, slot=gen.integers(0, 2, POOL), window=window,
                spare=gen.integers(0, 2, POOL).astype(np.uint32))


class Pool:
    """The states, their planes and -- computed once -- what the oracle says of all 40 actions of every running one."""

    def __init__(self, oracle, fields=None, L=L, M=M):
        """Without `fields`: the POOL states of _pool_fields at L = 10 / M = 40 and their coverage condition; with them: those states
        played at the game (L, M), the coverage left to the caller."""
        own = fields is None
        f = self.fields = _pool_fields(np.random.default_rng(1639)) if own else fields
        self.A, self.B = R.pack_state(f["rows"], f["lines"], f["moves"], f["state"], f["slot"], f["window"])
        self.B[:, 1] |= f["spare"] << np.uint32(31)
        back = R.decode_state(self.A, self.B)
        for k in ("rows", "lines", "moves", "state", "slot", "window"):
            assert np.array_equal(back[k].astype(np.int64), np.asarray(f[k]).astype(np.int64)), k
        n = self.n = self.A.shape[0]
        self.rows = np.zeros((n, 40, 20), np.uint16)
        self.lines, self.moves = np.zeros((n, 40), np.int64), np.zeros((n, 40), np.int64)
        self.state, self.ret = np.zeros((n, 40), np.int64), np.zeros((n, 40), np.int64)
        cur = (f["window"] & np.uint64(7)).astype(np.int64)
        for i in range(n):
            if f["state"][i] != 0:                             # frozen: the oracle is not asked
                self.rows[i], self.lines[i], self.moves[i], self.state[i] = f["rows"][i], f["lines"][i], f["moves"][i], -1
                continue
            for a in range(40):
                g = oracle.Game(L, M, rows=f["rows"][i], pieces=[cur[i]], lines_cleared=int(f["lines"][i]),
                                moves_used=int(f["moves"][i]))
                self.ret[i, a] = g.move(a // 10, a % 10)
                self.rows[i, a], self.lines[i, a], self.moves[i, a], self.state[i, a] = g.rows, g.lines_cleared, g.moves_used, g.state
        run = np.asarray(f["state"]) == 0
        self.running = run
        self.topout = (self.ret < 0) & run[:, None]
        self.cleared = np.where(run[:, None], np.maximum(self.ret, 0), 0)
        self.won = (self.state == 1) & run[:, None]
        self.limit = (self.state == 2) & ~self.topout & run[:, None]
        self.done = np.where(run[:, None], self.state != 0, True)
        if not own:
            return
        # the coverage condition, on the oracle's own outcomes
        seen = {k: int(((self.cleared == k) & run[:, None]).sum()) for k in range(5)}
        ends = dict(win=int(self.won.sum()), limit=int(self.limit.sum()), topout=int(self.topout.sum()), frozen=int((~run).sum()),
                    win_at_the_limit=int((self.won & (self.moves >= M)).sum()))
        print(f"oracle outcomes over {n} x 40: cleared {seen}, {ends}")
        assert min(seen.values()) > 0 and min(ends.values()) > 0, (seen, ends)
        assert set(cur[run].tolist()) == set(range(7)) and {1, 2, 3} <= set(np.asarray(f["state"]).tolist())
        assert {8, 9, 18, 19} <= set(np.asarray(f["moves"])[run].tolist())

    def take(self, n, offset):
        return (offset + np.arange(n)) % self.n

    def reward(self, idx, params):
        """float32 [n, 40]: one rounded multiply, at most one rounded add (numpy float32 operations round once each)."""
        r_line, r_win, r_lose = (np.float32(x) for x in params)
        r = r_line * self.cleared[idx].astype(np.float32)
        r = np.where(self.won[idx], r + r_win, r)
        r = np.where(self.limit[idx] | self.topout[idx], r + r_lose, r)
        return np.where(self.running[idx][:, None], r, np.float32(0.0)).astype(np.float32)


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def _run(A, B, params, skip=(), L=L, M=M):
    """tpl_afterstates of host planes at the game (L, M) through canary-framed buffers; `skip` names the outputs passed as NULL
    ("states" = both planes).  Returns host arrays of the outputs given."""
    n = A.shape[0]
    a, b = Framed(n * 16, 1), Framed(n * 16, 2)
    a.inner().copy_(torch.from_numpy(A.view(np.uint8).reshape(-1)))
    b.inner().copy_(torch.from_numpy(B.view(np.uint8).reshape(-1)))
    out = dict(out_a=Framed(n * 640, 3), out_b=Framed(n * 640, 4), reward=Framed(n * 160, 5), done=Framed(n * 40, 6),
               cleared=Framed(n * 40, 7), canonical=Framed(n * 40, 8))
    for f in out.values():
        f.inner().fill_(0xCD)
    given = {k: f for k, f in out.items() if k not in skip and not (k in ("out_a", "out_b") and "states" in skip)}
    p = lambda k: given[k].ptr() if k in given else None
    _check(_lib().tpl_afterstates(a.ptr(), b.ptr(), n, L, M, *params, p("out_a"), p("out_b"), p("reward"), p("done"), p("cleared"),
                                  p("canonical"), _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b)]:
        f.assert_canary((n, params, skip, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    for k, f in out.items():                                   # an output that was not given is not written
        if k not in given:
            assert (f.host() == 0xCD).all(), (skip, k)
    host = {k: f.host() for k, f in given.items()}
    for k in ("out_a", "out_b"):
        if k in host:
            host[k] = host[k].view(np.uint32).reshape(n, 40, 4)
    if "reward" in host:
        host["reward"] = host["reward"].view(np.float32).reshape(n, 40)
    for k in ("done", "cleared", "canonical"):
        if k in host:
            host[k] = host[k].reshape(n, 40)
    return host


def _assert_against_the_oracle(pool, idx, got, params, what):
    n = idx.size
    f = pool.fields
    if "out_a" in got:
        d = R.decode_state(got["out_a"].reshape(-1, 4), got["out_b"].reshape(-1, 4))
        d = {k: v.reshape(n, 40, *v.shape[1:]) for k, v in d.items()}
        run = pool.running[idx]
        assert np.array_equal(d["rows"][run], pool.rows[idx][run]), what
        assert np.array_equal(d["lines"][run], pool.lines[idx][run]) and np.array_equal(d["moves"][run], pool.moves[idx][run]), what
        state = d["state"].astype(np.int64)
        assert np.array_equal(np.where(state == 3, 2, state)[run], pool.state[idx][run]), what
        assert np.array_equal((state == 3)[run], pool.topout[idx][run]), what
        window = f["window"][idx]
        assert np.array_equal(d["window"][run], np.broadcast_to((window >> np.uint64(3))[:, None], (n, 40))[run]), what
        assert np.array_equal(d["slot"], np.broadcast_to(np.asarray(f["slot"])[idx][:, None], (n, 40))), what
        assert np.array_equal(got["out_b"][:, :, 1] >> np.uint32(31), np.broadcast_to(f["spare"][idx][:, None], (n, 40))), what
        # a finished board: all 40 afterstates are the state itself, bit for bit
        assert np.array_equal(got["out_a"][~run], np.broadcast_to(pool.A[idx][:, None], (n, 40, 4))[~run]), what
        assert np.array_equal(got["out_b"][~run], np.broadcast_to(pool.B[idx][:, None], (n, 40, 4))[~run]), what
    if "cleared" in got:
        assert np.array_equal(got["cleared"], pool.cleared[idx]), what
    if "done" in got:
        assert np.array_equal(got["done"], pool.done[idx].astype(np.uint8)), what
    if "reward" in got:
        assert np.array_equal(got["reward"].view(np.uint32), pool.reward(idx, params).view(np.uint32)), what
    if "canonical" in got:
        cur = (f["window"][idx] & np.uint64(7)).astype(np.int64)
        assert np.array_equal(got["canonical"], _m().canonical_actions(cur[:, None], np.arange(40)[None, :])), what


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("n", SIZES)
def test_the_kernel_is_the_oracle_move_for_every_board_and_action(pool, n):
    idx = pool.take(n, 0 if n == POOL else 7 * n)
    A, B = np.ascontiguousarray(pool.A[idx]), np.ascontiguousarray(pool.B[idx])
    full = {}
    for params in REWARDS:
        full[params] = _run(A, B, params)
        assert set(full[params]) == {"out_a", "out_b", "reward", "done", "cleared", "canonical"}
        _assert_against_the_oracle(pool, idx, full[params], params, (n, params))
    assert np.array_equal(full[REWARDS[0]]["out_a"], full[REWARDS[1]]["out_a"])
    if n == POOL:                                              # 0.1 * 3 + x: the rounding that a fused multiply-add changes
        r = full[REWARDS[1]]["reward"]
        assert (r[pool.cleared == 3] == np.float32(np.float32(0.1) * np.float32(3.0))).any()
    # each optional output left out once (the form without state planes among them): the others are unchanged
    params = REWARDS[1]
    for skip in ("states", "reward", "done", "cleared", "canonical"):
        got = _run(A, B, params, skip=(skip,))
        assert set(got) == set(full[params]) - ({"out_a", "out_b"} if skip == "states" else {skip})
        for k, v in got.items():
            assert np.array_equal(v.view(np.uint8), full[params][k].view(np.uint8)), (n, skip, k)
    got = _run(A, B, params, skip=("states", "reward", "done", "cleared"))          # one output alone
    assert np.array_equal(got["canonical"], full[params]["canonical"])


# ------------------------------------------------------------------------------------------------ 2. against the step
def test_the_kernel_is_the_step_kernel_action_by_action(pool):
    n, params = 65, REWARDS[1]
    env = T.BatchedTetris(L, M, n, device=DEV, seed=5, auto_reset=False, reward=params)
    gen = np.random.default_rng(65)
    env.load_configs(np.zeros((128, 20), np.uint16), gen.integers(0, 7, (128, M + 1)).astype(np.uint8))    # empty boards: all last
    slot = env.pool_info()["current_slot"]
    env.reset()
    spread = torch.tensor([0, 3, 6, 1, 4, 7, 2, 5, 8, 9], dtype=torch.uint8, device=DEV)    # flat pieces side by side: boards last
    refills = 0
    for clock in range(1, 20):
        env.step(spread[clock % 10].repeat(n), observe=False)
        if clock not in (9, 19):
            continue
        # the boards that are still running keep their counters and their window (it is the pool's: the refill at this move
        # continues it) and get mid-game rows and lines; the others become written mid-game states off the refill move
        a, b = (_np(x).view(np.uint32) for x in env.raw_planes())
        nat = R.decode_state(a, b)
        alive = (nat["state"] == 0) & (nat["moves"] == clock)
        assert alive.sum() >= 8, (clock, int(alive.sum()))
        idx = pool.take(n, 100 * clock)
        f = {k: np.asarray(v)[idx].copy() for k, v in pool.fields.items()}
        f["moves"] = np.where(f["moves"] % 10 == 9, f["moves"] - 1, f["moves"])
        for k in ("moves", "window"):
            f[k] = np.where(alive, nat[k], f[k])
        f["state"] = np.where(alive, 0, f["state"])
        f["lines"] = np.where(alive & (gen.random(n) < 0.3), L - 1, np.minimum(f["lines"], L - 1))
        A, B = R.pack_state(f["rows"], f["lines"], f["moves"], f["state"], slot, f["window"])
        env.write_raw_planes(_i32(A), _i32(B))
        saved = env.snapshot()
        want = T.afterstates(env)
        wa, wb = _np(want["states_a"]).view(np.uint32), _np(want["states_b"]).view(np.uint32)
        explicit = T.afterstates(env, _i32(A).to(DEV), _i32(B).to(DEV))
        for k, v in want.items():
            assert torch.equal(v, explicit[k]), k
        before = R.decode_state(A, B)
        refill = (before["state"] == 0) & ((before["moves"].astype(np.int64) + 1) % 10 == 0)
        assert np.array_equal(refill, alive)
        refills += int(refill.sum())
        mask_w = np.where(refill, np.uint32(0x3F), np.uint32(0xFFFFFFFF))          # entries 0 and 1 of B.w stay compared
        mask_z = np.where(refill, np.uint32(0x0FFFFFFF), np.uint32(0xFFFFFFFF))
        differs = 0
        for action in range(40):
            env.restore(saved)
            _, reward, done, _ = env.step(torch.full((n,), action, dtype=torch.uint8, device=DEV), observe=False)
            ga, gb = (_np(x).view(np.uint32) for x in env.raw_planes())
            what = (clock, action)
            assert np.array_equal(ga, wa[:, action]), what
            assert np.array_equal(gb[:, :2], wb[:, action, :2]), what
            assert np.array_equal(gb[:, 2] & mask_z, wb[:, action, 2] & mask_z), what
            assert np.array_equal(gb[:, 3] & mask_w, wb[:, action, 3] & mask_w), what
            assert np.array_equal(_np(reward).view(np.uint32), _np(want["reward"])[:, action].view(np.uint32)), what
            assert np.array_equal(_np(done).astype(np.uint8), _np(want["done"])[:, action]), what
            differs += int((gb[:, 3] != wb[:, action, 3])[refill].sum())
        assert differs > 0                                     # the exception is real: the step refilled, the enumeration did not
        env.restore(saved)
        a2, b2 = (_np(x).view(np.uint32) for x in env.raw_planes())
        assert np.array_equal(a2, A) and np.array_equal(b2, B)
        # play on from the environment's own boards: put back what was there before the rows were written
        env.write_raw_planes(_i32(a), _i32(b))
    assert refills >= 16
    env.terminate()


# ------------------------------------------------------------------------------------------------ 3. zero copy, the policy
def _resident(pool, n, offset, params, L=L, M=M):
    env = T.BatchedTetris(L, M, n, device=DEV, seed=9, reward=params)
    idx = pool.take(n, offset)
    env.write_raw_planes(_i32(pool.A[idx]), _i32(pool.B[idx]))
    return env, idx


def test_zero_copy_into_a_scratch_environment(pool):
    n = 300
    env, idx = _resident(pool, n, 11, REWARDS[1])
    plain = T.afterstates(env)
    assert plain["states_a"].shape == (n, 40, 4) and plain["states_a"].dtype == torch.int32
    assert plain["reward"].shape == (n, 40) and plain["reward"].dtype == torch.float32
    for k in ("done", "cleared", "canonical"):
        assert plain[k].shape == (n, 40) and plain[k].dtype == torch.uint8
    host = dict(out_a=_np(plain["states_a"]).view(np.uint32), out_b=_np(plain["states_b"]).view(np.uint32),
                reward=_np(plain["reward"]), done=_np(plain["done"]), cleared=_np(plain["cleared"]), canonical=_np(plain["canonical"]))
    _assert_against_the_oracle(pool, idx, host, REWARDS[1], "resident")
    scratch = T.BatchedTetris(L, M, 40 * n, device=DEV, seed=9)
    into = T.afterstates(env, into=scratch)
    assert set(into) == {"reward", "done", "cleared", "canonical"}
    sa, sb = scratch.raw_planes()
    assert torch.equal(sa, plain["states_a"].view(-1, 4)) and torch.equal(sb, plain["states_b"].view(-1, 4))
    for k in into:
        assert torch.equal(into[k], plain[k]), k
    bare = T.afterstates(env, with_states=False)
    assert set(bare) == set(into) and all(torch.equal(bare[k], plain[k]) for k in bare)
    a, b = env.raw_planes()                                    # the position itself is left alone
    assert np.array_equal(_np(a).view(np.uint32), pool.A[idx]) and np.array_equal(_np(b).view(np.uint32), pool.B[idx])
    with pytest.raises(ValueError, match="exactly"):
        T.afterstates(env, into=env)
    scratch.terminate()
    env.terminate()


def test_without_a_network_the_policy_takes_the_best_distinct_reward(pool):
    n, params = 300, (1.0, 0.0, -1.0)
    env, idx = _resident(pool, n, 500, params)
    out = T.afterstates(env)
    reward, canonical = _np(out["reward"]), _np(out["canonical"])
    state = R.decode_state(_np(out["states_a"]).reshape(-1, 4), _np(out["states_b"]).reshape(-1, 4))["state"].reshape(n, 40)
    for chunk in (16384, 128, 7):
        policy = T.LookaheadPolicy(env, image=None, chunk=chunk)
        assert policy.scratch is None and policy.chunk == min(chunk, n)
        act = _np(policy.act())
        assert act.dtype == np.uint8 and act.shape == (n,)
        distinct = canonical == np.arange(40)[None, :]
        masked = np.where(distinct, reward, -np.inf)
        want = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)       # the lowest index at the float32 maximum
        assert np.array_equal(act, want), chunk
    run = pool.running[idx]
    assert (act[~run] == 0).all() and (~run).any()
    picked_topout = state[np.arange(n), act] == 3
    escape = ((state != 3) & distinct).any(axis=1)
    assert not (picked_topout & escape & run).any()
    assert (picked_topout & run).any() or (((state == 3).any(axis=1)) & escape & run).any()     # there were top-outs to avoid
    buf = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    assert policy.act(out=buf) is buf and np.array_equal(_np(buf), want)
    env.terminate()


def test_with_a_network_the_chosen_action_has_the_best_score_within_the_roundings(pool):
    n, chunk, gamma, params = 300, 128, 0.99, REWARDS[1]
    env, idx = _resident(pool, n, 900, params)
    image = T.actor.policy_image(_model(12), env.device, f32="split")
    policy = T.LookaheadPolicy(env, image=image, gamma=gamma, chunk=chunk)
    assert policy.chunk == chunk and policy.scratch.num_envs == 40 * chunk     # three chunks, the last of 44 boards
    act = _np(policy.act()).astype(np.int64)
    # the score in float64 on the host: the kernel's reward and done, logits of a separate policy_act over the afterstates
    other = T.BatchedTetris(L, M, 40 * n, device=DEV, seed=2)
    out = T.afterstates(env, into=other)
    logits = torch.empty((40 * n, 14), dtype=torch.float32, device=DEV)
    other.policy_act(image, logits=logits)
    lg = _np(logits).astype(np.float64)
    V = (lg[:, :4].max(axis=1) + lg[:, 4:].max(axis=1)).reshape(n, 40)
    reward, done = _np(out["reward"]).astype(np.float64), _np(out["done"]).astype(np.float64)
    canonical = _np(out["canonical"])
    score = reward + gamma * (1.0 - done) * V
    tol = 4 * 2.0 ** -24 * (np.abs(reward) + gamma * np.abs(V))
    distinct = canonical == np.arange(40)[None, :]
    rows = np.arange(n)
    assert distinct[rows, act].all()
    best = np.where(distinct, score, -np.inf).argmax(axis=1)
    slack = tol[rows, act] + tol[rows, best]
    short = score[rows, best] - score[rows, act]
    print(f"n = {n}: {int((act != best).sum())} choices differ from the float64 arg-max, largest shortfall {short.max():.3e} "
          f"(tolerance there {slack[short.argmax()]:.3e}); distinct actions chosen: {len(set(act.tolist()))}")
    assert (short <= slack).all(), (short.max(), slack[short.argmax()])
    run = pool.running[idx]
    assert (act[~run] == 0).all() and (~run).any() and len(set(act[run].tolist())) > 3
    other.terminate()
    env.terminate()


# ------------------------------------------------------------------------------------------------ 4. the learner
def test_the_learner_evaluates_with_the_lookahead_and_the_default_path_is_untouched():
    n, seed = 4096, 3
    rows, pieces = T.generate_configs(2, 2, 64, seed=100 + seed)
    env = _env(2, 2, n, seed=seed, pool=(rows, pieces), reward=(0.0, 1.0, 0.0))
    learner = T.DQNLearner(env, model=_model(seed), capacity=1 << 14, batch_size=1024, seed=seed)
    learner.collect(2)
    learner.update(2)
    with pytest.raises(ValueError, match="epsilon"):
        learner.evaluate(4, epsilon=0.5, lookahead=True)
    got = learner.evaluate(4, lookahead=True)
    print("evaluate(4, lookahead=True):", got)
    assert set(got) == {"episodes", "wins", "win_rate"} and got["episodes"] > 0 and 0 <= got["wins"] <= got["episodes"]
    assert got["win_rate"] == got["wins"] / got["episodes"]
    assert learner.eval_env.step_clock() == 4
    assert learner.evaluate(4, lookahead=True) == got          # deterministic, from a full reset
    after = learner.evaluate(4)
    # a learner with the same online net that never used the lookahead
    env2 = _env(2, 2, n, seed=seed, pool=(rows, pieces), reward=(0.0, 1.0, 0.0))
    plain = T.DQNLearner(env2, model=copy.deepcopy(learner.model), capacity=1 << 14, batch_size=1024, seed=seed)
    assert plain.evaluate(4) == after and after["episodes"] > 0
    assert getattr(plain, "_lookahead", None) is None and learner._lookahead.scratch.num_envs == 40 * n
    env.terminate()
    env2.terminate()
