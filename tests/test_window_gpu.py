"""The exact search over a state's piece window and the proof policy on one MI355X (include/tpl_learn.h's rule;
tpl_placement_window_prove[_move] in csrc/learn/exact_window.hip; T.window_prove, T.ProofPolicy, the proof= argument of
T.evaluate_heuristic and NTupleLearner.evaluate).  THE KERNEL IS THE MIRROR, byte for byte, through guard-framed buffers filled with
0xCD; the mirror is pinned to placement_exact and placement_exact_nodes by tests/test_window_cpu.py.

The boards are an environment's own: a pool of the first 16 configurations of tests/golden/carved_L5_M20.npz (for L = 10 of
carved_L10_M40.npz, whose boards hold ten rows to clear; the lists cut to the game's M + 1) is played without auto-reset by a player that avoids clearing rows, so that boards are still running late, and by the
classical one-ply player for two moves; the resident planes are copied at moves 0, 1, 2, 9, 10, 11, 19 (those below M) and at the
end, when every board is finished.  A launch draws n boards from all of those, so it mixes the move counters with finished boards,
and in one case with skipped ones.

  1. the kernel against the mirror: both feature forms, n = 1, 63, 64, 65, 203, the games (1, 1), (2, 6), (5, 10), (5, 20), (10, 16),
     max_nodes 1, 64, 1024;
  2. the kernel against the existing kernel: T.window_prove's six shared outputs against T.prove_nodes on the node
     (rows, lines, M - H, i) over the list that holds the window from M - H on;
  3. the policy on 16 boards over the 16 configurations in the game (5, 10), reuse off and on; a dropped plan;
  4. the evaluate hooks.
"""
import functools

import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import load_golden
from learn_ref import decode_state
from test_learn_range_gpu import Framed, _check, _stream
from test_learner_gpu import _np
from test_solve_cpu import CW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNT = 16
NAMES = ("solved", "proved", "solution_len", "plan", "bound", "nodes", "horizon", "verdict")
DTYPES = dict(solved=np.uint8, proved=np.uint8, solution_len=np.int32, plan=np.uint8, bound=np.int32, nodes=np.uint32, horizon=np.uint8,
              verdict=np.uint8)
SNAPS = (0, 1, 2, 9, 10, 11, 19)
# rows cleared, won and lost all cost: the player stacks flat and keeps its boards running for as long as the board lets it
AVOID = np.array([-50, -100, -100, -1, -1, 0, -1, 0, 0, 0, 0, 0], np.float32)
# (L, M, n, max_nodes, skip every k-th board or 0)
CASES = [(1, 1, 1, 1, 0), (1, 1, 65, 64, 0), (2, 6, 63, 64, 0), (2, 6, 64, 1024, 0), (5, 10, 64, 64, 0), (5, 10, 65, 1, 0),
         (5, 20, 203, 64, 0), (5, 20, 65, 1024, 0), (5, 20, 64, 64, 3), (10, 16, 65, 64, 0), (10, 16, 63, 1024, 5)]


def _m():
    return T._learn_lib


def weights_of(count):
    return CW if count == 12 else np.array(T.DELLACHERIE_WEIGHTS, np.float32)


def _pool(M, L=5):
    g = load_golden("carved_L10_M40.npz" if L == 10 else "carved_L5_M20.npz")
    return g["rows"][:COUNT], np.ascontiguousarray(g["pieces"][:COUNT, :M + 1])


@functools.lru_cache(maxsize=None)
def boards_of(L, M):
    """The planes an environment of the game (L, M) went through (above): uint32 [K, 4] pairs and, per board, the move it was copied at
    (M for the last copy).  Made once per game; nobody writes to it."""
    rows, pieces = _pool(M, L)
    a, b, at = [], [], []
    for weights, times, last in ((AVOID, [t for t in SNAPS if t < M], True), (CW, [t for t in (1, 2) if t < M], False)):
        env = T.BatchedTetris(L, M, 64, device=DEV, seed=3, auto_reset=False)
        env.load_configs(rows, pieces)
        env.reset()
        player = T.HeuristicPolicy(env, weights)
        for t in range(M + 1):
            if t in times or (last and t == M):
                pa, pb = env.raw_planes()
                a.append(_np(pa).view(np.uint32)); b.append(_np(pb).view(np.uint32)); at.append(np.full(64, t))
            if t < M:
                env.step(player.act(), observe=False)
        env.terminate()
    return np.concatenate(a), np.concatenate(b), np.concatenate(at)


def launch_boards(L, M, n):
    """n boards of boards_of(L, M), drawn with a stride so that every launch mixes the copies: planes and decoded fields."""
    a, b, at = boards_of(L, M)
    pick = (np.arange(n) * 37 + 5) % a.shape[0]
    a, b = np.ascontiguousarray(a[pick]), np.ascontiguousarray(b[pick])
    return a, b, decode_state(a, b), at[pick]


@functools.lru_cache(maxsize=None)
def mirror(L, M, n, cap, skip, count):
    _, _, s, _ = launch_boards(L, M, n)
    return _m().placement_window_prove(s["rows"], s["lines"].astype(np.int64), s["moves"].astype(np.int64), s["state"].astype(np.int64),
                                       s["window"], L, M, weights_of(count), cap, skip=skip_of(n, skip))


def skip_of(n, skip):
    return None if not skip else (np.arange(n) % skip == 0).astype(np.uint8)


def _weight_buffer(w):
    """A weight row as the entries read it: twelve floats, or sixteen with NaN in the two entries that are never read."""
    if w.shape[0] == 12:
        return np.array(w, np.float32)
    out = np.full(16, np.nan, np.float32)
    out[:14] = w
    return out


def _launch(a, b, L, M, w, cap, skip=None, spare_weight=0.0):
    """tpl_placement_window_prove[_move] through guard-framed buffers, every output filled with 0xCD first: the outputs on the host."""
    n = a.shape[0]
    host = [a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1), _weight_buffer(np.asarray(w, np.float32)).view(np.uint8)]
    if skip is not None:
        host.append(np.ascontiguousarray(skip, np.uint8))
    frames = []
    for seed, x in enumerate(host):
        f = Framed(x.nbytes, seed + 1)
        f.inner().copy_(torch.from_numpy(np.ascontiguousarray(x)))
        frames.append(f)
    sizes = dict(solved=n, proved=n, solution_len=4 * n, plan=12 * n, bound=4 * n, nodes=4 * n, horizon=n, verdict=n)
    out = {k: Framed(sizes[k], 10 + j) for j, k in enumerate(NAMES)}
    for f in out.values():
        f.inner().fill_(0xCD)
    _check(_m().entry("window_prove", len(w))(frames[0].ptr(), frames[1].ptr(), n, L, M, frames[2].ptr(), float(spare_weight), int(cap),
                                              frames[3].ptr() if skip is not None else None, *(out[k].ptr() for k in NAMES), _stream()))
    for f in list(out.values()) + frames:
        f.assert_canary((L, M, n, cap))
    got = {k: out[k].host().view(DTYPES[k]).copy() for k in NAMES}
    got["plan"] = got["plan"].reshape(n, 12)
    return got


def _same(got, want, what):
    for name in NAMES:
        ref = np.ascontiguousarray(want[name])
        assert got[name].dtype == ref.dtype and got[name].shape == ref.shape, (what, name, got[name].shape, ref.shape)
        bad = np.argwhere(got[name].view(np.uint8) != ref.view(np.uint8))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ 1. the kernel is the mirror
@pytest.mark.parametrize("count", (12, 14))
@pytest.mark.parametrize("L,M,n,cap,skip", CASES)
def test_the_kernel_is_the_mirror_byte_for_byte(L, M, n, cap, skip, count):
    a, b, s, at = launch_boards(L, M, n)
    got = _launch(a, b, L, M, weights_of(count), cap, skip_of(n, skip))
    want = mirror(L, M, n, cap, skip, count)
    _same(got, want, (L, M, n, cap, skip, count))
    print((L, M, n, cap, skip, count), "moves", sorted(set(at.tolist())), "finished", int((s["state"] != 0).sum()), "verdicts",
          np.bincount(got["verdict"], minlength=4).tolist(), "horizons", sorted(set(got["horizon"].tolist())), "most nodes",
          int(got["nodes"].max()))
    running = s["state"] == 0
    assert (got["verdict"][~running] == 0).all() and (got["nodes"] <= cap).all()
    if skip:
        assert (got["nodes"][::skip] == 0).all() and (got["verdict"][::skip] == 0).all() and (got["proved"][::skip] == 0).all()
    if n >= 63:                                                # the launch mixes running boards of several moves with finished ones
        assert (~running).any() and running.any() and len(set(at[running].tolist())) >= min(3, M)
    assert np.array_equal(s["moves"][running], at[running])


def test_the_launches_cover_every_verdict_and_every_horizon_kind():
    """What the cases above met, from their mirrors: all four verdicts, H == rem and H < rem, a capped search and a skipped board."""
    seen, short, end = set(), False, False
    for L, M, n, cap, skip in CASES:
        _, _, s, _ = launch_boards(L, M, n)
        want = mirror(L, M, n, cap, skip, 12)
        seen |= set(want["verdict"].tolist())
        running = s["state"] == 0
        rem = M - s["moves"].astype(np.int64)
        short |= bool((running & (want["horizon"] < rem)).any())
        end |= bool((running & (want["horizon"] == rem) & (want["nodes"] > 0)).any())
    assert seen == {0, 1, 2, 3} and short and end
    # the environment's boards were still running at every move the launches are to mix
    for L, M in sorted({(L, M) for L, M, _, _, _ in CASES}):
        a, b, at = boards_of(L, M)
        s = decode_state(a, b)
        for t in (t for t in SNAPS if t < M):
            assert ((s["state"] == 0) & (at == t)).any(), (L, M, t)
        assert (s["state"][at == M] != 0).all()
    _, _, s, at = launch_boards(5, 20, 203)
    assert {0, 9, 10, 11, 19} <= set(at[s["state"] == 0].tolist())


# ------------------------------------------------------------------------------------------------ 2. the existing kernel
@pytest.mark.parametrize("count", (12, 14))
@pytest.mark.parametrize("L,M,n,cap", [(5, 20, 203, 64), (10, 16, 65, 64), (5, 20, 65, 1024), (2, 6, 63, 64)])      # launches of CASES: their mirrors are at hand
def test_window_prove_writes_what_prove_nodes_writes_for_the_shifted_node(L, M, n, cap, count):
    a, b, s, _ = launch_boards(L, M, n)
    env = T.BatchedTetris(L, M, n, device=DEV, seed=1, auto_reset=False)
    env.write_raw_planes(torch.from_numpy(a.view(np.int32)), torch.from_numpy(b.view(np.int32)))
    before = env.snapshot().data.clone()
    w = weights_of(count)
    got = T.window_prove(env, weights=w, max_nodes=cap)
    assert torch.equal(env.snapshot().data, before)            # read, never written
    H = _np(got["horizon"]).astype(np.int64)
    running = s["state"] == 0
    known = 12 - s["moves"].astype(np.int64) % 10
    assert np.array_equal(_np(got["known"]), known.astype(np.uint8))
    assert np.array_equal(H, np.where(running, np.minimum(known, M - s["moves"].astype(np.int64)), 0))
    q = _m().window_entries(s["window"])
    lists = np.full((n, M + 1), 7, np.uint8)
    for i in range(n):
        lists[i, M - H[i]:M] = q[i, :H[i]]
    lines = np.where(running, s["lines"], L)                   # a finished board is a finished node
    ref = T.prove_nodes(s["rows"], lines, M - H, np.arange(n), lists, L, M, weights=w, max_nodes=cap, device=DEV, validate=False)
    for name in ("solved", "proved", "solution_len", "bound", "nodes"):
        assert got[name].dtype == ref[name].dtype and torch.equal(got[name], ref[name]), name
    width = min(12, M)
    assert torch.equal(got["plan"][:, :width], ref["actions"][:, :width])
    assert bool((got["plan"][:, width:] == 255).all()) and bool((ref["actions"][:, width:] == 255).all())
    assert torch.equal(got["action"], got["plan"][:, 0])
    # through the Python layer the kernel is still the mirror
    want = mirror(L, M, n, cap, 0, count)
    for name in NAMES:
        assert np.array_equal(_np(got[name]).astype(want[name].dtype), want[name]), name
    env.terminate()


# ------------------------------------------------------------------------------------------------ 3. the policy
def _policy_env(auto_reset=True):
    rows, pieces = _pool(10)
    env = T.BatchedTetris(5, 10, COUNT, device=DEV, seed=2, auto_reset=auto_reset, assign="sequential", reward=(0.0, 1.0, 0.0))
    env.load_configs(rows, pieces)
    env.reset()
    assert np.array_equal(_np(T.config_index(env)), np.arange(COUNT))          # board i plays configuration i
    return env


@pytest.mark.parametrize("reuse", (False, True))
def test_a_proved_episode_is_won_after_exactly_its_length_and_the_base_plays_the_rest(reuse):
    env = _policy_env()
    base = T.HeuristicPolicy(env, CW)
    policy = T.ProofPolicy(env, base, max_nodes=1024, reuse=reuse)
    first = T.window_prove(env, max_nodes=1024)
    proved0 = _np(first["verdict"]) == 1
    length0 = _np(first["solution_len"]).astype(np.int64)
    assert proved0.sum() == 12 and proved0.tolist() == [bool(x) for x in [1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1]]
    action = torch.empty(COUNT, dtype=torch.uint8, device=DEV)
    verdict = torch.empty(COUNT, dtype=torch.uint8, device=DEV)
    reward = torch.empty(COUNT, dtype=torch.float32, device=DEV)
    done = torch.empty(COUNT, dtype=torch.uint8, device=DEV)
    ended = np.full(COUNT, -1)                                 # the step at which a board's first episode ended, and how
    won = np.zeros(COUNT, bool)
    followed = 0
    for t in range(10):
        own = _np(base.act()).copy()
        assert policy.act(out=action, verdict=verdict) is action
        v, played, nodes = _np(verdict), _np(policy.played), _np(policy.nodes)
        assert np.array_equal(_np(action)[~played], own[~played]), t           # no proof: the base's move
        first_episode = ended < 0
        live = first_episode & proved0 & (t < length0)
        assert played[live].all(), t
        if t == 0:
            assert np.array_equal(v == 1, proved0) and np.array_equal(_np(action)[proved0], _np(first["plan"])[proved0, 0])
        elif reuse:                                            # a live plan is followed, not searched for again
            assert (nodes[live] == 0).all() and (v[live] == 0).all(), t
            followed += int(live.sum())
        else:                                                  # searched again: one move on, a proof is one move shorter; a search that
            again = live & (v == 1)                            # the node budget stops leaves the kept plan in force
            assert (nodes[live] > 0).all() and np.array_equal(_np(policy._out["solution_len"])[again], (length0 - t)[again]), t
        assert np.array_equal(_np(policy.finishing)[live], (t == length0 - 1)[live]), t
        env.step_into(action, reward, done)
        d, r = _np(done).astype(bool), _np(reward)
        now = first_episode & d
        ended[now], won[now] = t, r[now] == 1.0
    assert np.array_equal(ended[proved0], length0[proved0] - 1) and won[proved0].all()      # won after exactly solution_len steps
    stats = policy.stats()
    print("reuse", reuse, "first episodes: ended at", ended.tolist(), "won", won.astype(int).tolist(), stats)
    assert stats["plan_moves"] >= int(length0[proved0].sum()) and stats["win"] >= 12
    if reuse:
        assert followed == int((length0[proved0] - 1).sum())
    env.terminate()


def test_a_plan_is_dropped_when_the_board_is_not_the_one_it_expects():
    m = _m()
    env = _policy_env()
    base = T.HeuristicPolicy(env, CW)
    policy = T.ProofPolicy(env, base, max_nodes=1024, reuse=True)
    action = policy.act().clone()
    held = _np(policy.played) & ~_np(policy.finishing)
    length = _np(policy._out["solution_len"])
    board = int(np.flatnonzero(held & (length >= 3))[0])
    cur = int(_np(env.packed_state()["cur"])[board])
    canonical = m.canonical_actions(cur, np.arange(40))
    other = int(np.flatnonzero(canonical != canonical[int(action[board])])[0])           # another placement of the same piece
    action[board] = other
    reward = torch.empty(COUNT, dtype=torch.float32, device=DEV)
    done = torch.empty(COUNT, dtype=torch.uint8, device=DEV)
    env.step_into(action, reward, done)
    assert not bool(done[board])                               # a shortest win of three moves or more: no single move ends the game won
    policy.act()
    nodes, verdict = _np(policy.nodes), _np(policy.verdict)
    assert verdict[board] != 0                                 # the plan was dropped: the board was searched again
    rest = held.copy()
    rest[board] = False
    assert rest.any() and (nodes[rest] == 0).all() and (verdict[rest] == 0).all() and _np(policy.played)[rest].all()
    # a full reset drops every plan
    env.reset()
    policy.act()
    assert (_np(policy.nodes) > 0).all() and np.array_equal(_np(policy.verdict) == 1, _np(T.window_prove(env, max_nodes=1024)["verdict"]) == 1)
    env.terminate()


# ------------------------------------------------------------------------------------------------ 4. the evaluate hooks
def test_the_evaluate_hooks_leave_results_alone_without_proof_and_count_wins_with_it():
    rows, pieces = _pool(10)
    env = T.BatchedTetris(5, 10, 64, device=DEV, seed=4, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=(rows, pieces))
    plain = T.evaluate_heuristic(env, CW, None, 30)
    same = T.evaluate_heuristic(env, CW, None, 30, proof=None)
    assert sorted(plain) == sorted(same) and all(np.array_equal(plain[k], same[k]) for k in plain)
    with_proof = T.evaluate_heuristic(env, CW, None, 30, proof=256)
    counted = env.stats()
    assert int(with_proof["episodes"].sum()) == counted["episodes"] and int(with_proof["wins"].sum()) == counted["wins"]
    assert with_proof["proof"]["win"] > 0 and with_proof["proof"]["plan_moves"] > 0
    print("one ply", plain["win_rate"], "with proofs", with_proof["win_rate"], with_proof["proof"])
    learner = T.NTupleLearner(env, shape="feat", seed=1)
    plain = learner.evaluate(30)
    same = learner.evaluate(30, proof=None)
    assert plain == same
    with_proof = learner.evaluate(30, proof=256)
    counted = env.stats()
    assert with_proof["episodes"] == counted["episodes"] and with_proof["wins"] == counted["wins"]      # a plan's last move is a win
    assert with_proof["proof"]["win"] > 0
    for bad in (0, True, 2.5, (1 << 24) + 1):
        with pytest.raises(ValueError):
            T.evaluate_heuristic(env, CW, None, 30, proof=bad)
        with pytest.raises(ValueError):
            learner.evaluate(30, proof=bad)
    env.terminate()
