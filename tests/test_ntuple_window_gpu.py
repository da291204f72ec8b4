"""The window proof search ordered by an n-tuple table, and the proof policy on top of it, on one MI355X (include/tpl_learn.h's rule
under tpl_ntuple_window_prove; csrc/learn/ntuple_window.hip; T.ntuple_window_prove, T.ProofPolicy(table=), the proof_table= argument of
T.evaluate_heuristic and NTupleLearner.evaluate).  THE KERNEL IS THE MIRROR, byte for byte in all eight outputs, through guard-framed
buffers filled with 0xCD, against tests/golden/ntuple_window_mirror.npz (tests/test_ntuple_window_cpu.py pins the file to
_learn_lib.ntuple_window_prove; tests/golden/make_golden_ntuple_window.py lists the cases).

A board is searched on its own, so the mirror's output for a launch of n boards drawn from a case's states is the case's recorded rows,
drawn the same way: the mirror's CPU share of this file is nothing.

  1. the kernel against the mirror: make_golden_window's mid-game and reset boards, drawn with a stride to n = 1, 63, 64, 65, 203; the
     games (5, 20), (5, 10) and the small game (2, 3); max_nodes 1, 64 and 1,024 under every form in (5, 20), 1 and 64 under "2x4" and "3x3"
     in the two other games; a skip mask; gamma 0.5 with reward (1, 10, -1); the zero table with zero reward; the huge table, whose sums are rounded;
  2. the kernel against the existing kernel: T.ntuple_window_prove's six shared outputs against T.ntuple_prove_configs per (lines, H)
     group, on boards an environment reached at moves 0, 1, 9, 10, 11;
  3. independence of the order on the device, against T.window_prove;
  4. the policy on 16 boards over the 16 configurations in the game (5, 10), reuse off and on; a dropped plan; table=None;
  5. the evaluate hooks.
"""
import functools
import sys

import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import GOLDEN, load_golden
from learn_ref import decode_state, pack_state
from test_learn_range_gpu import Framed, _check, _stream
from test_learner_gpu import _np
from test_solve_cpu import CW
from test_window_gpu import AVOID, COUNT, DTYPES, NAMES, _policy_env, _pool

sys.path.insert(0, GOLDEN)
import make_golden_ntuple_window as G  # noqa: E402  -- the cases
import make_golden_ntuple_exact as N  # noqa: E402  -- the tables

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIX = ("solved", "proved", "solution_len", "bound", "nodes")
_device_tables = {}
# (the recorded cases whose states are put one behind the other, n)
LAUNCHES = [
    (("mid_budget_c1024", "root_M20_budget_c1024"), 203), (("mid_feat_c1024", "root_M20_feat_c1024"), 65),
    (("mid_linear_c1024", "root_M20_linear_c1024"), 64), (("mid_budget_c64",), 63), (("mid_feat_c64",), 64), (("mid_linear_c64",), 65),
    (("mid_3x3_c64", "root_M20_3x3_c64"), 65), (("mid_2x4_c64", "root_M20_2x4_c64"), 203),
    (("mid_budget_c1", "root_M20_budget_c1"), 1), (("mid_feat_c1", "root_M20_feat_c1"), 65), (("mid_3x3_c1", "root_M20_3x3_c1"), 63),
    (("mid_2x4_c1", "root_M20_2x4_c1"), 64),
    (("mid_3x3_c1024", "root_M20_3x3_c1024"), 65), (("mid_2x4_c1024", "root_M20_2x4_c1024"), 64),
    (("mid_budget_skip",), 203), (("mid_budget_gamma",), 65), (("mid_ties_c64",), 64), (("mid_huge_c64",), 65),
    (("mid10_budget_c1024", "root_M10_budget_c1024"), 203), (("mid10_3x3_c64", "root_M10_3x3_c64"), 65),
    (("mid10_2x4_c64", "root_M10_2x4_c64"), 63), (("root_M10_feat_c1024",), 64), (("root_M10_linear_c1024",), 1),
    (("loss_small_budget_c1",), 1), (("loss_small_budget_c64",), 63), (("loss_small_budget_c1024",), 64), (("loss_small_feat_c1",), 65),
    (("loss_small_feat_c64",), 203), (("loss_small_feat_c1024",), 63), (("loss_small_3x3_c1",), 64), (("loss_small_3x3_c64",), 65),
    (("loss_small_2x4_c1",), 63), (("loss_small_2x4_c64",), 64),
]


def _m():
    return T._learn_lib


def _table(tag):
    """The table of a case in a guard-framed buffer of its own, uploaded once; every launch checks its canaries."""
    if tag not in _device_tables:
        t = N.table(*G.TABLES[tag])
        f = Framed(t.size * 4, 3)
        f.inner().copy_(torch.from_numpy(t.view(np.uint8).copy()))
        _device_tables[tag] = (f, t)
    return _device_tables[tag]


@functools.lru_cache(maxsize=None)
def boards(keys):
    """The states of the cases `keys` one behind the other as packed planes, their skip flags, and the recorded mirror outputs."""
    rec = load_golden("ntuple_window_mirror.npz")
    a, b, skip, want = [], [], [], {name: [] for name in NAMES}
    for key in keys:
        s = G.states_of(key)
        k = s["rows"].shape[0]
        pa, pb = pack_state(s["rows"], s["lines"], s["moves"], s["state"], 0, s["window"])
        back = decode_state(pa, pb)                            # the planes hold the states the mirror was given
        for name in ("rows", "lines", "moves", "state", "window"):
            assert np.array_equal(np.asarray(back[name]).astype(np.uint64), np.asarray(s[name]).astype(np.uint64)), (key, name)
        a.append(pa); b.append(pb)
        flags = G.skip_of(G.CASES[key], k)
        skip.append(np.zeros(k, np.uint8) if flags is None else flags)
        for name in NAMES:
            want[name].append(rec[f"{key}_{name}"])
    return np.concatenate(a), np.concatenate(b), np.concatenate(skip), {name: np.concatenate(v) for name, v in want.items()}


def _launch(a, b, L, M, tag, cap, skip=None, gamma=1.0, reward=(1.0, 0.0, 0.0)):
    """tpl_ntuple_window_prove through guard-framed buffers, every output filled with 0xCD first: the outputs on the host."""
    n = a.shape[0]
    host = [a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1)]
    if skip is not None:
        host.append(np.ascontiguousarray(skip, np.uint8))
    frames = []
    for seed, x in enumerate(host):
        f = Framed(x.nbytes, seed + 1)
        f.inner().copy_(torch.from_numpy(np.ascontiguousarray(x)))
        frames.append(f)
    tf, table = _table(tag)
    sizes = dict(solved=n, proved=n, solution_len=4 * n, plan=12 * n, bound=4 * n, nodes=4 * n, horizon=n, verdict=n)
    out = {k: Framed(sizes[k], 10 + j) for j, k in enumerate(NAMES)}
    for f in out.values():
        f.inner().fill_(0xCD)
    _check(_m().lib().tpl_ntuple_window_prove(frames[0].ptr(), frames[1].ptr(), n, L, M, tf.ptr(), table.size, *(float(r) for r in reward),
                                              float(gamma), int(cap), frames[2].ptr() if skip is not None else None,
                                              *(out[k].ptr() for k in NAMES), _stream()))
    for f in list(out.values()) + frames + [tf]:
        f.assert_canary((L, M, n, tag, cap))
    assert np.array_equal(tf.host().view(np.int32), table)     # nothing but the outputs is written
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
@pytest.mark.parametrize("keys,n", LAUNCHES, ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_the_kernel_is_the_mirror_byte_for_byte(keys, n):
    case = G.CASES[keys[0]]
    for key in keys[1:]:                                       # one launch: one game, one table, one cap
        assert all(G.CASES[key][k] == case[k] for k in ("table", "max_nodes", "gamma", "reward", "skip"))
    s = G.states_of(keys[0])
    L, M = s["L"], s["M"]
    a, b, skip, want = boards(keys)
    pick = (np.arange(n) * 37 + 5) % a.shape[0]
    a, b = np.ascontiguousarray(a[pick]), np.ascontiguousarray(b[pick])
    got = _launch(a, b, L, M, case["table"], case["max_nodes"], skip[pick] if case["skip"] else None, case["gamma"], case["reward"])
    _same(got, {name: want[name][pick] for name in NAMES}, (keys, n))
    print(keys, n, "verdicts", np.bincount(got["verdict"], minlength=4).tolist(), "horizons", sorted(set(got["horizon"].tolist())),
          "most nodes", int(got["nodes"].max()))
    assert (got["nodes"] <= case["max_nodes"]).all()
    if case["skip"]:
        assert skip[pick].any() and (got["nodes"][skip[pick] != 0] == 0).all() and (got["verdict"][skip[pick] != 0] == 0).all()
    if n >= 63 and keys[0].startswith("mid"):                  # the launch mixes running boards of several counters with finished ones
        assert (got["verdict"] == 0).any() and len(set(got["horizon"].tolist())) >= 3


def test_the_launches_cover_every_verdict_every_table_form_and_every_cap():
    seen, forms, caps, sizes, whole_window = set(), set(), set(), set(), False
    for keys, n in LAUNCHES:
        _, _, _, want = boards(keys)
        pick = (np.arange(n) * 37 + 5) % want["verdict"].shape[0]
        seen |= set(want["verdict"][pick].tolist())
        whole_window |= bool(((want["horizon"][pick] == 12) & (want["nodes"][pick] > 0)).any())
        forms.add(G.TABLES[G.CASES[keys[0]]["table"]])
        caps.add((G.TABLES[G.CASES[keys[0]]["table"]][0], G.CASES[keys[0]]["max_nodes"]))
        sizes.add(n)
    assert seen == {0, 1, 2, 3} and sizes == {1, 63, 64, 65, 203}
    assert whole_window                                        # a searched board with H = 12: the table order reads list entry 12, the 0
    assert {f for f, _ in forms} == {"2x4", "3x3", "feat", "feat+spare"} and {k for _, k in forms} == {"hashed", "linear", "zero", "huge"}
    assert {("feat", c) for c in (1, 64, 1024)} | {("feat+spare", c) for c in (1, 64, 1024)} | {("2x4", 1), ("2x4", 64), ("3x3", 1), ("3x3", 64)} <= caps


# ------------------------------------------------------------------------------------------------ 2. the existing kernel
@functools.lru_cache(maxsize=None)
def env_boards():
    """64 boards an environment of the game (5, 20) reached, its pool the first 16 configurations of the fixture: the planes copied at
    moves 0, 1, 9, 10 and 11 under a player that keeps its boards running, drawn with a stride."""
    rows, pieces = _pool(20)
    env = T.BatchedTetris(5, 20, 64, device=DEV, seed=3, auto_reset=False)
    env.load_configs(rows, pieces)
    env.reset()
    player = T.HeuristicPolicy(env, AVOID)
    a, b = [], []
    for t in range(12):
        if t in (0, 1, 9, 10, 11):
            pa, pb = env.raw_planes()
            a.append(_np(pa).view(np.uint32)); b.append(_np(pb).view(np.uint32))
        env.step(player.act(), observe=False)
    env.terminate()
    a, b = np.concatenate(a), np.concatenate(b)
    pick = (np.arange(64) * 37 + 5) % a.shape[0]
    return np.ascontiguousarray(a[pick]), np.ascontiguousarray(b[pick])


def _env_of(a, b):
    env = T.BatchedTetris(5, 20, a.shape[0], device=DEV, seed=1, auto_reset=False)
    env.write_raw_planes(torch.from_numpy(a.view(np.int32)), torch.from_numpy(b.view(np.int32)))
    return env


@pytest.mark.parametrize("tag,cap", [("budget", 1024), ("feat", 64), ("3x3", 64), ("2x4", 64)])
def test_ntuple_window_prove_writes_what_ntuple_prove_configs_writes_for_the_shifted_configuration(tag, cap):
    a, b = env_boards()
    s = decode_state(a, b)
    n, L, M = a.shape[0], 5, 20
    env = _env_of(a, b)
    before = env.snapshot().data.clone()
    table = torch.from_numpy(N.table(*G.TABLES[tag]).copy()).to(DEV)
    got = T.ntuple_window_prove(env, table, max_nodes=cap)
    assert torch.equal(env.snapshot().data, before)            # read, never written
    ref = T.window_prove(env, max_nodes=cap)
    assert sorted(got) == sorted(ref)
    for name in ref:                                           # window_prove's dict: the same keys, dtypes and shapes
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape and got[name].device == ref[name].device, name
    for name in ("bound", "horizon", "known"):
        assert torch.equal(got[name], ref[name]), name
    assert torch.equal(got["action"], got["plan"][:, 0])
    moves, lines = s["moves"].astype(np.int64), s["lines"].astype(np.int64)
    running = (s["state"] == 0) & (lines < L) & (moves < M)
    assert running.sum() >= 48 and {0, 1, 9, 10, 11} <= set(moves[running].tolist())
    H = np.where(running, np.minimum(12 - moves % 10, M - moves), 0)
    assert np.array_equal(_np(got["horizon"]).astype(np.int64), H)
    q = _m().window_entries(s["window"])
    host = {k: _np(v) for k, v in got.items()}
    for at_lines, h in sorted({(int(x), int(y)) for x, y in zip(lines[running], H[running])}):
        idx = np.flatnonzero(running & (lines == at_lines) & (H == h))
        lists = np.concatenate([q[idx, :h], np.zeros((idx.size, 1), np.int64)], axis=1).astype(np.uint8)
        want = T.ntuple_prove_configs(s["rows"][idx], lists, L - at_lines, h, table, max_nodes=cap, device=DEV)
        for name in SIX:
            assert np.array_equal(host[name][idx], _np(want[name])), (name, at_lines, h)
        assert np.array_equal(host["plan"][idx][:, :h], _np(want["actions"])) and (host["plan"][idx][:, h:] == 255).all()
    assert (host["verdict"][~running] == 0).all() and (host["nodes"][~running] == 0).all()
    # a numpy table is uploaded; gamma and the reward reach the kernel; the skip mask too
    again = T.ntuple_window_prove(env, N.table(*G.TABLES[tag]), max_nodes=cap)
    for name in got:
        assert torch.equal(again[name], got[name]), name
    if tag == "budget":
        skip = torch.arange(n, device=DEV) % 2 == 0
        other = T.ntuple_window_prove(env, table, gamma=0.5, reward=(1.0, 10.0, -1.0), max_nodes=cap, skip=skip)
        mirror = _m().ntuple_window_prove(s["rows"], lines, moves, s["state"].astype(np.int64), s["window"], L, M, N.table(*G.TABLES[tag]), cap,
                                          gamma=0.5, reward=(1.0, 10.0, -1.0), skip=_np(skip))
        for name in NAMES:
            assert np.array_equal(_np(other[name]).astype(mirror[name].dtype), mirror[name]), name
    env.terminate()


# ------------------------------------------------------------------------------------------------ 3. independence on the device
def test_where_both_orders_finish_they_prove_the_same():
    a, b = env_boards()
    env = _env_of(a, b)
    classical = {k: _np(v) for k, v in T.window_prove(env, max_nodes=1024).items()}
    met = 0
    for tag in ("budget", "linear", "feat", "3x3"):
        table = torch.from_numpy(N.table(*G.TABLES[tag]).copy()).to(DEV)
        got = {k: _np(v) for k, v in T.ntuple_window_prove(env, table, max_nodes=1024).items()}
        both = got["proved"] & classical["proved"] & (classical["verdict"] != 0)
        # the player that made these boards avoids clearing rows, so many searches run to the cap; the comparison must not be empty
        # and must hold wins among it: an eighth of the launch
        assert both.sum() >= 8 and (classical["verdict"][both] == 1).any(), (tag, int(both.sum()))
        for name in ("verdict", "solution_len", "solved", "bound"):
            assert np.array_equal(got[name][both], classical[name][both]), (tag, name)
        out = both & ~got["solved"]
        assert np.array_equal(got["nodes"][out], classical["nodes"][out]), tag
        met += int((got["nodes"][both] != classical["nodes"][both]).sum())
    assert met > 0                                             # the orders differ: some proof took another number of nodes
    env.terminate()


# ------------------------------------------------------------------------------------------------ 4. the policy
@pytest.mark.parametrize("reuse", (False, True))
def test_a_proved_episode_is_won_after_exactly_its_length_under_the_table_order(reuse):
    rec = load_golden("ntuple_window_mirror.npz")
    env = _policy_env()
    base = T.HeuristicPolicy(env, CW)
    table = torch.from_numpy(N.table(*G.TABLES["budget"]).copy()).to(DEV)
    policy = T.ProofPolicy(env, base, max_nodes=1024, reuse=reuse, table=table)
    assert isinstance(policy, T.TableProofPolicy) and policy.table.data_ptr() == table.data_ptr()      # held, not copied
    first = T.ntuple_window_prove(env, table, max_nodes=1024)
    proved0 = _np(first["verdict"]) == 1
    length0 = _np(first["solution_len"]).astype(np.int64)
    want = rec["root_M10_budget_c1024_verdict"] == 1           # the mirror's count at the reset: 11 of 16
    assert np.array_equal(proved0, want) and proved0.sum() == want.sum() >= 9
    assert np.array_equal(length0, rec["root_M10_budget_c1024_solution_len"])
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
        else:                                                  # searched again: one move on, a proof is one move shorter
            again = live & (v == 1)
            assert (nodes[live] > 0).all() and np.array_equal(_np(policy._out["solution_len"])[again], (length0 - t)[again]), t
        assert np.array_equal(_np(policy.finishing)[live], (t == length0 - 1)[live]), t
        env.step_into(action, reward, done)
        d, r = _np(done).astype(bool), _np(reward)
        now = first_episode & d
        ended[now], won[now] = t, r[now] == 1.0
    assert np.array_equal(ended[proved0], length0[proved0] - 1) and won[proved0].all()      # won after exactly solution_len steps
    stats = policy.stats()
    print("reuse", reuse, "first episodes: ended at", ended.tolist(), "won", won.astype(int).tolist(), stats)
    assert stats["plan_moves"] >= int(length0[proved0].sum()) and stats["win"] >= int(proved0.sum())
    if reuse:
        assert followed == int((length0[proved0] - 1).sum())
    env.terminate()


def test_a_plan_is_dropped_when_the_caller_steps_with_another_action_and_the_table_is_read_as_it_stands():
    m = _m()
    env = _policy_env()
    base = T.HeuristicPolicy(env, CW)
    table = torch.from_numpy(N.table(*G.TABLES["budget"]).copy()).to(DEV)
    policy = T.ProofPolicy(env, base, max_nodes=1024, reuse=True, table=table)
    action = policy.act().clone()
    hashed_nodes = _np(policy.nodes).copy()
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
    # the table is held: written in place, it orders the next search -- here as the linear table does
    table.copy_(torch.from_numpy(N.table(*G.TABLES["linear"]).copy()).to(DEV))
    env.reset()
    policy.act()
    linear = load_golden("ntuple_window_mirror.npz")["root_M10_linear_c1024_nodes"]
    assert np.array_equal(_np(policy.nodes).astype(np.uint32), linear) and not np.array_equal(linear, hashed_nodes.astype(np.uint32))
    env.terminate()


def test_without_a_table_the_policy_plays_todays_actions_byte_for_byte():
    envs = [_policy_env() for _ in range(2)]
    plain = T.ProofPolicy(envs[0], T.HeuristicPolicy(envs[0], CW), max_nodes=64)
    none = T.ProofPolicy(envs[1], T.HeuristicPolicy(envs[1], CW), max_nodes=64, table=None)
    assert type(plain) is T.ProofPolicy and none.table is None
    for t in range(12):
        a, b = plain.act(), none.act()
        assert torch.equal(a, b) and torch.equal(plain.verdict, none.verdict) and torch.equal(plain.nodes, none.nodes), t
        assert torch.equal(plain.played, none.played) and torch.equal(plain.finishing, none.finishing), t
        for env, act in zip(envs, (a, b)):
            env.step(act, observe=False)
    assert plain.stats() == none.stats()
    for env in envs:
        env.terminate()


# ------------------------------------------------------------------------------------------------ 5. the evaluate hooks
def test_the_evaluate_hooks_pass_the_table_through():
    rows, pieces = _pool(10)
    env = T.BatchedTetris(5, 10, 64, device=DEV, seed=4, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=(rows, pieces))
    table = torch.from_numpy(N.table(*G.TABLES["linear"]).copy()).to(DEV)
    plain = T.evaluate_heuristic(env, CW, None, 30, proof=64)
    same = T.evaluate_heuristic(env, CW, None, 30, proof=64, proof_table=None)
    assert sorted(plain) == sorted(same) and all(np.array_equal(plain[k], same[k]) for k in plain if k != "proof") and plain["proof"] == same["proof"]
    ordered = T.evaluate_heuristic(env, CW, None, 30, proof=64, proof_table=table)
    counted = env.stats()
    assert int(ordered["episodes"].sum()) == counted["episodes"] and int(ordered["wins"].sum()) == counted["wins"]
    assert ordered["proof"]["win"] > 0 and ordered["proof"]["plan_moves"] > 0 and ordered["proof"] != plain["proof"]
    print("classical order", plain["win_rate"], plain["proof"], "table order", ordered["win_rate"], ordered["proof"])
    learner = T.NTupleLearner(env, shape="feat", seed=1)
    plain = learner.evaluate(30, proof=64)
    assert learner.evaluate(30, proof=64, proof_table=False) == plain and learner.evaluate(30, proof=64, proof_table=None) == plain
    own = learner.evaluate(30, proof=64, proof_table=True)
    counted = env.stats()
    assert own["episodes"] == counted["episodes"] and own["wins"] == counted["wins"]      # a plan's last move is a win
    assert own["proof"]["win"] > 0
    given = learner.evaluate(30, proof=64, proof_table=table)
    assert given["proof"]["win"] > 0 and sorted(given) == sorted(plain)
    with pytest.raises(ValueError, match="needs proof"):
        learner.evaluate(30, proof_table=True)
    with pytest.raises(ValueError, match="needs proof"):
        T.evaluate_heuristic(env, CW, None, 30, proof_table=table)
    with pytest.raises(ValueError, match="four plain forms"):
        T.evaluate_heuristic(env, CW, None, 30, proof=64, proof_table=torch.zeros(_m().NTUPLE_ENTRIES_SUM, dtype=torch.int32, device=DEV))
    summed = T.NTupleLearner(env, shape="2x4+3x3", seed=1)     # a sum-shaped learner orders no search
    with pytest.raises(ValueError, match="four plain forms"):
        summed.evaluate(30, proof=64, proof_table=True)
    env.terminate()
