"""The exact searches in limited-discrepancy order on one MI355X (include/tpl_learn.h's rule, tpl_placement_exact_limited; the kernels
of csrc/learn/*_limited.hip; T.prove_configs_limited, T.window_prove_limited, T.ProofPolicy(discrepancy=)).  Every output buffer is
guard-framed and filled with 0xA5 before each launch, so a lane that skips a write shows.

  1. IDENTITY: every new kernel at first_limit = 65,535 writes its twin's outputs byte for byte, and limit = 65,535 where a search ran:
     the root kernels on the small games and the generated cases at caps 1, 7, 256 and 4,000 with 12 and 14 weights; the window kernels
     on an environment of 203 boards stepped to moves 0, 3, 9, 10 and 13 with finished boards and a skip mask; the table kernels in the
     four forms with a random table;
  2. THE MIRROR, byte for byte in all seven outputs (tests/golden/exact_limited_mirror.npz, pinned to the mirror by
     tests/test_exact_limited_cpu.py): first_limit 0, 1, 3, both growths, the four caps, n = 1, 33 and the full counts, the small games,
     a game of 254 moves; the window and table kernels against the mirror run here at small caps;
  3. proofs outside the mirror: where the plain and the limited kernel both proved, they agree, and every limited solution played move
     by move on BatchedTetris ends won after exactly solution_len moves;
  4. the gain: the carved case at 4,000 nodes gives the mirror's counts, at least 20 proved where tpl_placement_exact proves 12;
  5. ProofPolicy(discrepancy="add") on a tight pool of 256 boards: an episode that held a verdict 1 ends won.
"""
import functools
import sys

import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import GOLDEN, load_golden
from learn_ref import decode_state
from test_learn_range_gpu import Framed, _check, _stream
from test_learner_gpu import _np
from test_solve_cpu import CW

sys.path.insert(0, GOLDEN)
import make_golden_exact as G  # noqa: E402
import make_golden_exact_limited as GL  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOP = 65535
PLAIN = dict(G.cases())
CASES = dict(GL.cases())
ROOT_OUT = dict(solved=np.uint8, proved=np.uint8, solution_len=np.int32, actions=np.uint8, bound=np.int32, nodes=np.uint32, limit=np.int32)
WINDOW_OUT = dict(solved=np.uint8, proved=np.uint8, solution_len=np.int32, plan=np.uint8, bound=np.int32, nodes=np.uint32, limit=np.int32,
                  horizon=np.uint8, verdict=np.uint8)
AVOID = np.array([-50, -100, -100, -1, -1, 0, -1, 0, 0, 0, 0, 0], np.float32)      # keeps boards running: test_window_gpu's player
WL, WM, WN = 5, 16, 203
SNAPS = (0, 3, 9, 10, 13)


def _m():
    return T._learn_lib


def _frames(arrays):
    out = []
    for seed, x in enumerate(arrays):
        x = np.array(x, order="C")                          # a copy: a fixture's array may be read-only
        f = Framed(x.nbytes, seed + 1)
        f.inner().copy_(torch.from_numpy(x.view(np.uint8).reshape(-1)))
        out.append(f)
    return out


def _outputs(kinds, n, width, limited):
    names = [k for k in kinds if limited or k != "limit"]
    size = lambda k: n * width if k in ("actions", "plan") else n * np.dtype(kinds[k]).itemsize
    out = {k: Framed(size(k), 20 + j) for j, k in enumerate(names)}
    for f in out.values():
        f.inner().fill_(0xA5)
    return names, out


def _collect(kinds, names, out, frames, n, width, what):
    for f in list(out.values()) + frames:
        f.assert_canary(what)
    got = {k: out[k].host().view(kinds[k]).copy() for k in names}
    for k in ("actions", "plan"):
        if k in got:
            got[k] = got[k].reshape(n, width)
    return got


def _order_arguments(order):
    """The arguments between M and max_nodes: a weight row (12, or 14 in a row of 16 with NaN behind) or ("table", int32 array)."""
    if isinstance(order, tuple):
        return [order[1]], lambda f: [f.ptr(), int(order[1].shape[0]), 1.0, 0.0, 0.0, 1.0]
    w = np.asarray(order, np.float32)
    buf = w if w.shape[0] == 12 else np.concatenate([w, np.full(2, np.nan, np.float32)])
    return [buf], lambda f: [f.ptr(), 0.0]


def _entry(stem, order, limited):
    m = _m()
    if isinstance(order, tuple):
        return getattr(m.lib(), {"exact": "tpl_ntuple_exact", "window_prove": "tpl_ntuple_window_prove"}[stem] + ("_limited" if limited else ""))
    return m.entry(stem + ("_limited" if limited else ""), len(order))


def _root(rows, pieces, L, M, order, cap, shortest=True, rule=None):
    """A root kernel -- the plain one, or with rule = (first_limit, growth) the limited one -- through guard-framed buffers."""
    n = rows.shape[0]
    extra, tail = _order_arguments(order)
    frames = _frames([np.ascontiguousarray(rows, np.uint16), np.ascontiguousarray(pieces, np.uint8)] + extra)
    names, out = _outputs(ROOT_OUT, n, M, rule is not None)
    args = [frames[0].ptr(), frames[1].ptr(), n, L, M] + tail(frames[2]) + [int(cap), int(shortest)] + (list(rule) if rule else [])
    _check(_entry("exact", order, rule is not None)(*args, *(out[k].ptr() for k in names), _stream()))
    return _collect(ROOT_OUT, names, out, frames, n, M, (L, M, n, cap, rule))


def _window(a, b, L, M, order, cap, skip=None, rule=None):
    n = a.shape[0]
    extra, tail = _order_arguments(order)
    frames = _frames([a, b] + extra + ([np.ascontiguousarray(skip, np.uint8)] if skip is not None else []))
    names, out = _outputs(WINDOW_OUT, n, 12, rule is not None)
    args = [frames[0].ptr(), frames[1].ptr(), n, L, M] + tail(frames[2]) + [int(cap)] + (list(rule) if rule else []) + \
        [frames[3].ptr() if skip is not None else None]
    _check(_entry("window_prove", order, rule is not None)(*args, *(out[k].ptr() for k in names), _stream()))
    return _collect(WINDOW_OUT, names, out, frames, n, 12, (L, M, n, cap, rule))


def _bytes_equal(got, want, names, what):
    for name in names:
        ref = np.ascontiguousarray(want[name])
        assert got[name].dtype == ref.dtype and got[name].shape == ref.shape, (what, name, got[name].dtype, ref.dtype, got[name].shape, ref.shape)
        bad = np.argwhere(got[name].view(np.uint8) != ref.view(np.uint8))
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())


def _tables():
    m = _m()
    rng = np.random.default_rng(11)
    return {form: rng.integers(-(1 << 20), 1 << 20, m.ntuple_entries_of(form)).astype(np.int32) for form in m.NTUPLE_EXACT_FORMS}


@functools.lru_cache(maxsize=None)
def boards():
    """The planes an environment of 203 boards of the game (5, 16) went through, copied at moves 0, 3, 9, 10, 13 and at the end, when
    every board is finished; a launch takes 203 of them with a stride, so it mixes the move counters with finished boards."""
    g = load_golden("carved_L5_M20.npz")
    env = T.BatchedTetris(WL, WM, WN, device=DEV, seed=3, auto_reset=False)
    env.load_configs(g["rows"][:16], np.ascontiguousarray(g["pieces"][:16, :WM + 1]))
    env.reset()
    player = T.HeuristicPolicy(env, AVOID)
    a, b = [], []
    for t in range(WM + 1):
        if t in SNAPS or t == WM:
            pa, pb = env.raw_planes()
            a.append(_np(pa).view(np.uint32)); b.append(_np(pb).view(np.uint32))
        if t < WM:
            env.step(player.act(), observe=False)
    env.terminate()
    a, b = np.concatenate(a), np.concatenate(b)
    pick = (np.arange(WN) * 37 + 5) % a.shape[0]
    a, b = np.ascontiguousarray(a[pick]), np.ascontiguousarray(b[pick])
    s = decode_state(a, b)
    assert {0, 3, 9, 10, 13} <= set(s["moves"][s["state"] == 0].tolist()) and (s["state"] != 0).sum() >= 8
    return a, b, s, (np.arange(WN) % 5 == 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("key", [k for k, a in PLAIN.items() if k.startswith(("small_", "cfg_")) and a["spare_weight"] == 0.0])
def test_a_root_kernel_at_the_largest_first_limit_writes_its_twins_outputs(key):
    a = PLAIN[key]
    rows, pieces = G.inputs(a)
    w = G.weights()[a["F"]]
    plain = _root(rows, pieces, a["L"], a["M"], w, a["max_nodes"], a["shortest"])
    for growth in (0, 1):
        got = _root(rows, pieces, a["L"], a["M"], w, a["max_nodes"], a["shortest"], (TOP, growth))
        _bytes_equal(got, plain, G.NAMES, (key, growth))
        assert np.array_equal(got["limit"], np.where(plain["bound"] <= a["M"], TOP, 0).astype(np.int32)), key


@pytest.mark.parametrize("count", (12, 14))
@pytest.mark.parametrize("cap", (1, 64, 1024))
def test_a_window_kernel_at_the_largest_first_limit_writes_its_twins_outputs(cap, count):
    a, b, s, skip = boards()
    w = CW if count == 12 else np.array(T.DELLACHERIE_WEIGHTS, np.float32)
    for mask in (None, skip):
        plain = _window(a, b, WL, WM, w, cap, mask)
        got = _window(a, b, WL, WM, w, cap, mask, (TOP, 1))
        _bytes_equal(got, plain, [k for k in WINDOW_OUT if k != "limit"], (cap, count, mask is not None))
        searched = (plain["verdict"] != 0) & (plain["bound"] <= plain["horizon"])
        assert searched.any() and (~searched).any() and np.array_equal(got["limit"], np.where(searched, TOP, 0).astype(np.int32))
        assert (plain["nodes"][~searched] == 0).all()


@pytest.mark.parametrize("form", ("2x4", "3x3", "feat", "feat+spare"))
def test_the_table_kernels_at_the_largest_first_limit_write_their_twins_outputs(form):
    order = ("table", _tables()[form])
    rows, pieces = G.inputs(PLAIN["cfg_L3_M8_c256"])
    for cap in (7, 256):
        plain = _root(rows, pieces, 3, 8, order, cap)
        got = _root(rows, pieces, 3, 8, order, cap, True, (TOP, 0))
        _bytes_equal(got, plain, G.NAMES, (form, cap))
        assert (got["limit"][plain["bound"] <= 8] == TOP).all() and (got["limit"][plain["bound"] > 8] == 0).all()
    a, b, s, skip = boards()
    plain = _window(a, b, WL, WM, order, 64, skip)
    got = _window(a, b, WL, WM, order, 64, skip, (TOP, 0))
    _bytes_equal(got, plain, [k for k in WINDOW_OUT if k != "limit"], form)
    searched = (plain["verdict"] != 0) & (plain["bound"] <= plain["horizon"])
    assert np.array_equal(got["limit"], np.where(searched, TOP, 0).astype(np.int32))


# ------------------------------------------------------------------------------------------------ 2. the mirror
def _recorded(key):
    g = load_golden("exact_limited_mirror.npz")
    return {name: g[f"{key}_{name}"] for name in GL.NAMES}


def _run(key, pick=None):
    a = CASES[key]
    rows, pieces = G.inputs(a)
    if pick is not None:
        rows, pieces = rows[pick], pieces[pick]
    return _root(rows, pieces, a["L"], a["M"], G.weights()[a["F"]], a["max_nodes"], a["shortest"], (a["first_limit"], a["growth"]))


@pytest.mark.parametrize("key", list(CASES))
def test_the_limited_root_kernels_are_the_mirror_byte_for_byte_in_all_seven_outputs(key):
    got = _run(key)
    _bytes_equal(got, _recorded(key), GL.NAMES, key)
    cap = CASES[key]["max_nodes"]
    assert (got["nodes"] <= cap).all() and (got["nodes"][got["proved"] == 0] == cap).all() and (got["solved"] <= got["proved"]).all()


@pytest.mark.parametrize("n", (1, 33))
def test_a_launch_of_one_and_of_thirty_three_configurations_is_the_mirrors(n):
    for key in ("cfg_L3_M8_c256_k0_g0", "cfg_L3_M8_c4000_k1_g1", "cfg_L3_M8_c7_k3_g0"):
        want = {name: x[:n] for name, x in _recorded(key).items()}
        _bytes_equal(_run(key, np.arange(n)), want, GL.NAMES, (key, n))


@pytest.mark.parametrize("rule", ((0, 0), (1, 1), (3, 0)))
def test_the_limited_window_and_table_kernels_are_the_mirrors_run_here(rule):
    m = _m()
    a, b, s, skip = boards()
    n = 48                                                     # the mirror runs here: a launch it finishes in seconds
    fields = [s[k][:n].astype(np.int64) for k in ("lines", "moves", "state")]
    names = [k for k in WINDOW_OUT]
    for count, cap in ((12, 64), (14, 7)):
        w = CW if count == 12 else np.array(T.DELLACHERIE_WEIGHTS, np.float32)
        got = _window(a[:n], b[:n], WL, WM, w, cap, skip[:n], rule)
        want = m.placement_window_prove_limited(s["rows"][:n], *fields, s["window"][:n], WL, WM, w, cap, rule[0], rule[1], skip=skip[:n])
        _bytes_equal(got, want, names, ("window", rule, count))
    table = _tables()["feat+spare"]
    got = _window(a[:n], b[:n], WL, WM, ("table", table), 64, skip[:n], rule)
    want = m.ntuple_window_prove_limited(s["rows"][:n], *fields, s["window"][:n], WL, WM, table, 64, rule[0], rule[1], skip=skip[:n])
    _bytes_equal(got, want, names, ("table window", rule))
    rows, pieces = G.inputs(PLAIN["cfg_L3_M8_c256"])
    for form in ("2x4", "feat"):
        table = _tables()[form]
        got = _root(rows[:16], pieces[:16], 3, 8, ("table", table), 256, True, rule)
        want = dict(zip(GL.NAMES, m.ntuple_exact_limited(rows[:16], pieces[:16], 3, 8, table, 256, rule[0], rule[1])))
        _bytes_equal(got, want, GL.NAMES, ("table root", form, rule))


# ------------------------------------------------------------------------------------------------ 3. and 4. proofs and the gain
def _play(rows, pieces, L, M, actions):
    """Configuration i on board i, the actions played column by column: (state, moves) of every board at the end."""
    n = rows.shape[0]
    env = T.BatchedTetris(L, M, n, device=DEV, seed=1, auto_reset=False, assign="sequential", config_pool=(rows, pieces))
    env.reset()
    acts = torch.as_tensor(actions).to(DEV)
    length = (acts != 255).sum(dim=1)
    acts = torch.where(acts == 255, torch.zeros_like(acts), acts).contiguous()
    for j in range(int(length.max())):
        env.step(acts[:, j].contiguous())
    state = {k: _np(v) for k, v in env.packed_state().items()}
    env.terminate()
    return state["state"].astype(np.int64), state["moves"].astype(np.int64)


@pytest.mark.parametrize("growth", (0, 1))
def test_the_carved_case_gives_the_mirrors_counts_and_every_limited_solution_wins_on_the_environment(growth):
    rows, pieces, sol_len, L, M = G.carved_inputs()
    want = _recorded(f"carved_g{growth}")
    proved_plain = proved = 0
    for budget, idx in G.carved_groups(sol_len):
        r, p = rows[idx], np.ascontiguousarray(pieces[idx, :budget + 1])
        plain = _root(r, p, L, budget, T.CLASSICAL_WEIGHTS, G.CARVED_NODES)
        got = _root(r, p, L, budget, T.CLASSICAL_WEIGHTS, G.CARVED_NODES, True, (0, growth))
        for name in GL.NAMES:
            ref = want[name][idx, :budget] if name == "actions" else want[name][idx]
            assert np.array_equal(got[name], ref), (budget, name)
        both = (plain["proved"] == 1) & (got["proved"] == 1)
        for name in ("solved", "solution_len", "bound"):
            assert np.array_equal(plain[name][both], got[name][both]), (budget, name)
        assert (got["proved"][plain["proved"] == 1] == 1).all()        # here every plain proof is kept (no rule promises it)
        won = np.flatnonzero(got["solved"] == 1)
        if won.size:
            state, moves = _play(r[won], p[won], L, budget, got["actions"][won])
            assert (state == 1).all() and np.array_equal(moves, got["solution_len"][won]), budget
        proved_plain += int(plain["proved"].sum())
        proved += int(got["proved"].sum())
    print("carved, 4,000 nodes: plain proves", proved_plain, "limited", ("add", "double")[growth], proved)
    assert proved_plain == 12 and proved >= 20 and proved == (24, 22)[growth]


def test_where_both_kernels_prove_they_agree_and_limited_solutions_win_on_the_environment():
    for key in ("cfg_L5_M12_c4000", "cfg_L3_M8_c256", "cfg_L4_M6_c4000_owed"):
        a = PLAIN[key]
        rows, pieces = G.inputs(a)
        plain = _root(rows, pieces, a["L"], a["M"], CW, a["max_nodes"])
        for rule in ((0, 0), (0, 1), (2, 0)):
            got = _root(rows, pieces, a["L"], a["M"], CW, a["max_nodes"], True, rule)
            both = (plain["proved"] == 1) & (got["proved"] == 1)
            assert both.sum() >= 16
            for name in ("solved", "solution_len", "bound"):
                assert np.array_equal(plain[name][both], got[name][both]), (key, rule, name)
            won = np.flatnonzero(got["solved"] == 1)
            state, moves = _play(rows[won], pieces[won], a["L"], a["M"], got["actions"][won])
            assert (state == 1).all() and np.array_equal(moves, got["solution_len"][won]), (key, rule)
            lost = (got["proved"] == 1) & (got["solved"] == 0) & (got["nodes"] > 0)
            if "owed" in key:                                  # budgets searched out without a win: the price of the order
                assert lost.any() and (got["nodes"][lost & both] >= plain["nodes"][lost & both]).all()


def test_prove_configs_limited_returns_the_kernels_outputs_and_the_plain_function_is_untouched():
    key = "cfg_L5_M12_c256_k1_g1"
    a = CASES[key]
    rows, pieces = G.inputs(a)
    want = _recorded(key)
    out = T.prove_configs_limited(rows, pieces, a["L"], a["M"], "double", 1, max_nodes=256, device=DEV)
    assert set(out) == {"solved", "proved", "solution_len", "actions", "solution", "bound", "nodes", "optimal", "unwinnable", "limit"}
    assert out["limit"].dtype == torch.int32 and tuple(out["limit"].shape) == (rows.shape[0],)
    for name in GL.NAMES:
        assert np.array_equal(_np(out[name]).astype(want[name].dtype), want[name]), name
    plain = T.prove_configs(rows, pieces, a["L"], a["M"], max_nodes=256, device=DEV)
    none = T.prove_configs_limited(rows, pieces, a["L"], a["M"], None, max_nodes=256, device=DEV)
    top = T.prove_configs_limited(rows, pieces, a["L"], a["M"], "add", 8382, max_nodes=256, device=DEV)
    assert "limit" not in plain and set(none) == set(plain)
    for name in plain:
        assert torch.equal(plain[name], none[name]) and torch.equal(plain[name], top[name]), name
    table = torch.from_numpy(_tables()["feat"]).to(DEV)
    plain = T.ntuple_prove_configs(rows, pieces, a["L"], a["M"], table, max_nodes=256, device=DEV)
    top = T.ntuple_prove_configs_limited(rows, pieces, a["L"], a["M"], table, "double", TOP, max_nodes=256, device=DEV)
    low = T.ntuple_prove_configs_limited(rows, pieces, a["L"], a["M"], table, max_nodes=256, device=DEV)
    for name in plain:
        assert torch.equal(plain[name], top[name]), name
    both = plain["proved"] & low["proved"]
    assert both.any() and torch.equal(plain["solution_len"][both], low["solution_len"][both]) and low["limit"].max() > 0


# ------------------------------------------------------------------------------------------------ 5. the policy
def test_a_limited_proof_policy_wins_every_episode_that_held_a_verdict_1():
    g = load_golden("carved_L5_M20.npz")
    M = int(np.median(g["sol_len"]))                           # the budget the fixture's own solutions give: 7
    rows, pieces = T.tighten_pool(g["rows"], g["pieces"], np.ones(g["rows"].shape[0], bool), g["sol_len"], M)
    n, cap = 256, 64
    env = T.BatchedTetris(5, M, n, device=DEV, seed=5, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=(rows, pieces))
    env.reset()
    base = T.HeuristicPolicy(env, CW)
    policy = T.ProofPolicy(env, base, max_nodes=cap, discrepancy="add")
    assert type(policy) is T.LimitedProofPolicy and type(T.ProofPolicy(env, base, max_nodes=cap)) is T.ProofPolicy
    tabled = T.ProofPolicy(env, base, max_nodes=cap, table=torch.from_numpy(_tables()["feat"]).to(DEV), discrepancy="double", first_limit=1)
    assert type(tabled) is T.LimitedProofPolicy and tabled.table is not None and tabled._limited == (1, 1)
    action = torch.empty(n, dtype=torch.uint8, device=DEV)
    verdict = torch.empty(n, dtype=torch.uint8, device=DEV)
    reward = torch.empty(n, dtype=torch.float32, device=DEV)
    done = torch.empty(n, dtype=torch.uint8, device=DEV)
    held = np.zeros(n, bool)
    proved_episodes = lost_proofs = plan_moves = 0
    for t in range(3 * M):
        own = _np(base.act()).copy()
        probe = T.window_prove_limited(env, "add", max_nodes=cap)
        assert policy.act(out=action, verdict=verdict) is action
        v, played, act = _np(verdict), _np(policy.played), _np(action)
        assert np.array_equal(v, _np(probe["verdict"])) and np.array_equal(_np(policy.limit), _np(probe["limit"])), t
        found = v == 1
        assert np.array_equal(act[found], _np(probe["plan"])[found, 0]), t     # the plan's move where there is one
        assert np.array_equal(act[~played], own[~played]) and played[found].all(), t      # the base's move elsewhere
        held |= found
        plan_moves += int(played.sum())
        env.step_into(action, reward, done)
        d, r = _np(done).astype(bool), _np(reward)
        proved_episodes += int((d & held).sum())
        lost_proofs += int((d & held & (r != 1.0)).sum())
        held &= ~d
    tabled.act(out=action)
    assert _np(tabled.limit).max() >= 1
    print("episodes that held a verdict 1:", proved_episodes, "not won:", lost_proofs, "plan moves", plan_moves, policy.stats())
    assert proved_episodes >= n and lost_proofs == 0
    env.terminate()


def test_the_evaluate_hook_builds_a_limited_policy_only_when_asked(monkeypatch):
    g = load_golden("carved_L5_M20.npz")
    rows, pieces = T.tighten_pool(g["rows"], g["pieces"], np.ones(g["rows"].shape[0], bool), g["sol_len"], 7)
    seen = []
    stats = T.solve.ProofPolicy.stats
    monkeypatch.setattr(T.solve.ProofPolicy, "stats", lambda self: (seen.append(type(self)), stats(self))[1])
    got = []
    for order in ({}, dict(proof_discrepancy="add"), dict(proof_discrepancy="double")):
        env = T.BatchedTetris(5, 7, 64, device=DEV, seed=5, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=(rows, pieces))
        got.append(T.evaluate_heuristic(env, CW, None, 21, proof=64, **order))
        env.terminate()
    assert seen == [T.ProofPolicy, T.LimitedProofPolicy, T.LimitedProofPolicy]      # a default call is the class it always was
    assert all(x["proof"]["win"] > 0 and x["episodes"][0] > 0 for x in got)
