"""CPU-side checks of the window proof search ordered by an n-tuple table (include/tpl_learn.h's rule under tpl_ntuple_window_prove;
_learn_lib.ntuple_window_prove; solve.py's ntuple_window_prove and ProofPolicy(table=); csrc/learn/ntuple_window.hip).

The oracle is COMPOSITION, as the rule is: a running board with horizon H is the configuration (rows, [window entries 0 .. H - 1, 0]) of
the game (L - lines, H), searched by the existing _learn_lib.ntuple_exact; and, beside it, INDEPENDENCE OF THE ORDER: what a finished
search says is what _learn_lib.placement_window_prove says under the classical weights.  The cases are
tests/golden/make_golden_ntuple_window.py's: make_golden_window's states under make_golden_ntuple_exact's tables.

  1. the mirror is ntuple_exact on the reset boards, (5, 10) with H = rem = 10 and (5, 20) with H = 12 < rem, five tables;
  2. mid-game boards at counters 1, 9, 10, 11, 19 and finished ones: all four verdicts under every table, the verdict formula, the cap,
     the skip mask, gamma and reward, the table of ties;
  3. independence of the order against placement_window_prove; the table really orders;
  4. every verdict-1 plan replays on the C oracle to a win after exactly solution_len moves;
  5. verdict 2 by exhaustive enumeration;
  6. the Python refusals, every refusal of the entry, the header, the unit;  7. the resources;  8. the sanitizers;  9. the record.
"""
import ctypes
import functools
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_solve_cpu import CW, _first_winning_ply, _replay

import tetris_piclim as T

sys.path.insert(0, GOLDEN)
import make_golden_ntuple_window as G  # noqa: E402  -- the cases
import make_golden_window as W  # noqa: E402  -- the states
import make_golden_ntuple_exact as N  # noqa: E402  -- the tables

SIX = ("solved", "proved", "solution_len", "plan", "bound", "nodes")
# the classical mirror's recorded outputs (window_mirror.npz, pinned by test_window_cpu.py) where states and cap are a case of its own
RECORDED = {("root_M10", 1024): "root_M10", ("root_M20", 1024): "root_M20", ("mid", 1024): "mid", ("loss_small", 1 << 16): "loss_small",
            ("loss_owed", 1 << 14): "loss_owed"}


def _m():
    return T._learn_lib


@functools.lru_cache(maxsize=None)
def mirror(key):
    """The mirror as it stands on a case of the golden maker.  Computed once; nobody writes to it."""
    return G.run_case(_m(), key)


@functools.lru_cache(maxsize=None)
def classical(states, cap):
    """placement_window_prove under the classical weights on the states of a case at its cap, unskipped."""
    if (states, cap) in RECORDED:
        rec = load_golden("window_mirror.npz")
        return {name: rec[f"{RECORDED[(states, cap)]}_{name}"] for name in W.NAMES}
    s = G.STATES[states]()
    return _m().placement_window_prove(s["rows"], s["lines"], s["moves"], s["state"], s["window"], s["L"], s["M"], CW, cap)


def keys_of(states, tables=None):
    return [k for k, c in G.CASES.items() if c["states"] == states and (tables is None or c["table"] in tables)]


# ------------------------------------------------------------------------------------------------ 1. the reset boards
@pytest.mark.parametrize("key", keys_of("root_M10", G.FIVE) + [k for k in keys_of("root_M20", G.FIVE) if not k.endswith("_c1")])
def test_the_mirror_is_ntuple_exact_on_the_reset_boards(key):
    m, g, case = _m(), load_golden(W.FIXTURE), G.CASES[key]
    M = 10 if case["states"] == "root_M10" else 20
    H = min(12, M)
    got = mirror(key)
    assert (got["horizon"] == H).all() and (got["known"] == 12).all()
    lists = np.concatenate([g["pieces"][:W.COUNT, :H], np.zeros((W.COUNT, 1), np.uint8)], axis=1)
    want = m.ntuple_exact(g["rows"][:W.COUNT], lists, W.L5, H, G.table_of(key), case["max_nodes"], True)
    for name, ref in zip(SIX, want):
        mine = got[name][:, :H] if name == "plan" else got[name]
        assert mine.dtype == ref.dtype and np.array_equal(mine, ref), name
    assert (got["plan"][:, H:] == 255).all()
    rest = got["solved"] == 0
    assert rest.any() and (~rest).any()
    assert (got["nodes"][rest] == case["max_nodes"]).all() and (got["proved"][rest] == 0).all()      # capped: nothing is proved
    assert (got["verdict"][rest] == m.WINDOW_OPEN).all() and (got["verdict"][~rest] == m.WINDOW_WIN).all()
    assert np.array_equal(got["solution_len"][~rest], g["sol_len"][:W.COUNT][~rest])                  # the fixture's shortest


# ------------------------------------------------------------------------------------------------ 2. mid-game boards
@pytest.mark.parametrize("key", [k for k in keys_of("mid") + keys_of("mid10") if not k.endswith(("_c1", "_skip"))])
def test_mid_game_boards_meet_every_verdict_and_the_verdict_formula(key):
    m = _m()
    s, got, case = G.states_of(key), mirror(key), G.CASES[key]
    n, M = s["rows"].shape[0], s["M"]
    running = (s["state"] == 0) & (s["lines"] < s["L"]) & (s["moves"] < M)
    known = 12 - s["moves"] % 10
    rem = np.where(running, M - s["moves"], 0)
    H = np.minimum(known, rem)
    assert np.array_equal(got["known"], known.astype(np.uint8)) and np.array_equal(got["horizon"], H.astype(np.uint8))
    verdict = np.where(~running, 0, np.where(got["solved"] == 1, 1, np.where((got["proved"] == 1) & (H == rem), 2, 3)))
    assert np.array_equal(got["verdict"], verdict)
    assert set(np.unique(got["verdict"]).tolist()) == {0, 1, 2, 3}                            # under every table
    if case["states"] == "mid":
        assert running.sum() == len(W.GROUPS) * W.COUNT and sorted(set(s["moves"][running].tolist())) == list(W.COUNTERS)
    for name, value in (("solved", 0), ("proved", 1), ("solution_len", 0), ("bound", 0), ("nodes", 0), ("horizon", 0), ("verdict", 0)):
        assert (got[name][~running] == value).all(), name
    assert (got["plan"][~running] == 255).all()
    # per (lines, H) group the six shared outputs are ntuple_exact's on [q[:H], 0] in the game (L - lines, H); searched a second time
    # only where that is cheap -- the feature forms at 64 nodes, gamma and the ties among them
    q = m.window_entries(s["window"])
    again = case["max_nodes"] <= 64 and case["table"] in ("budget", "feat", "ties")
    for lines, h in sorted({(int(a), int(b)) for a, b in zip(s["lines"][running], H[running])} if again else ()):
        idx = np.flatnonzero(running & (s["lines"] == lines) & (H == h))
        lists = np.concatenate([q[idx, :h], np.zeros((idx.size, 1), np.int64)], axis=1)
        want = m.ntuple_exact(s["rows"][idx], lists, s["L"] - lines, h, G.table_of(key), case["max_nodes"], True, case["gamma"], case["reward"])
        for name, ref in zip(SIX, want):
            mine = got[name][idx][:, :h] if name == "plan" else got[name][idx]
            assert np.array_equal(mine, ref), (name, lines, h)
        assert (got["plan"][idx][:, h:] == 255).all()
    short = running & (H < rem) & (got["solved"] == 0) & (got["proved"] == 1)                 # searched out with pieces still unknown
    assert (short.any() or case["states"] == "mid10") and (got["verdict"][short] == m.WINDOW_OPEN).all()      # in (5, 10) H == rem throughout
    assert (got["nodes"] <= case["max_nodes"]).all() and (got["nodes"][got["proved"] == 0] == case["max_nodes"]).all()


def test_the_tables_give_the_verdict_counts_the_rule_was_measured_with():
    """The rule's author measured [4, 61, 16, 19] on `mid` at 1,024 nodes under the linear table and all four hashed ones.  This mirror
    gives that under four of the five.  Under the hashed "feat" table it gives [4, 58, 16, 22]: three boards that the other orders
    prove won run into the cap -- verdict 3 for 1, which a worse order may do and which claims nothing (the independence test holds
    on the 94 boards that table proves)."""
    counts = lambda key: np.bincount(mirror(key)["verdict"], minlength=4).tolist()
    for tag in ("linear", "budget", "3x3", "2x4"):
        assert counts(f"mid_{tag}_c1024") == [4, 61, 16, 19], tag
    assert counts("mid_feat_c1024") == [4, 58, 16, 22]
    feat, budget = mirror("mid_feat_c1024"), mirror("mid_budget_c1024")
    differ = feat["verdict"] != budget["verdict"]
    assert differ.sum() == 3 and (feat["verdict"][differ] == 3).all() and (feat["nodes"][differ] == 1024).all()
    assert counts("mid_budget_c64") == [4, 57, 16, 23] and counts("mid_3x3_c64") == [4, 55, 16, 25]


@pytest.mark.parametrize("tag", ("budget", "feat", "3x3", "2x4"))
def test_the_cap_gives_verdict_3_and_a_larger_one_takes_no_proof_back(tag):
    m = _m()
    one, full = mirror(f"mid_{tag}_c1"), mirror(f"mid_{tag}_c64")
    searched = full["nodes"] > 1
    assert searched.any()
    assert (one["verdict"][searched] == m.WINDOW_OPEN).all() and (one["proved"][searched] == 0).all()
    assert (one["nodes"][searched] == 1).all() and (one["plan"][searched] == 255).all() and (one["solution_len"][searched] == 0).all()
    decided = one["proved"] == 1                               # what one node (or none) decides stays as it is
    for name in W.NAMES:
        assert np.array_equal(one[name][decided], full[name][decided]), name
    for name in ("bound", "horizon", "known"):
        assert np.array_equal(one[name], full[name]), name


def test_a_skipped_board_is_not_searched_and_keeps_bound_and_horizon():
    got, full = mirror("mid_budget_skip"), mirror("mid_budget_c1024")
    skip = np.arange(got["verdict"].size) % 3 == 0
    for name, value in (("solved", 0), ("proved", 0), ("solution_len", 0), ("nodes", 0), ("verdict", 0)):
        assert (got[name][skip] == value).all(), name
    assert (got["plan"][skip] == 255).all()
    for name in ("bound", "horizon", "known"):
        assert np.array_equal(got[name], full[name]), name
    for name in W.NAMES:
        assert np.array_equal(got[name][~skip], full[name][~skip]), name


def test_gamma_the_reward_and_the_table_of_ties_reach_the_order():
    plain, other, ties = mirror("mid_budget_c64"), mirror("mid_budget_gamma"), mirror("mid_ties_c64")
    assert not np.array_equal(plain["nodes"], other["nodes"])                      # gamma 0.5, reward (1, 10, -1): another order
    assert not np.array_equal(plain["nodes"], ties["nodes"])
    # the zero table with reward (0, 0, 0): every key ties and the order is b alone -- the order of the weight form under twelve zero
    # weights, so the two mirrors, which share no value code, write the same nine arrays
    s = W.mid_states()
    zero = _m().placement_window_prove(s["rows"], s["lines"], s["moves"], s["state"], s["window"], s["L"], s["M"], np.zeros(12, np.float32), 64)
    assert (ties["verdict"] == 1).sum() >= 32 and (ties["nodes"] == 64).any()
    for name in W.NAMES:
        assert np.array_equal(ties[name], zero[name]), name


# ------------------------------------------------------------------------------------------------ 3. independence of the order
@pytest.mark.parametrize("key", list(G.CASES))
def test_what_a_finished_search_says_does_not_depend_on_the_order(key):
    case, got = G.CASES[key], mirror(key)
    ref = classical(case["states"], case["max_nodes"])
    both = (got["proved"] == 1) & (ref["proved"] == 1)
    for name in ("solved", "solution_len", "bound", "verdict"):
        assert np.array_equal(got[name][both], ref[name][both]), name
    out = both & (got["solved"] == 0)                          # searched out without a win: every running board once, in any order
    assert np.array_equal(got["nodes"][out], ref["nodes"][out])
    for name in ("bound", "horizon", "known"):                 # nothing of the frame depends on the order
        assert np.array_equal(got[name], ref[name]), name
    if case["states"] == "mid" and case["max_nodes"] == 1024 and case["skip"] is None:
        assert both.sum() >= 90, int(both.sum())
    if case["states"] == "loss_owed":
        assert both.sum() == 16 and out.sum() == 12 and (got["nodes"][out] > 1).any()


def test_the_table_really_orders_the_search():
    hashed, linear = mirror("root_M10_budget_c1024"), mirror("root_M10_linear_c1024")
    assert int(hashed["nodes"].sum()) == 6414 and int(linear["nodes"].sum()) == 5088
    ref = classical("root_M10", 1024)
    both = (hashed["verdict"] == 1) & (ref["verdict"] == 1)
    assert both.sum() >= 9 and (hashed["plan"][both] != ref["plan"][both]).any()             # another shortest win, or the same by another path
    assert np.array_equal(hashed["solution_len"][both], ref["solution_len"][both])


# ------------------------------------------------------------------------------------------------ 4. the replay
def test_every_verdict_1_plan_wins_on_the_oracle_after_exactly_its_length(oracle):
    m, g = _m(), load_golden(W.FIXTURE)
    wins = 0
    for key in keys_of("root_M10") + keys_of("root_M20"):
        M = G.states_of(key)["M"]
        got = mirror(key)
        for i in np.flatnonzero(got["verdict"] == m.WINDOW_WIN):
            n = int(got["solution_len"][i])
            assert _replay(oracle, W.L5, M, g["rows"][i], g["pieces"][i, :M + 1], got["plan"][i], n) == (1, n)
            assert (got["plan"][i, n:] == 255).all() and (got["plan"][i, :n] < 40).all()
            wins += 1
    assert wins >= 80
    # mid-game: the real game goes on from the board's own lines and moves with the pieces that follow it in the list
    for key in keys_of("mid") + keys_of("mid10"):
        s, got = G.states_of(key), mirror(key)
        found = np.flatnonzero(got["verdict"] == m.WINDOW_WIN)
        assert found.size >= (7 if s["M"] == 10 else 32) or key.endswith("_c1")
        for i in found:
            n, k, c = int(got["solution_len"][i]), int(s["played"][i]), int(s["config"][i])
            game = oracle.Game(W.L5, s["M"], rows=s["rows"][i], pieces=g["pieces"][c, k:], lines_cleared=int(s["lines"][i]),
                               moves_used=int(s["moves"][i]), state=0)
            for b in got["plan"][i, :n]:
                assert game.state == 0
                game.move(int(b) // 10, int(b) % 10)
            assert game.state == 1 and game.moves_used == int(s["moves"][i]) + n
            assert int(got["bound"][i]) <= n <= int(got["horizon"][i])


# ------------------------------------------------------------------------------------------------ 5. verdict 2
@pytest.mark.parametrize("key", ("loss_small_budget_c65536", "loss_owed_budget_c16384"))
def test_verdict_2_is_a_search_that_ended_at_the_end_of_the_game_and_no_enumeration_finds_a_win(oracle, key):
    m = _m()
    s, got = G.states_of(key), mirror(key)
    L, M = s["L"], s["M"]
    assert (got["horizon"] == M).all() and (got["proved"] == 1).all()                      # H == rem, and nothing was capped
    loss = got["verdict"] == m.WINDOW_LOSS
    by_search = loss & (got["nodes"] >= 1)                       # alive by the bound, dead by geometry
    assert by_search.sum() >= 2 and (got["bound"][by_search] <= M).all()
    assert np.array_equal(loss, got["solved"] == 0) and (got["verdict"][~loss] == m.WINDOW_WIN).all()
    lists = np.concatenate([s["pieces"][:, :M], np.zeros((loss.size, 1), np.uint8)], axis=1)
    want = m.ntuple_exact(s["rows"], lists, L, M, G.table_of(key), G.CASES[key]["max_nodes"])
    for name, ref in zip(SIX, want):
        assert np.array_equal(got[name][:, :M] if name == "plan" else got[name], ref), name
    if M <= 3:                                                 # 34^3 sequences a board: the enumeration is affordable
        for i in range(loss.size):
            first = _first_winning_ply(oracle, L, M, s["rows"][i], s["pieces"][i, :M + 1])
            assert first == int(got["solution_len"][i]) and (first == 0) == bool(loss[i]), i
    for i in np.flatnonzero(~loss):
        n = int(got["solution_len"][i])
        assert _replay(oracle, L, M, s["rows"][i], s["pieces"][i, :M + 1], got["plan"][i], n) == (1, n)


# ------------------------------------------------------------------------------------------------ 6. the refusals, the header, the unit
def test_python_refusals_of_the_mirror_the_entry_point_the_policy_and_the_hooks_need_no_gpu():
    import torch
    m = _m()
    s = W.root_states(10)
    n = s["rows"].shape[0]
    zero = N.table("feat+spare", "zero")
    good = dict(rows=s["rows"], lines=s["lines"], moves=s["moves"], state=s["state"], window=s["window"], L=5, M=10, table=zero, max_nodes=4)
    assert sorted(m.ntuple_window_prove(**good)) == sorted(W.NAMES)
    for bad in (dict(L=0), dict(L=251), dict(M=0), dict(M=255), dict(max_nodes=0), dict(max_nodes=True), dict(max_nodes=2.0),
                dict(max_nodes=(1 << 24) + 1), dict(gamma=np.inf), dict(gamma=None), dict(reward=(1.0, np.nan, 0.0)), dict(reward=(1.0, 0.0)),
                dict(table=np.zeros(21504, np.int64)), dict(table=np.zeros(m.NTUPLE_ENTRIES_SUM, np.int32)), dict(table=np.zeros(21503, np.int32)),
                dict(table=np.zeros(m.NTUPLE_ENTRIES_3X3_FEAT, np.int32)), dict(table=np.zeros(m.ntuple_staged_entries_of("3x3"), np.int32)),
                dict(lines=s["lines"][:3]), dict(moves=np.zeros(n)), dict(state=np.full(n, 4)), dict(window=np.full(n, 1 << 36, np.uint64)),
                dict(skip=np.zeros(3)), dict(rows=s["rows"][:0]), dict(lines=np.full(n, 256))):
        with pytest.raises(ValueError):
            m.ntuple_window_prove(**{**good, **bad})
    with pytest.raises(ValueError, match="four plain forms"):
        m.ntuple_window_prove(**dict(good, table=np.zeros(m.NTUPLE_ENTRIES_SUM, np.int32)))
    p = inspect.signature(m.ntuple_window_prove).parameters
    assert list(p) == ["rows", "lines", "moves", "state", "window", "L", "M", "table", "max_nodes", "gamma", "reward", "skip"]
    assert (p["gamma"].default, p["reward"].default, p["skip"].default) == (1.0, (1.0, 0.0, 0.0), None)

    # T.ntuple_window_prove: everything is checked before the environment's state is touched
    env = types.SimpleNamespace(num_envs=4, L=5, M=10, device=torch.device("cpu"))
    table = torch.from_numpy(zero.copy())
    p = inspect.signature(T.ntuple_window_prove).parameters
    assert list(p) == ["env", "table", "gamma", "reward", "max_nodes", "skip"]
    assert (p["gamma"].default, p["reward"].default, p["max_nodes"].default, p["skip"].default) == (1.0, (1.0, 0.0, 0.0), 1 << 12, None)
    for bad in (0, (1 << 24) + 1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_nodes"):
            T.ntuple_window_prove(env, table, max_nodes=bad)
    for bad in (np.inf, np.nan, 1e39):
        with pytest.raises(ValueError, match="gamma must be finite"):
            T.ntuple_window_prove(env, table, gamma=bad)
        with pytest.raises(ValueError, match=r"reward\[2\] must be finite"):
            T.ntuple_window_prove(env, table, reward=(1.0, 0.0, bad))
    for bad in (1.0, (1.0, 0.0), "abc", None):
        with pytest.raises(ValueError, match="reward"):
            T.ntuple_window_prove(env, table, reward=bad)
    for bad in (None, "feat", np.zeros(21504, np.int64), torch.zeros(21504, dtype=torch.float32), torch.zeros((2, 21504), dtype=torch.int32)):
        with pytest.raises(ValueError, match="table must be an int32 tensor"):
            T.ntuple_window_prove(env, bad)
    for entries in (m.NTUPLE_ENTRIES_SUM, m.NTUPLE_ENTRIES_3X3_FEAT, m.ntuple_staged_entries_of("2x4"), 21505, 0):
        for bad in (torch.zeros(entries, dtype=torch.int32), np.zeros(entries, np.int32)):      # a numpy table is uploaded, then checked
            with pytest.raises(ValueError, match="four plain forms") as e:
                T.ntuple_window_prove(env, bad)
            assert all(form in str(e.value) for form in ("'2x4'", "'3x3'", "'feat'", "'feat+spare'"))
    with pytest.raises(ValueError, match="skip must be"):
        T.ntuple_window_prove(env, table, skip=np.zeros(3, bool))
    with pytest.raises(ValueError, match="boards"):
        T.ntuple_window_prove(types.SimpleNamespace(num_envs=0), table)
    assert "proves nothing" in T.ntuple_window_prove.__doc__ and "never written" in T.ntuple_window_prove.__doc__

    # ProofPolicy(table=): one order, one of the four forms
    base = types.SimpleNamespace(act=lambda out=None: out, env=env)
    for bad in (dict(weights=CW), dict(spare_weight=0.5), dict(weights=np.array(T.DELLACHERIE_WEIGHTS))):
        with pytest.raises(ValueError, match="in place of weights and spare_weight"):
            T.ProofPolicy(env, base, table=table, **bad)
    with pytest.raises(ValueError, match="four plain forms"):
        T.ProofPolicy(env, base, table=torch.zeros(m.NTUPLE_ENTRIES_SUM, dtype=torch.int32))
    with pytest.raises(ValueError, match="table must be an int32 tensor"):
        T.ProofPolicy(env, base, table="feat")
    with pytest.raises(ValueError, match="gamma must be finite"):
        T.ProofPolicy(env, base, table=table, gamma=np.inf)
    with pytest.raises(ValueError, match="reward"):
        T.ProofPolicy(env, base, table=table, reward=(1.0, 0.0))
    for bad in (dict(gamma=0.5), dict(reward=(1.0, 10.0, -1.0)), dict(table=None, gamma=0.5)):      # nothing would read them: not ignored
        with pytest.raises(ValueError, match="without table= they are refused"):
            T.ProofPolicy(env, base, **bad)
    class Mine(T.ProofPolicy):                                 # only ProofPolicy itself is switched to the table form
        pass
    with pytest.raises(TypeError):
        Mine(env, base, table=table)
    assert issubclass(T.TableProofPolicy, T.ProofPolicy)
    p = inspect.signature(T.TableProofPolicy.__init__).parameters
    assert list(p) == ["self", "env", "base", "weights", "max_nodes", "spare_weight", "reuse", "table", "gamma", "reward"]
    assert (p["table"].default, p["gamma"].default, p["reward"].default) == (None, 1.0, (1.0, 0.0, 0.0))
    assert "HELD, not copied" in T.TableProofPolicy.__doc__

    # the hooks: proof_table needs proof; True needs a learner of one of the four forms
    assert inspect.signature(T.evaluate_heuristic).parameters["proof_table"].default is None
    assert inspect.signature(T.NTupleLearner.evaluate).parameters["proof_table"].default is False
    with pytest.raises(ValueError, match="needs proof"):
        T.evaluate_heuristic(env, CW, None, 10, proof_table=table)
    with pytest.raises(ValueError, match="per_config"):         # None and False both pass the proof_table check without `proof`
        T.evaluate_heuristic(env, CW, None, 10, per_config=1, proof_table=False)
    source = inspect.getsource(T.evaluate_heuristic)
    assert source.index("proof_table is False") < source.index("needs proof")
    for given in (True, table):
        with pytest.raises(ValueError, match="needs proof"):
            T.NTupleLearner.evaluate(types.SimpleNamespace(), 10, proof_table=given)
    for shape, staged in (("2x4+3x3", False), ("3x3+feat", False), ("2x4", True)):
        fake = types.SimpleNamespace(greedy=types.SimpleNamespace(shape=shape, staged=staged))
        with pytest.raises(ValueError, match="four plain forms") as e:
            T.NTupleLearner.evaluate(fake, 10, proof=64, proof_table=True)
        assert all(form in str(e.value) for form in ("'2x4'", "'3x3'", "'feat'", "'feat+spare'"))
    for name in ("ntuple_window_prove", "TableProofPolicy"):
        assert name in T.__all__ and name in T.solve.__all__ and getattr(T, name) is getattr(T.solve, name)


ENTRY = "tpl_ntuple_window_prove"
KERNELS = ("ntuple_window_kernel", "ntuple_window3_kernel", "ntuple_window_feature_kernel", "ntuple_window_budget_kernel")
ARGS = ["plane_a", "plane_b", "n", "L", "M", "table", "entries", "r_line", "r_win", "r_lose", "gamma", "max_nodes", "skip", "solved",
        "proved", "solution_len", "plan", "bound", "nodes", "horizon", "verdict", "stream"]


def test_every_refusal_of_the_entry_comes_back_as_a_status_without_a_gpu():
    m = _m()
    lib = m.lib()
    fn = lib.tpl_ntuple_window_prove
    assert len(fn.argtypes) == len(ARGS)
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    counts = [m.ntuple_entries_of(form) for form in m.NTUPLE_EXACT_FORMS]
    at_of = ARGS.index
    for entries in counts:
        ok = [fake, fake, 4, 2, 6, fake, entries, 1.0, 0.0, 0.0, 1.0, 100, None] + [fake] * 8 + [None]
        assert len(ok) == len(ARGS)
        required = [a for a in ARGS if a.startswith("plane") or a == "table" or at_of(a) > at_of("skip") and a != "stream"]
        assert len(required) == 11
        cases = [(at_of(a), None, "null") for a in required]
        cases += [(2, 0, "positive"), (2, -3, "positive"), (2, 1 << 31, "2^31"), (2, 1 << 40, "2^31"), (3, 0, "L and M"), (3, 251, "L and M"),
                  (4, 0, "L and M"), (4, 255, "L and M"), (0, fake + 8, "planes must be 16-byte"), (1, fake + 4, "planes must be 16-byte"),
                  (5, fake + 2, "table must be 4-byte"), (at_of("solution_len"), fake + 2, "solution_len must be 4-byte"),
                  (at_of("bound"), fake + 2, "bound must be 4-byte"), (at_of("nodes"), fake + 2, "nodes must be 4-byte"),
                  (11, 0, "max_nodes must be in [1, 16777216]"), (11, -1, "max_nodes must be in"), (11, (1 << 24) + 1, "max_nodes must be in")]
        for at in (7, 8, 9):
            cases += [(at, float("inf"), "r_line, r_win and r_lose must be finite"), (at, float("nan"), "must be finite")]
        cases += [(10, float("inf"), "gamma must be finite"), (10, float("-inf"), "gamma must be finite"), (10, float("nan"), "gamma must be finite")]
        for at, value, what in cases:
            args = list(ok)
            args[at] = value
            assert fn(*args) < 0 and ENTRY + ":" in err() and what in err(), (ARGS[at], value, err())
        for skip in (None, fake + 1):                          # the mask is optional and has no alignment; the largest arguments pass
            args = list(ok)
            args[2], args[3], args[4], args[11], args[12], args[5] = (1 << 31) - 1, 250, 254, 1 << 24, skip, fake + 2
            assert fn(*args) < 0 and "table must be 4-byte" in err()
    # any other entry count is refused, FIRST, with tpl_ntuple_exact's message
    others = [0, -1, 1, m.NTUPLE_ENTRIES_SUM, m.NTUPLE_ENTRIES_3X3_FEAT, 21505, 1 << 40] + \
        [m.ntuple_staged_entries_of(s) for s in ("2x4", "3x3", "2x4+3x3")]
    twin = lib.tpl_ntuple_exact
    for entries in others:
        for args in ([fake, fake, 4, 2, 6, fake, entries, 1.0, 0.0, 0.0, 1.0, 100, None] + [fake] * 8 + [None],
                     [None, None, 0, 0, 0, None, entries, float("nan"), 0.0, 0.0, float("inf"), 0, None] + [None] * 8 + [None]):
            assert fn(*args) < 0 and ENTRY + ": entries must be" in err(), (entries, err())
            assert all(f'"{form}"' in err() for form in m.NTUPLE_EXACT_FORMS) and all(str(c) in err() for c in counts), err()
            mine = err()
        assert twin(fake, fake, 4, 2, 6, fake, entries, 1.0, 0.0, 0.0, 1.0, 100, 1, fake, fake, fake, fake, fake, fake, None) < 0
        assert err().replace("tpl_ntuple_exact", ENTRY) == mine                                  # the twin's message, word for word


def test_the_header_states_the_rule_and_the_library_exports_the_entry():
    m = _m()
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_\w+)\s*\(", text))
    assert declared == set(m.LEARN_SYMBOLS) and ENTRY in declared
    lib = ctypes.CDLL(m.build_library())
    assert hasattr(lib, ENTRY)
    proto = re.search(r"int %s\((.*?)\);" % ENTRY, text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ARGS
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("tpl_ntuple_window_prove IS tpl_placement_window_prove WITH ONE THING REPLACED", "IS tpl_ntuple_exact's WITH shortest = 1",
                  "q[0], ..., q[H - 1], 0", "in the game (L - lines, H)", "BYTE FOR BYTE what tpl_ntuple_exact writes",
                  "plan is actions padded with 255", "V IS READ AT THE ITERATION'S BUDGET B", "spare = 4 (B - moves') - cells",
                  "NOTHING DEPENDS ON THE ABSOLUTE lines OR moves", "d + 1 < B <= H <= known",
                  "NO VALUE IS EVER READ UNDER A PIECE THE AGENT DOES NOT KNOW", "List entry H (index 12 where H = 12) is a defined 0",
                  "VERDICT 3 PROVES NOTHING ABOUT THE GAME", "ARE INDEPENDENT OF THE TABLE, gamma and the reward",
                  "nodes is independent of the order as well", "refused first, with tpl_ntuple_exact's message"):
        assert words in flat, words
    # a unit of its own: the search loop is duplicated, the parents' units are not part of it; static LDS, no barrier
    units = [os.path.basename(p) for p in m._UNITS]
    assert "ntuple_window.hip" in units and "ntuple_exact.hip" in units and "exact_window.hip" in units
    body = open(os.path.join(m._LEARN_CSRC, "ntuple_window.hip")).read()
    assert "__syncthreads" not in body and "extern __shared__" not in body
    assert '#include "exact' not in body and '#include "ntuple_exact' not in body
    assert '#include "tpl_beam.h"' in body and '#include "tpl_ntuple.h"' in body and "#define TPL_PLACEMENT_BOUND_UNIT" in body
    assert "ntuple_value<S>" in body and "prune_dead<" not in body and body.count("__launch_bounds__(kWindowWave, 8)") == 4
    assert any(p.endswith(os.path.join("learn", "ntuple_window.hip")) for p in m._sources())
    for doc in ("README.md", "DESIGN.md"):
        words = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "ntuple_window_prove" in words and "ProofPolicy(table=" in words, doc


# ------------------------------------------------------------------------------------------------ 7. the resources
def test_the_four_kernels_use_no_scratch_and_fill_a_simd_with_waves():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    num = lambda r, what: int(r[r.index(what) - 1])
    for kernel in KERNELS:
        mine = [r for r in rows if f"{len(kernel)}{kernel}E" in r[-1]]       # the whole mangled name: no name within another
        assert len(mine) == 1, (kernel, [r[-1] for r in rows])
        r = mine[0]
        assert num(r, "scratch") == 0, r
        assert num(r, "vgpr") <= 64, r                                       # eight waves a SIMD by the vector registers: no exception taken
        assert 80 * 12 <= num(r, "lds") <= 160 * 1024 // 32, r               # the stack is static, and 32 waves a CU have theirs


# ------------------------------------------------------------------------------------------------ 8. the sanitizers
def test_host_entry_code_under_address_and_ub_sanitizers(tmp_path):
    """The host side of csrc/learn/ntuple_window.hip (the entry's argument checks) compiled host-only with -fsanitize=address,undefined
    and driven by a stand-alone program over every refusal path.  Nothing is loaded into Python."""
    flags = ["--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
             "-I", os.path.join(ROOT, "include")]
    exe = str(tmp_path / "sanitize_ntuple_window")
    cmd = ["hipcc"] + flags + [os.path.join(_m()._LEARN_CSRC, "ntuple_window.hip"),
                               os.path.join(ROOT, "tests", "c_abi", "sanitize_ntuple_window.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "sanitizer run ok" in res.stdout, res.stdout + res.stderr


# ------------------------------------------------------------------------------------------------ 9. the record
def test_the_recorded_outputs_are_the_mirrors():
    rec = load_golden("ntuple_window_mirror.npz")
    assert sorted(rec.files) == sorted(f"{key}_{name}" for key in G.CASES for name in W.NAMES)
    for key in G.CASES:
        got = mirror(key)
        for name in W.NAMES:
            assert got[name].dtype == rec[f"{key}_{name}"].dtype and np.array_equal(got[name], rec[f"{key}_{name}"]), (key, name)
    got = mirror("root_M10_budget_c1024")
    assert [got[k].dtype for k in W.NAMES] == [np.uint8, np.uint8, np.int32, np.uint8, np.int32, np.uint32, np.uint8, np.uint8, np.uint8]
    assert got["plan"].shape == (W.COUNT, 12) and got["plan"].flags.c_contiguous
