"""CPU-side checks of the exact searches in limited-discrepancy order (include/tpl_learn.h's rule, tpl_placement_exact_limited;
_learn_lib._exact_search(first_limit=, growth=) and the four *_limited mirrors; solve.py's *_limited functions and LimitedProofPolicy;
the kernels of csrc/learn/*_limited.hip):

  1. a first limit that never cuts (8,382) is the plain mirror in all six outputs: the small games, slices of make_golden_exact's
     generate_configs cases, twelve and fourteen weights, and the table-ordered mirrors;
  2. on every small game, both growths and first limits 0, 1 and 3: the plain mirror's verdicts, solutions that win on the C oracle in
     solution_len moves, and where there is no win a last limit that is the first to cut nothing;
  3. the caps: a capped search reports nothing, a larger cap takes no proof back;
  4. THE GAIN: the carved case at 4,000 nodes, 12 proved by the plain rule, every one of them and at least 20 in all by the limited one;
  5. the refusals in Python and in the mirrors, every refusal of the six entries as a status, the header, the exports, the kernels'
     resources;
  6. the recorded outputs that the GPU tests compare the kernels with are the mirror's as it stands.

The plain functions keep the signatures the earlier tests pin: the limited order is reached through functions and a policy class of
their own (prove_configs_limited, ..., ProofPolicy(discrepancy=) making a LimitedProofPolicy)."""
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
from test_solve_cpu import CW, _replay

import tetris_piclim as T

sys.path.insert(0, GOLDEN)
import make_golden_exact as G  # noqa: E402  -- the inputs of every case here
import make_golden_exact_limited as GL  # noqa: E402

NEVER_CUTS = 8382
RULES = [(first, growth) for growth in (0, 1) for first in (0, 1, 3)]
DW = np.array(T.DELLACHERIE_WEIGHTS)


def _m():
    return T._learn_lib


def _same(a, b, what):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), what


def _limits(first, growth, last):
    """The limits of one budget from `first` up to `last`."""
    out = [first]
    while out[-1] < last:
        out.append(min(max(1, 2 * out[-1]) if growth else out[-1] + 1, 65535))
    return out


# ------------------------------------------------------------------------------------------------ 1. a limit that never cuts
@pytest.mark.parametrize("L,M,game_L,count", G.SMALL)
def test_a_first_limit_of_8382_is_the_plain_mirror_on_the_small_games(L, M, game_L, count):
    m = _m()
    rows, pieces = T.generate_configs(game_L, M, count, seed=31 + M)
    for w in (CW, DW):
        for shortest in (True, False):
            plain = m.placement_exact(rows, pieces, L, M, w, G.SMALL_NODES, shortest=shortest)
            for growth in (0, 1):
                got = m.placement_exact_limited(rows, pieces, L, M, w, G.SMALL_NODES, NEVER_CUTS, growth, shortest=shortest)
                assert len(got) == 7 and got[6].dtype == np.int32
                _same(got[:6], plain, (L, M, game_L, len(w), shortest, growth))
                assert np.array_equal(got[6], np.where(plain[4] <= M, NEVER_CUTS, 0))       # 0 where there was no iteration


def test_a_first_limit_of_8382_is_the_plain_mirror_on_slices_of_the_generated_cases():
    m = _m()
    for key, args in G.cases():
        if not key.startswith("cfg_") or args["max_nodes"] == 4000 and "owed" not in key:
            continue
        rows, pieces = G.inputs(args)
        pick = np.arange(0, rows.shape[0], 5)
        plain = G.run_case(m, args, pick)
        got = m.placement_exact_limited(rows[pick], pieces[pick], args["L"], args["M"], G.weights()[args["F"]], args["max_nodes"],
                                        NEVER_CUTS, 0, shortest=args["shortest"], spare_weight=args["spare_weight"])
        _same(got[:6], [plain[name] for name in G.NAMES], key)
    # first_limit=None is the plain rule itself: six arrays
    args = dict(G.cases())["cfg_L3_M8_c256"]
    rows, pieces = G.inputs(args)
    assert len(m.placement_exact_limited(rows[:4], pieces[:4], 3, 8, CW, 256, None)) == 6


def test_the_table_mirrors_are_held_to_the_same_equality():
    m = _m()
    rows, pieces = T.generate_configs(3, 8, 12, seed=7)
    rng = np.random.default_rng(5)
    for form in m.NTUPLE_EXACT_FORMS:
        table = rng.integers(-(1 << 18), 1 << 18, m.ntuple_entries_of(form)).astype(np.int32)
        for cap in (7, 256):
            plain = m.ntuple_exact(rows, pieces, 3, 8, table, cap)
            got = m.ntuple_exact_limited(rows, pieces, 3, 8, table, cap, NEVER_CUTS, 1)
            _same(got[:6], plain, (form, cap))
            low = m.ntuple_exact_limited(rows, pieces, 3, 8, table, 4000, 0, 0)
            full = m.ntuple_exact(rows, pieces, 3, 8, table, 4000)
            both = (low[1] == 1) & (full[1] == 1)
            assert both.any() and np.array_equal(low[0][both], full[0][both]) and np.array_equal(low[2][both], full[2][both])
    # the window mirrors: the frame passes the two arguments through and gathers `limit`
    z = np.zeros(12, np.int64)
    window = (pieces[:, :8].astype(np.uint64) << (np.uint64(3) * np.arange(8, dtype=np.uint64))).sum(axis=1).astype(np.uint64)
    state = z.copy()
    state[3] = 1                                               # a finished board among them
    skip = (np.arange(12) == 5).astype(np.uint8)
    table = rng.integers(-(1 << 18), 1 << 18, m.ntuple_entries_of("feat")).astype(np.int32)
    for plain, limited in ((lambda **k: m.placement_window_prove(rows, z, z, state, window, 3, 8, CW, 256, skip=skip),
                            lambda **k: m.placement_window_prove_limited(rows, z, z, state, window, 3, 8, CW, 256, skip=skip, **k)),
                           (lambda **k: m.ntuple_window_prove(rows, z, z, state, window, 3, 8, table, 256, skip=skip),
                            lambda **k: m.ntuple_window_prove_limited(rows, z, z, state, window, 3, 8, table, 256, skip=skip, **k))):
        a, b = plain(), limited(first_limit=NEVER_CUTS)
        assert set(b) == set(a) | {"limit"} and b["limit"].dtype == np.int32
        for name in a:
            assert np.array_equal(a[name], b[name]), name
        searched = (state == 0) & (skip == 0) & (a["bound"] <= a["horizon"])
        assert np.array_equal(b["limit"], np.where(searched, NEVER_CUTS, 0))
        c = limited(first_limit=0, growth=1)
        proved = (a["proved"] == 1) & (c["proved"] == 1)
        assert proved.any() and np.array_equal(a["verdict"][proved], c["verdict"][proved])
        assert np.array_equal(a["solution_len"][proved], c["solution_len"][proved])
        assert (c["limit"][~searched] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the small games
@pytest.mark.parametrize("L,M,game_L,count", G.SMALL)
def test_the_limited_mirror_proves_what_the_plain_one_proves_on_the_small_games(oracle, L, M, game_L, count):
    m = _m()
    rows, pieces = T.generate_configs(game_L, M, count, seed=31 + M)
    plain = m.placement_exact(rows, pieces, L, M, CW, G.SMALL_NODES)
    first_budget = m.placement_exact(rows, pieces, L, M, CW, G.SMALL_NODES, shortest=False)
    assert plain[1].all()
    for first, growth in RULES:
        solved, proved, length, actions, bound, nodes, limit = m.placement_exact_limited(rows, pieces, L, M, CW, G.SMALL_NODES, first, growth)
        assert proved.all()
        for got, want in ((solved, plain[0]), (length, plain[2]), (bound, plain[4])):
            assert np.array_equal(got, want), (first, growth)
        assert (nodes >= plain[5]).all() or first > 0          # from 0 every plain expansion is made again at least once
        for i in range(count):
            if solved[i]:
                assert _replay(oracle, L, M, rows[i], pieces[i], actions[i], length[i]) == (1, length[i])
                assert (actions[i, length[i]:] == 255).all() and (actions[i, :length[i]] < 40).all()
            else:
                assert length[i] == 0 and (actions[i] == 255).all()
        assert (limit[bound > M] == 0).all() and (nodes[bound > M] == 0).all()
        # no win: every budget was searched out, and the last limit is the first of its budget that cut nothing -- from it the budget
        # M alone takes the plain search's nodes, and from any limit before it the search comes to it
        lost = np.flatnonzero((solved == 0) & (bound <= M))
        for i in lost:
            seq = _limits(first, growth, int(limit[i]))
            assert seq[-1] == limit[i], (first, growth, i, seq)
            for k in seq:
                one = m.placement_exact_limited(rows[i:i + 1], pieces[i:i + 1], L, M, CW, G.SMALL_NODES, k, growth, shortest=False)
                assert one[6][0] == limit[i], (first, growth, i, k)
                if k == limit[i]:
                    assert one[5][0] == first_budget[5][i]
    if (L, M, game_L) == (2, 3, 1):
        assert ((plain[0] == 0) & (plain[4] <= M)).any()      # such games are among them


# ------------------------------------------------------------------------------------------------ 3. the caps
def test_a_capped_limited_search_reports_nothing_and_a_larger_cap_takes_no_proof_back():
    m = _m()
    L, M, n = 3, 8, 64
    rows, pieces = T.generate_configs(L, M, n, seed=7)
    for first, growth in ((0, 0), (1, 1), (3, 0)):
        runs = {cap: m.placement_exact_limited(rows, pieces, L, M, CW, cap, first, growth) for cap in (1, 7, 256)}
        for cap, (solved, proved, length, actions, bound, nodes, limit) in runs.items():
            capped = proved == 0
            assert (solved[capped] == 0).all() and (length[capped] == 0).all() and (actions[capped] == 255).all()
            assert (nodes[capped] == cap).all() and (nodes <= cap).all() and (solved <= proved).all()
        assert (runs[1][1] == 0).any() and runs[256][1].sum() > runs[7][1].sum() >= runs[1][1].sum()
        for lo, hi in ((1, 7), (7, 256)):
            was = runs[lo][1] == 1
            assert (runs[hi][1][was] == 1).all()
            for x, y in zip(runs[lo], runs[hi]):
                assert np.array_equal(x[was], y[was]), (first, growth, lo, hi)


# ------------------------------------------------------------------------------------------------ 4. the gain
@functools.lru_cache(maxsize=None)
def _carved(growth):
    return G.carved_case(_m()) if growth is None else GL.carved_case(_m(), growth)


def test_the_limited_order_proves_at_least_twenty_of_the_carved_case_where_the_plain_one_proves_twelve(oracle):
    """make_golden_exact's carved case: the first 32 configurations of carved_L10_M40.npz at M = sol_len, the classical weights, 4,000
    nodes.  The plain mirror proves 12 (test_exact_cpu.py's record).  The limited mirror from first_limit 0 proves 24 under "add" and 22
    under "double"; the issue's floor is 20 under "add", and 12 is what fails it."""
    rows, pieces, sol_len, L, _ = G.carved_inputs()
    plain, add, double = _carved(None), _carved(0), _carved(1)
    counts = tuple(int(x["proved"].sum()) for x in (plain, add, double))
    print("proved of", G.CARVED_COUNT, "at", G.CARVED_NODES, "nodes: plain", counts[0], "add", counts[1], "double", counts[2])
    print("nodes plain", plain["nodes"].tolist(), "add", add["nodes"].tolist(), "limit", add["limit"].tolist())
    assert counts[0] == 12
    assert counts[1] >= 20
    assert counts == (12, 24, 22)
    was = plain["proved"] == 1
    for got in (add, double):
        proved = got["proved"] == 1
        assert proved[was].all() and np.array_equal(got["solution_len"][was], plain["solution_len"][was])
        assert np.array_equal(got["bound"], sol_len)
        assert (got["solved"][proved] == 1).all() and np.array_equal(got["solution_len"][proved], sol_len[proved])
        assert (got["solved"][~proved] == 0).all() and (got["nodes"][~proved] == G.CARVED_NODES).all()
        for i in np.flatnonzero(proved):
            B = int(sol_len[i])
            assert _replay(oracle, L, B, rows[i], pieces[i, :B + 1], got["actions"][i], B) == (1, B)
            assert (got["actions"][i, B:] == 255).all()


# ------------------------------------------------------------------------------------------------ 6. the recorded outputs
def test_the_recorded_limited_outputs_are_the_mirrors():
    """tests/golden/exact_limited_mirror.npz (make_golden_exact_limited.py) against the mirror as it stands: slice_of()'s configurations
    of every case, and of the carved case (which the test above runs whole) both growths whole."""
    m = _m()
    g = load_golden("exact_limited_mirror.npz")
    keys = [k for k, _ in GL.cases()]
    assert sorted(g.files) == sorted(f"{k}_{name}" for k in keys + ["carved_g0", "carved_g1"] for name in GL.NAMES)
    for key, args in GL.cases():
        n = g[f"{key}_solved"].shape[0]
        pick = GL.slice_of(key, n)
        got = GL.run_case(m, args, pick)
        for name in GL.NAMES:
            want = g[f"{key}_{name}"][pick]
            assert got[name].dtype == want.dtype and np.array_equal(got[name], want), (key, name)
    for growth in (0, 1):
        got = _carved(growth)
        for name in GL.NAMES:
            want = g[f"carved_g{growth}_{name}"]
            assert got[name].dtype == want.dtype and np.array_equal(got[name], want), (growth, name)
    # what the recorded cases cover: limits past the first, capped searches, a deep stack
    cat = lambda name: np.concatenate([g[f"{k}_{name}"] for k in keys if k.startswith("cfg_")])
    assert (cat("limit") > 3).sum() >= 20 and (cat("proved") == 0).sum() >= 100 and ((cat("proved") == 1) & (cat("nodes") > 256)).sum() >= 10
    assert g["long_L105_s0_k0_g0_solution_len"].max() >= 250


# ------------------------------------------------------------------------------------------------ 5. arguments and plumbing
def test_python_refusals_of_the_limited_surface_and_of_the_mirrors_need_no_gpu():
    import torch
    m = _m()
    rows, pieces = np.zeros((4, 20), np.uint16), np.zeros((4, 7), np.uint8)
    env = types.SimpleNamespace(num_envs=4, L=5, M=10, device=torch.device("cpu"))
    table = torch.zeros(m.ntuple_entries_of("feat"), dtype=torch.int32)
    base = types.SimpleNamespace(act=lambda out=None: out, env=env)
    calls = {"prove_configs_limited": lambda **k: T.prove_configs_limited(rows, pieces, 2, 6, **k),
             "ntuple_prove_configs_limited": lambda **k: T.ntuple_prove_configs_limited(rows, pieces, 2, 6, table, **k),
             "window_prove_limited": lambda **k: T.window_prove_limited(env, **k),
             "ntuple_window_prove_limited": lambda **k: T.ntuple_window_prove_limited(env, table, **k),
             "ProofPolicy": lambda **k: T.ProofPolicy(env, base, **k),
             "TableProofPolicy": lambda **k: T.TableProofPolicy(env, base, table=table, **k)}
    for name, call in calls.items():
        for bad in ("plus", "ADD", 0, 1, True, b"add", ("add",)):
            with pytest.raises(ValueError, match="discrepancy must be None"):
                call(discrepancy=bad)
        for bad in (-1, 65536, 1.0, True, "0", None):
            with pytest.raises(ValueError, match="first_limit must be an integer in"):
                call(first_limit=bad)
            with pytest.raises(ValueError, match="first_limit must be an integer in"):
                call(discrepancy="double", first_limit=bad)
    for hook in (T.evaluate_heuristic, T.NTupleLearner.evaluate):
        assert inspect.signature(hook).parameters["proof_discrepancy"].default is None
    with pytest.raises(ValueError, match="proof_discrepancy orders the proofs"):
        T.evaluate_heuristic(env, CW, None, 4, proof_discrepancy="add")
    with pytest.raises(ValueError, match="discrepancy must be None"):
        T.evaluate_heuristic(env, CW, None, 4, proof=64, proof_discrepancy="both")
    # the surface: the plain functions are as they were, the limited ones take their arguments by keyword
    for name, lead in (("prove_configs", ["rows", "pieces", "L", "M"]), ("ntuple_prove_configs", ["rows", "pieces", "L", "M", "table"]),
                       ("window_prove", ["env"]), ("ntuple_window_prove", ["env", "table"])):
        plain, limited = getattr(T, name), getattr(T, name + "_limited")
        assert "discrepancy" not in inspect.signature(plain).parameters
        p = inspect.signature(limited).parameters
        assert list(p) == lead + ["discrepancy", "first_limit", "arguments"] and p["arguments"].kind is inspect.Parameter.VAR_KEYWORD
        assert (p["discrepancy"].default, p["first_limit"].default) == ("add", 0)
        assert limited is getattr(T.solve, name + "_limited") and name + "_limited" in T.__all__ and name + "_limited" in T.solve.__all__
        doc = re.sub(r"\s+", " ", limited.__doc__)
        for words in ("Verdicts do not change", "may name another win of the same length", "first_limit >= 8,382 gives the plain search's outputs byte for byte",
                      "at most 15 times", "up to 8,383 times"):
            assert words in doc, (name, words)
    assert "Verdict 3 still proves nothing" in re.sub(r"\s+", " ", T.window_prove_limited.__doc__)
    assert issubclass(T.LimitedProofPolicy, T.TableProofPolicy) and "LimitedProofPolicy" in T.__all__
    p = inspect.signature(T.LimitedProofPolicy.__init__).parameters
    assert list(p) == list(inspect.signature(T.TableProofPolicy.__init__).parameters) + ["discrepancy", "first_limit"]
    assert (p["discrepancy"].default, p["first_limit"].default) == ("add", 0)
    # the mirrors
    assert (m.LIMIT_TOP, m.LIMIT_NEVER_CUTS, m.DISCREPANCY_GROWTH) == (65535, NEVER_CUTS, {"add": 0, "double": 1})
    p = inspect.signature(m._exact_search).parameters
    assert list(p)[-2:] == ["first_limit", "growth"] and (p["first_limit"].default, p["growth"].default) == (None, 0)
    good = dict(rows=rows, pieces=pieces, L=2, M=6, max_nodes=4)
    zero = np.zeros(m.ntuple_entries_of("2x4"), np.int32)
    z = np.zeros(4, np.int64)
    states = dict(rows=rows, lines=z, moves=z, state=z, window=z.astype(np.uint64), L=2, M=6, max_nodes=4)
    for call in (lambda **k: m.placement_exact_limited(**good, weights=CW, **k), lambda **k: m.ntuple_exact_limited(**good, table=zero, **k),
                 lambda **k: m.placement_window_prove_limited(**states, weights=CW, **k),
                 lambda **k: m.ntuple_window_prove_limited(**states, table=zero, **k)):
        for bad in (-1, 65536, 1.5, True, "1"):
            with pytest.raises(ValueError, match="first_limit"):
                call(first_limit=bad)
        for bad in (2, -1, True, "add", None, 0.0):
            with pytest.raises(ValueError, match="growth"):
                call(first_limit=0, growth=bad)
        assert call(first_limit=65535, growth=1) is not None


ENTRIES = {
    "tpl_placement_exact_limited": ("exact", ["rows", "pieces", "n", "L", "M", "weights", "spare_weight", "max_nodes", "shortest"]),
    "tpl_placement_exact_limited_move": ("exact", ["rows", "pieces", "n", "L", "M", "weights", "spare_weight", "max_nodes", "shortest"]),
    "tpl_ntuple_exact_limited": ("exact", ["rows", "pieces", "n", "L", "M", "table", "entries", "r_line", "r_win", "r_lose", "gamma",
                                           "max_nodes", "shortest"]),
    "tpl_placement_window_prove_limited": ("window", ["plane_a", "plane_b", "n", "L", "M", "weights", "spare_weight", "max_nodes"]),
    "tpl_placement_window_prove_limited_move": ("window", ["plane_a", "plane_b", "n", "L", "M", "weights", "spare_weight", "max_nodes"]),
    "tpl_ntuple_window_prove_limited": ("window", ["plane_a", "plane_b", "n", "L", "M", "table", "entries", "r_line", "r_win", "r_lose",
                                                   "gamma", "max_nodes"]),
}
TAILS = {"exact": ["first_limit", "growth", "solved", "proved", "solution_len", "actions", "bound", "nodes", "limit", "stream"],
         "window": ["first_limit", "growth", "skip", "solved", "proved", "solution_len", "plan", "bound", "nodes", "limit", "horizon", "verdict",
                    "stream"]}
KERNELS = ("placement_exact_limited_kernel", "placement_exact_limited_move_kernel", "placement_window_prove_limited_kernel",
           "placement_window_prove_limited_move_kernel", "ntuple_exact_limited_kernel", "ntuple_exact3_limited_kernel",
           "ntuple_exact_feature_limited_kernel", "ntuple_exact_budget_limited_kernel", "ntuple_window_limited_kernel",
           "ntuple_window3_limited_kernel", "ntuple_window_feature_limited_kernel", "ntuple_window_budget_limited_kernel")


def _arguments(name):
    kind, lead = ENTRIES[name]
    return lead + TAILS[kind]


def test_every_refusal_of_the_six_entries_comes_back_as_a_status_without_a_gpu():
    m = _m()
    lib = m.lib()
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    values = dict(n=4, L=2, M=6, spare_weight=0.25, max_nodes=100, shortest=1, first_limit=0, growth=0, stream=None,
                  entries=m.ntuple_entries_of("feat"), r_line=1.0, r_win=0.0, r_lose=0.0, gamma=1.0)
    for name in ENTRIES:
        fn, args = getattr(lib, name), _arguments(name)
        ok = [values.get(a, fake) for a in args]
        at = args.index
        cases = [(at("first_limit"), -1, "first_limit must be in [0, 65535]"), (at("first_limit"), 65536, "first_limit must be in"),
                 (at("first_limit"), 1 << 30, "first_limit must be in"), (at("growth"), 2, "growth must be 0 (add) or 1 (double)"),
                 (at("growth"), -1, "growth must be 0"), (at("limit"), None, "null"), (at("limit"), fake + 2, "limit must be 4-byte aligned"),
                 (at("limit"), fake + 1, "limit must be 4-byte aligned"),
                 # and what the twin refuses is refused here under this entry's name
                 (at("n"), 0, "positive"), (at("n"), 1 << 31, "2^31"), (at("L"), 0, "L and M"), (at("M"), 255, "L and M"),
                 (at("max_nodes"), 0, "max_nodes must be in [1, 16777216]"), (at("max_nodes"), (1 << 24) + 1, "max_nodes must be in"),
                 (at("solved"), None, "null"), (at("nodes"), None, "null"), (at("nodes"), fake + 2, "nodes must be 4-byte"),
                 (at("bound"), fake + 2, "bound must be 4-byte"), (at("solution_len"), fake + 2, "solution_len must be 4-byte")]
        if "shortest" in args:
            cases += [(at("shortest"), 2, "shortest must be 0 or 1"), (at("rows"), None, "null"), (at("rows"), fake + 1, "rows must be 2-byte")]
        else:
            cases += [(at("plane_a"), None, "null"), (at("plane_b"), fake + 8, "planes must be 16-byte"), (at("verdict"), None, "null")]
        if "table" in args:
            cases += [(at("entries"), 12345, "the four plain forms"), (at("table"), None, "null"), (at("table"), fake + 2, "table must be 4-byte"),
                      (at("gamma"), float("nan"), "gamma must be finite")]
        else:
            cases += [(at("weights"), None, "null"), (at("weights"), fake + 4, "weights must be 16-byte"),
                      (at("spare_weight"), float("inf"), "spare_weight must be finite")]
        for index, value, what in cases:
            call = list(ok)
            call[index] = value
            assert fn(*call) < 0 and name + ":" in err() and what in err(), (name, args[index], value, err())
        # the largest first limit and both growths are not refused: a check that comes after them speaks
        for growth in (0, 1):
            call = list(ok)
            call[at("first_limit")], call[at("growth")], call[at("limit")] = 65535, growth, fake + 2
            assert fn(*call) < 0 and "limit must be 4-byte aligned" in err()


def test_the_header_states_the_limited_rule_and_the_library_exports_the_six_entries():
    m = _m()
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_\w+)\s*\(", text))
    assert declared == set(m.LEARN_SYMBOLS) and set(ENTRIES) <= declared
    lib = ctypes.CDLL(m.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name), name
        proto = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == _arguments(name), name
        twin = re.search(r"int %s\((.*?)\);" % name.replace("_limited", ""), text, flags=re.S).group(1)
        mine = [a.split()[-1].lstrip("*") for a in proto.split(",")]
        assert [a for a in mine if a not in ("first_limit", "growth", "limit")] == [a.split()[-1].lstrip("*") for a in twin.split(",")]
        assert re.search(r"int32_t first_limit,\s+int32_t growth", proto) and "int32_t* limit" in proto
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("AN ITERATION is (B, K)", "WHATEVER ITS RANK", "Only the children of rank <= rem are kept",
                  "The kept child of rank j is searched with rem - j", "K' = K + 1 with growth = 0 (\"add\"), K' = max(1, 2 K) with growth = 1 (\"double\")",
                  "clamped at 65,535", "a K >= 8,382 never cuts", "nodes counts the expansions of ALL iterations (B, K)",
                  "limit is the K of the last iteration begun, and 0 where there was no iteration",
                  "VERDICTS DO NOT CHANGE", "because the last iteration at every budget cut nothing", "THE SOLUTION MAY DIFFER",
                  "first_limit >= 8,382 gives the plain search's outputs BYTE FOR BYTE", "THE WORST CASE for a budget with no win is bounded",
                  "at most 15 T under \"double\"", "up to 8,383 T under \"add\"", "VERDICT 3 STILL PROVES NOTHING ABOUT THE GAME",
                  "first_limit outside [0, 65535], growth other than 0 or 1, a NULL limit, limit not 4-byte aligned"):
        assert words in flat, words
    # the search stays in one file: the limited units are the twins' text, built again
    for unit, twin in (("exact_limited.hip", "exact.hip"), ("exact_window_limited.hip", "exact_window.hip"),
                       ("ntuple_exact_limited.hip", "ntuple_exact.hip"), ("ntuple_window_limited.hip", "ntuple_window.hip")):
        code = [l for l in open(os.path.join(m._LEARN_CSRC, unit)).read().splitlines() if l.strip() and not l.startswith("//")]
        assert code == ["#define TPL_EXACT_LIMITED_UNIT", f'#include "{twin}"'], unit
        assert unit in [os.path.basename(p) for p in m._UNITS]
    for unit, twin in (("exact_limited_move.hip", "exact.hip"), ("exact_window_limited_move.hip", "exact_window.hip")):
        code = [l for l in open(os.path.join(m._LEARN_CSRC, unit)).read().splitlines() if l.strip() and not l.startswith("//")]
        assert code == ["#define TPL_PLACEMENT_MOVE_UNIT", "#define TPL_PLACEMENT_BOUND_UNIT", "#define TPL_EXACT_LIMITED_UNIT", f'#include "{twin}"']
    header = open(os.path.join(m._LEARN_CSRC, "tpl_exact.h")).read()
    assert "template <typename Order, bool Limited = false>" in header and header.count("kids[rank]") == 1
    assert "sizeof(Frame<uint32_t>) == 80 && sizeof(Frame<NoCarry>) == 80" in header


def test_the_limited_kernels_use_no_scratch_and_fill_a_simd_with_waves():
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
        print(kernel, "vgpr", num(r, "vgpr"), "sgpr", num(r, "sgpr"), "lds", num(r, "lds"))
        assert num(r, "scratch") == 0, r
        assert num(r, "vgpr") <= 64, r                                       # eight waves a SIMD by the vector registers: no exception
        static = num(r, "lds")
        twin = [t for t in rows if f"{len(kernel) - 8}{kernel.replace('_limited', '')}E" in t[-1]]
        assert len(twin) == 1 and num(twin[0], "lds") == static, (kernel, twin)   # the twin's LDS: a record is still 80 bytes
        assert 32 * (static + 80 * 40) <= 160 * 1024, r
