"""CPU-side checks of the exact depth-first solver (include/tpl_learn.h's rule; _learn_lib.placement_exact; solve.py's prove_configs;
tpl_placement_exact[_move] in csrc/learn/exact.hip):

  1. on test_solve_cpu's small games, with a node budget that is never reached, the mirror proves every configuration, reports the ply at
     which an exhaustive enumeration on the C oracle first finds a win, proves the others unwinnable, and every solution replays to a win;
  2. wherever the bounded beam, wide enough to keep everything, is `complete`, the two searches agree on solved and solution_len;
  3. shortest=False agrees with shortest=True on solved and is never shorter;
  4. the cap: max_nodes = 1 on a root without a winning child proves nothing and reports nothing; a larger cap never takes a proof
     back and never changes a proved result;
  5. the first 32 carved L = 10 configurations at a budget of their own sol_len, max_nodes = 4,000: what is proved is solved in sol_len =
     bound moves and wins on the oracle, and at least 8 are proved;
  6. the Python refusals, every refusal of both entries, the header against the exports, the kernels' resources;
  7. the recorded outputs that the GPU tests compare the kernels with are the mirror's as it stands (a slice of every case).
"""
import ctypes
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_solve_cpu import CW, _first_winning_ply, _replay

import tetris_piclim as T

sys.path.insert(0, GOLDEN)
import make_golden_exact as G  # noqa: E402  -- the cases, their inputs, the slices and the grouping of the carved case by budget

SMALL = [(1, 1, 1, 24), (1, 2, 1, 24), (2, 2, 1, 24), (2, 2, 2, 24), (2, 3, 2, 6), (2, 3, 1, 6)]
NEVER = 1 << 16                                                # a game of three moves has 1 + 34 + 34 * 34 nodes at most, three budgets


def _m():
    return T._learn_lib


def test_the_makers_small_games_are_test_solve_cpus():
    assert [tuple(c) for c in G.SMALL] == SMALL and G.SMALL_NODES == NEVER
    assert NEVER > 3 * (1 + 34 + 34 * 34)


# ------------------------------------------------------------------------------------------------ 1. - 3. the small games
@pytest.mark.parametrize("L,M,game_L,count", SMALL)
def test_the_mirror_is_the_exhaustive_search_and_the_complete_bounded_beam_on_the_small_games(oracle, L, M, game_L, count):
    m = _m()
    rows, pieces = T.generate_configs(game_L, M, count, seed=31 + M)
    solved, proved, length, actions, bound, nodes = m.placement_exact(rows, pieces, L, M, CW, NEVER)
    assert (solved.dtype, proved.dtype, length.dtype, actions.dtype, bound.dtype, nodes.dtype) == \
        (np.uint8, np.uint8, np.int32, np.uint8, np.int32, np.uint32)
    assert actions.shape == (count, M) and actions.flags.c_contiguous
    assert proved.all() and (nodes < NEVER).all()
    want = np.array([_first_winning_ply(oracle, L, M, rows[i], pieces[i]) for i in range(count)])
    assert np.array_equal(length, want), (length.tolist(), want.tolist())
    assert np.array_equal(solved, (want > 0).astype(np.uint8))
    assert np.array_equal(bound, (m.move_bound_cells(rows, L) + 3) // 4) and (length[solved == 1] >= bound[solved == 1]).all()
    assert (nodes[bound > M] == 0).all() and (nodes[bound <= M] >= 1).all()
    unwinnable = (proved == 1) & (solved == 0)
    if (L, M, game_L) in ((2, 2, 1), (2, 3, 1)):
        assert unwinnable.any()                                # proved: no sequence of placements wins
    if L == game_L:
        assert solved.all()                                    # carved for this game: winnable by construction
    for i in range(count):
        if solved[i]:
            assert _replay(oracle, L, M, rows[i], pieces[i], actions[i], length[i]) == (1, length[i])
            assert (actions[i, length[i]:] == 255).all() and (actions[i, :length[i]] < 40).all()
        else:
            assert length[i] == 0 and (actions[i] == 255).all()
    # 2. the bounded beam that keeps everything
    width = 34 ** (M - 1)
    b_solved, b_length, _, _, b_bound, complete = m.placement_solve(rows, pieces, L, M, CW, width, max_width=width, bound=True)
    assert complete.any()
    at = complete == 1
    assert np.array_equal(solved[at], b_solved[at]) and np.array_equal(length[at], b_length[at]) and np.array_equal(bound, b_bound)
    # 3. the first win at the full budget
    f_solved, f_proved, f_length, f_actions, f_bound, f_nodes = m.placement_exact(rows, pieces, L, M, CW, NEVER, shortest=False)
    assert f_proved.all() and np.array_equal(f_solved, solved) and (f_length >= length).all() and np.array_equal(f_bound, bound)
    for i in np.flatnonzero(f_solved):
        assert _replay(oracle, L, M, rows[i], pieces[i], f_actions[i], f_length[i]) == (1, f_length[i])
    # the fourteen weights order the children differently and prove the same
    d_solved, d_proved, d_length, _, _, _ = m.placement_exact(rows, pieces, L, M, np.array(T.DELLACHERIE_WEIGHTS), NEVER)
    assert d_proved.all() and np.array_equal(d_solved, solved) and np.array_equal(d_length, length)


# ------------------------------------------------------------------------------------------------ 4. the cap
def test_the_cap_proves_nothing_reports_nothing_and_a_larger_one_takes_no_proof_back(oracle):
    m = _m()
    L, M, n = 3, 8, 64
    rows, pieces = T.generate_configs(L, M, n, seed=7)
    runs = {cap: m.placement_exact(rows, pieces, L, M, CW, cap) for cap in (1, 2, 7, 64, 256, 4000)}
    solved, proved, length, actions, bound, nodes = runs[1]
    no_root_win = np.array([_first_winning_ply(oracle, L, 1, rows[i], pieces[i][:2]) == 0 for i in range(n)])
    assert no_root_win.any()
    at = no_root_win & (bound <= M)
    assert at.any() and (proved[at] == 0).all() and (solved[at] == 0).all() and (nodes[at] == 1).all()
    assert (length[at] == 0).all() and (actions[at] == 255).all()
    caps = sorted(runs)
    for lo, hi in zip(caps, caps[1:]):
        a, b = runs[lo], runs[hi]
        was = a[1] == 1
        assert (b[1][was] == 1).all(), (lo, hi)                # proved stays proved
        for x, y in zip(a, b):
            assert np.array_equal(x[was], y[was]), (lo, hi)    # and what was proved stays as it was, the node count included
        assert (b[5] >= a[5]).all() and (b[5] <= hi).all() and (b[5][b[1] == 0] == hi).all()
    assert runs[4000][1].all() and runs[7][1].any() and not runs[7][1].all()
    for cap in caps:                                           # solved always comes with proved; an unproved result reports nothing
        s, p, ln, act = runs[cap][:4]
        assert (s <= p).all() and (ln[p == 0] == 0).all() and (act[p == 0] == 255).all()
    # a root with a winning child is solved and proved by the one node
    rows, pieces = T.generate_configs(1, 1, 8, seed=32)
    one = m.placement_exact(rows, pieces, 1, 1, CW, 1)
    assert one[0].all() and one[1].all() and (one[2] == 1).all() and (one[5] == 1).all()


# ------------------------------------------------------------------------------------------------ 5. a real pool
@functools.lru_cache(maxsize=None)
def _carved():
    return G.carved_case(_m())


def test_what_is_proved_of_the_carved_pool_is_solved_at_the_bound_and_wins_on_the_oracle(oracle):
    """The first 32 configurations of carved_L10_M40.npz at M = sol_len, classical weights, max_nodes = 4,000.  A Python probe of the
    rule proved 12 while the rule was written; the floor of 8 keeps the test from passing on nothing."""
    rows, pieces, sol_len, L, _ = G.carved_inputs()
    got = _carved()
    proved = got["proved"] == 1
    print("proved", int(proved.sum()), "of", G.CARVED_COUNT, "nodes", got["nodes"].tolist())
    assert np.array_equal(got["bound"], sol_len)
    assert (got["solved"][proved] == 1).all() and np.array_equal(got["solution_len"][proved], sol_len[proved])
    assert (got["solved"][~proved] == 0).all() and (got["nodes"][~proved] == G.CARVED_NODES).all()
    for i in np.flatnonzero(proved):
        B = int(sol_len[i])
        assert _replay(oracle, L, B, rows[i], pieces[i, :B + 1], got["actions"][i], B) == (1, B)
        assert (got["actions"][i, B:] == 255).all()
    assert proved.sum() >= 8


# ------------------------------------------------------------------------------------------------ 7. the recorded outputs
def test_the_recorded_exact_outputs_are_the_mirrors():
    """tests/golden/exact_mirror.npz (make_golden_exact.py) against the mirror as it stands: the carved case whole, the others on
    slice_of()'s configurations -- the mirror treats every configuration on its own."""
    m = _m()
    g = load_golden("exact_mirror.npz")
    keys = [k for k, _ in G.cases()]
    assert sorted(g.files) == sorted(f"{k}_{name}" for k in keys + ["carved"] for name in G.NAMES)
    for key, args in G.cases():
        n = g[f"{key}_solved"].shape[0]
        pick = G.slice_of(key, n)
        got = G.run_case(m, args, pick)
        for name in G.NAMES:
            want = g[f"{key}_{name}"][pick]
            assert got[name].dtype == want.dtype and np.array_equal(got[name], want), (key, name)
    got = _carved()
    for name in G.NAMES:
        assert got[name].dtype == g[f"carved_{name}"].dtype and np.array_equal(got[name], g[f"carved_{name}"]), name
    # what the recorded cases cover: both verdicts, proofs of both kinds, the cap hit, a search over several budgets, a deep stack
    cat = lambda name: np.concatenate([g[f"{k}_{name}"] for k in keys])
    solved, proved, nodes = cat("solved"), cat("proved"), cat("nodes")
    assert ((proved == 1) & (solved == 0) & (nodes > 0)).sum() >= 4 and ((proved == 1) & (solved == 1)).sum() >= 200
    assert (proved == 0).sum() >= 100 and ((proved == 1) & (solved == 0) & (nodes == 0)).sum() >= 24
    k = "cfg_L4_M6_c4000_owed"                                 # wins past the first budget, and proofs that took a thousand nodes
    assert (g[f"{k}_solution_len"][g[f"{k}_solved"] == 1] > g[f"{k}_bound"][g[f"{k}_solved"] == 1]).sum() >= 4
    assert (g[f"{k}_nodes"][(g[f"{k}_proved"] == 1) & (g[f"{k}_solved"] == 0)] >= 1000).sum() >= 4
    assert g["long_L105_s0_solution_len"].max() >= 250         # a path as long as the stack


# ------------------------------------------------------------------------------------------------ 6. arguments and plumbing
def test_python_refusals_of_prove_configs_and_of_the_mirror_need_no_gpu():
    rows, pieces = np.zeros((4, 20), np.uint16), np.zeros((4, 7), np.uint8)
    ok = dict(rows=rows, pieces=pieces, L=2, M=6)
    for L in (0, 251, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="L must"):
            T.prove_configs(**dict(ok, L=L))
    for M in (0, 255, -1, 6.0, True):
        with pytest.raises(ValueError, match="M must"):
            T.prove_configs(**dict(ok, M=M))
    for bad in (0, (1 << 24) + 1, -1, 1.5, 8.0, True, "8", None):
        with pytest.raises(ValueError, match="max_nodes"):
            T.prove_configs(**ok, max_nodes=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="shortest must be"):
            T.prove_configs(**ok, shortest=bad)
    for bad in (np.inf, np.nan, 1e39, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            T.prove_configs(**ok, spare_weight=bad)
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(ValueError, match="spare_weight must be a number"):
            T.prove_configs(**ok, spare_weight=bad)
    for weights in (np.zeros(11), np.zeros((2, 12)), "classical", [None] * 12):
        with pytest.raises(ValueError, match="weights"):
            T.prove_configs(**ok, weights=weights)
    with pytest.raises(ValueError, match="finite"):
        T.prove_configs(**ok, weights=np.full(14, np.nan))
    for r, p in ((np.zeros((4, 19), np.uint16), pieces), (rows, np.zeros((4, 5), np.uint8)), (rows, np.zeros((3, 7), np.uint8)),
                 (np.zeros((4, 20, 9), bool), pieces)):
        with pytest.raises(ValueError, match="rows must be"):
            T.prove_configs(r, p, 2, 6)
    with pytest.raises(ValueError, match="at least one"):
        T.prove_configs(np.zeros((0, 20), np.uint16), np.zeros((0, 7), np.uint8), 2, 6)
    p = inspect.signature(T.prove_configs).parameters
    assert list(p) == ["rows", "pieces", "L", "M", "weights", "max_nodes", "shortest", "spare_weight", "device", "validate"]
    assert (p["weights"].default, p["max_nodes"].default, p["shortest"].default, p["spare_weight"].default, p["validate"].default) == \
        (None, 1 << 16, True, 0.0, True)
    assert T.prove_configs is T.solve.prove_configs and "prove_configs" in T.__all__ and "prove_configs" in T.solve.__all__
    assert "NOTHING is proved" in T.prove_configs.__doc__ and "IS a proof" in T.prove_configs.__doc__
    assert "prove_configs" in T.tighten_pool.__doc__ and "budget is exact" in T.tighten_pool.__doc__
    m = _m()
    p = inspect.signature(m.placement_exact).parameters
    assert list(p) == ["rows", "pieces", "L", "M", "weights", "max_nodes", "shortest", "spare_weight"]
    assert (p["shortest"].default, p["spare_weight"].default) == (True, 0.0)
    good = dict(rows=rows, pieces=pieces, L=2, M=6, weights=CW, max_nodes=4)
    for bad in (dict(L=0), dict(M=255), dict(max_nodes=0), dict(max_nodes=(1 << 24) + 1), dict(max_nodes=True), dict(max_nodes=2.0),
                dict(shortest=1), dict(spare_weight=np.inf), dict(weights=np.zeros(13)), dict(pieces=pieces[:, :6])):
        with pytest.raises(ValueError):
            m.placement_exact(**{**good, **bad})
    assert m.EXACT_MAX_NODES == 1 << 24


ENTRIES = ("tpl_placement_exact", "tpl_placement_exact_move")
KERNELS = ("placement_exact_kernel", "placement_exact_move_kernel")
ARGS = ["rows", "pieces", "n", "L", "M", "weights", "spare_weight", "max_nodes", "shortest", "solved", "proved", "solution_len", "actions",
        "bound", "nodes", "stream"]


def test_every_refusal_of_both_entries_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    for name in ENTRIES:
        fn = getattr(lib, name)
        ok = [fake, fake, 4, 2, 6, fake, 0.25, 100, 1, fake, fake, fake, fake, fake, fake, None]
        assert len(ok) == len(ARGS)
        cases = [(ARGS.index(a), None, "null") for a in ("rows", "pieces", "weights", "solved", "proved", "solution_len", "actions",
                                                           "bound", "nodes")]
        cases += [(2, 0, "positive"), (2, -3, "positive"), (2, 1 << 31, "2^31"), (2, 1 << 40, "2^31"), (3, 0, "L and M"), (3, 251, "L and M"),
                  (4, 0, "L and M"), (4, 255, "L and M"), (0, fake + 1, "rows must be 2-byte"), (5, fake + 4, "weights must be 16-byte"),
                  (11, fake + 2, "solution_len must be 4-byte"), (13, fake + 2, "bound must be 4-byte"), (14, fake + 2, "nodes must be 4-byte"),
                  (6, float("inf"), "spare_weight must be finite"), (6, float("nan"), "spare_weight must be finite"),
                  (7, 0, "max_nodes must be in [1, 16777216]"), (7, -1, "max_nodes must be in"), (7, (1 << 24) + 1, "max_nodes must be in"),
                  (8, 2, "shortest must be 0 or 1"), (8, -1, "shortest must be 0 or 1")]
        for at, value, what in cases:
            args = list(ok)
            args[at] = value
            assert fn(*args) < 0 and name + ":" in err() and what in err(), (name, ARGS[at], value, err())
        # the largest game and the largest node budget are not refused for their size: a check that comes after them speaks
        args = list(ok)
        args[3], args[4], args[7], args[0] = 250, 254, 1 << 24, fake + 1
        assert fn(*args) < 0 and "aligned" in err() and "L and M" not in err() and "max_nodes" not in err()


def test_the_header_states_the_rule_and_the_library_exports_both_entries():
    m = _m()
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_\w+)\s*\(", text))
    assert declared == set(m.LEARN_SYMBOLS) and set(ENTRIES) <= declared
    lib = ctypes.CDLL(m.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name), name
        proto = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ARGS, name
    assert "#define TPL_EXACT_MAX_NODES (1 << 24)" in raw
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("ONE ITERATION AT BUDGET B", "if nodes == max_nodes THE WHOLE SEARCH ENDS", "ordered by (value descending, b ascending)",
                  "If bound > M there is no iteration: solved = 0, proved = 1, nodes = 0", "proved = 1 iff the search was not stopped by max_nodes",
                  "UNDER proved = 1, solved = 0 PROVES", "WITH proved = 0 NOTHING IS PROVED", "THE SHORTEST THERE IS",
                  "Wherever tpl_placement_solve_bound reports complete = 1", "The result is a function of the inputs alone"):
        assert words in flat, words
    # the body is shared, not copied, and both units are of the bounded form
    here = os.path.dirname(m._UNITS[-1])
    units = [os.path.basename(p) for p in m._UNITS]
    assert "exact.hip" in units and "exact_move.hip" in units
    code = [l for l in open(os.path.join(here, "exact_move.hip")).read().splitlines() if l.strip() and not l.startswith("//")]
    assert code == ["#define TPL_PLACEMENT_MOVE_UNIT", "#define TPL_PLACEMENT_BOUND_UNIT", '#include "exact.hip"']
    body = open(os.path.join(here, "exact.hip")).read()
    assert "#define TPL_PLACEMENT_BOUND_UNIT" in body and "__syncthreads" not in body
    assert any(p.endswith(os.path.join("learn", "exact.hip")) for p in m._sources())


def test_the_five_exact_units_share_one_search_and_the_mirrors_one_stack_machine():
    m = _m()
    assert any(p.endswith(os.path.join("learn", "tpl_exact.h")) for p in m._sources())     # so the library's digest covers it
    here = os.path.dirname(m._UNITS[-1])
    loop = ("kids[rank]", "__builtin_amdgcn_readlane", "struct alignas(16) Frame")
    header = open(os.path.join(here, "tpl_exact.h")).read()
    assert all(words in header for words in loop)
    for unit in ("exact.hip", "exact_nodes.hip", "exact_window.hip", "ntuple_exact.hip", "ntuple_window.hip"):
        body = open(os.path.join(here, unit)).read()
        assert '#include "tpl_exact.h"' in body, unit
        assert body.index('#include "tpl_beam.h"') < body.index('#include "tpl_exact.h"'), unit
        for words in loop:
            assert words not in body, (unit, words)
    mirrors = open(m.__file__).read()
    assert mirrors.count("while stacks:") == 1 and mirrors.count("def _exact_search(") == 1


def test_the_exact_kernels_use_no_scratch_and_fill_a_simd_with_waves():
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
        assert num(r, "vgpr") <= 64, r                                       # eight waves a SIMD by the vector registers
        static = num(r, "lds")
        assert static + 80 * 254 <= 64 * 1024, r                             # the deepest stack is launchable without an attribute
        assert 32 * (static + 80 * 40) <= 160 * 1024, r                      # M = 40: the 32 waves of a CU each have their stack
    assert all(num(r, "scratch") == 0 for r in rows)
