"""CPU-side checks of the exact depth-first solver whose children a table orders (include/tpl_learn.h's rule under tpl_ntuple_exact;
_learn_lib.ntuple_exact; solve.py's ntuple_prove_configs; csrc/learn/ntuple_exact.hip):

  1. the recorded outputs that the GPU tests compare the kernels with are the mirror's as it stands (a slice of every case);
  2. against the recorded outputs of tpl_placement_exact's mirror, on three cases under the hashed "feat+spare" and "feat" tables: `bound`
     is equal everywhere; where both searches set `proved`, solved and solution_len are equal; where the recorded search is unwinnable
     the table-ordered one is proved and unwinnable with the same `nodes`; and the both-proved sets are not hollow;
  3. on test_solve_cpu's six small games the verdicts are the exhaustive enumeration's on the C oracle and every solution replays to a
     win after exactly solution_len moves;
  4. the cap: with max_nodes 1 and 7 nothing capped is reported solved, and a larger cap takes no proof back;
  5. the Python refusals of ntuple_prove_configs and of the mirror, every refusal of the entry as a status without a GPU, the header
     against LEARN_SYMBOLS and the exports, the four kernels' resources;
  6. the entry's host code refuses every bad argument under ASan + UBSan in a stand-alone program (tests/c_abi/sanitize_ntuple_exact.cpp).
"""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_solve_cpu import _first_winning_ply, _replay

import tetris_piclim as T

sys.path.insert(0, GOLDEN)
import make_golden_ntuple_exact as N  # noqa: E402  -- the cases, the tables, the slices
import make_golden_exact as G  # noqa: E402  -- the inputs and the twin's cases

CASES = dict(N.cases())
NEVER = G.SMALL_NODES


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ the tables of the maker
def test_the_makers_tables_are_what_its_docstring_says():
    m = _m()
    assert m.NTUPLE_EXACT_FORMS == ("2x4", "3x3", "feat", "feat+spare")
    for form in m.NTUPLE_EXACT_FORMS:
        assert N.table(form, "zero").shape == (m.ntuple_entries_of(form),) and not N.table(form, "zero").any()
    for form in ("feat", "feat+spare"):
        hashed, huge = N.table(form, "hashed").astype(np.int64), N.table(form, "huge").astype(np.int64)
        assert N.table(form, "hashed").dtype == np.int32 and np.abs(hashed).max() <= 1 << 18 and np.abs(hashed).max() > 1 << 17
        assert (hashed > 0).any() and (hashed < 0).any() and np.unique(hashed).size > hashed.size // 2
        assert ((np.abs(huge) <= 1 << 30) & (np.abs(huge) > (1 << 30) - (1 << 12))).all() and (huge > 0).any() and (huge < 0).any()
    # entry j is a function of j alone: the first entries of two forms are the same numbers
    assert np.array_equal(N.table("feat", "hashed")[:1000], N.table("3x3", "hashed")[:1000])


# ------------------------------------------------------------------------------------------------ 1. the recorded outputs
def test_the_recorded_file_holds_the_makers_cases_and_covers_both_verdicts_and_the_cap():
    g = load_golden("ntuple_exact_mirror.npz")
    keys = list(CASES)
    assert sorted(g.files) == sorted(f"{k}_{name}" for k in keys + ["carved"] for name in N.NAMES)
    cat = lambda name: np.concatenate([g[f"{k}_{name}"] for k in keys])
    solved, proved, nodes = cat("solved"), cat("proved"), cat("nodes")
    assert ((proved == 1) & (solved == 0) & (nodes > 0)).sum() >= 4 and ((proved == 1) & (solved == 1)).sum() >= 200
    assert (proved == 0).sum() >= 100 and ((proved == 1) & (solved == 0) & (nodes == 0)).sum() >= 24
    assert g["long_L105_s0_solution_len"].max() >= 250         # a path as long as the stack


@pytest.mark.parametrize("key", list(CASES))
def test_the_recorded_outputs_are_the_mirrors(key):
    """tests/golden/ntuple_exact_mirror.npz against _learn_lib.ntuple_exact as it stands, on slice_of()'s configurations -- the mirror
    treats every configuration on its own."""
    g = load_golden("ntuple_exact_mirror.npz")
    n = g[f"{key}_solved"].shape[0]
    pick = N.slice_of(key, n)
    got = N.run_case(_m(), CASES[key], pick)
    for name in N.NAMES:
        want = g[f"{key}_{name}"][pick]
        assert got[name].dtype == want.dtype and np.array_equal(got[name], want), (key, name)


def test_the_recorded_carved_outputs_are_the_mirrors_and_what_is_proved_wins_on_the_oracle(oracle):
    g = load_golden("ntuple_exact_mirror.npz")
    got = N.carved_case(_m(), N.CARVED_SLICE)
    for name in N.NAMES:
        assert got[name].dtype == g[f"carved_{name}"].dtype
        assert np.array_equal(got[name][N.CARVED_SLICE], g[f"carved_{name}"][N.CARVED_SLICE]), name
    rows, pieces, sol_len, L, _ = G.carved_inputs()
    proved = g["carved_proved"] == 1
    print("proved", int(proved.sum()), "of", G.CARVED_COUNT, "nodes", g["carved_nodes"].tolist())
    assert np.array_equal(g["carved_bound"], sol_len)
    assert (g["carved_solved"][proved] == 1).all() and np.array_equal(g["carved_solution_len"][proved], sol_len[proved])
    assert (g["carved_solved"][~proved] == 0).all() and (g["carved_nodes"][~proved] == N.CARVED_NODES).all()
    for i in np.flatnonzero(proved):
        B = int(sol_len[i])
        assert _replay(oracle, L, B, rows[i], pieces[i, :B + 1], g["carved_actions"][i], B) == (1, B)
        assert (g["carved_actions"][i, B:] == 255).all()
    assert proved.any()


# ------------------------------------------------------------------------------------------------ 2. what the order cannot change
@pytest.mark.parametrize("tag", ["budget", "feat"])
@pytest.mark.parametrize("key,floor", N.INVARIANT)
def test_verdicts_lengths_and_unwinnable_node_counts_are_the_weight_ordered_searchs(key, floor, tag):
    """The same configurations, the same L, M, cap and `shortest`, searched by tpl_placement_exact's mirror under the classical weights
    (exact_mirror.npz) and by this one under a hashed table: consequence 1 and 2 of the header."""
    twin, mine = load_golden("exact_mirror.npz"), load_golden("ntuple_exact_mirror.npz")
    a, b = dict(G.cases())[key], CASES[f"{key}_{tag}"]
    assert all(a[k] == b[k] for k in ("source", "L", "M", "max_nodes", "shortest"))
    t = {name: twin[f"{key}_{name}"] for name in N.NAMES}
    n = {name: mine[f"{key}_{tag}_{name}"] for name in N.NAMES}
    assert np.array_equal(t["bound"], n["bound"])
    both = (t["proved"] == 1) & (n["proved"] == 1)
    print(key, tag, "both proved", int(both.sum()), "of", both.size)
    assert np.array_equal(t["solved"][both], n["solved"][both]) and np.array_equal(t["solution_len"][both], n["solution_len"][both])
    unwinnable = (t["proved"] == 1) & (t["solved"] == 0)
    assert (n["proved"][unwinnable] == 1).all() and (n["solved"][unwinnable] == 0).all()
    assert np.array_equal(n["nodes"][unwinnable], t["nodes"][unwinnable])
    assert both.sum() >= floor                                 # not hollow


# ------------------------------------------------------------------------------------------------ 3. the oracle
@pytest.mark.parametrize("L,M,game_L,count", G.SMALL)
def test_on_the_small_games_the_verdicts_are_the_exhaustive_searchs_and_every_solution_wins_on_the_oracle(oracle, L, M, game_L, count):
    m = _m()
    rows, pieces = T.generate_configs(game_L, M, count, seed=31 + M)
    want = np.array([_first_winning_ply(oracle, L, M, rows[i], pieces[i]) for i in range(count)])
    for form, kind, gamma, reward in (("feat+spare", "hashed", 1.0, (1.0, 0.0, 0.0)), ("feat", "hashed", 0.5, (1.0, 10.0, -1.0)),
                                      ("feat+spare", "zero", 1.0, (0.0, 0.0, 0.0))):
        solved, proved, length, actions, bound, nodes = m.ntuple_exact(rows, pieces, L, M, N.table(form, kind), NEVER, gamma=gamma,
                                                                       reward=reward)
        assert (solved.dtype, proved.dtype, length.dtype, actions.dtype, bound.dtype, nodes.dtype) == \
            (np.uint8, np.uint8, np.int32, np.uint8, np.int32, np.uint32)
        assert actions.shape == (count, M) and actions.flags.c_contiguous
        assert proved.all() and (nodes < NEVER).all()
        assert np.array_equal(length, want), (form, kind, length.tolist(), want.tolist())
        assert np.array_equal(solved, (want > 0).astype(np.uint8))
        assert np.array_equal(bound, (m.move_bound_cells(rows, L) + 3) // 4)
        assert (nodes[bound > M] == 0).all() and (nodes[bound <= M] >= 1).all()
        for i in range(count):
            if solved[i]:
                assert _replay(oracle, L, M, rows[i], pieces[i], actions[i], length[i]) == (1, length[i])
                assert (actions[i, length[i]:] == 255).all() and (actions[i, :length[i]] < 40).all()
            else:
                assert length[i] == 0 and (actions[i] == 255).all()
    # the first win at the full budget: the same verdicts, never shorter
    f = m.ntuple_exact(rows, pieces, L, M, N.table("feat+spare", "hashed"), NEVER, shortest=False)
    assert f[1].all() and np.array_equal(f[0], (want > 0).astype(np.uint8)) and (f[2] >= want).all()
    for i in np.flatnonzero(f[0]):
        assert _replay(oracle, L, M, rows[i], pieces[i], f[3][i], f[2][i]) == (1, f[2][i])


# ------------------------------------------------------------------------------------------------ 4. the cap
@pytest.mark.parametrize("tag", ["budget", "feat"])
def test_nothing_capped_is_reported_solved_and_a_larger_cap_takes_no_proof_back(tag):
    g = load_golden("ntuple_exact_mirror.npz")
    for stem, caps in (("cfg_L3_M8", (1, 7, 256, 4000)), ("cfg_L5_M12", (7, 256, 4000))):
        runs = {cap: tuple(g[f"{stem}_c{cap}_{tag}_{name}"] for name in N.NAMES) for cap in caps}
        for cap in caps:
            solved, proved, length, actions, bound, nodes = runs[cap]
            assert (solved <= proved).all() and (length[proved == 0] == 0).all() and (actions[proved == 0] == 255).all()
            assert (nodes <= cap).all() and (nodes[proved == 0] == cap).all()
        for lo, hi in zip(caps, caps[1:]):
            a, b = runs[lo], runs[hi]
            was = a[1] == 1
            assert (b[1][was] == 1).all(), (lo, hi)            # proved stays proved
            for x, y in zip(a, b):
                assert np.array_equal(x[was], y[was]), (lo, hi)
            assert (b[5] >= a[5]).all()
        assert (runs[caps[0]][1] == 0).any() and (runs[7][1] == 0).any() and runs[7][1].any()
    # the mirror itself at max_nodes = 1: a root without a winning child proves nothing, a root with one is solved by the one node
    m = _m()
    rows, pieces = T.generate_configs(3, 8, 8, seed=7)
    one = m.ntuple_exact(rows, pieces, 3, 8, N.table("feat+spare", "hashed"), 1)
    capped = one[1] == 0                                       # no first move clears the three lines, or one does and is the proof
    assert capped.any() and (one[5] == 1).all() and (one[0][capped] == 0).all() and (one[3][capped] == 255).all()
    assert (one[0][~capped] == 1).all() and (one[2][~capped] == 1).all()
    rows, pieces = T.generate_configs(1, 1, 8, seed=32)
    one = m.ntuple_exact(rows, pieces, 1, 1, N.table("feat", "hashed"), 1)
    assert one[0].all() and one[1].all() and (one[2] == 1).all() and (one[5] == 1).all()


# ------------------------------------------------------------------------------------------------ 5. arguments and plumbing
def test_python_refusals_of_ntuple_prove_configs_and_of_the_mirror_need_no_gpu():
    import torch
    m = _m()
    rows, pieces = np.zeros((4, 20), np.uint16), np.zeros((4, 7), np.uint8)
    table = torch.zeros(m.ntuple_entries_of("feat+spare"), dtype=torch.int32)
    ok = dict(rows=rows, pieces=pieces, L=2, M=6, table=table)
    for L in (0, 251, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="L must"):
            T.ntuple_prove_configs(**dict(ok, L=L))
    for M in (0, 255, -1, 6.0, True):
        with pytest.raises(ValueError, match="M must"):
            T.ntuple_prove_configs(**dict(ok, M=M))
    for bad in (0, (1 << 24) + 1, -1, 1.5, 8.0, True, "8", None):
        with pytest.raises(ValueError, match="max_nodes"):
            T.ntuple_prove_configs(**ok, max_nodes=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="shortest must be"):
            T.ntuple_prove_configs(**ok, shortest=bad)
    for bad in (np.inf, np.nan, 1e39, -np.inf):
        with pytest.raises(ValueError, match="gamma must be finite"):
            T.ntuple_prove_configs(**ok, gamma=bad)
        with pytest.raises(ValueError, match=r"reward\[1\] must be finite"):
            T.ntuple_prove_configs(**ok, reward=(1.0, bad, 0.0))
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(ValueError, match="gamma must be a number"):
            T.ntuple_prove_configs(**ok, gamma=bad)
    for bad in (1.0, (1.0, 0.0), (1.0, 0.0, 0.0, 0.0), "abc", None, (1.0, None, 0.0), (True, 0.0, 0.0)):
        with pytest.raises(ValueError, match="reward"):
            T.ntuple_prove_configs(**ok, reward=bad)
    for r, p in ((np.zeros((4, 19), np.uint16), pieces), (rows, np.zeros((4, 5), np.uint8)), (rows, np.zeros((3, 7), np.uint8)),
                 (np.zeros((4, 20, 9), bool), pieces)):
        with pytest.raises(ValueError, match="rows must be"):
            T.ntuple_prove_configs(r, p, 2, 6, table)
    with pytest.raises(ValueError, match="at least one"):
        T.ntuple_prove_configs(np.zeros((0, 20), np.uint16), np.zeros((0, 7), np.uint8), 2, 6, table)
    # the table: a tensor of one of the four plain forms; a sum, a 3x3 + feature or a staged table is refused with the four named
    for bad in (None, np.zeros(21504, np.int32), torch.zeros(21504, dtype=torch.float32), torch.zeros((2, 21504), dtype=torch.int32), "feat"):
        with pytest.raises(ValueError, match="table must be an int32 tensor"):
            T.ntuple_prove_configs(**dict(ok, table=bad))
    for entries in (m.NTUPLE_ENTRIES_SUM, m.NTUPLE_ENTRIES_3X3_FEAT, m.ntuple_staged_entries_of("2x4"), 21505, 0):
        with pytest.raises(ValueError, match="four plain forms") as e:
            T.ntuple_prove_configs(**dict(ok, table=torch.zeros(entries, dtype=torch.int32)))
        assert all(form in str(e.value) for form in ("'2x4'", "'3x3'", "'feat'", "'feat+spare'"))
    p = inspect.signature(T.ntuple_prove_configs).parameters
    assert list(p) == ["rows", "pieces", "L", "M", "table", "gamma", "reward", "max_nodes", "shortest", "device", "validate"]
    assert (p["gamma"].default, p["reward"].default, p["max_nodes"].default, p["shortest"].default, p["device"].default,
            p["validate"].default) == (1.0, (1.0, 0.0, 0.0), 1 << 16, True, "cuda:0", True)
    assert T.ntuple_prove_configs is T.solve.ntuple_prove_configs
    assert "ntuple_prove_configs" in T.__all__ and "ntuple_prove_configs" in T.solve.__all__
    assert "NOTHING is proved" in T.ntuple_prove_configs.__doc__ and "IS a proof" in T.ntuple_prove_configs.__doc__
    assert "tighten_pool" in T.ntuple_prove_configs.__doc__
    # the mirror
    p = inspect.signature(m.ntuple_exact).parameters
    assert list(p) == ["rows", "pieces", "L", "M", "table", "max_nodes", "shortest", "gamma", "reward"]
    assert (p["shortest"].default, p["gamma"].default, p["reward"].default) == (True, 1.0, (1.0, 0.0, 0.0))
    good = dict(rows=rows, pieces=pieces, L=2, M=6, table=N.table("feat+spare", "zero"), max_nodes=4)
    for bad in (dict(L=0), dict(M=255), dict(max_nodes=0), dict(max_nodes=(1 << 24) + 1), dict(max_nodes=True), dict(max_nodes=2.0),
                dict(shortest=1), dict(gamma=np.inf), dict(gamma=None), dict(reward=(1.0, np.nan, 0.0)), dict(reward=(1.0, 0.0)),
                dict(table=np.zeros(21504, np.int64)), dict(table=np.zeros(m.NTUPLE_ENTRIES_SUM, np.int32)),
                dict(table=np.zeros(m.ntuple_staged_entries_of("3x3"), np.int32)), dict(table=np.zeros(21503, np.int32)),
                dict(pieces=pieces[:, :6])):
        with pytest.raises(ValueError):
            m.ntuple_exact(**{**good, **bad})
    with pytest.raises(ValueError, match="four plain forms"):
        m.ntuple_exact(**dict(good, table=np.zeros(m.NTUPLE_ENTRIES_SUM, np.int32)))


ENTRY = "tpl_ntuple_exact"
KERNELS = ("ntuple_exact_kernel", "ntuple_exact3_kernel", "ntuple_exact_feature_kernel", "ntuple_exact_budget_kernel")
ARGS = ["rows", "pieces", "n", "L", "M", "table", "entries", "r_line", "r_win", "r_lose", "gamma", "max_nodes", "shortest", "solved",
        "proved", "solution_len", "actions", "bound", "nodes", "stream"]


def test_every_refusal_of_the_entry_comes_back_as_a_status_without_a_gpu():
    m = _m()
    lib = m.lib()
    fn = lib.tpl_ntuple_exact
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    counts = [m.ntuple_entries_of(form) for form in m.NTUPLE_EXACT_FORMS]
    for entries in counts:
        ok = [fake, fake, 4, 2, 6, fake, entries, 1.0, 0.0, 0.0, 1.0, 100, 1, fake, fake, fake, fake, fake, fake, None]
        assert len(ok) == len(ARGS)
        cases = [(ARGS.index(a), None, "null") for a in ("rows", "pieces", "table", "solved", "proved", "solution_len", "actions", "bound",
                                                           "nodes")]
        cases += [(2, 0, "positive"), (2, -3, "positive"), (2, 1 << 31, "2^31"), (2, 1 << 40, "2^31"), (3, 0, "L and M"), (3, 251, "L and M"),
                  (4, 0, "L and M"), (4, 255, "L and M"), (0, fake + 1, "rows must be 2-byte"), (5, fake + 2, "table must be 4-byte"),
                  (15, fake + 2, "solution_len must be 4-byte"), (17, fake + 2, "bound must be 4-byte"), (18, fake + 2, "nodes must be 4-byte"),
                  (11, 0, "max_nodes must be in [1, 16777216]"), (11, -1, "max_nodes must be in"), (11, (1 << 24) + 1, "max_nodes must be in"),
                  (12, 2, "shortest must be 0 or 1"), (12, -1, "shortest must be 0 or 1")]
        for at in (7, 8, 9):
            cases += [(at, float("inf"), "r_line, r_win and r_lose must be finite"), (at, float("nan"), "must be finite")]
        cases += [(10, float("inf"), "gamma must be finite"), (10, float("-inf"), "gamma must be finite"), (10, float("nan"), "gamma must be finite")]
        for at, value, what in cases:
            args = list(ok)
            args[at] = value
            assert fn(*args) < 0 and ENTRY + ":" in err() and what in err(), (ARGS[at], value, err())
        # the largest game and the largest node budget are not refused for their size: a check that comes after them speaks
        args = list(ok)
        args[3], args[4], args[11], args[0] = 250, 254, 1 << 24, fake + 1
        assert fn(*args) < 0 and "aligned" in err() and "L and M" not in err() and "max_nodes" not in err()
    # any other entry count is refused, first, with the four forms named: a sum table, a 3x3 + feature table, the staged tables
    others = [0, -1, 1, m.NTUPLE_ENTRIES_SUM, m.NTUPLE_ENTRIES_3X3_FEAT, 21505, 1 << 40] + \
        [m.ntuple_staged_entries_of(s) for s in ("2x4", "3x3", "2x4+3x3")]
    for entries in others:
        for args in ([fake, fake, 4, 2, 6, fake, entries, 1.0, 0.0, 0.0, 1.0, 100, 1, fake, fake, fake, fake, fake, fake, None],
                     [None, None, 0, 0, 0, None, entries, 1.0, 0.0, 0.0, 1.0, 0, 7, None, None, None, None, None, None, None]):
            assert fn(*args) < 0 and ENTRY + ": entries must be" in err(), (entries, err())
            assert all(f'"{form}"' in err() for form in m.NTUPLE_EXACT_FORMS) and all(str(c) in err() for c in counts), err()


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
    assert len(m.lib().tpl_ntuple_exact.argtypes) == len(ARGS)
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("tpl_ntuple_exact IS tpl_placement_exact WITH ONE THING REPLACED", "OF THE CURRENT ITERATION", "V IS READ AT B, NOT AT M",
                  "value = reward + gamma * V if the child runs", "pieces[d + 1] exists", "ordered by (value descending, b ascending)",
                  "ARE INDEPENDENT OF THE TABLE", "PROVED UNWINNABLE, nodes is independent of the order too",
                  "WITH proved = 0 NOTHING IS PROVED", "no state addresses an entry outside the buffer"):
        assert words in flat, words
    # a unit of its own, of the bounded form, without a barrier; the twin's units are not touched by it
    units = [os.path.basename(p) for p in m._UNITS]
    assert "ntuple_exact.hip" in units and "exact.hip" in units and "exact_move.hip" in units
    body = open(os.path.join(m._LEARN_CSRC, "ntuple_exact.hip")).read()
    assert "#define TPL_PLACEMENT_BOUND_UNIT" in body and "__syncthreads" not in body and "ntuple_value<S>" in body
    assert '#include "exact.hip"' not in body and "prune_dead<" not in body
    assert any(p.endswith(os.path.join("learn", "ntuple_exact.hip")) for p in m._sources())


def test_the_four_kernels_use_no_scratch_and_their_stacks_fit_lds():
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


# ------------------------------------------------------------------------------------------------ 6. the sanitizers
def test_host_entry_code_under_address_and_ub_sanitizers(tmp_path):
    """The host side of csrc/learn/ntuple_exact.hip (the entry's argument checks) compiled host-only with -fsanitize=address,undefined
    and driven by a stand-alone program over every refusal path.  Nothing is loaded into Python."""
    flags = ["--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
             "-I", os.path.join(ROOT, "include")]
    exe = str(tmp_path / "sanitize_ntuple_exact")
    cmd = ["hipcc"] + flags + [os.path.join(_m()._LEARN_CSRC, "ntuple_exact.hip"),
                               os.path.join(ROOT, "tests", "c_abi", "sanitize_ntuple_exact.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, " ".join(cmd) + "\n" + res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "sanitizer run ok" in res.stdout, res.stdout + res.stderr
