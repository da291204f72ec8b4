"""CPU-side checks of the exact search over a state's piece window (include/tpl_learn.h's rule; _learn_lib.placement_window_prove;
solve.py's window_prove and ProofPolicy; tpl_placement_window_prove[_move] in csrc/learn/exact_window.hip).

The oracle is COMPOSITION: a running board with horizon H = min(12 - moves % 10, M - moves) is the configuration (rows, window entries
0 .. H - 1) of the game (L - lines, H), searched by the existing _learn_lib.placement_exact; and, one step further out, the node
(rows, lines, M - H, entry) of the game (L, M) over a list that holds the window's entries from M - H on, searched by
placement_exact_nodes.  The cases and their inputs are tests/golden/make_golden_window.py's.

  1. the mirror against placement_exact on the reset boards of the first 16 configurations of carved_L5_M20.npz, in (5, 10) and
     (5, 20): 12 of 16 solved at the fixture's sol_len, the four others capped, verdict 3 and never 2;
  2. every verdict 1 replays on the C oracle to a win after exactly solution_len moves;
  3. mid-game boards at move counters 1, 9, 10, 11, 19 against placement_exact_nodes over the rebuilt list; finished boards; the cap;
     the skip mask.  The fixture's recorded replays end by move 10, so only counter 1 is a replay's own: the other boards lie three
     (one group: four) moves before their solution's end and have their counter SET (make_golden_window.py says how);
  4. verdict 2: boards that the move bound lets live and the search searches out at H == rem, checked by exhaustive enumeration;
  5. the recorded mirror outputs; the Python refusals, every refusal of the two entries, the header, the units and the resources.
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
import make_golden_window as G  # noqa: E402  -- the cases and their inputs

SIX = ("solved", "proved", "solution_len", "plan", "bound", "nodes")
SOLVED = [1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1]
LENGTHS = [6, 7, 5, 7, 0, 8, 5, 0, 0, 0, 6, 6, 7, 6, 6, 6]


def _m():
    return T._learn_lib


@functools.lru_cache(maxsize=None)
def mirror(key):
    """The mirror as it stands on a case of the golden maker.  Computed once; nobody writes to it."""
    return G.run_case(_m(), key)


def shifted_lists(s, H):
    """pieces' of the specification: [n, M + 1] with pieces'[i, M - H + d] = window entry d for d < H, 7 ("no piece") elsewhere."""
    n, M = s["rows"].shape[0], s["M"]
    q = _m().window_entries(s["window"])
    lists = np.full((n, M + 1), 7, np.uint8)
    for i in range(n):
        lists[i, M - H[i]:M] = q[i, :H[i]]
    return lists


# ------------------------------------------------------------------------------------------------ 1. the reset boards
@pytest.mark.parametrize("M,H", [(10, 10), (20, 12)])
def test_the_mirror_is_placement_exact_on_the_reset_boards_of_the_fixture(M, H):
    m, g = _m(), load_golden(G.FIXTURE)
    got = mirror(f"root_M{M}")
    assert (got["horizon"] == H).all() and (got["known"] == 12).all()
    want = m.placement_exact(g["rows"][:G.COUNT], g["pieces"][:G.COUNT, :H + 1], G.L5, H, CW, G.CAP)
    for name, ref in zip(SIX, want):
        mine = got[name][:, :H] if name == "plan" else got[name]
        assert mine.dtype == ref.dtype and np.array_equal(mine, ref), name
    assert (got["plan"][:, H:] == 255).all()
    assert got["solved"].tolist() == SOLVED and int(got["solved"].sum()) == 12
    assert got["solution_len"].tolist() == LENGTHS
    assert np.array_equal(got["solution_len"][got["solved"] == 1], g["sol_len"][:G.COUNT][got["solved"] == 1])
    rest = got["solved"] == 0
    assert (got["nodes"][rest] == G.CAP).all() and (got["proved"][rest] == 0).all()          # capped: nothing is proved
    assert (got["verdict"][rest] == m.WINDOW_OPEN).all() and (got["verdict"][~rest] == m.WINDOW_WIN).all()
    assert (got["verdict"] != m.WINDOW_LOSS).all()


# ------------------------------------------------------------------------------------------------ 2. the replay
def test_every_verdict_1_plan_wins_on_the_oracle_after_exactly_its_length(oracle):
    m, g = _m(), load_golden(G.FIXTURE)
    for M in (10, 20):
        got = mirror(f"root_M{M}")
        for i in np.flatnonzero(got["verdict"] == m.WINDOW_WIN):
            n = int(got["solution_len"][i])
            assert _replay(oracle, G.L5, M, g["rows"][i], g["pieces"][i, :M + 1], got["plan"][i], n) == (1, n)
            assert (got["plan"][i, n:] == 255).all() and (got["plan"][i, :n] < 40).all()
    # mid-game: the real game goes on from the board's own lines and moves with the pieces that follow it in the list
    s, got = G.mid_states(), mirror("mid")
    wins = np.flatnonzero(got["verdict"] == m.WINDOW_WIN)
    assert wins.size >= 32
    for i in wins:
        n, k, c = int(got["solution_len"][i]), int(s["played"][i]), int(s["config"][i])
        game = oracle.Game(G.L5, s["M"], rows=s["rows"][i], pieces=g["pieces"][c, k:], lines_cleared=int(s["lines"][i]),
                           moves_used=int(s["moves"][i]), state=0)
        for b in got["plan"][i, :n]:
            assert game.state == 0
            game.move(int(b) // 10, int(b) % 10)
        assert game.state == 1 and game.moves_used == int(s["moves"][i]) + n
        assert n <= int(got["horizon"][i]) and n >= int(got["bound"][i])


# ------------------------------------------------------------------------------------------------ 3. mid-game boards
def test_mid_game_boards_are_placement_exact_nodes_over_the_rebuilt_list():
    m = _m()
    s, got = G.mid_states(), mirror("mid")
    n = s["rows"].shape[0]
    running = np.arange(n) < len(G.GROUPS) * G.COUNT
    assert sorted(set(s["moves"][running].tolist())) == list(G.COUNTERS)
    for counter, known in zip(G.COUNTERS, (11, 3, 12, 11, 3)):
        at = running & (s["moves"] == counter)
        assert (got["known"][at] == known).all() and (got["horizon"][at] == min(known, 20 - counter)).all()
    H = got["horizon"].astype(np.int64)
    assert (H[s["moves"] == 19][:G.COUNT] == 1).all()
    lists = shifted_lists(s, H)
    lines = np.where(running, s["lines"], G.L5)                # a finished board is a finished node: lines = L
    want = m.placement_exact_nodes(s["rows"], lines, s["M"] - H, np.arange(n), lists, G.L5, s["M"], CW, G.CAP)
    for name, ref in zip(SIX, want):
        if name == "plan":
            assert np.array_equal(got[name], ref[:, :12]) and (ref[:, 12:] == 255).all()
        else:
            assert np.array_equal(got[name], ref), name
    # the verdicts: 1 where solved, 2 where proved without a win and the window reaches the end of the game, else 3; 0 if finished
    rem = s["M"] - s["moves"]
    verdict = np.where(~running, 0, np.where(got["solved"] == 1, 1, np.where((got["proved"] == 1) & (H == rem), 2, 3)))
    assert np.array_equal(got["verdict"], verdict)
    assert set(np.unique(got["verdict"]).tolist()) == {0, 1, 2, 3}
    # finished boards: nothing searched, nothing but 255s, proved as the nodes entry finishes them
    for name, value in (("solved", 0), ("proved", 1), ("solution_len", 0), ("bound", 0), ("nodes", 0), ("horizon", 0), ("verdict", 0)):
        assert (got[name][~running] == value).all(), name
    assert (got["plan"][~running] == 255).all()
    # searched out with pieces still unknown: that is verdict 3, and it comes with proved = 1
    short = running & (H < rem) & (got["solved"] == 0) & (got["proved"] == 1)
    assert short.any() and (got["verdict"][short] == m.WINDOW_OPEN).all()


def test_the_cap_gives_verdict_3_and_a_larger_one_takes_no_proof_back():
    m = _m()
    one, full = mirror("mid_cap1"), mirror("mid")
    searched = full["nodes"] > 1
    assert searched.any()
    assert (one["verdict"][searched] == m.WINDOW_OPEN).all() and (one["proved"][searched] == 0).all()
    assert (one["nodes"][searched] == 1).all() and (one["plan"][searched] == 255).all() and (one["solution_len"][searched] == 0).all()
    decided = one["proved"] == 1                               # what one node (or none) decides stays as it is
    for name in G.NAMES:
        assert np.array_equal(one[name][decided], full[name][decided]), name
    for name in ("bound", "horizon", "known"):
        assert np.array_equal(one[name], full[name]), name
    # fourteen weights order the children differently; where both searches end they prove the same
    move = mirror("mid_F14")
    both = (move["proved"] == 1) & (full["proved"] == 1)
    assert both.sum() >= 60
    for name in ("solved", "solution_len", "verdict", "bound", "horizon"):
        assert np.array_equal(move[name][both], full[name][both]), name


def test_a_skipped_board_is_not_searched_and_keeps_bound_and_horizon():
    m = _m()
    got, full = mirror("mid_skip"), mirror("mid")
    n = got["verdict"].size
    skip = np.arange(n) % 3 == 0
    for name, value in (("solved", 0), ("proved", 0), ("solution_len", 0), ("nodes", 0), ("verdict", 0)):
        assert (got[name][skip] == value).all(), name
    assert (got["plan"][skip] == 255).all()
    for name in ("bound", "horizon", "known"):
        assert np.array_equal(got[name], full[name]), name
    for name in G.NAMES:
        assert np.array_equal(got[name][~skip], full[name][~skip]), name


# ------------------------------------------------------------------------------------------------ 4. verdict 2
@pytest.mark.parametrize("key", sorted(G.LOSS))
def test_verdict_2_is_a_search_that_ended_at_the_end_of_the_game_and_no_enumeration_finds_a_win(oracle, key):
    m = _m()
    s, got = G.loss_states(key), mirror(key)
    L, M = s["L"], s["M"]
    assert (got["horizon"] == M).all() and (got["proved"] == 1).all()                      # H == rem, and nothing was capped
    loss = got["verdict"] == m.WINDOW_LOSS
    by_search = loss & (got["nodes"] >= 1)                       # alive by the bound, dead by geometry
    assert by_search.sum() >= 2 and (got["bound"][by_search] <= M).all()
    assert np.array_equal(loss, got["solved"] == 0) and (got["verdict"][~loss] == m.WINDOW_WIN).all()
    want = m.placement_exact(s["rows"], s["pieces"][:, :M + 1], L, M, CW, G.CASES[key]["max_nodes"])
    for name, ref in zip(SIX, want):
        assert np.array_equal(got[name][:, :M] if name == "plan" else got[name], ref), name
    if M <= 3:                                                 # 34^3 sequences a board: the enumeration is affordable
        for i in range(got["verdict"].size):
            first = _first_winning_ply(oracle, L, M, s["rows"][i], s["pieces"][i, :M + 1])
            assert first == int(got["solution_len"][i]) and (first == 0) == bool(loss[i]), i
    for i in np.flatnonzero(~loss):
        n = int(got["solution_len"][i])
        assert _replay(oracle, L, M, s["rows"][i], s["pieces"][i, :M + 1], got["plan"][i], n) == (1, n)


# ------------------------------------------------------------------------------------------------ 5. the record, the refusals, the build
def test_the_recorded_window_outputs_are_the_mirrors():
    rec = load_golden("window_mirror.npz")
    assert sorted(rec.files) == sorted(f"{key}_{name}" for key in G.CASES for name in G.NAMES)
    for key in G.CASES:
        got = mirror(key)
        for name in G.NAMES:
            assert got[name].dtype == rec[f"{key}_{name}"].dtype and np.array_equal(got[name], rec[f"{key}_{name}"]), (key, name)
    got = mirror("root_M10")
    assert [got[k].dtype for k in G.NAMES] == [np.uint8, np.uint8, np.int32, np.uint8, np.int32, np.uint32, np.uint8, np.uint8, np.uint8]
    assert got["plan"].shape == (G.COUNT, 12) and got["plan"].flags.c_contiguous


def test_python_refusals_of_the_mirror_and_of_the_policy_need_no_gpu():
    m = _m()
    s = G.root_states(10)
    good = dict(rows=s["rows"], lines=s["lines"], moves=s["moves"], state=s["state"], window=s["window"], L=5, M=10, weights=CW,
                max_nodes=4)
    m.placement_window_prove(**good)
    n = s["rows"].shape[0]
    for bad in (dict(L=0), dict(L=251), dict(M=0), dict(M=255), dict(max_nodes=0), dict(max_nodes=True), dict(max_nodes=2.0),
                dict(max_nodes=(1 << 24) + 1), dict(spare_weight=np.inf), dict(weights=np.zeros(13)), dict(lines=s["lines"][:3]),
                dict(moves=np.zeros(n)), dict(state=np.full(n, 4)), dict(window=np.full(n, 1 << 36, np.uint64)), dict(skip=np.zeros(3)),
                dict(rows=s["rows"][:0]), dict(lines=np.full(n, 256))):
        with pytest.raises(ValueError):
            m.placement_window_prove(**{**good, **bad})
    assert list(inspect.signature(m.placement_window_prove).parameters) == ["rows", "lines", "moves", "state", "window", "L", "M", "weights",
                                                                          "max_nodes", "spare_weight", "skip"]
    assert (m.WINDOW_NONE, m.WINDOW_WIN, m.WINDOW_LOSS, m.WINDOW_OPEN, m.WINDOW_PLAN) == (0, 1, 2, 3, 12)
    assert m.window_entries(np.array([0o765432107654], np.uint64)).tolist() == [[4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 6, 7]]
    assert list(inspect.signature(T.window_prove).parameters) == ["env", "weights", "max_nodes", "spare_weight", "skip"]
    assert list(inspect.signature(T.ProofPolicy.__init__).parameters) == ["self", "env", "base", "weights", "max_nodes", "spare_weight",
                                                                          "reuse"]
    assert inspect.signature(T.window_prove).parameters["max_nodes"].default == 1 << 12
    assert list(inspect.signature(T.ProofPolicy.act).parameters)[:3] == ["self", "out", "verdict"]
    assert inspect.signature(T.evaluate_heuristic).parameters["proof"].default is None
    assert inspect.signature(T.NTupleLearner.evaluate).parameters["proof"].default is None
    assert "window_prove" in T.__all__ and "ProofPolicy" in T.__all__


ENTRIES = ("tpl_placement_window_prove", "tpl_placement_window_prove_move")
KERNELS = ("placement_window_prove_kernel", "placement_window_prove_move_kernel")
ARGS = ["plane_a", "plane_b", "n", "L", "M", "weights", "spare_weight", "max_nodes", "skip", "solved", "proved", "solution_len", "plan",
        "bound", "nodes", "horizon", "verdict", "stream"]


def test_every_refusal_of_both_entries_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error().decode()
    fake = 1 << 20                                             # aligned, never dereferenced: every call is refused
    ok = [fake, fake, 4, 2, 6, fake, 0.25, 100, None] + [fake] * 8 + [None]
    assert len(ok) == len(ARGS)
    required = [a for a in ARGS if a not in ("n", "L", "M", "spare_weight", "max_nodes", "skip", "stream")]
    cases = [(ARGS.index(a), None, "null") for a in required]
    cases += [(2, 0, "positive"), (2, -3, "positive"), (2, 1 << 31, "2^31"), (2, 1 << 40, "2^31"),
              (3, 0, "L and M"), (3, 251, "L and M"), (4, 0, "L and M"), (4, 255, "L and M"),
              (0, fake + 8, "planes must be 16-byte"), (1, fake + 4, "planes must be 16-byte"), (5, fake + 4, "weights must be 16-byte"),
              (6, float("inf"), "spare_weight must be finite"), (6, float("nan"), "spare_weight must be finite"),
              (7, 0, "max_nodes must be in [1, 16777216]"), (7, (1 << 24) + 1, "max_nodes must be in"),
              (ARGS.index("solution_len"), fake + 2, "solution_len must be 4-byte"), (ARGS.index("bound"), fake + 2, "bound must be 4-byte"),
              (ARGS.index("nodes"), fake + 2, "nodes must be 4-byte")]
    for name in ENTRIES:
        fn = getattr(lib, name)
        for at, value, what in cases:
            call = list(ok)
            call[at] = value
            assert fn(*call) < 0 and name + ":" in err() and what in err(), (name, ARGS[at], value, err())
        for skip in (None, fake + 1):                          # the mask is optional and has no alignment; the largest arguments pass
            call = list(ok)
            call[2], call[3], call[4], call[7], call[8], call[5] = (1 << 31) - 1, 250, 254, 1 << 24, skip, fake + 4
            assert fn(*call) < 0 and "weights must be 16-byte" in err()


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
    for k, name in enumerate(("NONE", "WIN", "LOSS", "OPEN")):
        assert f"#define TPL_WINDOW_{name} {k}\n" in raw
    assert "#define TPL_WINDOW_PLAN 12\n" in raw
    flat = re.sub(r"\s+", " ", raw.replace("\n *", " "))
    for words in ("known = 12 - moves % 10", "rem = M - moves", "H = min(known, rem), the HORIZON", "the game is (L - lines, H)",
                  "THE SEARCH IS tpl_placement_exact_nodes' WITH shortest = 1", "pieces'[i][M - H + d] = q[d]", "BYTE FOR BYTE",
                  "VERDICT 3 PROVES NOTHING ABOUT THE GAME", "proved, not solved, and H == rem", "NOT SEARCHED",
                  "bound and horizon are still written"):
        assert words in flat, words
    # the body is shared between the two forms, not copied; the search loop is duplicated, the existing units are not part of it
    here = os.path.dirname(m._UNITS[0])
    units = [os.path.basename(p) for p in m._UNITS]
    assert "exact_window.hip" in units and "exact_window_move.hip" in units
    code = [l for l in open(os.path.join(here, "exact_window_move.hip")).read().splitlines() if l.strip() and not l.startswith("//")]
    assert code == ["#define TPL_PLACEMENT_MOVE_UNIT", "#define TPL_PLACEMENT_BOUND_UNIT", '#include "exact_window.hip"']
    body = open(os.path.join(here, "exact_window.hip")).read()
    assert "__syncthreads" not in body and '#include "exact' not in body and '#include "tpl_beam.h"' in body
    assert "extern __shared__" not in body                     # twelve records: static LDS
    for doc in ("README.md", "DESIGN.md"):
        words = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "window_prove" in words and "ProofPolicy" in words and "proves nothing" in words, doc
    assert "**Verdict 3 proves nothing" in open(os.path.join(ROOT, "README.md")).read()


def test_the_window_kernels_use_no_scratch_and_fill_a_simd_with_waves():
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
        assert 80 * 12 <= num(r, "lds") <= 160 * 1024 // 32, r               # the stack is static, and 32 waves a CU have theirs
