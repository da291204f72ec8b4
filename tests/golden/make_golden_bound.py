#!/usr/bin/env python3
"""Recorded outputs of the BOUNDED whole-game solver's numpy mirror (_learn_lib.placement_solve(bound=True)), for
tests/test_bound_gpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_bound.py

As make_golden_solve.py: the mirror is far too slow for a GPU test, so it is run here once, and tests/test_bound_cpu.py recomputes a
slice of every case with the mirror as it stands, which pins this file to it.  The slice: at widths 1, 3 and 16 one (slack,
spare_weight) combination of every (case, feature form, width) in turn, at width 64 every combination at (2, 6) and one per feature
form at (3, 13).  The rest -- three quarters of the arrays at the narrow widths, and width 64 at (1, 1), (5, 20) and most of (3, 13)
-- is trusted as recorded: after a change of the mirror that could show only there, run this script again and compare.

  bound_mirror.npz   per (L, M) in CASES: COUNT carved configurations with their solutions' lengths (generate_configs, seed SEED), the
                     piece lists one piece longer than carving made them (piece (3 i + 1) mod 7 behind configuration i's), so that a
                     budget of sol_len + 1 has its M + 1 pieces even where sol_len = M.  Every configuration is searched at a budget of
                     ITS OWN sol_len + s, s in SLACKS -- a loose budget would never let the bound bite -- so the configurations of a
                     case are grouped by budget (groups(): ascending budget, the piece lists cut to budget + 1) and every group is one
                     call.  Per width in WIDTHS, weight row in WEIGHTS (twelve: the classical row; fourteen: Dellacherie's) and
                     spare_weight in SPARES: solved, solution_len, bound and complete [COUNT], actions and best_value [COUNT, M + 1]
                     (255 and +0 behind each configuration's budget), in the configurations' order;
                     the LONG game: long_rows / long_pieces of solve_mirror.npz at L = 105, M = 254, width 8, bounded, spare_weight 0.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

import tetris_piclim as T  # noqa: E402

CASES = ((1, 1), (2, 6), (3, 13), (5, 20))
WIDTHS = (1, 3, 16, 64)
SLACKS = (0, 1)
SPARES = (0.0, 0.25)
SEED, COUNT = 7, 32
LONG_L, LONG_M, LONG_WIDTH = 105, 254, 8
NAMES = ("solved", "solution_len", "actions", "best_value", "bound", "complete")


def weights():
    return {12: np.array(T.CLASSICAL_WEIGHTS), 14: np.array(T.DELLACHERIE_WEIGHTS)}


def inputs(L, M):
    """(rows, pieces [COUNT, M + 2], sol_len) of a case."""
    rows, pieces, _, sol_len = T.generate_configs(L, M, COUNT, seed=SEED, with_solutions=True)
    extra = ((3 * np.arange(COUNT) + 1) % 7).astype(np.uint8)
    return rows, np.concatenate([pieces, extra[:, None]], axis=1), sol_len


def groups(sol_len, slack):
    """[(budget, indices)] in ascending budget: the configurations searched at M = budget = sol_len + slack."""
    budget = sol_len.astype(np.int64) + slack
    return [(int(b), np.flatnonzero(budget == b)) for b in np.unique(budget)]


def gather(parts, sol_len, slack, M):
    """The outputs of a case's groups, [(indices, budget, six arrays)], in the configurations' order and one width M + 1."""
    n = sol_len.shape[0]
    out = dict(solved=np.zeros(n, np.uint8), solution_len=np.zeros(n, np.int32), actions=np.full((n, M + 1), 255, np.uint8),
               best_value=np.zeros((n, M + 1), np.float32), bound=np.zeros(n, np.int32), complete=np.zeros(n, np.uint8))
    for idx, budget, got in parts:
        for name, x in zip(NAMES, got):
            if x.ndim == 2:
                out[name][idx, :budget] = x
            else:
                out[name][idx] = x
    return out


def solve_case(m, rows, pieces, sol_len, L, M, slack, w, width, spare, bound=True):
    parts = []
    for budget, idx in groups(sol_len, slack):
        got = m.placement_solve(rows[idx], pieces[idx, :budget + 1], L, budget, w, width, bound=bound, spare_weight=spare)
        parts.append((idx, budget, got))
    return gather(parts, sol_len, slack, M)


def main():
    m = T._learn_lib
    out = {}
    for L, M in CASES:
        rows, pieces, sol_len = inputs(L, M)
        out[f"L{L}_M{M}_rows"], out[f"L{L}_M{M}_pieces"], out[f"L{L}_M{M}_sol_len"] = rows, pieces, sol_len
        for F, w in weights().items():
            for W in WIDTHS:
                t0 = time.time()
                differs = []
                for slack in SLACKS:
                    plain = solve_case(m, rows, pieces, sol_len, L, M, slack, w, W, 0.0, bound=False)
                    for spare in SPARES:
                        got = solve_case(m, rows, pieces, sol_len, L, M, slack, w, W, spare)
                        key = f"L{L}_M{M}_F{F}_W{W}_s{slack}_p{int(spare * 100)}_"
                        for name in NAMES:
                            out[key + name] = got[name]
                        differs.append(int(sum((got[name].view(np.uint8) != plain[name].view(np.uint8)).reshape(COUNT, -1).any(axis=1)
                                                for name in NAMES[:4]).astype(bool).sum()))
                        last = got
                print(f"L={L} M={M} F={F} W={W}: configurations that differ from the unbounded mirror per (slack, spare) {differs}, "
                      f"solved {int(last['solved'].sum())}/{COUNT}, complete {int(last['complete'].sum())}, {time.time() - t0:.1f}s",
                      flush=True)
    g = np.load(os.path.join(HERE, "solve_mirror.npz"))
    t0 = time.time()
    got = m.placement_solve(g["long_rows"], g["long_pieces"], LONG_L, LONG_M, T.CLASSICAL_WEIGHTS, LONG_WIDTH, bound=True)
    for name, x in zip(NAMES, got):
        out[f"long_L{LONG_L}_{name}"] = x
    print(f"long L={LONG_L}: solved {got[0].tolist()} lengths {got[1].tolist()} bound {got[4].tolist()} complete {got[5].tolist()}, "
          f"{time.time() - t0:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "bound_mirror.npz"), **out)


if __name__ == "__main__":
    main()
