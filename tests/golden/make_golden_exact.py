#!/usr/bin/env python3
"""Recorded outputs of the exact depth-first solver's numpy mirror (_learn_lib.placement_exact), for tests/test_exact_gpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_exact.py

As make_golden_bound.py: the mirror is too slow for a GPU test, so it is run here once, and tests/test_exact_cpu.py recomputes a slice
of every case with the mirror as it stands (slice_of() below says which configurations; the carved case whole), which pins this file to
it.  The rest is trusted as recorded: after a change of the mirror that could show only there, run this script again and compare.

  exact_mirror.npz   per case of cases(), under its key: solved, proved, solution_len, actions, bound and nodes as the mirror returns
                     them.  The inputs are not stored: inputs() makes them again from the host generators and the committed fixtures.
    small_*          test_solve_cpu's six small games -- boards carved for game_L lines, searched for L --, both values of
                     `shortest`, twelve weights (the classical row) and fourteen (Dellacherie's), a node budget that is never reached;
    cfg_*            generate_configs(3, 8, 64) and (5, 12, 32), seed 7, searched at their full M, so that the budget deepens, at
                     max_nodes 1, 7, 256 and 4,000; and on one of them spare_weight = 1, the fourteen weights, shortest = 0, n = 1, and the
                     (3, 8) boards searched for four lines in six moves, where a search of a thousand nodes and more proves that there
                     is no win;
    carved           the first 32 configurations of carved_L10_M40.npz, each at a budget of ITS OWN sol_len (grouped by budget as
                     make_golden_bound.py groups them), max_nodes = 4,000; actions [32, 40], 255 behind each budget;
    long_*           long_rows / long_pieces of solve_mirror.npz at M = 254 with max_nodes = 300: at shortest = 0 the descent follows
                     the first child of every node, so the stack reaches its deepest records.
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

NAMES = ("solved", "proved", "solution_len", "actions", "bound", "nodes")
SMALL = ((1, 1, 1, 24), (1, 2, 1, 24), (2, 2, 1, 24), (2, 2, 2, 24), (2, 3, 2, 6), (2, 3, 1, 6))     # L, M, game_L, count
SMALL_NODES = 1 << 16                                         # never reached: a game of three moves has 1 + 34 + 34 * 34 nodes at most
CONFIGS = ((3, 8, 64), (5, 12, 32))                           # L, M, count
CONFIG_SEED = 7
CAPS = (1, 7, 256, 4000)
CARVED, CARVED_COUNT, CARVED_NODES = "carved_L10_M40.npz", 32, 4000
LONG_M, LONG_NODES = 254, 300
LONG = ((105, False), (105, True), (112, False))              # L, shortest


def weights():
    return {12: np.array(T.CLASSICAL_WEIGHTS), 14: np.array(T.DELLACHERIE_WEIGHTS)}


def cases():
    """[(key, arguments)]: every case but the carved one, which is grouped by budget (carved_case).  The arguments are
    placement_exact's by name, with rows and pieces made when asked for (inputs)."""
    out = []
    for L, M, game_L, count in SMALL:
        for F in (12, 14):
            for shortest in (True, False):
                out.append((f"small_L{L}_M{M}_g{game_L}_F{F}_s{int(shortest)}",
                            dict(source=("generate", game_L, M, count, 31 + M), L=L, M=M, F=F, max_nodes=SMALL_NODES,
                                 shortest=shortest, spare_weight=0.0)))
    for L, M, count in CONFIGS:
        base = dict(source=("generate", L, M, count, CONFIG_SEED), L=L, M=M, F=12, shortest=True, spare_weight=0.0)
        for cap in CAPS:
            out.append((f"cfg_L{L}_M{M}_c{cap}", dict(base, max_nodes=cap)))
    L, M, count = CONFIGS[0]
    base = dict(source=("generate", L, M, count, CONFIG_SEED), L=L, M=M, F=12, shortest=True, spare_weight=0.0, max_nodes=256)
    out.append((f"cfg_L{L}_M{M}_c256_spare", dict(base, spare_weight=1.0)))
    out.append((f"cfg_L{L}_M{M}_c4000_first", dict(base, shortest=False, max_nodes=4000)))
    out.append((f"cfg_L{L}_M{M}_c256_one", dict(base, source=("generate", L, M, 1, CONFIG_SEED))))
    out.append((f"cfg_L{L + 1}_M{M - 2}_c4000_owed", dict(base, L=L + 1, M=M - 2, max_nodes=4000)))       # a line more, two moves fewer
    L, M, count = CONFIGS[1]
    out.append((f"cfg_L{L}_M{M}_c256_F14", dict(source=("generate", L, M, count, CONFIG_SEED), L=L, M=M, F=14, shortest=True,
                                                 spare_weight=0.0, max_nodes=256)))
    for L, shortest in LONG:
        out.append((f"long_L{L}_s{int(shortest)}", dict(source=("long",), L=L, M=LONG_M, F=12, shortest=shortest, spare_weight=0.0,
                                                        max_nodes=LONG_NODES)))
    return out


def inputs(args):
    """(rows, pieces [n, M + 1]) of a case: its source's configurations, the piece lists cut to the case's M."""
    source = args["source"]
    if source[0] == "generate":
        _, L, M, count, seed = source
        rows, pieces = T.generate_configs(L, M, count, seed=seed)
    else:
        g = np.load(os.path.join(HERE, "solve_mirror.npz"))
        rows, pieces = g["long_rows"], g["long_pieces"]
    return rows, np.ascontiguousarray(pieces[:, :args["M"] + 1])


def slice_of(key, n):
    """The configurations of a case that tests/test_exact_cpu.py recomputes: all of a small game, of a low cap and of the long games,
    six of a case that may run to 4,000 nodes."""
    if "c4000" in key:
        return np.array([0, 1, 2, n // 2, n - 2, n - 1])
    return np.arange(n)


def run_case(m, args, pick=None):
    rows, pieces = inputs(args)
    if pick is not None:
        rows, pieces = rows[pick], pieces[pick]
    got = m.placement_exact(rows, pieces, args["L"], args["M"], weights()[args["F"]], args["max_nodes"], shortest=args["shortest"],
                            spare_weight=args["spare_weight"])
    return dict(zip(NAMES, got))


def carved_inputs():
    f = np.load(os.path.join(HERE, CARVED))
    return f["rows"][:CARVED_COUNT], f["pieces"][:CARVED_COUNT], f["sol_len"][:CARVED_COUNT].astype(np.int64), int(f["L"]), int(f["M"])


def carved_groups(sol_len):
    """[(budget, indices)] in ascending budget: the configurations searched at M = budget = sol_len."""
    return [(int(b), np.flatnonzero(sol_len == b)) for b in np.unique(sol_len)]


def carved_gather(parts, n, M):
    """The outputs of the carved case's groups, [(indices, budget, six arrays)], in the configurations' order and one width M."""
    out = dict(solved=np.zeros(n, np.uint8), proved=np.zeros(n, np.uint8), solution_len=np.zeros(n, np.int32),
               actions=np.full((n, M), 255, np.uint8), bound=np.zeros(n, np.int32), nodes=np.zeros(n, np.uint32))
    for idx, budget, got in parts:
        for name, x in zip(NAMES, got):
            if x.ndim == 2:
                out[name][idx, :budget] = x
            else:
                out[name][idx] = x
    return out


def carved_case(m):
    rows, pieces, sol_len, L, M = carved_inputs()
    parts = []
    for budget, idx in carved_groups(sol_len):
        got = m.placement_exact(rows[idx], pieces[idx, :budget + 1], L, budget, T.CLASSICAL_WEIGHTS, CARVED_NODES)
        parts.append((idx, budget, got))
    return carved_gather(parts, CARVED_COUNT, M)


def main():
    m = T._learn_lib
    out = {}
    for key, args in cases():
        t0 = time.time()
        got = run_case(m, args)
        for name in NAMES:
            out[f"{key}_{name}"] = got[name]
        n = got["solved"].size
        print(f"{key}: n {n}, proved {int(got['proved'].sum())}, solved {int(got['solved'].sum())}, unwinnable "
              f"{int((got['proved'] & (1 - got['solved'])).sum())}, longest {int(got['solution_len'].max())}, nodes max "
              f"{int(got['nodes'].max())} mean {got['nodes'].mean():.1f}, {time.time() - t0:.1f}s", flush=True)
    t0 = time.time()
    got = carved_case(m)
    for name in NAMES:
        out[f"carved_{name}"] = got[name]
    print(f"carved: proved {int(got['proved'].sum())}, solved {int(got['solved'].sum())} of {CARVED_COUNT}, nodes {got['nodes'].tolist()}, "
          f"{time.time() - t0:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "exact_mirror.npz"), **out)


if __name__ == "__main__":
    main()
