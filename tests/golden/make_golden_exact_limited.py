#!/usr/bin/env python3
"""Recorded outputs of the limited-discrepancy search's numpy mirror (_learn_lib.placement_exact_limited), for
tests/test_exact_limited_gpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_exact_limited.py [jobs]

As make_golden_exact.py, whose inputs these cases take (its generate_configs cases, its small games, its long game, its carved case):
the mirror is too slow for a GPU test, so it is run here once -- `jobs` processes share the cases --, and tests/test_exact_limited_cpu.py
recomputes a slice of every case with the mirror as it stands (slice_of() below), which pins this file to it.

  exact_limited_mirror.npz   per case of cases(), under its key: solved, proved, solution_len, actions, bound, nodes and limit as the
                             mirror returns them.  The inputs are not stored.
    cfg_*_k{K}_g{G}    generate_configs(3, 8, 64) and (5, 12, 32), seed 7, at max_nodes 1, 7, 256 and 4,000, first_limit K in 0, 1, 3 and
                       growth G in 0 ("add"), 1 ("double"); the fourteen weights on the second at 256 nodes;
    small_*_k{K}_g{G}  the six small games, shortest, both weight rows, under (0, add), (1, double) and (3, add);
    long_*             the M = 254 game at 300 nodes: under K = 0 the first iteration follows the first child of every node, so the stack
                       reaches its deepest records;
    carved_g{G}        make_golden_exact's carved case (32 configurations at a budget of their own sol_len, 4,000 nodes) from first_limit 0.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tetris_piclim as T  # noqa: E402
import make_golden_exact as G  # noqa: E402

NAMES = G.NAMES + ("limit",)
FIRST = (0, 1, 3)
GROWTH = (0, 1)                                                # "add", "double"
SMALL_RULES = ((0, 0), (1, 1), (3, 0))                        # (first_limit, growth)
LONG = ((105, False, 0, 0), (105, True, 3, 1))                # L, shortest, first_limit, growth


def cases():
    """[(key, arguments)]: make_golden_exact's arguments by name with first_limit and growth; the carved case apart (carved_case)."""
    out = []
    for L, M, count in G.CONFIGS:
        base = dict(source=("generate", L, M, count, G.CONFIG_SEED), L=L, M=M, F=12, shortest=True, spare_weight=0.0)
        for cap in G.CAPS:
            for first in FIRST:
                for growth in GROWTH:
                    out.append((f"cfg_L{L}_M{M}_c{cap}_k{first}_g{growth}", dict(base, max_nodes=cap, first_limit=first, growth=growth)))
    L, M, count = G.CONFIGS[1]
    for first, growth in ((0, 0), (1, 1)):
        out.append((f"cfg_L{L}_M{M}_c256_F14_k{first}_g{growth}",
                    dict(source=("generate", L, M, count, G.CONFIG_SEED), L=L, M=M, F=14, shortest=True, spare_weight=0.0, max_nodes=256,
                         first_limit=first, growth=growth)))
    for L, M, game_L, count in G.SMALL:
        for F in (12, 14):
            for first, growth in SMALL_RULES:
                out.append((f"small_L{L}_M{M}_g{game_L}_F{F}_k{first}_g{growth}",
                            dict(source=("generate", game_L, M, count, 31 + M), L=L, M=M, F=F, max_nodes=G.SMALL_NODES, shortest=True,
                                 spare_weight=0.0, first_limit=first, growth=growth)))
    for L, shortest, first, growth in LONG:
        out.append((f"long_L{L}_s{int(shortest)}_k{first}_g{growth}",
                    dict(source=("long",), L=L, M=G.LONG_M, F=12, shortest=shortest, spare_weight=0.0, max_nodes=G.LONG_NODES,
                         first_limit=first, growth=growth)))
    return out


def slice_of(key, n):
    """The configurations of a case that tests/test_exact_limited_cpu.py recomputes: three of a case that may run to 4,000 nodes, eight
    of one at 256, all of the others."""
    if "_c4000_" in key:
        return np.array([0, n // 2, n - 1])
    if "_c256_" in key:
        return np.arange(0, n, max(1, n // 8))[:8]
    return np.arange(n)


def run_case(m, args, pick=None):
    rows, pieces = G.inputs(args)
    if pick is not None:
        rows, pieces = rows[pick], pieces[pick]
    got = m.placement_exact_limited(rows, pieces, args["L"], args["M"], G.weights()[args["F"]], args["max_nodes"], args["first_limit"],
                                    args["growth"], shortest=args["shortest"], spare_weight=args["spare_weight"])
    return dict(zip(NAMES, got))


def carved_case(m, growth, first_limit=0, pick=None):
    """make_golden_exact's carved case under the limited rule: its configurations -- or those of `pick` -- grouped by budget."""
    rows, pieces, sol_len, L, M = G.carved_inputs()
    pick = np.arange(G.CARVED_COUNT) if pick is None else np.asarray(pick)
    out = dict(solved=np.zeros(pick.size, np.uint8), proved=np.zeros(pick.size, np.uint8), solution_len=np.zeros(pick.size, np.int32),
               actions=np.full((pick.size, M), 255, np.uint8), bound=np.zeros(pick.size, np.int32), nodes=np.zeros(pick.size, np.uint32),
               limit=np.zeros(pick.size, np.int32))
    for budget in np.unique(sol_len[pick]):
        at = np.flatnonzero(sol_len[pick] == budget)
        idx = pick[at]
        got = m.placement_exact_limited(rows[idx], pieces[idx, :budget + 1], L, int(budget), T.CLASSICAL_WEIGHTS, G.CARVED_NODES,
                                        first_limit, growth)
        for name, x in zip(NAMES, got):
            if x.ndim == 2:
                out[name][at, :budget] = x
            else:
                out[name][at] = x
    return out


def _work(job):
    m = T._learn_lib
    t0 = time.time()
    key, args = job
    got = carved_case(m, args["growth"]) if key.startswith("carved") else run_case(m, args)
    return key, got, time.time() - t0


def main():
    jobs = [(f"carved_g{growth}", dict(growth=growth)) for growth in GROWTH] + cases()
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    if workers > 1:
        import multiprocessing
        with multiprocessing.Pool(workers) as pool:
            done = pool.map(_work, jobs, chunksize=1)
    else:
        done = [_work(job) for job in jobs]
    out = {}
    for key, got, seconds in done:
        for name in NAMES:
            out[f"{key}_{name}"] = got[name]
        print(f"{key}: n {got['solved'].size}, proved {int(got['proved'].sum())}, solved {int(got['solved'].sum())}, nodes max "
              f"{int(got['nodes'].max())} mean {got['nodes'].mean():.1f}, limit max {int(got['limit'].max())}, {seconds:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "exact_limited_mirror.npz"), **out)


if __name__ == "__main__":
    main()
