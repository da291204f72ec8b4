#!/usr/bin/env python3
"""Recorded outputs of the whole-game solver's numpy mirror (_learn_lib.placement_solve), for tests/test_solve_gpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_solve.py

The mirror moves and counts every candidate on 20 x 10 cell arrays: a width-64 case of 128 configurations takes it ten to twenty
seconds, the 254-move games half a minute, far beyond what a GPU test may spend.  So it is run here, once, on inputs made on the
host, and tests/test_solve_cpu.py recomputes a slice of every case with the mirror as it stands, which pins this file to it.

  solve_mirror.npz   per (L, M) in CASES: 64 carved configurations (generate_configs, seed SEED) followed by 64 synthetic ones (the
                     oracle's synth_boards / synth_pieces, seed SEED: what env.synthetic_configs makes on the device), and per
                     width in WIDTHS the mirror's solved, solution_len, actions and best_value under CLASSICAL_WEIGHTS;
                     the LONG games: 4 synthetic configurations at M = 254, width 64, one line goal that is reached after some 250
                     moves and one that is not reached.
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
from oracle import oracle as O  # noqa: E402

CASES = ((1, 1), (2, 6), (3, 13), (5, 20))
WIDTHS = (1, 3, 16, 64)
SEED, CARVED, SYNTHETIC = 7, 64, 64
LONG_M, LONG_WIDTH, LONG_COUNT, LONG_SEED, LONG_BOARD_L = 254, 64, 4, 11, 10
LONG_GOALS = (105, 112)


def inputs(L, M):
    rows, pieces = T.generate_configs(L, M, CARVED, seed=SEED)
    return (np.concatenate([rows, O.synth_boards(SEED, 0, SYNTHETIC, L)]),
            np.concatenate([pieces, O.synth_pieces(SEED, 0, SYNTHETIC, M)]))


def long_inputs():
    return O.synth_boards(LONG_SEED, 0, LONG_COUNT, LONG_BOARD_L), O.synth_pieces(LONG_SEED, 0, LONG_COUNT, LONG_M)


def main():
    m = T._learn_lib
    out = {}
    for L, M in CASES:
        rows, pieces = inputs(L, M)
        out[f"L{L}_M{M}_rows"], out[f"L{L}_M{M}_pieces"] = rows, pieces
        for W in WIDTHS:
            t0 = time.time()
            solved, length, actions, best = m.placement_solve(rows, pieces, L, M, T.CLASSICAL_WEIGHTS, W)
            key = f"L{L}_M{M}_W{W}_"
            out[key + "solved"], out[key + "solution_len"], out[key + "actions"], out[key + "best_value"] = solved, length, actions, best
            print(f"L={L} M={M} W={W}: solved {int(solved[:CARVED].sum())}/{CARVED} carved, {int(solved[CARVED:].sum())}/{SYNTHETIC} "
                  f"synthetic, longest {int(length.max())}, {time.time() - t0:.1f}s", flush=True)
    rows, pieces = long_inputs()
    out["long_rows"], out["long_pieces"] = rows, pieces
    for L in LONG_GOALS:
        t0 = time.time()
        solved, length, actions, best = m.placement_solve(rows, pieces, L, LONG_M, T.CLASSICAL_WEIGHTS, LONG_WIDTH)
        key = f"long_L{L}_"
        out[key + "solved"], out[key + "solution_len"], out[key + "actions"], out[key + "best_value"] = solved, length, actions, best
        print(f"long L={L}: solved {solved.tolist()} lengths {length.tolist()}, {time.time() - t0:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "solve_mirror.npz"), **out)


if __name__ == "__main__":
    main()
