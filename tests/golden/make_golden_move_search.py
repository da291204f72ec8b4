#!/usr/bin/env python3
"""Recorded two-ply choices of the numpy mirror in the 14-feature form, for tests/test_move_features_gpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_move_search.py

The mirror makes 1,600 moves and counts 1,600 boards for every state: 2,048 states take it about a minute, far beyond what a GPU test
may spend.  So it is run here, once, on states made on the host, and tests/test_move_features_cpu.py recomputes a slice with the mirror
as it stands and regenerates the states, which pins this file to both.

  move_search_mirror.npz   A, B: the planes of test_move_features_cpu.search_states(); weights, per: its population(2048), three rows
                           with a short last member; action, second, score: mirror_search's choice of every state under its row.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_move_features_cpu as C  # noqa: E402


def main():
    t0 = time.time()
    A, B = C.search_states()
    w, per = C.population(C.SEARCH_N)
    s = C.MirrorStates(A, B, C.SEARCH_L, C.SEARCH_M)
    action, second, score = C.mirror_search(s, np.arange(C.SEARCH_N), w[np.arange(C.SEARCH_N) // per])
    np.savez_compressed(os.path.join(HERE, "move_search_mirror.npz"), A=A, B=B, weights=w, per=np.int64(per), action=action,
                        second=second, score=score)
    print(f"{C.SEARCH_N} states, {int(s.running.sum())} running, {int((second != 255).sum())} with a second ply, "
          f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
