#!/usr/bin/env python3
"""Recorded outputs of the window search's numpy mirror (_learn_lib.placement_window_prove), for tests/test_window_cpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_window.py

tests/test_window_cpu.py recomputes every case with the mirror as it stands, which pins this file to it, and takes the cases' inputs
from states() below.  Nothing is stored but the mirror's outputs: the inputs are made again from the committed fixtures and the host
generator.

  window_mirror.npz   per case of CASES, under its key: solved, proved, solution_len, plan, bound, nodes, horizon, verdict and known.
    root_M10, root_M20  the first 16 configurations of carved_L5_M20.npz as reset boards, the window = pieces[:, :12], in the games
                        (5, 10) -- H = rem = 10 -- and (5, 20) -- H = 12 < rem; classical weights, max_nodes = 1,024;
    mid, mid_F14        boards of the fixture's recorded replays with the window rebuilt from the list, in the game (5, 20), at move
                        counters 1, 9, 10, 11 and 19 (known 11, 3, 12, 11, 3; at 19 H = rem = 1), and finished boards (won, lost,
                        lines = L, moves = M) among them; the twelve weights at 1,024 nodes and the fourteen at 64.  The recorded
                        solutions are 3 to 10 moves long, so only counter 1 is the replay's own: for the others the board is the one
                        three moves before its solution's end, with the pieces that follow it, and the counter is SET; a last
                        group at counter 9 lies four moves before the end, so that its three known pieces decide nothing;
    mid_cap1            `mid` at max_nodes = 1: a search that needs a second node is stopped, verdict 3;
    mid_skip            `mid` with every third board skipped;
    loss_small          make_golden_exact's small game (2, 3) on boards carved for one line: H = rem = 3, and the boards that the
                        move bound lets live and the search then searches out without a win get verdict 2;
    loss_owed           the first sixteen of make_golden_exact's generate_configs(3, 8, 64) boards searched for four lines in six
                        moves (H = rem = 6), where searches of up to a few thousand nodes prove that there is no win.
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

NAMES = ("solved", "proved", "solution_len", "plan", "bound", "nodes", "horizon", "verdict", "known")
FIXTURE, COUNT, L5, CAP = "carved_L5_M20.npz", 16, 5, 1024
COUNTERS = (1, 9, 10, 11, 19)
BACK = 3                                                      # a set counter's board: this many moves before its solution's end
GROUPS = tuple((m, BACK) for m in COUNTERS) + ((9, BACK + 1),)    # (counter, back): the last knows three pieces and needs four moves
# L, M, and the boards: generate_configs(game_L, game_M, count, seed)[:take]
LOSS = {"loss_small": (2, 3, 1, 3, 6, 6, 34), "loss_owed": (4, 6, 3, 8, 64, 16, 7)}


def weights(F):
    return np.array(T.CLASSICAL_WEIGHTS) if F == 12 else np.array(T.DELLACHERIE_WEIGHTS)


def pack_window(entries):
    """[n, k <= 12] piece ids -> the 36-bit windows, entry j at bits 3 j; entries that are not given are 0."""
    entries = np.asarray(entries).astype(np.uint64) & np.uint64(7)
    return (entries << (np.uint64(3) * np.arange(entries.shape[1], dtype=np.uint64))).sum(axis=1).astype(np.uint64)


def window_from_list(pieces, start, known):
    """The window of a board whose next piece is pieces[start]: `known` true entries, 0 behind them and behind the list's end."""
    pieces = np.asarray(pieces)
    out = np.zeros(12, np.int64)
    take = max(0, min(int(known), pieces.size - int(start)))
    out[:take] = pieces[start:start + take]
    return out


def fixture():
    return np.load(os.path.join(HERE, FIXTURE))


def root_states(M):
    g = fixture()
    z = np.zeros(COUNT, np.int64)
    return dict(rows=g["rows"][:COUNT], lines=z, moves=z, state=z, window=pack_window(g["pieces"][:COUNT, :12]), L=L5, M=M)


def mid_states():
    """One launch: for every group of GROUPS the 16 boards, then four finished boards.  `played` is how many of the list's pieces lie behind
    the board (the window starts there) and `config` the configuration."""
    g = fixture()
    M = int(g["M"])
    rows, lines, moves, state, window, played, config = [], [], [], [], [], [], []
    for m, back in GROUPS:
        for i in range(COUNT):
            k = 1 if m == 1 else int(g["sol_len"][i]) - back
            assert k >= 1 and g["r_state"][i, k - 1] == 0 and g["r_moves"][i, k - 1] == k
            rows.append(g["r_rows"][i, k - 1]); lines.append(int(g["r_lines"][i, k - 1])); moves.append(m); state.append(0)
            window.append(window_from_list(g["pieces"][i], k, 12 - m % 10)); played.append(k); config.append(i)
    for st, ln, mv in ((1, 5, 7), (2, 3, 20), (0, 5, 7), (0, 2, 20)):      # won, lost at the limit, lines = L, moves = M
        rows.append(g["rows"][0]); lines.append(ln); moves.append(mv); state.append(st)
        window.append(window_from_list(g["pieces"][0], 0, 12)); played.append(0); config.append(0)
    return dict(rows=np.array(rows, np.uint16), lines=np.array(lines), moves=np.array(moves), state=np.array(state),
                window=pack_window(np.array(window)), L=L5, M=M, played=np.array(played), config=np.array(config))


def loss_states(key):
    L, M, game_L, game_M, count, take, seed = LOSS[key]
    rows, pieces = T.generate_configs(game_L, game_M, count, seed=seed)
    rows, pieces = rows[:take], pieces[:take]
    z = np.zeros(take, np.int64)
    return dict(rows=rows, lines=z, moves=z, state=z, window=pack_window(pieces[:, :M]), L=L, M=M, pieces=pieces)


CASES = {
    "root_M10": dict(states=lambda: root_states(10), F=12, max_nodes=CAP, skip=None),
    "root_M20": dict(states=lambda: root_states(20), F=12, max_nodes=CAP, skip=None),
    "mid": dict(states=mid_states, F=12, max_nodes=CAP, skip=None),
    "mid_F14": dict(states=mid_states, F=14, max_nodes=64, skip=None),
    "mid_cap1": dict(states=mid_states, F=12, max_nodes=1, skip=None),
    "mid_skip": dict(states=mid_states, F=12, max_nodes=CAP, skip=3),
    "loss_small": dict(states=lambda: loss_states("loss_small"), F=12, max_nodes=1 << 16, skip=None),
    "loss_owed": dict(states=lambda: loss_states("loss_owed"), F=12, max_nodes=1 << 14, skip=None),
}


def skip_of(case, n):
    return None if case["skip"] is None else (np.arange(n) % case["skip"] == 0).astype(np.uint8)


def run_case(m, key):
    case = CASES[key]
    s = case["states"]()
    return m.placement_window_prove(s["rows"], s["lines"], s["moves"], s["state"], s["window"], s["L"], s["M"], weights(case["F"]),
                                    case["max_nodes"], skip=skip_of(case, s["rows"].shape[0]))


def main():
    m = T._learn_lib
    out = {}
    for key in CASES:
        t0 = time.time()
        got = run_case(m, key)
        for name in NAMES:
            out[f"{key}_{name}"] = got[name]
        print(f"{key}: n {got['verdict'].size}, verdicts {np.bincount(got['verdict'], minlength=4).tolist()}, horizons "
              f"{sorted(set(got['horizon'].tolist()))}, nodes max {int(got['nodes'].max())}, {time.time() - t0:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "window_mirror.npz"), **out)


if __name__ == "__main__":
    main()
