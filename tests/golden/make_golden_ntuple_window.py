#!/usr/bin/env python3
"""Recorded outputs of the table-ordered window search's numpy mirror (_learn_lib.ntuple_window_prove), for
tests/test_ntuple_window_cpu.py and tests/test_ntuple_window_gpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_ntuple_window.py

tests/test_ntuple_window_cpu.py recomputes every case with the mirror as it stands, which pins this file to it.  Nothing is stored but
the mirror's outputs: the states are make_golden_window.py's (root_states, mid_states, loss_states) and the tables
make_golden_ntuple_exact.py's (table(form, kind)), both imported and not changed.

  ntuple_window_mirror.npz   per case of CASES, under its key: solved, proved, solution_len, plan, bound, nodes, horizon, verdict, known.
    A key is <states>_<table>_<what>:
      states  root_M10, root_M20   the reset boards of the first 16 configurations of carved_L5_M20.npz in (5, 10) and (5, 20);
              mid                  make_golden_window's 96 running boards at counters 1, 9, 10, 11, 19 and four finished ones, (5, 20);
              mid10                the same boards in the game (5, 10): counters 1 and 9 run (H = 9 and 1), the others are finished;
              loss_small, loss_owed  the games (2, 3) and (4, 6) whose boards the search proves unwinnable;
      table   linear, budget ("feat+spare" linear and hashed), feat, 3x3, 2x4 (hashed), ties (the zero "feat+spare" table with reward
              (0, 0, 0): every key ties, the order is b alone), huge (the "feat+spare" table whose sums are rounded);
      what    c<max_nodes>; skip: every third board skipped; gamma: gamma 0.5 with reward (1, 10, -1).
    `mid` is run at 64 and at 1,024 nodes under all five tables, and so are the reset boards under the two window forms.  Those walk
    some 150 tuples a board in the mirror, so the small game and `mid10` have them at 1 and 64 nodes.
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
import make_golden_window as W  # noqa: E402  -- the states
import make_golden_ntuple_exact as N  # noqa: E402  -- the tables

NAMES = W.NAMES
TABLES = {"linear": (N.BUDGET, "linear"), "budget": (N.BUDGET, "hashed"), "feat": (N.FEAT, "hashed"), "3x3": ("3x3", "hashed"),
          "2x4": ("2x4", "hashed"), "ties": (N.BUDGET, "zero"), "huge": (N.BUDGET, "huge")}
FIVE = ("linear", "budget", "feat", "3x3", "2x4")
CHEAP = ("linear", "budget", "feat")                           # ten or eleven gathers a board: the reset boards at 1,024 alone, the small game at 1,024 too
PLAIN = dict(gamma=1.0, reward=(1.0, 0.0, 0.0), skip=None)


def mid10_states():
    return dict(W.mid_states(), M=10)


STATES = {"root_M10": lambda: W.root_states(10), "root_M20": lambda: W.root_states(20), "mid": W.mid_states, "mid10": mid10_states,
          "loss_small": lambda: W.loss_states("loss_small"), "loss_owed": lambda: W.loss_states("loss_owed")}


def _cases():
    out = {}
    for tag in FIVE:
        for cap in (W.CAP,) if tag in CHEAP else (64, W.CAP):
            for states in ("root_M10", "root_M20"):
                out[f"{states}_{tag}_c{cap}"] = dict(PLAIN, states=states, table=tag, max_nodes=cap)
        out[f"mid_{tag}_c64"] = dict(PLAIN, states="mid", table=tag, max_nodes=64)
        out[f"mid_{tag}_c{W.CAP}"] = dict(PLAIN, states="mid", table=tag, max_nodes=W.CAP)
    for tag in ("budget", "feat", "3x3", "2x4"):
        out[f"mid_{tag}_c1"] = dict(PLAIN, states="mid", table=tag, max_nodes=1)
        out[f"root_M20_{tag}_c1"] = dict(PLAIN, states="root_M20", table=tag, max_nodes=1)
        for cap in (1, 64) + ((W.CAP,) if tag in CHEAP else ()):
            out[f"loss_small_{tag}_c{cap}"] = dict(PLAIN, states="loss_small", table=tag, max_nodes=cap)
    out["mid_budget_skip"] = dict(PLAIN, states="mid", table="budget", max_nodes=W.CAP, skip=3)
    out["mid_budget_gamma"] = dict(PLAIN, states="mid", table="budget", max_nodes=64, gamma=0.5, reward=(1.0, 10.0, -1.0))
    out["mid_ties_c64"] = dict(PLAIN, states="mid", table="ties", max_nodes=64, reward=(0.0, 0.0, 0.0))
    out["mid_huge_c64"] = dict(PLAIN, states="mid", table="huge", max_nodes=64)
    out[f"mid10_budget_c{W.CAP}"] = dict(PLAIN, states="mid10", table="budget", max_nodes=W.CAP)
    out["mid10_3x3_c64"] = dict(PLAIN, states="mid10", table="3x3", max_nodes=64)
    out["mid10_2x4_c64"] = dict(PLAIN, states="mid10", table="2x4", max_nodes=64)
    out["loss_small_budget_c65536"] = dict(PLAIN, states="loss_small", table="budget", max_nodes=1 << 16)
    out["loss_owed_budget_c16384"] = dict(PLAIN, states="loss_owed", table="budget", max_nodes=1 << 14)
    return out


CASES = _cases()


def table_of(key):
    return N.table(*TABLES[CASES[key]["table"]])


def states_of(key):
    return STATES[CASES[key]["states"]]()


def skip_of(case, n):
    return None if case["skip"] is None else (np.arange(n) % case["skip"] == 0).astype(np.uint8)


def run_case(m, key):
    case = CASES[key]
    s = states_of(key)
    return m.ntuple_window_prove(s["rows"], s["lines"], s["moves"], s["state"], s["window"], s["L"], s["M"], table_of(key),
                                 case["max_nodes"], gamma=case["gamma"], reward=case["reward"], skip=skip_of(case, s["rows"].shape[0]))


def main():
    m = T._learn_lib
    out = {}
    for key in CASES:
        t0 = time.time()
        got = run_case(m, key)
        for name in NAMES:
            out[f"{key}_{name}"] = got[name]
        print(f"{key}: n {got['verdict'].size}, verdicts {np.bincount(got['verdict'], minlength=4).tolist()}, horizons "
              f"{sorted(set(got['horizon'].tolist()))}, proved {int(got['proved'].sum())}, nodes max {int(got['nodes'].max())} sum "
              f"{int(got['nodes'].sum())}, {time.time() - t0:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "ntuple_window_mirror.npz"), **out)


if __name__ == "__main__":
    main()
