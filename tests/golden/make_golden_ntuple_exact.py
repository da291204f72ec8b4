#!/usr/bin/env python3
"""Recorded outputs of the table-ordered exact solver's numpy mirror (_learn_lib.ntuple_exact), for tests/test_ntuple_exact_gpu.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_ntuple_exact.py

As make_golden_exact.py: the mirror is too slow for a GPU test, so it is run here once, and tests/test_ntuple_exact_cpu.py recomputes a
slice of every case with the mirror as it stands (slice_of() below), which pins this file to it.  The inputs are make_golden_exact.py's
own (inputs, carved_inputs, the long games), imported and not copied.

The tables are NOT stored -- a window table is megabytes --: table(form, kind) makes them again from a closed-form integer hash of the
entry index,
    h(j) = mix(j * 0x9E3779B97F4A7C15 + HASH_SALT),  mix the splitmix64 finaliser, all in 64 bits
    zero     every entry 0
    hashed   h(j) mod (2^19 + 1) - 2^18: entries in +-2^18, so that a child's value is a few units and the order a thorough shuffle
    huge     +-(2^30 - (h(j) >> 20) mod 2^12), the sign bit 63 of h(j): the 64-bit sum of ten entries passes 2^24, so the one
             rounding to float32 shows
    linear   a feature or budget table alone: row j < 9 of every piece holds -LINEAR[j] * q * 2^12 in bin q and everything else 0, the
             classical signs on the nine board features -- a table that plays well enough for a descent to go as deep as the game

  ntuple_exact_mirror.npz   per case of cases(), under its key: solved, proved, solution_len, actions, bound and nodes
    small_*    test_solve_cpu's six small games, both values of `shortest`, the zero and the hashed "feat+spare" table;
    cfg_*      generate_configs(3, 8, 64) at max_nodes 1, 7, 256 and 4,000 and (5, 12, 32) at 7, 256 and 4,000 and the (3, 8) boards
               searched for four lines in six moves at 4,000, under the hashed "feat+spare" and "feat" tables; and on (3, 8, 64) under
               "feat+spare": n = 1, shortest = 0, gamma 0.5 with reward (1, 10, -1), the zero table with reward (0, 0, 0) -- every key
               ties, the order is b alone --, the huge table, and the hashed "3x3" and "2x4" tables at 256 nodes;
    carved     the first 32 configurations of carved_L10_M40.npz, each at a budget of its own sol_len, max_nodes = 4,000, hashed
               "feat+spare";
    long_*     the games of 254 moves at max_nodes = 300, the linear "feat+spare" table: at shortest = 0 the descent follows the first
               child of every node to the deepest records, and the spare row is read at its clamp, bin 255.

main() also prints, for the three cases the CPU test compares with exact_mirror.npz, how many configurations both searches prove; the
test's floors are 48 of 64, 41 of 64 and 16 of 32.  If a hashed table falls under one, change HASH_SALT, not the floor.
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
import make_golden_exact as G  # noqa: E402  -- the inputs

NAMES = G.NAMES
BUDGET, FEAT = "feat+spare", "feat"
HASH_SALT = 0x7E7215
LINEAR = (8, 1, 0, 2, 3, 6, 3, 2, 1)                           # holes .. hole depth: the classical weights' magnitudes, times ten
CARVED_NODES = G.CARVED_NODES
LONG = ((105, False), (105, True))                             # L, shortest
INVARIANT = (("cfg_L3_M8_c4000", 48), ("cfg_L4_M6_c4000_owed", 41), ("cfg_L5_M12_c4000", 16))    # key in exact_mirror.npz, floor
_tables = {}


def table(form, kind):
    """The int32 table of `form` and `kind` (the module's docstring has the hash)."""
    if (form, kind) not in _tables:
        entries = T._learn_lib.ntuple_entries_of(form)
        if kind == "zero":
            out = np.zeros(entries, np.int32)
        elif kind == "linear":
            per = {FEAT: 9, BUDGET: 10}[form]                  # rows of 256 bins a piece
            j = np.arange(entries, dtype=np.int64)
            row, q = (j // 256) % per, j % 256
            weight = np.array(LINEAR + (0,), np.int64)[np.minimum(row, 9)]
            out = np.where(j < 8 * per * 256, -weight * q * (1 << 12), 0).astype(np.int32)
        else:
            with np.errstate(over="ignore"):
                h = np.arange(entries, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(HASH_SALT)
                h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
                h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
                h = h ^ (h >> np.uint64(31))
            if kind == "hashed":
                out = ((h % np.uint64((1 << 19) + 1)).astype(np.int64) - (1 << 18)).astype(np.int32)
            elif kind == "huge":
                mag = (1 << 30) - ((h >> np.uint64(20)) % np.uint64(1 << 12)).astype(np.int64)
                out = np.where((h >> np.uint64(63)) == 1, -mag, mag).astype(np.int32)
            else:
                raise ValueError(kind)
        out.setflags(write=False)
        _tables[(form, kind)] = out
    return _tables[(form, kind)]


def cases():
    """[(key, arguments)]: every case but the carved one.  The arguments are ntuple_exact's by name, with rows and pieces made when asked
    for (G.inputs reads source, L and M) and the table named by (form, kind)."""
    out = []
    plain = dict(gamma=1.0, reward=(1.0, 0.0, 0.0), shortest=True, form=BUDGET, kind="hashed")
    for L, M, game_L, count in G.SMALL:
        for shortest in (True, False):
            for kind in ("zero", "hashed"):
                out.append((f"small_L{L}_M{M}_g{game_L}_s{int(shortest)}_{kind}",
                            dict(plain, source=("generate", game_L, M, count, 31 + M), L=L, M=M, max_nodes=G.SMALL_NODES, shortest=shortest,
                                 kind=kind)))
    (L3, M3, n3), (L5, M5, n5) = G.CONFIGS
    first = dict(plain, source=("generate", L3, M3, n3, G.CONFIG_SEED), L=L3, M=M3)
    second = dict(plain, source=("generate", L5, M5, n5, G.CONFIG_SEED), L=L5, M=M5)
    for form in (BUDGET, FEAT):
        tag = "budget" if form == BUDGET else "feat"
        for cap in G.CAPS:
            out.append((f"cfg_L{L3}_M{M3}_c{cap}_{tag}", dict(first, max_nodes=cap, form=form)))
        for cap in G.CAPS[1:]:
            out.append((f"cfg_L{L5}_M{M5}_c{cap}_{tag}", dict(second, max_nodes=cap, form=form)))
        out.append((f"cfg_L{L3 + 1}_M{M3 - 2}_c4000_owed_{tag}", dict(first, L=L3 + 1, M=M3 - 2, max_nodes=4000, form=form)))
    base = dict(first, max_nodes=256)
    out.append((f"cfg_L{L3}_M{M3}_c256_one", dict(base, source=("generate", L3, M3, 1, G.CONFIG_SEED))))
    out.append((f"cfg_L{L3}_M{M3}_c256_first", dict(base, shortest=False)))
    out.append((f"cfg_L{L3}_M{M3}_c256_gamma", dict(base, gamma=0.5, reward=(1.0, 10.0, -1.0))))
    out.append((f"cfg_L{L3}_M{M3}_c256_ties", dict(base, kind="zero", reward=(0.0, 0.0, 0.0))))
    out.append((f"cfg_L{L3}_M{M3}_c256_huge", dict(base, kind="huge")))
    out.append((f"cfg_L{L3}_M{M3}_c256_3x3", dict(base, form="3x3")))
    out.append((f"cfg_L{L3}_M{M3}_c256_2x4", dict(base, form="2x4")))
    for L, shortest in LONG:
        out.append((f"long_L{L}_s{int(shortest)}", dict(plain, source=("long",), L=L, M=G.LONG_M, shortest=shortest, max_nodes=G.LONG_NODES, kind="linear")))
    return out


def slice_of(key, n):
    """The configurations of a case that tests/test_ntuple_exact_cpu.py recomputes: all of a small game, of a low cap and of the long
    games; six of a case that may run to 4,000 nodes, of the one at shortest = 0, where most run to the cap, and of a window form, whose mirror
    walks some 150 tuples a board."""
    if "c4000" in key or key.endswith(("_3x3", "_2x4", "_first")):
        return np.array([0, 1, 2, n // 2, n - 2, n - 1])
    return np.arange(n)


def run_case(m, args, pick=None):
    rows, pieces = G.inputs(args)
    if pick is not None:
        rows, pieces = rows[pick], pieces[pick]
    got = m.ntuple_exact(rows, pieces, args["L"], args["M"], table(args["form"], args["kind"]), args["max_nodes"],
                         shortest=args["shortest"], gamma=args["gamma"], reward=args["reward"])
    return dict(zip(NAMES, got))


def carved_case(m, pick=None):
    """The carved case, grouped by budget as G.carved_case groups it; pick: the configurations (of the 32) to search, the others 0 / 255."""
    rows, pieces, sol_len, L, M = G.carved_inputs()
    parts = []
    for budget, idx in G.carved_groups(sol_len):
        if pick is not None:
            idx = np.intersect1d(idx, pick)
        if idx.size:
            got = m.ntuple_exact(rows[idx], pieces[idx, :budget + 1], L, budget, table(BUDGET, "hashed"), CARVED_NODES)
            parts.append((idx, budget, got))
    return G.carved_gather(parts, G.CARVED_COUNT, M)


CARVED_SLICE = np.array([0, 2, 31])                            # two budgets, one search that runs to the cap


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
    print(f"carved: proved {int(got['proved'].sum())}, solved {int(got['solved'].sum())} of {G.CARVED_COUNT}, nodes {got['nodes'].tolist()}, "
          f"{time.time() - t0:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "ntuple_exact_mirror.npz"), **out)
    twin = np.load(os.path.join(HERE, "exact_mirror.npz"))
    for key, floor in INVARIANT:
        for tag in ("budget", "feat"):
            both = int(((twin[f"{key}_proved"] == 1) & (out[f"{key}_{tag}_proved"] == 1)).sum())
            print(f"{key} {tag}: both proved {both}, floor {floor}", "" if both >= floor else "-- UNDER THE FLOOR: change HASH_SALT")


if __name__ == "__main__":
    main()
