"""Stage-indexed n-tuple tables without a GPU (include/tpl_learn.h's "Staged tables"; the _staged entries of csrc/learn/ntuple.hip and
ntuple_beam.hip; _learn_lib.py's numpy mirror; ntuple.py):

  1. the constants, the layout and the three entry counts; ntuple_stage_map against a loop written out by hand;
  2. the numpy mirror: with eight distinct random blocks V is the plain mirror's V on block map[k] & 7, under maps with bits set above
     bit 2; the update and the trace update are the plain mirror's on the block of every state's stage, and leave the map alone;
  3. the header declares the five entries with their twins' arguments, `form` for `shape`, and the library exports them;
  4. no new kernel uses scratch, by the build's resource notes;
  5. every C refusal is a status, in the twin's order with the form first;
  6. the Python surface and its refusals: coherent=True with a map, a start of another shape, ntuple_parts of a staged table.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_heuristic_cpu import _Env
from test_ntuple_sum_cpu import _ages, _args, _boards, _errors, _full_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, M = 10, 40
FORMS = {"2x4": 314368, "3x3": 590848, "2x4+3x3": 905216}
STAGED = {"2x4": 2515968, "3x3": 4727808, "2x4+3x3": 7242752}
FORM_IDS = {"2x4": 0, "3x3": 1, "2x4+3x3": 2}


def _m():
    return T._learn_lib


def _wild_map(seed):
    """A map of random 32-bit words: every bit above bit 2 is noise that the mask drops."""
    return np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, 1024).astype(np.int32)


def _staged_table(seed, form, stage_map, span=None):
    """A staged table of eight distinct random blocks with `stage_map` behind them."""
    entries = FORMS[form]
    gen = np.random.default_rng(seed)
    body = gen.integers(-(1 << 31), 1 << 31, 8 * entries) if span is None else gen.integers(-span, span + 1, 8 * entries)
    return np.concatenate([body.astype(np.int32), np.asarray(stage_map, np.int32)])


# ------------------------------------------------------------------------------------------------ 1. constants, layout, the map
def test_the_constants_the_layout_and_the_entry_counts():
    m = _m()
    assert m.NTUPLE_STAGES == 8 and T.NTUPLE_STAGES == 8 and m.NTUPLE_FORM_IDS == FORM_IDS
    for form, entries in FORMS.items():
        assert m.ntuple_staged_entries_of(form) == STAGED[form] == 8 * entries + 1024
        assert m.ntuple_form_of(STAGED[form]) == (form, True) and m.ntuple_form_of(entries) == (form, False)
        assert (4 * entries) % 16 == 0 and entries % 512 == 0           # every block 16-byte aligned, and a whole number of pattern rows
        table = T.ntuple_table("cpu", form, staged=True)
        assert tuple(table.shape) == (STAGED[form],) and table.dtype == torch.int32 and int(table.abs().sum()) == 0
        assert T.ntuple_is_staged(table) and not T.ntuple_is_staged(T.ntuple_table("cpu", form)) and T.ntuple_shape(table) == form
        stages, stage_map = T.ntuple_stages(table), T.ntuple_map(table)
        assert len(stages) == 8 and [s.data_ptr() - table.data_ptr() for s in stages] == [4 * g * entries for g in range(8)]
        assert all(tuple(s.shape) == (entries,) and s.is_contiguous() and T.ntuple_shape(s) == form and not T.ntuple_is_staged(s) for s in stages)
        assert tuple(stage_map.shape) == (1024,) and stage_map.data_ptr() - table.data_ptr() == 32 * entries
        stages[3][7] = 5                                       # views: written through to the whole
        stage_map[9] = 6
        assert int(table[3 * entries + 7]) == 5 and int(table[8 * entries + 9]) == 6
        assert T.ntuple_is_symmetric(T.ntuple_table("cpu", form, staged=True))
    assert 4 * STAGED["2x4+3x3"] == 28971008 < 1 << 31         # byte offsets fit 32 bits
    # no plain table and no coherence buffer has one of the staged counts, and the old constants stay
    assert not set(STAGED.values()) & set(FORMS.values()) and set(m._ntuple_counts()) == set(FORMS.values())
    assert m.NTUPLE_SUMS == {"2x4+3x3": ("2x4", "3x3")} and set(m.NTUPLE_SHAPES) == {"2x4", "3x3"} and m.NTUPLE_ENTRIES_SUM == 905216
    with pytest.raises(ValueError):
        m.ntuple_form_of(STAGED["2x4"] + 1)
    for name in ("NTUPLE_STAGES", "ntuple_stage_map", "ntuple_staged", "ntuple_stages", "ntuple_map", "ntuple_is_staged"):
        assert name in T.__all__ and getattr(T, name) is getattr(T.ntuple, name)


@pytest.mark.parametrize("game", [(2, 2), (10, 40), (250, 254)])
def test_the_stage_map_is_the_loop_written_out_by_hand(game):
    game_l, game_m = game
    for lines, moves in ((1, 1), (1, 2), (1, 4), (1, 8), (2, 4), (2, 2), (2, 3), (4, 2), (8, 1)):
        want = np.zeros(1024, np.int32)
        for l in range(16):
            for m in range(64):
                bl = min(l * lines // (min(game_l, 15) + 1), lines - 1)
                bm = min(m * moves // (min(game_m, 63) + 1), moves - 1)
                want[64 * l + m] = bl * moves + bm
        got = _m().ntuple_stage_map(game_l, game_m, lines, moves)
        assert got.dtype == np.int32 and np.array_equal(got, want) and got.max() == lines * moves - 1 and got.min() == 0
        torch_map = T.ntuple_stage_map(game_l, game_m, lines=lines, moves=moves)
        assert torch_map.dtype == torch.int32 and np.array_equal(torch_map.numpy(), want)
        # every state the game can be in -- lines left 0 .. L, moves left 0 .. M -- lands in the bucket of its clamped counters
        k = _m().ntuple_counter_index(game_l, game_m, np.arange(game_l + 1)[:, None], np.arange(game_m + 1)[None, :])
        assert set(np.unique(want[k]).tolist()) <= set(range(lines * moves))
        if game == (10, 40) and (lines, moves) == (2, 4):
            assert len(set(want[k].reshape(-1).tolist())) == 8 and want[k][0, 0] == 7 and want[k][10, 40] == 0
    assert np.array_equal(_m().ntuple_stage_map(game_l, game_m), _m().ntuple_stage_map(game_l, game_m, 1, 4))
    for lines, moves in ((3, 3), (2, 5), (1, 9), (9, 1), (0, 4), (1, 0), (-1, -4), (1.0, 4), (True, 4), (None, 2)):
        with pytest.raises(ValueError):
            _m().ntuple_stage_map(game_l, game_m, lines, moves)
        with pytest.raises(ValueError):
            T.ntuple_stage_map(game_l, game_m, lines, moves)


# ------------------------------------------------------------------------------------------------ 2. the mirror
@pytest.mark.parametrize("form", list(FORMS))
def test_the_mirror_value_is_the_plain_value_of_the_block_the_masked_map_names(form):
    m, b, entries = _m(), _boards(31, 400), FORMS[form]
    wild = _wild_map(32)
    assert ((wild.astype(np.int64) & ~7) != 0).sum() > 1000   # bits above bit 2 are set
    table = _staged_table(33, form, wild)
    stage = m.ntuple_stages_of(table, L, M, b["lines"], b["moves"])
    k = 64 * np.clip(L - b["lines"], 0, 15) + np.clip(M - b["moves"], 0, 63)
    assert np.array_equal(stage, wild[k].astype(np.int64) & 7) and len(set(stage.tolist())) == 8
    got = m.ntuple_value(table, *_args(b), b["state"])
    want = np.zeros(400, np.float32)
    for g in range(8):
        block = np.ascontiguousarray(table[g * entries:(g + 1) * entries])
        want[stage == g] = m.ntuple_value(block, *_args(b), b["state"])[stage == g]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    run = b["state"] == 0
    assert (got.view(np.uint32)[~run] == 0).all() and (got[run] != 0).all()
    # another map, another value; the masked map alone decides
    other = table.copy()
    other[-1024:] = wild & 7
    assert np.array_equal(m.ntuple_value(other, *_args(b), b["state"]).view(np.uint32), got.view(np.uint32))
    other[-1024:] = (wild + 1) & 7
    assert not np.array_equal(m.ntuple_value(other, *_args(b), b["state"]).view(np.uint32), got.view(np.uint32))
    for bad in (np.zeros(STAGED[form] + 1, np.int32), np.zeros(STAGED[form], np.int64)):
        with pytest.raises(ValueError, match="table"):
            m.ntuple_value(bad, *_args(b), b["state"])


@pytest.mark.parametrize("form", list(FORMS))
def test_the_mirror_updates_add_in_the_block_of_every_states_stage_and_leave_the_map(form):
    m, k, horizon, entries = _m(), 96, 3, FORMS[form]
    wild = _wild_map(41)
    start = _staged_table(42, form, wild)
    b, error = _boards(43, k), _errors(44, k)
    got = m.ntuple_update(start.copy(), *_args(b), b["state"], error, 3000.0)
    stage = m.ntuple_stages_of(start, L, M, b["lines"], b["moves"])
    want = start.copy()
    for g in range(8):                                         # the states of stage g update block g as a plain table
        at = stage == g
        want[g * entries:(g + 1) * entries] = m.ntuple_update(start[g * entries:(g + 1) * entries].copy(), b["rows"][at], b["piece"][at],
                                                              L, M, b["lines"][at], b["moves"][at], b["state"][at], error[at], 3000.0)
    assert np.array_equal(got, want) and np.array_equal(got[-1024:], wild) and (got != start).any()
    # the trace update: the ages of a board may fall in different stages; symmetric or not
    ages = _ages(45, k, horizon)
    for symmetric in (False, True):
        got = m.ntuple_update_trace(start.copy(), ages, L, M, error, 3000.0, 0.7, symmetric)
        want = start.copy()
        for g in range(8):                                     # block g as a plain table: age by age, the plain update of the states
            block = start[g * entries:(g + 1) * entries].copy()  # of stage g whose trace is open, at the age's decayed rate
            open_ = np.ones(k, bool)
            w = np.float32(1.0)
            for age, (rows, piece, lines, moves, state) in enumerate(ages):
                if age:
                    w = np.float32(w * np.float32(0.7))
                open_ &= state == 0                            # a state of another stage that does not run still cuts the trace
                at = open_ & (m.ntuple_stages_of(start, L, M, lines, moves) == g)
                one = [(rows[at], piece[at], lines[at], moves[at], state[at])]
                m.ntuple_update_trace(block, one, L, M, error[at], np.float32(3000.0) * w, 0.0, symmetric)
            want[g * entries:(g + 1) * entries] = block
        assert np.array_equal(got, want), symmetric
        assert np.array_equal(got[-1024:], wild) and (got != start).any()
    # from zero blocks a symmetric update leaves every block symmetric, the other one does not
    zero = np.concatenate([np.zeros(8 * entries, np.int32), wild])
    sigma = m.ntuple_mirror_permutation(form)
    for symmetric in (False, True):
        left = m.ntuple_update_trace(zero.copy(), ages, L, M, error, 3000.0, 0.7, symmetric)
        blocks = [left[g * entries:(g + 1) * entries] for g in range(8)]
        assert sum(bool(x.any()) for x in blocks) >= 4
        assert all(np.array_equal(x[sigma], x) for x in blocks) == symmetric
        assert T.ntuple_is_symmetric(torch.from_numpy(left)) == symmetric
    with pytest.raises(ValueError, match="coherent|table"):
        m.ntuple_update_coherent(zero.copy(), np.zeros((entries, 2), np.int64), ages, L, M, error, 3000.0, 0.7, False)


# ------------------------------------------------------------------------------------------------ 3. header and library
STAGED_ENTRIES = {"tpl_ntuple_value_staged": "tpl_ntuple_value_shaped", "tpl_ntuple_act_staged": "tpl_ntuple_act_shaped",
                  "tpl_ntuple_search_staged": "tpl_ntuple_search_shaped", "tpl_ntuple_beam_staged": "tpl_ntuple_beam",
                  "tpl_ntuple_update_trace_staged": "tpl_ntuple_update_trace_shaped"}


def test_the_header_declares_the_staged_entries_and_the_library_exports_them():
    raw = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_m().LEARN_SYMBOLS) and set(STAGED_ENTRIES) <= declared
    names = lambda entry: [a.split()[-1].lstrip("*") for a in re.search(rf"int {entry}\((.*?)\);", text, flags=re.S).group(1).split(",")]
    for entry, twin in STAGED_ENTRIES.items():
        assert names(entry) == ["form" if a == "shape" else a for a in names(twin)] and "form" in names(entry), entry
    assert re.search(r"#define\s+TPL_NTUPLE_STAGES\s+8\b", text)
    assert re.search(r"TPL_NTUPLE_FORM_2X4 = 0, TPL_NTUPLE_FORM_3X3 = 1, TPL_NTUPLE_FORM_SUM = 2", text)
    for name in ("TPL_NTUPLE_ENTRIES_STAGED", "TPL_NTUPLE_ENTRIES_STAGED_3X3", "TPL_NTUPLE_ENTRIES_STAGED_SUM"):
        assert re.search(rf"#define\s+{name}\s", text), name
    for count in ("2,515,968", "4,727,808", "7,242,752", "map[k(s)] & 7"):
        assert count in raw, count
    lib = ctypes.CDLL(_m().build_library())
    for entry in STAGED_ENTRIES:
        assert hasattr(lib, entry), entry


# ------------------------------------------------------------------------------------------------ 4. the kernels' resources
NEW_KERNELS = ([f"ntuple_staged{shape}_{what}_kernel" for shape in ("", "3", "_sum") for what in ("value", "act", "search")]
               + ["ntuple_staged_beam_kernel", "ntuple_staged_beam3_kernel", "ntuple_staged_beam_sum_kernel"])


def test_no_staged_kernel_uses_scratch():
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _m().build_library()], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    field = lambda r, name: int(r[r.index(name) - 1])
    for kernel in NEW_KERNELS:
        mine = [r for r in rows if kernel in r[-1]]
        assert len(mine) == 1, kernel
        print(" ".join(mine[0]))
        assert field(mine[0], "scratch") == 0 and field(mine[0], "vgpr") <= 128
    for kernel in ("ntuple_staged_trace_kernel", "ntuple_staged3_trace_kernel"):     # symmetric or not
        mine = [r for r in rows if kernel in r[-1]]
        assert len(mine) == 2 and all(field(r, "scratch") == 0 and field(r, "lds") == 4096 for r in mine), kernel
    staged = [r for r in rows if "ntuple_staged" in r[-1]]
    assert len(staged) == 16 and all(field(r, "scratch") == 0 for r in rows if "ntuple" in r[-1])
    assert all(field(r, "lds") == 24904 for r in staged if "beam" in r[-1])          # the frame of the plain beam


# ------------------------------------------------------------------------------------------------ 5. C refusals
def test_every_refusal_of_the_staged_entries_is_a_status_in_the_twins_order_with_the_form_first():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    nan, inf = float("nan"), float("inf")

    def value(a=fake, b=fake, n=4, L=2, M=2, table=fake, value=fake, form=0):
        return lib.tpl_ntuple_value_staged(a, b, n, L, M, table, value, form, None)

    def act(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
            value=fake, form=1):
        return lib.tpl_ntuple_act_staged(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, score, after_a, after_b,
                                         value, form, None)

    def search(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, after_a=fake, after_b=fake, score=fake,
               value=fake, form=2):
        return lib.tpl_ntuple_search_staged(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, fake + 1, score, after_a,
                                            after_b, value, form, None)

    def beam(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, depth=3, width=8, action=fake, after_a=fake, after_b=fake,
             score=fake, form=2):
        return lib.tpl_ntuple_beam_staged(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, depth, width, action, fake + 1, score, after_a,
                                          after_b, form, None)

    def update(a=fake, b=fake, n=4, slots=3, head=1, horizon=2, L=2, M=2, table=fake, error=fake, rate=1.0, decay=0.5, form=2):
        return lib.tpl_ntuple_update_trace_staged(a, b, n, slots, head, horizon, L, M, table, error, rate, decay, 1, form, None)

    entries = ((value, b"tpl_ntuple_value_staged:"), (act, b"tpl_ntuple_act_staged:"), (search, b"tpl_ntuple_search_staged:"),
               (beam, b"tpl_ntuple_beam_staged:"), (update, b"tpl_ntuple_update_trace_staged:"))
    limit = -(-(1 << 31) // 40)
    for entry, name in entries:
        for form in (3, -1, 8, 1 << 20):                       # the form first, before any pointer is looked at
            assert entry(form=form) < 0 and b"form must be" in err() and name in err(), form
            assert entry(a=None, n=0, L=0, table=None, form=form) < 0 and b"form must be" in err()
        assert entry(a=None) < 0 and b"null" in err() and name in err()
        assert entry(b=None) < 0 and b"null" in err() and name in err()
        for n in (0, -1):
            assert entry(n=n) < 0 and b"positive" in err() and name in err(), n
        for n in (limit, 1 << 40):
            assert entry(n=n) < 0 and b"2^31" in err() and name in err(), n
        for plane in ("a", "b"):
            assert entry(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err()
        for L_, M_ in ((0, 2), (2, 256), (251, 2), (2, 255), (2, 0)):
            assert entry(L=L_, M=M_) < 0 and b"L and M" in err() and name in err(), (L_, M_)
        assert entry(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
        for off in (4, 8, 12):
            assert entry(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
        for form in (0, 1, 2):                                 # every known form gets past the form check, to the next refusal
            assert entry(table=None, form=form) < 0 and b"table" in err()
        # the order: planes before n before L and M before the table
        assert entry(a=None, n=0, L=0, table=None) < 0 and b"null" in err() and b"table" not in err()
        assert entry(n=0, L=0, table=None) < 0 and b"positive" in err()
        assert entry(L=0, table=None) < 0 and b"L and M" in err()
    assert value(value=None) < 0 and b"null" in err() and b"value" in err()
    assert value(value=fake + 2) < 0 and b"value must be 4-byte aligned" in err()
    assert value(table=None, value=None) < 0 and b"table" in err()
    for entry, name in entries[1:4]:
        assert entry(action=None) < 0 and b"null" in err() and b"action" in err() and name in err()
        assert entry(after_a=None) < 0 and b"go together" in err() and name in err()
        assert entry(after_b=fake + 4) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
        assert entry(score=fake + 2) < 0 and b"4-byte aligned" in err()
        for gamma in (nan, inf, -inf):
            assert entry(gamma=gamma) < 0 and b"gamma must be finite" in err() and name in err(), gamma
        assert entry(table=None, action=None) < 0 and b"table" in err()
        assert entry(action=None, after_a=None) < 0 and b"action" in err()
        assert entry(after_a=None, after_b=fake + 4) < 0 and b"go together" in err()
        assert entry(after_b=fake + 4, score=fake + 2) < 0 and b"16-byte aligned" in err()
        assert entry(score=fake + 2, gamma=nan) < 0 and b"4-byte aligned" in err()
    for entry in (act, search):
        assert entry(value=fake + 2) < 0 and b"score and value must be 4-byte aligned" in err()
        for epsilon in (-0.001, 1.001, nan, inf):
            assert entry(epsilon=epsilon) < 0 and b"epsilon must be in [0, 1]" in err(), epsilon
        assert entry(epsilon=2.0, gamma=nan) < 0 and b"epsilon" in err()
    for depth in (0, -1, 12):
        assert beam(depth=depth) < 0 and b"depth must be in [1, 11]" in err(), depth
    for width in (0, -1, 65):
        assert beam(width=width) < 0 and b"width must be in [1, 64]" in err(), width
    assert beam(gamma=nan, depth=0) < 0 and b"gamma" in err()
    # the update: tpl_ntuple_update_trace_shaped's order -- table, error, rate, then the ring
    assert update(error=None) < 0 and b"null" in err() and b"error" in err()
    assert update(error=fake + 2) < 0 and b"error must be 4-byte aligned" in err()
    for rate in (nan, inf, -inf):
        assert update(rate=rate) < 0 and b"rate must be finite" in err(), rate
    for slots in (0, -1, 18):
        assert update(slots=slots, head=0, horizon=1) < 0 and b"slots must be in [1, 17]" in err(), slots
    for head in (-1, 3):
        assert update(head=head) < 0 and b"head must be in [0, slots)" in err(), head
    for horizon in (0, 4, 17):
        assert update(horizon=horizon) < 0 and b"horizon must be in" in err(), horizon
    assert update(n=limit // 3 + 1) < 0 and b"40 * slots * n" in err()
    for decay in (-0.1, 1.1, nan):
        assert update(decay=decay) < 0 and b"decay must be in [0, 1]" in err(), decay
    assert update(table=None, error=None) < 0 and b"table" in err()
    assert update(error=None, rate=nan) < 0 and b"error" in err()
    assert update(rate=nan, slots=0) < 0 and b"rate" in err()
    assert update(slots=0, decay=2.0) < 0 and b"slots" in err()
    # the twins keep refusing the sum as a shape
    assert lib.tpl_ntuple_value_shaped(fake, fake, 4, 2, 2, fake, fake, 2, None) < 0 and b"shape" in err()


# ------------------------------------------------------------------------------------------------ 6. Python
def test_the_python_surface_and_its_refusals():
    N, m = T.ntuple, _m()
    env = _Env(8)
    plain = {form: torch.from_numpy(_full_range(50 + i, entries)) for i, (form, entries) in enumerate(FORMS.items())}
    wild = torch.from_numpy(_wild_map(60))
    for form, table in plain.items():
        staged = N.ntuple_staged(table, wild)
        assert tuple(staged.shape) == (STAGED[form],) and N.ntuple_is_staged(staged) and N.ntuple_shape(staged) == form
        assert all(torch.equal(block, table) for block in N.ntuple_stages(staged)) and torch.equal(N.ntuple_map(staged), wild)
        assert staged.data_ptr() != table.data_ptr()
        with pytest.raises(ValueError, match="ntuple_stages"):
            N.ntuple_parts(staged)                             # a staged table has stages, each of which has parts
        assert [tuple(p.shape) for p in N.ntuple_parts(N.ntuple_stages(staged)[5])] == [tuple(p.shape) for p in N.ntuple_parts(table)]
        with pytest.raises(ValueError, match="plain"):
            N.ntuple_staged(staged, wild)
        for bad in (wild[:-1], wild.to(torch.int64), wild.numpy(), None, torch.zeros((1024, 1), dtype=torch.int32)):
            with pytest.raises(ValueError, match="stage_map"):
                N.ntuple_staged(table, bad)
        # policies take it by its entry count
        for depth in (1, 2):
            p = N.NTuplePolicy(env, staged, depth=depth)
            assert p.staged is True and p.shape == form and N.NTuplePolicy(env, table, depth=depth).staged is False
        beam = N.NTupleBeamPolicy(env, staged, 3, 8)
        assert beam.staged is True and beam.shape == form and N.NTupleBeamPolicy(env, table, 3, 8).staged is False
        # symmetry: every block
        sigma = torch.from_numpy(m.ntuple_mirror_permutation(form))
        sym = N.ntuple_staged((table // 2) + (table // 2)[sigma], wild)
        assert N.ntuple_is_symmetric(sym) and not N.ntuple_is_symmetric(staged)
        at = 6 * FORMS[form] + (512 + 3 if form == "3x3" else 256 + 3)
        sym[at] += 1                                           # one entry of block 6 that is not its own image
        assert not N.ntuple_is_symmetric(sym)
    for bad in (torch.zeros(STAGED["2x4"] + 16, dtype=torch.int32), torch.zeros(STAGED["2x4"], dtype=torch.int64), None,
                N.ntuple_table("cpu", "3x3")):
        for call in (N.ntuple_stages, N.ntuple_map):
            with pytest.raises(ValueError, match="staged"):
                call(bad)
    with pytest.raises(ValueError, match="table"):
        N.ntuple_is_staged(torch.zeros(STAGED["2x4"] + 16, dtype=torch.int32))
    for staged in (1, None, "yes"):
        with pytest.raises(ValueError, match="staged"):
            N.ntuple_table("cpu", "2x4", staged=staged)
    # the learner
    four = N.ntuple_stage_map(env.L, env.M, moves=4)
    for form in FORMS:
        learner = N.NTupleLearner(env, shape=form, stage_map=four, start=plain[form], lam=0.8, horizon=4, symmetric=True)
        assert N.ntuple_is_staged(learner.table) and learner.shape == form and learner.policy.staged and learner.greedy.staged
        assert torch.equal(N.ntuple_map(learner.table), four) and all(torch.equal(b, plain[form]) for b in N.ntuple_stages(learner.table))
        assert learner.coherence is None and learner.policy.table is learner.table
        zero = N.NTupleLearner(env, shape=form, stage_map=four)
        assert int(zero.table[:-1024].abs().sum()) == 0 and torch.equal(N.ntuple_map(zero.table), four)
        begun = N.NTupleLearner(env, shape=form, start=plain[form])     # a start without a map: a plain table that begins as a copy
        assert not N.ntuple_is_staged(begun.table) and torch.equal(begun.table, plain[form]) and begun.table.data_ptr() != plain[form].data_ptr()
        with pytest.raises(ValueError, match="coheren"):
            N.NTupleLearner(env, shape=form, stage_map=four, coherent=True)
        for other in FORMS:
            if other != form:
                with pytest.raises(ValueError, match="start"):
                    N.NTupleLearner(env, shape=form, stage_map=four, start=plain[other])
        for bad in (N.ntuple_staged(plain[form], four), plain[form].to(torch.int64), plain[form].numpy(), 5):
            with pytest.raises(ValueError, match="start"):
                N.NTupleLearner(env, shape=form, stage_map=four, start=bad)
        for bad in (four[:-1], four.to(torch.int64), four.numpy(), 4):
            with pytest.raises(ValueError, match="stage_map"):
                N.NTupleLearner(env, shape=form, stage_map=bad)
    # the defaults leave the learner as it was
    default = N.NTupleLearner(env)
    assert not N.ntuple_is_staged(default.table) and tuple(default.table.shape) == (314368,) and not default.policy.staged
