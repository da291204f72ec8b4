"""A learned evaluation of the board a placement leaves: an n-tuple network on afterstates, trained by temporal-difference
learning on the device (the rule: include/tpl_learn.h; the kernels: csrc/learn/ntuple.hip).

    ntuple_table(device, shape="2x4")
                                  a zeroed table: int32 [314,368], in units of 2^-16; shape="3x3": int32 [590,848]
                                  shape="2x4+3x3": a SUM TABLE, int32 [905,216] -- a 2x4 table, then a 3x3 table, read together
    ntuple_shape(table)           "2x4", "3x3", "2x4+3x3", "feat", "3x3+feat" or "feat+spare", from the table's entry count
    ntuple_parts(table)           the per-shape views of a table or a coherence buffer (one for a plain table, two for a sum):
                                  they share its storage, and each is a valid table of its shape
    ntuple_value(source, table)   V of every resident board of an environment, or of plane pairs
    NTuplePolicy(env, table, gamma, epsilon, seed, depth=1).act()
                                  arg-max over the distinct placements of  r + gamma * V(afterstate)  in ONE launch; with epsilon a
                                  board explores uniformly over its DISTINCT placements (not over the 40 actions, 6 to 31 of which
                                  are aliases); act(score=, after=, value=) also gives the greedy score (the TD target), the
                                  afterstate of the action played and its value.  depth=2 searches the known next piece as well,
                                  still in one launch:  r + gamma * max_b (r_b + gamma * V)  -- the value of the afterstate itself,
                                  with the table one move further out; act(second=) gives the placement planned for that piece
    NTupleBeamPolicy(env, table, depth, width, gamma=0.99).act()
                                  a beam search over the pieces the window knows (up to 11 plies, up to 64 nodes a ply) with the
                                  table at the leaves, in ONE launch: greedy, no exploration; act(score=, plan=, after=) also gives
                                  the best leaf's folded value, its path and the one-ply afterstate of the action.  depth 1 is
                                  NTuplePolicy's greedy choice, depth 2 with width >= 34 its depth=2
    NTupleLearner(env, gamma, rate, epsilon, seed, depth=1, lam=0.0, horizon=1, symmetric=False, coherent=False, shape="2x4")
                                  TD(0) on afterstates: train(steps), evaluate(steps, depth=None, width=None); `table` is a plain tensor
                                  (torch.save it); a table trained at one depth can be played at the other.  horizon > 1 adds
                                  truncated TD(lambda) traces -- the error also goes, decayed by (gamma lam)^k, to the afterstates
                                  k < horizon moves back in the same episode --, symmetric=True adds every update to the entries of
                                  the reflected board as well, which keeps the table mirror-symmetric
                                  coherent=True gives every entry a step size of its own (temporal coherence): the ratio of the
                                  signed to the absolute sum of the steps it was sent, kept in `coherence`
    ntuple_is_symmetric(table)    whether table[sigma] == table under the mirror permutation of the entries
    ntuple_coherence(device, shape="2x4")
                                  a zeroed coherence buffer: int64 [entries of the shape, 2], the pairs (E, A)
    ntuple_step_sizes(coherence)  alpha of every entry: float32 [entries]
    ntuple_table(device, shape, staged=True)
                                  a zeroed STAGED TABLE: NTUPLE_STAGES = 8 whole tables of the form and a stage map, one int32 buffer
    ntuple_stage_map(L, M, lines=1, moves=4)
                                  int32 [1,024]: a grid of lines x moves <= 8 buckets over (lines left, moves left)
    ntuple_staged(table, stage_map)
                                  weight promotion: a staged table whose eight blocks are each a copy of a plain table, with the map
    ntuple_stages(table), ntuple_map(table), ntuple_is_staged(table)
                                  the eight per-stage views (each a valid plain table of the form), the map view, the test
    ntuple_table(device, "feat"), ntuple_table(device, "3x3+feat")
                                  a zeroed FEATURE TABLE, int32 [19,456], and a 3x3 table with a feature table behind it, int32 [610,304]
    ntuple_feature_bins(source)   uint8 [K, 9]: the nine bins a feature table is read at
    ntuple_table(device, "feat+spare")
                                  a zeroed BUDGET TABLE, int32 [21,504]: a feature table with a tenth row, read at the spare cells
    ntuple_budget(feat_table)     a budget table whose nine feature rows and counters are a "feat" table's and whose row 9 is zero
    ntuple_budget_bins(source)    uint8 [K, 10]: the ten bins a budget table is read at
    NTuplePolicy(..., bound=True), NTupleBeamPolicy(..., bound=True), NTupleLearner(..., shape="feat+spare", bound=True)
                                  the dead-board prune, for a budget table only
    NTupleRanker(table, L, M, gamma, reward, rate, margin, bound, symmetric)
                                  a supervised ranking update from proved move labels (T.label_moves): rank(planes, label) names the
                                  best-scored proved win, the best-scored proved loss and the greedy move of every state in ONE
                                  launch; step() then adds rint(rate) on the win's afterstate and subtracts it on the loss's through
                                  the update kernels above; fit(labelset, epochs, batch, seed).  One of the four plain forms, taught in
                                  place; label 3 proves nothing and teaches nothing

The value is a sum of table entries, one per 2 x 4 window of the board that is not empty, chosen by the falling piece, plus one
per (lines left, moves left); the update adds rint(rate * error) to the same entries.  Everything is integer, so two trainings
with one seed give the same bytes.  The window is the table's SHAPE: "2x4", two adjacent columns by four rows, or "3x3", three by
three -- a column with both of its neighbours.  Policy, value, the symmetry test and the step sizes take the shape from the table
(or buffer) they are given; a table of one shape cannot be played as the other.

Two shapes summed ("2x4+3x3", the standard form of an n-tuple network): V = float32(S_2x4 + S_3x3) * 2^-16, the two parts' exact
integer sums added before the one rounding.  The value, both policies and the beam read a sum table in one launch each (the _sum
entries of include/tpl_learn.h); the update kernels never read the table, so the learner sends its errors through the existing
update once per part.  Everything that takes a table takes a sum table, by its entry count.

Staged tables.  In a plain table the move budget enters the value additively: V = f(board, piece) + counter[lines left, moves left].
A staged table holds eight whole tables of one form ("2x4", "3x3" or "2x4+3x3") and a map from the counter index to one of them: the
stage of a state is map[k] & 7, and V is the form's value read from that block -- so the same stack can be worth one thing with
three moves left and another with thirty.  The stage is looked up wherever a table is read, ply by ply: a leaf of the two-ply search
or of the beam is valued in the block of its own lines and moves left.  Value, both policies, the beam, the symmetry test and the
learner (traces and symmetry; NOT temporal coherence) take a staged table by its entry count; a map that uses two or four stages
leaves the other blocks untouched.  ntuple_staged(trained_table, map) starts every stage from a trained plain table.

Feature tuples ("feat", "3x3+feat": NTUPLE_FEATURE_FORMS).  Every window is local; what carries HeuristicPolicy's hand-made score is
global: holes, aggregate height, bumpiness, transitions, wells.  A feature table holds, per falling piece, a row of 256 entries for each
of the nine board features, looked up at min(feature, 255) -- the piecewise-constant generalisation of that linear score, learned by the
same TD rule -- and the counters; "3x3+feat" sums it with a 3x3 table as "2x4+3x3" sums two shapes, one rounding.  The features do not
change under reflection, so the mirror image moves only the piece.  Value, both policies, the beam, the symmetry test and the learner
with traces and symmetry take either form by name or by entry count.  There is no staged and no coherent form, and both are refused:
each would be eight more kernels, and neither option raised a win rate in the record.

The budget table ("feat+spare": NTUPLE_BUDGET_FORMS).  A feature table sees the move budget only through one additive counter entry,
clamped at 15 lines and 63 moves.  A budget table adds a tenth row per falling piece, read at sbin = 0 for a dead board and else
min(spare + 1, 255), spare = 4 (M - moves) - cells being the move bound's (T.move_bound): what a board can still waste, from its own
lines and moves.  The row is learned by the same TD rule where HeuristicPolicy's spare_weight is set by hand.  ntuple_budget(table)
copies a trained "feat" table into one with row 9 zero, which plays as the source does, byte for byte.  bound=True on the policies is the
dead-board prune: a move that leaves a running board the bound proves lost is scored as a loss at the limit -- no gamma * V, nothing
searched below it --, while `after` and `value` stay the true afterstate's.  Only a budget table takes it; like "feat" it has no staged,
coherent or summed form.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _learn_lib
from ._learn_lib import (BEAM_MAX_WIDTH, NTUPLE_BEAM_MAX_DEPTH, NTUPLE_BUDGET_FORMS, NTUPLE_BUDGET_ROWS, NTUPLE_COUNTERS, NTUPLE_ENTRIES,
                         NTUPLE_ENTRIES_SUM, NTUPLE_FEATURE_FORMS,
                         NTUPLE_FEATURES, NTUPLE_FORM_IDS, NTUPLE_SHAPE_IDS, NTUPLE_SHAPES, NTUPLE_STAGES, NTUPLE_SUMS, NTUPLE_TRACE_MAX, check)
from .lookahead import _MAX_BOARDS, _boards, _ptr, _state_ptrs

__all__ = ["NTUPLE_ENTRIES", "NTUPLE_ENTRIES_SUM", "NTUPLE_SHAPES", "NTUPLE_SUMS", "ntuple_shape", "ntuple_parts", "ntuple_table", "ntuple_value", "ntuple_is_symmetric", "ntuple_coherence", "ntuple_step_sizes",
           "NTuplePolicy", "NTupleBeamPolicy", "NTupleLearner", "NTUPLE_FEATURE_FORMS", "ntuple_feature_bins", "NTUPLE_BUDGET_FORMS",
           "ntuple_budget", "ntuple_budget_bins", "NTUPLE_STAGES", "ntuple_stage_map", "ntuple_staged", "ntuple_stages",
           "ntuple_map", "ntuple_is_staged", "NTupleRanker"]

_STATE_WON = 1                                                 # bits 28..29 of B.y: 0 running, 1 won, 2 and 3 lost
_FINISHED_B_Y = _STATE_WON << 28                               # B.y of a state that is finished and otherwise empty


def _counts() -> dict:
    """Entry count -> name, for every shape and every sum of shapes."""
    return _learn_lib._ntuple_counts()


def _table_counts() -> dict:
    """Entry count -> name, for every plain table: the shapes, their sums, the feature forms and the budget table."""
    return {**_learn_lib._ntuple_counts(), **_learn_lib._ntuple_feature_counts(), **_learn_lib._ntuple_budget_counts()}


_NO_FEATURE_FORM = ("a feature table ({shape!r}) has no {what}: each would be eight more kernels, and neither staging nor temporal "
                    "coherence raised a win rate in the record (include/tpl_learn.h, \"Feature tuples\")")


_NO_BUDGET_FORM = ("a budget table ({shape!r}) has no {what}: like a feature table it has one plain form "
                   "(include/tpl_learn.h, \"The budget table\")")
_BOUND_NEEDS_BUDGET = ('bound=True is the dead-board prune of a budget table: the table must be of the form "feat+spare" '
                       "(ntuple_table(device, \"feat+spare\"), ntuple_budget), not {shape!r}")


def _entries(shape, windows_only: str = "") -> int:
    """The entries of a table of `shape`; windows_only: what a feature form or the budget table is refused for, where it is."""
    names = sorted(NTUPLE_SHAPES) + sorted(NTUPLE_SUMS) + sorted(NTUPLE_FEATURE_FORMS) + sorted(NTUPLE_BUDGET_FORMS)
    if not isinstance(shape, str) or shape not in names:
        raise ValueError(f"shape must be one of {names}, got {shape!r}")
    if windows_only and shape in NTUPLE_FEATURE_FORMS:
        raise ValueError(_NO_FEATURE_FORM.format(shape=shape, what=windows_only))
    if windows_only and shape in NTUPLE_BUDGET_FORMS:
        raise ValueError(_NO_BUDGET_FORM.format(shape=shape, what=windows_only))
    return _learn_lib.ntuple_entries_of(shape)


def _staged_counts() -> dict:
    """Entry count -> the form's name, for the staged table of every shape and every sum."""
    return _learn_lib._ntuple_staged_counts()


def ntuple_table(device="cuda:0", shape: str = "2x4", staged: bool = False) -> torch.Tensor:
    """A zeroed n-tuple table of `shape` on `device`: int32 [NTUPLE_SHAPES[shape] entries] (2x4: NTUPLE_ENTRIES); "2x4+3x3": a sum
    table, int32 [NTUPLE_ENTRIES_SUM] -- ntuple_parts gives its two tables.  "feat": a feature table, int32 [19,456]; "3x3+feat":
    int32 [610,304], a 3x3 table and a feature table (ntuple_parts); neither has a staged form.  staged=True: a staged table of that form, int32
    [NTUPLE_STAGES * entries + 1,024] -- ntuple_stages gives its eight tables, ntuple_map its map; the all-zero map sends every
    state to stage 0."""
    if not isinstance(staged, bool):
        raise ValueError(f"staged must be True or False, got {staged!r}")
    entries = _entries(shape, "staged form" if staged else "")
    return torch.zeros(NTUPLE_STAGES * entries + NTUPLE_COUNTERS if staged else entries, dtype=torch.int32, device=device)


def ntuple_is_staged(table) -> bool:
    """Whether `table` is a staged table, by its entry count (a tensor of no known count is refused, as ntuple_shape refuses it)."""
    ntuple_shape(table)
    return table.shape[0] in _staged_counts()


def _staged(table) -> torch.Tensor:
    if not (isinstance(table, torch.Tensor) and table.dim() == 1 and table.dtype == torch.int32 and table.shape[0] in _staged_counts()):
        sizes = ", ".join(f"{k} ({v})" for k, v in _staged_counts().items())
        raise ValueError(f"table must be a staged table: an int32 tensor of {sizes} entries (ntuple_table(staged=True), ntuple_staged)")
    return table


def ntuple_stages(table) -> tuple:
    """The NTUPLE_STAGES per-stage views of a staged table, stage 0 first.  Views, not copies: each is a valid, 16-byte aligned plain
    table of the form for everything that takes one, and what is written through it is written to the whole."""
    entries = _entries(_staged_counts()[_staged(table).shape[0]])
    return tuple(table[g * entries:(g + 1) * entries] for g in range(NTUPLE_STAGES))


def ntuple_map(table) -> torch.Tensor:
    """The stage map of a staged table: the view of its last 1,024 entries, one per counter index k; the stage of k is map[k] & 7."""
    return _staged(table)[-NTUPLE_COUNTERS:]


def ntuple_stage_map(L: int, M: int, lines: int = 1, moves: int = 4) -> torch.Tensor:
    """int32 [1,024] on the host: a stage map that cuts (lines left, moves left) of an L / M game into lines x moves <= 8 buckets of
    equal width -- entry 64 l + m holds bl * moves + bm, bm = m * moves // (min(M, 63) + 1) and bl = l * lines // (min(L, 15) + 1) on
    the counters as the counter index clamps them.  Any other map is one the user writes: 1,024 integers, of which bits 0..2 count."""
    return torch.from_numpy(_learn_lib.ntuple_stage_map(L, M, lines, moves))


def _stage_map(stage_map, device) -> torch.Tensor:
    if (not isinstance(stage_map, torch.Tensor) or stage_map.dtype != torch.int32 or tuple(stage_map.shape) != (NTUPLE_COUNTERS,)):
        raise ValueError(f"stage_map must be an int32 tensor of {NTUPLE_COUNTERS} entries (ntuple_stage_map)")
    return stage_map.to(device)


@torch.no_grad()
def ntuple_staged(table: torch.Tensor, stage_map: torch.Tensor) -> torch.Tensor:
    """Weight promotion: a new staged table on `table`'s device whose eight blocks are each a copy of the PLAIN table `table` (of any
    form), with `stage_map` (int32 [1,024]) as its map.  It values, and plays, exactly as `table` does, whatever the map holds, until
    it is trained."""
    if not isinstance(table, torch.Tensor) or ntuple_is_staged(table):
        raise ValueError("ntuple_staged promotes a plain table (ntuple_stages gives the plain tables of a staged one)")
    _table(table, table.device)
    _entries(ntuple_shape(table), "staged form")
    out = ntuple_table(table.device, ntuple_shape(table), staged=True)
    for block in ntuple_stages(out):
        block.copy_(table)
    ntuple_map(out).copy_(_stage_map(stage_map, table.device))
    return out


def ntuple_coherence(device="cuda:0", shape: str = "2x4") -> torch.Tensor:
    """A zeroed coherence buffer of `shape` on `device`: int64 [entries, 2], entry j the pair (E_j, A_j) of include/tpl_learn.h;
    of a sum, laid out as the sum table is."""
    return torch.zeros((_entries(shape, "coherence buffer"), 2), dtype=torch.int64, device=device)


def ntuple_shape(table) -> str:
    """"2x4", "3x3" or "2x4+3x3": the shape of a table (or, by its first dimension, of a coherence buffer), from its entry count;
    "feat", "3x3+feat" or "feat+spare" for a table of a feature form or a budget table; a tensor of any other size is refused."""
    if isinstance(table, torch.Tensor) and table.dim() >= 1 and table.shape[0] in _counts():
        return _counts()[table.shape[0]]
    if isinstance(table, torch.Tensor) and table.dim() == 1 and table.shape[0] in _table_counts():
        return _table_counts()[table.shape[0]]                 # a feature form, "feat" or "3x3+feat", or the budget table
    if isinstance(table, torch.Tensor) and table.dim() == 1 and table.shape[0] in _staged_counts():
        return _staged_counts()[table.shape[0]]                # a staged table: the form of its blocks
    sizes = ", ".join(f"{k} ({v})" for k, v in _table_counts().items())
    raise ValueError(f"table must be a tensor of {sizes} entries (ntuple_table)")


def ntuple_parts(table) -> tuple:
    """The per-shape views of a table or a coherence buffer, in the order they lie in it: (table,) for a plain one, (the 2x4 part,
    the 3x3 part) for a sum.  Views, not copies: each is a valid, 16-byte aligned table (buffer) of its shape for everything that
    takes one, and what is written through it is written to the whole.  A staged table is refused: ntuple_stages gives its eight
    tables, each of which has parts."""
    if isinstance(table, torch.Tensor) and table.dim() == 1 and table.shape[0] in _staged_counts():
        raise ValueError("a staged table has no parts of its own: ntuple_stages(table) gives its eight tables, ntuple_parts of one its parts")
    parts, at = [], 0
    for part in _learn_lib.ntuple_parts_of(ntuple_shape(table)):
        parts.append(table[at:at + _learn_lib._PART_ENTRIES[part]])
        at += _learn_lib._PART_ENTRIES[part]
    return tuple(parts)


@torch.no_grad()
def ntuple_step_sizes(coherence: torch.Tensor) -> torch.Tensor:
    """float32 [the buffer's entries] on the buffer's device: alpha of every entry as tpl_ntuple_update_coherent would read it now -- 1
    where A <= 0, else min(|E| / A, 1) in float32.  torch has no unsigned 64-bit conversion, so the one magnitude a signed
    conversion gets wrong, |INT64_MIN| = 2^63, is put in by a select; the quotient of the two float32 values is taken in float64
    and rounded to float32, which is the float32 quotient rounded once (53 >= 2 * 24 + 2 bits) whatever division torch's float32
    kernels were built with.  No host sync."""
    _coherence(coherence)
    e, a = coherence[:, 0], coherence[:, 1]
    lowest = e == torch.iinfo(torch.int64).min
    mag = torch.where(lowest, 2.0 ** 63, e.masked_fill(lowest, 0).abs().to(torch.float32))
    ratio = torch.clamp((mag.to(torch.float64) / a.to(torch.float32).to(torch.float64)).to(torch.float32), max=1.0)
    return torch.where(a <= 0, 1.0, ratio).to(torch.float32)


def _sizes() -> str:
    return " or ".join(f"{k} ({v})" for k, v in _table_counts().items())


def _coherence(coherence, table=None) -> torch.Tensor:
    """A coherence buffer of a shape's entry count -- of `table`'s, where one is given."""
    counts = list(_counts()) if table is None else [int(table.shape[0])]
    if (not isinstance(coherence, torch.Tensor) or coherence.dtype != torch.int64 or coherence.dim() != 2
            or coherence.shape[1] != 2 or coherence.shape[0] not in counts or not coherence.is_contiguous()
            or (table is not None and coherence.device != table.device)):
        want = _sizes() if table is None else f"{counts[0]}, the table's"
        raise ValueError(f"coherence must be a contiguous int64 tensor of shape (entries, 2), entries = {want} (ntuple_coherence)")
    return coherence


def _table(table, device) -> torch.Tensor:
    if (not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 1
            or (table.shape[0] not in _table_counts() and table.shape[0] not in _staged_counts()) or table.device != device
            or not table.is_contiguous()):
        raise ValueError(f"table must be a contiguous int32 tensor of {_sizes()} entries, or a staged table, on {device} (ntuple_table)")
    return table


def _bound(bound, shape: str, staged: bool = False) -> bool:
    """The prune flag of a policy on a table of `shape`: a bool, and True for a budget table alone."""
    if not isinstance(bound, bool):
        raise ValueError(f"bound must be True or False, got {bound!r}")
    if bound and (staged or shape not in NTUPLE_BUDGET_FORMS):
        raise ValueError(_BOUND_NEEDS_BUDGET.format(shape=("staged " if staged else "") + shape))
    return bound


def _shaped(lib, entry: str, shape: str, staged: bool = False, prune=None):
    """How the library reads a table of `shape` through `entry` ("tpl_ntuple_value", ...): (function, trailing arguments before
    `stream`) -- the _shaped twin with the C shape id, or for a sum of shapes the _sum twin, which takes none; for a staged table of
    any form the _staged twin with the C form id.  A budget table: the _budget twin, which takes no form, and for a policy
    (prune given) the prune flag where the others take their id."""
    if shape in NTUPLE_BUDGET_FORMS and not staged:
        return getattr(lib, entry + "_budget"), (() if prune is None else (int(prune),))
    if staged:
        return getattr(lib, entry + "_staged"), (NTUPLE_FORM_IDS[shape],)
    if shape in NTUPLE_FEATURE_FORMS:
        return getattr(lib, entry + "_feature"), (NTUPLE_FEATURE_FORMS[shape],)
    if shape in NTUPLE_SUMS:
        return getattr(lib, entry + "_sum"), ()
    return getattr(lib, entry + "_shaped"), (NTUPLE_SHAPE_IDS[shape],)


def _unit(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) <= 1.0:
        raise ValueError(f"{name} must be a number in [0, 1], got {v!r}")
    return float(v)


def _finite(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def _count(name: str, v, least: int = 0) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError(f"{name} must be an integer of at least {least}, got {v!r}")
    return int(v)


def _depth(depth) -> int:
    if isinstance(depth, bool) or depth not in (1, 2):
        raise ValueError(f"depth must be 1 or 2 (an afterstate knows its next piece and no more), got {depth!r}")
    return int(depth)


def _beam_shape(depth, width):
    """(depth, width) of an n-tuple beam: integers in 1 .. NTUPLE_BEAM_MAX_DEPTH and 1 .. BEAM_MAX_WIDTH."""
    if isinstance(depth, bool) or not isinstance(depth, int) or not 1 <= depth <= NTUPLE_BEAM_MAX_DEPTH:
        raise ValueError(f"depth must be an integer in 1 .. {NTUPLE_BEAM_MAX_DEPTH} (the leaf's piece must be a known one), got {depth!r}")
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= BEAM_MAX_WIDTH:
        raise ValueError(f"width must be an integer in 1 .. {BEAM_MAX_WIDTH}, got {width!r}")
    return int(depth), int(width)


def _horizon(horizon) -> int:
    if isinstance(horizon, bool) or not isinstance(horizon, int) or not 1 <= horizon <= NTUPLE_TRACE_MAX:
        raise ValueError(f"horizon must be an integer in 1 .. {NTUPLE_TRACE_MAX}, got {horizon!r}")
    return int(horizon)


def _planes(pair, device, what: str):
    """A pair of int32 [K, 4] planes on `device` (None: wherever the first one is), checked: (K, a, b)."""
    if not isinstance(pair, (tuple, list)) or len(pair) != 2 or not isinstance(pair[0], torch.Tensor):
        raise ValueError(f"{what} must be a pair of int32 [K, 4] tensors")
    a, b = pair
    device = a.device if device is None else device
    for t in (a, b):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 4 or t.device != device
                or not t.is_contiguous() or t.shape != a.shape):
            raise ValueError(f"{what} must be a pair of contiguous int32 [K, 4] tensors of equal shape on {device}")
    return int(a.shape[0]), a, b


def _value(planes_a, planes_b, k: int, L: int, M: int, table, out, device) -> None:
    stream = torch._C._cuda_getCurrentRawStream(device.index)
    entry, shape = _shaped(_learn_lib.lib(), "tpl_ntuple_value", ntuple_shape(table), ntuple_is_staged(table))
    check(entry(_ptr(planes_a), _ptr(planes_b), k, L, M, table.data_ptr(), out.data_ptr(), *shape, stream))


@torch.no_grad()
def ntuple_value(source, table: torch.Tensor, L: Optional[int] = None, M: Optional[int] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [K]: V of K states under `table`; 0 for a state that is not running.  `source` is an environment (its resident
    boards, read in place, under its L and M) or a pair (states_a, states_b) of int32 [K, 4] planes on the table's device, for
    which the game's L and M must be given.  No host sync, and no allocation when `out` is given."""
    if hasattr(source, "num_envs"):
        if L is not None or M is not None:
            raise ValueError("an environment brings its own L and M")
        k, device, L, M = _boards(source, "ntuple_value"), source.device, source.L, source.M
        _table(table, device)
        a, b = _state_ptrs(source)
    else:
        k, a, b = _planes(source, None, "source")
        device = a.device
        _table(table, device)
        if L is None or M is None:
            raise ValueError("planes need the game's L and M")
        if not 1 <= k <= _MAX_BOARDS:
            raise ValueError(f"ntuple_value takes 1 .. {_MAX_BOARDS} states")
    if out is None:
        out = torch.empty(k, dtype=torch.float32, device=device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (k,) or out.device != device
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 tensor of shape ({k},) on {device}")
    _value(a, b, k, int(L), int(M), table, out, device)
    return out


@torch.no_grad()
def ntuple_feature_bins(source, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [K, 9]: the nine bins a feature table is read at -- min(phi, 255) of holes, aggregate_height, max_height, bumpiness,
    row_transitions, column_transitions, wells, rows_with_holes and hole_depth -- of K states, running or not
    (tpl_ntuple_feature_bins).  `source` is an environment (its resident boards) or a pair (states_a, states_b) of int32 [K, 4]
    planes on one GPU.  No host sync, and no allocation when `out` is given."""
    if hasattr(source, "num_envs"):
        k, device = _boards(source, "ntuple_feature_bins"), source.device
        a, b = _state_ptrs(source)
    else:
        k, a, b = _planes(source, None, "source")
        device = a.device
        if not 1 <= k <= _MAX_BOARDS:
            raise ValueError(f"ntuple_feature_bins takes 1 .. {_MAX_BOARDS} states")
    if out is None:
        out = torch.empty((k, NTUPLE_FEATURES), dtype=torch.uint8, device=device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (k, NTUPLE_FEATURES) or out.device != device
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape ({k}, {NTUPLE_FEATURES}) on {device}")
    stream = torch._C._cuda_getCurrentRawStream(device.index)
    check(_learn_lib.lib().tpl_ntuple_feature_bins(_ptr(a), _ptr(b), k, out.data_ptr(), stream))
    return out


@torch.no_grad()
def ntuple_budget_bins(source, L: Optional[int] = None, M: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [K, 10]: the ten bins a budget table is read at -- ntuple_feature_bins' nine, then sbin = 0 for a dead board and else
    min(spare + 1, 255) of the move bound -- of K states, running or not (tpl_ntuple_budget_bins; a finished board has spare 0: bin 1).
    `source` is an environment (its resident boards, under its L and M) or a pair (states_a, states_b) of int32 [K, 4] planes on one
    GPU, for which the game's L and M must be given.  No host sync, and no allocation when `out` is given."""
    if hasattr(source, "num_envs"):
        if L is not None or M is not None:
            raise ValueError("an environment brings its own L and M")
        k, device, L, M = _boards(source, "ntuple_budget_bins"), source.device, source.L, source.M
        a, b = _state_ptrs(source)
    else:
        k, a, b = _planes(source, None, "source")
        device = a.device
        if L is None or M is None:
            raise ValueError("planes need the game's L and M")
        if not 1 <= k <= _MAX_BOARDS:
            raise ValueError(f"ntuple_budget_bins takes 1 .. {_MAX_BOARDS} states")
    if out is None:
        out = torch.empty((k, NTUPLE_BUDGET_ROWS), dtype=torch.uint8, device=device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (k, NTUPLE_BUDGET_ROWS) or out.device != device
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape ({k}, {NTUPLE_BUDGET_ROWS}) on {device}")
    stream = torch._C._cuda_getCurrentRawStream(device.index)
    check(_learn_lib.lib().tpl_ntuple_budget_bins(_ptr(a), _ptr(b), k, int(L), int(M), out.data_ptr(), stream))
    return out


@torch.no_grad()
def ntuple_budget(table: torch.Tensor) -> torch.Tensor:
    """Weight promotion: a new budget table ("feat+spare") on `table`'s device whose nine feature rows and counters are those of the
    "feat" table `table` and whose row 9 is zero.  Without the prune it values, and plays, exactly as `table` does until it is trained."""
    if not isinstance(table, torch.Tensor) or table.dim() != 1 or table.dtype != torch.int32 or ntuple_shape(table) != "feat":
        raise ValueError('ntuple_budget promotes a "feat" table: an int32 tensor of 19,456 entries (ntuple_table(device, "feat"))')
    out = ntuple_table(table.device, "feat+spare")
    bins = _learn_lib.NTUPLE_FEATURE_BINS
    rows = out[:-NTUPLE_COUNTERS].view(_learn_lib.NTUPLE_PIECES, NTUPLE_BUDGET_ROWS, bins)
    rows[:, :NTUPLE_FEATURES].copy_(table[:-NTUPLE_COUNTERS].view(_learn_lib.NTUPLE_PIECES, NTUPLE_FEATURES, bins))
    out[-NTUPLE_COUNTERS:].copy_(table[-NTUPLE_COUNTERS:])
    return out


_sigma = {}                                                    # the mirror permutation, once per device and shape


@torch.no_grad()
def ntuple_is_symmetric(table: torch.Tensor) -> bool:
    """Whether `table` is mirror-symmetric: table[sigma(j)] == table[j] for every j, sigma = _learn_lib.ntuple_mirror_permutation()
    (include/tpl_learn.h states the invariant; of a sum table: of every part).  Under such a table a board and its reflection have
    the same value, bit for bit.  A staged table: whether every one of its eight blocks is.
    One gather and one comparison on the table's device; the answer is a host bool, so this syncs."""
    if not isinstance(table, torch.Tensor):
        raise ValueError(f"table must be a contiguous int32 tensor of {_sizes()} entries (ntuple_table)")
    _table(table, table.device)
    key = (table.device, ntuple_shape(table))
    if key not in _sigma:
        _sigma[key] = torch.from_numpy(_learn_lib.ntuple_mirror_permutation(key[1])).to(table.device)
    blocks = ntuple_stages(table) if ntuple_is_staged(table) else (table,)
    return all(bool(torch.equal(block[_sigma[key]], block)) for block in blocks)


class NTuplePolicy:
    """The greedy / epsilon-greedy placement policy of an n-tuple table on the resident boards of `env`: act() scores every
    distinct placement a as  r_a  if it ends the game, else  r_a + gamma * V(afterstate)  (env.reward_params; float32, never
    fused) and plays the lowest a at the maximum; a finished board gets action 0.  With epsilon > 0 a running board explores
    with that probability, uniformly over its distinct placements, on the hash of (seed, step, board) -- deterministic.
    One launch that leaves the environment as it is.  `table` is read at every act(): train it in place.

    depth=2 (tpl_ntuple_search) looks at the known next piece too: where a placement leaves the game running, V(afterstate)
    gives way to the best  r_b + gamma * V  (r_b alone where b ends the game) over the distinct placements b of the next piece
    on that afterstate.  The draw, and what `after` and `value` mean, do not change with the depth.

    bound=True (a "feat+spare" table only; anything else is refused): the dead-board prune.  A placement, at either ply, that leaves
    a running board the move bound proves lost is scored as one that ends lost at the limit: its reward with r_lose, no gamma * V,
    nothing searched below it.  Only scores and the arg-max change: `after` and `value` are still the true afterstate and its table
    value, and exploration stays uniform over the distinct placements."""

    def __init__(self, env, table: torch.Tensor, gamma: float = 0.99, epsilon: float = 0.0, seed: int = 0, depth: int = 1,
                 bound: bool = False):
        _boards(env, "NTuplePolicy")
        self.env, self.table, self.depth = env, _table(table, env.device), _depth(depth)
        self.gamma, self.epsilon, self.seed = _finite("gamma", gamma), _unit("epsilon", epsilon), _count("seed", seed)
        self.shape = ntuple_shape(self.table)                  # "2x4", "3x3" or "2x4+3x3": the table's, which picks the kernels
        self.staged = ntuple_is_staged(self.table)             # with the shape: the _staged entries
        self.bound = _bound(bound, self.shape, self.staged)    # the dead-board prune: a budget table's alone
        self.step = 0                                          # the `step` of the next act() that is not given one
        self._planes = None

    @torch.no_grad()
    def act(self, out: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None, after=None,
            value: Optional[torch.Tensor] = None, step: Optional[int] = None, second: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [N]: the action of every resident board.  score (float32 [N], optional) receives the GREEDY maximum, whatever is
        played; after (a pair of int32 [N, 4] planes, optional) the afterstate of the action played -- the board itself where it
        is finished -- and value (float32 [N], optional) V of that afterstate.  step: the `step` of tpl_ntuple_act, which keys
        the exploration draw; None takes the policy's own counter and advances it.  second (uint8 [N], optional, depth 2 only):
        the placement planned for the next piece behind the action played, 255 where that action ends the game or the board is
        finished.  No host sync, and no allocation when `out` is given: capturable into a HIP graph (which replays the step it
        was captured with)."""
        env = self.env
        if second is not None:
            if self.depth != 2:
                raise ValueError("second is an output of depth 2 only")
            env._own(second, torch.uint8, "second")
        if out is None:
            out = torch.empty(env.num_envs, dtype=torch.uint8, device=env.device)
        env._own(out, torch.uint8, "out")
        if score is not None:
            env._own(score, torch.float32, "score")
        if value is not None:
            env._own(value, torch.float32, "value")
        after_a = after_b = None
        if after is not None:
            k, after_a, after_b = _planes(after, env.device, "after")
            if k != env.num_envs:
                raise ValueError(f"after must hold {env.num_envs} states")
        if step is None:
            step, self.step = self.step, self.step + 1
        else:
            step = _count("step", step)
        if self._planes is None:
            self._planes = _state_ptrs(env)                   # the resident planes live as long as the environment
        stream = torch._C._cuda_getCurrentRawStream(env.device.index)
        lib = _learn_lib.lib()
        head = (self._planes[0], self._planes[1], env.num_envs, env.L, env.M, *env.reward_params, self.gamma, self.table.data_ptr(),
                self.epsilon, self.seed % (1 << 64), step % (1 << 64), out.data_ptr())
        entry, shape = _shaped(lib, "tpl_ntuple_search" if self.depth == 2 else "tpl_ntuple_act", self.shape, self.staged, self.bound)
        tail = (_ptr(score), _ptr(after_a), _ptr(after_b), _ptr(value), *shape, stream)
        check(entry(*head, _ptr(second), *tail) if self.depth == 2 else entry(*head, *tail))
        return out


class NTupleBeamPolicy:
    """A beam search with an n-tuple table at the leaves on the resident boards of `env` (tpl_ntuple_beam; the rule is in
    include/tpl_learn.h).  At moves = m a state's window holds 12 - m mod 10 true pieces; act() searches min(depth, one less than
    that) plies -- the leaf is valued under the piece that falls next, which must be a known one.  Every ply expands each node of
    the beam by the distinct placements of its current piece, values a child as the rewards on its path folded over  gamma * V
    (env.reward_params; float32, never fused) and keeps the `width` best in candidate order; the action is the first placement of
    the best leaf.  Greedy: there is no exploration.  depth 1 is NTuplePolicy at epsilon 0; depth 2 with width >= 34 is
    NTuplePolicy(depth=2).  One launch that leaves the environment as it is; `table` is read at every act(), and its shape is the
    table's.  bound=True (a "feat+spare" table only): the dead-board prune at every ply -- a child that is left running and dead is a
    lost node, valued by its rewards alone and not expanded; `after` stays the true afterstate."""

    def __init__(self, env, table: torch.Tensor, depth: int, width: int, gamma: float = 0.99, bound: bool = False):
        _boards(env, "NTupleBeamPolicy")
        self.env, self.table = env, _table(table, env.device)
        self.depth, self.width = _beam_shape(depth, width)
        self.gamma = _finite("gamma", gamma)
        self.shape, self.staged = ntuple_shape(self.table), ntuple_is_staged(self.table)
        self.bound = _bound(bound, self.shape, self.staged)    # the dead-board prune: a budget table's alone
        self._planes = None

    @torch.no_grad()
    def act(self, out: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None,
            plan: Optional[torch.Tensor] = None, after=None) -> torch.Tensor:
        """uint8 [N]: the action of every resident board; `score` (float32 [N], optional) receives the chosen leaf's value and
        `plan` (uint8 [N, depth], optional) its path: plan[:, 0] is the action, 255 fills what was not searched (a finished
        board, a game that ends on the way, a window with fewer known pieces); `after` (a pair of int32 [N, 4] planes, optional)
        the ONE-PLY afterstate of the action -- the board itself where it is finished --, as NTuplePolicy.act gives it.  No host
        sync, and no allocation when `out` is given: capturable into a HIP graph."""
        env = self.env
        if out is None:
            out = torch.empty(env.num_envs, dtype=torch.uint8, device=env.device)
        env._own(out, torch.uint8, "out")
        if score is not None:
            env._own(score, torch.float32, "score")
        if plan is not None:
            env._own(plan, torch.uint8, "plan", (env.num_envs, self.depth))
        after_a = after_b = None
        if after is not None:
            k, after_a, after_b = _planes(after, env.device, "after")
            if k != env.num_envs:
                raise ValueError(f"after must hold {env.num_envs} states")
        if self._planes is None:
            self._planes = _state_ptrs(env)                   # the resident planes live as long as the environment
        stream = torch._C._cuda_getCurrentRawStream(env.device.index)
        lib = _learn_lib.lib()
        if self.staged:
            entry, shape = lib.tpl_ntuple_beam_staged, (NTUPLE_FORM_IDS[self.shape],)
        elif self.shape in NTUPLE_BUDGET_FORMS:
            entry, shape = lib.tpl_ntuple_beam_budget, (int(self.bound),)
        elif self.shape in NTUPLE_FEATURE_FORMS:
            entry, shape = lib.tpl_ntuple_beam_feature, (NTUPLE_FEATURE_FORMS[self.shape],)
        else:
            entry, shape = (lib.tpl_ntuple_beam_sum, ()) if self.shape in NTUPLE_SUMS else (lib.tpl_ntuple_beam, (NTUPLE_SHAPE_IDS[self.shape],))
        check(entry(self._planes[0], self._planes[1], env.num_envs, env.L, env.M, *env.reward_params, self.gamma,
                    self.table.data_ptr(), self.depth, self.width, out.data_ptr(), _ptr(plan), _ptr(score), _ptr(after_a),
                    _ptr(after_b), *shape, stream))
        return out


class NTupleLearner:
    """TD(0) on afterstates with an n-tuple table, entirely on the device.  `env`: an auto-reset environment with a
    configuration pool.  Each step of train() is one loop body -- no host sync, nothing allocated:

        1. act: the epsilon-greedy action, the greedy score and the afterstate of the action played (tpl_ntuple_act; at
           depth 2 tpl_ntuple_search, whose afterstate is the same one-ply afterstate and whose score is the two-ply one)
        2. error = greedy score - V(the afterstate kept from the step before), V as the table stands now (tpl_ntuple_value)
        3. the kept afterstates take  rint(rate * error)  on their table entries (tpl_ntuple_update)
        4. the environment steps
        5. the new afterstates are kept

    The greedy score of a state is the TD target of the afterstate that led to it: the state IS that afterstate, up to window
    entries the value does not read.  An afterstate that ended the game is not running, so it has value 0 and its update adds
    nothing: a board that auto-resets drops out by the rule, without a mask.  `rate` is in table units per unit of error: the
    step of V for one state alone is about rate * 2^-16 * (tuples in use + 1), and boards that share entries add up -- so it is
    small for many boards in lockstep.  At depth 2 `policy` and `greedy` search two plies, so the target of a kept afterstate
    is the two-ply greedy score of the state it became; nothing else in the loop changes.

    Traces and symmetry (tpl_ntuple_update_trace; both off by default, which leaves the table bytes of the loop above).  The
    afterstates of the last `horizon` steps stay in a ring of horizon + 1 slots, and step 3 adds  rint(rate * (gamma lam)^k *
    error)  to the afterstate k steps back, k < horizon, as long as it and every younger one run -- an episode's end cuts the
    trace by the same rule that drops a finished board.  Truncated TD(lambda): the effective step of V grows by about
    sum_k (gamma lam)^k, so `rate` wants to shrink with it.  Traces are NOT cut on exploratory moves (the naive form): the error
    of a step whose predecessor explored still reaches the older afterstates.  symmetric=True adds every update to the table
    entries of the reflected board too (L <-> J, S <-> Z): the table stays mirror-symmetric (ntuple_is_symmetric), each board
    teaches its reflection, and the step of V doubles once more.  Still five enqueues a step, no sync, nothing allocated.

    Temporal coherence (tpl_ntuple_update_coherent; coherent=False by default, which leaves the table bytes of the loop above).
    The learner owns `coherence` (ntuple_coherence), the signed and the absolute sum of the steps every entry was sent, and step 3
    scales an entry's step by alpha = |E| / A as it stood before the step (ntuple_step_sizes): an entry whose errors keep their
    sign learns at `rate`, one whose errors alternate -- an overshoot -- slows itself down.  A coherent step is never larger than
    the plain one.  forget() leaves `coherence` alone; it is a plain tensor, and coherence.zero_() starts the step sizes over.
    Still five enqueues a step (the entry launches two kernels), no sync, nothing allocated.

    shape ("2x4" by default, which leaves everything above as it was; "3x3"): the windows of the table, and of the coherence buffer
    if there is one.  Nothing else about the learner depends on it.

    shape="2x4+3x3": a sum table, and a coherence buffer laid out the same way.  Steps 1 and 2 read it through the _sum entries; step
    3 is the update above once per part with the same errors -- the 2x4 update on the first part, the 3x3 update on the second --,
    which is the update of the summed value because no update kernel reads the table: five enqueues plus one more update call, no
    sync, nothing allocated, and the same bytes in whatever order the adds arrive.  With symmetric=True each part is updated under
    its own sigma; with coherent=True each part's entries keep their own step sizes.  A state now adds to about 222 entries (both
    parts' non-empty windows and two counters) where it added to 107 to 115, so the step of V per unit of `rate` roughly DOUBLES,
    as it does under symmetry: `rate` wants to be about half of what a single shape takes.

    stage_map (None by default, which leaves everything above as it was; an int32 tensor of 1,024 entries: ntuple_stage_map): the
    learner owns a STAGED table of `shape` with that map.  Steps 1 and 2 read it through the _staged entries, a state in the block of
    its own lines and moves left; step 3 is tpl_ntuple_update_trace_staged, which adds in that block -- with traces and with symmetry
    as above, in one call for every form.  A stage sees only the states that fall in it, so each block learns from a share of the
    boards.  Temporal coherence has no staged form: coherent=True with a map is refused.
    start (None, or a plain table of `shape`): the table starts as a copy of it -- with a stage_map every stage does, which is
    weight promotion from a trained plain table.

    shape="feat" or "3x3+feat": a feature table, alone or behind a 3x3 table (the module's docstring).  Steps 1 and 2 read it through
    the _feature entries; step 3 is tpl_ntuple_update_trace_feature on the feature part and, for "3x3+feat", the 3x3 update on the
    first part with the same errors.  Traces, symmetry and start= work as above; stage_map= and coherent=True are refused.  One `rate`
    serves both parts of a sum.  A state adds to 10 entries of a feature table where it adds to about 107 of a 3x3 one, so the step of
    V per unit of `rate` is about a tenth: alone, `rate` is EXPECTED to want roughly ten times a window table's.  That is arithmetic
    on the step, not a measurement -- profiles/learner/README.md has what the sweep found.

    shape="feat+spare": a budget table (the module's docstring).  Steps 1 and 2 read it through the _budget entries, step 3 is
    tpl_ntuple_update_trace_budget: eleven adds a state.  Traces, symmetry and start= (a budget table: ntuple_budget promotes a "feat"
    one) work as above; stage_map= and coherent=True are refused.  bound=True (this form only) is the dead-board prune of the
    BEHAVIOUR policy and of the greedy target: the moves the learner plays and the scores it learns from skip what the move bound
    proves lost.  evaluate(bound=) plays the table with or without it, whatever it was trained with."""

    def __init__(self, env, gamma: float = 0.99, rate: float = 8.0, epsilon: float = 0.1, seed: int = 0, depth: int = 1,
                 lam: float = 0.0, horizon: int = 1, symmetric: bool = False, coherent: bool = False, shape: str = "2x4",
                 stage_map: Optional[torch.Tensor] = None, start: Optional[torch.Tensor] = None, bound: bool = False):
        n = _boards(env, "NTupleLearner")
        if not env.auto_reset:
            raise ValueError("NTupleLearner needs an auto-reset environment")
        self.env, self.rate = env, _finite("rate", rate)
        _entries(shape)
        if shape in NTUPLE_FEATURE_FORMS:
            if stage_map is not None:
                raise ValueError(_NO_FEATURE_FORM.format(shape=shape, what="staged form (stage_map=)"))
            if coherent is True:
                raise ValueError(_NO_FEATURE_FORM.format(shape=shape, what="coherent update (coherent=True)"))
        if shape in NTUPLE_BUDGET_FORMS:
            if stage_map is not None:
                raise ValueError(_NO_BUDGET_FORM.format(shape=shape, what="staged form (stage_map=)"))
            if coherent is True:
                raise ValueError(_NO_BUDGET_FORM.format(shape=shape, what="coherent update (coherent=True)"))
        self.shape, self.bound = shape, _bound(bound, shape, stage_map is not None)
        _unit("epsilon", epsilon), _finite("gamma", gamma), _count("seed", seed)
        self.lam, self.horizon = _unit("lam", lam), _horizon(horizon)
        if not isinstance(symmetric, bool):
            raise ValueError(f"symmetric must be True or False, got {symmetric!r}")
        if not isinstance(coherent, bool):
            raise ValueError(f"coherent must be True or False, got {coherent!r}")
        self.symmetric, self.coherent = symmetric, coherent
        self.decay = float(gamma) * self.lam                   # the C `decay`, passed as a float
        if not 0.0 <= self.decay <= 1.0:
            raise ValueError(f"gamma * lam must be in [0, 1] (it decays the trace), got {self.decay!r}")
        self.slots = self.horizon + 1
        if self.slots * n > _MAX_BOARDS:
            raise ValueError(f"(horizon + 1) * boards must stay at or below {_MAX_BOARDS}")
        d = env.device
        self.depth = _depth(depth)
        if stage_map is not None and coherent:
            raise ValueError("temporal coherence has no staged form (include/tpl_learn.h): coherent=True cannot go with a stage_map")
        if start is not None and (not isinstance(start, torch.Tensor) or start.dim() != 1 or start.dtype != torch.int32
                                  or start.shape[0] != _entries(shape)):
            raise ValueError(f"start must be a plain int32 table of the learner's shape, {shape} ({_entries(shape)} entries)")
        if stage_map is not None:
            _stage_map(stage_map, d)
        self.table = ntuple_table(d, shape, staged=stage_map is not None)
        for block in (ntuple_stages(self.table) if stage_map is not None else (self.table,)):
            if start is not None:
                block.copy_(start)
        if stage_map is not None:
            ntuple_map(self.table).copy_(_stage_map(stage_map, d))
        self.coherence = ntuple_coherence(d, shape) if coherent else None
        self.policy = NTuplePolicy(env, self.table, gamma, epsilon, seed, self.depth, bound=self.bound)
        self.greedy = NTuplePolicy(env, self.table, gamma, 0.0, seed, self.depth, bound=self.bound)
        self.steps = 0                                         # train() steps so far: the `step` of the exploration draw
        self._action = torch.empty(n, dtype=torch.uint8, device=d)
        self._done = torch.empty(n, dtype=torch.uint8, device=d)
        self._reward, self._score, self._kept_value, self._error = (torch.empty(n, dtype=torch.float32, device=d) for _ in range(4))
        # the afterstates of the last steps, slot-major: age k of the newest is slot (head - k) mod slots; act writes the next
        # ones into slot head + 1, the one slot no age of the update reads
        self._ring = tuple(torch.empty((self.slots, n, 4), dtype=torch.int32, device=d) for _ in range(2))
        self._slot = [(self._ring[0][k], self._ring[1][k]) for k in range(self.slots)]
        self._head = 0
        self.forget()

    @property
    def _kept(self):
        """The newest kept afterstates: slot `head` of the ring."""
        return self._slot[self._head]

    @property
    def _next(self):
        """Where act writes the afterstates of the step being made: slot head + 1."""
        return self._slot[(self._head + 1) % self.slots]

    def forget(self) -> None:
        """Nothing is kept from the steps before: every slot becomes finished states, which update nothing.  The table and the
        coherence buffer stay as they are."""
        for ring in self._ring:
            ring.zero_()
        self._ring[1][:, :, 1] = _FINISHED_B_Y

    @torch.no_grad()
    def train(self, steps: int, curriculum=None, refresh_every: int = 0) -> int:
        """`steps` steps of the loop above from the environment as it stands.  Whatever else moves the environment between two
        calls must be followed by forget(); evaluate() does it itself.  Returns the steps trained so far.
        curriculum (None by default, which leaves the loop and the table bytes as they are; a PoolCurriculum of this environment):
        its observe(action) is called before every step -- one more launch, which only reads the environment -- and, with
        refresh_every > 0, its refresh() whenever the steps trained so far reach a multiple of refresh_every."""
        steps = _count("steps", steps, 1)
        refresh_every = _count("refresh_every", refresh_every)
        if curriculum is not None and getattr(curriculum, "env", None) is not self.env:
            raise ValueError("curriculum belongs to another environment")
        if curriculum is None and refresh_every:
            raise ValueError("refresh_every needs a curriculum")
        env, n, lib = self.env, self.env.num_envs, _learn_lib.lib()
        stream = torch._C._cuda_getCurrentRawStream(env.device.index)
        ring_a, ring_b = self._ring[0].data_ptr(), self._ring[1].data_ptr()
        if self.coherent:
            _coherence(self.coherence, _table(self.table, env.device))   # a buffer of the other shape would be overrun
        # step 3 as a list of calls, each taking the ring's head: one per part of the table, each through the update entry of ITS kind --
        # a window part the _shaped entry (coherent or not) with the part's C shape id, a feature part tpl_ntuple_update_trace_feature,
        # which takes no shape; a staged table one call, whose entry launches the part updates itself
        staged = ntuple_is_staged(_table(self.table, env.device))
        if staged and self.coherent:
            raise ValueError("temporal coherence has no staged form (include/tpl_learn.h)")
        form_name = ntuple_shape(self.table)
        error, how = self._error.data_ptr(), (self.rate, self.decay, int(self.symmetric))

        def ring(table_ptr, head):
            return (ring_a, ring_b, n, self.slots, head, self.horizon, env.L, env.M, table_ptr)

        updates = []
        if staged:
            whole, form = self.table.data_ptr(), NTUPLE_FORM_IDS[form_name]
            updates.append(lambda head: lib.tpl_ntuple_update_trace_staged(*ring(whole, head), error, *how, form, stream))
        else:
            names = _learn_lib.ntuple_parts_of(form_name)
            if self.coherent and "feat" in names:
                raise ValueError(_NO_FEATURE_FORM.format(shape=form_name, what="coherent update"))
            buffers = ntuple_parts(self.coherence) if self.coherent else (None,) * len(names)
            for name, part, buffer in zip(names, ntuple_parts(self.table), buffers):
                t = part.data_ptr()
                if name in NTUPLE_BUDGET_FORMS:
                    if self.coherent:
                        raise ValueError(_NO_BUDGET_FORM.format(shape=form_name, what="coherent update"))
                    updates.append(lambda head, t=t: lib.tpl_ntuple_update_trace_budget(*ring(t, head), error, *how, stream))
                elif name == "feat":
                    updates.append(lambda head, t=t: lib.tpl_ntuple_update_trace_feature(*ring(t, head), error, *how, stream))
                elif self.coherent:
                    updates.append(lambda head, t=t, c=buffer.data_ptr(), s=NTUPLE_SHAPE_IDS[name]:
                                   lib.tpl_ntuple_update_coherent_shaped(*ring(t, head), c, error, *how, s, stream))
                else:
                    updates.append(lambda head, t=t, s=NTUPLE_SHAPE_IDS[name]:
                                   lib.tpl_ntuple_update_trace_shaped(*ring(t, head), error, *how, s, stream))
        for _ in range(steps):
            kept = self._kept
            self.policy.act(out=self._action, score=self._score, after=self._next, step=self.steps)
            _value(kept[0], kept[1], n, env.L, env.M, self.table, self._kept_value, env.device)
            torch.sub(self._score, self._kept_value, out=self._error)
            for update in updates:
                check(update(self._head))
            if curriculum is not None:
                curriculum.observe(self._action)
            env.step_into(self._action, self._reward, self._done)
            self._head = (self._head + 1) % self.slots
            self.steps += 1
            if refresh_every and self.steps % refresh_every == 0:
                curriculum.refresh()
        return self.steps

    @torch.no_grad()
    def evaluate(self, steps: int, depth: Optional[int] = None, width: Optional[int] = None, bound: Optional[bool] = None,
                 per_config: bool = False, proof: Optional[int] = None, proof_table=False, proof_discrepancy=None) -> dict:
        """Play `steps` greedy steps from a full reset and count: episodes (the steps' done flags), wins (the afterstates of the
        moves played whose state is "won": every reward parameter counts the same wins) and win_rate = wins / max(episodes, 1).
        depth: how deep the greedy policy searches -- None: the learner's own; 1 or 2 plays the table as it stands at that depth.
        width: None, or a beam width -- then NTupleBeamPolicy(depth, width) plays the table, `depth` must be given and may be
        1 .. 11.  bound: None -- the learner's own -- or whether the policy that plays prunes dead boards (a budget table only).
        The tallies stay on the device, with one sync at the end.  Training goes on from the boards this leaves, with
        nothing kept.  per_config=True: the dict gains episodes_by_config and wins_by_config, int32 device tensors over the loaded
        pool (a PoolTally observed before every step); the three other keys are what they are without it.
        proof: None, or a node budget -- then the policy plays inside a ProofPolicy(env, policy, max_nodes=proof) (solve.py): the
        first move of a plan that the exact search over the state's window proves winning, the table's move elsewhere; a plan's
        move wins exactly where it is the plan's last.  The dict gains proof, that policy's stats().  None leaves every result as
        it is.
        proof_table: False or None -- the proofs are ordered by the classical weights --, True -- by the learner's own table as it
        stands, with the learner's gamma and the environment's reward; refused where the table is not of one of the four plain forms
        "2x4", "3x3", "feat", "feat+spare" --, or a table of one of those forms, used as given with gamma 1 and reward (1, 0, 0)
        (solve.ntuple_window_prove).  It only orders the search, and needs `proof`.
        proof_discrepancy: None, or with `proof` "add" or "double" -- ProofPolicy's discrepancy: the proofs are searched in
        limited-discrepancy order from first_limit 0.  It changes which proofs fit the node budget, and nothing a proof promises."""
        if not isinstance(per_config, bool):
            raise ValueError("per_config must be True or False")
        ordered = proof_table is not None and proof_table is not False
        if proof is None and ordered:
            raise ValueError("proof_table orders the proofs: it needs proof, a node budget")
        order = {}
        if ordered and proof_table is True:
            from ._learn_lib import NTUPLE_EXACT_FORMS
            if self.greedy.staged or self.greedy.shape not in NTUPLE_EXACT_FORMS:
                raise ValueError(f"proof_table=True orders the proofs by the learner's table, which must be of one of the four plain "
                                 f"forms {', '.join(map(repr, NTUPLE_EXACT_FORMS))}; this learner's is "
                                 f"{'staged ' if self.greedy.staged else ''}{self.greedy.shape!r}")
            order = dict(table=self.table, gamma=self.greedy.gamma, reward=tuple(float(v) for v in self.env.reward_params))
        elif ordered:
            order = dict(table=proof_table)
        if proof is None and proof_discrepancy is not None:
            raise ValueError("proof_discrepancy orders the proofs: it needs proof, a node budget")
        if proof is not None:
            from .solve import ProofPolicy, _discrepancy, _max_nodes
            proof = _max_nodes(proof)
            _discrepancy(proof_discrepancy, 0)
            if proof_discrepancy is not None:                  # only then a LimitedProofPolicy
                order["discrepancy"] = proof_discrepancy
        steps = _count("steps", steps, 1)
        env, d = self.env, self.env.device
        greedy = self.greedy
        bound = greedy.bound if bound is None else _bound(bound, greedy.shape, greedy.staged)
        if width is not None:
            if depth is None:
                raise ValueError("evaluate(width=...) plays a beam: depth must be given with it (1 .. 11)")
            beam = NTupleBeamPolicy(env, self.table, *_beam_shape(depth, width), gamma=greedy.gamma, bound=bound)
            player, arguments = beam, dict(after=self._next)
        else:
            if (depth is not None and _depth(depth) != self.depth) or bound != greedy.bound:
                greedy = NTuplePolicy(env, self.table, greedy.gamma, 0.0, greedy.seed, self.depth if depth is None else depth, bound=bound)
            player, arguments = greedy, dict(after=self._next, step=0)
        prover = None if proof is None else ProofPolicy(env, player, max_nodes=proof, **order)
        act = lambda: (player if prover is None else prover).act(out=self._action, **arguments)
        episodes = torch.zeros(env.num_envs, dtype=torch.int32, device=d)
        wins = torch.zeros(env.num_envs, dtype=torch.int32, device=d)
        env.reset()
        tally = None
        if per_config:
            from .curriculum import PoolTally
            tally = PoolTally(env)
        for _ in range(steps):
            action = act()
            if tally is not None:
                tally.observe(action)
            env.step_into(action, self._reward, self._done)
            episodes += self._done
            won = ((self._next[1][:, 1] >> 28) & 3) == _STATE_WON             # an auto-reset board runs whenever it is asked to act
            wins += won if prover is None else torch.where(prover.played, prover.finishing, won)
        self.forget()
        ep, wn = int(episodes.sum(dtype=torch.int64)), int(wins.sum(dtype=torch.int64))
        result = dict(episodes=ep, wins=wn, win_rate=wn / max(ep, 1))
        if tally is not None:
            result.update(episodes_by_config=tally.episodes, wins_by_config=tally.wins)
        if prover is not None:
            result["proof"] = prover.stats()
        return result


RANK_OUTPUTS = ("win", "loss", "greedy", "violated", "gap", "err_win", "err_loss", "win_a", "win_b", "loss_a", "loss_b")


def _rank_table(table) -> torch.Tensor:
    """A table the ranking update teaches: a contiguous int32 tensor of one of the four plain forms on a GPU."""
    counts = {_learn_lib.ntuple_entries_of(name): name for name in _learn_lib.NTUPLE_RANK_FORMS}
    sizes = ", ".join(f"{k} ({v!r})" for k, v in counts.items())
    if not isinstance(table, torch.Tensor) or table.dim() != 1 or table.dtype != torch.int32 or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous int32 tensor of {sizes} entries (ntuple_table)")
    if int(table.shape[0]) not in counts:
        raise ValueError(f"table must be of one of the four plain forms, {sizes} entries: a sum or a staged table is taught no ranking; "
                         f"got {int(table.shape[0])} entries")
    if table.device.type != "cuda":
        raise ValueError(f"table must be on a GPU (cuda:N), not on {table.device}: the ranking update has no CPU path")
    return table


class NTupleRanker:
    """A supervised ranking update of an n-tuple table from proved move labels (the rule: include/tpl_learn.h, tpl_ntuple_rank; the
    kernel: csrc/learn/ntuple_rank.hip).  A label row (T.label_moves, T.label_states) says which placements of a board are proved
    winning (1) and which proved losing (2); **label 3 proves nothing and teaches nothing**.  rank() scores every distinct placement as
    NTuplePolicy does, names the best-scored proved win, the best-scored proved loss and the greedy choice, and says whether the table
    prefers the win by more than `margin`; step() then adds rint(rate) to the entries of the win's afterstate and subtracts it from the
    loss's, through the update kernels the learner uses -- a perceptron step on the hardest pair.  The table is read by one kernel and
    only added to by the others, so a step leaves the same bytes in any order and two runs give the same table.

    `table` is one of the four plain forms ("2x4", "3x3", "feat", "feat+spare") on a GPU and is TAUGHT IN PLACE, as the policies read it
    in place.  L and M are the game's; reward = (r_line, r_win, r_lose) as an environment's.  bound=True (a "feat+spare" table only) is
    the dead-board prune of NTuplePolicy(bound=True); symmetric=True adds every update to the reflected board's entries as well."""

    def __init__(self, table: torch.Tensor, L: int, M: int, gamma: float = 0.99, reward=(1.0, 0.0, 0.0), rate: float = 8.0,
                 margin: float = 0.0, bound: bool = False, symmetric: bool = False):
        self.table = _rank_table(table)
        self.shape = ntuple_shape(self.table)
        if isinstance(L, bool) or not isinstance(L, int) or not 1 <= L <= 250:
            raise ValueError(f"L must be an integer in [1, 250], got {L!r}")
        if isinstance(M, bool) or not isinstance(M, int) or not 1 <= M <= 254:
            raise ValueError(f"M must be an integer in [1, 254], got {M!r}")
        self.L, self.M = int(L), int(M)
        self.gamma, self.rate, self.margin = _finite("gamma", gamma), _finite("rate", rate), _finite("margin", margin)
        if isinstance(reward, (str, bytes)) or not hasattr(reward, "__len__") or len(reward) != 3:
            raise ValueError(f"reward must be three numbers (r_line, r_win, r_lose), got {reward!r}")
        self.reward = tuple(_finite(f"reward[{j}]", v) for j, v in enumerate(reward))
        self.bound = _bound(bound, self.shape)
        if not isinstance(symmetric, bool):
            raise ValueError(f"symmetric must be True or False, got {symmetric!r}")
        self.symmetric = symmetric
        self.device = self.table.device

    def buffers(self, k: int) -> dict:
        """The eleven outputs of rank() for k states, uninitialised, on the table's device: pass them as out= to allocate nothing."""
        d, k = self.device, _count("k", k, 1)
        out = {name: torch.empty(k, dtype=torch.uint8, device=d) for name in RANK_OUTPUTS[:4]}
        out.update({name: torch.empty(k, dtype=torch.float32, device=d) for name in RANK_OUTPUTS[4:7]})
        out.update({name: torch.empty((k, 4), dtype=torch.int32, device=d) for name in RANK_OUTPUTS[7:]})
        return out

    def _inputs(self, planes, label, out):
        k, a, b = _planes(planes, self.device, "planes")
        if not 1 <= k <= _MAX_BOARDS:
            raise ValueError(f"rank takes 1 .. {_MAX_BOARDS} states")
        if (not isinstance(label, torch.Tensor) or label.dtype != torch.uint8 or tuple(label.shape) != (k, 40) or label.device != self.device
                or not label.is_contiguous()):
            raise ValueError(f"label must be a contiguous uint8 tensor of shape ({k}, 40) on {self.device}")
        if out is None:
            out = self.buffers(k)
        else:
            if not isinstance(out, dict) or set(out) != set(RANK_OUTPUTS):
                raise ValueError(f"out must be a dict of {RANK_OUTPUTS} (NTupleRanker.buffers)")
            for j, name in enumerate(RANK_OUTPUTS):
                dtype = torch.uint8 if j < 4 else torch.float32 if j < 7 else torch.int32
                shape = (k,) if j < 7 else (k, 4)
                t = out[name]
                if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != self.device
                        or not t.is_contiguous()):
                    raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
        return k, a, b, out

    @torch.no_grad()
    def rank(self, planes, label: torch.Tensor, out: Optional[dict] = None) -> dict:
        """tpl_ntuple_rank on K states: planes a pair of int32 [K, 4] tensors, label uint8 [K, 40], both on the table's device.
        Returns a dict of device tensors: win, loss, greedy, violated uint8 [K] (win = loss = 255 where the node is undecided: a
        finished board, or no distinct placement labelled 1, or none labelled 2); gap, err_win, err_loss float32 [K]; win_a, win_b,
        loss_a, loss_b int32 [K, 4], the two afterstates.  The table is only read.  One launch, no host sync, and no allocation when
        out= (buffers(K)) is given."""
        k, a, b, out = self._inputs(planes, label, out)
        stream = torch._C._cuda_getCurrentRawStream(self.device.index)
        check(_learn_lib.lib().tpl_ntuple_rank(a.data_ptr(), b.data_ptr(), k, self.L, self.M, self.table.data_ptr(), int(self.table.shape[0]),
                                               label.data_ptr(), *self.reward, self.gamma, self.margin, int(self.bound),
                                               *(out[name].data_ptr() for name in RANK_OUTPUTS), stream))
        return out

    def _update(self, k: int, a: torch.Tensor, b: torch.Tensor, error: torch.Tensor, stream) -> None:
        """rint(rate * error) on the entries of k afterstates: the update entry of the table's form on a ring of one slot."""
        lib = _learn_lib.lib()
        head = (a.data_ptr(), b.data_ptr(), k, 1, 0, 1, self.L, self.M, self.table.data_ptr(), error.data_ptr(), self.rate, 1.0,
                int(self.symmetric))
        if self.shape in NTUPLE_BUDGET_FORMS:
            check(lib.tpl_ntuple_update_trace_budget(*head, stream))
        elif self.shape in NTUPLE_FEATURE_FORMS:
            check(lib.tpl_ntuple_update_trace_feature(*head, stream))
        else:
            check(lib.tpl_ntuple_update_trace_shaped(*head, NTUPLE_SHAPE_IDS[self.shape], stream))

    @torch.no_grad()
    def step(self, planes, label: torch.Tensor, out: Optional[dict] = None) -> dict:
        """One teaching step: rank(), then the update of the win afterstates with err_win and of the loss afterstates with err_loss.
        Three enqueues, no host sync.  Returns rank()'s dict, which describes the table BEFORE the adds."""
        out = self.rank(planes, label, out)
        k = int(label.shape[0])
        stream = torch._C._cuda_getCurrentRawStream(self.device.index)
        self._update(k, out["win_a"], out["win_b"], out["err_win"], stream)
        self._update(k, out["loss_a"], out["loss_b"], out["err_loss"], stream)
        return out

    @torch.no_grad()
    def fit(self, labelset, epochs: int, batch: int, seed: int = 0) -> list:
        """`epochs` passes over a LabelSet (anything with planes_a, planes_b int32 [K, 4] and label uint8 [K, 40] on the table's device),
        `batch` nodes a step in the order of a permutation seeded by `seed` (_learn_lib.rank_fit_order; the last minibatch of an epoch
        may be short).  Returns the violated count of every epoch -- each node counted when its minibatch was ranked, before that
        minibatch's adds -- with one host read an epoch."""
        epochs, batch, seed = _count("epochs", epochs, 1), _count("batch", batch, 1), _count("seed", seed)
        k, a, b = _planes((labelset.planes_a, labelset.planes_b), self.device, "labelset planes")
        label = labelset.label
        if k < 1 or not isinstance(label, torch.Tensor) or label.dtype != torch.uint8 or tuple(label.shape) != (k, 40) or label.device != self.device:
            raise ValueError(f"labelset must hold at least one node, with label a uint8 tensor of shape ({k}, 40) on {self.device}")
        order = torch.from_numpy(_learn_lib.rank_fit_order(k, epochs, seed)).to(self.device)
        buffers = {}
        counts = []
        for e in range(epochs):
            total = torch.zeros((), dtype=torch.int64, device=self.device)
            for lo in range(0, k, batch):
                pick = order[e, lo:lo + batch]
                size = int(pick.shape[0])
                if size not in buffers:
                    buffers[size] = self.buffers(size)
                out = self.step((a[pick], b[pick]), label[pick], buffers[size])
                total += out["violated"].sum(dtype=torch.int64)
            counts.append(int(total))
        return counts
