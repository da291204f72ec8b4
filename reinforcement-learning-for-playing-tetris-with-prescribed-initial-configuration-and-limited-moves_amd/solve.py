"""A whole-game beam solver for prescribed configurations (include/tpl_learn.h: tpl_placement_solve; csrc/learn/solve.hip).

Every policy here plans from an environment state, which shows at most twelve pieces.  A prescribed configuration is a board and
the WHOLE list of its M + 1 pieces; `solve_configs` runs the placement beam of `BeamPolicy` through that list, one workgroup per
configuration, stops at the first ply at which it sees a win and returns the moves.  What it is for: deciding which forward-generated
games to keep (`ForwardGames(solver="beam")`), checking pools from files for winnability on the device, and building pools with a
tighter move budget from the solution lengths (`tighten_pool`).

`solved = False` means that this beam, with these weights at this width, found no win.  It does NOT mean that there is none --
unless the search was the bounded one and `complete`: `solve_configs(bound=True)` prunes every board that the move bound
(include/tpl_learn.h) proves lost, reports `bound`, the least number of moves any solution can take (`config_bound` gives it alone),
and `complete`, under which `solved = False` IS a proof that there is no win and `solved = True` that the solution is the shortest.

`prove_configs` is the search that has no width to cut with: a depth-first search of the same game (tpl_placement_exact;
csrc/learn/exact.hip), one wavefront per configuration, which within the move bound's prune visits every running board or stops at a
node budget and says so (`proved`).  Its weights do one thing, they order a node's children; `ntuple_prove_configs` is the same search
with that order taken from an n-tuple table (tpl_ntuple_exact; csrc/learn/ntuple_exact.hip): a child is worth what the one-ply table
policy scores a move with, read at the budget of the iteration.  Verdicts do not depend on the order; the nodes a proof takes do.

`prove_nodes` starts that search at any node of a game -- a board, its lines and moves, and the list of its configuration -- instead
of at move 0 (tpl_placement_exact_nodes; csrc/learn/exact_nodes.hip): for the search a node is a fresh configuration of the game
(L - lines, M - moves).  `label_moves` applies it to the children of a node and labels every move proved winning, proved losing
or unproved (tpl_placement_exact_labels), `label_states` does so for the boards of an environment, and `blunders` marks where a
proved-losing move was taken although a proved-winning one was there.

`window_prove` is the exact search an honest agent can run: it searches over the pieces a state's own window shows, known =
12 - moves mod 10 of them, instead of a configuration's list (tpl_placement_window_prove; csrc/learn/exact_window.hip).  A win it
finds is a win of the real game; no win proves a loss only where the window reaches the end of the game, and otherwise proves
nothing.  `ProofPolicy` wraps any policy with it: a proved plan's move where there is one, the base policy's move elsewhere.
`ntuple_window_prove` is that search with its children ordered by an n-tuple table, as `ntuple_prove_configs` is `prove_configs`'
(tpl_ntuple_window_prove; csrc/learn/ntuple_window.hip), and `ProofPolicy(table=...)` plays with it.

`collect_labels` plays a policy on an environment with a pool and keeps the boards the labels decide -- a proved win and a proved loss
among their moves -- in a `LabelSet`, the input of `NTupleRanker.fit` (ntuple.py); `label_agreement` counts how often a table's greedy
move is labelled 1, 2 and 3 on such nodes.
"""
from __future__ import annotations

import numpy as np

from ._learn_lib import BEAM_MAX_WIDTH, EXACT_MAX_NODES, NUM_FEATURES, NUM_MOVE_FEATURES, SOLVE_MAX_MOVES

__all__ = ["CLASSICAL_WEIGHTS", "solve_configs", "prove_configs", "ntuple_prove_configs", "tighten_pool", "config_bound",
           "prove_nodes", "label_moves", "label_states", "blunders", "LabelSet", "collect_labels", "label_agreement", "window_prove",
           "ProofPolicy", "ntuple_window_prove", "TableProofPolicy", "prove_configs_limited", "ntuple_prove_configs_limited",
           "window_prove_limited", "ntuple_window_prove_limited", "LimitedProofPolicy"]

# cleared, won, lost, holes, aggregate height, max height, bumpiness, row and column transitions, wells, rows with holes, hole depth:
# the classical signs, a sensible default for the supply (0.99925 of a carved L = 10 / M = 40 pool at one ply)
CLASSICAL_WEIGHTS = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
CLASSICAL_WEIGHTS.setflags(write=False)


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _game(L, M) -> tuple:
    for name, v, hi in (("L", L, 250), ("M", M, SOLVE_MAX_MOVES)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in [1, {hi}], got {v!r}")
    return int(L), int(M)


def _width(width) -> int:
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= int(width) <= BEAM_MAX_WIDTH:
        raise ValueError(f"width must be an integer in [1, {BEAM_MAX_WIDTH}], got {width!r}")
    return int(width)


def _weight_row(weights) -> np.ndarray:
    """None -> CLASSICAL_WEIGHTS; anything array-like of twelve numbers -> a finite float32 [12]; of fourteen (the 14-feature form
    with landing_height and eroded_cells) -> a finite float32 [14]."""
    if weights is None:
        return CLASSICAL_WEIGHTS.copy()
    if _is_tensor(weights):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights)
    if w.dtype == object or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
        raise ValueError(f"weights must be {NUM_FEATURES} numbers (or {NUM_MOVE_FEATURES})")
    if w.shape not in ((NUM_FEATURES,), (1, NUM_FEATURES), (NUM_MOVE_FEATURES,), (1, NUM_MOVE_FEATURES)):
        raise ValueError(f"weights must be one row of shape [{NUM_FEATURES}] or [{NUM_MOVE_FEATURES}], got {tuple(w.shape)}")
    with np.errstate(over="ignore"):
        w = np.ascontiguousarray(w.reshape(-1), dtype=np.float32)
    if not np.isfinite(w).all():
        raise ValueError("weights must be finite (in float32)")
    return w


def _shapes(rows, pieces, M: int) -> int:
    """The shapes solve_configs takes, checked before anything moves to the device; returns n."""
    rs, ps = tuple(rows.shape), tuple(pieces.shape)
    n = rs[0] if rs else 0
    if not (rs == (n, 20) or rs == (n, 20, 10)) or ps not in ((n, M + 1), (n, M)):
        raise ValueError(f"rows must be [n, 20] row masks or [n, 20, 10] cells and pieces [n, {M + 1}] or [n, {M}]; got {rs} {ps}")
    if n < 1:
        raise ValueError("at least one configuration is needed")
    return n


def _spare_weight(spare_weight, bound) -> float:
    """The validated spare_weight of a bounded search: one finite float32; anything but 0 needs bound=True."""
    if not isinstance(bound, (bool, np.bool_)):
        raise ValueError(f"bound must be True or False, got {bound!r}")
    if isinstance(spare_weight, bool) or not isinstance(spare_weight, (int, float, np.integer, np.floating)):
        raise ValueError(f"spare_weight must be a number, got {spare_weight!r}")
    with np.errstate(over="ignore"):
        value = np.float32(spare_weight)
    if not np.isfinite(value):
        raise ValueError("spare_weight must be finite (in float32)")
    if value != 0 and not bound:
        raise ValueError("spare_weight belongs to the bounded search: give bound=True")
    return float(value)


def _device_rows(rows, d):
    """rows as solve_configs takes them -> a contiguous int16 / uint16 [n, 20] tensor on device d."""
    import torch
    if not _is_tensor(rows):
        if rows.ndim == 3:
            rows = (rows.astype(np.uint16) << np.arange(10, dtype=np.uint16)).sum(-1).astype(np.uint16)
        rows = torch.from_numpy(np.ascontiguousarray(rows.astype(np.uint16)).view(np.int16))
    elif rows.dim() == 3:
        rows = (rows.to(torch.int32) << torch.arange(10, device=rows.device, dtype=torch.int32)).sum(-1).to(torch.int16)
    rows = rows.to(d).contiguous()
    if rows.dtype not in (torch.int16, torch.uint16):
        rows = rows.to(torch.int16)
    return rows


def _device_pieces(pieces, n: int, M: int, d, validate: bool):
    """pieces as solve_configs takes them -> a contiguous uint8 [n, M + 1] tensor on device d, [n, M] padded with piece 0; the
    piece-id check (one host wait) unless validate is False."""
    import torch
    if not _is_tensor(pieces):
        pieces = torch.as_tensor(np.ascontiguousarray(pieces.astype(np.uint8)))
    pieces = pieces.to(device=d, dtype=torch.uint8)
    if pieces.shape[1] == M:
        pieces = torch.cat([pieces, torch.zeros((n, 1), dtype=torch.uint8, device=d)], dim=1)
    pieces = pieces.contiguous()
    if validate and int(pieces.max()) > 6:
        raise ValueError("piece ids must be in 0..6 (I L J T S Z O)")
    return pieces


def _solution(actions):
    """actions uint8 [n, M] (255 behind the end) -> uint8 [n, M, 2] as (rotations, location), zero behind the end."""
    import torch
    played = actions != 255
    a = torch.where(played, actions, torch.zeros_like(actions))
    return torch.stack([a // 10, a % 10], dim=2).to(torch.uint8)


def config_bound(rows, L: int, device="cuda:0"):
    """The least number of moves any solution of each configuration can take (include/tpl_learn.h: the move bound;
    tpl_move_bound_rows): int32 [n] on `device`, ceil(cells / 4) with cells the cells missing from the L cheapest rows.  rows as
    solve_configs takes them: tensors or arrays, [n, 20] row masks or [n, 20, 10] cells.  A configuration whose budget M is below
    this has no solution, whatever its pieces."""
    import torch
    from . import _learn_lib
    L, _ = _game(L, 1)
    if not _is_tensor(rows):
        rows = np.asarray(rows)
    rs = tuple(rows.shape)
    n = rs[0] if rs else 0
    if not (rs == (n, 20) or rs == (n, 20, 10)):
        raise ValueError(f"rows must be [n, 20] row masks or [n, 20, 10] cells; got {rs}")
    if n < 1:
        raise ValueError("at least one configuration is needed")
    d = torch.device(device)
    rows = _device_rows(rows, d)
    cells = torch.empty(n, dtype=torch.int32, device=d)
    stream = torch._C._cuda_getCurrentRawStream(d.index if d.index is not None else torch.cuda.current_device())
    _learn_lib.check(_learn_lib.lib().tpl_move_bound_rows(rows.data_ptr(), n, L, cells.data_ptr(), stream))
    return (cells + 3) // 4


def solve_configs(rows, pieces, L: int, M: int, weights=None, width: int = 16, device="cuda:0", best_value: bool = False,
                  validate: bool = True, bound: bool = False, spare_weight: float = 0.0) -> dict:
    """Search every configuration's whole game with the placement beam (the rule: include/tpl_learn.h, tpl_placement_solve).

    rows: [n, 20] int16 / uint16 (bit x = column x) or [n, 20, 10] bool, converted as `load_configs` converts them; pieces:
    [n, M + 1] uint8, or [n, M] (padded with piece 0: the piece behind the last move is never played); weights: one row of twelve
    (None = CLASSICAL_WEIGHTS) or of fourteen, which selects the 14-feature form; width in [1, 64].  Tensors or arrays; everything is enqueued on the current stream of `device`.
    Returns a dict of device tensors: solved bool [n], solution_len int32 [n], actions uint8 [n, M] (placements 10 r + l, 255
    behind the end), solution uint8 [n, M, 2] as (rotations, location) -- the layout of carved_configs(with_solutions=True) and
    forward_configs, zero behind the end -- and, with best_value=True, best_value float32 [n, M]: the value of the best candidate
    of every ply run, +0 behind.

    solved[i] = False means that THIS beam found no win for configuration i, not that there is none.

    bound=True searches in the bounded form (tpl_placement_solve_bound): a move that leaves a board which the move bound proves lost
    -- the cells missing from the rows still owed cannot be supplied in the moves left -- leaves it lost, and spare_weight (one
    finite number, 0 by default; refused without bound=True) times a node's spare cells is added to its value.  The dict then also
    holds bound int32 [n], the least number of moves any solution can take; complete bool [n], set where no cut dropped a running
    candidate; and optimal bool [n] = solved & ((solution_len == bound) | complete).  **With complete[i] set, solved[i] = False is a
    proof that configuration i has no win within M moves, and solved[i] = True a proof that solution_len[i] is the shortest there
    is; without it, solved[i] = False still proves nothing.**  bound=False launches the unbounded entry and returns its dict.
    No host wait except the piece-id check (ids 0..6, as load_configs'), which validate=False skips."""
    import torch
    from . import _learn_lib
    L, M = _game(L, M)
    width = _width(width)
    w = _weight_row(weights)
    spare_weight = _spare_weight(spare_weight, bound)
    if not _is_tensor(rows):
        rows = np.asarray(rows)
    if not _is_tensor(pieces):
        pieces = np.asarray(pieces)
    n = _shapes(rows, pieces, M)
    d = torch.device(device)
    rows = _device_rows(rows, d)
    pieces = _device_pieces(pieces, n, M, d, validate)
    wt = torch.from_numpy(_learn_lib.padded_weights(w)).to(d)
    out = dict(solved=torch.empty(n, dtype=torch.uint8, device=d), solution_len=torch.empty(n, dtype=torch.int32, device=d),
               actions=torch.empty((n, M), dtype=torch.uint8, device=d))
    if best_value:
        out["best_value"] = torch.empty((n, M), dtype=torch.float32, device=d)
    stream = torch._C._cuda_getCurrentRawStream(d.index if d.index is not None else torch.cuda.current_device())
    head = (rows.data_ptr(), pieces.data_ptr(), n, L, M, wt.data_ptr(), width)
    outs = (out["solved"].data_ptr(), out["solution_len"].data_ptr(), out["actions"].data_ptr(),
            out["best_value"].data_ptr() if best_value else None)
    if bound:
        out["bound"] = torch.empty(n, dtype=torch.int32, device=d)
        out["complete"] = torch.empty(n, dtype=torch.uint8, device=d)
        _learn_lib.check(_learn_lib.entry("solve", w.shape[0], bound=True)(*head, spare_weight, *outs, out["bound"].data_ptr(),
                                                                          out["complete"].data_ptr(), stream))
        out["complete"] = out["complete"].view(torch.bool)
    else:
        _learn_lib.check(_learn_lib.entry("solve", w.shape[0])(*head, *outs, stream))
    out["solved"] = out["solved"].view(torch.bool)
    if bound:
        out["optimal"] = out["solved"] & ((out["solution_len"] == out["bound"]) | out["complete"])
    out["solution"] = _solution(out["actions"])
    return out


def _max_nodes(max_nodes) -> int:
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or not 1 <= int(max_nodes) <= EXACT_MAX_NODES:
        raise ValueError(f"max_nodes must be an integer in [1, {EXACT_MAX_NODES}], got {max_nodes!r}")
    return int(max_nodes)


def _discrepancy(discrepancy, first_limit):
    """(growth, first_limit) of a limited search, or None for discrepancy=None, the plain one.  discrepancy is None, "add" or
    "double"; first_limit an integer in [0, 65535], looked at in every case."""
    from ._learn_lib import DISCREPANCY_GROWTH, LIMIT_TOP
    if discrepancy is not None and (not isinstance(discrepancy, str) or discrepancy not in DISCREPANCY_GROWTH):
        raise ValueError(f'discrepancy must be None, "add" or "double", got {discrepancy!r}')
    if isinstance(first_limit, bool) or not isinstance(first_limit, (int, np.integer)) or not 0 <= int(first_limit) <= LIMIT_TOP:
        raise ValueError(f"first_limit must be an integer in [0, {LIMIT_TOP}], got {first_limit!r}")
    return None if discrepancy is None else (DISCREPANCY_GROWTH[discrepancy], int(first_limit))


def _limited_parts(limited, names: tuple) -> tuple:
    """What a launch splices in for limited = (growth, first_limit): the entry name's suffix, the arguments first_limit and growth, which
    stand ahead of the entry's outputs, and the output names with `limit` behind `nodes`.  For limited = None, the plain entry:
    no suffix, no arguments, the names as they are."""
    if limited is None:
        return "", (), names
    at = names.index("nodes") + 1
    return "_limited", (limited[1], limited[0]), names[:at] + ("limit",) + names[at:]


ROOT_OUTPUTS = ("solved", "proved", "solution_len", "actions", "bound", "nodes")


def _root_buffers(n: int, M: int, d, limited=None) -> dict:
    """The outputs of a search from n roots of the game (L, M), uninitialised on d; `limit` with them for a limited search."""
    import torch
    kinds = dict(solved=torch.uint8, proved=torch.uint8, solution_len=torch.int32, actions=torch.uint8, bound=torch.int32,
                 nodes=torch.int32)
    if limited is not None:
        kinds["limit"] = torch.int32
    return {k: torch.empty((n, M) if k == "actions" else n, dtype=t, device=d) for k, t in kinds.items()}


def _root_result(out: dict, shortest) -> dict:
    """The filled buffers of _root_buffers as prove_configs' dict: the flags as bool, optimal, unwinnable and solution."""
    import torch
    out["solved"], out["proved"] = out["solved"].view(torch.bool), out["proved"].view(torch.bool)
    out["optimal"] = out["solved"] & bool(shortest)
    out["unwinnable"] = out["proved"] & ~out["solved"]
    out["solution"] = _solution(out["actions"])
    return out


def prove_configs(rows, pieces, L: int, M: int, weights=None, max_nodes: int = 1 << 16, shortest: bool = True,
                  spare_weight: float = 0.0, device="cuda:0", validate: bool = True) -> dict:
    """Search every configuration's whole game depth first and exactly (the rule: include/tpl_learn.h, tpl_placement_exact;
    csrc/learn/exact.hip), one wavefront per configuration.

    rows, pieces, weights (None = CLASSICAL_WEIGHTS; fourteen select the 14-feature form), device and validate are solve_configs';
    spare_weight is one finite number added, times a node's spare cells, to its value -- the search is always the bounded one, so it
    needs no switch.  max_nodes in [1, 2^24] caps the nodes a configuration may expand, over all its iterations.  shortest=True
    deepens the move budget from `bound` to M, so that the first win met is a shortest one; shortest=False searches at M alone and
    takes the first win it meets.  The weights only order the children: they decide how many nodes a search takes, not what a search
    that ends finds.
    Returns a dict of device tensors: solved bool [n], proved bool [n], solution_len int32 [n], actions uint8 [n, M] (placements
    10 r + l, 255 behind the end), solution uint8 [n, M, 2] in solve_configs' layout, bound int32 [n] (the least number of moves any
    solution can take), nodes int32 [n] (the nodes expanded, at most 2^24), optimal bool [n] = solved & shortest and unwinnable bool [n] =
    proved & ~solved.

    **proved[i] is set iff the search of configuration i was not stopped by max_nodes.  With it, solved[i] = False IS a proof that no
    sequence of placements wins within M moves, and with shortest=True solved[i] = True a proof that solution_len[i] is the shortest
    there is.  solved[i] = True always comes with proved[i].  Without proved[i] NOTHING is proved, neither way.**
    No host wait except the piece-id check, which validate=False skips."""
    return _prove_configs(rows, pieces, L, M, weights, max_nodes, shortest, spare_weight, device, validate, None, 0)


def prove_configs_limited(rows, pieces, L: int, M: int, discrepancy="add", first_limit: int = 0, **arguments) -> dict:
    """prove_configs in LIMITED-DISCREPANCY ORDER (the rule: include/tpl_learn.h, tpl_placement_exact_limited): the same search, its
    children, stop, budgets and node cap, with the paths that follow the children's order searched first.  The arguments are
    prove_configs', by keyword; the dict is prove_configs' with limit int32 [n], the K of the last iteration begun.
    discrepancy: "add" or "double" -- every budget is searched under a limit K on the steps a path may take off the children's order:
    K = first_limit (an integer in [0, 65535]) first, then K + 1 ("add") or max(1, 2 K) ("double"), until an iteration drops no
    child; `nodes` counts them all.  None is the plain search: the result of prove_configs as it stands, without `limit`.
    **Verdicts do not change: under proved, solved, solution_len, bound and unwinnable are the plain search's.  The solution may
    differ: actions may name another win of the same length, still a shortest one.  first_limit >= 8,382 gives the plain search's
    outputs byte for byte.  Searching out a budget that holds no win takes at most 15 times the plain search's nodes under "double"
    and up to 8,383 times under "add".**  What it buys is proofs within max_nodes where the order is good but not perfect."""
    return _prove_configs(rows, pieces, L, M, **arguments, discrepancy=discrepancy, first_limit=first_limit)


def _prove_configs(rows, pieces, L: int, M: int, weights=None, max_nodes: int = 1 << 16, shortest: bool = True,
                  spare_weight: float = 0.0, device="cuda:0", validate: bool = True, discrepancy=None, first_limit: int = 0) -> dict:
    """prove_configs and prove_configs_limited on their arguments; discrepancy None is the plain search."""
    import torch
    from . import _learn_lib
    L, M = _game(L, M)
    w = _weight_row(weights)
    max_nodes = _max_nodes(max_nodes)
    if not isinstance(shortest, (bool, np.bool_)):
        raise ValueError(f"shortest must be True or False, got {shortest!r}")
    spare_weight = _spare_weight(spare_weight, True)
    limited = _discrepancy(discrepancy, first_limit)
    if not _is_tensor(rows):
        rows = np.asarray(rows)
    if not _is_tensor(pieces):
        pieces = np.asarray(pieces)
    n = _shapes(rows, pieces, M)
    d = torch.device(device)
    rows = _device_rows(rows, d)
    pieces = _device_pieces(pieces, n, M, d, validate)
    wt = torch.from_numpy(_learn_lib.padded_weights(w)).to(d)
    out = _root_buffers(n, M, d, limited)
    stream = torch._C._cuda_getCurrentRawStream(d.index if d.index is not None else torch.cuda.current_device())
    suffix, limits, names = _limited_parts(limited, ROOT_OUTPUTS)
    _learn_lib.check(_learn_lib.entry("exact" + suffix, w.shape[0])(
        rows.data_ptr(), pieces.data_ptr(), n, L, M, wt.data_ptr(), spare_weight, max_nodes, int(bool(shortest)), *limits,
        *(out[k].data_ptr() for k in names), stream))
    return _root_result(out, shortest)


def _node_tensors(rows, lines, moves, entry, pieces, M: int, d, validate: bool):
    """The node arguments of prove_nodes and label_moves, checked before anything moves to the device, as contiguous tensors on
    d: rows int16 [n, 20], lines and moves uint8 [n], entry int32 [n] -- anything outside [0, n_cfg) becomes -1, which the kernels
    read as an entry out of range --, pieces uint8 [n_cfg, M + 1]; and n, n_cfg."""
    import torch
    rows, lines, moves, entry, pieces = (x if _is_tensor(x) else np.asarray(x) for x in (rows, lines, moves, entry, pieces))
    rs, ps = tuple(rows.shape), tuple(pieces.shape)
    n = rs[0] if rs else 0
    if not (rs == (n, 20) or rs == (n, 20, 10)):
        raise ValueError(f"rows must be [n, 20] row masks or [n, 20, 10] cells; got {rs}")
    if n < 1:
        raise ValueError("at least one node is needed")
    if len(ps) != 2 or ps[0] < 1 or ps[1] not in (M + 1, M):
        raise ValueError(f"pieces must be [n_cfg, {M + 1}] or [n_cfg, {M}] with n_cfg >= 1, the lists the entries name; got {ps}")
    n_cfg = ps[0]
    plain = []
    for name, x, top in (("lines", lines, 255), ("moves", moves, 255), ("entry", entry, None)):
        kind = str(x.dtype)
        if tuple(x.shape) != (n,) or "int" not in kind:
            raise ValueError(f"{name} must be {n} integers, one per node; got {tuple(x.shape)} {kind}")
        if not _is_tensor(x):
            if top is not None and n and (x.min() < 0 or x.max() > top):
                raise ValueError(f"{name} must be in [0, {top}]")
            x = torch.from_numpy(np.ascontiguousarray(x.astype(np.int64)))
        plain.append(x)
    lines, moves = (x.to(d).to(torch.uint8).contiguous() for x in plain[:2])
    entry = plain[2].to(d).to(torch.int64)
    entry = torch.where((entry < 0) | (entry >= n_cfg), torch.full_like(entry, -1), entry).to(torch.int32).contiguous()
    return _device_rows(rows, d), lines, moves, entry, _device_pieces(pieces, n_cfg, M, d, validate), n, n_cfg


def prove_nodes(rows, lines, moves, entry, pieces, L: int, M: int, weights=None, max_nodes: int = 1 << 16, shortest: bool = True,
                spare_weight: float = 0.0, device="cuda:0", validate: bool = True) -> dict:
    """prove_configs from any node of a prescribed game (the rule: include/tpl_learn.h, tpl_placement_exact_nodes;
    csrc/learn/exact_nodes.hip), one wavefront per node.

    A node is a board rows[i] ([n, 20] row masks or [n, 20, 10] cells), the lines[i] cleared and the moves[i] made so far (integers
    [n], 0..255), and entry[i] (integers [n]), the row of `pieces` ([n_cfg, M + 1] uint8, or [n_cfg, M]) that holds its
    configuration's list: its next piece is pieces[entry[i], moves[i]].  Nodes of one game share a list; nothing is copied.  The rest
    is prove_configs'.  For the search the node IS the configuration (rows[i], pieces[entry[i], moves[i]:]) of the game
    (L - lines[i], M - moves[i]), and the result is that search's, byte for byte.
    Returns prove_configs' dict: solved, proved, solution_len and actions [n, M] COUNTED FROM THE NODE, solution, bound (the least
    number of further moves any win can take), nodes, optimal = solved & shortest, unwinnable = proved & ~solved.  A node with
    lines >= L, moves >= M or an entry outside the lists is finished: proved, not solved, 0 nodes.

    **proved[i] is set iff the search from node i was not stopped by max_nodes.  With it, solved[i] = False IS a proof that no sequence
    of placements from the node wins within the M - moves[i] moves left.  Without proved[i] NOTHING is proved, neither way.**
    No host wait except the piece-id check, which validate=False skips."""
    import torch
    from . import _learn_lib
    L, M = _game(L, M)
    w = _weight_row(weights)
    max_nodes = _max_nodes(max_nodes)
    if not isinstance(shortest, (bool, np.bool_)):
        raise ValueError(f"shortest must be True or False, got {shortest!r}")
    spare_weight = _spare_weight(spare_weight, True)
    d = torch.device(device)
    rows, lines, moves, entry, pieces, n, n_cfg = _node_tensors(rows, lines, moves, entry, pieces, M, d, validate)
    wt = torch.from_numpy(_learn_lib.padded_weights(w)).to(d)
    out = _root_buffers(n, M, d)
    stream = torch._C._cuda_getCurrentRawStream(d.index if d.index is not None else torch.cuda.current_device())
    _learn_lib.check(_learn_lib.entry("exact_nodes", w.shape[0])(
        rows.data_ptr(), lines.data_ptr(), moves.data_ptr(), entry.data_ptr(), pieces.data_ptr(), n, n_cfg, L, M, wt.data_ptr(),
        spare_weight, max_nodes, int(bool(shortest)), *(out[k].data_ptr() for k in ROOT_OUTPUTS), stream))
    return _root_result(out, shortest)


# ------------------------------------------------------------------------------------------------ the search over a state's window
WINDOW_OUTPUTS = ("solved", "proved", "solution_len", "plan", "bound", "nodes", "horizon", "verdict")


def _resident_planes(env):
    """The two resident state planes of `env` as int32 [N, 4] VIEWS of its workspace (env.raw_planes() returns copies of them)."""
    import torch
    from .lookahead import _state_ptrs
    n, base = env.num_envs, env._workspace.data_ptr()
    return tuple(env._workspace[p - base: p - base + n * 16].view(torch.int32).view(n, 4) for p in _state_ptrs(env))


def _plane_fields(a, b):
    """moves, state and lines (int32 [N] each) of int32 [N, 4] planes (the layout: DESIGN.md section 2)."""
    moves = ((a[:, 1] >> 28) & 15) | (((a[:, 3] >> 28) & 15) << 4)
    return moves, (b[:, 1] >> 28) & 3, (b[:, 2] >> 20) & 255


def _window_buffers(n: int, d, limited=None) -> dict:
    import torch
    kinds = dict(solved=torch.uint8, proved=torch.uint8, solution_len=torch.int32, bound=torch.int32, nodes=torch.int32,
                 horizon=torch.uint8, verdict=torch.uint8)
    if limited is not None:
        kinds["limit"] = torch.int32
    out = {k: torch.empty(n, dtype=t, device=d) for k, t in kinds.items()}
    out["plan"] = torch.empty((n, 12), dtype=torch.uint8, device=d)
    return out


def _window_launch(env, planes, features: int, wt, spare_weight: float, max_nodes: int, skip, out: dict, limited=None) -> None:
    """tpl_placement_window_prove[_move] on the resident boards of `env` into the buffers of _window_buffers; with limited =
    (growth, first_limit) the _limited entry, which also fills out["limit"]."""
    import torch
    from . import _learn_lib
    stream = torch._C._cuda_getCurrentRawStream(env.device.index)
    suffix, limits, names = _limited_parts(limited, WINDOW_OUTPUTS)
    _learn_lib.check(_learn_lib.entry("window_prove" + suffix, features)(
        planes[0], planes[1], env.num_envs, env.L, env.M, wt.data_ptr(), spare_weight, max_nodes, *limits,
        None if skip is None else skip.data_ptr(), *(out[k].data_ptr() for k in names), stream))


def _window_result(env, out: dict) -> dict:
    """The filled buffers of _window_buffers as window_prove's dict: the flags as bool, known and action."""
    import torch
    out["solved"], out["proved"] = out["solved"].view(torch.bool), out["proved"].view(torch.bool)
    moves, _, _ = _plane_fields(*_resident_planes(env))
    out["known"] = (12 - moves % 10).to(torch.uint8)
    out["action"] = out["plan"][:, 0]
    return out


def _skip_mask(env, skip):
    """None, or a contiguous uint8 [N] on the environment's device: nonzero = do not search that board."""
    import torch
    if skip is None:
        return None
    if not _is_tensor(skip):
        skip = torch.from_numpy(np.ascontiguousarray(np.asarray(skip) != 0).view(np.uint8))
    if tuple(skip.shape) != (env.num_envs,) or skip.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"skip must be None or {env.num_envs} flags (bool or uint8), one per board")
    skip = skip.to(env.device)
    return (skip.view(torch.uint8) if skip.dtype == torch.bool else skip).contiguous()


def window_prove(env, weights=None, max_nodes: int = 1 << 12, spare_weight: float = 0.0, skip=None) -> dict:
    """The exact search over the pieces each resident board's window shows (the rule: include/tpl_learn.h,
    tpl_placement_window_prove; csrc/learn/exact_window.hip), one wavefront per board.  Nothing but the state is read: no pool, no
    piece list.

    A running board at moves = m knows known = 12 - m mod 10 true pieces, the falling one first, and has rem = M - m moves left; the
    search is prove_nodes' shortest search of the game (L - lines, H) with the HORIZON H = min(known, rem), its pieces the window's.
    weights (None = CLASSICAL_WEIGHTS; fourteen select the 14-feature form), spare_weight and max_nodes are prove_configs': they
    order the children and cap the nodes of a board, and decide no verdict but between 3 and the two others.  skip: None, or [N] flags
    (bool or uint8) -- a flagged board is not searched: verdict 0, nothing solved or proved, 0 nodes; bound and horizon still stand.
    Returns a dict of device tensors [N]: solved bool, proved bool, solution_len int32, plan uint8 [N, 12] (placements 10 r + l, 255
    behind the end), bound int32 (the least number of moves any win takes), nodes int32, horizon uint8, known uint8,
    action uint8 = plan[:, 0], and verdict uint8:
      0  the board is finished, or was skipped;
      1  WIN: the plan wins the real game in solution_len moves, and no shorter win exists;
      2  LOSS: searched out with the window reaching the end of the game (H == rem): no sequence of placements wins;
      3  OPEN: the node budget stopped the search, or it was searched out with H < rem, which says only that no win lies within the
         known pieces.
    **Verdict 3 proves nothing about the game, neither way.**  Verdicts 1 and 2 do not depend on max_nodes or on the weights.
    The environment is read, never written; no host wait."""
    return _window_prove(env, weights, max_nodes, spare_weight, skip, None, 0)


def window_prove_limited(env, discrepancy="add", first_limit: int = 0, **arguments) -> dict:
    """window_prove in LIMITED-DISCREPANCY ORDER (the rule: include/tpl_learn.h, tpl_placement_window_prove_limited).  The arguments
    are window_prove's, by keyword; the dict is window_prove's with limit int32 [N], the K of the last iteration begun and 0 where
    nothing was searched.  **Verdict 3 still proves nothing about the game.**
    discrepancy: "add" or "double" -- every budget is searched under a limit K on the steps a path may take off the children's order:
    K = first_limit (an integer in [0, 65535]) first, then K + 1 ("add") or max(1, 2 K) ("double"), until an iteration drops no
    child; `nodes` counts them all.  None is the plain search: the result of window_prove as it stands, without `limit`.
    **Verdicts do not change: under proved, solved, solution_len, bound and the verdicts 1 and 2 are the plain search's.  The solution may
    differ: plan may name another win of the same length, still a shortest one.  first_limit >= 8,382 gives the plain search's
    outputs byte for byte.  Searching out a budget that holds no win takes at most 15 times the plain search's nodes under "double"
    and up to 8,383 times under "add".**  What it buys is proofs within max_nodes where the order is good but not perfect."""
    return _window_prove(env, **arguments, discrepancy=discrepancy, first_limit=first_limit)


def _window_prove(env, weights=None, max_nodes: int = 1 << 12, spare_weight: float = 0.0, skip=None, discrepancy=None,
                 first_limit: int = 0) -> dict:
    """window_prove and window_prove_limited on their arguments; discrepancy None is the plain search."""
    import torch
    from . import _learn_lib
    from .lookahead import _boards, _state_ptrs
    _boards(env, "window_prove")
    w = _weight_row(weights)
    max_nodes = _max_nodes(max_nodes)
    spare_weight = _spare_weight(spare_weight, True)
    limited = _discrepancy(discrepancy, first_limit)
    skip = _skip_mask(env, skip)
    wt = torch.from_numpy(_learn_lib.padded_weights(w)).to(env.device)
    out = _window_buffers(env.num_envs, env.device, limited)
    _window_launch(env, _state_ptrs(env), w.shape[0], wt, spare_weight, max_nodes, skip, out, limited)
    return _window_result(env, out)


def _window_table(table, d):
    """A table that orders the window search: _exact_table's, a numpy int32 array uploaded first.  A tensor that already lies
    contiguous on device d is returned as it is, not copied.  d None: checked and left where it is."""
    import torch
    if isinstance(table, np.ndarray) and table.dtype == np.int32 and table.ndim == 1:
        table = torch.from_numpy(np.array(table, np.int32))    # a copy: the array may be read-only
    return _exact_table(table, table.device if d is None and _is_tensor(table) else d)


def _ntuple_window_launch(env, planes, table, reward, gamma: float, max_nodes: int, skip, out: dict, limited=None) -> None:
    """tpl_ntuple_window_prove on the resident boards of `env` into the buffers of _window_buffers; with limited = (growth,
    first_limit) the _limited entry, which also fills out["limit"]."""
    import torch
    from . import _learn_lib
    stream = torch._C._cuda_getCurrentRawStream(env.device.index)
    suffix, limits, names = _limited_parts(limited, WINDOW_OUTPUTS)
    _learn_lib.check(getattr(_learn_lib.lib(), "tpl_ntuple_window_prove" + suffix)(
        planes[0], planes[1], env.num_envs, env.L, env.M, table.data_ptr(), int(table.shape[0]), *reward, gamma, max_nodes, *limits,
        None if skip is None else skip.data_ptr(), *(out[k].data_ptr() for k in names), stream))


def ntuple_window_prove(env, table, gamma: float = 1.0, reward=(1.0, 0.0, 0.0), max_nodes: int = 1 << 12, skip=None) -> dict:
    """window_prove with the children of a node ordered by an n-tuple table instead of a weight row (the rule: include/tpl_learn.h,
    tpl_ntuple_window_prove; csrc/learn/ntuple_window.hip), one wavefront per board.

    table: an int32 tensor on the environment's device (a numpy int32 array is uploaded) of one of the four plain forms -- "2x4",
    "3x3", "feat" or "feat+spare" by its entry count; a sum, a staged or a "3x3+feat" table is refused.  gamma and reward = (r_line,
    r_win, r_lose) are ntuple_prove_configs': a child is worth reward, or reward + gamma * V(its board, the next KNOWN piece) where it
    runs, V read in the game (L - lines, B) of the iteration.  They and the table only order the children: they decide how many nodes
    a search takes, and no verdict but between 3 and the two others.  max_nodes and skip are window_prove's.
    Returns window_prove's dict with the same keys and dtypes.  **Verdict 3 proves nothing about the game, neither way.**
    The environment is read, never written; no host wait."""
    return _ntuple_window_prove(env, table, gamma, reward, max_nodes, skip, None, 0)


def ntuple_window_prove_limited(env, table, discrepancy="add", first_limit: int = 0, **arguments) -> dict:
    """ntuple_window_prove in LIMITED-DISCREPANCY ORDER (the rule: include/tpl_learn.h, tpl_ntuple_window_prove_limited).  The arguments
    are ntuple_window_prove's, by keyword; the dict is its dict with limit int32 [N], the K of the last iteration begun and 0 where
    nothing was searched.  **Verdict 3 still proves nothing about the game.**
    discrepancy: "add" or "double" -- every budget is searched under a limit K on the steps a path may take off the children's order:
    K = first_limit (an integer in [0, 65535]) first, then K + 1 ("add") or max(1, 2 K) ("double"), until an iteration drops no
    child; `nodes` counts them all.  None is the plain search: the result of ntuple_window_prove as it stands, without `limit`.
    **Verdicts do not change: under proved, solved, solution_len, bound and the verdicts 1 and 2 are the plain search's.  The solution may
    differ: plan may name another win of the same length, still a shortest one.  first_limit >= 8,382 gives the plain search's
    outputs byte for byte.  Searching out a budget that holds no win takes at most 15 times the plain search's nodes under "double"
    and up to 8,383 times under "add".**  What it buys is proofs within max_nodes where the order is good but not perfect."""
    return _ntuple_window_prove(env, table, **arguments, discrepancy=discrepancy, first_limit=first_limit)


def _ntuple_window_prove(env, table, gamma: float = 1.0, reward=(1.0, 0.0, 0.0), max_nodes: int = 1 << 12, skip=None,
                        discrepancy=None, first_limit: int = 0) -> dict:
    """ntuple_window_prove and ntuple_window_prove_limited on their arguments; discrepancy None is the plain search."""
    from .lookahead import _boards, _state_ptrs
    _boards(env, "ntuple_window_prove")
    max_nodes = _max_nodes(max_nodes)
    gamma = _number("gamma", gamma)
    reward = _reward(reward)
    limited = _discrepancy(discrepancy, first_limit)
    table = _window_table(table, env.device)
    skip = _skip_mask(env, skip)
    out = _window_buffers(env.num_envs, env.device, limited)
    _ntuple_window_launch(env, _state_ptrs(env), table, reward, gamma, max_nodes, skip, out, limited)
    return _window_result(env, out)


class ProofPolicy:
    """A base policy with proofs on top: act() runs window_prove on the resident boards and plays the first move of the proved plan
    where the verdict is 1 (WIN), and base.act()'s move everywhere else.  `base` is any policy of this environment with act(out=...):
    HeuristicPolicy, BeamPolicy, NTuplePolicy, NTupleBeamPolicy.  weights (None = CLASSICAL_WEIGHTS, or fourteen), max_nodes and
    spare_weight are window_prove's and only order and cap the search.

    **A verdict 1 is a proof: following the plan wins the game in solution_len moves.  Verdicts 2 and 3 change nothing -- the base
    plays --, and 3 proves nothing.**

    A proved plan is KEPT per board and stays live while the board is running, its `moves` is the move the plan expects next AND its
    cells are those the plan's last move was to leave (one afterstate enumeration per act()); anything else -- a reset, a caller
    that stepped with another action -- drops the plan.  Where a later search gives no verdict 1 -- the node budget can stop the
    search from the board one move on although it did not stop the first: the children's values carry the rows cleared on the path,
    and float rounding breaks their many ties differently from another root -- the live plan is followed: a proof once held is not
    thrown away.  reuse=False (the default) searches every board at every act() and takes a new proof over the kept one;
    reuse=True passes the boards that hold a live plan to the kernel as `skip` and follows their plans without searching them again.

    After an act(): `verdict` uint8 [N] (the kernel's; 0 where a board was skipped), `played` bool [N] (the action is a plan's
    move) and `finishing` bool [N] (it is the plan's last move: it wins), `nodes` int32 [N] (0 where nothing was searched).
    stats() counts since construction, on the device.  No host wait in act().

    ProofPolicy(env, base, ..., discrepancy="add", first_limit=0) -- the two given by keyword, with or without the three of a table
    below -- makes a LimitedProofPolicy, whose searches run in limited-discrepancy order.

    ProofPolicy(env, base, ..., table=None, gamma=1.0, reward=(1.0, 0.0, 0.0)) -- the three given by keyword -- makes a
    TableProofPolicy, whose search is ordered by an n-tuple table (below); without them this class is all there is.  Only
    ProofPolicy itself is switched: a subclass of ProofPolicy that wants the table order derives from TableProofPolicy, and one that
    does not is refused `table=` by its own __init__ (a TypeError), as any unknown argument is."""

    _limited = None                                            # (growth, first_limit) in a LimitedProofPolicy: the plain search here

    def __new__(cls, *args, **named):
        # the table-ordered policy is a subclass with three more arguments; ProofPolicy(..., table=...) makes one
        if cls is ProofPolicy and any(k in named for k in ("table", "gamma", "reward")):
            cls = TableProofPolicy
        # and the limited order is a subclass of that one with two more
        if cls in (ProofPolicy, TableProofPolicy) and any(k in named for k in ("discrepancy", "first_limit")):
            cls = LimitedProofPolicy
        return object.__new__(cls)

    def __init__(self, env, base, weights=None, max_nodes: int = 1 << 12, spare_weight: float = 0.0, reuse: bool = False):
        import torch
        from . import _learn_lib
        from .lookahead import _boards, _state_ptrs
        n = _boards(env, "ProofPolicy")
        if not callable(getattr(base, "act", None)):
            raise ValueError("base must be a policy with act(out=...): HeuristicPolicy, BeamPolicy, NTuplePolicy or NTupleBeamPolicy")
        if getattr(base, "env", env) is not env:
            raise ValueError("base belongs to another environment")
        if not isinstance(reuse, (bool, np.bool_)):
            raise ValueError(f"reuse must be True or False, got {reuse!r}")
        w = _weight_row(weights)
        self.env, self.base, self.reuse = env, base, bool(reuse)
        self.features, self.max_nodes = int(w.shape[0]), _max_nodes(max_nodes)
        self.spare_weight = _spare_weight(spare_weight, True)
        d = env.device
        self._weights = torch.from_numpy(_learn_lib.padded_weights(w)).to(d)
        self._ptrs, self._planes = _state_ptrs(env), _resident_planes(env)
        self._out = _window_buffers(n, d, self._limited)
        if self._limited is not None:
            self.limit = self._out["limit"]
        self._index = torch.arange(n, device=d)
        self._counts = torch.zeros(4, dtype=torch.int64, device=d)              # verdicts 1, 2, 3; plan moves played
        # the plans kept: the plan, its length, the next move's index, the `moves` it expects and the cells it is to find
        self._plan = torch.full((n, 12), 255, dtype=torch.uint8, device=d)
        self._length = torch.zeros(n, dtype=torch.int32, device=d)
        self._at = torch.zeros(n, dtype=torch.int32, device=d)
        self._expect = torch.full((n,), -1, dtype=torch.int32, device=d)
        self._cells = torch.zeros((n, 7), dtype=torch.int32, device=d)
        self._holds = torch.zeros(n, dtype=torch.bool, device=d)
        self.verdict, self.nodes = self._out["verdict"], self._out["nodes"]
        self.played = torch.zeros(n, dtype=torch.bool, device=d)
        self.finishing = torch.zeros(n, dtype=torch.bool, device=d)

    @staticmethod
    def _cells_of(a, b):
        """The seven words of a plane pair that hold its cells alone: moves, state, slot, lines and the window masked out."""
        import torch
        return torch.stack([a[..., 0], a[..., 1] & 0x0FFFFFFF, a[..., 2], a[..., 3] & 0x0FFFFFFF, b[..., 0], b[..., 1] & 0x0FFFFFFF,
                            b[..., 2] & 0xFFFFF], dim=-1)

    def _search(self, skip) -> None:
        """The window search of the resident boards into self._out."""
        _window_launch(self.env, self._ptrs, self.features, self._weights, self.spare_weight, self.max_nodes, skip, self._out,
                       self._limited)

    def act(self, out=None, verdict=None, **base_arguments):
        """uint8 [N]: the proved plan's move where this call's verdict is 1 or a live plan is held, base.act(out=out,
        **base_arguments)'s move elsewhere.  `verdict` (uint8 [N], optional) receives the kernel's verdicts.  No host wait."""
        import torch
        from .lookahead import afterstates
        env, n = self.env, self.env.num_envs
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=env.device)
        env._own(out, torch.uint8, "out")
        if verdict is not None:
            env._own(verdict, torch.uint8, "verdict")
        with torch.no_grad():
            self.base.act(out=out, **base_arguments)
            moves, state, _ = _plane_fields(*self._planes)
            same = (self._cells == self._cells_of(*self._planes)).all(dim=1)
            self._holds &= (state == 0) & (moves == self._expect) & same
            skip = self._holds.view(torch.uint8) if self.reuse else None
            self._search(skip)
            found = self._out["verdict"] == 1
            if verdict is not None:
                verdict.copy_(self._out["verdict"])
            self._counts[:3] += torch.stack([(self._out["verdict"] == k).sum() for k in (1, 2, 3)])
            self._plan.copy_(torch.where(found[:, None], self._out["plan"], self._plan))
            self._length.copy_(torch.where(found, self._out["solution_len"], self._length))
            self._at.copy_(torch.where(found, torch.zeros_like(self._at), self._at))
            self._holds |= found
            move = self._plan[self._index, self._at.clamp(0, 11).to(torch.int64)]
            out.copy_(torch.where(self._holds, move, out))
            # what the move is to leave: the cells of its afterstate (the window and the counters are the environment's own)
            after = afterstates(env)
            pick = out.to(torch.int64).clamp(0, 39)
            self._cells.copy_(self._cells_of(after["states_a"][self._index, pick], after["states_b"][self._index, pick]))
            self.played = self._holds.clone()
            self._at += self._holds.to(torch.int32)
            self._expect.copy_(moves + 1)
            self.finishing = self.played & (self._at == self._length)
            self._holds &= self._at < self._length
            self._counts[3] += self.played.sum()
        return out

    def stats(self) -> dict:
        """Counts since construction (one host read): the verdicts 1, 2 and 3 the kernel gave, and the plan moves played."""
        win, loss, open_, played = (int(v) for v in self._counts.cpu())
        return dict(win=win, loss=loss, open=open_, plan_moves=played)


class TableProofPolicy(ProofPolicy):
    """ProofPolicy with the search of every act() ordered by an n-tuple table: ntuple_window_prove for window_prove (the rule:
    include/tpl_learn.h, tpl_ntuple_window_prove).  ProofPolicy(env, base, table=...) makes one.  table, gamma and reward are
    ntuple_window_prove's; they only order the search, so everything a verdict 1 promises stands as it does there.

    **The table tensor is HELD, not copied: a tensor that lies contiguous on the environment's device is read as it stands at each
    act(), so a learner's table orders the proofs with whatever it has learnt by then.**  (A numpy table, or one on another device, is
    uploaded once.)  table together with weights or a non-zero spare_weight is refused: a search has one order.  table=None is
    ProofPolicy as it stands, weights and spare_weight included; a gamma or reward other than the defaults is then refused, since
    nothing would read it.  The kept plans, reuse, stats(), verdict, played, finishing and nodes
    are ProofPolicy's, untouched."""

    def __init__(self, env, base, weights=None, max_nodes: int = 1 << 12, spare_weight: float = 0.0, reuse: bool = False, table=None,
                 gamma: float = 1.0, reward=(1.0, 0.0, 0.0)):
        if table is None:
            if (_number("gamma", gamma), _reward(reward)) != (1.0, (1.0, 0.0, 0.0)):
                raise ValueError("gamma and reward order the search through a table: without table= they are refused, not ignored")
            super().__init__(env, base, weights, max_nodes, spare_weight, reuse)
            self.table = None
            return
        if weights is not None or _spare_weight(spare_weight, True) != 0.0:
            raise ValueError("table orders the search in place of weights and spare_weight: give the table, or those two")
        self.gamma, self.reward = _number("gamma", gamma), _reward(reward)
        table = _window_table(table, None)                     # the form, before anything of the environment is touched
        super().__init__(env, base, None, max_nodes, 0.0, reuse)
        self.table = _window_table(table, env.device)

    def _search(self, skip) -> None:
        if self.table is None:
            return super()._search(skip)
        _ntuple_window_launch(self.env, self._ptrs, self.table, self.reward, self.gamma, self.max_nodes, skip, self._out,
                              self._limited)


class LimitedProofPolicy(TableProofPolicy):
    """ProofPolicy, or with table= TableProofPolicy, with the search of every act() in LIMITED-DISCREPANCY ORDER:
    window_prove_limited for window_prove and ntuple_window_prove_limited for ntuple_window_prove (the rule: include/tpl_learn.h,
    tpl_placement_window_prove_limited).  ProofPolicy(env, base, discrepancy="add") makes one.  discrepancy -- "add", "double", or
    None for the plain search -- and first_limit are window_prove_limited's.  They change which proofs fit max_nodes and nothing a
    verdict 1 promises: following the plan wins the game in solution_len moves.  **Verdict 3 still proves nothing.**
    The kept plans, reuse, stats(), verdict, played, finishing and nodes are ProofPolicy's, untouched; after an act() `limit` int32
    [N] holds the kernel's limits (with a discrepancy)."""

    def __init__(self, env, base, weights=None, max_nodes: int = 1 << 12, spare_weight: float = 0.0, reuse: bool = False, table=None,
                 gamma: float = 1.0, reward=(1.0, 0.0, 0.0), discrepancy="add", first_limit: int = 0):
        self._limited = _discrepancy(discrepancy, first_limit)
        super().__init__(env, base, weights, max_nodes, spare_weight, reuse, table, gamma, reward)


def _best_move(label, length):
    """The lowest placement among the proved-winning ones of least length (uint8 [n]); 255 where none is proved."""
    import torch
    win = label == 1
    key = torch.where(win, length.to(torch.int64), torch.full((), 1 << 40, dtype=torch.int64, device=label.device))
    best = torch.argmin(key * 64 + torch.arange(40, device=label.device), dim=1)      # (length, b) in one word: b < 64
    return torch.where(win.any(dim=1), best, torch.full_like(best, 255)).to(torch.uint8)


def label_moves(rows, lines, moves, entry, pieces, L: int, M: int, weights=None, max_nodes: int = 1 << 12,
                spare_weight: float = 0.0, device="cuda:0", validate: bool = True) -> dict:
    """Every move of every node, proved (the rule: include/tpl_learn.h, tpl_placement_exact_labels; csrc/learn/exact_nodes.hip), one
    wavefront per (node, placement).

    The nodes are prove_nodes'.  Placement b = 10 r + l of node i's piece is made as the search makes a child, and
      label[i, b] = 0   b is no distinct placement of the piece (its canonical form is another b), or the node is finished;
                    1   PROVED WINNING: the move wins, or the shortest search from the board it leaves finds a win; length[i, b] is
                        then the fewest moves from the node, b included, in which a game through b can be won;
                    2   PROVED LOSING: the move ends the game lost or leaves a dead board, or the search from the board it leaves was
                        searched out without a win;
                    3   UNPROVED: that search was stopped by max_nodes, which caps each child on its own.
    **Label 3 proves nothing, neither way: a larger max_nodes may turn it into 1 or into 2.  Labels 1 and 2 do not depend on
    max_nodes or on the weights, which only order the search.**
    Returns a dict of device tensors: label uint8 [n, 40], length int32 [n, 40] (0 unless the label is 1), nodes int32 [n, 40] (the
    nodes the child's search expanded), winning bool [n, 40] = label == 1, and best uint8 [n]: the lowest placement among the
    proved-winning ones of least length, 255 where none is proved.  No host wait except the piece-id check."""
    import torch
    from . import _learn_lib
    L, M = _game(L, M)
    w = _weight_row(weights)
    max_nodes = _max_nodes(max_nodes)
    spare_weight = _spare_weight(spare_weight, True)
    d = torch.device(device)
    rows, lines, moves, entry, pieces, n, n_cfg = _node_tensors(rows, lines, moves, entry, pieces, M, d, validate)
    if 40 * n >= 1 << 31:
        raise ValueError("too many nodes: 40 n must stay below 2^31")
    wt = torch.from_numpy(_learn_lib.padded_weights(w)).to(d)
    out = dict(label=torch.empty((n, 40), dtype=torch.uint8, device=d), length=torch.empty((n, 40), dtype=torch.int32, device=d),
               nodes=torch.empty((n, 40), dtype=torch.int32, device=d))
    stream = torch._C._cuda_getCurrentRawStream(d.index if d.index is not None else torch.cuda.current_device())
    _learn_lib.check(_learn_lib.entry("exact_labels", w.shape[0])(
        rows.data_ptr(), lines.data_ptr(), moves.data_ptr(), entry.data_ptr(), pieces.data_ptr(), n, n_cfg, L, M, wt.data_ptr(),
        spare_weight, max_nodes, *(out[k].data_ptr() for k in ("label", "length", "nodes")), stream))
    out["winning"] = out["label"] == 1
    out["best"] = _best_move(out["label"], out["length"])
    return out


def label_states(env, pieces, weights=None, max_nodes: int = 1 << 12) -> dict:
    """label_moves for every board of an environment that plays a pool: the boards, lines and moves come from env.packed_state(),
    the entries from config_index(env), and `pieces` ([n_cfg, M + 1] uint8) is the piece lists of the pool the environment has
    loaded -- the pieces that load_configs took.  A finished board has no move to label: label 0 throughout, best 255.
    Returns label_moves' dict and, beside it, entry int32 [N] (config_index's, -1 for a finished board of an environment without
    auto-reset) and running bool [N].  The environment is read, never written.  Refused: an environment without a pool, and a
    `pieces` whose shape is not [n_cfg, M + 1] for the pool that is loaded.
    **Label 3 proves nothing** (label_moves)."""
    import torch
    from .curriculum import config_index
    info = env.pool_info()
    if info["n_configs"] == 0:
        raise ValueError("label_states needs an environment with a configuration pool (load_configs first)")
    if not hasattr(pieces, "shape") or tuple(pieces.shape) != (info["n_configs"], env.M + 1):
        raise ValueError(f"pieces must be the loaded pool's lists, [{info['n_configs']}, {env.M + 1}]; "
                         f"got {tuple(getattr(pieces, 'shape', ()))}")
    state = env.packed_state()
    entry = config_index(env)
    running = state["state"] == 0
    lines = torch.where(running, state["lines"], torch.full_like(state["lines"], env.L))      # lines = L: finished for the kernel
    out = label_moves(state["rows"], lines, state["moves"], entry, pieces, env.L, env.M, weights=weights, max_nodes=max_nodes,
                      device=env.device)
    out["entry"], out["running"] = entry, running
    return out


def blunders(label_before, action):
    """Where a game was thrown away: uint8 [n], 1 where the node had a proved-winning move (a label 1 among label_before [n, 40])
    and the action taken ([n], as the labels name it: the canonical placement 10 r + l) is labelled 2, proved losing.  An action
    labelled 3 is no proved blunder.  Tensors give a tensor, arrays an array."""
    if _is_tensor(label_before):
        import torch
        action = torch.as_tensor(action, device=label_before.device).to(torch.int64)
        if label_before.dim() != 2 or label_before.shape[1] != 40 or tuple(action.shape) != (label_before.shape[0],):
            raise ValueError("label_before must be [n, 40] and action [n]")
        taken = torch.gather(label_before, 1, action.clamp(0, 39)[:, None])[:, 0]
        return ((label_before == 1).any(dim=1) & (taken == 2) & (action >= 0) & (action < 40)).to(torch.uint8)
    label_before, action = np.asarray(label_before), np.asarray(action).astype(np.int64)
    if label_before.ndim != 2 or label_before.shape[1] != 40 or action.shape != (label_before.shape[0],):
        raise ValueError("label_before must be [n, 40] and action [n]")
    taken = label_before[np.arange(action.size), np.clip(action, 0, 39)]
    return ((label_before == 1).any(axis=1) & (taken == 2) & (action >= 0) & (action < 40)).astype(np.uint8)


class LabelSet:
    """Labelled nodes for NTupleRanker.fit, as device tensors: planes_a, planes_b int32 [K, 4] (the 32-byte states), label uint8
    [K, 40] (label_moves' rows) and entry int32 [K] (the pool entry a node's game began from; -1 where none is known).  It starts
    empty; append() adds nodes, split() cuts it in two by pool entry, so that no configuration has nodes on both sides."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        self.planes_a = torch.empty((0, 4), dtype=torch.int32, device=self.device)
        self.planes_b = torch.empty((0, 4), dtype=torch.int32, device=self.device)
        self.label = torch.empty((0, 40), dtype=torch.uint8, device=self.device)
        self.entry = torch.empty((0,), dtype=torch.int32, device=self.device)

    def __len__(self) -> int:
        return int(self.label.shape[0])

    def append(self, planes_a, planes_b, label, entry=None) -> "LabelSet":
        """k more nodes: planes int32 [k, 4] each, label uint8 [k, 40], entry [k] integers (None: -1).  Copies are kept."""
        import torch
        for name, t, dtype, tail in (("planes_a", planes_a, torch.int32, (4,)), ("planes_b", planes_b, torch.int32, (4,)),
                                     ("label", label, torch.uint8, (40,))):
            if not _is_tensor(t) or t.dtype != dtype or t.dim() != 2 or tuple(t.shape[1:]) != tail:
                raise ValueError(f"{name} must be a {dtype} tensor of shape [k, {tail[0]}]")
        k = int(label.shape[0])
        if int(planes_a.shape[0]) != k or int(planes_b.shape[0]) != k:
            raise ValueError("planes_a, planes_b and label must hold the same number of nodes")
        if entry is None:
            entry = torch.full((k,), -1, dtype=torch.int32, device=self.device)
        if not _is_tensor(entry) or tuple(entry.shape) != (k,) or entry.dtype.is_floating_point:
            raise ValueError(f"entry must be an integer tensor of shape [{k}]")
        d = self.device
        self.planes_a = torch.cat([self.planes_a, planes_a.to(d)]).contiguous()
        self.planes_b = torch.cat([self.planes_b, planes_b.to(d)]).contiguous()
        self.label = torch.cat([self.label, label.to(d)]).contiguous()
        self.entry = torch.cat([self.entry, entry.to(device=d, dtype=torch.int32)]).contiguous()
        return self

    def select(self, keep) -> "LabelSet":
        """The nodes where `keep` (bool [K]) is set, as a new set."""
        out = LabelSet(self.device)
        return out.append(self.planes_a[keep], self.planes_b[keep], self.label[keep], self.entry[keep])

    def split(self, fraction: float = 0.5, by: str = "entry"):
        """(first, second): by="entry" puts the nodes of the lowest ceil(fraction * E) of the E distinct pool entries into the first set
        and the rest into the second -- no entry has nodes in both --; by="node" cuts the nodes themselves in the order they were
        appended.  One host read."""
        import math
        import torch
        if isinstance(fraction, bool) or not isinstance(fraction, (int, float)) or not 0.0 <= float(fraction) <= 1.0:
            raise ValueError(f"fraction must be a number in [0, 1], got {fraction!r}")
        if by not in ("entry", "node"):
            raise ValueError(f'by must be "entry" or "node", got {by!r}')
        if by == "node":
            cut = math.ceil(float(fraction) * len(self))
            first = torch.arange(len(self), device=self.device) < cut
        else:
            entries = torch.unique(self.entry)                 # sorted
            cut = math.ceil(float(fraction) * int(entries.shape[0]))
            first = torch.isin(self.entry, entries[:cut])
        return self.select(first), self.select(~first)


def collect_labels(env, pieces, policy, steps: int, max_nodes: int = 1 << 12, weights=None) -> LabelSet:
    """Play `steps` steps of policy.act() on an environment that plays a pool and keep what the proofs decide.  Before every step the
    boards are labelled (label_states, max_nodes a child), and every DECIDED running board -- at least one placement labelled 1 and at
    least one labelled 2 -- goes into the returned LabelSet: a copy of its planes, its label row and its pool entry.  **Label 3 proves
    nothing**: a board whose only labels are 3 and 0, or that has no proved win or no proved loss, is not kept.
    The environment is read as label_states reads it and written only through env.step: it ends where `steps` plain steps of the same
    actions leave it.  One host wait a step (the piece-id check of label_moves and the selection)."""
    import torch
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError(f"steps must be an integer of at least 1, got {steps!r}")
    if not hasattr(policy, "act"):
        raise ValueError("policy must have an act() that returns the action of every board (NTuplePolicy, HeuristicPolicy, ...)")
    out = LabelSet(env.device)
    for _ in range(steps):
        labels = label_states(env, pieces, weights=weights, max_nodes=max_nodes)
        row = labels["label"]
        decided = labels["running"] & (row == 1).any(dim=1) & (row == 2).any(dim=1)
        a, b = env.raw_planes()
        out.append(a[decided], b[decided], row[decided], labels["entry"][decided])
        env.step(policy.act(), observe=False)
    return out


def label_agreement(table, planes, label, L: int, M: int, gamma: float = 0.99, reward=(1.0, 0.0, 0.0), margin: float = 0.0,
                    bound: bool = False) -> dict:
    """How a table's one-ply choice sits with the proofs, over the DECIDED nodes of (planes, label) -- running boards with a placement
    labelled 1 and one labelled 2: decided (their number), greedy_win, greedy_loss and greedy_open (how often the table's greedy
    placement, NTuplePolicy's at epsilon 0, is labelled 1, 2 and 3), violated (nodes whose best-scored proved win does not beat their
    best-scored proved loss by more than `margin`) and nodes (all that were given).  This is what NTupleRanker optimises; a greedy move
    labelled 3 is neither right nor wrong, **label 3 proves nothing**.  planes: a pair of int32 [K, 4] tensors; label uint8 [K, 40];
    the other arguments are NTupleRanker's.  One launch and one host read; the table is only read."""
    import torch
    from .ntuple import NTupleRanker
    out = NTupleRanker(table, L, M, gamma=gamma, reward=reward, margin=margin, bound=bound).rank(planes, label)
    decided = out["win"] != 255
    chosen = torch.gather(label, 1, out["greedy"].to(torch.int64)[:, None])[:, 0]
    counts = torch.stack([decided.sum(), (decided & (chosen == 1)).sum(), (decided & (chosen == 2)).sum(), (decided & (chosen == 3)).sum(),
                          out["violated"].sum(dtype=torch.int64)]).tolist()
    return dict(zip(("decided", "greedy_win", "greedy_loss", "greedy_open", "violated"), (int(c) for c in counts)), nodes=int(label.shape[0]))


def _number(name: str, v) -> float:
    """One finite float32 given as a Python or numpy number."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    with np.errstate(over="ignore"):
        value = np.float32(v)
    if not np.isfinite(value):
        raise ValueError(f"{name} must be finite (in float32), got {v!r}")
    return float(value)


def _reward(reward) -> tuple:
    if isinstance(reward, (str, bytes)) or not hasattr(reward, "__len__") or len(reward) != 3:
        raise ValueError(f"reward must be three numbers (r_line, r_win, r_lose), got {reward!r}")
    return tuple(_number(f"reward[{j}]", v) for j, v in enumerate(reward))


def _exact_table(table, d):
    """A table that orders an exact search: a contiguous int32 tensor of one of the four plain forms, moved to device d."""
    from ._learn_lib import NTUPLE_EXACT_FORMS, ntuple_entries_of
    counts = {ntuple_entries_of(name): name for name in NTUPLE_EXACT_FORMS}
    sizes = ", ".join(f"{k} ({v!r})" for k, v in counts.items())
    if not _is_tensor(table) or table.dim() != 1 or str(table.dtype) != "torch.int32":
        raise ValueError(f"table must be an int32 tensor of {sizes} entries (ntuple_table)")
    if int(table.shape[0]) not in counts:
        raise ValueError(f"table must be of one of the four plain forms, {sizes} entries: a sum or a staged table orders no search; "
                         f"got {int(table.shape[0])} entries")
    return table.to(d).contiguous()


def ntuple_prove_configs(rows, pieces, L: int, M: int, table, gamma: float = 1.0, reward=(1.0, 0.0, 0.0), max_nodes: int = 1 << 16,
                         shortest: bool = True, device="cuda:0", validate: bool = True) -> dict:
    """prove_configs with the children of a node ordered by an n-tuple table instead of a weight row (the rule: include/tpl_learn.h,
    tpl_ntuple_exact; csrc/learn/ntuple_exact.hip), one wavefront per configuration.

    rows, pieces, max_nodes, shortest, device and validate are prove_configs'.  table: an int32 tensor of one of the four plain forms
    -- "2x4", "3x3", "feat" or "feat+spare" by its entry count (ntuple_table, NTupleLearner.table); a sum or a staged table is refused.
    A child is worth reward, or reward + gamma * V(its board, the next piece of the list) where it runs, reward = (r_line, r_win,
    r_lose) as an environment's -- what NTuplePolicy(bound=True) scores a move with --, and V is read in the game (L, B) of the
    iteration: at the exact budget the low-spare bins of a table trained on a tight pool.  The table, gamma and the reward only order
    the children: they decide how many nodes a search takes, not what a search that ends finds.
    Returns prove_configs' dict of device tensors: solved, proved, solution_len, actions, solution, bound, nodes, optimal = solved &
    shortest and unwinnable = proved & ~solved; it feeds tighten_pool unchanged.

    **proved[i] is set iff the search of configuration i was not stopped by max_nodes.  With it, solved[i] = False IS a proof that no
    sequence of placements wins within M moves, and with shortest=True solved[i] = True a proof that solution_len[i] is the shortest
    there is.  solved[i] = True always comes with proved[i].  Without proved[i] NOTHING is proved, neither way.**
    No host wait except the piece-id check, which validate=False skips."""
    return _ntuple_prove_configs(rows, pieces, L, M, table, gamma, reward, max_nodes, shortest, device, validate, None, 0)


def ntuple_prove_configs_limited(rows, pieces, L: int, M: int, table, discrepancy="add", first_limit: int = 0, **arguments) -> dict:
    """ntuple_prove_configs in LIMITED-DISCREPANCY ORDER (the rule: include/tpl_learn.h, tpl_ntuple_exact_limited): prove_configs_limited
    with the children ordered by an n-tuple table.  The arguments are ntuple_prove_configs', by keyword; the dict is its dict with
    limit int32 [n], the K of the last iteration begun.
    discrepancy: "add" or "double" -- every budget is searched under a limit K on the steps a path may take off the children's order:
    K = first_limit (an integer in [0, 65535]) first, then K + 1 ("add") or max(1, 2 K) ("double"), until an iteration drops no
    child; `nodes` counts them all.  None is the plain search: the result of ntuple_prove_configs as it stands, without `limit`.
    **Verdicts do not change: under proved, solved, solution_len, bound and unwinnable are the plain search's.  The solution may
    differ: actions may name another win of the same length, still a shortest one.  first_limit >= 8,382 gives the plain search's
    outputs byte for byte.  Searching out a budget that holds no win takes at most 15 times the plain search's nodes under "double"
    and up to 8,383 times under "add".**  What it buys is proofs within max_nodes where the order is good but not perfect."""
    return _ntuple_prove_configs(rows, pieces, L, M, table, **arguments, discrepancy=discrepancy, first_limit=first_limit)


def _ntuple_prove_configs(rows, pieces, L: int, M: int, table, gamma: float = 1.0, reward=(1.0, 0.0, 0.0), max_nodes: int = 1 << 16,
                         shortest: bool = True, device="cuda:0", validate: bool = True, discrepancy=None, first_limit: int = 0) -> dict:
    """ntuple_prove_configs and ntuple_prove_configs_limited on their arguments; discrepancy None is the plain search."""
    import torch
    from . import _learn_lib
    L, M = _game(L, M)
    max_nodes = _max_nodes(max_nodes)
    if not isinstance(shortest, (bool, np.bool_)):
        raise ValueError(f"shortest must be True or False, got {shortest!r}")
    gamma = _number("gamma", gamma)
    r_line, r_win, r_lose = _reward(reward)
    limited = _discrepancy(discrepancy, first_limit)
    if not _is_tensor(rows):
        rows = np.asarray(rows)
    if not _is_tensor(pieces):
        pieces = np.asarray(pieces)
    n = _shapes(rows, pieces, M)
    d = torch.device(device)
    table = _exact_table(table, d)
    rows = _device_rows(rows, d)
    pieces = _device_pieces(pieces, n, M, d, validate)
    out = _root_buffers(n, M, d, limited)
    stream = torch._C._cuda_getCurrentRawStream(d.index if d.index is not None else torch.cuda.current_device())
    suffix, limits, names = _limited_parts(limited, ROOT_OUTPUTS)
    _learn_lib.check(getattr(_learn_lib.lib(), "tpl_ntuple_exact" + suffix)(
        rows.data_ptr(), pieces.data_ptr(), n, L, M, table.data_ptr(), int(table.shape[0]), r_line, r_win, r_lose, gamma, max_nodes,
        int(bool(shortest)), *limits, *(out[k].data_ptr() for k in names), stream))
    return _root_result(out, shortest)


def tighten_pool(rows, pieces, solved, solution_len, M_new: int, bound=None, slack=None):
    """A pool with a tighter move budget: (rows, pieces[:, :M_new + 1]) of the configurations that are `solved` with
    solution_len <= M_new -- a pool for BatchedTetris(L, M_new), every entry of it winnable within M_new moves by the solution
    that was found.  Tensors (one host wait) or arrays; M is read off pieces [n, M + 1].  M_new outside [1, M] is refused, and so
    is a result with nothing left.
    `bound` ([n], config_bound's or solve_configs(bound=True)'s) and `slack` (an integer >= 0), given together, also require
    bound >= M_new - slack: a pool whose budget is provably within `slack` moves of the least any solution can take.
    With prove_configs' solved and solution_len (shortest=True) the kept pool's budget is exact: solution_len is then every
    solved entry's shortest solution, so a proved entry is kept iff it can be won within M_new moves."""
    if (bound is None) != (slack is None):
        raise ValueError("bound and slack go together")
    if slack is not None and (isinstance(slack, bool) or not isinstance(slack, (int, np.integer)) or int(slack) < 0):
        raise ValueError(f"slack must be an integer >= 0, got {slack!r}")
    if len(pieces.shape) != 2 or pieces.shape[1] < 2:
        raise ValueError("pieces must be [n, M + 1]")
    n, M = int(pieces.shape[0]), int(pieces.shape[1]) - 1
    if isinstance(M_new, bool) or not isinstance(M_new, (int, np.integer)) or not 1 <= int(M_new) <= M:
        raise ValueError(f"M_new must be an integer in [1, {M}], got {M_new!r}")
    M_new = int(M_new)
    if tuple(rows.shape[:2]) != (n, 20) or tuple(solved.shape) != (n,) or tuple(solution_len.shape) != (n,):
        raise ValueError(f"rows must be [{n}, 20] and solved and solution_len [{n}]")
    if bound is not None and tuple(bound.shape) != (n,):
        raise ValueError(f"bound must be [{n}]")
    if _is_tensor(rows):
        keep = solved.to(device=rows.device).bool() & (solution_len.to(rows.device) <= M_new)
        if bound is not None:
            import torch
            keep = keep & (torch.as_tensor(bound).to(rows.device) >= M_new - int(slack))
        out = rows[keep], pieces.to(rows.device)[keep][:, :M_new + 1].contiguous()
    else:
        keep = np.asarray(solved).astype(bool) & (np.asarray(solution_len) <= M_new)
        if bound is not None:
            keep = keep & (np.asarray(bound.cpu() if _is_tensor(bound) else bound) >= M_new - int(slack))
        out = np.asarray(rows)[keep], np.ascontiguousarray(np.asarray(pieces)[keep][:, :M_new + 1])
    if out[0].shape[0] == 0:
        raise ValueError(f"no configuration is solved within {M_new} moves: nothing is left of the pool")
    return out
