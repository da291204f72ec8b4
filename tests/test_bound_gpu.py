"""The move bound and the bounded placement kernels on one MI355X (include/tpl_learn.h's rule; tpl_move_bound, tpl_move_bound_rows,
tpl_placement_solve[_move]_bound, tpl_placement_beam[_move]_bound; move_bound, config_bound, solve_configs(bound=True),
BeamPolicy(bound=True)).

  1. tpl_move_bound is the mirror: 4,096 states spread over a (10, 40) game by random play from a carved pool, finished boards among
     them; the one-move game; 64 synthetic boards at L = 250, where the lines owed go past the twenty rows of a board.
  2. tpl_move_bound_rows is the mirror, and carving's sol_len, on both carved fixtures.
  3. THE BOUNDED SOLVER IS THE MIRROR, bit for bit in solved, solution_len, actions, best_value, bound and complete: 32 carved
     configurations a case, each searched at a budget of ITS OWN sol_len and sol_len + 1 (grouped by budget), widths 1 / 3 / 16 / 64,
     twelve and fourteen weights, spare_weight 0 and 0.25, through guard-framed buffers, against tests/golden/bound_mirror.npz
     (tests/test_bound_cpu.py pins the file to the mirror).  In every case with more than one move the bounded outputs differ from
     the unbounded entry's for some configuration at the tight budget; in the one-move game the search ends at the first ply in both
     forms, so there the bounded entry writes its twin's bytes.
  4. one game of 254 moves, bounded, against the recorded mirror.
  5. THE BOUNDED BEAM: (a) its score on freshly reset boards is the bounded solver's best_value at depths 1 .. 12; (b) on 64 mid-game
     and late-game states of a (10, 16) game it is a numpy reference composed ply by ply from the mirror's move, features and bound,
     shapes (1, 1) .. (12, 64) on all 64 states, both feature forms, dead children among the candidates; (c) at spare_weight 0, where that reference
     meets no dead child, it gives the unbounded BeamPolicy's action, score and plan.
"""
import sys

import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from conftest import GOLDEN, load_golden
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np

sys.path.insert(0, GOLDEN)
import make_golden_bound as G  # noqa: E402  -- the cases, the grouping by budget and the gathering of a case's outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARANGE = np.arange(40)


def _m():
    return T._learn_lib


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32))


def _mirror_of(fields, L, M):
    return _m().move_bound(fields["rows"], L, M, fields["lines"].astype(np.int64), fields["moves"].astype(np.int64),
                           fields["state"].astype(np.int64))


def _bound_of(env, A, B):
    """T.move_bound on plane pairs, every output on the host."""
    out = T.move_bound(env, _i32(A).to(DEV), _i32(B).to(DEV))
    assert out["cells"].dtype == torch.int32 and out["spare"].dtype == torch.int32 and out["dead"].dtype == torch.bool
    return {k: _np(v) for k, v in out.items()}


def _same_bound(got, want, what):
    for k in ("cells", "spare", "need", "dead"):
        assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), (what, k)


# ------------------------------------------------------------------------------------------------ 1. tpl_move_bound
def _snapshots(L, M, n, pool, steps, seed):
    """Board i of a non-auto-reset environment after i mod (steps + 1) uniformly random moves: planes uint32 [n, 4] each."""
    env = T.BatchedTetris(L, M, n, device=DEV, seed=seed, auto_reset=False, config_pool=pool)
    env.reset()
    seen = [tuple(_np(x).view(np.uint32).copy() for x in env.raw_planes())]
    for t in range(steps):
        env.step(env.synthetic_actions(t), observe=False)
        seen.append(tuple(_np(x).view(np.uint32).copy() for x in env.raw_planes()))
    pick = np.arange(n) % (steps + 1)
    A = np.stack([seen[p][0][i] for i, p in enumerate(pick)])
    B = np.stack([seen[p][1][i] for i, p in enumerate(pick)])
    return env, A, B


def test_move_bound_is_the_mirror_over_a_whole_game_finished_boards_included():
    f = load_golden("carved_L10_M40.npz")
    L, M, n = 10, 40, 4096
    env, A, B = _snapshots(L, M, n, (f["rows"], f["pieces"]), M, 5)
    fields = R.decode_state(A, B)
    want = _mirror_of(fields, L, M)
    _same_bound(_bound_of(env, A, B), want, "states")
    run = fields["state"] == 0
    # random play tops out long before forty moves run short: finished boards and running ones, none of them dead
    assert (~run).sum() >= 200 and (run & ~want["dead"]).sum() >= 1000
    assert np.unique(fields["moves"]).size >= 12               # early, middle and late states of the boards that last
    # the resident boards, read in place; and guard-framed outputs of an odd count
    res = {k: _np(v) for k, v in T.move_bound(env).items()}
    _same_bound(res, _mirror_of(R.decode_state(*(_np(x).view(np.uint32) for x in env.raw_planes())), L, M), "resident")
    k = 1001
    a, b, cells, spare = Framed(16 * k, 1), Framed(16 * k, 2), Framed(4 * k, 3), Framed(4 * k, 4)
    a.inner().copy_(torch.from_numpy(A[:k].view(np.uint8).reshape(-1)))
    b.inner().copy_(torch.from_numpy(B[:k].view(np.uint8).reshape(-1)))
    _check(_lib().tpl_move_bound(a.ptr(), b.ptr(), k, L, M, cells.ptr(), spare.ptr(), _stream()))
    for x in (a, b, cells, spare):
        x.assert_canary("move_bound")
    assert np.array_equal(cells.host().view(np.int32), want["cells"][:k]) and np.array_equal(spare.host().view(np.int32), want["spare"][:k])
    env.terminate()
    # the same boards under a budget of sixteen moves: there a random move soon leaves a dead board
    rows, pieces = T.tighten_pool(f["rows"], f["pieces"], np.ones(256, bool), f["sol_len"], 16)
    env, A, B = _snapshots(L, 16, 1024, (rows, pieces), 16, 5)
    fields = R.decode_state(A, B)
    want = _mirror_of(fields, L, 16)
    _same_bound(_bound_of(env, A, B), want, "tight states")
    assert want["dead"].sum() >= 10 and ((fields["state"] == 0) & ~want["dead"]).sum() >= 10
    env.terminate()


def test_move_bound_in_the_one_move_game_and_at_250_lines():
    rows, pieces = T.generate_configs(1, 1, 64, seed=3)
    env, A, B = _snapshots(1, 1, 128, (rows, pieces), 1, 2)
    fields = R.decode_state(A, B)
    _same_bound(_bound_of(env, A, B), _mirror_of(fields, 1, 1), "(1, 1)")
    assert (fields["state"] == 0).sum() == 64 and (fields["state"] != 0).sum() == 64
    env.terminate()
    # L = 250: the lines owed go far past the twenty rows of a board
    gen = np.random.default_rng(250)
    n, L, M = 64, 250, 254
    rows = (gen.random((n, 20, 10)) < gen.random((n, 1, 1))).astype(np.uint16)
    rows = (rows << np.arange(10, dtype=np.uint16)).sum(axis=2).astype(np.uint16)
    rows[::4, 15:] = 0x3FF                                     # full rows that stand on the board
    lines, moves = gen.integers(0, 250, n), gen.integers(0, 254, n)
    lines[:4], moves[:4] = (0, 249, 0, 249), (0, 0, 253, 253)
    state = np.where(np.arange(n) % 8 == 7, gen.integers(1, 4, n), 0)
    A, B = R.pack_state(rows, lines, moves, state, 0, gen.integers(0, 1 << 36, n).astype(np.uint64))
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=1)
    want = _m().move_bound(rows, L, M, lines, moves, state)
    _same_bound(_bound_of(env, A, B), want, "L = 250")
    assert want["cells"].max() > 2000 and want["dead"].any() and (~want["dead"] & (state == 0)).any()
    env.terminate()


# ------------------------------------------------------------------------------------------------ 2. tpl_move_bound_rows
@pytest.mark.parametrize("name", ["carved_L10_M40.npz", "carved_L5_M20.npz"])
def test_config_bound_is_the_mirror_and_carvings_solution_length(name):
    f = load_golden(name)
    L = int(f["L"])
    rows = f["rows"]
    want = (_m().move_bound_cells(rows, L) + 3) // 4
    got = T.config_bound(rows, L, device=DEV)
    assert got.dtype == torch.int32 and tuple(got.shape) == (256,)
    assert np.array_equal(_np(got), want) and np.array_equal(_np(got), f["sol_len"])
    cells = ((rows[:, :, None] >> np.arange(10)) & 1).astype(bool)
    assert np.array_equal(_np(T.config_bound(cells, L, device=DEV)), want)
    assert np.array_equal(_np(T.config_bound(torch.from_numpy(rows.view(np.int16).copy()).to(DEV)[3:200], L, device=DEV)), want[3:200])
    for other in (1, 37, 250):                                 # any number of lines, through guard-framed buffers
        r, c = Framed(40 * 255, 1), Framed(4 * 255, 2)
        r.inner().copy_(torch.from_numpy(rows[:255].view(np.uint8).reshape(-1)))
        _check(_lib().tpl_move_bound_rows(r.ptr(), 255, other, c.ptr(), _stream()))
        r.assert_canary("rows"), c.assert_canary("cells")
        assert np.array_equal(c.host().view(np.int32), _m().move_bound_cells(rows[:255], other))


# ------------------------------------------------------------------------------------------------ 3. the bounded solver
NAMES4 = G.NAMES[:4]


def _weight_buffer(w):
    """A weight row as the entries read it: twelve floats, or sixteen with NaN in the two entries that are never read."""
    if w.shape[0] == 12:
        return np.array(w, np.float32)
    out = np.full(16, np.nan, np.float32)
    out[:14] = w
    return out


def _solve(rows, pieces, L, M, w, width, spare=None):
    """tpl_placement_solve[_move]_bound (spare given) or the unbounded twin (spare None) through guard-framed buffers, every output
    filled with 0xCD first."""
    n = rows.shape[0]
    wb = _weight_buffer(w)
    rf, pf, wf = Framed(n * 40, 1), Framed(n * (M + 1), 2), Framed(wb.size * 4, 3)
    rf.inner().copy_(torch.from_numpy(np.ascontiguousarray(rows, np.uint16).view(np.uint8).reshape(-1)))
    pf.inner().copy_(torch.from_numpy(np.ascontiguousarray(pieces, np.uint8).reshape(-1)))
    wf.inner().copy_(torch.from_numpy(wb.view(np.uint8)))
    out = dict(solved=Framed(n, 4), solution_len=Framed(4 * n, 5), actions=Framed(n * M, 6), best_value=Framed(4 * n * M, 7),
               bound=Framed(4 * n, 8), complete=Framed(n, 9))
    for f in out.values():
        f.inner().fill_(0xCD)
    entry = _m().entry("solve", w.shape[0], bound=spare is not None)
    head = (rf.ptr(), pf.ptr(), n, L, M, wf.ptr(), width)
    outs = tuple(out[k].ptr() for k in NAMES4)
    if spare is None:
        _check(entry(*head, *outs, _stream()))
    else:
        _check(entry(*head, float(spare), *outs, out["bound"].ptr(), out["complete"].ptr(), _stream()))
    for name, f in list(out.items()) + [("rows", rf), ("pieces", pf), ("weights", wf)]:
        f.assert_canary((L, M, width, n, name))
    got = (out["solved"].host().copy(), out["solution_len"].host().view(np.int32).copy(), out["actions"].host().reshape(n, M).copy(),
           out["best_value"].host().view(np.float32).reshape(n, M).copy())
    if spare is None:
        assert (out["bound"].host() == 0xCD).all() and (out["complete"].host() == 0xCD).all()
        return got
    return got + (out["bound"].host().view(np.int32).copy(), out["complete"].host().copy())


def _solve_case(rows, pieces, sol_len, L, M, slack, w, width, spare):
    parts = []
    for budget, idx in G.groups(sol_len, slack):
        parts.append((idx, budget, _solve(rows[idx], pieces[idx, :budget + 1], L, budget, w, width, spare)))
    return G.gather(parts, sol_len, slack, M)


@pytest.mark.parametrize("L,M", G.CASES)
def test_the_bounded_solver_is_the_mirror_bit_for_bit_at_budgets_that_make_the_bound_bite(L, M):
    g = load_golden("bound_mirror.npz")
    rows, pieces, sol_len = (g[f"L{L}_M{M}_{k}"] for k in ("rows", "pieces", "sol_len"))
    assert rows.shape == (G.COUNT, 20) and pieces.shape == (G.COUNT, M + 2)
    for F, w in G.weights().items():
        for W in G.WIDTHS:
            for slack in G.SLACKS:
                plain = _solve_case(rows, pieces, sol_len, L, M, slack, w, W, None)
                for spare in G.SPARES:
                    got = _solve_case(rows, pieces, sol_len, L, M, slack, w, W, spare)
                    key = f"L{L}_M{M}_F{F}_W{W}_s{slack}_p{int(spare * 100)}_"
                    for name in G.NAMES:
                        a, b = got[name].view(np.uint8), g[key + name].view(np.uint8)
                        bad = np.argwhere(a != b)
                        assert got[name].dtype == g[key + name].dtype and bad.size == 0, (key, name, len(bad), bad[:4].tolist())
                    differs = sum((got[name].view(np.uint8) != plain[name].view(np.uint8)).reshape(G.COUNT, -1).any(axis=1)
                                  for name in NAMES4).astype(bool)
                    if M == 1:
                        assert not differs.any(), key          # one move: the search ends at the first ply in both forms
                    elif slack == 0 or spare != 0:             # (with a move to spare and no spare term a case may show nothing:
                        assert differs.any(), key              # the recording run of make_golden_bound.py prints the counts)
                    assert np.array_equal(got["bound"], sol_len) and (got["solution_len"][got["solved"] == 1] >= sol_len[got["solved"] == 1]).all()


def test_one_game_of_254_moves_bounded_is_the_recorded_mirror_and_solve_configs_reports_the_proofs():
    g, s = load_golden("bound_mirror.npz"), load_golden("solve_mirror.npz")
    rows, pieces = s["long_rows"], s["long_pieces"]
    got = _solve(rows, pieces, G.LONG_L, G.LONG_M, T.CLASSICAL_WEIGHTS, G.LONG_WIDTH, 0.0)
    for name, x in zip(G.NAMES, got):
        want = g[f"long_L{G.LONG_L}_{name}"]
        assert x.dtype == want.dtype and np.array_equal(x.view(np.uint8), want.view(np.uint8)), name
    assert got[0].all() and got[1].min() >= 240 and (got[4] <= got[1]).all()
    # solve_configs: the bounded dict, and the unbounded one as it was
    L, M = 3, 13
    rows, pieces, sol_len = (g[f"L{L}_M{M}_{k}"] for k in ("rows", "pieces", "sol_len"))
    out = T.solve_configs(rows, pieces[:, :M + 1], L, M, width=16, device=DEV, best_value=True, bound=True, spare_weight=0.25)
    assert set(out) == {"solved", "solution_len", "actions", "solution", "best_value", "bound", "complete", "optimal"}
    assert out["bound"].dtype == torch.int32 and out["complete"].dtype == torch.bool and out["optimal"].dtype == torch.bool
    want = _m().placement_solve(rows, pieces[:, :M + 1], L, M, T.CLASSICAL_WEIGHTS, 16, bound=True, spare_weight=0.25)
    for name, x in zip(G.NAMES, want):
        assert np.array_equal(_np(out[name]).astype(x.dtype).view(np.uint8), x.view(np.uint8)), name
    solved, length, bound, complete = (_np(out[k]) for k in ("solved", "solution_len", "bound", "complete"))
    assert np.array_equal(_np(out["optimal"]), solved & ((length == bound) | complete)) and _np(out["optimal"]).any()
    assert np.array_equal(bound, sol_len) and np.array_equal(_np(T.config_bound(rows, L, device=DEV)), sol_len)
    plain = T.solve_configs(rows, pieces[:, :M + 1], L, M, width=16, device=DEV, best_value=True)
    assert set(plain) == {"solved", "solution_len", "actions", "solution", "best_value"}
    # a pool whose budget is provably the least possible: tighten_pool with the bound
    M_new = int(np.median(sol_len))
    t_rows, t_pieces = T.tighten_pool(torch.as_tensor(rows.view(np.int16)).to(DEV), torch.as_tensor(pieces[:, :M + 1]).to(DEV),
                                      out["solved"], out["solution_len"], M_new, bound=out["bound"], slack=0)
    keep = solved & (length <= M_new) & (bound >= M_new)
    assert keep.any() and np.array_equal(_np(t_rows).view(np.uint16), rows[keep]) and tuple(t_pieces.shape) == (keep.sum(), M_new + 1)
    assert (length[keep] == M_new).all()


# ------------------------------------------------------------------------------------------------ 5. the bounded beam
def reference_beam(fields, L, M, w, depth, width, bound, spare_weight):
    """The beam rule of include/tpl_learn.h on the host, in the bounded form where `bound` is set, composed ply by ply from the
    mirror's own pieces: host_moves_traced, board_features, move_bound, placement_score and beam_select.  fields: decode_state's.
    Returns action, plan, score and dead [n]: whether any candidate of the state's search was a dead child."""
    m = _m()
    w = np.asarray(w, np.float32)
    F = w.shape[0]
    n = fields["rows"].shape[0]
    sw = np.float32(spare_weight)
    moves0, state0, window = fields["moves"].astype(np.int64), fields["state"].astype(np.int64), fields["window"]
    plies = np.where(state0 == 0, np.minimum(depth, 12 - moves0 % 10), 0)
    beams = [dict(rows=fields["rows"][s:s + 1].astype(np.uint16), lines=fields["lines"][s:s + 1].astype(np.int64), moves=moves0[s:s + 1],
                  state=state0[s:s + 1], value=m.placement_score(np.zeros(F, np.int64), w)[None], carry=np.zeros((1, 3), np.int64),
                  path=np.full((1, depth), 255, np.uint8)) for s in range(n)]
    dead_seen = np.zeros(n, bool)
    placements = [np.flatnonzero(m.canonical_actions(p, ARANGE) == ARANGE) for p in range(8)]
    for j in range(int(plies.max(initial=0))):
        act = np.flatnonzero(plies > j)
        cfg, node, place, piece = [], [], [], []
        for s in act:
            cur = int((int(window[s]) >> (3 * j)) & 7)
            run = np.flatnonzero(beams[s]["state"] == 0)
            b = placements[cur]
            cfg.append(np.full(run.size * b.size, s)), node.append(np.repeat(run, b.size)), place.append(np.tile(b, run.size))
            piece.append(np.full(run.size * b.size, cur))
        cfg, node, place, piece = (np.concatenate(x) for x in (cfg, node, place, piece))
        total = cfg.size
        room = max(total, 1)                                   # no child at all where every node of every beam is finished
        c = dict(rows=np.zeros((room, 20), np.uint16), lines=np.zeros(room, np.int64), moves=np.zeros(room, np.int64),
                 state=np.zeros(room, np.int64), value=np.zeros(room, np.float32), carry=np.zeros((room, 3), np.int64))
        place = np.concatenate([place, np.zeros(room - total, np.int64)])
        gather = lambda key: np.concatenate([beams[s][key][node[cfg == s]] for s in act]) if total else None
        p_rows, p_lines, p_moves, p_carry = (gather(k) for k in ("rows", "lines", "moves", "carry"))
        for lo in range(0, total, 1 << 14):
            hi = min(total, lo + (1 << 14))
            r2, n2, l2, m2, s2, _, _, land, erod = m.host_moves_traced(p_rows[lo:hi], piece[lo:hi], place[lo:hi] // 10, place[lo:hi] % 10,
                                                                       L, M, p_lines[lo:hi], p_moves[lo:hi])
            carry = p_carry[lo:hi] + np.stack([n2, land, erod], axis=1)
            spare = np.zeros(hi - lo, np.int64)
            if bound:
                mb = m.move_bound(r2, L, M, l2, m2, s2)
                np.logical_or.at(dead_seen, cfg[lo:hi], mb["dead"])
                s2 = np.where(mb["dead"], 2, s2)
                spare = np.where(mb["dead"], 0, mb["spare"])
            else:
                np.logical_or.at(dead_seen, cfg[lo:hi], m.move_bound(r2, L, M, l2, m2, s2)["dead"])
            psi = np.concatenate([np.stack([carry[:, 0], s2 == 1, s2 >= 2], axis=1).astype(np.int64), m.board_features(r2)]
                                 + ([carry[:, 1:]] if F == 14 else []), axis=1)
            value = m.placement_score(psi, w)
            if bound:
                value = value + sw * spare.astype(np.float32)
            c["rows"][lo:hi], c["lines"][lo:hi], c["moves"][lo:hi], c["state"][lo:hi] = r2, l2, m2, s2
            c["value"][lo:hi], c["carry"][lo:hi] = value, carry
        first = 0
        for s in act:
            beam = beams[s]
            run = beam["state"] == 0
            count = placements[int((int(window[s]) >> (3 * j)) & 7)].size
            sizes = np.where(run, count, 1)
            parent = np.repeat(np.arange(run.size), sizes)
            child = np.full(int(sizes.sum()), -1, np.int64)
            mine = first + np.arange(int(run.sum()) * count)
            first += mine.size
            child[run[parent]] = mine
            moved = child >= 0
            c0 = np.maximum(child, 0)
            value = np.where(moved, c["value"][c0], beam["value"][parent]).astype(np.float32)
            keep = m.beam_select(value, width)
            kp, kc, km = parent[keep], c0[keep], moved[keep]
            path = beam["path"][kp].copy()
            path[km, j] = place[kc][km]
            beams[s] = dict(rows=np.where(km[:, None], c["rows"][kc], beam["rows"][kp]), lines=np.where(km, c["lines"][kc], beam["lines"][kp]),
                            moves=np.where(km, c["moves"][kc], beam["moves"][kp]), state=np.where(km, c["state"][kc], beam["state"][kp]),
                            carry=np.where(km[:, None], c["carry"][kc], beam["carry"][kp]), value=value[keep], path=path)
    best = [int(m.beam_select(beams[s]["value"], 1)[0]) for s in range(n)]
    plan = np.stack([beams[s]["path"][best[s]] for s in range(n)])
    return dict(action=np.where(plies > 0, plan[:, 0], 0).astype(np.uint8), plan=plan,
                score=np.array([beams[s]["value"][best[s]] for s in range(n)], np.float32), dead=dead_seen)


def _beam(env, w, depth, width, bound, spare):
    policy = T.BeamPolicy(env, w, depth, width, bound=bound, spare_weight=spare)
    n = env.num_envs
    score = torch.empty(n, dtype=torch.float32, device=DEV)
    plan = torch.full((n, depth), 77, dtype=torch.uint8, device=DEV)
    action = policy.act(score=score, plan=plan)
    return _np(action), _np(plan), _np(score)


def _same_beam(got, want, what):
    for name, g, w in zip(("action", "plan", "score"), got, (want["action"], want["plan"], want["score"])):
        g, w = (g.view(np.uint32), w.view(np.uint32)) if name == "score" else (g, w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("F", [12, 14])
def test_the_bounded_beams_score_on_fresh_boards_is_the_bounded_solvers_best_value(F):
    g = load_golden("bound_mirror.npz")
    L, M, W, spare = 5, 20, 16, 0.25
    rows, pieces = g[f"L{L}_M{M}_rows"], g[f"L{L}_M{M}_pieces"][:, :M + 1]
    w = G.weights()[F]
    n = rows.shape[0]
    out = T.solve_configs(rows, pieces, L, M, w, W, DEV, best_value=True, bound=True, spare_weight=spare)
    solved, length, best = _np(out["solved"]), _np(out["solution_len"]), _np(out["best_value"])
    env = T.BatchedTetris(L, M, n, device=DEV, seed=1, auto_reset=False, assign="sequential", config_pool=(rows, pieces))
    env.reset()
    scores, plans = np.zeros((n, 12), np.float32), {}
    for j in range(1, 13):
        _, plans[j], scores[:, j - 1] = _beam(env, w, j, W, True, spare)
    env.terminate()
    run = np.where(solved, length, (plans[12] != 255).sum(axis=1))    # plies run: as test_solve_gpu counts them
    checked = 0
    for j in range(1, 13):
        at = run >= j
        assert np.array_equal(best[at, j - 1].view(np.uint32), scores[at, j - 1].view(np.uint32)), (F, j)
        checked += int(at.sum())
    assert checked >= 6 * n


@pytest.fixture(scope="module")
def tight_states():
    """64 mid-game and late-game states of a (10, 16) game: boards of a pool tightened to sixteen moves, played by the one-ply
    classical player for 3 .. 14 moves -- budgets at which many children are dead."""
    f = load_golden("carved_L10_M40.npz")
    L, M, n = 10, 16, 64
    rows, pieces = T.tighten_pool(f["rows"], f["pieces"], np.ones(256, bool), f["sol_len"], M)
    env = T.BatchedTetris(L, M, n, device=DEV, seed=4, auto_reset=False, config_pool=(rows, pieces))
    env.reset()
    player = T.BeamPolicy(env, T.CLASSICAL_WEIGHTS, 1, 1)
    seen = []
    for t in range(15):
        seen.append(tuple(_np(x).view(np.uint32).copy() for x in env.raw_planes()))
        env.step(player.act(), observe=False)
    pick = 3 + np.arange(n) % 12                               # moves 3 .. 14
    A = np.stack([seen[p][0][i] for i, p in enumerate(pick)])
    B = np.stack([seen[p][1][i] for i, p in enumerate(pick)])
    env.write_raw_planes(_i32(A).to(DEV), _i32(B).to(DEV))
    fields = R.decode_state(A, B)
    assert (fields["state"] == 0).sum() >= 40 and fields["moves"].max() >= 13
    yield env, fields
    env.terminate()


# every shape on all 64 states; the widest, where the host reference takes seconds, as two cases of 32 states each
@pytest.mark.parametrize("depth,width,first,count", [(1, 1, 0, 64), (2, 3, 0, 64), (3, 8, 0, 64), (6, 16, 0, 64), (12, 64, 0, 32),
                                                     (12, 64, 32, 32)])
@pytest.mark.parametrize("F", [12, 14])
def test_the_bounded_beam_is_the_reference_composed_ply_by_ply(tight_states, depth, width, first, count, F):
    env, all_fields = tight_states
    w = G.weights()[F]
    sub = np.arange(first, first + count)
    fields = {k: v[sub] for k, v in all_fields.items()}
    for spare in (0.25, 0.0) if depth <= 3 else (0.25,):       # both spare weights where the reference is quick
        want = reference_beam(fields, env.L, env.M, w, depth, width, True, spare)
        _same_beam(tuple(x[sub] for x in _beam(env, w, depth, width, True, spare)), want, (F, depth, width, spare))
        assert want["dead"].sum() >= 4                         # dead children among the candidates
    if (depth, width) == (3, 8):                               # the reference itself, on the unbounded kernel; and the bound changes the play
        plain = reference_beam(fields, env.L, env.M, w, depth, width, False, 0.0)
        _same_beam(_beam(env, w, depth, width, False, 0.0), plain, (F, depth, width, "unbounded"))
        assert (plain["action"] != want["action"]).any()


@pytest.mark.parametrize("depth,width", [(1, 1), (3, 8), (8, 4)])
def test_without_a_dead_child_and_at_spare_weight_zero_the_bounded_beam_is_the_unbounded_one(depth, width):
    f = load_golden("carved_L10_M40.npz")
    L, M, n = 10, 20, 128                                      # a budget that some boards can spare moves under and others cannot
    env, A, B = _snapshots(L, M, n, (f["rows"], f["pieces"][:, :M + 1]), 12, 6)
    env.write_raw_planes(_i32(A).to(DEV), _i32(B).to(DEV))
    fields = R.decode_state(A, B)
    for w in G.weights().values():
        ref = reference_beam(fields, L, M, w, depth, width, True, 0.0)
        got = _beam(env, w, depth, width, True, 0.0)
        _same_beam(got, ref, (depth, width, "bounded"))
        plain = _beam(env, w, depth, width, False, 0.0)
        clean = ~ref["dead"]
        assert clean.sum() >= 16 and (~clean).sum() >= 1
        # the same bytes, the score's among them: a twin's -0 would come out +0 in the bounded form (score + 0 * spare; include/
        # tpl_learn.h says so), but no score of these weight rows on these running states is a zero of either sign (a finished
        # board scores the zeros' +0 in both forms, by the twin's own code)
        assert (plain[2][clean & (fields["state"] == 0)] != 0).all()
        assert np.array_equal(got[0][clean], plain[0][clean]) and np.array_equal(got[1][clean], plain[1][clean])
        assert np.array_equal(got[2][clean].view(np.uint32), plain[2][clean].view(np.uint32))
    env.terminate()
