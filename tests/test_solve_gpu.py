"""The whole-game beam solver on one MI355X (include/tpl_learn.h's rule, tpl_placement_solve, solve_configs, tighten_pool,
ForwardGames(solver="beam")).

  1. KERNEL AGAINST MIRROR, bit for bit: solved, solution_len, actions and best_value of 64 carved + 64 synthetic configurations at
     (L, M) in {(1, 1), (2, 6), (3, 13), (5, 20)} and W in {1, 3, 16, 64}, through guard-framed buffers, and one configuration alone.
     The mirror's outputs are recorded (tests/golden/solve_mirror.npz: a width-64 case takes the mirror ten seconds and more;
     tests/test_solve_cpu.py pins the file to the mirror); the synthetic inputs are checked against env.synthetic_configs.
  2. THE LONGEST GAME: M = 254 at W = 64, solutions of 250 moves and games that are not solved, against the mirror and by replay.
  3. REPLAY on the environment: every solved board is won with moves_used == solution_len, also on the tightened pool's environment.
  4. THE PLACEMENT BEAM: best_value[:, j - 1] is BeamPolicy(depth=j, width=W)'s score on freshly reset boards, and where the beam's
     plan wins at the solver's ply it is the solution.
  5. the entry: optional output, guard words, refusals that leave the outputs alone, two runs, save_pool.
  6. ForwardGames(solver="beam") replays to wins; solver="reference" is what it was.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import load_golden
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ((1, 1), (2, 6), (3, 13), (5, 20))
WIDTHS = (1, 3, 16, 64)
NAMES = ("solved", "solution_len", "actions", "best_value")
WON = 1


@pytest.fixture(scope="module")
def golden_solve():
    return load_golden("solve_mirror.npz")


def _solve(rows, pieces, L, M, weights, width, skip_best=False):
    """tpl_placement_solve through guard-framed buffers, every output filled with 0xCD first."""
    n = rows.shape[0]
    rf, pf, wf = Framed(n * 40, 1), Framed(n * (M + 1), 2), Framed(48, 3)
    rf.inner().copy_(torch.from_numpy(np.ascontiguousarray(rows, np.uint16).view(np.uint8).reshape(-1)))
    pf.inner().copy_(torch.from_numpy(np.ascontiguousarray(pieces, np.uint8).reshape(-1)))
    wf.inner().copy_(torch.from_numpy(np.array(weights, np.float32).view(np.uint8)))
    out = dict(solved=Framed(n, 4), solution_len=Framed(4 * n, 5), actions=Framed(n * M, 6), best_value=Framed(4 * n * M, 7))
    for f in out.values():
        f.inner().fill_(0xCD)
    _check(_lib().tpl_placement_solve(rf.ptr(), pf.ptr(), n, L, M, wf.ptr(), width, out["solved"].ptr(), out["solution_len"].ptr(),
                                      out["actions"].ptr(), None if skip_best else out["best_value"].ptr(), _stream()))
    for name, f in list(out.items()) + [("rows", rf), ("pieces", pf), ("weights", wf)]:
        f.assert_canary((L, M, width, n, name))                # the guard words stay intact
    assert np.array_equal(rf.host().view(np.uint16).reshape(n, 20), rows) and np.array_equal(pf.host().reshape(n, M + 1), pieces)
    if skip_best:
        assert (out["best_value"].host() == 0xCD).all()        # an output that is not given is not written
    return (out["solved"].host().copy(), out["solution_len"].host().view(np.int32).copy(),
            out["actions"].host().reshape(n, M).copy(), out["best_value"].host().view(np.float32).reshape(n, M).copy())


def _same(got, want, what, names=NAMES):
    for name, g, w in zip(NAMES, got, want):
        if name not in names:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        g, w = (g.view(np.uint32), w.view(np.uint32)) if name == "best_value" else (g, w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _recorded(g, key, pick=slice(None)):
    return tuple(g[key + name][pick] for name in NAMES)


# ------------------------------------------------------------------------------------------------ 1. kernel against mirror
@pytest.mark.parametrize("L,M", CASES)
def test_the_kernel_is_the_mirror_bit_for_bit(golden_solve, L, M):
    g = golden_solve
    rows, pieces = g[f"L{L}_M{M}_rows"], g[f"L{L}_M{M}_pieces"]
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=7)
    s_rows, s_pieces = env.synthetic_configs(64, seed=7, first=0)    # the recorded synthetic half is the device generator's
    assert np.array_equal(_np(s_rows).view(np.uint16), rows[64:]) and np.array_equal(_np(s_pieces), pieces[64:])
    env.terminate()
    for W in WIDTHS:
        want = _recorded(g, f"L{L}_M{M}_W{W}_")
        _same(_solve(rows, pieces, L, M, T.CLASSICAL_WEIGHTS, W), want, (L, M, W))
        for i in (0, 127):                                     # one configuration alone: a grid of one workgroup
            _same(_solve(rows[i:i + 1], pieces[i:i + 1], L, M, T.CLASSICAL_WEIGHTS, W), tuple(x[i:i + 1] for x in want), (L, M, W, i))
    want = _recorded(g, f"L{L}_M{M}_W16_")
    _same(_solve(rows, pieces, L, M, T.CLASSICAL_WEIGHTS, 16, skip_best=True), want, (L, M, "no best_value"), names=NAMES[:3])
    _same(_solve(rows[5:70], pieces[5:70], L, M, T.CLASSICAL_WEIGHTS, 16), tuple(x[5:70] for x in want), (L, M, "an odd count"))


def test_the_recorded_cases_hold_both_verdicts_and_every_kind_of_ending(golden_solve):
    g = golden_solve
    solved = np.concatenate([g[f"L{L}_M{M}_W{W}_solved"] for L, M in CASES for W in WIDTHS])
    assert 100 <= (solved == 0).sum() and (solved == 1).sum() >= 1000
    assert g["L5_M20_W1_solution_len"].max() == 20 and g["L3_M13_W1_solution_len"].max() == 13      # a win at the last ply
    assert (g["L2_M6_W1_solved"][:64] == 0).any()              # a carved configuration that width 1 misses and width 3 finds
    assert g["L2_M6_W3_solved"][:64].all()


# ------------------------------------------------------------------------------------------------ 2. the longest game
def _replay(rows, pieces, L, M, actions):
    """Configuration i on board i of a non-auto-reset environment (sequential assignment, as many boards as configurations), the
    actions played column by column, finished boards frozen; returns (state, moves) of every board."""
    n = rows.shape[0]
    env = T.BatchedTetris(L, M, n, device=DEV, seed=1, auto_reset=False, assign="sequential", config_pool=(rows, pieces))
    env.reset()
    acts = torch.as_tensor(actions).to(DEV)
    acts = torch.where(acts == 255, torch.zeros_like(acts), acts).contiguous()
    last = int((torch.as_tensor(actions) != 255).sum(dim=1).max())
    for j in range(last):
        env.step(acts[:, j].contiguous())
    state = {k: _np(v) for k, v in env.packed_state().items()}
    env.terminate()
    return state["state"].astype(np.int64), state["moves"].astype(np.int64)


def test_games_of_254_moves_are_the_mirrors_and_their_solutions_win(golden_solve):
    g = golden_solve
    rows, pieces = g["long_rows"], g["long_pieces"]
    assert pieces.shape == (4, 255)
    got = _solve(rows, pieces, 105, 254, T.CLASSICAL_WEIGHTS, 64)
    _same(got, _recorded(g, "long_L105_"), "long 105")
    assert got[0].all() and got[1].min() >= 240                # the tape is walked back over some 250 plies
    state, moves = _replay(rows, pieces, 105, 254, got[2])
    assert (state == WON).all() and np.array_equal(moves, got[1])
    got = _solve(rows, pieces, 112, 254, T.CLASSICAL_WEIGHTS, 64)          # not reached: the search runs to the move limit
    _same(got, _recorded(g, "long_L112_"), "long 112")
    assert not got[0].any() and (got[3][:, -1] != 0).any() and (got[2] == 255).all()


# ------------------------------------------------------------------------------------------------ 3. replay
@pytest.mark.parametrize("L,M,W", [(2, 6, 1), (3, 13, 3), (5, 20, 16)])
def test_solutions_replay_to_wins_on_the_environment_and_on_the_tightened_pool(golden_solve, L, M, W):
    g = golden_solve
    rows, pieces = g[f"L{L}_M{M}_rows"], g[f"L{L}_M{M}_pieces"]
    out = T.solve_configs(rows, pieces[:, :M] if W == 3 else pieces, L, M, width=W, device=DEV, best_value=True)
    if W != 3:                                                 # (with the last piece cut off and padded the result is the same)
        assert set(out) == {"solved", "solution_len", "actions", "solution", "best_value"}
    assert out["solved"].dtype == torch.bool and out["solution_len"].dtype == torch.int32 and out["actions"].dtype == torch.uint8
    assert tuple(out["solution"].shape) == (128, M, 2) and out["solution"].dtype == torch.uint8
    got = (_np(out["solved"]).astype(np.uint8), _np(out["solution_len"]), _np(out["actions"]), _np(out["best_value"]))
    _same(got, _recorded(g, f"L{L}_M{M}_W{W}_"), (L, M, W, "solve_configs"))
    solved, length, actions = got[0].astype(bool), got[1], got[2]
    sol = _np(out["solution"]).astype(np.int64)
    played = actions != 255
    assert np.array_equal((10 * sol[..., 0] + sol[..., 1])[played], actions[played]) and (sol[~played] == 0).all()
    state, moves = _replay(rows, pieces, L, M, actions)
    assert (state[solved] == WON).all() and np.array_equal(moves[solved], length[solved]) and solved.sum() >= 64
    # a pool with a tighter budget: the median solution length
    M_new = int(np.median(length[solved]))
    t_rows, t_pieces = T.tighten_pool(torch.as_tensor(rows.view(np.int16)).to(DEV), torch.as_tensor(pieces).to(DEV), out["solved"],
                                      out["solution_len"], M_new)
    keep = solved & (length <= M_new)
    assert 1 <= keep.sum() < solved.sum() or M_new == M
    assert np.array_equal(_np(t_rows).view(np.uint16), rows[keep]) and np.array_equal(_np(t_pieces), pieces[keep][:, :M_new + 1])
    state, moves = _replay(_np(t_rows).view(np.uint16), _np(t_pieces), L, M_new, actions[keep][:, :M_new])
    assert (state == WON).all() and np.array_equal(moves, length[keep])


# ------------------------------------------------------------------------------------------------ 4. the placement beam
@pytest.mark.parametrize("W", [3, 16])
def test_best_value_is_the_placement_beams_score_and_a_winning_plan_is_the_solution(golden_solve, W):
    g = golden_solve
    L, M = 5, 20
    rows, pieces = g[f"L{L}_M{M}_rows"], g[f"L{L}_M{M}_pieces"]
    n = rows.shape[0]
    solved, length, actions, best = _recorded(g, f"L{L}_M{M}_W{W}_")
    solved = solved.astype(bool)
    env = T.BatchedTetris(L, M, n, device=DEV, seed=1, auto_reset=False, assign="sequential", config_pool=(rows, pieces))
    env.reset()
    score, plan = torch.empty(n, dtype=torch.float32, device=DEV), {}
    scores = np.zeros((n, 12), np.float32)
    for j in range(1, 13):
        plan[j] = torch.empty((n, j), dtype=torch.uint8, device=DEV)
        T.BeamPolicy(env, T.CLASSICAL_WEIGHTS, depth=j, width=W).act(score=score, plan=plan[j])
        scores[:, j - 1] = _np(score)
        plan[j] = _np(plan[j])
    # plies run: the winning ply of a solved configuration; of an unsolved one at least the moves of the deepest plan's best node
    run = np.where(solved, length, (plan[12] != 255).sum(axis=1))
    assert (run >= 1).all() and (run[~solved] >= 1).all()
    checked = 0
    for j in range(1, 13):
        at = run >= j
        assert np.array_equal(best[at, j - 1].view(np.uint32), scores[at, j - 1].view(np.uint32)), (W, j)
        checked += int(at.sum())
    assert checked >= 6 * n
    # where the plan of depth j = the winning ply wins when it is played, the first candidate was itself won: it is the solution
    same = 0
    for j in sorted(set(length[solved & (length <= 12)].tolist())):
        env.reset()
        acts = torch.as_tensor(np.where(plan[j] == 255, 0, plan[j])).to(DEV)
        for t in range(j):
            env.step(acts[:, t].contiguous())
        state = _np(env.packed_state()["state"])
        at = solved & (length == j) & (state == WON)
        assert np.array_equal(plan[j][at], actions[at, :j]), (W, j)
        same += int(at.sum())
    assert same >= (solved & (length <= 12)).sum() // 2
    env.terminate()


# ------------------------------------------------------------------------------------------------ 5. the entry
def test_refusals_leave_the_outputs_alone_and_two_runs_give_the_same_bytes(golden_solve, tmp_path):
    g = golden_solve
    L, M = 3, 13
    rows, pieces = g[f"L{L}_M{M}_rows"][:66], g[f"L{L}_M{M}_pieces"][:66]
    n = 66
    lib, name = _lib(), b"tpl_placement_solve"
    r = torch.from_numpy(rows.view(np.int16).copy()).to(DEV)
    p = torch.from_numpy(pieces.copy()).to(DEV)
    w = torch.from_numpy(T.CLASSICAL_WEIGHTS.copy()).to(DEV)
    outs = [torch.full((n,), 0xCD, dtype=torch.uint8, device=DEV), torch.full((4 * n,), 0xCD, dtype=torch.uint8, device=DEV),
            torch.full((n * M,), 0xCD, dtype=torch.uint8, device=DEV), torch.full((4 * n * M,), 0xCD, dtype=torch.uint8, device=DEV)]

    def solve(rows=r.data_ptr(), pieces=p.data_ptr(), n=n, L=L, M=M, weights=w.data_ptr(), width=4, solved=outs[0].data_ptr(),
              length=outs[1].data_ptr(), actions=outs[2].data_ptr(), best=outs[3].data_ptr()):
        return lib.tpl_placement_solve(rows, pieces, n, L, M, weights, width, solved, length, actions, best, _stream())

    refused = [dict(n=0), dict(n=-1), dict(n=1 << 31), dict(rows=None), dict(pieces=None), dict(weights=None), dict(solved=None),
               dict(length=None), dict(actions=None), dict(weights=w.data_ptr() + 4), dict(length=outs[1].data_ptr() + 2),
               dict(best=outs[3].data_ptr() + 2), dict(rows=r.data_ptr() + 1), dict(L=0), dict(L=251), dict(M=0), dict(M=255),
               dict(width=0), dict(width=65)]
    for bad in refused:
        assert solve(**bad) < 0 and name in lib.tpl_learn_last_error(), bad
    torch.cuda.synchronize()
    assert all(bool((o == 0xCD).all()) for o in outs)          # refused before any launch: nothing was written
    first = T.solve_configs(rows, pieces, L, M, width=16, device=DEV, best_value=True)
    first = {k: _np(v).copy() for k, v in first.items()}
    again = T.solve_configs(r, p, L, M, T.CLASSICAL_WEIGHTS, 16, DEV, True, validate=False)
    for k, v in again.items():
        assert np.array_equal(_np(v).view(np.uint8), first[k].view(np.uint8)), k
    cells = ((rows[:, :, None] >> np.arange(10)) & 1).astype(bool)                # the [n, 20, 10] form of the boards
    for k, v in T.solve_configs(cells, pieces, L, M, width=16, device=DEV, best_value=True).items():
        assert np.array_equal(_np(v).view(np.uint8), first[k].view(np.uint8)), k
    with pytest.raises(ValueError, match="piece ids"):
        T.solve_configs(rows, np.where(pieces == 0, 7, pieces), L, M, device=DEV)
    # save_pool takes the solver's outputs as they are
    path = str(tmp_path / "solved.npz")
    T.save_pool(path, L, M, rows, pieces, solution=again["solution"].cpu(), solution_len=again["solution_len"].cpu())
    back = T.load_pool(path)
    assert np.array_equal(back["solution"], first["solution"]) and np.array_equal(back["solution_len"], first["solution_len"])
    assert back["solution"].dtype == np.uint8 and back["solution_len"].dtype == np.int32 and (back["L"], back["M"]) == (L, M)


# ------------------------------------------------------------------------------------------------ 6. the forward supply
def test_forward_games_kept_by_the_beam_replay_to_wins_and_the_reference_solver_is_as_it_was():
    L, M = 5, 20
    env = T.BatchedTetris(L, M, 8, device=DEV, seed=2)
    plain, named = T.ForwardGames(env, range(64)), T.ForwardGames(env, range(64), solver="reference")
    assert plain.solver == "reference" and (plain.tried, plain.count) == (named.tried, named.count)
    for key in ("rows", "sequence", "solution", "solution_len"):
        assert torch.equal(getattr(plain, key), getattr(named, key)), key
    beam = T.ForwardGames(env, range(64), solver="beam")
    wide = T.ForwardGames(env, range(64), solver="beam", weights=T.CLASSICAL_WEIGHTS, width=64)
    assert beam.solver == "beam" and beam.tried == 64 and 1 <= beam.count <= wide.tried == 64
    for games in (beam, wide):
        rows, pieces = games.translate(lead=False)             # the solution fits the untranslated sequence
        assert tuple(pieces.shape) == (games.count, M + 1)
        sol = _np(games.solution).astype(np.int64)
        length = _np(games.solution_len)
        actions = 10 * sol[..., 0] + sol[..., 1]
        actions[np.arange(M)[None, :] >= length[:, None]] = 255
        assert (length >= 1).all() and (actions[np.arange(M)[None, :] < length[:, None]] < 40).all()
        state, moves = _replay(_np(rows).view(np.uint16), _np(pieces), L, M, actions.astype(np.uint8))
        assert (state == WON).all() and np.array_equal(moves, length)
    env.terminate()
