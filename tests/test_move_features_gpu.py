"""The 14-feature form of the linear placement family on one MI355X (include/tpl_learn.h: features 12 landing_height and 13
eroded_cells; tpl_placement_features_move, _act_move, _search_move, _beam_move, _solve_move), every entry through canary-framed
buffers against the numpy mirror (_learn_lib.host_moves_traced, placement_score, search_choice, beam_select, placement_solve):

  FEATURES  4,096 states spread over games of random play plus the CPU file's edge boards, at (L, M) = (10, 40) and (1, 1): all 14
            columns are the mirror's, entries 14..15 zero, columns 0..11 and canonical tpl_placement_features' on the same states.
  ACT / SEARCH  a population of three weight rows with a short last member, one row non-zero only in 12 and 13: action, second
            and score are the mirror's bit for bit, act at up to 4,101 states, search at up to 2,048 against the recorded mirror;
            with w12 = w13 = 0 actions and seconds are the 12-feature kernels'.
  BEAM      (D, W) in {(1, 1), (2, 34), (3, 8), (12, 64)} on 64 boards against a ply-by-ply reference composed from T.afterstates,
            the mirror's move features and beam_select; depth 1 is the 14-form act, depth 2 at width 34 the 14-form search; the
            plan played move by move on the environment reaches a board whose psi, summed along the way, scores `score`.
  SOLVE     (L, M) in {(1, 1), (2, 6), (3, 13), (5, 20)} x W in {1, 3, 16, 64} against placement_solve in the 14 form; solutions
            replay to wins on the environment; best_value is the 14-form beam's score; games of M = 254, one whose landing sum
            passes 2^13; two runs, equal bytes.
  PYTHON    evaluate_heuristic and two generations of tune_heuristic(features=14) on a tiny pool; a captured graph of act().
"""
import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from conftest import load_golden
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_move_features_cpu import (EDGE_BOARDS, SEARCH_L, SEARCH_M, SEARCH_N, MirrorStates, _cells_to_rows, mirror_search,
                                    population as _population)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARANGE = np.arange(40)
CLASSICAL = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
W14 = np.concatenate([CLASSICAL, np.array([-0.25, 0.5], np.float32)])


def _m():
    return T._learn_lib


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32))


def _framed(array, seed):
    raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    f = Framed(raw.size, seed)
    f.inner().copy_(torch.from_numpy(raw))
    return f


def _planes(A, B):
    return _framed(A, 1), _framed(B, 2)


def _weights(w, stride):
    """Weight rows [P, 12] as they are, [P, 14] in rows of 16 with NaN in entries 14 and 15: they are never read."""
    w = np.ascontiguousarray(w, np.float32).reshape(-1, w.shape[-1])
    if stride == 16:
        w = np.concatenate([w, np.full((w.shape[0], 2), np.nan, np.float32)], axis=1)
    return _framed(w, 5), w


# ------------------------------------------------------------------------------------------------ the states and the mirror
def _played_states(L, M, boards, snapshots, every, seed):
    """`boards` x `snapshots` states of a non-auto-reset environment under random play, a snapshot every `every` steps."""
    env = T.BatchedTetris(L, M, boards, device=DEV, seed=seed, auto_reset=False)
    rows, pieces = env.synthetic_configs(64)
    env.load_configs(rows, pieces)
    env.reset()
    A, B = [], []
    for t in range(snapshots * every):
        if t % every == 0:
            a, b = env.raw_planes()
            A.append(_np(a).view(np.uint32)), B.append(_np(b).view(np.uint32))
        env.step(env.synthetic_actions(t))
    env.terminate()
    return np.concatenate(A), np.concatenate(B)


def _edge_states(L, M):
    rows = _cells_to_rows(np.stack(list(EDGE_BOARDS.values())))
    k = rows.shape[0]
    window = np.array([(p + 8 * ((p + 3) % 7)) for p in range(7)], np.uint64)             # every piece current, another next
    rows = np.repeat(rows, 7, axis=0)                          # each board under each of the seven pieces
    window = np.tile(window, k)
    lines = np.where(np.arange(rows.shape[0]) % 3 == 0, max(L - 1, 0), 0)
    moves = np.where(np.arange(rows.shape[0]) % 5 == 0, M - 1, 0)
    return R.pack_state(rows, lines, moves, 0, 0, window)


class States(MirrorStates):
    """The played states and the edge boards of a game (L, M), with the mirror's phi14."""

    def __init__(self, L, M):
        boards, snapshots, every = (512, 8, 3) if M > 1 else (2048, 2, 1)
        A, B = _played_states(L, M, boards, snapshots, every, 11)
        eA, eB = _edge_states(L, M)
        super().__init__(np.concatenate([eA, A]), np.concatenate([eB, B]), L, M)


@pytest.fixture(scope="module", params=[(10, 40), (1, 1)], ids=["L10_M40", "L1_M1"])
def states(request):
    return States(*request.param)


def _features(a, b, n, L, M, move, with_canonical=True):
    width = 16 if move else 12
    feats, canon = Framed(n * 40 * width * 2, 3), Framed(n * 40, 4)
    feats.inner().fill_(0xCD), canon.inner().fill_(0xCD)
    entry = _lib().tpl_placement_features_move if move else _lib().tpl_placement_features
    _check(entry(a.ptr(), b.ptr(), n, L, M, feats.ptr(), canon.ptr() if with_canonical else None, _stream()))
    for name, f in (("features", feats), ("canonical", canon), ("a", a), ("b", b)):
        f.assert_canary((n, move, name))
    if not with_canonical:
        assert (canon.host() == 0xCD).all()
    return feats.host().view(np.int16).reshape(n, 40, width).astype(np.int64), canon.host().reshape(n, 40).copy()


def test_features_all_14_columns_are_the_mirrors(states):
    s = states
    assert s.n >= 4096 + 8 and s.running.sum() > s.n // 4 and ((~s.running).sum() > 100 or s.M == 40)
    a, b = _planes(s.A, s.B)
    got, canon = _features(a, b, s.n, s.L, s.M, True)
    assert (got[:, :, 14:] == 0).all()
    bad = np.argwhere(got[:, :, :14] != s.phi)
    assert bad.size == 0, (bad[:5].tolist(), got[tuple(bad[0][:2])], s.phi[tuple(bad[0][:2])])
    twin, canon12 = _features(a, b, s.n, s.L, s.M, False)
    assert np.array_equal(got[:, :, :12], twin) and np.array_equal(canon, canon12) and np.array_equal(canon, s.canonical)
    _features(a, b, 13, s.L, s.M, True, with_canonical=False)
    assert np.array_equal(a.host(), s.A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), s.B.view(np.uint8).reshape(-1))
    if s.M == 40:                                              # the two features take many values on these states
        live = s.phi[s.running]
        assert np.unique(live[:, :, 12]).size >= 30 and {0, 2, 9, 16} <= set(np.unique(live[:, :, 13]).tolist())
        assert (s.left["state"][s.running] == 3).any()         # top-outs among them
    # the Python surface
    env = T.BatchedTetris(s.L, s.M, 8, device=DEV, seed=3)
    f14, c14 = T.placement_features(env, _i32(s.A[:300]).to(DEV), _i32(s.B[:300]).to(DEV), move=True)
    f12, c12 = T.placement_features(env, _i32(s.A[:300]).to(DEV), _i32(s.B[:300]).to(DEV))
    assert f14.shape == (300, 40, 14) and f14.dtype == torch.int16 and f12.shape == (300, 40, 12)
    assert np.array_equal(_np(f14), s.phi[:300]) and torch.equal(f14[:, :, :12], f12) and torch.equal(c14, c12)
    env.terminate()


# ------------------------------------------------------------------------------------------------ act and search
def _policy(a, b, n, L, M, w, per, plies, move, skip=None):
    wf, rows = _weights(w, 16 if move else 12)
    action, second, score = Framed(n, 6), Framed(n, 7), Framed(n * 4, 8)
    for f in (action, second, score):
        f.inner().fill_(0xCD)
    name = "tpl_placement_" + ("search" if plies == 2 else "act") + ("_move" if move else "")
    extra = (second.ptr(),) if plies == 2 else ()
    _check(getattr(_lib(), name)(a.ptr(), b.ptr(), n, L, M, wf.ptr(), per, action.ptr(), *extra, None if skip == "score" else score.ptr(),
                                 _stream()))
    for what, f in (("action", action), ("second", second), ("score", score), ("weights", wf), ("a", a), ("b", b)):
        f.assert_canary((name, n, per, what))
    assert np.array_equal(wf.host(), rows.view(np.uint8).reshape(-1))
    if skip == "score":
        assert (score.host() == 0xCD).all()
    return action.host().copy(), second.host().copy(), score.host().view(np.float32).copy()


def _lowest_at_max(score, mask):
    masked = np.where(mask, score, -np.inf)
    return np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)


@pytest.mark.parametrize("n", [1, 13, 4101])
def test_act_is_the_mirrors_arg_max_bit_for_bit(states, n):
    s, m = states, _m()
    idx = (np.arange(n) * 7 + 3) % s.n if n < s.n else np.arange(n) % s.n
    a, b = _planes(s.A[idx], s.B[idx])
    w, per = _population(n)
    rows = w[np.arange(n) // per]
    score = m.placement_score(s.phi[idx], rows[:, None, :])
    want = _lowest_at_max(score, s.distinct[idx])
    want_score = score[np.arange(n), want]
    want = np.where(s.running[idx], want, 0)
    got = _policy(a, b, n, s.L, s.M, w, per, 1, True)
    assert np.array_equal(got[0], want.astype(np.uint8))
    assert np.array_equal(got[2].view(np.uint32), want_score.astype(np.float32).view(np.uint32))
    assert np.array_equal(_policy(a, b, n, s.L, s.M, w, per, 1, True, skip="score")[0], got[0])
    # with w12 = w13 = 0 the 12-feature kernel's actions
    zero = w.copy()
    zero[:, 12:] = 0
    assert np.array_equal(_policy(a, b, n, s.L, s.M, zero, per, 1, True)[0], _policy(a, b, n, s.L, s.M, zero[:, :12], per, 1, False)[0])
    if n > 4000 and s.M == 40:
        assert (got[0] != _policy(a, b, n, s.L, s.M, w[:, :12], per, 1, False)[0]).any()        # the two features move choices


@pytest.mark.parametrize("n", [1, 13, 101])
def test_search_is_the_mirrors_two_ply_choice_bit_for_bit(states, n):
    s = states
    idx = (np.arange(n) * 5 + 1) % s.n
    a, b = _planes(s.A[idx], s.B[idx])
    w, per = _population(n)
    want = mirror_search(s, idx, w[np.arange(n) // per])               # live: a hundred states is what a test may spend on the mirror
    got = _policy(a, b, n, s.L, s.M, w, per, 2, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].astype(np.float32).view(np.uint32))
    zero = w.copy()
    zero[:, 12:] = 0
    g14, g12 = _policy(a, b, n, s.L, s.M, zero, per, 2, True), _policy(a, b, n, s.L, s.M, zero[:, :12], per, 2, False)
    assert np.array_equal(g14[0], g12[0]) and np.array_equal(g14[1], g12[1])


def test_search_on_2048_states_is_the_recorded_mirror_bit_for_bit():
    """The two-ply kernel under non-zero move weights at a few thousand boards, a count that is no multiple of 8 among them: the
    mirror's choices of tests/golden/move_search_mirror.npz (a minute of numpy, recorded; the CPU tests pin the file to the mirror)."""
    g = load_golden("move_search_mirror.npz")
    w, per = g["weights"], int(g["per"])
    assert g["A"].shape == (SEARCH_N, 4) and w.shape == (3, 14) and 2 * per < SEARCH_N < 3 * per
    a, b = _planes(g["A"], g["B"])
    got = _policy(a, b, SEARCH_N, SEARCH_L, SEARCH_M, w, per, 2, True)
    for name, x, y in (("action", got[0], g["action"]), ("second", got[1], g["second"]),
                       ("score", got[2].view(np.uint32), g["score"].view(np.uint32))):
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, bad[:5].tolist(), x[bad[:5]].tolist(), y[bad[:5]].tolist())
    n = 2 * per + 5                                            # 1,373: the last member short, the last block of eight boards too
    assert n % 8 != 0
    a, b = _planes(g["A"][:n], g["B"][:n])
    part = _policy(a, b, n, SEARCH_L, SEARCH_M, w, per, 2, True)
    assert np.array_equal(part[0], g["action"][:n]) and np.array_equal(part[1], g["second"][:n])
    assert np.array_equal(part[2].view(np.uint32), g["score"][:n].view(np.uint32))


def test_search_with_zero_move_weights_is_the_12_feature_kernel_on_every_state(states):
    s = states
    a, b = _planes(s.A, s.B)
    zero = np.concatenate([CLASSICAL, np.zeros(2, np.float32)])[None]
    g14, g12 = _policy(a, b, s.n, s.L, s.M, zero, s.n, 2, True), _policy(a, b, s.n, s.L, s.M, CLASSICAL[None], s.n, 2, False)
    assert np.array_equal(g14[0], g12[0]) and np.array_equal(g14[1], g12[1]) and np.array_equal(g14[2], g12[2])


# ------------------------------------------------------------------------------------------------ the beam
BL, BM, BN = 10, 40, 64


def _beam(a, b, n, w, per, depth, width, L=BL, M=BM):
    wf, rows = _weights(w, 16)
    action, plan, score = Framed(n, 6), Framed(n * depth, 7), Framed(n * 4, 8)
    for f in (action, plan, score):
        f.inner().fill_(0xCD)
    _check(_lib().tpl_placement_beam_move(a.ptr(), b.ptr(), n, L, M, wf.ptr(), per, depth, width, action.ptr(), plan.ptr(), score.ptr(),
                                          _stream()))
    for what, f in (("action", action), ("plan", plan), ("score", score), ("weights", wf), ("a", a), ("b", b)):
        f.assert_canary((n, depth, width, what))
    return action.host().copy(), plan.host().reshape(n, depth).copy(), score.host().view(np.float32).copy()


@pytest.fixture(scope="module")
def beam_boards():
    """64 boards of a played game: moves 0, 3, 8 and 9 among them (windows of 12, 9, 4 and 3 known pieces), finished ones too."""
    parts = [_played_states(BL, BM, 16, 1, 1, 21)]
    env = T.BatchedTetris(BL, BM, 16, device=DEV, seed=22, auto_reset=False)
    rows, pieces = env.synthetic_configs(16)
    env.load_configs(rows, pieces)
    env.reset()
    for t in range(30):
        env.step(env.synthetic_actions(t))
        if t + 1 in (3, 8, 9):
            x, y = env.raw_planes()
            parts.append((_np(x).view(np.uint32), _np(y).view(np.uint32)))
    env.terminate()
    A, B = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert A.shape[0] == BN
    return A, B


def compose14(env, A, B, w, depth, width):
    """The beam rule with every ply's boards made by T.afterstates, features 0..11 by the 12-feature kernel on them, the move
    features by the mirror (host_moves_traced on the decoded nodes), the sums carried, placement_score and beam_select; w [14]."""
    m = _m()
    n = A.shape[0]
    root = R.decode_state(A, B)
    plies = np.where(root["state"] == 0, np.minimum(depth, 12 - root["moves"].astype(np.int64) % 10), 0)
    action, plan, score = np.zeros(n, np.uint8), np.full((n, depth), 255, np.uint8), np.zeros(n, np.float32)
    for i in range(n):
        na, nb = A[i:i + 1].copy(), B[i:i + 1].copy()
        sums, path = np.zeros((1, 3), np.int64), np.full((1, depth), 255, np.uint8)
        value = np.array([m.placement_score(np.zeros(14, np.int64), w)], np.float32)               # a finished root: fourteen zeros
        for j in range(int(plies[i])):
            q_count = na.shape[0]
            f = R.decode_state(na, nb)
            run = f["state"] == 0
            after = T.afterstates(env, _i32(na).to(DEV), _i32(nb).to(DEV))
            phi12, canonical = T.placement_features(env, _i32(na).to(DEV), _i32(nb).to(DEV))
            sa, sb = (_np(after[key]).view(np.uint32).reshape(q_count, 40, 4) for key in ("states_a", "states_b"))
            distinct = _np(canonical).reshape(q_count, 40) == ARANGE
            at, a = np.repeat(np.arange(q_count), 40), np.tile(ARANGE, q_count)
            out = m.host_moves_traced(f["rows"][at], f["cur"][at].astype(np.int64), a // 10, a % 10, BL, BM,
                                      f["lines"][at].astype(np.int64), f["moves"][at].astype(np.int64))
            psi = np.concatenate([_np(phi12).astype(np.int64).reshape(q_count, 40, 12),
                                  np.stack([out[7], out[8]], axis=1).reshape(q_count, 40, 2)], axis=2)
            assert np.array_equal(psi[run][:, :, 0], out[1].reshape(q_count, 40)[run])
            psi[:, :, [0, 12, 13]] += sums[:, None, :]
            cand_value = np.where(run[:, None], m.placement_score(psi, w), value[:, None]).astype(np.float32)
            cand = np.where(run[:, None], distinct, ARANGE[None, :] == 0)
            flat = np.flatnonzero(cand.reshape(-1))            # node by node, ascending placement: the candidates' order
            keep = flat[m.beam_select(cand_value.reshape(-1)[flat], width)]
            q, b = keep // 40, keep % 40
            moved = run[q]
            new_path = path[q].copy()
            new_path[moved, j] = b[moved]
            na, nb = sa[q, b].copy(), sb[q, b].copy()          # a finished board's afterstate is itself
            sums = np.where(moved[:, None], psi[q, b][:, [0, 12, 13]], sums[q])
            value, path = cand_value[q, b], new_path
        best = int(m.beam_select(value, 1)[0])
        score[i] = value[best]
        if plies[i] > 0:
            action[i], plan[i] = path[best, 0], path[best]
    return action, plan, score, plies


@pytest.mark.parametrize("depth,width", [(1, 1), (2, 34), (3, 8), (12, 64)])
def test_the_beam_is_the_reference_composed_ply_by_ply(beam_boards, depth, width):
    A, B = beam_boards
    env = T.BatchedTetris(BL, BM, 8, device=DEV, seed=9)
    a, b = _planes(A, B)
    got = _beam(a, b, BN, W14[None], BN, depth, width)
    want = compose14(env, A, B, W14, depth, width)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert want[3].min() == 0 and want[3].max() == min(depth, 12) and (depth < 12 or {3, 4, 9, 12} <= set(want[3].tolist()))
    if depth == 1:
        act = _policy(a, b, BN, BL, BM, W14[None], BN, 1, True)
        assert np.array_equal(got[0], act[0]) and np.array_equal(got[2].view(np.uint32), act[2].view(np.uint32))
    if (depth, width) == (2, 34):
        sea = _policy(a, b, BN, BL, BM, W14[None], BN, 2, True)
        assert np.array_equal(got[0], sea[0]) and np.array_equal(got[1][:, 1], sea[1])
        assert np.array_equal(got[2].view(np.uint32), sea[2].view(np.uint32))
    env.terminate()


@pytest.mark.parametrize("depth,width", [(3, 8), (12, 64)])
def test_the_plan_played_on_the_environment_scores_score(beam_boards, depth, width):
    m = _m()
    A, B = beam_boards
    env = T.BatchedTetris(BL, BM, BN, device=DEV, seed=9, auto_reset=False)
    env.write_raw_planes(_i32(A), _i32(B))
    policy = T.BeamPolicy(env, W14, depth, width)
    score = torch.empty(BN, dtype=torch.float32, device=DEV)
    plan = torch.empty((BN, depth), dtype=torch.uint8, device=DEV)
    action = policy.act(score=score, plan=plan)
    plan, score = _np(plan), _np(score)
    assert np.array_equal(_np(action), np.where(plan[:, 0] == 255, 0, plan[:, 0]))
    length = (plan != 255).sum(axis=1)
    sums = np.zeros((BN, 3), np.int64)
    final = [None] * BN
    f = R.decode_state(A, B)
    for i in np.flatnonzero(length == 0):
        final[i] = None                                        # a finished root: fourteen zeros
    for j in range(int(length.max())):
        live = length > j
        at = np.flatnonzero(live)
        b = plan[at, j].astype(np.int64)
        out = m.host_moves_traced(f["rows"][at], f["cur"][at].astype(np.int64), b // 10, b % 10, BL, BM, f["lines"][at].astype(np.int64),
                                  f["moves"][at].astype(np.int64))
        sums[at] += np.stack([out[1], out[7], out[8]], axis=1)
        env.step(torch.as_tensor(np.where(live, plan[:, min(j, depth - 1)], 0).astype(np.uint8)).to(DEV))
        x, y = env.raw_planes()
        f = R.decode_state(_np(x).view(np.uint32), _np(y).view(np.uint32))
        assert np.array_equal(f["rows"][at], out[0]) and np.array_equal(f["state"][at], out[4])      # the environment made the mirror's move
        for i in at[length[at] == j + 1]:
            final[i] = (f["rows"][i].copy(), int(f["state"][i]))
    for i in range(BN):
        if final[i] is None:
            psi = np.zeros(14, np.int64)
        else:
            rows, state = final[i]
            psi = np.concatenate([[sums[i, 0], state == 1, state >= 2], m.board_features(rows)[0], sums[i, 1:]]).astype(np.int64)
        want = m.placement_score(psi, W14)
        assert np.float32(want).view(np.uint32) == score[i].view(np.uint32), (i, plan[i].tolist(), want, score[i])
    env.terminate()


# ------------------------------------------------------------------------------------------------ the solver
def _solve(rows, pieces, L, M, w, width, move=True, with_best=True):
    n = rows.shape[0]
    rf, pf = _framed(rows, 1), _framed(pieces, 2)
    wf, wrows = _weights(np.asarray(w, np.float32)[None], 16 if move else 12)
    solved, length, actions, best = Framed(n, 6), Framed(n * 4, 7), Framed(n * M, 8), Framed(n * M * 4, 9)
    for f in (solved, length, actions, best):
        f.inner().fill_(0xCD)
    entry = _lib().tpl_placement_solve_move if move else _lib().tpl_placement_solve
    _check(entry(rf.ptr(), pf.ptr(), n, L, M, wf.ptr(), width, solved.ptr(), length.ptr(), actions.ptr(), best.ptr() if with_best else None,
                 _stream()))
    for what, f in (("rows", rf), ("pieces", pf), ("weights", wf), ("solved", solved), ("length", length), ("actions", actions),
                    ("best", best)):
        f.assert_canary((L, M, width, what))
    if not with_best:
        assert (best.host() == 0xCD).all()
    return (solved.host().copy(), length.host().view(np.int32).copy(), actions.host().reshape(n, M).copy(),
            best.host().view(np.float32).reshape(n, M).copy())


def _same_solution(got, want, what):
    for name, g, x in zip(("solved", "length", "actions", "best_value"), got, want):
        g, x = (g.view(np.uint32), np.asarray(x, np.float32).view(np.uint32)) if name == "best_value" else (g, x)
        bad = np.argwhere(g != x)
        assert bad.size == 0, (what, name, bad[:5].tolist())


def _replay(rows, pieces, L, M, actions):
    n = rows.shape[0]
    env = T.BatchedTetris(L, M, n, device=DEV, seed=1, auto_reset=False, assign="sequential", config_pool=(rows, pieces))
    env.reset()
    acts = torch.as_tensor(np.where(actions == 255, 0, actions)).to(DEV)
    for j in range(int((actions != 255).sum(axis=1).max(initial=0))):
        env.step(acts[:, j].contiguous())
    state = {k: _np(v) for k, v in env.packed_state().items()}
    env.terminate()
    return state["state"].astype(np.int64), state["moves"].astype(np.int64)


SOLVE_N = 12


@pytest.mark.parametrize("width", [1, 3, 16, 64])
@pytest.mark.parametrize("L,M", [(1, 1), (2, 6), (3, 13), (5, 20)])
def test_the_solver_is_the_mirror_and_its_solutions_win(L, M, width):
    g = load_golden("solve_mirror.npz")
    rows, pieces = g[f"L{L}_M{M}_rows"][:SOLVE_N], g[f"L{L}_M{M}_pieces"][:SOLVE_N]
    want = _m().placement_solve(rows, pieces, L, M, W14, width)
    got = _solve(rows, pieces, L, M, W14, width)
    _same_solution(got, want, (L, M, width))
    again = _solve(rows, pieces, L, M, W14, width)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, again))          # two runs, equal bytes
    _same_solution(_solve(rows, pieces, L, M, W14, width, with_best=False)[:3], want[:3], "no best_value")
    solved = got[0].astype(bool)
    print(f"L={L} M={M} W={width}: {int(solved.sum())} of {SOLVE_N} solved, lengths {got[1][solved].tolist()}")
    state, moves = _replay(rows, pieces, L, M, got[2])
    assert (state[solved] == 1).all() and np.array_equal(moves[solved], got[1][solved])
    # the 12 form with w12 = w13 = 0
    zero = np.concatenate([CLASSICAL, np.zeros(2, np.float32)])
    _same_solution(_solve(rows, pieces, L, M, zero, width)[:3], _solve(rows, pieces, L, M, CLASSICAL, width, move=False)[:3], "zero")


@pytest.mark.parametrize("width", [3, 16])
def test_best_value_is_the_14_form_beams_score(width):
    L, M = 5, 20
    g = load_golden("solve_mirror.npz")
    rows, pieces = g[f"L{L}_M{M}_rows"][:SOLVE_N], g[f"L{L}_M{M}_pieces"][:SOLVE_N]
    solved, length, actions, best = _solve(rows, pieces, L, M, W14, width)
    env = T.BatchedTetris(L, M, SOLVE_N, device=DEV, seed=1, auto_reset=False, assign="sequential", config_pool=(rows, pieces))
    env.reset()
    score = torch.empty(SOLVE_N, dtype=torch.float32, device=DEV)
    plan12 = torch.empty((SOLVE_N, 12), dtype=torch.uint8, device=DEV)
    T.BeamPolicy(env, W14, depth=12, width=width).act(plan=plan12)
    run = np.where(solved.astype(bool), length, (_np(plan12) != 255).sum(axis=1))
    checked = 0
    for j in range(1, 13):
        T.BeamPolicy(env, W14, depth=j, width=width).act(score=score)
        at = run >= j
        assert np.array_equal(best[at, j - 1].view(np.uint32), _np(score)[at].view(np.uint32)), (width, j)
        checked += int(at.sum())
    assert checked >= 4 * SOLVE_N
    env.terminate()


def test_a_game_of_254_moves_is_the_mirrors():
    """The longest game the planes hold, with solutions of some 250 moves that win on the environment.  A game that is won stays
    low -- the landing sums of these solutions, printed here, are 1,007 and 1,439 half rows on an MI355X --, so the carry's upper bits
    are the next test's."""
    m = _m()
    g = load_golden("solve_mirror.npz")
    rows, pieces = g["long_rows"][:2], g["long_pieces"][:2]
    for L, width in ((105, 8), (112, 2)):
        want = m.placement_solve(rows, pieces, L, 254, W14, width)
        got = _solve(rows, pieces, L, 254, W14, width)
        _same_solution(got, want, ("long", L, width))
        plies = (got[3] != 0).sum(axis=1)
        print(f"M=254 L={L} W={width}: solved {got[0].tolist()} lengths {got[1].tolist()} plies run {plies.tolist()}")
        assert plies.max() >= 200
        solved = got[0].astype(bool)
        for i in np.flatnonzero(solved):                       # the landing sum along the solution, by the mirror
            r, lines, moves, total = rows[i:i + 1], 0, 0, 0
            for j in range(got[1][i]):
                b = int(got[2][i, j])
                out = m.host_moves_traced(r, int(pieces[i, j]), b // 10, b % 10, L, 254, lines, moves)
                r, lines, moves, total = out[0], out[2], out[3], total + int(out[7][0])
            print(f"  configuration {i}: landing sum {total} over {got[1][i]} moves")
        if solved.any():
            state, moves = _replay(rows, pieces, L, 254, got[2])
            assert (state[solved] == 1).all() and np.array_equal(moves[solved], got[1][solved])


def test_a_high_game_of_254_moves_carries_a_landing_sum_past_8192():
    """The carry's landing field: 14 bits for at most 254 * 38 = 9,652 half rows, below the eroded field at bit 22.  Rows 3 .. 19
    are filled but for one column, every piece is an O and L = 112 is out of reach: a placement that does not top out lands at
    drop 1 with landing height 35, every fifth O fills rows 1 and 2 and clears both (8 eroded cells), and the game runs all 254
    plies unsolved.  best_value holds the kernel to the mirror at every ply, so a wrong shift or mask in either field would show:
      landing only      value = the landing sum itself: 35 j after ply j, 8,190 after ply 234, 8,225 after 235, 8,890 at the end;
      landing + 3 eroded - 1000 lost   both fields in one value, the lost term at the move limit only;
      Dellacherie's signs               -0.25 landing + 0.5 eroded + 0.5 cleared - 1000 lost, the values falling."""
    m = _m()
    L, M = 112, 254
    rows = np.zeros((2, 20), np.uint16)
    rows[0, 3:], rows[1, 3:] = 0x3FF & ~(1 << 9), 0x3FF & ~1
    pieces = np.full((2, M + 1), 6, np.uint8)
    weights = np.zeros((3, 14), np.float32)
    weights[0, 12] = 1.0
    weights[1, [2, 12, 13]] = [-1000.0, 1.0, 3.0]
    weights[2, [0, 2, 12, 13]] = [0.5, -1000.0, -0.25, 0.5]
    for w, width in zip(weights, (2, 8, 8)):
        want = m.placement_solve(rows, pieces, L, M, w, width)
        got = _solve(rows, pieces, L, M, w, width)
        _same_solution(got, want, ("high", w.tolist(), width))
        assert not got[0].any() and (got[2] == 255).all() and (got[3][:, -1] != 0).all()         # all 254 plies were run
    landing = _solve(rows, pieces, L, M, weights[0], 2)[3]
    assert np.array_equal(landing, np.broadcast_to(35.0 * np.arange(1, M + 1, dtype=np.float32), (2, M)))
    assert landing[0, 233] == 8190 and landing[0, 234] == 8225 and landing[0, -1] == 8890 > 8192
    both = _solve(rows, pieces, L, M, weights[1], 8)[3]
    eroded = (both[:, :-1] - landing[:, :-1]) / 3                                   # exact: small integers in float32
    assert np.array_equal(eroded[0], 8.0 * (np.arange(1, M) // 5)) and both[0, -1] == 8890 + 3 * 400 - 1000


# ------------------------------------------------------------------------------------------------ python
def test_evaluate_tune_and_a_captured_graph_at_14_features():
    L, M, per, steps = 2, 2, 256, 8
    pool = T.generate_configs(L, M, 64, seed=107)
    w = np.stack([W14, np.array(T.DELLACHERIE_WEIGHTS), np.zeros(14, np.float32)])
    env = T.BatchedTetris(L, M, 3 * per, device=DEV, seed=5, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=pool)
    out = T.evaluate_heuristic(env, w, per, steps)
    print("evaluate_heuristic at 14 features: episodes", out["episodes"].tolist(), "wins", out["wins"].tolist())
    assert out["episodes"].shape == (3,) and (out["episodes"] > 0).all()
    beam = T.evaluate_heuristic(env, w, per, steps, depth=2, width=4)
    print("  beam (2, 4): wins", beam["wins"].tolist())
    # a captured graph of act(): no allocation, no host sync; set_weights is seen by the replay
    policy = T.HeuristicPolicy(env, w, per)
    assert tuple(policy.weights.shape) == (3, 14)
    env.reset()
    want = _np(policy.act()).copy()
    flipped = _np(T.HeuristicPolicy(env, w[::-1].copy(), per).act()).copy()
    buf = torch.empty(3 * per, dtype=torch.uint8, device=DEV)
    policy.act(out=buf)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            policy.act(out=buf)
    policy.set_weights(w[::-1].copy())
    buf.fill_(255)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np(buf), flipped) and not np.array_equal(flipped, want)
    env.terminate()
    tuned = T.tune_heuristic(L, M, pool, population=8, boards_per_member=per, steps=steps, generations=2, seed=3, device=DEV,
                             features=14, init_mean=np.concatenate([CLASSICAL, np.zeros(2, np.float32)]))
    print("tune_heuristic(features=14): best fitness", tuned["best_fitness"], "history", tuned["history"])
    assert tuned["mean"].shape == (14,) and tuned["best"].shape == (14,) and len(tuned["history"]) == 2
    twelve = T.tune_heuristic(L, M, pool, population=8, boards_per_member=per, steps=steps, generations=1, seed=3, device=DEV)
    assert twelve["mean"].shape == (12,)
