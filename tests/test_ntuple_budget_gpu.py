"""The budget table and the dead-board prune on one MI355X (include/tpl_learn.h's "The budget table"; the ntuple_budget_* kernels of
csrc/learn/ntuple.hip and ntuple_beam.hip; ntuple.py).  Floats are compared as bits and canaries frame every buffer the kernels are
handed.  Every output is held to the numpy mirror, or to a reference composed ply by ply from T.afterstates, T.move_bound on an
environment of the same game and the numpy folds of _learn_lib -- nothing of the kernels under test is in a reference but
T.ntuple_value, which test 1 holds to the mirror on the boards and on their afterstates first.

  1. A BOARD SET WITH DEAD, LIVE AND FINISHED BOARDS: (L, M) = (5, 8); the 219 configurations of carved_L5_M20.npz with sol_len <= 8,
     their pieces cut to nine; 2,048 boards stepped 0 .. 4 random moves, and 128 stepped 5 .. 8 moves (on this pool no game of
     eight moves is over after five random ones; after eight all are).  value, bins, act at epsilon 0 and 0.5, search, and the beam at (3, 8) and (6, 16),
     each with the prune off and on.
  2. THE CLAMPS: fresh boards at (2, 100) read bin 255 and at (20, 100) bin 201 -- a kernel that took lines and moves left from the
     clamped counter would read 103 --; the set's boards under (20, 100) and (250, 254); the beam at its limits (11, 64) on 64 boards.
  3. TWINS: ntuple_budget(feat_table), unpruned, writes the bytes of the _feature kernels' outputs for all four read kernels; with row 9
     random and the other rows zero V is row 9's entry at sbin plus the counter.
  4. THE PRUNE'S MEANING: under a table that is worth spare + 1 on a live board, with the prune on, no board with a live placement is
     given a dead one at one ply, two plies and beam (3, 8), and `after` is the true, running afterstate even where it is dead.
  5. THE UPDATE: 256 and 2,048 boards, horizon 1 and 4, symmetric off and on: the mirror's bytes, the same after the boards are
     permuted, and a symmetric training leaves a symmetric table; six learner steps are the loop composed by hand, with the
     prune off and on, and every evaluation runs.
"""
import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from conftest import load_golden
from test_bound_gpu import _snapshots
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_gpu import GAMMA, PARAMS, _fields, _framed
from test_ntuple_trace_gpu import _age

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BUDGET, FEAT = "feat+spare", "feat"
EB, EF = 21504, 19456
GAME = (5, 8)
STEPPED, LATE = 2048, 128
N = STEPPED + LATE                                             # the stepped boards, then boards late in the game (the fixture says which)
ARANGE = np.arange(40)
LOST_LIMIT = 2


def _m():
    return T._learn_lib


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32))


def _random(seed, entries=EB, span=1 << 20):
    return np.random.default_rng(seed).integers(-span, span + 1, entries).astype(np.int32)


def _pool58():
    f = load_golden("carved_L5_M20.npz")
    keep = f["sol_len"] <= GAME[1]
    assert int(f["L"]) == GAME[0] and keep.sum() == 219
    return f["rows"][keep], np.ascontiguousarray(f["pieces"][keep][:, :GAME[1] + 1])


def _indexed(f, game):
    index, used = _m().ntuple_indices(f["rows"], f["cur"], *game, f["lines"], f["moves"], shape=BUDGET)
    assert used.all()
    return dict(fields=f, index=index)


def _value_of(table, part, idx=None):
    """The mirror's V from indices computed once: eleven entries, one rounding; 0 for a state that does not run."""
    pick = (lambda v: v) if idx is None else (lambda v: v[idx])
    total = table[pick(part["index"])].astype(np.int64).sum(axis=1)
    return np.where(pick(part["fields"]["state"]) == 0, total.astype(np.float32) * np.float32(2.0 ** -16), np.float32(0.0)).astype(np.float32)


@pytest.fixture(scope="module")
def envs():
    """An environment per game with the reward parameters: T.afterstates and T.move_bound read L, M and the rewards from it."""
    made = {}

    def get(game, params=PARAMS):
        key = (game, params)
        if key not in made:
            made[key] = T.BatchedTetris(*game, 8, device=DEV, seed=9, reward=params)
        return made[key]
    yield get
    for env in made.values():
        env.terminate()


@pytest.fixture(scope="module")
def boards():
    """The 2,048 stepped boards, their decoded fields, the mirror's bound and indices.  On this pool four random moves finish no game
    of eight moves, and no fifth move does, so the set goes on with 128 boards stepped 5 .. 8 random moves, 32 of each: boards whose
    every move ends the game at the limit, and after eight moves finished ones.  Dead, live and finished boards are all there."""
    env, A, B = _snapshots(*GAME, STEPPED, _pool58(), 4, 11)
    env.terminate()
    env, XA, XB = _snapshots(*GAME, 9 * LATE // 4, _pool58(), GAME[1], 12)
    env.terminate()
    late = np.flatnonzero(np.arange(9 * LATE // 4) % 9 >= 5)
    A, B = np.ascontiguousarray(np.concatenate([A, XA[late]])), np.ascontiguousarray(np.concatenate([B, XB[late]]))
    f = _fields(A, B)
    assert A.shape[0] == N and (f["state"][-LATE:][np.arange(LATE) % 4 == 3] != 0).all()
    bound = _m().move_bound(f["rows"], *GAME, f["lines"], f["moves"], f["state"])
    run = f["state"] == 0
    count = dict(dead=int((run & bound["dead"]).sum()), live=int((run & ~bound["dead"]).sum()), finished=int((~run).sum()))
    print("the board set:", count, "spare of the live boards", int(bound["spare"][run & ~bound["dead"]].min()), "..",
          int(bound["spare"][run & ~bound["dead"]].max()))
    assert min(count.values()) >= 30, count                    # all three are there before anything is compared
    return dict(A=A, B=B, running=run, cur=f["cur"].astype(np.int64), dead=bound["dead"], **_indexed(f, GAME))


# ------------------------------------------------------------------------------------------------ the entries, framed
def _value(A, B, table, game, form=None):
    """tpl_ntuple_value_budget; form 0: tpl_ntuple_value_feature with that form."""
    n = A.shape[0]
    a, b, t, v = _framed(A, 1), _framed(B, 2), _framed(table, 3), Framed(4 * n, 4)
    v.inner().fill_(0xCD)
    if form is None:
        _check(_lib().tpl_ntuple_value_budget(a.ptr(), b.ptr(), n, *game, t.ptr(), v.ptr(), _stream()))
    else:
        _check(_lib().tpl_ntuple_value_feature(a.ptr(), b.ptr(), n, *game, t.ptr(), v.ptr(), form, _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("value", v)):
        f.assert_canary((n, game, k))
    assert np.array_equal(t.host().view(np.int32), table) and np.array_equal(a.host(), A.view(np.uint8).reshape(-1))
    return v.host().view(np.float32).copy()


def _bins(A, B, game):
    n = A.shape[0]
    a, b, out = _framed(A, 1), _framed(B, 2), Framed(10 * n, 3)
    out.inner().fill_(0xCD)
    _check(_lib().tpl_ntuple_budget_bins(a.ptr(), b.ptr(), n, *game, out.ptr(), _stream()))
    for k, f in (("a", a), ("b", b), ("bins", out)):
        f.assert_canary((n, game, k))
    return out.host().reshape(n, 10).copy()


def _policy(depth, A, B, table, game, prune, params=PARAMS, gamma=GAMMA, epsilon=0.0, seed=0, step=0, form=None):
    """tpl_ntuple_act_budget / _search_budget with `prune`; form 0: the _feature twin with that form in the flag's place."""
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, second=1, score=4, after_a=16, after_b=16, value=4)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    head = (a.ptr(), b.ptr(), n, *game, *params, gamma, t.ptr(), epsilon, seed, step, p("action"))
    tail = (p("score"), p("after_a"), p("after_b"), p("value"), int(prune) if form is None else form, _stream())
    kind = "budget" if form is None else "feature"
    search, act = getattr(_lib(), f"tpl_ntuple_search_{kind}"), getattr(_lib(), f"tpl_ntuple_act_{kind}")
    _check(search(*head, p("second"), *tail) if depth == 2 else act(*head, *tail))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((depth, n, game, prune, epsilon, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    assert np.array_equal(t.host().view(np.int32), table)
    if depth == 1:
        assert (out.pop("second").host() == 0xCD).all()
    host = {k: f.host().copy() for k, f in out.items()}
    for k in ("after_a", "after_b"):
        host[k] = host[k].view(np.uint32).reshape(n, 4)
    for k in ("score", "value"):
        host[k] = host[k].view(np.float32)
    return host


def _beam(A, B, table, game, depth, width, prune, params=PARAMS, gamma=GAMMA, form=None):
    n = A.shape[0]
    a, b, t = _framed(A, 1), _framed(B, 2), _framed(table, 3)
    sizes = dict(action=1, plan=depth, score=4, after_a=16, after_b=16)
    out = {k: Framed(size * n, 4 + j) for j, (k, size) in enumerate(sizes.items())}
    for f in out.values():
        f.inner().fill_(0xCD)
    p = lambda k: out[k].ptr()
    entry = _lib().tpl_ntuple_beam_budget if form is None else _lib().tpl_ntuple_beam_feature
    _check(entry(a.ptr(), b.ptr(), n, *game, *params, gamma, t.ptr(), depth, width, p("action"), p("plan"), p("score"), p("after_a"),
                 p("after_b"), int(prune) if form is None else form, _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t)]:
        f.assert_canary((n, game, depth, width, prune, k))
    assert np.array_equal(t.host().view(np.int32), table) and np.array_equal(a.host(), A.view(np.uint8).reshape(-1))
    host = {k: f.host().copy() for k, f in out.items()}
    for k in ("after_a", "after_b"):
        host[k] = host[k].view(np.uint32).reshape(n, 4)
    host["plan"], host["score"] = host["plan"].reshape(n, depth), host["score"].view(np.float32)
    return host


def _same(got, want, what, keys=None):
    """Every output of `want` (or `keys` of them), byte for byte."""
    for k in (want if keys is None else keys):
        g = np.ascontiguousarray(got[k]).view(np.uint8).reshape(len(got[k]), -1)
        w = np.ascontiguousarray(np.asarray(want[k]).astype(got[k].dtype)).view(np.uint8).reshape(len(want[k]), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (what, k, bad.size, bad[:5].tolist(), got[k][bad[:5]].tolist(), np.asarray(want[k])[bad[:5]].tolist())


# ------------------------------------------------------------------------------------------------ the references' one ply
def _children(env, pa, pb, prune, r_lose):
    """T.afterstates of K states and T.move_bound of their 40 K children: planes uint32 [40 K, 4], reward f32, ended, cleared,
    distinct [40 K] and which children are left running and dead.  With `prune` such a child is what the rule makes of it: ended, its
    reward the move's with r_lose -- move_reward for a state lost at the limit --, its packed state lost at the limit.  `true_ended`
    is the move's own outcome either way."""
    after = T.afterstates(env, pa, pb)
    sa, sb = after["states_a"].view(-1, 4), after["states_b"].view(-1, 4)
    ended = _np(after["done"]).reshape(-1) != 0
    reward = _np(after["reward"]).reshape(-1).astype(np.float32)
    dead = _np(T.move_bound(env, sa, sb)["dead"]).reshape(-1) & ~ended
    A, B = _np(sa).view(np.uint32).copy(), _np(sb).view(np.uint32).copy()
    out = dict(planes=(sa, sb), dead=dead, true_ended=ended, distinct=(_np(after["canonical"]) == ARANGE[None, :]).reshape(-1))
    if prune:
        reward = np.where(dead, reward + np.float32(r_lose), reward).astype(np.float32)
        ended = ended | dead
        B[dead, 1] = (B[dead, 1] & ~np.uint32(3 << 28)) | np.uint32(LOST_LIMIT << 28)
    return dict(out, A=A, B=B, reward=reward, ended=ended)


@pytest.fixture(scope="module")
def ply(boards, envs):
    """The first ply of the 2,048 boards, unpruned and pruned, with the mirror's indices of the 81,920 true afterstates."""
    pa, pb = _i32(boards["A"]).to(DEV), _i32(boards["B"]).to(DEV)
    out = {prune: _children(envs(GAME), pa, pb, prune, PARAMS[2]) for prune in (False, True)}
    f = _fields(out[False]["A"], out[False]["B"])
    assert np.array_equal(f["state"] != 0, out[False]["true_ended"])
    out["indexed"] = _indexed(f, GAME)
    cut = out[True]["dead"].reshape(N, 40) & out[True]["distinct"].reshape(N, 40) & boards["running"][:, None]
    print("first ply: boards with a dead placement", int(cut.any(axis=1).sum()), "with nothing but dead or ended ones",
          int((boards["running"] & (cut | out[False]["true_ended"].reshape(N, 40) | ~out[True]["distinct"].reshape(N, 40)).all(axis=1)).sum()))
    assert cut.any(axis=1).sum() >= 100
    return out


@pytest.fixture(scope="module")
def table():
    return _random(41)


# ------------------------------------------------------------------------------------------------ 1. the board set
def test_value_and_bins_are_the_mirror_on_the_boards_and_on_their_afterstates(boards, ply, table):
    got = _value(boards["A"], boards["B"], table, GAME)
    assert np.array_equal(_bits(got), _bits(_value_of(table, boards)))
    assert (_bits(got)[~boards["running"]] == 0).all() and (got[boards["running"]] != 0).all()
    f = boards["fields"]
    bins = _bins(boards["A"], boards["B"], GAME)
    want = _m().ntuple_budget_bins(f["rows"], *GAME, f["lines"], f["moves"], f["state"])
    assert np.array_equal(bins, want)
    run = boards["running"]
    assert (bins[run & boards["dead"], 9] == 0).all() and (bins[run & ~boards["dead"], 9] >= 1).all() and (bins[~run, 9] == 1).all()
    assert np.unique(bins[run, 9]).size >= 8
    # the public functions, at sizes around a block's edge; T.ntuple_value is what the deeper references take V from
    dev_table = torch.from_numpy(table).to(DEV)
    for size in (1, 7, 257):
        planes = tuple(_i32(x[5:5 + size]).to(DEV) for x in (boards["A"], boards["B"]))
        assert np.array_equal(_np(T.ntuple_budget_bins(planes, *GAME)), want[5:5 + size])
        assert np.array_equal(_bits(_np(T.ntuple_value(planes, dev_table, *GAME))), _bits(got[5:5 + size]))
    full = _random(18, span=(1 << 31) - 1)                     # the whole int32 range: the sum is rounded at the conversion
    wide = _value(boards["A"], boards["B"], full, GAME)
    assert np.array_equal(_bits(wide), _bits(_value_of(full, boards))) and (np.abs(wide) * 65536.0 > (1 << 24)).any()
    held = _np(T.ntuple_value(ply[False]["planes"], dev_table, *GAME))
    assert np.array_equal(_bits(held), _bits(_value_of(table, ply["indexed"])))
    cf = ply["indexed"]["fields"]
    child_bins = _np(T.ntuple_budget_bins(ply[False]["planes"], *GAME))
    assert np.array_equal(child_bins, _m().ntuple_budget_bins(cf["rows"], *GAME, cf["lines"], cf["moves"], cf["state"]))
    assert np.array_equal(child_bins[:, 9] == 0, ply[False]["dead"])          # T.move_bound's dead children are the mirror's bin 0


def _explored(boards, ply, greedy, epsilon, seed, step):
    """The action played: the greedy one, or where a running board explores the j-th of its distinct placements (ntuple_explore)."""
    run = boards["running"]
    explores, j = _m().ntuple_explore(seed, step, N, epsilon, np.array(_m().PIECE_PLACEMENTS)[boards["cur"]])
    explores &= run
    order = np.argsort(~ply[False]["distinct"].reshape(N, 40), axis=1, kind="stable")      # the distinct placements first, ascending
    return np.where(explores, order[np.arange(N), j], np.where(run, greedy, 0)), explores


def _outcome(boards, ply, v, action):
    """What follows from the action played, pruned or not: its TRUE one-ply afterstate (the board itself where it is finished) and V of it."""
    at, run = np.arange(N), boards["running"]
    true = ply[False]
    value = np.where(true["true_ended"].reshape(N, 40)[at, action] | ~run, np.float32(0.0), v[at, action]).astype(np.float32)
    return dict(after_a=np.where(run[:, None], true["A"].reshape(N, 40, 4)[at, action], boards["A"]),
                after_b=np.where(run[:, None], true["B"].reshape(N, 40, 4)[at, action], boards["B"]), value=value)


@pytest.mark.parametrize("prune", [False, True])
def test_act_is_the_arg_max_of_the_rule_at_both_epsilons(boards, ply, table, prune):
    v = _value_of(table, ply["indexed"]).reshape(N, 40)
    side = ply[prune]
    reward, ended, distinct = (side[k].reshape(N, 40) for k in ("reward", "ended", "distinct"))
    score = np.where(ended, reward, reward + np.float32(GAMMA) * v).astype(np.float32)
    score = np.where(boards["running"][:, None], score, np.float32(0.0))
    masked = np.where(distinct, score, -np.inf)
    greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    for epsilon in (0.0, 0.5):
        action, explores = _explored(boards, ply, greedy, epsilon, seed, step)
        want = dict(action=action.astype(np.uint8), score=score[np.arange(N), greedy], **_outcome(boards, ply, v, action))
        got = _policy(1, boards["A"], boards["B"], table, GAME, prune, epsilon=epsilon, seed=seed, step=step)
        _same(got, want, (prune, epsilon))
    run = boards["running"]
    assert 0.4 * run.sum() < explores.sum() < 0.6 * run.sum()
    assert (got["action"][~run] == 0).all() and (_bits(got["score"])[~run] == 0).all() and (_bits(got["value"])[~run] == 0).all()
    if prune:                                                  # the prune moved scores and choices, and exploration still plays dead moves
        other = _policy(1, boards["A"], boards["B"], table, GAME, False)
        greedy_got = _policy(1, boards["A"], boards["B"], table, GAME, True)
        assert (_bits(other["score"]) != _bits(greedy_got["score"])).sum() >= 20 and (other["action"] != greedy_got["action"]).sum() >= 20
        played_dead = ply[True]["dead"].reshape(N, 40)[np.arange(N), got["action"]] & run
        assert played_dead.sum() >= 20 and ((got["after_b"][played_dead, 1] >> 28) & 3 == 0).all() and (got["value"][played_dead] != 0).all()


@pytest.mark.parametrize("prune", [False, True])
def test_search_is_ntuple_search_choice_on_two_plies_of_the_rule(boards, ply, envs, table, prune):
    dev_table = torch.from_numpy(table).to(DEV)
    v1 = _value_of(table, ply["indexed"]).reshape(N, 40)
    side = ply[prune]
    two = _children(envs(GAME), *ply[False]["planes"], prune, PARAMS[2])
    v2 = _np(T.ntuple_value(two["planes"], dev_table, *GAME))   # of the true second afterstates; read only where the rule goes on
    cube = (N, 40, 40)
    run = boards["running"]
    greedy, _, score, _, second = _m().ntuple_search_choice(side["reward"].reshape(N, 40), side["ended"].reshape(N, 40),
                                                            side["distinct"].reshape(N, 40), two["reward"].reshape(cube),
                                                            two["ended"].reshape(cube), v2.reshape(cube), two["distinct"].reshape(cube),
                                                            GAMMA, running=run)
    seed, step = 0xDEADBEEFCAFEF00D, (1 << 40) + 3
    at = np.arange(N)
    for epsilon in (0.0, 0.5):
        action, explores = _explored(boards, ply, greedy.astype(np.int64), epsilon, seed, step)
        want = dict(action=action.astype(np.uint8), second=second[at, action], score=score, **_outcome(boards, ply, v1, action))
        got = _policy(2, boards["A"], boards["B"], table, GAME, prune, epsilon=epsilon, seed=seed, step=step)
        _same(got, want, (prune, epsilon))
        assert (got["action"][~run] == 0).all() and (got["second"][~run] == 255).all() and (_bits(got["score"])[~run] == 0).all()
    if prune:
        dead_second = two["dead"].reshape(cube) & two["distinct"].reshape(cube) & ~side["ended"].reshape(N, 40)[:, :, None]
        assert dead_second.any(axis=(1, 2)).sum() >= 100       # the second ply met dead children too
        played_dead = side["dead"].reshape(N, 40)[at, got["action"]] & run
        assert played_dead.sum() >= 20 and (got["second"][played_dead] == 255).all() and (got["value"][played_dead] != 0).all()
        other = _policy(2, boards["A"], boards["B"], table, GAME, False)
        greedy_got = _policy(2, boards["A"], boards["B"], table, GAME, True)
        assert (_bits(other["score"]) != _bits(greedy_got["score"])).sum() >= 20


def _state_of(B):
    return (B[..., 1] >> np.uint32(28)) & np.uint32(3)


def compose(env, table, A, B, game, depth, width, prune, params=PARAMS, gamma=GAMMA):
    """The beam's rule without the beam kernel, as test_ntuple_beam_gpu composes it: every ply is _children on the beam's planes -- with
    `prune` a dead child is a lost node from there on --, V of the children from T.ntuple_value, the numpy fold and ntuple_beam_ply."""
    m = _m()
    n = A.shape[0]
    dev_table = torch.from_numpy(table).to(DEV)
    f = _fields(A, B)
    plies = np.where(f["state"] == 0, np.minimum(depth, 11 - f["moves"] % 10), 0)
    nodeA, nodeB = A[:, None, :].copy(), B[:, None, :].copy()
    value = np.zeros((n, 1), np.float32)
    rewards = np.zeros((n, 1, depth), np.float32)
    path = np.full((n, 1, depth), 255, np.uint8)
    size = np.ones(n, np.int64)
    pruned = np.zeros(n, bool)
    for j in range(int(plies.max(initial=0))):
        act = np.flatnonzero(plies > j)
        k, wc = act.size, nodeA.shape[1]
        kids = _children(env, _i32(nodeA[act].reshape(-1, 4)).to(DEV), _i32(nodeB[act].reshape(-1, 4)).to(DEV), prune, params[2])
        v = _np(T.ntuple_value(kids["planes"], dev_table, *game))
        sa, sb = kids["A"].reshape(k, wc, 40, 4), kids["B"].reshape(k, wc, 40, 4)
        reward, ended, distinct, dead = (kids[key].reshape(k, wc, 40) for key in ("reward", "ended", "distinct", "dead"))
        run = _state_of(nodeB[act]) == 0
        before = np.broadcast_to(rewards[act][:, :, None, :j], (k, wc, 40, j))
        folded = m.ntuple_beam_values(np.concatenate([before, reward[..., None]], axis=3).reshape(-1, j + 1), ended.reshape(-1),
                                      v.reshape(-1), gamma).reshape(k, wc, 40)
        keep = []
        for t, s in enumerate(act):
            live = int(size[s])
            keep.append(m.ntuple_beam_ply(value[s, :live], run[t, :live], folded[t, :live], distinct[t, :live], width))
        wn = max(wc, max(q.size for q, _, _ in keep))
        grown = lambda x, fill: np.concatenate([x, np.full((n, wn - wc) + x.shape[2:], fill, x.dtype)], axis=1)
        nodeA, nodeB, value, rewards, path = (grown(x, fl) for x, fl in ((nodeA, 0), (nodeB, 0), (value, 0), (rewards, 0), (path, 255)))
        for t, s in enumerate(act):
            q, b, val = keep[t]
            moved = b != 255
            b0 = np.where(moved, b, 0)
            new_path, new_rewards = path[s, q].copy(), rewards[s, q].copy()
            new_path[moved, j] = b[moved]
            new_rewards[moved, j] = reward[t, q, b0][moved]
            pruned[s] |= bool((dead[t, q, b0] & moved & run[t, q]).any())
            nodeA[s, :q.size], nodeB[s, :q.size] = sa[t, q, b0], sb[t, q, b0]
            value[s, :q.size], path[s, :q.size], rewards[s, :q.size] = val, new_path, new_rewards
            size[s] = q.size
    at = np.arange(n)
    best = np.array([m.beam_select(value[s, :size[s]], 1)[0] for s in range(n)], np.int64)
    return dict(action=np.where(plies > 0, path[at, best, 0], 0).astype(np.uint8), plan=path[at, best], score=value[at, best],
                plies=plies, dead_kept=pruned)


@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("depth,width", [(3, 8), (6, 16)])
def test_the_beam_is_the_reference_composed_ply_by_ply(boards, ply, envs, table, depth, width, prune):
    A, B, run = boards["A"], boards["B"], boards["running"]
    want = compose(envs(GAME), table, A, B, GAME, depth, width, prune)
    got = _beam(A, B, table, GAME, depth, width, prune)
    _same(got, want, (depth, width, prune), keys=("action", "plan", "score"))
    assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all() and (_bits(got["score"][~run]) == 0).all()
    assert (got["plan"][run, 0] == got["action"][run]).all() and (want["plies"] >= min(depth, 3)).sum() >= 500
    # `after` is the true one-ply afterstate of the action, pruned or not
    at = np.arange(N)
    true = ply[False]
    assert np.array_equal(got["after_a"], np.where(run[:, None], true["A"].reshape(N, 40, 4)[at, got["action"]], A))
    assert np.array_equal(got["after_b"], np.where(run[:, None], true["B"].reshape(N, 40, 4)[at, got["action"]], B))
    print(f"beam ({depth}, {width}) prune {prune}: boards whose beam kept a dead child", int(want["dead_kept"].sum()))
    if prune:
        other = _beam(A, B, table, GAME, depth, width, False)
        assert (_bits(other["score"]) != _bits(got["score"])).sum() >= 20
    else:                                                      # depth 1 is act and (2, 34) search, as for every other form
        one, two = _policy(1, A, B, table, GAME, False), _policy(2, A, B, table, GAME, False)
        _same(_beam(A, B, table, GAME, 1, 5, False), one, "depth 1", keys=("action", "score", "after_a", "after_b"))
        _same(_beam(A, B, table, GAME, 2, 34, False), two, "depth 2", keys=("action", "score", "after_a", "after_b"))


def test_the_pruned_beam_at_depth_one_and_two_is_the_pruned_act_and_search(boards, table):
    A, B = boards["A"], boards["B"]
    _same(_beam(A, B, table, GAME, 1, 5, True), _policy(1, A, B, table, GAME, True), "depth 1", keys=("action", "score", "after_a", "after_b"))
    _same(_beam(A, B, table, GAME, 2, 34, True), _policy(2, A, B, table, GAME, True), "depth 2", keys=("action", "score", "after_a", "after_b"))


# ------------------------------------------------------------------------------------------------ 2. the clamps
def _spare_table():
    """Row 9 holds b * 2^16 at bin b under every piece, everything else 0: V of a running board is its sbin."""
    t = np.zeros(EB, np.int32)
    t[:20480].reshape(8, 10, 256)[:, 9] = (np.arange(256) << 16)[None, :]
    return t


def test_fresh_boards_read_bin_255_at_2_100_and_bin_201_at_20_100_and_never_the_clamped_counters_103(boards):
    window = (np.arange(16, dtype=np.uint64) % np.uint64(8)) | (np.uint64(0o1234560123) << np.uint64(3))
    A, B = R.pack_state(np.zeros((16, 20), np.uint16), 0, 0, 0, 0, window)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    for game, sbin in (((2, 100), 255), ((20, 100), 201), ((15, 63), 103)):
        assert (_bins(A, B, game)[:, 9] == sbin).all(), game
        assert (_value(A, B, _spare_table(), game) == np.float32(sbin)).all(), game
    # the set's boards under games whose counters pass the clamps: the mirror, bit for bit
    table = _random(7)
    f = boards["fields"]
    for game in ((20, 100), (250, 254), (2, 100)):
        part = _indexed(f, game)
        assert np.array_equal(_bits(_value(boards["A"], boards["B"], table, game)), _bits(_value_of(table, part))), game
        want = _m().ntuple_budget_bins(f["rows"], *game, f["lines"], f["moves"], f["state"])
        assert np.array_equal(_bins(boards["A"], boards["B"], game), want), game
        if game == (20, 100):                                  # every board here has more than 15 lines and 63 moves left
            assert (20 - f["lines"]).min() >= 15 and (100 - f["moves"]).min() >= 63
            spare = 4 * 63 - _m().move_bound_cells(f["rows"], 15)
            clamped = np.where(spare < 0, 0, np.minimum(spare + 1, 255))
            run = f["state"] == 0
            assert (clamped[run] != want[run, 9]).mean() > 0.9 # the reading from the clamped counters is another one: the test tells them apart


def test_the_beam_at_its_limits_on_64_fresh_boards_of_a_game_past_the_clamps(boards, envs):
    game = (20, 100)
    fresh = np.flatnonzero((boards["fields"]["moves"] == 0) & boards["running"])[:64]
    assert fresh.size == 64
    A, B = np.ascontiguousarray(boards["A"][fresh]), np.ascontiguousarray(boards["B"][fresh])
    table = _random(11)
    for prune in (False, True):
        want = compose(envs(game), table, A, B, game, 11, 64, prune)
        assert (want["plies"] == 11).all()
        _same(_beam(A, B, table, game, 11, 64, prune), want, ("limits", prune), keys=("action", "plan", "score"))
    spare = compose(envs(game), _spare_table(), A, B, game, 11, 64, False)      # leaves valued by their own spare alone
    _same(_beam(A, B, _spare_table(), game, 11, 64, False), spare, "limits, spare table", keys=("action", "plan", "score"))


# ------------------------------------------------------------------------------------------------ 3. twins
def test_a_promoted_feature_table_unpruned_writes_the_feature_kernels_bytes(boards):
    feat = _random(23, EF)
    promoted = _np(T.ntuple_budget(torch.from_numpy(feat).to(DEV)))
    assert promoted.shape == (EB,) and (promoted[:20480].reshape(8, 10, 256)[:, 9] == 0).all()
    A, B = boards["A"], boards["B"]
    assert np.array_equal(_bits(_value(A, B, promoted, GAME)), _bits(_value(A, B, feat, GAME, form=0)))
    seed, step = 77, 5
    for depth in (1, 2):
        for epsilon in (0.0, 0.5):
            _same(_policy(depth, A, B, promoted, GAME, False, epsilon=epsilon, seed=seed, step=step),
                  _policy(depth, A, B, feat, GAME, False, epsilon=epsilon, seed=seed, step=step, form=0), (depth, epsilon))
    for depth, width in ((3, 8), (6, 16)):
        _same(_beam(A, B, promoted, GAME, depth, width, False), _beam(A, B, feat, GAME, depth, width, False, form=0), (depth, width))
    # the prune is not the twin's: it changes what the promoted table plays
    assert (_policy(1, A, B, promoted, GAME, True)["action"] != _policy(1, A, B, promoted, GAME, False)["action"]).any()
    # row 9 random and the other rows zero: V is row 9's entry at sbin plus the counter
    only = np.zeros(EB, np.int32)
    full = _random(29)
    only[:20480].reshape(8, 10, 256)[:, 9] = full[:20480].reshape(8, 10, 256)[:, 9]
    only[20480:] = full[20480:]
    index = boards["index"]
    want = (only[index[:, 9]].astype(np.int64) + only[index[:, 10]]).astype(np.float32) * np.float32(2.0 ** -16)
    want = np.where(boards["running"], want, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(_bits(_value(A, B, only, GAME)), _bits(want)) and len(set(_bits(want).tolist())) > 100


# ------------------------------------------------------------------------------------------------ 4. the prune's meaning
MEANING = (0.0, 1.0, -1.0)                                     # r_line, r_win, r_lose of this test


def test_with_the_prune_no_board_with_a_live_placement_is_given_a_dead_one(boards, envs):
    """Row 9 is b * 2^16 at bin b >= 1 and a large negative at bin 0, everything else zero: V of a live board is spare + 1 >= 1.
    Rewards (0, 1, -1), gamma 0.99.  With the prune on a dead first move is worth exactly -1, at any depth.  A live first move is
    worth 0.99 * V >= 0.99 at one ply; deeper it is worth gamma times the best of what follows, and the worst that can follow is a
    loss, -1, so it is worth at least -0.99 > -1 -- and in the beam a live node's children, worth at least -0.99, pass every dead node
    at the cut.  So the arg-max never lands on a dead placement while a live one exists, by arithmetic and not by luck."""
    table = _spare_table()
    table[:20480].reshape(8, 10, 256)[:, 9, 0] = -(1 << 28)
    A, B, run = boards["A"], boards["B"], boards["running"]
    env = envs(GAME, MEANING)
    kids = _children(env, _i32(A).to(DEV), _i32(B).to(DEV), False, MEANING[2])
    dead = kids["dead"].reshape(N, 40) & kids["distinct"].reshape(N, 40)
    live = ~kids["true_ended"].reshape(N, 40) & ~kids["dead"].reshape(N, 40) & kids["distinct"].reshape(N, 40)
    has_live, only_dead = run & live.any(axis=1), run & dead.any(axis=1) & ~live.any(axis=1)
    print("boards with a live placement", int(has_live.sum()), "of them with a dead one too", int((has_live & dead.any(axis=1)).sum()),
          "with dead placements and no live one", int(only_dead.sum()))
    assert (has_live & dead.any(axis=1)).sum() >= 100 and only_dead.sum() >= 10
    at = np.arange(N)
    outs = dict(one=_policy(1, A, B, table, GAME, True, params=MEANING), two=_policy(2, A, B, table, GAME, True, params=MEANING),
                beam=_beam(A, B, table, GAME, 3, 8, True, params=MEANING))
    for name, got in outs.items():
        chosen_dead = dead[at, got["action"]] & run
        assert not (chosen_dead & has_live).any(), name
        # where a dead move is played all the same, `after` is the true afterstate: running, not lost
        stuck = chosen_dead & only_dead
        assert np.array_equal(got["after_a"][run], kids["A"].reshape(N, 40, 4)[at, got["action"]][run]), name
        assert np.array_equal(got["after_b"][run], kids["B"].reshape(N, 40, 4)[at, got["action"]][run]), name
        assert (_state_of(got["after_b"])[stuck] == 0).all(), name
        print(name, "boards that could only play a dead move and did", int(stuck.sum()))
    assert (dead[at, outs["one"]["action"]] & only_dead).sum() >= 1
    # a dead first move is worth its reward with r_lose and nothing else, though the table holds a large negative for it
    stuck = dead[at, outs["one"]["action"]] & run
    assert (outs["one"]["score"][stuck] == np.float32(-1.0)).all() and (outs["one"]["value"][stuck] == np.float32(-(1 << 12))).all()


# ------------------------------------------------------------------------------------------------ 5. the update
def _update(A, B, head, horizon, start, error, rate, decay, symmetric, game=GAME):
    """tpl_ntuple_update_trace_budget of a host ring (uint32 [slots, n, 4] each) through canary-framed buffers: the table it leaves."""
    slots, n = A.shape[:2]
    a, b, t, e = _framed(A, 1), _framed(B, 2), _framed(start, 3), _framed(error, 4)
    _check(_lib().tpl_ntuple_update_trace_budget(a.ptr(), b.ptr(), n, slots, head, horizon, *game, t.ptr(), e.ptr(), rate, decay,
                                                 int(symmetric), _stream()))
    for k, f in (("a", a), ("b", b), ("table", t), ("error", e)):
        f.assert_canary((n, slots, head, horizon, k))
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(e.host(), error.view(np.uint8))
    return t.host().view(np.int32).copy()


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("horizon,head", [(1, 4), (4, 1)])
@pytest.mark.parametrize("n", [256, STEPPED])
def test_the_update_leaves_the_mirrors_bytes_and_the_same_bytes_with_the_boards_permuted(boards, n, horizon, head, symmetric):
    slots = 5
    gen = np.random.default_rng(100 * horizon + n + symmetric)
    picks = gen.integers(0, N, (slots, n))
    A, B = np.ascontiguousarray(boards["A"][picks]), np.ascontiguousarray(boards["B"][picks])
    rate = 3000.0
    error = gen.normal(size=n).astype(np.float32)
    special = np.array([0.0, np.nan, 1e9, -1e9, 0.52 / rate, -0.0, np.inf], np.float32)
    error[gen.permutation(n)[:special.size]] = special
    start = np.random.default_rng(n).integers(-(1 << 31), 1 << 31, EB).astype(np.int32)
    start[::3] = np.int32((1 << 31) - 1)                       # entries at the top of the range: their adds wrap
    ages = [_age(boards["fields"], picks[(head - k) % slots]) for k in range(horizon)]
    assert horizon == 1 or head < horizon - 1                  # the older ages wrap past slot 0
    got = _update(A, B, head, horizon, start, error, rate, 0.9, symmetric)
    want = _m().ntuple_update_trace(start.copy(), ages, *GAME, error, rate, 0.9, bool(symmetric))
    assert np.array_equal(got, want) and (got != start).any()
    changed = (got != start)[:20480].reshape(8, 10, 256)
    assert changed[:, 9, 0].any() and changed[:, 9, 1:].any() and changed[:, :9].any() and (got != start)[20480:].any()
    order = gen.permutation(n)
    again = _update(np.ascontiguousarray(A[:, order]), np.ascontiguousarray(B[:, order]), head, horizon, start,
                    np.ascontiguousarray(error[order]), rate, 0.9, symmetric)
    assert np.array_equal(again, got)
    if symmetric:                                              # from a symmetric table a symmetric training leaves a symmetric one
        left = _update(A, B, head, horizon, np.zeros(EB, np.int32), error, rate, 0.9, 1)
        assert T.ntuple_is_symmetric(torch.from_numpy(left).to(DEV)) and np.count_nonzero(left) > 100
    else:
        left = _update(A, B, head, horizon, np.zeros(EB, np.int32), error, rate, 0.9, 0)
        assert not T.ntuple_is_symmetric(torch.from_numpy(left).to(DEV))


def _carved_env(n, seed=3):
    return T.BatchedTetris(*GAME, n, device=DEV, seed=seed, auto_reset=True, reward=PARAMS, config_pool=_pool58())


def _by_hand(env, steps, gamma, rate, epsilon, seed, bound):
    """The learner's loop from the public pieces: NTuplePolicy.act, ntuple_value, the subtraction, the update entry, the step."""
    n = env.num_envs
    table = T.ntuple_table(DEV, BUDGET)
    policy = T.NTuplePolicy(env, table, gamma, epsilon, seed, bound=bound)
    action, done = (torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(2))
    reward, score, error = (torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(3))
    kept = [torch.zeros((n, 4), dtype=torch.int32, device=DEV) for _ in range(2)]
    nxt = [torch.zeros((n, 4), dtype=torch.int32, device=DEV) for _ in range(2)]
    kept[1][:, 1] = 1 << 28                                    # finished states: nothing is kept before the first step
    for step in range(steps):
        policy.act(out=action, score=score, after=tuple(nxt), step=step)
        torch.sub(score, T.ntuple_value(tuple(kept), table, env.L, env.M), out=error)
        _check(_lib().tpl_ntuple_update_trace_budget(kept[0].data_ptr(), kept[1].data_ptr(), n, 1, 0, 1, env.L, env.M, table.data_ptr(),
                                                     error.data_ptr(), rate, 0.0, 0, _stream()))
        env.step_into(action, reward, done)
        kept, nxt = nxt, kept
    return table


@pytest.mark.parametrize("bound", [False, True])
def test_learner_steps_are_the_loop_composed_by_hand_and_every_evaluation_runs(bound):
    kw = dict(gamma=0.99, rate=64.0, epsilon=0.25, seed=5)
    n = 1024
    env = _carved_env(n)
    env.reset()
    want = _np(_by_hand(env, 6, bound=bound, **kw)).copy()
    env.terminate()
    env = _carved_env(n)
    env.reset()
    learner = T.NTupleLearner(env, shape=BUDGET, bound=bound, **kw)
    assert learner.shape == BUDGET and learner.bound is bound and learner.policy.bound is bound and tuple(learner.table.shape) == (EB,)
    assert learner.train(6) == 6
    got = _np(learner.table).copy()
    assert np.array_equal(got, want)
    body = got[:20480].reshape(8, 10, 256)
    assert np.count_nonzero(body[:, 9]) > 5 and np.count_nonzero(body[:, :9]) > 10 and np.count_nonzero(got[20480:]) > 0
    played = {(d, w, b): learner.evaluate(16, depth=d, width=w, bound=b) for d, w in ((1, None), (2, None), (3, 8)) for b in (False, True)}
    assert all(r["episodes"] > 0 for r in played.values())
    assert learner.evaluate(16) == played[(1, None, bound)] and torch.equal(learner.table, torch.from_numpy(got).to(DEV))
    print(f"bound {bound}: " + ", ".join(f"{k} {v['wins']} of {v['episodes']}" for k, v in played.items()))
    env.terminate()
    # symmetric with traces, from a promoted feature table with row 9 zero: stays symmetric where it started so
    env = _carved_env(n)
    start = T.ntuple_budget(T.ntuple_table(DEV, FEAT))
    sym = T.NTupleLearner(env, shape=BUDGET, bound=bound, lam=0.8, horizon=2, symmetric=True, start=start, **kw)
    sym.train(6)
    assert T.ntuple_is_symmetric(sym.table) and int((sym.table != 0).sum()) > 10
    env.terminate()
