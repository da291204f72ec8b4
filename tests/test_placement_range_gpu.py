"""The placement family on one MI355X at the ends of the game range: tpl_afterstates, tpl_placement_features, tpl_placement_act,
tpl_placement_search and tpl_placement_beam at (L, M) = (1, 1), (2, 3) and (250, 254), on the 320 states per game of
test_placement_range_cpu.py (whose CPU test asserts what they cover).  The sibling files play L = 10 / M = 40 only; their helpers
take the game as keyword arguments and are used here as they are, buffers framed by canaries, inputs asserted read only.

  1. AFTERSTATES: all 320 x 40 pairs against the C oracle as test_afterstates_gpu compares them; at (250, 254) `lines` reaches 253
     next to window bit 32, which stays the input's bit 35.
  2. FEATURES / ACT: the oracle's move and _learn_lib.board_features; the numpy arg-max of placement_score, bit for bit.
  3. SEARCH: composed from the one-ply kernels at this game on every state, and two oracle moves on 48 of them; at (1, 1) every
     first move ends the game, so `second` is 255 everywhere and action and score are tpl_placement_act's.
  4. BEAM: test_beam_gpu's compose() on every state and oracle_beam on 48; at (1, 1) any depth is depth 1; at (250, 254) the
     effective depth 12 - moves % 10 at moves in the hundreds; at (2, 3) wins after the first ply and finished nodes carried.
  5. The Python surface hands the environment's L and M to every entry.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from test_afterstates_gpu import REWARDS, _assert_against_the_oracle, _resident, _run
from test_beam_gpu import CLASSICAL, RANDOM, SMALL, States, _beam, compose, oracle_beam
from test_beam_gpu import _same as _same_beam
from test_heuristic_gpu import Cases, _act, _planes, _weight_sets
from test_learn_range_gpu import Framed, _check, _lib, _stream
from test_learner_gpu import _np
from test_placement_range_cpu import COUNT, GAMES, range_pool
from test_search_gpu import TwoPly, _search
from test_search_gpu import _same as _same_search

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NF = 12
N = COUNT
ARANGE = np.arange(40)
ALL = np.arange(N)
WEIGHTS = [(name, w) for name, w in _weight_sets() if not name.startswith(("one-hot", "all zero", "random, wide"))]
assert [name for name, _ in WEIGHTS][:3] == ["random", "small integers", "the classical signs"] and len(WEIGHTS) == 5
BEAM_SHAPES = [(2, 34), (3, 4), (12, 2)]
ORACLE_STATES = 48


def _m():
    return T._learn_lib


class World:
    """One game: the states and the oracle's outcomes (shared with the CPU file), phi of every pair, the planes on the device."""

    def __init__(self, oracle, L, M):
        self.L, self.M = L, M
        self.game = dict(L=L, M=M)
        self.pool = range_pool(oracle, L, M)
        print(f"(L, M) = ({L}, {M}): the oracle's outcomes over {N} x 40 pairs: {self.pool.coverage()}")
        self.cases = Cases(oracle, self.pool)
        self.states = States(self.pool.fields)
        assert np.array_equal(self.states.A, self.pool.A) and np.array_equal(self.states.B, self.pool.B)
        self.a, self.b = _planes(self.pool.A, self.pool.B)
        self.memo = {}

    def read_only(self):
        assert np.array_equal(self.a.host(), self.pool.A.view(np.uint8).reshape(-1))
        assert np.array_equal(self.b.host(), self.pool.B.view(np.uint8).reshape(-1))

    def reference(self, name, w, depth, width):
        """compose() of all 320 states at this game, once per (weights, depth, width)."""
        key = (name, depth, width)
        if key not in self.memo:
            env = T.BatchedTetris(self.L, self.M, 8, device=DEV, seed=9, reward=REWARDS[0])
            s = self.states
            self.memo[key] = compose(env, s.A, s.B, s.plies(ALL, depth), np.broadcast_to(np.asarray(w, np.float32), (N, NF)),
                                     depth, width)
            env.terminate()
        return self.memo[key]


_WORLDS = {}


def _world(oracle, L, M):
    if (L, M) not in _WORLDS:
        _WORLDS[(L, M)] = World(oracle, L, M)
    return _WORLDS[(L, M)]


@pytest.fixture
def world(oracle, L, M):
    return _world(oracle, L, M)


games = pytest.mark.parametrize("L,M", GAMES)


# ------------------------------------------------------------------------------------------------ 1. afterstates
@games
def test_afterstates_are_the_oracle_move_at_the_ends_of_the_game_range(world, L, M):
    pool = world.pool
    full = {}
    for params in REWARDS:
        got = full[params] = _run(pool.A, pool.B, params, **world.game)      # canaries and read-only inputs are asserted there
        assert set(got) == {"out_a", "out_b", "reward", "done", "cleared", "canonical"}
        _assert_against_the_oracle(pool, ALL, got, params, (L, M, params))
    assert np.array_equal(full[REWARDS[0]]["out_a"], full[REWARDS[1]]["out_a"])
    assert np.array_equal(full[REWARDS[0]]["out_b"], full[REWARDS[1]]["out_b"])
    # the window's top four bits, stated on the raw word: bits 28..31 of B.z are the input's window bit 35 and three zeros
    run = pool.running
    top = got["out_b"][:, :, 2] >> np.uint32(28)
    want = np.broadcast_to((pool.fields["window"] >> np.uint64(35)).astype(np.uint32)[:, None], (N, 40))
    assert np.array_equal(top[run], want[run]) and want[run].any() and not want[run].all()
    if (L, M) == (1, 1):
        assert (got["done"] == 1).all()
    if (L, M) == (250, 254):
        high = run[:, None] & (pool.lines >= 251)              # bits 20..27 of B.z full to 0xFB .. 0xFD, right under those four
        assert high.sum() >= 8 and (pool.lines[high] == 253).any()
        assert np.array_equal(top[high], want[high]) and want[high].any() and not want[high].all()
        assert np.array_equal((got["out_b"][:, :, 2] >> np.uint32(20))[high] & np.uint32(0xFF), pool.lines[high].astype(np.uint32))
        last = run[:, None] & pool.won & (pool.moves == M)     # won goes before the limit, with both counters at their top
        assert last.sum() >= 8 and (got["done"][last] == 1).all()
        assert ((got["out_b"][:, :, 1] >> np.uint32(28)) & np.uint32(3))[last].tolist() == [1] * int(last.sum())


# ------------------------------------------------------------------------------------------------ 2. features, act
def _features(a, b, n, L, M):
    """tpl_placement_features at the game (L, M) through canary-framed buffers: (features int64 [n, 40, 12], canonical u8 [n, 40])."""
    feats, canon = Framed(n * 40 * NF * 2, 3), Framed(n * 40, 4)
    feats.inner().fill_(0xCD)
    canon.inner().fill_(0xCD)
    _check(_lib().tpl_placement_features(a.ptr(), b.ptr(), n, L, M, feats.ptr(), canon.ptr(), _stream()))
    for name, f in (("features", feats), ("canonical", canon), ("a", a), ("b", b)):
        f.assert_canary((n, L, M, name))
    return feats.host().view(np.int16).reshape(n, 40, NF).astype(np.int64), canon.host().reshape(n, 40).copy()


@games
def test_features_are_the_oracle_move_and_the_mirror_and_the_action_is_the_numpy_arg_max(world, L, M):
    cases, pool = world.cases, world.pool
    got, canonical = _features(world.a, world.b, N, L, M)
    wrong = np.argwhere(got != cases.phi)
    assert wrong.size == 0, (wrong[:5].tolist(), got[tuple(wrong[0][:2])].tolist(), cases.phi[tuple(wrong[0][:2])].tolist())
    assert np.array_equal(canonical, cases.canonical)
    run = pool.running
    assert (got[~run] == 0).all() and (~run).any() and (got[run].reshape(-1, NF).max(axis=0) > 0).all()
    if (L, M) == (1, 1):                                       # every pair of a running board ends the game: won or lost
        assert ((got[run][:, :, 1] + got[run][:, :, 2]) == 1).all()
    for name, w in WEIGHTS:
        act, score = _act(world.a, world.b, N, w, N, **world.game)
        want_act, want_score = cases.best(ALL, w, N)
        assert np.array_equal(act, want_act), (name, np.flatnonzero(act != want_act)[:5])
        assert np.array_equal(score.view(np.uint32), want_score.view(np.uint32)), name
        assert cases.distinct[ALL, act].all() and (act[~run] == 0).all()
    per = 3                                                    # a population: 107 members, the last of two boards
    gen = np.random.default_rng(L + M)
    w = gen.normal(size=(-(-N // per), NF)).astype(np.float32)
    w[::3] = gen.integers(-2, 3, w[::3].shape)
    act, score = _act(world.a, world.b, N, w, per, **world.game)
    want_act, want_score = cases.best(ALL, w, per)
    assert np.array_equal(act, want_act) and np.array_equal(score.view(np.uint32), want_score.view(np.uint32))
    assert (cases.best(ALL, w[:1], N)[0] != want_act).any()     # the rows matter
    world.read_only()


# ------------------------------------------------------------------------------------------------ 3. search
@games
def test_the_search_is_the_one_ply_kernels_composed_and_two_oracle_moves(oracle, world, L, M):
    pool, cases = world.pool, world.cases
    run = pool.running
    # composed from the one-ply entries at this game (the test above compares them with the oracle), on every state
    env, idx = _resident(pool, N, 0, REWARDS[0], **world.game)
    phi1, canonical1 = T.placement_features(env)
    after = T.afterstates(env)
    phi2, canonical2 = T.placement_features(env, after["states_a"].view(-1, 4), after["states_b"].view(-1, 4))
    env.terminate()
    assert np.array_equal(idx, ALL) and np.array_equal(_np(phi1).astype(np.int64), cases.phi)
    done1 = _np(after["done"]) != 0
    psi = _np(phi2).reshape(N, 40, 40, NF).copy()
    psi[..., 0] += _np(after["cleared"]).astype(np.int16)[:, :, None]              # n1 + n2
    distinct1 = _np(canonical1) == ARANGE[None, :]
    distinct2 = _np(canonical2).reshape(N, 40, 40) == ARANGE[None, None, :]
    got = {}
    for name, w in WEIGHTS[:3]:
        want = _m().search_choice(_np(phi1), done1, distinct1, psi, distinct2, w)
        got[name] = _search(world.a, world.b, N, w, N, L_=L, M_=M)
        _same_search(got[name], want, (L, M, name))
        assert (got[name][0][~run] == 0).all() and (got[name][1][~run] == 255).all()
        assert np.array_equal(got[name][1] == 255, ~run | done1[ALL, got[name][0]]), name
        if (L, M) == (1, 1):                                   # the search ends inside itself: the one-ply choice and score
            act, score = _act(world.a, world.b, N, w, N, **world.game)
            assert (got[name][1] == 255).all()
            assert np.array_equal(got[name][0], act) and np.array_equal(got[name][2].view(np.uint32), score.view(np.uint32)), name
        else:
            assert (got[name][1][run] != 255).sum() >= 8, name
    # two oracle moves, on the running states whose two known pieces are real ones
    if "twoply" not in world.memo:
        world.memo["twoply"] = TwoPly(oracle, cases, L, M, most=ORACLE_STATES)
    two = world.memo["twoply"]
    K = two.idx.size
    assert 8 <= K <= ORACLE_STATES
    a, b = _planes(pool.A[two.idx], pool.B[two.idx])
    sel = np.arange(K)
    for name, w in WEIGHTS[:3]:
        want = two.want(sel, w, K)
        _same_search(_search(a, b, K, w, K, L_=L, M_=M), want, (L, M, name, "oracle"))
        _same_search(tuple(x[two.idx] for x in got[name]), want, (L, M, name, "oracle, among all"))
    if (L, M) == (1, 1):
        assert two.pairs == 0 and two.done1[two.distinct1].all()
    if (L, M) == (2, 3):                                       # the second ply decides games here
        assert two.count["win2"] >= 8 and two.count["limit2"] >= 8, two.count
    world.read_only()


# ------------------------------------------------------------------------------------------------ 4. beam
# (2, 3), the classical weights at (D, W) = (3, 4): half of what the reference measures -- 16 states whose chosen path wins at ply 2
# or 3, 248 with a finished node carried into the final beam -- as test_beam_gpu's COVERAGE_FLOOR, and never under 8
BEAM_2_3_FLOOR = dict(wins_after_the_first_ply=8, carried=124)


def _oracle_states(states, depth):
    """At most 48 running states whose first `depth` known pieces are real ones: the highest moves at residues 8 and 9, the highest
    moves of all, and the rest evenly spread."""
    plies = states.plies(ALL, depth)
    real = np.ones(N, bool)
    for j in range(depth):                                     # the oracle has no piece 7
        real &= (j >= plies) | (((states.fields["window"] >> np.uint64(3 * j)) & np.uint64(7)) <= 6)
    able = np.flatnonzero(states.running & real)
    by_moves = able[np.argsort(-states.moves[able], kind="stable")]
    at_8_9 = by_moves[np.isin(states.moves[by_moves] % 10, (8, 9))]
    spread = able[np.linspace(0, able.size - 1, ORACLE_STATES).astype(np.int64)]
    idx = np.array(list(dict.fromkeys(at_8_9[:16].tolist() + by_moves[:8].tolist() + spread.tolist()))[:ORACLE_STATES])
    return idx, plies, able


@games
def test_the_beam_is_the_parents_kernels_composed_and_oracle_moves(oracle, world, L, M):
    states, run = world.states, world.states.running
    for depth, width in BEAM_SHAPES:
        for name, w in (("classical", CLASSICAL), ("small integers", SMALL)):
            want = world.reference(name, w, depth, width)
            got = _beam(world.a, world.b, N, w, N, depth, width, **world.game)
            _same_beam(got, (want["action"], want["plan"], want["score"]), (L, M, name, depth, width))
            assert (got[0][~run] == 0).all() and (got[1][~run] == 255).all()
            assert (got[1][run, 0] == got[0][run]).all() and (got[0][run] < 40).all()
            assert ((got[1] != 255).sum(axis=1) <= states.plies(ALL, depth)).all()
    # the C oracle's moves and the host features at depth 3, width 4
    depth, width = 3, 4
    idx, plies, able = _oracle_states(states, depth)
    assert 8 <= idx.size <= ORACLE_STATES and np.unique(idx).size == idx.size
    top = set(np.sort(states.moves[able])[-2:].tolist())
    assert top <= set(states.moves[idx].tolist())
    if M > 9:
        at = states.moves[idx][np.isin(states.moves[idx] % 10, (8, 9))]
        assert {8, 9} <= set((at % 10).tolist()) and at.max() >= M - 10 and at.size >= 8
    a, b = _planes(states.A[idx], states.B[idx])
    for name, w in (("classical", CLASSICAL), ("small integers", SMALL)):
        got = _beam(a, b, idx.size, w, idx.size, depth, width, **world.game)
        for t, i in enumerate(idx):
            action, plan, score = oracle_beam(oracle, states.fields, i, int(plies[i]), w, depth, width, **world.game)
            assert (int(got[0][t]), got[1][t].tolist()) == (action, plan), (L, M, name, i, got[1][t].tolist(), plan)
            assert got[2][t].view(np.uint32) == np.float32(score).view(np.uint32), (L, M, name, i, got[2][t], score)
    world.read_only()


def test_at_1_1_a_beam_of_any_depth_is_the_depth_one_beam(oracle):
    world = _world(oracle, 1, 1)
    run = world.states.running
    for name, w in (("classical", CLASSICAL), ("small integers", SMALL), ("random", RANDOM)):
        act, score = _act(world.a, world.b, N, w, N, **world.game)
        for depth, width in ((2, 34), (12, 2), (2, 1), (12, 64)):
            one = _beam(world.a, world.b, N, w, N, 1, width, **world.game)
            got = _beam(world.a, world.b, N, w, N, depth, width, **world.game)
            assert np.array_equal(got[0], one[0]) and np.array_equal(got[2].view(np.uint32), one[2].view(np.uint32)), (name, depth)
            assert np.array_equal(got[0], act) and np.array_equal(got[2].view(np.uint32), score.view(np.uint32)), (name, depth)
            assert (got[1][:, 1:] == 255).all() and np.array_equal(got[1][:, 0], np.where(run, act, 255)), (name, depth)


def test_at_250_254_the_known_pieces_come_from_moves_in_the_hundreds(oracle):
    world = _world(oracle, 250, 254)
    states, run = world.states, world.states.running
    plies = states.plies(ALL, 12)
    high = run & (states.moves >= 128)
    print(f"effective depths at D = 12: all running {np.unique(plies[run]).tolist()}, at moves >= 128 {np.unique(plies[high]).tolist()}")
    assert np.unique(plies[run]).size >= 6 and np.unique(plies[high]).size >= 6
    assert np.array_equal(plies[run], np.minimum(12, 12 - states.moves[run] % 10)) and {3, 4} <= set(plies[high].tolist())
    want = world.reference("classical", CLASSICAL, 12, 2)
    length = (want["plan"] != 255).sum(axis=1)
    assert (length <= plies).all() and (length[run] >= 1).all()
    # a plan stops short of the effective depth only where the game ends: the boards far from every end run their depth out
    far = run & (states.moves <= 200) & (np.asarray(states.fields["lines"]) <= 200)
    print(f"plan lengths: {np.unique(length[run]).tolist()}; {int(far.sum())} states far from L and M, "
          f"{int((length[far] == plies[far]).sum())} of them planned to their depth")
    got = _beam(world.a, world.b, N, CLASSICAL, N, 12, 2, **world.game)
    _same_beam(got, (want["action"], want["plan"], want["score"]), "250 / 254, 12 x 2")


def test_at_2_3_the_beam_wins_after_its_first_ply_and_carries_finished_nodes(oracle):
    world = _world(oracle, 2, 3)
    narrow, deep = world.reference("classical", CLASSICAL, 3, 4), world.reference("classical", CLASSICAL, 12, 2)
    count = dict(wins_after_the_first_ply=int((narrow["wins"] & (narrow["plan"][:, 1] != 255)).sum()),
                 carried=int(narrow["carried"].sum()),
                 wins_after_the_first_ply_deep=int((deep["wins"] & (deep["plan"][:, 1] != 255)).sum()),
                 carried_deep=int(deep["carried"].sum()), wins=int(narrow["wins"].sum()))
    print("coverage of the reference's outcomes at (2, 3):", count)
    for name, least in BEAM_2_3_FLOOR.items():
        assert count[name] >= max(least, 8), (name, count)


# ------------------------------------------------------------------------------------------------ 5. the Python surface
@pytest.mark.parametrize("L,M", [(1, 1), (250, 254)])
def test_the_python_surface_hands_over_the_environments_game(world, L, M):
    pool = world.pool
    params, w = REWARDS[1], CLASSICAL
    env, idx = _resident(pool, N, 0, params, **world.game)
    assert (env.L, env.M) == (L, M) and np.array_equal(idx, ALL)

    def differs(x, y):
        return any(not np.array_equal(np.asarray(p).view(np.uint8), np.asarray(q).view(np.uint8)) for p, q in zip(x, y))

    # afterstates
    out = T.afterstates(env)
    names = ("states_a", "states_b", "reward", "done", "cleared", "canonical")
    got = tuple(_np(out[k]) for k in names)
    here, other = (_run(pool.A, pool.B, params, **game) for game in (world.game, dict(L=10, M=40)))
    keys = ("out_a", "out_b", "reward", "done", "cleared", "canonical")
    assert not differs(got, tuple(here[k] for k in keys)) and differs(got, tuple(other[k] for k in keys))
    # features
    feats, canon = T.placement_features(env)
    got = (_np(feats).astype(np.int64), _np(canon))
    assert not differs(got, _features(world.a, world.b, N, L, M)) and differs(got, _features(world.a, world.b, N, 10, 40))
    # one ply, two plies
    score = torch.empty(N, dtype=torch.float32, device=DEV)
    second = torch.full((N,), 77, dtype=torch.uint8, device=DEV)
    got = (_np(T.HeuristicPolicy(env, w).act(score=score)), _np(score))
    assert not differs(got, _act(world.a, world.b, N, w, N, **world.game)) and differs(got, _act(world.a, world.b, N, w, N))
    got = (_np(T.HeuristicPolicy(env, w, depth=2).act(score=score, second=second)), _np(second), _np(score))
    assert not differs(got, _search(world.a, world.b, N, w, N, L_=L, M_=M)) and differs(got, _search(world.a, world.b, N, w, N))
    # the beam
    plan = torch.full((N, 3), 77, dtype=torch.uint8, device=DEV)
    got = (_np(T.BeamPolicy(env, w, 3, 4).act(plan=plan, score=score)), _np(plan), _np(score))
    assert not differs(got, _beam(world.a, world.b, N, w, N, 3, 4, **world.game)) and differs(got, _beam(world.a, world.b, N, w, N, 3, 4))
    a, b = env.raw_planes()                                    # nothing above touched the environment's planes
    assert np.array_equal(_np(a).view(np.uint32), pool.A) and np.array_equal(_np(b).view(np.uint32), pool.B)
    env.terminate()
    world.read_only()
