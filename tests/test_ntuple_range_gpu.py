"""The n-tuple family on one MI355X over the whole game range and at the clamps of the counter index

    k = 64 min(max(L - lines, 0), 15) + min(max(M - moves, 0), 63)          (counter_index in csrc/learn/tpl_ntuple.h).

The sibling n-tuple files play L = 10 / M = 40, where neither `min` fires and `lines`, `moves` stay below 64; their helpers take the game
as keyword arguments and are used here as they are, buffers framed by canaries, inputs asserted read only.  The states are
test_ntuple_range_cpu.py's (whose CPU tests assert what they cover), five sets:

    1_1, 2_3, 250_254   the 320 states of test_placement_range_cpu.range_pool: the ends of the range; at (250, 254) both counters use
                        their high bits (`moves` two nibbles in A.y and A.w, `lines` in bits 20..27 of B.z under window bits 32..35)
                        and both clamps are live;
    play                256 boards of the game (16, 64), fresh and after a few oracle moves: the smallest game past both clamps;
    edge                128 states at (20, 100) with 15..19 lines and 63..65 moves left: moves that cross a clamp edge.

Forms: "2x4", "3x3", "2x4+3x3" plain; the same three staged, eight distinct random blocks under test_ntuple_stage_gpu's MOVES_MAP and
WILD_MAP; "feat"; "3x3+feat" -- eleven in all.

  1. COUNTER TABLES, a check that does not go through the mirror: a table that is zero but for  k << 16  in counter entry k (staged:
     (8 k + stage) << 16 in the block of `stage`), one part of a sum at a time.  V of a running board is then the integer that names
     the entry read, and must be 64 min(L - lines, 15) + min(M - moves, 63) of the decoded fields, on every state and afterstate of
     every set; with reward (0, 0, 0) and gamma = 1 the score of act, search and beam is the entry of the leaf reached by playing the
     returned actions on the C oracle, and act's score is the largest entry among the oracle's afterstates.
  2. VALUE: bit for bit the mirror's under a table over the whole int32 range, on every state and all 40 afterstates; finished: 0.
  3. ACT: action, score, afterstate planes and value are the mirror's arg-max over the oracle's afterstates (test_ntuple_gpu.Expected
     at the game) at epsilon 0 and 0.25; at (1, 1) the score is the reward alone.
  4. SEARCH: the one-ply kernels composed on every state, and two oracle moves (test_ntuple_search_cpu.TwoMoves) on 48 states of
     every set; at (1, 1) `second` is 255 everywhere and action and score are act's.
  5. BEAM: test_ntuple_beam_gpu.compose at the game at (D, W) = (2, 34), (3, 4), (11, 2); depth 1 is act, (2, 34) is search; at
     (250, 254) the effective depth 11 - moves mod 10 at moves in the hundreds, read off the plan; on the edge set (11, 64) on 32
     states with windows of real pieces.
  6. UPDATES: tpl_ntuple_update[_shaped], _update_trace[_shaped|_staged|_feature], _update_coherent[_shaped] leave the mirror's bytes
     at (250, 254) and on the edge set -- n = 255, 257 drawn with repetition; rings of 4 slots whose ages 0 and 1 are an afterstate and
     its root, so that they straddle the clamp edges (15 | 16 lines left, 63 | 64 moves left); horizon 1 and 4, symmetric off and on;
     the entry at k = 1023 takes many boards' steps; permuted boards leave the same bytes; at (1, 1) a finished age 0 adds nothing.
  7. The Python surface hands the environment's L and M to every entry; one learner of each kind leaves the mirror's table.

The oracle's coverage of the sets is in test_ntuple_range_cpu.py's docstring.  The two-move references play 48 states a set: 6,575
(a, b) pairs at (2, 3) with 41 wins and 4,434 limit losses on the second ply, 18,476 at (250, 254), 26,501 on the (16, 64) boards and
20,774 on the edge set; none at (1, 1), where all 1,125 first moves end the game.  At (250, 254) 207 running boards have moves >= 100
and effective depths 2..11; 110 to 125 of them plan to their depth, the others' plans end with the game.

Two mutants of counter_index, built from a scratch copy and never committed, were run against this file (401 tests; the cases at
(1, 1) and (2, 3), which no clamp reaches, pass under both):
  * clamped at 16 and at 64 instead of 15 and 63: 279 of 399 fail (the learner test was left out, its table has no canary frame) --
    every case of parts 1 to 6 on the three sets past the clamps, and the Python surface;
  * moves left masked with `& 63` instead of clamped: 190 fail -- counter tables and value on all three sets, act and the oracle-played
    leaves at (250, 254) and on the edge set, search at (250, 254), every update.  The beam cases pass under it: their reference takes V
    from tpl_ntuple_value, so they hold the search to the value kernel, and parts 1 and 2 hold that to the rule.
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
import test_ntuple_beam_gpu as BE
import test_ntuple_coherent_gpu as CO
import test_ntuple_feature_gpu as FE
import test_ntuple_gpu as G
import test_ntuple_search_gpu as SE
import test_ntuple_shape_gpu as SH
import test_ntuple_stage_gpu as ST
import test_ntuple_trace_gpu as TR
from test_afterstates_gpu import _assert_against_the_oracle, _resident, _run
from test_learn_range_gpu import _check, _lib, _stream
from test_learner_gpu import _np
from test_ntuple_coherent_cpu import coherence_by_class
from test_ntuple_range_cpu import COUNTERS, EDGE_GAME, PLAY_GAME, edge_pool, play_pool
from test_ntuple_search_cpu import TwoMoves
from test_placement_range_cpu import range_pool

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARAMS, GAMMA = G.PARAMS, G.GAMMA
ZERO = (0.0, 0.0, 0.0)
ARANGE = np.arange(40)
SUM = ST.SUM
GAME_OF = {"1_1": (1, 1), "2_3": (2, 3), "250_254": (250, 254), "play": PLAY_GAME, "edge": EDGE_GAME}
SETS = list(GAME_OF)
PAST_THE_CLAMPS = ["250_254", "play", "edge"]
MAPS = {"moves": ST.MOVES_MAP, "wild": ST.WILD_MAP}
BEAM_SHAPES = [(2, 34), (3, 4), (11, 2)]
DRAW = dict(seed=0xDEADBEEFCAFEF00D, step=(1 << 40) + 3)
f32 = np.float32


def _m():
    return T._learn_lib


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the forms
class Form:
    """One of the eleven forms: its tables and its entries behind one face -- the helpers of test_ntuple_stage_gpu (plain and staged
    window forms) and test_ntuple_feature_gpu at a given game."""

    def __init__(self, name, stage_map=None):
        self.name, self.map_name, self.staged = name, stage_map, stage_map is not None
        self.feature = name in FE.FORMS
        self.map = MAPS[stage_map] if self.staged else None
        self.entries = FE.ENTRIES[name] if self.feature else ST.FORMS[name]
        self.bases = [base for _, base in COUNTERS[name]]      # entry of counter 0 of every part, within a block
        self.id = name + (f" staged, {stage_map} map" if self.staged else "")
        self._tables = {}

    def __repr__(self):
        return self.id

    def table(self, span=1 << 20):
        """A random table of the form (staged: eight distinct blocks and the map), once per span."""
        if span not in self._tables:
            seed = 7000 + len(self.id) + 31 * len(self.name)
            if self.staged:
                self._tables[span] = ST._blocks(seed, self.name, self.map, span=span)
            else:
                self._tables[span] = np.random.default_rng(seed).integers(-span, span + 1, self.entries).astype(np.int32)
        return self._tables[span]

    def counter_table(self, part):
        """Zero but for the counters of `part`: entry k holds k << 16 (staged: (8 k + stage) << 16 in the block of `stage`)."""
        k = np.arange(1024, dtype=np.int64)
        base = self.bases[part]
        if not self.staged:
            t = np.zeros(self.entries, np.int32)
            t[base:base + 1024] = k << 16
            return t
        t = np.zeros(8 * self.entries + 1024, np.int32)
        for stage in range(8):
            t[stage * self.entries + base:stage * self.entries + base + 1024] = (8 * k + stage) << 16
        t[-1024:] = self.map
        return t

    def entry_read(self, L, M, lines, moves):
        """What V under a counter table must be for running boards: the rule, from the decoded fields."""
        lines, moves = np.asarray(lines, np.int64), np.asarray(moves, np.int64)
        k = 64 * np.minimum(np.maximum(L - lines, 0), 15) + np.minimum(np.maximum(M - moves, 0), 63)
        return 8 * k + (self.map[k].astype(np.int64) & 7) if self.staged else k

    def value(self, A, B, table, L, M):
        if self.feature:
            return FE._value(A, B, table, self.name, L=L, M=M)
        return ST._value(A, B, table, self.name, staged=self.staged, L=L, M=M)["value"]

    def policy(self, depth, A, B, table, L, M, **kw):
        if self.feature:
            return FE._policy(depth, A, B, table, self.name, L=L, M=M, **kw)
        return ST._policy(depth, A, B, table, self.name, staged=self.staged, L=L, M=M, **kw)

    def beam(self, A, B, table, depth, width, L, M, **kw):
        if self.feature:
            return FE._beam(A, B, table, depth, width, self.name, L=L, M=M, **kw)
        return ST._beam(A, B, table, depth, width, self.name, staged=self.staged, L=L, M=M, **kw)


FORMS = ([Form(name) for name in ST.FORMS] + [Form(name, m) for name in ST.FORMS for m in MAPS] + [Form(name) for name in FE.FORMS])
BY_ID = {form.id: form for form in FORMS}
assert len(FORMS) == 11 and len(BY_ID) == 11
forms = pytest.mark.parametrize("form", FORMS, ids=lambda form: form.id.replace(" ", "_").replace(",", ""))
sets = pytest.mark.parametrize("name", SETS)


# ------------------------------------------------------------------------------------------------ the sets
class World:
    """One set: the states and the oracle's outcomes (shared with the CPU file), their afterstates from tpl_afterstates at the game --
    held to the oracle here, bit for bit --, the decoded fields of both and the mirror's arg-max over the oracle's afterstates."""

    def __init__(self, oracle, name):
        L, M = self.L, self.M = GAME_OF[name]
        self.name, self.game = name, dict(L=L, M=M)
        self.pool = edge_pool(oracle) if name == "edge" else play_pool(oracle) if name == "play" else range_pool(oracle, L, M)
        p = self.pool
        n = self.n = p.n
        self.A, self.B, self.run = p.A, p.B, p.running
        self.f = G._fields(p.A, p.B)
        self.expected = G.Expected(p, L=L, M=M)
        ply = _run(p.A, p.B, PARAMS, L=L, M=M)                 # canaries and read-only inputs are asserted there
        _assert_against_the_oracle(p, np.arange(n), ply, PARAMS, name)
        assert np.array_equal(ply["out_a"], self.expected.A) and np.array_equal(ply["out_b"], self.expected.B), name
        self.after_A, self.after_B = (np.ascontiguousarray(ply[k].reshape(-1, 4)) for k in ("out_a", "out_b"))
        self.after_f = G._fields(self.after_A, self.after_B)
        self.reward, self.done, self.distinct = ply["reward"], ply["done"] != 0, ply["canonical"] == ARANGE[None, :]
        assert np.array_equal(self.distinct, self.expected.distinct) and np.array_equal(self.done, p.done)
        # roots, then afterstates: what the update tests draw from
        self.all_A, self.all_B = np.concatenate([self.A, self.after_A]), np.concatenate([self.B, self.after_B])
        self.all_f = {k: np.concatenate([self.f[k], self.after_f[k]]) for k in self.f}
        self.memo, self._env = {}, None

    @property
    def env(self):
        """Any environment of the game with the reward parameters: T.afterstates reads L, M and the rewards from it."""
        if self._env is None:
            self._env = T.BatchedTetris(self.L, self.M, 8, device=DEV, seed=9, reward=PARAMS)
        return self._env

    def close(self):
        if self._env is not None:
            self._env.terminate()
            self._env = None

    def plies(self, depth, A=None, B=None):
        return ST._plies(self.A if A is None else A, self.B if B is None else B, depth)

    def two(self, oracle):
        """Two oracle moves of 48 evenly spread running states whose next piece is a real one, once."""
        if "two" not in self.memo:
            f = self.pool.fields
            nxt = ((f["window"] >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
            idx = np.flatnonzero(self.run & (nxt <= 6))
            idx = idx[np.unique(np.linspace(0, idx.size - 1, min(48, idx.size)).astype(np.int64))]
            two = TwoMoves(oracle, f["rows"][idx], np.asarray(f["lines"])[idx], np.asarray(f["moves"])[idx], f["window"][idx],
                           self.L, self.M)
            two.idx = idx
            print(f"{self.name}: {idx.size} states, {int(two.played.sum())} (a, b) pairs; the oracle's outcomes: {two.count}")
            self.memo["two"] = two
        return self.memo["two"]

    def follow(self, oracle, i, plan):
        """State i after the actions of `plan` (up to the first 255 or the end of the game) on the C oracle: (lines, moves, ended);
        None where a piece it needs is 7, which the oracle has not."""
        f = self.pool.fields
        pieces = [(int(f["window"][i]) >> (3 * e)) & 7 for e in range(12)]
        g = oracle.Game(self.L, self.M, rows=f["rows"][i], pieces=pieces, lines_cleared=int(f["lines"][i]), moves_used=int(f["moves"][i]))
        for e, a in enumerate(plan):
            if a == 255 or g.state != 0:
                break
            if pieces[e] > 6:
                return None
            g.move(int(a) // 10, int(a) % 10)
        return g.lines_cleared, g.moves_used, g.state != 0


_WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_worlds():
    yield
    for w in _WORLDS.values():
        w.close()
    _WORLDS.clear()


def _world(oracle, name):
    if name not in _WORLDS:
        _WORLDS[name] = World(oracle, name)
    return _WORLDS[name]


@pytest.fixture
def world(oracle, name):
    return _world(oracle, name)


# ------------------------------------------------------------------------------------------------ 1. counter tables
@forms
@sets
def test_under_a_counter_table_the_value_names_the_entry_the_rule_reads(world, name, form):
    L, M = world.L, world.M
    for part in range(len(form.bases)):
        table = form.counter_table(part)
        for what, A, B, f in (("states", world.A, world.B, world.f), ("afterstates", world.after_A, world.after_B, world.after_f)):
            got = form.value(A, B, table, L, M)
            want = np.where(f["state"] == 0, form.entry_read(L, M, f["lines"], f["moves"]), 0).astype(np.float32)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, form.id, part, what, bad.size,
                                   [(int(f["lines"][i]), int(f["moves"][i]), float(got[i]), float(want[i])) for i in bad[:5]])
            assert (_bits(got)[f["state"] != 0] == 0).all()
    if name in PAST_THE_CLAMPS:                                # both sides of both clamps were read
        left, mleft = L - world.all_f["lines"][world.all_f["state"] == 0], M - world.all_f["moves"][world.all_f["state"] == 0]
        assert min((left > 15).sum(), (left <= 15).sum(), (mleft > 63).sum(), (mleft <= 63).sum()) >= 8


@forms
@pytest.mark.parametrize("name", PAST_THE_CLAMPS)
def test_with_no_reward_and_gamma_one_the_score_names_the_entry_of_the_chosen_leaf(oracle, world, name, form):
    L, M, run, pool = world.L, world.M, world.run, world.pool
    at = np.arange(world.n)
    kw = dict(gamma=1.0, params=ZERO)
    for part in range(len(form.bases)):
        table = form.counter_table(part)
        # one ply, against all 40 oracle afterstates: the largest entry among the distinct placements, the lowest of them
        leaf = np.where(pool.done, 0, form.entry_read(L, M, pool.lines, pool.moves)).astype(np.float32)
        masked = np.where(world.distinct, leaf, -np.inf)
        best = masked.max(axis=1)
        one = form.policy(1, world.A, world.B, table, L, M, **kw)
        bad = np.flatnonzero(run & (one["score"] != best))
        assert bad.size == 0, (name, form.id, part, bad[:5].tolist(), one["score"][bad[:5]].tolist(), best[bad[:5]].tolist())
        assert np.array_equal(one["action"][run], np.argmax(masked == best[:, None], axis=1)[run])
        assert np.array_equal(one["value"][run], leaf[at, one["action"]][run]) and (one["score"][~run] == 0).all()
        # any depth: the entry of the leaf that the returned actions reach on the oracle
        two = form.policy(2, world.A, world.B, table, L, M, **kw)
        plans = [("act", one["action"][:, None], one["score"]), ("search", np.stack([two["action"], two["second"]], axis=1), two["score"])]
        for depth, width in ((3, 4), (11, 2)):
            beam = form.beam(world.A, world.B, table, depth, width, L, M, **kw)
            plans.append((f"beam {depth} x {width}", beam["plan"], beam["score"]))
        for what, plan, score in plans:
            checked = crossed = 0
            for i in np.flatnonzero(run):
                end = world.follow(oracle, i, plan[i])
                if end is None:
                    continue
                want = 0 if end[2] else int(form.entry_read(L, M, end[0], end[1]))
                assert float(score[i]) == want, (name, form.id, part, what, int(i), plan[i].tolist(), float(score[i]), want, end)
                checked += 1
                crossed += int(not end[2] and ((L - pool.fields["lines"][i] > 15) != (L - end[0] > 15)
                                               or (M - pool.fields["moves"][i] > 63) != (M - end[1] > 63)))
            assert checked >= 32, (what, checked)
            assert crossed >= 4 or name == "250_254", (name, what, crossed)     # root and leaf on two sides of a clamp


# ------------------------------------------------------------------------------------------------ 2. value
@forms
@sets
def test_value_is_the_mirror_bit_for_bit_on_every_state_and_all_its_afterstates(world, name, form):
    L, M = world.L, world.M
    table = form.table(span=(1 << 31) - 1)                     # the whole int32 range: the rounding is at the conversion
    for what, A, B, f in (("states", world.A, world.B, world.f), ("afterstates", world.after_A, world.after_B, world.after_f)):
        got = form.value(A, B, table, L, M)
        want = _m().ntuple_value(table, f["rows"], f["cur"], L, M, f["lines"], f["moves"], f["state"])
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (name, form.id, what, bad.size, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        done = f["state"] != 0
        assert (_bits(got)[done] == 0).all() and (got[~done] != 0).sum() >= (~done).sum() - 2
    assert world.after_A.shape[0] == 40 * world.n


def test_the_2x4_entries_of_the_first_n_tuple_files_at_250_254_with_each_optional_output_left_out_once(oracle):
    """tpl_ntuple_value, _act, _search and _beam through test_ntuple_gpu's, test_ntuple_search_gpu's and test_ntuple_beam_gpu's own
    helpers at the game: the unshaped entries, which the forms above do not call, and every optional output passed as NULL once."""
    name = "250_254"
    world = _world(oracle, name)
    L, M, A, B, run = world.L, world.M, world.A, world.B, world.run
    form = BY_ID["2x4"]
    table = form.table()
    all_ = np.arange(world.n)
    assert form.name == "2x4" and table.shape[0] == G.ENTRIES
    got = G._value(world.after_A, world.after_B, table, **world.game)
    assert np.array_equal(_bits(got), _bits(G._mirror_value(table, world.after_f, **world.game)))
    # act
    full = G._act(A, B, table, **world.game)
    G._assert_choice(full, world.expected.choice(table, all_), name)
    for skip in ("score", "after", "value"):
        other = G._act(A, B, table, skip=(skip,), **world.game)
        assert set(other) == set(full) - ({"after_a", "after_b"} if skip == "after" else {skip})
        assert all(np.array_equal(v.view(np.uint8), full[k].view(np.uint8)) for k, v in other.items()), skip
    assert np.array_equal(G._act(A, B, table, skip=("score", "after", "value"), **world.game)["action"], full["action"])
    assert (full["action"] != G._act(A, B, table)["action"]).any()               # the game is not ignored
    # search
    composed = SE.Composed(A, B, table, GAMMA, **world.game)
    full = SE._search(A, B, table, **world.game)
    SE._same(full, composed.want(), name)
    for skip in ("second", "score", "after", "value"):
        other = SE._search(A, B, table, skip=(skip,), **world.game)
        assert set(other) == set(full) - ({"after_a", "after_b"} if skip == "after" else {skip})
        assert all(np.array_equal(v.view(np.uint8), full[k].view(np.uint8)) for k, v in other.items()), skip
    assert np.array_equal(SE._search(A, B, table, skip=("second", "score", "after", "value"), **world.game)["action"], full["action"])
    # beam
    for shape in ("2x4", "3x3"):
        t = Form(shape).table()
        want = BE.compose(world.env, t, A, B, world.plies(3), 3, 4, **world.game)
        full = BE._beam(A, B, t, 3, 4, **world.game)
        BE._same(full, dict(action=want["action"], plan=want["plan"], score=want["score"]), (name, shape))
        for skip in ("plan", "score", "after"):
            other = BE._beam(A, B, t, 3, 4, skip=(skip,), **world.game)
            assert set(other) == set(full) - ({"after_a", "after_b"} if skip == "after" else {skip})
            assert all(np.array_equal(v.view(np.uint8), full[k].view(np.uint8)) for k, v in other.items()), skip
        assert np.array_equal(BE._beam(A, B, t, 3, 4, skip=("plan", "score", "after"), **world.game)["action"], full["action"])
        assert (full["action"][~run] == 0).all() and (full["plan"][~run] == 255).all()


# ------------------------------------------------------------------------------------------------ 3. act
@forms
@sets
def test_act_is_the_mirror_arg_max_over_the_oracle_afterstates_at_both_epsilons(world, name, form):
    L, M, A, B, run, pool = world.L, world.M, world.A, world.B, world.run, world.pool
    table = form.table()
    all_, at = np.arange(world.n), np.arange(world.n)
    greedy = world.expected.choice(table, all_)
    got = form.policy(1, A, B, table, L, M)
    G._assert_choice(got, greedy, (name, form.id, 0.0))
    assert (got["action"][~run] == 0).all() and (_bits(got["score"])[~run] == 0).all() and (_bits(got["value"])[~run] == 0).all()
    assert np.array_equal(got["after_a"][~run], A[~run]) and np.array_equal(got["after_b"][~run], B[~run])
    ended = pool.done[at, got["action"]] & run                # chosen moves that end the game: the score is the bare reward
    assert (_bits(got["value"])[ended] == 0).all()
    assert np.array_equal(_bits(got["score"])[ended], _bits(world.expected.reward[at, got["action"]])[ended])
    want = world.expected.choice(table, all_, epsilon=0.25, **DRAW)
    explorer = form.policy(1, A, B, table, L, M, epsilon=0.25, **DRAW)
    G._assert_choice(explorer, want, (name, form.id, 0.25))
    assert want[5].sum() >= 16 and not want[5][~run].any() and (explorer["action"] != got["action"]).any()
    if name == "1_1":                                          # every placement ends the game: the best distinct reward, the lowest of them
        assert ended[run].all()
        masked = np.where(world.distinct, world.expected.reward, -np.inf)
        assert np.array_equal(got["action"][run], np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)[run])
        assert np.array_equal(_bits(got["score"])[run], _bits(masked.max(axis=1).astype(np.float32))[run])
    else:
        assert (~ended & run).sum() >= (32 if name in PAST_THE_CLAMPS else 1) and (got["value"][~ended & run] != 0).all()


# ------------------------------------------------------------------------------------------------ 4. search
def _composed(world, form, table, gamma=GAMMA):
    """tpl_ntuple_search's rule put together as test_ntuple_search_gpu.Composed does it, for any form: Q(a) = r1 + gamma * score' and
    second(a) = action' with r1 from tpl_afterstates and (score', action') from the form's one-ply entry over the 40 n afterstates;
    after and value are the afterstate of the action played and the form's value entry of it."""
    n, L, M = world.n, world.L, world.M
    ply = form.policy(1, world.after_A, world.after_B, table, L, M, gamma=gamma)
    value = form.value(world.after_A, world.after_B, table, L, M).reshape(n, 40)
    with np.errstate(invalid="ignore", over="ignore"):
        Q = np.where(world.done, world.reward, world.reward + f32(gamma) * ply["score"].reshape(n, 40)).astype(np.float32)
    second = np.where(world.done, 255, ply["action"].reshape(n, 40)).astype(np.uint8)
    masked = np.where(world.distinct, Q, -np.inf)
    greedy = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)
    at = np.arange(n)
    return dict(action=greedy.astype(np.uint8), second=second[at, greedy], score=Q[at, greedy],
                after_a=world.after_A.reshape(n, 40, 4)[at, greedy], after_b=world.after_B.reshape(n, 40, 4)[at, greedy],
                value=value[at, greedy])


@forms
@sets
def test_the_search_is_the_one_ply_kernels_composed_and_two_oracle_moves(oracle, world, name, form):
    L, M, A, B, run = world.L, world.M, world.A, world.B, world.run
    table = form.table()
    got = form.policy(2, A, B, table, L, M)
    SE._same(got, _composed(world, form, table), (name, form.id, "composed"))
    assert (got["action"][~run] == 0).all() and (got["second"][~run] == 255).all() and (_bits(got["score"])[~run] == 0).all()
    assert np.array_equal(got["second"] == 255, ~run | world.done[np.arange(world.n), got["action"]])
    # two oracle moves, on the running states whose two known pieces are real ones
    two = world.two(oracle)
    K = two.idx.size
    assert K == 48
    action, second, score, _, _ = _m().ntuple_search_choice(*two.inputs(table, PARAMS), GAMMA)
    want = dict(action=action, second=second, score=score)
    SE._same({k: v[two.idx] for k, v in got.items()}, want, (name, form.id, "oracle, among all"))
    sub = form.policy(2, np.ascontiguousarray(A[two.idx]), np.ascontiguousarray(B[two.idx]), table, L, M)
    SE._same(sub, want, (name, form.id, "oracle"))
    if name == "1_1":                                          # the search ends inside itself: the one-ply choice and score
        one = form.policy(1, A, B, table, L, M)
        assert (got["second"] == 255).all() and two.played.sum() == 0
        assert np.array_equal(got["action"], one["action"]) and np.array_equal(_bits(got["score"]), _bits(one["score"]))
    else:
        assert (got["second"][run] != 255).sum() >= 32 and two.played.sum() >= 1000
    if name == "2_3":                                          # the second ply decides games here
        assert two.count["win2"] >= 8 and two.count["limit2"] >= 8, two.count


# ------------------------------------------------------------------------------------------------ 5. beam
@forms
@sets
def test_the_beam_is_the_reference_composed_ply_by_ply_at_the_game(world, name, form):
    L, M, A, B, run = world.L, world.M, world.A, world.B, world.run
    table = form.table()
    for depth, width in BEAM_SHAPES:
        plies = world.plies(depth)
        want = BE.compose(world.env, table, A, B, plies, depth, width, **world.game)
        got = form.beam(A, B, table, depth, width, L, M)
        BE._same(got, dict(action=want["action"], plan=want["plan"], score=want["score"]), (name, form.id, depth, width))
        length = (got["plan"] != 255).sum(axis=1)
        assert (got["action"][~run] == 0).all() and (got["plan"][~run] == 255).all() and (_bits(got["score"])[~run] == 0).all()
        assert (got["plan"][run, 0] == got["action"][run]).all() and (got["action"][run] < 40).all()
        assert (length <= plies).all() and (length[run] >= 1).all()
        assert (got["plan"][np.arange(depth)[None, :] >= length[:, None]] == 255).all()        # behind the end: nothing
        if name == "1_1":
            assert (length[run] == 1).all()
    # depth 1 is act (action, score, after); depth 2 at width 34 is search (action, score)
    one, two = form.policy(1, A, B, table, L, M), form.policy(2, A, B, table, L, M)
    got = form.beam(A, B, table, 1, 4, L, M)
    BE._same(got, {k: one[k] for k in ("action", "score", "after_a", "after_b")}, (name, form.id, "depth 1"))
    assert (got["plan"][:, 0] == np.where(run, one["action"], 255)).all()
    got = form.beam(A, B, table, 2, 34, L, M)
    BE._same(got, {k: two[k] for k in ("action", "score", "after_a", "after_b")}, (name, form.id, "depth 2, width 34"))
    assert ((got["plan"][:, 1] == 255) == (two["second"] == 255)).all()


def test_at_250_254_the_effective_depth_is_taken_at_moves_in_the_hundreds(oracle, name="250_254"):
    world = _world(oracle, name)
    moves, run = world.f["moves"], world.run
    plies = world.plies(11)
    high = run & (moves >= 100)
    print(f"effective depths at D = 11: all running {np.unique(plies[run]).tolist()}, at moves >= 100 {np.unique(plies[high]).tolist()}")
    assert np.array_equal(plies[run], np.minimum(11, 11 - moves[run] % 10)) and np.unique(plies[high]).size >= 6 and high.sum() >= 64
    for form in (BY_ID["2x4"], BY_ID["3x3 staged, wild map"], BY_ID["feat"]):
        got = form.beam(world.A, world.B, form.table(), 11, 2, world.L, world.M)
        length = (got["plan"] != 255).sum(axis=1)
        assert (length <= plies).all() and (got["plan"][np.arange(11)[None, :] >= length[:, None]] == 255).all()
        # a plan stops short of the effective depth only where the game ends on the way
        full = high & (length == plies)
        short = np.flatnonzero(high & (length < plies))
        print(f"{form.id}: {int(full.sum())} of {int(high.sum())} boards at moves >= 100 planned to their depth "
              f"(lengths {np.unique(length[high]).tolist()})")
        assert full.sum() >= 8 and {2, 3} <= set(plies[full].tolist())
        for i in short:
            end = world.follow(oracle, i, got["plan"][i])
            assert end is None or end[2], (form.id, int(i), got["plan"][i].tolist(), end)


@forms
def test_on_the_edge_set_a_wide_deep_beam_on_windows_of_real_pieces(oracle, form, name="edge"):
    world = _world(oracle, name)
    n, depth, width = 32, 11, 64
    f = {k: np.asarray(v)[:n] for k, v in world.pool.fields.items()}
    gen = np.random.default_rng(64)
    pieces = gen.integers(0, 7, (n, 12))
    pieces[:, 0] = (f["window"] & np.uint64(7)).astype(np.int64)
    window = sum(pieces[:, e].astype(np.uint64) << np.uint64(3 * e) for e in range(12))
    states = BE.States(dict(f, window=window))
    plies = world.plies(depth, states.A, states.B)
    assert set(plies.tolist()) == {4, 5, 6} and states.running.all()                 # moves 35, 36, 37: every path crosses 64 | 63
    table = form.table()
    want = BE.compose(world.env, table, states.A, states.B, plies, depth, width, **world.game)
    got = form.beam(states.A, states.B, table, depth, width, world.L, world.M)
    BE._same(got, dict(action=want["action"], plan=want["plan"], score=want["score"]), (form.id, depth, width))
    assert ((got["plan"] != 255).sum(axis=1) == plies).sum() >= 16


# ------------------------------------------------------------------------------------------------ 6. updates
def _counter_hits(world, form, f, live):
    """How many of the live boards of `f` add to the counter entry k = 1023, and where that entry lies for each part."""
    L, M = world.L, world.M
    k = 64 * np.minimum(np.maximum(L - f["lines"], 0), 15) + np.minimum(np.maximum(M - f["moves"], 0), 63)
    block = int(form.map[1023]) & 7 if form.staged else 0
    return int((live & (k == 1023)).sum()), [block * form.entries + base + 1023 for base in form.bases]


@pytest.mark.parametrize("n", [255, 257])
@pytest.mark.parametrize("name", ["250_254", "edge"])
def test_the_plain_update_leaves_the_mirror_bytes_where_most_adds_meet_on_one_clamped_counter(world, name, n):
    L, M = world.L, world.M
    gen = np.random.default_rng(1000 * L + n)
    total, roots = world.all_A.shape[0], world.n
    picks = np.where(gen.random(n) < 0.5, gen.integers(0, roots, n), gen.integers(0, total, n))      # with repetition
    assert np.unique(picks).size < n
    A, B = np.ascontiguousarray(world.all_A[picks]), np.ascontiguousarray(world.all_B[picks])
    f = {k: v[picks] for k, v in world.all_f.items()}
    rate = 3000.0
    error = TR._errors(gen, n, rate)
    live = (f["state"] == 0) & (_m().ntuple_steps(error, rate) != 0)
    cases = [("tpl_ntuple_update", Form("2x4"), lambda start: G._update(A, B, start, error, rate, **world.game))]
    cases += [(f"tpl_ntuple_update_shaped, shape {s}", Form(shape), lambda start, s=s: SH._trace3(A, B, 0, 1, start, error, rate, 0.0, 0,
                                                                                                  shape=s, planes=True, **world.game))
              for s, shape in enumerate(("2x4", "3x3"))]
    for what, form, update in cases:
        start = SH._full_range(n, form.entries)
        want = _m().ntuple_update(start.copy(), f["rows"], f["cur"], L, M, f["lines"], f["moves"], f["state"], error, rate)
        got = update(start)
        assert np.array_equal(got, want), (name, what)
        hits, (entry,) = _counter_hits(world, form, f, live)
        assert hits >= 32 and want[entry] != start[entry], (name, what, hits)
        order = gen.permutation(n)                             # the boards in another order: the same bytes
        A2, B2, e2 = np.ascontiguousarray(A[order]), np.ascontiguousarray(B[order]), np.ascontiguousarray(error[order])
        if what == "tpl_ntuple_update":
            assert np.array_equal(G._update(A2, B2, start, e2, rate, **world.game), got)
            other = G._update(A, B, start, error, rate)        # L = 10 / M = 40: other counters
            assert not np.array_equal(other, got)


def _straddling_ring(world, gen, n):
    """A ring of 4 slots (head 1: the ages lie in slots 1, 0, 3, 2) for n boards, as indices into world.all_*: age 0 an afterstate and
    age 1 its root -- first every pair the oracle takes across a clamp edge, then random pairs --, ages 2 and 3 random states."""
    pool, L, M, roots = world.pool, world.L, world.M, world.n
    f = pool.fields
    left0, mleft0 = (L - np.asarray(f["lines"]))[:, None], (M - np.asarray(f["moves"]))[:, None]
    on = (pool.state == 0) & pool.running[:, None]
    cross_l = np.argwhere(on & (left0 > 15) & (L - pool.lines <= 15))
    cross_m = np.argwhere(on & (mleft0 > 63) & (M - pool.moves <= 63))
    pairs = np.concatenate([cross_l[:n // 4], cross_m[gen.permutation(len(cross_m))[:n // 4]]]) if len(cross_m) else cross_l[:n // 4]
    rest = n - len(pairs)
    running = np.flatnonzero(pool.running)
    pairs = np.concatenate([pairs.reshape(-1, 2), np.stack([running[gen.integers(0, running.size, rest)], gen.integers(0, 40, rest)], axis=1)])
    pairs = pairs[gen.permutation(n)]
    ages = np.stack([roots + 40 * pairs[:, 0] + pairs[:, 1], pairs[:, 0], gen.integers(0, world.all_A.shape[0], n),
                     gen.integers(0, roots, n)])
    return ages, dict(lines=int(len(cross_l[:n // 4])), moves=int(min(len(cross_m), n // 4)))


# (the entry, the form whose table it updates): all six trace and coherent entries, the staged one in each of its three forms
TRACE_ENTRIES = [("tpl_ntuple_update_trace", Form("2x4")), ("tpl_ntuple_update_trace_shaped", Form("3x3")),
                 ("tpl_ntuple_update_trace_staged", Form("2x4", "moves")), ("tpl_ntuple_update_trace_staged", Form("3x3", "wild")),
                 ("tpl_ntuple_update_trace_staged", Form(SUM, "moves")), ("tpl_ntuple_update_trace_feature", Form("feat")),
                 ("tpl_ntuple_update_coherent", Form("2x4")), ("tpl_ntuple_update_coherent_shaped", Form("3x3"))]


def _launch(entry, form, world, A, B, head, horizon, start, error, rate, decay, symmetric, coherence=None):
    """One call of a trace or coherent entry through the sibling files' framed helpers at the game: the table, or (table, sums)."""
    game = world.game
    if entry == "tpl_ntuple_update_trace":
        return TR._trace(A, B, head, horizon, start, error, rate, decay, symmetric, game=(world.L, world.M))
    if entry == "tpl_ntuple_update_trace_shaped":
        return SH._trace3(A, B, head, horizon, start, error, rate, decay, symmetric, shape=ST.FORM_IDS[form.name], **game)
    if entry == "tpl_ntuple_update_trace_staged":
        return ST._trace(A, B, head, horizon, start, error, rate, decay, symmetric, form.name, **game)
    if entry == "tpl_ntuple_update_trace_feature":
        return FE._update(A, B, head, horizon, start, error, rate, decay, symmetric, **game)
    if entry == "tpl_ntuple_update_coherent":
        return CO._coherent(A, B, head, horizon, start, coherence, error, rate, decay, symmetric, game=(world.L, world.M))
    assert entry == "tpl_ntuple_update_coherent_shaped"
    return SH._trace3(A, B, head, horizon, start, error, rate, decay, symmetric, shape=ST.FORM_IDS[form.name], coherence=coherence, **game)


def _start_of(form, seed):
    if form.staged:
        return ST._blocks(seed, form.name, form.map, span=(1 << 31) - 1)
    return FE._start(seed) if form.feature else SH._full_range(seed, form.entries)


def _coherence_of(form, seed):
    """A coherence buffer of the form's shape with every class of pair in it."""
    classes, _ = coherence_by_class(seed)
    return np.ascontiguousarray(np.resize(classes.reshape(-1), 2 * form.entries).reshape(form.entries, 2))


@pytest.mark.parametrize("horizon,symmetric", [(1, 0), (1, 1), (4, 0), (4, 1)])
@pytest.mark.parametrize("entry,form", TRACE_ENTRIES, ids=[f"{e[11:]}-{f.id.replace(' ', '_').replace(',', '')}" for e, f in TRACE_ENTRIES])
@pytest.mark.parametrize("name", ["250_254", "edge"])
def test_trace_and_coherent_updates_leave_the_mirror_bytes_in_a_ring_that_straddles_the_clamps(world, name, entry, form, horizon, symmetric):
    L, M, n, slots, head = world.L, world.M, 257, 4, 1
    gen = np.random.default_rng(100 * horizon + symmetric + L)
    ages, crossing = _straddling_ring(world, gen, n)
    slot_of = [(head - k) % slots for k in range(slots)]
    ring = np.empty((slots, n), np.int64)
    for k, s in enumerate(slot_of):
        ring[s] = ages[k]
    A, B = np.ascontiguousarray(world.all_A[ring]), np.ascontiguousarray(world.all_B[ring])
    fields = [TR._age(world.all_f, ages[k]) for k in range(horizon)]
    f0, f1 = ({k: v[ages[j]] for k, v in world.all_f.items()} for j in (0, 1))
    # the ring does straddle: age 0 at 15 lines left under age 1 at 16 or more, 63 moves left under 64 or more, both running
    both = (f0["state"] == 0) & (f1["state"] == 0)
    over_l = both & (L - f0["lines"] <= 15) & (L - f1["lines"] > 15)
    over_m = both & (M - f0["moves"] <= 63) & (M - f1["moves"] > 63)
    if name == "edge":
        assert crossing["lines"] >= 32 and over_l.sum() >= 32 and over_m.sum() >= 32, (crossing, int(over_l.sum()), int(over_m.sum()))
        assert ((L - f0["lines"] == 15) & (L - f1["lines"] == 16) & both).sum() >= 4
        assert ((M - f0["moves"] == 63) & (M - f1["moves"] == 64) & both).sum() >= 16
    else:
        assert (both & (L - f0["lines"] <= 15)).sum() >= 8 and (both & (L - f0["lines"] > 15)).sum() >= 8
        assert (both & (M - f0["moves"] <= 63)).sum() >= 8 and (both & (M - f0["moves"] > 63)).sum() >= 8
    rate, decay = 3000.0, 0.8
    error = TR._errors(gen, n, rate)
    start = _start_of(form, 10 * horizon + symmetric)
    coherent = "coherent" in entry
    if coherent:
        sums = _coherence_of(form, horizon + symmetric)
        got, got_sums = _launch(entry, form, world, A, B, head, horizon, start, error, rate, decay, symmetric, coherence=sums)
        want, want_sums = _m().ntuple_update_coherent(start.copy(), sums.copy(), fields, L, M, error, rate, decay, bool(symmetric))
        assert np.array_equal(got_sums, want_sums), (name, entry, form.id)
        assert (got_sums != sums).any()
    else:
        got = _launch(entry, form, world, A, B, head, horizon, start, error, rate, decay, symmetric)
        want = _m().ntuple_update_trace(start.copy(), fields, L, M, error, rate, decay, bool(symmetric))
    assert np.array_equal(got, want), (name, entry, form.id, int((got != want).sum()), np.flatnonzero(got != want)[:5].tolist())
    if form.staged:
        assert np.array_equal(got[-1024:], form.map)           # the map is read, never written
    # the one clamped counter entry took many boards' steps, and the mirror says it moved
    live = (f0["state"] == 0) & (_m().ntuple_steps(error, rate) != 0)
    hits, entries = _counter_hits(world, form, f0, live)
    assert hits >= (32 if name == "edge" else 16), hits
    moved = want_sums[:, 1] != sums[:, 1] if coherent else want != start
    assert all(moved[e] for e in entries), (name, entry, form.id, entries)
    # the boards in another order: the same bytes
    order = gen.permutation(n)
    A2, B2, e2 = np.ascontiguousarray(A[:, order]), np.ascontiguousarray(B[:, order]), np.ascontiguousarray(error[order])
    if coherent:
        again, again_sums = _launch(entry, form, world, A2, B2, head, horizon, start, e2, rate, decay, symmetric, coherence=sums)
        assert np.array_equal(again_sums, got_sums)
    else:
        again = _launch(entry, form, world, A2, B2, head, horizon, start, e2, rate, decay, symmetric)
    assert np.array_equal(again, got)


@pytest.mark.parametrize("entry,form", TRACE_ENTRIES, ids=[f"{e[11:]}-{f.id.replace(' ', '_').replace(',', '')}" for e, f in TRACE_ENTRIES])
def test_at_1_1_a_ring_whose_younger_ages_are_finished_adds_nothing_for_them(oracle, entry, form, name="1_1"):
    world = _world(oracle, name)
    L, M, n, slots, head, horizon = 1, 1, 257, 4, 1, 4
    gen = np.random.default_rng(11)
    running = np.flatnonzero(world.run)
    root = running[gen.integers(0, running.size, n)]
    after = world.n + 40 * root + gen.integers(0, 40, n)
    assert (world.all_f["state"][after] != 0).all() and (world.all_f["state"][root] == 0).all()     # every placement ends this game
    rate, decay = 3000.0, 0.8
    error = TR._errors(gen, n, rate)
    start = _start_of(form, 3)
    sums = _coherence_of(form, 4) if "coherent" in entry else None

    def launch(ages):
        ring = np.empty((slots, n), np.int64)
        for k in range(slots):
            ring[(head - k) % slots] = ages[k]
        out = _launch(entry, form, world, np.ascontiguousarray(world.all_A[ring]), np.ascontiguousarray(world.all_B[ring]), head, horizon,
                      start, error, rate, decay, 1, coherence=sums)
        return out if sums is not None else (out, None)

    # the afterstates are the newest: the trace of every board is cut at age 0, the running roots behind them add nothing
    got, got_sums = launch([after, root, root, root])
    assert np.array_equal(got, start) and (sums is None or np.array_equal(got_sums, sums))
    # the roots are the newest, finished states behind them: age 0 alone adds -- the bytes of the same call at horizon 1
    got, got_sums = launch([root, after, root, root])
    fields = [TR._age(world.all_f, root)]
    if sums is None:
        want = _m().ntuple_update_trace(start.copy(), fields, L, M, error, rate, decay, True)
    else:
        want, want_sums = _m().ntuple_update_coherent(start.copy(), sums.copy(), fields, L, M, error, rate, decay, True)
        assert np.array_equal(got_sums, want_sums)
    assert np.array_equal(got, want) and (want != start).any()


# ------------------------------------------------------------------------------------------------ 7. the Python surface, one learner
def _differs(x, y):
    return any(not np.array_equal(np.asarray(x[k]).view(np.uint8), np.asarray(y[k]).view(np.uint8)) for k in y)


def test_the_python_surface_hands_over_the_environments_game(oracle, name="play"):
    world = _world(oracle, name)
    L, M, A, B, n = world.L, world.M, world.A, world.B, world.n
    env, idx = _resident(world.pool, n, 0, PARAMS, **world.game)
    assert (env.L, env.M) == (16, 64) and np.array_equal(idx, np.arange(n))
    host = Form("2x4").table()
    table = torch.from_numpy(host).to(DEV)
    # the value
    got = dict(value=_np(T.ntuple_value(env, table)))
    assert not _differs(got, dict(value=G._value(A, B, host, **world.game))) and _differs(got, dict(value=G._value(A, B, host)))
    # one ply, two plies
    score, value = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    second = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
    planes = tuple(torch.empty((n, 4), dtype=torch.int32, device=DEV) for _ in range(2))
    kw = dict(epsilon=0.25, seed=9, step=4)

    def outputs(action, **more):
        return dict(action=_np(action), score=_np(score), value=_np(value), after_a=_np(planes[0]).view(np.uint32),
                    after_b=_np(planes[1]).view(np.uint32), **more)

    action = T.NTuplePolicy(env, table, gamma=GAMMA, epsilon=0.25, seed=9).act(score=score, after=planes, value=value, step=4)
    got = outputs(action)
    assert not _differs(got, G._act(A, B, host, **kw, **world.game)) and _differs(got, G._act(A, B, host, **kw))
    action = T.NTuplePolicy(env, table, gamma=GAMMA, epsilon=0.25, seed=9, depth=2).act(score=score, after=planes, value=value, step=4,
                                                                                       second=second)
    got = outputs(action, second=_np(second))
    assert not _differs(got, SE._search(A, B, host, **kw, **world.game)) and _differs(got, SE._search(A, B, host, **kw))
    # the beam, under a staged table
    staged = BY_ID["3x3 staged, wild map"]
    dev_staged = torch.from_numpy(staged.table()).to(DEV)
    plan = torch.full((n, 3), 77, dtype=torch.uint8, device=DEV)
    action = T.NTupleBeamPolicy(env, dev_staged, 3, 4, gamma=GAMMA).act(score=score, plan=plan, after=planes)
    got = dict(action=_np(action), plan=_np(plan), score=_np(score), after_a=_np(planes[0]).view(np.uint32), after_b=_np(planes[1]).view(np.uint32))
    assert not _differs(got, staged.beam(A, B, staged.table(), 3, 4, L, M)) and _differs(got, staged.beam(A, B, staged.table(), 3, 4, 10, 40))
    a, b = env.raw_planes()                                    # nothing above touched the environment's planes
    assert np.array_equal(_np(a).view(np.uint32), A) and np.array_equal(_np(b).view(np.uint32), B)
    env.terminate()


def _carved_env(n, seed=3):
    L, M = PLAY_GAME
    return T.BatchedTetris(L, M, n, device=DEV, seed=seed, auto_reset=True, reward=PARAMS,
                           config_pool=T.generate_configs(L, M, 64, seed=1000 * L + M))


def _played_by_hand(env, table, steps, gamma, L, M):
    """NTupleLearner.evaluate's loop on tpl_ntuple_act with the game GIVEN: the tallies and the planes the environment is left with."""
    n = env.num_envs
    pa, pb = T.lookahead._state_ptrs(env)
    action, done = (torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(2))
    reward = torch.empty(n, dtype=torch.float32, device=DEV)
    after = [torch.zeros((n, 4), dtype=torch.int32, device=DEV) for _ in range(2)]
    episodes, wins = 0, 0
    env.reset()
    for _ in range(steps):
        _check(_lib().tpl_ntuple_act(pa, pb, n, L, M, *env.reward_params, gamma, table.data_ptr(), 0.0, 0, 0, action.data_ptr(), None,
                                     after[0].data_ptr(), after[1].data_ptr(), None, _stream()))
        env.step_into(action, reward, done)
        episodes += int(done.sum())
        wins += int((((after[1][:, 1] >> 28) & 3) == 1).sum())
    a, b = env.raw_planes()
    return dict(episodes=episodes, wins=wins, win_rate=wins / max(episodes, 1)), _np(a).copy(), _np(b).copy()


def test_the_learners_evaluation_plays_the_environments_game():
    n, steps = 256, 24
    env = _carved_env(n)
    learner = T.NTupleLearner(env, gamma=GAMMA, rate=8.0, epsilon=0.1, seed=5)
    learner.table.copy_(torch.from_numpy(Form("2x4").table()).to(DEV))
    got = learner.evaluate(steps)
    planes = tuple(_np(x).copy() for x in env.raw_planes())
    assert learner.evaluate(steps) == got                      # from a full reset: the same games
    here, a, b = _played_by_hand(env, learner.table, steps, GAMMA, env.L, env.M)
    assert (env.L, env.M) == PLAY_GAME and here == got and np.array_equal(a, planes[0]) and np.array_equal(b, planes[1])
    other, a, b = _played_by_hand(env, learner.table, steps, GAMMA, 10, 40)
    print(f"evaluate({steps}) at (16, 64): {got}; the same loop with L = 10 / M = 40 given to the entry: {other}")
    assert not (np.array_equal(a, planes[0]) and np.array_equal(b, planes[1]))
    env.terminate()


@pytest.mark.parametrize("kind", ["2x4", "3x3 staged"])
def test_one_learner_with_traces_leaves_the_mirror_table_after_every_step_at_16_64(kind):
    """test_ntuple_trace_gpu's loop with the game passed through: after every train(1) the table is the mirror's update of the ring
    read back, with the learner's own errors."""
    n, steps, horizon = 256, 6, 4
    shape = kind.split()[0]
    gen = np.random.default_rng(len(kind))
    plain = gen.integers(-(1 << 12), (1 << 12) + 1, ST.FORMS[shape]).astype(np.int32)
    plain = torch.from_numpy(plain + plain[_m().ntuple_mirror_permutation(shape)])                # a symmetric start
    more = dict(stage_map=T.ntuple_stage_map(*PLAY_GAME, moves=4)) if "staged" in kind else {}
    kw = dict(gamma=1.0, rate=16.0, epsilon=0.25, seed=5, lam=0.8, horizon=horizon, symmetric=True, shape=shape, start=plain.to(DEV), **more)

    def run(check):
        env = _carved_env(n)
        env.reset()
        learner = T.NTupleLearner(env, **kw)
        assert (env.L, env.M) == PLAY_GAME and learner.slots == horizon + 1 and learner.policy.staged == ("staged" in kind)
        table = _np(learner.table).copy()
        first, changed, stages = learner.table.clone(), 0, set()
        for step in range(steps):
            learner.train(1)
            if not check:
                continue
            head = (learner._head - 1) % learner.slots         # the head the update was made with
            ring = [_np(r).view(np.uint32) for r in learner._ring]
            ages = [G._fields(ring[0][(head - k) % learner.slots], ring[1][(head - k) % learner.slots]) for k in range(horizon)]
            previous = table.copy()
            _m().ntuple_update_trace(table, [TR._age(f) for f in ages], env.L, env.M, _np(learner._error), 16.0, np.float32(0.8), True)
            assert np.array_equal(_np(learner.table), table), (kind, step)
            changed += int(not np.array_equal(table, previous))
            live = ages[0]["state"] == 0
            if more:
                stages |= set(_m().ntuple_stages_of(table, env.L, env.M, ages[0]["lines"][live], ages[0]["moves"][live]).tolist())
        if check:
            assert changed >= 4 and T.ntuple_is_symmetric(learner.table) is True
            assert not more or stages == {3}                   # the kept afterstates have 58 .. 63 moves left: the top bucket
        out = learner.table.clone()
        env.terminate()
        assert not torch.equal(out, first)
        return out

    run(check=True)
    a, b = run(check=False), run(check=False)
    assert torch.equal(a, b)                                   # one seed: the same bytes
