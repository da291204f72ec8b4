"""CPU-side checks of the two-ply n-tuple policy (include/tpl_learn.h's rule, tpl_ntuple_search in csrc/learn/ntuple.hip,
_learn_lib.ntuple_search_choice, ntuple.py's depth=2):

  * ntuple_search_choice on hand-built inputs: a first move that ends the game, ties in a and in b falling to the lowest index,
    the gamma products rounded once, a finished board;
  * on a few dozen states the same function, fed from two moves of the C oracle and _learn_lib.ntuple_value, agrees with a plain
    Python double loop that does one float32 operation at a time;
  * the header declares the entry, the library exports it, ntuple_search_kernel is in tools/kernel_resources.sh's output exactly
    once, without scratch and within 128 VGPRs; every refusal comes back as a status without a GPU;
  * depth=3 raises ValueError, and so does second= at depth 1.

TwoMoves -- every distinct (a, b) of given states played as two oracle moves -- is shared with tests/test_ntuple_search_gpu.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tetris_piclim as T
from test_heuristic_cpu import _Env

f32 = np.float32
ENTRIES = 8 * 153 * 256 + 1024
ARANGE = np.arange(40)


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ two oracle moves
class TwoMoves:
    """Every distinct first placement a of K running states and -- where the game goes on -- every distinct placement b of the
    next piece, played as two moves of the C oracle: rows cleared, end states and the boards, from which rewards and values are
    made for any reward parameters and any table.  The states need a real next piece (0..6): the oracle has no piece 7."""

    def __init__(self, oracle, rows, lines, moves, window, L, M):
        K = self.K = len(rows)
        self.L, self.M = L, M
        window = np.asarray(window, np.uint64)
        cur, nxt, third = (((window >> np.uint64(3 * e)) & np.uint64(7)).astype(np.int64) for e in range(3))
        assert K and nxt.max() <= 6
        self.cur, self.nxt, self.third = cur, nxt, third
        self.distinct1 = _m().canonical_actions(cur[:, None], ARANGE[None, :]) == ARANGE[None, :]
        self.distinct2 = _m().canonical_actions(nxt[:, None], ARANGE[None, :]) == ARANGE[None, :]
        self.n1, self.state1 = np.zeros((K, 40), np.int64), np.zeros((K, 40), np.int64)
        self.top1 = np.zeros((K, 40), bool)
        self.n2, self.state2 = np.zeros((K, 40, 40), np.int64), np.zeros((K, 40, 40), np.int64)
        self.top2 = np.zeros((K, 40, 40), bool)
        self.rows2 = np.zeros((K, 40, 40, 20), np.uint16)
        self.lines2, self.moves2 = np.zeros((K, 40, 40), np.int64), np.zeros((K, 40, 40), np.int64)
        self.played = np.zeros((K, 40, 40), bool)              # the (a, b) the oracle played
        for k in range(K):
            pieces = [int(cur[k]), int(nxt[k])]
            for a in np.flatnonzero(self.distinct1[k]):
                g1 = oracle.Game(L, M, rows=rows[k], pieces=pieces, lines_cleared=int(lines[k]), moves_used=int(moves[k]))
                ret1 = g1.move(int(a) // 10, int(a) % 10)
                self.n1[k, a], self.state1[k, a], self.top1[k, a] = max(ret1, 0), g1.state, ret1 < 0
                if g1.state != 0:
                    continue
                rows1, lines1, moves1 = g1.rows.tolist(), g1.lines_cleared, g1.moves_used
                for b in np.flatnonzero(self.distinct2[k]):
                    g = oracle.Game(L, M, rows=rows1, pieces=pieces[1:], lines_cleared=lines1, moves_used=moves1)
                    ret2 = g.move(int(b) // 10, int(b) % 10)
                    self.n2[k, a, b], self.state2[k, a, b], self.top2[k, a, b] = max(ret2, 0), g.state, ret2 < 0
                    self.rows2[k, a, b], self.lines2[k, a, b], self.moves2[k, a, b] = g.rows, g.lines_cleared, g.moves_used
                    self.played[k, a, b] = True
        self.done1 = self.state1 != 0
        self.done2 = self.state2 != 0
        d1 = self.distinct1
        self.count = dict(first_move_ends=int((self.done1 & d1).sum()), win2=int((self.played & (self.state2 == 1)).sum()),
                          topout2=int((self.played & self.top2).sum()),
                          limit2=int((self.played & (self.state2 == 2) & ~self.top2).sum()),
                          both_clear=int((self.played & (self.n1[:, :, None] > 0) & (self.n2 > 0)).sum()))
        self._values = {}

    @staticmethod
    def _reward(n, state, params):
        """step_reward's rule: one rounded multiply, at most one rounded add (numpy float32 operations round once each)."""
        r_line, r_win, r_lose = (f32(x) for x in params)
        r = r_line * n.astype(np.float32)
        r = np.where(state == 1, r + r_win, r)
        return np.where(state >= 2, r + r_lose, r).astype(np.float32)

    def values(self, table):
        """V(s_ab) f32 [K, 40, 40] under `table`, 0 where (a, b) was not played or ended the game; kept per table."""
        key = hash(table.tobytes())
        if key not in self._values:
            at = np.nonzero(self.played)
            v = np.zeros(self.played.shape, np.float32)
            v[at] = _m().ntuple_value(table, self.rows2[at], self.third[at[0]], self.L, self.M, self.lines2[at], self.moves2[at],
                                      self.state2[at])
            self._values[key] = v
        return self._values[key]

    def inputs(self, table, params):
        """ntuple_search_choice's arguments but gamma, for all K states."""
        return (self._reward(self.n1, self.state1, params), self.done1, self.distinct1,
                self._reward(self.n2, self.state2, params), self.done2, self.values(table), self.distinct2)


# ------------------------------------------------------------------------------------------------ 1. hand cases
def _blank(K=1):
    z2, z3 = np.zeros((K, 40), np.float32), np.zeros((K, 40, 40), np.float32)
    return dict(reward1=z2.copy(), done1=np.zeros((K, 40), bool), distinct1=np.ones((K, 40), bool), reward2=z3.copy(),
                done2=np.zeros((K, 40, 40), bool), value2=z3.copy(), distinct2=np.ones((K, 40), bool))


def _choice(c, gamma, running=None):
    return _m().ntuple_search_choice(c["reward1"], c["done1"], c["distinct1"], c["reward2"], c["done2"], c["value2"], c["distinct2"],
                                     gamma, running)


def test_a_first_move_that_ends_the_game_scores_its_reward_alone():
    c = _blank()
    c["value2"][:] = 100.0                                     # never read behind a move that ended the game
    c["reward2"][:] = 1.0
    c["done1"][0, 3], c["reward1"][0, 3] = True, 200.0
    action, second, score, Q, seconds = _choice(c, 1.0)
    assert action.dtype == np.uint8 and second.dtype == np.uint8 and score.dtype == np.float32 and Q.shape == (1, 40)
    assert (int(action[0]), int(second[0]), float(score[0])) == (3, 255, 200.0)
    assert float(Q[0, 4]) == 101.0 and seconds[0, 4] == 0 and seconds[0, 3] == 255
    c["reward1"][0, 3] = 50.0                                  # now the search behind every other move is worth more
    action, second, score, _, _ = _choice(c, 1.0)
    assert (int(action[0]), int(second[0]), float(score[0])) == (0, 0, 101.0)
    # a second move that ends the game scores its reward alone, too
    c["done2"][0, 7, 9], c["reward2"][0, 7, 9], c["value2"][0, 7, 9] = True, 150.0, 1e6
    action, second, score, _, _ = _choice(c, 1.0)
    assert (int(action[0]), int(second[0]), float(score[0])) == (7, 9, 150.0)


def test_ties_in_a_and_in_b_fall_to_the_lowest_distinct_index():
    c = _blank(2)
    c["distinct1"][:, :2] = False                              # a = 0, 1 are aliases; b = 0 .. 4 are
    c["distinct2"][:, :5] = False
    c["reward2"][:] = 1.0
    c["reward2"][:, :, :5] = 9.0                               # an alias never wins, whatever it would score
    c["reward1"][:, :2] = 9.0
    action, second, score, Q, _ = _choice(c, 0.5)
    assert action.tolist() == [2, 2] and second.tolist() == [5, 5] and score.tolist() == [0.5, 0.5]
    # -0 and +0 tie in both plies, and the score keeps the winner's own bits
    c = _blank()
    c["reward2"][0, :, 0], c["reward2"][0, :, 1] = -0.0, 0.0
    c["reward2"][0, :, 2:] = -1.0
    c["done2"][:] = True                                       # the bare rewards: -0 + gamma * 0 would be +0
    c["reward1"][0, 0] = -0.0
    action, second, score, Q, _ = _choice(c, 1.0)
    assert (int(action[0]), int(second[0])) == (0, 0) and score[0] == 0.0 and np.signbit(score[0])        # -0 + 1 * -0
    # a later index wins only when it is strictly better
    c["reward2"][0, 6, 30] = f32(1e-30)
    action, second, score, _, _ = _choice(c, 1.0)
    assert (int(action[0]), int(second[0])) == (6, 30) and score[0] == f32(1e-30)


def test_the_gamma_products_are_rounded_once_and_never_fused():
    # 1 + 0.1f * 9: the fused form ends in another bit (test_heuristic_cpu's case), in the second ply and in the first
    g = f32(0.1)
    stepwise = f32(f32(1.0) + f32(g * f32(9.0)))
    fused = f32(np.float64(g) * 9.0 + 1.0)
    assert stepwise.view(np.uint32) != fused.view(np.uint32)
    c = _blank()
    c["reward2"][:] = -5.0
    c["reward2"][0, 5, 7], c["value2"][0, 5, 7] = 1.0, 9.0
    action, second, score, Q, _ = _choice(c, 0.1)
    want = f32(f32(0.0) + f32(g * stepwise))
    assert (int(action[0]), int(second[0])) == (5, 7) and score[0].view(np.uint32) == want.view(np.uint32)
    # the outer product: r1 + gamma * W with W = 9 exactly
    c = _blank()
    c["reward2"][:] = -5.0
    c["reward2"][0, 11, 2], c["reward1"][0, 11] = 9.0, 1.0
    c["done2"][0, 11, 2] = True
    action, second, score, _, _ = _choice(c, 0.1)
    assert (int(action[0]), int(second[0])) == (11, 2) and score[0].view(np.uint32) == stepwise.view(np.uint32)
    # gamma itself is taken as a float32
    c["reward2"][0, 11, 2] = 3.0
    assert _choice(c, 0.1)[2][0] == f32(f32(1.0) + f32(g * f32(3.0)))


def test_a_finished_board_gets_action_0_second_255_and_score_0():
    c = _blank(3)
    c["reward1"][:] = 4.0
    c["reward2"][:] = 2.0
    running = np.array([True, False, True])
    action, second, score, Q, seconds = _choice(c, 1.0, running)
    assert action.tolist() == [0, 0, 0] and second.tolist() == [0, 255, 0] and score.tolist() == [6.0, 0.0, 6.0]
    assert (Q[1] == 0).all() and (seconds[1] == 255).all()
    for bad in (dict(reward1=c["reward1"][:, :39]), dict(reward2=c["reward2"][:, :, :39]), dict(distinct2=c["distinct2"][:2])):
        with pytest.raises(ValueError):
            _choice(dict(c, **bad), 1.0)


# ------------------------------------------------------------------------------------------------ 2. against a plain double loop
def _states(gen, K, L, M):
    """K running states: ragged boards of every height (tall ones top out), prepared wells, counters up to one short of L and M."""
    rows = np.zeros((K, 20), np.uint16)
    for k in range(K):
        top = (4, 9, 14, 19)[k % 4]
        for x, h in enumerate(gen.integers(max(top - 6, 0), top + 1, 10)):
            for j in range(int(h)):
                if gen.random() > 0.15:
                    rows[k, 19 - j] |= np.uint16(1 << x)
        if k % 3 == 0:                                         # two wells: an upright I in each clears two rows, one after the other
            w1, w2 = (int(w) for w in gen.choice(10, 2, replace=False))
            rows[k] = 0
            rows[k, 18:] = np.uint16(0x3FF & ~(1 << w1))
            rows[k, 16:18] = np.uint16(0x3FF & ~(1 << w1) & ~(1 << w2))
    lines = np.where(np.arange(K) % 5 == 0, L - 1, gen.integers(0, L - 1, K))
    moves = np.where(np.arange(K) % 4 == 1, M - 2, np.where(np.arange(K) % 7 == 2, M - 1, gen.integers(0, M - 2, K)))
    window = gen.integers(0, 7, (K, 3))
    window[::3, :2] = 0                                        # I then I: the prepared rows clear
    window = (window[:, 0] | (window[:, 1] << 3) | (window[:, 2] << 6)).astype(np.uint64)
    return rows, lines, moves, window


def _double_loop(two, k, table, params, gamma):
    """The rule as the header words it for state k, one float32 operation at a time: (action, second, score)."""
    g = f32(gamma)
    r_line, r_win, r_lose = (f32(x) for x in params)
    value = two.values(table)                                  # _learn_lib.ntuple_value of the oracle's boards

    def reward(n, state):
        r = f32(r_line * f32(n))
        if state == 1:
            r = f32(r + r_win)
        if state >= 2:
            r = f32(r + r_lose)
        return r

    best = None
    for a in range(40):
        if not two.distinct1[k, a]:
            continue
        r1 = reward(two.n1[k, a], two.state1[k, a])
        if two.state1[k, a] != 0:
            Q, second = r1, 255
        else:
            W = second = None
            for b in range(40):
                if not two.distinct2[k, b]:
                    continue
                q = reward(two.n2[k, a, b], two.state2[k, a, b])
                if two.state2[k, a, b] == 0:
                    q = f32(q + f32(g * value[k, a, b]))
                if W is None or q > W:                         # strict: the lowest b stays
                    W, second = q, b
            Q = f32(r1 + f32(g * W))
        if best is None or Q > best[2]:
            best = (a, second, Q)
    return best


def test_the_mirror_fed_from_two_oracle_moves_is_the_plain_double_loop(oracle):
    L, M, K = 10, 40, 36
    gen = np.random.default_rng(36)
    rows, lines, moves, window = _states(gen, K, L, M)
    two = TwoMoves(oracle, rows, lines, moves, window, L, M)
    print(f"{K} states, {int(two.played.sum())} (a, b) pairs; the oracle's outcomes: {two.count}")
    assert min(two.count.values()) >= 5, two.count
    tables = (gen.integers(-(1 << 20), (1 << 20) + 1, ENTRIES).astype(np.int32),
              (np.where(gen.random(ENTRIES) < 0.1, gen.integers(-1, 2, ENTRIES), 0).astype(np.int32) << np.int32(12)))      # ties
    went_on = ended = 0
    for table, params, gamma in ((tables[0], (0.1, 0.5, -0.25), 0.99), (tables[0], (1.0, 10.0, -1.0), 1.0),
                                 (tables[1], (0.0, 1.0, 0.0), 1.0)):
        action, second, score, Q, _ = _m().ntuple_search_choice(*two.inputs(table, params), gamma)
        for k in range(K):
            a, b, s = _double_loop(two, k, table, params, gamma)
            assert (int(action[k]), int(second[k])) == (a, b), (k, action[k], second[k], a, b)
            assert score[k].view(np.uint32) == s.view(np.uint32), (k, score[k], s)
            assert two.distinct1[k, a] and (b == 255) == bool(two.done1[k, a]) and (b == 255 or two.distinct2[k, b])
        went_on += int((second != 255).sum())
        ended += int((second == 255).sum())
    assert went_on >= 20 and ended >= 5, (went_on, ended)


# ------------------------------------------------------------------------------------------------ 3. symbols, resources, refusals
def test_the_header_declares_the_search_entry_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text))
    assert "tpl_ntuple_search" in declared and "tpl_ntuple_search" in _m().LEARN_SYMBOLS and declared == set(_m().LEARN_SYMBOLS)
    names = lambda entry: [a.split()[-1].lstrip("*") for a in re.search(rf"int {entry}\((.*?)\);", text, flags=re.S).group(1).split(",")]
    act = names("tpl_ntuple_act")
    assert names("tpl_ntuple_search") == act[:act.index("action") + 1] + ["second"] + act[act.index("action") + 1:]
    lib = ctypes.CDLL(_m().build_library())
    assert hasattr(lib, "tpl_ntuple_search")
    assert "ntuple_search_kernel" in open(os.path.join(os.path.dirname(_m()._UNITS[0]), "ntuple.hip")).read()


def test_the_search_kernel_uses_no_scratch_and_at_most_128_vgprs():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    mine = [r for r in rows if "ntuple_search_kernel" in r[-1]]
    assert len(mine) == 1, [r[-1] for r in rows]
    assert mine[0][mine[0].index("scratch") - 1] == "0", mine
    assert int(mine[0][mine[0].index("vgpr") - 1]) <= 128, mine
    assert len([r for r in rows if "ntuple_act_kernel" in r[-1]]) == 1         # neither name is part of the other


def test_every_refusal_of_the_search_entry_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused
    name = b"tpl_ntuple_search"
    nan, inf = float("nan"), float("inf")

    def search(a=fake, b=fake, n=4, L=2, M=2, gamma=0.99, table=fake, epsilon=0.1, action=fake, second=fake, score=fake,
               after_a=fake, after_b=fake, value=fake):
        return lib.tpl_ntuple_search(a, b, n, L, M, 0.0, 1.0, 0.0, gamma, table, epsilon, 1, 2, action, second, score, after_a,
                                     after_b, value, None)

    limit = -(-(1 << 31) // 40)
    assert search(a=None) < 0 and b"null" in err() and name in err()
    assert search(b=None) < 0 and b"null" in err() and name in err()
    for n in (0, -1):
        assert search(n=n) < 0 and b"positive" in err() and name in err(), n
    for n in (limit, 1 << 40):
        assert search(n=n) < 0 and b"2^31" in err() and name in err(), n
    for plane in ("a", "b"):
        assert search(**{plane: fake + 8}) < 0 and b"planes must be 16-byte aligned" in err() and name in err(), plane
    for L, M in ((0, 2), (2, 256), (251, 2), (255, 2), (2, 255), (2, 0)):
        assert search(L=L, M=M) < 0 and b"L and M" in err() and name in err(), (L, M)
    assert search(table=None) < 0 and b"null" in err() and b"table" in err() and name in err()
    for off in (4, 8, 12):
        assert search(table=fake + off) < 0 and b"table must be 16-byte aligned" in err() and name in err(), off
    assert search(action=None) < 0 and b"null" in err() and b"action" in err() and name in err()
    assert search(after_a=None) < 0 and b"go together" in err() and name in err()
    assert search(after_b=None) < 0 and b"go together" in err()
    assert search(after_a=fake + 8) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
    assert search(after_b=fake + 4) < 0 and b"after_a and after_b must be 16-byte aligned" in err()
    assert search(score=fake + 2) < 0 and b"4-byte aligned" in err() and name in err()
    assert search(value=fake + 1) < 0 and b"4-byte aligned" in err()
    for epsilon in (-0.001, 1.001, nan, inf, -inf):
        assert search(epsilon=epsilon) < 0 and b"epsilon must be in [0, 1]" in err() and name in err(), epsilon
    for gamma in (nan, inf, -inf):
        assert search(gamma=gamma) < 0 and b"gamma must be finite" in err() and name in err(), gamma
    # `second` has no alignment requirement: an odd pointer is not what refuses this call
    assert search(second=fake + 1, epsilon=2.0) < 0 and b"epsilon" in err()
    assert search(second=None, score=None, after_a=None, after_b=None, value=None, epsilon=2.0) < 0 and b"epsilon" in err()


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def test_python_refusals_of_the_depth_need_no_gpu():
    import torch
    nt = T.ntuple
    env = _Env(8)
    table = nt.ntuple_table("cpu")
    for depth in (0, 3, 1.5, True, -1, None, "2"):
        with pytest.raises(ValueError, match="depth"):
            nt.NTuplePolicy(env, table, depth=depth)
        with pytest.raises(ValueError, match="depth"):
            nt.NTupleLearner(env, depth=depth)
    one, two = nt.NTuplePolicy(env, table), nt.NTuplePolicy(env, table, 0.99, 0.0, 0, 2)
    assert one.depth == 1 and two.depth == 2 and nt.NTuplePolicy(env, table, depth=1).depth == 1
    with pytest.raises(ValueError, match="second"):
        one.act(second=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="second"):
        one.act(out=torch.zeros(8, dtype=torch.uint8), second=torch.zeros(8, dtype=torch.uint8))
    learner = nt.NTupleLearner(env, depth=2)
    assert learner.depth == 2 and learner.policy.depth == 2 and learner.greedy.depth == 2
    assert nt.NTupleLearner(env).depth == 1 and nt.NTupleLearner(env).greedy.depth == 1
    for depth in (0, 3, True, "1"):
        with pytest.raises(ValueError, match="depth"):
            learner.evaluate(4, depth=depth)
