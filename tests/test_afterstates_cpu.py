"""CPU-side checks of the afterstate enumeration (include/tpl_learn.h's rule, csrc/learn/afterstates.hip, _learn_lib.canonical_actions,
lookahead.py):

  * canonical actions: the numpy rule and tpl_canonical_action agree for every piece id and action, the distinct placements
    number 17, 34, 34, 34, 17, 17, 9, and -- against the C oracle, on ragged boards for every piece -- an action and its canonical
    alias are the same move: rows, lines, moves, state and the rows cleared;
  * every refusal of tpl_afterstates comes back as a status with a message, without a GPU;
  * the header declares what LEARN_SYMBOLS lists, the kernel is in tools/kernel_resources.sh's output without scratch, the code
    object is gfx950 only;
  * the Python refusals need no GPU, and importing the package leaves the learner library unloaded.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import tetris_piclim as T
from test_mirror_cpu import _stack

DISTINCT = [17, 34, 34, 34, 17, 17, 9]
NROT = [2, 4, 4, 4, 2, 2, 1, 1]


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ 1. canonical actions
def test_canonical_actions_on_the_host_and_in_the_library_agree():
    lib = _m().lib()
    table = _m().canonical_actions(np.arange(8)[:, None], np.arange(40)[None, :])
    assert table.dtype == np.uint8 and table.shape == (8, 40)
    for cur in range(8):
        for a in range(40):
            assert lib.tpl_canonical_action(cur, a) == table[cur, a], (cur, a)
    # the rule, restated: 10 (r mod nrot) + min(l, 10 - w), with piece id 7 reading O's table entry
    widths = np.array([[T.shape_info(p, r)[1] for r in range(4)] for p in range(7)])
    widths = np.concatenate([widths, widths[6:7]])
    for cur in range(8):
        for a in range(40):
            r, l = a // 10, a % 10
            assert table[cur, a] == 10 * (r % NROT[cur]) + min(l, 10 - widths[cur, r]), (cur, a)
    assert tuple(_m().PIECE_ROTATIONS) == tuple(NROT) and _m().NUM_ACTIONS == 40
    distinct = (table == np.arange(40)[None, :]).sum(axis=1)
    assert distinct[:7].tolist() == DISTINCT and distinct[7] == 9
    assert 40 - max(DISTINCT) == 6 and 40 - min(DISTINCT) == 31          # 6 to 31 of the 40 actions are aliases
    # idempotent, and an alias never has a larger index than the action
    for cur in range(8):
        assert np.array_equal(table[cur][table[cur]], table[cur]) and (table[cur] <= np.arange(40)).all()
    assert (table[:, 0] == 0).all()
    for cur, a in ((-1, 0), (8, 0), (0, -1), (0, 40), (0, 1 << 20)):
        assert lib.tpl_canonical_action(cur, a) == -1, (cur, a)
    for cur, a in ((8, 0), (0, 40), (-1, 3)):
        with pytest.raises(ValueError):
            _m().canonical_actions(cur, a)


def test_an_action_and_its_canonical_alias_are_one_move_against_the_oracle(oracle):
    L, M, boards = 10, 40, 700
    gen = np.random.default_rng(40)
    table = _m().canonical_actions(np.arange(8)[:, None], np.arange(40)[None, :])
    aliased = cleared = topouts = 0
    for i in range(boards):
        piece = i % 7
        tall = i % 5 == 4
        rows = _stack(gen.integers(14, 21, 10) if tall else gen.integers(0, 13, 10), gen, 0.3 * (i % 2))
        if i % 3 == 0:                                         # a nearly full row under the stack's top: clears happen
            rows[19] = np.uint16(0x3FF & ~(1 << int(gen.integers(0, 10))))
        lines, moves = ((0, 0), (L - 1, M - 1), (3, 17), (L - 1, 5))[i % 4]
        outcome = []
        for a in range(40):
            g = oracle.Game(L, M, rows=rows, pieces=[piece], lines_cleared=lines, moves_used=moves)
            ret = g.move(a // 10, a % 10)
            outcome.append((g.rows.tobytes(), g.lines_cleared, g.moves_used, g.state, ret))
            cleared += ret > 0
            topouts += ret < 0
        for a in range(40):
            c = int(table[piece, a])
            aliased += c != a
            assert outcome[a] == outcome[c], (i, piece, a, c)
    print(f"{boards} boards x 40 actions: {aliased} aliases, {cleared} clearing moves, {topouts} top-outs, no disagreement")
    assert aliased == 100 * sum(40 - d for d in DISTINCT) and cleared >= 100 and topouts >= 100


# ------------------------------------------------------------------------------------------------ 2. arguments
def test_every_refusal_comes_back_as_a_status_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                             # 16-byte aligned, never dereferenced: every call is refused

    def call(a=fake, b=fake, n=4, L=2, M=2, out_a=fake, out_b=fake, reward=fake, done=fake, cleared=fake, canonical=fake):
        return lib.tpl_afterstates(a, b, n, L, M, 1.0, 0.0, 0.0, out_a, out_b, reward, done, cleared, canonical, None)

    assert call(a=None) < 0 and b"null" in err()
    assert call(b=None) < 0 and b"null" in err()
    for n in (0, -1, -(1 << 40)):
        assert call(n=n) < 0 and b"positive" in err(), n
    limit = -(-(1 << 31) // 40)                                # the first n with 40 n >= 2^31
    assert 40 * limit >= 1 << 31 > 40 * (limit - 1)
    for n in (limit, limit + 1, 1 << 31, 1 << 40, (1 << 63) - 1):
        assert call(n=n) < 0 and b"2^31" in err(), n
    for name in ("a", "b", "out_a", "out_b"):
        for off in (4, 8, 1):
            assert call(**{name: fake + off}) < 0 and b"aligned" in err(), (name, off)
    assert call(out_a=None) < 0 and b"go together" in err()
    assert call(out_b=None) < 0 and b"go together" in err()
    assert call(out_a=None, out_b=None, reward=None, done=None, cleared=None, canonical=None) < 0 and b"at least one output" in err()
    for L, M in ((0, 2), (256, 2), (2, 0), (2, 256), (-1, -1), (251, 2), (255, 2), (2, 255)):
        assert call(L=L, M=M) < 0 and b"L and M" in err(), (L, M)
    # the environment's largest game is not refused for its size: the alignment check, which comes after L and M, speaks
    assert call(L=250, M=254, a=fake + 8) < 0 and b"aligned" in err() and b"L and M" not in err()
    assert call(reward=fake + 2) < 0 and b"aligned" in err()
    assert b"tpl_afterstates" in err()


# ------------------------------------------------------------------------------------------------ 3. symbols, resources
def test_the_header_declares_the_two_entry_points_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    assert re.search(r"#define TPL_PIECE_ROTATIONS \{2, 4, 4, 4, 2, 2, 1, 1\}", text)
    assert "GOOD FOR `cur` AND `next` ONLY" in text            # the window caveat is stated where the rule is
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text)))
    assert sorted(_m().LEARN_SYMBOLS) == declared
    assert "tpl_afterstates" in declared and "tpl_canonical_action" in declared
    lib = ctypes.CDLL(_m().build_library())
    for name in declared:
        assert hasattr(lib, name), name
    assert any(p.endswith(os.path.join("learn", "afterstates.hip")) for p in _m()._sources())


def test_the_afterstate_kernel_uses_no_scratch_and_targets_gfx950_only():
    path = _m().build_library()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), path], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    mine = [r for r in rows if "afterstates_kernel" in r[-1]]
    assert len(mine) == 1, [r[-1] for r in rows]
    assert mine[0][mine[0].index("scratch") - 1] == "0", mine
    for r in rows:                                             # and every other kernel of the library is as it was
        assert r[r.index("scratch") - 1] == "0", r
    blob = open(path, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx942", b"gfx90a", b"sm_"):
        assert other not in blob


# ------------------------------------------------------------------------------------------------ 4. the Python surface
class _Env:
    """What afterstates() reads of an environment before it touches the device."""

    def __init__(self, n):
        import torch
        self.L, self.M, self.num_envs, self.reward_params, self.device = 5, 20, n, (1.0, 0.0, 0.0), torch.device("cpu")


def test_python_refusals_need_no_gpu():
    import torch
    look = T.lookahead
    assert T.afterstates is look.afterstates and T.LookaheadPolicy is look.LookaheadPolicy
    env = _Env(4)
    good = torch.zeros((4, 4), dtype=torch.int32)
    for a, b in ((good, None), (None, good)):
        with pytest.raises(ValueError, match="go together"):
            look.afterstates(env, a, b)
    bad = (torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int64), torch.zeros((4, 4), dtype=torch.uint8),
           torch.zeros(16, dtype=torch.int32), torch.zeros((2, 2, 4), dtype=torch.int32), np.zeros((4, 4), np.int32), None)
    for t in bad[:-1]:
        for a, b in ((t, good), (good, t)):
            with pytest.raises(ValueError, match=r"int32 \[K, 4\]"):
                look.afterstates(env, a, b)
    with pytest.raises(ValueError, match="equal shape"):
        look.afterstates(env, good, torch.zeros((5, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="1 .."):
        look.afterstates(env, good[:0], good[:0])
    # into= must hold exactly 40 K boards: K = the environment's boards, or the planes given
    for into in (_Env(4), _Env(159), _Env(161), env):
        with pytest.raises(ValueError, match="exactly 160 boards"):
            look.afterstates(env, into=into)
    with pytest.raises(ValueError, match="exactly 80 boards"):
        look.afterstates(env, good[:2], good[:2], into=_Env(160))
    for chunk in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="chunk"):
            look.LookaheadPolicy(env, chunk=chunk)
    # the learner: lookahead is greedy
    learner = T.DQNLearner.__new__(T.DQNLearner)
    for eps in (0.1, 1.0, -0.5):
        with pytest.raises(ValueError, match="epsilon"):
            learner.evaluate(4, epsilon=eps, lookahead=True)
    with pytest.raises(AttributeError):                        # a good call goes on to the learner's environment
        learner.evaluate(4, lookahead=True)
    import inspect
    assert list(inspect.signature(T.DQNLearner.evaluate).parameters) == ["self", "steps", "epsilon", "lookahead"]


def test_importing_the_package_still_leaves_the_learner_library_unloaded():
    code = ("import sys; sys.path.insert(0, %r); import tetris_piclim as T; T._lib.lib(); T.BatchedTetris; "
            "before = int(any(m.endswith(('.learn', '._learn_lib', '.lookahead')) for m in sys.modules)); "
            "T.lookahead; T.afterstates; T.LookaheadPolicy; "
            "print(before, int('libtpl_learn' in open('/proc/self/maps').read()))") % ROOT
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    assert res.stdout.split() == ["0", "0"]
