"""CPU-side checks of the mirror symmetry (include/tpl_learn.h's rule, _learn_lib.mirror_states / mirror_actions / mirror_coins /
MIRROR_OBS_PERM, the argument checks of tpl_replay_sample_mirror and tpl_mirror_states, the Python refusals):

  * the symmetry itself, against the C oracle: for every piece x rotation x location, over empty, ragged, tall and prepared
    boards with lines and moves near L and M, to_move on the mirrored state and action is the mirror of to_move on the
    original -- rows, lines cleared, moves_used, state and the return value -- with every kind of ending reached at least 100
    times by the oracle alone;
  * the layout and action properties: an involution on all 256 bits, twice-mirrored actions are 10 r + l_eff, every mirrored
    action is below 40;
  * the observation of the mirrored state is the permutation MIRROR_OBS_PERM of the state's;
  * the coin is fair; the header declares what LEARN_SYMBOLS lists; every bad argument is refused without a GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import learn_ref as R
import tetris_piclim as T

PI = [0, 2, 1, 3, 5, 4, 6, 7]
FULL = 0x3FF


def _m():
    return T._learn_lib


# ------------------------------------------------------------------------------------------------ 1. the symmetry
def _stack(heights, gen, holes):
    """rows u16 [20] with column x filled from the bottom to `heights[x]` cells, each filled cell below the top one knocked out
    with probability `holes`."""
    rows = np.zeros(20, np.uint16)
    for x, h in enumerate(heights):
        for k in range(int(h)):
            if k == int(h) - 1 or gen.random() >= holes:
                rows[19 - k] |= np.uint16(1 << x)
    return rows


def _base_boards(gen):
    """(kind, rows): the empty board, ragged ones (heights 0..12, with and without holes), tall ones (heights 15..20)."""
    out = [("empty", np.zeros(20, np.uint16))]
    for k in range(10):
        out.append(("ragged", _stack(gen.integers(0, 13, 10), gen, 0.3 * (k % 2))))
    for k in range(8):
        out.append(("tall", _stack(gen.integers(15 + k % 4, 21, 10), gen, 0.2)))
    return out


def _prepared(oracle, rows, piece, rot, loc, k, gen):
    """`rows` with k of the rows in which (piece, rot, loc) comes to rest filled up to the piece's own cells, so that the move
    completes them -- unless the filling gets in the piece's way, which the oracle then shows.  None if the piece tops out."""
    g = oracle.Game(255, 255, rows=rows, pieces=[piece])
    if g.move(rot, loc) < 0:
        return None
    after = g.rows
    placed = after ^ rows                                  # the piece's four cells, unless the move cleared a row: then skip
    if sum(bin(int(v)).count("1") for v in placed) != 4:
        return None
    at = np.flatnonzero(placed)
    out = rows.copy()
    for r in gen.permutation(at)[:k]:
        out[r] = np.uint16(FULL & ~int(placed[r]))
    return out


def _cases(oracle, L, M):
    """Every case as (rows, piece, rot, loc, lines, moves).  (lines, moves) run over the start of a game, one line / one move
    from its end, and one move from the limit with the lines far from L."""
    gen = np.random.default_rng(20)
    counters = [(0, 0), (L - 1, M - 1), (L - 2, M - 2), (L - 4, 5), (0, M - 1)]
    bases = _base_boards(gen)
    cases = []
    for piece in range(7):
        for rot in range(4):
            for loc in range(10):
                for kind, rows in bases:
                    for lines, moves in (counters if kind != "tall" else counters[:2]):
                        cases.append((rows, piece, rot, loc, lines, moves))
                for kind, rows in bases[:7]:               # the empty board and six ragged ones, prepared for 1..4 clears
                    for k in (1, 2, 3, 4):
                        prepared = _prepared(oracle, rows, piece, rot, loc, k, gen)
                        if prepared is None:
                            continue
                        for lines, moves in counters[:4]:
                            cases.append((prepared, piece, rot, loc, lines, moves))
    return cases


def test_the_move_commutes_with_the_mirror_against_the_oracle(oracle):
    L, M = 10, 40
    cases = _cases(oracle, L, M)
    n = len(cases)
    gen = np.random.default_rng(21)
    rows = np.stack([c[0] for c in cases])
    piece, rot, loc, lines, moves = (np.array([c[k] for c in cases]) for k in range(1, 6))
    window = (gen.integers(0, 1 << 36, n, dtype=np.int64).astype(np.uint64) & ~np.uint64(7)) | piece.astype(np.uint64)
    A, B = R.pack_state(rows, lines, moves, 0, gen.integers(0, 2, n), window)
    action = (10 * rot + loc).astype(np.uint8)
    mA, mB = _m().mirror_states(A, B)
    m_action = _m().mirror_actions(action, A, B)
    m = R.decode_state(mA, mB)
    assert np.array_equal(m["cur"], np.array(PI)[piece]) and np.array_equal(m["lines"], lines) and np.array_equal(m["moves"], moves)
    assert (m_action < 40).all()

    after = dict(rows=np.zeros((n, 20), np.uint16), lines=np.zeros(n, np.int64), moves=np.zeros(n, np.int64))
    m_after = dict(rows=np.zeros((n, 20), np.uint16), lines=np.zeros(n, np.int64), moves=np.zeros(n, np.int64))
    tally = dict(clear={1: 0, 2: 0, 3: 0, 4: 0}, topout=0, win=0, limit=0)
    for i in range(n):
        g = oracle.Game(L, M, rows=rows[i], pieces=[piece[i]], lines_cleared=int(lines[i]), moves_used=int(moves[i]))
        h = oracle.Game(L, M, rows=m["rows"][i], pieces=[m["cur"][i]], lines_cleared=int(lines[i]), moves_used=int(moves[i]))
        ret = g.move(int(rot[i]), int(loc[i]))
        m_ret = h.move(int(m_action[i]) // 10, int(m_action[i]) % 10)
        what = (i, int(piece[i]), int(rot[i]), int(loc[i]), int(lines[i]), int(moves[i]))
        assert ret == m_ret, what
        assert (g.lines_cleared, g.moves_used, g.state) == (h.lines_cleared, h.moves_used, h.state), what
        for dst, game in ((after, g), (m_after, h)):
            dst["rows"][i], dst["lines"][i], dst["moves"][i] = game.rows, game.lines_cleared, game.moves_used
        if ret > 0:
            tally["clear"][ret] += 1
        tally["topout"] += ret < 0
        won = ret > 0 and g.lines_cleared >= L
        tally["win"] += won
        tally["limit"] += ret >= 0 and not won and g.moves_used >= M
        assert (g.state != 0) == bool(ret < 0 or won or g.moves_used >= M), what
    # the boards after the move: the mirror of the original's is the mirrored game's, through the packed layout
    zeros = np.zeros(n, np.int64)
    rA, rB = R.pack_state(after["rows"], after["lines"], after["moves"], zeros, zeros, zeros.astype(np.uint64))
    wA, wB = R.pack_state(m_after["rows"], m_after["lines"], m_after["moves"], zeros, zeros, zeros.astype(np.uint64))
    gA, gB = _m().mirror_states(rA, rB)
    bad = np.flatnonzero((gA != wA).any(axis=1) | (gB != wB).any(axis=1))
    assert bad.size == 0, [cases[i][1:] for i in bad[:5]]
    print(f"{n} cases: {tally}")
    assert min(tally["clear"].values()) >= 100 and tally["topout"] >= 100 and tally["win"] >= 100 and tally["limit"] >= 100, tally


# ------------------------------------------------------------------------------------------------ 2. layout and actions
def test_mirror_states_is_an_involution_on_all_256_bits():
    gen = np.random.default_rng(5)
    A, B = R.pack_state(**R.random_fields(gen, 5000))
    for spare in (0, 1):                                   # bit 31 of B.y, which no field uses, is carried over
        B1 = B | np.uint32(spare << 31)
        mA, mB = _m().mirror_states(A, B1)
        assert mA.dtype == np.uint32 and mB.dtype == np.uint32 and mA.shape == A.shape
        bA, bB = _m().mirror_states(mA, mB)
        assert np.array_equal(bA, A) and np.array_equal(bB, B1)
        f, g = R.decode_state(A, B1), R.decode_state(mA, mB)
        for k in ("lines", "moves", "state", "slot"):
            assert np.array_equal(f[k], g[k]), k
        assert np.array_equal(mB[:, 1] >> np.uint32(31), B1[:, 1] >> np.uint32(31))
        rev = np.zeros_like(f["rows"])
        for x in range(10):
            rev |= ((f["rows"] >> np.uint16(x)) & np.uint16(1)) << np.uint16(9 - x)
        assert np.array_equal(g["rows"], rev)
        pi = np.array(PI, dtype=np.uint64)
        for e in range(12):
            ent = lambda w: ((w >> np.uint64(3 * e)) & np.uint64(7)).astype(np.int64)
            assert np.array_equal(ent(g["window"]), pi[ent(f["window"])].astype(np.int64)), e
    assert (mA != A).any() and tuple(_m().PIECE_MIRROR) == tuple(PI)
    # int32 planes (as torch hands them over) are taken as they are
    iA, iB = _m().mirror_states(A.view(np.int32), B.view(np.int32))
    assert np.array_equal(iA, _m().mirror_states(A, B)[0]) and np.array_equal(iB, _m().mirror_states(A, B)[1])


def test_mirror_actions_over_every_action_byte_and_piece_id():
    widths = np.array([[T.shape_info(p, r)[1] for r in range(4)] for p in range(7)])
    assert np.array_equal(_m().shape_widths()[:7], widths) and np.array_equal(_m().shape_widths()[7], widths[6])
    act = np.tile(np.arange(256, dtype=np.uint8), 8)
    cur = np.repeat(np.arange(8), 256)
    A, B = R.pack_state(np.zeros((act.size, 20), np.uint16), 0, 0, 0, 0, cur.astype(np.uint64) | np.uint64(0o7070))
    got = _m().mirror_actions(act, A, B)
    assert got.dtype == np.uint8 and (got < 40).all()
    r, l = (act // 10) & 3, act % 10
    w = _m().shape_widths()[cur, r]
    l_eff = np.minimum(l, 10 - w)
    assert np.array_equal(got // 10, (4 - r) & 3) and np.array_equal(got % 10, 10 - w - l_eff)
    # twice: in the mirrored state the piece is pi(cur), whose entry [(4 - r) & 3] has the same width
    mA, mB = _m().mirror_states(A, B)
    twice = _m().mirror_actions(got, mA, mB)
    assert np.array_equal(twice, (10 * r + l_eff).astype(np.uint8))
    # the piece spans the same columns, reflected: [l_eff, l_eff + w) <-> [10 - w - l_eff, 10 - l_eff)
    assert np.array_equal(got % 10 + w, 10 - l_eff)


# ------------------------------------------------------------------------------------------------ 3. the observation
@pytest.mark.parametrize("L,M", [(10, 40), (1, 1), (255, 255)])
def test_observation_of_the_mirrored_state_is_the_permutation(L, M):
    perm = _m().MIRROR_OBS_PERM
    assert perm.shape == (217,) and sorted(perm.tolist()) == list(range(217)) and np.array_equal(perm[perm], np.arange(217))
    for y in (0, 7, 19):
        for x in range(10):
            assert perm[10 * y + x] == 10 * y + 9 - x
    for p in range(7):
        assert perm[200 + p] == 200 + PI[p] and perm[207 + p] == 207 + PI[p]
    assert perm[214:].tolist() == [214, 215, 216]
    gen = np.random.default_rng(L)
    fields = R.random_fields(gen, 3000, M=M)
    A, B = R.pack_state(**fields)
    plain = R.obs_from_fields(R.decode_state(A, B), L, M)
    mirrored = R.obs_from_fields(R.decode_state(*_m().mirror_states(A, B)), L, M)
    assert np.array_equal(mirrored, plain[:, perm])
    assert (mirrored != plain).any()


# ------------------------------------------------------------------------------------------------ 4. the coin
@pytest.mark.parametrize("seed,update", [(0, 0), (0, 1), (7, 123), (12345, 99999)])
def test_the_coin_is_fair(seed, update):
    draws = 1 << 20
    coins = _m().mirror_coins(seed, update, draws)
    assert coins.dtype == np.uint8 and coins.shape == (draws,) and set(np.unique(coins)) == {0, 1}
    sigma = 0.5 / 1024
    z = (float(coins.mean()) - 0.5) / sigma
    print(f"(seed, update) = ({seed}, {update}): mean of 2^20 coins {z:+.2f} sigma from 1/2")
    assert abs(z) <= 5.0, z
    # it is bit 0 of the word whose top bits are the uniform slot: the slot's parity says nothing about it
    slots = _m().replay_indices(seed, update, draws, 1 << 22)
    corr = float(np.corrcoef(coins.astype(np.float64), (slots & 1).astype(np.float64))[0, 1])
    assert abs(corr) < 5.0 / 1024, corr


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_the_header_declares_what_learn_symbols_lists():
    text = open(os.path.join(ROOT, "include", "tpl_learn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tpl_[a-z_0-9]+)\s*\(", text)))
    assert sorted(_m().LEARN_SYMBOLS) == declared
    assert "tpl_replay_sample_mirror" in declared and "tpl_mirror_states" in declared
    lib = ctypes.CDLL(_m().build_library())
    for name in declared:
        assert hasattr(lib, name), name
    assert re.search(r"TPL_MIRROR_NEVER = 0, TPL_MIRROR_COIN = 1, TPL_MIRROR_ALWAYS = 2", text)
    assert re.search(r"#define TPL_PIECE_MIRROR \{0, 2, 1, 3, 5, 4, 6, 7\}", text)


def test_argument_errors_come_back_as_statuses_without_a_gpu():
    lib = _m().lib()
    err = lambda: lib.tpl_learn_last_error()
    fake = 1 << 20                                         # 128-byte aligned, never dereferenced: every call below is refused

    def sample(ring=fake, tree=None, cap=16, size=16, head=0, stride=4, n_step=3, gamma=0.99, batch=8, L=2, M=2, obs=fake,
               dtype=0, ret=fake, discount=fake, done=fake, steps=fake, index=None, prob=None, mirror=1, mirrored=fake):
        return lib.tpl_replay_sample_mirror(ring, tree, cap, size, head, stride, n_step, gamma, batch, 0, 0, L, M, obs, dtype,
                                            fake, fake, fake, ret, discount, done, steps, index, prob, mirror, mirrored, None)

    for mirror in (-1, 3, 7, 1 << 20):
        assert sample(mirror=mirror) < 0 and b"mirror" in err(), mirror
        assert sample(mirror=mirror, n_step=0, discount=None, steps=None) < 0 and b"mirror" in err(), mirror
    # the n-step form's checks
    assert sample(ring=None) < 0 and b"null" in err()
    assert sample(obs=None) < 0 and b"null" in err()
    for name in ("ret", "discount", "done", "steps"):
        assert sample(**{name: None}) < 0 and b"null" in err(), name
    assert sample(tree=fake, index=None, prob=fake) < 0 and b"null" in err()
    assert sample(prob=fake) < 0 and b"prob" in err()
    assert sample(cap=0, size=0) < 0 and b"capacity" in err()
    assert sample(size=17) < 0 and b"size" in err()
    assert sample(batch=0) < 0 and b"batch" in err()
    assert sample(L=0) < 0 and b"L and M" in err()
    assert sample(dtype=7) < 0 and b"dtype" in err()
    assert sample(obs=fake + 4) < 0 and b"aligned" in err()
    assert sample(tree=fake + 16, index=fake, prob=fake) < 0 and b"aligned" in err()
    for n_step in (-1, 17):
        assert sample(n_step=n_step) < 0 and b"n_step" in err(), n_step
    assert sample(gamma=1.5) < 0 and b"gamma" in err()
    assert sample(stride=0) < 0 and b"stride" in err()
    assert sample(head=16) < 0 and b"head" in err()
    assert sample(size=10, head=3) < 0 and b"head must equal size" in err()
    # the 1-step form (n_step = 0) takes neither discount nor steps, and does not read head, stride or gamma
    assert sample(n_step=0) < 0 and b"1-step" in err()
    assert sample(n_step=0, discount=None) < 0 and b"1-step" in err()
    assert sample(n_step=0, discount=None, steps=None, ret=None) < 0 and b"null" in err()
    assert sample(n_step=0, discount=None, steps=None, size=0) < 0 and b"size" in err()
    assert sample(n_step=0, discount=None, steps=None, tree=fake, index=fake) < 0 and b"null" in err()
    assert b"tpl_replay_sample_mirror" in err()
    # the standalone entry
    ms = lib.tpl_mirror_states
    assert ms(4, None, fake, fake, fake, None, None, None) < 0 and b"null" in err()
    assert ms(4, fake, fake, fake, None, None, None, None) < 0 and b"null" in err()
    assert ms(4, fake, fake, fake, fake, fake, None, None) < 0 and b"go together" in err()
    assert ms(4, fake, fake, fake, fake, None, fake, None) < 0 and b"go together" in err()
    assert ms(0, fake, fake, fake, fake, None, None, None) < 0 and b"count" in err()
    assert ms(1 << 31, fake, fake, fake, fake, None, None, None) < 0 and b"count" in err()
    assert ms(4, fake + 8, fake, fake, fake, None, None, None) < 0 and b"aligned" in err()
    assert ms(4, fake, fake, fake, fake + 4, None, None, None) < 0 and b"aligned" in err()


def test_python_refusals_need_no_gpu():
    assert [_m().mirror_mode(v) for v in (False, True, "always")] == [0, 1, 2]
    bad = (0, 1, 2, None, "coin", "Always", "", 1.0, b"always", [True])
    for value in bad:
        with pytest.raises(ValueError, match="mirror"):
            _m().mirror_mode(value)
        for ring in (T.ReplayRing(64, "cpu"), T.PrioritizedReplayRing.__new__(T.PrioritizedReplayRing)):
            with pytest.raises(ValueError, match="mirror"):
                ring.sample(8, 0, 0, None, mirror=value)
    for value in (0, 1, "always", None, "yes"):            # the learner draws with the coin or not at all
        with pytest.raises(ValueError, match="mirror"):
            T.DQNLearner(None, mirror=value)
    with pytest.raises(ValueError, match="empty"):         # a good value goes on to the next check
        T.ReplayRing(64, "cpu").sample(8, 0, 0, None, mirror="always")
    with pytest.raises(AttributeError):                    # and the learner to its environment
        T.DQNLearner(None, mirror=True)
    with pytest.raises(TypeError):                         # keyword-only: __init__'s positional order has not moved
        T.DQNLearner(*([None] * 18))
    import inspect
    assert "mirror" not in inspect.signature(T.DQNLearner.__init__).parameters


def test_mirrored_kernels_exist_and_use_no_scratch():
    import subprocess
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), _m().build_library()],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    rows = [l.split() for l in res.stdout.splitlines() if " scratch " in l]
    names = [r[-1] for r in rows]
    for kernel in ("replay_sample_kernel", "replay_sample_prioritized_kernel"):
        for dtype in ("f", "14__hip_bfloat16"):
            for kn in (0, 1, 4, 8, 16):
                for mirror in (0, 1):
                    want = f"{kernel}I{dtype}Li{kn}ELb{mirror}EE"
                    assert any(want in n for n in names), (want, names)
    assert any("mirror_states_kernel" in n for n in names)
    for r in rows:
        assert r[r.index("scratch") - 1] == "0", r
