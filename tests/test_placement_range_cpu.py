"""States for the placement family (tpl_afterstates, tpl_placement_features / _act / _search / _beam) at the ends of the game range,
and what the C oracle says of them -- without a GPU.  test_afterstates_gpu's pool plays L = 10 / M = 40 only; here the games are
(1, 1), where every placement of a running board ends the game, (2, 3), where wins and limit losses fall on the second and third
ply of a search, and (250, 254), the environment's largest, where both counters use their high bits (`moves` is two nibbles in
A.y and A.w, `lines` sits in bits 20..27 of B.z under window bits 32..35).

  * range_fields(gen, L, M): 320 states of eight kinds for any game; RangePool: the oracle's move for all 40 actions of each.
  * the coverage conditions of every game, asserted on the oracle's own outcomes and printed: test_placement_range_gpu.py compares
    the kernels with exactly these states, so what they cover is checked here.
"""
import zlib

import numpy as np
import pytest

import learn_ref as R
from test_afterstates_gpu import Pool, _ragged, _well
from test_gpu_parity import _dense_boards

GAMES = [(1, 1), (2, 3), (250, 254)]
COUNT = 320
KINDS = 8
POOL_CRC = 0xC3D78176                        # of the planes and spare bits of test_afterstates_gpu._pool_fields


def _top_quarter(gen, limit, size):
    """Counters from the top quarter of 0 .. limit - 1."""
    return gen.integers(3 * (limit - 1) // 4, limit, size)


def _refill_moves(M):
    """The values of `moves` below M at residues 8 and 9 (the beam knows 4 and 3 pieces there), the largest and the smallest
    first: 249, 248, 8, 9, 239, 238, 18, 19, ... at M = 254; none at M <= 8."""
    up = [m for m in range(M) if m % 10 in (8, 9)]
    order = []
    for hi, lo in zip(up[::-1], up):
        order += [hi, lo]
    return list(dict.fromkeys(order))


def range_fields(gen, L, M, count=COUNT):
    """`count` states for the game (L, M), kind by index mod 8 (count / 8 of each):
      0 (a) wells of 1..4 rows under an upright I (the last fifth with a second hole: a split clear); (lines, moves) cycles through
            (L - 1, M - 1), (max(L - 4, 0), M - 1), (L - 1, 0), (0, M - 1);
      1 (b) ragged boards, lines uniform in [0, L - 1], moves uniform in [0, M - 1];
      2 (c) ragged boards with moves at residues 8 and 9 below M, the largest such values among them (uniform where M has none);
      3 (d) tall boards (column heights 14..20);
      4 (e) finished boards (states 1, 2, 3) whose counters are anything in 0..255, both ends included;
      5, 6, 7 (f, g, h) dense random boards with both counters from the top quarter of their ranges.
    Every state has all 36 window bits random behind a current piece of 0..6 (so piece 7 is among the later entries), a random slot
    bit and a random spare bit."""
    assert 1 <= L <= 250 and 1 <= M <= 254 and count % KINDS == 0
    dense = _dense_boards(gen, count)
    rows = np.zeros((count, 20), np.uint16)
    cur = gen.integers(0, 7, count)
    lines, moves, state = gen.integers(0, L, count), gen.integers(0, M, count), np.zeros(count, np.int64)
    refill = _refill_moves(M)
    for i in range(count):
        kind, k = i % KINDS, i // KINDS
        if kind == 0:
            j = k // 4
            split = j >= 8
            rows[i], _ = _well(gen, 3 + j % 2 if split else 1 + j % 4, split=split)
            cur[i] = 0
            lines[i], moves[i] = ((L - 1, M - 1), (max(L - 4, 0), M - 1), (L - 1, 0), (0, M - 1))[k % 4]
        elif kind == 1:
            rows[i] = _ragged(gen, 0, 10)
        elif kind == 2:
            rows[i] = _ragged(gen, 0, 13)
            if refill:
                moves[i] = refill[k % len(refill)]
        elif kind == 3:
            rows[i] = _ragged(gen, 14 + k % 4, 21)
        elif kind == 4:
            rows[i] = dense[i]
            state[i] = 1 + k % 3
            lines[i], moves[i] = gen.integers(0, 256, 2)
            if k < 4:
                lines[i], moves[i] = ((255, 255), (0, 0), (255, 0), (0, 255))[k]
        else:
            rows[i] = dense[i]
            lines[i], moves[i] = _top_quarter(gen, L, 1)[0], _top_quarter(gen, M, 1)[0]
    window = (gen.integers(0, 1 << 36, count, dtype=np.int64).astype(np.uint64) & ~np.uint64(7)) | cur.astype(np.uint64)
    return dict(rows=rows, lines=lines, moves=moves, state=state, slot=gen.integers(0, 2, count), window=window,
                spare=gen.integers(0, 2, count).astype(np.uint32))


class RangePool(Pool):
    """test_afterstates_gpu's Pool of range_fields(L, M) at the game (L, M): the planes and the oracle's 40 moves of every state."""

    def __init__(self, oracle, L, M):
        self.L, self.M = L, M
        super().__init__(oracle, range_fields(np.random.default_rng(1000 * L + M), L, M), L, M)

    def coverage(self):
        """Counts of the oracle's own outcomes: pairs are (state, action), 40 per state."""
        f, run, M = self.fields, self.running, self.M
        lines0, moves0 = np.asarray(f["lines"]), np.asarray(f["moves"])
        running_after = (self.state == 0) & run[:, None]
        count = dict(win=int(self.won.sum()), limit=int(self.limit.sum()), topout=int(self.topout.sum()),
                     frozen=40 * int((~run).sum()))
        count.update({f"cleared_{k}": int(((self.cleared == k) & run[:, None]).sum()) for k in (1, 2, 3, 4)})
        count.update(pairs_not_done=int((~self.done[run]).sum()),
                     moves_high_at_8_or_9=int((run & (moves0 >= 128) & np.isin(moves0 % 10, (8, 9))).sum()),
                     lines_high=int((run & (lines0 >= 128)).sum()),
                     win_at_the_limit=int((self.won & (self.moves == M)).sum()),
                     lines_after_251=int(((self.lines >= 251) & run[:, None]).sum()),
                     lines_after_253=int(((self.lines == 253) & run[:, None]).sum()),
                     running_after_moves_240=int((running_after & (self.moves >= 240)).sum()),
                     running_after_lines_1=int((running_after & (self.lines == 1)).sum()),
                     running_after_moves_2=int((running_after & (self.moves == 2)).sum()))
        return count


_POOLS = {}


def range_pool(oracle, L, M):
    """The RangePool of a game, played once per session (the GPU file shares it)."""
    if (L, M) not in _POOLS:
        _POOLS[(L, M)] = RangePool(oracle, L, M)
    return _POOLS[(L, M)]


def test_the_generator_is_deterministic_and_leaves_the_10_40_pool_alone():
    from test_afterstates_gpu import POOL, _pool_fields
    a, b = (range_fields(np.random.default_rng(7), 250, 254) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    f = _pool_fields(np.random.default_rng(1639))
    assert f["rows"].shape == (POOL, 20) and int(np.asarray(f["lines"]).max()) == 9 and int(np.asarray(f["moves"]).max()) == 39
    A, B = R.pack_state(f["rows"], f["lines"], f["moves"], f["state"], f["slot"], f["window"])
    digest = zlib.crc32(A.tobytes() + B.tobytes() + f["spare"].tobytes())
    assert digest == POOL_CRC, hex(digest)                     # the pool that the 10 / 40 files' coverage floors rest on


@pytest.mark.parametrize("L,M", GAMES)
def test_the_states_of_every_game_cover_what_the_kernels_distinguish(oracle, L, M):
    pool = range_pool(oracle, L, M)
    f, run = pool.fields, pool.running
    lines0, moves0, state0 = (np.asarray(f[k]) for k in ("lines", "moves", "state"))
    assert pool.n == COUNT and (np.bincount(np.arange(COUNT) % KINDS) == COUNT // KINDS).all()
    # the states are the game's: a running board has lines < L and moves < M; the window holds piece 7 behind a real current piece
    assert (lines0[run] < L).all() and (moves0[run] < M).all() and (lines0[run] >= 0).all() and (moves0[run] >= 0).all()
    assert set(state0.tolist()) == {0, 1, 2, 3} and (state0 != 0).sum() == COUNT // KINDS
    assert {0, 255} <= set(lines0[~run].tolist()) and {0, 255} <= set(moves0[~run].tolist())
    window = f["window"]
    cur = (window & np.uint64(7)).astype(np.int64)
    assert set(cur.tolist()) == set(range(7))
    later = np.stack([(window >> np.uint64(3 * j)) & np.uint64(7) for j in range(1, 12)], axis=1)
    assert (later == 7).any(axis=0).all() and ((window >> np.uint64(32)) != 0).sum() > COUNT // 2
    assert set(np.asarray(f["slot"]).tolist()) == {0, 1} and set(f["spare"].tolist()) == {0, 1}
    refill = [m for m in range(M) if m % 10 in (8, 9)]
    assert set(refill[-2:]) <= set(moves0[run].tolist())       # the largest moves at residues 8 and 9 (248, 249 at M = 254)
    assert {L - 1, max(L - 4, 0), 0} <= set(lines0[run].tolist()) and {M - 1, 0} <= set(moves0[run].tolist())

    count = pool.coverage()
    print(f"(L, M) = ({L}, {M}): the oracle's outcomes over {COUNT} x 40 pairs: {count}")
    for name in ("win", "limit", "topout", "frozen"):
        assert count[name] >= 8, (name, count)
    for k in (1, 2, 3, 4):
        assert count[f"cleared_{k}"] >= 1, (k, count)
    # the oracle at these ends: a finished game is won, lost at the limit or topped out; won goes before the limit
    assert (pool.lines[pool.won] >= L).all() and (pool.moves[pool.limit] == M).all() and (pool.lines[pool.limit] < L).all()
    assert (pool.moves[run] <= M).all() and (pool.lines[run] <= L + 3).all()
    if (L, M) == (1, 1):
        assert count["pairs_not_done"] == 0 and pool.done[run].all()
    else:
        assert count["pairs_not_done"] >= 8, count
    if (L, M) == (250, 254):
        for name in ("moves_high_at_8_or_9", "lines_high", "win_at_the_limit", "lines_after_251", "running_after_moves_240"):
            assert count[name] >= 8, (name, count)
        assert count["lines_after_253"] >= 1 and int(pool.lines[run].max()) == 253, count
    if (L, M) == (2, 3):
        assert count["running_after_lines_1"] >= 8 and count["running_after_moves_2"] >= 8, count
