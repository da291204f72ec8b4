"""States for the n-tuple family (tpl_ntuple_value / _act / _search / _beam and the update entries, in every form) over the whole game
range and at the clamps of the counter index, and what the rule and the C oracle say of them -- without a GPU.  The other n-tuple files
play L = 10 / M = 40, where no `min` and no `max` of

    k = 64 min(max(L - lines, 0), 15) + min(max(M - moves, 0), 63)          (counter_index in csrc/learn/tpl_ntuple.h)

ever fires on a running board.  test_ntuple_range_gpu.py compares the kernels with exactly the states built here, so what they cover is
asserted here, on the reference's own outcomes and never on a kernel's.

  * THE COUNTER RULE BY HAND: over L in {1, 2, 15, 16, 17, 250} x M in {1, 3, 63, 64, 65, 254} and all lines, moves in 0..255,
    ntuple_counter_index is the rule written out with Python ints, and the counter column of ntuple_indices of every plain form is the
    form's counter base + that k -- the mirror holds the formula in three places; lines > L and moves > M give 0 on their axis;
  * ntuple_stages_of under a map of random 32-bit words, at the clamped index 1023 and at 0;
  * range_pool (test_placement_range_cpu) at (250, 254): 280 of 320 states run, 215 with more than 15 lines left and 65 with at most
    15, 107 with more than 63 moves left and 173 with at most 63 -- at least 32 on each side of each clamp are asserted;
  * edge_fields / edge_pool, the EDGE SET at (20, 100): 128 states, half wells of 1..4 rows under an upright I, half ragged boards, lines
    left cycling through 15..19 and moves left through 63, 64, 65.  The oracle's 128 x 40 pairs: 8 / 6 / 6 / 6 go from 16 lines left to
    15 / 14 / 13 / 12 and still run, 8 go 17 -> 16 (both sides clamped: the same entry), 18 go 17 -> 15 or below; 1,680 / 1,680 / 1,760
    running pairs go 64 -> 63, 65 -> 64 and 63 -> 62 moves left (the floors: 4 each, and 100 each);
  * play_fields / play_pool, the (16, 64) boards: 64 carved configurations fresh -- 16 lines and 64 moves left, one past each edge --
    and 192 more after 1..12 random oracle moves: 195 of the 256 run, 171 of them with 16 lines left and 24 with fewer, 64 with 64
    moves left and 131 with fewer; 263 pairs take a board from 16 lines left to 15 or below.
"""
import numpy as np
import pytest

import tetris_piclim as T
from test_afterstates_gpu import Pool, _ragged, _well
from test_placement_range_cpu import range_pool

EDGE_GAME, EDGE_COUNT = (20, 100), 128
PLAY_GAME, PLAY_COUNT, PLAY_CONFIGS = (16, 64), 256, 64
LINES_LEFT, MOVES_LEFT = (15, 16, 17, 18, 19), (63, 64, 65)
GRID_L, GRID_M = (1, 2, 15, 16, 17, 250), (1, 3, 63, 64, 65, 254)
# (the column of ntuple_indices, the table entry of counter 0) of every counter a plain form has: include/tpl_learn.h's layouts
COUNTERS = {"2x4": ((153, 313344),), "3x3": ((144, 589824),), "2x4+3x3": ((153, 313344), (154 + 144, 314368 + 589824)),
            "feat": ((9, 18432),), "3x3+feat": ((144, 589824), (145 + 9, 590848 + 18432)), "feat+spare": ((10, 20480),)}


def _m():
    return T._learn_lib


def counter_by_hand(L, M, lines, moves):
    """The header's sentence with Python ints, one state at a time."""
    return 64 * min(max(int(L) - int(lines), 0), 15) + min(max(int(M) - int(moves), 0), 63)


# ------------------------------------------------------------------------------------------------ the states
def _random_windows(gen, cur):
    """All 36 window bits random behind the current piece."""
    count = len(cur)
    return (gen.integers(0, 1 << 36, count, dtype=np.int64).astype(np.uint64) & ~np.uint64(7)) | np.asarray(cur).astype(np.uint64)


def edge_fields(gen, L, M, count=EDGE_COUNT):
    """`count` running states around the clamp edges of the game (L, M): the even ones are wells of 1 + j % 4 rows under an upright I
    (j = index // 2), the odd ones ragged boards of heights 0..9 under any piece; lines left cycles through 15..19 (for the wells once
    per four, so that every depth of well meets every value) and moves left through 63, 64, 65.  The window bits behind the current
    piece, the slot bit and the spare bit are random, as in range_fields."""
    assert 19 <= L <= 250 and 65 <= M <= 254 and count % 2 == 0
    rows = np.zeros((count, 20), np.uint16)
    cur = gen.integers(0, 7, count)
    lines, moves = np.zeros(count, np.int64), np.zeros(count, np.int64)
    for i in range(count):
        j = i // 2
        if i % 2 == 0:
            rows[i], _ = _well(gen, 1 + j % 4, split=False)
            cur[i] = 0
            lines[i] = L - LINES_LEFT[(j // 4) % 5]
        else:
            rows[i] = _ragged(gen, 0, 10)
            lines[i] = L - LINES_LEFT[j % 5]
        moves[i] = M - MOVES_LEFT[j % 3]
    return dict(rows=rows, lines=lines, moves=moves, state=np.zeros(count, np.int64), slot=gen.integers(0, 2, count),
                window=_random_windows(gen, cur), spare=gen.integers(0, 2, count).astype(np.uint32))


def play_fields(oracle, gen, L, M, count=PLAY_COUNT, configs=PLAY_CONFIGS):
    """`count` states of the game (L, M) as play reaches them: `configs` carved configurations as they are reset -- nothing cleared, no
    move made --, then the same configurations after 1..12 random moves of the C oracle (a game that ends on the way stays as it ended).
    The window holds the configuration's pieces from the move count on, twelve of them, 7 behind the last."""
    rows0, pieces = T.generate_configs(L, M, configs, seed=1000 * L + M)
    rows = np.zeros((count, 20), np.uint16)
    lines, moves, state = np.zeros(count, np.int64), np.zeros(count, np.int64), np.zeros(count, np.int64)
    window = np.zeros(count, np.uint64)
    for i in range(count):
        c = i % configs
        g = oracle.Game(L, M, rows=rows0[c], pieces=pieces[c])
        for _ in range(0 if i < configs else int(gen.integers(1, 13))):
            if g.state != 0:
                break
            ret = g.move(int(gen.integers(0, 4)), int(gen.integers(0, 10)))
        rows[i], lines[i], moves[i] = g.rows, g.lines_cleared, g.moves_used
        state[i] = 0 if g.state == 0 else (3 if ret < 0 else g.state)      # the planes tell a top-out (3) from the limit (2)
        ahead = list(pieces[c][moves[i]:moves[i] + 12]) + [7] * 12
        window[i] = sum(int(p) << (3 * e) for e, p in enumerate(ahead[:12]))
    return dict(rows=rows, lines=lines, moves=moves, state=state, slot=gen.integers(0, 2, count), window=window,
                spare=gen.integers(0, 2, count).astype(np.uint32))


_POOLS = {}


def edge_pool(oracle):
    """The edge set at (20, 100) and the oracle's 40 moves of every state, played once per session (the GPU file shares it)."""
    if "edge" not in _POOLS:
        L, M = EDGE_GAME
        _POOLS["edge"] = Pool(oracle, edge_fields(np.random.default_rng(1000 * L + M), L, M), L, M)
    return _POOLS["edge"]


def play_pool(oracle):
    """The (16, 64) boards and the oracle's 40 moves of every running one, once per session."""
    if "play" not in _POOLS:
        L, M = PLAY_GAME
        _POOLS["play"] = Pool(oracle, play_fields(oracle, np.random.default_rng(1000 * L + M + 1), L, M), L, M)
    return _POOLS["play"]


def edge_coverage(pool, L, M):
    """Counts of (state, action) pairs by the lines and moves left before and after the oracle's move; all but lines_17_to_15_or_below
    count pairs that leave the game running."""
    f = pool.fields
    left0, mleft0 = (L - np.asarray(f["lines"]))[:, None], (M - np.asarray(f["moves"]))[:, None]
    left1, mleft1 = L - pool.lines, M - pool.moves
    on = (pool.state == 0) & pool.running[:, None]
    count = {f"lines_16_to_{16 - d}": int((on & (left0 == 16) & (left1 == 16 - d)).sum()) for d in (1, 2, 3, 4)}
    count.update(lines_17_to_16=int((on & (left0 == 17) & (left1 == 16)).sum()),
                 lines_17_to_15_or_below=int((pool.running[:, None] & (left0 == 17) & (left1 <= 15)).sum()),
                 moves_64_to_63=int((on & (mleft0 == 64) & (mleft1 == 63)).sum()),
                 moves_65_to_64=int((on & (mleft0 == 65) & (mleft1 == 64)).sum()),
                 moves_63_to_62=int((on & (mleft0 == 63) & (mleft1 == 62)).sum()))
    return count


def clamp_sides(pool, L, M):
    """The running states of a pool on each side of each clamp."""
    f, run = pool.fields, pool.running
    left, mleft = L - np.asarray(f["lines"]), M - np.asarray(f["moves"])
    return dict(running=int(run.sum()), lines_left_above_15=int((run & (left > 15)).sum()), lines_left_at_most_15=int((run & (left <= 15)).sum()),
                moves_left_above_63=int((run & (mleft > 63)).sum()), moves_left_at_most_63=int((run & (mleft <= 63)).sum()))


# ------------------------------------------------------------------------------------------------ 1. the counter rule by hand
@pytest.mark.parametrize("L", GRID_L)
def test_the_counter_index_is_the_rule_written_out_for_every_lines_and_moves(L):
    every = np.arange(256)
    for M in GRID_M:
        left_l = [min(max(L - l, 0), 15) for l in range(256)]              # Python ints: nothing here can wrap
        left_m = [min(max(M - m, 0), 63) for m in range(256)]
        want = 64 * np.array(left_l, np.int64)[:, None] + np.array(left_m, np.int64)[None, :]
        got = _m().ntuple_counter_index(L, M, every[:, None], every[None, :])
        assert got.shape == (256, 256) and got.dtype == np.int64 and np.array_equal(got, want), (L, M)
        assert want[3, 7] == counter_by_hand(L, M, 3, 7) and want[255, 255] == 0 == counter_by_hand(L, M, 255, 255)
        # finished boards carry anything in 0..255: past L or M the axis reads 0, it never wraps to a high counter
        assert (got[L:] // 64 == 0).all() and (got[:, M:] % 64 == 0).all() and 0 <= got.min() and got.max() <= 1023
        assert got[0, 0] == 64 * min(L, 15) + min(M, 63) and (got[:L] // 64 >= 1).all() and (got[:, :M] % 64 >= 1).all()
        # the unsigned forms of the narrow fields, where a subtraction in 8 or in 32 bits would wrap
        for dtype in (np.uint8, np.uint32, np.int32):
            assert np.array_equal(_m().ntuple_counter_index(L, M, every.astype(dtype)[:, None], every.astype(dtype)[None, :]), want), dtype


@pytest.mark.parametrize("shape", list(COUNTERS))
def test_the_counter_column_of_every_plain_form_is_its_base_plus_that_index(shape):
    gen = np.random.default_rng(len(shape))
    for L in GRID_L:
        for M in GRID_M:
            # every lines against the moves around the edges, and every moves against the lines around them
            edge_m = sorted({0, max(M - 64, 0), max(M - 63, 0), max(M - 62, 0), M - 1, M, min(M + 1, 255), 255})
            edge_l = sorted({0, max(L - 16, 0), max(L - 15, 0), max(L - 14, 0), L - 1, L, min(L + 1, 255), 255})
            pairs = [(l, m) for l in range(0, 256, 3) for m in edge_m] + [(l, m) for m in range(0, 256, 3) for l in edge_l]
            pairs += [(l, m) for l in edge_l for m in edge_m]
            lines, moves = (np.array(v, np.int64) for v in zip(*pairs))
            rows = np.zeros((lines.size, 20), np.uint16)
            rows[:, 19] = gen.integers(0, 0x3FF, lines.size)               # never a full row
            piece = gen.integers(0, 8, lines.size)
            index, used = _m().ntuple_indices(rows, piece, L, M, lines, moves, shape=shape)
            want = np.array([counter_by_hand(L, M, l, m) for l, m in pairs], np.int64)
            assert {0, 64 * min(L, 15) + min(M, 63)} <= set(want.tolist())
            for column, base in COUNTERS[shape]:
                assert np.array_equal(index[:, column], base + want), (shape, L, M, column)
                assert used[:, column].all()
            assert index.shape[1] == COUNTERS[shape][-1][0] + 1 and index.max() < _m().ntuple_entries_of(shape)
            assert [c for c, _ in COUNTERS[shape]] == _m()._counter_columns(shape)


def test_the_stage_of_a_state_is_the_map_word_at_its_counter_index_masked_to_three_bits():
    gen = np.random.default_rng(1023)
    stage_map = gen.integers(-(1 << 31), 1 << 31, 1024).astype(np.int32)
    stage_map[1023], stage_map[0] = np.int32(-3), np.int32(0x7FFFFFF6)      # ...101 and ...110: the high bits are dropped
    staged = np.concatenate([np.zeros(8 * 19456, np.int32), stage_map])    # a whole staged table reads its last 1,024 entries
    for L, M in ((250, 254), (16, 64), (20, 100), (17, 65), (15, 63), (1, 1)):
        lines, moves = np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij")
        lines, moves = lines.reshape(-1), moves.reshape(-1)
        want = np.array([int(stage_map[counter_by_hand(L, M, l, m)]) & 7 for l, m in zip(lines, moves)], np.int64)
        for table in (stage_map, staged):
            got = _m().ntuple_stages_of(table, L, M, lines, moves)
            assert got.dtype == np.int64 and np.array_equal(got, want), (L, M)
        # a fresh board past both clamps reads entry 1023, a board with nothing left entry 0
        fresh, spent = _m().ntuple_stages_of(stage_map, L, M, [0], [0]), _m().ntuple_stages_of(stage_map, L, M, [L], [M])
        assert int(spent[0]) == 6 and (int(fresh[0]) == 5 or L < 15 or M < 63)
        assert int(_m().ntuple_stages_of(stage_map, L, M, [255], [255])[0]) == 6


# ------------------------------------------------------------------------------------------------ 2. the coverage conditions
def test_the_range_pool_at_250_254_keeps_running_states_on_each_side_of_each_clamp(oracle):
    L, M = 250, 254
    count = clamp_sides(range_pool(oracle, L, M), L, M)
    print(f"(L, M) = ({L}, {M}): the running states of the range pool by the clamps: {count}")
    for name, n in count.items():
        assert n >= 32, (name, count)
    assert count["lines_left_above_15"] + count["lines_left_at_most_15"] == count["running"]


def test_the_generator_is_deterministic():
    a, b = (edge_fields(np.random.default_rng(7), 20, 100) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["rows"].shape == (EDGE_COUNT, 20)
    with pytest.raises(AssertionError):
        edge_fields(np.random.default_rng(7), 18, 100)
    with pytest.raises(AssertionError):
        edge_fields(np.random.default_rng(7), 20, 64)


def test_the_edge_set_crosses_every_clamp_edge_on_the_oracle(oracle):
    L, M = EDGE_GAME
    pool = edge_pool(oracle)
    f = pool.fields
    assert pool.n == EDGE_COUNT and pool.running.all()
    left, mleft = L - np.asarray(f["lines"]), M - np.asarray(f["moves"])
    assert set(left.tolist()) == set(LINES_LEFT) and set(mleft.tolist()) == set(MOVES_LEFT)
    assert {(int(a), int(b)) for a, b in zip(left, mleft)} == {(a, b) for a in LINES_LEFT for b in MOVES_LEFT}
    cur = (f["window"] & np.uint64(7)).astype(np.int64)
    assert (cur[0::2] == 0).all() and set(cur[1::2].tolist()) == set(range(7))
    assert ((f["window"] >> np.uint64(32)) != 0).sum() > EDGE_COUNT // 2 and set(np.asarray(f["slot"]).tolist()) == {0, 1}
    assert set(f["spare"].tolist()) == {0, 1}
    count = edge_coverage(pool, L, M)
    print(f"(L, M) = ({L}, {M}): the oracle's outcomes over {EDGE_COUNT} x 40 pairs of the edge set: {count}; "
          f"cleared {[int((pool.cleared == k).sum()) for k in range(5)]}, finished {int(pool.done.sum())}")
    for name in ("lines_16_to_15", "lines_16_to_14", "lines_16_to_13", "lines_16_to_12", "lines_17_to_16", "lines_17_to_15_or_below"):
        assert count[name] >= 4, (name, count)
    for name in ("moves_64_to_63", "moves_65_to_64", "moves_63_to_62"):
        assert count[name] >= 100, (name, count)
    # a move takes one move and clears at most four lines: nothing here ends by the counters
    assert not pool.won.any() and not pool.limit.any() and (pool.moves[pool.running] == np.asarray(f["moves"])[:, None] + 1).all()


def test_the_16_64_boards_start_one_past_each_edge_and_cross_both_in_play(oracle):
    L, M = PLAY_GAME
    pool = play_pool(oracle)
    f, run = pool.fields, pool.running
    lines, moves = np.asarray(f["lines"]), np.asarray(f["moves"])
    fresh = np.arange(PLAY_COUNT) < PLAY_CONFIGS
    assert pool.n == PLAY_COUNT and (lines[fresh] == 0).all() and (moves[fresh] == 0).all() and run[fresh].all()
    assert (_m().ntuple_counter_index(L, M, lines[fresh], moves[fresh]) == 1023).all()
    assert (_m().ntuple_counter_index(L, M, pool.lines[fresh], pool.moves[fresh]) % 64 == 63).all()     # 64 -> 63: still clamped
    count = clamp_sides(pool, L, M)
    stepped = run & ~fresh
    count.update(stepped_running=int(stepped.sum()), lines_left_exactly_16=int((run & (lines == 0)).sum()),
                 pairs_16_to_15_or_below=int((run[:, None] & (lines == 0)[:, None] & (pool.state == 0) & (pool.lines >= 1)).sum()),
                 distinct_counters=int(np.unique(_m().ntuple_counter_index(L, M, lines[run], moves[run])).size))
    print(f"(L, M) = ({L}, {M}): {PLAY_COUNT} boards, {count}")
    assert count["stepped_running"] >= 96 and count["lines_left_at_most_15"] >= 8 and count["moves_left_above_63"] == PLAY_CONFIGS
    assert count["moves_left_at_most_63"] >= 96 and count["pairs_16_to_15_or_below"] >= 8 and count["distinct_counters"] >= 16
    cur = (f["window"][run] & np.uint64(7)).astype(np.int64)
    assert cur.max() <= 6 and len(set(cur.tolist())) == 7
