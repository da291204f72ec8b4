"""Per-configuration tallies and the resampled pool on one MI355X (include/tpl_learn.h's "Per-configuration tallies and the resampled
pool"; config_index_kernel, pool_tally_kernel and pool_resample_kernel of csrc/learn/curriculum.hip; curriculum.py):

  * config_index is the oracle's assign(board, birth(board)) after a full reset and after 40 auto-reset steps, in both assignment
    modes, below, around and above N entries -- and, independently of every mirror, a board with moves_used == 0 holds rows[index];
  * the tallies equal np.bincount of the pre-step config_index over the boards that end, entry by entry, and their totals the
    steps' done flags and the environment's own win count; at n_cfg = 1, with auto-reset off, and across a pool swap;
  * observe writes nothing to the environment;
  * resample_pool equals its numpy mirror byte for byte; PoolCurriculum folds, reweights, resamples and loads as written;
  * the hooks of NTupleLearner and evaluate_heuristic add what they say and change nothing else.

N = 96 (three clock groups, not a multiple of 64) and N = 2,080 (nine blocks, the last one partial).
"""
import numpy as np
import pytest
import torch

import tetris_piclim as T
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = {"hash": 0, "sequential": 1}
GAMES = [(1, 2), (2, 3), (10, 40)]


def _m():
    return T._learn_lib


def _np(t):
    return t.cpu().numpy()


def _make(L, M, n, n_cfg, assign="hash", auto_reset=True, seed=5, global_offset=0):
    """An environment with a pool of n_cfg entries and the oracle twin that plays the same pool."""
    env = T.BatchedTetris(L, M, n, device=DEV, seed=seed, global_offset=global_offset, auto_reset=auto_reset, assign=assign,
                          reward=(0.0, 1.0, 0.0))
    if (L, M) == (10, 40):
        f = load_golden("carved_L10_M40.npz")
        pick = np.resize(np.arange(f["rows"].shape[0]), n_cfg)
        rows = torch.from_numpy(f["rows"][pick].astype(np.uint16).view(np.int16)).to(DEV)
        pieces = torch.from_numpy(np.ascontiguousarray(f["pieces"][pick][:, :M + 1])).to(DEV)
    else:
        rows, pieces = env.synthetic_configs(n_cfg)
    env.load_configs(rows, pieces)
    env.reset()
    return env, rows, pieces


def _twin(oracle, env, rows, pieces):
    cpu = oracle.Env(env.num_envs, env.L, env.M, env.global_offset, env.seed)
    cpu.set_pool(_np(rows).view(np.uint16), _np(pieces))
    cpu.set_options(auto_reset=env.auto_reset, assign_mode=MODES[env.assign], per_line=0.0, win=1.0, lose=0.0)
    cpu.reset()
    return cpu


def _oracle_index(cpu, n):
    return np.array([cpu.assign(i, cpu.birth(i)) for i in range(n)], dtype=np.int64)


def _cells(rows_u16):
    return ((rows_u16[:, :, None] >> np.arange(10)) & 1).astype(bool)


def _check_dealt_boards(env, rows, index):
    """Independent of any mirror: a board that has not moved yet IS the pool entry it was dealt."""
    cells, _, _, _, m_rem, state = env.get_state()
    fresh = (_np(m_rem) == env.M) & (_np(state) == 0)
    want = _cells(_np(rows).view(np.uint16))[index[fresh]]
    assert np.array_equal(_np(cells)[fresh], want)
    return int(fresh.sum())


# ---------------------------------------------------------------------------------------------------------------- config_index
@pytest.mark.parametrize("assign", ["hash", "sequential"])
@pytest.mark.parametrize("n_cfg", [1, 7, 200])
@pytest.mark.parametrize("n,game", [(96, (1, 2)), (96, (2, 3)), (2080, (2, 3)), (96, (10, 40)), (2080, (10, 40))])
def test_config_index_is_the_oracles_assignment_and_the_board_that_was_dealt(oracle, assign, n_cfg, n, game):
    env, rows, pieces = _make(*game, n, n_cfg, assign)
    cpu = _twin(oracle, env, rows, pieces)
    slot = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    index = _np(T.config_index(env, slot=slot)).astype(np.int64)
    assert np.array_equal(index, _oracle_index(cpu, n)) and not _np(slot).any()
    assert _check_dealt_boards(env, rows, index) == n
    seen_fresh = 0
    for t in range(40):
        a = env.synthetic_actions(t)
        env.step(a, observe=False)
        cpu.step(_np(a))
        if t in (0, 1, 2, 5, 17, 39):
            index = _np(T.config_index(env)).astype(np.int64)
            assert np.array_equal(index, _oracle_index(cpu, n)), t
            seen_fresh += _check_dealt_boards(env, rows, index)
    assert index.min() >= 0 and index.max() < n_cfg
    assert seen_fresh > 0                                   # the dealt-board check did see boards dealt by an auto-reset
    env.terminate()


def test_config_index_under_a_global_offset_past_2_to_the_33(oracle):
    env, rows, pieces = _make(2, 3, 96, 200, "hash", global_offset=(1 << 33) + 5)
    cpu = _twin(oracle, env, rows, pieces)
    for t in range(7):
        a = env.synthetic_actions(t)
        env.step(a, observe=False)
        cpu.step(_np(a))
    index = _np(T.config_index(env)).astype(np.int64)
    assert np.array_equal(index, _oracle_index(cpu, 96))
    assert np.array_equal(index, _m().assign_entries(np.arange(96), [cpu.birth(i) for i in range(96)], env.seed, (1 << 33) + 5, 200, 0))
    _check_dealt_boards(env, rows, index)
    env.terminate()


@pytest.mark.parametrize("assign", ["hash", "sequential"])
def test_finished_boards_keep_the_index_they_finished_with(oracle, assign):
    n = 96
    env, rows, pieces = _make(2, 3, n, 7, assign, auto_reset=False)
    cpu = _twin(oracle, env, rows, pieces)
    kept = T.config_index(env)
    for t in range(6):
        a = env.synthetic_actions(t)
        env.step(a, observe=False)
        cpu.step(_np(a))
        assert T.config_index(env, out=kept) is kept
        assert np.array_equal(_np(kept).astype(np.int64), _oracle_index(cpu, n)), t
    state = _np(env.state)
    assert (state != 0).all()                               # M = 3: every board is frozen by now
    # a fresh buffer cannot know a frozen board's entry and says so
    assert (_np(T.config_index(env)) == -1).all()
    with pytest.raises(ValueError):
        T.config_index(env, out=kept.to(torch.int64))
    with pytest.raises(ValueError):
        T.config_index(env, out=kept[:-1])
    env.terminate()


# ---------------------------------------------------------------------------------------------------------------- the tally
def _play_and_count(env, tally, steps, n_cfgs, first_step=0, on_step=None):
    """`steps` steps with observe() before each; the expected tallies by np.bincount of the pre-step config_index over the boards
    that end, per slot: {slot: (episodes, wins)}, and the number of ends."""
    n = env.num_envs
    want = {s: (np.zeros(c, np.int64), np.zeros(c, np.int64)) for s, c in n_cfgs.items()}
    ends = 0
    index = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    slot = torch.empty(n, dtype=torch.uint8, device=DEV)
    for t in range(first_step, first_step + steps):
        if on_step is not None:
            on_step(t, want)
        a = env.synthetic_actions(t)
        running = _np(env.state) == 0
        T.config_index(env, out=index, slot=slot)
        tally.observe(a)
        _, reward, done, _ = env.step(a, observe=False)
        ended = _np(done) & running
        won = ended & (_np(reward) == 1.0)
        idx, sl = _np(index).astype(np.int64), _np(slot)
        for s in want:
            here = sl == s
            want[s][0][:] += np.bincount(idx[ended & here], minlength=want[s][0].size)
            want[s][1][:] += np.bincount(idx[won & here], minlength=want[s][0].size)
        ends += int(ended.sum())
    return want, ends


@pytest.mark.parametrize("assign", ["hash", "sequential"])
@pytest.mark.parametrize("n_cfg", [1, 7, 200])
@pytest.mark.parametrize("n,game", [(96, (1, 2)), (2080, (1, 2)), (96, (2, 3)), (2080, (2, 3))])
def test_tally_is_the_bincount_of_the_config_index_over_the_boards_that_end(assign, n_cfg, n, game):
    env, rows, pieces = _make(*game, n, n_cfg, assign)
    tally = T.PoolTally(env)
    assert tally.episodes.dtype == torch.int32 and tuple(tally.episodes.shape) == (n_cfg,) and tally.previous_episodes is None
    before = env.stats()
    want, ends = _play_and_count(env, tally, 40, {0: n_cfg})
    after = env.stats()
    episodes, wins = _np(tally.episodes).astype(np.int64), _np(tally.wins).astype(np.int64)
    assert episodes.sum() == ends == after["episodes"] - before["episodes"] and ends > 0
    assert wins.sum() == after["wins"] - before["wins"]
    assert np.array_equal(episodes, want[0][0]) and np.array_equal(wins, want[0][1])
    assert (wins <= episodes).all()
    tally.zero()
    assert not _np(tally.episodes).any() and not _np(tally.wins).any()
    env.terminate()


def test_tally_counts_wins_on_the_carved_pool_under_a_policy_that_wins():
    """The carved L = 10 / M = 40 fixture under the one-ply classical weights: wins are not rare, entries differ."""
    n, n_cfg = 2080, 200
    env, rows, pieces = _make(10, 40, n, n_cfg)
    res = T.evaluate_heuristic(env, T.CLASSICAL_WEIGHTS, None, 60, per_config=True)
    again = T.evaluate_heuristic(env, T.CLASSICAL_WEIGHTS, None, 60, per_config=True)
    plain = T.evaluate_heuristic(env, T.CLASSICAL_WEIGHTS, None, 60)
    assert set(plain) == {"episodes", "wins", "win_rate"} and set(res) == set(plain) | {"episodes_by_config", "wins_by_config"}
    for k in plain:
        assert np.array_equal(res[k], plain[k])
    e, w = _np(res["episodes_by_config"]).astype(np.int64), _np(res["wins_by_config"]).astype(np.int64)
    assert e.shape == (n_cfg,) and e.sum() == int(res["episodes"].sum()) and w.sum() == int(res["wins"].sum()) and w.sum() > 0
    assert torch.equal(res["episodes_by_config"], again["episodes_by_config"]) and torch.equal(res["wins_by_config"], again["wins_by_config"])
    with pytest.raises(ValueError):
        T.evaluate_heuristic(env, T.CLASSICAL_WEIGHTS, None, 60, per_config=1)
    env.terminate()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64])
def test_tally_with_auto_reset_off_counts_each_board_once(dtype):
    n, n_cfg = 96, 7
    env, rows, pieces = _make(2, 3, n, n_cfg, auto_reset=False)
    tally = T.PoolTally(env)
    index = T.config_index(env)
    first = _np(index).astype(np.int64)
    wins = np.zeros(n, bool)
    for t in range(8):                                      # M = 3: every board ends within three steps, then stays frozen
        a = env.synthetic_actions(t).to(dtype)
        tally.observe(a)
        _, reward, _, _ = env.step(a, observe=False)
        wins |= _np(reward) == 1.0
    assert (_np(env.state) != 0).all()
    assert np.array_equal(_np(tally.episodes), np.bincount(first, minlength=n_cfg))
    assert np.array_equal(_np(tally.wins), np.bincount(first[wins], minlength=n_cfg))
    assert int(_np(tally.episodes).sum()) == n == env.stats()["episodes"] and int(_np(tally.wins).sum()) == env.stats()["wins"]
    with pytest.raises(ValueError):
        tally.observe(a.to(torch.int16))
    with pytest.raises(ValueError):
        tally.observe(a[:-1])
    env.terminate()


@pytest.mark.parametrize("n", [96, 2080])
def test_tally_across_a_pool_swap(n):
    env, rows, pieces = _make(2, 3, n, 7)
    tally = T.PoolTally(env)
    second = env.synthetic_configs(200, seed=99)
    state = {}

    def on_step(t, want):
        if t == 10:
            with pytest.raises(ValueError):
                tally.swap()                                # nothing was loaded yet
            env.load_configs(*second)
            with pytest.raises(ValueError):
                tally.observe(env.synthetic_actions(t))     # loaded, not swapped: the tally would count into the wrong pool
            tally.swap()
            state["slot"] = env.pool_info()["current_slot"]
            want[state["slot"]] = (np.zeros(200, np.int64), np.zeros(200, np.int64))

    before = env.stats()
    want, ends = _play_and_count(env, tally, 40, {0: 7}, on_step=on_step)
    new, old = state["slot"], state["slot"] ^ 1
    assert (new, old) == (1, 0)
    assert tuple(tally.episodes.shape) == (200,) and tuple(tally.previous_episodes.shape) == (7,)
    for got, exp in ((tally.previous_episodes, want[old][0]), (tally.previous_wins, want[old][1]), (tally.episodes, want[new][0]),
                     (tally.wins, want[new][1])):
        assert np.array_equal(_np(got).astype(np.int64), exp)
    total = int(_np(tally.episodes).sum()) + int(_np(tally.previous_episodes).sum())
    assert total == ends == env.stats()["episodes"] - before["episodes"]
    assert int(_np(tally.episodes).sum()) > 0 and int(_np(tally.previous_episodes).sum()) > 0
    assert int(_np(tally.wins).sum()) + int(_np(tally.previous_wins).sum()) == env.stats()["wins"] - before["wins"]
    env.terminate()


@pytest.mark.parametrize("game", GAMES)
def test_observe_writes_nothing_to_the_environment(game):
    env, rows, pieces = _make(*game, 2080, 7)
    tally = T.PoolTally(env)
    for t in range(5):
        env.step(env.synthetic_actions(t), observe=False)
    a = env.synthetic_actions(5)
    before, stats = env._workspace.clone(), env.stats()     # both planes, the clocks and the statistics live in the workspace
    planes = env.raw_planes()
    tally.observe(a)
    T.config_index(env)
    torch.cuda.synchronize()
    assert torch.equal(env._workspace, before) and env.stats() == stats
    assert all(torch.equal(x, y) for x, y in zip(env.raw_planes(), planes))
    env.terminate()


# ---------------------------------------------------------------------------------------------------------------- resample_pool
def _host_pool(n_cfg, M, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 10, (n_cfg, 20), dtype=np.uint16), rng.integers(0, 7, (n_cfg, M + 1), dtype=np.uint8)


def _resample_both(rows, pieces, weights, count, seed=0, round=0):
    got = T.resample_pool(torch.from_numpy(rows.view(np.int16)).to(DEV), torch.from_numpy(pieces).to(DEV),
                          torch.from_numpy(weights).to(DEV), count, seed, round)
    want = _m().pool_resample(rows, pieces, weights, count, seed, round)
    assert got[0].dtype == torch.int16 and got[1].dtype == torch.uint8 and got[2].dtype == torch.int32
    assert np.array_equal(_np(got[0]).view(np.uint16), want[0]) and np.array_equal(_np(got[1]), want[1])
    assert np.array_equal(_np(got[2]), want[2])
    return want[2]


@pytest.mark.parametrize("M", [2, 40])                      # M + 1 = 3 and 41: neither a multiple of 4
@pytest.mark.parametrize("count", [1, 63, 64, 1000])
def test_resample_pool_equals_its_mirror_byte_for_byte(M, count):
    rows, pieces = _host_pool(37, M, seed=count)
    weights = np.random.default_rng(1).integers(0, 5, 37).astype(np.int64)
    weights[[0, 5, 36]] = 0
    source = _resample_both(rows, pieces, weights, count, seed=3, round=2)
    assert (weights[source] > 0).all()
    one = np.zeros(37, np.int64)
    one[36] = 4
    assert (_resample_both(rows, pieces, one, count) == 36).all()


def test_resample_pool_at_large_totals_large_pools_and_the_pinned_split():
    rows, pieces = _host_pool(5, 2)
    _resample_both(rows, pieces, np.array([(1 << 59) + 3, 0, (1 << 60) - 1, 1, (1 << 59)], np.int64), 1000, seed=11)
    _resample_both(rows, pieces, np.array([0, 0, (1 << 62) - 1, 0, 0], np.int64), 64)
    rows, pieces = _host_pool(2, 2)
    assert int((_resample_both(rows, pieces, np.array([1, 3], np.int64), 4096) == 1).sum()) == 3111
    rows, pieces = _host_pool(5000, 40)                      # a search of thirteen levels, draws over many blocks
    weights = np.random.default_rng(2).integers(0, 1 << 40, 5000).astype(np.int64)
    _resample_both(rows, pieces, weights, 4097, seed=(1 << 64) - 1, round=(1 << 40) + 1)
    with pytest.raises(ValueError, match="negative"):
        T.resample_pool(torch.from_numpy(rows.view(np.int16)).to(DEV), torch.from_numpy(pieces).to(DEV),
                        torch.full((5000,), -1, dtype=torch.int64, device=DEV), 8)


# ---------------------------------------------------------------------------------------------------------------- PoolCurriculum
def test_pool_curriculum_folds_reweights_resamples_and_loads():
    n, n_base, M = 2080, 200, 3
    env = T.BatchedTetris(2, M, n, device=DEV, seed=2, auto_reset=True, reward=(0.0, 1.0, 0.0))
    rows, pieces = env.synthetic_configs(n_base)
    cur = T.PoolCurriculum(env, rows, pieces, seed=4, floor=1, gain=8)
    env.reset()
    assert np.array_equal(_np(cur.source), np.arange(n_base)) and env.n_configs == n_base and cur.count == n_base
    action = torch.zeros(n, dtype=torch.uint8, device=DEV)   # the policy that always plays action 0
    for _ in range(30):
        cur.observe(action)
        env.step(action, observe=False)
    e0, w0 = _np(cur.tally.episodes).astype(np.int64), _np(cur.tally.wins).astype(np.int64)
    assert e0.sum() == env.stats()["episodes"] and w0.sum() == env.stats()["wins"] and e0.sum() > 0
    assert cur.refresh() is True
    # the first pool is the base pool: folding through source = arange is the tallies themselves
    assert np.array_equal(_np(cur.base_episodes), e0) and np.array_equal(_np(cur.base_wins), w0)
    assert cur.base_episodes.dtype == torch.int64 and not _np(cur.tally.episodes).any()
    weights = _m().curriculum_weights(e0, w0, 1, 8)
    assert np.array_equal(_np(cur.weights()), weights)
    want = _m().pool_resample(_np(rows).view(np.uint16), _np(pieces), weights, n_base, seed=4, round=0)
    loaded_rows, loaded_pieces = env._pool
    assert np.array_equal(_np(loaded_rows).view(np.uint16), want[0]) and np.array_equal(_np(loaded_pieces), want[1])
    assert np.array_equal(_np(cur.source), want[2])
    rate = _np(cur.base_win_rate())
    assert np.allclose(rate, w0 / np.maximum(e0, 1)) and rate.dtype == np.float64
    # the other buffer is still in use: nothing changes
    assert env.pool_info()["steps_until_swap"] > 0
    generation, source = env.pool_generation, cur.source.clone()
    assert cur.refresh() is False
    assert env.pool_generation == generation and torch.equal(cur.source, source) and cur.refreshes == 1
    assert np.array_equal(_np(cur.base_episodes), e0)
    # on: boards of the old buffer finish into the previous pair, new episodes into the current one; the second refresh folds both
    for _ in range(2 * M + 1):                              # under this policy every episode lasts M steps, all boards in lockstep
        cur.observe(action)
        env.step(action, observe=False)
    e1, w1 = _np(cur.tally.episodes).astype(np.int64), _np(cur.tally.wins).astype(np.int64)
    ep, wp = _np(cur.tally.previous_episodes).astype(np.int64), _np(cur.tally.previous_wins).astype(np.int64)
    assert ep.sum() > 0 and e1.sum() > 0
    assert cur.refresh() is True and cur.refreshes == 2
    base_e, base_w = e0 + ep, w0 + wp
    np.add.at(base_e, want[2], e1)
    np.add.at(base_w, want[2], w1)
    assert np.array_equal(_np(cur.base_episodes), base_e) and np.array_equal(_np(cur.base_wins), base_w)
    assert int(base_e.sum()) == env.stats()["episodes"] and int(base_w.sum()) == env.stats()["wins"]
    want2 = _m().pool_resample(_np(rows).view(np.uint16), _np(pieces), _m().curriculum_weights(base_e, base_w, 1, 8), n_base, seed=4,
                               round=1)
    assert np.array_equal(_np(cur.source), want2[2]) and np.array_equal(_np(env._pool[0]).view(np.uint16), want2[0])
    with pytest.raises(ValueError):
        T.PoolCurriculum(env, rows, pieces[:, :3])
    env.terminate()


# ---------------------------------------------------------------------------------------------------------------- the hooks
def _learner_env(n=256):
    env = T.BatchedTetris(2, 3, n, device=DEV, seed=7, auto_reset=True)
    rows, pieces = env.synthetic_configs(64)
    env.load_configs(rows, pieces)
    env.reset()
    return env, rows, pieces


def test_learner_hooks_change_nothing_by_default_and_count_every_episode_with_a_curriculum():
    tables = []
    for kwargs in (None, dict(curriculum=None), dict(curriculum=None, refresh_every=0)):
        env, _, _ = _learner_env()
        learner = T.NTupleLearner(env, seed=1)
        learner.train(50) if kwargs is None else learner.train(50, **kwargs)
        tables.append(learner.table.clone())
        with pytest.raises(ValueError):
            learner.train(1, refresh_every=5)               # refresh_every needs a curriculum
        env.terminate()
    assert torch.equal(tables[0], tables[1]) and torch.equal(tables[0], tables[2]) and bool(tables[0].any())
    env, rows, pieces = _learner_env()
    learner = T.NTupleLearner(env, seed=1)
    cur = T.PoolCurriculum(env, rows, pieces, loaded=True)
    learner.train(50, curriculum=cur, refresh_every=10)
    assert cur.refreshes == 5
    cur.fold()
    assert int(cur.base_episodes.sum()) == env.stats()["episodes"] and int(cur.base_wins.sum()) == env.stats()["wins"]
    other, _, _ = _learner_env()
    with pytest.raises(ValueError):
        T.NTupleLearner(other, seed=1).train(1, curriculum=cur)
    other.terminate()
    env.terminate()


def test_learner_evaluate_per_config_totals_and_repeatability():
    env, _, _ = _learner_env()
    learner = T.NTupleLearner(env, seed=1)
    learner.train(20)
    plain = learner.evaluate(30)
    res, again = learner.evaluate(30, per_config=True), learner.evaluate(30, per_config=True)
    assert {k: res[k] for k in plain} == plain and set(res) == set(plain) | {"episodes_by_config", "wins_by_config"}
    assert tuple(res["episodes_by_config"].shape) == (64,) and res["episodes_by_config"].dtype == torch.int32
    assert int(res["episodes_by_config"].sum()) == res["episodes"] > 0 and int(res["wins_by_config"].sum()) == res["wins"]
    assert torch.equal(res["episodes_by_config"], again["episodes_by_config"]) and torch.equal(res["wins_by_config"], again["wins_by_config"])
    with pytest.raises(ValueError):
        learner.evaluate(30, per_config="yes")
    env.terminate()
