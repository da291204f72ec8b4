"""Host pins of the learner's references (tests/learn_ref.py), no GPU needed: the observation built from decoded fields is
the CPU oracle's expand_obs bit for bit over the game range, the state layout round-trips at every field's limits, and the
fallback draw that test_learn_range_gpu.py runs on the device really takes the fallback."""
import numpy as np
import pytest

import learn_ref as R


def _random_boards(oracle, L, M, n, steps, seed):
    """An oracle.Env of n boards after `steps` random steps with auto-reset off: running, won, lost and topped-out boards."""
    env = oracle.Env(n, L, M, 0, seed)
    rows = oracle.synth_boards(seed, 0, 64, L)
    pieces = oracle.synth_pieces(seed, 0, 64, M)
    env.set_pool(rows, pieces)
    env.set_options(auto_reset=False, assign_mode=0)
    env.reset()
    gen = np.random.default_rng(seed)
    snaps = []
    for t in range(steps):
        env.step(gen.integers(0, 40, n).astype(np.int64))
        snaps.append((env.get_state(), env.expand_obs()))
    env.close()
    return snaps


# the states random play reaches (2 is lost at the move limit or by top-out; top-outs are the 2s with moves < M)
REACHED = {(1, 1): {1, 2}, (1, 3): {0, 1, 2}, (5, 20): {0, 2}, (10, 40): {0, 2}, (250, 254): {0, 2}}


@pytest.mark.parametrize("L,M", sorted(REACHED))
def test_obs_from_fields_is_the_oracle_observation(oracle, L, M):
    seen, topouts = set(), 0
    for fields, obs in _random_boards(oracle, L, M, 512, min(M + 2, 48), seed=L + M):
        want = obs.astype(np.float32)
        got = R.obs_from_fields(fields, L, M)
        assert got.dtype == np.float64
        assert np.array_equal(got.astype(np.float32).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got, want.astype(np.float64))            # every feature is exact in float32
        seen |= set(np.unique(fields["state"]).tolist())
        topouts += int(((fields["state"] == 2) & (fields["moves"] < M)).sum())
    assert seen == REACHED[(L, M)] and (topouts > 0 or L == 1), (seen, topouts)


def test_state_layout_round_trips_at_every_limit():
    gen = np.random.default_rng(0)
    f = R.random_fields(gen, 4096)
    # every single bit of every field on its own as well
    k = np.arange(36)
    f1 = dict(rows=np.zeros((36, 20), np.uint16), lines=np.zeros(36), moves=np.zeros(36), state=np.zeros(36),
              slot=np.zeros(36), window=(np.uint64(1) << k.astype(np.uint64)))
    for fields in (f, f1):
        A, B = R.pack_state(**fields)
        d = R.decode_state(A, B)
        assert np.array_equal(d["rows"], fields["rows"])
        for key in ("lines", "moves", "state", "slot"):
            assert np.array_equal(d[key], np.asarray(fields[key]).astype(np.uint8)), key
        assert np.array_equal(d["window"], np.asarray(fields["window"], dtype=np.uint64))
        assert np.array_equal(d["cur"], (d["window"] & np.uint64(7)).astype(np.uint8))
        A2, B2 = R.pack_state(d["rows"], d["lines"], d["moves"], d["state"], d["slot"], d["window"])
        assert np.array_equal(A2, A) and np.array_equal(B2, B)
    # the fields cover their ranges and bit 31 of B.y is never set
    assert set(f["state"]) == {0, 1, 2, 3} and set(f["slot"]) == {0, 1}
    A, B = R.pack_state(**f)
    assert not (B[:, 1] >> np.uint32(31)).any()
    moves = np.arange(256)
    A, B = R.pack_state(np.zeros((256, 20), np.uint16), 255 - moves, moves, 0, 0, 0)
    d = R.decode_state(A, B)
    assert np.array_equal(d["moves"], moves) and np.array_equal(d["lines"], 255 - moves)
    # one set cell at every (row, column): one bit in one column word
    rows = np.zeros((200, 20), np.uint16)
    rows[np.arange(200), np.arange(200) // 10] = 1 << (np.arange(200) % 10)
    A, B = R.pack_state(rows, 0, 0, 0, 0, 0)
    words = np.concatenate([A, B], axis=1)
    assert (np.array([bin(int(w)).count("1") for w in words.ravel()]).reshape(200, 8).sum(1) == 1).all()
    assert np.array_equal(R.decode_state(A, B)["rows"], rows)


def test_decode_records_reads_every_field_of_the_record():
    gen = np.random.default_rng(1)
    k = 300
    f = R.random_fields(gen, k)
    A, B = R.pack_state(**f)
    na, nb = gen.integers(0, 1 << 32, (k, 4), dtype=np.uint64).astype(np.uint32), gen.integers(0, 1 << 32, (k, 4), dtype=np.uint64).astype(np.uint32)
    rec = np.zeros((k, 80), np.uint8)
    rec[:, 0:16], rec[:, 16:32] = A.view(np.uint8).reshape(k, 16), B.view(np.uint8).reshape(k, 16)
    rec[:, 32:48], rec[:, 48:64] = na.view(np.uint8).reshape(k, 16), nb.view(np.uint8).reshape(k, 16)
    rbits = gen.integers(0, 1 << 32, k, dtype=np.uint64).astype(np.uint32)
    rec[:, 64:68] = rbits.view(np.uint8).reshape(k, 4)
    rec[:, 68], rec[:, 69] = gen.integers(0, 40, k), gen.integers(0, 2, k)
    rec[:, 70:80] = gen.integers(0, 256, (k, 10))
    d = R.decode_records(rec)
    assert np.array_equal(d["s"]["rows"], f["rows"]) and np.array_equal(d["s"]["window"], f["window"])
    assert np.array_equal(d["sa"], A) and np.array_equal(d["sb"], B)
    assert np.array_equal(d["na"], na) and np.array_equal(d["nb"], nb)
    assert np.array_equal(d["reward_bits"], rbits)
    assert np.array_equal(d["action"], rec[:, 68]) and np.array_equal(d["done"], rec[:, 69])
    assert np.array_equal(d["tail"], rec[:, 70:80])


def test_obs_from_fields_of_decoded_states_has_the_documented_features():
    gen = np.random.default_rng(2)
    f = R.random_fields(gen, 2048, M=254)
    d = R.decode_state(*R.pack_state(**f))
    obs = R.obs_from_fields(d, 250, 254)
    cur, nxt = d["cur"].astype(int), d["nxt"].astype(int)
    assert set(cur) == set(range(8)) and set(nxt) == set(range(8))
    assert np.array_equal(obs[:, 200:207].sum(1), (cur < 7).astype(float))
    assert np.array_equal(obs[:, 207:214].sum(1), (nxt < 7).astype(float))
    assert obs[:, 214].min() == 250 - 255 and obs[:, 215].max() == 254 and obs[:, 215].min() == 0
    assert np.array_equal(obs[:, 216], (np.asarray(f["state"]) != 0).astype(float))
    assert np.array_equal(obs[:, :200].sum(1), [sum(bin(int(r)).count("1") for r in row) for row in f["rows"]])


# ------------------------------------------------------------------------------------------------ the descent's fallback
# A tree of exact sums (1 + 2 + 4 + 8 = 15 at slots 0, 17, 4095, 4496 of 4500).  With these keys the last of 2^20 + 1
# stratified targets rounds to the total: (B - 1) + U_i == B in float64.  At the root u = total is taken by no child (u equals
# the last child's sum after the subtractions), so the descent falls back to the last child with c_k > 0 and goes on with
# u = 0; a first-child fallback would end at slot 0 instead.
FALLBACK = dict(capacity=4500, slots=(0, 17, 4095, 4496), leaves=(1.0, 2.0, 4.0, 8.0), seed=0, update=47497320171,
                batch=(1 << 20) + 1)


def fallback_tree(L):
    tree = L.priority_tree_init(FALLBACK["capacity"])
    L.priority_tree_update(tree, np.array(FALLBACK["slots"]), np.array(FALLBACK["leaves"]))
    return tree


def _descend(tree, u, L, fallback):
    """One draw's descent in plain Python floats; `fallback` picks the child when none takes u ("last" or "first")."""
    offsets, _, _ = L.priority_layout(int(tree.view(np.int64)[1]))
    j, used = 0, 0
    for k in range(len(offsets) - 1, 0, -1):
        line = [float(x) for x in tree[offsets[k - 1] + 16 * j: offsets[k - 1] + 16 * j + 16]]
        pick = None
        for c, x in enumerate(line):
            if u < x:
                pick = c
                break
            u -= x
        if pick is None:
            live = [c for c, x in enumerate(line) if x > 0]
            pick = live[-1] if fallback == "last" else live[0]
            used += 1
        j = 16 * j + pick
    return j, used


def test_the_fallback_draw_takes_the_fallback():
    import tetris_piclim as T
    L = T._learn_lib
    tree = fallback_tree(L)
    offsets, _, _ = L.priority_layout(FALLBACK["capacity"])
    total = tree[offsets[-1]]
    assert total == 15.0
    B = FALLBACK["batch"]
    u = L.priority_targets(FALLBACK["seed"], FALLBACK["update"], B, total)
    assert u[-1] == total and (u[:-1] < total).all()
    assert L.lib().tpl_priority_target(FALLBACK["seed"], FALLBACK["update"], B - 1, B, total) == total
    slot, used = _descend(tree, float(u[-1]), L, "last")
    assert used == 1 and slot == 4496
    first, _ = _descend(tree, float(u[-1]), L, "first")
    assert first == 0                                                     # a first-child fallback would draw slot 0
    idx, prob = L.prioritized_draws(tree, FALLBACK["seed"], FALLBACK["update"], B)
    assert idx[-1] == 4496 and prob[-1] == np.float32(8.0 / 15.0)
    assert set(np.unique(idx)) == set(FALLBACK["slots"])
    # the other draws agree with the plain descent as well (a sample of them)
    for i in np.random.default_rng(0).choice(B - 1, 200, replace=False):
        assert _descend(tree, float(u[i]), L, "last")[0] == idx[i]
