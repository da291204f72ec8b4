"""The ranking update from proved move labels on one MI355X (include/tpl_learn.h's rule under tpl_ntuple_rank;
csrc/learn/ntuple_rank.hip; T.NTupleRanker, T.LabelSet, T.collect_labels, T.label_agreement).  THE KERNEL IS THE MIRROR, byte for byte in
all eleven outputs, through guard-framed buffers filled with 0xCD; tests/test_ntuple_rank_cpu.py pins the mirror and makes the nodes:

  1. all four forms, the prune off and on for the budget form, at n = 1, 8, 9 and 203 (a partial last block): the 128 labelled nodes
     of the CPU tests and 75 variants of them in the same launch -- finished boards, rows of random bytes, rows without a 1, rows
     without a 2 --, under tables of random small integers;
  2. greedy is NTuplePolicy.act() at epsilon 0, and the win afterstate is act(after=) where win == greedy;
  3. one step leaves the mirror's table bytes, for every form, symmetric and not; a symmetric step keeps a symmetric table symmetric;
     the same start twice gives the same bytes;
  4. collect_labels on 64 boards over a pool keeps exactly the decided boards, with the environment's planes at that step, and leaves
     the environment where the same actions leave it;
  5. NTupleRanker.fit reproduces the CPU test's per-epoch violated counts and the mirror's table, and label_agreement its figures;
  6. every Python refusal.
"""
import numpy as np
import pytest
import torch

import learn_ref as R
import tetris_piclim as T
from conftest import load_golden
from test_learn_range_gpu import Framed, _check, _stream
from test_learner_gpu import _np
from test_ntuple_rank_cpu import (FIT, FIT_COUNTS, FIT_REWARD, GAMMA, L5, M10, REWARD, all_nodes, fitted, rank_nodes, small_table)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORMS = [("2x4", False), ("3x3", False), ("feat", False), ("feat+spare", False), ("feat+spare", True)]
U8, F32, PLANES = ("win", "loss", "greedy", "violated"), ("gap", "err_win", "err_loss"), ("win_a", "win_b", "loss_a", "loss_b")


def _m():
    return T._learn_lib


def planes_of(nodes, seed=1):
    """The 32-byte states of nodes in row form: window entries 0 and 1 the node's two pieces, the ten behind them, the slot and the
    spare bit random.  (A, B) uint32 [K, 4] and the window, slot and spare they were packed with."""
    gen = np.random.default_rng(seed)
    k = nodes["rows"].shape[0]
    window = (nodes["piece"][:, 0].astype(np.uint64) | (nodes["piece"][:, 1].astype(np.uint64) << np.uint64(3))
              | (gen.integers(0, 1 << 30, k, dtype=np.int64).astype(np.uint64) << np.uint64(6)))
    slot, spare = gen.integers(0, 2, k), gen.integers(0, 2, k).astype(np.uint32)
    A, B = R.pack_state(nodes["rows"], nodes["lines"], nodes["moves"], nodes["state"], slot, window)
    B[:, 1] |= spare << np.uint32(31)
    return A, B, dict(window=window, slot=slot, spare=spare)


def expected_planes(out, side, A, B, extra):
    """The afterstate planes the mirror's row form packs to: the window popped by one entry, the slot and the spare bit kept; an
    undecided node's are the state itself."""
    f = out[side + "_fields"]
    A2, B2 = R.pack_state(out[side + "_rows"], f[:, 0], f[:, 1], f[:, 2], extra["slot"], extra["window"] >> np.uint64(3))
    B2[:, 1] |= extra["spare"] << np.uint32(31)
    decided = (out["win"] != 255)[:, None]
    return np.where(decided, A2, A), np.where(decided, B2, B)


@pytest.fixture(scope="module")
def boards():
    """203 boards: the 128 nodes, then 75 variants of them -- finished in each of the three ways, a row of random bytes, a row whose
    1s became 3s (empty W), a row whose 2s became 0s (empty X)."""
    base = all_nodes()
    gen = np.random.default_rng(7)
    idx = np.concatenate([np.arange(128), (np.arange(75) * 5) % 128])
    nodes = {k: np.array(base[k][idx]) for k in ("rows", "lines", "moves", "state", "piece", "label")}
    for j in range(128, 203):
        kind = j % 6
        if kind < 3:
            nodes["state"][j] = kind + 1
        elif kind == 3:                                        # any byte, and in half the places a small one, so that some rows decide
            row, small = gen.integers(0, 256, 40), gen.random(40) < 0.5
            row[small] = gen.integers(0, 4, int(small.sum()))
            nodes["label"][j] = row
        elif kind == 4:
            nodes["label"][j][nodes["label"][j] == 1] = 3
        else:
            nodes["label"][j][nodes["label"][j] == 2] = 0
    A, B, extra = planes_of(nodes)
    return dict(nodes=nodes, A=A, B=B, extra=extra)


def _pick(boards, sel):
    nodes = {k: np.ascontiguousarray(v[sel]) for k, v in boards["nodes"].items()}
    extra = {k: v[sel] for k, v in boards["extra"].items()}
    return nodes, np.ascontiguousarray(boards["A"][sel]), np.ascontiguousarray(boards["B"][sel]), extra


def _framed(host, seed):
    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    f = Framed(raw.size, seed)
    f.inner().copy_(torch.from_numpy(raw))
    return f


def _launch(A, B, table, label, reward, gamma, margin, prune):
    """tpl_ntuple_rank through guard-framed buffers, every output filled with 0xCD first: the eleven outputs on the host."""
    n = A.shape[0]
    a, b, t, lab = _framed(A, 1), _framed(B, 2), _framed(table, 3), _framed(label, 4)
    sizes = {**{k: n for k in U8}, **{k: 4 * n for k in F32}, **{k: 16 * n for k in PLANES}}
    out = {k: Framed(sizes[k], 10 + j) for j, k in enumerate(U8 + F32 + PLANES)}
    for f in out.values():
        f.inner().fill_(0xCD)
    _check(_m().lib().tpl_ntuple_rank(a.ptr(), b.ptr(), n, L5, M10, t.ptr(), table.shape[0], lab.ptr(), *(float(r) for r in reward),
                                      float(gamma), float(margin), int(prune), *(out[k].ptr() for k in U8 + F32 + PLANES), _stream()))
    for k, f in list(out.items()) + [("a", a), ("b", b), ("table", t), ("label", lab)]:
        f.assert_canary((n, k))
    assert np.array_equal(t.host().view(np.int32), table) and np.array_equal(lab.host(), label.reshape(-1))     # read only
    assert np.array_equal(a.host(), A.view(np.uint8).reshape(-1)) and np.array_equal(b.host(), B.view(np.uint8).reshape(-1))
    got = {k: out[k].host().copy() for k in U8}
    got.update({k: out[k].host().view(np.float32).copy() for k in F32})
    got.update({k: out[k].host().view(np.uint32).reshape(n, 4).copy() for k in PLANES})
    return got


def _mirror(nodes, A, B, extra, table, reward, gamma, margin, prune):
    out = _m().ntuple_rank(table, nodes["rows"], nodes["piece"], L5, M10, nodes["lines"], nodes["moves"], nodes["state"], nodes["label"],
                           gamma, reward, margin, bool(prune))
    want = {k: out[k] for k in U8 + F32}
    want["win_a"], want["win_b"] = expected_planes(out, "win", A, B, extra)
    want["loss_a"], want["loss_b"] = expected_planes(out, "loss", A, B, extra)
    return want, out


def _same(got, want, what):
    for k in U8 + F32 + PLANES:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(g.view(np.uint8) != w.view(np.uint8))
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ 1. the kernels are the mirror
@pytest.mark.parametrize("n", [1, 8, 9, 203])
@pytest.mark.parametrize("form,prune", FORMS)
def test_all_eleven_outputs_are_the_mirrors_byte_for_byte(boards, form, prune, n):
    sel = np.arange(203) if n == 203 else (np.arange(n) * 23 + 120) % 203      # the small ones reach into the variants
    nodes, A, B, extra = _pick(boards, sel)
    table = small_table(form, 100 + n)
    margin = 0.25
    got = _launch(A, B, table, nodes["label"], REWARD, GAMMA, margin, prune)
    want, out = _mirror(nodes, A, B, extra, table, REWARD, GAMMA, margin, prune)
    _same(got, want, (form, prune, n))
    if n == 203:                                               # the launch holds every kind of node
        decided = out["win"] != 255
        assert decided.sum() > 128 and (~decided).sum() >= 45 and (nodes["state"] != 0).sum() >= 36
        assert 0 < out["violated"].sum() < decided.sum()
        assert (out["err_win"] == 1).any() and (out["err_loss"] == -1).any()
        assert (got["greedy"][nodes["state"] != 0] == 0).all()
        # a margin that a win's reward does not reach: a won child is violated and teaches nothing
        wide = 12.0
        got = _launch(A, B, table, nodes["label"], REWARD, GAMMA, wide, prune)
        want, out = _mirror(nodes, A, B, extra, table, REWARD, GAMMA, wide, prune)
        _same(got, want, (form, prune, n, wide))
        assert ((out["violated"] == 1) & (out["err_win"] == 0)).any() and ((out["violated"] == 1) & (out["err_win"] == 1)).any()


@pytest.mark.parametrize("form,prune", FORMS)
def test_the_zero_table_ties_everywhere_and_a_negative_margin_is_not_violated(boards, form, prune):
    nodes, A, B, extra = _pick(boards, np.arange(203))
    table = np.zeros(_m().ntuple_entries_of(form), np.int32)
    for margin in (0.0, -1.0):
        got = _launch(A, B, table, nodes["label"], (0.0, 0.0, 0.0), GAMMA, margin, prune)
        want, out = _mirror(nodes, A, B, extra, table, (0.0, 0.0, 0.0), GAMMA, margin, prune)
        _same(got, want, (form, prune, margin))
        decided = got["win"] != 255
        assert (got["gap"].view(np.uint32) == 0).all() and np.array_equal(got["violated"] == 1, decided & (margin == 0.0))


# ------------------------------------------------------------------------------------------------ 2. against the policy
@pytest.mark.parametrize("form,prune", FORMS)
def test_greedy_is_the_policys_action_and_the_win_afterstate_is_its_afterstate(boards, form, prune):
    n = 203
    env = T.BatchedTetris(L5, M10, n, device=DEV, seed=1, reward=REWARD)
    a, b = (torch.from_numpy(x.view(np.int32)).to(DEV) for x in (boards["A"], boards["B"]))
    env.write_raw_planes(a, b)
    table = torch.from_numpy(small_table(form, 31)).to(DEV)
    after = (torch.empty((n, 4), dtype=torch.int32, device=DEV), torch.empty((n, 4), dtype=torch.int32, device=DEV))
    action = T.NTuplePolicy(env, table, gamma=GAMMA, epsilon=0.0, bound=prune).act(after=after)
    label = torch.from_numpy(boards["nodes"]["label"]).to(DEV)
    out = T.NTupleRanker(table, L5, M10, gamma=GAMMA, reward=REWARD, bound=prune).rank((a, b), label)
    assert torch.equal(out["greedy"], action)
    same = out["win"] == out["greedy"]
    assert int(same.sum()) >= 20
    assert torch.equal(out["win_a"][same], after[0][same]) and torch.equal(out["win_b"][same], after[1][same])
    env.terminate()


# ------------------------------------------------------------------------------------------------ 3. one step
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("form,prune", FORMS)
def test_one_step_leaves_the_mirrors_table_bytes(boards, form, prune, symmetric):
    m = _m()
    nodes, A, B, _ = _pick(boards, np.arange(203))
    a, b = (torch.from_numpy(x.view(np.int32)).to(DEV) for x in (A, B))
    label = torch.from_numpy(nodes["label"]).to(DEV)
    start = small_table(form, 77)
    rate = 37.4
    want = start.copy()
    m.ntuple_rank_step(want, nodes["rows"], nodes["piece"], L5, M10, nodes["lines"], nodes["moves"], nodes["state"], nodes["label"],
                       GAMMA, REWARD, 0.0, prune, rate, symmetric)
    assert not np.array_equal(want, start)
    tables = []
    for _ in range(2):                                         # the same start twice: the same bytes
        table = torch.from_numpy(start).to(DEV)
        ranker = T.NTupleRanker(table, L5, M10, gamma=GAMMA, reward=REWARD, rate=rate, margin=0.0, bound=prune, symmetric=symmetric)
        out = ranker.step((a, b), label, ranker.buffers(203))
        assert out["violated"].sum() > 0
        tables.append(_np(table))
    assert np.array_equal(tables[0], want) and np.array_equal(tables[1], want)
    if symmetric:                                              # from a symmetric start the table stays symmetric
        table = T.ntuple_table(DEV, form)
        T.NTupleRanker(table, L5, M10, gamma=GAMMA, reward=REWARD, rate=rate, bound=prune, symmetric=True).step((a, b), label)
        assert table.any() and T.ntuple_is_symmetric(table)
        zero = np.zeros_like(start)
        m.ntuple_rank_step(zero, nodes["rows"], nodes["piece"], L5, M10, nodes["lines"], nodes["moves"], nodes["state"], nodes["label"],
                           GAMMA, REWARD, 0.0, prune, rate, True)
        assert np.array_equal(_np(table), zero)


# ------------------------------------------------------------------------------------------------ 4. collect_labels
def _collect_case(L, M, rows, pieces, steps, seed):
    n = 64
    table = torch.from_numpy(small_table("feat+spare", 5)).to(DEV)

    def make():
        env = T.BatchedTetris(L, M, n, device=DEV, seed=seed, auto_reset=False)
        env.load_configs(rows, pieces)
        env.reset()
        return env, T.NTuplePolicy(env, table, gamma=GAMMA, epsilon=0.0, bound=True)

    env, policy = make()
    got = T.collect_labels(env, pieces, policy, steps, max_nodes=1 << 10)
    # the same run by hand on a second environment
    twin, twin_policy = make()
    want = dict(a=[], b=[], label=[], entry=[])
    for _ in range(steps):
        labels = T.label_states(twin, pieces, max_nodes=1 << 10)
        row = labels["label"]
        keep = labels["running"] & (row == 1).any(dim=1) & (row == 2).any(dim=1)
        a, b = twin.raw_planes()
        want["a"].append(a[keep]); want["b"].append(b[keep]); want["label"].append(row[keep]); want["entry"].append(labels["entry"][keep])
        twin.step(twin_policy.act(), observe=False)
    assert isinstance(got, T.LabelSet) and len(got) == sum(int(x.shape[0]) for x in want["a"])
    assert torch.equal(got.planes_a, torch.cat(want["a"])) and torch.equal(got.planes_b, torch.cat(want["b"]))
    assert torch.equal(got.label, torch.cat(want["label"])) and torch.equal(got.entry, torch.cat(want["entry"]).to(torch.int32))
    assert got.planes_a.dtype == torch.int32 and got.label.dtype == torch.uint8 and got.entry.dtype == torch.int32
    if len(got):                                               # only decided, running nodes of pool entries
        assert bool(((got.label == 1).any(dim=1) & (got.label == 2).any(dim=1)).all())
        assert bool((((got.planes_b[:, 1] >> 28) & 3) == 0).all()) and bool(((got.entry >= 0) & (got.entry < rows.shape[0])).all())
    assert torch.equal(env.snapshot().data, twin.snapshot().data)          # the environment ends as the played run leaves it
    count = len(got)
    env.terminate(); twin.terminate()
    return count


def test_collect_labels_keeps_the_decided_boards_and_plays_the_environment_on():
    g = load_golden("carved_L5_M20.npz")
    # the whole game, from the reset: 64 boards, L = 5 / M = 20, two steps
    loose = _collect_case(L5, int(g["M"]), g["rows"][:32], g["pieces"][:32], 2, seed=5)
    # and a tight one, where proofs decide: the ten configurations solved in six moves, in the game (5, 6)
    six = np.flatnonzero(g["sol_len"][:32] == 6)
    tight = _collect_case(L5, 6, g["rows"][six], np.ascontiguousarray(g["pieces"][six][:, :7]), 2, seed=5)
    print("decided nodes kept: loose", loose, "tight", tight)
    assert tight > 0


# ------------------------------------------------------------------------------------------------ 5. fit
def _label_set(nodes):
    A, B, _ = planes_of(nodes, seed=2)
    s = T.LabelSet(DEV)
    return s.append(torch.from_numpy(A.view(np.int32)), torch.from_numpy(B.view(np.int32)), torch.from_numpy(np.array(nodes["label"])),
                    torch.arange(A.shape[0]))


def test_fit_on_the_device_reproduces_the_cpu_tests_counts_and_the_mirrors_table():
    nodes = rank_nodes()
    s = _label_set(nodes)
    assert len(s) == 96
    table = T.ntuple_table(DEV, "feat+spare")
    kw = dict(gamma=GAMMA, reward=FIT_REWARD, margin=0.0, bound=True)
    before = T.label_agreement(table, (s.planes_a, s.planes_b), s.label, L5, M10, **kw)
    counts = T.NTupleRanker(table, L5, M10, rate=FIT["rate"], **kw).fit(s, FIT["epochs"], FIT["batch"], seed=FIT["seed"])
    after = T.label_agreement(table, (s.planes_a, s.planes_b), s.label, L5, M10, **kw)
    print("before", before, "per epoch", counts, "after", after)
    assert counts == FIT_COUNTS[1]
    assert (before["violated"], before["greedy_win"]) == FIT_COUNTS[0] and (after["violated"], after["greedy_win"]) == FIT_COUNTS[2]
    assert before["decided"] == after["decided"] == before["nodes"] == 96
    assert after["greedy_win"] + after["greedy_loss"] + after["greedy_open"] == 96 and after["greedy_open"] == 0
    assert np.array_equal(_np(table), fitted()[0])
    # the held-out half of a split by entry shares no entry with the training half
    train, held = s.split(0.5)
    assert len(train) == 48 and len(held) == 48 and not set(train.entry.tolist()) & set(held.entry.tolist())


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_every_python_refusal(boards):
    m = _m()
    ok = T.ntuple_table(DEV, "feat+spare")
    for shape, staged in (("2x4+3x3", False), ("3x3+feat", False), ("2x4", True), ("3x3", True)):
        with pytest.raises(ValueError, match="four plain forms"):
            T.NTupleRanker(T.ntuple_table(DEV, shape, staged=staged), L5, M10)
    for form in ("2x4", "3x3", "feat"):
        with pytest.raises(ValueError, match="bound=True is the dead-board prune"):
            T.NTupleRanker(T.ntuple_table(DEV, form), L5, M10, bound=True)
    for bad in (dict(L=0), dict(L=251), dict(L=5.0), dict(M=0), dict(M=255), dict(M=True), dict(gamma=float("inf")), dict(gamma="1"),
                dict(rate=float("nan")), dict(margin=float("inf")), dict(margin=None), dict(reward=(1.0, 0.0)),
                dict(reward=(1.0, float("nan"), 0.0)), dict(reward="abc"), dict(bound=1), dict(symmetric=1)):
        with pytest.raises(ValueError):
            T.NTupleRanker(**{**dict(table=ok, L=L5, M=M10), **bad})
    with pytest.raises(ValueError, match="on a GPU"):
        T.NTupleRanker(torch.zeros(21504, dtype=torch.int32), L5, M10)
    with pytest.raises(ValueError, match="contiguous int32"):
        T.NTupleRanker(torch.zeros(2 * 21504, dtype=torch.int32, device=DEV)[::2], L5, M10)
    ranker = T.NTupleRanker(ok, L5, M10)
    a, b = (torch.from_numpy(x[:8].view(np.int32)).to(DEV) for x in (boards["A"], boards["B"]))
    label = torch.from_numpy(boards["nodes"]["label"][:8]).to(DEV)
    ranker.rank((a, b), label)                                 # the good call
    for planes in ((a, b[:7]), (a.cpu(), b.cpu()), (a.to(torch.int64), b.to(torch.int64)), (a,), a, (a.reshape(-1), b.reshape(-1)),
                   (a.t().contiguous().t(), b)):
        with pytest.raises(ValueError, match="planes"):
            ranker.rank(planes, label)
    for lab in (label[:7], label.cpu(), label.to(torch.int32), label[:, :39], label.reshape(-1), None,
                torch.zeros((8, 80), dtype=torch.uint8, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="label must be"):
            ranker.rank((a, b), lab)
    good = ranker.buffers(8)
    for name, t in (("gap", good["gap"].to(torch.float64)), ("win", good["win"][:7]), ("win_a", good["win_a"].cpu()),
                    ("loss_b", good["loss_b"].reshape(-1)), ("violated", good["violated"].to(torch.int32))):
        with pytest.raises(ValueError, match="out"):
            ranker.step((a, b), label, {**good, name: t})
    with pytest.raises(ValueError, match="out must be a dict"):
        ranker.rank((a, b), label, {k: v for k, v in good.items() if k != "gap"})
    assert not ok.any()                                        # nothing was taught by a refused call: rank() alone ran
    s = T.LabelSet(DEV).append(a, b, label)
    for bad in (dict(epochs=0), dict(batch=0), dict(seed=-1), dict(epochs=1.5)):
        with pytest.raises(ValueError):
            ranker.fit(s, **{**dict(epochs=1, batch=4), **bad})
    with pytest.raises(ValueError):
        ranker.fit(T.LabelSet(DEV), 1, 4)                      # an empty set
    with pytest.raises(ValueError, match="four plain forms"):
        T.label_agreement(T.ntuple_table(DEV, "2x4+3x3"), (a, b), label, L5, M10)
    env = T.BatchedTetris(L5, M10, 8, device=DEV)
    with pytest.raises(ValueError, match="configuration pool"):
        T.collect_labels(env, np.zeros((1, M10 + 1), np.uint8), T.NTuplePolicy(env, ok), 1)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            T.collect_labels(env, np.zeros((1, M10 + 1), np.uint8), T.NTuplePolicy(env, ok), bad)
    with pytest.raises(ValueError, match="policy"):
        T.collect_labels(env, np.zeros((1, M10 + 1), np.uint8), None, 1)
    env.terminate()
    assert m.RANK_OUTPUTS[:7] == T.ntuple.RANK_OUTPUTS[:7]
