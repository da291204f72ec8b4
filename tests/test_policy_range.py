"""The policy kernels (csrc/policy_mlp.hip, policy_f32.hip, policy_split.hip) and their actor megakernels over the whole
game range, against references that do not go through the device.

test_policy_kernel.py pins the wiring at one game size (L=10, M=40, a few synthetic steps).  Here:
  * ACTOR LOOP: a plain CPU actor iteration -- oracle.Env.expand_obs() -> float64 MLP in numpy -> argmax (lowest index on
    ties) -> oracle.explore_actions -> oracle.Env.step -- against tpl_actor_rollout of all three image kinds, across L and M
    on both sides of every record-stride change and window word (advance_board's refill through pool_record), and against
    Actor(fused=True) stepped one iteration at a time.  The weights (a column leveller) are small integers, so every kernel
    must give the float64 logits exactly and the decisions bit for bit.
  * FEATURE EDGES: policy_act of all three kernels on states at the ends of the counters (M_rem 254 / 129 / 128 / 0, L_rem
    250 / 1 / below zero), every terminal state, every cur / nxt piece and nearly full boards; exact weights on features
    214-216 over several output rows.
  * SPLIT TERMS: constructions whose products and partial sums are all exact in float32, in which every one of the split
    kernel's piece products (three planes of layer 1, six terms of each hidden layer and of the head) carries a non-zero
    part of some logit -- the CPU tests show each is needed -- and biases with a full 24-bit significand for the float32 and
    split kernels.
"""
import numpy as np
import pytest

TERMS = {"all_xh": (2, 0), "ah_xll": (0, 2), "al_xl": (1, 1), "al_xh": (1, 0), "ah_xl": (0, 1), "ah_xh": (0, 0)}
KINDS = [False, True, "split"]           # pack_policy(..., f32=kind): bf16, float32, three bf16 pieces


# ------------------------------------------------------------------------------------------------- plain references
def _bf16_bits(a):
    """float32 -> bf16 bit pattern, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint32) << 16).astype(np.uint32).view(np.float32)


def _split3(a):
    """x = x_h + x_l + x_ll, each the RNE bf16 of what the earlier pieces leave (float32 arithmetic): bit patterns."""
    r = np.ascontiguousarray(a, dtype=np.float32)
    out = []
    for _ in range(3):
        bits = _bf16_bits(r)
        out.append(bits)
        r = (r - _bf16_value(bits)).astype(np.float32)
    return out


def _mlp64(obs, params, hidden=None):
    """Model(217, 14) in float64; `hidden`, a list, receives every hidden layer's activations."""
    x = np.asarray(obs, dtype=np.float64)
    for i, (w, b) in enumerate(params):
        x = x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if i < 4:
            x = np.maximum(x, 0.0)
            if hidden is not None:
                hidden.append(x)
    return x


def _split_emulation(obs, params, drop=None):
    """The split kernel's arithmetic in float64: weights and float32 activations as three bf16 pieces; layer 1 multiplies its
    three weight planes with the exact inputs, the other layers sum the six products of TERMS.  drop=(layer, piece pair)
    leaves one product out (layer 0: pair (plane, 0))."""
    x = np.asarray(obs, dtype=np.float64)
    for i, (w, b) in enumerate(params):
        wp = [_bf16_value(p).astype(np.float64) for p in _split3(w)]
        if i == 0:
            xp, pairs = [x], [(p, 0) for p in range(3)]
        else:
            xp = [_bf16_value(p).astype(np.float64) for p in _split3(x.astype(np.float32))]
            pairs = list(TERMS.values())
        y = np.broadcast_to(np.asarray(b, np.float64), (x.shape[0], w.shape[0])).copy()
        for pw, px in pairs:
            if drop != (i, (pw, px)):
                y += xp[px] @ wp[pw].T
        x = np.maximum(y, 0.0) if i < 4 else y
    return x


def _decode(logits):
    return (logits[:, :4].argmax(1) * 10 + logits[:, 4:].argmax(1)).astype(np.uint8)


def _assert_bf16_exact(values):
    v = np.asarray(values, np.float64)
    assert np.array_equal(_bf16_value(_bf16_bits(v.astype(np.float32))).astype(np.float64), v)


def _dense_boards(rng, n):
    """Tall, dense boards with nearly-full rows so that clears, multi-clears and top-outs all occur."""
    height = rng.integers(0, 21, n)
    cells = rng.random((n, 20, 10)) < rng.uniform(0.3, 0.95, (n, 1, 1))
    near = rng.random((n, 20)) < 0.5
    holes = rng.integers(0, 10, (n, 20))
    full = np.ones((n, 20, 10), bool)
    full[np.arange(n)[:, None], np.arange(20)[None, :], holes] = False
    cells = np.where(near[:, :, None], full, cells)
    cells &= (np.arange(20)[None, :, None] >= (20 - height)[:, None, None])
    return (cells.astype(np.uint16) << np.arange(10, dtype=np.uint16)).sum(-1).astype(np.uint16)


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    import tetris_piclim
    return tetris_piclim


def _image(T, params, kind, device):
    import torch
    return torch.from_numpy(T.pack_policy(params, f32=kind)).to(device)


def _model(T, params):
    import torch
    model = T.PolicyMLP()
    with torch.no_grad():
        for layer, (w, b) in zip((model.layer1, model.layer2, model.layer3, model.layer4, model.layer5), params):
            layer.weight.copy_(torch.from_numpy(w))
            layer.bias.copy_(torch.from_numpy(b))
    return model


# ------------------------------------------------------------------------------------------------- 1. the actor loop
def _leveller(L, M):
    """A column leveller, exact in small integers: h_x = the number of filled cells of column x; location logit -h_x.  The
    rotation logits read the counters and the terminal flag: 1.5 | relu(M_rem - (M - 4)) | 2 relu(L_rem - (L - 1)) +
    3 relu(-L_rem) | 2 x feature 216 -- rotation 1 on the first moves of an episode, 2 until its first line, 2 again on a
    frozen win whose last clear overshot L, 3 on any other frozen board, 0 otherwise."""
    w1, b1 = np.zeros((128, 217), np.float32), np.zeros(128, np.float32)
    for x in range(10):
        w1[x, x:200:10] = 1                                      # obs index 10 y + x
    w1[10, 215], b1[10] = 1, -(M - 4)
    w1[11, 214], b1[11] = 1, -(L - 1)
    w1[12, 216] = 1
    w1[13, 214] = -1
    eye, zero = np.eye(128, dtype=np.float32), np.zeros(128, np.float32)
    w5, b5 = np.zeros((14, 128), np.float32), np.zeros(14, np.float32)
    for x in range(10):
        w5[4 + x, x] = -1
    b5[0] = 1.5
    w5[1, 10] = 1
    w5[2, 11], w5[2, 13] = 2, 3
    w5[3, 12] = 2
    return [(w1, b1), (eye, zero), (eye, zero), (eye, zero), (w5, b5)]


def _actor_pool(L, M, count=300):
    """Mostly low boards (0..3 bottom rows, one hole per row) and random pieces."""
    rng = np.random.default_rng(L * 1000 + M)
    rows = np.zeros((count, 20), np.uint16)
    height = rng.integers(0, 4, count)
    for i in range(count):
        for r in range(20 - height[i], 20):
            rows[i, r] = int(rng.integers(0, 1 << 10)) & ~(1 << int(rng.integers(0, 10)))
    return rows, rng.integers(0, 7, (count, M + 1)).astype(np.uint8)


_REWARD = (1.0, 2.0, -1.0)
_OFFSET, _SEED, _XSEED, _STEP0 = 1000, 11, 5, 100


def _cpu_actor_loop(oracle, L, M, n, auto, eps, steps, params, pool):
    """The reference: oracle.Env.expand_obs -> float64 MLP -> argmax -> oracle.explore_actions -> oracle.Env.step."""
    cpu = oracle.Env(n, L, M, _OFFSET, _SEED)
    cpu.set_pool(*pool)
    cpu.set_options(auto_reset=auto, assign_mode=0, per_line=_REWARD[0], win=_REWARD[1], lose=_REWARD[2])
    cpu.reset()
    rec = {k: [] for k in ("obs", "moves", "state", "actions", "rewards", "dones")}
    for t in range(steps):
        obs = cpu.expand_obs()
        st = cpu.get_state()
        logits = _mlp64(obs, params)
        action = oracle.explore_actions(_decode(logits), eps, _XSEED, _STEP0 + t, _OFFSET)
        r, d = cpu.step(action)
        for k, v in (("obs", obs), ("moves", st["moves"]), ("state", st["state"]), ("actions", action), ("rewards", r),
                     ("dones", d)):
            rec[k].append(v)
    return {k: np.stack(v) for k, v in rec.items()}, cpu


def _gpu_env(T, L, M, n, auto, pool):
    env = T.BatchedTetris(L, M, n, seed=_SEED, auto_reset=auto, global_offset=_OFFSET, reward=_REWARD)
    env.load_configs(*pool)
    env.reset()
    return env


_N_ACTOR = 1509                          # not a multiple of 32 or 64: a ragged last tile


@pytest.mark.gpu
@pytest.mark.parametrize("L,M,auto,eps,steps", [
    (1, 9, True, 0.1, 24), (1, 11, False, 0.0, 24),            # M + 1 pieces: one window word / two
    (250, 40, True, 0.0, 32), (1, 49, False, 0.1, 32),         # the smallest record stride
    (250, 50, True, 0.1, 32), (250, 129, False, 0.0, 32),      # the second
    (1, 130, True, 0.0, 32), (250, 254, False, 0.05, 36),      # the third
    (250, 254, True, 0.0, 36)])
def test_actor_megakernels_equal_the_cpu_actor_loop(T, oracle, L, M, auto, eps, steps):
    """tpl_actor_rollout / _f32 / _split (two launches, the second resuming from the stored state; global_offset != 0; n not a
    multiple of the tile) against the CPU actor loop: actions, rewards, dones, every recorded state (expanded, against the
    oracle's observation at that step), the final packed state and the statistics, bit for bit.  The boards cross the window
    refills at moves 10 and 20 inside the launches (advance_board's pool_record(p, slot, cfg) with the record stride of M)."""
    import torch
    n = _N_ACTOR
    params, pool = _leveller(L, M), _actor_pool(L, M)
    rec, cpu = _cpu_actor_loop(oracle, L, M, n, auto, eps, steps, params, pool)
    hidden = []
    _mlp64(rec["obs"].reshape(-1, 217), params, hidden)
    for h in hidden:                                             # every kernel must give the float64 logits exactly
        _assert_bf16_exact(h)
    running = rec["state"] == 0
    crossed10 = (running & (rec["moves"] >= 10)).any(0).mean()
    crossed20 = (running & (rec["moves"] >= 20)).any(0).mean()
    if M >= 11:
        assert crossed10 > 0.85, crossed10                      # the refill at move 10 ran for most boards
    if M >= 40:
        assert crossed20 > 0.75, crossed20                      # and the one at move 20
    assert len(np.unique(rec["actions"] // 10)) >= 2             # the counter / terminal terms steer the rotation
    if eps > 0:
        assert (rec["actions"] != np.stack([_decode(_mlp64(o, params)) for o in rec["obs"]])).any()
    want_state, want_stats = cpu.get_state(), cpu.stats()
    k1 = steps // 3
    for kind in KINDS:
        env = _gpu_env(T, L, M, n, auto, pool)
        image = _image(T, params, kind, env.device)
        out1 = env.actor_rollout(image, k1, epsilon=eps, seed=_XSEED, step0=_STEP0, record_states=True)
        out2 = env.actor_rollout(image, steps - k1, epsilon=eps, seed=_XSEED, step0=_STEP0 + k1, record_states=True)
        out = {k: torch.cat([out1[k], out2[k]]) for k in out1}
        assert np.array_equal(_np(out["actions"]), rec["actions"]), kind
        assert np.array_equal(_np(out["rewards"]), rec["rewards"]), kind
        assert np.array_equal(_np(out["dones"]).astype(np.uint8), rec["dones"]), kind
        for t in range(steps):
            obs = _np(env.expand_states(out["states_a"][t], out["states_b"][t]))
            assert np.array_equal(obs, rec["obs"][t]), (kind, t)
        got = {k: _np(v) for k, v in env.packed_state().items()}
        for k, v in want_state.items():
            assert np.array_equal(got[k].view(np.uint16) if k == "rows" else got[k], v), (kind, k)
        assert env.stats() == want_stats, kind
        env.terminate()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_fused_actor_steps_equal_the_cpu_actor_loop_at_m254(T, oracle, kind):
    """Actor(fused=True) -- policy_act + step_into, one iteration at a time -- against the same CPU actor loop at L=250, M=254
    (the largest record stride, M_rem up to 254): the single-step path and the megakernels answer to one reference."""
    import torch
    L, M, n, steps = 250, 254, _N_ACTOR, 32
    params, pool = _leveller(L, M), _actor_pool(L, M)
    rec, cpu = _cpu_actor_loop(oracle, L, M, n, True, 0.0, steps, params, pool)
    env = _gpu_env(T, L, M, n, True, pool)
    dtype = torch.bfloat16 if kind is False else torch.float32
    actor = T.Actor(env, _model(T, params), dtype=dtype, use_graph=False, fused=True, split=kind == "split")
    for t in range(steps):
        actor.step()
        assert np.array_equal(_np(actor.action), rec["actions"][t]), t
        assert np.array_equal(_np(actor.reward), rec["rewards"][t]) and np.array_equal(_np(actor.done), rec["dones"][t]), t
    got = {k: _np(v) for k, v in env.packed_state().items()}
    for k, v in cpu.get_state().items():
        assert np.array_equal(got[k].view(np.uint16) if k == "rows" else got[k], v), k
    assert env.stats() == cpu.stats()
    env.terminate()


# ------------------------------------------------------------------------------------------------- 2. feature edges
def _edge_params(seed=7):
    """Exact weights with the counters and the terminal flag in play: 64 small units of three +-1 cell / piece features, 20
    counter units relu(+-feature + b) at thresholds where the extremes differ (M_rem 128 | 129, 253 | 254, 0; L_rem 249 | 250,
    1, below zero), carried by identity through the hidden layers while the small units mix; every head row reads two
    counter units and two small ones.  Every hidden value is an integer of magnitude <= 256 (exact in bf16)."""
    rng = np.random.default_rng(seed)
    w1, b1 = np.zeros((128, 217), np.float32), np.zeros(128, np.float32)
    for r in range(64):
        w1[r, rng.choice(214, 3, replace=False)] = rng.choice([-1, 1], 3)
        b1[r] = rng.integers(0, 2)
    counters = [(214, 1, 0), (214, 1, -249), (214, -1, 0), (214, -1, 2), (214, 1, -1), (214, -1, 250),
                (215, 1, 0), (215, 1, -128), (215, -1, 129), (215, 1, -253), (215, -1, 1), (215, 1, -127), (215, -1, 254),
                (216, 1, 0), (216, -1, 1), (216, 1, 2), (214, 1, 3), (215, 1, 1), (216, 3, 0), (214, -1, -1)]
    nc = len(counters)
    for j, (k, s, b) in enumerate(counters):
        w1[64 + j, k], b1[64 + j] = s, b
    params = [(w1, b1)]
    for _ in range(3):
        w, b = np.zeros((128, 128), np.float32), np.zeros(128, np.float32)
        for r in range(64):
            w[r, rng.choice(64, 2, replace=False)] = rng.choice([-1, 1], 2)
            b[r] = rng.integers(-1, 2)
        for r in range(64, 64 + nc):
            w[r, r] = 1
        params.append((w, b))
    w5, b5 = np.zeros((14, 128), np.float32), rng.integers(-3, 4, 14).astype(np.float32)
    for r in range(14):
        w5[r, 64 + r % nc] = rng.choice([-1, 1])
        w5[r, 64 + (r + 14) % nc] = rng.choice([-1, 1])
        w5[r, rng.choice(64, 2, replace=False)] = rng.choice([-1, 1], 2)
    params.append((w5, b5))
    return params


# (L, M, what the moves reach): every case starts from a fresh reset and records the features after 0..len(moves) moves
_EDGE_CASES = [
    (250, 254, "M_rem 254..251, L_rem 250, top-outs"),
    (1, 129, "M_rem 129, L_rem 1, wins that overshoot"),
    (1, 128, "M_rem 128, wins"),
    (250, 1, "M_rem 0: out of moves, no next piece"),
]


def _edge_pool(L, M, n, seed):
    """Dense boards; piece pairs (cur, nxt) cycling through all 49; every seventh board of an L=1 game set up for an
    upright I at x=0 to clear three rows at once (lines left 1 - 3 = -2)."""
    rng = np.random.default_rng(seed)
    rows = _dense_boards(rng, n)
    rows[rows == 0x3FF] = 0x3FE
    pieces = rng.integers(0, 7, (n, M + 1)).astype(np.uint8)
    idx = np.arange(n)
    pieces[:, 0] = idx % 7
    if M >= 1:
        pieces[:, 1] = (idx // 7) % 7
    over = (idx % 7 == 3) if L == 1 else np.zeros(n, bool)
    rows[over] = 0
    rows[over, 17:] = 0x3FE
    pieces[over, 0] = 0
    return rows, pieces, over


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 33, 1000])
@pytest.mark.parametrize("L,M,what", _EDGE_CASES)
def test_policy_logits_at_the_edges_of_the_state(T, oracle, L, M, what, n):
    """policy_act of the bf16, float32 and split kernels on boards at the ends of the counters, in every terminal state, with
    every cur / nxt piece, on nearly full boards: the logits equal the float64 MLP of oracle.Env.expand_obs() bit for bit."""
    import torch
    params = _edge_params()
    rows, pieces, over = _edge_pool(L, M, n, seed=M + n)
    gpu = T.BatchedTetris(L, M, n, assign="sequential", config_pool=(rows, pieces))
    cpu = oracle.Env(n, L, M)
    cpu.set_pool(rows, pieces)
    cpu.set_options(assign_mode=1)
    gpu.reset(); cpu.reset()
    images = {kind: _image(T, params, kind, gpu.device) for kind in KINDS}
    rng = np.random.default_rng(n)
    seen = []
    for t in range(min(M, 4) + 1):
        obs = cpu.expand_obs()
        hidden = []
        want = _mlp64(obs, params, hidden)
        for h in hidden:
            _assert_bf16_exact(h)
        for kind, image in images.items():
            logits = torch.full((n, 14), float("nan"), device=gpu.device)
            action = gpu.policy_act(image, logits=logits)
            assert np.array_equal(_np(logits), want.astype(np.float32)), (kind, t)
            assert np.array_equal(_np(action), _decode(want)), (kind, t)
        seen.append(obs)
        rot = rng.integers(0, 4, n).astype(np.uint8)
        loc = rng.integers(0, 10, n).astype(np.uint8)
        if t == 0:
            rot[over], loc[over] = 1, 0
        gpu.move(rot, loc); cpu.move(rot, loc)
    seen = np.concatenate(seen)
    if n == 1000:                                                # the edges this case is there for were reached
        st = cpu.stats()
        assert len({(c, x) for c, x in zip(seen[:, 200:207].argmax(1), seen[:, 207:214].argmax(1))}) == 49
        assert (seen[:, 216] == 1).any() and (seen[:, 216] == 0).any()
        assert seen[:, :200].sum(1).max() >= 170                 # nearly full boards
        if M == 254:
            assert set(seen[:, 215]) == {254, 253, 252, 251, 250} and seen[:, 214].max() == 250
            assert st["topouts"] > 0
        if M in (128, 129):
            assert seen[:, 215].max() == M and seen[:, 214].max() == 1
            assert (seen[:, 214] < 0).any() and st["wins"] > 0      # won, some by overshooting
        if M == 1:
            assert (seen[:, 215] == 0).any() and (seen[:, 207:214].sum(1) == 0).any()
            assert st["topouts"] > 0 and st["episodes"] - st["wins"] - st["topouts"] > 0     # and out of moves
    gpu.terminate()


# ------------------------------------------------------------------------------------------------- 3. split pieces
A_VAL = 1.0 + 2.0 ** -9 + 2.0 ** -18      # RNE pieces (1, 2^-9, 2^-18)
B_VAL = 1.0 + 2.0 ** -8                   # RNE pieces (1, 2^-8, 0): B * B = 1 + 2^-7 + 2^-16 is exact


def _term_params():
    """Every piece product of the split kernel carries part of some logit, and every product and partial sum is exact in
    float32.  P = a count of filled cells (0..4); A * P exercises a weight's mid and low pieces (al xh, all xh; layer 1: the
    three planes), 1 * (A P) an activation's (ah xl, ah xll), B * (B P) the product of two mid pieces (al xl).  Each layer
    makes A P, B P and P again for the next and hands its three results on by identity; the head gives each result a row."""
    w1, b1 = np.zeros((128, 217), np.float32), np.zeros(128, np.float32)
    P, XA, XB = 0, 1, 2
    w1[P, [198, 187, 176, 165]] = 1                              # P: four cells of the lower rows
    w1[XA, [199, 188, 177, 163]] = A_VAL                         # layer 1, all three planes: A x cells
    w1[XB, [197, 186, 175, 164]] = B_VAL
    w1[3, 215] = B_VAL                                           # B x M_rem: the counter operand, planes 0 and 1
    carried = [XA, 3]
    params = [(w1, b1)]
    nxt = 4
    for _ in range(3):
        w, b = np.zeros((128, 128), np.float32), np.zeros(128, np.float32)
        for u in carried:
            w[u, u] = 1
        p2, a2, b2, xa2, y2 = range(nxt, nxt + 5)
        w[p2, P] = 1
        w[a2, P] = A_VAL                                         # al xh, all xh
        w[b2, P] = B_VAL
        w[xa2, XA] = 1                                           # ah xl, ah xll
        w[y2, XB] = B_VAL                                        # al xl
        carried += [a2, xa2, y2]
        P, XA, XB, nxt = p2, a2, b2, nxt + 5
        params.append((w, b))
    w5, b5 = np.zeros((14, 128), np.float32), np.zeros(14, np.float32)
    w5[0, P] = A_VAL
    w5[1, XA] = 1
    w5[2, XB] = B_VAL
    assert len(carried) == 11
    for r, u in enumerate(carried):
        w5[3 + r, u] = 1
    params.append((w5, b5))
    return params


def _term_boards(oracle, n=256, L=10, M=40, seed=41):
    rng = np.random.default_rng(seed)
    rows = _dense_boards(rng, n)
    pieces = rng.integers(0, 7, (n, M + 1)).astype(np.uint8)
    cpu = oracle.Env(n, L, M)
    cpu.set_pool(rows, pieces)
    cpu.set_options(assign_mode=1)
    cpu.reset()
    return rows, pieces, cpu


def _full_significand(rng, size):
    """Values in [1, 2) whose last significand bit is set: 24 significant bits, far from any bf16 number."""
    return ((2 ** 23 + 2 * rng.integers(0, 2 ** 22, size) + 1) * 2.0 ** -23).astype(np.float32)


def _bias_params(layer, group, rng):
    """Biases of one layer, all 128 (or the head's 14) with a full 24-bit significand, made visible one per logit and board:
    earlier layers carry the current-piece one-hot in units 0..6; unit j of `layer` is its bias where the current piece is
    j % 7 and is switched off (-4 per other piece) elsewhere; later layers pass it on; head row r sums the units j with
    j // 7 = 14 group + r, of which exactly one is on.  Returns the parameters and the float32 biases under test."""
    eye, zero = np.eye(128, dtype=np.float32), np.zeros(128, np.float32)
    params = []
    for i in range(5):
        rows_in = 217 if i == 0 else 128
        w = np.zeros((14 if i == 4 else 128, rows_in), np.float32)
        b = np.zeros(w.shape[0], np.float32)
        if layer == 4:
            if i == 4:
                b = _full_significand(rng, 14)
        elif i < layer:
            for q in range(7):
                w[q, 200 + q if i == 0 else q] = 1
        elif i == layer:
            b = _full_significand(rng, 128)
            for j in range(128):
                for q in range(7):
                    if q != j % 7:
                        w[j, 200 + q if i == 0 else q] = -4
        elif i < 4:
            w, b = eye.copy(), zero.copy()
        else:
            for j in range(128):
                if 0 <= j // 7 - 14 * group < 14:
                    w[j // 7 - 14 * group, j] = 1
        params.append((w, b))
    return params, params[layer][1]


_BIAS_CASES = [(layer, group) for layer in range(4) for group in (0, 1)] + [(4, 0)]


def test_split_packer_pieces_equal_numpy_split3():
    """tpl_policy_pack_split against a numpy RNE split3: with every weight of a layer one constant, the fragment layout does
    not matter -- each u16 of a plane is that constant's piece (layer 1: half of it for the 0/1 features, which enter as 2.0,
    the constant itself for the counters 214, 215, zero for the seven padding k; head: zero for the padding rows 14, 15).
    The pieces add up to the constant exactly, and the biases are stored as float32."""
    import tetris_piclim as T
    plane1, plane5, off_b = 57344, 4096, 479232                    # policy_split.hip's chunk table
    chunk = [0, 57344, 114688, 172032, 221184, 270336, 319488, 368640, 417792, 466944]
    values = [A_VAL, B_VAL, -A_VAL, 0.1, -3.14159274, 1.0 / 3.0, 2.0 ** -20 * 1.2345678, 255.0 + 2.0 ** -15, 1.0]
    rng = np.random.default_rng(5)
    for v in values:
        v = np.float32(v)
        pieces = _split3(np.array([v, v / 2], np.float32))
        assert np.float64(v) == sum(_bf16_value(p[0]).astype(np.float64) for p in pieces)    # exact to the last place
        biases = [rng.standard_normal(128).astype(np.float32) for _ in range(4)] + [rng.standard_normal(14).astype(np.float32)]
        params = [(np.full((128, 217), v, np.float32), biases[0])] + \
                 [(np.full((128, 128), v, np.float32), biases[i]) for i in (1, 2, 3)] + \
                 [(np.full((14, 128), v, np.float32), biases[4])]
        image = T.pack_policy(params, f32="split")
        u16 = image[:off_b].view(np.uint16)
        for i in range(3):
            full, half = pieces[i][0], pieces[i][1]
            got = u16[(chunk[i]) // 2:(chunk[i] + plane1) // 2]              # layer 1, plane i: 128 rows x 224 k
            vals, counts = np.unique(got, return_counts=True)
            want = {}
            for val, cnt in ((half, 128 * 215), (full, 128 * 2), (0, 128 * 7)):
                want[int(val)] = want.get(int(val), 0) + cnt
            assert dict(zip(vals.tolist(), counts.tolist())) == {k: c for k, c in want.items() if c}, (v, i)
            for layer in range(3):                                 # hidden layers: chunks of two k-steps x three planes
                for half_no in range(2):
                    base = chunk[3 + 2 * layer + half_no]
                    for sl in range(2):
                        blk = u16[(base + (sl * 3 + i) * 8 * 1024) // 2:(base + ((sl * 3 + i) * 8 + 8) * 1024) // 2]
                        assert np.all(blk == full), (v, i, layer)
            head = u16[(chunk[9] + i * plane5) // 2:(chunk[9] + (i + 1) * plane5) // 2].reshape(4, 64, 8)
            row = np.arange(64) & 15
            assert np.all(head[:, row < 14] == full) and np.all(head[:, row >= 14] == 0), (v, i)
        stored = image[off_b:].view(np.float32)
        assert np.array_equal(stored[:526], np.concatenate(biases)) and np.all(stored[526:] == 0)


def test_split_constructions_are_sharp(oracle):
    """The constructions of the GPU tests below, in float64 on the CPU: the split kernel's arithmetic gives the float64 MLP
    exactly, and leaving out any one piece product -- a plane of layer 1, one of the six terms of a hidden layer or of the
    head -- changes some logit; the bias networks pass every bias through unchanged."""
    _, _, cpu = _term_boards(oracle)
    obs = cpu.expand_obs()
    params = _term_params()
    want = _mlp64(obs, params)
    assert np.array_equal(_split_emulation(obs, params), want)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)     # exact in float32
    for plane in range(3):
        assert not np.array_equal(_split_emulation(obs, params, drop=(0, (plane, 0))), want), plane
    for layer in range(1, 5):
        for name, pair in TERMS.items():
            assert not np.array_equal(_split_emulation(obs, params, drop=(layer, pair)), want), (layer, name)
    rng = np.random.default_rng(9)
    cur = obs[:, 200:207].argmax(1)
    assert set(cur) == set(range(7))
    for layer, group in _BIAS_CASES:
        params, bias = _bias_params(layer, group, rng)
        want = _mlp64(obs, params)
        assert np.array_equal(_split_emulation(obs, params), want)
        if layer == 4:
            assert np.array_equal(want, np.broadcast_to(bias.astype(np.float64), want.shape))
            continue
        for r in range(14):
            j = 7 * (14 * group + r) + cur
            expect = np.where(j < 128, bias[np.minimum(j, 127)].astype(np.float64), 0.0)
            assert np.array_equal(want[:, r], expect), (layer, group, r)
        assert not np.array_equal(_bf16_value(_bf16_bits(bias)), bias)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [True, "split"])
def test_every_piece_product_reaches_the_logits_exactly(T, oracle, kind):
    """The float32 and split kernels on _term_params (every piece product of the split kernel carries part of a logit; every
    product and partial sum exact in float32): logits equal the float64 MLP of the oracle's observation bit for bit."""
    import torch
    rows, pieces, cpu = _term_boards(oracle)
    n = rows.shape[0]
    gpu = T.BatchedTetris(10, 40, n, assign="sequential", config_pool=(rows, pieces))
    gpu.reset()
    params = _term_params()
    want = _mlp64(cpu.expand_obs(), params)
    logits = torch.full((n, 14), float("nan"), device=gpu.device)
    action = gpu.policy_act(_image(T, params, kind, gpu.device), logits=logits)
    assert np.array_equal(_np(logits), want.astype(np.float32))
    assert np.array_equal(_np(action), _decode(want))
    gpu.terminate()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [True, "split"])
def test_biases_keep_their_full_float32_significand(T, oracle, kind):
    """The float32 and split kernels on _bias_params: every bias of every layer, 24 significant bits, reaches a logit
    unchanged -- a bias loaded or added at bf16 width would not."""
    import torch
    rows, pieces, cpu = _term_boards(oracle)
    n = rows.shape[0]
    obs = cpu.expand_obs()
    gpu = T.BatchedTetris(10, 40, n, assign="sequential", config_pool=(rows, pieces))
    gpu.reset()
    rng = np.random.default_rng(9)
    for layer, group in _BIAS_CASES:
        params, _ = _bias_params(layer, group, rng)
        want = _mlp64(obs, params)
        logits = torch.full((n, 14), float("nan"), device=gpu.device)
        gpu.policy_act(_image(T, params, kind, gpu.device), logits=logits)
        assert np.array_equal(_np(logits), want.astype(np.float32)), (layer, group)
    gpu.terminate()
