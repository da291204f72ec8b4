"""Board features of every placement, a linear placement policy on them, and its tuning by the noisy cross-entropy method
(the rule: include/tpl_learn.h; the kernels: csrc/learn/heuristic.hip).

    placement_features(env)       phi(s, a) of all 40 actions of every board: int16 [K, 40, 12] (FEATURE_NAMES) and canonical
    HeuristicPolicy(env, weights).act()
                                  arg-max over the distinct placements of  w . phi(s, a)  in ONE launch: 32 bytes read and one
                                  written per board; `weights` [P, 12] plays a population, `boards_per_member` boards each
    HeuristicPolicy(env, weights, depth=2).act()
                                  two plies with the known next piece (window entry 1), still one launch: a first placement is
                                  worth the best placement of the next piece on the board it leaves
    BeamPolicy(env, weights, depth, width).act()
                                  a beam search over the pieces the state's window is known to hold (up to twelve), still one
                                  launch: each ply keeps the `width` best nodes; act(plan=...) also gives the chosen path
    evaluate_heuristic(env, weights, boards_per_member, steps)
                                  episodes and wins of every member of a population on an auto-reset environment
    tune_heuristic(L, M, config_pool, ...)
                                  the weights by the noisy cross-entropy method (Szita & Lorincz 2006), fitness = win rate

    move_bound(env)               the move bound of every board (include/tpl_learn.h): the cells its owed rows still miss, the spare
                                  cells its remaining moves leave, and whether it is dead -- provably lost whatever pieces come
    BeamPolicy(..., bound=True, spare_weight=x)
                                  the bounded form: a move that leaves a dead board leaves it lost, and x times a node's spare
                                  cells is added to its value; depth 1, width 1 is the bounded one-ply player

With weights (r_line, r_win, r_lose, 0, ..., 0) the policy is LookaheadPolicy(env, image=None): the best immediate reward.

The 14-feature form.  Weights of 14 entries ([14] or [P, 14], MOVE_FEATURE_NAMES) select it everywhere above: the twelve features
of the board a move leaves and the two of the move itself, landing_height and eroded_cells, which deeper than one ply add up along
the path as `cleared` does.  placement_features(env, move=True) gives int16 [K, 40, 14].  DELLACHERIE_WEIGHTS is Dellacherie's
published controller in this feature order, a named starting point with no win-rate claim attached.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _learn_lib
from ._learn_lib import (BEAM_MAX_DEPTH, BEAM_MAX_WIDTH, FEATURE_COUNTS, FEATURE_NAMES, MOVE_FEATURE_NAMES, MOVE_WEIGHT_STRIDE,
                         NUM_ACTIONS, NUM_FEATURES, NUM_MOVE_FEATURES, check)
from .lookahead import _boards, _ptr, _source_planes, _state_ptrs

__all__ = ["FEATURE_NAMES", "MOVE_FEATURE_NAMES", "DELLACHERIE_WEIGHTS", "placement_features", "HeuristicPolicy", "BeamPolicy",
           "evaluate_heuristic", "tune_heuristic", "move_bound"]

# Dellacherie's controller in MOVE_FEATURE_NAMES' order and units: holes -4, row and column transitions -1, wells -1, landing height
# -1 a row = -0.5 a half row, eroded cells +1; won and lost +-100 stand in for the end of the game, which his endless game has not
DELLACHERIE_WEIGHTS = np.array([0, 100, -100, -4, 0, 0, 0, -1, -1, -1, 0, 0, -0.5, 1], np.float32)
DELLACHERIE_WEIGHTS.setflags(write=False)


def placement_features(env, states_a: Optional[torch.Tensor] = None, states_b: Optional[torch.Tensor] = None, move: bool = False):
    """phi(s, a) for K states and all 40 actions: the resident boards of `env` (K = env.num_envs, read in place), or int32
    [K, 4] plane pairs as env.expand_states takes them, under env.L and env.M.  Returns (features int16 [K, 40, 12], canonical
    uint8 [K, 40]); entry [i, a] belongs to action a = 10 r + l played from state i, a == canonical[i, a] marks the distinct
    placements, and a finished board's features are all zero.  move=True: the 14-feature form, int16 [K, 40, 14] (a view of the
    kernel's 16-wide records), landing_height and eroded_cells behind the twelve."""
    if not isinstance(move, (bool, np.bool_)):
        raise ValueError("move must be True or False")
    k, src_a, src_b = _source_planes(env, states_a, states_b, "placement_features")
    d = env.device
    count = NUM_MOVE_FEATURES if move else NUM_FEATURES
    features = torch.empty((k, NUM_ACTIONS, MOVE_WEIGHT_STRIDE if move else NUM_FEATURES), dtype=torch.int16, device=d)
    canonical = torch.empty((k, NUM_ACTIONS), dtype=torch.uint8, device=d)
    stream = torch._C._cuda_getCurrentRawStream(d.index)
    check(_learn_lib.entry("features", count)(_ptr(src_a), _ptr(src_b), k, env.L, env.M, features.data_ptr(), canonical.data_ptr(),
                                              stream))
    return features[:, :, :count], canonical


def move_bound(env, states_a: Optional[torch.Tensor] = None, states_b: Optional[torch.Tensor] = None) -> dict:
    """The move bound of K states (include/tpl_learn.h; tpl_move_bound): the resident boards of `env` (read in place), or int32
    [K, 4] plane pairs as env.expand_states takes them, under env.L and env.M.  Returns device tensors [K]: cells int32, the cells
    missing from the cheapest rows still owed; spare int32 = 4 (moves left) - cells; need int32 = ceil(cells / 4), the least number
    of moves in which the board can still be won; dead bool = spare < 0: no continuation wins, whatever pieces come.  A finished
    board gives 0, 0, 0, False."""
    k, src_a, src_b = _source_planes(env, states_a, states_b, "move_bound")
    d = env.device
    cells = torch.empty(k, dtype=torch.int32, device=d)
    spare = torch.empty(k, dtype=torch.int32, device=d)
    stream = torch._C._cuda_getCurrentRawStream(d.index)
    check(_learn_lib.lib().tpl_move_bound(_ptr(src_a), _ptr(src_b), k, env.L, env.M, cells.data_ptr(), spare.data_ptr(), stream))
    return dict(cells=cells, spare=spare, need=(cells + 3) // 4, dead=spare < 0)


def _bounded(bound, spare_weight):
    """The validated (bound, spare_weight) of a beam player: a bool, and one finite float32 that is 0 unless bound is set."""
    from .solve import _spare_weight
    return bool(bound), _spare_weight(spare_weight, bound)


def _weights(weights) -> np.ndarray:
    """Anything array-like of shape [12] or [P, 12] -> finite float32 [P, 12]; [14] or [P, 14], the 14-feature form, likewise."""
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights)
    if w.dtype == object or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
        raise ValueError(f"weights must be numbers of shape [{NUM_FEATURES}] or [P, {NUM_FEATURES}] (or {NUM_MOVE_FEATURES})")
    if w.ndim == 1:
        w = w[None]
    if w.ndim != 2 or w.shape[1] not in FEATURE_COUNTS or w.shape[0] < 1:
        raise ValueError(f"weights must have shape [{NUM_FEATURES}] or [P, {NUM_FEATURES}] (or {NUM_MOVE_FEATURES}: the 14-feature "
                         f"form), got {tuple(np.shape(weights))}")
    with np.errstate(over="ignore"):
        w = np.ascontiguousarray(w, dtype=np.float32)
    if not np.isfinite(w).all():
        raise ValueError("weights must be finite (in float32)")
    return w


def _depth(depth) -> int:
    if isinstance(depth, bool) or depth not in (1, 2):
        raise ValueError("depth must be 1 (the current piece) or 2 (the current and the known next piece)")
    return int(depth)


def _beam_shape(depth, width):
    """The validated (depth, width) of a beam search: integers, not bools, in range."""
    for name, v, top in (("depth", depth, BEAM_MAX_DEPTH), ("width", width, BEAM_MAX_WIDTH)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= top:
            raise ValueError(f"{name} must be an integer in [1, {top}], got {v!r}")
    return int(depth), int(width)


def _members(n: int, rows: int, boards_per_member) -> int:
    """The validated boards_per_member of `rows` weight rows on n boards (None: n for one row, else an even split)."""
    if boards_per_member is None:
        if n % rows:
            raise ValueError(f"{n} boards do not split evenly among {rows} weight rows: give boards_per_member")
        boards_per_member = n // rows
    if isinstance(boards_per_member, bool) or int(boards_per_member) != boards_per_member or int(boards_per_member) < 1:
        raise ValueError("boards_per_member must be a positive integer")
    per = int(boards_per_member)
    if -(-n // per) != rows:
        raise ValueError(f"{n} boards at {per} per member are {-(-n // per)} members, but weights has {rows} rows")
    return per


class _WeightedPolicy:
    """What HeuristicPolicy and BeamPolicy share: the weight rows on the device and the outputs every act() takes."""

    def _setup(self, env, weights, boards_per_member) -> None:
        w = _weights(weights)
        n = _boards(env, type(self).__name__)
        self.boards_per_member = _members(n, w.shape[0], boards_per_member)
        self.env, self.members, self.features = env, int(w.shape[0]), int(w.shape[1])
        # the device buffer act() reads: [P, 12], or [P, 16] with the fourteen in front; `weights` shows [P, 12] or [P, 14] of it
        self._buffer = torch.from_numpy(_learn_lib.padded_weights(w)).to(env.device)
        self.weights = self._buffer[:, :self.features]
        self._planes = None

    def set_weights(self, weights) -> None:
        """Replace the weights (same shape) in the device buffer act() reads."""
        w = _weights(weights)
        if w.shape != tuple(self.weights.shape):
            raise ValueError(f"weights must keep their shape {tuple(self.weights.shape)}")
        self._buffer.copy_(torch.from_numpy(_learn_lib.padded_weights(w)), non_blocking=False)

    def _outputs(self, out, score) -> torch.Tensor:
        """`out` (made where it is None) and `score` checked, and the resident planes at hand."""
        env = self.env
        if out is None:
            out = torch.empty(env.num_envs, dtype=torch.uint8, device=env.device)
        env._own(out, torch.uint8, "out")
        if score is not None:
            env._own(score, torch.float32, "score")
        if self._planes is None:
            self._planes = _state_ptrs(env)                   # the resident planes live as long as the environment
        return out


class HeuristicPolicy(_WeightedPolicy):
    """The linear placement policy on the resident boards of `env`: act() gives every board the arg-max over the distinct
    placements of w . phi(s, a) (left to right in float32; the lowest action on ties; action 0 for a finished board), in one
    launch that leaves the environment as it is.

    weights: [12], or [P, 12] for a population -- board i plays row i // boards_per_member (the last member may be short;
    None: the boards split evenly) --, or [14] / [P, 14]: the 14-feature form with landing_height and eroded_cells.  They are checked finite and uploaded once; set_weights() replaces them in place, so a
    captured graph of act() plays the new ones.

    depth=2 searches two plies (tpl_placement_search): a first placement that does not end the game is worth the best score
    among the distinct placements of the next piece -- window entry 1, which every state carries -- on the board it leaves,
    scored on (rows cleared by both moves, won, lost, the nine features of the final board); one that ends the game is worth
    its one-ply score.  Still one launch and nothing written but the outputs."""

    def __init__(self, env, weights, boards_per_member: Optional[int] = None, depth: int = 1):
        self.depth = _depth(depth)
        self._setup(env, weights, boards_per_member)

    @torch.no_grad()
    def act(self, out: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None,
            second: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [N]: the action of every resident board; `score` (float32 [N], optional) receives the chosen action's score.
        At depth 2 `second` (uint8 [N], optional) receives the placement of the next piece that the score belongs to, 255 where
        the chosen move ends the game or the board is finished.  No host sync, and no allocation when `out` is given:
        capturable into a HIP graph."""
        env = self.env
        if second is not None and self.depth == 1:
            raise ValueError("second is the second ply's placement: this policy has depth 1")
        out = self._outputs(out, score)
        if second is not None:
            env._own(second, torch.uint8, "second")
        stream = torch._C._cuda_getCurrentRawStream(env.device.index)
        name, extra = ("search", (_ptr(second),)) if self.depth == 2 else ("act", ())
        check(_learn_lib.entry(name, self.features)(self._planes[0], self._planes[1], env.num_envs, env.L, env.M,
                                                    self._buffer.data_ptr(), self.boards_per_member, out.data_ptr(), *extra,
                                                    _ptr(score), stream))
        return out


class BeamPolicy(_WeightedPolicy):
    """A beam search with the linear placement score on the resident boards of `env` (tpl_placement_beam; the rule is in
    include/tpl_learn.h).  At moves = m a state's window holds 12 - m mod 10 true next pieces; act() searches
    min(depth, that many) plies: every ply expands each node of the beam by the distinct placements of its current piece,
    scores the child on (rows cleared on the way, won, lost, the nine features of its board) and keeps the `width` best in
    candidate order; the action is the first placement of the best leaf.  depth 1 is HeuristicPolicy; depth 2 with
    width >= 34 is HeuristicPolicy(depth=2).  One launch, nothing written but the outputs.

    weights, boards_per_member, members and set_weights() are HeuristicPolicy's.

    bound=True plays the bounded form (tpl_placement_beam_bound): a move that leaves a board which the move bound proves lost
    leaves it lost, and spare_weight -- one finite number for all weight rows, refused without bound=True -- times a node's spare
    cells is added to its value.  Depth 1 and width 1 make the bounded one-ply player."""

    def __init__(self, env, weights, depth: int, width: int, boards_per_member: Optional[int] = None, bound: bool = False,
                 spare_weight: float = 0.0):
        self.depth, self.width = _beam_shape(depth, width)
        self.bound, self.spare_weight = _bounded(bound, spare_weight)
        self._setup(env, weights, boards_per_member)

    @torch.no_grad()
    def act(self, out: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None,
            plan: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [N]: the action of every resident board; `score` (float32 [N], optional) receives the chosen leaf's value and
        `plan` (uint8 [N, depth], optional) its path: plan[:, 0] is the action, 255 fills what was not searched (a finished
        board, a game that ends on the way, a window with fewer known pieces).  No host sync, and no allocation when `out` is
        given: capturable into a HIP graph."""
        env = self.env
        out = self._outputs(out, score)
        if plan is not None:
            env._own(plan, torch.uint8, "plan", (env.num_envs, self.depth))
        stream = torch._C._cuda_getCurrentRawStream(env.device.index)
        spare = (self.spare_weight,) if self.bound else ()
        check(_learn_lib.entry("beam", self.features, self.bound)(self._planes[0], self._planes[1], env.num_envs, env.L, env.M,
                                                                  self._buffer.data_ptr(), self.boards_per_member, self.depth,
                                                                  self.width, *spare, out.data_ptr(), _ptr(plan), _ptr(score),
                                                                  stream))
        return out


def _player(depth, width):
    """(class, depth, width) of the policy that plays `depth` plies: HeuristicPolicy without a width, else BeamPolicy."""
    if width is None:
        return HeuristicPolicy, _depth(depth), None
    return (BeamPolicy,) + _beam_shape(depth, width)


def _build_player(env, weights, boards_per_member, depth, width, bound=False, spare_weight=0.0):
    if width is None:
        return HeuristicPolicy(env, weights, boards_per_member, depth=depth)
    return BeamPolicy(env, weights, depth, width, boards_per_member, bound=bound, spare_weight=spare_weight)


def _player_bound(width, bound, spare_weight):
    """(bound, spare_weight) of evaluate_heuristic and tune_heuristic: the bounded form is the beam's, so it needs a width."""
    bound, spare_weight = _bounded(bound, spare_weight)
    if bound and width is None:
        raise ValueError("bound=True plays the bounded beam: give a width (depth=1, width=1 is the bounded one-ply player)")
    return bound, spare_weight


def _win_count_reward(env) -> None:
    if tuple(env.reward_params) != (0.0, 1.0, 0.0):
        raise ValueError("evaluate_heuristic counts wins as summed reward: the environment's reward must be (0, 1, 0), "
                         f"not {tuple(env.reward_params)}")


@torch.no_grad()
def evaluate_heuristic(env, weights, boards_per_member: Optional[int], steps: int, policy=None, depth: int = 1,
                       width: Optional[int] = None, bound: bool = False, spare_weight: float = 0.0, per_config: bool = False,
                       proof: Optional[int] = None, proof_table=None, proof_discrepancy=None) -> dict:
    """Play `steps` steps of the population `weights` ([P, 12] or [12]) on `env` from a full reset: an auto-reset environment
    with a configuration pool and reward parameters (0, 1, 0), so that the summed reward is the number of wins.  Member p plays
    boards [p * boards_per_member, (p + 1) * boards_per_member).  Returns episodes and wins as int64 numpy arrays [P] and
    win_rate = wins / max(episodes, 1); the tallies are kept on the device, with one sync at the end.  `policy`: a
    HeuristicPolicy of this environment to reuse (its weights are replaced).  `depth`: 1 or 2 plies (HeuristicPolicy's); a
    `policy` that is passed must have been built with it.  `width`: None, or a beam width -- then a BeamPolicy(depth, width)
    plays, depth may be 1 .. 12, and a `policy` that is passed must be a BeamPolicy of that depth and width.  `bound` and
    `spare_weight` are BeamPolicy's and need a `width`; a `policy` that is passed must have been built with them.
    per_config=True: the dict gains episodes_by_config and wins_by_config, int32 device tensors over the loaded pool summed over the
    members (a PoolTally observed before every step); the three other keys are what they are without it.
    proof: None, or a node budget -- then the policy plays inside a ProofPolicy(env, policy, max_nodes=proof) (solve.py): the first
    move of a plan that the exact search over the state's window proves winning, the policy's own move elsewhere; the dict gains
    proof, that policy's stats().  None leaves every result as it is.
    proof_table: None or False, or with `proof` an n-tuple table of one of the four plain forms (solve.ntuple_window_prove's): the proofs are
    then ordered by it (gamma 1, reward (1, 0, 0)) instead of the classical weights.  It only orders the search.
    proof_discrepancy: None, or with `proof` "add" or "double" -- ProofPolicy's discrepancy: the proofs are searched in
    limited-discrepancy order from first_limit 0.  It changes which proofs fit the node budget, and nothing a proof promises."""
    if not isinstance(per_config, bool):
        raise ValueError("per_config must be True or False")
    if proof_table is False:                                   # NTupleLearner.evaluate's default: the classical order
        proof_table = None
    if proof is None and proof_table is not None:
        raise ValueError("proof_table orders the proofs: it needs proof, a node budget")
    if proof is None and proof_discrepancy is not None:
        raise ValueError("proof_discrepancy orders the proofs: it needs proof, a node budget")
    if proof is not None:
        from .solve import _discrepancy, _max_nodes
        proof = _max_nodes(proof)
        _discrepancy(proof_discrepancy, 0)
    kind, depth, width = _player(depth, width)
    bound, spare_weight = _player_bound(width, bound, spare_weight)
    if policy is not None:
        if isinstance(policy, BeamPolicy) != (kind is BeamPolicy):
            raise ValueError(f"policy is a {type(policy).__name__}, but width={width} asks for a {kind.__name__}")
        if policy.depth != depth:
            raise ValueError(f"policy was built with depth {policy.depth}, not {depth}")
        if width is not None and policy.width != width:
            raise ValueError(f"policy was built with width {policy.width}, not {width}")
        if width is not None and (policy.bound, policy.spare_weight) != (bound, spare_weight):
            raise ValueError(f"policy was built with bound={policy.bound}, spare_weight={policy.spare_weight}, not {bound}, {spare_weight}")
    _win_count_reward(env)
    if not env.auto_reset:
        raise ValueError("evaluate_heuristic needs an auto-reset environment")
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError("steps must be a positive integer")
    if policy is None:
        policy = _build_player(env, weights, boards_per_member, depth, width, bound, spare_weight)
    else:
        if policy.env is not env:
            raise ValueError("policy belongs to another environment")
        policy.set_weights(weights)
        if boards_per_member is not None and int(boards_per_member) != policy.boards_per_member:
            raise ValueError("policy was built with another boards_per_member")
    player = policy
    if proof is not None:
        from .solve import ProofPolicy
        order = {} if proof_table is None else dict(table=proof_table)
        if proof_discrepancy is not None:                      # only then a LimitedProofPolicy
            order["discrepancy"] = proof_discrepancy
        player = ProofPolicy(env, policy, max_nodes=proof, **order)
    n, d = env.num_envs, env.device
    action = torch.empty(n, dtype=torch.uint8, device=d)
    reward = torch.empty(n, dtype=torch.float32, device=d)
    done = torch.empty(n, dtype=torch.uint8, device=d)
    episodes = torch.zeros(n, dtype=torch.int32, device=d)
    wins = torch.zeros(n, dtype=torch.float32, device=d)     # a board wins fewer than 2^24 times: the float sum is exact
    env.reset()
    tally = None
    if per_config:
        from .curriculum import PoolTally
        tally = PoolTally(env)
    for _ in range(int(steps)):
        player.act(out=action)
        if tally is not None:
            tally.observe(action)
        env.step_into(action, reward, done)
        episodes += done
        wins += reward
    member = torch.arange(n, device=d) // policy.boards_per_member
    zeros = torch.zeros(policy.members, dtype=torch.int64, device=d)
    ep = zeros.index_add(0, member, episodes.to(torch.int64)).cpu().numpy()
    wn = zeros.index_add(0, member, wins.to(torch.int64)).cpu().numpy()
    result = dict(episodes=ep, wins=wn, win_rate=wn / np.maximum(ep, 1))
    if tally is not None:
        result.update(episodes_by_config=tally.episodes, wins_by_config=tally.wins)
    if proof is not None:
        result["proof"] = player.stats()
    return result


def tune_heuristic(L: int, M: int, config_pool, population: int = 64, boards_per_member: int = 4096, steps: Optional[int] = None,
                   generations: int = 20, elite_frac: float = 0.125, init_mean=None, init_std: float = 10.0, noise: float = 0.5,
                   seed: int = 0, device="cuda:0", depth: int = 1, width: Optional[int] = None, features: int = NUM_FEATURES,
                   bound: bool = False, spare_weight: float = 0.0) -> dict:
    """The noisy cross-entropy method on the twelve weights, or with features=14 on the fourteen of the 14-feature form (`init_mean`
    must have that length; at 12 the draws and the results are what they were before the argument existed).  Each generation samples `population` weight rows from
    N(mean, diag std^2) with a CPU torch.Generator seeded by `seed`, plays them side by side (`boards_per_member` boards each,
    `steps` steps from a full reset, default 4 M: some four episodes a board) on ONE evaluation environment of
    population * boards_per_member boards over `config_pool` = (rows, pieces) with reward (0, 1, 0), takes fitness = wins /
    max(episodes, 1), and refits mean and std to the best ceil(elite_frac * population) rows, std^2 = var(elite) + noise (the
    constant noise term that keeps the search from freezing early).  `depth`: the plies the members search (1 or 2); with a
    `width` the members are BeamPolicy(depth, width) and depth may be 1 .. 12; `bound` and `spare_weight` are then BeamPolicy's (one
    spare_weight for the whole population: it is not tuned) and are refused without a width.

    Returns mean (float32 [12] or [14], the final one), best (likewise, the best member seen) with best_fitness, and history: one
    dict of host floats per generation (population_mean, elite_mean, best).  Deterministic for a given seed."""
    from .env import BatchedTetris
    _, depth, width = _player(depth, width)
    bound, spare_weight = _player_bound(width, bound, spare_weight)
    for name, v in (("population", population), ("boards_per_member", boards_per_member), ("generations", generations)):
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError(f"{name} must be a positive integer")
    if not 0.0 < float(elite_frac) <= 1.0:
        raise ValueError("elite_frac must be in (0, 1]")
    if not (np.isfinite(init_std) and init_std > 0 and np.isfinite(noise) and noise >= 0):
        raise ValueError("init_std must be positive and noise non-negative")
    if isinstance(features, bool) or features not in FEATURE_COUNTS:
        raise ValueError(f"features must be {NUM_FEATURES} or {NUM_MOVE_FEATURES}, got {features!r}")
    F = int(features)
    P, per = int(population), int(boards_per_member)
    steps = 4 * int(M) if steps is None else int(steps)
    if init_mean is None:
        mean = np.zeros(F, np.float64)
    else:
        try:
            start = _weights(init_mean)
        except ValueError as e:
            raise ValueError(f"init_mean: {e}") from None
        if start.shape[1] != F:
            raise ValueError(f"init_mean must be one row of {F} weights (features={F}), got shape {tuple(np.shape(init_mean))}")
        mean = start[0].astype(np.float64)
    std = np.full(F, float(init_std), np.float64)
    elite = max(1, int(np.ceil(float(elite_frac) * P)))
    env = BatchedTetris(L, M, P * per, device=device, seed=int(seed), auto_reset=True, reward=(0.0, 1.0, 0.0),
                        config_pool=config_pool)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    policy, best, best_fitness, history = None, mean.astype(np.float32), -1.0, []
    try:
        for _ in range(int(generations)):
            z = torch.randn((P, F), generator=gen, dtype=torch.float64).numpy()
            rows = (mean[None, :] + std[None, :] * z).astype(np.float32)
            if policy is None:
                policy = _build_player(env, rows, per, depth, width, bound, spare_weight)
            fitness = evaluate_heuristic(env, rows, per, steps, policy=policy, depth=depth, width=width, bound=bound,
                                         spare_weight=spare_weight)["win_rate"]
            order = np.argsort(-fitness, kind="stable")        # ties: the lower member first
            top = rows[order[:elite]].astype(np.float64)
            if fitness[order[0]] > best_fitness:
                best, best_fitness = rows[order[0]].copy(), float(fitness[order[0]])
            mean, std = top.mean(axis=0), np.sqrt(top.var(axis=0) + float(noise))
            history.append(dict(population_mean=float(fitness.mean()), elite_mean=float(fitness[order[:elite]].mean()),
                                best=float(fitness[order[0]])))
    finally:
        env.terminate()
    return dict(mean=mean.astype(np.float32), best=best, best_fitness=best_fitness, history=history)
