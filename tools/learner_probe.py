"""Timings of the DQN learner on one GPU (profiles/learner/README.md).

    python3 tools/learner_probe.py                 runs every part below as a child process under `timeout -k 10 <s>`, stops at the
                                                   first failure, prints one JSON line per part
    python3 tools/learner_probe.py --part NAME     one part

Parts:
    sample    tpl_replay_sample at B = 65,536 and 2^20 (float32 and bf16 obs), as bytes/s against 6.3 TB/s achievable HBM
    push      tpl_replay_push against the actor_rollout launch that recorded the same chunk
    update    DQNLearner.update() per second at B = 128 and 65,536
    loop      collect(1) + update(4) rounds at N = 262,144 on an L=2 / M=2 pool (win-only reward): transitions/s end to end and
              the greedy win rate before and after
    priority  prioritized replay: tpl_replay_sample_prioritized against tpl_replay_sample (B = 65,536 and 2^20, float32 obs, a
              2^22 ring), tpl_priority_push against tpl_replay_push (16 x 262,144), tpl_priority_update (B = 128 and 65,536),
              DQNLearner.update() per second with and without prioritized=True (B = 128), and the loop's win rate with PER on
    nstep     n-step returns: tpl_replay_sample_nstep at n = 1, 3 and 5 against tpl_replay_sample (and, with the tree, against
              tpl_replay_sample_prioritized) at B = 65,536 and 2^20, float32 obs, a 2^22 ring, every variant timed in each of
              five alternating rounds; DQNLearner.update() at B = 128 with n_step = 1 and 3, alternated three times; the loop's
              win rate with n_step = 3
    mirror    mirror symmetry: tpl_replay_sample_mirror in modes 0 (never), 1 (the coin) and 2 (always) against the existing entry
              of each form -- uniform, prioritized and uniform n = 3 -- at 2^20 draws, float32 obs, a 2^22 ring, every variant
              timed in each of five alternating rounds; the loop's win rate and wall time with mirror=False and mirror=True
    afterstates  tpl_afterstates at 2^16, 2^18 and 2^20 boards (L=10 / M=40, mid-game), the full form and the form without state
              planes, alternated over five rounds: each time as a fraction of 6.3 TB/s over its bytes (32 in, 1,560 or 280 out per
              board) and against the VALU-issue yardstick (the kernel's static vector instructions per wave at 3.3 cycles each on
              1,024 SIMDs at 2.4 GHz); the loop's win rate under evaluate(lookahead=True) next to the greedy one, and one
              LookaheadPolicy.act() at 262,144 boards
    heuristic    the placement policy: tpl_placement_act and tpl_placement_features at 2^16, 2^18 and 2^20 boards (L=10 / M=40,
              mid-game), alternated over five rounds, each against 6.3 TB/s over its bytes and against the VALU-issue yardstick;
              HeuristicPolicy.act() against LookaheadPolicy(env, image=None).act() at 262,144 boards, alternated in one process;
              act() + step() env-steps/s at 2^20 boards; win rates of the uniform random policy, the reward weights and
              tune_heuristic's weights on the loop's L=2 / M=2 pool and on an L=10 / M=40 carved pool (>= 10^6 episodes each)
    search       the two-ply placement search: tpl_placement_search at 2^16, 2^18 and 2^20 boards (L=10 / M=40, mid-game) against its
              instruction price (per wave: the static vector instructions outside the second-ply loop once, the loop's as often as
              the wave's slowest board has distinct placements of its next piece); HeuristicPolicy(depth=2).act() against the
              composition it replaces at 262,144 boards (per 16,384-board chunk: afterstates into a scratch environment,
              tpl_placement_act over its 40 x 16,384 boards, a torch max), alternated in one process; win rates at depth 1 and 2
              of the classical signs and of a tuned row on the L=2 / M=2 pool and an L=10 / M=40 carved pool (>= 10^6 episodes
              each, with standard errors)
    beam         the beam search: BeamPolicy.act() at 2^16 and 2^20 boards (L=10 / M=40, mid-game) for (depth, width) in (2, 34),
              (3, 8), (4, 16), (6, 16), (12, 64) beside tpl_placement_search on the same boards, alternated over three rounds;
              the yardstick is the two-ply kernel of the same run and the prediction the moves per board of the two rules on these
              boards (their windows' known pieces and placement counts); win rates of the classical signs at depth 1 and 2 and
              at (3, 8), (4, 16) and (6, 16) on an L=10 / M=40 carved pool
    ntuple       the n-tuple value function: tpl_ntuple_act at 2^16, 2^18 and 2^20 boards (L=10 / M=40, mid-game, a random table)
              beside tpl_placement_act and tpl_placement_search on the same boards, and tpl_ntuple_value and tpl_ntuple_update
              against their gathered / added bytes (4 per tuple in use and the counter, counted on a sample of the boards) at the
              scattered-atomic figure of 0.08 TB/s, everything alternated over five rounds of 20 launches after 3 warm-ups; the
              win rate of NTupleLearner on the two-piece game and on an L=10 / M=40 carved pool (>= 10^6 episodes) beside the
              zero table's and the classical weights' at one ply
    ntuple_search  the two-ply n-tuple policy: tpl_ntuple_search at 2^16, 2^18 and 2^20 boards (L=10 / M=40, mid-game, a random
              table) beside tpl_ntuple_act and tpl_placement_search on the same boards, against its instruction price (per wave:
              tpl_ntuple_act's vector instructions outside its gather loop once, and per trip of the wave's slowest board the
              second-ply loop's outside its gather loop plus 17 times the gather loop's, all as built); NTuplePolicy(depth=2).act()
              against the composition it replaces at 262,144 boards (per 16,384-board chunk: afterstates into a scratch
              environment, tpl_ntuple_act over its 40 x 16,384 boards, a torch max), alternated in one process; on an L=10 / M=40
              carved pool the win rates at depth 1 and 2 of a table trained at depth 1 and of one trained at depth 2 (the shaped
              reward, 4,096 boards, 40,000 steps) beside the classical weights' at one and two plies
    ntuple_trace   the update with traces and mirror symmetry: tpl_ntuple_update_trace at 2^16, 2^18 and 2^20 boards for horizon 1, 4,
              8 and 16, symmetric and not, decay 0.9 and errors of order 1, over a ring of 17 slots that holds the boards' last 17
              states (L=10 / M=40, mid-game), alternated over five rounds with tpl_ntuple_update on the newest slot; the prediction
              is tpl_ntuple_update's time of the same run times the (board, age) pairs that add (the trace is open and the step is
              not 0) per board, times two where symmetric; bytes/s by the entries in use as part ntuple counts them
    ntuple_trace_sweep  NTupleLearner on part ntuple's L=10 / M=40 carved pool (the shaped reward, 4,096 boards, epsilon 0.05, gamma
              1, 40,000 steps, wins over 12,288 greedy steps): the TD(0) baseline at rate 16 re-run, then lambda in 0.5, 0.8, 0.9 x
              horizon in 4, 8 x symmetric or not x rate in 4, 8, 16, and symmetry alone (horizon 1) at the three rates
    ntuple_coherent  temporal-coherence step sizes: tpl_ntuple_update_coherent beside tpl_ntuple_update_trace (and tpl_ntuple_update
              on the newest slot) in the same alternated rounds, part ntuple_trace's ring, errors and method, at 2^16, 2^18 and
              2^20 boards for horizon 1 and 4, symmetric and not, on a coherence buffer that three calls with other errors have
              filled (most step sizes far below 1, so part of the steps round to 0 and their adds are skipped) and, as the other
              end, with errors of one sign on a buffer of its own (every step size 1, every add made); the two phases' own times
              from the kernel records of torch.profiler over five more calls; added bytes/s: 4 per entry and add for the step phase
              (which also gathers 16), 16 for the accumulate phase
    ntuple_coherent_sweep  part ntuple_trace_sweep's set-up unchanged (pool, seed, reward, epsilon, gamma, budget, evaluation) with
              coherent on and off: TD(0), lambda 0.5 / horizon 8 and symmetric lambda 0.8 / horizon 4 at rates 4, 8, 16, 32 and 64
              each (TD(0) at rate 16 without coherence is the baseline), and the two-piece game (4,096 boards, 300 steps) at rates
              64, 256 and 1,024; win rates after 10,000 and 40,000 steps, the largest entry, and alpha over the entries that were
              sent a step.  --chunk I/K runs every K-th cell from the I-th on, for a run in several processes
    ntuple_shape   the 3 x 3 table shape beside 2 x 4: on part ntuple_trace's ring (L=10 / M=40, mid-game, 17 slots) at 2^16, 2^18 and
              2^20 boards every _shaped entry at shape 1 beside the same entry at shape 0 in the same alternated rounds -- value,
              act, search, update, update_trace at horizon 4 plain and symmetric, update_coherent at horizon 4 --, each shape on a
              random table of its own size; the entries in use per running board of both shapes, and the static vector instructions
              of every kernel of both
    ntuple_shape_sweep  part ntuple_trace_sweep's set-up unchanged (pool, seed, reward, epsilon, gamma, budget, evaluation): the 2 x 4
              TD(0) baseline at rate 16 re-run, then shape 3 x 3 at rates 4, 8, 16 and 32 as TD(0), lambda 0.5 / horizon 8 and
              symmetric lambda 0.8 / horizon 4; the best 3 x 3 table is also played at depth 2
    ntuple_beam    the n-tuple beam search: tpl_ntuple_beam at 2^20 boards (L=10 / M=40, mid-game, a random table of each shape) for
              (depth, width) in (1, 1), (2, 34), (3, 8), (4, 16), (6, 16), (11, 64) beside tpl_ntuple_act and tpl_ntuple_search on the
              same boards and tpl_placement_beam at the same (depth, width), alternated over three rounds; the price is (tuples in
              use) x (moves per board, by the windows' known pieces and placement counts) gathers at the rate act and search resolve
              theirs in the same run; the ratio to tpl_ntuple_search at (2, 34), where both make the same moves and gathers; win
              rates of part ntuple_shape_sweep's TD(0) tables (2 x 4 and 3 x 3, rate 16, one seed) on the L=10 / M=40 carved pool
              at depth 1, at depth 2 and with beams (3, 8), (4, 16) and (6, 16)
    ntuple_sum     a sum table (2 x 4 and 3 x 3 summed in one value) beside its two twins, the tables that are its parts: on part
              ntuple_shape's boards at 2^16, 2^18 and 2^20 the value, act, search, the beam at (3, 8) and (6, 16) and one learner step,
              plain and coherent, of all three in the same alternated rounds, each as a ratio to the two twins' times added; the
              entries in use per running board
    ntuple_sum_sweep  part ntuple_shape_sweep's set-up unchanged: the 2 x 4 and 3 x 3 TD(0) runs at rate 16 again (they must reproduce
              win for win), then a sum table as TD(0) at rates 2, 4, 8 and 16; the best one is also played at depth 2 and at beam (3, 8)
    ntuple_stage   staged tables (eight tables of a form and a stage map) beside their plain twins: at 2^20 boards (L=10 / M=40,
              part ntuple_shape's, played on for 200 steps so that they stand in several stages) the value, act, search, the beam at (3, 8) and one learner step for each of the three
              forms -- the plain table, a staged one whose all-zero map keeps one stage live, and one under the four-stage moves=4 map,
              eight distinct random blocks each -- in the same alternated rounds, each staged time as a ratio to its plain twin's
    ntuple_stage_sweep  part ntuple_shape_sweep's set-up unchanged: the 3 x 3 TD(0) run at rate 16 again (it must reproduce win for
              win), then a staged 3 x 3 table under the maps moves=2, moves=4 and lines=2 x moves=4, each trained from zero and each
              promoted from the baseline's table and trained on for the same budget; every final table played at one ply, at depth 2
              and at beam (3, 8)
    ntuple_feature  feature tables ("feat", and "3x3+feat", a 3 x 3 table with a feature table behind it) beside the 3 x 3 table: at 2^20
              boards (part ntuple_shape's) the value, act, search, the beam at (3, 8) and (6, 16) and one learner step of all three in the
              same alternated rounds, "feat" as a ratio to the 3 x 3 twin and "3x3+feat" as a ratio to the two parts' times added; the
              update kernel alone at horizons 1 and 4 beside the 3 x 3 update
    ntuple_feature_sweep  part ntuple_shape_sweep's set-up unchanged: the 3 x 3 TD(0) run at rate 16 again (it must reproduce win for
              win) and the classical weights at one ply; "feat" as TD(0) at rates 2 .. 512 and "3x3+feat" at rates 2 .. 16; the best of
              each with symmetric updates; the best of each played at depth 2 and at beam (3, 8)
    ntuple_budget  the budget table ("feat+spare") beside its "feat" twin at 2^20 boards (part ntuple_shape's): value, act, search, the
              beam at (3, 8) and (6, 16) -- the policies with the prune off and on --, one learner step, and the update kernel alone
              at horizons 1 and 4, each as a ratio to the twin's time in the same alternated rounds
    ntuple_budget_sweep  the tight pool of the record (carved L=10 / M=40, 65,536 configurations, seed 7, solved at width 16,
              tighten_pool(M_new=16)): the rate-8 "feat" learner again (it must reproduce win for win), then "feat+spare" from zero at
              rates 2 .. 32 and from the promoted "feat" table, each trained with the prune off and on and played at one ply and at
              beam (3, 8) with the prune off and on; the promoted table untrained is the prune alone; the loose pool once
    exact     the exact depth-first solver (tpl_placement_exact, prove_configs) on the record's pool (carved L=10 / M=40, 65,536
              configurations, seed 7) at budgets of config_bound + 0, 1, 2 and max_nodes 2^12, 2^16 and 2^20: proved, solved and proved
              unwinnable, mean and maximum nodes, seconds and nodes a second, the bounded beam at widths 16 and 64 beside it, and how
              much of what width 64 leaves unsolved is then solved and proved shortest
    ntuple_exact  the exact search with its children ordered by a table (tpl_ntuple_exact, ntuple_prove_configs) on part exact's pool at
              the exact budget: the classical-weights rows of part exact at 2^12 and 2^16 nodes again (they must reproduce win for win),
              then the same under the rate-8 "feat" table trained on the loose pool and the "feat+spare" tables trained on the tight
              pool without and with the prune -- proved, mean nodes, seconds, the share of what the width-64 beam leaves unsolved that
              each closes, and the 2 x 2 of which configurations each ordering proves; and the nodes a second of the four kernels as
              a ratio to tpl_placement_exact's in five alternated rounds at 2^12 nodes
    ntuple_shape_ab  --parent LIB: the nine 2 x 4 n-tuple kernels of another build of the learner library against this tree's, both
              loaded into one process: the outputs of the six entries compared byte for byte on the ring of part ntuple_shape
              at 2^18 boards, then each entry timed in five rounds of the parent against itself and five of the parent against
              this build; a new median passes within the parent's own min-max or at most 2 % above the parent's median
    exact_ab  --parent LIB: the ten plain and the six limited entries of the five exact-search units (exact, exact_nodes,
              exact_window, ntuple_exact, ntuple_window) of another build of the learner library against this tree's, both loaded
              into one process: carved L=10 / M=40, 4,096 roots, and 4,096 nodes and resident boards ten moves on, max_nodes 2^12,
              the table entries under each of the four plain forms, the limited ones at first_limit 0; every output compared byte
              for byte (the limited under "add" and "double"), then each call timed by ntuple_shape_ab's protocol (the limited
              under "add"; --no-timing: the comparison alone)
    labels    the proved move labels (tpl_placement_exact_labels, label_states) on the tight pool of the record (part bound's: carved
              L=10 / M=40, 65,536 configurations, seed 7, solved at width 16, tighten_pool(M_new=16)): the classical weights at one ply
              and at beam (3, 8) play one episode on 4,096 boards, label_states (max_nodes 2^12 a child) before every step -- per move
              number the share of running boards whose every distinct move is proved and the blunder rate, the share of lost episodes
              with a proved first blunder, the milliseconds of a label_states call, and the nodes a second beside prove_configs on the
              same pool in the same run
    rank      the ranking update from proved move labels (tpl_ntuple_rank, NTupleRanker, collect_labels, label_agreement): rank() of
              each of the four forms beside NTuplePolicy.act() and a whole step() beside a learner step, alternated, at 2^20 boards;
              then on the tight pool of the record split by pool entry: labels collected under the rate-8 "feat+spare" TD table, fit()
              from that table and from zero, and on the held-out half label_agreement, the one-ply and the beam (3, 8) win rate before
              and after, with one sweep over rate and margin
    window    the exact search over a state's piece window and the proof policy (tpl_placement_window_prove, window_prove,
              ProofPolicy) on the tight pool of the record (part bound's): the record's two classical rows again (they must reproduce
              win for win), then on 4,096 boards the classical one-ply player and the beam (3, 8), each alone and inside a ProofPolicy
              at max_nodes 2^8, 2^12 and 2^16 -- win rate with its standard error, the verdicts 1, 2 and 3 per move number as shares of
              the running boards, the episodes that held a verdict 1 and did not end won (which must be 0), the milliseconds of a
              played step with reuse off and on beside the base's in alternated rounds, and the nodes a second of window_prove beside
              prove_nodes on the same boards; the loose pool once.  --sections and --budgets choose what one call runs
    limited   the exact searches in limited-discrepancy order (tpl_placement_exact_limited and its five kin; prove_configs_limited,
              ProofPolicy(discrepancy=)) beside the plain kernels IN THE SAME RUN, the legs alternated: the share of part exact's pool
              proved at its exact budget at 2^12 and 2^16 nodes under the plain order, "add" and "double", and what each closes of what
              the width-64 beam leaves unsolved; the nodes a second of each limited kernel at first_limit 65,535 -- the plain kernel's
              work -- as a ratio to its twin, and at first_limit 0; the nodes both growths take to search out budgets that hold no win,
              over the plain search's; on part window's tight pool the one-ply player and the beam (3, 8) inside a ProofPolicy at 2^8 and
              2^12 nodes, plain against "add".  Under the classical weights and under part ntuple_exact's "feat+spare" table, made here
              by its recipe.  --sections chooses what one call runs.  One seed, one pool
    solve     the whole-game beam solver (tpl_placement_solve, solve_configs) under the classical weights: the share of forward seeds
              0 .. 9,999 it solves at L=5 / M=20 and L=10 / M=40 at widths 1, 8, 16 and 64 beside the share the reference's solver marks
              winnable in the same forward_configs call, and the share of the sweeps' carved pool (65,536, seed 7) it solves; the
              histogram of its solution lengths there beside carving's; the pool tighten_pool makes at the median length and the win
              rates on it of the classical weights at one ply, of the beam (3, 8) and of the rate-8 "feat" learner trained on it under the
              sweeps' set-up; configurations a second at 2^16 and 2^20 configurations at widths 8, 16 and 64 (the median of five timings
              after a warm-up) beside tpl_placement_beam at (12, W) on as many freshly reset boards, scaled by the mean plies run over
              12, and beside the forward generator's games a second
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
PARTS = {"sample": 300, "push": 300, "update": 300, "loop": 600, "priority": 600, "nstep": 600, "mirror": 600, "afterstates": 600,
         "heuristic": 600, "search": 900, "beam": 900, "ntuple": 900,
         "ntuple_search": 900, "ntuple_trace": 600, "ntuple_trace_sweep": 1100, "ntuple_coherent": 600,
         "ntuple_coherent_sweep": 1700, "ntuple_shape": 600, "ntuple_shape_sweep": 1100, "ntuple_beam": 1100,
         "ntuple_sum": 600, "ntuple_sum_sweep": 600, "ntuple_stage": 600, "ntuple_stage_sweep": 900,
         "ntuple_feature": 600, "ntuple_feature_sweep": 900, "solve": 900, "move_features": 1100, "bound": 900,
         "ntuple_budget": 600, "ntuple_budget_sweep": 1100, "exact": 900, "ntuple_exact": 900, "labels": 900,
         "rank": 1100, "window": 1100, "ntuple_window": 1100, "limited": 1100}
SCATTERED_ATOMICS = 0.08e12                                 # 64 lanes of a wave adding into 64 rows (float adds; integer adds unmeasured)
VALU_CYCLES, SIMDS, CLOCK_HZ = 3.3, 1024, 2.4e9           # the move's instruction mix, 256 CUs x 4, the clock


def _timed(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / 1e3 / reps


def _filled_ring(n=1 << 18, steps=16, prioritized=False):
    import torch
    import tetris_piclim as T
    env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
    env.load_configs(*env.synthetic_configs(4096))
    env.reset()
    torch.manual_seed(0)
    image = T.actor.policy_image(T.PolicyMLP(), env.device, f32="split")
    ring = (T.PrioritizedReplayRing if prioritized else T.ReplayRing)(n * steps, env.device)
    traj = env.actor_rollout(image, steps, epsilon=0.5, seed=3, record=True, record_states=True)
    ring.push(env, traj)
    return env, image, ring, traj


def part_sample():
    import torch
    import tetris_piclim as T
    env, _, ring, _ = _filled_ring()
    out = []
    for batch in (65536, 1 << 20):
        next_env = T.BatchedTetris(10, 40, batch, device="cuda:0", seed=2)
        for dtype, obs_bytes in ((torch.float32, 868), (torch.bfloat16, 434)):
            k = [0]

            def draw():
                k[0] += 1
                ring.sample(batch, 7, k[0], next_env, obs_dtype=dtype)
            t = _timed(draw, 20)
            moved = batch * (80 + obs_bytes + 32 + 6)          # record read; obs, s' planes, action / reward / done written
            out.append(dict(batch=batch, obs=str(dtype).split(".")[-1], us=round(t * 1e6, 2), bytes_per_draw=80 + obs_bytes + 38,
                            tb_per_s=round(moved / t / 1e12, 3), of_achievable=round(moved / t / HBM_ACHIEVABLE, 3)))
        next_env.terminate()
    return dict(part="sample", ring=ring.capacity, rows=out)


def part_push():
    import torch
    env, image, ring, traj = _filled_ring()
    n, steps = env.num_envs, traj["actions"].shape[0]
    t_push = _timed(lambda: ring.push(env, traj), 20)
    t_roll = _timed(lambda: env.actor_rollout(image, steps, epsilon=0.5, seed=3, record=True, record_states=True), 5, warmup=1)
    moved = n * steps * (80 + 32 + 32 + 6)
    return dict(part="push", boards=n, steps=steps, push_us=round(t_push * 1e6, 1), rollout_us=round(t_roll * 1e6, 1),
                push_over_rollout=round(t_push / t_roll, 4), push_tb_per_s=round(moved / t_push / 1e12, 3))


def part_update():
    import torch
    import tetris_piclim as T
    rows = []
    for batch in (128, 65536):
        env = T.BatchedTetris(10, 40, 1 << 16, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        torch.manual_seed(0)
        learner = T.DQNLearner(env, capacity=1 << 20, batch_size=batch, seed=1)
        learner.collect(8)
        learner.update(5)
        torch.cuda.synchronize()
        reps = 200 if batch == 128 else 50
        t0 = time.perf_counter()
        learner.update(reps)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        rows.append(dict(batch=batch, updates_per_s=round(1 / dt, 1), ms_per_update=round(dt * 1e3, 3)))
        env.terminate()
    return dict(part="update", rows=rows)


def part_loop(prioritized=False, n_step=1, mirror=False, lookahead=False):
    import torch
    import tetris_piclim as T
    n, rounds, per = 262144, 300, 4
    rows, pieces = T.generate_configs(2, 2, 64, seed=100)
    env = T.BatchedTetris(2, 2, n, device="cuda:0", seed=0, auto_reset=True, reward=(0.0, 1.0, 0.0))
    env.load_configs(rows, pieces)
    env.reset()
    torch.manual_seed(0)
    learner = T.DQNLearner(env, capacity=1 << 22, batch_size=1024, eps_start=1.0, eps_end=0.05, eps_decay=10, tau=0.05,
                           lr=1e-3, seed=0, prioritized=prioritized, n_step=n_step, mirror=mirror)
    before = learner.evaluate(8)["win_rate"]
    random_rate = learner.evaluate(8, epsilon=1.0)["win_rate"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    curve = []
    for r in range(rounds):
        learner.collect(1)
        learner.update(per)
        if (r + 1) % 100 == 0:
            torch.cuda.synchronize()
            curve.append((r + 1, round(time.perf_counter() - t0, 2)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    after = learner.evaluate(8)
    out = dict(part="loop", boards=n, rounds=rounds, updates_per_round=per, batch=1024, seconds=round(dt, 2),
               transitions_per_s=round(rounds * n / dt), updates_per_s=round(rounds * per / dt, 1), elapsed_at=curve,
               win_rate_random=round(random_rate, 4), win_rate_greedy_before=round(before, 4),
               win_rate_greedy_after=round(after["win_rate"], 4), eval_episodes=after["episodes"])
    if lookahead:
        look = learner.evaluate(8, lookahead=True)
        policy = learner._lookahead
        action = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        t_act = _timed(lambda: policy.act(out=action), 5, warmup=1)
        bare = T.LookaheadPolicy(learner.eval_env, image=None)
        t_bare = _timed(lambda: bare.act(out=action), 5, warmup=1)
        out.update(win_rate_lookahead_after=round(look["win_rate"], 4), lookahead_eval_episodes=look["episodes"],
                   lookahead_act_ms=round(t_act * 1e3, 3), lookahead_act_without_network_ms=round(t_bare * 1e3, 3),
                   lookahead_chunk=policy.chunk)
    return out


def _update_rate(batch, prioritized, reps=200, n_step=1):
    import torch
    import tetris_piclim as T
    env = T.BatchedTetris(10, 40, 1 << 16, device="cuda:0", seed=1, auto_reset=True)
    env.load_configs(*env.synthetic_configs(4096))
    env.reset()
    torch.manual_seed(0)
    learner = T.DQNLearner(env, capacity=1 << 20, batch_size=batch, seed=1, prioritized=prioritized, n_step=n_step)
    learner.collect(8)
    learner.update(5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    learner.update(reps)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    env.terminate()
    return dt


def part_priority():
    import torch
    import tetris_piclim as T
    L = T._learn_lib.lib()
    out = dict(part="priority")
    env, _, ring, traj = _filled_ring(prioritized=True)
    stream = torch._C._cuda_getCurrentRawStream(0)
    # sample: prioritized against uniform on the same 2^22 ring (every slot at the running maximum)
    rows = []
    for batch in (65536, 1 << 20):
        next_env = T.BatchedTetris(10, 40, batch, device="cuda:0", seed=2)
        k = [0]

        def uniform():
            k[0] += 1
            T.ReplayRing.sample(ring, batch, 7, k[0], next_env)

        def prioritized():
            k[0] += 1
            ring.sample(batch, 7, k[0], next_env)
        tu, tp = _timed(uniform, 20), _timed(prioritized, 20)
        rows.append(dict(batch=batch, uniform_us=round(tu * 1e6, 2), prioritized_us=round(tp * 1e6, 2),
                         ratio=round(tp / tu, 3)))
        next_env.terminate()
    out["sample"] = dict(ring=ring.capacity, obs="float32", rows=rows)
    # push: the tree's share of a 16 x 262,144 push
    n, steps = env.num_envs, traj["actions"].shape[0]
    t_ring = _timed(lambda: T.ReplayRing.push(ring, env, traj), 20)
    t_tree = _timed(lambda: T._learn_lib.check(L.tpl_priority_push(ring.tree.data_ptr(), ring.capacity, 0, n * steps, stream)), 20)
    out["push"] = dict(transitions=n * steps, replay_push_us=round(t_ring * 1e6, 1), priority_push_us=round(t_tree * 1e6, 1),
                       ratio=round(t_tree / t_ring, 3))
    # write-back
    rows = []
    for batch in (128, 65536):
        index = torch.randint(0, ring.capacity, (batch,), device="cuda:0", dtype=torch.int64)
        prio = torch.rand(batch, device="cuda:0", dtype=torch.float64) + 0.5
        t = _timed(lambda: T._learn_lib.check(L.tpl_priority_update(ring.tree.data_ptr(), ring.capacity, batch, index.data_ptr(),
                                                                     prio.data_ptr(), stream)), 20)
        rows.append(dict(batch=batch, us=round(t * 1e6, 2)))
    out["update_priorities"] = rows
    env.terminate()
    del ring, traj
    torch.cuda.empty_cache()
    # DQNLearner.update(): both modes, same box, same run, alternated
    uni, per = [], []
    for _ in range(2):
        uni.append(_update_rate(128, False))
        per.append(_update_rate(128, True))
    tu, tp = min(uni), min(per)
    out["learner_update"] = dict(batch=128, uniform_updates_per_s=round(1 / tu, 1), prioritized_updates_per_s=round(1 / tp, 1),
                                 prioritized_overhead=round(tp / tu - 1, 4))
    torch.cuda.empty_cache()
    loop = part_loop(prioritized=True)
    loop["part"] = "loop_prioritized"
    out["loop"] = loop
    return out


def _spread(ts):
    """min / median / max of a list of seconds, in µs."""
    s = sorted(ts)
    return dict(min=round(s[0] * 1e6, 2), median=round(s[len(s) // 2] * 1e6, 2), max=round(s[-1] * 1e6, 2))


def part_nstep(rounds=5):
    import ctypes as C
    import torch
    import tetris_piclim as T
    L = T._learn_lib.lib()
    check = T._learn_lib.check
    out = dict(part="nstep")
    env, _, ring, _ = _filled_ring(prioritized=True)
    stream = torch._C._cuda_getCurrentRawStream(0)
    cap, size, head, stride = ring.capacity, ring.size, ring.head, ring.stride
    gamma, seed = 0.99, 7
    rows = []
    for batch in (65536, 1 << 20):
        next_env = T.BatchedTetris(10, 40, batch, device="cuda:0", seed=2)
        pa, pb = C.c_void_p(), C.c_void_p()
        T._lib.check(next_env._lib.tpl_state_ptrs(next_env._h, C.byref(pa), C.byref(pb)))
        e = lambda dt: torch.empty(batch, dtype=dt, device="cuda:0")
        obs = torch.empty((batch, 217), dtype=torch.float32, device="cuda:0")
        action, reward, done, steps = e(torch.uint8), e(torch.float32), e(torch.uint8), e(torch.uint8)
        discount, index, prob = e(torch.float32), e(torch.int64), e(torch.float32)
        f32 = T.learn._OBS_CODES[torch.float32]
        k = [0]

        def ref(tree):
            k[0] += 1
            if tree is None:
                check(L.tpl_replay_sample(ring.data.data_ptr(), cap, size, batch, seed, k[0], 10, 40, obs.data_ptr(), f32, pa.value,
                                          pb.value, action.data_ptr(), reward.data_ptr(), done.data_ptr(), index.data_ptr(),
                                          stream))
            else:
                check(L.tpl_replay_sample_prioritized(ring.data.data_ptr(), tree, cap, size, batch, seed, k[0], 10, 40,
                                                      obs.data_ptr(), f32, pa.value, pb.value, action.data_ptr(),
                                                      reward.data_ptr(), done.data_ptr(), index.data_ptr(), prob.data_ptr(),
                                                      stream))

        def nstep(tree, n):
            k[0] += 1
            check(L.tpl_replay_sample_nstep(ring.data.data_ptr(), tree, cap, size, head, stride, n, gamma, batch, seed, k[0], 10,
                                            40, obs.data_ptr(), f32, pa.value, pb.value, action.data_ptr(), reward.data_ptr(),
                                            discount.data_ptr(), done.data_ptr(), steps.data_ptr(), index.data_ptr(),
                                            None if tree is None else prob.data_ptr(), stream))
        for mode, tree in (("uniform", None), ("prioritized", ring.tree.data_ptr())):
            variants = [("ref", lambda: ref(tree))] + [(f"n{n}", (lambda n=n: nstep(tree, n))) for n in (1, 3, 5)]
            times = {name: [] for name, _ in variants}
            for _ in range(rounds):                              # alternate the variants round by round
                for name, fn in variants:
                    times[name].append(_timed(fn, 20))
            med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
            rows.append(dict(batch=batch, mode=mode, us={name: _spread(ts) for name, ts in times.items()},
                             ratio_of_medians={name: round(med[name] / med["ref"], 3) for name in med if name != "ref"}))
        next_env.terminate()
    out["sample"] = dict(ring=cap, obs="float32", rounds=rounds, launches_per_timing=20, rows=rows)
    env.terminate()
    del ring
    torch.cuda.empty_cache()
    one, three = [], []
    for _ in range(3):
        one.append(_update_rate(128, False))
        three.append(_update_rate(128, False, n_step=3))
    out["learner_update"] = dict(batch=128, n1_ms=[round(t * 1e3, 4) for t in one], n3_ms=[round(t * 1e3, 4) for t in three],
                                 n1_spread=round(max(one) / min(one) - 1, 4),
                                 n3_over_n1_median=round(sorted(three)[1] / sorted(one)[1] - 1, 4))
    torch.cuda.empty_cache()
    loop = part_loop(n_step=3)
    loop["part"] = "loop_nstep3"
    out["loop"] = loop
    return out


def part_mirror(rounds=5):
    import ctypes as C
    import torch
    import tetris_piclim as T
    L = T._learn_lib.lib()
    check = T._learn_lib.check
    out = dict(part="mirror")
    env, _, ring, _ = _filled_ring(prioritized=True)
    stream = torch._C._cuda_getCurrentRawStream(0)
    cap, size, head, stride = ring.capacity, ring.size, ring.head, ring.stride
    gamma, seed, batch = 0.99, 7, 1 << 20
    next_env = T.BatchedTetris(10, 40, batch, device="cuda:0", seed=2)
    pa, pb = C.c_void_p(), C.c_void_p()
    T._lib.check(next_env._lib.tpl_state_ptrs(next_env._h, C.byref(pa), C.byref(pb)))
    e = lambda dt: torch.empty(batch, dtype=dt, device="cuda:0")
    obs = torch.empty((batch, 217), dtype=torch.float32, device="cuda:0")
    action, reward, done, steps, mirrored = e(torch.uint8), e(torch.float32), e(torch.uint8), e(torch.uint8), e(torch.uint8)
    discount, index, prob = e(torch.float32), e(torch.int64), e(torch.float32)
    f32 = T.learn._OBS_CODES[torch.float32]
    tree = ring.tree.data_ptr()
    k = [0]
    front = (obs.data_ptr(), f32, pa.value, pb.value, action.data_ptr(), reward.data_ptr())

    def existing(form):
        k[0] += 1
        if form == "uniform":
            check(L.tpl_replay_sample(ring.data.data_ptr(), cap, size, batch, seed, k[0], 10, 40, *front, done.data_ptr(),
                                      index.data_ptr(), stream))
        elif form == "prioritized":
            check(L.tpl_replay_sample_prioritized(ring.data.data_ptr(), tree, cap, size, batch, seed, k[0], 10, 40, *front,
                                                  done.data_ptr(), index.data_ptr(), prob.data_ptr(), stream))
        else:
            check(L.tpl_replay_sample_nstep(ring.data.data_ptr(), None, cap, size, head, stride, 3, gamma, batch, seed, k[0], 10, 40,
                                            *front, discount.data_ptr(), done.data_ptr(), steps.data_ptr(), index.data_ptr(), None,
                                            stream))

    def mirror(form, mode):
        k[0] += 1
        n = 3 if form == "nstep3" else 0
        check(L.tpl_replay_sample_mirror(ring.data.data_ptr(), tree if form == "prioritized" else None, cap, size, head, stride, n,
                                         gamma, batch, seed, k[0], 10, 40, *front, discount.data_ptr() if n else None,
                                         done.data_ptr(), steps.data_ptr() if n else None, index.data_ptr(),
                                         prob.data_ptr() if form == "prioritized" else None, mode, mirrored.data_ptr(), stream))
    rows = []
    for form in ("uniform", "prioritized", "nstep3"):
        variants = [("existing", lambda: existing(form))] + [(f"mode{m}", (lambda m=m: mirror(form, m))) for m in (0, 1, 2)]
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                                  # alternate the variants round by round
            for name, fn in variants:
                times[name].append(_timed(fn, 20))
        med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        rows.append(dict(batch=batch, form=form, us={name: _spread(ts) for name, ts in times.items()},
                         ratio_to_mode0={name: round(med[name] / med["mode0"], 3) for name in med if name != "mode0"}))
    mirror("uniform", 1)
    torch.cuda.synchronize()
    out["sample"] = dict(ring=cap, obs="float32", rounds=rounds, launches_per_timing=20, rows=rows,
                         mirrored_fraction_of_last_coin_draw=round(float(mirrored.float().mean()), 4))
    next_env.terminate()
    env.terminate()
    del ring
    torch.cuda.empty_cache()
    loops = []
    for flag in (False, True, False, True):                      # alternated: the wall time's own spread shows
        loop = part_loop(mirror=flag)
        loop["part"] = "loop_mirror" if flag else "loop_plain"
        loops.append(loop)
        torch.cuda.empty_cache()
    out["loops"] = loops
    return out


def _static_valu(kernel, lib_path):
    """Vector ALU instructions in the kernel's code as built (tools/dump_isa.sh): every path once, loop bodies included."""
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "dump_isa.sh"), kernel, lib_path], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    return sum(1 for l in res.stdout.splitlines() if l.split()[:1] and l.split()[0].startswith("v_"))


def part_afterstates(rounds=5):
    import ctypes as C
    import torch
    import tetris_piclim as T
    L = T._learn_lib.lib()
    check = T._learn_lib.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    valu = _static_valu("afterstates_kernel", T._learn_lib.build_library())
    out = dict(part="afterstates", static_valu_per_wave=valu, valu_cycles=VALU_CYCLES, streaming_tb_per_s=HBM_ACHIEVABLE / 1e12)
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        for t in range(6):                                       # mid-game boards
            env.step(env.synthetic_actions(t), observe=False)
        pa, pb = C.c_void_p(), C.c_void_p()
        T._lib.check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
        sa = torch.empty((n, 40, 4), dtype=torch.int32, device="cuda:0")
        sb = torch.empty((n, 40, 4), dtype=torch.int32, device="cuda:0")
        reward = torch.empty((n, 40), dtype=torch.float32, device="cuda:0")
        done, cleared, canonical = (torch.empty((n, 40), dtype=torch.uint8, device="cuda:0") for _ in range(3))

        def launch(planes):
            check(L.tpl_afterstates(pa.value, pb.value, n, 10, 40, 1.0, 0.0, 0.0, sa.data_ptr() if planes else None,
                                    sb.data_ptr() if planes else None, reward.data_ptr(), done.data_ptr(), cleared.data_ptr(),
                                    canonical.data_ptr(), stream))
        variants = [("full", lambda: launch(True), 32 + 40 * 39), ("no_planes", lambda: launch(False), 32 + 40 * 7)]
        times = {name: [] for name, _, _ in variants}
        for _ in range(rounds):                                  # alternate the two forms round by round
            for name, fn, _ in variants:
                times[name].append(_timed(fn, 20))
        t_valu = (n * 40 / 64) * valu * VALU_CYCLES / SIMDS / CLOCK_HZ
        row = dict(boards=n, valu_yardstick_us=round(t_valu * 1e6, 2))
        for name, _, nbytes in variants:
            t = sorted(times[name])[rounds // 2]
            t_mem = n * nbytes / HBM_ACHIEVABLE
            row[name] = dict(us=_spread(times[name]), bytes_per_board=nbytes, tb_per_s=round(n * nbytes / t / 1e12, 3),
                             of_streaming=round(t_mem / t, 3), of_valu_yardstick=round(t_valu / t, 3),
                             bound="memory" if t_mem >= t_valu else "valu-issue")
        rows.append(row)
        env.terminate()
        del sa, sb
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=20, rows=rows)
    loop = part_loop(lookahead=True)
    loop["part"] = "loop_lookahead"
    out["loop"] = loop
    return out


def _win_rates(L_, M_, pool, n, steps, tuned, seed):
    """Win rates over `steps` steps of n auto-reset boards from a full reset: uniform random, the reward weights (0, 1, 0: the
    best immediate win), `tuned`."""
    import torch
    import tetris_piclim as T
    env = T.BatchedTetris(L_, M_, n, device="cuda:0", seed=seed, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=pool)
    env.reset()
    reward_sum, finished = env.rollout_random(steps, seed=seed + 1)
    out = dict(boards=n, steps=steps, seed=seed)
    out["random"] = dict(episodes=int(finished.sum()), wins=int(round(float(reward_sum.sum()))))
    for name, w in (("reward_weights", [0.0, 1.0, 0.0] + [0.0] * 9), ("tuned", tuned)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = T.evaluate_heuristic(env, w, None, steps)
        out[name] = dict(episodes=int(got["episodes"][0]), wins=int(got["wins"][0]), seconds=round(time.perf_counter() - t0, 3))
    for name in ("random", "reward_weights", "tuned"):
        out[name]["win_rate"] = round(out[name]["wins"] / max(out[name]["episodes"], 1), 5)
    env.terminate()
    return out


def part_heuristic(rounds=5):
    import ctypes as C
    import numpy as np
    import torch
    import tetris_piclim as T
    L = T._learn_lib.lib()
    check = T._learn_lib.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    lib_path = T._learn_lib.build_library()
    valu = dict(act=_static_valu("placement_act_kernel", lib_path), features=_static_valu("placement_features_kernel", lib_path),
                afterstates=_static_valu("afterstates_kernel", lib_path))
    out = dict(part="heuristic", static_valu_per_wave=valu, valu_cycles=VALU_CYCLES, streaming_tb_per_s=HBM_ACHIEVABLE / 1e12)
    classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
    weights = torch.from_numpy(classical).to("cuda:0")
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        for t in range(6):                                       # mid-game boards
            env.step(env.synthetic_actions(t), observe=False)
        pa, pb = C.c_void_p(), C.c_void_p()
        T._lib.check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
        feats = torch.empty((n, 40, 12), dtype=torch.int16, device="cuda:0")
        canonical = torch.empty((n, 40), dtype=torch.uint8, device="cuda:0")
        action = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        score = torch.empty(n, dtype=torch.float32, device="cuda:0")

        def act(with_score):
            check(L.tpl_placement_act(pa.value, pb.value, n, 10, 40, weights.data_ptr(), n, action.data_ptr(),
                                      score.data_ptr() if with_score else None, stream))

        def features():
            check(L.tpl_placement_features(pa.value, pb.value, n, 10, 40, feats.data_ptr(), canonical.data_ptr(), stream))
        variants = [("act", lambda: act(False), 32 + 1, "act"), ("act_with_score", lambda: act(True), 32 + 5, "act"),
                    ("features", features, 32 + 40 * 25, "features")]
        times = {name: [] for name, _, _, _ in variants}
        for _ in range(rounds):                                  # alternate the forms round by round
            for name, fn, _, _ in variants:
                times[name].append(_timed(fn, 20))
        row = dict(boards=n)
        for name, _, nbytes, kernel in variants:
            t = sorted(times[name])[rounds // 2]
            t_mem = n * nbytes / HBM_ACHIEVABLE
            t_valu = (n * 40 / 64) * valu[kernel] * VALU_CYCLES / SIMDS / CLOCK_HZ
            row[name] = dict(us=_spread(times[name]), bytes_per_board=nbytes, of_streaming=round(t_mem / t, 4),
                             valu_yardstick_us=round(t_valu * 1e6, 2), of_valu_yardstick=round(t_valu / t, 3),
                             bound="memory" if t_mem >= t_valu else "valu-issue")
        if n == 1 << 18:                                         # against the best-immediate-reward path that was there before
            fused = T.HeuristicPolicy(env, [1.0, 0.0, 0.0] + [0.0] * 9)
            parent = T.LookaheadPolicy(env, image=None)
            assert torch.equal(fused.act(), parent.act())
            ts = dict(fused=[], lookahead_without_network=[])
            for _ in range(rounds):
                ts["fused"].append(_timed(lambda: fused.act(out=action), 20))
                ts["lookahead_without_network"].append(_timed(lambda: parent.act(out=action), 20))
            row["policy_act"] = {k: _spread(v) for k, v in ts.items()}
            row["policy_act"]["lookahead_chunks"] = -(-n // parent.chunk)
        if n == 1 << 20:                                         # the host-driven loop: one act() and one step() per iteration
            policy = T.HeuristicPolicy(env, classical)
            reward = torch.empty(n, dtype=torch.float32, device="cuda:0")
            done = torch.empty(n, dtype=torch.uint8, device="cuda:0")

            def both():
                env.step_into(policy.act(out=action), reward, done)
            ts = [_timed(both, 20) for _ in range(rounds)]
            step_only = [_timed(lambda: env.step_into(action, reward, done), 20) for _ in range(rounds)]
            row["act_and_step"] = dict(us=_spread(ts), env_steps_per_s=round(n / sorted(ts)[rounds // 2]),
                                       step_alone_us=_spread(step_only))
        rows.append(row)
        env.terminate()
        del feats
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=20, rows=rows)
    # win rates: the loop's L=2 / M=2 pool (yardsticks: random 0.027, greedy 0.94, lookahead 0.97) ...
    small = T.generate_configs(2, 2, 64, seed=100)
    t0 = time.perf_counter()
    tuned = T.tune_heuristic(2, 2, small, population=64, boards_per_member=4096, steps=8, generations=10, seed=0)
    budget = dict(population=64, boards_per_member=4096, steps=8, generations=10, seed=0, seconds=round(time.perf_counter() - t0, 2))
    out["l2_m2"] = dict(tune=dict(budget, best_fitness=round(tuned["best_fitness"], 5), best=[round(float(x), 4) for x in tuned["best"]],
                                  history=tuned["history"]), rates=_win_rates(2, 2, small, 1 << 18, 8, tuned["best"], seed=0))
    # ... and an L=10 / M=40 carved pool: one seed, >= 10^6 episodes per policy
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()
    t0 = time.perf_counter()
    tuned = T.tune_heuristic(10, 40, big, population=64, boards_per_member=4096, steps=160, generations=40, seed=0)
    budget = dict(population=64, boards_per_member=4096, steps=160, generations=40, seed=0, pool=1 << 16, pool_seed=7,
                  seconds=round(time.perf_counter() - t0, 2))
    out["l10_m40"] = dict(tune=dict(budget, best_fitness=round(tuned["best_fitness"], 5),
                                    best=[round(float(x), 4) for x in tuned["best"]], mean=[round(float(x), 4) for x in tuned["mean"]],
                                    history=tuned["history"]),
                          rates=_win_rates(10, 40, big, 1 << 18, 200, tuned["best"], seed=11))
    return out


def _loop_valu(kernel, lib_path):
    """(vector ALU instructions of the kernel, those of its outermost loop): the loop is the backward branch with the longest
    span in the code as built (tools/dump_isa.sh); an inner loop's body counts once."""
    import re
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "dump_isa.sh"), kernel, lib_path], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    code = []                                                    # (address, mnemonic, branch offset in dwords or None)
    for l in res.stdout.splitlines():
        m = re.match(r"\s+(\S+)\s+(.*?)//\s*([0-9A-Fa-f]+):", l)
        if m:
            off = int(m.group(2).split()[0]) if m.group(1).startswith("s_cbranch") or m.group(1) == "s_branch" else None
            code.append((int(m.group(3), 16), m.group(1), off))
    total = sum(1 for _, op, _ in code if op.startswith("v_"))
    span = (0, 0)
    for addr, op, off in code:
        if off is not None and off >= 32768:                     # a 16-bit offset in dwords from the next instruction: backward
            target = addr + 4 + 4 * (off - 65536)
            if addr - target > span[1] - span[0]:
                span = (target, addr)
    return total, sum(1 for addr, op, _ in code if op.startswith("v_") and span[0] <= addr <= span[1])


def _search_rates(L_, M_, pool, n, steps, rows, seed):
    """Episodes, wins, win rate and its standard error of each named weight row at depth 1 and at depth 2, `steps` steps of n
    auto-reset boards from a full reset."""
    import torch
    import tetris_piclim as T
    env = T.BatchedTetris(L_, M_, n, device="cuda:0", seed=seed, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=pool)
    out = dict(boards=n, steps=steps, seed=seed)
    for name, w in rows:
        for depth in (1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = T.evaluate_heuristic(env, w, None, steps, depth=depth)
            e, wins = int(got["episodes"][0]), int(got["wins"][0])
            p = wins / max(e, 1)
            out[f"{name}_depth{depth}"] = dict(episodes=e, wins=wins, win_rate=round(p, 5),
                                               standard_error=round((p * (1 - p) / max(e, 1)) ** 0.5, 6),
                                               seconds=round(time.perf_counter() - t0, 3))
    env.terminate()
    return out


def part_search(rounds=5):
    import ctypes as C
    import numpy as np
    import torch
    import tetris_piclim as T
    L = T._learn_lib.lib()
    check = T._learn_lib.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    lib_path = T._learn_lib.build_library()
    total, loop = _loop_valu("placement_search_kernel", lib_path)
    out = dict(part="search", static_valu=dict(kernel=total, second_ply_loop=loop, placement_act_kernel=_static_valu("placement_act_kernel", lib_path)),
               valu_cycles=VALU_CYCLES, streaming_tb_per_s=HBM_ACHIEVABLE / 1e12)
    classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
    weights = torch.from_numpy(classical).to("cuda:0")
    trips_of = np.array([17, 34, 34, 34, 17, 17, 9, 9])          # the distinct placements of each piece id
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        for t in range(6):                                       # mid-game boards
            env.step(env.synthetic_actions(t), observe=False)
        pa, pb = C.c_void_p(), C.c_void_p()
        T._lib.check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
        action = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        second = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        score = torch.empty(n, dtype=torch.float32, device="cuda:0")
        # the trips of every wave: a block is 8 boards on 5 waves, wave v holds threads 64 v .. 64 v + 63 = boards 64 v / 40 ..
        # (64 v + 63) / 40 of the block, and runs as long as its slowest board
        b = env.raw_planes()[1].cpu().numpy().view(np.uint32)
        running = ((b[:, 1] >> 28) & 3) == 0
        trips = np.where(running, trips_of[(b[:, 3] >> 3) & 7], 0).reshape(-1, 8)
        wave_trips = np.stack([trips[:, (64 * v) // 40:(64 * v + 63) // 40 + 1].max(axis=1) for v in range(5)], axis=1)
        valu_per_wave = (total - loop) + loop * float(wave_trips.mean())

        def search(full):
            check(L.tpl_placement_search(pa.value, pb.value, n, 10, 40, weights.data_ptr(), n, action.data_ptr(),
                                         second.data_ptr() if full else None, score.data_ptr() if full else None, stream))
        variants = [("search", lambda: search(False), 32 + 1), ("search_with_second_and_score", lambda: search(True), 32 + 6)]
        times = {name: [] for name, _, _ in variants}
        for _ in range(rounds):                                  # alternate the forms round by round
            for name, fn, _ in variants:
                times[name].append(_timed(fn, 20))
        t_valu = (n * 40 / 64) * valu_per_wave * VALU_CYCLES / SIMDS / CLOCK_HZ
        row = dict(boards=n, running=int(running.sum()), mean_trips_per_board=round(float(trips.mean()), 2),
                   mean_trips_per_wave=round(float(wave_trips.mean()), 2), valu_per_wave=round(valu_per_wave),
                   valu_yardstick_us=round(t_valu * 1e6, 1))
        for name, _, nbytes in variants:
            t = sorted(times[name])[rounds // 2]
            row[name] = dict(us=_spread(times[name]), bytes_per_board=nbytes, of_streaming=round(n * nbytes / HBM_ACHIEVABLE / t, 5),
                             of_valu_yardstick=round(t_valu / t, 3))
        if n == 1 << 18:                                         # against the composition of the one-ply pieces it replaces
            chunk = 16384
            fused = T.HeuristicPolicy(env, classical, depth=2)
            scratch = T.BatchedTetris(10, 40, 40 * chunk, device="cuda:0", seed=1)
            inner = T.HeuristicPolicy(scratch, classical)
            inner_action = torch.empty(40 * chunk, dtype=torch.uint8, device="cuda:0")
            inner_score = torch.empty(40 * chunk, dtype=torch.float32, device="cuda:0")
            reward = torch.empty((chunk, 40), dtype=torch.float32, device="cuda:0")
            done, cleared, canonical = (torch.empty((chunk, 40), dtype=torch.uint8, device="cuda:0") for _ in range(3))
            ids = torch.arange(40, dtype=torch.int64, device="cuda:0")
            sa, sb = T.lookahead._state_ptrs(scratch)

            def composed():
                for first in range(0, n, chunk):
                    T.lookahead._enumerate(env, pa.value + 16 * first, pb.value + 16 * first, chunk, sa, sb, reward, done, cleared,
                                           canonical)
                    inner.act(out=inner_action, score=inner_score)
                    v = torch.where(canonical == ids, inner_score.view(chunk, 40), float("-inf"))
                    action[first:first + chunk] = v.max(dim=1).indices.to(torch.uint8)
            ts = dict(fused=[], composed=[])
            for _ in range(rounds):
                ts["fused"].append(_timed(lambda: fused.act(out=action), 20))
                ts["composed"].append(_timed(composed, 20))
            med = {k: sorted(v)[rounds // 2] for k, v in ts.items()}
            row["policy_act"] = dict(fused_us=_spread(ts["fused"]), composed_us=_spread(ts["composed"]), chunks=n // chunk,
                                     composed_over_fused=round(med["composed"] / med["fused"], 3))
            scratch.terminate()
        rows.append(row)
        env.terminate()
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=20, rows=rows)
    # win rates at depth 1 and 2: the classical signs and a row tuned at depth 2, >= 10^6 episodes per figure
    small = T.generate_configs(2, 2, 64, seed=100)
    t0 = time.perf_counter()
    tuned = T.tune_heuristic(2, 2, small, population=64, boards_per_member=4096, steps=8, generations=10, seed=0, depth=2)
    budget = dict(population=64, boards_per_member=4096, steps=8, generations=10, seed=0, depth=2, seconds=round(time.perf_counter() - t0, 2))
    out["l2_m2"] = dict(tune=dict(budget, best_fitness=round(tuned["best_fitness"], 5), best=[round(float(x), 4) for x in tuned["best"]]),
                        rates=_search_rates(2, 2, small, 1 << 18, 8, (("classical", classical), ("tuned", tuned["best"])), seed=0))
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()
    t0 = time.perf_counter()
    tuned = T.tune_heuristic(10, 40, big, population=32, boards_per_member=2048, steps=80, generations=10, seed=0, depth=2)
    budget = dict(population=32, boards_per_member=2048, steps=80, generations=10, seed=0, depth=2, pool=1 << 16, pool_seed=7,
                  seconds=round(time.perf_counter() - t0, 2))
    out["l10_m40"] = dict(tune=dict(budget, best_fitness=round(tuned["best_fitness"], 5), best=[round(float(x), 4) for x in tuned["best"]]),
                          rates=_search_rates(10, 40, big, 1 << 18, 160, (("classical", classical), ("tuned", tuned["best"])), seed=11))
    return out


BEAM_SHAPES = ((2, 34), (3, 8), (4, 16), (6, 16), (12, 64))


def _beam_model(a, b, depth, width, known=12):
    """Moves per board the two rules make on the states (a, b) (uint32 [n, 4] planes), by the known pieces of every window and
    the distinct placements of each: (beam at (depth, width), two-ply search), means over all boards (a finished board: 0).
    known: the plies a fresh window allows -- 12 for the placement beam, 11 for the n-tuple beam, whose leaf reads one piece more."""
    import numpy as np
    count = np.array([17, 34, 34, 34, 17, 17, 9, 9], np.int64)
    running = ((b[:, 1] >> 28) & 3) == 0
    moves = ((a[:, 1] >> 28) | ((a[:, 3] >> 28) << 4)).astype(np.int64)
    window = b[:, 3].astype(np.uint64) | ((b[:, 2] >> 28).astype(np.uint64) << np.uint64(32))
    plies = np.where(running, np.minimum(depth, known - moves % 10), 0)
    nodes, total = np.ones(a.shape[0], np.int64), np.zeros(a.shape[0], np.int64)
    for j in range(depth):
        c = count[((window >> np.uint64(3 * j)) & np.uint64(7)).astype(np.int64)]
        live = plies > j
        total += np.where(live, nodes * c, 0)
        nodes = np.where(live, np.minimum(width, nodes * c), nodes)
    c0, c1 = count[(window & np.uint64(7)).astype(np.int64)], count[((window >> np.uint64(3)) & np.uint64(7)).astype(np.int64)]
    return float(total.mean()), float(np.where(running, c0 * (1 + c1), 0).mean()), float(plies.mean())


def part_beam(rounds=3):
    import numpy as np
    import torch
    import tetris_piclim as T
    classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
    out = dict(part="beam", model="34 (1 + W (D - 1)) moves per board against the two-ply search's 34^2",
               nominal_ratio={f"{d}x{w}": round(34 * (1 + w * (d - 1)) / 34 ** 2, 3) for d, w in BEAM_SHAPES})
    rows = []
    for n in (1 << 16, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        for t in range(6):                                       # mid-game boards
            env.step(env.synthetic_actions(t), observe=False)
        a, b = (x.cpu().numpy().view(np.uint32) for x in env.raw_planes())
        action = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        two = T.HeuristicPolicy(env, classical, depth=2)
        beams = {shape: T.BeamPolicy(env, classical, *shape) for shape in BEAM_SHAPES}
        reps = 10 if n <= 1 << 16 else 3
        times = {shape: [] for shape in BEAM_SHAPES}
        times["search"] = []
        for _ in range(rounds):                                  # alternate the kernels round by round
            times["search"].append(_timed(lambda: two.act(out=action), reps, warmup=1))
            for shape in BEAM_SHAPES:
                times[shape].append(_timed(lambda: beams[shape].act(out=action), reps, warmup=1))
        t_search = sorted(times["search"])[rounds // 2]
        row = dict(boards=n, launches_per_timing=reps, rounds=rounds, search_us=_spread(times["search"]))
        for shape in BEAM_SHAPES:
            t = sorted(times[shape])[rounds // 2]
            beam_moves, search_moves, plies = _beam_model(a, b, *shape)
            row[f"{shape[0]}x{shape[1]}"] = dict(us=_spread(times[shape]), mean_plies=round(plies, 2), moves_per_board=round(beam_moves, 1),
                                                 search_moves_per_board=round(search_moves, 1), measured_over_search=round(t / t_search, 3),
                                                 predicted_over_search=round(beam_moves / search_moves, 3),
                                                 measured_over_predicted=round(t / t_search / (beam_moves / search_moves), 3))
        rows.append(row)
        env.terminate()
        torch.cuda.empty_cache()
    out["act"] = rows
    # play strength: the classical signs on an L = 10 / M = 40 carved pool
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()
    n, steps, seed = 1 << 16, 160, 11
    env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=seed, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=big)
    rates = dict(boards=n, steps=steps, seed=seed, pool=1 << 16, pool_seed=7)
    for depth, width in ((1, None), (2, None), (3, 8), (4, 16), (6, 16)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = T.evaluate_heuristic(env, classical, None, steps, depth=depth, width=width)
        e, wins = int(got["episodes"][0]), int(got["wins"][0])
        p = wins / max(e, 1)
        rates[f"depth{depth}" + (f"_width{width}" if width else "")] = dict(
            episodes=e, wins=wins, win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(e, 1)) ** 0.5, 6),
            seconds=round(time.perf_counter() - t0, 3))
    env.terminate()
    out["l10_m40"] = rates
    return out


NTUPLE_SMALL = dict(gamma=1.0, rate=8.0, epsilon=0.25)      # the two-piece game: tests/test_ntuple_gpu.py says why
# L=10 / M=40: a win-only reward never pays before the first win, which exploration does not find (the zero table wins 0 of
# 324,756 episodes and every TD error is 0), so the learner is trained on a shaped reward (r_line, r_win, r_lose) and judged on wins
NTUPLE_LARGE_REWARD = (1.0, 10.0, -1.0)
NTUPLE_LARGE = [dict(gamma=1.0, rate=rate, epsilon=0.05) for rate in (1.0, 4.0, 16.0)]


def part_ntuple(rounds=5):
    import ctypes as C
    import numpy as np
    import torch
    import tetris_piclim as T
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import learn_ref as R
    m = T._learn_lib
    L, check = m.lib(), m.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    lib_path = m.build_library()
    valu = {k: _static_valu(k, lib_path) for k in ("ntuple_act_kernel", "ntuple_value_kernel", "ntuple_trace_kernelILb0")}
    out = dict(part="ntuple", static_valu=valu, scattered_atomics_tb_per_s=SCATTERED_ATOMICS / 1e12)
    classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
    weights = torch.from_numpy(classical).to("cuda:0")
    host = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_ENTRIES).astype(np.int32)
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        for t in range(6):                                       # mid-game boards
            env.step(env.synthetic_actions(t), observe=False)
        pa, pb = C.c_void_p(), C.c_void_p()
        T._lib.check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
        a, b = (x[:4096].cpu().numpy().view(np.uint32) for x in env.raw_planes())
        f = R.decode_state(a, b)
        _, used = m.ntuple_indices(f["rows"], f["cur"], 10, 40, f["lines"].astype(np.int64), f["moves"].astype(np.int64))
        in_use = float(used[f["state"] == 0].sum(axis=1).mean())   # entries per running board, the counter included
        table = torch.from_numpy(host).to("cuda:0")
        action = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        score, value, error = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(3))
        error.normal_()
        after = [torch.empty((n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2)]

        def act(full):
            check(L.tpl_ntuple_act(pa.value, pb.value, n, 10, 40, 0.0, 1.0, 0.0, 0.99, table.data_ptr(), 0.0, 0, 0, action.data_ptr(),
                                   score.data_ptr() if full else None, after[0].data_ptr() if full else None,
                                   after[1].data_ptr() if full else None, value.data_ptr() if full else None, stream))
        variants = [
            ("ntuple_act", lambda: act(False)), ("ntuple_act_all_outputs", lambda: act(True)),
            ("placement_act", lambda: check(L.tpl_placement_act(pa.value, pb.value, n, 10, 40, weights.data_ptr(), n, action.data_ptr(),
                                                                None, stream))),
            ("placement_search", lambda: check(L.tpl_placement_search(pa.value, pb.value, n, 10, 40, weights.data_ptr(), n,
                                                                      action.data_ptr(), None, None, stream))),
            ("ntuple_value", lambda: check(L.tpl_ntuple_value(pa.value, pb.value, n, 10, 40, table.data_ptr(), value.data_ptr(), stream))),
            ("ntuple_update", lambda: check(L.tpl_ntuple_update(pa.value, pb.value, n, 10, 40, table.data_ptr(), error.data_ptr(),
                                                                100.0, stream))),
        ]
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                                  # alternate the kernels round by round
            for name, fn in variants:
                times[name].append(_timed(fn, 20))
        med = {name: sorted(ts)[rounds // 2] for name, ts in times.items()}
        row = dict(boards=n, entries_in_use_per_board=round(in_use, 1), us={name: _spread(ts) for name, ts in times.items()},
                   act_over_one_ply=round(med["ntuple_act"] / med["placement_act"], 2),
                   act_over_two_ply=round(med["ntuple_act"] / med["placement_search"], 3))
        for name in ("ntuple_value", "ntuple_update"):
            nbytes = n * in_use * 4
            row[name] = dict(bytes=round(nbytes), tb_per_s=round(nbytes / med[name] / 1e12, 3),
                             over_scattered_atomics=round(nbytes / med[name] / SCATTERED_ATOMICS, 2))
        rows.append(row)
        env.terminate()
        del table, after
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=20, rows=rows)

    def learn(L_, M_, pool, n, seed, train_steps, eval_steps, reward=(0.0, 1.0, 0.0), **kw):
        env = T.BatchedTetris(L_, M_, n, device="cuda:0", seed=seed, auto_reset=True, reward=reward, config_pool=pool)
        learner = T.NTupleLearner(env, seed=seed, **kw)
        got = dict(kw, boards=n, seed=seed, reward=list(reward), zero_table=learner.evaluate(eval_steps), trained=[])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for steps in train_steps:
            learner.train(steps)
            r = learner.evaluate(eval_steps)
            p = r["win_rate"]
            got["trained"].append(dict(r, steps=learner.steps, standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6),
                                       seconds=round(time.perf_counter() - t0, 2)))
        got["entries_in_use"] = int((learner.table != 0).sum())
        got["largest_entry"] = int(learner.table.abs().max())
        env.terminate()
        return got
    out["l2_m2"] = learn(2, 2, T.generate_configs(2, 2, 64, seed=107), 4096, 3, (100, 200), 64, **NTUPLE_SMALL)
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()
    env = T.BatchedTetris(10, 40, 1 << 16, device="cuda:0", seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=big)
    got = T.evaluate_heuristic(env, classical, None, 640)
    env.terminate()
    out["l10_m40"] = dict(pool=1 << 16, pool_seed=7,
                          classical_one_ply=dict(episodes=int(got["episodes"][0]), wins=int(got["wins"][0]),
                                                 win_rate=round(float(got["win_rate"][0]), 5)),
                          win_only_reward=learn(10, 40, big, 1 << 14, 11, (1500,), 160, gamma=1.0, rate=8.0, epsilon=0.05),
                          shaped_reward=[learn(10, 40, big, 4096, 11, (10000, 30000), 12288, reward=NTUPLE_LARGE_REWARD, **kw)
                                         for kw in NTUPLE_LARGE])
    return out


def _nested_loop_valu(kernel, lib_path):
    """(vector ALU instructions of the kernel, of its outermost loop, of the gather loop inside that one): loops are backward
    branches in the code as built (tools/dump_isa.sh), the outermost the one with the longest span, the gather loop the one inside
    it with the most global loads (a backward branch to the outer loop's own head is a trip that ends early, not a loop)."""
    import re
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "dump_isa.sh"), kernel, lib_path], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    code = []
    for l in res.stdout.splitlines():
        m = re.match(r"\s+(\S+)\s+(.*?)//\s*([0-9A-Fa-f]+):", l)
        if m:
            off = int(m.group(2).split()[0]) if m.group(1).startswith("s_cbranch") or m.group(1) == "s_branch" else None
            code.append((int(m.group(3), 16), m.group(1), off))
    spans = sorted(((addr + 4 + 4 * (off - 65536), addr) for addr, _, off in code if off is not None and off >= 32768),
                   key=lambda s: s[0] - s[1])                    # the longest first
    count = lambda span, prefix: sum(1 for addr, op, _ in code if op.startswith(prefix) and span[0] <= addr <= span[1])
    outer = spans[0]
    inside = [s for s in spans[1:] if outer[0] < s[0] and s[1] <= outer[1]]
    gather = max(inside, key=lambda s: count(s, "global_load"))
    return count((0, 1 << 62), "v_"), count(outer, "v_"), count(gather, "v_")


def part_ntuple_search(rounds=5):
    import ctypes as C
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    L, check = m.lib(), m.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    lib_path = m.build_library()
    total, loop, gather = _nested_loop_valu("ntuple_search_kernel", lib_path)
    act_total, act_gather = _loop_valu("ntuple_act_kernel", lib_path)
    trip = (loop - gather) + 17 * gather                         # one second placement: the move, the pop, the score and 17 gather trips
    out = dict(part="ntuple_search", valu_cycles=VALU_CYCLES,
               static_valu=dict(kernel=total, second_ply_loop=loop, gather_loop=gather, per_second_placement=trip,
                                ntuple_act_kernel=act_total, ntuple_act_gather_loop=act_gather,
                                ntuple_act_outside_its_loop=act_total - act_gather))
    classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
    weights = torch.from_numpy(classical).to("cuda:0")
    host = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_ENTRIES).astype(np.int32)
    trips_of = np.array([17, 34, 34, 34, 17, 17, 9, 9])          # the distinct placements of each piece id
    gamma = 0.99
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        for t in range(6):                                       # mid-game boards
            env.step(env.synthetic_actions(t), observe=False)
        pa, pb = C.c_void_p(), C.c_void_p()
        T._lib.check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
        table = torch.from_numpy(host).to("cuda:0")
        action, second = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        score, value = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
        after = [torch.empty((n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2)]
        # the trips of every wave, as part_search counts them: a wave runs as long as its slowest board
        b = env.raw_planes()[1].cpu().numpy().view(np.uint32)
        running = ((b[:, 1] >> 28) & 3) == 0
        trips = np.where(running, trips_of[(b[:, 3] >> 3) & 7], 0).reshape(-1, 8)
        wave_trips = np.stack([trips[:, (64 * v) // 40:(64 * v + 63) // 40 + 1].max(axis=1) for v in range(5)], axis=1)
        valu_per_wave = (act_total - act_gather) + trip * float(wave_trips.mean())
        t_valu = (n * 40 / 64) * valu_per_wave * VALU_CYCLES / SIMDS / CLOCK_HZ

        def search(full):
            check(L.tpl_ntuple_search(pa.value, pb.value, n, 10, 40, 0.0, 1.0, 0.0, gamma, table.data_ptr(), 0.0, 0, 0,
                                      action.data_ptr(), second.data_ptr() if full else None, score.data_ptr() if full else None,
                                      after[0].data_ptr() if full else None, after[1].data_ptr() if full else None,
                                      value.data_ptr() if full else None, stream))
        variants = [
            ("ntuple_search", lambda: search(False)), ("ntuple_search_all_outputs", lambda: search(True)),
            ("ntuple_act", lambda: check(L.tpl_ntuple_act(pa.value, pb.value, n, 10, 40, 0.0, 1.0, 0.0, gamma, table.data_ptr(), 0.0, 0,
                                                          0, action.data_ptr(), None, None, None, None, stream))),
            ("placement_search", lambda: check(L.tpl_placement_search(pa.value, pb.value, n, 10, 40, weights.data_ptr(), n,
                                                                      action.data_ptr(), None, None, stream))),
        ]
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                                  # alternate the kernels round by round
            for name, fn in variants:
                times[name].append(_timed(fn, 20))
        med = {name: sorted(ts)[rounds // 2] for name, ts in times.items()}
        row = dict(boards=n, running=int(running.sum()), mean_trips_per_board=round(float(trips.mean()), 2),
                   mean_trips_per_wave=round(float(wave_trips.mean()), 2), valu_per_wave=round(valu_per_wave),
                   price_us=round(t_valu * 1e6, 1), us={name: _spread(ts) for name, ts in times.items()},
                   price_over_measured=round(t_valu / med["ntuple_search"], 3),
                   search_over_act=round(med["ntuple_search"] / med["ntuple_act"], 2),
                   search_over_two_ply_heuristic=round(med["ntuple_search"] / med["placement_search"], 2))
        if n == 1 << 18:                                         # against the composition of the one-ply pieces it replaces
            chunk = 16384
            fused = T.NTuplePolicy(env, table, gamma=gamma, depth=2)
            scratch = T.BatchedTetris(10, 40, 40 * chunk, device="cuda:0", seed=1)
            inner = T.NTuplePolicy(scratch, table, gamma=gamma)
            inner_action = torch.empty(40 * chunk, dtype=torch.uint8, device="cuda:0")
            inner_score = torch.empty(40 * chunk, dtype=torch.float32, device="cuda:0")
            reward = torch.empty((chunk, 40), dtype=torch.float32, device="cuda:0")
            done, cleared, canonical = (torch.empty((chunk, 40), dtype=torch.uint8, device="cuda:0") for _ in range(3))
            ids = torch.arange(40, dtype=torch.int64, device="cuda:0")
            sa, sb = T.lookahead._state_ptrs(scratch)

            def composed():
                for first in range(0, n, chunk):
                    T.lookahead._enumerate(env, pa.value + 16 * first, pb.value + 16 * first, chunk, sa, sb, reward, done, cleared,
                                           canonical)
                    inner.act(out=inner_action, score=inner_score, step=0)
                    q = torch.where(done != 0, reward, reward + gamma * inner_score.view(chunk, 40))
                    q = torch.where(canonical == ids, q, float("-inf"))
                    action[first:first + chunk] = q.max(dim=1).indices.to(torch.uint8)
            fused_action = fused.act(step=0).clone()
            composed()
            torch.cuda.synchronize()
            ts = dict(fused=[], composed=[])
            for _ in range(rounds):
                ts["fused"].append(_timed(lambda: fused.act(out=second, step=0), 20))
                ts["composed"].append(_timed(composed, 20))
            medp = {k: sorted(v)[rounds // 2] for k, v in ts.items()}
            # torch's max takes a first index among equal maxima too; its product is rounded as the kernel's is
            row["policy_act"] = dict(fused_us=_spread(ts["fused"]), composed_us=_spread(ts["composed"]), chunks=n // chunk,
                                     composed_over_fused=round(medp["composed"] / medp["fused"], 3),
                                     boards_where_the_actions_differ=int((fused_action != action).sum()))
            scratch.terminate()
        rows.append(row)
        env.terminate()
        del table, after
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=20, gamma=gamma, rows=rows)

    # play strength on the L=10 / M=40 carved pool of part_ntuple: one table trained at each depth, each played at both
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()

    def rate(r):
        p = r["win_rate"]
        return dict(r, win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))

    kw = NTUPLE_LARGE[-1]
    trained = []
    for depth in (1, 2):
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        learner = T.NTupleLearner(env, seed=11, depth=depth, **kw)
        # part_ntuple's sequence, so that the table trained at depth 1 is the one its log records: the zero table played (the
        # full reset that training starts from), 10,000 steps, an evaluation, 30,000 steps
        zero = rate(learner.evaluate(12288))
        train_seconds = 0.0
        for steps in (10000, 30000):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            learner.train(steps)
            torch.cuda.synchronize()
            train_seconds += time.perf_counter() - t0
            if learner.steps == 10000:
                early = rate(learner.evaluate(12288))
        got = dict(kw, trained_at_depth=depth, boards=4096, seed=11, reward=list(NTUPLE_LARGE_REWARD), steps=learner.steps,
                   train_seconds=round(train_seconds, 2), zero_table_at_its_depth=zero, after_10000_steps_at_its_depth=early)
        for play in (1, 2):
            t0 = time.perf_counter()
            got[f"played_at_depth{play}"] = dict(rate(learner.evaluate(12288, depth=play)), seconds=round(time.perf_counter() - t0, 2))
        got["entries_in_use"] = int((learner.table != 0).sum())
        got["largest_entry"] = int(learner.table.abs().max())
        trained.append(got)
        env.terminate()
    env = T.BatchedTetris(10, 40, 1 << 16, device="cuda:0", seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=big)
    heuristic = {}
    for depth in (1, 2):
        got = T.evaluate_heuristic(env, classical, None, 640, depth=depth)
        e, wins = int(got["episodes"][0]), int(got["wins"][0])
        heuristic[f"classical_depth{depth}"] = rate(dict(episodes=e, wins=wins, win_rate=wins / max(e, 1)))
    env.terminate()
    out["l10_m40"] = dict(pool=1 << 16, pool_seed=7, eval_steps=12288, tables=trained, **heuristic)
    return out


def part_ntuple_trace(rounds=5, reps=10):
    import numpy as np
    import torch
    import tetris_piclim as T
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import learn_ref as R
    m = T._learn_lib
    L, check = m.lib(), m.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    slots, head, rate, decay = 17, 16, 100.0, 0.9
    out = dict(part="ntuple_trace", slots=slots, head=head, rate=rate, decay=decay,
               static_valu={k: _static_valu(k, m.build_library()) for k in ("ntuple_trace_kernelILb0", "ntuple_trace_kernelILb1")})
    host = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_ENTRIES).astype(np.int32)
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        ring = [torch.empty((slots, n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2)]
        for t in range(6 + slots):                               # mid-game boards: the last 17 states of every board, oldest first
            env.step(env.synthetic_actions(t), observe=False)
            if t >= 6:
                a, b = env.raw_planes()
                ring[0][t - 6].copy_(a)
                ring[1][t - 6].copy_(b)
        a, b = (x[head, :4096].cpu().numpy().view(np.uint32) for x in ring)
        f = R.decode_state(a, b)
        _, used = m.ntuple_indices(f["rows"], f["cur"], 10, 40, f["lines"].astype(np.int64), f["moves"].astype(np.int64))
        in_use = float(used[f["state"] == 0].sum(axis=1).mean())   # entries per running board of the newest slot, the counter included
        table = torch.from_numpy(host).to("cuda:0")
        error = torch.empty(n, dtype=torch.float32, device="cuda:0").normal_()
        # the (board, age) pairs that add: every state up to that age runs and rint(rate * decay^k * e) is not 0
        running = ((ring[1][:, :, 1] >> 28) & 3) == 0
        open_ = torch.cumprod(running.flip(0).to(torch.int32), dim=0).bool()         # [age, n]: slot head - age
        w = torch.tensor([decay], dtype=torch.float32, device="cuda:0") ** torch.arange(slots, device="cuda:0", dtype=torch.float32)
        adds = open_ & (torch.round(rate * w[:, None] * error[None, :]) != 0)
        pairs = {h: float(adds[:h].sum()) / n for h in (1, 4, 8, 16)}
        pa, pb = ring[0].data_ptr(), ring[1].data_ptr()

        def trace(horizon, symmetric):
            check(L.tpl_ntuple_update_trace(pa, pb, n, slots, head, horizon, 10, 40, table.data_ptr(), error.data_ptr(), rate, decay,
                                            symmetric, stream))
        variants = [("update", lambda: check(L.tpl_ntuple_update(ring[0][head].data_ptr(), ring[1][head].data_ptr(), n, 10, 40,
                                                                 table.data_ptr(), error.data_ptr(), rate, stream)))]
        variants += [(f"h{h}_s{sym}", (lambda h=h, sym=sym: trace(h, sym))) for h in (1, 4, 8, 16) for sym in (0, 1)]
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                                  # alternate the variants round by round
            for name, fn in variants:
                times[name].append(_timed(fn, reps))
        med = {name: sorted(ts)[rounds // 2] for name, ts in times.items()}
        row = dict(boards=n, entries_in_use_per_board=round(in_use, 1), running_share_of_the_newest_slot=round(float(running[head].float().mean()), 4),
                   adding_pairs_per_board={f"h{h}": round(p, 3) for h, p in pairs.items()},
                   update=dict(us=_spread(times["update"]), tb_per_s=round(n * pairs[1] * in_use * 4 / med["update"] / 1e12, 3)))
        for h in (1, 4, 8, 16):
            for sym in (0, 1):
                name = f"h{h}_s{sym}"
                predicted = med["update"] * pairs[h] / pairs[1] * (2 if sym else 1)
                nbytes = n * pairs[h] * (in_use * (2 if sym else 1) - (1 if sym else 0)) * 4       # the counter: once
                row[name] = dict(us=_spread(times[name]), over_update=round(med[name] / med["update"], 2),
                                 predicted_over_update=round(predicted / med["update"], 2),
                                 measured_over_predicted=round(med[name] / predicted, 3),
                                 tb_per_s=round(nbytes / med[name] / 1e12, 3))
        rows.append(row)
        env.terminate()
        del table, ring, running, open_, adds
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=reps, rows=rows)
    return out


def part_ntuple_trace_sweep(eval_steps=12288):
    import torch
    import tetris_piclim as T
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()

    def learn(**kw):
        """part_ntuple's sequence: the zero table played, 10,000 steps, an evaluation, 30,000 steps, an evaluation."""
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, **kw)
        learner.evaluate(eval_steps)
        got = dict(kw, trained=[])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for steps in (10000, 30000):
            learner.train(steps)
            r = learner.evaluate(eval_steps)
            p = r["win_rate"]
            got["trained"].append(dict(steps=learner.steps, episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5),
                                       standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6)))
        got.update(seconds=round(time.perf_counter() - t0, 2), entries_in_use=int((learner.table != 0).sum()),
                   largest_entry=int(learner.table.abs().max()), symmetric_table=T.ntuple_is_symmetric(learner.table))
        env.terminate()
        print(json.dumps(got), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        return got
    runs = [learn(rate=16.0)]
    runs += [learn(rate=rate, symmetric=True) for rate in (4.0, 8.0, 16.0)]
    runs += [learn(rate=rate, lam=lam, horizon=horizon, symmetric=symmetric) for lam in (0.5, 0.8, 0.9) for horizon in (4, 8)
             for symmetric in (False, True) for rate in (4.0, 8.0, 16.0)]
    best = max(runs, key=lambda r: r["trained"][-1]["win_rate"])
    return dict(part="ntuple_trace_sweep", boards=4096, seed=11, pool=1 << 16, pool_seed=7, reward=list(NTUPLE_LARGE_REWARD), gamma=1.0,
                epsilon=0.05, eval_steps=eval_steps, baseline=runs[0], best=best, runs=runs)


def _kernel_us(fn, names, calls=5):
    """The device time per call, in µs, of each kernel whose name holds one of `names`, from torch.profiler's kernel records over
    `calls` calls of fn; a string that says why where there are none."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        got = {}
        for name in names:
            ts = [e.device_time for e in prof.events() if name in e.name and e.device_time > 0]
            got[name] = round(sum(ts) / calls, 2) if ts else "no kernel records"
        return got
    except Exception as exc:                                     # the profiler is a measuring aid; the timings above stand without it
        return {name: f"profiler failed: {exc!r}"[:120] for name in names}


def part_ntuple_coherent(rounds=5, reps=10):
    import numpy as np
    import torch
    import tetris_piclim as T
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import learn_ref as R
    m = T._learn_lib
    L, check = m.lib(), m.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    slots, head, rate, decay = 17, 16, 100.0, 0.9
    kernels = ("ntuple_coherent_step_kernel", "ntuple_coherent_accumulate_kernel")
    out = dict(part="ntuple_coherent", slots=slots, head=head, rate=rate, decay=decay,
               static_valu={k: _static_valu(k, m.build_library()) for k in ("ntuple_trace_kernelILb0", "ntuple_trace_kernelILb1",
                            "coherent_step_kernelILb0", "coherent_step_kernelILb1", "coherent_accumulate_kernelILb0",
                            "coherent_accumulate_kernelILb1")})
    host = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_ENTRIES).astype(np.int32)
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
        env.load_configs(*env.synthetic_configs(4096))
        env.reset()
        ring = [torch.empty((slots, n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2)]
        for t in range(6 + slots):                               # part ntuple_trace's ring: the last 17 states of every board
            env.step(env.synthetic_actions(t), observe=False)
            if t >= 6:
                a, b = env.raw_planes()
                ring[0][t - 6].copy_(a)
                ring[1][t - 6].copy_(b)
        a, b = (x[head, :4096].cpu().numpy().view(np.uint32) for x in ring)
        f = R.decode_state(a, b)
        _, used = m.ntuple_indices(f["rows"], f["cur"], 10, 40, f["lines"].astype(np.int64), f["moves"].astype(np.int64))
        in_use = float(used[f["state"] == 0].sum(axis=1).mean())
        table = torch.from_numpy(host).to("cuda:0")
        coherence = T.ntuple_coherence("cuda:0")
        error = torch.empty(n, dtype=torch.float32, device="cuda:0").normal_()
        running = ((ring[1][:, :, 1] >> 28) & 3) == 0
        open_ = torch.cumprod(running.flip(0).to(torch.int32), dim=0).bool()
        w = torch.tensor([decay], dtype=torch.float32, device="cuda:0") ** torch.arange(slots, device="cuda:0", dtype=torch.float32)
        adds = open_ & (torch.round(rate * w[:, None] * error[None, :]) != 0)
        pairs = {h: float(adds[:h].sum()) / n for h in (1, 4)}
        pa, pb = ring[0].data_ptr(), ring[1].data_ptr()

        def trace(horizon, symmetric, e=error):
            check(L.tpl_ntuple_update_trace(pa, pb, n, slots, head, horizon, 10, 40, table.data_ptr(), e.data_ptr(), rate, decay,
                                            symmetric, stream))

        def coherent(horizon, symmetric, e=error, c=coherence):
            check(L.tpl_ntuple_update_coherent(pa, pb, n, slots, head, horizon, 10, 40, table.data_ptr(), c.data_ptr(),
                                               e.data_ptr(), rate, decay, symmetric, stream))
        one_sign, full = error.abs(), T.ntuple_coherence("cuda:0")   # E = A at every entry: alpha stays 1, no step rounds to 0
        for _ in range(3):                                       # step sizes of every kind before anything is timed
            coherent(4, 1, torch.empty_like(error).normal_())
        alpha = T.ntuple_step_sizes(coherence)[coherence[:, 1] > 0]
        steps = torch.round(rate * alpha.mean() * error)        # a rough share of the steps that round to 0 at the mean step size
        variants = [("update", lambda: check(L.tpl_ntuple_update(ring[0][head].data_ptr(), ring[1][head].data_ptr(), n, 10, 40,
                                                                 table.data_ptr(), error.data_ptr(), rate, stream)))]
        for h in (1, 4):
            for sym in (0, 1):
                variants.append((f"trace_h{h}_s{sym}", (lambda h=h, sym=sym: trace(h, sym))))
                variants.append((f"coherent_h{h}_s{sym}", (lambda h=h, sym=sym: coherent(h, sym))))
                variants.append((f"alpha1_h{h}_s{sym}", (lambda h=h, sym=sym: coherent(h, sym, one_sign, full))))
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                                  # alternate the variants round by round
            for name, fn in variants:
                times[name].append(_timed(fn, reps))
        med = {name: sorted(ts)[rounds // 2] for name, ts in times.items()}
        row = dict(boards=n, entries_in_use_per_board=round(in_use, 1), adding_pairs_per_board={f"h{h}": round(p, 3) for h, p in pairs.items()},
                   alpha_before_timing=dict(entries=int(alpha.numel()), mean=round(float(alpha.mean()), 3),
                                            below_half=round(float((alpha < 0.5).float().mean()), 3),
                                            steps_0_at_the_mean=round(float((steps == 0).float().mean()), 3)),
                   update=dict(us=_spread(times["update"])))
        for h in (1, 4):
            for sym in (0, 1):
                entries = n * pairs[h] * (in_use * (2 if sym else 1) - (1 if sym else 0))          # entry adds a call; the counter: once
                t, c = med[f"trace_h{h}_s{sym}"], med[f"coherent_h{h}_s{sym}"]
                phases = _kernel_us(lambda h=h, sym=sym: coherent(h, sym), kernels)
                cell = dict(trace_us=_spread(times[f"trace_h{h}_s{sym}"]), coherent_us=_spread(times[f"coherent_h{h}_s{sym}"]),
                            coherent_over_trace=round(c / t, 2), coherent_over_update=round(c / med["update"], 2),
                            trace_tb_per_s=round(entries * 4 / t / 1e12, 3), phases_us=phases)
                step, acc = phases[kernels[0]], phases[kernels[1]]
                if isinstance(step, float) and isinstance(acc, float):
                    cell.update(step_over_trace=round(step * 1e-6 / t, 2), accumulate_over_trace=round(acc * 1e-6 / t, 2),
                                step_added_tb_per_s=round(entries * 4 / (step * 1e-6) / 1e12, 3),
                                step_gathered_tb_per_s=round(entries * 16 / (step * 1e-6) / 1e12, 3),
                                accumulate_added_tb_per_s=round(entries * 16 / (acc * 1e-6) / 1e12, 3),
                                accumulate_atomics_per_s=round(entries * 2 / (acc * 1e-6) / 1e9, 2))
                a1 = med[f"alpha1_h{h}_s{sym}"]
                p1 = _kernel_us(lambda h=h, sym=sym: coherent(h, sym, one_sign, full), kernels)
                cell["every_step_size_1"] = dict(coherent_us=_spread(times[f"alpha1_h{h}_s{sym}"]), coherent_over_trace=round(a1 / t, 2),
                                                 coherent_over_update=round(a1 / med["update"], 2), phases_us=p1)
                if isinstance(p1[kernels[0]], float):
                    cell["every_step_size_1"].update(step_over_trace=round(p1[kernels[0]] * 1e-6 / t, 2),
                                                     step_added_tb_per_s=round(entries * 4 / (p1[kernels[0]] * 1e-6) / 1e12, 3))
                row[f"h{h}_s{sym}"] = cell
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        env.terminate()
        del table, coherence, full, ring, running, open_, adds
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=reps, rows=rows)
    return out


def _alpha_summary(T, coherence):
    import torch
    alpha = T.ntuple_step_sizes(coherence)[coherence[:, 1] > 0]
    if alpha.numel() == 0:
        return dict(entries=0)
    q = torch.quantile(alpha, torch.tensor([0.1, 0.5, 0.9], device=alpha.device))
    return dict(entries=int(alpha.numel()), mean=round(float(alpha.mean()), 4), q10=round(float(q[0]), 4), q50=round(float(q[1]), 4),
                q90=round(float(q[2]), 4), below_0_1=round(float((alpha < 0.1).float().mean()), 4),
                below_0_5=round(float((alpha < 0.5).float().mean()), 4), at_1=round(float((alpha == 1.0).float().mean()), 4))


def part_ntuple_coherent_sweep(eval_steps=12288, chunk=(0, 1)):
    import torch
    import tetris_piclim as T
    cells = []
    for form in (dict(), dict(lam=0.5, horizon=8), dict(lam=0.8, horizon=4, symmetric=True)):
        for rate in (4.0, 8.0, 16.0, 32.0, 64.0):
            for coherent in (False, True):
                cells.append(dict(game="l10_m40", rate=rate, coherent=coherent, **form))
    cells.sort(key=lambda c: (c != dict(game="l10_m40", rate=16.0, coherent=False)))               # the baseline first
    cells += [dict(game="two_piece", rate=rate, coherent=coherent) for rate in (64.0, 256.0, 1024.0) for coherent in (False, True)]
    mine = cells[chunk[0]::chunk[1]]
    big = None
    if any(c["game"] == "l10_m40" for c in mine):
        gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
        big = gen_env.carved_configs(1 << 16, seed=7)
        gen_env.terminate()

    def result(r):
        p = r["win_rate"]
        return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5),
                    standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))

    def learn(game, **kw):
        if game == "two_piece":                                  # test_ntuple_gpu.py's game and budget
            carved = T.generate_configs(2, 2, 64, seed=107)
            env = T.BatchedTetris(2, 2, 4096, device="cuda:0", seed=3, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=carved)
            learner, budget, evaluation = T.NTupleLearner(env, seed=5, gamma=1.0, epsilon=0.25, **kw), (100, 200), 16
        else:                                                    # part ntuple_trace_sweep's sequence
            env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
            learner, budget, evaluation = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, **kw), (10000, 30000), eval_steps
        got = dict(kw, game=game, zero_table=result(learner.evaluate(evaluation)), trained=[])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for steps in budget:
            learner.train(steps)
            got["trained"].append(dict(steps=learner.steps, **result(learner.evaluate(evaluation))))
        got.update(seconds=round(time.perf_counter() - t0, 2), entries_in_use=int((learner.table != 0).sum()),
                   largest_entry=int(learner.table.abs().max()), symmetric_table=T.ntuple_is_symmetric(learner.table))
        if learner.coherent:
            got["alpha"] = _alpha_summary(T, learner.coherence)
        env.terminate()
        print(json.dumps(got), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        return got
    runs = [learn(**cell) for cell in mine]
    large = [r for r in runs if r["game"] == "l10_m40"]
    return dict(part="ntuple_coherent_sweep", chunk=list(chunk), boards=4096, seed=11, pool=1 << 16, pool_seed=7,
                reward=list(NTUPLE_LARGE_REWARD), gamma=1.0, epsilon=0.05, eval_steps=eval_steps,
                best=max(large, key=lambda r: r["trained"][-1]["win_rate"]) if large else None, runs=runs)


def _shape_ring(T, n, slots=17):
    """Part ntuple_trace's ring: the last `slots` states of n mid-game boards (L=10 / M=40), oldest first, and the environment."""
    import torch
    env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
    env.load_configs(*env.synthetic_configs(4096))
    env.reset()
    ring = [torch.empty((slots, n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2)]
    for t in range(6 + slots):
        env.step(env.synthetic_actions(t), observe=False)
        if t >= 6:
            a, b = env.raw_planes()
            ring[0][t - 6].copy_(a)
            ring[1][t - 6].copy_(b)
    return env, ring


def _shape_calls(L, check, ring, n, head, slots, tables, coherences, error, out, stream, twin=None):
    """name -> call of the seven timed forms of the six entries, for table shape `s`: through the _shaped entries of library L, or,
    with twin=True, through the entries without a shape (2 x 4 only)."""
    pa, pb = ring[0].data_ptr(), ring[1].data_ptr()
    na, nb = ring[0][head].data_ptr(), ring[1][head].data_ptr()
    action, second, score, value, after_a, after_b = (t.data_ptr() for t in out)
    rate, decay = 100.0, 0.9

    def calls(s):
        t, c, e = tables[s].data_ptr(), coherences[s].data_ptr(), error.data_ptr()
        tail = (stream,) if twin else (s, stream)
        f = (lambda name: getattr(L, name)) if twin else (lambda name: getattr(L, name + "_shaped"))
        head_args = (na, nb, n, 10, 40, 1.0, 10.0, -1.0, 1.0, t, 0.05, 11, 3, action)
        return {
            "value": lambda: check(f("tpl_ntuple_value")(na, nb, n, 10, 40, t, value, *tail)),
            "act": lambda: check(f("tpl_ntuple_act")(*head_args, score, after_a, after_b, value, *tail)),
            "search": lambda: check(f("tpl_ntuple_search")(*head_args, second, score, after_a, after_b, value, *tail)),
            "update": lambda: check(f("tpl_ntuple_update")(na, nb, n, 10, 40, t, e, rate, *tail)),
            "trace_h4": lambda: check(f("tpl_ntuple_update_trace")(pa, pb, n, slots, head, 4, 10, 40, t, e, rate, decay, 0, *tail)),
            "trace_h4_symmetric": lambda: check(f("tpl_ntuple_update_trace")(pa, pb, n, slots, head, 4, 10, 40, t, e, rate, decay, 1, *tail)),
            "coherent_h4": lambda: check(f("tpl_ntuple_update_coherent")(pa, pb, n, slots, head, 4, 10, 40, t, c, e, rate, decay, 0, *tail)),
        }
    return calls


def _shape_buffers(T, m, n):
    import numpy as np
    import torch
    tables, coherences = {}, {}
    for s, name in ((0, "2x4"), (1, "3x3")):
        host = np.random.default_rng(s).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_SHAPES[name][2]).astype(np.int32)
        tables[s] = torch.from_numpy(host).to("cuda:0")
        coherences[s] = T.ntuple_coherence("cuda:0", name)
    error = torch.empty(n, dtype=torch.float32, device="cuda:0").normal_()
    out = [torch.empty(n, dtype=torch.uint8, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0"),
           torch.empty(n, dtype=torch.float32, device="cuda:0"), torch.empty(n, dtype=torch.float32, device="cuda:0"),
           torch.empty((n, 4), dtype=torch.int32, device="cuda:0"), torch.empty((n, 4), dtype=torch.int32, device="cuda:0")]
    return tables, coherences, error, out


def part_ntuple_shape(rounds=5, reps=10):
    import numpy as np
    import torch
    import tetris_piclim as T
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import learn_ref as R
    m = T._learn_lib
    L, check = m.lib(), m.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    slots, head = 17, 16
    kernels = ("value_kernel", "act_kernel", "search_kernel", "trace_kernelILb0", "trace_kernelILb1", "coherent_step_kernelILb0",
               "coherent_accumulate_kernelILb0")
    out = dict(part="ntuple_shape", slots=slots, head=head, rate=100.0, decay=0.9,
               static_valu={p + k: _static_valu(p + k, m.build_library()) for k in kernels for p in ("ntuple_", "ntuple3_")})
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env, ring = _shape_ring(T, n, slots)
        a, b = (x[head, :4096].cpu().numpy().view(np.uint32) for x in ring)
        f = R.decode_state(a, b)
        in_use = {}
        for name in ("2x4", "3x3"):
            _, used = m.ntuple_indices(f["rows"], f["cur"], 10, 40, f["lines"].astype(np.int64), f["moves"].astype(np.int64), shape=name)
            in_use[name] = round(float(used[f["state"] == 0].sum(axis=1).mean()), 1)         # the counter included
        tables, coherences, error, outputs = _shape_buffers(T, m, n)
        calls = _shape_calls(L, check, ring, n, head, slots, tables, coherences, error, outputs, stream)
        variants = [(f"{name}_{shape}", fn) for s, shape in ((0, "2x4"), (1, "3x3")) for name, fn in calls(s).items()]
        variants.sort(key=lambda v: v[0])                        # each entry's two shapes next to each other in every round
        for s in (0, 1):                                         # step sizes of every kind before anything is timed
            for _ in range(2):
                error.normal_()
                calls(s)["coherent_h4"]()
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                                  # alternate the variants round by round
            for name, fn in variants:
                times[name].append(_timed(fn, reps if "search" not in name else max(reps // 3, 2)))
        med = {name: sorted(ts)[rounds // 2] for name, ts in times.items()}
        row = dict(boards=n, entries_in_use_per_board=in_use)
        for name in calls(0):
            row[name] = {"2x4_us": _spread(times[name + "_2x4"]), "3x3_us": _spread(times[name + "_3x3"]),
                         "3x3_over_2x4": round(med[name + "_3x3"] / med[name + "_2x4"], 3)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        env.terminate()
        del tables, coherences, ring, outputs, error
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=reps, search_launches_per_timing=max(reps // 3, 2), rows=rows)
    return out


def part_ntuple_shape_sweep(eval_steps=12288):
    import torch
    import tetris_piclim as T
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()

    def result(r):
        p = r["win_rate"]
        return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5),
                    standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))

    def learn(keep=False, **kw):
        """part_ntuple_trace_sweep's sequence: the zero table played, 10,000 steps, an evaluation, 30,000 steps, an evaluation."""
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, **kw)
        got = dict(kw, zero_table=result(learner.evaluate(eval_steps)), trained=[])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for steps in (10000, 30000):
            learner.train(steps)
            got["trained"].append(dict(steps=learner.steps, **result(learner.evaluate(eval_steps))))
        got.update(seconds=round(time.perf_counter() - t0, 2), entries_in_use=int((learner.table != 0).sum()),
                   largest_entry=int(learner.table.abs().max()), symmetric_table=T.ntuple_is_symmetric(learner.table))
        table = learner.table.clone() if keep else None
        env.terminate()
        print(json.dumps(got), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        return got, table
    baseline, _ = learn(rate=16.0)
    runs, tables = [], []
    for form in (dict(), dict(lam=0.5, horizon=8), dict(lam=0.8, horizon=4, symmetric=True)):
        for rate in (4.0, 8.0, 16.0, 32.0):
            got, table = learn(keep=True, shape="3x3", rate=rate, **form)
            runs.append(got)
            tables.append(table)
    at = max(range(len(runs)), key=lambda i: runs[i]["trained"][-1]["win_rate"])
    env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
    player = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, shape="3x3")
    player.table.copy_(tables[at])
    deep = dict(depth_1=result(player.evaluate(eval_steps)), depth_2=result(player.evaluate(eval_steps, depth=2)))
    env.terminate()
    return dict(part="ntuple_shape_sweep", boards=4096, seed=11, pool=1 << 16, pool_seed=7, reward=list(NTUPLE_LARGE_REWARD), gamma=1.0,
                epsilon=0.05, eval_steps=eval_steps, baseline=baseline, best=runs[at], best_played=deep, runs=runs)


NTUPLE_BEAM_SHAPES = ((1, 1), (2, 34), (3, 8), (4, 16), (6, 16), (11, 64))


def part_ntuple_beam(rounds=3, n=1 << 20, eval_steps=12288):
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
    gamma = 0.99
    env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=1, auto_reset=True)
    env.load_configs(*env.synthetic_configs(4096))
    env.reset()
    for t in range(6):                                           # mid-game boards
        env.step(env.synthetic_actions(t), observe=False)
    a, b = (x.cpu().numpy().view(np.uint32) for x in env.raw_planes())
    action = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    placement = {shape: T.BeamPolicy(env, classical, *shape) for shape in NTUPLE_BEAM_SHAPES}
    sample = {k: v[:4096].cpu().numpy() for k, v in env.packed_state().items()}
    count = np.array([17, 34, 34, 34, 17, 17, 9, 9], np.int64)
    running = ((b[:, 1] >> 28) & 3) == 0
    window = b[:, 3].astype(np.uint64) | ((b[:, 2] >> 28).astype(np.uint64) << np.uint64(32))
    first = np.where(running, count[(window & np.uint64(7)).astype(np.int64)], 0)
    out = dict(part="ntuple_beam", boards=n, rounds=rounds, gamma=gamma,
               model="a ply costs (tuples in use) x (placements) x (nodes) gathers, at the rate act and search resolve theirs in this run")
    shapes = []
    for name in ("2x4", "3x3"):
        entries = m.NTUPLE_SHAPES[name][2]
        table = torch.from_numpy(np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, entries).astype(np.int32)).to("cuda:0")
        _, used = m.ntuple_indices(sample["rows"].view(np.uint16), sample["cur"], 10, 40, sample["lines"], sample["moves"], name)
        in_use = float(used.sum(axis=1).mean())                  # of the root boards: a child holds one piece more
        act, search = T.NTuplePolicy(env, table, gamma=gamma), T.NTuplePolicy(env, table, gamma=gamma, depth=2)
        beams = {shape: T.NTupleBeamPolicy(env, table, *shape, gamma=gamma) for shape in NTUPLE_BEAM_SHAPES}
        reps = {shape: 10 if shape[0] <= 2 else 3 if shape[1] < 64 else 1 for shape in NTUPLE_BEAM_SHAPES}
        times = {k: [] for k in ["act", "search"] + [("ntuple",) + s for s in NTUPLE_BEAM_SHAPES] + [("placement",) + s for s in NTUPLE_BEAM_SHAPES]}
        for _ in range(rounds):                                  # alternate the kernels round by round
            times["act"].append(_timed(lambda: act.act(out=action, step=0), 10, warmup=1))
            times["search"].append(_timed(lambda: search.act(out=action, step=0), 10, warmup=1))
            for shape in NTUPLE_BEAM_SHAPES:
                times[("ntuple",) + shape].append(_timed(lambda: beams[shape].act(out=action), reps[shape], warmup=1))
                times[("placement",) + shape].append(_timed(lambda: placement[shape].act(out=action), reps[shape], warmup=1))
        med = {k: sorted(v)[rounds // 2] for k, v in times.items()}
        act_moves = float(first.mean())
        _, search_moves, _ = _beam_model(a, b, 2, 34, known=11)
        rate_act = n * act_moves * in_use / med["act"]
        rate_search = n * search_moves * in_use / med["search"]
        row = dict(shape=name, tuples_in_use_per_board=round(in_use, 1), act_us=_spread(times["act"]), search_us=_spread(times["search"]),
                   act_moves_per_board=round(act_moves, 1), search_moves_per_board=round(search_moves, 1),
                   act_gathers_per_s=float(f"{rate_act:.3g}"), search_gathers_per_s=float(f"{rate_search:.3g}"))
        for shape in NTUPLE_BEAM_SHAPES:
            t = med[("ntuple",) + shape]
            moves, _, plies = _beam_model(a, b, *shape, known=11)
            gathers = n * moves * in_use
            row[f"{shape[0]}x{shape[1]}"] = dict(
                us=_spread(times[("ntuple",) + shape]), launches_per_timing=reps[shape], mean_plies=round(plies, 2),
                moves_per_board=round(moves, 1), gathers_per_s=float(f"{gathers / t:.3g}"),
                predicted_ms_at_act_rate=round(gathers / rate_act * 1e3, 2), predicted_ms_at_search_rate=round(gathers / rate_search * 1e3, 2),
                measured_over_predicted_at_search_rate=round(t / (gathers / rate_search), 3),
                over_ntuple_search=round(t / med["search"], 3), over_ntuple_act=round(t / med["act"], 3),
                placement_beam_us=_spread(times[("placement",) + shape]),
                over_placement_beam=round(t / med[("placement",) + shape], 3))
        shapes.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        del table, beams
    env.terminate()
    torch.cuda.empty_cache()
    out["act"] = shapes

    # play strength: part ntuple_shape_sweep's TD(0) run at rate 16 (the zero table played, 10,000 steps, an evaluation, 30,000
    # steps) for each shape, then the table played at every depth
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()

    def result(r, seconds):
        p = r["win_rate"]
        return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5),
                    standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6), seconds=round(seconds, 2))

    played = []
    for name in ("2x4", "3x3"):
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, rate=16.0, shape=name)
        learner.evaluate(eval_steps)
        learner.train(10000)
        learner.evaluate(eval_steps)
        learner.train(30000)
        got = dict(shape=name, rate=16.0, steps=learner.steps, entries_in_use=int((learner.table != 0).sum()))
        for depth, width in ((1, None), (2, None), (3, 8), (4, 16), (6, 16)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = learner.evaluate(eval_steps, depth=depth, width=width)
            got[f"depth{depth}" + (f"_width{width}" if width else "")] = result(r, time.perf_counter() - t0)
            print(json.dumps({name: got}), file=sys.stderr, flush=True)
        played.append(got)
        env.terminate()
    out["l10_m40"] = dict(boards=4096, seed=11, pool=1 << 16, pool_seed=7, reward=list(NTUPLE_LARGE_REWARD), gamma=1.0, epsilon=0.05,
                          eval_steps=eval_steps, tables=played)
    return out


NTUPLE_SUM = "2x4+3x3"


def part_ntuple_sum(rounds=5, reps=10):
    """A sum table beside its two twins -- the 2 x 4 and the 3 x 3 table that are its parts -- on part ntuple_shape's boards."""
    import numpy as np
    import torch
    import tetris_piclim as T
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import learn_ref as R
    m = T._learn_lib
    slots, head = 17, 16
    names = ("2x4", "3x3", NTUPLE_SUM)
    kernels = ("ntuple_value_kernel", "ntuple3_value_kernel", "ntuple_sum_value_kernel", "ntuple_act_kernel", "ntuple3_act_kernel",
               "ntuple_sum_act_kernel")
    out = dict(part="ntuple_sum", gamma=1.0, epsilon=0.05, learner_rate=1.0,
               static_valu={k: _static_valu(k, m.build_library()) for k in kernels})
    rows = []
    for n in (1 << 16, 1 << 18, 1 << 20):
        env, ring = _shape_ring(T, n, slots)                     # the environment stands at the ring's newest slot
        a, b = (x[head, :4096].cpu().numpy().view(np.uint32) for x in ring)
        f = R.decode_state(a, b)
        in_use = {}
        for name in names:
            _, used = m.ntuple_indices(f["rows"], f["cur"], 10, 40, f["lines"].astype(np.int64), f["moves"].astype(np.int64), shape=name)
            in_use[name] = round(float(used[f["state"] == 0].sum(axis=1).mean()), 1)         # the counters included
        del ring
        whole = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_ENTRIES_SUM).astype(np.int32)
        table = {NTUPLE_SUM: torch.from_numpy(whole).to("cuda:0")}
        table["2x4"], table["3x3"] = (p.clone() for p in T.ntuple_parts(table[NTUPLE_SUM]))          # the twins: its parts, on their own
        action, second = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        score, value = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
        after = tuple(torch.empty((n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2))
        variants = {}
        for name in names:
            act = T.NTuplePolicy(env, table[name], gamma=1.0, epsilon=0.05, seed=11)
            search = T.NTuplePolicy(env, table[name], gamma=1.0, epsilon=0.05, seed=11, depth=2)
            beams = {shape: T.NTupleBeamPolicy(env, table[name], *shape, gamma=1.0) for shape in ((3, 8), (6, 16))}
            variants[("value", name)] = (lambda t=table[name]: T.ntuple_value(env, t, out=value), reps)
            variants[("act", name)] = (lambda p=act: p.act(out=action, score=score, after=after, value=value, step=3), reps)
            variants[("search", name)] = (lambda p=search: p.act(out=action, score=score, after=after, value=value, step=3,
                                                                 second=second), max(reps // 3, 2))
            variants[("beam_3x8", name)] = (lambda p=beams[(3, 8)]: p.act(out=action), 3)
            variants[("beam_6x16", name)] = (lambda p=beams[(6, 16)]: p.act(out=action), 1)
        order = sorted(variants)                                 # an entry's three tables next to each other in every round
        times = {k: [] for k in order}
        for _ in range(rounds):                                  # alternate the variants round by round
            for k in order:
                fn, count = variants[k]
                times[k].append(_timed(fn, count, warmup=1))
        # one learner step -- act, value, subtract, update (a sum table: two update calls), environment step -- plain and coherent; the
        # learners step the environment, so they come last
        for coherent in (False, True):
            learners = {name: T.NTupleLearner(env, gamma=1.0, rate=1.0, epsilon=0.05, seed=11, shape=name, coherent=coherent) for name in names}
            for name in names:
                learners[name].table.copy_(table[name])          # the random table: gathers all over it, as in the kernels above
                learners[name].train(3)                          # step sizes of every kind before anything is timed
                times[("learner_step_coherent" if coherent else "learner_step", name)] = []
            for _ in range(rounds):
                for name in names:
                    k = ("learner_step_coherent" if coherent else "learner_step", name)
                    times[k].append(_timed(lambda l=learners[name]: l.train(1), reps, warmup=1))
            del learners
        med = {k: sorted(ts)[rounds // 2] for k, ts in times.items()}
        row = dict(boards=n, entries_in_use_per_board=in_use)
        for what in sorted({k[0] for k in times}):
            row[what] = {name + "_us": _spread(times[(what, name)]) for name in names}
            row[what]["sum_over_the_twins_together"] = round(med[(what, NTUPLE_SUM)] / (med[(what, "2x4")] + med[(what, "3x3")]), 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        env.terminate()
        del table, variants, after
        torch.cuda.empty_cache()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=reps, search_launches_per_timing=max(reps // 3, 2), beam_launches_per_timing=[3, 1],
                         rows=rows)
    return out


def part_ntuple_sum_sweep(eval_steps=12288):
    """Part ntuple_shape_sweep's set-up unchanged; its 2 x 4 and 3 x 3 TD(0) runs at rate 16 again, then a sum table as TD(0)."""
    import torch
    import tetris_piclim as T
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()

    def result(r):
        p = r["win_rate"]
        return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5),
                    standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))

    def learn(keep=False, **kw):
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, **kw)
        got = dict(kw, zero_table=result(learner.evaluate(eval_steps)), trained=[])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for steps in (10000, 30000):
            learner.train(steps)
            got["trained"].append(dict(steps=learner.steps, **result(learner.evaluate(eval_steps))))
        got.update(seconds=round(time.perf_counter() - t0, 2), entries_in_use=[int((p != 0).sum()) for p in T.ntuple_parts(learner.table)],
                   largest_entry=int(learner.table.abs().max()))
        table = learner.table.clone() if keep else None
        env.terminate()
        print(json.dumps(got), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        return got, table
    baselines = [learn(shape=shape, rate=16.0)[0] for shape in ("2x4", "3x3")]
    expected = [(1473217, 1480033), (1467276, 1469796)]           # profiles/learner/sweep_ntuple_shape.log
    reproduced = [(b["trained"][-1]["wins"], b["trained"][-1]["episodes"]) == e for b, e in zip(baselines, expected)]
    runs, tables = [], []
    for rate in (2.0, 4.0, 8.0, 16.0):
        got, table = learn(keep=True, shape=NTUPLE_SUM, rate=rate)
        runs.append(got)
        tables.append(table)
    at = max(range(len(runs)), key=lambda i: runs[i]["trained"][-1]["win_rate"])
    env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
    player = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, shape=NTUPLE_SUM)
    player.table.copy_(tables[at])
    deep = dict(depth_1=result(player.evaluate(eval_steps)), depth_2=result(player.evaluate(eval_steps, depth=2)),
                beam_3x8=result(player.evaluate(eval_steps, depth=3, width=8)))
    env.terminate()
    return dict(part="ntuple_sum_sweep", boards=4096, seed=11, pool=1 << 16, pool_seed=7, reward=list(NTUPLE_LARGE_REWARD), gamma=1.0,
                epsilon=0.05, eval_steps=eval_steps, baselines=baselines, baselines_reproduced_win_for_win=reproduced, best=runs[at],
                best_played=deep, runs=runs)


def part_ntuple_stage(rounds=5, reps=10, n=1 << 20):
    """Staged tables beside their plain twins on part ntuple_shape's boards: one stage live, and four."""
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    names = ("2x4", "3x3", NTUPLE_SUM)
    kinds = ("plain", "one_stage", "four_stages")
    env, ring = _shape_ring(T, n, 2)                           # the environment stands at the ring's newest slot
    del ring
    for t in range(8, 208):                                    # boards in lockstep share one stage: play on until episodes have ended
        env.step(env.synthetic_actions(t), observe=False)     # at different moves and the boards stand all over the game
    four = T.ntuple_stage_map(10, 40, moves=4)

    def stages():
        """How many of the first 4,096 boards stand in each stage of the four-stage map, as the form's timings begin."""
        k = m.ntuple_counter_index(10, 40, *(x.astype(np.int64) for x in _lines_and_moves(*env.raw_planes())))
        return {int(g): int(c) for g, c in zip(*np.unique(four.numpy()[k], return_counts=True))}
    out = dict(part="ntuple_stage", boards=n, gamma=1.0, epsilon=0.05, learner_rate=1.0, rounds=rounds, launches_per_timing=reps,
               search_launches_per_timing=max(reps // 3, 2), beam_launches_per_timing=3)
    action, second = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    score, value = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
    after = tuple(torch.empty((n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2))
    rows = []
    for name in names:
        entries = m.ntuple_entries_of(name)
        spread = stages()
        body = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, 8 * entries).astype(np.int32)
        table = {"plain": torch.from_numpy(body[:entries].copy()).to("cuda:0")}
        for kind, stage_map in (("one_stage", torch.zeros(1024, dtype=torch.int32)), ("four_stages", four)):
            table[kind] = torch.from_numpy(np.concatenate([body, stage_map.numpy()])).to("cuda:0")      # eight distinct blocks
        variants = {}
        for kind in kinds:
            act = T.NTuplePolicy(env, table[kind], gamma=1.0, epsilon=0.05, seed=11)
            search = T.NTuplePolicy(env, table[kind], gamma=1.0, epsilon=0.05, seed=11, depth=2)
            beam = T.NTupleBeamPolicy(env, table[kind], 3, 8, gamma=1.0)
            variants[("value", kind)] = (lambda t=table[kind]: T.ntuple_value(env, t, out=value), reps)
            variants[("act", kind)] = (lambda p=act: p.act(out=action, score=score, after=after, value=value, step=3), reps)
            variants[("search", kind)] = (lambda p=search: p.act(out=action, score=score, after=after, value=value, step=3,
                                                                 second=second), max(reps // 3, 2))
            variants[("beam_3x8", kind)] = (lambda p=beam: p.act(out=action), 3)
        order = sorted(variants)                                 # an entry's three tables next to each other in every round
        times = {key: [] for key in order}
        for _ in range(rounds):                                  # alternate the variants round by round
            for key in order:
                fn, count = variants[key]
                times[key].append(_timed(fn, count, warmup=1))
        # one learner step -- act, value, subtract, update, environment step; the learners step the environment, so they come last
        learners = {kind: T.NTupleLearner(env, gamma=1.0, rate=1.0, epsilon=0.05, seed=11, shape=name,
                                          stage_map=None if kind == "plain" else T.ntuple_map(table[kind]).cpu()) for kind in kinds}
        for kind in kinds:
            learners[kind].table.copy_(table[kind])              # the random blocks: gathers all over them, as in the kernels above
            learners[kind].train(3)
            times[("learner_step", kind)] = []
        for _ in range(rounds):
            for kind in kinds:
                times[("learner_step", kind)].append(_timed(lambda l=learners[kind]: l.train(1), reps, warmup=1))
        del learners
        med = {key: sorted(ts)[rounds // 2] for key, ts in times.items()}
        row = dict(form=name, stages_of_the_first_4096_boards=spread, table_bytes={kind: int(table[kind].numel() * 4) for kind in kinds},
                   bytes_in_use=dict(plain=4 * entries, one_stage=4 * entries + 4096, four_stages=16 * entries + 4096))
        for what in sorted({key[0] for key in times}):
            row[what] = {kind + "_us": _spread(times[(what, kind)]) for kind in kinds}
            for kind in kinds[1:]:
                row[what][kind + "_over_plain"] = round(med[(what, kind)] / med[(what, "plain")], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del table, variants
        torch.cuda.empty_cache()
    env.terminate()
    out["rows"] = rows
    return out


def _lines_and_moves(pa, pb):
    """(lines, moves) of packed states, through the tests' decoder."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import learn_ref as R
    f = R.decode_state(pa[:4096].cpu().numpy().view(np.uint32), pb[:4096].cpu().numpy().view(np.uint32))
    return f["lines"], f["moves"]


def part_ntuple_stage_sweep(eval_steps=12288):
    """Part ntuple_shape_sweep's set-up unchanged; its 3 x 3 TD(0) run at rate 16 again, then staged 3 x 3 tables under three maps, each
    from zero and each promoted from that run's table."""
    import torch
    import tetris_piclim as T
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()

    def result(r):
        p = r["win_rate"]
        return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5),
                    standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))

    def learn(label, **kw):
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, shape="3x3", rate=16.0, **kw)
        got = dict(run=label, before_training=result(learner.evaluate(eval_steps)), trained=[])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for steps in (10000, 30000):
            learner.train(steps)
            got["trained"].append(dict(steps=learner.steps, **result(learner.evaluate(eval_steps))))
        blocks = T.ntuple_stages(learner.table) if T.ntuple_is_staged(learner.table) else (learner.table,)
        got.update(seconds=round(time.perf_counter() - t0, 2), entries_in_use=[int((b != 0).sum()) for b in blocks],
                   depth_2=result(learner.evaluate(eval_steps, depth=2)), beam_3x8=result(learner.evaluate(eval_steps, depth=3, width=8)))
        table = learner.table.clone()
        env.terminate()
        print(json.dumps(got), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        return got, table
    baseline, trained = learn("3x3 plain")
    expected = (1467276, 1469796)                                 # profiles/learner/sweep_ntuple_shape.log
    reproduced = (baseline["trained"][-1]["wins"], baseline["trained"][-1]["episodes"]) == expected
    carried, _ = learn("3x3 plain, trained on from the baseline", start=trained)   # the control of the promoted runs: the same second budget
    runs = []
    for label, grid in (("moves=2", dict(moves=2)), ("moves=4", dict(moves=4)), ("lines=2 x moves=4", dict(lines=2, moves=4))):
        stage_map = T.ntuple_stage_map(10, 40, **grid)
        runs.append(learn("staged " + label + ", from zero", stage_map=stage_map)[0])
        runs.append(learn("staged " + label + ", promoted from the baseline", stage_map=stage_map, start=trained)[0])
    return dict(part="ntuple_stage_sweep", boards=4096, seed=11, pool=1 << 16, pool_seed=7, reward=list(NTUPLE_LARGE_REWARD), gamma=1.0,
                epsilon=0.05, rate=16.0, eval_steps=eval_steps, baseline=baseline, baseline_reproduced_win_for_win=reproduced,
                baseline_trained_on=carried, hand_made_features_win_rate=0.99925, runs=runs)


NTUPLE_FEATURE_FORMS = ("feat", "3x3+feat")


def part_ntuple_feature(rounds=5, reps=10, n=1 << 20):
    """Feature tables beside the 3 x 3 table on part ntuple_shape's boards."""
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    L, check = m.lib(), m.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    slots, head = 17, 16
    names = ("3x3",) + NTUPLE_FEATURE_FORMS
    kernels = ("ntuple3_value_kernel", "ntuple_feature_value_kernel", "ntuple_feature3_value_kernel", "ntuple3_act_kernel",
               "ntuple_feature_act_kernel", "ntuple_feature3_act_kernel")
    out = dict(part="ntuple_feature", boards=n, gamma=1.0, epsilon=0.05, learner_rate=1.0,
               static_valu={k: _static_valu(k, m.build_library()) for k in kernels})
    env, ring = _shape_ring(T, n, slots)                         # the environment stands at the ring's newest slot
    whole = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_ENTRIES_3X3_FEAT).astype(np.int32)
    table = {"3x3+feat": torch.from_numpy(whole).to("cuda:0")}
    table["3x3"], table["feat"] = (p.clone() for p in T.ntuple_parts(table["3x3+feat"]))             # the twins: its parts, on their own
    bins = T.ntuple_feature_bins(env)[:4096].cpu().numpy()
    out["distinct_bins_per_feature_of_4096_boards"] = [int(np.unique(bins[:, j]).size) for j in range(9)]
    # the update kernel alone, beside the 3 x 3 update, on the ring
    error = torch.empty(n, dtype=torch.float32, device="cuda:0").normal_()
    ra, rb = ring[0].data_ptr(), ring[1].data_ptr()
    scratch = {name: table[name].clone() for name in ("3x3", "feat")}
    update = {}
    for horizon in (1, 4):
        for symmetric in (0, 1):
            args = (ra, rb, n, slots, head, horizon, 10, 40)
            tail = (error.data_ptr(), 100.0, 0.9, symmetric)
            calls = {"feat": lambda a=args, t=tail: check(L.tpl_ntuple_update_trace_feature(*a, scratch["feat"].data_ptr(), *t, stream)),
                     "3x3": lambda a=args, t=tail: check(L.tpl_ntuple_update_trace_shaped(*a, scratch["3x3"].data_ptr(), *t, 1, stream))}
            times = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    times[k].append(_timed(fn, reps))
            med = {k: sorted(ts)[rounds // 2] for k, ts in times.items()}
            update[f"h{horizon}" + ("_symmetric" if symmetric else "")] = {
                "feat_us": _spread(times["feat"]), "3x3_us": _spread(times["3x3"]), "feat_over_3x3": round(med["feat"] / med["3x3"], 4)}
    out["update"] = update
    del ring, scratch
    action, second = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    score, value = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
    after = tuple(torch.empty((n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2))
    variants = {}
    for name in names:
        act = T.NTuplePolicy(env, table[name], gamma=1.0, epsilon=0.05, seed=11)
        search = T.NTuplePolicy(env, table[name], gamma=1.0, epsilon=0.05, seed=11, depth=2)
        beams = {shape: T.NTupleBeamPolicy(env, table[name], *shape, gamma=1.0) for shape in ((3, 8), (6, 16))}
        variants[("value", name)] = (lambda t=table[name]: T.ntuple_value(env, t, out=value), reps)
        variants[("act", name)] = (lambda p=act: p.act(out=action, score=score, after=after, value=value, step=3), reps)
        variants[("search", name)] = (lambda p=search: p.act(out=action, score=score, after=after, value=value, step=3, second=second),
                                      max(reps // 3, 2))
        variants[("beam_3x8", name)] = (lambda p=beams[(3, 8)]: p.act(out=action), 3)
        variants[("beam_6x16", name)] = (lambda p=beams[(6, 16)]: p.act(out=action), 1)
    order = sorted(variants)                                     # an entry's three tables next to each other in every round
    times = {k: [] for k in order}
    for _ in range(rounds):                                      # alternate the variants round by round
        for k in order:
            fn, count = variants[k]
            times[k].append(_timed(fn, count, warmup=1))
    # one learner step -- act, value, subtract, update (a sum form: two update calls), environment step; the learners step the
    # environment, so they come last
    learners = {name: T.NTupleLearner(env, gamma=1.0, rate=1.0, epsilon=0.05, seed=11, shape=name) for name in names}
    for name in names:
        learners[name].table.copy_(table[name])
        learners[name].train(3)
        times[("learner_step", name)] = []
    for _ in range(rounds):
        for name in names:
            times[("learner_step", name)].append(_timed(lambda l=learners[name]: l.train(1), reps, warmup=1))
    med = {k: sorted(ts)[rounds // 2] for k, ts in times.items()}
    row = {}
    for what in sorted({k[0] for k in times}):
        row[what] = {name + "_us": _spread(times[(what, name)]) for name in names}
        row[what]["feat_over_3x3"] = round(med[(what, "feat")] / med[(what, "3x3")], 3)
        row[what]["3x3+feat_over_the_parts_together"] = round(med[(what, "3x3+feat")] / (med[(what, "3x3")] + med[(what, "feat")]), 3)
    env.terminate()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=reps, search_launches_per_timing=max(reps // 3, 2), beam_launches_per_timing=[3, 1],
                         row=row)
    return out


def part_ntuple_feature_sweep(eval_steps=12288):
    """Part ntuple_shape_sweep's set-up unchanged; its 3 x 3 TD(0) run at rate 16 again, the classical weights, then the feature forms."""
    import numpy as np
    import torch
    import tetris_piclim as T
    gen_env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=7)
    big = gen_env.carved_configs(1 << 16, seed=7)
    gen_env.terminate()

    def result(r):
        p = r["win_rate"]
        return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5),
                    standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))

    def learn(keep=False, **kw):
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, **kw)
        got = dict(kw, zero_table=result(learner.evaluate(eval_steps)), trained=[])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for steps in (10000, 30000):
            learner.train(steps)
            got["trained"].append(dict(steps=learner.steps, **result(learner.evaluate(eval_steps))))
        got.update(seconds=round(time.perf_counter() - t0, 2), entries_in_use=[int((p != 0).sum()) for p in T.ntuple_parts(learner.table)],
                   largest_entry=int(learner.table.abs().max()))
        table = learner.table.clone() if keep else None
        env.terminate()
        print(json.dumps(got), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        return got, table

    baseline = learn(shape="3x3", rate=16.0)[0]
    reproduced = (baseline["trained"][-1]["wins"], baseline["trained"][-1]["episodes"]) == (1467276, 1469796)   # sweep_ntuple_shape.log
    classical = np.array([4, 100, -100, -8, -1, 0, -2, -3, -6, -3, -2, -1], np.float32) * np.float32(0.1)
    env = T.BatchedTetris(10, 40, 1 << 16, device="cuda:0", seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=big)
    got = T.evaluate_heuristic(env, classical, None, 640)
    e, wins = int(got["episodes"][0]), int(got["wins"][0])
    hand = result(dict(episodes=e, wins=wins, win_rate=wins / max(e, 1)))
    env.terminate()
    out = dict(part="ntuple_feature_sweep", boards=4096, seed=11, pool=1 << 16, pool_seed=7, reward=list(NTUPLE_LARGE_REWARD), gamma=1.0,
               epsilon=0.05, eval_steps=eval_steps, baseline=baseline, baseline_reproduced_win_for_win=reproduced,
               classical_weights_one_ply=hand, forms={})
    rates = {"feat": (2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0, 512.0), "3x3+feat": (2.0, 4.0, 8.0, 16.0)}
    for shape in NTUPLE_FEATURE_FORMS:
        runs, tables = [], []
        for rate in rates[shape]:
            got, table = learn(keep=True, shape=shape, rate=rate)
            runs.append(got)
            tables.append(table)
        at = max(range(len(runs)), key=lambda i: runs[i]["trained"][-1]["win_rate"])
        symmetric, sym_table = learn(keep=True, shape=shape, rate=rates[shape][at] / 2, symmetric=True)
        same_rate, _ = learn(shape=shape, rate=rates[shape][at], symmetric=True)
        env = T.BatchedTetris(10, 40, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=big)
        player = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, shape=shape)
        player.table.copy_(tables[at])
        deep = dict(depth_1=result(player.evaluate(eval_steps)), depth_2=result(player.evaluate(eval_steps, depth=2)),
                    beam_3x8=result(player.evaluate(eval_steps, depth=3, width=8)))
        env.terminate()
        out["forms"][shape] = dict(best=runs[at], best_played=deep, best_symmetric_at_half_the_rate=symmetric,
                                   best_symmetric_at_the_same_rate=same_rate, runs=runs)
    return out


def part_ntuple_budget(rounds=5, reps=10, n=1 << 20):
    """The budget table beside its "feat" twin on part ntuple_shape's boards: every time as a ratio to the twin's in the same rounds."""
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    L, check = m.lib(), m.check
    stream = torch._C._cuda_getCurrentRawStream(0)
    slots, head = 17, 16
    kernels = ("ntuple_feature_value_kernel", "ntuple_budget_value_kernel", "ntuple_feature_act_kernel", "ntuple_budget_act_kernel",
               "ntuple_feature_search_kernel", "ntuple_budget_search_kernel", "ntuple_feature_beam_kernel", "ntuple_budget_beam_kernel")
    out = dict(part="ntuple_budget", boards=n, gamma=1.0, epsilon=0.05, learner_rate=1.0,
               static_valu={k: _static_valu(k, m.build_library()) for k in kernels})
    env, ring = _shape_ring(T, n, slots)                         # the environment stands at the ring's newest slot
    feat = torch.from_numpy(np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, m.NTUPLE_ENTRIES_FEAT).astype(np.int32)).to("cuda:0")
    table = {"feat": feat, "feat+spare": T.ntuple_budget(feat)}
    table["feat+spare"][:-1024].view(8, 10, 256)[:, 9] = torch.randint(-(1 << 20), 1 << 20, (8, 256), dtype=torch.int32, device="cuda:0")
    bins = T.ntuple_budget_bins(env)
    out["spare_bin_of_the_boards"] = dict(dead=int((bins[:, 9] == 0).sum()), clamped=int((bins[:, 9] == 255).sum()),
                                          distinct=int(torch.unique(bins[:, 9]).numel()))
    error = torch.empty(n, dtype=torch.float32, device="cuda:0").normal_()
    ra, rb = ring[0].data_ptr(), ring[1].data_ptr()
    scratch = {name: table[name].clone() for name in table}
    update = {}
    for horizon in (1, 4):
        for symmetric in (0, 1):
            args = (ra, rb, n, slots, head, horizon, 10, 40)
            tail = (error.data_ptr(), 100.0, 0.9, symmetric)
            calls = {"feat": lambda a=args, t=tail: check(L.tpl_ntuple_update_trace_feature(*a, scratch["feat"].data_ptr(), *t, stream)),
                     "feat+spare": lambda a=args, t=tail: check(L.tpl_ntuple_update_trace_budget(*a, scratch["feat+spare"].data_ptr(), *t, stream))}
            times = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    times[k].append(_timed(fn, reps))
            med = {k: sorted(ts)[rounds // 2] for k, ts in times.items()}
            update[f"h{horizon}" + ("_symmetric" if symmetric else "")] = {
                "feat_us": _spread(times["feat"]), "feat+spare_us": _spread(times["feat+spare"]),
                "budget_over_feat": round(med["feat+spare"] / med["feat"], 4)}
    out["update"] = update
    del ring, scratch
    action, second = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    score, value = (torch.empty(n, dtype=torch.float32, device="cuda:0") for _ in range(2))
    after = tuple(torch.empty((n, 4), dtype=torch.int32, device="cuda:0") for _ in range(2))
    forms = (("feat", "feat", False), ("feat+spare", "feat+spare", False), ("feat+spare_pruned", "feat+spare", True))
    variants = {}
    for label, name, bound in forms:
        act = T.NTuplePolicy(env, table[name], gamma=1.0, epsilon=0.05, seed=11, bound=bound)
        search = T.NTuplePolicy(env, table[name], gamma=1.0, epsilon=0.05, seed=11, depth=2, bound=bound)
        beams = {shape: T.NTupleBeamPolicy(env, table[name], *shape, gamma=1.0, bound=bound) for shape in ((3, 8), (6, 16))}
        if not bound:
            variants[("value", label)] = (lambda t=table[name]: T.ntuple_value(env, t, out=value), reps)
        variants[("act", label)] = (lambda p=act: p.act(out=action, score=score, after=after, value=value, step=3), reps)
        variants[("search", label)] = (lambda p=search: p.act(out=action, score=score, after=after, value=value, step=3, second=second),
                                       max(reps // 3, 2))
        variants[("beam_3x8", label)] = (lambda p=beams[(3, 8)]: p.act(out=action), 3)
        variants[("beam_6x16", label)] = (lambda p=beams[(6, 16)]: p.act(out=action), 1)
    order = sorted(variants)
    times = {k: [] for k in order}
    for _ in range(rounds):                                      # alternate the variants round by round
        for k in order:
            fn, count = variants[k]
            times[k].append(_timed(fn, count, warmup=1))
    learners = {label: T.NTupleLearner(env, gamma=1.0, rate=1.0, epsilon=0.05, seed=11, shape=name, bound=bound) for label, name, bound in forms}
    for label, name, _ in forms:
        learners[label].table.copy_(table[name])
        learners[label].train(3)
        times[("learner_step", label)] = []
    for _ in range(rounds):
        for label, _, _ in forms:
            times[("learner_step", label)].append(_timed(lambda l=learners[label]: l.train(1), reps, warmup=1))
    med = {k: sorted(ts)[rounds // 2] for k, ts in times.items()}
    row = {}
    for what in sorted({k[0] for k in times}):
        labels = [label for label, _, _ in forms if (what, label) in times]
        row[what] = {label + "_us": _spread(times[(what, label)]) for label in labels}
        for label in labels[1:]:
            row[what][label + "_over_feat"] = round(med[(what, label)] / med[(what, "feat")], 3)
    env.terminate()
    out["kernel"] = dict(rounds=rounds, launches_per_timing=reps, search_launches_per_timing=max(reps // 3, 2), beam_launches_per_timing=[3, 1],
                         row=row)
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), m.build_library()], capture_output=True, text=True, cwd=ROOT)
    out["resources"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "ntuple_budget" in l or "ntuple_feature_" in l and "feature3" not in l]
    return out


def part_ntuple_budget_sweep(eval_steps=12288):
    """The tight pool of the record (part_solve's and part_bound's): the rate-8 "feat" learner again, then the budget table."""
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    L_, M_, n = 10, 40, 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(n, seed=7)
    env.terminate()
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    M_new = 16
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], M_new)
    out = dict(part="ntuple_budget_sweep", boards=4096, seed=11, pool_seed=7, tight_pool=int(tight[0].shape[0]), M_new=M_new,
               reward=list(NTUPLE_LARGE_REWARD), gamma=1.0, epsilon=0.05, eval_steps=eval_steps, train_steps=40000, runs=[])

    def result(r):
        p = r["win_rate"]
        return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))

    def played(learner):
        """The table as it stands at one ply and at beam (3, 8), each without and with the prune (a "feat" table: without)."""
        budget = learner.shape == "feat+spare"
        got = {}
        for name, kw in (("one_ply", {}), ("beam_3x8", dict(depth=3, width=8))):
            for bound in ((False, True) if budget else (False,)):
                got[name + ("_pruned" if bound else "")] = result(learner.evaluate(eval_steps, bound=bound, **kw))
        return got

    def learn(label, pool=tight, M_pool=M_new, train=True, keep=False, **kw):
        env = T.BatchedTetris(L_, M_pool, 4096, device=dev, seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=pool)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        before = None
        if train:                                                # as the record's run: the start table is played first, then 40,000 steps
            before = result(learner.evaluate(eval_steps))
            for steps in (10000, 30000):
                learner.train(steps)
        got = dict(label=label, pool="tight" if pool is tight else "loose", trained=bool(train),
                   **{k: v for k, v in kw.items() if k != "start"}, start_table=before, played=played(learner))
        got["seconds"] = round(time.perf_counter() - t0, 2)
        if learner.shape == "feat+spare":
            row9 = learner.table[:-1024].view(8, 10, 256)[:, 9]
            got["row_9"] = dict(entries_in_use=int((row9 != 0).sum()), bin_0_mean=round(float(row9[:, 0].float().mean()) / 65536, 4),
                                live_bins_mean=round(float(row9[:, 1:][row9[:, 1:] != 0].float().mean()) / 65536, 4) if bool((row9[:, 1:] != 0).any()) else None)
        table = learner.table.clone() if keep else None
        env.terminate()
        print(json.dumps(got), file=sys.stderr, flush=True)      # progress: a long part must not stay silent
        out["runs"].append(got)
        return got, table

    baseline, feat = learn("feat rate 8, the record's run", keep=True, shape="feat", rate=8.0)
    one = baseline["played"]["one_ply"]
    out["baseline_reproduced_win_for_win"] = round(one["win_rate"], 5) == 0.51983
    promoted = T.ntuple_budget(feat)
    for bound in (False, True):                                  # the promoted table as it stands: with bound=True the prune alone
        learn("promoted, untrained", train=False, shape="feat+spare", rate=8.0, start=promoted, bound=bound)
    for rate in (2.0, 4.0, 8.0, 16.0, 32.0):
        for bound in (False, True):
            learn("from zero", shape="feat+spare", rate=rate, bound=bound)
    for bound in (False, True):
        learn("promoted, trained on", shape="feat+spare", rate=8.0, start=promoted, bound=bound)
    loose = (rows, pieces)
    learn("feat rate 8 on the loose pool", pool=loose, M_pool=M_, shape="feat", rate=8.0)
    for bound in (False, True):
        learn("from zero on the loose pool", pool=loose, M_pool=M_, shape="feat+spare", rate=8.0, bound=bound)
    return out


def part_solve(rounds=5, eval_steps=12288):
    import numpy as np
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    widths = (1, 8, 16, 64)
    share = lambda x: round(float(x.float().mean()), 5)
    out = dict(part="solve", weights="CLASSICAL_WEIGHTS", forward={}, carved={}, tight={}, time=[])

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)     # a long part must not stay silent

    # yield: the forward generator's games, kept by the reference's solver and by the beam
    for L_, M_ in ((5, 20), (10, 40)):
        env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
        fw = env.forward_configs(np.arange(10000))
        got = dict(seeds=10000, reference_winnable=share(fw["winnable"]))
        for W in widths:
            found = T.solve_configs(fw["rows"], fw["sequence"], L_, M_, width=W, device=dev, validate=False)
            got[f"beam_w{W}"] = share(found["solved"])
            if W == 16:
                got["reference_winnable_that_w16_solves"] = share(found["solved"][fw["winnable"]]) if bool(fw["winnable"].any()) else None
                got["mean_solution_len_w16"] = round(float(found["solution_len"][found["solved"]].float().mean()), 2)
        out["forward"][f"L{L_}_M{M_}"] = got
        progress(got)
        env.terminate()

    # the sweeps' carved pool: winnable by construction, so everything short of 1 is the beam's miss rate
    L_, M_, n = 10, 40, 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces, _, carved_len = env.carved_configs(n, seed=7, with_solutions=True)
    env.terminate()
    hist = lambda x: np.bincount(x.cpu().numpy().astype(np.int64), minlength=M_ + 1).tolist()
    out["carved"] = dict(pool=n, pool_seed=7, L=L_, M=M_, carving_solution_len_histogram=hist(carved_len),
                         carving_mean=round(float(carved_len.float().mean()), 2), widths={})
    solved16 = None
    for W in widths:
        found = T.solve_configs(rows, pieces, L_, M_, width=W, device=dev, validate=False)
        ok = found["solved"]
        out["carved"]["widths"][f"w{W}"] = dict(solved=share(ok), mean_len=round(float(found["solution_len"][ok].float().mean()), 2),
                                                solution_len_histogram=hist(found["solution_len"][ok]))
        if W == 16:
            solved16 = found
    progress({k: v["solved"] for k, v in out["carved"]["widths"].items()})

    # a tight pool: the median solution length of width 16 as the move budget
    lens = solved16["solution_len"][solved16["solved"]]
    M_new = int(lens.float().median())
    t_rows, t_pieces = T.tighten_pool(rows, pieces, solved16["solved"], solved16["solution_len"], M_new)
    tight = (t_rows, t_pieces)

    def result(e, wins):
        p = wins / max(e, 1)
        return dict(episodes=int(e), wins=int(wins), win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(e, 1)) ** 0.5, 6))

    def hand(pool, M_pool, **kw):
        env = T.BatchedTetris(L_, M_pool, 1 << 14, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=pool)
        got = T.evaluate_heuristic(env, T.CLASSICAL_WEIGHTS, None, 16 * (M_pool + 1), **kw)
        env.terminate()
        return result(int(got["episodes"][0]), int(got["wins"][0]))

    def learned(pool, M_pool):
        env = T.BatchedTetris(L_, M_pool, 4096, device=dev, seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=pool)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, shape="feat", rate=8.0)
        zero = learner.evaluate(eval_steps)
        for steps in (10000, 30000):
            learner.train(steps)
        got = learner.evaluate(eval_steps)
        env.terminate()
        return dict(zero_table=result(zero["episodes"], zero["wins"]), trained_40000_steps=result(got["episodes"], got["wins"]))

    out["tight"] = dict(M_new=M_new, from_width=16, size=int(t_rows.shape[0]), of=n,
                        classical_one_ply=hand(tight, M_new), classical_beam_3x8=hand(tight, M_new, depth=3, width=8),
                        feat_rate_8=learned(tight, M_new),
                        the_full_pool_for_comparison=dict(classical_one_ply=hand((rows, pieces), M_), classical_beam_3x8=hand((rows, pieces), M_, depth=3, width=8)))
    progress(out["tight"])

    # time: the solver, the placement beam at (12, W) on as many freshly reset boards, the forward generator
    median = lambda ts: sorted(ts)[len(ts) // 2]
    for count in (1 << 16, 1 << 20):
        env = T.BatchedTetris(L_, M_, count, device=dev, seed=7, auto_reset=False, assign="sequential")
        rows, pieces = env.carved_configs(count, seed=7)
        env.load_configs(rows, pieces, validate=False)
        env.reset()
        for W in (8, 16, 64):
            found = T.solve_configs(rows, pieces, L_, M_, width=W, device=dev, validate=False)
            plies = torch.where(found["solved"], found["solution_len"], torch.full_like(found["solution_len"], M_)).float().mean()
            plies = float(plies)                                 # (an unsolved game counts as M plies: an upper bound)
            w = torch.from_numpy(T.CLASSICAL_WEIGHTS.copy()).to(dev)
            outs = (torch.empty(count, dtype=torch.uint8, device=dev), torch.empty(count, dtype=torch.int32, device=dev),
                    torch.empty((count, M_), dtype=torch.uint8, device=dev))
            lib, stream = T._learn_lib.lib(), torch._C._cuda_getCurrentRawStream(0)
            solve = lambda: T._learn_lib.check(lib.tpl_placement_solve(rows.data_ptr(), pieces.data_ptr(), count, L_, M_, w.data_ptr(), W,
                                                                        outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, stream))
            beam = T.BeamPolicy(env, T.CLASSICAL_WEIGHTS, depth=12, width=W)
            action = torch.empty(count, dtype=torch.uint8, device=dev)
            reps = 3 if count == 1 << 16 else 1
            ts, tb = [], []
            for _ in range(rounds):                              # alternated
                ts.append(_timed(solve, reps, warmup=1))
                tb.append(_timed(lambda: beam.act(out=action), reps, warmup=1))
            s_med, b_med = median(ts), median(tb)
            line = dict(configurations=count, width=W, solved=share(found["solved"]), mean_plies_run=round(plies, 2),
                        solve_ms=round(s_med * 1e3, 3), configurations_per_second=round(count / s_med),
                        beam_12_ms=round(b_med * 1e3, 3), beam_scaled_by_plies_ms=round(b_med * plies / 12 * 1e3, 3),
                        solve_over_scaled_beam=round(s_med / (b_med * plies / 12), 3))
            out["time"].append(line)
            progress(line)
        env.terminate()
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    seeds = np.arange(10000)
    tf = [_timed(lambda: env.forward_configs(seeds), 1, warmup=1) for _ in range(rounds)]
    out["forward_generator"] = dict(games=10000, L=L_, M=M_, ms=round(median(tf) * 1e3, 3), games_per_second=round(10000 / median(tf)))
    env.terminate()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "placement_solve_kernel" in l or "placement_beam_kernel" in l]
    out["lds_note"] = "the solve kernel's dynamic tape of 2 W M bytes comes on top of its static lds"
    return out


def part_move_features(rounds=5, generations=8, population=32, per=2048):
    """The 14-feature form beside the 12: time of every kernel against its twin in the same run, and whether landing height and eroded
    cells help on the tight pool of part_solve (carved L = 10 / M = 40, 65,536 configurations, seed 7, solved at width 16,
    tighten_pool at the median solution length)."""
    import numpy as np
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    L_, M_ = 10, 40
    out = dict(part="move_features", time=[], tight={}, full={}, solver={})
    median = lambda ts: sorted(ts)[len(ts) // 2]
    classical14 = np.concatenate([T.CLASSICAL_WEIGHTS, np.zeros(2, np.float32)])

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    # time: 2^20 mid-game boards (carved configurations after twelve random steps), each kernel and its twin alternated
    count = 1 << 20
    env = T.BatchedTetris(L_, M_, count, device=dev, seed=7, auto_reset=True)
    rows, pieces = env.carved_configs(1 << 16, seed=7)
    env.load_configs(rows, pieces, validate=False)
    env.reset()
    for t in range(12):
        env.step(env.synthetic_actions(t), observe=False)
    action = torch.empty(count, dtype=torch.uint8, device=dev)
    players = [("act", lambda w: T.HeuristicPolicy(env, w)), ("search", lambda w: T.HeuristicPolicy(env, w, depth=2)),
               ("beam_3x8", lambda w: T.BeamPolicy(env, w, 3, 8)), ("beam_6x16", lambda w: T.BeamPolicy(env, w, 6, 16))]
    for name, make in players:
        p12, p14 = make(T.CLASSICAL_WEIGHTS), make(classical14)
        same = bool(torch.equal(p12.act().clone(), p14.act()))
        t12, t14 = [], []
        for _ in range(rounds):
            t12.append(_timed(lambda: p12.act(out=action), 3, warmup=1))
            t14.append(_timed(lambda: p14.act(out=action), 3, warmup=1))
        line = dict(kernel=name, boards=count, ms_12=round(median(t12) * 1e3, 3), ms_14=round(median(t14) * 1e3, 3),
                    ratio=round(median(t14) / median(t12), 4), same_actions_with_zero_move_weights=same)
        out["time"].append(line)
        progress(line)
    env.terminate()
    for n in (1 << 16, 1 << 20):
        env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
        rows_n, pieces_n = env.carved_configs(n, seed=7)
        env.terminate()
        t12, t14 = [], []
        for _ in range(rounds):
            t12.append(_timed(lambda: T.solve_configs(rows_n, pieces_n, L_, M_, T.CLASSICAL_WEIGHTS, 16, device=dev, validate=False), 1, warmup=1))
            t14.append(_timed(lambda: T.solve_configs(rows_n, pieces_n, L_, M_, classical14, 16, device=dev, validate=False), 1, warmup=1))
        line = dict(kernel="solve_w16", configurations=n, ms_12=round(median(t12) * 1e3, 3), ms_14=round(median(t14) * 1e3, 3),
                    ratio=round(median(t14) / median(t12), 4))
        out["time"].append(line)
        progress(line)

    # does it help: the record's tight pool, rebuilt
    n = 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(n, seed=7)
    env.terminate()
    solved16 = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    M_new = int(solved16["solution_len"][solved16["solved"]].float().median())
    tight = T.tighten_pool(rows, pieces, solved16["solved"], solved16["solution_len"], M_new)

    def result(e, wins):
        p = wins / max(e, 1)
        return dict(episodes=int(e), wins=int(wins), win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(e, 1)) ** 0.5, 6))

    def play(pool, M_pool, w, **kw):
        env = T.BatchedTetris(L_, M_pool, 1 << 14, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=pool)
        got = T.evaluate_heuristic(env, w, None, 16 * (M_pool + 1), **kw)
        env.terminate()
        return result(int(got["episodes"][0]), int(got["wins"][0]))

    both = lambda pool, M_pool, w: dict(one_ply=play(pool, M_pool, w), beam_3x8=play(pool, M_pool, w, depth=3, width=8))
    out["tight"] = dict(M_new=M_new, size=int(tight[0].shape[0]), of=n, classical=both(tight, M_new, T.CLASSICAL_WEIGHTS))
    progress(out["tight"])
    tune = dict(population=population, boards_per_member=per, generations=generations, seed=5, device=dev, init_std=1.0, noise=0.05)
    tuned12 = T.tune_heuristic(L_, M_new, tight, init_mean=T.CLASSICAL_WEIGHTS, **tune)
    tuned14 = T.tune_heuristic(L_, M_new, tight, init_mean=classical14, features=14, **tune)
    out["tune"] = dict(tune, device=None, tuned12=[round(float(x), 4) for x in tuned12["best"]], tuned12_fitness=tuned12["best_fitness"],
                       tuned14=[round(float(x), 4) for x in tuned14["best"]], tuned14_fitness=tuned14["best_fitness"])
    progress(out["tune"])
    players = dict(dellacherie=T.DELLACHERIE_WEIGHTS, tuned12=tuned12["best"], tuned14=tuned14["best"])
    for name, w in players.items():
        out["tight"][name] = both(tight, M_new, w)
        progress({name: out["tight"][name]})
    for name, w in dict(players, classical=T.CLASSICAL_WEIGHTS).items():
        out["full"][name] = both((rows, pieces), M_, w)
        progress({"full_" + name: out["full"][name]})
    share = lambda x: round(float(x.float().mean()), 5)
    for W in (1, 8, 16):
        line = {}
        for name, w in (("classical", T.CLASSICAL_WEIGHTS), ("tuned14", tuned14["best"])):
            found = T.solve_configs(rows, pieces, L_, M_, w, W, device=dev, validate=False)
            line[name] = dict(solved=share(found["solved"]), mean_len=round(float(found["solution_len"][found["solved"]].float().mean()), 2))
        out["solver"][f"w{W}"] = line
    progress(out["solver"])
    out["not_measured"] = "other seeds, other M_new, other tuning budgets"
    return out


def part_bound(rounds=5):
    """The move bound (include/tpl_learn.h): what the bounded kernels cost beside their twins in the same run, what the prune and the
    spare term do for the players on the tight pool of part_solve (carved L = 10 / M = 40, 65,536 configurations, seed 7, solved at
    width 16, tighten_pool(M_new=16)), and what the bounded solver proves on the carved pool at budgets of config_bound + s.  One seed
    and one pool."""
    import numpy as np
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    L_, M_ = 10, 40
    share = lambda x: round(float(x.float().mean()), 5)
    median = lambda ts: sorted(ts)[len(ts) // 2]
    out = dict(part="bound", time=dict(solve=[], beam=[]), tight={}, solver=[])

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    classical = np.array(T.CLASSICAL_WEIGHTS)
    # the tuned rows as profiles/learner/README.md prints them, to four decimals
    tuned12 = np.array([0.7636, 9.9996, -10.2889, -2.1088, 0.0836, -1.2467, -0.65, -0.5988, -2.9422, -0.2366, -1.9736, -0.847], np.float32)
    tuned14 = np.array([-0.2654, 10.3718, -11.7624, -2.251, -0.1728, 0.3929, 0.325, -1.3091, -1.6597, -0.9162, -1.5434, -1.832, -0.9158,
                        0.2822], np.float32)
    players = dict(classical=classical, dellacherie=np.array(T.DELLACHERIE_WEIGHTS), tuned12=tuned12, tuned14=tuned14)

    # 1. the solver on the carved pool at M = config_bound + s and at M = 40, bounded and plain
    n = 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces, _, carved_len = env.carved_configs(n, seed=7, with_solutions=True)
    env.terminate()
    need = T.config_bound(rows, L_, device=dev)
    out["pool"] = dict(size=n, seed=7, L=L_, M=M_, config_bound_equals_carving_len=share(need == carved_len),
                       config_bound_mean=round(float(need.float().mean()), 2))
    for slack in (0, 1, 2, None):
        budget = torch.full_like(need, M_) if slack is None else torch.clamp(need + slack, max=M_)
        for W in (1, 8, 16, 64):
            line = dict(budget="M = 40" if slack is None else f"config_bound + {slack}", width=W)
            for form in ("plain", "bounded"):
                solved, length, complete = (torch.zeros(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                                            torch.zeros(n, dtype=torch.bool, device=dev))
                for b in torch.unique(budget).tolist():
                    at = torch.nonzero(budget == b).flatten()
                    got = T.solve_configs(rows[at], pieces[at][:, :b + 1].contiguous(), L_, b, width=W, device=dev, validate=False,
                                          bound=form == "bounded")
                    solved[at], length[at] = got["solved"], got["solution_len"]
                    if form == "bounded":
                        complete[at] = got["complete"]
                line[form] = dict(solved=share(solved), mean_len=round(float(length[solved].float().mean()), 2) if bool(solved.any()) else None)
                if form == "bounded":
                    optimal = solved & ((length == need) | complete)
                    line[form].update(complete=share(complete), optimal=share(optimal), proved_unwinnable=share(~solved & complete))
            out["solver"].append(line)
            progress(line)

    # 2. the tight pool of the record, and the players on it
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    M_new = 16
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], M_new)
    tight_need = T.config_bound(tight[0], L_, device=dev)
    out["tight"] = dict(M_new=M_new, size=int(tight[0].shape[0]), of=n, config_bound_mean=round(float(tight_need.float().mean()), 2),
                        share_with_config_bound_16=share(tight_need == 16), players={})

    def result(e, wins):
        p = wins / max(e, 1)
        return dict(episodes=int(e), wins=int(wins), win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(e, 1)) ** 0.5, 6))

    def play(w, depth, width, **kw):
        env = T.BatchedTetris(L_, M_new, 1 << 14, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=tight)
        got = T.evaluate_heuristic(env, w, None, 16 * (M_new + 1), depth=depth, width=width, **kw)
        env.terminate()
        return result(int(got["episodes"][0]), int(got["wins"][0]))

    out["tight"]["classical_one_ply_as_the_record_plays_it"] = play(classical, 1, None)
    out["tight"]["classical_beam_3x8_as_the_record_plays_it"] = play(classical, 3, 8)
    progress(out["tight"])
    for name, w in players.items():
        got = {}
        for depth, width in ((1, 1), (3, 8)):
            for label, kw in (("off", {}), ("on", dict(bound=True)), ("on_spare_0.25", dict(bound=True, spare_weight=0.25)),
                              ("on_spare_1", dict(bound=True, spare_weight=1.0))):
                got[f"beam_{depth}x{width}_{label}"] = play(w, depth, width, **kw)
        out["tight"]["players"][name] = got
        progress({name: {k: v["win_rate"] for k, v in got.items()}})

    # 3. time: every bounded kernel against its own twin in the same run, alternated
    count = 1 << 20
    env = T.BatchedTetris(L_, M_, count, device=dev, seed=7, auto_reset=False, assign="sequential")
    rows, pieces = env.carved_configs(count, seed=7)
    env.load_configs(rows, pieces, validate=False)
    env.reset()
    lib, stream = T._learn_lib.lib(), torch._C._cuda_getCurrentRawStream(0)
    outs = (torch.empty(count, dtype=torch.uint8, device=dev), torch.empty(count, dtype=torch.int32, device=dev),
            torch.empty((count, M_), dtype=torch.uint8, device=dev), torch.empty(count, dtype=torch.int32, device=dev),
            torch.empty(count, dtype=torch.uint8, device=dev))
    for F, w in ((12, classical), (14, players["dellacherie"])):
        wt = torch.from_numpy(T._learn_lib.padded_weights(w)).to(dev)
        head = (rows.data_ptr(), pieces.data_ptr(), count, L_, M_, wt.data_ptr())
        o = [x.data_ptr() for x in outs]
        for W in (8, 16, 64):
            twin = lambda: T._learn_lib.check(T._learn_lib.entry("solve", F)(*head, W, o[0], o[1], o[2], None, stream))
            mine = lambda: T._learn_lib.check(T._learn_lib.entry("solve", F, True)(*head, W, 0.0, o[0], o[1], o[2], None, o[3], o[4], stream))
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(_timed(twin, 1, warmup=1))
                tb.append(_timed(mine, 1, warmup=1))
            line = dict(kernel="solve", features=F, width=W, configurations=count, M=M_, twin_ms=round(median(ta) * 1e3, 3),
                        bounded_ms=round(median(tb) * 1e3, 3), ratio=round(median(tb) / median(ta), 4))
            out["time"]["solve"].append(line)
            progress(line)
        action = torch.empty(count, dtype=torch.uint8, device=dev)
        for depth, width in ((1, 1), (3, 8), (6, 16)):
            twin, mine = T.BeamPolicy(env, w, depth, width), T.BeamPolicy(env, w, depth, width, bound=True)
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(_timed(lambda: twin.act(out=action), 2, warmup=1))
                tb.append(_timed(lambda: mine.act(out=action), 2, warmup=1))
            line = dict(kernel="beam", features=F, depth=depth, width=width, boards=count, twin_ms=round(median(ta) * 1e3, 3),
                        bounded_ms=round(median(tb) * 1e3, 3), ratio=round(median(tb) / median(ta), 4))
            out["time"]["beam"].append(line)
            progress(line)
    env.terminate()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines()
                     if any(k in l for k in ("placement_solve", "placement_beam", "move_bound"))]
    out["scratch_bytes_over_every_kernel"] = sum(int(l.split()[l.split().index("scratch") - 1]) for l in res.stdout.splitlines() if " scratch " in l)
    out["note"] = "fresh boards at M = 40 have no dead child for many plies: the time ratios are the cost of the bound, not the gain of the prune"
    return out


def part_exact(slice_size=4096, minute=60.0):
    """The exact depth-first solver (include/tpl_learn.h: tpl_placement_exact) on the record's pool (carved L = 10 / M = 40, 65,536
    configurations, seed 7) at budgets of config_bound + 0, 1, 2 and max_nodes 2^12, 2^16 and 2^20: the shares proved, solved and proved
    unwinnable, the nodes, the time and the nodes a second, with the bounded beam at widths 16 and 64 beside it in the same run.  The
    2^20 leg runs on the whole pool only if the 2^16 leg at the same budget says that it would take about a minute at most (sixteen
    times as long at the worst); otherwise on the pool's first `slice_size` configurations.  One seed, one pool, one weight row."""
    import numpy as np
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    L_, M_ = 10, 40
    share = lambda x: round(float(x.float().mean()), 5)
    out = dict(part="exact", exact=[], beam=[], of_what_width_64_left_unsolved=[])

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    n = 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces, _, carved_len = env.carved_configs(n, seed=7, with_solutions=True)
    env.terminate()
    need = T.config_bound(rows, L_, device=dev)
    out["pool"] = dict(size=n, seed=7, L=L_, M=M_, weights="classical", config_bound_equals_carving_len=share(need == carved_len),
                       config_bound_mean=round(float(need.float().mean()), 2))

    def grouped(budget, count, search):
        """`search` on the first `count` configurations, grouped by budget: its dict's entries gathered, and the seconds it took."""
        got = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in torch.unique(budget[:count]).tolist():
            at = torch.nonzero(budget[:count] == b).flatten()
            part = search(rows[at], pieces[at][:, :b + 1].contiguous(), b)
            for k, v in part.items():
                if v.dim() == 1:
                    got.setdefault(k, torch.zeros(count, dtype=v.dtype, device=dev))[at] = v
        torch.cuda.synchronize()
        return got, time.perf_counter() - t0

    beam_solved = {}
    for slack in (0, 1, 2):
        budget = torch.clamp(need + slack, max=M_)
        for W in (16, 64):
            got, seconds = grouped(budget, n, lambda r, p, b: T.solve_configs(r, p, L_, b, width=W, device=dev, validate=False, bound=True))
            line = dict(budget=f"config_bound + {slack}", width=W, configurations=n, solved=share(got["solved"]),
                        complete=share(got["complete"]), optimal=share(got["optimal"]),
                        proved_unwinnable=share(~got["solved"] & got["complete"]), seconds=round(seconds, 3))
            beam_solved[(slack, W)] = got["solved"]
            out["beam"].append(line)
            progress(line)
        last = None
        for log2 in (12, 16, 20):
            count = n
            if log2 == 20 and (last is None or last * 16 > minute):
                count = slice_size
            got, seconds = grouped(budget, count, lambda r, p, b: T.prove_configs(r, p, L_, b, max_nodes=1 << log2, device=dev,
                                                                                  validate=False))
            nodes = got["nodes"].double()
            line = dict(budget=f"config_bound + {slack}", max_nodes=f"2^{log2}", configurations=count, proved=share(got["proved"]),
                        solved=share(got["solved"]), unwinnable=share(got["unwinnable"]), nodes_mean=round(float(nodes.mean()), 1),
                        nodes_max=int(nodes.max()), seconds=round(seconds, 3), nodes_per_second=round(float(nodes.sum()) / seconds, 1),
                        solution_len_equals_config_bound=share(got["solution_len"][got["solved"]] == need[:count][got["solved"]])
                        if bool(got["solved"].any()) else None)
            last = seconds if log2 == 16 else last
            out["exact"].append(line)
            progress(line)
            left = ~beam_solved[(slack, 64)][:count]
            if bool(left.any()):
                line = dict(budget=f"config_bound + {slack}", max_nodes=f"2^{log2}", configurations=count,
                            unsolved_at_width_64=share(left), of_them_solved_and_proved_shortest=share(got["optimal"][left]),
                            of_them_proved_unwinnable=share(got["unwinnable"][left]), of_them_not_proved=share(~got["proved"][left]))
                out["of_what_width_64_left_unsolved"].append(line)
                progress(line)
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "placement_exact" in l]
    out["not_measured"] = ("other weight rows and spare_weight other than 0; shortest=False; max_nodes above 2^20; pools other than this one; "
                           "the kernel's time against a launch bound other than eight waves a SIMD; the idle lanes and a transposition table "
                           "are not built")
    return out


def part_limited(sections=("proofs", "cost", "searching_out", "wins"), rounds=3, boards=4096):
    """The exact searches in limited-discrepancy order (include/tpl_learn.h: tpl_placement_exact_limited) beside the plain kernels in
    the same run, under the classical weights and under part ntuple_exact's "feat+spare, rate 8, tight pool" table, made here by its
    recipe.  Sections: proofs (part exact's pool at config_bound + 0, 2^12 and 2^16 nodes), cost (nodes a second of every limited
    kernel against its twin, alternated rounds), searching_out (budgets that hold no win) and wins (part window's tight pool, 4,096
    boards, 1,088 steps).  One seed, one pool."""
    import numpy as np
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    L_, M_, M_new = 10, 40, 16
    share = lambda x: round(float(x.float().mean()), 5)
    out = dict(part="limited", sections=list(sections))

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    n = 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(n, seed=7)
    env.terminate()
    need = T.config_bound(rows, L_, device=dev)
    budget = torch.clamp(need, max=M_)
    groups = [(b, torch.nonzero(budget == b).flatten()) for b in torch.unique(budget).tolist()]
    groups = [(b, at, rows[at], pieces[at][:, :b + 1].contiguous()) for b, at in groups]
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], M_new)
    classical = np.array(T.CLASSICAL_WEIGHTS)

    # the table of the record: part ntuple_exact's "feat+spare, rate 8, tight pool", by its recipe
    env = T.BatchedTetris(L_, M_new, 4096, device=dev, seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=tight)
    learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, rate=8.0, shape="feat+spare", bound=False)
    for steps in (10000, 30000):
        learner.train(steps)
    one = learner.evaluate(12288, bound=False)
    table = learner.table.clone()
    env.terminate()
    out["table"] = dict(table="feat+spare, rate 8, tight pool", one_ply_win_rate_on_its_pool=round(one["win_rate"], 5),
                        order="gamma 1, reward (1, 10, -1): the training's")
    progress(out["table"])
    ordered = dict(gamma=1.0, reward=NTUPLE_LARGE_REWARD)

    def grouped(search, count=n):
        got = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b, at, r, p in groups:
            keep = at < count
            if not bool(keep.any()):
                continue
            for k, v in search(r[keep], p[keep], b).items():
                if v.dim() == 1:
                    got.setdefault(k, torch.zeros(n, dtype=v.dtype, device=dev))[at[keep]] = v
        torch.cuda.synchronize()
        return {k: v[:count] for k, v in got.items()}, time.perf_counter() - t0

    def prove(rule, log2, first=0, **kw):
        """A root search of the pool under a weight row: plain (rule None) or limited."""
        if rule is None:
            return lambda r, p, b: T.prove_configs(r, p, L_, b, max_nodes=1 << log2, device=dev, validate=False, **kw)
        return lambda r, p, b: T.prove_configs_limited(r, p, L_, b, rule, first, max_nodes=1 << log2, device=dev, validate=False, **kw)

    def prove_tabled(tab, rule, log2, first=0):
        if rule is None:
            return lambda r, p, b: T.ntuple_prove_configs(r, p, L_, b, tab, max_nodes=1 << log2, device=dev, validate=False, **ordered)
        return lambda r, p, b: T.ntuple_prove_configs_limited(r, p, L_, b, tab, rule, first, max_nodes=1 << log2, device=dev,
                                                              validate=False, **ordered)

    if "proofs" in sections:
        beam, _ = grouped(lambda r, p, b: T.solve_configs(r, p, L_, b, width=64, device=dev, validate=False, bound=True))
        left = ~beam["solved"]
        out["pool"] = dict(size=n, seed=7, L=L_, M=M_, budget="config_bound + 0", unsolved_at_width_64=share(left))
        out["proofs"] = []
        record = {("classical weights", 12): 0.350, ("classical weights", 16): 0.650, ("feat+spare table", 12): 0.453,
                  ("feat+spare table", 16): 0.750}
        for label, make in (("classical weights", prove), ("feat+spare table", lambda rule, log2: prove_tabled(table, rule, log2))):
            for log2 in (12, 16):
                base = None
                for rule in (None, "add", "double"):
                    got, seconds = grouped(make(rule, log2))
                    nodes = got["nodes"].double()
                    line = dict(ordering=label, order=rule or "plain", max_nodes=f"2^{log2}", proved=share(got["proved"]),
                                solved=share(got["solved"]), unwinnable=share(got["unwinnable"]),
                                of_what_width_64_left_unsolved_closed=share(got["optimal"][left]),
                                nodes_mean=round(float(nodes.mean()), 1), seconds=round(seconds, 3),
                                nodes_per_second=round(float(nodes.sum()) / seconds, 1))
                    if rule is None:
                        base = got
                        line["reproduces_the_record"] = round(line["proved"], 3) == record[(label, log2)]
                    else:
                        both = base["proved"] & got["proved"]
                        line.update(plain_proofs_kept=share(got["proved"][base["proved"]]), limit_max=int(got["limit"].max()),
                                    limit_mean_of_proved=round(float(got["limit"][got["proved"]].float().mean()), 2),
                                    same_length_where_both_proved=bool((base["solution_len"][both] == got["solution_len"][both]).all()))
                    out["proofs"].append(line)
                    progress(line)

    if "cost" in sections:
        # nodes a second of every limited kernel beside its twin at 2^12 nodes, the legs alternated, the median of the rounds after a
        # warm-up round: the root kernels on the pool's first 16,384, the window kernels on 4,096 boards of the tight pool in mid-game
        count, log2 = 1 << 14, 12
        w14 = np.array(T.DELLACHERIE_WEIGHTS)
        zero = {form: torch.zeros(T._learn_lib.ntuple_entries_of(form), dtype=torch.int32, device=dev) for form in ("2x4", "3x3", "feat")}
        tables = dict(zero, **{"feat+spare": table})
        env = T.BatchedTetris(L_, M_new, boards, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=tight)
        env.reset()
        player = T.HeuristicPolicy(env, classical)
        for _ in range(40):
            env.step(player.act(), observe=False)

        def window(rule, first, **kw):
            if rule is None:
                return lambda: T.window_prove(env, max_nodes=1 << log2, **kw)
            return lambda: T.window_prove_limited(env, rule, first, max_nodes=1 << log2, **kw)

        def window_tabled(tab, rule, first):
            if rule is None:
                return lambda: T.ntuple_window_prove(env, tab, max_nodes=1 << log2, **ordered)
            return lambda: T.ntuple_window_prove_limited(env, tab, rule, first, max_nodes=1 << log2, **ordered)

        def once(search):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = search()
            torch.cuda.synchronize()
            return got, time.perf_counter() - t0

        root = lambda make: (lambda rule, first: (lambda s=make(rule, first): grouped(s, count)))
        flat = lambda make: (lambda rule, first: (lambda s=make(rule, first): once(s)))
        kernels = {"tpl_placement_exact": root(lambda rule, first: prove(rule, log2, first)),
                   "tpl_placement_exact_move": root(lambda rule, first: prove(rule, log2, first, weights=w14))}
        for form, tab in tables.items():
            kernels[f"tpl_ntuple_exact, {form!r}"] = root(lambda rule, first, tab=tab: prove_tabled(tab, rule, log2, first))
        kernels["tpl_placement_window_prove"] = flat(lambda rule, first: window(rule, first))
        kernels["tpl_placement_window_prove_move"] = flat(lambda rule, first: window(rule, first, weights=w14))
        for form, tab in tables.items():
            kernels[f"tpl_ntuple_window_prove, {form!r}"] = flat(lambda rule, first, tab=tab: window_tabled(tab, rule, first))
        out["cost"] = dict(max_nodes=f"2^{log2}", rounds=rounds, root_configurations=count, window_boards=boards,
                           tables='"feat+spare": the trained table; the three other forms: zero tables, whose order is the reward alone', rows=[])
        for name, make in kernels.items():
            legs = {"plain": make(None, 0), "limited_65535": make("add", 65535), "limited_0_add": make("add", 0),
                    "limited_0_double": make("double", 0)}
            rate = {k: [] for k in legs}
            for _ in range(rounds + 1):
                for k, run in legs.items():
                    got, seconds = run()
                    rate[k].append(float(got["nodes"].double().sum()) / seconds)
            med = {k: float(np.median(v[1:])) for k, v in rate.items()}
            line = dict(kernel=name, nodes_per_second={k: round(v, 1) for k, v in med.items()},
                        limited_65535_over_plain=round(med["limited_65535"] / med["plain"], 4),
                        limited_0_add_over_plain=round(med["limited_0_add"] / med["plain"], 4))
            out["cost"]["rows"].append(line)
            progress(line)
        env.terminate()

    if "searching_out" in sections:
        # The record's pool is carved, so at config_bound + 0 the first budget searched is the shortest length: it has no budget without a
        # win.  generate_configs(3, 8) boards searched for four lines in six moves have.
        g_rows, g_pieces = T.generate_configs(3, 8, 4096, seed=7)
        g_pieces = np.ascontiguousarray(g_pieces[:, :7])
        base = T.prove_configs(g_rows, g_pieces, 4, 6, max_nodes=1 << 20, device=dev)
        at = base["unwinnable"] & (base["nodes"] > 0)
        out["searching_out"] = dict(record_pool="none: carved configurations at their exact budget are all winnable, and the first budget "
                                    "searched is the shortest length", boards="generate_configs(3, 8, 4096, seed 7) searched for 4 lines in 6 moves",
                                    max_nodes="2^20", proved_without_a_win=int(at.sum()),
                                    plain_nodes_mean=round(float(base["nodes"][at].double().mean()), 1))
        for rule in ("add", "double"):
            got = T.prove_configs_limited(g_rows, g_pieces, 4, 6, rule, 0, max_nodes=1 << 20, device=dev)
            ratio = got["nodes"][at].double() / base["nodes"][at].double()
            total = float(got["nodes"][at].double().sum() / base["nodes"][at].double().sum())
            out["searching_out"][rule] = dict(still_proved_without_a_win=share(got["unwinnable"][at]), nodes_over_plain_total=round(total, 3),
                                              nodes_over_plain_max=round(float(ratio.max()), 2), limit_max=int(got["limit"][at].max()))
        progress(out["searching_out"])

    if "wins" in sections:                                     # part window's and part ntuple_window's set-up
        steps = 16 * (M_new + 1) * (1 << 14) // boards
        out["wins"] = dict(pool=dict(size=int(tight[0].shape[0]), L=L_, M=M_new), boards=boards, steps=steps, reuse=True, rows=[])
        record = {("classical weights", "one_ply", 8): 0.617, ("classical weights", "one_ply", 12): 0.738,
                  ("classical weights", "beam_3x8", 8): 0.865, ("classical weights", "beam_3x8", 12): 0.910,
                  ("feat+spare table", "one_ply", 8): 0.673, ("feat+spare table", "one_ply", 12): 0.774}
        for label, order in (("classical weights", {}), ("feat+spare table", dict(ordered, table=table))):
            for name, depth, width in (("one_ply", 1, None), ("beam_3x8", 3, 8)):
                for log2 in (8, 12):
                    for rule in (None, "add"):
                        env = T.BatchedTetris(L_, M_new, boards, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=tight)
                        env.reset()
                        base_policy = T.HeuristicPolicy(env, classical, depth=depth) if width is None else \
                            T.BeamPolicy(env, classical, depth, width)
                        limited = {} if rule is None else dict(discrepancy=rule)
                        player = T.ProofPolicy(env, base_policy, max_nodes=1 << log2, reuse=True, **order, **limited)
                        action = torch.empty(boards, dtype=torch.uint8, device=dev)
                        reward = torch.empty(boards, dtype=torch.float32, device=dev)
                        done = torch.empty(boards, dtype=torch.uint8, device=dev)
                        tallies = torch.zeros(4, dtype=torch.int64, device=dev)   # episodes, wins, episodes with a proof, broken proofs
                        held = torch.zeros(boards, dtype=torch.bool, device=dev)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(steps):
                            player.act(out=action)
                            held |= player.played
                            env.step_into(action, reward, done)
                            over, won = done.bool(), reward == 1.0
                            tallies += torch.stack([over.sum(), (over & won).sum(), (over & held).sum(), (over & held & ~won).sum()])
                            held &= ~over
                        torch.cuda.synchronize()
                        seconds = time.perf_counter() - t0
                        e, w, with_proof, broken = tallies.tolist()
                        env.terminate()
                        rate = w / max(e, 1)
                        line = dict(ordering=label, base=name, max_nodes=f"2^{log2}", order=rule or "plain", episodes=e, wins=w,
                                    win_rate=round(rate, 5), standard_error=round((rate * (1 - rate) / max(e, 1)) ** 0.5, 6),
                                    episodes_that_held_a_verdict_1=with_proof, of_them_not_won=broken,
                                    ms_per_step=round(seconds * 1e3 / steps, 3), stats=player.stats())
                        if rule is None and (label, name, log2) in record:
                            line["reproduces_the_record"] = round(rate, 3) == record[(label, name, log2)]
                        out["wins"]["rows"].append(line)
                        progress(line)
                        if broken:                              # a bug to fix before anything is recorded
                            raise RuntimeError(f"{broken} episodes held a verdict 1 and did not end won: {line}")
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "_limited_kernel" in l]
    out["not_measured"] = ("first limits other than 0 and 65,535; trained tables of the forms other than \"feat+spare\"; \"double\" in play; "
                           "pools other than this one; more than one seed")
    return out


def part_labels(boards=4096, log2_nodes=12):
    """The proved move labels (include/tpl_learn.h: tpl_placement_exact_labels; T.label_states) on the tight pool of the record --
    part_bound's: carved L = 10 / M = 40, 65,536 configurations, seed 7, solved at width 16, tighten_pool(M_new=16).  The classical
    weights at one ply and at beam (3, 8) play one episode each on `boards` boards without auto-reset, label_states before every
    step with max_nodes = 2^log2_nodes a child.  One seed, one pool, one weight row."""
    import numpy as np
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    L_, M_, M_new = 10, 40, 16
    share = lambda x: round(float(x.float().mean()), 5) if x.numel() else None
    out = dict(part="labels", boards=boards, max_nodes=f"2^{log2_nodes}", players={})

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    n = 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(n, seed=7)
    env.terminate()
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], M_new)
    out["pool"] = dict(size=int(tight[0].shape[0]), of=n, seed=7, L=L_, M=M_new, weights="classical")
    classical = np.array(T.CLASSICAL_WEIGHTS)
    canon = torch.from_numpy(np.stack([T._learn_lib.canonical_actions(p, np.arange(40)) for p in range(8)]).astype(np.int64)).to(dev)

    # the root search of the same pool in the same run: the rate the labels' searches stand beside
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    roots = T.prove_configs(tight[0], tight[1], L_, M_new, max_nodes=1 << log2_nodes, device=dev, validate=False)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    out["prove_configs"] = dict(configurations=int(tight[0].shape[0]), proved=share(roots["proved"]), solved=share(roots["solved"]),
                                seconds=round(seconds, 3), nodes_per_second=round(float(roots["nodes"].double().sum()) / seconds, 1))
    progress(out["prove_configs"])

    for name, depth, width in (("one_ply", 1, 1), ("beam_3x8", 3, 8)):
        env = T.BatchedTetris(L_, M_new, boards, device=dev, seed=11, auto_reset=False, reward=(0.0, 1.0, 0.0), config_pool=tight)
        env.reset()
        policy = T.BeamPolicy(env, classical, depth, width)
        action = torch.empty(boards, dtype=torch.uint8, device=dev)
        first = torch.full((boards,), -1, dtype=torch.int64, device=dev)          # the move number of a board's first proved blunder
        open_before = torch.zeros(boards, dtype=torch.bool, device=dev)           # an unproved move met before it (or ever)
        moves, nodes, spent = [], 0.0, 0.0
        for t in range(M_new):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lab = T.label_states(env, tight[1], weights=classical, max_nodes=1 << log2_nodes)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            running = lab["running"]
            policy.act(out=action)
            cur = env.packed_state()["cur"].to(torch.int64) & 7
            taken = canon[cur, action.to(torch.int64).clamp(max=39)]
            blunder = T.blunders(lab["label"], taken).bool() & running
            proved_all = ~(lab["label"] == 3).any(dim=1)
            first = torch.where((first < 0) & blunder, torch.full_like(first, t), first)
            open_before |= running & ~proved_all & (first < 0)
            count = float(lab["nodes"].double().sum())
            nodes, spent = nodes + count, spent + ms * 1e-3
            line = dict(move=t, running=int(running.sum()), every_move_proved=share(proved_all[running]),
                        has_a_proved_winning_move=share(lab["winning"].any(dim=1)[running]), blunder_rate=share(blunder[running]),
                        took_an_unproved_move=share((torch.gather(lab["label"], 1, taken[:, None])[:, 0] == 3)[running]),
                        label_states_ms=round(ms, 2), nodes=int(count))
            moves.append(line)
            progress({name: line})
            env.step(action, observe=False)
        won = env.state == 1
        lost = ~won
        got = dict(per_move=moves, win_rate=share(won), lost_episodes=int(lost.sum()),
                   lost_with_a_proved_first_blunder=share((first >= 0)[lost]),
                   lost_with_a_proved_first_blunder_and_every_earlier_move_proved=share(((first >= 0) & ~open_before)[lost]),
                   won_with_a_proved_blunder=share((first >= 0)[won]),
                   first_blunder_move_histogram=torch.bincount(first[first >= 0], minlength=M_new).tolist(),
                   label_states_ms_mean=round(spent * 1e3 / M_new, 2), nodes_per_second=round(nodes / spent, 1))
        env.terminate()
        out["players"][name] = got
        progress({name: {k: v for k, v in got.items() if k != "per_move"}})
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "placement_exact" in l]
    out["not_measured"] = ("other weight rows, the fourteen features and spare_weight other than 0; max_nodes other than this one; other pools and "
                           "seeds; learners; label_states' time includes the state export, config_index and the host's launch, not the kernel alone")
    return out


def part_ntuple_exact(rounds=5):
    """The table-ordered exact search (include/tpl_learn.h: tpl_ntuple_exact) on part exact's pool, every configuration at its exact
    budget (config_bound + 0), beside tpl_placement_exact under the classical weights in the same run.  One seed, one pool."""
    import torch
    import tetris_piclim as T
    dev = "cuda:0"
    L_, M_, n = 10, 40, 1 << 16
    share = lambda x: round(float(x.float().mean()), 5)
    out = dict(part="ntuple_exact", runs=[], two_by_two=[], kernel_cost=[])

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(n, seed=7)
    env.terminate()
    need = T.config_bound(rows, L_, device=dev)
    budget = torch.clamp(need, max=M_)
    groups = [(b, torch.nonzero(budget == b).flatten()) for b in torch.unique(budget).tolist()]
    groups = [(b, at, rows[at], pieces[at][:, :b + 1].contiguous()) for b, at in groups]

    def grouped(search):
        """`search` on the pool grouped by budget: its dict's entries gathered, and the seconds it took."""
        got = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b, at, r, p in groups:
            for k, v in search(r, p, b).items():
                if v.dim() == 1:
                    got.setdefault(k, torch.zeros(n, dtype=v.dtype, device=dev))[at] = v
        torch.cuda.synchronize()
        return got, time.perf_counter() - t0

    beam, _ = grouped(lambda r, p, b: T.solve_configs(r, p, L_, b, width=64, device=dev, validate=False, bound=True))
    left = ~beam["solved"]
    out["pool"] = dict(size=n, seed=7, L=L_, M=M_, budget="config_bound + 0", config_bound_mean=round(float(need.float().mean()), 2),
                       unsolved_at_width_64=share(left))

    # the tables of the record: part ntuple_budget_sweep's runs, 40,000 steps each
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], 16)

    def learn(pool, M_pool, **kw):
        env = T.BatchedTetris(L_, M_pool, 4096, device=dev, seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=pool)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, rate=8.0, **kw)
        for steps in (10000, 30000):
            learner.train(steps)
        one = learner.evaluate(12288, bound=kw.get("bound", False))
        table = learner.table.clone()
        env.terminate()
        return table, round(one["win_rate"], 5)

    tables = {}
    for label, pool, M_pool, kw in (("feat, rate 8, loose pool", (rows, pieces), M_, dict(shape="feat")),
                                    ("feat+spare, rate 8, tight pool", tight, 16, dict(shape="feat+spare", bound=False)),
                                    ("feat+spare, rate 8, tight pool, trained with the prune", tight, 16, dict(shape="feat+spare", bound=True))):
        tables[label], rate = learn(pool, M_pool, **kw)
        progress(dict(table=label, one_ply_win_rate_on_its_pool=rate))
        out.setdefault("tables", []).append(dict(table=label, one_ply_win_rate_on_its_pool=rate))

    def line(label, log2, got, seconds):
        nodes = got["nodes"].double()
        return dict(ordering=label, max_nodes=f"2^{log2}", proved=share(got["proved"]), solved=share(got["solved"]),
                    nodes_mean=round(float(nodes.mean()), 1), seconds=round(seconds, 3),
                    nodes_per_second=round(float(nodes.sum()) / seconds, 1),
                    of_unsolved_at_width_64_proved=share(got["proved"][left]), of_them_solved=share(got["solved"][left]))

    record = {12: 0.350, 16: 0.650}
    for log2 in (12, 16):
        classical, seconds = grouped(lambda r, p, b: T.prove_configs(r, p, L_, b, max_nodes=1 << log2, device=dev, validate=False))
        got = line("classical weights", log2, classical, seconds)
        got["reproduces_the_record"] = round(got["proved"], 3) == record[log2]
        out["runs"].append(got)
        progress(got)
        for label, table in tables.items():
            mine, seconds = grouped(lambda r, p, b: T.ntuple_prove_configs(r, p, L_, b, table, gamma=1.0, reward=NTUPLE_LARGE_REWARD,
                                                                           max_nodes=1 << log2, device=dev, validate=False))
            got = line(label, log2, mine, seconds)
            out["runs"].append(got)
            progress(got)
            a, b = classical["proved"], mine["proved"]
            both = a & b
            cell = dict(ordering=label, max_nodes=f"2^{log2}", both=int(both.sum()), classical_only=int((a & ~b).sum()),
                        table_only=int((~a & b).sum()), neither=int((~a & ~b).sum()),
                        verdicts_and_lengths_equal_where_both_prove=bool(torch.equal(classical["solved"][both], mine["solved"][both]) and
                                                                         torch.equal(classical["solution_len"][both], mine["solution_len"][both])))
            out["two_by_two"].append(cell)
            progress(cell)

    # the kernels: nodes a second at 2^12 nodes beside the twin, alternated; the window forms under random tables in +-2^18
    gen = torch.Generator(device=dev).manual_seed(5)
    forms = {"feat": tables["feat, rate 8, loose pool"], "feat+spare": tables["feat+spare, rate 8, tight pool"]}
    for shape in ("2x4", "3x3"):
        forms[shape] = torch.randint(-(1 << 18), (1 << 18) + 1, (T._learn_lib.ntuple_entries_of(shape),), generator=gen, device=dev,
                                     dtype=torch.int32)
    rate = lambda got, seconds: float(got["nodes"].double().sum()) / seconds
    twin = lambda: grouped(lambda r, p, b: T.prove_configs(r, p, L_, b, max_nodes=1 << 12, device=dev, validate=False))
    twin()
    for shape, table in forms.items():
        search = lambda: grouped(lambda r, p, b: T.ntuple_prove_configs(r, p, L_, b, table, gamma=1.0, reward=NTUPLE_LARGE_REWARD,
                                                                        max_nodes=1 << 12, device=dev, validate=False))
        search()
        a, b = [], []
        for _ in range(rounds):
            a.append(rate(*twin()))
            b.append(rate(*search()))
        ma, mb = sorted(a)[rounds // 2], sorted(b)[rounds // 2]
        got = dict(form=shape, twin_nodes_per_second=[round(x, 1) for x in a], nodes_per_second=[round(x, 1) for x in b],
                   twin_median=round(ma, 1), median=round(mb, 1), ratio_to_the_twin=round(mb / ma, 4))
        out["kernel_cost"].append(got)
        progress(got)
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "exact" in l]
    out["not_measured"] = ("budgets above config_bound; max_nodes above 2^16; shortest=False; tables trained at other rates, other seeds and "
                           "other pools; gamma and rewards other than the training's; trained window tables (the cost rows use random "
                           "ones); a launch bound other than eight waves a SIMD")
    return out


def part_rank(rounds=5, reps=10, n=1 << 20, boards=4096, eval_boards=16384, log2_nodes=12, epochs=4, batch=1024):
    """The ranking update from proved move labels (include/tpl_learn.h: tpl_ntuple_rank; T.NTupleRanker, T.collect_labels,
    T.label_agreement).  One seed, one pool.
      time   rank() for each of the four forms beside NTuplePolicy.act() with every output, alternated, on part ntuple_shape's 2^20
             mid-game boards with label rows drawn from 0 .. 3; a whole step() beside one NTupleLearner step of the form.
      buys   the tight pool of the record (part labels'), split by pool entry into a training and a held-out half.  The rate-8
             "feat+spare" TD table of part ntuple_exact plays one episode on each half under collect_labels; fit() on the training
             half's nodes from that table and from zero; on the held-out half label_agreement, the one-ply win rate and the beam (3, 8)
             win rate before and after, and a sweep over rate and margin from the TD table."""
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    dev = "cuda:0"
    out = dict(part="rank", time=dict(boards=n, rounds=rounds, launches_per_timing=reps, forms={}), buys={})

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    # ---- time
    env, ring = _shape_ring(T, n, 2)
    del ring
    a, b = env.raw_planes()
    label = torch.randint(0, 4, (n, 40), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    action = torch.empty(n, dtype=torch.uint8, device=dev)
    score, value = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    after = tuple(torch.empty((n, 4), dtype=torch.int32, device=dev) for _ in range(2))
    for form in m.NTUPLE_RANK_FORMS:
        host = np.random.default_rng(1).integers(-(1 << 20), (1 << 20) + 1, m.ntuple_entries_of(form)).astype(np.int32)
        table = torch.from_numpy(host).to(dev)
        policy = T.NTuplePolicy(env, table, gamma=1.0, epsilon=0.0, seed=11)
        ranker = T.NTupleRanker(table.clone(), 10, 40, gamma=1.0, reward=env.reward_params, rate=1.0)
        buffers = ranker.buffers(n)
        learner = T.NTupleLearner(env, gamma=1.0, rate=1.0, epsilon=0.05, seed=11, shape=form)
        learner.table.copy_(table)
        learner.train(3)
        decided = ranker.rank((a, b), label, buffers)["win"] != 255
        calls = {"act": lambda: policy.act(out=action, score=score, after=after, value=value, step=3),
                 "rank": lambda: ranker.rank((a, b), label, buffers),
                 "learner_step": lambda: learner.train(1),
                 "rank_step": lambda: ranker.step((a, b), label, buffers)}
        times = {k: [] for k in calls}
        for pair in (("act", "rank"), ("learner_step", "rank_step")):   # alternated round by round; the learner moves the boards, so it comes last
            for _ in range(rounds):
                for k in pair:
                    times[k].append(_timed(calls[k], reps, warmup=1))
        med = {k: sorted(ts)[rounds // 2] for k, ts in times.items()}
        got = {k + "_us": _spread(ts) for k, ts in times.items()}
        got.update(decided_share=round(float(decided.float().mean()), 4), rank_over_act=round(med["rank"] / med["act"], 4),
                   step_over_learner_step=round(med["rank_step"] / med["learner_step"], 4))
        out["time"]["forms"][form] = got
        progress({form: got})
        del learner, ranker, buffers, policy
    env.terminate()
    del a, b, label, action, score, value, after
    torch.cuda.empty_cache()

    # ---- what it buys
    L_, M_, M_new, count = 10, 40, 16, 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(count, seed=7)
    env.terminate()
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], M_new)
    size = int(tight[0].shape[0])
    half = size // 2
    halves = {"train": (tight[0][:half].contiguous(), tight[1][:half].contiguous()),
              "held_out": (tight[0][half:].contiguous(), tight[1][half:].contiguous())}
    buys = out["buys"]
    buys["pool"] = dict(size=size, of=count, seed=7, L=L_, M=M_new, train_entries=half, held_out_entries=size - half,
                        label_boards=boards, episode_boards=eval_boards)

    env = T.BatchedTetris(L_, M_new, 4096, device=dev, seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=tight)
    learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, rate=8.0, shape="feat+spare", bound=False)
    for steps in (10000, 30000):
        learner.train(steps)
    buys["td_table"] = dict(form="feat+spare", rate=8.0, steps=40000, pool="the whole tight pool",
                            one_ply_win_rate_on_its_pool=round(learner.evaluate(12288)["win_rate"], 5), record=0.56785)
    td = learner.table.clone()
    env.terminate()
    progress(buys["td_table"])

    def episode(table, pool, beam=None):
        """One episode on `eval_boards` boards of `pool` without auto-reset: the share won."""
        env = T.BatchedTetris(L_, M_new, eval_boards, device=dev, seed=11, auto_reset=False, reward=NTUPLE_LARGE_REWARD, config_pool=pool)
        env.reset()
        policy = T.NTupleBeamPolicy(env, table, *beam, gamma=1.0) if beam else T.NTuplePolicy(env, table, gamma=1.0, epsilon=0.0)
        for _ in range(M_new):
            env.step(policy.act(), observe=False)
        won = round(float((env.state == 1).float().mean()), 5)
        env.terminate()
        return won

    def collect(pool):
        env = T.BatchedTetris(L_, M_new, boards, device=dev, seed=11, auto_reset=False, reward=NTUPLE_LARGE_REWARD, config_pool=pool)
        env.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = T.collect_labels(env, pool[1], T.NTuplePolicy(env, td, gamma=1.0, epsilon=0.0), M_new, max_nodes=1 << log2_nodes)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        env.terminate()
        return got, seconds

    sets = {}
    for name, pool in halves.items():
        sets[name], seconds = collect(pool)
        moves = ((sets[name].planes_a[:, 1] >> 28) & 15) | (((sets[name].planes_a[:, 3] >> 28) & 15) << 4)
        buys.setdefault("labels", {})[name] = dict(nodes=len(sets[name]), boards=boards, steps=M_new, max_nodes=f"2^{log2_nodes}",
                                                   seconds=round(seconds, 2), by_move=torch.bincount(moves.to(torch.int64), minlength=M_new).tolist())
        progress({name: buys["labels"][name]})
    held = sets["held_out"]
    kw = dict(gamma=1.0, reward=NTUPLE_LARGE_REWARD)

    def measure(table, beam=True):
        got = dict(agreement=T.label_agreement(table, (held.planes_a, held.planes_b), held.label, L_, M_new, **kw),
                   one_ply=episode(table, halves["held_out"]))
        if beam:
            got["beam_3x8"] = episode(table, halves["held_out"], (3, 8))
        return got

    def fit(start, rate, margin, epochs=epochs):
        table = start.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts = T.NTupleRanker(table, L_, M_new, rate=rate, margin=margin, **kw).fit(sets["train"], epochs, batch, seed=0)
        torch.cuda.synchronize()
        return table, counts, round(time.perf_counter() - t0, 3)

    buys["held_out"] = {"td_table": measure(td)}
    progress(buys["held_out"])
    for name, start in (("fit_from_the_td_table", td), ("fit_from_zero", torch.zeros_like(td))):
        table, counts, seconds = fit(start, 8.0, 0.0)
        buys["held_out"][name] = dict(rate=8.0, margin=0.0, epochs=epochs, batch=batch, violated_per_epoch=counts, fit_seconds=seconds,
                                      train_nodes=len(sets["train"]), **measure(table))
        progress({name: buys["held_out"][name]})
    buys["sweep_from_the_td_table"] = []
    cells = [(rate, margin, epochs) for rate in (1.0, 8.0, 64.0, 512.0, 4096.0) for margin in (0.0, 1.0, 4.0)]
    cells += [(rate, 1.0, 4 * epochs) for rate in (64.0, 512.0)]
    for rate, margin, passes in cells:
        table, counts, _ = fit(td, rate, margin, passes)
        line = dict(rate=rate, margin=margin, epochs=passes, violated_first_and_last_epoch=[counts[0], counts[-1]],
                    **measure(table, beam=passes != epochs))
        buys["sweep_from_the_td_table"].append(line)
        progress(line)
    buys["one_ply_standard_error"] = round(0.5 / eval_boards ** 0.5, 4)
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), m.build_library()], capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "ntuple_rank" in l]
    out["not_measured"] = ("other seeds and pools; more epochs, other batch sizes; bound=True; symmetric=True; the window forms as learners; "
                           "labels collected under other policies or at other max_nodes; teaching through two plies or the beam; mixing "
                           "ranking steps into TD training; the time of rank() on real label rows (the timed rows are drawn from 0 .. 3)")
    return out


def part_window(sections=("record", "rates", "verdicts", "time", "loose"), budgets=(8, 12, 16), boards=4096, rounds=5):
    """The exact search over a state's window and the proof policy (include/tpl_learn.h: tpl_placement_window_prove; T.window_prove,
    T.ProofPolicy) on the tight pool of the record -- part_bound's: carved L = 10 / M = 40, 65,536 configurations, seed 7, solved at
    width 16, tighten_pool(M_new=16) -- and once on the loose pool.  One seed, one pool, the classical weight row."""
    import numpy as np
    import torch
    import tetris_piclim as T
    _plane_fields, _resident_planes = T.solve._plane_fields, T.solve._resident_planes
    dev = "cuda:0"
    L_, M_, M_new = 10, 40, 16
    out = dict(part="window", sections=list(sections), budgets=[f"2^{b}" for b in budgets], boards=boards)

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    n = 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(n, seed=7)
    env.terminate()
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], M_new)
    out["pool"] = dict(size=int(tight[0].shape[0]), of=n, seed=7, L=L_, M=M_new, weights="classical")
    classical = np.array(T.CLASSICAL_WEIGHTS)
    bases = (("one_ply", 1, None), ("beam_3x8", 3, 8))

    def result(e, wins):
        p = wins / max(e, 1)
        return dict(episodes=int(e), wins=int(wins), win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(e, 1)) ** 0.5, 6))

    def make(game_M, pool, depth, width, log2, reuse, count=boards):
        env = T.BatchedTetris(L_, game_M, count, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=pool)
        env.reset()
        base = T.HeuristicPolicy(env, classical, depth=depth) if width is None else T.BeamPolicy(env, classical, depth, width)
        return env, base if log2 is None else T.ProofPolicy(env, base, max_nodes=1 << log2, reuse=reuse)

    def play(env, player, steps, game_M):
        """`steps` steps from the reset: episodes, wins, the episodes that held a verdict 1 and did not end won, the verdicts per move
        number (column 0: a live plan was followed, or nothing was searched), and the seconds."""
        count = env.num_envs
        action = torch.empty(count, dtype=torch.uint8, device=dev)
        reward = torch.empty(count, dtype=torch.float32, device=dev)
        done = torch.empty(count, dtype=torch.uint8, device=dev)
        tallies = torch.zeros(4, dtype=torch.int64, device=dev)           # episodes, wins, episodes with a proof, broken proofs
        per_move = torch.zeros(game_M * 4, dtype=torch.int64, device=dev)
        held = torch.zeros(count, dtype=torch.bool, device=dev)
        proof = isinstance(player, T.ProofPolicy)
        planes = _resident_planes(env)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if proof:
                moves = _plane_fields(*planes)[0].to(torch.int64)
            player.act(out=action)
            if proof:
                per_move += torch.bincount(moves * 4 + player.verdict.to(torch.int64), minlength=game_M * 4)[:game_M * 4]
                held |= player.played
            env.step_into(action, reward, done)
            over, won = done.bool(), reward == 1.0
            tallies += torch.stack([over.sum(), (over & won).sum(), (over & held).sum(), (over & held & ~won).sum()])
            held &= ~over
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        e, w, with_proof, broken = tallies.tolist()
        got = dict(result(e, w), steps=steps, seconds=round(seconds, 2), ms_per_step=round(seconds * 1e3 / steps, 3))
        if proof:
            got.update(episodes_that_held_a_verdict_1=with_proof, of_them_not_won=broken, stats=player.stats())
            got["per_move"] = per_move.view(game_M, 4).tolist()
        return got

    if "record" in sections:                                   # the record's rows as the record plays them: they must reproduce
        out["record"] = {}
        for name, depth, width in bases:
            env = T.BatchedTetris(L_, M_new, 1 << 14, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=tight)
            got = T.evaluate_heuristic(env, classical, None, 16 * (M_new + 1), depth=depth, width=width)
            env.terminate()
            out["record"][name] = result(int(got["episodes"][0]), int(got["wins"][0]))
        progress(out["record"])

    steps = 16 * (M_new + 1) * (1 << 14) // boards               # the record's episode budget on fewer boards
    if "rates" in sections:
        out["rates"] = {}
        for name, depth, width in bases:
            got = {}
            for log2 in (None,) + tuple(budgets):
                env, player = make(M_new, tight, depth, width, log2, True)
                got["base" if log2 is None else f"proof_2^{log2}"] = play(env, player, steps, M_new)
                env.terminate()
                progress({name: {k: {x: y for x, y in v.items() if x != "per_move"} for k, v in got.items()}})
            out["rates"][name] = got
        out["rates"]["feat+spare_rate_8_table"] = "skipped: no table file is kept in the repository"

    if "verdicts" in sections:                                 # reuse off: every running board is searched at every move
        out["verdicts"] = {}
        for log2 in budgets:
            env, player = make(M_new, tight, 1, None, log2, False)
            got = play(env, player, 8 * (M_new + 1), M_new)
            env.terminate()
            table = []
            for move, (none, win, loss, open_) in enumerate(got.pop("per_move")):
                total = max(none + win + loss + open_, 1)
                table.append(dict(move=move, running=total, win=round(win / total, 5), loss=round(loss / total, 5),
                                  open=round(open_ / total, 5)))
            out["verdicts"][f"2^{log2}"] = dict(got, per_move=table)
            progress({f"2^{log2}": out["verdicts"][f"2^{log2}"]})

    if "time" in sections:
        out["time"] = dict(steps=[], search=[])
        median = lambda ts: sorted(ts)[len(ts) // 2]
        for name, depth, width in bases:
            for log2 in budgets:
                arms = {}
                for arm, (b, reuse) in (("base", (None, False)), ("reuse_off", (log2, False)), ("reuse_on", (log2, True))):
                    arms[arm] = make(M_new, tight, depth, width, b, reuse)
                times = {arm: [] for arm in arms}
                for _ in range(rounds):                        # alternated: each arm plays 64 steps on from where it stands
                    for arm, (env, player) in arms.items():
                        times[arm].append(play(env, player, 64, M_new)["ms_per_step"])
                for env, _ in arms.values():
                    env.terminate()
                line = dict(base=name, max_nodes=f"2^{log2}", boards=boards, ms_per_step={a: median(t) for a, t in times.items()},
                            min={a: min(t) for a, t in times.items()})
                line["ratio_to_base"] = {a: round(line["ms_per_step"][a] / line["ms_per_step"]["base"], 3) for a in ("reuse_off", "reuse_on")}
                out["time"]["steps"].append(line)
                progress(line)
        # nodes a second: window_prove beside prove_nodes on the same boards, mid-game, alternated
        env, player = make(M_new, tight, 1, None, None, False)
        play(env, player, 40, M_new)
        state = env.packed_state()
        for log2 in budgets:
            mine = T.window_prove(env, max_nodes=1 << log2)
            H = mine["horizon"].to(torch.int64)
            lists = torch.full((boards, M_new + 1), 7, dtype=torch.uint8, device=dev)
            planes = _resident_planes(env)
            window = (planes[1][:, 3].to(torch.int64) & 0xFFFFFFFF) | (((planes[1][:, 2] >> 28) & 15).to(torch.int64) << 32)
            d = torch.arange(12, device=dev)
            entries = ((window[:, None] >> (3 * d)) & 7).to(torch.uint8)
            at = (M_new - H)[:, None] + d
            keep = d[None, :] < H[:, None]
            lists[torch.arange(boards, device=dev)[:, None].expand(-1, 12)[keep], at[keep]] = entries[keep]
            args = (state["rows"], state["lines"], (M_new - H).to(torch.uint8), torch.arange(boards, device=dev, dtype=torch.int32), lists,
                    L_, M_new)
            ref = T.prove_nodes(*args, max_nodes=1 << log2, device=dev, validate=False)
            same = all(torch.equal(mine[k], ref[k]) for k in ("solved", "proved", "solution_len", "bound", "nodes"))
            total = float(mine["nodes"].double().sum())
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(_timed(lambda: T.prove_nodes(*args, max_nodes=1 << log2, device=dev, validate=False), 1, warmup=0))
                tb.append(_timed(lambda: T.window_prove(env, max_nodes=1 << log2), 1, warmup=0))
            line = dict(max_nodes=f"2^{log2}", boards=boards, nodes=int(total), outputs_equal=bool(same),
                        prove_nodes_ms=round(median(ta) * 1e3, 3), window_prove_ms=round(median(tb) * 1e3, 3),
                        prove_nodes_nodes_per_second=round(total / median(ta), 1), window_prove_nodes_per_second=round(total / median(tb), 1),
                        ratio=round(median(ta) / median(tb), 4))
            out["time"]["search"].append(line)
            progress(line)
        env.terminate()

    if "loose" in sections:                                    # the loose pool: every policy wins about 0.999 there
        loose = (rows, pieces)
        got = {}
        for log2 in (None, 12):
            env, player = make(M_, loose, 1, None, log2, True)
            got["base" if log2 is None else f"proof_2^{log2}"] = play(env, player, 16 * (M_ + 1), M_)
            env.terminate()
        for v in got.values():
            v.pop("per_move", None)
        out["loose"] = got
        progress(got)
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "window_prove" in l or "placement_exact_nodes" in l]
    out["not_measured"] = ("other weight rows, the fourteen features and spare_weight other than 0; other pools and seeds; learners and "
                           "table policies as bases; a step's milliseconds include the base's act(), the state reads, under reuse the "
                           "afterstate enumeration, and the environment's step")
    return out


# part window's rates on 4,096 boards (profiles/learner/probe_window.log): base -> (episodes, wins) alone and at 2^8 and 2^12 nodes
WINDOW_RECORD = {"one_ply": {None: (290486, 121962), 8: (305761, 188687), 12: (319886, 236021)},
                 "beam_3x8": {None: (309968, 247253), 8: (326378, 282375), 12: (333769, 303791)}}


def part_ntuple_window(budgets=(8, 12), boards=4096, rounds=5):
    """The window proof search ordered by an n-tuple table (include/tpl_learn.h: tpl_ntuple_window_prove; T.ntuple_window_prove,
    T.ProofPolicy(table=)) beside the classical order, on part window's set-up: the tight pool of the record, 4,096 boards, one seed,
    reuse on.  The table is part ntuple_exact's "feat+spare, rate 8, tight pool", made by its recipe."""
    import numpy as np
    import torch
    import tetris_piclim as T
    _plane_fields, _resident_planes = T.solve._plane_fields, T.solve._resident_planes
    dev = "cuda:0"
    L_, M_, M_new = 10, 40, 16
    out = dict(part="ntuple_window", budgets=[f"2^{b}" for b in budgets], boards=boards, rates={}, verdict_1_share_per_move={}, search=[])

    def progress(what):
        print(json.dumps(what), file=sys.stderr, flush=True)

    n = 1 << 16
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(n, seed=7)
    env.terminate()
    found = T.solve_configs(rows, pieces, L_, M_, width=16, device=dev, validate=False)
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], M_new)
    out["pool"] = dict(size=int(tight[0].shape[0]), of=n, seed=7, L=L_, M=M_new)
    classical = np.array(T.CLASSICAL_WEIGHTS)

    env = T.BatchedTetris(L_, M_new, 4096, device=dev, seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=tight)
    learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, rate=8.0, shape="feat+spare", bound=False)
    for steps in (10000, 30000):
        learner.train(steps)
    one = learner.evaluate(12288, bound=False)
    table = learner.table.clone()
    env.terminate()
    out["table"] = dict(table="feat+spare, rate 8, tight pool", one_ply_win_rate_on_its_pool=round(one["win_rate"], 5),
                        order="gamma 1, reward (1, 10, -1): the training's")
    progress(out["table"])
    order = dict(table=table, gamma=1.0, reward=NTUPLE_LARGE_REWARD)

    def make(depth, width, log2, ordered):
        env = T.BatchedTetris(L_, M_new, boards, device=dev, seed=11, auto_reset=True, reward=(0.0, 1.0, 0.0), config_pool=tight)
        env.reset()
        base = T.HeuristicPolicy(env, classical, depth=depth) if width is None else T.BeamPolicy(env, classical, depth, width)
        if log2 is None:
            return env, base
        return env, T.ProofPolicy(env, base, max_nodes=1 << log2, reuse=True, **(order if ordered else {}))

    def play(env, player, steps):
        """part window's play: episodes, wins, the episodes that held a verdict 1 and did not end won, the verdicts per move number."""
        action = torch.empty(boards, dtype=torch.uint8, device=dev)
        reward = torch.empty(boards, dtype=torch.float32, device=dev)
        done = torch.empty(boards, dtype=torch.uint8, device=dev)
        tallies = torch.zeros(4, dtype=torch.int64, device=dev)
        per_move = torch.zeros(M_new * 4, dtype=torch.int64, device=dev)
        held = torch.zeros(boards, dtype=torch.bool, device=dev)
        proof = isinstance(player, T.ProofPolicy)
        planes = _resident_planes(env)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if proof:
                moves = _plane_fields(*planes)[0].to(torch.int64)
            player.act(out=action)
            if proof:
                per_move += torch.bincount(moves * 4 + player.verdict.to(torch.int64), minlength=M_new * 4)[:M_new * 4]
                held |= player.played
            env.step_into(action, reward, done)
            over, won = done.bool(), reward == 1.0
            tallies += torch.stack([over.sum(), (over & won).sum(), (over & held).sum(), (over & held & ~won).sum()])
            held &= ~over
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        e, w, with_proof, broken = tallies.tolist()
        p = w / max(e, 1)
        got = dict(episodes=int(e), wins=int(w), win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(e, 1)) ** 0.5, 6),
                   steps=steps, seconds=round(seconds, 2), ms_per_step=round(seconds * 1e3 / steps, 3))
        if proof:
            got.update(episodes_that_held_a_verdict_1=with_proof, of_them_not_won=broken, stats=player.stats())
            got["per_move"] = per_move.view(M_new, 4).tolist()
        return got

    steps = 16 * (M_new + 1) * (1 << 14) // boards               # the record's episode budget on fewer boards
    broken = 0
    for name, depth, width in (("one_ply", 1, None), ("beam_3x8", 3, 8)):
        got = {}
        for log2 in (None,) + tuple(budgets):
            for ordered in ((False,) if log2 is None else (False, True)):
                env, player = make(depth, width, log2, ordered)
                key = "base" if log2 is None else f"proof_2^{log2}_{'table' if ordered else 'classical'}"
                got[key] = play(env, player, steps)
                env.terminate()
                if not ordered and log2 in WINDOW_RECORD[name]:    # part window's rows, win for win
                    got[key]["reproduces_part_window"] = (got[key]["episodes"], got[key]["wins"]) == WINDOW_RECORD[name][log2]
                    if not got[key]["reproduces_part_window"]:     # another set-up: nothing measured on it is comparable
                        raise RuntimeError(f"{name} {key}: {got[key]['episodes']} episodes and {got[key]['wins']} wins, part window has "
                                           f"{WINDOW_RECORD[name][log2]}: the set-up is not the record's, so the probe stops here")
                if log2 is not None:
                    broken += got[key]["of_them_not_won"]
                    shares = [dict(move=m, searched_or_followed=sum(v), verdict_1=round(v[1] / max(sum(v[1:]), 1), 5))
                              for m, v in enumerate(got[key].pop("per_move"))]
                    out["verdict_1_share_per_move"][f"{name}_{key}"] = shares      # of the boards searched at that move counter
                progress({name: {key: got[key]}})
        out["rates"][name] = got
    out["episodes_that_held_a_verdict_1_and_did_not_end_won"] = broken

    # nodes a second beside tpl_placement_window_prove on the same boards, mid-game, alternated rounds
    median = lambda ts: sorted(ts)[len(ts) // 2]
    env, player = make(1, None, None, False)
    play(env, player, 40)
    for log2 in budgets:
        theirs = T.window_prove(env, max_nodes=1 << log2)
        mine = T.ntuple_window_prove(env, max_nodes=1 << log2, **order)
        both = theirs["proved"] & mine["proved"]
        same = all(torch.equal(theirs[k][both], mine[k][both]) for k in ("solved", "solution_len", "verdict", "bound"))
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(_timed(lambda: T.window_prove(env, max_nodes=1 << log2), 1, warmup=0))
            tb.append(_timed(lambda: T.ntuple_window_prove(env, max_nodes=1 << log2, **order), 1, warmup=0))
        na, nb = float(theirs["nodes"].double().sum()), float(mine["nodes"].double().sum())
        line = dict(max_nodes=f"2^{log2}", boards=boards, classical=dict(nodes=int(na), proved=int(theirs["proved"].sum()),
                                                                        verdict_1=int((theirs["verdict"] == 1).sum()),
                                                                        ms=round(median(ta) * 1e3, 3), nodes_per_second=round(na / median(ta), 1)),
                    table=dict(nodes=int(nb), proved=int(mine["proved"].sum()), verdict_1=int((mine["verdict"] == 1).sum()),
                               ms=round(median(tb) * 1e3, 3), nodes_per_second=round(nb / median(tb), 1)),
                    both_proved=int(both.sum()), verdicts_and_lengths_equal_where_both_prove=bool(same),
                    nodes_per_second_ratio=round((nb / median(tb)) / (na / median(ta)), 4))
        out["search"].append(line)
        progress(line)
    env.terminate()
    res = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), T._learn_lib.build_library()],
                         capture_output=True, text=True, cwd=ROOT)
    out["kernel"] = [" ".join(l.split()) for l in res.stdout.splitlines() if "window" in l]
    out["not_measured"] = ("2^16 nodes; reuse off; other tables, seeds, pools, gammas and rewards; the window forms as an order; table "
                           "policies as bases; the loose pool; a step's milliseconds include the base's act(), the state reads, the "
                           "afterstate enumeration and the environment's step")
    return out


def part_ntuple_shape_ab(parent, rounds=5, reps=20, n=1 << 18):
    import ctypes as C
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    new, check = m.lib(), m.check
    old = C.CDLL(os.path.abspath(parent))
    for name in ("tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_update", "tpl_ntuple_search", "tpl_ntuple_update_trace",
                 "tpl_ntuple_update_coherent"):
        getattr(old, name).argtypes, getattr(old, name).restype = getattr(new, name).argtypes, C.c_int32
    stream = torch._C._cuda_getCurrentRawStream(0)
    slots, head = 17, 16
    env, ring = _shape_ring(T, n, slots)
    tables, coherences, error, outputs = _shape_buffers(T, m, n)
    start = tables[0].clone()
    libs = {"parent": _shape_calls(old, check, ring, n, head, slots, tables, coherences, error, outputs, stream, twin=True)(0),
            "new": _shape_calls(new, check, ring, n, head, slots, tables, coherences, error, outputs, stream, twin=True)(0)}
    for _ in range(2):                                           # a coherence buffer with step sizes of every kind
        error.normal_()
        libs["parent"]["coherent_h4"]()
    filled = coherences[0].clone()
    error.normal_()
    lines, equal = [], {}
    for name in libs["new"]:                                     # byte for byte, from the same table and coherence buffer
        left = {}
        for which in ("parent", "new"):
            tables[0].copy_(start)
            coherences[0].copy_(filled)
            for t in outputs:
                t.zero_()
            libs[which][name]()
            torch.cuda.synchronize()
            left[which] = [t.clone() for t in outputs] + [tables[0].clone(), coherences[0].clone()]
        equal[name] = all(torch.equal(x, y) for x, y in zip(left["parent"], left["new"]))
    tables[0].copy_(start)
    lines.append(dict(boards=n, outputs_equal=equal, table_changed_by_the_updates=bool(int((left["new"][-2] != start).sum()) > 0)))
    us = lambda t: round(t * 1e6, 2)
    for name in libs["new"]:
        fa, fb = libs["parent"][name], libs["new"][name]
        k = max(reps // 4, 3) if name == "search" else reps
        a, b, pa, nb = [], [], [], []
        for _ in range(rounds):                                  # the parent against itself: the noise of the method
            a.append(us(_timed(fa, k)))
            b.append(us(_timed(fa, k)))
        for _ in range(rounds):                                  # the parent against this build, alternated
            pa.append(us(_timed(fa, k)))
            nb.append(us(_timed(fb, k)))
        lo, hi = min(a + b), max(a + b)
        pm, nm = sorted(pa)[rounds // 2], sorted(nb)[rounds // 2]
        bound = max(hi, round(1.02 * pm, 2))
        lines.append(dict(boards=n, entry=name, parent_against_itself=dict(a=a, b=b, min=lo, max=hi), parent=pa, new=nb, parent_median=pm,
                          new_median=nm, ratio=round(nm / pm, 4), bound_us=bound, within=bool(nm <= bound)))
        print(json.dumps(lines[-1]), file=sys.stderr, flush=True)
    env.terminate()
    return dict(part="ntuple_shape_ab", rounds=rounds, launches_per_timing=reps, lines=lines,
                every_output_equal=all(equal.values()), every_median_within=all(l["within"] for l in lines[1:]))


def part_exact_ab(parent, rounds=5, reps=3, boards=4096, log2_nodes=12, timing=True):
    """The ten plain and the six limited entries of the five exact-search units of another build of the learner library against
    this tree's, both loaded into one process and reached through the package's own wrappers (the library handle is swapped under
    them): carved L = 10 / M = 40, seed 7, `boards` configurations as roots, and as nodes and resident boards after ten moves of the
    classical one-ply player; max_nodes 2^log2_nodes; the table entries under each of the four plain forms (random tables: an order
    is an order); the limited entries through the four *_limited wrappers at first_limit = 0.  Every output is compared byte for
    byte, a limited entry's under "add" and under "double"; then (timing) each call is timed by ntuple_shape_ab's protocol, a
    limited one under "add"."""
    import ctypes as C
    import numpy as np
    import torch
    import tetris_piclim as T
    m = T._learn_lib
    libs = {"new": m.lib(), "parent": C.CDLL(os.path.abspath(parent))}
    for name in m.LEARN_SYMBOLS:
        f, g = getattr(libs["new"], name), getattr(libs["parent"], name)
        g.argtypes, g.restype = f.argtypes, f.restype
    dev, L_, M_, cap = "cuda:0", 10, 40, 1 << log2_nodes
    env = T.BatchedTetris(L_, M_, 64, device=dev, seed=7)
    rows, pieces = env.carved_configs(boards, seed=7)
    env.terminate()
    env = T.BatchedTetris(L_, M_, boards, device=dev, seed=11, auto_reset=False, reward=(0.0, 1.0, 0.0), config_pool=(rows, pieces))
    env.reset()
    player, action = T.HeuristicPolicy(env, np.array(T.CLASSICAL_WEIGHTS), depth=1), torch.empty(boards, dtype=torch.uint8, device=dev)
    for _ in range(10):                                          # moves = 10: the window shows its twelve pieces again
        player.act(out=action)
        env.step(action, observe=False)
    state, entry = env.packed_state(), T.config_index(env)
    running = state["state"] == 0
    lines = torch.where(running, state["lines"], torch.full_like(state["lines"], L_))
    node = (state["rows"], lines, state["moves"], entry, pieces, L_, M_)
    rows12 = np.array(T.CLASSICAL_WEIGHTS)
    weights = {"": rows12, "_move": np.concatenate([rows12, np.array([-0.4, 0.3], np.float32)])}
    gen = torch.Generator(device="cpu").manual_seed(7)
    tables = {form: torch.randint(-(1 << 16), 1 << 16, (m.ntuple_entries_of(form),), generator=gen, dtype=torch.int32).to(dev)
              for form in m.NTUPLE_EXACT_FORMS}
    order = dict(gamma=0.99, reward=NTUPLE_LARGE_REWARD)
    calls = {}
    for form, w in weights.items():
        calls["tpl_placement_exact" + form] = lambda w=w: T.prove_configs(rows, pieces, L_, M_, weights=w, max_nodes=cap, device=dev,
                                                                        validate=False)
        calls["tpl_placement_exact_nodes" + form] = lambda w=w: T.prove_nodes(*node, weights=w, max_nodes=cap, device=dev, validate=False)
        calls["tpl_placement_exact_labels" + form] = lambda w=w: T.label_moves(*node, weights=w, max_nodes=cap, device=dev, validate=False)
        calls["tpl_placement_window_prove" + form] = lambda w=w: T.window_prove(env, weights=w, max_nodes=cap)
    for form, table in tables.items():
        calls[f"tpl_ntuple_exact {form}"] = lambda t=table: T.ntuple_prove_configs(rows, pieces, L_, M_, t, max_nodes=cap, device=dev,
                                                                                  validate=False, **order)
        calls[f"tpl_ntuple_window_prove {form}"] = lambda t=table: T.ntuple_window_prove(env, t, max_nodes=cap, **order)
    limited = {}                                                 # the limited entries: a call takes the growth rule, "add" unless told
    for form, w in weights.items():
        limited["tpl_placement_exact_limited" + form] = lambda rule, w=w: T.prove_configs_limited(
            rows, pieces, L_, M_, discrepancy=rule, first_limit=0, weights=w, max_nodes=cap, device=dev, validate=False)
        limited["tpl_placement_window_prove_limited" + form] = lambda rule, w=w: T.window_prove_limited(
            env, discrepancy=rule, first_limit=0, weights=w, max_nodes=cap)
    for form, table in tables.items():
        limited[f"tpl_ntuple_exact_limited {form}"] = lambda rule, t=table: T.ntuple_prove_configs_limited(
            rows, pieces, L_, M_, t, discrepancy=rule, first_limit=0, max_nodes=cap, device=dev, validate=False, **order)
        limited[f"tpl_ntuple_window_prove_limited {form}"] = lambda rule, t=table: T.ntuple_window_prove_limited(
            env, t, discrepancy=rule, first_limit=0, max_nodes=cap, **order)
    for name, call in limited.items():
        calls[name] = lambda rule="add", call=call: call(rule)

    def run(which, name, *rule):
        m._handle = libs[which]
        try:
            return calls[name](*rule)
        finally:
            m._handle = libs["new"]

    lines_, equal = [], {}
    for name in calls:                                           # byte for byte, every tensor the wrapper returns
        rules = [("double",), ("add",)] if name in limited else [()]
        equal[name] = True
        for rule in rules:
            got = {}
            for which in ("parent", "new"):
                got[which] = run(which, name, *rule)
                torch.cuda.synchronize()
            equal[name] &= set(got["parent"]) == set(got["new"]) and all(torch.equal(got["parent"][k], got["new"][k]) for k in got["new"])
        nodes = got["new"]["nodes"].double()                     # of the last rule: "add", the one timed
        lines_.append(dict(entry=name, outputs_equal=equal[name], searches=int(nodes.numel()), nodes=int(nodes.sum()),
                           capped=int((nodes == cap).sum()), **(dict(compared_under=["double", "add"]) if name in limited else {})))
        print(json.dumps(lines_[-1]), file=sys.stderr, flush=True)
    out = dict(part="exact_ab", boards=boards, max_nodes=f"2^{log2_nodes}", running_nodes=int(running.sum()), lines=lines_,
               every_output_equal=all(equal.values()))
    if timing:
        ms = lambda t: round(t * 1e3, 3)
        for name in calls:
            fa, fb = (lambda: run("parent", name)), (lambda: run("new", name))
            k = 1 if "labels" in name else reps                  # forty searches a node: one launch is long enough
            a, b, pa, nb = [], [], [], []
            for _ in range(rounds):                              # the parent against itself: the noise of the method
                a.append(ms(_timed(fa, k, warmup=1)))
                b.append(ms(_timed(fa, k, warmup=1)))
            for _ in range(rounds):                              # the parent against this build, alternated
                pa.append(ms(_timed(fa, k, warmup=1)))
                nb.append(ms(_timed(fb, k, warmup=1)))
            lo, hi = min(a + b), max(a + b)
            pm, nm = sorted(pa)[rounds // 2], sorted(nb)[rounds // 2]
            bound = max(hi, round(1.02 * pm, 3))
            lines_.append(dict(entry=name, parent_against_itself=dict(a=a, b=b, min=lo, max=hi), parent=pa, new=nb, parent_median_ms=pm,
                               new_median_ms=nm, ratio=round(nm / pm, 4), bound_ms=bound, within=bool(nm <= bound), launches_per_timing=k))
            print(json.dumps(lines_[-1]), file=sys.stderr, flush=True)
        out.update(rounds=rounds, launches_per_timing=reps, every_median_within=all(l["within"] for l in lines_ if "within" in l))
    env.terminate()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=sorted(PARTS) + ["ntuple_shape_ab", "exact_ab"])
    ap.add_argument("--parent", default=None, help="of parts ntuple_shape_ab and exact_ab: the learner library of the build to compare against")
    ap.add_argument("--no-timing", action="store_true", help="of part exact_ab: compare the outputs only")
    ap.add_argument("--chunk", default=None, help="I/K: of part ntuple_coherent_sweep, every K-th cell from the I-th on")
    ap.add_argument("--sections", default=None, help="of part window: which of record,rates,verdicts,time,loose to run (all); "
                    "of part limited: which of proofs,cost,searching_out,wins")
    ap.add_argument("--budgets", default=None, help="of part window: the log2 of the node budgets, e.g. 8,12 (8,12,16)")
    args = ap.parse_args()
    if args.part:
        kw = {}
        if args.chunk:
            if args.part != "ntuple_coherent_sweep":
                ap.error("--chunk goes with --part ntuple_coherent_sweep")
            i, k = (int(v) for v in args.chunk.split("/"))
            if not 0 <= i < k:
                ap.error("--chunk I/K needs 0 <= I < K")
            kw["chunk"] = (i, k)
        if args.sections or args.budgets:
            if args.part not in ("window", "limited") or (args.budgets and args.part != "window"):
                ap.error("--sections goes with --part window or limited, --budgets with --part window")
            if args.sections:
                kw["sections"] = tuple(args.sections.split(","))
            if args.budgets:
                kw["budgets"] = tuple(int(v) for v in args.budgets.split(","))
        if args.part in ("ntuple_shape_ab", "exact_ab"):
            if not args.parent:
                ap.error(f"--part {args.part} needs --parent LIB")
            kw["parent"] = args.parent
        if args.no_timing:
            if args.part != "exact_ab":
                ap.error("--no-timing goes with --part exact_ab")
            kw["timing"] = False
        print(json.dumps(globals()["part_" + args.part](**kw)), flush=True)
        return 0
    for name, limit in PARTS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", name]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
        if res.returncode != 0 or not lines:
            print(json.dumps(dict(part=name, failed=res.returncode, stderr=res.stderr[-2000:])), flush=True)
            return res.returncode or 1               # nothing more is started on the GPU after a failed step
        print(lines[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
