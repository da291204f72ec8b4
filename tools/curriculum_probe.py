#!/usr/bin/env python3
"""Per-configuration tallies and the resampled pool on one MI355X (profiles/learner/README.md, `--part curriculum`).

    --part cost        PoolTally.observe, config_index and resample_pool + load_configs beside env.step_into and one "feat" learner
                       step on mid-game L = 10 / M = 40 boards (4,096 and 2^20), medians of alternating rounds with their spread
    --part unchanged   step_into, NTuplePolicy.act and a learner step WITHOUT a curriculum: runs on this tree and on a parent tree
                       alike (it uses nothing this feature adds), so a caller can alternate the two on one box
    --part sweep       the record's learners ("feat", "feat+spare", rate 8, 40,000 steps of 4,096 boards, seed 11) on the loose pool
                       and on tighten_pool(M_new=16): uniform dealing first, then the curriculum at refresh_every x gain, each
                       evaluated on the UNIFORM base pool
    --part analysis    the classical weights at one ply and at beam (3, 8) on the tight pool: wins per configuration grouped by
                       M - config_bound and by the nodes prove_configs needs (max_nodes 2^12)

One JSON line per part on stdout, progress on stderr.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REWARD = (0.0, 1.0, 0.0)
NTUPLE_LARGE_REWARD = (1.0, 10.0, -1.0)          # tools/learner_probe.py's: the reward of the record's learners


def progress(what):
    print(json.dumps(what), file=sys.stderr, flush=True)


def _timed(fn, reps, warmup=3):
    """Microseconds per call of `reps` back-to-back calls between two events."""
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def _spread(ts):
    s = sorted(ts)
    return dict(median=round(s[len(s) // 2], 2), min=round(s[0], 2), max=round(s[-1], 2))


def _pool(T, n=1 << 16, seed=7):
    env = T.BatchedTetris(10, 40, 64, device="cuda:0", seed=seed)
    rows, pieces = env.carved_configs(n, seed=seed)
    env.terminate()
    return rows, pieces


def _mid_game(T, n, pool, steps=20):
    import torch
    env = T.BatchedTetris(10, 40, n, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=pool)
    env.reset()
    reward = torch.empty(n, dtype=torch.float32, device="cuda:0")
    done = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    for t in range(steps):
        env.step_into(env.synthetic_actions(t), reward, done)
    return env, reward, done


def part_unchanged(rounds=5, reps=50):
    import torch
    import tetris_piclim as T
    pool = _pool(T)
    out = dict(part="unchanged", tree=ROOT, rounds=rounds, launches_per_timing=reps, boards={})
    for n in (4096, 1 << 20):
        env, reward, done = _mid_game(T, n, pool)
        action = env.synthetic_actions(99)
        table = T.ntuple_table("cuda:0", "feat")
        policy = T.NTuplePolicy(env, table, 1.0, 0.05, 11)
        learner = T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.05, seed=11, shape="feat")
        learner.train(3)
        calls = dict(step=lambda: env.step_into(action, reward, done), act=lambda: policy.act(out=action, step=3),
                     learner_step=lambda: learner.train(1))
        times = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                times[k].append(_timed(fn, reps))
        out["boards"][str(n)] = {k + "_us": _spread(v) for k, v in times.items()}
        env.terminate()
    return out


def part_cost(rounds=5, reps=50):
    import torch
    import tetris_piclim as T
    pool = _pool(T)
    out = dict(part="cost", rounds=rounds, launches_per_timing=reps, pool=1 << 16, boards={})
    for n in (4096, 1 << 20):
        row = {}
        for n_cfg in (1 << 16, 8, 1):
            sub = (pool[0][:n_cfg].contiguous(), pool[1][:n_cfg].contiguous())
            env, reward, done = _mid_game(T, n, sub)
            action = env.synthetic_actions(99)
            tally = T.PoolTally(env)
            index = T.config_index(env)
            calls = dict(step=lambda: env.step_into(action, reward, done), observe=lambda: tally.observe(action),
                         config_index=lambda: T.config_index(env, out=index))
            if n_cfg == 1 << 16:
                learner = T.NTupleLearner(env, gamma=1.0, rate=8.0, epsilon=0.05, seed=11, shape="feat")
                cur = T.PoolCurriculum(env, *sub, loaded=True)
                learner.train(3)
                calls.update(learner_step=lambda: learner.train(1), learner_step_observed=lambda: learner.train(1, curriculum=cur))
            times = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    times[k].append(_timed(fn, reps))
            med = {k: sorted(v)[rounds // 2] for k, v in times.items()}
            got = {k + "_us": _spread(v) for k, v in times.items()}
            got["observe_over_step"] = round(med["observe"] / med["step"], 3)
            if "learner_step" in med:
                got["observe_over_learner_step"] = round(med["observe"] / med["learner_step"], 3)
                got["observed_learner_step_over_learner_step"] = round(med["learner_step_observed"] / med["learner_step"], 3)
            got["ends_counted_per_observe"] = round(float(tally.episodes.sum()) / max(sum(len(v) * (reps + 3) for k, v in times.items() if k == "observe"), 1), 1)
            row[f"n_cfg_{n_cfg}"] = got
            progress({str(n): {f"n_cfg_{n_cfg}": got}})
            env.terminate()
        out["boards"][str(n)] = row
    # resample_pool at n_cfg = count = 65,536 with the load_configs that follows it
    env, reward, done = _mid_game(T, 4096, pool, steps=45)
    weights = torch.randint(1, 1000, (1 << 16,), dtype=torch.int64, device="cuda:0")
    state = dict(round=0)

    def resample():
        state["round"] += 1
        return T.resample_pool(pool[0], pool[1], weights, 1 << 16, seed=3, round=state["round"])

    def resample_and_load():
        rows, pieces, _ = resample()
        env.reset()                                          # frees the other pool buffer (the guard counts steps otherwise)
        env.load_configs(rows, pieces, validate=False)

    def reset_only():
        env.reset()

    times = dict(resample=[], resample_reset_load=[], reset_only=[])
    for _ in range(rounds):
        times["resample"].append(_timed(resample, 10, warmup=1))
        times["resample_reset_load"].append(_timed(resample_and_load, 10, warmup=1))
        times["reset_only"].append(_timed(reset_only, 10, warmup=1))
    out["resample_65536"] = {k + "_us": _spread(v) for k, v in times.items()}
    out["resample_65536"]["note"] = "resample_pool includes torch.cumsum, the weights' check (one host sync) and three allocations"
    env.terminate()
    return out


def _result(r):
    p = r["win_rate"]
    return dict(episodes=r["episodes"], wins=r["wins"], win_rate=round(p, 5), standard_error=round((p * (1 - p) / max(r["episodes"], 1)) ** 0.5, 6))


def _pools(T):
    rows, pieces = _pool(T)
    found = T.solve_configs(rows, pieces, 10, 40, width=16, device="cuda:0", validate=False)
    tight = T.tighten_pool(rows, pieces, found["solved"], found["solution_len"], 16)
    return (rows, pieces), tight


def part_sweep(eval_steps=12288):
    import torch
    import tetris_piclim as T
    loose, tight = _pools(T)
    out = dict(part="sweep", boards=4096, seed=11, pool_seed=7, tight_pool=int(tight[0].shape[0]), M_new=16, reward=list(NTUPLE_LARGE_REWARD),
               gamma=1.0, epsilon=0.05, rate=8.0, eval_steps=eval_steps, train_steps=40000, floor=1, runs=[])

    def learn(pool_name, pool, M_pool, shape, refresh_every=0, gain=0):
        env = T.BatchedTetris(10, M_pool, 4096, device="cuda:0", seed=11, auto_reset=True, reward=NTUPLE_LARGE_REWARD, config_pool=pool)
        learner = T.NTupleLearner(env, seed=11, gamma=1.0, epsilon=0.05, shape=shape, rate=8.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        before = _result(learner.evaluate(eval_steps))      # as the record's run: the start table is played first
        cur = T.PoolCurriculum(env, pool[0], pool[1], seed=11, floor=1, gain=gain, loaded=True) if refresh_every else None
        for steps in (10000, 30000):
            if cur is None:
                learner.train(steps)
            else:
                learner.train(steps, curriculum=cur, refresh_every=refresh_every)
        got = dict(pool=pool_name, shape=shape, refresh_every=refresh_every, gain=gain, start_table=before)
        if cur is not None:
            cur.fold()
            e, w = cur.base_episodes, cur.base_wins
            got["training"] = dict(refreshes=cur.refreshes, episodes=int(e.sum()), wins=int(w.sum()), configurations_never_dealt=int((e == 0).sum()),
                                   configurations_never_won=int(((e > 0) & (w == 0)).sum()),
                                   largest_share_of_the_last_pool=round(float(torch.bincount(cur.source.long()).max()) / cur.count, 5))
            env.reset()
            env.load_configs(pool[0], pool[1], validate=False)   # evaluate on the UNIFORM base pool
        got["one_ply"] = _result(learner.evaluate(eval_steps))
        got["seconds"] = round(time.perf_counter() - t0, 2)
        env.terminate()
        progress(got)
        out["runs"].append(got)
        return got

    for pool_name, pool, M_pool in (("tight", tight, 16), ("loose", loose, 40)):
        for shape in ("feat", "feat+spare"):
            learn(pool_name, pool, M_pool, shape)
            for refresh_every in (1000, 5000):
                for gain in (1, 8):
                    learn(pool_name, pool, M_pool, shape, refresh_every, gain)
    return out


def part_analysis(steps=1280):
    import numpy as np
    import torch
    import tetris_piclim as T
    loose, tight = _pools(T)
    rows, pieces = tight
    n_cfg, L_, M_ = int(rows.shape[0]), 10, 16
    slack = (M_ - T.config_bound(rows, L_, device="cuda:0")).cpu().numpy()
    proof = T.prove_configs(rows, pieces, L_, M_, max_nodes=1 << 12, device="cuda:0", validate=False)
    nodes, proved, solved = (proof[k].cpu().numpy() for k in ("nodes", "proved", "solved"))
    bucket = np.where(~proved, 13, np.ceil(np.log2(np.maximum(nodes, 1))).astype(np.int64))       # 13 = not proved within 2^12 nodes
    bucket = np.where(bucket <= 13, np.maximum(bucket, 0), 13)
    out = dict(part="analysis", pool="tight", configurations=n_cfg, M=M_, boards=1 << 16, steps=steps, proved_within_4096_nodes=round(float(proved.mean()), 5),
               players={})
    env = T.BatchedTetris(L_, M_, 1 << 16, device="cuda:0", seed=11, auto_reset=True, reward=REWARD, config_pool=tight)
    for name, kw in (("one_ply", {}), ("beam_3x8", dict(depth=3, width=8))):
        got = T.evaluate_heuristic(env, T.CLASSICAL_WEIGHTS, None, steps, per_config=True, **kw)
        e, w = got["episodes_by_config"].cpu().numpy().astype(np.int64), got["wins_by_config"].cpu().numpy().astype(np.int64)
        assert e.sum() == int(got["episodes"].sum()) and w.sum() == int(got["wins"].sum())

        def grouped(key):
            table = {}
            for v in np.unique(key):
                at = key == v
                ee, ww = int(e[at].sum()), int(w[at].sum())
                p = ww / max(ee, 1)
                rate = w[at] / np.maximum(e[at], 1)
                table[str(int(v))] = dict(configurations=int(at.sum()), episodes=ee, wins=ww, win_rate=round(p, 5),
                                          standard_error=round((p * (1 - p) / max(ee, 1)) ** 0.5, 5),
                                          never_won=int(((e[at] > 0) & (w[at] == 0)).sum()), always_won=int(((e[at] > 0) & (w[at] == e[at])).sum()),
                                          median_config_rate=round(float(np.median(rate)), 4))
            return table

        out["players"][name] = dict(episodes=int(e.sum()), wins=int(w.sum()), win_rate=round(float(w.sum()) / max(int(e.sum()), 1), 5),
                                    by_slack_M_minus_config_bound=grouped(slack), by_log2_nodes_to_prove_13_is_not_proved=grouped(bucket))
        progress({name: out["players"][name]})
    env.terminate()
    return out


PARTS = dict(cost=part_cost, unchanged=part_unchanged, sweep=part_sweep, analysis=part_analysis)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=sorted(PARTS), required=True)
    args = ap.parse_args()
    print(json.dumps(PARTS[args.part]()), flush=True)


if __name__ == "__main__":
    main()
