#!/usr/bin/env python3
"""Dev tool: evaluate(persistent=False) -- the stepping loop: a PyTorch actor forward, a navsim_step launch and the quota
bookkeeping in torch per env step -- against evaluate(persistent=True) -- ONE launch of navsim_evaluate_mlp64 /
navsim_evaluate_resmlp512 -- in one process: 1024 episodes at n_parallel = 1024 on stage_1 with the 500-step cap, both policies
(random-init actors, seeded: which episodes are played does not depend on the path's speed).  One warm-up call of each path, then
five calls of each, alternating; the figure is the median of the wall clock around the stepping alone (evaluate()'s `timing`: env
creation and CSV excluded, the clock stops behind a device synchronise).  Next to it: the persistent launch's time per executed
env step and the training rollout's (PPOTrainer.rollout as tools/time_rollout.py times it) at the same env count, and what
PPOConfig.eval_every = 1 adds to an iteration of the headline configuration (4096 envs x 512 steps, 50 epochs).
usage: python tools/time_evaluate.py [--out profiles/eval_persistent.txt] [--quick]
       rocprofv3 --kernel-trace --stats ... -- python tools/time_evaluate.py --persistent-only     (the kernels' own time)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from navbot_ppo_amd import evaluate as ev
from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd.env import VecEnv

QUICK = "--quick" in sys.argv
KERNEL_ONLY = "--persistent-only" in sys.argv   # under rocprofv3 --kernel-trace --stats: four persistent evaluations per policy
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
N_EP, N_PAR, CAP = (64, 64, 40) if QUICK else (1024, 1024, 500)
REPS = 2 if QUICK else 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def rollout_us_per_step(policy, n_envs, T=512, reps=8):
    env = VecEnv(n_envs, map="stage_1", max_episode_steps=500, seed=0)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy=policy, rollout_len=T, seed=0))
    for _ in range(2):
        tr.rollout()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        tr.rollout()
    e1.record()
    torch.cuda.synchronize()
    env.close()
    return e0.elapsed_time(e1) / reps / T * 1e3


def main():
    dev = torch.device("cuda")
    if KERNEL_ONLY:
        for policy in ("mlp64x2", "resmlp512"):
            torch.manual_seed(0)
            actor, _ = nets.make_policy(policy, 16)
            for _ in range(4):
                tm = {}
                ev.evaluate(actor.to(dev).eval(), num_episodes=N_EP, max_timesteps_per_episode=CAP, n_parallel=N_PAR, seed=1, log=None,
                            persistent=True, timing=tm)
            say(f"{policy}: {tm['steps']} steps per launch (kernel time per step = the evaluation kernel's average in the trace / steps)")
        return
    say(f"# {torch.cuda.get_device_name(0)}; {N_EP} episodes, n_parallel {N_PAR}, stage_1, cap {CAP}; median of {REPS} after one warm-up, "
        "wall clock of the stepping alone")
    for policy in ("mlp64x2", "resmlp512"):
        torch.manual_seed(0)
        actor, _ = nets.make_policy(policy, 16)
        actor = actor.to(dev).eval()
        t = {False: [], True: []}
        steps, summ = {}, {}
        for rep in range(REPS + 1):
            for persistent in (False, True):   # alternating: both paths see the same machine state
                tm = {}
                s = ev.evaluate(actor, num_episodes=N_EP, max_timesteps_per_episode=CAP, n_parallel=N_PAR, seed=1, log=None,
                                persistent=persistent, timing=tm)
                if rep:   # rep 0 is the warm-up
                    t[persistent].append(tm["seconds"])
                steps[persistent], summ[persistent] = tm["steps"], s
        loop, pers = statistics.median(t[False]), statistics.median(t[True])
        say(f"{policy}: stepping loop {loop * 1e3:9.2f} ms ({steps[False]} steps, {loop / steps[False] * 1e6:7.1f} us per step; "
            f"min {min(t[False]) * 1e3:.2f} max {max(t[False]) * 1e3:.2f})")
        say(f"{policy}: persistent    {pers * 1e3:9.2f} ms ({steps[True]} steps, {pers / steps[True] * 1e6:7.2f} us per step; "
            f"min {min(t[True]) * 1e3:.2f} max {max(t[True]) * 1e3:.2f})   ratio {loop / pers:.1f}x")
        say(f"{policy}: success / collision / timeout  loop {summ[False]['success_rate']:.3f} / {summ[False]['collision_rate']:.3f} / "
            f"{summ[False]['timeout_rate']:.3f}   persistent {summ[True]['success_rate']:.3f} / {summ[True]['collision_rate']:.3f} / "
            f"{summ[True]['timeout_rate']:.3f}   (PyTorch actor against HIP actor: the same episodes up to float32 rounding of the actions)")
        if not QUICK:
            ro = rollout_us_per_step(policy, N_PAR)
            say(f"{policy}: training rollout at {N_PAR} envs {ro:6.2f} us per step; persistent evaluation {pers / steps[True] * 1e6:6.2f} us per "
                f"executed step (host clock of one launch: includes the reset, the launch and the synchronise)")
    if not QUICK:
        for policy in ("mlp64x2", "resmlp512"):
            res = {}
            for every in (0, 1):
                env = VecEnv(4096, map="stage_1", max_episode_steps=500, seed=0)
                tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy=policy, rollout_len=512, seed=0, eval_every=every, eval_episodes=100))
                its = [tr.iteration() for _ in range(4)][1:]
                res[every] = (statistics.median(i["iter_time"] for i in its),
                              statistics.median(i.get("eval_time", 0.0) for i in its), its[-1])
                env.close()
            lg = res[1][2]
            say(f"{policy}: headline iteration (4096 x 512, 50 epochs) {res[0][0] * 1e3:.1f} ms without, {res[1][0] * 1e3:.1f} ms with "
                f"eval_every=1 + {res[1][1] * 1e3:.2f} ms for the evaluation of 100 episodes ({lg['eval_steps']} steps; "
                f"{res[1][1] / res[1][0] * 100:.1f} % of an iteration)")
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
