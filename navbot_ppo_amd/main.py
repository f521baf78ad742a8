"""Command-line entry with the reference's flags (project_ppo/src/arguments.py:22-46, main.py:423-499).

    python -m navbot_ppo_amd.main --method_name baseline --steps_per_iteration 5000 --max_timesteps 100000
    python -m navbot_ppo_amd.main --eval --eval_episodes 100 --method_name baseline
    torchrun --nproc-per-node 8 -m navbot_ppo_amd.main --n_envs 32768 ...          # env shards + RCCL

Same flag names and defaults; what they mean on the batched simulator:
  --steps_per_iteration   timesteps per PPO batch = n_envs * rollout_len (rounded up to a whole rollout step of all envs)
  --timesteps_per_episode episode cap (the rollout's timeout, ppo.py:552)
  --max_timesteps         training budget, counted like the reference over COMPLETED episodes (ppo.py:258)
  --tiny_debug_run        20-step episodes / 40-step batches / 400 total steps (arguments.py:58-65)
  --use_external_sampler  start/goal from the curated GoalSpawnSampler tables (parsed but never wired in the reference)
Additions (not in the reference): --n_envs, --policy, --map, --seed, --eval_persistent (with --eval: one launch instead of the
stepping loop), --eval_every K (training: a persistent evaluation of --eval_episodes episodes every K iterations), --max_grad_norm
(per-net gradient clipping + non-finite guard inside the update), --target_kl (stop an update's remaining epochs once approx_kl
exceeds 1.5 x the target), --minibatch_size M / --minibatch_shuffle MODE (K = ceil(batch / M) optimiser steps per epoch on slices of the
batch, shuffled on the device), --norm_reward / --clip_reward C (rewards scaled by the running standard deviation of the discounted
return and clipped to +-C before the return scan), --lr_schedule adaptive|linear with --desired_kl / --lr_min / --lr_max (the KL-adaptive
step size decided on the device after every optimiser step, or a linear decay over --max_timesteps), --learn_var with --ent_coef /
--var_min / --var_max (the exploration variance learned by the update, with an entropy bonus, stepped on the device), --bootstrap_truncated (time-outs
bootstrap with gamma V of their own row and the batch end with V of the next observation instead of counting as terminal), --movers NAME / --movers_period P (moving obstacles beside the static map, training and evaluation; NAME random:K with --movers_seed or bank:a,b,... is a bank of scenarios, one per env), --eval_movers NAME / --eval_movers_seed (held-out scenarios for --eval_every), --scan_history (the mlp64x2 policy reads the last three
scans), --continue_rollouts (only the first rollout resets the envs; later ones go on where the last stopped), --scenario_stats /
--scenario_priority failure|abs_adv with --scenario_resample_every / --scenario_score_alpha / --scenario_temperature /
--scenario_uniform_mix (on a bank of scenarios: per-scenario training statistics from the device, and the envs re-assigned towards the
scenarios that score worst).  Vision flags are accepted and refused (the camera
modality is outside the LiDAR hot path); --mode test maps to --eval (the reference's test path is broken).
"""
import argparse
import os
import sys


def get_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mode", type=str, default="train")
    p.add_argument("--actor_model", type=str, default="")
    p.add_argument("--critic_model", type=str, default="")
    p.add_argument("--method_name", type=str, default="baseline")
    p.add_argument("--eval", action="store_true", default=False)
    p.add_argument("--eval_episodes", type=int, default=100)
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--timesteps_per_episode", type=int, default=500)
    p.add_argument("--max_timesteps", type=int, default=5000)
    p.add_argument("--steps_per_iteration", type=int, default=5000)
    p.add_argument("--save_every_iterations", type=int, default=2)
    p.add_argument("--resume", action="store_true", default=False)
    p.add_argument("--dry_run_vision", action="store_true", default=False)
    p.add_argument("--vision_backbone", type=str, default="mobilenet_v2")
    p.add_argument("--vision_proj_dim", type=int, default=64)
    p.add_argument("--use_external_sampler", action="store_true", default=False)
    p.add_argument("--tiny_debug_run", action="store_true", default=False)
    # batched-simulator additions
    p.add_argument("--n_envs", type=int, default=None, help="parallel envs over all ranks (default: min(steps_per_iteration, 4096))")
    p.add_argument("--policy", type=str, default="resmlp512", choices=["resmlp512", "mlp64x2"])
    p.add_argument("--map", type=str, default="stage_1")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--eval_persistent", action="store_true", default=False,
                   help="--eval: the whole evaluation in ONE launch (HIP actor + env step on chip) instead of the stepping loop")
    p.add_argument("--eval_every", type=int, default=0,
                   help="training: every this many iterations, a persistent deterministic evaluation of --eval_episodes episodes "
                        "(arrival threshold 0.4) on a second set of envs; 0 = off")
    p.add_argument("--max_grad_norm", type=float, default=None,
                   help="clip each net's gradient to this L2 norm in every epoch and skip a net's step when its gradient is not finite "
                        "(on the device, inside the fused update); default: off, as in the reference")
    p.add_argument("--target_kl", type=float, default=None,
                   help="stop an update -- both nets -- before the optimiser step of the first epoch whose approx_kl exceeds 1.5 x this "
                        "(decided on the device inside the fused update; the remaining epochs cost their launches only); default: off")
    p.add_argument("--minibatch_size", type=int, default=None,
                   help="samples per optimiser step and rank, a multiple of 32: every epoch takes ceil(batch / this) steps on slices of the "
                        "batch instead of one on all of it; default (or >= the batch): full-batch epochs, as in the reference")
    p.add_argument("--minibatch_shuffle", type=str, default="epoch", choices=["epoch", "update", "none"],
                   help="with --minibatch_size: a fresh device-side permutation of the batch before every epoch (epoch), one per update "
                        "(update), or contiguous slices of the batch as it lies (none)")
    p.add_argument("--norm_reward", action="store_true", default=False,
                   help="divide every rollout's rewards by the running standard deviation of the discounted return before the return "
                        "scan (VecNormalize's norm_reward, on the device); metrics and CSVs stay raw; default: off, as in the reference")
    p.add_argument("--clip_reward", type=float, default=10.0, help="with --norm_reward: the scaled rewards are clipped to +- this")
    p.add_argument("--lr_schedule", type=str, default=None, choices=["adaptive", "linear"],
                   help="adaptive: after every optimiser step lr /= 1.5 if its approx_kl > 2 x --desired_kl, lr *= 1.5 if below half of it "
                        "(decided on the device inside the fused update; not with --target_kl); linear: lr x (1 - t / max_timesteps) per "
                        "iteration; default: the constant lr of the reference")
    p.add_argument("--desired_kl", type=float, default=0.01, help="with --lr_schedule adaptive: the KL per optimiser step the rule steers towards")
    p.add_argument("--lr_min", type=float, default=1e-5, help="with --lr_schedule adaptive: the lower clamp of the learning rate")
    p.add_argument("--lr_max", type=float, default=1e-2, help="with --lr_schedule adaptive: the upper clamp of the learning rate")
    p.add_argument("--learn_var", action="store_true", default=False,
                   help="the exploration variance is a parameter of the actor (one isotropic log-variance, as Stable-Baselines3's "
                        "log_std), stepped on the device after every optimiser step, instead of the reference's fixed decay schedule; "
                        "not with --target_kl; one GPU only; default: off")
    p.add_argument("--ent_coef", type=float, default=0.0, help="with --learn_var: the coefficient of the entropy bonus in the actor's loss")
    p.add_argument("--var_min", type=float, default=1e-3, help="with --learn_var: the lower clamp of the variance")
    p.add_argument("--var_max", type=float, default=1.0, help="with --learn_var: the upper clamp of the variance")
    p.add_argument("--bootstrap_truncated", action="store_true", default=False,
                   help="partial-episode bootstrapping: an episode cut by --timesteps_per_episode adds gamma V of its last stored "
                        "observation (rsl_rl's rule) and the envs still running at the batch end bootstrap with V of the next one, for "
                        "every lambda; collisions and arrivals stay terminal; default: off, as in the reference")
    p.add_argument("--movers", type=str, default=None,
                   help="moving obstacles cast beside the static map (maps.movers_by_name: orbit4 = four pillars orbiting the spawn "
                        "pose); authored geometry: parity unpinned (no reference geometry); default: none")
    p.add_argument("--movers_period", type=int, default=None, help="env steps per cycle of --movers (default 64)")
    p.add_argument("--movers_seed", type=int, default=0, help="the seed of --movers random:K (maps.random_mover_bank)")
    p.add_argument("--eval_movers", type=str, default=None,
                   help="training with --eval_every: the movers of the EVALUATION envs only, e.g. random:32 with another "
                        "--eval_movers_seed -- a held-out set of scenarios; default: the training world's")
    p.add_argument("--eval_movers_seed", type=int, default=1, help="the seed of --eval_movers random:K")
    p.add_argument("--scan_history", action="store_true", default=False,
                   help="the mlp64x2 policy reads the last three LiDAR scans and the action between them (a 42-column row assembled on "
                        "the device, never across an episode start) instead of one scan; needs --policy mlp64x2; default: off")
    p.add_argument("--scan_pool", type=int, default=1, choices=[1, 2, 3, 4],
                   help="sector LiDAR, training and --eval: the simulator casts 10 K rays and each of the 10 scan columns is the nearest "
                        "return of K consecutive rays (thin obstacles between the 10 beams are seen -- and hit: a harder world); needs "
                        "--policy mlp64x2; default 1: the reference's 10 beams")
    p.add_argument("--continue_rollouts", action="store_true", default=False,
                   help="only the first rollout starts from a reset: every later one continues the envs' episodes across the iteration "
                        "boundary (short rollouts on many envs); needs --bootstrap_truncated; default: off, as in the reference")
    p.add_argument("--scenario_stats", action="store_true", default=False,
                   help="with a bank of scenarios (--movers random:K | bank:...): sum every rollout per scenario on the device, log the "
                        "worst and the mean scenario's success rate and append <method>_train_scenarios.csv; default: off")
    p.add_argument("--scenario_priority", type=str, default=None, choices=["failure", "abs_adv"],
                   help="re-assign the envs to the scenarios of the bank by rank-prioritised level replay on a score per scenario: "
                        "failure = 1 - success rate, abs_adv = mean |advantage| (needs --bootstrap_truncated); implies the statistics; "
                        "default: off, every env keeps the scenario it was given")
    p.add_argument("--scenario_resample_every", type=int, default=1, help="with --scenario_priority: iterations between re-assignments")
    p.add_argument("--scenario_score_alpha", type=float, default=0.5,
                   help="with --scenario_priority: the weight of the newest iteration in a scenario's running score, in [0, 1]")
    p.add_argument("--scenario_temperature", type=float, default=0.3,
                   help="with --scenario_priority: beta of the rank weights (1 / rank)^(1 / beta); smaller = sharper")
    p.add_argument("--scenario_uniform_mix", type=float, default=0.25,
                   help="with --scenario_priority: the share of the envs spread uniformly over the scenarios, in [0, 1]")
    args = p.parse_args(argv)
    if args.output_dir is None:
        args.output_dir = os.path.join(os.getcwd(), "runs")
    if args.tiny_debug_run:  # arguments.py:58-65
        args.timesteps_per_episode, args.steps_per_iteration, args.max_timesteps = 20, 40, 400
    if args.dry_run_vision or "vision" in args.method_name.lower():
        p.error("the camera / vision modality is not part of this package (LiDAR hot path only)")
    return args


def schedule(args, world=1):
    """(n_envs_total, rollout_len): steps_per_iteration timesteps per batch spread over the envs.  By default every rollout starts
    from a reset (ppo.py:486), so a rollout shorter than the episode cap could never finish a timed-out episode: the env count is
    chosen so that rollout_len >= timesteps_per_episode (5000/500 -> 10 envs x 500 steps; 2 M/500 -> 4096 x 512).  With
    --continue_rollouts the episodes run on across the batches and --n_envs may make the rollout as short as it likes."""
    if args.n_envs:
        n_envs = args.n_envs
    else:
        n_envs = max(1, min(args.steps_per_iteration // max(args.timesteps_per_episode, 1), 4096 * world))
        n_envs = max(world, n_envs // world * world)
    rollout = max(1, -(-args.steps_per_iteration // n_envs))
    return n_envs, rollout


def config_of(args, rollout):
    """The PPOConfig of a training run: every flag that has a field."""
    from . import ppo
    return ppo.PPOConfig(rollout_len=rollout, max_episode_steps=args.timesteps_per_episode, policy=args.policy, seed=args.seed,
                         save_freq=args.save_every_iterations, output_dir=args.output_dir, method_name=args.method_name,
                         eval_every=args.eval_every, eval_episodes=args.eval_episodes, max_grad_norm=args.max_grad_norm,
                         target_kl=args.target_kl, minibatch_size=args.minibatch_size, minibatch_shuffle=args.minibatch_shuffle,
                         norm_reward=args.norm_reward, clip_reward=args.clip_reward, lr_schedule=args.lr_schedule,
                         desired_kl=args.desired_kl, lr_min=args.lr_min, lr_max=args.lr_max,
                         learn_var=args.learn_var, ent_coef=args.ent_coef, var_min=args.var_min, var_max=args.var_max,
                         bootstrap_truncated=args.bootstrap_truncated, scan_history=args.scan_history,
                         continue_rollouts=args.continue_rollouts, scenario_stats=args.scenario_stats,
                         scenario_priority=args.scenario_priority, scenario_resample_every=args.scenario_resample_every,
                         scenario_score_alpha=args.scenario_score_alpha, scenario_temperature=args.scenario_temperature,
                         scenario_uniform_mix=args.scenario_uniform_mix,
                         eval_movers=movers_of(args.eval_movers, args.movers_period, args.eval_movers_seed))


def movers_of(name, period, seed):
    """--movers / --eval_movers -> VecEnv's ``movers``: a scene name, "random:K" (a seeded bank of scenarios, one per env) or
    "bank:scene,scene,..." (maps.resolve_movers)"""
    if not name:
        return None
    if name.startswith("random:"):
        return dict(name=name, seed=seed)
    return dict(name=name, period=period)


def main(argv=None):
    args = get_args(argv)
    movers = movers_of(args.movers, args.movers_period, args.movers_seed)
    import torch
    from . import evaluate as ev
    from . import maps, ppo
    from .env import VecEnv

    if args.eval or args.mode == "test":
        path = args.actor_model or ev.find_latest_checkpoint(args.output_dir, args.method_name)
        if not path:
            print("No checkpoint found for evaluation. Exiting.", flush=True)  # main.py:161-163
            return 0
        print(f"Loading actor: {path}", flush=True)
        actor, _ = ev.load_actor(path, "cuda")
        s = ev.evaluate(actor, num_episodes=args.eval_episodes, max_timesteps_per_episode=args.timesteps_per_episode, map=args.map,
                        seed=args.seed, output_dir=args.output_dir, method_name=args.method_name, persistent=args.eval_persistent,
                        movers=movers, scan_pool=args.scan_pool)
        return 0 if s["episodes"] == args.eval_episodes else 1

    ctx = ppo.DistCtx()
    n_envs, rollout = schedule(args, ctx.world)
    lo, hi = ctx.shard(n_envs)
    sampler = None
    if args.use_external_sampler:
        world_type = "stage1" if args.map.startswith("stage") else "small_house"
        st, g, dmin, dmax = maps.spawn_tables(world_type)
        n_st, n_g = len(st), len(g)
        st, g = maps.open_tables(maps.by_name(args.map), st, g)   # drop table points inside / against walls (stage tables too:
        if ctx.rank == 0 and (len(st) < n_st or len(g) < n_g):    # the reference's stage-1 goals at +-4.0 sit inside the outer wall)
            print(f"external sampler: dropped {n_st - len(st)} start poses and {n_g - len(g)} goals that are not in open space",
                  flush=True)
        sampler = (st, g, dmin, dmax)
    env = VecEnv(hi - lo, map=args.map, max_episode_steps=args.timesteps_per_episode, auto_reset=True, is_training=True,
                 seed=args.seed, env_id_base=lo, device=ctx.device, sampler=sampler, movers=movers, scan_pool=args.scan_pool)
    cfg = config_of(args, rollout)
    trainer = ppo.PPOTrainer(env, cfg, ctx)
    if args.resume or args.actor_model:  # main.py:52-89
        pa = args.actor_model or ev.find_latest_checkpoint(args.output_dir, args.method_name, "actor")
        pc = args.critic_model or ev.find_latest_checkpoint(args.output_dir, args.method_name, "critic")
        if pa and pc:
            trainer.load_checkpoint(pa, pc)
            if ctx.rank == 0:
                print(f"Resumed from {pa}", flush=True)
    if ctx.rank == 0:
        print(f"Learning... {n_envs} envs x {rollout} steps = {n_envs * rollout} timesteps per batch, episode cap "
              f"{args.timesteps_per_episode}, total budget {args.max_timesteps} timesteps, policy {args.policy}", flush=True)
    trainer.learn(args.max_timesteps)
    if cfg.output_dir and ctx.rank == 0:
        trainer.save_checkpoint()
    ctx.barrier()
    if ctx.enabled:
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
