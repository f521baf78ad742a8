"""PPO-clip rollout / return-scan / update loop over the batched simulator.

Follows ``project_ppo/src/ppo.py`` of the reference function by function, vectorised over N envs:

  rollout()        ppo.py:463-641   T policy steps x N envs; every buffer is a [T,N,...] device tensor
                                    the step kernel writes into directly (no host round trip)
  sample_action    ppo.py:673-706   MVN(mean, var*I) sample, clamp, log-prob of the CLAMPED action
  compute returns  ppo.py:643-671   navsim_rtg_scan (HIP): reward-to-go, no bootstrap
                                    PPOConfig.bootstrap_truncated: time-outs and the batch end stop being terminal -- a time-out row
                                    bootstraps with gamma V of its own observation (rsl_rl's rule), the batch end with V(obs_buf[T]),
                                    for every lambda (navsim_gae_scan_trunc; host mirror: env.truncated_returns_reference)
  evaluate         ppo.py:708-737
  update           ppo.py:275-397   A = rtg - V, normalised with the unbiased std (+1e-10); 50 full-batch
                                    epochs of clipped surrogate + MSE critic, Adam(lr 3e-4), no entropy
                                    term, no value clip, no gradient clipping (PPOConfig.max_grad_norm
                                    turns on per-net clipping + a non-finite guard; the gradient-norm
                                    check of ppo.py:356-379,414-416 is train_log.grad_guard)
                                    PPOConfig.minibatch_size: K optimiser steps per epoch on slices of the batch, shuffled
                                    on the device (navppo_shuffle_batch; host mirror: batch_permutation)
                                    PPOConfig.lr_schedule: "adaptive" = the learning rate follows every step's approx_kl, decided
                                    on the device (navppo_*_update_epoch_lr; host mirror: adaptive_lr_reference); "linear" = decay
                                    over learn()'s budget, set per iteration
                                    PPOConfig.learn_var: log var is a parameter of the actor, stepped on the device after every
                                    optimiser step, with an entropy bonus ent_coef (navppo_*_update_epoch_var; host mirror:
                                    learned_var_reference); the fixed decay schedule is off
                                    PPOConfig.scenario_stats / scenario_priority: on a bank of mover tapes the rollout is summed per
                                    scenario on the device (navppo_group_sums; host mirror: group_sums_reference) and the envs are
                                    re-assigned to the scenarios by rank-prioritised level replay (scenarios.ScenarioSampler)
  learn            ppo.py:218-461   iteration loop, timing, checkpoints (actor_iter%04d_step%08d.pth)

Multi-GPU (absent in the reference): one process per GPU, each owns a contiguous shard
of env ids; after each backward ONE all-reduce (RCCL over xGMI; gloo on CPU for tests) of the single
flat gradient buffer holding actor+critic; the advantage mean/std come from all-reduced
(sum, sum of squares, count) so they equal the single-process values of ppo.py:284.

This module is the import surface and holds no code of its own: rollout, iteration and learn live in trainer.py (PPOTrainer), update
and evaluate in updater.py (PPOUpdater), the options and their checks in config.py, the host mirrors in minibatch.py, reward_norm.py and
lr_schedule.py, the per-scenario sums, the scenario sampler and the scenario table in scenarios.py, the ranks in distributed.py.
  train_log.py    what an iteration writes: progress line, scalars.jsonl, TensorBoard, episode CSV, grad_diagnostics.txt (RunLog)
  checkpoint.py   the two reference-named state_dict files and the <kind>_<tag>.pth sidecars beside them
  evaluate.py     main.evaluate, and the periodic evaluation of PPOConfig.eval_every (make_eval_env, evaluate_params)
"""
import torch.distributed as dist  # noqa: F401

from .config import (LR_SCHEDULES, MINIBATCH_SHUFFLES, SCENARIO_PRIORITIES, PPOConfig, check_bootstrap_config,  # noqa: F401
                     check_continue_config, check_learn_var_config, check_lr_schedule_config, check_minibatch_config,
                     check_reward_norm_config, check_scan_history_config, check_scenario_config, check_update_config)
from .distributed import DistCtx, SingleProcessCtx, as_ctx, global_mean  # noqa: F401
from .explore_var import VAR_STATE_LEN, learned_var_reference, var_state_init  # noqa: F401
from .lr_schedule import LR_FACTOR, adaptive_lr_direction, adaptive_lr_reference, linear_lr  # noqa: F401
from .minibatch import batch_permutation, minibatch_counter, minibatch_key  # noqa: F401
from .reward_norm import RET_RMS_INIT, merge_return_moments, return_moments, reward_norm_reference, reward_scale  # noqa: F401
from .scenarios import GROUP_SUMS_COLS, ScenarioSampler, group_sums, group_sums_reference  # noqa: F401
from .trainer import PPOTrainer  # noqa: F401
from .updater import ADAM_HYPER, LOG_2PI, FlatParams, PPOUpdater, gaussian_log_prob, normalise_advantages, ppo_losses  # noqa: F401
