"""PPO.learn for a VecEnv shard (ppo.py:218-461): the loop -- rollout, return scan, update -- and the device state it runs on.  What
an iteration writes is train_log.py's, the checkpoint files are checkpoint.py's, the periodic evaluation is evaluate.py's."""
import ctypes as C
import functools
import math
import os
import time

import numpy as np
import torch

from . import checkpoint, nets, train_log
from ._native import _navppo, _ptr, check, lib
from .config import (PPOConfig, check_bootstrap_config, check_continue_config, check_learn_var_config, check_reward_norm_config,
                     check_scan_history_config, check_scenario_config)
from .distributed import as_ctx
from .env import HIST_CARRY, HIST_DIM, check_scan_pool, gae_scan, gae_scan_trunc, rtg_scan, stack_rows
from .evaluate import evaluate_params, make_eval_env
from .lr_schedule import linear_lr
from .reward_norm import RET_RMS_INIT, return_moments, reward_scale
from .scenarios import GROUP_SUMS_COLS, SCENARIO_CSV_HEADER, ScenarioSampler, group_sums, scenario_rows
from .updater import PPOUpdater, gaussian_log_prob


class PPOTrainer:
    """PPO.learn for a ``VecEnv`` shard.  Construct one per process (= per GPU)."""

    # Class-level defaults.  __init__ sets every attribute a trainer reads; these two are ALSO there on a trainer that never ran it:
    # the CPU tests build bare trainers (PPOTrainer.__new__, cfg and a few attributes, one method), and the methods they call --
    # save_checkpoint / load_checkpoint, tb_scalars, _grad_guard, learn -- read nothing else beyond the state of an option cfg has on.
    scenarios = None   # the ScenarioSampler of scenario_stats / scenario_priority (None: both off)
    _log = None        # the RunLog of the run's files, created at the first write (_run_log)

    @property
    def scan_pool(self):
        """the env's scan_pool as it stands now (1 on an env without one)"""
        return getattr(getattr(getattr(self, "env", None), "sim", None), "scan_pool", 1)

    def __init__(self, env, cfg=None, ctx=None):
        self.env, self.cfg = env, cfg or PPOConfig()
        self.ctx = ctx = as_ctx(ctx)
        self.device = env.device
        cfg = self.cfg
        N, T, D = env.N, cfg.rollout_len, env.D
        check_scan_history_config(cfg)
        # sector LiDAR is the env's option (VecEnv(scan_pool=k)): the trainer only refuses what its kernels lack and logs k
        check_scan_pool(self.scan_pool, env.B, policy=cfg.policy)
        self.scan_history = cfg.scan_history
        if self.scan_history:
            if env.B != 10:
                raise ValueError(f"scan_history needs n_beams == 10 (the history row stacks 10-beam scans), not {env.B}")
            if self.device.type != "cuda":
                raise ValueError("scan_history runs on the GPU only: the history rows are built by HIP kernels")
        # the width of the rows the nets read: the env's rows, or the scan-history rows built from them
        self.net_dim = HIST_DIM if self.scan_history else D
        torch.manual_seed(cfg.seed)  # same initial weights on every rank (then broadcast anyway)
        self.actor, self.critic = nets.make_policy(cfg.policy, self.net_dim, 2)
        self.actor.to(self.device)
        self.critic.to(self.device)
        self.updater = PPOUpdater(self.actor, self.critic, cfg, ctx, self.device)
        if self.scan_history and not (self.updater.fused_mlp64 and self.uses_persistent_rollout):
            raise ValueError("scan_history needs the persistent rollout and the fused update of policy 'mlp64x2' on the GPU")
        torch.manual_seed(cfg.seed * 1000003 + 17 + ctx.rank)  # exploration noise differs per shard
        dev = self.device
        f32, u8 = torch.float32, torch.uint8
        # the observation rows in the dtype the simulator writes them (float16 on an obs_f16 env: BASELINE configs[4]); half rows
        # are read directly by the fused kernels of both policies (round 6: the 512-wide ones too), a PyTorch policy widens them
        self.obs_buf = torch.zeros((T + 1, N, D), dtype=env.sim.obs_dtype, device=dev)
        self._half_obs = env.sim.obs_dtype == torch.float16
        # scan_history: the rows the nets read, built from obs_buf and ended_buf behind every rollout (navsim_stack_rows); obs_buf
        # stays what the simulator writes, 16 columns wide
        self.hist_buf = torch.zeros((T + 1, N, self.net_dim), dtype=env.sim.obs_dtype, device=dev) if self.scan_history else None
        self.act_buf = torch.zeros((T, N, 2), dtype=f32, device=dev)
        self.logp_buf = torch.zeros((T, N), dtype=f32, device=dev)
        self.rew_buf = torch.zeros((T, N), dtype=f32, device=dev)
        self.done_buf = torch.zeros((T, N), dtype=u8, device=dev)
        self.arrive_buf = torch.zeros((T, N), dtype=u8, device=dev)
        self.ended_buf = torch.zeros((T, N), dtype=u8, device=dev)
        self.epret_buf = torch.zeros((T, N), dtype=f32, device=dev)
        self.eplen_buf = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.eppath_buf = torch.zeros((T, N), dtype=f32, device=dev)
        self.rtg_buf = torch.zeros((T, N), dtype=f32, device=dev)
        check_reward_norm_config(cfg)
        check_bootstrap_config(cfg)
        check_continue_config(cfg)
        # continue_rollouts (off: not one tensor or launch more than before): whether the next rollout must reset, the generation of
        # the world the envs were last reset in, with scan_history the two history carries that take turns -- [0] belongs to row 0 of
        # the batch at hand, [1] receives row T's -- and with norm_reward the running return behind the last row (SB3's self.returns)
        self.continue_rollouts = cfg.continue_rollouts
        self._reset_pending, self._reset_gen, self._did_reset = True, None, True
        if self.continue_rollouts:
            if self.scan_history:
                self._hist_carry = [torch.zeros((N, HIST_CARRY), dtype=f32, device=dev) for _ in range(2)]
            if cfg.norm_reward:
                self._ret_carry = torch.zeros(N, dtype=torch.float64, device=dev)
        if cfg.norm_reward:   # (off: not one tensor, launch or read-back more than before)
            self._init_ret_rms(dev)
            self.rew_scaled_buf = torch.zeros((T, N), dtype=f32, device=dev)   # what the scans read; rew_buf keeps the raw rewards
            self._ret_rows = torch.zeros((ctx.world, 3), dtype=torch.float64, device=dev)   # one row per rank
        self.var = torch.full((), cfg.init_var, dtype=f32, device=dev)  # ppo.py:123-124 (0.8 * I)
        check_learn_var_config(cfg, ctx.world)
        if cfg.learn_var:   # a view of the updater's state: every rollout path reads the variance the last optimiser step left
            self.var = self.updater.var_state[1]
        self.var_host = float(cfg.init_var)   # host mirror, refreshed at every rollout start
        self._lo = torch.tensor([0.0, -1.0], device=dev)
        self._hi = torch.tensor([1.0, 1.0], device=dev)
        self._graph = self._graph_gen = None   # the captured hipGraph of per-step launches, and the generation of the world it froze
        self._gae = None        # (raw advantages, V) of the last rollout where a GAE scan ran
        self._sums_ws = None    # navppo_episode_sums' workspace, allocated by the first _rollout_metrics_dev
        self._eval_env = None   # the evaluation envs of eval_every, created by the first evaluate_now
        self._step_base = torch.zeros((), dtype=torch.int32, device=dev)  # rollout steps taken so far (noise counter)
        self._act_seed = (cfg.seed * 0x9E3779B97F4A7C15 + 0xAC7) & 0xFFFFFFFFFFFFFFFF
        self._env_id_base = int(env.sim.cfg.env_id_base)
        check_scenario_config(cfg)
        self.scenarios = None   # (both options off: not one tensor, launch, collective or log key more than before)
        if cfg.scenario_stats or cfg.scenario_priority is not None:
            self._init_scenarios()
        self.t_so_far = 0     # completed-episode steps, as the reference counts (ppo.py:258)
        self.env_steps = 0    # all simulated steps
        self.i_so_far = 0
        self.episode_starts = 0
        self.logger = {}

    @property
    def ctx(self):
        """the ranks of the run: a DistCtx, or the single-process context (also when None was assigned)"""
        return self._ctx

    @ctx.setter
    def ctx(self, ctx):
        self._ctx = as_ctx(ctx)

    @property
    def writes_files(self):
        """rank 0 alone logs, evaluates and writes checkpoints, CSVs and diagnostics"""
        return self.ctx.rank == 0

    # ---- PPOConfig.norm_reward: the running statistics of the discounted return and the scaled copy of a rollout's rewards
    def _init_ret_rms(self, device, mean=RET_RMS_INIT[0], var=RET_RMS_INIT[1], count=RET_RMS_INIT[2]):
        """ret_rms = (mean, var, count, scale), float64 on the device; a fresh run starts like RunningMeanStd (0, 1, 1e-4)."""
        mean, var, count = float(mean), float(var), float(count)
        self.ret_rms = torch.tensor([mean, var, count, 1.0 / math.sqrt(var + self.cfg.norm_reward_eps)], dtype=torch.float64, device=device)

    def _normalise_rewards(self):
        """Behind the rollout, in front of the return scan: this rank's (n, mean, M2) of the rollout's running returns (carry-in 0:
        the rollout starts from a reset -- or, with continue_rollouts, the running return the last rollout left, zeroed whenever the
        envs are reset), every rank's row gathered by ONE all-reduce of a zero-filled [world, 3] tensor (adding
        zeros is exact), all rows merged in rank order on every rank -- bit-identical statistics -- and the rollout scaled by them.
        Two entry points, no host round trip."""
        cfg, ctx = self.cfg, self.ctx
        rows = self._ret_rows
        if ctx.enabled and rows.shape[0] > 1:
            rows.zero_()
        carry = self._ret_carry if cfg.continue_rollouts else None   # (the tensor is there with the option alone)
        return_moments(self.rew_buf, self.ended_buf, cfg.gamma, carry=carry, out=rows[ctx.rank])
        ctx.all_reduce_sum(rows)
        return reward_scale(self.ret_rms, rows, self.rew_buf, clip=cfg.clip_reward, eps=cfg.norm_reward_eps, out=self.rew_scaled_buf)

    def _reward_norm_figures_dev(self):
        """(mean, var, count, scale, explained variance) as one float64 device tensor, queued behind the update and read with the
        iteration's one read-back.  explained_variance = 1 - Var(target - V0) / Var(target) over this rank's samples, V0 the critic
        before the update: scale-free, unlike critic_loss, whose units change with the option."""
        tgt, v0 = self.rtg_buf.reshape(-1).double(), self.updater._last_V0.reshape(-1).double()
        ev = 1.0 - (tgt - v0).var(unbiased=False) / tgt.var(unbiased=False)
        return torch.cat([self.ret_rms, ev.reshape(1)])

    # ---- PPOConfig.scenario_stats / scenario_priority: the rollout summed per scenario, and the envs re-assigned by what it shows
    def _init_scenarios(self):
        cfg, env, sim = self.cfg, self.env, self.env.sim
        K = int(getattr(sim, "movers_tapes", 0) or 0)
        if getattr(env, "mover_bank", None) is None or K < 2:
            raise ValueError("scenario_stats / scenario_priority need an env whose movers are a bank of at least 2 tapes "
                             "(VecEnv movers='random:K', 'bank:a,b,...' or dict(bank=...))")
        if self.device.type != "cuda":
            raise ValueError("scenario_stats / scenario_priority run on the GPU only: the sums are a HIP kernel's")
        self._n_global = env.N * self.ctx.world   # (DistCtx.shard cuts the global envs into equal shards)
        if self._env_id_base + env.N > self._n_global:
            raise ValueError("scenario_stats / scenario_priority: the shards of the run must hold the same number of envs")
        # stats alone: the score the table shows is the failure rate, and nothing is ever re-assigned
        self.scenarios = ScenarioSampler(K, mode=cfg.scenario_priority or "failure", alpha=cfg.scenario_score_alpha,
                                         temperature=cfg.scenario_temperature, uniform_mix=cfg.scenario_uniform_mix, seed=cfg.seed)
        self._scen_K, self._scen_cols = K, GROUP_SUMS_COLS
        self._scen_ws = torch.empty(int(lib().navppo_group_sums_ws_bytes(cfg.rollout_len, env.N, K)), dtype=torch.uint8, device=self.device)
        self._scen_ids_host = None   # every rank's ids, on the host (filled when the table first needs them)

    def _scenario_envs(self):
        """[K] envs per scenario over ALL ranks (the table's column): from the sampler's last assignment, or -- nothing re-assigned yet
        -- from the constructor's rule for every global env"""
        if self._scen_ids_host is None:
            bank, env = self.env.mover_bank, self.env
            if isinstance(bank.assign, str):
                self._scen_ids_host = bank.tape_ids(self._n_global, map_seed=env._map_seed, env_id_base=0)
            else:   # explicit ids: this rank's alone are known
                self._scen_ids_host = env.sim.movers_tape_id.cpu().numpy()
        return np.bincount(np.asarray(self._scen_ids_host), minlength=self._scen_K)

    def _scenario_sums_dev(self):
        """navppo_group_sums behind navppo_episode_sums: this rank's [K, 8] table, flat (the caller all-reduces it with the six sums)"""
        T, N = self.cfg.rollout_len, self.env.N
        adv = self._gae[0].reshape(T, N) if (self.cfg.scenario_priority == "abs_adv" and self._gae is not None) else None
        return group_sums(self.ended_buf, self.arrive_buf, self.done_buf, self.eplen_buf, self.epret_buf, self.env.sim.movers_tape_id,
                          self._scen_K, adv=adv, workspace=self._scen_ws).reshape(-1)

    def _scenario_step(self, G):
        """After the read-back (i_so_far already counts the iteration): the scores take in the iteration's global [K, 8] sums, the log
        and the table are written, and -- with scenario_priority, every scenario_resample_every iterations -- the envs get their next
        scenarios (the stream is idle)."""
        cfg, smp = self.cfg, self.scenarios
        G = np.asarray(G, dtype=np.float64).reshape(self._scen_K, self._scen_cols)
        smp.observe(G)
        played = G[:, 0] > 0
        rate = G[played, 1] / G[played, 0]
        out = dict(train_scenario_success_min=float(rate.min()) if rate.size else float("nan"),
                   train_scenario_success_mean=float(rate.mean()) if rate.size else float("nan"))
        self.scenario_table = self.scenario_rows(G)
        if cfg.output_dir and self.writes_files:
            train_log.append_rows(self._run_log().path("train_scenarios.csv"), SCENARIO_CSV_HEADER,
                                  [[r[h] for h in SCENARIO_CSV_HEADER] for r in self.scenario_table])
        if cfg.scenario_priority is not None and self.i_so_far % cfg.scenario_resample_every == 0:
            ids = smp.assign(self._n_global)
            self._scen_ids_host = ids
            self.env.assign_scenarios(ids[self._env_id_base:self._env_id_base + self.env.N])   # bumps sim.generation
        return out

    def scenario_rows(self, G):
        """the rows of <method>_train_scenarios.csv from the global [K, 8] sums of an iteration (scenarios.scenario_rows)"""
        return scenario_rows(G, self._scenario_envs(), self.scenarios, self.i_so_far)

    def _fused_act(self, t, noise=None):
        """PPO.get_action for all envs in ONE launch (csrc/ppo_mlp64.hip: mlp64_act, csrc/ppo_resmlp512.hip: resmlp_act)."""
        up = self.updater
        _navppo(up.fused + "_act", _ptr(up.fp.flat), *up._obs_args(self.obs_buf[t]), _ptr(noise), self.env.N, _ptr(self.var), self._act_seed,
                self._env_id_base, _ptr(self._step_base), t, _ptr(self.act_buf[t]), _ptr(self.logp_buf[t]), None)

    # ---- ppo.py:673-706 + env.step, for rollout step t (all envs)
    def _rollout_step(self, t):
        if self.updater.fused:
            self._fused_act(t)
        else:
            obs = self.obs_buf[t].float()
            mean = self.actor(obs)
            std = torch.sqrt(self.var)
            raw = torch.addcmul(mean, torch.randn_like(mean), std)          # dist.sample(), ppo.py:698
            act = self.act_buf[t]
            torch.clamp(raw, self._lo, self._hi, out=act)                   # ppo.py:700-703
            self.logp_buf[t] = gaussian_log_prob(mean, act, self.var)       # log-prob of the clamped action, :704
        self.env.sim.step(self.act_buf[t], self.obs_buf[t + 1], self.rew_buf[t], self.done_buf[t], self.arrive_buf[t],
                          self.ended_buf[t], self.epret_buf[t], self.eplen_buf[t], ep_path=self.eppath_buf[t])

    def _persistent_rollout(self):
        """ppo.py:505-594 in ONE launch (csrc/navsim.hip: rollout_kernel): policy step and env step alternate inside the
        kernel; same device functions and Philox keys as the per-step path, so the buffers come out bit-identical."""
        sim = self.env.sim
        name = "navsim_rollout_" + ("resmlp512" if self.updater.fused_resmlp512 else "mlp64_hist" if self.scan_history else "mlp64")
        carries = ()
        if self.scan_history and self.continue_rollouts:   # the carry of row 0 in (none behind a reset), the carry of row T out
            name += "_cont"
            carries = (None if self._did_reset else _ptr(self._hist_carry[0]), _ptr(self._hist_carry[1]))
        with torch.cuda.device(self.device):
            check(getattr(lib(), name)(sim._h, _ptr(self.updater.fp.flat), _ptr(self.obs_buf), _ptr(self.act_buf), _ptr(self.logp_buf),
                                       _ptr(self.rew_buf), _ptr(self.done_buf), _ptr(self.arrive_buf), _ptr(self.ended_buf),
                                       _ptr(self.epret_buf), _ptr(self.eplen_buf), _ptr(self.eppath_buf), _ptr(self.var), self._act_seed,
                                       _ptr(self._step_base), self.cfg.rollout_len, *carries,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
        self._step_base += self.cfg.rollout_len

    def _rollout_body(self):
        for t in range(self.cfg.rollout_len):
            self._rollout_step(t)
        self._step_base += self.cfg.rollout_len  # inside the captured graph: every replay draws fresh noise

    @property
    def uses_persistent_rollout(self):
        """All T steps of PPO.rollout in ONE launch: navsim_rollout_mlp64 (the (B + 6)-64-64 actor, 10 or 36 beams, float32 or float16
        rows) or navsim_rollout_resmlp512 (the reference's 512-wide actor, 10 beams, float32 or float16 rows).  Anything else runs the
        hipGraph of per-step launches."""
        return bool(self.cfg.persistent_rollout and ((self.updater.fused_mlp64 and self.env.B in (10, 36)) or
                                                     (self.updater.fused_resmlp512 and self.env.B == 10)))

    @property
    def net_obs(self):
        """[T + 1, N, .]: the rows the nets read -- obs_buf, or with scan_history the history rows built from it"""
        return self.hist_buf if self.scan_history else self.obs_buf

    @torch.no_grad()
    def rollout(self):
        self._collect()
        if self.scan_history:
            self._stack_history()
        self._compute_returns()
        self.env_steps += self.cfg.rollout_len * self.env.N

    def _collect(self):
        """T steps of all envs into the [T, N] buffers: ONE persistent launch, the replay of the captured hipGraph of per-step launches
        (captured here, behind a warm-up step, the first time and after a change of the world), or the per-step launches themselves."""
        cfg = self.cfg
        self._decay_exploration()
        self.epret_buf.zero_()
        self.eplen_buf.zero_()
        self.updater.invalidate_prepared()   # the kernels below rewrite obs_buf behind torch's version counter
        graph_path = not self.uses_persistent_rollout and cfg.use_graph and self.device.type == "cuda"
        if graph_path and self._graph is not None and self._graph_gen != self.env.sim.generation:
            self._graph = None   # set_map / set_spawn_sampler / set_goal_rects re-allocated what the capture froze
        self._begin_rollout(capturing=graph_path and self._graph is None)
        # (round 5: both rollout kernels have the tile-box cast of shared 65..4096-segment maps; until then shards up to 4096 envs on
        # such a map took the hipGraph of per-step launches)
        if self.uses_persistent_rollout:
            self._persistent_rollout()
        elif graph_path:
            if self._graph is None:
                self._graph_gen = self.env.sim.generation
                s = torch.cuda.Stream(self.device)
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):  # warm-up outside capture (allocator, hipBLASLt workspaces)
                    self._rollout_step(0)
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                self.env.sim.reset(self.obs_buf[0])   # (the warm-up stepped the envs; _begin_rollout made this a rollout that resets)
                self._graph = torch.cuda.CUDAGraph()
                # thread_local: other threads (the RCCL watchdog of torch.distributed) may touch the HIP runtime while
                # this thread captures; the default global mode would turn that into a capture error on multi-GPU runs
                with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
                    self._rollout_body()
            self._graph.replay()
        else:
            self._rollout_body()

    def _stack_history(self):
        """scan_history: the batch the nets read, [T + 1, N, 42], from obs_buf and ended_buf: one bandwidth kernel per iteration"""
        self.updater.invalidate_prepared()   # hist_buf is rewritten behind torch's version counter too
        if self.continue_rollouts:   # row 0 continues from its carry, so hist_buf[T] is the exact row the value bootstrap reads
            stack_rows(self.obs_buf, self.ended_buf, out=self.hist_buf, carry_in=None if self._did_reset else self._hist_carry[0])
            self._hist_carry.reverse()   # what the launch wrote for row T is the next batch's row 0's
        else:
            stack_rows(self.obs_buf, self.ended_buf, out=self.hist_buf)

    def _compute_returns(self):
        """rtg_buf, the critic's targets, from the rewards (norm_reward: scaled first; the scans are the same either way), and
        _gae = (raw advantages, V) where a GAE scan ran -- None behind the reference's reward-to-go (ppo.py:619 -> 643-671).
        gae_lambda alone, lambda < 1: the envs still running at the batch end are bootstrapped with V(obs_buf[T]), the observation
        behind the last row (an env that ended on the last row has ended[T-1] set, which cuts the bootstrap).  lambda = 1 keeps the
        reference's convention -- the batch end is terminal, ppo.py:601,658-666 -- and stays bit-identical to compute_rtgs.
        bootstrap_truncated: neither a time-out nor the batch end is the end of the robot.  V of all T + 1 stored rows; a time-out row
        adds gamma V of its own observation (the terminal observation is gone: the step kernels store the reset one), the envs still
        running on the last row bootstrap with V(obs_buf[T]) (ended[T-1] cuts that for an env that ended there) -- for every
        lambda; None runs as 1: the reference's A = R - V on truncation-aware returns.  rew is in the critic's units either way."""
        cfg = self.cfg
        self._gae = None
        rew = self._normalise_rewards() if cfg.norm_reward else self.rew_buf
        trunc, lam = cfg.bootstrap_truncated, cfg.gae_lambda
        if not trunc and lam is None:
            rtg_scan(rew, self.ended_buf, cfg.gamma, out=self.rtg_buf)
            return
        # extension: the critic's values of the stored observations -> lambda-returns (critic targets) and advantages
        T, N, D = cfg.rollout_len, self.env.N, self.net_dim
        lam = 1.0 if lam is None else lam
        boot = trunc or lam < 1.0   # V(obs_buf[T]) bootstraps the last row
        Vall = self.updater.value(self.net_obs[:T + 1 if boot else T].reshape(-1, D)).reshape(-1, N)
        V = Vall[:T].contiguous()
        last = Vall[T] if boot else None
        if trunc:
            adv, ret = gae_scan_trunc(rew, self.ended_buf, self.done_buf, self.arrive_buf, V, cfg.gamma, lam, last_value=last)
        else:
            adv, ret = gae_scan(rew, self.ended_buf, V, cfg.gamma, lam, last_value=last)
        self.rtg_buf.copy_(ret)
        self._gae = (adv.reshape(T * N), V.reshape(T * N))

    def reset_envs(self):
        """continue_rollouts: the next rollout starts from a reset of all envs (as the first one does, and the one behind a change of
        the world or load_checkpoint).  Without the option every rollout does anyway."""
        self._reset_pending = True

    def _begin_rollout(self, capturing=False):
        """Row 0 of the batch.  ppo.py:486: every batch starts from a reset -- the rule unless continue_rollouts, and then still the
        rule of the first rollout, of one behind reset_envs() / load_checkpoint, of one in a world whose generation changed and of
        one that captures its graph (the warm-up steps the envs).  Otherwise the envs go on: the handle holds their state, and the
        observations they stopped at, row T of the last batch, become row 0."""
        sim = self.env.sim
        self._did_reset = (not self.continue_rollouts or self._reset_pending or capturing or self._reset_gen != sim.generation)
        if self._did_reset:
            sim.reset(self.obs_buf[0])
            if self.continue_rollouts:
                self._reset_pending, self._reset_gen = False, sim.generation
                if self.cfg.norm_reward:
                    self._ret_carry.zero_()
        else:
            self.obs_buf[0].copy_(self.obs_buf[self.cfg.rollout_len])

    def _decay_exploration(self):
        """ppo.py:694-695 multiplies the covariance by 0.995 at every episode start once t_so_far > 50000 while
        it is >= 0.1, with t_so_far frozen during a rollout.  With N envs there are N x more episode starts per
        iteration, so the decay is applied once per N episode starts (per mean episode) -- identical for N=1
        up to being applied at the rollout boundary; documented deviation."""
        cfg = self.cfg
        v = float(self.var)   # the one read-back of the iteration, at its start (the stream is idle here)
        if cfg.learn_var:   # the update steps the variance; the schedule is off
            pass
        elif self.t_so_far > cfg.var_decay_after:
            k = int(round(self.episode_starts / max(self.env.N, 1)))
            for _ in range(k):
                if v >= cfg.var_floor:
                    v *= cfg.var_decay
            self.var.fill_(v)
        self.var_host = v
        self.episode_starts = 0

    def _rollout_metrics_dev(self):
        """The six sums behind the iteration's episode metrics as ONE device tensor (all-reduced over the ranks); nothing
        here waits for the GPU, so the update can be queued behind it.  With scenario_stats / scenario_priority the [K, 8] sums per
        scenario follow the six in the same tensor: one more launch, the same ONE collective.  Returns (tensor, its sections as
        train_log.join_sections names them: "episodes", then "scenarios")."""
        if self._sums_ws is None:
            self._sums_ws = torch.empty(256 * 6, dtype=torch.float64, device=self.device)
        m = torch.empty(6, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _navppo("navppo_episode_sums", _ptr(self.ended_buf), _ptr(self.arrive_buf), _ptr(self.done_buf), _ptr(self.eplen_buf),
                    _ptr(self.epret_buf), self.ended_buf.numel(), _ptr(m), _ptr(self._sums_ws))
        m, sections = train_log.join_sections([("episodes", m)] + ([] if self.scenarios is None else [("scenarios", self._scenario_sums_dev())]))
        self.ctx.all_reduce_sum(m)
        return m, sections

    def _rollout_metrics(self, m=None):
        m = self._rollout_metrics_dev()[0] if m is None else m   # (a tensor, or the six figures already on the host)
        ep, succ, coll, tmo, steps, ret = [float(x) for x in (m.tolist() if torch.is_tensor(m) else m)]
        self.episode_starts = ep / self.ctx.world + (self.env.N if self._did_reset else 0)   # (the reset started N episodes)
        return dict(episodes=int(ep), successes=int(succ), collisions=int(coll), timeouts=int(tmo),
                    completed_steps=int(steps), avg_ep_rews=(ret / ep if ep else 0.0),       # ppo.py:833
                    avg_ep_lens=(steps / ep if ep else 0.0), success_rate=(succ / ep if ep else 0.0))

    def iteration(self):
        """One pass of the loop of PPO.learn (ppo.py:241-459).  Rollout, metric sums and update are queued back to back and
        the host waits once, at the end; rollout / update times come from events on the stream (wall clock on CPU)."""
        cfg = self.cfg
        cuda = self.device.type == "cuda"
        T, N, D = cfg.rollout_len, self.env.N, self.net_dim
        t0 = time.time()
        if cuda:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        self.rollout()
        if cuda:
            ev[1].record()
        t1 = time.time()
        m, sections = self._rollout_metrics_dev()
        stats = self.updater.update(self.net_obs[:T].reshape(T * N, D), self.act_buf.reshape(T * N, 2),
                                    self.logp_buf.reshape(T * N), self.rtg_buf.reshape(T * N),
                                    self.var_host if self.updater.fused else self.var,
                                    **({} if self._gae is None else dict(adv_raw=self._gae[0], V0=self._gae[1])))
        if cuda:
            ev[2].record()
        if cfg.norm_reward:   # the option's figures ride on the episode sums' read-back below: one tensor, one copy
            rn = self._reward_norm_figures_dev()   # (behind the collective: every rank's own figures)
            m, sections = torch.cat([m, rn]), sections + [("reward_norm", rn.numel())]
        if cuda:
            torch.cuda.synchronize(self.device)
        t2 = time.time()
        if cuda:   # the host ran ahead of the stream: split the wall clock of the iteration by the stream's own stamps
            r_ms, u_ms = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
            t1 = t0 + (t2 - t0) * r_ms / max(r_ms + u_ms, 1e-9)
        back = train_log.split_sections(m, sections)   # the one read-back (the six alone: still the tensor, read by _rollout_metrics)
        if cfg.norm_reward:
            mean, var, _, scale, expl = back["reward_norm"]   # (_reward_norm_figures_dev)
            stats = dict(stats, reward_scale=scale, ret_rms_mean=mean, ret_rms_std=math.sqrt(max(var, 0.0)), explained_variance=expl)
        metrics = self._rollout_metrics(back["episodes"])
        world = self.ctx.world
        if cfg.bootstrap_truncated:   # the share of rows the scan bootstrapped as time-outs: the episode sums' figure, nothing launched
            stats = dict(stats, bootstrapped_frac=metrics["timeouts"] / max(T * N * world, 1))
        self.t_so_far += metrics["completed_steps"]
        self.i_so_far += 1
        if "scenarios" in back:
            stats = dict(stats, **self._scenario_step(back["scenarios"]))
        self._grad_guard(stats)
        self.logger = dict(metrics, **stats, iteration=self.i_so_far, t_so_far=self.t_so_far,
                           rollout_time=t1 - t0, update_time=t2 - t1, iter_time=t2 - t0,
                           steps_per_sec=T * N * world / (t2 - t0),                      # ppo.py:855
                           rollout_steps_per_sec=T * N * world / (t1 - t0),
                           # (learn_var: `var` is the update's figure -- what it ended on, what the next rollout draws with)
                           **(dict(rollout_var=self.var_host) if cfg.learn_var else dict(var=self.var_host)),
                           **(dict(scan_pool=self.scan_pool) if self.scan_pool != 1 else {}))   # (off: no key)
        if cfg.eval_every > 0 and self.i_so_far % cfg.eval_every == 0 and self.writes_files:
            self.logger.update(self.evaluate_now())   # rank 0 alone, no collective: the other ranks go on to their next rollout
        if cfg.output_dir and self.writes_files:
            if self.i_so_far % cfg.save_freq == 0:
                self.save_checkpoint()
            train_log.append_json_line(os.path.join(self.log_dir(), "scalars.jsonl"),
                                       dict(self.tb_scalars(), iteration=self.i_so_far, t_so_far=self.t_so_far))
            if cfg.episode_csv_rows:
                self.write_episode_csv(cfg.episode_csv_rows)
            self.write_tensorboard()
        return self.logger

    @property
    def stats(self):
        """the last iteration's figures (what iteration() returned)"""
        return self.logger

    def learn(self, total_timesteps, log=print):
        # The reference counts only COMPLETED episodes toward the budget (ppo.py:258); if a configuration never completes
        # one (rollout shorter than the episode cap) its loop would spin forever -- bound the iterations by the budget in
        # simulated steps instead of hanging.
        per_iter = self.cfg.rollout_len * self.env.N * self.ctx.world
        max_iters = 4 * (-(-int(total_timesteps) // per_iter)) + 4
        while self.t_so_far < total_timesteps and self.i_so_far < max_iters:  # ppo.py:245
            if self.cfg.lr_schedule == "linear":
                self.updater.set_lr(linear_lr(self.cfg.lr, self.t_so_far, total_timesteps))
            lg = self.iteration()
            if log and self.writes_files:
                log(train_log.progress_line(lg))
        return self.logger

    # ---- periodic evaluation (PPOConfig.eval_every)
    def evaluate_now(self):
        """evaluate.evaluate_params on the evaluation envs (created at the first call).  Reads the flat parameter buffer the update
        writes and nothing of the training env (its state, RNG counters, the noise counter and the captured graph are untouched).
        Returns the eval_* figures and appends one row to <method>_eval_history.csv."""
        cfg, up = self.cfg, self.updater
        if not (up.fused_mlp64 or up.fused_resmlp512):
            raise ValueError(f"PPOConfig.eval_every: no evaluation kernel for policy {cfg.policy!r} on this update path "
                             "(it needs the fused HIP update's flat parameter layout)")
        if self._eval_env is None:
            self._eval_env = make_eval_env(self.env, cfg, self.device)
        out = evaluate_params(self._eval_env, up.fp.flat, "resmlp512" if up.fused_resmlp512 else "mlp64x2", self.scan_history,
                              cfg.eval_episodes)
        if cfg.output_dir:
            figures = ("episodes", "success", "collision", "timeout", "length", "return", "path_length")
            train_log.append_rows(self._run_log().path("eval_history.csv"), self.EVAL_HISTORY_HEADER,
                                  [[self.i_so_far, self.t_so_far] + [out["eval_" + k] for k in figures]])
        return out

    # ---- the run's files: forwards to train_log.py, under the names the tests and tools/ call
    EPISODE_CSV_HEADER, EVAL_HISTORY_HEADER = train_log.EPISODE_CSV_HEADER, train_log.EVAL_HISTORY_HEADER

    def _run_log(self):
        if self._log is None:
            self._log = train_log.RunLog(self.cfg)
        return self._log

    def log_dir(self):
        return self._run_log().log_dir

    def tb_dir(self):
        return self._run_log().tb_dir

    def tb_scalars(self):
        return train_log.tb_scalars(self.logger, self.cfg)

    def _grad_guard(self, stats, log=print):
        return train_log.grad_guard(stats, self.cfg, self.i_so_far, self.updater._last_adv, self.writes_files, log)

    def write_episode_csv(self, max_rows=None):
        return self._run_log().write_episode_csv(self.ended_buf, self.done_buf, self.arrive_buf, self.eplen_buf, self.epret_buf,
                                                 self.eppath_buf, self.env_steps, self.logger.get("rollout_time", 0.0), max_rows)

    def write_tensorboard(self):
        self._run_log().write_tensorboard(self.i_so_far, self.logger, self.updater.loss_history, self.updater.stats, self.ended_buf,
                                          self.epret_buf, self.eplen_buf)

    # ---- checkpoints: the two reference-named files (checkpoint.py) and, beside them, one sidecar per option with state of its own
    sidecar_path = staticmethod(checkpoint.sidecar_path)

    retnorm_path = staticmethod(functools.partial(checkpoint.sidecar_path, "retnorm"))
    lrsched_path = staticmethod(functools.partial(checkpoint.sidecar_path, "lrsched"))

    def checkpoint_dir(self):
        return os.path.join(self.cfg.output_dir, self.cfg.method_name, "checkpoints")

    def _sidecars(self):
        """One row per sidecar, in the order load_checkpoint() reads them: (kind, the option is on, the payload to store, what takes
        the stored payload -- None: no such file --, the ONE warning line of a missing file with the path in its {}).  A row whose
        option is off is not touched: its two callables may read state that only the option creates."""
        cfg = self.cfg
        return (("lrsched", cfg.lr_schedule == "adaptive",   # the rate the next step starts from (on the host since the last read-back)
                 lambda: {"lr": float(self.updater.lr_value)}, lambda s: self.updater.set_lr(float(s["lr"] if s else cfg.lr)),
                 "lr_schedule='adaptive': {} not found -- the learning rate starts at lr = " + str(cfg.lr)),
                ("explore", cfg.learn_var,   # theta, its Adam moments and the steps taken
                 lambda: self.updater.var_state_dict(), lambda s: self.updater.load_var_state(s),
                 "learn_var: {} not found -- the exploration variance starts at init_var = " + str(cfg.init_var)),
                ("scenarios", self.scenarios is not None,   # the scores and the re-assignment counter (the next assignment is drawn from them)
                 lambda: dict(self.scenarios.state_dict(), score=[float(v) for v in self.scenarios.score]),
                 lambda s: self.scenarios.load_state_dict(s or {"score": [float("nan")] * self._scen_K, "counter": 0}),
                 "scenario_stats / scenario_priority: {} not found -- the scenario scores start fresh"),
                ("retnorm", cfg.norm_reward,   # the critic's units
                 lambda: dict(zip(("mean", "var", "count"), self.ret_rms[:3].tolist())),
                 lambda s: self._init_ret_rms(self.ret_rms.device, *((s["mean"], s["var"], s["count"]) if s else ())),
                 "norm_reward: {} not found -- the return statistics start fresh; the critic's units are off until they settle"))

    def save_checkpoint(self):
        pa, pc = checkpoint.save_nets(self.checkpoint_dir(), f"iter{self.i_so_far:04d}_step{self.t_so_far:08d}.pth", self.actor, self.critic)
        for kind, on, state, _, _ in self._sidecars():
            if on:
                checkpoint.save_sidecar(kind, pa, state())
        return pa, pc

    def load_checkpoint(self, actor_path, critic_path):
        """main.py:52-89: state_dicts only (optimiser state and covariance are not part of a checkpoint).  An option with a sidecar
        (_sidecars) takes its state from <kind>_<tag>.pth beside the actor's file; without that file: one warning line and the
        state of a fresh run (the learning rate: cfg.lr)."""
        self.reset_envs()   # (continue_rollouts: the episodes under way were the old weights')
        for kind, on, _, load, missing in self._sidecars():
            if on:
                load(checkpoint.load_sidecar(kind, actor_path, missing))
        checkpoint.load_nets(self.actor, self.critic, actor_path, critic_path)
