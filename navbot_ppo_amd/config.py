"""PPOConfig and the checks of its options.  A config is mutable, so every check runs at the construction of the config and again
where its option is put to use (the updater or the trainer); check_update_config runs at the updater only."""
import dataclasses
import math

MINIBATCH_SHUFFLES = ("epoch", "update", "none")
LR_SCHEDULES = (None, "adaptive", "linear")
SCENARIO_PRIORITIES = (None, "failure", "abs_adv")


@dataclasses.dataclass
class PPOConfig:
    rollout_len: int = 512                 # T: policy steps per env per iteration
    max_episode_steps: int = 500           # main.py / arguments.py:30 (timesteps_per_episode)
    gamma: float = 0.99                    # main.py:470
    n_updates_per_iteration: int = 50      # main.py:471
    lr: float = 3e-4                       # main.py:472 (lr_schedule: where the rate starts)
    clip: float = 0.2                      # main.py:473
    policy: str = "resmlp512"              # reference nets; "mlp64x2" = BASELINE config 2
    gae_lambda: float = None               # None = the reference's estimator A = rtgs - V (ppo.py:277); a number in [0, 1] turns
                                           # on GAE(lambda) (navsim_gae_scan): advantages and critic targets from the lambda-return
    # False = the reference: every episode end and the batch end are terminal (ppo.py:552-553,601,658-666).  True: partial-episode
    # bootstrapping (Pardo et al. 2018) by rsl_rl's rule -- a time-out (ended, neither done nor arrive) adds gamma V(s_t) of its own
    # row, the stand-in for the next state the in-kernel reset overwrote, and the envs still running on the last row bootstrap with
    # V(obs_buf[T]), for every lambda (gae_lambda = None runs as lambda = 1: A = R - V on truncation-aware returns).  Collisions and
    # arrivals stay terminal.  navsim_gae_scan_trunc on the device; per rank, no collective.
    bootstrap_truncated: bool = False
    init_var: float = 0.8                  # ppo.py:123
    var_decay: float = 0.995               # ppo.py:695
    var_floor: float = 0.1                 # ppo.py:694
    var_decay_after: int = 50000           # ppo.py:694
    # False = the reference: the variance follows the fixed schedule above and the update cannot change it.  True: theta = log var is a
    # parameter of the actor (the state-independent log-std of Stable-Baselines3 / rsl_rl / rl_games / CleanRL, one isotropic variance
    # as in the reference), stepped by Adam after every optimiser step of the nets -- at their rate, scaled by the actor's clip
    # coefficient -- on the gradient of actor_loss - ent_coef * entropy, clamped to [var_min, var_max]; it starts at init_var and the
    # schedule is off.  On one GPU the step is taken on the device (navppo_*_update_epoch_var; host mirror: learned_var_reference) and
    # every rollout reads the variance from the same device state.  Not with target_kl, overlap_allreduce or several ranks.
    learn_var: bool = False
    ent_coef: float = 0.0                  # learn_var: the entropy bonus' coefficient (0 = none)
    var_min: float = 1e-3                  # learn_var: the clamps of the variance
    var_max: float = 1.0
    save_freq: int = 2                     # ppo.py:774
    seed: int = 0
    use_graph: bool = True                 # capture the T-step rollout in one hipGraph
    persistent_rollout: bool = True        # on GPU: all T steps in ONE launch (navsim_rollout_mlp64 / navsim_rollout_resmlp512)
    fused_update: bool = True              # on GPU: fused HIP loss+gradient kernels (csrc/ppo_mlp64.hip, csrc/ppo_resmlp512.hip)
    # arithmetic of the fused update's matrix products: "bf16x3" = float32 products out of operands split into three bf16
    # pieces on the bf16 MFMA (six piece products, float32 accumulate: float32-equivalent by measurement), "f32" =
    # the f32-input MFMA (native float32 fma chains).  Inputs, outputs and everything around the products are float32 either way.
    # mlp64x2: both builds exist.  resmlp512: the fused kernels are "bf16x3" (split products where a k-step of the bf16 MFMA is
    # filled, f32-input MFMA elsewhere; V0 from navppo_resmlp512_value included); "f32" selects the PyTorch float32 path with a warning.
    update_arith: str = "bf16x3"
    # multi-GPU, mlp64x2: False = fused passes of both nets -> ONE all-reduce of the flat gradient -> Adam (the default: at one
    # RCCL rank this path costs 9-24 us per epoch over the single-GPU epoch, the per-net pipeline below 59-74 us, because two
    # pass launches pay the ramp / staging / reduction of the fused one twice -- more than a 43 KB all-reduce costs on the wire);
    # True = two-stage pipeline, each net's all-reduce under the other net's pass (_pipelined_epochs): hides the wire entirely
    overlap_allreduce: bool = False
    # None = the reference (its clip_grad_norm_(inf) calls only measure, ppo.py:352,389).  A number: in every epoch each net's
    # gradient is clipped to this L2 norm (torch's clip_grad_norm_) before its Adam step, and a net whose gradient is not finite
    # is not stepped at all (parameters and Adam moments untouched) -- on the device, inside the fused update (navppo_*_clipped)
    max_grad_norm: float = None
    # None = the reference: every update runs all its epochs.  A number > 0: an update stops -- both nets, Stable-Baselines3's
    # convention -- before the optimiser step of the first epoch whose approx_kl (the mean of (ratio - 1) - log ratio, ppo.py:326)
    # exceeds 1.5 x target_kl; on one GPU the decision is taken on the device and the remaining queued epochs return at the entry of
    # every kernel (navppo_*_update_epoch_kl).  Not with overlap_allreduce (the per-net pipeline has no place for the decision).
    target_kl: float = None
    # None, or a value >= the batch = the reference: every epoch is ONE optimiser step on the whole batch (ppo.py:237-240).  A positive
    # multiple of 32 (per rank): an epoch is K = ceil(n / minibatch_size) steps on slices of the batch, the last one shorter if n is no
    # multiple -- kept, not dropped; Adam's step counter, max_grad_norm and target_kl act per step.  Not with overlap_allreduce.
    minibatch_size: int = None
    # which samples a slice holds: "epoch" = a fresh permutation of the batch before every epoch (Stable-Baselines3, CleanRL), "update" =
    # one permutation per update, reused by its epochs, "none" = contiguous slices of the batch as it lies ([T, N]: time slices), no copy.
    # The permutations are batch_permutation(n, key(seed, rank), (update index, epoch index)): navppo_shuffle_batch on the device
    minibatch_shuffle: str = "epoch"
    # False = the reference: the critic regresses on raw returns (hundreds, at this simulator's rewards).  True: every rollout's rewards
    # are divided by the running standard deviation of the discounted return and clipped to +-clip_reward before the return scan
    # (Stable-Baselines3's VecNormalize(norm_reward=True); navppo_return_moments + navppo_reward_scale on the device, host mirror:
    # reward_norm_reference).  The critic then learns in scaled units; episode returns, metrics and CSVs stay raw.
    norm_reward: bool = False
    clip_reward: float = 10.0              # VecNormalize's clip_reward
    norm_reward_eps: float = 1e-8          # VecNormalize's epsilon: scale = 1 / sqrt(var + eps)
    # None = the reference: `lr` is one constant.  "adaptive" = the KL-adaptive step size of rsl_rl / rl_games: after every optimiser step
    # but the first of an update, lr /= 1.5 if that step's approx_kl > 2 desired_kl, lr *= 1.5 if 0 < approx_kl < desired_kl / 2, clamped
    # to [lr_min, lr_max]; it starts at `lr` and carries over from update to update.  On one GPU the decision is taken on the device, in
    # the step launch of navppo_*_update_epoch_lr (host mirror: adaptive_lr_reference).  Not with target_kl, not with overlap_allreduce.
    # "linear" = lr x max(0, 1 - t_so_far / total_timesteps), set at the start of every iteration of learn() (Stable-Baselines3's linear
    # schedule, CleanRL's anneal_lr): host only, the existing entry points take it as their lr argument.
    lr_schedule: str = None
    desired_kl: float = 0.01               # "adaptive": the KL the rule steers the per-step approx_kl towards
    lr_min: float = 1e-5                   # "adaptive": the clamps of the learning rate
    lr_max: float = 1e-2
    output_dir: str = ""                   # "" = no checkpoints / logs
    episode_csv_rows: int = 2000           # per-iteration cap on rows appended to <method>_train_episodes.csv (0 = off)
    tb_episode_rows: int = 256             # per-iteration cap on Episode_Rewards/train points in the TensorBoard file (0 = off)
    method_name: str = "baseline"
    # periodic evaluation while training: every eval_every iterations (0 = off) one persistent launch (VecEnv.evaluate_policy)
    # plays eval_episodes episodes with the DETERMINISTIC mean action at the evaluation arrival threshold 0.4 -- the success rate
    # the reference's users quote (main.py:135-252), not that of the noisy training rollouts -- on a second set of envs
    eval_every: int = 0
    eval_episodes: int = 100
    # None: the evaluation env is built from the training world (its movers included).  Anything else is resolved like VecEnv's
    # ``movers`` and given to the evaluation env only -- a held-out set of scenarios; with a bank of tapes the eval_* entries gain
    # eval_scenario_success_min / eval_scenario_success_mean
    eval_movers: object = None
    # False: the policy reads one 16-column row per step.  True (policy "mlp64x2", 10 beams, the persistent rollout and the fused
    # update, on the GPU): actor and critic are the 42-64-64 nets on SCAN-HISTORY rows -- the row, the scans of the two rows before
    # it and the action between them, never reaching across an episode's first row (env.stack_rows_reference).  The rollout assembles
    # the rows on chip (navsim_rollout_mlp64_hist); the update's batch comes from navsim_stack_rows, once per iteration.
    scan_history: bool = False
    # False = the reference: every rollout starts from a reset of all envs (ppo.py:486), so no training step ever sees an episode step
    # at or beyond rollout_len.  True: only the first rollout resets; every later one goes on where the last one stopped (the handle
    # holds the env state, row T of the observation buffer becomes row 0, with scan_history the history carry crosses the seam too:
    # navsim_rollout_mlp64_hist_cont / navsim_stack_rows_cont, with norm_reward the running return does) -- the regime of short
    # rollouts on many envs (rsl_rl, Stable-Baselines3 n_steps).  The envs are reset again when the world changes (set_map, set_movers,
    # the spawn sampler, ...), after load_checkpoint and on PPOTrainer.reset_envs().  Needs a batch end that is not terminal:
    # bootstrap_truncated=True or gae_lambda < 1.
    continue_rollouts: bool = False
    # Training on a bank of mover tapes (VecEnv movers="random:K", "bank:...", dict(bank=...); at least 2 tapes).  scenario_stats: one
    # navppo_group_sums launch per iteration sums the rollout per scenario on the device; its [K, 8] table rides on the iteration's one
    # all-reduce and one read-back, the log gains train_scenario_success_min / _mean and rank 0 appends <method>_train_scenarios.csv.
    # scenario_priority (implies the statistics): every scenario_resample_every iterations the envs are re-assigned to the scenarios by
    # rank-prioritised level replay (scenarios.ScenarioSampler) on a score per scenario -- "failure": 1 - success rate, "abs_adv": the
    # mean |advantage| (needs gae_lambda or bootstrap_truncated) -- an exponential average with weight scenario_score_alpha on the newest
    # iteration; weights (1 / rank)^(1 / scenario_temperature), mixed with the uniform distribution by scenario_uniform_mix.  A
    # re-assignment changes the world: with continue_rollouts the next rollout resets.  Both off: nothing differs.
    scenario_stats: bool = False
    scenario_priority: str = None
    scenario_resample_every: int = 1
    scenario_score_alpha: float = 0.5
    scenario_temperature: float = 0.3
    scenario_uniform_mix: float = 0.25

    def __post_init__(self):
        check_minibatch_config(self)
        check_reward_norm_config(self)
        check_lr_schedule_config(self)
        check_bootstrap_config(self)
        check_scan_history_config(self)
        check_continue_config(self)
        check_scenario_config(self)
        check_learn_var_config(self)


def check_learn_var_config(cfg, world=1):
    """PPOConfig.learn_var / ent_coef / var_min / var_max, at the construction of the config and again of the updater and the trainer
    (a config is mutable).  world: the number of ranks (the updater and the trainer know it)."""
    if not isinstance(cfg.learn_var, bool):
        raise ValueError(f"learn_var {cfg.learn_var!r}: True or False")
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)
    e, lo, hi = cfg.ent_coef, cfg.var_min, cfg.var_max
    if not num(e) or e < 0:
        raise ValueError(f"ent_coef {e!r}: a finite number >= 0")
    if not num(lo) or not lo > 0:
        raise ValueError(f"var_min {lo!r}: a finite number > 0")
    if not num(hi) or hi < lo:
        raise ValueError(f"var_max {hi!r}: a finite number >= var_min = {lo!r}")
    if not cfg.learn_var:
        if e != 0:
            raise ValueError(f"ent_coef {e!r} without learn_var: a fixed variance has no gradient for the entropy bonus to act on")
        return
    if not num(cfg.init_var) or not lo <= cfg.init_var <= hi:
        raise ValueError(f"init_var {cfg.init_var!r} outside [var_min, var_max] = [{lo!r}, {hi!r}]")
    if cfg.target_kl is not None:
        raise ValueError("learn_var with target_kl: the gated kernels are not combined with the learned variance's")
    if cfg.overlap_allreduce:
        raise ValueError("learn_var with overlap_allreduce=True: the per-net pipeline has no place for the variance's step")
    if world > 1:
        raise ValueError(f"learn_var on {world} ranks: the multi-GPU form is not built (one rank only)")


def check_scenario_config(cfg):
    """PPOConfig.scenario_stats / scenario_priority and their parameters, at the construction of the config and again of the trainer
    (a config is mutable).  What needs the env -- a bank of at least 2 tapes -- is checked by the trainer."""
    if not isinstance(cfg.scenario_stats, bool):
        raise ValueError(f"scenario_stats {cfg.scenario_stats!r}: True or False")
    if cfg.scenario_priority not in SCENARIO_PRIORITIES:
        raise ValueError(f"scenario_priority {cfg.scenario_priority!r}: one of {SCENARIO_PRIORITIES}")
    every = cfg.scenario_resample_every
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError(f"scenario_resample_every {every!r}: an integer >= 1")
    for name in ("scenario_score_alpha", "scenario_uniform_mix"):
        v = getattr(cfg, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:   # (NaN fails the comparison too)
            raise ValueError(f"{name} {v!r}: a number in [0, 1]")
    b = cfg.scenario_temperature
    if isinstance(b, bool) or not isinstance(b, (int, float)) or not (0.0 < b < float("inf")):
        raise ValueError(f"scenario_temperature {b!r}: a finite number > 0")
    if cfg.scenario_priority == "abs_adv" and cfg.gae_lambda is None and not cfg.bootstrap_truncated:
        raise ValueError("scenario_priority='abs_adv' needs the raw advantages in the trainer: set gae_lambda or bootstrap_truncated "
                         "(the reference's A = rtg - V is formed inside the update)")


def check_continue_config(cfg):
    """PPOConfig.continue_rollouts, at the construction of the config and again of the trainer (a config is mutable)."""
    if not isinstance(cfg.continue_rollouts, bool):
        raise ValueError(f"continue_rollouts {cfg.continue_rollouts!r}: True or False")
    if not cfg.continue_rollouts:
        return
    lam = cfg.gae_lambda
    if not (cfg.bootstrap_truncated is True or (lam is not None and float(lam) < 1.0)):
        raise ValueError("continue_rollouts=True needs bootstrap_truncated=True or gae_lambda < 1: the reference's convention treats "
                         "the batch end as terminal, which would cut every env's running episode in every iteration")


def check_scan_history_config(cfg):
    """PPOConfig.scan_history, at the construction of the config and again of the trainer (a config is mutable)."""
    if not isinstance(cfg.scan_history, bool):
        raise ValueError(f"scan_history {cfg.scan_history!r}: True or False")
    if cfg.scan_history and cfg.policy == "resmlp512":
        raise ValueError("scan_history with policy='resmlp512': its kernels read 16-column rows only; use policy='mlp64x2'")
    if cfg.scan_history and not (cfg.persistent_rollout and cfg.fused_update):
        raise ValueError("scan_history needs persistent_rollout=True and fused_update=True: only the persistent rollout kernel "
                         "keeps the scan history on chip, and only the fused update has the 42-column entry points")


def check_bootstrap_config(cfg):
    """PPOConfig.bootstrap_truncated, at the construction of the config and again of the trainer (a config is mutable)."""
    if not isinstance(cfg.bootstrap_truncated, bool):
        raise ValueError(f"bootstrap_truncated {cfg.bootstrap_truncated!r}: True or False")


def check_minibatch_config(cfg):
    """PPOConfig.minibatch_size / minibatch_shuffle, at the construction of the config and again of the updater (a config is mutable)."""
    mb = cfg.minibatch_size
    if mb is not None:
        if isinstance(mb, bool) or not isinstance(mb, int) or mb < 32 or mb % 32:
            raise ValueError(f"minibatch_size {mb!r}: None (full-batch epochs) or a positive multiple of 32")
        if cfg.overlap_allreduce:
            raise ValueError("minibatch_size with overlap_allreduce=True: the per-net pipeline runs whole-batch epochs only")
    if cfg.minibatch_shuffle not in MINIBATCH_SHUFFLES:
        raise ValueError(f"minibatch_shuffle {cfg.minibatch_shuffle!r}: one of {MINIBATCH_SHUFFLES}")


def check_reward_norm_config(cfg):
    """PPOConfig.norm_reward / clip_reward / norm_reward_eps, at the construction of the config and again of the trainer."""
    c, e = cfg.clip_reward, cfg.norm_reward_eps
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not c > 0:
        raise ValueError(f"clip_reward {c!r}: a number > 0")
    if isinstance(e, bool) or not isinstance(e, (int, float)) or not (0 <= e < math.inf):
        raise ValueError(f"norm_reward_eps {e!r}: a finite number >= 0")


def check_lr_schedule_config(cfg):
    """PPOConfig.lr_schedule and its parameters, at the construction of the config and again of the updater (a config is mutable)."""
    if cfg.lr_schedule not in LR_SCHEDULES:
        raise ValueError(f"lr_schedule {cfg.lr_schedule!r}: one of {LR_SCHEDULES}")
    if cfg.lr_schedule != "adaptive":
        return
    if cfg.target_kl is not None:
        raise ValueError("lr_schedule='adaptive' with target_kl: two answers to the same signal; choose one")
    if cfg.overlap_allreduce:
        raise ValueError("lr_schedule='adaptive' with overlap_allreduce=True: the per-net pipeline has no place for the decision")
    for name in ("desired_kl", "lr_min", "lr_max"):
        if not float(getattr(cfg, name)) > 0.0:   # (NaN fails the comparison too)
            raise ValueError(f"{name} {getattr(cfg, name)!r}: a number > 0")
    if not float(cfg.lr_max) >= float(cfg.lr_min):
        raise ValueError(f"lr_max {cfg.lr_max!r} < lr_min {cfg.lr_min!r}")
    if not float(cfg.lr_min) <= float(cfg.lr) <= float(cfg.lr_max):
        raise ValueError(f"lr {cfg.lr!r} outside [lr_min, lr_max] = [{cfg.lr_min!r}, {cfg.lr_max!r}]")


def check_update_config(cfg):
    """PPOConfig.update_arith / max_grad_norm / target_kl, at the construction of the updater (not of the config)."""
    if cfg.update_arith not in ("f32", "bf16x3"):
        raise ValueError(f"update_arith {cfg.update_arith!r}: 'f32' or 'bf16x3'")
    if cfg.max_grad_norm is not None and not float(cfg.max_grad_norm) > 0.0:   # (NaN fails the comparison too)
        raise ValueError(f"max_grad_norm {cfg.max_grad_norm!r}: None (off) or a number > 0")
    if cfg.target_kl is not None and not float(cfg.target_kl) > 0.0:   # (NaN fails the comparison too)
        raise ValueError(f"target_kl {cfg.target_kl!r}: None (off) or a number > 0")
    if cfg.target_kl is not None and cfg.overlap_allreduce:
        raise ValueError("target_kl with overlap_allreduce=True: the per-net pipeline has no place for the stop decision")
