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
                                    check of ppo.py:356-379,414-416 is PPOTrainer._grad_guard)
                                    PPOConfig.minibatch_size: K optimiser steps per epoch on slices of the batch, shuffled
                                    on the device (navppo_shuffle_batch; host mirror: batch_permutation)
                                    PPOConfig.lr_schedule: "adaptive" = the learning rate follows every step's approx_kl, decided
                                    on the device (navppo_*_update_epoch_lr; host mirror: adaptive_lr_reference); "linear" = decay
                                    over learn()'s budget, set per iteration
  learn            ppo.py:218-461   iteration loop, timing, checkpoints (actor_iter%04d_step%08d.pth)

Multi-GPU (absent in the reference): one process per GPU, each owns a contiguous shard
of env ids; after each backward ONE all-reduce (RCCL over xGMI; gloo on CPU for tests) of the single
flat gradient buffer holding actor+critic; the advantage mean/std come from all-reduced
(sum, sum of squares, count) so they equal the single-process values of ppo.py:284.
"""
import ctypes as C
import dataclasses
import math
import os
import time

import torch
import torch.distributed as dist

from . import nets
from ._native import check, lib

LOG_2PI = math.log(2.0 * math.pi)
ADAM_HYPER = (0.9, 0.999, 1e-8)   # Adam's (beta1, beta2, eps), torch's defaults (ppo.py:116-117): torch.optim.Adam and the fused steps


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if offset else C.c_void_p(t.data_ptr())


def _navppo(entry, *args):
    """Calls the navppo_* entry point `entry` (include/navppo.h) with `args` and the current stream; a failure raises under the name
    of the entry point that was called, with its message."""
    L = lib()
    if getattr(L, entry)(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
        raise RuntimeError(f"{entry} failed: {L.navppo_last_error().decode()}")


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

    def __post_init__(self):
        check_minibatch_config(self)
        check_reward_norm_config(self)
        check_lr_schedule_config(self)
        check_bootstrap_config(self)


def check_bootstrap_config(cfg):
    """PPOConfig.bootstrap_truncated, at the construction of the config and again of the trainer (a config is mutable)."""
    if not isinstance(cfg.bootstrap_truncated, bool):
        raise ValueError(f"bootstrap_truncated {cfg.bootstrap_truncated!r}: True or False")


# --------------------------------------------------------------------------- minibatch updates
MINIBATCH_SHUFFLES = ("epoch", "update", "none")


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


_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _philox4x32_10(ctr, key):
    """Philox4x32-10 of the kernels (csrc/mlp64_policy.h: philox10) on Python integers."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def batch_permutation(n, key, counter):
    """The permutation pi of navppo_shuffle_batch (include/navppo.h states it) as an int64 tensor on the CPU: out[i] = in[pi[i]].
    A pure function of (n, key, counter): a 6-round Feistel network on ceil(log2 n) bits whose halves trade places and widths every
    round, cycle-walked into [0, n); the round function is two of Philox's multiply-mix rounds, the round keys a Weyl sequence from
    Philox4x32-10 over (counter, n) keyed by `key`.  The kernel matches it exactly (tests/test_gpu_minibatch.py)."""
    import numpy as np
    n, key, counter = int(n), int(key) & _M64, int(counter) & _M64
    if not 1 <= n < 1 << 31:
        raise ValueError(f"batch_permutation: n = {n} outside [1, 2^31)")
    b = (n - 1).bit_length()
    a = b // 2
    c = b - a
    o = _philox4x32_10((counter & _M32, counter >> 32, n, 0x73687566), (key & _M32, key >> 32))
    u64 = np.uint64
    m32, s32 = u64(_M32), u64(32)

    def network(x):
        wl, wr, k0, k1 = a, c, o[0], o[1]
        for _ in range(6):
            left, r = x >> u64(wr), x & u64((1 << wr) - 1)
            p = u64(_PHILOX_M0) * ((r + u64(k0)) & m32)
            t = (p >> s32) ^ (p & m32) ^ u64(k1)
            q = u64(_PHILOX_M1) * t
            f = (q >> s32) ^ (q & m32)
            x = (r << u64(wl)) | (left ^ (f & u64((1 << wl) - 1)))
            wl, wr = wr, wl
            k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
        return x

    x = network(np.arange(n, dtype=u64))
    while True:   # cycle walking: the network is a bijection of [0, 2^b), so every walk from an index < n comes back below n
        walk = np.nonzero(x >= u64(n))[0]
        if walk.size == 0:
            break
        x[walk] = network(x[walk])
    return torch.from_numpy(x.astype(np.int64))


def minibatch_key(seed, rank=0):
    """`key` of an updater's permutations: PPOConfig.seed mixed with the global rank (every rank shuffles its own shard its own way)."""
    return (int(seed) * 0x9E3779B97F4A7C15 + 0x6D6273 + int(rank) * 0xD1B54A32D192ED03) & _M64


def minibatch_counter(update_index, epoch_index):
    """`counter` of a permutation: (update index, epoch index) -- no two epochs of a run share one."""
    return ((int(update_index) & _M32) << 32) | (int(epoch_index) & _M32)


# --------------------------------------------------------------------------- reward normalisation
RET_RMS_INIT = (0.0, 1.0, 1e-4)   # (mean, var, count) of a fresh run: Stable-Baselines3's RunningMeanStd(epsilon=1e-4)


def check_reward_norm_config(cfg):
    """PPOConfig.norm_reward / clip_reward / norm_reward_eps, at the construction of the config and again of the trainer."""
    c, e = cfg.clip_reward, cfg.norm_reward_eps
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not c > 0:
        raise ValueError(f"clip_reward {c!r}: a number > 0")
    if isinstance(e, bool) or not isinstance(e, (int, float)) or not (0 <= e < math.inf):
        raise ValueError(f"norm_reward_eps {e!r}: a finite number >= 0")


def _chk_rewards(what, rew, ended=None):
    from ._native import NavsimError
    if not rew.is_cuda:
        raise NavsimError(f"{what} needs device tensors; there is no CPU path")
    assert rew.dtype == torch.float32 and rew.is_contiguous(), f"{what}: rewards are contiguous float32"
    if ended is not None:
        assert rew.dim() == 2 and ended.dtype == torch.uint8 and ended.shape == rew.shape and ended.is_contiguous() and ended.device == rew.device


def _chk_f64(what, t, shape, device):
    assert t.dtype == torch.float64 and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == device, \
        f"{what}: a contiguous float64 tensor of shape {tuple(shape)} on {device}"


def return_moments(rew, ended, gamma, carry=None, out=None):
    """(n, mean, M2) of the T N forward discounted returns of a [T, N] rollout, as a float64 [3] device tensor (navppo_return_moments;
    `out`: where to write it).  carry: float64 [N], the running return in front of row 0 on entry and behind row T - 1 on return
    (None: every column starts at 0).  Asynchronous on the current stream; calls on one device must not overlap in time."""
    _chk_rewards("return_moments", rew, ended)
    T, N = rew.shape
    if out is None:
        out = torch.empty(3, dtype=torch.float64, device=rew.device)
    _chk_f64("return_moments: out", out, (3,), rew.device)
    if carry is not None:
        _chk_f64("return_moments: carry", carry, (N,), rew.device)
    with torch.cuda.device(rew.device):
        _navppo("navppo_return_moments", _ptr(rew), _ptr(ended), T, N, float(gamma), None if carry is None else _ptr(carry), _ptr(out))
    return out


def reward_scale(rms, moments, rew, clip=10.0, eps=1e-8, out=None):
    """Merges the rows of `moments` ([K, 3] or [3] float64, None = no row: frozen statistics) into rms = (mean, var, count, scale)
    (float64 [4], updated in place) and returns clamp(float32(rew * scale), -clip, clip) with scale = 1 / sqrt(var + eps)
    (navppo_reward_scale).  out: where to write the scaled rewards (may be `rew`).  Asynchronous on the current stream."""
    _chk_rewards("reward_scale", rew)
    _chk_f64("reward_scale: rms", rms, (4,), rew.device)
    K = 0
    if moments is not None:
        K = 1 if moments.dim() == 1 else int(moments.shape[0])
        _chk_f64("reward_scale: moments", moments, (3,) if moments.dim() == 1 else (K, 3), rew.device)
    if out is None:
        out = torch.empty_like(rew)
    assert out.dtype == torch.float32 and out.shape == rew.shape and out.is_contiguous() and out.device == rew.device
    with torch.cuda.device(rew.device):
        _navppo("navppo_reward_scale", _ptr(rms), None if K == 0 else _ptr(moments), K, _ptr(rew), _ptr(out), rew.numel(), float(eps),
                float(clip))
    return out


def merge_return_moments(rms, rows):
    """The merge rule of navppo_reward_scale on the host, float64: rms = (mean, var, count[, ...]), rows [K, 3] = (n, mean, M2) per
    batch, merged in order with the formula of RunningMeanStd.update_from_moments; a row with n <= 0 or a non-finite entry is skipped.
    Returns (mean, var, count) as a numpy array."""
    import numpy as np
    mean, var, count = (np.float64(v) for v in list(rms)[:3])
    for bn, bm, bm2 in np.asarray(rows, dtype=np.float64).reshape(-1, 3):
        if not (bn > 0 and np.isfinite(bn) and np.isfinite(bm) and np.isfinite(bm2)):
            continue
        d, tot = bm - mean, count + bn
        mean = mean + d * bn / tot
        var = (var * count + bm2 + d * d * count * bn / tot) / tot
        count = tot
    return np.array([mean, var, count], dtype=np.float64)


def reward_norm_reference(rew, ended, gamma, rms=RET_RMS_INIT, carry=None, clip=10.0, eps=1e-8):
    """Host mirror of navppo_return_moments followed by navppo_reward_scale(K = 1), numpy float64 -- the statement of the rule.
    rew [T, N] float32, ended [T, N] (non-zero = an episode ended on that row), rms = (mean, var, count) before the rollout,
    carry [N] float64 or None.  Returns a namespace: moments (n, mean, M2) of the T N running returns, carry [N] behind the last row,
    rms (mean, var, count, scale) after the merge, out [T, N] float32 = clip(float32(rew * scale), -clip, clip)."""
    import types
    import numpy as np
    rew = np.ascontiguousarray(np.asarray(rew, dtype=np.float32))
    done = np.asarray(ended) != 0
    T, N = rew.shape
    R = np.zeros(N, dtype=np.float64) if carry is None else np.array(carry, dtype=np.float64)
    g = np.float64(gamma)
    rets = np.empty((T, N), dtype=np.float64)
    for t in range(T):
        R = g * R + rew[t].astype(np.float64)
        rets[t] = R
        R = np.where(done[t], 0.0, R)
    mean = rets.mean()
    moments = np.array([float(T * N), mean, ((rets - mean) ** 2).sum()], dtype=np.float64)
    m = merge_return_moments(rms, moments)
    scale = np.float64(1.0) / np.sqrt(m[1] + np.float64(eps))
    out = np.clip((rew.astype(np.float64) * scale).astype(np.float32), np.float32(-clip), np.float32(clip))
    return types.SimpleNamespace(moments=moments, carry=R, rms=np.append(m, scale), out=out)


# --------------------------------------------------------------------------- learning-rate schedules
LR_SCHEDULES = (None, "adaptive", "linear")
LR_FACTOR = 1.5   # the rule's step (rsl_rl, rl_games); not configurable


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


def adaptive_lr_direction(kl, desired_kl, adapt=True):
    """The branch of the rule an optimiser step with approx_kl `kl` takes: -1 = lower, +1 = raise, 0 = keep.  float32 comparisons, the
    expressions of clip_adam_lr_kernel (include/navppo.h, "Adaptive learning rate"): a NaN or +inf kl lowers; kl <= 0 keeps."""
    import numpy as np
    f = np.float32
    if not adapt:
        return 0
    with np.errstate(all="ignore"):
        kl, tgt = f(kl), f(desired_kl)
        if not (kl <= f(2.0) * tgt):
            return -1
        if kl < f(0.5) * tgt and kl > f(0.0):
            return 1
    return 0


def adaptive_lr_reference(lr, kl, desired_kl, lr_min, lr_max, adapt=True):
    """Host mirror of the learning rate clip_adam_lr_kernel steps with: float32 arithmetic, bit for bit.  lr: the rate before the step;
    returns the rate of this step (a Python float holding the float32 value)."""
    import numpy as np
    f = np.float32
    lr = f(lr)
    d = adaptive_lr_direction(kl, desired_kl, adapt)
    with np.errstate(all="ignore"):
        if d < 0:
            lr = max(f(lr_min), lr / f(LR_FACTOR))
        elif d > 0:
            lr = min(f(lr_max), lr * f(LR_FACTOR))
    return float(lr)


def linear_lr(lr, t_so_far, total_timesteps):
    """lr_schedule="linear": the rate of an iteration that starts after t_so_far of total_timesteps"""
    return float(lr) * max(0.0, 1.0 - float(t_so_far) / float(total_timesteps))


# --------------------------------------------------------------------------- distributed context
class DistCtx:
    """torch.distributed wrapper that degrades to a no-op for a single process."""

    def __init__(self, device=None):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        # NAVBOT_DIST_FORCE=1: a single rank still creates its process group and sends every collective through the backend --
        # on a one-GPU box this is how the RCCL branch (init with device_id, all-reduces on RCCL's stream, the overlap of the
        # actor's all-reduce with the critic pass, navppo_adam_step's 1/world scale) is executed at all
        self.enabled = self.world > 1 or os.environ.get("NAVBOT_DIST_FORCE") == "1"
        if device is None:
            if torch.cuda.is_available():
                device = torch.device(f"cuda:{self.local_rank % torch.cuda.device_count()}")
            else:
                device = torch.device("cpu")
        self.device = torch.device(device)
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        self.backend, self.rccl_version = None, None
        if self.enabled and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29500")
            # "nccl" is RCCL on ROCm.  NAVBOT_DIST_BACKEND=gloo lets several ranks share one GPU (tests only:
            # RCCL refuses two ranks on the same device).
            backend = os.environ.get("NAVBOT_DIST_BACKEND") or ("nccl" if self.device.type == "cuda" else "gloo")
            kw = {"device_id": self.device} if backend == "nccl" else {}
            dist.init_process_group(backend=backend, rank=self.rank, world_size=self.world, **kw)
        if self.enabled:
            # a launcher may have created the group itself (backend=None or "cpu:gloo,cuda:nccl"): ask for the CUDA backend
            try:
                self.backend = dist.get_backend_config().get_device_backend_map().get("cuda", dist.get_backend())
            except Exception:
                self.backend = dist.get_backend()
            if self.device.type == "cuda" and not os.environ.get("NAVBOT_DIST_BACKEND") and "nccl" not in str(self.backend):
                import warnings
                warnings.warn(f"GPU ranks should talk RCCL (torch backend 'nccl'); the process group uses {self.backend!r}")
            if "nccl" in str(self.backend):
                self.backend = "nccl"
                try:
                    self.rccl_version = ".".join(str(v) for v in torch.cuda.nccl.version())
                except Exception:
                    self.rccl_version = "unknown"
                if self.rank == 0:   # one line per job: a scaling run shows how many ranks RCCL really connected
                    print(f"[navbot_ppo_amd] RCCL {self.rccl_version}: {dist.get_world_size()} ranks, one per GPU, "
                          f"flat-gradient all-reduce per epoch", flush=True)

    def all_reduce_sum(self, t):
        if self.enabled:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t

    def all_reduce_max(self, t):
        if self.enabled:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t

    def broadcast(self, t, src=0):
        if self.enabled:
            dist.broadcast(t, src=src)
        return t

    def barrier(self):
        if self.enabled:
            dist.barrier()

    def shard(self, n_total):
        """Contiguous env-id shard [lo, hi) of this rank."""
        per = n_total // self.world
        if per * self.world != n_total:
            raise ValueError(f"n_envs {n_total} not divisible by world size {self.world}")
        return self.rank * per, (self.rank + 1) * per


# --------------------------------------------------------------------------- flat parameters
class FlatParams:
    """All trainable tensors of actor + critic as views into ONE flat buffer, and their gradients as
    views into ONE flat gradient buffer: a single all-reduce and a single Adam update per epoch.
    (The reference's unused BatchNorm parameters never receive gradients -- net_actor.py:44,48 -- and
    stay ordinary tensors so state_dict keys are unchanged.)"""

    def __init__(self, modules, device):
        per_module = [[p for n, p in m.named_parameters() if ".bn" not in "." + n and not n.startswith("bn")] for m in modules]
        self.params = [p for ps in per_module for p in ps]
        self.module_numel = [sum(p.numel() for p in ps) for ps in per_module]   # [actor, critic] slices of the flat buffers
        total = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.grad = torch.zeros(total, dtype=torch.float32, device=device)
        off = 0
        for p in self.params:
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view_as(p)
            p.grad = self.grad[off:off + n].view_as(p)
            off += n
        self.numel = total
        self.proxy = torch.nn.Parameter(self.flat, requires_grad=True)
        self.proxy.data = self.flat
        self.proxy.grad = self.grad


def gaussian_log_prob(mean, action, var):
    """log N(action; mean, var*I) for a 2-D isotropic Gaussian = MultivariateNormal(mean, diag(var)).log_prob
    (ppo.py:696,704,734-735)."""
    k = mean.shape[-1]
    return -0.5 * (((action - mean) ** 2).sum(-1) / var) - 0.5 * k * LOG_2PI - 0.5 * k * torch.log(var)


def ppo_losses(actor, critic, obs, acts, logp_old, rtg, adv, var, clip):
    """One evaluation of ppo.py:307-343.  Returns (actor_loss, critic_loss, ratios, logp)."""
    V = critic(obs).squeeze(-1)
    mean = actor(obs)
    lo = mean.new_tensor([0.0, -1.0])
    hi = mean.new_tensor([1.0, 1.0])
    mean = torch.max(torch.min(mean, hi), lo)              # ppo.py:730-733 (no-op after sigmoid/tanh)
    logp = gaussian_log_prob(mean, acts, var)
    ratios = torch.exp(logp - logp_old)                    # ppo.py:316
    surr1 = ratios * adv                                   # ppo.py:319
    surr2 = torch.clamp(ratios, 1 - clip, 1 + clip) * adv  # ppo.py:320
    actor_loss = (-torch.min(surr1, surr2)).mean()         # ppo.py:342
    critic_loss = torch.nn.functional.mse_loss(V, rtg)     # ppo.py:343
    return actor_loss, critic_loss, ratios, logp, V


def normalise_advantages(adv, ctx=None):
    """(A - mean) / (std + 1e-10) with torch.std's unbiased estimator (ppo.py:284); with several ranks the
    moments are all-reduced so every rank uses the global mean/std."""
    a64 = adv.double()
    m = torch.stack([a64.sum(), (a64 * a64).sum(), torch.tensor(float(adv.numel()), dtype=torch.float64, device=adv.device)])
    if ctx is not None:
        ctx.all_reduce_sum(m)
    n = m[2]
    mean = m[0] / n
    var = (m[1] - n * mean * mean) / (n - 1)
    std = torch.sqrt(torch.clamp(var, min=0.0))
    return ((adv - mean.float()) / (std.float() + 1e-10))


# What each of PPOUpdater's four epoch runners hands to _summarise.  k: the epochs whose passes ran = the rows the statistics are taken
# over; steps, stopped: optimiser steps taken, whether target_kl stopped the update early (k = steps + stopped); losses: [n_ep, 2] per-epoch
# (actor, critic) loss, NaN behind a stop; sums: [4] sums over the k epochs of (actor loss, critic loss, approx_kl, clip_frac); gn_sum, v_sum:
# the same of the whole gradient's norm and the mean value; net_gn: [2] of the per-net norms, if the runner has them; net_gn_open: less the last's.
# Minibatches (K = slices per epoch > 1): k, steps and the sums count optimiser STEPS (K to an epoch); losses stays per epoch -- a row is
# the mean over the steps of its epoch that ran, NaN where none did
_Epochs = dataclasses.make_dataclass("_Epochs", ["k", "steps", "stopped", "losses", "sums", "gn_sum", "v_sum",
                                                 ("net_gn", object, None), ("net_gn_open", bool, False), ("K", int, 1)])


class PPOUpdater:
    """The update half of PPO.learn (ppo.py:275-397) on a fixed batch: the host side of the fused HIP update and its PyTorch formulation."""

    def __init__(self, actor, critic, cfg, ctx=None, device=None):
        self.actor, self.critic, self.cfg, self.ctx = actor, critic, cfg, ctx
        self.device = device or next(actor.parameters()).device
        self.fp = FlatParams([actor, critic], self.device)
        if ctx is not None:
            ctx.broadcast(self.fp.flat, 0)  # identical replicas; identical Adam steps keep them in sync
        fused = self.device.type == "cuda"
        self.opt = torch.optim.Adam([self.fp.proxy], lr=cfg.lr, betas=ADAM_HYPER[:2], eps=ADAM_HYPER[2], fused=fused)  # == ppo.py:116-117
        self.stats = {}
        # HIP paths: fused f32-MFMA kernels instead of ~40 (mlp64x2) / ~120 (resmlp512) PyTorch kernels per epoch
        on_gpu = self.device.type == "cuda" and cfg.fused_update
        # the D-64-64 heads: D = 16 (10 beams) or 42 (36 beams), rows float32 or float16 (obs_f16 envs) -- include/navppo.h
        self.fused_mlp64 = (on_gpu and cfg.policy == "mlp64x2" and isinstance(actor, nets.MLP64Actor)
                            and actor.layer1.in_features in (16, 42))
        self.obs_dim = actor.layer1.in_features if isinstance(actor, nets.MLP64Actor) else actor.rb1.f_in
        if cfg.update_arith not in ("f32", "bf16x3"):
            raise ValueError(f"update_arith {cfg.update_arith!r}: 'f32' or 'bf16x3'")
        if cfg.max_grad_norm is not None and not float(cfg.max_grad_norm) > 0.0:   # (NaN fails the comparison too)
            raise ValueError(f"max_grad_norm {cfg.max_grad_norm!r}: None (off) or a number > 0")
        self.max_norm = None if cfg.max_grad_norm is None else float(cfg.max_grad_norm)
        if cfg.target_kl is not None and not float(cfg.target_kl) > 0.0:   # (NaN fails the comparison too)
            raise ValueError(f"target_kl {cfg.target_kl!r}: None (off) or a number > 0")
        if cfg.target_kl is not None and cfg.overlap_allreduce:
            raise ValueError("target_kl with overlap_allreduce=True: the per-net pipeline has no place for the stop decision")
        self.kl_limit = None if cfg.target_kl is None else 1.5 * float(cfg.target_kl)   # Stable-Baselines3's factor
        check_minibatch_config(cfg)
        check_lr_schedule_config(cfg)
        # lr_schedule: lr_adaptive = the rule runs after every optimiser step; lr_value = the rate the next step starts from (adaptive),
        # or the rate set_lr() put in force ("linear": the trainer, per iteration); None = cfg.lr as it stands at every call
        self.lr_adaptive = cfg.lr_schedule == "adaptive"
        self.lr_value = float(cfg.lr) if self.lr_adaptive else None
        self.lr_state = None     # adaptive, fused: [4] (two rate slots, raises, lowerings) on the device, zeroed here: the first step starts at cfg.lr
        self.lr_counts = (0, 0)  # adaptive: raises and lowerings since construction
        self.kl_steps = None     # adaptive: [steps] the approx_kl (global, on several ranks) of every optimiser step of the last update()
        self._lr_step = 0        # adaptive: optimiser steps queued in the update in flight (the first one does not adapt)
        self.update_index = 0    # updates run so far: the high word of the shuffle's counter
        self._mb_key = minibatch_key(cfg.seed, ctx.rank if ctx is not None else 0)
        self._mb = None          # the minibatch plan of the update in flight (_plan_minibatches); None = whole-batch epochs
        self._shuf = self._shuf_key = None   # the ONE permuted copy of the batch (navppo_shuffle_batch's outputs), regrown like _prep
        # the clipped machinery runs and fills clip_stats: max_grad_norm, or target_kl alone -- at max_norm = +inf: the unclipped epochs' bits
        # (adaptive lr: the step launch is the clipped one's)
        self._clipping = self.max_norm is not None or self.kl_limit is not None or self.lr_adaptive
        self.kl_state = None     # target_kl on, fused: [4] (stopped, steps taken, tripping approx_kl, its step) of the last update(), on the device
        self.clip_stats = None   # clipping on: [n_ep, 4] (s_actor, s_critic, coef_actor, coef_critic) of the last update(), on the device
        self.fused_resmlp512 = (on_gpu and cfg.policy == "resmlp512" and isinstance(actor, nets.ResMLPActor)
                                and actor.rb1.f_in == 16 and actor.rb1.fc1.out_features == 512)
        if self.fused_resmlp512 and cfg.update_arith == "f32":
            # the fused 512-wide kernels exist in ONE arithmetic (csrc/ppo_resmlp512.hip: the products that fill a k-step of the
            # bf16 MFMA are split-bf16 float32 products, the rest f32-input MFMA).  A caller who asks for native float32
            # products gets them -- from PyTorch's float32 GEMMs, ~4 x slower per epoch -- instead of being ignored.
            import warnings
            warnings.warn("update_arith='f32' with policy='resmlp512': the fused 512-wide kernels have no all-f32-MFMA build; "
                          "this updater runs the PyTorch float32 path (slower).  Use update_arith='bf16x3' (default) for the fused kernels.")
            self.fused_resmlp512 = False
        self.fused = "navppo_mlp64" if self.fused_mlp64 else "navppo_resmlp512" if self.fused_resmlp512 else None
        self.bf16x3 = self.fused_mlp64 and cfg.update_arith == "bf16x3"   # (16- and 42-column rows, float32 or float16)
        self._prep = self._prep_key = None
        self._n_actor = self.fp.module_numel[0]   # the actor's slice of the flat buffers is [0, _n_actor), the critic's the rest
        if self.fused:
            d = self.obs_dim
            assert tuple(self.fp.module_numel) == ((64 * d + 4354, 64 * d + 4289) if self.fused_mlp64 else (50290, 50257))
            self._ws = None
            if self.fused_mlp64:
                self._ws = torch.empty(lib().navppo_mlp64_workspace_bytes(d) // 4, dtype=torch.float32, device=self.device)
            self._fstats = torch.zeros(8, dtype=torch.float32, device=self.device)
            self._fhist = torch.zeros((max(cfg.n_updates_per_iteration, 1), 8), dtype=torch.float32, device=self.device)
            # single GPU: Adam runs inside the kernel that sums the partial gradients (navppo_*_update_epoch)
            self._adam_m = torch.zeros_like(self.fp.flat)
            self._adam_v = torch.zeros_like(self.fp.flat)
            self._adam_t = 0
            if self.lr_adaptive:
                self.lr_state = torch.zeros(4, dtype=torch.float32, device=self.device)

    def _lr(self):
        """the `lr` argument of the fused entry points (adaptive: where a zeroed state starts)"""
        return float(self.cfg.lr if self.lr_value is None or self.lr_adaptive else self.lr_value)

    def set_lr(self, lr):
        """Puts a learning rate in force: lr_schedule="linear" (the trainer, per iteration), and the resumed rate of "adaptive" -- into
        BOTH slots of the device state, whichever the next step reads."""
        self.lr_value = float(lr)
        self.opt.param_groups[0]["lr"] = self.lr_value
        if self.lr_state is not None:
            self.lr_state[:2] = self.lr_value

    def _lr_args(self):
        """kl_target, lr_min, lr_max, adapt, lr_state_dev of the *_lr entry points; counts the step: the first of an update does not adapt"""
        cfg, adapt = self.cfg, int(self._lr_step > 0)
        self._lr_step += 1
        return (float(cfg.desired_kl), float(cfg.lr_min), float(cfg.lr_max), adapt, _ptr(self.lr_state))

    def _workspace(self, n):
        """Scratch of the fused kernels: fixed for the 2x64 heads, per-sample partial block outputs for the 512-wide nets."""
        if self.fused_resmlp512:
            need = lib().navppo_resmlp512_workspace_bytes(int(n)) // 4 + 4
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._ws

    def _obs_args(self, obs):
        """The observation arguments of the fused entry points -- (pointer, obs_dim, obs_f16) for the D-64-64 heads, (pointer, obs_f16)
        for the 512-wide nets -- after checking what is behind the pointer: rows of self.obs_dim columns, float32 or float16 (the
        kernels widen half rows as they load)."""
        ok = (torch.float32, torch.float16)
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim or obs.dtype not in ok or not obs.is_contiguous():
            raise ValueError(f"{self.fused}: observations must be contiguous [n, {self.obs_dim}] rows of {ok}, got "
                             f"{tuple(obs.shape)} {obs.dtype}")
        p = _ptr(obs)
        f16 = int(obs.dtype == torch.float16)
        return (p, self.obs_dim, f16) if self.fused_mlp64 else (p, f16)

    def prepare(self, obs):
        """bf16x3: split the batch's observations into bf16 pieces (navppo_mlp64_bf16x3_prepare) -- once per update, the rows do not
        change over the epochs.  The epoch entry points use the prepared buffer while `obs` is the tensor it was made from."""
        p, d, f16 = self._obs_args(obs)
        need = lib().navppo_mlp64_bf16x3_prep_bytes(int(obs.shape[0]), self.obs_dim)
        if self._prep is None or self._prep.numel() < need:
            self._prep = None
            self._prep = torch.empty(need, dtype=torch.uint8, device=self.device)
        _navppo("navppo_mlp64_bf16x3_prepare", p, d, f16, int(obs.shape[0]), _ptr(self._prep))
        self._prep_key = (obs.data_ptr(), tuple(obs.shape), obs.dtype, obs._version)

    def invalidate_prepared(self):
        """The rows behind a prepared tensor changed without torch noticing (the HIP rollout / step kernels write the trainer's
        buffers through raw pointers: no version bump).  PPOTrainer.rollout() calls this; any other writer of such a buffer must."""
        self._prep_key = None

    def _prepared(self, obs):
        """The pre-split pieces of `obs`.  Reused while `obs` is the very tensor prepare() saw, unchanged as far as torch knows
        (pointer, shape, dtype, version counter) AND nobody called invalidate_prepared() since."""
        if self._prep_key != (obs.data_ptr(), tuple(obs.shape), obs.dtype, obs._version):
            self.prepare(obs)
        return _ptr(self._prep)

    def _batch_args(self, obs, acts, logp_old, rtg, adv, var):
        """(family, the arguments every *_loss_grad / *_update_epoch entry point of it takes between params_dev and the step's): the
        rows -- obs, or their prepared pieces -- then acts, logp_old, rtg, adv, n, var, clip."""
        if self.bf16x3 and self._mb is not None:   # a slice of the prepared batch: whole tile blocks in front of it (start % 32 == 0)
            rows = (_ptr(self._prep, self._mb["prep_off"]), self.obs_dim)
        else:
            rows = (self._prepared(obs), self.obs_dim) if self.bf16x3 else self._obs_args(obs)
        fam = "navppo_mlp64_bf16x3" if self.bf16x3 else self.fused
        return fam, (*rows, _ptr(acts), _ptr(logp_old), _ptr(rtg), _ptr(adv), int(obs.shape[0]), float(var), float(self.cfg.clip))

    def _fused_loss_grad(self, obs, acts, logp_old, rtg, adv, var, stats=None):
        """evaluate + losses + backward of ppo.py:307-386 in the HIP kernels of csrc/ppo_mlp64.hip; gradients land
        in the flat gradient buffer, (actor_loss, approx_kl, clip_frac, -, critic_loss) in self._fstats."""
        for t in (acts, logp_old, rtg, adv):
            assert t.is_contiguous() and t.dtype == torch.float32
        fam, batch = self._batch_args(obs, acts, logp_old, rtg, adv, var)
        _navppo(fam + "_loss_grad", _ptr(self.fp.flat), *batch, _ptr(self.fp.grad), _ptr(self._fstats if stats is None else stats),
                _ptr(self._workspace(obs.shape[0])))

    def _fused_loss_grad_net(self, net, obs, acts, logp_old, rtg, adv, var, stats):
        """One net's half of _fused_loss_grad (navppo_mlp64[_bf16x3]_loss_grad_net): its slice of the flat gradient, its statistics."""
        fam, batch = self._batch_args(obs, acts, logp_old, rtg, adv, var)
        _navppo(fam + "_loss_grad_net", int(net), _ptr(self.fp.flat), *batch, _ptr(self.fp.grad), _ptr(stats),
                _ptr(self._workspace(obs.shape[0])))

    def _fused_adam(self, grad_scale, lo=0, n=None, step=None, cstats=None, kl_dev=None):
        """Scale + Adam on the flat buffer, or on the slice [lo, lo + n) at optimiser step `step` (one net of the pipelined epoch).
        cstats ([4], clipping on): navppo_adam_step_clipped -- per-net norm, guard and clip of the scaled gradient first.
        kl_dev ([1], target_kl on; with cstats): navppo_adam_step_kl -- the stop decision on the global approx_kl in front of that;
        adaptive lr: navppo_adam_step_lr -- the step's rate from the global approx_kl and the device state."""
        if step is None:
            self._adam_t += 1
            step = self._adam_t
        n_ = int(self.fp.numel - lo if n is None else n)
        head = tuple(_ptr(t, 4 * lo) for t in (self.fp.flat, self.fp.grad, self._adam_m, self._adam_v)) + (n_,)
        hyper = (self._lr(), *ADAM_HYPER, int(step))
        if cstats is None and kl_dev is None:
            entry, args = "navppo_adam_step", head + (float(grad_scale),) + hyper
        else:
            entry = "navppo_adam_step_clipped"
            args = head + (max(0, min(n_, self._n_actor - lo)), float(grad_scale), self._max_norm_arg()) + hyper + (_ptr(cstats),)
            if kl_dev is not None and self.lr_adaptive:
                entry, args = "navppo_adam_step_lr", args + self._lr_args() + (_ptr(kl_dev),)
            elif kl_dev is not None:
                entry, args = "navppo_adam_step_kl", args + (self.kl_limit, _ptr(self.kl_state), _ptr(kl_dev))
        _navppo(entry, *args)

    def _pipelined_epochs(self, n_ep, world, obs, acts, logp_old, rtg, adv, var_f):
        """The multi-GPU epochs of the 2x64 heads as a two-stage pipeline.  Actor and critic are disjoint nets whose losses share
        nothing inside the epoch loop (the advantages are fixed before it, ppo.py:275-284), so each net's all-reduce (RCCL's own
        stream) runs under the OTHER net's pass -- the actor's under the critic's pass of the same epoch, the critic's under the
        actor's pass of the next one -- and neither the wire time nor the cross-stream hand-over is on the compute stream's
        critical path.  Same kernels on the same data as the unpipelined order: the weights are bit-identical.
        Returns every epoch's squared norms of the mean (actor, critic) gradient.  Clipping on: each net's step is
        navppo_adam_step_clipped, which reports into its own row -- its net's columns are gathered into self.clip_stats at the end."""
        n_a = self._n_actor
        t0 = self._adam_t
        clipped = self.max_norm is not None
        nets_ = ((0, n_a, self.fp.grad[:n_a]), (n_a, self.fp.numel - n_a, self.fp.grad[n_a:]))   # (offset, parameters, gradient)
        if clipped:
            cs2 = torch.zeros((max(n_ep, 1), 2, 4), dtype=torch.float32, device=obs.device)
        else:
            gn_sq = torch.zeros((max(n_ep, 1), 2), device=obs.device)
        waits = [None, None]
        for ep in range(n_ep + 1):   # (the last round: only the steps of epoch n_ep - 1)
            for k, (lo, n, g) in enumerate(nets_):
                if waits[k] is not None:   # epoch ep - 1's gradient of net k has arrived (long ago: it had the other net's pass to do so)
                    waits[k].wait()
                    if clipped:
                        self._fused_adam(1.0 / world, lo, n, t0 + ep, cstats=cs2[ep - 1, k])
                    else:
                        self._fused_adam(1.0 / world, lo, n, t0 + ep)
                        gn_sq[ep - 1, k] = torch.dot(g, g)
                if ep < n_ep:
                    self._fused_loss_grad_net(k, obs, acts, logp_old, rtg, adv, var_f, self._fhist[ep])
                    waits[k] = dist.all_reduce(g, op=dist.ReduceOp.SUM, async_op=True)
        self._adam_t = t0 + n_ep
        if clipped:
            self.clip_stats = torch.stack([cs2[:n_ep, 0, 0], cs2[:n_ep, 1, 1], cs2[:n_ep, 0, 2], cs2[:n_ep, 1, 3]], 1)
            return self.clip_stats[:, :2]   # squared norms of the MEAN gradient, per epoch and net
        return gn_sq / float(world) ** 2

    def _fused_value(self, obs):
        """V = critic(obs).squeeze() (ppo.py:275) by the forward half of the critic's fused pass."""
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=obs.device)
        ws = (_ptr(self._workspace(obs.shape[0])),) if self.fused_resmlp512 else ()
        _navppo(self.fused + "_value", _ptr(self.fp.flat, 4 * self._n_actor), *self._obs_args(obs), int(obs.shape[0]), _ptr(out), *ws)
        return out

    def _max_norm_arg(self):
        """max_norm of the *_clipped / *_kl entry points: +inf = no clipping (target_kl without max_grad_norm)"""
        return math.inf if self.max_norm is None else self.max_norm

    def _fused_epoch(self, obs, acts, logp_old, rtg, adv, var, stats, cstats=None):
        """One epoch of ppo.py:305-392 on one GPU: losses, gradients and both Adam steps in four launches.  cstats ([4], clipping on):
        the *_update_epoch_clipped entry point -- one more small launch that clips and steps behind the reduction.  target_kl on (with
        cstats): the *_update_epoch_kl entry point -- gated twins of the same launches, the stop decision in the step launch."""
        self._adam_t += 1
        fam, batch = self._batch_args(obs, acts, logp_old, rtg, adv, var)
        mode, extra = "", ()
        if cstats is not None:
            mode, extra = "_clipped", (self._max_norm_arg(), _ptr(cstats))
        if self.kl_limit is not None:
            mode, extra = "_kl", extra + (self.kl_limit, _ptr(self.kl_state))
        elif self.lr_adaptive:   # the clipped epoch's launches, the step launch derives its rate on the device
            mode, extra = "_lr", extra + self._lr_args()
        _navppo(fam + "_update_epoch" + mode, _ptr(self.fp.flat), *batch, self._lr(), *ADAM_HYPER, int(self._adam_t),
                _ptr(self._adam_m), _ptr(self._adam_v), _ptr(self.fp.grad), _ptr(stats), _ptr(self._workspace(obs.shape[0])), *extra)

    def _clip_and_step(self, ep):
        """The PyTorch formulation of a clipped epoch's optimiser step (the CPU / gloo path and the tests' float32 reference), the
        contract of the navppo_*_clipped entry points per net: s = sum of squares of the net's gradient; s not finite: that net's
        slice of the parameters and of Adam's exp_avg / exp_avg_sq is restored after the step (the step counter advances), its
        coefficient is 0 and its gradient stays unclipped; else the gradient is scaled by min(1, max_norm / (sqrt(s) + 1e-6))."""
        n_a, cs = self._n_actor, self.clip_stats
        oks = []
        with torch.no_grad():
            for k, (lo, hi) in enumerate(((0, n_a), (n_a, self.fp.numel))):
                g = self.fp.grad[lo:hi]
                sq = (g * g).sum()
                ok = torch.isfinite(sq)
                coef = torch.where(ok, torch.clamp(self.max_norm / (sq.sqrt() + 1e-6), max=1.0), torch.zeros_like(sq))
                g.mul_(torch.where(ok, coef, torch.ones_like(coef)))
                cs[ep, k], cs[ep, 2 + k] = sq, coef
                oks.append(ok)
            st = self.opt.state.get(self.fp.proxy, {})
            keys = ("exp_avg", "exp_avg_sq")
            old = [self.fp.flat.clone()] + [st[key].clone() if key in st else torch.zeros_like(self.fp.flat) for key in keys]
        self.opt.step()
        with torch.no_grad():
            st = self.opt.state[self.fp.proxy]
            for k, (lo, hi) in enumerate(((0, n_a), (n_a, self.fp.numel))):
                for cur, was in zip([self.fp.flat] + [st[key] for key in keys], old):
                    cur[lo:hi].copy_(torch.where(oks[k], cur[lo:hi], was[lo:hi]))

    def value(self, obs):
        """V = critic(obs).squeeze() (ppo.py:275) for [n, D] rows."""
        with torch.no_grad():
            if self.fused and obs.is_contiguous() and obs.data_ptr() % 16 == 0 and obs.dtype in (torch.float32, torch.float16):
                return self._fused_value(obs)
            return self.critic(obs.float()).squeeze(-1)

    # ---- minibatches (PPOConfig.minibatch_size): the plan of an update, the one permuted copy, the steps in order
    def _plan_minibatches(self, n, multi):
        """None = whole-batch epochs (minibatch_size None or >= n: today's launches, nothing else runs), else the plan of this update:
        K slices of `size` samples per epoch (the last one shorter if n is no multiple), the shuffle mode, and -- bf16x3 -- the byte offset
        of the current slice in the prepared buffer.  Several ranks: all must hold the same n (one collective), else every rank raises."""
        cfg = self.cfg
        check_minibatch_config(cfg)
        if cfg.minibatch_size is None:
            return None
        if multi:
            nn = torch.tensor([n, -n], dtype=torch.int64, device=self.device)
            self.ctx.all_reduce_max(nn)
            hi, lo = int(nn[0]), -int(nn[1])
            if hi != lo:
                raise ValueError(f"minibatch_size: every rank must hold the same number of samples, got between {lo} and {hi} (this rank: {n})")
        if cfg.minibatch_size >= n:
            return None
        return dict(K=-(-n // cfg.minibatch_size), size=cfg.minibatch_size, n=n, mode=cfg.minibatch_shuffle, prep_off=0)

    def _shuffled(self, batch, counter):
        """`batch` gathered by batch_permutation(n, key, counter): always from the ORIGINAL batch into the one permuted copy.  Fused: one
        navppo_shuffle_batch launch (gated by kl_state: behind an early stop it returns at its entry), then -- bf16x3 -- the split of the
        permuted rows into the prepared buffer.  PyTorch: index_select by the host mirror."""
        obs = batch[0]
        n = int(obs.shape[0])
        if not self.fused:
            perm = batch_permutation(n, self._mb_key, counter).to(obs.device)
            return tuple(t.index_select(0, perm) for t in batch)
        key = (obs.dtype, obs.shape[1])
        if self._shuf is None or self._shuf_key != key or self._shuf[1].shape[0] < n:
            self._shuf = None
            f32 = dict(dtype=torch.float32, device=self.device)
            self._shuf = (torch.empty((n, obs.shape[1]), dtype=obs.dtype, device=self.device), torch.empty((n, 2), **f32),
                          torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32))
            self._shuf_key = key
        out = tuple(t[:n] for t in self._shuf)
        p, d, f16 = self._obs_args(obs)[:1] + (self.obs_dim, int(obs.dtype == torch.float16))
        _navppo("navppo_shuffle_batch", p, d, f16, *(_ptr(t) for t in batch[1:]), n, self._mb_key, int(counter), *(_ptr(t) for t in out),
                None if self.kl_state is None else _ptr(self.kl_state))
        if self.bf16x3:
            self.prepare(out[0])
        return out

    def _steps(self, n_ep, batch):
        """Every optimiser step's batch of an update, in order: n_ep times the whole batch, or -- minibatches -- per epoch its K slices,
        of the batch as it lies ("none") or of its permuted copy, drawn before every epoch ("epoch") or once ("update")."""
        mb = self._mb
        if mb is None:
            for _ in range(n_ep):
                yield batch
            return
        src = batch
        for ep in range(n_ep):
            if mb["mode"] == "epoch" or (mb["mode"] == "update" and ep == 0):
                src = self._shuffled(batch, minibatch_counter(self.update_index, ep if mb["mode"] == "epoch" else 0))
            for lo in range(0, mb["n"], mb["size"]):
                if self.bf16x3:
                    mb["prep_off"] = int(lib().navppo_mlp64_bf16x3_prep_bytes(lo, self.obs_dim))   # (0 samples: 0 bytes)
                yield tuple(t[lo:lo + mb["size"]] for t in src)

    def _epoch_losses(self, rows, k, n_ep):
        """[n_ep, 2] per-epoch (actor, critic) losses from the first k rows of `rows`, one per step that ran: K = 1 the rows themselves;
        else row e is the mean over the steps of epoch e that ran; NaN where none ran."""
        K = self._mb["K"] if self._mb is not None else 1
        if K == 1:
            losses = rows[:k].clone()
            return losses if k >= n_ep else torch.cat([losses, torch.full((n_ep - k, 2), math.nan, device=rows.device)])
        ran = (torch.arange(n_ep * K, device=rows.device) < k).reshape(n_ep, K, 1)
        r = torch.where(ran, rows[:n_ep * K].reshape(n_ep, K, 2), torch.zeros((), device=rows.device))
        return r.sum(1) / ran.sum(1)   # (0 / 0: NaN)

    def _clip_row(self, ep, c):
        """This epoch's clip-statistics row from the gradient as it stands, coefficient c: 0 = the update stopped before this step, 1 = unclipped."""
        g_a, g_c = self.fp.grad[:self._n_actor], self.fp.grad[self._n_actor:]
        self.clip_stats[ep] = torch.stack([(g_a * g_a).sum(), (g_c * g_c).sum(), g_a.new_full((), c), g_a.new_full((), c)])

    def _fused_record(self, n_ep, V0, world, r0, gn_sum=None, net_gn=None):
        """What every fused runner ends with: ONE synchronisation (kl_state) after the last epoch, then the record from the first k rows
        of _fhist.  gn_sum / net_gn: the runner's own sums of norms; the single-GPU epochs have none and take them from the rows."""
        if n_ep == 0:
            return r0
        K = self._mb["K"] if self._mb is not None else 1
        n_st = n_ep * K   # optimiser steps queued: with minibatches every row below is a STEP's
        steps, stopped = n_st, 0
        if self.kl_limit is not None:   # (the update synchronises for its statistics anyway)
            st = self.kl_state.tolist()
            steps, stopped = int(st[1]), int(st[0] != 0.0)
            self._adam_t -= n_st - steps   # Adam's bias correction counts steps TAKEN: every step's launch counted one
        k = steps + stopped
        h = self._fhist[:k]
        losses = self._epoch_losses(self._fhist[:, 0:5:4], k, n_ep)   # columns 0 (actor loss) and 4 (critic loss)
        gn_last = self.fp.grad.norm() / world   # multi-GPU: fp.grad holds the all-reduced SUM (the 1 / world scale is inside navppo_adam_step)
        own = gn_sum is not None
        if not own and not self._clipping:
            # every epoch's norms as the reference logs them (ppo.py:351-352, 389-390) without a norm launch per epoch: the fused epoch leaves
            # the squared per-net norms of the epoch BEFORE in columns 3 / 7 of its row (reduce_adam / resmlp_reduce), the last epoch's stand
            # (minibatches: a row per step, the slots of the step before -- reduce_adam's lie at a fixed place of the workspace and its grid
            # does not depend on n, so a shorter last slice and an epoch boundary change nothing; resmlp_reduce's lie BEHIND the per-sample
            # part of the workspace and move with n: _run_fused_single takes that family's norms itself when the slices are not all equal)
            if n_st > 1:
                prev = h[1:, 3:8:4].clone()   # [n_st - 1, (actor, critic)]
                gn_sum, net_gn = prev.sum(1).sqrt().sum() + gn_last, prev.sqrt().sum(0)
            else:
                gn_sum = gn_last * n_st
        return _Epochs(k=k, steps=steps, stopped=stopped, losses=losses, sums=h.sum(0)[[0, 4, 1, 2]], gn_sum=gn_sum, v_sum=V0.mean() * k,
                       net_gn=net_gn, net_gn_open=not own, K=K)

    def _run_fused_single(self, n_ep, batch, var_f, V0, multi, world, r0):
        """One GPU: _fused_epoch.  Per-epoch diagnostics land in row ep of a device buffer: no extra launches inside the epoch loop."""
        # gn (resmlp512 on slices of two lengths, no clip statistics): every step's per-net norms by two small launches -- the slot of
        # the step before is read at the wrong place when n changes between two calls (the shorter last slice, the epoch boundary)
        mb, n_a = self._mb, self._n_actor
        gn = (torch.zeros((n_ep * mb["K"], 2), device=self.device)
              if mb is not None and self.fused_resmlp512 and not self._clipping and mb["n"] % mb["size"] else None)
        for st, sl in enumerate(self._steps(n_ep, batch)):
            self._fused_epoch(*sl, var_f, self._fhist[st], self.clip_stats[st] if self._clipping else None)
            if gn is not None:
                gn[st] = torch.stack(torch._foreach_norm([self.fp.grad[:n_a], self.fp.grad[n_a:]]))
        if self.lr_adaptive:
            self.kl_steps = self._fhist[:self._lr_step, 1].clone()
        return self._fused_record(n_ep, V0, world, r0, *((gn.pow(2).sum(1).sqrt().sum(), gn.sum(0)) if gn is not None and n_ep > 0 else ()))

    def _run_fused_multi(self, n_ep, batch, var_f, V0, multi, world, r0):
        """Several GPUs: fused passes -> ONE all-reduce of the flat gradient (RCCL) -> scale + Adam in one launch."""
        ctx, n_a, gn = self.ctx, self._n_actor, None   # gn: step sums of the MEAN gradient's (actor, critic, whole) norm
        n_st = n_ep * (self._mb["K"] if self._mb is not None else 1)
        need_kl = self.kl_limit is not None or self.lr_adaptive   # (adaptive lr: every rank must derive the same rate)
        kl_glob = torch.zeros((max(n_st, 1), 2), dtype=torch.float32, device=self.device) if need_kl else None
        for ep, sl in enumerate(self._steps(n_ep, batch)):   # (ep: the step -- an epoch, or a slice of one)
            n = float(sl[0].shape[0])
            self._fused_loss_grad(*sl, var_f, stats=self._fhist[ep])
            ctx.all_reduce_sum(self.fp.grad)
            if need_kl:
                # the global approx_kl = sum(kl_r n_r) / sum(n_r), a 2-float collective; the passes are ungated: a stop only keeps the weights
                kg = kl_glob[ep]
                kg[0], kg[1] = self._fhist[ep, 1] * n, n
                ctx.all_reduce_sum(kg)
                kg[0] /= kg[1]
                self._fused_adam(1.0 / world, cstats=self.clip_stats[ep], kl_dev=kg)
            elif self._clipping:   # (the norms of the mean gradient are in the clip statistics)
                self._fused_adam(1.0 / world, cstats=self.clip_stats[ep])
            else:   # every epoch's norms of the MEAN gradient (two small launches beside an all-reduce)
                g3 = torch.stack(torch._foreach_norm([self.fp.grad[:n_a], self.fp.grad[n_a:], self.fp.grad])) / world
                gn = g3 if gn is None else gn + g3
                self._fused_adam(1.0 / world)
        if self.lr_adaptive:
            self.kl_steps = kl_glob[:n_st, 0]
        return self._fused_record(n_ep, V0, world, r0, *((gn[2], gn[:2]) if gn is not None else ()))

    def _run_fused_pipelined(self, n_ep, batch, var_f, V0, multi, world, r0):
        """Several GPUs, overlap_allreduce: every epoch runs in _pipelined_epochs; pg: its squared norms of the MEAN gradient."""
        pg = self._pipelined_epochs(n_ep, world, *batch, var_f)
        gn = torch.cat([pg.sqrt().sum(0), pg.sum(1).sqrt().sum().reshape(1)]) if n_ep > 0 else None
        return self._fused_record(n_ep, V0, world, r0, *((gn[2], gn[:2]) if gn is not None else ()))

    def _run_pytorch(self, n_ep, batch, var, V0, multi, world, r0):
        """CPU, gloo, and resmlp512 with update_arith="f32": ppo.py:305-392 in PyTorch."""
        K = self._mb["K"] if self._mb is not None else 1
        steps, stopped, losses = n_ep * K, 0, torch.zeros((n_ep * K, 2), device=batch[0].device)   # (a row per step)
        acc, net_gn = torch.zeros(6, device=batch[0].device), None  # sums over steps of the diagnostics and of the per-net gradient norms
        kls = []   # adaptive lr: every step's (global) approx_kl, float32
        for ep, (obs, acts, logp_old, rtg, adv) in enumerate(self._steps(n_ep, batch)):   # ppo.py:305 (ep: the step -- an epoch, or a slice of one)
            a_loss, c_loss, ratios, logp, _ = ppo_losses(self.actor, self.critic, obs, acts, logp_old, rtg, adv, var, self.cfg.clip)
            self.fp.grad.zero_()
            (a_loss + c_loss).backward()                       # disjoint nets: same grads as the two backward()s of :349,:386
            if multi:
                self.ctx.all_reduce_sum(self.fp.grad)
                self.fp.grad.div_(world)
            ratios, lr_, trip = ratios.detach(), logp.detach() - logp_old, False
            if self.kl_limit is not None:   # the check before the step, on the global approx_kl (weighted by the ranks' batch sizes); a NaN trips
                kg = torch.stack([((ratios - 1) - lr_).sum(), lr_.new_tensor(float(lr_.numel()))])
                if multi:
                    self.ctx.all_reduce_sum(kg)
                trip = not (float(kg[0] / kg[1]) <= self.kl_limit)
            if self.lr_adaptive:   # the rule before the step, on the global approx_kl, through the kernel's host mirror; not on an update's first step
                kl = float(((ratios - 1) - lr_).mean())
                if multi:   # (weighted by the ranks' batch sizes, as target_kl's)
                    kg = torch.stack([((ratios - 1) - lr_).sum(), lr_.new_tensor(float(lr_.numel()))])
                    self.ctx.all_reduce_sum(kg)
                    kl = float(kg[0] / kg[1])
                d = adaptive_lr_direction(kl, self.cfg.desired_kl, adapt=ep > 0)
                self.lr_value = adaptive_lr_reference(self.lr_value, kl, self.cfg.desired_kl, self.cfg.lr_min, self.cfg.lr_max, adapt=ep > 0)
                self.lr_counts = (self.lr_counts[0] + (d > 0), self.lr_counts[1] + (d < 0))
                self.opt.param_groups[0]["lr"] = self.lr_value
                kls.append(kl)
                self._lr_step += 1
            if trip:   # neither net is stepped; the gradient stays unclipped, the coefficients are reported as 0, the remaining epochs do not run
                steps, stopped = ep, 1
                self._clip_row(ep, 0.0)
            elif self.max_norm is not None:
                self._clip_and_step(ep)
            else:
                self.opt.step()                                # ppo.py:381,392
                if self._clipping:   # (target_kl without max_grad_norm: the norms of every epoch, coefficient 1)
                    self._clip_row(ep, 1.0)
            with torch.no_grad():                              # ppo.py:323-336
                losses[ep] = torch.stack([a_loss.detach(), c_loss.detach()])
                acc += torch.stack([a_loss.detach(), c_loss.detach(), ((ratios - 1) - lr_).mean(),
                                    ((ratios - 1).abs() > self.cfg.clip).float().mean(), self.fp.grad.norm(), V0.mean()])
                g2 = torch.stack(torch._foreach_norm([self.fp.grad[:self._n_actor], self.fp.grad[self._n_actor:]]))
                net_gn = g2 if net_gn is None else net_gn + g2
            if trip:
                break
        if self.lr_adaptive:
            self.kl_steps = torch.tensor(kls, dtype=torch.float32)
        return _Epochs(k=steps + stopped, steps=steps, stopped=stopped, losses=self._epoch_losses(losses, steps + stopped, n_ep), sums=acc[:4],
                       gn_sum=acc[4], v_sum=acc[5], net_gn=net_gn, K=K)

    def _summarise(self, r, flat_before, multi, world):
        """The record of the epochs that ran -> the stats dict.  Gradient norms are means over the r.k epochs, from the first source
        that has them: the clip statistics (every epoch's pre-clip norms), the runner's own sums, the gradient as it stands."""
        k, n_a, clipping = r.k, self._n_actor, self._clipping
        cs = self.clip_stats[:k] if clipping else None
        # every epoch's pre-clip norm of the whole gradient: folded in before the ranks' mean when fused, after it in PyTorch (not the same last bit)
        total = cs[:, :2].sum(1).sqrt() if clipping and k > 0 else None
        acc = torch.cat([r.sums, torch.stack([total.sum() if total is not None and self.fused else r.gn_sum, r.v_sum])]) / max(k, 1)
        if multi:
            self.ctx.all_reduce_sum(acc)
            acc = acc / world
        if total is not None and not self.fused:
            acc = torch.cat([acc[:4], total.mean().reshape(1), acc[5:]])
        d = self.fp.flat - flat_before                         # the parameter-delta diagnostics of ppo.py:402-403
        extra = torch.stack(torch._foreach_norm([self.fp.grad[:n_a], self.fp.grad[n_a:], d[:n_a], d[n_a:]]))
        if self.fused and multi:
            extra = extra * extra.new_tensor([1.0 / world, 1.0 / world, 1.0, 1.0])   # norms of the MEAN gradient, as on one GPU
        if total is not None:
            extra = torch.cat([cs[:, :2].sqrt().mean(0), extra[2:]])
        elif r.net_gn is not None:   # (open: the runner's sums lack the last epoch, whose gradient still stands)
            extra = torch.cat([(r.net_gn + extra[:2] if r.net_gn_open else r.net_gn) / k, extra[2:]])
        clip_cols = []
        if clipping:   # share of clipped epochs, skipped steps; identical on every rank
            # (not the tripping epoch: its coefficient is 0 because the update stopped, not because anything was clipped or skipped)
            clipped_ep = (cs[:, 2:] < 1.0)[:k - r.stopped]
            clip_cols = [clipped_ep.float().sum(0) / max(k, 1), (~torch.isfinite(cs[:, :2])).float().sum(0)]
            if k == 0:
                clip_cols = [torch.zeros(2, device=self.device)] * 2
        # (the last four keys exist with max_grad_norm only -- not with target_kl alone: without it the trainer's log dictionary is what it was)
        keys = ["actor_loss", "critic_loss", "approx_kl", "clip_frac", "grad_norm", "value_mean", "actor_grad_norm", "critic_grad_norm",
                "actor_param_delta", "critic_param_delta",
                "grad_clip_frac_actor", "grad_clip_frac_critic", "skipped_steps_actor", "skipped_steps_critic"]
        lr_cols = [self.lr_state] if self.lr_state is not None else []   # (adaptive lr, fused: the state rides on this read-back)
        vals = [float(v) for v in torch.cat([acc, extra] + (clip_cols if self.max_norm is not None else []) + lr_cols).tolist()]
        if lr_cols:   # the slot the last step wrote; the counts are cumulative
            vals, st = vals[:-4], vals[-4:]
            if self._lr_step > 0:
                self.lr_value = st[(self._adam_t + 1) & 1]
            ups, downs = int(st[2]), int(st[3])
        elif self.lr_adaptive:
            ups, downs = self.lr_counts
        stats = dict(zip(keys, vals[:12] + [int(v) for v in vals[12:]]))
        if self.lr_adaptive:   # the rate after the update's last step, the raises and lowerings of this update; identical on every rank
            stats["lr"], stats["lr_ups"], stats["lr_downs"] = self.lr_value, ups - self._lr_counts0[0], downs - self._lr_counts0[1]
            self.lr_counts = (ups, downs)
        elif self.lr_value is not None:   # ("linear": the rate this update ran with)
            stats["lr"] = self.lr_value
        if self.kl_limit is not None:   # steps taken (n_ep if the update never stopped) and whether it stopped; identical on every rank
            # (minibatches: kl_stop_step counts the steps, kl_stop_epoch the whole epochs completed)
            stats["kl_stop_epoch"], stats["kl_stopped"] = r.steps // r.K, r.stopped
            if r.K > 1:
                stats["kl_stop_step"] = r.steps
        return stats

    def update(self, obs, acts, logp_old, rtg, var, adv_raw=None, V0=None):
        """adv_raw / V0: advantages (before normalisation) and values computed by the caller (GAE); default = the reference's
        A = rtg - V (ppo.py:275-277).  Prologue, the epochs on the one path that applies, the summary, the published results."""
        cfg, ctx, n_ep = self.cfg, self.ctx, self.cfg.n_updates_per_iteration
        world, multi = (ctx.world, ctx.enabled) if ctx is not None else (1, False)   # multi: collectives run (also one forced rank)
        with torch.no_grad():
            V0 = self.value(obs) if V0 is None else V0
            adv = normalise_advantages(rtg - V0 if adv_raw is None else adv_raw, ctx)          # ppo.py:275-284
        flat_before = self.fp.flat.clone()
        zero = torch.zeros((), device=obs.device)   # n_updates_per_iteration == 0: nothing to report
        r0 = _Epochs(k=0, steps=0, stopped=0, losses=torch.zeros((n_ep, 2), device=obs.device), sums=torch.zeros(4, device=obs.device),
                     gn_sum=zero, v_sum=zero)
        if not (self.fused and obs.dtype == torch.float16):
            obs = obs.float()   # half rows (obs_f16 envs) are consumed as they are by the fused kernels only
        batch = (obs, acts, logp_old, rtg, adv)
        self._mb = self._plan_minibatches(int(obs.shape[0]), multi)
        self._lr_step, self._lr_counts0 = 0, self.lr_counts
        n_st = n_ep * (self._mb["K"] if self._mb is not None else 1)   # optimiser steps: a row of every per-step buffer each
        shuffling = self._mb is not None and self._mb["mode"] != "none"
        if self.fused:
            batch = tuple(t.contiguous() for t in batch)
            if self.bf16x3 and n_ep > 0 and not shuffling:   # (shuffling: the permuted copy is prepared behind every shuffle instead)
                self.prepare(batch[0])   # ALWAYS here: the rollout kernels fill the buffer behind torch's back (no version bump)
            if self._fhist.shape[0] < n_st:
                self._fhist = torch.zeros((n_st, 8), dtype=torch.float32, device=self.device)
            if self.kl_limit is not None:   # zeroed once per update; afterwards only the library writes it
                self.kl_state = torch.zeros(4, dtype=torch.float32, device=obs.device)
        if self._clipping:   # every step's (s_actor, s_critic, coef_actor, coef_critic): filled on the device, read once after the epochs
            self.clip_stats = torch.zeros((max(n_st, 1), 4), dtype=torch.float32, device=obs.device)
        self._last_adv = batch[4]   # (PPOTrainer._grad_guard's diagnostics)
        if cfg.norm_reward:
            self._last_V0 = V0      # (the trainer's explained_variance: the critic before this update)
        runner = (self._run_pytorch if not self.fused else self._run_fused_single if not multi else
                  self._run_fused_pipelined if self.fused_mlp64 and cfg.overlap_allreduce else self._run_fused_multi)
        try:
            run = runner(n_ep, batch, float(var) if self.fused else var, V0, multi, world, r0)
            self.stats = self._summarise(run, flat_before, multi, world)
        finally:   # (the plan belongs to this update: _batch_args of a later call on a whole batch must not see it)
            self._mb = None
            self.update_index += 1
        self.loss_history = run.losses   # per-epoch (actor, critic) loss, ppo.py:396-397; NaN rows behind an early stop
        last = (run.k - 1) // run.K      # the last epoch a step of which ran
        self.last_losses = (run.losses[last, 0].detach(), run.losses[last, 1].detach()) if run.k else (zero, zero)
        return self.stats


# --------------------------------------------------------------------------- trainer
class PPOTrainer:
    """PPO.learn for a ``VecEnv`` shard.  Construct one per process (= per GPU)."""

    def __init__(self, env, cfg=None, ctx=None):
        self.env, self.cfg = env, cfg or PPOConfig()
        self.ctx = ctx
        self.device = env.device
        cfg = self.cfg
        N, T, D = env.N, cfg.rollout_len, env.D
        torch.manual_seed(cfg.seed)  # same initial weights on every rank (then broadcast anyway)
        self.actor, self.critic = nets.make_policy(cfg.policy, D, 2)
        self.actor.to(self.device)
        self.critic.to(self.device)
        self.updater = PPOUpdater(self.actor, self.critic, cfg, ctx, self.device)
        rank = ctx.rank if ctx is not None else 0
        torch.manual_seed(cfg.seed * 1000003 + 17 + rank)  # exploration noise differs per shard
        dev = self.device
        f32, u8 = torch.float32, torch.uint8
        # the observation rows in the dtype the simulator writes them (float16 on an obs_f16 env: BASELINE configs[4]); half rows
        # are read directly by the fused kernels of both policies (round 6: the 512-wide ones too), a PyTorch policy widens them
        self.obs_buf = torch.zeros((T + 1, N, D), dtype=env.sim.obs_dtype, device=dev)
        self._half_obs = env.sim.obs_dtype == torch.float16
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
        if cfg.norm_reward:   # (off: not one tensor, launch or read-back more than before)
            self._init_ret_rms(dev)
            self.rew_scaled_buf = torch.zeros((T, N), dtype=f32, device=dev)   # what the scans read; rew_buf keeps the raw rewards
            self._ret_rows = torch.zeros((ctx.world if ctx is not None else 1, 3), dtype=torch.float64, device=dev)   # one row per rank
        self.var = torch.full((), cfg.init_var, dtype=f32, device=dev)  # ppo.py:123-124 (0.8 * I)
        self.var_host = float(cfg.init_var)   # host mirror, refreshed at every rollout start
        self._lo = torch.tensor([0.0, -1.0], device=dev)
        self._hi = torch.tensor([1.0, 1.0], device=dev)
        self._graph = None
        self._step_base = torch.zeros((), dtype=torch.int32, device=dev)  # rollout steps taken so far (noise counter)
        self._act_seed = (cfg.seed * 0x9E3779B97F4A7C15 + 0xAC7) & 0xFFFFFFFFFFFFFFFF
        self._env_id_base = int(env.sim.cfg.env_id_base)
        self.t_so_far = 0     # completed-episode steps, as the reference counts (ppo.py:258)
        self.env_steps = 0    # all simulated steps
        self.i_so_far = 0
        self.episode_starts = 0
        self.logger = {}

    # ---- PPOConfig.norm_reward: the running statistics of the discounted return and the scaled copy of a rollout's rewards
    def _init_ret_rms(self, device, mean=RET_RMS_INIT[0], var=RET_RMS_INIT[1], count=RET_RMS_INIT[2]):
        """ret_rms = (mean, var, count, scale), float64 on the device; a fresh run starts like RunningMeanStd (0, 1, 1e-4)."""
        mean, var, count = float(mean), float(var), float(count)
        self.ret_rms = torch.tensor([mean, var, count, 1.0 / math.sqrt(var + self.cfg.norm_reward_eps)], dtype=torch.float64, device=device)

    def _normalise_rewards(self):
        """Behind the rollout, in front of the return scan: this rank's (n, mean, M2) of the rollout's running returns (carry-in 0:
        every rollout starts from a reset), every rank's row gathered by ONE all-reduce of a zero-filled [world, 3] tensor (adding
        zeros is exact), all rows merged in rank order on every rank -- bit-identical statistics -- and the rollout scaled by them.
        Two entry points, no host round trip."""
        cfg, ctx = self.cfg, self.ctx
        rows = self._ret_rows
        multi = ctx is not None and ctx.enabled
        if multi and rows.shape[0] > 1:
            rows.zero_()
        return_moments(self.rew_buf, self.ended_buf, cfg.gamma, out=rows[ctx.rank if ctx is not None else 0])
        if multi:
            ctx.all_reduce_sum(rows)
        return reward_scale(self.ret_rms, rows, self.rew_buf, clip=cfg.clip_reward, eps=cfg.norm_reward_eps, out=self.rew_scaled_buf)

    def _reward_norm_figures_dev(self):
        """(mean, var, count, scale, explained variance) as one float64 device tensor, queued behind the update and read with the
        iteration's one read-back.  explained_variance = 1 - Var(target - V0) / Var(target) over this rank's samples, V0 the critic
        before the update: scale-free, unlike critic_loss, whose units change with the option."""
        tgt, v0 = self.rtg_buf.reshape(-1).double(), self.updater._last_V0.reshape(-1).double()
        ev = 1.0 - (tgt - v0).var(unbiased=False) / tgt.var(unbiased=False)
        return torch.cat([self.ret_rms, ev.reshape(1)])

    def _fused_act(self, t, noise=None):
        """PPO.get_action for all envs in ONE launch (csrc/ppo_mlp64.hip: mlp64_act, csrc/ppo_resmlp512.hip: resmlp_act)."""
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        L = lib()
        rc = getattr(L, self.updater.fused + "_act")(ptr(self.updater.fp.flat), *self.updater._obs_args(self.obs_buf[t]), ptr(noise), self.env.N,
                                                     ptr(self.var), self._act_seed, self._env_id_base, ptr(self._step_base), t,
                                                     ptr(self.act_buf[t]), ptr(self.logp_buf[t]), None,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"{self.updater.fused}_act failed: {L.navppo_last_error().decode()}")

    # ---- ppo.py:673-706 + env.step, for rollout step t (all envs)
    def _rollout_step(self, t):
        if self.updater.fused:
            self._fused_act(t)
            self.env.sim.step(self.act_buf[t], self.obs_buf[t + 1], self.rew_buf[t], self.done_buf[t], self.arrive_buf[t],
                              self.ended_buf[t], self.epret_buf[t], self.eplen_buf[t], ep_path=self.eppath_buf[t])
            return
        obs = self.obs_buf[t].float()
        mean = self.actor(obs)
        std = torch.sqrt(self.var)
        raw = torch.addcmul(mean, torch.randn_like(mean), std)          # dist.sample(), ppo.py:698
        act = self.act_buf[t]
        torch.clamp(raw, self._lo, self._hi, out=act)                   # ppo.py:700-703
        self.logp_buf[t] = gaussian_log_prob(mean, act, self.var)       # log-prob of the clamped action, :704
        self.env.sim.step(act, self.obs_buf[t + 1], self.rew_buf[t], self.done_buf[t], self.arrive_buf[t],
                          self.ended_buf[t], self.epret_buf[t], self.eplen_buf[t], ep_path=self.eppath_buf[t])

    def _persistent_rollout(self):
        """ppo.py:505-594 in ONE launch (csrc/navsim.hip: rollout_kernel): policy step and env step alternate inside the
        kernel; same device functions and Philox keys as the per-step path, so the buffers come out bit-identical."""
        ptr = lambda x: C.c_void_p(x.data_ptr())
        sim = self.env.sim
        entry = lib().navsim_rollout_resmlp512 if self.updater.fused_resmlp512 else lib().navsim_rollout_mlp64
        with torch.cuda.device(self.device):
            check(entry(sim._h, ptr(self.updater.fp.flat), ptr(self.obs_buf), ptr(self.act_buf),
                                             ptr(self.logp_buf), ptr(self.rew_buf), ptr(self.done_buf), ptr(self.arrive_buf),
                                             ptr(self.ended_buf), ptr(self.epret_buf), ptr(self.eplen_buf), ptr(self.eppath_buf),
                                             ptr(self.var), self._act_seed, ptr(self._step_base), self.cfg.rollout_len,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "navsim_rollout_" + ("resmlp512" if self.updater.fused_resmlp512 else "mlp64"))
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

    @torch.no_grad()
    def rollout(self):
        cfg = self.cfg
        self._decay_exploration()
        self.epret_buf.zero_()
        self.eplen_buf.zero_()
        self.updater.invalidate_prepared()   # the kernels below rewrite obs_buf behind torch's version counter
        self.env.sim.reset(self.obs_buf[0])  # ppo.py:486: every batch starts from a reset
        sim = self.env.sim
        # (round 5: both rollout kernels have the tile-box cast of shared 65..4096-segment maps; until then shards up to 4096 envs on
        # such a map took the hipGraph of per-step launches)
        if self.uses_persistent_rollout:
            self._persistent_rollout()
        elif cfg.use_graph and self.device.type == "cuda":
            if self._graph is not None and self._graph_gen != self.env.sim.generation:
                self._graph = None   # set_map / set_spawn_sampler / set_goal_rects re-allocated what the capture froze
            if self._graph is None:
                self._graph_gen = self.env.sim.generation
                s = torch.cuda.Stream(self.device)
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):  # warm-up outside capture (allocator, hipBLASLt workspaces)
                    self._rollout_step(0)
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                self.env.sim.reset(self.obs_buf[0])
                self._graph = torch.cuda.CUDAGraph()
                # thread_local: other threads (the RCCL watchdog of torch.distributed) may touch the HIP runtime while
                # this thread captures; the default global mode would turn that into a capture error on multi-GPU runs
                with torch.cuda.graph(self._graph, capture_error_mode="thread_local"):
                    self._rollout_body()
            self._graph.replay()
        else:
            self._rollout_body()
        from .env import gae_scan, gae_scan_trunc, rtg_scan
        self._gae = None
        rew = self._normalise_rewards() if cfg.norm_reward else self.rew_buf   # (the scans below are the same either way)
        if cfg.bootstrap_truncated:
            # extension: neither a time-out nor the batch end is the end of the robot.  V of all T + 1 stored rows; a time-out row adds
            # gamma V of its own observation (the terminal observation is gone: the step kernels store the reset one), the envs still
            # running on the last row bootstrap with V(obs_buf[T]) (ended[T-1] cuts that for an env that ended there) -- for every
            # lambda; None runs as 1: the reference's A = R - V on truncation-aware returns.  rew is in the critic's units either way.
            T, N, D = cfg.rollout_len, self.env.N, self.env.D
            Vall = self.updater.value(self.obs_buf.reshape(-1, D)).reshape(-1, N)
            V = Vall[:T].contiguous()
            adv, ret = gae_scan_trunc(rew, self.ended_buf, self.done_buf, self.arrive_buf, V, cfg.gamma,
                                      1.0 if cfg.gae_lambda is None else cfg.gae_lambda, last_value=Vall[T])
            self.rtg_buf.copy_(ret)
            self._gae = (adv.reshape(T * N), V.reshape(T * N))
        elif cfg.gae_lambda is None:
            rtg_scan(rew, self.ended_buf, cfg.gamma, out=self.rtg_buf)  # ppo.py:619 -> 643-671
        else:   # extension: the critic's values of the stored observations -> lambda-returns (critic targets) and advantages
            # lambda < 1: the envs still running at the batch end are bootstrapped with V(obs_buf[T]), the observation behind the last
            # row (an env that ended on the last row has ended[T-1] set, which cuts the bootstrap).  lambda = 1 keeps the reference's
            # convention -- the batch end is terminal, ppo.py:601,658-666 -- and stays bit-identical to compute_rtgs.
            T, N, D = cfg.rollout_len, self.env.N, self.env.D
            boot = cfg.gae_lambda < 1.0
            Vall = self.updater.value(self.obs_buf[:T + 1 if boot else T].reshape(-1, D)).reshape(-1, N)
            V = Vall[:T].contiguous()
            adv, ret = gae_scan(rew, self.ended_buf, V, cfg.gamma, cfg.gae_lambda, last_value=Vall[T] if boot else None)
            self.rtg_buf.copy_(ret)
            self._gae = (adv.reshape(T * N), V.reshape(T * N))
        self.env_steps += cfg.rollout_len * self.env.N

    def _decay_exploration(self):
        """ppo.py:694-695 multiplies the covariance by 0.995 at every episode start once t_so_far > 50000 while
        it is >= 0.1, with t_so_far frozen during a rollout.  With N envs there are N x more episode starts per
        iteration, so the decay is applied once per N episode starts (per mean episode) -- identical for N=1
        up to being applied at the rollout boundary; documented deviation."""
        cfg = self.cfg
        v = float(self.var)   # the one read-back of the iteration, at its start (the stream is idle here)
        if self.t_so_far > cfg.var_decay_after:
            k = int(round(self.episode_starts / max(self.env.N, 1)))
            for _ in range(k):
                if v >= cfg.var_floor:
                    v *= cfg.var_decay
            self.var.fill_(v)
        self.var_host = v
        self.episode_starts = 0

    def _rollout_metrics_dev(self):
        """The six sums behind the iteration's episode metrics as ONE device tensor (all-reduced over the ranks); nothing
        here waits for the GPU, so the update can be queued behind it."""
        ptr = lambda x: C.c_void_p(x.data_ptr())
        if getattr(self, "_sums_ws", None) is None:
            self._sums_ws = torch.empty(256 * 6, dtype=torch.float64, device=self.device)
        m = torch.empty(6, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = lib().navppo_episode_sums(ptr(self.ended_buf), ptr(self.arrive_buf), ptr(self.done_buf), ptr(self.eplen_buf),
                                           ptr(self.epret_buf), self.ended_buf.numel(), ptr(m), ptr(self._sums_ws),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"navppo_episode_sums failed: {lib().navppo_last_error().decode()}")
        if self.ctx is not None:
            self.ctx.all_reduce_sum(m)
        return m

    def _rollout_metrics(self, m=None):
        m = self._rollout_metrics_dev() if m is None else m   # (a tensor, or the six figures already on the host)
        ep, succ, coll, tmo, steps, ret = [float(x) for x in (m.tolist() if torch.is_tensor(m) else m)]
        self.episode_starts = ep / (self.ctx.world if self.ctx is not None else 1) + self.env.N
        return dict(episodes=int(ep), successes=int(succ), collisions=int(coll), timeouts=int(tmo),
                    completed_steps=int(steps), avg_ep_rews=(ret / ep if ep else 0.0),       # ppo.py:833
                    avg_ep_lens=(steps / ep if ep else 0.0), success_rate=(succ / ep if ep else 0.0))

    def iteration(self):
        """One pass of the loop of PPO.learn (ppo.py:241-459).  Rollout, metric sums and update are queued back to back and
        the host waits once, at the end; rollout / update times come from events on the stream (wall clock on CPU)."""
        cfg = self.cfg
        cuda = self.device.type == "cuda"
        T, N, D = cfg.rollout_len, self.env.N, self.env.D
        t0 = time.time()
        if cuda:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        self.rollout()
        if cuda:
            ev[1].record()
        t1 = time.time()
        m = self._rollout_metrics_dev()
        stats = self.updater.update(self.obs_buf[:T].reshape(T * N, D), self.act_buf.reshape(T * N, 2),
                                    self.logp_buf.reshape(T * N), self.rtg_buf.reshape(T * N),
                                    self.var_host if self.updater.fused else self.var,
                                    **({} if self._gae is None else dict(adv_raw=self._gae[0], V0=self._gae[1])))
        if cuda:
            ev[2].record()
        if cfg.norm_reward:   # the option's figures ride on the episode sums' read-back below: one tensor, one copy
            m = torch.cat([m, self._reward_norm_figures_dev()])
        if cuda:
            torch.cuda.synchronize(self.device)
        t2 = time.time()
        if cuda:   # the host ran ahead of the stream: split the wall clock of the iteration by the stream's own stamps
            r_ms, u_ms = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
            t1 = t0 + (t2 - t0) * r_ms / max(r_ms + u_ms, 1e-9)
        if cfg.norm_reward:
            m = m.tolist()
            rn, m = m[6:], m[:6]
            stats = dict(stats, reward_scale=rn[3], ret_rms_mean=rn[0], ret_rms_std=math.sqrt(max(rn[1], 0.0)), explained_variance=rn[4])
        metrics = self._rollout_metrics(m)
        if cfg.bootstrap_truncated:   # the share of rows the scan bootstrapped as time-outs: the episode sums' figure, nothing launched
            stats = dict(stats, bootstrapped_frac=metrics["timeouts"] / max(T * N * (self.ctx.world if self.ctx is not None else 1), 1))
        self.t_so_far += metrics["completed_steps"]
        self.i_so_far += 1
        self._grad_guard(stats)
        world = self.ctx.world if self.ctx is not None else 1
        self.logger = dict(metrics, **stats, iteration=self.i_so_far, t_so_far=self.t_so_far,
                           rollout_time=t1 - t0, update_time=t2 - t1, iter_time=t2 - t0,
                           steps_per_sec=T * N * world / (t2 - t0),                      # ppo.py:855
                           rollout_steps_per_sec=T * N * world / (t1 - t0), var=self.var_host)
        if cfg.eval_every > 0 and self.i_so_far % cfg.eval_every == 0 and (self.ctx is None or self.ctx.rank == 0):
            self.logger.update(self.evaluate_now())   # rank 0 alone, no collective: the other ranks go on to their next rollout
        if cfg.output_dir and (self.ctx is None or self.ctx.rank == 0):
            if self.i_so_far % cfg.save_freq == 0:
                self.save_checkpoint()
            import json
            os.makedirs(self.log_dir(), exist_ok=True)
            with open(os.path.join(self.log_dir(), "scalars.jsonl"), "a") as f:
                f.write(json.dumps(dict(self.tb_scalars(), iteration=self.i_so_far, t_so_far=self.t_so_far)) + "\n")
            if cfg.episode_csv_rows:
                self.write_episode_csv(cfg.episode_csv_rows)
            self.write_tensorboard()
        return self.logger

    # ---- the gradient check of the reference (ppo.py:356-379, 414-416), once per iteration on figures that are already on the host
    def _grad_guard(self, stats, log=print):
        """A per-net mean gradient norm that is <= 0 or not finite, a loss that is not finite, or a skipped step (max_grad_norm):
        the reference's warning line, and a block in <output_dir>/grad_diagnostics.txt.  No launch and no sync unless it triggers
        (then a few reductions over the advantages for the file); it reports only -- what happens to the weights is decided by
        PPOConfig.max_grad_norm inside the update -- and never raises.  Returns the nets that triggered."""
        cfg = self.cfg
        if cfg.n_updates_per_iteration < 1:
            return []
        hit = []
        for net in ("actor", "critic"):
            gn, loss, sk = stats.get(net + "_grad_norm", 0.0), stats.get(net + "_loss", 0.0), stats.get("skipped_steps_" + net, 0)
            if gn <= 0 or not math.isfinite(gn) or not math.isfinite(loss) or sk > 0:
                hit.append((net, gn, loss, sk))
        if not hit or not (self.ctx is None or self.ctx.rank == 0):
            return [h[0] for h in hit]
        try:
            for net, gn, loss, sk in hit:
                if log:
                    log(f"[WARNING] {net.capitalize()} grad norm invalid: {gn:.6f} at iteration {self.i_so_far}. Check grad_diagnostics.txt"
                        + (f" ({sk} of {cfg.n_updates_per_iteration} steps skipped)" if sk else ""), flush=True)
            if cfg.output_dir:
                adv = getattr(self.updater, "_last_adv", None)
                a = [float("nan")] * 4 if adv is None else [float(x) for x in (adv.mean(), adv.std(), adv.min(), adv.max())]
                os.makedirs(cfg.output_dir, exist_ok=True)
                with open(os.path.join(cfg.output_dir, "grad_diagnostics.txt"), "a") as f:
                    for net, gn, loss, sk in hit:
                        f.write(f"\n[{net.upper()} GRAD ISSUE] Iteration {self.i_so_far}\n")
                        f.write(f"  Net: {net}\n")
                        f.write(f"  {net.capitalize()} grad norm: {gn}\n")
                        f.write(f"  {net.capitalize()} loss: {loss}\n")
                        f.write(f"  Skipped steps: {sk} of {cfg.n_updates_per_iteration}\n")
                        f.write(f"  Advantage stats: mean={a[0]:.4f}, std={a[1]:.4f}, min={a[2]:.4f}, max={a[3]:.4f}\n")
                        f.write(f"  Clip fraction: {stats.get('clip_frac', 0.0):.4f}\n")
        except Exception as e:   # a diagnostics file must never end a run
            try:
                print(f"[WARNING] grad diagnostics not written: {e}", flush=True)
            except Exception:
                pass
        return [h[0] for h in hit]

    # ---- periodic evaluation (PPOConfig.eval_every)
    EVAL_HISTORY_HEADER = ["iteration", "timesteps", "episodes", "success_rate", "collision_rate", "timeout_rate", "mean_length",
                           "mean_return", "mean_path_length"]

    @property
    def stats(self):
        """the last iteration's figures (what iteration() returned)"""
        return self.logger

    def _make_eval_env(self):
        from .env import VecEnv
        w = dict(getattr(self.env, "world_args", None) or {})
        if not w:
            raise ValueError("PPOConfig.eval_every: the training env does not describe its world (VecEnv.world_args)")
        if torch.is_tensor(w["map"]) and w["map"].dim() == 3:
            raise ValueError("PPOConfig.eval_every: a per-env segment tensor cannot be reused for the evaluation envs; pass a map "
                             "name or a shared [S, 4] map (per_env_map=True replicates it)")
        n_par = min(int(self.cfg.eval_episodes), 1024)
        if n_par < 1:
            raise ValueError("PPOConfig.eval_episodes must be at least 1")
        seed = (int(self.cfg.seed) * 1000003 + 7919) & 0xFFFFFFFF   # its own goal / spawn stream, derived from cfg.seed
        return VecEnv(n_par, max_episode_steps=self.cfg.max_episode_steps, auto_reset=True, is_training=False, seed=seed,
                      device=self.device, **w)

    def evaluate_now(self):
        """eval_episodes episodes of the current actor in ONE launch on the evaluation envs (created at the first call): the
        deterministic mean action, arrival threshold 0.4, a fixed quota of whole episodes per env, rows cut slot-major to
        eval_episodes as evaluate() does.  Reads the flat parameter buffer the update writes and nothing of the training env
        (its state, RNG counters, the noise counter and the captured graph are untouched).  Returns the eval_* figures and
        appends one row to <method>_eval_history.csv."""
        cfg = self.cfg
        if not (self.updater.fused_mlp64 or self.updater.fused_resmlp512):
            raise ValueError(f"PPOConfig.eval_every: no evaluation kernel for policy {cfg.policy!r} on this update path "
                             "(it needs the fused HIP update's flat parameter layout)")
        if getattr(self, "_eval_env", None) is None:
            self._eval_env = self._make_eval_env()
        env = self._eval_env
        n_ep = int(cfg.eval_episodes)
        quota = -(-n_ep // env.N)
        t0 = time.time()
        tab = env.evaluate_policy(self.updater.fp.flat, quota, policy="resmlp512" if self.updater.fused_resmlp512 else "mlp64x2")
        cut = lambda x: x.reshape(-1)[:n_ep]
        fl = cut(tab.flags)
        sums = torch.stack([(fl & 1).sum().double(), ((fl >> 1) & 1).sum().double(), ((fl >> 2) & 1).sum().double(),
                            cut(tab.length).double().sum(), cut(tab.ret).double().sum(), cut(tab.path).double().sum(),
                            tab.count.min().double(), tab.steps.max().double()]).cpu().numpy()   # the one host sync
        if int(sums[6]) < quota:
            raise RuntimeError("evaluate_now: an env did not finish its quota of episodes")
        sums = [float(v) for v in sums]
        out = dict(eval_episodes=n_ep, eval_success=sums[0] / n_ep, eval_collision=sums[1] / n_ep, eval_timeout=sums[2] / n_ep,
                   eval_length=sums[3] / n_ep, eval_return=sums[4] / n_ep, eval_path_length=sums[5] / n_ep,
                   eval_steps=int(sums[7]), eval_time=time.time() - t0)
        if cfg.output_dir:
            import csv
            os.makedirs(self.log_dir(), exist_ok=True)
            path = os.path.join(self.log_dir(), f"{cfg.method_name}_eval_history.csv")
            new = not os.path.exists(path)
            with open(path, "a", newline="") as f:
                w = csv.writer(f)
                if new:
                    w.writerow(self.EVAL_HISTORY_HEADER)
                w.writerow([self.i_so_far, self.t_so_far, n_ep, out["eval_success"], out["eval_collision"], out["eval_timeout"],
                            out["eval_length"], out["eval_return"], out["eval_path_length"]])
        return out

    # ---- logging surface of the reference: per-episode CSV (ppo.py:159-163,739-746) and the TensorBoard scalar names
    #      (ppo.py:892-939) written as one JSON object per iteration (tensorboardX is not a dependency here)
    EPISODE_CSV_HEADER = ["episode", "timestep", "success", "collision", "timeout", "length", "return", "path_length", "time"]

    def log_dir(self):
        return os.path.join(self.cfg.output_dir, self.cfg.method_name, "logs")

    def write_episode_csv(self, max_rows=None):
        """Appends the episodes finished in the last rollout, in (step, env) order (ppo.py:739-746).  path_length is the
        simulator's per-episode accumulator (ppo.py:533-537 semantics: the final step's displacement is not part of it);
        time is the episode's share of the rollout wall clock, length x (rollout_time / T): the envs advance in lock
        step, so an episode of L steps occupied L / T of the rollout."""
        import csv
        os.makedirs(self.log_dir(), exist_ok=True)
        path = os.path.join(self.log_dir(), f"{self.cfg.method_name}_train_episodes.csv")
        new = not os.path.exists(path)
        ended = self.ended_buf.bool()
        t_idx, n_idx = torch.nonzero(ended, as_tuple=True)
        if max_rows is not None:
            t_idx, n_idx = t_idx[:max_rows], n_idx[:max_rows]
        d = self.done_buf[t_idx, n_idx].cpu().numpy()
        a = self.arrive_buf[t_idx, n_idx].cpu().numpy()
        ln = self.eplen_buf[t_idx, n_idx].cpu().numpy()
        rt = self.epret_buf[t_idx, n_idx].cpu().numpy()
        pl = self.eppath_buf[t_idx, n_idx].cpu().numpy()
        tt = t_idx.cpu().numpy()
        sec_per_step = float(self.logger.get("rollout_time", 0.0)) / max(self.cfg.rollout_len, 1)
        base = getattr(self, "_episode_count", 0)
        with open(path, "a", newline="") as f:
            w = csv.writer(f)
            if new:
                w.writerow(self.EPISODE_CSV_HEADER)
            for k in range(len(tt)):
                succ = int(a[k]); coll = int(d[k] and not a[k]); tmo = int(not d[k] and not a[k])  # ppo.py:558-560
                w.writerow([base + k, self.env_steps - (self.cfg.rollout_len - int(tt[k]) - 1) * self.env.N, succ, coll, tmo,
                            int(ln[k]), float(rt[k]), float(pl[k]), float(ln[k]) * sec_per_step])
        self._episode_count = base + len(tt)
        return path

    def tb_scalars(self):
        """The scalars the reference hands to SummaryWriter.add_scalar once per iteration, under its tag names
        (ppo.py:892-918), for the last iteration."""
        lg = self.logger
        ep = max(lg.get("episodes", 0), 1)
        n_ep = self.cfg.n_updates_per_iteration
        var = float(lg.get("var", self.cfg.init_var))
        sec_per_step = float(lg.get("rollout_time", 0.0)) / max(self.cfg.rollout_len, 1)
        return {"train/success_rate": lg.get("success_rate"), "train/collision_rate": lg.get("collisions", 0) / ep,
                "train/timeout_rate": lg.get("timeouts", 0) / ep, "train/mean_return": lg.get("avg_ep_rews"),
                "train/mean_ep_length": lg.get("avg_ep_lens"), "train/mean_ep_time": lg.get("avg_ep_lens", 0.0) * sec_per_step,
                "loss/actor": lg.get("actor_loss"), "loss/critic": lg.get("critic_loss"), "train/timesteps": lg.get("t_so_far"),
                "time/rollout": lg.get("rollout_time"), "time/update": lg.get("update_time"), "time/iteration": lg.get("iter_time"),
                "perf/steps_per_sec": lg.get("steps_per_sec"), "perf/actor_grad_steps": n_ep, "perf/critic_grad_steps": n_ep,
                "ppo/approx_kl": lg.get("approx_kl"),
                "ppo/entropy": 1.0 + LOG_2PI + math.log(max(var, 1e-30)),   # MultivariateNormal(mean, var I).entropy(), 2-D
                "ppo/clip_frac": lg.get("clip_frac"), "ppo/actor_grad_norm": lg.get("actor_grad_norm"),
                "ppo/critic_grad_norm": lg.get("critic_grad_norm"), "ppo/actor_param_delta": lg.get("actor_param_delta"),
                "ppo/critic_param_delta": lg.get("critic_param_delta"),
                "ppo/grad_clip_frac_actor": lg.get("grad_clip_frac_actor"), "ppo/grad_clip_frac_critic": lg.get("grad_clip_frac_critic"),
                "ppo/skipped_steps_actor": lg.get("skipped_steps_actor"), "ppo/skipped_steps_critic": lg.get("skipped_steps_critic"),
                "ppo/kl_stop_epoch": lg.get("kl_stop_epoch"), "ppo/kl_stopped": lg.get("kl_stopped"),   # (target_kl set)
                **({"ppo/kl_stop_step": lg["kl_stop_step"]} if "kl_stop_step" in lg else {}),           # (target_kl and minibatches)
                **({"ppo/" + k: lg[k] for k in ("lr", "lr_ups", "lr_downs") if k in lg}),               # (lr_schedule set)
                **({"ppo/" + k: lg[k] for k in ("reward_scale", "ret_rms_mean", "ret_rms_std", "explained_variance")}
                   if "reward_scale" in lg else {}),                                                    # (norm_reward)
                **({"ppo/bootstrapped_frac": lg["bootstrapped_frac"]} if "bootstrapped_frac" in lg else {}),   # (bootstrap_truncated)
                **({"eval/success_rate": lg["eval_success"], "eval/collision_rate": lg["eval_collision"],
                    "eval/timeout_rate": lg["eval_timeout"], "eval/mean_return": lg["eval_return"],
                    "eval/mean_ep_length": lg["eval_length"], "time/eval": lg["eval_time"]} if "eval_success" in lg else {})}

    def tb_dir(self):
        return os.path.join(self.cfg.output_dir, self.cfg.method_name, "tb")   # ppo.py:66

    def write_tensorboard(self):
        """The reference's TensorBoard stream (ppo.py:892-939): per-iteration scalars at step i_so_far, the per-epoch
        Actor_loss/train and Critic_loss/train series, Episode_Rewards/train (return / length of every finished episode,
        ppo.py:586, capped per iteration like the CSV) and avg_ep_rews/train."""
        from .tb_writer import SummaryWriter
        if getattr(self, "_tb", None) is None:
            self._tb = SummaryWriter(self.tb_dir())
            self._tb_loss_steps = self._tb_ep_steps = 0
        w, it = self._tb, self.i_so_far
        t0 = time.time()
        recs = [(k, float(v), it) for k, v in self.tb_scalars().items() if v is not None]
        hist = self.updater.loss_history.detach().cpu().numpy()
        hist = hist[:int(self.updater.stats.get("kl_stop_epoch", hist.shape[0])) + int(self.updater.stats.get("kl_stopped", 0))]   # (rows of epochs that ran)
        for k in range(hist.shape[0]):
            recs.append(("Actor_loss/train", float(hist[k, 0]), self._tb_loss_steps + k))
            recs.append(("Critic_loss/train", float(hist[k, 1]), self._tb_loss_steps + k))
        self._tb_loss_steps += hist.shape[0]
        cap = int(self.cfg.tb_episode_rows or 0)
        if cap:   # own cap, independent of the CSV's: with 4096 envs an iteration finishes ~1e5 episodes
            ended = self.ended_buf.bool()
            t_idx, n_idx = torch.nonzero(ended, as_tuple=True)
            t_idx, n_idx = t_idx[:cap], n_idx[:cap]
            per_step = (self.epret_buf[t_idx, n_idx] / self.eplen_buf[t_idx, n_idx].clamp(min=1)).cpu().numpy()
            recs.extend(("Episode_Rewards/train", float(r), self._tb_ep_steps + k) for k, r in enumerate(per_step))
            self._tb_ep_steps += len(per_step)
        recs.append(("avg_ep_rews/train", float(self.logger.get("avg_ep_rews", 0.0)), it))
        recs.append(("time/log", float(getattr(self, "_last_log_time", 0.0)), it))   # the previous iteration's logging cost
        w.add_scalars(recs)   # one TFRecord per point; CRCs vectorised over the records (tb_writer._masked_crc_many)
        w.flush()
        self._last_log_time = time.time() - t0

    def learn(self, total_timesteps, log=print):
        # The reference counts only COMPLETED episodes toward the budget (ppo.py:258); if a configuration never completes
        # one (rollout shorter than the episode cap) its loop would spin forever -- bound the iterations by the budget in
        # simulated steps instead of hanging.
        world = self.ctx.world if self.ctx is not None else 1
        per_iter = self.cfg.rollout_len * self.env.N * world
        max_iters = 4 * (-(-int(total_timesteps) // per_iter)) + 4
        while self.t_so_far < total_timesteps and self.i_so_far < max_iters:  # ppo.py:245
            if self.cfg.lr_schedule == "linear":
                self.updater.set_lr(linear_lr(self.cfg.lr, self.t_so_far, total_timesteps))
            lg = self.iteration()
            if log and (self.ctx is None or self.ctx.rank == 0):
                log(f"[iter {lg['iteration']:4d}] t={lg['t_so_far']:>10d} mean_ep_rew={lg['avg_ep_rews']:8.2f} "
                    f"succ={lg['success_rate']:.3f} ep_len={lg['avg_ep_lens']:6.1f} a_loss={lg['actor_loss']:.4f} "
                    f"c_loss={lg['critic_loss']:.2f} kl={lg['approx_kl']:.4f} steps/s={lg['steps_per_sec']:.0f} "
                    f"(rollout {lg['rollout_time']:.3f}s update {lg['update_time']:.3f}s)"
                    + (f" kl_stop_epoch={lg['kl_stop_epoch']} kl_stopped={lg['kl_stopped']}" if "kl_stop_epoch" in lg else "")
                    + (f" kl_stop_step={lg['kl_stop_step']}" if "kl_stop_step" in lg else "")
                    + (f" lr={lg['lr']:.3e}" if "lr" in lg else "")
                    + (f" lr_ups={lg['lr_ups']} lr_downs={lg['lr_downs']}" if "lr_ups" in lg else "")
                    + (f" bootstrapped_frac={lg['bootstrapped_frac']:.4f}" if "bootstrapped_frac" in lg else "")
                    + (f" eval: succ={lg['eval_success']:.3f} coll={lg['eval_collision']:.3f} tmo={lg['eval_timeout']:.3f} "
                       f"ret={lg['eval_return']:.2f} len={lg['eval_length']:.1f} ({lg['eval_time']:.3f}s)"
                       if "eval_success" in lg else ""))
        return self.logger

    # ---- ppo.py:452-457 file naming; state_dict keys match the reference's nets for policy resmlp512
    def checkpoint_dir(self):
        return os.path.join(self.cfg.output_dir, self.cfg.method_name, "checkpoints")

    def save_checkpoint(self):
        d = self.checkpoint_dir()
        os.makedirs(d, exist_ok=True)
        tag = f"iter{self.i_so_far:04d}_step{self.t_so_far:08d}.pth"
        pa, pc = os.path.join(d, "actor_" + tag), os.path.join(d, "critic_" + tag)
        torch.save({k: v.detach().cpu().clone() for k, v in self.actor.state_dict().items()}, pa)
        torch.save({k: v.detach().cpu().clone() for k, v in self.critic.state_dict().items()}, pc)
        if self.cfg.norm_reward:   # a third file beside the two reference-named ones: the critic's units
            mean, var, count = self.ret_rms[:3].tolist()
            torch.save({"mean": mean, "var": var, "count": count}, os.path.join(d, "retnorm_" + tag))
        if self.cfg.lr_schedule == "adaptive":   # the rate the next step starts from (on the host since the last update's read-back)
            torch.save({"lr": float(self.updater.lr_value)}, os.path.join(d, "lrsched_" + tag))
        return pa, pc

    @staticmethod
    def retnorm_path(actor_path):
        """retnorm_<tag>.pth beside actor_<tag>.pth"""
        d, base = os.path.split(actor_path)
        return os.path.join(d, "retnorm_" + (base[len("actor_"):] if base.startswith("actor_") else base))

    @staticmethod
    def lrsched_path(actor_path):
        """lrsched_<tag>.pth beside actor_<tag>.pth"""
        d, base = os.path.split(actor_path)
        return os.path.join(d, "lrsched_" + (base[len("actor_"):] if base.startswith("actor_") else base))

    def load_checkpoint(self, actor_path, critic_path):
        """main.py:52-89: state_dicts only (optimiser state and covariance are not part of a checkpoint).  With norm_reward the return
        statistics come from retnorm_<tag>.pth beside the actor's file; without that file: one warning line and fresh statistics.
        With lr_schedule="adaptive" the learning rate comes from lrsched_<tag>.pth; without that file: one warning line and cfg.lr."""
        if self.cfg.lr_schedule == "adaptive":
            pl = self.lrsched_path(actor_path)
            if os.path.exists(pl):
                self.updater.set_lr(float(torch.load(pl, map_location="cpu")["lr"]))
            else:
                import warnings
                warnings.warn(f"lr_schedule='adaptive': {pl} not found -- the learning rate starts at lr = {self.cfg.lr}")
                self.updater.set_lr(float(self.cfg.lr))
        if self.cfg.norm_reward:
            pr = self.retnorm_path(actor_path)
            if os.path.exists(pr):
                s = torch.load(pr, map_location="cpu")
                self._init_ret_rms(self.ret_rms.device, s["mean"], s["var"], s["count"])
            else:
                import warnings
                warnings.warn(f"norm_reward: {pr} not found -- the return statistics start fresh; the critic's units are off until they settle")
                self._init_ret_rms(self.ret_rms.device)
        sa = torch.load(actor_path, map_location="cpu")
        sc = torch.load(critic_path, map_location="cpu")
        with torch.no_grad():
            for mod, sd in ((self.actor, sa), (self.critic, sc)):
                own = mod.state_dict()
                missing = set(own) - set(sd)
                if missing:
                    raise KeyError(f"checkpoint lacks keys {sorted(missing)}")
                for k, v in own.items():
                    v.copy_(sd[k])  # in place: parameters stay views of the flat buffer
