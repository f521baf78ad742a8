"""The learning-rate schedules of PPOConfig.lr_schedule on the host: the mirror of the adaptive rule the step launch of
navppo_*_update_epoch_lr / navppo_adam_step_lr applies on the device, and the linear decay."""
LR_FACTOR = 1.5   # the rule's step (rsl_rl, rl_games); not configurable


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
