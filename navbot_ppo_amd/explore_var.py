"""The learned exploration variance of PPOConfig.learn_var on the host: the state the navppo_*_update_epoch_var entry points keep on the
device (include/navppo.h, "Learned exploration variance"), and the mirror of the step their last launch takes on it."""
import math

VAR_STATE_LEN = 8
# the slots of the state: theta = log var, var, Adam's m and v, the gradient of the last step taken (after the actor's clip coefficient),
# steps taken, steps skipped, the entropy after the last step taken
THETA, VAR, ADAM_M, ADAM_V, GRAD, STEPS, SKIPPED, ENTROPY = range(VAR_STATE_LEN)
ENTROPY_AT_ZERO = 2.8378770664093453   # 1 + log 2 pi: the entropy of the 2-D policy at theta = 0, the constant of var_step_kernel


def var_state_init(var0):
    """[8] the state a caller starts from: (log v0, v0, 0, ...) in float32, the logarithm taken in double and rounded once"""
    import numpy as np
    v0 = np.float32(var0)
    return [float(np.float32(math.log(float(v0)))), float(v0), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def learned_var_reference(state, grad_sum, coef, ent_coef, lr, betas, eps, step, var_min, var_max):
    """Host mirror of var_step_kernel (csrc/ppo_learned_var.hip): float32 arithmetic in the kernel's order of operations, bit for bit
    but for var = exp(theta), which is libm's here and the device's there.  state: [8]; grad_sum: the float32 sum over the samples of
    dL_dlp (1/2 (d0^2 + d1^2) / var - 1) (stats_dev[3] of the call); coef: the actor's clip coefficient of the step (clip_stats[2]);
    lr: the rate the nets stepped with; step: Adam's step count of the call.  Returns the new state as a list of Python floats holding
    float32 values."""
    import numpy as np
    f = np.float32
    s = [f(x) for x in state]
    beta1, beta2 = f(betas[0]), f(betas[1])
    with np.errstate(all="ignore"):
        g = (f(grad_sum) - f(ent_coef)) * f(coef)
        if f(coef) == f(0.0) or not np.isfinite(g):   # the actor's step was skipped, or theta's own gradient is not finite
            s[SKIPPED] = s[SKIPPED] + f(1.0)
            return [float(x) for x in s]
        # Adam's bias corrections: in double, rounded once (navppo_bias)
        bc1 = f(1.0 - float(beta1) ** int(step))
        bc2_sqrt = f(math.sqrt(1.0 - float(beta2) ** int(step)))
        mm = s[ADAM_M] + (g - s[ADAM_M]) * (f(1.0) - beta1)
        vv = beta2 * s[ADAM_V] + (f(1.0) - beta2) * (g * g)
        denom = np.sqrt(vv) / bc2_sqrt + f(eps)
        theta = s[THETA] - (f(lr) / bc1) * (mm / denom)
        lo, hi = f(math.log(float(f(var_min)))), f(math.log(float(f(var_max))))
        theta = min(max(theta, lo), hi)
        s[THETA], s[VAR], s[ADAM_M], s[ADAM_V], s[GRAD] = theta, f(math.exp(float(theta))), mm, vv, g
        s[STEPS] = s[STEPS] + f(1.0)
        s[ENTROPY] = f(ENTROPY_AT_ZERO) + theta
    return [float(x) for x in s]
