// navppo_internal.h -- shared by the translation units of libnavsim.so that implement include/navppo.h (not installed)
#pragma once

// stores the message navppo_last_error() returns (thread-local, defined in ppo_mlp64.hip)
void navppo_set_error(const char* msg);

// torch.optim.Adam's step (ppo.py:116-117,381,392: no weight decay, no amsgrad) on parameter q with gradient gr: exp_avg.lerp_(grad,
// 1 - beta1), exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2), then the bias-corrected update.  ONE expression for every kernel
// that steps (reduce_adam<true>, resmlp_reduce<true>, adam_step_kernel, clip_adam_kernel): under -ffp-contract=off they give the same bits.
__device__ __forceinline__ void navppo_adam_apply(float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, int q, float gr,
                                                  float lr, float beta1, float beta2, float eps, float bc1, float bc2_sqrt) {
    const float mm = m[q] + (gr - m[q]) * (1.0f - beta1);
    const float vv = beta2 * v[q] + (1.0f - beta2) * (gr * gr);
    m[q] = mm;
    v[q] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    params[q] -= (lr / bc1) * (mm / denom);
}

// max_norm of the *_clipped entry points: a positive number, +inf included
inline bool navppo_max_norm_ok(float max_norm) { return max_norm > 0.f; }

// The second launch of a clipped epoch (clip_adam_kernel, ppo_mlp64.hip): per net (actor = [0, n_first), critic = [n_first, n)) the
// squared norm s = sum of the net's `n_slots` squared-norm slots -- slot i of net k at slots[(j >> 3) * slot_pitch + (j & 7)],
// j = k * slot_stride + i (slot_pitch 8: contiguous) -- added in ONE fixed order by every block; s not finite: the net is left alone,
// coefficient 0; else coef = min(1, max_norm / (sqrt(s) + 1e-6)), grad = grad * grad_scale * coef, Adam on that.
// clip_stats[0..3] = s_actor, s_critic, coef_actor, coef_critic.  `stream` is a hipStream_t.
void navppo_launch_clip_adam(float* params, float* grad, float* m, float* v, int n, int n_first, float grad_scale, float max_norm, float lr,
                             float beta1, float beta2, float eps, int step, const float* slots, int n_slots, int slot_stride, int slot_pitch,
                             float* clip_stats, void* stream);
