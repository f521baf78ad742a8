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
// kl_state != nullptr (the *_kl entry points, include/navppo.h "Early stop at a KL limit"): clip_adam_kl_kernel instead -- returns at
// its entry when kl_state[0] != 0; trips when !(*kl <= kl_limit): no net is stepped, clip_stats = (s_actor, s_critic, 0, 0), block 0
// sets kl_state = (1, unchanged, *kl, step); else the step above, the same expression, and kl_state[1] += 1.  `kl` is a device scalar
// an EARLIER launch wrote (stats_dev[1]): every block derives the same decision from the same bits, no block waits for another.
void navppo_launch_clip_adam(float* params, float* grad, float* m, float* v, int n, int n_first, float grad_scale, float max_norm, float lr,
                             float beta1, float beta2, float eps, int step, const float* slots, int n_slots, int slot_stride, int slot_pitch,
                             float* clip_stats, void* stream, const float* kl = nullptr, float kl_limit = 0.f, float* kl_state = nullptr);

// kl_limit of the *_kl entry points: a positive number, +inf included (NaN fails)
inline bool navppo_kl_limit_ok(float kl_limit) { return kl_limit > 0.f; }

// The gate of the *_kl kernels: one uniform read of kl_state[0] at kernel entry.  The flag is only ever written by the LAST launch of an
// earlier epoch (clip_adam_kl_kernel), so every workgroup of a launch reads the same value; none of the gated kernels synchronises
// across workgroups, so a launch that returns here leaves nobody waiting.
__device__ __forceinline__ bool navppo_kl_stopped(const float* __restrict__ kl_state) { return kl_state[0] != 0.f; }

// The gated twins of the update's kernels are the SAME text compiled a second time: ppo_mlp64_kl.hip / ppo_resmlp512_kl.hip include
// ppo_mlp64.hip / ppo_resmlp512.hip with NAVPPO_KL_TU defined, and every kernel written with the three macros below is then
// `name_kl`, takes kl_state as one more (last) argument and starts with the gate; the host code of the included file is compiled out.
// Without NAVPPO_KL_TU the macros vanish: the ungated kernels are textually what they were, in a translation unit of their own.
// (Twins in the SAME translation unit changed the ungated kernels' listings: a helper that is not force-inlined then has two callers
// and the inliner decides differently -- mlp64_pass_both_x3s went from 491 to 486 registers, mlp64_pass_both_x3<16> from 268 to 192
// bytes of scratch -- and a hand-placed stream's listing is exactly what tests/test_isa_*.py pin: profiles/kl_gate_resources.txt.)
#ifdef NAVPPO_KL_TU
#define NAVPPO_KL_KERNEL(name) name##_kl
#define NAVPPO_KL_PARAM , const float* __restrict__ kl_state
#define NAVPPO_KL_GATE() \
    do {                 \
        if (navppo_kl_stopped(kl_state)) return; \
    } while (0)
#else
#define NAVPPO_KL_KERNEL(name) name
#define NAVPPO_KL_PARAM
#define NAVPPO_KL_GATE() \
    do {                 \
    } while (0)
#endif
