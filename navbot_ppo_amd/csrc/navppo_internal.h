// navppo_internal.h -- shared by the translation units of libnavsim.so that implement include/navppo.h (not installed)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

// stores the message navppo_last_error() returns (thread-local, defined in ppo_mlp64.hip)
void navppo_set_error(const char* msg);

// ---------------------------------------------------------------- what the entry points' host code shares
// an argument check failed (before any launch): "<entry point>: <what>" for navppo_last_error(), the return code -1
inline int navppo_bad_args(const char* who, const char* what) {
    navppo_set_error((std::string(who) + ": " + what).c_str());
    return -1;
}

// behind the last launch of an entry point: 0, or "<entry point>: <HIP's message>" and -2
inline int navppo_launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    navppo_set_error((std::string(who) + ": " + hipGetErrorString(e)).c_str());
    return -2;
}

// How an epoch (or navppo_adam_step*) ends -- the five step modes of include/navppo.h:
enum class NavppoMode {
    kGrad,     // *_loss_grad[_net]: the reduction alone, nothing is stepped
    kAdam,     // *_update_epoch, navppo_adam_step: Adam inside the reduction (or alone)
    kClip,     // *_clipped: the reduction with its squared-norm slots, then one launch that clips and steps (navppo_launch_clip_adam)
    kClipKl,   // *_kl: the gated twins of those launches, the KL decision in front of the clip (below)
    kClipLr,   // *_lr: kClip's (ungated) launches, the step launch derives its learning rate from the KL and lr_state (clip_adam_lr_kernel)
};

// the batch of an epoch: actions, old log-probabilities, rewards-to-go and advantages of n samples; the policy's variance, PPO's clip
struct NavppoBatch {
    const float *act, *logp_old, *rtg, *adv;
    int64_t n;
    float var, clip;
    bool ok() const { return act && logp_old && rtg && adv && n >= 1 && var > 0.f; }   // (a NaN variance fails)
};

// the optimiser's half of an entry point's arguments; a mode reads the members it needs (kGrad: none)
struct NavppoStep {
    float lr, beta1, beta2, eps;
    int32_t step;                        // Adam's step count, >= 1
    float *m, *v;                        // exp_avg, exp_avg_sq
    float max_norm; float* clip_stats;   // kClip, kClipKl
    float kl_limit; float* kl_state;     // kClipKl
    float kl_target, lr_min, lr_max;     // kClipLr: the desired KL and the clamps of the learning rate
    int32_t adapt; float* lr_state;      // kClipLr: 0 = keep the rate, 1 = apply the rule; [4] (two rate slots, raises, lowerings)
    float* var_state;                    // the *_var entry points (kClip / kClipLr of their translation units): [8], see NavppoVar
};

// the *_var entry points' own arguments (include/navppo.h "Learned exploration variance"): the entropy coefficient, the clamps of the
// variance and the state -- (theta, var, m, v, gradient, steps taken, steps skipped, entropy)
struct NavppoVar {
    float ent_coef, var_min, var_max;
    float* state;
    bool ok() const {   // (a NaN fails each comparison)
        return ent_coef >= 0.f && std::isfinite(ent_coef) && var_min > 0.f && var_max >= var_min && std::isfinite(var_max) && state &&
               ((uintptr_t)state & 15) == 0;
    }
};
inline int navppo_check_var(const char* who, const NavppoVar& v) {
    return v.ok() ? 0
                  : navppo_bad_args(who, "ent_coef >= 0 and finite, 0 < var_min <= var_max, both finite, and var_state_dev [8] not null, "
                                         "16-byte aligned");
}

// max_norm of the *_clipped entry points, kl_limit of the *_kl entry points: a positive number, +inf included (NaN fails)
inline bool navppo_max_norm_ok(float max_norm) { return max_norm > 0.f; }
inline bool navppo_kl_limit_ok(float kl_limit) { return kl_limit > 0.f; }
// the *_lr entry points' own arguments: kl_target > 0, 0 < lr_min <= lr_max (a NaN fails each), adapt 0 or 1, the state
inline bool navppo_lr_args_ok(const NavppoStep& s) {
    return s.kl_target > 0.f && s.lr_min > 0.f && s.lr_max >= s.lr_min && (s.adapt == 0 || s.adapt == 1) && s.lr_state;
}

// the step arguments of `mode`; 0, or the message and -1
inline int navppo_check_step(const char* who, NavppoMode mode, const NavppoStep& s) {
    if (mode == NavppoMode::kGrad) return 0;
    if (!s.m || !s.v || s.step < 1) return navppo_bad_args(who, "bad argument (adam_m_dev, adam_v_dev not null, step >= 1)");
    if (mode == NavppoMode::kAdam) return 0;
    if (!navppo_max_norm_ok(s.max_norm) || !s.clip_stats)
        return navppo_bad_args(who, "max_norm must be > 0 (+inf allowed) and clip_stats_dev [4] not null");
    if (mode == NavppoMode::kClipKl && (!navppo_kl_limit_ok(s.kl_limit) || !s.kl_state))
        return navppo_bad_args(who, "kl_limit must be > 0 (+inf allowed) and kl_state_dev [4] not null");
    if (mode == NavppoMode::kClipLr && !navppo_lr_args_ok(s))
        return navppo_bad_args(who, "kl_target > 0, 0 < lr_min <= lr_max, adapt 0 or 1 and lr_state_dev [4] not null");
    return 0;
}

// Adam's bias corrections at step count `step`: 1 - beta1^step and sqrt(1 - beta2^step), in double, rounded once
struct NavppoBias {
    float bc1, bc2_sqrt;
};
inline NavppoBias navppo_bias(float beta1, float beta2, int step) {
    return {(float)(1.0 - std::pow((double)beta1, (double)step)), (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step))};
}

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

// The second launch of a clipped epoch (clip_adam_kernel, ppo_mlp64.hip): per net (actor = [0, n_first), critic = [n_first, n)) the
// squared norm s = sum of the net's `n_slots` squared-norm slots -- slot i of net k at slots[(j >> 3) * slot_pitch + (j & 7)],
// j = k * slot_stride + i (slot_pitch 8: contiguous) -- added in ONE fixed order by every block; s not finite: the net is left alone,
// coefficient 0; else coef = min(1, max_norm / (sqrt(s) + 1e-6)), grad = grad * grad_scale * coef, Adam on that.
// clip_stats[0..3] = s_actor, s_critic, coef_actor, coef_critic.  `stream` is a hipStream_t.
// kl != nullptr (the *_kl entry points, include/navppo.h "Early stop at a KL limit"): clip_adam_kl_kernel instead -- returns at
// its entry when kl_state[0] != 0; trips when !(*kl <= kl_limit): no net is stepped, clip_stats = (s_actor, s_critic, 0, 0), block 0
// sets kl_state = (1, unchanged, *kl, step); else the step above, the same expression, and kl_state[1] += 1.  `kl` is a device scalar
// an EARLIER launch wrote (stats_dev[1]): every block derives the same decision from the same bits, no block waits for another.
// adaptive_lr (the *_lr entry points, include/navppo.h "Adaptive learning rate"; kl as above, never null): clip_adam_lr_kernel instead
// -- no gate, no trip: every block reads the rate slot lr_state[step & 1] (0 = not started: s.lr) and *kl, derives the step's rate by
// the rule, and steps as above with it; block 0 writes the rate to slot (step + 1) & 1 -- which no block of THIS launch reads -- and
// counts the raise or the lowering.
// `s`: max_norm, Adam's arguments, clip_stats; kl != nullptr: s.kl_limit and s.kl_state, or (adaptive_lr) s.kl_target .. s.lr_state.
void navppo_launch_clip_adam(float* params, float* grad, int n, int n_first, float grad_scale, const NavppoStep& s, const float* slots,
                             int n_slots, int slot_stride, int slot_pitch, void* stream, const float* kl = nullptr, bool adaptive_lr = false);

// The gate of the *_kl kernels: one uniform read of kl_state[0] at kernel entry.  The flag is only ever written by the LAST launch of an
// earlier epoch (clip_adam_kl_kernel), so every workgroup of a launch reads the same value; none of the gated kernels synchronises
// across workgroups, so a launch that returns here leaves nobody waiting.
__device__ __forceinline__ bool navppo_kl_stopped(const float* __restrict__ kl_state) { return kl_state[0] != 0.f; }

// The gated twins of the update's kernels are the SAME text compiled a second time: ppo_mlp64_kl.hip / ppo_resmlp512_kl.hip include
// ppo_mlp64.hip / ppo_resmlp512.hip with NAVPPO_KL_TU defined, and every kernel written with the first three macros below is then
// `name_kl`, takes kl_state as one more (last) argument and starts with the gate.  The host code that launches them is compiled a
// second time as well: the epoch function of each family (mlp64_epoch, loss_grad_impl) is ONE launch sequence, a template over
// NavppoMode that launches NAVPPO_KL_KERNEL(name) with NAVPPO_KL_ARG(kl_state) behind the last argument -- so a grid or an argument
// cannot change for the clipped epoch and not for the gated one.  A translation unit instantiates the modes it exports
// (kNavppoKlTu: kClipKl there, the other four here), hence only their kernels; the rest of the included file's host code --
// the entry points, the kernels that have no twin -- is compiled out of the twins' unit.
// Without NAVPPO_KL_TU the macros vanish: the ungated kernels are textually what they were, in a translation unit of their own.
// (Twins in the SAME translation unit changed the ungated kernels' listings: a helper that is not force-inlined then has two callers
// and the inliner decides differently -- mlp64_pass_both_x3s went from 491 to 486 registers, mlp64_pass_both_x3<16> from 268 to 192
// bytes of scratch -- and a hand-placed stream's listing is exactly what tests/test_isa_*.py pin: profiles/kl_gate_resources.txt.)
//
// A THIRD compilation of the same text gives the twins of the *_var entry points (ppo_mlp64_var.hip / ppo_resmlp512_var.hip define
// NAVPPO_VAR_TU, and NAVPPO_KL_TU with it so that the same code is compiled out): every kernel is then `name_var` and takes var_state
// as its last argument; there is no gate; the kernels that hold a loss block start with NAVPPO_VAR_READ(var) -- var = var_state[1], the
// by-value argument is ignored -- and, under `if constexpr (kNavppoVarTu)`, add the per-sample term of d/d(log var) into one more
// per-lane sum that leaves through the workgroup's statistics row (column 3).  The modes of those units are kClip and kClipLr.
#if defined(NAVPPO_VAR_TU)
#ifndef NAVPPO_KL_TU
#error "NAVPPO_VAR_TU is defined together with NAVPPO_KL_TU (the twins' translation units compile the same code out)"
#endif
constexpr bool kNavppoKlTu = false, kNavppoVarTu = true;
#define NAVPPO_KL_KERNEL(name) name##_var
#define NAVPPO_KL_PARAM , const float* __restrict__ var_state
#define NAVPPO_KL_ARG(var_state) , (const float*)(var_state)
#define NAVPPO_KL_GATE() \
    do {                 \
    } while (0)
#define NAVPPO_VAR_READ(var) \
    do {                     \
        var = var_state[1];  \
    } while (0)
#elif defined(NAVPPO_KL_TU)
constexpr bool kNavppoKlTu = true, kNavppoVarTu = false;
#define NAVPPO_KL_KERNEL(name) name##_kl
#define NAVPPO_KL_PARAM , const float* __restrict__ kl_state
#define NAVPPO_KL_ARG(kl_state) , (const float*)(kl_state)
#define NAVPPO_KL_GATE() \
    do {                 \
        if (navppo_kl_stopped(kl_state)) return; \
    } while (0)
#define NAVPPO_VAR_READ(var) \
    do {                     \
    } while (0)
#else
constexpr bool kNavppoKlTu = false, kNavppoVarTu = false;
#define NAVPPO_KL_KERNEL(name) name
#define NAVPPO_KL_PARAM
#define NAVPPO_KL_ARG(kl_state)
#define NAVPPO_KL_GATE() \
    do {                 \
    } while (0)
#define NAVPPO_VAR_READ(var) \
    do {                     \
    } while (0)
#endif

// the state pointer the twins' launches pass behind the last argument: kl_state (the gated twins) or var_state (the *_var twins)
inline const float* navppo_twin_state(const NavppoStep& s) { return kNavppoVarTu ? s.var_state : s.kl_state; }

// the per-sample term of d(actor loss)/d(log var), the log-probability being -1/2 (d0^2 + d1^2) / var - log 2 pi - log var:
// dL_dlp (1/2 (d0^2 + d1^2) / var - 1), the quotient written as the loss blocks write it
__device__ __forceinline__ float navppo_dlogvar_term(float dL_dlp, float d0, float d1, float var) {
    return dL_dlp * (0.5f * ((d0 * d0 + d1 * d1) / var) - 1.0f);
}

// The launch behind a *_var epoch's step launch (var_step_kernel, ppo_learned_var.hip): ONE workgroup adds column 0 of `n_rows` rows of
// pitch `row_pitch` at `col` (the workgroups' sums of the term above) in one fixed order, writes the sum to *sum_out, and steps
// log var with Adam (include/navppo.h has the rule).  lr_state: NULL, or the *_lr state whose slot (step + 1) & 1 the step launch wrote.
void navppo_launch_var_step(const float* col, int n_rows, int row_pitch, const NavppoStep& s, const NavppoVar& v, float* sum_out,
                            void* stream);
