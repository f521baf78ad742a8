// ppo_mlp64_kl.hip -- navppo_mlp64_update_epoch_kl and navppo_mlp64_bf16x3_update_epoch_kl: the clipped epochs of ppo_mlp64.hip with
// an early stop at a KL limit (include/navppo.h "Early stop at a KL limit").
//
// The kernels are ppo_mlp64.hip's own text compiled a second time as their gated twins (navppo_internal.h, NAVPPO_KL_TU):
// mlp64_pass_both_kl<IN, F16>, mlp64_pass_both_x3_kl<IN>, mlp64_pass_both_x3s_kl (the hand-placed stream; tests/test_target_kl_cpu.py
// lints its listing like the original's) and reduce_adam_kl<false> -- one uniform read of kl_state[0] at entry and a branch to the end,
// then the same body.  The step launch (clip_adam_kl_kernel, ppo_mlp64.hip) takes the decision.
#define NAVPPO_KL_TU 1
#include "ppo_mlp64.hip"

namespace {

bool kl_args_ok(const std::string& who, float max_norm, const float* clip_stats_dev, float kl_limit, const float* kl_state_dev) {
    if (!navppo_max_norm_ok(max_norm) || !clip_stats_dev) {
        navppo_set_error((who + ": max_norm must be > 0 (+inf allowed) and clip_stats_dev [4] not null").c_str());
        return false;
    }
    if (!navppo_kl_limit_ok(kl_limit) || !kl_state_dev) {
        navppo_set_error((who + ": kl_limit must be > 0 (+inf allowed) and kl_state_dev [4] not null").c_str());
        return false;
    }
    return true;
}

// the reduction alone (squared-norm slots in parity 0), then the norms, the KL decision, the clip and Adam -- as the clipped epochs
int reduce_and_step(const std::string& who, const PassPlan& pl, float* params_dev, float* adam_m_dev, float* adam_v_dev, float* grad_dev,
                    float* stats_dev, float lr, float beta1, float beta2, float eps, int32_t step, float max_norm, float* clip_stats_dev,
                    float kl_limit, float* kl_state_dev, void* stream) {
    const int rblocks = (pl.pa + pl.pc + 63) / 64;
    hipLaunchKernelGGL(reduce_adam_kl<false>, dim3(rblocks), dim3(64 * kRedGroups), 0, (hipStream_t)stream, pl.partial, pl.stats_partial, pl.partial_c,
                       pl.stats_partial_c, pl.blocks, pl.inv_n, grad_dev, stats_dev, nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f,
                       pl.pa, pl.pc, 0, pl.pa + pl.pc, pl.gn, 0, (const float*)kl_state_dev);
    navppo_launch_clip_adam(params_dev, grad_dev, adam_m_dev, adam_v_dev, pl.pa + pl.pc, pl.pa, 1.0f, max_norm, lr, beta1, beta2, eps, step, pl.gn,
                            rblocks, kGnSlots, 8, clip_stats_dev, stream, stats_dev + 1, kl_limit, kl_state_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        navppo_set_error((who + ": " + hipGetErrorString(e)).c_str());
        return -2;
    }
    return 0;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int navppo_mlp64_update_epoch_kl(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                                 const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                 float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                 float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                 float* clip_stats_dev, float kl_limit, float* kl_state_dev, void* stream) {
    const std::string who = "navppo_mlp64_update_epoch_kl";
    if (!kl_args_ok(who, max_norm, clip_stats_dev, kl_limit, kl_state_dev)) return -1;
    if (!params_dev || !obs_dev || !act_dev || !logp_old_dev || !rtg_dev || !adv_dev || !grad_dev || !stats_dev ||
        !workspace_dev || !adam_m_dev || !adam_v_dev || n_samples < 1 || !(var > 0.f) || step < 1 || (obs_dim != 16 && obs_dim != 42)) {
        navppo_set_error((who + ": bad argument (obs_dim is 16 or 42)").c_str());
        return -1;
    }
    if (!obs_aligned(obs_dev, obs_dim, obs_f16) || ((uintptr_t)act_dev & 7)) {
        navppo_set_error((who + ": obs must be 16-byte (42 columns: 8-byte, float16: 4-byte) and act 8-byte aligned").c_str());
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const PassPlan pl = plan_pass(workspace_dev, n_samples, obs_dim);
    const float* const params = params_dev;
    const float* const kls = kl_state_dev;
    for_obs(obs_dim, obs_f16, [&](auto in, auto f16) {
        hipLaunchKernelGGL((mlp64_pass_both_kl<decltype(in)::value, decltype(f16)::value>), dim3(pl.blocks), dim3(64 * Pad<decltype(in)::value>::NW), 0, st,
                           params, obs_dev, act_dev, logp_old_dev, rtg_dev, adv_dev, (long long)n_samples, var, clip, pl.inv_n, pl.partial,
                           pl.stats_partial, pl.partial_c, pl.stats_partial_c, grad_dev, stats_dev, kls);
    });
    return reduce_and_step(who, pl, params_dev, adam_m_dev, adam_v_dev, grad_dev, stats_dev, lr, beta1, beta2, eps, step, max_norm, clip_stats_dev,
                           kl_limit, kl_state_dev, stream);
}

int navppo_mlp64_bf16x3_update_epoch_kl(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                        const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                        float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                        float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                        float* clip_stats_dev, float kl_limit, float* kl_state_dev, void* stream) {
    const std::string who = "navppo_mlp64_bf16x3_update_epoch_kl";
    if (!kl_args_ok(who, max_norm, clip_stats_dev, kl_limit, kl_state_dev)) return -1;
    if (!params_dev || !prep_dev || !act_dev || !logp_old_dev || !rtg_dev || !adv_dev || !grad_dev || !stats_dev || !workspace_dev ||
        !adam_m_dev || !adam_v_dev || step < 1 || n_samples < 1 || !(var > 0.f) || (obs_dim != 16 && obs_dim != 42) ||
        ((uintptr_t)prep_dev & 15) || ((uintptr_t)act_dev & 7)) {
        navppo_set_error((who + ": bad argument (obs_dim is 16 or 42; prep 16-byte, act 8-byte aligned)").c_str());
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const PassPlan pl = plan_pass(workspace_dev, n_samples, obs_dim);
    const float* const params = params_dev;
    const unsigned char* const prep = reinterpret_cast<const unsigned char*>(prep_dev);
    const float* const kls = kl_state_dev;
    if (obs_dim == 16 && X3_SCHED)
        hipLaunchKernelGGL(mlp64_pass_both_x3s_kl, dim3(pl.blocks), dim3(64 * x3s::SW), 0, st, params, prep, act_dev, logp_old_dev, rtg_dev, adv_dev,
                           (long long)n_samples, var, clip, pl.inv_n, 3, pl.partial, pl.stats_partial, pl.partial_c, pl.stats_partial_c, kls);
    else if (obs_dim == 16)
        hipLaunchKernelGGL(mlp64_pass_both_x3_kl<16>, dim3(pl.blocks), dim3(64 * XPad<16>::NW), 0, st, params, prep, act_dev, logp_old_dev, rtg_dev,
                           adv_dev, (long long)n_samples, var, clip, pl.inv_n, 3, pl.partial, pl.stats_partial, pl.partial_c, pl.stats_partial_c, kls);
    else
        hipLaunchKernelGGL(mlp64_pass_both_x3_kl<42>, dim3(pl.blocks), dim3(64 * XPad<42>::NW), 0, st, params, prep, act_dev, logp_old_dev, rtg_dev,
                           adv_dev, (long long)n_samples, var, clip, pl.inv_n, 3, pl.partial, pl.stats_partial, pl.partial_c, pl.stats_partial_c, kls);
    return reduce_and_step(who, pl, params_dev, adam_m_dev, adam_v_dev, grad_dev, stats_dev, lr, beta1, beta2, eps, step, max_norm, clip_stats_dev,
                           kl_limit, kl_state_dev, stream);
}

}  // extern "C"
#pragma GCC visibility pop
