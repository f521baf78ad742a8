// ppo_resmlp512_kl.hip -- navppo_resmlp512_update_epoch_kl: the clipped epoch of ppo_resmlp512.hip with an early stop at a KL limit
// (include/navppo.h "Early stop at a KL limit").
//
// The kernels are ppo_resmlp512.hip's own text compiled a second time as their gated twins (navppo_internal.h, NAVPPO_KL_TU):
// resmlp_fwd_kl<16 | 32>, resmlp_e2_kl<false>, resmlp_bwd2s_kl<f16> (resmlp_bwd_kl<32, 2, 4> under -DRESMLP_BWD2S=0),
// resmlp_bwd_kl<16, 2, 8> and resmlp_reduce_kl<false> -- one uniform read of kl_state[0] at entry and a branch to the end, then
// the same body.  The step launch (clip_adam_kl_kernel, ppo_mlp64.hip) takes the decision.  Built with the flags of ppo_resmlp512.hip
// (navbot_ppo_amd/build.py): the hand-placed stream of resmlp_bwd2s_kl needs the same register-allocation flag, and
// tests/test_target_kl_cpu.py lints its listing like the original's.
#define NAVPPO_KL_TU 1
#include "ppo_resmlp512.hip"

#pragma GCC visibility push(default)
extern "C" {

int navppo_resmlp512_update_epoch_kl(float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                                     const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip, float lr,
                                     float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                     float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                     float kl_limit, float* kl_state_dev, void* stream) {
    const char* const name = "navppo_resmlp512_update_epoch_kl";
    if (!navppo_max_norm_ok(max_norm) || !clip_stats_dev) {
        navppo_set_error("navppo_resmlp512_update_epoch_kl: max_norm must be > 0 (+inf allowed) and clip_stats_dev [4] not null");
        return -1;
    }
    if (!navppo_kl_limit_ok(kl_limit) || !kl_state_dev) {
        navppo_set_error("navppo_resmlp512_update_epoch_kl: kl_limit must be > 0 (+inf allowed) and kl_state_dev [4] not null");
        return -1;
    }
    if (!params_dev || !obs_dev || !act_dev || !logp_old_dev || !rtg_dev || !adv_dev || !grad_dev || !stats_dev || !workspace_dev ||
        n_samples < 1 || !(var > 0.f) || !adam_m_dev || !adam_v_dev || step < 1) {
        navppo_set_error("navppo_resmlp512_update_epoch_kl: bad argument");
        return -1;
    }
    if (((uintptr_t)obs_dev & 15) || ((uintptr_t)act_dev & 7)) {
        navppo_set_error("navppo_resmlp512_update_epoch_kl: obs must be 16-byte and act 8-byte aligned");
        return -1;
    }
    // the launches of loss_grad_impl's clipped epoch (ppo_resmlp512.hip), same grids and arguments, every one its gated twin
    hipStream_t st = (hipStream_t)stream;
    const Plan p = make_plan(workspace_dev, n_samples, 2);
    const float inv_n = 1.0f / (float)n_samples;
    const int f16 = obs_f16 != 0;
    const long long n = n_samples;
    const float* const params = params_dev;
    const float* const kls = kl_state_dev;
    hipLaunchKernelGGL(resmlp_fwd_kl<16>, dim3(p.wgs), dim3(kThreads), 0, st, params, 0, 2, obs_dev, (const float*)nullptr, (float*)nullptr, n,
                       p.groups * FSP, p.p1, f16, kls);
    hipLaunchKernelGGL(resmlp_fwd_kl<32>, dim3(p.wgs), dim3(kThreads), 0, st, params, 0, 2, obs_dev, (const float*)p.p1, p.h1, n, p.groups * FSP,
                       p.p2, f16, kls);
    hipLaunchKernelGGL(resmlp_e2_kl<false>, dim3(p.e_blocks, 2), dim3(kEThreads), 0, st, params, 0, obs_dev, (const float*)p.h1, (const float*)p.p2,
                       act_dev, logp_old_dev, rtg_dev, adv_dev, n, var, clip, inv_n, p.dy2, p.epart, (float*)nullptr, f16, kls);
    if constexpr (RESMLP_BWD2S && kBwd2Waves == b2s::SW) {
        if (f16)
            hipLaunchKernelGGL(resmlp_bwd2s_kl<true>, dim3(p.wgs), dim3(64 * b2s::SW), 0, st, params, 2, obs_dev, (const float*)p.h1,
                               (const float*)p.dy2, n, p.groups, p.wpart, p.qb, kls);
        else
            hipLaunchKernelGGL(resmlp_bwd2s_kl<false>, dim3(p.wgs), dim3(64 * b2s::SW), 0, st, params, 2, obs_dev, (const float*)p.h1,
                               (const float*)p.dy2, n, p.groups, p.wpart, p.qb, kls);
    } else
        hipLaunchKernelGGL((resmlp_bwd_kl<32, 2, kBwd2Waves>), dim3(p.wgs), dim3(64 * kBwd2Waves), 0, st, params, 2, obs_dev, (const float*)p.h1,
                           (const float*)p.dy2, n, p.groups, p.wpart, p.qb, (const float*)nullptr, f16, kls);
    hipLaunchKernelGGL((resmlp_bwd_kl<16, 2, kBwd1Waves>), dim3(p.wgs), dim3(64 * kBwd1Waves), 0, st, params, 2, obs_dev, (const float*)p.h1,
                       (const float*)p.dy2, n, p.groups, p.wpart, (float*)nullptr, (const float*)p.qb, f16, kls);
    const int rblocks = (rp::P_ACTOR + rp::P_CRITIC + 63) / 64;
    hipLaunchKernelGGL(resmlp_reduce_kl<false>, dim3(rblocks), dim3(64 * kRedGroups), 0, st, (const float*)p.wpart, p.groups * kBwd1Waves,
                       p.groups * kBwd2Waves, (const float*)p.epart, p.e_blocks, inv_n, grad_dev, stats_dev, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f, p.epart, 0, kls);
    navppo_launch_clip_adam(params_dev, grad_dev, adam_m_dev, adam_v_dev, rp::P_ACTOR + rp::P_CRITIC, rp::P_ACTOR, 1.0f, max_norm, lr, beta1, beta2,
                            eps, step, p.epart, rblocks, kGnSlotsR, EP, clip_stats_dev, stream, stats_dev + 1, kl_limit, kl_state_dev);
    if (!launch_ok(name)) {
        navppo_set_error(g_err.c_str());
        return -2;
    }
    return 0;
}

}  // extern "C"
#pragma GCC visibility pop
