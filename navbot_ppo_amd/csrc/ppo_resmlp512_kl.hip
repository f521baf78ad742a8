// ppo_resmlp512_kl.hip -- navppo_resmlp512_update_epoch_kl: the clipped epoch of ppo_resmlp512.hip with an early stop at a KL limit
// (include/navppo.h "Early stop at a KL limit").
//
// The kernels are ppo_resmlp512.hip's own text compiled a second time as their gated twins (navppo_internal.h, NAVPPO_KL_TU):
// resmlp_fwd_kl<16 | 32>, resmlp_e2_kl<false>, resmlp_bwd2s_kl<f16> (resmlp_bwd_kl<32, 2, 4> under -DRESMLP_BWD2S=0),
// resmlp_bwd_kl<16, 2, 8> and resmlp_reduce_kl<false> -- one uniform read of kl_state[0] at entry and a branch to the end, then
// the same body.  The step launch (clip_adam_kl_kernel, ppo_mlp64.hip) takes the decision.  The launch sequence is compiled a second
// time too: loss_grad_impl<NavppoMode::kClipKl> of the included file, the clipped epoch's launches with every kernel its twin.  What
// is left here is the entry point.  Built with the flags of ppo_resmlp512.hip
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
    return loss_grad_impl<NavppoMode::kClipKl>("navppo_resmlp512_update_epoch_kl", params_dev, obs_dev, obs_f16,
                                               {act_dev, logp_old_dev, rtg_dev, adv_dev, n_samples, var, clip},
                                               {lr, beta1, beta2, eps, step, adam_m_dev, adam_v_dev, max_norm, clip_stats_dev, kl_limit, kl_state_dev},
                                               grad_dev, stats_dev, workspace_dev, stream);
}

}  // extern "C"
#pragma GCC visibility pop
