// ppo_mlp64_kl.hip -- navppo_mlp64_update_epoch_kl and navppo_mlp64_bf16x3_update_epoch_kl: the clipped epochs of ppo_mlp64.hip with
// an early stop at a KL limit (include/navppo.h "Early stop at a KL limit").
//
// The kernels are ppo_mlp64.hip's own text compiled a second time as their gated twins (navppo_internal.h, NAVPPO_KL_TU):
// mlp64_pass_both_kl<IN, F16>, mlp64_pass_both_x3_kl<IN>, mlp64_pass_both_x3s_kl (the hand-placed stream; tests/test_target_kl_cpu.py
// lints its listing like the original's) and reduce_adam_kl<false> -- one uniform read of kl_state[0] at entry and a branch to the end,
// then the same body.  The step launch (clip_adam_kl_kernel, ppo_mlp64.hip) takes the decision.
// The launch sequence is compiled a second time too: mlp64_epoch<NavppoMode::kClipKl> of the included file, the clipped epoch's
// launches with every kernel its twin.  What is left here are the two entry points.
#define NAVPPO_KL_TU 1
#include "ppo_mlp64.hip"

#pragma GCC visibility push(default)
extern "C" {

int navppo_mlp64_update_epoch_kl(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                                 const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                 float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                 float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                 float* clip_stats_dev, float kl_limit, float* kl_state_dev, void* stream) {
    return mlp64_epoch<NavppoMode::kClipKl>("navppo_mlp64_update_epoch_kl", params_dev, f32_rows(obs_dev, obs_dim, obs_f16),
                                            {act_dev, logp_old_dev, rtg_dev, adv_dev, n_samples, var, clip}, 3,
                                            {lr, beta1, beta2, eps, step, adam_m_dev, adam_v_dev, max_norm, clip_stats_dev, kl_limit, kl_state_dev},
                                            grad_dev, stats_dev, workspace_dev, stream);
}

int navppo_mlp64_bf16x3_update_epoch_kl(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                        const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                        float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                        float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                        float* clip_stats_dev, float kl_limit, float* kl_state_dev, void* stream) {
    return mlp64_epoch<NavppoMode::kClipKl>("navppo_mlp64_bf16x3_update_epoch_kl", params_dev, x3_rows(prep_dev, obs_dim),
                                            {act_dev, logp_old_dev, rtg_dev, adv_dev, n_samples, var, clip}, 3,
                                            {lr, beta1, beta2, eps, step, adam_m_dev, adam_v_dev, max_norm, clip_stats_dev, kl_limit, kl_state_dev},
                                            grad_dev, stats_dev, workspace_dev, stream);
}

}  // extern "C"
#pragma GCC visibility pop
