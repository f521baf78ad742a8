// ppo_mlp64_var.hip -- navppo_mlp64_update_epoch_var and navppo_mlp64_bf16x3_update_epoch_var: the clipped epochs of ppo_mlp64.hip with
// a learned exploration variance (include/navppo.h "Learned exploration variance").
//
// The kernels are ppo_mlp64.hip's own text compiled a third time (navppo_internal.h, NAVPPO_VAR_TU): mlp64_pass_both_var<IN, F16>,
// mlp64_pass_both_x3_var<IN>, mlp64_pass_both_x3s_var (the hand-placed stream) and reduce_adam_var<false>.  The passes read the
// variance from var_state[1] at their entry instead of the by-value argument and carry one more per-lane sum -- the per-sample term of
// d(actor loss)/d(log var) -- into column 3 of the actor's statistics rows; everything else is the same text, so the nets' gradients
// are the clipped epoch's bit for bit.  The launch sequence is mlp64_epoch<kClip | kClipLr> of the included file with every kernel
// its twin, then one launch that steps log var (ppo_learned_var.hip).  What is left here are the two entry points.
#define NAVPPO_VAR_TU 1
#define NAVPPO_KL_TU 1
#include "ppo_mlp64.hip"

namespace {

// lr_state_dev NULL: the clipped epoch at the constant `lr`; else the adaptive-rate epoch
int mlp64_epoch_var(const char* who, float* params, const Mlp64Rows& x, const NavppoBatch& b, NavppoStep s, float kl_target, float lr_min,
                    float lr_max, int32_t adapt, float* lr_state, const NavppoVar& lv, float* grad, float* stats, void* workspace,
                    void* stream) {
    s.var_state = lv.state;
    if (!lr_state) return mlp64_epoch<NavppoMode::kClip>(who, params, x, b, 3, s, grad, stats, workspace, stream, &lv);
    s.kl_target = kl_target;
    s.lr_min = lr_min;
    s.lr_max = lr_max;
    s.adapt = adapt;
    s.lr_state = lr_state;
    return mlp64_epoch<NavppoMode::kClipLr>(who, params, x, b, 3, s, grad, stats, workspace, stream, &lv);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int navppo_mlp64_update_epoch_var(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                                  const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float clip,
                                  float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                  float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                  float kl_target, float lr_min, float lr_max, int32_t adapt, float* lr_state_dev, float ent_coef,
                                  float var_min, float var_max, float* var_state_dev, void* stream) {
    // (the passes take the variance from var_state_dev[1]: the by-value member only has to pass the batch's check)
    return mlp64_epoch_var("navppo_mlp64_update_epoch_var", params_dev, f32_rows(obs_dev, obs_dim, obs_f16),
                           {act_dev, logp_old_dev, rtg_dev, adv_dev, n_samples, 1.0f, clip},
                           {lr, beta1, beta2, eps, step, adam_m_dev, adam_v_dev, max_norm, clip_stats_dev}, kl_target, lr_min, lr_max, adapt,
                           lr_state_dev, {ent_coef, var_min, var_max, var_state_dev}, grad_dev, stats_dev, workspace_dev, stream);
}

int navppo_mlp64_bf16x3_update_epoch_var(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                         const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float clip,
                                         float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                         float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                         float kl_target, float lr_min, float lr_max, int32_t adapt, float* lr_state_dev, float ent_coef,
                                         float var_min, float var_max, float* var_state_dev, void* stream) {
    return mlp64_epoch_var("navppo_mlp64_bf16x3_update_epoch_var", params_dev, x3_rows(prep_dev, obs_dim),
                           {act_dev, logp_old_dev, rtg_dev, adv_dev, n_samples, 1.0f, clip},
                           {lr, beta1, beta2, eps, step, adam_m_dev, adam_v_dev, max_norm, clip_stats_dev}, kl_target, lr_min, lr_max, adapt,
                           lr_state_dev, {ent_coef, var_min, var_max, var_state_dev}, grad_dev, stats_dev, workspace_dev, stream);
}

}  // extern "C"
#pragma GCC visibility pop
