// ppo_resmlp512_var.hip -- navppo_resmlp512_update_epoch_var: the clipped epoch of ppo_resmlp512.hip with a learned exploration
// variance (include/navppo.h "Learned exploration variance").
//
// The kernels are ppo_resmlp512.hip's own text compiled a third time (navppo_internal.h, NAVPPO_VAR_TU).  Only resmlp_e2_var<false>
// differs from its original: it reads the variance from var_state[1] at its entry and carries an 18th sum -- the per-sample term of
// d(actor loss)/d(log var) -- into column EC_STAT + 3 of the actor's streaming rows.  The other kernels (resmlp_fwd_var<16 | 32>,
// resmlp_bwd2s_var<f16>, resmlp_bwd_var<16, 2, 8>, resmlp_reduce_var<false>) take the state as an unused last argument: the launch
// sequence is ONE text for every unit (loss_grad_impl<kClip | kClipLr> of the included file), then one launch that steps log var
// (ppo_learned_var.hip).  Built with the flags of ppo_resmlp512.hip (navbot_ppo_amd/build.py): the hand-placed stream of
// resmlp_bwd2s_var needs the same register-allocation flag.
#define NAVPPO_VAR_TU 1
#define NAVPPO_KL_TU 1
#include "ppo_resmlp512.hip"

#pragma GCC visibility push(default)
extern "C" {

int navppo_resmlp512_update_epoch_var(float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                                      const float* rtg_dev, const float* adv_dev, int64_t n_samples, float clip, float lr, float beta1,
                                      float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev, float* grad_dev,
                                      float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev, float kl_target,
                                      float lr_min, float lr_max, int32_t adapt, float* lr_state_dev, float ent_coef, float var_min,
                                      float var_max, float* var_state_dev, void* stream) {
    const char* const who = "navppo_resmlp512_update_epoch_var";
    // (the streaming kernel takes the variance from var_state_dev[1]: the by-value member only has to pass the batch's check)
    const NavppoBatch b{act_dev, logp_old_dev, rtg_dev, adv_dev, n_samples, 1.0f, clip};
    const NavppoVar lv{ent_coef, var_min, var_max, var_state_dev};
    NavppoStep s{lr, beta1, beta2, eps, step, adam_m_dev, adam_v_dev, max_norm, clip_stats_dev};
    s.var_state = var_state_dev;
    if (!lr_state_dev)   // the clipped epoch at the constant `lr`
        return loss_grad_impl<NavppoMode::kClip>(who, params_dev, obs_dev, obs_f16, b, s, grad_dev, stats_dev, workspace_dev, stream, &lv);
    s.kl_target = kl_target;
    s.lr_min = lr_min;
    s.lr_max = lr_max;
    s.adapt = adapt;
    s.lr_state = lr_state_dev;
    return loss_grad_impl<NavppoMode::kClipLr>(who, params_dev, obs_dev, obs_f16, b, s, grad_dev, stats_dev, workspace_dev, stream, &lv);
}

}  // extern "C"
#pragma GCC visibility pop
