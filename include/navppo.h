/*
 * navppo.h -- C ABI of the fused PPO loss + gradient kernel for the D-64-64 heads (libnavsim.so).
 *
 * Replaces one pass of the reference's update loop body -- PPO.evaluate() (project_ppo/src/ppo.py:708-737),
 * the ratio / clipped-surrogate / MSE losses (ppo.py:316-343) and both backward() calls (ppo.py:349,386) --
 * for the "mlp64x2" policy (actor: Linear(D,64)-ReLU-Linear(64,64)-ReLU-{sigmoid(Linear(64,1)), tanh(Linear(64,1))},
 * critic: ...-Linear(64,1); net_actor.py:147-189, graph_code/ppo_for_beginners/network.py:11-50).
 * The optimiser step (Adam, ppo.py:381,392) and the gradient all-reduce stay with the caller.
 *
 * Observation rows (every `obs_dev` below): `obs_dim` = D = n_beams + 6 columns -- 16 (10 beams: main.py:18, BASELINE
 * configs[0..2] and [4]) or 42 (36 beams: configs[3]) -- of float32 (`obs_f16` = 0) or float16 (`obs_f16` = 1, configs[4]'s
 * "fp16 obs buffers", navsim_cfg.obs_f16), row-major and dense.  Half rows are widened to float32 as they are loaded; all
 * arithmetic behind the load is float32 either way.
 *
 * All pointers are DEVICE pointers owned by the caller; calls are asynchronous on `stream` (hipStream_t as void*);
 * return 0 or a negative code, message in navppo_last_error().  float32 arithmetic throughout (navppo_mlp64_*: f32-input MFMA, exact
 * f32 fma chains; navppo_mlp64_bf16x3_* and navppo_resmlp512_*: float32 products from three bf16 pieces per operand, see there);
 * no CPU fallback.  Alignment: params_dev / actor_params_dev 16 bytes, act_dev 8 bytes, obs_dev 16 bytes for
 * 16 columns, 8 bytes for 42 float32 columns, 4 bytes for 42 float16 columns (torch allocations are 256-byte aligned),
 * checked at the call.
 */
#ifndef NAVPPO_H
#define NAVPPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAVPPO_MLP64_ACTOR_PARAMS_D(d) ((d) * 64 + 64 + 64 * 64 + 64 + 64 + 1 + 64 + 1)  /* D = 16: 5378, D = 42: 7042 */
#define NAVPPO_MLP64_CRITIC_PARAMS_D(d) ((d) * 64 + 64 + 64 * 64 + 64 + 64 + 1)          /* D = 16: 5313, D = 42: 6977 */
#define NAVPPO_MLP64_ACTOR_PARAMS NAVPPO_MLP64_ACTOR_PARAMS_D(16)
#define NAVPPO_MLP64_CRITIC_PARAMS NAVPPO_MLP64_CRITIC_PARAMS_D(16)
#define NAVPPO_MLP64_MAX_BLOCKS 512     /* rows of the workspace (the kernel launches one persistent workgroup per CU) */

const char* navppo_last_error(void);

/* bytes of scratch `workspace_dev` must provide (per-workgroup partial gradients) for rows of obs_dim columns; 0 = bad obs_dim */
size_t navppo_mlp64_workspace_bytes(int32_t obs_dim);

/*
 *   params_dev   [PA + PC] f32       actor then critic (PA = NAVPPO_MLP64_ACTOR_PARAMS_D(D), PC = ..._CRITIC_PARAMS_D(D); D = 16:
 *                                    5378 + 5313), each in nn.Module.named_parameters() order:
 *                                    layer1.weight[64,D], layer1.bias[64], layer2.weight[64,64], layer2.bias[64],
 *                                    layer3.weight[1,64], layer3.bias[1] (, layer4.weight[1,64], layer4.bias[1])
 *   obs_dev      [n,D]   batch_obs (f32 | f16, see above)      act_dev [n,2] batch_acts (the clamped actions, ppo.py:546)
 *   logp_old_dev [n]     batch_log_probs  rtg_dev [n]   batch_rtgs      adv_dev [n] normalised advantages A_k (ppo.py:284)
 *   var          diagonal of cov_mat (ppo.py:123-124)   clip   PPO clip (ppo.py:770)
 *   grad_dev     [PA + PC] f32      out: d(actor_loss)/d(actor params), d(critic_loss)/d(critic params), losses being
 *                                    MEANS over the n samples (ppo.py:342-343) -- overwritten, not accumulated
 *   stats_dev    [8] f32            out: [0] actor_loss [1] approx_kl [2] clip_frac (ppo.py:326,335) [4] critic_loss
 */
int navppo_mlp64_loss_grad(const float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                           const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples,
                           float var, float clip, float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);

/*
 * One net of navppo_mlp64_loss_grad (net 0 = actor: ppo.py:316-342,349; net 1 = critic: :343,386): writes that net's slice of
 * grad_dev and its statistics only.  The multi-GPU epoch launches the actor's pass, starts the all-reduce of the actor's
 * gradient slice, and runs the critic's pass while that all-reduce is in flight (same arguments as navppo_mlp64_loss_grad).
 */
int navppo_mlp64_loss_grad_net(int32_t net, const float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16,
                               const float* act_dev, const float* logp_old_dev, const float* rtg_dev, const float* adv_dev,
                               int64_t n_samples, float var, float clip, float* grad_dev, float* stats_dev, void* workspace_dev,
                               void* stream);

/*
 * torch.optim.Adam's step (defaults: no weight decay, no amsgrad) on a flat buffer with the gradient scaled first: the
 * multi-GPU epoch is navppo_mlp64_loss_grad -> all-reduce(sum) of grad_dev over RCCL -> navppo_adam_step(grad_scale = 1 / world).
 */
int navppo_adam_step(float* params_dev, const float* grad_dev, float* adam_m_dev, float* adam_v_dev, int64_t n, float grad_scale,
                     float lr, float beta1, float beta2, float eps, int32_t step, void* stream);

/*
 * The episode sums behind one iteration's log line (ppo.py:552-560, :833) over the [T, N] buffers a rollout fills (n = T N
 * entries each): sums_dev [6] f64 = episodes (ended), successes (arrive), collisions (done and not arrive), timeouts (ended,
 * neither), sum of ep_length (all entries; the buffer is zero where no episode ended), sum of ep_return over ended entries.
 * workspace_dev: NAVPPO_EPISODE_SUMS_WS_BYTES.  Per-block partials are added in a fixed order: the result is deterministic.
 */
#define NAVPPO_EPISODE_SUMS_WS_BYTES (256 * 6 * 8)
int navppo_episode_sums(const uint8_t* ended_dev, const uint8_t* arrive_dev, const uint8_t* done_dev, const int32_t* ep_length_dev,
                        const float* ep_return_dev, int64_t n, double* sums_dev, void* workspace_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Per-group episode sums (csrc/ppo_group_sums.hip): navppo_episode_sums per GROUP of envs -- the scenario an env plays, its tape id
 * of a mover bank -- over the [T, N] buffers a rollout fills.  group_dev [N] i32: the group of every env.  sums_dev [K][8] f64, row k
 * over the columns n with group[n] == k:
 *   0 episodes (ended)   1 successes (arrive and ended)   2 collisions (done, not arrive, ended)   3 time-outs (ended, neither)
 *   4 sum of ep_length over all entries   5 sum of ep_return over ended entries   (entry by entry navppo_episode_sums' figures)
 *   6 sum of |adv| over all entries (adv_dev [T, N] f32, nullable: then 0)        7 rows: T x the number of envs of the group
 * A group without envs gives a zero row; an id outside [0, K) is counted in no row (and indexes nothing).  1 <= K <= 1024, T, N >= 1.
 * Columns 0..4 and 7 are exact integers; summed over k, columns 0..5 are navppo_episode_sums' (5 up to the summation order).
 * No atomics: every column's partial sums per chunk of T are stored to the workspace, then one workgroup per group adds its columns'
 * partials in ascending env order and a fixed tree -- two calls on the same buffers give the same bits.
 * ep_length / ep_return / adv / group 4-byte, sums / workspace 8-byte aligned.  workspace_dev: navppo_group_sums_ws_bytes(T, N, K)
 * bytes (0 = sizes the entry point refuses).  Null required pointers, bad sizes, a null workspace: -1 and navppo_last_error().
 */
#define NAVPPO_GROUP_SUMS_COLS 8
size_t navppo_group_sums_ws_bytes(int32_t T, int32_t N, int32_t K);
int navppo_group_sums(const uint8_t* ended_dev, const uint8_t* arrive_dev, const uint8_t* done_dev, const int32_t* ep_length_dev,
                      const float* ep_return_dev, const float* adv_dev, const int32_t* group_dev, int32_t T, int32_t N, int32_t K,
                      double* sums_dev, void* workspace_dev, void* stream);

/* V = critic(obs).squeeze() (ppo.py:275, :724) for n rows: the forward half of the critic's fused pass.  value_dev [n] f32. */
int navppo_mlp64_value(const float* critic_params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, int64_t n_samples,
                       float* value_dev, void* stream);

/*
 * One whole update epoch of ppo.py:305-392 on one GPU: navppo_mlp64_loss_grad followed by the two Adam steps of
 * ppo.py:381,392 (torch.optim.Adam defaults: no weight decay, no amsgrad) applied in place by the kernel that sums the
 * workgroups' partial gradients.  step = 1, 2, ... (Adam's bias correction); adam_m_dev / adam_v_dev [PA + PC] f32 are
 * the optimiser's moments (zero before the first step).  grad_dev and stats_dev are filled as by navppo_mlp64_loss_grad; in addition
 * stats_dev[3] / [7] receive the SQUARED gradient norms of the actor / the critic of the update_epoch call BEFORE this one on the same
 * workspace (calls with consecutive `step`; the value of the first call is meaningless): with the last epoch's norms taken from grad_dev
 * a caller has every epoch's norms for the means the reference logs (ppo.py:351-352, 389-390) at no extra launch.  The same holds for
 * navppo_mlp64_bf16x3_update_epoch and navppo_resmlp512_update_epoch.
 * Multi-GPU runs use navppo_mlp64_loss_grad + an all-reduce + their own optimiser step instead.
 */
int navppo_mlp64_update_epoch(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                              const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                              float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                              float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Update epochs with gradient-norm clipping and a non-finite guard ON THE DEVICE (the epochs of an update are queued without a host
 * round trip, so the host cannot guard them): navppo_mlp64_update_epoch_clipped, navppo_mlp64_bf16x3_update_epoch_clipped and
 * navppo_resmlp512_update_epoch_clipped take their unclipped twins' arguments plus `max_norm` and `clip_stats_dev` in front of
 * `stream`; navppo_adam_step_clipped is the multi-GPU form.  The same pass kernels produce the partial rows; the reduction then only
 * sums them and a second small launch clips and steps.  Per NET (the reference clips and steps the two nets separately,
 * ppo.py:352,381 / :389,392):
 *   1. s = the float32 sum of squares of the net's summed (and scaled) gradient, added in one fixed order.
 *   2. s not finite (NaN, or overflow to inf): the net's parameters and both its moments are NOT WRITTEN, its coefficient is reported
 *      as 0 and its slice of grad_dev keeps the unclipped sum.  The caller's `step` advances all the same: the host learns of a skipped
 *      step only from clip_stats_dev, i.e. after a synchronisation of its own -- a net that skipped k steps has taken k fewer Adam
 *      steps than `step` says (its bias corrections are those of `step`).
 *   3. else coef = min(1, max_norm / (sqrt(s) + 1e-6)) -- torch.nn.utils.clip_grad_norm_ -- and Adam runs on g * coef, with the very
 *      expression of the unclipped epochs: max_norm = +inf gives their bits.
 *   grad_dev        out: the CLIPPED gradient (what .grad holds after torch's call)
 *   clip_stats_dev  [4] f32 out: s_actor, s_critic, coef_actor, coef_critic of THIS call (no lag, no dependence on call parity)
 *   stats_dev       [0..2] and [4] as navppo_mlp64_loss_grad; [3] and [7] are unspecified
 *   max_norm        > 0, +inf allowed; 0, negative or NaN: -1.  clip_stats_dev NULL: -1.
 * Workspaces are those of the unclipped entry points (the squared-norm slots are shared): do not interleave clipped and unclipped
 * epochs on one workspace if stats_dev[3] / [7] of the unclipped ones are read.
 */
int navppo_mlp64_update_epoch_clipped(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                                      const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                      float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                      float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                      float* clip_stats_dev, void* stream);

/*
 * navppo_adam_step with the contract above: grad_dev [n] holds the all-reduced SUM; the norms are those of grad_dev x grad_scale, taken
 * separately over [0, n_first) (the actor) and [n_first, n) (the critic); 0 <= n_first <= n (an empty segment has s = 0, coefficient 1).
 * grad_dev receives grad x grad_scale x coef.
 */
int navppo_adam_step_clipped(float* params_dev, float* grad_dev, float* adam_m_dev, float* adam_v_dev, int64_t n, int64_t n_first,
                             float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int32_t step,
                             float* clip_stats_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Early stop at a KL limit ON THE DEVICE (`target_kl` of Stable-Baselines3 / Spinning Up: stop the update's remaining epochs once the
 * policy has moved too far from the one that collected the batch).  navppo_mlp64_update_epoch_kl, navppo_mlp64_bf16x3_update_epoch_kl
 * and navppo_resmlp512_update_epoch_kl take exactly the arguments of their *_clipped twins plus `kl_limit` and `kl_state_dev` in front
 * of `stream`; navppo_adam_step_kl is the multi-GPU form.  max_norm = +inf means "no clipping", as above.
 *   kl_state_dev  [4] f32.  The caller ZEROES it before the first epoch of an update; afterwards only the library writes it:
 *                 [0] stopped (0 or 1)   [1] number of calls since zeroing that went on to the optimiser step
 *                 [2] the approx_kl that tripped the stop (unchanged if nothing tripped)   [3] the `step` argument of the tripping call
 *   kl_limit      > 0, +inf allowed; 0, negative or NaN: -1.  kl_state_dev NULL: -1.  The *_clipped checks are unchanged.
 * Per call:
 *   1. stopped (kl_state[0] != 0 at entry): EVERY kernel of the epoch -- the pass launches (for the 512-wide nets also the streaming
 *      kernel), the reduction and the step launch -- returns at its entry.  Parameters, both moments, grad_dev, stats_dev,
 *      clip_stats_dev and kl_state_dev keep their contents; the workspace stays scratch.
 *   2. else the passes and the reduction run exactly as in the *_clipped entry point, and the step launch reads kl = stats_dev[1]
 *      (the mean of (ratio - 1) - log ratio, ppo.py:326), which the launch before it wrote: every workgroup derives the same decision
 *      from the same bits and none waits for another.
 *   3. trip, !(kl <= kl_limit) -- a NaN kl trips: NEITHER net is stepped (parameters and moments are not written), grad_dev keeps the
 *      unclipped sum, clip_stats_dev = (s_actor, s_critic, 0, 0), kl_state = (1, unchanged, kl, step).
 *   4. no trip: the clipped epoch's step with the very same expression, and kl_state[1] += 1.  kl_limit = +inf on a zeroed state gives
 *      the bits of *_update_epoch_clipped; with max_norm = +inf as well, those of *_update_epoch.
 * The check comes before the step and the stop covers BOTH nets (Stable-Baselines3's convention).  Keeping the critic training after
 * the actor stops (Spinning Up) would need a per-net Adam step count across this ABI and is not offered.  A caller whose Adam step
 * count must be the number of steps TAKEN reads kl_state[1] after its own synchronisation.  Every family's passes are gated (the
 * hand-placed streams included), so a stopped epoch costs its launches only.
 */
int navppo_mlp64_update_epoch_kl(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                                 const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                 float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                 float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                 float* clip_stats_dev, float kl_limit, float* kl_state_dev, void* stream);

/*
 * navppo_adam_step_clipped with the contract above.  kl_dev: a device scalar holding the GLOBAL approx_kl of this epoch (multi-GPU:
 * all-reduce [kl x n, n] and divide); the passes in front of it (navppo_*_loss_grad) are not gated, so no time is saved on this path.
 * On a trip grad_dev keeps the all-reduced sum and clip_stats_dev = (s_actor, s_critic, 0, 0).
 */
int navppo_adam_step_kl(float* params_dev, float* grad_dev, float* adam_m_dev, float* adam_v_dev, int64_t n, int64_t n_first,
                        float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int32_t step,
                        float* clip_stats_dev, float kl_limit, float* kl_state_dev, const float* kl_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Adaptive learning rate ON THE DEVICE (the KL-adaptive step size of rsl_rl / rl_games: after every optimiser step the rate is divided
 * by 1.5 when the policy moved more than twice the desired KL and multiplied by 1.5 when it moved less than half of it).  The epochs of
 * an update are queued without a host round trip, so the rate cannot be a by-value argument: it lives in lr_state_dev.
 * navppo_mlp64_update_epoch_lr, navppo_mlp64_bf16x3_update_epoch_lr and navppo_resmlp512_update_epoch_lr take exactly the arguments of
 * their *_clipped twins plus `kl_target, lr_min, lr_max, adapt, lr_state_dev` in front of `stream`; navppo_adam_step_lr is the multi-GPU
 * form.  The passes, the reduction and their launches are those of *_clipped (nothing is gated); only the step launch differs
 * (clip_adam_lr_kernel).  max_norm = +inf means "no clipping", as above.
 *   lr_state_dev  [4] f32.  [0], [1]: two learning-rate slots   [2] raises, [3] lowerings since the caller zeroed the state.
 *                 The caller zeroes it (a fresh run) or writes a saved rate into BOTH slots (a resumed run); afterwards only the
 *                 library writes it.
 *   kl_target     > 0;  lr_min > 0;  lr_max >= lr_min;  adapt 0 or 1;  lr_state_dev not NULL -- else -1 and nothing is launched (a NaN
 *                 fails each comparison).  The *_clipped checks are unchanged.
 * Per call, with Adam step count `step` (calls on one state use consecutive `step`, as for stats_dev[3] / [7]):
 *   1. lr_in = lr_state[step & 1]; a slot holding exactly 0.0f means "not started": lr_in = the `lr` argument.
 *   2. kl = stats_dev[1] of this call (the mean of (ratio - 1) - log ratio, ppo.py:326; navppo_adam_step_lr: *kl_dev), which an
 *      EARLIER launch wrote.  In float32, the expressions as written (the library is compiled with -ffp-contract=off):
 *        adapt == 0:                                   lr = lr_in
 *        else !(kl <= 2.0f * kl_target):               lr = fmaxf(lr_min, lr_in / 1.5f)      -- a NaN kl lowers
 *        else kl < 0.5f * kl_target && kl > 0.0f:      lr = fminf(lr_max, lr_in * 1.5f)
 *        else:                                         lr = lr_in
 *      Every workgroup of the step launch derives lr itself from the same bits; none waits for another.
 *   3. the clipped epoch's step with that lr, the very expression of *_clipped: the non-finite guard, max_norm, grad_dev and
 *      clip_stats_dev behave and are filled as there.
 *   4. workgroup 0 writes lr to lr_state[(step + 1) & 1] and adds 1 to [2] (the raising branch was taken) or [3] (the lowering branch
 *      was taken) -- also where a clamp held the rate, and whether or not a net was skipped.
 * Two slots because the step launch has many workgroups (42 to about 400) that must all step with ONE rate: a single slot rewritten
 * by workgroup 0 would be read by workgroups of the same launch that start later.  The slot a launch writes is read by the NEXT call only.
 * adapt = 0 on a zeroed state gives the bits of *_update_epoch_clipped with the same lr; with max_norm = +inf as well, those of
 * *_update_epoch.  A caller passes adapt = 0 for the first step of an update: the weights are then those that collected the batch and
 * kl is the rounding noise of two log-probability computations.  navbot_ppo_amd.ppo.adaptive_lr_reference is the host mirror of step 2.
 * Not combined with the *_kl entry points (two answers to the same signal).
 */
int navppo_mlp64_update_epoch_lr(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                                 const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                 float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                 float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                 float* clip_stats_dev, float kl_target, float lr_min, float lr_max, int32_t adapt, float* lr_state_dev,
                                 void* stream);

/*
 * navppo_adam_step_clipped with the contract above.  kl_dev: a device scalar holding the GLOBAL approx_kl of this step (multi-GPU:
 * all-reduce [kl x n, n] and divide), so that every rank derives the same rate; NULL: -1.
 */
int navppo_adam_step_lr(float* params_dev, float* grad_dev, float* adam_m_dev, float* adam_v_dev, int64_t n, int64_t n_first,
                        float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int32_t step,
                        float* clip_stats_dev, float kl_target, float lr_min, float lr_max, int32_t adapt, float* lr_state_dev,
                        const float* kl_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Learned exploration variance ON THE DEVICE (the state-independent log-std of Stable-Baselines3 / rsl_rl / rl_games / CleanRL, steered
 * by an entropy coefficient).  The policy stays MVN(mean, var I) with ONE variance; theta = log var becomes a parameter of the actor
 * that is stepped after every optimiser step of the nets, so the variance cannot be a by-value argument: it lives in var_state_dev.
 * navppo_mlp64_update_epoch_var, navppo_mlp64_bf16x3_update_epoch_var and navppo_resmlp512_update_epoch_var take the arguments of their
 * *_lr twins WITHOUT the by-value `var` and with `ent_coef, var_min, var_max, var_state_dev` in front of `stream`.
 *   lr_state_dev  may be NULL: the epoch is then that of *_clipped at the constant `lr` (kl_target .. adapt are not read); else that of *_lr.
 *   max_norm      = +inf means "no clipping", as above.
 *   var_state_dev [8] f32, 16-byte aligned; the caller starts it as (log v0, v0, 0, 0, 0, 0, 0, 0), afterwards only the library writes it:
 *                 [0] theta   [1] var -- what the passes read and what a caller hands to every rollout / *_act kernel as var_dev
 *                 [2] Adam's m   [3] Adam's v   [4] the gradient of the last step taken, after the coefficient
 *                 [5] steps taken   [6] steps skipped   [7] the entropy H = 1 + log 2 pi + theta after the last step taken
 *   ent_coef      >= 0 and finite;  var_min > 0;  var_max >= var_min, both finite;  var_state_dev not NULL and 16-byte aligned -- else -1
 *                 and nothing is launched.  The checks of *_clipped (lr_state_dev NULL) / *_lr are unchanged.
 * With lp = -1/2 (d0^2 + d1^2) / var - log 2 pi - log var (d measured from the clamped action) the actor's loss is L - ent_coef H and
 *   d/d theta = sum_i dL_dlp_i (1/2 (d0^2 + d1^2)_i / var - 1) - ent_coef,   dL_dlp_i the factor of the nets' gradient, 1 / n included.
 * Per call:
 *   1. the pass twins read var = var_state[1] at their entry and compute lp as ... - logf(var) from it: parameters, moments, grad_dev,
 *      clip_stats_dev and stats_dev[0..2], [4] are bit for bit those of *_clipped / *_lr called with that var by value.  The per-sample
 *      terms of the sum above are added per workgroup, then over the workgroups in one fixed order (two calls on the same buffers give
 *      the same bits); the sum is stored to stats_dev[3] ([7] stays unspecified).
 *   2. behind the nets' step launch one more launch steps theta: g = (sum - ent_coef) * clip_stats[2] -- theta follows the ACTOR's clip
 *      coefficient of this step but is not counted in the actor's norm (a deviation from Stable-Baselines3, where log_std lies inside
 *      the one clipped parameter set).  Coefficient 0 (the actor's step was skipped for a non-finite norm) or g not finite: nothing is
 *      written but [6] += 1.
 *   3. else Adam with the call's beta1, beta2, eps and the bias corrections of `step`, the expressions of the nets' step, at the rate
 *      the nets stepped with (`lr`, or the adaptive rule's rate of this step); theta is clamped to [log var_min, log var_max] (the
 *      logarithms taken in double and rounded once), var = expf(theta), and [2] .. [5], [7] are written.
 * Every launch of the NEXT call -- and every rollout queued behind this one on the same stream -- reads the new variance.
 * navbot_ppo_amd.ppo.learned_var_reference is the host mirror of steps 2 and 3.  Not combined with the *_kl entry points.  Workspaces
 * are those of the existing entry points.  The multi-GPU form (*_loss_grad twins, the scalar riding on the all-reduce) is not built.
 */
int navppo_mlp64_update_epoch_var(float* params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev,
                                  const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float clip,
                                  float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                  float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                  float kl_target, float lr_min, float lr_max, int32_t adapt, float* lr_state_dev, float ent_coef,
                                  float var_min, float var_max, float* var_state_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * The same update (ppo.py:305-397; 16- or 42-column rows, float32 or float16) with every matrix product evaluated on the bf16 MFMA from operands split into
 * three bf16 pieces -- "bf16x3": a = a0 + a1 + a2 exactly (8 + 8 + 8 significand bits), a b ~ the six leading piece products,
 * each exact in float32, float32 accumulation, small terms first.  float32-equivalent by measurement (against float64 the
 * error is not above the f32-MFMA path's on any contraction of the kernel: tests/test_gpu_bf16x3.py), 16 x the
 * MFMA rate per piece product; inputs, outputs, statistics and the Adam step are those of the float32 entry points above,
 * which stay available (PPOConfig.update_arith = "f32").
 *
 * The observations are split ONCE per update -- they do not change over the epochs -- into prep_dev
 * (navppo_mlp64_bf16x3_prep_bytes(n, obs_dim) bytes -- 192 per sample at 16 columns, 576 at 42 (48 on chip): row-major pieces
 * for the forward products, tile-transposed pieces for the weight gradient of layer 1); the epoch entry points then take
 * (prep_dev, obs_dim) in place of (obs_dev, obs_dim, obs_f16).
 */
size_t navppo_mlp64_bf16x3_prep_bytes(int64_t n_samples, int32_t obs_dim /* 16 | 42; anything else: 0 */);
int navppo_mlp64_bf16x3_prepare(const void* obs_dev, int32_t obs_dim /* 16 | 42 */, int32_t obs_f16, int64_t n_samples, void* prep_dev,
                                void* stream);
/* as navppo_mlp64_loss_grad / _loss_grad_net / _update_epoch, same workspace (navppo_mlp64_workspace_bytes(obs_dim)) */
int navppo_mlp64_bf16x3_loss_grad(const float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                  const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip,
                                  float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);
int navppo_mlp64_bf16x3_loss_grad_net(int32_t net, const float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                      const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                      float clip, float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);
int navppo_mlp64_bf16x3_update_epoch(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev, const float* logp_old_dev,
                                     const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip, float lr,
                                     float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                     float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);

/* navppo_mlp64_bf16x3_update_epoch with clipping and the non-finite guard: see navppo_mlp64_update_epoch_clipped */
int navppo_mlp64_bf16x3_update_epoch_clipped(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                             const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                             float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                             float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                             float* clip_stats_dev, void* stream);

/* navppo_mlp64_bf16x3_update_epoch_clipped with the early stop at a KL limit: see navppo_mlp64_update_epoch_kl */
int navppo_mlp64_bf16x3_update_epoch_kl(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                        const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                        float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                        float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                        float* clip_stats_dev, float kl_limit, float* kl_state_dev, void* stream);

/* navppo_mlp64_bf16x3_update_epoch_clipped with the adaptive learning rate: see navppo_mlp64_update_epoch_lr */
int navppo_mlp64_bf16x3_update_epoch_lr(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                        const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var,
                                        float clip, float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev,
                                        float* adam_v_dev, float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm,
                                        float* clip_stats_dev, float kl_target, float lr_min, float lr_max, int32_t adapt,
                                        float* lr_state_dev, void* stream);

/* navppo_mlp64_bf16x3_update_epoch_clipped / _lr with the learned exploration variance: see navppo_mlp64_update_epoch_var */
int navppo_mlp64_bf16x3_update_epoch_var(float* params_dev, const void* prep_dev, int32_t obs_dim, const float* act_dev,
                                         const float* logp_old_dev, const float* rtg_dev, const float* adv_dev, int64_t n_samples, float clip,
                                         float lr, float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                         float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                         float kl_target, float lr_min, float lr_max, int32_t adapt, float* lr_state_dev, float ent_coef,
                                         float var_min, float var_max, float* var_state_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Minibatch updates.  Every *_loss_grad / *_update_epoch[_clipped | _kl] entry point takes pointers and n_samples, so one optimiser
 * step on a CONTIGUOUS slice [start, start + m) of a batch is the same call with every pointer advanced by `start` samples and
 * n_samples = m; for the bf16x3 entry points prep_dev advances by navppo_mlp64_bf16x3_prep_bytes(start, obs_dim), which needs
 * start % 32 == 0 (prep_dev is an array of per-32-sample tile blocks; the slice's own end may lie anywhere).  Calls on slices of one
 * update use consecutive `step` numbers; stats_dev[3] / [7] of the 512-wide nets' *_update_epoch then hold the call before only while
 * n_samples does not change between the two calls (their squared-norm slots lie behind the per-sample part of the workspace).
 *
 * navppo_shuffle_batch makes the slices random subsets: out[i] = in[pi(i)], 0 <= i < n, for the five per-sample arrays of a batch
 * (rows as navppo_mlp64_loss_grad takes them), in one launch, pi computed per index on the device -- no table, no host round trip.
 * pi is a pure function of (n, key, counter); uint32_t arithmetic wraps, `hi(p)` / `lo(p)` are the words of a 64-bit product:
 *   b = the smallest integer with 2^b >= n;  a = b / 2 (rounded down);  c = b - a
 *   (o0, o1, .., ..) = Philox4x32-10(counter = (lo(counter), hi(counter), (uint32_t)n, 0x73687566), key = (lo(key), hi(key)))
 *   F(r, k0, k1):  p = (uint64_t)0xD2511F53 * (uint32_t)(r + k0);  t = hi(p) ^ lo(p) ^ k1;  q = (uint64_t)0xCD9E8D57 * t;  hi(q) ^ lo(q)
 *   E(x), a bijection of [0, 2^b): (wl, wr) = (a, c); for j = 0 .. 5: L = x >> wr, R = x & (2^wr - 1),
 *         x = (R << wl) | (L ^ (F(R, o0 + j * 0x9E3779B9, o1 + j * 0xBB67AE85) & (2^wl - 1))), then swap wl and wr
 *         (a 6-round Feistel network whose halves trade places and widths every round: unbalanced when b is odd)
 *   pi(i) = the first of E(i), E(E(i)), ... that is < n                                    (cycle walking; n = 1: pi(0) = 0)
 *   obs_dev / obs_out     [n, obs_dim] rows, float32 or float16 (obs_f16), aligned as for navppo_mlp64_loss_grad
 *   act_dev / act_out     [n, 2] f32, 8-byte aligned      logp_old_dev, rtg_dev, adv_dev and their outputs [n] f32
 *   gate_dev              nullable: the kl_state_dev [4] of the *_kl entry points -- gate_dev[0] != 0 (the update stopped): the kernel
 *                         returns at its entry and the outputs keep their contents
 * -1 and nothing launched: a null pointer (gate_dev aside), n_samples < 1 or >= 2^31, obs_dim not 16 or 42, a misaligned buffer, an
 * output that overlaps an input or another output.
 */
int navppo_shuffle_batch(const void* obs_dev, int32_t obs_dim /* 16 | 42 */, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                         const float* rtg_dev, const float* adv_dev, int64_t n_samples, uint64_t key, uint64_t counter, void* obs_out,
                         float* act_out, float* logp_out, float* rtg_out, float* adv_out, const float* gate_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Reward normalisation by a running variance of the discounted return (Stable-Baselines3's VecNormalize(norm_reward=True)): two entry
 * points that run IN FRONT of the return scan on the [T, N] buffers a rollout fills.  Both are asynchronous on `stream`, make no host
 * round trip and no device synchronisation, read nothing from the process environment and check their arguments before any HIP call
 * (-1 and nothing launched; message in navppo_last_error()).  float64 statistics throughout; navbot_ppo_amd.ppo.reward_norm_reference
 * is the host mirror of both.
 *
 * navppo_return_moments: per env column i the forward discounted return, in float64 --
 *     R = carry[i] (0 when carry_dev is NULL);  for t = 0 .. T - 1:  R = gamma R + rew[t, i];  R joins the batch;  R = 0 where ended[t, i]
 * -- afterwards carry[i] = R (if given: a rollout that continues passes the same buffer to its next call) and
 *     moments_dev [3] f64 = (n, mean, M2) of the T N values of R:  n = T N,  M2 = sum of (R - mean)^2
 * The column is split over T (chunks of 32 rows composed through float64 carries, as navsim_rtg_scan), so a value may differ from the
 * serial recurrence in its last float64 bits; the moments are combined with Chan's pairwise formula along one fixed tree (threads,
 * then workgroups, in index order; no floating-point atomics): the same input gives the same bits.
 *   rew_dev [T, N] f32   ended_dev [T, N] u8 (the layout navsim_rtg_scan takes)   carry_dev [N] f64, nullable, in / out
 * Refused: a null pointer (carry_dev aside), T < 1, N < 1, gamma outside [0, 1] (NaN included), rew_dev not 4-byte or
 * moments_dev / carry_dev not 8-byte aligned.  The workgroups' partial results pass through storage the library owns, one copy per
 * device: calls on ONE device must be ordered with each other (one stream, or streams that wait for each other).
 *
 * navppo_reward_scale: first merges rows k = 0 .. K - 1 of moments_dev [K, 3] f64 (each as navppo_return_moments writes it; K = 1 on
 * one GPU, one row per rank in rank order on several -- every rank then holds the same bits), in order, into the running statistics
 *   rms_dev [4] f64 = (mean, var, count, scale), in / out       (a fresh run: 0, 1, 1e-4, anything -- RunningMeanStd's start)
 *     d = bm - mean;  tot = count + bn;  mean += d bn / tot;  var = (var count + bM2 + d^2 count bn / tot) / tot;  count = tot
 * (a row with bn <= 0 or a non-finite bn, bm or bM2 is skipped and leaves the statistics as they are: one bad batch must not poison
 * them for good), then stores scale = 1 / sqrt(var + eps) to rms_dev[3] and writes
 *     rew_out[i] = clamp(float32(double(rew_in[i]) * scale), -clip, clip),  0 <= i < n          (a NaN reward stays NaN)
 * K = 0 scales with the statistics as they stand; n = 0 only merges; rew_out_dev may be rew_in_dev.  The bound is float32(clip).
 * Refused: rms_dev null, moments_dev null with K > 0, a reward pointer null with n > 0, K < 0, n < 0, eps negative or not finite,
 * clip not positive (+inf allowed), rms_dev / moments_dev not 8-byte or a reward pointer not 4-byte aligned.
 * Deviation from VecNormalize: it normalises step t with the statistics after step t; here the statistics take all T N returns of a
 * rollout at once and then scale the whole rollout.  The statistics after the rollout are the same (tests/test_reward_norm_cpu.py).
 */
int navppo_return_moments(const float* rew_dev, const uint8_t* ended_dev, int32_t T, int32_t N, double gamma, double* carry_dev,
                          double* moments_dev, void* stream);
int navppo_reward_scale(double* rms_dev, const double* moments_dev, int32_t K, const float* rew_in_dev, float* rew_out_dev, int64_t n,
                        double eps, double clip, void* stream);

/*
 * PPO.get_action() (ppo.py:673-706) for all envs of a shard in one launch: mean = actor(obs) (net_actor forward),
 * sample MVN(mean, var*I), clamp a0 to [0,1] and a1 to [-1,1] (ppo.py:700-703), log-prob of the CLAMPED action (:704).
 *   actor_params_dev [PA]   obs_dev [n,D] (f32 | f16)   act_dev [n,2] out   logp_dev [n] out   mean_dev [n,2] out, nullable
 *   noise_dev [n,2] standard normal draws, nullable: NULL = Philox4x32-10 keyed by (seed, env_id_base + i, step) +
 *   Box-Muller inside the kernel (the reference uses torch's global generator, unseeded by default: ppo.py:805-811);
 *   step = *step_base_dev (nullable = 0) + step_offset.  var_dev and step_base_dev are DEVICE scalars so that a
 *   captured hipGraph of T launches sees the current variance and a fresh noise stream on every replay.
 * The exploration-covariance decay of ppo.py:694-695 is the caller's (it changes `var` between launches).
 */
int navppo_mlp64_act(const float* actor_params_dev, const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* noise_dev,
                     int64_t n_envs, const float* var_dev, uint64_t seed, uint64_t env_id_base, const uint32_t* step_base_dev,
                     uint32_t step_offset, float* act_dev, float* logp_dev, float* mean_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * The reference's ACTIVE nets ("resmlp512"): NetActor / NetCritic (project_ppo/src/net_actor.py:56-144, net_critic.py:50-130),
 * two residual blocks ResBlock(16, 16) and ResBlock(32, 32) with 512 hidden units and LeakyReLU(0.2)
 * (net_actor.py:16-53), actor heads sigmoid(out1) / tanh(out2), critic head out.  Fused MFMA kernels (csrc/ppo_resmlp512.hip):
 * float32 in, float32 out, float32 accumulate; every matrix product except the weight gradients of the first block runs as float32
 * products rebuilt from three exact bf16 pieces per operand ("bf16x3", as navppo_mlp64_bf16x3_*; where a product contracts over 16
 * values only, two piece products share one MFMA), those run on the f32-input MFMA -- ONE arithmetic, also
 * for navppo_resmlp512_value (a caller who needs native float32 products throughout uses PyTorch: PPOConfig.update_arith = "f32").
 * Same contracts as the mlp64 entry points above unless stated.
 *
 *   params_dev  [50290 + 50257] f32   actor then critic, each in nn.Module.named_parameters() order WITHOUT the BatchNorm
 *               entries the reference's forward never uses (net_actor.py:44,48,137):
 *               rb1.fc1.weight[512,16], rb1.fc1.bias[512], rb1.fc2.weight[16,512], rb1.fc2.bias[16],
 *               rb2.fc1.weight[512,32], rb2.fc1.bias[512], rb2.fc2.weight[32,512], rb2.fc2.bias[32],
 *               out1.weight[1,32], out1.bias[1], out2.weight[1,32], out2.bias[1]      (critic: out.weight[1,32], out.bias[1])
 *   workspace_dev  navppo_resmlp512_workspace_bytes(n_samples) bytes (partial block outputs per hidden slice, 2.5 KB per
 *               sample, + partial-gradient rows); contents are scratch.
 */
#define NAVPPO_RESMLP512_ACTOR_PARAMS 50290
#define NAVPPO_RESMLP512_CRITIC_PARAMS 50257

size_t navppo_resmlp512_workspace_bytes(int64_t n_samples);

/* evaluate() + losses + both backward() calls of ppo.py:307-386; grad_dev [50290 + 50257], stats_dev [8] as navppo_mlp64_loss_grad.
 * obs_dev: [n, 16] rows, float32 (obs_f16 = 0) or float16 (obs_f16 = 1: BASELINE configs[4], navsim_cfg.obs_f16; ABI v6), 16-byte
 * aligned; half rows are widened as they are loaded, in every entry point below. */
int navppo_resmlp512_loss_grad(const float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                               const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip,
                               float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);

/* one whole epoch of ppo.py:305-392 on one GPU (losses, gradients, both Adam steps); as navppo_mlp64_update_epoch */
int navppo_resmlp512_update_epoch(float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                                  const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip, float lr,
                                  float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                  float* grad_dev, float* stats_dev, void* workspace_dev, void* stream);

/* navppo_resmlp512_update_epoch with clipping and the non-finite guard: see navppo_mlp64_update_epoch_clipped */
int navppo_resmlp512_update_epoch_clipped(float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                                          const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip, float lr,
                                          float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                          float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                          void* stream);

/* navppo_resmlp512_update_epoch_clipped with the early stop at a KL limit: see navppo_mlp64_update_epoch_kl */
int navppo_resmlp512_update_epoch_kl(float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                                     const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip, float lr,
                                     float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                     float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                     float kl_limit, float* kl_state_dev, void* stream);

/* navppo_resmlp512_update_epoch_clipped with the adaptive learning rate: see navppo_mlp64_update_epoch_lr */
int navppo_resmlp512_update_epoch_lr(float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                                     const float* rtg_dev, const float* adv_dev, int64_t n_samples, float var, float clip, float lr,
                                     float beta1, float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev,
                                     float* grad_dev, float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev,
                                     float kl_target, float lr_min, float lr_max, int32_t adapt, float* lr_state_dev, void* stream);

/* navppo_resmlp512_update_epoch_clipped / _lr with the learned exploration variance: see navppo_mlp64_update_epoch_var */
int navppo_resmlp512_update_epoch_var(float* params_dev, const void* obs_dev, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                                      const float* rtg_dev, const float* adv_dev, int64_t n_samples, float clip, float lr, float beta1,
                                      float beta2, float eps, int32_t step, float* adam_m_dev, float* adam_v_dev, float* grad_dev,
                                      float* stats_dev, void* workspace_dev, float max_norm, float* clip_stats_dev, float kl_target,
                                      float lr_min, float lr_max, int32_t adapt, float* lr_state_dev, float ent_coef, float var_min,
                                      float var_max, float* var_state_dev, void* stream);

/* V = critic(obs).squeeze() (ppo.py:275, :724); critic_params_dev [50257] (8-byte aligned suffices), value_dev [n] */
int navppo_resmlp512_value(const float* critic_params_dev, const void* obs_dev, int32_t obs_f16, int64_t n_samples, float* value_dev,
                           void* workspace_dev, void* stream);

/* PPO.get_action() (ppo.py:673-706) for all envs of a shard in one launch; arguments as navppo_mlp64_act, actor_params_dev [50290] */
int navppo_resmlp512_act(const float* actor_params_dev, const void* obs_dev, int32_t obs_f16, const float* noise_dev, int64_t n_envs,
                         const float* var_dev, uint64_t seed, uint64_t env_id_base, const uint32_t* step_base_dev,
                         uint32_t step_offset, float* act_dev, float* logp_dev, float* mean_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NAVPPO_H */
