/*
 * navsim.h -- C ABI of libnavsim.so: the MI355X (gfx950) batched LiDAR-navigation
 * simulator and return scan that replace the reference's Gazebo/ROS-backed
 * `Env.reset()/Env.step()` and `PPO.compute_rtgs()`.
 *
 * The reference exposes NO plugin / FFI / operator ABI for this path: its boundary is
 * a duck-typed Python class.  Each entry point below therefore cites
 * the reference *Python* interface it replaces; navbot_ppo_amd/env.py binds these with
 * ctypes and re-creates that Python surface (same names, argument meaning, error
 * behaviour).  INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; every function returns 0 on
 *     success or a negative NAVSIM_E_* code and never throws; navsim_last_error()
 *     gives the message for the calling thread.
 *   - `*_dev` pointers are DEVICE (HIP) pointers owned by the caller (e.g.
 *     torch.Tensor.data_ptr()); `*_host` pointers are host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 *     asynchronous and stream-ordered unless stated otherwise; no internal threads; a
 *     handle must not be used from two threads at once; distinct handles are independent.
 *   - there is no CPU fallback: without a HIP device every call that touches the
 *     device fails with NAVSIM_E_HIP.
 */
#ifndef NAVSIM_H
#define NAVSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAVSIM_ABI_VERSION 6

#define NAVSIM_OK 0
#define NAVSIM_E_ARG (-1)   /* bad argument / unsupported configuration */
#define NAVSIM_E_HIP (-2)   /* HIP runtime error (message has hipGetErrorString) */
#define NAVSIM_E_STATE (-3) /* call order: e.g. step before set_map */

typedef struct navsim navsim_t;

/*
 * Replaces the constructor arguments / module constants of the reference env:
 *   Env(is_training, ...)                    project_ppo/src/environment_new.py:27
 *   threshold_arrive 0.2 (train) / 0.4       environment_new.py:44-47
 *   max_timesteps_per_episode                project_ppo/src/ppo.py:552 (the caller-side timeout)
 *   spawn pose (0,0,0)                       turtlebot3_gazebo/launch/turtlebot3_stage_1.launch:3-5
 *   goal box U(-3.6,3.6)^2                   environment_new.py:337-338
 */
typedef struct navsim_cfg {
    int32_t n_envs;            /* N: envs simulated by this handle (one GPU's shard) */
    int32_t n_beams;           /* B: LiDAR samples (10 = reference, gazebo.xacro:111; 36 supported) */
    int32_t max_episode_steps; /* timeout in env steps; 0 = none */
    int32_t auto_reset;        /* 1: envs that end are reset inside step (ppo.py:582-593) and obs is the post-reset obs */
    int32_t respawn_on_arrive; /* 1: on arrival draw a new goal + re-base past_distance (environment_new.py:245-267) */
    int32_t obs_f16;           /* 1: obs buffers are IEEE half instead of float */
    int32_t lidar_below_min;   /* readings under range_min 0.12 m: 0 = clamp to 0.12 (default), 1 = -inf as Gazebo's ray sensor
                                  reports them; the reference passes -inf through unsanitised, which also suppresses the
                                  collision flag (environment_new.py:192-201) */
    float lidar_noise_sigma;   /* Gaussian range noise of the sensor (turtlebot3_burger.gazebo.xacro:122-126: 0.01); 0 = off
                                  (default, needed for bit-parity runs).  Applied to in-range readings, then clamped to
                                  [0.12, 3.5]; Philox keyed by (seed, env id, goal draws, episode step, beam) + Box-Muller */
    uint64_t seed;             /* Philox key */
    uint64_t env_id_base;      /* global id of env 0: RNG streams are keyed by (seed, env_id_base + i) */
    double threshold_arrive;
    double spawn_x, spawn_y, spawn_yaw;
    double goal_lo, goal_hi;
} navsim_cfg;

/* ABI / build info.  navsim_version() == NAVSIM_ABI_VERSION. */
int navsim_version(void);
const char* navsim_last_error(void);

/* Fills *cfg with the reference defaults (N=1, B=10, train threshold, stage_1 spawn and goal box). */
void navsim_default_cfg(navsim_cfg* cfg);

/* Env.__init__  (environment_new.py:27-47).  Allocates per-env state in HBM on the current device.  No entry point of the
 * library reads the process environment: everything a handle does follows from cfg, its map and navsim_set_shape, everything
 * a free function does from its arguments. */
int navsim_create(const navsim_cfg* cfg, navsim_t** out);
void navsim_destroy(navsim_t* h);

/*
 * Kernel-shape overrides of ONE handle (tests, A/B timing; no reference counterpart -- results never depend on them, every
 * shape writes the same rows).  envs_per_workgroup: 0 = the built-in rule (by shard size, beam count, map kind and entry
 * point), or 4 (navsim_rollout_mlp64 only) | 8 | 16 | 32 | 64.  pair_cast: -1 = the rule, 0 = 64-segment passes for every
 * map, 1 = 128-segment passes where the rule allows them.  Takes effect from the next launch.
 * With movers (navsim_set_movers) a forced shape applies to navsim_rollout_mlp64 ONLY, and only 32 or 64 do: every other stepping
 * entry point has the mover form in the 16-env shape alone and keeps it (step_epb / seq_epb stay 16 envs on 8 waves).
 */
int navsim_set_shape(navsim_t* h, int32_t envs_per_workgroup, int32_t pair_cast);

/*
 * What the handle is and which kernel instantiation each entry point would launch right now (a profile can then name the
 * kernel it timed).  `*_epb` = envs per workgroup, `*_waves` = waves per workgroup, `*_cast`: 0 = 64-segment passes,
 * 1 = 128-segment passes, 2 = 128-segment passes with non-temporal loads, 3 = tile bounding boxes.
 * rollout_kind: 0 = navsim_rollout_mlp64 unavailable for this handle, 1 = rollout_kernel (rollout_epb = 4 | 8 | 16 envs on 8
 * waves), 2 = rollout_big_kernel (rollout_epb = 64 envs on 16 waves, or 32 envs on 8 waves: tile-box maps on 4097..8192 envs and
 * the forced 32-env shape).  With movers: 1 = rollout_mov_kernel (16 envs on 8 waves), 2 = rollout_big_mov_kernel (the same shapes
 * under the same rule as without movers, rollout_cast 0 or 3) -- while step_* / seq_* keep reporting 16 envs on 8 waves.
 * forced_epb / forced_pair_cast: what navsim_set_shape was last given (0 / -1 = the rule).
 * The scan-history entry points (navsim_rollout_mlp64_hist, navsim_evaluate_mlp64_hist) always take 16 envs on 8 waves, in rounds of
 * workgroups beyond 4096 envs: a forced 32 / 64 shape does not apply to them and rollout_* does not describe them.
 */
typedef struct navsim_info {
    int32_t abi_version, n_envs, n_beams, obs_f16;
    int32_t n_segments, per_env_map, tile_boxes, has_map;
    int32_t forced_epb, forced_pair_cast;
    int32_t step_epb, step_waves, step_cast;       /* navsim_step */
    int32_t seq_epb, seq_waves, seq_cast;          /* navsim_step_seq */
    int32_t rollout_kind, rollout_epb, rollout_waves, rollout_cast;   /* navsim_rollout_mlp64 */
    /* resources of the selected step / tape instantiations as the loaded code object reports them (hipFuncGetAttributes):
       vector registers per lane, scratch bytes per lane (= spilled registers x 4; 0 = none), static LDS bytes per workgroup */
    int32_t step_vgprs, step_scratch_bytes, step_lds_bytes;
    int32_t seq_vgprs, seq_scratch_bytes, seq_lds_bytes;
    int32_t reserved[6];   /* reserved[0]: scan_pool (navsim_set_scan_pool; 1 = off) */
} navsim_info;
int navsim_get_info(navsim_t* h, navsim_info* out);

/*
 * Sector LiDAR -- an EXTENSION built on the reference's unused down-sampler (pick_laser.Pick(scan, len_batch): the minimum of
 * consecutive chunks of a denser scan).  scan_pool = k in 1..4, 1 = off (the default: today's behaviour, kernels and bits).  With
 * k > 1 on a 10-beam handle:
 *   dense fan     10 k rays, phi_i = A_min + i (A_max - A_min) / (10 k - 1): the beam angles of a handle with n_beams = 10 k.
 *   per ray       each dense ray goes through the sensor model on its own -- range limits, lidar_below_min, lidar_noise_sigma with
 *                 the noise keyed by the dense ray index i exactly as a 10 k-beam handle keys beam i (Gazebo's sensor, samples = 10 k).
 *   column c      min over the sanitised readings of rays k c .. k c + k - 1, divided by 3.5; a -inf reading (lidar_below_min) wins.
 *   collision     0 < min < 0.2 over all 10 k rays, i.e. over the 10 pooled columns.
 * So the pooled env IS the 10 k-beam env -- pose, goal draws, reward, flags, episode sums and RNG counters -- with its rows passed
 * through Pick(., k); columns 10..15, every row shape, net, history row and checkpoint are unchanged.  The pooled world is harder:
 * an obstacle that sat between two of the 10 beams (and was neither seen nor hit) is now seen, and hit.
 * Callable before or after navsim_set_map / navsim_set_movers / navsim_set_mover_bank, in any order, with the same resulting bits;
 * rebuilds the dense beam table and re-casts the cached spawn scans where a map is set; synchronises the device; takes effect from
 * the next launch (set it BEFORE a step is captured into a graph).  k = 1 restores exactly the kernels and bits of a fresh handle.
 * On a pooled handle every stepping entry point runs the pooled twin of the mover kernels' shape -- 16 envs on 8 waves, in rounds of
 * workgroups beyond 4096 envs, 64-segment passes or tile boxes; navsim_set_shape is accepted and has no effect; navsim_raycast
 * returns [N, 10] pooled noise-free scan values; navsim_get_info reports scan_pool in reserved[0], 16 / 8 / cast 0 | 3,
 * rollout_kind = 1 and the pooled twin's resources.
 * NAVSIM_E_ARG: k outside 1..4 (more than 4 rays per column is not built), and with k > 1: scan_pool > 1 needs n_beams == 10:
 * pooling a 36-beam scan is not built; scan_pool > 1 needs a shared static map: pooling over per-env maps is not built (a later
 * navsim_set_map(per_env = 1) on a pooled handle is refused likewise).  navsim_rollout_resmlp512 / navsim_evaluate_resmlp512 on a
 * pooled handle fail with NAVSIM_E_STATE: not built.
 */
int navsim_set_scan_pool(navsim_t* h, int32_t k);

/*
 * The static world the reference gets from Gazebo (worlds/train_world_new.world:85-416):
 * S line segments (ax,ay,bx,by) float32.  per_env=0: seg_dev is [S,4], shared by all envs;
 * per_env=1: seg_dev is [N,S,4], env i reads its own S segments.  The buffer is NOT copied:
 * it must stay alive and unchanged while the handle uses it.  (Exception: a shared map of 65..4096 segments is copied,
 * synchronously, into a handle-owned buffer in Morton order of the segment midpoints together with the bounding box of
 * every 64-segment tile, which lets the step kernel skip whole tiles; the order of segments does not affect any result.)  Also ray-casts the spawn pose
 * (the scan every reset observes) on `stream`.
 */
int navsim_set_map(navsim_t* h, const float* seg_dev, int32_t n_segments, int32_t per_env, void* stream);

/*
 * Moving obstacles -- an EXTENSION (the reference's worlds are static; its stated subject, mapless navigation in dynamic
 * environments, is not): a periodic TAPE of segments cast beside the static map by every step kernel.
 *   tape_dev   [period][n_segments][4] f32 (ax,ay,bx,by) as in navsim_set_map, 16-byte aligned, BORROWED like a per-env map (it must
 *              stay alive and unchanged while the handle uses it); 1 <= n_segments <= 64, 1 <= period <= 65536.  The kernels do no
 *              trajectory arithmetic: the host writes whatever motion it likes into the tape.  A segment with a NaN coordinate is
 *              never hit: the way to pad a phase that has fewer live segments.  NULL turns movers off: the handle then launches
 *              exactly what it launched before the first call.
 *   phase0_dev [N] i32, nullable (= all zero): per-env phase offset in [0, period).  Copied; validated on the host at this call.
 * Phase rule, k = env i's episode step counter before the step:
 *   a step's scan sees tape[(k + 1 + phase0[i]) mod period]; every reset observation (navsim_reset, the in-step auto-reset, the
 *   resets inside the persistent kernels) sees tape[phase0[i]] -- the batched form of Gazebo's reset_simulation, which puts every
 *   model back at its start.  navsim_raycast sees tape[(k + phase0[i]) mod period], the phase the env last observed.
 * Everything behind the scan -- collision rule, observation row, reward, episode logic -- is unchanged: a mover that reaches the robot
 * ends the episode as a wall does.  The scan equals, bit for bit, that of a static map holding the static segments and the phase's.
 * With a tape navsim_step, navsim_step_seq, navsim_rollout_resmlp512 and both evaluations run 16 envs on 8 waves per workgroup at
 * every shard size (navsim_set_shape has no effect on them).  navsim_rollout_mlp64 runs that shape up to 4096 envs and, as without
 * movers, 64 envs on 16 waves beyond (32 on 8 for tile-box maps up to 8192 envs), or the 32- / 64-env shape navsim_set_shape forces;
 * navsim_get_info reports the choice.  Every shape writes the same rows.
 * Like the map, the tape is part of the kernel arguments: set it BEFORE a step is captured into a graph.
 * Re-casts the spawn scans on `stream` (with phase0 they become per-env); a later navsim_set_map keeps the tape and does the same.
 * Synchronises `stream`.
 * NAVSIM_E_STATE before navsim_set_map.  NAVSIM_E_ARG: sizes or a phase0 value out of range, a misaligned tape, and: movers need 10
 * beams and a shared static map: movers with 36 beams or with a per-env static map are not built.
 */
int navsim_set_movers(navsim_t* h, const float* tape_dev, int32_t period, int32_t n_segments, const int32_t* phase0_dev,
                      void* stream);

/*
 * A BANK of tapes, one scenario per env, with per-tape goal rectangles.  navsim_set_movers IS this call with n_tapes = 1,
 * period[0] = period, no ids and no rectangles; a call of either replaces what the other set, bank_dev = NULL turns movers off.
 *   bank_dev        [n_tapes][max_period][n_segments][4] f32, 16-byte aligned, BORROWED like the tape.  n_segments <= 64,
 *                   max_period <= 65536, 1 <= n_tapes, n_tapes * max_period <= 2^24.  Rows period[k] .. max_period-1 of tape k are
 *                   never read; a tape with fewer segments is padded with NaN segments (never hit).
 *   period_host     [n_tapes] i32 on the HOST, 1 <= period[k] <= max_period.
 *   tape_id_dev     [N] i32, nullable (= all 0): the tape of env i, 0 <= id < n_tapes.  Copied; validated on the host at this call.
 *   phase0_dev      [N] i32, nullable (= all 0): 0 <= phase0[i] < period[tape_id[i]].  Copied; validated likewise.
 *   goal_rects_host [n_tapes][n_rects][4] f64 (xmin,xmax,ymin,ymax) on the HOST, nullable (= none), n_rects <= 8; a row with a NaN
 *                   entry is absent.  A uniform-box goal draw of env i (the reset draw and the arrival re-spawn draw) is rejected
 *                   if it lies in one of the handle's rectangles (navsim_set_goal_rects) OR in one of its tape's.  The draw stream,
 *                   the 64-try cap and the last-draw-kept rule are unchanged; with goal tables (navsim_set_spawn_sampler with
 *                   goals) they do not apply, as the handle's own do not.
 * Phase rule, k = env i's episode step counter before the step, t = tape_id[i]: a step's scan sees
 * bank[t][(k + 1 + phase0[i]) mod period[t]], a reset observation bank[t][phase0[i]], navsim_raycast
 * bank[t][(k + phase0[i]) mod period[t]]: the rule of navsim_set_movers with the period and the base row taken per env.
 * The tape of an env never changes between calls.  The spawn tables are per env as soon as ids or phases are given.
 * Everything else is as navsim_set_movers says (kernel shape, graphs, a later navsim_set_map, synchronises `stream`).
 * NAVSIM_E_STATE before navsim_set_map.  NAVSIM_E_ARG, with nothing changed on the handle: sizes out of range, a misaligned bank, an
 * id, a period or a phase out of range, n_rects outside 0..8 or rectangles without a pointer, and: movers need 10 beams and a shared
 * static map: movers with 36 beams or with a per-env static map are not built.
 */
int navsim_set_mover_bank(navsim_t* h, const float* bank_dev, int32_t n_tapes, int32_t max_period, int32_t n_segments,
                          const int32_t* period_host, const int32_t* tape_id_dev, const int32_t* phase0_dev,
                          const double* goal_rects_host, int32_t n_rects, void* stream);

/*
 * Goal-rejection rectangles (xmin,xmax,ymin,ymax; inclusive), host pointer, copied.
 * which=0: used by reset (environment_new.py:340-343); which=1: used by the arrival
 * re-spawn (environment_new.py:248-251).  Defaults are the reference's stage_1 values.
 * n_rects <= 16.  Synchronous.
 * Bound: the reference redraws until a goal is accepted (environment_new.py:340-345 loops forever on rectangles that
 * cover the goal box); the kernels draw at most 64 times and then keep the last draw.  With the stock rectangles
 * (18 % / 25 % of the box rejected) the chance of exhausting 64 draws is < 1e-38; rectangles covering more than ~70 %
 * of [goal_lo, goal_hi]^2 make accepted-after-64 goals inside a rectangle plausible (0.7^64 = 1e-10 per reset) -- keep
 * the rejected share below that or enlarge the goal box.
 */
int navsim_set_goal_rects(navsim_t* h, int32_t which, const double* rects_host, int32_t n_rects);

/*
 * GoalSpawnSampler  (project_ppo/src/spawn_goal_sampler.py:37-62; parsed as --use_external_sampler at arguments.py:41 but
 * never wired into the reference's Env): curated start poses [n_starts,3] (x,y,yaw) and goal points [n_goals,2], HOST
 * pointers, copied.  With n_goals > 0 every reset (and in-step auto-reset) picks a start pose and a goal uniformly from the
 * tables until min_dist <= |start - goal| <= max_dist (at most 100 attempts, then one unconditional pick) instead of the
 * fixed spawn pose + uniform goal box; n_goals == 0 keeps the uniform goal rule but resets to starts[0].  Re-casts the
 * scans of all start poses on `stream`.  Synchronous on `stream`.
 */
int navsim_set_spawn_sampler(navsim_t* h, const double* starts_host, int32_t n_starts, const double* goals_host,
                             int32_t n_goals, double min_dist, double max_dist, void* stream);

/*
 * Env.reset()  (environment_new.py:312-382), masked and batched: for every env i with
 * mask_dev[i] != 0 (all envs if mask_dev is NULL): pose <- spawn, goal <- sampled with the
 * reset rejection rule, past_distance <- distance to goal, episode counters <- 0,
 * past_action <- (0,0), and row i of obs_dev ([N, B+6]) <- the reset observation.
 * Rows of unmasked envs are not written.
 */
int navsim_reset(navsim_t* h, const uint8_t* mask_dev, void* obs_dev, void* stream);

/*
 * Env.step(action, past_action)  (environment_new.py:272-310) for all N envs:
 * action scaling (:273-278), 0.2 s of diff-drive motion, B-beam ray-cast, getOdometry
 * (:138-181), getState (:183-207), observation assembly (:289-301), setReward (:209-270),
 * plus the caller-side episode logic of PPO.rollout (ppo.py:543-593): episode step count,
 * timeout, and -- if cfg.auto_reset -- the masked reset.
 *
 *   action_dev       [N,2] f32  in   (a0 in [0,1] -> v=a0/4 m/s ; a1 in [-1,1] -> w rad/s)
 *   past_action_dev  [N,2] f32  in   nullable: NULL = the action of the previous step, (0,0)
 *                                    after a reset (ppo.py:543,591); non-NULL = Env.step's argument
 *   obs_dev          [N,B+6]    out  f32 (f16 if cfg.obs_f16): B lidar/3.5, past_action, dist/diag,
 *                                    yaw/360, rel_theta/360, diff_angle/180
 *   reward_dev       [N] f32    out
 *   done_dev         [N] u8     out  collision flag (0 < min(scan) < 0.2)
 *   arrive_dev       [N] u8     out  distance <= threshold_arrive
 *   ended_dev        [N] u8     out  nullable: done | arrive | timeout (the RTG episode-end flag)
 *   ep_return_dev    [N] f32    out  nullable: written only where ended: sum of the episode's rewards
 *   ep_length_dev    [N] i32    out  nullable: written only where ended: episode length in steps
 *   ep_path_dev      [N] f32    out  nullable: written only where ended: the episode's path length as PPO.rollout
 *                                    accumulates it (ppo.py:533-537: distances between the positions read BEFORE each
 *                                    step, so the last step's displacement is not part of it)
 *
 * Precision of the pose (what "identical" means for the float64 state): the motion model of turtlebot3_fake.cpp:154-163
 * integrates six 30 Hz sub-steps with one library sincos each.  The kernel evaluates the library sincos of the FINAL heading
 * (which also gives the sensor origin and the beam directions, i.e. everything the scan's bits depend on) and obtains the six
 * sub-step headings from it by angle addition, sums the sub-step displacements last-first and takes the step's path length
 * from the summed displacement.  x, y and the path length therefore agree with the serial integration to ~1e-16 per step
 * (relative 1e-15), not bit for bit; the heading itself (six additions of delta_theta) is bit-identical.  The tests hold the pose
 * to 1e-11 over hundreds of steps; observations and flags are compared separately (flags exactly, observations 1e-6, > 99 %
 * of the rows bit-identical -- a 1e-16 difference moves a float32 rounding or a decimal round() tie with probability ~1e-9).
 */
int navsim_step(navsim_t* h, const float* action_dev, const float* past_action_dev, void* obs_dev,
                float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, void* stream);

/*
 * Env attributes the reference's callers read or that tests / checkpoints need
 * (position.x/.y: ppo.py:535; goal_position, past_distance: environment_new.py:29-41).
 * HOST pointers, any of them may be NULL; SYNCHRONOUS (waits for `stream`).
 *   pose [N,3] f64 (x,y,theta) ; goal [N,2] f64 ; past_dist [N] f64 ; past_action [N,2] f32 ;
 *   ep_step [N] i32 ; rng_ctr [N] u32 (Philox draws consumed by env i)
 */
int navsim_get_state(navsim_t* h, double* pose_host, double* goal_host, double* past_dist_host,
                     float* past_action_host, int32_t* ep_step_host, uint32_t* rng_ctr_host, void* stream);
int navsim_set_state(navsim_t* h, const double* pose_host, const double* goal_host,
                     const double* past_dist_host, const float* past_action_host,
                     const int32_t* ep_step_host, const uint32_t* rng_ctr_host, void* stream);

/*
 * PPO.compute_rtgs()  (ppo.py:643-671) on the vectorised layout: rew_dev [T,N] f32,
 * ended_dev [T,N] u8 (last step of an episode), out_dev [T,N] f32:
 *   R[t,n] = rew[t,n] + gamma * (ended[t,n] ? 0 : R[t+1,n]),  R[T,n] = 0 (no bootstrap, ppo.py:601)
 * accumulated in float64 and stored as float32 like the reference (:665,:669).
 * N % 16 == 0 runs the scan split over T (chunk-local scans composed through float64 carries): every stored float32 is
 * within ONE ulp of the reference's serial recurrence (identical behind an episode end inside its 32-row chunk; elsewhere
 * a store differs with probability ~2e-8).  Any other N, or exact != 0, runs the serial recurrence: bit-identical, about 4x
 * slower.  (ABI v6: `exact` is an argument; up to v5 it was NAVSIM_RTG_EXACT in the process environment -- the library reads
 * nothing from the environment any more.)
 */
int navsim_rtg_scan(const float* rew_dev, const uint8_t* ended_dev, int32_t T, int32_t N, double gamma,
                    float* out_dev, int32_t exact, void* stream);

/*
 * Generalised advantage estimation -- the "GAE / return scan" BASELINE.json's north_star names; an EXTENSION: the reference
 * has only compute_rtgs (ppo.py:643-671) and A = rtgs - V (ppo.py:277), which is this scan at lambda = 1.  Off by default
 * (PPOConfig.gae_lambda = None).
 *   value_dev [T,N] f32 = V(s_t) of the stored observations; last_value_dev [N] f32, nullable: V of the state after the last
 *   row (NULL = the batch end is terminal, as in the reference, ppo.py:601,658); episode ends are always terminal (:552-553).
 *     R[t] = rew[t] + (ended[t] ? 0 : gamma (1 - lam) V[t+1] + gamma lam R[t+1])          float64 accumulate
 *     ret_dev [T,N] (nullable) = float32(R[t]) -- the lambda-return, the critic's target;   adv_dev [T,N] = float32(R[t]) - V[t]
 * lam = 1 and last_value_dev = NULL: ret_dev is bit-identical to navsim_rtg_scan's output and adv_dev to rtgs - V.  Same
 * kernel, same <= 1 ulp contract and the same `exact` / N % 16 rule as navsim_rtg_scan.
 */
int navsim_gae_scan(const float* rew_dev, const uint8_t* ended_dev, const float* value_dev, const float* last_value_dev, int32_t T,
                    int32_t N, double gamma, double lam, float* adv_dev, float* ret_dev, int32_t exact, void* stream);

/*
 * The truncation-aware form of navsim_gae_scan -- partial-episode bootstrapping (Pardo et al. 2018) by rsl_rl's rule; an EXTENSION,
 * off by default (PPOConfig.bootstrap_truncated = False).  The two scans above treat every episode end as terminal; an episode
 * that merely ran into max_episode_steps did not end for the robot, and regressing on "the return stops here" teaches the critic
 * a clock the observation does not hold.  A TIME-OUT is a row with ended set and neither done nor arrive (navppo_episode_sums'
 * definition); the value of the state behind it, which no buffer holds (the step kernels overwrite the terminal observation with
 * the reset one), is estimated by V of the row itself -- rsl_rl: rewards += gamma * values * time_outs.
 *   done_dev, arrive_dev [T,N] u8 as navsim_step / the rollouts write them; the other buffers as in navsim_gae_scan.
 * Per column, from the last row backwards, float64, the expressions as written (the library is built with -ffp-contract=off):
 *     trunc[t] = ended[t] && !done[t] && !arrive[t]
 *     add      = (double)rew[t] + (trunc[t] ? gamma * (double)V[t] : ended[t] ? 0.0 : gamma * (1 - lam) * (double)V[t+1])
 *     R[t]     = add + R[t+1] * (ended[t] ? 0.0 : gamma * lam)          V[T] = R[T] = last_value, or 0 when last_value_dev is NULL
 *     ret_dev [T,N] (nullable) = float32(R[t])     adv_dev [T,N] = float32(R[t]) - V[t]
 * Rows with done or arrive set but ended clear (respawn_on_arrive, handles without auto_reset) do not truncate.  What stays
 * terminal: collisions and arrivals, and the batch end unless last_value_dev bootstraps it.
 * Contract (that of the scans above): N % 16 == 0 and exact == 0 run the T-split kernel, every stored float32 within ONE ulp of the
 * serial recurrence and bit-identical to it on every row with ended set (the factor there is 0: the carry-in does not enter);
 * any other N, or exact != 0, runs the serial recurrence bit for bit.  With no time-out in the batch both outputs are bit-identical
 * to navsim_gae_scan's with the same arguments.  NAVSIM_E_ARG, before any HIP call: a negative size; (T, N > 0) a null rew / ended /
 * done / arrive / value / adv; lam outside [0, 1] (NaN included).  gamma is not checked.  T == 0 or N == 0: nothing to do, NAVSIM_OK.
 */
int navsim_gae_scan_trunc(const float* rew_dev, const uint8_t* ended_dev, const uint8_t* done_dev, const uint8_t* arrive_dev,
                          const float* value_dev, const float* last_value_dev, int32_t T, int32_t N, double gamma, double lam,
                          float* adv_dev, float* ret_dev, int32_t exact, void* stream);

/*
 * The hot loop of PPO.rollout (project_ppo/src/ppo.py:505-594) for the (B + 6)-64-64 policy, all n_steps steps in ONE launch:
 * per step PPO.get_action (ppo.py:673-706; what navppo_mlp64_act computes, include/navppo.h) followed by what navsim_step
 * computes, for every env, with the rows of step t written at offset t * N of each [n_steps, N, .] buffer.  A workgroup
 * keeps its envs for the whole rollout, so there is no kernel boundary and no observation round trip between steps; the
 * results are bit-identical to n_steps pairs of navppo_mlp64_act / navsim_step calls with the same seeds.
 *   actor_params_dev [NAVPPO_MLP64_ACTOR_PARAMS_D(B + 6)] f32  the actor in the layout of navppo.h (10 beams: 5378, 36: 7042)
 *   obs_buf_dev  [n_steps + 1, N, B + 6] f32 (f16 if cfg.obs_f16)   row 0 in: the observations the rollout starts from
 *                (navsim_reset); rows 1.. out.  With f16 buffers the policy reads every row as a reader of the buffer would:
 *                rounded to half (so the rows still equal the per-step path's bit for bit).
 *   act_buf_dev  [n_steps, N, 2]   logp_buf_dev [n_steps, N]   reward_dev [n_steps, N]   done / arrive / ended [n_steps, N] u8
 *   ep_return_dev / ep_length_dev / ep_path_dev  [n_steps, N], nullable, written where ended (as in navsim_step)
 *   var_dev  device scalar: exploration variance (ppo.py:123-124)
 *   act_seed, step_base_dev (device scalar, nullable = 0): action noise = Philox(act_seed, env id, *step_base_dev + t)
 * Workgroup shapes, same rows bit for bit: 16 envs on 8 waves (a latency chain per workgroup, one round of workgroups up to
 * 4096 envs; 64-segment passes, or tile boxes on shared 65..4096-segment maps; the only shape with 36 beams) and, with 10 beams
 * beyond 4096 envs per GPU, 64 envs on 16 waves with the cast variants of navsim_step (tile boxes, 128-segment passes of per-env
 * maps) -- 32 envs on 8 waves for tile-box maps on 4097..8192 envs: the closed-loop form of navsim_step_seq (navsim_set_shape:
 * 4 | 8 | 16 | 32 | 64 forces a shape; navsim_get_info reports the one a launch would take).  params_dev and obs_buf_dev must be
 * 16-byte aligned, act_buf_dev 8-byte (NAVSIM_E_ARG otherwise).
 */
int navsim_rollout_mlp64(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev,
                         float* logp_buf_dev, float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                         float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev,
                         uint64_t act_seed, const uint32_t* step_base_dev, int32_t n_steps, void* stream);

/*
 * The same hot loop (ppo.py:505-594) with the reference's ACTIVE actor choosing every action in the kernel: NetActor
 * (project_ppo/src/net_actor.py:56-144 -- two residual blocks of 512 hidden units, LeakyReLU(0.2), heads sigmoid / tanh), i.e. per
 * step what navppo_resmlp512_act computes (include/navppo.h) followed by what navsim_step computes, all n_steps steps in ONE launch;
 * buffers, noise keys and bit-for-bit equality with the per-step entry points as for navsim_rollout_mlp64.
 *   actor_params_dev [NAVPPO_RESMLP512_ACTOR_PARAMS = 50290] f32, the layout of navppo.h (no BatchNorm entries)
 *   obs_buf_dev [n_steps + 1, N, 16] f32 (f16 if cfg.obs_f16: the policy then reads every row rounded to half, as a reader of the
 *               buffer would -- the rows still equal the per-step path's bit for bit).   Needs n_beams == 10.
 * 16 envs on 8 waves per workgroup at every shard size (each wave owns 64 hidden units; the 197 KB of weights stream from L2 every
 * step), 64-segment passes for every map (no tile boxes: correct on every map, the house map just tests all its tiles).
 */
int navsim_rollout_resmlp512(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev, float* logp_buf_dev,
                             float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev, float* ep_return_dev,
                             int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev, uint64_t act_seed,
                             const uint32_t* step_base_dev, int32_t n_steps, void* stream);

/*
 * The evaluation loop (project_ppo/src/main.py:135-252) for the (B + 6)-64-64 actor in ONE launch: the workgroup of
 * navsim_rollout_mlp64 (16 envs on 8 waves, env state and observation tile on chip) with the DETERMINISTIC action
 * a = (clamp(mu0, 0, 1), clamp(mu1, -1, 1)) (main.py:197-199: no noise is drawn, no log-prob computed), no [n_steps, N, .] rows,
 * and an episode quota kept on chip: every env plays its episodes back to back (auto_reset) and the first `quota` of them are
 * recorded, one record each, in slot 0, 1, .. of the episode table; later episodes of that env are simulated but not recorded.
 * A workgroup leaves the step loop once all its envs have met the quota, at the latest after n_steps steps.
 *   actor_params_dev  as for navsim_rollout_mlp64
 *   obs0_dev      [N, B + 6] f32 (f16 if cfg.obs_f16): the observations the episodes start from (navsim_reset), read as
 *                 navsim_rollout_mlp64 reads row 0 of its obs_buf_dev
 *   quota >= 1, n_steps >= 1 (quota * max_episode_steps is always enough: every episode ends by its time-out)
 *   ep_flags_dev  [quota, N] u8   bit 0 success (arrive), bit 1 collision (done and not arrive), bit 2 timeout (ended, neither)
 *   ep_length_dev [quota, N] i32  ep_return_dev [quota, N] f32   ep_path_dev [quota, N] f32   as navsim_step's ep_* outputs
 *   count_dev     [N] i32         episodes recorded for env i (== quota unless n_steps ran out)
 *   steps_dev     [ceil(N / 16)] i32   env steps workgroup k (envs 16 k .. 16 k + 15) executed before it left the loop
 * Slots that were not reached keep what the caller put there.  Every record is bit-identical to what a loop of navppo_mlp64_act
 * (noise_dev = zeros) / navsim_step calls yields.  The handle's env state is written back after the loop as by the rollouts, but
 * is otherwise unspecified (the envs kept running after their quota): call navsim_reset before the handle is used again.
 * NAVSIM_E_ARG, before anything is launched: a null handle or pointer, quota < 1, n_steps < 1, a handle without auto_reset or
 * with max_episode_steps == 0 (an episode could never end), more than 4096 envs (only the 16-env workgroup shape has an
 * evaluation form; navsim_set_shape has no effect here), n_beams other than 10 or 36, actor_params_dev / obs0_dev not 16-byte
 * aligned.  The tile-box cast and the sensor-fidelity options are picked as for the rollout.
 */
int navsim_evaluate_mlp64(navsim_t* h, const float* actor_params_dev, const void* obs0_dev, int32_t quota, int32_t n_steps,
                          uint8_t* ep_flags_dev, int32_t* ep_length_dev, float* ep_return_dev, float* ep_path_dev,
                          int32_t* count_dev, int32_t* steps_dev, void* stream);

/*
 * The same with the reference's ACTIVE actor (NetActor, two residual blocks of 512 hidden units): the workgroup of
 * navsim_rollout_resmlp512, records bit-identical to a loop of navppo_resmlp512_act (noise_dev = zeros) / navsim_step calls.
 * Arguments, outputs and errors as for navsim_evaluate_mlp64; actor_params_dev as for navsim_rollout_resmlp512; needs
 * n_beams == 10 (NAVSIM_E_ARG otherwise).
 */
int navsim_evaluate_resmlp512(navsim_t* h, const float* actor_params_dev, const void* obs0_dev, int32_t quota, int32_t n_steps,
                              uint8_t* ep_flags_dev, int32_t* ep_length_dev, float* ep_return_dev, float* ep_path_dev,
                              int32_t* count_dev, int32_t* steps_dev, void* stream);

/*
 * SCAN HISTORY -- an EXTENSION: the policy sees the last three 10-beam scans instead of one.  A HISTORY ROW has 42 columns, every
 * one a copy of a value of the last three ordinary 16-column rows (row_t = what navsim_step / navsim_reset write: 10 beams / 3.5,
 * past_action (2), 4 goal columns):
 *     0..15   row_t[0:16]       the ordinary row, unchanged
 *     16..25  row_{t-1}[0:10]   the previous scan
 *     26..35  row_{t-2}[0:10]
 *     36..37  row_{t-1}[10:12]  the action between the two older scans (ego motion against obstacle motion)
 *     38..41  0
 * The episode cut: with r(t) the latest row index s <= t such that s == 0 or ended[s-1] != 0, row_{t-j} means
 * row_{max(t-j, r(t))}.  On an episode's first row all three frames are that row's scan and columns 36..37 its past_action (zeros
 * after a reset); a zero-filled frame would read as "obstacle at distance 0" in this normalisation.  Row 0 of a buffer counts as an
 * episode start for navsim_stack_rows, navsim_rollout_mlp64_hist and navsim_evaluate_mlp64_hist; a caller that continues episodes
 * across launches hands the history over the seam with the *_cont entry points below (the HISTORY CARRY) and loses nothing.  With
 * float16 rows every copy is a copy of the half value.  Nothing is recomputed, so everything below is exact.
 *
 * navsim_stack_rows builds the history rows of a whole buffer; it takes no handle.
 *   obs_dev   [R, N, 16] f32 (f16 if obs_f16 != 0)   rows as navsim_rollout_mlp64's obs_buf_dev holds them
 *   ended_dev [R - 1, N] u8   ended_dev[t] is the flag of the step between rows t and t + 1; NULL allowed when R == 1
 *   out_dev   [R, N, 42]      the type of obs_dev
 * Called on the three-row window t-2..t of a stepping loop (R = 3; shorter at the start) its LAST output row is the history row of
 * row t, whatever lies in front of the window: the rule never looks further back than two rows.
 * NAVSIM_E_ARG: R < 1, N < 1, a null obs_dev / out_dev, a null ended_dev with R > 1, obs_dev or out_dev not 16-byte aligned.
 */
int navsim_stack_rows(const void* obs_dev, int32_t obs_f16, const uint8_t* ended_dev, int32_t R, int32_t N, void* out_dev,
                      void* stream);

/*
 * navsim_rollout_mlp64 with the 42-64-64 actor (NAVPPO_MLP64_ACTOR_PARAMS_D(42) = 7042 parameters) reading the history row of
 * every step, assembled on chip: the two older scans and the older action pair of a workgroup's envs stay in LDS.  The argument
 * list and every buffer are navsim_rollout_mlp64's: obs_buf_dev stays [n_steps + 1, N, 16] -- the env side is bit-identical to the
 * 16-column rollout's for the same actions, navsim_step_seq replays it -- and row 0 counts as an episode start.  The results are
 * bit-identical to n_steps rounds of navsim_stack_rows (on the last three rows) / navppo_mlp64_act (obs_dim = 42) / navsim_step.
 * Needs n_beams == 10 (NAVSIM_E_ARG otherwise).  Always 16 envs on 8 waves per workgroup, in rounds of workgroups beyond 4096 envs:
 * navsim_set_shape has no effect, and the rollout_* fields of navsim_get_info describe navsim_rollout_mlp64, not this entry point.
 * Both cast variants of that shape, the sensor-fidelity options, float16 rows, a tape or a bank of tapes are covered.
 */
int navsim_rollout_mlp64_hist(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev,
                              float* logp_buf_dev, float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                              float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev,
                              uint64_t act_seed, const uint32_t* step_base_dev, int32_t n_steps, void* stream);

/*
 * Continuing across launches.  The HISTORY CARRY of a row is [N, 22] f32, 16-byte aligned: columns 16..37 of the row's history row,
 *     0..9    the scan of row t-1        10..19  the scan of row t-2        20..21  past_action of row t-1
 * each already clamped to the episode's first row by the rule above (on an episode's first row: the row's own scan, twice, and its
 * own past_action), with float16 rows the half values held as float.  The cut is inside the values, so whoever consumes a carry needs
 * no "did row 0 start an episode" flag.  k launches of T steps chained through carries (row T of one launch's obs_buf copied to row 0
 * of the next, step_base advanced by T, the handle untouched in between) write the bits ONE launch of k T steps writes.
 *
 * navsim_rollout_mlp64_hist_cont: navsim_rollout_mlp64_hist plus
 *   hist_in_dev   nullable: the carry of obs_buf_dev's row 0 (NULL = row 0 starts every env's episode, as navsim_rollout_mlp64_hist)
 *   hist_out_dev  nullable: receives the carry of row n_steps (the row behind the last step)
 * The two may be one buffer: a workgroup reads its envs' entries before its first step and writes them after its last.  Both NULL:
 * the bits of navsim_rollout_mlp64_hist.  NAVSIM_E_ARG, before anything is launched: whatever navsim_rollout_mlp64_hist refuses, a
 * carry that is not 16-byte aligned, and n_steps == 0 with a hist_out_dev that is not hist_in_dev (no row to write a carry for).
 *
 * navsim_stack_rows_cont: navsim_stack_rows plus
 *   carry_in_dev   nullable: the carry of obs_dev's row 0.  Output row 0's columns 16..37 are the carry; row 1 takes its oldest frame
 *                  (columns 26..35) from the carry's entries 0..9 unless ended_dev[0] is set; rows 2.. are navsim_stack_rows's.
 *   carry_out_dev  nullable: receives columns 16..37 of output row R - 1 as float -- the carry of that row, i.e. of row 0 of the
 *                  buffer that continues there (written by a second, N x 22-element launch behind the first: may be carry_in_dev)
 * Both NULL: the bits of navsim_stack_rows.  NAVSIM_E_ARG: whatever navsim_stack_rows refuses, a carry that is not 16-byte aligned.
 */
int navsim_rollout_mlp64_hist_cont(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev,
                                   float* logp_buf_dev, float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                                   float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev,
                                   uint64_t act_seed, const uint32_t* step_base_dev, int32_t n_steps, const float* hist_in_dev,
                                   float* hist_out_dev, void* stream);
int navsim_stack_rows_cont(const void* obs_dev, int32_t obs_f16, const uint8_t* ended_dev, int32_t R, int32_t N, void* out_dev,
                           const float* carry_in_dev, float* carry_out_dev, void* stream);

/*
 * navsim_evaluate_mlp64 with the 42-64-64 actor on history rows, as navsim_rollout_mlp64_hist: obs0_dev stays [N, 16] and counts as
 * every env's episode start.  Arguments, outputs and errors as for navsim_evaluate_mlp64, except that n_beams must be 10; every
 * record is bit-identical to a loop of navsim_stack_rows / navppo_mlp64_act (obs_dim = 42, noise_dev = zeros) / navsim_step calls.
 */
int navsim_evaluate_mlp64_hist(navsim_t* h, const float* actor_params_dev, const void* obs0_dev, int32_t quota, int32_t n_steps,
                               uint8_t* ep_flags_dev, int32_t* ep_length_dev, float* ep_return_dev, float* ep_path_dev,
                               int32_t* count_dev, int32_t* steps_dev, void* stream);

/*
 * n_steps calls of navsim_step with the actions of a tape, in ONE launch: the step loop of PPO.rollout (ppo.py:505-594) or of the
 * evaluation loop (main.py:176-235) when the actions do not depend on the observations being produced -- a recorded tape, a
 * scripted or random policy, an open-loop controller.  A workgroup keeps its envs for the whole tape (their state stays on chip
 * between the steps), so the launch ramp, the state round trips and the kernel boundaries of n_steps launches are paid once.
 *   actions_dev [n_steps, N, 2] f32 (8-byte aligned); row t is the `action_dev` of step t (past_action = the action executed before)
 *   obs_dev     [n_steps, N, B+6] f32 (f16 if cfg.obs_f16): the observation AFTER step t, as navsim_step writes it
 *   reward_dev / done_dev / arrive_dev / ended_dev (nullable)  [n_steps, N]
 *   ep_return_dev / ep_length_dev / ep_path_dev  [n_steps, N], nullable, written where ended (as in navsim_step)
 * Every row is bit-identical to what n_steps navsim_step calls write; the handle's state afterwards is the same too.
 */
int navsim_step_seq(navsim_t* h, const float* actions_dev, int32_t n_steps, void* obs_dev, float* reward_dev, uint8_t* done_dev,
                    uint8_t* arrive_dev, uint8_t* ended_dev, float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev,
                    void* stream);

/*
 * Env.getOdometry()  (environment_new.py:138-181) on its own, for n independent samples -- the odometry callback's arithmetic
 * exactly as the reference runs it, general quaternion included (the step kernel applies the same device functions to the
 * yaw-only quaternion of its planar pose):
 *   yaw        = round(degrees(atan2(2 (qx qy + qw qz), 1 - 2 (qy^2 + qz^2)))), + 360 if negative        (:142-147)
 *   rel_theta  = round(degrees(8-case quadrant angle of round(goal - pos, 1)), 2)                           (:149-169)
 *   diff_angle = round(wrap(yaw - rel_theta) to [-180, 180], 2)                                              (:170-176)
 * x_dev, y_dev [n] f64; quat_dev [n,4] f64 (qx, qy, qz, qw); goal_dev [n,2] f64; out_dev [n,3] f64 (yaw, rel_theta,
 * diff_angle).  Python round() semantics (half to even on the decimal value) are reproduced exactly.
 */
int navsim_odometry(int32_t n, const double* x_dev, const double* y_dev, const double* quat_dev, const double* goal_dev,
                    double* out_dev, void* stream);

/* LiDAR only (no state change): ranges_dev [N,B] f32 raw scan (inf = no return) for poses
 * pose_dev [N,3] f64.  Used by tests and by map tooling (spawn_goal_sampler-style validation). */
int navsim_raycast(navsim_t* h, const double* pose_dev, float* ranges_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NAVSIM_H */
