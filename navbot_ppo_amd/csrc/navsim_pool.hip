// navsim_pool.hip -- the sector-LiDAR twins (navsim_set_scan_pool, include/navsim.h "Sector LiDAR"): a handle with scan_pool = k
// casts 10 k rays and min-pools k consecutive ones into each of the 10 scan columns (the reference's pick_laser.Pick on a denser
// scan), so every row, net, history row and checkpoint keeps its shape.
//
// The kernels are navsim.hip's own text compiled a second time (NAVSIM_POOL_TU: everything up to and including the persistent
// bodies; the small kernels, the scans and the host side are compiled out) with step_body's POOL flag on, in a translation unit of
// their own: navsim.hip's kernels keep their symbols and their listings, and its build time stays what it was.  One form:
//   - k is a run-time count (Params::pool; arrays sized for kMaxPool = 4): one instantiation serves k = 2, 3, 4;
//   - the sensor-options form only (as kMovSens: with the options off it computes the same bits);
//   - the mover form only: a handle without a tape runs it over the handle's one-row tape of one absent (NaN) segment, which the
//     cull drops before any test;
//   - 10 columns, 16 envs on 8 waves, a shared static map: the shape and the restrictions of the mover twins; stage B takes the
//     entries of the 36-beam path (kPairB) on the 20 .. 40 rays.
// What is left here are the kernels' names, the pooled reset / ray-cast kernels and the resolver navsim.hip asks.
#define NAVSIM_POOL_TU 1
#include "navsim.hip"
#include "navsim_pool.h"

namespace {

using KPRef = const Params __attribute__((address_space(4)))&;
using KIORef = const StepIO __attribute__((address_space(4)))&;

template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void step_pool_mov_kernel(StepKArgs) {
    __shared__ StepSmemMov<10, 16, 8, true> sm;
    __shared__ int next_env;
    StepKArgsPtr A = (StepKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(A));
    step_body<10, 16, true, false, 8, BOXES, 0, KPRef, KIORef, NoHook, true, true>(A->P, sm, next_env, A->io);
}

template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void steps_pool_mov_kernel(SeqKArgs) {
    __shared__ StepSmemMov<10, 16, 8, true> sm;
    __shared__ int next_env;
    steps_body<10, 16, true, 8, BOXES, 0, true, true>(sm, next_env);
}

template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void rollout_pool_mov_kernel(Params P, RolloutArgs R) {
    using PL = mlp64::Layout<16>;
    __shared__ StepSmemMov<10, 16, 8, true> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ float2 pol_eps[16];
    __shared__ unsigned pol_cnt;
    rollout_body<10, 16, true, 8, BOXES, true, false, true>(P, R, sm, next_env, wts, pol_z, pol_eps, pol_cnt);
}

template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void rollout_hist_pool_mov_kernel(Params P, RolloutArgs R) {
    using PL = mlp64::Layout<kHistD>;
    __shared__ StepSmemMov<10, 16, 8, true> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ float2 pol_eps[16];
    __shared__ unsigned pol_cnt;
    __shared__ float hist[16 * kHistStride];
    rollout_body<10, 16, true, 8, BOXES, true, true, true>(P, R, sm, next_env, wts, pol_z, pol_eps, pol_cnt, hist);
}

template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void evaluate_pool_mov_kernel(Params P, EvalArgs R) {
    using PL = mlp64::Layout<16>;
    __shared__ StepSmemMov<10, 16, 8, true> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ unsigned pol_cnt;
    __shared__ int ep_cnt[16];
    evaluate_body<10, true, BOXES, true, false, true>(P, R, sm, next_env, wts, pol_z, pol_cnt, ep_cnt);
}

template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void evaluate_hist_pool_mov_kernel(Params P, EvalArgs R) {
    using PL = mlp64::Layout<kHistD>;
    __shared__ StepSmemMov<10, 16, 8, true> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ unsigned pol_cnt;
    __shared__ int ep_cnt[16];
    __shared__ float hist[16 * kHistStride];
    evaluate_body<10, true, BOXES, true, true, true>(P, R, sm, next_env, wts, pol_z, pol_cnt, ep_cnt, hist);
}

// ---------------------------------------------------------------- reset (Env.reset, masked) on a pooled handle
// reset_kernel with the scan of the dense fan: the spawn-scan row holds the raw hits of all B * pool rays, each goes through the
// sensor model with the noise of its own ray index (the key a handle with B * pool beams gives beam i), column c is the minimum of
// its `pool` readings.
__global__ void reset_pool_kernel(Params P, const uint8_t* __restrict__ mask, void* __restrict__ obs_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    if (mask && !mask[i]) return;
    const int B = P.B, D = B + 6, pool = P.pool, NC = B * pool;
    uint32_t ctr = P.rng_ctr[i];
    double gx, gy, yaw, rel_theta, diff;
    int k0;
    sample_episode<const Params&, true>(P, *P.rects, i, ctr, k0, gx, gy);
    const double x = P.starts[3 * k0], y = P.starts[3 * k0 + 1], th = P.starts[3 * k0 + 2];
    goal_angles(x, y, th, gx, gy, yaw, rel_theta, diff);
    const double dist = hypot(gx - x, gy - y);
    const float* sp = P.spawn_scan + ((P.spawn_per_env ? (size_t)i * P.K : 0) + k0) * NC;   // raw hits of the dense fan
    const uint64_t gid = P.env_id_base + (uint64_t)i;
    auto lidar = [&](int c) {
        float mn = INFINITY;
        for (int j = 0; j < pool; ++j) {
            const int b = pool * c + j;
            const float n = (P.sigma > 0.f) ? lidar_noise(P.key0, P.key1, gid, ctr, 0xFFFFu, b) : 0.f;
            float r = sensor_value(sp[b], P.sigma, n, P.below_min_mode);
            if (r == INFINITY) r = 3.5f;  // environment_new.py:193-194
            mn = r < mn ? r : mn;
        }
        return mn / 3.5f;                 // :362
    };
    const float tail[6] = {0.f, 0.f, (float)(dist / P.diag), (float)(yaw / 360), (float)(rel_theta / 360), (float)(diff / 180)};
    if (P.obs_f16) {
        __half* o = reinterpret_cast<__half*>(obs_out) + (size_t)i * D;
        for (int c = 0; c < B; ++c) o[c] = __float2half_rn(lidar(c));
        for (int k = 0; k < 6; ++k) o[B + k] = __float2half_rn(tail[k]);
    } else {
        float* o = reinterpret_cast<float*>(obs_out) + (size_t)i * D;
        for (int c = 0; c < B; ++c) o[c] = lidar(c);
        for (int k = 0; k < 6; ++k) o[B + k] = tail[k];
    }
    P.x[i] = x; P.y[i] = y; P.th[i] = th;
    P.gx[i] = gx; P.gy[i] = gy; P.past_dist[i] = dist;
    P.past_action[i] = make_float2(0.f, 0.f);
    P.ep_step[i] = 0;   // also clears kRecValid: the goal stream moved
    P.ep_ret[i] = 0;
    P.ep_path[i] = 0;
    P.rng_ctr[i] = ctr;
}

// ---------------------------------------------------------------- LiDAR only on a pooled handle (spawn scans, navsim_raycast)
// raycast_kernel over the dense fan.  raw (the spawn-scan table): the nearest hit of each of the B * pool rays, [n][B * pool].
// Else (navsim_raycast): [n][B] -- the minimum over each column's `pool` noise-free scan values (a -inf reading wins).
__global__ void raycast_pool_kernel(Params P, const double* __restrict__ pose, int n_poses_per_env, int shared_poses, int n,
                                    int raw, float* __restrict__ ranges) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int env = t / n_poses_per_env;
    const size_t pi = shared_poses ? (size_t)(t % n_poses_per_env) : (size_t)t;
    const double x = pose[pi * 3 + 0], y = pose[pi * 3 + 1], th = pose[pi * 3 + 2];
    const double cth = cos(th), sth = sin(th);
    const float ox = (float)(x + kLidarX * cth), oy = (float)(y + kLidarX * sth);
    const float4* __restrict__ sp = P.seg + (P.per_env ? (size_t)env * P.S : 0);
    const float4* __restrict__ mv = nullptr;
    if (P.mov_tape) {
        const uint32_t k = shared_poses ? 0u : ((uint32_t)P.ep_step[env] & kStepMask);
        mv = P.mov_tape + (size_t)mover_row(mover_bp<const Params&>(P, env), k, P.mov_phase0 ? (uint32_t)P.mov_phase0[env] : 0u) * (size_t)P.mov_M;
    }
    const int n_mov = mv ? P.mov_M : 0;
    const int pool = P.pool, NC = P.B * pool;
    float mn = INFINITY;
    for (int b = 0; b < NC; ++b) {
        const double bc = P.beam_cs[b], bs = P.beam_cs[NC + b];
        const float c = (float)(cth * bc - sth * bs);
        const float s = (float)(sth * bc + cth * bs);
        float best = INFINITY;
        for (int j = 0; j < P.S + n_mov; ++j) {
            const float4 g = (j < P.S) ? sp[j] : mv[j - P.S];
            const float rx = g.x - ox, ry = g.y - oy;
            const float ex = g.z - g.x, ey = g.w - g.y;
            const float k = fmaf(rx, ey, -(ry * ex));
            const float tt = ray_seg(rx, ry, ex, ey, k, c, s);
            best = tt < best ? tt : best;
        }
        if (raw) {
            ranges[(size_t)t * NC + b] = best;
        } else {
            const float r = sensor_value(best, 0.f, 0.f, P.below_min_mode);
            mn = r < mn ? r : mn;
            if (b % pool == pool - 1) {
                ranges[(size_t)t * P.B + b / pool] = mn;
                mn = INFINITY;
            }
        }
    }
}

}  // namespace

namespace navsim_pool {

const void* resolve(const int kernel, const bool boxes) {
    switch (kernel) {
        case kStep: return boxes ? (const void*)step_pool_mov_kernel<true> : (const void*)step_pool_mov_kernel<false>;
        case kSteps: return boxes ? (const void*)steps_pool_mov_kernel<true> : (const void*)steps_pool_mov_kernel<false>;
        case kRollout: return boxes ? (const void*)rollout_pool_mov_kernel<true> : (const void*)rollout_pool_mov_kernel<false>;
        case kRolloutHist: return boxes ? (const void*)rollout_hist_pool_mov_kernel<true> : (const void*)rollout_hist_pool_mov_kernel<false>;
        case kEvaluate: return boxes ? (const void*)evaluate_pool_mov_kernel<true> : (const void*)evaluate_pool_mov_kernel<false>;
        case kEvaluateHist: return boxes ? (const void*)evaluate_hist_pool_mov_kernel<true> : (const void*)evaluate_hist_pool_mov_kernel<false>;
        case kReset: return (const void*)reset_pool_kernel;
        case kRaycast: return (const void*)raycast_pool_kernel;
    }
    return nullptr;
}

}  // namespace navsim_pool
