// ppo_learned_var.hip -- the step of the learned exploration variance (include/navppo.h "Learned exploration variance"): the last launch
// of every *_var epoch, behind the nets' clip / step launch.
//
// The policy is MVN(mean, var I) with ONE variance; theta = log var is a parameter of the actor.  The pass twins (ppo_mlp64_var.hip,
// ppo_resmlp512_var.hip) leave per workgroup the sum of dL_dlp_i (1/2 (d0^2 + d1^2)_i / var - 1) in their statistics row; here ONE
// workgroup adds those rows in a fixed order and one thread takes Adam's step on theta -- a scalar, so there is nothing to spread over
// a grid, and a single workgroup needs no slot scheme: the state it writes is read by the NEXT call's launches only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "navppo_internal.h"

namespace {

constexpr int kVarThreads = 256;

__global__ __launch_bounds__(kVarThreads) void var_step_kernel(const float* __restrict__ col, int n_rows, int row_pitch,
                                                               const float* __restrict__ clip_stats, const float* __restrict__ lr_state,
                                                               float lr, float beta1, float beta2, float eps, float bc1, float bc2_sqrt,
                                                               int step, float ent_coef, float theta_min, float theta_max,
                                                               float* __restrict__ sum_out, float* __restrict__ state) {
    __shared__ float red[kVarThreads / 64];
    float s = 0.f;
    for (int b = threadIdx.x; b < n_rows; b += kVarThreads) s += col[(size_t)b * row_pitch];   // fixed order: rows, lanes, waves
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float sum = red[0];
#pragma unroll
    for (int k = 1; k < kVarThreads / 64; ++k) sum += red[k];
    *sum_out = sum;
    // theta follows the actor: its clip coefficient of this step scales the gradient, a skipped actor (coefficient 0) skips theta
    const float coef = clip_stats[2];
    const float g = (sum - ent_coef) * coef;   // d(L - ent_coef H)/d theta, H = 1 + log 2 pi + theta
    if (coef == 0.f || !isfinite(g)) {         // nothing but the counter is written
        state[6] += 1.f;
        return;
    }
    // the rate the nets stepped with: the *_lr step launch left it in the slot the next call reads
    const float lr_step = lr_state ? lr_state[(step + 1) & 1] : lr;
    const float m = state[2], v = state[3];
    const float mm = m + (g - m) * (1.0f - beta1);   // navppo_adam_apply's expressions on a scalar
    const float vv = beta2 * v + (1.0f - beta2) * (g * g);
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    float theta = state[0] - (lr_step / bc1) * (mm / denom);
    theta = fminf(fmaxf(theta, theta_min), theta_max);
    state[0] = theta;
    state[1] = expf(theta);
    state[2] = mm;
    state[3] = vv;
    state[4] = g;
    state[5] += 1.f;
    state[7] = 2.8378770664093453f + theta;   // 1 + log 2 pi + theta
}

}  // namespace

void navppo_launch_var_step(const float* col, int n_rows, int row_pitch, const NavppoStep& s, const NavppoVar& v, float* sum_out,
                            void* stream) {
    const NavppoBias bc = navppo_bias(s.beta1, s.beta2, s.step);
    // the clamps of theta: log var_min / log var_max in double, rounded once (the host mirror does the same)
    const float theta_min = (float)std::log((double)v.var_min), theta_max = (float)std::log((double)v.var_max);
    hipLaunchKernelGGL(var_step_kernel, dim3(1), dim3(kVarThreads), 0, (hipStream_t)stream, col, n_rows, row_pitch, (const float*)s.clip_stats,
                       (const float*)s.lr_state, s.lr, s.beta1, s.beta2, s.eps, bc.bc1, bc.bc2_sqrt, (int)s.step, v.ent_coef, theta_min, theta_max,
                       sum_out, v.state);
}
