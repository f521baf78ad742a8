// ppo_reward_norm.hip -- navppo_return_moments, navppo_reward_scale: reward normalisation by a running variance of the discounted return
// (include/navppo.h "Reward normalisation"; host mirror: navbot_ppo_amd.ppo.reward_norm_reference).
//
// navppo_return_moments is the FORWARD twin of the return scan (navsim.hip: rtg_kernel_split).  Per env column the running return
//   R = gamma R + r[t];  R joins the batch moments;  R = 0 where ended[t]          (t = 0 .. T - 1, float64)
// is a serial recurrence, so the column is split over T: a workgroup owns kRnCols adjacent columns and kRnChunks chunks of kRnRows rows
// (thread = column x chunk):
//   pass 1   every chunk scans its rows from registers with carry-in 0 -> B (R behind its last row) and A = gamma^rows, or 0 when an
//            episode ends inside the chunk: R_out = B + A R_in
//   carry    R_in of chunk c, composed serially from the (A, B) pairs of the chunks in front of it (LDS, <= 15 steps)
//   pass 2   the chunk re-runs the recurrence from its true carry-in, keeps its returns in registers and takes their (n, mean, M2) in
//            two passes (sum, then squared deviations from the chunk's own mean)
// T > 512: super-chunks of 512 rows from the batch start; rows past T are skipped (A = 1, B = 0).  The triples (n, mean, M2) are then
// combined with Chan's pairwise formula along ONE fixed tree: neighbouring threads of the workgroup (strides 1, 2, .. 128: the lanes
// of a wave first, then the waves), the super-chunks and column blocks of a workgroup in the order it visits them, the workgroups'
// partials in index order in a second launch of one workgroup.  No atomics: the same input gives the same bits.
// N % 16 != 0: thread = column, serial over T with Welford's update per value, the same tree behind it (as the return scan falls back).
//
// navppo_reward_scale: a 1-thread launch merges the K batch rows into the running statistics and stores the scale; the streaming pass
// behind it reads the scale and writes out = clamp(float(double(in) * scale), -clip, clip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "navppo.h"
#include "navppo_internal.h"

namespace {

constexpr int kRnCols = 16, kRnChunks = 16, kRnRows = 32, kRnSuper = kRnChunks * kRnRows, kRnThreads = kRnCols * kRnChunks;
constexpr int kRnMaxBlocks = 1024;   // workgroups of the first launch = rows of g_rn_partials; more column blocks: a workgroup takes several
constexpr int kScaleThreads = 256, kScaleMaxBlocks = 2048;

// The workgroups' partial triples between the two launches of navppo_return_moments.  The entry point takes no workspace, so the 24 KB
// live in the code object (one copy per device): two calls in flight AT THE SAME TIME on one device would share them -- calls on one
// device must be ordered (one stream, or streams that wait for each other), include/navppo.h says so.
__device__ double g_rn_partials[kRnMaxBlocks * 3];

struct Moments {
    double n, mean, m2;
};

// Chan et al.: (a, b) -> the moments of the union, a's values first.  An empty side returns the other side's bits.
__device__ __forceinline__ Moments chan_merge(const Moments& a, const Moments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean, q = b.n / n;
    return {n, a.mean + d * q, a.m2 + b.m2 + (d * d) * (a.n * q)};
}

// the workgroup's tree: thread t holds m; strides 1, 2, .., nthreads / 2 over neighbouring threads; the result is valid in thread 0.
// (every thread of the workgroup calls it; s_m has room for 3 * nthreads doubles)
__device__ __forceinline__ Moments block_tree(Moments m, double* s_m, int tid, int nthreads) {
    __syncthreads();   // (the buffer may still be read by the call before)
    s_m[tid * 3 + 0] = m.n;
    s_m[tid * 3 + 1] = m.mean;
    s_m[tid * 3 + 2] = m.m2;
    __syncthreads();
    for (int s = 1; s < nthreads; s <<= 1) {
        if ((tid & (2 * s - 1)) == 0 && tid + s < nthreads) {
            const Moments b = {s_m[(tid + s) * 3], s_m[(tid + s) * 3 + 1], s_m[(tid + s) * 3 + 2]};
            m = chan_merge(m, b);
            s_m[tid * 3 + 0] = m.n;
            s_m[tid * 3 + 1] = m.mean;
            s_m[tid * 3 + 2] = m.m2;
        }
        __syncthreads();
    }
    return m;
}

__global__ __launch_bounds__(kRnThreads) void return_moments_split(const float* __restrict__ rew, const uint8_t* __restrict__ ended, int T,
                                                                   int N, double gamma, double* __restrict__ carry, int n_colblocks) {
    __shared__ double s_b[kRnChunks][kRnCols], s_a[kRnChunks][kRnCols], s_sup[kRnCols], s_m[kRnThreads * 3];
    const int tid = threadIdx.x, col = tid & (kRnCols - 1), c = tid >> 4;
    Moments acc = {0.0, 0.0, 0.0};   // (thread 0's: the workgroup's running triple)
    for (int qb = blockIdx.x; qb < n_colblocks; qb += gridDim.x) {
        // one workgroup per column block and a block count that is a multiple of 64: runs of 8 adjacent column blocks per XCD, so that
        // a 128-byte line of rewards (2 column blocks) or flags (8) is fetched into one L2 (navsim.hip: rtg_kernel_split)
        int q = qb;
        if (n_colblocks == (int)gridDim.x && (n_colblocks & 63) == 0) {
            const int x = q & 7, y = q >> 3;
            q = ((y >> 3) * 8 + x) * 8 + (y & 7);
        }
        const size_t n = (size_t)q * kRnCols + col;   // N % 16 == 0: all 16 columns exist
        double rsup = carry ? carry[n] : 0.0;
        for (int t_lo = 0; t_lo < T; t_lo += kRnSuper) {
            const int t0 = t_lo + c * kRnRows, len = min(max(T - t0, 0), kRnRows);   // rows t0 .. t0 + len - 1 of this chunk
            float r[kRnRows];
            uint8_t e[kRnRows];
#pragma unroll
            for (int u = 0; u < kRnRows; ++u) {   // rows past T: loaded from row T - 1 (a valid address), never used
                const size_t k = (size_t)min(t0 + u, T - 1) * N + n;
                r[u] = rew[k];
                e[u] = ended[k];
            }
            double b = 0.0, a = 1.0;
            bool any = false;
#pragma unroll
            for (int u = 0; u < kRnRows; ++u) {
                if (u < len) {
                    b = gamma * b + (double)r[u];
                    if (e[u]) b = 0.0;
                    any |= e[u] != 0;
                    a *= gamma;
                }
            }
            s_b[c][col] = b;
            s_a[c][col] = any ? 0.0 : a;
            __syncthreads();
            double R = rsup;
#pragma unroll
            for (int k = 0; k < kRnChunks - 1; ++k)
                if (k < c) R = s_b[k][col] + s_a[k][col] * R;
            double v[kRnRows];
            double sum = 0.0;
#pragma unroll
            for (int u = 0; u < kRnRows; ++u) {
                if (u < len) {
                    R = gamma * R + (double)r[u];
                    v[u] = R;
                    sum += R;
                    if (e[u]) R = 0.0;
                } else {
                    v[u] = 0.0;
                }
            }
            Moments m = {(double)len, 0.0, 0.0};
            if (len > 0) {
                m.mean = sum / (double)len;
#pragma unroll
                for (int u = 0; u < kRnRows; ++u) {
                    const double d = v[u] - m.mean;
                    if (u < len) m.m2 += d * d;
                }
            }
            if (c == kRnChunks - 1) s_sup[col] = R;   // R behind the super-chunk's last row (a chunk without rows passes its carry-in on)
            m = block_tree(m, s_m, tid, kRnThreads);  // (its barriers also order s_sup, s_a and s_b against the next super-chunk)
            if (tid == 0) acc = chan_merge(acc, m);
            rsup = s_sup[col];
        }
        if (carry && c == 0) carry[n] = rsup;
        __syncthreads();   // (s_sup is rewritten by the next column block)
    }
    if (tid == 0) {
        g_rn_partials[blockIdx.x * 3 + 0] = acc.n;
        g_rn_partials[blockIdx.x * 3 + 1] = acc.mean;
        g_rn_partials[blockIdx.x * 3 + 2] = acc.m2;
    }
}

// any N: thread = env column, forward over T; Welford's update per value
__global__ __launch_bounds__(64) void return_moments_generic(const float* __restrict__ rew, const uint8_t* __restrict__ ended, int T, int N,
                                                             double gamma, double* __restrict__ carry, int n_colblocks) {
    __shared__ double s_m[64 * 3];
    const int tid = threadIdx.x;
    Moments acc = {0.0, 0.0, 0.0};
    for (int qb = blockIdx.x; qb < n_colblocks; qb += gridDim.x) {
        const long long n = (long long)qb * 64 + tid;
        Moments m = {0.0, 0.0, 0.0};
        if (n < N) {
            double R = carry ? carry[n] : 0.0;
            for (int t = 0; t < T; ++t) {
                const size_t k = (size_t)t * N + (size_t)n;
                R = gamma * R + (double)rew[k];
                m.n += 1.0;
                const double d = R - m.mean;
                m.mean += d / m.n;
                m.m2 += d * (R - m.mean);
                if (ended[k]) R = 0.0;
            }
            if (carry) carry[n] = R;
        }
        m = block_tree(m, s_m, tid, 64);
        if (tid == 0) acc = chan_merge(acc, m);
    }
    if (tid == 0) {
        g_rn_partials[blockIdx.x * 3 + 0] = acc.n;
        g_rn_partials[blockIdx.x * 3 + 1] = acc.mean;
        g_rn_partials[blockIdx.x * 3 + 2] = acc.m2;
    }
}

// the last stage: one workgroup; thread t merges partials [t per, (t + 1) per) in order, then the tree
__global__ __launch_bounds__(256) void return_moments_final(int n_partials, double* __restrict__ moments) {
    __shared__ double s_m[256 * 3];
    const int tid = threadIdx.x, per = (n_partials + 255) / 256;
    Moments m = {0.0, 0.0, 0.0};
    for (int j = 0; j < per; ++j) {
        const int p = tid * per + j;
        if (p < n_partials) m = chan_merge(m, Moments{g_rn_partials[p * 3], g_rn_partials[p * 3 + 1], g_rn_partials[p * 3 + 2]});
    }
    m = block_tree(m, s_m, tid, 256);
    if (tid == 0) {
        moments[0] = m.n;
        moments[1] = m.mean;
        moments[2] = m.m2;
    }
}

// the 1-thread prologue of navppo_reward_scale: rows k = 0 .. K - 1 into (mean, var, count), then the scale
__global__ void reward_rms_merge(double* __restrict__ rms, const double* __restrict__ rows, int K, double eps) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double mean = rms[0], var = rms[1], count = rms[2];
    for (int k = 0; k < K; ++k) {
        const double bn = rows[k * 3], bm = rows[k * 3 + 1], bm2 = rows[k * 3 + 2];
        if (!(bn > 0.0) || !isfinite(bn) || !isfinite(bm) || !isfinite(bm2)) continue;   // an empty or a poisoned batch: skipped
        const double d = bm - mean, tot = count + bn;
        mean = mean + d * bn / tot;
        var = (var * count + bm2 + d * d * count * bn / tot) / tot;
        count = tot;
    }
    rms[0] = mean;
    rms[1] = var;
    rms[2] = count;
    rms[3] = 1.0 / sqrt(var + eps);
}

// a NaN compares false both ways and stays
__device__ __forceinline__ float scale_clamp(float x, double scale, float clip) {
    const float y = (float)((double)x * scale);
    return y < -clip ? -clip : (y > clip ? clip : y);
}

template <bool VEC>
__global__ __launch_bounds__(kScaleThreads) void reward_scale_kernel(const double* __restrict__ rms, const float* in, float* out, long long n,
                                                                     float clip) {
    const double scale = rms[3];   // (written by the launch in front)
    const long long stride = (long long)gridDim.x * kScaleThreads, i0 = (long long)blockIdx.x * kScaleThreads + threadIdx.x;
    if (VEC) {   // both pointers 16-byte aligned: float4 body, scalar tail
        const long long n4 = n >> 2;
        const float4* const in4 = reinterpret_cast<const float4*>(in);
        float4* const out4 = reinterpret_cast<float4*>(out);
        for (long long i = i0; i < n4; i += stride) {
            float4 x = in4[i];
            x.x = scale_clamp(x.x, scale, clip);
            x.y = scale_clamp(x.y, scale, clip);
            x.z = scale_clamp(x.z, scale, clip);
            x.w = scale_clamp(x.w, scale, clip);
            out4[i] = x;
        }
        for (long long i = (n4 << 2) + i0; i < n; i += stride) out[i] = scale_clamp(in[i], scale, clip);
    } else {
        for (long long i = i0; i < n; i += stride) out[i] = scale_clamp(in[i], scale, clip);
    }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int navppo_return_moments(const float* rew_dev, const uint8_t* ended_dev, int32_t T, int32_t N, double gamma, double* carry_dev,
                          double* moments_dev, void* stream) {
    const char* const who = "navppo_return_moments";
    if (!rew_dev || !ended_dev || !moments_dev) return navppo_bad_args(who, "bad argument (null pointer)");
    if (T < 1 || N < 1) return navppo_bad_args(who, "bad argument (T >= 1, N >= 1)");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return navppo_bad_args(who, "bad argument (gamma in [0, 1])");
    if (((uintptr_t)rew_dev & 3) || ((uintptr_t)moments_dev & 7) || ((uintptr_t)carry_dev & 7))
        return navppo_bad_args(who, "rew_dev must be 4-byte, moments_dev and carry_dev 8-byte aligned");
    int blocks;
    if (N % kRnCols == 0) {
        const int nb = N / kRnCols;
        blocks = nb < kRnMaxBlocks ? nb : kRnMaxBlocks;
        hipLaunchKernelGGL(return_moments_split, dim3(blocks), dim3(kRnThreads), 0, (hipStream_t)stream, rew_dev, ended_dev, (int)T, (int)N, gamma,
                           carry_dev, nb);
    } else {
        const int nb = (int)(((int64_t)N + 63) / 64);
        blocks = nb < kRnMaxBlocks ? nb : kRnMaxBlocks;
        hipLaunchKernelGGL(return_moments_generic, dim3(blocks), dim3(64), 0, (hipStream_t)stream, rew_dev, ended_dev, (int)T, (int)N, gamma,
                           carry_dev, nb);
    }
    hipLaunchKernelGGL(return_moments_final, dim3(1), dim3(256), 0, (hipStream_t)stream, blocks, moments_dev);
    return navppo_launched(who);
}

int navppo_reward_scale(double* rms_dev, const double* moments_dev, int32_t K, const float* rew_in_dev, float* rew_out_dev, int64_t n,
                        double eps, double clip, void* stream) {
    const char* const who = "navppo_reward_scale";
    if (!rms_dev || (K > 0 && !moments_dev) || (n > 0 && (!rew_in_dev || !rew_out_dev))) return navppo_bad_args(who, "bad argument (null pointer)");
    if (K < 0 || n < 0) return navppo_bad_args(who, "bad argument (K >= 0, n >= 0)");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return navppo_bad_args(who, "bad argument (eps >= 0)");
    const float clipf = (float)clip;
    if (!(clip > 0.0) || !(clipf > 0.f)) return navppo_bad_args(who, "bad argument (clip > 0, +inf allowed)");
    if (((uintptr_t)rms_dev & 7) || ((uintptr_t)moments_dev & 7) || ((uintptr_t)rew_in_dev & 3) || ((uintptr_t)rew_out_dev & 3))
        return navppo_bad_args(who, "rms_dev and moments_dev must be 8-byte, the rewards 4-byte aligned");
    hipLaunchKernelGGL(reward_rms_merge, dim3(1), dim3(1), 0, (hipStream_t)stream, rms_dev, moments_dev, (int)K, eps);
    if (n > 0) {
        const bool vec = !(((uintptr_t)rew_in_dev | (uintptr_t)rew_out_dev) & 15);
        const int64_t work = vec ? (n + 3) / 4 : n, want = (work + kScaleThreads - 1) / kScaleThreads;
        const int blocks = (int)(want < kScaleMaxBlocks ? want : kScaleMaxBlocks);
        if (vec)
            hipLaunchKernelGGL(reward_scale_kernel<true>, dim3(blocks), dim3(kScaleThreads), 0, (hipStream_t)stream, rms_dev, rew_in_dev, rew_out_dev,
                               (long long)n, clipf);
        else
            hipLaunchKernelGGL(reward_scale_kernel<false>, dim3(blocks), dim3(kScaleThreads), 0, (hipStream_t)stream, rms_dev, rew_in_dev,
                               rew_out_dev, (long long)n, clipf);
    }
    return navppo_launched(who);
}

}  // extern "C"
#pragma GCC visibility pop
