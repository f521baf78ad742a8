// ppo_group_sums.hip -- navppo_group_sums: navppo_episode_sums per GROUP of envs (include/navppo.h "Per-group episode sums").
//
// The [T, N] buffers a rollout fills, the envs labelled with a group id (the scenario an env plays: its tape of a mover bank) ->
// sums [K][8] f64, row k over the columns n with group[n] == k: episodes, successes, collisions, time-outs, the sum of ep_length, the
// sum of ep_return over ended entries (episode_sums_partial's six figures, ppo_mlp64.hip, entry by entry), the sum of |adv| and the
// number of rows T x envs of the group.  Host mirror: navbot_ppo_amd.scenarios.group_sums_reference.
//
// No atomics: the result does not depend on the launch schedule (two calls on the same buffers give the same bits).  Store and sum:
//   1. group_sums_columns: lanes along N -- a lane owns ONE column, a workgroup 256 consecutive columns and one chunk of T, so every
//      wave reads 64 consecutive entries of a row per load (coalesced) -- and stores its column's seven partial sums of the chunk to
//      partial[chunk][figure][n] (coalesced as well).  It never looks at the group ids.
//   2. group_sums_final: one workgroup of 16 waves per group.  Lane l of wave w walks the columns l, l + 64, ... in ascending order and
//      adds, for those that belong to the group, the partials of the chunks w, w + 16, ...; the threads' sums are then added in a
//      fixed tree.  An id outside [0, K) matches no workgroup: such a column is counted nowhere and indexes nothing.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "navppo.h"
#include "navppo_internal.h"

namespace {

constexpr int kGsThreads = 256;
constexpr int kGsFigures = 7;       // what a column stores per chunk: the figures 0..6 (7, the rows, is T x the group's env count)
constexpr int kGsMinRows = 8;       // a chunk is at least this many rows of T (unless T itself is shorter)
constexpr int kGsWaves = 1024;      // the chunk count brings the first launch to about this many waves (4 per CU)

static_assert(NAVPPO_GROUP_SUMS_COLS == kGsFigures + 1, "sums_dev rows are the seven stored figures and the row count");

// how T is cut: rows per chunk and the number of chunks, a function of (T, N) alone -- the workspace size and both launches use it
struct GsCut {
    int rows, chunks;
};
GsCut gs_cut(int T, int N) {
    const long long blocks_n = ((long long)N + kGsThreads - 1) / kGsThreads;
    const long long want = (kGsWaves / (kGsThreads / 64) + blocks_n - 1) / blocks_n;   // <= 256
    const long long cap = ((long long)T + kGsMinRows - 1) / kGsMinRows;
    long long c = want < cap ? want : cap;
    if (c < 1) c = 1;
    GsCut cut;
    cut.rows = (int)(((long long)T + c - 1) / c);
    cut.chunks = (int)(((long long)T + cut.rows - 1) / cut.rows);
    return cut;
}

bool gs_sizes_ok(int32_t T, int32_t N, int32_t K) { return T >= 1 && N >= 1 && K >= 1 && K <= 1024; }

template <bool ADV>
__global__ __launch_bounds__(kGsThreads) void group_sums_columns(const uint8_t* __restrict__ ended, const uint8_t* __restrict__ arrive,
                                                                 const uint8_t* __restrict__ done, const int32_t* __restrict__ ep_len,
                                                                 const float* __restrict__ ep_ret, const float* __restrict__ adv, int T,
                                                                 int N, int rows, double* __restrict__ partial) {
    const long long n = (long long)blockIdx.x * kGsThreads + threadIdx.x;
    if (n >= N) return;
    const long long t0 = (long long)blockIdx.y * rows;   // < T: the grid has ceil(T / rows) chunks
    const long long t1 = t0 + rows < T ? t0 + rows : T;
    unsigned c_ep = 0, c_ok = 0, c_hit = 0, c_tmo = 0;
    long long len = 0;
    double ret = 0, aabs = 0;
    const size_t N_ = (size_t)N;
    size_t q = (size_t)t0 * N_ + (size_t)n;
#pragma unroll 8   // (eight rows' loads in flight per lane: the launch is a few waves per SIMD)
    for (long long t = t0; t < t1; ++t, q += N_) {
        // every load of the row first, none behind a condition: a load that is only needed when `ended` is set would be branched
        // around and waited for row by row
        const unsigned eb = ended[q], ab = arrive[q], db = done[q];
        const int l = ep_len[q];
        const float r = ep_ret[q];
        const bool e = eb != 0, a = (ab != 0) && e, d = (db != 0) && e;   // episode_sums_partial's `one`
        c_ep += e;
        c_ok += a;
        c_hit += d && !a;
        c_tmo += e && !d && !a;
        len += l;
        ret += (double)__uint_as_float(__float_as_uint(r) & (e ? 0xffffffffu : 0u));   // r where ended, +0.0 elsewhere
        if (ADV) aabs += (double)fabsf(adv[q]);
    }
    double* const out = partial + (size_t)blockIdx.y * kGsFigures * N_ + (size_t)n;
    out[0] = (double)c_ep;
    out[N_] = (double)c_ok;
    out[2 * N_] = (double)c_hit;
    out[3 * N_] = (double)c_tmo;
    out[4 * N_] = (double)len;
    out[5 * N_] = ret;
    if (ADV) out[6 * N_] = aabs;
}

// One workgroup of 16 waves per group.  The columns are walked in tiles of 4096: every thread compares FOUR ids of the tile with the
// group (so a workgroup reads the N ids once) and leaves the answers in LDS; then lane l of wave w takes the tile's columns l, l + 64,
// ... in ascending order and, for those of the group, adds the partials of the chunks w, w + 16, ... -- all loads of a column issued
// before the first add.  A fixed order per thread, then a fixed tree: the lanes of a wave by xor shuffles, the waves in order.
constexpr int kGsFinalThreads = 1024, kGsFinalWaves = kGsFinalThreads / 64, kGsTile = 4 * kGsFinalThreads;

template <bool ADV>   // ADV = false: figure 6 of the workspace was not written and is not read; its sum is 0
__global__ __launch_bounds__(kGsFinalThreads) void group_sums_final(const double* __restrict__ partial, const int32_t* __restrict__ group,
                                                                    int T, int N, int chunks, double* __restrict__ sums) {
    constexpr int F = ADV ? kGsFigures : kGsFigures - 1;
    __shared__ uint8_t match[kGsTile];
    __shared__ double red[kGsFinalWaves][NAVPPO_GROUP_SUMS_COLS];
    const int k = blockIdx.x, b = threadIdx.x, lane = b & 63, wave = __builtin_amdgcn_readfirstlane(b >> 6);
    const size_t N_ = (size_t)N;
    double acc[F];
#pragma unroll
    for (int j = 0; j < F; ++j) acc[j] = 0.0;
    unsigned envs = 0;
    for (long long base = 0; base < N; base += kGsTile) {
#pragma unroll
        for (int r = 0; r < kGsTile / kGsFinalThreads; ++r) {
            const long long own = base + b + r * kGsFinalThreads;
            const int32_t g = group[own < N ? own : (long long)N - 1];   // (clamped, not skipped: the four loads go out together)
            match[b + r * kGsFinalThreads] = (own < N && g == k) ? 1 : 0;
        }
        __syncthreads();
        for (int i = 0; i < kGsTile / 64; ++i) {
            const int col = lane + 64 * i;
            if (!match[col]) continue;   // (a column past N never matches)
            envs += wave == 0;
            for (int c = wave; c < chunks; c += kGsFinalWaves) {
                const double* const p = partial + (size_t)c * kGsFigures * N_ + (size_t)(base + col);
                double v[F];
#pragma unroll
                for (int j = 0; j < F; ++j) v[j] = p[(size_t)j * N_];
#pragma unroll
                for (int j = 0; j < F; ++j) acc[j] += v[j];
            }
        }
        __syncthreads();
    }
    double v[NAVPPO_GROUP_SUMS_COLS];
#pragma unroll
    for (int j = 0; j < kGsFigures; ++j) v[j] = j < F ? acc[j < F ? j : 0] : 0.0;
    v[kGsFigures] = (double)envs;
#pragma unroll
    for (int j = 0; j < NAVPPO_GROUP_SUMS_COLS; ++j)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[j] += __shfl_xor(v[j], m, 64);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NAVPPO_GROUP_SUMS_COLS; ++j) red[wave][j] = v[j];
    __syncthreads();
    if (b < NAVPPO_GROUP_SUMS_COLS) {
        double t = 0.0;
        for (int w = 0; w < kGsFinalWaves; ++w) t += red[w][b];
        sums[(size_t)k * NAVPPO_GROUP_SUMS_COLS + b] = b < kGsFigures ? t : t * (double)T;   // (an integer < 2^53: exact)
    }
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

size_t navppo_group_sums_ws_bytes(int32_t T, int32_t N, int32_t K) {
    if (!gs_sizes_ok(T, N, K)) return 0;
    return (size_t)gs_cut(T, N).chunks * kGsFigures * (size_t)N * sizeof(double);
}

int navppo_group_sums(const uint8_t* ended_dev, const uint8_t* arrive_dev, const uint8_t* done_dev, const int32_t* ep_length_dev,
                      const float* ep_return_dev, const float* adv_dev, const int32_t* group_dev, int32_t T, int32_t N, int32_t K,
                      double* sums_dev, void* workspace_dev, void* stream) {
    const char* const who = "navppo_group_sums";
    if (!ended_dev || !arrive_dev || !done_dev || !ep_length_dev || !ep_return_dev || !group_dev || !sums_dev)
        return navppo_bad_args(who, "bad argument (null pointer)");
    if (!gs_sizes_ok(T, N, K)) return navppo_bad_args(who, "bad argument (T >= 1, N >= 1, 1 <= K <= 1024)");
    if (!workspace_dev) return navppo_bad_args(who, "bad argument (workspace_dev: navppo_group_sums_ws_bytes(T, N, K) bytes)");
    if (((uintptr_t)ep_length_dev | (uintptr_t)ep_return_dev | (uintptr_t)adv_dev | (uintptr_t)group_dev) & 3)
        return navppo_bad_args(who, "ep_length, ep_return, adv and group must be 4-byte aligned");
    if (((uintptr_t)sums_dev | (uintptr_t)workspace_dev) & 7) return navppo_bad_args(who, "sums and workspace must be 8-byte aligned");
    const GsCut cut = gs_cut(T, N);
    double* const partial = reinterpret_cast<double*>(workspace_dev);
    const dim3 grid((unsigned)(((long long)N + kGsThreads - 1) / kGsThreads), (unsigned)cut.chunks), block(kGsThreads);
    if (adv_dev)
        hipLaunchKernelGGL(group_sums_columns<true>, grid, block, 0, (hipStream_t)stream, ended_dev, arrive_dev, done_dev, ep_length_dev,
                           ep_return_dev, adv_dev, (int)T, (int)N, cut.rows, partial);
    else
        hipLaunchKernelGGL(group_sums_columns<false>, grid, block, 0, (hipStream_t)stream, ended_dev, arrive_dev, done_dev, ep_length_dev,
                           ep_return_dev, adv_dev, (int)T, (int)N, cut.rows, partial);
    const dim3 fgrid((unsigned)K), fblock(kGsFinalThreads);
    if (adv_dev)
        hipLaunchKernelGGL(group_sums_final<true>, fgrid, fblock, 0, (hipStream_t)stream, partial, group_dev, (int)T, (int)N, cut.chunks, sums_dev);
    else
        hipLaunchKernelGGL(group_sums_final<false>, fgrid, fblock, 0, (hipStream_t)stream, partial, group_dev, (int)T, (int)N, cut.chunks, sums_dev);
    return navppo_launched(who);
}

}  // extern "C"
#pragma GCC visibility pop
