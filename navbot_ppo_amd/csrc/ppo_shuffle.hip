// ppo_shuffle.hip -- navppo_shuffle_batch: the device-side batch shuffle of the minibatch update (include/navppo.h "Minibatch updates").
//
// out[i] = in[pi(i)] for the five per-sample arrays of an update's batch (observation rows, actions, old log-probabilities,
// rewards-to-go, advantages), pi a bijection of [0, n) computed PER INDEX in the kernel: no permutation table in memory, no host round
// trip -- the epochs of an update are queued without one.
//
// The permutation (mirrored by navbot_ppo_amd.ppo.batch_permutation; include/navppo.h states it for a C caller): a 6-round Feistel
// network on b = ceil(log2 n) bits, unbalanced when b is odd (the halves swap widths every round), cycle-walked into [0, n).  The round
// function is two rounds of Philox's multiply-mix (mlp64_policy.h: philox10's multipliers, high ^ low word of the 32 x 32 product); the
// round keys are a Weyl sequence (Philox's increments) from two words of Philox4x32-10 over (counter, n) keyed by `key`, taken on the host.
//
// Layout: destination-ordered.  A workgroup owns 256 consecutive destination samples: every thread takes pi of ONE sample (and copies
// that sample's action and three scalars), leaves it in LDS, and the workgroup then copies the observation rows chunk by chunk --
// consecutive lanes take consecutive chunks of the destination rows, so the stores are coalesced and the lanes of one row read their
// source row as one contiguous run.  The chunk is the widest vector that divides the row: 64-byte rows (16 float32) and 32-byte rows
// (16 float16) 16 bytes, 168 bytes (42 float32) 8, 84 bytes (42 float16) 4.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "navppo.h"
#include "navppo_internal.h"

#ifndef NAVPPO_SHUFFLE_NT
#define NAVPPO_SHUFFLE_NT 0   // 1: non-temporal stores (A/B builds; DESIGN.md 5l has both figures)
#endif

namespace {

constexpr int kShufThreads = 256;   // = destination samples per workgroup
constexpr int kShufRounds = 6;
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// what the kernel needs of (n, key, counter): the widths of the two halves and the base round keys
struct ShufflePerm {
    uint32_t n, a, c, k0, k1;   // a = b / 2 (high half at even rounds), c = b - a; b = bits of n - 1
};

// Philox4x32-10 (the generator of mlp64_policy.h / navsim.hip) on the host
void philox10_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

ShufflePerm make_perm(int64_t n, uint64_t key, uint64_t counter) {
    ShufflePerm p;
    p.n = (uint32_t)n;
    uint32_t b = 0;
    while (((uint64_t)1 << b) < (uint64_t)n) ++b;
    p.a = b / 2;
    p.c = b - p.a;
    uint32_t o[4];
    philox10_host((uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)n, 0x73687566u /* "shuf" */, (uint32_t)key, (uint32_t)(key >> 32), o);
    p.k0 = o[0];
    p.k1 = o[1];
    return p;
}

// F(r; k0, k1): two multiply-mix rounds
__device__ __forceinline__ uint32_t shuffle_round_fn(uint32_t r, uint32_t k0, uint32_t k1) {
    const uint64_t p = (uint64_t)kPhiloxM0 * (uint32_t)(r + k0);
    const uint32_t t = (uint32_t)(p >> 32) ^ (uint32_t)p ^ k1;
    const uint64_t q = (uint64_t)kPhiloxM1 * t;
    return (uint32_t)(q >> 32) ^ (uint32_t)q;
}

// one pass of the network over [0, 2^(a + c)): round j splits x into (L: the high wl bits, R: the low wr bits), (wl, wr) = (a, c) at
// even j and (c, a) at odd j, and gives (R << wl) | (L ^ (F(R) & (2^wl - 1))) -- the halves trade places and widths
__device__ __forceinline__ uint32_t shuffle_feistel(uint32_t x, const ShufflePerm& p) {
    uint32_t wl = p.a, wr = p.c, k0 = p.k0, k1 = p.k1;
#pragma unroll
    for (int j = 0; j < kShufRounds; ++j) {
        const uint32_t ml = (1u << wl) - 1u, mr = (1u << wr) - 1u;
        const uint32_t l = x >> wr, r = x & mr;
        x = (r << wl) | (l ^ (shuffle_round_fn(r, k0, k1) & ml));
        const uint32_t t = wl; wl = wr; wr = t;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    return x;
}

// pi(i): cycle-walking -- the network is a bijection of the power-of-two domain, so the walk from an i < n returns to [0, n)
__device__ __forceinline__ uint32_t shuffle_pi(uint32_t i, const ShufflePerm& p) {
    uint32_t x = i;
    do x = shuffle_feistel(x, p);
    while (x >= p.n);
    return x;
}

template <class V>
__device__ __forceinline__ void shuffle_store(V* dst, const V& v) {
#if NAVPPO_SHUFFLE_NT
    __builtin_nontemporal_store(v, dst);
#else
    *dst = v;
#endif
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int ROW_BYTES> struct ShufChunk { using type = u32x4; };   // 64- and 32-byte rows
template <> struct ShufChunk<168> { using type = u32x2; };
template <> struct ShufChunk<84> { using type = uint32_t; };

template <int ROW_BYTES>
__global__ __launch_bounds__(kShufThreads) void shuffle_batch_kernel(const unsigned char* __restrict__ obs, const f32x2* __restrict__ act,
                                                                      const float* __restrict__ logp, const float* __restrict__ rtg,
                                                                      const float* __restrict__ adv, ShufflePerm p,
                                                                      unsigned char* __restrict__ obs_out, f32x2* __restrict__ act_out,
                                                                      float* __restrict__ logp_out, float* __restrict__ rtg_out,
                                                                      float* __restrict__ adv_out, const float* __restrict__ gate) {
    if (gate && navppo_kl_stopped(gate)) return;   // (uniform: written only by the step launch of an earlier epoch)
    using V = typename ShufChunk<ROW_BYTES>::type;
    constexpr int kLanesPerRow = ROW_BYTES / (int)sizeof(V);   // 4 | 2 | 21 | 21
    static_assert(kLanesPerRow * (int)sizeof(V) == ROW_BYTES, "the chunk divides the row");
    __shared__ uint32_t src_of[kShufThreads];
    const uint32_t base = blockIdx.x * (uint32_t)kShufThreads;   // < n < 2^31
    const uint32_t left = p.n - base, rows = left < (uint32_t)kShufThreads ? left : (uint32_t)kShufThreads;
    const uint32_t t = threadIdx.x;
    if (t < rows) {
        const uint32_t i = base + t, s = shuffle_pi(i, p);
        src_of[t] = s;
        shuffle_store(act_out + i, act[s]);
        shuffle_store(logp_out + i, logp[s]);
        shuffle_store(rtg_out + i, rtg[s]);
        shuffle_store(adv_out + i, adv[s]);
    }
    __syncthreads();
    const V* const in = reinterpret_cast<const V*>(obs);
    V* const out = reinterpret_cast<V*>(obs_out) + (size_t)base * kLanesPerRow;
    for (uint32_t c = t; c < rows * kLanesPerRow; c += kShufThreads) {
        const uint32_t row = c / kLanesPerRow, j = c - row * kLanesPerRow;
        shuffle_store(out + c, in[(size_t)src_of[row] * kLanesPerRow + j]);
    }
}

// [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int navppo_shuffle_batch(const void* obs_dev, int32_t obs_dim, int32_t obs_f16, const float* act_dev, const float* logp_old_dev,
                         const float* rtg_dev, const float* adv_dev, int64_t n_samples, uint64_t key, uint64_t counter, void* obs_out,
                         float* act_out, float* logp_out, float* rtg_out, float* adv_out, const float* gate_dev, void* stream) {
    const char* const who = "navppo_shuffle_batch";
    if (!obs_dev || !act_dev || !logp_old_dev || !rtg_dev || !adv_dev || !obs_out || !act_out || !logp_out || !rtg_out || !adv_out)
        return navppo_bad_args(who, "bad argument (null pointer)");
    if (n_samples < 1 || n_samples >= ((int64_t)1 << 31)) return navppo_bad_args(who, "bad argument (1 <= n_samples < 2^31)");
    if (obs_dim != 16 && obs_dim != 42) return navppo_bad_args(who, "bad argument (obs_dim is 16 or 42)");
    // the rule of the update's entry points (obs_aligned, ppo_mlp64.hip): rows are moved in the chunks they are read in there
    const uintptr_t omask = obs_dim == 16 ? 15 : (obs_f16 ? 3 : 7);
    if (((uintptr_t)obs_dev & omask) || ((uintptr_t)obs_out & omask) || ((uintptr_t)act_dev & 7) || ((uintptr_t)act_out & 7) ||
        (((uintptr_t)logp_old_dev | (uintptr_t)rtg_dev | (uintptr_t)adv_dev | (uintptr_t)logp_out | (uintptr_t)rtg_out | (uintptr_t)adv_out) & 3))
        return navppo_bad_args(who, "obs must be 16-byte (42 columns: 8-byte, float16: 4-byte), act 8-byte and the scalars 4-byte aligned, in and out");
    const size_t n = (size_t)n_samples, row = (size_t)obs_dim * (obs_f16 ? 2 : 4);
    const void* const ins[5] = {obs_dev, act_dev, logp_old_dev, rtg_dev, adv_dev};
    const void* const outs[5] = {obs_out, act_out, logp_out, rtg_out, adv_out};
    const size_t bytes[5] = {n * row, n * 8, n * 4, n * 4, n * 4};
    for (int o = 0; o < 5; ++o) {
        for (int i = 0; i < 5; ++i)
            if (ranges_overlap(outs[o], bytes[o], ins[i], bytes[i])) return navppo_bad_args(who, "an output overlaps an input");
        for (int q = 0; q < o; ++q)
            if (ranges_overlap(outs[o], bytes[o], outs[q], bytes[q])) return navppo_bad_args(who, "two outputs overlap");
    }
    const ShufflePerm p = make_perm(n_samples, key, counter);
    const dim3 grid((unsigned)((n_samples + kShufThreads - 1) / kShufThreads)), block(kShufThreads);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const unsigned char*>(obs_dev),
                           reinterpret_cast<const f32x2*>(act_dev), logp_old_dev, rtg_dev, adv_dev, p, reinterpret_cast<unsigned char*>(obs_out),
                           reinterpret_cast<f32x2*>(act_out), logp_out, rtg_out, adv_out, gate_dev);
    };
    switch ((int)row) {
        case 64: launch(shuffle_batch_kernel<64>); break;
        case 32: launch(shuffle_batch_kernel<32>); break;
        case 168: launch(shuffle_batch_kernel<168>); break;
        default: launch(shuffle_batch_kernel<84>); break;
    }
    return navppo_launched(who);
}

}  // extern "C"
#pragma GCC visibility pop
