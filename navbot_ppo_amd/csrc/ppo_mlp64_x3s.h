// ppo_mlp64_x3s.h -- round 6: the split-bf16 update pass of the 16-64-64 heads as ONE hand-placed instruction stream per wave.
// Included by ppo_mlp64.hip inside its anonymous namespace (uses Layout, XPad, kpos, wslot, split_pair, the pre-split observation
// buffer of mlp64_split_obs and the partial-row / reduce_adam contract of the other passes).  Same arithmetic as pass_body_x3 -- float32
// products from three exact bf16 pieces per operand, six piece products, small terms first, float32 accumulate -- reorganised
// around what round 5's counters and tools/ubench/gen_mfma_stream.py (profiles/r06_mfma_stream.txt) say about gfx950:
//   * ONE wave per SIMD hides up to ~6 vector instructions behind each v_mfma_f32_32x32x16_bf16 of its OWN stream (33.5 -> 37
//     cycles per MFMA slot), every further one costs ~4 cycles; two waves per SIMD do no better per SIMD, and the compiler
//     clusters MFMAs and vector work instead of interleaving them.  So: 4 waves x 512 registers (no spills; round 5's 8 x 256
//     spilled 130), every MFMA and every block of the splits an `asm volatile` statement -- the compiler allocates registers, inserts
//     the s_waitcnt of the LDS / global loads it still issues itself and loads MFMA operands straight into AGPRs, but cannot
//     re-order the stream -- with 5-6 vector instructions written behind each MFMA.
//   * H1 and dH2 are split ONCE (round 5: twice, 352 of 880 split instructions per tile): the bf16 pieces feed F2 / B2 from
//     registers (k = hidden unit), are stored to a wave-private LDS image [piece][sample][unit] and come back transposed for the
//     weight-gradient products (k = sample) through ds_read_b64_tr_b16; dH1 (G1's operand) takes the same way.  No float32 tile,
//     no second split, no wave_lds_fence round trips.
//   * the sample sums db2, dW3, dW4 are per-lane partial sums over the wave's tiles (a lane owns the same sample slot in every
//     tile), reduced across lanes once per launch; db1 rides on G1's operand (one MFMA with a ones operand per piece).
//   * layer 1 runs a tile ahead: F1 of the next tile sits inside G2, and the vector work that used to wait in front of F1, F2 and G2
//     (bias starts, relu1, the split of H1's first k-step, the relu mask of layer 1) is spread over the 60 MFMA slots of G2 + F1, a
//     third of which were empty.  The loop starts at F2's first MFMA; tools/verify/mfma_slot_report.py counts what sits in front of
//     every MFMA, tests/test_isa_schedule_cpu.py holds the counts.
//   * the heads ride on their neighbours: F2 ends with c2[0]'s nine products and then c2[1]'s, relu2 of c2[0] and its half of the two dot
//     products sit behind c2[1]'s MFMAs, c2[1]'s half behind G1's first eight; what stays bare is the loss arithmetic between the halves.
// MFMA -> vector hazards: the compiler does not see inside the asm statements, and gfx950 needs 11 wait states between an 8-pass XDL op and
// a vector instruction that reads its accumulators.  Every chain's reader sits two or more MFMA slots behind it: the slots' own
// instructions are the wait states, and the lint of the listing (below) counts them.
//
// LDS image of a 32-sample x 64-unit matrix of pieces: row m = 128 bytes, 8-byte slots ("quads": 4 units) XOR-swizzled by
//   f(m) = (m & 3) | ((m >> 2 ^ m >> 3) & 1) << 2 | ((m >> 1 ^ m >> 3) & 1) << 3
// -- conflict-free for the ds_write_b64 of 16 consecutive sample lanes, for the 4-row x 64-byte gathers of the 32x32x16 operands
// and for the 8-row x 32-byte gathers of the 16x16x32 operands.
#pragma once

namespace x3s {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int SW = 4;                    // waves per workgroup: one per SIMD, 512 registers each
constexpr int kPieceB = 32 * 128;        // one piece of an image: [32 samples][64 units] bf16
constexpr int kImgB = 3 * kPieceB;

struct SmemS {
    uint16_t W2p[3][H][H];               // as SmemX: rows = layer-2 units, k = layer-1 units (k-permuted, slots swizzled)
    uint16_t W2Tp[3][H][H];
    uint16_t W1p[3][H][16];
    float b1[H], b2[H], w3[H], w4[H];
    unsigned char img[SW][2][kImgB];     // per wave: [0] H1 pieces, [1] dH2 pieces, then dH1 pieces; at the end the reduction rows
};
static_assert(sizeof(SmemS) <= 160 * 1024, "LDS");
static_assert(offsetof(SmemS, img) % 128 == 0 && kImgB % 128 == 0, "image bases keep the low 7 address bits of a lane offset (the XOR swizzles)");
static_assert(sizeof(SmemS::img) >= 4 * ((Layout<16>::P_ACTOR + 6) & ~3) * sizeof(float), "reduction rows fit the images");
static_assert(sizeof(SmemS::img) / SW >= 96 * 64 * sizeof(float), "lane partials fit a wave's images");

// ---- the stream's building blocks.  Constraint letters: v = VGPR, a = AGPR (the compiler loads LDS / global operands straight into AGPRs)
// gfx950 does not interlock a vector-ALU write of a register against an MFMA that reads it as srcA / srcB in the NEXT instruction
// (tools/ubench/valu_mfma_hazard.hip: wrong products; one wait state cures it), and the compiler, which cannot see the MFMA inside
// the asm statement, may put a copy (v_mov, v_accvgpr_write / read) right in front of it.  A wait state in front of EVERY MFMA
// costs 17 % of the epoch (770 against 658 us: an s_nop takes an issue slot of the one wave), so: the MFMAs that open a phase --
// where operands arrive from compiler-issued loads and copies -- carry it (the ..G variants), inside a phase every operand is
// written by the stream itself at least one MFMA earlier, and tools/verify/mfma_hazard_lint.py checks the LISTING for both hazard
// kinds at every build of the test suite (tests/test_isa_lint_cpu.py): a compiler that places a copy elsewhere fails the test.
#ifndef X3S_GUARD
#define X3S_GUARD ""   // ("s_nop 0\n\t": the guard everywhere, for A/B runs)
#endif
#define X3S_G "s_nop 0\n\t"
#define X3S_MFMA32_V_AV(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(A), "v"(B))
#define X3S_MFMA32_V_AA(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(A), "a"(B))
#define X3S_MFMA32G_V_AV(acc, A, B) asm volatile(X3S_G "v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(A), "v"(B))
#define X3S_MFMA32G_V_AA(acc, A, B) asm volatile(X3S_G "v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(A), "a"(B))
#define X3S_MFMA32_VZ_AV(acc, A, B) asm volatile(X3S_G "v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "a"(A), "v"(B))
#define X3S_MFMA32_VZ_AA(acc, A, B) asm volatile(X3S_G "v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "a"(A), "a"(B))
#define X3S_MFMA32_A_AV(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(A), "v"(B))
#define X3S_MFMA32_AZ_AV(acc, A, B) asm volatile(X3S_G "v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&a"(acc) : "a"(A), "v"(B))
#define X3S_MFMA32_A_AA(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(A), "a"(B))
#define X3S_MFMA16_A_AA(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(A), "a"(B))
#define X3S_MFMA16_V_AA(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(A), "a"(B))
#define X3S_MFMA16G_V_AA(acc, A, B) asm volatile(X3S_G "v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(A), "a"(B))
#define X3S_MFMA16_A_VA(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(A), "a"(B))
#define X3S_MFMA16_V_VA(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(A), "a"(B))
#define X3S_MFMA16G_A_AA(acc, A, B) asm volatile(X3S_G "v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(A), "a"(B))
#define X3S_MFMA16_A_AV(acc, A, B) asm volatile(X3S_GUARD "v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "a"(A), "v"(B))

// sixty slots written out with constant slot numbers (a loop of this size is past the full-unroll limit, and a slot number that is not a
// constant turns the register arrays into scratch memory)
#define X3S_REP10(F, b) F(b + 0); F(b + 1); F(b + 2); F(b + 3); F(b + 4); F(b + 5); F(b + 6); F(b + 7); F(b + 8); F(b + 9);


// (a, b) -> p0 and the residuals: 5 instructions
__device__ __forceinline__ void split_a(unsigned& p0, float& ra, float& rb, const float a, const float b) {
    asm volatile("v_cvt_pk_bf16_f32 %0, %3, %4\n\t"
                 "v_lshlrev_b32 %1, 16, %0\n\t"
                 "v_and_b32 %2, 0xffff0000, %0\n\t"
                 "v_sub_f32 %1, %3, %1\n\t"
                 "v_sub_f32 %2, %4, %2"
                 : "=&v"(p0), "=&v"(ra), "=&v"(rb) : "v"(a), "v"(b));
}
// residuals -> p1, p2: 6 instructions
__device__ __forceinline__ void split_b(unsigned& p1, unsigned& p2, const float ra, const float rb) {
    float t0, t1;
    asm volatile("v_cvt_pk_bf16_f32 %0, %4, %5\n\t"
                 "v_lshlrev_b32 %2, 16, %0\n\t"
                 "v_and_b32 %3, 0xffff0000, %0\n\t"
                 "v_sub_f32 %2, %4, %2\n\t"
                 "v_sub_f32 %3, %5, %3\n\t"
                 "v_cvt_pk_bf16_f32 %1, %2, %3"
                 : "=&v"(p1), "=&v"(p2), "=&v"(t0), "=&v"(t1) : "v"(ra), "v"(rb));
}
// four accumulator registers: x = relu(x + b) -- 8 instructions (v_max_i32 on the bit pattern: relu_bits)
// four accumulator registers: h = relu(c) -- v_max_i32 on the bit pattern (relu_bits).  The bias is already in c: the accumulators of F1 /
// F2 START as the bias (as in the f32 pass), so sum and bias are rounded ONCE.  Adding the bias to the rounded sum afterwards -- rounds
// 1-5 did -- leaves a systematic error of ~2e-8 in the heads' pre-activations (the mean over samples does not average out; measured and
// modelled: tools/verify/x3_forward_error.py), which the actor's gradient sums amplify by their cancellation.
// (Accumulator values live on as SCALARS behind the MFMA chain: writing an asm result back into an element of the 16-register tuple
// costs a v_mov per value.)
__device__ __forceinline__ void relu4(float (&h)[16], const f32x16& c, const int g) {
    float y0, y1, y2, y3;
    asm volatile("v_max_i32 %0, %4, 0\n\tv_max_i32 %1, %5, 0\n\tv_max_i32 %2, %6, 0\n\tv_max_i32 %3, %7, 0"
                 : "=&v"(y0), "=&v"(y1), "=&v"(y2), "=&v"(y3) : "v"(c[4 * g]), "v"(c[4 * g + 1]), "v"(c[4 * g + 2]), "v"(c[4 * g + 3]));
    h[4 * g] = y0; h[4 * g + 1] = y1; h[4 * g + 2] = y2; h[4 * g + 3] = y3;
}
// four steps of the heads' dot products: z3 = fmaf(h[4 g + k], w3[k], z3), k = 0..3, and z4 alike (actor) -- the fmaf chain of the
// heads, one step after the other, as a block the caller places behind an MFMA  (8 / 4 instructions)
template <bool ACTOR>
__device__ __forceinline__ void dot4(float& z3, float& z4, const float (&h)[16], const int g, const v4f w3, const v4f w4) {
    if constexpr (ACTOR)
        asm volatile("v_fmac_f32 %0, %2, %6\n\tv_fmac_f32 %1, %2, %10\n\t"
                     "v_fmac_f32 %0, %3, %7\n\tv_fmac_f32 %1, %3, %11\n\t"
                     "v_fmac_f32 %0, %4, %8\n\tv_fmac_f32 %1, %4, %12\n\t"
                     "v_fmac_f32 %0, %5, %9\n\tv_fmac_f32 %1, %5, %13"
                     : "+v"(z3), "+v"(z4)
                     : "v"(h[4 * g]), "v"(h[4 * g + 1]), "v"(h[4 * g + 2]), "v"(h[4 * g + 3]), "v"(w3.x), "v"(w3.y), "v"(w3.z), "v"(w3.w),
                       "v"(w4.x), "v"(w4.y), "v"(w4.z), "v"(w4.w));
    else
        asm volatile("v_fmac_f32 %0, %1, %5\n\tv_fmac_f32 %0, %2, %6\n\tv_fmac_f32 %0, %3, %7\n\tv_fmac_f32 %0, %4, %8"
                     : "+v"(z3)
                     : "v"(h[4 * g]), "v"(h[4 * g + 1]), "v"(h[4 * g + 2]), "v"(h[4 * g + 3]), "v"(w3.x), "v"(w3.y), "v"(w3.z), "v"(w3.w));
}
// one value of the head's backward: h = H2 (>= 0) -> dH2 in place; the lane's partial sums  (7 / 5 instructions)
//   pw3 += h g3 ; pw4 += h g4 ; d = g3 w3 + g4 w4 (fma(g3, w3, g4 w4)) ; h = h > 0 ? d : 0 ; pb2 += h
template <bool ACTOR>
__device__ __forceinline__ void dh2_value(float& h, float& pw3, float& pw4, float& pb2, const float g3, const float g4, const float w3,
                                          const float w4) {
    float d;
    if constexpr (ACTOR)
        asm volatile("v_fmac_f32 %1, %0, %5\n\t"
                     "v_fmac_f32 %2, %0, %6\n\t"
                     "v_mul_f32 %4, %6, %8\n\t"
                     "v_fmac_f32 %4, %5, %7\n\t"
                     "v_cmp_lt_f32 vcc, 0, %0\n\t"
                     "v_cndmask_b32 %0, 0, %4, vcc\n\t"
                     "v_add_f32 %3, %3, %0"
                     : "+v"(h), "+v"(pw3), "+v"(pw4), "+v"(pb2), "=&v"(d) : "v"(g3), "v"(g4), "v"(w3), "v"(w4) : "vcc");
    else
        asm volatile("v_fmac_f32 %1, %0, %4\n\t"
                     "v_mul_f32 %3, %4, %5\n\t"
                     "v_cmp_lt_f32 vcc, 0, %0\n\t"
                     "v_cndmask_b32 %0, 0, %3, vcc\n\t"
                     "v_add_f32 %2, %2, %0"
                     : "+v"(h), "+v"(pw3), "+v"(pb2), "=&v"(d) : "v"(g3), "v"(w3) : "vcc");
}

// y_k = (bf16 half k of the words (w0, w1) != 0) ? x_k : 0 -- the relu mask from packed leading pieces: 8 instructions
__device__ __forceinline__ void mask4(float& y0, float& y1, float& y2, float& y3, const float x0, const float x1, const float x2,
                                      const float x3, const unsigned w0, const unsigned w1) {
    asm volatile("v_cmp_ne_u16 vcc, 0, %8\n\t"
                 "v_cndmask_b32 %0, 0, %4, vcc\n\t"
                 "v_cmp_lt_u32 vcc, 0xffff, %8\n\t"
                 "v_cndmask_b32 %1, 0, %5, vcc\n\t"
                 "v_cmp_ne_u16 vcc, 0, %9\n\t"
                 "v_cndmask_b32 %2, 0, %6, vcc\n\t"
                 "v_cmp_lt_u32 vcc, 0xffff, %9\n\t"
                 "v_cndmask_b32 %3, 0, %7, vcc"
                 : "=&v"(y0), "=&v"(y1), "=&v"(y2), "=&v"(y3) : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(w0), "v"(w1) : "vcc");
}

struct P3 {   // one k-step's operand: eight values as three packed pieces
    u32x4 p[3];
};

__device__ __forceinline__ int fswz(const int m) { return (m & 3) | ((((m >> 2) ^ (m >> 3)) & 1) << 2) | ((((m >> 1) ^ (m >> 3)) & 1) << 3); }

typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
__device__ __forceinline__ u32x2 tr_read(const unsigned char* p) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)p);
    u32x2 r;
    __builtin_memcpy(&r, &v, 8);
    return r;
}
__device__ __forceinline__ u32x4 cat(const u32x2 lo, const u32x2 hi) { return u32x4{lo.x, lo.y, hi.x, hi.y}; }

template <bool ACTOR>
__device__ __forceinline__ void pass_body(SmemS& sm, const float* __restrict__ params, const unsigned char* __restrict__ prep,
                                          const float* __restrict__ act, const float* __restrict__ logp_old,
                                          const float* __restrict__ rtg, const float* __restrict__ adv, long long M, float var,
                                          float clip, float inv_n, float* __restrict__ partial, float* __restrict__ stats_partial,
                                          const int block) {   // block: whose tiles this pass walks and whose row it writes (the wrapper pairs workgroups)
    using L = Layout<16>;
    constexpr int OFF_W1 = L::OFF_W1, OFF_B1 = L::OFF_B1, OFF_W2 = L::OFF_W2, OFF_B2 = L::OFF_B2, OFF_W3 = L::OFF_W3, OFF_B3 = L::OFF_B3,
                  OFF_W4 = L::OFF_W4, OFF_B4 = L::OFF_B4;
    constexpr int P = ACTOR ? L::P_ACTOR : L::P_CRITIC;
    constexpr int NT = 64 * SW, kTileBytes = XPad<16>::kTileBytes, kRowsBytes = XPad<16>::kRowsBytes;
    int tid = threadIdx.x;
    // (no instruction: the wrapper calls this body from a loop over its two phases, and everything below that depends on the thread
    // index alone would be computed once in front of that loop, for both nets, and held in registers -- or in scratch -- across it)
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lhi = lane >> 5, l15 = lane & 15, kk = lane >> 4;

    // ---- weights -> bf16 pieces in LDS (once per launch), as pass_body_x3
#ifdef X3S_EXPERIMENT_COPY_PROLOGUE
    // (timing experiment, profiles/x3s_fixed_cost.txt: what a launch would cost if the 55 KB of pieces arrived as a ready image -- a straight
    // 16-byte copy, global memory to LDS, here of as many bytes of `prep` -- instead of being split by every workgroup; results are wrong)
    for (int k = tid; k < (int)offsetof(SmemS, img) / 16; k += NT)
        reinterpret_cast<u32x4*>(&sm)[k] = reinterpret_cast<const u32x4*>(prep)[k + (ACTOR ? 0 : (int)offsetof(SmemS, img) / 16)];
#else
    for (int k = tid; k < H * H / 2; k += NT) {
        const int r = (2 * k) / H, c = (2 * k) % H;
        uint32_t p0, p1, p2;
        bf16x3::split_pair(params[OFF_W2 + r * H + c], params[OFF_W2 + r * H + c + 1], p0, p1, p2);
        const uint32_t pc[3] = {p0, p1, p2};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            *reinterpret_cast<uint32_t*>(&sm.W2p[i][0][0] + wslot(r, kpos(c))) = pc[i];
            (&sm.W2Tp[i][0][0])[wslot(c, kpos(r))] = (uint16_t)(pc[i] & 0xffffu);
            (&sm.W2Tp[i][0][0])[wslot(c + 1, kpos(r))] = (uint16_t)(pc[i] >> 16);
        }
    }
    for (int k = tid; k < H * 16 / 2; k += NT) {
        const int r = (2 * k) / 16, c = (2 * k) % 16;
        uint32_t p0, p1, p2;
        bf16x3::split_pair(params[OFF_W1 + r * 16 + c], params[OFF_W1 + r * 16 + c + 1], p0, p1, p2);
        *reinterpret_cast<uint32_t*>(&sm.W1p[0][r][c]) = p0;
        *reinterpret_cast<uint32_t*>(&sm.W1p[1][r][c]) = p1;
        *reinterpret_cast<uint32_t*>(&sm.W1p[2][r][c]) = p2;
    }
    if (tid < H) {
        sm.b1[tid] = params[OFF_B1 + tid];
        sm.b2[tid] = params[OFF_B2 + tid];
        sm.w3[tid] = params[OFF_W3 + tid];
        sm.w4[tid] = ACTOR ? params[OFF_W4 + tid] : 0.f;
    }
#endif
    const float b3 = params[OFF_B3];
    const float b4 = ACTOR ? params[OFF_B4] : 0.f;
    __syncthreads();

    // the wave's images as byte offsets into sm: H1 pieces at img0, dH2 (then dH1) pieces at img0 + kImgB -- the image base is folded
    // into every lane address below (it is a multiple of 128: the XOR swizzles of the low 7 bits pass through), the second image,
    // the piece and the k-step are immediate offsets of the DS instructions
    unsigned char* const smb = reinterpret_cast<unsigned char*>(&sm);
    const int img0 = (int)offsetof(SmemS, img) + wave * 2 * kImgB;
    constexpr int IMG_H = 0, IMG_D = kImgB;
    // ---- lane addresses (everything else is an immediate offset)
    // piece stores: lane (m = l31, lhi) owns the quads 8 t + 4 j + 2 b + lhi of row m
    const int st_base = img0 + l31 * 128 + ((fswz(l31) ^ lhi) << 3);
    auto st_off = [&](const int t, const int j, const int b) { return st_base ^ ((8 * t + 4 * j + 2 * b) << 3); };
    // 32x32x16 operand gathers: rows 16 s + 8 lhi + 4 rd + (l15 >> 2), quads 8 t + 4 ((lane >> 4) & 1) + (lane & 3)
    const int g_row = 8 * lhi + (l15 >> 2), g_quad = 4 * ((lane >> 4) & 1) + (lane & 3);
    const int g_base0 = img0 + g_row * 128 + ((g_quad ^ fswz(g_row)) << 3), g_base1 = img0 + (g_row + 4) * 128 + ((g_quad ^ fswz(g_row + 4)) << 3);
    auto g_off = [&](const int t, const int s, const int rd) { return ((rd ? g_base1 : g_base0) ^ (t << 6)) + s * 2048; };   // (two of the four are formed at the use)
    // 16x16x32 operand gathers: rows 8 kk + 4 rd + (l15 >> 2), quads 4 u + (lane & 3)
    const int h_row = 8 * kk + (l15 >> 2), h_quad = lane & 3;
    const int h_base0 = img0 + h_row * 128 + ((h_quad ^ fswz(h_row)) << 3), h_base1 = img0 + (h_row + 4) * 128 + ((h_quad ^ fswz(h_row + 4)) << 3);
    // weight rows: A operand of (row tile tt, k-step s, piece i)
    auto ldw = [&](const uint16_t* base, const int tt, const int s, const int i) {
        return *reinterpret_cast<const u32x4*>(base + i * H * H + wslot(32 * tt + l31, 16 * s + 8 * lhi));
    };
    const int vec_off = 4 * lhi;
    auto ldv = [&](const float* v, const int t, const int g) { return *reinterpret_cast<const v4f*>(v + 32 * t + 8 * g + vec_off); };

    // ---- accumulators that persist over this wave's tiles (zf: a zero the compiler cannot see through -- as `tid` above, registers of
    // zeros for both nets' accumulators would be set up in front of the wrapper's loop and held across it)
    float zf = 0.f;
    asm volatile("" : "+v"(zf));
    f32x16 aW2[2][2];
    v4f aW1[4], aB1[4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) aW2[a][b][r] = zf;
#pragma unroll
    for (int u = 0; u < 4; ++u) aW1[u] = aB1[u] = v4f{zf, zf, zf, zf};
    float pb2[2][16], pw3[2][16], pw4[2][16];   // per-lane partial sums over the tiles: db2, dW3, dW4 of the lane's 32 units
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) pb2[t][r] = pw3[t][r] = pw4[t][r] = zf;
    float adb3 = zf, adb4 = zf, st0 = zf, st1 = zf, st2 = zf, st3 = zf;
    float stv = zf;   // (the *_var twin: the sum of navppo_dlogvar_term, column 3 of the workgroup's statistics row)
    (void)stv;
    // (no instruction: a use of dW2's accumulators in the middle of the phases that do not touch them, so that the register allocator
    // does not park them elsewhere for those phases and fetch them back for G2 -- 96 copies per tile; dW1's likewise: moved aside over
    // F2 and back in front of G1, one copy right in front of its MFMA)
    auto keep_w2 = [&]() {
        asm volatile("" : "+a"(aW2[0][0]), "+a"(aW2[0][1]), "+a"(aW2[1][0]), "+a"(aW2[1][1]), "+a"(aW1[0]), "+a"(aW1[1]), "+a"(aW1[2]), "+a"(aW1[3]));
    };
    u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};   // bf16 1.0 in every k-slot
    asm volatile("" : "+a"(ones));   // lives in AGPRs for the whole launch

    const long long n_tiles = (M + 31) / 32;
    const long long gw = (long long)block * SW + wave, stride = (long long)gridDim.x * SW;
    // Operands that come from global memory -- the tile's observation rows (F1's B operand) and columns (G1's B operand), pre-split by
    // mlp64_split_obs -- are requested by asm loads straight into AGPRs (a compiler-issued load lands in vector registers, which are full,
    // and is copied over right in front of the MFMA: the hazard above) long before their use; `landed` is their s_waitcnt, placed a
    // few thousand cycles later and tied to the registers so that nothing reads or copies them before.  (Hidden loads are safe for the
    // compiler's own vmcnt bookkeeping: loads return in order, extra outstanding ones only make its waits longer.)
    u32x4 xp[3], xbn[3];   // rows of the tile whose F1 runs next ; columns of the tile whose G1 runs next (G1 runs one tile late)
    auto keep_cols = [&]() { asm volatile("" : "+a"(xbn[0]), "+a"(xbn[1]), "+a"(xbn[2])); };   // (as keep_w2, between F2 and G1: landed, not yet re-requested)
    float pre_a0 = 0.f, pre_a1 = 0.f, pre_lp = 0.f, pre_t = 0.f;
    // Each request is placed behind the last reader of the registers it lands in (F1 for the rows, G1 for the columns, the heads for the
    // sample's scalars: all three ride on B2's slots), so no copy of them is kept; `landed` sits in front of F1, some 85 MFMA slots
    // later.  All tiles are clamped by the caller: always valid.
    auto request_rows = [&](long long t) {
        asm volatile("" : "+s"(t));   // (the address arithmetic stays in this slot: hoisted, it stands in front of B2's first MFMA)
        const unsigned char* r = prep + (size_t)t * kTileBytes + ((l31 * 3) * 16 + 8 * lhi) * 2;   // rows past the batch are zero in `prep`
        asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:32\n\tglobal_load_dwordx4 %2, %3, off offset:64"
                     : "=a"(xp[0]), "=a"(xp[1]), "=a"(xp[2]) : "v"(r));
    };
    auto request_cols = [&](const long long t) {
        const unsigned char* c = prep + (size_t)t * kTileBytes + kRowsBytes + (l15 * 32 + 8 * kk) * 2;   // lane (f = l15, kk): samples 8 kk .. + 7
        asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:1024\n\tglobal_load_dwordx4 %2, %3, off offset:2048"
                     : "=a"(xbn[0]), "=a"(xbn[1]), "=a"(xbn[2]) : "v"(c));
    };
    auto request_scalars = [&](const long long t) {
        if constexpr (ACTOR) {
            const long long m = t * 32 + l31;
            if (m < M) {
                const float2 a = reinterpret_cast<const float2*>(act)[m];
                pre_a0 = a.x;
                pre_a1 = a.y;
                pre_lp = logp_old[m];
                pre_t = adv[m];
            }
        } else {
            // No branch in the critic's stream: with one here and its short loss block if-converted, the compiler lays the loop out
            // rotated (it then starts in the middle of B2).  A lane past the batch reads the last sample's return instead, which is used
            // under `valid` only.  The empty statement pins the address arithmetic to this slot (it would be hoisted to the front of B2).
            int l = l31;
            long long ts = t;
            asm volatile("" : "+v"(l), "+s"(ts));
            const long long m = ts * 32 + l;
            pre_t = rtg[m < M ? m : M - 1];
        }
    };
    auto landed = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" : "+a"(xp[0]), "+a"(xp[1]), "+a"(xp[2]), "+a"(xbn[0]), "+a"(xbn[1]), "+a"(xbn[2]));
    };
    static_assert(kTileBytes == 6144 && kRowsBytes == 3072, "offsets of the asm loads: pieces 32 bytes apart in a row, 1024 in the columns");

    // G1 of the tile whose dH1 pieces are in imgD: dW1 += dH1^T X (16x16x32, one k-step), db1 += dH1^T 1 -- as a stream of 36 MFMAs
    // (step k of 0..35: unit pair k / 18) that the caller places one by one behind its vector work; operands gathered up front
    struct G1Ops {
        P3 da[4];
    };
    // pair q of 0..11: (unit tile u = q / 3, piece i = q % 3) -- two 8-byte gathers; the caller spreads the twelve over MFMA slots
    auto g1_gather_pair = [&](G1Ops& o, const int q, const int hb0, const int hb1) {
        const int u = q / 3, i = q % 3;
        o.da[u].p[i] = cat(tr_read(smb + (hb0 ^ (u << 5)) + IMG_D + i * kPieceB), tr_read(smb + (hb1 ^ (u << 5)) + IMG_D + i * kPieceB));
    };
    auto g1_step = [&](const int k, const G1Ops& o, const u32x4 (&xb)[3], const bool guard = false) {
        const int t1 = k / 18, q = k % 18, u = 2 * t1 + (q & 1), e = q >> 1;   // e of 0..8: the pair's e-th product
        // products in the order of mma6_acc16_2 (small terms first), the ones-products of db1 between them
        constexpr int kind[9] = {0, 1, 0, 0, 1, 0, 0, 1, 0};    // 1: ones product
        constexpr int ai[9] = {2, 2, 1, 0, 1, 1, 0, 0, 0};      // piece of dH1
        constexpr int bi[9] = {0, 0, 1, 2, 0, 0, 1, 0, 0};      // piece of X (kind 0)
        if (guard) {   // (the tail after the tile loop: the compiler moves the accumulators around there -- every MFMA waits one state)
            if (kind[e]) { X3S_MFMA16G_V_AA(aB1[u], o.da[u].p[ai[e]], ones); }
            else { X3S_MFMA16G_A_AA(aW1[u], o.da[u].p[ai[e]], xb[bi[e]]); }
        } else {
            // dH1's pieces: accumulator registers in the actor's stream; the critic's has the vector registers of the actor's second head
            // free and keeps them there (in accumulator registers the allocator parks some of them in vector registers anyway and
            // copies them back right in front of their MFMA: the hazard of the lint)
            if (ACTOR) {
                if (kind[e]) { X3S_MFMA16_V_AA(aB1[u], o.da[u].p[ai[e]], ones); }
                else { X3S_MFMA16_A_AA(aW1[u], o.da[u].p[ai[e]], xb[bi[e]]); }
            } else {
                if (kind[e]) { X3S_MFMA16_V_VA(aB1[u], o.da[u].p[ai[e]], ones); }
                else { X3S_MFMA16_A_VA(aW1[u], o.da[u].p[ai[e]], xb[bi[e]]); }
            }
        }
    };
    // one k-step's pieces into both 8-byte slots of its two quads (6 stores)
    auto store_pieces = [&](const int img, const int t, const int j, const P3& q) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            *reinterpret_cast<u32x2*>(smb + st_off(t, j, 0) + img + i * kPieceB) = u32x2{q.p[i].x, q.p[i].y};
            *reinterpret_cast<u32x2*>(smb + st_off(t, j, 1) + img + i * kPieceB) = u32x2{q.p[i].z, q.p[i].w};
        }
    };
    // the eight values c[8 j .. 8 j + 7] -> pieces, as 8 blocks (block b of 0..7: pair b >> 1, first / second half)
    struct SplitState {
        float ra[4], rb[4];
    };
    auto split_block = [&](const float (&c)[16], const int j, const int b, P3& q, SplitState& ss) {
        const int pr = b >> 1;
        if ((b & 1) == 0) {
            unsigned p0;
            split_a(p0, ss.ra[pr], ss.rb[pr], c[8 * j + 2 * pr], c[8 * j + 2 * pr + 1]);
            q.p[0][pr] = p0;
        } else {
            unsigned p1, p2;
            split_b(p1, p2, ss.ra[pr], ss.rb[pr]);
            q.p[1][pr] = p1;
            q.p[2][pr] = p2;
        }
    };

    // ---- layer 1 runs one tile AHEAD of the rest of the stream: F1 of the next tile sits between G2's 36th and 37th MFMA, and the vector
    // work around it -- the b1 start of its accumulators and the W1 pieces in front, relu1, the b2 start of F2's accumulators, the split
    // of H1's k-step 0 and F2's first weight rows behind -- shares the 60 slots of G2 + F1 with the mask, split and stores of dH1 (the
    // table at G2).  So c2, h1, hb[0] and wn live across the back-edge and the loop starts at F2's first MFMA.  The prologue runs the
    // same slots without G2 for the wave's first tile; the last iteration runs them on a clamped (valid) tile and drops the result.
    // F1 runs c1[0]'s six products, then c1[1]'s (each accumulator sees its products in the order it always did): relu1 of c1[0] and the
    // split, which reads c1[0] only, start behind c1[1]'s MFMAs.
    f32x16 c1[2], c2[2];
    float h1[2][16];   // H1 = relu(b1 + ..): the values the split reads
    P3 hb[4];          // H1's pieces per k-step; [0] is made ahead
    u32x4 wn[2][3], wa[2][3];
    SplitState ss1;
    auto g2_step = [&](const int k, const P3 (&dA)[2][2], const P3 (&hB)[2][2], f32x16 (&aW2)[2][2]) {
        const int t2 = k / 24, sk = (k / 12) & 1, e = (k % 12) >> 1, t1 = k & 1;
        constexpr int ai[6] = {2, 1, 0, 1, 0, 0}, bi[6] = {0, 1, 2, 0, 1, 0};   // small terms first
        X3S_MFMA32_A_AA(aW2[t2][t1], dA[t2][sk].p[ai[e]], hB[t1][sk].p[bi[e]]);
    };
    auto b1_to_c1 = [&](const int q) {
        const v4f b = ldv(sm.b1, q >> 2, q & 3);
        c1[q >> 2][4 * (q & 3)] = b.x; c1[q >> 2][4 * (q & 3) + 1] = b.y; c1[q >> 2][4 * (q & 3) + 2] = b.z; c1[q >> 2][4 * (q & 3) + 3] = b.w;
    };
    auto b2_to_c2 = [&](const int q) {
        const v4f b = ldv(sm.b2, q >> 2, q & 3);
        c2[q >> 2][4 * (q & 3)] = b.x; c2[q >> 2][4 * (q & 3) + 1] = b.y; c2[q >> 2][4 * (q & 3) + 2] = b.z; c2[q >> 2][4 * (q & 3) + 3] = b.w;
    };
    auto ld_wa = [&](const int t, const int i) { wa[t][i] = *reinterpret_cast<const u32x4*>(&sm.W1p[i][32 * t + l31][8 * lhi]); };
    auto ld_wn = [&](const int t, const int i) { wn[t][i] = ldw(&sm.W2p[0][0][0], t, 0, i); };
    auto f1_mfma = [&](const int j) {   // j of 0..11: accumulator j / 6, its e-th product
        const int t = j / 6, e = j % 6;
        constexpr int wi[6] = {2, 1, 0, 1, 0, 0}, xi[6] = {0, 1, 2, 0, 1, 0};
        if (e == 0) { X3S_MFMA32G_V_AA(c1[t], wa[t][wi[e]], xp[xi[e]]); } else { X3S_MFMA32_V_AA(c1[t], wa[t][wi[e]], xp[xi[e]]); }
    };
    auto ahead_work = [&](const int n, const bool alone) {
        if (n == 11 || n == 13) ld_wa(0, (n - 11) / 2);
        if (n == 15 || n == 17) ld_wa(1, (n - 15) / 2);
        if (n == 19) { ld_wa(0, 2); ld_wa(1, 2); }
        if (n >= 22 && n <= 29) b1_to_c1(n - 22);
        if (n == 42) { ld_wn(0, 0); ld_wn(1, 0); ld_wn(0, 1); ld_wn(1, 1); }
        if (n == 43) {
            ld_wn(0, 2); ld_wn(1, 2);
            if (alone) asm volatile("s_nop 7" : "+v"(c1[0]));   // (the prologue has no dH1 work in these slots to make up the wait states)
            relu4(h1[0], c1[0], 0);
        }
        if (n == 44) relu4(h1[0], c1[0], 1);
        if (n >= 45 && n <= 52) { split_block(h1[0], 0, n - 45, hb[0], ss1); b2_to_c2(n - 45); }
        if (n == 53) relu4(h1[0], c1[0], 2);
        if (n == 54) relu4(h1[0], c1[0], 3);
        if (n >= 55 && n <= 58) relu4(h1[1], c1[1], n - 55);
    };

    // imgD starts as zeros: the first tile's "previous G1" then adds nothing (the stream below has no special first iteration)
    for (int k = lane; k < kImgB / 16; k += 64) reinterpret_cast<u32x4*>(smb + img0 + IMG_D)[k] = u32x4{0u, 0u, 0u, 0u};
    bool have_prev = false;
    // A wave with tiles: the look-ahead, the tile loop and the last tile's G1 in ONE block (closed behind that G1; the loop keeps its
    // indentation).  Closed in front of the loop, the operands requested here met "not requested" where the paths join, and the
    // compiler carried such registers from one phase of the wrapper's loop into the next, through both tile loops.
    if (gw < n_tiles) {
        request_rows(gw);
        request_cols(gw);   // (the first tile's "previous" columns: any finite values -- they meet zero pieces)
        request_scalars(gw);
        auto slot = [&](const int n) {
            if (n == 36) landed();
            if (n >= 36 && n < 48) f1_mfma(n - 36);
            ahead_work(n, true);
        };
        X3S_REP10(slot, 10) X3S_REP10(slot, 20) X3S_REP10(slot, 30) X3S_REP10(slot, 40) X3S_REP10(slot, 50)
    for (long long tile = gw; tile < n_tiles; tile += stride) {
        const bool valid = tile * 32 + l31 < M;
        const float cur_a0 = pre_a0, cur_a1 = pre_a1, cur_lp = pre_lp, cur_t = pre_t;
        const long long tile1 = tile + stride < n_tiles ? tile + stride : tile;       // the tile whose F1 runs behind this one's G2

        // ================================================================ F2: H2^T = relu(b2 + W2 H1^T); H1 split once, k-step s = (t1, j)
        G1Ops g1o;
        float h2[2][16];   // H2, then dH2 in place
        float z3 = 0.f, z4 = 0.f;   // the heads' pre-activations: sums over the lane's 32 units, c2[0]'s half first
        {
            u32x4 wk[4][2];   // the leading weight pieces again, for the big terms
            SplitState ss;    // (k-step 0 was split a tile ahead: ahead_work)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                u32x4 w[2][3];
#pragma unroll
                for (int i = 0; i < 3; ++i) { w[0][i] = wn[0][i]; w[1][i] = wn[1][i]; }
                keep_w2();
                keep_cols();
                // the stream of k-step s: 10 MFMAs; behind them the split of k-step s + 1 (8 blocks), this step's piece stores and the
                // next step's weight rows
                auto filler = [&](const int slot) {
                    if (slot >= 1 && slot <= 8) split_block(h1[(s + 1) >> 1], (s + 1) & 1, slot - 1, hb[s + 1], ss);
                    if (slot == 0 || slot == 4 || slot == 9) {
                        const int i = slot == 0 ? 0 : slot == 4 ? 1 : 2;
                        wn[0][i] = ldw(&sm.W2p[0][0][0], 0, s + 1, i);
                        wn[1][i] = ldw(&sm.W2p[0][0][0], 1, s + 1, i);
                    }
                    if (slot == 9) store_pieces(IMG_H, s >> 1, s & 1, hb[s]);
                };
                if (s == 0) { X3S_MFMA32G_V_AV(c2[0], w[0][2], hb[s].p[0]); } else { X3S_MFMA32_V_AV(c2[0], w[0][2], hb[s].p[0]); }
                filler(0);
                if (s == 0) { X3S_MFMA32G_V_AV(c2[1], w[1][2], hb[s].p[0]); } else { X3S_MFMA32_V_AV(c2[1], w[1][2], hb[s].p[0]); }
                filler(1);
                X3S_MFMA32_V_AV(c2[0], w[0][1], hb[s].p[1]); filler(2);
                X3S_MFMA32_V_AV(c2[1], w[1][1], hb[s].p[1]); filler(3);
                X3S_MFMA32_V_AV(c2[0], w[0][0], hb[s].p[2]); filler(4);
                X3S_MFMA32_V_AV(c2[1], w[1][0], hb[s].p[2]); filler(5);
                X3S_MFMA32_V_AV(c2[0], w[0][1], hb[s].p[0]); filler(6);
                X3S_MFMA32_V_AV(c2[1], w[1][1], hb[s].p[0]); filler(7);
                X3S_MFMA32_V_AV(c2[0], w[0][0], hb[s].p[1]); filler(8);
                X3S_MFMA32_V_AV(c2[1], w[1][0], hb[s].p[1]); filler(9);
            }
            // k-step 3 and the big terms, c2[0]'s nine and then c2[1]'s (each accumulator sees its products in the order it always did):
            // relu2 of c2[0] and its half of the heads' dot products start behind c2[1]'s MFMAs instead of waiting behind the chain.
            //   MFMA    0 1       2..8          |  9 10      11           12 13                      14..17
            //   c2[0]:  wk[.][0]  G1's gathers  |  c2[1]: wk[.][1]  store hb[3]  relu2 of c2[0], w3 / w4  z3 / z4 of c2[0]'s units
            // (G1's operands are those of the PREVIOUS tile: its dH1 pieces are still in imgD.  relu2 sits 4 MFMAs and 12 loads / stores
            // behind c2[0]'s last product: the listing is linted.)
            int hb0 = h_base0, hb1 = h_base1;
            asm volatile("" : "+v"(hb0), "+v"(hb1));   // the eight gather addresses are formed here, per tile: not hoisted into eight registers
            int gq = 0;
            auto gather = [&]() { g1_gather_pair(g1o, gq, hb0, hb1); ++gq; };
            auto ld_wk = [&](const int s, const int t) { wk[s][t] = ldw(&sm.W2p[0][0][0], t, s, 0); };
            keep_w2();
            keep_cols();
            X3S_MFMA32_V_AV(c2[0], wn[0][2], hb[3].p[0]); ld_wk(0, 0); ld_wk(1, 0);
            X3S_MFMA32_V_AV(c2[0], wn[0][1], hb[3].p[1]); ld_wk(2, 0); ld_wk(3, 0);
            X3S_MFMA32_V_AV(c2[0], wn[0][0], hb[3].p[2]); gather(); gather();
            X3S_MFMA32_V_AV(c2[0], wn[0][1], hb[3].p[0]); gather(); gather();
            X3S_MFMA32_V_AV(c2[0], wn[0][0], hb[3].p[1]); gather(); gather();
            X3S_MFMA32_V_AV(c2[0], wk[0][0], hb[0].p[0]); gather(); gather();
            X3S_MFMA32_V_AV(c2[0], wk[1][0], hb[1].p[0]); gather(); gather();
            X3S_MFMA32_V_AV(c2[0], wk[2][0], hb[2].p[0]); gather();
            X3S_MFMA32_V_AV(c2[0], wk[3][0], hb[3].p[0]); gather();
            v4f hw3[4], hw4[4] = {};   // w3 / w4 at the lane's units of c2[0]
            auto ld_hw = [&](const int g) {   // (each two slots ahead of its use: the vector registers are full here)
                hw3[g] = ldv(sm.w3, 0, g);
                if (ACTOR) hw4[g] = ldv(sm.w4, 0, g);
            };
            X3S_MFMA32_V_AV(c2[1], wn[1][2], hb[3].p[0]); ld_wk(0, 1); ld_wk(1, 1); ld_hw(0);
            X3S_MFMA32_V_AV(c2[1], wn[1][1], hb[3].p[1]); ld_wk(2, 1); ld_wk(3, 1); ld_hw(1);
            X3S_MFMA32_V_AV(c2[1], wn[1][0], hb[3].p[2]); store_pieces(IMG_H, 1, 1, hb[3]);
            X3S_MFMA32_V_AV(c2[1], wn[1][1], hb[3].p[0]); relu4(h2[0], c2[0], 0); relu4(h2[0], c2[0], 1);
            X3S_MFMA32_V_AV(c2[1], wn[1][0], hb[3].p[1]); relu4(h2[0], c2[0], 2); relu4(h2[0], c2[0], 3);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                X3S_MFMA32_V_AV(c2[1], wk[s][1], hb[s].p[0]);
                dot4<ACTOR>(z3, z4, h2[0], s, hw3[s], hw4[s]);
                if (s < 2) ld_hw(s + 2);
            }
        }

        // ================================================================ heads, loss, dH2 (in place), the lane's share of db2 / dW3 / dW4;
        // behind the vector work: G1 of the PREVIOUS tile, 36 MFMAs placed one by one.  c2[1]'s half of relu2 and of the dot products
        // rides on the first eight; its relu sits three of them (and the loads between) behind c2[1]'s last product: no s_nop.
        int g1k = 0;
        keep_w2();
        {
            v4f hw3[4], hw4[4] = {};
            g1_step(g1k++, g1o, xbn);
            hw3[0] = ldv(sm.w3, 1, 0); hw3[1] = ldv(sm.w3, 1, 1);
            if (ACTOR) { hw4[0] = ldv(sm.w4, 1, 0); hw4[1] = ldv(sm.w4, 1, 1); }
            g1_step(g1k++, g1o, xbn);
            hw3[2] = ldv(sm.w3, 1, 2); hw3[3] = ldv(sm.w3, 1, 3);
            if (ACTOR) { hw4[2] = ldv(sm.w4, 1, 2); hw4[3] = ldv(sm.w4, 1, 3); }
            g1_step(g1k++, g1o, xbn);
            relu4(h2[1], c2[1], 0); relu4(h2[1], c2[1], 1);
            g1_step(g1k++, g1o, xbn);
            relu4(h2[1], c2[1], 2); relu4(h2[1], c2[1], 3);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                g1_step(g1k++, g1o, xbn);
                dot4<ACTOR>(z3, z4, h2[1], g, hw3[g], hw4[g]);
            }
        }
        float g3 = 0.f, g4 = 0.f;
        {
            z3 += __shfl_xor(z3, 32, 64);
            if (ACTOR) z4 += __shfl_xor(z4, 32, 64);
            const float own = (lhi == 0) ? 1.f : 0.f;   // statistics are counted once per sample
            if (valid) {
                z3 += b3;
                z4 += b4;
#ifdef MLP64_DEBUG_Z   // (dev builds only, tools/verify/x3_forward_error.py: the heads' pre-activations into unused rows of the workspace)
                if (lhi == 0) {
                    float* const dbg = partial + (size_t)200 * P;
                    dbg[tile * 32 + l31] = z3;
                    if (ACTOR) dbg[M + tile * 32 + l31] = z4;
                }
#endif
                if (ACTOR) {
                    const float mu0 = 1.0f / (1.0f + expf(-z3));   // torch.sigmoid, net_actor.py:185
                    const float mu1 = tanhf(z4);                    // net_actor.py:186
                    const float d0 = cur_a0 - mu0, d1 = cur_a1 - mu1;
                    const float lp = -0.5f * ((d0 * d0 + d1 * d1) / var) - 1.8378770664093453f - logf(var);   // ppo.py:734-735
                    const float lr = lp - cur_lp;
                    const float ratio = expf(lr);                  // ppo.py:316
                    const float A = cur_t;
                    const float s1 = ratio * A;                     // ppo.py:319
                    const float rc = fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
                    const float s2 = rc * A;                        // ppo.py:320
                    st0 += own * -fminf(s1, s2);                    // ppo.py:342
                    st2 += own * ((ratio - 1.0f) - lr);             // approx KL, ppo.py:326
                    st3 += (fabsf(ratio - 1.0f) > clip) ? own : 0.f;  // clip fraction, ppo.py:335
                    const bool inside = (ratio >= 1.0f - clip) && (ratio <= 1.0f + clip);
                    const float dL_dratio = (inside || s1 < s2) ? -A : 0.f;
                    const float dL_dlp = dL_dratio * ratio * inv_n;
                    if constexpr (kNavppoVarTu) stv += own * navppo_dlogvar_term(dL_dlp, d0, d1, var);
                    g3 = dL_dlp * (d0 / var) * (mu0 * (1.0f - mu0));
                    g4 = dL_dlp * (d1 / var) * (1.0f - mu1 * mu1);
                } else {
                    const float e = z3 - cur_t;                     // critic(obs).squeeze(), ppo.py:724
                    st1 += own * (e * e);                           // MSELoss, ppo.py:343
                    g3 = 2.0f * e * inv_n;
                }
            }
            adb3 += own * g3;
            adb4 += own * g4;
#ifdef MLP64_DEBUG_Z
            if (valid && lhi == 0) {
                float* const dbg = partial + (size_t)200 * P;
                dbg[2 * M + tile * 32 + l31] = g3;
                if (ACTOR) dbg[3 * M + tile * 32 + l31] = g4;
            }
#endif
        }
        // dH2[m][u] = [H2 > 0] (g3 w3[u] + g4 w4[u]) in place; the lane's dW3 / dW4 / db2 sums; the rest of G1 behind it
        {
            v4f wn3 = ldv(sm.w3, 0, 0), wn4 = ACTOR ? ldv(sm.w4, 0, 0) : v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int t = q >> 2, g = q & 3;
                const v4f w = wn3, v = wn4;
                if (q < 7) {
                    wn3 = ldv(sm.w3, (q + 1) >> 2, (q + 1) & 3);
                    if (ACTOR) wn4 = ldv(sm.w4, (q + 1) >> 2, (q + 1) & 3);
                }
                const float wv3[4] = {w.x, w.y, w.z, w.w}, wv4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * g + j;
                    dh2_value<ACTOR>(h2[t][r], pw3[t][r], pw4[t][r], pb2[t][r], g3, g4, wv3[j], wv4[j]);
                    if (g1k < 36 && (j & 1)) g1_step(g1k++, g1o, xbn);
                }
                if (g1k < 36 && (g & 1)) g1_step(g1k++, g1o, xbn);
            }
        }
        // (8 + 16 + 4 so far; the last eight carry the split of dH2's k-step 0 in front of B2)

        // ================================================================ B2: dH1^T = (W2^T dH2^T) . [H1 > 0]; dH2 split once, k-step s = (t2, j)
        f32x16 c3[2];
        P3 hB[2][2], dA[2][2];   // G2's operands, [unit tile][sample k-step]: gathered behind B2's stream
        u32x2 mw[8];           // the leading piece of H1 at the lane's own slots: the relu mask of layer 1
        // [H1 > 0] from the leading piece of H1, read back from the lane's own slots of the image (keeping H1 itself would hold 32
        // vector registers through F2 / B2, where the file is full): bf16(H1) != 0.  Differs from H1 > 0 only for
        // 0 < H1 < 2^-126 (the bf16 conversion flushes / rounds such values to zero) -- not a value a sum of O(1) terms takes.
        float d1[2][16];   // dH1 = (W2^T dH2^T) . [H1 > 0]
        auto d_mask = [&](const int k) {   // k = (t, j, b): registers 8 j + 4 b .. + 3 of c3[t]
            const int t = k >> 2, r0 = 8 * ((k >> 1) & 1) + 4 * (k & 1);
            mask4(d1[t][r0], d1[t][r0 + 1], d1[t][r0 + 2], d1[t][r0 + 3], c3[t][r0], c3[t][r0 + 1], c3[t][r0 + 2], c3[t][r0 + 3], mw[k].x, mw[k].y);
        };
        {
            P3 db[4];
            u32x4 wk[4][2], wt[2][3];
            SplitState ss;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                wt[0][i] = ldw(&sm.W2Tp[0][0][0], 0, 0, i);
                wt[1][i] = ldw(&sm.W2Tp[0][0][0], 1, 0, i);
            }
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                g1_step(g1k++, g1o, xbn);
                split_block(h2[0], 0, b, db[0], ss);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                u32x4 w[2][3];
#pragma unroll
                for (int i = 0; i < 3; ++i) { w[0][i] = wt[0][i]; w[1][i] = wt[1][i]; }
                keep_w2();
                auto filler = [&](const int slot) {
                    // G1 has read the columns, the heads the sample's scalars: the next ones are requested here
                    if (s == 0 && slot == 0) request_cols(tile);
                    if (s == 0 && slot == 1) request_rows(tile1);
                    if (s == 3 && slot == 0) request_scalars(tile1);
                    if (s < 3 && slot >= 1 && slot <= 8) split_block(h2[(s + 1) >> 1], (s + 1) & 1, slot - 1, db[s + 1], ss);
                    if (s == 3 && slot < 8) wk[slot >> 1][slot & 1] = ldw(&sm.W2Tp[0][0][0], slot & 1, slot >> 1, 0);
                    // H1's side of G2 (imgH is complete since F2): pair q = (t, sk, i) of 0..11, three per k-step
                    if (slot == 2 || slot == 5 || slot == 8) {
                        const int q = 3 * s + (slot - 2) / 3, t = q / 6, sk = (q / 3) & 1, i = q % 3;
                        hB[t][sk].p[i] = cat(tr_read(smb + g_off(t, sk, 0) + IMG_H + i * kPieceB), tr_read(smb + g_off(t, sk, 1) + IMG_H + i * kPieceB));
                    }
                    if (s == 3 && (slot == 3 || slot == 4 || slot == 6 || slot == 7)) {   // the mask words: two 8-byte reads per slot
                        const int k0 = 2 * (slot - 3 - (slot > 4));
#pragma unroll
                        for (int k = k0; k < k0 + 2; ++k)
                            mw[k] = *reinterpret_cast<const u32x2*>(smb + st_off(k >> 2, (k >> 1) & 1, k & 1) + IMG_H);
                    }
                    if (s < 3 && (slot == 0 || slot == 4 || slot == 9)) {
                        const int i = slot == 0 ? 0 : slot == 4 ? 1 : 2;
                        wt[0][i] = ldw(&sm.W2Tp[0][0][0], 0, s + 1, i);
                        wt[1][i] = ldw(&sm.W2Tp[0][0][0], 1, s + 1, i);
                    }
                    if (slot == 9) store_pieces(IMG_D, s >> 1, s & 1, db[s]);
                };
                if (s == 0) { X3S_MFMA32_VZ_AV(c3[0], w[0][2], db[s].p[0]); } else { X3S_MFMA32_V_AV(c3[0], w[0][2], db[s].p[0]); }
                filler(0);
                if (s == 0) { X3S_MFMA32_VZ_AV(c3[1], w[1][2], db[s].p[0]); } else { X3S_MFMA32_V_AV(c3[1], w[1][2], db[s].p[0]); }
                filler(1);
                X3S_MFMA32_V_AV(c3[0], w[0][1], db[s].p[1]); filler(2);
                X3S_MFMA32_V_AV(c3[1], w[1][1], db[s].p[1]); filler(3);
                X3S_MFMA32_V_AV(c3[0], w[0][0], db[s].p[2]); filler(4);
                X3S_MFMA32_V_AV(c3[1], w[1][0], db[s].p[2]); filler(5);
                X3S_MFMA32_V_AV(c3[0], w[0][1], db[s].p[0]); filler(6);
                X3S_MFMA32_V_AV(c3[1], w[1][1], db[s].p[0]); filler(7);
                X3S_MFMA32_V_AV(c3[0], w[0][0], db[s].p[1]); filler(8);
                X3S_MFMA32_V_AV(c3[1], w[1][0], db[s].p[1]); filler(9);
            }
            // the big terms, c3[0]'s four and then c3[1]'s (each accumulator sees its products in the order it always did), so that the relu
            // mask of c3[0] can start behind c3[1]'s last two.  Behind the first six: dH2's side of G2 (every piece store of imgD is
            // issued), pair q = (t, sk, i)
            int dq = 0;
            auto gather_d = [&]() {
                const int t = dq / 6, sk = (dq / 3) & 1, i = dq % 3;
                dA[t][sk].p[i] = cat(tr_read(smb + g_off(t, sk, 0) + IMG_D + i * kPieceB), tr_read(smb + g_off(t, sk, 1) + IMG_D + i * kPieceB));
                ++dq;
            };
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                X3S_MFMA32_V_AV(c3[0], wk[s][0], db[s].p[0]);
                gather_d(); gather_d();
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                X3S_MFMA32_V_AV(c3[1], wk[s][1], db[s].p[0]);
                if (s < 2) { gather_d(); gather_d(); }
                else d_mask(s - 2);   // 15 wait states behind c3[0]'s last MFMA: eight reads and three MFMAs (the listing is linted)
            }
        }

        // ================================================================ G2: dW2 += dH2^T H1 over the tile's samples, both operands gathered
        // transposed from the piece images, with F1 of the next tile between its 36th and 37th MFMA.  Behind the 60 slots: the rest of
        // the relu mask of layer 1 on dH1 (c3[0]'s half first: the split starts with it), the split, the piece stores (into imgD: every
        // gather of dH2 is issued before the first of them), and layer 1's vector work of the next tile (ahead_work).
        //   slot   0 1   2..9    10     11..18  19     20 21   22..29  30     31 32   33..40  41     42..59
        //   dH1    mask  split 0 store  split 1 store  mask    split 2 store  mask    split 3 store
        //   ahead                       W1 pieces (6)          b1 (8)                                W2 rows, relu1, split, b2
        {
            P3 eb[4];
            SplitState ss;
            auto d_work = [&](const int n) {
                if (n == 0 || n == 1) d_mask(2 + n);
                if (n == 20 || n == 21) d_mask(4 + n - 20);
                if (n == 31 || n == 32) d_mask(6 + n - 31);
                const int s = n < 11 ? 0 : n < 20 ? 1 : n < 31 ? 2 : 3, n0 = s == 0 ? 2 : s == 1 ? 11 : s == 2 ? 22 : 33;
                if (n >= n0 && n < n0 + 8) split_block(d1[s >> 1], s & 1, n - n0, eb[s], ss);
                if (n == n0 + 8) store_pieces(IMG_D, s >> 1, s & 1, eb[s]);
            };
            auto slot = [&](const int n) {
                if (n == 36) landed();
                if (n < 36) g2_step(n, dA, hB, aW2);
                else if (n < 48) f1_mfma(n - 36);
                else g2_step(n - 12, dA, hB, aW2);
                d_work(n);
                ahead_work(n, false);
            };
            X3S_REP10(slot, 0) X3S_REP10(slot, 10) X3S_REP10(slot, 20) X3S_REP10(slot, 30) X3S_REP10(slot, 40) X3S_REP10(slot, 50)
        }
        have_prev = true;
    }
    if (have_prev) {   // G1 of the last tile
        G1Ops g1o;
#pragma unroll
        for (int q = 0; q < 12; ++q) g1_gather_pair(g1o, q, h_base0, h_base1);
#pragma unroll
        for (int k = 0; k < 36; ++k) g1_step(k, g1o, xbn, true);
        // (dW1 / db1 may be copied right behind this block, where the two paths around it meet: the last MFMAs' wait states)
        asm volatile("s_nop 7" : "+a"(aW1[0]), "+a"(aW1[1]), "+a"(aW1[2]), "+a"(aW1[3]), "+v"(aB1[0]), "+v"(aB1[1]), "+v"(aB1[2]), "+v"(aB1[3]));
    }
    }   // (gw < n_tiles)

    // ---- the lane partials -> sums over the 32 sample lanes of each half, through the wave's (now free) images
    __syncthreads();
    float rb2[2], rw3[2], rw4[2];   // lane (l31 = unit within the 32-unit tile t... ) see below
    {
        float* const scr = reinterpret_cast<float*>(&sm.img[wave][0][0]);   // [96][64]
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                scr[(0 * 32 + 16 * t + r) * 64 + lane] = pb2[t][r];
                scr[(1 * 32 + 16 * t + r) * 64 + lane] = pw3[t][r];
                scr[(2 * 32 + 16 * t + r) * 64 + lane] = pw4[t][r];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // lane (u = l31, half q = lhi) sums unit 32 t + u of tile t = q ... : unit n = 32 t + row, row = (r & 3) + 8 (r >> 2) + 4 hi  <->  (t, r, hi)
        // this lane takes unit n = 32 lhi + l31 of each of the three vectors: t = lhi, row = l31: hi = (row >> 2) & 1, r = (row & 3) + 4 (row >> 3)
        const int row = l31, hi = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3), t = lhi;
        float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const float* src = scr + (v * 32 + 16 * t + r) * 64 + 32 * hi;
#pragma unroll
            for (int m = 0; m < 32; m += 4) {
                const v4f q = *reinterpret_cast<const v4f*>(src + m);
                s[v] += (q.x + q.y) + (q.z + q.w);
            }
        }
        rb2[0] = s[0]; rw3[0] = s[1]; rw4[0] = s[2];
        rb2[1] = rw3[1] = rw4[1] = 0.f;
    }
    __syncthreads();

    // ---- workgroup reduction of the 4 waves' partial gradients in LDS, then one coalesced row of `partial`
    constexpr int RP = (P + 3 + 3) & ~3;
    float s3 = adb3, s4 = adb4, sA = ACTOR ? st0 : st1, sB = st2, sC = st3;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s3 += __shfl_xor(s3, o, 64); s4 += __shfl_xor(s4, o, 64);
        sA += __shfl_xor(sA, o, 64); sB += __shfl_xor(sB, o, 64); sC += __shfl_xor(sC, o, 64);
    }
    constexpr int kStatCols = (kNavppoVarTu && ACTOR) ? 4 : 3;   // (RP has room for the actor's fourth column, not for the critic's)
    static_assert(P + kStatCols <= RP, "the statistics fit the row");
    float sV = stv;
    if constexpr (kStatCols == 4) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sV += __shfl_xor(sV, o, 64);
    }
    float* const red0 = reinterpret_cast<float*>(&sm.img[0][0][0]);
    float* const rowp = red0 + wave * RP;
    {
        auto put = [&](int idx, float v) { rowp[idx] = v; };
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int t1 = 0; t1 < 2; ++t1)
#pragma unroll
                for (int r = 0; r < 16; ++r) put(OFF_W2 + (32 * t2 + c_row(r, lane)) * H + 32 * t1 + l31, aW2[t2][t1][r]);
        // unit 32 lhi + l31 of b2 / w3 / w4
        put(OFF_B2 + 32 * lhi + l31, rb2[0]);
        put(OFF_W3 + 32 * lhi + l31, rw3[0]);
        if (ACTOR) put(OFF_W4 + 32 * lhi + l31, rw4[0]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int r = 0; r < 4; ++r) put(OFF_W1 + (16 * u + 4 * kk + r) * 16 + l15, aW1[u][r]);
            if (l15 == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) put(OFF_B1 + 16 * u + 4 * kk + r, aB1[u][r]);
            }
        }
        if (lane == 0) {
            put(OFF_B3, s3);
            if (ACTOR) put(OFF_B4, s4);
            put(P + 0, sA);
            put(P + 1, sB);
            put(P + 2, sC);
            if constexpr (kStatCols == 4) put(P + 3, sV);
        }
    }
    __syncthreads();
    float* out = partial + (size_t)block * P;
    const float* red = red0;
    for (int k = tid; k < P; k += NT) out[k] = (red[k] + red[RP + k]) + (red[2 * RP + k] + red[3 * RP + k]);
    if (tid < kStatCols) stats_partial[block * 4 + tid] = (red[P + tid] + red[RP + P + tid]) + (red[2 * RP + P + tid] + red[3 * RP + P + tid]);
}

}  // namespace x3s

// X3S_PAIR: the block-index bit that joins two workgroups into a pair (0: no pairing, every workgroup walks its own tiles for both
// nets, actor then critic -- the A/B partner, tools/build_mlp64_variant.py).  Both nets read the same pre-split tiles; unpaired, a
// workgroup comes back to a tile a whole pass later, when the caches have long dropped it.  Paired, workgroup b runs the actor over
// the tiles of block b while b ^ X3S_PAIR runs the critic over the same tiles, then the two swap: the second reader of a tile follows
// the first by microseconds.  Workgroups are dealt round-robin over the 8 XCDs, so b and b ^ 8 share an L2 (a speed matter only: nothing
// is handed from one workgroup to the other).  WHICH workgroup computes a partial row does not change it -- every (wave, net) sums the
// same tiles in the same order into the same row -- so the results are bit for bit those of the unpaired launch.
#ifndef X3S_PAIR
#define X3S_PAIR 8
#endif
static_assert(X3S_PAIR >= 0 && (X3S_PAIR & (X3S_PAIR - 1)) == 0, "X3S_PAIR is 0 or one bit of the block index");

// both nets of one epoch in one launch (net_mask as mlp64_pass_both_x3), 16-column rows
__global__ __launch_bounds__(64 * x3s::SW) void NAVPPO_KL_KERNEL(mlp64_pass_both_x3s)(const float* __restrict__ params, const unsigned char* __restrict__ prep,
                                                                    const float* __restrict__ act, const float* __restrict__ logp_old,
                                                                    const float* __restrict__ rtg, const float* __restrict__ adv,
                                                                    long long M, float var, float clip, float inv_n, int net_mask,
                                                                    float* __restrict__ partial_a, float* __restrict__ stats_partial_a,
                                                                    float* __restrict__ partial_c, float* __restrict__ stats_partial_c NAVPPO_KL_PARAM) {
    __shared__ __attribute__((aligned(128))) x3s::SmemS sm;
    NAVPPO_KL_GATE();
    NAVPPO_VAR_READ(var);
#if X3S_PAIR
    // paired: both nets and whole pair groups only (single-net launches, small and odd grids keep the order below on their own block).
    // The critic's pass is always the partner's block: a workgroup with the pair bit clear runs actor(b), critic(b ^ X3S_PAIR), one with
    // it set runs critic(b ^ X3S_PAIR), actor(b) -- every row of either net is written once, by one workgroup.  One loop of two phases,
    // not unrolled: each body has ONE call site, so the listing holds each tile loop once (tests/test_isa_schedule_cpu.py).
    const int b = blockIdx.x;
    const bool paired = net_mask == 3 && gridDim.x % (2 * X3S_PAIR) == 0;
    const bool critic_first = paired && (b & X3S_PAIR);
#pragma nounroll
    for (int phase = 0; phase < 2; ++phase) {
        int blk = b;
        asm volatile("" : "+s"(blk));
        if (__builtin_expect((phase == 0) != critic_first, 1)) {
            if (net_mask & 1) x3s::pass_body<true>(sm, params, prep, act, logp_old, rtg, adv, M, var, clip, inv_n, partial_a, stats_partial_a, blk);
        } else {
            if (net_mask & 2)
                x3s::pass_body<false>(sm, params + Layout<16>::P_ACTOR, prep, act, logp_old, rtg, adv, M, var, clip, inv_n, partial_c, stats_partial_c,
                                      paired ? blk ^ X3S_PAIR : blk);
        }
        if (phase == 0 && net_mask == 3) __syncthreads();   // the first body's last LDS reads, the second's weight pieces
    }
#else
    if (net_mask & 1) x3s::pass_body<true>(sm, params, prep, act, logp_old, rtg, adv, M, var, clip, inv_n, partial_a, stats_partial_a, blockIdx.x);
    if (net_mask == 3) __syncthreads();
    if (net_mask & 2)
        x3s::pass_body<false>(sm, params + Layout<16>::P_ACTOR, prep, act, logp_old, rtg, adv, M, var, clip, inv_n, partial_c, stats_partial_c, blockIdx.x);
#endif
}
