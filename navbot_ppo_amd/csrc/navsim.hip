// navsim.hip -- gfx950 (MI355X / CDNA4) kernels + the C ABI of include/navsim.h.
//
// What runs here replaces, for N envs at once, the reference's
//   Env.step / Env.reset            project_ppo/src/environment_new.py:272-382
//   Env.getOdometry/getState/setReward               ... :138-270
//   the Gazebo diff-drive + ray sensor they wait on   turtlebot3_fake.cpp:110-180 (motion model),
//                                                     turtlebot3_burger.gazebo.xacro:104-127 (LiDAR)
//   PPO.compute_rtgs                project_ppo/src/ppo.py:643-671
//
// Arithmetic contract (DESIGN.md "numerics"): pose, goal geometry, angles, reward in float64
// (the reference's rounding rules -- round-half-even yaw, 1- and 2-decimal Python round() --
// cannot be met in float32); ray/segment tests in float32 with explicit fmaf and one
// correctly-rounded division per hit; min over hits is exact, so the result does not depend
// on how segments are split over lanes.  Compiled with -ffp-contract=off: every fused
// multiply-add is written out.
//
// Kernel layout: one workgroup = 4 waves = EPB (16) consecutive envs.
//   phase 1  wave 0, lane = env : integrate pose (f64), sensor origin + B beam directions -> LDS
//   phase 2  all 4 waves        : nearest hit per (env, beam)
//              shared map  : segments staged in LDS tiles, lane = ray (env, beam); every lane of a wave
//                            reads the same segment at the same time: LDS broadcast, no conflicts
//              per-env map : wave w takes envs 4w..4w+3; lane = segment (16 B/lane coalesced
//                            HBM loads, each segment read exactly once), B running minima per lane,
//                            wavefront min-reduce per beam
//   phase 3  wave 0, lane = env : getState / obs / reward / flags / timeout / auto-reset, state write-back
//   phase 4  all 4 waves        : the block's 64 x (B+6) observation tile leaves LDS as one contiguous,
//                                 fully coalesced store
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "navsim.h"
#include "mlp64_policy.h"
#include "resmlp_policy.h"

namespace {

constexpr double kWheelRadius = 0.033;  // turtlebot3_fake.h:39
constexpr double kWheelSep = 0.160;     // turtlebot3_fake.cpp:44
constexpr double kLidarX = -0.032;      // turtlebot3_burger.urdf.xacro:137
constexpr double kAngleMin = -1.5707975, kAngleMax = 1.5707975;  // gazebo.xacro:113-114
constexpr float kRangeMin = 0.12f, kRangeMax = 3.5f;             // gazebo.xacro:118-119
constexpr int kSubsteps = 6;     // 30 Hz drive updates per 5 Hz scan (gazebo.xacro:62,107)
constexpr int kMaxRects = 16;
constexpr int kMaxGoalTries = 64;

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(NAVSIM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

struct Rects {
    double r[2][kMaxRects][4];  // [which][k][xmin,xmax,ymin,ymax]
    int n[2];
};

struct Params {
    // The first 128 bytes hold what the first memory requests of a step launch need (the pose waves' state loads, the ray waves'
    // first segment tiles): they arrive with the first round of scalar kernarg loads.  In declaration order the compiler reached
    // the state pointers in its fourth dependent round, ~1 us into the launch.
    int N, S, per_env;        // per_env: bit 0 = one map per env, bits 1 / 2 = stream it with non-temporal loads (navsim_set_map)
    int seg_pack_log2;        // cast: log2(lanes per env in one 64-lane pass) = 6, or log2(pow2ceil(S)) when S <= 32
    const float4* seg;        // [S] or [N][S]
    double *th, *x, *y, *gx, *gy, *past_dist, *ep_ret, *ep_path;
    float2* past_action;
    int32_t* ep_step;         // low 30 bits: steps taken in the episode; kRecValid: the records below are current
    uint32_t* rng_ctr;
    const double* beam_cs;    // [2][B]: cos(phi_b), sin(phi_b)
    int B, respawn;
    // ---- 128 bytes
    int max_ep_steps, auto_reset, obs_f16, below_min_mode;
    float sigma;  // LiDAR range noise (0 = off)
    uint32_t key0, key1;
    uint64_t env_id_base;
    double thr, spawn_x, spawn_y, spawn_yaw, goal_lo, goal_hi, diag;
    // next-episode records, written by the step kernel when an env's goal stream has moved, read otherwise:
    double* rec_g;            // [2][3][N] goal x, y and start-to-goal distance
    float4* rec_tail;         // [2][N] the reset observation's (dist/diag, yaw/360, rel_theta/360, diff/180)
    uint2* rec_ck;            // [2][N] (draw counter after the reset, start-pose index)
    double* rsp_g;            // [2][N] the arrival re-spawn goal (respawn_on_arrive)
    uint32_t* rsp_ctr;        // [N] draw counter after the re-spawn draw
    const float4* tile_box;   // shared maps of 65..4096 segments (kept in Morton order by navsim_set_map): per 64-segment tile
                              // the bounding box (xmin, ymin, xmax, ymax) of its segments; else null
    const float* spawn_scan;  // [K][B] or [N][K][B] nearest hits (+inf = none) at the K start poses (K = 1: the cfg spawn pose)
    const float* spawn_obs;   // same shape: the noise-free lidar entries of the reset observation (sanitised scan / 3.5)
    const double* starts;     // [K][3] start poses (x, y, yaw)
    const double* starts_sc;  // [K] the integer-degree yaw of Env.getOdometry at each start pose, evaluated on the device
    const double* goals;      // [G][2] goal points; G == 0: uniform goal box + rejection rectangles
    int K, G;
    double min_dist, max_dist;
    const Rects* rects;
    // ---- moving obstacles (navsim_set_movers), appended: nothing above moves.  Read by the MOV instantiations, the reset /
    // ray-cast kernels and (spawn_per_env) the MOV spec lanes only.
    const float4* mov_tape;      // [mov_P][mov_M] segments, borrowed; null = no movers
    const int32_t* mov_phase0;   // [N] per-env phase offset in [0, mov_P), the handle's copy; null = all zero
    int mov_P, mov_M;
    int mov_pack_log2;           // mover pass: log2(lanes per env) = log2(pow2ceil(mov_M)), as seg_pack_log2 for the static map
    int spawn_per_env;           // spawn_scan / spawn_obs are [N][K][B]: per_env != 0, or movers with a per-env phase offset / tape
    // ---- a bank of tapes (navsim_set_mover_bank), appended.  mov_tape is then [K][Pmax][mov_M] and mov_P = period[0].
    const uint2* mov_bp;         // [N] (base row = tape_id * Pmax, period of the env's tape), the handle's; null = (0, mov_P) for all
    const int32_t* mov_tid;      // [N] tape id per env (the goal rectangles' index), the handle's; null = all zero
    const double* mov_rects;     // [K][mov_n_rects][4] per-tape goal rejection rectangles (a NaN row is absent), the handle's; null = none
    int mov_n_rects;
    // ---- sector LiDAR (navsim_set_scan_pool), in what was the struct's tail padding.  Read by the pooled twins (navsim_pool.hip) only:
    // they cast B * pool rays and min-pool `pool` consecutive ones into each of the B scan columns; beam_cs is then [2][B * pool] and
    // the rows of spawn_scan / spawn_obs hold B * pool entries.  1 = off.
    int pool;
};
static_assert(offsetof(Params, max_ep_steps) == 128, "the hot head of Params");

// The tape row env i casts: `k` = steps taken in the episode (a step's scan: k = the counter before the step, + 1; a reset
// observation and navsim_raycast before the first step: k = 0), `bp` = (base row, period) of the env's tape.
// k < 2^30 + 1, phase0 < period <= 65536, base < 2^24: no overflow.
__device__ __forceinline__ uint32_t mover_row(const uint2 bp, const uint32_t k, const uint32_t phase0) {
    return bp.x + (k + phase0) % bp.y;
}
// (base row, period) of env i's tape from global memory (the single-step kernels, reset scans, navsim_raycast)
template <class PRef>
__device__ __forceinline__ uint2 mover_bp(PRef P, const int i) {
    const uint2* const bp = P.mov_bp;
    return bp ? bp[i] : make_uint2(0u, (uint32_t)P.mov_P);
}

// ---------------------------------------------------------------- device helpers

// q / s for an integer-valued q with |q| < 2^26 and s in {10, 100} (also k/100 values over 180 or 360): one multiply by
// the rounded reciprocal plus one fma correction gives the correctly rounded quotient -- verified exhaustively over those
// domains by tools/verify/div_by_const_exact.c -- instead of the ~30-instruction IEEE float64 division sequence.
__device__ __forceinline__ double div_const(double q, double s, double inv_s) {
    const double r0 = q * inv_s;
    return fma(fma(-s, r0, q), inv_s, r0);
}

// Python round(x, nd), s = 10^nd: decimal rounding, ties-to-even on the exact binary value
// (environment_new.py:149-150,169-176).  x*s is held exactly as p + err.  Branch-free except for the out-of-domain
// quotient (|x s| >= 2^26: never with map coordinates in metres and angles in degrees).
__device__ __forceinline__ double py_round(double x, double s, double inv_s) {
    const double p = x * s;
    const double err = fma(x, s, -p);
    const double fl = floor(p);
    const double frac = p - fl;
    const double h = fl * 0.5;
    const bool odd = h != floor(h);                     // fl odd -> the even neighbour is fl + 1
    const bool up = (frac > 0.5) || ((frac == 0.5) && ((err > 0.0) || ((err == 0.0) && odd)));
    const double q = up ? fl + 1.0 : fl;
    double r = div_const(q, s, inv_s);
    if (__builtin_expect(!(fabs(q) < 0x1p26), 0)) r = q / s;   // also NaN / inf
    if (r == 0.0) r = copysign(0.0, x);
    return isfinite(x) ? r : x;
}

// yaw of Env.getOdometry, environment_new.py:142-147, for the yaw-only quaternion (qz, qw) = (sin, cos)(theta / 2)
__device__ __forceinline__ double yaw_from_quat4(double qx, double qy, double qz, double qw) {
    const double rad2deg = 180.0 / 3.14159265358979323846;
    double yaw = rint(atan2(2 * (qx * qy + qw * qz), 1 - 2 * (qy * qy + qz * qz)) * rad2deg);  // :142
    if (!(yaw >= 0)) yaw = yaw + 360;                                                            // :144-147
    return yaw + 0.0;   // Python's round() returns the int 0 for -0.4: no negative zero
}
__device__ __forceinline__ double yaw_from_quat(double qz, double qw) { return yaw_from_quat4(0.0, 0.0, qz, qw); }

// The same integer without the quaternion round trip: atan2(sin th, cos th) is th wrapped to (-pi, pi], so the yaw is
// rint(th in degrees, wrapped to [-180, 180]).  The two routes differ by < 1e-9 degree for |th| < 1e7 rad, so they round
// to the same integer unless the angle sits within 1e-6 of a half degree: then (*exact = false) the caller takes the
// quaternion route.
__device__ __forceinline__ double yaw_fast(double th, bool* exact) {
    const double rad2deg = 180.0 / 3.14159265358979323846;
    const double d = th * rad2deg;
    const double m = d - 360.0 * rint(d * (1.0 / 360.0));
    double yaw = rint(m);
    *exact = (fabs(d) < 5e8) && (fabs(fabs(m - yaw) - 0.5) > 1e-6);
    if (!(yaw >= 0)) yaw = yaw + 360;
    return yaw + 0.0;
}

// rel_theta and diff_angle of Env.getOdometry, environment_new.py:149-176; branch-free
__device__ __forceinline__ void goal_rel(double x, double y, double gx, double gy, double yaw, double& rel_theta, double& diff) {
    const double kPi = 3.14159265358979323846;
    const double rad2deg = 180.0 / kPi;
    const double dx = py_round(gx - x, 10.0, 0.1);                                       // :149
    const double dy = py_round(gy - y, 10.0, 0.1);                                       // :150
    const double at = atan(dy / dx);                                                     // :153-168
    double theta = kPi;
    theta = (dy == 0 && dx > 0) ? 0.0 : theta;
    theta = (dx == 0 && dy < 0) ? 1.5 * kPi : theta;
    theta = (dx == 0 && dy > 0) ? 0.5 * kPi : theta;
    theta = (dx < 0 && (dy < 0 || dy > 0)) ? kPi + at : theta;
    theta = (dx > 0 && dy < 0) ? 2 * kPi + at : theta;
    theta = (dx > 0 && dy > 0) ? at : theta;
    rel_theta = py_round(theta * rad2deg, 100.0, 0.01);                                  // :169
    const double d = yaw - rel_theta;                                                    // :170
    const double w = (d >= -180 && d <= 180) ? d : ((d < -180) ? 360 + d : -360 + d);    // :171-176
    diff = py_round(w, 100.0, 0.01);
}

// Env.getOdometry, environment_new.py:138-181, for the yaw-only quaternion Gazebo publishes.
__device__ __forceinline__ void goal_angles_q(double x, double y, double qz, double qw, double gx, double gy,
                                              double& yaw, double& rel_theta, double& diff) {
    yaw = yaw_from_quat(qz, qw);
    goal_rel(x, y, gx, gy, yaw, rel_theta, diff);
}

__device__ __forceinline__ void goal_angles(double x, double y, double th, double gx, double gy,
                                            double& yaw, double& rel_theta, double& diff) {
    goal_angles_q(x, y, sin(th / 2), cos(th / 2), gx, gy, yaw, rel_theta, diff);
}

// Parametric ray / segment test.  o + t d = a + u e  =>  t = cross(a-o, e) / cross(d, e),
// u = cross(a-o, d) / cross(d, e); hit iff t >= 0 and 0 <= u <= 1, decided on the signs of the
// numerators so the only division is the (correctly rounded) t of an actual hit.
__device__ __forceinline__ float ray_seg(float rx, float ry, float ex, float ey, float k, float c, float s) {
    const float den = fmaf(c, ey, -(s * ex));
    const float un = fmaf(rx, s, -(ry * c));
    const bool pos = (den > 0.0f) && (k >= 0.0f) && (un >= 0.0f) && (un <= den);
    const bool neg = (den < 0.0f) && (k <= 0.0f) && (un <= 0.0f) && (un >= den);
    return (pos || neg) ? (k / den) : INFINITY;
}

// LaserScan value from the nearest hit `best` (+inf if none), gazebo.xacro:117-126:
//   >= range_max -> +inf ; < range_min -> range_min (mode 0) or -inf (mode 1, Gazebo's ray sensor) ;
//   otherwise best + sigma * n clamped to [range_min, range_max]  (n = 0 when the noise is off)
__device__ __forceinline__ float sensor_value(float best, float sigma, float n, int below_min_mode) {
    if (!(best < kRangeMax)) return INFINITY;
    if (best < kRangeMin) return below_min_mode ? -INFINITY : kRangeMin;
    const float r = fmaf(sigma, n, best);
    return fminf(fmaxf(r, kRangeMin), kRangeMax);
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Standard-normal draw for LiDAR beam b of env `gid` at (goal draws so far, episode step): Philox4x32-10, one call per
// four beams, Box-Muller in float32.
__device__ __forceinline__ float lidar_noise(uint32_t k0, uint32_t k1, uint64_t gid, uint32_t ctr, uint32_t ep_step, int b) {
    uint32_t r[4];
    philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), ctr, 0x4C000000u | ((ep_step & 0xFFFFu) << 8) | (uint32_t)(b >> 2),
                  k0, k1, r);
    const int pr = (b >> 1) & 1;
    const float u1 = ((float)(r[2 * pr] >> 8) + 1.0f) * 0x1.0p-24f;  // (0, 1]
    const float u2 = (float)(r[2 * pr + 1] >> 8) * 0x1.0p-24f;       // [0, 1)
    const float rad = sqrtf(-2.0f * logf(u1));
    const float ang = 6.283185307179586f * u2;
    return (b & 1) ? rad * sinf(ang) : rad * cosf(ang);
}

// No early exit: the loop bounds and addresses are then wave-uniform (scalar loads from the constant cache, all
// rectangles in flight at once) instead of one dependent L2 round trip per rectangle per lane.
// (`R` is the workgroup's LDS copy in the step kernel -- from global memory every rectangle of every attempt was a
// dependent scalar-load round trip on the one wave the whole workgroup ends up waiting for, 0.8 us per attempt with the
// eight rectangles of stage_2 -- and the table in global memory in the reset kernel.)
__device__ __forceinline__ bool goal_rejected(const Rects& R, int which, double gx, double gy) {
    const int n = R.n[which];
    bool rej = false;
    for (int k = 0; k < n; ++k) {
        const double* q = R.r[which][k];
        rej |= (q[0] <= gx) & (gx <= q[1]) & (q[2] <= gy) & (gy <= q[3]);
    }
    return rej;
}

// goal ~ U(lo,hi)^2 with rejection (environment_new.py:337-345 reset, :245-253 respawn);
// one Philox call per attempt, counter = (env id, draws so far).
// MOV (the mover kernels, the reset kernel): the rectangles of env i's tape (Params::mov_rects, navsim_set_mover_bank) reject as
// the handle's do, for both `which`.  They are read from global memory: a goal is drawn at episode ends only.
template <class PRef, bool MOV = false>
__device__ __forceinline__ void sample_goal(PRef P, const Rects& R, int i, int which, uint32_t& ctr, double& gx, double& gy) {
    const uint64_t gid = P.env_id_base + (uint64_t)i;
    gx = 0;
    gy = 0;
    [[maybe_unused]] const double* tr = nullptr;
    [[maybe_unused]] int tn = 0;
    if constexpr (MOV) {
        if (P.mov_rects) {
            tn = P.mov_n_rects;
            tr = P.mov_rects + (size_t)(P.mov_tid ? P.mov_tid[i] : 0) * (size_t)tn * 4;
        }
    }
    for (int tries = 0; tries < kMaxGoalTries; ++tries) {
        uint32_t r[4];
        philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), ctr, 0x6e617673u, P.key0, P.key1, r);
        ctr += 1;
        const double ux = (double)((((uint64_t)r[0] << 32) | r[1]) >> 11) * 0x1.0p-53;
        const double uy = (double)((((uint64_t)r[2] << 32) | r[3]) >> 11) * 0x1.0p-53;
        gx = P.goal_lo + (P.goal_hi - P.goal_lo) * ux;
        gy = P.goal_lo + (P.goal_hi - P.goal_lo) * uy;
        bool rej = goal_rejected(R, which, gx, gy);
        if constexpr (MOV) {
            for (int k = 0; k < tn; ++k) {   // (a NaN entry compares false: the row is absent)
                const double* q = tr + 4 * k;
                rej |= (q[0] <= gx) & (gx <= q[1]) & (q[2] <= gy) & (gy <= q[3]);
            }
        }
        if (!rej) break;
    }
}

// Episode start: which start pose k (index into P.starts) and which goal.
//   G == 0  the reference Env.reset: the single spawn pose and a uniform goal with rectangle rejection.
//   G  > 0  GoalSpawnSampler.sample_start_and_goal (project_ppo/src/spawn_goal_sampler.py:52-62): uniform picks from the
//           start-pose and goal tables until min_dist <= |start - goal| <= max_dist, at most 100 attempts, then one
//           unconditional pick.  One Philox call per attempt.
template <class PRef, bool MOV = false>
__device__ __forceinline__ void sample_episode(PRef P, const Rects& R, int i, uint32_t& ctr, int& k, double& gx, double& gy) {
    if (P.G == 0) {
        k = 0;
        sample_goal<PRef, MOV>(P, R, i, 0, ctr, gx, gy);
        return;
    }
    const uint64_t gid = P.env_id_base + (uint64_t)i;
    for (int tries = 0; tries <= 100; ++tries) {
        uint32_t r[4];
        philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), ctr, 0x6e617673u, P.key0, P.key1, r);
        ctr += 1;
        k = (int)(((uint64_t)r[0] * (uint64_t)P.K) >> 32);
        const int g = (int)(((uint64_t)r[1] * (uint64_t)P.G) >> 32);
        gx = P.goals[2 * g];
        gy = P.goals[2 * g + 1];
        const double dx = P.starts[3 * k] - gx, dy = P.starts[3 * k + 1] - gy;
        const double dist = sqrt(dx * dx + dy * dy);  // np.linalg.norm, spawn_goal_sampler.py:57
        if (tries == 100 || (P.min_dist <= dist && dist <= P.max_dist)) break;
    }
}

constexpr uint32_t kRecValid = 0x40000000u;   // bit of the ep_step word: the cached next-episode records of this env are current
constexpr uint32_t kStepMask = 0x3FFFFFFFu;

// POOL (the sector-LiDAR twins, navsim_pool.hip): the block casts NB * Params::pool rays (pool <= kMaxPool) and writes NB scan
// columns, so everything indexed by ray -- dir, rng, noise, sp_scan, pe, beam -- is sized for NR = kMaxPool * NB rays and everything
// indexed by column keeps NB.  Off, NR == NB: the block is what it was.
constexpr int kMaxPool = 4;
template <int NB, int EPB, int NW = 4, bool POOL = false>
struct StepSmem {
    static constexpr int NR = POOL ? kMaxPool * NB : NB;   // rays the arrays hold
    float2 org[EPB];             // sensor origin per env
    float2 hd[EPB];              // heading (cos, sin) as float32: the cull only (never the ranges)
    float2 dir[NR * EPB];        // [beam][env] unit direction
    unsigned rng[NR * EPB];      // [beam][env] nearest hit as float bits (non-negative floats order like uints)
    float obs[EPB * (NB + 7)];   // [env][B+6 (+1 pad: odd row stride, conflict-free)] the block's output tile
    float noise[NR * EPB];       // [beam][env] standard-normal draws for the range noise (only written when sigma > 0)
    // env state parked by the part-1 lanes for the part-2/3 lanes
    double sv_d[13][EPB];        // x, y, th, gx, gy, past_dist, dist, (7-9 unused), ep_ret, step displacement, ep_path
    float2 sv_act[EPB], sv_pact[EPB];
    uint32_t sv_ctr[EPB];
    uint32_t sv_step[EPB];       // raw ep_step word (kRecValid | step)
    // next-episode records (cached in HBM, see Params::rec_*): [0] the reset that follows a collision / timeout,
    // [1] the reset that follows an arrival when the arrival re-spawn draw comes first (respawn_on_arrive)
    double sp_d[2][6][EPB];      // start x, y, yaw, goal x, y, distance
    float4 sp_tail[2][EPB];      // the four goal entries of the reset observation
    uint32_t sp_ctr[2][EPB];
    int sp_k[2][EPB];
    double sp_rg[2][EPB];        // the arrival re-spawn goal (environment_new.py:245-253) and the draw counter after it
    uint32_t sp_rctr[EPB];
    float sp_scan[2][EPB][NR];   // lidar entries of the reset observation (SENS: the raw nearest hits at the start pose)
    unsigned mn_bits[EPB];       // min over the sanitised scan as float bits, and whether a reading is negative (-inf, SENS)
    unsigned neg[EPB];
    // cast: per-wave queue of the segments that survive the cull (ring of 128)
    float4 q4[NW][128];
    unsigned qe[NW][128];
    float4 r4[NW][128];          // ... and of those whose angular extent holds at least one beam
    unsigned re[NW][128];        //     env | first beam of that extent << 8 | number of beams << 16
    unsigned pe[NW][(POOL || NB > 16) ? 128 : 1];   // 36 beams: stage-B work entries: r4 slot | first beam << 8 | beams to test << 16
    float4 tbox[64];             // Params::tile_box, staged once per launch (BOXES)
    Rects rects;                 // Params::rects, staged by the ray waves before barrier A (the spec lanes' goal rejection test)
    float2 act_l[EPB];           // persistent rollout: the action the policy phase chose for this step
    double beam[2 * NR];         // Params::beam_cs, staged by the pose waves (persistent rollout: once)
    // persistent rollout: the envs' state lives here between the steps (HBM sees it before the first and after the last)
    double st_d[8][EPB];         // x, y, th, gx, gy, past_dist, ep_ret, ep_path
    float2 st_pact[EPB];
    uint32_t st_step[EPB], st_ctr[EPB];
};
// What the MOV instantiations (moving obstacles, Params::mov_tape) keep in LDS on top of it: a kernel with movers declares this
// one, step_body takes the base and reaches the rest through a cast that only its MOV branches contain.
template <int NB, int EPB, int NW = 4, bool POOL = false>
struct StepSmemMov : StepSmem<NB, EPB, NW, POOL> {
    uint32_t mv_phase[EPB];      // the tape row each env's scan sees this step, published by the pose lanes before barrier A
    uint32_t mv_phase0[EPB];     // persistent kernels: Params::mov_phase0 of the workgroup's envs, staged once per launch
    uint2 mv_bp[EPB];            // ... and their tapes' (base row, period) (Params::mov_bp)
};

// Correctly rounded K / Dn for positive, normal-range operands (Dn in [2^-60, 2^20], K in {0} U [2^-60, 2^20]):
// the reciprocal-refinement sequence the compiler emits for an IEEE float32 divide (v_rcp, 2 fma to refine,
// quotient, two fma residual corrections), minus its exponent pre-scaling (v_div_scale x2) and special-case
// fix-up (v_div_fixup, v_div_fmas), which are no-ops in this range: 22 instead of 36 pipe cycles on gfx950
// (measured: v_fma/v_mul full rate, v_div_* half rate, v_rcp quarter rate).  Dn == 0 gives NaN.
__device__ __forceinline__ float div_pos(float K, float Dn) {
    float r = __builtin_amdgcn_rcpf(Dn);
    const float f0 = fmaf(-Dn, r, 1.0f);
    r = fmaf(f0, r, r);
    float q = K * r;
    float e = fmaf(-Dn, q, K);
    q = fmaf(e, r, q);
    e = fmaf(-Dn, q, K);
    return fmaf(e, r, q);
}

// One ray/segment test, same decisions and the same range bits as ray_seg(), built from full-rate VALU ops
// only (v_cmp / v_cndmask / v_min_f32 are half rate on gfx950):
//   p1 = k*den + 0 >= 0  <=>  k and den agree in sign or k == 0   (no underflow: |k|,|den| are 0 or >= 2^-56;
//   p2 = un*den + 0 >= 0,  w = |den| - |un| >= 0  <=>  0 <= u <= 1  the "+ 0" turns a -0 product into +0)
//   t  = |k| / |den|  ==  k / den  when the signs agree; >= +0, +inf or NaN, so its bit pattern orders like a uint.
// miss <=> sign bit of (p1 | p2 | w); an arithmetic shift makes that an all-ones mask OR-ed into t's bits, and the
// running nearest hit is an unsigned min over bit patterns (inf = 0x7f800000 is the identity, NaN never wins).
__device__ __forceinline__ unsigned ray_seg_bits(float rx, float ry, float ex, float ey, float k, float c, float s) {
    const float den = fmaf(c, ey, -(s * ex));
    const float un = fmaf(rx, s, -(ry * c));
    const float p1 = fmaf(k, den, 0.0f);
    const float p2 = fmaf(un, den, 0.0f);
    const float w = fabsf(den) - fabsf(un);
    const unsigned miss = (unsigned)((int)(__float_as_uint(p1) | __float_as_uint(p2) | __float_as_uint(w)) >> 31);
    return __float_as_uint(div_pos(fabsf(k), fabsf(den))) | miss;
}

// Beam coordinate of a point (x ahead, y left) in the robot frame: f = (theta + A) / delta, beam b sits at f = b.
// theta = 2 atan(u) with the half-angle tangent u = y / (r + x), monotone over (-pi, pi) and clamped to |u| <= 1.1 (just
// past the +-90 degree fan edge, where only the side matters); atan by a degree-9 odd polynomial, |error| < 2.4e-5 rad.
// Used ONLY to decide which segments are tested exactly, with a margin 40x above its error.  *bad: the point is within
// 3 cm of the sensor or within 4.5e-3 rad of straight behind it, where u is ill-conditioned -- the caller keeps the segment.
__device__ __forceinline__ float beam_coord(float x, float y, float two_inv_delta, float a_inv_delta, bool* bad) {
    const float r = __builtin_amdgcn_sqrtf(fmaf(x, x, y * y));
    const float d = r + x;
    *bad = !(d > 1e-5f * r) || (r < 0.03f);
    float u = y * __builtin_amdgcn_rcpf(d);
    u = __builtin_amdgcn_fmed3f(u, -1.1f, 1.1f);
    const float z = u * u;
    float p = fmaf(0.01608042f, z, -0.07488631f);
    p = fmaf(p, z, 0.1729194f);
    p = fmaf(p, z, -0.32846571f);
    p = fmaf(p, z, 0.99974538f);
    return fmaf(u * p, two_inv_delta, a_inv_delta);
}

// (A workgroup reserves ceil(waves / 4) slots on EVERY SIMD of its CU, so a 5-wave block costs as much residency as an 8-wave
// one: measured 1 block/CU.)

// lidar part of an observation row (environment_new.py:289-294) from nearest hits `best` (stride `bstride`);
// returns min(sanitised scan) for the collision rule (:200)
__device__ __forceinline__ float write_lidar(float* row, const float* best, int bstride, const float* noise, int nstride,
                                             float sigma, int below_min_mode, int B) {
    float mn = INFINITY;
    for (int b = 0; b < B; ++b) {
        float r = sensor_value(best[b * bstride], sigma, noise ? noise[b * nstride] : 0.f, below_min_mode);
        if (r == INFINITY) r = 3.5f;  // :193-194 (+inf only: -inf passes through like in the reference; NaN cannot occur)
        mn = r < mn ? r : mn;
        // (float)((double)r / 3.5) == r / 3.5f : double rounding is innocuous for a quotient of
        // two float32 values (53 >= 2*24+2), so the float32 divide gives the reference's bits.
        row[b] = r / 3.5f;            // :289
    }
    return mn;
}

// the same for a sector-LiDAR row: column c is the minimum over the sanitised readings of rays pool c .. pool c + pool - 1 (`best`:
// the raw hits of all B pool rays, stride 1; `noise` per ray)
__device__ __forceinline__ float write_lidar_pool(float* row, const float* best, const float* noise, int nstride, float sigma,
                                                  int below_min_mode, int B, int pool) {
    float mn_all = INFINITY;
    for (int c = 0; c < B; ++c) {
        float mn = INFINITY;
        for (int j = 0; j < pool; ++j) {
            const int k = pool * c + j;
            float r = sensor_value(best[k], sigma, noise ? noise[k * nstride] : 0.f, below_min_mode);
            if (r == INFINITY) r = 3.5f;
            mn = r < mn ? r : mn;
        }
        mn_all = mn < mn_all ? mn : mn_all;
        row[c] = mn / 3.5f;
    }
    return mn_all;
}

// ---------------------------------------------------------------- the step kernel
// One workgroup = 4 waves = EPB consecutive envs (EPB = 16: waves 0-1 are the "pose waves", 2-3 the "ray waves").
//   part 1   pose waves, 8 lanes per env: state loads, float64 motion, the 8 sincos of the step one per lane -> LDS
//            sensor origin + beam directions; the env's state is parked in LDS for its part-2/3 lane.
//            ray waves: the first segment loads of their first work item (nothing there depends on the pose)
//   barrier A
//   part 2   lane-dense (a wave instruction costs the same with 8 or 64 active lanes): wave 0, lane = env: goal geometry
//            of the new pose; last pose wave: the next-episode records of every env -- read back from HBM, or, for an env
//            whose goal stream moved since they were written, recomputed (Philox draw + start-pose geometry) and stored.
//            Meanwhile the cast, one work item = one env (several envs when the map has <= 32 segments), taken from an
//            LDS counter; lane = segment, 16 B/lane coalesced, every segment read from HBM once, two tiles ahead:
//              stage A  cull: a segment that lies wholly behind the +-90 degree beam fan, or farther than the 3.5 m sensor
//                       range, cannot change the scan (ranges >= 3.5 read as "no return", gazebo.xacro:119); the cull
//                       is conservative (margins far above float32 noise) so the result keeps its bits.  Survivors
//                       (about a quarter) are compacted into a per-wave LDS queue.
//              stage B  whenever 64 survivors are queued: the exact ray/segment test of every beam, nearest hit per
//                       (env, beam) by LDS atomic-min over float bit patterns.
//   barrier B
//   part 3   wave 0, lane = env: rules of getState / step / setReward, episode logic, state stores
//   barrier C
//   all:     the EPB x (B+6) observation tile leaves LDS as one contiguous, fully coalesced store.
// SENS = false compiles the sensor-fidelity options (range noise, -inf below range_min) out.
// PERSIST: called once per step by the persistent rollout kernel; the action comes from the policy phase through LDS and
// the env state stays in LDS (sm.st_*) from step to step; `last_step` also writes it back to HBM.
// NW: waves per workgroup (4; the persistent rollout kernel, one workgroup per CU, runs 8 for a shorter cast).
// BOXES: shared map with tile bounding boxes (Params::tile_box): whole 64-segment tiles that lie behind the beam fan or out of
// range are skipped without being loaded (the house map: 32 tiles, ~5 of them near any one pose).
// MOV: moving obstacles (Params::mov_tape, navsim_set_movers): the pose lanes publish each env's tape phase before barrier A and
// the ray waves cast that phase's segments (lane = segment) through the same stage-A queue, behind their static tiles.  `sm` is then
// the base of a StepSmemMov.  Off, nothing of it is compiled: every instantiation without it is what it was.  The 16-env shape holds
// its three mover passes in registers of their own from barrier A on; the 32- / 64-env shapes (six passes, a kernel at its
// 128 registers) feed them through the three request slots of the static tiles instead (kMovRot, in the cast).
// row0: element offset of this step's row in the [T, N] output buffers `io` points at (navsim_step_seq: t N; the pointers are
// then read from the kernarg segment at their use instead of living in SGPRs through the body; 0 elsewhere).
// PRef / IORef: how the parameter block and the I/O pointers are reached.  The persistent rollout passes plain references to its
// own copies.  step_kernel passes references into the kernarg segment (constant address space) behind a compiler barrier: every
// field is then a scalar load AT ITS USE.  As ordinary by-value kernel parameters all ~100 dwords were loaded and spilled to
// VGPR lanes in the entry block (not enough SGPRs), in five dependent rounds, before the first state load could leave: 1.1 us.
struct StepIO {
    const float2* action;
    const float2* past_override;
    void* obs_out;
    float* reward;
    uint8_t *done, *arrive, *ended;
    float* ep_return;
    int32_t* ep_length;
    float* ep_path_out;
};
// EvalIO: what the evaluation kernels (evaluate_kernel, evaluate_resmlp_kernel) pass as `io` instead: no [T, N, .] rows and no
// observation store; the rules lane of an env whose episode ends records it in slot cnt_l[env] of the [quota, N] episode table
// while that count is below the quota.  (The StepIO base is all null: nothing of it is read in the PERSIST form.)
struct EvalIO : StepIO {
    int* cnt_l;          // LDS, [EPB]: episodes recorded per env (absent envs of a tail workgroup: quota)
    int quota;
    uint8_t* rec_flags;   // [quota, N]: 1 success (arrive), 2 collision (done and not arrive), 4 timeout (ended, neither)
    int32_t* rec_length;  // [quota, N]
    float* rec_return;    // [quota, N]
    float* rec_path;      // [quota, N]
};
// Hook: called by EVERY wave right behind barrier B2 (the observation rows are complete but for a reset, which the rules lanes of
// wave 0 work out next): the persistent rollout kernels run the policy of the NEXT step there, on waves that would otherwise
// wait for the rules, reading the rows through next_obs_n below.  NoHook: nothing (step_kernel, steps_kernel).
struct NoHook {
    __device__ __forceinline__ void operator()(int, int) const {}
};
// POOL (sector LiDAR, navsim_set_scan_pool; the twins of navsim_pool.hip): NB stays the number of scan COLUMNS -- the observation
// tile, the policies' rows, the history rows and every output keep their shape -- while the rays the body casts become NC = NB *
// Params::pool, a run-time count (one instantiation serves pool = 2, 3, 4; StepSmem holds kMaxPool * NB rays).  Pose lanes, noise,
// cull, stage A2 and stage B (the entries of the 36-beam path: kPairB) work on the NC rays exactly as an NB = NC instantiation would;
// between barriers B and B2 lane (column, env) takes the minimum of its `pool` consecutive sanitised readings.  Off, NC == NB is a
// constant and nothing of it is compiled.
template <int NB, int EPB, bool SENS, bool PERSIST, int NW = 4, bool BOXES = false, int PAIR = 0, class PRef = const Params&,
          class IORef = const StepIO&, class Hook = NoHook, bool MOV = false, bool POOL = false>
__device__ __forceinline__ void step_body(PRef P, StepSmem<NB, EPB, NW, POOL>& sm, int& next_env, IORef io, const bool last_step = true,
                                          const size_t row0 = 0, Hook hook = Hook()) {
    static_assert(EPB <= 64 && EPB >= 4 && NB % 2 == 0, "EPB / NB");
    static_assert(!POOL || (MOV && SENS && NB == 10 && EPB == 16 && NW == 8 && PAIR == 0),
                  "sector LiDAR: the sensor-options form of the 16-env mover twins");
    static_assert(!(PAIR && BOXES), "tile boxes describe 64-segment tiles");
    static_assert(!MOV || (NB == 10 && PAIR == 0 && ((EPB == 16 && NW == 8) || (EPB == 32 && NW == 8) || (EPB == 64 && NW == 16))),
                  "movers: 10 beams without the 128-segment passes, on 16 or 32 envs and 8 waves or on 64 envs and 16 waves");
    // movers in the big shapes (32 / 64 envs): the mover passes go through the three request slots of the static tiles (see the cast)
    constexpr bool kMovRot = MOV && EPB > 16;
    constexpr int kThreads = 64 * NW;
    constexpr bool kEval = std::is_same<typename std::remove_cv<typename std::remove_reference<IORef>::type>::type, EvalIO>::value;
    static_assert(!kEval || PERSIST, "the episode table is the persistent evaluation kernels' output");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // readfirstlane tells the compiler what it cannot see: the wave index is wave-uniform, so the work positions, the loop
    // exits and every `wave < PW` test below live in SGPRs and scalar branches instead of VGPRs and exec-mask loops
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int base = blockIdx.x * EPB;
    constexpr int B = NB;       // host dispatch guarantees P.B == NB
    [[maybe_unused]] const int pool = POOL ? P.pool : 1;   // rays per scan column
    const int NC = POOL ? NB * pool : NB;                   // rays cast (a constant unless POOL)
    constexpr int D = B + 6;
    constexpr int DP = D + 1;   // padded LDS row stride
    const int nloc = min(EPB, P.N - base);  // envs in this block
    const unsigned kInfBits = 0x7f800000u;
    // Pose lanes: TWO lanes per env (four in the small shapes).  The step needs the heading's (cos, sin) at the six substep arguments th_k + dth/2 and at the
    // final heading; lane 0 of the pair evaluates sincos(final heading), lane 1 sincos(dth / 2), and the six substep values follow
    // by rotating back from the final heading (angle addition, explicit fma: |error| ~ 1e-15, i.e. 1e-17 m on the pose).  The beam
    // directions and the sensor origin -- everything the scan's bits depend on -- come from the library sincos of the final heading,
    // exactly as in the oracle.  Rounds 1-3 spent 8 lanes per env (one library sincos per substep and lane): 8 pose waves per 64
    // envs, i.e. four times the float64 instruction issue for the same chain length; at configs[2] the pose phase was a fifth of the
    // launch's vector-unit time and its second wave per SIMD reached barrier A 0.5 us behind the first.
    // Lane 0 of each pair owns the env's float64 state across the phases.
    constexpr int LPE = (EPB <= 16) ? 4 : 2;            // pose lanes per env (lanes 2, 3 of a quad only share the beam directions:
                                                        // the small shapes are latency chains, the big ones issue-bound)
    constexpr int PWP = (LPE * EPB + 63) / 64;          // pose waves
    double x = 0, y = 0, th = 0, gx = 0, gy = 0, pdist = 0, dist = 0, yaw = 0, rel_theta = 0, diff = 0, ret0 = 0, path0 = 0;
    float2 act = make_float2(0.f, 0.f), pact = make_float2(0.f, 0.f);
    uint32_t ctr = 0, stepw = 0;
    [[maybe_unused]] uint32_t mv_ph0 = 0;   // MOV: the env's phase offset (Params::mov_phase0)
    [[maybe_unused]] uint2 mv_bp = make_uint2(0u, 1u);   // MOV: (base row, period) of the env's tape (Params::mov_bp)
    const int el_pose = (64 / LPE) * wave + (lane / LPE);  // env (local) this pose lane works for
    const int rr = lane % LPE;
    const bool pose_lane = (wave < PWP) && (el_pose < EPB);
    const int i = base + el_pose;
    constexpr int kSpecWave0 = (EPB <= 8) ? 0 : PWP;
    constexpr int kSpecLane0 = (EPB <= 8) ? EPB : 0;
    constexpr int PW = (EPB <= 8) ? 1 : PWP + (2 * EPB + 63) / 64;   // "front" waves: pose + spec; the others are ray waves
    static_assert(PW < NW, "front waves + at least one ray wave");
    static_assert(kSpecLane0 + ((EPB <= 8) ? 2 * EPB : 0) <= 64, "spec lanes of the small shapes fit wave 0");
    // ---- cast geometry: lane -> (env of the pass, segment of the tile)
    const int spl = P.seg_pack_log2;            // log2(lanes per env in one pass): 6, smaller when the map has <= 32 segments
    const int epp = 64 >> spl;                  // envs per pass
    const int sub = lane >> spl;
    const int j0 = lane & ((1 << spl) - 1);
    const int n_items = (nloc + epp - 1) / epp;
    // (locals: read through the kernarg segment, P's fields are scalar loads at every use -- these sit in the cast loop)
    const int S = P.S;
    const bool per_env = P.per_env != 0;
    // Non-temporal hint on the per-env segment stream (128-segment passes), by measurement (profiles/r04_nontemporal_loads_ablation.txt,
    // 16384 envs, us per step, default / non-temporal loads):
    //   one launch per step   S=128 13.11 / 12.64   S=256 18.58 / 17.62   S=512-1024 equal   S=1280 66.2 / 60.8   S=1536 82.4 / 71.8
    //   persistent (tape)     S=128  9.74 / 10.93   S=256 14.69 / 16.91   S=1024 41.6 / 48.2  S=1280 equal         S=1536 73.8 / 71.5
    // A launch reads every segment once and the next launch finds nothing of a >= 35 MB stream in the 8 x 4 MB of L2 (LRU), so
    // allocating the lines there is pure overhead: step_kernel streams (PAIR == 2) whenever the per-env stream is >= 32 MiB AND the shape is a
    // big 10-beam one (32 / 64 envs per workgroup: pick_shape; the ablation above was taken there -- the 8 / 16-env shapes of shards up to
    // 8192 envs and the 36-beam shapes keep the default policy).  A persistent workgroup re-reads ITS envs' segments every
    // step from its own XCD's L2 / the Infinity Cache (traffic 0.77 x algorithmic at configs[2]) and keeps the default policy until
    // one step's stream exceeds 1.25 x the Infinity Cache (bit 1 of per_env, navsim_set_map), where nothing can be re-used either.
    // (Below 32 MiB the stream fits the L2s and is left there: bit 2.)  The host picks the PAIR == 2 instantiation accordingly.
    const float4* const segs = P.seg;
    const int ntiles = (S + 63) >> 6;
    // PAIR (maps of more than 64 segments, one env per pass): a pass takes 128 segments, two per lane (j and j + 64) -- the
    // work-queue, address and loop instructions of a pass, about as many as its arithmetic, are paid once per 128 segments
    const int ntl = PAIR ? (ntiles + 1) >> 1 : ntiles;   // passes per item
    struct Pos { int it, t; };
    auto grab = [&]() __attribute__((always_inline)) {
        int v = 0;
        if (lane == 0) v = atomicAdd(&next_env, 1);
        return __builtin_amdgcn_readfirstlane(v);
    };
    // Requests are unconditional (a position past the end re-reads a clamped, valid address and is flagged invalid): the count of
    // requests issued after any given one is then the same on every path, which is what lets `s_waitcnt vmcnt(n)` -- the counter
    // retires in order -- wait for the OLDEST slot only and leave the two younger requests in flight.  With exec-masked loads the
    // compiler had to assume the path that skipped them and waited for vmcnt(0) before every tile: no prefetch at all.
    auto ld = [&](const Pos p, float4& g, bool& v) __attribute__((always_inline)) {
        const int el = p.it * epp + sub, j = (p.t << 6) + j0;
        v = (p.it < n_items) && (el < nloc) && (j < S);
        g = segs[(per_env ? (size_t)(base + min(el, nloc - 1)) * (size_t)S : (size_t)0) + (size_t)min(j, S - 1)];
    };
    auto ld2 = [&](const Pos p, float4& ga, bool& va, float4& gb, bool& vb) __attribute__((always_inline)) {
        const int j = (p.t << 7) + lane;
        const bool item = (p.it < n_items) && (p.it < nloc);
        va = item && (j < S);
        vb = item && (j + 64 < S);
        const float4* src = segs + (per_env ? (size_t)(base + min(p.it, nloc - 1)) * (size_t)S : (size_t)0);
        if constexpr (PAIR == 2) {   // the stream carries the non-temporal hint (a compile-time variant: as a run-time branch the
                                     // compiler waited for vmcnt(0) in front of every request, i.e. no tile stayed in flight)
            typedef float v4f_nt __attribute__((ext_vector_type(4)));
            const v4f_nt* srcv = reinterpret_cast<const v4f_nt*>(src);
            const v4f_nt a4 = __builtin_nontemporal_load(srcv + min(j, S - 1));
            const v4f_nt b4 = __builtin_nontemporal_load(srcv + min(j + 64, S - 1));
            ga = make_float4(a4.x, a4.y, a4.z, a4.w);
            gb = make_float4(b4.x, b4.y, b4.z, b4.w);
        } else {
            ga = src[min(j, S - 1)];
            gb = src[min(j + 64, S - 1)];
        }
    };
    Pos p0 = {n_items, 0}, p1 = {n_items, 0}, p2 = {n_items, 0};
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, g2 = g0, g0b = g0, g1b = g0, g2b = g0;
    bool v0 = false, v1 = false, v2 = false, v0b = false, v1b = false, v2b = false;
    auto request = [&](const Pos p, float4& ga, bool& va, float4& gb, bool& vb) __attribute__((always_inline)) {
        if constexpr (PAIR) ld2(p, ga, va, gb, vb);
        else ld(p, ga, va);
    };

    // ---------------- the first memory requests of the launch, ahead of everything else: what they need sits in the first 128
    // bytes of Params, i.e. in the first round of scalar kernarg loads (the rest of the set-up below costs three more rounds)
    if (wave >= PW) {
        // ray waves: static positions k = 0, 1, 2 of ray wave r: item r + RW (k / ntiles), tile k % ntiles
        constexpr int RW = NW - PW;
        const int r = wave - PW;
        p0 = Pos{r, 0};
        p1 = (ntl >= 2) ? Pos{r, 1} : Pos{r + RW, 0};
        p2 = (ntl >= 3) ? Pos{r, 2} : ((ntl == 2) ? Pos{r + RW, 0} : Pos{r + 2 * RW, 0});
        request(p0, g0, v0, g0b, v0b);
        request(p1, g1, v1, g1b, v1b);
        request(p2, g2, v2, g2b, v2b);
    }
    // pose waves: the beam table goes through LDS (lane k requests entry k here, right behind the state; written to LDS behind the
    // sincos, read back per beam): held in registers per lane it
    // cost 4 NB / LPE VGPRs from here to the end of part 1.  (The persistent rollout stages it once, before its first step.)
    constexpr int kBeamLd = (2 * StepSmem<NB, EPB, NW, POOL>::NR + 63) / 64;
    double beam_ld[kBeamLd];
    if (wave < PWP) {
        if (!PERSIST && pose_lane && el_pose < nloc) {
            th = P.th[i];
            act = io.action[i];
            ctr = P.rng_ctr[i];
            stepw = (uint32_t)P.ep_step[i];
            if constexpr (MOV) {
                if (rr == 0 && P.mov_phase0) mv_ph0 = (uint32_t)P.mov_phase0[i];
                if (rr == 0) mv_bp = mover_bp<PRef>(P, i);
            }
            if (rr == 0) {
                x = P.x[i]; y = P.y[i];
                gx = P.gx[i]; gy = P.gy[i]; pdist = P.past_dist[i];
                pact = io.past_override ? io.past_override[i] : P.past_action[i];
                ret0 = P.ep_ret[i];
                path0 = P.ep_path[i];
            }
        }
        if (!PERSIST) {
#pragma unroll
            for (int q = 0; q < kBeamLd; ++q) beam_ld[q] = P.beam_cs[min(lane + 64 * q, 2 * NC - 1)];
        }
    }

    // sensor-fidelity options (range noise, -inf below range_min) are compiled out of the default instantiation:
    // carrying them as run-time branches cost 1.2 us per launch (28.2 -> 27.0 us, configs[2])
    const float sigma = SENS ? P.sigma : 0.f;
    const int below_min = SENS ? P.below_min_mode : 0;


    // Parts 2 and 3 run lane-dense (a wave instruction costs the same with 8 or 64 active lanes, and the float64 geometry is
    // ~1000 of them): the goal geometry and the rules of ALL the block's envs on lanes 0..EPB-1 of wave 0 (the "owners"); the
    // next-episode records on 2 EPB "spec" lanes -- behind the owners in wave 0 for the small shapes, else on the waves that
    // follow the pose waves (they have nothing else to do before barrier A, so their record requests leave at kernel entry).
    // State crosses from the part-1 lanes through LDS (sv_*).  PW = the "front" waves: pose + spec; the others are ray waves.
    const bool own = (wave == 0) && (lane < nloc);            // lane = env for the geometry / rules lanes
    const int n_rec = P.respawn ? 2 : 1;
    // spec lanes: record spec_c of env spec_e
    const int sl = (wave - kSpecWave0) * 64 + lane - kSpecLane0;
    const int spec_c = sl / EPB;
    const int spec_e = sl % EPB;
    const bool spec_lane = (wave >= kSpecWave0) && (wave < PW) && (sl >= 0) && (spec_c < n_rec) && (spec_e < nloc);

    // The spec lanes request the cached records at kernel entry, whether they will turn out current or not: the first of
    // the two dependent round trips of the record path then runs under the pose phase instead of after barrier A, where the
    // spec wave is the last one into the cast.
    const bool spec = spec_lane && (P.auto_reset || (spec_c == 1));
    double pf_rgx = 0, pf_rgy = 0, pf_g0 = 0, pf_g1 = 0, pf_g2 = 0;
    float4 pf_tl = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned long long pf_ck = 0ull;   // (counter, start-pose index) kept as ONE 64-bit value until it is used: a uint2 was split
                                       // right behind the load, which made the wave wait for the whole round trip there
    uint32_t pf_rctr = 0;
    auto prefetch_records = [&]() __attribute__((always_inline)) {
        if (spec) {   // (the persistent rollout calls this after barrier A: measured slower there at the top of the step)
            const int ie = base + spec_e, c = spec_c;
            const size_t N = (size_t)P.N;
            if (c == 1) {
                pf_rgx = P.rsp_g[ie]; pf_rgy = P.rsp_g[N + ie]; pf_rctr = P.rsp_ctr[ie];
            }
            if (P.auto_reset) {
                const double* rg = P.rec_g + (size_t)c * 3 * N + ie;
                pf_g0 = rg[0]; pf_g1 = rg[N]; pf_g2 = rg[2 * N];
                pf_tl = P.rec_tail[(size_t)c * N + ie];
                pf_ck = reinterpret_cast<const unsigned long long*>(P.rec_ck)[(size_t)c * N + ie];
            }
        }
    };

    if (wave < PW) {
        // ---------------- pose lanes, part 1: motion + sensor frame
        // spec lanes on a wave of their own: the cached records are requested at kernel entry
        if constexpr (EPB > 8) { if (!PERSIST) prefetch_records(); }
        double delta_s = 0, delta_theta = 0, arg = 0;
        if (pose_lane && el_pose < nloc) {
            if (PERSIST) {
                const int e = el_pose;
                th = sm.st_d[2][e];
                act = sm.act_l[e];
                ctr = sm.st_ctr[e];
                stepw = sm.st_step[e];
                if constexpr (MOV) {
                    mv_ph0 = static_cast<StepSmemMov<NB, EPB, NW, POOL>&>(sm).mv_phase0[e];
                    mv_bp = static_cast<StepSmemMov<NB, EPB, NW, POOL>&>(sm).mv_bp[e];
                }
                if (rr == 0) {
                    x = sm.st_d[0][e]; y = sm.st_d[1][e];
                    gx = sm.st_d[3][e]; gy = sm.st_d[4][e]; pdist = sm.st_d[5][e];
                    pact = sm.st_pact[e];
                    ret0 = sm.st_d[6][e];
                    path0 = sm.st_d[7][e];
                }
            }
            // environment_new.py:273-278
            const double v = (double)act.x / 4;
            const double w = (double)act.y;
            // turtlebot3_fake.cpp:117-118, :133-146, :154-155
            const double vl = v - (w * kWheelSep / 2);
            const double vr = v + (w * kWheelSep / 2);
            const double dt = 1.0 / 30.0;
            const double wl = vl / kWheelRadius, wr = vr / kWheelRadius;
            const double wheel_l = wl * dt, wheel_r = wr * dt;
            delta_s = kWheelRadius * (wheel_r + wheel_l) / 2.0;
            delta_theta = kWheelRadius * (wheel_r - wheel_l) / kWheelSep;
            // the heading after the step is th0 + kSubsteps additions of delta_theta (same roundings as the serial loop, :160)
            for (int k = 0; k < kSubsteps; ++k) th += delta_theta;
            arg = (rr == 0) ? th : (delta_theta / 2.0);
            // MOV: the row this step's scan sees, base + (k + 1 + phase0) mod period of the env's tape with k the step counter before
            // the step -- integer work that issues under the latency of the float64 chain above
            if constexpr (MOV) {
                if (rr == 0)
                    static_cast<StepSmemMov<NB, EPB, NW, POOL>&>(sm).mv_phase[el_pose] = mover_row(mv_bp, (stepw & kStepMask) + 1u, mv_ph0);
            }
        }
        // spec lanes that share wave 0 with the pose lanes (small shapes): behind the wheel arithmetic -- the wait for the state
        // loads is over, the sincos covers this round trip
        if constexpr (EPB <= 8) { if (!PERSIST) prefetch_records(); }
        double cth = 1.0, sth = 0.0;
        if (pose_lane) {
            double sn, cs;
            sincos(arg, &sn, &cs);
            // lane 0's and lane 1's pair to every lane of the env's group through DPP quad permutes: no LDS round trip on the
            // chain to barrier A
            auto bcast = [](const double vv, auto sel) __attribute__((always_inline)) {
                constexpr int kCtrl = (LPE == 4) ? (decltype(sel)::value ? 0x55 : 0x00)     // quad_perm [k, k, k, k]
                                                 : (decltype(sel)::value ? 0xF5 : 0xA0);    // quad_perm [k, k, 2 + k, 2 + k]
                const int lo = __builtin_amdgcn_mov_dpp(__double2loint(vv), kCtrl, 0xF, 0xF, true);
                const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(vv), kCtrl, 0xF, 0xF, true);
                return __hiloint2double(hi, lo);
            };
            cth = bcast(cs, std::integral_constant<int, 0>{});   // final heading
            sth = bcast(sn, std::integral_constant<int, 0>{});
            const double ch = bcast(cs, std::integral_constant<int, 1>{}), sh = bcast(sn, std::integral_constant<int, 1>{});    // half a substep's turn
            if (rr == 0) {
                // substep k integrates along th_k + dth / 2 = final heading - (kSubsteps - 1/2 - k) dth  (:158-159): rotate back
                // by dth / 2 once, then by dth (double angle) per substep; the displacements are summed as they come, last substep
                // first (the serial loop's order would keep all six pairs alive)
                const double cd = fma(ch, ch, -(sh * sh)), sd = 2.0 * (sh * ch);
                double c = fma(cth, ch, sth * sh), s = fma(sth, ch, -(cth * sh));
                double dx = delta_s * c, dy = delta_s * s;
#pragma unroll
                for (int k = kSubsteps - 2; k >= 0; --k) {
                    const double c1 = fma(c, cd, s * sd);
                    s = fma(s, cd, -(c * sd));
                    c = c1;
                    dx += delta_s * c;
                    dy += delta_s * s;
                }
                x += dx;
                y += dy;
                const double ox = x + kLidarX * cth;
                const double oy = y + kLidarX * sth;
                sm.org[el_pose] = make_float2((float)ox, (float)oy);
                sm.hd[el_pose] = make_float2((float)cth, (float)sth);
                if (el_pose < nloc) {  // hand the env over to its geometry / rules lane
                    const int e = el_pose;
                    sm.sv_d[0][e] = x; sm.sv_d[1][e] = y; sm.sv_d[2][e] = th; sm.sv_d[3][e] = gx; sm.sv_d[4][e] = gy;
                    sm.sv_d[5][e] = pdist; sm.sv_d[10][e] = ret0;
                    sm.sv_d[11][e] = sqrt(dx * dx + dy * dy);   // np.linalg.norm(curr_pos - prev_pos), ppo.py:536-537
                    sm.sv_d[12][e] = path0;
                    sm.sv_act[e] = act; sm.sv_pact[e] = pact; sm.sv_ctr[e] = ctr; sm.sv_step[e] = stepw;
                }
            }
        }
        if (!PERSIST && wave < PWP) {
#pragma unroll
            for (int q = 0; q < kBeamLd; ++q)
                if (lane + 64 * q < 2 * NC) sm.beam[lane + 64 * q] = beam_ld[q];
        }
        if (pose_lane) {
            // the table entries just written by this wave (LDS operations of a wave complete in order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if constexpr (POOL) {   // up to 40 rays: a loop (the table in registers would be 40 VGPRs beside the persistent kernels' policy)
#pragma unroll 2
                for (int b = rr; b < NC; b += LPE) {
                    const double bc = sm.beam[b], bs = sm.beam[NC + b];
                    const double c = cth * bc - sth * bs;
                    const double s = sth * bc + cth * bs;
                    sm.dir[b * EPB + el_pose] = make_float2((float)c, (float)s);
                }
            } else {
            constexpr int kBeamIt = (NB + LPE - 1) / LPE;
            double bc[kBeamIt], bs[kBeamIt];
#pragma unroll
            for (int q = 0; q < kBeamIt; ++q) {   // all reads first: one LDS latency
                const int b = min(rr + LPE * q, NB - 1);
                bc[q] = sm.beam[b];
                bs[q] = sm.beam[NB + b];
            }
#pragma unroll
            for (int q = 0; q < kBeamIt; ++q) {
                const int b = rr + LPE * q;
                if (b < NB) {
                    const double c = cth * bc[q] - sth * bs[q];
                    const double s = sth * bc[q] + cth * bs[q];
                    sm.dir[b * EPB + el_pose] = make_float2((float)c, (float)s);
                }
            }
            }
        }
        // the ray waves' first three tiles are pre-assigned (requested before barrier A): 1, 2 or 3 items per ray wave
        if (tid == 0) next_env = (NW - PW) * (ntl == 1 ? 3 : (ntl == 2 ? 2 : 1));
    }
    if (wave >= PW) {
        // ---------------- other waves, part 1 (their tile requests went out at the top): LDS traffic under that round trip
        for (int k = tid - 64 * PW; k < NC * EPB; k += kThreads - 64 * PW) sm.rng[k] = kInfBits;
        if (tid - 64 * PW < EPB) {
            sm.mn_bits[tid - 64 * PW] = kInfBits;
            sm.neg[tid - 64 * PW] = 0u;
        }
    }
    // the goal rejection rectangles (the spec lanes' recompute path reads them after barrier A) and the tile boxes: staged by the
    // waves behind the pose waves -- spec waves where the shape has them (their only other work before barrier A is the record
    // request), else the ray waves, behind their tile requests.  A ray wave that waits for this round trip also waits for its
    // three tiles (the counter retires in order), which is why the big shapes keep it off them.  (The persistent rollout stages
    // the rectangles once, before its first step.)
    if (wave >= PWP) {
        constexpr int kStageThreads = 64 * (NW - PWP);
        const int st = tid - 64 * PWP;
        constexpr bool kOnFront = (PW > PWP);   // staging waves = the front waves behind the pose waves
        const bool mine = kOnFront ? (wave < PW) : true;
        constexpr int kStride = kOnFront ? 64 * (PW - PWP) : kStageThreads;
        if (mine) {
            if (BOXES) for (int k = st; k < ntiles; k += kStride) sm.tbox[k] = P.tile_box[k];
            static_assert(sizeof(Rects) % 8 == 0, "Rects is copied in 8-byte words");
            if (!PERSIST)
                for (int k = st; k < (int)(sizeof(Rects) / 8); k += kStride)
                    reinterpret_cast<uint64_t*>(&sm.rects)[k] = reinterpret_cast<const uint64_t*>(P.rects)[k];
        }
    }
    __syncthreads();  // barrier A: origins / directions visible, work counter set

    if (sigma > 0.f && pose_lane && el_pose < nloc) {
        // range noise for this step: lane rr draws beams rr, rr + 2, ... (off the critical path: the others ray-cast)
        for (int b = rr; b < NC; b += LPE)   // (POOL: keyed by the dense ray index, as a handle with NC beams keys its beams)
            sm.noise[b * EPB + el_pose] = lidar_noise(P.key0, P.key1, P.env_id_base + (uint64_t)i, ctr, stepw & kStepMask, b);
    }
    // ---------------- part 2 (the other waves are already ray-casting): goal geometry.
    // An owner lane works on the pose its env just moved to.  The spec lanes hold the episode that starts if this step
    // ends the current one (ppo.py:582-593 + Env.reset, environment_new.py:312-382): an episode draws from the goal stream
    // only when it ends, so its successor is known from the moment it starts -- record 0 for an end by collision or
    // timeout (and by arrival when respawn_on_arrive is off), record 1 for an end by arrival after the arrival re-spawn
    // draw of :245-253.  Records live in HBM; kRecValid in the env's ep_step word says they match its draw counter.
    // A spec lane of an env whose flag is clear (it was reset, or its goal stream moved) recomputes and stores them.
    // (wave < PW is implied; spelt out so that the ray waves' path to the cast holds no request the compiler would have to
    // count: their three tile requests stay the youngest ones and the first cull waits for vmcnt(2), not vmcnt(0))
    if ((wave < PW) && (own || spec)) {
        const int e = own ? lane : spec_e;
        const int ie = base + e;
        if (own) {
            const double px = sm.sv_d[0][e], py = sm.sv_d[1][e], tgx = sm.sv_d[3][e], tgy = sm.sv_d[4][e];
            // yaw: rint of the heading in degrees; the quaternion route of :142 only when the two could round differently
            const double pth = sm.sv_d[2][e];
            bool exact;
            yaw = yaw_fast(pth, &exact);
            if (__builtin_expect(!exact, 0)) yaw = yaw_from_quat(sin(pth / 2), cos(pth / 2));
            goal_rel(px, py, tgx, tgy, yaw, rel_theta, diff);
            dist = hypot(tgx - px, tgy - py);  // environment_new.py:203 ; getGoalDistace, :116-120
            sm.sv_d[6][e] = dist;
            // the six non-lidar entries of the observation row depend on the pose only: written here, under the cast, instead
            // of in part 3 (the float64 division and the three exact constant divisions were a fifth of its dependent chain)
            float* row = sm.obs + e * DP;
            const float2 pa = sm.sv_pact[e];
            row[B + 0] = pa.x;                          // environment_new.py:299-300
            row[B + 1] = pa.y;
            row[B + 2] = (float)(dist / P.diag);        // :301
            row[B + 3] = (float)div_const(yaw, 360.0, 1.0 / 360.0);        // yaw / 360, rel_theta / 360, diff_angle / 180:
            row[B + 4] = (float)div_const(rel_theta, 360.0, 1.0 / 360.0);  // correctly rounded over these operands' domains
            row[B + 5] = (float)div_const(diff, 180.0, 1.0 / 180.0);       // (integers, k/100), tools/verify
        } else {
            const int c = spec_c;
            const size_t N = (size_t)P.N;
            double px = 0, py = 0, pth = 0, tgx = 0, tgy = 0, rgx = 0, rgy = 0, rdist = 0;
            float4 tl = make_float4(0.f, 0.f, 0.f, 0.f);
            uint32_t sctr = sm.sv_ctr[e], rctr = sctr;
            int sk = 0;
            // the scan every reset at start pose k observes: rows of NB floats are 8-byte aligned (NB even), all NB / 2 requests
            // go out before the first is awaited (one memory latency instead of NB / 2)
            // (POOL: the raw hits of all NC rays -- the noise is per ray; the row goes to LDS in a loop where it is stored below, not
            // through NC / 2 registers)
            float2 row[POOL ? 1 : NB / 2];
            [[maybe_unused]] const float2* row_src = nullptr;
            auto request_row = [&](const int k) __attribute__((always_inline)) {
                const float2* sp = reinterpret_cast<const float2*>((SENS ? P.spawn_scan : P.spawn_obs) +
                                                                   (((MOV ? P.spawn_per_env : P.per_env) ? (size_t)ie * P.K : 0) + k) * NC);
                if constexpr (POOL) {
                    row_src = sp;
                } else {
#pragma unroll
                for (int b = 0; b < NB / 2; ++b) row[b] = sp[b];
                }
            };
            const bool current = (sm.sv_step[e] & kRecValid) != 0;
            if (PERSIST && current) prefetch_records();
            if (current) {   // the records requested at kernel entry; their start pose and scan row are requested here, ahead of
                             // the recomputation the other lanes of the wave may have to go through
                if (c == 1) {
                    rgx = pf_rgx; rgy = pf_rgy; rctr = pf_rctr;
                }
                if (P.auto_reset) {
                    tgx = pf_g0; tgy = pf_g1; rdist = pf_g2;
                    tl = pf_tl;
                    sctr = (uint32_t)pf_ck; sk = (int)(uint32_t)(pf_ck >> 32);
                    px = P.starts[3 * sk]; py = P.starts[3 * sk + 1]; pth = P.starts[3 * sk + 2];
                    request_row(sk);
                }
            }
            if (!current) {
                if (c == 1) {
                    sample_goal<PRef, MOV>(P, sm.rects, ie, 1, sctr, rgx, rgy);
                    rctr = sctr;
                    P.rsp_g[ie] = rgx; P.rsp_g[N + ie] = rgy; P.rsp_ctr[ie] = rctr;
                }
                if (P.auto_reset) {
                    sample_episode<PRef, MOV>(P, sm.rects, ie, sctr, sk, tgx, tgy);
                    request_row(sk);
                    px = P.starts[3 * sk]; py = P.starts[3 * sk + 1]; pth = P.starts[3 * sk + 2];
                    double ryaw, rrel, rdiff;
                    ryaw = P.starts_sc[sk];   // = yaw_from_quat((sin, cos)(pth / 2)), tabulated by starts_sc_kernel
                    goal_rel(px, py, tgx, tgy, ryaw, rrel, rdiff);
                    rdist = hypot(tgx - px, tgy - py);
                    tl = make_float4((float)(rdist / P.diag), (float)(ryaw / 360), (float)(rrel / 360), (float)(rdiff / 180));
                    double* rg = P.rec_g + (size_t)c * 3 * N + ie;
                    rg[0] = tgx; rg[N] = tgy; rg[2 * N] = rdist;
                    P.rec_tail[(size_t)c * N + ie] = tl;
                    P.rec_ck[(size_t)c * N + ie] = make_uint2(sctr, (uint32_t)sk);
                }
            }
            if (P.auto_reset) {
                if constexpr (POOL) {
#pragma unroll 5
                    for (int b = 0; b < NC / 2; ++b) {
                        const float2 v = row_src[b];
                        sm.sp_scan[c][e][2 * b] = v.x;
                        sm.sp_scan[c][e][2 * b + 1] = v.y;
                    }
                } else {
#pragma unroll
                for (int b = 0; b < NB / 2; ++b) {
                    sm.sp_scan[c][e][2 * b] = row[b].x;
                    sm.sp_scan[c][e][2 * b + 1] = row[b].y;
                }
                }
            }
            sm.sp_d[c][0][e] = px; sm.sp_d[c][1][e] = py; sm.sp_d[c][2][e] = pth; sm.sp_d[c][3][e] = tgx;
            sm.sp_d[c][4][e] = tgy; sm.sp_d[c][5][e] = rdist;
            sm.sp_tail[c][e] = tl;
            sm.sp_ctr[c][e] = sctr;
            sm.sp_k[c][e] = sk;
            if (c == 1) {
                sm.sp_rg[0][e] = rgx; sm.sp_rg[1][e] = rgy;
                sm.sp_rctr[e] = rctr;
            }
        }
    }
    // ---------------- the cast
    {
        float4* const q4 = sm.q4[wave];
        unsigned* const qe = sm.qe[wave];
        float4* const r4 = sm.r4[wave];
        unsigned* const re = sm.re[wave];
        unsigned* const pe = sm.pe[wave];
        int qhead = 0, qtail = 0, rhead = 0, rtail = 0, phead = 0, ptail = 0;   // wave-uniform
        // Stage B, the exact tests.  With 10 beams every queued segment is tested against ALL beams (lane = segment: 206 vector
        // instructions per 64 segments).  With 36 beams that is 770 instructions in one wave, although stage A2 has just bounded
        // the beams the segment's arc can hold -- so there (kPairB) a queued segment is expanded into entries of kBeamsPerEntry
        // consecutive beams of that extent and a pass tests 64 ENTRIES (lane = entry): the same arithmetic on the same (a, b, o, d),
        // on the beams that can be hit only, so the scan keeps its bits (the extent is as conservative as the A2 cull itself).
        // Measured (tools/time_step.py, same box): BASELINE configs[3]'s shard (4096 envs, stage_4, 36 beams) 15.8 -> 12.5 us per
        // launch, tape form 12.7 -> 9.8 us per step.  At 10 beams the expansion costs more than it saves -- a wave of a configs[2]
        // workgroup queues only ~40 segments per step, one partial pass either way: 12.96 -> 13.19 us -- so it stays off there.
        constexpr bool kPairB = POOL || NB > 16;   // (POOL: 20..40 rays, the entries of the 36-beam path)
        // (Rejected, profiles/r04_stage_b_pool_ablation.txt: pooling what the 16 waves' stage-B queues hold at the end of a step --
        // a wave queues ~40 segments per step, so its one pass runs with 60 % of its lanes -- removes 6.5 of 16 passes per
        // workgroup and step and is 14-17 % SLOWER: the passes land on the tail of the slowest wave, behind dependent LDS atomics.)
        constexpr int kBeamsPerEntry = kPairB ? 4 : 2;
        auto exact_tests = [&](const bool on, const float4 g, const unsigned el, const int b_first, const int n_b, auto n_max)
                               __attribute__((always_inline)) {
            constexpr int kMaxB = decltype(n_max)::value;
            const float2 o = sm.org[el];
            const float rx = g.x - o.x, ry = g.y - o.y;
            const float ex = g.z - g.x, ey = g.w - g.y;
            const float k = fmaf(rx, ey, -(ry * ex));
            // div_pos needs |den| in [2^-60, 2^20]: true unless the segment is degenerate-small
            // (coordinates are documented to be < 2^19); such passes take the plain IEEE divide.
            const bool tiny = fmaxf(fabsf(ex), fabsf(ey)) < 0x1p-10f;
            if (__builtin_expect(__any(tiny), 0)) {
                // the empty volatile asm keeps this a real (wave-uniform) branch the compiler cannot speculate
                asm volatile("; degenerate-segment pass" ::: "memory");
                for (int u = 0; u < kMaxB; ++u) {
                    const int b = min(b_first + u, NC - 1);
                    const float2 d = sm.dir[b * EPB + el];
                    const unsigned bits = __float_as_uint(ray_seg(rx, ry, ex, ey, k, d.x, d.y)) & 0x7fffffffu;
                    if (on && u < n_b && bits < kInfBits) atomicMin(&sm.rng[b * EPB + el], bits);
                }
            } else {
#pragma unroll
                for (int u = 0; u < kMaxB; ++u) {
                    const int b = (kMaxB == NB) ? u : min(b_first + u, NC - 1);
                    const float2 d = sm.dir[b * EPB + el];
                    const unsigned bits = ray_seg_bits(rx, ry, ex, ey, k, d.x, d.y);
                    // hits only: same-address LDS atomics of a wave serialise, and most lanes miss
                    if (on && u < n_b && bits < kInfBits) atomicMin(&sm.rng[b * EPB + el], bits);
                }
            }
        };
        // up to 64 queued segments against every beam of their env (lane = segment): the tail of a small map, whose whole cast
        // is one pass -- there the two extra queue hops of expand / testB would only add latency
        auto flushB = [&](int n) __attribute__((always_inline)) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bool on = lane < n;
            const int slot = (rhead + lane) & 127;
            const float4 g = on ? r4[slot] : make_float4(0.f, 0.f, 1.f, 0.f);
            const unsigned el = on ? (kPairB ? (re[slot] & 255u) : re[slot]) : 0u;
            exact_tests(on, g, el, 0, NB, std::integral_constant<int, NB>{});
            rhead += n;
        };
        // (Measured without gain, round 4: splitting a wave's LAST pass -- ~40 segments at configs[2], 15-30 on a small shared map --
        // over two or four lanes per segment, each testing half / a quarter of the beams: 117 / 75 instead of 206 instructions on the
        // tail that barrier B waits for, and configs[2] 12.6-12.7 vs 12.6-12.7 us, the 16-env rollout 5.11-5.18 vs 5.06-5.10.)
        // up to 64 entries (lane = entry): kBeamsPerEntry consecutive beams of one queued segment
        auto testB = [&](int n) __attribute__((always_inline)) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bool on = lane < n;
            const unsigned e = on ? pe[(phead + lane) & 127] : 0u;
            const int slot = (int)(e & 127u);
            const float4 g = on ? r4[slot] : make_float4(0.f, 0.f, 1.f, 0.f);
            const unsigned el = on ? (re[slot] & 255u) : 0u;
            exact_tests(on, g, el, (int)((e >> 8) & 255u), (int)(e >> 16), std::integral_constant<int, kBeamsPerEntry>{});
            phead += n;
        };
        // the oldest n queued segments -> entries.  Lane = segment writes its j-th entry in round j (ballot compaction per round:
        // no prefix sum; a pillar facet is done after round 0, a wall across the whole fan after NB / kBeamsPerEntry rounds).
        auto expand = [&](int n) __attribute__((always_inline)) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int slot = (rhead + lane) & 127;
            const unsigned w = (lane < n) ? re[slot] : 0u;
            const int b0 = (int)((w >> 8) & 255u), c = (int)(w >> 16);
            const int ne = (c + kBeamsPerEntry - 1) / kBeamsPerEntry;   // 0 on the lanes beyond n
            rhead += n;
            for (int j = 0;; ++j) {   // wave-uniform
                const bool mine = ne > j;
                const unsigned long long bal = __ballot(mine);
                if (!bal) break;
                const int off = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                if (mine)
                    pe[(ptail + off) & 127] = (unsigned)slot | ((unsigned)(b0 + kBeamsPerEntry * j) << 8) |
                                              ((unsigned)min(kBeamsPerEntry, c - kBeamsPerEntry * j) << 16);
                ptail += __popcll(bal);
                if (ptail - phead >= 64) testB(64);
            }
            // ... and the rest: an entry names its segment by the r4 slot, and the next A2 pass may rewrite the slots of the
            // segments just expanded (the ring only protects the ones still queued), so no entry outlives its expansion
            if (ptail > phead) testB(ptail - phead);
        };
        // stage A2, dense over up to 64 survivors of the range / behind cull: does the arc the segment subtends, as seen
        // from the sensor, hold a beam at all -- and which?  (Beams are 20 degrees apart, a pillar facet at 2 m subtends 2.)
        constexpr float kInvDeltaNB = (float)((NB - 1) / (2.0 * kAngleMax)), kBeamMargin = 0.02f;
        // (POOL: the constant an NB = 20 | 30 | 40 instantiation folds)
        const float kInvDelta = !POOL ? kInvDeltaNB
                                      : pool == 2 ? (float)((2 * NB - 1) / (2.0 * kAngleMax))
                                      : pool == 3 ? (float)((3 * NB - 1) / (2.0 * kAngleMax)) : (float)((4 * NB - 1) / (2.0 * kAngleMax));
        auto flushA2 = [&](int n) __attribute__((always_inline)) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bool on = lane < n;
            const int slot = (qhead + lane) & 127;
            const float4 g = on ? q4[slot] : make_float4(0.f, 0.f, 1.f, 0.f);
            const unsigned el = on ? qe[slot] : 0u;
            const float2 o = sm.org[el], h = sm.hd[el];
            const float ax = g.x - o.x, ay = g.y - o.y, bx = g.z - o.x, by = g.w - o.y;
            const float xa = fmaf(ax, h.x, ay * h.y), ya = fmaf(ay, h.x, -(ax * h.y));
            const float xb = fmaf(bx, h.x, by * h.y), yb = fmaf(by, h.x, -(bx * h.y));
            bool bad_a, bad_b;
            const float fa = beam_coord(xa, ya, 2.f * kInvDelta, (float)kAngleMax * kInvDelta, &bad_a);
            const float fb = beam_coord(xb, yb, 2.f * kInvDelta, (float)kAngleMax * kInvDelta, &bad_b);
            const float lo = fminf(fa, fb), hi = fmaxf(fa, fb);
            // the arc runs through straight-behind iff the segment crosses the negative X axis: Y changes sign and the
            // crossing X = cross(a, b) / (yb - ya) is negative
            const float kl = fmaf(xa, yb, -(xb * ya)), ey = yb - ya, ex = xb - xa;
            const bool wrap = (ya * yb < 0.f) && (kl * ey < 0.f);
            const bool through = kl * kl <= 1e-6f * fmaf(ex, ex, ey * ey);   // the line passes within 1 mm of the sensor
            const float ce = ceilf(lo - kBeamMargin), fl = floorf(hi + kBeamMargin);
            const bool inside = (fl >= ce) && (fl >= 0.f) && (ce <= (float)(NC - 1));
            const bool outside = (lo + kBeamMargin >= 0.f) || (hi - kBeamMargin <= (float)(NC - 1));
            // an arc whose beam extent cannot be trusted (an endpoint next to the sensor or straight behind it, a line through the
            // sensor, an arc through straight-behind) keeps the segment for every beam
            const bool all = bad_a || bad_b || through || wrap;
            const bool keep = on && (all ? (bad_a || bad_b || through || outside) : inside);
            unsigned ext = 0u;
            if constexpr (kPairB) {   // beams ce .. fl of the fan (v_med3 clamps; a NaN coordinate has set `bad`)
                const float b_lo = __builtin_amdgcn_fmed3f(ce, 0.f, (float)(NC - 1)), b_hi = __builtin_amdgcn_fmed3f(fl, 0.f, (float)(NC - 1));
                ext = all ? ((unsigned)NC << 16) : (((unsigned)(int)b_lo << 8) | ((unsigned)((int)(b_hi - b_lo) + 1) << 16));
            }
            qhead += n;
            const unsigned long long bal = __ballot(keep);
            if (bal) {
                const int off = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                if (keep) {
                    const int s2 = (rtail + off) & 127;
                    r4[s2] = g;
                    re[s2] = el | ext;
                }
                rtail += __popcll(bal);
                if (rtail - rhead >= 64) {
                    if constexpr (kPairB) expand(64);
                    else flushB(64);
                }
            }
        };
        // stage A: cull + compaction of one tile (64 lanes = 64 segments, or 64 / epp segments of epp envs)
        // (Round 4 tried a leaner form -- the distance test in the world frame, "behind" as the half plane X < -1 mm: 12 fewer
        // vector instructions per 128-segment pass, SQ_INSTS_VALU -2.4 % -- and measured it SLOWER on the same box, configs[2]
        // 13.18 vs 13.08 us, the house map 34.6 vs 33.3 us: the cast is not bound by the instruction count alone.)
        auto keep_of = [&](const float4 g, const float2 o, const float2 h) __attribute__((always_inline)) -> bool {
            // endpoints in the robot frame (X ahead, Y left); float32 throughout: this decides only what is tested exactly
            const float ax = g.x - o.x, ay = g.y - o.y, bx = g.z - o.x, by = g.w - o.y;
            const float xa = fmaf(ax, h.x, ay * h.y), ya = fmaf(ay, h.x, -(ax * h.y));
            const float xb = fmaf(bx, h.x, by * h.y), yb = fmaf(by, h.x, -(bx * h.y));
            // behind: both endpoints inside the convex cone X < -1e-3 |Y|; the beams span +-(pi/2 + 1.2e-6)
            const bool behind = (fmaf(1e-3f, fabsf(ya), xa) < 0.f) && (fmaf(1e-3f, fabsf(yb), xb) < 0.f);
            // far: distance from the sensor to the segment above 3.5 m (threshold 12.3 = (3.5 * 1.002)^2).  The closest point
            // is a + t e with t = clamp(-a.e / e.e, 0, 1); the error of the hardware reciprocal moves it by < 1e-7 |e|, far
            // inside the 7 mm margin for any segment shorter than 10 km; a zero-length segment gives t = 0 (0 x inf = NaN
            // takes v_med3's minimum).  So the test stays conservative.
            const float ex = xb - xa, ey = yb - ya;
            const float e2 = fmaf(ex, ex, ey * ey), ae = fmaf(xa, ex, ya * ey);
            const float t = __builtin_amdgcn_fmed3f(-ae * __builtin_amdgcn_rcpf(e2), 0.f, 1.f);
            const float cx = fmaf(t, ex, xa), cy = fmaf(t, ey, ya);
            const float d2 = fmaf(cx, cx, cy * cy);
            // d2 < 1e-6: the segment passes within 1 mm of the sensor, where the angles are noise: keep
            return (d2 < 1e-6f) || !(behind || (d2 > 12.3f));
        };
        auto push = [&](const float4 g, const unsigned el, const bool keep) __attribute__((always_inline)) {
            const unsigned long long bal = __ballot(keep);
            if (bal) {
                const int off = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                if (keep) {
                    const int slot = (qtail + off) & 127;
                    q4[slot] = g;
                    qe[slot] = el;
                }
                qtail += __popcll(bal);
                if (qtail - qhead >= 64) flushA2(64);
            }
        };
        auto cull = [&](const Pos p, const float4 g, const bool v) __attribute__((always_inline)) {
            const int el = min(p.it * epp + sub, nloc - 1);
            const float2 o = sm.org[el], h = sm.hd[el];
            push(g, (unsigned)el, keep_of(g, o, h) & v);   // evaluated unconditionally, see cull2
        };
        auto cull2 = [&](const Pos p, const float4 ga, const bool va, const float4 gb, const bool vb) __attribute__((always_inline)) {
            const int el = min(p.it, nloc - 1);
            const float2 o = sm.org[el], h = sm.hd[el];
            // both tests unconditionally (an invalid lane holds a clamped, valid segment): `va && keep_of(...)` made each an exec-masked
            // branch of its own, one dependent chain after the other; as two independent chains the compiler interleaves them
            // (configs[2] 12.87 -> 12.62 us per launch, tape 9.30 -> 9.18, same box)
            const bool ka = keep_of(ga, o, h) & va, kb = keep_of(gb, o, h) & vb;
            push(ga, (unsigned)el, ka);   // at most 63 + 64 queued before either flush: the ring holds 128
            push(gb, (unsigned)el, kb);
        };
        auto consume = [&](const Pos p, const float4 ga, const bool va, const float4 gb, const bool vb) __attribute__((always_inline)) {
            if constexpr (PAIR) cull2(p, ga, va, gb, vb);
            else cull(p, ga, va);
        };
        // BOXES: bit t of item_live(env) = tile t can matter for this env's pose: lane = tile, the same conservative range /
        // behind-the-fan tests as stage A applied to the tile's bounding box (all four corners inside the behind cone)
        auto item_live = [&](const int it) __attribute__((always_inline)) -> unsigned long long {
            const int el = min(it, nloc - 1);
            const float2 o = sm.org[el], h = sm.hd[el];
            const float4 bx = sm.tbox[lane];
            const float dx = fmaxf(fmaxf(bx.x - o.x, o.x - bx.z), 0.f), dy = fmaxf(fmaxf(bx.y - o.y, o.y - bx.w), 0.f);
            const bool far = fmaf(dx, dx, dy * dy) > 12.3f;
            const float x0 = bx.x - o.x, x1 = bx.z - o.x, y0 = bx.y - o.y, y1 = bx.w - o.y;
            auto behind = [&](float cx, float cy) {
                const float X = fmaf(cx, h.x, cy * h.y), Y = fmaf(cy, h.x, -(cx * h.y));
                return fmaf(1e-3f, fabsf(Y), X) < 0.f;
            };
            const bool back = behind(x0, y0) && behind(x1, y0) && behind(x0, y1) && behind(x1, y1);
            return __ballot((lane < ntiles) && !(far || back));
        };
        unsigned long long cur_live = 0ull;   // BOXES: live tiles of the item the last assigned position belongs to
        auto next_item = [&]() __attribute__((always_inline)) -> Pos {   // BOXES: first live tile of the next item that has one
            for (;;) {
                const int it = grab();
                if (it >= n_items) return Pos{it, 0};
                cur_live = item_live(it);
                if (cur_live) return Pos{it, (int)__builtin_ctzll(cur_live)};
            }
        };
        auto advance = [&](const Pos p) __attribute__((always_inline)) -> Pos {
            if (p.it >= n_items) return p;
            if (BOXES) {
                const unsigned long long rest = (p.t >= 63) ? 0ull : (cur_live & (~0ull << (p.t + 1)));
                if (rest) return Pos{p.it, (int)__builtin_ctzll(rest)};
                return next_item();
            }
            if (p.t + 1 < ntl) return Pos{p.it, p.t + 1};
            return Pos{grab(), 0};
        };
        if (wave < PW) {   // pose waves join when part 2 is done
            p0 = BOXES ? next_item() : Pos{grab(), 0};
            request(p0, g0, v0, g0b, v0b);
            p1 = advance(p0);
            request(p1, g1, v1, g1b, v1b);
            p2 = advance(p1);
            request(p2, g2, v2, g2b, v2b);
        } else if (BOXES) {   // ray waves: the live tiles of the item their last pre-assigned tile belongs to
            cur_live = (p2.it < n_items) ? item_live(p2.it) : 0ull;
        }
        // MOV: the tape segments of this step, lane = segment (several envs per pass when the tape has <= 32 segments per phase, as
        // for a small static map).  Pass m covers envs m mepp .. m mepp + mepp - 1 and belongs to ray wave m % RW: static, so that
        // every request leaves here -- right behind barrier A, where the phases became visible -- and lands under the static
        // tiles.  The requests are unconditional and EVERY wave issues them (a front wave's, and a pass past the last env, re-read a
        // clamped valid address and are never consumed): the count of requests behind the three static slots is then the same on
        // every path into the loop below, which is what lets its waits name the oldest slot only.
        // (The 16-env shape: three passes.  The big shapes would hold six tiles here, beside the three static slots, in a kernel
        // that sits at its 128 registers: they take the rotation below instead.)
        constexpr int kMovRW = NW - PW, kMovPasses = (MOV && !kMovRot) ? (EPB + kMovRW - 1) / kMovRW : 1;
        [[maybe_unused]] float4 mg[kMovPasses];
        [[maybe_unused]] int m_el[kMovPasses];
        [[maybe_unused]] bool m_v[kMovPasses];
        if constexpr (MOV && !kMovRot) {
            const StepSmemMov<NB, EPB, NW, POOL>& ms = static_cast<const StepSmemMov<NB, EPB, NW, POOL>&>(sm);
            const int mspl = P.mov_pack_log2, M = P.mov_M;
            const int mepp = 64 >> mspl, msub = lane >> mspl, mj = lane & ((1 << mspl) - 1);
            const float4* const tape = P.mov_tape;
#pragma unroll
            for (int q = 0; q < kMovPasses; ++q) {
                const int el = ((wave - PW) + kMovRW * q) * mepp + msub;
                m_v[q] = (wave >= PW) && (el < nloc) && (mj < M);
                m_el[q] = min(max(el, 0), nloc - 1);
                mg[q] = tape[(size_t)ms.mv_phase[m_el[q]] * (size_t)M + (size_t)min(mj, M - 1)];
            }
        }
        // MOV in the big shapes (kMovRot): the mover passes are further positions of the SAME three-slot rotation.  Position
        // n_items + q of ray wave r is its q-th mover pass (envs (r + RW q) mepp ..: the static assignment of the 16-env shape), and
        // the wave's stream runs on behind its last static tile up to n_end = n_items + its number of passes that hold an env.  A slot
        // whose static stream has ended requests a mover pass where it used to re-read a clamped address, so the tape segments are in
        // flight under the last static tiles, no register holds a tile beside the three slots, and every turn of a slot still issues
        // exactly ONE request on every path (ld or ld_mov, by a wave-uniform test): the count of requests behind any given one stays
        // the same on every path, i.e. the waits of the loop still name the oldest slot only.  The phases are published at barrier A:
        // a position the ray waves pre-assigned past the last item before it (never requested as a mover pass there) is re-requested
        // here, in slot order, so the three slots are again requested oldest first on every path into the loop.
        [[maybe_unused]] int n_end_m = n_items, mv_spl = 6, mv_M = 1;
        [[maybe_unused]] const float4* mv_tape = nullptr;
        if constexpr (kMovRot) {
            mv_spl = P.mov_pack_log2;
            mv_M = P.mov_M;
            mv_tape = P.mov_tape;
            const int n_mit = (nloc + (64 >> mv_spl) - 1) >> (6 - mv_spl);   // mover passes of the workgroup
            if (wave >= PW && n_mit > wave - PW) n_end_m = n_items + (n_mit - (wave - PW) + kMovRW - 1) / kMovRW;
        }
        const int n_end = kMovRot ? n_end_m : n_items;
        // lane -> (env, segment) of mover pass q = p.it - n_items of this wave; the env clamped to a present one
        auto mov_el = [&](const Pos p, bool& present) __attribute__((always_inline)) -> int {
            const int el = ((wave - PW) + kMovRW * (p.it - n_items)) * (64 >> mv_spl) + (lane >> mv_spl);
            present = (p.it < n_end) && (el < nloc);
            return min(max(el, 0), nloc - 1);
        };
        auto ld_mov = [&](const Pos p, float4& g, bool& v) __attribute__((always_inline)) {
            const int mj = lane & ((1 << mv_spl) - 1);
            bool present;
            const int el = mov_el(p, present);
            v = present && (mj < mv_M);
            g = mv_tape[(size_t)static_cast<const StepSmemMov<NB, EPB, NW, POOL>&>(sm).mv_phase[el] * (size_t)mv_M + (size_t)min(mj, mv_M - 1)];
        };
        auto request_m = [&](const Pos p, float4& ga, bool& va, float4& gb, bool& vb) __attribute__((always_inline)) {
            if constexpr (kMovRot) {
                if (p.it >= n_items) ld_mov(p, ga, va);
                else request(p, ga, va, gb, vb);
            } else {
                request(p, ga, va, gb, vb);
            }
        };
        // the cull of a mover pass: that of a static tile, plus: a segment with a NaN coordinate (the documented padding of a phase)
        // is dropped here instead of failing every exact test
        auto consume_m = [&](const Pos p, const float4 ga, const bool va, const float4 gb, const bool vb) __attribute__((always_inline)) {
            if constexpr (kMovRot) {
                if (p.it >= n_items) {
                    bool present;
                    const int el = mov_el(p, present);
                    const float2 o = sm.org[el], h = sm.hd[el];
                    const float sum = (ga.x + ga.y) + (ga.z + ga.w);
                    push(ga, (unsigned)el, keep_of(ga, o, h) & va & (sum == sum));
                    return;
                }
            }
            consume(p, ga, va, gb, vb);
        };
        auto advance_m = [&](const Pos p) __attribute__((always_inline)) -> Pos {
            if constexpr (kMovRot) {
                if (p.it >= n_items) return Pos{p.it + 1, 0};   // the wave's next mover pass (from n_end on: the end)
                const Pos r = advance(p);
                return (r.it >= n_items) ? Pos{n_items, 0} : r;   // behind the last static tile: mover pass 0
            } else {
                return advance(p);
            }
        };
        if constexpr (kMovRot) {
            if (wave >= PW) {
                if (p0.it >= n_items) {
                    p0 = Pos{n_items, 0};
                    ld_mov(p0, g0, v0);
                }
                if (p1.it >= n_items) {
                    p1 = Pos{max(p0.it, n_items - 1) + 1, 0};
                    ld_mov(p1, g1, v1);
                }
                if (p2.it >= n_items) {
                    p2 = Pos{max(p1.it, n_items - 1) + 1, 0};
                    ld_mov(p2, g2, v2);
                }
            }
        }
        // three tiles in flight; the slots take turns (a register rotation would have to wait for the load it moves)
        for (;;) {   // wave-uniform
            if (p0.it >= n_end) break;
            consume_m(p0, g0, v0, g0b, v0b);
            p0 = advance_m(p2);
            request_m(p0, g0, v0, g0b, v0b);
            if (p1.it >= n_end) break;
            consume_m(p1, g1, v1, g1b, v1b);
            p1 = advance_m(p0);
            request_m(p1, g1, v1, g1b, v1b);
            if (p2.it >= n_end) break;
            consume_m(p2, g2, v2, g2b, v2b);
            p2 = advance_m(p1);
            request_m(p2, g2, v2, g2b, v2b);
        }
        // MOV: the mover passes join the stage-A queue like any tile: the same cull (plus: a segment with a NaN coordinate -- the
        // documented padding of a phase -- is dropped here instead of failing every exact test), the same queues, the same exact
        // tests and atomic-min -- so the scan is that of a static map holding the static segments and this phase's tape segments
        if constexpr (MOV && !kMovRot) {
#pragma unroll
            for (int q = 0; q < kMovPasses; ++q) {
                if (!__any(m_v[q])) continue;   // wave-uniform: a front wave, a pass past the last env
                const float4 g = mg[q];
                const float2 o = sm.org[m_el[q]], h = sm.hd[m_el[q]];
                const float sum = (g.x + g.y) + (g.z + g.w);
                push(g, (unsigned)m_el[q], keep_of(g, o, h) & m_v[q] & (sum == sum));
            }
        }
        // The tail.  10 beams: stage A2 only filters, so when everything that is left fits one stage-B pass it is skipped: the
        // stage-A survivors join the stage-B queue directly (one pass of 206 VALU instead of 75 + 206; a small map never needs A2).
        // 36 beams: a pass over all beams is the expensive thing, A2 and the expansion always run.
        if (!kPairB && qtail - qhead + rtail - rhead <= 64) {
            const int n = qtail - qhead;
            if (lane < n) {
                const int s1 = (qhead + lane) & 127, s2 = (rtail + lane) & 127;
                r4[s2] = q4[s1];
                re[s2] = qe[s1];
            }
            rtail += n;
            qhead += n;
        }
        if (qtail > qhead) flushA2(qtail - qhead);
        if (rtail > rhead) {
            if constexpr (kPairB) expand(rtail - rhead);
            else flushB(rtail - rhead);
        }
    }
    __syncthreads();  // barrier B: nearest hits complete

    // ---------------- scan -> observation entries, lane = (beam, env): sanitise (environment_new.py:192-198), / 3.5 (:289),
    // and min(scan) for the collision rule (:200).  Nearest hits are uint bit patterns of non-negative floats (inf = none).
    if constexpr (POOL) {
        // lane = (column, env): the nearest of the column's `pool` consecutive rays, each through the sensor model on its own.  A -inf
        // reading wins the minimum.  (The minimum commutes with the division by 3.5: the quotient of the nearest reading.)
        for (int idx = tid; idx < NB * EPB; idx += kThreads) {
            const int c = idx / EPB, e = idx % EPB;
            if (e < nloc) {
                float mn = INFINITY;
                for (int j = 0; j < pool; ++j) {
                    const int k = (pool * c + j) * EPB + e;
                    float r = sensor_value(__uint_as_float(sm.rng[k]), sigma, (sigma > 0.f) ? sm.noise[k] : 0.f, below_min);
                    if (r == INFINITY) r = 3.5f;
                    mn = r < mn ? r : mn;
                }
                sm.obs[e * DP + c] = mn / 3.5f;
                if (mn < 0.f)
                    atomicOr(&sm.neg[e], 1u);
                else
                    atomicMin(&sm.mn_bits[e], __float_as_uint(mn));
            }
        }
    } else
    for (int idx = tid; idx < NB * EPB; idx += kThreads) {
        const int b = idx / EPB, e = idx % EPB;
        if (e < nloc) {
            float r = sensor_value(__uint_as_float(sm.rng[idx]), sigma, (sigma > 0.f) ? sm.noise[idx] : 0.f, below_min);
            if (r == INFINITY) r = 3.5f;  // :193-194 (+inf only: -inf passes through like in the reference; NaN cannot occur)
            // (float)((double)r / 3.5) == r / 3.5f : double rounding is innocuous for a quotient of
            // two float32 values (53 >= 2*24+2), so the float32 divide gives the reference's bits.
            sm.obs[e * DP + b] = r / 3.5f;
            if (SENS && r < 0.f)
                atomicOr(&sm.neg[e], 1u);
            else
                atomicMin(&sm.mn_bits[e], __float_as_uint(r));
        }
    }
    __syncthreads();  // barrier B2: lidar entries and their minima complete
    hook(wave, lane);

    // ---------------- part 3 (wave 0, lane = env): rules of getState / step / setReward + episode logic
    if (own) {
        const int e = lane;
        const int i = base + e;
        x = sm.sv_d[0][e]; y = sm.sv_d[1][e]; th = sm.sv_d[2][e]; gx = sm.sv_d[3][e]; gy = sm.sv_d[4][e];
        pdist = sm.sv_d[5][e]; dist = sm.sv_d[6][e]; ret0 = sm.sv_d[10][e];
        double path = sm.sv_d[12][e];
        act = sm.sv_act[e]; pact = sm.sv_pact[e]; ctr = sm.sv_ctr[e];
        const uint32_t step0 = sm.sv_step[e] & kStepMask;
        float* row = sm.obs + e * DP;
        const float* noise = (sigma > 0.f) ? sm.noise + e : nullptr;
        const float mn = (SENS && sm.neg[e]) ? -INFINITY : __uint_as_float(sm.mn_bits[e]);
        // row[B .. B + 5] (past action, dist / diag, yaw / 360, rel_theta / 360, diff / 180) were written in part 2
        const bool d = (0.2 > (double)mn) && ((double)mn > 0);  // environment_new.py:200
        const bool a = dist <= P.thr;                             // :204
        // setReward, :209-222
        double r = 500. * (pdist - dist);
        pdist = dist;
        if (d) r = -100.;
        if (a) r = 120.;
        bool moved_stream = false;
        if (a && P.respawn) {  // :245-267 (drawn ahead by the spec lane of record 1)
            gx = sm.sp_rg[0][e]; gy = sm.sp_rg[1][e];
            ctr = sm.sp_rctr[e];
            moved_stream = true;
            if (!P.auto_reset) pdist = hypot(gx - x, gy - y);  // with auto_reset the arrival ends the episode: pdist is re-based below
        }
        uint32_t step = step0 + 1;
        double ret = ret0 + r;
        const bool timeout = (P.max_ep_steps > 0) && ((int)step >= P.max_ep_steps);  // ppo.py:552
        const bool end = d || a || timeout;
        if constexpr (kEval) {   // main.py:206-231: the env's first `quota` episodes, one record each; later ones are only simulated
            if (end) {
                const int c = io.cnt_l[e];
                if (c < io.quota) {
                    const size_t s = (size_t)c * (size_t)P.N + (size_t)i;
                    io.rec_flags[s] = a ? 1 : (d ? 2 : 4);
                    io.rec_length[s] = (int32_t)step;
                    io.rec_return[s] = (float)ret;
                    io.rec_path[s] = (float)path;   // ppo.py:533-537: the final step's displacement is never added
                    io.cnt_l[e] = c + 1;
                }
            }
        } else {
            io.reward[row0 + i] = (float)r;
            io.done[row0 + i] = d ? 1 : 0;
            io.arrive[row0 + i] = a ? 1 : 0;
            if (io.ended) io.ended[row0 + i] = end ? 1 : 0;
            if (end) {
                if (io.ep_return) io.ep_return[row0 + i] = (float)ret;
                if (io.ep_length) io.ep_length[row0 + i] = (int32_t)step;
                if (io.ep_path_out) io.ep_path_out[row0 + i] = (float)path;   // ppo.py:533-537: the final step's displacement is never added
            }
        }
        path += sm.sv_d[11][e];
        float2 next_pact = act;  // ppo.py:543
        if (end && P.auto_reset) {  // ppo.py:582-593 + Env.reset, environment_new.py:312-382: the record read / prepared in part 2
            const int c = (a && P.respawn) ? 1 : 0;
            x = sm.sp_d[c][0][e]; y = sm.sp_d[c][1][e]; th = sm.sp_d[c][2][e]; gx = sm.sp_d[c][3][e]; gy = sm.sp_d[c][4][e];
            dist = sm.sp_d[c][5][e];
            ctr = sm.sp_ctr[c][e];
            step = 0;
            ret = 0;
            path = 0;
            moved_stream = true;
            next_pact = make_float2(0.f, 0.f);
            pdist = dist;  // getGoalDistace, :116-120,:359
            if constexpr (POOL) {
                write_lidar_pool(row, sm.sp_scan[c][e], noise, EPB, sigma, below_min, B, pool);
            } else if (SENS) {
                write_lidar(row, sm.sp_scan[c][e], 1, noise, EPB, sigma, below_min, B);
            } else {
#pragma unroll 2
                for (int b = 0; b < NB; ++b) row[b] = sm.sp_scan[c][e][b];
            }
            const float4 tl = sm.sp_tail[c][e];
            row[B + 0] = 0.f; row[B + 1] = 0.f;        // :372-373
            row[B + 2] = tl.x; row[B + 3] = tl.y; row[B + 4] = tl.z; row[B + 5] = tl.w;
        }
        // the records written or read in part 2 stay current until the env's goal stream moves
        const bool rec_ok = (P.auto_reset || P.respawn) && !moved_stream;
        const uint32_t stepw_out = step | (rec_ok ? kRecValid : 0u);
        if (PERSIST) {
            sm.st_d[0][e] = x; sm.st_d[1][e] = y; sm.st_d[2][e] = th; sm.st_d[3][e] = gx; sm.st_d[4][e] = gy;
            sm.st_d[5][e] = pdist; sm.st_d[6][e] = ret; sm.st_d[7][e] = path;
            sm.st_pact[e] = next_pact;
            sm.st_step[e] = stepw_out;
            sm.st_ctr[e] = ctr;
        }
        if (!PERSIST || last_step) {
            P.x[i] = x; P.y[i] = y; P.th[i] = th;
            P.gx[i] = gx; P.gy[i] = gy; P.past_dist[i] = pdist;
            P.past_action[i] = next_pact;
            P.ep_step[i] = (int32_t)stepw_out;
            P.ep_ret[i] = ret;
            P.ep_path[i] = path;
            P.rng_ctr[i] = ctr;
        }
    }
    __syncthreads();  // barrier C: observation tile complete in LDS

    // ---------------- coalesced store of the block's observation tile (the evaluation kernels keep it in LDS only)
    if constexpr (kEval) return;
    const int n_out = nloc * D;
    if (P.obs_f16) {
        __half* o = reinterpret_cast<__half*>(io.obs_out) + (row0 + (size_t)base) * D;
        for (int k = tid; k < n_out; k += kThreads) o[k] = __float2half_rn(sm.obs[(k / D) * DP + (k % D)]);
    } else {
        float* o = reinterpret_cast<float*>(io.obs_out) + (row0 + (size_t)base) * D;
        for (int k = tid; k < n_out; k += kThreads) o[k] = sm.obs[(k / D) * DP + (k % D)];
    }
}

// write_lidar_pool's entry for column `col` of the reset observation of record c, env e: the start pose's raw hits through this
// step's range noise, ray by ray, then the minimum
template <int NB, int EPB, int NW>
__device__ __forceinline__ float pool_reset_entry(const StepSmem<NB, EPB, NW, true>& sm, const int c, const int e, const int col,
                                                  const int pool, const float sigma, const int below_min) {
    float mn = INFINITY;
    for (int j = 0; j < pool; ++j) {
        const int k = pool * col + j;
        float r = sensor_value(sm.sp_scan[c][e][k], sigma, (sigma > 0.f) ? sm.noise[k * EPB + e] : 0.f, below_min);
        if (r == INFINITY) r = 3.5f;
        mn = r < mn ? r : mn;
    }
    return mn / 3.5f;
}

// Entries f0 .. f0 + KS - 1 of the observation env `e` (local) will hold when this step is over (entries past the row: 0), readable
// from barrier B2 on -- i.e. BEFORE the rules lane of part 3 has run: the row in sm.obs as it stands, unless the step ends the
// episode and auto_reset replaces it by the reset observation (ppo.py:582-593).  Whether it does follows from three values that are
// final at barrier B2 -- the minimum of the scan (collision, environment_new.py:200), the goal distance (arrival, :204), the step
// count (time-out, ppo.py:552) -- and the reset observation is the record the spec lanes staged in part 2.  The same expressions as
// part 3 on the same operands, so the policy that reads its input through here sees exactly the row part 3 leaves in sm.obs.
template <int NB, int EPB, int NW, bool SENS, int KS, class PRef, bool POOL = false>
__device__ __forceinline__ void next_obs_n(PRef P, const StepSmem<NB, EPB, NW, POOL>& sm, const int e, const int f0, const float sigma,
                                           const int below_min, float (&x)[KS]) {
    constexpr int D = NB + 6, DP = NB + 7;
    const float* row = sm.obs + e * DP;
#pragma unroll
    for (int j = 0; j < KS; ++j) x[j] = (f0 + j < D) ? row[min(f0 + j, D - 1)] : 0.f;
    const float mn = (SENS && sm.neg[e]) ? -INFINITY : __uint_as_float(sm.mn_bits[e]);
    const bool d = (0.2 > (double)mn) && ((double)mn > 0);                                        // environment_new.py:200
    const bool a = sm.sv_d[6][e] <= P.thr;                                                       // :204
    const uint32_t step = (sm.sv_step[e] & kStepMask) + 1;
    const bool timeout = (P.max_ep_steps > 0) && ((int)step >= P.max_ep_steps);                  // ppo.py:552
    if ((d || a || timeout) && P.auto_reset) {
        const int c = (a && P.respawn) ? 1 : 0;
        const float4 tl = sm.sp_tail[c][e];
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            const int idx = f0 + j;
            float val;
            if (idx < NB) {
                if constexpr (POOL) {
                    val = pool_reset_entry<NB, EPB, NW>(sm, c, e, min(idx, NB - 1), P.pool, sigma, below_min);
                } else {
                val = sm.sp_scan[c][e][min(idx, NB - 1)];
                if (SENS) {   // write_lidar's entry: the start pose's nearest hit through this step's range noise
                    float r = sensor_value(val, sigma, (sigma > 0.f) ? sm.noise[min(idx, NB - 1) * EPB + e] : 0.f, below_min);
                    if (r == INFINITY) r = 3.5f;
                    val = r / 3.5f;
                }
                }
            } else if (idx < NB + 2) {
                val = 0.f;                                                                       // environment_new.py:372-373
            } else if (idx < D) {
                const int q = idx - NB - 2;
                val = q == 0 ? tl.x : q == 1 ? tl.y : q == 2 ? tl.z : tl.w;
            } else {
                val = 0.f;
            }
            x[j] = val;
        }
    }
}

// The kernarg segment of step_kernel: the kernel takes this struct as its ONLY by-value parameter, so the segment IS the struct
// (members at their natural alignment, in order) and the reads through the segment pointer below cannot drift from the signature.
struct StepKArgs {
    Params P;
    StepIO io;
};
typedef const StepKArgs __attribute__((address_space(4))) * StepKArgsPtr;
static_assert(std::is_trivially_copyable<StepKArgs>::value && offsetof(StepKArgs, P) == 0 && sizeof(StepIO) == 10 * sizeof(void*),
              "kernarg mirror of step_kernel");

// Eight envs on eight waves: two workgroups per CU overlap their chains only if both fit the register file, i.e. four waves per
// SIMD -- the second launch bound caps the allocation at 128 VGPRs there (the tape kernel took 133-153 without it, one workgroup
// per CU, 4096 envs in two rounds).  Sixteen envs on eight waves carry the bound only where the instantiation needs more than 128
// VGPRs AND the rule runs it with two workgroups per CU (pick_epb, 8192-env shards): a launch per step at 10 beams without the
// 128-segment passes (131 VGPRs; house map 8192 envs 38.8 -> 25.8 us, stage_1 4096 envs 7.6 -> 7.2) and the tape form at 36 beams
// or with the 128-segment passes (131-172; 36 beams 8192 envs 13.2 -> 8.2 us per step, per-env maps 11.6 -> 6.9).  On the other
// 16-env instantiations the bound changes nothing it should (they fit) and cost 2-5 % (the scheduler's occupancy target).  0 = none.
constexpr int min_waves_per_simd(int nb, int epb, int nw, int pair, bool tape) {
    if (nw != 8) return 0;
    if (epb == 8) return 4;
    if (epb == 16) return (tape ? (nb > 16 || pair != 0) : (nb == 10 && pair == 0)) ? 4 : 0;
    return 0;
}

template <int NB, int EPB, bool SENS, int NW = 4, bool BOXES = false, int PAIR = 0>
__global__ __launch_bounds__(64 * NW, min_waves_per_simd(NB, EPB, NW, PAIR, false)) void step_kernel(StepKArgs) {
    __shared__ StepSmem<NB, EPB, NW> sm;
    __shared__ int next_env;
    // the parameter is read through the kernarg segment pointer (see step_body): scalar loads at each use
    StepKArgsPtr A = (StepKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(A));
    step_body<NB, EPB, SENS, false, NW, BOXES, PAIR, const Params __attribute__((address_space(4)))&,
              const StepIO __attribute__((address_space(4)))&>(A->P, sm, next_env, A->io);
}

// The shared-memory block of a kernel: with movers the extended one (StepSmemMov)
template <int NB, int EPB, int NW, bool MOV, bool POOL = false>
using StepSmemFor = typename std::conditional<MOV, StepSmemMov<NB, EPB, NW, POOL>, StepSmem<NB, EPB, NW, POOL>>::type;

// Movers (navsim_set_movers): every entry point takes the 16-env, 8-wave shape with 10 beams; navsim_rollout_mlp64 alone also has
// the big shapes (rollout_big_mov_kernel below).  The MOV kernels are twins of their
// own name (`*_mov_kernel`), so that the kernels a handle without a tape launches keep their symbols and their code.
// No second launch bound (min_waves_per_simd): the mover passes hold three more tiles in registers.
// They are the SENS instantiations for every handle -- with the range noise off and below_min at its default those compute the
// same bits (sensor_value with sigma = 0, mode 0) -- which halves what movers add to the build time of this file.
constexpr bool kMovSens = true;
template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void step_mov_kernel(StepKArgs) {
    constexpr bool SENS = kMovSens;
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    StepKArgsPtr A = (StepKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(A));
    step_body<10, 16, SENS, false, 8, BOXES, 0, const Params __attribute__((address_space(4)))&,
              const StepIO __attribute__((address_space(4)))&, NoHook, true>(A->P, sm, next_env, A->io);
}

// persistent kernels with movers: the phase offsets of the workgroup's envs -> LDS, once per launch
template <int NB, int EPB, int NW, class PRef, bool POOL = false>
__device__ __forceinline__ void load_mover_phase0(PRef P, StepSmemMov<NB, EPB, NW, POOL>& sm, const int base, const int nloc) {
    const int32_t* const ph0 = P.mov_phase0;
    if ((int)threadIdx.x < nloc) {
        sm.mv_phase0[threadIdx.x] = ph0 ? (uint32_t)ph0[base + threadIdx.x] : 0u;
        sm.mv_bp[threadIdx.x] = mover_bp<PRef>(P, base + (int)threadIdx.x);   // (a bank: the tape of each env)
    }
}

// ---------------------------------------------------------------- the persistent rollout kernel (PPO.rollout, ppo.py:463-641)
// All T steps of the rollout in ONE launch for the 16-64-64 policy: a workgroup owns its EPB envs for the whole rollout and
// alternates   policy phase (wave 0: PPO.get_action of mlp64_policy.h on the observation tile in LDS -> action, log-prob)
//              step phases  (step_body above: motion, cast, rules, auto-reset; the next observation tile lands in LDS)
// with workgroup barriers only: no kernel boundary, no launch ramp and no observation round trip through HBM between the
// 2 T phases.  Every row of the [T, N, .] buffers is written exactly as the per-step entry points would write it (same
// device functions, same Philox keys), so the two paths produce the same bits.
struct RolloutArgs {
    const float* params;      // actor parameters (mlp64 layout)
    void* obs_buf;            // [T + 1, N, B + 6] f32 (f16: navsim_cfg.obs_f16): row 0 = the reset observations (input), rows 1..T written here
    float* act_buf;           // [T, N, 2]
    float* logp_buf;          // [T, N]
    float* reward;            // [T, N]
    uint8_t *done, *arrive, *ended;   // [T, N]
    float* ep_return;         // [T, N], nullable
    int32_t* ep_length;       // [T, N], nullable
    float* ep_path;           // [T, N], nullable
    const float* var_ptr;     // device scalar: exploration variance
    const uint32_t* step_base;   // device scalar, nullable: rollout steps taken before this launch (noise counter)
    uint64_t seed;
    int T;
    // navsim_rollout_mlp64_hist_cont: the [N, kHistLen] history carry of row 0 (null = row 0 starts every env's episode) and where
    // to leave the carry of row T (null = nowhere); may be one buffer.  Read by the scan-history kernels alone.
    const float* hist_in;
    float* hist_out;
};

// ---- what the persistent kernels (rollout_kernel, rollout_resmlp_kernel, evaluate_kernel, evaluate_resmlp_kernel, steps_kernel,
// rollout_big_kernel) do around step_body.  A workgroup owns envs base .. base + nloc - 1; PRef as in step_body.

// The state of env i (local e) between HBM (Params) and LDS (sm.st_*): in before the first step, out after the last.
template <int NB, int EPB, int NW, class PRef, bool POOL = false>
__device__ __forceinline__ void load_state(PRef P, StepSmem<NB, EPB, NW, POOL>& sm, const int e, const int i) {
    sm.st_d[0][e] = P.x[i]; sm.st_d[1][e] = P.y[i]; sm.st_d[2][e] = P.th[i]; sm.st_d[3][e] = P.gx[i]; sm.st_d[4][e] = P.gy[i];
    sm.st_d[5][e] = P.past_dist[i]; sm.st_d[6][e] = P.ep_ret[i]; sm.st_d[7][e] = P.ep_path[i];
    sm.st_pact[e] = P.past_action[i];
    sm.st_step[e] = (uint32_t)P.ep_step[i];
    sm.st_ctr[e] = P.rng_ctr[i];
}
template <int NB, int EPB, int NW, bool POOL = false>
__device__ __forceinline__ void store_state(const Params& P, const StepSmem<NB, EPB, NW, POOL>& sm, const int e, const int i) {
    P.x[i] = sm.st_d[0][e]; P.y[i] = sm.st_d[1][e]; P.th[i] = sm.st_d[2][e]; P.gx[i] = sm.st_d[3][e]; P.gy[i] = sm.st_d[4][e];
    P.past_dist[i] = sm.st_d[5][e]; P.ep_ret[i] = sm.st_d[6][e]; P.ep_path[i] = sm.st_d[7][e];
    P.past_action[i] = sm.st_pact[e];
    P.ep_step[i] = (int32_t)sm.st_step[e];
    P.rng_ctr[i] = sm.st_ctr[e];
}

// The workgroup's rows of an [N, B + 6] observation buffer (f32; f16 if half_rows) -> the observation tile sm.obs
template <int NB, int EPB, int NW, bool POOL = false>
__device__ __forceinline__ void load_obs_tile(StepSmem<NB, EPB, NW, POOL>& sm, const void* obs, const int base, const int nloc,
                                              const bool half_rows) {
    constexpr int D = NB + 6, DP = D + 1;
    for (int k = threadIdx.x; k < nloc * D; k += 64 * NW)
        sm.obs[(k / D) * DP + (k % D)] = half_rows ? __half2float(reinterpret_cast<const __half*>(obs)[(size_t)base * D + k])
                                                   : reinterpret_cast<const float*>(obs)[(size_t)base * D + k];
}

// The beam table and the goal rejection rectangles -> LDS, once for all steps of the launch
template <int NB, int EPB, int NW, class PRef, bool POOL = false>
__device__ __forceinline__ void load_tables(PRef P, StepSmem<NB, EPB, NW, POOL>& sm) {
    const int n_beam = POOL ? 2 * NB * P.pool : 2 * NB;   // (POOL: the dense fan's table)
    for (int k = threadIdx.x; k < n_beam; k += 64 * NW) sm.beam[k] = P.beam_cs[k];
    for (int k = threadIdx.x; k < (int)(sizeof(Rects) / 8); k += 64 * NW)
        reinterpret_cast<uint64_t*>(&sm.rects)[k] = reinterpret_cast<const uint64_t*>(P.rects)[k];
}

template <int KS>
struct ObsRow {
    float x[KS];
};
// The input of lane (env e, kk) of a 16-env mlp64 policy tile: obs[e][KS kk .. KS kk + KS - 1].  IN_STEP: inside a step, behind
// barrier B2, the row the step will leave (next_obs_n), rounded as the f16 buffer holds it; else the row in sm.obs (policy_row).
// An absent env (e >= nloc) feeds zeros.  (Returned by value: with the row as an output argument instead, rollout_kernel<10, 4 | 8,
// false, 8> took 169 VGPRs, one SIMD occupancy step below the 167 of the row written out in the kernel.)
template <int NB, int EPB, int NW, bool SENS, bool IN_STEP, class PRef, bool POOL = false>
__device__ __forceinline__ ObsRow<mlp64::Layout<NB + 6>::KS> mlp64_obs_row(PRef P, const StepSmem<NB, EPB, NW, POOL>& sm, const int e,
                                                                        const int kk, const int nloc, const bool half_rows,
                                                                        const float sigma, const int below_min) {
    using PL = mlp64::Layout<NB + 6>;
    constexpr int KS = PL::KS, DP = NB + 7;
    const bool valid = e < nloc;
    ObsRow<KS> r;
    float (&xs)[KS] = r.x;
    if constexpr (IN_STEP) {
        next_obs_n<NB, EPB, NW, SENS, KS, PRef>(P, sm, min(e, nloc - 1), KS * kk, sigma, below_min, xs);
        if (half_rows) {
#pragma unroll
            for (int j = 0; j < KS; ++j) xs[j] = __half2float(__float2half_rn(xs[j]));
        }
    } else {
        mlp64::policy_row<PL>(sm.obs + min(e, nloc - 1) * DP, kk, half_rows, xs);
    }
    if (!valid) {
#pragma unroll
        for (int j = 0; j < KS; ++j) xs[j] = 0.f;
    }
    return r;
}

// ---- scan history (navsim_rollout_mlp64_hist / navsim_evaluate_mlp64_hist): the 42-column row of navsim_stack_rows, assembled on
// chip.  Per env the workgroup keeps kHistLen = 22 floats in LDS: the scan of the previous row [0..9], the scan of the row before it
// [10..19] and the previous row's past_action [20..21] -- in that order they ARE columns 16..37 of a row that does not start an episode
// -- each clamped to the episode's first row (the cut) and, with float16 rows, rounded as the buffer holds it.  Row stride 23: odd.
constexpr int kHistLen = 22, kHistStride = 23, kHistD = 42;
// the column of the CURRENT 16-column row that column f (16..37) of the stacked row copies when the row starts an episode
__device__ __forceinline__ int hist_src_col(const int f) { return f < 26 ? f - 16 : f - 26; }

// Whether step t ends env e's episode, from the three values that are final at barrier B2: the predicate under which part 3 of
// step_body writes `ended` (d || a || timeout there; next_obs_n evaluates the same three).
template <int NB, int EPB, int NW, bool SENS, class PRef, bool POOL = false>
__device__ __forceinline__ bool hist_step_ends(PRef P, const StepSmem<NB, EPB, NW, POOL>& sm, const int e) {
    const float mn = (SENS && sm.neg[e]) ? -INFINITY : __uint_as_float(sm.mn_bits[e]);
    const bool d = (0.2 > (double)mn) && ((double)mn > 0);                                        // environment_new.py:200
    const bool a = sm.sv_d[6][e] <= P.thr;                                                       // :204
    const uint32_t step = (sm.sv_step[e] & kStepMask) + 1;
    const bool timeout = (P.max_ep_steps > 0) && ((int)step >= P.max_ep_steps);                  // ppo.py:552
    return d || a || timeout;
}
// Entry idx (0..11: the scan and past_action) of the row the step will leave for env e, behind barrier B2: next_obs_n's value for
// one run-time column (`ends`: hist_step_ends).  With auto_reset the reset observation's entry -- its scan through THIS step's range
// noise under SENS, past_action 0 -- else the row in sm.obs (which part 3 then leaves alone).
template <int NB, int EPB, int NW, bool SENS, class PRef, bool POOL = false>
__device__ __forceinline__ float hist_next_entry(PRef P, const StepSmem<NB, EPB, NW, POOL>& sm, const int e, const int idx, const bool ends,
                                                 const float sigma, const int below_min) {
    constexpr int DP = NB + 7;
    if (!(ends && P.auto_reset)) return sm.obs[e * DP + idx];
    if (idx >= NB) return 0.f;                                                                   // environment_new.py:372-373
    const int c = ((sm.sv_d[6][e] <= P.thr) && P.respawn) ? 1 : 0;
    if constexpr (POOL) return pool_reset_entry<NB, EPB, NW>(sm, c, e, idx, P.pool, sigma, below_min);
    float val = sm.sp_scan[c][e][idx];
    if (SENS) {
        float r = sensor_value(val, sigma, (sigma > 0.f) ? sm.noise[idx * EPB + e] : 0.f, below_min);
        if (r == INFINITY) r = 3.5f;
        val = r / 3.5f;
    }
    return val;
}
// The input of lane (env e, kk) of the 42-column policy tile: columns 11 kk .. 11 kk + 10 of the stacked row (44 padded features).
// Columns 0..15 are mlp64_obs_row's of the 16-column policy (next_obs_n / sm.obs); columns 16..37 come from `hist`, or -- on a row
// behind an ended step -- are copies of the row's own scan and past_action; 38..43 are 0.  Row 0 of the launch (!IN_STEP) reads
// `hist` as it was filled: by hist_init with those same copies (the row starts an episode), or from the caller's carry.  Every value rounded to half when the buffers are (idempotent on what hist already holds).
template <int NB, int EPB, int NW, bool SENS, bool IN_STEP, class PRef, bool POOL = false>
__device__ __forceinline__ ObsRow<11> hist_obs_row(PRef P, const StepSmem<NB, EPB, NW, POOL>& sm, const float* hist, const int e, const int kk,
                                                   const int nloc, const bool half_rows, const float sigma, const int below_min) {
    static_assert(NB == 10, "the history row stacks 10-beam scans");
    constexpr int KS = 11, D = NB + 6, DP = NB + 7;
    const bool valid = e < nloc;
    const int el = min(e, nloc - 1);
    ObsRow<KS> r;
    float (&xs)[KS] = r.x;
    bool ends = false;
    if constexpr (IN_STEP) {
        next_obs_n<NB, EPB, NW, SENS, KS, PRef>(P, sm, el, KS * kk, sigma, below_min, xs);   // (columns past 15: 0)
        ends = hist_step_ends<NB, EPB, NW, SENS, PRef>(P, sm, el);
    } else {
#pragma unroll
        for (int j = 0; j < KS; ++j) xs[j] = (KS * kk + j < D) ? sm.obs[el * DP + min(KS * kk + j, D - 1)] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
        const int f = KS * kk + j;
        if (f >= D && f < D + kHistLen) {
            float v = 0.f;
            if (ends) {
                if constexpr (IN_STEP) v = hist_next_entry<NB, EPB, NW, SENS, PRef>(P, sm, el, hist_src_col(f), true, sigma, below_min);
            } else {
                v = hist[el * kHistStride + (f - D)];
            }
            xs[j] = v;
        }
    }
    if (half_rows) {
#pragma unroll
        for (int j = 0; j < KS; ++j) xs[j] = __half2float(__float2half_rn(xs[j]));
    }
    if (!valid) {
#pragma unroll
        for (int j = 0; j < KS; ++j) xs[j] = 0.f;
    }
    return r;
}
// The history of the launch's row 0, straight from the observation buffer (before the first step overwrites the tile): both older
// frames are row 0's scan, the older action its past_action.
template <int NB, int NW>
__device__ __forceinline__ void hist_init(float* hist, const void* obs, const int base, const int nloc, const bool half_rows) {
    constexpr int D = NB + 6;
    for (int k = threadIdx.x; k < nloc * kHistLen; k += 64 * NW) {
        const int e = k / kHistLen, c = k % kHistLen;
        const size_t src = (size_t)(base + e) * D + (size_t)hist_src_col(D + c);
        hist[e * kHistStride + c] = half_rows ? __half2float(reinterpret_cast<const __half*>(obs)[src])
                                              : reinterpret_cast<const float*>(obs)[src];
    }
}
// Between the steps `hist` is one row ahead of a history row's columns: in front of step t it holds (scan of row t, scan of row
// t - 1, past_action of row t) -- what row t + 1 reads unless step t ends the episode -- while columns 16..37 of row t, the CARRY of
// row t (include/navsim.h), are (scan of row t - 1, scan of row t - 2, past_action of row t - 1).  So a launch that continues from a
// caller's carry ([N, kHistLen] f32) fills `hist` with the carry itself, which the policy of row 0 reads as its columns 16..37
// (hist_obs_row, !IN_STEP), and then moves it one row on (hist_enter); the episode cut is inside the carry's values, so nothing
// here asks whether row 0 starts an episode.
template <int NW>
__device__ __forceinline__ void hist_load(float* hist, const float* carry, const int base, const int nloc) {
    for (int k = threadIdx.x; k < nloc * kHistLen; k += 64 * NW)
        hist[(k / kHistLen) * kHistStride + (k % kHistLen)] = carry[(size_t)base * kHistLen + k];
}
// lane = env e, behind the policy of row 0 and in front of step 0: the carry of row 0 -> the block in front of step 0.  Row 0's own
// scan and past_action come from the observation tile (float16 rows: the half values, as load_obs_tile widened them).
template <int NB, int EPB, int NW, bool POOL = false>
__device__ __forceinline__ void hist_enter(const StepSmem<NB, EPB, NW, POOL>& sm, float* hist, const int e) {
    constexpr int DP = NB + 7;
    float* h = hist + e * kHistStride;
    for (int c = 0; c < NB; ++c) {
        h[NB + c] = h[c];
        h[c] = sm.obs[e * DP + c];
    }
    h[2 * NB] = sm.obs[e * DP + NB];
    h[2 * NB + 1] = sm.obs[e * DP + NB + 1];
}
// lane = env e, behind the launch's LAST step (no policy ran in it: the block is as the shift of the step before left it; the
// observation tile holds the row the step left, the reset observation where it ended an episode): the carry of that row.  The
// block IS its columns 16..37 unless the step ended the episode (`ended`: the flag this lane stored for the step); then they are
// copies of the new row's own scan and past_action.  8 bytes per store (rows of 88 bytes in a 16-byte aligned buffer).
template <int NB, int EPB, int NW, bool POOL = false>
__device__ __forceinline__ void hist_leave(const StepSmem<NB, EPB, NW, POOL>& sm, float* hist, float* carry, const int base, const int e,
                                           const bool ended, const bool half_rows) {
    constexpr int DP = NB + 7;
    float* h = hist + e * kHistStride;
    if (ended) {
        for (int c = 0; c < NB + 2; ++c) {
            float v = sm.obs[e * DP + c];
            if (half_rows) v = __half2float(__float2half_rn(v));
            if (c < NB) h[c] = v;
            h[NB + c] = v;
        }
    }
    float2* o = reinterpret_cast<float2*>(carry + (size_t)(base + e) * kHistLen);
#pragma unroll
    for (int c = 0; c < kHistLen / 2; ++c) o[c] = make_float2(h[2 * c], h[2 * c + 1]);
}
// The shift, lane = env, by the wave that arrives last at the in-step policy (last_arrival: the four tile waves have read `hist`,
// and the next read is behind barrier B2 of the next step, which no wave reaches before this wave has passed barrier C):
// the row the step leaves becomes the previous row.  On a row that starts an episode both frames become its scan.
template <int NB, int EPB, int NW, bool SENS, class PRef, bool POOL = false>
__device__ __forceinline__ void hist_shift(PRef P, const StepSmem<NB, EPB, NW, POOL>& sm, float* hist, const int e, const bool half_rows,
                                           const float sigma, const int below_min) {
    const bool ends = hist_step_ends<NB, EPB, NW, SENS, PRef>(P, sm, e);
    float* h = hist + e * kHistStride;
    for (int c = 0; c < NB + 2; ++c) {
        float v = hist_next_entry<NB, EPB, NW, SENS, PRef>(P, sm, e, c, ends, sigma, below_min);
        if (half_rows) v = __half2float(__float2half_rn(v));
        if (c < NB) {
            h[NB + c] = ends ? v : h[c];
            h[c] = v;
        } else {
            h[NB + c] = v;   // [20..21]
        }
    }
}

// Each of K waves calls this once its part of a phase is in LDS; the wave that arrives last resets the counter for the next phase
// and runs finish(): an LDS counter -- a wave's LDS operations are performed in order, so the one that reads K - 1 sees what the
// other waves wrote.
template <unsigned K, class Finish>
__device__ __forceinline__ void last_arrival(unsigned& cnt, const int lane, Finish finish) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    unsigned old = 0u;
    if (lane == 0) old = atomicAdd(&cnt, 1u);
    if (__builtin_amdgcn_readfirstlane(old) == K - 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (lane == 0) cnt = 0u;
        finish();
    }
}

// The resmlp512 policy step (resmlp_policy.h) on the observation tile in LDS, all eight waves, up to the pre-activations z3, z4 of
// the two output units (valid on wave 0: lane (env lane & 15, q = 0)).  Lane (env l15, q) feeds obs[l15][4 q .. 4 q + 3].
template <int NB, int EPB, int NW>
__device__ __forceinline__ void resmlp_preact(const float* params, const StepSmem<NB, EPB, NW>& sm, const resmlp::Block1Smem& bs,
                                              resmlp::PolicySmem& ps, const int lane, const int wave, const int nloc,
                                              const bool half_rows, float& z3, float& z4) {
    constexpr int DP = NB + 7;
    const int l15 = lane & 15, q = lane >> 4;
    resmlp::f32x4 xq = resmlp::zero4();
    if (l15 < nloc) {
        const float* row = sm.obs + l15 * DP + 4 * q;
        xq = resmlp::f32x4{row[0], row[1], row[2], row[3]};
        if (half_rows) {   // (the tile in LDS is float32; the row in the buffer -- what navppo_resmlp512_act would read -- is its rounding to half)
#pragma unroll
            for (int j = 0; j < 4; ++j) xq[j] = __half2float(__float2half_rn(xq[j]));
        }
    }
    resmlp::Weights W;
    resmlp::load_weights_b(params, lane, wave, W);   // requested first: in flight while block 1 runs out of LDS
    resmlp::load_weights_a_lds(bs, lane, wave, W);
    resmlp::policy_preact_w(W, bs.b2a, bs.tail, xq, lane, wave, ps, z3, z4);
}

// The I/O of rollout step t (tn = t N): row t + 1 of the [T + 1, N, D] observation buffer (f16 if half_rows), row t of the [T, N]
// buffers (the statistics nullable).  rollout_big_kernel takes the one of step 0 and reaches row t through step_body's row0.
__host__ __device__ __forceinline__ StepIO rollout_io(const RolloutArgs& R, const size_t N, const size_t D, const size_t tn,
                                                      const bool half_rows) {
    void* const obs_row = half_rows ? (void*)(reinterpret_cast<__half*>(R.obs_buf) + (tn + N) * D)
                                    : (void*)(reinterpret_cast<float*>(R.obs_buf) + (tn + N) * D);
    return StepIO{nullptr, nullptr, obs_row, R.reward + tn, R.done + tn, R.arrive + tn, R.ended + tn,
                  R.ep_return ? R.ep_return + tn : nullptr, R.ep_length ? R.ep_length + tn : nullptr,
                  R.ep_path ? R.ep_path + tn : nullptr};
}

// (A persistent kernel and its *_mov_kernel twin share one body function; each declares its own LDS variables, under the names
// they had, and hands them to the body.  What the move into a body function did to the kernels without movers -- one or two VGPRs in
// twelve instantiations, nothing else -- is listed in profiles/movers_kernel_resources.txt.)
// HIST (navsim_rollout_mlp64_hist): the policy is the 42-64-64 one on the stacked row of the last three 10-beam scans (hist_obs_row;
// `hist`: the workgroup's [16][kHistStride] LDS block); the env side and every buffer are those of the 16-column form.  Off, nothing
// of it is compiled.
template <int NB, int EPB, bool SENS, int NW, bool BOXES, bool MOV, bool HIST = false, bool POOL = false>   // POOL: as in step_body
__device__ __forceinline__ void rollout_body(const Params& P, const RolloutArgs& R, StepSmemFor<NB, EPB, NW, MOV, POOL>& sm, int& next_env,
                                             float* const wts, float2 (&pol_z)[4][16], float2 (&pol_eps)[16], unsigned& pol_cnt,
                                             [[maybe_unused]] float* const hist = nullptr) {
    constexpr int D = NB + 6, kThreads = 64 * NW;
    static_assert(!HIST || (NB == 10 && EPB == 16), "scan history: 16 envs, 10 beams");
    using PL = mlp64::Layout<HIST ? kHistD : D>;   // the (B + 6)-64-64 policy: 16-wide rows with 10 beams, 42-wide with 36 (HIST: 42-wide on 10)
    constexpr int KS = PL::KS;
    static_assert(NW >= 6 && EPB <= 16, "policy phase: four tile waves + the noise wave beside wave 0's rules; one 16-env policy tile per workgroup");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int base = blockIdx.x * EPB;
    const int nloc = min(EPB, P.N - base);
    const size_t N = (size_t)P.N;
    for (int k = tid; k < PL::P_ACTOR; k += kThreads) wts[k] = R.params[k];
    if (tid < nloc) load_state<NB, EPB, NW, const Params&>(P, sm, tid, base + tid);   // the envs' state for the whole rollout
    const bool half_rows = P.obs_f16 != 0;   // float16 observation buffers: the policy reads what a reader of the buffers would
    load_obs_tile<NB, EPB, NW>(sm, R.obs_buf, base, nloc, half_rows);
    load_tables<NB, EPB, NW, const Params&>(P, sm);
    if constexpr (MOV) load_mover_phase0<NB, EPB, NW, const Params&>(P, sm, base, nloc);
    if constexpr (HIST) {
        if (R.hist_in) hist_load<NW>(hist, R.hist_in, base, nloc);
        else hist_init<NB, NW>(hist, R.obs_buf, base, nloc, half_rows);
    }
    const uint32_t step0 = R.step_base ? *R.step_base : 0u;
    const float var = *R.var_ptr;
    if (tid == 0) pol_cnt = 0u;
    __syncthreads();
    // The policy (mlp64_policy.h) as the kernel runs it: four "tile waves" each compute layer 1 and one 16-row tile of layer 2 with
    // its share of the two output units (tile_part), one wave draws the step's action noise meanwhile, and -- behind a barrier --
    // wave 0 finishes (sigmoid / tanh, clamp, log-prob) and publishes the action (finish).
    const float sigma = SENS ? P.sigma : 0.f;
    const int below_min = SENS ? P.below_min_mode : 0;
    auto tile_part = [&](const int t2, auto in_step) __attribute__((always_inline)) {
        const int e = lane & 15, kk = lane >> 4;
        if constexpr (HIST) {
            const auto row = hist_obs_row<NB, EPB, NW, SENS, decltype(in_step)::value, const Params&>(P, sm, hist, e, kk, nloc,
                                                                                                    half_rows, sigma, below_min);
            const float (&xs)[KS] = row.x;
            mlp64::f32x4 c1[4];
            mlp64::policy_hidden1<PL>(wts, xs, lane, c1);
            float pz3, pz4;
            mlp64::policy_tile2<PL>(wts, c1, lane, t2, pz3, pz4);
            if (kk == 0) pol_z[t2][e] = make_float2(pz3, pz4);
        } else {
        const auto row = mlp64_obs_row<NB, EPB, NW, SENS, decltype(in_step)::value, const Params&>(P, sm, e, kk, nloc, half_rows,
                                                                                                 sigma, below_min);
        const float (&xs)[KS] = row.x;
        mlp64::f32x4 c1[4];
        mlp64::policy_hidden1<PL>(wts, xs, lane, c1);
        float pz3, pz4;
        mlp64::policy_tile2<PL>(wts, c1, lane, t2, pz3, pz4);
        if (kk == 0) pol_z[t2][e] = make_float2(pz3, pz4);
        }
    };
    auto draw_noise = [&](const uint32_t step) __attribute__((always_inline)) {
        float e0, e1;
        mlp64::policy_noise(step, R.seed, P.env_id_base + (uint64_t)(base + lane), e0, e1);
        pol_eps[lane] = make_float2(e0, e1);
    };
    const float sd = sqrtf(var), log_var = logf(var);   // policy_finish's sqrtf(var) / logf(var), once per launch: same bits
    auto finish = [&](const size_t tn) __attribute__((always_inline)) {   // any wave, lane = env: row tn / N of act_buf / logp_buf
        const int e = lane;
        const float pz3[4] = {pol_z[0][e].x, pol_z[1][e].x, pol_z[2][e].x, pol_z[3][e].x};
        const float pz4[4] = {pol_z[0][e].y, pol_z[1][e].y, pol_z[2][e].y, pol_z[3][e].y};
        const float2 eps = pol_eps[e];
        const mlp64::PolicyOut o = mlp64::policy_finish_pre<PL>(wts, pz3, pz4, var, sd, log_var, eps.x, eps.y);
        sm.act_l[e] = make_float2(o.a0, o.a1);
        reinterpret_cast<float2*>(R.act_buf)[tn + base + e] = make_float2(o.a0, o.a1);
        R.logp_buf[tn + base + e] = o.logp;
    };
    // the action of step 0, from the reset observations
    if (wave < 4) tile_part(wave, std::false_type{});
    else if (wave == 4 && lane < nloc) draw_noise(step0);
    __syncthreads();
    if (wave == 0 && lane < nloc) finish(0);
    if constexpr (HIST) {   // (the tile waves have read the carry as row 0's columns: now the block in front of step 0)
        if (wave == 1 && lane < nloc && R.hist_in) hist_enter<NB, EPB, NW>(sm, hist, lane);
    }
    __syncthreads();
    for (int t = 0; t < R.T; ++t) {
        const size_t tn = (size_t)t * N;
        asm volatile("" ::: "memory");   // keeps the weight reads of the policy phase inside the loop (registers are scarce)
        const StepIO io = rollout_io(R, N, D, tn, half_rows);
        // The policy of step t + 1 runs INSIDE step t, behind barrier B2.  Wave 0 works through the rules there (a float64 latency
        // chain, 0.85 us) and every other wave would only wait for it at barrier C; instead waves 1-4 run the tile parts, wave 5
        // draws the noise, and whichever of the five arrives last (last_arrival) finishes and publishes the action -- all before
        // barrier C, so the next step starts right behind this one.  What the rules still have to decide about the observation tile --
        // whether an env's row is replaced by its reset observation -- the tile waves work out themselves from the values that
        // are final at B2 (next_obs_n), so they read exactly the rows the step leaves: same device functions on the same inputs,
        // the buffers keep their bits.  Round 3 ran the phase between the steps with the whole workgroup waiting (5.2 us per
        // step); stamps of this form in profiles/r04_rollout16_phase_stamps.txt.
        const bool more = t + 1 < R.T;
        auto hook = [&](const int wv, const int ln) __attribute__((always_inline)) {
            // (measured: the parts on waves 1, 2, 3, 5 -- keeping them off wave 0's SIMD if waves land round robin -- 5.34 instead
            // of 5.01 us per step)
            if (more && wv >= 1 && wv <= 5) {
                if (wv <= 4) tile_part(wv - 1, std::true_type{});
                else if (ln < nloc) draw_noise(step0 + (uint32_t)(t + 1));
                last_arrival<5>(pol_cnt, ln, [&]() __attribute__((always_inline)) {
                    if (ln < nloc) finish(tn + N);
                    if constexpr (HIST) {
                        if (ln < nloc) hist_shift<NB, EPB, NW, SENS, const Params&>(P, sm, hist, ln, half_rows, sigma, below_min);
                    }
                });
            }
        };
        step_body<NB, EPB, SENS, true, NW, BOXES, 0, const Params&, const StepIO&, decltype(hook), MOV, POOL>(P, sm, next_env, io,
                                                                                                            t == R.T - 1, 0, hook);
        // the observation tile of step t + 1 is in sm.obs (its store only reads it), its action in sm.act_l
    }
    if constexpr (HIST) {   // the carry of row T, by the lanes that wrote the last step's flags (wave 0, lane = env)
        if (R.hist_out && wave == 0 && lane < nloc)
            hist_leave<NB, EPB, NW>(sm, hist, R.hist_out, base, lane, R.ended[(size_t)(R.T - 1) * N + base + lane] != 0, half_rows);
    }
}
template <int NB, int EPB, bool SENS, int NW, bool BOXES = false>
__global__ __launch_bounds__(64 * NW) void rollout_kernel(Params P, RolloutArgs R) {
    using PL = mlp64::Layout<NB + 6>;
    __shared__ StepSmem<NB, EPB, NW> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];   // the actor, staged once for all T steps
    __shared__ float2 pol_z[4][16];   // policy phase: per-tile partial sums of the two output units
    __shared__ float2 pol_eps[16];    // ... and the step's action noise
    __shared__ unsigned pol_cnt;      // arrivals of the in-step policy's five waves (the last one finishes)
    rollout_body<NB, EPB, SENS, NW, BOXES, false>(P, R, sm, next_env, wts, pol_z, pol_eps, pol_cnt);
}
template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void rollout_mov_kernel(Params P, RolloutArgs R) {
    using PL = mlp64::Layout<16>;
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ float2 pol_eps[16];
    __shared__ unsigned pol_cnt;
    rollout_body<10, 16, kMovSens, 8, BOXES, true>(P, R, sm, next_env, wts, pol_z, pol_eps, pol_cnt);
}

// The scan-history twins (navsim_rollout_mlp64_hist): 16 envs on 8 waves, 10 beams, the 42-64-64 actor staged in LDS.  Kernels of
// their own names, so that what a rollout without history launches keeps its symbols and its code.
template <bool SENS, bool BOXES>
__global__ __launch_bounds__(64 * 8) void rollout_hist_kernel(Params P, RolloutArgs R) {
    using PL = mlp64::Layout<kHistD>;
    __shared__ StepSmem<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ float2 pol_eps[16];
    __shared__ unsigned pol_cnt;
    __shared__ float hist[16 * kHistStride];   // the two older scans and the older action pair of the workgroup's envs
    rollout_body<10, 16, SENS, 8, BOXES, false, true>(P, R, sm, next_env, wts, pol_z, pol_eps, pol_cnt, hist);
}
template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void rollout_hist_mov_kernel(Params P, RolloutArgs R) {
    using PL = mlp64::Layout<kHistD>;
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ float2 pol_eps[16];
    __shared__ unsigned pol_cnt;
    __shared__ float hist[16 * kHistStride];
    rollout_body<10, 16, kMovSens, 8, BOXES, true, true>(P, R, sm, next_env, wts, pol_z, pol_eps, pol_cnt, hist);
}

// ---------------------------------------------------------------- the persistent rollout for the reference's ACTIVE actor
// PPO.rollout (ppo.py:463-641) with NetActor (net_actor.py:56-144: two residual blocks of 512 hidden units) choosing every action
// in the kernel: rollout_kernel's workgroup (16 envs on 8 waves, env state and observation tile in LDS for all T steps) with the
// policy step of csrc/resmlp_policy.h -- the one navppo_resmlp512_act launches per step -- in front of every env step: all eight
// waves (each owns 64 hidden units), two workgroup sums, wave 0 finishes (clamp, log-prob of the clamped action); the Philox /
// Box-Muller noise of step t + 1 is drawn inside step t (wave 5, behind barrier B2, where it would only wait for the rules).
// Same device functions and Philox keys as the per-step entry points: every row of the [T, N, .] buffers keeps its bits.
//
// Where the weights live decides the time.  A CU pulls L2 hits at ~37 GB/s (measured here: 197 KB in 5 us, the same with 64 and
// with 256 workgroups -- outstanding misses x latency, not a shared limit), so the 197 KB of weights streamed per step were the
// longest phase of the first version.  Block 1 (66 KB) and the 114 small tail parameters now stay in LDS for the whole launch
// (145 KB per workgroup with the step body's 79 KB: one workgroup per CU); block 2 (130 KB) still streams, requested first so
// that it is in flight while block 1 runs.  Per 512-step rollout at 4096 envs: 9.1 ms as a hipGraph of 512 x (policy launch +
// step launch), 6.4 ms persistent with everything streamed, 5.9 ms now (bench.py resmlp512.rollout_ms).  Requesting the
// weights a phase early, inside the env step, was measured and is not done: the 128 registers per lane do not fit beside the
// step body (24-58 spilled VGPRs, 6.9-7.4 ms).  The phases of one step (tools/resmlp_rollout_phases.py; profiles/
// r05_rollout_resmlp_phases.txt): block 1 2.1 us, sum 1.9 (it waits for block 2's weights), block 2 2.3 (the f32 MFMA floor of
// both blocks on one CU is 2.6), sum + finish 1.3, env step 4.0.
template <bool SENS, bool MOV>
__device__ __forceinline__ void rollout_resmlp_body(const Params& P, const RolloutArgs& R, StepSmemFor<10, 16, 8, MOV>& sm, int& next_env,
                                                    resmlp::PolicySmem& ps, resmlp::Block1Smem& bs, float2 (&pol_eps)[16]) {
    constexpr int NB = 10, EPB = 16, NW = 8, D = NB + 6;
    static_assert(D == resmlp::rp::D && EPB == resmlp::kPolEnvs && NW == resmlp::kPolWaves, "the policy step's workgroup");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int base = blockIdx.x * EPB;
    const int nloc = min(EPB, P.N - base);
    const size_t N = (size_t)P.N;
    if (tid < nloc) load_state<NB, EPB, NW, const Params&>(P, sm, tid, base + tid);   // the envs' state for the whole rollout
    const bool half_rows = P.obs_f16 != 0;   // float16 observation buffers (BASELINE configs[4]): the policy reads what a reader of the buffers would
    load_obs_tile<NB, EPB, NW>(sm, R.obs_buf, base, nloc, half_rows);
    load_tables<NB, EPB, NW, const Params&>(P, sm);
    if constexpr (MOV) load_mover_phase0<NB, EPB, NW, const Params&>(P, sm, base, nloc);
    const uint32_t step0 = R.step_base ? *R.step_base : 0u;
    const float var = *R.var_ptr;
    const int l15 = lane & 15, q = lane >> 4;
    const bool valid = l15 < nloc;
    auto draw_noise = [&](const uint32_t step) __attribute__((always_inline)) {   // lane = env
        float e0, e1;
        mlp64::policy_noise(step, R.seed, P.env_id_base + (uint64_t)(base + lane), e0, e1);
        pol_eps[lane] = make_float2(e0, e1);
    };
    // The weights of a policy step (this wave's 64 hidden units: 128 registers) are REQUESTED inside the env step in front of it --
    // behind barrier B2, where every wave but wave 0 only waits for the rules -- and arrive during the step's tail: the L2 round
    // trip of 197 KB per workgroup and step is off the critical path.  (They cannot simply stay in registers: the step body needs them.)
    resmlp::stage_block1(R.params, lane, wave, bs);
    if (wave == 5 && lane < nloc) draw_noise(step0);
    __syncthreads();
    for (int t = 0; t < R.T; ++t) {
        const size_t tn = (size_t)t * N;
        // ---- PPO.get_action (ppo.py:673-706) on the observation tile the previous step (or the reset) left in LDS
        float z3, z4;
        resmlp_preact<NB, EPB, NW>(R.params, sm, bs, ps, lane, wave, nloc, half_rows, z3, z4);
        if (wave == 0 && q == 0 && valid) {
            const float2 eps = pol_eps[l15];
            const resmlp::Action o = resmlp::policy_finish(bs.tail, z3, z4, var, eps.x, eps.y);
            sm.act_l[l15] = make_float2(o.a0, o.a1);
            reinterpret_cast<float2*>(R.act_buf)[tn + base + l15] = make_float2(o.a0, o.a1);
            R.logp_buf[tn + base + l15] = o.logp;
        }
        __syncthreads();
        // ---- the env step: the same step body as every other entry point; behind its barrier B2 the next policy step's weights are
        // requested and its noise is drawn
        const StepIO io = rollout_io(R, N, D, tn, half_rows);
        const bool more = t + 1 < R.T;
        auto hook = [&](const int wv, const int ln) __attribute__((always_inline)) {
            if (more) {
                if (wv == 5 && ln < nloc) draw_noise(step0 + (uint32_t)(t + 1));
            }
        };
        step_body<NB, EPB, SENS, true, NW, false, 0, const Params&, const StepIO&, decltype(hook), MOV>(P, sm, next_env, io, t == R.T - 1, 0, hook);
        __syncthreads();   // the observation tile of step t + 1 is complete in sm.obs (the tile store only reads it)
    }
}
template <bool SENS>
__global__ __launch_bounds__(64 * 8) void rollout_resmlp_kernel(Params P, RolloutArgs R) {
    constexpr int NB = 10, EPB = 16, NW = 8;
    __shared__ StepSmem<NB, EPB, NW> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) resmlp::PolicySmem ps;
    __shared__ __attribute__((aligned(16))) resmlp::Block1Smem bs;   // block 1's weights + the small tail of the parameters
    __shared__ float2 pol_eps[EPB];   // the action noise of the next policy step (drawn inside the env step in front of it)
    rollout_resmlp_body<SENS, false>(P, R, sm, next_env, ps, bs, pol_eps);
}
#ifndef NAVSIM_POOL_TU   // (a kernel that is no template: not compiled a second time in the sector-LiDAR twins' translation unit)
__global__ __launch_bounds__(64 * 8) void rollout_resmlp_mov_kernel(Params P, RolloutArgs R) {
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) resmlp::PolicySmem ps;
    __shared__ __attribute__((aligned(16))) resmlp::Block1Smem bs;
    __shared__ float2 pol_eps[16];
    rollout_resmlp_body<kMovSens, true>(P, R, sm, next_env, ps, bs, pol_eps);
}
#endif   // NAVSIM_POOL_TU

// ---------------------------------------------------------------- the evaluation form of the two persistent rollouts
// main.evaluate (main.py:135-252) in ONE launch: rollout_kernel's / rollout_resmlp_kernel's workgroup (16 envs on 8 waves, env
// state and observation tile in LDS) with
//   - the deterministic action a = (clamp(mu0, 0, 1), clamp(mu1, -1, 1)) (main.py:197-199): no Philox draw, no Box-Muller, no
//     log-prob, no noise wave and no pol_eps exchange;
//   - no [T, N, .] rows at all: the only global stores of a step are an episode record (EvalIO, written by the env's rules lane)
//     when an episode ends and the env's count is still below the quota -- later episodes are simulated but not recorded;
//   - an early exit: behind barrier C of every step each wave reads the 16 counts from LDS and the workgroup leaves the loop once
//     every env has met the quota (absent envs of a tail workgroup start at the quota).  The counts are written by wave 0 in
//     front of barrier C and not again before barriers A / B / B2 of the next step, which no wave passes before every wave has
//     read them: all waves of a workgroup see the same 16 values and take the same branch.  The loop is bounded by n_steps.
// Same device functions on the same inputs as the per-step entry points (navppo_*_act with zero noise + navsim_step): the table
// keeps their bits.  The env state goes back to HBM after the loop (the envs ran on past their quota: callers reset before reuse).
struct EvalArgs {
    const float* params;      // actor parameters (mlp64 / resmlp512 layout)
    const void* obs0;         // [N, B + 6] f32 (f16: navsim_cfg.obs_f16): the reset observations
    uint8_t* ep_flags;        // [quota, N]
    int32_t* ep_length;       // [quota, N]
    float* ep_return;         // [quota, N]
    float* ep_path;           // [quota, N]
    int32_t* count;           // [N]
    int32_t* steps;           // [ceil(N / 16)]
    int quota;
    int T;
};

// the episode table of a launch, counted in cnt_l (LDS)
__device__ __forceinline__ EvalIO eval_io(const EvalArgs& R, int* cnt_l) {
    return EvalIO{StepIO{}, cnt_l, R.quota, R.ep_flags, R.ep_length, R.ep_return, R.ep_path};
}
// behind a barrier that follows the rules lanes' count updates: true on every wave of the workgroup, or on none
template <int EPB>
__device__ __forceinline__ bool eval_quota_met(const int* ep_cnt, const int lane, const int quota) {
    return __builtin_amdgcn_ballot_w64(ep_cnt[lane & (EPB - 1)] < quota) == 0ull;
}

template <int NB, bool SENS, bool BOXES, bool MOV, bool HIST = false, bool POOL = false>   // HIST: as in rollout_body (navsim_evaluate_mlp64_hist)
__device__ __forceinline__ void evaluate_body(const Params& P, const EvalArgs& R, StepSmemFor<NB, 16, 8, MOV, POOL>& sm, int& next_env,
                                              float* const wts, float2 (&pol_z)[4][16], unsigned& pol_cnt, int (&ep_cnt)[16],
                                              [[maybe_unused]] float* const hist = nullptr) {
    constexpr int EPB = 16, NW = 8, D = NB + 6, kThreads = 64 * NW;
    static_assert(!HIST || NB == 10, "scan history: 10 beams");
    using PL = mlp64::Layout<HIST ? kHistD : D>;
    constexpr int KS = PL::KS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int base = blockIdx.x * EPB;
    const int nloc = min(EPB, P.N - base);
    for (int k = tid; k < PL::P_ACTOR; k += kThreads) wts[k] = R.params[k];
    if (tid < nloc) load_state<NB, EPB, NW, const Params&>(P, sm, tid, base + tid);
    if (tid < EPB) ep_cnt[tid] = (tid < nloc) ? 0 : R.quota;
    const bool half_rows = P.obs_f16 != 0;
    load_obs_tile<NB, EPB, NW>(sm, R.obs0, base, nloc, half_rows);
    load_tables<NB, EPB, NW, const Params&>(P, sm);
    if constexpr (MOV) load_mover_phase0<NB, EPB, NW, const Params&>(P, sm, base, nloc);
    if constexpr (HIST) hist_init<NB, NW>(hist, R.obs0, base, nloc, half_rows);
    if (tid == 0) pol_cnt = 0u;
    __syncthreads();
    const float sigma = SENS ? P.sigma : 0.f;
    const int below_min = SENS ? P.below_min_mode : 0;
    auto tile_part = [&](const int t2, auto in_step) __attribute__((always_inline)) {   // as in rollout_kernel
        const int e = lane & 15, kk = lane >> 4;
        if constexpr (HIST) {
            const auto row = hist_obs_row<NB, EPB, NW, SENS, decltype(in_step)::value, const Params&>(P, sm, hist, e, kk, nloc,
                                                                                                    half_rows, sigma, below_min);
            const float (&xs)[KS] = row.x;
            mlp64::f32x4 c1[4];
            mlp64::policy_hidden1<PL>(wts, xs, lane, c1);
            float pz3, pz4;
            mlp64::policy_tile2<PL>(wts, c1, lane, t2, pz3, pz4);
            if (kk == 0) pol_z[t2][e] = make_float2(pz3, pz4);
        } else {
        const auto row = mlp64_obs_row<NB, EPB, NW, SENS, decltype(in_step)::value, const Params&>(P, sm, e, kk, nloc, half_rows,
                                                                                                 sigma, below_min);
        const float (&xs)[KS] = row.x;
        mlp64::f32x4 c1[4];
        mlp64::policy_hidden1<PL>(wts, xs, lane, c1);
        float pz3, pz4;
        mlp64::policy_tile2<PL>(wts, c1, lane, t2, pz3, pz4);
        if (kk == 0) pol_z[t2][e] = make_float2(pz3, pz4);
        }
    };
    auto finish = [&]() __attribute__((always_inline)) {   // any wave, lane = env
        const int e = lane;
        const float pz3[4] = {pol_z[0][e].x, pol_z[1][e].x, pol_z[2][e].x, pol_z[3][e].x};
        const float pz4[4] = {pol_z[0][e].y, pol_z[1][e].y, pol_z[2][e].y, pol_z[3][e].y};
        sm.act_l[e] = mlp64::policy_finish_mean<PL>(wts, pz3, pz4);
    };
    // the action of step 0, from the reset observations
    if (wave < 4) tile_part(wave, std::false_type{});
    __syncthreads();
    if (wave == 0 && lane < nloc) finish();
    __syncthreads();
    const EvalIO io = eval_io(R, ep_cnt);
    int n_done = 0;   // env steps executed
    for (int t = 0; t < R.T; ++t) {
        asm volatile("" ::: "memory");   // keeps the weight reads of the policy phase inside the loop (registers are scarce)
        // the policy of step t + 1 inside step t, behind barrier B2 (see rollout_kernel): waves 1-4 run the tile parts and the last
        // of the four to arrive finishes, all before barrier C
        const bool more = t + 1 < R.T;
        auto hook = [&](const int wv, const int ln) __attribute__((always_inline)) {
            if (more && wv >= 1 && wv <= 4) {
                tile_part(wv - 1, std::true_type{});
                last_arrival<4>(pol_cnt, ln, [&]() __attribute__((always_inline)) {
                    if (ln < nloc) finish();
                    if constexpr (HIST) {
                        if (ln < nloc) hist_shift<NB, EPB, NW, SENS, const Params&>(P, sm, hist, ln, half_rows, sigma, below_min);
                    }
                });
            }
        };
        step_body<NB, EPB, SENS, true, NW, BOXES, 0, const Params&, const EvalIO&, decltype(hook), MOV, POOL>(P, sm, next_env, io, false, 0, hook);
        n_done = t + 1;
        if (eval_quota_met<EPB>(ep_cnt, lane, R.quota)) break;   // behind barrier C: workgroup-uniform (see above)
    }
    if (tid < nloc) {
        store_state<NB, EPB, NW>(P, sm, tid, base + tid);
        R.count[base + tid] = ep_cnt[tid];
    }
    if (tid == 0) R.steps[blockIdx.x] = n_done;
}
template <int NB, bool SENS, bool BOXES>
__global__ __launch_bounds__(64 * 8) void evaluate_kernel(Params P, EvalArgs R) {
    constexpr int EPB = 16, NW = 8;
    using PL = mlp64::Layout<NB + 6>;
    __shared__ StepSmem<NB, EPB, NW> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];   // the actor, staged once for the whole launch
    __shared__ float2 pol_z[4][16];   // policy phase: per-tile partial sums of the two output units
    __shared__ unsigned pol_cnt;      // arrivals of the in-step policy's four tile waves (the last one finishes)
    __shared__ int ep_cnt[EPB];       // episodes recorded per env
    evaluate_body<NB, SENS, BOXES, false>(P, R, sm, next_env, wts, pol_z, pol_cnt, ep_cnt);
}
template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void evaluate_mov_kernel(Params P, EvalArgs R) {
    using PL = mlp64::Layout<16>;
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ unsigned pol_cnt;
    __shared__ int ep_cnt[16];
    evaluate_body<10, kMovSens, BOXES, true>(P, R, sm, next_env, wts, pol_z, pol_cnt, ep_cnt);
}

// the scan-history twins (navsim_evaluate_mlp64_hist), as rollout_hist_kernel / rollout_hist_mov_kernel
template <bool SENS, bool BOXES>
__global__ __launch_bounds__(64 * 8) void evaluate_hist_kernel(Params P, EvalArgs R) {
    using PL = mlp64::Layout<kHistD>;
    __shared__ StepSmem<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ unsigned pol_cnt;
    __shared__ int ep_cnt[16];
    __shared__ float hist[16 * kHistStride];
    evaluate_body<10, SENS, BOXES, false, true>(P, R, sm, next_env, wts, pol_z, pol_cnt, ep_cnt, hist);
}
template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void evaluate_hist_mov_kernel(Params P, EvalArgs R) {
    using PL = mlp64::Layout<kHistD>;
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[PL::P_ACTOR + 2];
    __shared__ float2 pol_z[4][16];
    __shared__ unsigned pol_cnt;
    __shared__ int ep_cnt[16];
    __shared__ float hist[16 * kHistStride];
    evaluate_body<10, kMovSens, BOXES, true, true>(P, R, sm, next_env, wts, pol_z, pol_cnt, ep_cnt, hist);
}

// (evaluate_resmlp_kernel keeps the parent commit's form of the staging, the policy phase and the EvalIO set-up: through
// load_obs_tile / load_tables / resmlp_preact / eval_io it took 5.503 instead of 5.482-5.498 ms per launch, profiles/
// persistent_refactor_ab.txt)
template <bool SENS, bool MOV>
__device__ __forceinline__ void evaluate_resmlp_body(const Params& P, const EvalArgs& R, StepSmemFor<10, 16, 8, MOV>& sm, int& next_env,
                                                     resmlp::PolicySmem& ps, resmlp::Block1Smem& bs, int (&ep_cnt)[16]) {
    constexpr int NB = 10, EPB = 16, NW = 8, D = NB + 6, DP = D + 1, kThreads = 64 * NW;
    static_assert(D == resmlp::rp::D && EPB == resmlp::kPolEnvs && NW == resmlp::kPolWaves, "the policy step's workgroup");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int base = blockIdx.x * EPB;
    const int nloc = min(EPB, P.N - base);
    if (tid < nloc) load_state<NB, EPB, NW, const Params&>(P, sm, tid, base + tid);
    if (tid < EPB) ep_cnt[tid] = (tid < nloc) ? 0 : R.quota;
    const bool half_rows = P.obs_f16 != 0;
    for (int k = tid; k < nloc * D; k += kThreads)
        sm.obs[(k / D) * DP + (k % D)] = half_rows ? __half2float(reinterpret_cast<const __half*>(R.obs0)[(size_t)base * D + k])
                                                   : reinterpret_cast<const float*>(R.obs0)[(size_t)base * D + k];
    for (int k = tid; k < 2 * NB; k += kThreads) sm.beam[k] = P.beam_cs[k];
    for (int k = tid; k < (int)(sizeof(Rects) / 8); k += kThreads)
        reinterpret_cast<uint64_t*>(&sm.rects)[k] = reinterpret_cast<const uint64_t*>(P.rects)[k];
    if constexpr (MOV) load_mover_phase0<NB, EPB, NW, const Params&>(P, sm, base, nloc);
    const int l15 = lane & 15, q = lane >> 4;
    const bool valid = l15 < nloc;
    resmlp::Weights W;
    resmlp::stage_block1(R.params, lane, wave, bs);
    __syncthreads();
    EvalIO io;
    io.action = nullptr; io.past_override = nullptr; io.obs_out = nullptr; io.reward = nullptr; io.done = nullptr;
    io.arrive = nullptr; io.ended = nullptr; io.ep_return = nullptr; io.ep_length = nullptr; io.ep_path_out = nullptr;
    io.cnt_l = ep_cnt; io.quota = R.quota; io.rec_flags = R.ep_flags; io.rec_length = R.ep_length; io.rec_return = R.ep_return;
    io.rec_path = R.ep_path;
    int n_done = 0;   // env steps executed
    for (int t = 0; t < R.T; ++t) {
        // ---- the mean of PPO.get_action (ppo.py:673-697) on the observation tile the previous step (or the reset) left in LDS
        resmlp::f32x4 xq = resmlp::zero4();
        if (valid) {
            const float* row = sm.obs + l15 * DP + 4 * q;
            xq = resmlp::f32x4{row[0], row[1], row[2], row[3]};
            if (half_rows) {
#pragma unroll
                for (int j = 0; j < 4; ++j) xq[j] = __half2float(__float2half_rn(xq[j]));
            }
        }
        float z3, z4;
        resmlp::load_weights_b(R.params, lane, wave, W);   // requested first: in flight while block 1 runs out of LDS
        resmlp::load_weights_a_lds(bs, lane, wave, W);
        resmlp::policy_preact_w(W, bs.b2a, bs.tail, xq, lane, wave, ps, z3, z4);
        if (wave == 0 && q == 0 && valid) sm.act_l[l15] = resmlp::policy_finish_mean(bs.tail, z3, z4);
        __syncthreads();
        // ---- the env step
        step_body<NB, EPB, SENS, true, NW, false, 0, const Params&, const EvalIO&, NoHook, MOV>(P, sm, next_env, io, false, 0);
        n_done = t + 1;    // (behind barrier C: the observation tile of step t + 1 is complete in sm.obs)
        if (eval_quota_met<EPB>(ep_cnt, lane, R.quota)) break;   // workgroup-uniform (see above)
    }
    if (tid < nloc) {
        store_state<NB, EPB, NW>(P, sm, tid, base + tid);
        R.count[base + tid] = ep_cnt[tid];
    }
    if (tid == 0) R.steps[blockIdx.x] = n_done;
}
template <bool SENS>
__global__ __launch_bounds__(64 * 8) void evaluate_resmlp_kernel(Params P, EvalArgs R) {
    constexpr int NB = 10, EPB = 16, NW = 8;
    __shared__ StepSmem<NB, EPB, NW> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) resmlp::PolicySmem ps;
    __shared__ __attribute__((aligned(16))) resmlp::Block1Smem bs;   // block 1's weights + the small tail of the parameters
    __shared__ int ep_cnt[EPB];       // episodes recorded per env
    evaluate_resmlp_body<SENS, false>(P, R, sm, next_env, ps, bs, ep_cnt);
}
#ifndef NAVSIM_POOL_TU
__global__ __launch_bounds__(64 * 8) void evaluate_resmlp_mov_kernel(Params P, EvalArgs R) {
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) resmlp::PolicySmem ps;
    __shared__ __attribute__((aligned(16))) resmlp::Block1Smem bs;
    __shared__ int ep_cnt[16];
    evaluate_resmlp_body<kMovSens, true>(P, R, sm, next_env, ps, bs, ep_cnt);
}
#endif   // NAVSIM_POOL_TU

// ---------------------------------------------------------------- n steps of an action tape in ONE launch (navsim_step_seq)
// The step loop of PPO.rollout / the evaluation loop (ppo.py:505-594, main.py:176-235) when the actions are already known -- a
// recorded tape, a scripted or random policy: a workgroup keeps its envs for all n steps, their state lives in LDS between the
// steps (HBM sees it before the first and after the last), and the steps follow each other with workgroup barriers only.  What a
// step kernel launch pays around its cast -- the launch ramp of 256 x 16 waves, the kernarg and state round trips ahead of the
// pose, the boundary between two graph nodes -- is paid once per tape; the segment stream of step t + 1 is requested while the
// pose of step t + 1 is computed.  Same step_body, same workgroup shapes as step_kernel: the rows are bit-identical to n
// navsim_step calls.  (Built with MachineLICM off, navbot_ppo_amd/build.py: the pass hoists the float64 constants of the whole
// step body out of the step loop and holds them in 60+ registers across it -- spills in the 16-wave shape, 11.3 instead of 9.4 us
// per step at configs[2].)
struct SeqArgs {
    StepIO io;   // the [T, N, .] buffers: action = the tape, obs_out [T, N, B + 6] (f32 or f16), reward / flags / episode statistics
                 // [T, N] (nullable as in navsim_step); step_body addresses row t through its row0 argument
    int T;
};
struct SeqKArgs {
    Params P;
    SeqArgs R;
};
typedef const SeqKArgs __attribute__((address_space(4))) * SeqKArgsPtr;

static_assert(std::is_trivially_copyable<SeqKArgs>::value && offsetof(SeqKArgs, P) == 0, "kernarg mirror of steps_kernel");

template <int NB, int EPB, bool SENS, int NW, bool BOXES, int PAIR, bool MOV, bool POOL = false>
__device__ __forceinline__ void steps_body(StepSmemFor<NB, EPB, NW, MOV, POOL>& sm, int& next_env) {
    // parameters through the kernarg segment pointer, as in step_kernel (scalar loads at each use, no spilled SGPRs)
    SeqKArgsPtr A = (SeqKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(A));
    using PRef = const Params __attribute__((address_space(4)))&;
    PRef P = A->P;
    const SeqArgs __attribute__((address_space(4)))& R = A->R;
    const int tid = threadIdx.x;
    const int base = blockIdx.x * EPB;
    const int nloc = min(EPB, P.N - base);
    const int T = R.T;
    float2 a_next = make_float2(0.f, 0.f);
    if (tid < nloc) {   // the envs' state: HBM -> LDS for the whole tape; the first action
        const int e = tid, i = base + e;
        a_next = R.io.action[i];
        load_state<NB, EPB, NW, PRef>(P, sm, e, i);
    }
    load_tables<NB, EPB, NW, PRef>(P, sm);
    if constexpr (MOV) load_mover_phase0<NB, EPB, NW, PRef>(P, sm, base, nloc);
    for (int t = 0; t < T; ++t) {
        const size_t N = (size_t)P.N;
        const size_t tn = (size_t)t * N;
        if (tid < nloc) {
            sm.act_l[tid] = a_next;
            if (t + 1 < T) a_next = R.io.action[tn + N + base + tid];   // lands under this step
        }
        __syncthreads();
        step_body<NB, EPB, SENS, true, NW, BOXES, PAIR, PRef, const StepIO __attribute__((address_space(4)))&, NoHook, MOV, POOL>(
            P, sm, next_env, R.io, t == T - 1, tn);
    }
}
template <int NB, int EPB, bool SENS, int NW = 4, bool BOXES = false, int PAIR = 0>
__global__ __launch_bounds__(64 * NW, min_waves_per_simd(NB, EPB, NW, PAIR, true)) void steps_kernel(SeqKArgs) {   // the segment IS the struct (see step_kernel)
    __shared__ StepSmem<NB, EPB, NW> sm;
    __shared__ int next_env;
    steps_body<NB, EPB, SENS, NW, BOXES, PAIR, false>(sm, next_env);
}
template <bool BOXES>
__global__ __launch_bounds__(64 * 8) void steps_mov_kernel(SeqKArgs) {
    __shared__ StepSmemMov<10, 16, 8> sm;
    __shared__ int next_env;
    steps_body<10, 16, kMovSens, 8, BOXES, 0, true>(sm, next_env);
}

// ---------------------------------------------------------------- the persistent rollout at the big shard shapes
// navsim_rollout_mlp64 for shards beyond 4096 envs: steps_kernel's workgroup (64 envs on 16 waves, one per CU, the cast at its
// vector-issue bound, the cast variants of the step kernel) with a policy phase in front of every step -- the closed-loop form of the
// tape kernel: the action of step t is PPO.get_action (ppo.py:673-706) of the observation tile step t - 1 left in LDS.
// The phase is bound by the SIMDs' MFMA pipes (64 envs x 10.2 kFLOP at the f32 MFMA rate of 64 FLOP per cycle and SIMD = 2560
// cycles), so each of the EPB / 16 policy tiles of 16 envs belongs to ONE wave -- the waves of a workgroup land on the SIMDs round
// robin, one tile per SIMD -- which runs policy_wave16's sequence: layer 1, the four 16-row tiles of layer 2 in order, the finish
// on its lanes 0-15 (no partial sums through LDS, no redundant layer 1: two waves per tile measured 2.05 us per step over the tape
// kernel, this 1.6).  The action noise does not depend on the observation: wave EPB / 16 draws the noise of step t + 1 during the
// policy phase of step t (two LDS rows that take turns).  Same device functions, same order of the partial sums and same Philox
// keys as rollout_kernel / navppo_mlp64_act: the rows are bit-identical to the per-step entry points.
struct BigKArgs {
    Params P;
    RolloutArgs R;
    StepIO io;   // rows of step t at element offset t N: obs_out = obs_buf + N D (row t + 1 of obs_buf), reward / flags / statistics
};
typedef const BigKArgs __attribute__((address_space(4))) * BigKArgsPtr;

static_assert(std::is_trivially_copyable<BigKArgs>::value && offsetof(BigKArgs, P) == 0, "kernarg mirror of rollout_big_kernel");

// (rollout_big_kernel and its twin with movers, rollout_big_mov_kernel, share this body.  Unlike the other twins' bodies it declares
// the LDS variables itself -- one set per instantiation, i.e. per kernel, as each is inlined into exactly one: these kernels sit
// at their 128 registers, and with the variables handed in as references three SENS instantiations WITHOUT movers changed their
// scratch; see profiles/movers_big_kernel_resources.txt.)
template <int EPB, bool SENS, int NW, bool BOXES, int PAIR, bool MOV>
__device__ __forceinline__ void rollout_big_body() {
    constexpr int NB = 10, D = NB + 6, DP = D + 1, kThreads = 64 * NW;
    constexpr int TW = EPB / 16;   // policy tiles = MFMA waves of the policy phase
    using PL = mlp64::Layout<D>;
    constexpr int KS = PL::KS;
    static_assert(D == mlp64::IN, "64-env workgroups: the 10-beam tile (36 beams do not fit the LDS)");
    static_assert(EPB % 16 == 0 && EPB <= 64 && TW < NW, "policy phase: EPB / 16 tile waves + the noise wave");
    __shared__ StepSmemFor<NB, EPB, NW, MOV> sm;   // (movers: 16 bytes per env more, 153,352 bytes at 64 envs)
    __shared__ int next_env;
    __shared__ __attribute__((aligned(16))) float wts[mlp64::P_ACTOR + 2];   // the actor, staged once for all T steps
    __shared__ float2 pol_eps[2][EPB];   // action noise of this step and of the next one
    BigKArgsPtr A = (BigKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(A));
    using PRef = const Params __attribute__((address_space(4)))&;
    PRef P = A->P;
    const RolloutArgs __attribute__((address_space(4)))& R = A->R;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int base = blockIdx.x * EPB;
    const int nloc = min(EPB, P.N - base);
    const int T = R.T;
    {
        const float* const prm = R.params;
        for (int k = tid; k < mlp64::P_ACTOR; k += kThreads) wts[k] = prm[k];
    }
    if (tid < nloc) load_state<NB, EPB, NW, PRef>(P, sm, tid, base + tid);   // the envs' state for the whole rollout
    const bool half_rows = P.obs_f16 != 0;   // float16 observation buffers: the policy reads what a reader of the buffers would
    load_obs_tile<NB, EPB, NW>(sm, R.obs_buf, base, nloc, half_rows);
    load_tables<NB, EPB, NW, PRef>(P, sm);
    if constexpr (MOV) load_mover_phase0<NB, EPB, NW, PRef>(P, sm, base, nloc);
    const uint32_t step0 = R.step_base ? *R.step_base : 0u;
    const float var = *R.var_ptr;
    const uint64_t seed = R.seed, gid = P.env_id_base + (uint64_t)(base + lane);
    // policy tile k (envs 16 k .. 16 k + 15) belongs to wave TW + k -- the waves of a workgroup land on the SIMDs round robin, one
    // tile per SIMD -- and the noise of a row to wave 2 TW; wave 0 stays free for the rules (see the hook below)
    constexpr int kTileWave0 = TW, kNoiseWave = 2 * TW;
    static_assert(kNoiseWave < NW, "tile waves and the noise wave beside wave 0");
    // get_action (ppo.py:673-706) of policy tile `k` on the observation tile in LDS -> action / log-prob of row tn / N
    const float sigma = SENS ? P.sigma : 0.f;
    const int below_min = SENS ? P.below_min_mode : 0;
    const float sd = sqrtf(var), log_var = logf(var);   // policy_finish's sqrtf(var) / logf(var), once per launch: same bits
    auto tile_policy = [&](const int k, const size_t tn, const int eps_row, auto in_step) __attribute__((always_inline)) {
        const int e = 16 * k + (lane & 15), kk = lane >> 4;   // lane (env, kk) feeds obs[env][4 kk .. 4 kk + 3]
        const bool valid = e < nloc;
        // (mlp64_obs_row's code, written out: through the helper the SENS instantiations with the 128-segment passes spill 28 instead
        // of 20 bytes of scratch)
        float xs[KS];
        if constexpr (decltype(in_step)::value) {   // inside a step, behind barrier B2: the rows the step will leave
            next_obs_n<NB, EPB, NW, SENS, KS, PRef>(P, sm, min(e, nloc - 1), KS * kk, sigma, below_min, xs);
            if (half_rows) {
#pragma unroll
                for (int j = 0; j < KS; ++j) xs[j] = __half2float(__float2half_rn(xs[j]));
            }
        } else {
            mlp64::policy_row<PL>(sm.obs + min(e, nloc - 1) * DP, kk, half_rows, xs);
        }
        if (!valid) {
#pragma unroll
            for (int j = 0; j < KS; ++j) xs[j] = 0.f;
        }
        const float2 eps = pol_eps[eps_row][min(e, nloc - 1)];   // requested ahead of the MFMA chain, used behind it
        mlp64::f32x4 c1[4];
        mlp64::policy_hidden1<PL>(wts, xs, lane, c1);
        float pz3[4], pz4[4];
#pragma unroll
        for (int t2 = 0; t2 < 4; ++t2) mlp64::policy_tile2<PL>(wts, c1, lane, t2, pz3[t2], pz4[t2]);
        if (kk == 0 && valid) {
            const mlp64::PolicyOut o = mlp64::policy_finish_pre<PL>(wts, pz3, pz4, var, sd, log_var, eps.x, eps.y);
            sm.act_l[e] = make_float2(o.a0, o.a1);
            reinterpret_cast<float2*>(R.act_buf)[tn + base + e] = make_float2(o.a0, o.a1);
            R.logp_buf[tn + base + e] = o.logp;
        }
    };
    auto draw_noise = [&](const int t) __attribute__((always_inline)) {   // the noise of rollout row t: rows take turns in two LDS rows
        float e0, e1;
        if constexpr (MOV) {
            // the global env id is worked out HERE, from a lane index the compiler cannot follow out of the step loop: held in a
            // register pair across the steps it was the one value the 64-env twin with tile boxes spilled (12 bytes of scratch)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            mlp64::policy_noise(step0 + (uint32_t)t, seed, P.env_id_base + (uint64_t)(base + ln), e0, e1);
        } else {
            mlp64::policy_noise(step0 + (uint32_t)t, seed, gid, e0, e1);
        }
        pol_eps[t & 1][lane] = make_float2(e0, e1);
    };
    if (wave == kNoiseWave && lane < nloc) {
        draw_noise(0);
        if (T > 1) draw_noise(1);
    }
    __syncthreads();
    // the action of step 0, from the reset observations
    if (wave >= kTileWave0 && wave < kTileWave0 + TW) tile_policy(wave - kTileWave0, 0, 0, std::false_type{});
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const size_t N = (size_t)P.N;
        const size_t tn = (size_t)t * N;
        asm volatile("" ::: "memory");   // keeps the weight reads of the policy phase inside the loop
        // The policy of step t + 1 runs INSIDE step t, behind barrier B2, while wave 0 works through the rules (a float64 latency
        // chain) and the other waves would only wait for it at barrier C.  Whether the rules replace an env's observation row by its
        // reset observation (ppo.py:582-593) the tile waves work out themselves from the values that are final at B2 (next_obs_n):
        // they read exactly the rows the step leaves -- same device functions on the same inputs, the buffers keep their bits --
        // and the action is in LDS before barrier C, so the next step starts without a policy phase in front of it.  Round 3 ran
        // the phase between the steps, the whole workgroup waiting for it: + 1.6 us per step over the tape kernel.
        const bool more = t + 1 < T;
        auto hook = [&](const int wv, const int ln) __attribute__((always_inline)) {
            if (more) {
                if (wv >= kTileWave0 && wv < kTileWave0 + TW) tile_policy(wv - kTileWave0, tn + N, (t + 1) & 1, std::true_type{});
                else if (wv == kNoiseWave && ln < nloc && t + 2 < T) draw_noise(t + 2);   // row (t + 2) & 1: not the one being read
            }
        };
        step_body<NB, EPB, SENS, true, NW, BOXES, PAIR, PRef, const StepIO __attribute__((address_space(4)))&, decltype(hook), MOV>(
            P, sm, next_env, A->io, t == T - 1, tn, hook);
        // the observation tile of step t + 1 is in sm.obs (its store only reads it) and its action in sm.act_l
    }
}
template <int EPB, bool SENS, int NW, bool BOXES = false, int PAIR = 0>
__global__ __launch_bounds__(64 * NW) void rollout_big_kernel(BigKArgs) {   // the segment IS the struct (see step_kernel)
    rollout_big_body<EPB, SENS, NW, BOXES, PAIR, false>();
}
// Movers in the big shapes (navsim_rollout_mlp64 only: pick_rollout): 64 envs on 16 waves or 32 on 8, with the 64-segment passes or
// the tile boxes (movers need a shared static map, so the 128-segment passes never meet a tape).  SENS is a parameter here, unlike
// in the 16-env twins: the 64-env workgroup sits at its 128 registers, and a handle without the sensor options should not carry
// them there (registers, scratch and LDS of the eight twins beside their siblings: profiles/movers_big_kernel_resources.txt).
template <int EPB, bool SENS, int NW, bool BOXES>
__global__ __launch_bounds__(64 * NW) void rollout_big_mov_kernel(BigKArgs) {
    rollout_big_body<EPB, SENS, NW, BOXES, 0, true>();
}

#ifndef NAVSIM_POOL_TU   // (down to the end of the file: the small kernels, the scans and the host side / C ABI are navsim.hip's own;
                         // navsim_pool.hip compiles the step body and what stands around it, above, a second time)
// Env.getOdometry (environment_new.py:138-181) for n independent (position, orientation quaternion, goal) triples
__global__ void odometry_kernel(int n, const double* __restrict__ px, const double* __restrict__ py, const double* __restrict__ q,
                                const double* __restrict__ goal, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double yaw = yaw_from_quat4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
    double rel, diff;
    goal_rel(px[i], py[i], goal[2 * i], goal[2 * i + 1], yaw, rel, diff);
    out[3 * i] = yaw; out[3 * i + 1] = rel; out[3 * i + 2] = diff;
}

// clears kRecValid of every env: the cached next-episode records no longer match (tables / rectangles / counters changed)
__global__ void invalidate_records_kernel(int32_t* __restrict__ ep_step, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) ep_step[i] = (int32_t)((uint32_t)ep_step[i] & kStepMask);
}

// The yaw of Env.getOdometry (environment_new.py:142-147) at every start pose, tabulated with the device's own sin / cos /
// atan2 through the same device function the reset kernel calls, so that the step kernel's speculative lanes reproduce
// goal_angles(x, y, yaw, ...) bit for bit without the quaternion round trip (an atan2 off the record path)
__global__ void starts_sc_kernel(const double* __restrict__ starts, int K, double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const double th = starts[3 * k + 2];
    out[k] = yaw_from_quat(sin(th / 2), cos(th / 2));
}

// ---------------------------------------------------------------- reset (Env.reset, masked)
__global__ void reset_kernel(Params P, const uint8_t* __restrict__ mask, void* __restrict__ obs_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    if (mask && !mask[i]) return;
    const int B = P.B, D = B + 6;
    uint32_t ctr = P.rng_ctr[i];
    double gx, gy, yaw, rel_theta, diff;
    int k0;
    sample_episode<const Params&, true>(P, *P.rects, i, ctr, k0, gx, gy);
    const double x = P.starts[3 * k0], y = P.starts[3 * k0 + 1], th = P.starts[3 * k0 + 2];
    goal_angles(x, y, th, gx, gy, yaw, rel_theta, diff);
    const double dist = hypot(gx - x, gy - y);
    const float* sp = P.spawn_scan + ((P.spawn_per_env ? (size_t)i * P.K : 0) + k0) * B;  // nearest hits at the start pose
    const uint64_t gid = P.env_id_base + (uint64_t)i;
    auto lidar = [&](int b) {
        const float n = (P.sigma > 0.f) ? lidar_noise(P.key0, P.key1, gid, ctr, 0xFFFFu, b) : 0.f;
        float r = sensor_value(sp[b], P.sigma, n, P.below_min_mode);
        if (r == INFINITY) r = 3.5f;  // environment_new.py:193-194
        return r / 3.5f;              // :362
    };
    const float tail[6] = {0.f, 0.f, (float)(dist / P.diag), (float)(yaw / 360), (float)(rel_theta / 360), (float)(diff / 180)};
    if (P.obs_f16) {
        __half* o = reinterpret_cast<__half*>(obs_out) + (size_t)i * D;
        for (int b = 0; b < B; ++b) o[b] = __float2half_rn(lidar(b));
        for (int k = 0; k < 6; ++k) o[B + k] = __float2half_rn(tail[k]);
    } else {
        float* o = reinterpret_cast<float*>(obs_out) + (size_t)i * D;
        for (int b = 0; b < B; ++b) o[b] = lidar(b);
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

// ---------------------------------------------------------------- LiDAR only (spawn scans, tests, tooling)
// thread = (env, pose): thread t casts pose[(t % n_poses_per_env) or t] against env (t / n_poses_per_env)'s map.
//   spawn scans:  n_poses_per_env = K, shared_poses = 1 : pose table [K][3] reused by every env
//   navsim_raycast: n_poses_per_env = 1, shared_poses = 0 : pose[t]
// Movers (Params::mov_tape): the env's tape phase joins its static map -- the reset phase phase0[env] for the spawn scans
// (shared_poses = 1), the phase the env last observed, (ep_step + phase0) mod P, for navsim_raycast (shared_poses = 0); with a
// bank of tapes (navsim_set_mover_bank) P and the base row are those of the env's own tape (mover_bp).
__global__ void raycast_kernel(Params P, const double* __restrict__ pose, int n_poses_per_env, int shared_poses, int n,
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
    for (int b = 0; b < P.B; ++b) {
        const double bc = P.beam_cs[b], bs = P.beam_cs[P.B + b];
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
        // raw: the nearest hit itself (spawn-scan table, noise is applied when it is used); else the noise-free scan value
        ranges[(size_t)t * P.B + b] = raw ? best : sensor_value(best, 0.f, 0.f, P.below_min_mode);
    }
}

// noise-free lidar entries of a reset observation from the nearest hits at the start pose (environment_new.py:192-198,:362)
__global__ void spawn_obs_kernel(const float* __restrict__ best, int n, int below_min_mode, float* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float r = sensor_value(best[k], 0.f, 0.f, below_min_mode);
    if (r == INFINITY) r = 3.5f;
    out[k] = r / 3.5f;
}

// ---------------------------------------------------------------- navsim_stack_rows: [R, N, 16] rows -> [R, N, 42] history rows
// Column c of out[r][n] is a copy of one entry of obs[r'][n], r' in {r, r - 1, r - 2} clamped to the episode's first row (the rule
// is written out in include/navsim.h; env.stack_rows_reference is its host mirror).  A bandwidth kernel: the output is one flat
// array, a thread owns 16 bytes of it (4 floats / 8 halves, crossing a row boundary where they do) and stores them at once;
// neighbouring threads read neighbouring entries of the same three source rows, which the caches serve (each input row is read
// three times, the output written once: 3.6 x the input's bytes in all).
// CONT (navsim_stack_rows_cont with a carry-in): row 0 does not start the episodes -- its columns 16..37 ARE the carry ([N, kHistLen]
// f32: the two scans and the action pair in front of row 0, the episode cut already inside), and row 1, unless ended[0] cuts it off,
// takes its oldest frame from the carry's first scan.  From row 2 on nothing looks in front of row 0.
template <class T, bool CONT = false>
__global__ __launch_bounds__(256) void stack_rows_kernel(const T* __restrict__ obs, const uint8_t* __restrict__ ended, const int R,
                                                         const int N, T* __restrict__ out,
                                                         [[maybe_unused]] const float* __restrict__ carry = nullptr) {
    constexpr int V = 16 / (int)sizeof(T), DI = 16, DO = kHistD;
    const size_t total = (size_t)R * (size_t)N * DO;
    const size_t k0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (k0 >= total) return;
    size_t q = k0 / DO;             // flat row index r N + n
    int c = (int)(k0 - q * DO);
    const size_t n_rows = (size_t)R * (size_t)N;
    size_t s0 = 0, s1 = 0, s2 = 0;   // element offsets of the rows frames 0, 1, 2 are copied from
    [[maybe_unused]] const float* cr = nullptr;   // CONT: the env's carry row
    [[maybe_unused]] bool c1 = false, c2 = false;   // CONT: columns 16..25 and 36..37 / columns 26..35 come from the carry
    auto locate = [&](const size_t row) {
        const size_t r = row / (size_t)N;
        const bool cut0 = (r == 0) || (ended[row - (size_t)N] != 0);                  // row r starts an episode
        const bool cut1 = cut0 || (r == 1) || (ended[row - 2 * (size_t)N] != 0);      // ... or row r - 1 does
        s0 = row * DI;
        s1 = cut0 ? s0 : s0 - (size_t)N * DI;
        s2 = cut0 ? s0 : (cut1 ? s1 : s1 - (size_t)N * DI);
        if constexpr (CONT) {
            cr = carry + (row - r * (size_t)N) * kHistLen;
            c1 = r == 0;
            c2 = c1 || (r == 1 && !cut0);
        }
    };
    locate(q);
    alignas(16) T v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        T x = T(0.f);
        if (q < n_rows) {
            if constexpr (CONT) {   // (the carry holds the rows' own values as float: the conversion back is exact)
                if (c < DI) x = obs[s0 + c];
                else if (c < 26) x = c1 ? T(cr[c - 16]) : obs[s1 + (c - 16)];
                else if (c < 36) x = c2 ? T(cr[c1 ? c - 16 : c - 26]) : obs[s2 + (c - 26)];
                else if (c < 38) x = c1 ? T(cr[c - 16]) : obs[s1 + (c - 26)];
            } else {
            if (c < DI) x = obs[s0 + c];
            else if (c < 26) x = obs[s1 + (c - 16)];
            else if (c < 36) x = obs[s2 + (c - 26)];
            else if (c < 38) x = obs[s1 + (c - 26)];   // past_action of the previous row: columns 10, 11
            }
        }
        v[j] = x;
        if (++c == DO) {
            c = 0;
            ++q;
            if (q < n_rows) locate(q);
        }
    }
    if (k0 + V <= total) {
        *reinterpret_cast<uint4*>(out + k0) = *reinterpret_cast<const uint4*>(v);
    } else {
        for (int j = 0; j < V; ++j)
            if (k0 + j < total) out[k0 + j] = v[j];
    }
}

// navsim_stack_rows_cont's carry-out: columns 16..37 of the last output row as float, [N, kHistLen].  Launched behind the kernel
// above, so a caller may hand in the buffer the carry-in came from.
template <class T>
__global__ __launch_bounds__(256) void stack_rows_carry_kernel(const T* __restrict__ last_row, const int N, float* __restrict__ carry) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N * kHistLen) return;
    carry[k] = (float)last_row[(size_t)(k / kHistLen) * kHistD + 16 + (k % kHistLen)];
}

// ---------------------------------------------------------------- return scan (PPO.compute_rtgs)
// R[t] = r[t] + gamma R[t+1], restarting at 0 behind every episode end and at the batch end (ppo.py:658-666), float64
// accumulate, float32 store.  Per env column that is a serial recurrence of T dependent float64 multiply -> add pairs
// (~35 cycles each: 7.5 us for T = 512 however the memory is fed -- rounds 1-2: 40 us, then 16.5 us with an LDS pipeline).
// This kernel splits the column over T instead: a workgroup owns kRtgCols adjacent columns and kRtgChunks chunks of
// kRtgRows rows (thread = column x chunk, 1024 waves at N = 4096 with 64 loads in flight per lane):
//   pass 1   every chunk scans its rows from registers with carry-in 0 -> B (the return at its first row) and
//            A = gamma^kRtgRows, or 0 when an episode ends inside the chunk: R_first = B + A R_in
//   carry    R_in of chunk c = R_first of chunk c + 1, composed serially from the (A, B) pairs in LDS (<= 15 steps)
//   pass 2   the chunk re-runs the reference's recurrence from its true carry-in and stores
// Every row behind (earlier than) an episode end inside its chunk carries the reference's bits by construction; the others see
// a carry-in whose float64 rounding differs from the serial chain's (relative 1e-15), which moves the float32 store by one ulp
// with probability ~2e-8 per element.  Contract: <= 1 float32 ulp from ppo.py:660-669, flags untouched (tests state it);
// `exact` != 0 (argument of navsim_rtg_scan / navsim_gae_scan) selects the serial kernel below, which is bit-identical.  "if ended: disc = 0" is folded into the
// factor: disc * 0 is (+-)0 and r + (+-)0 == r, so the value is that of ppo.py:660-665 while the select leaves the chain.
// T > 512: super-chunks of 512 rows from the batch end, the carry between them is the stored float64 of pass 2.
constexpr int kRtgCols = 16, kRtgChunks = 16, kRtgRows = 32, kRtgSuper = kRtgChunks * kRtgRows;

//
// GAE (north-star extension, off by default; navsim_gae_scan): the lambda-return obeys the same kind of recurrence,
//   R[t] = (r[t] + gamma (1 - lambda) V[t+1]) + gamma lambda R[t+1]      behind an episode end / the batch end: R[t] = r[t]
// (episode ends and the batch end are terminal as in ppo.py:552-553,658-666; last_value bootstraps the batch end only when
// given), advantage A[t] = float32(R[t]) - V[t].  lambda = 1 without bootstrap: the additive term is r[t] + 0 and the factor
// gamma * 1, i.e. the arithmetic of the return scan bit for bit, and A = rtg - V (ppo.py:277).
//
// TRUNC (off by default; navsim_gae_scan_trunc): a time-out -- ended without done or arrive, navppo_episode_sums' definition -- is
// not the end of the robot: the value of the next state the batch never saw is estimated by V of the row itself (rsl_rl:
// rewards += gamma * values * time_outs), so the additive term of such a row is r[t] + gamma V[t] while its factor stays 0 like
// that of every episode end.  Two more byte streams (done, arrive), folded into the chunk's ended byte right at the load; rows
// without a time-out evaluate the expressions of the GAE form, so a batch without one comes out bit-identical to it.
template <bool GAE, bool TRUNC = false>
__global__ __launch_bounds__(256) void rtg_kernel_split(const float* __restrict__ rew, const uint8_t* __restrict__ ended, int T, int N,
                                                        double gamma, float* __restrict__ out, const float* __restrict__ value,
                                                        const float* __restrict__ last_value, double lam, float* __restrict__ adv,
                                                        const uint8_t* __restrict__ done = nullptr,
                                                        const uint8_t* __restrict__ arrive = nullptr) {
    static_assert(GAE || !TRUNC, "a time-out bootstraps with V: the truncation-aware scan is a GAE scan");
    __shared__ double s_b[kRtgChunks][kRtgCols], s_a[kRtgChunks][kRtgCols], s_sup[kRtgCols];
    const int tid = threadIdx.x, col = tid & (kRtgCols - 1), c = tid >> 4;
    // Workgroups go round-robin over the 8 XCDs (one L2 each) while a 128-byte line holds the rewards of 2 column blocks and
    // the flags of 8: give each XCD runs of 8 adjacent column blocks so that a line is fetched into one L2, not into eight
    // (measured 33.6 MB instead of 10.5 MB over the fabric otherwise).  Needs the block count to be a multiple of 64.
    int q = blockIdx.x;
    if ((gridDim.x & 63) == 0) {
        const int x = q & 7, y = q >> 3;
        q = ((y >> 3) * 8 + x) * 8 + (y & 7);
    }
    const size_t n = (size_t)q * kRtgCols + col;   // N % 16 == 0: all 16 columns exist
    const double gl = GAE ? gamma * lam : gamma, gv = GAE ? gamma * (1.0 - lam) : 0.0;
    double gpow = 1.0;
#pragma unroll
    for (int u = 0; u < kRtgRows; ++u) gpow *= gl;
    double rsup = (GAE && last_value) ? (double)last_value[n] : 0.0;  // ppo.py:660 (GAE: R beyond the batch end = the bootstrap value)
    for (int t_hi = T; t_hi > 0; t_hi -= kRtgSuper) {
        // rows t0 .. t0 + 31 of this chunk; t < 0 only below the first row of the batch (the lowest super-chunk): loaded from
        // row 0 (any valid address), never stored, and nothing valid depends on them (the scan runs towards them)
        const int t0 = t_hi - kRtgSuper + c * kRtgRows;
        float r[kRtgRows];
        uint8_t e[kRtgRows];
        float v[GAE ? kRtgRows + 1 : 1];   // GAE: V of rows t0 .. t0 + 32 (the row after the chunk; beyond the batch: last_value or 0)
        if (GAE) {
            const int tn = t0 + kRtgRows;
            v[kRtgRows] = tn < T ? value[(size_t)max(tn, 0) * N + n] : (last_value ? last_value[n] : 0.f);
        }
#pragma unroll
        for (int u = kRtgRows - 1; u >= 0; --u) {   // requested in the order pass 1 consumes them
            const size_t k = (size_t)max(t0 + u, 0) * N + n;
            r[u] = rew[k];
            e[u] = ended[k];
            if (GAE) v[u] = value[k];
            if constexpr (TRUNC) {   // both bytes loaded whatever `ended` holds (a load behind a select would wait for that byte first)
                const uint8_t term = done[k] | arrive[k];
                e[u] = e[u] ? (term ? 1 : 2) : 0;   // 2 = a time-out: ended, neither done nor arrive
            }
        }
        // The batch end is terminal like an episode end (ppo.py:601,658) unless last_value bootstraps it: then the last row's
        // factor stays gamma lambda and R beyond it is last_value (rsup above), so R[T-1] = r + gamma (1-lambda) V_last + gamma lambda V_last
        double b = 0;
        bool any = false;
#pragma unroll
        for (int u = kRtgRows - 1; u >= 0; --u) {
            const double g = e[u] ? 0.0 : gl;
            double add = GAE ? (double)r[u] + (e[u] ? 0.0 : gv * (double)v[u + 1]) : (double)r[u];
            if constexpr (TRUNC) add = (double)r[u] + (e[u] == 2 ? gamma * (double)v[u] : e[u] ? 0.0 : gv * (double)v[u + 1]);
            b = add + b * g;
            any |= e[u] != 0;
        }
        s_b[c][col] = b;
        s_a[c][col] = any ? 0.0 : gpow;
        __syncthreads();
        double ak[kRtgChunks], bk[kRtgChunks];
#pragma unroll
        for (int k = 1; k < kRtgChunks; ++k) {
            ak[k] = s_a[k][col];
            bk[k] = s_b[k][col];
        }
        double R = rsup;
#pragma unroll
        for (int k = kRtgChunks - 1; k >= 1; --k)
            if (k > c) R = bk[k] + ak[k] * R;
#pragma unroll
        for (int u = kRtgRows - 1; u >= 0; --u) {
            const double g = e[u] ? 0.0 : gl;
            double add = GAE ? (double)r[u] + (e[u] ? 0.0 : gv * (double)v[u + 1]) : (double)r[u];
            if constexpr (TRUNC) add = (double)r[u] + (e[u] == 2 ? gamma * (double)v[u] : e[u] ? 0.0 : gv * (double)v[u + 1]);
            R = add + R * g;   // ppo.py:665
            if (t0 + u >= 0) {
                const size_t k = (size_t)(t0 + u) * N + n;
                if (out) out[k] = (float)R;   // ppo.py:669
                if (GAE) adv[k] = (float)R - v[u];
            }
        }
        if (t_hi > kRtgSuper) {   // uniform: another super-chunk follows
            if (c == 0) s_sup[col] = R;
            __syncthreads();
            rsup = s_sup[col];
        }
    }
}

// any N / alignment, and the bit-exact mode: thread = env column, reverse over T
__global__ void rtg_kernel_generic(const float* __restrict__ rew, const uint8_t* __restrict__ ended, int T, int N, double gamma,
                                   float* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double disc = 0;  // ppo.py:660
#pragma unroll 8
    for (int t = T - 1; t >= 0; --t) {
        const size_t k = (size_t)t * N + n;
        const float r = rew[k];
        if (ended[k]) disc = 0;
        disc = (double)r + disc * gamma;  // ppo.py:665
        out[k] = (float)disc;             // ppo.py:669
    }
}

// GAE, any N: thread = env column, reverse over T (the recurrence of rtg_kernel_split<true>, serially)
__global__ void gae_kernel_generic(const float* __restrict__ rew, const uint8_t* __restrict__ ended, const float* __restrict__ value,
                                   const float* __restrict__ last_value, int T, int N, double gamma, double lam,
                                   float* __restrict__ adv, float* __restrict__ ret) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double gl = gamma * lam, gv = gamma * (1.0 - lam);
    double R = last_value ? (double)last_value[n] : 0.0;
    float vnext = last_value ? last_value[n] : 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t k = (size_t)t * N + n;
        const bool e = ended[k] != 0;
        const float vt = value[k];
        const double g = e ? 0.0 : gl;
        const double add = (double)rew[k] + (e ? 0.0 : gv * (double)vnext);
        R = add + R * g;
        if (ret) ret[k] = (float)R;
        adv[k] = (float)R - vt;
        vnext = vt;
    }
}

// the truncation-aware twin of gae_kernel_generic (navsim_gae_scan_trunc; the recurrence of rtg_kernel_split<true, true>, serially):
// a time-out's additive term is r + gamma V of the row itself, everything else as above
__global__ void gae_trunc_kernel_generic(const float* __restrict__ rew, const uint8_t* __restrict__ ended, const uint8_t* __restrict__ done,
                                         const uint8_t* __restrict__ arrive, const float* __restrict__ value,
                                         const float* __restrict__ last_value, int T, int N, double gamma, double lam,
                                         float* __restrict__ adv, float* __restrict__ ret) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double gl = gamma * lam, gv = gamma * (1.0 - lam);
    double R = last_value ? (double)last_value[n] : 0.0;
    float vnext = last_value ? last_value[n] : 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t k = (size_t)t * N + n;
        const bool e = ended[k] != 0;
        const uint8_t term = done[k] | arrive[k];   // loaded whatever `ended` holds: no load waits for another
        const bool trunc = e && !term;
        const float vt = value[k];
        const double g = e ? 0.0 : gl;
        const double add = (double)rew[k] + (trunc ? gamma * (double)vt : e ? 0.0 : gv * (double)vnext);
        R = add + R * g;
        if (ret) ret[k] = (float)R;
        adv[k] = (float)R - vt;
        vnext = vt;
    }
}

#endif   // NAVSIM_POOL_TU
}  // namespace

#ifndef NAVSIM_POOL_TU
// ==================================================================== host side / C ABI
#include "navsim_select.h"   // which instantiation runs for a handle: the rule, its thresholds and the measurements behind them
#include "navsim_pool.h"     // the sector-LiDAR twins: kernels of a translation unit of their own (navsim_pool.hip)
namespace sel = navsim_select;
static_assert(kMovSens == sel::kMovTwinsSens, "the 16-env mover twins are built in the form the rule picks");
static_assert(kMaxPool == sel::kMaxScanPool, "the pooled twins hold the rays of the largest scan_pool the rule admits");

// A hipMalloc allocation and its owner (move-only): freed by reset(), by the next alloc() and with the owner
template <class T>
class DevBuf {
    T* p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    ~DevBuf() { (void)reset(); }
    hipError_t alloc(size_t n) {   // n elements
        (void)reset();
        return hipMalloc(&p_, sizeof(T) * n);
    }
    hipError_t reset() {
        const hipError_t e = hipFree(p_);
        p_ = nullptr;
        return e;
    }
    T* get() const { return p_; }
};

struct navsim {
    navsim_cfg cfg;
    Params P;
    DevBuf<unsigned char> state_block;   // one allocation for all per-env state
    DevBuf<double> beam_cs_dev;
    DevBuf<Rects> rects_dev;
    Rects rects_host;
    DevBuf<float4> seg_sorted_dev;   // shared maps of 65..4096 segments: the handle's own Morton-ordered copy
    DevBuf<float4> tile_box_dev;
    DevBuf<float> spawn_scan_dev;
    DevBuf<float> spawn_obs_dev;
    DevBuf<double> starts_dev;   // [K][3]
    DevBuf<double> starts_sc_dev;  // [K]
    DevBuf<double> goals_dev;    // [G][2]
    DevBuf<int32_t> mov_phase0_dev;   // navsim_set_movers: the handle's copy of the per-env phase offsets
    DevBuf<uint2> mov_bp_dev;         // navsim_set_mover_bank: (base row, period), the tape id and the tapes' goal rectangles
    DevBuf<int32_t> mov_tid_dev;
    DevBuf<double> mov_rects_dev;
    bool has_map = false;
    // kernel-shape overrides of THIS handle (navsim_set_shape; tests and A/B timing): envs per workgroup, 0 = the rule of
    // navsim_select::pick_epb; pair_cast false = 64-segment passes for every map
    int force_epb = 0;
    bool pair_cast = true;
    int pair_cast_request = -1;   // what navsim_set_shape was given (-1 = the rule): reported by navsim_get_info
    // sector LiDAR (navsim_set_scan_pool): rays per scan column, mirrored in P.pool; the pooled twins are mover kernels, and a handle
    // without a tape hands them this one-row tape of one absent (NaN) segment (launch_params)
    int scan_pool = 1;
    DevBuf<float4> pool_tape_dev;
};

// The parameter block a stepping launch passes: the handle's, and on a pooled handle without movers the one-row tape of one absent
// segment (period 1, no phase offsets), which the cull of the mover pass drops -- the scan is that of the static map alone.
static Params launch_params(const navsim* h) {
    Params P = h->P;
    if (h->scan_pool > 1 && !P.mov_tape) {
        P.mov_tape = h->pool_tape_dev.get();
        P.mov_P = 1;
        P.mov_M = 1;
        P.mov_pack_log2 = 0;
    }
    return P;
}

// What entry point `e` launches for this handle (navsim_select.h holds the rule)
static sel::Pick pick_for(const navsim* h, sel::Entry e) {
    return sel::pick(e, sel::Facts{h->P.N, h->P.B, h->P.S, (h->P.per_env & 1) != 0, h->P.mov_tape != nullptr,
                                   sel::sens_on(h->P.sigma, h->P.below_min_mode), h->force_epb, h->pair_cast, h->scan_pool});
}

// ---- pick -> kernel.  One resolve function per kernel signature: it spells out the instantiations that are built and answers null
// for every other pick (launch() below turns that into an error: nothing is ever launched in a missing kernel's place).  The envs
// and waves per workgroup of a resolved kernel are the pick's.

// step_kernel | steps_kernel behind one name each, so that one ladder serves both
struct StepK {
    using Fn = void (*)(StepKArgs);
    template <int NB, int EPB, bool S, int NW, bool BX, int PAIR> static Fn of() { return step_kernel<NB, EPB, S, NW, BX, PAIR>; }
    template <bool BX> static Fn mov() { return step_mov_kernel<BX>; }
    static Fn pool(bool bx) { return reinterpret_cast<Fn>(const_cast<void*>(navsim_pool::resolve(navsim_pool::kStep, bx))); }
};
struct SeqK {
    using Fn = void (*)(SeqKArgs);
    template <int NB, int EPB, bool S, int NW, bool BX, int PAIR> static Fn of() { return steps_kernel<NB, EPB, S, NW, BX, PAIR>; }
    template <bool BX> static Fn mov() { return steps_mov_kernel<BX>; }
    static Fn pool(bool bx) { return reinterpret_cast<Fn>(const_cast<void*>(navsim_pool::resolve(navsim_pool::kSteps, bx))); }
};
// the cast variants of one shape: tile boxes, 64-segment passes, 128-segment passes and (the big 10-beam shapes) their streaming form
template <class K, int NB, int EPB, int NW, bool S>
static typename K::Fn step_cast(const int cast) {
    if (cast == 3) return K::template of<NB, EPB, S, NW, true, 0>();
    if (cast == 0) return K::template of<NB, EPB, S, NW, false, 0>();
    if (cast == 1) return K::template of<NB, EPB, S, NW, false, 1>();
    if constexpr (NB == 10 && EPB >= 32)
        if (cast == 2) return K::template of<NB, EPB, S, NW, false, 2>();
    return nullptr;
}
template <class K, int NB, bool S>
static typename K::Fn step_shape(const sel::Pick& p) {
    if (p.epb == 8 && p.waves == 8) return step_cast<K, NB, 8, 8, S>(p.cast);
    if (p.epb == 16 && p.waves == 8) return step_cast<K, NB, 16, 8, S>(p.cast);
    if (p.epb == 32 && p.waves == 8) return step_cast<K, NB, 32, 8, S>(p.cast);
    if constexpr (NB == 10)   // (the 36-beam tile does not fit the LDS at 64 envs)
        if (p.epb == 64 && p.waves == 16) return step_cast<K, NB, 64, 16, S>(p.cast);
    return nullptr;
}
template <class K>   // K: StepK (navsim_step) | SeqK (navsim_step_seq)
static typename K::Fn resolve_step(const sel::Pick& p) {
    if (p.family != sel::kSmall || p.hist || sel::policy_of(p.entry) >= 0) return nullptr;
    if (p.pool > 1)   // the pooled twin: 10 columns, 16 envs on 8 waves, a shared map
        return (p.beams == 10 && p.epb == 16 && p.waves == 8 && (p.cast == 0 || p.cast == 3)) ? K::pool(p.cast == 3) : nullptr;
    if (p.mov)   // 10 beams, 16 envs on 8 waves, a shared map
        return !(p.beams == 10 && p.epb == 16 && p.waves == 8 && p.sens == kMovSens) ? nullptr
               : p.cast == 3 ? K::template mov<true>() : p.cast == 0 ? K::template mov<false>() : nullptr;
    if (p.beams == 10) return p.sens ? step_shape<K, 10, true>(p) : step_shape<K, 10, false>(p);
    if (p.beams == 36) return p.sens ? step_shape<K, 36, true>(p) : step_shape<K, 36, false>(p);
    return nullptr;
}

// the rollout_* | evaluate_* kernels of the 16-env workgroup on 8 waves behind one set of names, as StepK / SeqK
struct RolloutK {
    using Fn = void (*)(Params, RolloutArgs);
    static constexpr bool kEval = false;
    template <int NB, bool S, bool BX> static Fn mlp64() { return rollout_kernel<NB, 16, S, 8, BX>; }
    template <int EPB, bool S> static Fn narrow() { return rollout_kernel<10, EPB, S, 8>; }   // navsim_set_shape: 4 | 8 envs
    template <bool BX> static Fn mlp64_mov() { return rollout_mov_kernel<BX>; }
    template <bool S, bool BX> static Fn hist() { return rollout_hist_kernel<S, BX>; }
    template <bool BX> static Fn hist_mov() { return rollout_hist_mov_kernel<BX>; }
    template <bool S> static Fn resmlp() { return rollout_resmlp_kernel<S>; }
    static Fn resmlp_mov() { return rollout_resmlp_mov_kernel; }
    static Fn pool(bool hist, bool bx) {
        return reinterpret_cast<Fn>(const_cast<void*>(navsim_pool::resolve(hist ? navsim_pool::kRolloutHist : navsim_pool::kRollout, bx)));
    }
};
struct EvalK {
    using Fn = void (*)(Params, EvalArgs);
    static constexpr bool kEval = true;
    template <int NB, bool S, bool BX> static Fn mlp64() { return evaluate_kernel<NB, S, BX>; }
    template <bool BX> static Fn mlp64_mov() { return evaluate_mov_kernel<BX>; }
    template <bool S, bool BX> static Fn hist() { return evaluate_hist_kernel<S, BX>; }
    template <bool BX> static Fn hist_mov() { return evaluate_hist_mov_kernel<BX>; }
    template <bool S> static Fn resmlp() { return evaluate_resmlp_kernel<S>; }
    static Fn resmlp_mov() { return evaluate_resmlp_mov_kernel; }
    static Fn pool(bool hist, bool bx) {
        return reinterpret_cast<Fn>(const_cast<void*>(navsim_pool::resolve(hist ? navsim_pool::kEvaluateHist : navsim_pool::kEvaluate, bx)));
    }
};
template <class K, bool S, bool BX>
static typename K::Fn policy_fn(const sel::Pick& p) {   // the mover twins: 10 beams, one form whatever S says (kMovSens)
    switch (sel::policy_of(p.entry)) {
        case 0: return p.mov ? K::template mlp64_mov<BX>() : p.beams == 36 ? K::template mlp64<36, S, BX>() : K::template mlp64<10, S, BX>();
        case 1: return p.mov ? K::template hist_mov<BX>() : K::template hist<S, BX>();
        case 2: return BX ? nullptr : p.mov ? K::resmlp_mov() : K::template resmlp<S>();   // (64-segment passes on every map)
    }
    return nullptr;
}
template <class K>   // K: RolloutK (navsim_rollout_*, the small family) | EvalK (navsim_evaluate_*)
static typename K::Fn resolve_policy(const sel::Pick& p) {
    const int pol = sel::policy_of(p.entry);
    const bool BX = p.cast == 3, S = p.sens;
    if (pol < 0 || K::kEval != (p.entry >= sel::kEvaluateMlp64) || p.family != sel::kSmall || p.hist != (pol == 1)) return nullptr;
    if (p.waves != 8 || (p.cast != 0 && !BX)) return nullptr;
    if (p.pool > 1) return (p.beams == 10 && p.epb == 16 && pol != 2) ? K::pool(pol == 1, BX) : nullptr;
    if (p.mov ? !(p.beams == 10 && S == kMovSens) : !(p.beams == 10 || (p.beams == 36 && pol == 0))) return nullptr;
    if constexpr (!K::kEval)
        if ((p.epb == 4 || p.epb == 8) && pol == 0 && p.beams == 10 && !p.mov && !BX)
            return p.epb == 4 ? (S ? K::template narrow<4, true>() : K::template narrow<4, false>())
                              : (S ? K::template narrow<8, true>() : K::template narrow<8, false>());
    if (p.epb != 16) return nullptr;
    return BX ? (S ? policy_fn<K, true, true>(p) : policy_fn<K, false, true>(p))
              : (S ? policy_fn<K, true, false>(p) : policy_fn<K, false, false>(p));
}

// navsim_rollout_mlp64's big family: 64 envs on 16 waves with the cast variants of the step kernel, or 32 envs on 8 waves (tile
// boxes; forced: any map without the 128-segment passes); with movers a shared map, cast 0 or 3
using BigFn = void (*)(BigKArgs);
template <bool S>
static BigFn big_fn(const sel::Pick& p) {
    const bool BX = p.cast == 3;
    if (p.epb == 32 && p.waves == 8 && (p.cast == 0 || BX)) {
        if (p.mov) return BX ? rollout_big_mov_kernel<32, S, 8, true> : rollout_big_mov_kernel<32, S, 8, false>;
        return BX ? rollout_big_kernel<32, S, 8, true, 0> : rollout_big_kernel<32, S, 8, false, 0>;
    }
    if (p.epb != 64 || p.waves != 16) return nullptr;
    if (p.mov) return BX ? rollout_big_mov_kernel<64, S, 16, true> : p.cast == 0 ? rollout_big_mov_kernel<64, S, 16, false> : nullptr;
    if (BX) return rollout_big_kernel<64, S, 16, true, 0>;
    if (p.cast == 2) return rollout_big_kernel<64, S, 16, false, 2>;
    if (p.cast == 1) return rollout_big_kernel<64, S, 16, false, 1>;
    return p.cast == 0 ? rollout_big_kernel<64, S, 16, false, 0> : nullptr;
}
static BigFn resolve_big(const sel::Pick& p) {
    if (p.family != sel::kBig || p.entry != sel::kRolloutMlp64 || p.beams != 10 || p.hist || p.pool > 1) return nullptr;
    return p.sens ? big_fn<true>(p) : big_fn<false>(p);
}

// The one launch of a stepping entry point `who`: the grid covers n_envs with the pick's envs per workgroup.  A pick without a
// kernel is an error that names the pick.
template <class... A>
static int launch(const char* who, const sel::Pick& p, void (*kernel)(A...), const int n_envs, hipStream_t st, const A&... args) {
    if (p.not_built) return fail(NAVSIM_E_STATE, std::string(who) + ": " + p.not_built);
    if (!kernel) {
        char s[160];
        std::snprintf(s, sizeof(s), ": no kernel is built for the pick {%s family, %d beams, %d envs on %d waves, cast %d, sens %d, mov %d, hist %d, pool %d}",
                      p.family == sel::kBig ? "big" : "small", p.beams, p.epb, p.waves, p.cast, (int)p.sens, (int)p.mov, (int)p.hist, p.pool);
        return fail(NAVSIM_E_STATE, std::string(who) + s);
    }
    hipLaunchKernelGGL(kernel, dim3((n_envs + p.epb - 1) / p.epb), dim3(64 * p.waves), 0, st, args...);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

static int invalidate_records(navsim* h, hipStream_t st) {
    hipLaunchKernelGGL(invalidate_records_kernel, dim3((h->P.N + 255) / 256), dim3(256), 0, st, h->P.ep_step, h->P.N);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

// Uploads the start-pose table [K][3] and tabulates its half-angle (cos, sin) on the device.
static int upload_starts(navsim* h, const double* starts_host, int K, hipStream_t st) {
    (void)h->starts_dev.reset();
    (void)h->starts_sc_dev.reset();
    HIP_TRY(h->starts_dev.alloc(3 * (size_t)K));
    HIP_TRY(h->starts_sc_dev.alloc((size_t)K));
    HIP_TRY(hipMemcpy(h->starts_dev.get(), starts_host, sizeof(double) * 3 * K, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(starts_sc_kernel, dim3((K + 63) / 64), dim3(64), 0, st, h->starts_dev.get(), K, h->starts_sc_dev.get());
    HIP_TRY(hipGetLastError());
    h->P.starts = h->starts_dev.get();
    h->P.starts_sc = h->starts_sc_dev.get();
    h->P.K = K;
    return NAVSIM_OK;
}

// beam table: n samples evenly over [min_angle, max_angle] (gazebo.xacro:110-115); n = n_beams, or n_beams * scan_pool: the dense
// fan of a pooled handle IS the table of a handle with that many beams
static int upload_beam_table(navsim* h, const int n) {
    double cs[2 * 64];
    for (int i = 0; i < n; ++i) {
        const double phi = kAngleMin + (double)i * ((kAngleMax - kAngleMin) / (double)(n - 1));
        cs[i] = std::cos(phi);
        cs[n + i] = std::sin(phi);
    }
    HIP_TRY(h->beam_cs_dev.alloc(2 * (size_t)n));
    HIP_TRY(hipMemcpy(h->beam_cs_dev.get(), cs, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    h->P.beam_cs = h->beam_cs_dev.get();
    return NAVSIM_OK;
}

static const double kResetRects[4][4] = {  // environment_new.py:340-343
    {1.7, 2.3, -1.2, 1.2}, {-2.3, -1.7, -1.2, 1.2}, {-1.2, 1.2, 1.7, 2.3}, {-1.2, 1.2, -2.3, -1.7}};
static const double kRespawnRects[4][4] = {  // environment_new.py:248-251
    {1.6, 2.4, -1.4, 1.4}, {-2.4, -1.6, -1.4, 1.4}, {-1.4, 1.4, 1.6, 2.4}, {-1.4, 1.4, -2.4, -1.6}};

// Allocations and tables of a new handle (navsim_create frees the handle if any step fails).
static int init_handle(navsim* h, const navsim_cfg* cfg) {
    h->cfg = *cfg;
    const size_t N = (size_t)cfg->n_envs;
    const int B = cfg->n_beams;
    // one block: 8 f64 state arrays + 6 + 2 f64 record arrays, 2 float4, float2 past_action, 2 uint2, i32 ep_step, 2 u32
    const size_t bytes = N * (16 * sizeof(double) + 2 * sizeof(float4) + sizeof(float2) + 2 * sizeof(uint2) +
                              sizeof(int32_t) + 2 * sizeof(uint32_t));
    HIP_TRY(h->state_block.alloc(bytes));
    HIP_TRY(hipMemset(h->state_block.get(), 0, bytes));
    Params& P = h->P;
    std::memset(&P, 0, sizeof(P));
    double* d = reinterpret_cast<double*>(h->state_block.get());
    P.x = d; P.y = d + N; P.th = d + 2 * N; P.gx = d + 3 * N; P.gy = d + 4 * N;
    P.past_dist = d + 5 * N; P.ep_ret = d + 6 * N; P.ep_path = d + 7 * N;
    P.rec_g = d + 8 * N; P.rsp_g = d + 14 * N;
    P.rec_tail = reinterpret_cast<float4*>(d + 16 * N);   // 16-byte aligned: hipMalloc base + a multiple of 128 N bytes
    P.rec_ck = reinterpret_cast<uint2*>(P.rec_tail + 2 * N);
    P.past_action = reinterpret_cast<float2*>(P.rec_ck + 2 * N);
    P.ep_step = reinterpret_cast<int32_t*>(P.past_action + N);
    P.rng_ctr = reinterpret_cast<uint32_t*>(P.ep_step + N);
    P.rsp_ctr = P.rng_ctr + N;
    P.seg_pack_log2 = 6;
    P.N = cfg->n_envs;
    P.B = B;
    P.max_ep_steps = cfg->max_episode_steps;
    P.auto_reset = cfg->auto_reset;
    P.respawn = cfg->respawn_on_arrive;
    P.obs_f16 = cfg->obs_f16;
    P.below_min_mode = cfg->lidar_below_min ? 1 : 0;
    P.sigma = cfg->lidar_noise_sigma;
    P.key0 = (uint32_t)cfg->seed;
    P.key1 = (uint32_t)(cfg->seed >> 32);
    P.env_id_base = cfg->env_id_base;
    P.thr = cfg->threshold_arrive;
    P.spawn_x = cfg->spawn_x; P.spawn_y = cfg->spawn_y; P.spawn_yaw = cfg->spawn_yaw;
    P.goal_lo = cfg->goal_lo; P.goal_hi = cfg->goal_hi;
    P.diag = std::sqrt(2.0) * (3.8 + 3.8);  // environment_new.py:21

    P.pool = 1;
    {
        const int rc = upload_beam_table(h, B);
        if (rc != NAVSIM_OK) return rc;
    }

    std::memset(&h->rects_host, 0, sizeof(Rects));
    std::memcpy(h->rects_host.r[0], kResetRects, sizeof(kResetRects));
    std::memcpy(h->rects_host.r[1], kRespawnRects, sizeof(kRespawnRects));
    h->rects_host.n[0] = h->rects_host.n[1] = 4;
    HIP_TRY(h->rects_dev.alloc(1));
    HIP_TRY(hipMemcpy(h->rects_dev.get(), &h->rects_host, sizeof(Rects), hipMemcpyHostToDevice));
    P.rects = h->rects_dev.get();

    // start-pose table: K = 1, the cfg spawn pose (turtlebot3_stage_1.launch:3-5) until navsim_set_spawn_sampler
    {
        const double sp[3] = {cfg->spawn_x, cfg->spawn_y, cfg->spawn_yaw};
        const int rc = upload_starts(h, sp, 1, nullptr);
        if (rc != NAVSIM_OK) return rc;
        P.G = 0;
        P.goals = nullptr;
    }
    return NAVSIM_OK;
}

static int rebuild_spawn_scans(navsim* h, hipStream_t st);   // (below, with navsim_set_map)

#pragma GCC visibility push(default)
extern "C" {

int navsim_version(void) { return NAVSIM_ABI_VERSION; }

const char* navsim_last_error(void) { return g_err.c_str(); }

void navsim_default_cfg(navsim_cfg* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->n_envs = 1;
    c->n_beams = 10;            // gazebo.xacro:111
    c->threshold_arrive = 0.2;  // environment_new.py:45
    c->goal_lo = -3.6;          // environment_new.py:337
    c->goal_hi = 3.6;
}

int navsim_create(const navsim_cfg* cfg, navsim_t** out) {
    if (!cfg || !out) return fail(NAVSIM_E_ARG, "navsim_create: null argument");
    *out = nullptr;
    if (cfg->n_envs < 1) return fail(NAVSIM_E_ARG, "navsim_create: n_envs must be >= 1");
    if (cfg->n_beams != 10 && cfg->n_beams != 36)
        return fail(NAVSIM_E_ARG, "navsim_create: n_beams must be 10 or 36");
    if (!(cfg->goal_hi > cfg->goal_lo)) return fail(NAVSIM_E_ARG, "navsim_create: empty goal box");
    if (!(cfg->lidar_noise_sigma >= 0.f)) return fail(NAVSIM_E_ARG, "navsim_create: negative lidar_noise_sigma");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(NAVSIM_E_HIP, "navsim_create: no HIP device (there is no CPU path)");

    navsim* h = new navsim();
    const int rc = init_handle(h, cfg);
    if (rc != NAVSIM_OK) {
        delete h;   // frees whatever was allocated before the failure
        return rc;
    }
    *out = h;
    return NAVSIM_OK;
}

void navsim_destroy(navsim_t* h) { delete h; }

int navsim_set_shape(navsim_t* h, int32_t envs_per_workgroup, int32_t pair_cast) {
    if (!h) return fail(NAVSIM_E_ARG, "navsim_set_shape: null handle");
    const int v = envs_per_workgroup;
    if (!(v == 0 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) || pair_cast < -1 || pair_cast > 1)
        return fail(NAVSIM_E_ARG, "navsim_set_shape: envs_per_workgroup is 0 | 4 | 8 | 16 | 32 | 64, pair_cast -1 | 0 | 1");
    h->force_epb = v;
    h->pair_cast = pair_cast != 0;
    h->pair_cast_request = pair_cast;
    return NAVSIM_OK;
}

int navsim_set_scan_pool(navsim_t* h, int32_t k) {
    if (!h) return fail(NAVSIM_E_ARG, "navsim_set_scan_pool: null handle");
    if (k < 1 || k > sel::kMaxScanPool)
        return fail(NAVSIM_E_ARG, "navsim_set_scan_pool: scan_pool must be 1, 2, 3 or 4 (more than 4 rays per column is not built)");
    if (k > 1)
        if (const char* why = sel::scan_pool_not_built(h->P.B, (h->P.per_env & 1) != 0))
            return fail(NAVSIM_E_ARG, std::string("navsim_set_scan_pool: ") + why);
    HIP_TRY(hipDeviceSynchronize());   // launches in flight read the old beam table / spawn scans
    if (k > 1 && !h->pool_tape_dev.get()) {
        const float nan4[4] = {NAN, NAN, NAN, NAN};
        HIP_TRY(h->pool_tape_dev.alloc(1));
        HIP_TRY(hipMemcpy(h->pool_tape_dev.get(), nan4, sizeof(nan4), hipMemcpyHostToDevice));
    }
    // k, the beam table and the spawn rows change together: a step that fails puts the old k back with its tables, so that no launch
    // ever reads rows of another stride than its k
    auto apply = [h](const int kk) -> int {
        h->scan_pool = kk;
        h->P.pool = kk;
        const int rc = upload_beam_table(h, h->P.B * kk);   // the dense fan (k = 1: the table of a fresh handle)
        if (rc != NAVSIM_OK) return rc;
        if (h->has_map) {   // the cached spawn scans: the raw hits of the new fan
            const int rs = rebuild_spawn_scans(h, nullptr);
            if (rs != NAVSIM_OK) return rs;
            HIP_TRY(hipDeviceSynchronize());
        }
        return NAVSIM_OK;
    };
    const int old = h->scan_pool;
    const int rc = apply(k);
    if (rc != NAVSIM_OK && old != k) {
        const std::string why = g_err;
        (void)apply(old);
        g_err = why;
    }
    return rc;
}

int navsim_get_info(navsim_t* h, navsim_info* out) {
    if (!h || !out) return fail(NAVSIM_E_ARG, "navsim_get_info: null argument");
    std::memset(out, 0, sizeof(*out));
    out->abi_version = NAVSIM_ABI_VERSION;
    out->n_envs = h->P.N; out->n_beams = h->P.B; out->obs_f16 = h->P.obs_f16;
    out->n_segments = h->P.S; out->per_env_map = h->P.per_env & 1; out->tile_boxes = h->P.tile_box != nullptr;
    out->has_map = h->has_map;
    out->forced_epb = h->force_epb; out->forced_pair_cast = h->pair_cast_request;
    out->reserved[0] = h->scan_pool;
    if (h->has_map) {
        const sel::Pick a = pick_for(h, sel::kStep), b = pick_for(h, sel::kStepSeq), r = pick_for(h, sel::kRolloutMlp64);
        out->step_epb = a.epb; out->step_waves = a.waves; out->step_cast = a.cast;
        out->seq_epb = b.epb; out->seq_waves = b.waves; out->seq_cast = b.cast;
        out->rollout_kind = r.not_built ? 0 : (r.family == sel::kBig ? 2 : 1);
        out->rollout_epb = r.epb; out->rollout_waves = r.waves; out->rollout_cast = r.cast;
        // the resources (registers, scratch = spilled registers, LDS) of what the rule picks: the run-time check that it fits the
        // way the rule assumes
        hipFuncAttributes fa;
        std::memset(&fa, 0, sizeof(fa));
        if (const auto k = resolve_step<StepK>(a)) (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k));
        out->step_vgprs = fa.numRegs; out->step_scratch_bytes = (int32_t)fa.localSizeBytes; out->step_lds_bytes = (int32_t)fa.sharedSizeBytes;
        std::memset(&fa, 0, sizeof(fa));
        if (const auto k = resolve_step<SeqK>(b)) (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k));
        out->seq_vgprs = fa.numRegs; out->seq_scratch_bytes = (int32_t)fa.localSizeBytes; out->seq_lds_bytes = (int32_t)fa.sharedSizeBytes;
    }
    return NAVSIM_OK;
}

int navsim_set_goal_rects(navsim_t* h, int32_t which, const double* rects_host, int32_t n_rects) {
    if (!h || (which != 0 && which != 1) || n_rects < 0 || n_rects > kMaxRects || (n_rects && !rects_host))
        return fail(NAVSIM_E_ARG, "navsim_set_goal_rects: bad argument");
    HIP_TRY(hipDeviceSynchronize());
    std::memcpy(h->rects_host.r[which], rects_host, sizeof(double) * 4 * n_rects);
    h->rects_host.n[which] = n_rects;
    HIP_TRY(hipMemcpy(h->rects_dev.get(), &h->rects_host, sizeof(Rects), hipMemcpyHostToDevice));
    const int rc = invalidate_records(h, nullptr);
    if (rc != NAVSIM_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return NAVSIM_OK;
}

// the pooled handle's reset / ray-cast kernels (navsim_pool.hip), under the signatures of reset_kernel / raycast_kernel
using ResetFn = void (*)(Params, const uint8_t*, void*);
using RaycastFn = void (*)(Params, const double*, int, int, int, int, float*);
static ResetFn pool_reset_kernel() { return reinterpret_cast<ResetFn>(const_cast<void*>(navsim_pool::resolve(navsim_pool::kReset, false))); }
static RaycastFn pool_raycast_kernel() { return reinterpret_cast<RaycastFn>(const_cast<void*>(navsim_pool::resolve(navsim_pool::kRaycast, false))); }

static int rebuild_spawn_scans(navsim* h, hipStream_t st) {
    Params& P = h->P;
    P.spawn_per_env = (P.per_env || (P.mov_tape && (P.mov_phase0 || P.mov_bp))) ? 1 : 0;   // movers with phase offsets or tape ids: every env resets into its own row
    const size_t n_poses = (size_t)(P.spawn_per_env ? P.N : 1) * P.K;
    const size_t n_rays = (size_t)P.B * (size_t)P.pool;   // entries of a row: on a pooled handle the raw hits of the dense fan
    if (h->spawn_scan_dev.get()) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(h->spawn_scan_dev.reset());
        HIP_TRY(h->spawn_obs_dev.reset());
    }
    HIP_TRY(h->spawn_scan_dev.alloc(n_poses * n_rays));
    P.spawn_scan = h->spawn_scan_dev.get();
    P.spawn_obs = nullptr;
    if (P.pool == 1) {   // (the pooled twins are sensor-options kernels: they read the raw hits, never the noise-free entries)
        HIP_TRY(h->spawn_obs_dev.alloc(n_poses * n_rays));
        P.spawn_obs = h->spawn_obs_dev.get();
    }
    const RaycastFn cast = P.pool > 1 ? pool_raycast_kernel() : raycast_kernel;
    hipLaunchKernelGGL(cast, dim3((unsigned)((n_poses + 63) / 64)), dim3(64), 0, st, P, h->starts_dev.get(), P.K, 1, (int)n_poses, 1,
                       h->spawn_scan_dev.get());
    if (P.pool == 1)
        hipLaunchKernelGGL(spawn_obs_kernel, dim3((unsigned)((n_poses * n_rays + 255) / 256)), dim3(256), 0, st, h->spawn_scan_dev.get(),
                           (int)(n_poses * n_rays), P.below_min_mode, h->spawn_obs_dev.get());
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

int navsim_set_map(navsim_t* h, const float* seg_dev, int32_t n_segments, int32_t per_env, void* stream) {
    if (!h || !seg_dev || n_segments < 1) return fail(NAVSIM_E_ARG, "navsim_set_map: bad argument");
    if (h->P.mov_tape && per_env)
        return fail(NAVSIM_E_ARG, "navsim_set_map: movers are set and " + std::string(sel::kMoversNotBuilt));
    if (h->scan_pool > 1 && per_env)
        return fail(NAVSIM_E_ARG, "navsim_set_map: scan_pool is set and " + std::string(sel::kPoolPerEnvNotBuilt));
    Params& P = h->P;
    P.seg = reinterpret_cast<const float4*>(seg_dev);
    P.S = n_segments;
    const sel::MapFacts mf = sel::map_facts(P.N, n_segments, per_env != 0);   // the bits of per_env, tile boxes or not, the packing
    P.per_env = mf.per_env;
    P.seg_pack_log2 = mf.seg_pack_log2;
    P.tile_box = nullptr;
    if (h->seg_sorted_dev.get() || h->tile_box_dev.get()) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        (void)h->seg_sorted_dev.reset();
        (void)h->tile_box_dev.reset();
    }
    if (mf.tile_boxes) {
        // A shared map big enough to tile: keep an own copy in Morton order of the segment midpoints, so that a 64-segment
        // tile is a compact patch of the map, with the bounding box of every tile.  The order of the segments does not
        // change the scan (the nearest hit is a min).
        const int S = n_segments, nt = (S + 63) / 64;
        std::vector<float4> seg((size_t)S);
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        HIP_TRY(hipMemcpy(seg.data(), seg_dev, sizeof(float4) * S, hipMemcpyDeviceToHost));
        float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
        for (const float4& g : seg) {
            const float mx = 0.5f * (g.x + g.z), my = 0.5f * (g.y + g.w);
            if (std::isfinite(mx) && std::isfinite(my)) {
                lo[0] = std::fmin(lo[0], mx); hi[0] = std::fmax(hi[0], mx);
                lo[1] = std::fmin(lo[1], my); hi[1] = std::fmax(hi[1], my);
            }
        }
        auto spread = [](uint32_t v) {   // 16 bits -> every other bit
            v &= 0xFFFFu;
            v = (v | (v << 8)) & 0x00FF00FFu; v = (v | (v << 4)) & 0x0F0F0F0Fu;
            v = (v | (v << 2)) & 0x33333333u; v = (v | (v << 1)) & 0x55555555u;
            return v;
        };
        std::vector<std::pair<uint32_t, int>> key((size_t)S);
        for (int j = 0; j < S; ++j) {
            const float mx = 0.5f * (seg[j].x + seg[j].z), my = 0.5f * (seg[j].y + seg[j].w);
            uint32_t code = 0xFFFFFFFFu;   // non-finite segments go last
            if (std::isfinite(mx) && std::isfinite(my)) {
                const float sx = (hi[0] > lo[0]) ? (mx - lo[0]) / (hi[0] - lo[0]) : 0.f;
                const float sy = (hi[1] > lo[1]) ? (my - lo[1]) / (hi[1] - lo[1]) : 0.f;
                code = spread((uint32_t)(sx * 65535.f)) | (spread((uint32_t)(sy * 65535.f)) << 1);
            }
            key[j] = {code, j};
        }
        std::sort(key.begin(), key.end());
        std::vector<float4> sorted((size_t)S), box((size_t)nt);
        for (int j = 0; j < S; ++j) sorted[j] = seg[key[j].second];
        for (int t = 0; t < nt; ++t) {
            // NaN coordinates make the box NaN-free but that segment can never be hit either (every test on it fails)
            float4 b = make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY);
            for (int j = 64 * t; j < std::min(S, 64 * t + 64); ++j) {
                const float4 g = sorted[j];
                b.x = std::fmin(b.x, std::fmin(g.x, g.z)); b.y = std::fmin(b.y, std::fmin(g.y, g.w));
                b.z = std::fmax(b.z, std::fmax(g.x, g.z)); b.w = std::fmax(b.w, std::fmax(g.y, g.w));
            }
            box[t] = b;
        }
        HIP_TRY(h->seg_sorted_dev.alloc((size_t)S));
        HIP_TRY(h->tile_box_dev.alloc((size_t)nt));
        HIP_TRY(hipMemcpy(h->seg_sorted_dev.get(), sorted.data(), sizeof(float4) * S, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->tile_box_dev.get(), box.data(), sizeof(float4) * nt, hipMemcpyHostToDevice));
        P.seg = h->seg_sorted_dev.get();
        P.tile_box = h->tile_box_dev.get();
    }
    const int rc = rebuild_spawn_scans(h, (hipStream_t)stream);
    if (rc != NAVSIM_OK) return rc;
    h->has_map = true;
    return NAVSIM_OK;
}

// The one implementation behind navsim_set_movers (K = 1, no ids, no rectangles) and navsim_set_mover_bank: every check comes
// before the first change of the handle.  `fn` names the entry point in the messages.
static int set_mover_bank_impl(navsim* h, const char* fn, const float* bank_dev, int32_t K, int32_t Pmax, int32_t M,
                               const int32_t* period_host, const int32_t* tape_id_dev, const int32_t* phase0_dev,
                               const double* rects_host, int32_t n_rects, hipStream_t st) {
    Params& P = h->P;
    const std::string pre = std::string(fn) + ": ";
    HIP_TRY(hipStreamSynchronize(st));   // launches in flight read the old tape / phase offsets
    std::vector<int32_t> ph0, tid;
    std::vector<uint2> bp;
    if (bank_dev) {
        for (int k = 0; k < K; ++k)
            if (period_host[k] < 1 || period_host[k] > Pmax) return fail(NAVSIM_E_ARG, pre + "a period lies outside [1, max_period]");
        if (tape_id_dev) {
            tid.resize((size_t)P.N);
            HIP_TRY(hipMemcpy(tid.data(), tape_id_dev, sizeof(int32_t) * P.N, hipMemcpyDeviceToHost));
            for (const int32_t v : tid)
                if (v < 0 || v >= K) return fail(NAVSIM_E_ARG, pre + "a tape id lies outside [0, n_tapes)");
        }
        if (phase0_dev) {
            ph0.resize((size_t)P.N);
            HIP_TRY(hipMemcpy(ph0.data(), phase0_dev, sizeof(int32_t) * P.N, hipMemcpyDeviceToHost));
            for (int i = 0; i < P.N; ++i)
                if (ph0[i] < 0 || ph0[i] >= period_host[tid.empty() ? 0 : tid[i]])
                    return fail(NAVSIM_E_ARG, pre + "a phase0 value lies outside [0, period)");
        }
        if (!tid.empty()) {
            bp.resize((size_t)P.N);
            for (int i = 0; i < P.N; ++i) bp[i] = make_uint2((uint32_t)tid[i] * (uint32_t)Pmax, (uint32_t)period_host[tid[i]]);
        }
    }
    const bool had_rects = P.mov_rects != nullptr;
    (void)h->mov_phase0_dev.reset();
    (void)h->mov_bp_dev.reset();
    (void)h->mov_tid_dev.reset();
    (void)h->mov_rects_dev.reset();
    P.mov_tape = nullptr;
    P.mov_phase0 = nullptr;
    P.mov_bp = nullptr;
    P.mov_tid = nullptr;
    P.mov_rects = nullptr;
    P.mov_P = P.mov_M = P.mov_pack_log2 = P.mov_n_rects = 0;
    if (bank_dev) {
        if (!ph0.empty()) {
            HIP_TRY(h->mov_phase0_dev.alloc((size_t)P.N));
            HIP_TRY(hipMemcpy(h->mov_phase0_dev.get(), ph0.data(), sizeof(int32_t) * P.N, hipMemcpyHostToDevice));
        }
        if (!tid.empty()) {
            HIP_TRY(h->mov_tid_dev.alloc((size_t)P.N));
            HIP_TRY(hipMemcpy(h->mov_tid_dev.get(), tid.data(), sizeof(int32_t) * P.N, hipMemcpyHostToDevice));
            HIP_TRY(h->mov_bp_dev.alloc((size_t)P.N));
            HIP_TRY(hipMemcpy(h->mov_bp_dev.get(), bp.data(), sizeof(uint2) * P.N, hipMemcpyHostToDevice));
        }
        if (rects_host && n_rects > 0) {
            HIP_TRY(h->mov_rects_dev.alloc(4 * (size_t)n_rects * (size_t)K));
            HIP_TRY(hipMemcpy(h->mov_rects_dev.get(), rects_host, sizeof(double) * 4 * (size_t)n_rects * (size_t)K, hipMemcpyHostToDevice));
            P.mov_rects = h->mov_rects_dev.get();
            P.mov_n_rects = n_rects;
        }
        P.mov_tape = reinterpret_cast<const float4*>(bank_dev);
        P.mov_phase0 = h->mov_phase0_dev.get();
        P.mov_bp = h->mov_bp_dev.get();
        P.mov_tid = h->mov_tid_dev.get();
        P.mov_P = period_host[0];
        P.mov_M = M;
        int lg = 0;
        while ((1 << lg) < M) ++lg;
        P.mov_pack_log2 = lg;
    }
    // per-tape goal rectangles came or went: the cached next-episode records hold goals drawn under the old ones
    if (had_rects || P.mov_rects) {
        const int rc = invalidate_records(h, st);
        if (rc != NAVSIM_OK) return rc;
    }
    // the reset observation sees bank[t][phase0[i]]: the spawn tables (and with them the cached next-episode records' scan rows,
    // which are read through the tables at every step) are rebuilt for the new world
    return rebuild_spawn_scans(h, st);
}

int navsim_set_movers(navsim_t* h, const float* tape_dev, int32_t period, int32_t n_segments, const int32_t* phase0_dev,
                      void* stream) {
    if (!h) return fail(NAVSIM_E_ARG, "navsim_set_movers: null handle");
    if (!h->has_map) return fail(NAVSIM_E_STATE, "navsim_set_movers: call navsim_set_map first");
    if (tape_dev) {
        if (period < 1 || period > 65536 || n_segments < 1 || n_segments > 64)
            return fail(NAVSIM_E_ARG, "navsim_set_movers: 1 <= period <= 65536 and 1 <= n_segments <= 64");
        if ((uintptr_t)tape_dev & 15) return fail(NAVSIM_E_ARG, "navsim_set_movers: the tape must be 16-byte aligned");
        if (const char* why = sel::movers_not_built(h->P.B, (h->P.per_env & 1) != 0)) return fail(NAVSIM_E_ARG, std::string("navsim_set_movers: ") + why);
    }
    // the bank with one tape, ids 0 and no rectangles
    return set_mover_bank_impl(h, "navsim_set_movers", tape_dev, 1, period, n_segments, &period, nullptr, phase0_dev, nullptr, 0,
                               (hipStream_t)stream);
}

int navsim_set_mover_bank(navsim_t* h, const float* bank_dev, int32_t n_tapes, int32_t max_period, int32_t n_segments,
                          const int32_t* period_host, const int32_t* tape_id_dev, const int32_t* phase0_dev,
                          const double* goal_rects_host, int32_t n_rects, void* stream) {
    if (!h) return fail(NAVSIM_E_ARG, "navsim_set_mover_bank: null handle");
    if (!h->has_map) return fail(NAVSIM_E_STATE, "navsim_set_mover_bank: call navsim_set_map first");
    if (bank_dev) {
        if (n_tapes < 1 || max_period < 1 || max_period > 65536 || n_segments < 1 || n_segments > 64 ||
            (int64_t)n_tapes * (int64_t)max_period > ((int64_t)1 << 24))
            return fail(NAVSIM_E_ARG, "navsim_set_mover_bank: 1 <= n_tapes, 1 <= max_period <= 65536, n_tapes * max_period <= 2^24 "
                                      "and 1 <= n_segments <= 64");
        if (!period_host) return fail(NAVSIM_E_ARG, "navsim_set_mover_bank: the periods are missing");
        if ((uintptr_t)bank_dev & 15) return fail(NAVSIM_E_ARG, "navsim_set_mover_bank: the bank must be 16-byte aligned");
        if (n_rects < 0 || n_rects > 8) return fail(NAVSIM_E_ARG, "navsim_set_mover_bank: 0 <= n_rects <= 8");
        if (n_rects > 0 && !goal_rects_host) return fail(NAVSIM_E_ARG, "navsim_set_mover_bank: n_rects > 0 without rectangles");
        if (const char* why = sel::movers_not_built(h->P.B, (h->P.per_env & 1) != 0)) return fail(NAVSIM_E_ARG, std::string("navsim_set_mover_bank: ") + why);
    }
    return set_mover_bank_impl(h, "navsim_set_mover_bank", bank_dev, n_tapes, max_period, n_segments, period_host, tape_id_dev,
                               phase0_dev, goal_rects_host, n_rects, (hipStream_t)stream);
}

int navsim_set_spawn_sampler(navsim_t* h, const double* starts_host, int32_t n_starts, const double* goals_host,
                             int32_t n_goals, double min_dist, double max_dist, void* stream) {
    if (!h || !starts_host || n_starts < 1 || n_goals < 0 || (n_goals > 0 && !goals_host) || !(max_dist >= min_dist))
        return fail(NAVSIM_E_ARG, "navsim_set_spawn_sampler: bad argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(st));
    Params& P = h->P;
    (void)h->goals_dev.reset();
    {
        const int rc = upload_starts(h, starts_host, n_starts, st);
        if (rc != NAVSIM_OK) return rc;
    }
    if (n_goals > 0) {
        HIP_TRY(h->goals_dev.alloc(2 * (size_t)n_goals));
        HIP_TRY(hipMemcpy(h->goals_dev.get(), goals_host, sizeof(double) * 2 * n_goals, hipMemcpyHostToDevice));
    }
    P.goals = h->goals_dev.get();
    P.G = n_goals;
    P.min_dist = min_dist;
    P.max_dist = max_dist;
    {
        const int rc = invalidate_records(h, st);
        if (rc != NAVSIM_OK) return rc;
    }
    if (h->has_map) return rebuild_spawn_scans(h, st);
    return NAVSIM_OK;
}

int navsim_reset(navsim_t* h, const uint8_t* mask_dev, void* obs_dev, void* stream) {
    if (!h || !obs_dev) return fail(NAVSIM_E_ARG, "navsim_reset: bad argument");
    if (!h->has_map) return fail(NAVSIM_E_STATE, "navsim_reset: call navsim_set_map first");
    const ResetFn reset = h->scan_pool > 1 ? pool_reset_kernel() : reset_kernel;
    hipLaunchKernelGGL(reset, dim3((h->P.N + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->P, mask_dev, obs_dev);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

int navsim_step(navsim_t* h, const float* action_dev, const float* past_action_dev, void* obs_dev,
                float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, void* stream) {
    if (!h || !action_dev || !obs_dev || !reward_dev || !done_dev || !arrive_dev)
        return fail(NAVSIM_E_ARG, "navsim_step: null required buffer");
    if (!h->has_map) return fail(NAVSIM_E_STATE, "navsim_step: call navsim_set_map first");
    const StepKArgs ka = {launch_params(h), StepIO{(const float2*)action_dev, (const float2*)past_action_dev, obs_dev, reward_dev, done_dev,
                                       arrive_dev, ended_dev, ep_return_dev, ep_length_dev, ep_path_dev}};
    const sel::Pick p = pick_for(h, sel::kStep);
    return launch("navsim_step", p, resolve_step<StepK>(p), h->P.N, (hipStream_t)stream, ka);
}

// The one body of the three rollout entry points: what they check before anything is launched, the RolloutArgs they pass, the
// pick of entry point `e` and its launch.  NAVSIM_OK with n_steps == 0: nothing to launch.
static int rollout_entry(const sel::Entry e, const char* fn, const navsim* h, const float* params, void* obs_buf, float* act_buf,
                         float* logp_buf, float* reward, uint8_t* done, uint8_t* arrive, uint8_t* ended, float* ep_return,
                         int32_t* ep_length, float* ep_path, const float* var, uint64_t seed, const uint32_t* step_base,
                         int32_t n_steps, void* stream, const float* hist_in = nullptr, float* hist_out = nullptr) {
    const std::string f = std::string(fn) + ": ";
    if (!h || !params || !obs_buf || !act_buf || !logp_buf || !reward || !done || !arrive || !ended || !var || n_steps < 0)
        return fail(NAVSIM_E_ARG, f + "bad argument");
    if (((uintptr_t)hist_in & 15) || ((uintptr_t)hist_out & 15)) return fail(NAVSIM_E_ARG, f + "the history carries must be 16-byte aligned");
    if (n_steps == 0 && hist_out && hist_out != hist_in)
        return fail(NAVSIM_E_ARG, f + "n_steps == 0 leaves no row to write a carry for (pass hist_out = hist_in, or none)");
    if (!h->has_map) return fail(NAVSIM_E_STATE, f + "call navsim_set_map first");
    if (const char* why = sel::beams_not_built(e, h->P.B)) return fail(NAVSIM_E_ARG, f + why);
    if (((uintptr_t)params & 15) || ((uintptr_t)act_buf & 7) || ((uintptr_t)obs_buf & 15))
        return fail(NAVSIM_E_ARG, f + "params and obs must be 16-byte, act 8-byte aligned");
    if (n_steps == 0) return NAVSIM_OK;
    const RolloutArgs R = {params, obs_buf, act_buf, logp_buf, reward, done, arrive, ended, ep_return, ep_length, ep_path, var,
                           step_base, seed, n_steps, hist_in, hist_out};
    const sel::Pick p = pick_for(h, e);
    if (p.family == sel::kBig) {
        const BigKArgs ka = {h->P, R, rollout_io(R, (size_t)h->P.N, (size_t)h->P.B + 6, 0, h->P.obs_f16 != 0)};
        return launch(fn, p, resolve_big(p), h->P.N, (hipStream_t)stream, ka);
    }
    return launch(fn, p, resolve_policy<RolloutK>(p), h->P.N, (hipStream_t)stream, launch_params(h), R);
}

int navsim_rollout_mlp64(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev,
                         float* logp_buf_dev, float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                         float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev,
                         uint64_t act_seed, const uint32_t* step_base_dev, int32_t n_steps, void* stream) {
    return rollout_entry(sel::kRolloutMlp64, "navsim_rollout_mlp64", h, actor_params_dev, obs_buf_dev, act_buf_dev, logp_buf_dev,
                         reward_dev, done_dev, arrive_dev, ended_dev, ep_return_dev, ep_length_dev, ep_path_dev, var_dev, act_seed,
                         step_base_dev, n_steps, stream);
}

int navsim_rollout_mlp64_hist(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev,
                              float* logp_buf_dev, float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                              float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev,
                              uint64_t act_seed, const uint32_t* step_base_dev, int32_t n_steps, void* stream) {
    return rollout_entry(sel::kRolloutMlp64Hist, "navsim_rollout_mlp64_hist", h, actor_params_dev, obs_buf_dev, act_buf_dev,
                         logp_buf_dev, reward_dev, done_dev, arrive_dev, ended_dev, ep_return_dev, ep_length_dev, ep_path_dev, var_dev,
                         act_seed, step_base_dev, n_steps, stream);
}

int navsim_rollout_mlp64_hist_cont(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev,
                                   float* logp_buf_dev, float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev,
                                   float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev,
                                   uint64_t act_seed, const uint32_t* step_base_dev, int32_t n_steps, const float* hist_in_dev,
                                   float* hist_out_dev, void* stream) {
    return rollout_entry(sel::kRolloutMlp64Hist, "navsim_rollout_mlp64_hist_cont", h, actor_params_dev, obs_buf_dev, act_buf_dev,
                         logp_buf_dev, reward_dev, done_dev, arrive_dev, ended_dev, ep_return_dev, ep_length_dev, ep_path_dev, var_dev,
                         act_seed, step_base_dev, n_steps, stream, hist_in_dev, hist_out_dev);
}

int navsim_rollout_resmlp512(navsim_t* h, const float* actor_params_dev, void* obs_buf_dev, float* act_buf_dev, float* logp_buf_dev,
                             float* reward_dev, uint8_t* done_dev, uint8_t* arrive_dev, uint8_t* ended_dev, float* ep_return_dev,
                             int32_t* ep_length_dev, float* ep_path_dev, const float* var_dev, uint64_t act_seed,
                             const uint32_t* step_base_dev, int32_t n_steps, void* stream) {
    return rollout_entry(sel::kRolloutResmlp512, "navsim_rollout_resmlp512", h, actor_params_dev, obs_buf_dev, act_buf_dev,
                         logp_buf_dev, reward_dev, done_dev, arrive_dev, ended_dev, ep_return_dev, ep_length_dev, ep_path_dev, var_dev,
                         act_seed, step_base_dev, n_steps, stream);
}

// The one body of the three evaluation entry points, as rollout_entry
static int evaluate_entry(const sel::Entry e, const char* fn, const navsim* h, const float* params, const void* obs0, int32_t quota,
                          int32_t n_steps, uint8_t* flags, int32_t* length, float* ret, float* path, int32_t* count, int32_t* steps,
                          void* stream) {
    const std::string f = std::string(fn) + ": ";
    if (!h) return fail(NAVSIM_E_ARG, f + "null handle");
    if (!params || !obs0 || !flags || !length || !ret || !path || !count || !steps) return fail(NAVSIM_E_ARG, f + "null pointer");
    if (quota < 1) return fail(NAVSIM_E_ARG, f + "quota must be at least 1");
    if (n_steps < 1) return fail(NAVSIM_E_ARG, f + "n_steps must be at least 1");
    if (!h->P.auto_reset) return fail(NAVSIM_E_ARG, f + "the handle needs auto_reset (an env plays its episodes back to back)");
    if (h->P.max_ep_steps <= 0) return fail(NAVSIM_E_ARG, f + "max_episode_steps == 0: an episode could never end");
    if (h->P.N > 16 * 256)
        return fail(NAVSIM_E_ARG, f + "more than 4096 envs (only the 16-env workgroup shape has an evaluation form)");
    if (const char* why = sel::beams_not_built(e, h->P.B)) return fail(NAVSIM_E_ARG, f + why);
    if (((uintptr_t)params & 15) || ((uintptr_t)obs0 & 15)) return fail(NAVSIM_E_ARG, f + "params and obs0 must be 16-byte aligned");
    if (((uintptr_t)length & 3) || ((uintptr_t)ret & 3) || ((uintptr_t)path & 3) || ((uintptr_t)count & 3) || ((uintptr_t)steps & 3))
        return fail(NAVSIM_E_ARG, f + "ep_length, ep_return, ep_path, count and steps must be 4-byte aligned");
    if (!h->has_map) return fail(NAVSIM_E_STATE, f + "call navsim_set_map first");
    const EvalArgs R = {params, obs0, flags, length, ret, path, count, steps, quota, n_steps};
    const sel::Pick p = pick_for(h, e);
    return launch(fn, p, resolve_policy<EvalK>(p), h->P.N, (hipStream_t)stream, launch_params(h), R);
}

int navsim_evaluate_mlp64(navsim_t* h, const float* actor_params_dev, const void* obs0_dev, int32_t quota, int32_t n_steps,
                          uint8_t* ep_flags_dev, int32_t* ep_length_dev, float* ep_return_dev, float* ep_path_dev,
                          int32_t* count_dev, int32_t* steps_dev, void* stream) {
    return evaluate_entry(sel::kEvaluateMlp64, "navsim_evaluate_mlp64", h, actor_params_dev, obs0_dev, quota, n_steps, ep_flags_dev,
                          ep_length_dev, ep_return_dev, ep_path_dev, count_dev, steps_dev, stream);
}

int navsim_evaluate_mlp64_hist(navsim_t* h, const float* actor_params_dev, const void* obs0_dev, int32_t quota, int32_t n_steps,
                               uint8_t* ep_flags_dev, int32_t* ep_length_dev, float* ep_return_dev, float* ep_path_dev,
                               int32_t* count_dev, int32_t* steps_dev, void* stream) {
    return evaluate_entry(sel::kEvaluateMlp64Hist, "navsim_evaluate_mlp64_hist", h, actor_params_dev, obs0_dev, quota, n_steps,
                          ep_flags_dev, ep_length_dev, ep_return_dev, ep_path_dev, count_dev, steps_dev, stream);
}

int navsim_evaluate_resmlp512(navsim_t* h, const float* actor_params_dev, const void* obs0_dev, int32_t quota, int32_t n_steps,
                              uint8_t* ep_flags_dev, int32_t* ep_length_dev, float* ep_return_dev, float* ep_path_dev,
                              int32_t* count_dev, int32_t* steps_dev, void* stream) {
    return evaluate_entry(sel::kEvaluateResmlp512, "navsim_evaluate_resmlp512", h, actor_params_dev, obs0_dev, quota, n_steps,
                          ep_flags_dev, ep_length_dev, ep_return_dev, ep_path_dev, count_dev, steps_dev, stream);
}

int navsim_step_seq(navsim_t* h, const float* actions_dev, int32_t n_steps, void* obs_dev, float* reward_dev, uint8_t* done_dev,
                    uint8_t* arrive_dev, uint8_t* ended_dev, float* ep_return_dev, int32_t* ep_length_dev, float* ep_path_dev,
                    void* stream) {
    if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev || !arrive_dev || n_steps < 0)
        return fail(NAVSIM_E_ARG, "navsim_step_seq: bad argument");
    if (!h->has_map) return fail(NAVSIM_E_STATE, "navsim_step_seq: call navsim_set_map first");
    if ((uintptr_t)actions_dev & 7) return fail(NAVSIM_E_ARG, "navsim_step_seq: actions must be 8-byte aligned");
    if (n_steps == 0) return NAVSIM_OK;
    SeqArgs R;
    R.io = StepIO{reinterpret_cast<const float2*>(actions_dev), nullptr, obs_dev, reward_dev, done_dev, arrive_dev, ended_dev,
                  ep_return_dev, ep_length_dev, ep_path_dev};
    R.T = n_steps;
    const SeqKArgs ka = {launch_params(h), R};
    const sel::Pick p = pick_for(h, sel::kStepSeq);
    return launch("navsim_step_seq", p, resolve_step<SeqK>(p), h->P.N, (hipStream_t)stream, ka);
}

int navsim_odometry(int32_t n, const double* x_dev, const double* y_dev, const double* quat_dev, const double* goal_dev,
                    double* out_dev, void* stream) {
    if (n < 0 || (n > 0 && (!x_dev || !y_dev || !quat_dev || !goal_dev || !out_dev)))
        return fail(NAVSIM_E_ARG, "navsim_odometry: bad argument");
    if (n == 0) return NAVSIM_OK;
    hipLaunchKernelGGL(odometry_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, x_dev, y_dev, quat_dev,
                       goal_dev, out_dev);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

int navsim_raycast(navsim_t* h, const double* pose_dev, float* ranges_dev, void* stream) {
    if (!h || !pose_dev || !ranges_dev) return fail(NAVSIM_E_ARG, "navsim_raycast: bad argument");
    if (!h->has_map) return fail(NAVSIM_E_STATE, "navsim_raycast: call navsim_set_map first");
    const RaycastFn cast = h->scan_pool > 1 ? pool_raycast_kernel() : raycast_kernel;
    hipLaunchKernelGGL(cast, dim3((h->P.N + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->P, pose_dev, 1, 0, h->P.N, 0, ranges_dev);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

int navsim_get_state(navsim_t* h, double* pose, double* goal, double* past_dist, float* past_action,
                     int32_t* ep_step, uint32_t* rng_ctr, void* stream) {
    if (!h) return fail(NAVSIM_E_ARG, "navsim_get_state: null handle");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const size_t N = (size_t)h->P.N;
    const Params& P = h->P;
    if (pose) {
        std::vector<double> tmp(3 * N);
        HIP_TRY(hipMemcpy(tmp.data(), P.x, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));  // x,y,th are adjacent
        for (size_t i = 0; i < N; ++i) {
            pose[3 * i] = tmp[i];
            pose[3 * i + 1] = tmp[N + i];
            pose[3 * i + 2] = tmp[2 * N + i];
        }
    }
    if (goal) {
        std::vector<double> tmp(2 * N);
        HIP_TRY(hipMemcpy(tmp.data(), P.gx, sizeof(double) * 2 * N, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; ++i) {
            goal[2 * i] = tmp[i];
            goal[2 * i + 1] = tmp[N + i];
        }
    }
    if (past_dist) HIP_TRY(hipMemcpy(past_dist, P.past_dist, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (past_action) HIP_TRY(hipMemcpy(past_action, P.past_action, sizeof(float2) * N, hipMemcpyDeviceToHost));
    if (ep_step) {
        HIP_TRY(hipMemcpy(ep_step, P.ep_step, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; ++i) ep_step[i] = (int32_t)((uint32_t)ep_step[i] & kStepMask);
    }
    if (rng_ctr) HIP_TRY(hipMemcpy(rng_ctr, P.rng_ctr, sizeof(uint32_t) * N, hipMemcpyDeviceToHost));
    return NAVSIM_OK;
}

int navsim_set_state(navsim_t* h, const double* pose, const double* goal, const double* past_dist,
                     const float* past_action, const int32_t* ep_step, const uint32_t* rng_ctr, void* stream) {
    if (!h) return fail(NAVSIM_E_ARG, "navsim_set_state: null handle");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const size_t N = (size_t)h->P.N;
    const Params& P = h->P;
    if (pose) {
        std::vector<double> tmp(3 * N);
        for (size_t i = 0; i < N; ++i) {
            tmp[i] = pose[3 * i];
            tmp[N + i] = pose[3 * i + 1];
            tmp[2 * N + i] = pose[3 * i + 2];
        }
        HIP_TRY(hipMemcpy(P.x, tmp.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    }
    if (goal) {
        std::vector<double> tmp(2 * N);
        for (size_t i = 0; i < N; ++i) {
            tmp[i] = goal[2 * i];
            tmp[N + i] = goal[2 * i + 1];
        }
        HIP_TRY(hipMemcpy(P.gx, tmp.data(), sizeof(double) * 2 * N, hipMemcpyHostToDevice));
    }
    if (past_dist) HIP_TRY(hipMemcpy(P.past_dist, past_dist, sizeof(double) * N, hipMemcpyHostToDevice));
    if (past_action) HIP_TRY(hipMemcpy(P.past_action, past_action, sizeof(float2) * N, hipMemcpyHostToDevice));
    if (ep_step) HIP_TRY(hipMemcpy(P.ep_step, ep_step, sizeof(int32_t) * N, hipMemcpyHostToDevice));
    if (rng_ctr) HIP_TRY(hipMemcpy(P.rng_ctr, rng_ctr, sizeof(uint32_t) * N, hipMemcpyHostToDevice));
    if (rng_ctr && !ep_step) {   // the goal stream moved: the cached next-episode records are stale (ep_step clears the flag itself)
        const int rc = invalidate_records(h, (hipStream_t)stream);
        if (rc != NAVSIM_OK) return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    }
    return NAVSIM_OK;
}

int navsim_rtg_scan(const float* rew_dev, const uint8_t* ended_dev, int32_t T, int32_t N, double gamma,
                    float* out_dev, int32_t exact, void* stream) {
    if (T < 0 || N < 0) return fail(NAVSIM_E_ARG, "navsim_rtg_scan: negative size");
    if (T == 0 || N == 0) return NAVSIM_OK;  // empty batch: nothing to scan (pointers may be null)
    if (!rew_dev || !ended_dev || !out_dev) return fail(NAVSIM_E_ARG, "navsim_rtg_scan: null buffer");
    if (N % kRtgCols == 0 && !exact)
        hipLaunchKernelGGL(rtg_kernel_split<false>, dim3(N / kRtgCols), dim3(256), 0, (hipStream_t)stream, rew_dev, ended_dev, T, N, gamma,
                           out_dev, (const float*)nullptr, (const float*)nullptr, 1.0, (float*)nullptr);
    else
        hipLaunchKernelGGL(rtg_kernel_generic, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, rew_dev, ended_dev, T, N,
                           gamma, out_dev);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

int navsim_gae_scan(const float* rew_dev, const uint8_t* ended_dev, const float* value_dev, const float* last_value_dev, int32_t T,
                    int32_t N, double gamma, double lam, float* adv_dev, float* ret_dev, int32_t exact, void* stream) {
    if (T < 0 || N < 0) return fail(NAVSIM_E_ARG, "navsim_gae_scan: negative size");
    if (T == 0 || N == 0) return NAVSIM_OK;
    if (!rew_dev || !ended_dev || !value_dev || !adv_dev) return fail(NAVSIM_E_ARG, "navsim_gae_scan: null buffer");
    if (!(lam >= 0.0 && lam <= 1.0)) return fail(NAVSIM_E_ARG, "navsim_gae_scan: lambda outside [0, 1]");
    if (N % kRtgCols == 0 && !exact)
        hipLaunchKernelGGL(rtg_kernel_split<true>, dim3(N / kRtgCols), dim3(256), 0, (hipStream_t)stream, rew_dev, ended_dev, T, N, gamma,
                           ret_dev, value_dev, last_value_dev, lam, adv_dev);
    else
        hipLaunchKernelGGL(gae_kernel_generic, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, rew_dev, ended_dev, value_dev,
                           last_value_dev, T, N, gamma, lam, adv_dev, ret_dev);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

int navsim_gae_scan_trunc(const float* rew_dev, const uint8_t* ended_dev, const uint8_t* done_dev, const uint8_t* arrive_dev,
                          const float* value_dev, const float* last_value_dev, int32_t T, int32_t N, double gamma, double lam,
                          float* adv_dev, float* ret_dev, int32_t exact, void* stream) {
    if (T < 0 || N < 0) return fail(NAVSIM_E_ARG, "navsim_gae_scan_trunc: negative size");
    if (T == 0 || N == 0) return NAVSIM_OK;
    if (!rew_dev || !ended_dev || !done_dev || !arrive_dev || !value_dev || !adv_dev)
        return fail(NAVSIM_E_ARG, "navsim_gae_scan_trunc: null buffer");
    if (!(lam >= 0.0 && lam <= 1.0)) return fail(NAVSIM_E_ARG, "navsim_gae_scan_trunc: lambda outside [0, 1]");
    if (N % kRtgCols == 0 && !exact)
        hipLaunchKernelGGL((rtg_kernel_split<true, true>), dim3(N / kRtgCols), dim3(256), 0, (hipStream_t)stream, rew_dev, ended_dev, T, N,
                           gamma, ret_dev, value_dev, last_value_dev, lam, adv_dev, done_dev, arrive_dev);
    else
        hipLaunchKernelGGL(gae_trunc_kernel_generic, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, rew_dev, ended_dev, done_dev,
                           arrive_dev, value_dev, last_value_dev, T, N, gamma, lam, adv_dev, ret_dev);
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

// The one body of navsim_stack_rows and navsim_stack_rows_cont
static int stack_rows_entry(const char* fn, const void* obs_dev, int32_t obs_f16, const uint8_t* ended_dev, int32_t R, int32_t N,
                            void* out_dev, const float* carry_in, float* carry_out, void* stream) {
    const std::string f = std::string(fn) + ": ";
    if (R < 1 || N < 1) return fail(NAVSIM_E_ARG, f + "R and N must be at least 1");
    if (!obs_dev || !out_dev) return fail(NAVSIM_E_ARG, f + "null buffer");
    if (R > 1 && !ended_dev) return fail(NAVSIM_E_ARG, f + "ended_dev may be null only when R == 1");
    if (((uintptr_t)obs_dev & 15) || ((uintptr_t)out_dev & 15))
        return fail(NAVSIM_E_ARG, f + "obs_dev and out_dev must be 16-byte aligned");
    if (((uintptr_t)carry_in & 15) || ((uintptr_t)carry_out & 15)) return fail(NAVSIM_E_ARG, f + "the carries must be 16-byte aligned");
    if (carry_out && (int64_t)N * kHistLen > 0x7fffffffll) return fail(NAVSIM_E_ARG, f + "too many envs for a carry");
    const size_t total = (size_t)R * (size_t)N * (size_t)kHistD;
    const size_t per = obs_f16 ? 8 : 4;
    const size_t blocks = ((total + per - 1) / per + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(NAVSIM_E_ARG, f + "too many rows for one launch");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), cgrid((unsigned)(((size_t)N * kHistLen + 255) / 256));
    const size_t last = (size_t)(R - 1) * (size_t)N * (size_t)kHistD;
    if (obs_f16) {
        const __half* obs = reinterpret_cast<const __half*>(obs_dev);
        __half* out = reinterpret_cast<__half*>(out_dev);
        if (carry_in) hipLaunchKernelGGL(HIP_KERNEL_NAME(stack_rows_kernel<__half, true>), grid, dim3(256), 0, st, obs, ended_dev, R, N, out, carry_in);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(stack_rows_kernel<__half, false>), grid, dim3(256), 0, st, obs, ended_dev, R, N, out, nullptr);
        HIP_TRY(hipGetLastError());
        if (carry_out) hipLaunchKernelGGL(stack_rows_carry_kernel<__half>, cgrid, dim3(256), 0, st, out + last, N, carry_out);
    } else {
        const float* obs = reinterpret_cast<const float*>(obs_dev);
        float* out = reinterpret_cast<float*>(out_dev);
        if (carry_in) hipLaunchKernelGGL(HIP_KERNEL_NAME(stack_rows_kernel<float, true>), grid, dim3(256), 0, st, obs, ended_dev, R, N, out, carry_in);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(stack_rows_kernel<float, false>), grid, dim3(256), 0, st, obs, ended_dev, R, N, out, nullptr);
        HIP_TRY(hipGetLastError());
        if (carry_out) hipLaunchKernelGGL(stack_rows_carry_kernel<float>, cgrid, dim3(256), 0, st, out + last, N, carry_out);
    }
    HIP_TRY(hipGetLastError());
    return NAVSIM_OK;
}

int navsim_stack_rows(const void* obs_dev, int32_t obs_f16, const uint8_t* ended_dev, int32_t R, int32_t N, void* out_dev,
                      void* stream) {
    return stack_rows_entry("navsim_stack_rows", obs_dev, obs_f16, ended_dev, R, N, out_dev, nullptr, nullptr, stream);
}

int navsim_stack_rows_cont(const void* obs_dev, int32_t obs_f16, const uint8_t* ended_dev, int32_t R, int32_t N, void* out_dev,
                           const float* carry_in_dev, float* carry_out_dev, void* stream) {
    return stack_rows_entry("navsim_stack_rows_cont", obs_dev, obs_f16, ended_dev, R, N, out_dev, carry_in_dev, carry_out_dev, stream);
}

}  // extern "C"
#pragma GCC visibility pop
#endif   // NAVSIM_POOL_TU
