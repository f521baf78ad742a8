// Which instantiation of the step body runs for a handle: the whole rule, as host C++ without a HIP header (g++ compiles this file
// alone: tests/test_kernel_select_cpu.py enumerates it against a table).  navsim.hip builds the Facts of a handle, asks pick() and
// maps the Pick to a kernel pointer (its resolve_* functions, which spell out every instantiation that is built); nothing else in
// the host side decides a shape.
#pragma once
#include <cstddef>
#include <cstdint>

namespace navsim_select {

// ---------------------------------------------------------------- what navsim_set_map derives from a map
struct MapFacts {
    int per_env;         // Params::per_env: bit 0 = every env has its own map, bits 1 and 2 below
    bool tile_boxes;     // a shared map big enough to tile: Morton-ordered copy + the bounding box of every 64-segment tile
    int seg_pack_log2;   // maps of up to 32 segments: several envs share one 64-lane pass of the cast
};
inline MapFacts map_facts(int n_envs, int n_segments, bool per_env) {
    MapFacts m = {per_env ? 1 : 0, false, 6};
    const size_t stream = (size_t)n_envs * (size_t)n_segments * 16;   // the per-env segment stream of one step (N x S x 16 B)
    // bit 1: the per-env segment stream of one step (N x S x 16 B) exceeds 1.25 x the 256 MiB Infinity Cache -> the persistent
    // kernels load it non-temporally too (the PAIR == 2 instantiations)
    if (per_env && stream >= (size_t)320 << 20) m.per_env |= 2;
    // bit 2: it does not fit the 8 x 4 MiB of L2 -> the one-launch-per-step kernel loads it non-temporally
    if (per_env && stream >= (size_t)32 << 20) m.per_env |= 4;
    m.tile_boxes = !per_env && n_segments > 64 && n_segments <= 4096;
    if (n_segments <= 32) {   // several envs share one 64-lane pass of the cast
        int lg = 0;
        while ((1 << lg) < n_segments) ++lg;
        m.seg_pack_log2 = lg;
    }
    return m;
}

// ---------------------------------------------------------------- the facts the rule reads
struct Facts {
    int n_envs, n_beams, n_segments;
    bool per_env;     // navsim_set_map: every env has its own map
    bool movers;      // navsim_set_movers / navsim_set_mover_bank: a tape is set
    bool sens;        // sens_on()
    int force_epb;    // navsim_set_shape: envs per workgroup, 0 = the rule of pick_epb
    bool pair_cast;   // navsim_set_shape: false = 64-segment passes for every map
    int scan_pool = 1;   // navsim_set_scan_pool: rays per scan column (sector LiDAR); 1 = off
};

// The SENS flag of a handle's instantiations: the sensor-fidelity options (range noise, -inf below range_min) are on
inline bool sens_on(float sigma, int below_min_mode) { return sigma > 0.f || below_min_mode != 0; }

// The 16-env mover twins (step_mov_kernel ... evaluate_resmlp_mov_kernel) exist in ONE form, built with the sensor options' code: a
// handle without the options runs it and gets the same bits.  (The big mover twins, rollout_big_mov_kernel, exist in both forms.)
constexpr bool kMovTwinsSens = true;

// what navsim_set_movers (and a navsim_set_map behind it) refuses; the same sentence stands in include/navsim.h.  (What IS built
// beside the 16-env twins: the big shapes of navsim_rollout_mlp64, rollout_big_mov_kernel; every other stepping entry point keeps 16
// envs on 8 waves whatever navsim_set_shape says.)
constexpr const char* kMoversNotBuilt =
    "movers need 10 beams and a shared static map: movers with 36 beams or with a per-env static map are not built";
inline const char* movers_not_built(int n_beams, bool per_env) { return (n_beams != 10 || per_env) ? kMoversNotBuilt : nullptr; }

// Sector LiDAR (navsim_set_scan_pool, k > 1): the pooled twins of navsim_pool.hip exist in ONE form -- 10 scan columns, 16 envs on 8
// waves, a shared static map, the mover and sensor-options code compiled in (a handle without a tape or without the options runs it
// and gets the same bits), 64-segment passes or tile boxes -- for navsim_step, navsim_step_seq and the two mlp64 policies' rollouts and
// evaluations.  The sentences of the refusals; the same stand in include/navsim.h.
constexpr int kMaxScanPool = 4;
constexpr const char* kPoolBeamsNotBuilt = "scan_pool > 1 needs n_beams == 10: pooling a 36-beam scan is not built";
constexpr const char* kPoolPerEnvNotBuilt = "scan_pool > 1 needs a shared static map: pooling over per-env maps is not built";
constexpr const char* kPoolResmlpNotBuilt = "scan_pool > 1 with the 512-wide nets is not built (the pooled twins carry the mlp64 policies)";
inline const char* scan_pool_not_built(int n_beams, bool per_env) {
    return n_beams != 10 ? kPoolBeamsNotBuilt : per_env ? kPoolPerEnvNotBuilt : nullptr;
}

// The stepping entry points of the C ABI (policy_of() reads the order: step, step_seq, then the three policies twice)
enum Entry {
    kStep, kStepSeq,
    kRolloutMlp64, kRolloutMlp64Hist, kRolloutResmlp512,
    kEvaluateMlp64, kEvaluateMlp64Hist, kEvaluateResmlp512,
};

// null: the entry point's policy has an instantiation for this beam count; else the message of the refusal
inline const char* beams_not_built(Entry e, int n_beams) {
    if (e == kRolloutMlp64Hist || e == kEvaluateMlp64Hist)
        return n_beams == 10 ? nullptr : "the scan-history policy stacks 10-beam scans (n_beams must be 10)";
    if (e == kRolloutResmlp512 || e == kEvaluateResmlp512)
        return n_beams == 10 ? nullptr : "the reference's nets read 16-wide observations (10 beams)";
    if (n_beams == 10 || n_beams == 36) return nullptr;
    return (e == kStep || e == kStepSeq) ? "n_beams must be 10 or 36" : "the (B + 6)-64-64 policy needs 10 or 36 beams";
}

// Envs per workgroup.  Bigger workgroups make the float64 lanes of the geometry / rules phases denser (a wave instruction
// costs the same with 16 or 64 active lanes) and start fewer workgroups, but need N / EPB >= the number of CUs to fill the
// chip: measured (tools/time_step.py) 16384 envs: 18.5 / 16.7 / 15.9 us with 16 / 32 / 64; 8192: 69.8 / 64.8 / 73.9; 4096: 8.9 / 8.6 / 9.8.
// Round 4 swept shard size x shape x beam count on shared maps (tools/epb_sweep.py, profiles/r04_epb_sweep.txt), us per step,
// shapes 8 / 16 / 32:
//   36 beams, tape form    1024 envs 6.3 / 10.0 / 9.9   2048: 6.5 / 10.1 / 9.8   4096: 7.0 / 10.2 / 9.9   8192: 13.0 / 11.0 / 10.0
//   36 beams, one launch   1024: 10.5 / 12.9 / 12.7     2048: 11.0 / 13.1 / 12.9  4096: 11.9 / 13.5 / 13.1  8192: 13.9 / 14.6 / 13.5
//   10 beams, tape form    1024:  4.45 / 5.06 / 4.72    2048: 4.49 / 5.09 / 4.70  4096: 4.94 / 5.27 / 4.81
//   10 beams, one launch   1024:  8.6 / 7.6 / 7.2       2048: 8.8 / 7.8 / 7.3     4096: 9.2 / 8.0 / 7.6
// With 36 beams a workgroup's chain is long (36 beam directions per env in the pose phase, stage B per beam group) and eight envs
// on four waves, two to four workgroups per CU, overlap their chains: up to 4096 envs the 8-env shape; small 10-beam shards take it
// in the tape form only (a launch per step pays for 4 x as many workgroups to start) and the 32-env shape otherwise.
// The 36-beam 8-env shape then went from four to eight waves (one env's beam groups per wave; min_waves_per_simd keeps two
// workgroups on a CU): tape form 1024 / 2048 / 4096 envs 6.3 / 6.5 / 7.0 -> 5.2 / 5.4 / 6.3 us per step, a launch per step
// unchanged (10.4 / 11.0 / 12.0); with 10 beams eight waves gain 2-3 % at 1024-2048 envs and nothing at 4096: four stay.
// The same on the shared 2048-segment house map (tile boxes; EPB_MAP=house): 8 / 32 envs per workgroup, tape form 1024-4096 envs
// 18.5-20.2 / 29.1-29.8 us per step, 8192: 25.0 / 30.7; one launch per step 1024-4096: 20.8-22.6 / 31.3-32.2, 8192: 38.2 / 32.6;
// 16384 envs: the 64-env shape (35 / 37 us) ahead of every smaller one.
// Per-env stage_2 maps (EPB_MAP=per_env), 8 / 32: tape 1024-2048 envs 5.6 / 7.2, 4096: 6.2 / 7.3, 8192: 11.5 / 7.7; a launch per step 9.2-10.2 / 9.2-9.4.
// Waves of the 8-env workgroup.  Eight (one env per wave) halve each wave's cast chain: on the house map (tile boxes) the tape runs
// 18.4 / 18.7 / 20.2 -> 12.1 / 12.6 / 15.0 us per step at 1024 / 2048 / 4096 envs and a launch per step 20.7 / 21.2 / 22.4 -> 14.8 /
// 15.4 / 18.0; per-env stage_2 maps as a tape 5.5 / 5.6 / 6.1 -> 4.6 / 4.7 / 5.6; 36 beams see the comment above.  Two such
// workgroups fit a CU (128 VGPRs each: min_waves_per_simd), so beyond 4096 envs the shape runs in rounds and is not chosen.
// The 16-env workgroup went from four to eight waves the same way (two envs per wave; us per step, the rule before / 16 envs on eight waves):
//   stage_1, 10 beams, tape form   1024: 4.30 / 3.90   2048: 4.36 / 3.91   4096: 4.80 / 4.09   8192: 4.97 / 4.97   (a launch per step: equal)
//   per-env maps, a launch per step 1024: 9.13 / 7.86   2048: 9.24 / 8.18   4096: 9.42 / 8.47   8192: 10.5 / 10.0   (tape: the 8-env shape stays)
//   36 beams, a launch per step    1024: 10.3 / 9.3    2048: 11.0 / 9.7    4096: 12.1 / 10.1   8192: 13.6 / 11.8   16384: 25.0 / 21.3
//   house map, tape form           8192: 24.6 (8 envs on four waves) / 23.6 -- the last user of a four-wave shape, which is gone
// With the 128-VGPR bound on the 16-env instantiations that need it (min_waves_per_simd), the rule before / 16 envs: 36 beams, tape
// 8192: 9.95 / 8.16   16384: 19.7 / 16.0; house map, a launch per step 8192: 32.7 / 25.8; per-env maps, tape 8192: 7.58 / 6.89;
// stage_1, a launch per step 1024: 7.17 / 6.77   4096: 7.59 / 7.23   8192: 7.96 / 8.00.
inline int pick_epb(int force_epb, int n_envs, int n_beams, bool tape, bool boxes, bool per_env) {
    if (force_epb >= 8) return force_epb;
    if (n_beams > 16) return (tape && n_envs <= 4096) ? 8 : (n_envs <= 16384 ? 16 : 32);
    if (boxes && n_envs <= 8192) return n_envs <= 4096 ? 8 : 16;
    if (per_env && tape && n_envs <= 8192) return n_envs <= 4096 ? 8 : 16;
    if (per_env && !tape && n_envs <= 8192) return 16;
    if (n_envs >= 16384) return 64;
    if (!boxes && !per_env && n_envs <= 4096) return 16;
    return 32;
}

// ---------------------------------------------------------------- the pick
enum Family {
    kSmall,   // the step body in a workgroup of the step kernels' making: step / steps / rollout / evaluate kernels and their twins
    kBig,     // rollout_big_kernel / rollout_big_mov_kernel (navsim_rollout_mlp64 beyond 4096 envs)
};

// What one entry point launches for one handle.  `cast` is already the variant that exists for the shape: 0 = 64-segment passes
// (PAIR 0), 1 / 2 = 128-segment passes (PAIR 1 / 2), 3 = tile boxes (BOXES).  `not_built` non-null: there is no such kernel, and why.
struct Pick {
    Entry entry;
    const char* not_built;
    Family family;
    int beams, epb, waves, cast;
    bool sens, mov, hist;   // the SENS, MOV and HIST template flags
    int pool = 1;           // > 1: the pooled twin (navsim_pool.hip) casts 10 * pool rays; sens and mov are then its one form's (true)
};

// The instantiation navsim_step (tape = false) / navsim_step_seq (tape = true) launches for this handle: envs and waves per
// workgroup and the cast variant -- 0 = 64-segment passes, 1 = 128-segment passes (maps of 65+ segments without tile boxes:
// per-env maps, shared maps beyond 4096 segments), 2 = the same with non-temporal loads (the stream does not fit the caches,
// navsim_set_map; exists for the big 10-beam shapes), 3 = tile bounding boxes (shared maps of 65..4096 segments).
inline void pick_shape(const Facts& f, const MapFacts& m, bool tape, Pick& sp) {
    const int NB = f.n_beams;
    const bool boxes = m.tile_boxes;
    sp.epb = 16, sp.waves = 8, sp.cast = boxes ? 3 : 0;
    if (f.movers) return;   // movers: the one shape that has the MOV form (navsim_set_movers)
    const int want = pick_epb(f.force_epb, f.n_envs, NB, tape, boxes, m.per_env != 0);
    if (want == 8) sp.epb = 8, sp.waves = 8;                                    // eight waves: one env per wave
    else if (want == 32 || (want == 64 && NB > 10)) sp.epb = 32, sp.waves = 8;  // float64 geometry / rules lanes twice as dense
    else if (want == 64) sp.epb = 64, sp.waves = 16;                            // (10 beams: the 36-beam tile does not fit the LDS)
    else sp.epb = 16, sp.waves = 8;                                             // two envs per wave
    const bool pair = f.pair_cast && !boxes && f.n_segments > 64 && m.seg_pack_log2 == 6;
    const bool nt = (m.per_env & (tape ? 2 : 4)) != 0;   // navsim_set_map: the per-env stream does not fit the L2s / the Infinity Cache
    sp.cast = boxes ? 3 : (pair ? ((nt && NB == 10 && sp.epb >= 32) ? 2 : 1) : 0);
}

// navsim_rollout_mlp64's kernel for this handle: kSmall = rollout_kernel (EPB envs on 8 waves, any beam
// count), kBig = rollout_big_kernel (64 envs on 16 waves, 10 beams, the cast variants of the step kernel).
// A 16-env workgroup is ONE latency chain per step whatever its size: measured (tools/time_rollout.py, 512 steps) 4096 / 2048 /
// 1024 / 512 envs take 2.92 / 2.90 / 2.89 / 2.97 ms with 16 envs per workgroup, 3.05-3.06 ms with 8 and 2.96 ms with 4 wherever the
// grid still fits one round of 256 CUs (a second round doubles the time: 256 registers x 8 waves fill a CU) -- spreading a small
// shard over more CUs buys nothing.  Beyond 4096 envs (10 beams): the tape kernel's 64-env workgroup with the policy phase inside
// every step -- the 16-env shape needs a second round of workgroups there (measured, us per step, 16-env / 64-env shape: 4608 envs
// 10.6 / 7.3, 8192 10.5 / 7.4, 12288 15.5 / 7.4, 16384 20.5 / 7.6; 4096: 5.3 / 7.5), while a 64-env workgroup costs the same
// 7.3-7.6 us whether 72 or 256 CUs hold one.  36 beams: the 16-env shape at every size (the 64-env tile does not fit the LDS).
inline void pick_rollout(const Facts& f, const MapFacts& m, Pick& rp) {
    const bool boxes = m.tile_boxes;
    const bool pair = f.pair_cast && !boxes && f.n_segments > 64 && m.seg_pack_log2 == 6;
    // movers: rollout_big_mov_kernel under the same rule (the tape needs a shared map: cast 0 or 3), else rollout_mov_kernel.
    // Measured (profiles/movers_big_rollout.txt; orbit_movers M = 32, 512 steps, ms per rollout, the 16-env twin / the big twin):
    // stage_1 8192 envs 6.66 / 5.25, 16384 envs 13.29 / 5.30; the 2048-segment house map (tile boxes, 32 envs on 8 waves) 8192 envs
    // 17.36 / 14.95 -- each far outside the spread of the blocks (0.01-0.06 ms), so the rule is the one without movers.
    if (f.n_beams == 10 && (f.force_epb == 64 || f.force_epb == 32 || (f.force_epb == 0 && f.n_envs > 16 * 256))) {
        rp.family = kBig; rp.epb = 64; rp.waves = 16;
        // tile-box maps (the 2048-segment house map: a vector-issue-bound cast) on 4097..8192 envs: 64-env workgroups would leave half
        // the CUs empty (8192 envs: 35.4 us per step) -- 32 envs on 8 waves, one workgroup on every CU
        if (f.force_epb == 32 || (f.force_epb == 0 && boxes && f.n_envs <= 32 * 256)) rp.epb = 32, rp.waves = 8;
        rp.cast = boxes ? 3 : (pair ? ((m.per_env & 2) ? 2 : 1) : 0);   // 2: one step's per-env stream exceeds 1.25 x the Infinity Cache
        if ((rp.epb == 32 || f.movers) && rp.cast != 3) rp.cast = 0;   // (the forced 32-env shape, and every shape with movers, exists with 64-segment passes and with tile boxes)
        return;
    }
    rp.family = kSmall; rp.waves = 8;
    rp.cast = boxes ? 3 : 0;   // (round 5: the 16-env shape has the tile-box cast too -- the house map on shards up to 4096 envs)
    // (movers: the 16-env shape is the only small one with the MOV form)
    rp.epb = (!f.movers && f.n_beams == 10 && !boxes && (f.force_epb == 4 || f.force_epb == 8)) ? f.force_epb : 16;
}

// 0 = the (B + 6)-64-64 policy, 1 = the scan-history policy, 2 = the 512-wide nets; -1 = no policy (navsim_step, navsim_step_seq)
inline int policy_of(Entry e) { return e < kRolloutMlp64 ? -1 : (e - kRolloutMlp64) % 3; }

inline Pick pick(Entry e, const Facts& f) {
    Pick p = {e, nullptr, kSmall, f.n_beams, 0, 0, 0, f.sens, f.movers, policy_of(e) == 1};
    if ((p.not_built = beams_not_built(e, f.n_beams))) return p;
    if (f.movers && (p.not_built = movers_not_built(f.n_beams, f.per_env))) return p;
    const MapFacts m = map_facts(f.n_envs, f.n_segments, f.per_env);
    if (f.scan_pool > 1) {
        // the one pooled shape at every shard size and whatever navsim_set_shape says: beyond 4096 envs the workgroups run in rounds
        p.pool = f.scan_pool;
        if ((p.not_built = scan_pool_not_built(f.n_beams, f.per_env))) return p;
        if (policy_of(e) == 2) p.not_built = kPoolResmlpNotBuilt;
        p.epb = 16; p.waves = 8; p.cast = m.tile_boxes ? 3 : 0;
        p.sens = true; p.mov = true;
        return p;
    }
    if (e == kStep || e == kStepSeq) pick_shape(f, m, e == kStepSeq, p);
    else if (e == kRolloutMlp64) pick_rollout(f, m, p);
    else {
        // always 16 envs on 8 waves, whatever navsim_set_shape says: beyond 4096 envs the workgroups run in rounds.  (The 512-wide
        // nets' kernels cast in 64-segment passes on every map.)
        p.epb = 16; p.waves = 8;
        p.cast = (m.tile_boxes && policy_of(e) != 2) ? 3 : 0;
    }
    if (p.mov && p.family == kSmall) p.sens = kMovTwinsSens;
    return p;
}

}  // namespace navsim_select
