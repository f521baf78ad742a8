// Prints what navsim_select.h picks for handles with scan_pool set (sector LiDAR): the companion of kernel_select_dump.cpp.
//     kernel_select_pool_dump k1     the rows of `kernel_select_dump table` with Facts::scan_pool spelt out as 1: the same text
//     kernel_select_pool_dump pool   scan_pool 2..4 over envs x beams x maps x movers x sensor options x forced shapes: one line per
//                                    handle, the facts and the pick of each of the eight stepping entry points
//                                    (family:envs:waves:cast:sens:mov:hist:pool, or `-` and the reason where nothing is built)
// tests/test_scan_pool_cpu.py compiles this file with g++ (no HIP header is involved) and reads the output.
#include <cstdio>
#include <cstring>

#include "navsim_select.h"

namespace sel = navsim_select;

static const int kEnvs[] = {1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193, 16383, 16384, 65536};
static const int kBeams[] = {10, 36};
static const struct { int S; bool per_env; } kMaps[] = {{8, false}, {32, false}, {33, false}, {64, false}, {65, false}, {2048, false},
                                                        {4096, false}, {4097, false}, {64, true}, {128, true}, {1536, true}};
static const int kForced[] = {0, 4, 8, 16, 32, 64};
static const sel::Entry kEntries[] = {sel::kStep, sel::kStepSeq, sel::kRolloutMlp64, sel::kRolloutMlp64Hist, sel::kRolloutResmlp512,
                                      sel::kEvaluateMlp64, sel::kEvaluateMlp64Hist, sel::kEvaluateResmlp512};

static void k1_rows() {   // kernel_select_dump.cpp's `table`, through a Facts whose scan_pool is written out
    long row = 0;
    for (const int N : kEnvs)
        for (const int B : kBeams)
            for (const auto& m : kMaps)
                for (int mov = 0; mov < 2; ++mov) {
                    if (mov && sel::movers_not_built(B, m.per_env)) continue;
                    for (int sens = 0; sens < 2; ++sens)
                        for (const int fe : kForced)
                            for (int pc = 0; pc < 2; ++pc) {
                                if (row++ % 19) continue;
                                sel::Facts f = {N, B, m.S, m.per_env, mov != 0, sens != 0, fe, pc != 0};
                                f.scan_pool = 1;
                                const sel::MapFacts mf = sel::map_facts(N, m.S, m.per_env);
                                std::printf("%d %d %d %d %d %d %d %d | %d %d %d |", N, B, m.S, (int)m.per_env, mov, sens, fe, pc, mf.per_env,
                                            (int)mf.tile_boxes, mf.seg_pack_log2);
                                for (const sel::Entry e : kEntries) {
                                    const sel::Pick p = sel::pick(e, f);
                                    if (p.not_built || p.pool != 1) std::printf(" -");
                                    else std::printf(" %d:%d:%d:%d:%d:%d:%d", (int)p.family, p.epb, p.waves, p.cast, (int)p.sens, (int)p.mov, (int)p.hist);
                                }
                                std::printf("\n");
                            }
                }
}

static void pool_rows() {
    for (int k = 2; k <= sel::kMaxScanPool; ++k)
        for (const int N : kEnvs)
            for (const int B : kBeams)
                for (const auto& m : kMaps)
                    for (int mov = 0; mov < 2; ++mov) {
                        if (mov && sel::movers_not_built(B, m.per_env)) continue;
                        for (int sens = 0; sens < 2; ++sens)
                            for (const int fe : kForced) {
                                sel::Facts f = {N, B, m.S, m.per_env, mov != 0, sens != 0, fe, true};
                                f.scan_pool = k;
                                const sel::MapFacts mf = sel::map_facts(N, m.S, m.per_env);
                                std::printf("%d %d %d %d %d %d %d %d %d |", k, N, B, m.S, (int)m.per_env, mov, sens, fe, (int)mf.tile_boxes);
                                for (const sel::Entry e : kEntries) {
                                    const sel::Pick p = sel::pick(e, f);
                                    if (p.not_built) std::printf(" -%s;", p.not_built);
                                    else std::printf(" %d:%d:%d:%d:%d:%d:%d:%d;", (int)p.family, p.epb, p.waves, p.cast, (int)p.sens, (int)p.mov,
                                                     (int)p.hist, p.pool);
                                }
                                std::printf("\n");
                            }
                    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "k1")) k1_rows();
    else if (argc > 1 && !std::strcmp(argv[1], "pool")) pool_rows();
    else return 2;
    return 0;
}
