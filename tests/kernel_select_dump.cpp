// Prints what navsim_select.h picks over a grid of handles: one line per handle, the facts, what navsim_set_map derives and the
// pick of each of the eight stepping entry points (family:envs:waves:cast:sens:mov:hist, or `-` where nothing is built).
//     kernel_select_dump full    every row of the grid
//     kernel_select_dump table   every 19th row (tests/kernel_select_table.txt; 19 shares no factor with any axis of the grid, so
//                                every value of every axis, the boundaries among them, is in the table many times)
// tests/test_kernel_select_cpu.py compiles this file with g++ (no HIP header is involved) and compares the output.
#include <cstdio>
#include <cstring>

#include "navsim_select.h"

namespace sel = navsim_select;

static void print_pick(const sel::Pick& p) {
    if (p.not_built) std::printf(" -");
    else std::printf(" %d:%d:%d:%d:%d:%d:%d", (int)p.family, p.epb, p.waves, p.cast, (int)p.sens, (int)p.mov, (int)p.hist);
}

int main(int argc, char** argv) {
    const bool full = argc > 1 && !std::strcmp(argv[1], "full");
    if (!full && !(argc > 1 && !std::strcmp(argv[1], "table"))) return 2;
    const int envs[] = {1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193, 16383, 16384, 65536};
    const int beams[] = {10, 36};
    const struct { int S; bool per_env; } maps[] = {{8, false}, {32, false}, {33, false}, {64, false}, {65, false}, {2048, false},
                                                    {4096, false}, {4097, false}, {64, true}, {128, true}, {1536, true}};
    const int forced[] = {0, 4, 8, 16, 32, 64};
    const sel::Entry entries[] = {sel::kStep, sel::kStepSeq, sel::kRolloutMlp64, sel::kRolloutMlp64Hist, sel::kRolloutResmlp512,
                                  sel::kEvaluateMlp64, sel::kEvaluateMlp64Hist, sel::kEvaluateResmlp512};
    long row = 0;
    for (const int N : envs)
        for (const int B : beams)
            for (const auto& m : maps)
                for (int mov = 0; mov < 2; ++mov) {
                    if (mov && sel::movers_not_built(B, m.per_env)) continue;   // navsim_set_movers refuses these handles
                    for (int sens = 0; sens < 2; ++sens)
                        for (const int fe : forced)
                            for (int pc = 0; pc < 2; ++pc) {
                                if (!full && row++ % 19) continue;
                                const sel::Facts f = {N, B, m.S, m.per_env, mov != 0, sens != 0, fe, pc != 0};
                                const sel::MapFacts mf = sel::map_facts(N, m.S, m.per_env);
                                std::printf("%d %d %d %d %d %d %d %d | %d %d %d |", N, B, m.S, (int)m.per_env, mov, sens, fe, pc, mf.per_env,
                                            (int)mf.tile_boxes, mf.seg_pack_log2);
                                for (const sel::Entry e : entries) print_pick(sel::pick(e, f));
                                std::printf("\n");
                            }
                }
    return 0;
}
