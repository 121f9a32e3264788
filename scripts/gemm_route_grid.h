// The grid of dense launches over which the routing function (s2d_amd/csrc/gemm_route.h) is compared with the dispatcher it replaced
// (profiles/gemm_route/parity.txt) and run under sanitizers (scripts/gemm_route_main.cpp).  A launch is described as
// s2d_gemm_route_describe takes it: GEMM_D_COUNT integers and GEMM_F_* flag bits.
#pragma once
#include <vector>

#include "gemm_route_describe.h"

// one switch at one non-default value at a time (index into GemmSwitches' member order, value); entry 0: all defaults
struct GemmSwitchSetting { int index, value; };
static const GemmSwitchSetting GEMM_SWITCH_SETTINGS[] = {
    {-1, 0}, {0, 0}, {0, 2}, {1, 0}, {2, 1}, {2, 2}, {3, 0}, {3, 1}, {4, 0}, {5, 0}, {6, 0}, {6, 2}, {7, 2}, {7, 4}, {8, 0}, {8, 2}, {9, 0}, {10, 1}, {11, 0}, {12, 16},
};
constexpr int GEMM_SWITCH_SETTING_COUNT = sizeof(GEMM_SWITCH_SETTINGS) / sizeof(GEMM_SWITCH_SETTINGS[0]);

inline void gemm_switch_setting(int i, int *switches)
{
    const GemmSwitches d;
    const int dflt[GEMM_SWITCH_COUNT] = {d.rows, d.small, d.ws, d.hi, d.hi_pre, d.pipe, d.w128, d.wm, d.halo, d.halo64, d.halo_pipe, d.stem, d.stem_ph};
    for (int k = 0; k < GEMM_SWITCH_COUNT; ++k) switches[k] = dflt[k];
    if (GEMM_SWITCH_SETTINGS[i].index >= 0) switches[GEMM_SWITCH_SETTINGS[i].index] = GEMM_SWITCH_SETTINGS[i].value;
}

// emit(const long launch[GEMM_D_COUNT], int flags) for every launch of the grid; returns their number
template <class F>
long gemm_route_grid(F emit)
{
    struct Shape { long M, N, K, Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad; bool conv; };
    std::vector<Shape> shapes;
    // both sides of every threshold of the rules; the tile counts cdiv(M, 128 | 256) * cdiv(N, 128) straddle 256 and 512 at N <= 128 with
    // M = 65 280 .. 131 073, N . K straddles 65 536 at (256, 256) / (256, 224), (128, 512) / (127, 512), ...
    const long Ms[] = {1, 200, 256, 257, 32767, 32768, 65280, 65281, 65408, 65409, 65535, 65536, 65537, 130816, 130817, 131072, 131073, 942080};
    const long Ns[] = {32, 33, 64, 65, 100, 127, 128, 256, 544, 1024, 16384, 16388};
    const long Ks[] = {12, 32, 64, 128, 160, 193, 224, 256, 288, 512, 2304};
    for (long M : Ms) for (long N : Ns) for (long K : Ks) shapes.push_back({M, N, K, 0, 0, 0, 0, 0, 0, 0, 0, 0, false});
    // the gemm rows of profiles/gemm_rows/dense_table_head.txt
    const long table[][3] = {{471040, 100, 256}, {942080, 256, 64}, {942080, 256, 256}, {235520, 512, 128}, {58880, 1024, 256}, {235520, 768, 256}, {58880, 256, 1024},
                             {200, 256, 256}, {942080, 64, 256}, {235520, 256, 512}, {235520, 128, 512}, {14720, 2048, 512}, {309120, 544, 256}, {942080, 128, 256},
                             {200, 256, 2048}, {58880, 768, 256}, {58880, 512, 1024}, {14720, 512, 2048}, {117760, 100, 256}, {19320, 288, 256}, {942080, 64, 64},
                             {200, 2048, 256}, {14720, 768, 256}, {200, 512, 256}, {200, 2, 256}, {14720, 256, 2048}, {29440, 100, 256}, {1, 768, 256}};
    for (const auto &t : table) shapes.push_back({t[0], t[1], t[2], 0, 0, 0, 0, 0, 0, 0, 0, 0, false});
    // its conv rows whose channel counts the lists below do not have (16 frames; kernel size, H, W, Cin, Cout)
    const long ctable[][5] = {{3, 23, 40, 512, 512}, {1, 92, 160, 256, 512}, {1, 46, 80, 512, 1024}, {1, 23, 40, 1024, 2048}};
    for (const auto &t : ctable) shapes.push_back({16 * t[1] * t[2], t[4], t[3] * t[0] * t[0], t[1], t[2], t[3], t[1], t[2], t[0], t[0], 1, t[0] / 2, true});
    // convolutions: 1 x 1, 3 x 3 stride 1 pad 1, 3 x 3 stride 2 pad 1, 7 x 7 stride 2 pad 3; the inputs of the c4 pyramid (its conv rows in
    // the table: 16 frames of 184 x 320, 92 x 160, 46 x 80, 23 x 40; the stem reads 736 x 1280 x 4), 23 x 40 against 24 x 48 for the halo
    // overhang ratio (0.80 / 1.00 against the 0.88 of the rule), 15 x 33 (0.64) and 16 x 31 (0.97)
    const long geo[][4] = {{1, 1, 1, 0}, {3, 3, 1, 1}, {3, 3, 2, 1}, {7, 7, 2, 3}};
    const long in[][2] = {{23, 40}, {24, 48}, {15, 33}, {16, 31}, {46, 80}, {92, 160}, {184, 320}, {736, 1280}};
    const long cins[] = {4, 16, 32, 48, 64, 128, 256, 512};
    const long imgs[] = {1, 16};
    for (const auto &g : geo) for (const auto &hw : in) for (long Cin : cins) for (long n : imgs) for (long N : Ns) {
        const long Ho = (hw[0] + 2 * g[3] - g[0]) / g[2] + 1, Wo = (hw[1] + 2 * g[3] - g[1]) / g[2] + 1;
        if (hw[0] == 736 && (Cin > 4 || n > 1) && g[0] != 7) continue;        // the stem's input only at the stem's own channel count
        shapes.push_back({n * Ho * Wo, N, Cin * g[0] * g[1], hw[0], hw[1], Cin, Ho, Wo, g[0], g[1], g[2], g[3], true});
    }
    struct Batch { long batch, sB; };
    const Batch batches[] = {{1, 0}, {2, 0}, {2, 1}};                         // sB 1: a per-slice B (N * K elements)
    const long res_rows[] = {0, 32, 64};
    // alignment: all 16-B, then one at a time off by 2 words (the & 3 tests) or by 4 (the & 7 tests of the dropout epilogue)
    enum { AL_NONE, AL_A, AL_LDA, AL_LDC2, AL_LDC4, AL_LDR2, AL_LDR4, AL_RC1, AL_RC4, AL_LDG, AL_COUNT };
    long count = 0;
    for (const Shape &s : shapes)
        for (int bits = 0; bits < 128; ++bits)                               // f16, Bsplit, Asplit, res, gate, scale, drop
            for (const Batch &b : batches)
                for (long rr : res_rows)
                    for (int al = 0; al < AL_COUNT; ++al) {
                        const int flags = (s.conv ? GEMM_F_CONV : 0) | (bits << 1) | (al == AL_A ? 0 : GEMM_F_A_ALIGNED);
                        if ((rr || al == AL_LDR2 || al == AL_LDR4 || al == AL_RC1 || al == AL_RC4) && !(flags & GEMM_F_RES)) continue;   // the residual's fields without one
                        if (al == AL_LDG && !(flags & GEMM_F_GATE)) continue;
                        if ((al == AL_RC1 || al == AL_RC4) && s.N <= 4) continue;
                        long v[GEMM_D_COUNT] = {};
                        v[GEMM_D_M] = s.M; v[GEMM_D_N] = s.N; v[GEMM_D_K] = s.K;
                        v[GEMM_D_LDA] = s.K + (al == AL_LDA ? 2 : 0); v[GEMM_D_LDB] = s.K;
                        v[GEMM_D_LDC] = s.N + (al == AL_LDC2 ? 2 : al == AL_LDC4 ? 4 : 0);
                        v[GEMM_D_LDR] = s.N + (al == AL_LDR2 ? 2 : al == AL_LDR4 ? 4 : 0);
                        v[GEMM_D_LDG] = s.N + (al == AL_LDG ? 2 : 0);
                        v[GEMM_D_SB] = b.sB * s.N * s.K; v[GEMM_D_BATCH] = b.batch;
                        v[GEMM_D_RES_ROWS] = rr; v[GEMM_D_RES_COLS] = s.N - (al == AL_RC1 ? 1 : al == AL_RC4 ? 4 : 0);
                        v[GEMM_D_HIN] = s.Hin; v[GEMM_D_WIN] = s.Win; v[GEMM_D_CIN] = s.Cin; v[GEMM_D_HOUT] = s.Hout; v[GEMM_D_WOUT] = s.Wout;
                        v[GEMM_D_KH] = s.KH; v[GEMM_D_KW] = s.KW; v[GEMM_D_STRIDE] = s.stride; v[GEMM_D_PAD] = s.pad;
                        emit(v, flags);
                        ++count;
                    }
    return count;
}
