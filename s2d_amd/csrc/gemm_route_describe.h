// Test hook of the dense dispatch: the route of a launch (gemm_route.h) as text, from plain integers.  Host only, no HIP; exported from
// gemm_bf16.hip as s2d_gemm_route_describe and kept out of include/s2d_hip.h.
#pragma once
#include <stdio.h>

#include "gemm_route.h"

// A launch as plain integers (pointers as presence bits), for s2d_gemm_route_describe: a CPU reads the route of any launch.
enum { GEMM_D_M, GEMM_D_N, GEMM_D_K, GEMM_D_LDA, GEMM_D_LDB, GEMM_D_LDC, GEMM_D_LDR, GEMM_D_LDG, GEMM_D_SB, GEMM_D_RES_ROWS, GEMM_D_RES_COLS, GEMM_D_BATCH,
       GEMM_D_HIN, GEMM_D_WIN, GEMM_D_CIN, GEMM_D_HOUT, GEMM_D_WOUT, GEMM_D_KH, GEMM_D_KW, GEMM_D_STRIDE, GEMM_D_PAD, GEMM_D_COUNT };
enum { GEMM_F_CONV = 1, GEMM_F_F16 = 2, GEMM_F_BSPLIT = 4, GEMM_F_ASPLIT = 8, GEMM_F_RES = 16, GEMM_F_GATE = 32, GEMM_F_SCALE = 64, GEMM_F_DROP = 128,
       GEMM_F_A_ALIGNED = 256 };
constexpr int GEMM_SWITCH_COUNT = 13;   // in the member order of GemmSwitches

// launch[GEMM_D_COUNT], flags (GEMM_F_*), switches[GEMM_SWITCH_COUNT] -> a stable text name of the route in out; returns its length, < 0: out too short
inline int s2d_gemm_route_text(const long *launch, int flags, const int *switches, char *out, int out_len)
{
    // never dereferenced: the rules read pointers for presence and, of A, 16-B alignment
    const auto sentinel = [](bool on, uintptr_t v) { return on ? reinterpret_cast<const float *>(v) : nullptr; };
    GemmParams p = {};
    p.M = (int)launch[GEMM_D_M]; p.N = (int)launch[GEMM_D_N]; p.K = (int)launch[GEMM_D_K];
    p.lda = launch[GEMM_D_LDA]; p.ldb = launch[GEMM_D_LDB]; p.ldc = launch[GEMM_D_LDC]; p.ldr = launch[GEMM_D_LDR]; p.ldg = launch[GEMM_D_LDG];
    p.sB = launch[GEMM_D_SB]; p.res_rows = (int)launch[GEMM_D_RES_ROWS]; p.res_cols = (int)launch[GEMM_D_RES_COLS];
    p.Hin = (int)launch[GEMM_D_HIN]; p.Win = (int)launch[GEMM_D_WIN]; p.Cin = (int)launch[GEMM_D_CIN]; p.Hout = (int)launch[GEMM_D_HOUT]; p.Wout = (int)launch[GEMM_D_WOUT];
    p.KH = (int)launch[GEMM_D_KH]; p.KW = (int)launch[GEMM_D_KW]; p.stride = (int)launch[GEMM_D_STRIDE]; p.pad = (int)launch[GEMM_D_PAD];
    p.A = sentinel(true, (flags & GEMM_F_A_ALIGNED) ? 0x1000 : 0x1004);
    p.Bsplit = reinterpret_cast<const unsigned int *>(sentinel(flags & GEMM_F_BSPLIT, 0x2000));
    p.Asplit = reinterpret_cast<const unsigned int *>(sentinel(flags & GEMM_F_ASPLIT, 0x3000));
    p.res = sentinel(flags & GEMM_F_RES, 0x4000); p.gate = sentinel(flags & GEMM_F_GATE, 0x5000); p.scale = sentinel(flags & GEMM_F_SCALE, 0x6000);
    p.drop_thresh = (flags & GEMM_F_DROP) ? 26u : 0u;
    const bool conv = flags & GEMM_F_CONV;
    const int batch = (int)launch[GEMM_D_BATCH], f16 = (flags & GEMM_F_F16) ? 1 : 0;
    GemmSwitches sw;
    int *const member[GEMM_SWITCH_COUNT] = {&sw.rows, &sw.small, &sw.ws, &sw.hi, &sw.hi_pre, &sw.pipe, &sw.w128, &sw.wm, &sw.halo, &sw.halo64, &sw.halo_pipe, &sw.stem, &sw.stem_ph};
    for (int i = 0; i < GEMM_SWITCH_COUNT; ++i) *member[i] = switches[i];
    const GemmRoute r = s2d_gemm_extents(p, conv, batch) ? s2d_gemm_route(p, conv, batch, f16, sw) : GemmRoute();
    int n = -1;
    switch (r.family) {
    case GEMM_ERR_ARG: n = snprintf(out, out_len, "err_arg"); break;
    case GEMM_ROWS: n = snprintf(out, out_len, "rows"); break;
    case GEMM_SMALL_M: n = snprintf(out, out_len, "small_m"); break;
    case GEMM_F16_WS: n = snprintf(out, out_len, "f16_ws<conv=%d,bsplit=%d,drop=%d,res=%d,asplit=%d>", r.conv, r.bsplit, r.drop, r.res, r.asplit); break;
    case GEMM_F16_HI: n = snprintf(out, out_len, "f16_hi<conv=%d,bsplit=%d,pre=%d>", r.conv, r.bsplit, r.pre); break;
    case GEMM_F16: n = snprintf(out, out_len, "f16<conv=%d,pipe=%d,bsplit=%d,drop=%d>", r.conv, r.pipe, r.bsplit, r.drop); break;
    case GEMM_CONV3X3_HALO: n = snprintf(out, out_len, "conv3x3_halo<ph=%d,pipe=%d>", r.ph, r.pipe); break;
    case GEMM_CONV7X7S2_STEM: n = snprintf(out, out_len, "conv7x7s2_stem<ph=%d>", r.ph); break;
    case GEMM_W128: n = snprintf(out, out_len, "w128<bsplit=%d>", r.bsplit); break;
    case GEMM_T2: n = snprintf(out, out_len, "t<2,conv=%d>", r.conv); break;
    case GEMM_T4: n = snprintf(out, out_len, "t<4,conv=%d>", r.conv); break;
    }
    return n < out_len ? n : -1;
}
