// Which kernel a dense launch of the split-bf16 / split-fp16 dispatcher (s2d_launch_gemm_bf16x3, gemm_bf16.hip) takes: the whole decision as
// one pure function of the launch and the switches.  Host only, no HIP: it compiles under a plain C++ compiler and is checked on a CPU
// (gemm_route_describe.h: tests/test_gemm_route_cpu.py against tests/golden/gemm_routes.json, scripts/gemm_route_main.cpp under sanitizers).
#pragma once
#include <stdint.h>

#include "gemm_params.h"

// geometry the rules share with the kernels of gemm_bf16.hip
constexpr int GEMM_BN = 128, GEMM_BK = 32;            // column tile, k-tile
constexpr int HALO_PH = 8, HALO_PW = 16;              // patch of the 3 x 3 input-halo kernel (16 x 16 when Cout <= 64)
constexpr int WS_CONST_N = 16384;                     // length of the zeros / ones vectors of the wave-specialised kernel

// One int per environment switch the dense dispatch reads, S2D_GEMM_<ROWS ... WM> and S2D_CONV_<HALO ... STEM_PH> (values, read time and
// tests: the table in DESIGN.md "Switches"); the initialisers are the defaults.
struct GemmSwitches {
    int rows = 1, small = 1, ws = 0, hi = 2, hi_pre = 1, pipe = 1, w128 = 1, wm = 0;
    int halo = 1, halo64 = 1, halo_pipe = 0, stem = 1, stem_ph = 8;
};

enum GemmFamily {
    GEMM_ERR_ARG, GEMM_ROWS, GEMM_SMALL_M, GEMM_F16_WS, GEMM_F16_HI, GEMM_F16, GEMM_CONV3X3_HALO, GEMM_CONV7X7S2_STEM, GEMM_W128, GEMM_T2, GEMM_T4
};

// The kernel family and what selects the template instantiation inside gemm_bf16.hip: a family reads the fields its kernels are templated
// on (s2d_gemm_route_text below lists them per family).  rows / small_m: the family alone (their NKB / PARTS / NW choice is in their own files).
struct GemmRoute {
    GemmFamily family = GEMM_ERR_ARG;
    bool conv = false, bsplit = false, drop = false, res = false, asplit = false;
    bool pipe = false, pre = false;   // pipe: f16 software-pipelined main loop, conv3x3_halo fragment reads a group ahead; pre: f16_hi residual prefetch
    int ph = 0;                       // patch height: conv7x7s2_stem 8 / 16; conv3x3_halo 8 (8 x 16 x 128 channels) / 16 (Cout <= 64: 16 x 16 x 64 channels)
};

static inline int gemm_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Fills the derived fields (bytesA, bytesB, kblocks); false: an extent exceeds the 32-bit buffer offsets (S2D_ERR_ARG)
inline bool s2d_gemm_extents(GemmParams &p, bool conv, int batch)
{
    const long bA = conv ? (long)(p.M / ((long)p.Hout * p.Wout)) * p.Hin * p.Win * p.Cin * 4L : ((long)(p.M - 1) * p.lda + p.K) * 4L;
    const long bB = ((long)(p.N - 1) * p.ldb + p.K) * 4L;
    if (bA > 0xFFFFFF00L || bB > 0xFFFFFF00L) return false;   // 32-bit buffer offsets
    p.bytesA = (unsigned int)bA; p.bytesB = (unsigned int)bB;
    if (p.Bsplit) {
        if ((batch > 1 && p.sB != 0) || (long)p.N * ((p.K + 31) / 32) * 128L > 0xFFFFFF00L) return false;
        p.kblocks = (p.K + 31) / 32;
    }
    return true;
}

// what the row-resident kernel takes (f16: the split-fp16 mode)
inline bool s2d_gemm_rows_ok(const GemmParams &p, bool conv, int batch, int f16)
{
    const long bC = ((long)(p.M - 1) * p.ldc + p.N) * 4L, bR = p.res ? ((long)((p.res_rows ? p.res_rows : p.M) - 1) * p.ldr + p.N) * 4L : 0;
    return f16 && !conv && batch == 1 && p.M >= 1 && p.Bsplit && !p.Asplit && !p.gate && !p.drop_thresh && p.K % 32 == 0 && p.K >= 32 && p.K <= 256 &&
           p.N >= 128 && ((p.N | p.ldc | p.ldr | p.res_cols) & 3) == 0 && bC <= 0xFFFFFF00L && bR <= 0xFFFFFF00L;
}

// what the few-rows kernel (gemm_small.hip) takes: few rows, static pre-split B, K in whole 64-wide chunks per wave, a plain epilogue,
// 16-B aligned A rows
inline bool s2d_gemm_small_m_ok(const GemmParams &p, bool conv, int batch, int f16, const GemmSwitches &sw)
{
    return sw.small && f16 && !conv && batch == 1 && p.M >= 1 && p.M <= 256 && p.Bsplit && !p.Asplit && !p.gate && !p.drop_thresh && p.K >= 64 && p.K % 64 == 0 &&
           (p.lda & 3) == 0 && ((reinterpret_cast<uintptr_t>(p.A) & 15) == 0);
}

// Where the row-resident kernel (gemm_rows.hip) is taken by default: the shape classes in which it measured >= 5 % faster than the tiled
// kernels in isolation (scripts/mb_gemm_rows.py, profiles/gemm_rows/per_shape.txt; time tiled / time row-resident):
//   58 880 x 1024 x 256  1.48     235 520 x 768 x 256  1.17     309 120 x 544 x 256  1.21     235 520 x 512 x 128  1.11     942 080 x 256 x 256  1.08
//   942 080 x 256 x 64   0.97     942 080 x 128 x 256  0.94      58 880 x 768 x 256  1.00      14 720 x 768 x 256  0.56
// What it saves per row is the re-load and re-split of K values for every 64-column tile after the first, ~ N . K: the winners have
// N . K >= 64 K values, the two large-M losers 16 K and 32 K.  It launches M / 128 workgroups that run two to a CU and have a
// serial prologue each (load, split, first weight stage), so it needs M >= 64 K rows = two full rounds of the chip; below that only
// the widest output still wins (58 880 rows: N = 1024 yes, N = 768 a tie), and at 115 workgroups it loses to the tiled kernels' 1 380.
inline bool gemm_rows_wins(const GemmParams &p)
{
    if (p.M >= 65536) return (long)p.N * p.K >= 65536;
    return p.M >= 32768 && p.N >= 1024 && p.K >= 256;
}

// The whole decision, in dispatch order.  p: a launch s2d_gemm_extents accepted.
inline GemmRoute s2d_gemm_route(const GemmParams &p, bool conv, int batch, int f16, const GemmSwitches &sw)
{
    constexpr int BN = GEMM_BN, BK = GEMM_BK;
    GemmRoute r;
    const auto to = [&r](GemmFamily f) { r.family = f; return r; };
    if (!f16 && (p.Asplit || p.gate || p.drop_thresh)) return to(GEMM_ERR_ARG);
    // row-resident kernel (gemm_rows.hip; S2D_GEMM_ROWS, read per call: 0 never, 2 every launch it takes, 1 = default: by the rule above)
    if (sw.rows && s2d_gemm_rows_ok(p, conv, batch, f16) && (sw.rows == 2 || gemm_rows_wins(p))) return to(GEMM_ROWS);
    if (s2d_gemm_small_m_ok(p, conv, batch, f16, sw)) return to(GEMM_SMALL_M);      // the video decoder's query side (M = 200)
    r.conv = conv; r.bsplit = p.Bsplit != nullptr; r.drop = p.drop_thresh != 0; r.res = p.res != nullptr;

    // wave-specialised persistent kernel: one batch slice, >= 7 k-tiles (the previous tile's write-back is spread over the
    // k-loop), 16-B rows for the row-wise epilogue, 32-bit buffer offsets into C and the residual
    const long bC = ((long)(p.M - 1) * p.ldc + p.N) * 4L, bR = p.res ? ((long)((p.res_rows ? p.res_rows : p.M) - 1) * p.ldr + p.N) * 4L : 0;
    const bool ws_ok = sw.ws && f16 && batch == 1 && !p.gate && p.N <= WS_CONST_N && (conv || !p.scale) && p.K >= 7 * BK - (BK - 1) && ((p.N | p.ldc | p.ldr | p.res_cols) & 3) == 0 &&
                       (conv ? (p.Cin % 4 == 0 && (p.Bsplit || p.K % BK == 0)) : p.K % BK == 0) &&
                       bC <= 0xFFFFFF00L && bR <= 0xFFFFFF00L && (!p.res_rows || p.res_rows >= 64) &&
                       (!p.drop_thresh || (((p.N | p.ldc) & 7) == 0 && (!p.res || ((p.ldr | p.res_cols) & 7) == 0)));
    if (p.Asplit) {
        // pre-split A: only the wave-specialised kernel reads it (its producers copy); the caller guarantees a static B image
        const bool ok = f16 && !conv && batch == 1 && p.Bsplit && !p.scale && p.N <= WS_CONST_N && p.K >= 7 * BK - (BK - 1) && p.K % BK == 0 &&
                        ((p.N | p.ldc | p.ldr | p.res_cols) & 3) == 0 && bC <= 0xFFFFFF00L && bR <= 0xFFFFFF00L &&
                        (long)p.M * p.kblocks * 128L <= 0xFFFFFF00L && (!p.res_rows || p.res_rows >= 64) &&
                        (!p.drop_thresh || (((p.N | p.ldc) & 7) == 0 && (!p.res || ((p.ldr | p.res_cols) & 7) == 0)));
        if (!ok) return to(GEMM_ERR_ARG);
        r.asplit = true;
        return to(GEMM_F16_WS);
    }
    if (ws_ok && !conv && (sw.ws == 2 || (p.Bsplit && (long)gemm_cdiv(p.M, 128) * gemm_cdiv(p.N, BN) >= 512))) return to(GEMM_F16_WS);
    if (ws_ok && conv && !p.drop_thresh && (sw.ws == 2 || (long)gemm_cdiv(p.M, 128) * gemm_cdiv(p.N, BN) >= 512)) return to(GEMM_F16_WS);
    if (p.gate && (!f16 || batch != 1 || p.drop_thresh || ((p.N | p.ldc | p.ldr | p.res_cols | p.ldg) & 3))) return to(GEMM_ERR_ARG);
    if (p.drop_thresh) {
        // fused dropout lives in the vector epilogue of the pipelined 128x128 split-fp16 kernel (the three encoder-layer
        // GEMMs that carry it all dispatch there): 8-column mask blocks, 16-B aligned rows
        if (!f16 || conv || ((p.N | p.ldc) & 7) || (p.res && (((p.ldr | p.res_cols) & 7)))) return to(GEMM_ERR_ARG);
        r.pipe = true;
        return to(GEMM_F16);
    }
    if (f16) {
        // measured (scripts/mb_shapes.py, mb_pipe.py): the pipelined 128x128 kernel wins on the spatial convolutions and, once
        // the weights arrive pre-split, on the GEMMs with K >= 512 (+9..23 %) and on K = 256 when 128-wide tiles waste no
        // more columns than 64-wide ones; the 16-waves/CU 128x64 kernel keeps the short-K (<= 128: two to four k-steps,
        // all prologue/epilogue), narrow (N <= 64) and dynamic-B launches
        // the R50 stem geometry: its own halo kernel
        if (sw.stem && conv && p.KH == 7 && p.KW == 7 && p.stride == 2 && p.pad == 3 && p.Cin == 4 && p.N <= 64 && p.N > 32 && p.Bsplit && batch == 1 &&
            ((p.N | p.ldc | p.ldr) & 3) == 0 && !p.res_rows && p.res_cols == p.N && !p.gate && (long)p.Hin * p.Win * 16L * (p.M / ((long)p.Hout * p.Wout)) < 0x7fffffffL) {
            r.ph = sw.stem_ph == 16 ? 16 : 8;
            return to(GEMM_CONV7X7S2_STEM);
        }
        // 3 x 3 / stride 1 / pad 1 on whole 32-channel blocks with static weights: the input-halo kernel
        // ... when its 8 x 16 patches cover the image without much overhang (23 x 40 -> 24 x 48 wastes 20 %: implicit GEMM wins)
        const int ph = p.N <= 64 ? 16 : HALO_PH;              // Cout <= 64: 16 x 16 patches x 64 channels
        if (sw.halo && conv && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Cin % 32 == 0 && p.Bsplit && batch == 1 && (p.N > 64 || (sw.halo64 && p.N > 32)) &&
            ((p.N | p.ldc | p.ldr) & 3) == 0 && !p.res_rows && p.res_cols == p.N && !p.gate &&
            (sw.halo == 2 || (long)p.Hin * p.Win * 100 >= (long)gemm_cdiv(p.Hin, ph) * ph * gemm_cdiv(p.Win, HALO_PW) * HALO_PW * 88)) {
            // the pipelined form is opt-in (S2D_CONV_HALO_PIPE=1, read per call): measured +2.6 % on 942 080 x 256 x 2 304, -1..-2 % on the smaller 3 x 3 shapes, -9 % on the
            // 64-channel form (scripts/mb_conv3_pipe.py, profiles/r5_experiments/not_adopted.txt): at two waves per SIMD the fragment latency the
            // round-4 form exposes is already covered by the other wave
            r.ph = ph;
            r.pipe = sw.halo_pipe != 0;
            return to(GEMM_CONV3X3_HALO);
        }
        bool use_hi;
        if (sw.hi != 2) use_hi = sw.hi == 1;
        else if (conv && p.KH > 1) use_hi = p.N <= 64;     // N <= 64: half a 128-wide tile would idle
        else if (p.N <= 64 || p.K <= 128 || !p.Bsplit) use_hi = true;
        else if (p.K >= 512) use_hi = false;
        else {
            const float w128 = (float)(gemm_cdiv(p.N, 128) * 128) / p.N, w64 = (float)(gemm_cdiv(p.N, 64) * 64) / p.N;
            use_hi = w128 > w64 + 0.1f;
        }
        if (use_hi) {
            // residual prefetch: short K (the 1 x 1 convolutions of res2 / res3 that close a bottleneck), vector epilogue, no gate
            r.pre = sw.hi_pre && p.Bsplit && p.res && !p.gate && p.K <= 4 * BK && ((p.N | p.ldc | p.ldr | p.res_cols) & 3) == 0;
            return to(GEMM_F16_HI);
        }
        r.pipe = sw.pipe != 0;                                // measured +6..12 %
        return to(GEMM_F16);
    }
    // 128 x 64 per wave: GEMMs with enough tiles for two workgroups per CU (the implicit-GEMM form needs more address registers
    // than the 256-register budget leaves and spills: convolutions stay on the 64 x 64 kernels)
    if (sw.w128 && !conv && (long)gemm_cdiv(p.M, 256) * gemm_cdiv(p.N, BN) * batch >= (sw.w128 == 2 ? 1 : 512)) return to(GEMM_W128);
    // 256-row tiles only when they still fill the chip
    bool big = (long)gemm_cdiv(p.M, 256) * gemm_cdiv(p.N, BN) * batch >= 256;
    if (sw.wm == 2) big = false;
    if (sw.wm == 4) big = true;
    return to(big ? GEMM_T4 : GEMM_T2);
}
