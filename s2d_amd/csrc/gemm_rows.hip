// Row-resident split-fp16 x3 NT GEMM for a short contraction (32 <= K <= 256, K % 32 == 0) against static pre-split weights.
//
// The tiled kernels of gemm_bf16.hip give a workgroup one (row tile, column tile) pair: the 128 rows of A are loaded and split into
// fp16 hi / lo once per column tile, N / 64 or N / 128 times per launch, although their content never changes.  Here a workgroup owns
// 128 rows of A for ALL N columns:
//   prologue   every wave loads its 32 rows in whole 128-B lines, turns them through its LDS staging block into MFMA A fragments and
//              splits them once (split8 = two split4, the tiled kernels' function); the 2 K / 32 k-steps x (hi, lo) fragments stay
//              in registers for the whole launch (128 VGPRs at K = 256)
//   tile walk  the 64-column tiles of the weight image [N][K / 32][16 w hi | 16 w lo] arrive in LDS by `buffer_load ... lds`, no
//              registers and no split: stages of two 32-wide k-blocks (16 KB) in a ring of three, two stages ahead of the MFMAs, one
//              workgroup barrier and 24 MFMAs per wave and stage.  The LDS image of a k-block is [64 columns][128 B] with the 16-B
//              piece index XORed by (column >> 1) & 7 -- on the SOURCE address of the copy (the copy's LDS side is lane-linear) and on
//              the fragment reads: the 16 lanes of a ds_read_b128 group then cover all 64 banks
//   epilogue   per wave through its LDS staging block, 32 x 32 values at a time: 8 lanes x 16 B = one 128-B row segment per store
// Arithmetic = the tiled kernels', bit for bit: rows of A as the MFMA A operand, k = 32 kt + 16 s + 8 h + j ascending, per k-step
// cross += al.bh, cross += ah.bl, main += ah.bh, join, row_tail.  PARTS: a launch the few-rows kernel of gemm_small.hip would take
// adds the K / 64-wide partial sums of that kernel's waves in its order.
// One accumulator set: at K = 256 the resident fragments (128) + accumulators (64) + weight fragments leave no room for a second
// one under the 256 registers that two waves per SIMD allow; the stores of a tile are in flight during the next tile's MFMAs anyway.
#include "gemm_epilogue.h"
#include "gemm_route.h"
#include <atomic>

namespace {

constexpr int BM = 128, TN = 64;
constexpr int GRAN = TN * 128;                      // one k-block of a column tile: 64 columns x (16 words hi | 16 words lo)
constexpr int STAGE = 2 * GRAN, NSLOT = 3;
constexpr int EPS = 36;                             // staging row stride (words)
constexpr int EPW = 32 * EPS * 4;                   // staging block of one wave
constexpr int LDS_BYTES = NSLOT * STAGE + 4 * EPW;  // 66 KB: two workgroups per CU

// One 1-KB piece global -> LDS: lane l's 16 B at rs[voff + soff] land at LDS byte dst + 16 l (dst, soff wave-uniform).  An asm statement on
// purpose: the compiler orders every later LDS read behind an LDS-writing load it knows of with `s_waitcnt vmcnt(0)`, which would empty the
// ring at each stage; this one it does not count, and the kernel waits for its copies itself.  M0 (the LDS base of the copy) is the
// compiler's: saved and restored inside the statement.
__device__ __forceinline__ void dma_piece(const u32x4 rs, int voff, int soff, unsigned int dst)
{
    unsigned int keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rs), "s"(soff), "s"(dst) : "memory");
}

template <int NKB, bool PARTS>
__global__ __launch_bounds__(256, PARTS ? 1 : 2) void gemm_rows_kernel(GemmParams p)     // PARTS: 32 more accumulators, a handful of workgroups
{
    constexpr int SPT = (NKB + 1) / 2;              // stages per column tile; the last one of an odd NKB holds one k-block
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * BM + wave * 32;     // this wave's rows
    const int NT = (p.N + TN - 1) / TN;
    const int Q = NT * SPT;

    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.A), 0, (int)p.bytesA, 0x00020000);
    // the weight image's descriptor, by hand for dma_piece: base, stride 0, bytes, the flags make_buffer_rsrc is given everywhere here
    const unsigned long long bsp = reinterpret_cast<unsigned long long>(p.Bsplit);
    const u32x4 rsB = {(unsigned int)bsp, (unsigned int)(bsp >> 32) & 0xFFFFu, (unsigned int)((long)p.N * NKB * 128L), 0x00020000u};
    const unsigned int lds_base = (unsigned int)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char *)lds);

    // ---- weight stages.  Piece i (0..7) of a k-block = columns 8 i .. 8 i + 7, 1 KB, one wave instruction: lane -> column 8 i + lane / 8,
    // LDS piece lane % 8 of it, which holds source piece (lane % 8) ^ ((column >> 1) & 7).  Wave w copies pieces 2 w, 2 w + 1.  Columns past N
    // read column N - 1 (in range: an out-of-range load would retire ahead of older ones and break the counted waits); nobody stores them.
    auto issue = [&](int t, int sidx, int slot) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = wave * 2 + e;
            int n = t * TN + i * 8 + (lane >> 3);
            n = n < p.N ? n : p.N - 1;
            const int piece = (lane & 7) ^ (e * 4 + (lane >> 4));
            const int voff = n * (NKB * 128) + piece * 16;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int kb = 2 * sidx + g;
                if (kb < NKB) dma_piece(rsB, voff, kb * 128, lds_base + slot * STAGE + g * GRAN + i * 1024);
            }
        }
    };
    // stage q = (tile q / SPT, k-blocks 2 (q % SPT), + 1) lives in slot q % NSLOT
    issue(0, 0, 0);
    if (Q > 1) issue(SPT > 1 ? 0 : 1, SPT > 1 ? 1 : 0, 1);

    // ---- this wave's rows -> resident hi / lo fragments.  Rows past M read row M - 1; their products are never stored.
    float *ep = reinterpret_cast<float *>(lds + NSLOT * STAGE + wave * EPW);
    f16x8 ah[2 * NKB], al[2 * NKB];
    {
        const int c8 = lane & 7, r8 = lane >> 3;
        unsigned int aoff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + i * 8 + r8;
            aoff[i] = (unsigned int)((long)(m < p.M ? m : p.M - 1) * p.lda * 4L) + (unsigned int)(c8 * 16);
        }
        f32x4 ra[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[0][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)aoff[i], 0, 0));
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (kb + 1 < NKB) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    ra[(kb + 1) & 1][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)aoff[i], (kb + 1) * 128, 0));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4 *>(&ep[(i * 8 + r8) * EPS + c8 * 4]) = ra[kb & 1][i];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const f32x4 x0 = *reinterpret_cast<const f32x4 *>(&ep[l32 * EPS + 16 * s + 8 * h]);
                const f32x4 x1 = *reinterpret_cast<const f32x4 *>(&ep[l32 * EPS + 16 * s + 8 * h + 4]);
                split8(x0, x1, ah[2 * kb + s], al[2 * kb + s]);
            }
        }
    }

    // fragment reads: lane (l32, h) reads column j * 32 + l32 of the tile, source piece 2 cc + h (cc = s: hi of k-step s, 2 + s: lo)
    int boff[4];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) boff[cc] = l32 * 128 + (((2 * cc + h) ^ ((l32 >> 1) & 7)) * 16);

    f32x16 accm[2], accx[2], sum[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { accm[j][r] = 0.f; accx[j][r] = 0.f; sum[j][r] = 0.f; }

    // stage 0 has landed once at most stage 1's copies are outstanding (the rows' loads behind them have all been consumed)
    if (Q == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if ((NKB & 1) && (SPT > 1 ? 1 : 0) == SPT - 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");

    const int c4e = lane & 7, rr = lane >> 3;
    int slot = 0;
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int sidx = 0; sidx < SPT; ++sidx) {
            // Every wave waited for its own copies of stage q before it came here (below); behind the barrier all of them have landed.
            // lgkmcnt(0): this wave's reads of stage q - 1 have returned before anyone refills its slot.
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // stage q + 2 -> the slot stage q - 1 left
            const int s2 = (sidx + 2) % SPT, dt = (sidx + 2) / SPT;      // constants of the unrolled body
            const bool more = t + dt < NT;
            if (more) issue(t + dt, s2, slot >= 1 ? slot - 1 : NSLOT - 1);
            const unsigned char *sb = lds + slot * STAGE;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int kb = 2 * sidx + g;
                if (kb >= NKB) continue;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int ks = 2 * kb + s;
                    f16x8 bh[2], bl[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        bh[j] = *reinterpret_cast<const f16x8 *>(sb + g * GRAN + j * 4096 + boff[s]);
                        bl[j] = *reinterpret_cast<const f16x8 *>(sb + g * GRAN + j * 4096 + boff[2 + s]);
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        accx[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ks], bh[j], accx[j], 0, 0, 0);
                        accx[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ks], bl[j], accx[j], 0, 0, 0);
                        accm[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ks], bh[j], accm[j], 0, 0, 0);
                    }
                }
            }
            slot = slot + 1 == NSLOT ? 0 : slot + 1;
            // This wave's copies of stage q + 1 have landed once at most those of stage q + 2 are outstanding: in-range loads and stores
            // retire in order, and the tile's stores below are issued behind this wait, so no later wait sits on them.
            // (the launch's last but one stage has nothing behind it to count on and drains the queue, the last stage waits for nothing)
            if (!more) { if (t + 1 < NT || sidx + 1 < SPT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
            else if ((NKB & 1) && s2 == SPT - 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            if constexpr (PARTS) {
                // the few-rows kernel: wave w owns k in [64 w, 64 w + 64) = this stage; v = 0, v += partial of wave 0, 1, ...
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        sum[j][r] += join(accm[j][r], accx[j][r]);
                        accm[j][r] = 0.f; accx[j][r] = 0.f;
                    }
            }
        }
        // ---- the tile's 32 rows x 64 columns of this wave
        const int n0 = t * TN;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // row_tail (gemm_epilogue.h) step by step and without a divergent path around a load: rows past M and columns past N (or past
            // res_cols) read a clamped address and only the store (the residual's sum) is conditional, so the four residual rows are in
            // flight together and no load is left pending on a path that skips its use (the compiler answers that with vmcnt(0))
            const int col = n0 + j * 32 + c4e * 4;
            const int colc = col < p.N ? col : p.N - 4;
            const bool take = col < p.res_cols;
            f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f}, rs[4];
            if (p.scale) sc = *reinterpret_cast<const f32x4 *>(p.scale + colc);
            if (p.bias) bi = *reinterpret_cast<const f32x4 *>(p.bias + colc);
            if (p.res) {
                const int colr = take ? col : p.res_cols - 4;
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int row = m0 + it * 8 + rr, rowc = row < p.M ? row : p.M - 1;
                    rs[it] = *reinterpret_cast<const f32x4 *>(p.res + (long)(p.res_rows ? rowc % p.res_rows : rowc) * p.ldr + colr);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                ep[mfma32_row(r, h) * EPS + l32] = PARTS ? sum[j][r] : join(accm[j][r], accx[j][r]);
                accm[j][r] = 0.f; accx[j][r] = 0.f; sum[j][r] = 0.f;
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = m0 + it * 8 + rr;
                f32x4 v = *reinterpret_cast<const f32x4 *>(&ep[(it * 8 + rr) * EPS + c4e * 4]);
                v = v * sc + bi;
                if (p.res) {
                    const f32x4 vr = v + rs[it];
                    v = take ? vr : v;
                }
                v = row_act<false>(p, v, row, col);
                if (row < p.M && col < p.N) *reinterpret_cast<f32x4 *>(p.C + (long)row * p.ldc + col) = v;
            }
        }
    }
}

std::atomic<long> g_launches{0};

template <int NKB, bool PARTS>
int launch_rows(const GemmParams &p, hipStream_t st)
{
    static S2dDevOnce attr_set;
    if (!attr_set.done()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_rows_kernel<NKB, PARTS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
            return S2D_ERR_LAUNCH;
        attr_set.mark();
    }
    hipLaunchKernelGGL((gemm_rows_kernel<NKB, PARTS>), dim3(cdiv(p.M, BM)), dim3(256), LDS_BYTES, st, p);
    S2D_CHECK_LAUNCH();
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return S2D_OK;
}

}  // namespace

// the launches s2d_gemm_rows_ok (gemm_route.h) admits: the dispatcher of gemm_bf16.hip asks first
int s2d_launch_gemm_rows(const GemmParams &p, const GemmSwitches &sw, hipStream_t st)
{
    // a launch the few-rows kernel would take today sums K in that kernel's order (K / 64 = 2 or 4 -> 2 or 4 waves of 64)
    const bool parts = s2d_gemm_small_m_ok(p, false, 1, 1, sw) && (p.K == 128 || p.K == 256);
    switch (p.K / 32) {
    case 1: return launch_rows<1, false>(p, st);
    case 2: return launch_rows<2, false>(p, st);
    case 3: return launch_rows<3, false>(p, st);
    case 4: return parts ? launch_rows<4, true>(p, st) : launch_rows<4, false>(p, st);
    case 5: return launch_rows<5, false>(p, st);
    case 6: return launch_rows<6, false>(p, st);
    case 7: return launch_rows<7, false>(p, st);
    case 8: return parts ? launch_rows<8, true>(p, st) : launch_rows<8, false>(p, st);
    }
    return S2D_ERR_ARG;
}

extern "C" long s2d_gemm_rows_launches(void) { return g_launches.load(std::memory_order_relaxed); }
