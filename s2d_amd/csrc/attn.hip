// Masked cross-attention of the video decoder, streamed over the key axis (never materialises the
// [B*8, Q, K] bool mask nor the score matrix), plus the attention-mask builder.
//
// Replaces, per decoder layer (video_mask2former_transformer_decoder.py):
//   :460-465  F.interpolate(outputs_mask -> level size) ; sigmoid() < 0.5 ; repeat over 8 heads
//   :413      rows that are entirely masked are reset to all-False
//   :99-111   nn.MultiheadAttention core: softmax(q k^T / sqrt(d) + mask) v   (projections are GEMMs)
//
// Layouts: keys of clip b are the NHWC tokens of its T frames, [B][K = T*h*w][256] (t-major, matching the
// reference's (T*hw) x B x C order at :394-397); mask logits are pixel-major [B][T*hm*wm][ldq] (the natural
// row-major output of the mask-logit GEMM); the attention mask is a bit matrix [B][K][4 words] (bit q of a
// key's 128-bit row = "query q may NOT attend"), 16 B per key instead of 8*Q bytes.
//
// Cross-attention kernel: one workgroup = (clip, head, key split); 4 waves = 4 x 32 queries.  Scores are
// computed TRANSPOSED on the fp32 MFMA, S^T[key][q] = K . Q^T (A = K tile from LDS, B = Q in registers), so
// a lane owns one query column: the online-softmax max/sum are per-lane scalars, and the probabilities P
// (the accumulator registers) are directly the B operand of O^T[d][q] += V^T . P^T -- no LDS round trip
// for P and no cross-lane rescale.  Partial (O, m, l) per key split are merged by a second tiny kernel.
//
// tests/test_gpu_attn_masks.py pins, against float64, what the model's own masks and logits ask of these kernels: whole tiles, whole
// forward / backward splits and trailing empty splits masked for a query (m = -1e30, l = 0 carried and dropped by the merges, exact-zero
// dK / dV rows), K = 1 .. 129 against Q = 1 .. 128, scores up to |s| ~ 270 with a common-mode part, and fp16-subnormal probability
// splits (profiles/attn_masks_parity.txt).  The MFMA backward recomputes the scores with the forward's own arithmetic, so s - lse is
// consistent at any magnitude; the scalar pair (S2D_ATTN_BWD_MFMA=0) forms them with fp32 FMAs against the forward's lse and is held
// to the bound at unit-scale scores only (at |s| ~ 270 its dQ is 1.8e-3 off).
#include "split_f16.h"
#include <stdlib.h>

namespace {

constexpr int QW = 4;            // 32-bit mask words per key (Q <= 128)
constexpr int KT = 32;           // keys per tile
constexpr int LSTR = 36;         // LDS row stride (floats)

// ------------------------------------------------------------------------------------------------
// attention-mask builder: 32 lanes per key, lane g owns queries 4g..4g+3
// COHERENT: system-scope loads of the mask logits (a round-1 diagnostic form; the shipped launch uses plain 16-B loads)
template <bool COHERENT>
__global__ __launch_bounds__(256) void attn_mask_kernel(const float *__restrict__ ml, int ldq, int Q, int T, int hm, int wm,
                                                        int hl, int wl, uint32_t *__restrict__ bits,
                                                        uint32_t *__restrict__ unmasked, int compact)
{
    __shared__ uint32_t um[QW];
    const int b = blockIdx.y;
    const int K = T * hl * wl;                 // < 2^31 (checked on the host): 32-bit index decomposition
    if (threadIdx.x < QW) um[threadIdx.x] = 0u;
    __syncthreads();
    const int g = threadIdx.x & 31;
    const int key = blockIdx.x * 8 + (threadIdx.x >> 5);
    uint32_t nib = 0u, valid = 0u;
    if (key < K) {
        const int x = key % wl, yy = key / wl, y = yy % hl, t = yy / hl;
        // ATen bilinear source index, align_corners=False
        float sy = ((float)hm / hl) * (y + 0.5f) - 0.5f; if (sy < 0.f) sy = 0.f;
        float sx = ((float)wm / wl) * (x + 0.5f) - 0.5f; if (sx < 0.f) sx = 0.f;
        const int y0 = (int)sy, x0 = (int)sx, y1 = y0 + (y0 < hm - 1 ? 1 : 0), x1 = x0 + (x0 < wm - 1 ? 1 : 0);
        const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
        const float *base = ml + ((long)b * T + t) * hm * wm * ldq;
        const int q0 = 4 * g;
        if (q0 < Q) {
            const float *p00 = base + ((long)y0 * wm + x0) * ldq + q0, *p01 = base + ((long)y0 * wm + x1) * ldq + q0;
            const float *p10 = base + ((long)y1 * wm + x0) * ldq + q0, *p11 = base + ((long)y1 * wm + x1) * ldq + q0;
            if (compact) {       // logits were computed only at the four source pixels of each key: rows [b][key][4]
                const float *cb = ml + (((long)b * K + key) * 4) * ldq + q0;
                p00 = cb; p01 = cb + ldq; p10 = cb + 2 * ldq; p11 = cb + 3 * ldq;
            }
            f32x4 a00, a01, a10, a11;
            if (q0 + 3 < Q && !COHERENT && (ldq & 3) == 0) {      // rows are 16-B aligned: one 16-B load per tap
                a00 = *reinterpret_cast<const f32x4 *>(p00); a01 = *reinterpret_cast<const f32x4 *>(p01);
                a10 = *reinterpret_cast<const f32x4 *>(p10); a11 = *reinterpret_cast<const f32x4 *>(p11);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = q0 + j < Q;
                    if (COHERENT) {
                        a00[j] = ok ? __hip_atomic_load(p00 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0.f;
                        a01[j] = ok ? __hip_atomic_load(p01 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0.f;
                        a10[j] = ok ? __hip_atomic_load(p10 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0.f;
                        a11[j] = ok ? __hip_atomic_load(p11 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0.f;
                    } else {
                        a00[j] = ok ? p00[j] : 0.f; a01[j] = ok ? p01[j] : 0.f; a10[j] = ok ? p10[j] : 0.f; a11[j] = ok ? p11[j] : 0.f;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (q0 + j < Q) {
                    const float v = hy * (hx * a00[j] + lx * a01[j]) + ly * (hx * a10[j] + lx * a11[j]);
                    valid |= 1u << j;
                    // sigmoid(v) < 0.5  <=>  v < 0   (:463)
                    if (v < 0.f) nib |= 1u << j;
                }
            }
        }
    }
    // assemble 32-bit words from 8 lanes' nibbles
    uint32_t w = nib << (4 * (g & 7));
    uint32_t open = (valid & ~nib) << (4 * (g & 7));   // queries that CAN attend this key
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        w |= __shfl_xor(w, o, 64);
        open |= __shfl_xor(open, o, 64);
    }
    if ((g & 7) == 0 && key < K) {
        bits[((long)b * K + key) * QW + (g >> 3)] = w;
        if (open) atomicOr(&um[g >> 3], open);
    }
    __syncthreads();
    // every workgroup of a clip ORs into the same four words: test first, so that once the bits are set (after the first
    // few workgroups) nobody queues on the L2 atomic unit any more -- a stale read only costs a redundant atomic
    if (threadIdx.x < QW && um[threadIdx.x]) {
        const uint32_t want = um[threadIdx.x];
        const uint32_t have = __hip_atomic_load(&unmasked[b * QW + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((have & want) != want) atomicOr(&unmasked[b * QW + threadIdx.x], want);
    }
}

// ---- regression variant ------------------------------------------------------------------------
// Round 1's form of the kernel above (guarded 4-B tap loads, the four taps of a query consumed together).  Under the
// compiler's SLP vectorisation its arithmetic became v_pk_mul_f32 issued straight behind `s_waitcnt vmcnt(0)`, with the
// youngest global_load_dword's register as a source, and on MI355X that packed op computed with 0 in lanes 48..63 whenever
// a second HIP stream kept the CUs busy (profiles/r2_two_stream_diagnosis/, DESIGN.md "Streams").  The library is now
// built without SLP / loop vectorisation and scripts/isa_lint.py rejects the shape; this source stays, selected by
// S2D_ATTN_MASK_DWORD_TAPS=1, so that tests/test_gpu_fullsize.py can run the two-stream schedule on it.
__global__ __launch_bounds__(256) void attn_mask_kernel_dword_taps(const float *__restrict__ ml, int ldq, int Q, int T, int hm, int wm,
                                                                   int hl, int wl, uint32_t *__restrict__ bits,
                                                                   uint32_t *__restrict__ unmasked)
{
    __shared__ uint32_t um[QW];
    const int b = blockIdx.y;
    const long K = (long)T * hl * wl;
    if (threadIdx.x < QW) um[threadIdx.x] = 0u;
    __syncthreads();
    const int g = threadIdx.x & 31;
    const long key = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    uint32_t nib = 0u, valid = 0u;
    if (key < K) {
        const int x = (int)(key % wl), y = (int)((key / wl) % hl), t = (int)(key / ((long)wl * hl));
        float sy = ((float)hm / hl) * (y + 0.5f) - 0.5f; if (sy < 0.f) sy = 0.f;
        float sx = ((float)wm / wl) * (x + 0.5f) - 0.5f; if (sx < 0.f) sx = 0.f;
        const int y0 = (int)sy, x0 = (int)sx, y1 = y0 + (y0 < hm - 1 ? 1 : 0), x1 = x0 + (x0 < wm - 1 ? 1 : 0);
        const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
        const float *base = ml + ((long)b * T + t) * hm * wm * ldq;
        const int q0 = 4 * g;
        if (q0 < Q) {
            float v[4];
            const float *p00 = base + ((long)y0 * wm + x0) * ldq + q0, *p01 = base + ((long)y0 * wm + x1) * ldq + q0;
            const float *p10 = base + ((long)y1 * wm + x0) * ldq + q0, *p11 = base + ((long)y1 * wm + x1) * ldq + q0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (q0 + j < Q) {
                    const float a00 = p00[j], a01 = p01[j], a10 = p10[j], a11 = p11[j];
                    v[j] = hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11);
                    valid |= 1u << j;
                    if (v[j] < 0.f) nib |= 1u << j;
                }
            }
        }
    }
    uint32_t w = nib << (4 * (g & 7));
    uint32_t open = (valid & ~nib) << (4 * (g & 7));
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        w |= __shfl_xor(w, o, 64);
        open |= __shfl_xor(open, o, 64);
    }
    if ((g & 7) == 0 && key < K) {
        bits[((long)b * K + key) * QW + (g >> 3)] = w;
        if (open) atomicOr(&um[g >> 3], open);
    }
    __syncthreads();
    if (threadIdx.x < QW && um[threadIdx.x]) atomicOr(&unmasked[b * QW + threadIdx.x], um[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// split-fp16 x3 attention: both products of the forward and all five of the backward on the scheme of split_f16.h

struct AttnParams {
    const float *q, *k, *v;      // q [B][Q][C] (projected, unscaled); k, v [B][K][C]
    const uint32_t *bits;        // [B][K][QW] or null
    const uint32_t *unmasked;    // [B][QW] or null
    float *wo, *wm, *wl;         // partials: wo [B][H][S][32][128], wm/wl [B][H][S][128]
    int Q, K, C, H, S, tiles_per_split;
    long ldk, ldv;               // row strides of k and v (>= C): a slice of a wider projection output
    float qscale;                // 1/sqrt(d) * log2(e)
};

__global__ __launch_bounds__(256) void cross_attn_kernel(AttnParams p)
{
    // K tile as split fp16 (row = 16 words hi | 16 words lo | pad): Q.K^T runs on the f16 matrix cores at fp32-class
    // accuracy (3 x 32 cycles per 16 dims instead of 8 x 64 for the fp32-input MFMA); V stays fp32 for the P.V product
    __shared__ __attribute__((aligned(16))) unsigned int Ks[2][KT][LSTR];
    // V tile transposed and split: Vth / Vtl [d][key slot] in fp16, key slots permuted so that the 8 keys a lane holds of P
    // in the MFMA C layout (16 st + 8 (j >> 2) + 4 h + (j & 3), j = 0..7) are 8 consecutive halves of row d
    constexpr int VROW = 40;
    __shared__ __attribute__((aligned(16))) unsigned short Vth[2][32][VROW], Vtl[2][32][VROW];
    __shared__ uint32_t Ms[2][KT][QW];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l32 = lane & 31, h = lane >> 5;
    const int split = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;
    const int q = wv * 32 + l32;
    const bool qok = q < p.Q;

    // Q fragment in registers, split: MFMA step st covers dims 16 st .. 16 st + 15, lane half h owns 8 h .. 8 h + 7 of them
    f16x8 qh[2], ql[2];
    {
        const float *qp = p.q + ((long)b * p.Q + (qok ? q : 0)) * p.C + hd * 32 + 8 * h;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            f32x4 t0 = qok ? *reinterpret_cast<const f32x4 *>(qp + 16 * st) : f32x4(0.f);
            f32x4 t1 = qok ? *reinterpret_cast<const f32x4 *>(qp + 16 * st + 4) : f32x4(0.f);
            t0 *= p.qscale; t1 *= p.qscale;
            u32x2 h0, l0, h1, l1;
            split4(t0, h0, l0);
            split4(t1, h1, l1);
            const u32x4 hv = {h0[0], h0[1], h1[0], h1[1]}, lv = {l0[0], l0[1], l1[0], l1[1]};
            qh[st] = __builtin_bit_cast(f16x8, hv);
            ql[st] = __builtin_bit_cast(f16x8, lv);
        }
    }
    bool use_mask = p.bits != nullptr;
    if (use_mask && p.unmasked) {
        // a query whose every key is masked attends everywhere instead (:413)
        const uint32_t u = p.unmasked[b * QW + wv];
        if (!((u >> l32) & 1u)) use_mask = false;
    }

    const int tile0 = split * p.tiles_per_split;
    const int ntiles_all = (p.K + KT - 1) / KT;
    const int tile1 = min(ntiles_all, tile0 + p.tiles_per_split);

    // staging: thread t loads float4 #(t&7) of key row (t>>3) for K and V; threads < 128 load one mask word
    const int srow = tid >> 3, sc4 = tid & 7;
    const float *kbase = p.k + (long)b * p.K * p.ldk + hd * 32 + sc4 * 4;
    const float *vbase = p.v + (long)b * p.K * p.ldv + hd * 32 + sc4 * 4;
    f32x4 rk, rv;
    uint32_t rm = 0u;
    auto load_tile = [&](int tile) {
        const long key = (long)tile * KT + srow;
        rk = f32x4(0.f); rv = f32x4(0.f);
        if (key < p.K) {
            rk = *reinterpret_cast<const f32x4 *>(kbase + key * p.ldk);
            rv = *reinterpret_cast<const f32x4 *>(vbase + key * p.ldv);
        }
        if (p.bits && tid < KT * QW) {
            const long mk = (long)tile * KT + (tid >> 2);
            rm = mk < p.K ? p.bits[((long)b * p.K + mk) * QW + (tid & 3)] : 0xFFFFFFFFu;
        }
    };
    auto store_tile = [&](int buf) {
        u32x2 kh, kl;
        split4(rk, kh, kl);
        *reinterpret_cast<u32x2 *>(&Ks[buf][srow][sc4 * 2]) = kh;
        *reinterpret_cast<u32x2 *>(&Ks[buf][srow][16 + sc4 * 2]) = kl;
        u32x2 vh, vl;
        split4(rv, vh, vl);
        const int k16 = srow & 15;
        const int pos = (srow >> 4) * 16 + ((k16 >> 2) & 1) * 8 + (((k16 >> 3) << 2) | (k16 & 3));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Vth[buf][sc4 * 4 + e][pos] = (unsigned short)(vh[e >> 1] >> (16 * (e & 1)));
            Vtl[buf][sc4 * 4 + e][pos] = (unsigned short)(vl[e >> 1] >> (16 * (e & 1)));
        }
        if (p.bits && tid < KT * QW) Ms[buf][tid >> 2][tid & 3] = rm;
    };

    f32x16 o, ox;                                    // main / cross accumulators of O^T
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[r] = 0.f; ox[r] = 0.f; }
    float m = -1e30f, l = 0.f;

    if (tile0 < tile1) {
        load_tile(tile0);
        store_tile(0);
    }
    __syncthreads();
    for (int tile = tile0; tile < tile1; ++tile) {
        const int cur = (tile - tile0) & 1;
        if (tile + 1 < tile1) load_tile(tile + 1);

        // S^T[key][q] = sum_d K[key][d] * Q[q][d]   (split-fp16 x3: main + cross / 2^11)
        f32x16 s, sx;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; sx[r] = 0.f; }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const f16x8 kh = *reinterpret_cast<const f16x8 *>(&Ks[cur][l32][8 * st + 4 * h]);
            const f16x8 kl = *reinterpret_cast<const f16x8 *>(&Ks[cur][l32][16 + 8 * st + 4 * h]);
            sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[st], sx, 0, 0, 0);
            sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[st], sx, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[st], s, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = join(s[r], sx[r]);
        // mask + tail, tile max  (only the last tile of the key range can have a tail: uniform branch)
        float tmax = -INFINITY;
        const int kleft = p.K - tile * KT;                   // keys of this tile that exist (>= KT except on the last tile)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = (r & 3) + 8 * (r >> 2) + 4 * h;      // mfma32_row (common.h) written out
            bool dead = kr >= kleft;
            if (use_mask) dead = dead || ((Ms[cur][kr][wv] >> l32) & 1u);
            s[r] = dead ? -INFINITY : s[r];
            tmax = fmaxf(tmax, s[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);
        // raw v_exp_f32: arguments are <= 0 (or -inf -> 0); results below the normal range flush to zero, which is what a
        // softmax weight of 2^-126 is worth
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - mn);
            ps += s[r];
        }
        l = l * alpha + ps;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[r] *= alpha; ox[r] *= alpha; }
        // O^T[d][q] += sum_key V[key][d] * P[q][key]: the lane's own 8 probabilities of step st are the B fragment
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            u32x4 phv, plv;
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {
                // split2 (split_f16.h) written out, as in frag_from_acc below
                const float a = s[8 * st + 2 * jp], bq = s[8 * st + 2 * jp + 1];
                const h16x2 hh = __builtin_amdgcn_cvt_pkrtz(a, bq);
                const h16x2 ll = __builtin_amdgcn_cvt_pkrtz((a - (float)hh[0]) * SPLIT_SCALE, (bq - (float)hh[1]) * SPLIT_SCALE);
                phv[jp] = __builtin_bit_cast(unsigned int, hh);
                plv[jp] = __builtin_bit_cast(unsigned int, ll);
            }
            const f16x8 ph = __builtin_bit_cast(f16x8, phv), pl = __builtin_bit_cast(f16x8, plv);
            const f16x8 vth = *reinterpret_cast<const f16x8 *>(&Vth[cur][l32][16 * st + 8 * h]);
            const f16x8 vtl = *reinterpret_cast<const f16x8 *>(&Vtl[cur][l32][16 * st + 8 * h]);
            ox = __builtin_amdgcn_mfma_f32_32x32x16_f16(vtl, ph, ox, 0, 0, 0);
            ox = __builtin_amdgcn_mfma_f32_32x32x16_f16(vth, pl, ox, 0, 0, 0);
            o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vth, ph, o, 0, 0, 0);
        }
        if (tile + 1 < tile1) store_tile(cur ^ 1);
        __syncthreads();
    }
    l += __shfl_xor(l, 32, 64);
    const long pidx = (((long)b * p.H + hd) * p.S + split);
    if (h == 0) {
        p.wm[pidx * 128 + q] = m;
        p.wl[pidx * 128 + q] = l;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = (r & 3) + 8 * (r >> 2) + 4 * h;            // mfma32_row (common.h) written out
        p.wo[(pidx * 32 + d) * 128 + q] = join(o[r], ox[r]);
    }
}

// merge the S partials: out[b][q][hd*32+d]
__global__ void attn_merge_kernel(const float *__restrict__ wo, const float *__restrict__ wm, const float *__restrict__ wl,
                                  int B, int Q, int C, int H, int S, float *__restrict__ out, float *__restrict__ lse)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)B * H * 32 * 128;
    if (i >= total) return;
    const int q = (int)(i % 128);
    const int d = (int)((i / 128) % 32);
    const int hd = (int)((i / (128 * 32)) % H);
    const int b = (int)(i / ((long)128 * 32 * H));
    if (q >= Q) return;
    const long base = ((long)b * H + hd) * S;
    float M = -1e30f;
    for (int s = 0; s < S; ++s) M = fmaxf(M, wm[(base + s) * 128 + q]);
    float L = 0.f, O = 0.f;
    for (int s = 0; s < S; ++s) {
        const float f = exp2f(wm[(base + s) * 128 + q] - M);
        L += wl[(base + s) * 128 + q] * f;
        O += wo[((base + s) * 32 + d) * 128 + q] * f;
    }
    out[((long)b * Q + q) * C + hd * 32 + d] = O / L;
    if (lse && d == 0) lse[((long)b * H + hd) * 128 + q] = M + log2f(L);      // base-2 log-sum-exp of the scaled scores (backward)
}

// ---- backward.  With s = q.k * scale (+ mask), P = softmax_k(s), O = P V:
//   dV = P^T dO,   dP = dO V^T,   dS = P o (dP - rowsum(dO o O)),   dQ = dS K * scale,   dK = dS^T Q * scale.
// P is recomputed from the saved log-sum-exp (nothing of size Q x K is stored).  Two fp32 kernels, neither needs a
// cross-lane reduction in its inner loop: attn_bwd_kv_kernel owns a tile of 64 keys (a thread = one key x a quarter of the
// queries, accumulating that key's dK / dV rows in registers), attn_bwd_q_kernel owns the queries over a range of key tiles
// (a thread = one query x half of the keys, accumulating the query's dQ row) and leaves per-range partials that
// attn_bwd_merge_kernel adds in a fixed order (reproducible).
struct AttnBwdParams {
    const float *q, *k, *v, *o, *dout, *lse;
    long ldk, ldv;
    const uint32_t *bits, *unmasked;
    int Q, K, C, H, S, tiles_per_split;
    float qscale;                      // 1/sqrt(d) * log2(e)
    float *dk, *dv, *dq_part;          // dk, dv [B][K][lddk / lddv] (row strides >= C: column slices of a wider gradient buffer); dq_part [B][H][S][128][32]
    long lddk, lddv;
};
constexpr int BT = 64;                 // keys per backward tile
constexpr float LN2 = 0.6931471805599453f;

// stage this head's scaled q rows, dO rows, delta = sum_d dO o O and lse for all queries
__device__ __forceinline__ void stage_queries(const AttnBwdParams &p, int b, int hd, float (*qs)[33], float (*dos)[33], float *delta, float *lses)
{
    for (int i = threadIdx.x; i < 128 * 8; i += 256) {
        const int qq = i >> 3, c = (i & 7) * 4;
        f32x4 a = f32x4(0.f), g = f32x4(0.f);
        if (qq < p.Q) {
            a = *reinterpret_cast<const f32x4 *>(p.q + ((long)b * p.Q + qq) * p.C + hd * 32 + c) * p.qscale;
            g = *reinterpret_cast<const f32x4 *>(p.dout + ((long)b * p.Q + qq) * p.C + hd * 32 + c);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { qs[qq][c + j] = a[j]; dos[qq][c + j] = g[j]; }
    }
    if (threadIdx.x < 128) {
        const int qq = threadIdx.x;
        float dl = 0.f, ls = 0.f;
        if (qq < p.Q) {
            const float *op = p.o + ((long)b * p.Q + qq) * p.C + hd * 32, *gp = p.dout + ((long)b * p.Q + qq) * p.C + hd * 32;
            for (int d = 0; d < 32; ++d) dl += op[d] * gp[d];
            ls = p.lse[((long)b * p.H + hd) * 128 + qq];
        }
        delta[qq] = dl; lses[qq] = ls;
    }
}

__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(AttnBwdParams p)
{
    __shared__ float qs[128][33], dos[128][33];
    __shared__ float delta[128], lses[128];
    __shared__ uint32_t ign[QW];                       // queries whose mask is ignored (no attendable key, :413)
    const int hd = blockIdx.y, b = blockIdx.z;
    const int kk = threadIdx.x & 63, quarter = threadIdx.x >> 6;
    const long key = (long)blockIdx.x * BT + kk;
    const bool kok = key < p.K;
    stage_queries(p, b, hd, qs, dos, delta, lses);
    if (threadIdx.x < QW) ign[threadIdx.x] = (p.bits && p.unmasked) ? ~p.unmasked[b * QW + threadIdx.x] : (p.bits ? 0u : 0xFFFFFFFFu);
    float kr[32], vr[32], dK[32], dV[32];
#pragma unroll
    for (int d = 0; d < 32; d += 4) {
        f32x4 a = f32x4(0.f), c = f32x4(0.f);
        if (kok) {
            a = *reinterpret_cast<const f32x4 *>(p.k + ((long)b * p.K + key) * p.ldk + hd * 32 + d);
            c = *reinterpret_cast<const f32x4 *>(p.v + ((long)b * p.K + key) * p.ldv + hd * 32 + d);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { kr[d + j] = a[j]; vr[d + j] = c[j]; dK[d + j] = 0.f; dV[d + j] = 0.f; }
    }
    uint32_t mw[QW] = {0u, 0u, 0u, 0u};
    if (p.bits && kok)
#pragma unroll
        for (int w = 0; w < QW; ++w) mw[w] = p.bits[((long)b * p.K + key) * QW + w];
    __syncthreads();
#pragma unroll
    for (int w = 0; w < QW; ++w) mw[w] &= ~ign[w];     // bit set = this (query, key) pair does not attend
    // two channels per vector instruction (v_pk_fma_f32): the loop is bound by its 128 multiply-adds per (query, key) pair.  Even /
    // odd channels accumulate separately and are added at the end: a fixed order.
    for (int qq = quarter; qq < p.Q; qq += 4) {
        if ((mw[qq >> 5] >> (qq & 31)) & 1u) continue;
        f32x2 s2v = {0.f, 0.f}, dpv = {0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 32; d += 2) {
            const f32x2 q2 = {qs[qq][d], qs[qq][d + 1]}, g2 = {dos[qq][d], dos[qq][d + 1]};
            const f32x2 k2 = {kr[d], kr[d + 1]}, v2 = {vr[d], vr[d + 1]};
            s2v = __builtin_elementwise_fma(q2, k2, s2v); dpv = __builtin_elementwise_fma(g2, v2, dpv);
        }
        const float s2 = s2v[0] + s2v[1], dp = dpv[0] + dpv[1];
        const float pr = kok ? exp2f(s2 - lses[qq]) : 0.f;
        const float ds = pr * (dp - delta[qq]);
        const f32x2 pr2 = {pr, pr}, ds2 = {ds, ds};
#pragma unroll
        for (int d = 0; d < 32; d += 2) {
            const f32x2 q2 = {qs[qq][d], qs[qq][d + 1]}, g2 = {dos[qq][d], dos[qq][d + 1]};
            f32x2 a = {dV[d], dV[d + 1]}, c = {dK[d], dK[d + 1]};
            a = __builtin_elementwise_fma(pr2, g2, a); c = __builtin_elementwise_fma(ds2, q2, c);
            dV[d] = a[0]; dV[d + 1] = a[1]; dK[d] = c[0]; dK[d + 1] = c[1];
        }
    }
    __syncthreads();
    // add the four query quarters (fixed order) through LDS: reuse qs / dos as [4][64][33] would not fit -> two rounds
    float (*red)[64][33] = reinterpret_cast<float (*)[64][33]>(&qs[0][0]);   // 2 x 64 x 33 floats fit in qs (128 x 33)
    for (int round = 0; round < 2; ++round) {
        const float *src = round == 0 ? dK : dV;
        // quarters 1..3 deposit in turn, quarter 0 accumulates: three steps keep the order fixed
        for (int step = 1; step < 4; ++step) {
            if (quarter == step)
#pragma unroll
                for (int d = 0; d < 32; ++d) red[0][kk][d] = src[d];
            __syncthreads();
            if (quarter == 0) {
                float *dst = round == 0 ? dK : dV;
#pragma unroll
                for (int d = 0; d < 32; ++d) dst[d] += red[0][kk][d];
            }
            __syncthreads();
        }
    }
    if (quarter == 0 && kok) {
        float *ko = p.dk + ((long)b * p.K + key) * p.lddk + hd * 32, *vo = p.dv + ((long)b * p.K + key) * p.lddv + hd * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            const f32x4 a = {dK[d] * LN2, dK[d + 1] * LN2, dK[d + 2] * LN2, dK[d + 3] * LN2};   // qs carries log2(e): back to natural scale
            const f32x4 c = {dV[d], dV[d + 1], dV[d + 2], dV[d + 3]};
            *reinterpret_cast<f32x4 *>(ko + d) = a;
            *reinterpret_cast<f32x4 *>(vo + d) = c;
        }
    }
}

__global__ __launch_bounds__(256) void attn_bwd_q_kernel(AttnBwdParams p)
{
    __shared__ float ks[BT][33], vs[BT][33];
    __shared__ uint32_t ms[BT][QW];
    __shared__ float red[128][33];
    const int split = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;
    const int qq = threadIdx.x & 127, half = threadIdx.x >> 7;
    const bool qok = qq < p.Q;
    float qr[32], gr[32], dq[32];
    float dl = 0.f, ls = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) { qr[d] = 0.f; gr[d] = 0.f; dq[d] = 0.f; }
    if (qok) {
        const float *qp = p.q + ((long)b * p.Q + qq) * p.C + hd * 32, *gp = p.dout + ((long)b * p.Q + qq) * p.C + hd * 32;
        const float *op = p.o + ((long)b * p.Q + qq) * p.C + hd * 32;
#pragma unroll
        for (int d = 0; d < 32; ++d) { qr[d] = qp[d] * p.qscale; gr[d] = gp[d]; dl += op[d] * gp[d]; }
        ls = p.lse[((long)b * p.H + hd) * 128 + qq];
    }
    bool use_mask = p.bits != nullptr;
    if (use_mask && p.unmasked && qok && !((p.unmasked[b * QW + (qq >> 5)] >> (qq & 31)) & 1u)) use_mask = false;
    const int ntiles = (p.K + BT - 1) / BT;
    const int t0 = split * p.tiles_per_split, t1 = min(ntiles, t0 + p.tiles_per_split);
    for (int t = t0; t < t1; ++t) {
        __syncthreads();
        for (int i = threadIdx.x; i < BT * 8; i += 256) {
            const int r = i >> 3, c = (i & 7) * 4;
            const long key = (long)t * BT + r;
            f32x4 a = f32x4(0.f), g = f32x4(0.f);
            if (key < p.K) {
                a = *reinterpret_cast<const f32x4 *>(p.k + ((long)b * p.K + key) * p.ldk + hd * 32 + c);
                g = *reinterpret_cast<const f32x4 *>(p.v + ((long)b * p.K + key) * p.ldv + hd * 32 + c);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { ks[r][c + j] = a[j]; vs[r][c + j] = g[j]; }
        }
        if (threadIdx.x < BT * QW) {
            const int r = threadIdx.x / QW, w = threadIdx.x % QW;
            const long key = (long)t * BT + r;
            ms[r][w] = key < p.K ? (p.bits ? p.bits[((long)b * p.K + key) * QW + w] : 0u) : 0xFFFFFFFFu;   // keys past K never attend
        }
        __syncthreads();
        if (!qok) continue;
        for (int r = half; r < BT; r += 2) {
            const uint32_t w = ms[r][qq >> 5];
            const bool beyond = (long)t * BT + r >= p.K;
            if (beyond || (use_mask && ((w >> (qq & 31)) & 1u))) continue;
            f32x2 s2v = {0.f, 0.f}, dpv = {0.f, 0.f};
#pragma unroll
            for (int d = 0; d < 32; d += 2) {
                const f32x2 k2 = {ks[r][d], ks[r][d + 1]}, v2 = {vs[r][d], vs[r][d + 1]};
                const f32x2 q2 = {qr[d], qr[d + 1]}, g2 = {gr[d], gr[d + 1]};
                s2v = __builtin_elementwise_fma(q2, k2, s2v); dpv = __builtin_elementwise_fma(g2, v2, dpv);
            }
            const float ds = exp2f((s2v[0] + s2v[1]) - ls) * ((dpv[0] + dpv[1]) - dl);
            const f32x2 ds2 = {ds, ds};
#pragma unroll
            for (int d = 0; d < 32; d += 2) {
                const f32x2 k2 = {ks[r][d], ks[r][d + 1]};
                f32x2 a = {dq[d], dq[d + 1]};
                a = __builtin_elementwise_fma(ds2, k2, a);
                dq[d] = a[0]; dq[d + 1] = a[1];
            }
        }
    }
    __syncthreads();
    if (half == 1)
#pragma unroll
        for (int d = 0; d < 32; ++d) red[qq][d] = dq[d];
    __syncthreads();
    if (half == 0) {
        float *o = p.dq_part + ((((long)b * p.H + hd) * p.S + split) * 128 + qq) * 32;
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] = dq[d] + red[qq][d];
    }
}

__global__ void attn_bwd_merge_kernel(const float *__restrict__ part, int B, int Q, int C, int H, int S, float factor, float *__restrict__ dq)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * Q * C) return;
    const int c = (int)(i % C), q = (int)((i / C) % Q), b = (int)(i / ((long)C * Q));
    const int hd = c >> 5, d = c & 31;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += part[((((long)b * H + hd) * S + s) * 128 + q) * 32 + d];
    dq[i] = a * factor;
}

// ---- backward on the matrix cores -------------------------------------------------------------------------------------------
// Same mathematics as the two scalar kernels above, every product a split-fp16 x3 MFMA contraction (fp32-class).  A workgroup =
// (key split, head, clip), its 4 waves take the split's 32-key tiles round robin; a wave owns a key tile against ALL 128 query
// rows, so dK / dV of the tile are complete inside the wave (no cross-wave sums, no atomics) and are written once, and dQ is
// accumulated per wave over its tiles, added across the 4 waves in a fixed order at the end and left as a per-split partial for
// attn_bwd_merge_kernel (as before).  Nothing of size Q x K is stored: per (key tile, 32-query tile) the scores are formed TWICE,
// once per orientation, because the two kinds of products want their (probability, dS) tile in different operand layouts --
//   lane = query:  S^T = K.Q^T, dP^T = V.dO^T  ->  dS^T  is the B operand of  dQ^T[d][q] += K^T[d][key] . dS^T[key][q]
//   lane = key:    S = Q.K^T,   dP = dO.V^T    ->  P, dS are the B operands of  dV^T[d][key] += dO^T[d][q] . P[q][key]  and
//                                                                              dK^T[d][key] += Q^T[d][q] . dS[q][key]
// (an accumulator tile has its column on the lane and 16 rows in registers: that IS the B-operand layout once the contraction
// index is permuted the same way in the A operand, which is how the transposed copies Qt / Gt / Kt are stored) -- 42 MFMAs per
// (key tile, query tile) instead of a 32 x 32 transpose through LDS.  Q, dO (split, row-major and transposed), delta = rowsum(dO o O)
// and the log-sum-exp are staged once per workgroup; K / V tiles live in wave-private LDS, so the tile loop has no barrier.
constexpr int QROW = 136;         // halves per row of the transposed Q / dO images (128 query slots + pad: rows 4 banks apart)
constexpr int KROW = 40;          // halves per row of a wave's transposed K tile

__device__ __forceinline__ int perm16(int k16) { return ((k16 >> 2) & 1) * 8 + (((k16 >> 3) << 2) | (k16 & 3)); }

// 8 accumulator registers (one MFMA k-step's worth of a C-layout tile) -> hi / lo B fragments.  The split is written out (split2 of
// split_f16.h, with the high part converted per element): the form these two kernels were compiled with
__device__ __forceinline__ void frag_from_acc(const float *v, f16x8 &fh, f16x8 &fl)
{
    u32x4 hv, lv;
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
        const float a = v[2 * jp], bq = v[2 * jp + 1];
        const h16x2 hh = __builtin_amdgcn_cvt_pkrtz(a, bq);
        const h16x2 ll = __builtin_amdgcn_cvt_pkrtz((a - (float)hh[0]) * SPLIT_SCALE, (bq - (float)hh[1]) * SPLIT_SCALE);
        hv[jp] = __builtin_bit_cast(unsigned int, hh);
        lv[jp] = __builtin_bit_cast(unsigned int, ll);
    }
    fh = __builtin_bit_cast(f16x8, hv);
    fl = __builtin_bit_cast(f16x8, lv);
}

struct AttnBwdLds {
    unsigned int Qs[128][LSTR], Gs[128][LSTR];                         // scaled q rows / dO rows: 16 words hi | 16 words lo
    unsigned short Qth[32][QROW], Qtl[32][QROW], Gth[32][QROW], Gtl[32][QROW];   // [d][query slot], slots permuted per 16 (perm16)
    float delta[128], lses[128];
    uint32_t ign[QW];
    unsigned int Ks[4][KT][LSTR], Vs[4][KT][LSTR];                      // per wave: the key tile's K / V rows, split
    unsigned short Kth[4][32][KROW], Ktl[4][32][KROW];                  // per wave: K tile transposed, key slots permuted
    uint32_t Ms[4][KT][QW];
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void attn_bwd_mfma_kernel(AttnBwdParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char attn_bwd_smem[];
    AttnBwdLds &L = *reinterpret_cast<AttnBwdLds *>(attn_bwd_smem);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l32 = lane & 31, h = lane >> 5;
    const int split = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;

    // ---- stage the head's queries: scaled q and dO, split; row-major and transposed; delta and lse
    for (int i = tid; i < 128 * 8; i += 256) {
        const int qq = i >> 3, c4 = i & 7;
        f32x4 a = f32x4(0.f), g = f32x4(0.f);
        if (qq < p.Q) {
            a = *reinterpret_cast<const f32x4 *>(p.q + ((long)b * p.Q + qq) * p.C + hd * 32 + c4 * 4) * p.qscale;
            g = *reinterpret_cast<const f32x4 *>(p.dout + ((long)b * p.Q + qq) * p.C + hd * 32 + c4 * 4);
        }
        u32x2 ah, al, gh, gl;
        split4(a, ah, al);
        split4(g, gh, gl);
        *reinterpret_cast<u32x2 *>(&L.Qs[qq][c4 * 2]) = ah; *reinterpret_cast<u32x2 *>(&L.Qs[qq][16 + c4 * 2]) = al;
        *reinterpret_cast<u32x2 *>(&L.Gs[qq][c4 * 2]) = gh; *reinterpret_cast<u32x2 *>(&L.Gs[qq][16 + c4 * 2]) = gl;
        const int pos = (qq & ~15) + perm16(qq & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            L.Qth[c4 * 4 + e][pos] = (unsigned short)(ah[e >> 1] >> (16 * (e & 1)));
            L.Qtl[c4 * 4 + e][pos] = (unsigned short)(al[e >> 1] >> (16 * (e & 1)));
            L.Gth[c4 * 4 + e][pos] = (unsigned short)(gh[e >> 1] >> (16 * (e & 1)));
            L.Gtl[c4 * 4 + e][pos] = (unsigned short)(gl[e >> 1] >> (16 * (e & 1)));
        }
    }
    if (tid < 128) {
        float dl = 0.f, ls = INFINITY;                       // rows past Q: probability exp2(s - inf) = 0
        if (tid < p.Q) {
            const float *op = p.o + ((long)b * p.Q + tid) * p.C + hd * 32, *gp = p.dout + ((long)b * p.Q + tid) * p.C + hd * 32;
            for (int d = 0; d < 32; ++d) dl += op[d] * gp[d];
            ls = p.lse[((long)b * p.H + hd) * 128 + tid];
        }
        L.delta[tid] = dl; L.lses[tid] = ls;
    }
    if (tid < QW) L.ign[tid] = (p.bits && p.unmasked) ? ~p.unmasked[b * QW + tid] : (p.bits ? 0u : 0xFFFFFFFFu);
    __syncthreads();

    const int ntiles_all = (p.K + KT - 1) / KT;
    const int t_lo = split * p.tiles_per_split, t_hi = min(ntiles_all, t_lo + p.tiles_per_split);
    // persistent accumulators hold main + cross / 2^11 already folded: the cross products of a (key tile, query tile) go to a short-lived
    // accumulator and are added scaled right away -- 96 accumulator registers live across the loop instead of 192
    f32x16 dq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[j][r] = 0.f;

    // a lane stages 4 float4 of K and of V per tile: rows (lane >> 3) + 8 i, float4 #(lane & 7)
    const int srow = lane >> 3, sc4 = lane & 7;
    const float *kbase = p.k + (long)b * p.K * p.ldk + hd * 32 + sc4 * 4;
    const float *vbase = p.v + (long)b * p.K * p.ldv + hd * 32 + sc4 * 4;
    f32x4 rk[4], rv[4];
    uint32_t rm[2];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long key = (long)tile * KT + srow + 8 * i;
            rk[i] = f32x4(0.f); rv[i] = f32x4(0.f);
            if (key < p.K) {
                rk[i] = *reinterpret_cast<const f32x4 *>(kbase + key * p.ldk);
                rv[i] = *reinterpret_cast<const f32x4 *>(vbase + key * p.ldv);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int w = lane + 64 * i;                     // word w & 3 of key w >> 2
            const long mk = (long)tile * KT + (w >> 2);
            rm[i] = mk < p.K ? (p.bits ? p.bits[((long)b * p.K + mk) * QW + (w & 3)] & ~L.ign[w & 3] : 0u) : 0xFFFFFFFFu;      // bit set = the pair does not attend; keys past K never do
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = srow + 8 * i;
            u32x2 kh, kl, vh, vl;
            split4(rk[i], kh, kl);
            split4(rv[i], vh, vl);
            *reinterpret_cast<u32x2 *>(&L.Ks[wv][row][sc4 * 2]) = kh; *reinterpret_cast<u32x2 *>(&L.Ks[wv][row][16 + sc4 * 2]) = kl;
            *reinterpret_cast<u32x2 *>(&L.Vs[wv][row][sc4 * 2]) = vh; *reinterpret_cast<u32x2 *>(&L.Vs[wv][row][16 + sc4 * 2]) = vl;
            const int pos = (row & ~15) + perm16(row & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                L.Kth[wv][sc4 * 4 + e][pos] = (unsigned short)(kh[e >> 1] >> (16 * (e & 1)));
                L.Ktl[wv][sc4 * 4 + e][pos] = (unsigned short)(kl[e >> 1] >> (16 * (e & 1)));
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) { const int w = lane + 64 * i; L.Ms[wv][w >> 2][w & 3] = rm[i]; }
    };

    int tile = t_lo + wv;
    if (tile < t_hi) load_tile(tile);
    for (; tile < t_hi; tile += 4) {
        store_tile();
        if (tile + 4 < t_hi) load_tile(tile + 4);            // in flight during this tile's arithmetic
        f32x16 dk, dv;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[r] = 0.f; dv[r] = 0.f; }
        // K / V fragments of the tile: rows = keys (A operand of the lane = query products, B operand of the lane = key ones)
        f16x8 kh[2], kl[2], vh[2], vl[2];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            kh[st] = *reinterpret_cast<const f16x8 *>(&L.Ks[wv][l32][8 * st + 4 * h]);
            kl[st] = *reinterpret_cast<const f16x8 *>(&L.Ks[wv][l32][16 + 8 * st + 4 * h]);
            vh[st] = *reinterpret_cast<const f16x8 *>(&L.Vs[wv][l32][8 * st + 4 * h]);
            vl[st] = *reinterpret_cast<const f16x8 *>(&L.Vs[wv][l32][16 + 8 * st + 4 * h]);
        }
        const uint32_t mkey[QW] = {L.Ms[wv][l32][0], L.Ms[wv][l32][1], L.Ms[wv][l32][2], L.Ms[wv][l32][3]};     // this lane's key x all queries
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (32 * j >= p.Q) break;                        // uniform
            __builtin_amdgcn_sched_barrier(0);               // keep the four query tiles' fragment loads from being hoisted together (registers)
            f16x8 qh[2], ql[2], gh[2], gl[2];
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                qh[st] = *reinterpret_cast<const f16x8 *>(&L.Qs[32 * j + l32][8 * st + 4 * h]);
                ql[st] = *reinterpret_cast<const f16x8 *>(&L.Qs[32 * j + l32][16 + 8 * st + 4 * h]);
                gh[st] = *reinterpret_cast<const f16x8 *>(&L.Gs[32 * j + l32][8 * st + 4 * h]);
                gl[st] = *reinterpret_cast<const f16x8 *>(&L.Gs[32 * j + l32][16 + 8 * st + 4 * h]);
            }
            f32x16 s, sx, dp, dpx;
            // ---- lane = query: S^T[key][q], dP^T[key][q]
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; sx[r] = 0.f; dp[r] = 0.f; dpx[r] = 0.f; }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl[st], qh[st], sx, 0, 0, 0);
                sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[st], ql[st], sx, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[st], qh[st], s, 0, 0, 0);
                dpx = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl[st], gh[st], dpx, 0, 0, 0);
                dpx = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[st], gl[st], dpx, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[st], gh[st], dp, 0, 0, 0);
            }
            {
                const float lq = L.lses[32 * j + l32], dlq = L.delta[32 * j + l32];
                f32x16 cx;
#pragma unroll
                for (int r = 0; r < 16; ++r) cx[r] = 0.f;
                // dQ^T[d][q] += K^T[d][key] . dS^T[key][q], one k-step (8 of the lane's 16 keys) at a time
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    float dst[8];
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) {
                        const int r = 8 * st + jj;
                        const int kr = mfma32_row(r, h);
                        const bool dead = (L.Ms[wv][kr][j] >> l32) & 1u;
                        const float arg = dead ? -INFINITY : join(s[r], sx[r]) - lq;       // exp2(-inf) = 0
                        dst[jj] = __builtin_amdgcn_exp2f(arg) * (join(dp[r], dpx[r]) - dlq);
                    }
                    f16x8 bh, bl;
                    frag_from_acc(dst, bh, bl);
                    const f16x8 ath = *reinterpret_cast<const f16x8 *>(&L.Kth[wv][l32][16 * st + 8 * h]);
                    const f16x8 atl = *reinterpret_cast<const f16x8 *>(&L.Ktl[wv][l32][16 * st + 8 * h]);
                    cx = __builtin_amdgcn_mfma_f32_32x32x16_f16(atl, bh, cx, 0, 0, 0);
                    cx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ath, bl, cx, 0, 0, 0);
                    dq[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ath, bh, dq[j], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) dq[j][r] = __builtin_fmaf(cx[r], SPLIT_INV, dq[j][r]);     // join_fma (split_f16.h) written out
            }
            // ---- lane = key: S[q][key], dP[q][key]
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; sx[r] = 0.f; dp[r] = 0.f; dpx[r] = 0.f; }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ql[st], kh[st], sx, 0, 0, 0);
                sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh[st], kl[st], sx, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh[st], kh[st], s, 0, 0, 0);
                dpx = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl[st], vh[st], dpx, 0, 0, 0);
                dpx = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh[st], vl[st], dpx, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh[st], vh[st], dp, 0, 0, 0);
            }
            {
                // dV^T[d][key] += dO^T[d][q] . P[q][key];  dK^T[d][key] += Q^T[d][q] . dS[q][key], one k-step (8 query rows) at a time:
                // the lane's rows of step st are 16 st + 8 g + 4 h + e (g = 0, 1; e = 0..3): two 16-B reads of lse / delta
                f32x16 dkx, dvx;
#pragma unroll
                for (int r = 0; r < 16; ++r) { dkx[r] = 0.f; dvx[r] = 0.f; }
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    float pv[8], dsv[8];
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        const int q0 = 32 * j + 16 * st + 8 * g + 4 * h;
                        const f32x4 l4 = *reinterpret_cast<const f32x4 *>(&L.lses[q0]), d4 = *reinterpret_cast<const f32x4 *>(&L.delta[q0]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int r = 8 * st + 4 * g + e;
                            const bool dead = (mkey[j] >> (q0 - 32 * j + e)) & 1u;
                            const float arg = dead ? -INFINITY : join(s[r], sx[r]) - l4[e];
                            const float pr = __builtin_amdgcn_exp2f(arg);
                            pv[4 * g + e] = pr;
                            dsv[4 * g + e] = pr * (join(dp[r], dpx[r]) - d4[e]);
                        }
                    }
                    f16x8 ph, pl, sh, sl;
                    frag_from_acc(pv, ph, pl);
                    frag_from_acc(dsv, sh, sl);
                    const int col = 32 * j + 16 * st + 8 * h;
                    const f16x8 gth = *reinterpret_cast<const f16x8 *>(&L.Gth[l32][col]), gtl = *reinterpret_cast<const f16x8 *>(&L.Gtl[l32][col]);
                    const f16x8 qth = *reinterpret_cast<const f16x8 *>(&L.Qth[l32][col]), qtl = *reinterpret_cast<const f16x8 *>(&L.Qtl[l32][col]);
                    dvx = __builtin_amdgcn_mfma_f32_32x32x16_f16(gtl, ph, dvx, 0, 0, 0);
                    dvx = __builtin_amdgcn_mfma_f32_32x32x16_f16(gth, pl, dvx, 0, 0, 0);
                    dv = __builtin_amdgcn_mfma_f32_32x32x16_f16(gth, ph, dv, 0, 0, 0);
                    dkx = __builtin_amdgcn_mfma_f32_32x32x16_f16(qtl, sh, dkx, 0, 0, 0);
                    dkx = __builtin_amdgcn_mfma_f32_32x32x16_f16(qth, sl, dkx, 0, 0, 0);
                    dk = __builtin_amdgcn_mfma_f32_32x32x16_f16(qth, sh, dk, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) { dk[r] = __builtin_fmaf(dkx[r], SPLIT_INV, dk[r]); dv[r] = __builtin_fmaf(dvx[r], SPLIT_INV, dv[r]); }
            }
        }
        // the tile's dK / dV rows: lane = key, registers = d rows (r & 3) + 8 (r >> 2) + 4 h -> four 16-B runs per lane
        const long key = (long)tile * KT + l32;
        if (key < p.K) {
            float *ko = p.dk + ((long)b * p.K + key) * p.lddk + hd * 32 + 4 * h, *vo = p.dv + ((long)b * p.K + key) * p.lddv + hd * 32 + 4 * h;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                f32x4 a, c;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = dk[4 * g4 + e] * LN2;                            // the staged q carries log2(e): back to natural scale
                    c[e] = dv[4 * g4 + e];
                }
                *reinterpret_cast<f32x4 *>(ko + 8 * g4) = a;
                *reinterpret_cast<f32x4 *>(vo + 8 * g4) = c;
            }
        }
    }
    // ---- dQ: the 4 waves' partials added in wave order, one [128][32] partial per split
    __syncthreads();                                          // every wave is done with the staged queries: their LDS becomes the exchange area
    float (*red)[128][33] = reinterpret_cast<float (*)[128][33]>(attn_bwd_smem);      // [4][128][33] floats = 67.6 KB <= the Q / dO images
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = mfma32_row(r, h);
            red[wv][32 * j + l32][d] = dq[j][r];
        }
    __syncthreads();
    float *o = p.dq_part + (((long)b * p.H + hd) * p.S + split) * 128 * 32;
    for (int i = tid; i < 128 * 32; i += 256) {
        const int qq = i >> 5, d = i & 31;
        o[i] = ((red[0][qq][d] + red[1][qq][d]) + red[2][qq][d]) + red[3][qq][d];
    }
}

}  // namespace

extern "C" {

int s2d_attn_mask_bits(const float *mask_logits, int ldq, int B, int Q, int T, int hm, int wm, int hl, int wl, int compact,
                       uint32_t *bits, uint32_t *unmasked, hipStream_t stream)
{
    if (Q > 128 || Q <= 0 || ldq < Q) return S2D_ERR_ARG;
    const long K = (long)T * hl * wl;
    if (B == 0 || K == 0) return S2D_OK;
    if (K >= (1L << 31) - 8) return S2D_ERR_ARG;
    if (s2d_zero_async(unmasked, sizeof(uint32_t) * QW * B, stream) != S2D_OK) return S2D_ERR_LAUNCH;
    static const int dword_taps = s2d_env_int("S2D_ATTN_MASK_DWORD_TAPS", 0);
    if (dword_taps && !compact) {          // regression variant (tests only), see attn_mask_kernel_dword_taps
        hipLaunchKernelGGL(attn_mask_kernel_dword_taps, dim3(cdiv(K, 8), B), dim3(256), 0, stream, mask_logits, ldq, Q, T, hm, wm, hl, wl,
                           bits, unmasked);
        S2D_CHECK_LAUNCH();
        return S2D_OK;
    }
    hipLaunchKernelGGL(attn_mask_kernel<false>, dim3(cdiv(K, 8), B), dim3(256), 0, stream, mask_logits, ldq, Q, T, hm, wm, hl,
                       wl, bits, unmasked, compact);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

long s2d_attn_workspace_floats(int B, int H, int K)
{
    const int tiles = (K + KT - 1) / KT;
    int S = tiles / 4; if (S < 1) S = 1; if (S > 32) S = 32;   // 64 / 128 splits measured slower (merge + per-workgroup fixed cost)
    return (long)B * H * S * (32 * 128 + 2 * 128);
}

static int attn_bwd_splits(int K)
{
    const int tiles = (K + BT - 1) / BT;
    int S = tiles / 4; if (S < 1) S = 1; if (S > 64) S = 64;
    return S;
}

long s2d_attn_backward_workspace_floats(int B, int H, int K) { return (long)B * H * attn_bwd_splits(K) * 128 * 32; }

int s2d_masked_attn_backward_strided_f32(const float *q, const float *k, const float *v, long ldk, long ldv, const uint32_t *bits,
                                         const uint32_t *unmasked, const float *out, const float *lse, const float *dout, int B, int Q, int K,
                                         int C, int H, float *workspace, float *dq, float *dk, long lddk, float *dv, long lddv, hipStream_t stream)
{
    if (Q > 128 || Q <= 0 || C != H * 32 || K <= 0 || ldk < C || ldv < C || (ldk & 3) || (ldv & 3) || lddk < C || lddv < C || (lddk & 3) || (lddv & 3) ||
        ((reinterpret_cast<uintptr_t>(dk) | reinterpret_cast<uintptr_t>(dv)) & 15))
        return S2D_ERR_ARG;
    if (B == 0) return S2D_OK;
    AttnBwdParams p;
    p.q = q; p.k = k; p.v = v; p.o = out; p.dout = dout; p.lse = lse; p.ldk = ldk; p.ldv = ldv; p.bits = bits; p.unmasked = unmasked;
    p.Q = Q; p.K = K; p.C = C; p.H = H;
    p.S = attn_bwd_splits(K);
    const int tiles = (K + BT - 1) / BT;
    p.tiles_per_split = (tiles + p.S - 1) / p.S;
    p.qscale = 0.17677669529663687f * 1.4426950408889634f;
    p.dk = dk; p.dv = dv; p.dq_part = workspace; p.lddk = lddk; p.lddv = lddv;
    static const int mfma = s2d_env_int("S2D_ATTN_BWD_MFMA", 1);      // 0: the two scalar fp32 kernels (A/B runs, tests)
    if (mfma) {
        static S2dDevOnce attr;
        if (!attr.done()) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(attn_bwd_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)sizeof(AttnBwdLds)) != hipSuccess)
                return S2D_ERR_LAUNCH;
            attr.mark();
        }
        const int tiles32 = (K + KT - 1) / KT;
        p.tiles_per_split = (tiles32 + p.S - 1) / p.S;
        hipLaunchKernelGGL(attn_bwd_mfma_kernel, dim3(p.S, H, B), dim3(256), sizeof(AttnBwdLds), stream, p);
    } else {
        hipLaunchKernelGGL(attn_bwd_kv_kernel, dim3(tiles, H, B), dim3(256), 0, stream, p);
        hipLaunchKernelGGL(attn_bwd_q_kernel, dim3(p.S, H, B), dim3(256), 0, stream, p);
    }
    const long total = (long)B * Q * C;
    hipLaunchKernelGGL(attn_bwd_merge_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, workspace, B, Q, C, H, p.S,
                       0.17677669529663687f, dq);      // dS carries natural-scale probabilities; dQ = dS K / sqrt(d)
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

int s2d_masked_attn_backward_f32(const float *q, const float *k, const float *v, long ldk, long ldv, const uint32_t *bits,
                                 const uint32_t *unmasked, const float *out, const float *lse, const float *dout, int B, int Q, int K,
                                 int C, int H, float *workspace, float *dq, float *dk, float *dv, hipStream_t stream)
{
    return s2d_masked_attn_backward_strided_f32(q, k, v, ldk, ldv, bits, unmasked, out, lse, dout, B, Q, K, C, H, workspace, dq, dk, C, dv, C, stream);
}

int s2d_masked_attn_f32(const float *q, const float *k, const float *v, long ldk, long ldv, const uint32_t *bits,
                        const uint32_t *unmasked, int B, int Q, int K, int C, int H, float *workspace, float *out, float *lse,
                        hipStream_t stream)
{
    if (Q > 128 || Q <= 0 || C != H * 32 || K <= 0 || ldk < C || ldv < C || (ldk & 3) || (ldv & 3)) return S2D_ERR_ARG;
    if (B == 0) return S2D_OK;
    const int tiles = (K + KT - 1) / KT;
    int S = tiles / 4; if (S < 1) S = 1; if (S > 32) S = 32;   // 64 / 128 splits measured slower (merge + per-workgroup fixed cost)
    AttnParams p;
    p.q = q; p.k = k; p.v = v; p.bits = bits; p.unmasked = unmasked;
    p.ldk = ldk; p.ldv = ldv;
    p.Q = Q; p.K = K; p.C = C; p.H = H; p.S = S; p.tiles_per_split = (tiles + S - 1) / S;
    p.wo = workspace;
    p.wm = workspace + (long)B * H * S * 32 * 128;
    p.wl = p.wm + (long)B * H * S * 128;
    p.qscale = 0.17677669529663687f * 1.4426950408889634f;  // 1/sqrt(32) * log2(e)
    hipLaunchKernelGGL(cross_attn_kernel, dim3(S, H, B), dim3(256), 0, stream, p);
    const long total = (long)B * H * 32 * 128;
    hipLaunchKernelGGL(attn_merge_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, p.wo, p.wm, p.wl, B, Q, C, H, S, out, lse);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
