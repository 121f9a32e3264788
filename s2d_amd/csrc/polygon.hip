// Polygon annotations -> bit planes on the device (s2d_amd/data/image_clip.py): the polygon half of a COCO image annotation
// file, written in the layout s2d_rle_decode_bits writes (row-major flat pixel i -> word i/32, bit i%32, tail bits zero), so
// that the RLE and the polygon instances of one image go through s2d_aug_warp_mask_bits together.
//
// Fill rule (the project's own; pycocotools' frPoly -- a 5x-upsampled boundary walk -- is not restated): pixel
// (x, y) of a plane is set iff its centre (x + 0.5, y + 0.5) is inside at least one of the plane's polygons by the even-odd rule.
// An edge (x0, y0)-(x1, y1) counts for a centre (cx, cy) when (y0 <= cy) != (y1 <= cy) and
// cx < x0 + (cy - y0) * (x1 - x0) / (y1 - y0), in float32 in this order; a polygon closes from its last vertex to its first.
//
// One lane owns one output word: 32 consecutive pixels, i.e. one or two row segments (more where W < 32).  On a row the
// crossing abscissa of an edge is one number, so the centres it counts for are a PREFIX of the segment: the lane computes
// the crossing once per (edge, row segment), turns it into a prefix length n = #{x in segment : x + 0.5 < crossing} and
// toggles those n bits of the polygon's parity word.  At a polygon's last edge the parity word is OR-ed into the plane's word.
// A workgroup is one plane and PT consecutive words (stores of a wave are 256 contiguous bytes); the plane's edges are staged
// through LDS PT at a time, every lane of a wave reads the same edge (an LDS broadcast), so the vertex count has no cap.
// Each word is stored once by its lane: no atomics, no read-modify-write, and no zero fill in front of the kernel.
#include "common.h"

namespace {

constexpr int PT = 256;    // threads = words per workgroup = edges per LDS chunk

__global__ __launch_bounds__(PT) void polygons_to_bits_kernel(const float2 *__restrict__ verts, int V, const int *__restrict__ poly_off,
                                                              int NP, const int *__restrict__ plane_off, const int *__restrict__ dst_plane,
                                                              int rows, int H, int W, long wpp, uint32_t *__restrict__ bits)
{
    __shared__ float4 edge[PT];      // x0, y0, x1, y1
    __shared__ int last[PT];         // 1: the last edge of its polygon
    const int p = blockIdx.y;
    const long w = (long)blockIdx.x * PT + threadIdx.x;
    const long hw = (long)H * W;
    const long px = w * 32;
    const int nbit = px >= hw ? 0 : (hw - px < 32 ? (int)(hw - px) : 32);
    const int row0 = (int)(px / W), col0 = (int)(px - (long)row0 * W);

    // the plane's polygons [qa, qb) and their vertices [va, vb): clamped, so that no table can index outside verts
    const int qa = min(max(plane_off[p], 0), NP), qb = min(max(plane_off[p + 1], qa), NP);
    const int va = min(max(poly_off[qa], 0), V), vb = min(max(poly_off[qb], va), V);

    uint32_t acc = 0u, par = 0u;
    for (int v0 = va; v0 < vb; v0 += PT) {
        const int n = min(PT, vb - v0);
        __syncthreads();                                     // the previous chunk has been walked
        if ((int)threadIdx.x < n) {
            const int v = v0 + threadIdx.x;
            int lo = qa, hi = qb;                            // the polygon of vertex v: the largest q with poly_off[q] <= v
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (poly_off[mid] <= v) lo = mid; else hi = mid;
            }
            const int s = max(poly_off[lo], va), e = min(poly_off[lo + 1], vb);
            float4 ed = make_float4(0.f, 0.f, 0.f, 0.f);     // y0 == y1: counts for no centre
            if (v >= s && v < e && e - s >= 3) {
                const float2 a = verts[v], b = verts[v + 1 == e ? s : v + 1];
                ed = make_float4(a.x, a.y, b.x, b.y);
            }
            edge[threadIdx.x] = ed;
            last[threadIdx.x] = v + 1 >= e;
        }
        __syncthreads();
        if (nbit == 0) continue;
        for (int i = 0; i < n; ++i) {
            const float4 ed = edge[i];
            int y = row0, c = col0, used = 0;
            while (used < nbit) {
                const int len = min(nbit - used, W - c);
                const float cy = (float)y + 0.5f;
                if ((ed.y <= cy) != (ed.w <= cy)) {
                    const float xi = ed.x + (cy - ed.y) * (ed.z - ed.x) / (ed.w - ed.y);
                    // k = #{integer x : x + 0.5 < xi}, wanted inside [c, c + len] only: an estimate clamped to one past either
                    // end (a NaN crossing gives the low end), then made exact with the rule's own comparison
                    float kf = fminf(fmaxf(ceilf(xi - 0.5f), (float)(c - 1)), (float)(c + len + 1));
                    int k = (int)kf;
                    if (!((float)(k - 1) + 0.5f < xi)) --k;
                    if ((float)k + 0.5f < xi) ++k;
                    const int m = min(max(k - c, 0), len);
                    const uint32_t run = m >= 32 ? 0xFFFFFFFFu : ((1u << m) - 1u);
                    par ^= run << used;
                }
                used += len; c = 0; ++y;
            }
            if (last[i]) { acc |= par; par = 0u; }
        }
    }
    acc |= par;
    const int d = dst_plane ? dst_plane[p] : p;
    if (w < wpp && d >= 0 && d < rows) bits[(long)d * wpp + w] = acc;
}

// offsets of a table [n + 1]: non-negative, non-decreasing, the last one within `limit`
bool monotone(const int *off, int n, int limit)
{
    if (off[0] < 0 || off[n] > limit) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

}  // namespace

extern "C" {

int s2d_polygons_to_bits(const float *verts, int V, const int *poly_off, const int *poly_off_host, int NP, const int *plane_off,
                         const int *plane_off_host, int P, const int *dst_plane, int rows, int H, int W, uint32_t *bits,
                         hipStream_t stream)
{
    if (V < 0 || NP < 0 || P < 0 || P >= 65536 || rows < 0 || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return S2D_ERR_ARG;
    const long wpp = ((long)H * W + 31) / 32;
    if ((long)rows * wpp >= (1L << 31) || (!dst_plane && rows < P)) return S2D_ERR_ARG;
    if (P == 0) return S2D_OK;
    if (!poly_off_host || !plane_off_host || !monotone(poly_off_host, NP, V) || !monotone(plane_off_host, P, NP)) return S2D_ERR_ARG;
    hipLaunchKernelGGL(polygons_to_bits_kernel, dim3(cdiv(wpp, PT), P), dim3(PT), 0, stream, reinterpret_cast<const float2 *>(verts), V,
                       poly_off, NP, plane_off, dst_plane, rows, H, W, wpp, bits);
    S2D_CHECK_LAUNCH();
    return S2D_OK;
}

}  // extern "C"
