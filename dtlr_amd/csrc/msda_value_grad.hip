// Gradient of the deformable attention with respect to `value`: output 1 of its backward (include/dtlr_msdagrad.h states the entry point,
// DESIGN.md section 25 the scheme).  The reference scatters every sample's four corner terms with float atomics; here the scatter is a
// gather by ownership:
//   workgroup = 4 wavefronts = one tile of 64 consecutive rows of one (image, head) of grad_value [N, S, 8, 32]
//   lane      = one pixel, its 32 channel sums in registers
//   wavefront = one fixed quarter of the queries, [w ceil(Lq / 4), (w + 1) ceil(Lq / 4))
// For each level the tile meets, a wavefront walks its queries' samples of that level in ascending (q, p), 64 at a time: every lane takes
// one sample, forms msda_grad_geo.h's point for it (the one cross_grad.hip's kernels form) and tests its corners against the tile; a
// ballot gives the hits.  The hits are taken
// in ascending order: the sample's (y0, x0, ly, lx, attn) are broadcast, its grad_out row is read through a wavefront-uniform address, and
// every lane adds weight x row, the weight being zero unless the lane's pixel is one of the four corners.  The four wavefronts' sums meet
// in LDS and are added in segment order by the first, which stores each row once.  No atomics; the order of every sum depends on Lq alone.
#include "gfx950_prims.h"
#include "msda_grad_geo.h"
#include "../../include/dtlr_msdagrad.h"

namespace dtlr {

constexpr int VG_TILE = DTLR_VGRAD_TILE, VG_SEG = DTLR_VGRAD_SEGMENTS, VG_HD = 32, VG_ROW = 256;
static_assert(VG_TILE == 64 && VG_SEG == 4, "a lane a pixel, a wavefront a segment, 256 threads");

__device__ __forceinline__ int vg_bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float vg_bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// grid: N * 8 * tiles workgroups, tiles = ceil(S / 64).  loc [N,Lq,8,4,4,2], attn [N,Lq,8,4,4], go [N,Lq,256] -> gv [N,S,8,32]
__global__ __launch_bounds__(256) void vg_value_grad_kernel(const long* __restrict__ shapes, const long* __restrict__ lsi,
                                                            const float* __restrict__ loc, const float* __restrict__ attn,
                                                            const float* __restrict__ go, int S, int Lq, int tiles, float* __restrict__ gv)
{
    __shared__ float red[(VG_SEG - 1) * VG_HD * VG_TILE];          // 24 KB: segments 1..3, [segment][channel][lane]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const int nh = (int)(blockIdx.x / (unsigned)tiles);
    const int h = nh & 7, n = nh >> 3;
    const int f0 = tile * VG_TILE, f = f0 + lane;                   // the lane's row of the flat map ; f >= S: nothing stored
    const int segq = (Lq + VG_SEG - 1) / VG_SEG;
    const int q0 = min(wave * segq, Lq), q1 = min(q0 + segq, Lq);
    const int j0 = q0 * 4, j1 = q1 * 4;                             // this wavefront's samples of a level: j = q * 4 + p
    float acc[VG_HD];
#pragma unroll
    for (int c = 0; c < VG_HD; ++c) acc[c] = 0.f;
    bool owned = false;                                             // a row belongs to the first level that claims it
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
        // the level's entry of the table, made safe as geo_levels makes it: 1 <= H, W <= 2^15, 0 <= start <= S - 1 (S < 2^23: all of this fits an int)
        const int H = (int)geo_clamp(shapes[2 * l], 1, 32768), W = (int)geo_clamp(shapes[2 * l + 1], 1, 32768);
        const int st = (int)geo_clamp(lsi[l], 0, (long)S - 1);
        const int HW = H * W;
        const bool mine = !owned && (unsigned)(f - st) < (unsigned)HW;
        owned = owned || mine;
        if (st >= f0 + VG_TILE || st + HW <= f0) continue;           // workgroup-uniform: the tile does not meet the level
        const int pl = mine ? f - st : 0;
        const int ypix = mine ? pl / W : -4, xpix = mine ? pl % W : -4;       // -4: no corner (y0, x0 >= -1) is ever 0 or 1 below it
        for (int base = j0; base < j1; base += 64) {
            const bool have = base + lane < j1;
            const int j = min(base + lane, j1 - 1);
            const long si = ((long)n * Lq + (j >> 2)) * 8 + h;
            const int lp = l * 4 + (j & 3);
            const float2 c = *reinterpret_cast<const float2*>(loc + si * 32 + lp * 2);
            const float a = attn[si * 16 + lp];
            const GeoPoint pt = geo_point(c.x, c.y, H, W);
            const int y0 = pt.y0, x0 = pt.x0;
            bool hit = false;
#pragma unroll
            for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                for (int cx = 0; cx < 2; ++cx) {
                    const int yy = y0 + cy, xx = x0 + cx;
                    hit = hit || ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W && (unsigned)(st + yy * W + xx - f0) < (unsigned)VG_TILE);
                }
            unsigned long long m = __ballot(hit && have && pt.inside);
            while (m) {                                             // wavefront-uniform: ascending samples
                const int i = __builtin_ctzll(m);
                m &= m - 1;
                const int sy0 = vg_bcast(y0, i), sx0 = vg_bcast(x0, i);
                const float slh = vg_bcast(pt.lh, i), slw = vg_bcast(pt.lw, i), sa = vg_bcast(a, i);
                const int qi = __builtin_amdgcn_readfirstlane((base + i) >> 2);
                const float* __restrict__ g = go + ((long)n * Lq + qi) * VG_ROW + h * VG_HD;
                const int dy = ypix - sy0, dx = xpix - sx0;
                const float wy = dy == 0 ? 1.f - slh : (dy == 1 ? slh : 0.f);
                const float wx = dx == 0 ? 1.f - slw : (dx == 1 ? slw : 0.f);
                const float w = sa * (wy * wx);
#pragma unroll
                for (int k = 0; k < VG_HD; ++k) acc[k] = fmaf(w, g[k], acc[k]);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < VG_HD; ++k) red[((wave - 1) * VG_HD + k) * VG_TILE + lane] = acc[k];
    }
    __syncthreads();
    if (wave > 0 || f >= S) return;
#pragma unroll
    for (int s = 0; s < VG_SEG - 1; ++s)                            // ((s0 + s1) + s2) + s3
#pragma unroll
        for (int k = 0; k < VG_HD; ++k) acc[k] += red[(s * VG_HD + k) * VG_TILE + lane];
    float4* out = reinterpret_cast<float4*>(gv + ((long)n * S + f) * VG_ROW + h * VG_HD);
#pragma unroll
    for (int k = 0; k < VG_HD / 4; ++k) out[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_msda_value_grad(const long* shapes, const long* lsi, const float* loc, const float* attn, const float* grad_out, int N, int S,
                                    int M, int D, int L, int Lq, int P, float* grad_value, void* stream)
{
    clear_stale_error();
    if (!shapes || !lsi || !loc || !attn || !grad_out || !grad_value) return DTLR_EINVAL;
    if (N <= 0 || S <= 0 || M <= 0 || D <= 0 || L <= 0 || Lq <= 0 || P <= 0) return DTLR_EINVAL;
    if (M != 8 || D != VG_HD || L != 4 || P != 4) return DTLR_ESHAPE;
    if (S >= (1 << 23) || (long)N * Lq > (1l << 31)) return DTLR_ESHAPE;
    const int tiles = (S + VG_TILE - 1) / VG_TILE;
    const long blocks = (long)N * 8 * tiles;
    if (blocks >= (1l << 31)) return DTLR_ESHAPE;
    if (misaligned(loc, 15) || misaligned(attn, 15) || misaligned(grad_out, 15) || misaligned(grad_value, 15)) return DTLR_EINVAL;
    return launch<vg_value_grad_kernel>(dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, shapes, lsi, loc, attn, grad_out, S, Lq, tiles,
                                        grad_value);
}
