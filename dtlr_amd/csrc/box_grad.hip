// Gradient of the shared box head (bbox_embed: Linear 256 -> 256, ReLU, Linear 256 -> 256, ReLU, Linear 256 -> 4) with the trunk frozen
// (dtlr_amd/adapt.py; include/dtlr_boxgrad.h states the entry points).
//   dtlr_box_refine_grad   dboxes -> the gradients at the MLP's outputs, through the final sigmoid (dz) and, for "look forward twice",
//                          through inverse_sigmoid(r_l) and the sigmoid that made r_l (du): elementwise, all outputs in one launch
//   dtlr_box_mlp_grad      sum over A applications (x_a, dy_a) of the MLP's parameter gradient.  Four launches:
//     1. W0, W1 -> their transposes in the workspace, so that every GEMM below reads its weight coalesced along the output index;
//     2. one workgroup per tile of 32 listed rows of one application: a tile without a non-zero dy leaves live[tile] = 0 and ends.
//        Otherwise the tile's x goes to LDS ([k][row], fp32) and each of the 256 threads owns one output column for the 32 rows:
//          h0 = relu(W0 x + b0), h1 = relu(W1 h0 + b1), da1 = [a1 > 0] W2^T dy, da0 = [a0 > 0] W1^T da1
//        three 32 x 256 x 256 products, the weight streamed from L2 (512 KB + 256 KB, resident: LDS could hold neither), the
//        activations broadcast from LDS, sums in fp32 over blocks of 32 terms added in order.  x, h0, h1, da0, da1, dy of the tile go
//        to the workspace, compacted: row (tile, r).
//     3. dW0 = da0^T x, dW1 = da1^T h0, dW2 = dy^T h1 with their bias sums: dtlr_head_grad's tile routine (head_grad_tile.h) over the
//        compacted rows, the three products as blockIdx.z of one launch, dead tiles skipped by their live flag;
//     4. the splits' partials added in split order in fp64 into the flat gradient.
//   Only matched queries carry a non-zero dy (about T of 900 rows a line and output), so the caller hands a row list built from the
//   matcher's match_q: a compacted list costs no scan on the device -- match_q IS the list, its -1 entries (lines with fewer targets
//   than Tmax) are holes that sit together at the end of each line and mostly fill whole tiles, which are skipped.  Skipping at tile
//   granularity alone would not do: with 60 of 900 rows live, two thirds of all 32-row tiles of the dense order hold a live row.
#include "dtlr_common.h"
#include "grad_rows.h"
#include "head_grad_tile.h"
#include "../../include/dtlr_boxgrad.h"

namespace dtlr {

constexpr long BG_NW = (long)GR_D * GR_D;
constexpr long BG_OFF_W0 = 0, BG_OFF_W1 = BG_NW + GR_D, BG_OFF_W2 = 2 * (BG_NW + GR_D);
static_assert(BG_OFF_W2 + 4 * GR_D + 4 == DTLR_BOX_GRAD_FLOATS, "flat gradient layout");
static_assert(GR_TR == 32 && GR_TR == HG_MK, "one mask bit a row, one stage of the d^T x products a tile");

__global__ __launch_bounds__(256) void box_refine_grad_kernel(const float* __restrict__ g, const float* __restrict__ p, const float* __restrict__ r,
                                                              float* __restrict__ dz, float* __restrict__ du, long n, long total, float eps)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float gv = g[i], pv = p[i];
    const float z = gv == 0.f ? 0.f : gv * (pv * (1.f - pv));
    dz[i] = z;
    if (i >= n) {                                               // output l >= 1: through isg(r_l) and r_l = sigmoid(u)
        float d = 0.f;
        if (z != 0.f) {
            const float x = r[i];
            const bool lo = x > eps, hi = 1.f - x > eps;        // (1 / x + 1 / (1 - x)) x (1 - x) = 1: no rounding where neither clamp binds
            d = lo && hi ? z : lo ? z * (1.f - x) : hi ? z * x : 0.f;
        }
        du[i - n] = d;
    }
}

struct BgApps { const void* x[DTLR_BOX_GRAD_MAX_APPS]; const float* dy[DTLR_BOX_GRAD_MAX_APPS]; };

// the workspace of one call
struct BgWs { float *W0T, *W1T, *Xc, *H0c, *H1c, *DA0c, *DA1c, *DYc, *part0, *part1, *part2; int* live; double *pb0, *pb1, *pb2; long bytes; };
static inline BgWs bg_ws(float* ws, long Rp, int splits)
{
    BgWs w;
    const long ntiles = Rp / GR_TR, nlive = (ntiles + 3) / 4 * 4;
    float* p = ws;
    w.W0T = p; p += BG_NW;
    w.W1T = p; p += BG_NW;
    w.live = reinterpret_cast<int*>(p); p += nlive;
    w.Xc = p; p += Rp * GR_D;
    w.H0c = p; p += Rp * GR_D;
    w.H1c = p; p += Rp * GR_D;
    w.DA0c = p; p += Rp * GR_D;
    w.DA1c = p; p += Rp * GR_D;
    w.DYc = p; p += Rp * 4;
    w.part0 = p; p += (long)splits * BG_NW;
    w.part1 = p; p += (long)splits * BG_NW;
    w.part2 = p; p += (long)splits * 4 * GR_D;                // every count above is a multiple of 4 floats: p stays 16-byte aligned
    double* q = reinterpret_cast<double*>(p);
    w.pb0 = q; q += (long)splits * GR_D;
    w.pb1 = q; q += (long)splits * GR_D;
    w.pb2 = q; q += (long)splits * 4;
    w.bytes = (long)(reinterpret_cast<char*>(q) - reinterpret_cast<char*>(ws));
    return w;
}

__global__ __launch_bounds__(256) void box_mlp_transpose_kernel(const float* __restrict__ W0, const float* __restrict__ W1,
                                                                float* __restrict__ W0T, float* __restrict__ W1T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;               // grid: 2 * 256 blocks ; element (k, n) of a transpose
    const int which = i >> 16, e = i & 0xffff, k = e >> 8, n = e & 255;
    (which ? W1T : W0T)[e] = (which ? W1 : W0)[n * GR_D + k];
}

// acc[r] = sum_k Wt[k][n] buf[k][r] over the 256 rows of a transposed weight: the stages of 32 terms added in order in fp32, 32-bit
// indices (grad_rows.h)
__device__ __forceinline__ void bg_matvec(const float* __restrict__ Wt, const float* buf, float (&acc)[GR_TR], int n)
{
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) acc[r] = 0.f;
    gr_mac<float, false, int>(Wt, GR_D, n, true, buf, GR_D, GR_D, acc);
}

// grid: one workgroup a tile of 32 list entries of one application ; dynamic LDS 2 x [256][GR_LD] floats
__global__ __launch_bounds__(256) void box_mlp_rows_kernel(BgApps apps, const int* __restrict__ rows, long M, long R, long Rpad, int x_h16,
                                                           const float* __restrict__ W0T, const float* __restrict__ b0,
                                                           const float* __restrict__ W1T, const float* __restrict__ b1,
                                                           const float* __restrict__ W1, const float* __restrict__ W2,
                                                           int* __restrict__ live, float* __restrict__ Xc, float* __restrict__ H0c,
                                                           float* __restrict__ H1c, float* __restrict__ DA0c, float* __restrict__ DA1c,
                                                           float* __restrict__ DYc)
{
    extern __shared__ __attribute__((aligned(16))) float bg_lds[];
    float* bufA = bg_lds;
    float* bufB = bg_lds + GR_D * GR_LD;
    __shared__ __attribute__((aligned(16))) float dys[GR_TR][4];
    __shared__ long ridx[GR_TR];
    const long tile = blockIdx.x, tiles_app = Rpad / GR_TR;
    const int a = (int)(tile / tiles_app), n = threadIdx.x;
    const long k0 = (tile - (long)a * tiles_app) * GR_TR;
    int nz = 0;
    if (n < GR_TR) {
        const long k = k0 + n;
        long idx = -1;
        if (k < R) idx = rows ? (long)rows[(long)a * R + k] : k;
        if (idx < 0 || idx >= M) idx = -1;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx >= 0) d = *reinterpret_cast<const float4*>(apps.dy[a] + idx * 4);
        nz = d.x != 0.f || d.y != 0.f || d.z != 0.f || d.w != 0.f;
        ridx[n] = nz ? idx : -1;                                // a row without a gradient is not read
        *reinterpret_cast<float4*>(dys[n]) = d;
    }
    if (!__syncthreads_or(nz)) {                                // workgroup-uniform
        if (n == 0) live[tile] = 0;
        return;
    }
    if (n == 0) live[tile] = 1;
    const long base = tile * GR_TR;                             // the tile's rows in the compacted buffers
    if (n < GR_TR * 4) DYc[base * 4 + n] = dys[n >> 2][n & 3];
    {                                                           // not gr_load: through it the compiler schedules this loop differently
        const float* xf = static_cast<const float*>(apps.x[a]);
        const uint16_t* xh = static_cast<const uint16_t*>(apps.x[a]);
#pragma unroll 4
        for (int r = 0; r < GR_TR; ++r) {
            const long idx = ridx[r];
            float v = 0.f;
            if (idx >= 0) v = x_h16 ? bf16_to_f32(xh[idx * GR_D + n]) : xf[idx * GR_D + n];
            bufA[n * GR_LD + r] = v;
            Xc[(base + r) * GR_D + n] = v;
        }
    }
    __syncthreads();
    float acc[GR_TR];
    unsigned m0 = 0;
    bg_matvec(W0T, bufA, acc, n);
    {
        const float bn = b0[n];
#pragma unroll
        for (int r = 0; r < GR_TR; ++r) {
            float v = acc[r] + bn;
            if (v > 0.f) m0 |= 1u << r; else v = 0.f;
            bufB[n * GR_LD + r] = v;
            H0c[(base + r) * GR_D + n] = v;
        }
    }
    __syncthreads();
    bg_matvec(W1T, bufB, acc, n);
    {
        const float bn = b1[n];
        const float w20 = W2[n], w21 = W2[GR_D + n], w22 = W2[2 * GR_D + n], w23 = W2[3 * GR_D + n];
#pragma unroll
        for (int r = 0; r < GR_TR; ++r) {
            const float v = acc[r] + bn;
            const bool pos = v > 0.f;
            H1c[(base + r) * GR_D + n] = pos ? v : 0.f;
            const float4 d = *reinterpret_cast<const float4*>(dys[r]);
            const float dh = fmaf(d.w, w23, fmaf(d.z, w22, fmaf(d.y, w21, d.x * w20)));
            const float da = pos ? dh : 0.f;
            DA1c[(base + r) * GR_D + n] = da;
            bufA[n * GR_LD + r] = da;                           // bufA's x was last read before the barrier above
        }
    }
    __syncthreads();
    bg_matvec(W1, bufA, acc, n);                                // dh0[r][n] = sum_m W1[m][n] da1[r][m]
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) DA0c[(base + r) * GR_D + n] = ((m0 >> r) & 1u) ? acc[r] : 0.f;
}

struct BgProb { const float* G; const float* X; float* part; double* partb; int C; };

// grid (16, splits, 3): the three d^T x products over the compacted rows
__global__ __launch_bounds__(256) void box_mlp_partial_kernel(BgProb p0, BgProb p1, BgProb p2, const int* __restrict__ live, long Rp, long chunk)
{
    __shared__ __attribute__((aligned(16))) float Gs[HG_MK][HG_TC];
    __shared__ __attribute__((aligned(16))) float Xs[HG_MK][HG_TD];
    const BgProb p = blockIdx.z == 0 ? p0 : blockIdx.z == 1 ? p1 : p2;
    const int tiles_d = GR_D / HG_TD;
    if ((int)blockIdx.x >= ((p.C + HG_TC - 1) / HG_TC) * tiles_d) return;
    hg_partial_tile(Gs, Xs, p.G, p.X, p.part, p.partb, live, Rp, p.C, GR_D, tiles_d, chunk, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(256) void box_mlp_reduce_kernel(BgProb p0, BgProb p1, BgProb p2, float* __restrict__ grad, int splits)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= DTLR_BOX_GRAD_FLOATS) return;
    const int z = i < BG_OFF_W1 ? 0 : i < BG_OFF_W2 ? 1 : 2;
    const BgProb p = z == 0 ? p0 : z == 1 ? p1 : p2;
    const long off = z == 0 ? BG_OFF_W0 : z == 1 ? BG_OFF_W1 : BG_OFF_W2, nW = (long)p.C * GR_D;
    hg_reduce(p.part, p.partb, grad + off, grad + off + nW, nW, p.C, splits, i - off);
}

struct BgPlan { long R, Rpad, Rp; int splits; long chunk; bool ok; };
static inline BgPlan bg_plan(int A, long M, int R)
{
    BgPlan q{};
    if (A < 1 || A > DTLR_BOX_GRAD_MAX_APPS || M <= 0) return q;
    q.R = R > 0 ? (long)R : M;
    q.Rpad = (q.R + GR_TR - 1) / GR_TR * GR_TR;
    q.Rp = (long)A * q.Rpad;
    if (q.Rp > 0x7fffffffl || M > 0x7fffffffl) return q;
    const HgPlan h = hg_plan(q.Rp, GR_D, GR_D);
    q.splits = h.splits;
    q.chunk = h.chunk;
    q.ok = true;
    return q;
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_box_refine_grad(const float* dboxes, const float* pred_boxes, const float* refs, float* dz, float* du, int L, long M,
                                    float eps, void* stream)
{
    clear_stale_error();
    if (!dboxes || !pred_boxes || !refs || !dz || L <= 0 || M <= 0) return DTLR_EINVAL;
    if (L > 1 && !du) return DTLR_EINVAL;
    if (M > (1l << 40) / L) return DTLR_ESHAPE;
    const long n = M * 4, total = n * L;
    if ((total + 255) / 256 > 0x7fffffffl) return DTLR_ESHAPE;
    return launch<box_refine_grad_kernel>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dboxes, pred_boxes, refs,
                                          dz, du, n, total, eps);
}

extern "C" long dtlr_box_mlp_grad_workspace_bytes(int A, long M, int R)
{
    const BgPlan q = bg_plan(A, M, R);
    if (!q.ok) return 0;
    return bg_ws(nullptr, q.Rp, q.splits).bytes;
}

extern "C" int dtlr_box_mlp_grad(const void* x_ptrs, const void* dy_ptrs, const int* rows, int A, long M, int R, int x_dtype,
                                 const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                                 float* grad, void* workspace, void* stream)
{
    clear_stale_error();
    (void)b2;                                                   // the last bias does not enter its own gradient
    if (!x_ptrs || !dy_ptrs || !W0 || !b0 || !W1 || !b1 || !W2 || !b2 || !grad || !workspace) return DTLR_EINVAL;
    if (A < 1 || M <= 0 || (rows && R <= 0)) return DTLR_EINVAL;
    if (A > DTLR_BOX_GRAD_MAX_APPS) return DTLR_ESHAPE;
    if (!is_f32_or_h16(x_dtype)) return DTLR_EDTYPE;
    const BgPlan q = bg_plan(A, M, rows ? R : 0);
    if (!q.ok) return DTLR_ESHAPE;
    if (misaligned(workspace, 15)) return DTLR_EINVAL;
    BgApps apps{};
    for (int a = 0; a < A; ++a) {
        apps.x[a] = static_cast<const void* const*>(x_ptrs)[a];
        apps.dy[a] = static_cast<const float* const*>(dy_ptrs)[a];
        if (!apps.x[a] || !apps.dy[a] || misaligned(apps.dy[a], 15)) return DTLR_EINVAL;
        if (misaligned(apps.x[a], x_dtype == DTLR_F32 ? 3 : 1)) return DTLR_EINVAL;
    }
    const BgWs w = bg_ws(static_cast<float*>(workspace), q.Rp, q.splits);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = launch<box_mlp_transpose_kernel>(dim3(512), dim3(256), 0, st, W0, W1, w.W0T, w.W1T)) return rc;
    const size_t lds = (size_t)2 * GR_D * GR_LD * sizeof(float);
    if (int rc = launch<box_mlp_rows_kernel>(dim3((unsigned)(q.Rp / GR_TR)), dim3(256), lds, st, apps, rows, M, q.R, q.Rpad,
                                             (int)(x_dtype != DTLR_F32), (const float*)w.W0T, b0, (const float*)w.W1T, b1, W1, W2, w.live,
                                             w.Xc, w.H0c, w.H1c, w.DA0c, w.DA1c, w.DYc)) return rc;
    const BgProb p0{w.DA0c, w.Xc, w.part0, w.pb0, GR_D}, p1{w.DA1c, w.H0c, w.part1, w.pb1, GR_D}, p2{w.DYc, w.H1c, w.part2, w.pb2, 4};
    if (int rc = launch<box_mlp_partial_kernel>(dim3(16, (unsigned)q.splits, 3), dim3(256), 0, st, p0, p1, p2, (const int*)w.live, q.Rp, q.chunk)) return rc;
    return launch<box_mlp_reduce_kernel>(dim3((DTLR_BOX_GRAD_FLOATS + 255) / 256), dim3(256), 0, st, p0, p1, p2, grad, q.splits);
}
