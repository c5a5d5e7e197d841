// The 32-row x 256-column tile product shared by the row kernels of dtlr_box_mlp_grad (box_grad.hip), of the decoder tail's gradient
// (tail_grad.hip: tg_rows_gemm_kernel, tg_box_dx_kernel) and of grad_rows.hip (gr_rows_gemm256_kernel): thread n owns one output column for the tile's 32 rows, the activations lie in
// LDS transposed ([k][row], pitch GR_LD) and are broadcast from there, the weight is read k-major, coalesced over n.  Plain fp32 FMAs,
// 32 terms a stage in an fp32 accumulator; the stages are added in order into an accumulator of the caller's type.
// Below it, the three launches that several gradient files make, each kernel defined once in grad_rows.hip: the 32 x 32 transpose
// (tail_grad.hip, cross_grad.hip, self_grad.hip), the LayerNorm forward over rows of 256 and the K = 256 two-stream row product
// (cross_grad.hip, self_grad.hip).  tg_rows_gemm_kernel (runtime K, long weight index, ReLU / mask / accumulate epilogue) has one user
// and stays in tail_grad.hip.
#pragma once
#include "dtlr_common.h"

namespace dtlr {

constexpr int GR_D = 256, GR_TR = 32, GR_LD = 36;             // GR_LD: row pitch of the [k][row] LDS images (16-byte rows, 8 banks apart)

// element i of a row-major matrix of fp32 or (h16) of the library's 16-bit format
__device__ __forceinline__ float gr_load(const void* p, int h16, long i)
{
    return h16 ? bf16_to_f32(static_cast<const uint16_t*>(p)[i]) : static_cast<const float*>(p)[i];
}

// acc[r] += sum_(k < klen) Wt[k][n] buf[k][r], klen % 32 == 0.  Acc: the type the stages are added in (the box head's weight gradient
// keeps fp32, the tail's chain fp64).  Guard: rows k >= kvalid of Wt are not read (buf holds zeros there) and a thread without a column
// (nvalid false) reads no weight at all; without it both arguments are ignored.  Idx: the type Wt's index is formed in -- int where
// klen * ldw is known to fit, which spares the 64-bit address arithmetic.
template <typename Acc, bool Guard, typename Idx>
__device__ __forceinline__ void gr_mac(const float* __restrict__ Wt, Idx ldw, int n, bool nvalid, const float* buf, int klen, int kvalid,
                                       Acc (&acc)[GR_TR])
{
    for (int kc = 0; kc < klen; kc += 32) {
        float c[GR_TR];
#pragma unroll
        for (int r = 0; r < GR_TR; ++r) c[r] = 0.f;
#pragma unroll 4
        for (int k = kc; k < kc + 32; ++k) {
            const float w = (!Guard || (nvalid && k < kvalid)) ? Wt[(Idx)k * ldw + n] : 0.f;
            const float4* row = reinterpret_cast<const float4*>(buf + k * GR_LD);
#pragma unroll
            for (int q = 0; q < GR_TR / 4; ++q) {
                const float4 v = row[q];
                c[4 * q] = fmaf(w, v.x, c[4 * q]);
                c[4 * q + 1] = fmaf(w, v.y, c[4 * q + 1]);
                c[4 * q + 2] = fmaf(w, v.z, c[4 * q + 2]);
                c[4 * q + 3] = fmaf(w, v.w, c[4 * q + 3]);
            }
        }
#pragma unroll
        for (int r = 0; r < GR_TR; ++r) acc[r] += (Acc)c[r];
    }
}

// the 32-row tiles of M rows: the x extent of every row product's grid
inline unsigned gr_tiles(long M) { return (unsigned)((M + GR_TR - 1) / GR_TR); }

// out[m][n] = sum_k (A[m][k] + A2[m][k]) Wt[k][n] + bias[n] + res[m][n], K = 256, m < M, n < N.  A, A2 (optional; both 16-bit when
// a_h16) and res (optional; row pitch N, 16-bit when res_h16) in fp32 or the 16-bit format ; Wt k-major with row pitch ldw ; out has row
// pitch ldo, out2 (optional, row pitch ldo2) receives the same values ; xsum (optional) receives A + A2 in fp32, [M,256].
struct GrRows256 {
    const void* A; const void* A2; int a_h16; long M;
    const float* Wt; int ldw; int N; const float* bias;
    const void* res; int res_h16;
    float* out; int ldo; float* out2; int ldo2; float* xsum;
};

// Each enqueues one launch on `stream` and returns DTLR_OK or DTLR_ELAUNCH (defined in grad_rows.hip).
int gr_transpose(const float* src, float* dst, int R, int C, hipStream_t stream);                     // dst[c][r] = src[r][c], src [R, C]
int gr_layernorm256(const float* x, const float* gamma, const float* beta, float* out, long M, float eps, hipStream_t stream);
int gr_rows_gemm256(const GrRows256& g, hipStream_t stream);

}  // namespace dtlr
