// The 32-row x 256-column tile product shared by the row kernels of dtlr_box_mlp_grad (box_grad.hip) and of the decoder tail's gradient
// (tail_grad.hip: tg_rows_gemm_kernel, tg_box_dx_kernel): thread n owns one output column for the tile's 32 rows, the activations lie in
// LDS transposed ([k][row], pitch GR_LD) and are broadcast from there, the weight is read k-major, coalesced over n.  Plain fp32 FMAs,
// 32 terms a stage in an fp32 accumulator; the stages are added in order into an accumulator of the caller's type.  No launches here.
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

}  // namespace dtlr
