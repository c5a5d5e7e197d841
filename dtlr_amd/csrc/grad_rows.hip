// The kernels that several gradient files launch, each defined once (grad_rows.h declares the three host functions and says who calls
// them): the 32 x 32 transpose that makes a k-major image of a master weight, the LayerNorm forward over rows of 256, and the K = 256
// row product with two input streams that the recomputed forwards of the cross-attention and self-attention blocks run on.  The
// product is grad_rows.h's 32-row tile product (exact fp32 FMAs, 32 terms in fp32, the stages in fp64).
#include "grad_rows.h"

namespace dtlr {

// out[m][n] = sum_k (A[m][k] + A2[m][k]) Wt[k][n] + bias[n] + res[m][n], K = 256 ; A, A2 (optional), res (optional) in fp32 or the 16-bit
// format ; out has row pitch ldo, out2 (optional, row pitch ldo2) receives the same values ; xsum (optional): receives A + A2 in fp32.
// grid (ceil(M / 32), ceil(N / 256)).
__global__ __launch_bounds__(256) void gr_rows_gemm256_kernel(const void* __restrict__ A, const void* __restrict__ A2, int a_h16, long M,
                                                              const float* __restrict__ Wt, int ldw, int N, const float* __restrict__ bias,
                                                              const void* __restrict__ res, int res_h16, float* __restrict__ out, int ldo,
                                                              float* __restrict__ out2, int ldo2, float* __restrict__ xsum)
{
    __shared__ __attribute__((aligned(16))) float As[32 * GR_LD];
    const long m0 = (long)blockIdx.x * GR_TR;
    const int n = (int)blockIdx.y * 256 + threadIdx.x;
    const bool nvalid = n < N;
    const int sr = threadIdx.x >> 3, sk = (threadIdx.x & 7) * 4;
    const long sm = m0 + sr;
    double acc[GR_TR];
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) acc[r] = 0.0;
    for (int kc = 0; kc < GR_D; kc += 32) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kc + sk + j;
            float v = 0.f;
            if (sm < M) {
                v = gr_load(A, a_h16, sm * GR_D + k);
                if (A2) v += gr_load(A2, a_h16, sm * GR_D + k);
                if (xsum && blockIdx.y == 0) xsum[sm * GR_D + k] = v;
            }
            As[(sk + j) * GR_LD + sr] = v;
        }
        __syncthreads();
        gr_mac<double, true, int>(Wt + (long)kc * ldw, ldw, n, nvalid, As, 32, GR_D - kc, acc);
    }
    if (!nvalid) return;
    const double bn = (double)bias[n];
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) {
        const long m = m0 + r;
        if (m >= M) continue;
        double v = acc[r] + bn;
        if (res) v += (double)gr_load(res, res_h16, m * N + n);
        out[m * ldo + n] = (float)v;
        if (out2) out2[m * ldo2 + n] = (float)v;
    }
}

// dst[c][r] = src[r][c], src [R, C].  grid (ceil(C / 32), ceil(R / 32)).
__global__ __launch_bounds__(256) void gr_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C)
{
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) t[j][tx] = src[(long)(r0 + j) * C + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) dst[(long)(c0 + j) * R + r0 + tx] = t[tx][j];
}

// out = LayerNorm(x) over rows of 256: one wavefront a row, statistics fp32 two-pass (as dtlr_ln_backward takes them)
__global__ __launch_bounds__(256) void gr_layernorm256_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ out, long M, float eps)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;                                           // wavefront-uniform
    const float4 t = *reinterpret_cast<const float4*>(x + row * GR_D + 4 * lane);
    float v[4] = {t.x, t.y, t.z, t.w};
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / GR_D);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] -= mean; q += v[j] * v[j]; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / GR_D) + eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] * rstd * gamma[4 * lane + j] + beta[4 * lane + j];      // views of a flat buffer: no alignment
    *reinterpret_cast<float4*>(out + row * GR_D + 4 * lane) = make_float4(v[0], v[1], v[2], v[3]);
}

int gr_transpose(const float* src, float* dst, int R, int C, hipStream_t stream)
{
    return launch<gr_transpose_kernel>(dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32)), dim3(256), 0, stream, src, dst, R, C);
}

int gr_layernorm256(const float* x, const float* gamma, const float* beta, float* out, long M, float eps, hipStream_t stream)
{
    return launch<gr_layernorm256_kernel>(dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, x, gamma, beta, out, M, eps);
}

int gr_rows_gemm256(const GrRows256& g, hipStream_t stream)
{
    return launch<gr_rows_gemm256_kernel>(dim3(gr_tiles(g.M), (unsigned)((g.N + 255) / 256)), dim3(256), 0, stream, g.A, g.A2, g.a_h16, g.M, g.Wt,
                                          g.ldw, g.N, g.bias, g.res, g.res_h16, g.out, g.ldo, g.out2, g.ldo2, g.xsum);
}

}  // namespace dtlr
