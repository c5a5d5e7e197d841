// The class head's training step on the device (dtlr_amd/adapt.py): weight gradient, clip coefficient, AdamW.
//   dtlr_head_grad        dW[C, D] = G^T[C, M] . X[M, D],  db[C] = sum_m G[m, :]      (G = dlogits, X = decoder states)
//   dtlr_grad_norm_scale  L2 norm of a flat fp32 buffer and clip_grad_norm_'s coefficient, left in device memory
//   dtlr_adamw_step       torch.optim.AdamW's update over a flat fp32 parameter buffer, gradient scale read from device memory
//
// dtlr_head_grad: both operands are stored M-major and M is the reduction dimension, so no operand needs a transpose to be read
// coalesced: a stage of 32 rows of G (64 channels) and of X (64 features) goes to LDS as it lies in memory and every thread forms
// the 4 x 4 outer products of its channels and features.  Products and sums are plain fp32 FMAs: exact fp32 products, as the exact
// fp32 MFMA would give, on the vector units -- at C = 166 the whole contraction is 2.4 GFLOP, and the tolerance (4 x the error of an
// fp32 CPU matmul) leaves no room for the 2^-22 operand rounding of the split-fp16 form.  Summation is blocked like a CPU GEMM's: a
// stage's 32 terms in an fp32 accumulator, the stages in an fp64 one (16 fp64 adds per 512 FMAs), so the error is that of the 32-term
// sums alone.  M is split over workgroups so that the grid fills the chip; the partial tiles (fp32; the bias partials fp64) go to the
// caller's workspace and a second kernel adds them in split order -- no float atomics, two runs give the same bits.
#include "dtlr_common.h"
#include "head_grad_tile.h"

namespace dtlr {

// grid (tiles_c * tiles_d, splits): part[split][C][D] and partb[split][C] (head_grad_tile.h: the routine dtlr_box_mlp_grad shares)
__global__ __launch_bounds__(256) void head_grad_partial_kernel(const float* __restrict__ G, const float* __restrict__ X,
                                                                float* __restrict__ part, double* __restrict__ partb,
                                                                long M, int C, int D, int tiles_d, long chunk)
{
    __shared__ __attribute__((aligned(16))) float Gs[HG_MK][HG_TC];
    __shared__ __attribute__((aligned(16))) float Xs[HG_MK][HG_TD];
    hg_partial_tile(Gs, Xs, G, X, part, partb, nullptr, M, C, D, tiles_d, chunk, (int)blockIdx.x, (int)blockIdx.y);
}

// dW | db = the partials added in split order
__global__ __launch_bounds__(256) void head_grad_reduce_kernel(const float* __restrict__ part, const double* __restrict__ partb,
                                                               float* __restrict__ dW, float* __restrict__ db, long nW, int C, int splits)
{
    hg_reduce(part, partb, dW, db, nW, C, splits, (long)blockIdx.x * 256 + threadIdx.x);
}

constexpr int GN_BLOCKS = 256;

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ partial)
{
    __shared__ double red[4];
    double a = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) { const double v = (double)g[i]; a = fma(v, v, a); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), or 1 when max_norm <= 0 ; out[1] = norm
__global__ __launch_bounds__(64) void norm_scale_kernel(const double* __restrict__ partial, int nblocks, float max_norm, float* __restrict__ out)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 64) a += partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(a);
        float coef = 1.f;
        if (max_norm > 0.f) coef = fminf(max_norm / (norm + 1e-6f), 1.f);
        out[0] = coef;
        out[1] = norm;
    }
}

// torch.optim.AdamW (single-tensor form): p *= 1 - lr wd ; m = lerp(m, g, 1 - b1) ; v = b2 v + (1 - b2) g g ;
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                    const float* __restrict__ grad, const float* __restrict__ grad_scale, long n,
                                                    float decay, float beta1, float beta2, float eps, float step_size, float bc2_sqrt)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float sc = grad_scale ? grad_scale[0] : 1.f;
    const float g = grad[i] * sc;
    const float pw = p[i] * decay;
    const float mi = m[i] + (g - m[i]) * (1.f - beta1);
    const float vi = v[i] * beta2 + (1.f - beta2) * g * g;
    m[i] = mi;
    v[i] = vi;
    p[i] = pw - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_head_grad_workspace_bytes(long M, int C, int D)
{
    if (M <= 0 || C <= 0 || D <= 0 || D % HG_TD) return 0;
    const HgPlan p = hg_plan(M, C, D);
    return (long)p.splits * (4l * C * D + 8l * C);
}

extern "C" int dtlr_head_grad(const float* G, const float* X, float* dW, float* db, float* workspace, long M, int C, int D, void* stream)
{
    clear_stale_error();
    if (!G || !X || !dW || !db || !workspace) return DTLR_EINVAL;
    if (M <= 0 || C <= 0 || D <= 0) return DTLR_EINVAL;
    if (D % HG_TD) return DTLR_ESHAPE;
    if (misaligned(X, 15) || misaligned(workspace, 15)) return DTLR_EINVAL;
    const HgPlan p = hg_plan(M, C, D);
    const long nW = (long)C * D;
    float* part = workspace;
    double* partb = reinterpret_cast<double*>(workspace + (long)p.splits * nW);      // 8-byte aligned: D % 64 == 0
    if (int rc = launch<head_grad_partial_kernel>(dim3((unsigned)(p.tiles_c * p.tiles_d), (unsigned)p.splits), dim3(256), 0, (hipStream_t)stream,
                                                  G, X, part, partb, M, C, D, p.tiles_d, p.chunk)) return rc;
    return launch<head_grad_reduce_kernel>(dim3((unsigned)((nW + C + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                           part, partb, dW, db, nW, C, p.splits);
}

extern "C" long dtlr_grad_norm_scale_workspace_bytes(void) { return (long)GN_BLOCKS * 8; }

extern "C" int dtlr_grad_norm_scale(const float* grad, long n, float max_norm, float* scale_out, void* workspace, void* stream)
{
    clear_stale_error();
    if (!grad || !scale_out || !workspace || n <= 0) return DTLR_EINVAL;
    if (misaligned(workspace, 7)) return DTLR_EINVAL;
    long nb = (n + 255) / 256;
    if (nb > GN_BLOCKS) nb = GN_BLOCKS;
    if (int rc = launch<sumsq_partial_kernel>(dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, grad, n, (double*)workspace)) return rc;
    return launch<norm_scale_kernel>(dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, (int)nb, max_norm, scale_out);
}

extern "C" int dtlr_adamw_step(float* param, float* exp_avg, float* exp_avg_sq, const float* grad, const float* grad_scale, long n,
                               float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream)
{
    clear_stale_error();
    if (!param || !exp_avg || !exp_avg_sq || !grad || n <= 0 || step <= 0) return DTLR_EINVAL;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const float decay = (float)(1.0 - (double)lr * (double)weight_decay);
    return launch<adamw_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, exp_avg, exp_avg_sq, grad,
                                grad_scale, n, decay, beta1, beta2, eps, (float)((double)lr / bc1), (float)sqrt(bc2));
}
