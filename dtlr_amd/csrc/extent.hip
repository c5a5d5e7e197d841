// Per-line batching: a padded batch in which every line gets the result it would get alone (engine.forward(per_line=True)).
//   dtlr_line_extents              (h, w) of every line from the padding mask: the reference's valid_H / valid_W
//   dtlr_zero_outside_extent_nhwc  zero a [B, H, W, C] map outside each line's extent at stride 2^s (the input of a 3x3 convolution
//                                  must read zeros past the line's border, as the zero padding of the line alone)
// The extent of a line at stride 2^s is (ceil(h / 2^s), ceil(w / 2^s)): the output size of every stride-2 stage of the ResNet path
// (7x7/s2/p3, 3x3/s2/p1, 1x1/s2) applied s times.  Extents stay on the device: nothing here synchronises with the host.
#include "dtlr_common.h"

namespace dtlr {

// one workgroup per line: unmasked rows of column 0 and unmasked columns of row 0
__global__ __launch_bounds__(256) void line_extents_kernel(const uint8_t* __restrict__ mask, int H, int W, int* __restrict__ ext)
{
    __shared__ int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint8_t* mb = mask + (long)blockIdx.x * H * W;
    int ch = 0, cw = 0;
    for (int i = threadIdx.x; i < H; i += 256) ch += mb[(long)i * W] ? 0 : 1;
    for (int j = threadIdx.x; j < W; j += 256) cw += mb[j] ? 0 : 1;
    ch = wave_sum_i(ch);
    cw = wave_sum_i(cw);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_cnt[0], ch); atomicAdd(&s_cnt[1], cw); }
    __syncthreads();
    if (threadIdx.x == 0) { ext[2 * blockIdx.x] = s_cnt[0]; ext[2 * blockIdx.x + 1] = s_cnt[1]; }
}

// one workgroup per (row, line); nv 16-byte vectors per pixel.  A row below the extent is zeroed whole, a row inside it from column
// ew on; in-extent bytes are never touched, so the work is proportional to the padding (a workgroup with nothing to write exits).
__global__ __launch_bounds__(256) void zero_outside_extent_kernel(uint4* __restrict__ x, const int* __restrict__ ext, int s, int H, int W, int nv)
{
    const int y = blockIdx.x, b = blockIdx.y;
    const int eh = (ext[2 * b] + (1 << s) - 1) >> s, ew = (ext[2 * b + 1] + (1 << s) - 1) >> s;
    const int x0 = y >= eh ? 0 : ew;
    if (x0 >= W) return;
    uint4* row = x + ((long)b * H + y) * (long)W * nv;
    const int n = (W - x0) * nv;
    for (int i = threadIdx.x; i < n; i += 256) row[(long)x0 * nv + i] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_line_extents(const unsigned char* mask, int* ext, int B, int H, int W, void* stream)
{
    clear_stale_error();
    if (!mask || !ext) return DTLR_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0) return DTLR_EINVAL;
    return launch<line_extents_kernel>(dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, mask, H, W, ext);
}

extern "C" int dtlr_zero_outside_extent_nhwc(void* x, const int* ext, int s, int B, int H, int W, int C, int dtype, void* stream)
{
    clear_stale_error();
    if (!x || !ext) return DTLR_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || s < 0 || s > 16) return DTLR_EINVAL;
    int esize;
    if (dtype == DTLR_F32) esize = 4;
    else if (dtype == DTLR_BF16 || dtype == DTLR_F16) esize = 2;      // the zero pattern is the same in both 16-bit formats
    else return DTLR_EDTYPE;
    if (((long)C * esize) % 16 != 0 || (reinterpret_cast<uintptr_t>(x) & 15) != 0) return DTLR_ESHAPE;
    if (B > 65535) return DTLR_ESHAPE;
    const int nv = (int)((long)C * esize / 16);
    return launch<zero_outside_extent_kernel>(dim3((unsigned)H, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                                              (uint4*)x, ext, s, H, W, nv);
}
