// Weight-resident projection GEMM for K = 256 (bf16):   C[M, N] = epi( A[M, 256] . W[N, 256]^T ),  N = 256 or 384.
//
// The encoder's value / [offsets|weights] projections and the decoder's batched value projection (SURVEY.md appendix C:
// T x 256 x 256, T x 256 x 384, T x 256 x 1536 with T = 174,080 tokens) move 512 bytes in and 512..768 bytes out per token
// for 131..197 kflop: they are HBM streams, and the tiled kernel (gemm.hip: 128x128 tiles, 4 K-slabs per tile, an epilogue
// during which its loader waves stall) holds them at 3.3-3.8 TB/s of compulsory bytes.  Here the roles are turned around:
//   * the WEIGHT is the resident operand: wave w of the 8 keeps its N/8 output channels x 256 k as MFMA A-fragments in
//     registers for the whole kernel (64 VGPRs at N = 256, 96 at N = 384), loaded once per workgroup from L2;
//   * TOKENS stream: tiles of 64 tokens (32 KB) are DMA'd global -> LDS (global_load_lds_dwordx4: no VGPR staging, no
//     ds_write pass) through a 4-stage ring, three tiles in flight per CU; every DMA instruction reads 8 rows x 128 bytes
//     (full lines).  The 16-byte chunks of a row are permuted on the SOURCE side (chunk c of row r lands in slot c ^ r of its
//     128-byte LDS row) so that the B-fragment reads of the 16x16x32 MFMA -- 16 tokens x 4 k-chunks per ds_read_b128 group --
//     hit 16 distinct 16-byte slots (cdna_hip_programming.md rule 21: linear destination, permuted source, same permutation
//     on the read);
//   * one barrier per 64 tokens (publishes the tile, frees the stage read two barriers ago); no K loop state, no tile
//     epilogue stall: a wave's accumulators ARE its output slice of the tile (C^T layout: a lane holds 4 consecutive channels
//     of one token), rounded, paired with v_permlane16_swap into 16-byte stores exactly like gemm.hip's epilogue;
//   * persistent: one workgroup per CU walks a contiguous run of token tiles.
// Epilogue options: + bias[N] (fp32); + R[(m % res_rows), :] (bf16, row-broadcast: the encoder's pos . W^T term of an
// unpadded batch, see engine.py); rows with row_mask[m] != 0 written as zeros (value.masked_fill, ms_deform_attn.py:95-96);
// C row stride ldc >= N (column slices of a wider matrix: the six decoder value projections share one [T, 1536] buffer).
// HBM-bound by construction: per CU and 64-token tile 64..80 KB of traffic against 64..96 MFMAs per wave.
#include "gfx950_prims.h"
#include "../../include/dtlr_k256multi.h"

namespace dtlr {

constexpr int K2_TOK = 64;                       // tokens per stage
constexpr int K2_STAGE = K2_TOK * 512;           // 32 KB
constexpr int K2_NS = 4;                         // ring stages
constexpr int K2_LDS = K2_NS * K2_STAGE;         // 128 KB: one workgroup per CU

__device__ __forceinline__ uint2 k2_load8(const void* p) {
    uint2 r;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}
// scalar base + 32-bit lane offset + immediate: one address register per load instead of two, and the per-row-tile column step is free
template <int OFF> __device__ __forceinline__ uint2 k2_load8_so(const void* sbase, unsigned voff) {
    uint2 r;
    asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
    return r;
}
__device__ __forceinline__ unsigned k2_load_u8_so(const void* sbase, unsigned voff) {
    unsigned r;
    asm volatile("global_load_ubyte %0, %1, %2" : "=v"(r) : "v"(voff), "s"(sbase) : "memory");
    return r;
}
__device__ __forceinline__ unsigned k2_load_u8(const void* p) {
    unsigned r;
    asm volatile("global_load_ubyte %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}

// NRT = 16-channel row tiles per wave: N = 128 * NRT (2 -> 256, 3 -> 384).  Wp: the weight in fragment order (dtlr_k256_pack:
// block ((wave * NRT + rt) * 8 + ks) = 64 lanes x 8 elements, lane (m = l & 15, g = l >> 4) <- W[(wave*NRT + rt)*16 + m][32 ks + 8 g ..]).
template <int NRT, bool RES>
__global__ __launch_bounds__(512, 2) void gemm_k256_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Wp, const float* __restrict__ bias,
    const uint16_t* __restrict__ resid, int res_rows, const uint8_t* __restrict__ row_mask,
    uint16_t* __restrict__ C, int ldc, int M, int tiles_per_wg, int n_img)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char k2_smem[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)k2_smem;
    constexpr int N = 128 * NRT;
    constexpr int E = (NRT / 2) * 4 + (NRT & 1) * 4;          // global stores per tile per wave (16-byte pairs + 8-byte odd tile)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = lane & 15, g = lane >> 4;
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    // workgroup b runs on XCD b % 8; logical ids are contiguous inside an XCD
    const int nwg = (int)gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = (int)blockIdx.x & 7;
    const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + ((int)blockIdx.x >> 3);
    const int t_begin = logical * tiles_per_wg;
    const int t_end = min(t_begin + tiles_per_wg, ntiles);
    if (t_begin >= t_end) return;
    const int nt = t_end - t_begin;
    // Tile order.  n_img == 0: tile t = rows [64 t, 64 t + 64).  n_img > 0 (broadcast residual over n_img images of res_rows rows,
    // res_rows % 64 == 0): tile t = position tile t / n_img of image t % n_img -- a workgroup's run of tiles, and the whole band of
    // tiles one XCD owns, reuse a few 64-row residual tiles out of L2 instead of sweeping the whole residual once per image
    // (FETCH_SIZE in row order: 351 MB per launch for 223 MB of operands, the 4 MB residual re-fetched for every image).
    auto row0 = [&](int t) -> long {
        if (RES && n_img > 0) { const int pt = t / n_img; return (long)(t - pt * n_img) * res_rows + (long)pt * K2_TOK; }
        return (long)t * K2_TOK;
    };

    // ---- DMA of token tile t into ring slot: 32 blocks of 8 rows x 128 B; this wave issues blocks j = 4 wave + u ------------
    const int dr = lane >> 3, dc = (lane & 7) ^ dr;           // row within the block; SOURCE chunk that lands in slot (lane & 7)
    auto issue = [&](int t, int slot) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * wave + u, tt8 = j >> 2, kb = j & 3;
            const long tok = min(row0(t) + tt8 * 8 + dr, (long)M - 1);
            glds16(A + tok * 256 + kb * 64 + dc * 8, lds_base + (unsigned)(slot * K2_STAGE + j * 1024));
        }
    };
    // prologue: up to three tiles in flight, then the resident operand
    issue(t_begin, 0);
    if (nt > 1) issue(t_begin + 1, 1);
    if (nt > 2) issue(t_begin + 2, 2);
    uint4 wf[NRT][8];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wf[rt][ks] = load16(Wp + ((long)((wave * NRT + rt) * 8 + ks) * 64 + lane) * 8);
    float4 bv[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
        bv[rt] = bias ? *reinterpret_cast<const float4*>(bias + (wave * NRT + rt) * 16 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);

    // B-fragment read addresses: token tile tt, k-step ks: block (2 tt + (n >> 3), ks >> 1), row n & 7, slot ((ks & 1) * 4 + g) ^ (n & 7)
    const unsigned rd0 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + ((g ^ (n & 7)) * 16));
    const unsigned rd1 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + (((4 + g) ^ (n & 7)) * 16));

    // Row-wise epilogue operands (RES): tile i + 1's residual rows and padding flags are loaded in the epilogue of tile i BEFORE the
    // next DMA group and tile i's stores, waited for at the end of that epilogue with vmcnt(E + 4) -- everything but those E stores and
    // that DMA group -- and folded into the INITIAL value of tile i + 1's accumulators (bias + residual), so they occupy no register
    // across the MFMA phase and are never live in a register the compiler might copy before the data has landed.
    // (First version: loaded at the top of iteration i and waited for in the same iteration with vmcnt(4); the counter is in order,
    // so that wait also drained the PREVIOUS tile's stores, a write acknowledgement from HBM per tile: 73 us against 50 us for the
    // same launch without the residual.)
    // Row order (n_img == 0): residual row of this lane's tokens advanced by 64 per tile (no 64-bit modulo per tile).
    int rrow[4] = {0, 0, 0, 0};
    if constexpr (RES) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) rrow[tt] = (int)(((long)t_begin * K2_TOK + tt * 16 + n) % res_rows);
    }
    const int radv = (RES && res_rows > 0) ? K2_TOK % res_rows : 0;
    uint2 rs[NRT][4];
    unsigned msk[4] = {0, 0, 0, 0};
    auto load_row_operands = [&](int t, uint2 (&r)[NRT][4], unsigned (&m)[4]) {
        if (n_img > 0) {
            const int pt = t / n_img;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) rrow[tt] = pt * K2_TOK + tt * 16 + n;
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const unsigned voff = (unsigned)rrow[tt] * (unsigned)(N * 2) + (unsigned)(wave * NRT * 32 + 8 * g);
            r[0][tt] = k2_load8_so<0>(resid, voff);
            if constexpr (NRT > 1) r[1][tt] = k2_load8_so<32>(resid, voff);
            if constexpr (NRT > 2) r[2][tt] = k2_load8_so<64>(resid, voff);
            rrow[tt] += radv;
            if (rrow[tt] >= res_rows) rrow[tt] -= res_rows;
        }
        if (row_mask) {
            const int r0 = (int)row0(t);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) m[tt] = k2_load_u8_so(row_mask, (unsigned)min(r0 + tt * 16 + n, M - 1));
        }
    };
    if constexpr (RES) load_row_operands(t_begin, rs, msk);
    wait_vm<0>();

    f32x4_t acc[NRT][4];
    unsigned zero_bits = 0;
    auto seed_accumulators = [&]() {                          // RES: acc <- bias + residual row; padding flags -> bits
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            if (row_mask && msk[tt]) zero_bits |= 1u << tt;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
                acc[rt][tt] = f32x4_t{bv[rt].x + h16_lo(rs[rt][tt].x), bv[rt].y + h16_hi(rs[rt][tt].x),
                                         bv[rt].z + h16_lo(rs[rt][tt].y), bv[rt].w + h16_hi(rs[rt][tt].y)};
        }
    };
    if constexpr (RES) seed_accumulators();

    for (int i = 0; i < nt; ++i) {
        const int t = t_begin + i;
        const int slot = i & 3;
        __builtin_amdgcn_s_barrier();                         // tile i published by every wave; stage (i + 3) & 3 no longer read
        const long trow = row0(t);
        if constexpr (!RES) {
            if (row_mask) {
                // (they must be OLDER than the next DMA group: waited with vmcnt(4))
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) msk[tt] = k2_load_u8(row_mask + min(trow + tt * 16 + n, (long)M - 1));
            }
            if (i + 3 < nt) issue(t + 3, (i + 3) & 3);
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc[rt][tt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        const unsigned char* sb = k2_smem + slot * K2_STAGE;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            uint4 bf[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
                bf[tt] = *reinterpret_cast<const uint4*>(sb + ((ks & 1) ? rd1 : rd0) + tt * 8192 + (ks >> 1) * 1024);
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc[rt][tt] = mma16(wf[rt][ks], bf[tt], acc[rt][tt]);
        }
        // ---- epilogue: bias, broadcast residual, padding rows, bf16, paired 16-byte stores ---------------------------------
        if constexpr (RES) {
            __builtin_amdgcn_sched_barrier(0);
            if (i + 1 < nt) load_row_operands(t + 1, rs, msk);
            if (i + 3 < nt) issue(t + 3, (i + 3) & 3);
        } else {
            zero_bits = 0;
            if (row_mask) {
                if (i + 3 < nt) wait_vm<4>(); else wait_vm<0>();
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) if (msk[tt]) zero_bits |= 1u << tt;
            }
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const long tok = trow + tt * 16 + n;
            const bool live = tok < M;
            const bool zero = (zero_bits >> tt) & 1u;
            uint32_t pk_lo = 0, pk_hi = 0;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                float v[4] = {acc[rt][tt][0], acc[rt][tt][1], acc[rt][tt][2], acc[rt][tt][3]};
                if constexpr (!RES) { v[0] += bv[rt].x; v[1] += bv[rt].y; v[2] += bv[rt].z; v[3] += bv[rt].w; }
                if (zero) { v[0] = v[1] = v[2] = v[3] = 0.f; }
                const uint32_t lo = pack_bf16x2(v[0], v[1]), hi = pack_bf16x2(v[2], v[3]);
                if ((rt & 1) == 0 && rt + 1 < NRT) { pk_lo = lo; pk_hi = hi; }
                else if (rt & 1) {
                    // pair the row tiles (rt - 1, rt): exchange halves between lane rows g and g ^ 1 -> a lane owns 8 consecutive channels
                    const auto s0 = __builtin_amdgcn_permlane16_swap(pk_lo, lo, false, false);
                    const auto s1 = __builtin_amdgcn_permlane16_swap(pk_hi, hi, false, false);
                    uint16_t* dst = C + tok * (long)ldc + (wave * NRT + rt - 1 + (g & 1)) * 16 + 8 * (g >> 1);
                    if (live) *reinterpret_cast<uint4*>(dst) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                } else {                                      // odd NRT: the last row tile alone, 8-byte stores
                    uint16_t* dst = C + tok * (long)ldc + (wave * NRT + rt) * 16 + 4 * g;
                    if (live) *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
                }
            }
        }
        if constexpr (RES) {
            // in flight after this wait: this tile's E stores and the DMA group issued just before them (none in the last three
            // iterations).  Older, hence landed: the next tile's row operands and DMA groups i + 1, i + 2.  A ragged tile (fewer
            // stores than E) is always a workgroup's last, where nothing is waited for.
            zero_bits = 0;
            if (i + 3 < nt) wait_vm<E + 4>();
            else if (i + 1 < nt) wait_vm<E>();
            if (i + 1 < nt) seed_accumulators();
        } else {
            // tile i + 1 must have landed (mine) before the next barrier: everything but the two newest DMA groups and the
            // stores issued around them may stay in flight
            if (i + 3 < nt) wait_vm<2 * E + 8 <= 16 ? 16 : 24>();
            else wait_vm<0>();
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------
// An encoder layer's value and [offsets | logits] projections of an unpadded batch in ONE pass over src:
//     V[m, 0:256] = A[m, :] Wv^T + bv          O[m, 0:384] = A[m, :] Wo^T + R[m % res_rows, :]          (A = src; R = pos Wo^T + bo)
// Run as two launches (gemm_k256_kernel<2, false>, then gemm_kres.hip's 384-channel column) they read the same 512 bytes per token twice.
// Here one workgroup computes all 640 channels of a token tile, so the tile comes from HBM once by construction: wave w keeps FIVE row
// tiles resident (160 VGPRs: 32 channels of Wv, 48 of Wo, both images as dtlr_k256_pack_weights lays them out), and a 64-token tile is
// walked in four 16-token groups -- 20 accumulator registers instead of 80 -- each finished and stored before the next one starts, every
// B-fragment read from LDS feeding all five row tiles.
//   * LDS: a THREE-stage token ring (two tiles in flight; reads are 2/7 of this kernel's traffic) and ONE 64-row residual tile (48 KB,
//     rows DMA'd like a token tile's: chunk c of row r in slot c ^ (r & 7) of its 128-byte block).  Tiles are walked position-major
//     (tile t = position tile t / n_img of image t % n_img), so the residual tile changes once per n_img tiles: the wave that sees the
//     change DMAs the new tile right after the barrier that retires the old one, and waits for it (own pieces, then a second barrier)
//     between the first group's MFMAs and its epilogue.  No residual load ever sits in a VGPR across a tile.
//   * vmcnt is counted by hand as above: E = 12 stores per wave and tile, 4 DMA instructions per token tile, and a tile's stores are
//     never waited for except where the residual tile changes.
// Both outputs are BIT-identical to the two launches: zero accumulator, k-steps 0..7 on the same MFMA, then V: + bias, round (the !RES
// path above); O: + 0.0f (gemm_kres_kernel's absent bias), + residual, round (its "epilogue: + bias + residual").  M % 64 == 0.
constexpr int VO_NS = 3;
constexpr int VO_RES_OFF = VO_NS * K2_STAGE;                // the residual tile: [8 row groups][6 blocks][8 rows x 128 B]
constexpr int VO_LDS = VO_RES_OFF + K2_TOK * 768;           // 144 KB
constexpr int VO_E = 12;                                    // stores per wave and tile: 4 groups x (V: one 16-byte; O: one 16-byte + one 8-byte)

__global__ __launch_bounds__(512, 2) void gemm_k256_vow_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Wv, const float* __restrict__ bias_v, const uint16_t* __restrict__ Wo,
    const uint16_t* __restrict__ resid, int res_rows, uint16_t* __restrict__ V, int ldv, uint16_t* __restrict__ O, int M, int tiles_per_wg,
    int n_img)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char k2_smem[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)k2_smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = lane & 15, g = lane >> 4;
    const int ntiles = M / K2_TOK;
    // workgroup b runs on XCD b % 8; logical ids are contiguous inside an XCD
    const int nwg = (int)gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = (int)blockIdx.x & 7;
    const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + ((int)blockIdx.x >> 3);
    const int t_begin = logical * tiles_per_wg;
    const int t_end = min(t_begin + tiles_per_wg, ntiles);
    if (t_begin >= t_end) return;
    const int nt = t_end - t_begin;
    auto row0 = [&](int t, int pt) -> long { return (long)(t - pt * n_img) * res_rows + (long)pt * K2_TOK; };

    const int dr = lane >> 3, dc = (lane & 7) ^ dr;           // row within a DMA block; SOURCE chunk that lands in slot (lane & 7)
    auto issue = [&](int t, int slot) {                       // token tile: this wave's blocks j = 4 wave + u (as in gemm_k256_kernel)
        const long r0 = row0(t, t / n_img);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * wave + u, tt8 = j >> 2, kb = j & 3;
            glds16(A + (r0 + tt8 * 8 + dr) * 256 + kb * 64 + dc * 8, lds_base + (unsigned)(slot * K2_STAGE + j * 1024));
        }
    };
    auto issue_res = [&](int pt) {                            // residual tile: this wave's row group (rows 8 wave ..), 6 blocks
        const uint16_t* src = resid + ((long)pt * K2_TOK + wave * 8 + dr) * 384 + dc * 8;
#pragma unroll
        for (int nb = 0; nb < 6; ++nb) glds16(src + nb * 64, lds_base + (unsigned)(VO_RES_OFF + (wave * 6 + nb) * 1024));
    };
    int pt_cur = t_begin / n_img;
    issue_res(pt_cur);
    issue(t_begin, 0);
    if (nt > 1) issue(t_begin + 1, 1);
    uint4 wv[2][8], wo[3][8];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wv[rt][ks] = load16(Wv + ((long)((wave * 2 + rt) * 8 + ks) * 64 + lane) * 8);
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wo[rt][ks] = load16(Wo + ((long)((wave * 3 + rt) * 8 + ks) * 64 + lane) * 8);
    float4 bv[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
        bv[rt] = bias_v ? *reinterpret_cast<const float4*>(bias_v + (wave * 2 + rt) * 16 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    float zero = 0.f;                                         // gemm_kres_kernel's "+ bias" without a bias: kept as an addition
    wait_vm<0>();
    // the compiler's own wait for the bias loads belongs HERE, not at their first use inside the ring loop
    asm volatile("" : "+v"(bv[0].x), "+v"(bv[0].y), "+v"(bv[0].z), "+v"(bv[0].w), "+v"(bv[1].x), "+v"(bv[1].y), "+v"(bv[1].z), "+v"(bv[1].w), "+v"(zero));

    const unsigned rd0 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + ((g ^ (n & 7)) * 16));
    const unsigned rd1 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + (((4 + g) ^ (n & 7)) * 16));
    // residual of row tile rt, token n of group tt: bytes o = 96 wave + 32 rt + 8 g .. + 7 of row 16 tt + n -> row group 2 tt + (n >> 3),
    // block o >> 7, chunk (o >> 4) & 7, half o & 8
    unsigned rres[3];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt) {
        const int o = 96 * wave + 32 * rt + 8 * g;
        rres[rt] = (unsigned)(VO_RES_OFF + ((n >> 3) * 6 + (o >> 7)) * 1024 + (n & 7) * 128 + ((((o >> 4) & 7) ^ (n & 7)) * 16) + (o & 8));
    }

    int slot = 0;
    for (int i = 0; i < nt; ++i) {
        const int t = t_begin + i;
        __builtin_amdgcn_s_barrier();                         // tile i published; stage (i + 2) % 3 and (on a change) the residual tile no longer read
        const int pt = t / n_img;
        const bool new_res = pt != pt_cur;
        pt_cur = pt;
        const bool more = i + 2 < nt;
        if (new_res) issue_res(pt);
        if (more) issue(t + 2, slot == 0 ? 2 : slot - 1);
        const long trow = row0(t, pt);
        const unsigned char* sb = k2_smem + slot * K2_STAGE;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            f32x4_t av[2], ao[3];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) av[rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rt = 0; rt < 3; ++rt) ao[rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const uint4 bf = *reinterpret_cast<const uint4*>(sb + ((ks & 1) ? rd1 : rd0) + tt * 8192 + (ks >> 1) * 1024);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) av[rt] = mma16(wv[rt][ks], bf, av[rt]);
#pragma unroll
                for (int rt = 0; rt < 3; ++rt) ao[rt] = mma16(wo[rt][ks], bf, ao[rt]);
            }
            if (tt == 0 && new_res) {
                // my pieces of the new residual tile (older than the token DMA group issued after them), then everybody's
                if (more) wait_vm<4>(); else wait_vm<0>();
                __builtin_amdgcn_s_barrier();
            }
            const long tok = trow + tt * 16 + n;
            // ---- V: + bias, round, row tiles (0, 1) paired into a 16-byte store (gemm_k256_kernel's !RES epilogue) --------------------
            {
                const uint32_t lo0 = pack_bf16x2(av[0][0] + bv[0].x, av[0][1] + bv[0].y), hi0 = pack_bf16x2(av[0][2] + bv[0].z, av[0][3] + bv[0].w);
                const uint32_t lo1 = pack_bf16x2(av[1][0] + bv[1].x, av[1][1] + bv[1].y), hi1 = pack_bf16x2(av[1][2] + bv[1].z, av[1][3] + bv[1].w);
                const auto s0 = __builtin_amdgcn_permlane16_swap(lo0, lo1, false, false);
                const auto s1 = __builtin_amdgcn_permlane16_swap(hi0, hi1, false, false);
                *reinterpret_cast<uint4*>(V + tok * (long)ldv + (wave * 2 + (g & 1)) * 16 + 8 * (g >> 1)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
            }
            // ---- O: + 0, + residual (one 8-byte LDS read per row tile), round; row tiles (0, 1) paired, row tile 2 an 8-byte store ----------
            uint32_t lo[3], hi[3];
#pragma unroll
            for (int rt = 0; rt < 3; ++rt) {
                const uint2 rr = *reinterpret_cast<const uint2*>(k2_smem + rres[rt] + tt * 12288);
                float v[4] = {ao[rt][0] + zero, ao[rt][1] + zero, ao[rt][2] + zero, ao[rt][3] + zero};
                v[0] += h16_lo(rr.x); v[1] += h16_hi(rr.x); v[2] += h16_lo(rr.y); v[3] += h16_hi(rr.y);
                lo[rt] = pack_bf16x2(v[0], v[1]);
                hi[rt] = pack_bf16x2(v[2], v[3]);
            }
            {
                const auto s0 = __builtin_amdgcn_permlane16_swap(lo[0], lo[1], false, false);
                const auto s1 = __builtin_amdgcn_permlane16_swap(hi[0], hi[1], false, false);
                uint16_t* dst = O + tok * 384;
                *reinterpret_cast<uint4*>(dst + (wave * 3 + (g & 1)) * 16 + 8 * (g >> 1)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                *reinterpret_cast<uint2*>(dst + (wave * 3 + 2) * 16 + 4 * g) = make_uint2(lo[2], hi[2]);
            }
        }
        // my pieces of tile i + 1 must have landed before the next barrier.  Issued after them: tile i - 1's stores, this iteration's DMA
        // group (if any; a residual tile's pieces were waited for above), this tile's stores.
        if (more) wait_vm<2 * VO_E + 4>();
        else if (i + 1 < nt) wait_vm<2 * VO_E>();
        slot = slot == 2 ? 0 : slot + 1;
    }
}


// ---------------------------------------------------------------------------------------------------------------------------
// All decoder layers' value projections of `memory` in ONE launch:   C[m, 0:N] = A[m, :] W^T + bias,   N = 256 L (L = decoder layers).
// As launches of gemm_k256_kernel<3, false> over 384-channel slices, `memory` is read once per slice and every wave writes 96-byte
// pieces of the rows.  Here the N channels are cut into COLUMN GROUPS of NRT x 128 channels (NRT <= 5: the 160 resident VGPRs of
// gemm_k256_vow_kernel), blockIdx.y = group, and the tile loop is gemm_k256_vow_kernel's: a three-stage token ring, a 64-token tile
// walked in four 16-token groups, each finished and stored before the next starts.
//   * groups: units of 128 channels spread as evenly as they go over ceil(N / 640) groups (k256_multi_plan): L = 6 gives 3 x 512, so
//     the three workgroups of a token tile do the same work, and a wave owns 64 channels = ONE 128-byte line of every token, written by
//     two back-to-back 16-byte-per-lane stores.  Uneven splits (L = 7: 640 + 640 + 512) run the NRT - 1 body in their last groups.
//   * placement: gridDim.x is a multiple of 8 and gridDim.x * gridDim.y <= CUs, so the workgroups (x, 0 .. groups - 1) are all resident,
//     sit on XCD x % 8 and walk the same run of token tiles at the same pace: the tile comes from HBM once and from that XCD's L2 after.
//   * bit-identical to the slice launches: zero accumulator, k-steps 0..7 on the same MFMA with the weight as the A operand, + bias,
//     one rounding; rows with row_mask[m] != 0 written as zeros.
// vmcnt by hand: E stores per wave and tile, 4 DMA instructions per token tile.  A ragged tile (fewer stores) is a workgroup's last.
constexpr int KM_NS = 3;
constexpr int KM_LDS = KM_NS * K2_STAGE;                    // 96 KB
constexpr int KM_MAX_NRT = DTLR_K256_MULTI_MAX_UNITS;

template <int NRT, bool MASK>
__device__ __forceinline__ void k256_multi_body(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Wp, const float* __restrict__ bias, const uint8_t* __restrict__ row_mask,
    uint16_t* __restrict__ C, int ldc, int M, int tiles_per_wg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char k2_smem[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)k2_smem;
    constexpr int E = 4 * (NRT / 2 + (NRT & 1));             // stores per wave and tile
    static_assert(2 * E + 4 < 64, "vmcnt is a 6-bit counter");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = lane & 15, g = lane >> 4;
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    // workgroup (x, y) runs on XCD x % 8 (gridDim.x % 8 == 0); logical ids are contiguous inside an XCD
    const int q8 = (int)gridDim.x >> 3, xcd = (int)blockIdx.x & 7;
    const int logical = xcd * q8 + ((int)blockIdx.x >> 3);
    const int t_begin = logical * tiles_per_wg;
    const int t_end = min(t_begin + tiles_per_wg, ntiles);
    if (t_begin >= t_end) return;
    const int nt = t_end - t_begin;

    const int dr = lane >> 3, dc = (lane & 7) ^ dr;           // row within a DMA block; SOURCE chunk that lands in slot (lane & 7)
    auto issue = [&](int t, int slot) {                       // token tile: this wave's blocks j = 4 wave + u (as in gemm_k256_kernel)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * wave + u, tt8 = j >> 2, kb = j & 3;
            const long tok = min((long)t * K2_TOK + tt8 * 8 + dr, (long)M - 1);
            glds16(A + tok * 256 + kb * 64 + dc * 8, lds_base + (unsigned)(slot * K2_STAGE + j * 1024));
        }
    };
    issue(t_begin, 0);
    if (nt > 1) issue(t_begin + 1, 1);
    uint4 wf[NRT][8];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wf[rt][ks] = load16(Wp + ((long)((wave * NRT + rt) * 8 + ks) * 64 + lane) * 8);
    float4 bv[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
        bv[rt] = bias ? *reinterpret_cast<const float4*>(bias + (wave * NRT + rt) * 16 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    wait_vm<0>();
    // the compiler's own wait for the bias loads belongs HERE, not at their first use inside the ring loop
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) asm volatile("" : "+v"(bv[rt].x), "+v"(bv[rt].y), "+v"(bv[rt].z), "+v"(bv[rt].w));

    const unsigned rd0 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + ((g ^ (n & 7)) * 16));
    const unsigned rd1 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + (((4 + g) ^ (n & 7)) * 16));

    int slot = 0;
    for (int i = 0; i < nt; ++i) {
        const int t = t_begin + i;
        __builtin_amdgcn_s_barrier();                         // tile i published; stage (i + 2) % 3 no longer read
        const bool more = i + 2 < nt;
        const long trow = (long)t * K2_TOK;
        unsigned msk[4] = {0, 0, 0, 0};
        if constexpr (MASK) {                                 // older than the DMA group below: waited for with vmcnt(4)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) msk[tt] = k2_load_u8(row_mask + min(trow + tt * 16 + n, (long)M - 1));
        }
        if (more) issue(t + 2, slot == 0 ? 2 : slot - 1);
        const unsigned char* sb = k2_smem + slot * K2_STAGE;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            f32x4_t acc[NRT];
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) acc[rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const uint4 bf = *reinterpret_cast<const uint4*>(sb + ((ks & 1) ? rd1 : rd0) + tt * 8192 + (ks >> 1) * 1024);
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt) acc[rt] = mma16(wf[rt][ks], bf, acc[rt]);
            }
            if constexpr (MASK) {
                if (tt == 0) {
                    if (more) wait_vm<4>(); else wait_vm<0>();
                    asm volatile("" : "+v"(msk[0]), "+v"(msk[1]), "+v"(msk[2]), "+v"(msk[3]));      // read only after the wait
                }
            }
            const long tok = trow + tt * 16 + n;
            const bool live = tok < M;
            const bool zero = MASK && msk[tt] != 0;
            // ---- + bias, padding rows, round, paired 16-byte stores (gemm_k256_kernel's !RES epilogue) ------------------------------
            uint32_t pk_lo = 0, pk_hi = 0;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                float v[4] = {acc[rt][0] + bv[rt].x, acc[rt][1] + bv[rt].y, acc[rt][2] + bv[rt].z, acc[rt][3] + bv[rt].w};
                if (zero) { v[0] = v[1] = v[2] = v[3] = 0.f; }
                const uint32_t lo = pack_bf16x2(v[0], v[1]), hi = pack_bf16x2(v[2], v[3]);
                if ((rt & 1) == 0 && rt + 1 < NRT) { pk_lo = lo; pk_hi = hi; }
                else if (rt & 1) {
                    // pair the row tiles (rt - 1, rt): exchange halves between lane rows g and g ^ 1 -> a lane owns 8 consecutive channels
                    const auto s0 = __builtin_amdgcn_permlane16_swap(pk_lo, lo, false, false);
                    const auto s1 = __builtin_amdgcn_permlane16_swap(pk_hi, hi, false, false);
                    uint16_t* dst = C + tok * (long)ldc + (wave * NRT + rt - 1 + (g & 1)) * 16 + 8 * (g >> 1);
                    if (live) *reinterpret_cast<uint4*>(dst) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                } else {                                      // odd NRT: the last row tile alone, 8-byte stores
                    uint16_t* dst = C + tok * (long)ldc + (wave * NRT + rt) * 16 + 4 * g;
                    if (live) *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
                }
            }
        }
        // my pieces of tile i + 1 must have landed before the next barrier.  Issued after them: tile i - 1's stores, this iteration's
        // DMA group (if any), this tile's stores (and, MASK, this tile's flags: waited for above, with everything older).
        if (more) wait_vm<2 * E + 4>();
        else if (i + 1 < nt) wait_vm<2 * E>();
        slot = slot == 2 ? 0 : slot + 1;
    }
}

// blockIdx.y = column group: the first n_hi groups hold NRT_HI units of 128 channels, the others NRT_HI - 1; the images and the columns
// of the groups follow each other in that order (dtlr_k256_multi_pack_weights).
template <int NRT_HI, bool MASK>
__global__ __launch_bounds__(512, 2) void gemm_k256_multi_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Wp, const float* __restrict__ bias, const uint8_t* __restrict__ row_mask,
    uint16_t* __restrict__ C, int ldc, int M, int tiles_per_wg, int n_hi)
{
    const int gi = (int)blockIdx.y;
    const int col0 = 128 * (gi < n_hi ? gi * NRT_HI : n_hi * NRT_HI + (gi - n_hi) * (NRT_HI - 1));
    Wp += (long)col0 * 256;
    C += col0;
    if (bias) bias += col0;
    if constexpr (NRT_HI == KM_MAX_NRT) {                     // the only width an even number of units splits unevenly at
        if (gi >= n_hi) { k256_multi_body<NRT_HI - 1, MASK>(A, Wp, bias, row_mask, C, ldc, M, tiles_per_wg); return; }
    }
    k256_multi_body<NRT_HI, MASK>(A, Wp, bias, row_mask, C, ldc, M, tiles_per_wg);
}


// ---------------------------------------------------------------------------------------------------------------------------
// The weight-resident body with TWO token streams:   C[M, 384] = (A + A2)[M, 256] . W^T + bias      ([offsets | logits] of tgt + query_pos
// in the decoder, of src + pos in a padded encoder batch; deformable_transformer.py:797-812, ms_deform_attn.py:97-98).
// The tiled GEMM's A + A2 prologue (gemm.hip: GT<uint16_t>::add) forms every operand element as round16(float(a) + float(a2)); so does
// this kernel, ONCE per element: the A and A2 tiles of 64 tokens are DMA'd side by side (64 KB per stage, two stages, proj_ln_k256's
// ring), and each wave, as soon as ITS OWN DMA pieces of a tile have landed (vmcnt), adds its 4 KB of A2 into its 4 KB of A in place --
// before the barrier that publishes the tile, so the sum costs no barrier of its own and 1/8 of the tile's additions per wave.  The MFMA
// phase then reads the summed tile exactly as gemm_k256_kernel<3, false> reads A: same fragments, k-steps 0..7 from a zero accumulator,
// + bias, one rounding -- bit-identical to the tiled kernel with the prologue.  A2 == nullptr: no second stream, no addition.
constexpr int KA_STAGE = 2 * K2_STAGE;                      // A tile | A2 tile
constexpr int KA_LDS = 2 * KA_STAGE;                        // 128 KB
constexpr int KA_E = 8;                                     // stores per wave and tile: 4 groups x (one 16-byte + one 8-byte)

__device__ __forceinline__ uint4 k2_add16(uint4 a, uint4 b) {            // gemm.hip's GT<uint16_t>::add
    const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pack_bf16x2(h16_lo(x[i]) + h16_lo(y[i]), h16_hi(x[i]) + h16_hi(y[i]));
    return make_uint4(o[0], o[1], o[2], o[3]);
}

template <bool MASK>
__global__ __launch_bounds__(512, 2) void gemm_k256_a2_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ A2, const uint16_t* __restrict__ Wp, const float* __restrict__ bias,
    const uint8_t* __restrict__ row_mask, uint16_t* __restrict__ C, int M, int tiles_per_wg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char k2_smem[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)k2_smem;
    constexpr int NRT = 3;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = lane & 15, g = lane >> 4;
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    const int t_begin = (int)blockIdx.x * tiles_per_wg;
    const int t_end = min(t_begin + tiles_per_wg, ntiles);
    if (t_begin >= t_end) return;
    const int nt = t_end - t_begin;
    const bool two = A2 != nullptr;                           // wave-uniform: the DMA count per tile is 8 or 4
    const int dr = lane >> 3, dc = (lane & 7) ^ dr;
    auto issue = [&](int t, int slot) {                       // this wave's 4 blocks of the A tile, then of the A2 tile
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * wave + u, tt8 = j >> 2, kb = j & 3;
            const long tok = min((long)t * K2_TOK + tt8 * 8 + dr, (long)M - 1);
            glds16(A + tok * 256 + kb * 64 + dc * 8, lds_base + (unsigned)(slot * KA_STAGE + j * 1024));
        }
        if (two) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = 4 * wave + u, tt8 = j >> 2, kb = j & 3;
                const long tok = min((long)t * K2_TOK + tt8 * 8 + dr, (long)M - 1);
                glds16(A2 + tok * 256 + kb * 64 + dc * 8, lds_base + (unsigned)(slot * KA_STAGE + K2_STAGE + j * 1024));
            }
        }
    };
    // A <- round16(A + A2) on the 4 KB this wave DMA'd itself (landed: the caller waited on vmcnt); done before the publishing barrier
    auto sum_own = [&](int slot) {
        if (!two) return;
        unsigned char* p = k2_smem + slot * KA_STAGE + wave * 4096 + lane * 16;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 a = *reinterpret_cast<const uint4*>(p + u * 1024), b = *reinterpret_cast<const uint4*>(p + K2_STAGE + u * 1024);
            *reinterpret_cast<uint4*>(p + u * 1024) = k2_add16(a, b);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // my LDS writes are done before I arrive at the barrier
    };
    issue(t_begin, 0);
    uint4 wf[NRT][8];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wf[rt][ks] = load16(Wp + ((long)((wave * NRT + rt) * 8 + ks) * 64 + lane) * 8);
    float4 bv[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
        bv[rt] = bias ? *reinterpret_cast<const float4*>(bias + (wave * NRT + rt) * 16 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    wait_vm<0>();
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) asm volatile("" : "+v"(bv[rt].x), "+v"(bv[rt].y), "+v"(bv[rt].z), "+v"(bv[rt].w));
    sum_own(0);

    const unsigned rd0 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + ((g ^ (n & 7)) * 16));
    const unsigned rd1 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + (((4 + g) ^ (n & 7)) * 16));

    for (int i = 0; i < nt; ++i) {
        const int t = t_begin + i;
        const int slot = i & 1;
        __builtin_amdgcn_s_barrier();                         // tile i summed and published; stage (i + 1) & 1 no longer read
        const bool more = i + 1 < nt;
        const long trow = (long)t * K2_TOK;
        unsigned msk[4] = {0, 0, 0, 0};
        if constexpr (MASK) {                                 // older than the DMA group below
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) msk[tt] = k2_load_u8(row_mask + min(trow + tt * 16 + n, (long)M - 1));
        }
        if (more) issue(t + 1, slot ^ 1);
        const unsigned char* sb = k2_smem + slot * KA_STAGE;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            f32x4_t acc[NRT];
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) acc[rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const uint4 bf = *reinterpret_cast<const uint4*>(sb + ((ks & 1) ? rd1 : rd0) + tt * 8192 + (ks >> 1) * 1024);
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt) acc[rt] = mma16(wf[rt][ks], bf, acc[rt]);
            }
            if constexpr (MASK) {
                if (tt == 0) {                                // the flags, and nothing newer than the DMA group issued after them
                    if (!more) wait_vm<0>(); else if (two) wait_vm<8>(); else wait_vm<4>();
                    asm volatile("" : "+v"(msk[0]), "+v"(msk[1]), "+v"(msk[2]), "+v"(msk[3]));
                }
            }
            const long tok = trow + tt * 16 + n;
            const bool live = tok < M;
            const bool zero = MASK && msk[tt] != 0;
            uint32_t lo[NRT], hi[NRT];
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                float v[4] = {acc[rt][0] + bv[rt].x, acc[rt][1] + bv[rt].y, acc[rt][2] + bv[rt].z, acc[rt][3] + bv[rt].w};
                if (zero) { v[0] = v[1] = v[2] = v[3] = 0.f; }
                lo[rt] = pack_bf16x2(v[0], v[1]);
                hi[rt] = pack_bf16x2(v[2], v[3]);
            }
            const auto s0 = __builtin_amdgcn_permlane16_swap(lo[0], lo[1], false, false);
            const auto s1 = __builtin_amdgcn_permlane16_swap(hi[0], hi[1], false, false);
            uint16_t* dst = C + tok * 384;
            if (live) {
                *reinterpret_cast<uint4*>(dst + (wave * 3 + (g & 1)) * 16 + 8 * (g >> 1)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                *reinterpret_cast<uint2*>(dst + (wave * 3 + 2) * 16 + 4 * g) = make_uint2(lo[2], hi[2]);
            }
        }
        // my pieces of tile i + 1 (older than this tile's KA_E stores) must have landed: I add them up, then arrive at the barrier
        if (more) { wait_vm<KA_E>(); sum_own(slot ^ 1); }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------
// Output projection + residual + LayerNorm in the same weight-resident form:   Y = LayerNorm(R + A W^T + b),  all [M, 256] bf16.
// (`src = norm1(src + self_attn(...))`, the last op of self_attn being output_proj: models/dino/deformable_transformer.py:810-815,
// ops/modules/ms_deform_attn.py:124.)  ffn.hip's proj_ln_bf16_kernel keeps the TOKENS in registers and re-streams the 128 KB weight
// from L2 for every 64 tokens (348 MB of L2 -> LDS traffic per encoder call on top of 267 MB of HBM traffic); here the weight stays in
// registers and the A and R tiles of 64 tokens are DMA'd through a 2-stage LDS ring (64 KB per stage).  W's rows are assigned to MFMA
// rows so that a lane's two accumulator tiles are 8 CONSECUTIVE channels (row tile e of wave w, MFMA row m <-> channel
// 32 w + 8 (m >> 2) + 4 e + (m & 3)): the residual is one 16-byte LDS read and the result one 16-byte store per token, no lane
// exchange.  LayerNorm statistics are two-pass fp32 like ATen's; the 8 waves of a token exchange partial sums through LDS
// (three barriers per 64 tokens including the one that publishes the tile).
constexpr int PK_STAGE = 2 * K2_STAGE;                      // A tile | R tile
constexpr int PK_LN_OFF = 2 * PK_STAGE;                     // two stages, then [2][64 tokens][8 waves] floats
constexpr int PK_LDS = PK_LN_OFF + 2 * 64 * 8 * 4;

__global__ __launch_bounds__(512, 2) void proj_ln_k256_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Wp, const float* __restrict__ bias, const uint16_t* __restrict__ R,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, uint16_t* __restrict__ Y, int M, int tiles_per_wg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char k2_smem[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)k2_smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n = lane & 15, g = lane >> 4;
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    const int t_begin = (int)blockIdx.x * tiles_per_wg;
    const int t_end = min(t_begin + tiles_per_wg, ntiles);
    if (t_begin >= t_end) return;
    const int nt = t_end - t_begin;
    const int dr = lane >> 3, dc = (lane & 7) ^ dr;
    auto issue = [&](int t, int slot) {                      // 8 DMA instructions per wave: its 4 blocks of the A tile and of the R tile
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = 4 * wave + u, tt8 = j >> 2, kb = j & 3;
            const long tok = min((long)t * K2_TOK + tt8 * 8 + dr, (long)M - 1);
            glds16(A + tok * 256 + kb * 64 + dc * 8, lds_base + (unsigned)(slot * PK_STAGE + j * 1024));
            glds16(R + tok * 256 + kb * 64 + dc * 8, lds_base + (unsigned)(slot * PK_STAGE + K2_STAGE + j * 1024));
        }
    };
    issue(t_begin, 0);
    uint4 wf[2][8];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wf[e][ks] = load16(Wp + ((long)((wave * 2 + e) * 8 + ks) * 64 + lane) * 8);
    const int ch = 32 * wave + 8 * g;                         // this lane's 8 consecutive channels
    float bs[8], gm[8], bt[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { bs[e] = bias[ch + e]; gm[e] = gamma[ch + e]; bt[e] = beta[ch + e]; }
    wait_vm<0>();
    const unsigned rd0 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + ((g ^ (n & 7)) * 16));
    const unsigned rd1 = (unsigned)((n >> 3) * 4096 + (n & 7) * 128 + (((4 + g) ^ (n & 7)) * 16));
    // residual chunk of this lane: 16-byte chunk 4 wave + g of the row -> block kb = wave >> 1, chunk c = 4 (wave & 1) + g
    const unsigned rres = (unsigned)(K2_STAGE + (n >> 3) * 4096 + (wave >> 1) * 1024 + (n & 7) * 128 + (((4 * (wave & 1) + g) ^ (n & 7)) * 16));
    float* lnsum = reinterpret_cast<float*>(k2_smem + PK_LN_OFF);
    float* lnsq = lnsum + 64 * 8;

    for (int i = 0; i < nt; ++i) {
        const int t = t_begin + i;
        const int slot = i & 1;
        __builtin_amdgcn_s_barrier();                         // tile i published; stage (i + 1) & 1 and the LN buffers are free
        if (i + 1 < nt) issue(t + 1, slot ^ 1);
        f32x4_t acc[2][4];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc[e][tt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const unsigned char* sb = k2_smem + slot * PK_STAGE;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            uint4 bf[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
                bf[tt] = *reinterpret_cast<const uint4*>(sb + ((ks & 1) ? rd1 : rd0) + tt * 8192 + (ks >> 1) * 1024);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc[e][tt] = mma16(wf[e][ks], bf[tt], acc[e][tt]);
        }
        // v = acc + bias + residual ; first pass: row sums
        float v[4][8], sm[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const uint4 rr = *reinterpret_cast<const uint4*>(sb + rres + tt * 8192);
            const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
            sm[tt] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float r = (e & 1) ? h16_hi(rw[e >> 1]) : h16_lo(rw[e >> 1]);
                v[tt][e] = acc[e >> 2][tt][e & 3] + bs[e] + r;
                sm[tt] += v[tt][e];
            }
            sm[tt] += __shfl_xor(sm[tt], 16, 64);
            sm[tt] += __shfl_xor(sm[tt], 32, 64);
            if (g == 0) lnsum[(tt * 16 + n) * 8 + wave] = sm[tt];
        }
        __syncthreads();
        float mean[4], q[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const float4 a = *reinterpret_cast<const float4*>(lnsum + (tt * 16 + n) * 8), c = *reinterpret_cast<const float4*>(lnsum + (tt * 16 + n) * 8 + 4);
            mean[tt] = ((a.x + a.y) + (a.z + a.w) + (c.x + c.y) + (c.z + c.w)) * (1.0f / 256.0f);
            q[tt] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[tt][e] - mean[tt]; q[tt] += d * d; }
            q[tt] += __shfl_xor(q[tt], 16, 64);
            q[tt] += __shfl_xor(q[tt], 32, 64);
            if (g == 0) lnsq[(tt * 16 + n) * 8 + wave] = q[tt];
        }
        __syncthreads();
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const float4 a = *reinterpret_cast<const float4*>(lnsq + (tt * 16 + n) * 8), c = *reinterpret_cast<const float4*>(lnsq + (tt * 16 + n) * 8 + 4);
            const float rstd = rsqrtf(((a.x + a.y) + (a.z + a.w) + (c.x + c.y) + (c.z + c.w)) * (1.0f / 256.0f) + eps);
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[tt][e] - mean[tt]) * rstd * gm[e] + bt[e];
            const long tok = (long)t * K2_TOK + tt * 16 + n;
            if (tok < M)
                *reinterpret_cast<uint4*>(Y + tok * 256 + ch) =
                    make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
        }
        // my pieces of tile i + 1 must have landed before the next barrier; this tile's 4 stores may stay in flight
        if (i + 1 < nt) wait_vm<4>(); else wait_vm<0>();
    }
}

}  // namespace dtlr

using namespace dtlr;

// W [256, 256] row-major bf16 (host) -> fragment order with the channel permutation of proj_ln_k256_kernel (host, 65536 elements):
// block ((wave * 2 + e) * 8 + ks) lane (m, g) <- W[32 wave + 8 (m >> 2) + 4 e + (m & 3)][32 ks + 8 g ..]
extern "C" int dtlr_proj_ln_k256_pack_weights(const unsigned short* w_host, unsigned short* wp_host)
{
    if (!w_host || !wp_host) return DTLR_EINVAL;
    for (int wave = 0; wave < 8; ++wave)
        for (int e = 0; e < 2; ++e)
            for (int ks = 0; ks < 8; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int m = lane & 15, g = lane >> 4;
                    const int row = 32 * wave + 8 * (m >> 2) + 4 * e + (m & 3);
                    for (int x = 0; x < 8; ++x)
                        wp_host[((long)((wave * 2 + e) * 8 + ks) * 64 + lane) * 8 + x] = w_host[(long)row * 256 + ks * 32 + g * 8 + x];
                }
    return DTLR_OK;
}

extern "C" int dtlr_proj_ln_k256(const void* A, const void* Wp, const float* bias, const void* R, const float* gamma, const float* beta,
                                 float eps, void* Y, int M, void* stream)
{
    clear_stale_error();
    if (!A || !Wp || !bias || !R || !gamma || !beta || !Y) return DTLR_EINVAL;
    if (M <= 0) return DTLR_EINVAL;
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    const int ncu = 256;
    const int grid = ntiles < ncu ? ntiles : ncu;
    const int per = (ntiles + grid - 1) / grid;
    const int g2 = (ntiles + per - 1) / per;
    return launch<proj_ln_k256_kernel>(dim3(g2), dim3(512), PK_LDS, (hipStream_t)stream, (const uint16_t*)A, (const uint16_t*)Wp, bias,
                                       (const uint16_t*)R, gamma, beta, eps, (uint16_t*)Y, M, per);
}

// compute units of the current device, asked once (one persistent workgroup per CU)
static int k2_cu_count()
{
    static int cached = 0;
    if (!cached) { int d = 0; hipDeviceProp_t p; if (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0) cached = p.multiProcessorCount; else cached = 256; (void)hipGetLastError(); }
    return cached;
}

// W [N, 256] row-major bf16 (host memory) -> fragment order (host memory, N * 256 elements).
extern "C" int dtlr_k256_pack_weights(const unsigned short* w_host, unsigned short* wp_host, int N)
{
    if (!w_host || !wp_host) return DTLR_EINVAL;
    if (N != 256 && N != 384) return DTLR_ESHAPE;
    const int NRT = N / 128;
    for (int wave = 0; wave < 8; ++wave)
        for (int rt = 0; rt < NRT; ++rt)
            for (int ks = 0; ks < 8; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int m = lane & 15, g = lane >> 4;
                    const int row = (wave * NRT + rt) * 16 + m;
                    for (int e = 0; e < 8; ++e)
                        wp_host[((long)((wave * NRT + rt) * 8 + ks) * 64 + lane) * 8 + e] = w_host[(long)row * 256 + ks * 32 + g * 8 + e];
                }
    return DTLR_OK;
}

// value and [offsets | logits] of an unpadded batch in one pass over A (gemm_k256_vow_kernel): dtlr_gemm_k256's N = 640 form.
//     V[m, 0:256] = A[m, :] Wv^T + bias_v        O[m, :] = A[m, :] Wow^T + R[m % res_rows, :]        A [M, 256], O [M, 384], R [res_rows, 384]
static int k256_vow_launch(const void* A, const void* Wv, const float* bias_v, const void* Wow, const void* R, int res_rows,
                           void* V, int ldv, void* O, int M, hipStream_t st)
{
    if (ldv < 256 || (ldv & 7)) return DTLR_EINVAL;
    if ((res_rows % K2_TOK) || (M % res_rows) || (long)res_rows * 384 * 2 >= (1L << 31)) return DTLR_ESHAPE;
    const int ntiles = M / K2_TOK;
    const int ncu = k2_cu_count();
    const int grid = ntiles < ncu ? ntiles : ncu;
    const int per = (ntiles + grid - 1) / grid;
    const int g2 = (ntiles + per - 1) / per;
    return launch<gemm_k256_vow_kernel>(dim3(g2), dim3(512), VO_LDS, st, (const uint16_t*)A, (const uint16_t*)Wv, bias_v,
                                        (const uint16_t*)Wow, (const uint16_t*)R, res_rows, (uint16_t*)V, ldv, (uint16_t*)O, M, per, M / res_rows);
}

extern "C" int dtlr_gemm_k256(const void* A, const void* Wp, const float* bias, const void* resid, int res_rows,
                              const unsigned char* row_mask, void* C, int ldc, int M, int N, void* stream)
{
    clear_stale_error();
    if (!A || !Wp || !C) return DTLR_EINVAL;
    if (N == 640) {
        // both encoder projections: Wp = the N = 256 image then the N = 384 image, bias [256], resid [res_rows, 384]; C = V [M, ldc], then
        // O [M, 384] right behind it
        if (M <= 0 || !resid || res_rows <= 0 || row_mask) return DTLR_EINVAL;
        return k256_vow_launch(A, Wp, bias, (const uint16_t*)Wp + 256 * 256, resid, res_rows, C, ldc, (uint16_t*)C + (long)M * ldc, M, (hipStream_t)stream);
    }
    if (M <= 0 || ldc < N || (ldc & 7)) return DTLR_EINVAL;
    if (resid && (res_rows <= 0 || (long)res_rows * N * 2 >= (1L << 31))) return DTLR_EINVAL;
    if (N != 256 && N != 384) return DTLR_ESHAPE;
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    const int ncu = k2_cu_count();
    const int grid = ntiles < ncu ? ntiles : ncu;
    const int per = (ntiles + grid - 1) / grid;
    const int g2 = (ntiles + per - 1) / per;
    hipStream_t st = (hipStream_t)stream;
    static const bool pos_major = exp_env_int("DTLR_K256_POS_MAJOR", 1) != 0;   // experiment builds: A/B timing only
    const int n_img = (pos_major && resid && res_rows % K2_TOK == 0 && M % res_rows == 0 && M / res_rows > 1) ? M / res_rows : 0;
#define K2_LAUNCH(NRT, RES)                                                                        \
    {                                                                                              \
        return launch<gemm_k256_kernel<NRT, RES>>(dim3(g2), dim3(512), K2_LDS, st, (const uint16_t*)A, (const uint16_t*)Wp, bias, \
                                                  (const uint16_t*)resid, res_rows, row_mask, (uint16_t*)C, ldc, M, per, n_img);  \
    }
    if (N == 256) { if (resid) K2_LAUNCH(2, true) else K2_LAUNCH(2, false) }
    else { if (resid) K2_LAUNCH(3, true) else K2_LAUNCH(3, false) }
#undef K2_LAUNCH
}

// The column groups of dtlr_gemm_k256_multi for N = 256 L channels: N / 128 units over ceil(N / 640) groups, as evenly as they go; the
// first n_hi groups hold nrt_hi units, the others nrt_hi - 1.  False: N is not a positive multiple of 256.
static bool k256_multi_plan(int N, int* ngroups, int* nrt_hi, int* n_hi)
{
    if (N <= 0 || N % 256) return false;
    const int units = N / 128;
    *ngroups = (units + KM_MAX_NRT - 1) / KM_MAX_NRT;
    *nrt_hi = (units + *ngroups - 1) / *ngroups;
    *n_hi = units - (*nrt_hi - 1) * *ngroups;
    return true;
}

// W [N, 256] row-major (host) -> the groups' dtlr_k256_pack_weights-style images one after the other (host, N * 256 elements): group gi
// with nrt units starts at channel col0 (the units before it x 128), and its block ((wave * nrt + rt) * 8 + ks) = 64 lanes x 8 elements,
// lane (m, g) <- W[col0 + (wave * nrt + rt) * 16 + m][32 ks + 8 g ..].
extern "C" int dtlr_k256_multi_pack_weights(const unsigned short* w_host, unsigned short* wp_host, int N)
{
    if (!w_host || !wp_host) return DTLR_EINVAL;
    int ngroups, nrt_hi, n_hi;
    if (!k256_multi_plan(N, &ngroups, &nrt_hi, &n_hi)) return DTLR_ESHAPE;
    int col0 = 0;
    for (int gi = 0; gi < ngroups; ++gi) {
        const int nrt = gi < n_hi ? nrt_hi : nrt_hi - 1;
        unsigned short* img = wp_host + (long)col0 * 256;
        for (int wave = 0; wave < 8; ++wave)
            for (int rt = 0; rt < nrt; ++rt)
                for (int ks = 0; ks < 8; ++ks)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int m = lane & 15, g = lane >> 4;
                        const int row = col0 + (wave * nrt + rt) * 16 + m;
                        for (int e = 0; e < 8; ++e)
                            img[((long)((wave * nrt + rt) * 8 + ks) * 64 + lane) * 8 + e] = w_host[(long)row * 256 + ks * 32 + g * 8 + e];
                    }
        col0 += nrt * 128;
    }
    return DTLR_OK;
}

extern "C" int dtlr_gemm_k256_multi(const void* A, const void* Wp, const float* bias, const unsigned char* row_mask, void* C, int ldc,
                                    int M, int N, int K, void* stream)
{
    clear_stale_error();
    if (!A || !Wp || !C) return DTLR_EINVAL;
    if (M <= 0 || N <= 0 || ldc < N || (ldc & 7)) return DTLR_EINVAL;
    int ngroups, nrt_hi, n_hi;
    if (K != 256 || !k256_multi_plan(N, &ngroups, &nrt_hi, &n_hi)) return DTLR_ESHAPE;
    if (n_hi < ngroups && nrt_hi != KM_MAX_NRT) return DTLR_ESHAPE;      // (cannot happen for an even number of units)
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    // every workgroup resident at once, one per CU, and the groups of a token run a multiple of 8 workgroup ids apart (same XCD)
    int gx = k2_cu_count() / ngroups & ~7;
    if (gx < 8) gx = 8;
    const int per = (ntiles + gx - 1) / gx;
    gx = ((ntiles + per - 1) / per + 7) & ~7;
    hipStream_t st = (hipStream_t)stream;
#define KM_LAUNCH(NRT, MASK)                                                                       \
    return launch<gemm_k256_multi_kernel<NRT, MASK>>(dim3(gx, ngroups), dim3(512), KM_LDS, st, (const uint16_t*)A, (const uint16_t*)Wp, bias, \
                                                     row_mask, (uint16_t*)C, ldc, M, per, n_hi);
    switch (nrt_hi) {
    case 2: if (row_mask) { KM_LAUNCH(2, true) } else { KM_LAUNCH(2, false) }
    case 3: if (row_mask) { KM_LAUNCH(3, true) } else { KM_LAUNCH(3, false) }
    case 4: if (row_mask) { KM_LAUNCH(4, true) } else { KM_LAUNCH(4, false) }
    default: if (row_mask) { KM_LAUNCH(5, true) } else { KM_LAUNCH(5, false) }
    }
#undef KM_LAUNCH
}

extern "C" int dtlr_gemm_k256_a2(const void* A, const void* A2, const void* Wp, const float* bias, const unsigned char* row_mask, void* C,
                                 int M, int N, int K, void* stream)
{
    clear_stale_error();
    if (!A || !Wp || !C) return DTLR_EINVAL;
    if (M <= 0) return DTLR_EINVAL;
    if (N != 384 || K != 256) return DTLR_ESHAPE;
    const int ntiles = (M + K2_TOK - 1) / K2_TOK;
    const int ncu = k2_cu_count();
    const int grid = ntiles < ncu ? ntiles : ncu;
    const int per = (ntiles + grid - 1) / grid;
    const int g2 = (ntiles + per - 1) / per;
    hipStream_t st = (hipStream_t)stream;
    if (row_mask)
        return launch<gemm_k256_a2_kernel<true>>(dim3(g2), dim3(512), KA_LDS, st, (const uint16_t*)A, (const uint16_t*)A2, (const uint16_t*)Wp, bias,
                                                 row_mask, (uint16_t*)C, M, per);
    return launch<gemm_k256_a2_kernel<false>>(dim3(g2), dim3(512), KA_LDS, st, (const uint16_t*)A, (const uint16_t*)A2, (const uint16_t*)Wp, bias,
                                              row_mask, (uint16_t*)C, M, per);
}
