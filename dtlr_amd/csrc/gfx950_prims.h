// The inline-asm and MFMA primitives of the gfx950 kernels: ONE definition of each, included by every .hip file that stages through the
// LDS-DMA, counts its own waits or issues MFMAs (dtlr_common.h does not include it).  What the compiler cannot check about them:
//
// 1. M0.  The LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 bytes, global -> LDS without VGPR staging) takes its destination from M0: the
//    wave-uniform LDS byte address, to which the hardware adds 16 * lane (+ the instruction's immediate offset, which also applies to the
//    global address).  hipcc reserves M0 for itself and neither preserves it around an asm statement nor accepts it as a clobber, so every
//    statement here saves M0 to a scratch SGPR, sets it, issues the load and restores it -- all inside ONE string.  `s_nop 0` is the one wait
//    state the hardware requires between an SALU write of M0 and the LDS-DMA that reads it; nobody inserts it inside an asm string.
// 2. Waits.  A load issued from an asm string is absent from hipcc's s_waitcnt bookkeeping: the compiler emits no wait for it.  That is the
//    point of load16 and the glds16 family (a compiler-counted load in a ring loop is waited for with vmcnt(0) at the back-edge, which drains
//    the whole DMA queue every iteration), and it is the caller's debt: count the loads issued after the ones you need and wait with
//    vmcnt(N) yourself.  LDS-DMA data additionally needs a workgroup barrier between the wait and another wave's ds_read (__syncthreads alone
//    does not wait for it); a load16 destination must not be read, copied or spilled before its wait.  Two wait forms, kept apart on purpose:
//    wait_vm<N> ends with sched_barrier(0), so nothing -- in particular no MFMA or register-only consumer, which a "memory" clobber does not
//    order -- is scheduled across it; DTLR_WAITCNT* is the bare instruction, for places whose surrounding code pins the order already
//    (a barrier follows, or the consumers are LDS reads the "memory" clobber orders).
// 3. MFMA hazards.  The builtin forms (mma16*, mma32, mma32_f16) are ordinary instructions to hipcc: it schedules them and pads their hazards.
//    The asm forms (mma32_v0 / mma32_v, and the AGPR-tied ones ffn4.hip keeps) are invisible to the hazard recogniser: no wait states are
//    inserted between them and their neighbours.  Callers owe: A / B operands that are not fresh VALU results (ds_read results or long-lived
//    registers: the compiler waits for asm inputs, but pads no VALU-write -> MFMA-read hazard), an accumulator that is next touched by the
//    following MFMA as its whole SrcC or by a VALU reader at least two issued MFMAs (or an explicit s_nop pad) later.
#pragma once
#include "dtlr_common.h"

namespace dtlr {

// ---- vector types (h16 = the library's 16-bit format, f16 = always IEEE fp16: the hi / lo split engines) ----------------------------------
typedef __attribute__((ext_vector_type(8))) h16_hw_t h16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

// ---- LDS-DMA (note 1; uncounted: note 2) --------------------------------------------------------------------------------------------------
// per-lane 64-bit source address
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// wave-uniform base in SGPRs + 32-bit per-lane byte offset (one VGPR instead of a 64-bit address per source)
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// same with an immediate byte offset (< 4096) that applies to BOTH the global address and the LDS destination: pieces that lie equally far
// apart in both (the 1 KB fragments of a chunk image) share one base pair.  OFF must fold to a constant (template argument).
template <int OFF> __device__ __forceinline__ void glds16so(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%4\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst), "n"(OFF) : "memory");
}

// ---- 16-byte global load the compiler does not count (note 2) -----------------------------------------------------------------------------
__device__ __forceinline__ uint4 load16(const void* p) {
    uint4 r;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}

// ---- hand-counted waits (note 2) ----------------------------------------------------------------------------------------------------------
// vmcnt(N), then a scheduling barrier
template <int N> __device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// the bare instruction, NO scheduling barrier; the counter that is not named is "don't care".  Macros that paste the counts into the string,
// not a template with "n" operands: an asm statement with operands weighs more in hipcc's loop cost model than one without, and in
// gemm_k256s.hip that alone changed how the tile loop was laid out.  The counts are literal numbers (vmcnt < 64, lgkmcnt < 16).
#define DTLR_WAITCNT(VM, LGKM) asm volatile("s_waitcnt vmcnt(" #VM ") lgkmcnt(" #LGKM ")" ::: "memory")
#define DTLR_WAITCNT_VM(VM) asm volatile("s_waitcnt vmcnt(" #VM ")" ::: "memory")
#define DTLR_WAITCNT_LGKM(LGKM) asm volatile("s_waitcnt lgkmcnt(" #LGKM ")" ::: "memory")

// ---- MFMA on two 16-byte fragments (note 3).  mma16 / mma32: the library's 16-bit format (bf16, or fp16 under -DDTLR_HALF_IS_F16);
// *_f16: always fp16 (the hi / lo split kernels, whatever the library's format) ---------------------------------------------------------------
__device__ __forceinline__ f32x4_t mma16(const uint4& a, const uint4& b, f32x4_t c) {              // 16x16x32
    return DTLR_MFMA_16x16x32_H16(__builtin_bit_cast(h16x8_t, a), __builtin_bit_cast(h16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mma16_f16(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16_t mma32(const uint4& a, const uint4& b, f32x16_t c) {            // 32x32x16
    return DTLR_MFMA_32x32x16_H16(__builtin_bit_cast(h16x8_t, a), __builtin_bit_cast(h16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16_t mma32_f16(const uint4& a, const uint4& b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
// 32x32x16 with the accumulator pinned to ARCHITECTURAL VGPRs (read by the VALU right after; left to itself hipcc parks every accumulator in
// the AGPRs and shuttles tiles through v_accvgpr moves).  Inline asm: note 3.
__device__ __forceinline__ void mma32_v0(const uint4& a, const uint4& b, f32x16_t& c) {            // c = a b: a true definition of c
    const u32x4_t av = {a.x, a.y, a.z, a.w}, bv = {b.x, b.y, b.z, b.w};
    asm volatile("v_mfma_f32_32x32x16_" DTLR_H16_ASM_SUFFIX " %0, %1, %2, 0" : "=&v"(c) : "v"(av), "v"(bv));
}
__device__ __forceinline__ void mma32_v(const uint4& a, const uint4& b, f32x16_t& c) {             // c += a b
    const u32x4_t av = {a.x, a.y, a.z, a.w}, bv = {b.x, b.y, b.z, b.w};
    asm volatile("v_mfma_f32_32x32x16_" DTLR_H16_ASM_SUFFIX " %0, %1, %2, %0" : "+v"(c) : "v"(av), "v"(bv));
}

// ---- conversions --------------------------------------------------------------------------------------------------------------------------
// 2 fp32 -> packed fp16 hi pair and lo pair (lo = fp16(x - hi): the difference is exact, both conversions round to nearest even)
__device__ __forceinline__ void split2_f16(float x0, float x1, uint32_t& hi, uint32_t& lo) {
    const f16x2_t a = __builtin_convertvector(f32x2_hw_t{x0, x1}, f16x2_t);
    const f16x2_t b = __builtin_convertvector(f32x2_hw_t{x0 - (float)a[0], x1 - (float)a[1]}, f16x2_t);
    hi = __builtin_bit_cast(uint32_t, a);
    lo = __builtin_bit_cast(uint32_t, b);
}
// 8 values of the library's 16-bit format -> 8 floats
__device__ __forceinline__ void unpack8_h16(const uint4& t, float (&v)[8]) {
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = h16_lo(w[i]); v[2 * i + 1] = h16_hi(w[i]); }
}
// ReLU as ONE instruction, v_med3_f32(x, 0, +inf) (fmaxf canonicalises its operand first: two v_max per value)
__device__ __forceinline__ float relu_med3(float x) { return __builtin_amdgcn_fmed3f(x, 0.f, __builtin_huge_valf()); }

// ---- DPP lane move (quad_perm / row_shr / ... by CTRL), all rows and banks enabled.  BOUND_CTRL is spelled out at every call: false = a lane
// whose source is out of bounds keeps the `old` operand (0 here), true = it reads 0 through bound_ctrl; the two encode differently -----------
template <int CTRL, bool BOUND_CTRL> __device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, BOUND_CTRL); }
template <int CTRL, bool BOUND_CTRL> __device__ __forceinline__ float dpp_f(float v) { return __int_as_float(dpp_i<CTRL, BOUND_CTRL>(__float_as_int(v))); }
template <int CTRL, bool BOUND_CTRL> __device__ __forceinline__ uint32_t dpp_u(uint32_t v) { return (uint32_t)dpp_i<CTRL, BOUND_CTRL>((int)v); }

}  // namespace dtlr
