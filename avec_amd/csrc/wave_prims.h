// Wave-level device primitives of the MFMA kernels (gfx950, wave64), each defined once: the bf16 matrix instruction, the transposing LDS read, the LDS-DMA
// through M0 with its zero page, and the counted wait that goes with it.  Every kernel file that uses the matrix cores or the LDS-DMA includes this header
// (directly or through gemm_dev.h); the hardware rules behind each primitive are stated here and nowhere else.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((address_space(1))) const void* gptr_t;      // operands of __builtin_amdgcn_global_load_lds; (unsigned)(uintptr_t)(lptr_t)p is the LDS byte address of p
typedef __attribute__((address_space(3))) void* lptr_t;

// ---- v_mfma_f32_32x32x16_bf16: c += A (32 x 16) * B^T (32 x 16).  Lane l holds row l & 31, k-elements 8 (l >> 5) .. + 7 of both operands (16 bytes, as they lie in
// memory); c[r] is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of the 32 x 32 result.
__device__ __forceinline__ f32x16 mma16(const chunk16& a, const chunk16& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mma16(const u32x4& a, const u32x4& b, f32x16 c) {      // fragments as lds_read128 (gemm_dev.h) returns them
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// ---- ds_read_b64_tr_b16, the transposing LDS read: operands that lie [k][row] in LDS (the reduction index outermost, as the LDS-DMA copied them from memory).
// A 16-lane group reads a [4 k][16 rows] block and every lane receives the 4 consecutive k of ITS row: half of a 32x32x16 operand, so the lane layout is that of
// the block, not of a plain 8-byte read.  lds_tr8 packs the two halves (p0: k 0-3, p1: k 4-7 of the lane's eight) into one MFMA operand.  The 4 k-rows of a block
// must fall on distinct banks: the images are XOR-swizzled per 16-byte chunk on the DMA's source side (tr_swz in gemm.hip, aswz in attention_mfma.hip).
__device__ __forceinline__ chunk16 lds_tr8(const char* p0, const char* p1) {
  typedef __attribute__((address_space(3))) v4s_t* lp_t;
  const v4s_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)p0), b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)p1);
  const uint2 ua = __builtin_bit_cast(uint2, a), ub = __builtin_bit_cast(uint2, b);
  chunk16 f; f.w[0] = ua.x; f.w[1] = ua.y; f.w[2] = ub.x; f.w[3] = ub.y; return f;
}

// ---- LDS-DMA (global_load_lds_dwordx4): 16 bytes per lane from memory into LDS without a VGPR round trip; lane l of the wave writes lds_dst_uniform + 16 l.
//  * The LDS base travels in M0, which the compiler reserves and does not preserve around a statement (an "m0" clobber only draws a warning): M0 is saved, written,
//    used and restored inside ONE asm statement, with the s_nop 0 the hardware wants between the SALU write of M0 and the load that reads it.
//  * The DMA is hidden from hipcc on purpose (cdna_hip_programming.md 5.7): issued through __builtin_amdgcn_global_load_lds, the compiler drains the queue
//    (s_waitcnt vmcnt(0)) in front of the next LDS access it cannot prove disjoint from the DMA target, i.e. right behind a prefetch.  The asm form is absent from its
//    bookkeeping, so completion is counted by hand: AVEC_WAIT_VM(loads still allowed in flight), then a barrier, then the LDS reads; __syncthreads() does not wait.
//  * lds_dst_uniform must be provably wave-uniform ("s" operand: readfirstlane what derives from threadIdx).
//  * Source addresses need 2-byte alignment only (tools/glds_align_probe.hip: any even offset copies right).
//  * The DMA has no fill value: zero borders are read from the zero page below.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst_uniform) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_dst_uniform) : "memory");
}
// the same with a scalar base and a per-lane 32-bit byte offset (no 64-bit VALU address arithmetic on the issue path)
__device__ __forceinline__ void glds16_s(const void* sbase, unsigned voff, unsigned lds_dst_uniform) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst_uniform) : "memory");
}
// ... and N such pieces per lane as one group: LDS destinations lds0 + 4096 i (wave-uniform), M0 saved and restored once per group
#define AVEC_GLDS_HEAD "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
#define AVEC_GLDS_NEXT(k) "s_add_u32 m0, m0, 0x1000\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %" #k ", %2\n\t"
#define AVEC_GLDS_TAIL "s_mov_b32 m0, %0"
template <int N> __device__ __forceinline__ void glds16_group(const unsigned (&v)[N], const void* sbase, unsigned lds0) {
  static_assert(N >= 1 && N <= 5, "group size");
  unsigned keep;
  if constexpr (N == 1) asm volatile(AVEC_GLDS_HEAD AVEC_GLDS_TAIL : "=&s"(keep) : "v"(v[0]), "s"(sbase), "s"(lds0) : "memory", "scc");
  if constexpr (N == 2) asm volatile(AVEC_GLDS_HEAD AVEC_GLDS_NEXT(4) AVEC_GLDS_TAIL : "=&s"(keep) : "v"(v[0]), "s"(sbase), "s"(lds0), "v"(v[1]) : "memory", "scc");
  if constexpr (N == 3) asm volatile(AVEC_GLDS_HEAD AVEC_GLDS_NEXT(4) AVEC_GLDS_NEXT(5) AVEC_GLDS_TAIL : "=&s"(keep) : "v"(v[0]), "s"(sbase), "s"(lds0), "v"(v[1]), "v"(v[2]) : "memory", "scc");
  if constexpr (N == 4) asm volatile(AVEC_GLDS_HEAD AVEC_GLDS_NEXT(4) AVEC_GLDS_NEXT(5) AVEC_GLDS_NEXT(6) AVEC_GLDS_TAIL
                                     : "=&s"(keep) : "v"(v[0]), "s"(sbase), "s"(lds0), "v"(v[1]), "v"(v[2]), "v"(v[3]) : "memory", "scc");
  if constexpr (N == 5) asm volatile(AVEC_GLDS_HEAD AVEC_GLDS_NEXT(4) AVEC_GLDS_NEXT(5) AVEC_GLDS_NEXT(6) AVEC_GLDS_NEXT(7) AVEC_GLDS_TAIL
                                     : "=&s"(keep) : "v"(v[0]), "s"(sbase), "s"(lds0), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]) : "memory", "scc");
}
#undef AVEC_GLDS_HEAD
#undef AVEC_GLDS_NEXT
#undef AVEC_GLDS_TAIL

// at most n of this wave's vector-memory loads (the hand-counted LDS-DMA above) are still in flight behind this point; n is a compile-time constant
#define AVEC_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")

// 64 zero bytes, the LDS-DMA source of zero borders, invalid rows / taps and K tails.  One copy per translation unit (no relocatable device code in this build);
// nothing on the host names it.  An inline variable, not a static one: kernels name it inside lambdas, which are implicitly __host__ __device__, and clang treats
// that as a use by host code -- a static variable then gets external linkage and is reached through the GOT (a scalar load in front of every use), one that no
// lambda names becomes a local symbol whose known contents change the code around it.  The inline variable is addressed by a pc-relative literal, like a plain
// __device__ global.  (stem3p.hip has a static page of its own: its kernels were tuned with the GOT form and keep their code.)
inline __device__ __attribute__((aligned(64))) unsigned char avec_zero16[64];
