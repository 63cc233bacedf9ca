// The split-bf16 ("x6") device primitives, defined once for linear.hip,
// graphconv.hip and attention.hip.  An fp32 value v is
// v0 + v1 + v2 with v0 = bf16(v), v1 = bf16(v - v0), v2 = bf16(v - v0 - v1)
// (round to nearest even; exact for 2^-100 <= |v| < 3.39e38:
// tests/test_x6_split.py), and a product of two such values is the six plane
// products a_i b_j with i + j <= 2 on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation.  The kernels that must agree bitwise (the one-kernel GraphConv
// and the SpMM + GEMM chain) agree because they share these functions.
// That every kernel issues each of the six products, from the right planes
// at every fragment and staging slot, is checked on inputs where one product
// sum decides each output element, within 2^-22 of the float64 product:
// tests/test_gpu_x6_planes.py (the numpy model of the six products and the
// proof that a single wrong product breaks the bound: tests/x6_isolate.py,
// tests/test_x6_isolate.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace grl {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef short i16x4_t __attribute__((ext_vector_type(4)));
typedef short i16x8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) uint16_t lds_u16;

// ---- split and pack --------------------------------------------------------
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
  f32x2_t p = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(p, bf16x2_t));
}
__device__ __forceinline__ float lo_f(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hi_f(uint32_t u) { return __uint_as_float(u & 0xFFFF0000u); }

// one value -> its three bf16 parts (v == p0 + p1 + p2 exactly)
__device__ __forceinline__ void split1(float v, uint16_t& p0, uint16_t& p1, uint16_t& p2) {
  const uint32_t h0 = pack_bf16(v, 0.0f) & 0xFFFFu;
  const float r1 = v - lo_f(h0);
  const uint32_t h1 = pack_bf16(r1, 0.0f) & 0xFFFFu;
  const float r2 = r1 - lo_f(h1);
  const uint32_t h2 = pack_bf16(r2, 0.0f) & 0xFFFFu;
  p0 = (uint16_t)h0;
  p1 = (uint16_t)h1;
  p2 = (uint16_t)h2;
}

// v (4 floats) -> three planes of 4 bf16 (v == p0 + p1 + p2 exactly)
__device__ __forceinline__ void split3(float4 v, uint2& p0, uint2& p1, uint2& p2) {
  p0.x = pack_bf16(v.x, v.y);
  p0.y = pack_bf16(v.z, v.w);
  float4 r = make_float4(v.x - lo_f(p0.x), v.y - hi_f(p0.x), v.z - lo_f(p0.y), v.w - hi_f(p0.y));
  p1.x = pack_bf16(r.x, r.y);
  p1.y = pack_bf16(r.z, r.w);
  r = make_float4(r.x - lo_f(p1.x), r.y - hi_f(p1.x), r.z - lo_f(p1.y), r.w - hi_f(p1.y));
  p2.x = pack_bf16(r.x, r.y);
  p2.y = pack_bf16(r.z, r.w);
}

// 8 floats -> three bf16x8 planes
__device__ __forceinline__ void split8(float4 lo, float4 hi, bf16x8_t& a0, bf16x8_t& a1, bf16x8_t& a2) {
  uint2 l0, l1, l2, h0, h1, h2;
  split3(lo, l0, l1, l2);
  split3(hi, h0, h1, h2);
  a0 = __builtin_bit_cast(bf16x8_t, make_uint4(l0.x, l0.y, h0.x, h0.y));
  a1 = __builtin_bit_cast(bf16x8_t, make_uint4(l1.x, l1.y, h1.x, h1.y));
  a2 = __builtin_bit_cast(bf16x8_t, make_uint4(l2.x, l2.y, h2.x, h2.y));
}

// ---- the six plane products -------------------------------------------------
// one plane product: acc += a b over one 32x32x16 block
__device__ __forceinline__ void mfma_bf16(f32x16& acc, bf16x8_t a, bf16x8_t b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}

// acc += a b for split operands.  The order is a numerical contract:
// small terms first (i + j = 2, then 1), the leading product a0 b0 last.
// Every x6 kernel runs this sequence, so kernels computing the same product
// from the same planes give the same bits.
__device__ __forceinline__ void x6_mfma(f32x16& acc, bf16x8_t a0, bf16x8_t a1, bf16x8_t a2, bf16x8_t b0, bf16x8_t b1, bf16x8_t b2) {
  mfma_bf16(acc, a2, b0);
  mfma_bf16(acc, a1, b1);
  mfma_bf16(acc, a0, b2);
  mfma_bf16(acc, a1, b0);
  mfma_bf16(acc, a0, b1);
  mfma_bf16(acc, a0, b0);
}
// (planes held in arrays: the same six products, spelled out rather than
// forwarded -- copying the planes out of the arrays first changed the
// register allocation of graphconv_ws_kernel)
__device__ __forceinline__ void x6_mfma(f32x16& acc, const bf16x8_t (&a)[3], const bf16x8_t (&b)[3]) {
  mfma_bf16(acc, a[2], b[0]);
  mfma_bf16(acc, a[1], b[1]);
  mfma_bf16(acc, a[0], b[2]);
  mfma_bf16(acc, a[1], b[0]);
  mfma_bf16(acc, a[0], b[1]);
  mfma_bf16(acc, a[0], b[0]);
}

// acc += a b for a split a and a b that is ONE bf16 plane (values stored as
// bf16: b1 = b2 = 0): x6_mfma's sequence without its three products on a zero
// plane.  Those add exact zeros to an accumulator that is never -0 (it starts
// at +0), so the result is bitwise x6_mfma's on the widened b.
__device__ __forceinline__ void x3_mfma(f32x16& acc, const bf16x8_t (&a)[3], bf16x8_t b) {
  mfma_bf16(acc, a[2], b);
  mfma_bf16(acc, a[1], b);
  mfma_bf16(acc, a[0], b);
}

// acc += a b for an a that is ONE bf16 plane (values stored as bf16:
// a1 = a2 = 0) and a split b: x6_mfma's sequence without its three products
// on a zero plane (a2 b0, a1 b1, a1 b0), leaving a b2, a b1, a b0 in that
// order.  The MFMA's operand positions are not interchangeable, so this is
// not x3_mfma with its arguments swapped.  The skipped products add sums of
// +-0 to the accumulator: x + (+-0) = x for x != 0 and +0 + (+-0) = +0 under
// round to nearest, so an accumulator that starts at +0 (never -0 afterwards)
// gets x6_mfma's bits on the widened a (DESIGN.md §4.19's argument).  An
// accumulator that can hold -0 when the call begins (the attention forward's
// o after an alpha rescale that underflowed) keeps it here where x6_mfma's
// first zero product turns it into +0: equal values, a zero's sign apart
// (DESIGN.md §4.22).
__device__ __forceinline__ void x3a_mfma(f32x16& acc, bf16x8_t a, const bf16x8_t (&b)[3]) {
  mfma_bf16(acc, a, b[2]);
  mfma_bf16(acc, a, b[1]);
  mfma_bf16(acc, a, b[0]);
}

// acc += a b for an a and a b that are each ONE bf16 plane (both stored as
// bf16): the single product a0 b.  It is bitwise x3_mfma on an a whose planes
// 1 and 2 are +0 (what split3 gives for a value that is a bf16 already: both
// residuals are v - v = +0): that sequence runs a2 b and a1 b first, and each
// adds sums of +-0 products to an accumulator that starts at +0 and, under
// round to nearest, is never -0 afterwards (x + (+-0) = x for x != 0, and
// +0 + (-0) = +0), so the accumulator a0 b meets is the one it meets here
// (DESIGN.md §4.19's argument, applied to the other operand: §4.21).
__device__ __forceinline__ void x1_mfma(f32x16& acc, bf16x8_t a, bf16x8_t b) { mfma_bf16(acc, a, b); }

// ---- LDS-DMA ----------------------------------------------------------------
// global -> LDS DMA of one 16 B chunk per lane (lane l lands at lds_base + 16 l).
// Issued from asm so that hipcc's waitcnt pass neither sees nor waits on it
// (seeing an LDS write in flight, it would wait vmcnt(0) before every ds_read);
// completion is ordered by the kernel's counted `s_waitcnt vmcnt` and barrier.
// M0 = the wave-uniform LDS byte address, saved and restored around the load.
__device__ __forceinline__ void dma16(const void* src, const void* lds_base) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(lds_base));
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(dst)
      : "memory");
}

// ---- transposed LDS reads ---------------------------------------------------
// Two ds_read_b64_tr_b16 (per 16-lane group a 4 row x 16 column block, lane i
// receiving column i: cdna_hip_programming.md T10) -> one MFMA fragment of 8
// consecutive k.  tr8s takes LDS-space pointers, so constant offsets fold into
// the reads' immediates; tr8 takes generic pointers into LDS.
__device__ __forceinline__ bf16x8_t tr8s(const lds_u16* p0, const lds_u16* p1) {
  typedef __attribute__((address_space(3))) i16x4_t lds_v4;
  const i16x4_t x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)p0);
  const i16x4_t x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)p1);
  const i16x8_t v = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t tr8(const uint16_t* p0, const uint16_t* p1) {
  return tr8s((const lds_u16*)(uintptr_t)(uint32_t)(uintptr_t)p0, (const lds_u16*)(uintptr_t)(uint32_t)(uintptr_t)p1);
}

}  // namespace grl
