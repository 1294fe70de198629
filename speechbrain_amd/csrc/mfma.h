// MFMA fragment traits shared by the GEMM and attention kernels.
//
// One abstraction for both compute dtypes: a lane of a 16x16 MFMA tile holds
// 8 consecutive K elements (k = 8*(lane>>4) + j, j = 0..7) of its A row and
// of its B column.
//   bf16: one v_mfma_f32_16x16x32_bf16 consumes the 8-element fragment.
//   f32 : eight v_mfma_f32_16x16x4_f32 (exact f32 FMA chains), instruction s
//         taking element s of every lane group, so together they cover the
//         same 32-wide K slice.  This keeps LDS layouts identical across
//         dtypes (8 contiguous K elements per lane = one or two 16-B reads).
// C/D layout of 16x16 MFMA: col = lane & 15, row = 4*(lane >> 4) + reg.
#pragma once
#include "sbk_common.h"

namespace sbk {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef uint16_t bf16_t;  // bf16 storage

template <typename T>
struct MT;

// k-transposed bf16 fragment from a row-major [k][ld] tile X in LDS: the
// operand rows are X's columns dbase + (lane & 15), the 8 k are
// {k0 + 4g .. k0 + 4g + 3} ∪ {k0 + 16 + 4g .. +3}.  Two transposing reads
// (ds_read_b64_tr_b16): lane 4q+p of each 16-lane group addresses row q,
// columns 4p..4p+3 of the block.  swz(row) is XORed onto the row's 16-B chunk
// index (it must be equal for rows r and r + 16); NoSwizzle: plain rows.
struct NoSwizzle {
  __device__ __forceinline__ int operator()(int) const { return 0; }
};
template <typename Swz = NoSwizzle>
__device__ __forceinline__ bf16x8 frag_tr(const bf16_t* X, int ld, int k0, int dbase, int lane, Swz swz = Swz{}) {
  typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int r0 = k0 + 4 * g + q, col = dbase + 4 * p;
  const bf16_t* a0 = X + r0 * ld + ((((col >> 3) ^ swz(r0)) << 3) | (col & 7));
  const bf16_t* a1 = a0 + 16 * ld;
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)(a0));
  const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)(a1));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <>
struct MT<bf16_t> {
  using frag = bf16x8;
  static constexpr int VEC = 8;  // elements per 16-byte chunk
  static constexpr int PAD = 8;  // LDS row padding (elements) = 16 bytes
  __device__ static __forceinline__ frag load(const bf16_t* p) { return *reinterpret_cast<const frag*>(p); }
  __device__ static __forceinline__ void mma(f32x4& c, const frag& a, const frag& b) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  __device__ static __forceinline__ frag zero() { return frag{}; }
  // elements 0..3 from p0, 4..7 from p1 (permuted-k fragments)
  __device__ static __forceinline__ frag load2x4(const bf16_t* p0, const bf16_t* p1) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const bf16x4 a = *reinterpret_cast<const bf16x4*>(p0);
    const bf16x4 b = *reinterpret_cast<const bf16x4*>(p1);
    return frag{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  }
  __device__ static __forceinline__ frag from8(const float* v) {
    frag f;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (__bf16)v[i];
    return f;
  }
  __device__ static __forceinline__ bf16_t from_f32(float v) { return f32_to_bf16(v); }
  __device__ static __forceinline__ float to_f32(bf16_t v) { return bf16_to_f32(v); }
};

template <>
struct MT<float> {
  using frag = f32x8;
  static constexpr int VEC = 4;
  static constexpr int PAD = 4;
  __device__ static __forceinline__ frag load(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    frag v;
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    return v;
  }
  __device__ static __forceinline__ void mma(f32x4& c, const frag& a, const frag& b) {
#pragma unroll
    for (int s = 0; s < 8; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], c, 0, 0, 0);
  }
  __device__ static __forceinline__ frag zero() { return frag{}; }
  __device__ static __forceinline__ frag load2x4(const float* p0, const float* p1) {
    const float4 a = *reinterpret_cast<const float4*>(p0);
    const float4 b = *reinterpret_cast<const float4*>(p1);
    frag v;
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    return v;
  }
  __device__ static __forceinline__ frag from8(const float* v) {
    frag f;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = v[i];
    return f;
  }
  __device__ static __forceinline__ float from_f32(float v) { return v; }
  __device__ static __forceinline__ float to_f32(float v) { return v; }
};

}  // namespace sbk
