// What a recurrent step kernel is made of, shared by gru.hip and lstm.hip.
//
// One launch per time step, forward and backward; the dependency between
// steps is stream order.  No persistent kernel, no grid barrier, no flag
// between workgroups, no float atomics.  The host side of the library
// enqueues all launches of a layer (launch_steps), so a sequence costs one
// call into the library.
//
// A workgroup of 8 waves owns 16 hidden units (one MFMA tile of columns) and
// up to 32 batch rows (kMT row tiles).  Its recurrent product is
//   acc[m][g] = A[b0 + 16m .., :K] . W[g * gate_rows + j0 .., :K]^T
// for the G gates of a forward step (A = the previous h, K = H) or the one
// tile of a backward step (A = the arriving gate gradients, W = W_hh^T,
// K = G' * H).  The rows of W are MFMA B operands read from memory as they are
// (8 consecutive K elements per lane); the fp32 rows of A are the A operand,
// rounded to bf16 in bf16 mode (exact-fp32 MFMA in fp32 mode).  K is dealt to
// the eight waves in 32-element chunks (product; the backward kernels keep
// the one-tile form of that loop in place, see there); their partial tiles
// meet in LDS (meet) and are added in wave order 0 .. 7 (total), which makes a
// result independent of everything but its operands.  The cell's epilogue then
// runs one (row, unit) pair per thread.
#pragma once
#include "mfma.h"

namespace sbk {
namespace rnnstep {

constexpr int kThreads = 512;
constexpr int kWaves = 8;
constexpr int kSlice = 16;  // hidden units of a workgroup: one MFMA tile
constexpr int kRows = 32;   // batch rows of a workgroup
constexpr int kMT = kRows / 16;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 8 elements row[k0 .. k0 + 8) of a K-element row as an MFMA fragment, zero
// past K.  vec: the row start and K allow 16-byte reads.
template <typename T>
__device__ __forceinline__ typename MT<T>::frag load_w8(const T* row, int k0, int K, bool vec) {
  if (vec && k0 + 8 <= K) return MT<T>::load(row + k0);
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = k0 + i < K ? MT<T>::to_f32(row[k0 + i]) : 0.f;
  return MT<T>::from8(v);
}

// the same from an fp32 row, converted to T
template <typename T>
__device__ __forceinline__ typename MT<T>::frag load_f8(const float* row, int k0, int K, bool vec) {
  float v[8];
  if (vec && k0 + 8 <= K) {
    const float4 a = *reinterpret_cast<const float4*>(row + k0);
    const float4 b = *reinterpret_cast<const float4*>(row + k0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = k0 + i < K ? row[k0 + i] : 0.f;
  }
  return MT<T>::from8(v);
}

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

// Row of the one-hot input's table that token v reads: the blank has none
// (-1), ids above it are shifted down.
__device__ __forceinline__ int token_row(int v, int blank) {
  return v == blank ? -1 : (v < blank ? v : v - 1);
}

// out[m][g] = A[b0 + 16m + (lane & 15), :K] . W[g * gate_rows + j0 + (lane & 15), :K],
// this wave's share of K; zero for a null A, past H units and past B rows.
// The accumulators are local and copied out once: accumulated through the
// reference they cost the forward kernels 18-28 VGPRs of copies.
// G = 3, 4: with G = 1 the one-element fragment array compiles to eight bound
// compares at the head of every iteration that the scalar form does not have.
template <typename T, int G>
__device__ __forceinline__ void product(f32x4 (&out)[kMT][G], const T* W, int gate_rows, int K, const float* A,
                                        long long lda, int j0, int b0, int B, int H, int mts, bool vec_w,
                                        bool vec_a, int lane, int w) {
  f32x4 acc[kMT][G];
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int g = 0; g < G; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (A) {
    const int unit = j0 + (lane & 15);
#pragma unroll 2
    for (int k0 = w * 32; k0 < K; k0 += kWaves * 32) {
      const int kk = k0 + 8 * (lane >> 4);
      typename MT<T>::frag bw[G];
#pragma unroll
      for (int g = 0; g < G; ++g)
        bw[g] = unit < H ? load_w8<T>(W + ((long long)g * gate_rows + unit) * K, kk, K, vec_w) : MT<T>::zero();
#pragma unroll
      for (int m = 0; m < kMT; ++m) {
        if (m < mts) {
          const int row = b0 + m * 16 + (lane & 15);
          const typename MT<T>::frag af = row < B ? load_f8<T>(A + row * lda, kk, K, vec_a) : MT<T>::zero();
#pragma unroll
          for (int g = 0; g < G; ++g) MT<T>::mma(acc[m][g], af, bw[g]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int g = 0; g < G; ++g) out[m][g] = acc[m][g];
}

// The partial tiles of the eight waves meet in LDS: red[w][g][16m + 4 *
// (lane >> 4) + r][lane & 15] = acc[m][g][r].  The constant part of the index
// is kept apart from the lane's, which keeps the paired 64-byte-stride stores.
template <int G>
__device__ __forceinline__ void meet(float (&red)[kWaves][G][kRows][kSlice], const f32x4 (&acc)[kMT][G], int mts,
                                     int lane, int w) {
  float* mine = &red[w][0][4 * (lane >> 4)][lane & 15];
#pragma unroll
  for (int m = 0; m < kMT; ++m) {
    if (m < mts) {
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[(g * kRows + m * 16 + r) * kSlice] = acc[m][g][r];
    }
  }
  __syncthreads();
}

// gate g of (row rr, unit jj): the partial sums added in wave order
template <int G>
__device__ __forceinline__ float total(const float (&red)[kWaves][G][kRows][kSlice], int g, int rr, int jj) {
  float s = red[0][g][rr][jj];
#pragma unroll
  for (int ww = 1; ww < kWaves; ++ww) s += red[ww][g][rr][jj];
  return s;
}

// n launches of a step kernel on grid (ceil(H / 16), ceil(B / 32), D), steps
// first, first + dir, ...
template <typename Args>
inline int launch_steps(void (*kernel)(Args, int), const Args& a, int D, int first, int n, int dir, void* stream) {
  const dim3 grid((a.H + kSlice - 1) / kSlice, (a.B + kRows - 1) / kRows, D);
  for (int i = 0; i < n; ++i) {
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, a, first + i * dir);
    SBK_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace rnnstep
}  // namespace sbk
