// The CRDNN CNN_Block layer in one launch: Conv2d 3x3, stride 1, "same"
// reflect padding -> LayerNorm over (freq, chan) -> LeakyReLU -> [max-pool over
// frequency] -> [per-(utterance, bin) scale] (lobes/models/CRDNN.py:197-276),
// and the element-wise part of its backward in one launch.
//
// Forward (conv_ln_kernel).  A workgroup of four waves owns TF whole time
// frames of one utterance: M = TF * F output rows (row m = (frame, bin)) by
// N = Co columns, K = 9 * Ci, an implicit GEMM.  No col matrix exists: the
// input slab (TF + 2 frames, F + 2 bins, Ci channels, the reflection applied
// as it is staged) lies in LDS once, and tap (kt, kf) of the A operand is the
// same slab read at a row offset of (kt (F + 2) + kf).  The weights come as an
// image of K-chunks of 32 (tap-major, Ci padded to 32 per tap), each chunk the
// byte image of its LDS tile (Co rows of 32 + pad), streamed L2 -> LDS by
// LDS-DMA through a ring of two stages: chunk j + 1 is in flight while chunk j
// feeds the MFMAs.  Wave w holds the 16-column tiles w, w + 4, ... of all (up
// to 10) 16-row tiles: up to 40 accumulator tiles, so a weight fragment read
// from LDS is used for ten MFMAs and a slab fragment for four.
// 9 Ci <= 32 (the lobe's first conv, Ci = 1): all nine taps are one K-chunk,
// the A fragment gathered tap by tap from the slab — one padded MFMA step.
//
// Epilogue.  bias; the pre-norm output is stored as c in the compute dtype
// for the backward, while the statistics and y come from the fp32
// accumulators (no extra rounding in the forward); per-row sums
// over the wave's columns by DPP, across waves and rows of a frame through
// LDS, mean then centred variance; then frame by frame the normalised rows go
// to an LDS tile (F, Co) fp32 and every thread finishes whole output vectors:
// affine, LeakyReLU, the pool's maximum over its p bins, the scale, one
// contiguous store of the pooled frame.
//
// Backward epilogue (conv_ln_bwd_kernel).  A workgroup walks frames
// blockIdx.x, + gridDim.x, ...: it recomputes the normalised values and
// activations from c, mean and rstd, routes dy to the first maximum of each
// pool window, applies LeakyReLU' and the LayerNorm backward, writes dc, and
// keeps its dgamma / dbeta sums in LDS (every element has one owner thread,
// in a fixed order: no atomics, bit-identical runs), stored once per
// workgroup as partials for sbk_colsum.
#include "lds_dma.h"
#include "mfma.h"
#include "sbk_common.h"

namespace sbk {
namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = 4;
constexpr int CL_MT = 10;              // 16-row tiles of a workgroup
constexpr int CL_ROWS = 16 * CL_MT;    // at most 160 output rows (frames * bins)
constexpr int CL_NT = 4;               // 16-column tiles of a wave: Co <= 256
constexpr int CL_TFMAX = 8;            // frames of a workgroup
constexpr int CL_KC = 32;              // K of a ring stage
constexpr int CL_DMAX = 16384;         // F * Co (the LDS frame tile; the LayerNorm backward's limit too)
constexpr int CL_LDS = 160 * 1024;
constexpr int CL_SMALL = (CL_WAVES * CL_ROWS + 2 * CL_TFMAX) * (int)sizeof(float);
constexpr int CL_BWD_THREADS = 512;

struct ClPlan {
  int tf;           // frames per workgroup
  int packed;       // 9 Ci <= 32: all taps in one K-chunk
  int cip;          // slab row stride, elements
  int cb;           // 32-channel blocks per tap
  int kchunks;      // ring chunks
  int stage_bytes;  // one chunk / ring stage (a multiple of 1 KB)
  int slab_bytes;
  int lds_bytes;
};

template <typename T>
bool cl_plan(int F, int Ci, int Co, ClPlan& p) {
  if (F < 2 || F > CL_ROWS || Ci < 1 || Co < 16 || Co > 16 * CL_NT * CL_WAVES || Co % 16) return false;
  if ((long long)F * Co > CL_DMAX || Ci > 4096) return false;
  p.packed = 9 * Ci <= CL_KC;
  const int cir = (Ci + CL_KC - 1) / CL_KC * CL_KC;
  p.cip = p.packed ? Ci : cir + MT<T>::PAD;
  p.cb = p.packed ? 1 : cir / CL_KC;
  p.kchunks = p.packed ? 1 : 9 * p.cb;
  p.stage_bytes = (Co * (CL_KC + MT<T>::PAD) * (int)sizeof(T) + 1023) / 1024 * 1024;
  const int ybuf = F * (Co + 4) * (int)sizeof(float);
  int tf = CL_ROWS / F;
  if (tf > CL_TFMAX) tf = CL_TFMAX;
  for (; tf >= 1; --tf) {
    p.slab_bytes = ((tf + 2) * (F + 2) * p.cip * (int)sizeof(T) + 15) / 16 * 16;
    const int main_bytes = p.slab_bytes + 2 * p.stage_bytes;
    p.lds_bytes = (main_bytes > ybuf ? main_bytes : ybuf) + CL_SMALL;
    if (p.lds_bytes <= CL_LDS) break;
  }
  p.tf = tf;
  return tf >= 1;
}

// sum over the 16 lanes of a DPP row (one row of a 16x16 MFMA tile's columns)
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f32<0x140>(v);
  v += dpp_f32<0x141>(v);
  v += dpp_f32<0x4E>(v);
  v += dpp_f32<0xB1>(v);
  return v;
}

__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return i < 0 ? 0 : (i >= n ? n - 1 : i);  // rows past the halo of a ragged last workgroup: any valid row
}

template <typename T>
__device__ __forceinline__ void store4(T* p, float a, float b, float c, float d);
template <>
__device__ __forceinline__ void store4<float>(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
template <>
__device__ __forceinline__ void store4<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
}

// The weight image: chunk j = tap * cb + block (tap = 3 kt + kf) holds rows
// co of 32 k (channels 32 block .. + 31 of the tap, zero past Ci) + pad; with
// 9 Ci <= 32 the one chunk's k is tap * Ci + ci.  w (Co, Ci, kF, kT) fp32.
template <typename T>
__global__ void cl_image_kernel(const float* __restrict__ w, int Ci, int Co, int packed, int cb, int kchunks,
                                int stage_elems, T* __restrict__ img) {
  const long long n = (long long)kchunks * stage_elems;
  constexpr int LD = CL_KC + MT<T>::PAD;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i / stage_elems), r = (int)(i - (long long)j * stage_elems);
    const int co = r / LD, kk = r - co * LD;
    float v = 0.f;
    if (co < Co && kk < CL_KC) {
      int tap, ci;
      if (packed) {
        tap = kk / Ci;
        ci = kk - tap * Ci;
      } else {
        tap = j / cb;
        ci = (j - tap * cb) * CL_KC + kk;
      }
      if (tap < 9 && ci < Ci) {
        const int kt = tap / 3, kf = tap - 3 * kt;
        v = w[(((long long)co * Ci + ci) * 3 + kf) * 3 + kt];
      }
    }
    img[i] = MT<T>::from_f32(v);
  }
}

struct ClArgs {
  const void* x;
  const void* img;
  const float* bias;
  const float* gamma;
  const float* beta;
  const float* scale;
  void* y;
  void* c;
  float* mean;
  float* rstd;
  int B, T, F, Ci, Co, pool;
  float eps, slope;
  int tf, packed, cip, cb, kchunks, stage_bytes, slab_bytes, main_bytes, vec;
};

template <typename T>
__global__ __launch_bounds__(CL_THREADS) void conv_ln_kernel(const ClArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using M = MT<T>;
  constexpr int LDW = CL_KC + M::PAD;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the DMA's LDS address is a scalar
  const int F = a.F, Ci = a.Ci, Co = a.Co, T_ = a.T, cip = a.cip, F2 = F + 2;
  const int b = blockIdx.y, t0 = blockIdx.x * a.tf;
  const int rows = a.tf * F, mtiles = (rows + 15) >> 4;
  const int ntv = (Co / 16 - w + CL_WAVES - 1) / CL_WAVES;  // this wave's column tiles: nt * 4 + w
  T* slab = reinterpret_cast<T*>(smem);
  char* ring = smem + a.slab_bytes;
  float* ybuf = reinterpret_cast<float*>(smem);  // the frame tile of the epilogue, over slab and ring
  float* rs = reinterpret_cast<float*>(smem + a.main_bytes);
  float* stat = rs + CL_WAVES * CL_ROWS;  // [0, TFMAX): mean, [TFMAX, 2 TFMAX): rstd
  const T* x = static_cast<const T*>(a.x);
  const char* img = static_cast<const char*>(a.img);
  const int pieces = a.stage_bytes >> 10;

  auto issue = [&](int j) {
    const uint32_t la = lds_addr(ring + (j & 1) * a.stage_bytes);
    for (int pc = w; pc < pieces; pc += CL_WAVES)
      lds_dma16(img + (size_t)j * a.stage_bytes + (pc << 10) + (lane << 4),
                __builtin_amdgcn_readfirstlane(la + (pc << 10)));
  };
  issue(0);

  // the slab: frame t0 - 1 + tt, bin ff - 1, reflected
  const int srows = (a.tf + 2) * F2;
  if (a.vec) {
    constexpr int V = M::VEC;
    const int cpv = cip / V;
    for (int i = tid; i < srows * cpv; i += CL_THREADS) {
      const int r = i / cpv, cv = (i - r * cpv) * V;
      const int tt = r / F2, ff = r - tt * F2;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (cv < Ci)
        v = *reinterpret_cast<const uint4*>(
            x + (((size_t)b * T_ + reflect(t0 - 1 + tt, T_)) * F + reflect(ff - 1, F)) * Ci + cv);
      *reinterpret_cast<uint4*>(slab + (size_t)r * cip + cv) = v;
    }
  } else {
    for (int i = tid; i < srows * cip; i += CL_THREADS) {
      const int r = i / cip, ci = i - r * cip;
      const int tt = r / F2, ff = r - tt * F2;
      T v = M::from_f32(0.f);
      if (ci < Ci) v = x[(((size_t)b * T_ + reflect(t0 - 1 + tt, T_)) * F + reflect(ff - 1, F)) * Ci + ci];
      slab[(size_t)r * cip + ci] = v;
    }
  }

  // slab offset of this lane's A row in every row tile (rows past the last: the last)
  int base[CL_MT];
#pragma unroll
  for (int mi = 0; mi < CL_MT; ++mi) {
    int r = mi * 16 + l16;
    r = r < rows ? r : rows - 1;
    const int t = r / F;
    base[mi] = (t * F2 + (r - t * F)) * cip;
  }

  f32x4 acc[CL_MT][CL_NT];
#pragma unroll
  for (int mi = 0; mi < CL_MT; ++mi)
#pragma unroll
    for (int nt = 0; nt < CL_NT; ++nt) acc[mi][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  if (a.packed) {
    // k = 8 g + i = tap * Ci + ci: the slab offset of each of this lane's 8 k
    int koff[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = 8 * g + i, tap = k / Ci, kt = tap / 3;
      koff[i] = k < 9 * Ci ? (kt * F2 + (tap - 3 * kt)) * cip + (k - tap * Ci) : -1;
    }
    const T* wst = reinterpret_cast<const T*>(ring);
    typename M::frag bw[CL_NT];
#pragma unroll
    for (int nt = 0; nt < CL_NT; ++nt)
      bw[nt] = nt < ntv ? M::load(wst + ((nt * CL_WAVES + w) * 16 + l16) * LDW + 8 * g) : M::zero();
#pragma unroll
    for (int mi = 0; mi < CL_MT; ++mi) {
      if (mi < mtiles) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = koff[i] >= 0 ? M::to_f32(slab[base[mi] + koff[i]]) : 0.f;
        const typename M::frag av = M::from8(v);
#pragma unroll
        for (int nt = 0; nt < CL_NT; ++nt)
          if (nt < ntv) M::mma(acc[mi][nt], av, bw[nt]);
      }
    }
  } else {
    int tap = 0, blk = 0;
    for (int j = 0; j < a.kchunks; ++j) {
      if (j + 1 < a.kchunks) issue(j + 1);  // into the stage read at j - 1: free since that step's barrier
      const T* wst = reinterpret_cast<const T*>(ring + (j & 1) * a.stage_bytes);
      const int kt = tap / 3, kf = tap - 3 * kt;
      const int aoff = (kt * F2 + kf) * cip + blk * CL_KC + 8 * g;
      typename M::frag bw[CL_NT];
#pragma unroll
      for (int nt = 0; nt < CL_NT; ++nt)
        bw[nt] = nt < ntv ? M::load(wst + ((nt * CL_WAVES + w) * 16 + l16) * LDW + 8 * g) : M::zero();
#pragma unroll
      for (int mi = 0; mi < CL_MT; ++mi) {
        if (mi < mtiles) {
          const typename M::frag av = M::load(slab + base[mi] + aoff);
#pragma unroll
          for (int nt = 0; nt < CL_NT; ++nt)
            if (nt < ntv) M::mma(acc[mi][nt], av, bw[nt]);
        }
      }
      if (++blk == a.cb) {
        blk = 0;
        ++tap;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // chunk j + 1 landed
      __syncthreads();                                   // and every wave is done with chunk j
    }
  }
  __syncthreads();  // slab and ring are free: the frame tile lies over them

  // ---- epilogue.  Lane: rows 4 g + reg of each row tile, column l16 of its column tiles
  const int tfv = T_ - t0 < a.tf ? T_ - t0 : a.tf;  // frames of this workgroup inside the utterance
  const int vrows = tfv * F;
  T* cg = static_cast<T*>(a.c);
#pragma unroll
  for (int nt = 0; nt < CL_NT; ++nt) {
    if (nt < ntv) {
      const int co = (nt * CL_WAVES + w) * 16 + l16;
      const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
      for (int mi = 0; mi < CL_MT; ++mi) {
        if (mi < mtiles) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int r = mi * 16 + 4 * g + reg;
            acc[mi][nt][reg] += bv;
            if (cg && r < vrows) cg[(((size_t)b * T_ + t0) * F + r) * Co + co] = M::from_f32(acc[mi][nt][reg]);
          }
        }
      }
    }
  }

  const float inv_d = 1.f / (float)(F * Co);
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    // pass 0: sums -> mean, rows centred in place; pass 1: centred squares -> rstd
#pragma unroll
    for (int mi = 0; mi < CL_MT; ++mi) {
      if (mi < mtiles) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          float s = 0.f;
#pragma unroll
          for (int nt = 0; nt < CL_NT; ++nt)
            if (nt < ntv) s += pass ? acc[mi][nt][reg] * acc[mi][nt][reg] : acc[mi][nt][reg];
          s = row16_sum(s);
          if (l16 == 0) rs[w * CL_ROWS + mi * 16 + 4 * g + reg] = s;
        }
      }
    }
    __syncthreads();
    for (int tf = w; tf < a.tf; tf += CL_WAVES) {
      float s = 0.f;
      for (int i = lane; i < CL_WAVES * F; i += 64) s += rs[(i & 3) * CL_ROWS + tf * F + (i >> 2)];
      s = wave_sum(s) * inv_d;
      if (lane == 0) stat[pass * CL_TFMAX + tf] = pass ? rsqrtf(s + a.eps) : s;
    }
    __syncthreads();
    if (pass == 0) {
      for (int tf = 0; tf < a.tf; ++tf) {
        const float m = stat[tf];
        const int lo = tf * F, hi = lo + F;
#pragma unroll
        for (int mi = 0; mi < CL_MT; ++mi) {
          if (mi < mtiles && mi * 16 < hi && mi * 16 + 16 > lo) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int r = mi * 16 + 4 * g + reg;
              if (r >= lo && r < hi) {
#pragma unroll
                for (int nt = 0; nt < CL_NT; ++nt) acc[mi][nt][reg] -= m;
              }
            }
          }
        }
      }
    }
  }
  if (a.mean && tid < tfv) {
    a.mean[(size_t)b * T_ + t0 + tid] = stat[tid];
    a.rstd[(size_t)b * T_ + t0 + tid] = stat[CL_TFMAX + tid];
  }

  const int p = a.pool, Fo = F / p, ldy = Co + 4, co4 = Co >> 2;
  T* yg = static_cast<T*>(a.y);
  for (int tf = 0; tf < tfv; ++tf) {
    const float rstd = stat[CL_TFMAX + tf];
    const int lo = tf * F, hi = lo + F;
#pragma unroll
    for (int mi = 0; mi < CL_MT; ++mi) {
      if (mi < mtiles && mi * 16 < hi && mi * 16 + 16 > lo) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int r = mi * 16 + 4 * g + reg;
          if (r >= lo && r < hi) {
#pragma unroll
            for (int nt = 0; nt < CL_NT; ++nt)
              if (nt < ntv) ybuf[(r - lo) * ldy + (nt * CL_WAVES + w) * 16 + l16] = acc[mi][nt][reg] * rstd;
          }
        }
      }
    }
    __syncthreads();
    T* yrow = yg + ((size_t)b * T_ + t0 + tf) * Fo * Co;
    for (int i = tid; i < Fo * co4; i += CL_THREADS) {
      const int fo = i / co4, c4 = (i - fo * co4) * 4;
      float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      for (int j = 0; j < p; ++j) {
        const int f = fo * p + j;
        const float4 n = *reinterpret_cast<const float4*>(ybuf + f * ldy + c4);
        const float4 gm = *reinterpret_cast<const float4*>(a.gamma + f * Co + c4);
        const float4 bt = *reinterpret_cast<const float4*>(a.beta + f * Co + c4);
        const float v[4] = {n.x * gm.x + bt.x, n.y * gm.y + bt.y, n.z * gm.z + bt.z, n.w * gm.w + bt.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) best[q] = fmaxf(best[q], v[q] > 0.f ? v[q] : v[q] * a.slope);
      }
      const float sc = a.scale ? a.scale[b * Fo + fo] : 1.f;
      store4<T>(yrow + fo * Co + c4, best[0] * sc, best[1] * sc, best[2] * sc, best[3] * sc);
    }
    __syncthreads();
  }
}

struct ClBwdArgs {
  const void* dy;
  const void* c;
  const float* mean;
  const float* rstd;
  const float* gamma;
  const float* beta;
  const float* scale;
  void* dc;
  float* part;
  int rows, T, F, Co, pool;
  float slope;
};

// the pool window of output element (fo, co) of one frame: the first maximum
// j, its normalised value n and dL/d(activation input) per unit of dy
template <typename T>
__device__ __forceinline__ void cl_window(const ClBwdArgs& a, const T* crow, float m, float r, int fo, int co, int& jm,
                                          float& nm, float& dact) {
  float best = -INFINITY;
  jm = 0;
  nm = 0.f;
  dact = a.slope;
  for (int j = 0; j < a.pool; ++j) {
    const int e = (fo * a.pool + j) * a.Co + co;
    const float n = (MT<T>::to_f32(crow[e]) - m) * r;
    const float v = n * a.gamma[e] + a.beta[e];
    const float act = v > 0.f ? v : v * a.slope;
    if (act > best) {
      best = act;
      jm = j;
      nm = n;
      dact = v > 0.f ? 1.f : a.slope;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(CL_BWD_THREADS) void conv_ln_bwd_kernel(const ClBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using M = MT<T>;
  const int tid = threadIdx.x;
  const int F = a.F, Co = a.Co, p = a.pool, Fo = F / p, D = F * Co, Do = Fo * Co;
  float* gsum = reinterpret_cast<float*>(smem);
  float* bsum = gsum + D;
  float* red = bsum + D;
  for (int e = tid; e < 2 * D; e += CL_BWD_THREADS) gsum[e] = 0.f;
  __syncthreads();
  const float inv_d = 1.f / (float)D;
  for (int row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const T* crow = static_cast<const T*>(a.c) + (size_t)row * D;
    const T* dyrow = static_cast<const T*>(a.dy) + (size_t)row * Do;
    T* dcrow = static_cast<T*>(a.dc) + (size_t)row * D;
    const float* sc = a.scale ? a.scale + (size_t)(row / a.T) * Fo : nullptr;
    const float m = a.mean[row], r = a.rstd[row];
    float s1 = 0.f, s2 = 0.f;
    // output element q = (fo, co) and its window belong to thread q % 512 in every frame
    for (int q = tid; q < Do; q += CL_BWD_THREADS) {
      const int fo = q / Co, co = q - fo * Co;
      int jm;
      float nm, dact;
      cl_window<T>(a, crow, m, r, fo, co, jm, nm, dact);
      const float dn = M::to_f32(dyrow[q]) * (sc ? sc[fo] : 1.f) * dact;
      const int e = (fo * p + jm) * Co + co;
      gsum[e] += dn * nm;
      bsum[e] += dn;
      const float dh = dn * a.gamma[e];
      s1 += dh;
      s2 += dh * nm;
    }
    s1 = block_sum(s1, red) * inv_d;
    s2 = block_sum(s2, red) * inv_d;
    for (int q = tid; q < Do; q += CL_BWD_THREADS) {
      const int fo = q / Co, co = q - fo * Co;
      int jm;
      float nm, dact;
      cl_window<T>(a, crow, m, r, fo, co, jm, nm, dact);
      const int em = (fo * p + jm) * Co + co;
      const float dh = M::to_f32(dyrow[q]) * (sc ? sc[fo] : 1.f) * dact * a.gamma[em];
      for (int j = 0; j < p; ++j) {
        const int e = (fo * p + j) * Co + co;
        const float n = j == jm ? nm : (M::to_f32(crow[e]) - m) * r;
        dcrow[e] = M::from_f32(r * ((j == jm ? dh : 0.f) - s1 - n * s2));
      }
    }
    // bins the floor-mode pool drops: no dy reaches them
    for (int e = Fo * p * Co + tid; e < D; e += CL_BWD_THREADS)
      dcrow[e] = M::from_f32(r * (-s1 - (M::to_f32(crow[e]) - m) * r * s2));
  }
  __syncthreads();
  float* part = a.part + (size_t)blockIdx.x * 2 * D;
  for (int e = tid; e < 2 * D; e += CL_BWD_THREADS) part[e] = gsum[e];
}

template <typename T>
int cl_launch(ClArgs& a, const ClPlan& p, hipStream_t s) {
  a.tf = p.tf;
  a.packed = p.packed;
  a.cip = p.cip;
  a.cb = p.cb;
  a.kchunks = p.kchunks;
  a.stage_bytes = p.stage_bytes;
  a.slab_bytes = p.slab_bytes;
  a.main_bytes = p.lds_bytes - CL_SMALL;
  a.vec = !p.packed && a.Ci % MT<T>::VEC == 0 && ((uintptr_t)a.x & 15) == 0;
  if (hipError_t e = lds_optin(reinterpret_cast<const void*>(&conv_ln_kernel<T>), p.lds_bytes)) return (int)e;
  conv_ln_kernel<T><<<dim3((a.T + p.tf - 1) / p.tf, a.B), CL_THREADS, p.lds_bytes, s>>>(a);
  SBK_CHECK_LAUNCH();
  return 0;
}

}  // namespace
}  // namespace sbk

using namespace sbk;

SBK_API int sbk_conv3x3_ln_frames(int bf16, int F, int Ci, int Co) {
  ClPlan p;
  const bool ok = bf16 ? cl_plan<bf16_t>(F, Ci, Co, p) : cl_plan<float>(F, Ci, Co, p);
  return ok ? p.tf : 0;
}

SBK_API long long sbk_conv3x3_ln_image_elems(int bf16, int Ci, int Co) {
  ClPlan p;
  const bool ok = bf16 ? cl_plan<bf16_t>(2, Ci, Co, p) : cl_plan<float>(2, Ci, Co, p);
  return ok ? (long long)p.kchunks * (p.stage_bytes / (bf16 ? 2 : 4)) : 0;
}

SBK_API int sbk_conv3x3_ln_image(int bf16, const float* w, int Ci, int Co, void* img, void* stream) {
  ClPlan p;
  const bool ok = bf16 ? cl_plan<bf16_t>(2, Ci, Co, p) : cl_plan<float>(2, Ci, Co, p);
  if (!ok || !w || !img) return SBK_ERR_ARG;
  const int se = p.stage_bytes / (bf16 ? 2 : 4);
  const long long n = (long long)p.kchunks * se;
  const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipStream_t s = (hipStream_t)stream;
  if (bf16)
    cl_image_kernel<bf16_t><<<grid, 256, 0, s>>>(w, Ci, Co, p.packed, p.cb, p.kchunks, se, static_cast<bf16_t*>(img));
  else
    cl_image_kernel<float><<<grid, 256, 0, s>>>(w, Ci, Co, p.packed, p.cb, p.kchunks, se, static_cast<float*>(img));
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_conv3x3_ln(int bf16, const void* x, int B, int T, int F, int Ci, int Co, const void* img,
                           const float* bias, const float* gamma, const float* beta, float eps, float slope, int pool,
                           const float* scale, void* y, void* c, float* mean, float* rstd, void* stream) {
  ClPlan p;
  const bool ok = bf16 ? cl_plan<bf16_t>(F, Ci, Co, p) : cl_plan<float>(F, Ci, Co, p);
  if (!ok || B < 1 || B > 65535 || T < 2 || pool < 1 || pool > F || !x || !img || !gamma || !beta || !y)
    return SBK_ERR_ARG;
  if ((c != nullptr) != (mean != nullptr) || (c != nullptr) != (rstd != nullptr)) return SBK_ERR_ARG;
  ClArgs a{x, img, bias, gamma, beta, scale, y, c, mean, rstd, B, T, F, Ci, Co, pool, eps, slope};
  return bf16 ? cl_launch<bf16_t>(a, p, (hipStream_t)stream) : cl_launch<float>(a, p, (hipStream_t)stream);
}

SBK_API int sbk_conv3x3_ln_bwd_blocks(int rows) { return rows < 256 ? (rows > 0 ? rows : 1) : 256; }

SBK_API int sbk_conv3x3_ln_bwd(int bf16, const void* dy, const void* c, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, const float* scale, int B, int T, int F, int Co,
                               int pool, float slope, void* dc, float* part, void* stream) {
  if (B < 1 || T < 1 || F < 1 || Co < 1 || (long long)F * Co > CL_DMAX || pool < 1 || pool > F ||
      (long long)B * T > 0x7fffffffLL || !dy || !c || !mean || !rstd || !gamma || !beta || !dc || !part)
    return SBK_ERR_ARG;
  ClBwdArgs a{dy, c, mean, rstd, gamma, beta, scale, dc, part, B * T, T, F, Co, pool, slope};
  const size_t lds = ((size_t)2 * F * Co + 16) * sizeof(float);
  const int grid = sbk_conv3x3_ln_bwd_blocks(a.rows);
  hipStream_t s = (hipStream_t)stream;
  if (bf16) {
    if (hipError_t e = lds_optin(reinterpret_cast<const void*>(&conv_ln_bwd_kernel<bf16_t>), lds)) return (int)e;
    conv_ln_bwd_kernel<bf16_t><<<grid, CL_BWD_THREADS, lds, s>>>(a);
  } else {
    if (hipError_t e = lds_optin(reinterpret_cast<const void*>(&conv_ln_bwd_kernel<float>), lds)) return (int)e;
    conv_ln_bwd_kernel<float><<<grid, CL_BWD_THREADS, lds, s>>>(a);
  }
  SBK_CHECK_LAUNCH();
  return 0;
}
