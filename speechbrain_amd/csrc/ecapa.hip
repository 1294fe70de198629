// The eval forward of the ECAPA-TDNN lobe (lobes/models/ECAPA_TDNN.py), time
// major: activations are (N, L, C) with C contiguous, read and written
// through a row stride so that a layer can work on a channel range of a wider
// buffer (a Res2Net chunk, a block's slot of the MFA concatenation).
//
// tdnn_kernel — one TDNN layer, Conv1d "same" reflect -> act -> eval
// BatchNorm (a per-channel scale and shift) [-> tanh], as an implicit GEMM.
// A workgroup of four waves owns TD_TT frames of one utterance and up to 256
// output channels: M = 64 rows, N = 256 columns, K = k * Ci.  The input slab
// (TD_TT + (k - 1) d rows, reflected over the utterance's L frames as it is
// staged, an optional addend summed in — the Res2Net step's x_i + y_{i-1})
// lies in LDS in channel blocks of 512 bytes a row; tap j of the A operand is
// the same slab read j d rows further down.  The weight, laid out (k, Co,
// Ci padded to 32) on the host, streams through an LDS ring of two K-chunks
// of 32: chunk q + 1 is fetched into registers before the MFMAs of chunk q
// and stored to the other stage after them.  Wave w holds column tiles w,
// w + 4, ... of the four row tiles: sixteen accumulators, a weight fragment
// used four times.  Epilogue from the fp32 accumulators: bias (per channel or
// per utterance), LeakyReLU(slope) (slope 0: ReLU, slope 1: none), affine,
// tanh, the store, and the column sums of the frames below the utterance's
// valid count, one (N, tiles, Co) partial per workgroup — every element has
// one owner lane, no atomics.
//
// se_gate_kernel / se_apply_kernel — the squeeze-excitation block from those
// partials: s = sigmoid(W2 relu(W1 m + b1) + b2), out = s x + residual.
//
// asp_stats_kernel / asp_pool_kernel — attentive statistics pooling without
// the (N, 3C, L) concatenation or the (N, C, L) attention tensor: the masked
// mean and deviation per (n, c); then, per utterance and 64 channels, frame
// tiles of 16: logits = h W_c^T + b_c by MFMA, an online softmax over time
// per channel, and running sums of p, p (x - mu), p (x - mu)^2 about the
// global mean mu as pivot, so that a channel constant over time pools to a
// variance of 0 (the reference's clamp: std = 1e-6) and not to the
// cancellation error of E[x^2] - mean^2.
#include "mfma.h"
#include "sbk_common.h"

namespace sbk {
namespace {

constexpr int TD_THREADS = 256;
constexpr int TD_WAVES = 4;
constexpr int TD_TT = 64;         // frames of a workgroup
constexpr int TD_MT = TD_TT / 16;
constexpr int TD_NT = 4;          // column tiles of a wave
constexpr int TD_COB = 16 * TD_NT * TD_WAVES;  // output channels of a workgroup
constexpr int TD_KC = 32;         // K of a ring stage
constexpr int TD_HALO = 32;       // (k - 1) d at most
constexpr int TD_KB_BYTES = 512;  // slab channel block, bytes per row

__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return i < 0 ? 0 : (i >= n ? n - 1 : i);  // rows past the halo of a ragged last tile: any valid row
}

template <typename T>
struct alignas(16) Vec {
  T e[MT<T>::VEC];
};

struct TdArgs {
  const void* x;
  const void* add;
  const void* wp;
  const float* bias;
  const float* scale;
  const float* shift;
  const int* valid;
  void* out;
  float* part;
  long long ldx, ldadd, ldo;
  int N, L, Ci, Co, k, d, cipad, bias_per_utt, tanh_, vec;
  float slope;
};

template <typename T>
__global__ __launch_bounds__(TD_THREADS) void tdnn_kernel(const TdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using M = MT<T>;
  constexpr int V = M::VEC;
  constexpr int KB = TD_KB_BYTES / (int)sizeof(T);  // channels of a slab block
  constexpr int LDS_ = KB + M::PAD;                 // slab row stride
  constexpr int LDW = TD_KC + M::PAD;               // ring row stride
  constexpr int PPR = TD_KC / V;                    // 16-byte pieces of a ring row
  constexpr int MAXP = TD_COB * PPR / TD_THREADS;   // pieces of a thread
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15, w = tid >> 6;
  const int L = a.L, Ci = a.Ci, Co = a.Co, d = a.d;
  const int n = blockIdx.y, t0 = blockIdx.x * TD_TT, co0 = blockIdx.z * TD_COB;
  const int cob = Co - co0 < TD_COB ? Co - co0 : TD_COB;
  const int ntv = ((cob + 15) / 16 - w + TD_WAVES - 1) / TD_WAVES;  // a last half tile (Co a multiple of 8) included
  const int pad = (a.k - 1) / 2 * d;
  const int rows = L - t0 < TD_TT ? L - t0 : TD_TT;
  const int mtiles = (rows + 15) >> 4;
  const int srows = TD_TT + 2 * pad;
  T* slab = reinterpret_cast<T*>(smem);
  T* ring = slab + (TD_TT + TD_HALO) * LDS_;
  const T* x = static_cast<const T*>(a.x) + (size_t)n * L * a.ldx;
  const T* ad = a.add ? static_cast<const T*>(a.add) + (size_t)n * L * a.ldadd : nullptr;
  const T* wp = static_cast<const T*>(a.wp);

  const int npieces = cob * PPR;
  const int kblocks = (a.cipad + KB - 1) / KB;
  Vec<T> wreg[MAXP];
  // chunk (kb, tap, blk): weight rows co0 .., channels kb KB + 32 blk .. + 31 of tap
  auto fetch = [&](int kb, int tap, int blk) {
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int pc = tid + i * TD_THREADS;
      if (pc < npieces) {
        const int r = pc / PPR, p = pc - r * PPR;
        wreg[i] = *reinterpret_cast<const Vec<T>*>(wp + ((size_t)tap * Co + co0 + r) * a.cipad + kb * KB + blk * TD_KC +
                                                   p * V);
      }
    }
  };
  auto stash = [&](int stage) {
    T* st = ring + stage * TD_COB * LDW;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int pc = tid + i * TD_THREADS;
      if (pc < npieces) {
        const int r = pc / PPR, p = pc - r * PPR;
        *reinterpret_cast<Vec<T>*>(st + r * LDW + p * V) = wreg[i];
      }
    }
  };

  f32x4 acc[TD_MT][TD_NT];
#pragma unroll
  for (int mi = 0; mi < TD_MT; ++mi)
#pragma unroll
    for (int nt = 0; nt < TD_NT; ++nt) acc[mi][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0, 0, 0);
  stash(0);
  int q = 0;
  for (int kb = 0; kb < kblocks; ++kb) {
    const int kc0 = kb * KB;
    const int kw = a.cipad - kc0 < KB ? a.cipad - kc0 : KB;  // channels of this block, a multiple of 32
    // the slab block: row s is frame t0 - pad + s reflected, zero past Ci
    if (a.vec) {
      const int cpv = kw / V;
      for (int i = tid; i < srows * cpv; i += TD_THREADS) {
        const int s = i / cpv, cv = (i - s * cpv) * V;
        const size_t t = (size_t)reflect(t0 - pad + s, L);
        Vec<T> v;
        if (kc0 + cv < Ci) {
          v = *reinterpret_cast<const Vec<T>*>(x + t * a.ldx + kc0 + cv);
          if (ad) {
            const Vec<T> u = *reinterpret_cast<const Vec<T>*>(ad + t * a.ldadd + kc0 + cv);
#pragma unroll
            for (int e = 0; e < V; ++e) v.e[e] = M::from_f32(M::to_f32(v.e[e]) + M::to_f32(u.e[e]));
          }
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) v.e[e] = M::from_f32(0.f);
        }
        *reinterpret_cast<Vec<T>*>(slab + s * LDS_ + cv) = v;
      }
    } else {
      for (int i = tid; i < srows * kw; i += TD_THREADS) {
        const int s = i / kw, c = i - s * kw;
        const size_t t = (size_t)reflect(t0 - pad + s, L);
        float v = 0.f;
        if (kc0 + c < Ci) {
          v = M::to_f32(x[t * a.ldx + kc0 + c]);
          if (ad) v += M::to_f32(ad[t * a.ldadd + kc0 + c]);
        }
        slab[s * LDS_ + c] = M::from_f32(v);
      }
    }
    __syncthreads();  // the slab block and the stage of chunk q
    const int bpt = kw / TD_KC;
    for (int tap = 0; tap < a.k; ++tap) {
      for (int blk = 0; blk < bpt; ++blk, ++q) {
        // the chunk after this one, in the order (kb, tap, blk)
        int nb = blk + 1, ntap = tap, nkb = kb;
        if (nb == bpt) {
          nb = 0;
          if (++ntap == a.k) {
            ntap = 0;
            ++nkb;
          }
        }
        const bool more = nkb < kblocks;
        if (more) fetch(nkb, ntap, nb);
        const T* wst = ring + (q & 1) * TD_COB * LDW;
        typename M::frag bw[TD_NT];
#pragma unroll
        for (int nt = 0; nt < TD_NT; ++nt)
          bw[nt] = nt < ntv ? M::load(wst + ((nt * TD_WAVES + w) * 16 + l16) * LDW + 8 * g) : M::zero();
#pragma unroll
        for (int mi = 0; mi < TD_MT; ++mi) {
          if (mi < mtiles) {
            const typename M::frag av = M::load(slab + (mi * 16 + l16 + tap * d) * LDS_ + blk * TD_KC + 8 * g);
#pragma unroll
            for (int nt = 0; nt < TD_NT; ++nt)
              if (nt < ntv) M::mma(acc[mi][nt], av, bw[nt]);
          }
        }
        if (more) stash((q + 1) & 1);  // read last at chunk q - 1, before that chunk's barrier
        __syncthreads();
      }
    }
  }

  // ---- epilogue.  Lane: rows 4 g + reg of each row tile, column l16 of its column tiles
  const int cnt = a.valid ? a.valid[n] : L;
  const int tiles = gridDim.x;
  T* out = static_cast<T*>(a.out) + ((size_t)n * L + t0) * a.ldo;
#pragma unroll
  for (int nt = 0; nt < TD_NT; ++nt) {
    if (nt < ntv) {
      const int co = co0 + (nt * TD_WAVES + w) * 16 + l16;
      const bool live = co < Co;  // the upper half of a last half tile holds whatever the ring held: never stored
      const int cc = live ? co : Co - 1;
      const float bv = a.bias ? a.bias[(a.bias_per_utt ? (size_t)n * Co : 0) + cc] : 0.f;
      const float sc = a.scale ? a.scale[cc] : 1.f, sh = a.shift ? a.shift[cc] : 0.f;
      float cs = 0.f;
#pragma unroll
      for (int mi = 0; mi < TD_MT; ++mi) {
        if (mi < mtiles) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int r = mi * 16 + 4 * g + reg;
            float v = acc[mi][nt][reg] + bv;
            v = v > 0.f ? v : v * a.slope;
            v = v * sc + sh;
            if (a.tanh_) v = tanhf(v);
            if (r < rows && live) {
              out[(size_t)r * a.ldo + co] = M::from_f32(v);
              if (t0 + r < cnt) cs += v;
            }
          }
        }
      }
      if (a.part) {
        cs = col4_sum(cs);
        if (g == 0 && live) a.part[((size_t)n * tiles + blockIdx.x) * Co + co] = cs;
      }
    }
  }
}

template <typename T>
int td_launch(const TdArgs& a, hipStream_t s) {
  using M = MT<T>;
  constexpr int KB = TD_KB_BYTES / (int)sizeof(T);
  const size_t lds =
      ((size_t)(TD_TT + TD_HALO) * (KB + M::PAD) + 2 * (size_t)TD_COB * (TD_KC + M::PAD)) * sizeof(T);
  if (hipError_t e = lds_optin(reinterpret_cast<const void*>(&tdnn_kernel<T>), lds)) return (int)e;
  const dim3 grid((a.L + TD_TT - 1) / TD_TT, a.N, (a.Co + TD_COB - 1) / TD_COB);
  tdnn_kernel<T><<<grid, TD_THREADS, lds, s>>>(a);
  SBK_CHECK_LAUNCH();
  return 0;
}

// ---- squeeze-excitation
constexpr int SE_THREADS = 256;

__global__ __launch_bounds__(SE_THREADS) void se_gate_kernel(const float* __restrict__ part, int tiles,
                                                             const int* __restrict__ valid, int L, int C, int S,
                                                             const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2,
                                                             float* __restrict__ s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* m = reinterpret_cast<float*>(smem);
  float* h = m + C;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float cnt = (float)(valid ? valid[n] : L);
  for (int c = tid; c < C; c += SE_THREADS) {
    float v = 0.f;
    for (int t = 0; t < tiles; ++t) v += part[((size_t)n * tiles + t) * C + c];
    m[c] = v / cnt;
  }
  __syncthreads();
  for (int j = w; j < S; j += SE_THREADS / 64) {
    float v = 0.f;
    for (int c = lane; c < C; c += 64) v += w1[(size_t)j * C + c] * m[c];
    v = wave_sum(v);
    if (lane == 0) h[j] = fmaxf(v + (b1 ? b1[j] : 0.f), 0.f);
  }
  __syncthreads();
  for (int c = tid; c < C; c += SE_THREADS) {
    float v = b2 ? b2[c] : 0.f;
    for (int j = 0; j < S; ++j) v += w2[(size_t)c * S + j] * h[j];
    s[(size_t)n * C + c] = 1.f / (1.f + expf(-v));
  }
}

template <typename T>
__global__ void se_apply_kernel(const T* __restrict__ x, const float* __restrict__ s, const T* __restrict__ res,
                                long long ldr, T* __restrict__ out, long long ldo, int L, int C, long long total) {
  using M = MT<T>;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / C;
    const int c = (int)(i - row * C);
    const int n = (int)(row / L);
    out[row * ldo + c] = M::from_f32(s[(size_t)n * C + c] * M::to_f32(x[i]) + (res ? M::to_f32(res[row * ldr + c]) : 0.f));
  }
}

// ---- attentive statistics pooling
constexpr int AS_THREADS = 256;
constexpr int AS_CB = 64;  // channels of a workgroup

template <typename T>
__global__ __launch_bounds__(AS_THREADS) void asp_stats_kernel(const T* __restrict__ x, long long ldx,
                                                               const int* __restrict__ valid, int L, int C,
                                                               float* __restrict__ mean, float* __restrict__ sd) {
  __shared__ float red[AS_THREADS / AS_CB][AS_CB];
  using M = MT<T>;
  const int n = blockIdx.y, tid = threadIdx.x, cl = tid & (AS_CB - 1), rg = tid / AS_CB;
  const int c = blockIdx.x * AS_CB + cl;
  int cnt = valid ? valid[n] : L;
  cnt = cnt < L ? cnt : L;
  const T* xn = x + (size_t)n * L * ldx;
  float mu = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    float v = 0.f;
    if (c < C)
      for (int t = rg; t < cnt; t += AS_THREADS / AS_CB) {
        const float e = M::to_f32(xn[(size_t)t * ldx + c]) - mu;
        v += pass ? e * e : e;
      }
    __syncthreads();
    red[rg][cl] = v;
    __syncthreads();
    v = 0.f;
#pragma unroll
    for (int i = 0; i < AS_THREADS / AS_CB; ++i) v += red[i][cl];
    v /= (float)cnt;
    if (pass == 0) mu = v;
    else if (rg == 0 && c < C) {
      mean[(size_t)n * C + c] = mu;
      sd[(size_t)n * C + c] = sqrtf(fmaxf(v, 1e-12f));
    }
  }
}

template <typename T>
__global__ __launch_bounds__(AS_THREADS) void asp_pool_kernel(const T* __restrict__ h, const T* __restrict__ wc,
                                                              const float* __restrict__ bc, const T* __restrict__ x,
                                                              long long ldx, const float* __restrict__ mu,
                                                              const int* __restrict__ valid, int L, int A, int C,
                                                              float* __restrict__ out) {
  using M = MT<T>;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15, w = tid >> 6;
  const int n = blockIdx.y, c = blockIdx.x * AS_CB + w * 16 + l16;
  if (blockIdx.x * AS_CB + w * 16 >= C) return;  // C is a multiple of 16: whole waves leave
  int cnt = valid ? valid[n] : L;
  cnt = cnt < L ? cnt : L;
  const T* hn = h + (size_t)n * L * A;
  const T* xn = x + (size_t)n * L * ldx;
  const float pivot = mu[(size_t)n * C + c], bias = bc ? bc[c] : 0.f;
  const int ksteps = (A + 31) / 32;
  float mx = -INFINITY, s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int t0 = 0; t0 < cnt; t0 += 16) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int tr = t0 + l16 < cnt ? t0 + l16 : cnt - 1;  // the A row of this lane, inside the utterance
    for (int ks = 0; ks < ksteps; ++ks) {
      const int k = ks * 32 + 8 * g;
      typename M::frag av = M::zero(), bv = M::zero();
      if (k < A) {  // A is a multiple of 8
        av = M::load(hn + (size_t)tr * A + k);
        bv = M::load(wc + (size_t)c * A + k);
      }
      M::mma(acc, av, bv);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int t = t0 + 4 * g + reg;
      if (t < cnt) {
        const float lg = acc[reg] + bias;
        const float e = M::to_f32(xn[(size_t)t * ldx + c]) - pivot;
        const float nm = fmaxf(mx, lg);
        const float f = __expf(mx - nm), p = __expf(lg - nm);  // mx = -inf at the first frame: f = 0
        s0 = s0 * f + p;
        s1 = s1 * f + p * e;
        s2 = s2 * f + p * e * e;
        mx = nm;
      }
    }
  }
  // the four lanes of a channel
  const float gm = col4_max(mx);
  const float f = mx == -INFINITY ? 0.f : __expf(mx - gm);
  s0 = col4_sum(s0 * f);
  s1 = col4_sum(s1 * f);
  s2 = col4_sum(s2 * f);
  if (g == 0) {
    const float m1 = s1 / s0;
    out[(size_t)n * 2 * C + c] = pivot + m1;
    out[(size_t)n * 2 * C + C + c] = sqrtf(fmaxf(s2 / s0 - m1 * m1, 1e-12f));
  }
}


// ---- the whole Res2Net block in one launch.  A workgroup owns R2_TT frames
// of one utterance plus a halo of (scale - 1) h frames a side, h = d (k - 1)
// / 2.  One LDS buffer holds u_i by absolute frame: row s is frame fb + s,
// fb = t0 - (scale - 1) h, and only frames inside [0, L) are ever written.
// Step i reads tap j of output frame f at row refl(f + (j - (k - 1) / 2) d)
// - fb, the reflection over the utterance's L frames: at a sequence end the
// rows a step reads are u_i's own mirrored rows, never a recomputed halo, and
// a short utterance whose two mirrors overlap needs no special case.  The
// row tiles computed shrink by h a side per step.  After the K loop of step
// i the accumulators take bias, ReLU and the affine; y_i, rounded to the
// compute dtype, goes to channels [i w, (i + 1) w) of the tile's frames and
// u_{i+1} = x_{i+1} + y_i overwrites the buffer in place.  The step weights
// stream through a ring of two K-chunks of 32 as in tdnn_kernel.
constexpr int R2_TT = 64;
constexpr int R2_ROWS = 128;  // R2_TT + 2 (scale - 1) h at most
constexpr int R2_MT = R2_ROWS / 16;
constexpr int R2_NT = 2;      // column tiles of a wave: w <= 128
constexpr int R2_W = 16 * R2_NT * TD_WAVES;

struct R2Args {
  const void* x;
  const void* wp;
  const float* bias;
  const float* scale;
  const float* shift;
  void* out;
  long long ldx, ldo;
  int N, L, w, steps, k, d, cipad;
};

template <typename T>
__global__ __launch_bounds__(TD_THREADS) void res2net_kernel(const R2Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using M = MT<T>;
  constexpr int V = M::VEC;
  constexpr int LDW = TD_KC + M::PAD;
  constexpr int PPR = TD_KC / V;
  constexpr int MAXP = R2_W * PPR / TD_THREADS;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15, wv = tid >> 6;
  const int L = a.L, w = a.w, d = a.d, S = a.steps;
  const int n = blockIdx.y, t0 = blockIdx.x * R2_TT;
  const int h = (a.k - 1) / 2 * d, fb = t0 - S * h, R = R2_TT + 2 * S * h;
  const int ldu = a.cipad + M::PAD;
  const int ntv = ((w + 15) / 16 - wv + TD_WAVES - 1) / TD_WAVES;
  const int trows = L - t0 < R2_TT ? L - t0 : R2_TT;
  T* U = reinterpret_cast<T*>(smem);
  T* ring = U + R2_ROWS * ldu;
  const T* x = static_cast<const T*>(a.x) + (size_t)n * L * a.ldx;
  T* out = static_cast<T*>(a.out) + (size_t)n * L * a.ldo;
  const T* wp = static_cast<const T*>(a.wp);
  const int npieces = w * PPR, bpt = a.cipad / TD_KC, nchunks = a.k * bpt;

  // u_1 = x_1 over the frames inside the utterance, zero past w; chunk 0 copied through
  for (int i = tid; i < R * a.cipad; i += TD_THREADS) {
    const int s = i / a.cipad, c = i - s * a.cipad, f = fb + s;
    T v = M::from_f32(0.f);
    if (c < w && f >= 0 && f < L) v = x[(size_t)f * a.ldx + w + c];
    U[s * ldu + c] = v;
  }
  for (int i = tid; i < trows * w; i += TD_THREADS) {
    const int r = i / w, c = i - r * w;
    out[(size_t)(t0 + r) * a.ldo + c] = x[(size_t)(t0 + r) * a.ldx + c];
  }

  Vec<T> wreg[MAXP];
  for (int st = 1; st <= S; ++st) {
    const T* wst_g = wp + (size_t)(st - 1) * a.k * w * a.cipad;
    auto fetch = [&](int q) {
      const int tap = q / bpt, blk = q - tap * bpt;
#pragma unroll
      for (int i = 0; i < MAXP; ++i) {
        const int pc = tid + i * TD_THREADS;
        if (pc < npieces) {
          const int r = pc / PPR, p = pc - r * PPR;
          wreg[i] = *reinterpret_cast<const Vec<T>*>(wst_g + ((size_t)tap * w + r) * a.cipad + blk * TD_KC + p * V);
        }
      }
    };
    auto stash = [&](int stage) {
      T* sp = ring + stage * R2_W * LDW;
#pragma unroll
      for (int i = 0; i < MAXP; ++i) {
        const int pc = tid + i * TD_THREADS;
        if (pc < npieces) {
          const int r = pc / PPR, p = pc - r * PPR;
          *reinterpret_cast<Vec<T>*>(sp + r * LDW + p * V) = wreg[i];
        }
      }
    };
    // output rows of this step: [st h, R - st h), the row tiles that meet them
    const int mlo = (st * h) >> 4, mhi = (R - st * h + 15) >> 4;
    f32x4 acc[R2_MT][R2_NT];
#pragma unroll
    for (int mi = 0; mi < R2_MT; ++mi)
#pragma unroll
      for (int nt = 0; nt < R2_NT; ++nt) acc[mi][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    stash(0);
    __syncthreads();  // u_st and the first stage
    for (int q = 0; q < nchunks; ++q) {
      if (q + 1 < nchunks) fetch(q + 1);
      const int tap = q / bpt, blk = q - tap * bpt;
      const T* wst = ring + (q & 1) * R2_W * LDW;
      typename M::frag bw[R2_NT];
#pragma unroll
      for (int nt = 0; nt < R2_NT; ++nt)
        bw[nt] = nt < ntv ? M::load(wst + ((nt * TD_WAVES + wv) * 16 + l16) * LDW + 8 * g) : M::zero();
#pragma unroll
      for (int mi = 0; mi < R2_MT; ++mi) {
        if (mi >= mlo && mi < mhi) {
          int s = reflect(fb + mi * 16 + l16 + (tap - (a.k - 1) / 2) * d, L) - fb;  // u_st's own mirrored row
          s = s < 0 ? 0 : (s >= R2_ROWS ? R2_ROWS - 1 : s);                          // rows no output needs
          const typename M::frag av = M::load(U + s * ldu + blk * TD_KC + 8 * g);
#pragma unroll
          for (int nt = 0; nt < R2_NT; ++nt)
            if (nt < ntv) M::mma(acc[mi][nt], av, bw[nt]);
        }
      }
      if (q + 1 < nchunks) stash((q + 1) & 1);
      __syncthreads();  // after the last chunk: every wave is done with u_st
    }
    // y_st and u_{st + 1}
#pragma unroll
    for (int nt = 0; nt < R2_NT; ++nt) {
      if (nt < ntv) {
        const int co = (nt * TD_WAVES + wv) * 16 + l16;
        if (co < w) {
          const int pi = (st - 1) * w + co;
          const float bv = a.bias ? a.bias[pi] : 0.f, sc = a.scale[pi], sh = a.shift[pi];
#pragma unroll
          for (int mi = 0; mi < R2_MT; ++mi) {
            if (mi >= mlo && mi < mhi) {
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                const int s = mi * 16 + 4 * g + reg, f = fb + s;
                if (s < R && f >= 0 && f < L) {
                  const T yb = M::from_f32(fmaxf(acc[mi][nt][reg] + bv, 0.f) * sc + sh);
                  if (f >= t0 && f < t0 + trows) out[(size_t)f * a.ldo + st * w + co] = yb;
                  if (st < S)
                    U[s * ldu + co] = M::from_f32(M::to_f32(x[(size_t)f * a.ldx + (st + 1) * w + co]) + M::to_f32(yb));
                }
              }
            }
          }
        }
      }
    }
    // the next step's first barrier orders these writes before its reads
  }
}

template <typename T>
int r2_launch(const R2Args& a, hipStream_t s) {
  using M = MT<T>;
  const size_t lds = ((size_t)R2_ROWS * (a.cipad + M::PAD) + 2 * (size_t)R2_W * (TD_KC + M::PAD)) * sizeof(T);
  if (hipError_t e = lds_optin(reinterpret_cast<const void*>(&res2net_kernel<T>), lds)) return (int)e;
  res2net_kernel<T><<<dim3((a.L + R2_TT - 1) / R2_TT, a.N), TD_THREADS, lds, s>>>(a);
  SBK_CHECK_LAUNCH();
  return 0;
}

}  // namespace
}  // namespace sbk

using namespace sbk;

SBK_API int sbk_tdnn_tile(void) { return TD_TT; }

SBK_API int sbk_tdnn(int bf16, const void* x, long long ldx, const void* add, long long ldadd, int N, int L, int Ci,
                     int Co, int k, int d, const void* wp, int cipad, const float* bias, int bias_per_utt, float slope,
                     const float* scale, const float* shift, int tanh_, void* out, long long ldo, const int* valid,
                     float* part, void* stream) {
  if (N < 1 || N > 65535 || L < 1 || Ci < 1 || Co < 8 || Co % 8 || Co > 65535 * TD_COB || k < 1 || k > 5 ||
      !(k & 1) || d < 1 || (k - 1) * d > TD_HALO || (k - 1) / 2 * d >= L || cipad < Ci || cipad % TD_KC ||
      cipad >= Ci + TD_KC || ldx < Ci || ldo < Co || (add && ldadd < Ci) || !x || !wp || !out ||
      (long long)N * L > 0x7fffffffLL)
    return SBK_ERR_ARG;
  const int esz = bf16 ? 2 : 4, v = 16 / esz;
  if (((uintptr_t)wp & 15) || ((uintptr_t)x | (uintptr_t)out | (uintptr_t)add) % esz) return SBK_ERR_ARG;
  TdArgs a{x, add, wp, bias, scale, shift, valid, out, part, ldx, ldadd, ldo, N, L, Ci, Co, k, d, cipad,
           bias_per_utt, tanh_, 0, slope};
  a.vec = Ci % v == 0 && ldx % v == 0 && ((uintptr_t)x & 15) == 0 &&
          (!add || (ldadd % v == 0 && ((uintptr_t)add & 15) == 0));
  return bf16 ? td_launch<bf16_t>(a, (hipStream_t)stream) : td_launch<float>(a, (hipStream_t)stream);
}

SBK_API int sbk_se_gate(const float* part, int tiles, const int* valid, int N, int L, int C, int S, const float* w1,
                        const float* b1, const float* w2, const float* b2, float* s, void* stream) {
  if (N < 1 || L < 1 || tiles < 1 || C < 1 || S < 1 || (long long)(C + S) * 4 > 64 * 1024 || !part || !w1 || !w2 || !s)
    return SBK_ERR_ARG;
  se_gate_kernel<<<N, SE_THREADS, (size_t)(C + S) * sizeof(float), (hipStream_t)stream>>>(part, tiles, valid, L, C, S,
                                                                                          w1, b1, w2, b2, s);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_se_apply(int bf16, const void* x, const float* s, const void* res, long long ldr, void* out,
                         long long ldo, int N, int L, int C, void* stream) {
  if (N < 1 || L < 1 || C < 1 || (res && ldr < C) || ldo < C || !x || !s || !out) return SBK_ERR_ARG;
  const long long total = (long long)N * L * C;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    se_apply_kernel<bf16_t><<<grid, 256, 0, st>>>(static_cast<const bf16_t*>(x), s, static_cast<const bf16_t*>(res), ldr,
                                                  static_cast<bf16_t*>(out), ldo, L, C, total);
  else
    se_apply_kernel<float><<<grid, 256, 0, st>>>(static_cast<const float*>(x), s, static_cast<const float*>(res), ldr,
                                                 static_cast<float*>(out), ldo, L, C, total);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_asp_stats(int bf16, const void* x, long long ldx, const int* valid, int N, int L, int C, float* mean,
                          float* sd, void* stream) {
  if (N < 1 || N > 65535 || L < 1 || C < 1 || ldx < C || !x || !mean || !sd) return SBK_ERR_ARG;
  const dim3 grid((C + AS_CB - 1) / AS_CB, N);
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    asp_stats_kernel<bf16_t><<<grid, AS_THREADS, 0, st>>>(static_cast<const bf16_t*>(x), ldx, valid, L, C, mean, sd);
  else
    asp_stats_kernel<float><<<grid, AS_THREADS, 0, st>>>(static_cast<const float*>(x), ldx, valid, L, C, mean, sd);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_asp_pool(int bf16, const void* h, const void* wc, const float* bc, const void* x, long long ldx,
                         const float* mu, const int* valid, int N, int L, int A, int C, float* out, void* stream) {
  if (N < 1 || N > 65535 || L < 1 || A < 8 || A % 8 || C < 16 || C % 16 || ldx < C || !h || !wc || !x || !mu || !out)
    return SBK_ERR_ARG;
  if (((uintptr_t)h | (uintptr_t)wc) & 15) return SBK_ERR_ARG;
  const dim3 grid((C + AS_CB - 1) / AS_CB, N);
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    asp_pool_kernel<bf16_t><<<grid, AS_THREADS, 0, st>>>(static_cast<const bf16_t*>(h), static_cast<const bf16_t*>(wc),
                                                         bc, static_cast<const bf16_t*>(x), ldx, mu, valid, L, A, C, out);
  else
    asp_pool_kernel<float><<<grid, AS_THREADS, 0, st>>>(static_cast<const float*>(h), static_cast<const float*>(wc), bc,
                                                        static_cast<const float*>(x), ldx, mu, valid, L, A, C, out);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_res2net_supported(int w, int scale, int k, int d) {
  return w >= 8 && w % 8 == 0 && w <= R2_W && scale >= 2 && k >= 1 && k <= 5 && (k & 1) && d >= 1 &&
         R2_TT + 2 * (scale - 1) * ((k - 1) / 2 * d) <= R2_ROWS;
}

SBK_API int sbk_res2net(int bf16, const void* x, long long ldx, int N, int L, int w, int scale, int k, int d,
                        const void* wp, const float* bias, const float* aff_scale, const float* aff_shift, void* out,
                        long long ldo, void* stream) {
  if (!sbk_res2net_supported(w, scale, k, d) || N < 1 || N > 65535 || L < 1 || (k - 1) / 2 * d >= L ||
      ldx < (long long)w * scale || ldo < (long long)w * scale || !x || !wp || !aff_scale || !aff_shift || !out ||
      x == out || ((uintptr_t)wp & 15) || (long long)N * L > 0x7fffffffLL)
    return SBK_ERR_ARG;
  R2Args a{x, wp, bias, aff_scale, aff_shift, out, ldx, ldo, N, L, w, scale - 1, k, d, (w + TD_KC - 1) / TD_KC * TD_KC};
  return bf16 ? r2_launch<bf16_t>(a, (hipStream_t)stream) : r2_launch<float>(a, (hipStream_t)stream);
}
