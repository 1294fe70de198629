// Time-domain augmentation (processing/speech_augmentation.py:435-1173 and
// lobes/augment.py:204-299 of the reference): the polyphase resampler behind
// SpeedPerturb, DropFreq's 101-tap filter, DropChunk's segment fill, and the
// three fused into one launch for TimeDomainSpecAugment.
//
// Every kernel is built from the same device functions (rs_at, fir_window,
// seg_*), each with one fixed accumulation order written as explicit fmaf
// calls, so the fused kernel's output is bit-identical to the three kernels
// run one after another.  One workgroup of 256 threads owns kTile output
// elements of one batch row; its input span, the polyphase table, the taps and
// the row's segment table sit in LDS; global loads and stores are unit-stride
// across the workgroup.
#include "sbk_common.h"

using namespace sbk;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;                 // output elements per workgroup
constexpr int kPer = kTile / kThreads;      // outputs per thread
constexpr int kTaps = 101;
constexpr int kHalo = kTaps / 2;
constexpr int kFirN = kTile + 2 * kHalo;    // filter input of one tile
constexpr int kWMax = 2048;                 // polyphase weights held in LDS (L * W floats)
constexpr int kLMax = 128;                  // polyphase phases held in LDS
constexpr int kSpanMax = 4096;              // staged input floats of one tile
constexpr int kSegMax = 64;                 // segments per utterance
constexpr int kAmpChunks = 64;              // partial |x| sums per row

static_assert(kPer == 4, "fir_window reads its inputs as one float4 per four outputs");
static_assert(kFirN % 4 == 0, "the filter input is read as float4");

// the polyphase table in global memory: output n = k L + i reads
// x[first[i] + k M + j], j < W, against w[i][j]
struct RsTab {
  const int* first;
  const float* w;
  int L, M, W;
};

// table -> LDS; lo / hi: the smallest and largest first index (every thread)
__device__ __forceinline__ void rs_load(const RsTab& g, float* sw, int* sf, int& lo, int& hi) {
  for (int i = threadIdx.x; i < g.L * g.W; i += kThreads) sw[i] = g.w[i];
  for (int i = threadIdx.x; i < g.L; i += kThreads) sf[i] = g.first[i];
  __syncthreads();
  lo = hi = sf[0];
  for (int i = 1; i < g.L; ++i) {
    lo = min(lo, sf[i]);
    hi = max(hi, sf[i]);
  }
}

// the input samples [t_lo, t_lo + span) that outputs [na, nb) read
__device__ __forceinline__ void rs_span(const RsTab& g, int lo, int hi, int na, int nb, int& t_lo, long long& span) {
  t_lo = lo + (na / g.L) * g.M;
  span = (long long)hi + (long long)((nb - 1) / g.L) * g.M + g.W - t_lo;
}

// xr (T, C) -> sx[(t - t_lo) * C + c], zero outside [0, T)
__device__ __forceinline__ void rs_stage(const float* __restrict__ xr, int T, int C, int t_lo, int nflt, float* sx) {
  const long long off = (long long)t_lo * C;
  const long long end = (long long)T * C;
  for (int e = threadIdx.x; e < nflt; e += kThreads) {
    const long long g = off + e;
    sx[e] = (g >= 0 && g < end) ? xr[g] : 0.f;
  }
}

// output sample n of channel c: sum_j w[i][j] x[first[i] + k M + j], j ascending.
// STAGED: src is the LDS span starting at t_lo; otherwise the global row.
template <bool STAGED>
__device__ __forceinline__ float rs_at(const RsTab& g, const float* sw, const int* sf, const float* src, int n, int c,
                                       int C, int T, int t_lo) {
  const int i = n % g.L, k = n / g.L;
  const int base = sf[i] + k * g.M;
  const float* wr = sw + i * g.W;
  float acc = 0.f;
  for (int j = 0; j < g.W; ++j) {
    const int t = base + j;
    float xv;
    if (STAGED)
      xv = src[(t - t_lo) * C + c];
    else
      xv = (t >= 0 && t < T) ? src[(long long)t * C + c] : 0.f;
    acc = fmaf(wr[j], xv, acc);
  }
  return acc;
}

// y[t0 + r] = sum_k f[k] s[r + k], k ascending, for the thread's four
// consecutive outputs (s: this thread's 104-sample window of the LDS tile,
// read once as 26 float4 and kept in registers four at a time)
__device__ __forceinline__ void fir_window(const float* sr, const float* st, float acc[kPer]) {
  const float4* s4 = reinterpret_cast<const float4*>(sr) + threadIdx.x;
#pragma unroll
  for (int r = 0; r < kPer; ++r) acc[r] = 0.f;
#pragma unroll
  for (int q = 0; q < (kTaps + kPer - 1 + 3) / 4; ++q) {
    const float4 v = s4[q];
    const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
#pragma unroll
      for (int r = 0; r < kPer; ++r) {
        const int k = 4 * q + mm - r;
        if (k >= 0 && k < kTaps) acc[r] = fmaf(st[k], xs[mm], acc[r]);
      }
    }
  }
}

// filters the staged tile in place: sr[e] becomes output tile0 + e
__device__ __forceinline__ void fir_tile(float* sr, const float* st) {
  float acc[kPer];
  fir_window(sr, st, acc);
  __syncthreads();
  reinterpret_cast<float4*>(sr)[threadIdx.x] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  __syncthreads();
}

__device__ __forceinline__ void seg_load(const int* __restrict__ segs, int b, int S, int* ss) {
  for (int i = threadIdx.x; i < 2 * S; i += kThreads) ss[i] = segs[(long long)b * 2 * S + i];
}

// the last segment [start, end) that covers t, or -1
__device__ __forceinline__ int seg_last(const int* ss, int S, int t) {
  int last = -1;
  for (int j = 0; j < S; ++j)
    if (t >= ss[2 * j] && t < ss[2 * j + 1]) last = j;
  return last;
}

// ---------------------------------------------------------------- resample

__global__ void __launch_bounds__(kThreads)
    resample_kernel(const float* __restrict__ x, int T, int C, RsTab g, int T_out, float* __restrict__ y) {
  __shared__ float sw[kWMax];
  __shared__ int sf[kLMax];
  __shared__ float sx[kSpanMax];
  const int nt = max(1, kTile / C);
  const int n0 = blockIdx.x * nt;
  const int nb = min(n0 + nt, T_out);
  const float* xr = x + (long long)blockIdx.y * T * C;
  float* yr = y + ((long long)blockIdx.y * T_out + n0) * C;
  int lo, hi, t_lo;
  long long span;
  rs_load(g, sw, sf, lo, hi);
  rs_span(g, lo, hi, n0, nb, t_lo, span);
  const int nel = (nb - n0) * C;
  if (span * C <= kSpanMax) {
    rs_stage(xr, T, C, t_lo, (int)span * C, sx);
    __syncthreads();
    for (int e = threadIdx.x; e < nel; e += kThreads)
      yr[e] = rs_at<true>(g, sw, sf, sx, n0 + e / C, e % C, C, T, t_lo);
  } else {
    for (int e = threadIdx.x; e < nel; e += kThreads)
      yr[e] = rs_at<false>(g, sw, sf, xr, n0 + e / C, e % C, C, T, 0);
  }
}

// ------------------------------------------------------------ 101-tap filter

__global__ void __launch_bounds__(kThreads)
    fir101_kernel(const float* __restrict__ x, int T, const float* __restrict__ taps, float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float sr[kFirN];
  __shared__ float st[kTaps];
  const int tile0 = blockIdx.x * kTile;
  const float* xr = x + (long long)blockIdx.y * T;
  float* yr = y + (long long)blockIdx.y * T;
  if (threadIdx.x < kTaps) st[threadIdx.x] = taps[threadIdx.x];
  for (int e = threadIdx.x; e < kFirN; e += kThreads) {
    const int t = tile0 - kHalo + e;
    sr[e] = (t >= 0 && t < T) ? xr[t] : 0.f;
  }
  __syncthreads();
  fir_tile(sr, st);
  for (int e = threadIdx.x; e < kTile; e += kThreads)
    if (tile0 + e < T) yr[tile0 + e] = sr[e];
}

// ------------------------------------------------------------- chunk fill

// partial[b][c] = sum |x[b, t]| over the row's c-th slice of `chunk` samples
__global__ void __launch_bounds__(kThreads)
    abs_partial_kernel(const float* __restrict__ x, int T, int chunk, float* __restrict__ partial) {
  __shared__ float red[kThreads];
  const float* xr = x + (long long)blockIdx.y * T;
  const long long beg = (long long)blockIdx.x * chunk;
  const int end = (int)min((long long)T, beg + chunk);
  float s = 0.f;
  for (int t = (int)min(beg, (long long)T) + threadIdx.x; t < end; t += kThreads) s += fabsf(xr[t]);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.y * kAmpChunks + blockIdx.x] = red[0];
}

// y = x with every segment zeroed, or (noise != null) filled with
// 2 nm u - nm, nm = 2 amp_b noise_factor, u the segment's uploaded draws
__global__ void __launch_bounds__(kThreads)
    drop_chunks_kernel(const float* __restrict__ x, int T, int C, const int* __restrict__ segs, int S,
                       const int* __restrict__ noff, const float* __restrict__ noise, long long n_noise,
                       const int* __restrict__ lengths, float noise_factor, const float* __restrict__ partial,
                       float* __restrict__ amp, float* __restrict__ y) {
  __shared__ int ss[2 * kSegMax];
  __shared__ int so[kSegMax];
  __shared__ float samp;
  const int b = blockIdx.y;
  seg_load(segs, b, S, ss);
  if (noise) {
    for (int i = threadIdx.x; i < S; i += kThreads) so[i] = noff[(long long)b * S + i];
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int i = 0; i < kAmpChunks; ++i) s += partial[b * kAmpChunks + i];
      samp = s / (float)lengths[b];
      if (blockIdx.x == 0) amp[b] = samp;
    }
  }
  __syncthreads();
  const float nm = noise ? __fmul_rn(__fmul_rn(2.f, samp), noise_factor) : 0.f;
  const long long row = (long long)b * T * C;
  const long long nel = (long long)T * C;
  const long long e0 = (long long)blockIdx.x * kTile;
  for (int r = 0; r < kPer; ++r) {
    const long long e = e0 + threadIdx.x + r * kThreads;
    if (e >= nel) break;
    const int t = (int)(e / C);
    float v = x[row + e];
    const int j = seg_last(ss, S, t);
    if (j >= 0) {
      v = 0.f;
      if (noise) {
        const long long i = (long long)so[j] + (t - ss[2 * j]);
        const float u = (i >= 0 && i < n_noise) ? noise[i] : 0.f;
        v = __fsub_rn(__fmul_rn(__fmul_rn(2.f, nm), u), nm);
      }
    }
    y[row + e] = v;
  }
}

// ------------------------------------------------------------------- fused

// resample -> filter -> segment zeroing of one (B, T) batch in one launch.
// The workgroup resamples its tile plus the filter's halo into LDS (zero
// outside [0, T_out): the filter pads the resampled signal), filters out of
// LDS and zeroes the segments on the store.
template <bool RS, bool FIR>
__global__ void __launch_bounds__(kThreads)
    tdaug_kernel(const float* __restrict__ x, int T, RsTab g, int T_out, const float* __restrict__ taps,
                 const int* __restrict__ segs, int S, float* __restrict__ y) {
  __shared__ float sw[RS ? kWMax : 1];
  __shared__ int sf[RS ? kLMax : 1];
  __shared__ float sx[RS ? kSpanMax : 1];
  __shared__ __attribute__((aligned(16))) float sr[FIR ? kFirN : 4];
  __shared__ float st[FIR ? kTaps : 1];
  __shared__ int ss[2 * kSegMax];
  const int tile0 = blockIdx.x * kTile;
  const float* xr = x + (long long)blockIdx.y * T;
  float* yr = y + (long long)blockIdx.y * T_out;
  seg_load(segs, blockIdx.y, S, ss);
  if (FIR && threadIdx.x < kTaps) st[threadIdx.x] = taps[threadIdx.x];
  int t_lo = 0;
  bool staged = false;
  if (RS) {
    const int na = max(tile0 - (FIR ? kHalo : 0), 0);
    const int nb = min(tile0 + kTile + (FIR ? kHalo : 0), T_out);
    int lo, hi;
    long long span;
    rs_load(g, sw, sf, lo, hi);
    rs_span(g, lo, hi, na, nb, t_lo, span);
    staged = span <= kSpanMax;
    if (staged) rs_stage(xr, T, 1, t_lo, (int)span, sx);
  }
  __syncthreads();
  if (FIR) {
    for (int e = threadIdx.x; e < kFirN; e += kThreads) {
      const int n = tile0 - kHalo + e;
      float v = 0.f;
      if (n >= 0 && n < T_out) {
        if (!RS)
          v = xr[n];
        else if (staged)
          v = rs_at<true>(g, sw, sf, sx, n, 0, 1, T, t_lo);
        else
          v = rs_at<false>(g, sw, sf, xr, n, 0, 1, T, 0);
      }
      sr[e] = v;
    }
    __syncthreads();
    fir_tile(sr, st);
  }
  for (int e = threadIdx.x; e < kTile; e += kThreads) {
    const int n = tile0 + e;
    if (n >= T_out) break;
    float v;
    if (FIR)
      v = sr[e];
    else if (!RS)
      v = xr[n];
    else if (staged)
      v = rs_at<true>(g, sw, sf, sx, n, 0, 1, T, t_lo);
    else
      v = rs_at<false>(g, sw, sf, xr, n, 0, 1, T, 0);
    yr[n] = seg_last(ss, S, n) >= 0 ? 0.f : v;
  }
}

bool table_ok(const int* first, const float* w, int L, int M, int W) {
  return first && w && L > 0 && M > 0 && W > 0 && L <= kLMax && (long long)L * W <= kWMax;
}

constexpr int kGridY = 65535;

}  // namespace

// Output elements one workgroup of these kernels owns (the tests place their
// lengths around it).
SBK_API int sbk_tdaug_tile(void) { return kTile; }

// y (B, T_out, C) fp32 = x (B, T, C) fp32 resampled with the polyphase table
// first (L) int32, w (L, W) fp32: y[kL + i] = sum_j w[i][j] x[first[i] + kM + j],
// x zero outside [0, T), j ascending.
SBK_API int sbk_resample(const float* x, int B, int T, int C, const int* first, const float* w, int L, int M, int W,
                         int T_out, float* y, void* stream) {
  if (!x || !y || B <= 0 || B > kGridY || T <= 0 || C <= 0 || T_out <= 0 || !table_ok(first, w, L, M, W))
    return SBK_ERR_ARG;
  if ((long long)T * C > 0x7fffffffLL || (long long)T_out * C > 0x7fffffffLL) return SBK_ERR_ARG;
  const int nt = kTile / C > 0 ? kTile / C : 1;
  const RsTab g{first, w, L, M, W};
  hipLaunchKernelGGL(resample_kernel, dim3((T_out + nt - 1) / nt, B), dim3(kThreads), 0, (hipStream_t)stream, x, T, C, g,
                     T_out, y);
  SBK_CHECK_LAUNCH();
  return 0;
}

// y (B, T) fp32: y[t] = sum_k taps[k] x[t + k - 50], x zero outside [0, T), k
// ascending; taps (101) fp32.
SBK_API int sbk_fir101(const float* x, int B, int T, const float* taps, float* y, void* stream) {
  if (!x || !y || !taps || B <= 0 || B > kGridY || T <= 0) return SBK_ERR_ARG;
  hipLaunchKernelGGL(fir101_kernel, dim3((T + kTile - 1) / kTile, B), dim3(kThreads), 0, (hipStream_t)stream, x, T, taps,
                     y);
  SBK_CHECK_LAUNCH();
  return 0;
}

// y (B, T, C) fp32 = x with the samples of segs (B, S, 2) int32 [start, end)
// zeroed (empty segments pad a row to S).  With noise (n_noise draws in
// [0, 1)) the samples of segment j of row b become 2 nm u - nm instead,
// u = noise[noff[b][j] + t - start], nm = 2 amp_b noise_factor, amp_b =
// sum_t |x[b, t]| / lengths[b]; where segments overlap the last one wins.
// That path needs C == 1, noff (B, S) and lengths (B) int32, partial
// (B, 64) and amp (B) fp32; amp receives amp_b.
SBK_API int sbk_drop_chunks(const float* x, int B, int T, int C, const int* segs, int S, const int* noff,
                            const float* noise, long long n_noise, const int* lengths, float noise_factor,
                            float* partial, float* amp, float* y, void* stream) {
  if (!x || !y || B <= 0 || B > kGridY || T <= 0 || C <= 0 || S < 0 || S > kSegMax || (S > 0 && !segs))
    return SBK_ERR_ARG;
  if ((long long)T * C > 0x7fffffffLL) return SBK_ERR_ARG;
  if (noise && (C != 1 || !noff || !lengths || !partial || !amp || n_noise <= 0 || S == 0)) return SBK_ERR_ARG;
  if (noise) {
    const int chunk = (T + kAmpChunks - 1) / kAmpChunks;
    hipLaunchKernelGGL(abs_partial_kernel, dim3(kAmpChunks, B), dim3(kThreads), 0, (hipStream_t)stream, x, T, chunk,
                       partial);
    SBK_CHECK_LAUNCH();
  }
  const long long nel = (long long)T * C;
  hipLaunchKernelGGL(drop_chunks_kernel, dim3((unsigned)((nel + kTile - 1) / kTile), B), dim3(kThreads), 0,
                     (hipStream_t)stream, x, T, C, segs, S, noff, noise, n_noise, lengths, noise_factor, partial, amp, y);
  SBK_CHECK_LAUNCH();
  return 0;
}

// y (B, T_out) fp32 = sbk_resample -> sbk_fir101 -> sbk_drop_chunks (zero
// fill) of x (B, T) in one launch, bit-identical to the three in sequence.
// first == null: no resample (T_out == T); taps == null: no filter; S == 0:
// no segments; none of the three: a copy.
SBK_API int sbk_tdaug(const float* x, int B, int T, const int* first, const float* w, int L, int M, int W, int T_out,
                      const float* taps, const int* segs, int S, float* y, void* stream) {
  if (!x || !y || B <= 0 || B > kGridY || T <= 0 || T_out <= 0 || S < 0 || S > kSegMax || (S > 0 && !segs))
    return SBK_ERR_ARG;
  if (first ? !table_ok(first, w, L, M, W) : T_out != T) return SBK_ERR_ARG;
  const RsTab g{first, w, L, M, W};
  const dim3 grid((T_out + kTile - 1) / kTile, B), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
  if (first && taps)
    hipLaunchKernelGGL((tdaug_kernel<true, true>), grid, block, 0, s, x, T, g, T_out, taps, segs, S, y);
  else if (first)
    hipLaunchKernelGGL((tdaug_kernel<true, false>), grid, block, 0, s, x, T, g, T_out, taps, segs, S, y);
  else if (taps)
    hipLaunchKernelGGL((tdaug_kernel<false, true>), grid, block, 0, s, x, T, g, T_out, taps, segs, S, y);
  else if (S > 0)
    hipLaunchKernelGGL((tdaug_kernel<false, false>), grid, block, 0, s, x, T, g, T_out, taps, segs, S, y);
  else
    return (int)hipMemcpyAsync(y, x, (size_t)B * T * sizeof(float), hipMemcpyDeviceToDevice, s);
  SBK_CHECK_LAUNCH();
  return 0;
}
