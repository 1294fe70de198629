// RelPosMHAXL with query != key/value and q_len != k_len: the attention core
// of speechbrain/nnet/attention.py:554-639 for separate q / k / v
// projections (the projections themselves run on sbk_gemm), with the
// reference's rel_shift (:468-483) on a (q_len, P) positional band, its
// mask_pos_future tril, attn_mask, key padding, softmax, attention dropout
// and P·V — and the backward of all of it.
//
// Not on the encoder's hot path (every Conformer call site is
// self-attention, which runs in the fused flash kernel of attention.hip), so
// these kernels are plain fp32 VALU.  The per-row kernels take one workgroup
// per (query row | key row | band column, head, batch), the row of scores in
// LDS; they serve any shape and alignment.  The blocked kernels (*_qb_kernel:
// 16 rows per workgroup, the other operand through LDS in chunks of 64 rows,
// thread (row, sub) of 16 threads per row) are assembled from one set of tile
// primitives, each defined once below: xq_stage_rows (global rows -> padded
// LDS rows), dot4 (a thread's four scores of a chunk), fma8 / acc8_rows (its
// eight output dims), store8 (their guarded store) and row16_max / row16_sum
// (the reductions over a row's 16 threads).  Every kernel's dynamic-LDS
// carve-up is one *_lds() layout that the kernel and its launch both read,
// and every dropout is sbk::Dropout.  What the kernels must get
// right is the rel_shift of a non-square band: output (i, j) of the
// reference's pad / view / drop-row trick is flat element
// p = i*P + j + q_len of the left-padded (q_len, P+1) band, i.e. row
// r = p / (P+1), column c = p % (P+1) (c == 0: the zero pad, else
// bd[r][c-1]).  For q_len > k_len, r can be i + 1 or further: the reference
// reads the next row there, and so do these kernels.
//
// Layouts: q (B*Lq, ldq), k (B*Lk, ldk), v (B*Lk, ldv), pk (P, ldp), head h
// at columns [h*dh, (h+1)*dh), fp32 or bf16; pbu / pbv (H*dh) fp32 (the
// (dh, H) parameters read as (H, dh), attention.py:586-592); probabilities
// (B, H, Lq, Lk) fp32.
//
// pk == nullptr selects plain scaled dot-product attention (the
// MultiheadAttention drop-in's general path, attention.py:642-778): no
// positional term, no u / v biases (pbu / pbv may be null), and the backward
// skips the band passes — dq comes straight out of the row pass.
#include "sbk_common.h"

#include <math.h>

#include <initializer_list>

namespace {

using sbk::bf16_to_f32;
using sbk::Dropout;
using sbk::f32_to_bf16;

constexpr int kThreads = 256;

__device__ __forceinline__ float ld(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ float ld(const uint16_t* p, long long i) { return bf16_to_f32(p[i]); }
__device__ __forceinline__ void st(float* p, long long i, float v) { p[i] = v; }
__device__ __forceinline__ void st(uint16_t* p, long long i, float v) { p[i] = f32_to_bf16(v); }

// Dynamic-LDS layout of a kernel: N consecutive float arrays, array i at
// sm + off[i].  Each kernel's layout is one function next to it; the kernel
// carves its pointers from it and the host sizes the launch from it.
template <int N>
struct Lds {
  int off[N + 1];
  __host__ __device__ size_t bytes() const { return (size_t)off[N] * sizeof(float); }
};
template <typename... S>
__host__ __device__ __forceinline__ Lds<sizeof...(S)> lds_of(S... floats) {
  Lds<sizeof...(S)> l{};
  int i = 0, n = 0;
  ((l.off[i++] = n, n += floats), ...);
  l.off[i] = n;
  return l;
}

__device__ float block_reduce(float v, float* red, bool is_max) {
  v = is_max ? sbk::wave_max(v) : sbk::wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int k = 1; k < kThreads / 64; ++k) r = is_max ? fmaxf(r, red[k]) : r + red[k];
  return r;
}

// y[d] = sum_n w[n] * X[n][d] over n < N for d < dh; X row n at X + n * ldx
// (+ head offset already applied); w in LDS.  Four 64-lane groups split n;
// partials combine through `part` (4 * 64 floats).  Calls fn(d, y) once per d.
template <typename TI, typename F>
__device__ void weighted_rows(const float* w, const TI* X, long long ldx, int N, int dh, float* part, F fn) {
  const int dl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  for (int d0 = 0; d0 < dh; d0 += 64) {
    const int d = d0 + dl;
    float acc = 0.f;
    if (d < dh)
      for (int n = grp; n < N; n += 4) acc += w[n] * ld(X, n * ldx + d);
    __syncthreads();
    part[grp * 64 + dl] = acc;
    __syncthreads();
    if (grp == 0 && d < dh) fn(d, part[dl] + part[64 + dl] + part[128 + dl] + part[192 + dl]);
  }
}

// the source element of output (i, j) of rel_shift: returns the band row r
// and column c (c < 0: the zero pad or a mask_pos_future zero)
__device__ __forceinline__ void shift_src(int i, int j, int Lq, int P, int mpf, int& r, int& c) {
  const long long p = (long long)i * P + j + Lq;
  r = (int)(p / (P + 1));
  c = (int)(p % (P + 1)) - 1;
  if (mpf && j - i > P - Lq) c = -1;
}

// forward and backward row pass, per row: s | qu | red | part, g | dor | red | part
__host__ __device__ inline Lds<4> row_lds(int Lk, int dh) { return lds_of(Lk, dh, 64, 256); }

template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_fwd_kernel(
    const TI* __restrict__ q, int ldq, const TI* __restrict__ k, int ldk, const TI* __restrict__ v, int ldv,
    const TI* __restrict__ pk, int ldp, int P, const float* __restrict__ pbu, const float* __restrict__ pbv, int mpf,
    const unsigned char* __restrict__ kpm, const float* __restrict__ am, long long am_sb, long long am_sh, int Lq,
    int Lk, int H, int dh, float scale, Dropout drop, TI* __restrict__ out, int ldo, float* __restrict__ probs,
    float* __restrict__ attn) {
  extern __shared__ float sm[];
  const auto L = row_lds(Lk, dh);
  float* s = sm + L.off[0];     // Lk scores -> probabilities (dropped)
  float* qu = sm + L.off[1];    // q_i + u
  float* red = sm + L.off[2];   // 64
  float* part = sm + L.off[3];  // 256
  const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const TI* qrow = q + (long long)(b * Lq + i) * ldq + h * dh;
  for (int d = threadIdx.x; d < dh; d += kThreads) qu[d] = ld(qrow, d) + (pbu ? pbu[h * dh + d] : 0.f);
  __syncthreads();
  const float* am_row = am ? am + b * am_sb + h * am_sh + (long long)i * Lk : nullptr;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < Lk; j += kThreads) {
    const TI* krow = k + (long long)(b * Lk + j) * ldk + h * dh;
    float ac = 0.f;
    for (int d = 0; d < dh; ++d) ac += qu[d] * ld(krow, d);
    float bd = 0.f;
    int r = 0, c = -1;
    if (pk) shift_src(i, j, Lq, P, mpf, r, c);
    if (c >= 0) {
      const TI* qr = q + (long long)(b * Lq + r) * ldq + h * dh;
      const TI* pr = pk + (long long)c * ldp + h * dh;
      for (int d = 0; d < dh; ++d) bd += (ld(qr, d) + pbv[h * dh + d]) * ld(pr, d);
    }
    float sc = (ac + bd) * scale;
    if (am_row) sc += am_row[j];
    if (kpm && kpm[(long long)b * Lk + j]) sc = -INFINITY;
    s[j] = sc;
    mx = fmaxf(mx, sc);
  }
  mx = block_reduce(mx, red, true);
  float sum = 0.f;
  for (int j = threadIdx.x; j < Lk; j += kThreads) {
    const float e = expf(s[j] - mx);  // all -inf: NaN, as the reference's softmax
    s[j] = e;
    sum += e;
  }
  sum = block_reduce(sum, red, false);
  const float inv = 1.f / sum;
  const long long prow = (((long long)b * H + h) * Lq + i) * Lk;
  for (int j = threadIdx.x; j < Lk; j += kThreads) {
    const float pv = s[j] * inv;
    probs[prow + j] = pv;
    const float pd = drop.apply(prow + j, pv);
    if (drop.use) attn[prow + j] = pd;
    s[j] = pd;
  }
  __syncthreads();
  TI* orow = out + (long long)(b * Lq + i) * ldo + h * dh;
  weighted_rows(s, v + (long long)b * Lk * ldv + h * dh, ldv, Lk, dh, part,
                [&](int d, float y) { st(orow, d, y); });
}

// ---------------------------------------------------------------- blocked
// One workgroup per (XQ_QB rows, head, batch).  The per-row kernels give
// every score its own thread and walk a key row dimension by dimension, so
// a wave reads 64 different rows element-wise and every query row re-reads
// all of K and V (decoder cross-attention over 376 keys: 1.2-2x torch's
// GEMM-based MHA, profiles/r06u_mha_decoder_timing.log).  Here the other
// operand passes through LDS in chunks of XQ_KC rows, read once per XQ_QB
// rows with coalesced loads, and thread (ri, sub) = (tid / 16, tid % 16)
// owns row ri: in a score step the chunk rows sub + 16 m, in an output step
// the dims 8 sub .. 8 sub + 7.  The LDS rows are padded to DP = dh + 4 floats
// so the dot products read 16 B at a time, the 16 chunk rows of a lane group
// 4 banks apart.  fp32 VALU as above (exact fp32 operands for the parity
// path).  The tile steps, each written once:
constexpr int XQ_QB = 16, XQ_KC = 64, XQ_DMAX = 128, XQ_LKMAX = 1024;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const uint16_t* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}

// Stage: rows row0 .. row0 + ROWS - 1 of src (row stride ld_src elements,
// 4-element aligned) -> dst (row stride ld_dst floats); rows outside
// [0, rows_total) -> 0 (one unsigned compare: a signed two-sided bound cost
// 50-160 instructions per kernel).  Every load of the thread is issued
// before the first LDS store (a load -> store loop per element paid the
// global latency once per element: the first version of these kernels spent
// most of its time there).
template <int ROWS, typename TI>
__device__ __forceinline__ void xq_stage_rows(float* dst, int ld_dst, const TI* src, long long ld_src, int row0,
                                              int rows_total, int dh) {
  constexpr int PT = (ROWS * (XQ_DMAX / 4) + kThreads - 1) / kThreads;  // float4 per thread at dh = XQ_DMAX
  const int q4 = dh >> 2, total = ROWS * q4;
  float4 v[PT];
#pragma unroll
  for (int u = 0; u < PT; ++u) {
    const int e = threadIdx.x + u * kThreads;
    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < total) {
      const int r = e / q4, c = (e - r * q4) * 4, gr = row0 + r;
      if ((unsigned)gr < (unsigned)rows_total) v[u] = ld4(src + (long long)gr * ld_src + c);
    }
  }
#pragma unroll
  for (int u = 0; u < PT; ++u) {
    const int e = threadIdx.x + u * kThreads;
    if (e < total) {
      const int r = e / q4, c = (e - r * q4) * 4;
      *reinterpret_cast<float4*>(dst + r * ld_dst + c) = v[u];
    }
  }
}
// the first rmax rows of src (src already at its first row)
template <int ROWS, typename TI>
__device__ __forceinline__ void xq_stage(float* dst, int ld_dst, const TI* src, long long ld_src, int rmax, int dh) {
  xq_stage_rows<ROWS>(dst, ld_dst, src, ld_src, 0, rmax, dh);
}

// Four dots, one float4 step: acc[m] += x · T[row(m)] over the four dims at
// T (the staged tile, already offset to the step's dim; rows DP apart).
template <typename R>
__device__ __forceinline__ void dot4(float (&acc)[XQ_KC / 16], const float4 x, const float* T, int DP, R row) {
#pragma unroll
  for (int m = 0; m < XQ_KC / 16; ++m) {
    const float4 t = ld4(T + row(m) * DP);
    acc[m] += x.x * t.x + x.y * t.y + x.z * t.z + x.w * t.w;
  }
}

// Eight dims of one row: acc[0..8) += w * x[0..8).
__device__ __forceinline__ void fma8(float (&acc)[8], float w, const float* x) {
  const float4 a = ld4(x), b = ld4(x + 4);
  acc[0] += w * a.x; acc[1] += w * a.y; acc[2] += w * a.z; acc[3] += w * a.w;
  acc[4] += w * b.x; acc[5] += w * b.y; acc[6] += w * b.z; acc[7] += w * b.w;
}
// ... of the n rows of a staged tile: acc += sum_r w[r] * X[r][0..8) (X
// already offset to the thread's first dim; rows DP apart).
__device__ __forceinline__ void acc8_rows(float (&acc)[8], const float* w, const float* X, int DP, int n) {
  for (int r = 0; r < n; ++r) fma8(acc, w[r], X + r * DP);
}

// fn(d, acc[d - d0]) for the thread's dims d0 <= d < min(d0 + 8, dh)
template <typename F>
__device__ __forceinline__ void store8(const float (&acc)[8], int d0, int dh, F fn) {
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (d0 + e < dh) fn(d0 + e, acc[e]);
}

// max / sum over the 16 threads of a row (lanes 16 ri .. 16 ri + 15 of one wave)
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 16));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

// Forward, query-blocked: the scores of the block stay in LDS (QB x Lk) for
// the softmax, and P·V accumulates per (row, 8 output dims).
//
// POS: the rel-pos band term as well.  Output (i, j) takes band element
// (r, c) = shift_src(i, j); for the common r == i it is (q_i + v)·pk_c with
// c = j - i + Lq - 1, so the (QB + KC - 1) band rows a block-chunk needs are
// staged beside the K chunk (XQ_BR rows from c_base); the wrap rows of the
// reference's rel_shift (r > i: q_len > k_len) read global memory.
constexpr int XQ_BR = XQ_QB + XQ_KC;  // staged band rows per chunk (79 used)

// qs | kv | qv (POS) | band (POS) | s
__host__ __device__ inline Lds<5> fwd_qb_lds(int dh, int Lk, bool pos) {
  const int DP = dh + 4;
  return lds_of(XQ_QB * DP, XQ_KC * DP, pos ? XQ_QB * DP : 0, pos ? XQ_BR * DP : 0, XQ_QB * Lk);
}

template <typename TI, bool POS>
__global__ __launch_bounds__(kThreads) void xattn_fwd_qb_kernel(
    const TI* __restrict__ q, int ldq, const TI* __restrict__ k, int ldk, const TI* __restrict__ v, int ldv,
    const TI* __restrict__ pk, int ldp, int P, const float* __restrict__ pbu, const float* __restrict__ pbv, int mpf,
    const unsigned char* __restrict__ kpm, const float* __restrict__ am, long long am_sb, long long am_sh, int Lq,
    int Lk, int H, int dh, float scale, Dropout drop, TI* __restrict__ out, int ldo, float* __restrict__ probs,
    float* __restrict__ attn) {
  extern __shared__ float sm[];
  const int DP = dh + 4;  // padded LDS row (floats): 16-B aligned, rows 4 banks apart
  const auto L = fwd_qb_lds(dh, Lk, POS);
  float* qs = sm + L.off[0];    // XQ_QB x DP (POS: q + u)
  float* kv = sm + L.off[1];    // XQ_KC x DP (K chunk, then V chunk)
  float* qv = sm + L.off[2];    // POS: XQ_QB x DP, q + v
  float* band = sm + L.off[3];  // POS: XQ_BR x DP band rows from c_base
  float* s = sm + L.off[4];     // XQ_QB x Lk scores -> probabilities (dropped)
  const int i0 = blockIdx.x * XQ_QB, h = blockIdx.y, b = blockIdx.z;
  const int nq = min(XQ_QB, Lq - i0);
  const int tid = threadIdx.x, ri = tid >> 4, sub = tid & 15;  // row ri, 16 threads per row
  const TI* qblk = q + (long long)(b * Lq + i0) * ldq + h * dh;
  xq_stage<XQ_QB>(qs, DP, qblk, ldq, nq, dh);
  if constexpr (POS) {
    xq_stage<XQ_QB>(qv, DP, qblk, ldq, nq, dh);
    __syncthreads();
    for (int e = tid; e < XQ_QB * dh; e += kThreads) {
      const int r = e / dh, d = e - r * dh;
      qs[r * DP + d] += pbu[h * dh + d];
      qv[r * DP + d] += pbv[h * dh + d];
    }
  }
  const int i = i0 + ri;
  // scores: thread (ri, sub) takes keys j0 + sub + 16 m of each chunk
  for (int j0 = 0; j0 < Lk; j0 += XQ_KC) {
    const int nk = min(XQ_KC, Lk - j0);
    const int cb = j0 - i0 - (XQ_QB - 1) + Lq - 1;  // band row of (i0 + 15, j0) when r == i
    __syncthreads();  // the previous chunk's readers are done (and qs is staged)
    xq_stage<XQ_KC>(kv, DP, k + (long long)(b * Lk + j0) * ldk + h * dh, ldk, nk, dh);
    if constexpr (POS) xq_stage_rows<XQ_BR>(band, DP, pk + h * dh, ldp, cb, P, dh);
    __syncthreads();
    float ac[XQ_KC / 16] = {};
    float bd[XQ_KC / 16] = {};
    int bro[XQ_KC / 16];  // POS: LDS band row of each key (-1: zero term; -2: wrap row, global)
    int wr[XQ_KC / 16], wc[XQ_KC / 16];
    if constexpr (POS) {
#pragma unroll
      for (int m = 0; m < XQ_KC / 16; ++m) {
        const int j = j0 + sub + 16 * m;
        int r = 0, c = -1;
        if (j < Lk && ri < nq) shift_src(i, j, Lq, P, mpf, r, c);
        wr[m] = r;
        wc[m] = c;
        bro[m] = c < 0 ? -1 : (r == i && c - cb >= 0 && c - cb < XQ_BR) ? c - cb : -2;
      }
    }
    const float* qr = qs + ri * DP;
    const float* vr = qv + ri * DP;
    for (int d = 0; d < dh; d += 4) {
      dot4(ac, ld4(qr + d), kv + d, DP, [&](int m) { return sub + 16 * m; });
      if constexpr (POS) dot4(bd, ld4(vr + d), band + d, DP, [&](int m) { return max(bro[m], 0); });
    }
    if constexpr (POS) {
#pragma unroll
      for (int m = 0; m < XQ_KC / 16; ++m) {
        if (bro[m] == -1) bd[m] = 0.f;
        if (bro[m] == -2) {  // rel_shift wrap row (r > i): (q_r + v)·pk_c from global memory
          const TI* qrow = q + (long long)(b * Lq + wr[m]) * ldq + h * dh;
          const TI* prow = pk + (long long)wc[m] * ldp + h * dh;
          float t = 0.f;
          for (int d = 0; d < dh; ++d) t += (ld(qrow, d) + pbv[h * dh + d]) * ld(prow, d);
          bd[m] = t;
        }
      }
    }
    const float* am_row = (am && ri < nq) ? am + b * am_sb + h * am_sh + (long long)i * Lk : nullptr;
#pragma unroll
    for (int m = 0; m < XQ_KC / 16; ++m) {
      const int j = j0 + sub + 16 * m;
      if (j >= Lk) continue;
      float sc = (ac[m] + bd[m]) * scale;
      if (am_row) sc += am_row[j];
      if (kpm && kpm[(long long)b * Lk + j]) sc = -INFINITY;
      s[ri * Lk + j] = sc;
    }
  }
  __syncthreads();
  // softmax per row
  float mx = -INFINITY;
  for (int j = sub; j < Lk; j += 16) mx = fmaxf(mx, s[ri * Lk + j]);
  mx = row16_max(mx);
  float sum = 0.f;
  for (int j = sub; j < Lk; j += 16) {
    const float e = expf(s[ri * Lk + j] - mx);  // all -inf: NaN, as the reference's softmax
    s[ri * Lk + j] = e;
    sum += e;
  }
  sum = row16_sum(sum);
  const float inv = 1.f / sum;
  const long long prow = (((long long)b * H + h) * Lq + i0 + ri) * Lk;
  for (int j = sub; j < Lk; j += 16) {
    const float pv = s[ri * Lk + j] * inv;
    float pd = pv;
    if (ri < nq) {
      probs[prow + j] = pv;
      pd = drop.apply(prow + j, pv);
      if (drop.use) attn[prow + j] = pd;
    }
    s[ri * Lk + j] = pd;
  }
  // out[ri][8 sub .. 8 sub + 7] (+ 128 per extra pass for dh > 128: not taken, dh <= XQ_DMAX)
  float acc[8] = {};
  const int d0 = 8 * sub;
  for (int j0 = 0; j0 < Lk; j0 += XQ_KC) {
    const int nk = min(XQ_KC, Lk - j0);
    __syncthreads();
    xq_stage<XQ_KC>(kv, DP, v + (long long)(b * Lk + j0) * ldv + h * dh, ldv, nk, dh);
    __syncthreads();
    if (d0 < dh) acc8_rows(acc, s + ri * Lk + j0, kv + d0, DP, nk);
  }
  if (ri < nq && d0 < dh) {
    TI* orow = out + (long long)(b * Lq + i0 + ri) * ldo + h * dh;
    store8(acc, d0, dh, [&](int d, float y) { st(orow, d, y); });
  }
}

// Backward, row pass: per query row i, dP = dO·Vᵀ (through the dropout
// mask), G = P ⊙ (dP - Σ P dP) · scale (the gradient of the pre-scale
// score (ac + bd)), and dq_ac = G·K.
template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_bwd_rows_kernel(
    const TI* __restrict__ k, int ldk, const TI* __restrict__ v, int ldv, const TI* __restrict__ dO, int lddo,
    const float* __restrict__ probs, int Lq, int Lk, int H, int dh, float scale, Dropout drop,
    float* __restrict__ G, float* __restrict__ dqu) {
  extern __shared__ float sm[];
  const auto L = row_lds(Lk, dh);
  float* g = sm + L.off[0];     // Lk
  float* dor = sm + L.off[1];   // dh
  float* red = sm + L.off[2];   // 64
  float* part = sm + L.off[3];  // 256
  const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const TI* drow = dO + (long long)(b * Lq + i) * lddo + h * dh;
  for (int d = threadIdx.x; d < dh; d += kThreads) dor[d] = ld(drow, d);
  __syncthreads();
  const long long prow = (((long long)b * H + h) * Lq + i) * Lk;
  float dot = 0.f;
  for (int j = threadIdx.x; j < Lk; j += kThreads) {
    const TI* vrow = v + (long long)(b * Lk + j) * ldv + h * dh;
    float dp = 0.f;
    for (int d = 0; d < dh; ++d) dp += dor[d] * ld(vrow, d);
    dp = drop.apply(prow + j, dp);
    g[j] = dp;
    dot += probs[prow + j] * dp;
  }
  dot = block_reduce(dot, red, false);
  for (int j = threadIdx.x; j < Lk; j += kThreads) {
    const float gv = probs[prow + j] * (g[j] - dot) * scale;
    g[j] = gv;
    G[prow + j] = gv;
  }
  __syncthreads();
  float* dq = dqu + (long long)(b * Lq + i) * H * dh + h * dh;
  weighted_rows(g, k + (long long)b * Lk * ldk + h * dh, ldk, Lk, dh, part, [&](int d, float y) { dq[d] = y; });
}

// ds | kv | g
__host__ __device__ inline Lds<3> bwd_rows_qb_lds(int dh, int Lk) {
  return lds_of(XQ_QB * (dh + 4), XQ_KC * (dh + 4), XQ_QB * Lk);
}

// No-position backward row pass, query-blocked like xattn_fwd_qb_kernel:
// dP = dO·Vᵀ over V chunks in LDS, G = P ⊙ (dP - Σ P dP) · scale (written
// to global for the key-row pass), dq = G·K over K chunks in LDS.
template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_bwd_rows_qb_kernel(
    const TI* __restrict__ k, int ldk, const TI* __restrict__ v, int ldv, const TI* __restrict__ dO, int lddo,
    const float* __restrict__ probs, int Lq, int Lk, int H, int dh, float scale, Dropout drop,
    float* __restrict__ G, float* __restrict__ dq) {
  extern __shared__ float sm[];
  const int DP = dh + 4;
  const auto L = bwd_rows_qb_lds(dh, Lk);
  float* ds = sm + L.off[0];  // XQ_QB x DP: dO rows
  float* kv = sm + L.off[1];  // XQ_KC x DP: V chunk, then K chunk
  float* g = sm + L.off[2];   // XQ_QB x Lk: dP, then G
  const int i0 = blockIdx.x * XQ_QB, h = blockIdx.y, b = blockIdx.z;
  const int nq = min(XQ_QB, Lq - i0);
  const int tid = threadIdx.x, ri = tid >> 4, sub = tid & 15;
  xq_stage<XQ_QB>(ds, DP, dO + (long long)(b * Lq + i0) * lddo + h * dh, lddo, nq, dh);
  const long long prow = (((long long)b * H + h) * Lq + i0 + ri) * Lk;
  for (int j0 = 0; j0 < Lk; j0 += XQ_KC) {
    const int nk = min(XQ_KC, Lk - j0);
    __syncthreads();
    xq_stage<XQ_KC>(kv, DP, v + (long long)(b * Lk + j0) * ldv + h * dh, ldv, nk, dh);
    __syncthreads();
    float dp[XQ_KC / 16] = {};
    const float* dr = ds + ri * DP;
    for (int d = 0; d < dh; d += 4) dot4(dp, ld4(dr + d), kv + d, DP, [&](int m) { return sub + 16 * m; });
#pragma unroll
    for (int m = 0; m < XQ_KC / 16; ++m) {
      const int j = j0 + sub + 16 * m;
      if (j >= Lk) continue;
      float x = dp[m];
      if (ri < nq) x = drop.apply(prow + j, x);
      g[ri * Lk + j] = x;
    }
  }
  __syncthreads();
  float dot = 0.f;
  if (ri < nq)
    for (int j = sub; j < Lk; j += 16) dot += probs[prow + j] * g[ri * Lk + j];
  dot = row16_sum(dot);
  for (int j = sub; j < Lk; j += 16) {
    float gv = 0.f;
    if (ri < nq) {
      gv = probs[prow + j] * (g[ri * Lk + j] - dot) * scale;
      G[prow + j] = gv;
    }
    g[ri * Lk + j] = gv;
  }
  float acc[8] = {};
  const int d0 = 8 * sub;
  for (int j0 = 0; j0 < Lk; j0 += XQ_KC) {
    const int nk = min(XQ_KC, Lk - j0);
    __syncthreads();
    xq_stage<XQ_KC>(kv, DP, k + (long long)(b * Lk + j0) * ldk + h * dh, ldk, nk, dh);
    __syncthreads();
    if (d0 < dh) acc8_rows(acc, g + ri * Lk + j0, kv + d0, DP, nk);
  }
  if (ri < nq && d0 < dh) {
    float* dqr = dq + (long long)(b * Lq + i0 + ri) * H * dh + h * dh;
    store8(acc, d0, dh, [&](int d, float y) { dqr[d] = y; });
  }
}

// the band gradient dBD[r][c] of row r of batch b / head h: the G element
// whose rel_shift source is (r, c), or 0 (pad, masked, or sliced away)
__device__ __forceinline__ float dband(const float* Gbh, int r, int c, int Lq, int Lk, int P, int mpf) {
  const long long f = (long long)r * (P + 1) + c + 1 - Lq;
  if (f < 0) return 0.f;
  const int i = (int)(f / P), j = (int)(f % P);
  if (i >= Lq || j >= Lk) return 0.f;
  if (mpf && j - i > P - Lq) return 0.f;
  return Gbh[(long long)i * Lk + j];
}

// w | part
__host__ __device__ inline Lds<2> bwd_qv_lds(int P) { return lds_of(P, 256); }

// Backward, band-row pass: dq_bd[r] = Σ_c dBD[r][c] pk[c]; dq = dq_ac + dq_bd.
template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_bwd_qv_kernel(
    const TI* __restrict__ pk, int ldp, int P, const float* __restrict__ G, const float* __restrict__ dqu, int Lq,
    int Lk, int H, int dh, int mpf, float* __restrict__ dqv, float* __restrict__ dq) {
  extern __shared__ float sm[];
  const auto L = bwd_qv_lds(P);
  float* w = sm + L.off[0];     // P
  float* part = sm + L.off[1];  // 256
  const int r = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const float* Gbh = G + ((long long)b * H + h) * Lq * Lk;
  for (int c = threadIdx.x; c < P; c += kThreads) w[c] = dband(Gbh, r, c, Lq, Lk, P, mpf);
  __syncthreads();
  const long long o = (long long)(b * Lq + r) * H * dh + h * dh;
  weighted_rows(w, pk + h * dh, ldp, P, dh, part, [&](int d, float y) {
    dqv[o + d] = y;
    dq[o + d] = dqu[o + d] + y;
  });
}

// gc | pc | part
__host__ __device__ inline Lds<3> bwd_kv_lds(int Lq) { return lds_of(Lq, Lq, 256); }

// Backward, key-row pass: dk[j] = Σ_i G[i][j] (q_i + u), dv[j] = Σ_i Pd[i][j] dO_i.
template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_bwd_kv_kernel(
    const TI* __restrict__ q, int ldq, const TI* __restrict__ dO, int lddo, const float* __restrict__ pbu,
    const float* __restrict__ probs, const float* __restrict__ G, int Lq, int Lk, int H, int dh, Dropout drop,
    float* __restrict__ dk, float* __restrict__ dv) {
  extern __shared__ float sm[];
  const auto L = bwd_kv_lds(Lq);
  float* gc = sm + L.off[0];    // Lq: G[:, j]
  float* pc = sm + L.off[1];    // Lq: Pd[:, j]
  float* part = sm + L.off[2];  // 256
  const int j = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long long base = ((long long)b * H + h) * Lq * Lk + j;
  float gsum = 0.f;
  for (int i = threadIdx.x; i < Lq; i += kThreads) {
    const long long e = base + (long long)i * Lk;
    gc[i] = G[e];
    pc[i] = drop.apply(e, probs[e]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < Lq; i += kThreads) gsum += gc[i];
  float* red = part;  // reused below only after this reduction completes
  gsum = block_reduce(gsum, red, false);
  __syncthreads();
  const long long o = (long long)(b * Lk + j) * H * dh + h * dh;
  // Σ_i G[i][j] (q_i + u) = Σ_i G[i][j] q_i + u Σ_i G[i][j]
  weighted_rows(gc, q + (long long)b * Lq * ldq + h * dh, ldq, Lq, dh, part,
                [&](int d, float y) { dk[o + d] = y + (pbu ? pbu[h * dh + d] * gsum : 0.f); });
  weighted_rows(pc, dO + (long long)b * Lq * lddo + h * dh, lddo, Lq, dh, part,
                [&](int d, float y) { dv[o + d] = y; });
}

// gs | ps | qs | os
__host__ __device__ inline Lds<4> bwd_kv_qb_lds(int dh) {
  return lds_of(XQ_KC * XQ_QB, XQ_KC * XQ_QB, XQ_KC * (dh + 4), XQ_KC * (dh + 4));
}

// Key-row pass, key-blocked (dh <= XQ_DMAX): one workgroup per (XQ_QB key
// rows, head, batch) walks the query rows in chunks of XQ_KC: the G / P
// column slices of its keys (16 consecutive floats of each row) and the q /
// dO rows of the chunk go through LDS, thread (key row, 8 dims) accumulates
// dk and dv.  (The per-key kernel above read each G / P column element by
// element at a stride of Lk: 25 % of a decoder cross-attention's backward.)
template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_bwd_kv_qb_kernel(
    const TI* __restrict__ q, int ldq, const TI* __restrict__ dO, int lddo, const float* __restrict__ pbu,
    const float* __restrict__ probs, const float* __restrict__ G, int Lq, int Lk, int H, int dh, Dropout drop,
    float* __restrict__ dk, float* __restrict__ dv) {
  extern __shared__ float sm[];
  const int DP = dh + 4;
  const auto L = bwd_kv_qb_lds(dh);
  float* gs = sm + L.off[0];  // XQ_KC x XQ_QB: G[i][j0 + jj]
  float* ps = sm + L.off[1];  // XQ_KC x XQ_QB: Pd
  float* qs = sm + L.off[2];  // XQ_KC x DP: q rows
  float* os = sm + L.off[3];  // XQ_KC x DP: dO rows
  const int j0 = blockIdx.x * XQ_QB, h = blockIdx.y, b = blockIdx.z;
  const int nj = min(XQ_QB, Lk - j0);
  const int tid = threadIdx.x, rj = tid >> 4, sub = tid & 15, d0 = 8 * sub;
  const long long gbase = ((long long)b * H + h) * Lq * Lk + j0;
  float adk[8] = {}, adv[8] = {};
  float gsum = 0.f;
  for (int i0 = 0; i0 < Lq; i0 += XQ_KC) {
    const int ni = min(XQ_KC, Lq - i0);
    __syncthreads();
    for (int e = tid; e < XQ_KC * XQ_QB; e += kThreads) {
      const int ii = e / XQ_QB, jj = e - ii * XQ_QB;
      float gv = 0.f, pv = 0.f;
      if (ii < ni && jj < nj) {
        const long long x = gbase + (long long)(i0 + ii) * Lk + jj;
        gv = G[x];
        pv = drop.apply(x, probs[x]);
      }
      gs[e] = gv;
      ps[e] = pv;
    }
    xq_stage<XQ_KC>(qs, DP, q + (long long)(b * Lq + i0) * ldq + h * dh, ldq, ni, dh);
    xq_stage<XQ_KC>(os, DP, dO + (long long)(b * Lq + i0) * lddo + h * dh, lddo, ni, dh);
    __syncthreads();
    if (d0 < dh)
      for (int ii = 0; ii < ni; ++ii) {  // acc8_rows for dk and dv in one walk (and gsum)
        const float gj = gs[ii * XQ_QB + rj], pj = ps[ii * XQ_QB + rj];
        gsum += gj;
        fma8(adk, gj, qs + ii * DP + d0);
        fma8(adv, pj, os + ii * DP + d0);
      }
  }
  if (rj < nj && d0 < dh) {
    const long long o = (long long)(b * Lk + j0 + rj) * H * dh + h * dh;
    store8(adk, d0, dh, [&](int d, float y) { dk[o + d] = y + (pbu ? pbu[h * dh + d] * gsum : 0.f); });
    store8(adv, d0, dh, [&](int d, float y) { dv[o + d] = y; });
  }
}

// ps | w
__host__ __device__ inline Lds<2> bwd_qv_qb_lds(int dh) { return lds_of(XQ_KC * (dh + 4), XQ_QB * XQ_KC); }

// Band-row pass, blocked (dh <= XQ_DMAX, 16-B aligned pk): one workgroup
// per (XQ_QB band rows, head, batch) walks the band in chunks of XQ_KC
// rows staged through LDS (the per-row kernel above re-read all P rows of
// pk for every band row): w[r][c] = dBD[r][c] of the chunk into LDS, then
// thread (row, 8 dims) accumulates dq_bd = Σ_c w pk_c.
template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_bwd_qv_qb_kernel(
    const TI* __restrict__ pk, int ldp, int P, const float* __restrict__ G, const float* __restrict__ dqu, int Lq,
    int Lk, int H, int dh, int mpf, float* __restrict__ dqv, float* __restrict__ dq) {
  extern __shared__ float sm[];
  const int DP = dh + 4;
  const auto L = bwd_qv_qb_lds(dh);
  float* ps = sm + L.off[0];  // XQ_KC x DP: pk rows of the chunk
  float* w = sm + L.off[1];   // XQ_QB x XQ_KC: dBD of the chunk
  const int r0 = blockIdx.x * XQ_QB, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, ri = tid >> 4, sub = tid & 15, d0 = 8 * sub;
  const float* Gbh = G + ((long long)b * H + h) * Lq * Lk;
  float acc[8] = {};
  for (int c0 = 0; c0 < P; c0 += XQ_KC) {
    const int nc = min(XQ_KC, P - c0);
    __syncthreads();
    xq_stage<XQ_KC>(ps, DP, pk + (long long)c0 * ldp + h * dh, ldp, nc, dh);
    for (int e = tid; e < XQ_QB * XQ_KC; e += kThreads) {
      const int rr = e / XQ_KC, cc = e - rr * XQ_KC;
      w[e] = (r0 + rr < Lq && cc < nc) ? dband(Gbh, r0 + rr, c0 + cc, Lq, Lk, P, mpf) : 0.f;
    }
    __syncthreads();
    if (d0 < dh) acc8_rows(acc, w + ri * XQ_KC, ps + d0, DP, nc);
  }
  if (r0 + ri < Lq && d0 < dh) {
    const long long o = (long long)(b * Lq + r0 + ri) * H * dh + h * dh;
    store8(acc, d0, dh, [&](int d, float y) {
      dqv[o + d] = y;
      dq[o + d] = dqu[o + d] + y;
    });
  }
}

// w | part | red
__host__ __device__ inline Lds<3> bwd_pk_lds(int Lq) { return lds_of(Lq, 256, 64); }

// Backward, band-column pass: dpk[c] = Σ_b Σ_r dBD[b][r][c] (q_r + v).
template <typename TI>
__global__ __launch_bounds__(kThreads) void xattn_bwd_pk_kernel(
    const TI* __restrict__ q, int ldq, const float* __restrict__ pbv, const float* __restrict__ G, int B, int Lq,
    int Lk, int H, int dh, int P, int mpf, float* __restrict__ dpk) {
  extern __shared__ float sm[];
  const auto L = bwd_pk_lds(Lq);
  float* w = sm + L.off[0];     // Lq
  float* part = sm + L.off[1];  // 256
  float* red = sm + L.off[2];
  const int c = blockIdx.x, h = blockIdx.y;
  const int dl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int nd = (dh + 63) / 64;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // dh <= 256
  float wsum = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* Gbh = G + ((long long)b * H + h) * Lq * Lk;
    __syncthreads();
    for (int r = threadIdx.x; r < Lq; r += kThreads) {
      const float x = dband(Gbh, r, c, Lq, Lk, P, mpf);
      w[r] = x;
      wsum += x;
    }
    __syncthreads();
    const TI* qb = q + (long long)b * Lq * ldq + h * dh;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int d = t * 64 + dl;
      if (t < nd && d < dh)
        for (int r = grp; r < Lq; r += 4) acc[t] += w[r] * ld(qb, (long long)r * ldq + d);
    }
  }
  wsum = block_reduce(wsum, red, false);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= nd) break;
    const int d = t * 64 + dl;
    __syncthreads();
    part[grp * 64 + dl] = acc[t];
    __syncthreads();
    if (grp == 0 && d < dh)
      dpk[(long long)c * H * dh + h * dh + d] =
          part[dl] + part[64 + dl] + part[128 + dl] + part[192 + dl] + pbv[h * dh + d] * wsum;
  }
}

// ------------------------------------------------------------------- host
// operands the blocked kernels can stage 4 elements at a time
template <typename TI>
bool qb_aligned(std::initializer_list<const void*> ps, std::initializer_list<int> lds, int dh) {
  if (dh > XQ_DMAX || dh % 4) return false;
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) % (4 * sizeof(TI))) return false;
  for (int l : lds)
    if (l % 4) return false;
  return true;
}

// one launch of kThreads threads with `lds` bytes of dynamic LDS; the
// arguments convert to the kernel's parameter types (const void* -> const TI*)
template <typename... KA, typename... A>
int launch(void (*kern)(KA...), dim3 grid, size_t lds, hipStream_t st, A... args) {
  if (lds > 160 * 1024) return SBK_ERR_ARG;
  if (sbk::lds_optin((const void*)kern, lds) != hipSuccess) return SBK_ERR_ARG;
  hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, st, static_cast<KA>(args)...);
  SBK_CHECK_LAUNCH();
  return 0;
}

bool bad_dims(int B, int Lq, int Lk, int H, int dh, int P) {
  return B <= 0 || Lq <= 0 || Lk <= 0 || H <= 0 || dh <= 0 || dh > 256 || P < Lk || Lq > 65535 || Lk > 65535 ||
         H > 65535 || B > 65535 || P > 65535 * 2;
}

// the validated arguments of the two entry points, in the order of their C signatures
struct FwdArgs {
  const void *q; int ldq; const void* k; int ldk; const void* v; int ldv; const void* pk; int ldp, P;
  const float *pbu, *pbv; const unsigned char* kpm; const float* am; long long am_sb, am_sh;
  int B, Lq, Lk, H, dh; float scale; int mpf; float p; unsigned long long seed;
  void* out; int ldo; float *probs, *attn; hipStream_t st;
};
struct BwdArgs {
  const void *q; int ldq; const void* k; int ldk; const void* v; int ldv; const void* pk; int ldp, P;
  const float *pbu, *pbv, *probs; const void* dO; int lddo, B, Lq, Lk, H, dh; float scale; int mpf; float p;
  unsigned long long seed; float *G, *dqu, *dqv, *dq, *dk, *dv, *dpk; hipStream_t st;
};

template <typename TI>
int xattn_fwd(const FwdArgs& a) {
  const Dropout drop(a.p, a.seed);
  if (drop.use && !a.attn) return SBK_ERR_ARG;
  const size_t lq = fwd_qb_lds(a.dh, a.Lk, a.pk != nullptr).bytes();
  const bool qb = a.Lk <= XQ_LKMAX && lq <= 160 * 1024 &&
                  (a.pk ? qb_aligned<TI>({a.q, a.k, a.v, a.pk}, {a.ldq, a.ldk, a.ldv, a.ldp}, a.dh)
                        : qb_aligned<TI>({a.q, a.k, a.v}, {a.ldq, a.ldk, a.ldv}, a.dh));
  const auto kern = !qb ? xattn_fwd_kernel<TI> : a.pk ? xattn_fwd_qb_kernel<TI, true> : xattn_fwd_qb_kernel<TI, false>;
  return launch(kern, dim3(qb ? (a.Lq + XQ_QB - 1) / XQ_QB : a.Lq, a.H, a.B), qb ? lq : row_lds(a.Lk, a.dh).bytes(),
                a.st, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, a.pk, a.ldp, a.P, a.pbu, a.pbv, a.mpf, a.kpm, a.am, a.am_sb,
                a.am_sh, a.Lq, a.Lk, a.H, a.dh, a.scale, drop, a.out, a.ldo, a.probs, a.attn);
}

template <typename TI>
int xattn_bwd(const BwdArgs& a) {
  const Dropout drop(a.p, a.seed);
  const dim3 per_q(a.Lq, a.H, a.B), blk_q((a.Lq + XQ_QB - 1) / XQ_QB, a.H, a.B);
  const bool rows_qb = a.Lk <= XQ_LKMAX && qb_aligned<TI>({a.k, a.v, a.dO}, {a.ldk, a.ldv, a.lddo}, a.dh);
  if (int rc = launch(rows_qb ? xattn_bwd_rows_qb_kernel<TI> : xattn_bwd_rows_kernel<TI>, rows_qb ? blk_q : per_q,
                      rows_qb ? bwd_rows_qb_lds(a.dh, a.Lk).bytes() : row_lds(a.Lk, a.dh).bytes(), a.st, a.k, a.ldk,
                      a.v, a.ldv, a.dO, a.lddo, a.probs, a.Lq, a.Lk, a.H, a.dh, a.scale, drop, a.G,
                      a.pk ? a.dqu : a.dq))
    return rc;
  if (a.pk) {
    const bool qv_qb = qb_aligned<TI>({a.pk}, {a.ldp}, a.dh);
    if (int rc = launch(qv_qb ? xattn_bwd_qv_qb_kernel<TI> : xattn_bwd_qv_kernel<TI>, qv_qb ? blk_q : per_q,
                        qv_qb ? bwd_qv_qb_lds(a.dh).bytes() : bwd_qv_lds(a.P).bytes(), a.st, a.pk, a.ldp, a.P, a.G,
                        a.dqu, a.Lq, a.Lk, a.H, a.dh, a.mpf, a.dqv, a.dq))
      return rc;
  }
  const bool kv_qb = qb_aligned<TI>({a.q, a.dO}, {a.ldq, a.lddo}, a.dh);
  if (int rc = launch(kv_qb ? xattn_bwd_kv_qb_kernel<TI> : xattn_bwd_kv_kernel<TI>,
                      dim3(kv_qb ? (a.Lk + XQ_QB - 1) / XQ_QB : a.Lk, a.H, a.B),
                      kv_qb ? bwd_kv_qb_lds(a.dh).bytes() : bwd_kv_lds(a.Lq).bytes(), a.st, a.q, a.ldq, a.dO, a.lddo,
                      a.pbu, a.probs, a.G, a.Lq, a.Lk, a.H, a.dh, drop, a.dk, a.dv))
    return rc;
  if (a.pk)  // (a column-blocked variant over 188 workgroups measured 2x slower: 550 vs 276 us)
    return launch(xattn_bwd_pk_kernel<TI>, dim3(a.P, a.H, 1), bwd_pk_lds(a.Lq).bytes(), a.st, a.q, a.ldq, a.pbv, a.G,
                  a.B, a.Lq, a.Lk, a.H, a.dh, a.P, a.mpf, a.dpk);
  return 0;
}

}  // namespace

SBK_API int sbk_relpos_xattn_fwd(int dtype_bf16, const void* q, int ldq, const void* k, int ldk, const void* v,
                                 int ldv, const void* pk, int ldp, int P, const float* pbu, const float* pbv,
                                 const unsigned char* kpm, const float* am, long long am_sb, long long am_sh, int B,
                                 int Lq, int Lk, int H, int dh, float scale, int mask_pos_future, float p_drop,
                                 unsigned long long seed, void* out, int ldo, float* probs, float* attn,
                                 void* stream) {
  if (!q || !k || !v || (pk && (!pbu || !pbv || ldp < H * dh)) || !out || !probs || bad_dims(B, Lq, Lk, H, dh, P) ||
      p_drop < 0.f || p_drop >= 1.f || ldq < H * dh || ldk < H * dh || ldv < H * dh || ldo < H * dh)
    return SBK_ERR_ARG;
  const FwdArgs a{q, ldq, k, ldk, v, ldv, pk, ldp, P, pbu, pbv, kpm, am, am_sb, am_sh, B, Lq, Lk, H, dh, scale,
                  mask_pos_future, p_drop, seed, out, ldo, probs, attn, (hipStream_t)stream};
  return dtype_bf16 ? xattn_fwd<uint16_t>(a) : xattn_fwd<float>(a);
}

SBK_API int sbk_relpos_xattn_bwd(int dtype_bf16, const void* q, int ldq, const void* k, int ldk, const void* v,
                                 int ldv, const void* pk, int ldp, int P, const float* pbu, const float* pbv,
                                 const float* probs, const void* dO, int lddo, int B, int Lq, int Lk, int H, int dh,
                                 float scale, int mask_pos_future, float p_drop, unsigned long long seed, float* G,
                                 float* dqu, float* dqv, float* dq, float* dk, float* dv, float* dpk, void* stream) {
  if (!q || !k || !v || !probs || !dO || !G || !dq || !dk || !dv ||
      (pk && (!pbu || !pbv || !dqu || !dqv || !dpk || ldp < H * dh)) || bad_dims(B, Lq, Lk, H, dh, P) ||
      p_drop < 0.f || p_drop >= 1.f || ldq < H * dh || ldk < H * dh || ldv < H * dh || lddo < H * dh)
    return SBK_ERR_ARG;
  const BwdArgs a{q, ldq, k, ldk, v, ldv, pk, ldp, P, pbu, pbv, probs, dO, lddo, B, Lq, Lk, H, dh, scale,
                  mask_pos_future, p_drop, seed, G, dqu, dqv, dq, dk, dv, dpk, (hipStream_t)stream};
  return dtype_bf16 ? xattn_bwd<uint16_t>(a) : xattn_bwd<float>(a);
}
