// Attentional GRU decoder steps (nnet/RNN.py:713-958 of the reference with
// rnn_type "gru", one layer; nnet/attention.py:23-234, content-based and
// location-aware attention).
//
//   cell   x_t = [inp_t | c_{t-1}] (dropout mask applied), torch.nn.GRUCell gates
//   query  dech = h_t W_dec^T + (b_dec + b_loc)
//   score  e[l][f] = P[l][f] + dech[f] + sum_c W_loc[f][c] F[l][c],  P = enc W_enc^T + b_enc
//          F[l][c] = sum_j w_conv[c][j] prev_attn[l - k + j]          (location only)
//          s[l] = scaling * sum_f w_attn[f] tanh(e[l][f]),  -inf at l >= enc_len
//   attn = softmax(s);  ctx = attn . enc;  c_t = ctx W_out^T + b_out
//
// Forward, five launches per step, stream order between them, nothing
// persistent, no flag between workgroups, no float atomics:
//   1 cell    rnnstep.h skeleton: two products (c_{t-1} against W_ih[:, I:],
//             K = O; h_{t-1} against W_hh, K = H) meet as four tiles (r and z
//             summed per wave, the n gate's two halves apart) in one epilogue
//   2 query   skeleton, one tile
//   3 score   grid (ceil(L / 32), B), 256 threads.  The workgroup stages the
//             taps, the window of prev_attn around its 32 frames and the
//             location features F in LDS; wave w takes the 16-column tiles
//             w, w + 4, .. of attn_dim for all 32 frames: the C-contraction on
//             exact-fp32 MFMA (16x16x4, k = 4 s + lane group, so C = 10 costs
//             three instructions), P streamed once, tanh, the w_attn-weighted
//             column sum.  Then the tile's softmax share, flash style: tile
//             maximum m, p = exp(s - m), their sum, and sum_l p[l] enc[l, :].
//             e, tanh(e) and the location features never reach memory.
//   4 combine one workgroup per row joins the tile partials in tile order,
//             writes attn[b, t, :] (zero at padded frames) and ctx[b, t, :]
//   5 cproj   skeleton, one tile: c_t, and c_t times the next step's dropout mask
//
// Backward step t = T-1 .. 0, five launches:
//   1 dc      dC_t += m_c[t+1] * (dgi_{t+1} W_ih[:, I:])            (t < T-1)
//   2 dctx    dctx_t = dC_t W_out
//   3 score   same grid and staging as the forward score kernel; recomputes
//             F, e, tanh(e) from attn[t-1], dech[t], P; dalpha = dctx . enc +
//             dattn, the softmax row term from the saved ctx (no cross-tile
//             reduction), ds, de; dP += de (one owner per element), the tile's
//             share of d dech, and this workgroup's slot of the dw_attn, dW_loc
//             (de^T F on MFMA) and dw_conv (through dF = de W_loc on MFMA) sums
//   4 tilesum d dech_t = sum over tiles, in tile order
//   5 cell    dh_t = dH_t + z_{t+1} dh_{t+1} + dgh_{t+1} W_hh + d dech_t W_dec,
//             then the gate gradients dgi_t, dgh_t as gru.hip's backward
// prev_attn is detached in the reference: nothing flows through F into earlier
// steps.  The slot sums are reduced once after the loop by the caller.
//
// bf16 mode: W_ih[:, I:], W_hh, W_dec, W_out (and their transposes) are bf16 and
// the fp32 state operand is rounded at the MFMA; everything else, the W_loc F
// contraction included, is fp32 in both modes.
#include "rnnstep.h"

using namespace sbk;
using namespace sbk::rnnstep;

namespace {

constexpr int kLT = 32;            // frames of a score workgroup
constexpr int kST = 256;           // its threads
constexpr int kSW = kST / 64;      // its waves
constexpr int kLMT = kLT / 16;     // its MFMA row tiles
constexpr int kCT = 4;             // 16-channel tiles the score backward holds: C <= 64

// acc[m][0] += X[b0 + 16 m .., :K] . W[j0 .., :K]^T, this wave's share of K: the
// one-tile form of rnnstep.h's product (see gru.hip's backward), adding onto acc
template <typename T>
__device__ __forceinline__ void product1(f32x4 (&acc)[kMT][1], const T* W, int K, const float* X, long long ldx,
                                         int j0, int b0, int B, int N, int mts, bool vec_w, bool vec_x, int lane,
                                         int w) {
  const int unit = j0 + (lane & 15);
#pragma unroll 2
  for (int k0 = w * 32; k0 < K; k0 += kWaves * 32) {
    const int kk = k0 + 8 * (lane >> 4);
    const typename MT<T>::frag bw = unit < N ? load_w8<T>(W + (long long)unit * K, kk, K, vec_w) : MT<T>::zero();
#pragma unroll
    for (int m = 0; m < kMT; ++m) {
      if (m < mts) {
        const int row = b0 + m * 16 + (lane & 15);
        const typename MT<T>::frag af = row < B ? load_f8<T>(X + row * ldx, kk, K, vec_x) : MT<T>::zero();
        MT<T>::mma(acc[m][0], af, bw);
      }
    }
  }
}

struct Dims {
  int B, T, L, H, A, O, E, C, ksz, nt;
};

// ---------------------------------------------------------------- forward
struct FwdArgs {
  const void *w_ic, *w_hh, *w_dec, *w_out;   // (3H, O), (3H, H), (A, H), (O, E) in the compute dtype
  const float *b_hh, *b_q, *b_out;           // (3H), (A), (O) or null
  const float *gx, *mc;                      // (B, T, 3H); (B, T, O) or null
  const float *P, *enc;                      // (B, L, A), (B, L, E)
  const int* enc_len;                        // (B)
  const float *w_conv, *w_loc, *w_attn;      // (C, 2k+1), (A, C) or null; (A)
  const float *h0, *c0, *attn0;              // (B, H), (B, O), (B, L) or null
  float *hstate, *cstate, *ctx, *attn, *dech, *save;  // (B, T, H | O | E | L | A | 4H)
  float *cdrop, *scores, *ms, *pctx;         // (B, O), (B, L), (B, nt, 2), (B, nt, E)
  float scaling;
  Dims d;
  int vec_ic, vec_hh, vec_dec, vec_out, vec_c, vec_h, vec_x;
};

template <typename T>
__global__ void __launch_bounds__(kThreads) cell_fwd_kernel(FwdArgs a, int t) {
  __shared__ float red[kWaves][4][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.d.H, B = a.d.B, Tn = a.d.T, O = a.d.O;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const float* hprev = t == 0 ? a.h0 : a.hstate + (long long)(t - 1) * H;
  const long long ldh = t == 0 ? H : (long long)Tn * H;
  const float* cprev = t == 0 ? a.c0 : (a.mc ? a.cdrop : a.cstate + (long long)(t - 1) * O);
  const long long ldc = (t == 0 || a.mc) ? O : (long long)Tn * O;

  f32x4 ai[kMT][3], ah[kMT][3], acc[kMT][4];
  product<T, 3>(ai, static_cast<const T*>(a.w_ic), H, O, cprev, ldc, j0, b0, B, H, mts, a.vec_ic, a.vec_c, lane, w);
  product<T, 3>(ah, static_cast<const T*>(a.w_hh), H, H, hprev, ldh, j0, b0, B, H, mts, a.vec_hh, a.vec_h, lane, w);
#pragma unroll
  for (int m = 0; m < kMT; ++m) {
    acc[m][0] = ai[m][0] + ah[m][0];
    acc[m][1] = ai[m][1] + ah[m][1];
    acc[m][2] = ai[m][2];
    acc[m][3] = ah[m][2];
  }
  meet<4>(red, acc, mts, lane, w);

  const long long H3 = 3LL * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    float s[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) s[g] = total<4>(red, g, rr, jj);
    const float br = a.b_hh ? a.b_hh[j] : 0.f, bz = a.b_hh ? a.b_hh[H + j] : 0.f, bn = a.b_hh ? a.b_hh[2 * H + j] : 0.f;
    const long long bt = (long long)b * Tn + t;
    const float* gx = a.gx + bt * H3;
    const float hp = hprev ? hprev[b * ldh + j] : 0.f;
    const float r = sigmoid_exact(gx[j] + (s[0] + br));
    const float z = sigmoid_exact(gx[H + j] + (s[1] + bz));
    const float q = s[3] + bn;
    const float n = tanhf(gx[2 * H + j] + s[2] + r * q);
    a.hstate[bt * H + j] = (1.f - z) * n + z * hp;
    if (a.save) {
      float* sv = a.save + bt * 4 * H + j;
      sv[0] = r;
      sv[H] = z;
      sv[2 * H] = n;
      sv[3 * H] = q;
    }
  }
}

// out[b, :] = X[b, :K] . W^T + bias over the N rows of W, one tile per workgroup
template <typename T>
__device__ __forceinline__ void tile_rows(float (&red)[kWaves][1][kRows][kSlice], f32x4 (&acc)[kMT][1], const T* W,
                                          int K, const float* X, long long ldx, int B, int N, bool vec_w, bool vec_x,
                                          int& nrows) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
#pragma unroll
  for (int m = 0; m < kMT; ++m) acc[m][0] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (X) product1<T>(acc, W, K, X, ldx, j0, b0, B, N, mts, vec_w, vec_x, lane, w);
  meet<1>(red, acc, mts, lane, w);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) query_kernel(FwdArgs a, int t) {
  __shared__ float red[kWaves][1][kRows][kSlice];
  f32x4 acc[kMT][1];
  const int H = a.d.H, A = a.d.A, Tn = a.d.T;
  int nrows;
  tile_rows<T>(red, acc, static_cast<const T*>(a.w_dec), H, a.hstate + (long long)t * H, (long long)Tn * H, a.d.B, A,
               a.vec_dec, a.vec_h, nrows);
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  for (int e = threadIdx.x; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, j = j0 + (e & 15);
    if (j >= A) continue;
    const float s = total<1>(red, 0, rr, e & 15);
    a.dech[((long long)(b0 + rr) * Tn + t) * A + j] = a.b_q ? s + a.b_q[j] : s;
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) cproj_kernel(FwdArgs a, int t) {
  __shared__ float red[kWaves][1][kRows][kSlice];
  f32x4 acc[kMT][1];
  const int O = a.d.O, E = a.d.E, Tn = a.d.T;
  int nrows;
  tile_rows<T>(red, acc, static_cast<const T*>(a.w_out), E, a.ctx + (long long)t * E, (long long)Tn * E, a.d.B, O,
               a.vec_out, a.vec_x, nrows);
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  for (int e = threadIdx.x; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, j = j0 + (e & 15), b = b0 + rr;
    if (j >= O) continue;
    const float s = total<1>(red, 0, rr, e & 15);
    const float c = a.b_out ? s + a.b_out[j] : s;
    const long long bt = (long long)b * Tn + t;
    a.cstate[bt * O + j] = c;
    if (a.mc && t + 1 < Tn) a.cdrop[(long long)b * O + j] = c * a.mc[(bt + 1) * O + j];
  }
}

// ---- what the score kernels share: the staging of taps, window and location
// features, and the e tile of one 16-column slice of attn_dim

struct ScoreLds {
  float *taps, *win, *F;  // [C][2k+1], [kLT + 2k], [kLT][Cq]
  int Cq, KW;
};

__host__ __device__ inline int cq_of(int C) { return (C + 3) & ~3; }
// floats of the staging area
__host__ __device__ inline int stage_floats(int C, int ksz) {
  return C ? C * (2 * ksz + 1) + (kLT + 2 * ksz) + kLT * cq_of(C) : 0;
}

__device__ __forceinline__ ScoreLds carve(float* base, int C, int ksz) {
  ScoreLds s;
  s.KW = 2 * ksz + 1;
  s.Cq = cq_of(C);
  s.taps = base;
  s.win = s.taps + C * s.KW;
  s.F = s.win + kLT + 2 * ksz;
  return s;
}

// taps and the window prev[l0 - k .. l0 + kLT + k) (zero outside [0, L)), then
// F[l][c] for the tile's frames; columns C .. Cq of F are zero
__device__ __forceinline__ void stage_location(const ScoreLds& s, const float* w_conv, const float* prev, int l0, int L,
                                               int C, int ksz) {
  const int tid = threadIdx.x;
  for (int i = tid; i < C * s.KW; i += kST) s.taps[i] = w_conv[i];
  for (int i = tid; i < kLT + 2 * ksz; i += kST) {
    const int f = l0 - ksz + i;
    s.win[i] = f >= 0 && f < L ? prev[f] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < kLT * s.Cq; i += kST) {
    const int c = i / kLT, l = i - c * kLT;
    float acc = 0.f;
    if (c < C && l0 + l < L) {
      // taps that meet frames inside [0, L)
      const int lo = ksz - l0 - l > 0 ? ksz - l0 - l : 0;
      const int hi = L - 1 - l0 - l + ksz < 2 * ksz ? L - 1 - l0 - l + ksz : 2 * ksz;
      const float* tp = s.taps + c * s.KW;
      for (int j = lo; j <= hi; ++j) acc += tp[j] * s.win[l + j];
    }
    s.F[l * s.Cq + c] = acc;
  }
  __syncthreads();
}

// e[m][r] of frames l0 + 16 m + 4 (lane >> 4) + r, column f = 16 ft + (lane & 15):
// the location term on exact-fp32 MFMA (instruction s takes k = 4 s + lane
// group), plus P and dech; zero for a frame past len or a column past A
__device__ __forceinline__ void e_tile(f32x4 (&e)[kLMT], const ScoreLds& s, const float* w_loc, const float* Prow,
                                       const float* dech, int ft, int l0, int len, int A, int C, int lane) {
  const int f = ft * 16 + (lane & 15), g = lane >> 4;
#pragma unroll
  for (int m = 0; m < kLMT; ++m) e[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (w_loc) {
    for (int k = g; k < s.Cq; k += 4) {
      const float bw = f < A && k < C ? w_loc[(long long)f * C + k] : 0.f;
#pragma unroll
      for (int m = 0; m < kLMT; ++m)
        e[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(s.F[(m * 16 + (lane & 15)) * s.Cq + k], bw, e[m], 0, 0, 0);
    }
  }
  const float dq = f < A ? dech[f] : 0.f;
#pragma unroll
  for (int m = 0; m < kLMT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + m * 16 + 4 * g + r;
      e[m][r] = f < A && l < len ? e[m][r] + Prow[(long long)l * A + f] + dq : 0.f;
    }
}

// sum over the 16 lanes that share lane >> 4 (the columns of an MFMA tile row)
__device__ __forceinline__ float row16_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

__global__ void __launch_bounds__(kST) score_fwd_kernel(FwdArgs a, int t) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  const int L = a.d.L, A = a.d.A, E = a.d.E, C = a.w_loc ? a.d.C : 0, Tn = a.d.T, nt = a.d.nt;
  const int tile = blockIdx.x, b = blockIdx.y, l0 = tile * kLT;
  int len = a.enc_len[b];
  len = len < 0 ? 0 : (len > L ? L : len);
  const ScoreLds s = carve(lds, C, a.d.ksz);
  float* sred = lds + stage_floats(C, a.d.ksz);  // [kSW][kLT]
  float* sc = sred + kSW * kLT;                  // [kLT] scores, then p
  if (C) {
    const float* prev = t == 0 ? a.attn0 + (long long)b * L : a.attn + ((long long)b * Tn + t - 1) * L;
    stage_location(s, a.w_conv, prev, l0, L, C, a.d.ksz);
  }
  const float* Prow = a.P + (long long)b * L * A;
  const float* dech = a.dech + ((long long)b * Tn + t) * A;
  float sp[kLMT][4] = {};
  for (int ft = w; ft * 16 < A; ft += kSW) {
    f32x4 e[kLMT];
    e_tile(e, s, a.w_loc, Prow, dech, ft, l0, len, A, C, lane);
    const int f = ft * 16 + (lane & 15);
    const float wa = f < A ? a.w_attn[f] : 0.f;
#pragma unroll
    for (int m = 0; m < kLMT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) sp[m][r] += wa * tanhf(e[m][r]);
  }
#pragma unroll
  for (int m = 0; m < kLMT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = row16_sum(sp[m][r]);
      if ((lane & 15) == 0) sred[w * kLT + m * 16 + 4 * g + r] = v;
    }
  __syncthreads();
  if (tid < kLT) {
    float v = sred[tid];
#pragma unroll
    for (int ww = 1; ww < kSW; ++ww) v += sred[ww * kLT + tid];
    v = l0 + tid < len ? a.scaling * v : -INFINITY;
    sc[tid] = v;
    if (l0 + tid < L) a.scores[(long long)b * L + l0 + tid] = v;
  }
  __syncthreads();
  float mx = sc[0];
#pragma unroll
  for (int l = 1; l < kLT; ++l) mx = fmaxf(mx, sc[l]);
  __syncthreads();
  if (tid < kLT) sc[tid] = l0 + tid < len ? expf(sc[tid] - mx) : 0.f;
  __syncthreads();
  if (tid == 0) {
    float sum = 0.f;
    for (int l = 0; l < kLT; ++l) sum += sc[l];
    float* o = a.ms + ((long long)b * nt + tile) * 2;
    o[0] = mx;
    o[1] = sum;
  }
  const int nl = len - l0 < kLT ? len - l0 : kLT;
  const float* en = a.enc + ((long long)b * L + l0) * E;
  for (int e = tid; e < E; e += kST) {
    float acc = 0.f;
    for (int l = 0; l < nl; ++l) acc += sc[l] * en[(long long)l * E + e];
    a.pctx[((long long)b * nt + tile) * E + e] = acc;
  }
}

__global__ void __launch_bounds__(kST) combine_kernel(FwdArgs a, int t) {
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = a.d.L, E = a.d.E, Tn = a.d.T, nt = a.d.nt;
  int len = a.enc_len[b];
  len = len < 0 ? 0 : (len > L ? L : len);
  const float* ms = a.ms + (long long)b * nt * 2;
  float M = ms[0];
  for (int i = 1; i < nt; ++i) M = fmaxf(M, ms[2 * i]);
  float S = 0.f;
  for (int i = 0; i < nt; ++i)
    if (ms[2 * i + 1] > 0.f) S += ms[2 * i + 1] * expf(ms[2 * i] - M);
  const float inv = 1.f / S;
  const long long bt = (long long)b * Tn + t;
  for (int l = tid; l < L; l += kST) a.attn[bt * L + l] = l < len ? expf(a.scores[(long long)b * L + l] - M) * inv : 0.f;
  for (int e = tid; e < E; e += kST) {
    float acc = 0.f;
    for (int i = 0; i < nt; ++i)
      if (ms[2 * i + 1] > 0.f) acc += a.pctx[((long long)b * nt + i) * E + e] * expf(ms[2 * i] - M);
    a.ctx[bt * E + e] = acc * inv;
  }
}

// --------------------------------------------------------------- backward
struct BwdArgs {
  const void *w_icT, *w_hhT, *w_decT, *w_outT;  // (O, 3H), (H, 3H), (H, A), (E, O) in the compute dtype
  const float *P, *enc;
  const int* enc_len;
  const float *w_conv, *w_loc, *w_attn;
  const float *h0, *attn0, *mc;
  const float *hstate, *ctx, *attn, *dech, *save;
  const float *dattn, *dhproj;                  // (B, T, L) or null; (B, T, H)
  float *dcall, *dgi, *dgh, *dctx, *dP, *ddech; // (B, T, O | 3H | 3H | E), (B, L, A), (B, T, A)
  float *slots;                                 // (B * nt, A + A * C + C * (2k+1))
  float *dhw, *ddp;                             // (2, B, H), (B, nt, A)
  float scaling;
  Dims d;
  int vec_icT, vec_hhT, vec_decT, vec_outT, vec_g, vec_a, vec_o;
};

// dC_t[:, J] += m_c[t+1] * (dgi_{t+1} . W_ih[:, I + J])
template <typename T>
__global__ void __launch_bounds__(kThreads) dc_kernel(BwdArgs a, int t) {
  __shared__ float red[kWaves][1][kRows][kSlice];
  f32x4 acc[kMT][1];
  const int O = a.d.O, Tn = a.d.T, K = 3 * a.d.H;
  int nrows;
  tile_rows<T>(red, acc, static_cast<const T*>(a.w_icT), K, a.dgi + (long long)(t + 1) * K, (long long)Tn * K, a.d.B, O,
               a.vec_icT, a.vec_g, nrows);
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  for (int e = threadIdx.x; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, j = j0 + (e & 15);
    if (j >= O) continue;
    const long long bt = (long long)(b0 + rr) * Tn + t;
    const float s = total<1>(red, 0, rr, e & 15);
    a.dcall[bt * O + j] += a.mc ? s * a.mc[(bt + 1) * O + j] : s;
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) dctx_kernel(BwdArgs a, int t) {
  __shared__ float red[kWaves][1][kRows][kSlice];
  f32x4 acc[kMT][1];
  const int O = a.d.O, E = a.d.E, Tn = a.d.T;
  int nrows;
  tile_rows<T>(red, acc, static_cast<const T*>(a.w_outT), O, a.dcall + (long long)t * O, (long long)Tn * O, a.d.B, E,
               a.vec_outT, a.vec_o, nrows);
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  for (int e = threadIdx.x; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, j = j0 + (e & 15);
    if (j >= E) continue;
    a.dctx[((long long)(b0 + rr) * Tn + t) * E + j] = total<1>(red, 0, rr, e & 15);
  }
}

__global__ void __launch_bounds__(kST) score_bwd_kernel(BwdArgs a, int t) {
  extern __shared__ float lds[];
  __shared__ float red16[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  const int L = a.d.L, A = a.d.A, E = a.d.E, C = a.w_loc ? a.d.C : 0, Tn = a.d.T, nt = a.d.nt, ksz = a.d.ksz;
  const int tile = blockIdx.x, b = blockIdx.y, l0 = tile * kLT;
  int len = a.enc_len[b];
  len = len < 0 ? 0 : (len > L ? L : len);
  const ScoreLds s = carve(lds, C, ksz);
  float* ds = lds + stage_floats(C, ksz);   // [kLT]
  float* det = ds + kLT;                    // [kSW][kLT][16]: a wave's de tile
  float* dFr = det + kSW * kLT * 16;        // [kSW][kLT][16 kCT'] per-wave dF, then their sum in wave 0's part
  const int nct = (C + 15) >> 4, CW = nct * 16;
  if (C) {
    const float* prev = t == 0 ? a.attn0 + (long long)b * L : a.attn + ((long long)b * Tn + t - 1) * L;
    stage_location(s, a.w_conv, prev, l0, L, C, ksz);
  }
  const long long bt = (long long)b * Tn + t;
  const float* alpha = a.attn + bt * L;
  const float* dattn = a.dattn ? a.dattn + bt * L : nullptr;
  const float* dctx = a.dctx + bt * E;
  // the softmax row term: dctx . ctx_t + sum_l alpha dattn
  float part = 0.f;
  for (int e = tid; e < E; e += kST) part += dctx[e] * a.ctx[bt * E + e];
  if (dattn)
    for (int l = tid; l < len; l += kST) part += alpha[l] * dattn[l];
  const float rowterm = block_sum(part, red16);
  // dalpha of the tile's frames, 8 per wave, and ds
  for (int l = w; l < kLT; l += kSW) {
    const int fr = l0 + l;
    float v = 0.f;
    if (fr < len) {
      const float* en = a.enc + ((long long)b * L + fr) * E;
      for (int e = lane; e < E; e += 64) v += dctx[e] * en[e];
    }
    v = wave_sum(v);
    if (lane == 0) ds[l] = fr < len ? a.scaling * alpha[fr] * (v + (dattn ? dattn[fr] : 0.f) - rowterm) : 0.f;
  }
  __syncthreads();

  const float* Prow = a.P + (long long)b * L * A;
  float* dProw = a.dP + (long long)b * L * A;
  const float* dech = a.dech + bt * A;
  float* slot = a.slots + ((long long)b * nt + tile) * ((long long)A + (long long)A * a.d.C + (long long)a.d.C * (2 * ksz + 1));
  float* s_attn = slot;
  float* s_loc = slot + A;
  float* s_conv = s_loc + (long long)A * a.d.C;
  float* ddp = a.ddp + ((long long)b * nt + tile) * A;
  float* my = det + w * kLT * 16;
  f32x4 dF[kLMT][kCT];
#pragma unroll
  for (int m = 0; m < kLMT; ++m)
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct) dF[m][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nft = (A + 15) >> 4, nround = (nft + kSW - 1) / kSW;
  for (int rd = 0; rd < nround; ++rd) {   // every wave runs every round: the barriers below are uniform
    const int ft = rd * kSW + w;
    const int f = ft * 16 + (lane & 15);
    f32x4 e[kLMT];
    e_tile(e, s, a.w_loc, Prow, dech, ft, l0, len, A, C, lane);
    const float wa = f < A ? a.w_attn[f] : 0.f;
    float cs = 0.f, ca = 0.f;
#pragma unroll
    for (int m = 0; m < kLMT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int l = m * 16 + 4 * g + r;
        const float th = tanhf(e[m][r]);
        const float de = ds[l] * wa * (1.f - th * th);
        ca += ds[l] * th;
        cs += de;
        if (f < A && l0 + l < len) dProw[(long long)(l0 + l) * A + f] += de;
        if (C) my[l * 16 + (lane & 15)] = de;
      }
    cs += __shfl_xor(cs, 16);
    cs += __shfl_xor(cs, 32);
    ca += __shfl_xor(ca, 16);
    ca += __shfl_xor(ca, 32);
    if (g == 0 && f < A) {
      ddp[f] = cs;
      s_attn[f] += ca;
    }
    if (C) {
      __syncthreads();
      // dW_loc[f][c] += sum_l de[l][f] F[l][c]: rows f, K = the tile's frames
      for (int ct = 0; ct < nct; ++ct) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const int c = ct * 16 + (lane & 15);
#pragma unroll
        for (int k = 0; k < kLT; k += 4)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(my[(k + g) * 16 + (lane & 15)],
                                                     c < s.Cq ? s.F[(k + g) * s.Cq + c] : 0.f, acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int fo = ft * 16 + 4 * g + r;
          if (fo < A && c < C) s_loc[(long long)fo * C + c] += acc[r];
        }
      }
      // dF[l][c] += sum_f de[l][f] W_loc[f][c]: rows l, K = the 16 columns of this slice
#pragma unroll
      for (int ct = 0; ct < kCT; ++ct) {
        if (ct < nct) {
          const int c = ct * 16 + (lane & 15);
#pragma unroll
          for (int k = 0; k < 16; k += 4) {
            const int fk = ft * 16 + k + g;
            const float bw = fk < A && c < C ? a.w_loc[(long long)fk * C + c] : 0.f;
#pragma unroll
            for (int m = 0; m < kLMT; ++m)
              dF[m][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(my[(m * 16 + (lane & 15)) * 16 + k + g], bw, dF[m][ct], 0,
                                                               0, 0);
          }
        }
      }
      __syncthreads();
    }
  }
  if (C) {
    // the waves' dF meet, are added in wave order, and meet the window: dw_conv
    float* mine = dFr + w * kLT * CW;
#pragma unroll
    for (int m = 0; m < kLMT; ++m)
#pragma unroll
      for (int ct = 0; ct < kCT; ++ct)
        if (ct < nct)
#pragma unroll
          for (int r = 0; r < 4; ++r) mine[(m * 16 + 4 * g + r) * CW + ct * 16 + (lane & 15)] = dF[m][ct][r];
    __syncthreads();
    for (int i = tid; i < kLT * CW; i += kST) {
      float v = dFr[i];
#pragma unroll
      for (int ww = 1; ww < kSW; ++ww) v += dFr[ww * kLT * CW + i];
      dFr[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < C * s.KW; i += kST) {
      const int c = i / s.KW, j = i - c * s.KW;
      float acc = 0.f;
      for (int l = 0; l < kLT; ++l) acc += dFr[l * CW + c] * s.win[l + j];
      s_conv[i] += acc;
    }
  }
}

// d dech_t = the tiles' shares added in tile order
__global__ void __launch_bounds__(256) tilesum_kernel(BwdArgs a, int t) {
  const int A = a.d.A, nt = a.d.nt, Tn = a.d.T;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.d.B * A) return;
  const int b = (int)(i / A), f = (int)(i - (long long)b * A);
  const float* p = a.ddp + (long long)b * nt * A + f;
  float v = p[0];
  for (int k = 1; k < nt; ++k) v += p[(long long)k * A];
  a.ddech[((long long)b * Tn + t) * A + f] = v;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) cell_bwd_kernel(BwdArgs a, int t) {
  __shared__ float red[kWaves][1][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.d.H, B = a.d.B, Tn = a.d.T, A = a.d.A;
  const int K = 3 * H;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const int s = t + 1;
  f32x4 acc[kMT][1];
#pragma unroll
  for (int m = 0; m < kMT; ++m) acc[m][0] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s < Tn)
    product1<T>(acc, static_cast<const T*>(a.w_hhT), K, a.dgh + (long long)s * K, (long long)Tn * K, j0, b0, B, H, mts,
                a.vec_hhT, a.vec_g, lane, w);
  product1<T>(acc, static_cast<const T*>(a.w_decT), A, a.ddech + (long long)t * A, (long long)Tn * A, j0, b0, B, H, mts,
              a.vec_decT, a.vec_a, lane, w);
  meet<1>(red, acc, mts, lane, w);

  const long long BH = (long long)B * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    const long long bj = (long long)b * H + j, bt = (long long)b * Tn + t;
    float dh = total<1>(red, 0, rr, jj) + a.dhproj[bt * H + j];
    if (s < Tn) dh += a.save[(bt + 1) * 4 * H + H + j] * a.dhw[(s & 1) * BH + bj];
    a.dhw[(t & 1) * BH + bj] = dh;
    const float* sv = a.save + bt * 4 * H + j;
    const float r = sv[0], z = sv[H], n = sv[2 * H], q = sv[3 * H];
    const float hp = t == 0 ? (a.h0 ? a.h0[bj] : 0.f) : a.hstate[(bt - 1) * H + j];
    float nn;
    {
#pragma clang fp contract(off)
      nn = n * n;
    }
    const float dn = dh * (1.f - z) * (1.f - nn);
    const float dz = dh * (hp - n) * z * (1.f - z);
    const float dr = dn * q * r * (1.f - r);
    float* gi = a.dgi + bt * K + j;
    float* gh = a.dgh + bt * K + j;
    gi[0] = dr;
    gi[H] = dz;
    gi[2 * H] = dn;
    gh[0] = dr;
    gh[H] = dz;
    gh[2 * H] = dn * r;
  }
}

// ------------------------------------------------- beam-grouped decode step
// One step over N = B * G hypotheses (row n = b * G + g) that share the B
// utterances' enc, P and enc_len.  Row n continues row parent[n] of the
// previous step: every per-row operand is read through parent from one buffer
// and written at n into the other, so a beam permutation moves no state.

constexpr int kGH = 16;   // hypotheses of a score workgroup: one MFMA row tile

struct BeamArgs {
  const void *w_ic, *w_hh;                    // (3H, O), (3H, H) in the compute dtype
  const float *b_hh, *gx;                     // (3H) or null; (V, 3H) table with token, else (N, 3H)
  const int* token;                           // (N) or null
  const float *P, *enc;                       // (B, L, A), (B, L, E)
  const int* enc_len;                         // (B)
  const float *w_conv, *w_loc, *w_attn;
  const int* parent;                          // (N)
  const float *h_prev, *c_prev, *attn_prev, *cov_prev;  // (N, H | O | L | L)
  const int* peak_prev;                       // (N)
  const float* dech;                          // (N, A)
  float *h, *attn, *cov, *ctx, *pen;          // (N, H | L | L | E), (N)
  int *peak, *shift_ok;                       // (N)
  float *scores, *ms, *pctx;                  // (N, L), (N, nt, 2), (N, nt, E)
  float scaling;
  int first, max_shift, V;
  int B, G, N, L, H, A, O, E, C, ksz, nt;
  int vec_ic, vec_hh, vec_c, vec_h;
};

// the row that row n continues, held inside n's utterance
__device__ __forceinline__ int parent_row(const int* parent, int n, int G) {
  const int lo = n / G * G, p = parent[n];
  return p < lo ? lo : (p >= lo + G ? lo + G - 1 : p);
}

// rnnstep.h's product with the rows of X mapped: tile row 16 m + (lane & 15)
// reads X row src[m] (none when negative)
template <typename T, int G>
__device__ __forceinline__ void product_rows(f32x4 (&out)[kMT][G], const T* W, int gate_rows, int K, const float* X,
                                             long long ldx, const int (&src)[kMT], int j0, int H, int mts, bool vec_w,
                                             bool vec_x, int lane, int w) {
  f32x4 acc[kMT][G];
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int g = 0; g < G; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        const typename MT<T>::frag af = src[m] >= 0 ? load_f8<T>(X + src[m] * ldx, kk, K, vec_x) : MT<T>::zero();
#pragma unroll
        for (int g = 0; g < G; ++g) MT<T>::mma(acc[m][g], af, bw[g]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int g = 0; g < G; ++g) out[m][g] = acc[m][g];
}

// cell_fwd_kernel with h and c gathered through parent and the input half of
// the gates read from row token[n] of the (V, 3H) table
template <typename T>
__global__ void __launch_bounds__(kThreads) beam_cell_kernel(BeamArgs a) {
  __shared__ float red[kWaves][4][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, N = a.N, O = a.O;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = N - b0 < kRows ? N - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  int src[kMT];
#pragma unroll
  for (int m = 0; m < kMT; ++m) {
    const int row = b0 + m * 16 + (lane & 15);
    src[m] = row < N ? parent_row(a.parent, row, a.G) : -1;
  }
  f32x4 ai[kMT][3], ah[kMT][3], acc[kMT][4];
  product_rows<T, 3>(ai, static_cast<const T*>(a.w_ic), H, O, a.c_prev, O, src, j0, H, mts, a.vec_ic, a.vec_c, lane, w);
  product_rows<T, 3>(ah, static_cast<const T*>(a.w_hh), H, H, a.h_prev, H, src, j0, H, mts, a.vec_hh, a.vec_h, lane, w);
#pragma unroll
  for (int m = 0; m < kMT; ++m) {
    acc[m][0] = ai[m][0] + ah[m][0];
    acc[m][1] = ai[m][1] + ah[m][1];
    acc[m][2] = ai[m][2];
    acc[m][3] = ah[m][2];
  }
  meet<4>(red, acc, mts, lane, w);

  const long long H3 = 3LL * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int n = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    float s[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) s[g] = total<4>(red, g, rr, jj);
    const float br = a.b_hh ? a.b_hh[j] : 0.f, bz = a.b_hh ? a.b_hh[H + j] : 0.f, bn = a.b_hh ? a.b_hh[2 * H + j] : 0.f;
    int xrow = n;
    if (a.token) {
      const int v = a.token[n];
      xrow = v < 0 ? 0 : (v >= a.V ? a.V - 1 : v);
    }
    const float* gx = a.gx + xrow * H3;
    const float hp = a.h_prev[(long long)parent_row(a.parent, n, a.G) * H + j];
    const float r = sigmoid_exact(gx[j] + (s[0] + br));
    const float z = sigmoid_exact(gx[H + j] + (s[1] + bz));
    const float q = s[3] + bn;
    const float nn = tanhf(gx[2 * H + j] + s[2] + r * q);
    a.h[(long long)n * H + j] = (1.f - z) * nn + z * hp;
  }
}

// floats of the group's staging area: taps, kGH windows, kGH location-feature tiles
__host__ __device__ inline int beam_stage_floats(int C, int ksz) {
  return C ? C * (2 * ksz + 1) + kGH * (kLT + 2 * ksz) + kGH * kLT * cq_of(C) : 0;
}

// sum over the 16 lanes of an MFMA tile row on DPP row permutes (no LDS round trip)
__device__ __forceinline__ float row16_sum_v(float v) {
  v += dpp_f32<0x140>(v);
  v += dpp_f32<0x141>(v);
  v += dpp_f32<0x4E>(v);
  v += dpp_f32<0xB1>(v);
  return v;
}

// Grid (ceil(L / 32), B, ceil(G / kGH)).  The workgroup owns 32 frames of one
// utterance and up to kGH of its hypotheses.  Staged once: the taps; per
// hypothesis the prev_attn window of its parent row and its location features.
// Wave w walks the 16-column tiles w, w + 4, .. of attn_dim: per tile the P
// values, the W_loc fragment and w_attn are fetched once and kept in
// registers across the hypotheses' e tiles (the fp32 MFMA contraction of
// e_tile, + P + dech[n], tanh, the w_attn-weighted column sum, added into the
// wave's LDS slot of (hypothesis, frame)).  Then each hypothesis's softmax
// share, and the context partial (kGH x 32 probabilities) . (32 x E) on fp32
// MFMA: enc is read once per workgroup, the waves split E.
__global__ void __launch_bounds__(kST) beam_score_kernel(BeamArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  const int L = a.L, A = a.A, E = a.E, C = a.w_loc ? a.C : 0, nt = a.nt, ksz = a.ksz;
  const int tile = blockIdx.x, b = blockIdx.y, g0 = blockIdx.z * kGH, l0 = tile * kLT;
  const int gh = a.G - g0 < kGH ? a.G - g0 : kGH;
  const int n0 = b * a.G + g0;
  int len = a.enc_len[b];
  len = len < 0 ? 0 : (len > L ? L : len);
  const int KW = 2 * ksz + 1, Cq = cq_of(C), WW = kLT + 2 * ksz;
  float* taps = lds;                             // [C][KW]
  float* win = taps + C * KW;                    // [kGH][WW]
  float* F = win + kGH * WW;                     // [kGH][kLT][Cq]
  float* sred = lds + beam_stage_floats(C, ksz); // [kSW][kGH][kLT]
  float* sc = sred + kSW * kGH * kLT;            // [kGH][kLT] scores, then p
  for (int i = lane; i < kGH * kLT; i += 64) sred[w * kGH * kLT + i] = 0.f;
  if (C) {
    for (int i = tid; i < C * KW; i += kST) taps[i] = a.w_conv[i];
    for (int i = tid; i < gh * WW; i += kST) {
      const int gg = i / WW, x = i - gg * WW, f = l0 - ksz + x;
      const float* prev = a.attn_prev + (long long)parent_row(a.parent, n0 + gg, a.G) * L;
      win[i] = f >= 0 && f < L ? prev[f] : 0.f;
    }
    __syncthreads();
    const int per = kLT * Cq;
    for (int i = tid; i < kGH * per; i += kST) {
      const int gg = i / per, rem = i - gg * per;
      const int c = rem / kLT, l = rem - c * kLT;
      float acc = 0.f;
      if (gg < gh && c < C && l0 + l < L) {
        const int lo = ksz - l0 - l > 0 ? ksz - l0 - l : 0;
        const int hi = L - 1 - l0 - l + ksz < 2 * ksz ? L - 1 - l0 - l + ksz : 2 * ksz;
        const float* tp = taps + c * KW;
        const float* wn = win + gg * WW + l;
        for (int j = lo; j <= hi; ++j) acc += tp[j] * wn[j];
      }
      F[(gg * kLT + l) * Cq + c] = acc;
    }
  }
  __syncthreads();

  const float* Prow = a.P + (long long)b * L * A;
  const int nks = Cq >> 2;
  float* mine = sred + w * kGH * kLT;
  for (int ft = w; ft * 16 < A; ft += kSW) {
    const int f = ft * 16 + (lane & 15);
    const bool fin = f < A;
    float bw[4 * kCT];
#pragma unroll
    for (int s = 0; s < 4 * kCT; ++s) {
      const int k = 4 * s + g;
      bw[s] = s < nks && fin && k < C ? a.w_loc[(long long)f * C + k] : 0.f;
    }
    float pv[kLMT][4];
#pragma unroll
    for (int m = 0; m < kLMT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int l = l0 + m * 16 + 4 * g + r;
        pv[m][r] = fin && l < len ? Prow[(long long)l * A + f] : 0.f;
      }
    const float wa = fin ? a.w_attn[f] : 0.f;
    for (int gg = 0; gg < gh; ++gg) {
      f32x4 e[kLMT];
#pragma unroll
      for (int m = 0; m < kLMT; ++m) e[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* Fg = F + (gg * kLT + (lane & 15)) * Cq + g;
#pragma unroll
      for (int s = 0; s < 4 * kCT; ++s)
        if (s < nks) {
#pragma unroll
          for (int m = 0; m < kLMT; ++m)
            e[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(Fg[m * 16 * Cq + 4 * s], bw[s], e[m], 0, 0, 0);
        }
      const float dq = fin ? a.dech[(long long)(n0 + gg) * A + f] : 0.f;
#pragma unroll
      for (int m = 0; m < kLMT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = row16_sum_v(wa * tanhf(e[m][r] + pv[m][r] + dq));
          if ((lane & 15) == 0) mine[gg * kLT + m * 16 + 4 * g + r] += v;
        }
    }
  }
  __syncthreads();
  for (int i = tid; i < kGH * kLT; i += kST) {
    const int gg = i / kLT, l = i - gg * kLT;
    float v = sred[i];
#pragma unroll
    for (int ww = 1; ww < kSW; ++ww) v += sred[ww * kGH * kLT + i];
    v = gg < gh && l0 + l < len ? a.scaling * v : -INFINITY;
    sc[i] = v;
    if (gg < gh && l0 + l < L) a.scores[(long long)(n0 + gg) * L + l0 + l] = v;
  }
  __syncthreads();
  // a hypothesis's tile maximum, p = exp(s - m) and their sum: one wave per hypothesis, both halves alike
  for (int gg = w; gg < kGH; gg += kSW) {
    const int l = lane & (kLT - 1);
    const float s = sc[gg * kLT + l];
    float mx = s;
#pragma unroll
    for (int o = kLT / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float p = gg < gh && l0 + l < len ? expf(s - mx) : 0.f;
    float sum = p;
#pragma unroll
    for (int o = kLT / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane < kLT) sc[gg * kLT + l] = p;
    if (lane == 0 && gg < gh) {
      float* o = a.ms + ((long long)(n0 + gg) * nt + tile) * 2;
      o[0] = mx;
      o[1] = sum;
    }
  }
  __syncthreads();
  // rows = hypotheses, K = the tile's frames, columns = 16 of E
  float pa[kLT / 4];
#pragma unroll
  for (int s = 0; s < kLT / 4; ++s) pa[s] = sc[(lane & 15) * kLT + 4 * s + g];
  const float* en = a.enc + (long long)b * L * E;
  for (int et = w; et * 16 < E; et += kSW) {
    const int e = et * 16 + (lane & 15);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kLT / 4; ++s) {
      const int l = l0 + 4 * s + g;
      const float bv = e < E && l < len ? en[(long long)l * E + e] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s], bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gg = 4 * g + r;
      if (gg < gh && e < E) a.pctx[((long long)(n0 + gg) * nt + tile) * E + e] = acc[r];
    }
  }
}

// combine_kernel for row n, and in the same pass over the row: the first
// index of its maximum, the attention-shift condition against the parent's
// peak, the coverage cov_prev[parent] + attn (2 attn at the first step, as the
// reference initialises with the step's attention and then adds it) and the
// coverage penalty sum_l max(cov, 0.5) - 0.5 L
__global__ void __launch_bounds__(kST) beam_combine_kernel(BeamArgs a) {
  __shared__ float red16[16];
  __shared__ float bestv[kSW];
  __shared__ int besti[kSW];
  const int tid = threadIdx.x, n = blockIdx.x, b = n / a.G;
  const int L = a.L, E = a.E, nt = a.nt;
  int len = a.enc_len[b];
  len = len < 0 ? 0 : (len > L ? L : len);
  const int p = parent_row(a.parent, n, a.G);
  const float* ms = a.ms + (long long)n * nt * 2;
  float M = ms[0];
  for (int i = 1; i < nt; ++i) M = fmaxf(M, ms[2 * i]);
  float S = 0.f;
  for (int i = 0; i < nt; ++i)
    if (ms[2 * i + 1] > 0.f) S += ms[2 * i + 1] * expf(ms[2 * i] - M);
  const float inv = 1.f / S;
  float bv = -INFINITY, part = 0.f;
  int bi = 0x7fffffff;
  for (int l = tid; l < L; l += kST) {
    const float v = l < len ? expf(a.scores[(long long)n * L + l] - M) * inv : 0.f;
    a.attn[(long long)n * L + l] = v;
    const float cv = (a.first ? v : a.cov_prev[(long long)p * L + l]) + v;
    a.cov[(long long)n * L + l] = cv;
    part += fmaxf(cv, 0.5f);
    if (v > bv) {
      bv = v;
      bi = l;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    bestv[tid >> 6] = bv;
    besti[tid >> 6] = bi;
  }
  const float pen = block_sum(part, red16);   // its barriers publish bestv / besti
  if (tid == 0) {
    for (int ww = 1; ww < kSW; ++ww)
      if (bestv[ww] > bv || (bestv[ww] == bv && besti[ww] < bi)) {
        bv = bestv[ww];
        bi = besti[ww];
      }
    const int pk = bi < L ? bi : 0, pp = a.peak_prev[p];
    a.peak[n] = pk;
    a.shift_ok[n] = pk <= pp + a.max_shift && pk > pp - a.max_shift;
    a.pen[n] = pen - 0.5f * (float)L;
  }
  for (int e = tid; e < E; e += kST) {
    float acc = 0.f;
    for (int i = 0; i < nt; ++i)
      if (ms[2 * i + 1] > 0.f) acc += a.pctx[((long long)n * nt + i) * E + e] * expf(ms[2 * i] - M);
    a.ctx[(long long)n * E + e] = acc * inv;
  }
}

inline bool bad_dims(int B, int T, int L, int H, int A, int O, int E) {
  if (B <= 0 || T <= 0 || L <= 0 || H <= 0 || A <= 0 || O <= 0 || E <= 0 || B > 65535) return true;
  const long long lim = 0x7fffffffLL;
  return 3LL * H * H > lim || 3LL * H * O > lim || (long long)A * H > lim || (long long)O * E > lim ||
         (long long)B * T > lim / 4;
}

inline int vecw(const void* p, int K, int bf16) { return aligned16(p) && K % (bf16 ? 8 : 4) == 0; }
inline int vecx(const void* p, int K) { return (!p || aligned16(p)) && K % 4 == 0; }

template <typename Args>
inline int launch(void (*kernel)(Args, int), const Args& a, int N, int t, void* stream) {
  const dim3 grid((N + kSlice - 1) / kSlice, (a.d.B + kRows - 1) / kRows);
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, a, t);
  SBK_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// frames of a score workgroup: the tile count of the scratch sizes below is ceil(L / this)
SBK_API int sbk_attdec_tile() { return kLT; }

// See include/sbk.h.
SBK_API int sbk_attdec_fwd(int bf16, const void* w_ic, const void* w_hh, const float* b_hh, const void* w_dec,
                           const float* b_q, const void* w_out, const float* b_out, const float* gx, const float* mc,
                           const float* P, const float* enc, const int* enc_len, const float* w_conv,
                           const float* w_loc, const float* w_attn, float scaling, const float* h0, const float* c0,
                           const float* attn0, int B, int T, int L, int H, int A, int O, int E, int C, int ksz,
                           float* hstate, float* cstate, float* ctx, float* attn, float* dech, float* save, float* ws,
                           void* stream) {
  const bool cell = w_hh != nullptr;
  if (!w_dec || !w_out || !P || !enc || !enc_len || !w_attn || !hstate || !cstate || !ctx || !attn || !dech || !ws)
    return SBK_ERR_ARG;
  if (cell ? (!w_ic || !gx) : (T != 1 || w_ic || gx || mc)) return SBK_ERR_ARG;
  if (bad_dims(B, T, L, H, A, O, E)) return SBK_ERR_ARG;
  if (w_loc ? (!w_conv || !attn0 || C <= 0 || C > 16 * kCT || ksz < 0) : (w_conv != nullptr)) return SBK_ERR_ARG;
  const int Ck = w_loc ? C : 0, nt = (L + kLT - 1) / kLT;
  const size_t lds = sizeof(float) * ((size_t)stage_floats(Ck, ksz) + kSW * kLT + kLT);
  if (lds > 160 * 1024 - 1024) return SBK_ERR_ARG;
  if (lds > 64 * 1024)
    if (hipError_t e = lds_optin((const void*)score_fwd_kernel, lds)) return (int)e;
  FwdArgs a;
  a.w_ic = w_ic; a.w_hh = w_hh; a.w_dec = w_dec; a.w_out = w_out;
  a.b_hh = b_hh; a.b_q = b_q; a.b_out = b_out; a.gx = gx; a.mc = mc; a.P = P; a.enc = enc; a.enc_len = enc_len;
  a.w_conv = w_conv; a.w_loc = w_loc; a.w_attn = w_attn; a.h0 = h0; a.c0 = c0; a.attn0 = attn0;
  a.hstate = hstate; a.cstate = cstate; a.ctx = ctx; a.attn = attn; a.dech = dech; a.save = save;
  a.cdrop = ws;
  a.scores = a.cdrop + (size_t)B * O;
  a.ms = a.scores + (size_t)B * L;
  a.pctx = a.ms + (size_t)B * nt * 2;
  a.scaling = scaling;
  a.d = Dims{B, T, L, H, A, O, E, Ck, ksz, nt};
  a.vec_ic = w_ic && vecw(w_ic, O, bf16);
  a.vec_hh = w_hh && vecw(w_hh, H, bf16);
  a.vec_dec = vecw(w_dec, H, bf16);
  a.vec_out = vecw(w_out, E, bf16);
  a.vec_c = vecx(cstate, O) && vecx(c0, O) && vecx(ws, O);
  a.vec_h = vecx(hstate, H) && vecx(h0, H);
  a.vec_x = vecx(ctx, E);
  for (int t = 0; t < T; ++t) {
    if (cell)
      if (int rc = launch(bf16 ? cell_fwd_kernel<bf16_t> : cell_fwd_kernel<float>, a, H, t, stream)) return rc;
    if (int rc = launch(bf16 ? query_kernel<bf16_t> : query_kernel<float>, a, A, t, stream)) return rc;
    hipLaunchKernelGGL(score_fwd_kernel, dim3(nt, B), dim3(kST), lds, (hipStream_t)stream, a, t);
    SBK_CHECK_LAUNCH();
    hipLaunchKernelGGL(combine_kernel, dim3(B), dim3(kST), 0, (hipStream_t)stream, a, t);
    SBK_CHECK_LAUNCH();
    if (int rc = launch(bf16 ? cproj_kernel<bf16_t> : cproj_kernel<float>, a, O, t, stream)) return rc;
  }
  return 0;
}

// See include/sbk.h.
SBK_API int sbk_attdec_bwd(int bf16, const void* w_icT, const void* w_hhT, const void* w_decT, const void* w_outT,
                           const float* P, const float* enc, const int* enc_len, const float* w_conv,
                           const float* w_loc, const float* w_attn, float scaling, const float* h0, const float* attn0,
                           const float* mc, const float* hstate, const float* ctx, const float* attn,
                           const float* dech, const float* save, const float* dattn, const float* dhproj, int B, int T,
                           int L, int H, int A, int O, int E, int C, int ksz, float* dcall, float* dgi, float* dgh,
                           float* dctx, float* dP, float* ddech, float* slots, float* ws, void* stream) {
  if (!w_icT || !w_hhT || !w_decT || !w_outT || !P || !enc || !enc_len || !w_attn || !hstate || !ctx || !attn ||
      !dech || !save || !dhproj || !dcall || !dgi || !dgh || !dctx || !dP || !ddech || !slots || !ws)
    return SBK_ERR_ARG;
  if (bad_dims(B, T, L, H, A, O, E)) return SBK_ERR_ARG;
  if (w_loc ? (!w_conv || !attn0 || C <= 0 || C > 16 * kCT || ksz < 0) : (w_conv != nullptr)) return SBK_ERR_ARG;
  const int Ck = w_loc ? C : 0, nt = (L + kLT - 1) / kLT, CW = (Ck + 15) / 16 * 16;
  const size_t lds = sizeof(float) * ((size_t)stage_floats(Ck, ksz) + kLT + kSW * kLT * 16 + (size_t)kSW * kLT * CW);
  if (lds > 160 * 1024 - 1024) return SBK_ERR_ARG;
  if (lds > 64 * 1024)
    if (hipError_t e = lds_optin((const void*)score_bwd_kernel, lds)) return (int)e;
  BwdArgs a;
  a.w_icT = w_icT; a.w_hhT = w_hhT; a.w_decT = w_decT; a.w_outT = w_outT;
  a.P = P; a.enc = enc; a.enc_len = enc_len; a.w_conv = w_conv; a.w_loc = w_loc; a.w_attn = w_attn;
  a.h0 = h0; a.attn0 = attn0; a.mc = mc; a.hstate = hstate; a.ctx = ctx; a.attn = attn; a.dech = dech; a.save = save;
  a.dattn = dattn; a.dhproj = dhproj;
  a.dcall = dcall; a.dgi = dgi; a.dgh = dgh; a.dctx = dctx; a.dP = dP; a.ddech = ddech; a.slots = slots;
  a.dhw = ws;
  a.ddp = a.dhw + (size_t)2 * B * H;
  a.scaling = scaling;
  a.d = Dims{B, T, L, H, A, O, E, Ck, ksz, nt};
  a.vec_icT = vecw(w_icT, 3 * H, bf16);
  a.vec_hhT = vecw(w_hhT, 3 * H, bf16);
  a.vec_decT = vecw(w_decT, A, bf16);
  a.vec_outT = vecw(w_outT, O, bf16);
  a.vec_g = vecx(dgi, 3 * H) && vecx(dgh, 3 * H);
  a.vec_a = vecx(ddech, A);
  a.vec_o = vecx(dcall, O);
  const long long BA = (long long)B * A;
  for (int t = T - 1; t >= 0; --t) {
    if (t < T - 1)
      if (int rc = launch(bf16 ? dc_kernel<bf16_t> : dc_kernel<float>, a, O, t, stream)) return rc;
    if (int rc = launch(bf16 ? dctx_kernel<bf16_t> : dctx_kernel<float>, a, E, t, stream)) return rc;
    hipLaunchKernelGGL(score_bwd_kernel, dim3(nt, B), dim3(kST), lds, (hipStream_t)stream, a, t);
    SBK_CHECK_LAUNCH();
    hipLaunchKernelGGL(tilesum_kernel, dim3((unsigned)((BA + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, t);
    SBK_CHECK_LAUNCH();
    if (int rc = launch(bf16 ? cell_bwd_kernel<bf16_t> : cell_bwd_kernel<float>, a, H, t, stream)) return rc;
  }
  return 0;
}

// hypotheses of one beam-score workgroup: its grid is (nt, B, ceil(G / this))
SBK_API int sbk_attdec_beam_group() { return kGH; }

// See include/sbk.h.
SBK_API int sbk_attdec_beam_step(int bf16, const void* w_ic, const void* w_hh, const float* b_hh, const void* w_dec,
                                 const float* b_q, const void* w_out, const float* b_out, const float* gx,
                                 const int* token, const float* P, const float* enc, const int* enc_len,
                                 const float* w_conv, const float* w_loc, const float* w_attn, float scaling,
                                 const int* parent, const float* h_prev, const float* c_prev, const float* attn_prev,
                                 const float* cov_prev, const int* peak_prev, int first, int max_shift, int V, int B,
                                 int G, int L, int H, int A, int O, int E, int C, int ksz, float* h, float* c,
                                 float* attn, float* cov, int* peak, int* shift_ok, float* pen, float* ctx,
                                 float* dech, float* ws, void* stream) {
  if (!w_ic || !w_hh || !w_dec || !w_out || !gx || !P || !enc || !enc_len || !w_attn || !parent || !h_prev ||
      !c_prev || !cov_prev || !peak_prev || !h || !c || !attn || !cov || !peak || !shift_ok || !pen || !ctx || !dech ||
      !ws)
    return SBK_ERR_ARG;
  if (G <= 0 || B <= 0 || (long long)B * G > 65535 || max_shift < 0 || max_shift > (1 << 30) || (token && V <= 0))
    return SBK_ERR_ARG;
  const int N = B * G;
  if (bad_dims(N, 1, L, H, A, O, E)) return SBK_ERR_ARG;
  if (w_loc ? (!w_conv || !attn_prev || C <= 0 || C > 16 * kCT || ksz < 0) : (w_conv != nullptr)) return SBK_ERR_ARG;
  const int Ck = w_loc ? C : 0, nt = (L + kLT - 1) / kLT;
  const size_t lds = sizeof(float) * ((size_t)beam_stage_floats(Ck, ksz) + (kSW + 1) * kGH * kLT);
  if (lds > 160 * 1024 - 1024) return SBK_ERR_ARG;
  if (lds > 64 * 1024)
    if (hipError_t e = lds_optin((const void*)beam_score_kernel, lds)) return (int)e;
  BeamArgs a;
  a.w_ic = w_ic; a.w_hh = w_hh; a.b_hh = b_hh; a.gx = gx; a.token = token; a.P = P; a.enc = enc; a.enc_len = enc_len;
  a.w_conv = w_conv; a.w_loc = w_loc; a.w_attn = w_attn; a.parent = parent;
  a.h_prev = h_prev; a.c_prev = c_prev; a.attn_prev = attn_prev; a.cov_prev = cov_prev; a.peak_prev = peak_prev;
  a.dech = dech; a.h = h; a.attn = attn; a.cov = cov; a.ctx = ctx; a.pen = pen; a.peak = peak; a.shift_ok = shift_ok;
  a.scores = ws;
  a.ms = a.scores + (size_t)N * L;
  a.pctx = a.ms + (size_t)N * nt * 2;
  a.scaling = scaling; a.first = first; a.max_shift = max_shift; a.V = V;
  a.B = B; a.G = G; a.N = N; a.L = L; a.H = H; a.A = A; a.O = O; a.E = E; a.C = Ck; a.ksz = ksz; a.nt = nt;
  a.vec_ic = vecw(w_ic, O, bf16);
  a.vec_hh = vecw(w_hh, H, bf16);
  a.vec_c = vecx(c_prev, O);
  a.vec_h = vecx(h_prev, H);
  // the query and the context projection are the sequence kernels at T = 1 over the N rows
  FwdArgs f = {};
  f.w_dec = w_dec; f.w_out = w_out; f.b_q = b_q; f.b_out = b_out;
  f.hstate = h; f.cstate = c; f.ctx = ctx; f.dech = dech;
  f.d = Dims{N, 1, L, H, A, O, E, Ck, ksz, nt};
  f.vec_dec = vecw(w_dec, H, bf16);
  f.vec_out = vecw(w_out, E, bf16);
  f.vec_h = vecx(h, H);
  f.vec_x = vecx(ctx, E);
  const dim3 cgrid((H + kSlice - 1) / kSlice, (N + kRows - 1) / kRows);
  hipLaunchKernelGGL(bf16 ? beam_cell_kernel<bf16_t> : beam_cell_kernel<float>, cgrid, dim3(kThreads), 0,
                     (hipStream_t)stream, a);
  SBK_CHECK_LAUNCH();
  if (int rc = launch(bf16 ? query_kernel<bf16_t> : query_kernel<float>, f, A, 0, stream)) return rc;
  hipLaunchKernelGGL(beam_score_kernel, dim3(nt, B, (G + kGH - 1) / kGH), dim3(kST), lds, (hipStream_t)stream, a);
  SBK_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_combine_kernel, dim3(N), dim3(kST), 0, (hipStream_t)stream, a);
  SBK_CHECK_LAUNCH();
  return launch(bf16 ? cproj_kernel<bf16_t> : cproj_kernel<float>, f, O, 0, stream);
}
