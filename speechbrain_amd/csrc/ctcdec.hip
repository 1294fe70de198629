// Joint CTC/attention decoding: the CTC prefix scorer's step and state
// advance, and the CTC greedy decode.
//
// Reference: speechbrain/decoders/ctc.py
//   CTCPrefixScorer.forward_step :84-243, permute_mem :245-294
//   ctc_greedy_decode :334-376, filter_ctc_output :297-331
// (Algorithm 2 of Watanabe et al., "Hybrid CTC/attention architecture for
// end-to-end speech recognition", MERL TR2017-190).
//
// Layouts: x (B, T, V) fp32 CTC log-probs, already masked past each
// utterance's length; the scorer state r (T, 2, N) fp32 with N = B·beam rows
// (r[t, 0, n] ends in a non-blank, r[t, 1, n] in blank); psi (N) fp32.
//
// One prefix h = g·c is scored by a walk over the frames t = start … end−1:
//   r_nb[t] = logaddexp(r_nb[t−1], phi[t−1]) + x[t, c]
//   r_b[t]  = logaddexp(r_nb[t−1], r_b[t−1]) + x[t, blank]
//   phi[t]  = logaddexp(r_prev[t, 0], r_prev[t, 1]),  or r_prev[t, 1] when c is g's last token
//   psi     = log( exp(r_nb[start−1]) + Σ_t exp(phi[t−1] + x[t, c]) )
// The reference materialises r for every (row, candidate) — (T, 2, N, C)
// floats per decoded token — and then keeps `beam` columns per utterance.
// Here the step keeps no per-candidate state: it returns only the (N, V)
// scores, and the advance kernel reruns the walk for the N surviving
// (parent row, token) pairs through the same prefix_walk(), so what it stores
// is bit for bit what the step scored.
//
// The reference's finite sentinel −1e20 is kept as is: logaddexp of two
// sentinels is the sentinel (−1e20 + log 2 rounds to −1e20 in fp32), and
// sums of sentinels stay finite.
#include "sbk_common.h"

#include <limits.h>

using namespace sbk;

namespace {

constexpr float kNeg = -1e20f;
constexpr int kMaxFrames = 4096;  // 3·T floats of LDS per workgroup, <= 48 KiB

__device__ __forceinline__ float lae(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  const float d = (lo == hi) ? 0.f : lo - hi;  // equal infinities: no NaN
  return hi + logf(1.f + expf(d));
}

// The walk of one (row, candidate) pair.  xc = &x[b, 0, c], ldx = V.
// prev(t, rsum, rb, xb) gives logaddexp(r_prev[t−1, 0], r_prev[t−1, 1]),
// r_prev[t−1, 1] and x[b, t, blank]; emit(t, r_nb[t], r_b[t]) receives every
// frame of the walk.  The next frame's inputs are fetched before this frame's
// exp / log chain, which is the latency of the kernel.  psi is a running
// (maximum, rescaled sum) pair: one exp per frame.
template <class Prev, class Emit>
__device__ __forceinline__ float prefix_walk(const float* __restrict__ xc, long long ldx, Prev prev, bool is_last,
                                             int prefix_len, int start, int end, Emit emit) {
  float rnb = (prefix_len == 0 && start == 1) ? xc[0] : kNeg;
  float rb = kNeg;
  float m = rnb, s = 1.f;
  float xt = 0.f, rsum = 0.f, rbp = 0.f, xb = 0.f;
  if (start < end) {
    xt = xc[(long long)start * ldx];
    prev(start, rsum, rbp, xb);
  }
  for (int t = start; t < end; ++t) {
    float xt_n = 0.f, rsum_n = 0.f, rbp_n = 0.f, xb_n = 0.f;
    if (t + 1 < end) {
      xt_n = xc[(long long)(t + 1) * ldx];
      prev(t + 1, rsum_n, rbp_n, xb_n);
    }
    const float phi = is_last ? rbp : rsum;
    const float nnb = lae(rnb, phi) + xt;
    const float nb = lae(rnb, rb) + xb;
    const float v = phi + xt;
    const float e = (v == m) ? 1.f : expf(-fabsf(v - m));
    s = (v > m) ? fmaf(s, e, 1.f) : s + e;
    m = fmaxf(m, v);
    rnb = nnb;
    rb = nb;
    emit(t, rnb, rb);
    xt = xt_n;
    rsum = rsum_n;
    rbp = rbp_n;
    xb = xb_n;
  }
  return m + logf(s);
}

__device__ __forceinline__ int wrap_frame(int lf, int T) {
  if (lf < 0) lf += T;  // enc_len 0: the reference's index −1 is the last frame
  return min(max(lf, 0), T - 1);
}

// grid (N, tiles): workgroup (n, j) scores the candidates j·blockDim … of row
// n.  Candidates of a row sit on consecutive lanes, so in full mode the
// x[t, ·] reads of a wave are one contiguous 256-byte run per frame.  The
// row's r_prev column is the same for all its candidates: it is staged once
// per workgroup as rsum[t], r_b[t], next to x[t, blank] (3·T floats of LDS).
// In partial mode (cand != null) the grid has one tile, which first fills the
// whole output row with the sentinel and the eos column.
__global__ void __launch_bounds__(256)
    ctc_prefix_step_kernel(const float* __restrict__ x, const float* __restrict__ r_prev,
                           const float* __restrict__ psi_prev, const long long* __restrict__ last_tok,
                           const long long* __restrict__ cand, const int* __restrict__ last_frame, int beam, int N,
                           int T, int V, int C, int prefix_len, int start, int end, int blank, int eos,
                           float* __restrict__ out) {
  extern __shared__ float lds[];
  float* rsum = lds;
  float* rbv = lds + T;
  float* xbv = lds + 2 * T;
  const int n = blockIdx.x, b = n / beam, tid = threadIdx.x;
  const float* xu = x + (long long)b * T * V;
  for (int t = tid; t < T; t += blockDim.x) {
    const float r0 = r_prev[((long long)t * 2 + 0) * N + n];
    const float r1 = r_prev[((long long)t * 2 + 1) * N + n];
    rsum[t] = lae(r0, r1);
    rbv[t] = r1;
    xbv[t] = xu[(long long)t * V + blank];
  }
  __syncthreads();
  const int lf = wrap_frame(last_frame[b], T);
  const float pp = psi_prev ? psi_prev[n] : 0.f;
  const long long last = (prefix_len > 0 && last_tok) ? last_tok[n] : 0;
  const float eos_score = rsum[lf];
  float* orow = out + (long long)n * V;
  if (cand) {
    for (int v = tid; v < V; v += blockDim.x) orow[v] = ((v == eos && v != blank) ? eos_score : kNeg) - pp;
    __syncthreads();
  }
  auto prev = [&](int t, float& s, float& rb, float& xb) {
    s = rsum[t - 1];
    rb = rbv[t - 1];
    xb = xbv[t];
  };
  auto emit = [](int, float, float) {};
  for (int ci = blockIdx.y * blockDim.x + tid; ci < C; ci += gridDim.y * blockDim.x) {
    const long long c = cand ? cand[(long long)n * C + ci] : ci;
    if (c < 0 || c >= V) continue;
    float psi = prefix_walk(xu + c, V, prev, c == last, prefix_len, start, end, emit);
    if (c == eos) psi = eos_score;
    if (c == blank) psi = kNeg;
    orow[c] = psi - pp;
  }
}

// One thread per new row: the walk of (parent row, token), stored as column n
// of r_new, and its psi.  In partial mode a token that was not among its
// parent's candidates takes the parent's candidate 0 for r (ctc.py:281-283)
// and the sentinel for psi.
__global__ void __launch_bounds__(64)
    ctc_prefix_advance_kernel(const float* __restrict__ x, const float* __restrict__ r_prev,
                              const long long* __restrict__ last_tok, const long long* __restrict__ cand,
                              const int* __restrict__ last_frame, const long long* __restrict__ parent,
                              const long long* __restrict__ token, int beam, int N, int T, int V, int C,
                              int prefix_len, int start, int end, int blank, int eos, float* __restrict__ r_new,
                              float* __restrict__ psi_new) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const long long p = parent[n], tok = token[n];
  long long col = tok;
  bool scored = true;
  bool ok = p >= 0 && p < N && tok >= 0 && tok < V;
  if (ok && cand) {
    scored = false;
    for (int j = 0; j < C; ++j) scored = scored || cand[p * C + j] == tok;
    if (!scored) col = cand[p * C];
    ok = col >= 0 && col < V;
  }
  float* r0 = r_new + n;
  float* r1 = r_new + N + n;
  const long long ldr = 2LL * N;
  if (!ok) {  // an index outside the table: sentinel state, nothing read
    for (int t = 0; t < T; ++t) r0[t * ldr] = r1[t * ldr] = kNeg;
    psi_new[n] = kNeg;
    return;
  }
  const int b = (int)(p / beam);
  const float* xu = x + (long long)b * T * V;
  const float* rp0 = r_prev + p;
  const float* rp1 = r_prev + N + p;
  const long long last = (prefix_len > 0 && last_tok) ? last_tok[p] : 0;
  // frames outside the walk keep the reference's initial fill
  const int head = min(start, T);
  for (int t = 0; t < head; ++t) {
    r0[t * ldr] = (t == 0 && prefix_len == 0) ? xu[col] : kNeg;
    r1[t * ldr] = kNeg;
  }
  for (int t = max(start, end); t < T; ++t) r0[t * ldr] = r1[t * ldr] = kNeg;
  auto prev = [&](int t, float& s, float& rb, float& xb) {
    const float a = rp0[(t - 1) * ldr], c = rp1[(t - 1) * ldr];
    s = lae(a, c);
    rb = c;
    xb = xu[(long long)t * V + blank];
  };
  auto emit = [&](int t, float nb, float bl) {
    r0[t * ldr] = nb;
    r1[t * ldr] = bl;
  };
  float psi = prefix_walk(xu + col, V, prev, col == last, prefix_len, start, end, emit);
  if (!scored) psi = kNeg;
  if (tok == eos) {
    const int lf = wrap_frame(last_frame[b], T);
    psi = lae(rp0[lf * ldr], rp1[lf * ldr]);
  }
  if (tok == blank) psi = kNeg;
  psi_new[n] = psi;
}

// One workgroup per utterance.  Pass 1: a wave per frame takes the argmax
// over V (lowest index on a tie) into tokens[b, t].  Pass 2: frames in chunks
// of 256 — keep a frame whose label is neither blank nor its predecessor's,
// prefix-count the kept ones with a ballot per wave, and write them
// compacted over the front of the same row (a kept frame never lands behind
// its own position, and every read of a chunk precedes its writes).
__global__ void __launch_bounds__(256)
    ctc_greedy_kernel(const float* __restrict__ x, long long sb, long long st, long long sv,
                      const int* __restrict__ lens, int T, int V, int blank, int* __restrict__ tokens,
                      int* __restrict__ counts) {
  __shared__ int wtot[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int len = min(max(lens[b], 0), T);
  int* row = tokens + (long long)b * T;
  for (int t = wave; t < len; t += 4) {
    const float* xr = x + b * sb + t * st;
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int v = lane; v < V; v += 64) {
      const float f = xr[v * sv];
      if (bi == INT_MAX || f > best) {
        best = f;
        bi = v;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (oi != INT_MAX && (bi == INT_MAX || ob > best || (ob == best && oi < bi))) {
        best = ob;
        bi = oi;
      }
    }
    if (lane == 0) row[t] = bi;
  }
  __syncthreads();
  int base = 0, carry = -1;
  for (int c0 = 0; c0 < len; c0 += 256) {
    const int t = c0 + tid;
    const int a = t < len ? row[t] : -1;
    const int p = tid == 0 ? carry : (t < len ? row[t - 1] : -1);
    const int next_carry = (c0 + 255 < len) ? row[c0 + 255] : -1;
    const bool keep = t < len && a != blank && a != p;
    const unsigned long long mask = __ballot(keep);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(mask);
    __syncthreads();
    int off = base, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) off += wtot[w];
      total += wtot[w];
    }
    if (keep) row[off + pre] = a;
    base += total;
    carry = next_carry;
    __syncthreads();
  }
  if (tid == 0) counts[b] = base;
}

bool prefix_args_ok(const float* x, const float* r_prev, const int* last_frame, int B, int beam, int T, int V,
                    const long long* cand, int C, int prefix_len, int start, int end, int blank, int eos) {
  if (!x || !r_prev || !last_frame) return false;
  if (B <= 0 || beam <= 0 || T <= 0 || T > kMaxFrames || V <= 0) return false;
  if ((long long)B * beam > INT_MAX) return false;
  if (cand ? (C < 1 || C > V) : C != 0) return false;
  if (blank < 0 || blank >= V || eos < 0 || eos >= V) return false;
  if (prefix_len < 0 || start < 1 || start > T || end > T) return false;
  return true;
}

}  // namespace

// One step of the prefix scorer: out (N, V) = psi − psi_prev, N = B·beam.
SBK_API int sbk_ctc_prefix_step(const float* x, const float* r_prev, const float* psi_prev,
                                const long long* last_tok, const long long* cand, const int* last_frame, int B,
                                int beam, int T, int V, int C, int prefix_len, int start, int end, int blank, int eos,
                                float* out, void* stream) {
  if (!prefix_args_ok(x, r_prev, last_frame, B, beam, T, V, cand, C, prefix_len, start, end, blank, eos) || !out)
    return SBK_ERR_ARG;
  const int N = B * beam;
  const int nc = cand ? C : V;
  const int bd = nc <= 64 ? 64 : nc <= 128 ? 128 : 256;
  const int tiles = cand ? 1 : (V + bd - 1) / bd;
  if (tiles > 65535) return SBK_ERR_ARG;
  hipLaunchKernelGGL(ctc_prefix_step_kernel, dim3(N, tiles), dim3(bd), (size_t)3 * T * sizeof(float),
                     (hipStream_t)stream, x, r_prev, psi_prev, last_tok, cand, last_frame, beam, N, T, V, nc,
                     prefix_len, start, end, blank, eos, out);
  SBK_CHECK_LAUNCH();
  return 0;
}

// The state of the N surviving beams: r_new (T, 2, N) and psi_new (N) of the
// (parent row, token) pairs, from the same inputs the step took.
SBK_API int sbk_ctc_prefix_advance(const float* x, const float* r_prev, const long long* last_tok,
                                   const long long* cand, const int* last_frame, const long long* parent,
                                   const long long* token, int B, int beam, int T, int V, int C, int prefix_len,
                                   int start, int end, int blank, int eos, float* r_new, float* psi_new,
                                   void* stream) {
  if (!prefix_args_ok(x, r_prev, last_frame, B, beam, T, V, cand, C, prefix_len, start, end, blank, eos) || !parent ||
      !token || !r_new || !psi_new)
    return SBK_ERR_ARG;
  const int N = B * beam;
  hipLaunchKernelGGL(ctc_prefix_advance_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, r_prev,
                     last_tok, cand, last_frame, parent, token, beam, N, T, V, C, prefix_len, start, end, blank, eos,
                     r_new, psi_new);
  SBK_CHECK_LAUNCH();
  return 0;
}

// CTC greedy decode: x (B, T, V) fp32 with element strides sb, st, sv;
// lens (B) absolute; tokens (B, T) int32, counts (B) int32.
SBK_API int sbk_ctc_greedy_decode(const float* x, long long sb, long long st, long long sv, const int* lens, int B,
                                  int T, int V, int blank, int* tokens, int* counts, void* stream) {
  if (!x || !lens || !tokens || !counts || B <= 0 || T <= 0 || V <= 0) return SBK_ERR_ARG;
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, sb, st, sv, lens, T, V, blank,
                     tokens, counts);
  SBK_CHECK_LAUNCH();
  return 0;
}
