// Incremental transformer decoding: one decode step of the decoder's masked
// self-attention over an append-only key/value cache, and one decode step of
// its cross-attention over encoder keys / values that were projected once.
//
// Reference semantics: torch.nn.MultiheadAttention as the reference's decoder
// calls it (speechbrain/lobes/models/transformer/Transformer.py:489-654,
// nnet/attention.py:642-778), restricted to the last query position: exact
// softmax with the row maximum subtracted, scale 1/sqrt(dh), head h owning
// columns [h*dh, (h+1)*dh) of a row.  fp32 throughout.
//
// Every row pointer takes a row stride in floats, so q / k_new / v_new can be
// the three column blocks of one (N, 3E) in_proj GEMM output and the encoder
// K / V the two blocks of one (B*S, 2E) output, without copies.
//
// Self-attention cache: kc, vc (cap, N, E), position-major, never moved.  A
// beam permutation touches only the ancestry table anc (N, anc_ld) int32:
// row n's key at position j is kc[j][anc[n][j]].  Every anc value is clamped
// to [0, N) before it indexes the cache.
#include "sbk_common.h"

#include <limits.h>

using namespace sbk;

namespace {

constexpr int kDhMax = 128;
constexpr int kChunk = 256;  // keys per chunk of the cross kernel = its threads

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float dot4(float4 a, float4 b, float s) {
  s = fmaf(a.x, b.x, s);
  s = fmaf(a.y, b.y, s);
  s = fmaf(a.z, b.z, s);
  return fmaf(a.w, b.w, s);
}

// grid N*H, one wave per (row n, head h).  A lane holds columns lane and
// lane + 64 of the row's q, k_new and v_new in registers: it stores the k / v
// pair into slot L-1 of the caches, and the new position's score and its P*V
// term come from those registers, never back from the cache (no other row
// reads slot [L-1][n] in this launch: anc[m][L-1] = m).  The older positions:
// a lane owns one position of a 64-position chunk and walks its key row in
// 16-byte loads against q in LDS; the probabilities and the clamped ancestors
// go through LDS; P*V: the lane's two columns over the chunk's value rows
// (one coalesced run per position).  Online softmax across chunks.
//
// MASKED: keymask (cap, N) bytes, nonzero = the key is masked (the language
// model's padding mask: the token at that position is pad_idx).  Row n's key
// at j < L-1 is masked by keymask[j][anc[n][j]], its new key by
// keymask[L-1][n]; a masked score is -inf.  A chunk, or every chunk so far,
// may then hold no finite score: the exponentials are taken against 0 while
// the running maximum is still -inf, so they are exp(-inf) = 0, never
// exp(-inf - -inf).  A (row, head) with every key masked ends with l = 0 and
// writes 0 / 0 = NaN, as a softmax over an all -inf row does.  With no byte
// set the arithmetic is the unmasked kernel's, operation for operation.
template <bool MASKED>
__global__ void __launch_bounds__(64)
    kv_self_kernel(const float* __restrict__ q, const float* __restrict__ k_new, const float* __restrict__ v_new,
                   long long ld, float* __restrict__ kc, float* __restrict__ vc, const int* __restrict__ anc,
                   long long anc_ld, const uint8_t* __restrict__ keymask, int N, int H, int dh, int L, float scale,
                   float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float qs[kDhMax];
  __shared__ float ps[64];
  __shared__ int an[64];
  const int n = blockIdx.x / H, h = blockIdx.x % H, lane = threadIdx.x;
  const long long E = (long long)H * dh;
  const long long in_off = (long long)n * ld + (long long)h * dh;
  const long long slot = ((long long)(L - 1) * N + n) * E + (long long)h * dh;
  const bool c0_ok = lane < dh, c1_ok = lane + 64 < dh;
  float kn0 = 0.f, kn1 = 0.f, vn0 = 0.f, vn1 = 0.f, qk = 0.f;
  if (c0_ok) {
    const float q0 = q[in_off + lane];
    kn0 = k_new[in_off + lane];
    vn0 = v_new[in_off + lane];
    qs[lane] = q0;
    kc[slot + lane] = kn0;
    vc[slot + lane] = vn0;
    qk = q0 * kn0;
  }
  if (c1_ok) {
    const float q1 = q[in_off + lane + 64];
    kn1 = k_new[in_off + lane + 64];
    vn1 = v_new[in_off + lane + 64];
    qs[lane + 64] = q1;
    kc[slot + lane + 64] = kn1;
    vc[slot + lane + 64] = vn1;
    qk = fmaf(q1, kn1, qk);
  }
  const float s_new = wave_sum(qk) * scale;
  __syncthreads();
  float acc0 = 0.f, acc1 = 0.f, m = -INFINITY, l = 0.f;
  for (int c0 = 0; c0 < L; c0 += 64) {
    const int j = c0 + lane;
    float s = (j == L - 1) ? s_new : -INFINITY;
    int a = n;
    if (j < L - 1) {
      a = min(max(anc[(long long)n * anc_ld + j], 0), N - 1);
      const float* kr = kc + ((long long)j * N + a) * E + (long long)h * dh;
      float d = 0.f;
      for (int i = 0; i < dh / 4; ++i) d = dot4(*reinterpret_cast<const float4*>(qs + 4 * i), ld4(kr + 4 * i), d);
      s = d * scale;
    }
    if constexpr (MASKED) {
      if (j < L && keymask[(long long)j * N + a]) s = -INFINITY;  // j = L-1: a = n
    }
    an[lane] = a;
    float m_new = fmaxf(m, wave_max(s));  // unmasked: finite, every chunk holds a position < L
    float m_ref = m_new;                  // what the exponentials are taken against
    if constexpr (MASKED) {
      if (m_new == -INFINITY) m_ref = 0.f;  // nothing unmasked yet: p = alpha = exp(-inf) = 0
    }
    const float p = (j < L) ? expf(s - m_ref) : 0.f;
    const float alpha = expf(m - m_ref);  // first chunk: exp(-inf) = 0
    l = l * alpha + wave_sum(p);
    acc0 *= alpha;
    acc1 *= alpha;
    m = m_new;
    ps[lane] = p;
    __syncthreads();
    const int cnt = min(64, L - 1 - c0);  // cached positions of this chunk
#pragma unroll 4
    for (int jj = 0; jj < cnt; ++jj) {
      const float* vr = vc + ((long long)(c0 + jj) * N + an[jj]) * E + (long long)h * dh;
      const float pj = ps[jj];
      if (c0_ok) acc0 = fmaf(pj, vr[lane], acc0);
      if (c1_ok) acc1 = fmaf(pj, vr[lane + 64], acc1);
    }
    if (L - 1 - c0 < 64) {  // the new position is in this (the last) chunk
      const float pj = ps[L - 1 - c0];
      acc0 = fmaf(pj, vn0, acc0);
      acc1 = fmaf(pj, vn1, acc1);
    }
    __syncthreads();
  }
  float* orow = out + (long long)n * E + (long long)h * dh;
  const float inv = 1.f / l;
  if (c0_ok) orow[lane] = acc0 * inv;
  if (c1_ok) orow[lane + 64] = acc1 * inv;
}

// The scores of key j against the R staged query rows: the key row is read
// once, in 16-byte loads, for all R rows (queries broadcast from LDS).
template <int R>
__device__ __forceinline__ void cross_scores(const float* __restrict__ kr, const float* qs, int dh, float (&s)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) s[r] = 0.f;
#pragma unroll 2
  for (int i = 0; i < dh / 4; ++i) {
    const float4 k4 = ld4(kr + 4 * i);
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = dot4(*reinterpret_cast<const float4*>(qs + r * dh + 4 * i), k4, s[r]);
  }
}

// grid B*H, 256 threads: workgroup (b, h) serves the `group` beam rows of
// utterance b, R rows per pass, so a K / V row is read once per pass for R
// beams (once in all when group <= R).  Per 256-key chunk:
//   A  thread = key: its scores against the R rows -> ps[r][key]
//   B  wave = row: chunk maximum, running maximum / sum, ps <- exp(s - m)
//   C  thread = (column d, key slice): acc[r] += p[r][j] * V[j][d]; the
//      256 / nd slices (nd = dh rounded up to 16 / 32 / 64 / 128) are summed
//      through LDS at the end of the pass.
// probs, when asked for, is a second walk over the keys with the final
// (maximum, sum) of each row.
template <int R>
__global__ void __launch_bounds__(kChunk)
    kv_cross_kernel(const float* __restrict__ q, long long q_ld, const float* __restrict__ k,
                    const float* __restrict__ v, long long kv_ld, const int* __restrict__ klen, int group, int H,
                    int dh, int S, int nd, float scale, float* __restrict__ out, float* __restrict__ probs) {
  __shared__ __attribute__((aligned(16))) float qs[R * kDhMax];
  __shared__ __attribute__((aligned(16))) float ps[R * kChunk];
  __shared__ float ms[R], ls[R], al[R];
  __shared__ int kl[R];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long E = (long long)H * dh;
  const float* kb = k + (long long)b * S * kv_ld + (long long)h * dh;
  const float* vb = v + (long long)b * S * kv_ld + (long long)h * dh;
  const int d = tid % nd, slice = tid / nd, slices = kChunk / nd;

  for (int r0 = 0; r0 < group; r0 += R) {
    for (int i = tid; i < R * dh; i += kChunk) {
      const int r = i / dh, dd = i - r * dh;
      qs[i] = (r0 + r < group) ? q[((long long)b * group + r0 + r) * q_ld + (long long)h * dh + dd] : 0.f;
    }
    if (tid < R) {
      const bool live = r0 + tid < group;
      kl[tid] = (live && klen) ? min(max(klen[(long long)b * group + r0 + tid], 1), S) : S;
      ms[tid] = -INFINITY;
      ls[tid] = 0.f;
    }
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    __syncthreads();

    for (int c0 = 0; c0 < S; c0 += kChunk) {
      {  // A
        const int j = c0 + tid;
        float s[R];
        cross_scores<R>(kb + (long long)min(j, S - 1) * kv_ld, qs, dh, s);  // j >= S: masked below
#pragma unroll
        for (int r = 0; r < R; ++r) ps[r * kChunk + tid] = (j < kl[r]) ? s[r] * scale : -INFINITY;  // kl <= S
      }
      __syncthreads();
      for (int r = wave; r < R; r += 4) {  // B
        float x[4];
        float cm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[i] = ps[r * kChunk + lane + 64 * i];
          cm = fmaxf(cm, x[i]);
        }
        const float m_old = ms[r], l_old = ls[r];
        const float m_new = fmaxf(m_old, wave_max(cm));  // finite: key 0 is never masked (kl >= 1)
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = expf(x[i] - m_new);
          ps[r * kChunk + lane + 64 * i] = e;
          sum += e;
        }
        sum = wave_sum(sum);
        if (lane == 0) {
          const float a = expf(m_old - m_new);  // first chunk: exp(-inf) = 0
          ms[r] = m_new;
          al[r] = a;
          ls[r] = l_old * a + sum;
        }
      }
      __syncthreads();
      {  // C
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] *= al[r];
        const int jb = c0 + slice * nd;  // nd keys per slice: slices * nd = kChunk
        const int je = min(jb + nd, S);
        if (d < dh) {
          for (int j = jb; j < je; j += 4) {
            const float* vr = vb + (long long)j * kv_ld + d;
            const float v0 = vr[0];
            const float v1 = (j + 1 < je) ? vr[kv_ld] : 0.f;
            const float v2 = (j + 2 < je) ? vr[2 * kv_ld] : 0.f;
            const float v3 = (j + 3 < je) ? vr[3 * kv_ld] : 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const float4 p4 = *reinterpret_cast<const float4*>(ps + r * kChunk + (j - c0));
              acc[r] = fmaf(p4.x, v0, acc[r]);
              acc[r] = fmaf(p4.y, v1, acc[r]);
              acc[r] = fmaf(p4.z, v2, acc[r]);
              acc[r] = fmaf(p4.w, v3, acc[r]);
            }
          }
        }
      }
      __syncthreads();
    }

    // the slices' partial sums -> out
#pragma unroll
    for (int r = 0; r < R; ++r) ps[(slice * R + r) * nd + d] = acc[r];
    __syncthreads();
    for (int i = tid; i < R * dh; i += kChunk) {
      const int r = i / dh, dd = i - r * dh;
      if (r0 + r >= group) continue;
      float sum = 0.f;
      for (int sl = 0; sl < slices; ++sl) sum += ps[(sl * R + r) * nd + dd];
      out[((long long)b * group + r0 + r) * E + (long long)h * dh + dd] = sum / ls[r];
    }
    if (probs) {
      for (int c0 = 0; c0 < S; c0 += kChunk) {
        const int j = c0 + tid;
        if (j >= S) continue;
        float s[R];
        cross_scores<R>(kb + (long long)j * kv_ld, qs, dh, s);
        float* pr = probs + (((long long)b * group + r0) * H + h) * S + j;  // row r: + r*H*S
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r0 + r >= group) continue;
          pr[(long long)r * H * S] = (j < kl[r]) ? expf(s[r] * scale - ms[r]) / ls[r] : 0.f;
        }
      }
    }
    __syncthreads();  // the next pass restages qs / ms / ls / ps
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// One decode step of masked self-attention over the cache.  q, k_new, v_new
// (N, E) views with row stride ld; kc, vc (cap, N, E); anc (N, anc_ld) int32
// with anc[n][L-1] = n; out (N, E).  Stores k_new / v_new into slot L-1, then
// row n attends kc / vc[j][anc[n][j]] for j < L.
SBK_API int sbk_kv_decode_self_attn(const float* q, const float* k_new, const float* v_new, long long ld, float* kc,
                                    float* vc, int cap, const int* anc, long long anc_ld, int N, int H, int dh,
                                    int L, float* out, void* stream) {
  if (!q || !k_new || !v_new || !kc || !vc || !anc || !out) return SBK_ERR_ARG;
  if (N <= 0 || H <= 0 || dh <= 0 || L <= 0 || dh % 4 != 0 || dh > kDhMax || L > cap) return SBK_ERR_ARG;
  const long long E = (long long)H * dh;
  if (ld < E || ld % 4 != 0 || anc_ld < L || (long long)N * H > INT_MAX || E > INT_MAX) return SBK_ERR_ARG;
  if (!aligned16(q) || !aligned16(k_new) || !aligned16(v_new) || !aligned16(kc) || !aligned16(vc)) return SBK_ERR_ARG;
  hipLaunchKernelGGL(kv_self_kernel<false>, dim3(N * H), dim3(64), 0, (hipStream_t)stream, q, k_new, v_new, ld, kc, vc,
                     anc, anc_ld, nullptr, N, H, dh, L, 1.f / sqrtf((float)dh), out);
  SBK_CHECK_LAUNCH();
  return 0;
}

// The same step with a key mask (the decode step of a language model that
// masks its padding token): keymask (cap, N) uint8, nonzero = masked, slot
// L-1 filled by the caller before the call.  Row n's key at j < L-1 is masked
// by keymask[j][anc[n][j]], its new key by keymask[L-1][n].  A (row, head)
// whose keys are all masked gets NaN.  With an all-zero mask the result is
// bit-equal to sbk_kv_decode_self_attn.
SBK_API int sbk_kv_decode_self_attn_masked(const float* q, const float* k_new, const float* v_new, long long ld,
                                           float* kc, float* vc, int cap, const int* anc, long long anc_ld,
                                           const unsigned char* keymask, int N, int H, int dh, int L, float* out,
                                           void* stream) {
  if (!q || !k_new || !v_new || !kc || !vc || !anc || !keymask || !out) return SBK_ERR_ARG;
  if (N <= 0 || H <= 0 || dh <= 0 || L <= 0 || dh % 4 != 0 || dh > kDhMax || L > cap) return SBK_ERR_ARG;
  const long long E = (long long)H * dh;
  if (ld < E || ld % 4 != 0 || anc_ld < L || (long long)N * H > INT_MAX || E > INT_MAX) return SBK_ERR_ARG;
  if (!aligned16(q) || !aligned16(k_new) || !aligned16(v_new) || !aligned16(kc) || !aligned16(vc)) return SBK_ERR_ARG;
  hipLaunchKernelGGL(kv_self_kernel<true>, dim3(N * H), dim3(64), 0, (hipStream_t)stream, q, k_new, v_new, ld, kc, vc,
                     anc, anc_ld, keymask, N, H, dh, L, 1.f / sqrtf((float)dh), out);
  SBK_CHECK_LAUNCH();
  return 0;
}

// One decode step of cross-attention.  q (N, E) with row stride q_ld; k, v
// (B, S, E) with row stride kv_ld, B = N / group; row n attends utterance
// n / group, keys j < klen[n] (int32, clamped to 1 .. S; null: all S keys);
// out (N, E); probs (N, H, S) or null, 0 at j >= klen.
SBK_API int sbk_kv_decode_cross_attn(const float* q, long long q_ld, const float* k, const float* v, long long kv_ld,
                                     const int* klen, int N, int group, int H, int dh, int S, float* out,
                                     float* probs, void* stream) {
  if (!q || !k || !v || !out) return SBK_ERR_ARG;
  if (N <= 0 || group <= 0 || H <= 0 || dh <= 0 || S <= 0 || dh % 4 != 0 || dh > kDhMax) return SBK_ERR_ARG;
  if (N % group != 0) return SBK_ERR_ARG;
  const long long E = (long long)H * dh;
  const long long B = N / group;
  if (q_ld < E || kv_ld < E || q_ld % 4 != 0 || kv_ld % 4 != 0 || B * H > INT_MAX || E > INT_MAX) return SBK_ERR_ARG;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v)) return SBK_ERR_ARG;
  const int nd = dh <= 16 ? 16 : dh <= 32 ? 32 : dh <= 64 ? 64 : 128;
  const float scale = 1.f / sqrtf((float)dh);
  const dim3 grid((unsigned)(B * H));
  if (group <= 4)
    hipLaunchKernelGGL(kv_cross_kernel<4>, grid, dim3(kChunk), 0, (hipStream_t)stream, q, q_ld, k, v, kv_ld, klen,
                       group, H, dh, S, nd, scale, out, probs);
  else
    hipLaunchKernelGGL(kv_cross_kernel<16>, grid, dim3(kChunk), 0, (hipStream_t)stream, q, q_ld, k, v, kv_ld, klen,
                       group, H, dh, S, nd, scale, out, probs);
  SBK_CHECK_LAUNCH();
  return 0;
}
