// The tail of LM fusion in a beam-search step (decoders/seq2seq.py:756-760,
// :1391-1398 of the reference): log_probs + lm_weight * log_softmax(lm_logits
// / temperature_lm) as one kernel instead of four passes over (N, V) —
// divide, log-softmax, scale, add.
//
//   out[n][v] = base[n][v] + w * (logits[n][v] * invT - logsumexp_v(logits[n][:] * invT))
//
// fp32; exact: the row maximum is subtracted before the exponentials.  base
// may be null (plain scaled log-softmax).  Its -inf / -1e20 sentinels pass
// through as fp32 addition gives them.
#include "sbk_common.h"

using namespace sbk;

namespace {

constexpr int kThreads = 256;
constexpr int kRowMax = 8192;  // floats of a row kept in LDS (32 KB): the recipes' vocab is 5000

// grid N, one workgroup per row.  ONCHIP: the scaled row is staged in LDS
// while its maximum is taken, so HBM is read once; the sum and the output
// pass read LDS.  Otherwise (V > kRowMax) the row is read twice: an online
// (maximum, sum) pass, then the output pass.
template <bool ONCHIP>
__global__ void __launch_bounds__(kThreads)
    log_softmax_fuse_kernel(const float* __restrict__ logits, long long ld, const float* __restrict__ base,
                            long long base_ld, int V, float invT, float w, float* __restrict__ out) {
  __shared__ float row[ONCHIP ? kRowMax : 1];
  __shared__ float red[kThreads / 64];
  const int tid = threadIdx.x;
  const float* x = logits + (long long)blockIdx.x * ld;
  float m = -INFINITY, sum = 0.f;
  if constexpr (ONCHIP) {
    for (int v = tid; v < V; v += kThreads) {
      const float s = x[v] * invT;
      row[v] = s;
      m = fmaxf(m, s);
    }
    m = block_max(m, red);  // its barriers also publish row[]
    for (int v = tid; v < V; v += kThreads) sum += expf(row[v] - m);
  } else {
    for (int v = tid; v < V; v += kThreads) {  // per-thread online pair
      const float s = x[v] * invT;
      if (s > m) {
        sum = sum * expf(m - s) + 1.f;  // first element: 0 * exp(-inf) + 1
        m = s;
      } else if (s != -INFINITY) {  // a -inf logit adds 0, also while m is still -inf (NaN stays NaN)
        sum += expf(s - m);
      }
    }
    const float mt = m;
    m = block_max(m, red);
    sum *= expf(mt - m);  // a thread of an all -inf slice: mt = -inf, sum = 0 (m = -inf too: NaN, as torch)
  }
  sum = block_sum(sum, red);
  const float lse = logf(sum);
  float* o = out + (long long)blockIdx.x * V;
  const float* b = base ? base + (long long)blockIdx.x * base_ld : nullptr;
  for (int v = tid; v < V; v += kThreads) {
    const float s = ONCHIP ? row[v] : x[v] * invT;
    const float lp = w * ((s - m) - lse);
    o[v] = b ? b[v] + lp : lp;
  }
}

}  // namespace

// out (N, V) contiguous = base + w * log_softmax(logits * invT) over each row.
// logits (N, V) with row stride ld, base (N, V) with row stride base_ld or
// null.  Any V >= 1: rows up to 8192 floats are read from memory once.
SBK_API int sbk_log_softmax_fuse(const float* logits, long long ld, const float* base, long long base_ld, int N, int V,
                                 float invT, float w, float* out, void* stream) {
  if (!logits || !out) return SBK_ERR_ARG;
  if (N <= 0 || V <= 0 || ld < V || (base && base_ld < V)) return SBK_ERR_ARG;
  if (V <= kRowMax)
    hipLaunchKernelGGL(log_softmax_fuse_kernel<true>, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, logits, ld, base,
                       base_ld, V, invT, w, out);
  else
    hipLaunchKernelGGL(log_softmax_fuse_kernel<false>, dim3(N), dim3(kThreads), 0, (hipStream_t)stream, logits, ld,
                       base, base_ld, V, invT, w, out);
  SBK_CHECK_LAUNCH();
  return 0;
}
