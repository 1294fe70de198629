// Kernels of the Embedding drop-in (nnet/embedding.py:14-114 of the
// reference): the one-hot table, the gather, and the per-token segment sum
// that its backward and the RNNs' one-hot dW_ih use.  One workgroup per row.
#include "rnnstep.h"

using namespace sbk;

namespace {

constexpr int kRowThreads = 256;

// out (N, D) = rows of the one-hot table of Embedding(consider_as_one_hot):
// D = V - 1 columns, the blank row zero, ids above the blank shifted down
__global__ void __launch_bounds__(kRowThreads)
    embed_onehot_kernel(const int* __restrict__ ids, int blank, int D, float* __restrict__ out) {
  const int idx = rnnstep::token_row(ids[blockIdx.x], blank);
  float* o = out + (long long)blockIdx.x * D;
  for (int d = threadIdx.x; d < D; d += kRowThreads) o[d] = d == idx ? 1.f : 0.f;
}

// out (N, D) = weight[ids] (an id outside [0, V) gives a zero row)
__global__ void __launch_bounds__(kRowThreads)
    embed_gather_kernel(const int* __restrict__ ids, const float* __restrict__ weight, int V, int D,
                        float* __restrict__ out) {
  const int v = ids[blockIdx.x];
  const bool hit = v >= 0 && v < V;
  float* o = out + (long long)blockIdx.x * D;
  const float* wr = weight + (long long)(hit ? v : 0) * D;
  for (int d = threadIdx.x; d < D; d += kRowThreads) o[d] = hit ? wr[d] : 0.f;
}

// grid ncodes: out[code] = sum of src rows order[offs[code] .. offs[code+1]),
// added in list order (order: row ids stably sorted by code)
__global__ void __launch_bounds__(kRowThreads)
    segsum_rows_kernel(const float* __restrict__ src, const long long* __restrict__ order,
                       const long long* __restrict__ offs, long long items, int D, float* __restrict__ out) {
  const int code = blockIdx.x;
  long long beg = offs[code], end = offs[code + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > items ? items : end;
  for (int d = threadIdx.x; d < D; d += kRowThreads) {
    float s = 0.f;
    for (long long i = beg; i < end; ++i) {
      const long long it = order[i];
      if (it >= 0 && it < items) s += src[it * D + d];
    }
    out[(long long)code * D + d] = s;
  }
}

}  // namespace

// out (N, V - 1) fp32: the one-hot rows of ids (N) int32 with a zero row for `blank`.
SBK_API int sbk_embed_onehot(const int* ids, int N, int V, int blank, float* out, void* stream) {
  if (!ids || !out || N <= 0 || V <= 1 || blank < 0 || blank >= V) return SBK_ERR_ARG;
  hipLaunchKernelGGL(embed_onehot_kernel, dim3(N), dim3(kRowThreads), 0, (hipStream_t)stream, ids, blank, V - 1, out);
  SBK_CHECK_LAUNCH();
  return 0;
}

// out (N, D) fp32 = weight (V, D)[ids (N) int32].
SBK_API int sbk_embed_gather(const int* ids, const float* weight, int N, int V, int D, float* out, void* stream) {
  if (!ids || !weight || !out || N <= 0 || V <= 0 || D <= 0) return SBK_ERR_ARG;
  hipLaunchKernelGGL(embed_gather_kernel, dim3(N), dim3(kRowThreads), 0, (hipStream_t)stream, ids, weight, V, D, out);
  SBK_CHECK_LAUNCH();
  return 0;
}

// out (ncodes, D) fp32: per-code sums of the rows of src (items, D) fp32 over
// order (items) int64 — row ids stably sorted by code — and offs (ncodes + 1)
// int64, the start of every code's run.  Rows are added in list order: no
// atomics, run-to-run identical.
SBK_API int sbk_segsum_rows(const float* src, const long long* order, const long long* offs, long long items,
                            int ncodes, int D, float* out, void* stream) {
  if (!src || !order || !offs || !out || items <= 0 || ncodes <= 0 || D <= 0) return SBK_ERR_ARG;
  hipLaunchKernelGGL(segsum_rows_kernel, dim3(ncodes), dim3(kRowThreads), 0, (hipStream_t)stream, src, order, offs, items,
                     D, out);
  SBK_CHECK_LAUNCH();
  return 0;
}
