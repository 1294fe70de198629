// GRU recurrence of the transducer prediction network (nnet/RNN.py:280-388 of
// the reference, torch.nn.GRU semantics, gate order r, z, n) and the kernels
// of the Embedding drop-in (nnet/embedding.py:14-114).
//
//   r = sigmoid(gi_r + W_hr h + b_hr)        z = sigmoid(gi_z + W_hz h + b_hz)
//   q = W_hn h + b_hn                        n = tanh(gi_n + r * q)
//   h_t = (1 - z) * n + z * h_{t-1}
//
// One launch per time step, forward and backward; the dependency between
// steps is stream order.  No persistent kernel, no grid barrier, no flag
// between workgroups, no float atomics.  sbk_gru_fwd / sbk_gru_bwd enqueue
// the T launches of a sequence from the host side of the library, so a
// sequence costs one call into the library.
//
// Forward step t, grid (ceil(H / 16), ceil(B / 32)), 8 waves.  A workgroup
// owns 16 hidden units and up to 32 batch rows: the three 16-column tiles
// W_hh[g * H + j0 .. j0 + 16, :] (g = r, z, n) are MFMA B operands read from
// memory as they are (8 consecutive K elements per lane), h_{t-1} rows are the
// A operand (fp32 state, rounded to bf16 in bf16 mode; exact-fp32 MFMA in
// fp32 mode).  The K range is dealt to the eight waves in 32-element chunks;
// their partial tiles meet in LDS and are added in wave order.  The epilogue
// adds the input pre-activations — rows of the dense gi (B, T, 3H), or rows of
// the W_ih^T table gathered by token id (one-hot input; the blank adds b_ih
// only) — applies the gates and writes h_t.  Step t reads state[:, t-1, :]
// (hx at t = 0) and writes state[:, t, :]: nothing is updated in place.
// With lengths, a row with t >= len_b keeps its state (state[b, t] =
// state[b, t-1]) and its output row y[b, t] is zero.  When training, r, z, n
// and q are kept in save (B, T, 4, H).
//
// Backward step t = T-1 .. 0, same grid.  The workgroup of units J forms
//   dh_t[:, J] = dy_t[:, J] + z_{t+1} * dh_{t+1}[:, J] + dgh_{t+1} . W_hh[:, J]
// (the product on MFMA against W_hh^T (H, 3H), K = 3H dealt to the waves; a
// row masked at t+1 passes dh_{t+1} through), then the gate gradients of its
// units from the saved activations, and writes dgi_t, dgh_t = (dr, dz, dn * r).
// One more launch of the carry part alone gives dhx.  dh ping-pongs between
// the two halves of a (2, B, H) buffer.
#include "mfma.h"

using namespace sbk;

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = 8;
constexpr int kSlice = 16;  // hidden units of a workgroup: one MFMA tile
constexpr int kRows = 32;   // batch rows of a workgroup
constexpr int kRowThreads = 256;  // the row kernels of the Embedding
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

struct FwdArgs {
  const void* w_hh;      // (3H, H) in the compute dtype
  const float* b_hh;     // (3H) or null
  const float* hx;       // (B, H) or null
  const float* gi;       // (B, T, 3H) or null
  const int* tok;        // (B, T) or null
  const float* table;    // (I, 3H): W_ih^T
  const float* b_ih;     // (3H) or null (token mode)
  const int* lens;       // (B) or null
  float* state;          // (B, T, H)
  float* y;              // (B, T, H) or null
  float* save;           // (B, T, 4, H) or null
  int blank, I, B, T, H;
  int vec_w, vec_h;
};

template <typename T>
__global__ void __launch_bounds__(kThreads) gru_fwd_step_kernel(FwdArgs a, int t) {
  __shared__ float red[kWaves][3][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, B = a.B, Tn = a.T;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const float* hprev = t == 0 ? a.hx : a.state + (long long)(t - 1) * H;
  const long long ldh = t == 0 ? H : (long long)Tn * H;
  const bool vec_h = a.vec_h;

  f32x4 acc[kMT][3];
#pragma unroll
  for (int m = 0; m < kMT; ++m)
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (hprev) {
    const T* W = static_cast<const T*>(a.w_hh);
    const int unit = j0 + (lane & 15);
#pragma unroll 2
    for (int k0 = w * 32; k0 < H; k0 += kWaves * 32) {
      const int kk = k0 + 8 * (lane >> 4);
      typename MT<T>::frag bw[3];
#pragma unroll
      for (int g = 0; g < 3; ++g)
        bw[g] = unit < H ? load_w8<T>(W + ((long long)g * H + unit) * H, kk, H, a.vec_w) : MT<T>::zero();
#pragma unroll
      for (int m = 0; m < kMT; ++m) {
        if (m < mts) {
          const int row = b0 + m * 16 + (lane & 15);
          const typename MT<T>::frag af =
              row < B ? load_f8<T>(hprev + row * ldh, kk, H, vec_h) : MT<T>::zero();
#pragma unroll
          for (int g = 0; g < 3; ++g) MT<T>::mma(acc[m][g], af, bw[g]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < kMT; ++m) {
    if (m < mts) {
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][g][m * 16 + 4 * (lane >> 4) + r][lane & 15] = acc[m][g][r];
    }
  }
  __syncthreads();

  const long long H3 = 3LL * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      float s = red[0][g][rr][jj];
#pragma unroll
      for (int ww = 1; ww < kWaves; ++ww) s += red[ww][g][rr][jj];
      gh[g] = a.b_hh ? s + a.b_hh[g * H + j] : s;
    }
    const long long bt = (long long)b * Tn + t;
    float gi[3];
    if (a.tok) {
      const int v = a.tok[bt];
      const int idx = v == a.blank ? -1 : (v < a.blank ? v : v - 1);
      const bool hit = idx >= 0 && idx < a.I;
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const float x = hit ? a.table[idx * H3 + g * H + j] : 0.f;
        gi[g] = a.b_ih ? x + a.b_ih[g * H + j] : x;
      }
    } else {
#pragma unroll
      for (int g = 0; g < 3; ++g) gi[g] = a.gi[bt * H3 + g * H + j];
    }
    const float hp = hprev ? hprev[b * ldh + j] : 0.f;
    const float r = sigmoid_exact(gi[0] + gh[0]);
    const float z = sigmoid_exact(gi[1] + gh[1]);
    const float q = gh[2];
    const float n = tanhf(gi[2] + r * q);
    const float h = (1.f - z) * n + z * hp;
    const bool active = !a.lens || t < a.lens[b];
    a.state[bt * H + j] = active ? h : hp;
    if (a.y) a.y[bt * H + j] = active ? h : 0.f;
    if (a.save) {
      float* s = a.save + bt * 4 * H + j;
      s[0] = r;
      s[H] = z;
      s[2 * H] = n;
      s[3 * H] = q;
    }
  }
}

struct BwdArgs {
  const void* w_hhT;     // (H, 3H) in the compute dtype
  const float* hx;       // (B, H) or null
  const float* state;    // (B, T, H)
  const float* save;     // (B, T, 4, H)
  const float* dy;       // (B, T, H) or null
  const float* dhn;      // (B, H) or null
  const int* lens;       // (B) or null
  float* dgi;            // (B, T, 3H)
  float* dgh;            // (B, T, 3H)
  float* dhw;            // (2, B, H)
  float* dhx;            // (B, H)
  int B, T, H;
  int vec_w, vec_g;
};

// t in [-1, T-1]; t = -1 computes the carry into dhx only
template <typename T>
__global__ void __launch_bounds__(kThreads) gru_bwd_step_kernel(BwdArgs a, int t) {
  __shared__ float red[kWaves][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, B = a.B, Tn = a.T;
  const int K = 3 * H;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const int s = t + 1;  // the step whose gradients arrive

  f32x4 acc[kMT];
#pragma unroll
  for (int m = 0; m < kMT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s < Tn) {
    const T* W = static_cast<const T*>(a.w_hhT);
    const int unit = j0 + (lane & 15);
#pragma unroll 2
    for (int k0 = w * 32; k0 < K; k0 += kWaves * 32) {
      const int kk = k0 + 8 * (lane >> 4);
      const typename MT<T>::frag bw =
          unit < H ? load_w8<T>(W + (long long)unit * K, kk, K, a.vec_w) : MT<T>::zero();
#pragma unroll
      for (int m = 0; m < kMT; ++m) {
        if (m < mts) {
          const int row = b0 + m * 16 + (lane & 15);
          const typename MT<T>::frag af =
              row < B ? load_f8<T>(a.dgh + ((long long)row * Tn + s) * K, kk, K, a.vec_g) : MT<T>::zero();
          MT<T>::mma(acc[m], af, bw);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < kMT; ++m) {
    if (m < mts) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[w][m * 16 + 4 * (lane >> 4) + r][lane & 15] = acc[m][r];
    }
  }
  __syncthreads();

  const long long BH = (long long)B * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    const long long bj = (long long)b * H + j;
    float carry;
    if (s >= Tn) {
      carry = a.dhn ? a.dhn[bj] : 0.f;
    } else {
      const float dnext = a.dhw[(s & 1) * BH + bj];
      if (!a.lens || s < a.lens[b]) {
        float mm = red[0][rr][jj];
#pragma unroll
        for (int ww = 1; ww < kWaves; ++ww) mm += red[ww][rr][jj];
        const float zn = a.save[((long long)b * Tn + s) * 4 * H + H + j];
        carry = zn * dnext + mm;
      } else {
        carry = dnext;
      }
    }
    if (t < 0) {
      a.dhx[bj] = carry;
      continue;
    }
    const long long bt = (long long)b * Tn + t;
    const bool active = !a.lens || t < a.lens[b];
    const float dh = carry + (active && a.dy ? a.dy[bt * H + j] : 0.f);
    a.dhw[(t & 1) * BH + bj] = dh;
    float dr = 0.f, dz = 0.f, dn = 0.f, dnr = 0.f;
    if (active) {
      const float* sv = a.save + bt * 4 * H + j;
      const float r = sv[0], z = sv[H], n = sv[2 * H], q = sv[3 * H];
      const float hp = t == 0 ? (a.hx ? a.hx[bj] : 0.f) : a.state[(bt - 1) * H + j];
      dn = dh * (1.f - z) * (1.f - n * n);
      dz = dh * (hp - n) * z * (1.f - z);
      dr = dn * q * r * (1.f - r);
      dnr = dn * r;
    }
    float* gi = a.dgi + bt * K + j;
    float* gh = a.dgh + bt * K + j;
    gi[0] = dr;
    gi[H] = dz;
    gi[2 * H] = dn;
    gh[0] = dr;
    gh[H] = dz;
    gh[2 * H] = dnr;
  }
}

// out (N, D) = rows of the one-hot table of Embedding(consider_as_one_hot):
// D = V - 1 columns, the blank row zero, ids above the blank shifted down
__global__ void __launch_bounds__(kRowThreads)
    embed_onehot_kernel(const int* __restrict__ ids, int blank, int D, float* __restrict__ out) {
  const int v = ids[blockIdx.x];
  const int idx = v == blank ? -1 : (v < blank ? v : v - 1);
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

// The T forward steps of one GRU layer.  bf16: w_hh is bf16 (else fp32), both
// (3H, H) row-major.  Input pre-activations: gi (B, T, 3H) fp32 with b_ih
// already added, or tok (B, T) int32 token ids with table = W_ih^T (I, 3H)
// fp32 and b_ih (token id `blank` has no row; ids above it use row id - 1).
// hx (B, H) or null (zeros).  lens (B) int32 steps per row, or null.
// state (B, T, H): the carried state after every step; y (B, T, H) or null:
// the output (zero past a row's length); save (B, T, 4, H) or null: r, z, n, q.
SBK_API int sbk_gru_fwd(int bf16, const void* w_hh, const float* b_hh, const float* hx, const float* gi,
                        const int* tok, int blank, const float* table, int I, const float* b_ih, const int* lens,
                        int B, int T, int H, float* state, float* y, float* save, void* stream) {
  if (!w_hh || !state || (!gi && !tok) || (gi && tok)) return SBK_ERR_ARG;
  if (tok && (!table || I <= 0)) return SBK_ERR_ARG;
  if (B <= 0 || T <= 0 || H <= 0) return SBK_ERR_ARG;
  if ((long long)3 * H * H > 0x7fffffffLL || (long long)B * T > 0x7fffffffLL / 4) return SBK_ERR_ARG;
  FwdArgs a;
  a.w_hh = w_hh; a.b_hh = b_hh; a.hx = hx; a.gi = gi; a.tok = tok; a.table = table; a.b_ih = b_ih; a.lens = lens;
  a.state = state; a.y = y; a.save = save;
  a.blank = blank; a.I = I; a.B = B; a.T = T; a.H = H;
  a.vec_w = aligned16(w_hh) && H % (bf16 ? 8 : 4) == 0;
  a.vec_h = aligned16(state) && H % 4 == 0 && (!hx || aligned16(hx));
  const dim3 grid((H + kSlice - 1) / kSlice, (B + kRows - 1) / kRows);
  for (int t = 0; t < T; ++t) {
    if (bf16)
      hipLaunchKernelGGL(gru_fwd_step_kernel<bf16_t>, grid, dim3(kThreads), 0, (hipStream_t)stream, a, t);
    else
      hipLaunchKernelGGL(gru_fwd_step_kernel<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a, t);
    SBK_CHECK_LAUNCH();
  }
  return 0;
}

// The backward steps t = T-1 .. 0 and the carry into dhx.  w_hhT = W_hh^T
// (H, 3H) in the compute dtype; state and save as sbk_gru_fwd wrote them; dy
// (B, T, H) or null, dhn (B, H) or null.  Writes dgi, dgh (B, T, 3H) fp32
// (zero rows past a row's length), dhx (B, H); dhw (2, B, H) is scratch.
SBK_API int sbk_gru_bwd(int bf16, const void* w_hhT, const float* hx, const float* state, const float* save,
                        const float* dy, const float* dhn, const int* lens, int B, int T, int H, float* dgi,
                        float* dgh, float* dhw, float* dhx, void* stream) {
  if (!w_hhT || !state || !save || !dgi || !dgh || !dhw || !dhx) return SBK_ERR_ARG;
  if (B <= 0 || T <= 0 || H <= 0) return SBK_ERR_ARG;
  if ((long long)3 * H * H > 0x7fffffffLL || (long long)B * T > 0x7fffffffLL / 4) return SBK_ERR_ARG;
  BwdArgs a;
  a.w_hhT = w_hhT; a.hx = hx; a.state = state; a.save = save; a.dy = dy; a.dhn = dhn; a.lens = lens;
  a.dgi = dgi; a.dgh = dgh; a.dhw = dhw; a.dhx = dhx;
  a.B = B; a.T = T; a.H = H;
  a.vec_w = aligned16(w_hhT) && (3 * H) % (bf16 ? 8 : 4) == 0;
  a.vec_g = aligned16(dgh) && (3 * H) % 4 == 0;
  const dim3 grid((H + kSlice - 1) / kSlice, (B + kRows - 1) / kRows);
  for (int t = T - 1; t >= -1; --t) {
    if (bf16)
      hipLaunchKernelGGL(gru_bwd_step_kernel<bf16_t>, grid, dim3(kThreads), 0, (hipStream_t)stream, a, t);
    else
      hipLaunchKernelGGL(gru_bwd_step_kernel<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a, t);
    SBK_CHECK_LAUNCH();
  }
  return 0;
}

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
