// The wav2vec 2.0 pre-training objective (fp32): the contrastive loss of
// speechbrain/nnet/losses.py:1198-1251 and the Gumbel vector quantiser of
// speechbrain/nnet/quantisers.py:13-123, without their temporaries.
//
// Contrastive loss.  Row r = (b, t) of x (R, C) is scored against N + 1
// candidate rows: candidate 0 is the positive y[r], candidate j >= 1 is
//   float mode   negs[j-1][r]      (the reference's (N, B, T, C) tensor, read in place)
//   index mode   y[idx[r][j-1]]    (negs is never built)
//   logit_j = cos(x_r, c_j) / temp
//   cos(a, b) = <a, b> / (max(|a|, eps) * max(|b|, eps)),  eps = 1e-8
// which is torch.cosine_similarity's formula (each vector divided by its
// clamped norm; checked on the CPU against torch 2.10 with rows of norm
// < eps: the older <a,b> / sqrt(max(|a|²|b|², eps²)) form differs there).
// A negative equal to y[r] element for element gets logit -inf (neg_is_pos).
//   rowloss_r = logsumexp_j(logit_j) - logit_0,   correct_r = [logit_0 is the row maximum]
// Backward, with w_j = go * (softmax_j - [j == 0]) / temp (0 for a -inf
// candidate), a_j = w_j / (max(|x|, eps) max(|c_j|, eps)) and
// b_j = [|c_j| > eps] w_j cos_j / |c_j|²:
//   dx_r   = sum_j a_j c_j - [|x| > eps] (sum_j w_j cos_j) / |x|² · x
//   dc_j   = a_j x_r - b_j c_j
// In float mode every candidate row is referenced once, so dnegs and the
// positive's dy are written directly.  In index mode dy is a scatter: the
// x-kernel stores (a_j, b_j) per (row, candidate) pair and the y-kernel sums,
// per target row, the pairs of a precomputed inverse index in their sorted
// order — no float atomics, bitwise reproducible.
//
// Quantiser.  Per (row, group) of the (Rq, G, V) logits: arg-max (lowest
// index on ties), hard-code counts (integer atomics), softmax column sums
// (per-wave partial rows, reduced afterwards), the chosen code and, in
// training, y_soft = softmax((logits + gumbels) / tau); the output row is the
// chosen rows of vars, concatenated over groups.  Straight-through backward:
//   gy[v] = <dout_g, vars[g V + v]>,  dlogits = y_soft (gy - sum_v gy y_soft) / tau
//   dvars[code] = sum of dout_g over the (row, group) items that chose it (sorted lists).
#include "sbk_common.h"

using namespace sbk;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kBatch = 4;  // candidates a wave loads and reduces together
constexpr float kCosEps = 1e-8f;
constexpr int kMaxLds = 64 * 1024;

__device__ __forceinline__ int rup4(int n) { return (n + 3) & ~3; }

template <bool INDEX>
__device__ __forceinline__ const float* cand_row(const float* y, const float* negs, const int* idx, long long r, int j,
                                                 int R, int N, int C, long long s_row, long long s_neg) {
  if (j == 0) return y + r * C;
  if constexpr (INDEX) {
    int q = idx[r * N + (j - 1)];
    q = q < 0 ? 0 : (q >= R ? R - 1 : q);  // never read outside y
    return y + (long long)q * C;
  } else {
    return negs + r * s_row + (long long)(j - 1) * s_neg;
  }
}

// sums of squares of up to kBatch candidate rows at once (all lanes get them)
template <bool VEC>
__device__ __forceinline__ void cand_sqnorms(const float* const* p, int C, int lane, float* nn) {
#pragma unroll
  for (int u = 0; u < kBatch; ++u) nn[u] = 0.f;
  if constexpr (VEC) {
    for (int c = lane; c < C / 4; c += kWave) {
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const float4 v = reinterpret_cast<const float4*>(p[u])[c];
        nn[u] += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      }
    }
  } else {
    for (int c = lane; c < C; c += kWave) {
#pragma unroll
      for (int u = 0; u < kBatch; ++u) nn[u] += p[u][c] * p[u][c];
    }
  }
#pragma unroll
  for (int u = 0; u < kBatch; ++u) nn[u] = wave_sum_v(nn[u]);
}

// grid R, one workgroup per row; wave w takes candidates in batches of kBatch.
// Dynamic LDS: x row, y row (rup4(C) floats each), 16 reduction floats, N + 1 logits.
template <bool INDEX, bool VEC>
__global__ void __launch_bounds__(kThreads)
    contrast_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ negs,
                        const int* __restrict__ idx, int R, int C, int N, long long s_row, long long s_neg, float temp,
                        float* __restrict__ logits, float* __restrict__ rowloss, float* __restrict__ correct,
                        float* __restrict__ aux) {
  extern __shared__ float4 smem4[];
  const int Cp = rup4(C);
  float* sx = reinterpret_cast<float*>(smem4);
  float* sy = sx + Cp;
  float* red = sy + Cp;
  float* sl = red + 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long r = blockIdx.x;
  float nx2 = 0.f;
  for (int c = tid; c < C; c += kThreads) {
    const float a = x[r * C + c];
    sx[c] = a;
    sy[c] = y[r * C + c];
    nx2 += a * a;
  }
  nx2 = block_sum(nx2, red);  // its barriers publish sx / sy
  const float nx = sqrtf(nx2);
  const float nxc = fmaxf(nx, kCosEps);

  for (int jb = w * kBatch; jb <= N; jb += kWaves * kBatch) {
    const float* p[kBatch];
    float dot[kBatch], nn[kBatch];
    int eq[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int j = jb + u <= N ? jb + u : 0;  // a slot past the end re-reads the positive, result unused
      p[u] = cand_row<INDEX>(y, negs, idx, r, j, R, N, C, s_row, s_neg);
      dot[u] = 0.f;
      nn[u] = 0.f;
      eq[u] = 1;
    }
    if constexpr (VEC) {
      for (int c = lane; c < C / 4; c += kWave) {
        const float4 xv = reinterpret_cast<const float4*>(sx)[c];
        const float4 yv = reinterpret_cast<const float4*>(sy)[c];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const float4 v = reinterpret_cast<const float4*>(p[u])[c];
          dot[u] += v.x * xv.x + v.y * xv.y + v.z * xv.z + v.w * xv.w;
          nn[u] += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
          eq[u] &= (v.x == yv.x) & (v.y == yv.y) & (v.z == yv.z) & (v.w == yv.w);
        }
      }
    } else {
      for (int c = lane; c < C; c += kWave) {
        const float xv = sx[c], yv = sy[c];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const float v = p[u][c];
          dot[u] += v * xv;
          nn[u] += v * v;
          eq[u] &= (v == yv);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      dot[u] = wave_sum_v(dot[u]);
      nn[u] = wave_sum_v(nn[u]);
      const int same = __all(eq[u]);
      const int j = jb + u;
      if (lane == 0 && j <= N) {
        const float cs = dot[u] / (nxc * fmaxf(sqrtf(nn[u]), kCosEps));
        sl[j] = (j > 0 && same) ? -INFINITY : cs / temp;
      }
    }
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = tid; j <= N; j += kThreads) m = fmaxf(m, sl[j]);
  m = block_max(m, red);
  float s = 0.f;
  for (int j = tid; j <= N; j += kThreads) s += expf(sl[j] - m);
  s = block_sum(s, red);
  for (int j = tid; j <= N; j += kThreads) logits[r * (N + 1) + j] = sl[j];
  if (tid == 0) {
    rowloss[r] = (m + logf(s)) - sl[0];
    correct[r] = sl[0] == m ? 1.f : 0.f;  // argmax == 0: the first maximum wins a tie
    aux[2 * r] = nx;
    aux[2 * r + 1] = m + logf(s);
  }
}

// grid R.  Writes dx; float mode: dnegs ([r][j-1][C]) and the positive's dy
// (either may be null); index mode: the pair coefficients ca / cb (R, N + 1).
// Dynamic LDS: x row, y row, kWaves accumulator rows (rup4(C) each), 16 floats.
template <bool INDEX, bool VEC>
__global__ void __launch_bounds__(kThreads)
    contrast_bwd_x_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ negs,
                          const int* __restrict__ idx, const float* __restrict__ logits,
                          const float* __restrict__ aux, const float* __restrict__ go, int R, int C, int N, long long s_row, long long s_neg,
                          float temp, float* __restrict__ dx, float* __restrict__ dy, float* __restrict__ dnegs,
                          float* __restrict__ ca, float* __restrict__ cb) {
  extern __shared__ float4 smem4[];
  const int Cp = rup4(C);
  float* sx = reinterpret_cast<float*>(smem4);
  float* sy = sx + Cp;
  float* acc = sy + Cp;
  float* red = acc + kWaves * Cp;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long r = blockIdx.x;
  for (int c = tid; c < C; c += kThreads) {
    sx[c] = x[r * C + c];
    sy[c] = y[r * C + c];
  }
  float* my = acc + w * Cp;
  for (int c = lane; c < Cp; c += kWave) my[c] = 0.f;
  __syncthreads();
  const float g = go[r];
  const float* lr = logits + r * (N + 1);
  const float nx = aux[2 * r], lse = aux[2 * r + 1];
  const float nxc = fmaxf(nx, kCosEps);
  float swc = 0.f;  // sum of w_j cos_j over this wave's candidates (wave-uniform)

  for (int jb = w * kBatch; jb <= N; jb += kWaves * kBatch) {
    const float* p[kBatch];
    float nn[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      p[u] = cand_row<INDEX>(y, negs, idx, r, jb + u <= N ? jb + u : 0, R, N, C, s_row, s_neg);
    cand_sqnorms<VEC>(p, C, lane, nn);
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int j = jb + u;
      if (j > N) break;
      const float lg = lr[j];
      float wj = 0.f;
      if (lg != -INFINITY) wj = g * (expf(lg - lse) - (j == 0 ? 1.f : 0.f)) / temp;
      const float cs = lg * temp;
      const float nc = sqrtf(nn[u]);
      const float a = wj == 0.f ? 0.f : wj / (nxc * fmaxf(nc, kCosEps));
      const float b = (wj == 0.f || !(nc > kCosEps)) ? 0.f : wj * cs / nn[u];
      if (wj != 0.f) swc += wj * cs;
      if constexpr (INDEX) {
        if (lane == 0) {
          ca[r * (N + 1) + j] = a;
          cb[r * (N + 1) + j] = b;
        }
      }
      float* dc = nullptr;  // where this candidate's own gradient goes (float mode)
      if constexpr (!INDEX) {
        if (j == 0) dc = dy ? dy + r * C : nullptr;
        else dc = dnegs ? dnegs + (r * N + (j - 1)) * C : nullptr;
      }
      if (wj == 0.f) {
        if (dc)
          for (int c = lane; c < C; c += kWave) dc[c] = 0.f;
        continue;
      }
      if constexpr (VEC) {
        for (int c = lane; c < C / 4; c += kWave) {
          const float4 v = reinterpret_cast<const float4*>(p[u])[c];
          float4 t = reinterpret_cast<float4*>(my)[c];
          t.x += a * v.x, t.y += a * v.y, t.z += a * v.z, t.w += a * v.w;
          reinterpret_cast<float4*>(my)[c] = t;
          if (dc) {
            const float4 xv = reinterpret_cast<const float4*>(sx)[c];
            reinterpret_cast<float4*>(dc)[c] =
                make_float4(a * xv.x - b * v.x, a * xv.y - b * v.y, a * xv.z - b * v.z, a * xv.w - b * v.w);
          }
        }
      } else {
        for (int c = lane; c < C; c += kWave) {
          const float v = p[u][c];
          my[c] += a * v;
          if (dc) dc[c] = a * sx[c] - b * v;
        }
      }
    }
  }
  if (lane == 0) red[w] = swc;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) tot += red[i];
  const float kx = nx > kCosEps ? tot / (nx * nx) : 0.f;
  for (int c = tid; c < C; c += kThreads) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) s += acc[i * Cp + c];
    dx[r * C + c] = s - kx * sx[c];
  }
}

// Index mode: grid R, one workgroup per target row q.  order: the pair ids
// r (N + 1) + j sorted (stably) by the target row they reference; offs (R + 1):
// where each row's list starts.  dy[q] = sum ca[p] x[r(p)] - (sum cb[p]) y[q],
// every wave over its pairs in list order, the waves added in wave order.
// Dynamic LDS: kWaves accumulator rows of rup4(C) floats, 16 floats.
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
    contrast_bwd_y_kernel(const float* __restrict__ x, const float* __restrict__ y,
                          const long long* __restrict__ order, const long long* __restrict__ offs,
                          const float* __restrict__ ca, const float* __restrict__ cb, int R, int C, int N,
                          float* __restrict__ dy) {
  extern __shared__ float4 smem4[];
  const int Cp = rup4(C);
  float* acc = reinterpret_cast<float*>(smem4);
  float* red = acc + kWaves * Cp;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long q = blockIdx.x;
  float* my = acc + w * Cp;
  for (int c = lane; c < Cp; c += kWave) my[c] = 0.f;
  __syncthreads();
  const long long npairs = (long long)R * (N + 1);
  long long beg = offs[q], end = offs[q + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > npairs ? npairs : end;
  float sb = 0.f;
  for (long long i = beg + w; i < end; i += kWaves) {
    const long long pr = order[i];
    if (pr < 0 || pr >= npairs) continue;
    const float a = ca[pr], b = cb[pr];
    sb += b;
    if (a == 0.f) continue;
    const float* xr = x + (pr / (N + 1)) * C;
    if constexpr (VEC) {
      for (int c = lane; c < C / 4; c += kWave) {
        const float4 v = reinterpret_cast<const float4*>(xr)[c];
        float4 t = reinterpret_cast<float4*>(my)[c];
        t.x += a * v.x, t.y += a * v.y, t.z += a * v.z, t.w += a * v.w;
        reinterpret_cast<float4*>(my)[c] = t;
      }
    } else {
      for (int c = lane; c < C; c += kWave) my[c] += a * xr[c];
    }
  }
  if (lane == 0) red[w] = sb;
  __syncthreads();
  float tb = 0.f;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) tb += red[i];
  for (int c = tid; c < C; c += kThreads) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) s += acc[i * Cp + c];
    dy[q * C + c] = s - tb * y[q * C + c];
  }
}

// ---------------------------------------------------------------- quantiser

// (value, index) arg-max over the wave: larger value wins, lower index on a tie
__device__ __forceinline__ void wave_argmax(float& m, int& mi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o);
    const int oi = __shfl_xor(mi, o);
    if (om > m || (om == m && oi < mi)) {
      m = om;
      mi = oi;
    }
  }
}

// One wave per (row, group) item, items strided over all waves of the grid.
// Dynamic LDS: per wave G*V floats of softmax column sums (lane-owned columns);
// part (gridDim.x * kWaves, G*V) receives every wave's sums.
__global__ void __launch_bounds__(kThreads)
    gumbel_vq_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ gum, float inv_tau, int Rq, int G,
                         int V, const float* __restrict__ vars, int D, float* __restrict__ out,
                         int* __restrict__ codes, int* __restrict__ counts, float* __restrict__ part,
                         float* __restrict__ ysoft) {
  extern __shared__ float4 smem4[];
  const int GV = G * V;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* acc = reinterpret_cast<float*>(smem4) + (long long)w * GV;
  for (int i = lane; i < GV; i += kWave) acc[i] = 0.f;
  const long long items = (long long)Rq * G;
  const long long wid = (long long)blockIdx.x * kWaves + w, nw = (long long)gridDim.x * kWaves;
  for (long long it = wid; it < items; it += nw) {
    const int g = (int)(it % G);
    const float* l = logits + it * V;
    const float* gn = gum ? gum + it * V : nullptr;
    float m = -INFINITY, m2 = -INFINITY;
    int mi = 0x7fffffff, mi2 = 0x7fffffff;
    for (int v = lane; v < V; v += kWave) {
      const float a = l[v];
      if (a > m) m = a, mi = v;
      if (gn) {
        const float b = a + gn[v];
        if (b > m2) m2 = b, mi2 = v;
      }
    }
    wave_argmax(m, mi);
    if (gn) wave_argmax(m2, mi2);
    float s = 0.f, s2 = 0.f;
    for (int v = lane; v < V; v += kWave) {
      const float a = l[v];
      s += expf(a - m);
      if (gn) s2 += expf(((a + gn[v]) - m2) * inv_tau);
    }
    s = wave_sum_v(s);
    if (gn) s2 = wave_sum_v(s2);
    const float is = 1.f / s, is2 = gn ? 1.f / s2 : 0.f;
    for (int v = lane; v < V; v += kWave) {
      const float a = l[v];
      acc[g * V + v] += expf(a - m) * is;
      if (gn) ysoft[it * V + v] = expf(((a + gn[v]) - m2) * inv_tau) * is2;
    }
    if (mi >= V) mi = 0;  // a row without an ordered maximum (NaN): stay inside vars
    if (mi2 >= V) mi2 = 0;
    const int k = gn ? mi2 : mi;
    if (lane == 0) {
      codes[it] = g * V + k;
      atomicAdd(&counts[g * V + mi], 1);  // integer: exact in any order
    }
    const float* vr = vars + (long long)(g * V + k) * D;
    float* o = out + it * D;  // row (it / G), columns [g D, (g+1) D)
    for (int d = lane; d < D; d += kWave) o[d] = vr[d];
  }
  float* pw = part + wid * GV;
  for (int i = lane; i < GV; i += kWave) pw[i] = acc[i];
}

constexpr int kQRows = 16;   // (row, group) items of one group per workgroup
constexpr int kQChunk = 256;  // dout columns staged per step

// grid (ceil(Rq / kQRows), G).  Thread t owns code columns v = t, t + 256, ...
// of group g for kQRows rows: gy = <dout_g[row], vars[gV + v]> over D in LDS
// chunks, stored to dlogits as scratch, then dlogits = ys (gy - <gy, ys>) / tau.
__global__ void __launch_bounds__(kThreads)
    gumbel_vq_dlogits_kernel(const float* __restrict__ dout, const float* __restrict__ vars,
                             const float* __restrict__ ysoft, float inv_tau, int Rq, int G, int V, int D,
                             float* __restrict__ dlogits) {
  __shared__ float4 sd4[kQChunk][kQRows / 4];  // [d][row]: a thread reads its 16 rows of one d as 4 x 16 bytes
  float(*sd)[kQRows] = reinterpret_cast<float(*)[kQRows]>(sd4);
  __shared__ float red[kWaves][kQRows];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * kQRows;
  const int rows = (int)((long long)Rq - row0 < kQRows ? (long long)Rq - row0 : kQRows);
  float t[kQRows];
#pragma unroll
  for (int i = 0; i < kQRows; ++i) t[i] = 0.f;
  for (int v0 = 0; v0 < V; v0 += kThreads) {
    const int v = v0 + tid;
    float gy[kQRows];
#pragma unroll
    for (int i = 0; i < kQRows; ++i) gy[i] = 0.f;
    for (int d0 = 0; d0 < D; d0 += kQChunk) {
      const int dn = D - d0 < kQChunk ? D - d0 : kQChunk;
      __syncthreads();
      for (int e = tid; e < kQRows * kQChunk; e += kThreads) {
        const int i = e / kQChunk, d = e % kQChunk;
        sd[d][i] = (i < rows && d < dn) ? dout[((row0 + i) * G + g) * D + d0 + d] : 0.f;
      }
      __syncthreads();
      if (v < V) {
        const float* vr = vars + ((long long)g * V + v) * D + d0;
        for (int d = 0; d < dn; ++d) {
          const float a = vr[d];
#pragma unroll
          for (int i4 = 0; i4 < kQRows / 4; ++i4) {
            const float4 q = sd4[d][i4];
            gy[4 * i4] += a * q.x, gy[4 * i4 + 1] += a * q.y, gy[4 * i4 + 2] += a * q.z, gy[4 * i4 + 3] += a * q.w;
          }
        }
      }
    }
    if (v < V) {
#pragma unroll
      for (int i = 0; i < kQRows; ++i) {
        if (i < rows) {
          const long long e = ((row0 + i) * G + g) * V + v;
          dlogits[e] = gy[i];
          t[i] += gy[i] * ysoft[e];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kQRows; ++i) t[i] = wave_sum_v(t[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kQRows; ++i) red[w][i] = t[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kQRows; ++i) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s += red[k][i];
    t[i] = s;
  }
  for (int v = tid; v < V; v += kThreads) {  // the same thread re-reads what it stored
#pragma unroll
    for (int i = 0; i < kQRows; ++i) {
      if (i < rows) {
        const long long e = ((row0 + i) * G + g) * V + v;
        dlogits[e] = ysoft[e] * (dlogits[e] - t[i]) * inv_tau;
      }
    }
  }
}

// One wave per (row, group) item: the gradient of the softmax column sums,
// dlogits (+)= p (gp - <p, gp>) with p = softmax(logits) and gp (G*V) the
// gradient of the sums.
__global__ void __launch_bounds__(kThreads)
    softmax_colsum_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ gp, int Rq, int G, int V,
                              int accumulate, float* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long items = (long long)Rq * G;
  const long long nw = (long long)gridDim.x * kWaves;
  for (long long it = (long long)blockIdx.x * kWaves + w; it < items; it += nw) {
    const float* l = logits + it * V;
    const float* gg = gp + (it % G) * V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += kWave) m = fmaxf(m, l[v]);
    m = wave_max(m);
    float s = 0.f, t = 0.f;
    for (int v = lane; v < V; v += kWave) {
      const float e = expf(l[v] - m);
      s += e;
      t += e * gg[v];
    }
    s = wave_sum_v(s);
    t = wave_sum_v(t);
    const float is = 1.f / s;
    t *= is;
    for (int v = lane; v < V; v += kWave) {
      const float d = expf(l[v] - m) * is * (gg[v] - t);
      dlogits[it * V + v] = accumulate ? dlogits[it * V + v] + d : d;
    }
  }
}

// grid G*V, one workgroup per code.  order: (row, group) item ids sorted
// (stably) by their code; offs (G*V + 1).  Wave w sums the w-th quarter of the
// list in order; the four partial rows are added in wave order.
__global__ void __launch_bounds__(kThreads)
    gumbel_vq_dvars_kernel(const float* __restrict__ dout, const long long* __restrict__ order,
                           const long long* __restrict__ offs, long long items, int D, float* __restrict__ dvars) {
  __shared__ float red[kWaves][kWave];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int code = blockIdx.x;
  long long beg = offs[code], end = offs[code + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > items ? items : end;
  const long long n = end > beg ? end - beg : 0;
  const long long q = (n + kWaves - 1) / kWaves;
  const long long b0 = beg + w * q, b1 = b0 + q < end ? b0 + q : end;
  for (int d0 = 0; d0 < D; d0 += kWave) {
    const int d = d0 + lane;
    float s = 0.f;
    if (d < D) {
      for (long long i = b0; i < b1; ++i) {
        const long long it = order[i];
        if (it >= 0 && it < items) s += dout[it * D + d];
      }
    }
    __syncthreads();
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && d < D) {
      float tsum = 0.f;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) tsum += red[k][lane];
      dvars[(long long)code * D + d] = tsum;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

#define W2V_DISPATCH(KERN, index, vec, ...)                                                        \
  do {                                                                                             \
    if (index) {                                                                                   \
      if (vec) hipLaunchKernelGGL((KERN<true, true>), __VA_ARGS__);                                \
      else hipLaunchKernelGGL((KERN<true, false>), __VA_ARGS__);                                   \
    } else {                                                                                       \
      if (vec) hipLaunchKernelGGL((KERN<false, true>), __VA_ARGS__);                               \
      else hipLaunchKernelGGL((KERN<false, false>), __VA_ARGS__);                                  \
    }                                                                                              \
  } while (0)

SBK_API int sbk_w2v_contrast_fwd(const float* x, const float* y, const float* negs, const int* idx, int R, int C, int N,
                                 long long s_row, long long s_neg, float temp, float* logits, float* rowloss,
                                 float* correct, float* aux, void* stream) {
  if (R <= 0 || C <= 0 || N <= 0) return SBK_ERR_ARG;
  if (!x || !y || !logits || !rowloss || !correct || !aux) return SBK_ERR_ARG;
  if ((negs != nullptr) == (idx != nullptr)) return SBK_ERR_ARG;  // exactly one candidate source
  if (!(temp > 0.f) || (long long)R * (N + 1) > 0x7fffffffLL) return SBK_ERR_ARG;
  if (negs && (s_row < 0 || s_neg < 0)) return SBK_ERR_ARG;
  const size_t lds = (size_t)(2 * ((C + 3) & ~3) + 16 + N + 1) * sizeof(float);
  if (lds > (size_t)kMaxLds) return SBK_ERR_ARG;
  const bool index = idx != nullptr;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(y) &&
                   (index || (aligned16(negs) && s_row % 4 == 0 && s_neg % 4 == 0));
  W2V_DISPATCH(contrast_fwd_kernel, index, vec, dim3(R), dim3(kThreads), lds, (hipStream_t)stream, x, y, negs, idx, R,
               C, N, s_row, s_neg, temp, logits, rowloss, correct, aux);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_w2v_contrast_bwd_x(const float* x, const float* y, const float* negs, const int* idx,
                                   const float* logits, const float* aux, const float* go,
                                   int R, int C, int N, long long s_row, long long s_neg, float temp, float* dx,
                                   float* dy, float* dnegs, float* ca, float* cb, void* stream) {
  if (R <= 0 || C <= 0 || N <= 0) return SBK_ERR_ARG;
  if (!x || !y || !logits || !aux || !go || !dx) return SBK_ERR_ARG;
  if ((negs != nullptr) == (idx != nullptr)) return SBK_ERR_ARG;
  if (idx && (!ca || !cb)) return SBK_ERR_ARG;
  if (!(temp > 0.f) || (long long)R * (N + 1) > 0x7fffffffLL) return SBK_ERR_ARG;
  if (negs && (s_row < 0 || s_neg < 0)) return SBK_ERR_ARG;
  const size_t lds = (size_t)((2 + kWaves) * ((C + 3) & ~3) + 16) * sizeof(float);
  if (lds > (size_t)kMaxLds) return SBK_ERR_ARG;
  const bool index = idx != nullptr;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(dx) &&
                   (index || (aligned16(negs) && s_row % 4 == 0 && s_neg % 4 == 0 && aligned16(dy) &&
                              aligned16(dnegs)));
  W2V_DISPATCH(contrast_bwd_x_kernel, index, vec, dim3(R), dim3(kThreads), lds, (hipStream_t)stream, x, y, negs, idx,
               logits, aux, go, R, C, N, s_row, s_neg, temp, dx, dy, dnegs, ca, cb);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_w2v_contrast_bwd_y(const float* x, const float* y, const long long* order, const long long* offs,
                                   const float* ca, const float* cb, int R, int C, int N, float* dy, void* stream) {
  if (R <= 0 || C <= 0 || N <= 0) return SBK_ERR_ARG;
  if (!x || !y || !order || !offs || !ca || !cb || !dy) return SBK_ERR_ARG;
  if ((long long)R * (N + 1) > 0x7fffffffLL) return SBK_ERR_ARG;
  const size_t lds = (size_t)(kWaves * ((C + 3) & ~3) + 16) * sizeof(float);
  if (lds > (size_t)kMaxLds) return SBK_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(x);
  if (vec)
    hipLaunchKernelGGL(contrast_bwd_y_kernel<true>, dim3(R), dim3(kThreads), lds, (hipStream_t)stream, x, y, order,
                       offs, ca, cb, R, C, N, dy);
  else
    hipLaunchKernelGGL(contrast_bwd_y_kernel<false>, dim3(R), dim3(kThreads), lds, (hipStream_t)stream, x, y, order,
                       offs, ca, cb, R, C, N, dy);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_gumbel_vq_parts(int Rq, int G) {
  if (Rq <= 0 || G <= 0) return 0;
  const long long items = (long long)Rq * G;
  const long long blocks = (items + kWaves - 1) / kWaves;
  return (int)(blocks < 256 ? blocks : 256) * kWaves;
}

SBK_API int sbk_gumbel_vq_fwd(const float* logits, const float* gumbels, float tau, int Rq, int G, int V,
                              const float* vars, int ncodes, int D, float* out, int* codes, int* counts, float* part,
                              float* ysoft, void* stream) {
  if (Rq <= 0 || G <= 0 || V <= 0 || D <= 0) return SBK_ERR_ARG;
  if ((long long)G * V != ncodes) return SBK_ERR_ARG;
  if (!logits || !vars || !out || !codes || !counts || !part) return SBK_ERR_ARG;
  if ((gumbels != nullptr) != (ysoft != nullptr) || !(tau > 0.f)) return SBK_ERR_ARG;
  const size_t lds = (size_t)kWaves * ncodes * sizeof(float);
  if (lds > (size_t)kMaxLds) return SBK_ERR_ARG;
  const int blocks = sbk_gumbel_vq_parts(Rq, G) / kWaves;
  hipLaunchKernelGGL(gumbel_vq_fwd_kernel, dim3(blocks), dim3(kThreads), lds, (hipStream_t)stream, logits, gumbels,
                     1.f / tau, Rq, G, V, vars, D, out, codes, counts, part, ysoft);
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_gumbel_vq_bwd(const float* dout, const float* vars, const float* logits, const float* ysoft,
                              const float* gpsum, float tau, const long long* order, const long long* offs, int Rq,
                              int G, int V, int ncodes, int D, float* dlogits, float* dvars, void* stream) {
  if (Rq <= 0 || G <= 0 || V <= 0 || D <= 0) return SBK_ERR_ARG;
  if ((long long)G * V != ncodes) return SBK_ERR_ARG;
  if (!dout || !vars || !logits || !gpsum || !order || !offs || !dlogits || !dvars || !(tau > 0.f)) return SBK_ERR_ARG;
  if (ysoft) {  // training: the straight-through term
    hipLaunchKernelGGL(gumbel_vq_dlogits_kernel, dim3((Rq + kQRows - 1) / kQRows, G), dim3(kThreads), 0,
                       (hipStream_t)stream, dout, vars, ysoft, 1.f / tau, Rq, G, V, D, dlogits);
    SBK_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(softmax_colsum_bwd_kernel, dim3(sbk_gumbel_vq_parts(Rq, G) / kWaves), dim3(kThreads), 0,
                     (hipStream_t)stream, logits, gpsum, Rq, G, V, ysoft ? 1 : 0, dlogits);
  SBK_CHECK_LAUNCH();
  hipLaunchKernelGGL(gumbel_vq_dvars_kernel, dim3(ncodes), dim3(kThreads), 0, (hipStream_t)stream, dout, order, offs,
                     (long long)Rq * G, D, dvars);
  SBK_CHECK_LAUNCH();
  return 0;
}
