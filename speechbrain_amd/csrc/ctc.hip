// CTC loss (fused log-softmax gather, α/β lattice, dense one-pass gradient)
// and the row kernel of the sequence losses (nll_loss / kldiv_loss).
//
// Reference: speechbrain/nnet/losses.py
//   ctc_loss   :245-294  torch.nn.functional.ctc_loss(zero_infinity=True)
//   nll_loss   :405-452, kldiv_loss :525-594, compute_masked_loss :623-687
//
// Layouts: x (B, T, V) fp32 log-probs or logits (batch first, as the recipes
// hold them), targets (B, Lmax) int32 without blanks, in_len / tg_len (B,)
// int32 absolute lengths on the device.  The extended sequence of utterance b
// is l' = (∅, y1, ∅, ..., y_L, ∅), S = 2·L_b + 1 states, Smax = 2·Lmax + 1.
//
// Lattice arithmetic: α and β are kept in f64 (LDS rows and the workspace):
// they are running sums of ~T log-probs, thousands in magnitude at the recipe
// shape, and the gradient takes exp(α + β + nll − lp), a difference of such
// sums — in f32 one ulp of α is 2.4e-4 there and that is the gradient's
// relative error.  The exp / log of each step act on differences of O(1) and
// stay f32 (their error does not scale with |α|); f64 add / max are full rate.
//
// Gradient convention (torch.nn.functional.ctc_loss): wrt log-probs
//   g[t,v] = (exp(lp[t,v]) − Σ_{s: l'_s = v} exp(α[t,s] + β[t,s] + nll − lp[t,v])) · grad_out[b]
// (β includes lp[t,s]); wrt logits the same with softmax(logits) for exp(lp).
// Rows t >= in_len[b] and infeasible utterances (nll = +inf) get 0.
#include "sbk_common.h"

#include <type_traits>

using namespace sbk;

#define SBK_ERR_CTC_STATES 1002  // 2*Lmax + 1 exceeds the lattice's LDS rows

namespace {

constexpr int kCtcMaxStates = 3073;  // 20 bytes of LDS per state, < 64 KiB

__device__ __forceinline__ bool lens_ok(int Tb, int Lb, int T, int Lmax) {
  return Tb >= 0 && Tb <= T && Lb >= 0 && Lb <= Lmax;
}

// log-sum-exp of one row, one wave.  VEC = 4 needs V % 4 == 0 and a
// 16-byte-aligned row.
// One sweep: each lane keeps a running maximum and the sum rescaled to it.
template <int VEC>
__device__ __forceinline__ float row_lse(const float* __restrict__ xr, int V, int lane) {
  float m = -INFINITY, s = 0.f;
  if (VEC == 4) {
    const float4* x4 = reinterpret_cast<const float4*>(xr);
    for (int i = lane; i < V / 4; i += 64) {
      const float4 v = x4[i];
      const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
      if (mx > m) {
        s *= expf(m - mx);  // m = -inf: s is 0 and stays 0
        m = mx;
      }
      if (m > -INFINITY) s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
    }
  } else {
    for (int v = lane; v < V; v += 64) {
      const float xv = xr[v];
      if (xv > m) {
        s *= expf(m - xv);
        m = xv;
      }
      if (m > -INFINITY) s += expf(xv - m);
    }
  }
  const float M = wave_max(m);
  if (m > -INFINITY) s *= expf(m - M);
  return M + logf(wave_sum(s));
}

// One wave per (b, t < in_len[b]) row: lse (logits input) and the compact
// lp[b, t, s] of the S extended states.
template <int VEC>
__global__ void __launch_bounds__(256) ctc_gather_kernel(const float* __restrict__ x, const int* __restrict__ tgt,
                                                         const int* __restrict__ in_len,
                                                         const int* __restrict__ tg_len, int B, int T, int V,
                                                         int Lmax, int blank, int is_logits, float* __restrict__ lp,
                                                         float* __restrict__ lse_out) {
  const long long rows = (long long)B * T;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / T), t = (int)(row % T);
  const int Tb = in_len[b], Lb = tg_len[b];
  if (!lens_ok(Tb, Lb, T, Lmax) || t >= Tb) return;
  const float* xr = x + row * V;
  const float lse = is_logits ? row_lse<VEC>(xr, V, lane) : 0.f;
  if (is_logits && lane == 0) lse_out[row] = lse;
  const int S = 2 * Lb + 1, Smax = 2 * Lmax + 1;
  const int* y = tgt + (long long)b * Lmax;
  float* o = lp + row * Smax;
  for (int s = lane; s < S; s += 64) {
    // a label outside [0, V) poisons its state (NaN loss), never indexes the row
    const int v = (s & 1) ? y[s >> 1] : blank;
    o[s] = (unsigned)v < (unsigned)V ? xr[v] - lse : __builtin_nanf("");
  }
}

// grid (B, 2): y = 0 -> α (t ascending), y = 1 -> β (t descending).  Threads
// over states (loop if S > blockDim); the previous row sits in an LDS double
// buffer, one barrier per time step.  The β block also links the repeated
// symbols of the target (chain), for the gradient's fixed summation order.
__global__ void __launch_bounds__(256) ctc_lattice_kernel(const float* __restrict__ lp, const int* __restrict__ tgt,
                                                          const int* __restrict__ in_len,
                                                          const int* __restrict__ tg_len, int T, int Lmax,
                                                          double* __restrict__ alpha, double* __restrict__ beta,
                                                          double* __restrict__ nll, int* __restrict__ chain,
                                                          float* __restrict__ loss) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Smax = 2 * Lmax + 1;
  double* rowbuf = reinterpret_cast<double*>(smem);         // 2 x Smax
  int* skip = reinterpret_cast<int*>(rowbuf + 2 * Smax);    // Smax
  const int b = blockIdx.x, tid = threadIdx.x, bd = blockDim.x;
  const bool fwd = blockIdx.y == 0;
  const int Tb = in_len[b], Lb = tg_len[b];
  if (!lens_ok(Tb, Lb, T, Lmax)) {
    // lengths outside the (T, Lmax) lattice: NaN loss for this utterance
    if (fwd && tid == 0) {
      nll[b] = __builtin_nan("");
      loss[b] = __builtin_nanf("");
    }
    return;
  }
  const int S = 2 * Lb + 1;
  const int* y = tgt + (long long)b * Lmax;
  // skip transition s-2 -> s only where l'_s is a label differing from l'_{s-2}
  for (int s = tid; s < S; s += bd) skip[s] = (s & 1) && s >= 3 && y[s >> 1] != y[(s >> 1) - 1];
  if (!fwd) {
    // chain[j] = 2 * (next j' > j with y[j'] == y[j], or -1) + 2 + [j is the first occurrence]
    for (int j = tid; j < Lb; j += bd) {
      const int v = y[j];
      int first = 1, nx = -1;
      for (int i = 0; i < j; ++i)
        if (y[i] == v) {
          first = 0;
          break;
        }
      for (int i = j + 1; i < Lb; ++i)
        if (y[i] == v) {
          nx = i;
          break;
        }
      chain[(long long)b * Lmax + j] = (nx + 1) * 2 + first;
    }
  }
  __syncthreads();
  const long long base = (long long)b * T * Smax;
  const float* lpb = lp + base;
  double* out = (fwd ? alpha : beta) + base;
  const double NEG = -(double)INFINITY;
  // The log-prob of this thread's first state is loaded kPf steps ahead into
  // a register ring (statically indexed: the step loop is unrolled by kPf), so
  // no step waits for global memory.  Step and state are clamped into the
  // utterance's lattice: the load is unconditional and the compiler does not
  // wait for it where it is issued.  S <= blockDim (one state per thread) runs
  // without the state loop, whose in-place loads of the further states would
  // make every wait a full one.
  constexpr int kPf = 4;
  const int s0 = tid < S ? tid : S - 1;
  auto lp0 = [&](int n) {
    n = n < Tb ? n : Tb - 1;
    return lpb[(long long)(fwd ? n : Tb - 1 - n) * Smax + s0];
  };
  auto state = [&](int n, int t, int s, float l) {
    double* cur = rowbuf + (n & 1) * Smax;
    const double* prv = rowbuf + ((n & 1) ^ 1) * Smax;
    double v;
    if (n == 0) {
      v = (fwd ? s <= 1 : s >= S - 2) ? (double)l : NEG;
    } else {
      const double a0 = prv[s];
      double a1 = NEG, a2 = NEG;
      if (fwd) {
        if (s >= 1) a1 = prv[s - 1];
        if (skip[s]) a2 = prv[s - 2];
      } else {
        if (s + 1 < S) a1 = prv[s + 1];
        if (s + 2 < S && skip[s + 2]) a2 = prv[s + 2];
      }
      const double m = fmax(a0, fmax(a1, a2));
      if (m == NEG)
        v = NEG;
      else
        v = m + (double)logf(expf((float)(a0 - m)) + expf((float)(a1 - m)) + expf((float)(a2 - m))) + (double)l;
    }
    cur[s] = v;
    out[(long long)t * Smax + s] = v;
  };
  auto run = [&](auto one_state) {
    constexpr bool kOne = decltype(one_state)::value;
    auto step = [&](int n, float l0) {
      const int t = fwd ? n : Tb - 1 - n;
      if (kOne) {
        if (tid < S) state(n, t, tid, l0);
      } else {
        for (int s = tid; s < S; s += bd) state(n, t, s, s == tid ? l0 : lpb[(long long)t * Smax + s]);
      }
      __syncthreads();
    };
    float ring[kPf];
#pragma unroll
    for (int k = 0; k < kPf; ++k) ring[k] = lp0(k);
    int n = 0;
    for (; n + kPf <= Tb; n += kPf) {
#pragma unroll
      for (int k = 0; k < kPf; ++k) {
        const float l0 = ring[k];
        ring[k] = lp0(n + k + kPf);
        step(n + k, l0);
      }
    }
#pragma unroll
    for (int k = 0; k < kPf - 1; ++k)
      if (n + k < Tb) step(n + k, ring[k]);
  };
  if (Tb > 0) {
    if (S <= bd)
      run(std::true_type{});
    else
      run(std::false_type{});
  }
  if (fwd && tid == 0) {
    double ll;
    if (Tb == 0) {
      ll = S == 1 ? 0.0 : NEG;  // no frames: only the empty target has a path
    } else {
      const double* last = rowbuf + ((Tb - 1) & 1) * Smax;
      const double a = last[S - 1], c = S > 1 ? last[S - 2] : NEG;
      const double m = fmax(a, c);
      ll = m == NEG ? NEG : m + log(exp(a - m) + exp(c - m));
    }
    nll[b] = -ll;
    // zero_infinity=True: an infeasible utterance contributes loss 0 (and gradient 0)
    loss[b] = ll == NEG ? 0.f : (float)(-ll);
  }
}

template <int VEC>
__device__ __forceinline__ void fill_row(float* __restrict__ o, int V, int lane, float val) {
  if (VEC == 4) {
    float4* o4 = reinterpret_cast<float4*>(o);
    for (int i = lane; i < V / 4; i += 64) o4[i] = make_float4(val, val, val, val);
  } else {
    for (int v = lane; v < V; v += 64) o[v] = val;
  }
}

// Dense gradient, one wave per (b, t) row, one pass over (B, T, V): the row
// is written as p·g (p = exp(lp) or softmax), then the wave rewrites the
// <= L_b + 1 entries that carry occupancy.  The occupancy of a repeated symbol
// is summed by the lane of its first occurrence along the chain, the blank's
// by a strided loop and the fixed shuffle tree: bit-identical run to run.
template <int VEC>
__global__ void __launch_bounds__(256) ctc_grad_kernel(const float* __restrict__ x, const int* __restrict__ tgt,
                                                       const int* __restrict__ in_len,
                                                       const int* __restrict__ tg_len,
                                                       const double* __restrict__ alpha,
                                                       const double* __restrict__ beta,
                                                       const double* __restrict__ nll, const float* __restrict__ lp,
                                                       const float* __restrict__ lse, const int* __restrict__ chain,
                                                       const float* __restrict__ go, int B, int T, int V, int Lmax,
                                                       int blank, int is_logits, float* __restrict__ out) {
  const long long rows = (long long)B * T;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / T), t = (int)(row % T);
  const int Tb = in_len[b], Lb = tg_len[b];
  float* orow = out + row * V;
  if (!lens_ok(Tb, Lb, T, Lmax)) {
    fill_row<VEC>(orow, V, lane, __builtin_nanf(""));  // invalid lengths: NaN gradient, as the loss
    return;
  }
  const double nl = nll[b];
  if (t >= Tb || nl == (double)INFINITY) {
    fill_row<VEC>(orow, V, lane, 0.f);
    return;
  }
  const float g = go[b];
  const float* xr = x + row * V;
  const float l = is_logits ? lse[row] : 0.f;
  if (VEC == 4) {
    const float4* x4 = reinterpret_cast<const float4*>(xr);
    float4* o4 = reinterpret_cast<float4*>(orow);
    for (int i = lane; i < V / 4; i += 64) {
      const float4 v = x4[i];
      o4[i] = make_float4(expf(v.x - l) * g, expf(v.y - l) * g, expf(v.z - l) * g, expf(v.w - l) * g);
    }
  } else {
    for (int v = lane; v < V; v += 64) orow[v] = expf(xr[v] - l) * g;
  }
  const int S = 2 * Lb + 1, Smax = 2 * Lmax + 1;
  const long long base = row * Smax;
  const int* y = tgt + (long long)b * Lmax;
  const int* ch = chain + (long long)b * Lmax;
  auto occ = [&](int s) { return expf((float)(alpha[base + s] + beta[base + s] + nl - (double)lp[base + s])); };
  // the stores below follow the row's stores above in this wave's program order
  float acc = 0.f;
  for (int s = lane; s < S; s += 64)
    if (!(s & 1) || y[s >> 1] == blank) acc += occ(s);
  acc = wave_sum(acc);
  if (lane == 0) orow[blank] = (expf(xr[blank] - l) - acc) * g;
  for (int j = lane; j < Lb; j += 64) {
    if (!(ch[j] & 1)) continue;
    const int v = y[j];
    if (v == blank || (unsigned)v >= (unsigned)V) continue;
    float a = 0.f;
    for (int i = j; i >= 0; i = (ch[i] >> 1) - 1) a += occ(2 * i + 1);
    orow[v] = (expf(xr[v] - l) - a) * g;
  }
}

// Sequence-loss row kernel: x viewed as (B, U, V) with batch stride sb (rows
// of a truncated (B, U', V) tensor are not contiguous across b).
template <int VEC>
__global__ void __launch_bounds__(256) nll_rows_fwd_kernel(const float* __restrict__ x,
                                                           const int* __restrict__ tgt, int B, int U, long long sb,
                                                           int V, float* __restrict__ sel,
                                                           float* __restrict__ rsum) {
  const long long rows = (long long)B * U;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + (row / U) * sb + (row % U) * V;
  float s = 0.f;
  if (VEC == 4) {
    const float4* x4 = reinterpret_cast<const float4*>(xr);
    for (int i = lane; i < V / 4; i += 64) {
      const float4 v = x4[i];
      s += (v.x + v.y) + (v.z + v.w);
    }
  } else {
    for (int v = lane; v < V; v += 64) s += xr[v];
  }
  s = wave_sum(s);
  if (lane == 0) {
    const int y = tgt[row];
    rsum[row] = s;
    sel[row] = (unsigned)y < (unsigned)V ? xr[y] : __builtin_nanf("");
  }
}

template <int VEC>
__global__ void __launch_bounds__(256) nll_rows_bwd_kernel(const int* __restrict__ tgt, const float* __restrict__ a,
                                                           const float* __restrict__ c, int B, int U, long long sb,
                                                           int V, float* __restrict__ grad) {
  const long long rows = (long long)B * U;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  float* gr = grad + (row / U) * sb + (row % U) * V;
  const int y = tgt[row];
  const float av = a[row], cv = c[row];
  if (VEC == 4) {
    float4* g4 = reinterpret_cast<float4*>(gr);
    for (int i = lane; i < V / 4; i += 64) {
      const int v = 4 * i;
      g4[i] = make_float4(cv + (v == y ? av : 0.f), cv + (v + 1 == y ? av : 0.f), cv + (v + 2 == y ? av : 0.f),
                          cv + (v + 3 == y ? av : 0.f));
    }
  } else {
    for (int v = lane; v < V; v += 64) gr[v] = cv + (v == y ? av : 0.f);
  }
}

inline bool vec4_ok(const void* p, int V) { return V % 4 == 0 && ((uintptr_t)p & 15) == 0; }

// ws: [α f64 (n) | β f64 (n) | nll f64 (B) | lp (n) | lse (B*T) | chain int (B*Lmax)], n = B*T*Smax
struct CtcWs {
  double *alpha, *beta, *nll;
  float *lp, *lse;
  int* chain;
};
inline CtcWs ctc_ws(float* ws, int B, int T, int Lmax) {
  const long long n = (long long)B * T * (2 * Lmax + 1);
  CtcWs w;
  w.alpha = reinterpret_cast<double*>(ws);
  w.beta = w.alpha + n;
  w.nll = w.beta + n;
  w.lp = reinterpret_cast<float*>(w.nll + B);
  w.lse = w.lp + n;
  w.chain = reinterpret_cast<int*>(w.lse + (long long)B * T);
  return w;
}

}  // namespace

SBK_API long long sbk_ctc_workspace_floats(int B, int T, int Lmax) {
  return 5LL * B * T * (2 * Lmax + 1) + (long long)B * T + 2LL * B + (long long)B * Lmax;
}

// Forward: compact log-probs (log-softmax fused when is_logits), α, β, the
// repeat chain and the per-utterance loss (B floats; 0 where infeasible, NaN
// for lengths outside the lattice).  ws: sbk_ctc_workspace_floats(B, T, Lmax)
// floats, 8-byte aligned, kept for the backward.
SBK_API int sbk_ctc_forward(const float* x, const int* targets, const int* in_len, const int* tg_len, int B, int T,
                            int V, int Lmax, int blank, int is_logits, float* ws, float* loss, void* stream) {
  if (B <= 0 || T <= 0 || V <= 0 || Lmax < 0 || blank < 0 || blank >= V || !x || !in_len || !tg_len || !ws || !loss ||
      (Lmax > 0 && !targets) || ((uintptr_t)ws & 7))
    return SBK_ERR_ARG;
  const int Smax = 2 * Lmax + 1;
  if (Smax > kCtcMaxStates) return SBK_ERR_CTC_STATES;
  hipStream_t s = (hipStream_t)stream;
  const CtcWs w = ctc_ws(ws, B, T, Lmax);
  const long long rows = (long long)B * T;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (vec4_ok(x, V))
    hipLaunchKernelGGL(ctc_gather_kernel<4>, grid, dim3(256), 0, s, x, targets, in_len, tg_len, B, T, V, Lmax, blank,
                       is_logits, w.lp, w.lse);
  else
    hipLaunchKernelGGL(ctc_gather_kernel<1>, grid, dim3(256), 0, s, x, targets, in_len, tg_len, B, T, V, Lmax, blank,
                       is_logits, w.lp, w.lse);
  SBK_CHECK_LAUNCH();
  const int bd = Smax >= 256 ? 256 : ((Smax + 63) / 64) * 64;
  hipLaunchKernelGGL(ctc_lattice_kernel, dim3(B, 2), dim3(bd), (size_t)Smax * 20, s, w.lp, targets, in_len, tg_len, T,
                     Lmax, w.alpha, w.beta, w.nll, w.chain, loss);
  SBK_CHECK_LAUNCH();
  return 0;
}

// Dense gradient (B, T, V) from the forward's workspace, rows scaled by
// grad_out[b]: wrt the log-probs (is_logits = 0, torch's ctc_loss convention)
// or wrt the logits (is_logits = 1).
SBK_API int sbk_ctc_backward(const float* x, const int* targets, const int* in_len, const int* tg_len, int B, int T,
                             int V, int Lmax, int blank, int is_logits, const float* ws, const float* grad_out,
                             float* grad, void* stream) {
  if (B <= 0 || T <= 0 || V <= 0 || Lmax < 0 || blank < 0 || blank >= V || !x || !in_len || !tg_len || !ws ||
      !grad_out || !grad || (Lmax > 0 && !targets))
    return SBK_ERR_ARG;
  if (2 * Lmax + 1 > kCtcMaxStates) return SBK_ERR_CTC_STATES;
  const CtcWs w = ctc_ws(const_cast<float*>(ws), B, T, Lmax);
  const long long rows = (long long)B * T;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (vec4_ok(x, V) && vec4_ok(grad, V))
    hipLaunchKernelGGL(ctc_grad_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, targets, in_len, tg_len,
                       w.alpha, w.beta, w.nll, w.lp, w.lse, w.chain, grad_out, B, T, V, Lmax, blank, is_logits, grad);
  else
    hipLaunchKernelGGL(ctc_grad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, targets, in_len, tg_len,
                       w.alpha, w.beta, w.nll, w.lp, w.lse, w.chain, grad_out, B, T, V, Lmax, blank, is_logits, grad);
  SBK_CHECK_LAUNCH();
  return 0;
}

// sel[r] = x[r, targets[r]] (NaN for a target outside [0, V)), rsum[r] = Σ_v x[r, v]
// over the rows r = b*U + u of x (B, U, V) with batch stride sb floats.
SBK_API int sbk_nll_rows_forward(const float* x, const int* targets, int B, int U, long long sb, int V, float* sel,
                                 float* rsum, void* stream) {
  if (B <= 0 || U <= 0 || V <= 0 || sb < (long long)U * V || !x || !targets || !sel || !rsum) return SBK_ERR_ARG;
  const long long rows = (long long)B * U;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (vec4_ok(x, V) && sb % 4 == 0)
    hipLaunchKernelGGL(nll_rows_fwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, targets, B, U, sb, V, sel,
                       rsum);
  else
    hipLaunchKernelGGL(nll_rows_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, targets, B, U, sb, V, sel,
                       rsum);
  SBK_CHECK_LAUNCH();
  return 0;
}

// grad[r, v] = a[r]·[v == targets[r]] + c[r] over the same rows.
SBK_API int sbk_nll_rows_backward(const int* targets, const float* a, const float* c, int B, int U, long long sb, int V,
                                  float* grad, void* stream) {
  if (B <= 0 || U <= 0 || V <= 0 || sb < (long long)U * V || !targets || !a || !c || !grad) return SBK_ERR_ARG;
  const long long rows = (long long)B * U;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (vec4_ok(grad, V) && sb % 4 == 0)
    hipLaunchKernelGGL(nll_rows_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, targets, a, c, B, U, sb, V,
                       grad);
  else
    hipLaunchKernelGGL(nll_rows_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, targets, a, c, B, U, sb, V,
                       grad);
  SBK_CHECK_LAUNCH();
  return 0;
}
