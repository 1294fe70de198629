// LiGRU recurrence (nnet/RNN.py:961-1325 of the reference), one or two
// directions: a two-gate cell with no recurrent bias and no cell state.
//
//   gates = wn[:, t] + h_{t-1} U^T          U (2H, H), shared by both directions
//   a, zpre = gates[:H], gates[H:]          z = sigmoid(zpre)
//   hc = act(a) * mask[row]                 mask (rows, H), constant over time
//   h_t = z * h_{t-1} + (1 - z) * hc
//
// act is ReLU, LeakyReLU(0.01), tanh or sin.  wn is the normalised input
// projection; the kernels read the raw GEMM output and normalise in the
// epilogue,
//   wn = (raw - mu[row]) * rs[row] * cscale[col] + cshift[col],
// the row terms being optional: LayerNorm passes the row mean and reciprocal
// standard deviation with gamma, beta as the column terms, BatchNorm folds its
// statistics into the column terms alone.
//
// One launch per time step on the skeleton of rnnstep.h.  Both directions of
// a bidirectional layer share a launch and the weights: grid (ceil(H / 16),
// ceil(B / 32), D), launch s working on frame s in direction 0 and T-1-s in
// direction 1.  Both read the same raw[b, t]: the reference's
// cat([x, x.flip(1)]) makes the second half's pre-activations the flip of the
// first, so a layer has one input GEMM and one normalisation.  The batch rows
// of direction d are rows d * B .. d * B + B of hx and mask.
//
// Forward step.  The product is the previous h of direction d against the two
// 16-row tiles U[g * H + j0 .. j0 + 16, :].  The epilogue normalises the two
// pre-activations, applies the gates and writes h_t into out (B, T, D * H) at
// frame t: step s reads out at the frame before it (hx at s = 0), nothing is
// updated in place.  When training, a and z are kept in save (B, T, D, 2H).
//
// Backward step, same grid, order mirrored per direction; one more launch
// gives the carry into dhx.  With ts the frame whose gradients arrive (t + 1
// forward, t - 1 reverse):
//   dh_t = dy_t + z_ts * dh_ts + dG_ts . U[:, J]    (the product against U^T, K = 2H)
//   da = dh (1 - z) mask act'(a)          dz = dh (h_{t-1} - hc) z (1 - z)
// dG (B, T, D, 2H) at true frame positions is both the gradient of wn (the two
// directions add) and the operand of the next step's product.  dh ping-pongs
// between the two halves of a (2, D, B, H) buffer.
#include "rnnstep.h"

using namespace sbk;
using namespace sbk::rnnstep;

namespace {

enum { kRelu = 0, kLeaky = 1, kTanh = 2, kSin = 3 };

__device__ __forceinline__ float act_of(int code, float a) {
  switch (code) {
    case kLeaky: return a > 0.f ? a : 0.01f * a;
    case kTanh: return tanhf(a);
    case kSin: return sinf(a);
    default: return a > 0.f ? a : 0.f;
  }
}

// act'(a); v = act(a)
__device__ __forceinline__ float dact_of(int code, float a, float v) {
  switch (code) {
    case kLeaky: return a > 0.f ? 1.f : 0.01f;
    case kTanh: return 1.f - v * v;
    case kSin: return cosf(a);
    default: return a > 0.f ? 1.f : 0.f;
  }
}

struct FwdArgs {
  const void* u;         // (2H, H) in the compute dtype
  const float* hx;       // (D, B, H) or null
  const float* raw;      // (B, T, 2H): the input projection before normalisation
  const float* mu;       // (B * T) or null
  const float* rs;       // (B * T) or null
  const float* cscale;   // (2H) or null
  const float* cshift;   // (2H) or null
  const float* mask;     // (D, B, H) or null
  float* out;            // (B, T, D * H)
  float* save;           // (B, T, D, 2H) or null: a, z
  int act, B, T, H, D;
  int vec_w, vec_h;
};

// launch s in [0, T): frame s in direction 0, T-1-s in direction 1
template <typename T>
__global__ void __launch_bounds__(kThreads) ligru_fwd_step_kernel(FwdArgs a, int s) {
  __shared__ float red[kWaves][2][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, B = a.B, Tn = a.T, D = a.D;
  const int d = blockIdx.z;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const int t = d ? Tn - 1 - s : s;
  const int tp = d ? t + 1 : t - 1;      // the frame this one continues
  const long long DH = (long long)D * H;
  const long long ldp = s == 0 ? H : Tn * DH;
  const long long offp = s == 0 ? (long long)d * B * H : tp * DH + (long long)d * H;
  const float* hprev = s == 0 ? (a.hx ? a.hx + offp : nullptr) : a.out + offp;

  f32x4 acc[kMT][2];
  product<T, 2>(acc, static_cast<const T*>(a.u), H, H, hprev, ldp, j0, b0, B, H, mts, a.vec_w, a.vec_h, lane, w);
  meet<2>(red, acc, mts, lane, w);

  const long long H2 = 2LL * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    const long long bt = (long long)b * Tn + t;
    const float mu = a.mu ? a.mu[bt] : 0.f;
    const float rs = a.rs ? a.rs[bt] : 1.f;
    float pre[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int col = g * H + j;
      float x = (a.raw[bt * H2 + col] - mu) * rs;
      if (a.cscale) x *= a.cscale[col];
      if (a.cshift) x += a.cshift[col];
      pre[g] = x + total<2>(red, g, rr, jj);
    }
    const float hp = hprev ? hprev[b * ldp + j] : 0.f;
    const float z = sigmoid_exact(pre[1]);
    float hc = act_of(a.act, pre[0]);
    if (a.mask) hc *= a.mask[((long long)d * B + b) * H + j];
    a.out[bt * DH + (long long)d * H + j] = z * hp + (1.f - z) * hc;
    if (a.save) {
      float* sv = a.save + (bt * D + d) * H2 + j;
      sv[0] = pre[0];
      sv[H] = z;
    }
  }
}

struct BwdArgs {
  const void* uT;        // (H, 2H) in the compute dtype
  const float* hx;       // (D, B, H) or null
  const float* out;      // (B, T, D * H)
  const float* save;     // (B, T, D, 2H)
  const float* mask;     // (D, B, H) or null
  const float* dy;       // (B, T, D * H) or null
  float* dG;             // (B, T, D, 2H)
  float* dhw;            // (2, D, B, H)
  float* dhx;            // (D, B, H)
  int act, B, T, H, D;
  int vec_w, vec_g;
};

// launch s in [0, T]: frame T-1-s in direction 0, s in direction 1; the last
// launch (frame -1 / T) computes the carry into dhx only
template <typename T>
__global__ void __launch_bounds__(kThreads) ligru_bwd_step_kernel(BwdArgs a, int s) {
  __shared__ float red[kWaves][1][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, B = a.B, Tn = a.T, D = a.D;
  const int K = 2 * H;
  const int d = blockIdx.z;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const int t = d ? s : Tn - 1 - s;
  const int ts = d ? t - 1 : t + 1;      // the frame whose gradients arrive
  const int tp = d ? t + 1 : t - 1;      // the frame this one continued
  const bool arrives = s > 0;
  const bool last = s == Tn;
  const long long DH = (long long)D * H;

  // the K loop of rnnstep.h's product for one tile, kept here as in gru.hip
  // and lstm.hip: the shared one compiles to a slower loop for a single tile
  // 
  f32x4 acc[kMT][1];
#pragma unroll
  for (int m = 0; m < kMT; ++m) acc[m][0] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (arrives) {
    const T* W = static_cast<const T*>(a.uT);
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
              row < B ? load_f8<T>(a.dG + (((long long)row * Tn + ts) * D + d) * K, kk, K, a.vec_g)
                      : MT<T>::zero();
          MT<T>::mma(acc[m][0], af, bw);
        }
      }
    }
  }
  meet<1>(red, acc, mts, lane, w);

  const long long BH = (long long)B * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    const long long bj = d * BH + (long long)b * H + j;
    float carry = 0.f;   // what frame ts hands to the h it started from
    if (arrives) {
      const float zs = a.save[(((long long)b * Tn + ts) * D + d) * K + H + j];
      carry = zs * a.dhw[(ts & 1) * D * BH + bj] + total<1>(red, 0, rr, jj);
    }
    if (last) {
      a.dhx[bj] = carry;
      continue;
    }
    const long long bt = (long long)b * Tn + t;
    const float dh = carry + (a.dy ? a.dy[bt * DH + (long long)d * H + j] : 0.f);
    a.dhw[(t & 1) * D * BH + bj] = dh;
    const float* sv = a.save + (bt * D + d) * K + j;
    const float av = sv[0], z = sv[H];
    const float m = a.mask ? a.mask[bj] : 1.f;
    const float v = act_of(a.act, av);
    const float hp = s == Tn - 1 ? (a.hx ? a.hx[bj] : 0.f) : a.out[((long long)b * Tn + tp) * DH + (long long)d * H + j];
    float* g = a.dG + (bt * D + d) * K + j;
    g[0] = dh * (1.f - z) * m * dact_of(a.act, av, v);
    g[H] = dh * (hp - v * m) * z * (1.f - z);
  }
}

}  // namespace

// The T forward launches of one LiGRU layer, D = 1 or 2 directions sharing u.
// bf16: u is bf16 (else fp32), (2H, H) row-major.  raw (B, T, 2H) fp32 is the
// input projection; mu, rs (B * T) or null and cscale, cshift (2H) or null
// normalise it in the epilogue.  hx (D, B, H) or null (zeros); mask (D, B, H)
// or null (ones).  act: 0 ReLU, 1 LeakyReLU(0.01), 2 tanh, 3 sin.  out
// (B, T, D * H): h after every step; save (B, T, D, 2H) or null: a, z.
SBK_API int sbk_ligru_fwd(int bf16, int D, int act, const void* u, const float* hx, const float* raw, const float* mu,
                          const float* rs, const float* cscale, const float* cshift, const float* mask, int B, int T,
                          int H, float* out, float* save, void* stream) {
  if (!u || !raw || !out || (!mu) != (!rs)) return SBK_ERR_ARG;
  if (B <= 0 || T <= 0 || H <= 0 || (D != 1 && D != 2) || act < 0 || act > 3) return SBK_ERR_ARG;
  if ((long long)2 * H * H > 0x7fffffffLL || (long long)B * T * D > 0x7fffffffLL / 4) return SBK_ERR_ARG;
  FwdArgs a;
  a.u = u; a.hx = hx; a.raw = raw; a.mu = mu; a.rs = rs; a.cscale = cscale; a.cshift = cshift; a.mask = mask;
  a.out = out; a.save = save;
  a.act = act; a.B = B; a.T = T; a.H = H; a.D = D;
  a.vec_w = aligned16(u) && H % (bf16 ? 8 : 4) == 0;
  a.vec_h = aligned16(out) && H % 4 == 0 && (!hx || aligned16(hx));
  return launch_steps(bf16 ? ligru_fwd_step_kernel<bf16_t> : ligru_fwd_step_kernel<float>, a, D, 0, T, 1, stream);
}

// The T backward launches (order mirrored per direction) and one more for the
// carry into dhx.  uT = U^T (H, 2H) in the compute dtype; hx, mask, out, save
// as given to / written by sbk_ligru_fwd; dy (B, T, D * H) or null.  Writes dG
// (B, T, D, 2H) fp32 and dhx (D, B, H); dhw (2, D, B, H) is scratch.
SBK_API int sbk_ligru_bwd(int bf16, int D, int act, const void* uT, const float* hx, const float* out,
                          const float* save, const float* mask, const float* dy, int B, int T, int H, float* dG,
                          float* dhw, float* dhx, void* stream) {
  if (!uT || !out || !save || !dG || !dhw || !dhx) return SBK_ERR_ARG;
  if (B <= 0 || T <= 0 || H <= 0 || (D != 1 && D != 2) || act < 0 || act > 3) return SBK_ERR_ARG;
  if ((long long)2 * H * H > 0x7fffffffLL || (long long)B * T * D > 0x7fffffffLL / 4) return SBK_ERR_ARG;
  BwdArgs a;
  a.uT = uT; a.hx = hx; a.out = out; a.save = save; a.mask = mask; a.dy = dy;
  a.dG = dG; a.dhw = dhw; a.dhx = dhx;
  a.act = act; a.B = B; a.T = T; a.H = H; a.D = D;
  // rows of 2H elements: 16-byte aligned in fp32 for even H, in bf16 for H % 4 == 0
  a.vec_w = aligned16(uT) && H % (bf16 ? 4 : 2) == 0;
  a.vec_g = aligned16(dG) && H % 2 == 0;
  return launch_steps(bf16 ? ligru_bwd_step_kernel<bf16_t> : ligru_bwd_step_kernel<float>, a, D, 0, T + 1, 1, stream);
}
