// GRU recurrence of the transducer prediction network (nnet/RNN.py:280-388 of
// the reference, torch.nn.GRU semantics, gate order r, z, n).
//
//   r = sigmoid(gi_r + W_hr h + b_hr)        z = sigmoid(gi_z + W_hz h + b_hz)
//   q = W_hn h + b_hn                        n = tanh(gi_n + r * q)
//   h_t = (1 - z) * n + z * h_{t-1}
//
// One launch per time step on the skeleton of rnnstep.h: grid (ceil(H / 16),
// ceil(B / 32)), the recurrent product dealt to eight waves and summed in
// wave order.  sbk_gru_fwd / sbk_gru_bwd enqueue the launches of a sequence.
//
// Forward step t.  The product is h_{t-1} against the three 16-column tiles
// W_hh[g * H + j0 .. j0 + 16, :] (g = r, z, n).  The epilogue adds the input
// pre-activations — rows of the dense gi (B, T, 3H), or rows of the W_ih^T
// table gathered by token id (one-hot input; the blank adds b_ih only) —
// applies the gates and writes h_t.  Step t reads state[:, t-1, :] (hx at
// t = 0) and writes state[:, t, :]: nothing is updated in place.  With
// lengths, a row with t >= len_b keeps its state (state[b, t] =
// state[b, t-1]) and its output row y[b, t] is zero.  When training, r, z, n
// and q are kept in save (B, T, 4, H).
//
// Backward step t = T-1 .. 0, same grid.  The workgroup of units J forms
//   dh_t[:, J] = dy_t[:, J] + z_{t+1} * dh_{t+1}[:, J] + dgh_{t+1} . W_hh[:, J]
// (the product against W_hh^T (H, 3H), K = 3H; a row masked at t+1 passes
// dh_{t+1} through), then the gate gradients of its units from the saved
// activations, and writes dgi_t, dgh_t = (dr, dz, dn * r).  One more launch
// of the carry part alone gives dhx.  dh ping-pongs between the two halves of
// a (2, B, H) buffer.
#include "rnnstep.h"

using namespace sbk;
using namespace sbk::rnnstep;

namespace {

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

  f32x4 acc[kMT][3];
  product<T, 3>(acc, static_cast<const T*>(a.w_hh), H, H, hprev, ldh, j0, b0, B, H, mts, a.vec_w, a.vec_h, lane, w);
  meet<3>(red, acc, mts, lane, w);

  const long long H3 = 3LL * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const float s = total<3>(red, g, rr, jj);
      gh[g] = a.b_hh ? s + a.b_hh[g * H + j] : s;
    }
    const long long bt = (long long)b * Tn + t;
    float gi[3];
    if (a.tok) {
      const int idx = token_row(a.tok[bt], a.blank);
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
  __shared__ float red[kWaves][1][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, B = a.B, Tn = a.T;
  const int K = 3 * H;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const int s = t + 1;  // the step whose gradients arrive

  // the K loop of rnnstep.h's product for one tile, kept here as in lstm.hip:
  // the shared one compiles to a slower loop for a single tile
  f32x4 acc[kMT][1];
#pragma unroll
  for (int m = 0; m < kMT; ++m) acc[m][0] = f32x4{0.f, 0.f, 0.f, 0.f};
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
    const long long bj = (long long)b * H + j;
    float carry;
    if (s >= Tn) {
      carry = a.dhn ? a.dhn[bj] : 0.f;
    } else {
      const float dnext = a.dhw[(s & 1) * BH + bj];
      if (!a.lens || s < a.lens[b]) {
        const float mm = total<1>(red, 0, rr, jj);
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
      // n * n is rounded before the subtraction: left to the compiler, whether
      // 1 - n * n becomes one fma turned on how the code around it was written
      float nn;
      {
#pragma clang fp contract(off)
        nn = n * n;
      }
      dn = dh * (1.f - z) * (1.f - nn);
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
  return launch_steps(bf16 ? gru_fwd_step_kernel<bf16_t> : gru_fwd_step_kernel<float>, a, 1, 0, T, 1, stream);
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
  return launch_steps(bf16 ? gru_bwd_step_kernel<bf16_t> : gru_bwd_step_kernel<float>, a, 1, T - 1, T + 1, -1, stream);
}
