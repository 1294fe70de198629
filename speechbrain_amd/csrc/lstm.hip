// LSTM recurrence (nnet/RNN.py:169-277 of the reference, torch.nn.LSTM
// semantics, gate order i, f, g, o), one or two directions.
//
//   i = sigmoid(gi_i + W_hi h + b_hi)        f = sigmoid(gi_f + W_hf h + b_hf)
//   g = tanh(gi_g + W_hg h + b_hg)           o = sigmoid(gi_o + W_ho h + b_ho)
//   c_t = f * c_{t-1} + i * g                h_t = o * tanh(c_t)
//
// One launch per time step on the skeleton of rnnstep.h.  Both directions of
// a bidirectional layer share a launch: grid (ceil(H / 16), ceil(B / 32), D),
// launch s working on time s in direction 0 and T-1-s in direction 1, so a
// bidirectional layer costs T launches forward and T+1 backward like a
// unidirectional one.  sbk_lstm_fwd / sbk_lstm_bwd enqueue all launches of a
// layer.
//
// Forward step.  A workgroup owns 16 hidden units of one direction for all
// four gates: the product is the previous h of that direction against the
// four 16-column tiles W_hh[d][g * H + j0 .. j0 + 16, :].  The partial tiles
// take 4 gates x 8 waves x 32 rows x 16 units of fp32 in LDS, the 64 KiB of a
// static allocation, two workgroups per CU.  The epilogue adds the input
// pre-activations (rows of the dense gi (B, T, D, 4H), or rows of the W_ih^T
// table gathered by token id, the blank adding b_ih only), applies the gates
// and writes h_t and c_t into hstate / cstate (B, T, D * H) at time t:
// nothing is updated in place.  With lengths, a row with t >= len_b keeps
// (h, c) and its output row is zero; in the reverse scan the row so carries
// (h0, c0) through its padding and starts at t = len_b - 1.  When training,
// i, f, g, o are kept in save (B, T, D, 4H); tanh(c_t) is recomputed in the
// backward from cstate.
//
// Backward step, same grid, order mirrored per direction; one more launch
// gives the carry into dh0 / dc0.  With s the step whose gradients arrive
// (t + 1 forward, t - 1 reverse):
//   dh_t = dy_t + dG_s . W_hh[:, J]       (the product against W_hh^T, K = 4H)
//   dc_t = f_s * dc_s + dh_t * o_t * (1 - tanh^2 c_t)
//   di = dc g i(1-i)   df = dc c_prev f(1-f)   dg = dc i (1-g^2)   do = dh tanh(c) o(1-o)
// dG (B, T, D, 4H) is both the gradient of gi and the operand of the next
// step's product.  A row masked at s passes dh and dc through; a row inactive
// at t writes zero dG.  dh and dc ping-pong between the two halves of a
// (2, 2, D, B, H) buffer.
#include "rnnstep.h"

using namespace sbk;
using namespace sbk::rnnstep;

namespace {

struct FwdArgs {
  const void* w_hh;      // (D, 4H, H) in the compute dtype
  const float* b_hh;     // (D, 4H) or null
  const float* hx;       // (D, B, H) or null
  const float* cx;       // (D, B, H) or null
  const float* gi;       // (B, T, D, 4H) or null
  const int* tok;        // (B, T) or null
  const float* table;    // (I, D, 4H): the stacked W_ih, transposed
  const float* b_ih;     // (D, 4H) or null (token mode)
  const int* lens;       // (B) or null
  float* hstate;         // (B, T, D * H)
  float* cstate;         // (B, T, D * H)
  float* y;              // (B, T, D * H) or null
  float* save;           // (B, T, D, 4H) or null
  int blank, I, B, T, H, D;
  int vec_w, vec_h;
};

// launch s in [0, T): time s in direction 0, T-1-s in direction 1
template <typename T>
__global__ void __launch_bounds__(kThreads) lstm_fwd_step_kernel(FwdArgs a, int s) {
  __shared__ float red[kWaves][4][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, B = a.B, Tn = a.T, D = a.D;
  const int d = blockIdx.z;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const int t = d ? Tn - 1 - s : s;
  const int tp = d ? t + 1 : t - 1;      // the step this one continues
  const long long DH = (long long)D * H;
  // previous (h, c) of direction d: rows of (hx, cx) at the first launch
  const long long ldp = s == 0 ? H : Tn * DH;
  const long long offp = s == 0 ? (long long)d * B * H : tp * DH + (long long)d * H;
  const float* hprev = s == 0 ? (a.hx ? a.hx + offp : nullptr) : a.hstate + offp;
  const float* cprev = s == 0 ? (a.cx ? a.cx + offp : nullptr) : a.cstate + offp;

  f32x4 acc[kMT][4];
  product<T, 4>(acc, static_cast<const T*>(a.w_hh) + (long long)d * 4 * H * H, H, H, hprev, ldp, j0, b0, B, H, mts,
                a.vec_w, a.vec_h, lane, w);
  meet<4>(red, acc, mts, lane, w);

  const long long H4 = 4LL * H;
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    const long long bt = (long long)b * Tn + t;
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float sum = total<4>(red, g, rr, jj);
      pre[g] = a.b_hh ? sum + a.b_hh[d * H4 + g * H + j] : sum;
    }
    if (a.tok) {
      const int idx = token_row(a.tok[bt], a.blank);
      const bool hit = idx >= 0 && idx < a.I;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float x = hit ? a.table[((long long)idx * D + d) * H4 + g * H + j] : 0.f;
        pre[g] += a.b_ih ? x + a.b_ih[d * H4 + g * H + j] : x;
      }
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[g] += a.gi[(bt * D + d) * H4 + g * H + j];
    }
    const float hp = hprev ? hprev[b * ldp + j] : 0.f;
    const float cp = cprev ? cprev[b * ldp + j] : 0.f;
    const float ig = sigmoid_exact(pre[0]);
    const float fg = sigmoid_exact(pre[1]);
    const float gg = tanhf(pre[2]);
    const float og = sigmoid_exact(pre[3]);
    const float c = fg * cp + ig * gg;
    const float h = og * tanhf(c);
    const bool active = !a.lens || t < a.lens[b];
    const long long o = bt * DH + (long long)d * H + j;
    a.hstate[o] = active ? h : hp;
    a.cstate[o] = active ? c : cp;
    if (a.y) a.y[o] = active ? h : 0.f;
    if (a.save) {
      float* sv = a.save + (bt * D + d) * H4 + j;
      sv[0] = ig;
      sv[H] = fg;
      sv[2 * H] = gg;
      sv[3 * H] = og;
    }
  }
}

struct BwdArgs {
  const void* w_hhT;     // (D, H, 4H) in the compute dtype
  const float* cx;       // (D, B, H) or null
  const float* cstate;   // (B, T, D * H)
  const float* save;     // (B, T, D, 4H)
  const float* dy;       // (B, T, D * H) or null
  const float* dhn;      // (D, B, H) or null
  const float* dcn;      // (D, B, H) or null
  const int* lens;       // (B) or null
  float* dG;             // (B, T, D, 4H)
  float* dw;             // (2, 2, D, B, H): parity, (dh, dc)
  float* dhx;            // (D, B, H)
  float* dcx;            // (D, B, H)
  int B, T, H, D;
  int vec_w, vec_g;
};

// launch s in [0, T]: time T-1-s in direction 0, s in direction 1; the last
// launch (time -1 / T) computes the carry into dhx, dcx only
template <typename T>
__global__ void __launch_bounds__(kThreads) lstm_bwd_step_kernel(BwdArgs a, int s) {
  __shared__ float red[kWaves][1][kRows][kSlice];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, B = a.B, Tn = a.T, D = a.D;
  const int K = 4 * H;
  const int d = blockIdx.z;
  const int j0 = blockIdx.x * kSlice, b0 = blockIdx.y * kRows;
  const int nrows = B - b0 < kRows ? B - b0 : kRows;
  const int mts = (nrows + 15) >> 4;
  const int t = d ? s : Tn - 1 - s;
  const int ts = d ? t - 1 : t + 1;      // the step whose gradients arrive
  const int tp = d ? t + 1 : t - 1;      // the step this one continued
  const bool arrives = s > 0;
  const bool last = s == Tn;
  const long long DH = (long long)D * H;

  // the K loop of rnnstep.h's product for one tile, kept here: through the
  // shared one a bf16 forward + backward call was 3-4 % slower
  f32x4 acc[kMT][1];
#pragma unroll
  for (int m = 0; m < kMT; ++m) acc[m][0] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (arrives) {
    const T* W = static_cast<const T*>(a.w_hhT) + (long long)d * H * K;
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
  const long long half = 2 * D * BH;     // one parity of dw
  for (int e = tid; e < nrows * kSlice; e += kThreads) {
    const int rr = e >> 4, jj = e & 15;
    const int b = b0 + rr, j = j0 + jj;
    if (j >= H) continue;
    const long long bj = d * BH + (long long)b * H + j;
    float ch, cc;   // what step ts hands to the (h, c) it started from
    if (!arrives) {
      ch = a.dhn ? a.dhn[bj] : 0.f;
      cc = a.dcn ? a.dcn[bj] : 0.f;
    } else {
      const float* src = a.dw + (ts & 1) * half + bj;
      const float dhs = src[0], dcs = src[D * BH];
      if (!a.lens || ts < a.lens[b]) {
        ch = total<1>(red, 0, rr, jj);
        cc = a.save[(((long long)b * Tn + ts) * D + d) * K + H + j] * dcs;
      } else {
        ch = dhs;
        cc = dcs;
      }
    }
    if (last) {
      a.dhx[bj] = ch;
      a.dcx[bj] = cc;
      continue;
    }
    const long long bt = (long long)b * Tn + t;
    const bool active = !a.lens || t < a.lens[b];
    const float dh = ch + (active && a.dy ? a.dy[bt * DH + (long long)d * H + j] : 0.f);
    float dc = cc;
    float di = 0.f, df = 0.f, dg = 0.f, dov = 0.f;
    if (active) {
      const float* sv = a.save + (bt * D + d) * K + j;
      const float ig = sv[0], fg = sv[H], gg = sv[2 * H], og = sv[3 * H];
      const float tc = tanhf(a.cstate[bt * DH + (long long)d * H + j]);
      const float cp = s == Tn - 1 ? (a.cx ? a.cx[bj] : 0.f)
                              : a.cstate[((long long)b * Tn + tp) * DH + (long long)d * H + j];
      dc += dh * og * (1.f - tc * tc);
      di = dc * gg * ig * (1.f - ig);
      df = dc * cp * fg * (1.f - fg);
      dg = dc * ig * (1.f - gg * gg);
      dov = dh * tc * og * (1.f - og);
    }
    float* dst = a.dw + (t & 1) * half + bj;
    dst[0] = dh;
    dst[D * BH] = dc;
    float* g = a.dG + (bt * D + d) * K + j;
    g[0] = di;
    g[H] = df;
    g[2 * H] = dg;
    g[3 * H] = dov;
  }
}

}  // namespace

// The T forward launches of one LSTM layer, D = 1 or 2 directions.  bf16:
// w_hh is bf16 (else fp32), (D, 4H, H) row-major.  Input pre-activations: gi
// (B, T, D, 4H) fp32 with b_ih already added, or tok (B, T) int32 token ids
// with table = the stacked W_ih transposed (I, D, 4H) fp32 and b_ih (D, 4H)
// (token id `blank` has no row; ids above it use row id - 1).  hx, cx
// (D, B, H) or null (zeros).  lens (B) int32 steps per row, or null.  hstate,
// cstate (B, T, D * H): the carried (h, c) after every step; y (B, T, D * H)
// or null: the output (zero past a row's length); save (B, T, D, 4H) or null:
// i, f, g, o.
SBK_API int sbk_lstm_fwd(int bf16, int D, const void* w_hh, const float* b_hh, const float* hx, const float* cx,
                         const float* gi, const int* tok, int blank, const float* table, int I, const float* b_ih,
                         const int* lens, int B, int T, int H, float* hstate, float* cstate, float* y, float* save,
                         void* stream) {
  if (!w_hh || !hstate || !cstate || (!gi && !tok) || (gi && tok)) return SBK_ERR_ARG;
  if (tok && (!table || I <= 0)) return SBK_ERR_ARG;
  if (B <= 0 || T <= 0 || H <= 0 || (D != 1 && D != 2)) return SBK_ERR_ARG;
  if ((long long)D * 4 * H * H > 0x7fffffffLL || (long long)B * T * D > 0x7fffffffLL / 4) return SBK_ERR_ARG;
  FwdArgs a;
  a.w_hh = w_hh; a.b_hh = b_hh; a.hx = hx; a.cx = cx; a.gi = gi; a.tok = tok; a.table = table; a.b_ih = b_ih;
  a.lens = lens; a.hstate = hstate; a.cstate = cstate; a.y = y; a.save = save;
  a.blank = blank; a.I = I; a.B = B; a.T = T; a.H = H; a.D = D;
  a.vec_w = aligned16(w_hh) && H % (bf16 ? 8 : 4) == 0;
  a.vec_h = aligned16(hstate) && H % 4 == 0 && (!hx || aligned16(hx));
  return launch_steps(bf16 ? lstm_fwd_step_kernel<bf16_t> : lstm_fwd_step_kernel<float>, a, D, 0, T, 1, stream);
}

// The T backward launches and the carry into (dhx, dcx).  w_hhT = W_hh^T per
// direction (D, H, 4H) in the compute dtype; cx, cstate, save, lens as given
// to / written by sbk_lstm_fwd; dy (B, T, D * H) or null, dhn, dcn (D, B, H)
// or null.  Writes dG (B, T, D, 4H) fp32 (zero rows past a row's length) and
// dhx, dcx (D, B, H); dw (2, 2, D, B, H) is scratch.
SBK_API int sbk_lstm_bwd(int bf16, int D, const void* w_hhT, const float* cx, const float* cstate, const float* save,
                         const float* dy, const float* dhn, const float* dcn, const int* lens, int B, int T, int H,
                         float* dG, float* dw, float* dhx, float* dcx, void* stream) {
  if (!w_hhT || !cstate || !save || !dG || !dw || !dhx || !dcx) return SBK_ERR_ARG;
  if (B <= 0 || T <= 0 || H <= 0 || (D != 1 && D != 2)) return SBK_ERR_ARG;
  if ((long long)D * 4 * H * H > 0x7fffffffLL || (long long)B * T * D > 0x7fffffffLL / 4) return SBK_ERR_ARG;
  BwdArgs a;
  a.w_hhT = w_hhT; a.cx = cx; a.cstate = cstate; a.save = save; a.dy = dy; a.dhn = dhn; a.dcn = dcn; a.lens = lens;
  a.dG = dG; a.dw = dw; a.dhx = dhx; a.dcx = dcx;
  a.B = B; a.T = T; a.H = H; a.D = D;
  // rows of 4H elements: 16-byte aligned in fp32, in bf16 for even H
  a.vec_w = aligned16(w_hhT) && (!bf16 || H % 2 == 0);
  a.vec_g = aligned16(dG);
  return launch_steps(bf16 ? lstm_bwd_step_kernel<bf16_t> : lstm_bwd_step_kernel<float>, a, D, 0, T + 1, 1, stream);
}
