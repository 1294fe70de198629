// Fused Transformer-XL relative-position self-attention (RelPosMHAXL).
//
// Reference: speechbrain/nnet/attention.py:485-639 (RelPosMHAXL.forward),
// rel_shift :468-483.  For query i, key j (T queries = T keys):
//   score[i,j] = ( (q_i + u)·k_j  +  (q_i + v)·p_{T-1-i+j} ) / sqrt(d_model)
//   key-padding -> -inf, softmax over j, out_i = Σ_j P[i,j] v_j
// with p = linear_pos(RelPosEncXL) and rel_shift in closed form
// (out[i,j] = bd[i, T-1-i+j]); the (B,H,T,2T-1) bd tensor the reference
// materialises (145 MB at B=32, T=376) never exists.
//
// Flash-style, transposed formulation (MI355X wave64 + 16x16 MFMA):
//  * workgroup = (b, h, 64 queries), 4 waves x 16 queries; 64-key chunks of
//    K, V^T and the 127 positional rows the chunk needs are staged in LDS
//    with 16-B loads, shared by the 4 waves.
//  * each wave computes S^T = K·Qu^T (4 tiles) — the query sits on the lane,
//    so softmax statistics are per-lane (+2 xor-shuffles) — and
//    G^T = P_band·Qv^T (5 tiles); the rel_shift gather S^T[jj][ii] +=
//    G^T[15-ii+jj][ii] stays inside the lane's column via a 5 KB per-wave
//    LDS scratch.
//  * O^T = V^T·P^T accumulates with P taken straight from the S registers
//    (permuted-k fragments: keys {4g..4g+3, 16+4g..16+4g+3} per 32-key step,
//    V^T read in the same order) — no LDS round trip for P.
//  * online softmax (running max / sum, rescale) when no probabilities are
//    requested; with probabilities (the reference's returned attention map)
//    a stats pass then an exact pass that writes P and accumulates P·V.
// bf16 operands use v_mfma_f32_16x16x32_bf16, fp32 operands exact f32 MFMA
// (mfma.h); softmax and accumulators are fp32.
#include "lds_dma.h"
#include "mfma.h"

using namespace sbk;

namespace {


constexpr int QB = 64;        // queries per workgroup
constexpr int KC = 64;        // keys per chunk
constexpr int PBR = KC + QB;  // positional band rows staged per chunk (127 used)
constexpr int GR = 80;        // G^T rows per wave (79 used)
constexpr int GS = 20;        // G^T scratch row stride (floats): conflict-free writes and shifted reads

constexpr float LOG2E = 1.4426950408889634f;

template <typename T, int DHP>
struct FlashLds {
  // bf16: +32 B row pad makes the 16-lane ds_read_b128 groups of the K / P
  // fragment reads and the ds_read_b64_tr_b16 V reads conflict-free (+16 B
  // left 2-way conflicts); fp32: +16 B
  static constexpr int PAD = sizeof(T) == 2 ? 2 * MT<T>::PAD : MT<T>::PAD;
  static constexpr bool TRV = sizeof(T) == 2;  // bf16: V row-major + ds_read_tr16; fp32: V^T staged transposed
  static constexpr int KR = DHP + PAD;  // Ks / Ps / V(row-major) row stride
  static constexpr int VR = KC + PAD;   // Vt row stride (fp32 path)
  static constexpr size_t ks = (size_t)KC * KR * sizeof(T);
  static constexpr size_t vt = TRV ? (size_t)KC * KR * sizeof(T) : (size_t)DHP * VR * sizeof(T);
  static constexpr size_t ps = (size_t)PBR * KR * sizeof(T);
  static constexpr size_t gs = (size_t)4 * GR * GS * 4;
  static constexpr size_t ms = (size_t)(KC + 4) * 4;  // key mask + 'chunk has a masked key' flag
  // The per-wave G^T scratch aliases the K and positional-band tiles, which
  // are dead once every wave's S / G MFMAs have consumed them (one barrier):
  // 66 -> 40 KB per workgroup, three workgroups per CU instead of two, and
  // the 768 workgroups of a B = 32, T = 376 launch fit in one round.
  static_assert(gs <= ks + ps, "G^T scratch fits over Ks + Ps");
  static constexpr size_t bytes = ks + ps + vt + ms;
};

// Out-of-range K / V / positional rows are zeroed at commit.  (Tried:
// committing the clamped loads unmasked — the rows only meet masked scores —
// measured 36 -> 54 us: the compiler then sank the prefetch loads to their
// stores; and head dims >= dh must stay zero when dh is not a multiple of the
// 8-dim Q fragment, whose vector loads then read the next section.)
// component-wise select (a struct-valued ?: takes the operands' addresses and
// sends the staging arrays to scratch)
__device__ __forceinline__ uint4 sel4(bool c, const uint4& a) {
  return make_uint4(c ? a.x : 0u, c ? a.y : 0u, c ? a.z : 0u, c ? a.w : 0u);
}

// ---------------------------------------------------------------------------
// Pieces shared by the two kernels below (the k-transposed V fragment reader
// is frag_tr of mfma.h, the LDS-DMA piece lds_dma16 of lds_dma.h).  Each kernel
// keeps its own Q-fragment build, S^T / G^T and P·V loops and output store:
// written as shared steps they changed the LDS-DMA kernel's chunk loop or
// added spills to the general kernel
// (profiles/attn_tile_primitives_asm_vs_parent.md).  The row max / row sum
// reductions differ on purpose: they round differently.
// ---------------------------------------------------------------------------

// Where a workgroup works: head h of utterance b, queries i0 .. i0 + QB - 1.
// XCD-aware bijective remap: workgroups are dealt round-robin to the 8 XCDs;
// give each XCD a contiguous run of tiles so the query blocks of one (b, h)
// share an L2 and its K/V/positional rows are fetched from HBM once.
template <typename T>
struct TileOrigin {
  int tile, h, b, i0, d_model;
  long long row3;  // qkv row stride
  const T* qkv_b;  // this (b, h)'s [q|k|v] section of row 0
  const T* pk_h;   // this head's columns of the positional rows
};
template <typename T>
__device__ __forceinline__ TileOrigin<T> tile_origin(const T* qkv, const T* pk, int Tn, int H, int dh) {
  TileOrigin<T> o;
  o.d_model = H * dh;
  o.row3 = 3LL * o.d_model;
  const int nqb = (Tn + QB - 1) / QB;
  o.tile = xcd_tile(gridDim.x, blockIdx.x);
  const int qb = o.tile % nqb, bh = o.tile / nqb;
  o.h = bh % H;
  o.b = bh / H;
  o.i0 = qb * QB;
  o.qkv_b = qkv + (long long)o.b * Tn * o.row3 + o.h * 3 * dh;
  o.pk_h = pk + o.h * dh;
  return o;
}

// ---- key mask staging and softmax step of the general kernel ----
// additive key mask of key j: -inf past Tn and for a padded key
__device__ __forceinline__ float key_mask(const uint8_t* kpm, int b, int j, int Tn) {
  return (j < Tn && !(kpm && kpm[(long long)b * Tn + min(j, Tn - 1)])) ? 0.f : -INFINITY;
}
// wave 0 (KC == 64): mask values and the chunk's any-masked flag
__device__ __forceinline__ void stage_mask(float* Ms, int tid, float mv) {
  Ms[tid] = mv;
  const bool anym = __any(mv != 0.f);
  if (tid == 0) reinterpret_cast<int*>(Ms)[KC] = anym;
}
// One chunk of the online softmax: p = exp2(sc - max), row sum as a serial
// sum and two xor-shuffles, l_run / m_run updated; returns the rescale of
// what was accumulated under the old maximum.
__device__ __forceinline__ float chunk_expsum(const float (&sc)[4][4], float cmax, float& m_run, float& l_run,
                                              float (&p)[4][4]) {
  const float m_new = fmaxf(m_run, cmax);
  const float mref = m_new == -INFINITY ? 0.f : m_new;
  const float alpha = __builtin_amdgcn_exp2f(m_run - mref);
  float ls = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[t][r] = __builtin_amdgcn_exp2f(sc[t][r] - mref);
      ls += p[t][r];
    }
  ls += __shfl_xor(ls, 16);
  ls += __shfl_xor(ls, 32);
  l_run = l_run * alpha + ls;
  m_run = m_new;
  return alpha;
}

// s_memtime marks of the waves of one workgroup, and per workgroup its
// memrealtime / memtime at start and end (probe builds only)
SBK_PROBE_BUFFER(g_att_tl, 4, 64)
SBK_PROBE_BUFFER(g_att_wg, 4096, 4)
#define ATT_TL(i) SBK_PROBE(if (tl_on && lane == 0 && (i) < 64) g_att_tl[w][i] = __builtin_amdgcn_s_memtime();)

template <typename T, int DHP, bool PROBS>
__global__ void __launch_bounds__(256, 2) relpos_flash_kernel(const T* __restrict__ qkv, const T* __restrict__ pk,
                                                           const float* __restrict__ pbu,
                                                           const float* __restrict__ pbv,
                                                           const uint8_t* __restrict__ kpm, int Tn, int H,
                                                           int dh, float scale, T* __restrict__ out,
                                                           float* __restrict__ probs, int vec_ok, int ldp,
                                                           const float* __restrict__ am, long long am_sb,
                                                           long long am_sh) {
  using Tr = MT<T>;
  using L = FlashLds<T, DHP>;
  constexpr int KR = L::KR, VR = L::VR, VEC = Tr::VEC;
  constexpr bool TRV = L::TRV;
  constexpr int KS = DHP / 32;   // k-steps over the head dim
  constexpr int NDT = DHP / 16;  // O^T tiles (head-dim rows)
  constexpr int CPR = DHP / VEC; // 16-B chunks per staged row
  constexpr int NKC = KC * CPR / 256;   // K (and V) chunks per thread
  constexpr int NPC = PBR * CPR / 256;  // P-band chunks per thread
  static_assert(KC == 64, "mask staging: one wave per chunk");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* Ks = reinterpret_cast<T*>(smem);
  T* Ps = reinterpret_cast<T*>(smem + L::ks);
  T* Vs = reinterpret_cast<T*>(smem + L::ks + L::ps);
  float* Gs = reinterpret_cast<float*>(smem);  // over Ks + Ps (dead after the S / G MFMAs)
  float* Ms = reinterpret_cast<float*>(smem + L::ks + L::ps + L::vt);

  const TileOrigin<T> o = tile_origin(qkv, pk, Tn, H, dh);
  const int h = o.h, b = o.b, i0 = o.i0;
  const long long row3 = o.row3;
  const T* qkv_b = o.qkv_b;
  const T* pk_h = o.pk_h;
  SBK_PROBE(const bool tl_on = o.tile == 200 && sizeof(T) == 2 && !PROBS;)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int my_i = i0 + 16 * w + c16;  // this lane's query
  float* Gw = Gs + w * GR * GS;

  // ---- Qu / Qv as B-operand fragments (query on the lane), pre-scaled by
  // scale * log2(e) so scores come out of the MFMAs in the exp2 domain ----
  const float qscale = scale * LOG2E;
  typename Tr::frag fqu[KS], fqv[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    float qu[8], qv[8];
    const int d0 = 32 * s + 8 * g;
    if (vec_ok && d0 < dh) {  // 8 consecutive head dims: 16-B (bf16) / 2x16-B (fp32) loads
      const T* qp = qkv_b + (long long)min(my_i, Tn - 1) * row3 + d0;
      float qf[8];
      if constexpr (sizeof(T) == 2) {
        const uint4 q4 = *reinterpret_cast<const uint4*>(qp);
        const uint32_t wv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = __uint_as_float((wv[e >> 1] >> (16 * (e & 1))) << 16);
      } else {
        const float4 a4 = *reinterpret_cast<const float4*>(qp), b4 = *reinterpret_cast<const float4*>(qp + 4);
        qf[0] = a4.x; qf[1] = a4.y; qf[2] = a4.z; qf[3] = a4.w;
        qf[4] = b4.x; qf[5] = b4.y; qf[6] = b4.z; qf[7] = b4.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // fp32 with dh % 8 == 4: the fragment's upper half lies past this
        // head's dims (qf holds the K section's first values there, and the
        // biases would be the next head's, or past the end of the vectors for
        // the last head).  Bias loads stay unconditional on a clamped index;
        // those dims are zero in the fragment.
        const bool live = my_i < Tn && d0 + e < dh;
        const int db = h * dh + min(d0 + e, dh - 1);
        qu[e] = live ? (qf[e] + pbu[db]) * qscale : 0.f;
        qv[e] = live ? (qf[e] + pbv[db]) * qscale : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int d = d0 + e;
        if (my_i < Tn && d < dh) {
          const float q = Tr::to_f32(qkv_b[(long long)my_i * row3 + d]);
          qu[e] = (q + pbu[h * dh + d]) * qscale;
          qv[e] = (q + pbv[h * dh + d]) * qscale;
        } else {
          qu[e] = 0.f;
          qv[e] = 0.f;
        }
      }
    }
    fqu[s] = Tr::from8(qu);
    fqv[s] = Tr::from8(qv);
  }

  float m_run = -INFINITY, l_run = 0.f;
  f32x4 acc_o[NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t) acc_o[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int Tp = (Tn + KC - 1) / KC * KC;
  const int nchunk = Tp / KC;

  // ---- staging: registers (vector path) -> LDS ----
  uint4 rk[NKC], rv[NKC], rp[NPC];
  float rm = 0.f;
  // loads are unconditional (indices clamped into range) and out-of-range
  // values are zeroed at commit: a predicated load would make the compiler
  // wait for it on its own path, serialising the prefetch with the chunk math
  bool okk[NKC], okp[NPC];
  auto fetch = [&](int j0, bool need_v) {
    const int rbase = Tn - QB - i0 + j0;
#pragma unroll
    for (int i = 0; i < NKC; ++i) {
      const int c = tid + 256 * i, r = c / CPR, d = (c % CPR) * VEC, j = j0 + r;
      okk[i] = j < Tn && d < dh;
      const T* src = qkv_b + (long long)min(j, Tn - 1) * row3 + dh + min(d, dh - VEC);
      rk[i] = *reinterpret_cast<const uint4*>(src);
      rv[i] = *reinterpret_cast<const uint4*>(src + (need_v ? dh : 0));  // (stats pass: unused re-read of K)
    }
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int c = tid + 256 * i, rr = c / CPR, d = (c % CPR) * VEC, r = rbase + rr;
      okp[i] = rr < PBR - 1 && r >= 0 && r <= 2 * Tn - 2 && d < dh;
      rp[i] = *reinterpret_cast<const uint4*>(pk_h + (long long)min(max(r, 0), 2 * Tn - 2) * ldp +
                                              min(d, dh - VEC));
    }
    if (tid < KC) rm = key_mask(kpm, b, j0 + tid, Tn);
  };
  auto commit = [&](bool need_v) {
#pragma unroll
    for (int i = 0; i < NKC; ++i) {
      const int c = tid + 256 * i, r = c / CPR, d = (c % CPR) * VEC;
      *reinterpret_cast<uint4*>(Ks + r * KR + d) = sel4(okk[i], rk[i]);
      if (need_v) {
        const uint4 vv = sel4(okk[i], rv[i]);
        if (TRV) {
          *reinterpret_cast<uint4*>(Vs + r * KR + d) = vv;
        } else {
          const T* ve = reinterpret_cast<const T*>(&vv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) Vs[(d + e) * VR + r] = ve[e];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int c = tid + 256 * i, rr = c / CPR, d = (c % CPR) * VEC;
      *reinterpret_cast<uint4*>(Ps + rr * KR + d) = sel4(okp[i], rp[i]);
    }
    if (tid < KC) stage_mask(Ms, tid, rm);
  };
  auto stage_scalar = [&](int j0, bool need_v) {  // unaligned head dims (e.g. d=144, H=4)
    const int rbase = Tn - QB - i0 + j0;
    for (int e = tid; e < KC * DHP; e += 256) {
      const int r = e / DHP, d = e - r * DHP, j = j0 + r;
      const bool ok = j < Tn && d < dh;
      Ks[r * KR + d] = ok ? qkv_b[(long long)j * row3 + dh + d] : Tr::from_f32(0.f);
      if (need_v) {
        const T v = ok ? qkv_b[(long long)j * row3 + 2 * dh + d] : Tr::from_f32(0.f);
        if (TRV)
          Vs[r * KR + d] = v;
        else
          Vs[d * VR + r] = v;
      }
    }
    for (int e = tid; e < PBR * DHP; e += 256) {
      const int rr = e / DHP, d = e - rr * DHP, r = rbase + rr;
      Ps[rr * KR + d] = (rr < PBR - 1 && r >= 0 && r <= 2 * Tn - 2 && d < dh) ? pk_h[(long long)r * ldp + d]
                                                                              : Tr::from_f32(0.f);
    }
    if (tid < KC) stage_mask(Ms, tid, key_mask(kpm, b, j0 + tid, Tn));
  };

  constexpr int NPASS = PROBS ? 2 : 1;
  for (int pass = 0; pass < NPASS; ++pass) {
    const bool stats_only = PROBS && pass == 0;
    const bool need_v = !stats_only;
    __syncthreads();
    if (vec_ok) {
      fetch(0, need_v);
      commit(need_v);
    } else {
      stage_scalar(0, need_v);
    }
    __syncthreads();
    ATT_TL(0);
    for (int ch = 0; ch < nchunk; ++ch) {
      ATT_TL(1 + 6 * ch);
      const int j0 = ch * KC;
      const bool more = ch + 1 < nchunk;
      if (vec_ok && more) fetch(j0 + KC, need_v);  // next chunk in flight during this chunk's math

      // ---- S^T (keys x queries) and G^T (band rows x queries) ----
      // per 32-wide head-dim step: all 9 fragment reads, then the 9 MFMAs;
      // G^T goes to the scratch only after its last MFMA (no read -> MFMA ->
      // store serialisation per tile)
      f32x4 acc_s[4], acc_g[5];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc_s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 5; ++t) acc_g[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int pofs = 48 - 16 * w;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        typename Tr::frag fk[4], fpb[5];
#pragma unroll
        for (int t = 0; t < 4; ++t) fk[t] = Tr::load(Ks + (16 * t + c16) * KR + 8 * g + 32 * s);
#pragma unroll
        for (int t = 0; t < 5; ++t) fpb[t] = Tr::load(Ps + (pofs + 16 * t + c16) * KR + 8 * g + 32 * s);
#pragma unroll
        for (int t = 0; t < 4; ++t) Tr::mma(acc_s[t], fk[t], fqu[s]);
#pragma unroll
        for (int t = 0; t < 5; ++t) Tr::mma(acc_g[t], fpb[t], fqv[s]);
      }
      __syncthreads();  // every wave's Ks / Ps fragment reads are done: the scratch may overwrite them
#pragma unroll
      for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) Gw[(16 * t + 4 * g + r) * GS + c16] = acc_g[t][r];
      // G^T scratch is per wave: its LDS writes only need to have completed
      // (in-order per wave) before the shifted reads, no workgroup barrier
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

      ATT_TL(2 + 6 * ch);
      // ---- scores for this lane's query: keys jj = 16t + 4g + r ----
      // (log2 domain: Qu/Qv carry scale * log2(e), probabilities are exp2)
      const bool masked_chunk = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(Ms)[KC]) != 0;
      float sc[4][4];
      float cmax = -INFINITY;
      // additive attention mask (attn_mask, attention.py:604-611), scaled into
      // the log2 domain of the scores; bool masks arrive as 0 / -inf
      const float* amrow = am ? am + b * am_sb + h * am_sh + (long long)min(my_i, Tn - 1) * Tn : nullptr;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int jj = 16 * t + 4 * g + r;
          float v = acc_s[t][r] + Gw[(15 - c16 + jj) * GS + c16];
          if (masked_chunk) v += Ms[jj];
          if (amrow && j0 + jj < Tn) v += amrow[j0 + jj] * LOG2E;
          sc[t][r] = v;
          cmax = fmaxf(cmax, v);
        }
      cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
      cmax = fmaxf(cmax, __shfl_xor(cmax, 32));

      float p[4][4];
      if (stats_only) {
        chunk_expsum(sc, cmax, m_run, l_run, p);
      } else {
        if (PROBS) {
          const float mref = m_run == -INFINITY ? 0.f : m_run;
          const float inv = 1.0f / l_run;
          float* prow = probs + (((long long)b * H + h) * Tn + my_i) * Tn;
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int j = j0 + 16 * t + 4 * g + r;
              p[t][r] = __builtin_amdgcn_exp2f(sc[t][r] - mref) * inv;
              if (my_i < Tn && j < Tn) prow[j] = p[t][r];
            }
        } else {
          const float alpha = chunk_expsum(sc, cmax, m_run, l_run, p);
#pragma unroll
          for (int t = 0; t < NDT; ++t) acc_o[t] *= alpha;
        }
        ATT_TL(3 + 6 * ch);
        // ---- O^T += V^T · P^T  (2 k-steps of 32 keys) ----
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          float pv[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            pv[r] = p[2 * s2][r];
            pv[4 + r] = p[2 * s2 + 1][r];
          }
          const typename Tr::frag fp = Tr::from8(pv);
#pragma unroll
          for (int t = 0; t < NDT; ++t) {
            typename Tr::frag fa;
            if constexpr (TRV) {
              fa = frag_tr(Vs, KR, 32 * s2, 16 * t, lane);
            } else {
              const T* vrow = Vs + (16 * t + c16) * VR + 32 * s2 + 4 * g;
              fa = Tr::load2x4(vrow, vrow + 16);
            }
            Tr::mma(acc_o[t], fa, fp);
          }
        }
      }
      ATT_TL(4 + 6 * ch);
      __syncthreads();  // every wave done with this chunk's Ks / Vs / Ps / Gs
      ATT_TL(5 + 6 * ch);
      if (more) {
        if (vec_ok)
          commit(need_v);
        else
          stage_scalar(j0 + KC, need_v);
        __syncthreads();
      }
    }
  }
  ATT_TL(62);
  // ---- write O (row = this lane's query, cols d = 16t + 4g + r) ----
  if (my_i < Tn) {
    const float inv = PROBS ? 1.0f : 1.0f / l_run;
    T* orow = out + ((long long)b * Tn + my_i) * o.d_model + h * dh;
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
      const int d = 16 * t + 4 * g;
      if (vec_ok && d + 3 < dh) {  // 4 consecutive head dims: one 8-B (bf16) / 16-B (fp32) store
        if constexpr (sizeof(T) == 2) {
          uint2 pk2;
          pk2.x = pack_bf16x2(acc_o[t][0] * inv, acc_o[t][1] * inv);
          pk2.y = pack_bf16x2(acc_o[t][2] * inv, acc_o[t][3] * inv);
          *reinterpret_cast<uint2*>(orow + d) = pk2;
        } else {
          *reinterpret_cast<float4*>(orow + d) =
              make_float4(acc_o[t][0] * inv, acc_o[t][1] * inv, acc_o[t][2] * inv, acc_o[t][3] * inv);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (d + r < dh) orow[d + r] = Tr::from_f32(acc_o[t][r] * inv);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The encoder's inference path — bf16, dh = 64, no probabilities — with
// three workgroups per CU.  The kernel above carries the next chunk's K / V /
// band rows in 32 VGPRs (212 in all), so it runs two waves per SIMD: at
// B = 32, T = 376 its 768 workgroups take 1.5 rounds of 512.  Its score
// assembly was also 16 serialised LDS round trips per chunk (a per-chunk
// "any key masked" branch split it into read -> wait -> add steps).
// Here the tiles go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no
// VGPRs, no ds_write) into unpadded 128-B rows whose 16-B chunks are
// XOR-swizzled on the global source address — K and the band:
// chunk ^ ((row >> 1) & 7), conflict-free ds_read_b128 fragments; V:
// chunk ^ (((row >> 1) & 3) << 1), conflict-free ds_read_b64_tr_b16.  G^T goes
// to a query-major scratch with the rel_shift applied on the write (row R of
// query ii lands at position R - (15 - ii); the first / last tile's positions
// outside the chunk's 64 keys clamp onto two spare slots), so the scores are
// four aligned 16-B reads.  Key padding: a 64-bit bitmap of the chunks that
// hold a padded key is built once per workgroup; only those chunks (and the
// last, for keys past Tn) apply a mask, so no wave writes a per-chunk mask row
// the others wait for.  Row max / sum: permlane half-swaps.  Two barriers per
// chunk:
//   A  this chunk's K / band landed in every wave and every wave is past the
//      previous chunk's P·V  -> issue this chunk's V;
//   B  V landed and every wave's S / G fragment reads are done -> read the
//      scratch, then issue the next chunk's K / band, which land under the
//      softmax and P·V.
// The band is a ring of two 64-row segments in the 16 KB of Ps: segment s
// holds band rows rbase0 + 64 s .. + 63 (rbase0 = Tn - QB - i0, rows clamped
// to [0, 2 Tn - 2]) in half s & 1, and chunk c reads segments c and c + 1 (its
// window row r is physical row (r + 64 (c & 1)) & 127).  The prologue stages
// segments 0 and 1; after barrier B of chunk c only segment c + 2 is staged,
// over segment c.  That needs no further barrier or wait: a wave passes B
// only after its own lgkmcnt(0), so every wave's fragment reads of segment c
// have returned before any wave issues the DMA that overwrites it, and the
// vmcnt(0) + barrier of A in chunk c + 1 puts the new rows in front of that
// chunk's reads, exactly as for K.  Segment c + 1 is not written while chunks
// c and c + 1 read it.  Per chunk and workgroup the DMA moves 24 KB (K 8,
// band 8, V 8; 32 KB when all 128 band rows were staged again), six pieces a
// wave instead of eight.  (Staging the band twice cost 0.8 us of the 20.4 us
// launch at B = 32, T = 376: profiles/attn_band_ring_timing.txt.)
// Measured (s_memtime / s_memrealtime per workgroup, B = 32, T = 376,
// profiles/r02_att_dma_timeline.log): all 768 workgroups start within 1 us
// (one round, three per CU); a CU's three finish in turn at ~12.5 / 15.3 /
// 17.5 us (oldest-first issue), i.e. the CU is issue / LDS bound, not waiting
// on memory.  Tried and slower: six waves x 16 queries per workgroup with
// double-buffered V and two workgroups per CU (27.5 us: the waves of a second
// workgroup do not always fit beside the first).
// The tiles are distinct __shared__ objects and the other LDS accesses come
// before a DMA is issued, so the compiler's LDS-DMA alias guard (a vmcnt wait
// before an LDS access it cannot tell apart from a DMA in flight) has little
// to wait for.  50 KB of LDS and 158 VGPRs (76 without the band): three
// workgroups per CU (168 VGPRs would still fit three waves per SIMD).
namespace dmak {
typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int RB = 64;   // bf16 per staged row (dh = 64): 128 B
constexpr int PB = 128;  // band rows a chunk reads (127 used): two segments of the ring
constexpr int PSEG = 64;  // band rows per ring segment (= KC: the window moves one segment per chunk)
constexpr int G2 = 72;   // G scratch row (floats): 18 16-B slots, ≡ 2 mod 4
constexpr int GO = 4;    // scratch index of key 0 (spare slots GO - 1 and GO + KC)
__device__ __forceinline__ int swz_kp(int row) { return (row >> 1) & 7; }
// V's chunk swizzle; equal for rows r and r + 16 (frag_tr)
__device__ __forceinline__ int swz_v(int row) { return ((row >> 1) & 3) << 1; }
// One LDS-DMA piece (lds_dma16: 64 lanes x 16 B to lds + 16 * lane; with the
// builtin the compiler waited for the next chunk's K / band before the P·V
// reads).  dma_barrier's vmcnt(0) + s_barrier is what orders the fills and
// the reads.
__device__ __forceinline__ void dma16(const bf16_t* src, bf16_t* lds) { lds_dma16(src, lds_addr(lds)); }

// The same piece from a wave-uniform base (SGPR pair) plus a per-lane byte
// offset computed once before the chunk loop; m0 (the LDS destination) is a
// precomputed scalar.  The interior chunks issue their DMAs with no VALU
// address arithmetic at all (the clamped form above cost ~75 VALU
// instructions per chunk, 8 of them quarter-rate multiplies, in a kernel
// whose chunk time is VALU issue).
__device__ __forceinline__ void dma16s(const void* sbase, uint32_t voff, uint32_t la) {
  asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(la) : "memory", "m0");
}
// LDS byte address of p, per lane (lds_addr is the wave-uniform form)
__device__ __forceinline__ uint32_t lds_lane_addr(const void* p) {
  return (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)p);
}
// this wave's DMA pieces and LDS accesses done, then the workgroup barrier
__device__ __forceinline__ void dma_barrier() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
}  // namespace dmak

// BAND = false: plain scaled dot-product attention (MultiheadAttention of the
// TransformerEncoder, attention.py:642-779 over nn.MultiheadAttention): no
// positional band, no u / v biases — no band DMA, no G tiles, no scatter,
// 16 KB of LDS; otherwise the same chunk loop.
template <bool BAND>
__global__ void __launch_bounds__(256, 3) relpos_flash_dma_kernel(const bf16_t* __restrict__ qkv,
                                                                  const bf16_t* __restrict__ pk, int ldp,
                                                                  const float* __restrict__ pbu,
                                                                  const float* __restrict__ pbv,
                                                                  const uint8_t* __restrict__ kpm, int Tn, int H,
                                                                  float scale, bf16_t* __restrict__ out) {
  using namespace dmak;
  constexpr int dh = 64;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[KC * RB];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[BAND ? PB * RB : 8];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[KC * RB];
  __shared__ __attribute__((aligned(16))) float Gs[BAND ? 4 * 16 * G2 : 4];
  __shared__ unsigned long long Mb[4];  // per-wave partial bitmaps of the chunks holding a padded key

  const TileOrigin<bf16_t> o = tile_origin(qkv, pk, Tn, H, dh);
  const int h = o.h, b = o.b, i0 = o.i0;
  const long long row3 = o.row3;
  const bf16_t* qkv_b = o.qkv_b;
  const bf16_t* pk_h = o.pk_h;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  const int my_i = i0 + 16 * w + c16;
  SBK_PROBE(const int orig = blockIdx.x; const bool tl_on = o.tile == 200;)
  float* gq = Gs + w * 16 * G2 + c16 * G2 + GO;  // this lane's query row of the G scratch, at key 0
  const int lrow = lane >> 3, lchk = lane & 7;   // DMA piece: 8 rows x 8 16-B chunks

  // per-lane byte offsets of the interior-chunk DMA pieces (row stride x row
  // + swizzled 16-B chunk); the chunk's base goes in the scalar operand
  uint32_t offk[2], offv[2], offp[2], lak[2], lav[2], lap[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r0 = 16 * w + 8 * i, row = r0 + lrow;
    offk[i] = (uint32_t)(row * row3 + ((lchk ^ swz_kp(row)) << 3)) * 2u;
    offv[i] = (uint32_t)(row * row3 + ((lchk ^ swz_v(row)) << 3)) * 2u;
    offp[i] = BAND ? (uint32_t)(row * ldp + ((lchk ^ swz_kp(row)) << 3)) * 2u : 0u;
    lak[i] = lds_addr(Ks + r0 * RB);
    lav[i] = lds_addr(Vs + r0 * RB);
    lap[i] = BAND ? lds_addr(Ps + r0 * RB) : 0u;
  }
  auto dma_k = [&](int j0) {
    if (j0 + KC <= Tn) {  // no row clamped
      const bf16_t* sk = qkv_b + (long long)j0 * row3 + dh;
#pragma unroll
      for (int i = 0; i < 2; ++i) dma16s(sk, offk[i], lak[i]);
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // K rows 16w .. 16w+15
      const int r0 = 16 * w + 8 * i, row = r0 + lrow;
      dma16(qkv_b + (long long)min(j0 + row, Tn - 1) * row3 + dh + ((lchk ^ swz_kp(row)) << 3), Ks + r0 * RB);
    }
  };
  // band segment sg (rows rbase0 + 64 sg .. + 63) into half `half` (= sg & 1)
  // of the ring: this wave's rows 16w .. 16w+15 of the segment
  auto dma_p = [&](int sg, int half) {
    const int rb = Tn - QB - i0 + PSEG * sg;    // the segment's band row 0
    if (rb >= 0 && rb + PSEG <= 2 * Tn - 1) {  // none of the 64 rows clamped
      const bf16_t* sp = pk_h + (long long)rb * ldp;
#pragma unroll
      for (int i = 0; i < 2; ++i) dma16s(sp, offp[i], lap[i] + half * (PSEG * RB * 2));
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r0 = 16 * w + 8 * i, rr = r0 + lrow;
      const int pr = min(max(rb + rr, 0), 2 * Tn - 2);
      dma16(pk_h + (long long)pr * ldp + ((lchk ^ swz_kp(rr)) << 3), Ps + (half * PSEG + r0) * RB);
    }
  };
  auto dma_v = [&](int j0) {
    if (j0 + KC <= Tn) {
      const bf16_t* sv = qkv_b + (long long)j0 * row3 + 2 * dh;
#pragma unroll
      for (int i = 0; i < 2; ++i) dma16s(sv, offv[i], lav[i]);
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r0 = 16 * w + 8 * i, row = r0 + lrow;
      dma16(qkv_b + (long long)min(j0 + row, Tn - 1) * row3 + 2 * dh + ((lchk ^ swz_v(row)) << 3), Vs + r0 * RB);
    }
  };
  ATT_TL(0);
  SBK_PROBE(if (tid == 0 && orig < 4096) {
    g_att_wg[orig][0] = __builtin_amdgcn_s_memrealtime();
    g_att_wg[orig][2] = __builtin_amdgcn_s_memtime();
  })
  dma_k(0);
  if constexpr (BAND) {
    dma_p(0, 0);
    dma_p(1, 1);
  }
  const int nchunk = (Tn + KC - 1) / KC;  // <= 64 (launcher)
  // Key padding: which chunks hold a padded key, as a 64-bit chunk bitmap
  // built once (wave w scans chunks w, w + 4, ...; merged after barrier A of
  // chunk 0).  Chunks without one add no mask at all; keys past Tn are masked
  // arithmetically in the last chunk.  (A per-chunk mask row written by one
  // wave made the other three wait for it at every barrier.)
  {
    unsigned long long bits = 0;
    if (kpm) {
      const uint8_t* kb = kpm + (long long)b * Tn;
      for (int c0 = w; c0 < nchunk; c0 += 8) {
        const int c1 = c0 + 4, ja = c0 * KC + lane, jb = c1 * KC + lane;
        const int ma = kb[min(ja, Tn - 1)];
        const int mb = c1 < nchunk ? (int)kb[min(jb, Tn - 1)] : 0;
        if (__ballot(ja < Tn && ma != 0)) bits |= 1ull << c0;
        if (__ballot(jb < Tn && mb != 0)) bits |= 1ull << c1;
      }
    }
    if (lane == 0) Mb[w] = bits;
  }
  uint32_t mlo = 0, mhi = 0;  // the merged bitmap (wave-uniform)

  // Qu / Qv B-operand fragments, pre-scaled into the exp2 domain
  const float qscale = scale * LOG2E;
  bf16x8 fqu[2], fqv[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int d0 = 32 * s + 8 * g;
    const uint4 q4 = *reinterpret_cast<const uint4*>(qkv_b + (long long)min(my_i, Tn - 1) * row3 + d0);
    const uint32_t wv[4] = {q4.x, q4.y, q4.z, q4.w};
    // biases by unconditional vector loads (guarded scalar loads each became
    // a branch and a full wait)
    const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 bu0 = BAND ? *reinterpret_cast<const f32x4*>(pbu + h * dh + d0) : z4;
    const f32x4 bu1 = BAND ? *reinterpret_cast<const f32x4*>(pbu + h * dh + d0 + 4) : z4;
    const f32x4 bv0 = BAND ? *reinterpret_cast<const f32x4*>(pbv + h * dh + d0) : z4;
    const f32x4 bv1 = BAND ? *reinterpret_cast<const f32x4*>(pbv + h * dh + d0 + 4) : z4;
    float qu[8], qv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float q = __uint_as_float((wv[e >> 1] >> (16 * (e & 1))) << 16);
      const float bu = e < 4 ? bu0[e & 3] : bu1[e & 3], bv = e < 4 ? bv0[e & 3] : bv1[e & 3];
      qu[e] = my_i < Tn ? (q + bu) * qscale : 0.f;
      qv[e] = my_i < Tn ? (q + bv) * qscale : 0.f;
    }
    fqu[s] = MT<bf16_t>::from8(qu);
    fqv[s] = MT<bf16_t>::from8(qv);
  }

  float m_run = -INFINITY, l_run = 0.f;
  f32x4 acc_o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc_o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // This wave's G tile t reads window rows pofs + 16t + c16; in the ring that
  // is physical row (row + 64 (ch & 1)) & 127.  A tile lies within one half
  // (pofs is a multiple of 16), so an odd chunk moves it by + or - 64 rows
  // wave-uniformly: tiles t <= w (first segment) up, the others down.  The
  // chunk loop is unrolled by two and each copy reads through LDS addresses
  // formed here, once: even chunks pa0[s] + 2048 t; odd chunks pa0[s] + 8192
  // for tile 0 (always up), pa0[s] + 0 for tile 4 (always down) and the
  // selected pa1[s][t - 1] for tiles 1..3.  swz_kp takes bits 1..3 of the row,
  // i.e. of c16, in either half.  (Left as expressions of the row, the
  // compiler re-added the odd chunk's ten addresses inside the loop.)
  const int pofs = 48 - 16 * w;
  uint32_t pa0[2] = {0u, 0u}, pa1[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
  if constexpr (BAND)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      pa0[s] = lds_lane_addr(Ps + (pofs + c16) * RB + (((4 * s + g) ^ swz_kp(c16)) << 3));
#pragma unroll
      for (int t = 1; t < 4; ++t) {
        pa1[s][t - 1] = pa0[s] + 2 * RB * (16 * t + (t <= w ? PSEG : -PSEG));
        asm volatile("" : "+v"(pa1[s][t - 1]));  // kept in a register, not re-derived per chunk
      }
      asm volatile("" : "+v"(pa0[s]));
    }
  auto band_frag = [&](int par, int s, int t) {  // par, s, t: constants once unrolled
    const bool odd = par != 0;
    const uint32_t a = !odd ? pa0[s] + 2 * RB * 16 * t
                            : t == 0 ? pa0[s] + 2 * RB * PSEG : t == 4 ? pa0[s] : pa1[s][t - 1];
    return *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(a);
  };
  // BAND: two chunks per trip, so that par = ch & 1 is a constant in each copy
  // BAND: two chunks per trip, so that par = ch & 1 is a constant in each copy
  for (int ch = 0; ch < nchunk;)
#pragma unroll
  for (int par = 0; par < (BAND ? 2 : 1) && ch < nchunk; ++par, ++ch) {
    const int j0 = ch * KC;
    const bool more = ch + 1 < nchunk;
    dma_barrier();  // A
    ATT_TL(1 + 5 * ch);
    if (ch == 0) {
      const unsigned long long m = Mb[0] | Mb[1] | Mb[2] | Mb[3];
      mlo = __builtin_amdgcn_readfirstlane((uint32_t)m);
      mhi = __builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
    }
    __builtin_amdgcn_sched_barrier(0);
    dma_v(j0);

    // S^T = K·Qu^T (4 tiles), G^T = P_band·Qv^T (5 tiles)
    f32x4 acc_s[4], acc_g[5];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc_s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 5; ++t) acc_g[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 fk[4], fpb[5];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = 16 * t + c16;
        fk[t] = *reinterpret_cast<const bf16x8*>(Ks + row * RB + (((4 * s + g) ^ swz_kp(row)) << 3));
      }
      if constexpr (BAND)
#pragma unroll
        for (int t = 0; t < 5; ++t) fpb[t] = band_frag(par, s, t);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc_s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk[t], fqu[s], acc_s[t], 0, 0, 0);
      if constexpr (BAND)
#pragma unroll
        for (int t = 0; t < 5; ++t) acc_g[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fpb[t], fqv[s], acc_g[t], 0, 0, 0);
    }
    // rel_shift on the write: row R = 16t + 4g + r -> position R - (15 - c16)
    if constexpr (BAND)
#pragma unroll
      for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int p = 16 * t + 4 * g + r + c16 - 15;
          if (t == 0) p = max(p, -1);
          if (t == 4) p = min(p, KC);
          gq[p] = acc_g[t][r];
        }
    ATT_TL(2 + 5 * ch);
    dma_barrier();  // B
    ATT_TL(3 + 5 * ch);

    // scores for this lane's query, keys jj = 16t + 4g + r (log2 domain)
    f32x4 gv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      gv[t] = BAND ? *reinterpret_cast<const f32x4*>(gq + 16 * t + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
    const bool chunk_padded = ((ch < 32 ? mlo >> ch : mhi >> (ch - 32)) & 1u) != 0u;
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
      dma_k(j0 + KC);
      if constexpr (BAND) dma_p(ch + 2, par);  // over segment ch: every wave read it before B
    }
    float p[4][4];
    float cmax = -INFINITY;
    // S + G as packed fp32 pairs (v_pk_add_f32: half the instructions of the
    // per-element adds; the chunk loop is VALU-issue bound)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const v2f sg = BAND ? v2f{acc_s[t][r], acc_s[t][r + 1]} + v2f{gv[t][r], gv[t][r + 1]}
                            : v2f{acc_s[t][r], acc_s[t][r + 1]};
        p[t][r] = sg[0];
        p[t][r + 1] = sg[1];
      }
    if (chunk_padded) {  // uniform branch, only in chunks holding a padded key
      const uint8_t* kb = kpm + (long long)b * Tn;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kb[min(j0 + 16 * t + 4 * g + r, Tn - 1)]) p[t][r] = -INFINITY;
    }
    if (j0 + KC > Tn) {  // last chunk: keys past Tn (their staged rows are clamped copies)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j0 + 16 * t + 4 * g + r >= Tn) p[t][r] = -INFINITY;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) cmax = fmaxf(cmax, p[t][r]);
    cmax = col4_max(cmax);
    const float m_new = fmaxf(m_run, cmax);
    const float mref = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - mref);
    // p - m as packed pairs; the row sum as a tree of packed pairs (one
    // serial chain of 16 dependent adds before)
    v2f ls2[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v2f e[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const v2f d = v2f{p[t][2 * h2], p[t][2 * h2 + 1]} - v2f{mref, mref};
        e[h2] = v2f{__builtin_amdgcn_exp2f(d[0]), __builtin_amdgcn_exp2f(d[1])};
        p[t][2 * h2] = e[h2][0];
        p[t][2 * h2 + 1] = e[h2][1];
      }
      ls2[t] = e[0] + e[1];
    }
    const v2f lsv = (ls2[0] + ls2[1]) + (ls2[2] + ls2[3]);
    l_run = l_run * alpha + col4_sum(lsv[0] + lsv[1]);
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc_o[t] *= alpha;
    ATT_TL(4 + 5 * ch);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float pv[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pv[r] = p[2 * s2][r];
        pv[4 + r] = p[2 * s2 + 1][r];
      }
      const bf16x8 fp = MT<bf16_t>::from8(pv);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc_o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr(Vs, RB, 32 * s2, 16 * t, lane, swz_v), fp, acc_o[t], 0, 0, 0);
    }
    ATT_TL(5 + 5 * ch);
  }
  if (my_i < Tn) {
    const float inv = 1.0f / l_run;
    bf16_t* orow = out + ((long long)b * Tn + my_i) * o.d_model + h * dh;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint2 pk2;
      pk2.x = pack_bf16x2(acc_o[t][0] * inv, acc_o[t][1] * inv);
      pk2.y = pack_bf16x2(acc_o[t][2] * inv, acc_o[t][3] * inv);
      *reinterpret_cast<uint2*>(orow + 16 * t + 4 * g) = pk2;
    }
  }
  ATT_TL(62);
  SBK_PROBE(__syncthreads(); if (tid == 0 && orig < 4096) {
    g_att_wg[orig][1] = __builtin_amdgcn_s_memrealtime();
    g_att_wg[orig][3] = __builtin_amdgcn_s_memtime();
  })
}

bool aligned16(const void* a, const void* b, const void* c) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) % 16) == 0;
}

int launch_dma(const void* qkv, const void* pk, int ldp, const float* pbu, const float* pbv, const uint8_t* kpm, int B,
               int Tn, int H, float scale, void* out, hipStream_t s) {
  const int grid = B * H * ((Tn + QB - 1) / QB);
  const auto kern = pk ? relpos_flash_dma_kernel<true> : relpos_flash_dma_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(qkv),
                     reinterpret_cast<const bf16_t*>(pk), ldp, pbu, pbv, kpm, Tn, H, scale,
                     reinterpret_cast<bf16_t*>(out));
  SBK_CHECK_LAUNCH();
  return 0;
}

// The general kernel's instantiation for a dtype and head dim: f gets an
// Inst<T, DHP> tag.
template <typename T_, int DHP_>
struct Inst {
  using T = T_;
  static constexpr int DHP = DHP_;
};
template <typename F>
auto with_inst(int dtype_bf16, int dh, F f) {
  if (dtype_bf16) return dh <= 64 ? f(Inst<bf16_t, 64>{}) : f(Inst<bf16_t, 128>{});
  return dh <= 64 ? f(Inst<float, 64>{}) : f(Inst<float, 128>{});
}

int launch(int dtype_bf16, const void* qkv, const void* pk, int ldp, const float* pbu, const float* pbv,
           const uint8_t* kpm, int B, int Tn, int H, int dh, float scale, void* out, float* probs, hipStream_t s,
           const float* am = nullptr, long long am_sb = 0, long long am_sh = 0) {
  return with_inst(dtype_bf16, dh, [&](auto inst) {
    using T = typename decltype(inst)::T;
    constexpr int DHP = decltype(inst)::DHP;
    constexpr size_t lds = FlashLds<T, DHP>::bytes;
    static_assert(lds <= 160 * 1024, "LDS budget");
    const int grid = B * H * ((Tn + QB - 1) / QB);
    const int VEC = MT<T>::VEC;
    const int vec_ok = (dh % VEC == 0) && ((H * dh) % VEC == 0) && (ldp % VEC == 0) && aligned16(qkv, pk, out);
    const auto kern = probs ? relpos_flash_kernel<T, DHP, true> : relpos_flash_kernel<T, DHP, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, reinterpret_cast<const T*>(qkv),
                       reinterpret_cast<const T*>(pk), pbu, pbv, kpm, Tn, H, dh, scale, reinterpret_cast<T*>(out), probs,
                       vec_ok, ldp, am, am_sb, am_sh);
    SBK_CHECK_LAUNCH();
    return 0;
  });
}

}  // namespace

// qkv: (B, T, 3*d) head-interleaved in_proj output [h][q|k|v][dh];
// pk: (2T-1, d) linear_pos output; pbu/pbv: (H*dh) fp32; kpm: (B, T) uint8 or null;
// out: (B, T, d); probs: (B, H, T, T) fp32 or null.
SBK_API int sbk_relpos_attention_ld(int dtype_bf16, const void* qkv, const void* pk, int ldp, const float* pbu,
                                    const float* pbv, const uint8_t* kpm, int B, int Tn, int H, int dh, float scale,
                                    void* out, float* probs, void* stream) {
  if (B <= 0 || Tn <= 0 || H <= 0 || dh <= 0 || dh > 128 || ldp < H * dh || !pk) return SBK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  // the encoder's inference path: bf16, dh = 64, no probabilities
  if (dtype_bf16 && dh == 64 && !probs && ldp % 8 == 0 && Tn <= 64 * 64 && aligned16(qkv, pk, out))
    return launch_dma(qkv, pk, ldp, pbu, pbv, kpm, B, Tn, H, scale, out, s);
  return launch(dtype_bf16, qkv, pk, ldp, pbu, pbv, kpm, B, Tn, H, dh, scale, out, probs, s);
}

// Plain scaled dot-product attention over the same head-interleaved qkv
// (no positional band, no biases): the band-free LDS-DMA kernel; bf16,
// dh = 64, T <= 4096, 16-B aligned operands (else SBK_ERR_ARG: the caller
// takes sbk_relpos_attention_ld with a zero band).
SBK_API int sbk_mha_attention(const void* qkv, const uint8_t* kpm, int B, int Tn, int H, int dh, float scale, void* out,
                              void* stream) {
  if (B <= 0 || Tn <= 0 || H <= 0 || dh != 64 || Tn > 64 * 64 || !aligned16(qkv, nullptr, out)) return SBK_ERR_ARG;
  return launch_dma(qkv, nullptr, 0, nullptr, nullptr, kpm, B, Tn, H, scale, out, (hipStream_t)stream);
}

SBK_API int sbk_relpos_attention(int dtype_bf16, const void* qkv, const void* pk, const float* pbu, const float* pbv,
                                 const uint8_t* kpm, int B, int Tn, int H, int dh, float scale, void* out, float* probs,
                                 void* stream) {
  return sbk_relpos_attention_ld(dtype_bf16, qkv, pk, H * dh, pbu, pbv, kpm, B, Tn, H, dh, scale, out, probs, stream);
}

// sbk_relpos_attention_ld with an additive attention mask am (fp32): score
// (b, h, i, j) += am[b * am_sb + h * am_sh + i * T + j] after the 1/sqrt(d)
// scale, before the key-padding mask and the softmax (attention.py:598-611;
// a bool mask is passed as 0 / -inf).  A 2-D (T, T) mask has am_sb = am_sh
// = 0, a 3-D (B*H, T, T) one am_sb = H*T*T, am_sh = T*T.  General kernel.
SBK_API int sbk_relpos_attention_mask(int dtype_bf16, const void* qkv, const void* pk, int ldp, const float* pbu,
                                      const float* pbv, const uint8_t* kpm, const float* am, long long am_sb,
                                      long long am_sh, int B, int Tn, int H, int dh, float scale, void* out,
                                      float* probs, void* stream) {
  if (B <= 0 || Tn <= 0 || H <= 0 || dh <= 0 || dh > 128 || ldp < H * dh || !pk || !am || am_sb < 0 ||
      am_sh < 0)
    return SBK_ERR_ARG;
  return launch(dtype_bf16, qkv, pk, ldp, pbu, pbv, kpm, B, Tn, H, dh, scale, out, probs, (hipStream_t)stream, am, am_sb,
                am_sh);
}

SBK_PROBE_EXPORT(sbk_probe_att_tl, g_att_tl)
SBK_PROBE_EXPORT(sbk_probe_att_wg, g_att_wg)

SBK_API long long sbk_relpos_attention_lds(int dtype_bf16, int Tn, int dh) {
  (void)Tn;
  return with_inst(dtype_bf16, dh, [](auto inst) {
    return (long long)FlashLds<typename decltype(inst)::T, decltype(inst)::DHP>::bytes;
  });
}
