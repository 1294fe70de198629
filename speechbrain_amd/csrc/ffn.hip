// Fused Conformer feed-forward block (bf16 MFMA):
//
//   z   = x + alpha * ( act( LN0(x) · W1^T + b1 ) · W2^T + b2 )
//   out = LNp(z)            (optional post-LayerNorm, e.g. norm2)
//   u   = LNn(out)          (optional, bf16/fp32 input of the next consumer)
//
// Reference: speechbrain/lobes/models/transformer/Conformer.py:239-260
// (macaron FFNs: ffn_module = Sequential(LayerNorm, PositionalwiseFeedForward,
// Dropout), 0.5-scaled residuals, norm2 after the second FFN) and
// speechbrain/nnet/attention.py:823-839 (PositionalwiseFeedForward).
//
// Optional projection tail (sbk_ffn_proj): y = u · Wp^T in bf16 — the
// MHSA in_proj of the next block (attention.py:549-553, RelPosMHAXL has no
// in_proj bias) — so u never leaves the CU and the QKV GEMM is no launch of
// its own.
//
// Design (MI355X): one workgroup (8 waves) owns BM = 48 rows for
// the whole block, so neither LN0(x) nor the (BM x H) hidden activation ever
// leaves the CU:
//   prologue : x rows (fp32) -> LayerNorm -> bf16 Xn; its MFMA fragments are
//              then held in VGPRs (96 per lane) for every phase-1 step; b1 -> LDS;
//   per chunk of HC = 256 hidden units (8 K-steps of 64):
//     phase 1: Hc^T = W1[c]·Xn^T  -> +b1, act -> bf16 Hs (LDS);
//     phase 2: acc2^T += W2[:, c]·Hs^T  (accumulators stay in VGPRs);
//   epilogue : +b2, alpha, residual, optional post-LN and next-LN over the
//              full rows (cross-wave reduction through LDS), float4 stores;
//   tail     : (projection) u -> Xn (LDS), its fragments read in each of the
//              K1 steps per 256 output columns of Wp through the same ring;
//              bf16 stores of 16 B, interleaved into the next block's steps.
// Weight tiles (256 rows x 64 k = 32 KB) stream L2 -> LDS by LDS-DMA
// (global_load_lds_dwordx4: full 128-B lines, no VGPRs) into a 2-slot ring,
// one tile in flight behind the one being read (counted vmcnt; the last FFN
// steps already fetch the projection's first tiles).  Each wave stages only
// the weight rows it multiplies, so the ring steps need no workgroup barrier.
// The ring image is lane-linear; bank conflicts are removed by XOR-swizzling
// the 16-B chunk index with (row >> 1) & 7 on the global source address and
// on the fragment reads.  HBM traffic per row: D fp32 in + D fp32 out (+ D u
// out, or np bf16 projection outputs).
//
// Measured (M = 12032, H = 1024, s_memtime timeline of one workgroup of 251):
// prologue 10.6k cycles (x rows from HBM in lockstep with every other CU,
// then tile 0), 32 K-steps of ~650-700 cycles (12 MFMAs = 192 issue cycles
// per wave, 2 waves per SIMD; ~110 GB/s of weights into the CU, the DMA
// wait < 80 cycles), +1,400 on each chunk's activation step (Swish on 24
// values per lane: VALU), epilogue 8.3k (18 MB of out/u stores from every CU
// at once: HBM).  H = 2048 adds 0.5 us per K-step, so ~14 us of the 29.6 us
// launch is the fixed prologue/epilogue/launch cost, not the weight stream.
// Tried and slower or equal: 8-wave register-staged ring (48 us), 4 waves
// (69 us), fragment-shaped loads straight to VGPRs (64 us), row-owner waves
// with the hidden chunk in registers (78 us), a shared 3-slot ring with a
// barrier per K-step (42 us), LN'd rows re-read from LDS each step instead
// of VGPRs (36.7 us), a per-XCD rotated chunk order (35.0 us), a 3-slot ring
// with one hidden buffer (37.2 us), a third slot aliased onto Xn after the
// VGPR load (30.3 us), a tile-contiguous weight image (29.3 us).
// Round 2 (layer chain, 58 us): a single-pass row LayerNorm (sum and sum of
// squares in one LDS exchange, affine prefetched) was no faster (58.4 us).
// Round 3: no s_waitcnt vmcnt(0) left outside the last step.  The compiler
// guards a visible LDS access or the first use of a visible global load
// with vmcnt(0) (it does not count LDS-DMA in order), and __syncthreads()
// waits for vmcnt(0): each drained the two weight tiles in flight (and, in
// the tail, the stores).  Hence asm LDS accesses, asm prologue loads with
// one counted wait, LDS-only barriers, the epilogue vectors copied to LDS in
// the prologue, lane offsets recomputed instead of hoisted (spills 13 -> 4),
// and the out / projection stores interleaved into the projection steps
// with counted waits.  s_memtime timeline: 129.5k -> 128.5k cycles, the
// steps unchanged at ~1,030 cycles: a step issues 32 KB of LDS-DMA per CU,
// ~40 B/clk, the per-CU LDS-DMA issue rate (MI355X_MICROARCH ldsdma-fill:
// 16 KiB per 0.154 us), while its 12 MFMAs per wave fill 384 of them.
// Fewer weight bytes per CU need more rows per CU than M / 256 = 47.
// Round 7: conv_chain_kernel runs the convolution module of layer i
// (convstage.h: conv_module_kernel<true>'s phases on this kernel's 8-wave
// thread map) as the prologue of the layer chain, on one 48-frame tile of
// one utterance; the module's output lands in the chain's residual layout
// and never leaves the CU.  69.9 us per launch against 48.6 (chain) + 28.3
// (conv module), 85.7 MB of HBM traffic against 110.2.
// Round 8: the two ends of the stack.  conv_tail_kernel is the CONV prologue
// in front of one block with post-LN and next-LN and no `out` (the last
// layer: 47.0 us against 28.5 + 26.6).  src_ffn_kernel adds a second
// prologue kind, SRC: the rows are A Ws^T + bs (the Linear in front of the
// stack), its 48 A rows staged in the LDS that is free until LN0 writes Xn,
// Ws streamed through the ring from its own image, the accumulators the
// residual layout; it also stores its rows' key-padding bytes (37.6 us
// against 32.9 + ~12 + 5.0).
// Round 9: the phases that are not GEMM run with the MFMA pipe and the weight
// stream idle on every CU at once, so their VALU issue is on the critical
// path.  row_ln, the epilogues and the conv stage take v_rsq_f32 instead of
// the IEEE 1 / sqrt expansion and packed fp32 pairs (v2f) where the values
// sit in adjacent registers; the rounding points are where they were.
// conv_chain_kernel<1>: 4,444 -> 3,721 static VALU instructions per wave,
// 161.7k -> 155.4k cycles, 76.3 -> 73.6 us.
// Round 10: the projection tail (the in_proj of the next layer, 11 % of the
// chain launch).  Its y rows went out as two 8-B stores per lane and row
// (units 4g.. of the wave's two 16-column tiles, 32 B apart): 18 store
// instructions per wave and column block, and the waves that finish last
// queued behind their issue.  One v_permlane16_swap pair per row exchanges
// tiles between lane rows, so a lane holds 8 consecutive columns and stores
// 16 B: 9 instructions, same bytes, same values.  Timeline of workgroup 128:
// tail 17.5k -> 14.0k cycles, launch 157.6k -> 152.7k; conv_chain_kernel<1>
// 73.9 -> 72.4 us.  Holding u's fragments in VGPRs for the 12 steps (as phase
// 1 does) was measured on top and alone: no gain either way (DESIGN section
// 3, round 10).
// Round 11: the start of the conv stage (convstage.h, phase -1: 22.6k of the
// chain launch's 152.7k cycles before the first useful MFMA result).  Two
// loads under a branch (the LN0 affine, the out_proj bias) each drew an
// s_waitcnt vmcnt(0) into the middle of the launch-start burst, the second
// in front of half of wo; and a wave reached the first barrier, which needs
// o only, after issuing all 31 of its loads into a queue that stalls when
// full.  Now: unconditional loads, o first across the workgroup (a bare
// s_barrier), wo of four K-steps ahead, the rest of wo and x issued behind
// the MFMAs under the compiler's counted waits.  The stretch ends at 18.1k
// cycles instead of 25.0k in the probe build, the same bits;
// conv_chain_kernel<1> and the step: DESIGN section 3, round 11.
// Round 12: the bytes of that burst.  (1) The conv-stage launches take their
// tile from sbk::xcd_tile(gridDim.x, blockIdx.x) instead of blockIdx.x.  At
// T = 376 an utterance has 8 tiles and workgroups are dealt round-robin to
// the 8 XCDs, so two neighbouring tiles never shared an L2 and each fetched
// the 30 halo rows of x and o between them from beyond it; now the blocks of
// one blockIdx.x % 8 own whole utterances.  FETCH_SIZE x 2 per chain launch
// 54.8 -> 43.8 MB (the halo), conv_tail_kernel 43.1 -> 32.0 MB.  (2) wo goes
// through a 2-slot ring from an image of its own (sbk_wo_image, cached per
// weight like the other images; the `wo` argument of sbk_conv_ffn_chain /
// sbk_conv_ffn_tail is that image) by LDS-DMA, as phases 1 and 3, instead
// of as fragments into 64 staging VGPRs; every load of phase -1 is asm with
// a counted wait (convstage.h).  Same MFMA sequence per accumulator, the same
// bits.  Step, alternating same-box A/B (ms): parent 1.0814, (1) alone
// 1.0728, (2) alone 1.0710, both 1.0614.
#include "mfma.h"

using namespace sbk;

namespace {

enum Act { ACT_NONE = 0, ACT_SWISH = 1, ACT_GLU = 2, ACT_LRELU = 3, ACT_GELU = 4 };

struct FfnArgs {
  const float* x;  // (M, D) fp32
  int M, H;
  const float *g0, *b0;
  float eps0;
  // the launch's weight stream: ST tiles of 256 rows x 64 k (32 KB) in
  // stream order, each row's 16-B chunks pre-swizzled (sbk_ffn_image), so a
  // wave's share of a tile is one contiguous 4 KB run
  const bf16_t* img;
  const float* b1;
  int act;
  float slope;
  const float* b2;
  float alpha;
  const float *gp, *bp;  // post-LN (or null)
  float epsp;
  float* out;  // (M, D) fp32, may alias x
  const float *gn, *bn;  // next-LN (or null)
  float epsn;
  void* u;
  int u_bf16;
  int np;      // projection of next-LN(out): np output columns (0: none)
  bf16_t* yp;  // (M, np) bf16
  // CHAIN: a second FFN block on the first one's output, which stays on chip
  // (the first block's `out` is not written): FFN2 + norm2 of layer i, then
  // FFN1 of layer i+1 with its own LN0, alpha, w1/b1/w2/b2; its result goes
  // to `out`, next-LN and the projection tail as for a single block
  const float *g0b, *b0b;  // null: one block
  float eps0b;
  const float *b1b, *b2b;
  float alphab;
  // LayerNorm statistics over the first d_eff of the D columns (the others
  // are zero-padded channels: D = 256 carrying a d_model < 256 model whose
  // LN gains / biases and weight rows are zero there): inv_n = 1 / d_eff,
  // npad = D - d_eff (each padded zero adds mean^2 to the centred sum)
  float inv_n, npad;
  // SRC: the rows come from a Linear in front of the block, x = sa . Ws^T + sbias
  // (sa (M, Kin) bf16; simg: sbk_src_image(Ws), Kin / 64 tiles of Ws (256, Kin);
  // sbias fp32 or null), and the workgroup stores the key-padding bytes of its
  // rows, kpm_out[m] = length_mask_byte(rel_len[m / Tm], m % Tm, Tm) (rel_len null: none)
  const bf16_t *sa, *simg;
  const float* sbias;
  int Kin, Tm;
  const float* rel_len;
  uint8_t* kpm_out;
};

__device__ __forceinline__ bf16x8 ld8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

template <int V>
struct IntC {
  static constexpr int value = V;
};

constexpr int FFN_BM = 48;
// the conv-stage launches take their tiles in the XCD-contiguous order (a probe build may switch it off)
#ifndef FFN_XCD_ORDER
#define FFN_XCD_ORDER 1
#endif
constexpr int FFN_PAD = 16;  // LDS row pad (elements): conflict-free b128 reads (8 measured slower)
constexpr int FFN_NW = 8, FFN_NT = FFN_NW * 64;  // 8 waves: LN'd rows fit in VGPRs (2 waves/SIMD)
// Xn / Hs rows: element (row, col) at row * stride + (col ^ ffn_sw(row)), the
// 16-B chunks of rows with bit 2 set swapped in pairs.  The 8-B column stores
// (16 rows fr of one column per ds_write_b64 lane group: MI355X_MICROARCH
// §LDS) were 4-way conflicted at the 544-B pitch — rows fr, fr + 4, fr + 8,
// fr + 12 on one bank pair — and are 2-way with it, the floor for 16-B-aligned
// rows; the b128 fragment reads stay conflict-free.  Counted: 720 of the 942
// conflict cycles per wave (SQ_LDS_BANK_CONFLICT, profiles/r04t_chain_sq_counters.txt).
__device__ __forceinline__ constexpr int ffn_sw(int row) { return ((row >> 2) & 1) << 3; }
static_assert(FFN_NW % 8 == 0, "rows w + FFN_NW * i share bit 2 with w (their swizzle is ffn_sw(w))");
// row-reduction scratch stride (floats): 16-B-aligned rows whose partial
// stores (16 lanes, rows fr) are 2-way and whose b128 reads are conflict-free
// (a stride of NW = 8 made them 4-way and 2-way: 66 conflict cycles per LayerNorm)
constexpr int FFN_RS = 12;

typedef float v2f __attribute__((ext_vector_type(2)));  // fp32 pairs: v_pk_add / v_pk_mul / v_pk_fma

#define FFN_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_bf16((A), (B), (C), 0, 0, 0)

template <int ACT>
__device__ __forceinline__ float act_fn(float v, float slope) {
  if (ACT == ACT_SWISH) return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));  // bf16 hidden: approx rcp
  if (ACT == ACT_LRELU) return v >= 0.f ? v : v * slope;
  if (ACT == ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
  return v;
}

// LDS read the compiler cannot see (it would guard a visible one with
// s_waitcnt vmcnt(0) against the in-flight LDS-DMA tiles, draining stores too)
__device__ __forceinline__ f32x4 lds_f4(const float* p) {
  f32x4 v;
  const uint32_t la = (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) float*)p);
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(la) : "memory");
  return v;
}

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) char*)p);
}
__device__ __forceinline__ float lds_f1(const float* p) {
  float v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(lds_addr(p)) : "memory");
  return v;
}
__device__ __forceinline__ void lds_st1(float* p, float v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_st4(float* p, f32x4 v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_st2(void* p, uint2 v) {
  const unsigned long long u = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
  asm volatile("ds_write_b64 %0, %1" ::"v"(lds_addr(p)), "v"(u) : "memory");
}
// s_waitcnt lgkmcnt(0) that a value read by the asm LDS loads above depends
// on: its uses cannot be scheduled before the wait (the first tie waits, the
// others retire at once)
template <typename V>
__device__ __forceinline__ void tie(V& v) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v));
}
// workgroup barrier on LDS traffic only: __syncthreads() also waits for
// vmcnt(0), i.e. for every LDS-DMA tile and store in flight
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// global load the compiler cannot see: it would follow a visible one's first
// use with s_waitcnt vmcnt(0) (it does not count LDS-DMA in order), draining
// the weight tiles issued after it.  The caller waits (asm) and then vtie()s.
__device__ __forceinline__ f32x4 gld4(const float* p) {
  f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void vtie(f32x4& v) { asm volatile("" : "+v"(v)); }

// s_waitcnt vmcnt(n) for a wave-uniform n known only at run time
__device__ __forceinline__ void vm_wait(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
  }
}

// Full-row LayerNorm of the epilogue values z (in place).  Lane (w, g, fr)
// holds rows mt*16 + fr, units (w*T2 + j)*16 + 4g + e; row statistics are
// reduced over g by shuffles and over the NW waves through red[BM][FFN_RS]; gam /
// bet are LDS copies.  Every LDS access is explicit (asm) and the barriers
// wait on LDS only, so the weight tiles and stores in flight stay in flight.
// (One barrier per pass with a buffer per pass measured 1.5 us slower per
// chain launch than two barriers over one buffer.)
template <int D, int T2, int MT, int NW>
__device__ __forceinline__ void row_ln(float (&z)[T2][MT][4], float* red, const float* gam, const float* bet, float eps,
                                       int w, int g, int fr, float inv_n, float npad) {
  static_assert(NW == 8, "two b128 reads per row");
  float mean[MT], rstd[MT];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    float part[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      // (packed pair sums here cost the GELU chain instance 4 more bytes of scratch)
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < T2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dv = pass ? z[j][mt][e] - mean[mt] : z[j][mt][e];
          s += pass ? dv * dv : dv;
        }
      part[mt] = col4_sum(s);
    }
    lds_barrier();  // the previous readers of red are done
    if (g == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) lds_st1(red + (mt * 16 + fr) * FFN_RS + w, part[mt]);
    }
    lds_barrier();
    f32x4 rv[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      rv[mt][0] = lds_f4(red + (mt * 16 + fr) * FFN_RS);
      rv[mt][1] = lds_f4(red + (mt * 16 + fr) * FFN_RS + 4);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      tie(rv[mt][0]);
      tie(rv[mt][1]);
      const float t = (rv[mt][0][0] + rv[mt][0][1]) + (rv[mt][0][2] + rv[mt][0][3]) + (rv[mt][1][0] + rv[mt][1][1]) +
                      (rv[mt][1][2] + rv[mt][1][3]);
      if (pass)  // v_rsq_f32 (1 ulp) on a value >= eps, instead of the IEEE sqrt and divide expansions
        rstd[mt] = __builtin_amdgcn_rsqf((t - npad * mean[mt] * mean[mt]) * inv_n + eps);
      else
        mean[mt] = t * inv_n;
    }
  }
  f32x4 gv[T2], bv[T2];
#pragma unroll
  for (int j = 0; j < T2; ++j) {
    const int d = (w * T2 + j) * 16 + 4 * g;
    gv[j] = lds_f4(gam + d);
    bv[j] = lds_f4(bet + d);
  }
#pragma unroll
  for (int j = 0; j < T2; ++j) {
    tie(gv[j]);
    tie(bv[j]);
#pragma unroll
    for (int e = 0; e < 4; e += 2)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const v2f y = (v2f{z[j][mt][e], z[j][mt][e + 1]} - v2f{mean[mt], mean[mt]}) * v2f{rstd[mt], rstd[mt]} *
                          v2f{gv[j][e], gv[j][e + 1]} + v2f{bv[j][e], bv[j][e + 1]};
        z[j][mt][e] = y[0];
        z[j][mt][e + 1] = y[1];
      }
  }
}

// The projection's bf16 results of one row, paired for a 16-B store.  A lane
// (g, fr) holds units 4g .. 4g+3 of the wave's tile 0 (v0) and of tile 1 (v1),
// 32 B apart.  v_permlane16_swap exchanges tile 1 of the even lane rows
// (g = 0, 2) with tile 0 of the odd ones, row fr by row fr: afterwards the
// lane holds units 8 (g >> 1) .. +7 of tile g & 1, i.e. the 8 consecutive
// columns 16 (g & 1) + 8 (g >> 1) .. of the wave's 32.  (The same pairing by
// a row permutation of the image's projection tiles would change the image.)
__device__ __forceinline__ uint4 proj_pair(const f32x4& v0, const f32x4& v1) {
  const uint32_t a0 = pack_bf16x2(v0[0], v0[1]), a1 = pack_bf16x2(v0[2], v0[3]);
  const uint32_t b0 = pack_bf16x2(v1[0], v1[1]), b1 = pack_bf16x2(v1[2], v1[3]);
  const auto lo = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
  return make_uint4(lo[0], hi[0], lo[1], hi[1]);
}

// A-operand fragments of the LayerNorm'd rows (Xn, bf16, row stride XS)
// into VGPRs for every K-step of a block
template <int K1, int KS, int MT, int XS, int BK>
__device__ __forceinline__ void load_frags(bf16x8 (&xa)[K1][KS][MT], const bf16_t* Xn, int fr, int fk) {
#pragma unroll
  for (int r = 0; r < K1; ++r)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        asm volatile("ds_read_b128 %0, %1"
                     : "=v"(xa[r][ks][mt])
                     : "v"(lds_addr(Xn + (mt * 16 + fr) * XS + r * BK + ks * 32 + fk))
                     : "memory");
#pragma unroll
  for (int r = 0; r < K1; ++r)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) tie(xa[r][ks][mt]);
}

// s_memtime timeline of the waves of workgroup 128 (rows 0 .. 7) and of
// workgroup 127 (rows 8 .. 15: at T = 376 a last tile of 40 live rows, the
// projection tail's !full path); probe builds only; the conv stage's marks
// are entries 210.. of each wave's row
SBK_PROBE_BUFFER(g_ffn_tl, 16, 256)
#define FFN_TL(i) SBK_PROBE(if (tl_rec >= 0 && lane == 0) g_ffn_tl[tl_rec][i] = __builtin_amdgcn_s_memtime();)

#include "convstage.h"

// The body of ffn_kernel and conv_chain_kernel.  CONV: the workgroup's rows
// are one 48-frame tile of one utterance and come out of the convolution
// module (conv_stage) in registers instead of from a.x.  SRC: they come out of
// the source Linear (a.sa . Ws^T + a.sbias) in registers.
template <int D, int ACT, bool PROJ, bool CHAIN, bool CONV, bool SRC = false>
__device__ __forceinline__ void ffn_body(const FfnArgs& a, const ConvStageArgs* cs) {
  static_assert(!(CONV && SRC), "one kind of prologue");
  constexpr int BM = FFN_BM, HC = 256, NW = FFN_NW, NT = FFN_NT;
  constexpr int XS = D + FFN_PAD, HS = HC + FFN_PAD;   // LDS row strides (elements), +32 B pad: conflict-free b128 reads
  constexpr int MT = BM / 16;                // m-tiles (3)
  constexpr int T = 256 / 16 / FFN_NW;       // 16-row weight tiles per wave (HC/16/NW = D/16/NW)
  constexpr int BK = 64;                     // K per step: one 128-B line per weight row
  constexpr int K1 = D / BK, K2 = HC / BK, SPC = K1 + K2;
  constexpr int NB = 2;                      // ring slots: a slot is refilled as soon as its fragments are in VGPRs
  constexpr int TROWS = 256;                 // rows per weight tile (HC for W1, D for W2, 256 output columns of Wp)
  constexpr int GL = TROWS * BK * 2 / 16 / NT;  // LDS-DMA instructions per thread per tile (4)
  static_assert(GL * 8 == T * 16, "each wave stages exactly the weight rows it multiplies");
  constexpr int PER = D / 64;                // LN: floats per lane (4)
  static_assert(PER == 4 && D == 256 && HC / 16 / NW == T && D / 16 / NW == T, "shape");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* ring = reinterpret_cast<bf16_t*>(smem);          // NB x TROWS x BK (linear 128-B rows)
  bf16_t* Xn = ring + NB * TROWS * BK;                      // BM x XS
  bf16_t* Hs = Xn + BM * XS;                                // 2 x BM x HS
  float* b1s = reinterpret_cast<float*>(Hs + 2 * BM * HS);  // H (CHAIN: 2 H, block A then B)
  float* red = b1s + (CHAIN ? 2 : 1) * a.H;                 // BM x FFN_RS row partials
  // epilogue vectors, copied to LDS in the prologue so that no global load
  // (and its in-order vmcnt wait behind the weight tiles) sits between blocks
  float* prm = red + BM * FFN_RS;                           // P_* x D
  enum { P_B2 = 0, P_GP, P_BP, P_G0B, P_B0B, P_B2B, P_GN, P_BN, P_N };
  static_assert(P_N == NW, "one parameter row per wave");

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, g = lane >> 4, fk = (8 * g) ^ ffn_sw(fr);  // chunk g of the swizzled rows mt*16 + fr
  // rows m0 .. m0 + BM - 1, live below mlim (CONV: the utterance's end, not the flat M)
  // CONV: the tile comes from the XCD-contiguous order, so that the tiles of
  // one utterance, which share their halo rows of x and o, share an L2; the
  // flat-row kernels have no halo and keep the launch order
  const int tile = CONV && FFN_XCD_ORDER ? xcd_tile(gridDim.x, blockIdx.x) : (int)blockIdx.x;
  int m0 = tile * BM, mlim = a.M;
  if constexpr (CONV) {
    const int nblk = (cs->T + BM - 1) / BM, b = tile / nblk;
    m0 = b * cs->T + (tile - b * nblk) * BM;
    mlim = (b + 1) * cs->T;
  }
  const int NCH = a.H / HC;
  const int S = NCH * SPC;                              // K-steps of one FFN block
  const int SF = CHAIN ? 2 * S : S;                     // FFN K-steps (blocks A, B)
  const int SP = PROJ ? (a.np / TROWS) * K1 : 0;        // projection K-steps (image tiles after the FFN ones)
  const int ST = SF + SP;
  SBK_PROBE(const int tl_rec = blockIdx.x == 128 ? w : blockIdx.x == 127 ? NW + w : -1;)
  FFN_TL(0);

  // ---- weight tile s -> ring slot (LDS-DMA, 1 KB = 8 rows per wave-instruction)
  // lane L of instruction i writes row R0 + L/8, 16-B chunk L%8 (linear image)
  // and fetches source chunk (L%8) ^ ((row >> 1) & 7): the read side applies
  // the same involution.  Steps S.. are the projection's (256 columns of Wp
  // by 64 k per tile, column block after column block).
  auto issue = [&](int s, int slot) __attribute__((always_inline)) {
    // tile s of the image: wave w's 4 KB (its 32 rows, lane-linear) by GL
    // pieces of 1 KB from one base address and immediate offsets, which the
    // instruction applies to the global and the LDS address alike (one m0
    // per tile; the per-piece address arithmetic and tile-index logic of a
    // strided source cost ~100 scalar and vector instructions per step)
    const bf16_t* src = a.img + (long long)s * (TROWS * BK) + w * (GL * 512) + lane * 8;
    bf16_t* dst = ring + slot * (TROWS * BK) + w * (GL * 512);
    const auto gs = (const __attribute__((address_space(1))) void*)src;
    const auto ls = (__attribute__((address_space(3))) void*)dst;
    static_assert(GL == 4, "four 1-KB pieces per wave and tile");
    __builtin_amdgcn_global_load_lds(gs, ls, 16, 0, 0);
    __builtin_amdgcn_global_load_lds(gs, ls, 16, 1024, 0);
    __builtin_amdgcn_global_load_lds(gs, ls, 16, 2048, 0);
    __builtin_amdgcn_global_load_lds(gs, ls, 16, 3072, 0);
  };
  // ---- prologue.  Every HBM read of the launch is issued here, before the
  // weight stream: the residual x values of this lane's epilogue outputs
  // (held in VGPRs through the main loop; rows clamped, masked at the end) and
  // the x rows of the LayerNorm, so their latency overlaps the first weight
  // tiles instead of being paid again after the last MFMA.
  constexpr int NRW = (BM + NW - 1) / NW;    // LN rows per wave
  f32x4 xres[T][MT];
  if constexpr (CONV || SRC) {
    // ---- the convolution module in front of block A.  Its LDS ([0, CS_LDS))
    // lies under the ring, Xn and the hidden-chunk buffers; b1, the reduction
    // scratch and the parameter rows are past it and are staged while it
    // runs, and block A's LN0 affine waits in the tail of the second hidden
    // buffer (free until chunk 1's activation step).  SRC: the A rows of the
    // source Linear lie over Xn and the hidden-chunk buffers, below the affine.
    static_assert(T == 2 && MT == CS_MT3, "conv_stage hands over the chain's residual layout");
    constexpr int HS_END = (NB * TROWS * BK + BM * XS + 2 * BM * HS) * 2;  // bytes
    float* ga0 = reinterpret_cast<float*>(smem + (CONV ? CS_LDS : HS_END - 2 * D * 4));  // [g0 | b0] of block A
    static_assert(CS_LDS + 2 * D * 4 <= HS_END, "LN0 affine below b1");
    static_assert(CS_LDS >= (NB * TROWS * BK + BM * XS + BM * HS) * 2, "LN0 affine in the second hidden buffer");
    const float* psrc = w == P_B2 ? a.b2 : w == P_GP ? a.gp : w == P_BP ? a.bp : w == P_G0B ? a.g0b
                      : w == P_B0B ? a.b0b : w == P_B2B ? a.b2b : w == P_GN ? a.gn : a.bn;
    const bool b1t = tid * 4 < a.H;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pv = z4, b1v = z4, b1bv = z4, gav = z4;
    if (psrc) pv = *reinterpret_cast<const float4*>(psrc + lane * PER);
    if (b1t) {
      b1v = *reinterpret_cast<const float4*>(a.b1 + tid * 4);
      if (CHAIN) b1bv = *reinterpret_cast<const float4*>(a.b1b + tid * 4);
    }
    if (tid < D / 2) gav = *reinterpret_cast<const float4*>((tid < D / 4 ? a.g0 : a.b0) + 4 * (tid % (D / 4)));
    auto stage_params = [&]() __attribute__((always_inline)) {
      if (psrc) *reinterpret_cast<float4*>(prm + w * D + lane * PER) = pv;
      if (b1t) {
        *reinterpret_cast<float4*>(b1s + tid * 4) = b1v;
        if (CHAIN) *reinterpret_cast<float4*>(b1s + a.H + tid * 4) = b1bv;
      }
      if (tid < D / 2) *reinterpret_cast<float4*>(ga0 + 4 * tid) = gav;
    };
    if constexpr (CONV) {
      const int nblk = (cs->T + BM - 1) / BM, ub = tile / nblk;
      conv_stage(*cs, a.inv_n, a.npad, smem, ub, (tile - ub * nblk) * BM, xres, stage_params);
    } else {
      // ---- the source Linear: xres = A Ws^T + bs for the workgroup's 48 rows.
      // The A rows (bf16, Kin <= 768) wait in LDS, row stride Kin + FFN_PAD (as
      // Xn: conflict-free b128 fragment reads); Ws streams through the ring as
      // Kin / 64 tiles of its 256 rows x 64 k (a.simg, the image's row
      // swizzle), one tile in flight behind the one being read.  A step is a
      // phase-1 step's wave map — wave w: output columns (2w + t) * 16 .. —
      // so the accumulators are the residual layout.  Rows at or past M are
      // copies of row M - 1 and are never stored.
      bf16_t* As = Xn;
      const int AS = a.Kin + FFN_PAD, KS = a.Kin / BK, cpr = a.Kin / 8;  // row stride, K-steps, 16-B chunks per row
      // wave w: rows w + 8 i, lane: chunks lane and lane + 64 of a row (cpr <= 96)
      constexpr int NRA = BM / NW;
      static_assert(NRA * NW == BM && 768 / 8 <= 2 * 64, "two chunks per lane cover a row");
      bf16x8 av[NRA * 2];
#pragma unroll
      for (int i = 0; i < NRA * 2; ++i) {
        const int ch = min(lane + 64 * (i & 1), cpr - 1);
        av[i] = ld8(a.sa + (long long)min(m0 + w + NW * (i >> 1), mlim - 1) * a.Kin + ch * 8);
      }
      f32x4 sb[T];
#pragma unroll
      for (int j = 0; j < T; ++j) {
        sb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a.sbias) sb[j] = *reinterpret_cast<const f32x4*>(a.sbias + (w * T + j) * 16 + 4 * g);
      }
      // the key-padding bytes of the workgroup's rows
      if (a.rel_len && tid < BM && m0 + tid < mlim) {
        const int m = m0 + tid, ub = m / a.Tm;
        a.kpm_out[m] = length_mask_byte(a.rel_len[ub], m - ub * a.Tm, a.Tm);
      }
#pragma unroll
      for (int i = 0; i < NRA * 2; ++i) {
        const int ch = lane + 64 * (i & 1);
        if (ch < cpr) *reinterpret_cast<bf16x8*>(As + (w + NW * (i >> 1)) * AS + ch * 8) = av[i];
      }
      stage_params();
      __syncthreads();
      auto issue_src = [&](int s, int slot) __attribute__((always_inline)) {
        const bf16_t* src = a.simg + (long long)s * (TROWS * BK) + w * (GL * 512) + lane * 8;
        bf16_t* dst = ring + slot * (TROWS * BK) + w * (GL * 512);
        const auto gs = (const __attribute__((address_space(1))) void*)src;
        const auto ls = (__attribute__((address_space(3))) void*)dst;
        __builtin_amdgcn_global_load_lds(gs, ls, 16, 0, 0);
        __builtin_amdgcn_global_load_lds(gs, ls, 16, 1024, 0);
        __builtin_amdgcn_global_load_lds(gs, ls, 16, 2048, 0);
        __builtin_amdgcn_global_load_lds(gs, ls, 16, 3072, 0);
      };
      issue_src(0, 0);
      issue_src(min(1, KS - 1), 1);
      f32x4 accs[T][MT];
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) accs[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < KS; ++s) {
        // this wave's rows of tile s landed (the tile behind it stays in flight)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL * (NB - 1)) : "memory");
        const bf16_t* tile = ring + (s % NB) * TROWS * BK;
        bf16x8 fw[BK / 32][T], fa[BK / 32][MT];
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const int row = w * (T * 16) + t * 16 + fr;
            fw[ks][t] = ld8(tile + row * BK + (((ks * 4 + g) ^ ((row >> 1) & 7)) << 3));
          }
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) fa[ks][mt] = ld8(As + (mt * 16 + fr) * AS + s * BK + ks * 32 + 8 * g);
        }
        // the slot takes tile s + 2 (at the end a harmless reload of the last tile)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        issue_src(min(s + NB, KS - 1), s % NB);
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks)
#pragma unroll
          for (int t = 0; t < T; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) accs[t][mt] = FFN_MFMA(fw[ks][t], fa[ks][mt], accs[t][mt]);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // retire the tail reloads before the ring is reused
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xres[j][mt] = accs[j][mt] + sb[j];
    }
    // every wave is done with V and the conv ring (SRC: the A rows and the
    // source tiles): block A's first two tiles land under its LN0 (the
    // prologue's output rows are A's residual)
    lds_barrier();
    issue(0, 0);
    issue(1, 1);
    float z[T][MT][4];
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) z[j][mt][e] = xres[j][mt][e];
    row_ln<D, T, MT, NW>(z, red, ga0, ga0 + D, a.eps0, w, g, fr, a.inv_n, a.npad);
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int d = (w * T + j) * 16 + 4 * g;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        uint2 pk;
        pk.x = pack_bf16x2(z[j][mt][0], z[j][mt][1]);
        pk.y = pack_bf16x2(z[j][mt][2], z[j][mt][3]);
        lds_st2(Xn + (mt * 16 + fr) * XS + (d ^ ffn_sw(fr)), pk);
      }
    }
  } else {
#pragma unroll
  for (int j = 0; j < T; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = min(m0 + mt * 16 + fr, mlim - 1);
      xres[j][mt] = gld4(a.x + (long long)row * D + (w * T + j) * 16 + 4 * g);
    }
  f32x4 xv[NRW];
#pragma unroll
  for (int i = 0; i < NRW; ++i) {
    const int rr = w + i * NW, row = min(m0 + rr, mlim - 1);
    xv[i] = gld4(a.x + (long long)row * D + lane * PER);
  }
  f32x4 g04 = gld4(a.g0 + lane * PER), b04 = gld4(a.b0 + lane * PER);
  // wave w loads parameter row w (null rows are never read); lane-quads of b1 / b1b
  const float* psrc = w == P_B2 ? a.b2 : w == P_GP ? a.gp : w == P_BP ? a.bp : w == P_G0B ? a.g0b
                    : w == P_B0B ? a.b0b : w == P_B2B ? a.b2b : w == P_GN ? a.gn : a.bn;
  f32x4 pv = f32x4{0.f, 0.f, 0.f, 0.f}, b1v = pv, b1bv = pv;
  if (psrc) pv = gld4(psrc + lane * PER);
  const bool b1t = tid * 4 < a.H;
  if (b1t) b1v = gld4(a.b1 + tid * 4);
  if (CHAIN && b1t) b1bv = gld4(a.b1b + tid * 4);
  issue(0, 0);
  issue(1, 1);
  // every load above has landed; the two tiles stay in flight
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB * GL) : "memory");
#pragma unroll
  for (int j = 0; j < T; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) vtie(xres[j][mt]);
#pragma unroll
  for (int i = 0; i < NRW; ++i) vtie(xv[i]);
  vtie(g04);
  vtie(b04);
  vtie(pv);
  vtie(b1v);
  vtie(b1bv);

  // LayerNorm of the workgroup's rows -> Xn (bf16); b1 -> LDS
#pragma unroll
  for (int i = 0; i < NRW; ++i) {
    const int rr = w + i * NW;
    if (rr >= BM) break;
    const bool live = m0 + rr < mlim;
    const float v[4] = {live ? xv[i][0] : 0.f, live ? xv[i][1] : 0.f, live ? xv[i][2] : 0.f, live ? xv[i][3] : 0.f};
    const float mean = wave_sum_v(v[0] + v[1] + v[2] + v[3]) * a.inv_n;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) q += (v[e] - mean) * (v[e] - mean);
    const float rstd = __builtin_amdgcn_rsqf((wave_sum_v(q) - a.npad * mean * mean) * a.inv_n + a.eps0);
    uint2 pk;
    pk.x = pack_bf16x2((v[0] - mean) * rstd * g04[0] + b04[0], (v[1] - mean) * rstd * g04[1] + b04[1]);
    pk.y = pack_bf16x2((v[2] - mean) * rstd * g04[2] + b04[2], (v[3] - mean) * rstd * g04[3] + b04[3]);
    lds_st2(Xn + rr * XS + ((lane * PER) ^ ffn_sw(w)), pk);  // rr = w + i * NW, NW % 8 == 0
  }
  static_assert(2048 <= NT * 4, "b1 in one float4 per thread");
  if (psrc) lds_st4(prm + w * D + lane * PER, pv);
  if (b1t) lds_st4(b1s + tid * 4, b1v);
  if (CHAIN && b1t) lds_st4(b1s + a.H + tid * 4, b1bv);
  }  // !CONV

  f32x4 acc1[T][MT], acc2[T][MT];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      acc1[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc2[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  // ---- main loop.  Every wave stages (LDS-DMA) and reads only its own weight
  // rows, so the 2-slot ring needs no workgroup barrier: a slot takes tile
  // s+2 as soon as the wave's fragments of tile s are in VGPRs.  Barriers
  // remain only where waves share data: Xn (before the loop) and the hidden
  // chunk Hs (written at r == K1-1, read from r == K1; double-buffered by
  // chunk parity).  The LayerNorm'd rows are the A operand of every phase-1
  // step: their fragments stay in VGPRs for the whole launch (96 VGPRs).
  // (Tried and slower: fragments of step s+1 read under the MFMAs of step s —
  // 8 waves 40.8 us, 16 waves spill; weights streamed straight into VGPRs
  // with 4 steps in flight instead of LDS-DMA — 45 us at 8 or 16 waves.)
  FFN_TL(1);
  lds_barrier();
  bf16x8 xa[K1][BK / 32][MT];
  load_frags<K1, BK / 32, MT, XS, BK>(xa, Xn, fr, fk);
  // one K-step: tile s landed -> this wave's fragments (phase 1: the held Xn
  // fragments of k-step r; phase 2: the hidden chunk Hc at k-step r) -> the
  // slot takes tile s+NB -> 12 MFMAs into acc1 / acc2
  auto step = [&](int s, int r, bool ph2, const bf16_t* Hc, bool bar, auto&& post) __attribute__((always_inline)) {
    // this wave's rows of tile s landed (tile s+1 stays in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GL * (NB - 1)) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (bar) __builtin_amdgcn_s_barrier();
    if (s < 96) FFN_TL(2 + 2 * s);
    const bf16_t* tile = ring + (s % NB) * TROWS * BK;
    bf16x8 fw[BK / 32][T], fa[BK / 32][MT];
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int row = w * (T * 16) + t * 16 + fr;
        fw[ks][t] = ld8(tile + row * BK + (((ks * 4 + g) ^ ((row >> 1) & 7)) << 3));
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        fa[ks][mt] = ph2 ? ld8(Hc + (mt * 16 + fr) * HS + r * BK + ks * 32 + fk) : xa[ph2 ? 0 : r][ks][mt];
    }
    // once this step's fragments are in VGPRs its slot takes tile s+2 (tail:
    // the projection's first tiles, or a harmless reload of the last tile)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    issue(min(s + NB, ST - 1), s % NB);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks)
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if (ph2)
            acc2[t][mt] = FFN_MFMA(fw[ks][t], fa[ks][mt], acc2[t][mt]);
          else
            acc1[t][mt] = FFN_MFMA(fw[ks][t], fa[ks][mt], acc1[t][mt]);
        }
    // (a sched_barrier here, keeping the MFMAs above the next step's tile
    // wait instead of letting the scheduler sink most of them below it,
    // measured equal: 55.4-56.4 vs 53.8-56.6 us, profiles/r04i_chain_time.log)
    post();  // VALU work that rides under this step's MFMAs (after its DMA issue)
    if (s < 96) FFN_TL(3 + 2 * s);
  };
  auto none = []() __attribute__((always_inline)) {};
  // hidden tiles i = t*MT + mt in [i0, i1) of acc1 -> +b1, act -> Hn (4
  // consecutive units per lane, one 8-B store); acc1 tiles zeroed.  b1 and Hn
  // by explicit ds_read / ds_write: compiler-visible LDS accesses here get an
  // s_waitcnt vmcnt(0) (alias guard against the in-flight LDS-DMA tiles),
  // draining the weight stream
  auto act_tiles = [&](int i0, int i1, const float* b1c, bf16_t* Hn) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if ((t + 1) * MT <= i0 || t * MT >= i1) continue;
      const int n = w * (T * 16) + t * 16 + 4 * g;
      f32x4 bb;
      asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(bb) : "v"(lds_addr(b1c + n)) : "memory");
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int i = t * MT + mt;
        if (i < i0 || i >= i1) continue;
        const f32x4 v = acc1[t][mt];
        uint2 pk;
        pk.x = pack_bf16x2(act_fn<ACT>(v[0] + bb[0], a.slope), act_fn<ACT>(v[1] + bb[1], a.slope));
        pk.y = pack_bf16x2(act_fn<ACT>(v[2] + bb[2], a.slope), act_fn<ACT>(v[3] + bb[3], a.slope));
        const unsigned long long pv = (unsigned long long)pk.x | ((unsigned long long)pk.y << 32);
        asm volatile("ds_write_b64 %0, %1" ::"v"(lds_addr(Hn + (mt * 16 + fr) * HS + (n ^ ffn_sw(fr)))), "v"(pv) : "memory");
        acc1[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  for (int stage = 0; stage < (CHAIN ? 2 : 1); ++stage) {
  if (CHAIN && stage == 1) {
    FFN_TL(197);
    // ---- between the blocks: A's rows z = x + alpha (acc2 + b2) -> post-LN
    // (norm2) are B's residual (held in xres) and, through B's LN0, its
    // phase-1 operand (Xn -> VGPR fragments); nothing goes to HBM
    float z[T][MT][4];
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int d = (w * T + j) * 16 + 4 * g;
      f32x4 bb = lds_f4(prm + P_B2 * D + d);
      tie(bb);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const f32x4 xr = xres[j][mt];
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const v2f zz = v2f{xr[e], xr[e + 1]} +
                         v2f{a.alpha, a.alpha} * (v2f{acc2[j][mt][e], acc2[j][mt][e + 1]} + v2f{bb[e], bb[e + 1]});
          z[j][mt][e] = zz[0];
          z[j][mt][e + 1] = zz[1];
        }
        acc1[j][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc2[j][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    FFN_TL(200);
    if (a.gp) row_ln<D, T, MT, NW>(z, red, prm + P_GP * D, prm + P_BP * D, a.epsp, w, g, fr, a.inv_n, a.npad);
    FFN_TL(201);
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xres[j][mt] = f32x4{z[j][mt][0], z[j][mt][1], z[j][mt][2], z[j][mt][3]};
    row_ln<D, T, MT, NW>(z, red, prm + P_G0B * D, prm + P_B0B * D, a.eps0b, w, g, fr, a.inv_n, a.npad);
    FFN_TL(202);
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int d = (w * T + j) * 16 + 4 * g;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        uint2 pk;
        pk.x = pack_bf16x2(z[j][mt][0], z[j][mt][1]);
        pk.y = pack_bf16x2(z[j][mt][2], z[j][mt][3]);
        lds_st2(Xn + (mt * 16 + fr) * XS + (d ^ ffn_sw(fr)), pk);
      }
    }
    lds_barrier();
    FFN_TL(203);
    load_frags<K1, BK / 32, MT, XS, BK>(xa, Xn, fr, fk);
    FFN_TL(198);
  }
  const float* b1st = b1s + stage * a.H;  // this block's b1 (LDS)
  for (int c = 0; c < NCH; ++c) {
    const int s0 = stage * S + c * SPC;
#pragma unroll
    for (int r = 0; r < K1; ++r) step(s0 + r, r, false, nullptr, false, none);
    // hidden chunk -> +b1, act -> Hc; phase 2 reads it after the next step's
    // barrier.  The buffer written here was last read in chunk c-2, before
    // every wave passed chunk c-1's first phase-2 barrier.
    bf16_t* Hc = Hs + (c & 1) * BM * HS;
    act_tiles(0, T * MT, b1st + c * HC, Hc);
#pragma unroll
    for (int p = 0; p < K2; ++p) step(s0 + K1 + p, p, true, Hc, p == 0, none);
  }
  }  // stage
  if (!PROJ) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // retire the tail reloads
  FFN_TL(194);

  // ---- epilogue: lane holds rows m = mt*16 + fr, units d = (w*T + j)*16 + 4g .. +3
  // (CHAIN: the parameters of block B, which has no post-LN)
  const float* b2f = prm + (CHAIN ? P_B2B : P_B2) * D;
  const float alphaf = CHAIN ? a.alphab : a.alpha;
  const bool postln = !CHAIN && a.gp;
  float z[T][MT][4];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int d = (w * T + j) * 16 + 4 * g;
    f32x4 bb = lds_f4(b2f + d);
    tie(bb);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 xr = xres[j][mt];
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        const v2f zz = v2f{xr[e], xr[e + 1]} +
                       v2f{alphaf, alphaf} * (v2f{acc2[j][mt][e], acc2[j][mt][e + 1]} + v2f{bb[e], bb[e + 1]});
        z[j][mt][e] = zz[0];
        z[j][mt][e + 1] = zz[1];
      }
    }
  }
  FFN_TL(195);
  if (postln) row_ln<D, T, MT, NW>(z, red, prm + P_GP * D, prm + P_BP * D, a.epsp, w, g, fr, a.inv_n, a.npad);
  if (PROJ) {
    // the out rows wait in LDS (over the hidden-chunk buffers, free once the
    // row_ln barriers have passed) until the last weight tile has landed: a
    // store is counted by vmcnt like the LDS-DMA tiles, so a store issued
    // before a tile wait would hold that wait for its HBM write
    float* Zo = reinterpret_cast<float*>(Hs);  // BM x ZS fp32
    constexpr int ZS = D + 4;
    static_assert(BM * ZS * 4 <= 2 * BM * HS * 2, "out rows fit over Hs");
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xres[j][mt] = f32x4{z[j][mt][0], z[j][mt][1], z[j][mt][2], z[j][mt][3]};
    // u = next-LN(out) -> Xn (bf16) -> VGPR fragments, the A operand of the projection
    row_ln<D, T, MT, NW>(z, red, prm + P_GN * D, prm + P_BN * D, a.epsn, w, g, fr, a.inv_n, a.npad);
    FFN_TL(204);
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int d = (w * T + j) * 16 + 4 * g;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        lds_st4(Zo + (mt * 16 + fr) * ZS + d, xres[j][mt]);
        uint2 pk;
        pk.x = pack_bf16x2(z[j][mt][0], z[j][mt][1]);
        pk.y = pack_bf16x2(z[j][mt][2], z[j][mt][3]);
        lds_st2(Xn + (mt * 16 + fr) * XS + (d ^ ffn_sw(fr)), pk);
      }
    }
    lds_barrier();
    FFN_TL(205);
    // ---- projection y = u . Wp^T (bf16), 256 output columns per K1 steps.
    // Stores go out during the first MT steps of every column block, each
    // right after that step's DMA issue: the out rows in block 0 (T stores of
    // 16 B per step), block nc-1's y rows in block nc (one 16-B store per
    // step: proj_pair; the last block's after the loop).  A
    // tile wait counts the stores younger than its tile, so a store only has
    // to land before the wait two steps on instead of holding the next one
    // (a store counts in vmcnt like the LDS-DMA tiles).  Workgroups with rows
    // past M store unconditionally-counted nothing: their stores come at the
    // block ends / the end and their waits assume none younger.  No reloads
    // past ST-1.
    static_assert(MT <= K1, "stores of a column block fit in its steps");
    static_assert(T == 2, "a lane's two tiles of a row pair up into one 16-B store");
    const int ncp = a.np / TROWS;
    const bool full = m0 + BM <= mlim;
    // the previous column block's y (bf16): the 8 consecutive columns
    // 32w + 16 (g & 1) + 8 (g >> 1) .. of row mt*16 + fr (proj_pair)
    uint4 yq[MT];
    // stores of step r of column block c
    auto kst = [&](int c, int r) __attribute__((always_inline)) { return r < MT ? (c == 0 ? T : 1) : 0; };
    for (int nc = 0; nc < ncp; ++nc) {
#pragma unroll
      for (int r = 0; r < K1; ++r) {
        const int s = SF + nc * K1 + r;
        // stores of the two steps before (the first block has none before it)
        const int k1 = r >= 1 ? kst(nc, r - 1) : nc > 0 ? kst(nc - 1, K1 - 1) : 0;
        const int k2 = r >= 2 ? kst(nc, r - 2) : nc > 0 ? kst(nc - 1, K1 + r - 2) : 0;
        vm_wait((s + 1 < ST ? GL : 0) + (full ? k1 + k2 : 0));
        const bf16_t* tile = ring + (s % NB) * TROWS * BK;
        // fragment offsets from an opaque lane id (hoisted, they spill)
        int ln;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const int lfr = ln & 15, lg = ln >> 4;
        bf16x8 fw[BK / 32][T];
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks)
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const int row = w * (T * 16) + t * 16 + lfr;
            fw[ks][t] = ld8(tile + row * BK + (((ks * 4 + lg) ^ ((row >> 1) & 7)) << 3));
          }
        // the A operand from Xn each step.  (Held in VGPRs for all column
        // blocks, as phase 1 holds its operand: the 24 reads up front, with
        // every wave behind the same barrier, cost the ~800 cycles the steps
        // then saved; equal in the A/B, +13 .. 16 VGPRs: round 10.)
        bf16x8 fx[BK / 32][MT];
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const uint32_t la = (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) bf16_t*)(
                Xn + (mt * 16 + fr) * XS + r * BK + ks * 32 + fk));
            asm volatile("ds_read_b128 %0, %1" : "=v"(fx[ks][mt]) : "v"(la) : "memory");
          }
        f32x4 ov[T];
        if (r < MT && full && nc == 0) {
#pragma unroll
          for (int j = 0; j < T; ++j) ov[j] = lds_f4(Zo + (r * 16 + lfr) * ZS + (w * T + j) * 16 + 4 * lg);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (s + NB < ST) issue(s + NB, s % NB);
        asm volatile("" ::: "memory");  // the stores stay behind the DMA issue (the counts above)
        if (r < MT && full) {
          const long long row = m0 + r * 16 + lfr;
          if (nc == 0) {
#pragma unroll
            for (int j = 0; j < T; ++j)
              *reinterpret_cast<f32x4*>(a.out + row * D + (w * T + j) * 16 + 4 * lg) = ov[j];
          } else {
            *reinterpret_cast<uint4*>(a.yp + row * a.np + (nc - 1) * TROWS + w * (T * 16) + 16 * (lg & 1) + 8 * (lg >> 1)) =
                yq[r < MT ? r : 0];
          }
        }
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks)
#pragma unroll
          for (int t = 0; t < T; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              acc1[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ks][t], fx[ks][mt], acc1[t][mt], 0, 0, 0);
      }
      int ln;
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        yq[mt] = proj_pair(acc1[0][mt], acc1[1][mt]);
        acc1[0][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc1[1][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int row = m0 + mt * 16 + (ln & 15), lg = ln >> 4;
        if ((!full || nc == ncp - 1) && row < mlim)
          *reinterpret_cast<uint4*>(a.yp + (long long)row * a.np + nc * TROWS + w * (T * 16) + 16 * (lg & 1) + 8 * (lg >> 1)) =
              yq[mt];
      }
    }
    FFN_TL(206);
    if (!full) {
      f32x4 ov[T][MT];
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) ov[j][mt] = lds_f4(Zo + (mt * 16 + fr) * ZS + (w * T + j) * 16 + 4 * g);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int row = m0 + mt * 16 + fr;
          if (row < mlim) *reinterpret_cast<f32x4*>(a.out + (long long)row * D + (w * T + j) * 16 + 4 * g) = ov[j][mt];
        }
    }
    SBK_PROBE(asm volatile("s_waitcnt vmcnt(0)" ::: "memory");)  // the end mark includes the store drain
    FFN_TL(196);
    return;
  }
  // all residual reads of x are done before out (which may alias x) is written
  // (a null out is not stored: conv_tail_kernel keeps only u)
#pragma unroll
  for (int j = 0; j < T; ++j) {
    if (!a.out) break;
    const int d = (w * T + j) * 16 + 4 * g;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = m0 + mt * 16 + fr;
      if (row < mlim)
        *reinterpret_cast<float4*>(a.out + (long long)row * D + d) =
            make_float4(z[j][mt][0], z[j][mt][1], z[j][mt][2], z[j][mt][3]);
    }
  }
  if (a.gn) {
    row_ln<D, T, MT, NW>(z, red, prm + P_GN * D, prm + P_BN * D, a.epsn, w, g, fr, a.inv_n, a.npad);
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int d = (w * T + j) * 16 + 4 * g;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int row = m0 + mt * 16 + fr;
        if (row >= mlim) continue;
        if (a.u_bf16) {
          uint2 pk;
          pk.x = pack_bf16x2(z[j][mt][0], z[j][mt][1]);
          pk.y = pack_bf16x2(z[j][mt][2], z[j][mt][3]);
          *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.u) + (long long)row * D + d) = pk;
        } else {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.u) + (long long)row * D + d) =
              make_float4(z[j][mt][0], z[j][mt][1], z[j][mt][2], z[j][mt][3]);
        }
      }
    }
  }
  FFN_TL(196);
}

template <int D, int ACT, bool PROJ, bool CHAIN>
__global__ void __launch_bounds__(FFN_NT) ffn_kernel(FfnArgs a) {
  ffn_body<D, ACT, PROJ, CHAIN, false>(a, nullptr);
}

// [out_proj + residual + conv module of layer i] + [FFN2 + norm2 of layer i,
// FFN1 + norm1 + in_proj of layer i+1] on one 48-frame tile of one utterance:
// the conv module's output rows never leave the CU.  Grid: B * ceil(T / 48).
template <int ACT>
__global__ void __launch_bounds__(FFN_NT) conv_chain_kernel(FfnArgs a, ConvStageArgs c) {
  ffn_body<256, ACT, true, true, true>(a, &c);
}

// [out_proj + residual + conv module] + [FFN2 + norm2 + the closing
// LayerNorm] of the last layer on one 48-frame tile of one utterance: only
// u = LNn(LNp(z)) goes to HBM.  Grid: B * ceil(T / 48).
template <int ACT>
__global__ void __launch_bounds__(FFN_NT) conv_tail_kernel(FfnArgs a, ConvStageArgs c) {
  ffn_body<256, ACT, false, false, true>(a, &c);
}

// [src Linear (+ key-padding bytes)] + [FFN1 + norm1 + in_proj of layer 0]:
// ffn_kernel<256, ACT, true, false> on rows that come out of a.sa . Ws^T + bs
// in registers.  Grid: ceil(M / 48), the flat row tiling of ffn_kernel.
template <int ACT>
__global__ void __launch_bounds__(FFN_NT) src_ffn_kernel(FfnArgs a) {
  ffn_body<256, ACT, true, false, false, true>(a, nullptr);
}

template <int D>
size_t ffn_lds(int H, bool chain) {
  // 2-slot weight ring, Xn, two hidden-chunk buffers, b1 (two with CHAIN), the row-reduction scratch,
  // the epilogue parameter rows
  return ((size_t)2 * 256 * 64 + (size_t)FFN_BM * (D + FFN_PAD) + (size_t)2 * FFN_BM * (256 + FFN_PAD)) *
             sizeof(bf16_t) +
         (size_t)(chain ? 2 : 1) * H * 4 + (size_t)FFN_RS * FFN_BM * 4 + (size_t)FFN_NW * D * 4;
}

template <int D, int ACT, bool PROJ, bool CHAIN>
int launch_ffn_act(const FfnArgs& a, size_t lds, hipStream_t s) {
  // > 64 KB dynamic LDS: opted in per device, raised when a launch (a larger H) needs more
  if (hipError_t e = sbk::lds_optin(reinterpret_cast<const void*>(&ffn_kernel<D, ACT, PROJ, CHAIN>), lds))
    return (int)e;
  hipLaunchKernelGGL((ffn_kernel<D, ACT, PROJ, CHAIN>), dim3((a.M + FFN_BM - 1) / FFN_BM), dim3(FFN_NT), lds, s, a);
  return 0;
}

template <int D, bool PROJ, bool CHAIN>
int launch_ffn(const FfnArgs& a, hipStream_t s) {
  const size_t lds = ffn_lds<D>(a.H, CHAIN);
  if (lds > 160 * 1024) return SBK_ERR_ARG;
  switch (a.act) {
    case ACT_SWISH: return launch_ffn_act<D, ACT_SWISH, PROJ, CHAIN>(a, lds, s);
    case ACT_LRELU: return launch_ffn_act<D, ACT_LRELU, PROJ, CHAIN>(a, lds, s);
    case ACT_GELU: return launch_ffn_act<D, ACT_GELU, PROJ, CHAIN>(a, lds, s);
    case ACT_NONE: return launch_ffn_act<D, ACT_NONE, PROJ, CHAIN>(a, lds, s);
    default: return SBK_ERR_ARG;
  }
}

int ffn_dispatch(const FfnArgs& a, hipStream_t s) {
  const bool proj = a.np > 0, chain = a.g0b != nullptr;
  if (chain) return proj ? launch_ffn<256, true, true>(a, s) : launch_ffn<256, false, true>(a, s);
  return proj ? launch_ffn<256, true, false>(a, s) : launch_ffn<256, false, false>(a, s);
}

template <int ACT>
int launch_src_ffn_act(const FfnArgs& a, size_t lds, hipStream_t s) {
  if (hipError_t e = sbk::lds_optin(reinterpret_cast<const void*>(&src_ffn_kernel<ACT>), lds)) return (int)e;
  hipLaunchKernelGGL((src_ffn_kernel<ACT>), dim3((a.M + FFN_BM - 1) / FFN_BM), dim3(FFN_NT), lds, s, a);
  return 0;
}

int src_ffn_dispatch(const FfnArgs& a, hipStream_t s) {
  const size_t lds = ffn_lds<256>(a.H, false);
  // the A rows, row stride Kin + FFN_PAD, lie over Xn and the hidden-chunk buffers below the LN0 affine
  if (lds > 160 * 1024 || (size_t)FFN_BM * (a.Kin + FFN_PAD) > (size_t)3 * FFN_BM * (256 + FFN_PAD) - 2 * 256 * 2)
    return SBK_ERR_ARG;
  switch (a.act) {
    case ACT_SWISH: return launch_src_ffn_act<ACT_SWISH>(a, lds, s);
    case ACT_LRELU: return launch_src_ffn_act<ACT_LRELU>(a, lds, s);
    case ACT_GELU: return launch_src_ffn_act<ACT_GELU>(a, lds, s);
    case ACT_NONE: return launch_src_ffn_act<ACT_NONE>(a, lds, s);
    default: return SBK_ERR_ARG;
  }
}

template <int ACT, bool TAIL>
int launch_conv_chain_act(const FfnArgs& a, const ConvStageArgs& c, unsigned grid, size_t lds, hipStream_t s) {
  const auto kern = TAIL ? &conv_tail_kernel<ACT> : &conv_chain_kernel<ACT>;
  if (hipError_t e = sbk::lds_optin(reinterpret_cast<const void*>(kern), lds)) return (int)e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FFN_NT), lds, s, a, c);
  return 0;
}

// TAIL: one block and no projection (conv_tail_kernel)
template <bool TAIL>
int conv_chain_dispatch(const FfnArgs& a, const ConvStageArgs& c, hipStream_t s) {
  const size_t lds = ffn_lds<256>(a.H, !TAIL);
  static_assert(CS_LDS + 2 * 256 * 4 <= (2 * 256 * 64 + FFN_BM * (256 + FFN_PAD) * 3) * 2, "the conv stage lies under ring, Xn, Hs");
  if (lds > 160 * 1024) return SBK_ERR_ARG;
  const long long grid = (long long)c.B * ((c.T + FFN_BM - 1) / FFN_BM);
  if (grid > 0x7fffffffLL) return SBK_ERR_ARG;
  switch (a.act) {
    case ACT_SWISH: return launch_conv_chain_act<ACT_SWISH, TAIL>(a, c, (unsigned)grid, lds, s);
    case ACT_LRELU: return launch_conv_chain_act<ACT_LRELU, TAIL>(a, c, (unsigned)grid, lds, s);
    case ACT_GELU: return launch_conv_chain_act<ACT_GELU, TAIL>(a, c, (unsigned)grid, lds, s);
    case ACT_NONE: return launch_conv_chain_act<ACT_NONE, TAIL>(a, c, (unsigned)grid, lds, s);
    default: return SBK_ERR_ARG;
  }
}

// the conv stage's image: tile q < 8 (phase 1, K-step q / 2, half q % 2): row
// 32w + i = W1p row 64w + 32 (q % 2) + i, k (q / 2)*64 ..; tile 8 + kt (phase
// 3): W2 rows, k kt*64 ..; the ring's row swizzle as below
__global__ void __launch_bounds__(256) conv_image_kernel(const bf16_t* __restrict__ w1p, const bf16_t* __restrict__ w2,
                                                         bf16_t* __restrict__ img) {
  const int n = (CS_P1T + CS_P3T) * 256 * 8;  // 16-B chunks
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int s = i >> 11, rem = i & 2047, r = rem >> 3, jp = rem & 7;
    const int j = jp ^ ((r >> 1) & 7);
    const bf16_t* src = s < CS_P1T ? w1p + (long long)((r >> 5) * 64 + (s & 1) * 32 + (r & 31)) * CS_D + (s >> 1) * 64
                                   : w2 + (long long)r * CS_D + (s - CS_P1T) * 64;
    *reinterpret_cast<uint4*>(img + (long long)i * 8) = *reinterpret_cast<const uint4*>(src + 8 * j);
  }
}

// the out_proj image of the conv stage's phase -1: tile kt = wo's 256 rows, k
// kt*64 .., as the phase-3 tiles above
__global__ void __launch_bounds__(256) wo_image_kernel(const bf16_t* __restrict__ wo, bf16_t* __restrict__ img) {
  const int n = CS_WOT * 256 * 8;  // 16-B chunks
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int s = i >> 11, rem = i & 2047, r = rem >> 3, jp = rem & 7;
    const int j = jp ^ ((r >> 1) & 7);
    *reinterpret_cast<uint4*>(img + (long long)i * 8) =
        *reinterpret_cast<const uint4*>(wo + (long long)r * CS_D + s * 64 + 8 * j);
  }
}

// the depthwise-tap image of the conv stage's phase 2a: block j < CS_NP writes
// tap pair j of every channel with the rounding phase 2a applied per launch
// before (pack_bf16x2), block CS_NP the biases
__global__ void __launch_bounds__(CS_D) dw_image_kernel(const float* __restrict__ wc, const float* __restrict__ bc,
                                                        int K, uint32_t* __restrict__ img) {
  const int j = blockIdx.x, c = threadIdx.x;
  if (j == CS_NP) {
    img[j * CS_D + c] = __float_as_uint(bc ? bc[c] : 0.f);
    return;
  }
  const float lo = 2 * j < K ? wc[2 * j * CS_D + c] : 0.f;
  const float hi = 2 * j + 1 < K ? wc[(2 * j + 1) * CS_D + c] : 0.f;
  img[j * CS_D + c] = pack_bf16x2(lo, hi);
}

// ---- the weight-stream image.  Tile s (256 rows x 64 k, 32 KB) in the order
// ffn_kernel streams them: per FFN block (A, then B for a chain) and hidden
// chunk c of 256 units: K1 = D / 64 tiles of W1 rows c*256.. (k over D), then
// 4 tiles of W2 (all D rows, k over the chunk's units); then the projection:
// per 256 output columns nc, K1 tiles of Wp rows nc*256.. .  Row r of a tile
// holds its 8 chunks of 8 k in the order j' -> source chunk j' ^ ((r >> 1) & 7)
// (the ring's bank swizzle, applied here once instead of on every load).
struct ImgSrc {
  const bf16_t *w1, *w2, *w1b, *w2b, *wp;
  int D, H, ntile_blk, ntile_ffn, chain;
};

__device__ __forceinline__ void img_tile_src(const ImgSrc& q, int s, const bf16_t** mat, int* ld, int* row0,
                                             int* k0) {
  const int K1 = q.D / 64, SPC = K1 + 4;
  if (s >= q.ntile_ffn) {  // projection
    const int pj = s - q.ntile_ffn, nc = pj / K1, r = pj - nc * K1;
    *mat = q.wp; *ld = q.D; *row0 = nc * 256; *k0 = r * 64;
    return;
  }
  const bool sb = s >= q.ntile_blk;
  const int sl = sb ? s - q.ntile_blk : s, c = sl / SPC, r = sl - c * SPC;
  if (r < K1) {
    *mat = sb ? q.w1b : q.w1; *ld = q.D; *row0 = c * 256; *k0 = r * 64;
  } else {
    *mat = sb ? q.w2b : q.w2; *ld = q.H; *row0 = 0; *k0 = c * 256 + (r - K1) * 64;
  }
}

__global__ void __launch_bounds__(256) ffn_image_kernel(ImgSrc q, int ntile, bf16_t* __restrict__ img) {
  const long long n = (long long)ntile * 256 * 8;  // 16-B chunks
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int s = (int)(i >> 11), rem = (int)(i & 2047), r = rem >> 3, jp = rem & 7;
    const bf16_t* mat;
    int ld, row0, k0;
    img_tile_src(q, s, &mat, &ld, &row0, &k0);
    const int j = jp ^ ((r >> 1) & 7);
    *reinterpret_cast<uint4*>(img + i * 8) =
        *reinterpret_cast<const uint4*>(mat + (long long)(row0 + r) * ld + k0 + 8 * j);
  }
}

int ffn_tiles(int D, int H, int np, int chain) {
  const int per_blk = (H / 256) * (D / 64 + 4);
  return (chain ? 2 : 1) * per_blk + (np / 256) * (D / 64);
}

}  // namespace

SBK_PROBE_EXPORT(sbk_probe_ffn_tl, g_ffn_tl)

SBK_API int sbk_ffn_supported(int D, int H) { return D == 256 && H > 0 && H % 256 == 0 && H <= 2048; }

SBK_API long long sbk_ffn_image_elems(int D, int H, int np, int chain) {
  if (!sbk_ffn_supported(D, H) || np < 0 || np % 256) return -1;
  return (long long)ffn_tiles(D, H, np, chain) * 256 * 64;
}

SBK_API int sbk_ffn_image(const void* w1, const void* w2, const void* w1b, const void* w2b, const void* wp, int D,
                          int H, int np, void* img, void* stream) {
  const int chain = w1b != nullptr;
  if (!sbk_ffn_supported(D, H) || !w1 || !w2 || !img || (chain && !w2b) || np < 0 || np % 256 || (np > 0) != (wp != nullptr))
    return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(w1b) |
       reinterpret_cast<uintptr_t>(w2b) | reinterpret_cast<uintptr_t>(wp) | reinterpret_cast<uintptr_t>(img)) & 15)
    return SBK_ERR_ARG;
  ImgSrc q;
  q.w1 = reinterpret_cast<const bf16_t*>(w1); q.w2 = reinterpret_cast<const bf16_t*>(w2);
  q.w1b = reinterpret_cast<const bf16_t*>(w1b); q.w2b = reinterpret_cast<const bf16_t*>(w2b);
  q.wp = reinterpret_cast<const bf16_t*>(wp);
  q.D = D; q.H = H; q.chain = chain;
  q.ntile_blk = (H / 256) * (D / 64 + 4);
  q.ntile_ffn = (chain ? 2 : 1) * q.ntile_blk;
  const int nt = ffn_tiles(D, H, np, chain);
  const long long chunks = (long long)nt * 2048;
  hipLaunchKernelGGL(ffn_image_kernel, dim3((unsigned)std::min<long long>((chunks + 255) / 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, q, nt, reinterpret_cast<bf16_t*>(img));
  SBK_CHECK_LAUNCH();
  return 0;
}

namespace {
int ffn_check(const float* x, int M, int D, int H, const float* g0, const float* b0, const void* img,
              long long img_elems, int chain, const float* b1, int act, const float* b2, const float* gp,
              const float* bp, float* out, const float* gn, const float* bn, void* u, int np, void* yp,
              bool out_opt = false) {
  if (M <= 0 || !sbk_ffn_supported(D, H) || !g0 || !b0 || !img || !b1 || !b2 || (!out && !out_opt)) return SBK_ERR_ARG;
  // the image must be the one sbk_ffn_image built for this (D, H, np, chain):
  // the kernel streams exactly that many tiles from it
  if (np < 0 || np % 256 || img_elems != sbk_ffn_image_elems(D, H, np, chain)) return SBK_ERR_ARG;
  if (act == ACT_GLU || act < 0 || act > ACT_GELU || (gn && !u && np == 0)) return SBK_ERR_ARG;
  // projection tail: y = next-LN(out) . Wp^T, whole 256-column blocks; it
  // replaces the u output
  if (np < 0 || np % 256 || (np > 0 && (!gn || !bn || u || !yp))) return SBK_ERR_ARG;
  // float4 loads of rows and LayerNorm parameters, 16-B image pieces
  const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g0) |
                       reinterpret_cast<uintptr_t>(b0) | reinterpret_cast<uintptr_t>(b1) |
                       reinterpret_cast<uintptr_t>(b2) | reinterpret_cast<uintptr_t>(gp) |
                       reinterpret_cast<uintptr_t>(bp) | reinterpret_cast<uintptr_t>(out) |
                       reinterpret_cast<uintptr_t>(gn) | reinterpret_cast<uintptr_t>(bn) |
                       reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(yp);
  return (al & 15) ? SBK_ERR_ARG : 0;
}
}  // namespace

SBK_API int sbk_ffn_proj(const float* x, int M, int D, int d_eff, int H, const float* g0, const float* b0, float eps0,
                         const void* img, long long img_elems, const float* b1, int act, float slope, const float* b2,
                         float alpha, const float* gp, const float* bp, float epsp, float* out, const float* gn,
                         const float* bn, float epsn, void* u, int u_bf16, int np, void* yp, void* stream) {
  if (ffn_check(x, M, D, H, g0, b0, img, img_elems, 0, b1, act, b2, gp, bp, out, gn, bn, u, np, yp) || d_eff <= 0 ||
      d_eff > D)
    return SBK_ERR_ARG;
  FfnArgs a{};
  a.inv_n = 1.0f / (float)d_eff; a.npad = (float)(D - d_eff);
  a.x = x; a.M = M; a.H = H;
  a.g0 = g0; a.b0 = b0; a.eps0 = eps0;
  a.img = reinterpret_cast<const bf16_t*>(img); a.b1 = b1; a.act = act; a.slope = slope;
  a.b2 = b2; a.alpha = alpha;
  a.gp = gp; a.bp = bp; a.epsp = epsp;
  a.out = out;
  a.gn = gn; a.bn = bn; a.epsn = epsn; a.u = u; a.u_bf16 = u_bf16;
  a.np = np; a.yp = reinterpret_cast<bf16_t*>(yp);
  a.g0b = nullptr; a.b0b = nullptr; a.eps0b = 0.f; a.b1b = nullptr; a.b2b = nullptr; a.alphab = 0.f;
  const int rc = ffn_dispatch(a, (hipStream_t)stream);
  if (rc) return rc;
  SBK_CHECK_LAUNCH();
  return 0;
}

// Two consecutive FFN blocks in one launch (the second on the first's
// output, which never leaves the CU): block A (g0 .. gp: e.g. FFN2 + norm2 of
// Conformer layer i) then block B (g0b .. alphab: FFN1 of layer i+1, no
// post-LN), then next-LN / projection tail as sbk_ffn_proj.  out receives
// block B's output only.  img: sbk_ffn_image of (w1, w2, w1b, w2b, wp).
SBK_API int sbk_ffn_chain(const float* x, int M, int D, int d_eff, int H, int act, float slope, const float* g0,
                          const float* b0,
                          float eps0, const float* b1, const float* b2, float alpha, const float* gp, const float* bp,
                          float epsp, const float* g0b, const float* b0b, float eps0b, const float* b1b,
                          const float* b2b, float alphab, float* out, const float* gn, const float* bn, float epsn,
                          void* u, int u_bf16, const void* img, long long img_elems, int np, void* yp,
                          void* stream) {
  if (!g0b || !b0b || !b1b || !b2b) return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(g0b) | reinterpret_cast<uintptr_t>(b0b) | reinterpret_cast<uintptr_t>(b1b) |
       reinterpret_cast<uintptr_t>(b2b)) & 15)
    return SBK_ERR_ARG;
  if (ffn_check(x, M, D, H, g0, b0, img, img_elems, 1, b1, act, b2, gp, bp, out, gn, bn, u, np, yp) || d_eff <= 0 ||
      d_eff > D)
    return SBK_ERR_ARG;
  FfnArgs a{};
  a.inv_n = 1.0f / (float)d_eff; a.npad = (float)(D - d_eff);
  a.x = x; a.M = M; a.H = H;
  a.g0 = g0; a.b0 = b0; a.eps0 = eps0;
  a.img = reinterpret_cast<const bf16_t*>(img); a.b1 = b1; a.act = act; a.slope = slope;
  a.b2 = b2; a.alpha = alpha;
  a.gp = gp; a.bp = bp; a.epsp = epsp;
  a.out = out;
  a.gn = gn; a.bn = bn; a.epsn = epsn; a.u = u; a.u_bf16 = u_bf16;
  a.np = np; a.yp = reinterpret_cast<bf16_t*>(yp);
  a.g0b = g0b; a.b0b = b0b; a.eps0b = eps0b;
  a.b1b = b1b; a.b2b = b2b; a.alphab = alphab;
  const int rc = ffn_dispatch(a, (hipStream_t)stream);
  if (rc) return rc;
  SBK_CHECK_LAUNCH();
  return 0;
}

SBK_API int sbk_ffn(const float* x, int M, int D, int d_eff, int H, const float* g0, const float* b0, float eps0,
                    const void* img, long long img_elems, const float* b1, int act, float slope, const float* b2,
                    float alpha, const float* gp, const float* bp, float epsp, float* out, const float* gn,
                    const float* bn, float epsn, void* u, int u_bf16, void* stream) {
  return sbk_ffn_proj(x, M, D, d_eff, H, g0, b0, eps0, img, img_elems, b1, act, slope, b2, alpha, gp, bp, epsp, out, gn, bn,
                      epsn, u, u_bf16, 0, nullptr, stream);
}

// The source Linear's weight ws (256, Kin) bf16 as Kin / 64 tiles of 256 rows
// x 64 k in K order, rows swizzled as in sbk_ffn_image: the weight stream of
// sbk_src_ffn_proj's first stage.  Kin % 64 == 0, Kin <= 768 (the 48 A rows
// of a workgroup wait in LDS).
SBK_API long long sbk_src_image_elems(int Kin) {
  return Kin > 0 && Kin % 64 == 0 && Kin <= 768 ? (long long)(Kin / 64) * 256 * 64 : -1;
}

SBK_API int sbk_src_image(const void* ws, int Kin, void* img, void* stream) {
  if (sbk_src_image_elems(Kin) < 0 || !ws || !img) return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(img)) & 15) return SBK_ERR_ARG;
  // one "projection" of 256 columns over K = Kin: tile s = rows 0 .. 255, k s*64 ..
  ImgSrc q{};
  q.wp = reinterpret_cast<const bf16_t*>(ws);
  q.D = Kin; q.H = 0; q.chain = 0; q.ntile_blk = 0; q.ntile_ffn = 0;
  const int nt = Kin / 64;
  hipLaunchKernelGGL(ffn_image_kernel, dim3(nt * 8), dim3(256), 0, (hipStream_t)stream, q, nt,
                     reinterpret_cast<bf16_t*>(img));
  SBK_CHECK_LAUNCH();
  return 0;
}

// sbk_gemm (the src Linear: x = a ws^T + sbias, a (M, Kin) bf16, simg =
// sbk_src_image(ws)) followed by sbk_ffn_proj on x in one launch: x never
// reaches HBM.  With rel_len (B floats, M == B * T) the launch also writes the
// key-padding mask kpm_out (M bytes) as sbk_length_mask does; rel_len null:
// no mask (kpm_out unused).  out (M, D) fp32, yp (M, np) bf16, np > 0.
SBK_API int sbk_src_ffn_proj(const void* a_, int Kin, const void* simg, long long simg_elems, const float* sbias,
                             const float* rel_len, int T, unsigned char* kpm_out, int M, int D, int d_eff, int H,
                             const float* g0, const float* b0, float eps0, const void* img, long long img_elems,
                             const float* b1, int act, float slope, const float* b2, float alpha, const float* gp,
                             const float* bp, float epsp, float* out, const float* gn, const float* bn, float epsn,
                             int np, void* yp, void* stream) {
  if (!a_ || !simg || sbk_src_image_elems(Kin) < 0 || simg_elems != sbk_src_image_elems(Kin) || np <= 0) return SBK_ERR_ARG;
  if (rel_len && (!kpm_out || T <= 0 || M % T)) return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(a_) | reinterpret_cast<uintptr_t>(simg) | reinterpret_cast<uintptr_t>(sbias)) & 15)
    return SBK_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(rel_len) & 3) return SBK_ERR_ARG;
  // ffn_check's x: the rows are not read from memory; `out` stands in (checked as out)
  if (ffn_check(out, M, D, H, g0, b0, img, img_elems, 0, b1, act, b2, gp, bp, out, gn, bn, nullptr, np, yp) ||
      d_eff <= 0 || d_eff > D)
    return SBK_ERR_ARG;
  if (reinterpret_cast<const void*>(out) == a_) return SBK_ERR_ARG;
  FfnArgs a{};
  a.inv_n = 1.0f / (float)d_eff; a.npad = (float)(D - d_eff);
  a.x = nullptr; a.M = M; a.H = H;
  a.g0 = g0; a.b0 = b0; a.eps0 = eps0;
  a.img = reinterpret_cast<const bf16_t*>(img); a.b1 = b1; a.act = act; a.slope = slope;
  a.b2 = b2; a.alpha = alpha;
  a.gp = gp; a.bp = bp; a.epsp = epsp;
  a.out = out;
  a.gn = gn; a.bn = bn; a.epsn = epsn; a.u = nullptr; a.u_bf16 = 1;
  a.np = np; a.yp = reinterpret_cast<bf16_t*>(yp);
  a.sa = reinterpret_cast<const bf16_t*>(a_); a.simg = reinterpret_cast<const bf16_t*>(simg); a.sbias = sbias;
  a.Kin = Kin; a.Tm = T; a.rel_len = rel_len; a.kpm_out = rel_len ? kpm_out : nullptr;
  const int rc = src_ffn_dispatch(a, (hipStream_t)stream);
  if (rc) return rc;
  SBK_CHECK_LAUNCH();
  return 0;
}

// the tile that launch index `orig` of `nwg` workgroups owns in the XCD-contiguous
// order of the conv-stage launches, the GEMMs and the attention kernels
// (sbk::xcd_tile on the host; -1: no such workgroup)
SBK_API int sbk_xcd_tile(int nwg, int orig) { return nwg > 0 && orig >= 0 && orig < nwg ? xcd_tile(nwg, orig) : -1; }

SBK_API long long sbk_conv_image_elems(int D) { return D == CS_D ? (long long)(CS_P1T + CS_P3T) * CS_TILE : -1; }

SBK_API int sbk_conv_image(const void* w1p, const void* w2, int D, void* img, void* stream) {
  if (D != CS_D || !w1p || !w2 || !img) return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(w1p) | reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(img)) & 15)
    return SBK_ERR_ARG;
  hipLaunchKernelGGL(conv_image_kernel, dim3((CS_P1T + CS_P3T) * 8), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const bf16_t*>(w1p), reinterpret_cast<const bf16_t*>(w2),
                     reinterpret_cast<bf16_t*>(img));
  SBK_CHECK_LAUNCH();
  return 0;
}

// The out_proj weight wo (D, D) bf16 as the conv stage streams it: CS_WOT
// tiles of 256 rows x 64 k in the ring's format (as many elements as wo).
// sbk_conv_ffn_chain / sbk_conv_ffn_tail take this image as their `wo`.
SBK_API long long sbk_wo_image_elems(int D) { return D == CS_D ? (long long)CS_WOT * CS_TILE : -1; }

SBK_API int sbk_wo_image(const void* wo, int D, void* img, void* stream) {
  if (D != CS_D || !wo || !img || wo == img) return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(wo) | reinterpret_cast<uintptr_t>(img)) & 15) return SBK_ERR_ARG;
  hipLaunchKernelGGL(wo_image_kernel, dim3(CS_WOT * 8), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const bf16_t*>(wo), reinterpret_cast<bf16_t*>(img));
  SBK_CHECK_LAUNCH();
  return 0;
}

// The depthwise taps wc (K, D) fp32, tap-major, and the conv bias bc (D) or
// null as the conv stage's phase 2a reads them: 16 rows of D packed bf16 tap
// pairs (taps 2j, 2j + 1; taps >= K are zero), then a row of D fp32 biases
// (zero for a null bc), sbk_dw_image_elems(D) 32-bit words in all.
// sbk_conv_ffn_chain / sbk_conv_ffn_tail take this image as their `dwimg`.
SBK_API long long sbk_dw_image_elems(int D) { return D == CS_D ? (long long)CS_DW_WORDS : -1; }

SBK_API int sbk_dw_image(const float* wc, const float* bc, int K, int D, void* img, void* stream) {
  if (D != CS_D || K < 1 || K > CS_KMAX || !wc || !img || wc == img) return SBK_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(img) & 15) return SBK_ERR_ARG;
  hipLaunchKernelGGL(dw_image_kernel, dim3(CS_NP + 1), dim3(CS_D), 0, (hipStream_t)stream, wc, bc, K,
                     reinterpret_cast<uint32_t*>(img));
  SBK_CHECK_LAUNCH();
  return 0;
}

namespace {
// the convolution-module stage's arguments of sbk_conv_ffn_chain / sbk_conv_ffn_tail, checked
int conv_stage_args(ConvStageArgs& c, const float* x, const void* o, const void* wo, const float* bo, int B, int T, int D,
                    int d_eff, const float* cln0_w, const float* cln0_b, float ceps0, const void* cimg,
                    long long cimg_elems, const float* cb1p, const void* dwimg, int K, int causal,
                    const float* cln1_w, const float* cln1_b, float ceps1, const float* cb2, const unsigned char* kpm,
                    const void* out) {
  if (B <= 0 || T <= 0 || (long long)B * T > 0x7fffffffLL || D != CS_D || K < 1 || K > CS_KMAX || !x || !out ||
      x == out || d_eff <= 0 || d_eff > D)
    return SBK_ERR_ARG;
  if (!o || !wo || !cln0_w || !cln0_b || !cimg || !cb1p || !dwimg || !cln1_w || !cln1_b) return SBK_ERR_ARG;
  if (cimg_elems != sbk_conv_image_elems(D)) return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(o) | reinterpret_cast<uintptr_t>(wo) | reinterpret_cast<uintptr_t>(bo) |
       reinterpret_cast<uintptr_t>(cln0_w) | reinterpret_cast<uintptr_t>(cln0_b) | reinterpret_cast<uintptr_t>(cimg) |
       reinterpret_cast<uintptr_t>(cb1p) | reinterpret_cast<uintptr_t>(dwimg) | reinterpret_cast<uintptr_t>(cln1_w) | reinterpret_cast<uintptr_t>(cln1_b) |
       reinterpret_cast<uintptr_t>(cb2)) & 15)
    return SBK_ERR_ARG;
  c.x = x; c.B = B; c.T = T; c.K = K; c.padL = causal ? K - 1 : (K - 1) / 2;
  c.g0 = cln0_w; c.b0 = cln0_b; c.eps0 = ceps0;
  c.img = reinterpret_cast<const bf16_t*>(cimg); c.b1 = cb1p; c.dw = reinterpret_cast<const uint32_t*>(dwimg);
  c.g1 = cln1_w; c.b1n = cln1_b; c.eps1 = ceps1;
  c.b2 = cb2; c.kpm = reinterpret_cast<const uint8_t*>(kpm);
  c.o = reinterpret_cast<const bf16_t*>(o); c.wo = reinterpret_cast<const bf16_t*>(wo); c.bo = bo;
  return 0;
}
}  // namespace

// sbk_conv_module_pre followed by sbk_ffn_chain (with the projection tail) in
// one launch: x_c = x + o wo^T + bo through the convolution module (c*
// arguments, cimg = sbk_conv_image(w1p, w2c)), then the chain on x_c's rows,
// which stay on the CU.  out (B*T, D) fp32 must not alias x (neighbouring
// tiles read x for the conv halo); yp (B*T, np) bf16.
SBK_API int sbk_conv_ffn_chain(const float* x, const void* o, const void* wo, const float* bo, int B, int T, int D,
                               int d_eff, const float* cln0_w, const float* cln0_b, float ceps0, const void* cimg,
                               long long cimg_elems, const float* cb1p, const void* dwimg, const float* bc, int K,
                               int causal, const float* cln1_w, const float* cln1_b, float ceps1, const float* cb2,
                               const unsigned char* kpm, int H, int act, float slope, const float* g0, const float* b0,
                               float eps0, const float* b1, const float* b2, float alpha, const float* gp,
                               const float* bp, float epsp, const float* g0b, const float* b0b, float eps0b,
                               const float* b1b, const float* b2b, float alphab, float* out, const float* gn,
                               const float* bn, float epsn, const void* img, long long img_elems, int np, void* yp,
                               void* stream) {
  ConvStageArgs c;
  if (conv_stage_args(c, x, o, wo, bo, B, T, D, d_eff, cln0_w, cln0_b, ceps0, cimg, cimg_elems, cb1p, dwimg, K, causal,
                      cln1_w, cln1_b, ceps1, cb2, kpm, out))
    return SBK_ERR_ARG;
  if (!g0b || !b0b || !b1b || !b2b || !gn || !bn || !yp || np <= 0) return SBK_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(g0b) | reinterpret_cast<uintptr_t>(b0b) | reinterpret_cast<uintptr_t>(b1b) |
       reinterpret_cast<uintptr_t>(b2b)) & 15)
    return SBK_ERR_ARG;
  const int M = B * T;
  if (ffn_check(x, M, D, H, g0, b0, img, img_elems, 1, b1, act, b2, gp, bp, out, gn, bn, nullptr, np, yp))
    return SBK_ERR_ARG;
  FfnArgs a{};
  a.inv_n = 1.0f / (float)d_eff; a.npad = (float)(D - d_eff);
  a.x = x; a.M = M; a.H = H;
  a.g0 = g0; a.b0 = b0; a.eps0 = eps0;
  a.img = reinterpret_cast<const bf16_t*>(img); a.b1 = b1; a.act = act; a.slope = slope;
  a.b2 = b2; a.alpha = alpha;
  a.gp = gp; a.bp = bp; a.epsp = epsp;
  a.out = out;
  a.gn = gn; a.bn = bn; a.epsn = epsn; a.u = nullptr; a.u_bf16 = 1;
  a.np = np; a.yp = reinterpret_cast<bf16_t*>(yp);
  a.g0b = g0b; a.b0b = b0b; a.eps0b = eps0b;
  a.b1b = b1b; a.b2b = b2b; a.alphab = alphab;
  const int rc = conv_chain_dispatch<false>(a, c, (hipStream_t)stream);
  if (rc) return rc;
  SBK_CHECK_LAUNCH();
  return 0;
}

// sbk_conv_module_pre followed by sbk_ffn with its post-LN and next-LN in one
// launch, the end of the encoder stack: the last layer's convolution module,
// FFN2 + norm2 (g0 .. epsp) and the closing LayerNorm (gn, bn).  Only
// u (B*T, D) fp32 = LNn(LNp(x_c + alpha FFN(LN0(x_c)))) is written; it must
// not alias x.  img = sbk_ffn_image(w1, w2) of one block, no projection.
SBK_API int sbk_conv_ffn_tail(const float* x, const void* o, const void* wo, const float* bo, int B, int T, int D,
                              int d_eff, const float* cln0_w, const float* cln0_b, float ceps0, const void* cimg,
                              long long cimg_elems, const float* cb1p, const void* dwimg, const float* bc, int K,
                              int causal, const float* cln1_w, const float* cln1_b, float ceps1, const float* cb2,
                              const unsigned char* kpm, int H, int act, float slope, const float* g0, const float* b0,
                              float eps0, const float* b1, const float* b2, float alpha, const float* gp,
                              const float* bp, float epsp, const float* gn, const float* bn, float epsn, float* u,
                              const void* img, long long img_elems, void* stream) {
  ConvStageArgs c;
  if (conv_stage_args(c, x, o, wo, bo, B, T, D, d_eff, cln0_w, cln0_b, ceps0, cimg, cimg_elems, cb1p, dwimg, K, causal,
                      cln1_w, cln1_b, ceps1, cb2, kpm, u))
    return SBK_ERR_ARG;
  if (!gn || !bn) return SBK_ERR_ARG;
  const int M = B * T;
  if (ffn_check(x, M, D, H, g0, b0, img, img_elems, 0, b1, act, b2, gp, bp, nullptr, gn, bn, u, 0, nullptr, true))
    return SBK_ERR_ARG;
  FfnArgs a{};
  a.inv_n = 1.0f / (float)d_eff; a.npad = (float)(D - d_eff);
  a.x = x; a.M = M; a.H = H;
  a.g0 = g0; a.b0 = b0; a.eps0 = eps0;
  a.img = reinterpret_cast<const bf16_t*>(img); a.b1 = b1; a.act = act; a.slope = slope;
  a.b2 = b2; a.alpha = alpha;
  a.gp = gp; a.bp = bp; a.epsp = epsp;
  a.out = nullptr;
  a.gn = gn; a.bn = bn; a.epsn = epsn; a.u = u; a.u_bf16 = 0;
  a.np = 0; a.yp = nullptr;
  a.g0b = nullptr; a.b0b = nullptr; a.eps0b = 0.f; a.b1b = nullptr; a.b2b = nullptr; a.alphab = 0.f;
  const int rc = conv_chain_dispatch<true>(a, c, (hipStream_t)stream);
  if (rc) return rc;
  SBK_CHECK_LAUNCH();
  return 0;
}
