// The Conformer convolution module as a stage of the layer-chain kernel
// (ffn.hip: conv_chain_kernel), included there inside its namespace.
//
// The arithmetic and its rounding points are those of convmod.hip's
// conv_module_kernel<true> (phase -1 .. phase 3, see its header); the thread
// map is the chain's: 8 waves at up to 256 VGPRs instead of 16 at 128, so
// that one register budget serves both and phase 3's accumulators land in
// the chain's residual layout — wave w, lane (g, fr): rows mt*16 + fr, units
// (w*2 + j)*16 + 4g + e — and never leave the CU.
//   phase -1: wave w owns 32 out_proj units (two 16-unit tiles) of the 80
//             staged frames; o first across the workgroup, wo as four
//             image tiles through a 2-slot ring (LDS-DMA, as phases 1 and
//             3), x behind the last tile;
//   phase 1 : wave w owns GLU groups 2w and 2w + 1 (64 permuted rows of
//             W1p): the U fragments of a K-step are read once per 64 weight
//             rows instead of once per 32;
//   phase 2a: thread (channel, half) slides its window over 24 frames;
//   phase 2b: one wave per frame, 6 frames per wave;
//   phase 3 : wave w: units (w*2 + j)*16, three 16-frame m-tiles.
// Phases 1 and 3 stream their weights as the chain does: a pre-tiled,
// pre-swizzled image in stream order (sbk_conv_image: 8 tiles of W1p, 4 of
// W2, 256 rows x 64 k each, ffn_image_kernel's row swizzle), a wave's share of
// a tile one contiguous 4 KB run, through a 2-slot ring (one tile in flight
// behind the one being read) in the buffers the phase does not use.
// Round 12: phase -1 streams wo the same way (sbk_wo_image: 4 tiles; slots in
// Us and the front of Cv, both free until LN0 writes U).  Before, its
// fragments came from L2 16 rows x 64 B per wave instruction into 64 VGPRs
// that were only a staging area, K-step by K-step, with x trickled in
// between.  Now the queue holds, in order: o and the parameter rows (every
// wave's, by a bare s_barrier), tiles 0 and 1, tile 2 once tile 0's fragments
// are read, tile 3 and then all of x once tile 1's are.  The compiler does
// not count asm LDS-DMA, so every load here is asm with a counted wait.
// What it still adds: the chain's own parameter loads in front of this stage
// are visible ones, and their first use (stage()) draws s_waitcnt vmcnt(0),
// which also waits for tiles 0 and 1, in flight right behind o.  Timeline of
// workgroup 128 (probe builds, cycles): o landed 5.2k -> 3.7k, last out_proj
// MFMA 14.1k -> 12.0k, x landed 15.9k -> 13.1k, out_proj + sums done 18.0k ->
// 15.2k with the XCD-contiguous tile order of ffn.hip round 12.  The K loop
// is still 5.6k cycles for 80 MFMAs per wave: ~1.4k per tile, one tile's
// fetch latency, since a 2-slot ring has one tile in flight.
// Round 13: the small launch-constant parameter vectors of the middle phases
// were each fetched behind their phase's barrier and waited for at once, by
// all eight waves, with nothing else in flight.  Now each is on its way one
// phase early, by loads the compiler cannot see and a counted wait at first
// use: phase 1's bias b1 rides in the launch-start burst (threads that re-read
// b0 and dropped it) into LDS beside the LN0 affine; phase 2a's taps and bias
// come as 17 words per thread from an image (sbk_dw_image: the bf16 rounding
// and pairing that every workgroup of every launch did on 32 fp32 loads),
// issued behind phase 1's K loop; phase 2b's LN1 affine, b2 and the mask
// bytes go out at the head of phase 2a.  Middle phases of workgroup 128
// (probe builds, same box, cycles): GLU epilogue 3.5k -> 3.2k, phase 2a 7.4k
// -> 6.1k, phase 2b 5.1k -> 4.4k; the launch ends 2.4-2.7k earlier.  Measured
// equal and not kept: the residual's 24 ds_bpermute behind LN0's partial-sum
// stores, the statistics waves reducing before they issue phase 1's tiles, and
// sched_group_barriers for a deeper pipeline of phase 2a's window reads.
#pragma once

struct ConvStageArgs {
  const float* x;  // (B*T, D) fp32 residual stream
  int B, T, K, padL;
  const float *g0, *b0;  // LN0
  float eps0;
  const bf16_t* img;  // sbk_conv_image(w1p, w2)
  const float* b1;    // (2D) permuted like w1p
  const uint32_t* dw; // sbk_dw_image of the depthwise taps and the conv bias
  const float *g1, *b1n;  // LN1
  float eps1;
  const float* b2;      // (D) or null
  const uint8_t* kpm;   // (B*T) padding mask or null
  const bf16_t* o;      // (B*T, D) attention output
  const bf16_t* wo;     // sbk_wo_image of the (D, D) out_proj weight
  const float* bo;      // (D) or null
};

constexpr int CS_D = 256, CS_BM = FFN_BM, CS_KMAX = 31;
constexpr int CS_ROWS = 80;  // staged frames (BM + K - 1 <= 78, padded to 5 m-tiles)
constexpr int CS_MT1 = CS_ROWS / 16, CS_MT3 = CS_BM / 16;
constexpr int CS_NW = FFN_NW, CS_NT = FFN_NT;
constexpr int CS_S = CS_D + FFN_PAD;  // U / G row stride: rows swizzled by ffn_sw, as Xn / Hs
constexpr int CS_TILE = 256 * 64;     // elements of an image tile
constexpr int CS_P1T = 8, CS_P3T = 4; // image tiles of phase 1 (4 K-steps x 2 group halves) and phase 3
constexpr int CS_WOT = CS_D / 64;     // image tiles of the out_proj weight (sbk_wo_image)
constexpr int CS_NP = (CS_KMAX + 1) / 2;  // depthwise tap pairs (tap 31 is zero)
// sbk_dw_image: CS_NP rows of CS_D packed bf16 tap pairs (pair-major: a wave's
// load of one pair is one 256-B run), then a row of fp32 conv biases (0 for none)
constexpr int CS_DW_WORDS = (CS_NP + 1) * CS_D;
// LDS (bytes): U/V, G, the fp32 conv tile; ring slot 0 over G, slot 1 over the conv tile's front
constexpr int CS_OFF_G = CS_ROWS * CS_S * 2, CS_OFF_CV = 2 * CS_OFF_G;
constexpr int CS_LDS = CS_OFF_CV + CS_BM * CS_D * 4;
static_assert(CS_TILE * 2 <= CS_OFF_G && CS_TILE * 2 <= CS_BM * CS_D * 4, "ring slots fit");
// LN0's affine and phase 1's bias, staged by the prologue (floats into the conv
// tile: past ring slot 1, the LN0 partials and statistics)
constexpr int CS_GB0 = CS_TILE / 2 + 2 * CS_ROWS * (CS_NW + 4) + 2 * CS_ROWS;

// wave w's 4 KB of an image tile -> its 4 KB of a ring slot, four 1-KB LDS-DMA
// pieces from one base (the instruction offset applies to both addresses).
// From inline asm: the compiler sees no LDS write in flight, so the stage's
// plain LDS accesses get no alias-guard waits, and the ring waits are
// explicit counted vmcnt.  (m0 is written here and by the chain's DMA builtin
// only, each right before its use.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void cs_issue(const bf16_t* img, int tile, bf16_t* slot, int w, int lane) {
  const bf16_t* src = img + (long long)tile * CS_TILE + w * 2048 + lane * 8;
  const uint32_t la = __builtin_amdgcn_readfirstlane(lds_addr(slot + w * 2048));
  asm volatile(
      "s_mov_b32 m0, %1\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %0, off\n\t"
      "global_load_lds_dwordx4 %0, off offset:1024\n\t"
      "global_load_lds_dwordx4 %0, off offset:2048\n\t"
      "global_load_lds_dwordx4 %0, off offset:3072" ::"v"(src),
      "s"(la)
      : "memory", "m0");
}
#pragma clang diagnostic pop
// fragment of slot row `row`, 16-B chunk c (8 consecutive k)
__device__ __forceinline__ bf16x8 cs_frag(const bf16_t* slot, int row, int c) {
  return *reinterpret_cast<const bf16x8*>(slot + row * 64 + ((c ^ ((row >> 1) & 7)) << 3));
}
// 16 B of bf16 by a load the compiler cannot see (the caller waits by count)
typedef unsigned int cs_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ cs_u4 cs_gld16(const bf16_t* p) {
  cs_u4 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// one dword at p + OFF bytes, likewise
template <int OFF>
__device__ __forceinline__ uint32_t cs_gldw(const uint32_t* p) {
  uint32_t v;
  asm volatile("global_load_dword %0, %1, off offset:%2" : "=v"(v) : "v"(p), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ int cs_gldu8(const uint8_t* p) {
  int v;
  asm volatile("global_load_ubyte %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// conv-stage marks of the chain's timeline buffer (probe builds only): 210 + i
#define CS_TL(i)                                                                    \
  SBK_PROBE(if ((blockIdx.x == 128 || blockIdx.x == 127) && lane == 0)              \
                g_ffn_tl[(blockIdx.x == 127 ? 8 : 0) + w][210 + (i)] = __builtin_amdgcn_s_memtime();)
__device__ __forceinline__ void cs_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// 1 / (1 + exp(-x)) of a value pair, the sigmoid factor of GLU and Swish as
// `rcpf(1.0f + __expf(-x))` computes it (v_exp_f32 of x * -log2(e), approx
// rcp), with the multiply and the add in packed fp32
__device__ __forceinline__ v2f cs_rcp1pexp(v2f x) {
  const v2f t = x * v2f{-1.44269504088896340736f, -1.44269504088896340736f};
  const v2f d = v2f{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} + v2f{1.0f, 1.0f};
  return v2f{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}

// One tile (frames t0 .. t0 + 47 of utterance b) of the convolution module on
// x + o wo^T + bo.  zres[j][mt]: the module's output rows in the chain's
// residual layout, zero for frames at or past T.  `stage()` runs once before
// the first workgroup barrier (the caller's own LDS staging, outside
// [0, CS_LDS)).
template <typename F>
__device__ __forceinline__ void conv_stage(const ConvStageArgs& a, float inv_n, float npad, unsigned char* smem, int b,
                                           int t0, f32x4 (&zres)[2][CS_MT3], F&& stage) {
  bf16_t* Us = reinterpret_cast<bf16_t*>(smem);           // CS_ROWS x CS_S (U, later V)
  bf16_t* Gs = reinterpret_cast<bf16_t*>(smem + CS_OFF_G);  // CS_ROWS x CS_S
  float* Cv = reinterpret_cast<float*>(smem + CS_OFF_CV);   // CS_BM x CS_D fp32 conv output
  bf16_t* slot[2] = {Gs, reinterpret_cast<bf16_t*>(Cv)};

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, g = lane >> 4, fk = 8 * g;
  const int fks = fk ^ ffn_sw(fr);
  const int f0 = t0 - a.padL;  // frame of staged row 0
  const int nrows = CS_BM + a.K - 1;
  const long long ubase = (long long)b * a.T;
  CS_TL(0);

  // ---- phase -1: x_att = x + o wo^T + bo over the staged frames, LN0 -> U
  float4 xres[2][CS_MT3];
  {
    constexpr int OC = CS_ROWS * (CS_D / 8) / CS_NT;  // 16-B o chunks per thread
    static_assert(OC * CS_NT == CS_ROWS * (CS_D / 8), "whole chunks");
    // Every load of this phase is asm with a counted wait of its own: wo
    // streams through a ring by asm LDS-DMA, which the compiler does not count,
    // so its waits for visible loads in flight beside the tiles would drain them
    cs_u4 ov[OC];
#pragma unroll
    for (int i = 0; i < OC; ++i) {
      const int c = tid + i * CS_NT;
      const int r = c / (CS_D / 8), ch = c - r * (CS_D / 8);
      const int fc = min(max(f0 + r, 0), a.T - 1);
      ov[i] = cs_gld16(a.o + (ubase + fc) * CS_D + ch * 8);
    }
    // LN0's scratch (partials, statistics, affine) sits past ring slot 1
    float* lnscr = Cv + CS_TILE / 2;
    constexpr int RS = CS_NW + 4;  // partial-row stride (floats), 16-B aligned
    static_assert(CS_TILE / 2 + 2 * CS_ROWS * RS + 2 * CS_ROWS + 4 * CS_D <= CS_BM * CS_D, "LN0 scratch fits");
    float* gb0s = Cv + CS_GB0;  // [g0 | b0 | b1 (2 CS_D, for the GLU epilogue)]
    static_assert(CS_GB0 == CS_TILE / 2 + 2 * CS_ROWS * RS + 2 * CS_ROWS, "behind the partials and the statistics");
    // unconditional, as bo below (threads CS_D.. read b0 again and drop it).
    // Threads CS_D / 2 .. CS_D - 1 used to do the same: they fetch phase 1's
    // bias b1 instead, at no further load in the burst, and the GLU epilogue
    // reads it from LDS instead of from L2 behind its barrier
    static_assert(CS_NT >= CS_D, "one float4 of [g0 | b0 | b1] per thread");
    f32x4 gbv = gld4(tid < CS_D / 4   ? a.g0 + 4 * tid
                     : tid < CS_D / 2 ? a.b0 + 4 * (tid - CS_D / 4)
                     : tid < CS_D     ? a.b1 + 4 * (tid - CS_D / 2)
                                      : a.b0 + 4 * (tid % (CS_D / 4)));
    // wave w: units (w*2 + j)*16 .. +15 of all CS_MT1 frame tiles; D[unit 4g + e][frame mt*16 + fr]
    f32x4 xv[2][CS_MT1], bo4[2];
    const float* bop = a.bo ? a.bo : a.g0;  // a null bo reads g0 instead and is zeroed at the residual add
#pragma unroll
    for (int j = 0; j < 2; ++j) bo4[j] = gld4(bop + (w * 2 + j) * 16 + 4 * g);
    constexpr int NA = OC + 1 + 2;  // loads in front of the first data barrier: o, the LN0 affine, bo
    // The first data barrier needs o and the parameter rows only.  The CU's
    // one vector-memory queue returns in order and issue stalls while it is
    // full, so: a bare s_barrier (it waits for no data) puts every wave's o
    // requests ahead of any wave's wo request; the first two of wo's four
    // tiles (sbk_wo_image: 256 rows x 64 k, this wave's 32 rows one 4 KB run)
    // follow by LDS-DMA into the ring -- Us and the front of Cv, free until
    // LN0 writes U; LN0's scratch sits past the second slot -- and land while o
    // is staged; tile kt + 2 is issued when tile kt's fragments are in VGPRs;
    // x (needed only at the residual add) goes behind the last tile, so that
    // no wo tile waits for x in the in-order queue.
    constexpr int KT = CS_WOT;  // wo tiles = K-steps of 64
    bf16_t* wslot[2] = {Us, reinterpret_cast<bf16_t*>(Cv)};
    static_assert(CS_TILE * 2 <= CS_OFF_G, "a wo slot fits in Us");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    cs_issue(a.wo, 0, wslot[0], w, lane);
    cs_issue(a.wo, 1, wslot[1], w, lane);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // the NA loads landed, the two tiles stay in flight
    static_assert(NA == 8, "the burst's loads in front of the two tiles");
#pragma unroll
    for (int i = 0; i < OC; ++i) asm volatile("" : "+v"(ov[i]));
    vtie(gbv);
    vtie(bo4[0]);
    vtie(bo4[1]);
    CS_TL(9);  // o landed
#pragma unroll
    for (int i = 0; i < OC; ++i) {
      const int c = tid + i * CS_NT;
      const int r = c / (CS_D / 8), ch = c - r * (CS_D / 8), f = f0 + r;
      const bool live = r < nrows && f >= 0 && f < a.T;
      *reinterpret_cast<cs_u4*>(Gs + r * CS_S + ((ch * 8) ^ ffn_sw(r))) = live ? ov[i] : cs_u4{0u, 0u, 0u, 0u};
    }
    if (tid < CS_D) *reinterpret_cast<f32x4*>(gb0s + 4 * tid) = gbv;
    stage();
    cs_barrier();
    CS_TL(1);
    f32x4 acc[2][CS_MT1];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int mt = 0; mt < CS_MT1; ++mt) acc[j][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K order kk = 2 kt + ks = 0 .. 7 and the operand roles are those of the
    // fragment loads this replaces: every accumulator sees the same MFMAs
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      // tile kt landed; behind it in the queue: the next tile, and x once issued
      if (kt == 0 || kt == 1)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else if (kt == 2)
        asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
      static_assert(KT == 4 && 2 * CS_MT1 == 10, "the counted waits above");
      if (kt == 0) {
        CS_TL(10);  // the first wo tile landed: first MFMA
      }
      bf16x8 fw[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 2; ++j) fw[ks][j] = cs_frag(wslot[kt & 1], w * 32 + j * 16 + fr, ks * 4 + g);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (kt + 2 < KT) cs_issue(a.wo, kt + 2, wslot[kt & 1], w, lane);  // the slot's fragments are in VGPRs
      if (kt + 2 == KT - 1) {
#pragma unroll
        for (int i = 0; i < 2 * CS_MT1; ++i) {
          const int j = i / CS_MT1, mt = i - j * CS_MT1;
          const int f = min(max(f0 + mt * 16 + fr, 0), a.T - 1);
          xv[j][mt] = gld4(a.x + (ubase + f) * CS_D + (w * 2 + j) * 16 + 4 * g);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mt = 0; mt < CS_MT1; ++mt) {
          const bf16x8 fo = *reinterpret_cast<const bf16x8*>(Gs + (mt * 16 + fr) * CS_S + (kt * 2 + ks) * 32 + fks);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[j][mt] = FFN_MFMA(fw[ks][j], fo, acc[j][mt]);
        }
    }
    SBK_PROBE(asm volatile("" ::"s"(__builtin_amdgcn_readfirstlane(__float_as_int(acc[1][CS_MT1 - 1][0]))));)
    CS_TL(11);  // last MFMA retired
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int mt = 0; mt < CS_MT1; ++mt) vtie(xv[j][mt]);
    CS_TL(12);  // x landed
    if (!a.bo) bo4[0] = bo4[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float xa[2][CS_MT1][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int mt = 0; mt < CS_MT1; ++mt) {
        const v2f lo = v2f{xv[j][mt][0], xv[j][mt][1]} + (v2f{acc[j][mt][0], acc[j][mt][1]} + v2f{bo4[j][0], bo4[j][1]});
        const v2f hi = v2f{xv[j][mt][2], xv[j][mt][3]} + (v2f{acc[j][mt][2], acc[j][mt][3]} + v2f{bo4[j][2], bo4[j][3]});
        xa[j][mt][0] = lo[0];
        xa[j][mt][1] = lo[1];
        xa[j][mt][2] = hi[0];
        xa[j][mt][3] = hi[1];
      }
    // phase 3's residual: output frame mt*16 + fr is staged row mt*16 + fr +
    // padL, held (same units) by lane (fr + padL) % 16 of tile (mt*16 + fr +
    // padL) / 16.  The lane map is a permutation, so the source lane knows
    // its reader: lane fr is read for the upper tile exactly when fr < rr
    // (reader fr - rr + 16), and selects before the one permute per value
    {
      const int q = a.padL >> 4, rr = a.padL & 15;  // q <= 1 (K <= 31)
      const int src = ((lane & 0x30) + ((fr + rr) & 15)) << 2;
      const bool hi = fr < rr;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int mt = 0; mt < CS_MT3; ++mt) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo_v = q == 0 ? xa[j][mt][e] : xa[j][mt + 1][e];
            const float hi_v = q == 0 ? xa[j][mt + 1][e] : xa[j][mt + 2][e];
            v[e] = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(hi ? hi_v : lo_v)));
          }
          xres[j][mt] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    SBK_PROBE(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");)
    CS_TL(17);  // the residual's relocation returned
    // LN0 over the 256 units of each frame: 8 per lane, 4 lanes per wave
    // (col4), 8 waves through LDS; sum and sum of squares in one exchange
    // (var = E[x^2] - mean^2 in fp32, as conv_module_kernel<true>)
    float* red = lnscr;  // [CS_ROWS][RS] sums, then [CS_ROWS][RS] squares
#pragma unroll
    for (int mt = 0; mt < CS_MT1; ++mt) {
      v2f s2 = v2f{0.f, 0.f}, q2 = v2f{0.f, 0.f};  // value pairs (e, e + 1): packed adds / fmas
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const v2f xx = v2f{xa[j][mt][e], xa[j][mt][e + 1]};
          s2 += xx;
          q2 = __builtin_elementwise_fma(xx, xx, q2);
        }
      const float ps = col4_sum(s2[0] + s2[1]), pq = col4_sum(q2[0] + q2[1]);
      if (g == 0) {
        red[(mt * 16 + fr) * RS + w] = ps;
        red[CS_ROWS * RS + (mt * 16 + fr) * RS + w] = pq;
      }
    }
    CS_TL(2);
    cs_barrier();
    CS_TL(18);  // first exchange barrier
    // every wave is past its reads of Gs: phase 1's first two tiles land
    // under the statistics exchange and the LN0 application
    cs_issue(a.img, 0, slot[0], w, lane);
    cs_issue(a.img, 1, slot[1], w, lane);
    float* stat = red + 2 * CS_ROWS * RS;  // [CS_ROWS] mean, [CS_ROWS] rstd
    if (w < (CS_ROWS + 63) / 64 && w * 64 + lane < CS_ROWS) {
      const int row = w * 64 + lane;
      float t = 0.f, t2 = 0.f;
#pragma unroll
      for (int k4 = 0; k4 < CS_NW / 4; ++k4) {
        const float4 a4 = *reinterpret_cast<const float4*>(red + row * RS + 4 * k4);
        const float4 q4 = *reinterpret_cast<const float4*>(red + CS_ROWS * RS + row * RS + 4 * k4);
        t += a4.x; t += a4.y; t += a4.z; t += a4.w;
        t2 += q4.x; t2 += q4.y; t2 += q4.z; t2 += q4.w;
      }
      const float mu = t * inv_n;  // padded channels are zero: they add nothing to t or t2
      stat[row] = mu;
      stat[CS_ROWS + row] = __builtin_amdgcn_rsqf(fmaxf(t2 * inv_n - mu * mu, 0.f) + a.eps0);  // v_rsq_f32, 1 ulp
    }
    cs_barrier();
    CS_TL(19);  // second exchange barrier
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int u0 = (w * 2 + j) * 16 + 4 * g;
      const float4 g04 = *reinterpret_cast<const float4*>(gb0s + u0);
      const float4 b04 = *reinterpret_cast<const float4*>(gb0s + CS_D + u0);
#pragma unroll
      for (int mt = 0; mt < CS_MT1; ++mt) {
        const float mean = stat[mt * 16 + fr], rstd = stat[CS_ROWS + mt * 16 + fr];
        const int r = mt * 16 + fr, f = f0 + r;
        const bool live = r < nrows && f >= 0 && f < a.T;
        uint2 pk = make_uint2(0u, 0u);
        if (live) {
          const v2f m2 = v2f{mean, mean}, r2 = v2f{rstd, rstd};
          const v2f lo = (v2f{xa[j][mt][0], xa[j][mt][1]} - m2) * r2 * v2f{g04.x, g04.y} + v2f{b04.x, b04.y};
          const v2f hi = (v2f{xa[j][mt][2], xa[j][mt][3]} - m2) * r2 * v2f{g04.z, g04.w} + v2f{b04.z, b04.w};
          pk.x = pack_bf16x2(lo[0], lo[1]);
          pk.y = pack_bf16x2(hi[0], hi[1]);
        }
        *reinterpret_cast<uint2*>(Us + r * CS_S + (u0 ^ ffn_sw(fr))) = pk;
      }
    }
  }
  cs_barrier();
  CS_TL(3);

  // ---- phase 1: G = GLU(U W1p^T + b1p) over CS_ROWS frames.  Tile q = K-step
  // q / 2, half q % 2: wave w's rows of it are GLU group 2w + q % 2 (16 value
  // rows, 16 gate rows)
  uint32_t tw[CS_NP + 1];  // phase 2a's tap pairs and bias, loaded behind the K loop
  {
    f32x4 acc[2][2][CS_MT1];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int mt = 0; mt < CS_MT1; ++mt) acc[h][t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 fa[2][CS_MT1];  // U fragments of the K-step, shared by its two tiles
#pragma unroll
    for (int q = 0; q < CS_P1T; ++q) {
      const int kt = q >> 1, h = q & 1;
      // this tile landed; the one issued after it stays in flight
      if (q + 1 < CS_P1T)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      bf16x8 fw[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t) fw[ks][t] = cs_frag(slot[q & 1], w * 32 + t * 16 + fr, ks * 4 + g);
      if (h == 0) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mt = 0; mt < CS_MT1; ++mt)
            fa[ks][mt] = *reinterpret_cast<const bf16x8*>(Us + (mt * 16 + fr) * CS_S + kt * 64 + ks * 32 + fks);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (q + 2 < CS_P1T) cs_issue(a.img, q + 2, slot[q & 1], w, lane);  // the slot's fragments are in VGPRs
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int mt = 0; mt < CS_MT1; ++mt) acc[h][t][mt] = FFN_MFMA(fw[ks][t], fa[ks][mt], acc[h][t][mt]);
    }
    // Phase 2a's taps and bias (sbk_dw_image: packed pairs, pair-major, then
    // the bias row) go out here, one phase early: the queue is empty, and the
    // barrier and the GLU epilogue cover their latency.  b1 comes from LDS,
    // where the prologue put it, read before the barrier for the same reason
    {
      const uint32_t* dwp = a.dw + (tid & (CS_D - 1));
#pragma unroll
      for (int j4 = 0; j4 < CS_NP; j4 += 4) {
        tw[j4] = cs_gldw<0>(dwp + j4 * CS_D);
        tw[j4 + 1] = cs_gldw<CS_D * 4>(dwp + j4 * CS_D);
        tw[j4 + 2] = cs_gldw<2 * CS_D * 4>(dwp + j4 * CS_D);
        tw[j4 + 3] = cs_gldw<3 * CS_D * 4>(dwp + j4 * CS_D);
      }
      tw[CS_NP] = cs_gldw<0>(dwp + CS_NP * CS_D);
      static_assert(CS_NP % 4 == 0 && 3 * CS_D * 4 < 4096, "four loads per base, 12-bit offsets");
    }
    float4 b1a[2], b1g[2];  // b1 of the value / gate rows of channel group 2w + h
    {
      const float* b1s = Cv + CS_GB0 + 2 * CS_D;  // behind [g0 | b0]
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        b1a[h] = *reinterpret_cast<const float4*>(b1s + (w * 2 + h) * 32 + 4 * g);
        b1g[h] = *reinterpret_cast<const float4*>(b1s + (w * 2 + h) * 32 + 4 * g + 16);
      }
    }
    cs_barrier();  // every wave's ring reads are done before G overwrites Gs
    CS_TL(4);
    // GLU epilogue: lane holds frames mt*16 + fr, units 4g..4g+3 of each
    // tile; tiles (0, 1) = (value, gate) of channel group 2w + h
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ch = (w * 2 + h) * 16 + 4 * g;            // output channels ch .. ch + 3
      const float4 ba = b1a[h], bg = b1g[h];  // permuted rows (w*2 + h)*32 + 4g of value, + 16 of gate
      const v2f bav[2] = {v2f{ba.x, ba.y}, v2f{ba.z, ba.w}}, bgv[2] = {v2f{bg.x, bg.y}, v2f{bg.z, bg.w}};
      SBK_PROBE(if (h == 0) { asm volatile("" ::"v"(ba.x), "v"(bg.x) : "memory"); })
      if (h == 0) {
        CS_TL(13);  // the b1 vectors landed
      }
#pragma unroll
      for (int mt = 0; mt < CS_MT1; ++mt) {
        const int r = mt * 16 + fr, f = f0 + r;
        const bool live = r < nrows && f >= 0 && f < a.T;
        // value pairs (e, e + 1) in packed fp32; dead frames masked on the packed bf16 words
        uint32_t o[2];
#pragma unroll
        for (int e2 = 0; e2 < 2; ++e2) {
          const v2f va = v2f{acc[h][0][mt][2 * e2], acc[h][0][mt][2 * e2 + 1]} + bav[e2];
          const v2f vg = v2f{acc[h][1][mt][2 * e2], acc[h][1][mt][2 * e2 + 1]} + bgv[e2];
          const v2f sg = va * cs_rcp1pexp(vg);  // bf16 output: approx rcp
          o[e2] = pack_bf16x2(sg[0], sg[1]);
        }
        const uint2 pk = live ? make_uint2(o[0], o[1]) : make_uint2(0u, 0u);
        *reinterpret_cast<uint2*>(Gs + r * CS_S + (ch ^ ffn_sw(fr))) = pk;
      }
    }
  }
  cs_barrier();
  CS_TL(5);

  // ---- phase 2a: depthwise conv, thread (channel c, half h) over 24 frames,
  // two taps per v_dot2 (bf16 operands, fp32 accumulation) -> fp32 tile
  // The taps come packed from the image (before: 32 fp32 loads, 32 selects and
  // 16 packs per thread and launch, issued and waited for here).  Phase 2b's
  // LN1 affine, phase 3's bias and the key-padding bytes go out in their turn,
  // one phase early, under the window assembly and the dot loop
  f32x4 bb2[2], g14, b14;
  int km[CS_MT3];
  {
    const int c = tid & (CS_D - 1), h = tid >> 8;
    constexpr int NF = CS_BM / (CS_NT / CS_D);
    constexpr int NP = CS_NP;
    static_assert((CS_NT / CS_D - 1) * NF + NF + 2 * NP - 1 <= CS_ROWS, "every window row is staged");
    static_assert(NF % 4 == 0, "h * NF keeps bits 0-1 of the row; frame pairs");
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    bf2 tp[NP], ev[NF / 2 + NP - 1], od[NF / 2 + NP - 1];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the taps and the bias (nothing else is in flight)
#pragma unroll
    for (int j = 0; j <= NP; ++j) asm volatile("" : "+v"(tw[j]));
#pragma unroll
    for (int j = 0; j < NP; ++j) tp[j] = __builtin_bit_cast(bf2, tw[j]);
    const float bias = __uint_as_float(tw[NP]);
    CS_TL(14);  // the taps landed
    SBK_PROBE(asm volatile("" ::: "memory");)
    g14 = gld4(a.g1 + lane * 4);
    b14 = gld4(a.b1n + lane * 4);
    // unconditional (a null b2 / kpm reads g1 instead and is zeroed after the
    // wait): a load under a branch would be merged with the zero by a
    // register copy the compiler places before the data has landed
    const float* b2p = a.b2 ? a.b2 : a.g1;
#pragma unroll
    for (int j = 0; j < 2; ++j) bb2[j] = gld4(b2p + (w * 2 + j) * 16 + 4 * g);
#pragma unroll
    for (int mt = 0; mt < CS_MT3; ++mt)
      km[mt] = cs_gldu8(a.kpm ? a.kpm + ubase + min(t0 + mt * 16 + fr, a.T - 1) : reinterpret_cast<const uint8_t*>(a.g1));
    // row h * NF + k: its swizzle is ffn_sw(k) ^ ffn_sw(h * NF)
    const int cx = c ^ ffn_sw(h * NF);
    const unsigned short* Gu0 = reinterpret_cast<const unsigned short*>(Gs) + h * NF * CS_S + cx;
    const unsigned short* Gu1 = reinterpret_cast<const unsigned short*>(Gs) + h * NF * CS_S + (cx ^ 8);
    auto gu = [&](int k) __attribute__((always_inline)) { return (uint32_t)(ffn_sw(k) ? Gu1 : Gu0)[k * CS_S]; };
    uint32_t g0 = gu(0);
#pragma unroll
    for (int r = 0; r < NF / 2 + NP - 1; ++r) {
      const uint32_t g1 = gu(2 * r + 1), g2 = gu(2 * r + 2);
      ev[r] = __builtin_bit_cast(bf2, g0 | (g1 << 16));
      od[r] = __builtin_bit_cast(bf2, g1 | (g2 << 16));
      g0 = g2;
    }
    SBK_PROBE(for (int r = 0; r < NF / 2 + NP - 1; ++r) asm volatile("" : "+v"(ev[r]), "+v"(od[r])::"memory");)
    CS_TL(15);  // the window assembled
    SBK_PROBE(asm volatile("" ::: "memory");)
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      float s = bias;
#pragma unroll
      for (int j = 0; j < NP; ++j) s = __builtin_amdgcn_fdot2_f32_bf16(tp[j], (i & 1) ? od[i / 2 + j] : ev[i / 2 + j], s, false);
      Cv[(h * NF + i) * CS_D + c] = s;
    }
  }
  cs_barrier();
  CS_TL(6);

  // ---- phase 2b: LN1 -> Swish -> V (over U), one wave per frame, 4 channels
  // per lane.  Gs is free: phase 3's first tile lands under this phase (the
  // LN1 affine and phase 3's bias / key-padding bytes are in flight since
  // phase 2a and are waited for by count, ahead of it)
  {
    cs_issue(a.img, CS_P1T, slot[0], w, lane);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    vtie(g14);
    vtie(b14);
    vtie(bb2[0]);
    vtie(bb2[1]);
#pragma unroll
    for (int mt = 0; mt < CS_MT3; ++mt) asm volatile("" : "+v"(km[mt]));
    CS_TL(16);  // the LN1 affine, b2 and the mask bytes landed
    if (!a.b2) bb2[0] = bb2[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!a.kpm) km[0] = km[1] = km[2] = 0;
    const v2f gm[2] = {v2f{g14[0], g14[1]}, v2f{g14[2], g14[3]}}, bt[2] = {v2f{b14[0], b14[1]}, v2f{b14[2], b14[3]}};
    constexpr int FPW = CS_BM / CS_NW;  // frames per wave, side by side: their reduction chains interleave
    // channel pairs (e, e + 1) in packed fp32 (two-pass variance, as before)
    v2f v[FPW][2];
    float mean[FPW], rstd[FPW];
#pragma unroll
    for (int u = 0; u < FPW; ++u) {
      const float4 v4 = *reinterpret_cast<const float4*>(Cv + (w + u * CS_NW) * CS_D + lane * 4);
      v[u][0] = v2f{v4.x, v4.y};
      v[u][1] = v2f{v4.z, v4.w};
    }
#pragma unroll
    for (int u = 0; u < FPW; ++u) mean[u] = wave_sum_v((v[u][0][0] + v[u][0][1]) + (v[u][1][0] + v[u][1][1])) * inv_n;
#pragma unroll
    for (int u = 0; u < FPW; ++u) {
      const v2f m2 = v2f{mean[u], mean[u]}, d0 = v[u][0] - m2, d1 = v[u][1] - m2;
      const v2f q = __builtin_elementwise_fma(d1, d1, d0 * d0);
      rstd[u] = q[0] + q[1];
    }
#pragma unroll
    for (int u = 0; u < FPW; ++u)  // v_rsq_f32 (1 ulp) on a value >= eps
      rstd[u] = __builtin_amdgcn_rsqf((wave_sum_v(rstd[u]) - npad * mean[u] * mean[u]) * inv_n + a.eps1);
#pragma unroll
    for (int u = 0; u < FPW; ++u) {
      uint2 pk;
#pragma unroll
      for (int e2 = 0; e2 < 2; ++e2) {
        const v2f z = (v[u][e2] - v2f{mean[u], mean[u]}) * v2f{rstd[u], rstd[u]} * gm[e2] + bt[e2];
        const v2f sw = z * cs_rcp1pexp(z);  // bf16 output (as the GLU above)
        (e2 ? pk.y : pk.x) = pack_bf16x2(sw[0], sw[1]);
      }
      *reinterpret_cast<uint2*>(Us + (w + u * CS_NW) * CS_S + ((lane * 4) ^ ffn_sw(w))) = pk;  // CS_NW % 8 == 0
    }
  }
  cs_barrier();
  CS_TL(7);

  // ---- phase 3: z = x_att + rowmask0(V W2^T + b2), kept in registers
  {
    f32x4 acc[2][CS_MT3];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int mt = 0; mt < CS_MT3; ++mt) acc[j][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    cs_issue(a.img, CS_P1T + 1, slot[1], w, lane);  // the conv tile is free: the LN1 statistics are read
#pragma unroll
    for (int kt = 0; kt < CS_P3T; ++kt) {
      if (kt + 1 < CS_P3T)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      bf16x8 fw[2][2], fa[2][CS_MT3];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int j = 0; j < 2; ++j) fw[ks][j] = cs_frag(slot[kt & 1], w * 32 + j * 16 + fr, ks * 4 + g);
#pragma unroll
        for (int mt = 0; mt < CS_MT3; ++mt)
          fa[ks][mt] = *reinterpret_cast<const bf16x8*>(Us + (mt * 16 + fr) * CS_S + kt * 64 + ks * 32 + fks);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (kt + 2 < CS_P3T) cs_issue(a.img, CS_P1T + kt + 2, slot[kt & 1], w, lane);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int mt = 0; mt < CS_MT3; ++mt) acc[j][mt] = FFN_MFMA(fw[ks][j], fa[ks][mt], acc[j][mt]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int mt = 0; mt < CS_MT3; ++mt) {
        const bool live = t0 + mt * 16 + fr < a.T;
        const bool m = km[mt] != 0;
        const float4 xv = xres[j][mt];
        const v2f z2 = v2f{0.f, 0.f};
        const v2f c0 = v2f{acc[j][mt][0], acc[j][mt][1]} + v2f{bb2[j][0], bb2[j][1]};
        const v2f c1 = v2f{acc[j][mt][2], acc[j][mt][3]} + v2f{bb2[j][2], bb2[j][3]};
        const v2f o0 = v2f{xv.x, xv.y} + (m ? z2 : c0), o1 = v2f{xv.z, xv.w} + (m ? z2 : c1);
        zres[j][mt] = live ? f32x4{o0[0], o0[1], o1[0], o1[1]} : f32x4{0.f, 0.f, 0.f, 0.f};
      }
  }
  CS_TL(8);
}
