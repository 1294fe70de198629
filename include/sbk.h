/*
 * sbk.h — C ABI of libsbk.so, the MI355X (gfx950) kernel library behind
 * speechbrain_amd.  Plain pointers, sizes and a hipStream_t passed as void*;
 * no torch types.  Every entry point launches asynchronously on `stream`
 * and returns 0, a hipError_t code, or SBK_ERR_ARG (1001) for an invalid
 * shape/configuration detected on the host.  All pointers are device
 * pointers unless stated otherwise.
 *
 * The reference (Sinica-SLAM/speechbrain 0.5.13) has no FFI: its plugin
 * boundary is the nn.Module import path resolved by HyperPyYAML
 * (SURVEY.md §8b).  Each entry point below names the reference operation it
 * replaces; the Python drop-in modules in speechbrain_amd/ call these
 * through ctypes (speechbrain_amd/_lib.py).
 */
#ifndef SBK_H
#define SBK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBK_ERR_ARG 1001

/* ---------------------------------------------------------------- features */

/* 1 if n_fft (even) factors into radices {8,5,4,3,2} (the LDS FFT plan). */
int sbk_fft_supported(int n_fft);

/* STFT family, replaces torch.stft in STFT.forward
 * (speechbrain/processing/features.py:133-188), spectral_magnitude
 * (:327-356) and, fused, Filterbank.forward + _amplitude_to_DB before the
 * top_db clamp (:490-560, :691-712) — Fbank.forward (lobes/features.py:130-147).
 *   mode 0: STFT  -> out[bo*os_b + c*os_c + t*os_t + k*os_k + ri*os_ri]
 *   mode 1: power -> out[bo*os_b + c*os_c + t*os_t + k*os_k]  (power, eps, log_mag)
 *   mode 2: Fbank -> out (Bo, T, M) dB; slot_max (Bo, sbk_spectrum_slots(..)) receives one
 *           partial max per 8 frames (input of sbk_topdb_clamp; no atomics, deterministic)
 * n_fft 400 with C == 1 in modes 1 / 2 (M <= 128) runs the register-FFT kernel (8 lanes per
 * frame, LDS-DMA staged waveform); other sizes / modes the LDS Stockham kernels.  Both write
 * the same slot layout, so consumers of slot_max see no difference. 
 * wav: (Bo, S, C) fp32; window: n_fft fp32 (win centred, zero padded);
 * twiddle_nc: n_fft/2 complex W_{n_fft/2}^m; twiddle_nfft: n_fft/2+1 complex W_{n_fft}^k;
 * out_strides: HOST array of 5 int64 (modes 0/1); mel_*: per-filter CSR of the
 * (n_fft/2+1, M) filter matrix (start bin, length, offset into mel_w of n_melw weights). */
int sbk_spectrum(int mode, const float* wav, int Bo, int S, int C, int n_fft, int hop, int center, int pad_mode,
                 int T, const float* window, const float* twiddle_nc, const float* twiddle_nfft, int onesided,
                 float norm_scale, float power, float eps, int log_mag, const long long* out_strides,
                 const int* mel_start, const int* mel_len, const int* mel_off, const float* mel_w, int n_melw,
                 int M, int log_mel, float multiplier, float db_offset, float amin, float* out, float* slot_max,
                 void* stream);

/* Number of per-sequence partial-max slots sbk_spectrum(mode 2) writes. */
int sbk_spectrum_slots(int n_fft, int hop, int T, int M, int n_melw);

/* Filterbank.forward on a spectrogram (N, T, F) -> (N, T, M) (features.py:490-560):
 * sparse CSR filters, or a dense (F, M) matrix when `dense` is non-null
 * (learnable filters, freeze=False). */
int sbk_filterbank(const float* spec, int N, int T, int F, const int* mel_start, const int* mel_len,
                   const int* mel_off, const float* mel_w, const float* dense, int M, int log_mel, float multiplier,
                   float db_offset, float amin, float* out, float* slot_max, void* stream);

/* Number of per-sequence partial-max slots sbk_filterbank writes. */
int sbk_filterbank_slots(int T, int F);

/* top_db floor of _amplitude_to_DB (features.py:706-711), in place:
 * x[n, :] = max(x[n, :], max_n - top_db) for nseq sequences of per_seq values,
 * max_n = max of slot_max[n, 0:nslot]. */
int sbk_topdb_clamp(float* x, const float* slot_max, int nslot, long long per_seq, int nseq, float top_db,
                    void* stream);

/* Backward of the dB + top_db stage of Filterbank (features.py:691-712, what
 * autograd gives the reference for freeze=False filters, :476-482):
 * x = linear filterbank energies (N, per_seq) recomputed with
 * sbk_filterbank(log_mel=0), g = dL/d(output) -> dx = dL/dx, including the
 * amax (top_db reference) path with ties split as torch.maximum / amax do.
 * stats: 3*N floats of workspace.  log_mel=0 copies g. */
int sbk_filterbank_db_bwd(const float* x, const float* g, int N, long long per_seq, int log_mel, float multiplier,
                          float db_offset, float amin, float top_db, float* stats, float* dx, void* stream);

/* Dense filter-matrix gradient partials: part[c] (F, M) = sum over rows of chunk
 * c of spec[r, :]^T dx[r, :] (rows = N*T, M <= 128); reduce the
 * ceil(rows / rows_per_chunk) partials with sbk_colsum. */
int sbk_filterbank_wgrad(const float* spec, const float* dx, long long rows, int F, int M, long long rows_per_chunk,
                         float* part, void* stream);

/* spectral_magnitude (features.py:347-356): y[i] = f(sum_q x[i, q]^2), q < L. */
int sbk_magnitude(const float* x, float* y, long long n, int L, float power, float eps, int log_mag, void* stream);

/* DCT.forward (features.py:765-786): y (rows, n_out) = x (rows, n_in) @ D (n_in, n_out). */
int sbk_dct(const float* x, const float* D, float* y, long long rows, int n_in, int n_out, void* stream);

/* Deltas.forward (features.py:829-852) along time of (N, T, F); concat=1
 * writes [x | d1 | d2] (N, T, 3F) in one pass (lobes/features.py:141-144). */
int sbk_deltas(const float* x, float* y, int N, int T, int F, int window_length, int concat, void* stream);
/* processing/features.py:706-711 + lobes/features.py:141-144: the
 * [x | Δx | ΔΔx] concat of a log-mel fbank whose top_db floor was deferred
 * (sbk_spectrum's per-workgroup maxima slot_max (N, nslot)); x is floored
 * at max_b - top_db as it loads.  F % 4 == 0, 16-B aligned. */
int sbk_deltas_floor(const float* x, float* y, int N, int T, int F, int window_length, const float* slot_max,
                     int nslot, float top_db, void* stream);

/* ContextWindow.forward (features.py:917-937): (N, T, F) -> (N, T, F*(l+r+1)). */
int sbk_context_window(const float* x, float* y, int N, int T, int F, int left, int right, void* stream);

/* SpecAugment.forward (speechbrain/lobes/augment.py:106-201) on x (N, T, F)
 * fp32, in place: time warp (c, w; c < 0 = none; warp_mode 0 bicubic,
 * 1 bilinear — the align_corners interpolate modes of :134-148), then
 * frequency / time masks given as device int32 (N, n, 2) [len, pos] arrays
 * drawn on the host, filled with 0 or the running means (use_mean; `partial`
 * scratch of max(2*N*ceil(T/4), 3*N*(F/4)) + 4 floats, 16-B aligned;
 * n_fcells = number of frequency-masked cells, or < 0 to count them on the
 * device from the mask table).  F % 4 == 0, F <= 1024 with 16-B aligned x,
 * |c - w| <= 381 and <= 32 masks of each kind runs in place with no copy (x read once, the
 * unmasked cells written once, the masked cells written after the means);
 * otherwise the warp goes through `tmp` (a copy of x) —
 * sbk_specaugment_needs_scratch says which. */
int sbk_specaugment(float* x, int N, int T, int F, int c, int w, int warp_mode, float* tmp, const int* fmask,
                    int n_fmask, const int* tmask, int n_tmask, int use_mean, float* partial, long long n_fcells,
                    void* stream);
int sbk_specaugment_needs_scratch(int N, int T, int F, int c, int w, int n_fmask, int n_tmask, int x_aligned);

/* ------------------------------------------------------------ RNN-T loss */

/* Transducer forward (speechbrain/nnet/loss/transducer_loss.py:31-287 and
 * losses.py:79-85): x (B, T, U1, V) logits (is_logits=1: log-softmax fused)
 * or log-probs; labels (B, U1-1) int32; Tl, Ul (B,) int32 absolute lengths.
 * Computes per-cell blank/label log-probs, the α and β lattices
 * (anti-diagonal wavefront), log P, the sparse gradients and the reduced
 * loss: loss_mode 0 = SpeechBrain semantics -(α+lp)/T, 1 = -log P;
 * reduction 0 mean, 1 sum, 2 none (out holds B values).
 * ws: sbk_rnnt_workspace_floats(B, T, U1) floats, kept for the backward. */
int sbk_rnnt_forward(const float* x, const int* labels, const int* Tl, const int* Ul, int B, int T, int U1, int V,
                     int blank, int is_logits, int loss_mode, int reduction, float* ws, float* out, void* stream);
long long sbk_rnnt_workspace_floats(int B, int T, int U1);

/* Dense gradient (B, T, U1, V) from the forward's workspace: mode 0 wrt the
 * log-probs (Transducer.apply contract, zero except blank/label entries),
 * mode 1 wrt the logits through the log-softmax; rows scaled by scale[b]
 * (scale_per_b) or scale[0]. */
int sbk_rnnt_backward(const float* x, const int* labels, int B, int T, int U1, int V, int blank, int mode,
                      const float* ws, const float* scale, int scale_per_b, float* grad, void* stream);

/* The lattice half of sbk_rnnt_forward (α, β, log P, sparse gradients,
 * reduced loss) for per-cell log-probs already in ws[0 .. 3n) as
 * [lpb | lpl | lse], n = B*T*U1 — written by sbk_thead_fwd. */
int sbk_rnnt_lattice(const int* Tl, const int* Ul, int B, int T, int U1, int loss_mode, int reduction, float* ws,
                     float* out, void* stream);

/* ------------------------------------------------------------- CTC loss */

/* CTC (speechbrain.nnet.losses.ctc_loss, losses.py:245-294, i.e.
 * torch.nn.functional.ctc_loss with zero_infinity=True): x (B, T, V) fp32
 * logits (is_logits=1: log-softmax fused) or log-probs, batch first;
 * targets (B, Lmax) int32 without blanks (entries at j >= tg_len[b] are never
 * read); in_len, tg_len (B,) int32 absolute lengths on the device.  Computes
 * the compact log-probs of the 2*L_b+1 extended states, the α and β lattices
 * and loss[b] = -log P (B floats; 0 for an utterance with no valid alignment,
 * NaN for lengths outside [0, T] x [0, Lmax] or a label outside [0, V)).
 * ws: sbk_ctc_workspace_floats(B, T, Lmax) floats, 8-byte aligned, kept for
 * the backward.  Returns 1002 (before any launch) if 2*Lmax+1 > 3073. */
int sbk_ctc_forward(const float* x, const int* targets, const int* in_len, const int* tg_len, int B, int T, int V,
                    int Lmax, int blank, int is_logits, float* ws, float* loss, void* stream);
long long sbk_ctc_workspace_floats(int B, int T, int Lmax);

/* Dense gradient (B, T, V) from the forward's workspace, rows scaled by
 * grad_out[b].  is_logits=0: torch's ctc_loss convention wrt the log-probs,
 * exp(lp) - occupancy (every row sums to 0); is_logits=1: wrt the logits,
 * softmax - occupancy.  Rows t >= in_len[b] and utterances without a valid
 * alignment are zero.  Bit-identical from run to run. */
int sbk_ctc_backward(const float* x, const int* targets, const int* in_len, const int* tg_len, int B, int T, int V,
                     int Lmax, int blank, int is_logits, const float* ws, const float* grad_out, float* grad,
                     void* stream);

/* Row kernel of nll_loss / kldiv_loss (losses.py:405-452, 525-594): over the
 * rows r = b*U + u of x (B, U, V) fp32 with batch stride sb floats,
 * sel[r] = x[r, targets[r]] (NaN for a target outside [0, V)) and
 * rsum[r] = sum_v x[r, v]; the backward writes
 * grad[r, v] = a[r]*[v == targets[r]] + c[r] in the same layout. */
int sbk_nll_rows_forward(const float* x, const int* targets, int B, int U, long long sb, int V, float* sel,
                         float* rsum, void* stream);
int sbk_nll_rows_backward(const int* targets, const float* a, const float* c, int B, int U, long long sb, int V,
                          float* grad, void* stream);

/* ------------------------------------------------- fused transducer head */

/* Joint ("sum" + nonlinearity, transducer_joint.py:57-95) -> Linear(J -> V,
 * no bias) -> log-softmax -> RNN-T gather (losses.py:27-85 with
 * transducer_loss.py:31-106) without the (B, T, U1, V) logits:
 * z = act(tn[b,t] + pn[b,u]) rounded to bf16, S = z w^T (bf16 MFMA, fp32),
 * lse / lpb / lpl (B*T*U1 each; the ws layout of sbk_rnnt_lattice).
 * tn (B, T, J), pn (B, U1, J) fp32; w (sbk_thead_vpad(V), J) bf16 with rows
 * >= V zero; labels (B, U1-1) int32; J in {128, 256, 512, 1024}; act 0 none,
 * 3 LeakyReLU (slope), 6 ReLU. */
int sbk_thead_fwd(const float* tn, const float* pn, const void* w, const int* labels, int B, int T, int U1, int J,
                  int V, int blank, int act, float slope, float* lse, float* lpb, float* lpl, void* stream);
/* V rounded up to the head's column tiles (the row stride of dS). */
int sbk_thead_vpad(int V);
/* dS = ∂loss/∂logits (transducer_loss.py:183-236 through the log-softmax),
 * recomputed from tn, pn, w and the forward's lse, with the sparse
 * gradients gb, gl (sbk_rnnt_lattice's ws) scaled by scale[b] (scale_per_b)
 * or scale[0]: ds (B*T*U1, sbk_thead_vpad(V)) bf16, columns >= V zero;
 * w as for sbk_thead_fwd. */
int sbk_thead_dlogits(const float* tn, const float* pn, const void* w, const int* labels, int B, int T, int U1,
                      int J, int V, int blank, int act, float slope, const float* lse, const float* gb,
                      const float* gl, const float* scale, int scale_per_b, void* ds, void* stream);
/* dw (V, J) fp32 += ds^T z over the rows t < Tl[b] of every utterance (z
 * regenerated as in sbk_thead_fwd); dw must be initialised by the caller. */
int sbk_thead_wgrad(const void* ds, const float* tn, const float* pn, const int* Tl, int B, int T, int U1, int J,
                    int V, int act, float slope, float* dw, void* stream);

/* ----------------------------------------------------------------- encoder */

/* Key padding mask from relative lengths: out[b, t] = t > floor(rel_len[b] * T)
 * (uint8, (B, T)); TransformerASR.py:295-301 (make_transformer_src_mask's
 * length_to_mask on round(wav_len * T) in its fp32 form). */
int sbk_length_mask(const float* rel_len, int B, int T, uint8_t* out, void* stream);

/* Output channels per wave tile in the GLU-paired GEMM (weights are
 * row-permuted in groups of this size). */
int sbk_gemm_glu_group(int dtype_bf16);

/* out = res + alpha * act(A @ W^T + bias), masked rows -> 0 before the residual.
 * A (M, K) lda, W (N, K) ldw, both bf16 (dtype_bf16=1) or fp32; act: 0 none,
 * 1 Swish, 2 GLU (N/2 outputs, W permuted), 3 LeakyReLU(slope), 4 GELU;
 * res fp32 (M, ldr) or null; rowmask uint8 (M) or null; out fp32 or bf16.
 * Replaces nn.Linear / 1x1 Conv1d sites: attention.py:549-553,581,636,823-839;
 * Conformer.py:73-79,87-92,105; TransformerASR.py:127-135. */
int sbk_gemm(int dtype_bf16, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
             const float* bias, int act, float slope, const float* res, int ldr, float alpha,
             const uint8_t* rowmask, void* out, int ldc, int out_bf16, int tile, void* stream);

/* sbk_gemm (act none, fp32 out) followed by u = LN(out row; ln_g, ln_b, ln_eps) in
 * the same launch (full-row tiles: N == 256).  The attention output projection +
 * residual and the convolution module's LayerNorm: attention.py:636 with
 * Conformer.py:69-72.  u (M, ldu) bf16 when u_bf16, else fp32; tile 0 default. */
int sbk_gemm_ln(int dtype_bf16, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                const float* bias, const float* res, int ldr, float alpha, const uint8_t* rowmask, float* out,
                int ldc, const float* ln_g, const float* ln_b, float ln_eps, void* u, int ldu, int u_bf16, int tile,
                void* stream);

/* 1 if the fused FFN kernel supports d_model D and d_ffn H (D == 256, H % 256 == 0, H <= 2048). */
int sbk_ffn_supported(int D, int H);

/* Batched C[z] = A[z] W[z]^T (bf16 (dtype_bf16) or fp32 operands, K-contiguous
 * rows; fp32 or bf16 out), element strides sA / sW per batch; batch z is
 * stored at (z / zdiv) * sCo + (z % zdiv) * sC when zdiv > 0, else at z * sC.
 * The per-(utterance, head) products of the rel-pos attention backward and
 * the dropout product drop(P) V (attention.py:626-633), written straight
 * into the (B*T, H*dh) layout with zdiv = H. */
int sbk_gemm_batched(int dtype_bf16, const void* A, int lda, long long sA, const void* W, int ldw, long long sW, int M,
                     int N, int K, int batch, void* out, int ldc, long long sC, int zdiv, long long sCo, int out_bf16,
                     void* stream);

/* Weight-gradient GEMM (bf16 MFMA): C[b] += A[b]^T B[b], A (K, M) and B
 * (K, N) row-major with row strides lda / ldb (the token rows of dY and X:
 * dW = dY^T X of nn.Linear / conv backward, linear.py:15-76), C (M, N) fp32
 * (row stride ldc) accumulated with atomics (caller-initialised); sA / sB /
 * sC batch strides (elements).  M, N, lda, ldb % 8 == 0; A, B 16-B aligned. */
int sbk_gemm_tn(const void* A, long long lda, long long sA, const void* B, long long ldb, long long sB, int M, int N,
                int K, int batch, float* C, long long ldc, long long sC, void* stream);
/* sbk_gemm_tn with an explicit tile (64 / 128; 0 = auto) and token-range split count (0 = auto). */
int sbk_gemm_tn_cfg(const void* A, long long lda, long long sA, const void* B, long long ldb, long long sB, int M,
                    int N, int K, int batch, float* C, long long ldc, long long sC, int tile, int nsplit, void* stream);
/* Exact-fp32 weight-gradient GEMM (v_mfma_f32_16x16x4_f32): arguments as
 * sbk_gemm_tn_cfg with fp32 A, B and tile 64; any M, N, lda, ldb (element-wise
 * loads when not 16-B aligned); nsplit 0 = choose, 1 = deterministic.  The
 * fp32 (parity) training path. */
int sbk_gemm_tn_f32(const float* A, long long lda, long long sA, const float* B, long long ldb, long long sB, int M,
                    int N, int K, int batch, float* C, long long ldc, long long sC, int nsplit, void* stream);

/* Weight-stream image of the fused FFN kernels: the launch's bf16 weights as
 * 32-KB tiles (256 rows x 64 k) in the order the kernel streams them — per
 * FFN block (w1 (H, D), w2 (D, H); a chain's second block w1b, w2b) and
 * hidden chunk of 256 units: D/64 tiles of w1, then 4 of w2; then the
 * projection wp (np, D), D/64 tiles per 256 output columns — with the LDS
 * bank swizzle applied (row r's 16-B chunk j' holds chunk j' ^ ((r >> 1) & 7)),
 * so every wave streams one contiguous 4 KB per tile.  Built once per weight
 * version by the caller (a cache), read by sbk_ffn / sbk_ffn_proj /
 * sbk_ffn_chain.  sbk_ffn_image_elems: its size in bf16 elements (host only;
 * -1 for an unsupported shape); chain != 0 counts the second block. */
long long sbk_ffn_image_elems(int D, int H, int np, int chain);
int sbk_ffn_image(const void* w1, const void* w2, const void* w1b, const void* w2b, const void* wp, int D, int H,
                  int np, void* img, void* stream);

/* Fused macaron feed-forward block, bf16 MFMA (Conformer.py:239-260 with
 * attention.py:823-839):
 *   z = x + alpha * (act(LN0(x) W1^T + b1) W2^T + b2);  out = LNp(z) if gp;
 *   u = LNn(out) if gn (bf16 when u_bf16, else fp32).
 * x, out (M, D) fp32 (out may alias x); img = sbk_ffn_image(w1, w2) of
 * w1 (H, D), w2 (D, H) bf16; b1, b2 required (zeros when the Linear has no
 * bias); act as sbk_gemm (not GLU).  img_elems: the image's size in bf16
 * elements, which must equal sbk_ffn_image_elems(D, H, np, chain) of this
 * call (SBK_ERR_ARG otherwise: an image built for another shape or for one
 * block instead of a chain is refused, never read out of bounds).
 * d_eff (1..D): the LayerNorms' statistics run over the first d_eff columns;
 * columns d_eff..D-1 must be zero-padded channels (zero in x, in the LN
 * gains / biases and in every weight row or column that reaches them), so a
 * d_model < 256 model (conformer_small.yaml: 144) runs these kernels at
 * D = 256 with results equal to the unpadded arithmetic.  d_eff = D: plain. */
int sbk_ffn(const float* x, int M, int D, int d_eff, int H, const float* g0, const float* b0, float eps0, const void* img,
            long long img_elems, const float* b1, int act, float slope, const float* b2, float alpha, const float* gp, const float* bp,
            float epsp, float* out, const float* gn, const float* bn, float epsn, void* u, int u_bf16, void* stream);

/* sbk_ffn with a projection tail: with np > 0 (np % 256 == 0; img =
 * sbk_ffn_image(w1, w2, null, null, wp), wp (np, D) bf16) the next-LN output
 * is not written (u must be null) but projected on chip: yp (M, np) bf16 =
 * LNn(out) wp^T — the following MHSA's in_proj (attention.py:549-553,
 * Conformer.py:186-197), replacing its QKV GEMM launch.  np == 0 behaves as
 * sbk_ffn. */
int sbk_ffn_proj(const float* x, int M, int D, int d_eff, int H, const float* g0, const float* b0, float eps0, const void* img,
                 long long img_elems, const float* b1, int act, float slope, const float* b2, float alpha, const float* gp,
                 const float* bp, float epsp, float* out, const float* gn, const float* bn, float epsn, void* u,
                 int u_bf16, int np, void* yp, void* stream);

/* Two consecutive FFN blocks in one launch: block A (g0 .. epsp, as
 * sbk_ffn with its post-LN) then block B (g0b .. alphab: LN0, biases and
 * alpha, no post-LN) on A's output, which never leaves the CU; then next-LN
 * and the projection tail as sbk_ffn_proj.  out receives B's output.  img =
 * sbk_ffn_image(w1, w2, w1b, w2b, wp).  The Conformer's FFN2 + norm2 of
 * layer i with FFN1 + norm1 + in_proj of layer i+1 (Conformer.py:239-260,
 * attention.py:549-553); H is common to both. */
int sbk_ffn_chain(const float* x, int M, int D, int d_eff, int H, int act, float slope, const float* g0,
                  const float* b0,
                  float eps0, const float* b1, const float* b2, float alpha, const float* gp, const float* bp,
                  float epsp, const float* g0b, const float* b0b, float eps0b, const float* b1b, const float* b2b,
                  float alphab, float* out, const float* gn, const float* bn, float epsn, void* u, int u_bf16,
                  const void* img, long long img_elems, int np, void* yp, void* stream);

/* Tile owned by launch index orig of nwg workgroups in the XCD-contiguous
 * order (sbk_conv_ffn_chain / sbk_conv_ffn_tail, the GEMMs, attention):
 * blocks of one orig % 8 own one contiguous run of tiles, the runs ascending
 * with the residue.  A bijection of [0, nwg); -1 outside it.  Host only. */
int sbk_xcd_tile(int nwg, int orig);

/* The out_proj weight wo (D, D) bf16 as the conv stage of sbk_conv_ffn_chain /
 * sbk_conv_ffn_tail streams it: 4 tiles of 256 rows x 64 k, rows swizzled as
 * in sbk_ffn_image (as many elements as wo).  Those two entry points take
 * this image as their `wo` argument; sbk_conv_module_pre takes wo itself.
 * D = 256; img must not alias wo. */
long long sbk_wo_image_elems(int D);
int sbk_wo_image(const void* wo, int D, void* img, void* stream);

/* The depthwise taps wc (K, D) fp32, tap-major, and the conv bias bc (D) or
 * null as the conv stage of sbk_conv_ffn_chain / sbk_conv_ffn_tail reads them:
 * 16 rows of D words, word c of row j = taps 2j, 2j + 1 of channel c rounded
 * to bf16 (low, high half; taps >= K are zero), then a row of D fp32 biases
 * (zero for a null bc): sbk_dw_image_elems(D) 32-bit words.  Those two entry
 * points take this image as their `dwimg` argument; sbk_conv_module_pre takes
 * wc and bc themselves.  D = 256, 1 <= K <= 31; img 16-byte aligned. */
long long sbk_dw_image_elems(int D);
int sbk_dw_image(const float* wc, const float* bc, int K, int D, void* img, void* stream);

/* Weight-stream image of the convolution-module stage of sbk_conv_ffn_chain:
 * w1p (2D, D) GLU-permuted and w2 (D, D) bf16 as 12 tiles of 256 rows x 64 k
 * in stream order (8 of w1p: per 64 k, the first then the second GLU group of
 * every wave; 4 of w2), rows swizzled as in sbk_ffn_image.  D = 256. */
long long sbk_conv_image_elems(int D);
int sbk_conv_image(const void* w1p, const void* w2, int D, void* img, void* stream);

/* sbk_conv_module_pre (o, wo required) followed by sbk_ffn_chain with its
 * projection tail (np > 0) in one launch, one workgroup per 48-frame tile of
 * one utterance: the convolution module's output rows stay on the CU as the
 * chain's input and residual.  c* arguments: the convolution module's (as
 * sbk_conv_module_pre, except that wo is sbk_wo_image(wo), not wo itself, and
 * that dwimg = sbk_dw_image(wc, bc) stands for the taps: it carries the conv
 * bias, so bc is not read here and keeps its place in the list only;
 * cimg = sbk_conv_image(w1p, w2)); H .. yp: the chain's (as sbk_ffn_chain).  out (B*T, D) fp32 receives block B's output and must
 * not alias x; yp (B*T, np) bf16.  D = 256, K <= 31. */
int sbk_conv_ffn_chain(const float* x, const void* o, const void* wo, const float* bo, int B, int T, int D, int d_eff,
                       const float* cln0_w, const float* cln0_b, float ceps0, const void* cimg, long long cimg_elems,
                       const float* cb1p, const void* dwimg, const float* bc, int K, int causal, const float* cln1_w,
                       const float* cln1_b, float ceps1, const float* cb2, const unsigned char* kpm, int H, int act,
                       float slope, const float* g0, const float* b0, float eps0, const float* b1, const float* b2,
                       float alpha, const float* gp, const float* bp, float epsp, const float* g0b, const float* b0b,
                       float eps0b, const float* b1b, const float* b2b, float alphab, float* out, const float* gn,
                       const float* bn, float epsn, const void* img, long long img_elems, int np, void* yp,
                       void* stream);

/* sbk_conv_module_pre (o, wo required) followed by sbk_ffn with its post-LN
 * and next-LN in one launch, the end of the encoder stack: the last layer's
 * convolution module, FFN2 + norm2 (g0 .. epsp) and the encoder's closing
 * LayerNorm (gn, bn; Conformer.py:340).  Same grid and arguments as
 * sbk_conv_ffn_chain without block B and the projection; img =
 * sbk_ffn_image(w1, w2).  Only u (B*T, D) fp32 = LNn(LNp(z)) is written (the
 * module's output and the pre-LN rows stay on the CU); u must not alias x. */
int sbk_conv_ffn_tail(const float* x, const void* o, const void* wo, const float* bo, int B, int T, int D, int d_eff,
                      const float* cln0_w, const float* cln0_b, float ceps0, const void* cimg, long long cimg_elems,
                      const float* cb1p, const void* dwimg, const float* bc, int K, int causal, const float* cln1_w,
                      const float* cln1_b, float ceps1, const float* cb2, const unsigned char* kpm, int H, int act,
                      float slope, const float* g0, const float* b0, float eps0, const float* b1, const float* b2,
                      float alpha, const float* gp, const float* bp, float epsp, const float* gn, const float* bn,
                      float epsn, float* u, const void* img, long long img_elems, void* stream);

/* Weight-stream image of the source Linear of sbk_src_ffn_proj: ws (256, Kin)
 * bf16 as Kin / 64 tiles of 256 rows x 64 k in K order, rows swizzled as in
 * sbk_ffn_image.  Kin % 64 == 0, Kin <= 768 (-1 / SBK_ERR_ARG otherwise). */
long long sbk_src_image_elems(int Kin);
int sbk_src_image(const void* ws, int Kin, void* img, void* stream);

/* sbk_gemm (x = a ws^T + sbias: the src Linear of TransformerASR.py:169-182,
 * a (M, Kin) bf16, simg = sbk_src_image(ws), sbias (256) fp32 or null)
 * followed by sbk_ffn_proj on x in one launch; x never reaches memory.  With
 * rel_len (B floats; M == B * T) the launch also writes the key-padding mask
 * kpm_out (M bytes) exactly as sbk_length_mask; rel_len null: no mask.  M ..
 * yp: as sbk_ffn_proj (np > 0); out must not alias a.  D = 256. */
int sbk_src_ffn_proj(const void* a, int Kin, const void* simg, long long simg_elems, const float* sbias,
                     const float* rel_len, int T, unsigned char* kpm_out, int M, int D, int d_eff, int H,
                     const float* g0, const float* b0, float eps0, const void* img, long long img_elems,
                     const float* b1, int act, float slope, const float* b2, float alpha, const float* gp,
                     const float* bp, float epsp, float* out, const float* gn, const float* bn, float epsn, int np,
                     void* yp, void* stream);

/* LayerNorm (normalization.py:172-223; Conformer.py:178,194,340): one or two
 * chained LayerNorms over rows of x (M, D) fp32, D <= 1024. */
int sbk_layernorm(const float* x, int M, int D, const float* g1, const float* b1, float eps1, void* out1,
                  int out1_bf16, const float* g2, const float* b2, float eps2, void* out2, int out2_bf16,
                  void* stream);

/* ConvolutionModule middle (Conformer.py:106-113): depthwise Conv1d(K) over
 * time (zero pad (K-1)/2, or K-1 left when causal) + bias -> LayerNorm(C)
 * -> Swish.  x (B*T, C) bf16/fp32 -> out (B*T, C). */
int sbk_dwconv_ln_swish(int in_bf16, const void* x, int B, int T, int C, const float* w, const float* bias, int K,
                        int causal, const float* g, const float* beta, float eps, void* out, int out_bf16,
                        void* stream);

/* ConvBlock (convolution.py:169-175 + CNN.py:616-657) with Cin = 1:
 * Conv2d 3x3 stride 2 reflect pad -> LayerNorm(Fout x Cout) -> LeakyReLU.
 * x (B, Tin, Fin) fp32 -> out (B, Tout, Fout, Cout).  x == NULL: shape query. */
int sbk_conv_block_c1(const float* x, int B, int Tin, int Fin, int Cout, const float* w, const float* bias,
                      const float* g, const float* beta, float eps, float slope, void* out, int out_bf16, int* Tout,
                      int* Fout, void* stream);

/* Same block for Cin % 8 == 0 as an MFMA implicit GEMM; wperm (Cout, 3 time,
 * 3 freq, Cin) in the input dtype. */
int sbk_conv_block_mfma(int in_bf16, const void* x, int B, int Tin, int Fin, int Cin, int Cout, const void* wperm,
                        const float* bias, const float* g, const float* beta, float eps, float slope, void* out,
                        int out_bf16, int* Tout, int* Fout, void* stream);

/* ConvolutionFrontEnd with two ConvBlocks in one launch (convolution.py:12-84,
 * 169-175): block 1 (Cin = 1 -> C1 = 64, w1 as sbk_conv_block_c1) feeds block 2
 * (C1 -> C2, wp2 as sbk_conv_block_mfma in the dtype_bf16 type) through LDS;
 * x (B, Tin, Fin) fp32 -> out (B, T2, F2, C2); bf16 compute only (dtype_bf16 = 1), C1 = 64, F1 <= 40, F2 <= 32, C2 <= 32.
 * slot_max (B, nslot) non-null: x is an Fbank output before its top_db floor
 * (sbk_spectrum mode 2's partial maxima) and the floor max_b - top_db is
 * applied as the rows are loaded (features.py:706-711; no separate
 * sbk_topdb_clamp pass).  x == NULL: shape query. */
int sbk_conv_frontend2(int dtype_bf16, const float* x, int B, int Tin, int Fin, const float* w1, const float* b1,
                       const float* g1, const float* be1, float eps1, float slope1, int C1, const void* wp2,
                       const float* b2, const float* g2, const float* be2, float eps2, float slope2, int C2, void* out,
                       int out_bf16, const float* slot_max, int nslot, float top_db, int* Tout, int* Fout,
                       void* stream);

/* fp32 -> bf16 cast (n elements). */
int sbk_cast_bf16(const float* x, void* y, long long n, void* stream);

/* Swish (activations.py:111-142): y = x * sigmoid(beta * x). */
int sbk_swish(const float* x, float* y, long long n, float beta, void* stream);

/* RelPosMHAXL core (attention.py:566-636 incl. rel_shift :468-483):
 * qkv (B*T, 3d) head-interleaved in_proj output, pk (2T-1, d) linear_pos
 * output, pbu/pbv (H*dh) fp32, kpm (B, T) uint8 or null; out (B*T, d);
 * probs (B, H, T, T) fp32 or null.  dh <= 128. */
int sbk_relpos_attention(int dtype_bf16, const void* qkv, const void* pk, const float* pbu, const float* pbv,
                         const uint8_t* kpm, int B, int T, int H, int dh, float scale, void* out, float* probs,
                         void* stream);

/* Same with the positional rows at row stride ldp (>= d): the p_k of every layer
 * can come from ONE linear_pos GEMM over the stacked weights, (2T-1, L*d), layer l
 * at column offset l*d.  bf16, dh == 64, no probs, ldp % 8 == 0, 16-B aligned
 * operands and T <= 4096 take the LDS-DMA kernel (key padding as a per-workgroup
 * chunk bitmap); every other case takes the general kernel.  Same results. */
int sbk_relpos_attention_ld(int dtype_bf16, const void* qkv, const void* pk, int ldp, const float* pbu,
                            const float* pbv, const unsigned char* kpm, int B, int T, int H, int dh, float scale,
                            void* out, float* probs, void* stream);
/* sbk_relpos_attention_ld with an additive fp32 attention mask (attn_mask,
 * attention.py:598-611; bool masks as 0 / -inf): score (b, h, i, j) +=
 * am[b * am_sb + h * am_sh + i * T + j] after the scale, before the key
 * padding and the softmax.  2-D (T, T) mask: am_sb = am_sh = 0; 3-D
 * (B*H, T, T): am_sb = H*T*T, am_sh = T*T.  Probabilities optional. */
int sbk_relpos_attention_mask(int dtype_bf16, const void* qkv, const void* pk, int ldp, const float* pbu,
                              const float* pbv, const unsigned char* kpm, const float* am, long long am_sb,
                              long long am_sh, int B, int T, int H, int dh, float scale, void* out, float* probs,
                              void* stream);
/* Plain scaled dot-product attention over the same head-interleaved qkv
 * (MultiheadAttention, attention.py:642-779: no positional term, no u / v
 * biases): bf16, dh == 64, T <= 4096, 16-B aligned qkv / out; kpm (B, T)
 * uint8 or null; no probabilities.  Equal to sbk_relpos_attention_ld with a
 * zero band and zero biases; SBK_ERR_ARG outside that envelope. */
int sbk_mha_attention(const void* qkv, const unsigned char* kpm, int B, int T, int H, int dh, float scale, void* out,
                      void* stream);
/* LDS bytes one attention workgroup needs (host-side capacity check). */
long long sbk_relpos_attention_lds(int dtype_bf16, int T, int dh);

/* RelPosMHAXL with query != key/value and q_len != k_len (csrc/xattn.hip):
 * the attention core of attention.py:554-639 after the separate q / k / v
 * projections (:554-564), with the reference's rel_shift (:468-483) of a
 * (Lq, P) band (P = pos_embs rows, P//2 + 1 == Lk) and its mask_pos_future
 * tril (:479-481).  q (B*Lq, ldq), k / v (B*Lk, ldk / ldv), pk (P, ldp), head
 * h at columns h*dh; fp32 or bf16 (dtype_bf16).  pbu / pbv (H*dh) fp32; kpm
 * (B, Lk) uint8 or null; am additive fp32 or null, element (b, h, i, j) at
 * am[b*am_sb + h*am_sh + i*Lk + j].  out (B*Lq, ldo) in the input dtype;
 * probs (B, H, Lq, Lk) fp32, the softmax; with p_drop > 0 attn receives the
 * dropped probabilities (the reference's returned weights) and out = attn·V.
 * dh <= 256; Lk, Lq, P within one workgroup's LDS.  pk == NULL: plain scaled
 * dot-product attention (the MultiheadAttention drop-in, attention.py:642-778;
 * torch.nn.MultiheadAttention's core) — no positional term, pbu / pbv and
 * ldp ignored, P only range-checked (>= Lk). */
int sbk_relpos_xattn_fwd(int dtype_bf16, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                         const void* pk, int ldp, int P, const float* pbu, const float* pbv, const unsigned char* kpm,
                         const float* am, long long am_sb, long long am_sh, int B, int Lq, int Lk, int H, int dh,
                         float scale, int mask_pos_future, float p_drop, unsigned long long seed, void* out, int ldo,
                         float* probs, float* attn, void* stream);
/* Its backward from dO (B*Lq, lddo) in the input dtype and the forward's
 * probs / seed: dq (B*Lq, H*dh), dk, dv (B*Lk, H*dh), dpk (P, H*dh) fp32;
 * workspace G (B*H*Lq*Lk) fp32 (score gradients), dqu / dqv (B*Lq, H*dh)
 * fp32 — the content and positional parts of dq, whose column sums are the
 * pos_bias_u / pos_bias_v gradients.  pk == NULL (the forward's no-position
 * mode): the band passes are skipped, dq is written directly, and dqu / dqv /
 * dpk / pbu / pbv may be NULL. */
int sbk_relpos_xattn_bwd(int dtype_bf16, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                         const void* pk, int ldp, int P, const float* pbu, const float* pbv, const float* probs,
                         const void* dO, int lddo, int B, int Lq, int Lk, int H, int dh, float scale,
                         int mask_pos_future, float p_drop, unsigned long long seed, float* G, float* dqu, float* dqv,
                         float* dq, float* dk, float* dv, float* dpk, void* stream);

/* Whole Conformer convolution module in one launch (csrc/convmod.hip; Conformer.py:54-115,254-255),
 * bf16 MFMA: out = x + rowmask0(Linear2(Swish(LN1(dwconv_K(GLU(Linear1(LN0(x))))))));
 * x, out (B*T, 256) fp32, out must not alias x; w1p (512, 256) bf16 rows GLU-permuted in
 * [value16 | gate16] groups (sbk_gemm_glu_group), b1p permuted alike; wc (K, 256) fp32 taps
 * (tap-major: the transpose of Conv1d.weight (256, 1, K)),
 * bc (256) or null; w2 (256, 256) bf16, b2 or null; kpm (B*T) uint8 or null.  K <= 31.
 * d_eff: the LayerNorms' statistics over the first d_eff channels, the rest
 * zero-padded (as sbk_ffn). */
int sbk_conv_module_supported(int D, int K);
int sbk_conv_module(const float* x, float* out, int B, int T, int D, int d_eff, const float* ln0_w, const float* ln0_b,
                    float eps0, const void* w1p, const float* b1p, const float* wc, const float* bc, int K, int causal,
                    const float* ln1_w, const float* ln1_b, float eps1, const void* w2, const float* b2,
                    const unsigned char* kpm, void* stream);
/* sbk_conv_module with the MHSA output projection applied first: the module
 * runs on x_att = x + o wo^T + bo (attention.py:636 out_proj and the residual
 * of Conformer.py:247-252) without x_att leaving the workgroup except as
 * this launch's own output rows: out = x_att + rowmask0(ConvModule(x_att)).
 * o (B*T, 256) bf16 (the attention heads concatenated), wo (256, 256) bf16,
 * bo (256) fp32 or null; o == null behaves as sbk_conv_module. */
int sbk_conv_module_pre(const float* x, const void* o, const void* wo, const float* bo, float* out, int B, int T,
                        int D, int d_eff, const float* ln0_w, const float* ln0_b, float eps0, const void* w1p, const float* b1p,
                        const float* wc, const float* bc, int K, int causal, const float* ln1_w, const float* ln1_b,
                        float eps1, const void* w2, const float* b2, const unsigned char* kpm, void* stream);

/* InputNormalization (processing/features.py:940-1231), csrc/norm.hip.  x (B, T, F) fp32,
 * len (B) relative lengths (frames = rintf(len * T), clamped to [0, T]), F <= 256.
 *   partials: part = sbk_inorm_slices(T) Welford slices per (b, f), 3 doubles each;
 *   stats:    per-utterance mean / unbiased std (>= eps; NaN for <= 1 frame) into mean, std (B, F)
 *             (either may be null); with cur_mean / cur_std (F) also their batch means, and
 *             upd 1: glob = cur, 2: glob = keep * glob + wgt * cur (in place);
 *   apply:    y = (x - mean) / std, per utterance (B, F) or shared (F); y may alias x. */
int sbk_inorm_slices(int T);
int sbk_inorm_partials(const float* x, const float* len, int B, int T, int F, double* part, void* stream);
int sbk_inorm_stats(const double* part, int B, int T, int F, int mean_norm, int std_norm, float eps, float* mean,
                    float* std, float* cur_mean, float* cur_std, int upd, float keep, float wgt, float* glob_mean,
                    float* glob_std, void* stream);
int sbk_inorm_apply(const float* x, int B, int T, int F, const float* mean, const float* std, int per_utt, float* y,
                    void* stream);

/* ------------------------------------------------------------ training path
 * Backward of the Conformer-Transducer encoder (csrc/backward.hip).  The
 * dense contractions of the backward (dX = dY W, dW = dY^T X, attention's
 * batched products) run on sbk_gemm / sbk_gemm_tn{,_f32} / sbk_gemm_batched;
 * these entry points are the element-wise / reduction / layout parts.  *_bf16 flags select bf16 (1)
 * or fp32 (0) storage per operand. */

/* LayerNorm backward over rows of x (M, D) fp32, D <= 16384 (nn.LayerNorm as
 * used by normalization.py:172-223, Conformer.py:178,194,340 and the ConvBlock
 * (freq x channel) norm, convolution.py:169-175):
 *   dx = rstd (dy g - mean(dy g) - xhat mean(dy g xhat)) (+ dres if non-null);
 * part (sbk_layernorm_bwd_blocks(M), 2, D) receives per-block [dgamma | dbeta]
 * partials (reduce with sbk_colsum).  part may be null. */
int sbk_layernorm_bwd_blocks(int M);
int sbk_layernorm_bwd(const float* x, const void* dy, int dy_bf16, int M, int D, const float* g, float eps,
                      const float* dres, float* dx, float* part, void* stream);

/* LayerNorm forward over rows of any width (the ConvBlock norm over freq x
 * channels: a wave per row up to D = 2560, a workgroup per row beyond). */
int sbk_layernorm_wide(const float* x, int M, int D, const float* g, const float* b, float eps, void* y, int y_bf16,
                       void* stream);

/* out[c] (+)= sum_r part[r, c] (deterministic). */
int sbk_colsum(const float* part, int rows, int cols, float* out, int accumulate, void* stream);

/* out[c] (+)= sum_r x[r, c]; part: sbk_rowsum_chunks(rows) * cols floats. (Linear bias gradients.) */
int sbk_rowsum_chunks(long long rows);
/* out[z, c] (+)= sum_r x[z, r, c] for z < batch; part: sbk_rowsum_chunks(rows) * batch * cols floats. */
int sbk_rowsum_batched(const void* x, int x_bf16, int batch, long long rows, int cols, float* part, float* out,
                       int accumulate, void* stream);
int sbk_rowsum(const void* x, int x_bf16, long long rows, int cols, float* part, float* out, int accumulate,
               void* stream);

/* Activations and their backward: mode 1 Swish (activations.py:111-142),
 * 2 GLU over [a | gate] halves of 2*cols inputs (Conformer.py:73-79, nn.GLU(dim=1)),
 * 3 LeakyReLU(slope) (convolution.py:169-175), 4 GELU with the exact erf
 * (torch.nn.GELU, Transformer.py's FFN).  dx has the shape of x. */
int sbk_act_fwd(int mode, const void* x, int x_bf16, long long rows, int cols, void* y, int y_bf16, float slope,
                void* stream);
int sbk_act_bwd(int mode, const void* x, int x_bf16, const void* dy, int dy_bf16, long long rows, int cols, void* dx,
                int dx_bf16, float slope, void* stream);

/* Depthwise Conv1d over time with bias (Conformer.py:80-86,106; zero pad (K-1)/2,
 * or K-1 left when causal): x, y (B*T, C). */
int sbk_dwconv_fwd(const void* x, int x_bf16, int B, int T, int C, const float* w, const float* bias, int K,
                   int causal, void* y, int y_bf16, void* stream);
/* Its backward: dx (optional) and per-chunk partials part (sbk_dwconv_wgrad_chunks(B, T), C, K + 1)
 * of [dw taps | dbias] (reduce with sbk_colsum).  K <= 31. */
int sbk_dwconv_wgrad_chunks(int B, int T);
int sbk_dwconv_bwd(const void* x, int x_bf16, const float* dy, int B, int T, int C, const float* w, int K, int causal,
                   void* dx, int dx_bf16, float* part, void* stream);

/* RelPosMHAXL backward (attention.py:566-633 differentiated).  Every
 * per-(b, h) operand is stored over Tp >= T rows (T rounded up to 8) and
 * dhp >= dh columns, zero-filled, so the MFMA GEMMs' 16-B rows hold for any
 * T and head size; bf16 (dtype_bf16) or fp32 storage.
 *   sbk_attn_prep: qu = q + pos_bias_u, v, doh (B*H, Tp, dhp); kT, vT
 *     (B*H, dhp, Tp); qv = q + pos_bias_v head-major (H, B*T, dhp); pkT
 *     (H, dhp, Wp) from pk (2T-1, ldp), Wp >= 2T-1.  Outputs nullable.
 *   sbk_attn_probs_pad (forward dropout, :626): attn = D P (fp32 (B*H, T, T),
 *     nullable) and Pd = D P over (B*H, Tp, Tp), D = keep / (1 - p) from the
 *     sbk_dropout_add hash of (seed, index into P).
 *   sbk_relpos_softmax_bwd_pad: P (B*H, T, T) fp32, dP = dO V^T (B*H, Tp, Tp):
 *     Pd = D P, dS = scale * P (D dP - rowsum(P D dP)) (B*H, Tp, Tp) and the
 *     pre-rel_shift image dBD (H, B*T, Wp) with dBD[i, T-1-i+j] = dS[i, j]
 *     (:468-483 transposed), zero elsewhere.
 *   sbk_attn_dqkv: dqkv (B*T, H*3*dh) in the in_proj layout from dq_ac, dk,
 *     dv (B*H, Tp, dhp) and dq_bd (H, B*T, dhp), fp32 in; dq = dq_ac + dq_bd. */
int sbk_attn_prep(int dtype_bf16, const void* qkv, const void* dO, const void* pk, int ldp, const float* pbu,
                  const float* pbv, int B, int H, int T, int dh, int Tp, int dhp, int Wp, void* qu, void* qv, void* kT,
                  void* v, void* vT, void* doh, void* pkT, void* stream);
int sbk_attn_probs_pad(const float* P, int BH, int T, int Tp, float p, unsigned long long seed, float* attn, void* Pd,
                       int pd_bf16, void* stream);
int sbk_relpos_softmax_bwd_pad(int dtype_bf16, const float* P, const void* dP, int B, int H, int T, int Tp, int Wp,
                               float scale, float p, unsigned long long seed, void* dS, void* Pd, void* dBD,
                               void* stream);
int sbk_attn_dqkv(const float* dq_ac, const float* dq_bd, const float* dk, const float* dv, int B, int H, int T,
                  int dh, int Tp, int dhp, void* out, int out_bf16, void* stream);

/* Conv2d with "same" reflect padding (CNN.py:616-700, get_padding_elem
 * :1459-1481) as a GEMM, any kernel (kt time x kf freq taps), stride (st,
 * sf) and padding (pt, pf < the input size): x (B, Ti, Fi, Ci) -> col
 * (B*To*Fo, ldcol >= kt*kf*Ci), columns ordered (time tap, freq tap, ci),
 * zero beyond kt*kf*Ci; To = (Ti + 2 pt - kt) / st + 1.  col2im is its
 * adjoint (reflected taps folded back, a deterministic gather), dx
 * (B, Ti, Fi, Ci). */
int sbk_im2col(const void* x, int x_bf16, int B, int Ti, int Fi, int Ci, int kt, int kf, int st, int sf, int pt,
               int pf, int ldcol, void* col, int col_bf16, void* stream);
int sbk_col2im(const void* dcol, int dcol_bf16, int B, int Ti, int Fi, int Ci, int kt, int kf, int st, int sf, int pt,
               int pf, int ldcol, void* dx, int dx_bf16, void* stream);

/* The general Conv2d geometry of the standalone drop-in (CNN.py:556-700):
 * dilation (dt, df), leading pads (pt, pf; the trailing ones follow from the
 * given To, Fo), pad mode 0 reflect, 1 zeros, 2 replicate, 3 circular
 * (F.pad; "same" with any padding_mode, "valid", "causal").  Same col layout
 * as sbk_im2col.  sbk_col2im_x: its adjoint through dxpad, fp32 scratch of
 * B*Tp*Fp*Ci with Tp = (To-1) st + (kt-1) dt + 1, Fp alike (gathered onto
 * the padded grid, then folded onto x in a fixed order: deterministic). */
int sbk_im2col_x(const void* x, int x_bf16, int B, int Ti, int Fi, int Ci, int kt, int kf, int st, int sf, int dt,
                 int df, int pt, int pf, int To, int Fo, int mode, int ldcol, void* col, int col_bf16, void* stream);
int sbk_col2im_x(const void* dcol, int dcol_bf16, int B, int Ti, int Fi, int Ci, int kt, int kf, int st, int sf,
                 int dt, int df, int pt, int pf, int To, int Fo, int mode, int ldcol, float* dxpad, void* dx,
                 int dx_bf16, void* stream);

/* Transducer_joint "sum" (transducer_joint.py:57-95): z[b,t,u,:] = act(tn[b,t,:] + pn[b,u,:]),
 * act 0 none, 3 LeakyReLU(slope), 5 tanh, 6 ReLU; tn (B, T, J), pn (B, U1, J) fp32, z fp32/bf16.
 * Backward: dtn = sum_u dz act', dpn = sum_t dz act' — one pass over dz (block per
 * (b, 16-frame run, 512 columns)), per-run dpn partials in ws
 * (sbk_joint_bwd_workspace_floats floats) reduced deterministically.  Vector paths for J % 4 == 0
 * (fwd) / J % 2 == 0 (bwd), scalar otherwise. */
long long sbk_joint_bwd_workspace_floats(int B, int T, int U1, int J);
int sbk_joint_fwd(const float* tn, const float* pn, int B, int T, int U1, int J, int act, float slope, void* z,
                  int z_bf16, void* stream);
int sbk_joint_bwd(const float* tn, const float* pn, const void* dz, int dz_bf16, int B, int T, int U1, int J, int act,
                  float slope, float* dtn, float* dpn, float* ws, void* stream);

/* Dropout + residual (nn.Dropout before the residual adds of Conformer.py:242-259,
 * attention.py:630, convolution.py:175, TransformerASR custom_src_module):
 *   out = res + alpha * rowmask0(drop_p(x)),  drop_p(x) = keep ? x / (1 - p) : 0,
 * keep drawn from a counter-based hash of (seed, element index), so the backward is
 * the same call on dy with res = null.  res / rowmask may be null; p = 0 skips the draw. */
int sbk_dropout_add(const void* x, int x_bf16, const float* res, long long rows, int cols,
                    const unsigned char* rowmask, float alpha, float p, unsigned long long seed, void* out,
                    int out_bf16, void* stream);

/* Transducer decoding step (decoders/transducer.py:137-377): log-softmax of
 * the joint logits x (R, V) and its top-k per row (ties -> lower index):
 * vals (R, k) = log-probs, idx (R, k) int64.  k = 1 is the greedy max. */
int sbk_logsoftmax_topk(const float* x, long long ldx, int R, int V, int k, float* vals, long long* idx,
                        void* stream);

/* ---- config 5: wav2vec2 latent extractor + TransformerEncoder (MXFP8) ---- */

/* Per-utterance mean / rstd of F.layer_norm(wav, wav.shape[1:]) (wav2vec.py:92-93):
 * stats[2b] = mean, stats[2b+1] = 1/sqrt(var + eps). */
int sbk_w2v_wav_stats(const float* wav, int B, long long S, float eps, float* stats, void* stream);

/* Latent-extractor layer 0 (wav2vec.py:28-88: Conv1d(1 -> C, K, stride, "valid",
 * no bias) -> LayerNorm(C) -> GELU), waveform normalisation (stats, nullable)
 * applied on load.  out (B, T0, C): out_mode 0 fp32, 1 bf16, 2 MXFP8 e4m3 with
 * scales (B*T0, C/32) E8M0 bytes.  C <= 1024, K <= 16. */
int sbk_w2v_conv0(const float* wav, const float* stats, int B, long long S, int T0, int C, int K, int stride,
                  const float* w, const float* g, const float* b, float eps, void* out, int out_mode,
                  uint8_t* scales, void* stream);

/* Row LayerNorm (g non-null; eps) -> activation (0 none, 3 ReLU, 4 GELU) -> fp32 /
 * bf16 / MXFP8 output, one wave per row, D in {64,...,4096} (powers of two).
 * Extractor layers 1..6 after their GEMM; TransformerEncoderLayer norm1/norm2
 * producing the MXFP8 A operands (Transformer.py:321-376).  Other D: fp32 / bf16 only. */
int sbk_ln_act(const void* x, int in_bf16, long long ldx, int M, int D, const float* g, const float* b, float eps,
               int act, void* out, long long ldo, int out_mode, uint8_t* scales, long long lds, void* stream);

/* MXFP8 GEMM C = epi(A W^T) on v_mfma_scale_f32_32x32x64_f8f6f4: A e4m3 (M, K) +
 * E8M0 scales (M, K/32); W e4m3 (N, K) + scales.  Row m of A starts at
 * A + (m / rpb)*a_bs + (m % rpb)*lda (conv rows; rpb >= M for a plain GEMM).
 * Epilogue: + bias, act (0/3/4), alpha*val + res, out fp32 / bf16 / MXFP8 (+scales).
 * K % 128 == 0, N % 128 == 0.  Replaces nn.Linear / Conv1d in
 * Transformer.py:246-376, attention.py:642-839, wav2vec.py:28-88. */
int sbk_mx_gemm(const uint8_t* A, const uint8_t* SA, long long lda, long long ldsa, long long rpb, long long a_bs,
                long long s_bs, const uint8_t* W, const uint8_t* SW, long long ldw, long long ldsw, int M, int N,
                int K, const float* bias, int act, float alpha, const float* res, long long ldr, void* out,
                long long ldc, int out_mode, uint8_t* out_scales, long long ldso, void* stream);

/* sbk_mx_gemm with an fp32 workspace (16-B aligned) for the 256-tile
 * kernel's split-K tail: when the tiles past the last full round of
 * workgroups fill at most half the CUs and K >= 2048, each of them runs as
 * two K halves plus an epilogue pass (config 5's FFN down-projection, 376
 * tiles on 256 CUs).  ws_floats >= sbk_mx_gemm_ws_floats(M, N, K, out_mode)
 * enables it (fp32 out only; 0 = no split at this shape); results equal
 * sbk_mx_gemm's up to the fp32 order of the two halves' sum. */
long long sbk_mx_gemm_ws_floats(int M, int N, int K, int out_mode);
int sbk_mx_gemm_ws(const uint8_t* A, const uint8_t* SA, long long lda, long long ldsa, long long rpb, long long a_bs,
                   long long s_bs, const uint8_t* W, const uint8_t* SW, long long ldw, long long ldsw, int M, int N,
                   int K, const float* bias, int act, float alpha, const float* res, long long ldr, void* out,
                   long long ldc, int out_mode, uint8_t* out_scales, long long ldso, float* ws, long long ws_floats,
                   void* stream);

/* sbk_mx_gemm on the 256 x 256-tile multi-phase kernel (csrc/gemm256.hip):
 * same arguments; N % 256 == 0, K % 128 == 0 (SBK_ERR_ARG otherwise).
 * sbk_mx_gemm takes this kernel by itself when the shape allows and M is
 * large; this entry point forces it. */
int sbk_mx_gemm256(const uint8_t* A, const uint8_t* SA, long long lda, long long ldsa, long long rpb, long long a_bs,
                   long long s_bs, const uint8_t* W, const uint8_t* SW, long long ldw, long long ldsw, int M, int N,
                   int K, const float* bias, int act, float alpha, const float* res, long long ldr, void* out,
                   long long ldc, int out_mode, uint8_t* out_scales, long long ldso, void* stream);

/* x[m, :] += pe[m % T, :] in place, x (M, D) fp32 (EncoderWrapper positional table). */
int sbk_add_rows_periodic(float* x, int M, int D, const float* pe, int T, void* stream);

/* MXFP8 quantisation of a fp32 / bf16 (M, K) matrix, K % 32 == 0 (weights, cached). */
int sbk_mx_quant(const void* x, int in_bf16, long long ldx, int M, int K, uint8_t* q, long long ldq,
                 uint8_t* scales, long long ldsq, void* stream);

/* fp32 value of an MXFP8 matrix (tests). */
int sbk_mx_dequant(const uint8_t* q, long long ldq, const uint8_t* scales, long long ldsq, int M, int K, float* out,
                   void* stream);

/* ------------------------------------------ joint CTC/attention decoding */

/* One step of CTCPrefixScorer.forward_step (decoders/ctc.py:84-243) without
 * its (T, 2, N, C) state tensor.  N = B*beam rows; x (B, T, V) fp32 masked CTC
 * log-probs; r_prev (T, 2, N) fp32; psi_prev (N) fp32 or null (0); last_tok
 * (N) int64, the last token of each row's prefix (null or prefix_len 0: token
 * 0, as the reference); cand (N, C) int64 with 1 <= C <= V, or null with
 * C = 0 for all V tokens; last_frame (B) int32 (a negative index counts from
 * T).  Frames start ... end-1 are walked, 1 <= start <= T, end <= T (start >=
 * end: no frame), T <= 4096.  out (N, V) = psi - psi_prev: the eos column is
 * logaddexp(r_prev[last_frame, 0], r_prev[last_frame, 1]), the blank column
 * and, with cand, every column outside cand are the sentinel -1e20. */
int sbk_ctc_prefix_step(const float* x, const float* r_prev, const float* psi_prev, const long long* last_tok,
                        const long long* cand, const int* last_frame, int B, int beam, int T, int V, int C,
                        int prefix_len, int start, int end, int blank, int eos, float* out, void* stream);

/* CTCPrefixScorer.permute_mem (ctc.py:245-294) from the step's inputs: new
 * row n continues row parent[n] (in [0, N)) with token[n]; r_new (T, 2, N)
 * and psi_new (N) are that pair's forward variables and psi, bit for bit
 * what sbk_ctc_prefix_step scored (one shared device function).  With cand, a
 * token outside its parent's candidates takes the parent's candidate 0 for
 * r_new and the sentinel for psi_new. */
int sbk_ctc_prefix_advance(const float* x, const float* r_prev, const long long* last_tok, const long long* cand,
                           const int* last_frame, const long long* parent, const long long* token, int B, int beam,
                           int T, int V, int C, int prefix_len, int start, int end, int blank, int eos, float* r_new,
                           float* psi_new, void* stream);

/* ctc_greedy_decode (ctc.py:334-376): per frame the argmax over V (lowest
 * index on a tie) of x (B, T, V) fp32 with element strides sb, st, sv, over
 * the first lens[b] frames (int32, clipped to [0, T]); repeats merged, blanks
 * dropped, the rest compacted into tokens (B, T) int32, counts (B) int32. */
int sbk_ctc_greedy_decode(const float* x, long long sb, long long st, long long sv, const int* lens, int B, int T,
                          int V, int blank, int* tokens, int* counts, void* stream);

/* ---- kvdec.hip: incremental transformer decoding (fp32) ----------------- */

/* One decode step of the decoder's masked self-attention over an append-only
 * key/value cache.  q, k_new, v_new: (N, E) views with row stride ld floats
 * (E = H*dh; the three column blocks of one (N, 3E) in_proj output); kc, vc
 * (cap, N, E) position-major; anc (N, anc_ld) int32 ancestry table, values
 * clamped to [0, N), anc[n][L-1] = n; out (N, E).  k_new[n] / v_new[n] are
 * stored into slot [L-1][n] (no other slot is written), then row n attends
 * positions j < L through kc / vc[j][anc[n][j]]: exact softmax, scale
 * 1/sqrt(dh), head h = columns [h*dh, (h+1)*dh).  Needs dh % 4 == 0,
 * dh <= 128, L <= cap, ld >= E, ld % 4 == 0, anc_ld >= L, 16-byte aligned
 * float pointers. */
int sbk_kv_decode_self_attn(const float* q, const float* k_new, const float* v_new, long long ld, float* kc,
                            float* vc, int cap, const int* anc, long long anc_ld, int N, int H, int dh, int L,
                            float* out, void* stream);

/* One decode step of the decoder's cross-attention.  q (N, E) with row stride
 * q_ld; k, v (B, S, E) with row stride kv_ld (the two column blocks of one
 * (B*S, 2E) projection), B = N / group; row n attends utterance n / group,
 * keys j < klen[n] (int32, clamped to 1 .. S; null: all S keys).  out (N, E);
 * probs (N, H, S) or null, 0 at j >= klen.  A workgroup serves one
 * (utterance, head) and reads each K / V row once for up to 16 of its beams.
 * Needs dh % 4 == 0, dh <= 128, N % group == 0, strides >= E and % 4 == 0,
 * 16-byte aligned q / k / v.  Any S (online softmax over 256-key chunks). */
int sbk_kv_decode_cross_attn(const float* q, long long q_ld, const float* k, const float* v, long long kv_ld,
                             const int* klen, int N, int group, int H, int dh, int S, float* out, float* probs,
                             void* stream);

/* sbk_kv_decode_self_attn with a key mask: the decode step of a language
 * model that masks its padding token.  keymask (cap, N) uint8, nonzero =
 * masked; the caller fills slot L-1 before the call.  Row n's key at j < L-1
 * is masked by keymask[j][anc[n][j]], its new key by keymask[L-1][n].  A chunk
 * of 64 positions may be masked whole; a (row, head) whose keys are all
 * masked gets NaN (a softmax over -inf), without a fault.  An all-zero mask
 * gives sbk_kv_decode_self_attn's result bit for bit.  The same requirements,
 * and keymask not null. */
int sbk_kv_decode_self_attn_masked(const float* q, const float* k_new, const float* v_new, long long ld, float* kc,
                                   float* vc, int cap, const int* anc, long long anc_ld,
                                   const unsigned char* keymask, int N, int H, int dh, int L, float* out,
                                   void* stream);

/* ---- lmfuse.hip: the LM-fusion tail of a beam-search step (fp32) -------- */

/* out[n][v] = base[n][v] + w * (logits[n][v]*invT - logsumexp_v(logits[n][:]*invT)),
 * one kernel, the row maximum subtracted.  logits (N, V) with row stride ld;
 * base (N, V) with row stride base_ld, or null (plain scaled log-softmax); out
 * (N, V) contiguous.  -inf / -1e20 entries of base pass through as fp32
 * addition gives them.  Any V >= 1: a row of up to 8192 floats is read from
 * memory once (kept in LDS), a wider one twice.  Needs ld >= V, base_ld >= V. */
int sbk_log_softmax_fuse(const float* logits, long long ld, const float* base, long long base_ld, int N, int V,
                         float invT, float w, float* out, void* stream);

/* ---- w2vloss.hip: the wav2vec 2.0 pre-training objective (fp32) --------- */

/* Contrastive loss forward (losses.py:1198-1251).  x, y (R, C) contiguous.
 * Row r is scored against N + 1 candidates: y[r], then either
 * negs[r*s_row + (j-1)*s_neg ...] (float mode: idx null; strides in floats,
 * unit column stride) or y[idx[r*N + j-1]] (index mode: negs null; idx int32,
 * clamped to [0, R)).  logits (R, N+1) = cos / temp with torch's
 * cosine_similarity formula (eps 1e-8), -inf where a negative equals y[r]
 * element for element; rowloss (R) = logsumexp - logits[:, 0]; correct (R) =
 * 1.0 where candidate 0 is the row maximum; aux (R, 2) = (|x_r|, logsumexp).
 * Any C, N >= 1 with (2*roundup4(C) + N + 17) floats <= 64 KB; 16-byte row
 * loads when C % 4 == 0 and the pointers and strides allow.  R, C, N <= 0,
 * temp <= 0, both or neither of negs / idx: 1001. */
int sbk_w2v_contrast_fwd(const float* x, const float* y, const float* negs, const int* idx, int R, int C, int N,
                         long long s_row, long long s_neg, float temp, float* logits, float* rowloss, float* correct,
                         float* aux, void* stream);

/* Backward wrt x, from the forward's logits and aux; go (R) the gradient of
 * rowloss.  dx (R, C).  Float mode also writes dnegs (R, N, C) — the gradient
 * of candidate j of row r at [r][j-1] — and the positive's term dy (R, C);
 * either may be null.  Index mode writes the per-pair coefficients ca, cb
 * (R, N+1) that sbk_w2v_contrast_bwd_y consumes.  -inf candidates get zeros.
 * Needs (6*roundup4(C) + 16) floats <= 64 KB. */
int sbk_w2v_contrast_bwd_x(const float* x, const float* y, const float* negs, const int* idx, const float* logits,
                           const float* aux, const float* go, int R, int C, int N, long long s_row, long long s_neg,
                           float temp, float* dx, float* dy, float* dnegs, float* ca, float* cb, void* stream);

/* Index mode's dy (R, C): order (R*(N+1)) int64 = the pair ids r*(N+1)+j
 * sorted stably by the row of y they reference (pair (r, 0) references r),
 * offs (R+1) int64 = each row's list start.  A gather per target row in list
 * order: no atomics, bitwise reproducible. */
int sbk_w2v_contrast_bwd_y(const float* x, const float* y, const long long* order, const long long* offs,
                           const float* ca, const float* cb, int R, int C, int N, float* dy, void* stream);

/* Rows of the partial-sum buffer sbk_gumbel_vq_fwd fills (one per wave). */
int sbk_gumbel_vq_parts(int Rq, int G);

/* GumbelVectorQuantizer after the projection (quantisers.py:86-122).  logits
 * (Rq*G, V); gumbels the same shape (training) or null (eval); vars
 * (ncodes = G*V, D).  Writes out (Rq, G*D) = the chosen vars rows side by
 * side; codes (Rq*G) int32 = g*V + chosen index — argmax of logits + gumbels
 * in training, of logits in eval, lowest index on a tie; counts (ncodes)
 * int32, zeroed by the caller, += 1 at g*V + argmax(logits); part
 * (sbk_gumbel_vq_parts, ncodes) partial column sums of softmax(logits), to be
 * summed over rows by the caller; ysoft (Rq*G, V) = softmax((logits +
 * gumbels) / tau) in training, null in eval.  Needs 4*ncodes floats <= 64 KB.
 * G*V != ncodes, a size <= 0, tau <= 0: 1001. */
int sbk_gumbel_vq_fwd(const float* logits, const float* gumbels, float tau, int Rq, int G, int V, const float* vars,
                      int ncodes, int D, float* out, int* codes, int* counts, float* part, float* ysoft, void* stream);

/* Backward.  dout (Rq, G*D); gpsum (ncodes) the gradient of the summed
 * softmax columns; order (Rq*G) int64 = item ids sorted stably by code, offs
 * (ncodes+1) int64.  dlogits (Rq*G, V) = [ysoft given: the straight-through
 * term ysoft*(gy - <gy, ysoft>)/tau, gy[v] = <dout_g, vars[gV+v]>] +
 * p*(gpsum - <p, gpsum>), p = softmax(logits); dvars (ncodes, D) = per code
 * the sum of dout_g over its items in list order. */
int sbk_gumbel_vq_bwd(const float* dout, const float* vars, const float* logits, const float* ysoft,
                      const float* gpsum, float tau, const long long* order, const long long* offs, int Rq, int G,
                      int V, int ncodes, int D, float* dlogits, float* dvars, void* stream);

/* ---- gru.hip: GRU recurrence (nnet/RNN.py:280-388) ---- */

/* The T forward steps of one GRU layer, one launch per step (torch.nn.GRU
 * semantics, gate order r, z, n).  bf16 != 0: w_hh (3H, H) is bf16 and the
 * h_{t-1} operand is rounded to bf16; else fp32 and exact-fp32 MFMA.  The
 * state is fp32 in both.  Input pre-activations: gi (B, T, 3H) fp32 with b_ih
 * already added, or tok (B, T) int32 token ids with table = W_ih^T (I, 3H)
 * fp32 and b_ih (3H) or null — token `blank` adds b_ih only, ids above it
 * read row id - 1.  Exactly one of gi / tok.  b_hh (3H) or null; hx (B, H)
 * or null (zeros); lens (B) int32 = steps per row, or null: a row keeps its
 * state from step lens[b] on and its y rows are zero there.  state (B, T, H)
 * = the carried state after every step; y (B, T, H) or null; save
 * (B, T, 4, H) or null = r, z, n and W_hn h + b_hn for the backward.  Any
 * B, T, H, I >= 1.  A null required pointer, a size <= 0, both or neither of
 * gi / tok: 1001. */
int sbk_gru_fwd(int bf16, const void* w_hh, const float* b_hh, const float* hx, const float* gi, const int* tok,
                int blank, const float* table, int I, const float* b_ih, const int* lens, int B, int T, int H,
                float* state, float* y, float* save, void* stream);

/* The backward steps t = T-1 .. 0 and the carry into dhx, one launch each.
 * w_hhT = W_hh^T (H, 3H) in the compute dtype; hx, state, save, lens as given
 * to / written by sbk_gru_fwd; dy (B, T, H) or null; dhn (B, H) or null.
 * Writes dgi and dgh = (dr, dz, dn * r) (B, T, 3H) fp32, zero past a row's
 * length, and dhx (B, H).  dhw (2, B, H) fp32 is scratch.  No atomics. */
int sbk_gru_bwd(int bf16, const void* w_hhT, const float* hx, const float* state, const float* save, const float* dy,
                const float* dhn, const int* lens, int B, int T, int H, float* dgi, float* dgh, float* dhw,
                float* dhx, void* stream);

/* ---- embedding.hip: Embedding (nnet/embedding.py) ---- */

/* out (N, V-1) fp32: the one-hot rows of ids (N) int32 as Embedding(
 * consider_as_one_hot=True) returns them: a zero row for `blank`, ids above
 * it shifted down by one.  V <= 1 or blank outside [0, V): 1001. */
int sbk_embed_onehot(const int* ids, int N, int V, int blank, float* out, void* stream);

/* out (N, D) fp32 = weight (V, D)[ids (N) int32]; an id outside [0, V) gives a zero row. */
int sbk_embed_gather(const int* ids, const float* weight, int N, int V, int D, float* out, void* stream);

/* out (ncodes, D) fp32 = per-code sums of the rows of src (items, D) fp32.
 * order (items) int64 = row ids sorted stably by code, offs (ncodes+1) int64
 * = the start of every code's run.  Added in list order: no atomics, bitwise
 * reproducible (the Embedding weight gradient; dW_ih of a one-hot GRU input). */
int sbk_segsum_rows(const float* src, const long long* order, const long long* offs, long long items, int ncodes,
                    int D, float* out, void* stream);

/* ---- lstm.hip: LSTM recurrence (nnet/RNN.py:169-277), one or two directions ---- */

/* The T forward launches of one LSTM layer (torch.nn.LSTM semantics, gate
 * order i, f, g, o), D = 1 or 2 directions in the same launches: launch s
 * works on time s in direction 0 and T-1-s in direction 1.  bf16 != 0: w_hh
 * (D, 4H, H) is bf16 and the h operand is rounded to bf16; else fp32 and
 * exact-fp32 MFMA.  The (h, c) state is fp32 in both.  Input
 * pre-activations: gi (B, T, D, 4H) fp32 with b_ih already added, or tok
 * (B, T) int32 token ids with table = the stacked W_ih transposed
 * (I, D, 4H) fp32 and b_ih (D, 4H) or null — token `blank` adds b_ih only,
 * ids above it read row id - 1.  Exactly one of gi / tok.  b_hh (D, 4H) or
 * null; hx, cx (D, B, H) or null (zeros); lens (B) int32 = steps per row, or
 * null: a row keeps (h, c) at every t >= lens[b] and its y rows are zero
 * there, so the reverse direction carries (hx, cx) through the padding.
 * hstate, cstate (B, T, D*H) = the carried state after every step; y
 * (B, T, D*H) or null; save (B, T, D, 4H) or null = i, f, g, o for the
 * backward.  Any B, T, H, I >= 1.  A null required pointer, a size <= 0, D
 * outside {1, 2}, both or neither of gi / tok, D*4*H*H or 4*B*T*D past
 * int32: 1001. */
int sbk_lstm_fwd(int bf16, int D, const void* w_hh, const float* b_hh, const float* hx, const float* cx,
                 const float* gi, const int* tok, int blank, const float* table, int I, const float* b_ih,
                 const int* lens, int B, int T, int H, float* hstate, float* cstate, float* y, float* save,
                 void* stream);

/* The T backward launches (order mirrored per direction) and one more for
 * the carry into dhx, dcx.  w_hhT = W_hh^T per direction (D, H, 4H) in the
 * compute dtype; cx, cstate, save, lens as given to / written by
 * sbk_lstm_fwd; dy (B, T, D*H) or null; dhn, dcn (D, B, H) or null.  Writes
 * dG (B, T, D, 4H) fp32 — the gradient of the gate pre-activations, of gi and
 * of the recurrent product alike, zero past a row's length — and dhx, dcx
 * (D, B, H).  dw (2, 2, D, B, H) fp32 is scratch.  No atomics. */
int sbk_lstm_bwd(int bf16, int D, const void* w_hhT, const float* cx, const float* cstate, const float* save,
                 const float* dy, const float* dhn, const float* dcn, const int* lens, int B, int T, int H,
                 float* dG, float* dw, float* dhx, float* dcx, void* stream);

/* ---- ligru.hip: LiGRU recurrence (nnet/RNN.py:961-1325), one or two directions ---- */

/* The T forward launches of one LiGRU layer:
 *   gates = wn[:, t] + h U^T;  a, zpre = the halves of gates;  z = sigmoid(zpre)
 *   h' = z * h + (1 - z) * act(a) * mask[row]
 * D = 1 or 2 directions in the same launches, sharing u: launch s works on
 * frame s in direction 0 and T-1-s in direction 1, and both read the same
 * raw[b, t].  bf16 != 0: u (2H, H) is bf16 and the h operand is rounded to
 * bf16; else fp32 and exact-fp32 MFMA.  The state is fp32 in both.  raw
 * (B, T, 2H) fp32 is the input projection before normalisation; the epilogue
 * forms wn = (raw - mu[row]) * rs[row] * cscale[col] + cshift[col] with mu, rs
 * (B*T) both given or both null and cscale, cshift (2H) each or null.  hx
 * (D, B, H) or null (zeros); mask (D, B, H) or null (ones).  act: 0 ReLU,
 * 1 LeakyReLU(0.01), 2 tanh, 3 sin.  out (B, T, D*H) = h after every step;
 * save (B, T, D, 2H) or null = a, z for the backward.  Any B, T, H >= 1.  A
 * null required pointer, one of mu / rs without the other, a size <= 0, D
 * outside {1, 2}, act outside 0..3, 2*H*H or 4*B*T*D past int32: 1001. */
int sbk_ligru_fwd(int bf16, int D, int act, const void* u, const float* hx, const float* raw, const float* mu,
                  const float* rs, const float* cscale, const float* cshift, const float* mask, int B, int T, int H,
                  float* out, float* save, void* stream);

/* The T backward launches (order mirrored per direction) and one more for
 * the carry into dhx.  uT = U^T (H, 2H) in the compute dtype; hx, mask, out,
 * save as given to / written by sbk_ligru_fwd; dy (B, T, D*H) or null.
 * Writes dG (B, T, D, 2H) fp32 at true frame positions — the gradient of
 * the gate pre-activations; the gradient of wn is the sum over D — and dhx
 * (D, B, H).  dhw (2, D, B, H) fp32 is scratch.  No atomics. */
int sbk_ligru_bwd(int bf16, int D, int act, const void* uT, const float* hx, const float* out, const float* save,
                  const float* mask, const float* dy, int B, int T, int H, float* dG, float* dhw, float* dhx,
                  void* stream);

/* ------------------------------------------- time-domain augmentation */

/* csrc/tdaug.hip: the waveform stage of the reference's
 * TimeDomainSpecAugment (processing/speech_augmentation.py:435-1173).  All
 * waveforms fp32; tables int32 / fp32 device arrays computed by the caller.
 * Limits (SBK_ERR_ARG beyond them, before any launch): B <= 65535,
 * L <= 128, L * W <= 2048, S <= 64, T * C and T_out * C within int32. */

/* Output elements one workgroup of these kernels owns. */
int sbk_tdaug_tile(void);

/* Polyphase resampler: y (B, T_out, C) from x (B, T, C), channels fastest.
 * first (L), w (L, W): y[k L + i] = sum_j w[i][j] x[first[i] + k M + j], x
 * zero outside [0, T), j ascending, for every k L + i < T_out. */
int sbk_resample(const float* x, int B, int T, int C, const int* first, const float* w, int L, int M, int W,
                 int T_out, float* y, void* stream);

/* y (B, T): y[t] = sum_k taps[k] x[t + k - 50] (a correlation with zero
 * padding), taps (101), k ascending. */
int sbk_fir101(const float* x, int B, int T, const float* taps, float* y, void* stream);

/* y (B, T, C) = x with the samples of segs (B, S, 2) [start, end) zeroed
 * (an empty segment pads a row).  With noise (n_noise uniform draws) segment
 * j of row b is filled with 2 nm u - nm instead, u = noise[noff[b][j] + t -
 * start], nm = 2 amp_b noise_factor, amp_b = sum_t |x[b, t]| / lengths[b]
 * over all T; overlapping segments: the last wins.  That path needs C == 1,
 * noff (B, S), lengths (B), and the scratch partial (B, 64) and amp (B),
 * which receives amp_b (a row reduction launched before the fill). */
int sbk_drop_chunks(const float* x, int B, int T, int C, const int* segs, int S, const int* noff, const float* noise,
                    long long n_noise, const int* lengths, float noise_factor, float* partial, float* amp, float* y,
                    void* stream);

/* One launch for resample -> filter -> zero fill of x (B, T) into y
 * (B, T_out), bit-identical to the three entry points above in sequence
 * (the filter sees the resampled signal zero-padded, not extrapolated).
 * first == null: no resample (T_out == T); taps == null: no filter;
 * S == 0: no segments; none of them: a copy. */
int sbk_tdaug(const float* x, int B, int T, const int* first, const float* w, int L, int M, int W, int T_out,
              const float* taps, const int* segs, int S, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SBK_H */
