"""torch.library custom ops over the sbk C ABI.

Every op launches hand-written HIP kernels (libsbk.so) on the current stream
of the input's device; none has a CPU or eager-PyTorch implementation.  The
`register_fake` rules only describe output shapes, so modules stay
traceable (torch.jit.trace / torch.compile graph capture) as the reference's
tests require (tests/unittests/test_features.py:14,39,56,66,97,107).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, custom_op, ptr, require_device, stream_of

_f32 = torch.float32


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------
# spectral front-end
# ---------------------------------------------------------------------------

PAD_MODES = {"constant": 0, "reflect": 1, "replicate": 2, "circular": 3}


def n_frames(S, n_fft, hop, center):
    pad = n_fft // 2 if center else 0
    return 1 + (S + 2 * pad - n_fft) // hop


@custom_op("sbk::stft", mutates_args=())
def stft(x: torch.Tensor, window: torch.Tensor, tw_nc: torch.Tensor, tw_nfft: torch.Tensor,
         n_fft: int, hop: int, center: bool, pad_mode: int, onesided: bool, normalized: bool) -> torch.Tensor:
    """torch.stft(return_complex=False) layout (features.py:161-183):
    (B,S)->(B,T,F,2); (B,S,C)->(B,T,F,2,C)."""
    require_device(x, window, tw_nc, tw_nfft)
    x = _c(x.to(_f32))
    B, S = x.shape[0], x.shape[1]
    C = x.shape[2] if x.dim() == 3 else 1
    T = n_frames(S, n_fft, hop, center)
    Fo = n_fft // 2 + 1 if onesided else n_fft
    if x.dim() == 3:
        out = torch.empty(B, T, Fo, 2, C, device=x.device, dtype=_f32)
        strides = [T * Fo * 2 * C, 1, Fo * 2 * C, 2 * C, C]
    else:
        out = torch.empty(B, T, Fo, 2, device=x.device, dtype=_f32)
        strides = [T * Fo * 2, 0, Fo * 2, 2, 1]
    st = np.array(strides, dtype=np.int64)
    st_p = st.ctypes.data_as(ctypes.c_void_p)
    scale = float(n_fft) ** -0.5 if normalized else 1.0
    rc = _lib.lib().sbk_spectrum(0, ptr(x), B, S, C, n_fft, hop, int(center), pad_mode, T, ptr(window),
                                 ptr(tw_nc), ptr(tw_nfft), int(onesided), scale, 1.0, 0.0, 0, st_p,
                                 None, None, None, None, 0, 0, 0, 0.0, 0.0, 0.0, ptr(out), None, stream_of(x))
    check(rc, "sbk_spectrum(stft)")
    return out


@stft.register_fake
def _(x, window, tw_nc, tw_nfft, n_fft, hop, center, pad_mode, onesided, normalized):
    T = n_frames(x.shape[1], n_fft, hop, center)
    Fo = n_fft // 2 + 1 if onesided else n_fft
    if x.dim() == 3:
        return x.new_empty(x.shape[0], T, Fo, 2, x.shape[2])
    return x.new_empty(x.shape[0], T, Fo, 2)


def _spec_strides(t):
    """(batch, channel, frame, bin, re/im) element strides of a (B,T,F,2) or
    (B,T,F,2,C) tensor as a host int64 array (kept alive by the caller)."""
    s = t.stride()
    return np.array([s[0], s[4] if t.dim() == 5 else 0, s[1], s[2], s[3]], dtype=np.int64)


def _overlap_add(spec, window, tw_nc, tw_nfft, n_fft, hop, fold, sc_edge, sc_int, envelope, start, length):
    """sbk_istft on a spectrum in its own layout (any strides, no copy):
    (B,T,F,2)->(B,length); (B,T,F,2,C)->(B,length,C)."""
    require_device(spec, window, tw_nc, tw_nfft)
    if spec.dim() not in (4, 5) or spec.shape[3] != 2:
        raise ValueError(f"expected a (B,T,F,2) or (B,T,F,2,C) spectrum, got {tuple(spec.shape)}")
    spec = spec.to(_f32)
    B, T = spec.shape[0], spec.shape[1]
    C = spec.shape[4] if spec.dim() == 5 else 1
    out = torch.empty((B, length, C) if spec.dim() == 5 else (B, length), device=spec.device, dtype=_f32)
    st = _spec_strides(spec)
    rc = _lib.lib().sbk_istft(ptr(spec), st.ctypes.data_as(ctypes.c_void_p), B, C, T, n_fft, hop, int(fold),
                              sc_edge, sc_int, int(envelope), start, length, ptr(window), ptr(tw_nc), ptr(tw_nfft),
                              ptr(out), stream_of(spec))
    check(rc, "sbk_istft")
    return out


def _istft_scale(n_fft, normalized):
    return (float(n_fft) ** -0.5) if normalized else 1.0 / n_fft


@custom_op("sbk::istft", mutates_args=())
def istft(x: torch.Tensor, window: torch.Tensor, tw_nc: torch.Tensor, tw_nfft: torch.Tensor,
          n_fft: int, hop: int, center: bool, onesided: bool, normalized: bool, length: int) -> torch.Tensor:
    """torch.istft on the STFT layout (features.py:273-324): (B,T,F,2)->(B,length),
    (B,T,F,2,C)->(B,length,C); only bins 0..n_fft/2 are read.  The caller
    (ISTFT.forward) has checked the window envelope over the returned range."""
    if x.dim() in (4, 5) and x.shape[2] != (n_fft // 2 + 1 if onesided else n_fft):
        raise ValueError(f"expected {n_fft // 2 + 1 if onesided else n_fft} bins, got {x.shape[2]}")
    sc = _istft_scale(n_fft, normalized)
    return _overlap_add(x, window, tw_nc, tw_nfft, n_fft, hop, False, sc, sc, True,
                        n_fft // 2 if center else 0, length)


@istft.register_fake
def _(x, window, tw_nc, tw_nfft, n_fft, hop, center, onesided, normalized, length):
    return x.new_empty((x.shape[0], length, x.shape[4]) if x.dim() == 5 else (x.shape[0], length))


@custom_op("sbk::istft_bwd", mutates_args=())
def istft_bwd(dy: torch.Tensor, window: torch.Tensor, tw_nc: torch.Tensor, tw_nfft: torch.Tensor, T: int, Fo: int,
              n_fft: int, hop: int, center: bool, normalized: bool) -> torch.Tensor:
    """Gradient of sbk::istft with respect to the spectrum: dy (B,L) or
    (B,L,C) -> (B,T,Fo,2[,C]); exact zeros in the imaginary parts of DC and
    Nyquist and in every bin above n_fft/2."""
    require_device(dy, window, tw_nc, tw_nfft)
    dy = _c(dy.to(_f32))
    B, L = dy.shape[0], dy.shape[1]
    C = dy.shape[2] if dy.dim() == 3 else 1
    out = torch.empty((B, T, Fo, 2, C) if dy.dim() == 3 else (B, T, Fo, 2), device=dy.device, dtype=_f32)
    st = _spec_strides(out)
    rc = _lib.lib().sbk_istft_bwd(ptr(dy), B, C, T, n_fft, hop, _istft_scale(n_fft, normalized),
                                  n_fft // 2 if center else 0, L, ptr(window), ptr(tw_nc), ptr(tw_nfft), Fo,
                                  st.ctypes.data_as(ctypes.c_void_p), ptr(out), stream_of(dy))
    check(rc, "sbk_istft_bwd")
    return out


@istft_bwd.register_fake
def _(dy, window, tw_nc, tw_nfft, T, Fo, n_fft, hop, center, normalized):
    return dy.new_empty((dy.shape[0], T, Fo, 2, dy.shape[2]) if dy.dim() == 3 else (dy.shape[0], T, Fo, 2))


def _istft_setup(ctx, inputs, output):
    x, window, tw_nc, tw_nfft, n_fft, hop, center, onesided, normalized, length = inputs
    ctx.save_for_backward(window, tw_nc, tw_nfft)
    ctx.args = (x.shape[1], x.shape[2], n_fft, hop, center, normalized)


def _istft_backward(ctx, grad):
    return (istft_bwd(grad, *ctx.saved_tensors, *ctx.args),) + (None,) * 9


istft.register_autograd(_istft_backward, setup_context=_istft_setup)


@custom_op("sbk::stft_bwd", mutates_args=())
def stft_bwd(g: torch.Tensor, window: torch.Tensor, tw_nc: torch.Tensor, tw_nfft: torch.Tensor, S: int,
             n_fft: int, hop: int, center: bool, pad_mode: int, onesided: bool, normalized: bool) -> torch.Tensor:
    """Gradient of sbk::stft with respect to the waveform: g (B,T,F,2[,C]) ->
    (B,S[,C]).  The synthesis kernel in its adjoint role (bin weights ½ on
    the interior bins, a two-sided gradient folded on load, no envelope)
    writes the padded axis; the `center` padding (n_fft/2 samples at each
    end) is folded back with slice ops."""
    pad = n_fft // 2 if center else 0
    sc = float(n_fft) ** -0.5 if normalized else 1.0
    d = _overlap_add(g, window, tw_nc, tw_nfft, n_fft, hop, not onesided, sc, 0.5 * sc, False, 0, S + 2 * pad)
    if not pad:
        return d
    dx = d[:, pad:pad + S].clone()
    lo, hi = d[:, :pad], d[:, pad + S:]
    if pad_mode == PAD_MODES["reflect"]:  # padded[i] = x[pad - i]; padded[pad + S + i] = x[S - 2 - i]
        dx[:, 1:pad + 1] += lo.flip(1)
        dx[:, S - 1 - pad:S - 1] += hi.flip(1)
    elif pad_mode == PAD_MODES["replicate"]:
        dx[:, 0] += lo.sum(1)
        dx[:, S - 1] += hi.sum(1)
    elif pad_mode == PAD_MODES["circular"]:  # padded[i] = x[S - pad + i]; padded[pad + S + i] = x[i]
        dx[:, S - pad:] += lo
        dx[:, :pad] += hi
    return dx


@stft_bwd.register_fake
def _(g, window, tw_nc, tw_nfft, S, n_fft, hop, center, pad_mode, onesided, normalized):
    return g.new_empty((g.shape[0], S, g.shape[4]) if g.dim() == 5 else (g.shape[0], S))


def _stft_setup(ctx, inputs, output):
    x, window, tw_nc, tw_nfft, n_fft, hop, center, pad_mode, onesided, normalized = inputs
    if center and pad_mode in (PAD_MODES["reflect"], PAD_MODES["circular"]) and \
            n_fft // 2 > x.shape[1] - (pad_mode == PAD_MODES["reflect"]):
        raise ValueError("STFT backward: the center padding wraps more than once (n_fft/2 exceeds the signal)")
    ctx.save_for_backward(window, tw_nc, tw_nfft)
    ctx.args = (x.shape[1], n_fft, hop, center, pad_mode, onesided, normalized)


def _stft_backward(ctx, grad):
    return (stft_bwd(grad, *ctx.saved_tensors, *ctx.args),) + (None,) * 9


stft.register_autograd(_stft_backward, setup_context=_stft_setup)


@custom_op("sbk::power_spectrum", mutates_args=())
def power_spectrum(x: torch.Tensor, window: torch.Tensor, tw_nc: torch.Tensor, tw_nfft: torch.Tensor,
                   n_fft: int, hop: int, center: bool, pad_mode: int, normalized: bool,
                   power: float, eps: float, log_mag: bool) -> torch.Tensor:
    """Fused STFT → spectral_magnitude for mono (B,S) input → (B,T,F)."""
    require_device(x, window, tw_nc, tw_nfft)
    x = _c(x.to(_f32))
    B, S = x.shape
    T = n_frames(S, n_fft, hop, center)
    Fo = n_fft // 2 + 1
    out = torch.empty(B, T, Fo, device=x.device, dtype=_f32)
    st = np.array([T * Fo, 0, Fo, 1, 0], dtype=np.int64)
    scale = float(n_fft) ** -0.5 if normalized else 1.0
    rc = _lib.lib().sbk_spectrum(1, ptr(x), B, S, 1, n_fft, hop, int(center), pad_mode, T, ptr(window),
                                 ptr(tw_nc), ptr(tw_nfft), 1, scale, float(power), float(eps), int(log_mag),
                                 st.ctypes.data_as(ctypes.c_void_p), None, None, None, None, 0, 0, 0, 0.0, 0.0,
                                 0.0, ptr(out), None, stream_of(x))
    check(rc, "sbk_spectrum(power)")
    return out


@power_spectrum.register_fake
def _(x, window, tw_nc, tw_nfft, n_fft, hop, center, pad_mode, normalized, power, eps, log_mag):
    return x.new_empty(x.shape[0], n_frames(x.shape[1], n_fft, hop, center), n_fft // 2 + 1)


@custom_op("sbk::fbank", mutates_args=())
def fbank(x: torch.Tensor, window: torch.Tensor, tw_nc: torch.Tensor, tw_nfft: torch.Tensor,
          mel_start: torch.Tensor, mel_len: torch.Tensor, mel_off: torch.Tensor, mel_w: torch.Tensor,
          n_fft: int, hop: int, center: bool, pad_mode: int, n_mels: int, log_mel: bool,
          multiplier: float, db_offset: float, amin: float, top_db: float) -> torch.Tensor:
    """Fused Fbank: wav (B,S) → STFT → |X|^2 → mel → dB → top_db (B,T,M).
    lobes/features.py:130-147 with processing/features.py:133-188,327-356,490-560,691-712."""
    require_device(x, window, tw_nc, tw_nfft, mel_start, mel_len, mel_off, mel_w)
    x = _c(x.to(_f32))
    B, S = x.shape
    T = n_frames(S, n_fft, hop, center)
    out = torch.empty(B, T, n_mels, device=x.device, dtype=_f32)
    L = _lib.lib()
    nslot = L.sbk_spectrum_slots(n_fft, hop, T, n_mels, mel_w.numel())
    slot_max = torch.empty(B, max(nslot, 1), device=x.device, dtype=_f32)
    s = stream_of(x)
    rc = L.sbk_spectrum(2, ptr(x), B, S, 1, n_fft, hop, int(center), pad_mode, T, ptr(window), ptr(tw_nc),
                        ptr(tw_nfft), 1, 1.0, 1.0, 0.0, 0, None, ptr(mel_start), ptr(mel_len), ptr(mel_off),
                        ptr(mel_w), mel_w.numel(), n_mels, int(log_mel), multiplier, db_offset, amin, ptr(out),
                        ptr(slot_max), s)
    check(rc, "sbk_spectrum(fbank)")
    if log_mel:
        check(L.sbk_topdb_clamp(ptr(out), ptr(slot_max), nslot, T * n_mels, B, top_db, s), "sbk_topdb_clamp")
    return out


@fbank.register_fake
def _(x, window, tw_nc, tw_nfft, mel_start, mel_len, mel_off, mel_w, n_fft, hop, center, pad_mode, n_mels,
      log_mel, multiplier, db_offset, amin, top_db):
    return x.new_empty(x.shape[0], n_frames(x.shape[1], n_fft, hop, center), n_mels)


@custom_op("sbk::fbank_deferred", mutates_args=())
def fbank_deferred(x: torch.Tensor, window: torch.Tensor, tw_nc: torch.Tensor, tw_nfft: torch.Tensor,
                   mel_start: torch.Tensor, mel_len: torch.Tensor, mel_off: torch.Tensor, mel_w: torch.Tensor,
                   n_fft: int, hop: int, center: bool, pad_mode: int, n_mels: int, multiplier: float,
                   db_offset: float, amin: float) -> tuple[torch.Tensor, torch.Tensor]:
    """fbank (log_mel) WITHOUT the top_db floor: (dB features (B,T,M), the
    per-workgroup partial maxima (B, nslot)).  The consumer applies
    max(x, max_b - top_db) as it loads the rows (sbk_conv_frontend2), so the
    clamp pass over the features never runs; features.py:691-712 otherwise."""
    require_device(x, window, tw_nc, tw_nfft, mel_start, mel_len, mel_off, mel_w)
    x = _c(x.to(_f32))
    B, S = x.shape
    T = n_frames(S, n_fft, hop, center)
    out = torch.empty(B, T, n_mels, device=x.device, dtype=_f32)
    L = _lib.lib()
    nslot = L.sbk_spectrum_slots(n_fft, hop, T, n_mels, mel_w.numel())
    slot_max = torch.empty(B, max(nslot, 1), device=x.device, dtype=_f32)
    rc = L.sbk_spectrum(2, ptr(x), B, S, 1, n_fft, hop, int(center), pad_mode, T, ptr(window), ptr(tw_nc),
                        ptr(tw_nfft), 1, 1.0, 1.0, 0.0, 0, None, ptr(mel_start), ptr(mel_len), ptr(mel_off),
                        ptr(mel_w), mel_w.numel(), n_mels, 1, multiplier, db_offset, amin, ptr(out),
                        ptr(slot_max), stream_of(x))
    check(rc, "sbk_spectrum(fbank)")
    return out, slot_max


@fbank_deferred.register_fake
def _(x, window, tw_nc, tw_nfft, mel_start, mel_len, mel_off, mel_w, n_fft, hop, center, pad_mode, n_mels,
      multiplier, db_offset, amin):
    B = x.shape[0]
    T = n_frames(x.shape[1], n_fft, hop, center)
    nslot = _lib.lib().sbk_spectrum_slots(n_fft, hop, T, n_mels, mel_w.numel())
    return x.new_empty(B, T, n_mels), x.new_empty(B, max(nslot, 1))


@custom_op("sbk::topdb_clamp", mutates_args=())
def topdb_clamp(x: torch.Tensor, slot_max: torch.Tensor, top_db: float) -> torch.Tensor:
    """max(x, max_b - top_db) per sequence b of fbank_deferred's output
    (features.py:706-711), into a new tensor."""
    require_device(x, slot_max)
    y = _c(x.to(_f32)).clone()
    B = y.shape[0]
    check(_lib.lib().sbk_topdb_clamp(ptr(y), ptr(slot_max), slot_max.shape[1], y.numel() // B, B, float(top_db),
                                     stream_of(y)), "sbk_topdb_clamp")
    return y


@topdb_clamp.register_fake
def _(x, slot_max, top_db):
    return torch.empty_like(x, dtype=_f32)


@custom_op("sbk::filterbank", mutates_args=())
def filterbank(spec: torch.Tensor, mel_start: torch.Tensor, mel_len: torch.Tensor, mel_off: torch.Tensor,
               mel_w: torch.Tensor, n_mels: int, log_mel: bool, multiplier: float, db_offset: float,
               amin: float, top_db: float) -> torch.Tensor:
    """Filterbank.forward on a (N,T,F) spectrogram (features.py:490-560)."""
    require_device(spec, mel_start, mel_len, mel_off, mel_w)
    spec = _c(spec.to(_f32))
    N, T, Fd = spec.shape
    out = torch.empty(N, T, n_mels, device=spec.device, dtype=_f32)
    L = _lib.lib()
    nslot = L.sbk_filterbank_slots(T, Fd)
    slot_max = torch.empty(N, max(nslot, 1), device=spec.device, dtype=_f32)
    s = stream_of(spec)
    rc = L.sbk_filterbank(ptr(spec), N, T, Fd, ptr(mel_start), ptr(mel_len), ptr(mel_off), ptr(mel_w), None,
                          n_mels, int(log_mel), multiplier, db_offset, amin, ptr(out), ptr(slot_max), s)
    check(rc, "sbk_filterbank")
    if log_mel:
        check(L.sbk_topdb_clamp(ptr(out), ptr(slot_max), nslot, T * n_mels, N, top_db, s), "sbk_topdb_clamp")
    return out


@filterbank.register_fake
def _(spec, mel_start, mel_len, mel_off, mel_w, n_mels, log_mel, multiplier, db_offset, amin, top_db):
    return spec.new_empty(spec.shape[0], spec.shape[1], n_mels)


@custom_op("sbk::filterbank_dense", mutates_args=())
def filterbank_dense(spec: torch.Tensor, mat: torch.Tensor, log_mel: bool, multiplier: float,
                     db_offset: float, amin: float, top_db: float) -> torch.Tensor:
    """Filterbank with a dense (F, M) matrix (learnable filters, freeze=False)."""
    require_device(spec, mat)
    spec = _c(spec.to(_f32))
    mat = _c(mat.to(_f32))
    N, T, Fd = spec.shape
    M = mat.shape[1]
    out = torch.empty(N, T, M, device=spec.device, dtype=_f32)
    L = _lib.lib()
    nslot = L.sbk_filterbank_slots(T, Fd)
    slot_max = torch.empty(N, max(nslot, 1), device=spec.device, dtype=_f32)
    s = stream_of(spec)
    rc = L.sbk_filterbank(ptr(spec), N, T, Fd, None, None, None, None, ptr(mat), M, int(log_mel), multiplier,
                          db_offset, amin, ptr(out), ptr(slot_max), s)
    check(rc, "sbk_filterbank(dense)")
    if log_mel:
        check(L.sbk_topdb_clamp(ptr(out), ptr(slot_max), nslot, T * M, N, top_db, s), "sbk_topdb_clamp")
    return out


@filterbank_dense.register_fake
def _(spec, mat, log_mel, multiplier, db_offset, amin, top_db):
    return spec.new_empty(spec.shape[0], spec.shape[1], mat.shape[1])


@custom_op("sbk::magnitude", mutates_args=())
def magnitude(x: torch.Tensor, power: float, eps: float, log_mag: bool) -> torch.Tensor:
    """spectral_magnitude: reduce the last axis by sum of squares (features.py:347-356)."""
    require_device(x)
    x = _c(x.to(_f32))
    L = x.shape[-1]
    out = torch.empty(x.shape[:-1], device=x.device, dtype=_f32)
    n = out.numel()
    check(_lib.lib().sbk_magnitude(ptr(x), ptr(out), n, L, float(power), float(eps), int(log_mag),
                                   stream_of(x)), "sbk_magnitude")
    return out


@magnitude.register_fake
def _(x, power, eps, log_mag):
    return x.new_empty(x.shape[:-1])


@custom_op("sbk::dct", mutates_args=())
def dct(x: torch.Tensor, mat: torch.Tensor) -> torch.Tensor:
    """x (..., n_in) @ mat (n_in, n_out) (features.py:765-786)."""
    require_device(x, mat)
    x = _c(x.to(_f32))
    mat = _c(mat.to(_f32))
    n_in, n_out = mat.shape
    out = torch.empty(*x.shape[:-1], n_out, device=x.device, dtype=_f32)
    rows = x.numel() // n_in
    check(_lib.lib().sbk_dct(ptr(x), ptr(mat), ptr(out), rows, n_in, n_out, stream_of(x)), "sbk_dct")
    return out


@dct.register_fake
def _(x, mat):
    return x.new_empty(*x.shape[:-1], mat.shape[1])


@custom_op("sbk::deltas", mutates_args=())
def deltas(x: torch.Tensor, window_length: int, concat: bool) -> torch.Tensor:
    """Deltas along dim 1 of (N,T,F) (features.py:829-852); concat=True
    returns [x | Δx | ΔΔx] in one pass (lobes/features.py:141-144)."""
    require_device(x)
    x = _c(x.to(_f32))
    N, T, Fd = x.shape
    out = torch.empty(N, T, 3 * Fd if concat else Fd, device=x.device, dtype=_f32)
    check(_lib.lib().sbk_deltas(ptr(x), ptr(out), N, T, Fd, window_length, int(concat), stream_of(x)),
          "sbk_deltas")
    return out


@deltas.register_fake
def _(x, window_length, concat):
    return x.new_empty(x.shape[0], x.shape[1], 3 * x.shape[2] if concat else x.shape[2])


@custom_op("sbk::deltas_floor", mutates_args=())
def deltas_floor(x: torch.Tensor, window_length: int, slot_max: torch.Tensor, top_db: float) -> torch.Tensor:
    """[max(x, max_b - top_db) | Δ | ΔΔ] of fbank_deferred's output: the
    top_db floor (features.py:706-711) applied as the concat deltas kernel
    loads its rows (lobes/features.py:141-144), no clamp pass."""
    require_device(x, slot_max)
    x = _c(x.to(_f32))
    N, T, Fd = x.shape
    out = torch.empty(N, T, 3 * Fd, device=x.device, dtype=_f32)
    check(_lib.lib().sbk_deltas_floor(ptr(x), ptr(out), N, T, Fd, window_length, ptr(slot_max), slot_max.shape[1],
                                      float(top_db), stream_of(x)), "sbk_deltas_floor")
    return out


@deltas_floor.register_fake
def _(x, window_length, slot_max, top_db):
    return x.new_empty(x.shape[0], x.shape[1], 3 * x.shape[2])


@custom_op("sbk::context_window", mutates_args=())
def context_window(x: torch.Tensor, left: int, right: int) -> torch.Tensor:
    """ContextWindow on (N,T,F) → (N,T,F·(l+r+1)) (features.py:917-937)."""
    require_device(x)
    x = _c(x.to(_f32))
    N, T, Fd = x.shape
    out = torch.empty(N, T, Fd * (left + right + 1), device=x.device, dtype=_f32)
    check(_lib.lib().sbk_context_window(ptr(x), ptr(out), N, T, Fd, left, right, stream_of(x)),
          "sbk_context_window")
    return out


@context_window.register_fake
def _(x, left, right):
    return x.new_empty(x.shape[0], x.shape[1], x.shape[2] * (left + right + 1))


# ---------------------------------------------------------------------------
# autograd for the learnable-filter path (Filterbank(freeze=False),
# Fbank/MFCC(requires_grad=True); features.py:476-482): the reference gets
# these gradients from torch autograd; here they are HIP kernels too
# ---------------------------------------------------------------------------

@custom_op("sbk::filterbank_dense_bwd", mutates_args=())
def filterbank_dense_bwd(grad: torch.Tensor, spec: torch.Tensor, mat: torch.Tensor, log_mel: bool,
                         multiplier: float, db_offset: float, amin: float,
                         top_db: float) -> tuple[torch.Tensor, torch.Tensor]:
    """(dL/dspec, dL/dmat) of filterbank_dense: the linear energies are
    recomputed by the forward's own kernel (bit-identical dB values for the
    top_db tie rule), sbk_filterbank_db_bwd differentiates dB + top_db,
    dspec = dx·matᵀ runs on the dense filterbank kernel with matᵀ, and dmat
    is a chunked specᵀ·dx reduced by sbk_colsum (deterministic)."""
    require_device(grad, spec, mat)
    spec = _c(spec.to(_f32))
    mat = _c(mat.to(_f32))
    grad = _c(grad.to(_f32))
    N, T, Fd = spec.shape
    M = mat.shape[1]
    L = _lib.lib()
    s = stream_of(spec)
    x = torch.empty(N, T, M, device=spec.device, dtype=_f32)
    check(L.sbk_filterbank(ptr(spec), N, T, Fd, None, None, None, None, ptr(mat), M, 0, multiplier, db_offset, amin,
                           ptr(x), None, s), "sbk_filterbank(recompute)")
    dx = torch.empty_like(x)
    stats = torch.empty(3 * N, device=spec.device, dtype=_f32)
    check(L.sbk_filterbank_db_bwd(ptr(x), ptr(grad), N, T * M, int(log_mel), multiplier, db_offset, amin, top_db,
                                  ptr(stats), ptr(dx), s), "sbk_filterbank_db_bwd")
    matT = mat.t().contiguous()
    dspec = torch.empty(N, T, Fd, device=spec.device, dtype=_f32)
    check(L.sbk_filterbank(ptr(dx), N, T, M, None, None, None, None, ptr(matT), Fd, 0, 1.0, 0.0, 0.0, ptr(dspec),
                           None, s), "sbk_filterbank(dx·matT)")
    rows = N * T
    chunk = 256
    nch = (rows + chunk - 1) // chunk
    part = torch.empty(nch, Fd * M, device=spec.device, dtype=_f32)
    check(L.sbk_filterbank_wgrad(ptr(spec), ptr(dx), rows, Fd, M, chunk, ptr(part), s), "sbk_filterbank_wgrad")
    dmat = torch.empty(Fd, M, device=spec.device, dtype=_f32)
    check(L.sbk_colsum(ptr(part), nch, Fd * M, ptr(dmat), 0, s), "sbk_colsum")
    return dspec, dmat


@filterbank_dense_bwd.register_fake
def _(grad, spec, mat, log_mel, multiplier, db_offset, amin, top_db):
    return spec.new_empty(spec.shape), mat.new_empty(mat.shape)


def _fbd_setup(ctx, inputs, output):
    spec, mat, log_mel, mult, off, amin, top_db = inputs
    ctx.save_for_backward(spec, mat)
    ctx.args = (log_mel, mult, off, amin, top_db)


def _fbd_backward(ctx, grad):
    spec, mat = ctx.saved_tensors
    dspec, dmat = filterbank_dense_bwd(grad, spec, mat, *ctx.args)
    return (dspec if ctx.needs_input_grad[0] else None, dmat if ctx.needs_input_grad[1] else None,
            None, None, None, None, None)


filterbank_dense.register_autograd(_fbd_backward, setup_context=_fbd_setup)


def _dct_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])


def _dct_backward(ctx, grad):
    """y = x·D is linear: dx = g·Dᵀ on the same kernel (the DCT matrix is a
    fixed buffer in the reference, so it gets no gradient)."""
    (mat,) = ctx.saved_tensors
    return dct(grad, mat.t().contiguous()), None


dct.register_autograd(_dct_backward, setup_context=_dct_setup)
