"""Drop-ins for the arithmetic classes of
speechbrain.processing.speech_augmentation: Resample (:511-821), SpeedPerturb
(:435-508), DropFreq (:909-1010) and DropChunk (:1013-1173).

Every random draw is made on the host with the CPU generator in exactly the
reference's order, and the polyphase table and the notch filters are computed
on the host in float32 with the torch ops of the reference's CPU path, so a
given torch.manual_seed reproduces that path's decisions and tables bit for
bit — also for ROCm tensors, where the reference would take sin / cos and
the noise from the device.  The arithmetic on the waveform runs in
speechbrain_amd/csrc/tdaug.hip.  Each module splits into `draws` (host) and
`apply` (device), which lobes.augment.TimeDomainSpecAugment uses to run the
three stages in one launch; `last_draws` keeps what the last forward drew.

Inputs are contiguous fp32 device tensors; anything else raises.  There is no
CPU fallback.
"""
import math
from typing import Optional

import torch

from .._lib import OPS, check, custom_op, lib, ptr, require_device, stream_of

__all__ = ["Resample", "SpeedPerturb", "DropFreq", "DropChunk"]

FILTER_LENGTH = 101
_PAD = FILTER_LENGTH // 2
_AMP_CHUNKS = 64  # partial sums per row of sbk_drop_chunks' amplitude


# ------------------------------------------------------------------ custom ops

def _btc(x):
    return (x.shape[0], x.shape[1], 1 if x.dim() == 2 else x.shape[2])


@custom_op("sbk::resample", mutates_args=())
def resample(x: torch.Tensor, first: torch.Tensor, w: torch.Tensor, M: int, T_out: int) -> torch.Tensor:
    """x (B, T) or (B, T, C) fp32 through the polyphase table first (L)
    int32, w (L, W) fp32 with input stride M: (B, T_out[, C])."""
    B, T, C = _btc(x)
    y = x.new_empty((B, T_out) + tuple(x.shape[2:]))
    check(lib().sbk_resample(ptr(x), B, T, C, ptr(first), ptr(w), w.shape[0], M, w.shape[1], T_out, ptr(y),
                             stream_of(x)), "sbk_resample")
    return y


@resample.register_fake
def _(x, first, w, M, T_out):
    return x.new_empty((x.shape[0], T_out) + tuple(x.shape[2:]))


@custom_op("sbk::fir101", mutates_args=())
def fir101(x: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    """y[t] = sum_k taps[k] x[t + k - 50] on x (B, T) fp32, taps (101)."""
    y = torch.empty_like(x)
    check(lib().sbk_fir101(ptr(x), x.shape[0], x.shape[1], ptr(taps), ptr(y), stream_of(x)), "sbk_fir101")
    return y


@fir101.register_fake
def _(x, taps):
    return torch.empty_like(x)


@custom_op("sbk::drop_chunks", mutates_args=())
def drop_chunks(x: torch.Tensor, segs: torch.Tensor, noff: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                lengths: Optional[torch.Tensor], noise_factor: float) -> torch.Tensor:
    """x (B, T[, C]) with the [start, end) segments of segs (B, S, 2) int32
    zeroed, or (noise given) filled with the uploaded draws scaled by the
    row's amplitude (speech_augmentation.py:1160-1171)."""
    B, T, C = _btc(x)
    y = torch.empty_like(x)
    partial = amp = None
    if noise is not None:
        partial = x.new_empty(B * _AMP_CHUNKS)
        amp = x.new_empty(B)
    check(lib().sbk_drop_chunks(ptr(x), B, T, C, ptr(segs), segs.shape[1], ptr(noff), ptr(noise),
                                noise.numel() if noise is not None else 0, ptr(lengths), float(noise_factor),
                                ptr(partial), ptr(amp), ptr(y), stream_of(x)), "sbk_drop_chunks")
    return y


@drop_chunks.register_fake
def _(x, segs, noff, noise, lengths, noise_factor):
    return torch.empty_like(x)


@custom_op("sbk::tdaug", mutates_args=())
def tdaug(x: torch.Tensor, first: Optional[torch.Tensor], w: Optional[torch.Tensor], M: int, T_out: int,
          taps: Optional[torch.Tensor], segs: Optional[torch.Tensor]) -> torch.Tensor:
    """resample -> fir101 -> drop_chunks (zero fill) of x (B, T) in one
    launch; a stage whose table is None is dropped."""
    B, T = x.shape
    y = x.new_empty((B, T_out))
    L, W = (w.shape[0], w.shape[1]) if w is not None else (0, 0)
    check(lib().sbk_tdaug(ptr(x), B, T, ptr(first), ptr(w), L, M, W, T_out, ptr(taps), ptr(segs),
                          segs.shape[1] if segs is not None else 0, ptr(y), stream_of(x)), "sbk_tdaug")
    return y


@tdaug.register_fake
def _(x, first, w, M, T_out, taps, segs):
    return x.new_empty((x.shape[0], T_out))


# ---------------------------------------------------------------- host helpers

class _Pinned:
    """Host tables (int32 / fp32) -> device in one asynchronous copy out of a
    reused pinned buffer (a pageable copy would block the host)."""

    def __init__(self):
        self.buf = None
        self.ev = None

    def upload(self, parts, device):
        n = sum(p.numel() for p in parts)
        if self.buf is None or self.buf.numel() < n:
            self.buf = torch.empty(max(n, 1024), dtype=torch.int32).pin_memory()
            self.ev = None
        if self.ev is not None:
            self.ev.synchronize()  # the previous copy out of the buffer is done
        o = 0
        for p in parts:
            self.buf[o:o + p.numel()].copy_(p.contiguous().reshape(-1).view(torch.int32))
            o += p.numel()
        dev = self.buf[:n].to(device, non_blocking=True)
        self.ev = torch.cuda.Event()
        self.ev.record(torch.cuda.current_stream(device))
        out, o = [], 0
        for p in parts:
            out.append(dev[o:o + p.numel()].view(p.dtype).view(p.shape))
            o += p.numel()
        return out


def _check_wave(x, what):
    require_device(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError(f"{what} kernel expects a contiguous fp32 tensor")


_TABLES = {}  # (orig, new, width, device) -> (first int32, weights fp32) on the device


def notch_filter(notch_freq, filter_width=FILTER_LENGTH, notch_width=0.05):
    """The band-reject kernel of signal_processing.notch_filter (:373-430): a
    Blackman-windowed sinc low-pass at the notch frequency plus the spectral
    inversion of one just above it, (filter_width,) float32.  notch_freq is
    the 0-d float32 draw; the operations and their order are the
    reference's, so the taps are bit-identical to its CPU path."""
    assert 0 < notch_freq <= 1
    assert filter_width % 2 != 0
    pad = filter_width // 2
    pos = torch.arange(filter_width) - pad
    centre = notch_freq + notch_width  # the reference shifts the draw up by one width first

    def sinc(arg):
        return torch.cat([torch.sin(arg[:pad]) / arg[:pad], torch.ones(1), torch.sin(arg[pad + 1:]) / arg[pad + 1:]])

    low = sinc(3 * (centre - notch_width) * pos)
    low *= torch.blackman_window(filter_width)
    low /= torch.sum(low)
    high = sinc(3 * (centre + notch_width) * pos)
    high *= torch.blackman_window(filter_width)
    high /= -torch.sum(high)
    high[pad] += 1
    return low + high


def combined_filter(frequencies, drop_width=0.05):
    """The filter DropFreq applies for the drawn frequencies (:991-1004): a
    101-tap delta run through one zero-padded conv1d per notch, hence cut back
    to 101 taps after every notch, and applied as a correlation."""
    # (batch, time, channel) tensors transposed for conv1d, as the reference
    # holds them: torch picks its conv1d path by the strides, and the paths
    # differ in the last bit
    taps = torch.zeros(1, FILTER_LENGTH, 1)
    taps[0, _PAD, 0] = 1
    for f in frequencies:
        notch = notch_filter(f, FILTER_LENGTH, drop_width).view(1, -1, 1)
        taps = torch.nn.functional.conv1d(taps.transpose(2, 1), notch.transpose(2, 1), padding=_PAD).transpose(2, 1)
    return taps.reshape(-1)


# --------------------------------------------------------------------- modules

class Resample(torch.nn.Module):
    """Sinc-interpolation resampler (Kaldi's LinearResample); `first_indices`
    and `weights` are the reference's table, computed on the host."""

    def __init__(self, orig_freq=16000, new_freq=16000, lowpass_filter_width=6):
        super().__init__()
        self.orig_freq = orig_freq
        self.new_freq = new_freq
        self.lowpass_filter_width = lowpass_filter_width
        self._compute_strides()
        assert self.orig_freq % self.conv_stride == 0
        assert self.new_freq % self.conv_transpose_stride == 0

    def _compute_strides(self):
        base = math.gcd(self.orig_freq, self.new_freq)
        self.conv_stride = self.orig_freq // base              # M: input samples per unit
        self.output_samples = self.new_freq // base            # L: output samples (phases) per unit
        self.conv_transpose_stride = self.output_samples

    def _output_samples(self, input_num_samp):
        """Outputs in the half-open interval the input covers
        (LinearResample::GetNumOutputSamples), in exact integer ticks."""
        a, b = int(self.orig_freq), int(self.new_freq)
        ticks = a * b // math.gcd(a, b)
        span = input_num_samp * (ticks // a)
        if span <= 0:
            return 0
        per_out = ticks // b
        last = span // per_out
        if last * per_out == span:
            last -= 1
        return last + 1

    def _indices_and_weights(self, waveforms=None):
        """The polyphase table (LinearResample::SetIndexesAndWeights) in
        float32 on the host, operation for operation the reference's."""
        low = min(self.orig_freq, self.new_freq)
        cutoff = 0.99 * 0.5 * low
        assert cutoff * 2 <= low
        half_width = self.lowpass_filter_width / (2.0 * cutoff)
        out_t = torch.arange(start=0.0, end=self.output_samples)
        out_t /= self.new_freq
        t_min = out_t - half_width
        t_max = out_t + half_width
        first = torch.ceil(t_min * self.orig_freq)
        last = torch.floor(t_max * self.orig_freq)
        width = (last - first + 1).max()
        j = torch.arange(width)
        index = first.unsqueeze(1) + j.unsqueeze(0)
        dt = (index / self.orig_freq) - out_t.unsqueeze(1)
        weights = torch.zeros_like(dt)
        inside = dt.abs().lt(half_width)
        # Hann window of the filter's width ...
        weights[inside] = 0.5 * (1 + torch.cos(2 * math.pi * cutoff / self.lowpass_filter_width * dt[inside]))
        at_zero = dt.eq(0.0)
        off_zero = ~at_zero
        # ... times the sinc, and its limit at 0
        weights[off_zero] *= torch.sin(2 * math.pi * cutoff * dt[off_zero]) / (math.pi * dt[off_zero])
        weights[at_zero] *= 2 * cutoff
        weights /= self.orig_freq
        self.first_indices = first
        self.weights = weights

    def table(self, device):
        """(first int32 (L), weights fp32 (L, W)) on `device`, cached per
        (orig, new, width, device)."""
        key = (self.orig_freq, self.new_freq, self.lowpass_filter_width, str(device))
        if key not in _TABLES:
            if not hasattr(self, "first_indices"):
                self._indices_and_weights()
            _TABLES[key] = _Pinned().upload([self.first_indices.to(torch.int32), self.weights], device)
        return _TABLES[key]

    def apply(self, waveforms):
        first, w = self.table(waveforms.device)
        return OPS.resample(waveforms, first, w, self.conv_stride, self._output_samples(waveforms.shape[1]))

    def forward(self, waveforms):
        """(batch, time) or (batch, time, channels) -> the same at new_freq."""
        _check_wave(waveforms, "Resample")
        if not hasattr(self, "first_indices"):
            self._indices_and_weights()
        if self.orig_freq == self.new_freq:
            return waveforms
        if waveforms.dim() not in (2, 3):
            raise ValueError("Input must be 2 or 3 dimensions")
        return self.apply(waveforms)


class SpeedPerturb(torch.nn.Module):
    def __init__(self, orig_freq, speeds=[90, 100, 110], perturb_prob=1.0):
        super().__init__()
        self.orig_freq = orig_freq
        self.speeds = speeds
        self.perturb_prob = perturb_prob
        self.samp_index = 0
        self.resamplers = [Resample(orig_freq=orig_freq, new_freq=orig_freq * s // 100) for s in speeds]
        self.last_draws = None

    def draws(self):
        """(rand(1), index into speeds or None below perturb_prob)."""
        u = torch.rand(1)
        if u > self.perturb_prob:
            return u, None
        return u, torch.randint(len(self.speeds), (1,))[0]

    def forward(self, waveform):
        _check_wave(waveform, "SpeedPerturb")
        self.last_draws = u, idx = self.draws()
        if idx is None:
            return waveform.clone()
        self.samp_index = idx
        return self.resamplers[idx](waveform)


class DropFreq(torch.nn.Module):
    def __init__(self, drop_freq_low=1e-14, drop_freq_high=1, drop_count_low=1, drop_count_high=2, drop_width=0.05,
                 drop_prob=1):
        super().__init__()
        self.drop_freq_low = drop_freq_low
        self.drop_freq_high = drop_freq_high
        self.drop_count_low = drop_count_low
        self.drop_count_high = drop_count_high
        self.drop_width = drop_width
        self.drop_prob = drop_prob
        self.last_draws = None
        self._pin = _Pinned()

    def draws(self):
        """(rand(1), count, frequencies, combined 101-tap filter); the last
        three None below drop_prob."""
        u = torch.rand(1)
        if u > self.drop_prob:
            return u, None, None, None
        count = torch.randint(low=self.drop_count_low, high=self.drop_count_high + 1, size=(1,))
        freqs = torch.rand(count) * (self.drop_freq_high - self.drop_freq_low) + self.drop_freq_low
        return u, count, freqs, combined_filter(freqs, self.drop_width)

    def forward(self, waveforms):
        """(batch, time) or (batch, time, 1) -> (batch, time)."""
        _check_wave(waveforms, "DropFreq")
        if waveforms.dim() not in (2, 3):
            raise ValueError("Convolve1D expects a 3-dimensional tensor")
        self.last_draws = u, count, freqs, taps = self.draws()
        if count is None:
            return waveforms.clone()
        if waveforms.dim() == 3 and waveforms.shape[2] != 1:
            raise RuntimeError(f"DropFreq filters one channel; got {waveforms.shape[2]} (the reference's conv1d "
                               "raises on the channel count as well)")
        x = waveforms.view(waveforms.shape[0], waveforms.shape[1])
        if int(count) == 0:
            return x.clone()  # the filter is the delta it started as
        return OPS.fir101(x, self._pin.upload([taps], x.device)[0])


class DropChunk(torch.nn.Module):
    def __init__(self, drop_length_low=100, drop_length_high=1000, drop_count_low=1, drop_count_high=10, drop_start=0,
                 drop_end=None, drop_prob=1, noise_factor=0.0):
        super().__init__()
        self.drop_length_low = drop_length_low
        self.drop_length_high = drop_length_high
        self.drop_count_low = drop_count_low
        self.drop_count_high = drop_count_high
        self.drop_start = drop_start
        self.drop_end = drop_end
        self.drop_prob = drop_prob
        self.noise_factor = noise_factor
        if drop_length_low > drop_length_high:
            raise ValueError("Low limit must not be more than high limit")
        if drop_count_low > drop_count_high:
            raise ValueError("Low limit must not be more than high limit")
        if drop_end is not None and drop_end >= 0:
            if drop_start > drop_end:
                raise ValueError("Low limit must not be more than high limit")
            # a chunk is no longer than the window it may start in
            self.drop_length_low = min(drop_length_low, drop_end - drop_start)
            self.drop_length_high = min(drop_length_high, drop_end - drop_start)
        self.last_draws = None
        self._pin = _Pinned()

    def draws(self, lengths):
        """Host draws for a batch with absolute `lengths` (B ints):
        (rand(1), drop_times (B) or None below drop_prob, per utterance
        (length, start) or None for a zero count, per utterance the list of
        noise vectors)."""
        u = torch.rand(1)
        if u > self.drop_prob:
            return u, None, None, None
        lengths = [int(v) for v in lengths]
        B = len(lengths)
        times = torch.randint(low=self.drop_count_low, high=self.drop_count_high + 1, size=(B,))
        chunks, noise = [], []
        for i, n in enumerate(times.tolist()):
            if n == 0:
                chunks.append(None)
                noise.append([])
                continue
            length = torch.randint(low=self.drop_length_low, high=self.drop_length_high + 1, size=(n,))
            lo = self.drop_start
            if lo < 0:
                lo += lengths[i]
            hi = self.drop_end
            if hi is None:
                hi = lengths[i]
            if hi < 0:
                hi += lengths[i]
            hi = max(0, hi - int(length.max()))
            start = torch.randint(low=lo, high=hi + 1, size=(n,))
            chunks.append((length, start))
            noise.append([torch.rand(int(length[j])) for j in range(n)] if self.noise_factor else [])
        return u, times, chunks, noise

    @staticmethod
    def segments(chunks, T):
        """(B, S, 2) int32 [start, end) per chunk as the reference's slice
        takes them — an end past T clipped at T — padded with empty
        segments; None when no utterance drew a chunk."""
        rows = []
        for c in chunks:
            row = []
            if c is not None:
                for n, at in zip(c[0].tolist(), c[1].tolist()):
                    s, e, _ = slice(at, at + n).indices(T)
                    row.append((s, max(s, e)))
            rows.append(row)
        S = max(len(r) for r in rows)
        if S == 0:
            return None
        return torch.tensor([r + [(0, 0)] * (S - len(r)) for r in rows], dtype=torch.int32)

    def host_lengths(self, waveforms, lengths):
        """The absolute lengths, computed as the reference computes them (on
        the tensor's device) and brought to the host — B values, the one
        device -> host copy of this stage: the draws depend on them."""
        require_device(lengths)
        return (lengths * waveforms.size(1)).long().cpu()

    def apply(self, waveforms, lengths_abs, chunks, noise):
        T = waveforms.shape[1]
        segs = self.segments(chunks, T)
        if segs is None:
            return waveforms.clone()
        if not self.noise_factor:
            return OPS.drop_chunks(waveforms, self._pin.upload([segs], waveforms.device)[0], None, None, None, 0.0)
        noff = torch.zeros(segs.shape[0], segs.shape[1], dtype=torch.int32)
        flat, o = [], 0
        for i, c in enumerate(chunks):
            for j, v in enumerate(noise[i]):
                if int(segs[i, j, 1]) - int(segs[i, j, 0]) != v.numel():
                    raise RuntimeError(f"DropChunk: a chunk of {v.numel()} samples at {int(c[1][j])} does not fit "
                                       f"the {T} samples (the reference's slice assignment raises as well)")
                noff[i, j] = o
                flat.append(v)
                o += v.numel()
        if o == 0:
            return waveforms.clone()  # only zero-length chunks were drawn
        segs_d, noff_d, len_d, noise_d = self._pin.upload(
            [segs, noff, lengths_abs.to(torch.int32), torch.cat(flat)], waveforms.device)
        return OPS.drop_chunks(waveforms, segs_d, noff_d, noise_d, len_d, float(self.noise_factor))

    def forward(self, waveforms, lengths):
        """(batch, time) or (batch, time, channels) and relative lengths
        (batch) -> the same shape with the drawn chunks zeroed / noised."""
        _check_wave(waveforms, "DropChunk")
        if waveforms.dim() not in (2, 3):
            raise ValueError("Input must be 2 or 3 dimensions")
        if self.noise_factor and waveforms.dim() == 3:
            raise RuntimeError("DropChunk with noise takes (batch, time) waveforms")
        lengths_abs = self.host_lengths(waveforms, lengths)
        self.last_draws = u, times, chunks, noise = self.draws(lengths_abs)
        if times is None:
            return waveforms.clone()
        return self.apply(waveforms, lengths_abs, chunks, noise)
