"""Drop-in for speechbrain.lobes.augment.SpecAugment (augment.py:32-201).

Random draws (warp centre/width, mask lengths/positions) are made on the host
with the CPU generator in exactly the reference's order, so a given
torch.manual_seed reproduces the reference CPU path's mask indices bit for
bit — also for ROCm tensors, where the reference would draw masks on the
device generator.  The warp / mask / mean-fill arithmetic runs in
speechbrain_amd/csrc/augment.hip; the input is mutated in place and
returned, as in the reference.

TimeDomainSpecAugment (augment.py:204-299) chains the SpeedPerturb, DropFreq
and DropChunk drop-ins of processing.speech_augmentation; with zero-fill
chunks its three stages run as one launch of sbk_tdaug.
"""
from typing import Optional

import torch

from .._lib import OPS, check, custom_op, lib, ptr, require_device, stream_of
from ..processing.speech_augmentation import DropChunk, DropFreq, SpeedPerturb, _check_wave, _Pinned

__all__ = ["SpecAugment", "TimeDomainSpecAugment"]

_WARP_MODES = {"bicubic": 0, "bilinear": 1}


@custom_op("sbk::specaugment_", mutates_args=("x",))
def specaugment_(x: torch.Tensor, N: int, T: int, F: int, c: int, w: int, fm: Optional[torch.Tensor],
                 tm: Optional[torch.Tensor], use_mean: bool, n_fcells: int, warp_mode: int = 0) -> None:
    """Applies the drawn warp (c, w; -1 = none; warp_mode 0 bicubic, 1
    bilinear) and freq / time masks
    (fm, tm: (N, n, 2) int32 [len, pos]) to x (N, T, F) fp32 in place, with
    the batch-mean fill when use_mean (augment.py:116-201)."""
    n_f = fm.shape[1] if fm is not None else 0
    n_t = tm.shape[1] if tm is not None else 0
    # the in-place path (the float4 shapes of the recipe) needs no scratch copy
    tmp = (torch.empty_like(x) if lib().sbk_specaugment_needs_scratch(N, T, F, c, w, n_f, n_t,
                                                                       int(x.data_ptr() % 16 == 0)) else None)
    # partial sums: the copy path's 2 per 4 rows (+ its two fills), the
    # in-place path's 3 per column slab
    npart = max(2 * N * ((T + 3) // 4), 3 * N * (F // 4))
    partial = torch.empty(npart + 4, device=x.device, dtype=torch.float32) if use_mean else None
    rc = lib().sbk_specaugment(ptr(x), N, T, F, c, w, int(warp_mode), ptr(tmp), ptr(fm), n_f, ptr(tm), n_t,
                               int(use_mean),
                               ptr(partial), n_fcells, stream_of(x))
    check(rc, "sbk_specaugment")


@specaugment_.register_fake
def _(x, N, T, F, c, w, fm, tm, use_mean, n_fcells, warp_mode=0):
    return None


class SpecAugment(torch.nn.Module):
    def __init__(self, time_warp=True, time_warp_window=5, time_warp_mode="bicubic", freq_mask=True,
                 freq_mask_width=(0, 20), n_freq_mask=2, time_mask=True, time_mask_width=(0, 100), n_time_mask=2,
                 replace_with_zero=True):
        super().__init__()
        assert time_warp or freq_mask or time_mask, \
            "at least one of time_warp, time_mask, or freq_mask should be applied"
        if time_warp and time_warp_mode not in _WARP_MODES:
            # the reference interpolates with align_corners=True (augment.py:134-148), which torch
            # accepts for the (bi)linear / bicubic modes only; the other modes raise there too
            raise ValueError(f"time_warp_mode {time_warp_mode!r}: align_corners interpolation needs one of "
                             f"{sorted(_WARP_MODES)}")
        self.apply_time_warp = time_warp
        self.time_warp_window = time_warp_window
        self.time_warp_mode = time_warp_mode
        self.freq_mask = freq_mask
        if isinstance(freq_mask_width, int):
            freq_mask_width = (0, freq_mask_width)
        self.freq_mask_width = freq_mask_width
        self.n_freq_mask = n_freq_mask
        self.time_mask = time_mask
        if isinstance(time_mask_width, int):
            time_mask_width = (0, time_mask_width)
        self.time_mask_width = time_mask_width
        self.n_time_mask = n_time_mask
        self.replace_with_zero = replace_with_zero
        self.last_draws = None
        self._pin = None     # pinned staging of the mask draws (reused; see _upload)
        self._pin_ev = None  # completion of the last upload out of it

    def _upload(self, parts, device):
        """int32 host draws (concatenated) -> device, asynchronously from a
        reused pinned buffer (a pageable copy would block the host for the
        transfer)."""
        n = sum(p.numel() for p in parts)
        if self._pin is None or self._pin.numel() < n:
            self._pin = torch.empty(max(n, 1024), dtype=torch.int32).pin_memory()
            self._pin_ev = None
        if self._pin_ev is not None:
            self._pin_ev.synchronize()  # the previous copy out of the buffer is done
        o = 0
        for p in parts:
            self._pin[o:o + p.numel()].copy_(p)
            o += p.numel()
        dev = self._pin[:n].to(device, non_blocking=True)
        self._pin_ev = torch.cuda.Event()
        self._pin_ev.record(torch.cuda.current_stream(device))
        return dev

    def draws(self, N, T, F):
        """Host draws in the reference order (augment.py:131-133, :175-186)."""
        c = w = -1
        if self.apply_time_warp:
            win = self.time_warp_window
            if T - win > win:
                c = int(torch.randint(win, T - win, (1,))[0])
                w = int(torch.randint(c - win, c + win, (1,))[0]) + 1
        # (int32 draws: the same values as the reference's int64 ones — one
        # 32-bit generator draw per element either way, tests/test_augment_draws.py)
        i32 = torch.int32
        fm = tm = None
        if self.freq_mask:
            ln = torch.randint(self.freq_mask_width[0], self.freq_mask_width[1], (N, self.n_freq_mask), dtype=i32)
            ps = torch.randint(0, max(1, F - int(ln.max())), (N, self.n_freq_mask), dtype=i32)
            fm = torch.stack([ln, ps], -1)
        if self.time_mask:
            ln = torch.randint(self.time_mask_width[0], self.time_mask_width[1], (N, self.n_time_mask), dtype=i32)
            ps = torch.randint(0, max(1, T - int(ln.max())), (N, self.n_time_mask), dtype=i32)
            tm = torch.stack([ln, ps], -1)
        return c, w, fm, tm

    def forward(self, x):
        """Takes in input a tensor and returns an augmented one (in place)."""
        require_device(x)
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise TypeError("SpecAugment kernel expects a contiguous fp32 tensor")
        if x.dim() == 3:
            N, T, F = x.shape
        elif x.dim() == 4:
            N, T, F = x.shape[0] * x.shape[1], x.shape[2], x.shape[3]
        else:
            raise ValueError("expected (batch, time, freq) or (batch, channel, time, freq)")
        c, w, fm, tm = self.draws(N, T, F)
        if c == w:
            c = w = -1  # identical segment sizes: the resize is the identity
        self.last_draws = (c, w, fm, tm)
        # both mask tables in one asynchronous pinned host -> device copy (the
        # per-step host work is this module's cost at config 2, not its
        # kernels); the second mean's masked-cell count is taken on the
        # device from the table (n_fcells = -1)
        parts = [m.reshape(-1) for m in (fm, tm) if m is not None]
        fm_d = tm_d = None
        if parts:
            buf = self._upload(parts, x.device)
            nf = fm.numel() if fm is not None else 0
            fm_d = buf[:nf].view(fm.shape) if fm is not None else None
            tm_d = buf[nf:].view(tm.shape) if tm is not None else None
        OPS.specaugment_(x, N, T, F, c, w, fm_d, tm_d, not self.replace_with_zero, -1,
                                   _WARP_MODES.get(self.time_warp_mode, 0))
        return x


class TimeDomainSpecAugment(torch.nn.Module):
    """Speed perturbation, frequency dropping and chunk dropping on the
    waveform.  `fused` (default True) selects the one-launch path, taken for
    (batch, time) input and zero-fill chunks; otherwise — white-noise chunks
    need the filtered signal's amplitude first — the three stages run one
    after another.  Both make the same draws in the same order."""

    def __init__(self, perturb_prob=1.0, drop_freq_prob=1.0, drop_chunk_prob=1.0, speeds=[95, 100, 105],
                 sample_rate=16000, drop_freq_count_low=0, drop_freq_count_high=3, drop_chunk_count_low=0,
                 drop_chunk_count_high=5, drop_chunk_length_low=1000, drop_chunk_length_high=2000,
                 drop_chunk_noise_factor=0):
        super().__init__()
        self.speed_perturb = SpeedPerturb(perturb_prob=perturb_prob, orig_freq=sample_rate, speeds=speeds)
        self.drop_freq = DropFreq(drop_prob=drop_freq_prob, drop_count_low=drop_freq_count_low,
                                  drop_count_high=drop_freq_count_high)
        self.drop_chunk = DropChunk(drop_prob=drop_chunk_prob, drop_count_low=drop_chunk_count_low,
                                    drop_count_high=drop_chunk_count_high, drop_length_low=drop_chunk_length_low,
                                    drop_length_high=drop_chunk_length_high, noise_factor=drop_chunk_noise_factor)
        self.fused = True
        self.last_draws = None
        self._pin = _Pinned()

    def draws(self, T, lengths):
        """The three stages' host draws for a (batch, T) input, in the
        reference's order: (resampler or None, T_out, 101 taps or None,
        (B, S, 2) segments or None).  A stage that is not applied — below
        its probability, speed 100, zero notches, zero chunks — is None."""
        sp, df, dc = self.speed_perturb, self.drop_freq, self.drop_chunk
        sp.last_draws = _, idx = sp.draws()
        rs = None
        if idx is not None:
            sp.samp_index = idx
            if sp.resamplers[idx].orig_freq != sp.resamplers[idx].new_freq:
                rs = sp.resamplers[idx]
                if not hasattr(rs, "first_indices"):
                    rs._indices_and_weights()
        T_out = rs._output_samples(T) if rs is not None else T
        df.last_draws = _, count, _, taps = df.draws()
        if count is None or int(count) == 0:
            taps = None
        # the chunk draws depend on the absolute lengths of the resampled
        # batch: B values device -> host, as the reference syncs for them
        lengths_abs = (lengths * T_out).long().cpu()
        dc.last_draws = _, times, chunks, _ = dc.draws(lengths_abs)
        segs = dc.segments(chunks, T_out) if times is not None else None
        return rs, T_out, taps, segs

    def _forward_fused(self, x, lengths):
        require_device(lengths)
        rs, T_out, taps, segs = self.draws(x.shape[1], lengths)
        first = w = taps_d = segs_d = None
        if rs is not None:
            first, w = rs.table(x.device)
        parts = [p for p in (taps, segs) if p is not None]
        if parts:
            dev = self._pin.upload(parts, x.device)
            taps_d = dev[0] if taps is not None else None
            segs_d = dev[-1] if segs is not None else None
        return OPS.tdaug(x, first, w, rs.conv_stride if rs is not None else 1, T_out, taps_d, segs_d)

    def forward(self, waveforms, lengths):
        """Returns the distorted waveforms."""
        _check_wave(waveforms, "TimeDomainSpecAugment")
        with torch.no_grad():
            if self.fused and waveforms.dim() == 2 and not self.drop_chunk.noise_factor:
                waveforms = self._forward_fused(waveforms, lengths)
            else:
                waveforms = self.speed_perturb(waveforms)
                waveforms = self.drop_freq(waveforms)
                waveforms = self.drop_chunk(waveforms, lengths)
        self.last_draws = (self.speed_perturb.last_draws, self.drop_freq.last_draws, self.drop_chunk.last_draws)
        return waveforms
