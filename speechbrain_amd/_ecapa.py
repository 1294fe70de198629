"""Wrappers over csrc/ecapa.hip: the time-major eval forward of the ECAPA-TDNN
lobe.  Activations are (N, L, C) tensors in the compute dtype whose last axis
is contiguous and whose frames lie stride(1) elements apart — a plain tensor
or a channel slice of a wider buffer; the kernels read and write them in
place through that stride.  No autograd: the lobe takes these only when no
gradient is needed."""
import torch

from . import _enc
from ._lib import check, lib, ptr, require_device, stream_of

_bf16 = torch.bfloat16
_f32 = torch.float32


def tile():
    """Frames of a sbk_tdnn workgroup."""
    return int(lib().sbk_tdnn_tile())


def _rows(t):
    """Row stride of a time-major activation (N, L, C)."""
    if t.dim() != 3 or (t.stride(2) != 1 and t.shape[2] > 1):
        raise ValueError("time-major activations are (N, L, C), C contiguous")
    if t.shape[1] == 1:  # one frame: its stride is free, the utterances' is the row stride
        return t.stride(0) if t.shape[0] > 1 else t.shape[2]
    if t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError("time-major activations hold their utterances L rows apart")
    return t.stride(1)


def valid_counts(lengths, L):
    """Frames inside each utterance as the reference's mask counts them
    (length_to_mask(lengths * L, max_len=L).sum()), int32."""
    ar = torch.arange(L, device=lengths.device, dtype=lengths.dtype)
    return (ar[None] < (lengths * L)[:, None]).sum(1).to(torch.int32)


def tdnn_weight(w, dtype):
    """(Co, Ci, k) -> the kernel's (k, Co, Ci padded to 32) in the compute dtype."""
    Ci = w.shape[1]
    wp = torch.nn.functional.pad(w.detach().float().permute(2, 0, 1), (0, -Ci % 32))
    return wp.to(dtype).contiguous()


def bn_affine(bn):
    """Eval BatchNorm as a per-channel scale and shift (fp32)."""
    scale = torch.rsqrt(bn.running_var.float() + bn.eps)
    if bn.weight is not None:
        scale = scale * bn.weight.detach().float()
    shift = -bn.running_mean.float() * scale
    if bn.bias is not None:
        shift = shift + bn.bias.detach().float()
    return scale.contiguous(), shift.contiguous()


def tdnn(x, wp, Ci, k, d, bias=None, slope=0.0, scale=None, shift=None, tanh=False, add=None, out=None, valid=None,
         colsum=False):
    """One TDNN layer (sbk_tdnn) on x (N, L, Ci) -> out (N, L, Co); add: a second
    input summed into x; bias (Co) or (N, Co); colsum: also the (N, tiles, Co)
    partial column sums over each utterance's valid frames."""
    require_device(x, wp)
    N, L, _ = x.shape
    Co = wp.shape[1]
    if x.dtype != wp.dtype or x.shape[2] != Ci:
        raise ValueError(f"sbk_tdnn: input {tuple(x.shape)} {x.dtype} against a {wp.dtype} weight of {Ci} channels")
    if out is None:
        out = torch.empty(N, L, Co, device=x.device, dtype=x.dtype)
    part = torch.empty(N, -(-L // tile()), Co, device=x.device, dtype=_f32) if colsum else None
    per_utt = bias is not None and bias.dim() == 2
    check(lib().sbk_tdnn(int(x.dtype == _bf16), ptr(x), _rows(x), ptr(add), _rows(add) if add is not None else 0,
                         N, L, Ci, Co, k, d, ptr(wp), wp.shape[2], ptr(bias), int(per_utt), float(slope), ptr(scale),
                         ptr(shift), int(tanh), ptr(out), _rows(out), ptr(valid), ptr(part), stream_of(x)), "sbk_tdnn")
    return (out, part) if colsum else out


def res2net_supported(w, scale, k, d):
    return bool(lib().sbk_res2net_supported(w, scale, k, d))


def res2net(x, scale, k, d, wp, bias, aff_scale, aff_shift):
    """The whole Res2Net block (sbk_res2net) on x (N, L, scale * w) -> a new (N, L, scale * w)."""
    require_device(x, wp)
    N, L, C = x.shape
    if x.dtype != wp.dtype:
        raise ValueError(f"sbk_res2net: {x.dtype} input against a {wp.dtype} weight")
    out = torch.empty(N, L, C, device=x.device, dtype=x.dtype)
    check(lib().sbk_res2net(int(x.dtype == _bf16), ptr(x), _rows(x), N, L, C // scale, scale, k, d, ptr(wp), ptr(bias),
                            ptr(aff_scale), ptr(aff_shift), ptr(out), _rows(out), stream_of(x)), "sbk_res2net")
    return out


def se_gate(part, valid, L, w1, b1, w2, b2):
    N, tiles, C = part.shape
    s = torch.empty(N, C, device=part.device, dtype=_f32)
    check(lib().sbk_se_gate(ptr(part), tiles, ptr(valid), N, L, C, w1.shape[0], ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                            ptr(s), stream_of(part)), "sbk_se_gate")
    return s


def se_apply(x, s, res, out):
    """out = s[n, c] * x (+ res); x (N, L, C) contiguous, res and out strided."""
    N, L, C = x.shape
    if not x.is_contiguous():
        raise ValueError("sbk_se_apply: x must be contiguous")
    check(lib().sbk_se_apply(int(x.dtype == _bf16), ptr(x), ptr(s), ptr(res), _rows(res) if res is not None else 0, ptr(out), _rows(out), N, L, C,
                             stream_of(x)), "sbk_se_apply")
    return out


def asp_stats(x, valid):
    N, L, C = x.shape
    mean = torch.empty(N, C, device=x.device, dtype=_f32)
    sd = torch.empty_like(mean)
    check(lib().sbk_asp_stats(int(x.dtype == _bf16), ptr(x), _rows(x), ptr(valid), N, L, C, ptr(mean), ptr(sd),
                              stream_of(x)), "sbk_asp_stats")
    return mean, sd


def asp_pool(h, wc, bc, x, mu, valid):
    """(N, 2 C) fp32: the attention-weighted mean and deviation of x over time."""
    N, L, C = x.shape
    out = torch.empty(N, 2 * C, device=x.device, dtype=_f32)
    check(lib().sbk_asp_pool(int(x.dtype == _bf16), ptr(h), ptr(wc), ptr(bc), ptr(x), _rows(x), ptr(mu), ptr(valid),
                             N, L, h.shape[2], C, ptr(out), stream_of(x)), "sbk_asp_pool")
    return out


def to_time_major(x, dtype):
    """(N, C, L) of a sub-block's interface -> (N, L, C) contiguous in the compute dtype."""
    return _enc.to_compute(x.transpose(1, 2), dtype)
