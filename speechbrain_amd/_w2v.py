"""torch.library custom ops over the config-5 kernels (csrc/w2v.hip,
csrc/mxgemm.hip): the wav2vec2 latent extractor's layer 0, the row
LayerNorm / activation / MXFP8 quantisation kernel and the MXFP8 GEMM.

MXFP8 tensors travel as two tensors: e4m3 bytes (uint8, (M, K)) and one
E8M0 scale byte per 32 consecutive K elements (uint8, (M, K/32)).  `MX`
bundles them for the module code.  No op has a CPU path.

Second half: the pre-training objective's ops over csrc/w2vloss.hip — the
contrastive loss (float negatives or row indices, with its backward) and the
Gumbel vector quantiser after the projection (with its backward)."""
import functools
from typing import NamedTuple, Optional

import torch

from ._lib import OPS, check, custom_op, lib, ptr, require_device, stream_of

_f32, _bf16, _u8 = torch.float32, torch.bfloat16, torch.uint8
OUT = {_f32: 0, _bf16: 1, "mx": 2}
ACT = {None: 0, "none": 0, "relu": 3, "gelu": 4}


class MX(NamedTuple):
    """An MXFP8 matrix: q (M, K) e4m3 bytes, s (M, K/32) E8M0 bytes."""
    q: torch.Tensor
    s: torch.Tensor


def _empty_out(M, N, mode, dev):
    if mode == 2:
        return torch.empty(M, N, device=dev, dtype=_u8), torch.empty(M, N // 32, device=dev, dtype=_u8)
    return torch.empty(M, N, device=dev, dtype=_bf16 if mode == 1 else _f32), torch.empty(0, device=dev, dtype=_u8)


def _fake_out(x, M, N, mode):
    if mode == 2:
        return x.new_empty(M, N, dtype=_u8), x.new_empty(M, N // 32, dtype=_u8)
    return x.new_empty(M, N, dtype=_bf16 if mode == 1 else _f32), x.new_empty(0, dtype=_u8)


# ---------------------------------------------------------------------------
@custom_op("sbk::w2v_wav_stats", mutates_args=())
def wav_stats(wav: torch.Tensor, eps: float) -> torch.Tensor:
    """(B, 2) [mean, rstd] of F.layer_norm(wav, wav.shape[1:]) (wav2vec.py:92-93)."""
    B, S = wav.shape
    st = torch.empty(B, 2, device=wav.device, dtype=_f32)
    check(lib().sbk_w2v_wav_stats(ptr(wav), B, S, float(eps), ptr(st), stream_of(wav)), "sbk_w2v_wav_stats")
    return st


@wav_stats.register_fake
def _(wav, eps):
    return wav.new_empty(wav.shape[0], 2)


@custom_op("sbk::w2v_conv0", mutates_args=())
def _conv0_op(wav: torch.Tensor, stats: Optional[torch.Tensor], w: torch.Tensor, g: torch.Tensor, b: torch.Tensor,
              eps: float, stride: int, out_mode: int) -> tuple[torch.Tensor, torch.Tensor]:
    B, S = wav.shape
    C, K = w.shape
    T0 = (S - K) // stride + 1
    out, sc = _empty_out(B * T0, C, out_mode, wav.device)
    check(lib().sbk_w2v_conv0(ptr(wav), ptr(stats), B, S, T0, C, K, stride, ptr(w), ptr(g), ptr(b), float(eps),
                              ptr(out), out_mode, ptr(sc) if out_mode == 2 else None, stream_of(wav)),
          "sbk_w2v_conv0")
    return out, sc


@_conv0_op.register_fake
def _(wav, stats, w, g, b, eps, stride, out_mode):
    T0 = (wav.shape[1] - w.shape[1]) // stride + 1
    return _fake_out(wav, wav.shape[0] * T0, w.shape[0], out_mode)


def conv0(wav, stats, w, g, b, eps, stride, out):
    """Layer 0 of the latent extractor: (B, S) → (B*T0, C) in `out`
    (torch.float32 | torch.bfloat16 | "mx")."""
    require_device(wav, w)
    y, s = OPS.w2v_conv0(wav.contiguous(), stats, w.contiguous(), g, b, float(eps), int(stride), OUT[out])
    return MX(y, s) if out == "mx" else y


@custom_op("sbk::ln_act", mutates_args=())
def _ln_act_op(x: torch.Tensor, g: Optional[torch.Tensor], b: Optional[torch.Tensor], eps: float, act: int,
               out_mode: int) -> tuple[torch.Tensor, torch.Tensor]:
    M, D = x.shape
    out, sc = _empty_out(M, D, out_mode, x.device)
    check(lib().sbk_ln_act(ptr(x), int(x.dtype == _bf16), x.stride(0), M, D, ptr(g), ptr(b), float(eps), act,
                           ptr(out), out.stride(0), out_mode, ptr(sc) if out_mode == 2 else None,
                           sc.stride(0) if out_mode == 2 else 0, stream_of(x)), "sbk_ln_act")
    return out, sc


@_ln_act_op.register_fake
def _(x, g, b, eps, act, out_mode):
    return _fake_out(x, x.shape[0], x.shape[1], out_mode)


def ln_act(x, ln=None, act=None, out=_f32):
    """Row LayerNorm (ln = (weight, bias, eps) or None) → activation → output
    fp32 / bf16 / "mx".  x: (M, D) fp32 or bf16, unit column stride."""
    require_device(x)
    if x.stride(-1) != 1:
        x = x.contiguous()
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    y, s = OPS.ln_act(x, g, b, float(eps), ACT[act], OUT[out])
    return MX(y, s) if out == "mx" else y


@custom_op("sbk::mx_quant", mutates_args=())
def _mx_quant_op(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    M, K = x.shape
    q = torch.empty(M, K, device=x.device, dtype=_u8)
    s = torch.empty(M, K // 32, device=x.device, dtype=_u8)
    check(lib().sbk_mx_quant(ptr(x), int(x.dtype == _bf16), x.stride(0), M, K, ptr(q), q.stride(0), ptr(s),
                             s.stride(0), stream_of(x)), "sbk_mx_quant")
    return q, s


@_mx_quant_op.register_fake
def _(x):
    return x.new_empty(x.shape, dtype=_u8), x.new_empty(x.shape[0], x.shape[1] // 32, dtype=_u8)


def mx_quant(x):
    """fp32 / bf16 (M, K) → MX (power-of-two block scales, e4m3 elements)."""
    require_device(x)
    q, s = OPS.mx_quant(x if x.stride(-1) == 1 else x.contiguous())
    return MX(q, s)


def mx_dequant(m):
    """MX → fp32 (tests)."""
    M, K = m.q.shape
    out = torch.empty(M, K, device=m.q.device, dtype=_f32)
    check(lib().sbk_mx_dequant(ptr(m.q), m.q.stride(0), ptr(m.s), m.s.stride(0), M, K, ptr(out),
                               stream_of(m.q)), "sbk_mx_dequant")
    return out


@custom_op("sbk::mx_gemm", mutates_args=())
def _mx_gemm_op(aq: torch.Tensor, asc: torch.Tensor, M: int, K: int, lda: int, ldsa: int, rpb: int, a_bs: int,
                s_bs: int, wq: torch.Tensor, wsc: torch.Tensor, bias: Optional[torch.Tensor], act: int, alpha: float,
                res: Optional[torch.Tensor], out_mode: int) -> tuple[torch.Tensor, torch.Tensor]:
    N = wq.shape[0]
    out, sc = _empty_out(M, N, out_mode, aq.device)
    # the 256-tile kernel's split-K tail workspace (config 5's FFN
    # down-projection); 0 floats at shapes that do not split
    nws = _ws_floats(M, N, K, out_mode)
    ws = torch.empty(nws, device=aq.device, dtype=_f32) if nws else None
    check(lib().sbk_mx_gemm_ws(ptr(aq), ptr(asc), lda, ldsa, rpb, a_bs, s_bs, ptr(wq), ptr(wsc), wq.stride(0),
                               wsc.stride(0), M, N, K, ptr(bias), act, float(alpha), ptr(res),
                               res.stride(0) if res is not None else 0, ptr(out), out.stride(0), out_mode,
                               ptr(sc) if out_mode == 2 else None, sc.stride(0) if out_mode == 2 else 0, ptr(ws), nws,
                               stream_of(aq)), "sbk_mx_gemm_ws")
    return out, sc


@functools.lru_cache(maxsize=None)
def _ws_floats(M, N, K, out_mode):
    return int(lib().sbk_mx_gemm_ws_floats(M, N, K, out_mode))


@_mx_gemm_op.register_fake
def _(aq, asc, M, K, lda, ldsa, rpb, a_bs, s_bs, wq, wsc, bias, act, alpha, res, out_mode):
    return _fake_out(aq, M, wq.shape[0], out_mode)


def mx_gemm(a, w, bias=None, act=None, alpha=1.0, res=None, out=_f32):
    """out = res + alpha * act(A·Wᵀ + bias), A and W as MX (row-major, K-contiguous)."""
    require_device(a.q, w.q)
    M, K = a.q.shape
    if w.q.shape[1] != K:
        raise ValueError(f"mx_gemm K mismatch {K} vs {w.q.shape[1]}")
    if res is not None and (res.dtype != _f32 or res.stride(-1) != 1):
        raise ValueError("residual must be fp32, row-contiguous")
    y, s = OPS.mx_gemm(a.q, a.s, M, K, a.q.stride(0), a.s.stride(0), M, 0, 0, w.q, w.s, bias, ACT[act],
                                 float(alpha), res, OUT[out])
    return MX(y, s) if out == "mx" else y


def mx_conv_gemm(x, B, T_in, C, k, stride, w, out=_f32):
    """Conv1d(C → N, kernel k, stride, "valid", no bias) over channels-last
    MX rows x (B*T_in, C) as ONE GEMM: output row (b, t) reads the k
    consecutive input rows from (b, stride*t) — K = k*C, lda = stride*C,
    batch stride T_in*C (scales likewise); w: MX of the weight permuted to
    [out][tap][in] (CNN.py:309-516, padding "valid")."""
    T_out = (T_in - k) // stride + 1
    M = B * T_out
    y, s = OPS.mx_gemm(x.q, x.s, M, k * C, stride * C, stride * C // 32, T_out, T_in * C,
                                 T_in * C // 32, w.q, w.s, None, 0, 1.0, None, OUT[out])
    return (MX(y, s) if out == "mx" else y), T_out


@custom_op("sbk::add_posenc", mutates_args=("x",))
def add_posenc(x: torch.Tensor, pe: torch.Tensor, T: int) -> None:
    """x (B*T, D) fp32 += pe[t] (EncoderWrapper: latents + positional_encoding,
    wav2vec.py:222)."""
    M, D = x.shape
    check(lib().sbk_add_rows_periodic(ptr(x), M, D, ptr(pe), int(T), stream_of(x)), "sbk_add_rows_periodic")


@add_posenc.register_fake
def _(x, pe, T):
    return None


# ---------------------------------------------------------------------------
# The pre-training objective (csrc/w2vloss.hip): contrastive loss and the
# Gumbel vector quantiser.  fp32 device tensors; no CPU path.
_i32, _i64 = torch.int32, torch.int64


def _neg_strides(negs):
    """(row stride, negative stride) in floats of negs (N, B, T, C) whose
    (B, T) dims collapse to one row index (checked by the caller)."""
    return (negs.stride(2) if negs.shape[2] > 1 else negs.stride(1)), negs.stride(0)


@custom_op("sbk::w2v_contrast", mutates_args=())
def contrast(x: torch.Tensor, y: torch.Tensor, negs: Optional[torch.Tensor], idx: Optional[torch.Tensor],
             order: Optional[torch.Tensor], offs: Optional[torch.Tensor],
             temp: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """x, y (R, C) fp32; negs (N, B, T, C) fp32 or idx (R, N) int32 (exactly
    one).  Returns (rowloss (R), correct (R), logits (R, N+1), aux (R, 2)).
    order / offs: idx's inverse index, only carried for the backward."""
    R, C = x.shape
    N = negs.shape[0] if negs is not None else idx.shape[1]
    logits = torch.empty(R, N + 1, device=x.device, dtype=_f32)
    rowloss = torch.empty(R, device=x.device, dtype=_f32)
    correct = torch.empty(R, device=x.device, dtype=_f32)
    aux = torch.empty(R, 2, device=x.device, dtype=_f32)
    s_row, s_neg = _neg_strides(negs) if negs is not None else (0, 0)
    check(lib().sbk_w2v_contrast_fwd(ptr(x), ptr(y), ptr(negs), ptr(idx), R, C, N, s_row, s_neg, float(temp),
                                     ptr(logits), ptr(rowloss), ptr(correct), ptr(aux), stream_of(x)),
          "sbk_w2v_contrast_fwd")
    return rowloss, correct, logits, aux


@contrast.register_fake
def _(x, y, negs, idx, order, offs, temp):
    R = x.shape[0]
    N = negs.shape[0] if negs is not None else idx.shape[1]
    return x.new_empty(R), x.new_empty(R), x.new_empty(R, N + 1), x.new_empty(R, 2)


@custom_op("sbk::w2v_contrast_grad", mutates_args=())
def contrast_grad(x: torch.Tensor, y: torch.Tensor, negs: Optional[torch.Tensor], idx: Optional[torch.Tensor],
                  order: Optional[torch.Tensor], offs: Optional[torch.Tensor], logits: torch.Tensor,
                  aux: torch.Tensor, go: torch.Tensor, temp: float, need_dy: bool,
                  need_dnegs: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx (R, C), dy (R, C), dnegs (R, N, C)); a gradient that is not needed
    (or, for dnegs, does not exist in index mode) comes back empty."""
    R, C = x.shape
    N = logits.shape[1] - 1
    dev = x.device
    dx = torch.empty(R, C, device=dev, dtype=_f32)
    dy = torch.empty(R, C if need_dy else 0, device=dev, dtype=_f32)
    L = lib()
    if idx is None:
        dnegs = torch.empty(R, N, C if need_dnegs else 0, device=dev, dtype=_f32)
        s_row, s_neg = _neg_strides(negs)
        check(L.sbk_w2v_contrast_bwd_x(ptr(x), ptr(y), ptr(negs), None, ptr(logits), ptr(aux), ptr(go), R, C, N, s_row,
                                       s_neg, float(temp), ptr(dx), ptr(dy) if need_dy else None,
                                       ptr(dnegs) if need_dnegs else None, None, None, stream_of(x)),
              "sbk_w2v_contrast_bwd_x")
        return dx, dy, dnegs
    ca = torch.empty(R, N + 1, device=dev, dtype=_f32)
    cb = torch.empty(R, N + 1, device=dev, dtype=_f32)
    check(L.sbk_w2v_contrast_bwd_x(ptr(x), ptr(y), None, ptr(idx), ptr(logits), ptr(aux), ptr(go), R, C, N, 0, 0,
                                   float(temp), ptr(dx), None, None, ptr(ca), ptr(cb), stream_of(x)),
          "sbk_w2v_contrast_bwd_x")
    if need_dy:
        check(L.sbk_w2v_contrast_bwd_y(ptr(x), ptr(y), ptr(order), ptr(offs), ptr(ca), ptr(cb), R, C, N, ptr(dy),
                                       stream_of(x)), "sbk_w2v_contrast_bwd_y")
    return dx, dy, torch.empty(R, N, 0, device=dev, dtype=_f32)


@contrast_grad.register_fake
def _(x, y, negs, idx, order, offs, logits, aux, go, temp, need_dy, need_dnegs):
    R, C = x.shape
    N = logits.shape[1] - 1
    return (x.new_empty(R, C), x.new_empty(R, C if need_dy else 0),
            x.new_empty(R, N, C if need_dnegs and idx is None else 0))


def _contrast_setup(ctx, inputs, output):
    x, y, negs, idx, order, offs, temp = inputs
    ctx.save_for_backward(x, y, negs, idx, order, offs, output[2], output[3])
    ctx.temp = temp


def _contrast_backward(ctx, g_loss, g_correct, g_logits, g_aux):
    x, y, negs, idx, order, offs, logits, aux = ctx.saved_tensors
    need_dy = ctx.needs_input_grad[1]
    need_dn = negs is not None and ctx.needs_input_grad[2]
    if need_dy and idx is not None and order is None:
        raise RuntimeError("sbk::w2v_contrast: y requires grad in index mode but no inverse index was passed")
    go = g_loss.detach().to(_f32).contiguous()
    dx, dy, dn = contrast_grad(x, y, negs, idx, order, offs, logits, aux, go, ctx.temp, need_dy, need_dn)
    if need_dn:  # (R, N, C) -> the (N, B, T, C) view of the same memory
        dn = dn.view(negs.shape[1], negs.shape[2], negs.shape[0], negs.shape[3]).permute(2, 0, 1, 3)
    return dx, dy if need_dy else None, dn if need_dn else None, None, None, None, None


contrast.register_autograd(_contrast_backward, setup_context=_contrast_setup)


def inverse_index(idx):
    """idx (R, N) int32 rows of y referenced by row r's negatives → (order,
    offs): the pair ids r·(N+1) + j (j = 0 the positive, which references row
    r) sorted stably by referenced row, and each row's list start (R + 1).
    Device-side torch, once per forward."""
    R, N = idx.shape
    keys = torch.cat([torch.arange(R, device=idx.device, dtype=_i32)[:, None], idx], 1).reshape(-1)
    skeys, order = torch.sort(keys, stable=True)
    offs = torch.searchsorted(skeys, torch.arange(R + 1, device=idx.device, dtype=_i32))
    return order.contiguous(), offs.to(_i64).contiguous()


def contrastive_rows(x, y, negs, temp):
    """Per-row contrastive loss (R,), correct flags (R,) and logits (R, N+1)
    of x, y (B, T, C) and negs — float (N, B, T, C) or integer (B, T·N) flat
    row indices into y.view(-1, C).  Differentiable wrt x, y and float negs."""
    require_device(x, y, negs)
    if x.dim() != 3 or y.shape != x.shape:
        raise ValueError(f"expected x and y of one (B, T, C) shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    B, T, C = x.shape
    R = B * T
    x2 = x.float().reshape(R, C).contiguous()
    y2 = y.float().reshape(R, C).contiguous()
    if negs.is_floating_point():
        if negs.dim() != 4 or tuple(negs.shape[1:]) != (B, T, C):
            raise ValueError(f"expected negs (N, {B}, {T}, {C}), got {tuple(negs.shape)}")
        negs = negs.float()
        if negs.stride(3) != 1 or (B > 1 and T > 1 and negs.stride(1) != T * negs.stride(2)):
            negs = negs.contiguous()
        return contrast(x2, y2, negs, None, None, None, float(temp))[:3]
    if negs.dim() != 2 or negs.shape[0] != B or negs.shape[1] % T:
        raise ValueError(f"expected integer negs (B, T*N) = ({B}, {T}*N), got {tuple(negs.shape)}")
    idx = negs.reshape(R, -1).clamp(0, R - 1).to(_i32).contiguous()
    order = offs = None
    if torch.is_grad_enabled() and y2.requires_grad:
        order, offs = inverse_index(idx)
    return contrast(x2, y2, None, idx, order, offs, float(temp))[:3]


@custom_op("sbk::gumbel_vq", mutates_args=())
def gumbel_vq(logits: torch.Tensor, gumbels: Optional[torch.Tensor], vars: torch.Tensor, tau: float,
              groups: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """logits (Rq·G, V) fp32, gumbels the same shape (training) or None
    (eval), vars (G·V, D).  Returns (out (Rq, G·D), codes (Rq·G) int32 =
    g·V + chosen, counts (G·V) int32 of argmax(logits), psum (G·V) column
    sums of softmax(logits), ysoft (training; empty in eval))."""
    M, V = logits.shape
    G = int(groups)
    Rq = M // G
    ncodes, D = vars.shape
    dev = logits.device
    L = lib()
    out = torch.empty(Rq, G * D, device=dev, dtype=_f32)
    codes = torch.empty(M, device=dev, dtype=_i32)
    counts = torch.zeros(ncodes, device=dev, dtype=_i32)
    nparts = int(L.sbk_gumbel_vq_parts(Rq, G))
    part = torch.empty(max(nparts, 1), ncodes, device=dev, dtype=_f32)
    ysoft = torch.empty(M, V, device=dev, dtype=_f32) if gumbels is not None else torch.empty(0, device=dev, dtype=_f32)
    check(L.sbk_gumbel_vq_fwd(ptr(logits), ptr(gumbels), float(tau), Rq, G, V, ptr(vars), ncodes, D, ptr(out),
                              ptr(codes), ptr(counts), ptr(part), ptr(ysoft) if gumbels is not None else None,
                              stream_of(logits)), "sbk_gumbel_vq_fwd")
    psum = torch.empty(ncodes, device=dev, dtype=_f32)
    check(L.sbk_colsum(ptr(part), nparts, ncodes, ptr(psum), 0, stream_of(logits)), "sbk_colsum")
    return out, codes, counts, psum, ysoft


@gumbel_vq.register_fake
def _(logits, gumbels, vars, tau, groups):
    M, V = logits.shape
    ncodes, D = vars.shape
    return (logits.new_empty(M // groups, groups * D), logits.new_empty(M, dtype=_i32),
            logits.new_empty(ncodes, dtype=_i32), logits.new_empty(ncodes),
            logits.new_empty(M, V) if gumbels is not None else logits.new_empty(0))


@custom_op("sbk::gumbel_vq_grad", mutates_args=())
def gumbel_vq_grad(dout: torch.Tensor, gpsum: torch.Tensor, logits: torch.Tensor, vars: torch.Tensor,
                   codes: torch.Tensor, ysoft: Optional[torch.Tensor], tau: float,
                   groups: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(dlogits (Rq·G, V), dvars (G·V, D)): the straight-through term where
    ysoft is given, the gradient of the softmax column sums, and dout summed
    per chosen code over a stable sort of the codes."""
    M, V = logits.shape
    G = int(groups)
    ncodes, D = vars.shape
    dev = logits.device
    skeys, order = torch.sort(codes, stable=True)
    offs = torch.searchsorted(skeys, torch.arange(ncodes + 1, device=dev, dtype=_i32)).to(_i64)
    dlogits = torch.empty(M, V, device=dev, dtype=_f32)
    dvars = torch.empty(ncodes, D, device=dev, dtype=_f32)
    check(lib().sbk_gumbel_vq_bwd(ptr(dout), ptr(vars), ptr(logits), ptr(ysoft), ptr(gpsum), float(tau), ptr(order),
                                  ptr(offs), M // G, G, V, ncodes, D, ptr(dlogits), ptr(dvars), stream_of(logits)),
          "sbk_gumbel_vq_bwd")
    return dlogits, dvars


@gumbel_vq_grad.register_fake
def _(dout, gpsum, logits, vars, codes, ysoft, tau, groups):
    return torch.empty_like(logits), torch.empty_like(vars)


def _vq_setup(ctx, inputs, output):
    logits, gumbels, vars, tau, groups = inputs
    ctx.training = gumbels is not None
    ctx.save_for_backward(logits, vars, output[1], output[4])
    ctx.tau, ctx.groups = tau, groups


def _vq_backward(ctx, g_out, g_codes, g_counts, g_psum, g_ysoft):
    logits, vars, codes, ysoft = ctx.saved_tensors
    dlogits, dvars = gumbel_vq_grad(g_out.detach().float().contiguous(), g_psum.detach().float().contiguous(), logits,
                                    vars, codes, ysoft if ctx.training else None, ctx.tau, ctx.groups)
    return dlogits, None, dvars, None, None


gumbel_vq.register_autograd(_vq_backward, setup_context=_vq_setup)
