"""Host side of csrc/attdec.hip: the attentional GRU decoder's sequence call
(sbk_attdec_fwd / sbk_attdec_bwd) with the GEMMs that do not depend on the
recurrence taken out of the loop, as one autograd Function, and the
grad-free single steps the searchers use (forward_step, a standalone
attention call).  See DESIGN.md §3 "Attentional decoder"."""
import torch

from . import _autograd as A
from . import _enc
from ._lib import check, lib, ptr, stream_of

_f32 = torch.float32
_bf16 = torch.bfloat16


def score_tile():
    """Frames per workgroup of the score kernel."""
    return int(lib().sbk_attdec_tile())


def _t(cache, key, w, dtype, rows=None):
    """Cached kernel copy of w[rows]^T."""
    return cache.get(f"{key}T{int(dtype == _bf16)}", [w], lambda: _enc.to_compute(
        (w.detach() if rows is None else w.detach()[:, rows]).t(), dtype))


def _part(cache, key, w, dtype, cols):
    """Cached kernel copy of the column block w[:, cols]."""
    return cache.get(f"{key}{int(dtype == _bf16)}", [w], lambda: _enc.to_compute(w.detach()[:, cols], dtype))


def _loc(w_conv, w_loc):
    if w_loc is None:
        return None, None, 0, 0
    C, _, KW = w_conv.shape
    return A._cont(w_conv.detach().float().reshape(C, KW)), A._cont(w_loc.detach().float()), C, (KW - 1) // 2


def precompute(enc, w_enc, b_enc, dtype, cache):
    """mlp_enc(enc_states) (B, L, A) fp32 on the MFMA GEMM."""
    B, L, E = enc.shape
    P = _enc.gemm(_enc.to_compute(enc.detach().reshape(B * L, E), dtype), A.kernel_weight(w_enc, dtype, cache, "enc"),
                  bias=None if b_enc is None else b_enc.detach())
    return P.view(B, L, -1)


def run_fwd(dtype, cache, W, gx, mc, P, enc, len32, h0, c0, attn0, scaling, T, save):
    """The launches of T steps.  W: the module's weights by name; gx None:
    attention only (h0 is the query's input).  Returns (hstate, cstate, ctx,
    attn, dech, save)."""
    B, L, E = enc.shape
    dev = enc.device
    Adim, H = W["w_dec"].shape
    O = W["w_out"].shape[0]
    cell = gx is not None
    wconv, wloc, C, ksz = _loc(W.get("w_conv"), W.get("w_loc"))
    b_q = W["b_dec"].detach() if wloc is None else W["b_dec"].detach() + W["b_loc"].detach()
    new = lambda *s: torch.empty(*s, device=dev, dtype=_f32)  # noqa: E731
    hstate = new(B, T, H) if cell else h0.detach().float().contiguous().view(B, 1, H)
    cstate, ctxs, attn, dech = new(B, T, O), new(B, T, E), new(B, T, L), new(B, T, Adim)
    sv = new(B, T, 4, H) if save else None
    nt = -(-L // score_tile())
    ws = new(B * (O + L + nt * (2 + E)))
    I = W["w_ih"].shape[1] - O if cell else 0
    w_ic = _part(cache, "ic", W["w_ih"], dtype, slice(I, None)) if cell else None
    w_hh = A.kernel_weight(W["w_hh"], dtype, cache, "hh") if cell else None
    check(lib().sbk_attdec_fwd(
        int(dtype == _bf16), ptr(w_ic), ptr(w_hh), ptr(W["b_hh"].detach() if cell and W["b_hh"] is not None else None),
        ptr(A.kernel_weight(W["w_dec"], dtype, cache, "dec")), ptr(b_q),
        ptr(A.kernel_weight(W["w_out"], dtype, cache, "out")), ptr(W["b_out"].detach()), ptr(gx), ptr(mc), ptr(P),
        ptr(enc), ptr(len32), ptr(wconv), ptr(wloc), ptr(A._cont(W["w_attn"].detach().float().reshape(-1))),
        float(scaling), ptr(h0 if cell else None), ptr(c0), ptr(attn0), B, T, L, H, Adim, O, E, C, ksz, ptr(hstate),
        ptr(cstate), ptr(ctxs), ptr(attn), ptr(dech), ptr(sv), ptr(ws), stream_of(enc)), "sbk_attdec_fwd")
    return hstate, cstate, ctxs, attn, dech, sv


NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w_enc", "b_enc", "w_dec", "b_dec", "w_attn", "w_out", "b_out", "w_proj",
         "b_proj", "w_conv", "w_loc", "b_loc")


def weights_of(dec):
    """The decoder's parameters in NAMES order (None where it has none)."""
    cell, at = dec.rnn.rnn_cells[0], dec.attn
    loc = hasattr(at, "conv_loc")
    return (cell.weight_ih, cell.weight_hh, getattr(cell, "bias_ih", None), getattr(cell, "bias_hh", None),
            at.mlp_enc.weight, at.mlp_enc.bias, at.mlp_dec.weight, at.mlp_dec.bias, at.mlp_attn.weight,
            at.mlp_out.weight, at.mlp_out.bias, dec.proj.weight, dec.proj.bias,
            at.conv_loc.weight if loc else None, at.mlp_loc.weight if loc else None, at.mlp_loc.bias if loc else None)


def _gx(x2, W, I, dtype, cache):
    return _enc.gemm(_enc.to_compute(x2, dtype), _part(cache, "ihx", W["w_ih"], dtype, slice(0, I)),
                     bias=None if W["b_ih"] is None else W["b_ih"].detach())


def _project(cstate, hstate, W, dtype, cache):
    B, T = cstate.shape[:2]
    ch = torch.cat([cstate, hstate], -1).view(B * T, -1)
    out = _enc.gemm(_enc.to_compute(ch, dtype), A.kernel_weight(W["w_proj"], dtype, cache, "proj"),
                    bias=W["b_proj"].detach())
    return out.view(B, T, -1), ch


class AttDecFn(torch.autograd.Function):
    """AttentionalRNNDecoder.forward: inp (B, T, I), enc (B, L, E), len32 (B)
    int32, mask (B, T, I + A) dropout keep-mask or None, attn0 (B, L) or None
    -> (outputs (B, T, H), attn (B, T, L), P)."""

    @staticmethod
    def forward(ctx, inp, enc, len32, mask, attn0, scaling, dtype, cache, *weights):
        W = dict(zip(NAMES, weights))
        B, T, I = inp.shape
        enc_c = enc.detach().float().contiguous()
        O = W["w_out"].shape[0]
        x = inp.detach().float()
        mc = None
        if mask is not None:
            x = x * mask[..., :I]
            mc = mask[..., I:].contiguous()
        gx = _gx(x.reshape(B * T, I), W, I, dtype, cache)
        P = precompute(enc_c, W["w_enc"], W["b_enc"], dtype, cache)
        need = any(ctx.needs_input_grad)
        hstate, cstate, ctxs, attn, dech, sv = run_fwd(dtype, cache, W, gx, mc, P, enc_c, len32, None, None, attn0,
                                                       scaling, T, need)
        out, ch = _project(cstate, hstate, W, dtype, cache)
        if need:
            ctx.save_for_backward(x, enc_c, len32, mc, attn0, P, hstate, cstate, ctxs, attn, dech, sv, *weights)
            ctx.cfg = (scaling, dtype, cache, inp.dtype, enc.dtype, None if mask is None else mask[..., :I])
        ctx.mark_non_differentiable(P)
        return out, attn, P

    @staticmethod
    def backward(ctx, dout, dattn, _dP):
        x, enc, len32, mc, attn0, P, hstate, cstate, ctxs, attn, dech, sv, *weights = ctx.saved_tensors
        scaling, dtype, cache, inp_dt, enc_dt, minp = ctx.cfg
        W = dict(zip(NAMES, weights))
        B, T, I = x.shape
        L, E = enc.shape[1:]
        H, O, Adim = hstate.shape[2], cstate.shape[2], dech.shape[2]
        dev = x.device
        bf = int(dtype == _bf16)
        zeros = lambda *s: torch.zeros(*s, device=dev, dtype=_f32)  # noqa: E731
        new = lambda *s: torch.empty(*s, device=dev, dtype=_f32)  # noqa: E731
        dout2 = (zeros(B * T, H) if dout is None else dout.detach().float().contiguous().view(B * T, H))
        dattn = None if dattn is None else dattn.detach().float().contiguous()
        # d [C_all | H_all] from d outputs in one GEMM
        dch = _enc.gemm(A._as(dout2, dtype), _t(cache, "proj", W["w_proj"], dtype))
        dcall = dch[:, :O].contiguous().view(B, T, O)
        dhproj = dch[:, O:].contiguous().view(B, T, H)
        wconv, wloc, C, ksz = _loc(W["w_conv"], W["w_loc"])
        nt = -(-L // score_tile())
        dgi, dgh, dctx, ddech = new(B, T, 3 * H), new(B, T, 3 * H), new(B, T, E), new(B, T, Adim)
        dP = zeros(B, L, Adim)
        width = Adim + Adim * C + C * (2 * ksz + 1)
        slots = zeros(B * nt, width)
        ws = new(2 * B * H + B * nt * Adim)
        check(lib().sbk_attdec_bwd(
            bf, ptr(_t(cache, "ic", W["w_ih"], dtype, slice(I, None))), ptr(_t(cache, "hh", W["w_hh"], dtype)),
            ptr(_t(cache, "dec", W["w_dec"], dtype)), ptr(_t(cache, "out", W["w_out"], dtype)), ptr(P), ptr(enc),
            ptr(len32), ptr(wconv), ptr(wloc), ptr(A._cont(W["w_attn"].detach().float().reshape(-1))), float(scaling),
            None, ptr(attn0), ptr(mc), ptr(hstate), ptr(ctxs), ptr(attn), ptr(dech), ptr(sv), ptr(dattn), ptr(dhproj),
            B, T, L, H, Adim, O, E, C, ksz, ptr(dcall), ptr(dgi), ptr(dgh), ptr(dctx), ptr(dP), ptr(ddech), ptr(slots),
            ptr(ws), stream_of(x)), "sbk_attdec_bwd")
        gi2, gh2, dq2, dc2, dP2 = (dgi.view(B * T, -1), dgh.view(B * T, -1), ddech.view(B * T, -1),
                                   dcall.view(B * T, O), dP.view(B * L, Adim))
        first = zeros(B, 1, H)
        hprev = torch.cat([first, hstate[:, :T - 1]], 1).reshape(B * T, H)
        cprev = torch.cat([zeros(B, 1, O), cstate[:, :T - 1]], 1)
        if mc is not None:
            cprev = cprev * mc
        cell_in = torch.cat([x, cprev], -1).view(B * T, I + O)
        red = A.colsum(slots, B * nt, width)
        ch = torch.cat([cstate, hstate], -1).view(B * T, O + H)
        g = {
            # fp32 operands for dW_ih in both modes, as the GRU layer's input gradient (RNN.py)
            "w_ih": A.wgrad(gi2, cell_in),
            "w_hh": A.wgrad(A._as(gh2, dtype), A._as(hprev, dtype)),
            "b_ih": A.rowsum(gi2), "b_hh": A.rowsum(gh2),
            "w_enc": A.wgrad(A._as(dP2, dtype), A._as(enc.view(B * L, E), dtype)),
            "w_dec": A.wgrad(A._as(dq2, dtype), A._as(hstate.view(B * T, H), dtype)),
            "b_dec": A.rowsum(dq2),
            "w_attn": red[:Adim].reshape(1, Adim),
            "w_out": A.wgrad(A._as(dc2, dtype), A._as(ctxs.view(B * T, E), dtype)),
            "b_out": A.rowsum(dc2),
            "w_proj": A.wgrad(A._as(dout2, dtype), A._as(ch, dtype)),
            "b_proj": A.rowsum(dout2),
        }
        # every bias that enters e sees the same sum of de
        g["b_enc"] = g["b_dec"].clone()
        if wloc is not None:
            g["b_loc"] = g["b_dec"].clone()
            g["w_loc"] = red[Adim:Adim + Adim * C].reshape(Adim, C)
            g["w_conv"] = red[Adim + Adim * C:].reshape(C, 1, 2 * ksz + 1)
        dinp = _enc.gemm(A._as(gi2, dtype), _t(cache, "ihx", W["w_ih"], dtype, slice(0, I))).view(B, T, I)
        if minp is not None:
            dinp = dinp * minp
        # d enc = dP W_enc + sum_t attn_t (x) dctx_t, the second as one (L x T)(T x E) product per row
        denc = _enc.gemm(A._as(dP2, dtype), _t(cache, "enc", W["w_enc"], dtype)).view(B, L, E) + _enc.gemm_tn(attn, dctx)
        grads = [g.get(n) if w is not None else None for n, w in zip(NAMES, weights)]
        return (dinp.to(inp_dt), denc.to(enc_dt), None, None, None, None, None, None, *grads)


def step(dec, inp, h0, c0, P, enc, len32, attn0):
    """One grad-free decoder step: (dec_out (B, H), h (B, H), c (B, A), attn (B, L))."""
    W = dict(zip(NAMES, weights_of(dec)))
    dtype, cache = _enc.compute_dtype(), dec._wc
    I = inp.shape[1]
    gx = _gx(inp.detach().float(), W, I, dtype, cache)
    enc_c = enc.detach().float().contiguous()
    hstate, cstate, _, attn, _, _ = run_fwd(dtype, cache, W, gx, None, P, enc_c, len32, h0, c0, attn0, dec.scaling, 1,
                                            False)
    out, _ = _project(cstate, hstate, W, dtype, cache)
    return out[:, 0], hstate[:, 0], cstate[:, 0], attn[:, 0]


def attend(at, enc, dec_states, attn0):
    """One grad-free attention call of module at: (context (B, O), attn (B, L))."""
    loc = hasattr(at, "conv_loc")
    W = {"w_dec": at.mlp_dec.weight, "b_dec": at.mlp_dec.bias, "w_attn": at.mlp_attn.weight,
         "w_out": at.mlp_out.weight, "b_out": at.mlp_out.bias}
    if loc:
        W.update(w_conv=at.conv_loc.weight, w_loc=at.mlp_loc.weight, b_loc=at.mlp_loc.bias)
    enc_c = enc.detach().float().contiguous()
    _, cstate, _, attn, _, _ = run_fwd(_enc.compute_dtype(), at._wc, W, None, None, at.precomputed_enc_h, enc_c,
                                       at._len32, dec_states, None, attn0, at.scaling, 1, False)
    return cstate[:, 0], attn[:, 0]
