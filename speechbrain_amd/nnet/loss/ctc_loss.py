"""CTC loss and the sequence-loss row kernel on HIP (speechbrain_amd/csrc/ctc.hip).

sbk::ctc / sbk::ctc_grad: the per-utterance CTC negative log-likelihood of
torch.nn.functional.ctc_loss(zero_infinity=True) (the function the reference's
ctc_loss calls, losses.py:245-294) on batch-first (B, T, V) fp32 log-probs or
logits, with torch's gradient convention wrt the log-probs
(exp(lp) - occupancy) or, for logits, softmax - occupancy in one pass.
sbk::nll_rows / sbk::nll_rows_grad: per row of a (B, U, V) log-prob tensor the
target's log-prob and the row sum — everything nll_loss and kldiv_loss need.

Lengths stay on the device: no host synchronisation, capturable in a graph.
fp32 device tensors only; CPU tensors raise SbkError (no fallback).
"""
import torch

from ..._lib import check, custom_op, lib, ptr, require_device, stream_of


@custom_op("sbk::ctc", mutates_args=())
def ctc(x: torch.Tensor, targets: torch.Tensor, in_len: torch.Tensor, tg_len: torch.Tensor, blank: int,
        is_logits: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """Gather (+ fused log-softmax) and the α/β lattice.  Returns (loss (B,),
    workspace kept for the backward)."""
    B, T, V = x.shape
    Lmax = targets.shape[1]
    L = lib()
    ws = torch.empty(int(L.sbk_ctc_workspace_floats(B, T, Lmax)), device=x.device, dtype=torch.float32)
    loss = torch.empty(B, device=x.device, dtype=torch.float32)
    check(L.sbk_ctc_forward(ptr(x), ptr(targets), ptr(in_len), ptr(tg_len), B, T, V, Lmax, int(blank),
                            int(is_logits), ptr(ws), ptr(loss), stream_of(x)), "sbk_ctc_forward")
    return loss, ws


@ctc.register_fake
def _(x, targets, in_len, tg_len, blank, is_logits):
    B, T, _ = x.shape
    Lmax = targets.shape[1]
    return x.new_empty(B), x.new_empty(5 * B * T * (2 * Lmax + 1) + B * T + 2 * B + B * Lmax)


@custom_op("sbk::ctc_grad", mutates_args=())
def ctc_grad(x: torch.Tensor, targets: torch.Tensor, in_len: torch.Tensor, tg_len: torch.Tensor, ws: torch.Tensor,
             go: torch.Tensor, blank: int, is_logits: bool) -> torch.Tensor:
    """Dense (B, T, V) gradient, rows scaled by go[b]."""
    B, T, V = x.shape
    grad = torch.empty_like(x)
    check(lib().sbk_ctc_backward(ptr(x), ptr(targets), ptr(in_len), ptr(tg_len), B, T, V, targets.shape[1],
                                 int(blank), int(is_logits), ptr(ws), ptr(go), ptr(grad), stream_of(x)),
          "sbk_ctc_backward")
    return grad


@ctc_grad.register_fake
def _(x, targets, in_len, tg_len, ws, go, blank, is_logits):
    return torch.empty_like(x)


def _ctc_setup(ctx, inputs, output):
    x, targets, in_len, tg_len, blank, is_logits = inputs
    ctx.save_for_backward(x, targets, in_len, tg_len, output[1])
    ctx.blank = blank
    ctx.is_logits = is_logits


def _ctc_backward(ctx, grad_loss, grad_ws):
    x, targets, in_len, tg_len, ws = ctx.saved_tensors
    go = grad_loss.detach().to(torch.float32).contiguous()
    return ctc_grad(x, targets, in_len, tg_len, ws, go, ctx.blank, ctx.is_logits), None, None, None, None, None


ctc.register_autograd(_ctc_backward, setup_context=_ctc_setup)


def ctc_nll(x, targets, in_len, tg_len, blank, is_logits):
    """Per-utterance CTC loss (B,) of x (B, T, V) fp32 with absolute lengths."""
    require_device(x, targets, in_len, tg_len)
    if x.dtype != torch.float32:
        raise TypeError("CTC loss kernels take fp32 logits / log-probs")
    if x.dim() != 3 or targets.dim() != 2 or targets.shape[0] != x.shape[0]:
        raise ValueError(f"expected (B, T, V) inputs and (B, L) targets, got {tuple(x.shape)} and "
                         f"{tuple(targets.shape)}")
    x = x.contiguous()
    tg = targets.to(device=x.device, dtype=torch.int32).contiguous()
    il = in_len.to(device=x.device, dtype=torch.int32).contiguous()
    tl = tg_len.to(device=x.device, dtype=torch.int32).contiguous()
    return ctc(x, tg, il, tl, int(blank), bool(is_logits))[0]


@custom_op("sbk::nll_rows", mutates_args=())
def nll_rows(x: torch.Tensor, targets: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """x (B, U, V) fp32 with contiguous rows (any batch stride), targets
    (B, U) int32 -> (x[b, u, targets[b, u]], sum_v x[b, u, v]), each (B, U)."""
    B, U, V = x.shape
    sel = torch.empty(B, U, device=x.device, dtype=torch.float32)
    rsum = torch.empty(B, U, device=x.device, dtype=torch.float32)
    check(lib().sbk_nll_rows_forward(ptr(x), ptr(targets), B, U, x.stride(0), V, ptr(sel), ptr(rsum), stream_of(x)),
          "sbk_nll_rows_forward")
    return sel, rsum


@nll_rows.register_fake
def _(x, targets):
    B, U, _ = x.shape
    return x.new_empty(B, U), x.new_empty(B, U)


@custom_op("sbk::nll_rows_grad", mutates_args=())
def nll_rows_grad(targets: torch.Tensor, a: torch.Tensor, c: torch.Tensor, V: int) -> torch.Tensor:
    """grad[b, u, v] = a[b, u]·[v == targets[b, u]] + c[b, u], (B, U, V)."""
    B, U = targets.shape
    grad = torch.empty(B, U, V, device=a.device, dtype=torch.float32)
    check(lib().sbk_nll_rows_backward(ptr(targets), ptr(a), ptr(c), B, U, U * V, V, ptr(grad), stream_of(a)),
          "sbk_nll_rows_backward")
    return grad


@nll_rows_grad.register_fake
def _(targets, a, c, V):
    return a.new_empty(*targets.shape, V)


def _rows_setup(ctx, inputs, output):
    x, targets = inputs
    ctx.save_for_backward(targets)
    ctx.V = x.shape[2]


def _rows_backward(ctx, g_sel, g_sum):
    (targets,) = ctx.saved_tensors
    a = g_sel.detach().to(torch.float32).contiguous()
    c = g_sum.detach().to(torch.float32).contiguous()
    return nll_rows_grad(targets, a, c, ctx.V), None


nll_rows.register_autograd(_rows_backward, setup_context=_rows_setup)


def row_stats(log_probs, targets):
    """(lp[b, u, targets[b, u]], sum_v lp[b, u, v]) of log_probs (B, U, V) and
    targets (B, U), differentiable wrt log_probs.  A U-slice of a contiguous
    tensor is taken as it is (batch stride), not copied."""
    require_device(log_probs, targets)
    if log_probs.dtype != torch.float32:
        raise TypeError("sequence loss kernels take fp32 log-probabilities")
    B, U, V = log_probs.shape
    x = log_probs
    if x.stride(2) != 1 or x.stride(1) != V or x.stride(0) < U * V:
        x = x.contiguous()
    tg = targets.to(device=x.device, dtype=torch.int32).contiguous()
    return nll_rows(x, tg)
