"""float64 restatement of the fused transducer head (csrc/thead.hip) on the
kernels' operand rounding, for the GPU tests of the head and of the RNN-T
loss (test infrastructure, CPU only).

    pre    = tn[b, t] + pn[b, u]                    fp32, as the kernel adds them
    z      = bf16(max(pre, slope * pre))            identity: slope 1, ReLU: 0
    logits = z . bf16(W)^T                          float64 from here on
    lp     = logits - lse
    nll_b  = -log P(y_b | x_b)                      oracle/rnnt.py lattice, float64
    dS     = scale[b] * (g_lp - softmax * sum_v g_lp)
    dtn    = sum_u dZ * act'(pre),  dpn = sum_t dZ * act'(pre),  dZ = dS . bf16(W)
    dW     = dS^T . z

g_lp is the un-normalised d(nll_b)/d(lp) the kernels produce in both loss
modes (the Numba semantics divide the loss by T_b and not its gradient);
scale[b] carries grad_output and, for the torchaudio mean, the 1/B.
test_transducer_ref_cpu.py pins all of it to torch.autograd in float64 and to
brute-force path enumeration.
"""
from types import SimpleNamespace

import numpy as np
import torch

import oracle.rnnt as OR

# name -> (act code of the C ABI, slope of max(v, slope * v) as the fp32 value
# the kernels receive, torch module factory)
ACTS = {
    "identity": (0, 1.0, lambda: torch.nn.Identity()),
    "relu": (6, 0.0, lambda: torch.nn.ReLU()),
    "leaky": (3, float(np.float32(0.01)), lambda: torch.nn.LeakyReLU(0.01)),
}


def joint_bf16(tn, pn, slope):
    """(pre fp32 (B, T, U1, J), z = bf16(act(pre)) as float64)."""
    tn, pn = tn.detach().cpu().float(), pn.detach().cpu().float()
    pre = tn[:, :, None, :] + pn[:, None, :, :]
    z = torch.maximum(pre, pre * slope).to(torch.bfloat16).double()
    return pre, z


def labels_other_than(rng, blank, V, shape):
    """Labels drawn from the V - 1 symbols that are not the blank."""
    y = rng.integers(0, V - 1, shape)
    return (y + (y >= blank)).astype(np.int32)


def head_reference(tn, pn, w, labels, Tl, Ul, blank, act="leaky", scale=None):
    """tn (B, T, J), pn (B, U1, J), w (V, J), labels (B, U1 - 1) ints (every
    label of a row u < U_b inside [0, V)), Tl / Ul absolute lengths, scale
    None (ones) or (B,).  Returns float64 tensors: z, logits, lse / lp_blank /
    lp_label (B, T, U1) (lp_label 0 at u = U1 - 1, NaN for a label outside
    [0, V)), nll (B,) = -log P, loss_numba = nll / T_b, gb / gl (B, T, U1), dS
    (B, T, U1, V), dtn, dpn, dW."""
    slope = ACTS[act][1]
    pre, z = joint_bf16(tn, pn, slope)
    wb = w.detach().cpu().float().to(torch.bfloat16).double()
    B, T, U1, _ = z.shape
    V = wb.shape[0]
    logits = z @ wb.t()
    lse = torch.logsumexp(logits, -1)
    lp = logits - lse[..., None]
    lab = np.asarray(labels).reshape(B, U1 - 1).astype(np.int64)
    Tl = np.asarray(Tl).astype(np.int64)
    Ul = np.asarray(Ul).astype(np.int64)
    lp_label = torch.zeros(B, T, U1, dtype=torch.float64)
    for b in range(B):
        for u in range(U1 - 1):
            y = int(lab[b, u])
            lp_label[b, :, u] = lp[b, :, u, y] if 0 <= y < V else float("nan")
    loss_numba, g_lp, _, _ = OR.transducer_forward(lp.numpy(), lab, Tl, Ul, blank, "none", dtype=np.float64)
    g_lp = torch.from_numpy(g_lp)
    gl = torch.zeros(B, T, U1, dtype=torch.float64)
    for b in range(B):
        for u in range(int(Ul[b])):
            gl[b, :, u] = g_lp[b, :, u, int(lab[b, u])]
    sc = torch.ones(B, dtype=torch.float64) if scale is None else torch.as_tensor(scale, dtype=torch.float64).reshape(B)
    dS = (g_lp - lp.exp() * g_lp.sum(-1, keepdim=True)) * sc.reshape(B, 1, 1, 1)
    da = (dS @ wb) * torch.where(pre >= 0, 1.0, slope).to(torch.float64)
    return SimpleNamespace(
        pre=pre, z=z, wb=wb, logits=logits, lse=lse, lp_blank=lp[..., blank], lp_label=lp_label,
        loss_numba=torch.from_numpy(np.asarray(loss_numba)), nll=torch.from_numpy(np.asarray(loss_numba) * Tl),
        gb=g_lp[..., blank], gl=gl, dS=dS, dtn=da.sum(2), dpn=da.sum(1),
        dW=dS.reshape(-1, V).t() @ z.reshape(B * T * U1, -1))


def reduce_loss(loss_b, reduction):
    """mean | sum | none of a (B,) loss, as Transducer.forward reduces."""
    return {"mean": loss_b.mean(), "sum": loss_b.sum(), "none": loss_b}[reduction]


def head_loss(ref, use_torchaudio, reduction):
    """The wrapper's loss from a head_reference result: use_torchaudio ->
    -log P, otherwise -log P / T_b (the Numba semantics)."""
    return reduce_loss(ref.nll if use_torchaudio else ref.loss_numba, reduction)


def grad_scale(B, use_torchaudio, reduction, grad_output=None):
    """scale[b] of the gradients for a wrapper call followed by
    backward(grad_output): grad_output itself (one value, or one per
    utterance for "none"), divided by B only for the torchaudio mean — the
    Numba semantics never normalise the gradients."""
    go = torch.ones(B, dtype=torch.float64) if grad_output is None else torch.as_tensor(
        grad_output, dtype=torch.float64).reshape(-1).expand(B).clone()
    return go / B if (use_torchaudio and reduction == "mean") else go
