"""float64 restatement of the GRU the drop-in computes (torch.nn.GRU's
equations, gate order r, z, n, batch first) with the per-row step mask that
stands for the reference's pack_padded_sequence / pad_packed_sequence pair.
test_rnn_cpu.py holds it to the reference's own outputs and gradients
(tests/golden/rnn.npz) at 1e-6; the GPU tests then use it as their oracle.

    r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)
    z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn))
    h' = (1 - z) * n + z * h

round_bf16: W_ih, W_hh and the h_{t-1} operand of the recurrent product are
rounded to bf16 (straight-through for the gradients) — the yardstick of the
bf16 kernels, whose state stays fp32.
"""
import torch


def steps_of(lengths, T):
    """Steps per row as torch's packing derives them from the relative lengths."""
    return (torch.as_tensor(lengths, dtype=torch.float32) * T).to(torch.int64)


def _rb(t):
    return t + (t.detach().float().bfloat16().to(t.dtype) - t.detach())


def layer_params(sd, layer, dtype=torch.float64, prefix="rnn."):
    """(w_ih, w_hh, b_ih | None, b_hh | None) of a layer from a state dict, as leaf tensors."""
    out = []
    for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
        k = f"{prefix}{n}_l{layer}"
        out.append(torch.as_tensor(sd[k]).detach().to(dtype).clone().requires_grad_(True) if k in sd else None)
    return tuple(out)


def gru_ref(x, params, hx=None, steps=None, round_bf16=False):
    """x (B, T, I); params: per layer (w_ih, w_hh, b_ih | None, b_hh | None);
    hx (L, B, H) or None; steps (B,) int or None.  Returns (output (B, Tn, H),
    hn (L, B, H)), Tn = max(steps)."""
    B, T = x.shape[:2]
    if steps is not None:
        T = int(steps.max())
        x = x[:, :T]
    inp, hns = x, []
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(params):
        H = w_hh.shape[1]
        if round_bf16:
            w_ih, w_hh = _rb(w_ih), _rb(w_hh)
        h = hx[l] if hx is not None else torch.zeros(B, H, dtype=x.dtype)
        gi = inp @ w_ih.t()
        if b_ih is not None:
            gi = gi + b_ih
        outs = []
        for t in range(T):
            gh = (_rb(h) if round_bf16 else h) @ w_hh.t()
            if b_hh is not None:
                gh = gh + b_hh
            r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
            hnew = (1 - z) * n + z * h
            if steps is not None:
                act = (t < steps).to(x.dtype).unsqueeze(1)
                h = act * hnew + (1 - act) * h
                outs.append(act * hnew)
            else:
                h = hnew
                outs.append(h)
        inp = torch.stack(outs, 1)
        hns.append(h)
    return inp, torch.stack(hns, 0)


def onehot_table(V, blank, dtype=torch.float64):
    """The frozen table of Embedding(V, consider_as_one_hot=True, blank_id=blank)."""
    tab = torch.zeros(V, V - 1, dtype=dtype)
    for v in range(V):
        if v != blank:
            tab[v, v if v < blank else v - 1] = 1
    return tab
