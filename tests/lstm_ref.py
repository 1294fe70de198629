"""float64 restatement of the LSTM the drop-in computes (torch.nn.LSTM's
equations, gate order i, f, g, o, batch first, one or two directions) with the
per-row step mask that stands for the reference's pack_padded_sequence /
pad_packed_sequence pair.  test_lstm_cpu.py holds it to the reference's own
outputs and gradients (tests/golden/lstm.npz) at 1e-6 and to torch's packed
float64 bidirectional LSTM; the GPU tests then use it as their oracle.

    i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)    f = sigmoid(W_if x + b_if + W_hf h + b_hf)
    g = tanh(W_ig x + b_ig + W_hg h + b_hg)       o = sigmoid(W_io x + b_io + W_ho h + b_ho)
    c' = f * c + i * g                            h' = o * tanh(c')

The mask: a row with t >= steps[b] keeps (h, c) and its output row is zero.
The reverse direction scans t = T-1 .. 0 under the same mask, so a row carries
(h0, c0) through its padding and starts at t = steps[b] - 1.

round_bf16: W_ih, W_hh and the h operand of the recurrent product are rounded
to bf16 (straight-through for the gradients) — the yardstick of the bf16
kernels, whose (h, c) state stays fp32.
"""
import torch

from rnn_ref import _rb, onehot_table, steps_of  # noqa: F401  (shared with the GRU's restatement)

NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def layer_params(sd, layer, D=1, dtype=torch.float64, prefix="rnn."):
    """Per direction (w_ih, w_hh, b_ih | None, b_hh | None) of a layer from a state dict, as leaf tensors."""
    out = []
    for sfx in ("", "_reverse")[:D]:
        ps = []
        for n in NAMES:
            k = f"{prefix}{n}_l{layer}{sfx}"
            ps.append(torch.as_tensor(sd[k]).detach().to(dtype).clone().requires_grad_(True) if k in sd else None)
        out.append(tuple(ps))
    return out


def lstm_ref(x, params, hx=None, steps=None, round_bf16=False):
    """x (B, T, I); params: per layer a list over directions of (w_ih, w_hh,
    b_ih | None, b_hh | None); hx: (h0, c0), each (L * D, B, H), or None; steps
    (B,) int or None.  Returns (output (B, Tn, D * H), (hn, cn) each
    (L * D, B, H)), Tn = max(steps)."""
    B, T = x.shape[:2]
    if steps is not None:
        T = int(steps.max())
        x = x[:, :T]
    inp, hns, cns = x, [], []
    for l, dirs in enumerate(params):
        D = len(dirs)
        outs_d = []
        for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(dirs):
            H = w_hh.shape[1]
            if round_bf16:
                w_ih, w_hh = _rb(w_ih), _rb(w_hh)
            h = hx[0][l * D + d] if hx is not None else torch.zeros(B, H, dtype=x.dtype)
            c = hx[1][l * D + d] if hx is not None else torch.zeros(B, H, dtype=x.dtype)
            gi = inp @ w_ih.t()
            if b_ih is not None:
                gi = gi + b_ih
            outs = [None] * T
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                gh = (_rb(h) if round_bf16 else h) @ w_hh.t()
                if b_hh is not None:
                    gh = gh + b_hh
                pre = gi[:, t] + gh
                i, f = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H])
                g, o = torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
                cnew = f * c + i * g
                hnew = o * torch.tanh(cnew)
                if steps is not None:
                    act = (t < steps).to(x.dtype).unsqueeze(1)
                    h = act * hnew + (1 - act) * h
                    c = act * cnew + (1 - act) * c
                    outs[t] = act * hnew
                else:
                    h, c = hnew, cnew
                    outs[t] = h
            outs_d.append(torch.stack(outs, 1))
            hns.append(h)
            cns.append(c)
        inp = torch.cat(outs_d, 2)
    return inp, (torch.stack(hns, 0), torch.stack(cns, 0))
