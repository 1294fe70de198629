"""Restatement of the LiGRU the drop-in computes (speechbrain/nnet/RNN.py:961-
1325 of the reference), in the dtype of its inputs: float64 as the oracle of
the GPU tests, float32 as their E32 yardstick.  test_ligru_cpu.py holds it to
the reference's own outputs and gradients (tests/golden/ligru.npz) at 1e-6.

Per layer, literally as the reference: a bidirectional layer runs on
cat([x, x.flip(1)], 0), one Linear w, one normalisation over the (doubled)
rows, then

    gates = wn[:, t] + h_{t-1} U^T ;  a, zpre = gates.chunk(2)
    z = sigmoid(zpre) ;  hc = act(a) * mask ;  h_t = z * h_{t-1} + (1 - z) * hc

and the second half of the batch is flipped back next to the first.  The
returned h is x[:, -1] per layer, stacked, then transposed (one direction) or
reshaped raw (two), as the reference does it.

round_bf16: x, w, u and the h_{t-1} operand of the recurrent product are
rounded to bf16 (straight-through for the gradients) — the yardstick of the
bf16 kernels, whose state and normalisation stay fp32.
"""
import torch

from rnn_ref import _rb, onehot_table  # noqa: F401  (shared with the GRU's restatement)

ACTS = {"tanh": torch.tanh, "sin": torch.sin, "leaky_relu": lambda a: torch.nn.functional.leaky_relu(a, 0.01)}
EPS = 1e-5
MOMENTUM = 0.05


def layer_params(sd, layer, dtype=torch.float64, prefix="rnn."):
    """{w, u, gamma, beta} as leaves and {rmean, rvar} (batchnorm) of a layer from a state dict."""
    p = {}
    for n, k in (("w", "w.weight"), ("u", "u.weight"), ("gamma", "norm.weight"), ("beta", "norm.bias")):
        p[n] = torch.as_tensor(sd[f"{prefix}{layer}.{k}"]).detach().to(dtype).clone().requires_grad_(True)
    for n, k in (("rmean", "norm.running_mean"), ("rvar", "norm.running_var")):
        if f"{prefix}{layer}.{k}" in sd:
            p[n] = torch.as_tensor(sd[f"{prefix}{layer}.{k}"]).detach().to(dtype).clone()
    return p


def ligru_layer_ref(x, p, hx=None, mask=None, nonlinearity="relu", training=True, bidirectional=False,
                    round_bf16=False, info=None):
    """x (B, T, I); p as layer_params gives it (batchnorm if it has rmean);
    hx, mask (D * B, H) or None.  Updates p's running statistics when training.
    info (a dict) receives min_abs_a, the smallest |a| seen (the ReLU kink)."""
    act = ACTS.get(nonlinearity, torch.relu)
    w, u = p["w"], p["u"]
    H = u.shape[1]
    if bidirectional:
        x = torch.cat([x, x.flip(1)], 0)
    if round_bf16:
        x, w, u = _rb(x), _rb(w), _rb(u)
    rows, T = x.shape[:2]
    flat = (x @ w.t()).reshape(rows * T, 2 * H)
    if "rmean" in p:
        if training:
            n = rows * T
            mean, var = flat.mean(0), flat.var(0, unbiased=False)
            with torch.no_grad():
                p["rmean"] = (1 - MOMENTUM) * p["rmean"] + MOMENTUM * mean.detach()
                p["rvar"] = (1 - MOMENTUM) * p["rvar"] + MOMENTUM * var.detach() * n / (n - 1)
        else:
            mean, var = p["rmean"], p["rvar"]
        wn = (flat - mean) / torch.sqrt(var + EPS)
    else:
        mean, var = flat.mean(1, keepdim=True), flat.var(1, unbiased=False, keepdim=True)
        wn = (flat - mean) / torch.sqrt(var + EPS)
    wn = (wn * p["gamma"] + p["beta"]).reshape(rows, T, 2 * H)
    h = hx if hx is not None else x.new_zeros(1, H)
    hs = []
    for k in range(T):
        gates = wn[:, k] + (_rb(h) if round_bf16 else h) @ u.t()
        a, z = gates[:, :H], torch.sigmoid(gates[:, H:])
        if info is not None:
            info["min_abs_a"] = min(info.get("min_abs_a", float("inf")), float(a.detach().abs().min()))
        hc = act(a)
        if mask is not None:
            hc = hc * mask
        h = z * h + (1 - z) * hc
        hs.append(h)
    h = torch.stack(hs, 1)
    if bidirectional:
        hf, hb = h.chunk(2, 0)
        h = torch.cat([hf, hb.flip(1)], 2)
    return h


def ligru_ref(x, params, hx=None, masks=None, nonlinearity="relu", training=True, bidirectional=False, batch_size=None,
              round_bf16=False, info=None):
    """x (B, T, I); params: per layer a dict of layer_params; hx (L, B, H), or
    for two directions anything that reshapes to (L, 2 * batch_size, H);
    masks: per layer (D * B, H) or None.  Returns (output (B, T, D * H), h)."""
    L = len(params)
    H = params[0]["u"].shape[1]
    if hx is not None and bidirectional:
        hx = hx.reshape(L, (batch_size or x.shape[0]) * 2, H)
    hs = []
    for i, p in enumerate(params):
        x = ligru_layer_ref(x, p, None if hx is None else hx[i], None if masks is None else masks[i], nonlinearity,
                            training, bidirectional, round_bf16, info)
        hs.append(x[:, -1, :])
    h = torch.stack(hs, 1)
    h = h.reshape(h.shape[1] * 2, h.shape[0], H) if bidirectional else h.transpose(0, 1)
    return x, h
