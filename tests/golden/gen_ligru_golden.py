"""Generate tests/golden/ligru.npz from the REAL reference's LiGRU
(speechbrain/nnet/RNN.py:961-1325) on the CPU.

    python tests/golden/gen_ligru_golden.py

Runs only where the reference checkout is present (as gen_lstm_golden.py, whose
pattern this follows); the committed ligru.npz is what the tests read.  The
file holds data only.

Keys
  signature.LiGRU, signature.LiGRU_Layer
                  JSON [[parameter, kind, repr(default) | "<empty>"], ...] of __init__
  init.names; init.{n}.kw (JSON of the constructor's keyword arguments);
  init.{n}.sd.*   the state_dict right after torch.manual_seed(0) and construction
                  (re_init true / false x num_layers 1 / 2 x bidirectional)
  init.{n}.next   torch.rand(4) drawn right after that construction
  case.names; per case c (B 4, T 10, I 20, H 5):
    case.{c}.kw       JSON of LiGRU's keyword arguments
    case.{c}.train    1: the module is in training mode (the default), 0: eval
    case.{c}.calls    number of consecutive forward + backward calls (2 for "dropout")
    case.{c}.sd.*     the state_dict before the first call (construction under the case's own seed;
                      "bn_eval": running statistics set to drawn values)
    case.{c}.emb_kw   ("onehot") the Embedding's keyword arguments
    per call k = 0 ..:
    case.{c}.{k}.x    the input ((B, T, I), 4-D for "4d"; "onehot": case.{c}.{k}.tokens (B, T) int64)
    case.{c}.{k}.hx   where the case has it: (L, B, H), bidirectional (L, 2B, H)
    case.{c}.{k}.proj, .projh   the fixed randn of the scalar sum(output · proj) + sum(h · projh)
    case.{c}.{k}.out, .h; case.{c}.{k}.grad.{parameter}, .grad.x, .grad.hx
    case.{c}.{k}.after.*   the normalisation's buffers after the call (batchnorm in training)
"""
import inspect
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import gen_s2s_golden as S  # noqa: E402,F401  (installs the stubs, puts the reference on sys.path)

import torch  # noqa: E402
from speechbrain.nnet.RNN import LiGRU, LiGRU_Layer  # noqa: E402
from speechbrain.nnet.embedding import Embedding  # noqa: E402

SHAPE = (4, 10, 20)
INITS = {}
for _re in (True, False):
    for _l in (1, 2):
        for _bi in (False, True):
            INITS[f"re{int(_re)}_l{_l}_bi{int(_bi)}"] = dict(hidden_size=5, input_shape=SHAPE, num_layers=_l,
                                                            re_init=_re, bidirectional=_bi)

# name: (LiGRU kwargs, input shape, hx?, training?, calls)
CASES = {
    "doctest": (dict(hidden_size=5, input_shape=SHAPE), SHAPE, False, True, 1),
    "hx": (dict(hidden_size=5, input_shape=SHAPE), SHAPE, True, True, 1),
    "4d": (dict(hidden_size=5, input_shape=(4, 10, 5, 4)), (4, 10, 5, 4), False, True, 1),
    "layers2": (dict(hidden_size=5, input_shape=SHAPE, num_layers=2), SHAPE, True, True, 1),
    "bidir": (dict(hidden_size=5, input_shape=SHAPE, bidirectional=True), SHAPE, False, True, 1),
    "bidir_hx": (dict(hidden_size=5, input_shape=SHAPE, num_layers=2, bidirectional=True), SHAPE, True, True, 1),
    "layernorm": (dict(hidden_size=5, input_shape=SHAPE, normalization="layernorm", num_layers=2), SHAPE, True, True,
                  1),
    "none": (dict(hidden_size=5, input_shape=SHAPE, normalization="none"), SHAPE, False, True, 1),
    "act_relu": (dict(hidden_size=5, input_shape=SHAPE, nonlinearity="relu", bidirectional=True), SHAPE, True, False,
                 1),
    "act_leaky_relu": (dict(hidden_size=5, input_shape=SHAPE, nonlinearity="leaky_relu"), SHAPE, True, True, 1),
    "act_tanh": (dict(hidden_size=5, input_shape=SHAPE, nonlinearity="tanh"), SHAPE, True, True, 1),
    "act_sin": (dict(hidden_size=5, input_shape=SHAPE, nonlinearity="sin"), SHAPE, True, True, 1),
    "act_other": (dict(hidden_size=5, input_shape=SHAPE, nonlinearity="gelu"), SHAPE, False, True, 1),
    "bn_train": (dict(hidden_size=5, input_shape=SHAPE, num_layers=2, bidirectional=True), SHAPE, False, True, 2),
    "bn_eval": (dict(hidden_size=5, input_shape=SHAPE, num_layers=2, bidirectional=True), SHAPE, True, False, 1),
    "dropout": (dict(hidden_size=5, input_shape=SHAPE, dropout=0.3, num_layers=2, bidirectional=True), SHAPE, True,
                True, 2),
}
ONEHOT = dict(emb_kw=dict(num_embeddings=7, consider_as_one_hot=True, blank_id=3),
              kw=dict(hidden_size=5, input_shape=(4, 10, 6), normalization="layernorm"),
              tokens=[[3, 0, 6, 6, 2, 3, 1, 1, 5, 3], [3] * 10, [3, 5, 5, 1, 4, 0, 0, 2, 6, 4],
                      [3, 6, 2, 2, 2, 6, 3, 3, 0, 1]])


def signature(cls):
    return np.array(json.dumps(
        [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
         for p in inspect.signature(cls.__init__).parameters.values()]))


def kw_json(kw):
    return np.array(json.dumps({k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}))


def run_call(out, pre, net, x, hx, g):
    net.zero_grad(set_to_none=True)
    if hx is not None:
        hx = hx.clone().requires_grad_(True)
        out[pre + "hx"] = hx.detach().numpy().copy()
    y, h = net(x, hx=hx)
    proj = torch.randn(y.shape, generator=g)
    projh = torch.randn(h.shape, generator=g)
    ((y * proj).sum() + (h * projh).sum()).backward()
    out[pre + "proj"], out[pre + "projh"] = proj.numpy(), projh.numpy()
    out[pre + "out"] = y.detach().numpy().copy()
    out[pre + "h"] = h.detach().numpy().copy()
    for k, p in net.named_parameters():
        out[pre + "grad." + k] = p.grad.numpy().copy()
    if x.requires_grad:
        out[pre + "grad.x"] = x.grad.numpy().copy()
    if hx is not None:
        out[pre + "grad.hx"] = hx.grad.numpy().copy()
    for k, v in net.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out[pre + "after." + k] = v.numpy().copy()
    print(f"{pre} out {tuple(y.shape)}, h {tuple(h.shape)}")


def main():
    out = {"signature.LiGRU": signature(LiGRU), "signature.LiGRU_Layer": signature(LiGRU_Layer)}
    out["init.names"] = np.array(list(INITS), dtype="U16")
    for name, kw in INITS.items():
        torch.manual_seed(0)
        m = LiGRU(**kw)
        out[f"init.{name}.kw"] = kw_json(kw)
        for k, v in m.state_dict().items():
            out[f"init.{name}.sd.{k}"] = v.numpy().copy()
        out[f"init.{name}.next"] = torch.rand(4).numpy()
    out["case.names"] = np.array(list(CASES) + ["onehot"], dtype="U24")
    for i, (name, (kw, shape, with_hx, train, calls)) in enumerate(CASES.items()):
        torch.manual_seed(220 + i)
        net = LiGRU(**kw)
        g = torch.Generator().manual_seed(260 + i)
        H, L, D = kw["hidden_size"], kw.get("num_layers", 1), 2 if kw.get("bidirectional") else 1
        if name == "bn_eval":
            with torch.no_grad():
                for lay in net.rnn:
                    lay.norm.running_mean.copy_(0.3 * torch.randn(2 * H, generator=g))
                    lay.norm.running_var.copy_(0.5 + torch.rand(2 * H, generator=g))
        net.train(train)
        pre = f"case.{name}."
        out[pre + "kw"] = kw_json(kw)
        out[pre + "train"] = np.array(int(train))
        out[pre + "calls"] = np.array(calls)
        for k, v in net.state_dict().items():
            out[pre + "sd." + k] = v.numpy().copy()
        for c in range(calls):
            x = torch.rand(shape, generator=g).requires_grad_(True)
            hx = torch.randn(L, D * shape[0], H, generator=g) if with_hx else None
            out[f"{pre}{c}.x"] = x.detach().numpy().copy()
            run_call(out, f"{pre}{c}.", net, x, hx, g)
    torch.manual_seed(250)
    emb = Embedding(**ONEHOT["emb_kw"])
    net = LiGRU(**ONEHOT["kw"])
    tokens = torch.tensor(ONEHOT["tokens"])
    pre = "case.onehot."
    out[pre + "kw"] = kw_json(ONEHOT["kw"])
    out[pre + "emb_kw"] = kw_json(ONEHOT["emb_kw"])
    out[pre + "train"] = np.array(1)
    out[pre + "calls"] = np.array(1)
    out[pre + "0.tokens"] = tokens.numpy()
    for k, v in net.state_dict().items():
        out[pre + "sd." + k] = v.numpy().copy()
    run_call(out, pre + "0.", net, emb(tokens), torch.randn(1, 4, 5, generator=torch.Generator().manual_seed(251)),
             torch.Generator().manual_seed(252))
    path = os.path.join(OUT, "ligru.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
