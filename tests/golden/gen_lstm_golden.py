"""Generate tests/golden/lstm.npz from the REAL reference's LSTM
(speechbrain/nnet/RNN.py) on the CPU.

    python tests/golden/gen_lstm_golden.py

Runs only where the reference checkout is present (as gen_rnn_golden.py, whose
pattern this follows); the committed lstm.npz is what the tests read.  The file
holds data only.

Keys
  signature.LSTM  JSON [[parameter, kind, repr(default) | "<empty>"], ...] of __init__
  init.names; init.{n}.kw (JSON of the constructor's keyword arguments);
  init.{n}.sd.*   the state_dict right after torch.manual_seed(0) and construction
                  (re_init true / false x num_layers 1 / 2 x bidirectional, bias false)
  init.{n}.next   torch.rand(4) drawn right after that construction
  case.names; per case c (B 4, T 10, I 20, H 5):
    case.{c}.kw       JSON of LSTM's keyword arguments
    case.{c}.sd.*     the LSTM's state_dict (construction under the case's own seed)
    case.{c}.x        the input ((B, T, I), 4-D for "4d"; "onehot": case.{c}.tokens (B, T) int64, case.{c}.emb_kw)
    case.{c}.hx, case.{c}.cx (L * D, B, H), case.{c}.lengths (B) where the case has them
    case.{c}.steps    the integer lengths torch's packing used (cases with lengths)
    case.{c}.proj, .projh, .projc   the fixed randn of the scalar
                      sum(output · proj) + sum(hn · projh) + sum(cn · projc)
    case.{c}.out, .hn, .cn; case.{c}.grad.{parameter}, case.{c}.grad.x, case.{c}.grad.hx, case.{c}.grad.cx
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
from speechbrain.nnet.RNN import LSTM  # noqa: E402
from speechbrain.nnet.embedding import Embedding  # noqa: E402

INITS = {}
for _re in (True, False):
    for _l in (1, 2):
        for _bi in (False, True):
            INITS[f"re{int(_re)}_l{_l}_bi{int(_bi)}"] = dict(hidden_size=5, input_size=20, num_layers=_l, re_init=_re,
                                                            bidirectional=_bi)
INITS["nobias"] = dict(hidden_size=5, input_size=20, bias=False)

SHAPE = (4, 10, 20)
# name: (LSTM kwargs, input shape, hx?, lengths)
CASES = {
    "doctest": (dict(hidden_size=5, input_shape=SHAPE), SHAPE, False, None),
    "hx": (dict(hidden_size=5, input_shape=SHAPE), SHAPE, True, None),
    "4d": (dict(hidden_size=5, input_shape=(4, 10, 5, 4)), (4, 10, 5, 4), False, None),
    "layers2": (dict(hidden_size=5, input_shape=SHAPE, num_layers=2), SHAPE, True, None),
    "bidir": (dict(hidden_size=5, input_shape=SHAPE, bidirectional=True), SHAPE, True, None),
    "bidir_layers2": (dict(hidden_size=5, input_shape=SHAPE, num_layers=2, bidirectional=True), SHAPE, False, None),
    "len_full": (dict(hidden_size=5, input_shape=SHAPE), SHAPE, True, [1.0, 0.55, 0.1, 0.8]),
    "len_short": (dict(hidden_size=5, input_shape=SHAPE), SHAPE, False, [0.7, 0.55, 0.1, 0.3]),
    "len_bidir_layers2": (dict(hidden_size=5, input_shape=SHAPE, num_layers=2, bidirectional=True), SHAPE, True,
                          [0.7, 0.55, 0.1, 0.3]),
}
ONEHOT = dict(emb_kw=dict(num_embeddings=7, consider_as_one_hot=True, blank_id=3),
              lstm_kw=dict(hidden_size=5, input_size=6, bidirectional=True),
              tokens=[[3, 0, 6, 6, 2, 3, 1, 1, 5, 3], [3] * 10, [3, 5, 5, 1, 4, 0, 0, 2, 6, 4],
                      [3, 6, 2, 2, 2, 6, 3, 3, 0, 1]])


def signature(cls):
    return np.array(json.dumps(
        [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
         for p in inspect.signature(cls.__init__).parameters.values()]))


def kw_json(kw):
    return np.array(json.dumps({k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}))


def run_case(out, name, lstm, x, hx, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    pre = f"case.{name}."
    for k, v in lstm.state_dict().items():
        out[pre + "sd." + k] = v.numpy().copy()
    if hx is not None:
        hx = tuple(h.clone().requires_grad_(True) for h in hx)
        out[pre + "hx"] = hx[0].detach().numpy().copy()
        out[pre + "cx"] = hx[1].detach().numpy().copy()
    lens = None
    if lengths is not None:
        lens = torch.tensor(lengths)
        out[pre + "lengths"] = lens.numpy().copy()
        out[pre + "steps"] = torch.as_tensor((lens * x.size(1)).cpu(), dtype=torch.int64).numpy()
    y, (hn, cn) = lstm(x, hx=hx, lengths=lens)
    proj = torch.randn(y.shape, generator=g)
    projh = torch.randn(hn.shape, generator=g)
    projc = torch.randn(cn.shape, generator=g)
    ((y * proj).sum() + (hn * projh).sum() + (cn * projc).sum()).backward()
    out[pre + "proj"], out[pre + "projh"], out[pre + "projc"] = proj.numpy(), projh.numpy(), projc.numpy()
    out[pre + "out"] = y.detach().numpy()
    out[pre + "hn"] = hn.detach().numpy()
    out[pre + "cn"] = cn.detach().numpy()
    for k, p in lstm.named_parameters():
        out[pre + "grad." + k] = p.grad.numpy().copy()
    if x.requires_grad:
        out[pre + "grad.x"] = x.grad.numpy().copy()
    if hx is not None:
        out[pre + "grad.hx"] = hx[0].grad.numpy().copy()
        out[pre + "grad.cx"] = hx[1].grad.numpy().copy()
    print(f"{name}: out {tuple(y.shape)}, hn {tuple(hn.shape)}")


def main():
    out = {"signature.LSTM": signature(LSTM)}
    out["init.names"] = np.array(list(INITS), dtype="U16")
    for name, kw in INITS.items():
        torch.manual_seed(0)
        m = LSTM(**kw)
        out[f"init.{name}.kw"] = kw_json(kw)
        for k, v in m.state_dict().items():
            out[f"init.{name}.sd.{k}"] = v.numpy().copy()
        out[f"init.{name}.next"] = torch.rand(4).numpy()
    out["case.names"] = np.array(list(CASES) + ["onehot"], dtype="U24")
    for i, (name, (kw, shape, with_hx, lengths)) in enumerate(CASES.items()):
        torch.manual_seed(120 + i)
        lstm = LSTM(**kw)
        g = torch.Generator().manual_seed(140 + i)
        x = torch.rand(shape, generator=g).requires_grad_(True)
        LD = kw.get("num_layers", 1) * (2 if kw.get("bidirectional") else 1)
        hx = None
        if with_hx:
            hx = (torch.randn(LD, shape[0], kw["hidden_size"], generator=g),
                  torch.randn(LD, shape[0], kw["hidden_size"], generator=g))
        out[f"case.{name}.kw"] = kw_json(kw)
        out[f"case.{name}.x"] = x.detach().numpy().copy()
        run_case(out, name, lstm, x, hx, lengths, 160 + i)
    torch.manual_seed(130)
    emb = Embedding(**ONEHOT["emb_kw"])
    lstm = LSTM(**ONEHOT["lstm_kw"])
    tokens = torch.tensor(ONEHOT["tokens"])
    out["case.onehot.kw"] = kw_json(ONEHOT["lstm_kw"])
    out["case.onehot.emb_kw"] = kw_json(ONEHOT["emb_kw"])
    out["case.onehot.tokens"] = tokens.numpy()
    run_case(out, "onehot", lstm, emb(tokens), None, None, 170)
    path = os.path.join(OUT, "lstm.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
