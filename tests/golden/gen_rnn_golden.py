"""Generate tests/golden/rnn.npz from the REAL reference's GRU
(speechbrain/nnet/RNN.py) and Embedding (speechbrain/nnet/embedding.py) on the
CPU.

    python tests/golden/gen_rnn_golden.py

Runs only where the reference checkout is present (as gen_s2s_golden.py, whose
inert stubs for torchaudio, hyperpyyaml and ruamel it uses); the committed
rnn.npz is what the tests read.  The file holds data only.

Keys
  signature.GRU / signature.Embedding   JSON [[parameter, kind, repr(default) | "<empty>"], ...] of __init__
  init.names; init.{n}.kw (JSON of the constructor's keyword arguments);
  init.{n}.sd.*   the state_dict right after torch.manual_seed(0) and construction
                  (re_init true / false, num_layers 1 / 2, bias false)
  init.{n}.next   torch.rand(4) drawn right after that construction: the position the
                  global generator was left at (the orthogonal weight_hh of rnn_init come
                  out of a LAPACK QR, whose last bits differ between builds; the draws do not)
  onehot.{blank}  the frozen table of Embedding(7, consider_as_one_hot=True, blank_id=blank), blank 0, 3, 6
  case.names; per case c:
    case.{c}.kw       JSON of GRU's keyword arguments
    case.{c}.sd.*     the GRU's state_dict (construction under the case's own seed)
    case.{c}.x        the input ((B, T, I), 4-D for "4d"; "onehot": case.{c}.tokens (B, U) int64, case.{c}.emb_kw)
    case.{c}.hx (L, B, H), case.{c}.lengths (B) where the case has them
    case.{c}.steps    the integer lengths torch's packing used (cases with lengths)
    case.{c}.proj     the fixed randn of the scalar sum(output · proj)
    case.{c}.out, case.{c}.hn; case.{c}.grad.{parameter}, case.{c}.grad.x, case.{c}.grad.hx
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
from speechbrain.nnet.RNN import GRU  # noqa: E402
from speechbrain.nnet.embedding import Embedding  # noqa: E402

INITS = {
    "re1_l1": dict(hidden_size=5, input_size=20),
    "re0_l1": dict(hidden_size=5, input_size=20, re_init=False),
    "re1_l2": dict(hidden_size=5, input_size=20, num_layers=2),
    "re0_l2": dict(hidden_size=5, input_size=20, num_layers=2, re_init=False),
    "nobias": dict(hidden_size=5, input_size=20, bias=False),
}

# name: (GRU kwargs, input shape, hx?, lengths)
CASES = {
    "doctest": (dict(hidden_size=5, input_shape=(4, 10, 20)), (4, 10, 20), False, None),
    "hx": (dict(hidden_size=5, input_shape=(4, 10, 20)), (4, 10, 20), True, None),
    "4d": (dict(hidden_size=5, input_shape=(4, 10, 5, 4)), (4, 10, 5, 4), False, None),
    "layers2": (dict(hidden_size=5, input_shape=(4, 10, 20), num_layers=2), (4, 10, 20), True, None),
    "len_full": (dict(hidden_size=5, input_shape=(4, 10, 20)), (4, 10, 20), True, [1.0, 0.55, 0.1, 0.8]),
    "len_short": (dict(hidden_size=5, input_shape=(4, 10, 20)), (4, 10, 20), False, [0.7, 0.55, 0.1, 0.3]),
    "len_layers2": (dict(hidden_size=5, input_shape=(4, 10, 20), num_layers=2), (4, 10, 20), True,
                    [0.7, 0.55, 0.1, 0.3]),
}
ONEHOT = dict(emb_kw=dict(num_embeddings=7, consider_as_one_hot=True, blank_id=3),
              gru_kw=dict(hidden_size=5, input_size=6),
              tokens=[[3, 0, 6, 6, 2, 3], [3, 3, 3, 3, 3, 3], [3, 5, 5, 1, 4, 0], [3, 6, 2, 2, 2, 6]])


def signature(cls):
    return np.array(json.dumps(
        [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
         for p in inspect.signature(cls.__init__).parameters.values()]))


def kw_json(kw):
    return np.array(json.dumps({k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}))


def run_case(out, name, gru, x, hx, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    pre = f"case.{name}."
    for k, v in gru.state_dict().items():
        out[pre + "sd." + k] = v.numpy().copy()
    if hx is not None:
        hx = hx.clone().requires_grad_(True)
        out[pre + "hx"] = hx.detach().numpy().copy()
    lens = None
    if lengths is not None:
        lens = torch.tensor(lengths)
        out[pre + "lengths"] = lens.numpy().copy()
        out[pre + "steps"] = torch.as_tensor((lens * x.size(1)).cpu(), dtype=torch.int64).numpy()
    y, hn = gru(x, hx=hx, lengths=lens)
    proj = torch.randn(y.shape, generator=g)
    (y * proj).sum().backward()
    out[pre + "proj"] = proj.numpy()
    out[pre + "out"] = y.detach().numpy()
    out[pre + "hn"] = hn.detach().numpy()
    for k, p in gru.named_parameters():
        out[pre + "grad." + k] = p.grad.numpy().copy()
    if x.requires_grad:
        out[pre + "grad.x"] = x.grad.numpy().copy()
    if hx is not None:
        out[pre + "grad.hx"] = hx.grad.numpy().copy()
    print(f"{name}: out {tuple(y.shape)}, hn {tuple(hn.shape)}")


def main():
    out = {"signature.GRU": signature(GRU), "signature.Embedding": signature(Embedding)}
    out["init.names"] = np.array(list(INITS), dtype="U16")
    for name, kw in INITS.items():
        torch.manual_seed(0)
        m = GRU(**kw)
        out[f"init.{name}.kw"] = kw_json(kw)
        for k, v in m.state_dict().items():
            out[f"init.{name}.sd.{k}"] = v.numpy().copy()
        out[f"init.{name}.next"] = torch.rand(4).numpy()
    for blank in (0, 3, 6):
        emb = Embedding(7, consider_as_one_hot=True, blank_id=blank)
        assert not emb.Embedding.weight.requires_grad
        out[f"onehot.{blank}"] = emb.state_dict()["Embedding.weight"].numpy().copy()
    out["case.names"] = np.array(list(CASES) + ["onehot"], dtype="U16")
    for i, (name, (kw, shape, with_hx, lengths)) in enumerate(CASES.items()):
        torch.manual_seed(20 + i)
        gru = GRU(**kw)
        g = torch.Generator().manual_seed(40 + i)
        x = torch.rand(shape, generator=g).requires_grad_(True)
        hx = torch.randn(kw.get("num_layers", 1), shape[0], kw["hidden_size"], generator=g) if with_hx else None
        out[f"case.{name}.kw"] = kw_json(kw)
        out[f"case.{name}.x"] = x.detach().numpy().copy()
        run_case(out, name, gru, x, hx, lengths, 60 + i)
    torch.manual_seed(30)
    emb = Embedding(**ONEHOT["emb_kw"])
    gru = GRU(**ONEHOT["gru_kw"])
    tokens = torch.tensor(ONEHOT["tokens"])
    out["case.onehot.kw"] = kw_json(ONEHOT["gru_kw"])
    out["case.onehot.emb_kw"] = kw_json(ONEHOT["emb_kw"])
    out["case.onehot.tokens"] = tokens.numpy()
    run_case(out, "onehot", gru, emb(tokens), None, None, 70)
    path = os.path.join(OUT, "rnn.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
