"""Generate tests/golden/attdec.npz from the REAL reference's
AttentionalRNNDecoder (speechbrain/nnet/RNN.py) and its attention modules
(speechbrain/nnet/attention.py) on the CPU.

    python tests/golden/gen_attdec_golden.py

Runs only where the reference checkout is present (as gen_lstm_golden.py, whose
pattern this follows); the committed attdec.npz is what the tests read.  The
file holds data only.

Keys
  attn.names; per standalone attention case a (the reference's doctest sizes, L 10):
    attn.{a}.kw (JSON), attn.{a}.sd.*, attn.{a}.enc (B, L, E), attn.{a}.enc_len (B),
    attn.{a}.dec (3, B, dec_dim): three calls in sequence; attn.{a}.context (3, B, out), attn.{a}.attn (3, B, L)
  dec.names; per decoder case d:
    dec.{d}.kw (JSON), dec.{d}.sd.*, dec.{d}.inp (B, T, I), dec.{d}.enc (B, L, E), dec.{d}.wav_len (B)
    dec.{d}.r1, .r2   the fixed randn of the loss sum(outputs r1) + sum(attn r2)
    dec.{d}.outputs, .attn; dec.{d}.grad.{parameter}, dec.{d}.grad.inp, dec.{d}.grad.enc
    dec.{d}.step.out / .hs / .c / .w   three forward_step calls in sequence on inp[:, 0..2]
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import gen_s2s_golden as S  # noqa: E402,F401  (installs the stubs, puts the reference on sys.path)

import torch  # noqa: E402
from speechbrain.nnet.RNN import AttentionalRNNDecoder  # noqa: E402
from speechbrain.nnet.attention import ContentBasedAttention, LocationAwareAttention  # noqa: E402

ATTN = {
    "location": (LocationAwareAttention, dict(enc_dim=20, dec_dim=25, attn_dim=30, output_dim=5, conv_channels=10,
                                              kernel_size=100)),
    "content": (ContentBasedAttention, dict(enc_dim=20, dec_dim=25, attn_dim=30, output_dim=5)),
}
_DOC = dict(rnn_type="gru", hidden_size=7, attn_dim=5, num_layers=1, enc_dim=20, input_size=6)
# name: (kwargs, B, T, L, wav_len)
DEC = {
    "doctest_content": (dict(_DOC, attn_type="content"), 4, 5, 10, [1.0, 0.72, 0.33, 0.9]),
    "doctest_location": (dict(_DOC, attn_type="location", channels=10, kernel_size=100), 4, 5, 10,
                         [1.0, 0.72, 0.33, 0.9]),
    "ragged": (dict(rnn_type="gru", attn_type="location", hidden_size=16, attn_dim=12, num_layers=1, enc_dim=24,
                    input_size=8, channels=10, kernel_size=15, scaling=2.0), 3, 4, 40, [1.0, 0.6, 0.03]),
}


def kw_json(kw):
    return np.array(json.dumps(kw))


def main():
    out = {"attn.names": np.array(list(ATTN), dtype="U16"), "dec.names": np.array(list(DEC), dtype="U24")}
    for i, (name, (cls, kw)) in enumerate(ATTN.items()):
        torch.manual_seed(300 + i)
        net = cls(**kw)
        g = torch.Generator().manual_seed(310 + i)
        enc = torch.rand(4, 10, 20, generator=g)
        enc_len = torch.tensor([10, 7, 1, 4])
        dec = torch.randn(3, 4, 25, generator=g)
        pre = f"attn.{name}."
        out[pre + "kw"] = kw_json(kw)
        for k, v in net.state_dict().items():
            out[pre + "sd." + k] = v.numpy().copy()
        with torch.no_grad():
            res = [net(enc, enc_len, dec[s]) for s in range(3)]
        out[pre + "enc"], out[pre + "enc_len"], out[pre + "dec"] = enc.numpy(), enc_len.numpy(), dec.numpy()
        out[pre + "context"] = torch.stack([r[0] for r in res]).numpy()
        out[pre + "attn"] = torch.stack([r[1] for r in res]).numpy()
        print(name, out[pre + "context"].shape, out[pre + "attn"].shape)
    for i, (name, (kw, B, T, L, wav_len)) in enumerate(DEC.items()):
        torch.manual_seed(320 + i)
        net = AttentionalRNNDecoder(**kw)
        g = torch.Generator().manual_seed(330 + i)
        inp = torch.randn(B, T, kw["input_size"], generator=g).requires_grad_(True)
        enc = torch.randn(B, L, kw["enc_dim"], generator=g).requires_grad_(True)
        wl = torch.tensor(wav_len)
        pre = f"dec.{name}."
        out[pre + "kw"] = kw_json(kw)
        for k, v in net.state_dict().items():
            out[pre + "sd." + k] = v.numpy().copy()
        outputs, attn = net(inp, enc, wl)
        r1 = torch.randn(outputs.shape, generator=g)
        r2 = torch.randn(attn.shape, generator=g)
        ((outputs * r1).sum() + (attn * r2).sum()).backward()
        out[pre + "inp"], out[pre + "enc"], out[pre + "wav_len"] = inp.detach().numpy(), enc.detach().numpy(), wl.numpy()
        out[pre + "r1"], out[pre + "r2"] = r1.numpy(), r2.numpy()
        out[pre + "outputs"], out[pre + "attn"] = outputs.detach().numpy(), attn.detach().numpy()
        for k, p in net.named_parameters():
            out[pre + "grad." + k] = p.grad.numpy().copy()
        out[pre + "grad.inp"], out[pre + "grad.enc"] = inp.grad.numpy().copy(), enc.grad.numpy().copy()
        with torch.no_grad():
            net.attn.reset()
            enc_len = torch.round(L * wl).long()
            hs, c = None, torch.zeros(B, kw["attn_dim"])
            steps = []
            for t in range(3):
                o, hs, c, w = net.forward_step(inp[:, t], hs, c, enc, enc_len)
                steps.append((o, hs, c, w))
        for j, key in enumerate(("out", "hs", "c", "w")):
            out[pre + "step." + key] = torch.stack([s[j] for s in steps]).numpy()
        print(name, tuple(outputs.shape), tuple(attn.shape))
    path = os.path.join(OUT, "attdec.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
