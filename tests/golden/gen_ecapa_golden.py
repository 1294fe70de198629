"""Generate tests/golden/ecapa.npz from the REAL reference's ECAPA_TDNN lobe
(speechbrain/lobes/models/ECAPA_TDNN.py) on the CPU.

    python tests/golden/gen_ecapa_golden.py

Runs only where the reference checkout is present (as gen_crdnn_golden.py,
whose pattern this follows); the committed ecapa.npz is what the tests read.
The file holds data only.

Keys: case.names; per case c: case.{c}.cls, .kw (JSON), .train, .sd.* (the
state_dict of the forward, BatchNorm statistics and affines drawn), .x,
.lengths (absent: None), .out; model_relu also .init.* (after the seeded
construction); model_leaky / model_train .shares = "model_relu" (same seeds:
its init.* and sd.*); the training case .proj and .grad.*.  The training case
uses lengths (1.0, 0.75, 0.5): at 0.2 one channel of the 7-frame utterance
pools to a variance at the 1e-12 clamp, where the root's gradient jumps; every
pooled variance of that case is asserted >= 1e-2, as the pooling tests keep
it.  Sub-blocks: the doctest calls at batch 2, 40 frames.  Every array is fp32."""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import gen_s2s_golden as S  # noqa: E402,F401  (installs the stubs, puts the reference on sys.path)

import torch  # noqa: E402
from speechbrain.lobes.models import ECAPA_TDNN as E  # noqa: E402

SMALL = dict(input_size=24, lin_neurons=16, channels=[32, 32, 32, 32, 96], attention_channels=16, se_channels=16,
             res2net_scale=4)
LENS = [1.0, 0.5, 0.2]
# name: (class, kwargs, input shape, lengths, training?)
CASES = {
    "model_relu": ("ECAPA_TDNN", SMALL, (3, 37, 24), LENS, False),
    "model_leaky": ("ECAPA_TDNN", dict(SMALL, activation="LeakyReLU"), (3, 37, 24), None, False),
    "model_train": ("ECAPA_TDNN", SMALL, (3, 37, 24), [1.0, 0.75, 0.5], True),
    "tdnn": ("TDNNBlock", dict(in_channels=64, out_channels=64, kernel_size=3, dilation=1), (2, 64, 40), None, False),
    "res2net": ("Res2NetBlock", dict(in_channels=64, out_channels=64, scale=4, dilation=3), (2, 64, 40), None, False),
    "se": ("SEBlock", dict(in_channels=64, se_channels=16, out_channels=64), (2, 64, 40), [1.0, 0.6], False),
    "asp": ("AttentiveStatisticsPooling", dict(channels=64), (2, 64, 40), [1.0, 0.6], False),
    "seres2net": ("SERes2NetBlock", dict(in_channels=64, out_channels=64, res2net_scale=4), (2, 64, 40), None, False),
}


def main():
    out = {"case.names": np.array(list(CASES), dtype="U24")}
    for i, (name, (cls, kw, shape, lens, train)) in enumerate(CASES.items()):
        model = cls == "ECAPA_TDNN"
        i = 0 if model else i  # the three model cases share seeds: one construction, one drawn state, one input
        torch.manual_seed(400 + i)
        args = dict(kw)
        if "activation" in args:
            args["activation"] = getattr(torch.nn, args["activation"])
        net = getattr(E, cls)(**args)
        pre = f"case.{name}."
        if name == "model_relu":
            for k, v in net.state_dict().items():
                out[pre + "init." + k] = v.numpy().copy()
        g = torch.Generator().manual_seed(440 + i)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                if k.endswith("running_mean"):
                    v.copy_(0.3 * torch.randn(v.shape, generator=g))
                elif k.endswith("running_var"):
                    v.copy_(0.5 + torch.rand(v.shape, generator=g))
                elif k.endswith("norm.weight"):
                    v.copy_(1.0 + 0.2 * torch.randn(v.shape, generator=g))
                elif k.endswith("norm.bias"):
                    v.copy_(0.2 * torch.randn(v.shape, generator=g))
        net.train(train)
        out[pre + "cls"] = np.array(cls)
        out[pre + "kw"] = np.array(json.dumps(kw))
        out[pre + "train"] = np.array(int(train))
        if model and name != "model_relu":
            out[pre + "shares"] = np.array("model_relu")  # its init.* and sd.* are this case's too
        else:
            for k, v in net.state_dict().items():  # before the forward: a training-mode call updates the statistics
                out[pre + "sd." + k] = v.numpy().copy()
        x = torch.randn(shape, generator=g).requires_grad_(train)
        call = {}
        if lens is not None:
            call["lengths"] = torch.tensor(lens)
            out[pre + "lengths"] = np.array(lens, dtype=np.float32)
        pooled = []
        if train:
            net.asp.register_forward_hook(lambda m, i, o: pooled.append(o.detach()))
        y = net(x, **call)
        if train:
            assert float(pooled[0][:, pooled[0].shape[1] // 2:].min()) ** 2 >= 1e-2, "a pooled variance below 1e-2"
        out[pre + "x"] = x.detach().numpy().copy()
        if train:
            proj = torch.randn(y.shape, generator=g)
            (y * proj).sum().backward()
            out[pre + "proj"] = proj.numpy()
            out[pre + "grad.x"] = x.grad.numpy().copy()
            for k, p in net.named_parameters():
                out[pre + "grad." + k] = p.grad.numpy().copy()
        out[pre + "out"] = y.detach().numpy().copy()
        print(f"{pre} out {tuple(y.shape)}")
    path = os.path.join(OUT, "ecapa.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
