"""Generate tests/golden/crdnn.npz from the REAL reference's CRDNN and
CNN_Block (speechbrain/lobes/models/CRDNN.py:14-276) on the CPU.

    python tests/golden/gen_crdnn_golden.py

Runs only where the reference checkout is present (as gen_ligru_golden.py,
whose pattern this follows); the committed crdnn.npz is what the tests read.
The file holds data only.

Keys
  case.names; per case c:
    case.{c}.cls     "CRDNN" or "CNN_Block"
    case.{c}.kw      JSON of the constructor's keyword arguments (rnn_class by name)
    case.{c}.train   1: training mode, 0: eval
    case.{c}.sd.*    the state_dict (norm affines and BatchNorm running statistics set to drawn values,
                     the DNN / projection Linear weights scaled by 8)
    case.{c}.x       the input (B, T, F)
    case.{c}.proj    the fixed randn of the scalar sum(output * proj)
    case.{c}.out; case.{c}.grad.{parameter}, case.{c}.grad.x
Cases: the two doctest calls, CRDNN(input_shape=(10, 15, 60)) and
CNN_Block(channels=32) on (10, 15, 60), at batch 2 and, for the lobe, with
the channel / neuron widths cut down (LiGRU, two layers), so that the file
stays a few hundred KB (dropout 0 keeps the LiGRU's drop_masks buffers constant) — both in eval mode,
where their dropouts are off; and a small recipe-like lobe (LSTM, one layer,
dropout 0) in eval and in training mode.  Every array is fp32.
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
import speechbrain as sb  # noqa: E402
from speechbrain.lobes.models.CRDNN import CRDNN, CNN_Block  # noqa: E402

SMALL = dict(input_shape=(3, 9, 12), dropout=0.0, cnn_blocks=2, cnn_channels=[16, 16], rnn_class="LSTM",
             rnn_layers=1, rnn_neurons=12, rnn_bidirectional=True, dnn_blocks=2, dnn_neurons=20)
# name: (class, kwargs, input shape, training?)
CASES = {
    "doctest_crdnn": ("CRDNN", dict(input_shape=(2, 15, 60), dropout=0.0, cnn_channels=[16, 16], rnn_neurons=16,
                                    rnn_layers=2,
                                    dnn_neurons=32), (2, 15, 60), False),
    "doctest_block": ("CNN_Block", dict(input_shape=(2, 15, 60), channels=32), (2, 15, 60), False),
    "small_eval": ("CRDNN", SMALL, (3, 9, 12), False),
    "small_train": ("CRDNN", SMALL, (3, 9, 12), True),
}


def main():
    out = {"case.names": np.array(list(CASES), dtype="U24")}
    for i, (name, (cls, kw, shape, train)) in enumerate(CASES.items()):
        torch.manual_seed(300 + i)
        args = dict(kw)
        if "rnn_class" in args:
            args["rnn_class"] = getattr(sb.nnet.RNN, args["rnn_class"])
        net = (CRDNN if cls == "CRDNN" else CNN_Block)(**args)
        g = torch.Generator().manual_seed(340 + i)
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
                elif k.endswith("linear.w.weight"):
                    # a training-mode BatchNorm cancels the bias in front of it: that bias' gradient is
                    # identically zero and what is recorded is rounding noise proportional to 1 / std of
                    # the Linear's output; the larger weights keep that std, and so the noise, in range
                    v.mul_(8.0)
        net.train(train)
        pre = f"case.{name}."
        out[pre + "cls"] = np.array(cls)
        out[pre + "kw"] = np.array(json.dumps({k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}))
        out[pre + "train"] = np.array(int(train))
        for k, v in net.state_dict().items():
            out[pre + "sd." + k] = v.numpy().copy()
        x = torch.rand(shape, generator=g).requires_grad_(True)
        y = net(x)
        proj = torch.randn(y.shape, generator=g)
        (y * proj).sum().backward()
        out[pre + "x"] = x.detach().numpy().copy()
        out[pre + "proj"] = proj.numpy()
        out[pre + "out"] = y.detach().numpy().copy()
        out[pre + "grad.x"] = x.grad.numpy().copy()
        for k, p in net.named_parameters():
            out[pre + "grad." + k] = p.grad.numpy().copy()
        print(f"{pre} out {tuple(y.shape)}")
    path = os.path.join(OUT, "crdnn.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
