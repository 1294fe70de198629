"""The ECAPA-TDNN drop-in's boundary on the CPU: the reference's state_dict
(tests/golden/ecapa.npz) loads with strict=True, a seeded construction gives
the reference's parameters bit for bit, and the arguments the reference
refuses are refused."""
import json

import numpy as np
import pytest
import torch


def build(g, name):
    from speechbrain_amd.lobes.models import ECAPA_TDNN as E
    kw = json.loads(str(g[f"case.{name}.kw"]))
    if "activation" in kw:
        kw["activation"] = getattr(torch.nn, kw["activation"])
    return getattr(E, str(g[f"case.{name}.cls"]))(**kw)


def state(g, name, part="sd"):
    key = f"case.{name}.shares"
    pre = f"case.{str(g[key]) if key in g.files else name}.{part}."
    return {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def test_strict_load(golden):
    g = golden("ecapa")
    for name in g["case.names"]:
        build(g, str(name)).load_state_dict(state(g, str(name)), strict=True)


def test_seeded_init(golden):
    g = golden("ecapa")
    torch.manual_seed(400)
    sd = build(g, "model_relu").state_dict()
    ref = state(g, "model_relu", "init")
    assert list(sd) == list(ref)
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), ref[k].numpy()), k


def test_refused_arguments():
    from speechbrain_amd._lib import SbkError
    from speechbrain_amd.lobes.models.ECAPA_TDNN import ECAPA_TDNN, Res2NetBlock
    from speechbrain_amd.nnet.CNN import Conv1d
    with pytest.raises(ValueError):
        Conv1d(out_channels=8, kernel_size=4, input_shape=(2, 10, 4))   # even kernel with "same"
    with pytest.raises(ValueError):
        Conv1d(out_channels=8, kernel_size=3)                           # neither input_shape nor in_channels
    with pytest.raises(AssertionError):
        Res2NetBlock(60, 64, scale=8)
    with pytest.raises(AssertionError):
        ECAPA_TDNN(24, channels=[32, 32], kernel_sizes=[5, 3, 1])
    net = ECAPA_TDNN(24, lin_neurons=16, channels=[32, 32, 96], kernel_sizes=[5, 3, 1], dilations=[1, 2, 1],
                     attention_channels=16, se_channels=16, res2net_scale=4).eval()
    with pytest.raises(SbkError):
        net(torch.randn(2, 20, 24))                                     # CPU tensors: no fallback
