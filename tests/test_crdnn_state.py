"""CPU check of the CRDNN drop-in's boundary: the lobe and its CNN_Block
construct without a GPU and carry exactly the reference's state_dict keys and
shapes (tests/golden/crdnn.npz, recorded from the reference)."""
import json

import pytest


@pytest.mark.parametrize("name", ["doctest_crdnn", "doctest_block", "small_train"])
def test_state_dict_keys_and_shapes_match_the_reference(golden, name):
    from speechbrain_amd.lobes.models import CRDNN as M
    from speechbrain_amd.nnet import RNN
    g, pre = golden("crdnn"), f"case.{name}."
    kw = json.loads(str(g[pre + "kw"]))
    kw["input_shape"] = tuple(kw["input_shape"])
    if "rnn_class" in kw:
        kw["rnn_class"] = getattr(RNN, kw["rnn_class"])
    net = getattr(M, str(g[pre + "cls"]))(**kw)
    want = {k[len(pre) + 3:]: g[k].shape for k in g.files if k.startswith(pre + "sd.")}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want
