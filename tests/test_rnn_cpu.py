"""CPU checks of the prediction-network drop-ins (speechbrain_amd.nnet.RNN.GRU,
speechbrain_amd.nnet.embedding.Embedding) against tests/golden/rnn.npz, written
by the reference on the CPU (gen_rnn_golden.py): constructor signatures,
state-dict keys and shapes, seeded init, the frozen one-hot tables; the float64
restatement the GPU tests use as their oracle (tests/rnn_ref.py) reproduces
every fixture output and gradient to 1e-6; CPU tensors and bidirectional are
refused; the sbk_gru_* / sbk_embed_* / sbk_segsum_rows entry points are
declared, bound, exported and return 1001 before any launch for null pointers
and non-positive sizes."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import rnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbk_gru_fwd", "sbk_gru_bwd", "sbk_embed_onehot", "sbk_embed_gather", "sbk_segsum_rows"]


def _signature(cls):
    return [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(cls.__init__).parameters.values()]


def _kw(g, key):
    kw = json.loads(str(g[key]))
    if "input_shape" in kw:
        kw["input_shape"] = tuple(kw["input_shape"])
    return kw


def _sub(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


def test_signatures(golden):
    from speechbrain_amd.nnet.RNN import GRU
    from speechbrain_amd.nnet.embedding import Embedding
    g = golden("rnn")
    assert _signature(GRU) == json.loads(str(g["signature.GRU"]))
    assert _signature(Embedding) == json.loads(str(g["signature.Embedding"]))


def test_seeded_init_and_state_dict(golden):
    """Same seed, the reference's tensors.  torch's uniform init is bit-exact
    on every machine.  The weight_hh that rnn_init re-draws are the Q of a
    LAPACK QR of exactly reproducible normal draws (torch.nn.init.orthogonal_,
    signs fixed by diag(R)): its last bits depend on the LAPACK build, so those
    tensors are held to 64 fp32 epsilons (7.6e-6) of the fixture — a Householder
    QR of a 15 x 5 matrix with entries below 1 is backward stable to a small
    multiple of m * eps (an fp32 QR of such draws lies within 2.7e-7 of the
    float64 one over 200 seeds), while a different draw is off by O(1) — and
    must be orthonormal.  That the constructor consumed exactly the reference's draws
    is checked bit for bit on the next torch.rand after construction."""
    from speechbrain_amd.nnet.RNN import GRU
    g = golden("rnn")
    for name in g["init.names"]:
        kw = _kw(g, f"init.{name}.kw")
        torch.manual_seed(0)
        m = GRU(**kw)
        after = torch.rand(4)
        want = _sub(g, f"init.{name}.sd.")
        sd = m.state_dict()
        assert list(sd) == list(want), name
        for k, v in sd.items():
            assert v.shape == want[k].shape, (name, k)
            if "weight_hh" in k and kw.get("re_init", True):
                assert float((v - want[k]).abs().max()) <= 64 * 2.0 ** -23, (name, k)
                H = v.shape[1]
                assert float((v.double().t() @ v.double() - torch.eye(H, dtype=torch.float64)).abs().max()) <= 1e-5
            else:
                assert np.array_equal(v.numpy(), want[k].numpy()), (name, k)
        assert np.array_equal(after.numpy(), g[f"init.{name}.next"]), name
        m.load_state_dict(want, strict=True)


@pytest.mark.parametrize("blank", [0, 3, 6])
def test_onehot_table(golden, blank):
    from speechbrain_amd.nnet.embedding import Embedding
    emb = Embedding(7, consider_as_one_hot=True, blank_id=blank)
    assert list(emb.state_dict()) == ["Embedding.weight"]
    w = emb.Embedding.weight
    assert not w.requires_grad
    assert (emb.num_embeddings, emb.embedding_dim, emb.blank_id, emb.consider_as_one_hot) == (7, 6, blank, True)
    assert np.array_equal(w.numpy(), golden("rnn")[f"onehot.{blank}"])
    assert np.array_equal(R.onehot_table(7, blank).numpy(), golden("rnn")[f"onehot.{blank}"])
    tr = Embedding(5, embedding_dim=3)
    assert tr.Embedding.weight.requires_grad and tr.embedding_dim == 3 and tuple(tr.Embedding.weight.shape) == (5, 3)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert err <= 1e-6, (what, err)


def fixture_case(g, name, dtype=torch.float64):
    """(x leaf or None, params, hx leaf or None, steps or None, proj, tokens or None) of a fixture case."""
    kw = _kw(g, f"case.{name}.kw")
    sd = _sub(g, f"case.{name}.sd.")
    params = [R.layer_params(sd, l, dtype) for l in range(kw.get("num_layers", 1))]
    key = f"case.{name}."
    hx = torch.from_numpy(g[key + "hx"]).to(dtype).requires_grad_(True) if key + "hx" in g.files else None
    steps = None
    if key + "lengths" in g.files:
        T = g[key + "x"].shape[1]
        steps = R.steps_of(g[key + "lengths"], T)
        assert steps.tolist() == g[key + "steps"].tolist(), name   # the integer lengths torch's packing used
    proj = torch.from_numpy(g[key + "proj"]).to(dtype)
    if key + "tokens" in g.files:
        return None, params, hx, steps, proj, torch.from_numpy(g[key + "tokens"])
    x = torch.from_numpy(g[key + "x"]).to(dtype).requires_grad_(True)
    return x, params, hx, steps, proj, None


def test_float64_restatement_reproduces_fixture(golden):
    g = golden("rnn")
    for name in g["case.names"]:
        x, params, hx, steps, proj, tokens = fixture_case(g, name)
        if tokens is not None:
            ekw = json.loads(str(g[f"case.{name}.emb_kw"]))
            xin = R.onehot_table(ekw["num_embeddings"], ekw["blank_id"])[tokens]
        else:
            xin = x.reshape(x.shape[0], x.shape[1], -1)
        out, hn = R.gru_ref(xin, params, hx, steps)
        (out * proj).sum().backward()
        key = f"case.{name}."
        _close(out.detach(), g[key + "out"], name + " out")
        _close(hn.detach(), g[key + "hn"], name + " hn")
        for l, ps in enumerate(params):
            for n, p in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), ps):
                if p is not None:
                    _close(p.grad, g[f"{key}grad.rnn.{n}_l{l}"], f"{name} {n}_l{l}")
        if x is not None:
            _close(x.grad, g[key + "grad.x"], name + " dx")
        if hx is not None:
            _close(hx.grad, g[key + "grad.hx"], name + " dhx")
    # a length case really is ragged and short: one-frame row, output cut to the longest row
    assert g["case.len_full.steps"].tolist() == [10, 5, 1, 8]
    assert g["case.len_short.steps"].tolist() == [7, 5, 1, 3] and g["case.len_short.out"].shape[1] == 7


def test_cpu_tensors_are_refused():
    from speechbrain_amd._lib import SbkError
    from speechbrain_amd.nnet.RNN import GRU
    from speechbrain_amd.nnet.embedding import Embedding
    with pytest.raises(SbkError):
        GRU(5, input_shape=(4, 10, 20))(torch.rand(4, 10, 20))
    with pytest.raises(SbkError):
        Embedding(7, consider_as_one_hot=True, blank_id=0)(torch.tensor([[1, 2]]))
    with pytest.raises(SbkError):
        Embedding(7, embedding_dim=4)(torch.tensor([[1, 2]]))


def test_bidirectional_is_refused():
    from speechbrain_amd.nnet.RNN import GRU
    with pytest.raises(NotImplementedError):
        GRU(5, input_size=20, bidirectional=True)
    with pytest.raises(ValueError):
        GRU(5)


def test_searcher_dispatches_on_the_class_name():
    from speechbrain_amd.decoders.transducer import _RNN_NAMES
    from speechbrain_amd.nnet.RNN import GRU
    assert GRU.__name__ in _RNN_NAMES


def test_entry_points_declared_bound_exported_and_checked():
    from speechbrain_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sbk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        from speechbrain_amd import _build
        _build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
        getattr(lib, s).argtypes = _lib.SIGNATURES[s]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)   # a non-null pointer; nothing is launched below
    N = None
    # sbk_gru_fwd(bf16, w_hh, b_hh, hx, gi, tok, blank, table, I, b_ih, lens, B, T, H, state, y, save, stream)
    assert lib.sbk_gru_fwd(0, N, N, N, p, N, 0, N, 0, N, N, 2, 2, 4, p, N, N, N) == 1001      # no w_hh
    assert lib.sbk_gru_fwd(0, p, N, N, p, N, 0, N, 0, N, N, 2, 2, 4, N, N, N, N) == 1001      # no state
    assert lib.sbk_gru_fwd(0, p, N, N, N, N, 0, N, 0, N, N, 2, 2, 4, p, N, N, N) == 1001      # neither gi nor tok
    assert lib.sbk_gru_fwd(0, p, N, N, p, p, 0, p, 3, N, N, 2, 2, 4, p, N, N, N) == 1001      # both
    assert lib.sbk_gru_fwd(0, p, N, N, N, p, 0, N, 3, N, N, 2, 2, 4, p, N, N, N) == 1001      # tok without table
    assert lib.sbk_gru_fwd(1, p, N, N, N, p, 0, p, 0, N, N, 2, 2, 4, p, N, N, N) == 1001      # I = 0
    for B, T, H in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (-1, 2, 4)):
        assert lib.sbk_gru_fwd(0, p, N, N, p, N, 0, N, 0, N, N, B, T, H, p, N, N, N) == 1001
    # sbk_gru_bwd(bf16, w_hhT, hx, state, save, dy, dhn, lens, B, T, H, dgi, dgh, dhw, dhx, stream)
    good = [0, p, N, p, p, p, N, N, 2, 2, 4, p, p, p, p, N]
    for i in (1, 3, 4, 11, 12, 13, 14):
        a = list(good)
        a[i] = N
        assert lib.sbk_gru_bwd(*a) == 1001, i
    for i in (8, 9, 10):
        a = list(good)
        a[i] = 0
        assert lib.sbk_gru_bwd(*a) == 1001, i
    # sbk_embed_onehot(ids, N, V, blank, out, stream)
    assert lib.sbk_embed_onehot(N, 2, 7, 0, p, N) == 1001
    assert lib.sbk_embed_onehot(p, 2, 7, 0, N, N) == 1001
    assert lib.sbk_embed_onehot(p, 0, 7, 0, p, N) == 1001
    assert lib.sbk_embed_onehot(p, 2, 1, 0, p, N) == 1001
    assert lib.sbk_embed_onehot(p, 2, 7, 7, p, N) == 1001
    assert lib.sbk_embed_onehot(p, 2, 7, -1, p, N) == 1001
    # sbk_embed_gather(ids, weight, N, V, D, out, stream)
    assert lib.sbk_embed_gather(N, p, 2, 7, 4, p, N) == 1001
    assert lib.sbk_embed_gather(p, N, 2, 7, 4, p, N) == 1001
    assert lib.sbk_embed_gather(p, p, 2, 7, 4, N, N) == 1001
    for n, v, d in ((0, 7, 4), (2, 0, 4), (2, 7, 0)):
        assert lib.sbk_embed_gather(p, p, n, v, d, p, N) == 1001
    # sbk_segsum_rows(src, order, offs, items, ncodes, D, out, stream)
    good = [p, p, p, 4, 2, 4, p, N]
    for i in (0, 1, 2, 6):
        a = list(good)
        a[i] = N
        assert lib.sbk_segsum_rows(*a) == 1001, i
    for i in (3, 4, 5):
        a = list(good)
        a[i] = 0
        assert lib.sbk_segsum_rows(*a) == 1001, i
