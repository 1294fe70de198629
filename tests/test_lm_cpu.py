"""CPU checks of the TransformerLM drop-in and of key/value-cached LM fusion
(lobes/models/transformer/TransformerLM.py, csrc/kvdec.hip's masked decode
step, csrc/lmfuse.hip, the search's USE_LM_KV_CACHE) against
tests/golden/lm.npz: the module tree, the seeded construction and the
constructor signature are the reference's; both new C entry points refuse bad
arguments before any launch; the incremental step names what it supports; the
cache is off by default."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

ACT = {"GELU": torch.nn.GELU, "ReLU": torch.nn.ReLU}
PE = "positional_encoding.pe"


def _lm(kw):
    from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM
    return TransformerLM(**{**kw, "activation": ACT[kw["activation"]]})


def _sub(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


@pytest.mark.parametrize("name", ["A", "B"])
def test_state_dict_loads_strictly(golden, name):
    g = golden("lm")
    assert g["lm.names"].tolist() == ["A", "B"]
    lm = _lm(json.loads(str(g[f"lm.{name}.kw"])))
    sd = _sub(g, f"lm.{name}.sd.")
    pe = lm.state_dict()[PE]
    assert np.allclose(pe[:, :16].numpy(), g["lm.pe_head"], rtol=1e-6, atol=1e-7)
    assert sorted(list(sd) + [PE]) == sorted(lm.state_dict())
    sd[PE] = pe     # the sine table is a buffer: the fixture keeps its head only
    lm.load_state_dict(sd, strict=True)
    assert (lm.embedding_proj is not None) == (name == "B")
    assert not hasattr(lm, "decoder")
    layers = lm.output_proj.layers
    assert [type(m).__name__ for m in layers] == ["Linear", "LayerNorm", "Linear"] and layers[1].eps == 1e-6
    assert type(lm.custom_src_module).__name__ == "NormalizedEmbedding"


@pytest.mark.parametrize("name", ["A", "B"])
def test_seeded_construction_is_the_reference(golden, name):
    g = golden("lm")
    torch.manual_seed(0)
    lm = _lm(json.loads(str(g[f"lm.{name}.kw"])))
    want = _sub(g, f"lm.{name}.init.")
    have = {k: v for k, v in lm.state_dict().items() if k != PE}
    assert list(have) == list(want)             # the construction order too
    for k, v in have.items():
        assert np.array_equal(v.numpy(), want[k].numpy()), k


def test_constructor_signature(golden):
    from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM
    want = json.loads(str(golden("lm")["lm.signature"]))
    have = [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(TransformerLM.__init__).parameters.values()]
    assert have == want


def test_decoder_variant_builds_the_decoder():
    kw = dict(vocab=11, d_model=16, nhead=2, num_encoder_layers=1, d_ffn=32, dropout=0.0, activation="ReLU")
    lm = _lm({**kw, "num_decoder_layers": 1})
    assert any(k.startswith("decoder.layers.0.mutihead_attn.") for k in lm.state_dict())
    assert any(k.startswith("decoder.norm.") for k in lm.state_dict())


def test_decode_step_supported():
    kw = dict(vocab=11, d_model=16, nhead=2, num_encoder_layers=1, d_ffn=32, dropout=0.0, activation="GELU")
    assert _lm(kw).decode_step_supported() is True
    assert _lm({**kw, "activation": "ReLU", "normalize_before": True, "d_embedding": 8}).decode_step_supported() is True
    assert _lm({**kw, "attention_type": "RelPosMHAXL"}).decode_step_supported() is False
    assert _lm({**kw, "num_decoder_layers": 1}).decode_step_supported() is False
    assert _lm({**kw, "d_model": 24, "nhead": 4}).decode_step_supported() is False      # dh 6
    with pytest.raises(NotImplementedError):
        _lm({**kw, "d_model": 24, "nhead": 4}).init_decode_state(4)


def test_lm_cache_is_off_by_default():
    from speechbrain_amd.decoders.seq2seq import S2SBeamSearcher, S2STransformerBeamSearch
    assert S2STransformerBeamSearch.USE_LM_KV_CACHE is False
    assert S2STransformerBeamSearch.USE_KV_CACHE is False
    # the hook of the base loop is the reference's line
    s = S2SBeamSearcher(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=2,
                        lm_weight=0.6)
    a, b = torch.randn(4, 7), torch.randn(4, 7)
    assert torch.equal(s._add_lm_scores(a, b), a + 0.6 * b)


def _lib():
    from speechbrain_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from speechbrain_amd import _build
        _build.build()
    return _lib.lib()


def _dummy():
    """A non-null, 16-byte aligned pointer that is never dereferenced."""
    buf = (ctypes.c_double * 8)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(addr)


def test_masked_self_attn_entry_point_checks_arguments_on_the_host():
    lib = _lib()
    buf, p = _dummy()
    # (q, k_new, v_new, ld, kc, vc, cap, anc, anc_ld, keymask, N, H, dh, L, out, stream)
    call = lambda q=p, k=p, v=p, ld=96, kc=p, vc=p, cap=8, anc=p, anc_ld=8, km=p, N=6, H=2, dh=16, L=3, out=p: \
        lib.sbk_kv_decode_self_attn_masked(q, k, v, ld, kc, vc, cap, anc, anc_ld, km, N, H, dh, L, out, None)
    for name in ("q", "k", "v", "kc", "vc", "anc", "km", "out"):
        assert call(**{name: None}) == 1001, name               # a null required pointer, the mask among them
    for name in ("N", "H", "dh", "L"):
        assert call(**{name: 0}) == 1001 and call(**{name: -1}) == 1001, name
    assert call(dh=18, ld=108) == 1001                          # dh % 4 != 0
    assert call(dh=132, ld=3 * 264) == 1001                     # dh > 128
    assert call(L=9) == 1001 and call(cap=2) == 1001            # cap smaller than L
    assert call(anc_ld=2) == 1001
    assert call(ld=31) == 1001 and call(ld=28) == 1001          # a stride smaller than E = 32


def test_log_softmax_fuse_entry_point_checks_arguments_on_the_host():
    lib = _lib()
    buf, p = _dummy()
    # (logits, ld, base, base_ld, N, V, invT, w, out, stream)
    call = lambda x=p, ld=40, base=p, base_ld=40, N=3, V=40, out=p: \
        lib.sbk_log_softmax_fuse(x, ld, base, base_ld, N, V, 1.0, 0.6, out, None)
    assert call(x=None) == 1001 and call(out=None) == 1001
    for name in ("N", "V"):
        assert call(**{name: 0}) == 1001 and call(**{name: -1}) == 1001, name
    assert call(ld=39) == 1001 and call(base_ld=39) == 1001     # a stride smaller than V
    assert call(V=41) == 1001


def test_ops_are_registered_and_refuse_cpu_tensors():
    from speechbrain_amd._kvdec import LMDecodeState, kv_decode_self_attn_masked, log_softmax_fuse
    from speechbrain_amd._lib import OPS, SbkError
    for op in ("kv_decode_self_attn_masked", "log_softmax_fuse"):
        assert getattr(OPS, op) is not None and hasattr(torch.ops.sbk, op)
    with pytest.raises(SbkError):
        kv_decode_self_attn_masked(torch.zeros(2, 48), torch.zeros(4, 2, 16), torch.zeros(4, 2, 16),
                                   torch.zeros(2, 4, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.uint8), 2, 1)
    with pytest.raises(SbkError):
        log_softmax_fuse(torch.zeros(2, 5), None, 1.0, 0.6)
    lm = _lm(dict(vocab=11, d_model=16, nhead=2, num_encoder_layers=1, d_ffn=32, dropout=0.0, activation="GELU"))
    with pytest.raises(SbkError):
        lm.init_decode_state(4)                 # a model on the CPU
    with pytest.raises(SbkError):
        lm.decode_step(torch.tensor([1, 1]), LMDecodeState(2, 1, 16, 2, torch.device("cpu")))


def test_lm_state_capacity_mask_and_permute():
    """DecodeState's scheme plus the key mask: the capacity doubles by copy,
    slot L−1 of the mask is the step's, permute moves the ancestry rows only."""
    from speechbrain_amd._kvdec import LMDecodeState
    state = LMDecodeState(4, 2, 8, 2, torch.device("cpu"))
    assert state.capacity == 32 and state.kc[1].shape == (32, 4, 8) and state.keymask.shape == (32, 4)
    assert state.keymask.dtype == torch.uint8 and len(state.kc) == len(state.vc) == 2
    for t in range(33):
        masked = torch.tensor([t % 2 == 0, False, t == 32, True])
        assert state.begin_step(masked) == t + 1
        state.steps = t + 1
        assert state.keymask[t].tolist() == masked.int().tolist()
        if t == 1:
            kc, km = state.kc[0], state.keymask
            assert state.permute(torch.tensor([1, 1, 0, 3])) is state
            assert state.kc[0] is kc and state.keymask is km
            assert state.anc[:, :2].tolist() == [[1, 1], [1, 1], [0, 0], [3, 3]]
    assert state.capacity == 64 and state.keymask.shape == (64, 4) and state.kc[0].shape == (64, 4, 8)
    assert state.keymask[:33, 0].tolist() == [1 - t % 2 for t in range(33)]
    assert state.keymask[32].tolist() == [1, 0, 1, 1] and not bool(state.keymask[33:].any())
