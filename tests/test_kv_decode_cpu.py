"""CPU checks of incremental transformer decoding (csrc/kvdec.hip,
speechbrain_amd._kvdec, TransformerASR.decode_step, the search's
USE_KV_CACHE): both C entry points refuse bad arguments before any launch,
the ops are registered, CPU tensors are refused (no fallback), and the search
keeps the cache off by default."""
import ctypes
import os

import pytest
import torch


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


def test_self_attn_entry_point_checks_arguments_on_the_host():
    lib = _lib()
    buf, p = _dummy()
    # (q, k_new, v_new, ld, kc, vc, cap, anc, anc_ld, N, H, dh, L, out, stream)
    call = lambda q=p, k=p, v=p, ld=96, kc=p, vc=p, cap=8, anc=p, anc_ld=8, N=6, H=2, dh=16, L=3, out=p: \
        lib.sbk_kv_decode_self_attn(q, k, v, ld, kc, vc, cap, anc, anc_ld, N, H, dh, L, out, None)
    for name in ("q", "k", "v", "kc", "vc", "anc", "out"):
        assert call(**{name: None}) == 1001, name               # a null required pointer
    for name in ("N", "H", "dh", "L"):
        assert call(**{name: 0}) == 1001 and call(**{name: -1}) == 1001, name
    assert call(dh=18, ld=108) == 1001                          # dh % 4 != 0
    assert call(dh=132, ld=3 * 264) == 1001                     # dh > 128
    assert call(L=9) == 1001                                    # L > cap
    assert call(ld=31) == 1001                                  # a stride smaller than E = 32
    assert call(ld=28) == 1001


def test_cross_attn_entry_point_checks_arguments_on_the_host():
    lib = _lib()
    buf, p = _dummy()
    # (q, q_ld, k, v, kv_ld, klen, N, group, H, dh, S, out, probs, stream)
    call = lambda q=p, q_ld=32, k=p, v=p, kv_ld=64, klen=None, N=6, group=2, H=2, dh=16, S=21, out=p, probs=None: \
        lib.sbk_kv_decode_cross_attn(q, q_ld, k, v, kv_ld, klen, N, group, H, dh, S, out, probs, None)
    for name in ("q", "k", "v", "out"):
        assert call(**{name: None}) == 1001, name
    for name in ("N", "H", "dh", "S", "group"):
        assert call(**{name: 0}) == 1001 and call(**{name: -1}) == 1001, name
    assert call(dh=18, q_ld=36, kv_ld=72) == 1001               # dh % 4 != 0
    assert call(dh=132, q_ld=264, kv_ld=528) == 1001            # dh > 128
    assert call(group=4) == 1001                                # N % group != 0
    assert call(q_ld=28) == 1001 and call(kv_ld=28) == 1001     # a stride smaller than E = 32
    assert call(klen=p, probs=p, group=4) == 1001               # the optional pointers change nothing


def test_ops_are_registered():
    from speechbrain_amd.decoders import seq2seq  # noqa: F401
    from speechbrain_amd._lib import OPS
    for op in ("kv_decode_self_attn", "kv_decode_cross_attn"):
        assert getattr(OPS, op) is not None
        assert hasattr(torch.ops.sbk, op)


def _tiny():
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    return TransformerASR(tgt_vocab=11, input_size=8, d_model=16, nhead=2, num_encoder_layers=1,
                          num_decoder_layers=1, d_ffn=32, dropout=0.0, normalize_before=True).eval()


def test_cpu_tensors_raise():
    from speechbrain_amd._kvdec import DecodeState, kv_decode_cross_attn, kv_decode_self_attn
    from speechbrain_amd._lib import SbkError
    tr = _tiny()
    assert tr.decode_step_supported()
    with pytest.raises(SbkError):
        tr.init_decode_state(torch.randn(2, 5, 16))
    state = DecodeState([torch.zeros(2, 5, 32)], None, 1, 2)   # a state of CPU tensors
    with pytest.raises(SbkError):
        tr.decode_step(torch.tensor([1, 1]), state)
    with pytest.raises(SbkError):
        kv_decode_self_attn(torch.zeros(2, 48), torch.zeros(4, 2, 16), torch.zeros(4, 2, 16),
                            torch.zeros(2, 4, dtype=torch.int32), 2, 1)
    with pytest.raises(SbkError):
        kv_decode_cross_attn(torch.zeros(2, 16), torch.zeros(2, 5, 32), None, 1, 2, False)


def test_decode_step_supported_follows_the_head_size():
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    kw = dict(tgt_vocab=11, input_size=8, num_encoder_layers=1, num_decoder_layers=1, d_ffn=32, dropout=0.0,
              normalize_before=True)
    assert TransformerASR(d_model=24, nhead=4, **kw).decode_step_supported() is False      # dh 6
    assert TransformerASR(d_model=24, nhead=2, **kw).decode_step_supported() is True       # dh 12
    assert TransformerASR(d_model=16, nhead=2, **{**kw, "num_decoder_layers": 0}).decode_step_supported() is False


def test_state_capacity_and_permute():
    """The capacity starts at 32 positions and doubles by copy; permute moves
    the ancestry rows only."""
    from speechbrain_amd._kvdec import INITIAL_CAPACITY, DecodeState
    state = DecodeState([torch.zeros(2, 5, 8)], None, 3, 2)
    assert INITIAL_CAPACITY == 32 and state.capacity == 32 and state.rows == 6 and state.d_model == 4
    assert state.kc[0].shape == (32, 6, 4) and state.anc.shape == (6, 32)
    state.kc[0].copy_(torch.arange(32 * 6 * 4).view(32, 6, 4))
    for t in range(33):
        assert state.begin_step() == t + 1
        state.steps = t + 1
        if t == 1:
            kc = state.kc[0]
            assert state.permute(torch.tensor([1, 0, 2, 3, 5, 5])) is state
            assert state.kc[0] is kc                                         # the cache is not moved
            assert state.anc[:, :2].tolist() == [[1, 1], [0, 0], [2, 2], [3, 3], [5, 5], [5, 5]]
    assert state.capacity == 64 and state.kc[0].shape == (64, 6, 4) and state.anc.shape == (6, 64)
    assert torch.equal(state.kc[0][:32], torch.arange(32 * 6 * 4).view(32, 6, 4).float())
    assert state.anc[:, 0].tolist() == [1, 0, 2, 3, 5, 5] and state.anc[:, 32].tolist() == list(range(6))


def test_cache_is_off_by_default():
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    assert S2STransformerBeamSearch.USE_KV_CACHE is False
