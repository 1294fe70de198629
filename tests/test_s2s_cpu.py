"""CPU checks of the decoding drop-ins (speechbrain_amd.decoders.ctc /
.seq2seq): the C entry points refuse bad arguments before any launch, the
public signatures are the reference's (recorded in tests/golden/s2s.npz by
gen_s2s_golden.py from the reference's own signatures), CPU tensors are
refused (no fallback), and the pure-Python helpers give the fixture's
outputs."""
import ctypes
import inspect
import json
import os

import pytest
import torch


def _lib():
    from speechbrain_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from speechbrain_amd import _build
        _build.build()
    return _lib.lib()


def test_prefix_entry_points_check_arguments_on_the_host():
    lib = _lib()
    buf = (ctypes.c_double * 4)()   # non-null; never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (x, r_prev, psi_prev, last_tok, cand, last_frame, B, beam, T, V, C, prefix_len, start, end, blank, eos, out, stream)
    step = lambda x=p, cand=None, B=2, beam=3, T=9, V=7, C=0, plen=0, start=1, end=9, blank=0, eos=2, out=p: \
        lib.sbk_ctc_prefix_step(x, p, None, None, cand, p, B, beam, T, V, C, plen, start, end, blank, eos, out, None)
    adv = lambda x=p, cand=None, B=2, beam=3, T=9, V=7, C=0, plen=0, start=1, end=9, blank=0, eos=2, parent=p: \
        lib.sbk_ctc_prefix_advance(x, p, None, cand, p, parent, p, B, beam, T, V, C, plen, start, end, blank, eos,
                                   p, p, None)
    for fn in (step, adv):
        assert fn(x=None) == 1001                   # a null x
        assert fn(T=0, end=0) == 1001               # T = 0
        assert fn(cand=p, C=8) == 1001              # C > V
        assert fn(cand=p, C=0) == 1001              # candidates without a count
        assert fn(C=4) == 1001                      # a count without candidates
        assert fn(beam=0) == 1001                   # beam = 0
        assert fn(end=10) == 1001                   # end > T
        assert fn(start=0) == 1001 and fn(start=10) == 1001
        assert fn(blank=7) == 1001 and fn(eos=-1) == 1001
        assert fn(T=4097, end=4097) == 1001         # above the staged frames
    assert step(out=None) == 1001
    assert adv(parent=None) == 1001


def test_greedy_entry_point_checks_arguments_on_the_host():
    lib = _lib()
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.sbk_ctc_greedy_decode(None, 10, 5, 1, p, 1, 2, 5, 0, p, p, None) == 1001
    assert lib.sbk_ctc_greedy_decode(p, 10, 5, 1, p, 1, 0, 5, 0, p, p, None) == 1001
    assert lib.sbk_ctc_greedy_decode(p, 10, 5, 1, p, 0, 2, 5, 0, p, p, None) == 1001
    assert lib.sbk_ctc_greedy_decode(p, 10, 5, 1, p, 1, 2, 5, 0, p, None, None) == 1001


def _resolve(name):
    from speechbrain_amd.decoders import ctc, seq2seq
    mod, *path = name.split(".")
    obj = {"ctc": ctc, "seq2seq": seq2seq}[mod]
    for part in path:
        obj = getattr(obj, part)
    return obj


def test_public_signatures_are_the_references(golden):
    sigs = json.loads(str(golden("s2s")["signatures"]))
    assert len(sigs) == 15
    for name, want in sigs.items():
        got = [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(_resolve(name)).parameters.values()]
        assert got == want, name
    from speechbrain_amd._lib import OPS
    for op in ("ctc_prefix_step", "ctc_prefix_advance", "ctc_greedy_decode"):
        assert getattr(OPS, op) is not None


def test_pure_helpers_give_the_fixture_outputs(golden):
    from speechbrain_amd.decoders.ctc import filter_ctc_output
    from speechbrain_amd.decoders.seq2seq import filter_seq2seq_output
    rows = json.loads(str(golden("s2s")["filters"]))
    assert len(rows) == 10
    for fn, inp, ident, want in rows:
        if fn == "filter_seq2seq_output":
            assert filter_seq2seq_output(list(inp), eos_id=ident) == want
        else:
            assert filter_ctc_output(list(inp), blank_id=ident) == want
    with pytest.raises(ValueError, match="must be a list"):
        filter_seq2seq_output((1, 2, 3), eos_id=2)
    with pytest.raises(ValueError, match="python lists"):
        filter_ctc_output("aab", blank_id="b")


def test_cpu_tensors_raise():
    from speechbrain_amd._lib import SbkError
    from speechbrain_amd.decoders.ctc import CTCPrefixScorer, ctc_greedy_decode
    with pytest.raises(SbkError):
        ctc_greedy_decode(torch.rand(2, 4, 3), torch.ones(2), 0)
    with pytest.raises(SbkError):
        CTCPrefixScorer(torch.randn(1, 4, 5).log_softmax(-1), torch.tensor([4]), 1, 2, 0, 2)


def test_constructor_errors_need_no_gpu():
    from speechbrain_amd.decoders.seq2seq import S2SBeamSearcher
    base = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=4)
    with pytest.raises(ValueError, match="length normalization"):
        S2SBeamSearcher(**base, length_rewarding=1.0)
    with pytest.raises(ValueError, match="different indexes"):
        S2SBeamSearcher(**base, ctc_weight=0.3, blank_index=1)
    with pytest.raises(NotImplementedError, match="RNN-searcher-only"):
        S2SBeamSearcher(**base, using_max_attn_shift=True)
    with pytest.raises(NotImplementedError, match="RNN-searcher-only"):
        S2SBeamSearcher(**base, coverage_penalty=0.1)
