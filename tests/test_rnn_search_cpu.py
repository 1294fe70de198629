"""CPU checks of the RNN searchers' public surface (no GPU needed)."""
import pytest


def test_rnn_searchers_take_coverage_and_attention_shift():
    from speechbrain_amd import decoders
    from speechbrain_amd.decoders.seq2seq import S2SBeamSearcher
    base = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=4)
    s = decoders.S2SRNNBeamSearcher(None, None, None, coverage_penalty=1.5, using_max_attn_shift=True,
                                    max_attn_shift=240, **base)
    assert (s.coverage_penalty, s.using_max_attn_shift, s.max_attn_shift) == (1.5, True, 240)
    assert issubclass(decoders.S2SRNNBeamSearchLM, decoders.S2SRNNBeamSearcher) and issubclass(
        decoders.S2SRNNBeamSearchTransformerLM, decoders.S2SRNNBeamSearcher)
    decoders.S2SRNNGreedySearcher(None, None, None, bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0)
    with pytest.raises(NotImplementedError, match="RNN-searcher-only"):
        S2SBeamSearcher(coverage_penalty=1.5, **base)
    with pytest.raises(ValueError, match="ctc_fc is required"):
        decoders.S2SRNNBeamSearcher(None, None, None, ctc_weight=0.4, **base)
