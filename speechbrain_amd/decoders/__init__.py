"""Decoders (speechbrain/decoders): the transducer beam searcher
(transducer.py), the CTC prefix scorer and CTC greedy decode (ctc.py), and
the attention decoders' search — S2SGreedySearcher, S2SBeamSearcher,
S2STransformerBeamSearch with joint CTC/attention scoring and the RNN
searchers S2SRNNGreedySearcher, S2SRNNBeamSearcher, S2SRNNBeamSearchLM,
S2SRNNBeamSearchTransformerLM (seq2seq.py)."""
from .seq2seq import (S2SRNNBeamSearcher, S2SRNNBeamSearchLM, S2SRNNBeamSearchTransformerLM,  # noqa: F401
                      S2SRNNGreedySearcher)
