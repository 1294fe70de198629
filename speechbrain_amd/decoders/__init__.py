"""Decoders (speechbrain/decoders): the transducer beam searcher
(transducer.py), the CTC prefix scorer and CTC greedy decode (ctc.py), and
the attention decoders' search — S2SGreedySearcher, S2SBeamSearcher and
S2STransformerBeamSearch with joint CTC/attention scoring (seq2seq.py)."""
