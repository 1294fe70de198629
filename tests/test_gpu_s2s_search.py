"""GPU checks of speechbrain_amd.decoders.seq2seq against tests/golden/s2s.npz:
the reference's S2STransformerBeamSearch (and its greedy base class) run on
the CPU by gen_s2s_golden.py, on a seeded tiny TransformerASR + seq_lin /
ctc_lin whose state_dicts the drop-ins load with strict=True.

Hypotheses must equal the fixture's exactly (the generator stores only cases
whose hypotheses survive 1e-4 relative noise on the encoder states); scores
and log-probs within |a − b| <= 1e-4·max(1, |b|).  Largest deviation observed
on an MI355X over all cases: 9.5e-7 on topk_scores, 1.8e-6 on log_probs
(see DESIGN §7)."""
import json

import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

CASES = ["w0.0_full", "w0.0_partial", "w0.4_full", "w0.4_partial", "w1.0_full", "w1.0_partial", "beam1",
         "no_lennorm", "eos_thr"]


@pytest.fixture(scope="module")
def setup(golden, dev):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from speechbrain_amd.nnet.linear import Linear
    g = golden("s2s")
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=64, nhead=4, num_encoder_layers=1,
                        num_decoder_layers=2, d_ffn=128, dropout=0.0, activation=torch.nn.GELU,
                        normalize_before=True)
    seq_lin = Linear(input_size=64, n_neurons=23)
    ctc_lin = Linear(input_size=64, n_neurons=23)

    def sub(prefix):
        return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}

    sd = sub("search.sd.tr.")
    # the sine table is a buffer, not a weight: the fixture keeps its head only
    pe = tr.state_dict()["positional_encoding.pe"]
    assert_close(pe[:, :32], g["search.pe_head"], rtol=1e-6, name="pe")
    sd["positional_encoding.pe"] = pe
    tr.load_state_dict(sd, strict=True)
    seq_lin.load_state_dict(sub("search.sd.seq."), strict=True)
    ctc_lin.load_state_dict(sub("search.sd.ctc."), strict=True)
    modules = [m.to(dev).eval() for m in (tr, seq_lin, ctc_lin)]
    enc = torch.from_numpy(g["search.enc"]).to(dev)
    wav_len = torch.from_numpy(g["search.wav_len"]).to(dev)
    return g, modules, enc, wav_len


def _unpad(a, fill):
    keep = ~np.isnan(a) if np.isnan(fill) else a != fill
    return [row[k].tolist() for row, k in zip(a, keep)]


def _check(g, name, res):
    pred = _unpad(g[f"search.{name}.pred"], -1)
    assert res[0] == pred, name
    ref = g[f"search.{name}.scores"]
    dev_scores = float(np.max(np.abs(res[1].cpu().numpy() - ref) / np.maximum(1, np.abs(ref))))
    print(f"{name}: topk_scores max deviation {dev_scores:.3e}")
    assert_close(res[1], ref, name=f"{name}.scores")
    if f"search.{name}.log_probs" in g.files:
        want = _unpad(g[f"search.{name}.log_probs"], np.nan)
        assert len(res[2]) == len(want)
        for got, w in zip(res[2], want):
            w = np.asarray(w, dtype=np.float32)
            print(f"{name}: log_probs max deviation "
                  f"{float(np.max(np.abs(got.cpu().numpy() - w) / np.maximum(1, np.abs(w)))):.3e}")
            assert_close(got, w, name=f"{name}.log_probs")
    else:
        assert len(res) == 2


@pytest.mark.parametrize("name", CASES)
def test_beam_search_matches_reference(setup, name):
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    g, modules, enc, wav_len = setup
    assert sorted(g["search.names"].tolist()) == sorted(CASES)
    cfg = json.loads(str(g[f"search.{name}.cfg"]))
    searcher = S2STransformerBeamSearch(modules=modules, **cfg)
    _check(g, name, searcher(enc.clone(), wav_len))


def test_full_and_partial_differ_at_joint_weight(setup):
    """The two modes are different searches, not one code path twice."""
    g = setup[0]
    assert not np.array_equal(g["search.w0.4_full.pred"], g["search.w0.4_partial.pred"])


def test_search_on_a_side_stream(setup, dev):
    """The kernels run on the caller's stream: the same search inside a
    non-default stream gives the same result."""
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    g, modules, enc, wav_len = setup
    cfg = json.loads(str(g["search.w0.4_partial.cfg"]))
    searcher = S2STransformerBeamSearch(modules=modules, **cfg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = searcher(enc.clone(), wav_len)
    side.synchronize()
    _check(g, "w0.4_partial", res)


def test_greedy_searcher_matches_reference(setup):
    from speechbrain_amd.decoders.seq2seq import S2SGreedySearcher, S2STransformerBeamSearch, _update_mem
    g, modules, enc, wav_len = setup

    class Greedy(S2SGreedySearcher):
        def __init__(self, modules, **kw):
            super().__init__(**kw)
            self.model, self.fc = modules[0], modules[1]

        def reset_mem(self, batch_size, device):
            return None

        def forward_step(self, inp_tokens, memory, enc_states, enc_lens):
            memory = _update_mem(inp_tokens, memory)
            pred, attn = self.model.decode(memory, enc_states)
            return self.fc(pred).log_softmax(-1)[:, -1, :], memory, attn

    pred, scores = Greedy(modules, bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0)(enc, wav_len)
    assert pred == _unpad(g["greedy.pred"], -1)
    assert_close(np.asarray(scores, dtype=np.float32), g["greedy.scores"], name="greedy.scores")
    assert S2STransformerBeamSearch.forward_step is not S2SGreedySearcher.forward_step


def test_constructor_errors(setup):
    from speechbrain_amd.decoders.seq2seq import S2SBeamSearcher, S2STransformerBeamSearch
    modules = setup[1]
    base = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=4)
    with pytest.raises(ValueError, match="length normalization is not compatible"):
        S2SBeamSearcher(**base, length_rewarding=0.5)
    S2SBeamSearcher(**base, length_normalization=False, length_rewarding=0.5)
    for clash in (dict(blank_index=2), dict(blank_index=1), dict(bos_index=2)):
        with pytest.raises(ValueError, match="different indexes"):
            S2STransformerBeamSearch(modules=modules, **{**base, "ctc_weight": 0.4, **clash})
    S2STransformerBeamSearch(modules=modules, **{**base, "blank_index": 2})      # no CTC term: no clash
    with pytest.raises(NotImplementedError, match="using_max_attn_shift is RNN-searcher-only"):
        S2STransformerBeamSearch(modules=modules, **base, using_max_attn_shift=True)
    with pytest.raises(NotImplementedError, match="coverage_penalty is RNN-searcher-only"):
        S2STransformerBeamSearch(modules=modules, **base, coverage_penalty=0.5)


def test_window_with_attention_is_refused_by_the_search(setup):
    """The third NotImplementedError: the attention-peak CTC window."""
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    g, modules, enc, wav_len = setup
    searcher = S2STransformerBeamSearch(modules=modules, bos_index=1, eos_index=2, min_decode_ratio=0.0,
                                        max_decode_ratio=1.0, beam_size=2, ctc_weight=0.4, ctc_window_size=5)
    with pytest.raises(NotImplementedError, match="ctc_window_size"):
        searcher(enc.clone(), wav_len)


def test_helpers(dev):
    from speechbrain_amd.decoders.seq2seq import batch_filter_seq2seq_output, inflate_tensor, mask_by_condition
    t = torch.tensor([[1., 2., 3.], [4., 5., 6.]], device=dev)
    assert inflate_tensor(t, 2, dim=0).tolist() == [[1, 2, 3], [1, 2, 3], [4, 5, 6], [4, 5, 6]]
    cond = torch.tensor([[True, True, False], [True, False, False]], device=dev)
    assert mask_by_condition(t, cond, 0).tolist() == [[1, 2, 0], [4, 0, 0]]
    preds = [torch.tensor([1, 2, 3, 4], device=dev), torch.tensor([2, 3, 4, 5, 6], device=dev)]
    assert batch_filter_seq2seq_output(preds, eos_id=4) == [[1, 2, 3], [2, 3]]
