"""GPU checks of speechbrain_amd.decoders.ctc against tests/golden/s2s.npz
(the reference's CTCPrefixScorer run on the CPU by gen_s2s_golden.py) and of
the CTC greedy decode against a plain Python restatement.

Bound: the project's fp32 bound |a − b| <= 1e-4·max(1, |b|), sentinel
(−1e20) entries included.  Largest deviation observed on an MI355X over all
scorer scripts: 8.4e-7 (wide_full)."""
from itertools import groupby

import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

SCRIPTS = ["small_full", "small_partial", "single", "wide_full", "long_prefix", "blank3"]


def _scorer(g, name, dev):
    from speechbrain_amd.decoders.ctc import CTCPrefixScorer
    k = f"scorer.{name}"
    beam, blank, eos, n_steps, C = (int(v) for v in g[k + ".cfg"])
    x = torch.from_numpy(g[k + ".x"]).to(dev)
    lens = torch.from_numpy(g[k + ".lens"]).to(dev)
    return CTCPrefixScorer(x, lens, x.shape[0], beam, blank, eos), n_steps, C


def _step_inputs(g, name, i, C, dev):
    k = f"scorer.{name}.{i}"
    cand = torch.from_numpy(g[k + ".cand"]).to(dev) if C else None
    return torch.from_numpy(g[k + ".g"]).to(dev), cand, torch.from_numpy(g[k + ".index"]).to(dev)


@pytest.mark.parametrize("name", SCRIPTS)
def test_scorer_script_matches_reference(golden, dev, name):
    g = golden("s2s")
    assert sorted(g["scorer.names"].tolist()) == sorted(SCRIPTS)
    scorer, n_steps, C = _scorer(g, name, dev)
    state, worst = None, 0.0
    for i in range(n_steps):
        prefixes, cand, index = _step_inputs(g, name, i, C, dev)
        out, memory = scorer.forward_step(prefixes, state, cand, None)
        state = scorer.permute_mem(memory, index)
        for what, got in (("out", out), ("r", state[0]), ("psi", state[1])):
            ref = g[f"scorer.{name}.{i}.{what}"]
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            worst = max(worst, float(err.max()))
            print(f"{name} step {i} {what}: max deviation {err.max():.3e}")
            assert_close(got, ref, name=f"{name}.{i}.{what}")
    print(f"{name}: largest deviation {worst:.3e}")


def test_masking_is_in_place_and_writes_column_zero(golden, dev):
    """ctc.py:58-62: padded frames get the sentinel, then column 0 (not
    blank_index) gets 0 — on the caller's tensor."""
    from speechbrain_amd.decoders.ctc import CTCPrefixScorer
    g = golden("s2s")
    x = torch.from_numpy(g["scorer.blank3.x"]).to(dev)
    before = x.clone()
    CTCPrefixScorer(x, torch.tensor([9, 6], device=dev), 2, 3, 3, 2)
    assert torch.equal(x[0], before[0]) and torch.equal(x[1, :6], before[1, :6])
    assert (x[1, 6:, 0] == 0).all() and (x[1, 6:, 1:] == -1e20).all()


@pytest.mark.parametrize("name", ["small_full", "small_partial", "wide_full"])
def test_step_and_advance_agree_bit_for_bit(golden, dev, name):
    """What the advance stores is what the step scored: with psi_prev = None
    the step's columns are psi itself, and (a) psi_new of the advance equals
    the step's column of every (parent, token) pair, (b) the eos column of the
    NEXT step equals, for every surviving beam, the advance's own log-sum of
    the last valid frame of the state it wrote (its psi_new for token = eos),
    both bit for bit; that log-sum is also torch.logaddexp of the two r rows."""
    from speechbrain_amd.decoders.ctc import ctc_prefix_advance, ctc_prefix_step
    g = golden("s2s")
    scorer, n_steps, C = _scorer(g, name, dev)
    V, beam, N = scorer.vocab_size, scorer.beam_size, scorer.batch_size * scorer.beam_size
    eos = scorer.eos_index
    state = None
    for i in range(n_steps):
        prefixes, cand, index = _step_inputs(g, name, i, C, dev)
        r_prev = scorer._initial_state()[0] if state is None else state[0]
        last = prefixes[:, -1].contiguous() if i > 0 else None
        start = max(1, i)
        args = (beam, i, start, scorer.max_enc_len, scorer.blank_index, eos)
        psi = ctc_prefix_step(scorer.x, r_prev, None, last, cand, scorer._last_frame, *args)
        parent = (index // V + scorer.beam_offset[:, None]).reshape(-1)
        token = (index % V).reshape(-1)
        r_new, psi_new = ctc_prefix_advance(scorer.x, r_prev, last, cand, scorer._last_frame, parent, token, *args)
        assert torch.equal(psi_new, psi[parent, token]), (name, i)
        # the next step on the advanced state, empty walk arguments aside
        nxt_prefix = torch.cat([prefixes[parent], token[:, None]], 1)
        nxt_last = nxt_prefix[:, -1].contiguous()
        nargs = (beam, i + 1, max(1, i + 1), scorer.max_enc_len, scorer.blank_index, eos)
        nxt = ctc_prefix_step(scorer.x, r_new, None, nxt_last, None, scorer._last_frame, *nargs)
        rows = torch.arange(N, device=dev)
        _, eos_psi = ctc_prefix_advance(scorer.x, r_new, nxt_last, None, scorer._last_frame, rows,
                                        torch.full_like(rows, eos), *nargs)
        assert torch.equal(nxt[:, eos], eos_psi), (name, i)
        lf = scorer._last_frame.long().repeat_interleave(beam)
        lse = torch.logaddexp(r_new[lf, 0, rows], r_new[lf, 1, rows])
        assert_close(nxt[:, eos], lse, rtol=1e-6, name=f"{name}.{i}.eos")
        state = (r_new, psi_new)


def test_window_with_attention_is_refused(golden, dev):
    from speechbrain_amd.decoders.ctc import CTCPrefixScorer
    g = golden("s2s")
    x = torch.from_numpy(g["scorer.single.x"]).to(dev)
    scorer = CTCPrefixScorer(x, torch.tensor([2], device=dev), 1, 1, 0, 2, ctc_window_size=3)
    prefixes = torch.empty(1, 0, dtype=torch.long, device=dev)
    with pytest.raises(NotImplementedError, match="ctc_window_size"):
        scorer.forward_step(prefixes, None, None, torch.zeros(1, 2, device=dev))
    out, _ = scorer.forward_step(prefixes, None, None, None)      # no attention map: the full walk
    assert out.shape == (1, 5)


# ------------------------------------------------------------------- greedy
def _greedy_restated(probs, rel_lens, blank):
    """argmax per frame (first index on a tie), group, filter."""
    probs = probs.cpu().numpy()
    B, T, V = probs.shape
    if blank < 0:
        blank += V
    outs = []
    for b in range(B):
        n = int(torch.round(rel_lens[b].cpu() * T))
        labels = [int(np.argmax(probs[b, t])) for t in range(n)]
        outs.append([k for k, _ in groupby(labels) if k != blank])
    return outs


def test_greedy_doctest(dev):
    from speechbrain_amd.decoders.ctc import ctc_greedy_decode
    probs = torch.tensor([[[0.3, 0.7], [0.0, 0.0]], [[0.2, 0.8], [0.9, 0.1]]], device=dev)
    assert ctc_greedy_decode(probs, torch.tensor([0.51, 1.0], device=dev), 0) == [[1], [1]]


@pytest.mark.parametrize("blank", [0, -1, 5])
def test_greedy_seeded_batch(dev, blank):
    from speechbrain_amd.decoders.ctc import ctc_greedy_decode
    gen = torch.Generator().manual_seed(21)
    # few distinct winners, so that repeats and blanks occur
    probs = torch.randn(3, 37, 29, generator=gen)
    probs[:, :, [0, 5, 28]] += 2.0
    probs = probs.log_softmax(-1).to(dev)
    lens = torch.tensor([1.0, 0.4, 0.0], device=dev)
    want = _greedy_restated(probs, lens, blank)
    assert want[2] == [] and 0 < len(want[1]) < len(want[0]) < 37
    assert ctc_greedy_decode(probs, lens, blank) == want
    # strided input (time-major storage) and CPU lengths
    tm = probs.transpose(0, 1).contiguous().transpose(0, 1)
    assert not tm.is_contiguous()
    assert ctc_greedy_decode(tm, lens.cpu(), blank) == want


def test_greedy_wide_vocabulary_tie_and_long_utterance(dev):
    from speechbrain_amd.decoders.ctc import ctc_greedy_decode
    gen = torch.Generator().manual_seed(22)
    probs = torch.rand(2, 5, 1000, generator=gen)
    probs[0, 2, 700] = probs[0, 2, 333] = 2.0      # a tie: the lower index wins
    probs[1, 0, 999] = probs[1, 1, 999] = 3.0      # a repeat in the last class
    probs = probs.to(dev)
    lens = torch.ones(2, device=dev)
    want = _greedy_restated(probs, lens, 0)
    assert 333 in want[0] and 700 not in want[0] and want[1][0] == 999
    assert ctc_greedy_decode(probs, lens, 0) == want
    assert ctc_greedy_decode(probs, lens, -1) == _greedy_restated(probs, lens, -1)
    # more frames than one compaction chunk (256), every frame kept / runs across the chunk edge
    T = 600
    labels = torch.arange(T) % 7 + 1
    labels[250:262] = 3
    long = torch.nn.functional.one_hot(labels, 9).float()[None].to(dev)
    one = torch.ones(1, device=dev)
    assert ctc_greedy_decode(long, one, 0) == _greedy_restated(long, one, 0)


def test_filter_ctc_output_refuses_non_lists():
    from speechbrain_amd.decoders.ctc import filter_ctc_output
    assert filter_ctc_output(["a", "a", "blank", "b", "b", "blank", "c"], blank_id="blank") == ["a", "b", "c"]
    with pytest.raises(ValueError, match="python lists"):
        filter_ctc_output(torch.tensor([1, 1, 2]), blank_id=0)
