"""Drop-ins for speechbrain.decoders.seq2seq (decoders/seq2seq.py) on MI355X:
S2SBaseSearcher, S2SGreedySearcher, S2SBeamSearcher, S2STransformerBeamSearch
and the helpers inflate_tensor, mask_by_condition,
batch_filter_seq2seq_output, filter_seq2seq_output.

Same constructor arguments, defaults and return values as the reference
(seq2seq.py:410-475, :1353-1364): (predictions, topk_scores[, log_probs]).
What runs where:
  * the decoder step — model.decode of the package's TransformerASR and the
    seq_lin / ctc_lin drop-in Linears (HIP);
  * the CTC term — speechbrain_amd.decoders.ctc.CTCPrefixScorer: one kernel
    per step and one per beam permutation, in "full" or "partial" mode;
  * the search itself — the reference's order of operations, kept so that the
    hypotheses match: att_weight scaling, eos blocked below min_decode_steps,
    the eos threshold, LM fusion, blank blocked + the CTC term, length
    normalisation, top-k over beam·V, predecessor permutation, eos
    bookkeeping, the final fill-up.  This is torch plumbing on device
    tensors; collecting the finished hypotheses reads the eos positions back
    once per step (the reference reads once per row).
Not carried over, both RNN-searcher features that the reference itself
mishandles for the transformer's 3-D attention map: using_max_attn_shift and
coverage_penalty raise NotImplementedError.
Incremental decoding: with S2STransformerBeamSearch.USE_KV_CACHE set (class or
instance attribute; off by default) and a decoder that
TransformerASR.decode_step_supported() takes, a step runs decode_step — the
newest token only, against a key/value cache and cross-attention K / V
projected once for the un-inflated utterances (csrc/kvdec.hip) — and a beam
permutation moves the cache's (N, L) ancestry table, not the cache.  Otherwise,
like the reference, every step re-decodes the whole prefix.
LM fusion has the same switch, USE_LM_KV_CACHE (off by default): with
lm_modules a TransformerLM that decode_step_supported() takes, the LM step
embeds the newest token only against the LM's own key/value cache, and
log_probs + lm_weight · log_softmax(logits / temperature_lm) is one kernel
(csrc/lmfuse.hip) through the _add_lm_scores hook.  With any other lm_modules
the LM runs on the whole prefix, as in the reference.
"""
import torch

from .. import _kvdec  # registers the decode-step ops the cached search runs
from ..lobes.models.transformer.TransformerLM import TransformerLM
from .ctc import CTCPrefixScorer


class S2SBaseSearcher(torch.nn.Module):
    """seq2seq.py:16-150: the interface of the searchers."""

    def __init__(self, bos_index, eos_index, min_decode_ratio, max_decode_ratio):
        super().__init__()
        self.bos_index = bos_index
        self.eos_index = eos_index
        self.min_decode_ratio = min_decode_ratio
        self.max_decode_ratio = max_decode_ratio

    def forward(self, enc_states, wav_len):
        raise NotImplementedError

    def forward_step(self, inp_tokens, memory, enc_states, enc_lens):
        """→ (log_probs, memory, attn) of one autoregressive step."""
        raise NotImplementedError

    def reset_mem(self, batch_size, device):
        raise NotImplementedError

    def lm_forward_step(self, inp_tokens, memory):
        """→ (log_probs, memory) of one language-model step."""
        raise NotImplementedError

    def reset_lm_mem(self, batch_size, device):
        raise NotImplementedError


class S2SGreedySearcher(S2SBaseSearcher):
    """seq2seq.py:153-196."""

    @torch.no_grad()
    def forward(self, enc_states, wav_len):
        enc_lens = torch.round(enc_states.shape[1] * wav_len).int()
        device = enc_states.device
        batch_size = enc_states.shape[0]
        memory = self.reset_mem(batch_size, device=device)
        inp_tokens = enc_states.new_zeros(batch_size).fill_(self.bos_index).long()
        log_probs_lst = []
        max_decode_steps = int(enc_states.shape[1] * self.max_decode_ratio)
        for t in range(max_decode_steps):
            log_probs, memory, _ = self.forward_step(inp_tokens, memory, enc_states, enc_lens)
            log_probs_lst.append(log_probs)
            inp_tokens = log_probs.argmax(dim=-1)
        log_probs = torch.stack(log_probs_lst, dim=1)
        scores, predictions = log_probs.max(dim=-1)
        scores = scores.sum(dim=1).tolist()
        predictions = batch_filter_seq2seq_output(predictions, eos_id=self.eos_index)
        return predictions, scores


class S2SBeamSearcher(S2SBaseSearcher):
    """seq2seq.py:349-961."""

    def __init__(self, bos_index, eos_index, min_decode_ratio, max_decode_ratio, beam_size, topk=1,
                 return_log_probs=False, using_eos_threshold=True, eos_threshold=1.5, length_normalization=True,
                 length_rewarding=0, coverage_penalty=0.0, lm_weight=0.0, lm_modules=None, ctc_weight=0.0,
                 blank_index=0, ctc_score_mode="full", ctc_window_size=0, using_max_attn_shift=False,
                 max_attn_shift=60, minus_inf=-1e20):
        super().__init__(bos_index, eos_index, min_decode_ratio, max_decode_ratio)
        self.beam_size = beam_size
        self.topk = topk
        self.return_log_probs = return_log_probs
        self.length_normalization = length_normalization
        self.length_rewarding = length_rewarding
        self.coverage_penalty = coverage_penalty
        self.coverage = None

        if self.length_normalization and self.length_rewarding > 0:
            raise ValueError("length normalization is not compatible with length rewarding.")
        if using_max_attn_shift:
            raise NotImplementedError(
                "using_max_attn_shift is RNN-searcher-only: it takes the peak of a 2-D attention vector, and the "
                "reference mishandles the transformer's 3-D attention map (seq2seq.py:500-525)")
        if coverage_penalty > 0:
            raise NotImplementedError(
                "coverage_penalty is RNN-searcher-only: the reference's transformer branch never updates the "
                "coverage it penalises (seq2seq.py:833-835)")

        self.using_eos_threshold = using_eos_threshold
        self.eos_threshold = eos_threshold
        self.using_max_attn_shift = using_max_attn_shift
        self.max_attn_shift = max_attn_shift
        self.lm_weight = lm_weight
        self.lm_modules = lm_modules

        self.ctc_weight = ctc_weight
        self.blank_index = blank_index
        self.att_weight = 1.0 - ctc_weight
        assert 0.0 <= self.ctc_weight <= 1.0, "ctc_weight should not > 1.0 and < 0.0"
        if self.ctc_weight > 0.0:
            if len({self.bos_index, self.eos_index, self.blank_index}) < 3:
                raise ValueError("To perform joint ATT/CTC decoding, set blank, eos and bos to different indexes.")

        self.minus_inf = minus_inf
        self.ctc_score_mode = ctc_score_mode
        self.ctc_window_size = ctc_window_size

    def _check_full_beams(self, hyps, beam_size):
        """Every utterance has beam_size finished hypotheses."""
        return [len(lst) for lst in hyps] == [self.beam_size] * len(hyps)

    def _check_eos_threshold(self, log_probs):
        """eos is kept where its log-prob exceeds eos_threshold × the row's best."""
        max_probs, _ = torch.max(log_probs, dim=-1)
        eos_probs = log_probs[:, self.eos_index]
        return eos_probs > (self.eos_threshold * max_probs)

    def _update_hyp_and_scores(self, inp_tokens, alived_seq, alived_log_probs, hyps_and_scores, scores, timesteps):
        """Store the rows whose token is eos (seq2seq.py:546-596).  One
        read-back, of the eos positions; what is stored stays on the device."""
        is_eos = inp_tokens.eq(self.eos_index)
        for index in torch.nonzero(is_eos, as_tuple=True)[0].tolist():
            batch_id = index // self.beam_size
            if len(hyps_and_scores[batch_id]) == self.beam_size:
                continue
            final_scores = scores[index] + self.length_rewarding * (timesteps + 1)
            hyps_and_scores[batch_id].append((alived_seq[index, :], alived_log_probs[index, :], final_scores))
        return is_eos

    def _get_top_score_prediction(self, hyps_and_scores, topk):
        """seq2seq.py:598-648 → (topk_hyps (batch, topk, L), topk_scores,
        topk_lengths, topk_log_probs)."""
        top_hyps, top_log_probs, top_scores, top_lengths = [], [], [], []
        batch_size = len(hyps_and_scores)
        for i in range(len(hyps_and_scores)):
            hyps, log_probs, scores = zip(*hyps_and_scores[i])
            top_hyps += hyps
            top_scores += scores
            top_log_probs += log_probs
            top_lengths += [len(hyp) for hyp in hyps]
        top_hyps = torch.nn.utils.rnn.pad_sequence(top_hyps, batch_first=True, padding_value=0)
        top_scores = torch.stack(top_scores, dim=0).view(batch_size, -1)
        top_lengths = torch.tensor(top_lengths, dtype=torch.int, device=top_scores.device)
        topk_scores, indices = top_scores.topk(self.topk, dim=-1)
        indices = (indices + self.beam_offset.unsqueeze(1)).view(batch_size * self.topk)
        topk_hyps = torch.index_select(top_hyps, dim=0, index=indices).view(batch_size, self.topk, -1)
        topk_lengths = torch.index_select(top_lengths, dim=0, index=indices).view(batch_size, self.topk)
        topk_log_probs = [top_log_probs[i] for i in indices.tolist()]
        return topk_hyps, topk_scores, topk_lengths, topk_log_probs

    @torch.no_grad()
    def forward(self, enc_states, wav_len):  # noqa: C901
        """Beam search (seq2seq.py:650-920) → (predictions, topk_scores[, log_probs])."""
        enc_lens = torch.round(enc_states.shape[1] * wav_len).int()
        device = enc_states.device
        batch_size = enc_states.shape[0]

        memory = self.reset_mem(batch_size * self.beam_size, device=device)
        if self.lm_weight > 0:
            lm_memory = self.reset_lm_mem(batch_size * self.beam_size, device)
        if self.ctc_weight > 0:
            ctc_outputs = self.ctc_forward_step(enc_states)
            ctc_scorer = CTCPrefixScorer(ctc_outputs, enc_lens, batch_size, self.beam_size, self.blank_index,
                                         self.eos_index, self.ctc_window_size)
            ctc_memory = None

        enc_states = inflate_tensor(enc_states, times=self.beam_size, dim=0)
        enc_lens = inflate_tensor(enc_lens, times=self.beam_size, dim=0)
        inp_tokens = torch.full((batch_size * self.beam_size,), self.bos_index, device=device, dtype=torch.long)
        self.beam_offset = torch.arange(batch_size, device=device) * self.beam_size

        # only the first beam of each utterance is alive at the start
        sequence_scores = torch.full((batch_size * self.beam_size,), float("-inf"), device=device)
        sequence_scores.index_fill_(0, self.beam_offset, 0.0)
        scores = sequence_scores

        hyps_and_scores = [[] for _ in range(batch_size)]
        alived_seq = torch.empty(batch_size * self.beam_size, 0, device=device).long()
        alived_log_probs = torch.empty(batch_size * self.beam_size, 0, device=device)

        min_decode_steps = int(enc_states.shape[1] * self.min_decode_ratio)
        max_decode_steps = int(enc_states.shape[1] * self.max_decode_ratio)
        batch_index = torch.arange(batch_size, device=device).unsqueeze(1)

        for t in range(max_decode_steps):
            if self._check_full_beams(hyps_and_scores, self.beam_size):
                break

            log_probs, memory, attn = self.forward_step(inp_tokens, memory, enc_states, enc_lens)
            log_probs = self.att_weight * log_probs
            log_probs_clone = log_probs.clone().reshape(batch_size, -1)
            vocab_size = log_probs.shape[-1]

            if t < min_decode_steps:
                log_probs[:, self.eos_index] = self.minus_inf
            if self.using_eos_threshold:
                cond = self._check_eos_threshold(log_probs)
                log_probs[:, self.eos_index] = mask_by_condition(log_probs[:, self.eos_index], cond,
                                                                 fill_value=self.minus_inf)
            if self.lm_weight > 0:
                lm_log_probs, lm_memory = self.lm_forward_step(inp_tokens, lm_memory)
                log_probs = self._add_lm_scores(log_probs, lm_log_probs)
            if self.ctc_weight > 0:
                g = alived_seq
                log_probs[:, self.blank_index] = self.minus_inf
                if self.ctc_weight != 1.0 and self.ctc_score_mode == "partial":
                    _, ctc_candidates = log_probs.topk(self.beam_size * 2, dim=-1)
                else:
                    ctc_candidates = None
                ctc_log_probs, ctc_memory = ctc_scorer.forward_step(g, ctc_memory, ctc_candidates, attn)
                log_probs = log_probs + self.ctc_weight * ctc_log_probs

            scores = sequence_scores.unsqueeze(1).expand(-1, vocab_size)
            scores = scores + log_probs
            if self.length_normalization:
                scores = scores / (t + 1)

            scores, candidates = scores.view(batch_size, -1).topk(self.beam_size, dim=-1)
            inp_tokens = (candidates % vocab_size).view(batch_size * self.beam_size)
            scores = scores.view(batch_size * self.beam_size)
            # without length normalisation sequence_scores IS scores, as in the
            # reference: the eos rows blocked below are blocked in both
            sequence_scores = scores
            if self.length_normalization:
                sequence_scores = sequence_scores * (t + 1)

            predecessors = (torch.div(candidates, vocab_size, rounding_mode="floor")
                            + self.beam_offset.unsqueeze(1).expand_as(candidates)).view(batch_size * self.beam_size)
            memory = self.permute_mem(memory, index=predecessors)
            if self.lm_weight > 0:
                lm_memory = self.permute_lm_mem(lm_memory, index=predecessors)
            if self.ctc_weight > 0:
                ctc_memory = ctc_scorer.permute_mem(ctc_memory, candidates)

            alived_seq = torch.cat([torch.index_select(alived_seq, dim=0, index=predecessors),
                                    inp_tokens.unsqueeze(1)], dim=-1)
            beam_log_probs = log_probs_clone[batch_index, candidates].reshape(batch_size * self.beam_size)
            alived_log_probs = torch.cat([torch.index_select(alived_log_probs, dim=0, index=predecessors),
                                          beam_log_probs.unsqueeze(1)], dim=-1)

            is_eos = self._update_hyp_and_scores(inp_tokens, alived_seq, alived_log_probs, hyps_and_scores, scores,
                                                 timesteps=t)
            sequence_scores.masked_fill_(is_eos, float("-inf"))

        if not self._check_full_beams(hyps_and_scores, self.beam_size):
            # fill up with the alive rows, as if each ended in eos now
            eos = torch.full((batch_size * self.beam_size,), self.eos_index, device=device, dtype=torch.long)
            self._update_hyp_and_scores(eos, alived_seq, alived_log_probs, hyps_and_scores, scores,
                                        timesteps=max_decode_steps)

        topk_hyps, topk_scores, topk_lengths, log_probs = self._get_top_score_prediction(hyps_and_scores,
                                                                                         topk=self.topk)
        predictions = batch_filter_seq2seq_output(topk_hyps[:, 0, :], eos_id=self.eos_index)
        if self.return_log_probs:
            return predictions, topk_scores, log_probs
        return predictions, topk_scores

    def _add_lm_scores(self, log_probs, lm_log_probs):
        """LM fusion (seq2seq.py:756-760): what lm_forward_step returned, weighted, onto the step's scores."""
        return log_probs + self.lm_weight * lm_log_probs

    def ctc_forward_step(self, x):
        logits = self.ctc_fc(x)
        return self.softmax(logits)

    def permute_mem(self, memory, index):
        raise NotImplementedError

    def permute_lm_mem(self, memory, index):
        raise NotImplementedError


def inflate_tensor(tensor, times, dim):
    """Repeat every slice along dim `times` times, neighbours together."""
    return torch.repeat_interleave(tensor, times, dim=dim)


def mask_by_condition(tensor, cond, fill_value):
    """tensor where cond, else fill_value."""
    return torch.where(cond, tensor, torch.full((), fill_value, dtype=tensor.dtype, device=tensor.device))


def _update_mem(inp_tokens, memory):
    """Append the last step's tokens to the decoded prefixes."""
    if memory is None:
        return inp_tokens.unsqueeze(1)
    return torch.cat([memory, inp_tokens.unsqueeze(1)], dim=-1)


class S2STransformerBeamSearch(S2SBeamSearcher):
    """seq2seq.py:1334-1398.  modules = [TransformerASR, seq_lin, ctc_lin]."""

    # incremental decoding through TransformerASR.decode_step; the constructor
    # is the reference's, so this is an attribute (as Conformer.USE_CONV_CHAIN)
    USE_KV_CACHE = False
    # the same for LM fusion: lm_modules a TransformerLM that takes decode_step
    USE_LM_KV_CACHE = False

    def __init__(self, modules, temperature=1.0, temperature_lm=1.0, **kwargs):
        super().__init__(**kwargs)
        self.model = modules[0]
        self.fc = modules[1]
        self.ctc_fc = modules[2]
        self.softmax = torch.nn.LogSoftmax(dim=-1)
        self.temperature = temperature
        self.temperature_lm = temperature_lm

    def reset_mem(self, batch_size, device):
        return None

    def reset_lm_mem(self, batch_size, device):
        return None

    def _kv_cache(self):
        return self.USE_KV_CACHE and self.model.decode_step_supported()

    def permute_mem(self, memory, index):
        if self._kv_cache():
            return memory.permute(index)
        return torch.index_select(memory, dim=0, index=index)

    def _lm_kv_cache(self):
        return (self.USE_LM_KV_CACHE and isinstance(self.lm_modules, TransformerLM)
                and self.lm_modules.decode_step_supported())

    def permute_lm_mem(self, memory, index):
        if self._lm_kv_cache():
            return memory.permute(index)
        return torch.index_select(memory, dim=0, index=index)

    def forward_step(self, inp_tokens, memory, enc_states, enc_lens):
        if self._kv_cache():
            # memory is the decode state: enc_states arrives inflated, every
            # beam_size-th row is one utterance
            if memory is None:
                memory = self.model.init_decode_state(enc_states[::self.beam_size], group=self.beam_size)
            pred, attn = self.model.decode_step(inp_tokens, memory)
            prob_dist = self.softmax(self.fc(pred) / self.temperature)
            return prob_dist[:, -1, :], memory, attn
        memory = _update_mem(inp_tokens, memory)
        pred, attn = self.model.decode(memory, enc_states)
        prob_dist = self.softmax(self.fc(pred) / self.temperature)
        return prob_dist[:, -1, :], memory, attn

    def lm_forward_step(self, inp_tokens, memory):
        if self._lm_kv_cache():
            # memory is the LM's decode state; what is returned are the raw
            # logits of the newest position: _add_lm_scores takes them
            if not next(self.lm_modules.parameters()).is_cuda:
                self.lm_modules.to(inp_tokens.device)
            if memory is None:
                memory = self.lm_modules.init_decode_state(inp_tokens.shape[0])
            return self.lm_modules.decode_step(inp_tokens, memory), memory
        memory = _update_mem(inp_tokens, memory)
        if not next(self.lm_modules.parameters()).is_cuda:
            self.lm_modules.to(inp_tokens.device)
        logits = self.lm_modules(memory)
        log_probs = self.softmax(logits / self.temperature_lm)
        return log_probs[:, -1, :], memory

    def _add_lm_scores(self, log_probs, lm_log_probs):
        if self._lm_kv_cache():
            # lm_log_probs are the logits: temperature, log-softmax, weight and add in one kernel
            return _kvdec.log_softmax_fuse(lm_log_probs, log_probs, 1.0 / self.temperature_lm, self.lm_weight)
        return super()._add_lm_scores(log_probs, lm_log_probs)


def batch_filter_seq2seq_output(prediction, eos_id=-1):
    """filter_seq2seq_output over a batch of token tensors (a 2-D tensor is
    read back in one copy)."""
    rows = prediction.tolist() if isinstance(prediction, torch.Tensor) else [p.tolist() for p in prediction]
    return [filter_seq2seq_output(p, eos_id=eos_id) for p in rows]


def filter_seq2seq_output(string_pred, eos_id=-1):
    """The tokens before the first eos (seq2seq.py:1547-1579)."""
    if isinstance(string_pred, list):
        try:
            eos_index = next(i for i, v in enumerate(string_pred) if v == eos_id)
        except StopIteration:
            eos_index = len(string_pred)
        string_out = string_pred[:eos_index]
    else:
        raise ValueError("The input must be a list.")
    return string_out
