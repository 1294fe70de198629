"""Drop-ins for speechbrain.decoders.ctc (decoders/ctc.py:13-376) on MI355X:
CTCPrefixScorer, ctc_greedy_decode and filter_ctc_output.

Same constructors, signatures, defaults and return values as the reference.
What runs where:
  * CTCPrefixScorer.forward_step — ONE kernel (sbk_ctc_prefix_step) instead
    of the reference's Python loop over the encoder frames (three or four
    torch ops per frame) and its loops over the batch·beam rows.  One thread
    owns one (row, candidate) pair and walks the frames; the step returns the
    (N, V) scores and keeps no per-candidate state.
  * CTCPrefixScorer.permute_mem — ONE kernel (sbk_ctc_prefix_advance) that
    reruns the walk for the N surviving (parent row, token) pairs and writes
    their state r (T, 2, N) and psi (N).  The reference writes r for every
    candidate, (T, 2, N, C) floats per decoded token, and index_selects N
    columns of it; here the state is O(T·N).
  * ctc_greedy_decode — one kernel (argmax per frame, merge repeats, drop
    blanks, compact) and one device→host copy for the whole batch.
The set-up (padded-frame masking, the blank cumsum of the initial state) is
torch plumbing: it runs once per search.  There is no host read inside a
step, and no CPU fallback.
"""
from itertools import groupby
from typing import Optional

import torch

from .._lib import check, custom_op, lib, ptr, require_device, stream_of


@custom_op("sbk::ctc_prefix_step", mutates_args=())
def ctc_prefix_step(x: torch.Tensor, r_prev: torch.Tensor, psi_prev: Optional[torch.Tensor],
                    last_tok: Optional[torch.Tensor], candidates: Optional[torch.Tensor], last_frame: torch.Tensor,
                    beam: int, prefix_len: int, start: int, end: int, blank: int, eos: int) -> torch.Tensor:
    """x (B, T, V), r_prev (T, 2, N), psi_prev (N) | None, last_tok (N) int64 | None, candidates (N, C)
    int64 | None, last_frame (B) int32 → psi − psi_prev (N, V)."""
    B, T, V = x.shape
    C = 0 if candidates is None else candidates.shape[1]
    out = torch.empty(B * beam, V, device=x.device, dtype=torch.float32)
    check(lib().sbk_ctc_prefix_step(ptr(x), ptr(r_prev), ptr(psi_prev), ptr(last_tok), ptr(candidates),
                                    ptr(last_frame), B, beam, T, V, C, prefix_len, start, end, blank, eos, ptr(out),
                                    stream_of(x)), "sbk_ctc_prefix_step")
    return out


@ctc_prefix_step.register_fake
def _(x, r_prev, psi_prev, last_tok, candidates, last_frame, beam, prefix_len, start, end, blank, eos):
    return x.new_empty(x.shape[0] * beam, x.shape[2])


@custom_op("sbk::ctc_prefix_advance", mutates_args=())
def ctc_prefix_advance(x: torch.Tensor, r_prev: torch.Tensor, last_tok: Optional[torch.Tensor],
                       candidates: Optional[torch.Tensor], last_frame: torch.Tensor, parent: torch.Tensor,
                       token: torch.Tensor, beam: int, prefix_len: int, start: int, end: int, blank: int,
                       eos: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The step's inputs plus parent (N) and token (N) int64 → (r_new (T, 2, N), psi_new (N))."""
    B, T, V = x.shape
    N = B * beam
    C = 0 if candidates is None else candidates.shape[1]
    r_new = torch.empty(T, 2, N, device=x.device, dtype=torch.float32)
    psi_new = torch.empty(N, device=x.device, dtype=torch.float32)
    check(lib().sbk_ctc_prefix_advance(ptr(x), ptr(r_prev), ptr(last_tok), ptr(candidates), ptr(last_frame),
                                       ptr(parent), ptr(token), B, beam, T, V, C, prefix_len, start, end, blank, eos,
                                       ptr(r_new), ptr(psi_new), stream_of(x)), "sbk_ctc_prefix_advance")
    return r_new, psi_new


@ctc_prefix_advance.register_fake
def _(x, r_prev, last_tok, candidates, last_frame, parent, token, beam, prefix_len, start, end, blank, eos):
    N = x.shape[0] * beam
    return x.new_empty(x.shape[1], 2, N), x.new_empty(N)


@custom_op("sbk::ctc_greedy_decode", mutates_args=())
def _greedy_decode(x: torch.Tensor, lens: torch.Tensor, blank: int) -> torch.Tensor:
    """x (B, T, V) fp32 (any strides), lens (B) int32 absolute → int32 (B·T + B): the compacted tokens of
    every utterance, row by row, then the B counts."""
    B, T, V = x.shape
    buf = torch.empty(B * T + B, device=x.device, dtype=torch.int32)
    check(lib().sbk_ctc_greedy_decode(ptr(x), x.stride(0), x.stride(1), x.stride(2), ptr(lens), B, T, V, blank,
                                      ptr(buf), ptr(buf[B * T:]), stream_of(x)), "sbk_ctc_greedy_decode")
    return buf


@_greedy_decode.register_fake
def _(x, lens, blank):
    return x.new_empty(x.shape[0] * x.shape[1] + x.shape[0], dtype=torch.int32)


def _i64(t):
    return t if t.dtype == torch.int64 and t.is_contiguous() else t.long().contiguous()


class CTCPrefixScorer:
    """ctc.py:13-294.  x (batch, T, V) CTC log-probs (masked in place past
    enc_lens, as the reference does), enc_lens (batch) absolute lengths."""

    def __init__(self, x, enc_lens, batch_size, beam_size, blank_index, eos_index, ctc_window_size=0):
        require_device(x)
        self.blank_index = blank_index
        self.eos_index = eos_index
        self.max_enc_len = x.size(1)
        self.batch_size = batch_size
        self.beam_size = beam_size
        self.vocab_size = x.size(-1)
        self.device = x.device
        self.minus_inf = -1e20
        enc_lens = enc_lens.to(self.device)
        self.last_frame_index = enc_lens - 1
        self.ctc_window_size = ctc_window_size

        # frames >= enc_lens: every column the sentinel, then column 0 (not
        # blank_index: the reference's own choice, ctc.py:62) zero
        mask = torch.arange(self.max_enc_len, device=self.device)[None, :] >= enc_lens[:, None]
        x.masked_fill_(mask.unsqueeze(-1), self.minus_inf)
        x[:, :, 0].masked_fill_(mask, 0)
        x = x.detach()
        self.x = x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()
        self._last_frame = self.last_frame_index.to(torch.int32).contiguous()

        self.beam_offset = torch.arange(batch_size, device=self.device) * self.beam_size

    def _initial_state(self):
        """r_prev (T, 2, N): non-blank the sentinel, blank the running sum of
        the blank log-probs (ctc.py:104-117)."""
        N = self.batch_size * self.beam_size
        r_prev = torch.full((self.max_enc_len, 2, N), self.minus_inf, device=self.device, dtype=torch.float32)
        blank_sum = torch.cumsum(self.x[:, :, self.blank_index].transpose(0, 1), 0)        # (T, batch)
        r_prev[:, 1] = blank_sum.repeat_interleave(self.beam_size, dim=1)
        return r_prev, None

    def forward_step(self, g, state, candidates=None, attn=None):
        """g (N, prefix length) the prefixes, state the (r, psi) of permute_mem
        or None, candidates (N, C) for partial scoring → (psi − psi_prev
        (N, V), memory).  memory is opaque: it is what permute_mem needs."""
        if self.ctc_window_size != 0 and attn is not None:
            raise NotImplementedError(
                "CTCPrefixScorer: ctc_window_size > 0 with an attention map (the attention-peak window) is an "
                "RNN-searcher feature and has no kernel here; the transformer recipes leave it 0")
        prefix_length = g.size(1)
        self.num_candidates = self.vocab_size if candidates is None else candidates.size(-1)
        if state is None:
            r_prev, psi_prev = self._initial_state()
        else:
            r_prev, psi_prev = state
            r_prev = r_prev.contiguous()
            if psi_prev.dim() == 2:      # permute_mem's (N, V): one value per row
                psi_prev = psi_prev[:, 0]
            psi_prev = psi_prev.float().contiguous()
        last_tok = _i64(g[:, -1]) if prefix_length > 0 else None
        if candidates is not None:
            candidates = _i64(candidates)
        start = max(1, prefix_length)
        end = self.max_enc_len
        out = ctc_prefix_step(self.x, r_prev, psi_prev, last_tok, candidates, self._last_frame, self.beam_size,
                              prefix_length, start, end, self.blank_index, self.eos_index)
        return out, (r_prev, last_tok, candidates, prefix_length, start, end)

    def permute_mem(self, memory, index):
        """index (batch, beam): the kept entries of the flattened (beam·V)
        scores of each utterance → (r (T, 2, N), psi (N, V)) of the new rows."""
        r_prev, last_tok, candidates, prefix_length, start, end = memory
        parent = (torch.div(index, self.vocab_size, rounding_mode="floor")
                  + self.beam_offset.unsqueeze(1)).reshape(-1)
        token = (index % self.vocab_size).reshape(-1)
        r, psi = ctc_prefix_advance(self.x, r_prev, last_tok, candidates, self._last_frame, _i64(parent),
                                    _i64(token), self.beam_size, prefix_length, start, end, self.blank_index,
                                    self.eos_index)
        return r, psi.unsqueeze(1).expand(-1, self.vocab_size)


def filter_ctc_output(string_pred, blank_id=-1):
    """Merge repeats, then drop blanks (ctc.py:297-331)."""
    if isinstance(string_pred, list):
        string_out = [i[0] for i in groupby(string_pred)]
        string_out = list(filter(lambda elem: elem != blank_id, string_out))
    else:
        raise ValueError("filter_ctc_out can only filter python lists")
    return string_out


def ctc_greedy_decode(probabilities, seq_lens, blank_id=-1):
    """Greedy CTC decode of (batch, time, classes) probabilities or
    log-probabilities with relative seq_lens → list of lists (ctc.py:334-376).
    A negative blank_id counts down from the last class."""
    require_device(probabilities)
    if isinstance(blank_id, int) and blank_id < 0:
        blank_id = probabilities.shape[-1] + blank_id
    B, T, _ = probabilities.shape
    x = probabilities.detach()
    if x.dtype != torch.float32:
        x = x.float()
    seq_lens = torch.as_tensor(seq_lens)
    lens = torch.round(seq_lens * T).to(device=x.device, dtype=torch.int32).contiguous()
    buf = _greedy_decode(x, lens, int(blank_id)).cpu().numpy()
    counts = buf[B * T:]
    return [buf[b * T: b * T + counts[b]].tolist() for b in range(B)]
