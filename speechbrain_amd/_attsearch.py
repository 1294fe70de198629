"""Host side of the beam-grouped decoder step (sbk_attdec_beam_step in
csrc/attdec.hip): the state of an RNN beam search over N = B * beam hypotheses
that share the B utterances' encoder states.  See DESIGN.md §3 "RNN beam
search"."""
import torch

from . import _attdec
from . import _autograd as A
from . import _enc
from ._lib import check, lib, ptr, stream_of

_f32 = torch.float32
_bf16 = torch.bfloat16
_i32 = torch.int32


def group():
    """Hypotheses per workgroup of the beam score kernel."""
    return int(lib().sbk_attdec_beam_group())


def embedding_weight(emb):
    """The (V, I) table of an embedding module the token table can be built from, else None."""
    inner = getattr(emb, "Embedding", emb)
    return inner.weight if isinstance(inner, torch.nn.Embedding) else None


class BeamState:
    """dec: the package's AttentionalRNNDecoder; emb: the embedding module;
    enc_states (B, L, E) and enc_lens (B) NOT inflated.  mlp_enc runs once over
    the B utterances; the per-hypothesis state (h, c, attention, coverage,
    attention peak) lives in two sets of buffers that a step reads through
    `parent` from one and writes into the other."""

    def __init__(self, dec, emb, enc_states, enc_lens, beam_size, max_attn_shift=0):
        self.dec, self.emb = dec, emb
        B, L, E = enc_states.shape
        dev = enc_states.device
        self.B, self.G, self.N, self.L, self.E = B, beam_size, B * beam_size, L, E
        N = self.N
        W = dict(zip(_attdec.NAMES, _attdec.weights_of(dec)))
        self.H, self.A, self.O = W["w_hh"].shape[1], W["w_dec"].shape[0], W["w_out"].shape[0]
        self.enc = enc_states.detach().float().contiguous()
        self.len32 = enc_lens.to(device=dev, dtype=_i32).contiguous()
        self.P = _attdec.precompute(self.enc, W["w_enc"], W["b_enc"], _enc.compute_dtype(), dec._wc)
        self.max_shift = int(min(max(int(max_attn_shift), 0), 1 << 30))
        z = lambda *s: torch.zeros(*s, device=dev, dtype=_f32)  # noqa: E731
        start = (torch.arange(L, device=dev)[None, :] < self.len32[:, None]).float() / self.len32[:, None].float()
        # [h, c, attn, cov, peak] twice: set `cur` holds the last step's rows
        self.bufs = [[z(N, self.H), z(N, self.O), torch.repeat_interleave(start, beam_size, dim=0).contiguous(),
                      z(N, L), torch.zeros(N, device=dev, dtype=_i32)],
                     [z(N, self.H), z(N, self.O), z(N, L), z(N, L), torch.zeros(N, device=dev, dtype=_i32)]]
        self.cur = 0
        self._ident = torch.arange(N, device=dev, dtype=_i32)
        self.parent = self._ident
        self.shift_ok = torch.empty(N, device=dev, dtype=_i32)
        self.pen = z(N)
        self.ctx, self.dech = z(N, E), z(N, self.A)
        nt = -(-L // _attdec.score_tile())
        self.ws = z(N * (L + nt * (2 + E)))
        self.t = 0

    def _table(self, W, dtype, cache):
        """(V, 3H) = emb.weight W_ih[:, :I]^T + b_ih, once per weight version."""
        ew = embedding_weight(self.emb)
        if ew is None:
            return None
        I = W["w_ih"].shape[1] - self.O
        params = [ew, W["w_ih"]] + ([] if W["b_ih"] is None else [W["b_ih"]])
        return cache.get(f"gxtab{int(dtype == _bf16)}", params,
                         lambda: _attdec._gx(ew.detach().float(), W, I, dtype, cache))

    def step(self, tokens):
        """tokens (N) -> (dec_out (N, H), attn (N, L)); the state advances one step."""
        dec = self.dec
        W = dict(zip(_attdec.NAMES, _attdec.weights_of(dec)))
        dtype, cache = _enc.compute_dtype(), dec._wc
        I = W["w_ih"].shape[1] - self.O
        table = self._table(W, dtype, cache)
        if table is None:
            gx, tok, V = _attdec._gx(self.emb(tokens).detach().float(), W, I, dtype, cache), None, 0
        else:
            gx, tok, V = table, tokens.to(_i32).contiguous(), table.shape[0]
        wconv, wloc, C, ksz = _attdec._loc(W.get("w_conv"), W.get("w_loc"))
        b_q = W["b_dec"].detach() if wloc is None else W["b_dec"].detach() + W["b_loc"].detach()
        hp, cp, ap, vp, pp = self.bufs[self.cur]
        h, c, attn, cov, peak = self.bufs[1 - self.cur]
        check(lib().sbk_attdec_beam_step(
            int(dtype == _bf16), ptr(_attdec._part(cache, "ic", W["w_ih"], dtype, slice(I, None))),
            ptr(A.kernel_weight(W["w_hh"], dtype, cache, "hh")), ptr(None if W["b_hh"] is None else W["b_hh"].detach()),
            ptr(A.kernel_weight(W["w_dec"], dtype, cache, "dec")), ptr(b_q),
            ptr(A.kernel_weight(W["w_out"], dtype, cache, "out")), ptr(W["b_out"].detach()), ptr(gx), ptr(tok),
            ptr(self.P), ptr(self.enc), ptr(self.len32), ptr(wconv), ptr(wloc),
            ptr(A._cont(W["w_attn"].detach().float().reshape(-1))), float(dec.scaling), ptr(self.parent), ptr(hp),
            ptr(cp), ptr(ap), ptr(vp), ptr(pp), int(self.t == 0), self.max_shift, V, self.B, self.G, self.L, self.H,
            self.A, self.O, self.E, C, ksz, ptr(h), ptr(c), ptr(attn), ptr(cov), ptr(peak), ptr(self.shift_ok),
            ptr(self.pen), ptr(self.ctx), ptr(self.dech), ptr(self.ws), stream_of(self.enc)), "sbk_attdec_beam_step")
        self.cur = 1 - self.cur
        self.t += 1
        # the rows just written are their own parents until the search permutes them
        self.parent = self._ident
        out, _ = _attdec._project(c.view(self.N, 1, -1), h.view(self.N, 1, -1), W, dtype, cache)
        return out[:, 0], attn

    def permute(self, index):
        """The beam permutation: row n of the next step continues row index[n].  Moves no data."""
        self.parent = index.to(_i32).contiguous()
        return self

    # what the last step left, by row of that step
    @property
    def h(self):
        return self.bufs[self.cur][0]

    @property
    def c(self):
        return self.bufs[self.cur][1]

    @property
    def cov(self):
        return self.bufs[self.cur][3]

    @property
    def peak(self):
        return self.bufs[self.cur][4]
