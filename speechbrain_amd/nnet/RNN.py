"""Drop-in for speechbrain.nnet.RNN.GRU (RNN.py:280-388) on HIP: the
transducer recipes' prediction network `dec`.

Same constructor, forward(x, hx=None, lengths=None) -> (output, hn) and
state_dict keys (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0,
rnn.bias_hh_l0, ..., torch's gate order r, z, n) as the reference, so its
checkpoints load unchanged; `self.rnn` is a torch.nn.GRU used as the parameter
container only (torch's init, then the reference's rnn_init), never called.

What runs (csrc/gru.hip): the input projection of every layer is one MFMA GEMM
over all time steps — or, for layer 0 fed by speechbrain_amd's one-hot
Embedding, no GEMM at all: the step kernel gathers rows of a cached W_ih^T by
token id.  The recurrence is one launch per time step with the gate math
fused; the backward is one launch per step too, followed by the weight /
input-gradient GEMMs of _autograd.  fp32 by default, bf16 operands (fp32
state) under torch.autocast(bf16).

`lengths` are relative, as in the reference's pack_padded_sequence /
pad_packed_sequence pair: row b runs int(lengths[b] * T) steps, its later
outputs are zero, hn is its last valid state and the output is cut to the
longest row.  Implemented as a per-row step mask inside the kernels.

Unidirectional only (`bidirectional=True` raises NotImplementedError); device
tensors only (SbkError, no fallback).
"""
import torch

from .. import _autograd as A
from .. import _enc
from .._lib import check, lib, ptr, require_device, stream_of
from .embedding import segsum_rows

_f32 = torch.float32
_bf16 = torch.bfloat16


def rnn_init(module):
    """RNN.py:1592-1610: orthogonal recurrent weights."""
    for name, param in module.named_parameters():
        if "weight_hh" in name or ".u.weight" in name:
            torch.nn.init.orthogonal_(param)


def _rows_of_tokens(tok, blank, I):
    """Row of W_ih^T each token reads (I for the blank: no row)."""
    t = tok.to(torch.int64)
    return torch.where(t == blank, torch.full_like(t, I), torch.where(t < blank, t, t - 1))


class _GRULayerFn(torch.autograd.Function):
    """One GRU layer over a sequence.  x (B, T, I) or None with tok (B, T)
    int32 one-hot token ids; hx (B, H) or None; lens (B,) int32 or None."""

    @staticmethod
    def forward(ctx, x, tok, blank, w_ih, w_hh, b_ih, b_hh, hx, lens, dtype, cache, key):
        H3, I = w_ih.shape
        H = H3 // 3
        dev = w_hh.device
        bf = int(dtype == _bf16)
        need = any(ctx.needs_input_grad)
        whh = A.kernel_weight(w_hh, dtype, cache, key + "hh")
        bih = None if b_ih is None else b_ih.detach()
        bhh = None if b_hh is None else b_hh.detach()
        hx0 = None if hx is None else hx.detach().float().contiguous()
        a = wk = gi = table = xs = None
        if tok is not None:
            B, T = tok.shape
            # W_ih^T (I, 3H) fp32, holding the compute dtype's values
            table = cache.get(key + "tab" + str(bf), [w_ih], lambda: (
                w_ih.detach().to(dtype).float().t().contiguous()))
        else:
            B, T = x.shape[:2]
            vec = 8 if bf else 4
            Kp = -(-I // vec) * vec
            # kernel copy of W_ih, K zero-padded to the GEMM's 16-byte vectors
            wk = cache.get(key + "ih" + str(bf), [w_ih], lambda: _enc.to_compute(
                torch.nn.functional.pad(w_ih.detach(), (0, Kp - I)), dtype))
            xs = x.detach().reshape(B * T, I)
            a = _enc.to_compute(xs, dtype)
            if Kp != I:
                a = torch.nn.functional.pad(a, (0, Kp - I))
            gi = _enc.gemm(a, wk, bias=bih)
        state = torch.empty(B, T, H, device=dev, dtype=_f32)
        y = state if lens is None else torch.empty(B, T, H, device=dev, dtype=_f32)
        save = torch.empty(B, T, 4, H, device=dev, dtype=_f32) if need else None
        check(lib().sbk_gru_fwd(bf, ptr(whh), ptr(bhh), ptr(hx0), ptr(gi), ptr(tok), int(blank), ptr(table), I,
                                ptr(bih) if tok is not None else None, ptr(lens), B, T, H, ptr(state),
                                ptr(y) if lens is not None else None, ptr(save), stream_of(state)), "sbk_gru_fwd")
        hn = state[:, T - 1].clone()
        if need:
            ctx.save_for_backward(state, save, hx0, lens, xs, wk, tok)
            ctx.cfg = (dtype, cache, key, blank, B, T, H, I, w_hh, None if x is None else x.dtype)
            ctx.has = (b_ih is not None, b_hh is not None, hx is not None)
        return y, hn

    @staticmethod
    def backward(ctx, dy, dhn):
        state, save, hx0, lens, xs, wk, tok = ctx.saved_tensors
        dtype, cache, key, blank, B, T, H, I, w_hh, xdt = ctx.cfg
        has_bih, has_bhh, has_hx = ctx.has
        dev = state.device
        bf = int(dtype == _bf16)
        whhT = cache.get(key + "hhT" + str(bf), [w_hh], lambda: _enc.to_compute(w_hh.detach().t(), dtype))
        dy = None if dy is None else dy.detach().float().contiguous()
        dhn = None if dhn is None else dhn.detach().float().contiguous()
        dgi = torch.empty(B, T, 3 * H, device=dev, dtype=_f32)
        dgh = torch.empty(B, T, 3 * H, device=dev, dtype=_f32)
        dhw = torch.empty(2, B, H, device=dev, dtype=_f32)
        dhx = torch.empty(B, H, device=dev, dtype=_f32)
        check(lib().sbk_gru_bwd(bf, ptr(whhT), ptr(hx0), ptr(state), ptr(save), ptr(dy), ptr(dhn), ptr(lens), B, T, H,
                                ptr(dgi), ptr(dgh), ptr(dhw), ptr(dhx), stream_of(state)), "sbk_gru_bwd")
        gi2, gh2 = dgi.view(B * T, 3 * H), dgh.view(B * T, 3 * H)
        first = hx0.unsqueeze(1) if hx0 is not None else torch.zeros(B, 1, H, device=dev, dtype=_f32)
        hprev = torch.cat([first, state[:, :T - 1]], 1).reshape(B * T, H)
        need = ctx.needs_input_grad
        dx = dw_ih = dw_hh = db_ih = db_hh = None
        if need[4]:
            dw_hh = A.wgrad(A._as(gh2, dtype), A._as(hprev, dtype))
        if tok is not None:
            if need[3]:
                # per-token sum of the dgi rows: rows of d(W_ih^T); the blank has none
                dw_ih = segsum_rows(gi2, _rows_of_tokens(tok, blank, I), I).t().contiguous()
        else:
            if need[3]:
                # fp32 operands in both modes: with dgi and x both rounded to bf16 this
                # gradient left the bf16 bound of tests/test_gpu_rnn.py
                dw_ih = A.wgrad(gi2, xs.float())
            if need[0]:
                dx = A.dgrad(A._as(gi2, dtype), wk)[:, :I].reshape(B, T, I).to(xdt)
        if has_bih and need[5]:
            db_ih = A.rowsum(gi2)
        if has_bhh and need[6]:
            db_hh = A.rowsum(gh2)
        return dx, None, None, dw_ih, dw_hh, db_ih, db_hh, (dhx if has_hx and need[7] else None), None, None, None, None


class GRU(torch.nn.Module):
    def __init__(self, hidden_size, input_shape=None, input_size=None, num_layers=1, bias=True, dropout=0.0,
                 re_init=True, bidirectional=False):
        super().__init__()
        self.reshape = False
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size.")
        if bidirectional:
            raise NotImplementedError("speechbrain_amd GRU is unidirectional (the transducer prediction network); "
                                      "bidirectional=True has no kernel")
        if input_size is None:
            if len(input_shape) > 3:
                self.reshape = True
            input_size = torch.prod(torch.tensor(input_shape[2:])).item()
        # parameter container: torch's names and init; its forward is never called
        self.rnn = torch.nn.GRU(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers,
                                dropout=dropout, bidirectional=False, bias=bias, batch_first=True)
        if re_init:
            rnn_init(self.rnn)
        self._wc = _enc.WeightCache()

    @staticmethod
    def _steps(lengths, T):
        """Steps per row, as torch's packing derives them from lengths * T."""
        steps = (lengths * T).cpu().to(torch.int64)
        if steps.dim() != 1 or int(steps.min()) < 1 or int(steps.max()) > T:
            raise ValueError(f"lengths * T must lie in [1, {T}] (got {steps.tolist()})")
        return steps

    def forward(self, x, hx=None, lengths=None):
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        rnn = self.rnn
        require_device(x, hx, rnn.weight_hh_l0)
        if x.ndim != 3 or x.shape[-1] != rnn.input_size:
            raise ValueError(f"GRU expects (batch, time, {rnn.input_size}) (got {tuple(x.shape)})")
        B, T, _ = x.shape
        L, H = rnn.num_layers, rnn.hidden_size
        if hx is not None and tuple(hx.shape) != (L, B, H):
            raise ValueError(f"hx must be {(L, B, H)} (got {tuple(hx.shape)})")
        tag = getattr(x, "_sbk_onehot", None)
        tok = blank = None
        if tag is not None and tag[2] == x._version and tuple(tag[0].shape) == (B, T):
            tok, blank = tag[0], tag[1]   # unmodified one-hot rows: layer 0 never reads x
        lens = None
        if lengths is not None:
            steps = self._steps(lengths, T)
            Tn = int(steps.max())
            if Tn < T:
                x = x[:, :Tn]
                tok = None if tok is None else tok[:, :Tn].contiguous()
                T = Tn
            if int(steps.min()) < T:
                lens = steps.to(device=x.device, dtype=torch.int32)
        dtype = _enc.compute_dtype()
        y, hns = x, []
        for layer in range(L):
            w = [getattr(rnn, f"{n}_l{layer}", None) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            h0 = None if hx is None else hx[layer]
            if layer == 0 and tok is not None:
                y, hn = _GRULayerFn.apply(None, tok, blank, *w, h0, lens, dtype, self._wc, f"l{layer}")
            else:
                y, hn = _GRULayerFn.apply(y, None, 0, *w, h0, lens, dtype, self._wc, f"l{layer}")
            hns.append(hn)
            if layer < L - 1 and rnn.dropout > 0:
                y = A.dropout(y, rnn.dropout, self.training)
        return y, torch.stack(hns, 0)
