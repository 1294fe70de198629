"""Drop-ins for speechbrain.nnet.RNN.GRU (RNN.py:280-388), the transducer
recipes' prediction network `dec`, and LSTM (RNN.py:169-277) on HIP.

Same constructor, forward(x, hx=None, lengths=None) -> (output, hn) — (hn, cn)
for the LSTM, whose hx is a tuple (h0, c0) — and state_dict keys
(rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, ..., the
LSTM's second direction with `_reverse` suffixes; torch's gate order r, z, n /
i, f, g, o) as the reference, so its checkpoints load unchanged; `self.rnn` is
a torch.nn.GRU / torch.nn.LSTM used as the parameter container only (torch's
init, then the reference's rnn_init), never called.

What runs (csrc/gru.hip, csrc/lstm.hip on the skeleton of csrc/rnnstep.h):
the input projection of every layer is one MFMA GEMM over all time steps, for
both directions of an LSTM at once — or, for layer 0 fed by speechbrain_amd's
one-hot Embedding, no GEMM at all: the step kernel gathers rows of a cached
W_ih^T by token id.  The recurrence is one launch per time step with the gate
math fused, both directions of an LSTM in the same launch (layers >= 1 read
the 2H-wide output); the backward is one launch per step too, followed by the
weight / input-gradient GEMMs of _autograd.  fp32 by default, bf16 operands
(fp32 state) under torch.autocast(bf16).

`lengths` are relative, as in the reference's pack_padded_sequence /
pad_packed_sequence pair: row b runs int(lengths[b] * T) steps, its later
outputs are zero, hn is its last valid state and the output is cut to the
longest row.  Implemented as a per-row step mask inside the kernels, mirrored
for the LSTM's reverse direction.

The GRU is unidirectional only (`bidirectional=True` raises
NotImplementedError); device tensors only (SbkError, no fallback).

LiGRU and LiGRU_Layer (RNN.py:961-1325; csrc/ligru.hip) are drop-ins for the
reference's own two-gate cell: same constructors, forward(x, hx=None) ->
(output, h) and state_dict (rnn.{i}.w.weight, rnn.{i}.u.weight, rnn.{i}.norm.*,
rnn.{i}.h_init, rnn.{i}.drop_masks, rnn.{i}.drop_mask_te), seeded
construction included.  Per layer one input GEMM serves both directions (the
reference's cat([x, x.flip(1)]) makes the reverse half's pre-activations the
flip of the forward half's), the batch / layer normalisation is applied in
the step kernel's epilogue from per-row and per-column terms, and one launch
per time step runs both directions on the shared u, forward and backward.  The
recurrent-dropout pool, its counter and its resampling rules are the
reference's, in host torch.  The CRDNN lobe that wraps this cell is not
provided: it needs pooling, BatchNorm and container drop-ins.
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


def _steps(lengths, T):
    """Steps per row, as torch's packing derives them from lengths * T."""
    steps = (lengths * T).cpu().to(torch.int64)
    if steps.dim() != 1 or int(steps.min()) < 1 or int(steps.max()) > T:
        raise ValueError(f"lengths * T must lie in [1, {T}] (got {steps.tolist()})")
    return steps


def _input_preact(x, tok, w_ih, bih, dtype, cache, key):
    """Input pre-activations of a layer for the stacked w_ih (each (G * H, I)):
    the dense gi = x W_ih^T + bih of x (B, T, I), or, for one-hot token ids tok
    (B, T), the table W_ih^T the step kernel gathers from.  Returns (gi, table,
    xs, wk, B, T); xs (B * T, I) and the kernel copy wk serve the backward."""
    bf = int(dtype == _bf16)
    I = w_ih[0].shape[1]
    gi = table = xs = wk = None
    if tok is not None:
        B, T = tok.shape
        # the stacked W_ih transposed (I, D * G * H) fp32, holding the compute dtype's values
        table = cache.get(key + "tab" + str(bf), w_ih, lambda: (
            torch.cat([w.detach() for w in w_ih]).to(dtype).float().t().contiguous()))
    else:
        B, T = x.shape[:2]
        vec = 8 if bf else 4
        Kp = -(-I // vec) * vec
        # K zero-padded to the GEMM's 16-byte vectors: one GEMM gives every direction's gi
        wk = cache.get(key + "ih" + str(bf), w_ih, lambda: _enc.to_compute(
            torch.nn.functional.pad(torch.cat([w.detach() for w in w_ih]), (0, Kp - I)), dtype))
        xs = x.detach().reshape(B * T, I)
        a = _enc.to_compute(xs, dtype)
        if Kp != I:
            a = torch.nn.functional.pad(a, (0, Kp - I))
        gi = _enc.gemm(a, wk, bias=bih)
    return gi, table, xs, wk, B, T


def _input_grads(g2, tok, blank, I, xs, wk, dtype, xdt, B, T, want_w, want_x):
    """(dW_ih stacked, dx) from g2 (B * T, D * G * H), the gradient of gi."""
    dw_ih = dx = None
    if tok is not None:
        if want_w:
            # per-token sum of the rows of g2: rows of d(W_ih^T); the blank has none
            dw_ih = segsum_rows(g2, _rows_of_tokens(tok, blank, I), I).t().contiguous()
    else:
        if want_w:
            # fp32 operands in both modes: with g2 and x both rounded to bf16 this
            # gradient left the bf16 bound of tests/test_gpu_rnn.py
            dw_ih = A.wgrad(g2, xs.float())
        if want_x:
            dx = A.dgrad(A._as(g2, dtype), wk)[:, :I].reshape(B, T, I).to(xdt)
    return dw_ih, dx


def _hprev(state, h0, reverse=False):
    """(B * T, H): the h every step of one direction started from; state
    (B, T, H) carried, h0 (B, H) or None.  The reverse scan's carried padding
    makes [state[:, 1:], h0] right for ragged rows."""
    B, T, H = state.shape
    first = h0.unsqueeze(1) if h0 is not None else torch.zeros(B, 1, H, device=state.device, dtype=_f32)
    return torch.cat([state[:, 1:], first] if reverse else [first, state[:, :T - 1]], 1).reshape(B * T, H)


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
        gi, table, xs, wk, B, T = _input_preact(x, tok, [w_ih], bih, dtype, cache, key)
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
        need = ctx.needs_input_grad
        dw_hh = db_ih = db_hh = None
        if need[4]:
            dw_hh = A.wgrad(A._as(gh2, dtype), A._as(_hprev(state, hx0), dtype))
        dw_ih, dx = _input_grads(gi2, tok, blank, I, xs, wk, dtype, xdt, B, T, need[3], need[0])
        if has_bih and need[5]:
            db_ih = A.rowsum(gi2)
        if has_bhh and need[6]:
            db_hh = A.rowsum(gh2)
        return dx, None, None, dw_ih, dw_hh, db_ih, db_hh, (dhx if has_hx and need[7] else None), None, None, None, None


class _LSTMLayerFn(torch.autograd.Function):
    """One LSTM layer over a sequence, D = 1 or 2 directions in the same
    launches.  x (B, T, I) or None with tok (B, T) int32 one-hot token ids;
    h0, c0 (D, B, H) or None; lens (B,) int32 or None; weights: per direction
    w_ih (4H, I), w_hh (4H, H), b_ih, b_hh (4H) or None.  Returns the output
    (B, T, D * H) and hn, cn (D, B, H)."""

    @staticmethod
    def forward(ctx, x, tok, blank, h0, c0, lens, dtype, cache, key, D, *weights):
        w_ih, w_hh = list(weights[0::4]), list(weights[1::4])
        b_ih, b_hh = list(weights[2::4]), list(weights[3::4])
        H4, I = w_ih[0].shape
        H = H4 // 4
        dev = w_hh[0].device
        bf = int(dtype == _bf16)
        need = any(ctx.needs_input_grad)
        # kernel copies, the directions stacked: W_hh (D, 4H, H), W_ih (D * 4H, I), biases (D * 4H)
        whh = cache.get(key + "hh" + str(bf), w_hh, lambda: _enc.to_compute(
            torch.stack([w.detach() for w in w_hh]), dtype))
        bih = None if b_ih[0] is None else torch.cat([b.detach() for b in b_ih])
        bhh = None if b_hh[0] is None else torch.cat([b.detach() for b in b_hh])
        hx0 = None if h0 is None else h0.detach().float().contiguous()
        cx0 = None if c0 is None else c0.detach().float().contiguous()
        gi, table, xs, wk, B, T = _input_preact(x, tok, w_ih, bih, dtype, cache, key)
        hstate = torch.empty(B, T, D * H, device=dev, dtype=_f32)
        cstate = torch.empty(B, T, D * H, device=dev, dtype=_f32)
        y = hstate if lens is None else torch.empty(B, T, D * H, device=dev, dtype=_f32)
        save = torch.empty(B, T, D, 4 * H, device=dev, dtype=_f32) if need else None
        check(lib().sbk_lstm_fwd(bf, D, ptr(whh), ptr(bhh), ptr(hx0), ptr(cx0), ptr(gi), ptr(tok), int(blank),
                                 ptr(table), I, ptr(bih) if tok is not None else None, ptr(lens), B, T, H,
                                 ptr(hstate), ptr(cstate), ptr(y) if lens is not None else None, ptr(save),
                                 stream_of(hstate)), "sbk_lstm_fwd")
        # the carried state makes the last step of either scan the final state of every row
        ends = [(T - 1, 0)] if D == 1 else [(T - 1, 0), (0, H)]
        hn = torch.stack([hstate[:, t, o:o + H] for t, o in ends])
        cn = torch.stack([cstate[:, t, o:o + H] for t, o in ends])
        if need:
            ctx.save_for_backward(hstate, cstate, save, hx0, cx0, lens, xs, wk, tok)
            ctx.cfg = (dtype, cache, key, blank, B, T, H, I, D, w_hh, None if x is None else x.dtype)
            ctx.has = (b_ih[0] is not None, b_hh[0] is not None, h0 is not None, c0 is not None)
        return y, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn, dcn):
        hstate, cstate, save, hx0, cx0, lens, xs, wk, tok = ctx.saved_tensors
        dtype, cache, key, blank, B, T, H, I, D, w_hh, xdt = ctx.cfg
        has_bih, has_bhh, has_h0, has_c0 = ctx.has
        dev = hstate.device
        bf = int(dtype == _bf16)
        whhT = cache.get(key + "hhT" + str(bf), w_hh, lambda: _enc.to_compute(
            torch.stack([w.detach().t() for w in w_hh]), dtype))
        dy = None if dy is None else dy.detach().float().contiguous()
        dhn = None if dhn is None else dhn.detach().float().contiguous()
        dcn = None if dcn is None else dcn.detach().float().contiguous()
        dG = torch.empty(B, T, D, 4 * H, device=dev, dtype=_f32)
        dw = torch.empty(2, 2, D, B, H, device=dev, dtype=_f32)
        dhx = torch.empty(D, B, H, device=dev, dtype=_f32)
        dcx = torch.empty(D, B, H, device=dev, dtype=_f32)
        check(lib().sbk_lstm_bwd(bf, D, ptr(whhT), ptr(cx0), ptr(cstate), ptr(save), ptr(dy), ptr(dhn), ptr(dcn),
                                 ptr(lens), B, T, H, ptr(dG), ptr(dw), ptr(dhx), ptr(dcx), stream_of(hstate)),
              "sbk_lstm_bwd")
        g2 = dG.view(B * T, D * 4 * H)
        need = ctx.needs_input_grad
        nw = 10                      # position of the first weight among forward's inputs
        grads = [None] * (4 * D)
        for d in range(D):
            if need[nw + 4 * d + 1]:
                hprev = _hprev(hstate[:, :, d * H:(d + 1) * H], None if hx0 is None else hx0[d], reverse=d == 1)
                gd = dG[:, :, d].reshape(B * T, 4 * H)
                grads[4 * d + 1] = A.wgrad(A._as(gd, dtype), A._as(hprev, dtype))
        want_ih = any(need[nw + 4 * d] for d in range(D))
        dw_ih, dx = _input_grads(g2, tok, blank, I, xs, wk, dtype, xdt, B, T, want_ih, need[0])
        if want_ih:
            for d in range(D):
                grads[4 * d] = dw_ih[d * 4 * H:(d + 1) * 4 * H]
        if has_bih or has_bhh:
            db = A.rowsum(g2)        # dgi and dgh are the same rows: one sum serves b_ih and b_hh
            for d in range(D):
                if has_bih and need[nw + 4 * d + 2]:
                    grads[4 * d + 2] = db[d * 4 * H:(d + 1) * 4 * H]
                if has_bhh and need[nw + 4 * d + 3]:
                    grads[4 * d + 3] = db[d * 4 * H:(d + 1) * 4 * H].clone()
        return (dx, None, None, dhx if has_h0 and need[3] else None, dcx if has_c0 and need[4] else None,
                None, None, None, None, None, *grads)


_LIGRU_ACT = {"relu": 0, "leaky_relu": 1, "tanh": 2, "sin": 3}


class _LiGRULayerFn(torch.autograd.Function):
    """One LiGRU layer over a sequence, D = 1 or 2 directions in the same
    launches and on the same weights.  x (B, T, I); w (2H, I), u (2H, H);
    gamma, beta (2H); hx, mask (D * B, H) or None (the rows of direction 1
    after those of direction 0).  kind: "layer" (LayerNorm over the 2H
    pre-activations of a row), "batch_train" (BatchNorm with the statistics of
    this call) or "batch_eval" (with rmean, rvar).  Returns the output
    (B, T, D * H) and the column mean and biased variance of the input
    projection ("batch_train"; else empty)."""

    @staticmethod
    def forward(ctx, x, w, u, gamma, beta, hx, mask, rmean, rvar, kind, eps, act, D, dtype, cache, key):
        H2, I = w.shape
        H = H2 // 2
        dev = u.device
        bf = int(dtype == _bf16)
        need = any(ctx.needs_input_grad)
        uk = A.kernel_weight(u, dtype, cache, key + "u")
        hx0 = None if hx is None else hx.detach().float().contiguous()
        m0 = None if mask is None else mask.detach().float().contiguous()
        raw, _, xs, wk, B, T = _input_preact(x, None, [w], None, dtype, cache, key)
        ga, be = gamma.detach().float(), beta.detach().float()
        mu = rs = mean = rstd = None
        if kind == "layer":
            var, mu = torch.var_mean(raw, dim=1, unbiased=False)
            rs = torch.rsqrt(var + eps)
            cscale, cshift = ga.contiguous(), be.contiguous()
            var, mean = raw.new_empty(0), raw.new_empty(0)
        else:
            if kind == "batch_train":
                var, mean = torch.var_mean(raw, dim=0, unbiased=False)
            else:
                var, mean = rvar.detach().float(), rmean.detach().float()
            rstd = torch.rsqrt(var + eps)
            cscale = ga * rstd
            cshift = be - mean * cscale
        out = torch.empty(B, T, D * H, device=dev, dtype=_f32)
        save = torch.empty(B, T, D, 2 * H, device=dev, dtype=_f32) if need else None
        check(lib().sbk_ligru_fwd(bf, D, act, ptr(uk), ptr(hx0), ptr(raw), ptr(mu), ptr(rs), ptr(cscale), ptr(cshift),
                                  ptr(m0), B, T, H, ptr(out), ptr(save), stream_of(out)), "sbk_ligru_fwd")
        if need:
            ctx.save_for_backward(out, save, hx0, m0, raw, mu, rs, mean, rstd, cscale, ga, xs, wk)
            ctx.cfg = (kind, eps, act, D, dtype, cache, key, B, T, H, I, u, x.dtype)
        ctx.mark_non_differentiable(mean, var)
        return out, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        out, save, hx0, m0, raw, mu, rs, mean, rstd, cscale, ga, xs, wk = ctx.saved_tensors
        kind, eps, act, D, dtype, cache, key, B, T, H, I, u, xdt = ctx.cfg
        dev = out.device
        bf = int(dtype == _bf16)
        uT = cache.get(key + "uT" + str(bf), [u], lambda: _enc.to_compute(u.detach().t(), dtype))
        dy = None if dy is None else dy.detach().float().contiguous()
        dG = torch.empty(B, T, D, 2 * H, device=dev, dtype=_f32)
        dhw = torch.empty(2, D, B, H, device=dev, dtype=_f32)
        dhx = torch.empty(D * B, H, device=dev, dtype=_f32)
        check(lib().sbk_ligru_bwd(bf, D, act, ptr(uT), ptr(hx0), ptr(out), ptr(save), ptr(m0), ptr(dy), B, T, H,
                                  ptr(dG), ptr(dhw), ptr(dhx), stream_of(out)), "sbk_ligru_bwd")
        need = ctx.needs_input_grad
        du = None
        if need[2]:
            # the weights are shared: one weight-gradient GEMM over the rows of both directions
            hp = [_hprev(out[:, :, d * H:(d + 1) * H], None if hx0 is None else hx0[d * B:(d + 1) * B], reverse=d == 1)
                  for d in range(D)]
            hp = hp[0] if D == 1 else torch.stack(hp, 1).reshape(B * T * D, H)
            du = A.wgrad(A._as(dG.view(B * T * D, 2 * H), dtype), A._as(hp, dtype))
        # gradient of the normalised projection: both directions read the same rows
        g = dG.view(B * T, 2 * H) if D == 1 else (dG[:, :, 0] + dG[:, :, 1]).view(B * T, 2 * H)
        M = B * T
        if kind == "layer":
            L = lib()
            nblk = int(L.sbk_layernorm_bwd_blocks(M))
            part = torch.empty(nblk * 4 * H, device=dev, dtype=_f32)
            draw = torch.empty(M, 2 * H, device=dev, dtype=_f32)
            check(L.sbk_layernorm_bwd(ptr(raw), ptr(g), 0, M, 2 * H, ptr(ga), float(eps), None, ptr(draw), ptr(part),
                                      stream_of(out)), "sbk_layernorm_bwd")
            gb = A.colsum(part, nblk, 4 * H)
            dgamma, dbeta = gb[:2 * H], gb[2 * H:]
        else:
            xhat = (raw - mean) * rstd
            dbeta = A.rowsum(g)
            dgamma = A.rowsum(g * xhat)
            if kind == "batch_train":
                # over the reference's doubled batch this is the plain backward with the directions' gradients summed
                draw = cscale * (g - dbeta / M - xhat * (dgamma / M))
            else:
                draw = g * cscale
        dw, dx = _input_grads(draw, None, 0, I, xs, wk, dtype, xdt, B, T, need[1], need[0])
        return (dx, dw, du, dgamma if need[3] else None, dbeta if need[4] else None,
                dhx if hx0 is not None and need[5] else None, None, None, None, None, None, None, None, None, None, None)


class LiGRU_Layer(torch.nn.Module):
    """Drop-in for speechbrain.nnet.RNN.LiGRU_Layer (RNN.py:1125-1325): same
    constructor, parameters, buffers and forward(x, hx=None) -> h.  The
    normalisation and the recurrence run in csrc/ligru.hip; the recurrent
    dropout pool is the reference's, in host torch."""

    def __init__(self, input_size, hidden_size, num_layers, batch_size, dropout=0.0, nonlinearity="relu",
                 normalization="batchnorm", bidirectional=False):
        super().__init__()
        self.hidden_size = int(hidden_size)
        self.input_size = int(input_size)
        self.batch_size = batch_size
        self.bidirectional = bidirectional
        self.dropout = dropout
        self.w = torch.nn.Linear(self.input_size, 2 * self.hidden_size, bias=False)
        self.u = torch.nn.Linear(self.hidden_size, 2 * self.hidden_size, bias=False)
        if self.bidirectional:
            self.batch_size = self.batch_size * 2
        # any other string still normalises with a LayerNorm, as the reference's else branch does
        if normalization == "batchnorm":
            self.norm = torch.nn.BatchNorm1d(2 * self.hidden_size, momentum=0.05)
        else:
            self.norm = torch.nn.LayerNorm(2 * self.hidden_size)
        self.normalize = True
        self.register_buffer("h_init", torch.zeros(1, self.hidden_size))
        self._init_drop(self.batch_size)
        # parameter-free: the kernel applies the activation; any other string means ReLU
        self.act = _LIGRU_ACT.get(nonlinearity, 0)
        self._wc = _enc.WeightCache()

    def _init_drop(self, batch_size):
        self.drop = torch.nn.Dropout(p=self.dropout, inplace=False)
        self.N_drop_masks = 16000
        self.drop_mask_cnt = 0
        self.register_buffer("drop_masks", self.drop(torch.ones(self.N_drop_masks, self.hidden_size)).data)
        self.register_buffer("drop_mask_te", torch.tensor([1.0]).float())

    def _sample_drop_mask(self, device):
        """The mask rows of this call (RNN.py:1286-1309); None in eval."""
        if not self.training:
            return None
        if self.drop_mask_cnt + self.batch_size > self.N_drop_masks:
            self.drop_mask_cnt = 0
            self.drop_masks = self.drop(torch.ones(self.N_drop_masks, self.hidden_size, device=device)).data
        mask = self.drop_masks[self.drop_mask_cnt:self.drop_mask_cnt + self.batch_size]
        self.drop_mask_cnt = self.drop_mask_cnt + self.batch_size
        return mask

    def _change_batch_size(self, rows, device):
        if self.batch_size != rows:
            self.batch_size = rows
            if self.training:
                self.drop_masks = self.drop(torch.ones(self.N_drop_masks, self.hidden_size, device=device)).data

    def forward(self, x, hx=None):
        require_device(x, hx, self.w.weight)
        H, D = self.hidden_size, 2 if self.bidirectional else 1
        if x.ndim != 3 or x.shape[-1] != self.input_size:
            raise ValueError(f"LiGRU_Layer expects (batch, time, {self.input_size}) (got {tuple(x.shape)})")
        B, T, _ = x.shape
        rows = D * B
        self._change_batch_size(rows, x.device)
        mask = self._sample_drop_mask(x.device)
        if mask is not None and tuple(mask.shape) != (rows, H):
            raise ValueError(f"the dropout pool yields {tuple(mask.shape)} mask rows for a batch of {rows}")
        if hx is not None:
            if hx.shape[-1] != H or hx.numel() not in (H, rows * H):
                raise ValueError(f"hx must be {(rows, H)} or {(1, H)} (got {tuple(hx.shape)})")
            hx = hx.reshape(-1, H).expand(rows, H)
        norm = self.norm
        batch = isinstance(norm, torch.nn.BatchNorm1d)
        kind = "layer" if not batch else ("batch_train" if self.training or norm.running_mean is None else "batch_eval")
        n = rows * T
        if kind == "batch_train" and n <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[n, 2 * H]}")
        out, mean, var = _LiGRULayerFn.apply(x, self.w.weight, self.u.weight, norm.weight, norm.bias, hx, mask,
                                             norm.running_mean if batch else None, norm.running_var if batch else None,
                                             kind, norm.eps, self.act, D, _enc.compute_dtype(), self._wc, "ligru")
        if kind == "batch_train" and self.training and norm.running_mean is not None:
            # torch's update for the reference's row count: both directions' rows, n / (n - 1) unbiased
            with torch.no_grad():
                norm.num_batches_tracked += 1
                mom = norm.momentum if norm.momentum is not None else 1.0 / float(norm.num_batches_tracked)
                norm.running_mean.mul_(1 - mom).add_(mean, alpha=mom)
                norm.running_var.mul_(1 - mom).add_(var, alpha=mom * n / (n - 1))
        return out


class LiGRU(torch.nn.Module):
    """Drop-in for speechbrain.nnet.RNN.LiGRU (RNN.py:961-1122): same
    constructor, forward(x, hx=None) -> (output, h) and state_dict."""

    def __init__(self, hidden_size, input_shape, nonlinearity="relu", normalization="batchnorm", num_layers=1,
                 bias=True, dropout=0.0, re_init=True, bidirectional=False):
        super().__init__()
        self.hidden_size = hidden_size
        self.nonlinearity = nonlinearity
        self.num_layers = num_layers
        self.normalization = normalization
        self.bias = bias
        self.dropout = dropout
        self.re_init = re_init
        self.bidirectional = bidirectional
        self.reshape = False
        if len(input_shape) > 3:
            self.reshape = True
        self.fea_dim = float(torch.prod(torch.tensor(input_shape[2:])))
        self.batch_size = input_shape[0]
        self.rnn = self._init_layers()
        if self.re_init:
            rnn_init(self.rnn)

    def _init_layers(self):
        rnn = torch.nn.ModuleList([])
        current_dim = self.fea_dim
        for _ in range(self.num_layers):
            rnn.append(LiGRU_Layer(current_dim, self.hidden_size, self.num_layers, self.batch_size,
                                   dropout=self.dropout, nonlinearity=self.nonlinearity,
                                   normalization=self.normalization, bidirectional=self.bidirectional))
            current_dim = self.hidden_size * 2 if self.bidirectional else self.hidden_size
        return rnn

    def forward(self, x, hx=None):
        require_device(x, hx, self.rnn[0].w.weight)
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        h = []
        if hx is not None and self.bidirectional:
            hx = hx.reshape(self.num_layers, self.batch_size * 2, self.hidden_size)
        for i, lay in enumerate(self.rnn):
            x = lay(x, hx=None if hx is None else hx[i])
            h.append(x[:, -1, :])
        # the reference's own ops: the bidirectional form is a raw reshape, not a transpose
        h = torch.stack(h, dim=1)
        if self.bidirectional:
            h = h.reshape(h.shape[1] * 2, h.shape[0], self.hidden_size)
        else:
            h = h.transpose(0, 1)
        return x, h


class _Recurrent(torch.nn.Module):
    """The constructor and the forward preamble of both cells."""

    _cell = None            # torch.nn.GRU / torch.nn.LSTM: the parameter container
    _one_way = None         # why bidirectional=True is refused, where it has no kernel

    def __init__(self, hidden_size, input_shape=None, input_size=None, num_layers=1, bias=True, dropout=0.0,
                 re_init=True, bidirectional=False):
        super().__init__()
        self.reshape = False
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size.")
        if bidirectional and self._one_way:
            raise NotImplementedError(self._one_way)
        if input_size is None:
            if len(input_shape) > 3:
                self.reshape = True
            input_size = torch.prod(torch.tensor(input_shape[2:])).item()
        # parameter container: torch's names and init; its forward is never called
        self.rnn = self._cell(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers,
                              dropout=dropout, bidirectional=bidirectional, bias=bias, batch_first=True)
        if re_init:
            rnn_init(self.rnn)
        self._wc = _enc.WeightCache()

    def _prepare(self, x, lengths):
        """x as (batch, time, input_size), cut to the longest row; the token
        ids tok (B, T) and blank of an unmodified one-hot Embedding output (or
        None, None); lens (B,) int32 steps per row when the rows are ragged
        (or None).  Returns (x, tok, blank, lens, T)."""
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        if x.ndim != 3 or x.shape[-1] != self.rnn.input_size:
            raise ValueError(f"{self._cell.__name__} expects (batch, time, {self.rnn.input_size}) "
                             f"(got {tuple(x.shape)})")
        B, T, _ = x.shape
        tag = getattr(x, "_sbk_onehot", None)
        tok = blank = None
        if tag is not None and tag[2] == x._version and tuple(tag[0].shape) == (B, T):
            tok, blank = tag[0], tag[1]   # unmodified one-hot rows: layer 0 never reads x
        lens = None
        if lengths is not None:
            steps = _steps(lengths, T)
            Tn = int(steps.max())
            if Tn < T:
                x = x[:, :Tn]
                tok = None if tok is None else tok[:, :Tn].contiguous()
                T = Tn
            if int(steps.min()) < T:
                lens = steps.to(device=x.device, dtype=torch.int32)
        return x, tok, blank, lens, T


class GRU(_Recurrent):
    _cell = torch.nn.GRU
    _one_way = ("speechbrain_amd GRU is unidirectional (the transducer prediction network); "
                "bidirectional=True has no kernel")

    def forward(self, x, hx=None, lengths=None):
        rnn = self.rnn
        require_device(x, hx, rnn.weight_hh_l0)
        x, tok, blank, lens, T = self._prepare(x, lengths)
        B, L, H = x.shape[0], rnn.num_layers, rnn.hidden_size
        if hx is not None and tuple(hx.shape) != (L, B, H):
            raise ValueError(f"hx must be {(L, B, H)} (got {tuple(hx.shape)})")
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


class LSTM(_Recurrent):
    _cell = torch.nn.LSTM

    def forward(self, x, hx=None, lengths=None):
        rnn = self.rnn
        if hx is not None and not (isinstance(hx, (tuple, list)) and len(hx) == 2):
            raise ValueError("hx must be a tuple (h0, c0)")
        h0, c0 = (None, None) if hx is None else hx
        x, tok, blank, lens, T = self._prepare(x, lengths)
        B, L, H, D = x.shape[0], rnn.num_layers, rnn.hidden_size, 2 if rnn.bidirectional else 1
        for s in (h0, c0):
            if hx is not None and (not torch.is_tensor(s) or tuple(s.shape) != (L * D, B, H)):
                raise ValueError(f"hx must be two tensors of {(L * D, B, H)} "
                                 f"(got {tuple(s.shape) if torch.is_tensor(s) else type(s).__name__})")
        require_device(x, h0, c0, rnn.weight_hh_l0)
        dtype = _enc.compute_dtype()
        y, hns, cns = x, [], []
        for layer in range(L):
            w = [getattr(rnn, f"{n}_l{layer}{sfx}", None) for sfx in ("", "_reverse")[:D]
                 for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            hl = None if hx is None else h0[layer * D:(layer + 1) * D]
            cl = None if hx is None else c0[layer * D:(layer + 1) * D]
            if layer == 0 and tok is not None:
                y, hn, cn = _LSTMLayerFn.apply(None, tok, blank, hl, cl, lens, dtype, self._wc, f"l{layer}", D, *w)
            else:
                y, hn, cn = _LSTMLayerFn.apply(y, None, 0, hl, cl, lens, dtype, self._wc, f"l{layer}", D, *w)
            hns.append(hn)
            cns.append(cn)
            if layer < L - 1 and rnn.dropout > 0:
                y = A.dropout(y, rnn.dropout, self.training)
        return y, (torch.cat(hns, 0), torch.cat(cns, 0))
