"""Drop-in for speechbrain.lobes.models.transformer.TransformerLM
(TransformerLM.py:23-169 over TransformerInterface, Transformer.py:83-192):
the decoder-only language model of LM fusion
(recipes/LibriSpeech/ASR/transformer/hparams/transformer.yaml lm_model, and the
model recipes/LibriSpeech/LM/hparams/transformer.yaml trains).

The constructor is the reference's — signature, defaults, module tree and
construction order — so the LM checkpoint loads with strict=True and a seeded
construction gives the reference's weights:
  positional_encoding, encoder (TransformerEncoder), decoder (only with
  num_decoder_layers > 0), custom_src_module (a NormalizedEmbedding, not
  wrapped), embedding_proj (only with d_embedding), output_proj.layers.{0,1,2}
  = Linear, LayerNorm(eps 1e-6), Linear.
forward(src, hx=None) is the reference's, statement by statement, on the
drop-in modules: the embedding, the MFMA GEMM Linears, TransformerEncoder's
module path (a lookahead mask plus the key padding mask src == 0), the HIP
LayerNorm; differentiable.  What computes is attention_type="regularMHA" with
num_decoder_layers = 0 — the recipes' LM.  The other variants build their tree
and then behave as the reference's forward does there, which fails
(RelPosMHAXL: the (1, 2T−1, d) table does not add to (B, T, d); a decoder
without decoder_use_memory is called with an argument it does not take).

Incremental decoding (decode_step_supported / init_decode_state /
decode_step): the newest token of every row against per-layer key/value caches
(csrc/kvdec.hip, the masked decode-step kernel), for the searcher's
USE_LM_KV_CACHE.
"""
import torch
from torch import nn

from .... import _autograd as A
from .... import _enc
from .... import _kvdec
from ...._lib import require_device
from ....nnet.attention import RelPosEncXL
from ....nnet.linear import Linear
from ....nnet.normalization import LayerNorm
from .Transformer import (NormalizedEmbedding, PositionalEncoding, TransformerDecoder, TransformerEncoder,
                          get_key_padding_mask, get_lookahead_mask)
from .TransformerASR import _ModuleList

_f32 = torch.float32


class TransformerLM(nn.Module):
    def __init__(self, vocab, d_model=512, nhead=8, num_encoder_layers=12, num_decoder_layers=0, d_ffn=2048,
                 dropout=0.1, activation=nn.ReLU, positional_encoding="fixed_abs_sine", normalize_before=False,
                 d_embedding=None, max_length=2500, causal=True, attention_type="regularMHA",
                 decoder_use_memory=False):
        super().__init__()
        # TransformerInterface.__init__ (Transformer.py:108-192), encoder_module "transformer"
        self.causal = causal
        self.attention_type = attention_type
        self.positional_encoding_type = positional_encoding
        self.encoder_kdim = self.encoder_vdim = self.decoder_kdim = self.decoder_vdim = None
        assert attention_type in ["regularMHA", "RelPosMHAXL"]
        assert positional_encoding in ["fixed_abs_sine", None]
        assert num_encoder_layers + num_decoder_layers > 0, \
            "number of encoder layers and number of decoder layers cannot both be 0!"
        if positional_encoding == "fixed_abs_sine":
            self.positional_encoding = PositionalEncoding(d_model, max_length)
        if attention_type == "RelPosMHAXL":  # overrides any other pos_embedding (:130-135)
            self.positional_encoding = RelPosEncXL(d_model)
            self.positional_encoding_decoder = PositionalEncoding(d_model, max_length)
        if num_encoder_layers > 0:
            self.encoder = TransformerEncoder(nhead=nhead, num_layers=num_encoder_layers, d_ffn=d_ffn,
                                              d_model=d_model, dropout=dropout, activation=activation,
                                              normalize_before=normalize_before, causal=self.causal,
                                              attention_type=self.attention_type)
        if num_decoder_layers > 0:  # always regularMHA, causal (:177-192)
            self.decoder = TransformerDecoder(num_layers=num_decoder_layers, nhead=nhead, d_ffn=d_ffn, d_model=d_model,
                                              dropout=dropout, activation=activation,
                                              normalize_before=normalize_before, causal=True,
                                              attention_type="regularMHA")
        # TransformerLM.__init__ (TransformerLM.py:89-112)
        self.d_embedding = d_embedding
        if d_embedding is None:
            self.d_embedding = d_model
        self.custom_src_module = NormalizedEmbedding(self.d_embedding, vocab)
        self.embedding_proj = None
        if d_embedding is not None:
            self.embedding_proj = Linear(input_size=self.d_embedding, n_neurons=d_model)
        self.output_proj = _ModuleList(Linear(input_size=d_model, n_neurons=d_model), LayerNorm(d_model, eps=1e-6),
                                       Linear(input_size=d_model, n_neurons=vocab))
        self.num_encoder_layers = num_encoder_layers
        self.num_decoder_layers = num_decoder_layers
        self.decoder_use_memory = decoder_use_memory
        self._reset_params()

    def forward(self, src, hx=None):
        """TransformerLM.py:114-151: src (B, T) tokens → (B, T, vocab) logits."""
        src_mask, src_key_padding_mask = self.make_masks(src)
        src = self.custom_src_module(src)
        if self.embedding_proj is not None:
            src = self.embedding_proj(src)
        src = src + self.positional_encoding(src)
        if self.num_encoder_layers > 0:
            encoder_out, _ = self.encoder(src=src, src_mask=src_mask, src_key_padding_mask=src_key_padding_mask)
        if self.num_decoder_layers > 0:
            if self.decoder_use_memory:
                encoder_out, _, _ = self.decoder(tgt=src, memory=encoder_out, tgt_mask=src_mask,
                                                 tgt_key_padding_mask=src_key_padding_mask)
            else:
                encoder_out, _ = self.decoder(src=src, tgt=src, tgt_mask=src_mask,
                                              tgt_key_padding_mask=src_key_padding_mask)
        pred = self.output_proj(encoder_out)
        return pred

    def _reset_params(self):
        for p in self.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)

    def make_masks(self, src, pad_idx=0, look_ahead_mask=True, padding_mask=True):
        """TransformerLM.py:158-169 → (src_mask, src_key_padding_mask)."""
        src_mask = None
        if look_ahead_mask:
            src_mask = get_lookahead_mask(src)
        src_key_padding_mask = None
        if padding_mask:
            src_key_padding_mask = get_key_padding_mask(src, pad_idx)
        return src_mask, src_key_padding_mask

    # ------------------------------------------------ incremental decoding
    def decode_step_supported(self):
        """decode_step's kernels take this model: regularMHA encoder layers
        and no decoder, the absolute sine table, head size a multiple of 4 up
        to 128, the default in_proj layout (bias, kdim = vdim = d_model, no
        bias_kv / zero_attn), a GELU or ReLU FFN."""
        if (self.attention_type != "regularMHA" or self.num_decoder_layers > 0 or self.num_encoder_layers == 0
                or self.positional_encoding_type != "fixed_abs_sine"):
            return False
        for layer in self.encoder.layers:
            att = layer.self_att
            a = att.att
            dh = att.d_model // att.nhead
            if (dh % 4 or dh > _kvdec.SELF_DH_MAX or not a._qkv_same_embed_dim or a.bias_k is not None
                    or a.add_zero_attn or a.in_proj_bias is None):
                return False
            try:
                name, slope = layer.pos_ffn.act_name()
            except NotImplementedError:
                return False
            if not (name == "gelu" or (name in ("relu", "leaky_relu") and slope == 0.0)):
                return False
        return True

    @torch.no_grad()
    def init_decode_state(self, rows):
        """The state of decode_step for `rows` prefixes decoded in step."""
        if not self.decode_step_supported():
            raise NotImplementedError("TransformerLM.decode_step: this model is not on the incremental path "
                                      "(see decode_step_supported); use forward()")
        w = self.encoder.layers[0].self_att.att.in_proj_weight
        require_device(w)
        att = self.encoder.layers[0].self_att
        return _kvdec.LMDecodeState(int(rows), len(self.encoder.layers), att.d_model, att.nhead, w.device)

    @torch.no_grad()
    def decode_step(self, tokens, state, pad_idx=0):
        """One incremental step of forward(): tokens (N,) — the newest token
        of every row — → (N, vocab) logits, equal to forward(prefixes)[:, -1]
        of the rows' prefixes.  The embedding (and embedding_proj) plus the
        sine row of the position; per layer, in TransformerEncoderLayer's
        order: LayerNorm → one in_proj GEMM (N × 3E) →
        sbk_kv_decode_self_attn_masked over the cache, the keys whose token
        was pad_idx masked as forward's key padding mask does → out_proj
        (+ residual) → LayerNorm → the FFN (+ residual); the encoder's closing
        LayerNorm; output_proj.  Nothing is read back to the host."""
        require_device(tokens)
        N, H = state.rows, state.nhead
        if tokens.shape != (N,):
            raise ValueError(f"decode_step: tokens {tuple(tokens.shape)} != ({N},) rows of the state")
        pe = self.positional_encoding.pe[0]
        if state.steps >= pe.shape[0]:
            raise ValueError(f"decode_step: position {state.steps} is beyond the sine table ({pe.shape[0]})")
        dtype = _enc.compute_dtype()
        x = self.custom_src_module(tokens.unsqueeze(1))[:, 0]
        if self.embedding_proj is not None:
            x = self.embedding_proj(x)
        x = x + pe[state.steps]
        L = state.begin_step(tokens.eq(pad_idx))
        for i, layer in enumerate(self.encoder.layers):
            pre = layer.normalize_before
            sa = layer.self_att
            u = layer.norm1(x) if pre else x
            qkv = A.linear(u, sa.att.in_proj_weight, sa.att.in_proj_bias, dtype, sa._wc, "kv_in", out_dtype=_f32)
            o = _kvdec.kv_decode_self_attn_masked(qkv, state.kc[i], state.vc[i], state.anc, state.keymask, H, L)
            x = A.linear(o, sa.att.out_proj.weight, sa.att.out_proj.bias, dtype, sa._wc, "g_out", res=x)
            if not pre:
                x = layer.norm1(x)
            u = layer.norm2(x) if pre else x
            x = layer.pos_ffn.run(_enc.to_compute(u, dtype), dtype, residual=x)
            if not pre:
                x = layer.norm2(x)
        x = self.encoder.norm(x)
        state.steps = L
        return self.output_proj(x)
