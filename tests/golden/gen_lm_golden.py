"""Generate tests/golden/lm.npz from the REAL reference's TransformerLM
(speechbrain/lobes/models/transformer/TransformerLM.py) and its
S2STransformerBeamSearch with LM fusion (decoders/seq2seq.py), on the CPU.

    python tests/golden/gen_lm_golden.py

Runs only where the reference checkout is present (as gen_s2s_golden.py, whose
inert stubs for torchaudio, hyperpyyaml and ruamel it uses); the committed
lm.npz is what the tests read.  The file holds data only.

Keys
  lm.names = [A, B].  A: vocab 30, d_model 32, 4 heads, 2 layers, d_ffn 64,
  GELU, post-norm; B: the same sizes with d_embedding 16, pre-norm, ReLU.
  lm.{m}.kw          JSON of the constructor's keyword arguments (activation by name)
  lm.{m}.init.*      the state_dict right after torch.manual_seed(0) and construction
  lm.{m}.sd.*        the state_dict the outputs below were computed with: a
                     construction under another seed whose biases and LayerNorm
                     parameters were then drawn, so that none is 0 / 1
                     (both without the sine table, a buffer: lm.pe_head holds its first 16 rows)
  lm.tokens (3, 9)   int64: zeros in the middle of row 0, trailing zeros in row 1, none in column 0
  lm.proj (3, 9, 30) the fixed randn of the scalar sum(logits · proj)
  lm.{m}.logits (3, 9, 30); lm.{m}.grad.{parameter} for the parameters of lm.grad_names
  lm.signature       JSON [[parameter, kind, repr(default) | "<empty>"], ...] of TransformerLM.__init__
  search.sd.lm.*     the LM of the searches (A's sizes, vocab 23), without the sine table
  search.names; search.{c}.cfg (JSON of the searcher's keyword arguments),
  .enc (3, 21, 64) (only where the case does not use s2s.npz's search.enc),
  .pred (B, L) int64 padded with -1, .scores (B, topk), .log_probs (B·topk, L)
  padded with NaN
The ASR model, wav_len and (unless a case stores its own) the encoder states of
the searches are s2s.npz's (search.sd.*, search.wav_len, search.enc).
Checks made here, before writing — gen_s2s_golden.py's admission rule: every
search case must give identical hypotheses when enc_states is multiplied by
1 + 1e-4·randn, for three noise seeds, and no returned score may carry the
−1e20 sentinel; a case that fails gets another seed, never a tolerance.  The
token-0 case (ctc_weight 0, so that blank / pad index 0 may be emitted and the
LM's key padding mask acts inside the search) is the first encoder seed whose
case passes that rule AND whose stored prefixes contain a 0.
"""
import inspect
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import gen_s2s_golden as S  # noqa: E402  (installs the stubs, puts the reference on sys.path)

import torch  # noqa: E402
from speechbrain.decoders import seq2seq as RS  # noqa: E402
from speechbrain.lobes.models.transformer.TransformerASR import TransformerASR  # noqa: E402
from speechbrain.lobes.models.transformer.TransformerLM import TransformerLM  # noqa: E402
from speechbrain.nnet.linear import Linear  # noqa: E402

ACT = {"GELU": torch.nn.GELU, "ReLU": torch.nn.ReLU}
LMS = {
    "A": dict(vocab=30, d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=0, d_ffn=64, dropout=0.0,
              activation="GELU", normalize_before=False),
    "B": dict(vocab=30, d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=0, d_ffn=64, dropout=0.0,
              activation="ReLU", normalize_before=True, d_embedding=16),
}
GRAD_NAMES = ["encoder.layers.0.self_att.att.in_proj_weight", "custom_src_module.emb.Embedding.weight"]
PE = "positional_encoding.pe"


def build_lm(kw, seed):
    torch.manual_seed(seed)
    return TransformerLM(**{**kw, "activation": ACT[kw["activation"]]}).eval()


def draw_small_parameters(lm, seed):
    """Biases and LayerNorm parameters away from their 0 / 1 initial values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn(p.shape, generator=g))


def put_sd(out, prefix, lm):
    for k, v in lm.state_dict().items():
        if k != PE:
            out[prefix + k] = v.numpy().copy()


def gen_lm(out):
    tokens = torch.tensor([[5, 11, 0, 0, 7, 3, 29, 1, 4],
                           [9, 2, 17, 4, 21, 8, 0, 0, 0],
                           [1, 28, 6, 13, 2, 19, 10, 23, 12]])
    assert bool((tokens[:, 0] != 0).all())
    proj = torch.randn(3, 9, 30, generator=torch.Generator().manual_seed(41))
    out["lm.names"] = np.array(list(LMS), dtype="U8")
    out["lm.tokens"] = tokens.numpy()
    out["lm.proj"] = proj.numpy()
    out["lm.grad_names"] = np.array(GRAD_NAMES, dtype="U64")
    for i, (name, kw) in enumerate(LMS.items()):
        out[f"lm.{name}.kw"] = np.array(json.dumps(kw))
        init = build_lm(kw, 0)
        put_sd(out, f"lm.{name}.init.", init)
        out["lm.pe_head"] = init.state_dict()[PE][:, :16].numpy().copy()
        lm = build_lm(kw, 31 + i)
        draw_small_parameters(lm, 51 + i)
        put_sd(out, f"lm.{name}.sd.", lm)
        logits = lm(tokens)
        assert bool(torch.isfinite(logits).all())
        (logits * proj).sum().backward()
        out[f"lm.{name}.logits"] = logits.detach().numpy()
        params = dict(lm.named_parameters())
        for gname in GRAD_NAMES:
            out[f"lm.{name}.grad.{gname}"] = params[gname].grad.numpy().copy()
        print(f"lm.{name}: logits {tuple(logits.shape)}, |logits| max {float(logits.abs().max()):.3f}")
    out["lm.signature"] = np.array(json.dumps(
        [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
         for p in inspect.signature(TransformerLM.__init__).parameters.values()]))


# ------------------------------------------------------------------ searches
LM_SEARCH_KW = {**LMS["A"], "vocab": 23}
LM_SEARCH_SEED = 61
BASE = dict(S.BASE, beam_size=3, topk=2, using_eos_threshold=False, return_log_probs=True, lm_weight=0.6,
            temperature=1.15, temperature_lm=1.15, length_normalization=True)
# lm_w0.0: without a CTC term this model ends two of its utterances at once
# ([[], [], [3]]); eos is held back for the first 0.3 · 21 steps so that the
# case decodes prefixes
CASES = {"lm_w0.0": dict(ctc_weight=0.0, min_decode_ratio=0.3), "lm_w0.4": dict(ctc_weight=0.4), "lm_tok0": dict(ctc_weight=0.0)}


def load_asr():
    """The ASR model of s2s.npz."""
    g = np.load(os.path.join(OUT, "s2s.npz"))
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=64, nhead=4, num_encoder_layers=1,
                        num_decoder_layers=2, d_ffn=128, dropout=0.0, activation=torch.nn.GELU,
                        normalize_before=True).eval()
    seq_lin = Linear(input_size=64, n_neurons=23).eval()
    ctc_lin = Linear(input_size=64, n_neurons=23).eval()

    def sub(prefix):
        return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}

    sd = sub("search.sd.tr.")
    sd[PE] = tr.state_dict()[PE]
    tr.load_state_dict(sd, strict=True)
    seq_lin.load_state_dict(sub("search.sd.seq."), strict=True)
    ctc_lin.load_state_dict(sub("search.sd.ctc."), strict=True)
    return [tr, seq_lin, ctc_lin], torch.from_numpy(g["search.enc"]), torch.from_numpy(g["search.wav_len"])


def build_search_lm():
    lm = build_lm(LM_SEARCH_KW, LM_SEARCH_SEED)
    draw_small_parameters(lm, LM_SEARCH_SEED + 1)
    with torch.no_grad():
        for p in lm.output_proj.layers[2].parameters():
            p.mul_(6.0)      # a peaked distribution: the LM term moves the search
    return lm


def admit(searcher, enc, wav_len, name):
    """The result of a case, or the reason it is not admitted."""
    res = searcher(enc.clone(), wav_len)
    if not float(res[1].min()) > -1e10:
        return None, "a returned hypothesis carries a sentinel"
    for seed in (101, 102, 103):
        noise = 1 + 1e-4 * torch.randn(enc.shape, generator=torch.Generator().manual_seed(seed))
        again = searcher(enc * noise, wav_len)
        if again[0] != res[0]:
            return None, f"hypotheses change under 1e-4 noise (seed {seed})"
        for i in range(len(res[0])):      # the second-best hypothesis too (topk_scores' order)
            if torch.argsort(again[1][i], descending=True).tolist() != torch.argsort(res[1][i],
                                                                                     descending=True).tolist():
                return None, f"the order of the hypotheses changes under 1e-4 noise (seed {seed})"
        if [lp.shape for lp in again[2]] != [lp.shape for lp in res[2]]:
            return None, f"the second-best hypotheses change under 1e-4 noise (seed {seed})"
    return res, None


def gen_search(out):
    modules, enc0, wav_len = load_asr()
    lm = build_search_lm()
    put_sd(out, "search.sd.lm.", lm)
    out["search.lm_kw"] = np.array(json.dumps(LM_SEARCH_KW))
    out["search.names"] = np.array(list(CASES), dtype="U32")
    with torch.no_grad():
        for name, kw in CASES.items():
            cfg = {**BASE, **kw}
            searcher = RS.S2STransformerBeamSearch(modules=modules, lm_modules=lm, **cfg)
            if name != "lm_tok0":
                res, why = admit(searcher, enc0, wav_len, name)
                assert res is not None, f"{name}: {why}; pick another LM seed"
                enc = enc0
            else:
                # encoder seeds in order; the first whose case is admitted and decodes a 0
                for seed in range(200, 400):
                    enc = 3.0 * torch.randn(3, 21, 64, generator=torch.Generator().manual_seed(seed))
                    res, why = admit(searcher, enc, wav_len, name)
                    if res is None:
                        print(f"{name}: encoder seed {seed}: {why}")
                        continue
                    if any(0 in p for p in res[0]):
                        print(f"{name}: encoder seed {seed}")
                        break
                    print(f"{name}: encoder seed {seed}: no 0 in the hypotheses")
                else:
                    raise AssertionError("no encoder seed gives an admitted case that decodes a 0")
                out[f"search.{name}.enc"] = enc.numpy()
            if name == "lm_tok0":
                assert any(0 in p for p in res[0]), "no stored prefix of the token-0 case contains a 0"
            out[f"search.{name}.cfg"] = np.array(json.dumps(cfg))
            out[f"search.{name}.pred"] = S._pad(res[0], -1, np.int64)
            out[f"search.{name}.scores"] = res[1].numpy()
            out[f"search.{name}.log_probs"] = S._pad([lp.tolist() for lp in res[2]], np.nan, np.float32)
            print(f"search.{name}: {res[0]}, stable")
        # the LM term moves the search: without it the first case decodes something else
        plain = RS.S2STransformerBeamSearch(modules=modules, **{**BASE, **CASES["lm_w0.0"], "lm_weight": 0.0})
        assert plain(enc0.clone(), wav_len)[0] != S_unpad(out["search.lm_w0.0.pred"]), \
            "LM fusion does not change the hypotheses of lm_w0.0; pick another LM seed"


def S_unpad(a):
    return [row[row != -1].tolist() for row in a]


if __name__ == "__main__":
    out = {}
    gen_lm(out)
    gen_search(out)
    path = os.path.join(OUT, "lm.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
