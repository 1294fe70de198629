"""Generate tests/golden/rnn_search.npz (data only) from the REAL reference's RNN
searchers (decoders/seq2seq.py) on the CPU, where the reference checkout is
present (gen_s2s_golden.py's stubs):  python tests/golden/gen_rnn_search_golden.py

Keys: sd.{dec.location,dec.content,emb,fc,ctc,gru_lm,tlm}.* the seeded
state_dicts (no sine table); wav_len (3); names; {c}.cfg (JSON: "cls", "kind",
the searcher's keyword arguments), {c}.enc (3, 40, 20), {c}.pred (B, L) int64
padded with -1, {c}.scores (B, topk) ((B) for greedy).
Admission rule (gen_s2s_golden.py's): a case's hypotheses are identical when
enc_states is multiplied by 1 + 1e-4·randn, for three noise seeds, and no score
carries the −1e20 sentinel; the attention-shift case also differs from the same
search without the mask.  A case keeps the first encoder seed from 0 that passes.
"""
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
from speechbrain.lobes.models.transformer.TransformerLM import TransformerLM  # noqa: E402
from speechbrain.nnet.embedding import Embedding  # noqa: E402
from speechbrain.nnet.linear import Linear  # noqa: E402
from speechbrain.nnet.RNN import AttentionalRNNDecoder  # noqa: E402
from rnn_search_common import build_modules, make_searcher  # noqa: E402

E, B, L = 20, 3, 40
BASE = dict(bos_index=1, eos_index=2, blank_index=0, min_decode_ratio=0.1, max_decode_ratio=0.5)
BEAM = dict(beam_size=17, topk=2, using_eos_threshold=False)
CASES = {
    "location": dict(cls="S2SRNNBeamSearcher", kind="location", **BEAM),
    "content": dict(cls="S2SRNNBeamSearcher", kind="content", **{**BEAM, "using_eos_threshold": True}),
    "cov_shift": dict(cls="S2SRNNBeamSearcher", kind="location", coverage_penalty=1.5, using_max_attn_shift=True,
                      max_attn_shift=15, **BEAM),
    "no_lennorm": dict(cls="S2SRNNBeamSearcher", kind="location", coverage_penalty=1.5, length_normalization=False,
                       **BEAM),
    "ctc_full": dict(cls="S2SRNNBeamSearcher", kind="location", ctc_weight=0.4, ctc_score_mode="full", **BEAM),
    "greedy": dict(cls="S2SRNNGreedySearcher", kind="location"),
    "gru_lm": dict(cls="S2SRNNBeamSearchLM", kind="location", lm_weight=0.5, **BEAM),
    "tlm": dict(cls="S2SRNNBeamSearchTransformerLM", kind="content", lm_weight=0.5, **BEAM),
}
WAV_LEN = torch.tensor([1.0, 0.62, 0.81])


def seeded_modules():
    torch.manual_seed(23)
    m = build_modules(AttentionalRNNDecoder, Embedding, Linear, TransformerLM)
    with torch.no_grad():
        for name in ("fc", "ctc"):
            for p in m[name].parameters():
                p.mul_(6.0)      # peaked distributions
        m["fc"].w.bias[2] += 2.0   # eos likely enough for hypotheses to finish inside the search
    return {k: v.eval() for k, v in m.items()}


def admitted(s, enc, plain):
    res = s(enc.clone(), WAV_LEN)
    scores = torch.as_tensor(res[1])
    if float(scores.min()) <= -1e10:
        return None, "sentinel"
    for seed in (101, 102, 103):
        noise = 1 + 1e-4 * torch.randn(enc.shape, generator=torch.Generator().manual_seed(seed))
        again = s(enc * noise, WAV_LEN)
        if again[0] != res[0]:
            return None, f"hypotheses change under noise {seed}"
        if scores.dim() == 2 and torch.argsort(again[1], -1, True).tolist() != torch.argsort(res[1], -1, True).tolist():
            return None, f"top-k order changes under noise {seed}"
    if plain is not None and plain(enc.clone(), WAV_LEN)[0] == res[0]:
        return None, "the shift mask blocks nothing"
    return res, None


if __name__ == "__main__":
    out = {}
    m = seeded_modules()
    for name, mod in m.items():
        for k, v in mod.state_dict().items():
            if k != "positional_encoding.pe":
                out[f"sd.{name}.{k}"] = v.numpy().copy()
    out["wav_len"] = WAV_LEN.numpy()
    out["names"] = np.array(list(CASES), dtype="U32")
    with torch.no_grad():
        for name, case in CASES.items():
            cfg = {**BASE, **case}
            s = make_searcher(RS, m, cfg)
            plain = make_searcher(RS, m, {**cfg, "using_max_attn_shift": False}) if cfg.get("using_max_attn_shift") else None
            for seed in range(40):
                enc = 2.0 * torch.randn(B, L, E, generator=torch.Generator().manual_seed(seed))
                res, _ = admitted(s, enc, plain)
                if res is not None:
                    break
            assert res is not None, name
            out[f"{name}.cfg"] = np.array(json.dumps(cfg))
            out[f"{name}.enc"] = enc.numpy()
            out[f"{name}.pred"] = S._pad(res[0], -1, np.int64)
            out[f"{name}.scores"] = np.asarray(torch.as_tensor(res[1]).numpy(), dtype=np.float32)
            print(f"{name}: encoder seed {seed}, lengths {[len(p) for p in res[0]]}, stable")
    path = os.path.join(OUT, "rnn_search.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
