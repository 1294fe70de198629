"""Generate tests/golden/s2s.npz from the REAL reference's CTC prefix scorer
(speechbrain/decoders/ctc.py) and S2S searchers (decoders/seq2seq.py) on the
CPU.

    python tests/golden/gen_s2s_golden.py

Runs only where the reference checkout is present (as gen_losses_golden.py);
the committed s2s.npz is what the tests read.  torchaudio, hyperpyyaml and
ruamel.yaml are absent here and unused by the decoders, so inert stubs stand
in for them before `import speechbrain`.  The file holds data only.

Keys
  scorer.names                      the scorer scripts
  scorer.{s}.x (B, T, V) fp32 log-probs BEFORE the scorer's in-place masking,
  .lens (B) int64, .cfg = [beam, blank, eos, n_steps, C (0 = full)];
  scorer.{s}.{i}.g (N, i) the prefixes given to step i, .cand (N, C) (partial),
  .out = the returned psi − psi_prev (N, V), .index (B, beam) given to
  permute_mem, .r (T, 2, N) and .psi (N, V) = what permute_mem returned.
  search.sd.tr.* / .seq.* / .ctc.*  the seeded state_dicts, without the
  positional sine table (a buffer: search.pe_head holds its first 32 rows)
  search.enc (3, 21, 64), search.wav_len
  search.names; search.{c}.cfg (JSON of the searcher's keyword arguments),
  .pred (B, L) int64 padded with -1, .scores (B, topk), .log_probs
  (B·topk, L) padded with NaN (where returned)
  greedy.pred / greedy.scores       S2SGreedySearcher on the same model
  signatures                        JSON {name: [[parameter, kind, repr(default) | "<empty>"], ...]}
  filters                           JSON [[function, input, eos / blank id, output], ...]
Checks made here, before writing:
  * every scorer script is rerun with torch.set_default_dtype(float64) and
    must agree with the stored fp32 values to 1e-5·max(1, |v|);
  * every search case must give identical hypotheses when enc_states is
    multiplied by 1 + 1e-4·randn, for three noise seeds, and no returned
    score may carry the −1e20 sentinel (such scores tie exactly in fp32) — a
    case that fails either gets another seed, never a tolerance.
"""
import inspect
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def _install_stubs():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    def _raise(*a, **k):
        raise RuntimeError("stubbed dependency")

    ta = stub("torchaudio", set_audio_backend=lambda *a, **k: None, load=_raise, save=_raise, info=_raise)
    ta.transforms = stub("torchaudio.transforms")
    ta.functional = stub("torchaudio.functional")
    stub("hyperpyyaml", resolve_references=_raise, load_hyperpyyaml=_raise)
    r = stub("ruamel")
    r.yaml = stub("ruamel.yaml", YAML=_raise)
    sys.path.insert(0, REF)


_install_stubs()
import torch  # noqa: E402

torch.set_num_threads(4)
from speechbrain.decoders import ctc as RC  # noqa: E402
from speechbrain.decoders import seq2seq as RS  # noqa: E402
from speechbrain.lobes.models.transformer.TransformerASR import TransformerASR  # noqa: E402
from speechbrain.nnet.linear import Linear  # noqa: E402


def _agree(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.size == 0 or err.max() <= 1e-5, (what, err.max())


# ------------------------------------------------------------------- scorer
# name: (B, beam, T, V, lens, C (0 = full), blank, eos, n_steps, seed)
SCRIPTS = {
    "small_full": (2, 3, 9, 7, [9, 6], 0, 0, 2, 3, 11),
    "small_partial": (2, 3, 9, 7, [9, 6], 4, 0, 2, 3, 12),
    "single": (1, 1, 2, 5, [2], 0, 0, 2, 3, 13),
    "wide_full": (3, 4, 21, 300, [21, 13, 17], 0, 0, 2, 3, 14),
    "long_prefix": (2, 2, 5, 6, [5, 4], 0, 0, 2, 6, 15),
    "blank3": (2, 3, 9, 7, [9, 6], 0, 3, 2, 3, 16),
}


def script_plan(name):
    """The inputs of a script, fixed by its seed: x, and for every step the
    candidates (partial) and the (B, beam) index given to permute_mem.  The
    prefixes follow from the indices."""
    B, beam, T, V, lens, C, blank, eos, n_steps, seed = SCRIPTS[name]
    g = torch.Generator().manual_seed(seed)
    N = B * beam
    x = torch.randn(B, T, V, generator=g).log_softmax(-1)
    prefixes = torch.empty(N, 0, dtype=torch.long)
    steps = []
    for i in range(n_steps):
        cand = None
        if C:
            rows = []
            for n in range(N):
                perm = torch.randperm(V, generator=g).tolist()
                if i > 0 and n % 2 == 0:      # the row's last token is a candidate: the phi = r_b path
                    last = int(prefixes[n, -1])
                    perm = [last] + [p for p in perm if p != last]
                rows.append(perm[:C])
            cand = torch.tensor(rows)
        index = torch.empty(B, beam, dtype=torch.long)
        for b in range(B):
            for k in range(beam):
                parent = int(torch.randint(0, beam, (1,), generator=g))
                if C:
                    row = cand[b * beam + parent].tolist()
                    if i == 0 and (b, k) == (0, 1):   # a token that is not a candidate: the candidate-0 fallback
                        tok = next(v for v in range(V) if v not in row)
                    else:
                        tok = row[int(torch.randint(0, C, (1,), generator=g))]
                elif k == 0 and i > 0:                # repeat the parent's last token
                    tok = int(prefixes[b * beam + parent, -1])
                elif (b, k) == (0, 1):
                    tok = eos
                else:
                    tok = int(torch.randint(0, V, (1,), generator=g))
                index[b, k] = parent * V + tok
        steps.append((prefixes, cand, index))
        parent_rows = (index // V + torch.arange(B).unsqueeze(1) * beam).view(-1)
        prefixes = torch.cat([prefixes[parent_rows], (index % V).view(-1, 1)], dim=1)
    return x, steps


def run_script(name, dtype):
    B, beam, T, V, lens, C, blank, eos, n_steps, seed = SCRIPTS[name]
    x, steps = script_plan(name)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        scorer = RC.CTCPrefixScorer(x.clone().to(dtype), torch.tensor(lens), B, beam, blank, eos)
        state, res = None, []
        for prefixes, cand, index in steps:
            out, memory = scorer.forward_step(prefixes, state, cand, None)
            state = scorer.permute_mem(memory, index)
            res.append((out.clone(), state[0].clone(), state[1].clone()))
    finally:
        torch.set_default_dtype(prev)
    return x, steps, res


def gen_scorer(out):
    out["scorer.names"] = np.array(list(SCRIPTS), dtype="U32")
    for name, (B, beam, T, V, lens, C, blank, eos, n_steps, seed) in SCRIPTS.items():
        x, steps, r32 = run_script(name, torch.float32)
        _, _, r64 = run_script(name, torch.float64)
        k = f"scorer.{name}"
        out[k + ".x"] = x.numpy()
        out[k + ".lens"] = np.array(lens, dtype=np.int64)
        out[k + ".cfg"] = np.array([beam, blank, eos, n_steps, C], dtype=np.int64)
        for i, ((prefixes, cand, index), a, b) in enumerate(zip(steps, r32, r64)):
            for what, u, v in zip(("out", "r", "psi"), a, b):
                assert u.dtype == torch.float32 and v.dtype == torch.float64
                _agree(u.numpy(), v.numpy(), (name, i, what))
                out[f"{k}.{i}.{what}"] = u.numpy()
            out[f"{k}.{i}.g"] = prefixes.numpy()
            out[f"{k}.{i}.index"] = index.numpy()
            if cand is not None:
                out[f"{k}.{i}.cand"] = cand.numpy()
        print(f"{k}: {n_steps} steps, fp32 vs fp64 ok")


# ------------------------------------------------------------------ searches
BASE = dict(bos_index=1, eos_index=2, blank_index=0, min_decode_ratio=0.0, max_decode_ratio=1.0)
CASES = {}
for _w in (0.0, 0.4, 1.0):
    for _m in ("full", "partial"):
        CASES[f"w{_w}_{_m}"] = dict(beam_size=4, topk=2, using_eos_threshold=False, ctc_weight=_w, ctc_score_mode=_m)
CASES["beam1"] = dict(beam_size=1, topk=1, using_eos_threshold=False, ctc_weight=0.4, ctc_score_mode="partial")
CASES["no_lennorm"] = dict(beam_size=4, topk=2, using_eos_threshold=False, ctc_weight=0.4, ctc_score_mode="partial",
                           length_normalization=False)
CASES["eos_thr"] = dict(beam_size=4, topk=2, using_eos_threshold=True, ctc_weight=0.4, ctc_score_mode="full",
                        min_decode_ratio=0.2, return_log_probs=True)


# Seeds 3 / 4 were tried first.  With them the ctc_weight 0 cases change under
# the noise, and the eos-threshold case decodes past the utterances' frame
# counts: every beam then carries one CTC sentinel (0.4 · −1e20), next to which
# all fp32 scores tie exactly, and the hypotheses are whatever order top-k
# gives ties.  Model seeds 3-17 × encoder seeds 4-11 were searched in order
# for the first pair with every case stable and free of sentinels.
MODEL_SEED, ENC_SEED = 17, 4


def build_model(seed=None):
    torch.manual_seed(MODEL_SEED if seed is None else seed)
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=64, nhead=4, num_encoder_layers=1,
                        num_decoder_layers=2, d_ffn=128, dropout=0.0, activation=torch.nn.GELU,
                        normalize_before=True).eval()
    seq_lin = Linear(input_size=64, n_neurons=23).eval()
    ctc_lin = Linear(input_size=64, n_neurons=23).eval()
    with torch.no_grad():
        for lin in (seq_lin, ctc_lin):
            for p in lin.parameters():
                p.mul_(6.0)      # peaked distributions
    return tr, seq_lin, ctc_lin


class _RefGreedy(RS.S2SGreedySearcher):
    """The reference has no transformer greedy searcher: its base class with
    S2STransformerBeamSearch's forward_step."""

    def __init__(self, modules, **kw):
        super().__init__(**kw)
        self.model, self.fc = modules[0], modules[1]
        self.softmax = torch.nn.LogSoftmax(dim=-1)

    def reset_mem(self, batch_size, device):
        return None

    def forward_step(self, inp_tokens, memory, enc_states, enc_lens):
        memory = RS._update_mem(inp_tokens, memory)
        pred, attn = self.model.decode(memory, enc_states)
        return self.softmax(self.fc(pred))[:, -1, :], memory, attn


def _pad(rows, fill, dtype):
    L = max(len(r) for r in rows)
    a = np.full((len(rows), L), fill, dtype=dtype)
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a


def gen_search(out):
    tr, seq_lin, ctc_lin = build_model()
    n_par = sum(p.numel() for m in (tr, seq_lin, ctc_lin) for p in m.parameters())
    for pre, mod in (("tr", tr), ("seq", seq_lin), ("ctc", ctc_lin)):
        for k, v in mod.state_dict().items():
            if k == "positional_encoding.pe":     # the (1, 2500, 64) sine table: a buffer, 640 kB, no seed in it
                out["search.pe_head"] = v[:, :32].numpy()
                continue
            out[f"search.sd.{pre}.{k}"] = v.numpy()
    enc = 3.0 * torch.randn(3, 21, 64, generator=torch.Generator().manual_seed(ENC_SEED))
    wav_len = torch.tensor([1.0, 0.62, 0.81])
    out["search.enc"] = enc.numpy()
    out["search.wav_len"] = wav_len.numpy()
    out["search.names"] = np.array(list(CASES), dtype="U32")
    preds = {}
    with torch.no_grad():
        for name, kw in CASES.items():
            cfg = {**BASE, **kw}
            searcher = RS.S2STransformerBeamSearch(modules=[tr, seq_lin, ctc_lin], **cfg)
            res = searcher(enc.clone(), wav_len)
            assert float(res[1].min()) > -1e10, f"{name}: a returned hypothesis carries a sentinel; pick another seed"
            for seed in (101, 102, 103):
                noise = 1 + 1e-4 * torch.randn(enc.shape, generator=torch.Generator().manual_seed(seed))
                again = searcher(enc * noise, wav_len)
                assert again[0] == res[0], f"{name}: hypotheses change under 1e-4 noise (seed {seed}); pick another seed"
                for i in range(len(res[0])):      # the second-best hypothesis too (topk_scores' order)
                    assert torch.argsort(again[1][i], descending=True).tolist() == \
                        torch.argsort(res[1][i], descending=True).tolist(), name
            out[f"search.{name}.cfg"] = np.array(json.dumps(cfg))
            out[f"search.{name}.pred"] = _pad(res[0], -1, np.int64)
            out[f"search.{name}.scores"] = res[1].numpy()
            if cfg.get("return_log_probs"):
                out[f"search.{name}.log_probs"] = _pad([lp.tolist() for lp in res[2]], np.nan, np.float32)
            preds[name] = res[0]
            print(f"search.{name}: lengths {[len(p) for p in res[0]]}, stable")
        assert preds["w0.4_full"] != preds["w0.0_full"] or preds["w0.4_full"] != preds["w1.0_full"]
        greedy = _RefGreedy([tr, seq_lin], bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0)
        gp, gs = greedy(enc.clone(), wav_len)
        out["greedy.pred"] = _pad(gp, -1, np.int64)
        out["greedy.scores"] = np.array(gs, dtype=np.float32)
    print(f"search model: {n_par} parameters")


# ------------------------------------------------- signatures, pure helpers
PUBLIC = {
    "ctc.CTCPrefixScorer": RC.CTCPrefixScorer, "ctc.CTCPrefixScorer.forward_step": RC.CTCPrefixScorer.forward_step,
    "ctc.CTCPrefixScorer.permute_mem": RC.CTCPrefixScorer.permute_mem,
    "ctc.ctc_greedy_decode": RC.ctc_greedy_decode, "ctc.filter_ctc_output": RC.filter_ctc_output,
    "seq2seq.S2SBaseSearcher": RS.S2SBaseSearcher, "seq2seq.S2SGreedySearcher": RS.S2SGreedySearcher,
    "seq2seq.S2SBeamSearcher": RS.S2SBeamSearcher, "seq2seq.S2STransformerBeamSearch": RS.S2STransformerBeamSearch,
    "seq2seq.S2SBaseSearcher.forward": RS.S2SBaseSearcher.forward,
    "seq2seq.S2SBaseSearcher.forward_step": RS.S2SBaseSearcher.forward_step,
    "seq2seq.inflate_tensor": RS.inflate_tensor, "seq2seq.mask_by_condition": RS.mask_by_condition,
    "seq2seq.batch_filter_seq2seq_output": RS.batch_filter_seq2seq_output,
    "seq2seq.filter_seq2seq_output": RS.filter_seq2seq_output,
}


def gen_signatures(out):
    sigs = {}
    for name, obj in PUBLIC.items():
        sigs[name] = [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
                      for p in inspect.signature(obj).parameters.values()]
    out["signatures"] = np.array(json.dumps(sigs))
    filters = []
    for inp, eos in ((["a", "b", "c", "d", "eos", "e"], "eos"), ([5, 2, 7, 2], 2), ([4, 4, 4], 9), ([], 2), ([2], 2)):
        filters.append(["filter_seq2seq_output", inp, eos, RS.filter_seq2seq_output(list(inp), eos_id=eos)])
    for inp, blank in ((["a", "a", "blank", "b", "b", "blank", "c"], "blank"), ([0, 0, 3, 3, 0, 3, 1, 1], 0),
                       ([2, 2, 2], 2), ([], 0), ([5, 0, 5, 5, 0, 0, 6], 0)):
        filters.append(["filter_ctc_output", inp, blank, RC.filter_ctc_output(list(inp), blank_id=blank)])
    out["filters"] = np.array(json.dumps(filters))


if __name__ == "__main__":
    out = {}
    gen_scorer(out)
    gen_search(out)
    gen_signatures(out)
    path = os.path.join(OUT, "s2s.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
