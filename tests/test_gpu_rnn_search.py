"""The RNN beam searchers and the beam-grouped decoder step (sbk_attdec_beam_step,
_attsearch.BeamState).  One grouped step, two steps deep, against a float64
restatement of the reference's step on index_select-ed state, bounds as
tests/test_gpu_attdec.py: fp32 max(1e-5, 8 * E32) per tensor, bf16 (autocast)
2 * the bf16-rounded restatement's deviation + 1e-5.  Whole searches against
tests/golden/rnn_search.npz (the reference's CPU searchers): hypotheses
exactly, scores at 1e-4 * max(1, |ref|), with USE_BEAM_STEP on and off; largest
score deviation observed on an MI355X over all cases: 5.3e-7."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from test_gpu_attdec import rel_err

pytestmark = pytest.mark.gpu
GH = 16   # hypotheses of a beam-score workgroup (sbk_attdec_beam_group; checked in test_grouped_step)
H, I, V = 7, 6, 9
KEYS = ("dec_out", "h", "c", "attn", "cov", "pen")


def restate(p, embw, enc, lens, G, kind, scaling, ksz, tokens, parents, shift, bf16=False):
    """Two steps of the reference's search state in plain torch ops, in the dtype of enc."""
    def r(t):
        return t.bfloat16().to(t.dtype) if bf16 else t
    (B, L, _), N = enc.shape, enc.shape[0] * G
    rep = lambda t: torch.repeat_interleave(t, G, dim=0)  # noqa: E731
    valid = rep(torch.arange(L)[None] < lens[:, None])
    P = rep(r(enc) @ r(p["attn.mlp_enc.weight"]).T + p["attn.mlp_enc.bias"])
    encN = rep(enc)
    h, c = enc.new_zeros(N, H), enc.new_zeros(N, P.shape[-1])
    prev, cov, peak = valid.to(enc.dtype) / rep(lens)[:, None], None, torch.zeros(N, dtype=torch.long)
    steps = []
    for s, (tok, idx) in enumerate(zip(tokens, parents)):
        h, c, prev, peak0 = h[idx], c[idx], prev[idx], peak[idx]
        x = torch.cat([embw[tok], c], 1)
        gi = r(x) @ r(p["rnn.rnn_cells.0.weight_ih"]).T + p["rnn.rnn_cells.0.bias_ih"]
        gh = r(h) @ r(p["rnn.rnn_cells.0.weight_hh"]).T + p["rnn.rnn_cells.0.bias_hh"]
        (ir, iz, inn), (hr, hz, hn) = gi.chunk(3, 1), gh.chunk(3, 1)
        rg, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
        h = (1 - z) * torch.tanh(inn + rg * hn) + z * h
        e = P + (r(h) @ r(p["attn.mlp_dec.weight"]).T + p["attn.mlp_dec.bias"])[:, None]
        if kind == "location":
            loc = F.conv1d(prev[:, None], p["attn.conv_loc.weight"], padding=ksz).transpose(1, 2)
            e = e + loc @ p["attn.mlp_loc.weight"].T + p["attn.mlp_loc.bias"]
        sc = (torch.tanh(e) @ p["attn.mlp_attn.weight"].T).squeeze(-1) * scaling
        prev = torch.softmax(sc.masked_fill(~valid, float("-inf")), -1)
        c = r(torch.bmm(prev[:, None], encN)[:, 0]) @ r(p["attn.mlp_out.weight"]).T + p["attn.mlp_out.bias"]
        out = r(torch.cat([c, h], 1)) @ r(p["proj.weight"]).T + p["proj.bias"]
        peak = prev.max(1)[1]
        ok = (peak <= peak0 + shift) & (peak > peak0 - shift)
        cov = 2 * prev if s == 0 else cov[idx] + prev     # the reference's step-0 rule
        pen = torch.clamp(cov, min=0.5).sum(-1) - 0.5 * L
        steps.append(dict(dec_out=out, h=h, c=c, attn=prev, cov=cov, pen=pen, peak=peak, ok=ok, d=peak - peak0))
    return steps


def make_case(kind, L, G, B, ksz, C, A, E, scaling, seed=0):
    from speechbrain_amd.nnet.RNN import AttentionalRNNDecoder
    g = torch.Generator().manual_seed(seed)
    m = AttentionalRNNDecoder("gru", kind, H, A, 1, E, I, scaling=scaling, channels=C, kernel_size=ksz)
    p = {k: torch.randn(v.shape, generator=g) / (v.shape[-1] ** 0.5 if v.dim() > 1 else 4.0)
         for k, v in m.state_dict().items()}
    m.load_state_dict(p, strict=True)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    if B > 1:
        lens[-1] = 1      # a one-frame utterance
    N = B * G
    base = torch.arange(N) // G * G
    parents = [torch.arange(N), base + torch.randint(0, G, (N,), generator=g)]   # repeats, crossings, own utterance
    tokens = [torch.randint(0, V, (N,), generator=g) for _ in range(2)]
    s = dict(m=m, p=p, kind=kind, G=G, scaling=scaling, ksz=ksz, lens=lens, parents=parents, tokens=tokens,
             embw=torch.randn(V, I, generator=g), enc=torch.randn(B, L, E, generator=g))
    d = torch.cat([st["d"].abs() for st in run_ref(s, torch.float64, 0)])
    free = [k for k in range(1, L + 4) if int((d - k).abs().min()) >= 2]
    s["shift"] = free[0]   # at least 2 away from every |peak - prev_peak|, blocking something where it can
    return s


def run_ref(s, dtype, shift=None, bf16=False):
    p = {k: v.to(dtype) for k, v in s["p"].items()}
    return restate(p, s["embw"].to(dtype), s["enc"].to(dtype), s["lens"], s["G"], s["kind"], s["scaling"], s["ksz"],
                   s["tokens"], s["parents"], s["shift"] if shift is None else shift, bf16)


def run_gpu(s, dev, autocast=False):
    from speechbrain_amd import _attsearch
    m = s["m"].to(dev).eval()
    emb = torch.nn.Embedding(V, I).to(dev)
    emb.weight.data.copy_(s["embw"])
    steps = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        st = _attsearch.BeamState(m, emb, s["enc"].to(dev), s["lens"].to(dev), s["G"], s["shift"])
        for tok, idx in zip(s["tokens"], s["parents"]):
            st.permute(idx.to(dev))
            out, attn = st.step(tok.to(dev))
            got = dict(dec_out=out, h=st.h, c=st.c, attn=attn, cov=st.cov, pen=st.pen, peak=st.peak, ok=st.shift_ok)
            steps.append({k: v.detach().double().cpu() for k, v in got.items()})
    return steps


SWEEP = [("location", 1, 1, 1, 1, 1, 5, 20, 1.0),
         ("location", 31, GH - 1, 3, 3, 10, 72, 24, 2.0),
         ("location", 32, GH, 3, 100, 17, 5, 70, 1.0),
         ("location", 33, GH + 1, 1, 3, 10, 72, 20, 2.0),
         ("location", 65, 2 * GH + 1, 3, 100, 10, 5, 24, 1.0),
         ("location", 33, GH, 3, 1, 17, 72, 70, 2.0),
         ("location", 65, 1, 3, 3, 1, 5, 20, 2.0),
         ("location", 32, GH + 1, 1, 1, 10, 72, 24, 1.0),
         ("content", 65, 2 * GH + 1, 3, None, None, 72, 70, 1.0),
         ("content", 1, GH - 1, 3, None, None, 5, 20, 2.0),
         ("content", 32, GH, 1, None, None, 72, 24, 1.0),
         ("content", 31, GH + 1, 3, None, None, 5, 70, 2.0)]
_ID = lambda c: "%s_L%d_G%d_B%d_k%s_C%s_A%d_E%d_s%g" % c  # noqa: E731  (kind, L, G, B, ksz, C, A, E, scaling)


@pytest.mark.parametrize("case", SWEEP, ids=_ID)
def test_grouped_step(dev, case):
    from speechbrain_amd import _attsearch
    assert _attsearch.group() == GH
    s = make_case(*case)
    got, ref, t32 = run_gpu(s, dev), run_ref(s, torch.float64), run_ref(s, torch.float32)
    pad = torch.repeat_interleave(torch.arange(case[1])[None] >= s["lens"][:, None], s["G"], dim=0)
    for i, (g, r, t) in enumerate(zip(got, ref, t32)):
        assert bool((g["attn"][pad] == 0).all()), "attn at padded frames"
        assert float((g["attn"].sum(-1) - 1).abs().max()) <= 1e-5
        for k in KEYS:
            e, bound = rel_err(g[k], r[k].double()), max(1e-5, 8 * rel_err(t[k].double(), r[k].double()))
            print(f"{_ID(case)} step {i} {k}: err {e:.3e}, bound {bound:.3e}")
            assert bool(torch.isfinite(g[k]).all()) and e <= bound, f"step {i} {k}: {e:.3e} > {bound:.3e}"
        assert torch.equal(g["peak"].long(), r["peak"]), f"step {i} peak"
        assert torch.equal(g["ok"].bool(), r["ok"]), f"step {i} shift_ok (shift {s['shift']})"


@pytest.mark.parametrize("case", [SWEEP[2], SWEEP[3], SWEEP[8]], ids=_ID)
def test_grouped_step_bf16(dev, case):
    s = make_case(*case, seed=3)
    exact, yard, got = run_ref(s, torch.float64), run_ref(s, torch.float64, bf16=True), run_gpu(s, dev, autocast=True)
    for i, (g, x, y) in enumerate(zip(got, exact, yard)):
        for k in KEYS:
            e, bound = rel_err(g[k], y[k]), 2 * rel_err(y[k], x[k]) + 1e-5
            print(f"bf16 {_ID(case)} step {i} {k}: restatement deviation {rel_err(y[k], x[k]):.3e}, kernel {e:.3e}")
            assert bool(torch.isfinite(g[k]).all()) and e <= bound, f"step {i} {k}: {e:.3e} > {bound:.3e}"


CASES = ["location", "content", "cov_shift", "no_lennorm", "ctc_full", "greedy", "gru_lm", "tlm"]


@pytest.fixture(scope="module")
def setup(golden, dev):
    from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.RNN import AttentionalRNNDecoder
    from rnn_search_common import build_modules
    g, m = golden("rnn_search"), build_modules(AttentionalRNNDecoder, Embedding, Linear, TransformerLM)
    for name, mod in m.items():
        pre = f"sd.{name}."
        sd = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
        if name == "tlm":     # the sine table is a buffer, not a weight
            sd["positional_encoding.pe"] = mod.state_dict()["positional_encoding.pe"]
        mod.load_state_dict(sd, strict=True)
        mod.to(dev).eval()
    return g, m


def _search_and_check(g, m, name, dev, beam_step, what):
    from rnn_search_common import make_searcher
    from speechbrain_amd import decoders
    searcher = make_searcher(decoders, m, json.loads(str(g[f"{name}.cfg"])))
    searcher.USE_BEAM_STEP = beam_step
    res = searcher(torch.from_numpy(g[f"{name}.enc"]).to(dev), torch.from_numpy(g["wav_len"]).to(dev))
    assert res[0] == [row[row != -1].tolist() for row in g[f"{name}.pred"]], name
    ref = g[f"{name}.scores"]
    got = np.asarray(torch.as_tensor(res[1]).cpu().numpy(), dtype=np.float32)
    print(f"{name} ({what}): scores max deviation {float(np.max(np.abs(got - ref) / np.maximum(1, np.abs(ref)))):.3e}")
    assert_close(got, ref, name=f"{name}.scores")


@pytest.mark.parametrize("beam_step", [True, False], ids=["grouped", "reference_step"])
@pytest.mark.parametrize("name", CASES)
def test_search_matches_reference(setup, dev, name, beam_step):
    g, m = setup
    assert g["names"].tolist() == CASES
    _search_and_check(g, m, name, dev, beam_step, "grouped" if beam_step else "reference step")


def test_search_on_a_side_stream(setup, dev):
    g, m = setup
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _search_and_check(g, m, "cov_shift", dev, True, "side stream")
    side.synchronize()

