"""csrc/gru.hip through the drop-ins speechbrain_amd.nnet.RNN.GRU and
speechbrain_amd.nnet.embedding.Embedding, against the float64 restatement of
tests/rnn_ref.py (held to the reference's fixture by test_rnn_cpu.py).

Shapes.  The forward / backward step kernels give a workgroup 16 hidden units
and up to 32 batch rows, deal K to eight waves in chunks of 32 (256 per round)
and read 8 K elements per lane, vectorised when H % 4 == 0 (fp32).  The sweep
therefore takes H in {5, 15, 16, 17, 20, 64, 72, 264} (below / at / past a
slice, a K tail inside a chunk, two chunks, a K that is no multiple of 32, and
264: a second round of chunks with a tail of 8, four rounds in the backward's
K = 3H), B in {1, 3, 17, 33, 65} (33: a second batch group of one row, 65: a
third), T in {1, 2, 7} and I in {1, 19, 32} (19: 76-byte rows, a misaligned K
tail of the input GEMM), rotated over thirteen shapes so that every value
occurs; each shape runs the eight combinations of
hx / bias / ragged lengths (with a one-frame row where B > 1), forward and
backward, the loss being sum(output · P) + sum(hn · Q).

Guard bands.  x, hx, the token ids' embedding and every parameter are views
into larger device buffers whose other elements are NaN (as
test_gpu_selfattn_paths.py); the buffers of the variants without hx start one
element off 16-byte alignment, which sends the kernels down their scalar
loads.  A read outside an operand that reaches arithmetic comes out as NaN and
is reported before any comparison.

Bounds.  Inputs are N(0, 1), weights N(0, 1) / sqrt(H), so no gate saturates.
fp32: per tensor max |err| / max(1, |ref|_inf) <= max(1e-5, 8 * E32), E32 the
same figure for torch's own fp32 CPU nn.GRU against the float64 restatement on
the same case (the rule of test_gpu_selfattn_paths.py); the fixture cases also
meet 1e-4.  bf16 (autocast): the yardstick is the float64 restatement with
W_ih, W_hh and the h_{t-1} operand rounded to bf16; the kernel stays within
2 * (that restatement's deviation from the unrounded one) + 1e-5 of it.
"""
import json
import zlib

import numpy as np
import pytest
import torch

import rnn_ref as R

gpu = pytest.mark.gpu
NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


# ------------------------------------------------------------------ cases
def make_spec(H, B, T, I, L=1, bias=True, hx=True, ragged=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = []
    for l in range(L):
        i = I if l == 0 else H
        params.append((torch.randn(3 * H, i, generator=g) / H ** 0.5, torch.randn(3 * H, H, generator=g) / H ** 0.5,
                       torch.randn(3 * H, generator=g) / H ** 0.5 if bias else None,
                       torch.randn(3 * H, generator=g) / H ** 0.5 if bias else None))
    s = dict(params=params, x=torch.randn(B, T, I, generator=g),
             hx=torch.randn(L, B, H, generator=g) if hx else None, steps=None, lengths=None)
    if ragged:
        steps = torch.randint(1, T + 1, (B,), generator=g)
        steps[0] = T if B > 1 else max(1, T - 1)
        if B > 1:
            steps[B - 1] = 1
        s["steps"] = steps
        s["lengths"] = (steps.float() + 0.5) / T       # int(lengths * T) == steps whatever the rounding
        assert R.steps_of(s["lengths"], T).tolist() == steps.tolist()
    Tn = T if s["steps"] is None else int(s["steps"].max())
    s["proj"] = torch.randn(B, Tn, H, generator=g)
    s["projh"] = torch.randn(L, B, H, generator=g)
    return s


def _collect(out, hn, params, x, hx):
    res = {"out": out.detach(), "hn": hn.detach()}
    for l, ps in enumerate(params):
        for n, p in zip(NAMES, ps):
            if p is not None and p.grad is not None:
                res[f"d{n}_l{l}"] = p.grad
    if x is not None and x.grad is not None:
        res["dx"] = x.grad
    if hx is not None:
        res["dhx"] = hx.grad
    return {k: v.detach().double().cpu() for k, v in res.items()}


def run_ref64(s, round_bf16=False, xin=None):
    f64 = torch.float64
    params = [tuple(None if p is None else p.to(f64).clone().requires_grad_(True) for p in ps) for ps in s["params"]]
    x = (s["x"] if xin is None else xin).to(f64).clone().requires_grad_(xin is None)
    hx = None if s["hx"] is None else s["hx"].to(f64).clone().requires_grad_(True)
    out, hn = R.gru_ref(x, params, hx, s["steps"], round_bf16)
    ((out * s["proj"].to(f64)).sum() + (hn * s["projh"].to(f64)).sum()).backward()
    return _collect(out, hn, params, x if xin is None else None, hx)


def run_torch32(s):
    """torch's own fp32 CPU nn.GRU (packed where the case has lengths)."""
    H, I = s["params"][0][1].shape[1], s["params"][0][0].shape[1]
    L, bias = len(s["params"]), s["params"][0][2] is not None
    m = torch.nn.GRU(I, H, L, bias=bias, batch_first=True)
    with torch.no_grad():
        for l, ps in enumerate(s["params"]):
            for n, p in zip(NAMES, ps):
                if p is not None:
                    getattr(m, f"{n}_l{l}").copy_(p)
    x = s["x"].clone().requires_grad_(True)
    hx = None if s["hx"] is None else s["hx"].clone().requires_grad_(True)
    inp = x
    if s["steps"] is not None:
        inp = torch.nn.utils.rnn.pack_padded_sequence(x, s["steps"], batch_first=True, enforce_sorted=False)
    out, hn = m(inp, hx)
    if s["steps"] is not None:
        out = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True)[0]
    ((out * s["proj"]).sum() + (hn * s["projh"]).sum()).backward()
    params = [tuple(getattr(m, f"{n}_l{l}", None) for n in NAMES) for l in range(L)]
    return _collect(out, hn, params, x, hx)


def _guard(t, dev, front=64, dtype=None):
    """t as a view into a larger device buffer whose other elements are NaN
    (token ids: -7, an id no table has)."""
    dtype = dtype or t.dtype
    fill = float("nan") if dtype.is_floating_point else -7
    buf = torch.full((front + t.numel() + 64,), fill, device=dev, dtype=dtype)
    v = buf[front:front + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def build_gpu(s, dev, front=64):
    from speechbrain_amd.nnet.RNN import GRU
    H, I = s["params"][0][1].shape[1], s["params"][0][0].shape[1]
    m = GRU(H, input_size=I, num_layers=len(s["params"]), bias=s["params"][0][2] is not None).to(dev)
    for l, ps in enumerate(s["params"]):
        for n, p in zip(NAMES, ps):
            if p is not None:
                getattr(m.rnn, f"{n}_l{l}").data = _guard(p, dev, front)
    return m


def run_gpu(s, dev, front=64, autocast=False, module=None, xin=None):
    """xin: an already embedded (tagged) input; else s["x"] inside guard bands."""
    m = module or build_gpu(s, dev, front)
    for p in m.parameters():
        p.grad = None
    x = _guard(s["x"], dev, front).requires_grad_(True) if xin is None else xin
    hx = None if s["hx"] is None else _guard(s["hx"], dev, front).requires_grad_(True)
    lengths = None if s["lengths"] is None else s["lengths"].to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out, hn = m(x, hx=hx, lengths=lengths)
    assert out.dtype == torch.float32 and hn.dtype == torch.float32
    ((out * s["proj"].to(dev)).sum() + (hn * s["projh"].to(dev)).sum()).backward()
    params = [tuple(getattr(m.rnn, f"{n}_l{l}", None) for n in NAMES) for l in range(len(s["params"]))]
    return _collect(out, hn, params, x if xin is None else None, hx)


def rel_err(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def check_fp32(got, ref, t32, what, extra=None):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert bool(torch.isfinite(got[k]).all()), f"{what} {k}: NaN / inf (a read outside an operand?)"
        bound = max(1e-5, 8 * rel_err(t32[k], ref[k])) if k in t32 else 1e-5
        if extra is not None:
            bound = min(bound, extra)
        e = rel_err(got[k], ref[k])
        assert e <= bound, f"{what} {k}: {e:.3e} > {bound:.3e}"


# (H, B, T, I): every H, B, T and I of the module docstring occurs
SHAPES = [(5, 1, 1, 1), (15, 3, 2, 19), (16, 17, 7, 32), (17, 33, 7, 19), (20, 65, 2, 1), (64, 3, 7, 32),
          (72, 33, 7, 19), (72, 17, 1, 32), (64, 1, 2, 1), (20, 3, 7, 19), (16, 33, 1, 1), (5, 17, 2, 32),
          (264, 3, 2, 1)]


# ------------------------------------------------------------------ fixture
@gpu
def test_fixture_cases(dev, golden):
    from speechbrain_amd.nnet.RNN import GRU
    from speechbrain_amd.nnet.embedding import Embedding
    g = golden("rnn")
    for name in g["case.names"]:
        key = f"case.{name}."
        kw = json.loads(str(g[key + "kw"]))
        if "input_shape" in kw:
            kw["input_shape"] = tuple(kw["input_shape"])
        m = GRU(**kw)
        m.load_state_dict({k[len(key) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(key + "sd.")},
                          strict=True)
        m = m.to(dev)
        L = kw.get("num_layers", 1)
        sd = {k[len(key) + 3:]: g[k] for k in g.files if k.startswith(key + "sd.")}
        params = [tuple(torch.from_numpy(sd[f"rnn.{n}_l{l}"]) for n in NAMES) for l in range(L)]
        hx = torch.from_numpy(g[key + "hx"]).to(dev).requires_grad_(True) if key + "hx" in g.files else None
        lengths = torch.from_numpy(g[key + "lengths"]).to(dev) if key + "lengths" in g.files else None
        if name == "onehot":
            emb = Embedding(**json.loads(str(g[key + "emb_kw"]))).to(dev)
            x = emb(torch.from_numpy(g[key + "tokens"]).to(dev))
            assert hasattr(x, "_sbk_onehot")
            x64 = R.onehot_table(7, 3)[torch.from_numpy(g[key + "tokens"])].float()
        else:
            x = torch.from_numpy(g[key + "x"]).to(dev).requires_grad_(True)
            x64 = torch.from_numpy(g[key + "x"]).reshape(x.shape[0], x.shape[1], -1)
        out, hn = m(x, hx=hx, lengths=lengths)
        (out * torch.from_numpy(g[key + "proj"]).to(dev)).sum().backward()
        got = {"out": out, "hn": hn}
        want = {"out": g[key + "out"], "hn": g[key + "hn"]}
        for k, p in m.named_parameters():
            got["grad." + k], want["grad." + k] = p.grad, g[key + "grad." + k]
        if name != "onehot":
            got["grad.x"], want["grad.x"] = x.grad, g[key + "grad.x"]
        if hx is not None:
            got["grad.hx"], want["grad.hx"] = hx.grad, g[key + "grad.hx"]
        # E32 of this case: torch's fp32 CPU GRU (the fixture itself) against the float64 restatement
        s = dict(params=params, x=x64, hx=None if hx is None else torch.from_numpy(g[key + "hx"]),
                 steps=None if lengths is None else torch.from_numpy(g[key + "steps"]), lengths=None,
                 proj=torch.from_numpy(g[key + "proj"]), projh=torch.zeros(L, x.shape[0], kw["hidden_size"]))
        ref = run_ref64(s)
        ren = {"out": "out", "hn": "hn", "grad.x": "dx", "grad.hx": "dhx"}
        for k in want:
            r = ref[ren.get(k, "d" + k[len("grad.rnn."):])]
            w = torch.from_numpy(np.asarray(want[k])).double().reshape(r.shape)
            bound = min(1e-4, max(1e-5, 8 * rel_err(w, r)))
            v = got[k].detach().double().cpu().reshape(r.shape)
            assert bool(torch.isfinite(v).all()), (name, k)
            assert rel_err(v, w) <= bound, f"{name} {k}: {rel_err(v, w):.3e} > {bound:.3e}"


# ------------------------------------------------------------------ edge sweep
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d_B%d_T%d_I%d" % s)
def test_edge_sweep_fp32(dev, shape):
    H, B, T, I = shape
    for hx in (True, False):
        for bias in (True, False):
            for ragged in (False, True):
                what = f"H{H} B{B} T{T} I{I} hx{int(hx)} bias{int(bias)} ragged{int(ragged)}"
                s = make_spec(H, B, T, I, 1, bias, hx, ragged, seed=zlib.crc32(what.encode()))
                got = run_gpu(s, dev, front=64 if hx else 65)
                check_fp32(got, run_ref64(s), run_torch32(s), what)


@gpu
def test_two_layers_ragged_fp32(dev):
    s = make_spec(20, 5, 7, 19, L=2, bias=True, hx=True, ragged=True, seed=5)
    check_fp32(run_gpu(s, dev), run_ref64(s), run_torch32(s), "two layers")


@gpu
def test_interlayer_dropout_runs_in_training_only(dev):
    from speechbrain_amd.nnet.RNN import GRU
    torch.manual_seed(0)
    m = GRU(16, input_size=8, num_layers=2, dropout=0.5).to(dev)
    x = torch.randn(3, 4, 8, device=dev)
    m.eval()
    a, b = m(x)[0], m(x)[0]
    assert torch.equal(a, b)
    m.train()
    c = m(x)[0]
    assert bool(torch.isfinite(c).all()) and not torch.equal(a, c)


# ------------------------------------------------------------------ one-hot path
def _tokens(V, blank, B, U, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, V, (B, U), generator=g)
    tok[:, 0] = blank
    tok[1] = blank                       # a row that is all blank
    tok[2, 1:4] = tok[2, 1]              # a token repeated within a row
    tok[0, 2] = tok[2, 1]                # ... and across rows of the batch
    return tok


@gpu
@pytest.mark.parametrize("V", [7, 40])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_onehot_path(dev, V, where, idt):
    from speechbrain_amd.nnet.embedding import Embedding
    blank = {"first": 0, "middle": V // 2, "last": V - 1}[where]
    B, U, H = 4, 6, 20
    tok = _tokens(V, blank, B, U, seed=V + blank)
    s = make_spec(H, B, U, V - 1, 1, True, True, False, seed=100 + V + blank)
    x64 = R.onehot_table(V, blank)[tok]
    s["x"] = x64.float()
    ref, t32 = run_ref64(s), run_torch32(s)
    ref.pop("dx")
    emb = Embedding(V, consider_as_one_hot=True, blank_id=blank).to(dev)
    m = build_gpu(s, dev)
    e = emb(_guard(tok.to(idt), dev, dtype=idt))
    assert torch.equal(e.cpu().double(), x64)                 # the dense rows any other consumer reads
    e.data.fill_(float("nan"))                                # the tagged path never reads them (no version bump)
    hot = run_gpu(s, dev, module=m, xin=e)
    check_fp32(hot, ref, t32, f"one-hot V{V} blank{blank}")
    # modified in place: the tag is stale, the GRU takes the dense path
    e2 = emb(tok.to(dev).to(idt))
    e2.mul_(1.0)
    dense = run_gpu(s, dev, module=m, xin=e2)
    check_fp32(dense, ref, t32, f"dense after in-place V{V} blank{blank}")
    for k in ref:
        bound = max(1e-5, 8 * rel_err(t32[k], ref[k]))
        assert rel_err(hot[k], dense[k]) <= bound, (k, rel_err(hot[k], dense[k]), bound)


@gpu
def test_onehot_path_is_deterministic(dev):
    """H 20, B 3, T 7, no dense dW_ih GEMM: two forward + backward runs are bit-identical."""
    from speechbrain_amd.nnet.embedding import Embedding
    V, blank, H, B, T = 40, 0, 20, 3, 7
    tok = _tokens(V, blank, B, T, seed=3).to(dev)
    s = make_spec(H, B, T, V - 1, 1, True, True, False, seed=9)
    emb = Embedding(V, consider_as_one_hot=True, blank_id=blank).to(dev)
    m = build_gpu(s, dev)
    a = run_gpu(s, dev, module=m, xin=emb(tok))
    b = run_gpu(s, dev, module=m, xin=emb(tok))
    for k in ("out", "hn", "dhx", "dweight_ih_l0", "dbias_ih_l0", "dbias_hh_l0"):
        assert torch.equal(a[k], b[k]), k


@gpu
def test_decode_steps_equal_sequence(dev):
    """T = 1 calls with hx given reproduce the full-sequence output bit for bit (fp32)."""
    s = make_spec(20, 3, 7, 19, 1, True, True, False, seed=11)
    m = build_gpu(s, dev)
    x, hx = s["x"].to(dev), s["hx"].to(dev)
    with torch.no_grad():
        full, hn = m(x, hx=hx)
        h, outs = hx, []
        for t in range(7):
            o, h = m(x[:, t:t + 1], hx=h)
            outs.append(o)
    assert torch.equal(torch.cat(outs, 1), full) and torch.equal(h, hn)


# ------------------------------------------------------------------ bf16
@gpu
@pytest.mark.parametrize("shape", [(72, 33, 7, 32), (20, 3, 7, 19)], ids=lambda s: "H%d_B%d_T%d_I%d" % s)
def test_bf16_against_rounded_restatement(dev, shape):
    """Largest case (H 72, B 33, T 7, I 32), forward tensors, measured on an
    MI355X: see DESIGN.md (GRU section)."""
    H, B, T, I = shape
    s = make_spec(H, B, T, I, 1, True, True, True, seed=21)
    exact, yard = run_ref64(s), run_ref64(s, round_bf16=True)
    got = run_gpu(s, dev, autocast=True)
    for k in exact:
        dev_k = rel_err(yard[k], exact[k])
        e = rel_err(got[k], yard[k])
        print(f"bf16 H{H} B{B} T{T} I{I} {k}: restatement deviation {dev_k:.3e}, kernel error {e:.3e}")
    for k in exact:
        assert bool(torch.isfinite(got[k]).all()), k
        bound = 2 * rel_err(yard[k], exact[k]) + 1e-5
        assert rel_err(got[k], yard[k]) <= bound, f"{k}: {rel_err(got[k], yard[k]):.3e} > {bound:.3e}"


# ------------------------------------------------------------------ trainable Embedding
@gpu
def test_trainable_embedding(dev):
    from speechbrain_amd.nnet.embedding import Embedding
    torch.manual_seed(3)
    V, D = 11, 19
    emb = Embedding(V, embedding_dim=D).to(dev)
    ref = torch.nn.Embedding(V, D)
    with torch.no_grad():
        ref.weight.copy_(emb.Embedding.weight.cpu())
    emb.Embedding.weight.data = _guard(ref.weight.detach(), dev)
    ids = torch.tensor([[1, 1, 4, 10, 0], [4, 4, 4, 1, 7]])
    proj = torch.randn(2, 5, D)
    runs = []
    for idt in (torch.int64, torch.int32):
        emb.Embedding.weight.grad = None
        y = emb(_guard(ids.to(idt), dev, dtype=idt))
        (y * proj.to(dev)).sum().backward()
        runs.append((y.detach().cpu(), emb.Embedding.weight.grad.cpu()))
    yr = ref(ids)
    (yr * proj).sum().backward()
    assert torch.equal(runs[0][0], yr.detach())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert rel_err(runs[0][1].double(), ref.weight.grad.double()) <= 1e-6
