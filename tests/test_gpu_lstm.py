"""csrc/lstm.hip through the drop-in speechbrain_amd.nnet.RNN.LSTM, against the
float64 restatement of tests/lstm_ref.py (held to the reference's fixture and
to torch's packed float64 LSTM by test_lstm_cpu.py).  The method is that of
test_gpu_rnn.py.

Shapes.  The forward / backward step kernels give a workgroup 16 hidden units
of one direction and up to 32 batch rows, deal K to eight waves in chunks of
32 (256 per round) and read 8 K elements per lane, vectorised when H % 4 == 0
(fp32).  The sweep therefore takes H in {5, 15, 16, 17, 20, 64, 72, 264}
(below / at / past a slice, a K tail inside a chunk, two chunks, a K that is
no multiple of 32, and 264: a second round of chunks with a tail of 8 in the
forward, K = 4H = 1056 in the backward: four rounds of chunks plus a tail), B
in {1, 3, 17, 33, 65} (33: a second batch group of one row, 65: a third), T
in {1, 2, 7} and I in {1, 19, 32} (19: 76-byte rows, a misaligned K tail of
the input GEMM), rotated over thirteen shapes so that every value occurs; each
shape runs the sixteen combinations of D in {1, 2} / hx / bias / ragged lengths
(with a full row and a one-frame row where B > 1), forward and backward, the
loss being sum(output · P) + sum(hn · Q) + sum(cn · R), so that dc0 and the cn
path are live.

Guard bands.  x, (h0, c0) and every parameter are views into larger device
buffers whose other elements are NaN; the buffers of the variants without hx
start one element off 16-byte alignment, which sends the kernels down their
scalar loads.  A read outside an operand that reaches arithmetic comes out as
NaN and is reported before any comparison.

Bounds.  Inputs are N(0, 1), weights N(0, 1) / sqrt(H), so no gate saturates.
fp32: per tensor max |err| / max(1, |ref|_inf) <= max(1e-5, 8 * E32), E32 the
same figure for torch's own fp32 CPU nn.LSTM (packed where ragged) against the
float64 restatement on the same case; the fixture cases also meet 1e-4.  bf16
(autocast): the yardstick is the float64 restatement with W_ih, W_hh and the h
operand rounded to bf16; the kernel stays within 2 * (that restatement's
deviation from the unrounded one) + 1e-5 of it.
"""
import json
import zlib

import numpy as np
import pytest
import torch

import lstm_ref as R

gpu = pytest.mark.gpu
NAMES = R.NAMES
SFX = ("", "_reverse")


# ------------------------------------------------------------------ cases
def make_spec(H, B, T, I, L=1, D=1, bias=True, hx=True, ragged=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = []
    for l in range(L):
        i = I if l == 0 else D * H
        params.append([(torch.randn(4 * H, i, generator=g) / H ** 0.5, torch.randn(4 * H, H, generator=g) / H ** 0.5,
                        torch.randn(4 * H, generator=g) / H ** 0.5 if bias else None,
                        torch.randn(4 * H, generator=g) / H ** 0.5 if bias else None) for _ in range(D)])
    s = dict(params=params, x=torch.randn(B, T, I, generator=g),
             hx=(torch.randn(L * D, B, H, generator=g), torch.randn(L * D, B, H, generator=g)) if hx else None,
             steps=None, lengths=None)
    if ragged:
        steps = torch.randint(1, T + 1, (B,), generator=g)
        steps[0] = T if B > 1 else max(1, T - 1)
        if B > 1:
            steps[B - 1] = 1
        s["steps"] = steps
        s["lengths"] = (steps.float() + 0.5) / T       # int(lengths * T) == steps whatever the rounding
        assert R.steps_of(s["lengths"], T).tolist() == steps.tolist()
    Tn = T if s["steps"] is None else int(s["steps"].max())
    s["proj"] = torch.randn(B, Tn, D * H, generator=g)
    s["projh"] = torch.randn(L * D, B, H, generator=g)
    s["projc"] = torch.randn(L * D, B, H, generator=g)
    return s


def _collect(out, hn, cn, params, x, hx):
    res = {"out": out.detach(), "hn": hn.detach(), "cn": cn.detach()}
    for l, dirs in enumerate(params):
        for d, ps in enumerate(dirs):
            for n, p in zip(NAMES, ps):
                if p is not None and p.grad is not None:
                    res[f"d{n}_l{l}{SFX[d]}"] = p.grad
    if x is not None and x.grad is not None:
        res["dx"] = x.grad
    if hx is not None:
        res["dhx"], res["dcx"] = hx[0].grad, hx[1].grad
    return {k: v.detach().double().cpu() for k, v in res.items()}


def _loss(out, hn, cn, s, conv=lambda t: t):
    return (out * conv(s["proj"])).sum() + (hn * conv(s["projh"])).sum() + (cn * conv(s["projc"])).sum()


def run_ref64(s, round_bf16=False, xin=None):
    f64 = torch.float64
    params = [[tuple(None if p is None else p.to(f64).clone().requires_grad_(True) for p in ps) for ps in dirs]
              for dirs in s["params"]]
    x = (s["x"] if xin is None else xin).to(f64).clone().requires_grad_(xin is None)
    hx = None if s["hx"] is None else tuple(h.to(f64).clone().requires_grad_(True) for h in s["hx"])
    out, (hn, cn) = R.lstm_ref(x, params, hx, s["steps"], round_bf16)
    _loss(out, hn, cn, s, lambda t: t.to(f64)).backward()
    return _collect(out, hn, cn, params, x if xin is None else None, hx)


def run_torch32(s):
    """torch's own fp32 CPU nn.LSTM (packed where the case has lengths)."""
    H, I = s["params"][0][0][1].shape[1], s["params"][0][0][0].shape[1]
    L, D, bias = len(s["params"]), len(s["params"][0]), s["params"][0][0][2] is not None
    m = torch.nn.LSTM(I, H, L, bias=bias, batch_first=True, bidirectional=D == 2)
    with torch.no_grad():
        for l, dirs in enumerate(s["params"]):
            for d, ps in enumerate(dirs):
                for n, p in zip(NAMES, ps):
                    if p is not None:
                        getattr(m, f"{n}_l{l}{SFX[d]}").copy_(p)
    x = s["x"].clone().requires_grad_(True)
    hx = None if s["hx"] is None else tuple(h.clone().requires_grad_(True) for h in s["hx"])
    inp = x
    if s["steps"] is not None:
        inp = torch.nn.utils.rnn.pack_padded_sequence(x, s["steps"], batch_first=True, enforce_sorted=False)
    out, (hn, cn) = m(inp, hx)
    if s["steps"] is not None:
        out = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True)[0]
    _loss(out, hn, cn, s).backward()
    params = [[tuple(getattr(m, f"{n}_l{l}{SFX[d]}", None) for n in NAMES) for d in range(D)] for l in range(L)]
    return _collect(out, hn, cn, params, x, hx)


def _guard(t, dev, front=64, dtype=None):
    """t as a view into a larger device buffer whose other elements are NaN
    (token ids: -7, an id no table has)."""
    dtype = dtype or t.dtype
    fill = float("nan") if dtype.is_floating_point else -7
    buf = torch.full((front + t.numel() + 64,), fill, device=dev, dtype=dtype)
    v = buf[front:front + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def build_gpu(s, dev, front=64, dropout=0.0):
    from speechbrain_amd.nnet.RNN import LSTM
    H, I = s["params"][0][0][1].shape[1], s["params"][0][0][0].shape[1]
    m = LSTM(H, input_size=I, num_layers=len(s["params"]), bias=s["params"][0][0][2] is not None,
             bidirectional=len(s["params"][0]) == 2, dropout=dropout).to(dev)
    for l, dirs in enumerate(s["params"]):
        for d, ps in enumerate(dirs):
            for n, p in zip(NAMES, ps):
                if p is not None:
                    getattr(m.rnn, f"{n}_l{l}{SFX[d]}").data = _guard(p, dev, front)
    return m


def run_gpu(s, dev, front=64, autocast=False, module=None, xin=None):
    """xin: an already embedded (tagged) input; else s["x"] inside guard bands."""
    m = module or build_gpu(s, dev, front)
    for p in m.parameters():
        p.grad = None
    x = _guard(s["x"], dev, front).requires_grad_(True) if xin is None else xin
    hx = None if s["hx"] is None else tuple(_guard(h, dev, front).requires_grad_(True) for h in s["hx"])
    lengths = None if s["lengths"] is None else s["lengths"].to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out, (hn, cn) = m(x, hx=hx, lengths=lengths)
    assert out.dtype == torch.float32 and hn.dtype == torch.float32 and cn.dtype == torch.float32
    _loss(out, hn, cn, s, lambda t: t.to(dev)).backward()
    L, D = len(s["params"]), len(s["params"][0])
    params = [[tuple(getattr(m.rnn, f"{n}_l{l}{SFX[d]}", None) for n in NAMES) for d in range(D)] for l in range(L)]
    return _collect(out, hn, cn, params, x if xin is None else None, hx)


def rel_err(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def check_fp32(got, ref, t32, what, extra=None):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert bool(torch.isfinite(got[k]).all()), f"{what} {k}: NaN / inf (a read outside an operand?)"
    worst = (0.0, 0.0, "")
    for k in ref:
        e32 = rel_err(t32[k], ref[k]) if k in t32 else 0.0
        bound = max(1e-5, 8 * e32)
        if extra is not None:
            bound = min(bound, extra)
        e = rel_err(got[k], ref[k])
        if e > worst[0]:
            worst = (e, e32, k)
        assert e <= bound, f"{what} {k}: {e:.3e} > {bound:.3e}"
    return worst


# (H, B, T, I): every H, B, T and I of the module docstring occurs
SHAPES = [(5, 1, 1, 1), (15, 3, 2, 19), (16, 17, 7, 32), (17, 33, 7, 19), (20, 65, 2, 1), (64, 3, 7, 32),
          (72, 33, 7, 19), (72, 17, 1, 32), (64, 1, 2, 1), (20, 3, 7, 19), (16, 33, 1, 1), (5, 17, 2, 32),
          (264, 3, 2, 1)]


# ------------------------------------------------------------------ fixture
@gpu
def test_fixture_cases(dev, golden):
    from speechbrain_amd.nnet.RNN import LSTM
    from speechbrain_amd.nnet.embedding import Embedding
    g = golden("lstm")
    for name in g["case.names"]:
        key = f"case.{name}."
        kw = json.loads(str(g[key + "kw"]))
        if "input_shape" in kw:
            kw["input_shape"] = tuple(kw["input_shape"])
        sd = {k[len(key) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(key + "sd.")}
        m = LSTM(**kw)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev)
        L, D, H = kw.get("num_layers", 1), 2 if kw.get("bidirectional") else 1, kw["hidden_size"]
        params = [[tuple(sd.get(f"rnn.{n}_l{l}{SFX[d]}") for n in NAMES) for d in range(D)] for l in range(L)]
        hx = None
        if key + "hx" in g.files:
            hx = tuple(torch.from_numpy(g[key + n]).to(dev).requires_grad_(True) for n in ("hx", "cx"))
        lengths = torch.from_numpy(g[key + "lengths"]).to(dev) if key + "lengths" in g.files else None
        if name == "onehot":
            emb = Embedding(**json.loads(str(g[key + "emb_kw"]))).to(dev)
            x = emb(torch.from_numpy(g[key + "tokens"]).to(dev))
            assert hasattr(x, "_sbk_onehot")
            x64 = R.onehot_table(7, 3)[torch.from_numpy(g[key + "tokens"])].float()
        else:
            x = torch.from_numpy(g[key + "x"]).to(dev).requires_grad_(True)
            x64 = torch.from_numpy(g[key + "x"]).reshape(x.shape[0], x.shape[1], -1)
        out, (hn, cn) = m(x, hx=hx, lengths=lengths)
        s = dict(params=params, x=x64, hx=None if hx is None else (torch.from_numpy(g[key + "hx"]),
                                                                  torch.from_numpy(g[key + "cx"])),
                 steps=None if lengths is None else torch.from_numpy(g[key + "steps"]), lengths=None,
                 proj=torch.from_numpy(g[key + "proj"]), projh=torch.from_numpy(g[key + "projh"]),
                 projc=torch.from_numpy(g[key + "projc"]))
        _loss(out, hn, cn, s, lambda t: t.to(dev)).backward()
        got = {"out": out, "hn": hn, "cn": cn}
        want = {"out": g[key + "out"], "hn": g[key + "hn"], "cn": g[key + "cn"]}
        for k, p in m.named_parameters():
            got["grad." + k], want["grad." + k] = p.grad, g[key + "grad." + k]
        if name != "onehot":
            got["grad.x"], want["grad.x"] = x.grad, g[key + "grad.x"]
        if hx is not None:
            got["grad.hx"], want["grad.hx"] = hx[0].grad, g[key + "grad.hx"]
            got["grad.cx"], want["grad.cx"] = hx[1].grad, g[key + "grad.cx"]
        # E32 of this case: torch's fp32 CPU LSTM (the fixture itself) against the float64 restatement
        ref = run_ref64(s)
        ren = {"out": "out", "hn": "hn", "cn": "cn", "grad.x": "dx", "grad.hx": "dhx", "grad.cx": "dcx"}
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
    worst = (0.0, 0.0, "")
    for D in (1, 2):
        for hx in (True, False):
            for bias in (True, False):
                for ragged in (False, True):
                    what = f"H{H} B{B} T{T} I{I} D{D} hx{int(hx)} bias{int(bias)} ragged{int(ragged)}"
                    s = make_spec(H, B, T, I, 1, D, bias, hx, ragged, seed=zlib.crc32(what.encode()))
                    got = run_gpu(s, dev, front=64 if hx else 65)
                    w = check_fp32(got, run_ref64(s), run_torch32(s), what)
                    worst = max(worst, (w[0], w[1], what + " " + w[2]))
    print(f"fp32 H{H} B{B} T{T} I{I}: worst kernel error {worst[0]:.3e} (E32 {worst[1]:.3e}) at {worst[2]}")


@gpu
def test_two_layers_bidirectional_ragged_fp32(dev):
    """Layer 1 reads the 2H-wide output of layer 0."""
    s = make_spec(20, 5, 7, 19, L=2, D=2, bias=True, hx=True, ragged=True, seed=5)
    check_fp32(run_gpu(s, dev), run_ref64(s), run_torch32(s), "two layers bidirectional")


@gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_single_step_bidirectional_fp32(dev, ragged):
    """T = 1: both directions' only step is the first and the last."""
    s = make_spec(20, 3, 1, 19, 1, 2, True, True, ragged, seed=6)
    check_fp32(run_gpu(s, dev), run_ref64(s), run_torch32(s), "T1 bidirectional")


@gpu
def test_interlayer_dropout_runs_in_training_only(dev):
    from speechbrain_amd.nnet.RNN import LSTM
    torch.manual_seed(0)
    m = LSTM(16, input_size=8, num_layers=2, dropout=0.5, bidirectional=True).to(dev)
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
@pytest.mark.parametrize("D", [1, 2])
def test_onehot_path(dev, V, where, D):
    from speechbrain_amd.nnet.embedding import Embedding
    blank = {"first": 0, "middle": V // 2, "last": V - 1}[where]
    B, U, H = 4, 6, 20
    tok = _tokens(V, blank, B, U, seed=V + blank)
    s = make_spec(H, B, U, V - 1, 1, D, True, True, False, seed=100 + V + blank + D)
    x64 = R.onehot_table(V, blank)[tok]
    s["x"] = x64.float()
    ref, t32 = run_ref64(s), run_torch32(s)
    ref.pop("dx")
    emb = Embedding(V, consider_as_one_hot=True, blank_id=blank).to(dev)
    m = build_gpu(s, dev)
    e = emb(_guard(tok, dev, dtype=torch.int64))
    assert torch.equal(e.cpu().double(), x64)                 # the dense rows any other consumer reads
    e.data.fill_(float("nan"))                                # the tagged path never reads them (no version bump)
    hot = run_gpu(s, dev, module=m, xin=e)
    check_fp32(hot, ref, t32, f"one-hot V{V} blank{blank} D{D}")
    # modified in place: the tag is stale, the LSTM takes the dense path
    e2 = emb(tok.to(dev))
    e2.mul_(1.0)
    dense = run_gpu(s, dev, module=m, xin=e2)
    check_fp32(dense, ref, t32, f"dense after in-place V{V} blank{blank} D{D}")
    for k in ref:
        bound = max(1e-5, 8 * rel_err(t32[k], ref[k]))
        assert rel_err(hot[k], dense[k]) <= bound, (k, rel_err(hot[k], dense[k]), bound)


@gpu
def test_forward_backward_repeat_is_bit_identical(dev):
    """H 20, B 5, T 7, bidirectional ragged: no atomics anywhere, so two runs agree bit for bit."""
    s = make_spec(20, 5, 7, 19, 1, 2, True, True, True, seed=9)
    m = build_gpu(s, dev)
    a = run_gpu(s, dev, module=m)
    b = run_gpu(s, dev, module=m)
    assert set(a) == set(b) and "dcx" in a and "dweight_hh_l0_reverse" in a
    for k in a:
        assert torch.equal(a[k], b[k]), k


@gpu
def test_decode_steps_equal_sequence(dev):
    """T = 1 calls handing the (h, c) tuple on reproduce the full-sequence output bit for bit (fp32, D = 1)."""
    s = make_spec(20, 3, 7, 19, 1, 1, True, True, False, seed=11)
    m = build_gpu(s, dev)
    x, hx = s["x"].to(dev), tuple(h.to(dev) for h in s["hx"])
    with torch.no_grad():
        full, (hn, cn) = m(x, hx=hx)
        h, outs = hx, []
        for t in range(7):
            o, h = m(x[:, t:t + 1], hx=h)
            outs.append(o)
    assert isinstance(h, tuple) and len(h) == 2
    assert torch.equal(torch.cat(outs, 1), full) and torch.equal(h[0], hn) and torch.equal(h[1], cn)


# ------------------------------------------------------------------ bf16
@gpu
@pytest.mark.parametrize("shape", [(72, 33, 7, 32), (20, 3, 7, 19)], ids=lambda s: "H%d_B%d_T%d_I%d" % s)
def test_bf16_against_rounded_restatement(dev, shape):
    """Both bidirectional and ragged.  Figures measured on an MI355X: see
    DESIGN.md (LSTM section)."""
    H, B, T, I = shape
    s = make_spec(H, B, T, I, 1, 2, True, True, True, seed=21)
    exact, yard = run_ref64(s), run_ref64(s, round_bf16=True)
    got = run_gpu(s, dev, autocast=True)
    assert set(got) == set(exact)
    for k in exact:
        dev_k = rel_err(yard[k], exact[k])
        e = rel_err(got[k], yard[k])
        print(f"bf16 H{H} B{B} T{T} I{I} {k}: restatement deviation {dev_k:.3e}, kernel error {e:.3e}")
    for k in exact:
        assert bool(torch.isfinite(got[k]).all()), k
        bound = 2 * rel_err(yard[k], exact[k]) + 1e-5
        assert rel_err(got[k], yard[k]) <= bound, f"{k}: {rel_err(got[k], yard[k]):.3e} > {bound:.3e}"
