"""csrc/ligru.hip through the drop-in speechbrain_amd.nnet.RNN.LiGRU, against
the float64 restatement of tests/ligru_ref.py (held to the reference's fixture
by test_ligru_cpu.py).  The method is that of test_gpu_lstm.py.

Shapes.  The step kernels give a workgroup 16 hidden units of one direction and
up to 32 batch rows, deal K to eight waves in chunks of 32 and read 8 K elements
per lane, vectorised when H % 4 == 0 (fp32 forward; H % 2 == 0 backward, K =
2H).  The sweep takes H in {5, 15, 16, 17, 20, 64, 72, 264}, B in {1, 3, 17, 33,
65}, T in {1, 2, 7} and I in {1, 19, 32}, rotated over thirteen shapes so that
every value occurs; each shape runs the twelve combinations of D in {1, 2} / hx
/ {batchnorm in training, batchnorm in eval, layernorm}, with a non-trivial
recurrent-dropout mask wherever the module is training (eval passes none, as
the reference), forward and backward of sum(out · P) + sum(h · Q).  The
activations rotate over the shapes.

Guard bands.  x, hx, the mask pool, every parameter and the running statistics
are views into larger device buffers whose other elements are NaN; the buffers
of the variants without hx start one element off 16-byte alignment, which sends
the kernels down their scalar loads.

Bounds.  Inputs are N(0, 1), u N(0, 1) / sqrt(H), gamma 1 + 0.3 N, beta 0.3 N.
The entries of w are +-(0.5 + U(0, 1)) / sqrt(I): a column of the input
projection is divided by its own spread in the normalisation, so an entry of w
near zero at I = 1 (where a column is x times that one entry, and dw and dx
are sums that cancel analytically) would make every figure below a measure of
1 / |w| rather than of the kernels.  fp32: per tensor max |err| / max(1, |ref|_inf) <=
max(1e-5, 8 * E32), E32 the same figure for the fp32 CPU run of the restatement
against its float64 run; the fixture cases meet 1e-4 against the reference's
own values.  bf16 (autocast): the yardstick is the float64 restatement with x,
w, u and the h operand rounded to bf16; the kernel stays within 2 * (that
restatement's deviation from the unrounded one) + 1e-5 of it.

The ReLU / LeakyReLU kink.  A pre-activation a within rounding of 0 flips act',
so a gradient check with these activations holds only where no a is that
small: min |a| >= 1e-4 in the float64 restatement for fp32, >= 0.02 in both
restatements for bf16.  The condition is asserted, never skipped on: a case's
seeds are tried in order on the CPU and the first whose restatement alone meets
the condition is used.  That bounds the shapes (about 10k pre-activations for
fp32, about 100 for bf16); the largest shapes use tanh / sin.
"""
import json
import zlib

import pytest
import torch

import ligru_ref as R

gpu = pytest.mark.gpu
PNAMES = (("w", "w.weight"), ("u", "u.weight"), ("gamma", "norm.weight"), ("beta", "norm.bias"))
NORMS = ("bn_train", "bn_eval", "layernorm")


# ------------------------------------------------------------------ cases
def make_spec(H, B, T, I, L=1, D=1, hx=True, norm="bn_train", act="relu", seed=0):
    g = torch.Generator().manual_seed(seed)
    params = []
    for l in range(L):
        i = I if l == 0 else D * H
        w = (0.5 + torch.rand(2 * H, i, generator=g)) * (2.0 * torch.randint(0, 2, (2 * H, i), generator=g) - 1)
        p = dict(w=w / i ** 0.5, u=torch.randn(2 * H, H, generator=g) / H ** 0.5,
                 gamma=1 + 0.3 * torch.randn(2 * H, generator=g), beta=0.3 * torch.randn(2 * H, generator=g))
        if norm != "layernorm":
            p["rmean"] = 0.3 * torch.randn(2 * H, generator=g)
            p["rvar"] = 0.5 + torch.rand(2 * H, generator=g)
        params.append(p)
    train = norm != "bn_eval"
    s = dict(params=params, x=torch.randn(B, T, I, generator=g), D=D, act=act, norm=norm, train=train,
             hx=torch.randn(L, D * B, H, generator=g) if hx else None,
             masks=[(torch.rand(D * B, H, generator=g) > 0.3).float() / 0.7 for _ in range(L)] if train else None,
             proj=torch.randn(B, T, D * H, generator=g), projh=torch.randn(L * D, B, H, generator=g))
    return s


def run_ref(s, dtype=torch.float64, round_bf16=False):
    params = []
    for p in s["params"]:
        q = {k: v.to(dtype).clone() for k, v in p.items()}
        for n, _ in PNAMES:
            q[n].requires_grad_(True)
        params.append(q)
    x = s["x"].to(dtype).clone().requires_grad_(True)
    hx = None if s["hx"] is None else s["hx"].to(dtype).clone().requires_grad_(True)
    masks = None if s["masks"] is None else [m.to(dtype) for m in s["masks"]]
    info = {}
    out, h = R.ligru_ref(x, params, hx, masks, s["act"], s["train"], s["D"] == 2, x.shape[0], round_bf16, info)
    ((out * s["proj"].to(dtype)).sum() + (h * s["projh"].to(dtype)).sum()).backward()
    res = {"out": out, "h": h, "dx": x.grad}
    for l, q in enumerate(params):
        for n, _ in PNAMES:
            res[f"d{n}_l{l}"] = q[n].grad
        if "rmean" in q:
            res[f"rmean_l{l}"], res[f"rvar_l{l}"] = q["rmean"], q["rvar"]
    if hx is not None:
        res["dhx"] = hx.grad
    return {k: v.detach().double() for k, v in res.items()}, info["min_abs_a"]


def kink_free(H, B, T, I, what, floor, both=False, **kw):
    """The first seed of the case whose restatement(s) keep every |a| >= floor;
    returns (spec, float64 results)."""
    base = zlib.crc32(what.encode())
    for k in range(400):
        s = make_spec(H, B, T, I, seed=base + k, **kw)
        ref, lo = run_ref(s)
        if both:
            lo = min(lo, run_ref(s, round_bf16=True)[1])
        if lo >= floor:
            return s, ref, lo
    raise AssertionError(f"{what}: no seed in 400 keeps min |a| >= {floor}")


def _guard(t, dev, front=64):
    """t as a view into a larger device buffer whose other elements are NaN."""
    buf = torch.full((front + t.numel() + 64,), float("nan"), device=dev, dtype=t.dtype)
    v = buf[front:front + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def build_gpu(s, dev, front=64):
    from speechbrain_amd.nnet.RNN import LiGRU
    B, T, I = s["x"].shape
    H = s["params"][0]["u"].shape[1]
    m = LiGRU(H, (B, T, I), nonlinearity=s["act"], normalization="layernorm" if s["norm"] == "layernorm" else "batchnorm",
              num_layers=len(s["params"]), bidirectional=s["D"] == 2, re_init=False).to(dev)
    for lay, p in zip(m.rnn, s["params"]):
        for n, k in PNAMES:
            mod, attr = k.split(".")
            getattr(getattr(lay, mod), attr).data = _guard(p[n], dev, front)
    m.train(s["train"])
    return m


def _arm(m, s, dev, front):
    """Fresh running statistics and the case's masks as the rows the pool yields next."""
    for lay, p, i in zip(m.rnn, s["params"], range(len(s["params"]))):
        if "rmean" in p:
            lay.norm.running_mean = _guard(p["rmean"], dev, front)
            lay.norm.running_var = _guard(p["rvar"], dev, front)
        if s["masks"] is not None:
            lay.drop_masks = _guard(s["masks"][i], dev, front)
            lay.N_drop_masks = s["masks"][i].shape[0]
            lay.drop_mask_cnt = 0


def run_gpu(s, dev, front=64, autocast=False, module=None):
    m = module or build_gpu(s, dev, front)
    _arm(m, s, dev, front)
    for p in m.parameters():
        p.grad = None
    x = _guard(s["x"], dev, front).requires_grad_(True)
    hx = None if s["hx"] is None else _guard(s["hx"], dev, front).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out, h = m(x, hx=hx)
    assert out.dtype == torch.float32 and h.dtype == torch.float32
    ((out * s["proj"].to(dev)).sum() + (h * s["projh"].to(dev)).sum()).backward()
    res = {"out": out, "h": h, "dx": x.grad}
    for l, lay in enumerate(m.rnn):
        for n, k in PNAMES:
            mod, attr = k.split(".")
            res[f"d{n}_l{l}"] = getattr(getattr(lay, mod), attr).grad
        if "rmean" in s["params"][l]:
            res[f"rmean_l{l}"], res[f"rvar_l{l}"] = lay.norm.running_mean, lay.norm.running_var
    if hx is not None:
        res["dhx"] = hx.grad
    return {k: v.detach().double().cpu() for k, v in res.items()}


def rel_err(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def check_fp32(got, ref, t32, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert bool(torch.isfinite(got[k]).all()), f"{what} {k}: NaN / inf (a read outside an operand?)"
    worst = (0.0, 0.0, "")
    for k in ref:
        e32 = rel_err(t32[k], ref[k])
        bound = max(1e-5, 8 * e32)
        e = rel_err(got[k], ref[k])
        if e > worst[0]:
            worst = (e, e32, k)
        assert e <= bound, f"{what} {k}: {e:.3e} > {bound:.3e} (E32 {e32:.3e})"
    return worst


# (H, B, T, I, activation): every H, B, T and I of the module docstring occurs; ReLU / LeakyReLU
# stay at or below about 10k pre-activations (2 * B * T * H for two directions)
SHAPES = [(5, 1, 2, 1, "relu"), (15, 3, 2, 19, "leaky_relu"), (16, 17, 7, 32, "tanh"), (17, 33, 7, 19, "sin"),
          (20, 65, 2, 1, "relu"), (64, 3, 7, 32, "leaky_relu"), (72, 33, 2, 19, "relu"), (72, 17, 1, 32, "tanh"),
          (64, 1, 2, 1, "sin"), (20, 3, 7, 19, "relu"), (16, 33, 1, 1, "leaky_relu"), (5, 17, 2, 32, "tanh"),
          (264, 3, 2, 1, "sin")]


# ------------------------------------------------------------------ fixture
def _kw(g, key):
    kw = json.loads(str(g[key]))
    if "input_shape" in kw:
        kw["input_shape"] = tuple(kw["input_shape"])
    return kw


@gpu
def test_fixture_cases(dev, golden):
    """Every case of the reference's fixture at 1e-4: outputs, h, gradients and
    the running statistics after each call."""
    from speechbrain_amd.nnet.RNN import LiGRU
    from speechbrain_amd.nnet.embedding import Embedding
    g = golden("ligru")
    assert len(g["case.names"]) == 17
    for name in g["case.names"]:
        kw = _kw(g, f"case.{name}.kw")
        sd = {k[len(f"case.{name}.sd."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"case.{name}.sd.")}
        m = LiGRU(**kw)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).train(bool(int(g[f"case.{name}.train"])))
        for c in range(int(g[f"case.{name}.calls"])):
            key = f"case.{name}.{c}."
            m.zero_grad(set_to_none=True)
            hx = torch.from_numpy(g[key + "hx"]).to(dev).requires_grad_(True) if key + "hx" in g.files else None
            if name == "onehot":
                emb = Embedding(**json.loads(str(g[f"case.{name}.emb_kw"]))).to(dev)
                x = emb(torch.from_numpy(g[key + "tokens"]).to(dev))
            else:
                x = torch.from_numpy(g[key + "x"]).to(dev).requires_grad_(True)
            out, h = m(x, hx=hx)
            ((out * torch.from_numpy(g[key + "proj"]).to(dev)).sum()
             + (h * torch.from_numpy(g[key + "projh"]).to(dev)).sum()).backward()
            got = {"out": out, "h": h}
            for k, p in m.named_parameters():
                got["grad." + k] = p.grad
            if name != "onehot":
                got["grad.x"] = x.grad
            if hx is not None:
                got["grad.hx"] = hx.grad
            for k, v in m.state_dict().items():
                if "running_" in k or "num_batches" in k:
                    got["after." + k] = v
            want = {k[len(key):] for k in g.files if k.startswith(key)} - {"x", "hx", "proj", "projh", "tokens"}
            assert set(got) == want, (name, sorted(got), sorted(want))
            for k, v in got.items():
                w = torch.from_numpy(g[key + k]).double()
                v = v.detach().double().cpu()
                assert v.shape == w.shape, (name, c, k, v.shape, w.shape)
                assert bool(torch.isfinite(v).all()), (name, c, k)
                assert rel_err(v, w) <= 1e-4, f"{name} call {c} {k}: {rel_err(v, w):.3e}"


@gpu
def test_frame_by_frame_equals_sequence(dev):
    """The reference's unit test: a two-layer layernorm LiGRU fed frame by
    frame with the returned h equals the whole-sequence call (1e-3 there; both
    are fp32 runs of the same kernels here, so the fp32 floor of 1e-5)."""
    from speechbrain_amd.nnet.RNN import LiGRU
    torch.manual_seed(0)
    for shape in ((1, 2, 2), (3, 7, 19)):
        inputs = torch.randn(shape).to(dev)
        net = LiGRU(hidden_size=5, input_shape=inputs.shape, num_layers=2, bidirectional=False,
                    normalization="layernorm").to(dev)
        with torch.no_grad():
            output, hn = net(inputs)
            outs, hn_t = [], None
            for t in range(inputs.shape[1]):
                out_t, hn_t = net(inputs[:, t, :].unsqueeze(1), hn_t)
                outs.append(out_t.squeeze(1))
        out_steps = torch.stack(outs, dim=1)
        assert hn.shape == hn_t.shape == (2, shape[0], 5)
        assert float((out_steps - output).abs().max()) <= 1e-5
        assert float((hn_t - hn).abs().max()) <= 1e-5


@gpu
def test_layer_works_on_its_own(dev):
    from speechbrain_amd.nnet.RNN import LiGRU_Layer
    s = make_spec(20, 3, 7, 19, 1, 2, True, "layernorm", "tanh", seed=3)
    lay = LiGRU_Layer(19, 20, 1, 3, normalization="layernorm", nonlinearity="tanh", bidirectional=True).to(dev)
    for n, k in PNAMES:
        mod, attr = k.split(".")
        getattr(getattr(lay, mod), attr).data = s["params"][0][n].to(dev)
    lay.drop_masks, lay.N_drop_masks = s["masks"][0].to(dev), 6
    out = lay(s["x"].to(dev), s["hx"][0].to(dev))
    ref, _ = run_ref(s)
    assert rel_err(out.detach().double().cpu(), ref["out"]) <= 1e-5


# ------------------------------------------------------------------ edge sweep
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d_B%d_T%d_I%d_%s" % s)
def test_edge_sweep_fp32(dev, shape):
    H, B, T, I, act = shape
    kink = act in ("relu", "leaky_relu")
    worst = (0.0, 0.0, "")
    for D in (1, 2):
        for hx in (True, False):
            for norm in NORMS:
                what = f"H{H} B{B} T{T} I{I} {act} D{D} hx{int(hx)} {norm}"
                kw = dict(L=1, D=D, hx=hx, norm=norm, act=act)
                if kink:
                    s, ref, lo = kink_free(H, B, T, I, what, 1e-4, **kw)
                    assert lo >= 1e-4, (what, lo)
                else:
                    s = make_spec(H, B, T, I, seed=zlib.crc32(what.encode()), **kw)
                    ref, _ = run_ref(s)
                got = run_gpu(s, dev, front=64 if hx else 65)
                w = check_fp32(got, ref, run_ref(s, torch.float32)[0], what)
                worst = max(worst, (w[0], w[1], what + " " + w[2]))
    print(f"fp32 H{H} B{B} T{T} I{I} {act}: worst kernel error {worst[0]:.3e} (E32 {worst[1]:.3e}) at {worst[2]}")


@gpu
@pytest.mark.parametrize("norm", NORMS)
def test_two_layers_bidirectional_fp32(dev, norm):
    """Layer 1 reads the 2H-wide output of layer 0; h is the raw reshape."""
    s = make_spec(20, 5, 7, 19, L=2, D=2, hx=True, norm=norm, act="tanh", seed=5)
    ref, _ = run_ref(s)
    assert ref["h"].shape == (4, 5, 20)
    check_fp32(run_gpu(s, dev), ref, run_ref(s, torch.float32)[0], "two layers bidirectional " + norm)


@gpu
def test_running_statistics_after_training_calls(dev):
    """Two consecutive training calls of a bidirectional batchnorm layer: the
    unbiased factor is n / (n - 1) with n = 2 * B * T, the counter advances."""
    s = make_spec(16, 3, 2, 19, 1, 2, False, "bn_train", "sin", seed=8)
    m = build_gpu(s, dev)
    got = run_gpu(s, dev, module=m)
    ref, _ = run_ref(s)
    for k in ("rmean_l0", "rvar_l0"):
        assert rel_err(got[k], ref[k]) <= 1e-6, (k, rel_err(got[k], ref[k]))
    n = 2 * 3 * 2
    biased = (ref["rvar_l0"] - 0.95 * s["params"][0]["rvar"].double()) / 0.05 * (n - 1) / n
    wrong = 0.95 * s["params"][0]["rvar"].double() + 0.05 * biased * (n // 2) / (n // 2 - 1)
    assert rel_err(got["rvar_l0"], wrong) > 1e-4       # not the B * T row count
    assert int(m.rnn[0].norm.num_batches_tracked) == 1
    m(s["x"].to(dev))
    assert int(m.rnn[0].norm.num_batches_tracked) == 2
    m.eval()
    before = m.rnn[0].norm.running_var.clone()
    m(s["x"].to(dev))
    assert torch.equal(before, m.rnn[0].norm.running_var) and int(m.rnn[0].norm.num_batches_tracked) == 2


@gpu
def test_dropout_pool_counter_and_eval(dev):
    """The pool is sliced batch_size rows per call from a running counter;
    another batch size resamples it; eval passes no mask."""
    from speechbrain_amd.nnet.RNN import LiGRU
    torch.manual_seed(1)
    m = LiGRU(8, (3, 4, 6), dropout=0.5, bidirectional=True, normalization="layernorm").to(dev)
    lay = m.rnn[0]
    assert lay.batch_size == 6 and lay.drop_masks.shape == (16000, 8)
    x = torch.randn(3, 4, 6, device=dev)
    a, b = m(x)[0], m(x)[0]
    assert lay.drop_mask_cnt == 12 and not torch.equal(a, b)
    pool = lay.drop_masks
    m(torch.randn(2, 4, 6, device=dev))
    assert lay.batch_size == 4 and lay.drop_masks is not pool and lay.drop_mask_cnt == 16
    m.eval()
    c, d = m(x)[0], m(x)[0]
    assert torch.equal(c, d) and lay.drop_mask_cnt == 16


@gpu
def test_forward_backward_repeat_is_bit_identical(dev):
    """H 20, B 5, T 7, bidirectional, batchnorm in training: no atomics anywhere."""
    s = make_spec(20, 5, 7, 19, 1, 2, True, "bn_train", "tanh", seed=9)
    m = build_gpu(s, dev)
    a = run_gpu(s, dev, module=m)
    b = run_gpu(s, dev, module=m)
    assert set(a) == set(b) and "dhx" in a and "du_l0" in a
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------ bf16
def _check_bf16(got, exact, yard, what):
    assert set(got) == set(exact)
    for k in exact:
        print(f"bf16 {what} {k}: restatement deviation {rel_err(yard[k], exact[k]):.3e}, "
              f"kernel error {rel_err(got[k], yard[k]):.3e}")
    for k in exact:
        assert bool(torch.isfinite(got[k]).all()), k
        bound = 2 * rel_err(yard[k], exact[k]) + 1e-5
        assert rel_err(got[k], yard[k]) <= bound, f"{what} {k}: {rel_err(got[k], yard[k]):.3e} > {bound:.3e}"


@gpu
@pytest.mark.parametrize("case", [(72, 33, 7, 32, "tanh", "bn_train"), (20, 3, 7, 19, "sin", "layernorm")],
                         ids=lambda c: "H%d_B%d_T%d_I%d_%s_%s" % c)
def test_bf16_against_rounded_restatement(dev, case):
    """Both bidirectional with hx.  Figures measured on an MI355X: see DESIGN.md (LiGRU section)."""
    H, B, T, I, act, norm = case
    s = make_spec(H, B, T, I, 1, 2, True, norm, act, seed=21)
    _check_bf16(run_gpu(s, dev, autocast=True), run_ref(s)[0], run_ref(s, round_bf16=True)[0], f"H{H} B{B} T{T} I{I}")


@gpu
@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_bf16_kink_gradients(dev, act):
    """H 17, B 3, T 2, one direction: 102 pre-activations, every one at least 0.02 from the kink in both restatements."""
    what = f"bf16 kink {act}"
    s, exact, lo = kink_free(17, 3, 2, 19, what, 0.02, both=True, L=1, D=1, hx=True, norm="layernorm", act=act)
    assert lo >= 0.02, lo
    _check_bf16(run_gpu(s, dev, autocast=True), exact, run_ref(s, round_bf16=True)[0], what)


# ------------------------------------------------------------------ the transducer's prediction network
class TorchLiGRU(torch.nn.Module):
    """The restatement as a module the searcher can drive (it dispatches on the class name)."""

    def __init__(self, params):
        super().__init__()
        self.params = params

    def forward(self, x, hx=None):
        p = [{k: v.to(x.device) for k, v in q.items()} for q in self.params]
        return R.ligru_ref(x, p, hx, None, "relu", False)


TorchLiGRU.__name__ = "LiGRU"


@gpu
def test_greedy_transducer_search_on_embedding_and_ligru(dev):
    """TransducerBeamSearcher greedy decode with [Embedding, LiGRU(layernorm)]
    (the TIMIT transducer recipe's dec) matches the same search driven by the
    torch restatement on a tiny lattice.  Encoder seeds are tried in order; one
    is admitted if the restatement's search is unchanged under 1 + 1e-4 * randn
    noise for three seeds and emits at least one token."""
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.nnet.RNN import LiGRU
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.transducer.transducer_joint import Transducer_joint
    V, H, BLANK = 12, 16, 0
    g = torch.Generator().manual_seed(4)
    s = make_spec(H, 2, 1, V - 1, 1, 1, False, "layernorm", "relu", seed=31)
    dec = LiGRU(H, (2, 1, V - 1), normalization="layernorm", re_init=False)
    for n, k in PNAMES:
        mod, attr = k.split(".")
        getattr(getattr(dec.rnn[0], mod), attr).data = s["params"][0][n].clone()
    cls = Linear(V, input_size=H)
    bias = 0.5 * torch.randn(V, generator=g)
    bias[BLANK] += 2.0
    cls.load_state_dict({"w.weight": torch.randn(V, H, generator=g) / H ** 0.5, "w.bias": bias})
    cls = cls.to(dev).eval()
    emb = Embedding(V, consider_as_one_hot=True, blank_id=BLANK).to(dev).eval()
    kw = dict(tjoint=Transducer_joint(joint="sum", nonlinearity=torch.nn.LeakyReLU), classifier_network=[cls],
              blank_id=BLANK, beam_size=1, nbest=1, lm_module=None, lm_weight=0.0, state_beam=2.3, expand_beam=2.3)
    ours = TransducerBeamSearcher(decode_network_lst=[emb, dec.to(dev).eval()], **kw)
    theirs = TransducerBeamSearcher(decode_network_lst=[emb, TorchLiGRU(s["params"]).eval()], **kw)
    with torch.no_grad():
        for seed in range(300, 306):
            tn = 2.0 * torch.randn(2, 5, H, generator=torch.Generator().manual_seed(seed))
            base = theirs(tn.to(dev))
            stable = any(len(h) > 0 for h in base[0])
            for ns in (101, 102, 103):
                noise = 1 + 1e-4 * torch.randn(tn.shape, generator=torch.Generator().manual_seed(ns))
                stable = stable and theirs((tn * noise).to(dev))[0] == base[0]
            if stable:
                break
        else:
            raise AssertionError("no encoder seed in 300..305 gives an admitted case")
        res = ours(tn.to(dev))
    assert res[0] == base[0], (res[0], base[0])
    assert abs(float(res[1]) - float(base[1])) <= 1e-4
