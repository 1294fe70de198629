"""The fused CNN_Block layer (csrc/convln.hip through _autograd.CnnBlockFn)
against a float64 restatement in plain torch on the CPU — reflect F.pad,
F.conv2d, layer_norm over (F, Co), leaky_relu, max_pool2d over frequency —
and the CRDNN lobe against the reference's recorded outputs and gradients
(tests/golden/crdnn.npz).

Bounds.  fp32: per tensor max(1e-5, 8 * E32), E32 the error of the same
restatement in float32, errors relative to max(1, |reference|max).  bf16
(autocast): within 2 * (the deviation of the float64 restatement with x and w
rounded to bf16 from the exact one) + 1e-5.  Inputs are continuous random
draws: no ties inside a pool window."""
import json

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
EPS, SLOPE = 1e-5, 0.01
NAMES = ("y", "dx", "dw", "db", "dg", "dbeta")


def make(B, T, Fq, Ci, Co, pool, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=r(B, T, Fq, Ci), w=r(Co, Ci, 3, 3) / (3.0 * Ci ** 0.5), b=0.1 * r(Co), g=1 + 0.2 * r(Fq, Co),
                beta=0.2 * r(Fq, Co), R=r(B, T, Fq // pool, Co), pool=pool)


def restate(s, dtype, bf16=False):
    def rnd(t):  # a bf16 MFMA operand: rounded, gradient passed straight through
        return t + (t.detach().bfloat16().to(t.dtype) - t.detach()) if bf16 else t
    p = {k: s[k].to(dtype).clone().requires_grad_(True) for k in ("x", "w", "b", "g", "beta")}
    xp = F.pad(rnd(p["x"]).permute(0, 3, 2, 1), (1, 1, 1, 1), mode="reflect")        # (B, Ci, F + 2, T + 2)
    c = F.conv2d(xp, rnd(p["w"]), p["b"]).permute(0, 3, 2, 1)                        # (B, T, F, Co)
    a = F.leaky_relu(F.layer_norm(c, c.shape[2:], p["g"], p["beta"], EPS), SLOPE)
    if s["pool"] > 1:
        a = F.max_pool2d(a.permute(0, 3, 1, 2), (1, s["pool"])).permute(0, 2, 3, 1)
    (a * s["R"].to(dtype)).sum().backward()
    return dict(zip(NAMES, [a.detach().double()] + [p[k].grad.double() for k in ("x", "w", "b", "g", "beta")]))


def run_gpu(s, dev, dtype=torch.float32, fused=True):
    from speechbrain_amd import _autograd as A
    from speechbrain_amd import _enc
    p = {k: s[k].clone().to(dev).requires_grad_(True) for k in ("x", "w", "b", "g", "beta")}
    y = A.cnn_block(p["x"], p["w"], p["b"], p["g"], p["beta"], EPS, SLOPE, s["pool"], None, dtype,
                    _enc.WeightCache(), "img", fused=fused)
    assert y.dtype == dtype
    (y.float() * s["R"].to(dev)).sum().backward()
    return dict(zip(NAMES, [y.detach().double().cpu()] + [p[k].grad.double().cpu()
                                                           for k in ("x", "w", "b", "g", "beta")]))


def rel_err(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def frames(dtype, Fq, Ci, Co):
    from speechbrain_amd import _autograd as A
    return A.cnn_block_frames(dtype, Fq, Ci, Co)


# B, T (an int, or in frames per workgroup n: "n-1", "n", "n+1", "2n+1"), F, Ci, Co, pool.  F = 5 with pool 2
# drops the trailing bin; 7 frames of F = 21 leave the last 16-row tile part empty; B = 3: distinct utterances,
# where a halo frame read across the utterance boundary would show.
SWEEP = [(1, 2, 2, 1, 16, 1), (3, 3, 3, 3, 16, 3), (1, "n-1", 5, 32, 128, 2), (3, "n", 5, 3, 16, 2),
         (1, "n+1", 40, 1, 128, 2), (3, "2n+1", 40, 32, 256, 2), (1, "2n+1", 21, 128, 128, 3),
         (1, "n+1", 40, 128, 256, 2), (1, "n-1", 40, 32, 16, 1), (3, "n", 3, 128, 256, 1),
         (1, "2n+1", 2, 3, 128, 2), (3, "n+1", 20, 256, 256, 2)]
_ID = lambda c: "B%d_T%s_F%d_Ci%d_Co%d_p%d" % c  # noqa: E731


def resolve(case, dtype):
    B, T, Fq, Ci, Co, pool = case
    n = frames(dtype, Fq, Ci, Co)
    assert n > 0, "the sweep's shapes are all in the kernel's set"
    if isinstance(T, str):
        T = max(2, {"n-1": n - 1, "n": n, "n+1": n + 1, "2n+1": 2 * n + 1}[T])
    return B, T, Fq, Ci, Co, pool


@gpu
@pytest.mark.parametrize("case", SWEEP, ids=_ID)
def test_sweep_fp32(dev, case):
    s = make(*resolve(case, torch.float32))
    ref, t32, got = restate(s, torch.float64), restate(s, torch.float32), run_gpu(s, dev)
    for k in NAMES:
        e, bound = rel_err(got[k], ref[k]), max(1e-5, 8 * rel_err(t32[k], ref[k]))
        print(f"fp32 {_ID(case)} {k}: err {e:.3e}, bound {bound:.3e}")
        assert bool(torch.isfinite(got[k]).all()) and e <= bound, f"{k}: {e:.3e} > {bound:.3e}"


@gpu
@pytest.mark.parametrize("case", [SWEEP[4], SWEEP[5], SWEEP[6], SWEEP[7]], ids=_ID)
def test_bf16_against_rounded_restatement(dev, case):
    s = make(*resolve(case, torch.bfloat16), seed=3)
    exact, yard = restate(s, torch.float64), restate(s, torch.float64, bf16=True)
    got = run_gpu(s, dev, torch.bfloat16)
    for k in NAMES:
        e, bound = rel_err(got[k], yard[k]), 2 * rel_err(yard[k], exact[k]) + 1e-5
        print(f"bf16 {_ID(case)} {k}: restatement deviation {rel_err(yard[k], exact[k]):.3e}, kernel error {e:.3e}")
        assert bool(torch.isfinite(got[k]).all()) and e <= bound, f"{k}: {e:.3e} > {bound:.3e}"


@gpu
def test_unsupported_geometry_takes_the_fallback(dev):
    assert frames(torch.float32, 168, 8, 16) == 0   # more bins than a workgroup's rows
    s = make(1, 3, 168, 8, 16, 2)
    ref, t32, got = restate(s, torch.float64), restate(s, torch.float32), run_gpu(s, dev)
    for k in NAMES:
        assert rel_err(got[k], ref[k]) <= max(1e-5, 8 * rel_err(t32[k], ref[k])), k


@gpu
def test_argument_errors_write_nothing(dev):
    from speechbrain_amd._lib import lib, ptr, stream_of
    x = torch.randn(1, 4, 6, 8, device=dev)
    y = torch.full((1, 4, 6, 32), 7.0, device=dev)
    aff = torch.ones(6, 32, device=dev)
    img = torch.zeros(1 << 16, device=dev)
    for T, Fq, Co, pool in ((4, 6, 24, 1), (1, 6, 32, 1), (4, 1, 32, 1), (4, 6, 272, 1), (4, 6, 32, 7)):
        rc = lib().sbk_conv3x3_ln(0, ptr(x), 1, T, Fq, 8, Co, ptr(img), None, ptr(aff), ptr(aff), EPS, SLOPE, pool,
                                  None, ptr(y), None, None, None, stream_of(x))
        assert rc == 1001, (T, Fq, Co, pool)
    assert lib().sbk_conv3x3_ln_bwd(0, ptr(y), ptr(y), ptr(aff), ptr(aff), ptr(aff), ptr(aff), None, 1, 4, 128, 256, 1,
                                    SLOPE, ptr(y), ptr(y), stream_of(x)) == 1001  # F * Co > 16384
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


@gpu
def test_backward_runs_are_bit_identical(dev):
    s = make(3, 9, 20, 32, 64, 2, seed=5)
    a, b = run_gpu(s, dev, torch.bfloat16), run_gpu(s, dev, torch.bfloat16)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", ["doctest_crdnn", "doctest_block", "small_eval", "small_train"])
def test_lobe_against_reference_fixture(dev, golden, monkeypatch, name, fused):
    from speechbrain_amd.lobes.models import CRDNN as M
    monkeypatch.setattr(M.CRDNN, "USE_FUSED_CNN", fused)
    from speechbrain_amd.nnet import RNN
    g, pre = golden("crdnn"), f"case.{name}."
    kw = json.loads(str(g[pre + "kw"]))
    kw["input_shape"] = tuple(kw["input_shape"])
    if "rnn_class" in kw:
        kw["rnn_class"] = getattr(RNN, kw["rnn_class"])
    net = getattr(M, str(g[pre + "cls"]))(**kw)
    net.load_state_dict({k[len(pre) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre + "sd.")},
                        strict=True)
    net.to(dev).train(bool(g[pre + "train"]))
    x = torch.from_numpy(g[pre + "x"]).to(dev).requires_grad_(True)
    y = net(x)
    assert y.dtype == torch.float32
    (y * torch.from_numpy(g[pre + "proj"]).to(dev)).sum().backward()
    got = {"out": y.detach(), "grad.x": x.grad, **{"grad." + k: p.grad for k, p in net.named_parameters()}}
    assert set(got) == {k[len(pre):] for k in g.files if k.startswith((pre + "out", pre + "grad."))}
    for k, v in got.items():
        e = rel_err(v.double().cpu(), torch.from_numpy(g[pre + k]).double())
        print(f"{name} {k}: {e:.3e}")
        assert e <= 1e-4, f"{k}: {e:.3e}"
