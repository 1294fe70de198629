"""tests/layer_ref.py, the float64 reference of the fused layer launches, on
the CPU (no kernel runs here):

* anchors: with rounding off it is test_gpu_proj_tail._ffn64,
  test_gpu_layer_phases._boundary64 and oracle.conformer's restatement of the
  same modules, to 1e-12;
* the exact probes: the closed form of layer_ref.probe_expected is what the
  reference computes with rounding on, in float64 and (every value being exact)
  in float32, bit for bit;
* the E32 table is not below the re-measured float32 deviations;
* the comparison helper implements the two bound forms;
* every term is visible: dropped or altered in the reference alone it moves a
  compared output by at least 4 times its bound in at least half of the rows it
  reaches, in every reference case that has it;
* the reference cases and probes launch all 28 instantiations.
"""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import layer_ref as R
import oracle.conformer as OC
from test_gpu_layer_phases import _boundary64, ln64
from test_gpu_proj_tail import _ffn64

D = R.D


def _rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


# --------------------------------------------------------------------- anchors
@pytest.mark.parametrize("act,deff,H", [("swish", 256, 256), ("gelu", 256, 1024), ("swish", 144, 256), ("gelu", 144, 2048)])
def test_anchor_ffn64(act, deff, H):
    """One block, rounding off, against test_gpu_proj_tail._ffn64 and its projection."""
    c = R.make_case("ffn_proj", act, H, 768, deff, M=50, post=False, seed=3)
    got = R.reference(c, rounding=False)
    A = c["A"]
    ref_out = _ffn64(c["x"], A["ln0"], A, 0.5, act, deff)
    ref_y = ln64(ref_out, *c["next_ln"], deff=deff) @ c["wp"].double().T
    assert _rel(got["out"], ref_out) <= 1e-12
    assert _rel(got["yp"], ref_y) <= 1e-12


def _as_modules(c):
    """Case c's conv stage and blocks in the shape test_gpu_layer_phases._boundary64 reads."""
    cv, A, B = c["conv"], c["A"], c["B"]
    lin = lambda w, b: SimpleNamespace(weight=w.float(), bias=b)  # noqa: E731
    lnm = lambda p: SimpleNamespace(weight=p[0], bias=p[1], eps=p[2])  # noqa: E731
    cm = SimpleNamespace(layer_norm=lnm(cv["ln0"]), bottleneck=[lin(cv["w1"].reshape(2 * D, D, 1), cv["b1"])],
                         conv=lin(cv["taps"].T.reshape(D, 1, cv["K"]).contiguous(), cv["bc"]),
                         after_conv=[lnm(cv["ln1"]), None, lin(cv["w2"], cv["b2"])])
    ffn = lambda p: SimpleNamespace(ffn=[lin(p["w1"], p["b1"]), None, None, lin(p["w2"], p["b2"])])  # noqa: E731
    return SimpleNamespace(x=c["x"], o=cv["o"].float(), wo=cv["wo"].float(), bo=cv["bo"], cm=cm, fa=ffn(A), fb=ffn(B),
                           lns=[A["ln0"], A["post_ln"], B["ln0"], c["next_ln"]], wp=c["wp"].float())


def _tail_of(c):
    """The conv_ffn_tail launch on the chain case's conv stage and block A."""
    t = dict(c, launch="conv_ffn_tail", B=None, wp=None, np=0, u_bf16=False)
    return t


@pytest.mark.parametrize("B,T,K,masked,deff", [(2, 50, 31, False, 256), (2, 97, 31, True, 256), (2, 50, 15, True, 144)])
def test_anchor_boundary64(B, T, K, masked, deff):
    """The conv launches, rounding off, against test_gpu_layer_phases._boundary64
    (which rounds the taps to bf16: the case's taps are rounded beforehand)."""
    c = R.make_case("conv_ffn_chain", "swish", 512, 768, deff, B=B, T=T, K=K, masked=masked, seed=5)
    c["conv"]["taps"] = R.rbf(c["conv"]["taps"])
    ref_out, ref_y, ref_u = _boundary64(_as_modules(c), B, T, K, c["conv"]["kpm"], deff)
    got = R.reference(c, rounding=False)
    assert _rel(got["out"], ref_out) <= 1e-12
    assert _rel(got["yp"], ref_y) <= 1e-12
    assert _rel(R.reference(_tail_of(c), rounding=False)["u"], ref_u) <= 1e-12


@pytest.mark.parametrize("K,causal,masked", [(31, False, True), (15, False, False), (31, True, True)])
def test_anchor_oracle(K, causal, masked):
    """The same launches against oracle.conformer's conv_module and ffn_module in float64."""
    B, T = 2, 61
    c = R.make_case("conv_ffn_chain", "swish", 512, 256, 256, B=B, T=T, K=K, causal=causal, masked=masked, seed=6)
    cv, A, Bk = c["conv"], c["A"], c["B"]
    d = lambda t: t.double()  # noqa: E731
    sd = {"cm.layer_norm.weight": d(cv["ln0"][0]), "cm.layer_norm.bias": d(cv["ln0"][1]),
          "cm.bottleneck.0.weight": d(cv["w1"]).reshape(2 * D, D, 1), "cm.bottleneck.0.bias": d(cv["b1"]),
          "cm.conv.weight": d(cv["taps"]).T.reshape(D, 1, K).contiguous(), "cm.conv.bias": d(cv["bc"]),
          "cm.after_conv.0.weight": d(cv["ln1"][0]), "cm.after_conv.0.bias": d(cv["ln1"][1]),
          "cm.after_conv.2.weight": d(cv["w2"]), "cm.after_conv.2.bias": d(cv["b2"])}
    for name, p in (("fa.", A), ("fb.", Bk)):
        sd.update({name + "0.weight": d(p["ln0"][0]), name + "0.bias": d(p["ln0"][1]),
                   name + "1.ffn.0.weight": d(p["w1"]), name + "1.ffn.0.bias": d(p["b1"]),
                   name + "1.ffn.3.weight": d(p["w2"]), name + "1.ffn.3.bias": d(p["b2"])})
    lnf = lambda t, p: F.layer_norm(t, (D,), d(p[0]), d(p[1]), p[2])  # noqa: E731
    xa = d(c["x"]) + d(cv["o"]) @ d(cv["wo"]).T + d(cv["bo"])
    mask = cv["kpm"].bool().reshape(B, T, 1) if masked else None
    xc = xa + OC.conv_module(xa.reshape(B, T, D), sd, "cm.", K, causal, mask).reshape(B * T, D)
    zp = lnf(xc + 0.5 * OC.ffn_module(xc, sd, "fa."), A["post_ln"])
    out = zp + 0.5 * OC.ffn_module(zp, sd, "fb.")
    got = R.reference(c, rounding=False)
    assert _rel(got["out"], out) <= 1e-12
    assert _rel(got["yp"], lnf(out, c["next_ln"]) @ d(c["wp"]).T) <= 1e-12
    assert _rel(R.reference(_tail_of(c), rounding=False)["u"], lnf(zp, c["next_ln"])) <= 1e-12


def test_anchor_src_and_mask():
    """The source Linear and the key-padding bytes, stated once more."""
    c = R.make_case("src_ffn_proj", "swish", 256, 256, 256, M=98, Kin=256, rel=True, post=False, seed=7)
    s = c["src"]
    x = s["a"].double() @ s["ws"].double().T + s["sbias"].double()
    got = R.reference(c, rounding=False)
    assert _rel(got["out"], _ffn64(x, c["A"]["ln0"], c["A"], 0.5, "swish", 256)) <= 1e-12
    lim = torch.floor(torch.tensor([1.0, 0.55]) * 49)
    assert torch.equal(got["kpm_out"], (torch.arange(49)[None].float() > lim[:, None]).to(torch.uint8).reshape(-1))
    assert int(got["kpm_out"].sum()) == 49 - 27  # floor(0.55 * 49) = 26: frames 27 .. 48 of the second utterance


# ---------------------------------------------------------------------- probes
def _probe_sample():
    import test_gpu_layer_terms as G
    return list(G.all_probes())[::9]


def test_probe_closed_form_is_the_reference():
    """probe_expected (closed form, then float64 LayerNorms) against the
    reference with rounding on: the exact stage bit for bit in float64 and in
    float32 (nothing rounds, the reciprocal square root's error included),
    the outputs behind further LayerNorms to 1e-12."""
    n = 0
    for c in _probe_sample():
        exp, exact = R.probe_expected(c)
        r64, r32 = R.reference(c), R.reference(c, dtype=torch.float32)
        assert set(exp) == set(r64)
        for name, e in exp.items():
            if name == "kpm_out" or name in exact:
                assert torch.equal(r64[name].double(), e.double()), (c["id"], name)
                assert torch.equal(r32[name].double(), e.double()), (c["id"], name, "float32")
                n += name in exact
            elif name == "yp":  # the selection of bf16(u): within half a bf16 step (at most 2^-8 |u|) of u
                assert bool(((r64[name] - e).abs() <= 2.0 ** -8 * e.abs() + 1e-12).all()), (c["id"], name)
                assert bool(((r32[name].double() - e).abs() <= 2.0 ** -8 * e.abs() + 1e-5).all()), (c["id"], name, "float32")
            else:
                assert _rel(r64[name], e) <= 1e-12, (c["id"], name)
                assert _rel(r32[name].double(), e) <= 1e-4, (c["id"], name, "float32")
    assert n >= 10


def test_probe_rows_and_columns_are_distinguishable():
    """Over the rows of a probe (M >= 8) no two rows and no two columns of the
    expected `out` agree; every hidden value is a bf16 number."""
    for c in (R.probe_case("ffn", "lrelu", 1024, 3, M=47), R.probe_case("ffn_proj", "none", 256, 0, M=97, np_=256),
              R.probe_case("src_ffn_proj", "none", 512, 1, M=50, np_=256, Kin=64)):  # 6-bit masks: rows repeat every 64 columns
        out = R.probe_expected(c)[0]["out"]
        assert len({tuple(r.tolist()) for r in out}) == out.shape[0]
        assert len({tuple(col.tolist()) for col in out.T}) == out.shape[1]
        p = c["A"]
        xn = R.rbf(R.ln(c["x"].double() if "x" in c else 4 * c["w"].double(), p["ln0"]))
        assert torch.equal(xn, c["w"].double() + p["ln0"][1].double())  # Xn = b0 + w_r exactly
        a = R.act_fn(xn @ p["w1"].double().T + p["b1"].double(), c["act"], c["slope"])
        assert torch.equal(R.rbf(a), a)


# ------------------------------------------------------------------------- E32
_E32 = {}


def _measured():
    if not _E32:
        for c in R.ref_cases():
            f = _E32.setdefault(R.family(c), {})
            for k, v in R.measure_e32(c).items():
                f[k] = max(f.get(k, 0.0), v)
    return _E32


def test_e32_table():
    """The table holds every family of the reference cases and is not below
    the deviation of the float32 evaluation re-measured here."""
    meas = _measured()
    assert set(meas) == set(R.E32)
    for fam, row in sorted(meas.items()):
        for name, v in row.items():
            print(f"{fam} {name}: measured {v:.2e}, table {R.E32[fam][name]:.2e}")
            assert R.E32[fam][name] >= v, (fam, name, v)


def test_bound_forms():
    """fp32: per tensor against max(1, max|ref|); bf16: one bf16 step of the
    reference element on top of it."""
    ref = torch.tensor([[4.0, 0.001, -2.0]], dtype=torch.float64)
    assert R.excess(ref + torch.tensor([[0.0, 3.9e-3, 0.0]]), ref, 1e-3, False)[0] == pytest.approx(0.975)
    assert R.excess(ref + torch.tensor([[0.0, 4.1e-3, 0.0]]), ref, 1e-3, False)[0] > 1.0
    assert R.excess(ref + torch.tensor([[4.0 * 2 ** -8 + 3.9e-3, 0.0, 0.0]]), ref, 1e-3, True)[0] < 1.0
    assert R.excess(ref + torch.tensor([[0.0, 4.1e-3, 0.0]]), ref, 1e-3, True)[0] > 1.0
    assert R.excess(ref * float("nan"), ref, 1e-3, False)[0] == float("inf")
    c = R.ref_cases()[0]
    assert R.bound(c, "out") == max(1e-5, 8 * R.E32[R.family(c)]["out"])


# ------------------------------------------------------------------ visibility
def _moved(c, term):
    """The largest share, over the compared outputs, of the rows the term
    reaches in which it moves the output by at least 4 times its bound."""
    ref = R.cached_reference(c)
    c2, kw = R.altered(c, term)
    alt = R.reference(c2, **kw)
    rows = R.reached_rows(c, term)
    best = 0.0
    for name, r in ref.items():
        if name == "kpm_out":
            continue
        big = max(1.0, float(r.abs().max()))
        lim = 4 * R.bound(c, name) * big
        if name in R.bf16_out(c):
            lim = lim + 4 * 2.0 ** -8 * r.abs()
        hit = ((alt[name] - r).abs() >= lim).any(dim=1)
        best = max(best, float(hit[rows].float().mean()))
    return best


def test_every_term_is_visible():
    """A condition on the inputs of test_gpu_layer_terms.py::test_reference,
    asserted for every case and every term it has: the share of the rows the
    term reaches (layer_ref.reached_rows) in which a compared output moves by
    at least 4 bounds is at least a half."""
    share, weak = {}, []
    for c in R.ref_cases():
        for term in R.terms(c):
            s = _moved(c, term)
            share.setdefault((c["launch"], term), []).append(s)
            if s < 0.5:
                weak.append((c["id"], term, round(s, 2)))
    for (launch, term), v in sorted(share.items()):
        print(f"{launch:15s} {term:14s} {len(v)} cases, smallest share {min(v):.2f}")
    assert not weak, weak
    expected = {"A.ln0_gain", "A.ln0_bias", "A.ln0_eps", "A.b1", "A.b2", "A.alpha", "A.act", "A.h64", "B.ln0_gain",
                "B.ln0_bias", "B.ln0_eps", "B.b1", "B.b2", "B.alpha", "B.act", "B.h64", "post.gain", "post.bias",
                "next.gain", "next.bias", "conv.bo", "conv.bc", "conv.b1_value", "conv.b1_gate", "conv.tap0",
                "conv.tapK", "conv.ln1_bias", "conv.b2", "conv.kpm", "conv.halo", "src.sbias"}
    assert {t for _, t in share} == expected


# --------------------------------------------------------------- instantiations
def test_every_instantiation_is_launched():
    import test_gpu_layer_terms as G
    ref = {R.instantiation(c) for c in R.ref_cases()}
    both = ref | {R.instantiation(c) for c in G.all_probes()}
    want = ({f"ffn_kernel<256, {a}, PROJ {p}, CHAIN {ch}>" for a in R.ACTS for p in (0, 1) for ch in (0, 1)}
            | {f"{k}<{a}>" for k in ("conv_chain_kernel", "conv_tail_kernel", "src_ffn_kernel") for a in R.ACTS})
    assert len(want) == 28 and both == want
    assert ref == want  # the reference cases alone reach all 28
    # the shapes the cases have to span
    cs = R.ref_cases()
    assert {c["M"] for c in cs if "conv" not in c and "src" not in c} == {48, 49, 97}
    assert {(c["conv"]["K"], c["conv"]["causal"]) for c in cs if "conv" in c} == {(31, False), (15, False), (31, True)}
    assert {c["np"] for c in cs if c["np"]} == {256, 768} and {c["deff"] for c in cs} == {256, 144}
    assert {c["H"] for c in cs if c["launch"] in ("ffn", "ffn_proj")} == {256, 1024, 2048}
    assert {c["H"] for c in cs if c["launch"] not in ("ffn", "ffn_proj", "src_ffn_proj")} == {256, 1024}
    assert any(c["conv"]["kpm"] is not None and 0 < int(c["conv"]["kpm"].sum()) < c["M"] for c in cs if "conv" in c)
