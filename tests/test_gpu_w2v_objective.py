"""The wav2vec 2.0 pre-training objective on HIP (csrc/w2vloss.hip) against
the reference fixture tests/golden/w2v_objective.npz: ContrastiveLoss in its
two negs modes (values, accuracy, gradients, neg_is_pos, determinism), the
GumbelVectorQuantizer in eval and training mode, and one recipe step
(train_sb_wav2vec2.py:37-120) against its restatement with torch ops on the
CPU.  Values and gradients at the suite's 1e-4 (conftest.assert_close)."""
import copy
import random

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu

LOSS_CASES = [0, 1, 2, 3, 4]  # (2,7,24,5), the same with duplicated targets, (3,7,256,100), (2,2,24,3), (1,5,6,4)
VQ_CASES = [0, 1, 2]          # (B,T,in,V,G,vq) = (2,5,24,10,2,16), (2,5,24,320,2,256), (1,4,12,6,3,12)


@pytest.fixture(scope="module")
def g(golden):
    return golden("w2v_objective")


def _t(a, dev=None):
    t = torch.from_numpy(np.asarray(a))
    return t if dev is None else t.to(dev)


_runs = {}


def _loss_run(g, i, dev, mode):
    """One forward + backward of ContrastiveLoss on fixture case i, cached.
    mode: "index" | "float" (negs a permuted view, as sample_negatives gives
    it) | "float_c" (contiguous negs)."""
    if (i, mode) in _runs:
        return _runs[i, mode]
    from speechbrain_amd.nnet.losses import ContrastiveLoss
    k = f"loss{i}"
    x = _t(g[k + ".x"], dev).requires_grad_()
    y = _t(g[k + ".y"], dev).requires_grad_()
    idx = _t(g[k + ".idx"], dev)
    B, T, C = x.shape
    N = idx.shape[1] // T
    if mode == "index":
        negs = idx
    else:
        negs = y.detach().view(-1, C)[idx.view(-1)].view(B, T, N, C).permute(2, 0, 1, 3)
        negs = (negs.contiguous() if mode == "float_c" else negs).detach().requires_grad_()
    loss, acc = ContrastiveLoss(float(g[k + ".temp"]))(x, y, negs)
    (loss * float(g[k + ".go"])).backward()
    r = {"loss": loss.detach(), "acc": acc.detach(), "dx": x.grad, "dy": y.grad,
         "dnegs": None if mode == "index" else negs.grad, "x": x, "y": y, "negs": negs}
    _runs[i, mode] = r
    return r


@pytest.mark.parametrize("mode", ["index", "float", "float_c"])
@pytest.mark.parametrize("i", LOSS_CASES)
def test_contrastive_loss_vs_reference(g, dev, i, mode):
    k = f"loss{i}"
    r = _loss_run(g, i, dev, mode)
    assert r["loss"].dtype == torch.float32 and r["loss"].dim() == 0
    assert_close(r["loss"], g[k + ".loss"], name="loss")
    assert abs(float(r["acc"]) - float(g[k + ".acc"])) < 1e-6
    assert_close(r["dx"], g[k + ".dx"], name="dx")
    if mode == "index":
        assert_close(r["dy"], g[k + ".dy_index"], name="dy")
    else:
        assert_close(r["dy"], g[k + ".dy_float"], name="dy")
        sel = _t(g[k + ".dnegs_sel"], dev)
        assert r["dnegs"].shape == r["negs"].shape
        assert_close(r["dnegs"][sel], g[k + ".dnegs"], name="dnegs")


@pytest.mark.parametrize("i", LOSS_CASES)
def test_negs_modes_agree(g, dev, i):
    a, b, c = (_loss_run(g, i, dev, m) for m in ("index", "float", "float_c"))
    for o in (b, c):
        assert_close(o["loss"], a["loss"], rtol=1e-6, name="loss")
        assert float(o["acc"]) == float(a["acc"])
        assert_close(o["dx"], a["dx"], rtol=1e-6, name="dx")
    # index mode's dy = float mode's positive term + the scatter of dnegs
    k = f"loss{i}"
    y = a["y"]
    idx = _t(g[k + ".idx"], dev)
    B, T, C = y.shape
    N = idx.shape[1] // T
    scat = torch.zeros(B * T, C, device=dev, dtype=torch.float64)
    scat.index_add_(0, idx.view(-1), b["dnegs"].permute(1, 2, 0, 3).reshape(-1, C).double())
    assert_close(a["dy"], (b["dy"].double() + scat.view(B, T, C)).float(), name="dy index vs float")


@pytest.mark.parametrize("i", LOSS_CASES)
def test_logits_rows_and_accuracy(g, dev, i):
    from speechbrain_amd import _w2v
    k = f"loss{i}"
    x, y, idx = (_t(g[k + n], dev) for n in (".x", ".y", ".idx"))
    B, T, C = x.shape
    N = idx.shape[1] // T
    with torch.no_grad():
        rowloss, correct, logits = _w2v.contrastive_rows(x, y, idx, float(g[k + ".temp"]))
    ref = _t(g[k + ".logits"]).view(T, B, N + 1).transpose(0, 1).reshape(B * T, N + 1)  # the reference's rows are (t, b)
    got = logits.cpu()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin) and bool((got[~fin] == float("-inf")).all())
    assert_close(got[fin], ref[fin], name="logits")
    ref_rows = torch.logsumexp(ref.double(), -1) - ref[:, 0].double()
    assert_close(rowloss, ref_rows.float(), name="row losses")
    assert torch.equal(correct.cpu() > 0, ref.argmax(-1) == 0)


def test_neg_is_pos_rows(g, dev):
    """loss1: quantised-looking targets.  Utterance 0 is one row repeated, so
    every negative of its rows equals the positive: -inf logits, row loss 0,
    zero gradients."""
    from speechbrain_amd import _w2v
    k = "loss1"
    x, y, idx = (_t(g[k + n], dev) for n in (".x", ".y", ".idx"))
    T = x.shape[1]
    with torch.no_grad():
        rowloss, correct, logits = _w2v.contrastive_rows(x, y, idx, float(g[k + ".temp"]))
    assert bool((logits[:T, 1:] == float("-inf")).all()) and bool(torch.isfinite(logits[:, 0]).all())
    assert bool((rowloss[:T] == 0).all()) and bool((correct[:T] == 1).all())
    assert bool(torch.isinf(logits[T:, 1:]).any())  # duplicates in utterance 1 as well
    for mode in ("index", "float"):
        r = _loss_run(g, 1, dev, mode)
        assert float(r["dx"][0].abs().max()) == 0.0
    r = _loss_run(g, 1, dev, "float")
    assert float(r["dy"][0].abs().max()) == 0.0 and float(r["dnegs"][:, 0].abs().max()) == 0.0
    assert bool(torch.isfinite(r["dnegs"]).all()) and bool(torch.isfinite(_loss_run(g, 1, dev, "index")["dy"]).all())


def test_index_backward_is_deterministic(g, dev):
    from speechbrain_amd.nnet.losses import ContrastiveLoss
    k = "loss2"
    idx = _t(g[k + ".idx"], dev)
    grads = []
    for _ in range(2):
        x = _t(g[k + ".x"], dev).requires_grad_()
        y = _t(g[k + ".y"], dev).requires_grad_()
        loss, _ = ContrastiveLoss(float(g[k + ".temp"]))(x, y, idx)
        loss.backward()
        grads.append((x.grad.clone(), y.grad.clone(), loss.detach().clone()))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_grad_scaler_scaled_loss(g, dev):
    from speechbrain_amd.nnet.losses import ContrastiveLoss
    k = "loss0"
    assert float(g[k + ".go"]) == 1.0
    x = _t(g[k + ".x"], dev).requires_grad_()
    y = _t(g[k + ".y"], dev).requires_grad_()
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    loss, _ = ContrastiveLoss(float(g[k + ".temp"]))(x, y, _t(g[k + ".idx"], dev))
    scaler.scale(loss).backward()
    assert_close(x.grad / 1024.0, g[k + ".dx"], name="dx")
    assert_close(y.grad / 1024.0, g[k + ".dy_index"], name="dy")


def test_loss_is_fp32_under_bf16_autocast(g, dev):
    from speechbrain_amd.nnet.losses import ContrastiveLoss
    k = "loss0"
    x, y, idx = (_t(g[k + n], dev) for n in (".x", ".y", ".idx"))
    xb, yb = x.bfloat16(), y.bfloat16()
    want, _ = ContrastiveLoss(0.1)(xb.float(), yb.float(), idx)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got, acc = ContrastiveLoss(0.1)(xb, yb, idx)
    assert got.dtype == torch.float32 and acc.dtype == torch.float32 and torch.equal(got, want)


# ---------------------------------------------------------------- quantiser
def _vq_module(g, i, dev):
    from speechbrain_amd.nnet.quantisers import GumbelVectorQuantizer
    k = f"vq{i}"
    w, v = g[k + ".weight"], g[k + ".vars"]
    G = int(g[k + ".groups"])
    m = GumbelVectorQuantizer(w.shape[1], w.shape[0] // G, (float(g[k + ".tau"]), 0.25, 0.999995), G, v.shape[1] * G)
    m.load_state_dict({"vars": _t(v)[None], "weight_proj.weight": _t(w), "weight_proj.bias": _t(g[k + ".bias"]),
                       "max_ent": m.max_ent.data}, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("i", VQ_CASES)
def test_quantiser_eval_module(g, dev, i):
    k = f"vq{i}"
    m = _vq_module(g, i, dev).eval()
    x = _t(g[k + ".x"], dev).requires_grad_()
    res = m(x)
    assert res["num_vars"] == m.num_vars * m.groups and res["temp"] == m.curr_temp
    assert_close(res["x"], g[k + ".eval.out"], name="out")
    assert_close(res["code_perplexity"], g[k + ".eval.cp"], name="code_perplexity")
    assert_close(res["prob_perplex"], g[k + ".eval.pp"], name="prob_perplex")
    (torch.sum(res["x"] * _t(g[k + ".gout"], dev)) + 0.7 * res["prob_perplex"]).backward()
    assert_close(m.vars.grad[0], g[k + ".eval.dvars"], name="dvars")
    assert_close(m.weight_proj.weight.grad, g[k + ".eval.dweight"], name="dweight")
    assert_close(x.grad, g[k + ".eval.dx"], name="dx")


@pytest.mark.parametrize("i", VQ_CASES)
def test_quantiser_training_op_with_stored_noise(g, dev, i):
    k = f"vq{i}"
    m = _vq_module(g, i, dev).train()
    logits = _t(g[k + ".train.logits"], dev).requires_grad_()
    out, cp, pp = m.quantise(logits, _t(g[k + ".train.gumbels"], dev))
    gout = _t(g[k + ".gout"], dev)
    assert_close(out, g[k + ".train.out"].reshape(out.shape), name="out")
    assert_close(cp, g[k + ".train.cp"], name="code_perplexity")
    assert_close(pp, g[k + ".train.pp"], name="prob_perplex")
    (torch.sum(out * gout.view(out.shape)) + 0.7 * pp).backward()
    assert_close(logits.grad, g[k + ".train.dlogits"], name="dlogits")
    assert_close(m.vars.grad[0], g[k + ".train.dvars"], name="dvars")


def test_quantiser_backward_is_deterministic(g, dev):
    k = "vq1"
    m = _vq_module(g, 1, dev).train()
    gout = _t(g[k + ".gout"], dev)
    grads = []
    for _ in range(2):
        m.zero_grad()
        logits = _t(g[k + ".train.logits"], dev).requires_grad_()
        out, _, pp = m.quantise(logits, _t(g[k + ".train.gumbels"], dev))
        (torch.sum(out * gout.view(out.shape)) + 0.7 * pp).backward()
        grads.append((logits.grad.clone(), m.vars.grad.clone(), pp.detach().clone()))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_quantiser_argmax_tie_picks_lowest_index(dev):
    """Identical weight_proj rows — 3 and 7 (codes 3 and 7 of group 0), 12 and
    15 (codes 2 and 5 of group 1) — give bit-equal winning logits: the lower
    code is chosen, as torch's max does on the CPU."""
    from speechbrain_amd.nnet.quantisers import GumbelVectorQuantizer
    torch.manual_seed(5)
    m = GumbelVectorQuantizer(12, 10, (2.0, 0.25, 0.999995), 2, 8)
    with torch.no_grad():
        for r in (3, 7, 12, 15):
            m.weight_proj.weight[r] = 5.0
    m = m.to(dev).eval()
    x = torch.rand(2, 6, 12, device=dev) + 0.1  # positive inputs: the all-5 rows win by far
    want = torch.cat([m.vars[0, 3], m.vars[0, 10 + 2]]).expand(12, -1)
    with torch.no_grad():
        res = m(x)
        # the same tie handed to the kernel directly
        lg = torch.randn(24, 10, device=dev)
        lg[0::2, 3] = lg[0::2, 7] = 9.0
        lg[1::2, 2] = lg[1::2, 5] = 9.0
        out, cp, _ = m.quantise(lg)
    assert torch.equal(res["x"].reshape(12, -1), want)
    assert torch.equal(out, want)
    assert_close(cp, 2.0, name="code_perplexity")  # one code per group: exp(0) + exp(0)


def test_quantiser_training_draw_is_gumbel_softmax_draw(dev):
    """The module draws its noise as F.gumbel_softmax does, from torch's
    generator on the logits' device: the same calls under the same seed, fed
    to quantise(), give the module's output bit for bit."""
    from speechbrain_amd.nnet.quantisers import GumbelVectorQuantizer
    torch.manual_seed(2)
    m = GumbelVectorQuantizer(12, 10, (2.0, 0.25, 0.999995), 2, 8).to(dev).train()
    x = torch.randn(2, 6, 12, device=dev)
    with torch.no_grad():
        torch.manual_seed(77)
        res = m(x)
        m.eval()
        hard = m(x)
        m.train()
        lin = m.weight_proj
        from speechbrain_amd import _autograd as A
        logits = A.linear(x.reshape(-1, 12), lin.weight, lin.bias, torch.float32, m._wc, "vq_proj").view(24, 10)
        torch.manual_seed(77)
        gumbels = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
        out, cp, pp = m.quantise(logits, gumbels)
    assert torch.equal(res["x"].reshape(12, -1), out) and torch.equal(res["prob_perplex"], pp)
    assert not torch.equal(res["x"], hard["x"])  # the noise changed some codes
    ref = F.one_hot(((logits + gumbels) / 2.0).argmax(-1), 10).float().view(12, 20)
    want = (ref.unsqueeze(-1) * m.vars[0]).view(12, 2, 10, -1).sum(-2).view(12, -1)
    assert_close(out, want, name="selected rows")


# -------------------------------------------------------------- recipe step
def _ref_step(ext, wrap, feat_proj, tq, wavs, wav_lens, mask, idx, N, temp, div_w):
    """compute_forward / compute_objectives (train_sb_wav2vec2.py:37-120) with
    torch ops, fp32, CPU; the modules only hold the weights."""
    from test_gpu_mha_general import _ref_layer
    B = wavs.shape[0]
    h = wavs.unsqueeze(2)  # normalize_signal=False
    for i in range(len(ext.kernel_sizes)):
        convs = getattr(ext.extractor, f"convblock_{i}").convs
        h = F.gelu(convs.norm_0.norm(convs.conv_0.conv(h.transpose(1, -1)).transpose(1, -1)))
    latents = ext.norm(h)
    T = latents.shape[1]
    e = wrap.input_projector(latents).clone()
    e[mask] = wrap.mask_emb
    pad = ~(torch.arange(T)[None, :] < torch.round(wav_lens * T)[:, None])
    e = e + wrap.positional_encoding.pe[:, :T]
    for layer in wrap.latent_encoder.layers:
        e, _ = _ref_layer(layer, e, None, pad, None)
    e = wrap.latent_encoder.norm.norm(e)
    emb = F.linear(e[mask], feat_proj.w.weight, feat_proj.w.bias).view(B, -1, feat_proj.w.out_features)
    lat = latents[mask].view(B, -1, latents.size(2))
    # eval-mode quantiser (quantisers.py:75-123) and its projection
    q = tq.quantiser
    lg = q.weight_proj(lat.reshape(-1, lat.size(2))).view(-1, q.num_vars)
    hard = torch.zeros_like(lg).scatter_(-1, lg.max(-1)[1].view(-1, 1), 1.0)
    avg = torch.softmax(lg.view(-1, q.groups, q.num_vars), dim=-1).mean(0)
    pp = torch.exp(-torch.sum(avg * torch.log(avg + 1e-7), dim=-1)).sum()
    qx = (hard.view(-1, q.groups * q.num_vars).unsqueeze(-1) * q.vars).view(-1, q.groups, q.num_vars, q.vars.shape[-1])
    targets = tq.proj(qx.sum(-2).view(B, -1, q.vq_dim))
    nv = q.groups * q.num_vars
    div = (nv - pp) / nv
    # sample_negatives + ContrastiveLoss (losses.py:1217-1251)
    M, C = targets.shape[1], targets.shape[2]
    negs = targets.reshape(-1, C)[idx.view(-1)].view(B, M, N, C).permute(2, 0, 1, 3)
    nip = (targets == negs).all(-1)
    lgt = torch.cosine_similarity(emb, torch.cat([targets.unsqueeze(0), negs], 0), dim=-1)
    lgt[1:][nip] = float("-inf")
    lgt = lgt.transpose(0, 2).reshape(-1, N + 1)
    loss = F.cross_entropy(lgt / temp, torch.zeros(lgt.size(0), dtype=torch.long), reduction="sum")
    acc = torch.sum(lgt.argmax(-1) == 0) / lgt.size(0)
    return loss + div * div_w * mask.sum(), acc


def test_recipe_step_vs_torch_restatement(dev):
    from speechbrain_amd.lobes.models.transformer.Transformer import TransformerEncoder
    from speechbrain_amd.lobes.models.wav2vec import (EncoderWrapper, W2VLatentExtractor, W2VTargetQuantiser,
                                                      compute_mask, sample_negative_indices)
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.losses import ContrastiveLoss
    torch.manual_seed(11)
    random.seed(11)
    np.random.seed(11)
    N, temp, div_w = 5, 0.1, 0.1
    ext = W2VLatentExtractor(out_channels=[16, 24, 24], kernel_sizes=[11, 3, 3], strides=[5, 2, 2])
    enc = TransformerEncoder(num_layers=2, nhead=4, d_ffn=64, d_model=32, activation=nn.GELU, normalize_before=True)
    wrap = EncoderWrapper(24, 32, enc)
    feat_proj = Linear(16, input_size=32)
    tq = W2VTargetQuantiser(24, 16, num_vars=10)
    mods = nn.ModuleList([ext, wrap, feat_proj, tq]).eval()  # eval-mode quantiser, no dropout
    ref = copy.deepcopy(mods)
    wavs = torch.randn(2, 1500)
    wavs[1, 1200:] = 0
    wav_lens = torch.tensor([1.0, 0.8])
    lens = [int(v) for v in ext.get_output_lengths(torch.tensor([1500, 1200]))]
    mask = torch.as_tensor(compute_mask((2, max(lens)), lens, 0.5, 4), dtype=torch.bool)
    M = int(mask[0].sum())
    torch.manual_seed(12)
    idx = sample_negative_indices(torch.empty(2, M, 16), N)
    want, want_acc = _ref_step(*ref, wavs, wav_lens, mask, idx, N, temp, div_w)
    want.backward()

    mods = mods.to(dev)
    ext, wrap, feat_proj, tq = mods
    wd, ld, md = wavs.to(dev), wav_lens.to(dev), mask.to(dev)
    # compute_forward
    latents = ext(wd, normalize_signal=False)
    results = wrap(latents, mask=md, wav_lens=ld)
    emb = feat_proj(results["embeddings"][md])
    emb = emb.view(2, -1, emb.size(1))
    targets, meta = tq(latents[md].view(2, -1, latents.size(2)))
    results.update(meta)
    # compute_objectives, negatives as indices (the fused path), the same CPU draw
    torch.manual_seed(12)
    negs = sample_negative_indices(targets, N)
    assert torch.equal(negs.cpu(), idx)
    loss, acc = ContrastiveLoss(temp)(emb, targets, negs)
    got = loss + results["diversity_loss"] * div_w * results["num_masked"]
    got.backward()
    assert_close(got, want, name="backprop_loss")
    assert float(acc) == float(want_acc)
    r_ext, r_wrap, r_fp, r_tq = ref
    assert_close(wrap.mask_emb.grad, r_wrap.mask_emb.grad, name="d mask_emb")
    assert_close(feat_proj.w.weight.grad, r_fp.w.weight.grad, name="d feat_proj.weight")
    assert_close(tq.proj.weight.grad, r_tq.proj.weight.grad, name="d target_quantiser.proj.weight")
    c0 = "convblock_0"
    assert_close(getattr(ext.extractor, c0).convs.conv_0.conv.weight.grad,
                 getattr(r_ext.extractor, c0).convs.conv_0.conv.weight.grad, name="d conv_0.weight")
