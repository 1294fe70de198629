"""Generate tests/golden/w2v_objective.npz from the REAL reference's wav2vec 2.0
pre-training pieces on the CPU: GumbelVectorQuantizer (nnet/quantisers.py),
W2VTargetQuantiser, compute_mask, sample_negatives
(lobes/models/wav2vec.py) and ContrastiveLoss (nnet/losses.py).

    python tests/golden/gen_w2v_golden.py

Runs only where the reference checkout is present (as gen_losses_golden.py,
with the same inert stubs for the packages the reference imports and these
pieces do not use); the committed w2v_objective.npz is what the tests read.

Keys
  init.gvq.{key} / init.tq.{key}: state dicts after torch.manual_seed(0) of
    GumbelVectorQuantizer(24, 10, (2.0, 0.25, 0.999995), 2, 16) and
    W2VTargetQuantiser(24, 16, num_vars=10).
  temp.steps / temp.values: update_temp of that quantiser.
  mask{i}.seed / .shape / .lens / .prob / .length / .mask: compute_mask after
    random.seed(seed); np.random.seed(seed).  mask2 has unequal lengths and
    takes the "add missing indices" branch (asserted here).
  outlen.in / outlen.out: W2VLatentExtractor.get_output_lengths (defaults).
  neg{i}.seed / .B / .T / .N / .idx: the flat row indices sample_negatives
    drew after torch.manual_seed(seed), recovered from its output on a tensor
    whose rows are their own row numbers.
  loss{i}.x / .y (B, T, C), .idx (B, T·N), .temp, .go (grad_output scalar),
    .loss, .acc, .logits (T·B, N+1; the reference's row order is (t, b)),
    .dx; .dy_index: y's gradient when negs = y.view(-1, C)[idx] is built from
    y (the index mode's gradient); .dy_float / .dnegs: gradients with negs a
    separate leaf (the float mode's).  .dnegs_sel: the negatives whose dnegs
    rows are stored (all of them unless the tensor would be large).
    loss1 has duplicated target rows (neg_is_pos) and an utterance of equal
    rows, whose negatives all equal the positive: row loss 0, zero gradients.
  vq{i}.vars / .weight / .bias / .x (B, T, in), .tau, .groups;
    .eval.out / .cp / .pp, and for L = sum(out·gout) + 0.7·pp:
    .gout, .eval.dvars / .dweight / .dx;
    .train.logits (fp32, what the reference's weight_proj gave), .train.gumbels
    (the noise F.gumbel_softmax drew: drawn here first with the same call
    after the same seed), .train.out / .cp / .pp / .dlogits / .dvars.
Conditions asserted on the inputs (seeds are re-drawn until they hold): in
every (row, group) the top-2 gap of logits and of logits + gumbels exceeds
1e-3; in every loss row the two largest distinct finite logits differ by more
than 1e-3 (negatives are drawn with replacement, so a row repeats candidates:
copies of one candidate share one logit exactly and decide nothing); no
zero-norm rows.  Before writing, every stored value is checked
against a float64 run of the same computation: |a-b| <= 1e-5·max(1,|b|).
"""
import os
import random
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
from speechbrain.lobes.models import wav2vec as RW  # noqa: E402
from speechbrain.nnet import losses as RL  # noqa: E402
from speechbrain.nnet.quantisers import GumbelVectorQuantizer as RefGVQ  # noqa: E402

GAP = 1e-3


def _agree(a, b, what):
    a, b = a.detach().double().numpy(), b.detach().double().numpy()
    fin = np.isfinite(b)
    ok = np.array_equal(a[~fin], b[~fin], equal_nan=True) & (np.isfinite(a) == fin).all()
    err = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
    assert ok and (err.size == 0 or err.max() <= 1e-5), (what, err.max() if err.size else None)


# ------------------------------------------------------------------ modules
def gen_init(out):
    torch.manual_seed(0)
    q = RefGVQ(24, 10, (2.0, 0.25, 0.999995), 2, 16)
    for k, v in q.state_dict().items():
        out["init.gvq." + k] = v.numpy()
    torch.manual_seed(0)
    tq = RW.W2VTargetQuantiser(24, 16, num_vars=10)
    for k, v in tq.state_dict().items():
        out["init.tq." + k] = v.numpy()
    steps = [0, 1, 1000, 100000, 10000000]
    vals = []
    for s in steps:
        q.update_temp(s)
        vals.append(q.curr_temp)
    out["temp.steps"] = np.array(steps, dtype=np.int64)
    out["temp.values"] = np.array(vals, dtype=np.float64)
    lens = torch.tensor([400, 16000, 31999, 240000])
    ns = types.SimpleNamespace(kernel_sizes=[11, 3, 3, 3, 3, 3, 3], strides=[5, 2, 2, 2, 2, 2, 2])
    out["outlen.in"] = lens.numpy()
    out["outlen.out"] = RW.W2VLatentExtractor.get_output_lengths(ns, lens).numpy()


def gen_masks(out):
    cases = [(3, (2, 40), [40, 40], 0.65, 10), (11, (3, 50), [50, 50, 50], 0.3, 4), (5, (3, 60), [60, 41, 33], 0.65, 10)]
    for i, (seed, shape, lens, prob, length) in enumerate(cases):
        random.seed(seed)
        np.random.seed(seed)
        mask = RW.compute_mask(shape, lens, prob, length)
        k = f"mask{i}"
        out[k + ".seed"] = np.int64(seed)
        out[k + ".shape"] = np.array(shape, dtype=np.int64)
        out[k + ".lens"] = np.array(lens, dtype=np.int64)
        out[k + ".prob"] = np.float64(prob)
        out[k + ".length"] = np.int64(length)
        out[k + ".mask"] = mask
        if i == 2:
            # the top-up branch ran iff some sample's spans overlapped: then its row
            # holds frames outside every span-start window; replay to be sure
            random.seed(seed)
            np.random.seed(seed)
            num_mask = int(prob * min(lens) / float(length) + random.random() + 1)
            short = False
            for n in lens:
                st = np.random.choice(n - length, num_mask, replace=False)
                fr = np.unique((st[:, None] + np.arange(length)[None]).reshape(-1))
                short |= len(fr[fr < n]) < num_mask * length
            assert short, "mask2 does not exercise the add-missing-indices branch"
            assert (mask.sum(1) == num_mask * length).all()


def ref_indices(seed, B, T, N):
    """The reference's draw as flat row indices (B, T*N), from its output."""
    ids = torch.arange(B * T, dtype=torch.float32).view(B, T, 1)
    torch.manual_seed(seed)
    negs = RW.sample_negatives(ids, N)  # (N, B, T, 1)
    return negs[..., 0].permute(1, 2, 0).reshape(B, T * N).long()


def gen_negs(out):
    for i, (seed, B, T, N) in enumerate([(0, 2, 2, 3), (1, 3, 7, 5), (2, 3, 7, 100), (3, 1, 5, 4), (4, 4, 9, 2)]):
        k = f"neg{i}"
        idx = ref_indices(seed, B, T, N)
        out[k + ".seed"], out[k + ".B"], out[k + ".T"], out[k + ".N"] = (np.int64(v) for v in (seed, B, T, N))
        out[k + ".idx"] = idx.numpy()
        if (B, T) == (3, 7):
            # the b·(T-1) offset: utterance b's window starts b rows early
            assert idx[2].min() >= 2 * 6 and idx[2].max() <= 2 * 6 + 6 and (idx[1] < 7).any()


# --------------------------------------------------------------------- loss
def _loss_run(x, y, idx, N, temp, go, dtype, tie_y):
    """The reference's loss with negs gathered from y by idx.  tie_y: negs is
    built from y (index-mode gradient); otherwise negs is a separate leaf."""
    B, T, C = x.shape
    x = x.detach().clone().to(dtype).requires_grad_()
    y = y.detach().clone().to(dtype).requires_grad_()
    if tie_y:
        negs = y.view(-1, C)[idx.view(-1)].view(B, T, N, C).permute(2, 0, 1, 3)
    else:
        negs = y.detach().view(-1, C)[idx.view(-1)].view(B, T, N, C).permute(2, 0, 1, 3).clone().requires_grad_()
    loss, acc = RL.ContrastiveLoss(temp)(x, y, negs)
    (loss * go).backward()
    return loss.detach(), acc.detach(), x.grad, y.grad, None if tie_y else negs.grad


def _ref_logits(x, y, idx, N, temp):
    B, T, C = x.shape
    negs = y.view(-1, C)[idx.view(-1)].view(B, T, N, C).permute(2, 0, 1, 3)
    nip = (y == negs).all(-1)
    lg = torch.cosine_similarity(x.double(), torch.cat([y.unsqueeze(0), negs], 0).double(), dim=-1)
    lg[1:][nip] = float("-inf")
    return lg.transpose(0, 2).reshape(-1, N + 1) / temp


def _loss_inputs_ok(x, y, idx, N, temp):
    if (x.norm(dim=-1) == 0).any() or (y.norm(dim=-1) == 0).any():
        return False
    lg = _ref_logits(x, y, idx, N, temp) * temp
    for row in lg:
        # negatives are drawn with replacement (and quantised targets repeat), so a
        # row holds the same candidate several times: such copies have one logit
        # bit for bit and cannot change the loss, the arg-max test or a gradient.
        # The gap is asked of the two largest DISTINCT finite values.
        top = torch.unique(row[torch.isfinite(row)]).flip(0)
        if top.numel() > 1 and not float(top[0] - top[1]) > GAP:
            return False
    return True


def gen_losses(out):
    #        B  T  C    N    temp go    dup
    cases = [(2, 7, 24, 5, 0.1, 1.0, False),
             (2, 7, 24, 5, 0.1, 2.5, True),
             (3, 7, 256, 100, 0.1, 1.0, False),
             (2, 2, 24, 3, 0.1, 0.5, False),
             (1, 5, 6, 4, 0.5, 1.0, False)]
    for i, (B, T, C, N, temp, go, dup) in enumerate(cases):
        for seed in range(100 * i, 100 * i + 100):
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(B, T, C, generator=g)
            if dup:  # quantised-looking targets: few distinct rows; utterance 0 one row throughout
                book = torch.randn(5, C, generator=g)
                y = book[torch.randint(0, 5, (B, T), generator=g)]
                y[0] = book[0]
            else:
                y = torch.randn(B, T, C, generator=g)
            idx = ref_indices(seed, B, T, N)
            if _loss_inputs_ok(x, y, idx, N, temp):
                break
        else:
            raise AssertionError(f"loss{i}: no seed satisfies the input conditions")
        k = f"loss{i}"
        print(f"{k}: seed {seed}")
        r32 = _loss_run(x, y, idx, N, temp, go, torch.float32, True)
        r64 = _loss_run(x, y, idx, N, temp, go, torch.float64, True)
        f32 = _loss_run(x, y, idx, N, temp, go, torch.float32, False)
        f64 = _loss_run(x, y, idx, N, temp, go, torch.float64, False)
        for a, b, w in zip(r32[:4] + f32[2:], r64[:4] + f64[2:], ("loss", "acc", "dx", "dy_index", "dx_f", "dy_float",
                                                                  "dnegs")):
            _agree(a, b, (k, w))
        _agree(f32[0], r32[0], (k, "loss float vs index"))
        lg32 = _ref_logits(x, y, idx, N, temp).float()
        if dup:
            nip = ~torch.isfinite(lg32)
            assert nip.any() and nip[:, 1:].all(-1).any(), "dup case lacks neg_is_pos / an all-equal row"
            assert float(r32[2][0].abs().max()) == 0.0  # zero gradient on the all-equal utterance
        sel = list(range(N)) if N * B * T * C <= 20000 else [0, N // 2 + 7, N - 1]
        out[k + ".x"], out[k + ".y"], out[k + ".idx"] = x.numpy(), y.numpy(), idx.numpy()
        out[k + ".temp"], out[k + ".go"] = np.float64(temp), np.float64(go)
        out[k + ".loss"], out[k + ".acc"] = r32[0].numpy(), r32[1].numpy()
        out[k + ".logits"] = lg32.numpy()
        out[k + ".dx"], out[k + ".dy_index"] = r32[2].numpy(), r32[3].numpy()
        out[k + ".dy_float"] = f32[3].numpy()
        out[k + ".dnegs_sel"] = np.array(sel, dtype=np.int64)
        out[k + ".dnegs"] = f32[4][sel].numpy()


# ---------------------------------------------------------------- quantiser
def _vq_restated(logits, gumbels, vars_, tau, G):
    """quantisers.py:86-122 in the dtype of its inputs, the noise injected.
    logits (Rq*G, V); vars_ (G*V, D).  Returns (out (Rq, G*D), cp, pp)."""
    M, V = logits.shape
    Rq = M // G
    k = logits.max(-1)[1]
    hard = torch.zeros_like(logits).scatter_(-1, k.view(-1, 1), 1.0).view(Rq, G, V)
    hp = hard.mean(0)
    cp = torch.exp(-torch.sum(hp * torch.log(hp + 1e-7), dim=-1)).sum()
    ap = torch.softmax(logits.view(Rq, G, V), dim=-1).mean(0)
    pp = torch.exp(-torch.sum(ap * torch.log(ap + 1e-7), dim=-1)).sum()
    if gumbels is not None:
        ys = ((logits + gumbels) / tau).softmax(-1)
        yh = torch.zeros_like(logits).scatter_(-1, ys.max(-1, keepdim=True)[1], 1.0)
        sel = yh - ys.detach() + ys
    else:
        sel = hard.view(M, V)
    o = (sel.reshape(Rq, G * V).unsqueeze(-1) * vars_.unsqueeze(0)).view(Rq, G, V, -1).sum(-2)
    return o.reshape(Rq, -1), cp, pp


def _gaps_ok(t):
    top = torch.topk(t, 2, dim=-1).values
    return bool(((top[:, 0] - top[:, 1]) > GAP).all())


def gen_vq(out):
    #        B  T  in  V    G  vq   tau
    cases = [(2, 5, 24, 10, 2, 16, 2.0), (2, 5, 24, 320, 2, 256, 0.5), (1, 4, 12, 6, 3, 12, 1.3)]
    for i, (B, T, fin, V, G, vq, tau) in enumerate(cases):
        for seed in range(1000 + 100 * i, 1100 + 100 * i):
            torch.manual_seed(seed)
            q = RefGVQ(fin, V, (tau, 0.25, 0.999995), G, vq)
            x = torch.randn(B, T, fin)
            gout = torch.randn(B, T, vq)
            with torch.no_grad():
                logits = q.weight_proj(x.reshape(-1, fin)).view(B * T * G, V)
            torch.manual_seed(seed + 7)
            gumbels = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
            if _gaps_ok(logits) and _gaps_ok(logits + gumbels):
                break
        else:
            raise AssertionError(f"vq{i}: no seed satisfies the input conditions")
        k = f"vq{i}"
        print(f"{k}: seed {seed}")
        out[k + ".vars"] = q.vars.detach()[0].numpy()
        out[k + ".weight"] = q.weight_proj.weight.detach().numpy()
        out[k + ".bias"] = q.weight_proj.bias.detach().numpy()
        out[k + ".x"], out[k + ".gout"] = x.numpy(), gout.numpy()
        out[k + ".tau"], out[k + ".groups"] = np.float64(tau), np.int64(G)
        for mode in ("eval", "train"):
            q.train(mode == "train")
            q.zero_grad()
            got = {}

            def keep(mod, args, o):
                o.retain_grad()
                got["logits"] = o

            h = q.weight_proj.register_forward_hook(keep)
            xr = x.clone().requires_grad_()
            torch.manual_seed(seed + 7)  # the module's F.gumbel_softmax draws what was drawn above
            res = q(xr)
            h.remove()
            (torch.sum(res["x"] * gout) + 0.7 * res["prob_perplex"]).backward()
            lg = got["logits"]
            # float64 restatement with the same logits (and noise)
            l64 = lg.detach().double().view(B * T * G, V).requires_grad_()
            v64 = q.vars.detach()[0].double().requires_grad_()
            o64, cp64, pp64 = _vq_restated(l64, gumbels.double() if mode == "train" else None, v64, tau, G)
            (torch.sum(o64 * gout.double().view(B * T, -1)) + 0.7 * pp64).backward()
            _agree(res["x"].reshape(B * T, -1), o64, (k, mode, "out"))
            _agree(res["code_perplexity"], cp64, (k, mode, "cp"))
            _agree(res["prob_perplex"], pp64, (k, mode, "pp"))
            _agree(lg.grad.view(B * T * G, V), l64.grad, (k, mode, "dlogits"))
            _agree(q.vars.grad[0], v64.grad, (k, mode, "dvars"))
            p = f"{k}.{mode}."
            out[p + "out"] = res["x"].detach().numpy()
            out[p + "cp"] = res["code_perplexity"].detach().numpy()
            out[p + "pp"] = res["prob_perplex"].detach().numpy()
            out[p + "dvars"] = q.vars.grad[0].numpy().copy()
            if mode == "eval":
                out[p + "dweight"] = q.weight_proj.weight.grad.numpy().copy()
                out[p + "dx"] = xr.grad.numpy()
            else:
                out[p + "logits"] = lg.detach().view(B * T * G, V).numpy()
                out[p + "gumbels"] = gumbels.numpy()
                out[p + "dlogits"] = lg.grad.view(B * T * G, V).numpy().copy()


if __name__ == "__main__":
    out = {}
    gen_init(out)
    gen_masks(out)
    gen_negs(out)
    gen_losses(out)
    gen_vq(out)
    path = os.path.join(OUT, "w2v_objective.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
