"""Generate tests/golden/losses.npz from the REAL reference's ctc_loss,
kldiv_loss and nll_loss (speechbrain/nnet/losses.py) on the CPU.

    python tests/golden/gen_losses_golden.py

Runs only where the reference checkout is present (as gen_golden.py); the
committed losses.npz is what the tests read.  torchaudio, hyperpyyaml and
ruamel.yaml are absent here and unused by the losses, so inert stubs stand in
for them before `import speechbrain`.

Keys
  ctc{i}.logits / .lp (= log_softmax(logits), fp32) (B, T, V), .targets (B, L)
  int64, .ilen / .tlen relative lengths fp32, .blank;
  ctc{i}.{red}.out, .{red}.go (the grad_output used), .{red}.grad (wrt lp),
  .{red}.grad_logits (wrt logits, through the log-softmax) for red in
  mean | sum | none | batch | batchmean.  Gradients are omitted where the
  reference's own result is not finite ("batch" divides by a zero target
  length).
  seq{i}.lp, .targets, .length (absent = None), .pad_idx;
  seq{i}.{fn}.ls{0|1}.{red}.out / .go / .grad for fn in kldiv | nll; a
  combination the reference itself raises on is absent and listed in
  seq{i}.raises.
Before writing, every stored value is checked against the same computation in
float64: they must agree to 1e-5 (|a-b| <= 1e-5·max(1,|b|)), which leaves the
suite's 1e-4 bound ten times that.
"""
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
from speechbrain.nnet import losses as RL  # noqa: E402

CTC_REDS = ("mean", "sum", "none", "batch", "batchmean")
SEQ_REDS = ("mean", "batchmean", "batch", "sum", "none")


def _go(out):
    if out.dim() == 0:
        return torch.ones((), dtype=out.dtype)
    return torch.linspace(0.5, 1.5, out.numel(), dtype=out.dtype).reshape(out.shape)


def _agree(a, b, what):
    a, b = a.double().numpy(), b.double().numpy()
    fin = np.isfinite(b)
    ok = np.array_equal(a[~fin], b[~fin], equal_nan=True) & (np.isfinite(a) == fin)
    err = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
    assert ok.all() and (err.size == 0 or err.max() <= 1e-5), (what, err.max() if err.size else None)


def _ctc_run(logits, targets, ilen, tlen, blank, red, dtype):
    x = logits.detach().clone().to(dtype).requires_grad_()
    lp = x.log_softmax(-1)
    lp.retain_grad()
    out = RL.ctc_loss(lp, targets, ilen, tlen, blank, reduction=red)
    go = _go(out.detach())
    out.backward(go)
    return out.detach(), go, lp.grad, x.grad


def ctc_cases():
    g = torch.Generator().manual_seed(1234)
    cases = []
    # T <= 6 (brute-force checkable): repeat, L = 0, input_len < T, infeasible (3 + 2 repeats > 4)
    for blank in (0, 4):
        lab = [1, 2, 3] if blank == 0 else [0, 1, 2]
        a, b, c = lab
        targets = torch.tensor([[a, a, b], [c, c, c], [b, c, a], [c, c, c]])
        logits = torch.randn(4, 6, 5, generator=g)
        ilen = torch.tensor([1.0, 1.0, 0.5, 0.66])     # 6, 6, 3, round(3.96) = 4
        tlen = torch.tensor([1.0, 0.0, 0.67, 1.0])     # 3, 0, round(2.01) = 2, 3
        cases.append((logits, targets, ilen, tlen, blank))
    # V = 37, T = 20: relative lengths rounding up and down, input_len = 1, L = 0, infeasible, repeats
    for blank in (0, 36):
        lo = 1 if blank == 0 else 0
        targets = torch.randint(lo, lo + 36, (4, 7), generator=g)
        targets[0, 2] = targets[0, 1]                  # repeated label
        targets[3, :] = targets[3, 0]                  # 6 repeats: 7 + 6 > 10 frames, infeasible
        logits = 0.5 * torch.randn(4, 20, 37, generator=g)  # scaled: fp32 and fp64 torch agree to 1e-5
        ilen = torch.tensor([0.73, 0.05, 1.0, 0.52])   # round(14.6) = 15, 1, 20, round(10.4) = 10
        tlen = torch.tensor([0.65, 0.143, 0.0, 1.0])   # round(4.55) = 5, round(1.001) = 1, 0, 7
        cases.append((logits, targets, ilen, tlen, blank))
    return cases


def gen_ctc(out):
    for i, (logits, targets, ilen, tlen, blank) in enumerate(ctc_cases()):
        k = f"ctc{i}"
        out[k + ".logits"] = logits.numpy()
        out[k + ".lp"] = logits.log_softmax(-1).numpy()
        out[k + ".targets"] = targets.numpy()
        out[k + ".ilen"] = ilen.numpy()
        out[k + ".tlen"] = tlen.numpy()
        out[k + ".blank"] = np.int64(blank)
        for red in CTC_REDS:
            o32, go, glp32, gx32 = _ctc_run(logits, targets, ilen, tlen, blank, red, torch.float32)
            o64, _, glp64, gx64 = _ctc_run(logits, targets, ilen.double(), tlen.double(), blank, red, torch.float64)
            _agree(o32, o64, (k, red, "out"))
            out[f"{k}.{red}.out"] = o32.numpy()
            out[f"{k}.{red}.go"] = go.numpy()
            if torch.isfinite(glp64).all() and torch.isfinite(gx64).all():
                _agree(glp32, glp64, (k, red, "grad"))
                _agree(gx32, gx64, (k, red, "grad_logits"))
                out[f"{k}.{red}.grad"] = glp32.numpy()
                out[f"{k}.{red}.grad_logits"] = gx32.numpy()
            else:
                print(f"{k} {red}: reference gradient not finite, omitted")


def seq_cases():
    g = torch.Generator().manual_seed(4321)

    def mk(B, U, V, Ut=None, two_d=False):
        if two_d:
            lp = torch.randn(B, V, generator=g).log_softmax(-1)
            tg = torch.randint(0, V, (B,), generator=g)
            tg[1] = 0
            return lp, tg
        lp = torch.randn(B, U, V, generator=g).log_softmax(-1)
        tg = torch.randint(1, V, (B, Ut or U), generator=g)
        tg[0, -2:] = 0   # pad_idx rows
        tg[2, 1] = 0
        return lp, tg

    return [
        (*mk(3, 6, 11), torch.tensor([1.0, 0.5, 0.67])),   # equal lengths, masked
        (*mk(3, 8, 11, Ut=6), torch.tensor([1.0, 0.5, 0.67])),   # predictions 2 longer
        (*mk(3, 6, 11, Ut=8), torch.tensor([1.0, 0.5, 0.67])),   # targets 2 longer
        (*mk(5, 0, 11, two_d=True), None),                 # 2-D
        (*mk(3, 6, 11), None),                             # 3-D, no length
    ]


def gen_seq(out):
    fns = {"kldiv": lambda lp, tg, ln, ls, red: RL.kldiv_loss(lp, tg, ln, label_smoothing=ls, pad_idx=0, reduction=red),
           "nll": lambda lp, tg, ln, ls, red: RL.nll_loss(lp, tg, ln, label_smoothing=ls, reduction=red)}
    for i, (lp, tg, ln) in enumerate(seq_cases()):
        k = f"seq{i}"
        out[k + ".lp"] = lp.numpy()
        out[k + ".targets"] = tg.numpy()
        if ln is not None:
            out[k + ".length"] = ln.numpy()
        out[k + ".pad_idx"] = np.int64(0)
        raises = []
        for fn, f in fns.items():
            for li, ls in enumerate((0.0, 0.1)):
                for red in SEQ_REDS:
                    res = []
                    try:
                        for dt in (torch.float32, torch.float64):
                            x = lp.detach().clone().to(dt).requires_grad_()
                            o = f(x, tg, None if ln is None else ln.to(dt), ls, red)
                            go = _go(o.detach())
                            o.backward(go)
                            res.append((o.detach(), go, x.grad))
                    except Exception as e:  # the reference's own refusal of this combination
                        raises.append(f"{fn}.ls{li}.{red}")
                        print(f"{k} {fn} ls={ls} {red}: reference raises {type(e).__name__}")
                        continue
                    _agree(res[0][0], res[1][0], (k, fn, ls, red, "out"))
                    _agree(res[0][2], res[1][2], (k, fn, ls, red, "grad"))
                    out[f"{k}.{fn}.ls{li}.{red}.out"] = res[0][0].numpy()
                    out[f"{k}.{fn}.ls{li}.{red}.go"] = res[0][1].numpy()
                    out[f"{k}.{fn}.ls{li}.{red}.grad"] = res[0][2].numpy()
        out[k + ".raises"] = np.array(raises, dtype="U32")


if __name__ == "__main__":
    out = {}
    gen_ctc(out)
    gen_seq(out)
    path = os.path.join(OUT, "losses.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
