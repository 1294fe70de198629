"""Generate tests/golden/tdaug.npz from the REAL reference's CPU path.

Runs only where the reference is checked out (see gen_golden.py, whose stubs
for the three absent, unused packages it repeats); the committed .npz is what
the tests read.

    python tests/golden/gen_tdaug_golden.py

Inventory (float32 unless noted; `draws` is float64 and holds, in call order,
every value torch.rand / torch.randint returned during the forward):
  signature.{class}.{__init__|forward}
                                 JSON [[parameter, kind, repr(default) | "<empty>"], ...]
  rs.x.T{T}.C{C}                 inputs of the Resample cases, |x| <= 1
  rs.{speed}.first / .weights    Resample._indices_and_weights
  rs.{speed}.T{T}.C{C}           Resample(16000, 16000 * speed // 100) output
  sp.x, sp.{seed}.draws / .out   SpeedPerturb(16000, [95, 100, 105])
  df.x, df.{seed}.draws / .filter / .out
                                 DropFreq(drop_count_low=0, drop_count_high=3)
  dc.x, dc.lens, dc.{seed}.draws / .out            DropChunk, zero fill
  dcn.{seed}.draws / .out        the same with noise_factor 0.5
  dcs.x, dcs.lens, dcs.{seed}.draws / .out
                                 T = 150 with chunks of 100..200 samples
  td.x, td.lens, td.{seed}.draws / .filter / .s1 / .s2 / .out
                                 TimeDomainSpecAugment(speeds=[95, 100, 105])
                                 on (3, 4000); s1 / s2 (after the speed and
                                 the frequency stage) are stored only where
                                 they differ from the stage before
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

torch.set_num_threads(8)

from speechbrain.processing import speech_augmentation as SA  # noqa: E402
from speechbrain.lobes.augment import TimeDomainSpecAugment  # noqa: E402

SPEEDS = (95, 105, 90, 110, 80, 50, 200)
SEEDS = range(8)


def t2n(x):
    return x.detach().cpu().numpy().astype(np.float32)


class Recorder:
    """Logs what torch.rand / torch.randint return, and the kernel of every
    convolve1d call, while the reference runs."""

    def __enter__(self):
        self.draws, self.kernels = [], []
        self._rand, self._randint, self._conv = torch.rand, torch.randint, SA.convolve1d

        def rand(*a, **k):
            v = self._rand(*a, **k)
            self.draws.append(v.detach().double().reshape(-1).numpy().copy())
            return v

        def randint(*a, **k):
            v = self._randint(*a, **k)
            self.draws.append(v.detach().double().reshape(-1).numpy().copy())
            return v

        def conv(waveform, kernel, *a, **k):
            self.kernels.append(t2n(kernel).reshape(-1))
            return self._conv(waveform, kernel, *a, **k)

        torch.rand, torch.randint, SA.convolve1d = rand, randint, conv
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randint, SA.convolve1d = self._rand, self._randint, self._conv

    def flat(self):
        return np.concatenate(self.draws) if self.draws else np.zeros(0)


def wave(shape, seed, lens=None):
    """Uniform in [-1, 1], zero past each row's relative length."""
    x = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    if lens is not None:
        for b, r in enumerate(lens):
            x[b, int(r * shape[1]):] = 0
    return x


def signature(fn):
    return np.array(json.dumps(
        [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
         for p in inspect.signature(fn).parameters.values()]))


def main():
    out = {}
    for cls in (SA.Resample, SA.SpeedPerturb, SA.DropFreq, SA.DropChunk, TimeDomainSpecAugment):
        for fn in ("__init__", "forward"):
            out[f"signature.{cls.__name__}.{fn}"] = signature(getattr(cls, fn))
    # Resample: the table and the outputs at seven rates
    for T in (1, 12, 257, 1000):
        out[f"rs.x.T{T}.C1"] = t2n(wave((2, T), 100 + T))
        out[f"rs.x.T{T}.C2"] = t2n(wave((1, T, 2), 200 + T))
    for speed in SPEEDS:
        m = SA.Resample(16000, 16000 * speed // 100)
        for T in (1, 12, 257, 1000):
            for C in (1, 2):
                out[f"rs.{speed}.T{T}.C{C}"] = t2n(m(torch.from_numpy(out[f"rs.x.T{T}.C{C}"])))
        out[f"rs.{speed}.first"] = t2n(m.first_indices)
        out[f"rs.{speed}.weights"] = t2n(m.weights)

    def run(key, module, *args):
        for seed in SEEDS:
            torch.manual_seed(seed)
            with Recorder() as rec:
                y = module(*args)
            out[f"{key}.{seed}.draws"] = rec.flat()
            out[f"{key}.{seed}.out"] = t2n(y)
            if rec.kernels:
                out[f"{key}.{seed}.filter"] = rec.kernels[-1]

    out["sp.x"] = t2n(wave((2, 300), 1))
    run("sp", SA.SpeedPerturb(16000, speeds=[95, 100, 105]), torch.from_numpy(out["sp.x"]))
    out["df.x"] = t2n(wave((2, 300), 2))
    run("df", SA.DropFreq(drop_count_low=0, drop_count_high=3), torch.from_numpy(out["df.x"]))
    lens = torch.tensor([1.0, 0.75, 0.5])
    out["dc.x"] = t2n(wave((3, 400), 3, lens))
    out["dc.lens"] = t2n(lens)
    kw = dict(drop_length_low=10, drop_length_high=60, drop_count_low=0, drop_count_high=5)
    run("dc", SA.DropChunk(**kw), torch.from_numpy(out["dc.x"]), lens)
    run("dcn", SA.DropChunk(noise_factor=0.5, **kw), torch.from_numpy(out["dc.x"]), lens)
    slens = torch.tensor([1.0, 0.8])
    out["dcs.x"] = t2n(wave((2, 150), 4, slens))
    out["dcs.lens"] = t2n(slens)
    run("dcs", SA.DropChunk(drop_length_low=100, drop_length_high=200, drop_count_low=1, drop_count_high=3),
        torch.from_numpy(out["dcs.x"]), slens)

    # TimeDomainSpecAugment at the recipe arguments, stage by stage
    tlens = torch.tensor([1.0, 0.6, 0.35])
    out["td.x"] = t2n(wave((3, 4000), 5, tlens))
    out["td.lens"] = t2n(tlens)
    td = TimeDomainSpecAugment(speeds=[95, 100, 105])
    stages = {}
    for name in ("speed_perturb", "drop_freq"):
        getattr(td, name).register_forward_hook(lambda m, i, o, name=name: stages.__setitem__(name, t2n(o)))
    x = torch.from_numpy(out["td.x"])
    speeds, notches, chunks = set(), set(), set()
    for seed in SEEDS:
        torch.manual_seed(seed)
        with Recorder() as rec:
            y = td(x, tlens)
        d = rec.flat()
        out[f"td.{seed}.draws"] = d
        out[f"td.{seed}.filter"] = rec.kernels[-1]
        out[f"td.{seed}.out"] = t2n(y)
        if not np.array_equal(stages["speed_perturb"], out["td.x"]):
            out[f"td.{seed}.s1"] = stages["speed_perturb"]
        if not np.array_equal(stages["drop_freq"], stages["speed_perturb"]):
            out[f"td.{seed}.s2"] = stages["drop_freq"]
        # draws: rand, speed index, rand, notch count, frequencies, rand, chunk counts (3), ...
        speeds.add(int(d[1]))
        notches.add(int(d[3]))
        chunks.update(int(c) for c in d[5 + int(d[3]):8 + int(d[3])])
    assert speeds == {0, 1, 2}, speeds
    assert {0, 3} <= notches, notches
    assert {0, 5} <= chunks, chunks

    path = os.path.join(OUT, "tdaug.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
