"""CPU checks of the time-domain augmentation drop-ins against
tests/golden/tdaug.npz, which the reference's CPU path wrote
(gen_tdaug_golden.py): the host draws, the polyphase tables, the combined
notch filters and the chunk tables are the reference's bit for bit; the
float64 restatement (tdaug_ref.py) reproduces the reference's outputs within
max(1e-6, 8 E32); the signatures are the reference's; the error cases raise;
and the check the GPU tests apply rejects modelled wrong kernels.
"""
import ctypes
import inspect
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdaug_ref as R  # noqa: E402

SPEEDS = (95, 105, 90, 110, 80, 50, 200)
# M, L, taps, first_indices[0], T_out at T = 257, measured on the reference
SIZES = {95: (20, 19, 13, -6, 245), 105: (20, 21, 13, -6, 270), 90: (10, 9, 14, -6, 232), 110: (10, 11, 13, -6, 283),
         80: (5, 4, 16, -7, 206), 50: (2, 1, 25, -12, 129), 200: (1, 2, 13, -6, 514)}
SEEDS = range(8)
DC_KW = dict(drop_length_low=10, drop_length_high=60, drop_count_low=0, drop_count_high=5)
DCS_KW = dict(drop_length_low=100, drop_length_high=200, drop_count_low=1, drop_count_high=3)


@pytest.fixture(scope="module")
def g(golden):
    return golden("tdaug")


def _resampler(speed):
    from speechbrain_amd.processing.speech_augmentation import Resample
    m = Resample(16000, 16000 * speed // 100)
    m._indices_and_weights()
    return m


def _close(got, r64, r32):
    bad = R.mismatch(got, r64, r32)
    assert bad is None, bad


def test_signatures(g):
    from speechbrain_amd.lobes.augment import TimeDomainSpecAugment
    from speechbrain_amd.processing import speech_augmentation as SA
    for cls in (SA.Resample, SA.SpeedPerturb, SA.DropFreq, SA.DropChunk, TimeDomainSpecAugment):
        for fn in ("__init__", "forward"):
            have = [[p.name, p.kind.name, "<empty>" if p.default is inspect.Parameter.empty else repr(p.default)]
                    for p in inspect.signature(getattr(cls, fn)).parameters.values()]
            assert have == json.loads(str(g[f"signature.{cls.__name__}.{fn}"])), (cls.__name__, fn)


@pytest.mark.parametrize("speed", SPEEDS)
def test_resample_table_bit_for_bit(g, speed):
    m = _resampler(speed)
    M, L, W, f0, t257 = SIZES[speed]
    assert (m.conv_stride, m.output_samples, m.weights.shape[1], int(m.first_indices[0])) == (M, L, W, f0)
    assert m._output_samples(257) == t257
    assert np.array_equal(m.first_indices.numpy(), g[f"rs.{speed}.first"])
    assert np.array_equal(m.weights.numpy(), g[f"rs.{speed}.weights"])
    for T in (1, 12, 257, 1000):
        assert m._output_samples(T) == g[f"rs.{speed}.T{T}.C1"].shape[1]


@pytest.mark.parametrize("speed", SPEEDS)
def test_restatement_resample(g, speed):
    m = _resampler(speed)
    for T in (1, 12, 257, 1000):
        for C in (1, 2):
            x, want = g[f"rs.x.T{T}.C{C}"], g[f"rs.{speed}.T{T}.C{C}"]
            args = (x, m.first_indices.numpy(), m.weights.numpy(), m.conv_stride, want.shape[1])
            _close(want, R.resample(*args), R.resample(*args, dtype=np.float32))


def test_speed_perturb_draws(g):
    from speechbrain_amd.processing.speech_augmentation import SpeedPerturb
    m = SpeedPerturb(16000, speeds=[95, 100, 105])
    for s in SEEDS:
        torch.manual_seed(s)
        m.last_draws = m.draws()
        assert np.array_equal(R.flat_draws(m), g[f"sp.{s}.draws"])
        rs = m.resamplers[m.last_draws[1]]
        assert rs._output_samples(300) == g[f"sp.{s}.out"].shape[1]


def test_drop_freq_draws_filter_and_restatement(g):
    from speechbrain_amd.processing.speech_augmentation import DropFreq
    m = DropFreq(drop_count_low=0, drop_count_high=3)
    counts = set()
    for s in SEEDS:
        torch.manual_seed(s)
        m.last_draws = m.draws()
        assert np.array_equal(R.flat_draws(m), g[f"df.{s}.draws"])
        taps = m.last_draws[3].numpy()
        assert taps.dtype == np.float32 and np.array_equal(taps, g[f"df.{s}.filter"])
        counts.add(int(m.last_draws[1]))
        _close(g[f"df.{s}.out"], R.fir101(g["df.x"], taps), R.fir101(g["df.x"], taps, np.float32))
    assert {0, 3} <= counts


def _noise_tables(segs, noise):
    noff = np.zeros(segs.shape[:2], np.int64)
    flat, o = [], 0
    for i, vs in enumerate(noise):
        for j, v in enumerate(vs):
            noff[i, j] = o
            flat.append(v.numpy())
            o += len(v)
    return noff, np.concatenate(flat) if flat else None


@pytest.mark.parametrize("key,kw,nf", [("dc", DC_KW, 0.0), ("dcn", DC_KW, 0.5), ("dcs", DCS_KW, 0.0)])
def test_drop_chunk_draws_tables_and_restatement(g, key, kw, nf):
    from speechbrain_amd.processing.speech_augmentation import DropChunk
    m = DropChunk(noise_factor=nf, **kw)
    src = "dcs" if key == "dcs" else "dc"
    x, lens = g[f"{src}.x"], torch.from_numpy(g[f"{src}.lens"])
    T = x.shape[1]
    lengths = (lens * T).long()
    past = False
    for s in SEEDS:
        torch.manual_seed(s)
        m.last_draws = _, times, chunks, noise = m.draws(lengths)
        assert np.array_equal(R.flat_draws(m), g[f"{key}.{s}.draws"])
        segs = m.segments(chunks, T)
        want = g[f"{key}.{s}.out"]
        if segs is None:
            assert np.array_equal(want, x)
            continue
        segs = segs.numpy()
        past |= any(int(c[0][j]) + int(c[1][j]) > T for c in chunks if c is not None for j in range(len(c[0])))
        assert segs[..., 1].max() <= T
        if not nf:
            # the table against the reference's output: zero exactly there
            assert np.array_equal(R.drop_chunks(x, segs, dtype=np.float32), want)
        else:
            noff, flat = _noise_tables(segs, noise)
            args = dict(noise=flat, noff=noff, lengths=lengths.numpy(), noise_factor=nf)
            _close(want, R.drop_chunks(x, segs, **args), R.drop_chunks(x, segs, dtype=np.float32, **args))
    if key == "dcs":
        assert past, "no chunk passed the end of the utterance"


def test_time_domain_spec_augment_draws_and_restatement(g):
    from speechbrain_amd.lobes.augment import TimeDomainSpecAugment
    m = TimeDomainSpecAugment(speeds=[95, 100, 105])
    x, lens = g["td.x"], torch.from_numpy(g["td.lens"])
    for s in SEEDS:
        torch.manual_seed(s)
        rs, T_out, taps, segs = m.draws(x.shape[1], lens)
        assert np.array_equal(R.flat_draws(m), g[f"td.{s}.draws"])
        want = g[f"td.{s}.out"]
        assert want.shape == (3, T_out)
        assert (rs is not None) == (f"td.{s}.s1" in g.files)
        assert (taps is not None) == (f"td.{s}.s2" in g.files)
        table = taps_n = segs_n = None
        if rs is not None:
            table = (rs.first_indices.numpy(), rs.weights.numpy(), rs.conv_stride, T_out)
            _close(g[f"td.{s}.s1"], R.chain(x, table), R.chain(x, table, dtype=np.float32))
        if taps is not None:
            taps_n = taps.numpy()
            assert np.array_equal(taps_n, g[f"td.{s}.filter"])
            _close(g[f"td.{s}.s2"], R.chain(x, table, taps_n), R.chain(x, table, taps_n, dtype=np.float32))
        if segs is not None:
            segs_n = segs.numpy()
            for b in range(3):
                for s0, e0 in segs_n[b]:
                    assert not want[b, s0:e0].any()
        _close(want, R.chain(x, table, taps_n, segs_n), R.chain(x, table, taps_n, segs_n, dtype=np.float32))


def test_error_cases():
    from speechbrain_amd._lib import SbkError
    from speechbrain_amd.lobes.augment import TimeDomainSpecAugment
    from speechbrain_amd.processing.speech_augmentation import DropChunk, DropFreq, Resample, SpeedPerturb
    x = torch.zeros(2, 300)
    for m, args in ((Resample(16000, 8000), (x,)), (Resample(), (x,)), (SpeedPerturb(16000), (x,)), (DropFreq(), (x,)),
                    (DropChunk(), (x, torch.ones(2))), (TimeDomainSpecAugment(), (x, torch.ones(2)))):
        with pytest.raises(SbkError):  # no CPU fallback
            m(*args)
    for kw in (dict(drop_length_low=5, drop_length_high=4), dict(drop_count_low=3, drop_count_high=2),
               dict(drop_start=10, drop_end=5)):
        with pytest.raises(ValueError):
            DropChunk(**kw)
    m = DropChunk(drop_length_low=100, drop_length_high=1000, drop_start=10, drop_end=50)
    assert (m.drop_length_low, m.drop_length_high) == (40, 40)
    # drop_start past a short utterance: the start's randint has an empty range
    with pytest.raises(RuntimeError):
        DropChunk(drop_length_low=10, drop_length_high=20, drop_start=200).draws(torch.tensor([100]))
    # a chunk whose end passes T is clipped at T, and one longer than the
    # utterance starts at 0
    torch.manual_seed(0)
    d = DropChunk(drop_length_low=150, drop_length_high=150, drop_count_low=1, drop_count_high=1)
    _, _, chunks, _ = d.draws(torch.tensor([100]))
    assert d.segments(chunks, 100).tolist() == [[[0, 100]]]


def test_entry_points_refuse_bad_arguments():
    """Argument errors return SBK_ERR_ARG before any launch (no GPU needed)."""
    from speechbrain_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from speechbrain_amd import _build
        _build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sbk_tdaug_tile", "sbk_resample", "sbk_fir101", "sbk_drop_chunks", "sbk_tdaug"):
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    assert lib.sbk_tdaug_tile() > 0
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.sbk_resample(None, 1, 8, 1, p, p, 1, 1, 1, 8, p, None) == 1001          # null input
    assert lib.sbk_resample(p, 1, 0, 1, p, p, 1, 1, 1, 8, p, None) == 1001             # T <= 0
    assert lib.sbk_resample(p, 1, 8, 1, p, p, 64, 1, 33, 8, p, None) == 1001           # table wider than the LDS plan
    assert lib.sbk_resample(p, 1, 8, 1, p, p, 129, 1, 1, 8, p, None) == 1001
    assert lib.sbk_fir101(p, 1, 8, None, p, None) == 1001
    assert lib.sbk_fir101(p, 1, 0, p, p, None) == 1001
    assert lib.sbk_drop_chunks(p, 1, 8, 1, None, 1, None, None, 0, None, 0.0, None, None, p, None) == 1001
    assert lib.sbk_drop_chunks(p, 1, 8, 1, p, 65, None, None, 0, None, 0.0, None, None, p, None) == 1001
    assert lib.sbk_drop_chunks(p, 1, 8, 2, p, 1, p, p, 8, p, 0.5, p, p, p, None) == 1001  # noise with channels
    assert lib.sbk_tdaug(p, 1, 8, None, None, 0, 1, 0, 9, None, None, 0, p, None) == 1001  # no resample, T_out != T
    assert lib.sbk_tdaug(p, 1, 8, p, None, 1, 1, 1, 8, None, None, 0, p, None) == 1001
    assert lib.sbk_tdaug(p, 1, 0, None, None, 0, 1, 0, 0, None, None, 0, p, None) == 1001


# ------------------------------------------------ the checker rejects wrong kernels

def _case():
    rng = np.random.default_rng(0)
    m = _resampler(95)
    T = 1000
    x = rng.uniform(-1, 1, (2, T)).astype(np.float32)
    table = (m.first_indices.numpy(), m.weights.numpy(), m.conv_stride, m._output_samples(T))
    taps = (rng.uniform(-1, 1, 101) * np.hanning(101) / 8).astype(np.float32)
    return x, table, taps


@pytest.mark.parametrize("fault", ["phase", "sign", "truncate"])
def test_checker_rejects_wrong_resample(fault):
    x, table, _ = _case()
    good, g32 = R.resample(x, *table), R.resample(x, *table, dtype=np.float32)
    assert R.mismatch(g32, good, g32) is None
    assert R.mismatch(R.resample(x, *table, dtype=np.float32, fault=fault), good, g32) is not None


def test_checker_rejects_truncated_last_window_only_at_the_end():
    """The truncation fault touches nothing but the last partial windows."""
    x, table, _ = _case()
    good = R.resample(x, *table, dtype=np.float32)
    bad = R.resample(x, *table, dtype=np.float32, fault="truncate")
    differs = np.flatnonzero((good != bad).any(0))
    assert 0 < len(differs) <= 13 and differs.min() >= good.shape[1] - 13


def test_checker_rejects_flipped_filter():
    x, _, taps = _case()
    good, g32 = R.fir101(x, taps), R.fir101(x, taps, np.float32)
    assert R.mismatch(g32, good, g32) is None
    assert R.mismatch(R.fir101(x, taps, np.float32, fault="flip"), good, g32) is not None


def test_checker_rejects_extrapolated_halo():
    x, table, taps = _case()
    good, g32 = R.chain(x, table, taps), R.chain(x, table, taps, dtype=np.float32)
    assert R.mismatch(g32, good, g32) is None
    assert R.mismatch(R.chain(x, table, taps, dtype=np.float32, fault="halo"), good, g32) is not None


def test_checker_rejects_unclipped_chunk_end():
    x, _, _ = _case()
    T = x.shape[1]
    clipped = np.array([[[T - 20, T]], [[0, 0]]])
    unclipped = np.array([[[T - 20, T + 30]], [[0, 0]]])
    good = R.drop_chunks(x, clipped)
    g32 = R.drop_chunks(x, clipped, dtype=np.float32)
    assert R.mismatch(g32, good, g32) is None
    assert R.mismatch(R.drop_chunks(x, unclipped, dtype=np.float32, fault="noclip"), good, g32) is not None
