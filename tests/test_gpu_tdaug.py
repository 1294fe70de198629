"""GPU tests of the time-domain augmentation kernels (csrc/tdaug.hip) and
drop-ins.  Every operand sits inside NaN (int tables: INT_MAX) guard bands at
an odd element offset, and every output between sentinels: an output has to
be finite, fully written, and no sentinel outside it may move.

Exact probes: unit impulses through sbk_resample / sbk_fir101 give the table
entries bit for bit (each product is 1 * w); zero-fill sbk_drop_chunks is
compared bit for bit.  Values: against tests/golden/tdaug.npz (the
reference's CPU path) and the float64 restatement tdaug_ref.py within
max(1e-6, 8 E32).  The fused sbk_tdaug is bit-identical to the three kernels
in sequence.  Lengths sit around the kernels' tile (sbk_tdaug_tile()).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdaug_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 255  # odd: no operand is 16-byte aligned by accident
SENT = 12345.0
SPEEDS = (95, 105, 90, 110, 80, 50, 200)
SEEDS = range(8)
DC_KW = dict(drop_length_low=10, drop_length_high=60, drop_count_low=0, drop_count_high=5)


@pytest.fixture(scope="module")
def g(golden):
    return golden("tdaug")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def abi():
    from speechbrain_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def tile(abi):
    return abi.sbk_tdaug_tile()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_ALIVE = []  # operands of the launch in flight (Out.get drops them after its synchronise)


def _put(a, dev):
    """A host array inside guard bands on the device (None -> None); the
    tensor is kept alive until the launch's output has been read."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    ints = a.dtype.kind == "i"
    t = torch.from_numpy(a.astype(np.int32 if ints else np.float32)).reshape(-1)
    buf = torch.full((t.numel() + 2 * GUARD,), 2**31 - 1 if ints else float("nan"), dtype=t.dtype)
    buf[GUARD:GUARD + t.numel()] = t
    buf = buf.to(dev)
    _ALIVE.append(buf)
    return buf[GUARD:GUARD + t.numel()]


class Out:
    """An output buffer between sentinels."""

    def __init__(self, shape, dev):
        self.shape = tuple(shape)
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENT, device=dev)
        self.view = self.buf[GUARD:GUARD + self.n]

    def get(self, what):
        torch.cuda.synchronize()
        _ALIVE.clear()
        buf = self.buf.cpu().numpy()
        assert (buf[:GUARD] == SENT).all() and (buf[GUARD + self.n:] == SENT).all(), f"{what}: a sentinel moved"
        y = buf[GUARD:GUARD + self.n].reshape(self.shape)
        assert np.isfinite(y).all(), f"{what}: non-finite output (a guard band was read)"
        assert not (y == SENT).any(), f"{what}: an output element was not written"
        return y


def _table(speed):
    from speechbrain_amd.processing.speech_augmentation import Resample
    m = Resample(16000, 16000 * speed // 100)
    m._indices_and_weights()
    return m, m.first_indices.numpy().astype(np.int32), m.weights.numpy()


def _t_for(m, T_out):
    """(T, its output length): the shortest input that gives T_out outputs —
    or, where an upsampling rate skips T_out, the next length above it."""
    T = max(1, T_out * m.conv_stride // m.output_samples - 2)
    while m._output_samples(T) < T_out:
        T += 1
    if m.output_samples <= m.conv_stride:
        assert m._output_samples(T) == T_out
    return T, m._output_samples(T)


def run_resample(abi, dev, x, first, w, M, T_out, what="resample"):
    B, T = x.shape[:2]
    C = 1 if x.ndim == 2 else x.shape[2]
    out = Out((B, T_out) + x.shape[2:], dev)
    rc = abi.sbk_resample(_vp(_put(x, dev)), B, T, C, _vp(_put(first, dev)), _vp(_put(w, dev)), w.shape[0], M,
                          w.shape[1], T_out, _vp(out.view), None)
    assert rc == 0, f"{what}: rc {rc}"
    return out.get(what)


def run_fir(abi, dev, x, taps, what="fir101"):
    out = Out(x.shape, dev)
    rc = abi.sbk_fir101(_vp(_put(x, dev)), x.shape[0], x.shape[1], _vp(_put(taps, dev)), _vp(out.view), None)
    assert rc == 0, f"{what}: rc {rc}"
    return out.get(what)


def run_drop(abi, dev, x, segs, noise=None, noff=None, lengths=None, nf=0.0, what="drop_chunks"):
    B, T = x.shape[:2]
    C = 1 if x.ndim == 2 else x.shape[2]
    out = Out(x.shape, dev)
    amp = Out((B,), dev) if noise is not None else None
    partial = torch.empty(B * 64, device=dev) if noise is not None else None
    rc = abi.sbk_drop_chunks(_vp(_put(x, dev)), B, T, C, _vp(_put(segs, dev)), segs.shape[1], _vp(_put(noff, dev)),
                             _vp(_put(noise, dev)), 0 if noise is None else len(noise), _vp(_put(lengths, dev)), nf,
                             _vp(partial), _vp(amp.view) if amp else None, _vp(out.view), None)
    assert rc == 0, f"{what}: rc {rc}"
    return out.get(what), (amp.get(what + " amp") if amp else None)


def run_tdaug(abi, dev, x, table, taps, segs, what="tdaug"):
    B, T = x.shape
    first, w, M, T_out = table if table is not None else (None, None, 1, T)
    out = Out((B, T_out), dev)
    rc = abi.sbk_tdaug(_vp(_put(x, dev)), B, T, _vp(_put(first, dev)), _vp(_put(w, dev)),
                       0 if w is None else w.shape[0], M, 0 if w is None else w.shape[1], T_out, _vp(_put(taps, dev)),
                       _vp(_put(segs, dev)), 0 if segs is None else segs.shape[1], _vp(out.view), None)
    assert rc == 0, f"{what}: rc {rc}"
    return out.get(what)


def run_sequence(abi, dev, x, table, taps, segs):
    """Kernels 1 -> 2 -> 3, a dropped stage left out."""
    y = x
    if table is not None:
        y = run_resample(abi, dev, y, *table)
    if taps is not None:
        y = run_fir(abi, dev, y, taps)
    if segs is not None:
        y, _ = run_drop(abi, dev, y, segs)
    return y


def _close(got, r64, r32, what):
    bad = R.mismatch(got, r64, r32)
    assert bad is None, f"{what}: {bad}"


def _close_fixture(got, want, r64, r32, what):
    """`got` against the reference's float32 output `want`, within the bound
    of the restatement pair (r64, r32) of the same case."""
    _close(got, want.astype(np.float64), want + (np.asarray(r32, np.float64) - r64), what)


def _wave(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def _taps(seed):
    """Asymmetric taps of a plausible size."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, 101) * np.hanning(103)[1:-1] / 8).astype(np.float32)


# ------------------------------------------------------------------ exact probes

@pytest.mark.parametrize("speed", SPEEDS)
def test_resample_impulse_gives_the_table(abi, dev, speed):
    m, first, w = _table(speed)
    T, (L, W), M = 257, w.shape, m.conv_stride
    T_out = m._output_samples(T)
    n = np.arange(T_out)
    for p in (0, 100, T - 1):
        x = np.zeros((1, T), np.float32)
        x[0, p] = 1
        j = p - first[n % L] - (n // L) * M
        want = np.where((j >= 0) & (j < W), w[n % L, np.clip(j, 0, W - 1)], np.float32(0))[None]
        got = run_resample(abi, dev, x, first, w, M, T_out, f"impulse at {p}")
        assert np.array_equal(got, want), f"speed {speed}, impulse at {p}: differs at {np.flatnonzero(got != want)[:8]}"


def test_fir_impulse_gives_the_taps_in_correlation_order(abi, dev, tile):
    taps = _taps(1)
    T = tile + 1
    t = np.arange(T)
    for p in (0, 70, tile - 1, T - 1):
        x = np.zeros((1, T), np.float32)
        x[0, p] = 1
        k = p - t + 50
        want = np.where((k >= 0) & (k < 101), taps[np.clip(k, 0, 100)], np.float32(0))[None]
        got = run_fir(abi, dev, x, taps, f"impulse at {p}")
        assert np.array_equal(got, want), f"impulse at {p}: differs at {np.flatnonzero(got != want)[:8]}"


@pytest.mark.parametrize("B,C", [(1, 1), (3, 1), (3, 2)])
def test_drop_chunks_zero_fill_bit_for_bit(abi, dev, tile, B, C):
    for T in (1, tile // C - 1, tile // C, tile // C + 1, 2 * tile // C + 1):
        x = _wave((B, T) if C == 1 else (B, T, C), T)
        segs = np.zeros((B, 3, 2), np.int32)
        segs[0] = [[0, min(T, 7)], [T // 2, min(T, T // 2 + 40)], [max(0, T - 5), T]]
        if B > 1:
            segs[2, 1] = [T // 3, T // 3 + 1]
        got, _ = run_drop(abi, dev, x, segs, what=f"T {T}")
        assert np.array_equal(got, R.drop_chunks(x, segs, dtype=np.float32)), f"T {T}"


# ------------------------------------------------------------------------ values

@pytest.mark.parametrize("speed", SPEEDS)
def test_resample_fixture(abi, dev, g, speed):
    """T = 1 and T below the tap count included; C = 2."""
    m, first, w = _table(speed)
    for T in (1, 12, 257, 1000):
        for C in (1, 2):
            x, want = g[f"rs.x.T{T}.C{C}"], g[f"rs.{speed}.T{T}.C{C}"]
            args = (x, first, w, m.conv_stride, want.shape[1])
            got = run_resample(abi, dev, *args, what=f"T {T} C {C}")
            r64, r32 = R.resample(*args), R.resample(*args, dtype=np.float32)
            _close(got, r64, r32, f"speed {speed} T {T} C {C} vs restatement")
            _close_fixture(got, want, r64, r32, f"speed {speed} T {T} C {C} vs fixture")


@pytest.mark.parametrize("speed", (95, 50, 105))
@pytest.mark.parametrize("B,C", [(1, 1), (3, 1), (1, 2)])
def test_resample_tile_edges(abi, dev, tile, speed, B, C):
    m, first, w = _table(speed)
    nt = tile // C
    for T_out in (nt - 1, nt, nt + 1, 2 * nt + 1):
        T, T_out = _t_for(m, T_out)
        x = _wave((B, T) if C == 1 else (B, T, C), T_out)
        args = (x, first, w, m.conv_stride, T_out)
        _close(run_resample(abi, dev, *args, what=f"T_out {T_out}"), R.resample(*args),
               R.resample(*args, dtype=np.float32), f"speed {speed} T_out {T_out}")


@pytest.mark.parametrize("C", (1, 2))
def test_resample_span_past_the_lds_plan(abi, dev, tile, C):
    """16 kHz -> 4 kHz: a tile's input span (4 samples per output plus the
    window) no longer fits the staged span, so the kernel reads the row
    directly — the same sums, the other path."""
    m, first, w = _table(25)
    assert (tile // C) * m.conv_stride * C + w.shape[1] > 4096
    for T_out in (tile // C, 2 * (tile // C) + 1):
        T, _ = _t_for(m, T_out)
        x = _wave((2, T) if C == 1 else (2, T, C), T_out)
        args = (x, first, w, m.conv_stride, T_out)
        _close(run_resample(abi, dev, *args, what=f"T_out {T_out}"), R.resample(*args),
               R.resample(*args, dtype=np.float32), f"C {C} T_out {T_out}")


@pytest.mark.parametrize("B", (1, 3))
def test_fir_tile_edges(abi, dev, tile, B):
    taps = _taps(2)
    for T in (1, 50, tile - 1, tile, tile + 1, 2 * tile + 1):
        x = _wave((B, T), T)
        _close(run_fir(abi, dev, x, taps, f"T {T}"), R.fir101(x, taps), R.fir101(x, taps, np.float32), f"T {T}")


def test_fir_fixture(abi, dev, g):
    x = g["df.x"]
    for s in SEEDS:
        taps = g[f"df.{s}.filter"]
        r64, r32 = R.fir101(x, taps), R.fir101(x, taps, np.float32)
        got = run_fir(abi, dev, x, taps, f"seed {s}")
        _close(got, r64, r32, f"seed {s} vs restatement")
        _close_fixture(got, g[f"df.{s}.out"], r64, r32, f"seed {s} vs fixture")


def _noise_tables(segs, noise):
    noff = np.zeros(segs.shape[:2], np.int32)
    flat, o = [], 0
    for i, vs in enumerate(noise):
        for j, v in enumerate(vs):
            noff[i, j] = o
            flat.append(v.numpy())
            o += len(v)
    return noff, np.concatenate(flat)


def test_drop_chunks_noise_and_amplitude(abi, dev, g):
    from speechbrain_amd.processing.speech_augmentation import DropChunk
    m = DropChunk(noise_factor=0.5, **DC_KW)
    x = g["dc.x"]
    T = x.shape[1]
    lengths = (torch.from_numpy(g["dc.lens"]) * T).long()
    for s in SEEDS:
        torch.manual_seed(s)
        _, times, chunks, noise = m.draws(lengths)
        segs = m.segments(chunks, T)
        if segs is None:
            continue
        segs = segs.numpy()
        noff, flat = _noise_tables(segs, noise)
        ln = lengths.numpy().astype(np.int32)
        got, amp = run_drop(abi, dev, x, segs, flat, noff, ln, 0.5, f"seed {s}")
        kw = dict(noise=flat, noff=noff, lengths=ln, noise_factor=0.5)
        r64, r32 = R.drop_chunks(x, segs, **kw), R.drop_chunks(x, segs, dtype=np.float32, **kw)
        _close(got, r64, r32, f"seed {s} vs restatement")
        _close_fixture(got, g[f"dcn.{s}.out"], r64, r32, f"seed {s} vs fixture")
        _close(amp, R.amplitude(x, ln), R.amplitude(x, ln, np.float32), f"seed {s} amplitude")


# ------------------------------------------------------------------------- fused

def _fused_equals_sequence(abi, dev, x, table, taps, segs, what):
    fused = run_tdaug(abi, dev, x, table, taps, segs, what)
    seq = run_sequence(abi, dev, x, table, taps, segs)
    assert fused.shape == seq.shape
    assert np.array_equal(fused, seq), f"{what}: fused != 1 -> 2 -> 3 at {np.argwhere(fused != seq)[:8].tolist()}"
    return fused


def test_fused_recipe_seeds(abi, dev, g):
    """The recipe arguments on the fixture's batch: bit-identical to the
    sequence, and the fixture's output within the bound."""
    from speechbrain_amd.lobes.augment import TimeDomainSpecAugment
    m = TimeDomainSpecAugment(speeds=[95, 100, 105])
    x, lens = g["td.x"], torch.from_numpy(g["td.lens"])
    for s in SEEDS:
        torch.manual_seed(s)
        rs, T_out, taps, segs = m.draws(x.shape[1], lens)
        table = None if rs is None else (rs.first_indices.numpy().astype(np.int32), rs.weights.numpy(),
                                         rs.conv_stride, T_out)
        taps = None if taps is None else taps.numpy()
        segs = None if segs is None else segs.numpy()
        got = _fused_equals_sequence(abi, dev, x, table, taps, segs, f"seed {s}")
        r64, r32 = R.chain(x, table, taps, segs), R.chain(x, table, taps, segs, dtype=np.float32)
        _close(got, r64, r32, f"seed {s} vs restatement")
        _close_fixture(got, g[f"td.{s}.out"], r64, r32, f"seed {s} vs fixture")


@pytest.mark.parametrize("B", (1, 3))
def test_fused_tile_edges_and_chunk_positions(abi, dev, tile, B):
    """T_out around the tile; chunks at 0, across a tile boundary, across
    T_out and wholly past it."""
    m, first, w = _table(95)
    taps = _taps(3)
    for T_out in (tile - 1, tile, tile + 1, 2 * tile + 1):
        T, _ = _t_for(m, T_out)
        x = _wave((B, T), T_out)
        segs = np.zeros((B, 4, 2), np.int32)
        segs[0] = [[0, 30], [tile - 40, tile + 60], [T_out - 10, T_out + 40], [T_out + 5, T_out + 50]]
        if B > 1:
            segs[1, 2] = [T_out // 2, T_out // 2 + 100]
        table = (first, w, m.conv_stride, T_out)
        got = _fused_equals_sequence(abi, dev, x, table, taps, segs, f"T_out {T_out}")
        clipped = np.clip(segs, 0, T_out)
        _close(got, R.chain(x, table, taps, clipped), R.chain(x, table, taps, clipped, dtype=np.float32),
               f"T_out {T_out}")
        assert not got[0, :30].any() and not got[0, tile - 40:tile + 60].any() and not got[0, T_out - 10:].any()


def test_fused_span_past_the_lds_plan(abi, dev, tile):
    """The fused kernel on the unstaged path (16 kHz -> 4 kHz), with and
    without the filter."""
    m, first, w = _table(25)
    T, T_out = _t_for(m, 2 * tile + 1)
    x = _wave((2, T), 11)
    segs = np.array([[[0, 9], [tile - 5, tile + 5]], [[T_out - 3, T_out], [0, 0]]], np.int32)
    table = (first, w, m.conv_stride, T_out)
    for taps in (_taps(5), None):
        got = _fused_equals_sequence(abi, dev, x, table, taps, segs, f"filter {taps is not None}")
        _close(got, R.chain(x, table, taps, segs), R.chain(x, table, taps, segs, dtype=np.float32),
               f"filter {taps is not None}")


@pytest.mark.parametrize("speed", (105, 50))
def test_fused_each_stage_dropped(abi, dev, tile, speed):
    m, first, w = _table(speed)
    T, T_out = _t_for(m, tile + 37)
    x = _wave((2, T), 9)
    taps = _taps(4)
    for rs_on in (True, False):
        n = T_out if rs_on else T
        segs = np.array([[[5, 90], [n - 20, n]], [[0, 0], [tile - 3, tile + 3]]], np.int32)
        for taps_on in (True, False):
            for segs_on in (True, False):
                args = ((first, w, m.conv_stride, T_out) if rs_on else None, taps if taps_on else None,
                        segs if segs_on else None)
                what = f"resample {rs_on} filter {taps_on} chunks {segs_on}"
                got = _fused_equals_sequence(abi, dev, x, *args, what)
                ref = args[:2] + (np.clip(segs, 0, n) if segs_on else None,)
                _close(got, R.chain(x, *ref), R.chain(x, *ref, dtype=np.float32), what)
                if not (rs_on or taps_on or segs_on):
                    assert np.array_equal(got, x)  # the plain case is a clone


# ----------------------------------------------------------------------- modules

def test_modules_draws_and_outputs(dev, g):
    from speechbrain_amd.processing.speech_augmentation import DropChunk, DropFreq, Resample, SpeedPerturb
    x = torch.from_numpy(g["sp.x"]).to(dev)
    assert Resample(16000, 16000)(x) is x
    assert SpeedPerturb(16000, speeds=[100])(x) is x
    below = SpeedPerturb(16000, speeds=[90], perturb_prob=0.0)(x)
    assert below is not x and torch.equal(below, x)
    sp = SpeedPerturb(16000, speeds=[95, 100, 105])
    df = DropFreq(drop_count_low=0, drop_count_high=3)
    xf = torch.from_numpy(g["df.x"]).to(dev)
    for s in SEEDS:
        torch.manual_seed(s)
        y = sp(x)
        assert np.array_equal(R.flat_draws(sp), g[f"sp.{s}.draws"])
        assert y.dtype == torch.float32
        if sp.last_draws[1] is not None and sp.speeds[sp.last_draws[1]] != 100:
            rs = sp.resamplers[sp.last_draws[1]]
            args = (g["sp.x"], rs.first_indices.numpy(), rs.weights.numpy(), rs.conv_stride, y.shape[1])
            _close_fixture(y.cpu().numpy(), g[f"sp.{s}.out"], R.resample(*args), R.resample(*args, dtype=np.float32),
                           f"SpeedPerturb seed {s}")
        else:
            assert y is x
        torch.manual_seed(s)
        y = df(xf)
        assert np.array_equal(R.flat_draws(df), g[f"df.{s}.draws"])
        taps = df.last_draws[3].numpy()
        assert y is not xf
        _close_fixture(y.cpu().numpy(), g[f"df.{s}.out"], R.fir101(g["df.x"], taps),
                       R.fir101(g["df.x"], taps, np.float32), f"DropFreq seed {s}")
    # (B, T, 1) comes back as (B, T); more channels raise
    assert df(xf.unsqueeze(-1)).shape == xf.shape
    with pytest.raises(RuntimeError):
        df(torch.zeros(2, 300, 2, device=dev))
    with pytest.raises(TypeError):
        df(xf.double())
    with pytest.raises(TypeError):
        sp(torch.zeros(2, 300, 2, device=dev)[:, :, 0])
    # (B, T, C) through Resample and zero-fill DropChunk
    x2 = torch.from_numpy(g["rs.x.T257.C2"]).to(dev)
    rs = Resample(16000, 15200)
    y2 = rs(x2).cpu().numpy()
    args = (g["rs.x.T257.C2"], rs.first_indices.numpy(), rs.weights.numpy(), rs.conv_stride, y2.shape[1])
    _close_fixture(y2, g["rs.95.T257.C2"], R.resample(*args), R.resample(*args, dtype=np.float32), "Resample C 2")
    lens = torch.from_numpy(g["dc.lens"]).to(dev)
    xc = torch.from_numpy(g["dc.x"]).to(dev)
    dc, dcn = DropChunk(**DC_KW), DropChunk(noise_factor=0.5, **DC_KW)
    for s in SEEDS:
        torch.manual_seed(s)
        y = dc(xc, lens)
        assert np.array_equal(R.flat_draws(dc), g[f"dc.{s}.draws"])
        assert y is not xc and np.array_equal(y.cpu().numpy(), g[f"dc.{s}.out"])
        torch.manual_seed(s)
        y3 = dc(xc.unsqueeze(-1).repeat(1, 1, 2).contiguous(), lens)
        assert np.array_equal(y3[:, :, 1].cpu().numpy(), g[f"dc.{s}.out"])
        torch.manual_seed(s)
        y = dcn(xc, lens)
        assert np.array_equal(R.flat_draws(dcn), g[f"dcn.{s}.draws"])
        _, times, chunks, noise = dcn.last_draws
        segs = dcn.segments(chunks, 400)
        if segs is None:
            assert np.array_equal(y.cpu().numpy(), g[f"dcn.{s}.out"])
            continue
        noff, flat = _noise_tables(segs.numpy(), noise)
        kw = dict(noise=flat, noff=noff, lengths=np.array([400, 300, 200]), noise_factor=0.5)
        _close_fixture(y.cpu().numpy(), g[f"dcn.{s}.out"], R.drop_chunks(g["dc.x"], segs.numpy(), **kw),
                       R.drop_chunks(g["dc.x"], segs.numpy(), dtype=np.float32, **kw), f"DropChunk noise seed {s}")
    with pytest.raises(RuntimeError):
        dcn(torch.zeros(3, 400, 2, device=dev), lens)


def test_time_domain_spec_augment_module(dev, g):
    from speechbrain_amd.lobes.augment import TimeDomainSpecAugment
    m = TimeDomainSpecAugment(speeds=[95, 100, 105])
    x, lens = torch.from_numpy(g["td.x"]).to(dev), torch.from_numpy(g["td.lens"]).to(dev)
    host = TimeDomainSpecAugment(speeds=[95, 100, 105])
    for s in SEEDS:
        torch.manual_seed(s)
        rs, T_out, taps, segs = host.draws(4000, torch.from_numpy(g["td.lens"]))
        args = (g["td.x"], None if rs is None else (rs.first_indices.numpy(), rs.weights.numpy(), rs.conv_stride, T_out),
                None if taps is None else taps.numpy(), None if segs is None else segs.numpy())
        outs = []
        for fused in (True, False):
            m.fused = fused
            torch.manual_seed(s)
            outs.append(m(x, lens))
            assert np.array_equal(R.flat_draws(m), g[f"td.{s}.draws"]), f"seed {s} fused {fused}"
        assert outs[0] is not x and torch.equal(outs[0], outs[1]), f"seed {s}: fused != unfused"
        _close_fixture(outs[0].cpu().numpy(), g[f"td.{s}.out"], R.chain(*args), R.chain(*args, dtype=np.float32),
                       f"seed {s}")
    # the white-noise variant takes the three-kernel route
    n = TimeDomainSpecAugment(speeds=[95, 100, 105], drop_chunk_count_low=1, drop_chunk_length_low=100,
                              drop_chunk_length_high=200, drop_chunk_noise_factor=0.5)
    torch.manual_seed(0)
    y = n(x, lens)
    assert y.shape[0] == 3 and bool(torch.isfinite(y).all())
