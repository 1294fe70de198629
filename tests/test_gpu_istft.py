"""ISTFT (sbk_istft), its gradient (sbk_istft_bwd) and the waveform gradient
of STFT (sbk_istft in its adjoint role) against torch.istft / torch.stft on
the CPU in float64, forward and through float64 autograd.

Bound, per tensor: max |err| / max(1, |ref|_inf) <= max(1e-5, 8 * E32), E32
the same figure for the same CPU reference run in float32.  Every spectrum
operand is a view at an odd element offset inside a NaN-filled buffer (guard
bands), and the bins above n_fft/2 of a two-sided spectrum are NaN: they must
not be read.  The float64 reference passes `normalized` to torch.istft (the
inverse of STFT(normalized_stft=True)); the reference module accepts the flag
and drops it.  T is placed at the tile edges from sbk_istft_hops (HB hops per
workgroup, R = ceil(n_fft / hop) frames over a sample).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SETTINGS = {  # name: ISTFT arguments (ms at 16 kHz), n_fft, hop in samples
    "win400_infer": (dict(win_length=25, hop_length=10), 400, 160),  # the defaults: n_fft from 201 bins
    "fft512_hop128": (dict(n_fft=512, win_length=32, hop_length=8), 512, 128),
    "win400_in_fft512": (dict(n_fft=512, win_length=25, hop_length=10), 512, 160),  # padded window
    "fft480_radix3": (dict(n_fft=480, win_length=30, hop_length=10), 480, 160),  # runtime plan, radix 3
}
FRAMES = ["1", "R-1", "R", "HB-1", "HB", "HB+1", "2HB+1"]
LENGTHS = [None, "short", "natural", "long"]  # natural - 37, natural, natural + n_fft + 5 (zero tail)
FLAGS = {"center_false": dict(center=False), "twosided": dict(onesided=False),
         "normalized": dict(normalized_stft=True), "channels": dict()}


def err(a, ref):
    return float((a.detach().double().cpu() - ref).abs().max() / max(1.0, float(ref.abs().max())))


def guarded(x, dev):
    buf = torch.full((x.numel() + 8,), float("nan"), device=dev)
    v = buf[3:3 + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def n_frames(name, n_fft, hop):
    from speechbrain_amd import _lib
    hb, r = _lib.lib().sbk_istft_hops(n_fft, hop), -(-n_fft // hop)
    assert hb >= 1
    return {"1": 1, "R-1": r - 1, "R": r, "HB-1": hb - 1, "HB": hb, "HB+1": hb + 1, "2HB+1": 2 * hb + 1}[name]


def reference_istft(x, window, n_fft, hop, center, onesided, normalized, length):
    """ISTFT.forward of the reference module, at x's dtype on the CPU."""
    shape = x.shape
    x = x.permute(0, 4, 2, 1, 3).reshape(-1, shape[2], shape[1], 2) if x.dim() == 5 else x.permute(0, 2, 1, 3)
    y = torch.istft(torch.complex(x[..., 0], x[..., 1]), n_fft=n_fft, hop_length=hop, win_length=window.numel(),
                    window=window.to(x.dtype), center=center, onesided=onesided, normalized=normalized,
                    length=length)
    return y.reshape(shape[0], shape[4], -1).transpose(1, 2) if len(shape) == 5 else y


def run_istft(dev, setting, frames, length, C=0, **flags):
    from speechbrain_amd.processing.features import ISTFT
    kw, n_fft, hop = SETTINGS[setting]
    mod = ISTFT(16000, **kw, **flags)
    center, onesided = flags.get("center", True), flags.get("onesided", True)
    T = n_frames(frames, n_fft, hop)
    g = torch.Generator().manual_seed(T)
    x = torch.randn((2, T, n_fft // 2 + 1 if onesided else n_fft, 2) + ((C,) if C else ()), generator=g,
                    dtype=torch.float64)
    x[:, :, n_fft // 2 + 1:] = float("nan")
    full, start = (T - 1) * hop + n_fft, n_fft // 2 if center else 0
    natural = full - 2 * start
    length = {None: None, "short": natural - 37, "natural": natural, "long": natural + n_fft + 5}[length]
    dy = torch.randn((2, natural if length is None else length) + ((C,) if C else ()), generator=g,
                     dtype=torch.float64)

    def ref(dt):
        xr = x.detach().to(dt).clone().requires_grad_()
        y = reference_istft(xr, mod.window, n_fft, hop, center, onesided, flags.get("normalized_stft", False), length)
        y.backward(dy.to(dt))
        return y.detach().double(), xr.grad.double()

    try:
        (y64, g64), (y32, g32) = ref(torch.float64), ref(torch.float32)
    except RuntimeError as e:  # a zero envelope inside the range (the padded window's zeros at an end): same refusal
        assert "window overlap add min" in str(e)
        with pytest.raises(RuntimeError, match="window overlap add min"):
            mod(x.float().to(dev), length)
        return
    xd = guarded(x.float(), dev).requires_grad_()
    y = mod(xd, length)
    assert torch.equal(y, mod(xd, length))  # no atomics: bit-identical
    y.backward(dy.float().to(dev))
    e, e32, eg, eg32 = err(y, y64), err(y32, y64), err(xd.grad, g64), err(g32, g64)
    print(f"T {T} y err {e:.3e} E32 {e32:.3e}  dspec err {eg:.3e} E32 {eg32:.3e}")
    assert y.shape == y64.shape and e <= max(1e-5, 8 * e32)
    assert (y[:, full - start:] == 0).all()  # past the overlap-added signal: exact zeros
    assert eg <= max(1e-5, 8 * eg32)
    assert (xd.grad[:, :, [0, n_fft // 2], 1] == 0).all() and (xd.grad[:, :, n_fft // 2 + 1:] == 0).all()


# T = 1 centred has an empty natural range: only an explicit longer sig_length returns samples
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_istft_tile_edges(dev, setting, frames, length):
    run_istft(dev, setting, frames, "long" if frames == "1" else length)


@pytest.mark.parametrize("length", ["short", "long"])
@pytest.mark.parametrize("frames", ["1", "HB+1"])
@pytest.mark.parametrize("flag", list(FLAGS))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_istft_flags(dev, setting, flag, frames, length):
    if frames == "1" and flag != "center_false":
        length = "long"
    run_istft(dev, setting, frames, length, C=2 if flag == "channels" else 0, **FLAGS[flag])


def test_istft_round_trip_and_errors(dev):
    from speechbrain_amd.processing.features import ISTFT, STFT
    x = torch.randn(10, 16000, generator=torch.Generator().manual_seed(0))
    y = ISTFT(sample_rate=16000, win_length=25, hop_length=10)(STFT(sample_rate=16000)(x.to(dev)))
    assert y.shape == (10, 16000)
    assert err(y, x.double()) <= 1e-4  # two transforms at the 1e-5 floor each, envelope >= 1 inside the trim
    spec = torch.randn(2, 9, 201, 2)
    hann = ISTFT(16000, center=False, window_fn=torch.hann_window)
    with pytest.raises(RuntimeError):  # w[0] = 0: zero envelope at the first sample
        reference_istft(spec, hann.window, 400, 160, False, True, False, None)
    with pytest.raises(RuntimeError):
        hann(spec.to(dev))
    with pytest.raises((RuntimeError, ValueError)):  # 201 = 3 * 67: no FFT plan
        ISTFT(16000, n_fft=402)(torch.randn(2, 9, 202, 2, device=dev))
    with pytest.raises(RuntimeError):  # no CPU fallback
        ISTFT(16000)(spec)


STFT_SHAPES = {"mono_400": (dict(n_fft=400, win_length=25, hop_length=10), 400, 160, 0),
               "stereo_win400_in_512": (dict(n_fft=512, win_length=25, hop_length=8), 512, 128, 2)}


@pytest.mark.parametrize("onesided,normalized", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("frames", ["1", "HB+1"])
@pytest.mark.parametrize("pad", ["constant", "reflect", "replicate", "circular", "no_center"])
@pytest.mark.parametrize("shape", list(STFT_SHAPES))
def test_stft_backward(dev, shape, pad, frames, onesided, normalized):
    from speechbrain_amd.processing.features import STFT
    if frames == "1" and pad in ("reflect", "circular"):
        frames = "R"  # torch.stft refuses to wrap a signal shorter than n_fft/2: the fewest frames past that
    kw, n_fft, hop, C = STFT_SHAPES[shape]
    center, mode = pad != "no_center", "constant" if pad == "no_center" else pad
    mod = STFT(16000, **kw, center=center, pad_mode=mode, onesided=onesided, normalized_stft=normalized)
    T = n_frames(frames, n_fft, hop)
    S = (T - 1) * hop + 57 + (0 if center else n_fft)  # 57 samples past the last frame when T > 1
    g = torch.Generator().manual_seed(T)
    x = torch.randn((2, S) + ((C,) if C else ()), generator=g, dtype=torch.float64)
    Y = torch.randn((2, T, n_fft // 2 + 1 if onesided else n_fft, 2) + ((C,) if C else ()), generator=g,
                    dtype=torch.float64)

    def ref(dt):
        xr = x.detach().to(dt).clone().requires_grad_()
        rows = xr.transpose(1, 2).reshape(-1, S) if C else xr
        s = torch.view_as_real(torch.stft(rows, n_fft, hop, mod.win_length, mod.window.to(dt), center, mode,
                                          normalized, onesided, return_complex=True)).transpose(1, 2)
        s = s.reshape(2, C, T, -1, 2).permute(0, 2, 3, 4, 1) if C else s
        (s * Y.to(dt)).sum().backward()
        return xr.grad.double()

    g64, g32 = ref(torch.float64), ref(torch.float32)
    xd = x.float().to(dev).requires_grad_()
    out = mod(xd)
    (out * guarded(Y.float(), dev)).sum().backward()
    e, e32 = err(xd.grad, g64), err(g32, g64)
    print(f"T {T} S {S} dx err {e:.3e} E32 {e32:.3e}")
    assert e <= max(1e-5, 8 * e32)
    # adjointness <STFT x, Y> = <x, grad> in float64 on the host; each side carries the 1e-5 bound above
    lhs, rhs = (out.detach().double().cpu() * Y).sum(), (x.float().double() * xd.grad.double().cpu()).sum()
    tol = 1e-5 * (float(out.detach().abs().max()) * float(Y.abs().sum()) + float(xd.grad.abs().max()) * float(x.abs().sum()))
    assert abs(float(lhs - rhs)) <= tol
