"""Host-side checks of the fused encoder ends (no GPU): sbk_conv_ffn_tail and
sbk_src_ffn_proj refuse bad arguments with the argument error code before any
launch, the image sizes they check agree with the Python-side sizes, and the row-slice
arithmetic of the kept linear_pos table holds on the host."""
import ctypes
import os

import pytest
import torch

ERR_ARG = 1001


@pytest.fixture(scope="module")
def lib():
    from speechbrain_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from speechbrain_amd import _build
        _build.build()
    return _lib.lib()


def _tail_args(lib, p, H=1024):
    """A call that passes every check (never made: it would launch)."""
    return dict(x=p, o=p, wo=p, bo=p, B=2, T=50, D=256, d_eff=256, cln0_w=p, cln0_b=p, ceps0=1e-5, cimg=p,
                cimg_elems=lib.sbk_conv_image_elems(256), cb1p=p, wc=p, bc=p, K=31, causal=0, cln1_w=p, cln1_b=p,
                ceps1=1e-5, cb2=p, kpm=None, H=H, act=1, slope=0.0, g0=p, b0=p, eps0=1e-5, b1=p, b2=p, alpha=0.5,
                gp=p, bp=p, epsp=1e-5, gn=p, bn=p, epsn=1e-6, u=None, img=p,
                img_elems=lib.sbk_ffn_image_elems(256, H, 0, 0), stream=None)


def test_tail_refuses_bad_arguments(lib):
    buf = (ctypes.c_double * 16)()          # non-null, 16-byte aligned below; never dereferenced
    base = ctypes.addressof(buf)
    base += -base % 16
    p, p2, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 32), ctypes.c_void_p(base + 8)

    def call(**kw):
        a = _tail_args(lib, p)
        a["u"] = p2
        a.update(kw)
        return lib.sbk_conv_ffn_tail(*a.values())

    assert call(x=None) == ERR_ARG and call(u=None) == ERR_ARG and call(o=None) == ERR_ARG
    assert call(wo=None) == ERR_ARG and call(cimg=None) == ERR_ARG and call(img=None) == ERR_ARG
    assert call(gn=None) == ERR_ARG and call(bn=None) == ERR_ARG and call(b1=None) == ERR_ARG
    assert call(u=p) == ERR_ARG                      # u aliases x (neighbouring tiles read x for the halo)
    assert call(x=odd) == ERR_ARG and call(u=odd) == ERR_ARG and call(gn=odd) == ERR_ARG and call(o=odd) == ERR_ARG
    assert call(B=0) == ERR_ARG and call(T=0) == ERR_ARG and call(D=144) == ERR_ARG
    assert call(d_eff=0) == ERR_ARG and call(d_eff=257) == ERR_ARG
    assert call(K=0) == ERR_ARG and call(K=32) == ERR_ARG
    assert call(H=1000) == ERR_ARG and call(act=2) == ERR_ARG
    # an image built for another shape, for a chain or with a projection is refused
    assert call(img_elems=lib.sbk_ffn_image_elems(256, 512, 0, 0)) == ERR_ARG
    assert call(img_elems=lib.sbk_ffn_image_elems(256, 1024, 0, 1)) == ERR_ARG
    assert call(img_elems=lib.sbk_ffn_image_elems(256, 1024, 768, 0)) == ERR_ARG
    assert call(cimg_elems=lib.sbk_conv_image_elems(256) - 1) == ERR_ARG


def _head_args(lib, p, Kin=640, H=1024, NP=768):
    return dict(a=p, Kin=Kin, simg=p, simg_elems=lib.sbk_src_image_elems(Kin), sbias=p, rel_len=None, T=50,
                kpm_out=None, M=100, D=256, d_eff=256, H=H, g0=p, b0=p, eps0=1e-5, img=p,
                img_elems=lib.sbk_ffn_image_elems(256, H, NP, 0), b1=p, act=1, slope=0.0, b2=p, alpha=0.5, gp=None,
                bp=None, epsp=0.0, out=None, gn=p, bn=p, epsn=1e-5, np=NP, yp=p, stream=None)


def test_head_refuses_bad_arguments(lib):
    buf = (ctypes.c_double * 16)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, p2, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 32), ctypes.c_void_p(base + 8)

    def call(**kw):
        a = _head_args(lib, p)
        a["out"] = p2
        a.update(kw)
        return lib.sbk_src_ffn_proj(*a.values())

    assert call(a=None) == ERR_ARG and call(simg=None) == ERR_ARG and call(out=None) == ERR_ARG
    assert call(img=None) == ERR_ARG and call(yp=None) == ERR_ARG and call(gn=None) == ERR_ARG
    assert call(a=odd) == ERR_ARG and call(sbias=odd) == ERR_ARG and call(out=odd) == ERR_ARG and call(yp=odd) == ERR_ARG
    assert call(out=p) == ERR_ARG                       # out aliases a
    assert call(np=0) == ERR_ARG and call(np=-256) == ERR_ARG and call(np=100) == ERR_ARG
    for kin in (0, 96, 832):                            # no whole K-steps / the A rows do not fit in LDS
        assert lib.sbk_src_image_elems(kin) == -1
        assert call(Kin=kin) == ERR_ARG and call(Kin=kin, simg_elems=(max(kin, 64) // 64) * 256 * 64) == ERR_ARG
        assert lib.sbk_src_image(p, kin, p2, None) == ERR_ARG
    assert call(simg_elems=lib.sbk_src_image_elems(64)) == ERR_ARG
    assert call(img_elems=lib.sbk_ffn_image_elems(256, 1024, 0, 0)) == ERR_ARG
    # a mask needs its buffer and M = B * T
    assert call(rel_len=p) == ERR_ARG and call(rel_len=p, kpm_out=p2, T=0) == ERR_ARG
    assert call(rel_len=p, kpm_out=p2, T=33) == ERR_ARG
    assert call(M=0) == ERR_ARG and call(D=144) == ERR_ARG and call(d_eff=0) == ERR_ARG and call(H=1000) == ERR_ARG
    assert lib.sbk_src_image(None, 640, p, None) == ERR_ARG and lib.sbk_src_image(p, 640, odd, None) == ERR_ARG


def test_image_sizes_agree_with_the_python_side(lib):
    for kin in (64, 640, 768):
        assert lib.sbk_src_image_elems(kin) == (kin // 64) * 256 * 64
    from speechbrain_amd import _lib as L
    assert len(L.SIGNATURES["sbk_src_ffn_proj"]) == len(_head_args(lib, None))
    tile = 256 * 64
    for H in (512, 1024):
        assert lib.sbk_ffn_image_elems(256, H, 0, 0) == (H // 256) * (256 // 64 + 4) * tile
    assert lib.sbk_conv_image_elems(256) == 12 * tile
    from speechbrain_amd import _lib
    assert len(_lib.SIGNATURES["sbk_conv_ffn_tail"]) == len(_tail_args(lib, None))


@pytest.mark.parametrize("T,Tc", [(1, 1), (5, 128), (50, 128), (97, 128), (128, 128), (7, 8)])
def test_table_slice_arithmetic(T, Tc):
    """Row r of table(T) is row r + (Tc - T) of table(Tc): the rows
    [Tc - T, Tc + T - 1) of the longer table, in fp32 and after the bf16 cast."""
    from speechbrain_amd.nnet.attention import RelPosEncXL
    enc = RelPosEncXL(256)
    for dtype in (torch.float32, torch.bfloat16):
        small = enc.table(T, "cpu", dtype)[0]
        big = enc.table(Tc, "cpu", dtype)[0]
        assert small.shape[0] == 2 * T - 1
        assert torch.equal(small, big[Tc - T:Tc + T - 1])
