"""Bit identity of the GEMM family between two builds of libsbk.so (GPU box,
not the product): what the exact integer probes of tests/gemm_ref.py cannot
see — the rounding order of Swish, GELU, GLU and the row LayerNorm — plus the
random inputs of tests/test_gpu_gemm256.py (bf16 and MXFP8, split-K tail
included).

    [SBK_PROBE_LIB=other/libsbk.so] python scripts/gemm_parity.py dump OUT.npz
    python scripts/gemm_parity.py compare A.npz B.npz

`dump` launches, in a fixed order and from fixed seeds, the scaled
(inexact-epilogue) cases of gemm_ref.gemm_cases for every tile id and both
operand dtypes, gemm_ln_cases, batched_cases, the nsplit == 1 cases of
tn_cases / tn_f32_cases (several splits add with atomics, whose order is not
stable), and the launches of test_gpu_gemm256.py; every output goes into one
.npz as raw integers.  `compare` prints one line per array and the totals."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speechbrain_amd._lib as _L  # noqa: E402
if os.environ.get("SBK_PROBE_LIB"):
    _L.LIB_PATH = os.path.abspath(os.environ["SBK_PROBE_LIB"])


def _raw(t):
    t = t.detach().contiguous().cpu()
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.view(iv).numpy()


def dump(path):
    import gemm_ref as R
    import test_gpu_gemm_tiles as T
    import test_gpu_gemm256 as G
    from speechbrain_amd import _enc, _w2v
    from speechbrain_amd._lib import lib, ptr, stream_of
    dev = torch.device("cuda")
    out = {}

    def put(key, t):
        assert key not in out, key
        out[key] = _raw(t)

    for bf16, tiles in ((True, R.TILES_BF16), (False, R.TILES_F32)):
        for tile in tiles:
            for i, case in enumerate(R.gemm_cases(bf16, tile)):
                if case.scaled and not case.expect_err:
                    rc, _, o = T.launch_gemm(case, dev)
                    assert rc == 0, str(case)
                    put(f"gemm/{i}/{case}", o)
    for inst in R.LN_INST:
        for i, case in enumerate(R.gemm_ln_cases(inst)):
            rc, _, o, _, u = T.launch_ln(case, dev)
            assert rc == 0, str(case)
            put(f"gemm_ln/{inst}/{i}/out/{case}", o)
            put(f"gemm_ln/{inst}/{i}/u/{case}", u)
    for bf16 in (True, False):
        tdt = torch.bfloat16 if bf16 else torch.float32
        for i, case in enumerate(R.batched_cases(bf16)):
            o = R.operands(case)
            Bt, M, N, K = case.batch, case.M, case.N, case.K
            A, W = o.A.to(dev, tdt).contiguous(), o.W.to(dev, tdt).contiguous()
            H = case.zdiv or 1
            c = torch.zeros(Bt // H, M, H, N, device=dev, dtype=torch.bfloat16 if case.out_bf16 else torch.float32)
            sC, sCo = (N, M * H * N) if case.zdiv else (M * N, 0)
            rc = lib().sbk_gemm_batched(int(bf16), ptr(A), K, M * K, ptr(W), K, N * K, M, N, K, Bt, ptr(c),
                                        H * N if case.zdiv else N, sC, case.zdiv, sCo, int(case.out_bf16), stream_of(c))
            assert rc == 0, str(case)
            put(f"batched/{i}/{case}", c)
    for name, cases in (("tn64", R.tn_cases(64)), ("tn128", R.tn_cases(128)), ("tn_f32", R.tn_f32_cases())):
        for i, case in enumerate(cases):
            if case.nsplit == 1:
                rc, _, c = T.launch_tn(case, dev)
                assert rc == 0, str(case)
                put(f"{name}/{i}/{case}", c)

    # tests/test_gpu_gemm256.py: test_gemm256_bf16_epilogues
    for (M, N, K) in ((256, 256, 64), (300, 512, 128), (1000, 768, 256), (777, 256, 1024)):
        torch.manual_seed(M)
        a, w = G._rnd(dev, M, K).to(torch.bfloat16), G._rnd(dev, N, K).to(torch.bfloat16)
        b, r = G._rnd(dev, N), G._rnd(dev, M, N)
        mask = (torch.rand(M, device=dev) < 0.1).to(torch.uint8)
        for act in (None, "swish", "gelu"):
            for odt in (torch.float32, torch.bfloat16):
                o = _enc.gemm(a, w, bias=b, act=act, res=r, alpha=0.5, rowmask=mask, out_dtype=odt, tile=30)
                put(f"gemm256/{M}x{N}x{K}/{act}/{odt}", o)
    # test_mx256_vs_dequantised_and_small_tile
    L = lib()
    for (M, N, K) in ((300, 256, 128), (1000, 512, 256), (2048, 768, 1024)):
        torch.manual_seed(K)
        a, w = _w2v.mx_quant(G._rnd(dev, M, K)), _w2v.mx_quant(G._rnd(dev, N, K))
        bias, res = G._rnd(dev, N), G._rnd(dev, M, N)
        o, _ = G._mx_call(L.sbk_mx_gemm256, a, w, M, N, K, 0, bias, 0, res)
        put(f"mx256/{M}x{N}x{K}/res", o)
        for mode, act in ((0, 4), (1, 4), (2, 4), (2, 0)):
            for fn in ("sbk_mx_gemm", "sbk_mx_gemm256"):
                o, s = G._mx_call(getattr(L, fn), a, w, M, N, K, mode, bias, act)
                put(f"{fn}/{M}x{N}x{K}/mode{mode}/act{act}", o)
                if mode == 2:
                    put(f"{fn}/{M}x{N}x{K}/mode{mode}/act{act}/scales", s)
    # test_mx256_split_k_tail (the workspace entry; the tail's partial sums are one add each, so order-stable)
    M, N = 17820, 1024
    for act, with_res, K in ((0, True, 2048), (4, False, 2048), (3, True, 2176)):
        nws = int(L.sbk_mx_gemm_ws_floats(M, N, K, 0))
        torch.manual_seed(act + 7)
        a, w = _w2v.mx_quant(G._rnd(dev, M, K)), _w2v.mx_quant(G._rnd(dev, N, K))
        bias = G._rnd(dev, N)
        res = G._rnd(dev, M, N) if with_res else None
        ws = torch.full((max(nws, 1),), float("nan"), device=dev)
        o1 = torch.full((M, N), float("nan"), device=dev)
        rc = L.sbk_mx_gemm_ws(ptr(a.q), ptr(a.s), a.q.stride(0), a.s.stride(0), M, 0, 0, ptr(w.q), ptr(w.s),
                              w.q.stride(0), w.s.stride(0), M, N, K, ptr(bias), act, 1.0, ptr(res),
                              res.stride(0) if res is not None else 0, ptr(o1), o1.stride(0), 0, None, 0, ptr(ws), nws,
                              stream_of(a.q))
        assert rc == 0, rc
        put(f"mx_split_tail/K{K}/act{act}/ws{nws}", o1)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} arrays from {_L.LIB_PATH} -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    bad = 0
    for k in a.files:
        x, y = a[k], b[k]
        n = int((x != y).sum()) if x.shape == y.shape and x.dtype == y.dtype else x.size
        bad += n > 0
        if n:
            print(f"DIFFERS {k}: {n} of {x.size} elements")
    groups = {}
    for k in a.files:
        g = k.split("/")[0]
        groups[g] = groups.get(g, 0) + 1
    print("arrays per group: " + ", ".join(f"{g} {n}" for g, n in sorted(groups.items())))
    print(f"{len(a.files)} arrays, {len(a.files) - bad} bit-identical, {bad} differ")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
