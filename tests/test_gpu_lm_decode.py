"""The TransformerLM drop-in and key/value-cached LM fusion on the GPU
(lobes/models/transformer/TransformerLM.py, csrc/kvdec.hip's masked decode
step, csrc/lmfuse.hip, S2STransformerBeamSearch.USE_LM_KV_CACHE).

  * sbk_kv_decode_self_attn_masked against a float64 restatement written here
    with torch on the CPU, at test_gpu_kv_decode.py's bound for the unmasked
    kernel (conftest.assert_close: |a − b| <= 1e-4·max(1, |b|)); bit-equal to
    the unmasked op under an all-zero mask; NaN, and only there, where every
    key of a row is masked;
  * sbk_log_softmax_fuse against float64, |a − b| <= 1e-5·max(1, |b|);
  * TransformerLM.forward and two gradients against tests/golden/lm.npz (the
    reference on the CPU), decode_step against forward of the whole prefix,
    both at assert_close's bound;
  * every search case of lm.npz with the flag off and on: the fixture's
    hypotheses exactly, scores and log_probs at assert_close's bound.
Every comparison prints the largest deviation it saw."""
import json
import math

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_gpu_kv_decode import _dev, _self_case
from test_gpu_s2s_search import _check

pytestmark = pytest.mark.gpu

ACT = {"GELU": torch.nn.GELU, "ReLU": torch.nn.ReLU}
PE = "positional_encoding.pe"


# --------------------------------------------------------------------------
# masked decode-step self-attention
# --------------------------------------------------------------------------
def _keymask(kind, N, L, cap, seed):
    """(cap, N) uint8, indexed like the caches: [position][the row that wrote it]."""
    km = torch.zeros(cap, N, dtype=torch.uint8)
    if kind == "own":            # the new token of rows 0, 2, 4 is the padding index
        km[L - 1, 0::2] = 1
    elif kind == "chunk1":       # the whole second 64-position chunk
        km[64:128] = 1
    elif kind == "chunk0":       # the whole first chunk: nothing unmasked until position 64
        km[0:64] = 1
    elif kind == "random":       # about 30 % of the positions; position 0 is kept
        km[:L] = (torch.rand(L, N, generator=torch.Generator().manual_seed(seed)) < 0.3).to(torch.uint8)
        km[0] = 0
    else:
        assert kind == "none"
    return km


def _masked_ref(qkv, kc, vc, anc, km, H, L):
    """float64: row n attends kc / vc[j][a] with a = clamp(anc[n][j]) for j < L−1 and its own new k / v at
    L−1; key j is masked by km[j][a] (a = n at L−1).  A row with every key masked is NaN (softmax of −inf)."""
    N, E3 = qkv.shape
    E = E3 // 3
    dh = E // H
    q, k_new, v_new = (t.double() for t in qkv.split(E, dim=1))
    a = anc[:, :L].long().clamp(0, N - 1)
    a[:, L - 1] = torch.arange(N)
    pos = torch.arange(L)
    keys = kc.double()[pos[None, :], a]                         # (N, L, E)
    vals = vc.double()[pos[None, :], a]
    keys[:, L - 1] = k_new
    vals[:, L - 1] = v_new
    masked = km[pos[None, :], a].bool()                          # (N, L)
    s = q.view(N, H, 1, dh) @ keys.view(N, L, H, dh).permute(0, 2, 3, 1) / math.sqrt(dh)       # (N, H, 1, L)
    s = s.masked_fill(masked[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    p0 = torch.nan_to_num(p, nan=0.0)
    out = (p0 @ vals.view(N, L, H, dh).transpose(1, 2)).reshape(N, E)
    out[masked.all(dim=1)] = float("nan")
    return out


def _run_masked(dev, qkv, kc, vc, anc, km, H, L):
    from speechbrain_amd._kvdec import kv_decode_self_attn_masked
    E = qkv.shape[1] // 3
    kc_d, vc_d = kc.to(dev), vc.to(dev)
    out = kv_decode_self_attn_masked(qkv.to(dev), kc_d, vc_d, anc.to(dev), km.to(dev), H, L)
    torch.cuda.current_stream().synchronize()
    for name, cache, new, before in (("kc", kc_d, qkv[:, E:2 * E], kc), ("vc", vc_d, qkv[:, 2 * E:], vc)):
        got = cache.cpu()
        assert torch.equal(got[L - 1], new), f"{name}: slot L-1 is not the step's row bit for bit"
        keep = torch.ones(before.shape[0], dtype=torch.bool)
        keep[L - 1] = False
        assert torch.equal(got[keep], before[keep]), f"{name}: a slot other than L-1 changed"
    return out.cpu()


def _close_with_nan(out, ref, name):
    """The same NaN pattern, and assert_close where the reference is finite."""
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out), nan), f"{name}: NaN at other places than the all-masked rows"
    fin = ~nan
    if bool(fin.any()):
        _dev(name, out[fin], ref[fin])
        assert_close(out[fin], ref[fin].float(), name=name)


MASK_CASES = [(kind, L) for L in (1, 2, 64, 65, 130) for kind in ("none", "own", "random")]
MASK_CASES += [("chunk1", 130), ("chunk0", 130), ("chunk0", 65)]


@pytest.mark.parametrize("kind,L", MASK_CASES)
@pytest.mark.parametrize("dh", [4, 64, 68, 128])
def test_masked_self_attn_kernel(dev, dh, kind, L):
    N, H = 6, 2
    qkv, kc, vc, anc = _self_case(N, H, dh, L, seed=1000 * dh + L)
    km = _keymask(kind, N, L, kc.shape[0], seed=7 * dh + L)
    out = _run_masked(dev, qkv, kc, vc, anc, km, H, L)
    ref = _masked_ref(qkv, kc, vc, anc, km, H, L)
    if not (kind == "own" and L == 1):
        assert not bool(torch.isnan(ref).any())       # position 0 / the other chunks are unmasked
    _close_with_nan(out, ref, f"masked self dh={dh} L={L} mask={kind}")


@pytest.mark.parametrize("dh,L", [(4, 1), (64, 64), (68, 65), (128, 130)])
def test_all_zero_mask_is_bit_equal_to_the_unmasked_op(dev, dh, L):
    from speechbrain_amd._kvdec import kv_decode_self_attn
    N, H = 6, 2
    qkv, kc, vc, anc = _self_case(N, H, dh, L, seed=31 * dh + L)
    km = torch.zeros(kc.shape[0], N, dtype=torch.uint8)
    masked = _run_masked(dev, qkv, kc, vc, anc, km, H, L)
    plain = kv_decode_self_attn(qkv.to(dev), kc.to(dev), vc.to(dev), anc.to(dev), H, L).cpu()
    assert torch.equal(masked, plain)


def test_a_row_with_every_key_masked_is_nan_and_only_that_row(dev):
    N, H, dh, L = 6, 2, 64, 1
    qkv, kc, vc, anc = _self_case(N, H, dh, L, seed=77)
    km = torch.zeros(kc.shape[0], N, dtype=torch.uint8)
    km[0, 3] = 1
    out = _run_masked(dev, qkv, kc, vc, anc, km, H, L)
    assert bool(torch.isnan(out[3]).all())
    rest = torch.tensor([0, 1, 2, 4, 5])
    assert bool(torch.isfinite(out[rest]).all())
    ref = _masked_ref(qkv, kc, vc, anc, km, H, L)
    assert_close(out[rest], ref[rest].float(), name="rows beside the all-masked one")


def test_masked_op_refuses_a_short_mask(dev):
    from speechbrain_amd._kvdec import kv_decode_self_attn_masked
    N, H, dh, L = 6, 2, 16, 9
    qkv, kc, vc, anc = (t.to(dev) for t in _self_case(N, H, dh, L, seed=5))
    with pytest.raises(ValueError, match="keymask"):
        kv_decode_self_attn_masked(qkv, kc, vc, anc, torch.zeros(L - 1, N, dtype=torch.uint8, device=dev), H, L)
    with pytest.raises(ValueError, match="keymask"):
        kv_decode_self_attn_masked(qkv, kc, vc, anc, torch.zeros(L, N, dtype=torch.bool, device=dev), H, L)


# --------------------------------------------------------------------------
# the LM-fusion tail
# --------------------------------------------------------------------------
def _fuse_close(out, ref, name):
    """|a − b| <= 1e-5·max(1, |b|); −inf where, and only where, the reference has it."""
    out = out.double().cpu().numpy()
    ref = ref.numpy()
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(out), inf), f"{name}: -inf at other places"
    assert np.isfinite(out[~inf]).all(), name
    err = np.abs(out[~inf] - ref[~inf]) / np.maximum(1.0, np.abs(ref[~inf]))
    worst = float(err.max()) if err.size else 0.0
    print(f"{name}: max deviation {worst:.3e}")
    assert worst <= 1e-5, f"{name}: max deviation {worst:.3e} > 1e-5"


def _strided(t, dev):
    """t (N, V) on the device as the first V columns of an (N, V + 3) tensor."""
    wide = torch.zeros(t.shape[0], t.shape[1] + 3, device=dev)
    wide[:, :t.shape[1]] = t.to(dev)
    return wide[:, :t.shape[1]]


def _fuse_case(dev, N, V):
    from speechbrain_amd._kvdec import log_softmax_fuse
    g = torch.Generator().manual_seed(100 * V + N)
    w = 0.6
    # row stride V + 3 on both operands; logits of magnitude ~80
    x = ((torch.rand(N, V + 3, generator=g) * 2 - 1) * 80)[:, :V]
    finite = (5 * torch.randn(N, V + 3, generator=g))[:, :V]
    sent = finite.clone()
    sent[:, 0] = float("-inf")
    sent[:, V // 2] = -1e20
    sent[N - 1, V - 1] = -1e20
    x_d = _strided(x, dev)
    assert x_d.stride(0) == V + 3 and torch.equal(x_d.cpu(), x)
    for inv_t in (1.0, float(np.float32(1 / 1.15))):
        lp = torch.log_softmax(x.double() * inv_t, dim=-1)
        for tag, base in (("null", None), ("finite", finite), ("sentinels", sent)):
            out = log_softmax_fuse(x_d, None if base is None else _strided(base, dev), inv_t, w)
            assert out.shape == (N, V) and out.is_contiguous()
            ref = w * lp if base is None else base.double() + w * lp
            _fuse_close(out, ref, f"fuse N={N} V={V} invT={inv_t:.4f} base={tag}")
            if tag == "sentinels":      # −1e20 + anything of this size is −1e20 in fp32
                assert bool((out[:, V // 2].cpu() == torch.tensor(-1e20)).all())


@pytest.mark.parametrize("N", [1, 7])
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 300, 5000, 5003])
def test_log_softmax_fuse(dev, V, N):
    _fuse_case(dev, N, V)


@pytest.mark.parametrize("V", [8192, 8193])
def test_log_softmax_fuse_at_the_on_chip_limit(dev, V):
    """8192 floats is the widest row kept on chip; 8193 takes the two-pass kernel."""
    _fuse_case(dev, 2, V)


def test_log_softmax_fuse_two_pass_with_minus_inf_logits(dev):
    """−inf logits in the two-pass kernel's online (maximum, sum) pair, also as a thread's first elements."""
    from speechbrain_amd._kvdec import log_softmax_fuse
    V = 8200
    x = torch.randn(2, V, generator=torch.Generator().manual_seed(3)) * 10
    x[0, :600] = float("-inf")
    x[1, 5::7] = float("-inf")
    out = log_softmax_fuse(x.to(dev), None, 1.0, 1.0)
    _fuse_close(out, torch.log_softmax(x.double(), dim=-1), "fuse two-pass -inf logits")


# --------------------------------------------------------------------------
# the LM against the fixtures; decode_step against forward
# --------------------------------------------------------------------------
def _sub(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


def _load_lm(g, kw, prefix, dev):
    from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM
    lm = TransformerLM(**{**kw, "activation": ACT[kw["activation"]]})
    sd = _sub(g, prefix)
    sd[PE] = lm.state_dict()[PE]
    lm.load_state_dict(sd, strict=True)
    return lm.to(dev).eval()


@pytest.fixture(scope="module")
def lms(golden, dev):
    g = golden("lm")
    return g, {name: _load_lm(g, json.loads(str(g[f"lm.{name}.kw"])), f"lm.{name}.sd.", dev) for name in ("A", "B")}


@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_and_gradients_match_reference(lms, dev, name):
    g, models = lms
    lm = models[name]
    tokens = torch.from_numpy(g["lm.tokens"]).to(dev)
    proj = torch.from_numpy(g["lm.proj"]).to(dev)
    lm.zero_grad()
    logits = lm(tokens)
    _dev(f"lm.{name}.logits", logits, g[f"lm.{name}.logits"])
    assert_close(logits, g[f"lm.{name}.logits"], name=f"lm.{name}.logits")
    (logits * proj).sum().backward()
    params = dict(lm.named_parameters())
    for gname in g["lm.grad_names"].tolist():
        _dev(f"lm.{name}.grad.{gname}", params[gname].grad, g[f"lm.{name}.grad.{gname}"])
        assert_close(params[gname].grad, g[f"lm.{name}.grad.{gname}"], name=f"lm.{name}.grad.{gname}")
    lm.zero_grad()
    with torch.no_grad():               # the inference call gives the same logits
        assert_close(lm(tokens), g[f"lm.{name}.logits"], name=f"lm.{name}.logits (no_grad)")


def _steps_match_forward(lm, tokens, permute_after=(), tag=""):
    """decode_step at every t against forward(prefixes)[:, -1]; after the
    steps in permute_after the rows are permuted (state.permute), and so are
    the prefixes forward sees."""
    N, T = tokens.shape
    state = lm.init_decode_state(N)
    prefixes = tokens[:, :0]
    gen = torch.Generator().manual_seed(3)
    worst = 0.0
    with torch.no_grad():
        for t in range(T):
            prefixes = torch.cat([prefixes, tokens[:, t:t + 1]], dim=1)
            got = lm.decode_step(tokens[:, t], state)
            want = lm(prefixes)[:, -1]
            assert got.shape == want.shape and bool(torch.isfinite(want).all())
            worst = max(worst, float(((got - want).abs() / want.abs().clamp(min=1)).max()))
            assert_close(got, want, name=f"{tag} logits at t={t}")
            if t in permute_after:
                index = torch.randint(0, N, (N,), generator=gen).to(tokens.device)
                assert state.permute(index) is state
                prefixes = prefixes.index_select(0, index)
    print(f"{tag}: max deviation {worst:.3e} over {T} steps")
    return state


@pytest.mark.parametrize("name", ["A", "B"])
def test_decode_step_matches_forward_on_the_fixture_prefixes(lms, dev, name):
    """The rows with padding tokens included: zeros in the middle of a prefix and at its end."""
    g, models = lms
    tokens = torch.from_numpy(g["lm.tokens"]).to(dev).repeat(2, 1)
    assert bool((tokens == 0).any()) and bool((tokens[:, 0] != 0).all())
    state = _steps_match_forward(models[name], tokens, permute_after=(4,), tag=f"lm.{name} fixture prefixes")
    assert state.steps == tokens.shape[1] and bool(state.keymask[:9].any())


@pytest.mark.parametrize("name", ["A", "B"])
def test_decode_step_matches_forward_past_the_initial_capacity(lms, dev, name):
    from speechbrain_amd._kvdec import INITIAL_CAPACITY
    g, models = lms
    gen = torch.Generator().manual_seed(9)
    tokens = torch.randint(1, 30, (6, INITIAL_CAPACITY + 8), generator=gen)
    tokens[:, 1:][torch.rand(6, INITIAL_CAPACITY + 7, generator=gen) < 0.2] = 0      # column 0 is never the padding
    state = _steps_match_forward(models[name], tokens.to(dev), permute_after=(10, 30, 35), tag=f"lm.{name} 40 steps")
    assert state.capacity == 2 * INITIAL_CAPACITY and state.steps == INITIAL_CAPACITY + 8


# --------------------------------------------------------------------------
# the searches
# --------------------------------------------------------------------------
LM_CASES = ["lm_w0.0", "lm_w0.4", "lm_tok0"]


@pytest.fixture(scope="module")
def search(golden, dev):
    """The ASR model of s2s.npz (as test_gpu_s2s_search.py loads it) and the LM of lm.npz."""
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from speechbrain_amd.nnet.linear import Linear
    s, g = golden("s2s"), golden("lm")
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=64, nhead=4, num_encoder_layers=1,
                        num_decoder_layers=2, d_ffn=128, dropout=0.0, activation=torch.nn.GELU,
                        normalize_before=True)
    seq_lin = Linear(input_size=64, n_neurons=23)
    ctc_lin = Linear(input_size=64, n_neurons=23)
    sd = _sub(s, "search.sd.tr.")
    sd[PE] = tr.state_dict()[PE]
    tr.load_state_dict(sd, strict=True)
    seq_lin.load_state_dict(_sub(s, "search.sd.seq."), strict=True)
    ctc_lin.load_state_dict(_sub(s, "search.sd.ctc."), strict=True)
    modules = [m.to(dev).eval() for m in (tr, seq_lin, ctc_lin)]
    lm = _load_lm(g, json.loads(str(g["search.lm_kw"])), "search.sd.lm.", dev)
    wav_len = torch.from_numpy(s["search.wav_len"]).to(dev)
    return g, modules, lm, torch.from_numpy(s["search.enc"]).to(dev), wav_len


def _enc_of(g, name, enc, dev):
    key = f"search.{name}.enc"
    return torch.from_numpy(g[key]).to(dev) if key in g.files else enc


def _forward_must_not_run(*a, **kw):
    raise AssertionError("TransformerLM.forward ran: the search did not take the LM's key/value cache")


def test_every_stored_search_case_is_tested(search):
    g = search[0]
    assert sorted(g["search.names"].tolist()) == sorted(LM_CASES)
    pred = g["search.lm_tok0.pred"]
    assert bool((pred == 0).any()), "the token-0 case decodes no 0"


@pytest.mark.parametrize("flag", [False, True], ids=["whole_prefix", "lm_kv_cache"])
@pytest.mark.parametrize("name", LM_CASES)
def test_lm_fusion_search_matches_reference(search, dev, monkeypatch, name, flag):
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    g, modules, lm, enc, wav_len = search
    cfg = json.loads(str(g[f"search.{name}.cfg"]))
    assert cfg["lm_weight"] == 0.6 and cfg["temperature_lm"] == 1.15
    searcher = S2STransformerBeamSearch(modules=modules, lm_modules=lm, **cfg)
    searcher.USE_LM_KV_CACHE = flag
    if flag:
        monkeypatch.setattr(lm, "forward", _forward_must_not_run)
    _check(g, name, searcher(_enc_of(g, name, enc, dev).clone(), wav_len))
    assert S2STransformerBeamSearch.USE_LM_KV_CACHE is False


def test_lm_fusion_search_with_both_caches(search, dev, monkeypatch):
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    g, modules, lm, enc, wav_len = search
    searcher = S2STransformerBeamSearch(modules=modules, lm_modules=lm, **json.loads(str(g["search.lm_w0.4.cfg"])))
    searcher.USE_LM_KV_CACHE = searcher.USE_KV_CACHE = True
    monkeypatch.setattr(lm, "forward", _forward_must_not_run)
    _check(g, "lm_w0.4", searcher(enc.clone(), wav_len))


@pytest.mark.parametrize("kind", ["head_size", "other_module"])
def test_unsupported_lm_with_the_flag_on_changes_nothing(search, dev, kind):
    """dh = 6, or an lm_modules that is no TransformerLM: the same hypotheses, scores and log_probs bit for
    bit with the flag on and off, and the module's forward is what ran."""
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM
    g, modules, _, enc, wav_len = search
    torch.manual_seed(23)
    lm = TransformerLM(vocab=23, d_model=24, nhead=4, num_encoder_layers=1, d_ffn=48, dropout=0.0,
                       activation=torch.nn.GELU).to(dev).eval()
    assert not lm.decode_step_supported()
    calls = []

    class Wrapped(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            calls.append(1)
            return self.inner(x)

    if kind == "other_module":
        torch.manual_seed(24)
        lm = Wrapped(TransformerLM(vocab=23, d_model=32, nhead=4, num_encoder_layers=1, d_ffn=48, dropout=0.0,
                                   activation=torch.nn.GELU).to(dev).eval())
    else:
        forward = lm.forward
        lm.forward = lambda *a, **kw: (calls.append(1), forward(*a, **kw))[1]
    cfg = {**json.loads(str(g["search.lm_w0.4.cfg"])), "max_decode_ratio": 0.4}
    res = []
    for flag in (False, True):
        s = S2STransformerBeamSearch(modules=modules, lm_modules=lm, **cfg)
        s.USE_LM_KV_CACHE = flag
        n = len(calls)
        res.append(s(enc.clone(), wav_len))
        assert len(calls) > n
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
