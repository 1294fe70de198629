"""Incremental transformer decoding on the GPU (csrc/kvdec.hip,
TransformerASR.decode_step, S2STransformerBeamSearch.USE_KV_CACHE).

  * the two kernels against a float64 restatement written here with torch on
    the CPU (the self-attention one gathering through the ancestry table);
  * decode_step against decode() of the whole prefix, step by step — decode()
    is pinned to the reference by test_gpu_recipe.py;
  * the cached search against tests/golden/s2s.npz with model.decode patched
    to raise, so only the cached path can have produced the result.

Bound: conftest.assert_close's |a − b| <= 1e-4·max(1, |b|), the project's fp32
parity bound; every test prints the largest deviation it saw."""
import json
import math

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_gpu_s2s_search import CASES, _check, _unpad

pytestmark = pytest.mark.gpu


def _dev(name, a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    print(f"{name}: max deviation {float(np.max(np.abs(a - b) / np.maximum(1, np.abs(b)))):.3e}")


# --------------------------------------------------------------------------
# kernels
# --------------------------------------------------------------------------
def _self_case(N, H, dh, L, seed):
    """qkv (N, 3E), caches (cap, N, E) filled everywhere, anc (N, cap): rows 0
    and 1 share an ancestor at even positions, rows 2 and 3 swap at odd ones
    (their chains cross), the rest is drawn; anc[:, L−1] = the row itself."""
    g = torch.Generator().manual_seed(seed)
    E, cap = H * dh, L + 3
    qkv = torch.randn(N, 3 * E, generator=g)
    kc = torch.randn(cap, N, E, generator=g)
    vc = torch.randn(cap, N, E, generator=g)
    anc = torch.randint(0, N, (N, cap), generator=g, dtype=torch.int32)
    anc[1, 0::2] = anc[0, 0::2]
    anc[2, 1::2] = 3
    anc[3, 1::2] = 2
    anc[:, L - 1] = torch.arange(N, dtype=torch.int32)
    return qkv, kc, vc, anc


def _self_ref(qkv, kc, vc, anc, H, L):
    """float64: row n attends kc / vc[j][clamp(anc[n][j])] for j < L−1 and its own new k / v at L−1."""
    N, E3 = qkv.shape
    E = E3 // 3
    dh = E // H
    q, k_new, v_new = (t.double() for t in qkv.split(E, dim=1))
    a = anc[:, :L].long().clamp(0, N - 1)
    pos = torch.arange(L)
    keys = kc.double()[pos[None, :], a]                         # (N, L, E)
    vals = vc.double()[pos[None, :], a]
    keys[:, L - 1] = k_new
    vals[:, L - 1] = v_new
    qh = q.view(N, H, 1, dh)
    kh = keys.view(N, L, H, dh).transpose(1, 2)
    vh = vals.view(N, L, H, dh).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    return (p @ vh).reshape(N, E)


def _run_self(dev, qkv, kc, vc, anc, H, L):
    from speechbrain_amd._kvdec import kv_decode_self_attn
    E = qkv.shape[1] // 3
    kc_d, vc_d = kc.to(dev), vc.to(dev)
    out = kv_decode_self_attn(qkv.to(dev), kc_d, vc_d, anc.to(dev), H, L)
    torch.cuda.current_stream().synchronize()
    for name, cache, new, before in (("kc", kc_d, qkv[:, E:2 * E], kc), ("vc", vc_d, qkv[:, 2 * E:], vc)):
        got = cache.cpu()
        assert torch.equal(got[L - 1], new), f"{name}: slot L-1 is not the step's row bit for bit"
        keep = torch.ones(before.shape[0], dtype=torch.bool)
        keep[L - 1] = False
        assert torch.equal(got[keep], before[keep]), f"{name}: a slot other than L-1 changed"
    return out


@pytest.mark.parametrize("L", [1, 2, 64, 65, 130])
@pytest.mark.parametrize("dh", [16, 20, 64, 128])
def test_self_attn_kernel(dev, dh, L):
    N, H = 6, 2
    qkv, kc, vc, anc = _self_case(N, H, dh, L, seed=1000 * dh + L)
    out = _run_self(dev, qkv, kc, vc, anc, H, L)
    ref = _self_ref(qkv, kc, vc, anc, H, L)
    _dev(f"self dh={dh} L={L}", out, ref)
    assert_close(out, ref.float(), name=f"self dh={dh} L={L}")


def test_self_attn_kernel_on_a_side_stream(dev):
    N, H, dh, L = 6, 2, 64, 65
    qkv, kc, vc, anc = _self_case(N, H, dh, L, seed=7)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = _run_self(dev, qkv, kc, vc, anc, H, L)
    side.synchronize()
    assert_close(out, _self_ref(qkv, kc, vc, anc, H, L).float(), name="self side stream")


def test_self_attn_kernel_clamps_the_ancestry_table(dev):
    """Values outside [0, N) are clamped, never used as they are."""
    N, H, dh, L = 6, 2, 16, 9
    qkv, kc, vc, anc = _self_case(N, H, dh, L, seed=11)
    anc[0, 0], anc[1, 1], anc[4, 2], anc[5, 3] = -5, N, N + 40, -1
    out = _run_self(dev, qkv, kc, vc, anc, H, L)
    assert_close(out, _self_ref(qkv, kc, vc, anc, H, L).float(), name="self clamp")


def _cross_ref(q, kv, klen, group, H):
    """float64 → (out (N, E), probs (N, H, S)); keys j ≥ klen get probability 0."""
    N, E = q.shape
    B, S, _ = kv.shape
    dh = E // H
    k, v = (t.double().repeat_interleave(group, dim=0) for t in kv.split(E, dim=2))     # (N, S, E)
    s = q.double().view(N, H, 1, dh) @ k.view(N, S, H, dh).permute(0, 2, 3, 1) / math.sqrt(dh)   # (N, H, 1, S)
    if klen is not None:
        masked = torch.arange(S)[None, :] >= klen.long()[:, None]
        s = s.masked_fill(masked[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = p @ v.view(N, S, H, dh).transpose(1, 2)
    return out.reshape(N, E), p.reshape(N, H, S)


@pytest.mark.parametrize("S", [21, 64, 65, 257])
@pytest.mark.parametrize("group", [1, 4, 10, 17])
@pytest.mark.parametrize("dh", [16, 64])
def test_cross_attn_kernel(dev, dh, group, S):
    from speechbrain_amd._kvdec import kv_decode_cross_attn
    B, H = 3, 2
    N, E = B * group, H * dh
    g = torch.Generator().manual_seed(10000 * dh + 100 * group + S)
    q = torch.randn(N, E, generator=g)
    kv = torch.randn(B * S, 2 * E, generator=g).view(B, S, 2 * E)       # K and V: the blocks of one tensor
    ragged = torch.randint(1, S + 1, (N,), generator=g, dtype=torch.int32)
    ragged[0], ragged[-1] = 1, S
    q_d, kv_d = q.to(dev), kv.to(dev)
    for klen in (None, ragged):
        tag = f"cross dh={dh} group={group} S={S} klen={'none' if klen is None else 'ragged'}"
        klen_d = None if klen is None else klen.to(dev)
        out, probs = kv_decode_cross_attn(q_d, kv_d, klen_d, group, H, True)
        out_only, none = kv_decode_cross_attn(q_d, kv_d, klen_d, group, H, False)
        ref_out, ref_probs = _cross_ref(q, kv, klen, group, H)
        _dev(tag + " out", out, ref_out)
        _dev(tag + " probs", probs, ref_probs)
        assert_close(out, ref_out.float(), name=tag + " out")
        assert_close(probs, ref_probs.float(), name=tag + " probs")
        assert none.numel() == 0 and torch.equal(out_only, out), tag + ": out differs when probs is not asked for"
        sums = probs.double().sum(-1).cpu()
        assert float((sums - 1).abs().max()) <= 1e-5, tag
        if klen is not None:
            masked = (torch.arange(S)[None, :] >= klen.long()[:, None])[:, None, :].expand(N, H, S)
            assert bool((probs.cpu()[masked] == 0).all()), tag + ": a key at j >= klen has weight"


# --------------------------------------------------------------------------
# decode_step against decode() of the whole prefix
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(golden, dev):
    """The s2s.npz model, loaded as test_gpu_s2s_search.py does."""
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from speechbrain_amd.nnet.linear import Linear
    g = golden("s2s")
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=64, nhead=4, num_encoder_layers=1,
                        num_decoder_layers=2, d_ffn=128, dropout=0.0, activation=torch.nn.GELU,
                        normalize_before=True)
    seq_lin = Linear(input_size=64, n_neurons=23)
    ctc_lin = Linear(input_size=64, n_neurons=23)

    def sub(prefix):
        return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}

    sd = sub("search.sd.tr.")
    sd["positional_encoding.pe"] = tr.state_dict()["positional_encoding.pe"]
    tr.load_state_dict(sd, strict=True)
    seq_lin.load_state_dict(sub("search.sd.seq."), strict=True)
    ctc_lin.load_state_dict(sub("search.sd.ctc."), strict=True)
    modules = [m.to(dev).eval() for m in (tr, seq_lin, ctc_lin)]
    enc = torch.from_numpy(g["search.enc"]).to(dev)
    wav_len = torch.from_numpy(g["search.wav_len"]).to(dev)
    return g, modules, enc, wav_len


def _steps_match_decode(tr, enc, tokens, group, enc_len=None, permute_after=(), tag=""):
    """decode_step at every t against decode(prefixes)[:, -1:].  tokens (N, T)
    are the tokens fed at each step; after the steps in permute_after the
    rows are permuted (state.permute) and so are the prefixes decode() sees."""
    N, T = tokens.shape
    enc_inf = enc.repeat_interleave(group, dim=0)
    len_inf = None if enc_len is None else enc_len.repeat_interleave(group)
    state = tr.init_decode_state(enc, enc_len=enc_len, group=group)
    prefixes = tokens[:, :0]
    worst = 0.0
    g = torch.Generator().manual_seed(3)
    for t in range(T):
        prefixes = torch.cat([prefixes, tokens[:, t:t + 1]], dim=1)
        pred, attn = tr.decode_step(tokens[:, t], state)
        want_pred, want_attn = tr.decode(prefixes, enc_inf, len_inf)
        assert pred.shape == (N, 1, want_pred.shape[-1]) and attn.shape == (N, 1, enc.shape[1])
        for got, want in ((pred, want_pred[:, -1:]), (attn, want_attn[:, -1:])):
            worst = max(worst, float(((got - want).abs() / want.abs().clamp(min=1)).max()))
        assert_close(pred, want_pred[:, -1:], name=f"{tag} prediction at t={t}")
        assert_close(attn, want_attn[:, -1:], name=f"{tag} attn at t={t}")
        if t in permute_after:
            # within an utterance's group, as a beam search permutes
            index = (torch.randint(0, group, (N,), generator=g) + torch.arange(N) // group * group).to(enc.device)
            assert state.permute(index) is state
            prefixes = prefixes.index_select(0, index)
    print(f"{tag}: max deviation {worst:.3e} over {T} steps")
    return state


def _tokens(N, T, vocab, dev, seed=5):
    return torch.randint(0, vocab, (N, T), generator=torch.Generator().manual_seed(seed)).to(dev)


def test_step_matches_whole_prefix_decode(setup, dev):
    g, modules, enc, wav_len = setup
    B = 3
    _steps_match_decode(modules[0], enc[:B], _tokens(6, 12, 23, dev), group=2, tag="plain")


def test_step_matches_decode_after_beam_permutations(setup, dev):
    g, modules, enc, wav_len = setup
    _steps_match_decode(modules[0], enc[:3], _tokens(6, 12, 23, dev), group=2, permute_after=(3, 7), tag="permuted")


def test_step_matches_decode_with_enc_len(setup, dev):
    g, modules, enc, wav_len = setup
    S = enc.shape[1]
    enc_len = torch.tensor([S, max(1, S // 2), max(1, S - 3)], device=dev)       # decode() needs max = S
    _steps_match_decode(modules[0], enc[:3], _tokens(6, 12, 23, dev), group=2, enc_len=enc_len, tag="enc_len")


def test_step_matches_decode_over_forty_steps(setup, dev):
    """The capacity doubles once past 32 positions."""
    g, modules, enc, wav_len = setup
    state = _steps_match_decode(modules[0], enc[:3], _tokens(6, 40, 23, dev), group=2, permute_after=(30, 35),
                                tag="40 steps")
    assert state.capacity == 64 and state.steps == 40


def test_step_matches_decode_post_norm(setup, dev):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    g, modules, enc, wav_len = setup
    torch.manual_seed(21)
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=64, nhead=4, num_encoder_layers=1, num_decoder_layers=2,
                        d_ffn=128, dropout=0.0, activation=torch.nn.GELU, normalize_before=False).to(dev).eval()
    _steps_match_decode(tr, enc[:3], _tokens(6, 12, 23, dev), group=2, permute_after=(3, 7), tag="post-norm")


def test_step_matches_decode_relpos_conformer(setup, dev):
    """RelPosMHAXL: the decoder's sine table is added to the encoder states too."""
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    g, modules, enc, wav_len = setup
    torch.manual_seed(22)
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=64, nhead=4, num_encoder_layers=1, num_decoder_layers=2,
                        d_ffn=128, dropout=0.0, activation=torch.nn.GELU, normalize_before=True,
                        attention_type="RelPosMHAXL", encoder_module="conformer").to(dev).eval()
    _steps_match_decode(tr, enc[:3], _tokens(6, 12, 23, dev), group=2, permute_after=(3, 7), tag="relpos")


# --------------------------------------------------------------------------
# the search
# --------------------------------------------------------------------------
def _decode_must_not_run(*a, **kw):
    raise AssertionError("model.decode ran: the search did not take the key/value cache path")


@pytest.mark.parametrize("name", CASES)
def test_cached_beam_search_matches_reference(setup, monkeypatch, name):
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    g, modules, enc, wav_len = setup
    cfg = json.loads(str(g[f"search.{name}.cfg"]))
    searcher = S2STransformerBeamSearch(modules=modules, **cfg)
    searcher.USE_KV_CACHE = True
    monkeypatch.setattr(modules[0], "decode", _decode_must_not_run)
    _check(g, name, searcher(enc.clone(), wav_len))
    assert S2STransformerBeamSearch.USE_KV_CACHE is False


def test_cached_search_on_a_side_stream(setup, monkeypatch):
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    g, modules, enc, wav_len = setup
    cfg = json.loads(str(g["search.w0.4_partial.cfg"]))
    searcher = S2STransformerBeamSearch(modules=modules, **cfg)
    searcher.USE_KV_CACHE = True
    monkeypatch.setattr(modules[0], "decode", _decode_must_not_run)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = searcher(enc.clone(), wav_len)
    side.synchronize()
    _check(g, "w0.4_partial", res)


def test_cached_greedy_searcher_matches_reference(setup, monkeypatch):
    from speechbrain_amd.decoders.seq2seq import S2SGreedySearcher
    g, modules, enc, wav_len = setup

    class Greedy(S2SGreedySearcher):
        def __init__(self, modules, **kw):
            super().__init__(**kw)
            self.model, self.fc = modules[0], modules[1]

        def reset_mem(self, batch_size, device):
            return None

        def forward_step(self, inp_tokens, memory, enc_states, enc_lens):
            if memory is None:
                memory = self.model.init_decode_state(enc_states)
            pred, attn = self.model.decode_step(inp_tokens, memory)
            return self.fc(pred).log_softmax(-1)[:, -1, :], memory, attn

    monkeypatch.setattr(modules[0], "decode", _decode_must_not_run)
    pred, scores = Greedy(modules, bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0)(enc, wav_len)
    assert pred == _unpad(g["greedy.pred"], -1)
    _dev("greedy.scores", np.asarray(scores), g["greedy.scores"])
    assert_close(np.asarray(scores, dtype=np.float32), g["greedy.scores"], name="greedy.scores")


def test_unsupported_head_size_falls_back_to_whole_prefix_decode(setup, dev):
    """dh = 6: the flag changes nothing — same hypotheses, same scores, and decode() is what ran."""
    from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from speechbrain_amd.nnet.linear import Linear
    torch.manual_seed(23)
    tr = TransformerASR(tgt_vocab=23, input_size=40, d_model=24, nhead=4, num_encoder_layers=1, num_decoder_layers=2,
                        d_ffn=48, dropout=0.0, activation=torch.nn.GELU, normalize_before=True).to(dev).eval()
    assert not tr.decode_step_supported()
    modules = [tr, Linear(input_size=24, n_neurons=23).to(dev).eval(), Linear(input_size=24, n_neurons=23).to(dev).eval()]
    enc = torch.randn(2, 9, 24, device=dev)
    wav_len = torch.tensor([1.0, 0.8], device=dev)
    calls = []
    decode = tr.decode
    tr.decode = lambda *a, **kw: (calls.append(1), decode(*a, **kw))[1]
    res = []
    for flag in (False, True):
        s = S2STransformerBeamSearch(modules=modules, bos_index=1, eos_index=2, min_decode_ratio=0.0,
                                     max_decode_ratio=1.0, beam_size=3, return_log_probs=True)
        s.USE_KV_CACHE = flag
        n = len(calls)
        res.append(s(enc.clone(), wav_len))
        assert len(calls) > n
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
