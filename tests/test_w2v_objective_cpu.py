"""CPU checks of the wav2vec 2.0 pre-training drop-ins against the reference
fixture (tests/golden/w2v_objective.npz, written by gen_w2v_golden.py from the
real reference): module structure and seeded init, the temperature schedule,
compute_mask and sample_negative_indices bit for bit, and the refusal of CPU
tensors by the HIP-backed loss and quantiser."""
import random

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def g(golden):
    return golden("w2v_objective")


def _sub(g, prefix):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def test_quantiser_state_dict_and_seeded_init(g):
    from speechbrain_amd.nnet.quantisers import GumbelVectorQuantizer
    torch.manual_seed(0)
    q = GumbelVectorQuantizer(24, 10, (2.0, 0.25, 0.999995), 2, 16)
    ref = _sub(g, "init.gvq.")
    sd = q.state_dict()
    assert sorted(sd) == sorted(ref) == sorted(["vars", "weight_proj.weight", "weight_proj.bias", "max_ent"])
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), ref[k]), k
    assert not q.max_ent.requires_grad and q.curr_temp == 2.0
    with pytest.raises(AssertionError):
        GumbelVectorQuantizer(24, 10, (2.0, 0.25, 0.999995), 3, 16)  # vq_dim % groups
    with pytest.raises(AssertionError):
        GumbelVectorQuantizer(24, 10, (2.0, 0.25), 2, 16)


def test_target_quantiser_state_dict_and_seeded_init(g):
    from speechbrain_amd.lobes.models.wav2vec import W2VTargetQuantiser
    torch.manual_seed(0)
    tq = W2VTargetQuantiser(24, 16, num_vars=10)
    ref = _sub(g, "init.tq.")
    sd = tq.state_dict()
    assert sorted(sd) == sorted(ref)
    assert all(k.startswith(("quantiser.", "proj.")) for k in sd)
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), ref[k]), k


def test_update_temp(g):
    from speechbrain_amd.nnet.quantisers import GumbelVectorQuantizer
    q = GumbelVectorQuantizer(24, 10, (2.0, 0.25, 0.999995), 2, 16)
    for s, v in zip(g["temp.steps"], g["temp.values"]):
        q.update_temp(int(s))
        assert q.curr_temp == float(v)
    assert q.curr_temp == 0.25  # the floor


@pytest.mark.parametrize("i", [0, 1, 2])
def test_compute_mask_bit_identical(g, i):
    from speechbrain_amd.lobes.models.wav2vec import compute_mask
    k = f"mask{i}"
    seed = int(g[k + ".seed"])
    random.seed(seed)
    np.random.seed(seed)
    mask = compute_mask(tuple(int(v) for v in g[k + ".shape"]), [int(v) for v in g[k + ".lens"]],
                        float(g[k + ".prob"]), int(g[k + ".length"]))
    assert mask.dtype == np.bool_ and np.array_equal(mask, g[k + ".mask"])
    for row, n in zip(mask, g[k + ".lens"]):
        assert not row[int(n):].any()  # nothing in the padding


def test_mask_collate_fn(g):
    from speechbrain_amd.lobes.models.wav2vec import W2VLatentExtractor, compute_mask, w2v_mask_collate_fn
    ext = W2VLatentExtractor(out_channels=[8, 8], kernel_sizes=[11, 3], strides=[5, 2])
    sigs = [torch.randn(1200), torch.randn(900)]
    samples = [{"id": str(i), "sig": s} for i, s in enumerate(sigs)]
    random.seed(4)
    np.random.seed(4)
    wavs, lens, mask = w2v_mask_collate_fn(samples, ext.get_output_lengths, 0.5, 4)
    assert wavs.shape == (2, 1200) and torch.equal(wavs[1, :900], sigs[1]) and not wavs[1, 900:].any()
    assert torch.allclose(lens, torch.tensor([1.0, 0.75]))
    tl = [int(ext.get_output_lengths(torch.as_tensor(s.numel()))) for s in sigs]
    random.seed(4)
    np.random.seed(4)
    assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), compute_mask((2, max(tl)), tl, 0.5, 4))


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4])
def test_sample_negative_indices_bit_identical(g, i):
    from speechbrain_amd.lobes.models.wav2vec import sample_negative_indices, sample_negatives
    k = f"neg{i}"
    B, T, N = (int(g[k + "." + n]) for n in ("B", "T", "N"))
    y = torch.arange(B * T * 3, dtype=torch.float32).view(B, T, 3)
    torch.manual_seed(int(g[k + ".seed"]))
    idx = sample_negative_indices(y, N)
    assert idx.shape == (B, T * N) and idx.dtype == torch.int64
    assert np.array_equal(idx.numpy(), g[k + ".idx"])
    # the materialised negatives are those rows, in the reference's (N, B, T, C) layout
    torch.manual_seed(int(g[k + ".seed"]))
    negs = sample_negatives(y, N)
    assert negs.shape == (N, B, T, 3)
    assert torch.equal(negs, y.view(-1, 3)[idx.view(-1)].view(B, T, N, 3).permute(2, 0, 1, 3))


def test_negative_indices_keep_the_reference_batch_offset(g):
    """B = 3, T = 7: utterance b's negatives come from rows b·(T-1) ..
    b·(T-1) + T-1 of y.view(-1, C) — the reference's offset, not b·T — so the
    last utterance reaches into the one before it."""
    idx = g["neg1.idx"]
    assert int(g["neg1.B"]) == 3 and int(g["neg1.T"]) == 7
    for b in range(3):
        assert idx[b].min() >= 6 * b and idx[b].max() <= 6 * b + 6
    assert (idx[2] < 14).any()  # rows 12, 13 belong to utterance 1


def test_sample_negatives_is_differentiable():
    from speechbrain_amd.lobes.models.wav2vec import sample_negatives
    y = torch.randn(2, 5, 4, requires_grad=True)
    torch.manual_seed(0)
    sample_negatives(y, 3).sum().backward()
    assert y.grad is not None and float(y.grad.sum()) == 2 * 5 * 3 * 4


def test_get_output_lengths_unchanged(g):
    from speechbrain_amd.lobes.models.wav2vec import W2VLatentExtractor
    ext = W2VLatentExtractor(out_channels=[4] * 7)
    out = ext.get_output_lengths(torch.from_numpy(g["outlen.in"]))
    assert out.dtype == torch.long and np.array_equal(out.numpy(), g["outlen.out"])


def test_exports():
    from speechbrain_amd.lobes.models import wav2vec
    for name in ("W2VTargetQuantiser", "compute_mask", "sample_negatives", "sample_negative_indices",
                 "w2v_mask_collate_fn", "W2VLatentExtractor", "EncoderWrapper"):
        assert name in wav2vec.__all__ and hasattr(wav2vec, name)


def test_cpu_tensors_are_refused():
    from speechbrain_amd._lib import SbkError
    from speechbrain_amd.lobes.models.wav2vec import W2VTargetQuantiser, sample_negative_indices, sample_negatives
    from speechbrain_amd.nnet.losses import ContrastiveLoss
    from speechbrain_amd.nnet.quantisers import GumbelVectorQuantizer
    x, y = torch.randn(2, 5, 8), torch.randn(2, 5, 8)
    loss = ContrastiveLoss(0.1)
    with pytest.raises(SbkError):
        loss(x, y, sample_negatives(y, 3))
    with pytest.raises(SbkError):
        loss(x, y, sample_negative_indices(y, 3))
    with pytest.raises(SbkError):
        GumbelVectorQuantizer(8, 6, (2.0, 0.25, 0.999995), 2, 4)(x)
    with pytest.raises(SbkError):
        W2VTargetQuantiser(8, 4, num_vars=6)(x)


def test_entry_points_refuse_bad_arguments():
    """R, C, N <= 0 and a groups·num_vars that does not match vars: 1001 before
    any launch (argument checks only: no GPU is touched)."""
    from speechbrain_amd import _lib
    L = _lib.lib()
    for R, C, N in ((0, 8, 3), (4, 0, 3), (4, 8, 0), (-1, 8, 3)):
        assert L.sbk_w2v_contrast_fwd(None, None, None, None, R, C, N, 0, 0, 0.1, None, None, None, None, None) == 1001
        assert L.sbk_w2v_contrast_bwd_x(None, None, None, None, None, None, None, R, C, N, 0, 0, 0.1, None, None, None,
                                        None, None, None) == 1001
        assert L.sbk_w2v_contrast_bwd_y(None, None, None, None, None, None, R, C, N, None, None) == 1001
    # G·V = 2·10 against 19 rows of vars
    assert L.sbk_gumbel_vq_fwd(None, None, 1.0, 4, 2, 10, None, 19, 8, None, None, None, None, None, None) == 1001
    assert L.sbk_gumbel_vq_bwd(None, None, None, None, None, 1.0, None, None, 4, 2, 10, 19, 8, None, None, None) == 1001
    assert L.sbk_gumbel_vq_fwd(None, None, 1.0, 0, 2, 10, None, 20, 8, None, None, None, None, None, None) == 1001


def test_kernel_cosine_formula_is_torchs():
    """csrc/w2vloss.hip computes <a, b> / (max(|a|, eps) · max(|b|, eps)), eps =
    1e-8.  That is the installed torch's cosine_similarity, also for rows whose
    norm is below eps or zero, where the older <a, b> / sqrt(max(|a|²|b|², eps²))
    form gives something else."""
    torch.manual_seed(0)
    a, b = torch.randn(6, 9, dtype=torch.float64), torch.randn(6, 9, dtype=torch.float64)
    a[0] *= 1e-9
    b[1] *= 1e-9
    a[2] = 0
    a[3] *= 1e-9
    b[3] *= 1e-9
    eps = 1e-8
    na, nb = a.norm(dim=-1), b.norm(dim=-1)
    mine = (a * b).sum(-1) / (na.clamp_min(eps) * nb.clamp_min(eps))
    ref = torch.cosine_similarity(a, b, dim=-1, eps=eps)
    assert torch.allclose(mine, ref, rtol=1e-12, atol=0)
    old = (a * b).sum(-1) / torch.sqrt((na * na * nb * nb).clamp_min(eps * eps))
    assert not torch.allclose(old[:2], ref[:2], rtol=1e-3, atol=0)
