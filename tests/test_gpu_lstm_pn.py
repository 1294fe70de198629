"""A transducer prediction network emb -> dec -> dec_lin whose `dec` is the
LSTM drop-in (speechbrain_amd Embedding(consider_as_one_hot) -> LSTM ->
Linear) under TransducerBeamSearcher, greedy and beam search: the searcher
dispatches on the class name `LSTM` and carries the (h, c) tuple per
hypothesis.  Compared against the same searcher given torch.nn modules on the
GPU: identical token sequences, scores within 1e-4.

The admission rule, the blank biases and the counting guard are those of
test_gpu_transducer_pn.py: a case is admitted only if the torch-module searcher
returns the same hypotheses when the encoder output is multiplied by
1 + 1e-4 * randn, for three noise seeds, and decodes at least one token;
encoder seeds are tried in order and the first admitted one is used — a seed
that fails is replaced, never a tolerance.  The classifier's blank bias is +3
for the greedy decode and +5 for the beam search, and a counting wrapper
around the classifier fails the test after 2000 joint steps.
"""
import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu
V, H, J, BLANK = 40, 32, 32, 0


class TorchEmbedding(torch.nn.Module):
    """The reference's Embedding(consider_as_one_hot=True) on torch.nn.Embedding."""

    def __init__(self, table):
        super().__init__()
        self.Embedding = torch.nn.Embedding.from_pretrained(table.clone(), freeze=True)

    def forward(self, x):
        return self.Embedding(x.long())


class LSTM(torch.nn.Module):
    """speechbrain.nnet.RNN.LSTM's layout and call convention on torch.nn.LSTM
    (the searcher dispatches on the class name)."""

    def __init__(self, inp, hid):
        super().__init__()
        self.rnn = torch.nn.LSTM(inp, hid, batch_first=True)

    def forward(self, x, hx=None):
        return self.rnn(x, hx)


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    sd = {"rnn.weight_ih_l0": torch.randn(4 * H, V - 1, generator=g) / H ** 0.5,
          "rnn.weight_hh_l0": torch.randn(4 * H, H, generator=g) / H ** 0.5,
          "rnn.bias_ih_l0": torch.randn(4 * H, generator=g) / H ** 0.5,
          "rnn.bias_hh_l0": torch.randn(4 * H, generator=g) / H ** 0.5}
    return sd, torch.randn(J, H, generator=g) / H ** 0.5


class Counted(torch.nn.Module):
    """The classifier, failing the test if a search runs away."""

    def __init__(self, lin):
        super().__init__()
        self.lin, self.calls = lin, 0

    def forward(self, x):
        self.calls += 1
        if self.calls > 2000:
            raise AssertionError("the search does not end: blank is too rarely among the best tokens")
        return self.lin(x)


def _searchers(dev, beam):
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.nnet.RNN import LSTM as SbkLSTM
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.transducer.transducer_joint import Transducer_joint
    sd, wlin = _weights(3)
    g = torch.Generator().manual_seed(4)
    dec_lin = Linear(J, input_size=H, bias=False)
    dec_lin.load_state_dict({"w.weight": wlin})
    cls = Linear(V, input_size=J)
    weight = torch.randn(V, J, generator=g) / J ** 0.5
    bias = 0.5 * torch.randn(V, generator=g)
    bias[BLANK] += 3.0 if beam <= 1 else 5.0
    cls.load_state_dict({"w.weight": weight, "w.bias": bias})
    dec_lin, cls = dec_lin.to(dev).eval(), Counted(cls.to(dev).eval())
    tjoint = Transducer_joint(joint="sum", nonlinearity=torch.nn.LeakyReLU)
    emb = Embedding(V, consider_as_one_hot=True, blank_id=BLANK).to(dev).eval()
    dec = SbkLSTM(H, input_size=V - 1)
    dec.load_state_dict(sd, strict=True)
    temb = TorchEmbedding(R.onehot_table(V, BLANK).float()).to(dev).eval()
    tdec = LSTM(V - 1, H)
    tdec.load_state_dict(sd)
    kw = dict(tjoint=tjoint, classifier_network=[cls], blank_id=BLANK, beam_size=beam, nbest=2, lm_module=None,
              lm_weight=0.0, state_beam=2.3, expand_beam=2.3)
    ours = TransducerBeamSearcher(decode_network_lst=[emb, dec.to(dev).eval(), dec_lin], **kw)
    theirs = TransducerBeamSearcher(decode_network_lst=[temb, tdec.to(dev).eval(), dec_lin], **kw)
    return ours, theirs


def _hyps(res, beam):
    return res[0] if beam <= 1 else (res[0], res[2])


@pytest.mark.parametrize("beam", [1, 2], ids=["greedy", "beam2"])
def test_searcher_on_lstm_dropin_matches_torch_modules(dev, beam):
    ours, theirs = _searchers(dev, beam)

    def search(searcher, enc):
        searcher.classifier_network[0].calls = 0     # the 2000-step guard is per search
        return searcher(enc.to(dev))

    with torch.no_grad():
        for seed in range(200, 206):
            tn = 2.0 * torch.randn(2, 6, J, generator=torch.Generator().manual_seed(seed))
            base = search(theirs, tn)
            stable = any(len(h) > 0 for h in base[0])
            for ns in (101, 102, 103):
                noise = 1 + 1e-4 * torch.randn(tn.shape, generator=torch.Generator().manual_seed(ns))
                stable = stable and _hyps(search(theirs, tn * noise), beam) == _hyps(base, beam)
            if stable:
                break
            print(f"encoder seed {seed} not admitted")
        else:
            raise AssertionError("no encoder seed in 200..205 gives an admitted case")
        res = search(ours, tn)
    assert _hyps(res, beam) == _hyps(base, beam), (res[0], base[0])
    assert abs(float(res[1]) - float(base[1])) <= 1e-4
    if beam > 1:
        for a, b in zip(res[3], base[3]):
            for x, y in zip(a, b):
                assert abs(float(x) - float(y)) <= 1e-4
