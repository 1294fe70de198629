"""What gen_rnn_search_golden.py and tests/test_gpu_rnn_search.py share: the
fixture's module sizes, its stand-in GRU language model ((tokens (N), hx) ->
(logits (N, V), hx (1, N, dim)), one step per call) and how a case's cfg
becomes a searcher, over the reference's classes or the package's."""
import torch

DEC = dict(rnn_type="gru", hidden_size=16, attn_dim=12, num_layers=1, enc_dim=20, input_size=8, scaling=2.0,
           channels=5, kernel_size=7, dropout=0.0)
TLM = dict(vocab=23, d_model=24, nhead=4, num_encoder_layers=1, num_decoder_layers=0, d_ffn=48, dropout=0.0)


class TinyGRULM(torch.nn.Module):
    def __init__(self, vocab=23, dim=16):
        super().__init__()
        self.emb = torch.nn.Embedding(vocab, dim)
        self.rnn = torch.nn.GRU(dim, dim, batch_first=True)
        self.out = torch.nn.Linear(dim, vocab)

    def forward(self, tokens, hx=None):
        y, h = self.rnn(self.emb(tokens).unsqueeze(1), hx)
        return self.out(y[:, 0]), h


def build_modules(AttentionalRNNDecoder, Embedding, Linear, TransformerLM):
    return {"dec.location": AttentionalRNNDecoder(attn_type="location", **DEC),
            "dec.content": AttentionalRNNDecoder(attn_type="content", **DEC),
            "emb": Embedding(23, 8), "fc": Linear(input_size=16, n_neurons=23),
            "ctc": Linear(input_size=20, n_neurons=23), "gru_lm": TinyGRULM(23, 16),
            "tlm": TransformerLM(activation=torch.nn.GELU, **TLM)}


def make_searcher(ns, m, cfg):
    """ns: the module or namespace that holds the searcher classes."""
    kw = {k: v for k, v in cfg.items() if k not in ("cls", "kind")}
    args = dict(embedding=m["emb"], decoder=m["dec." + cfg["kind"]], linear=m["fc"])
    if cfg["cls"] == "S2SRNNGreedySearcher":
        kw.pop("blank_index")
    elif cfg["cls"] == "S2SRNNBeamSearchLM":
        args["language_model"] = m["gru_lm"]
    elif cfg["cls"] == "S2SRNNBeamSearchTransformerLM":
        args["language_model"] = m["tlm"]
    if kw.get("ctc_weight", 0) > 0:
        args["ctc_linear"] = m["ctc"]
    return getattr(ns, cfg["cls"])(**args, **kw)
