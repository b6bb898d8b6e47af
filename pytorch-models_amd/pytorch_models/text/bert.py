"""BERT / RoBERTa encoder on MI355X: drop-in for /root/reference pytorch_models/text/bert.py (BERT, from_hf,
load_hf_state_dict; parameter names token_embs, pos_embs, norm, layers).  Token-type embeddings, pooler and classifier
are not part of the reference class either (bert.py:14); the token-type row 0 is merged into pos_embs at load time."""
from __future__ import annotations

import math

import torch
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..transformer import Encoder, LayerNorm, _f32, _wb


class BERT(nn.Module):
    def __init__(self, vocab_size: int, n_layers: int, d_model: int, max_seq_len: int = 512, dropout: float = 0.0,
                 norm_eps: float = 1e-12) -> None:
        super().__init__()
        vocab_size = math.ceil(vocab_size / 64) * 64  # padded to a multiple of 64, as the reference does (bert.py:29)
        self.token_embs = nn.Embedding(vocab_size, d_model)
        self.pos_embs = nn.Parameter(torch.zeros(max_seq_len, d_model))
        self.norm = LayerNorm(d_model, norm_eps)
        self.layers = Encoder(n_layers, d_model, dropout=dropout, pre_norm=False, norm_eps=norm_eps)

    def forward(self, x: Tensor, lengths=None) -> Tensor:
        """token ids (..., L) int64 -> hidden states (..., L, d) bf16 (bert.py:35-40).
        ``lengths`` (B ints or an integer tensor, each in 1..L; ``x`` is then (B, L), right-padded): a ragged batch.  Row b on
        [:lengths[b]] is what forward(x[b:b+1, :lengths[b]]) returns, rows past the length are exactly 0, and no padded position
        is embedded, normalised, multiplied or attended to: the batch runs as one packed (sum(lengths), d) matrix
        (pm_embed_tokens_varlen, the row-wise kernels as they are, pm_attention_varlen_bf16, pm_rows_unpack)."""
        if lengths is not None:
            h, seq = self._packed_hidden(x, lengths)
            return _cpu.rows_unpack(h, seq.lengths, seq.L) if not h.is_cuda else ops.rows_unpack(h, seq)
        E = self.token_embs.weight  # fp32 table -> fp32 rows (and fp32 blocks behind them), bf16 -> bf16
        lead = x.shape
        h = ops.embed_tokens(x.reshape(-1, lead[-1]), E, _f32(self, "pos", self.pos_embs))
        h = self.layers(self.norm(h))
        return h.view(*lead, h.shape[-1])

    def _packed_hidden(self, x: Tensor, lengths):
        """The packed hidden state (sum(lengths), d) of a right-padded (B, L) batch and its extents (ops.SeqLens)."""
        if x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError(f"BERT: with lengths the ids must be int64 (B, L), got {tuple(x.shape)} {x.dtype}")
        B, L = x.shape
        E = self.token_embs.weight
        cpu = _cpu.on_cpu(x, E)
        seq = ops.seq_lens([L] * B if lengths is None else lengths, L, x.device, lo=1)
        if seq.B != B:
            raise ValueError(f"BERT: {seq.B} lengths for a batch of {B}")
        if L > self.pos_embs.shape[0]:
            raise ValueError(f"BERT: {L} positions, the model has {self.pos_embs.shape[0]}")
        if cpu:
            h = _cpu.rows_pack(_cpu.embed_tokens(x, E, self.pos_embs), seq.lengths)
        else:
            if E.is_cuda and E.dtype != torch.bfloat16:
                raise NotImplementedError(f"BERT: variable-length batches need bf16 parameters (got {E.dtype}); call model.to(torch.bfloat16)")
            h = ops.embed_tokens_varlen(x, E, _f32(self, "pos", self.pos_embs), seq)
        return self.layers.forward_packed(self.norm(h), seq), seq

    def embed(self, x: Tensor, lengths=None, pool: str = "mean") -> Tensor:
        """One fp32 (B, d) vector per sequence of a right-padded (B, L) batch: ``pool="mean"`` is the mean of the valid rows of
        the last hidden state (pm_segment_mean: fp32 sums in row order), ``"cls"`` each sequence's first row.  Taken from the
        packed hidden state - nothing is unpacked.  ``lengths=None``: every row is full."""
        if pool not in ("mean", "cls"):
            raise ValueError(f"BERT.embed: pool must be 'mean' or 'cls', got {pool!r}")
        h, seq = self._packed_hidden(x, lengths)
        if pool == "cls":
            return h[seq.cu[:-1].long()].float()
        return ops.segment_mean(h, seq) if h.is_cuda else _cpu.segment_mean(h, seq.lengths)

    @staticmethod
    def from_config(config: dict, **kwargs) -> "BERT":
        """A Hugging Face config.json as a dict (the reference downloads it: bert.py:44-58; here it is passed in)."""
        max_pos = config["max_position_embeddings"]
        if "roberta" in config["model_type"]:  # RoBERTa never uses its first two position rows (bert.py:56-58)
            max_pos -= 2
        return BERT(vocab_size=config["vocab_size"], n_layers=config["num_hidden_layers"], d_model=config["hidden_size"],
                    max_seq_len=max_pos, norm_eps=config["layer_norm_eps"], **kwargs)

    @staticmethod
    def from_hf(model_tag: str, *, pretrained: bool = False, **kwargs) -> "BERT":
        raise NotImplementedError(
            f"BERT.from_hf({model_tag!r}) fetches config.json (and weights) from the network, which this build does not do; "
            "use BERT.from_config(json.load(open('config.json'))) and load_hf_state_dict(torch.load(path, weights_only=True)).")

    def load_hf_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        """Hugging Face BertModel / RobertaModel state_dict (converters.load_hf_bert; placement as bert.py:79-107)."""
        from ..converters import load_hf_bert

        load_hf_bert(self, state_dict)
