"""CTC heads for the wav2vec2 family (Wav2Vec2 / HuBERT, Data2VecAudio, SEW): transcripts, likelihoods and timestamps from the
encoders' hidden rows.  Beyond the reference, which stops at hidden states ("CTC heads").

    log_probs   encoder rows -> pm_ctc_head_bf16          projection + bias + log-softmax + arg-max in one pass
    decode      .. -> pm_ctc_greedy                        best path: repeats merged, blanks removed, first frame per token
    score       .. -> pm_ctc_forward_f32                   log p(target | clip), the alpha recursion in log space
    align       .. -> pm_ctc_viterbi_f32                   first / one-past-last frame of each target token on the best path

With ``lengths`` (samples per clip, as Wav2Vec2.forward takes them) the head and everything behind it run on the encoder's
PACKED rows (Wav2Vec2._packed_rows): no padded frame is ever projected.  A module and input that both live on the CPU take the
plain-torch forms of pytorch_models/_cpu.py.  Inference only.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import _cpu
from .._hip import ops
from ..transformer import Linear, _f32
from .wav2vec2 import Wav2Vec2


class Wav2Vec2CTC(nn.Module):
    """``encoder``: a Wav2Vec2, Data2VecAudio or SEW instance; ``lm_head``: Linear(d_model, vocab_size); ``blank``: the CTC
    blank id (Hugging Face's pad_token_id)."""

    frame_stride = 320  # samples per frame of the wav2vec2 / HuBERT stem: seconds = frame * frame_stride / sample_rate

    def __init__(self, encoder: Wav2Vec2, vocab_size: int, blank: int = 0) -> None:
        super().__init__()
        if not isinstance(encoder, Wav2Vec2):
            raise TypeError(f"Wav2Vec2CTC: the encoder must be a Wav2Vec2 / Data2VecAudio / SEW instance, got {type(encoder).__name__}")
        if not 2 <= vocab_size <= ops.CTC_MAX_VOCAB:
            raise ValueError(f"Wav2Vec2CTC: 2 <= vocab_size <= {ops.CTC_MAX_VOCAB}, got {vocab_size}")
        if not 0 <= blank < vocab_size:
            raise ValueError(f"Wav2Vec2CTC: blank must lie in [0, {vocab_size}), got {blank}")
        self.encoder = encoder
        self.lm_head = Linear(encoder.norm.normalized_shape[0], vocab_size)
        self.vocab_size, self.blank = vocab_size, blank

    # ---- encoder rows -> packed log-probabilities
    def _rows(self, x: Tensor, lengths):
        """(packed final hidden rows (sum frames, d), SeqLens of the frames)"""
        if x.dim() >= 1 and x.shape[0] == 0:  # (the CPU form has no empty batch either: it has no rows to concatenate)
            raise ValueError(f"Wav2Vec2CTC: an empty batch of clips is refused (got {tuple(x.shape)})")
        cpu = _cpu.on_cpu(x, self.lm_head.weight)
        if not cpu and self.lm_head.weight.dtype != torch.bfloat16:
            raise NotImplementedError(
                f"Wav2Vec2CTC: bf16 parameters only on a HIP device (got {self.lm_head.weight.dtype}); call model.to(torch.bfloat16)")
        if lengths is not None:
            return self.encoder._packed_rows(x, lengths)  # encoders without lengths= refuse here, as their forward does
        if cpu:  # the encoders' only CPU form is the lengths= one: every clip at its full length
            n = x.shape[-1]
            return self.encoder._packed_rows(x, [n] * x.shape[0])
        h = self.encoder(x)
        B, T, d = h.shape
        return h.reshape(B * T, d), self._full_seq(B, T, h.device)

    def _full_seq(self, B: int, T: int, device):
        """The extents of a batch whose clips all run to the last frame: built (one upload) at the first call of a geometry and
        KEPT per (B, T, device) - a captured forward holds the pointer of ``cu``, so a call at another geometry in between must
        not replace it, and a replay must not upload.  clear_derived drops the table."""
        cache = self.__dict__.setdefault("_pm_tables", {})
        key = (B, T, str(device))
        if key not in cache:
            cache[key] = ops.seq_lens([T] * B, T, device)
        return cache[key]

    def _head(self, x: Tensor, lengths):
        """(logp f32 (sum frames, V), best int32, best_logp f32, SeqLens)"""
        h, seq = self._rows(x, lengths)
        w, b = self.lm_head.weight, self.lm_head.bias
        if not h.is_cuda:
            return (*_cpu.ctc_head(h, w, b), seq)
        V = self.vocab_size
        out = None
        if V % 4 and seq.total != seq.B * seq.L:  # pm_rows_unpack moves 16-byte pieces: rows padded to a multiple of 4 floats
            out = torch.empty((h.shape[0], (V + 3) // 4 * 4), dtype=torch.float32, device=h.device)[:, :V]
        return (*ops.ctc_head(h, w, _f32(self.lm_head, "b", b), out=out), seq)

    @staticmethod
    def _unpack(logp: Tensor, seq) -> Tensor:
        V = logp.shape[1]
        if seq.total == seq.B * seq.L:
            return logp.view(seq.B, seq.L, V)
        if not logp.is_cuda:
            return _cpu.rows_unpack(logp, seq.lengths, seq.L)
        if logp.stride(0) != V:  # the padded rows of _head: unpack them whole; the copy drops the (never written) padding columns
            ld = logp.stride(0)
            return ops.rows_unpack(logp.as_strided((logp.shape[0], ld), (ld, 1)), seq)[..., :V].contiguous()
        return ops.rows_unpack(logp, seq)

    @torch.no_grad()
    def log_probs(self, x: Tensor, lengths=None) -> Tensor:
        """waveform (B, L) -> (B, T, V) fp32 log-probabilities; with ``lengths`` the frames past a clip's end are exactly 0."""
        logp, _, _, seq = self._head(x, lengths)
        return self._unpack(logp, seq)

    @torch.no_grad()
    def decode(self, x: Tensor, lengths=None):
        """Best-path decoding -> (ids int32 (B, T), n int32 (B), start int32 (B, T), path_logp f32 (B)): per clip the arg-max
        sequence with repeats merged and the blank removed (then -1), the number of tokens, the first frame of each token (then
        -1; seconds = start * frame_stride / sample_rate) and the log-probability of the arg-max path."""
        _, best, blp, seq = self._head(x, lengths)
        if not best.is_cuda:
            return _cpu.ctc_greedy(best, seq.lengths, seq.L, blp, self.blank)
        return ops.ctc_greedy(best, seq, blp, self.blank)

    def _targets(self, targets, target_lengths, B: int, device):
        """Host validation in front of every launch -> (targets int32 (B, max(target_lengths)) on ``device``, target_lengths
        list): columns no clip uses are trimmed before the launch (align pads its outputs back to the width passed in)."""
        ops.no_capture("Wav2Vec2CTC", "reads targets and target_lengths on the host")
        t = torch.as_tensor(targets)
        if t.dim() != 2 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"Wav2Vec2CTC: targets must be an integer (B, U) tensor, got {tuple(t.shape)} {t.dtype}")
        tl = [int(v) for v in (target_lengths.tolist() if isinstance(target_lengths, Tensor) else target_lengths)]
        if len(tl) != B or t.shape[0] != B:
            raise ValueError(f"Wav2Vec2CTC: {t.shape[0]} target rows and {len(tl)} target_lengths for a batch of {B}")
        Umax = t.shape[1]
        if any(not 0 <= v <= Umax for v in tl):
            raise ValueError(f"Wav2Vec2CTC: target_lengths must lie in [0, {Umax}], got {tl}")
        if max(tl, default=0) > ops.CTC_MAX_TARGET:
            raise ValueError(f"Wav2Vec2CTC: at most {ops.CTC_MAX_TARGET} labels per clip, got {max(tl)}")
        Umax = max(tl, default=0)
        th = t[:, :Umax].cpu().to(torch.int64)
        live = torch.arange(Umax)[None, :] < torch.tensor(tl, dtype=torch.int64)[:, None]
        bad = live & ((th < 0) | (th >= self.vocab_size) | (th == self.blank))
        if bool(bad.any()):
            raise ValueError(f"Wav2Vec2CTC: target id {int(th[bad][0])} is the blank ({self.blank}) or outside [0, {self.vocab_size})")
        return th.to(torch.int32).contiguous().to(device), tl

    @torch.no_grad()
    def score(self, x: Tensor, targets, target_lengths, lengths=None) -> Tensor:
        """(B) fp32 log p(targets[b, :target_lengths[b]] | clip b): the negative of ctc_loss(reduction="none"); -inf where the
        clip has too few frames for the target with its repeats."""
        t, tl = self._targets(targets, target_lengths, x.shape[0], x.device)
        logp, _, _, seq = self._head(x, lengths)
        if not logp.is_cuda:
            return _cpu.ctc_forward(logp, seq.lengths, t, tl, self.blank)
        return ops.ctc_forward(logp, seq, t, tl, self.blank)

    @torch.no_grad()
    def align(self, x: Tensor, targets, target_lengths, lengths=None):
        """Forced alignment -> (start int32 (B, U), stop int32 (B, U), score f32 (B)) in frames, U the width of ``targets`` as
        passed in (also where it exceeds max(target_lengths)): the first frame and one past the last frame of each target token
        on the best CTC path (-1 past target_lengths[b]) and that path's log-probability; -1 everywhere and -inf for an
        infeasible pair."""
        t, tl = self._targets(targets, target_lengths, x.shape[0], x.device)
        logp, _, _, seq = self._head(x, lengths)
        if not logp.is_cuda:
            start, stop, score = _cpu.ctc_viterbi(logp, seq.lengths, t, tl, self.blank)
        else:
            start, stop, score = ops.ctc_viterbi(logp, seq, t, tl, self.blank)
        U = torch.as_tensor(targets).shape[1] - t.shape[1]  # the columns _targets trimmed: no clip has a token there
        if U:
            start, stop = F.pad(start, (0, U), value=-1), F.pad(stop, (0, U), value=-1)
        return start, stop, score

    def forward(self, x: Tensor, lengths=None) -> Tensor:
        return self.log_probs(x, lengths)

    # ---- loading
    @classmethod
    def from_hf(cls, model_tag: str, *, config: dict | str | None = None, encoder_cls=Wav2Vec2, **kwargs):
        """A Hugging Face ``*ForCTC`` config (dict or path to a local config.json; no network in this build): the encoder through
        ``encoder_cls.from_hf``, ``vocab_size`` and ``pad_token_id`` (the blank) from the config."""
        import json

        if isinstance(config, str):
            with open(config) as f:
                config = json.load(f)
        encoder = encoder_cls.from_hf(model_tag, config=config, **kwargs)  # raises without a config
        return cls(encoder, int(config["vocab_size"]), int(config.get("pad_token_id", 0)))

    def load_hf_state_dict(self, state_dict: dict[str, Tensor]) -> None:
        """A Hugging Face ``Wav2Vec2ForCTC`` / ``HubertForCTC`` / ``Data2VecAudioForCTC`` / ``SEWForCTC`` state dict: the encoder keys
        under their model prefix, ``lm_head.weight``, ``lm_head.bias``.  Prints the keys it did not use, like the encoders."""
        from ..converters import load_hf_wav2vec2_ctc

        left = load_hf_wav2vec2_ctc(self, state_dict)
        print(dict.fromkeys(left).keys())
