"""The reduced audio context, restated on the oracle (oracle/whisper_ref.py WhisperRef): what ccx_whisper_encode_ctx is defined to
compute (include/ccx.h).  Built from the oracle's own _attn / _mlp / _ln, so that n = n_audio_ctx IS WhisperRef.encode, op for op.

Definition: the conv stem runs on the usual 3000-frame log-mel; positions [0, n) are kept, with rows [0, n) of the positional
embedding; every encoder layer attends over those positions only; then ln_post."""
from typing import List, Sequence, Union

import torch
import torch.nn.functional as F


def _stem(ref, mel: torch.Tensor) -> torch.Tensor:
    mel = mel.to(ref.dtype)
    x = F.gelu(F.conv1d(mel, ref.sd["encoder.conv1.weight"], ref.sd["encoder.conv1.bias"], padding=1))
    x = F.gelu(F.conv1d(x, ref.sd["encoder.conv2.weight"], ref.sd["encoder.conv2.bias"], stride=2, padding=1))
    return x.permute(0, 2, 1)


def _layers(ref, x: torch.Tensor, mask=None) -> torch.Tensor:
    d = ref.dims
    for l in range(d.n_audio_layer):
        p = f"encoder.blocks.{l}"
        x = x + ref._attn(ref._ln(x, p + ".attn_ln"), p + ".attn", d.n_audio_head, mask=mask)
        x = x + ref._mlp(ref._ln(x, p + ".mlp_ln"), p)
    return ref._ln(x, "encoder.ln_post")


def encode_ctx(ref, mel: torch.Tensor, n: Union[int, Sequence[int]]) -> Union[torch.Tensor, List[torch.Tensor]]:
    """mel [B, n_mels, 3000].  n an int: [B, n, D], every window at n positions.  n a sequence of B ints: a list of [n[b], D], every
    window truncated on its own (the definition)."""
    if isinstance(n, int):
        x = _stem(ref, mel)
        return _layers(ref, x[:, :n] + ref.sd["encoder.positional_embedding"][:n])
    assert len(n) == mel.shape[0]
    return [encode_ctx(ref, mel[b:b + 1], int(k))[0] for b, k in enumerate(n)]


def encode_ctx_masked(ref, mel: torch.Tensor, n: Sequence[int]) -> List[torch.Tensor]:
    """The same as ONE batch at max(n) rows per window, the way the library runs it: keys at or beyond n[b] masked out of window b's
    attention, its rows at or beyond n[b] computed and dropped.  -> list of [n[b], D]."""
    B, S = mel.shape[0], max(int(k) for k in n)
    assert S >= B, "the oracle slices its mask [:T, :T]: a [B, 1, S, S] mask survives that only while B <= S"
    x = _stem(ref, mel)[:, :S] + ref.sd["encoder.positional_embedding"][:S]
    mask = torch.zeros(B, 1, S, S, dtype=ref.dtype)
    for b, k in enumerate(n):
        mask[b, :, :, int(k):] = float("-inf")
    out = _layers(ref, x, mask=mask)
    return [out[b, :int(k)] for b, k in enumerate(n)]


def padded_xa(rows: List[torch.Tensor], n_audio_ctx: int) -> torch.Tensor:
    """[B, n_audio_ctx, D] with every window's valid rows in front and zeros behind (only the valid rows may ever be read)"""
    out = torch.zeros(len(rows), n_audio_ctx, rows[0].shape[-1], dtype=rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out
