"""Voice prompts: a few seconds of a speaker, as semantic ids and the EnCodec codes of the same stretch of audio, that the sources of a
call continue. ``P`` semantic ids go with ``3 P / 2`` frames (``ids_per_source_token = 3`` coarse ids per semantic id, two per frame), so ``P`` is even.
Rows 0 and 1 of the codes are the GPT stage's first carry (``SemanticToAcoustic.to_acoustic_long(voice=)``); all 8 rows are the fine stage's history
(``to_fine(history=)``)."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

CODEBOOK_SIZE = 1024


def _int_array(x, what: str) -> np.ndarray:
    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
    if a.dtype.kind not in "iu":
        raise ValueError(f"VoicePrompt: {what} must be integers, got {a.dtype}")
    return a.astype(np.int64)


class VoicePrompt:
    """``semantic``: int64 ``[P]``; ``codes``: int64 ``[8, 3P/2]``, or ``[2, 3P/2]`` when only the GPT stage will use it. Refused: an odd or empty ``P``,
    a frame count other than ``3P/2``, a negative id (or one at or above ``semantic_vocab``, where given), a code outside ``[0, 1024)``."""

    def __init__(self, semantic, codes, semantic_vocab: Optional[int] = None):
        sem = _int_array(semantic, "the semantic ids").reshape(-1)
        c = _int_array(codes, "the codes")
        P = int(sem.size)
        if P < 2 or P % 2:
            raise ValueError(f"VoicePrompt: the number of semantic ids must be even, at least 2, got {P}")
        if c.ndim != 2 or c.shape[0] not in (2, 8):
            raise ValueError(f"VoicePrompt: codes must be [8, F] or [2, F], got {tuple(c.shape)}")
        if c.shape[1] != 3 * P // 2:
            raise ValueError(f"VoicePrompt: {P} semantic ids go with {3 * P // 2} frames of codes, got {c.shape[1]}")
        if sem.min() < 0 or (semantic_vocab is not None and sem.max() >= semantic_vocab):
            raise ValueError("VoicePrompt: a semantic id lies outside the vocabulary")
        if c.min() < 0 or c.max() >= CODEBOOK_SIZE:
            raise ValueError(f"VoicePrompt: codes must lie in [0, {CODEBOOK_SIZE})")
        self.semantic = torch.from_numpy(sem)
        self.codes = torch.from_numpy(np.ascontiguousarray(c))

    def __len__(self) -> int:
        return int(self.semantic.numel())

    @property
    def frames(self) -> int:
        return int(self.codes.shape[1])

    @staticmethod
    def aligned_stretch(n_ids: int, frames: int, max_ids: int):
        """``(a, P)``: the latest aligned stretch of a clip of ``n_ids`` semantic ids and ``frames`` frames. ``P`` is the largest even number
        ``<= min(max_ids, n_ids, floor(2 frames / 3))``; ``a`` is the even id that makes ids ``[a, a + P)`` and frames ``[3a/2, 3a/2 + 3P/2)`` end as late as
        both arrays allow."""
        usable = min(int(n_ids), 2 * int(frames) // 3)
        P = min(int(max_ids), usable) // 2 * 2
        if P < 2:
            raise ValueError(f"VoicePrompt.from_tokens: {n_ids} ids and {frames} frames with max_ids = {max_ids} leave no aligned pair of ids")
        return (usable - P) // 2 * 2, P

    @classmethod
    def from_tokens(cls, sem_ids, codes, max_ids: int, semantic_vocab: Optional[int] = None) -> "VoicePrompt":
        """Cuts the latest aligned stretch (``aligned_stretch``) out of a clip's tokens: ``sem_ids`` any shape, flattened; ``codes`` ``[8, F]``, ``[2, F]``
        or with a leading batch dimension of 1."""
        sem = _int_array(sem_ids, "the semantic ids").reshape(-1)
        c = _int_array(codes, "the codes")
        if c.ndim == 3 and c.shape[0] == 1:
            c = c[0]
        if c.ndim != 2:
            raise ValueError(f"VoicePrompt.from_tokens: codes must be [K, F], got {tuple(c.shape)}")
        a, P = cls.aligned_stretch(sem.size, c.shape[1], max_ids)
        return cls(sem[a:a + P], c[:, 3 * a // 2:3 * a // 2 + 3 * P // 2], semantic_vocab)


def per_row(voice, n: int, what: str = "voice") -> List[Optional[VoicePrompt]]:
    """``voice`` as one entry per row: None, one object shared by all rows, or a list with one entry (or None) per row."""
    if voice is None or isinstance(voice, VoicePrompt):
        return [voice] * n
    if not isinstance(voice, (list, tuple)) or len(voice) != n or any(v is not None and not isinstance(v, VoicePrompt) for v in voice):
        raise ValueError(f"{what} must be None, a VoicePrompt, or a list of {n} of them (None where a row has none)")
    return list(voice)


def voice_table(voice, n: int, semantic_vocab: int, codebook_size: int, r: int):
    """The prompt table of a GPT call, or None when no row has a prompt: ``(sem int32 [n_p, p_stride], codes int32 [n_p, 2, f_stride], lengths, entry of
    each row or -1)``. Rows that share one object share one entry."""
    rows = per_row(voice, n)
    if all(v is None for v in rows):
        return None
    if r != 3:
        raise ValueError(f"voice prompts pair 3 coarse ids with a semantic id, the model's config has {r}")
    entries, index, of_row = [], {}, []
    for v in rows:
        if v is None:
            of_row.append(-1)
            continue
        if id(v) not in index:
            if int(v.semantic.max()) >= semantic_vocab or int(v.codes[:2].max()) >= codebook_size:
                raise ValueError("voice prompt: an id lies outside the model's semantic vocabulary or code books")
            index[id(v)] = len(entries)
            entries.append(v)
        of_row.append(index[id(v)])
    p_stride, f_stride = max(len(v) for v in entries), max(v.frames for v in entries)
    sem = np.zeros((len(entries), p_stride), dtype=np.int32)
    codes = np.zeros((len(entries), 2, f_stride), dtype=np.int32)
    for e, v in enumerate(entries):
        sem[e, :len(v)] = v.semantic.numpy()
        codes[e, :, :v.frames] = v.codes[:2].numpy()
    return sem, codes, [len(v) for v in entries], of_row
