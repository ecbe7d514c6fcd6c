"""Shared by tests/test_resample_stream_cpu.py and tests/test_resample_stream_gpu.py: the signals, rates and push schedules of the streaming resampler's
tests (not a test module)."""
import functools

import numpy as np

from audiotoken_amd import resample_stream as RS

MODEL_RATE = 24000
RATES = [44100, 48000, 22050, 16000, 8000, 24000]


def signal_length(rate: int) -> int:
    """2.3 s + 13 samples: three 1 s chunks, two seams, a ragged end."""
    return int(2.3 * rate) + 13


@functools.lru_cache(maxsize=None)
def signal(rate: int, seed: int = 0) -> np.ndarray:
    """Seeded tone plus noise, float32 in [-1, 1)."""
    L = signal_length(rate)
    rng = np.random.default_rng(1000 * seed + rate)
    t = np.arange(L, dtype=np.float64) / rate
    x = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t + 0.7) + 0.3 * rng.uniform(-1.0, 1.0, L)
    x = np.clip(x, -1.0, 1.0 - 2.0 ** -15).astype(np.float32)
    x.setflags(write=False)
    return x


def as_format(x: np.ndarray, fmt: str):
    """The float signal quantised into a storage format: ``(array, AT_PCM_* code, scale)``."""
    from audiotoken_amd import _cabi
    if fmt == "s16":
        return np.round(x * 32767.0).astype(np.int16), _cabi.PCM_S16, 1.0 / 32768.0
    if fmt == "s32":
        return np.round(x.astype(np.float64) * (2 ** 31 - 1)).astype(np.int32), _cabi.PCM_S32, 1.0 / 2147483648.0
    if fmt == "u8":
        return (np.round(x * 127.0) + 128).astype(np.uint8), _cabi.PCM_U8, 1.0 / 128.0
    assert fmt == "f32"
    return x.copy(), _cabi.PCM_F32, 1.0


def push_sizes(rate: int, L: int, seed: int = 0):
    """Push sizes that sum to L: 1 sample, width - 1, o, o + 1, 4096 and a random remainder, over and over until the signal is used up."""
    o, n, width = RS.ratio(rate, MODEL_RATE)
    rng = np.random.default_rng(seed + rate)
    sizes, left = [], L
    while left > 0:
        for s in (1, max(width - 1, 0), o, o + 1, 4096, int(rng.integers(1, 9000))):
            s = min(s, left)
            sizes.append(s)
            left -= s
            if left == 0:
                break
    return sizes


def plans(rate: int, sizes, flush_empty: bool):
    """The planner run over a schedule: ``[(first new sample, PushPlan)]``; the last push is final, or (``flush_empty``) a final push of nothing follows."""
    pos = RS.StreamPosition(*RS.ratio(rate, MODEL_RATE))
    steps = [(s, False) for s in sizes]
    if flush_empty:
        steps.append((0, True))
    else:
        steps[-1] = (steps[-1][0], True)
    out, start = [], 0
    for s, final in steps:
        plan = RS.plan_push(pos, s, final)
        out.append((start, plan, pos.tail_len))
        RS.commit(pos, plan)
        start += s
    return out
