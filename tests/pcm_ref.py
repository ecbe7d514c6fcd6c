"""The ONE restatement of the float -> 16-bit PCM rule of decode_batch_files / save_audio, in numpy, every operation in float32 and in the
order the rule is stated. Tests of the device writer, of ``save_audio`` and of the file pipeline compare against this file, never against product code.

For every sample x, in order:
  1. a NaN becomes 0 and is counted as non-finite;
  2. +-infinity goes to +-limit and is counted as non-finite;
  3. otherwise y = x * scale (float32), clamped to [-limit, +limit]; a sample the clamp changed is counted as clipped;
  4. q = rint(y * 32768): round half to even; stored as int16. limit = 0.99, so |q| <= 32440.
The file scale of rescale=True is min(0.99 / peak, 1) in float32, peak = max |x| over the finite samples.
"""
import numpy as np

LIMIT = np.float32(0.99)
F32 = np.float32


def peak(x) -> np.float32:
    x = np.asarray(x, dtype=np.float32).ravel()
    best = F32(0.0)
    finite = x[np.isfinite(x)]
    if finite.size:
        best = F32(np.max(np.abs(finite)))
    return best


def file_scale(p) -> np.float32:
    p = F32(p)
    if p == 0:
        return F32(1.0)
    s = LIMIT / p                       # float32 / float32
    return s if s < F32(1.0) else F32(1.0)


def quantise(x, scale=1.0, limit=LIMIT):
    """(int16 array, clipped count, non-finite count)."""
    x = np.asarray(x, dtype=np.float32).ravel()
    scale, limit = F32(scale), F32(limit)
    q = np.zeros(x.shape, dtype=np.int16)
    is_nan = np.isnan(x)
    is_inf = np.isinf(x)
    fin = ~(is_nan | is_inf)
    # 1. NaN -> 0 (q is already 0)
    # 2. +-inf -> +-limit
    y_inf = np.where(x[is_inf] > 0, limit, -limit).astype(np.float32)
    q[is_inf] = np.rint(y_inf * F32(32768.0)).astype(np.int16)
    # 3. finite: scale, clamp
    with np.errstate(over="ignore"):
        y = (x[fin] * scale).astype(np.float32)
    c = np.clip(y, -limit, limit).astype(np.float32)
    clipped = int(np.sum(c != y))
    # 4. round half to even
    q[fin] = np.rint(c * F32(32768.0)).astype(np.int16)
    return q, clipped, int(np.sum(~fin))
