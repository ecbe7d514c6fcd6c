"""CPU twin of the sampler's truncation (audiotoken_amd/csrc/gpt_model.hip): the top-k of §17, then ``min_p`` and the nucleus, stated in
float64 on the fp32 tempered values. ``truncate`` gives the final set, ``draw`` is steps 4 and 5 of §17 on a set given by its threshold, ``sample`` both."""
import numpy as np

# |G(x) / S_K - top_p| below this and the device's comparison may fall on either side (DESIGN.md §24 derives it): a 2-ulp expf on both sums,
# 2 (2^-22), the floors of up to 65536 integer masses on both, 2 (65536 2^-40), and the rest (the ceiling of the cut, one double product) rounded up.
NUCLEUS_WINDOW = 2.0 ** -21 + 2.0 ** -22


def draw_window(kept):
    """§17's window on the distance of a draw from a CDF boundary: ``kept`` sequential fp32 additions and a 2-ulp expf, on both sides."""
    return 2.0 * (kept * 2.0 ** -24 + 2.0 ** -22)


def tempered(logits_f32, temperature, allow=None):
    """Steps 1 and 2: one fp32 division, then -inf outside the allow ranges ``(lo0, hi0, lo1, hi1)``."""
    z = np.asarray(logits_f32, dtype=np.float32)
    zt = (z / np.float32(temperature)).astype(np.float32)
    if allow is not None:
        ids = np.arange(z.shape[0])
        ok = ((ids >= allow[0]) & (ids < allow[1])) | ((ids >= allow[2]) & (ids < allow[3]))
        zt = np.where(ok, zt, np.float32(-np.inf)).astype(np.float32)
    return zt


def log_min_p(min_p):
    """``lmin``: the logarithm of the fp32 ``min_p`` in float64, rounded to fp32 once."""
    return np.float32(np.log(np.float64(np.float32(min_p))))


def truncate(logits_f32, temperature, top_k, top_p=None, min_p=None, allow=None):
    """Steps 1 to 3b: ``(zt, thresh, kept, margin, k_size)``. ``thresh`` is the lowest tempered value that stays (fp32), ``kept`` the number of ids with
    ``zt >= thresh``, ``margin`` the smallest ``|G(x) / S_K - top_p|`` over the distinct values of the top-k set K (inf with the nucleus off), ``k_size``
    the size of K."""
    zt = tempered(logits_f32, temperature, allow)
    V = zt.shape[0]
    k = min(int(top_k), V)
    v_k = np.partition(zt, V - k)[V - k]
    zk = zt[zt >= v_k]                                   # K, ties at the threshold included
    m = zk.max()
    d = (zk - m).astype(np.float32)                      # one fp32 subtraction, as the device makes it
    keep = np.ones(zk.shape[0], dtype=bool)
    if min_p is not None and float(min_p) > 0.0:
        keep &= d >= log_min_p(min_p)
    margin = float("inf")
    if top_p is not None and np.float32(top_p) < np.float32(1.0):
        p = np.exp(d.astype(np.float64))
        vals, inv = np.unique(zk, return_inverse=True)  # the distinct values, ascending
        mass = np.bincount(inv.reshape(-1), weights=p, minlength=vals.shape[0])
        S = mass.sum()
        above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])   # G(x): the mass strictly above each distinct value
        tp = np.float64(np.float32(top_p))
        keep &= (above < tp * S)[inv.reshape(-1)]
        margin = float(np.abs(above / S - tp).min())
    thresh = np.float32(zk[keep].min())
    return zt, thresh, int((zt >= thresh).sum()), margin, int(zk.shape[0])


def draw(zt, thresh, u):
    """Steps 4 and 5 of §17 on the ids with ``zt >= thresh``: ``(token, dist, kept)``, ``dist`` the distance from ``u`` to the nearest boundary between two
    kept ids in the set's normalised CDF."""
    kept = np.nonzero(zt >= np.float32(thresh))[0]
    z64 = zt[kept].astype(np.float64)
    p = np.exp(z64 - z64.max())
    cdf = np.cumsum(p)
    S = cdf[-1]
    u64 = np.float64(np.float32(u))
    over = np.nonzero(cdf > u64 * S)[0]
    token = int(kept[over[0]]) if over.size else int(kept[z64 > -np.inf][-1])
    dist = float(np.abs(cdf[:-1] / S - u64).min()) if kept.size > 1 else float("inf")
    return token, dist, int(kept.size)


def sample(logits_f32, temperature, top_k, u, top_p=None, min_p=None, allow=None):
    """The whole rule on one fp32 logit vector: ``(token, kept, thresh, margin)``."""
    zt, thresh, kept, margin, _ = truncate(logits_f32, temperature, top_k, top_p, min_p, allow)
    token, _, n = draw(zt, thresh, u)
    assert n == kept
    return token, kept, thresh, margin
