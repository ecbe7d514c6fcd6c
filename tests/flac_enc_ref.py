"""The ONE restatement of the FLAC encoding rule of decode_batch_files(audio_format="flac") / save_audio("x.flac"), in numpy and Python
integers, written from the rule's statement and RFC 9639 — never from the C++. Tests of the device encoder, of the host twin and of the framing compare against
this file. Every decision is integer arithmetic, so equality is asked byte for byte.

Stream: mono, 16 bit, variable block size (blocking-strategy bit 1; the frame header codes the first sample's index). Every ROW is cut into blocks of 4096
samples plus one shorter last block. One subframe per frame, 8-bit subframe header, no wasted bits:
  CONSTANT  when all n samples are equal (n = 1 included);
  VERBATIM  otherwise when n <= 32;
  FIXED     otherwise orders o = 0..4 compete: residual r (int32), folded u = (r << 1) ^ (r >> 31); partitioned Rice method 0 (4-bit parameters, no escape),
            partition orders p = 0..pmax, pmax = the largest p <= 6 with n % 2^p == 0 and (n >> p) >= 32. A partition of cnt residuals costs
            4 + min over k = 0..14 of cnt (k + 1) + sum(u >> k), ties to the smaller k; partition 0 excludes the o warm-up samples.
            bits(o, p) = 8 + 16 o + 6 + sum of its partitions; the smallest wins, ties to the smaller o, then the smaller p;
  VERBATIM  instead when that is >= 8 + 16 n.
Frame: header (<= 14 bytes) + CRC-8, the subframe zero-padded to a byte, CRC-16. Block-size code 12 for 4096, otherwise 6 / 7 with the 8- / 16-bit (n - 1)
field; sample-rate code from the RFC's table (24 kHz = 7) or 0; channel code 0; sample-size code 4. STREAMINFO: min / max block size over the non-last blocks
(max = the largest block; a stream of one block: that block), min / max frame size, 36-bit total, MD5 all zero.
"""
import numpy as np

BLOCK = 4096
CONSTANT, VERBATIM, FIXED = 0, 1, 2
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}


class Bits:
    """MSB-first bit string as a Python integer."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, length):
        assert 0 <= value < (1 << length)
        self.v = (self.v << length) | value
        self.n += length

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def pmax_of(n):
    best = 0
    for p in range(7):
        if n % (1 << p) == 0 and (n >> p) >= 32:
            best = p
    return best


def residual(s, o):
    r = np.asarray(s, dtype=np.int64)
    for _ in range(o):
        r = np.concatenate([r[:1], np.diff(r)])     # (entries before index o are not residuals and are never read)
    return r


def fold(r):
    r = np.asarray(r, dtype=np.int64)
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def choose(s):
    """(kind, order, porder, [k per partition], bits) of one block of integer samples."""
    s = np.asarray(s, dtype=np.int64)
    n = len(s)
    if np.all(s == s[0]):
        return CONSTANT, 0, 0, [], 8 + 16
    if n <= 32:
        return VERBATIM, 0, 0, [], 8 + 16 * n
    best = None
    for o in range(5):
        u = fold(residual(s, o))
        shifted = np.stack([u >> k for k in range(15)])            # [15, n]
        for p in range(pmax_of(n) + 1):
            length = n >> p
            bits, ks = 8 + 16 * o + 6, []
            for j in range(1 << p):
                a = max(j * length, o) if j == 0 else j * length
                cnt = (j + 1) * length - a
                costs = cnt * np.arange(1, 16) + shifted[:, a:(j + 1) * length].sum(axis=1)
                k = int(np.argmin(costs))                           # the first minimum: ties to the smaller k
                ks.append(k)
                bits += 4 + int(costs[k])
            if best is None or bits < best[4]:                       # o ascending, p ascending: strict < keeps the smaller o, then the smaller p
                best = (FIXED, o, p, ks, bits)
    if best[4] >= 8 + 16 * n:
        return VERBATIM, 0, 0, [], 8 + 16 * n
    return best


def subframe(s):
    """(bytes, kind, order, porder, ks) of one block."""
    s = np.asarray(s, dtype=np.int64)
    n = len(s)
    kind, o, p, ks, bits = choose(s)
    b = Bits()
    if kind == CONSTANT:
        b.put(0b00000000, 8)
        b.put(int(s[0]) & 0xffff, 16)
    elif kind == VERBATIM:
        b.put(0b00000010, 8)
        for x in s:
            b.put(int(x) & 0xffff, 16)
    else:
        b.put((0b001000 | o) << 1, 8)
        for x in s[:o]:
            b.put(int(x) & 0xffff, 16)
        b.put(0, 2)
        b.put(p, 4)
        u = fold(residual(s, o))
        length = n >> p
        for j in range(1 << p):
            k = ks[j]
            b.put(k, 4)
            for i in range(max(j * length, o) if j == 0 else j * length, (j + 1) * length):
                q = int(u[i]) >> k
                if q:
                    b.put(0, q)
                b.put(1, 1)
                if k:
                    b.put(int(u[i]) & ((1 << k) - 1), k)
    assert b.n == bits, (b.n, bits)
    return b.bytes(), kind, o, p, ks


def crc8(data):
    c = 0
    for x in data:
        c ^= x
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xff if c & 0x80 else (c << 1) & 0xff
    return c


def crc16(data):
    c = 0
    for x in data:
        c ^= x << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xffff if c & 0x8000 else (c << 1) & 0xffff
    return c


def coded_number(v):
    assert 0 <= v < (1 << 36)
    if v < 0x80:
        return bytes([v])
    for nbytes, limit in ((2, 1 << 11), (3, 1 << 16), (4, 1 << 21), (5, 1 << 26), (6, 1 << 31), (7, 1 << 36)):
        if v < limit:
            lead = (0xff << (8 - nbytes)) & 0xff
            out = [lead | (v >> (6 * (nbytes - 1)))] if nbytes < 7 else [0xfe]
            out += [0x80 | ((v >> (6 * i)) & 0x3f) for i in range(nbytes - 2, -1, -1)]
            return bytes(out)


def frame(sub, n, first_sample, sample_rate):
    bs = 12 if n == 4096 else (6 if n <= 256 else 7)
    h = bytes([0xff, 0xf9, (bs << 4) | RATE_CODES.get(sample_rate, 0), (0 << 4) | (4 << 1)]) + coded_number(first_sample)
    if bs == 6:
        h += bytes([n - 1])
    elif bs == 7:
        h += (n - 1).to_bytes(2, "big")
    h += bytes([crc8(h)])
    body = h + sub
    return body + crc16(body).to_bytes(2, "big")


def blocks_of(n):
    return [(a, min(BLOCK, n - a)) for a in range(0, n, BLOCK)]


def streaminfo(sample_rate, sizes, frame_sizes, total):
    non_last = sizes[:-1] if len(sizes) > 1 else sizes
    b = Bits()
    b.put(min(non_last) if sizes else 0, 16)
    b.put(max(sizes) if sizes else 0, 16)
    b.put(min(frame_sizes) if sizes else 0, 24)
    b.put(max(frame_sizes) if sizes else 0, 24)
    b.put(sample_rate, 20)
    b.put(0, 3)
    b.put(15, 5)
    b.put(total, 36)
    b.put(0, 128)
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + b.bytes()


def encode_rows(rows, sample_rate=24000):
    """The whole file of a list of rows (each an integer array): bytes, plus per block (row, first, n, kind, order, porder, ks, subframe bytes)."""
    frames, info, sizes, pos = [], [], [], 0
    for r, s in enumerate(rows):
        s = np.asarray(s, dtype=np.int64)
        for a, n in blocks_of(len(s)):
            sub, kind, o, p, ks = subframe(s[a:a + n])
            frames.append(frame(sub, n, pos + a, sample_rate))
            info.append((r, a, n, kind, o, p, ks, sub))
            sizes.append(n)
        pos += len(s)
    return streaminfo(sample_rate, sizes, [len(f) for f in frames], pos) + b"".join(frames), info


# ---- the test inputs: integer samples q with |q| <= 32440, so that the float q / 32768 quantises back to q ------------------------------------------------------
SIGNALS = ("silence", "beyond_limit", "uniform_full", "alternating", "spike", "uniform_pm3", "sine_a4096", "sine_a256", "sine_a16", "sine_a0")
LENGTHS = (1, 5, 32, 33, 64, 1408, 2240, 4095, 4096, 4097, 4160, 9600)


def signal(name, n):
    rng = np.random.default_rng(sum(name.encode()) * 100003 + n)
    if name == "silence":
        return np.zeros(n, dtype=np.int64)
    if name == "beyond_limit":                       # a waveform beyond +limit throughout: every sample clamps to 32440
        return np.full(n, 32440, dtype=np.int64)
    if name == "uniform_full":
        return rng.integers(-32440, 32441, size=n)
    if name == "alternating":                        # the largest order-4 residual
        return np.where(np.arange(n) % 2 == 0, 32440, -32440).astype(np.int64)
    if name == "spike":
        q = np.zeros(n, dtype=np.int64)
        q[n // 2] = 30000
        return q
    if name == "uniform_pm3":
        return rng.integers(-3, 4, size=n)
    a = int(name.split("_a")[1])
    tone = np.round(12000.0 * np.sin(2.0 * np.pi * 440.0 * np.arange(n) / 24000.0)).astype(np.int64)
    return tone + (rng.integers(-a, a + 1, size=n) if a else 0)


def bursts(n, seed):
    """Not one of SIGNALS: a tone under noise whose amplitude changes every 64 samples (0, 8, 300 or 5000), so that the partitions of one block want
    different Rice parameters and a high partition order wins."""
    rng = np.random.default_rng(seed)
    amp = np.repeat(np.array([0, 8, 300, 5000])[rng.integers(0, 4, size=n // 64 + 1)], 64)[:n]
    return signal("sine_a0", n) + np.round(rng.uniform(-1.0, 1.0, size=n) * amp).astype(np.int64)


def as_float(q):
    return (np.asarray(q, dtype=np.float64) / 32768.0).astype(np.float32)
