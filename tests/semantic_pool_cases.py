"""What the CPU and the GPU tests of the stream pools share: fixed-seed interleavings of opens, pushes and flushes, the calls they make
of a pool, and a brute-force statement of the rule of one call, written without ``pool_schedule``."""
import numpy as np

CHECK_EVERY = 16


def interleaving(lens, seed, most=6, late=(), width=(3, 8)):
    """A fixed-seed schedule for sources of ``lens`` ids: a list of calls ``{"open": [i], "push": {i: n}, "flush": [i]}``. Every call names a random
    subset of the open, unfinished streams; each pushes 1 to ``most`` ids (or nothing, when all its ids are in) and a stream whose ids are all in is
    flushed in that call or in a later one. The streams in ``late`` are opened only after some other stream was flushed."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    left, opened, flushed = list(lens), set(), set()
    calls = []
    while len(flushed) < n:
        call = {"open": [], "push": {}, "flush": []}
        for i in range(n):
            if i not in opened and (i not in late or flushed):
                opened.add(i)
                call["open"].append(i)
        live = [i for i in sorted(opened) if i not in flushed]
        k = min(len(live), int(rng.integers(width[0], width[1] + 1)))
        for i in sorted(rng.choice(live, size=k, replace=False).tolist()):
            m = min(left[i], int(rng.integers(1, most + 1)))
            if m:
                call["push"][i] = m
                left[i] -= m
            if left[i] == 0 and (m == 0 or rng.random() < 0.5):
                call["flush"].append(i)
                flushed.add(i)
        calls.append(call)
    assert all(x == 0 for x in left)
    return calls


def call_streams(calls, n):
    """Per call the pool's view of it: ``[(i, ids before, ids pushed, flushed)]`` in ascending i for every stream the call names."""
    had = [0] * n
    out = []
    for c in calls:
        named = sorted(set(c["push"]) | set(c["flush"]))
        out.append([(i, had[i], c["push"].get(i, 0), i in c["flush"]) for i in named])
        for i, m in c["push"].items():
            had[i] += m
    return out


def pushes_of(calls, i):
    """The ids stream i pushed call by call, from its first push to its flush (a flush-only call counts as a push of 0)."""
    out = []
    for c in calls:
        if i in c["push"] or i in c["flush"]:
            out.append(c["push"].get(i, 0))
        if i in c["flush"]:
            break
    return out


# ---- the rule of one call, by brute force -------------------------------------------------------------------------------------------------------------
class _Stream:
    """One stream of a call as §25 states it: a ring of at most 2 S ids, a window k that runs once one id past it exists, the final one at the flush."""

    def __init__(self, before, new, final, S, H, r, block, max_new):
        self.S, self.H, self.r, self.block, self.max_new = S, H, r, block, max_new
        self.k = 0
        while before > self.k * H + S:
            self.k += 1
        self.ring = before - self.k * H          # ids held: from id k H of the source on
        self.left, self.final, self.total = new, final, before
        self.ended = False

    def round(self):
        """The windows of the stream's next round as ``[(k, final, prompt tokens, steps)]``, or None when it has no round left."""
        if self.ended:
            return None
        S, H, r = self.S, self.H, self.r
        take = min(self.left, 2 * S - self.ring)
        self.ring += take
        self.left -= take
        self.total += take
        assert self.ring <= 2 * S, "no ring exceeds 2 S"
        wins = []
        while self.total > self.k * H + S:
            carry = r * (S - H) if self.k else 0
            wins.append((self.k, False, S + 1 + carry, r * S - carry))
            self.k += 1
            self.ring -= H
        if self.left == 0:
            self.ended = True
            if self.final:
                carry = r * (S - H) if self.k else 0
                P = self.total - self.k * H + 1 + carry
                wins.append((self.k, True, P, min(self.max_new, self.block - P)))
        return wins if take or wins else None


def brute_call(streams, S, H, r, block, max_new, slots, tick_tokens, final_steps=None):
    """``streams``: ``[(ids before, ids pushed, flushed)]`` in ascending id. Returns ``(ticks, windows)``: per tick ``(round, [(slot, stream, k, final,
    tokens)])`` with ``tokens`` 1 for a step and the prompt's length for a start, and per stream the windows it ran, ``[(k, final)]``. Independent §25
    streams, merged tick by tick by §20's rule."""
    ss = [_Stream(b, m, f, S, H, r, block, max_new) for b, m, f in streams]
    ticks, ran = [], [[] for _ in ss]
    g = 0
    while True:
        chains = [s.round() for s in ss]
        if all(c is None for c in chains):
            break
        queue = [i for i, c in enumerate(chains) if c]
        row = {}                                 # slot -> [stream, windows left of its chain, steps left of the running window or None, final, ends early after]
        while queue or row:
            for j in range(slots):
                if j not in row and queue:
                    i = queue.pop(0)
                    row[j] = [i, list(chains[i]), None, False, None]
            tick, used = [], sum(1 for x in row.values() if x[2] is not None)
            for j in sorted(row):
                x = row[j]
                if x[2] is not None:
                    tick.append((j, x[0], x[5], x[3], 1))
            blocked = False
            for j in sorted(row):
                x = row[j]
                if x[2] is None and not blocked:
                    k, final, P, steps = x[1][0]
                    if used + P > tick_tokens:
                        blocked = True
                        continue
                    used += P
                    x[1].pop(0)
                    early = steps if not final or final_steps is None else min(steps, int(final_steps[x[0]]))
                    x[2:] = [steps, final, early, k, 0]
                    ran[x[0]].append((k, final))
                    tick.append((j, x[0], k, final, P))
            assert tick and used <= tick_tokens, "no tick is empty or over tick_tokens"
            ticks.append((g, tick))
            in_final = False
            for j, *_ in tick:
                x = row[j]
                x[2] -= 1
                x[6] += 1
                if x[2] > 0:
                    in_final = in_final or x[3]
                    continue
                x[2] = None
                if not x[1]:
                    del row[j]
            if in_final and len(ticks) % CHECK_EVERY == 0:
                for j in list(row):
                    x = row[j]
                    if x[2] is not None and x[3] and x[6] >= x[4]:
                        del row[j]
        g += 1
    return ticks, ran
