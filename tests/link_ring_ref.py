"""The process links' FIFOs of the compiled-in simulator builds, restated in
Python (k_sim's links_append / links_pop, fantoch_amd/csrc/sim_wave.hip) beside
a plain model, one deque per link.

Link (p, q), p != q, is lane p (n - 1) + (q if q < p else q - 1).  Its lane
holds D entries (time, insertion seq, payload), oldest first, the kinds four
bits each in one word, and a count.  An entry past the count holds time NONE,
so the shift of a pop empties the head without a look at the count.  A send of
process p to the targets in `mask` appends in every target's link lane at that
lane's count, with insertion seq = seq + (targets below q): the numbers the
one-by-one loop over ascending targets hands out.  A link that holds D when it
is a target fails the whole send before anything is written.

With an overflow list (GeoCT::link_ovf, `pool` = R entries) a full lane's new
message goes to the link's list in the pool instead, the list's oldest message
refills the lane's last entry after a pop, and the send fails only where more
than R messages would be in flight on all links together: the pool builds'
capacity."""
from collections import deque

NONE = 0xFFFFFFFF


class Capacity(Exception):
    """A target link was full: the kernel's fail_cap (FX_ERR_SIM_CAPACITY)."""


def link_of(n, p, q):
    assert p != q
    return p * (n - 1) + (q if q < p else q - 1)


def ends_of(n, link):
    p, qi = divmod(link, n - 1)
    return p, (qi if qi < p else qi + 1)


class LaneRing:
    """The registers of the link lanes, entry 0 first (the kernel keeps entry
    0's time and seq in the link heads ht / hs)."""

    def __init__(self, n, depth, delay, pool=0):
        self.n, self.D = n, depth
        self.NP = n * (n - 1)
        # overflow lists (pool > 0): (time | kind << 28, seq, payload) per link
        self.pool, self.nfree = pool, pool
        self.lists = [deque() for _ in range(self.NP)]
        self.t = [[NONE] * depth for _ in range(self.NP)]
        self.s = [[NONE] * depth for _ in range(self.NP)]
        self.w = [[0] * depth for _ in range(self.NP)]
        self.kinds = [0] * self.NP
        self.count = [0] * self.NP
        # the lane's constants: sender, target, delay
        self.const = [ends_of(n, l) + (delay[ends_of(n, l)[0]][ends_of(n, l)[1]],) for l in range(self.NP)]
        self.seq = 0

    def append(self, now, p, mask, kind, w2):
        k = bin(mask).count("1")
        if k == 0:
            return
        target = [lp == p and (mask >> lq) & 1 == 1 for lp, lq, _ in self.const]
        if self.pool:
            if self.nfree < k:
                raise Capacity()
            self.nfree -= k
        elif any(tl and self.count[l] >= self.D for l, tl in enumerate(target)):
            raise Capacity()
        for l, tl in enumerate(target):  # every lane at once in the kernel
            if not tl:
                continue
            _, lq, d = self.const[l]
            c = self.count[l]
            if c >= self.D:  # a full lane: to the link's list (bit 31 of the kinds word)
                self.lists[l].append(((now + d) | (kind << 28), self.seq + bin(mask & ((1 << lq) - 1)).count("1"), w2))
                self.kinds[l] |= 1 << 31
                continue
            self.t[l][c] = now + d
            self.s[l][c] = self.seq + bin(mask & ((1 << lq) - 1)).count("1")
            self.w[l][c] = w2
            self.kinds[l] |= kind << (4 * c)
            self.count[l] = c + 1
        self.seq += k

    def head(self, l):
        return self.t[l][0], self.s[l][0]

    def pop(self, l):
        """(time, seq, kind, payload) of the oldest message of link l."""
        out = (self.t[l][0], self.s[l][0], self.kinds[l] & 15, self.w[l][0])
        self.t[l] = self.t[l][1:] + [NONE]
        self.s[l] = self.s[l][1:] + [NONE]
        self.w[l] = self.w[l][1:] + [self.w[l][-1]]
        more = self.kinds[l] >> 31
        self.kinds[l] = ((self.kinds[l] >> 4) & ((1 << 4 * (self.D - 1)) - 1)) | (self.kinds[l] & (1 << 31))
        self.count[l] -= 1
        if self.pool:
            self.nfree += 1
        if more:  # refill the last entry from the list
            w0, w1, w2 = self.lists[l].popleft()
            self.t[l][self.D - 1], self.s[l][self.D - 1], self.w[l][self.D - 1] = w0 & 0x0FFFFFFF, w1, w2
            self.kinds[l] |= (w0 >> 28) << 4 * (self.D - 1)
            if not self.lists[l]:
                self.kinds[l] &= 0x7FFFFFFF
            self.count[l] += 1
        return out

    def held(self, l):
        return self.count[l] + len(self.lists[l])


class DequeLinks:
    """The plain model: one deque per link, targets sent to one by one in
    ascending order, each taking the next insertion seq."""

    def __init__(self, n, depth, delay, pool=0):
        self.n, self.D, self.delay, self.pool = n, depth, delay, pool
        self.q = [deque() for _ in range(n * (n - 1))]
        self.seq = 0

    def append(self, now, p, mask, kind, w2):
        targets = [q for q in range(self.n) if (mask >> q) & 1]
        if self.pool:
            if sum(len(q) for q in self.q) + len(targets) > self.pool:
                raise Capacity()
        elif any(len(self.q[link_of(self.n, p, q)]) >= self.D for q in targets):
            raise Capacity()
        for q in targets:
            self.q[link_of(self.n, p, q)].append((now + self.delay[p][q], self.seq, kind, w2))
            self.seq += 1

    def head(self, l):
        return self.q[l][0][:2] if self.q[l] else (NONE, NONE)

    def pop(self, l):
        return self.q[l].popleft()
