"""The slot allocator's rules (include/rtlfm_slots.h) in plain Python integers - what csrc/slots.cpp is compared with.

Per source and step: frames == 0 freezes the source; a bound slot whose bin is below close_level (power < close * frames)
counts a quiet run, any other bound slot resets its count; a count above `hang` frees the slot; the bins that are not
masked, not bound and at or above open_level (power >= open * frames), by power descending and ties to the lower bin,
fill the idle slots in ascending slot order; a bound slot is never moved.  An idle slot is None here, -1 in an event and
`park` in bins().
"""


class SlotsModel:
    def __init__(self, nsources, K, slots, open_level, close_level, hang=0, park=0, mask=None):
        assert close_level <= open_level and hang >= 0 and 0 <= park < K
        self.nsources, self.K, self.slots = nsources, K, slots
        self.open, self.close, self.hang, self.park = int(open_level), int(close_level), int(hang), int(park)
        self.mask = [bool(m) for m in mask] if mask is not None else [False] * K
        self.bin = [[None] * slots for _ in range(nsources)]
        self.quiet = [[0] * slots for _ in range(nsources)]
        self.events = []

    def step(self, power, frames):
        self.events = []
        for a in range(self.nsources):
            fr = int(frames[a])
            if fr == 0:
                continue
            pw = [int(v) for v in power[a]]
            before = list(self.bin[a])
            for s in range(self.slots):
                b = self.bin[a][s]
                if b is None:
                    continue
                self.quiet[a][s] = self.quiet[a][s] + 1 if pw[b] < self.close * fr else 0
                if self.quiet[a][s] > self.hang:
                    self.bin[a][s] = None
                    self.quiet[a][s] = 0
            bound = {b for b in self.bin[a] if b is not None}
            cand = [k for k in range(self.K) if not self.mask[k] and k not in bound and pw[k] >= self.open * fr]
            cand.sort(key=lambda k: (-pw[k], k))
            for s in range(self.slots):
                if self.bin[a][s] is None and cand:
                    self.bin[a][s] = cand.pop(0)
                    self.quiet[a][s] = 0
            for s in range(self.slots):
                if self.bin[a][s] != before[s]:
                    self.events.append(dict(source=a, slot=s, old_bin=-1 if before[s] is None else before[s],
                                            new_bin=-1 if self.bin[a][s] is None else self.bin[a][s]))

    def bins(self):
        return [[self.park if b is None else b for b in row] for row in self.bin]

    def idle(self):
        return [[b is None for b in row] for row in self.bin]
