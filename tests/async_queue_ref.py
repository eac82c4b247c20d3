"""Pure-Python model of the ready queue of the asynchronous step (bp_bd_queue_*): plain lists, no torch.

States of an env: IDLE (has an action, starts in the next recv), BUSY, QUEUED (held, in the ring), TAKEN (held, delivered by a recv and awaiting its send).
The ring is modelled with explicit head / count arithmetic over a list of E slots so that wraps are visible."""

IDLE, BUSY, QUEUED, TAKEN = "idle", "busy", "queued", "taken"


class QueueModel:
    def __init__(self, num_envs, batch):
        assert 1 <= batch <= num_envs
        self.E, self.M = num_envs, batch
        self.ring = [0] * num_envs
        self.head = 0
        self.count = 0
        self.wraps = 0            # enqueues or takes whose ring index ran past the end
        self.rejected = 0
        self.state = [QUEUED] * num_envs
        self.fresh = [True] * num_envs
        self._enqueue(range(num_envs), True)   # open: every env is held and queued as a fresh row, in env-id order

    def _enqueue(self, envs, fresh):
        for e in sorted(envs):
            pos = self.head + self.count
            if pos >= self.E:
                pos -= self.E
                self.wraps += 1
            self.ring[pos] = e
            self.count += 1
            assert self.count <= self.E, "an env is in the ring at most once"
            self.state[e] = QUEUED
            self.fresh[e] = fresh

    def queued(self):
        return [self.ring[(self.head + k) % self.E] for k in range(self.count)]

    def recv(self, emitted, full_only=False):
        """emitted: the envs that emitted in the slice call (every IDLE env started in it: the others are BUSY afterwards).  Returns (ids, count, counts)."""
        emitted = sorted(emitted)
        for e in range(self.E):
            if self.state[e] == IDLE:
                self.state[e] = BUSY
        for e in emitted:
            assert self.state[e] == BUSY, "only a busy (or just started) env emits"
        self._enqueue(emitted, False)
        busy = sum(s == BUSY for s in self.state)
        n = min(self.M, self.count)
        if full_only and self.count < self.M and busy > 0:
            n = 0
        ids = []
        for _ in range(n):
            e = self.ring[self.head]
            self.head += 1
            if self.head == self.E:
                self.head = 0
                self.wraps += 1
            self.count -= 1
            self.state[e] = TAKEN
            ids.append(e)
        taken = sum(s == TAKEN for s in self.state)
        return ids + [-1] * (self.M - n), n, [n, self.count, busy, taken, self.rejected]

    def send(self, ids, reset=None):
        """Returns (accepted action rows, accepted reset rows) as lists of (j, env)."""
        assert len(ids) == self.M
        acts, resets, seen = [], [], set()
        for j, e in enumerate(ids):
            if e == -1:
                continue
            first = e not in seen      # the smallest row that names an env decides; later rows are rejected whatever became of the first
            seen.add(e)
            if not first or not (0 <= e < self.E) or self.state[e] != TAKEN:
                self.rejected += 1
                continue
            if reset is not None and reset[j]:
                resets.append((j, e))
            else:
                acts.append((j, e))
        for _, e in acts:
            self.state[e] = IDLE
        self._enqueue([e for _, e in resets], True)
        return acts, resets

    def close(self):
        """The envs the drain finishes."""
        busy = [e for e in range(self.E) if self.state[e] == BUSY]
        self.state = [IDLE] * self.E
        self.count = 0
        return busy

    def check(self):
        """An env is never in two places."""
        q = self.queued()
        assert len(set(q)) == len(q)
        for e in range(self.E):
            assert (self.state[e] == QUEUED) == (e in q), e
        assert sum(s in (QUEUED, TAKEN, BUSY, IDLE) for s in self.state) == self.E
