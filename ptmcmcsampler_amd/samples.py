"""Thinned posterior samples of every cold chain, kept on the device (csrc/ptmi_samples.hip, include/ptmi.h ``ptmi_samples_*``;
``PTEngine.with_stages(samples=64)``, ``PTSampler.posterior_samples``): the host's side of the stage -- the spec the engine and the
sampler take, the schedule that decides which iteration goes to which slot of the bounded buffer, and the flat view that plotting
tools take."""
import heapq

import numpy as np

NSLOTS_MAX = 65535


def samples_spec(spec):
    """``samples=`` of ``PTEngine.with_stages`` -> (slots, every), checked: an integer is ``slots`` with ``every = 1``; a dict has the keys
    ``slots`` (``1 <= slots <= 65535``, ``ptmi_samples_attach``) and, optionally, ``every`` (``>= 1``: the candidates are the iterations
    ``samples_from + every * m``)."""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))      # noqa: E731
    if isinstance(spec, dict):
        extra = sorted(set(spec) - {"slots", "every"})
        if extra:
            raise ValueError("samples: a dict has the keys slots and every (got %s)" % ", ".join(repr(k) for k in extra))
        if "slots" not in spec:
            raise ValueError("samples: a dict names slots, {\"slots\": n, \"every\": k}")
        slots, every = spec["slots"], spec.get("every", 1)
    else:
        slots, every = spec, 1
    if not is_int(slots) or not 1 <= int(slots) <= NSLOTS_MAX:
        raise ValueError("samples: slots = %r: an integer, 1 <= slots <= %d" % (slots, NSLOTS_MAX))
    if not is_int(every) or int(every) < 1:
        raise ValueError("samples: every = %r: an integer >= 1" % (every,))
    return int(slots), int(every)


class SlotPlan(object):
    """Which iterations a buffer of ``nslots`` snapshots holds, for a run whose length nobody knows in advance.  The candidates are the
    iterations ``first + every * m``, ``m = 1, 2, ...``; the plan keeps those with ``m`` a multiple of ``2 ** level``.  When a candidate
    finds no free slot the level goes up by one -- every other held snapshot is let go -- so the held set is always evenly spaced over
    the whole run so far: ``first + every * 2 ** level * j`` for ``j = 1 .. M >> level``, ``M`` the candidates seen, between
    ``nslots // 2`` and ``nslots`` of them once ``M >= nslots``.  ``slot_iter [nslots]``: the iteration a slot holds, -1 = free; with
    ``level`` it is the whole state (a checkpoint carries the two)."""

    def __init__(self, nslots, every=1):
        self.nslots, self.every, self.level = int(nslots), int(every), 0
        self.slot_iter = np.full(self.nslots, -1, dtype=np.int64)

    @property
    def stride(self):
        """Iterations between two held snapshots."""
        return self.every << self.level

    def held(self):
        """(iters, slots) of the held snapshots, by ascending iteration."""
        slots = np.flatnonzero(self.slot_iter >= 0)
        order = np.argsort(self.slot_iter[slots], kind="stable")
        return self.slot_iter[slots][order], slots[order]

    def take(self, first, lo, hi):
        """The ``(iteration, slot)`` pairs to gather for iterations ``lo .. hi``, by ascending iteration, with the state brought up to
        ``hi``.  The list is the call's FINAL assignment: a snapshot placed and let go again inside the call is not in it, so no slot
        appears twice.  The result does not depend on how a run is cut into calls."""
        first, lo, hi, every = int(first), int(lo), int(hi), self.every
        out = {}                                                      # slot -> iteration
        free = np.flatnonzero(self.slot_iter < 0).tolist()            # a heap of the free slots (ascending: a heap as it stands), kept up
                                                                      # through the call: a placement costs log nslots, not a scan
        m = max(1, -((first - lo) // every))                          # the first candidate at or behind lo
        m_hi = (hi - first) // every
        while m <= m_hi:
            step = 1 << self.level
            if m % step:
                m += step - m % step                                  # the next candidate this level keeps
                continue
            if not free:
                self.level += 1
                step = 1 << self.level
                gone = np.flatnonzero(((self.slot_iter - first) // every) % step != 0)      # every slot is held here
                self.slot_iter[gone] = -1
                free = gone.tolist()
                for s in free:
                    out.pop(s, None)
                if m % step:
                    m += 1
                    continue
            s = heapq.heappop(free)
            self.slot_iter[s] = first + m * every
            out[s] = first + m * every
            m += 1
        return sorted((i, s) for s, i in out.items())


def flat(samples):
    """``engine.samples()`` / ``PTSampler.samples`` as one array per quantity, for tools that take a single chain: ``(x [n * W][d],
    lnprob [n * W], lnlike [n * W])``, snapshot-major (the two last ones ``None`` where the run kept no lnL)."""
    x = np.asarray(samples["x"])
    one = lambda k: np.asarray(samples[k]).reshape(-1) if k in samples else None      # noqa: E731
    return x.reshape(-1, x.shape[-1]), one("lnprob"), one("lnlike")
