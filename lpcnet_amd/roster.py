"""The roster of a batch whose streams come and go (include/lpcnet_batch.h: lpcnet_batch_set_active, lpcnet_batch_copy_streams).

A batch is a capacity; of every shard's streams the first `active` ones run.  StreamRoster keeps the map caller id <-> slot so that every
shard's streams stay a dense prefix: a joining stream takes the slot at its shard's count, and when streams leave, the holes they leave below
the new count are filled from the tail (swap-remove).  The rules are those of lpcnet_amd/csrc/api_roster.h, restated here in Python so that
the book can be kept without the library; given a batch, the roster also drives its three calls.
"""
from __future__ import annotations


def plan_leave(spans, active, leaving):
    """spans [(first, count)] per shard, active [count per shard], leaving: slots (distinct, all active).  Returns (pairs [(src, dst)],
    new_active): after the copies every shard's survivors are exactly its first new_active[k] slots.  The fewest copies there can be: a leaving
    slot at or above its shard's new count costs none; the lowest hole takes the lowest survivor of the tail."""
    gone = set()
    new_active = list(active)
    for s in leaving:
        k = next((k for k, (f, c) in enumerate(spans) if f <= s < f + c), None)
        if k is None or s - spans[k][0] >= active[k] or s in gone:
            raise ValueError(f"slot {s} is not an active stream (or leaves twice)")
        gone.add(s)
        new_active[k] -= 1
    pairs = []
    for k, (f, _) in enumerate(spans):
        movers = (s for s in range(f + new_active[k], f + active[k]) if s not in gone)
        pairs += [(next(movers), hole) for hole in range(f, f + new_active[k]) if hole in gone]
    return pairs, new_active


class StreamRoster:
    """caller ids <-> slots of a batch of the given shard spans [(first, count)] (LPCNetBatch.shards without the device), or of `batch`.
    With a batch, join() and leave() make the API calls themselves: join resets the slot (reset, and analysis_reset / plc_reset where
    `analysis` / `plc` say the batch uses them) and raises the count; leave enqueues the copies and lowers the counts."""

    def __init__(self, spans=None, batch=None, analysis=False, plc=False):
        if spans is None:
            spans = [(f, c) for f, c, _ in batch.shards]
        self.spans = [(int(f), int(c)) for f, c in spans]
        self.active = [0] * len(self.spans)
        self.batch, self.analysis, self.plc = batch, analysis, plc
        self._slot = {}               # id -> slot
        self._id = {}                 # slot -> id
        if batch is not None:
            self._push()

    def _push(self):
        self.batch.active = self.active[0] if len(self.active) == 1 else self.active

    def slots(self):
        """{id: slot}"""
        return dict(self._slot)

    def join(self, ident):
        """the slot of a new stream: on the least-loaded shard with room, the first of them on a tie"""
        if ident in self._slot:
            raise ValueError(f"{ident!r} is in the roster already")
        free = [k for k, (_, c) in enumerate(self.spans) if self.active[k] < c]
        if not free:
            raise RuntimeError("the batch is full")
        k = min(free, key=lambda k: (self.active[k], k))
        slot = self.spans[k][0] + self.active[k]
        if self.batch is not None:
            if self.plc:
                self.batch.plc_reset(slot, 1)         # (resets the synthesis and analysis states too)
            else:
                self.batch.reset(slot, 1)
                if self.analysis:
                    self.batch.analysis_reset(slot, 1)
        self.active[k] += 1
        self._slot[ident] = slot
        self._id[slot] = ident
        if self.batch is not None:
            self._push()
        return slot

    def leave(self, idents):
        """the streams `idents` go: returns (pairs [(src, dst)], new counts per shard); the ids of the moved streams now name their new slots"""
        idents = list(idents)
        pairs, new_active = plan_leave(self.spans, self.active, [self._slot[i] for i in idents])
        for i in idents:
            del self._id[self._slot.pop(i)]
        for src, dst in pairs:
            ident = self._id.pop(src)
            self._id[dst] = ident
            self._slot[ident] = dst
        self.active = new_active
        if self.batch is not None:
            if pairs:
                self.batch.copy_streams([p[0] for p in pairs], [p[1] for p in pairs])
            self._push()
        return pairs, list(new_active)

    def migrate(self, idents, other: "StreamRoster"):
        """the streams `idents` move to `other`'s batch: they join `other` on its least-loaded shards (no reset: the records arrive whole), one
        copy_streams_to carries them, then they leave this roster with the usual swap-remove.  Returns {id: slot in other}."""
        idents = list(idents)
        if len(set(idents)) != len(idents) or any(i not in self._slot for i in idents):
            raise ValueError("migrate: ids must be distinct streams of this roster")
        if any(i in other._slot for i in idents):
            raise ValueError("migrate: an id is in the other roster already")
        load = list(other.active)
        dst = []
        for _ in idents:                  # (planned before either book changes)
            free = [k for k, (_, c) in enumerate(other.spans) if load[k] < c]
            if not free:
                raise RuntimeError("the other batch is full")
            k = min(free, key=lambda k: (load[k], k))
            dst.append(other.spans[k][0] + load[k])
            load[k] += 1
        src = [self._slot[i] for i in idents]
        if self.batch is not None and other.batch is not None and idents:
            self.batch.copy_streams_to(src, other.batch, dst)
        for i, d in zip(idents, dst):
            other._slot[i] = d
            other._id[d] = i
        other.active = load
        if other.batch is not None:
            other._push()
        self.leave(idents)
        return dict(zip(idents, dst))
