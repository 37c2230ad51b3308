"""Values derived from parameters, kept until a parameter changes.

One rule for every such value (prepared weight layouts, concatenated parameters, the LSTM's transposed weights and bias sum, the
python float of a constant): an entry is valid while ``(p._version, p.data_ptr())`` of every owner is what it was when the value
was made; it lives under ``id()`` of the first owner (the anchor) and goes when the anchor dies; an ``id()`` handed out again
after that finds nothing.  Imports torch and weakref only: CPU tensors do.
"""
import weakref

import torch  # noqa: F401  (the owners are tensors: `_version`, `data_ptr()`)


def stamp(owners):
    """(version counter, storage address) of every owner.  Writers that go through ``.data`` (dist.broadcast(t.data), load_state_dict
    on a rebound tensor, Module.to()) do not always bump the version, but most of them move or re-bind the storage; the in-tree
    ``.data`` writers bump the version explicitly (dp.broadcast_module, host.moving_average, host.weights_init)."""
    return tuple([(o._version, o.data_ptr()) for o in owners])


class Cache:
    """id(anchor) -> (weakref to the anchor, {key: (stamp, value, extra)}), anchor = owners[0]."""

    def __init__(self):
        self.slots = {}

    def __len__(self):
        """Anchors with a slot."""
        return len(self.slots)

    def entries(self, anchor):
        """The {key: entry} dict of a live anchor; an empty one (kept nowhere) for an anchor that has none."""
        slot = self.slots.get(id(anchor))
        return slot[1] if slot is not None and slot[0]() is anchor else {}

    def get(self, owners, key, at=None):
        """The entry (stamp, value, extra) of `key` if no owner changed since it was stored, else None.  `at`: a stamp the caller
        took earlier, instead of the owners' present one."""
        anchor = owners[0]
        slot = self.slots.get(id(anchor))
        if slot is not None and slot[0]() is anchor:
            ent = slot[1].get(key)
            # (`stamp(owners)` written out: this is the path of every launch, and the call costs as much as the dict lookup)
            if ent is not None and ent[0] == (tuple([(o._version, o.data_ptr()) for o in owners]) if at is None else at):
                return ent
        return None

    def put(self, owners, key, value, extra=None, at=None):
        """Store `value` under the owners' present stamp, or under `at` (the stamp of the values it was made from)."""
        anchor, aid, slots = owners[0], id(owners[0]), self.slots
        slot = slots.get(aid)
        if slot is None or slot[0]() is not anchor:

            def drop(ref):          # (only the slot this weakref guards: the id may belong to a newer anchor by now)
                if slots.get(aid, (None,))[0] is ref:
                    del slots[aid]
            slot = slots[aid] = (weakref.ref(anchor, drop), {})
        slot[1][key] = (stamp(owners) if at is None else at, value, extra)
        return value

    def restamp(self, anchor, key, at):
        """The entry of `key` was rebuilt in place (refresh_prepared): same value and extra, valid at `at`."""
        ents = self.entries(anchor)
        ents[key] = (at,) + ents[key][1:]
