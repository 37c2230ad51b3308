"""The rule of hipdwc/derived.py on CPU tensors: an entry is valid while (version, storage address) of every owner is unchanged,
lives under id() of the first owner, goes when that owner dies, and is not found by an id() handed out again."""
import gc
import weakref

import torch

from hipdwc import derived


def _owners(n=1):
    return tuple(torch.nn.Parameter(torch.zeros(4)) for _ in range(n))


def test_stamp_is_version_and_address_of_every_owner():
    a, b = _owners(2)
    assert derived.stamp((a, b)) == ((a._version, a.data_ptr()), (b._version, b.data_ptr()))


def test_hit_returns_the_same_object():
    c, (p,) = derived.Cache(), _owners()
    v = object()
    assert c.get((p,), "k") is None
    assert c.put((p,), "k", v, {"n": 1}) is v
    ent = c.get((p,), "k")
    assert ent[0] == derived.stamp((p,)) and ent[1] is v and ent[2] == {"n": 1}
    assert c.get((p,), "k")[1] is v and len(c) == 1


def test_version_bump_misses():
    c, (p,) = derived.Cache(), _owners()
    c.put((p,), "k", 1)
    with torch.no_grad():
        p.add_(1.0)
    assert c.get((p,), "k") is None


def test_data_rebind_misses_with_the_version_unchanged():
    c, (p,) = derived.Cache(), _owners()
    c.put((p,), "k", 1)
    version = p._version
    other = torch.ones(4)
    p.data = other
    assert p._version == version and p.data_ptr() == other.data_ptr()
    assert c.get((p,), "k") is None


def test_of_two_owners_either_change_misses():
    for changed in (0, 1):
        c, ps = derived.Cache(), _owners(2)
        c.put(ps, "k", 1)
        assert c.get(ps, "k")[1] == 1
        with torch.no_grad():
            ps[changed].mul_(2.0)
        assert c.get(ps, "k") is None


def test_an_old_stamp_neither_finds_nor_relabels_a_newer_entry():
    c, ps = derived.Cache(), _owners(2)
    old = derived.stamp(ps)
    with torch.no_grad():
        ps[1].add_(1.0)
    c.put(ps, "k", "new")
    assert c.get(ps, "k", old) is None                       # the newer entry is not found under the old stamp
    c.put(ps, "k", "old", None, old)                         # values read before the step are stored as what they are
    assert c.get(ps, "k", old)[1] == "old" and c.get(ps, "k", old)[0] == old
    assert c.get(ps, "k") is None                            # and never pass for values of the present stamp


def test_dead_anchor_leaves_nothing():
    c, ps = derived.Cache(), _owners(2)
    c.put(ps, "k", torch.zeros(2))
    c.put(ps[:1], "j", 2)
    assert len(c) == 1
    alive = ps[1]
    del ps
    gc.collect()
    assert len(c) == 0 and c.slots == {} and alive is not None


def test_a_slot_under_a_reused_id_is_not_served():
    c, (p,) = derived.Cache(), _owners()
    (other,) = _owners()
    dead = torch.zeros(1)
    dead_ref = weakref.ref(dead)
    del dead
    gc.collect()
    assert dead_ref() is None
    for ref in (dead_ref, weakref.ref(other)):               # planted: the slot of an object that had this id before
        c.slots[id(p)] = (ref, {"k": (derived.stamp((p,)), "stale", None)})
        assert c.get((p,), "k") is None and c.entries(p) == {}
        c.put((p,), "k", "fresh")
        assert c.get((p,), "k")[1] == "fresh" and c.slots[id(p)][0]() is p


def test_callback_of_a_dead_anchor_keeps_a_newer_slot_of_its_id():
    class Cell:                                              # (any weakly referenceable owner: the rule reads _version and data_ptr())
        _version = 0

        def data_ptr(self):
            return 0

    c = derived.Cache()
    old, new = Cell(), Cell()
    c.put((old,), "k", "old")
    aid = id(old)
    slot = c.slots.pop(aid)                                  # the id is handed out again while the first object's weakref is alive:
    c.put((new,), "k", "new")                                # file the newer anchor's slot under it
    c.slots[aid] = c.slots.pop(id(new))
    del old
    gc.collect()                                             # the first slot's callback runs now
    assert slot[0]() is None
    assert c.slots[aid][0]() is new and c.slots[aid][1]["k"][1] == "new"


def test_keys_under_one_anchor_are_independent():
    c, (p,) = derived.Cache(), _owners()
    c.put((p,), "a", 1)
    c.put((p,), ("b", 2), 2)
    assert c.get((p,), "a")[1] == 1 and c.get((p,), ("b", 2))[1] == 2 and sorted(map(str, c.entries(p))) == ["('b', 2)", "a"]
    stale = derived.stamp((p,))
    with torch.no_grad():
        p.add_(1.0)
    c.put((p,), "a", 3)
    assert c.get((p,), "a")[1] == 3 and c.get((p,), ("b", 2)) is None and c.entries(p)[("b", 2)][0] == stale
    c.restamp(p, ("b", 2), derived.stamp((p,)))              # (refresh_prepared: the value was rebuilt in place)
    assert c.get((p,), ("b", 2)) == (derived.stamp((p,)), 2, None) and c.get((p,), "a")[1] == 3
