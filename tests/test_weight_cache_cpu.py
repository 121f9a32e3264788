"""The contract of the weight-derived copies (s2d_amd/weight_cache.py) on CPU tensors: a copy is served while its owners are the same
objects at the same version, refreshed into the same buffer when only the version moved, rebuilt when an owner was replaced -- also
under a recycled address -- and dropped some time after an owner died.  build / refresh are counting stand-ins for the kernels."""
import gc

import pytest
import torch

from s2d_amd import weight_cache as wc


_MADE = []


def new_cache(**kw):
    _MADE.append(wc.DerivedCache(**kw))
    return _MADE[-1]


@pytest.fixture(autouse=True)
def _unregister():
    yield
    for c in _MADE:                                # the caches made here do not stay registered after the test
        wc._CACHES.remove(c)
    del _MADE[:]


class Derive:
    """copy = 2 * operands' sum; counts the builds and the refreshes.  Like the library's front ends it identifies the owners first and
    works on detached aliases, which are fresh objects on every call"""

    def __init__(self, cache):
        self.cache, self.builds, self.refreshes = cache, 0, 0

    def get(self, *ts, key=None):
        owners = tuple(wc.owner_of(t) for t in ts)
        ts = [t.detach() for t in ts]

        def build():
            self.builds += 1
            return 2 * sum(ts)

        def refresh(buf):
            self.refreshes += 1
            buf.copy_(2 * sum(ts))

        return self.cache.get(key or tuple(t.data_ptr() for t in ts), owners, build, refresh)

    @property
    def counts(self):
        return self.builds, self.refreshes


def test_hit_serves_the_same_object_without_build_or_refresh():
    d, w = Derive(new_cache()), torch.ones(4)
    a = d.get(w)
    assert d.get(w) is a and d.counts == (1, 0) and len(d.cache) == 1
    assert torch.equal(a, torch.full((4,), 2.0))


def test_in_place_write_refreshes_into_the_same_buffer():
    d, w = Derive(new_cache()), torch.ones(4)
    a = d.get(w)
    ptr = a.data_ptr()
    w.add_(1)
    b = d.get(w)
    assert b is a and b.data_ptr() == ptr and d.counts == (1, 1) and torch.equal(b, torch.full((4,), 4.0))
    assert d.get(w) is a and d.counts == (1, 1)


def test_bump_version_alone_refreshes():
    d, w = Derive(new_cache()), torch.ones(4)
    a = d.get(w)
    v = w._version
    wc.bump_version(w)                             # (a raw-pointer write: torch's counter does not move)
    assert w._version == v and d.get(w) is a and d.counts == (1, 1)


def test_a_view_resolves_to_its_base():
    d, w = Derive(new_cache()), torch.ones(2, 4)
    view = w[0]
    assert wc.owner_of(view) is w and wc.owner_of(w) is w
    a = d.get(view)
    w.mul_(3)                                      # through the base
    assert d.get(view) is a and d.counts == (1, 1)
    for _ in range(3):                             # a fresh view, and inside Derive.get a fresh detached alias, per call
        assert d.get(w[0]) is a
    assert d.counts == (1, 1) and a.shape == (4,)
    assert wc.owner_of(w.detach()) is not w        # (why the owner is identified before detaching)
    wc.bump_version(view)                          # ... and a bump through the view lands on the base
    assert d.get(view) is a and d.counts == (1, 2)


def test_a_recycled_address_is_built_not_hit_and_not_refreshed():
    d = Derive(new_cache())
    w1, w2 = torch.ones(4), torch.full((4,), 5.0)
    assert w1._version == w2._version              # the version alone could not tell them apart
    a = d.get(w1, key="address")
    b = d.get(w2, key="address")
    assert b is not a and d.counts == (2, 0) and torch.equal(a, torch.full((4,), 2.0)) and torch.equal(b, torch.full((4,), 10.0))
    del w2
    gc.collect()
    w3 = torch.zeros(4)                            # ... and after the entry's tensor died
    assert d.get(w3, key="address") is not b and d.counts == (3, 0) and len(d.cache) == 1


def test_dead_owners_leave_at_an_amortised_sweep():
    floor = 8
    d = Derive(new_cache(floor=floor))
    live = [torch.ones(2) for _ in range(3)]
    for i, w in enumerate(live):
        d.get(w, key=("live", i))
    dead_key = ("dead", 0)
    for i in range(40):
        w = torch.ones(2)
        d.get(w, key=("dead", i))
        del w
        gc.collect()
        assert len(d.cache) <= 2 * len(live) + floor
    assert dead_key not in d.cache.entries and len(d.cache) < 3 + floor
    for i, w in enumerate(live):                   # the live entries survived every sweep
        d.get(w, key=("live", i))
    assert d.builds == 43 and d.refreshes == 0
    # the threshold follows the live population: with 3 * floor live entries no sweep runs per key
    many = [torch.ones(2) for _ in range(3 * floor)]
    for i, w in enumerate(many):
        d.get(w, key=("many", i))
    assert d.cache.threshold >= 2 * floor and len(d.cache) <= 2 * (len(live) + len(many)) + floor


def test_multi_owner_entry():
    d = Derive(new_cache(floor=64))
    w1, w2, w3 = torch.ones(4), torch.ones(4), torch.ones(4)
    a = d.get(w1, w2, w3, key="ffn")
    assert d.get(w1, w2, w3, key="ffn") is a and d.counts == (1, 0)
    for n, w in enumerate((w1, w2, w3)):           # a version change of any one owner refreshes
        w.add_(1) if n != 1 else wc.bump_version(w)
        assert d.get(w1, w2, w3, key="ffn") is a and d.counts == (1, n + 1)
    for n, pos in enumerate(range(3)):             # replacing any one owner rebuilds
        ws = [w1, w2, w3]
        ws[pos] = torch.ones(4)
        b = d.get(*ws, key="ffn")
        assert b is not a and d.counts == (2 + 2 * n, 3)
        a = d.get(w1, w2, w3, key="ffn")           # (and back: the entry now belongs to the other set)
        assert a is not b and d.counts == (3 + 2 * n, 3)


def test_static_copies_chain_into_the_next_cache():
    first, second = Derive(new_cache(static=True)), Derive(new_cache())     # the transposed weight, then its split image
    w = torch.ones(4)
    wt = first.get(w)
    assert wt._s2d_static is True and wt._s2d_version == 0
    img = second.get(wt)
    assert not hasattr(img, "_s2d_version") and not hasattr(img, "_s2d_static")
    for step in (1, 2, 3):
        wc.bump_version(w)                         # the optimizer step
        assert first.get(w) is wt and wt._s2d_version == step and first.counts == (1, step)
        assert second.get(wt) is img and second.counts == (1, step)
        assert second.get(wt) is img and second.counts == (1, step)
    assert wc.version_of(wt) == wt._version + 3      # (a refresh by a kernel, which torch's counter misses, moves it just as far)


def test_clear_weight_cache_empties_every_instance():
    caches = [new_cache(), new_cache(static=True), new_cache(floor=4)]
    ws = [torch.ones(2) for _ in range(6)]
    for c in caches:
        d = Derive(c)
        for w in ws:
            d.get(w)
    caches[2].threshold = 99
    assert [len(c) for c in caches] == [6, 6, 6]
    wc.clear_weight_cache()
    assert [len(c) for c in caches] == [0, 0, 0] and caches[2].threshold == 4


def test_the_library_caches_are_registered():
    from s2d_amd import backward as B, ops
    for c in (ops._SPLIT, ops._FFN_PACK, B._WT, B._WF, B._WS2):
        assert isinstance(c, wc.DerivedCache) and c in wc._CACHES
    assert not ops._SPLIT.static and not ops._FFN_PACK.static and B._WT.static and B._WF.static and B._WS2.static
    assert ops.version_of is wc.version_of and ops.clear_weight_cache is wc.clear_weight_cache


def test_packed_slot():
    slot = wc.PackedSlot()
    a, b = torch.nn.Parameter(torch.ones(3, 2)), torch.nn.Parameter(torch.ones(2))
    builds = []

    def build():
        builds.append(1)
        return torch.cat([a.detach(), a.detach()], 0), None, b.detach()

    p = slot.get((a, b), build)
    assert slot.get((a, b), build) is p and len(builds) == 1 and p[1] is None
    assert p[0]._s2d_static and p[2]._s2d_static
    ptrs = (p[0].data_ptr(), p[2].data_ptr())
    v0 = wc.version_of(p[0])
    with torch.no_grad():
        a.add_(1)                                  # a version bump of any source changes the key ...
    q = slot.get((a, b), build)
    assert len(builds) == 2 and (q[0] is p[0] and q[2] is p[2]) and (q[0].data_ptr(), q[2].data_ptr()) == ptrs
    assert torch.equal(q[0], torch.full((6, 2), 2.0)) and wc.version_of(q[0]) > v0       # ... refreshed in place, visibly to the next cache
    wc.bump_version(b)
    assert slot.get((a, b), build)[0] is p[0] and len(builds) == 3
    a.data = torch.ones(4, 2)                      # a shape change replaces the member (and only that one)
    wc.bump_version(a)
    r = slot.get((a, b), build)
    assert len(builds) == 4 and r[0] is not p[0] and r[0].shape == (8, 2) and r[2] is p[2]
    slot.reset()                                   # reset() forces a build
    assert slot.key is None and slot.value is None
    s = slot.get((a, b), build)
    assert len(builds) == 5 and s[0] is not r[0]
    one = wc.PackedSlot().get((b,), lambda: b.detach() * 2)                               # a single tensor comes back as a 1-tuple
    assert isinstance(one, tuple) and len(one) == 1 and torch.equal(one[0], torch.full((2,), 2.0))


def test_invalidate_weight_caches_finds_slots_by_type():
    from s2d_amd.checkpoint import invalidate_weight_caches

    class Leaf(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.ones(2, 2))
            self.some_arbitrary_name = wc.PackedSlot()

        def packed(self):
            return self.some_arbitrary_name.get((self.weight,), lambda: self.weight.detach().t())[0]

    tree = torch.nn.Sequential(Leaf(), torch.nn.Sequential(Leaf()))
    first = [m.packed() for m in (tree[0], tree[1][0])]
    cache = new_cache()
    Derive(cache).get(first[0])
    assert [m.packed() for m in (tree[0], tree[1][0])][0] is first[0] and len(cache) == 1
    invalidate_weight_caches(tree)
    assert tree[0].some_arbitrary_name.key is None and tree[1][0].some_arbitrary_name.value is None and len(cache) == 0
    assert tree[0].packed() is not first[0]
