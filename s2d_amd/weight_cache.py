"""Weight-derived copies: the one place that decides when such a copy is valid.

Every dense launch reads its weights through a derived copy (a pre-split fp16 image, the fused FFN's fragment image, a transposed /
flipped / re-tapped dgrad weight, a module's concatenated or permuted pack).  All of them obey one contract:

* a copy is valid only while its sources are the same OBJECTS at the same content version (version_of: torch's in-place counter plus
  the count of rewrites torch cannot see, bump_version);
* when only the version moved (an optimizer step), the copy is refreshed INTO THE SAME BUFFER, so that the caches hanging off its
  address refresh too instead of gaining a dead generation per step;
* a cache holds weak references to the sources only: a replaced weight dies, and its copies with it at the next sweep;
* an address that another tensor now occupies is never mistaken for the old one (the identity test).

DerivedCache implements this for the global caches keyed by address, PackedSlot for the packs a module keeps.  One sweep policy for all
DerivedCaches: when an entry is built and the cache holds `threshold` entries, the entries with a dead source are dropped and the
threshold becomes max(floor, 2 * live) -- O(1) amortised, dead entries bounded by the live ones.  (Before this module existed the
transposed / flipped / stride-2 dgrad caches swept at every new key and the FFN image cache whenever it held 64 entries.)

No device and no native library is needed here: tests/test_weight_cache_cpu.py drives everything with CPU tensors."""
import weakref


def version_of(t):
    """content version of a tensor for this library's caches: torch's in-place counter of the owning tensor + the count of rewrites
    torch cannot see (the multi-tensor optimizer kernel updates parameters and EMA copies through raw pointers: bump_version)"""
    base = t._base if t._base is not None else t
    return base._version + getattr(base, "_s2d_version", 0)


def bump_version(t):
    """declare that t's storage was rewritten behind torch's back (a kernel of this library wrote through its raw pointer)"""
    base = t._base if t._base is not None else t
    base._s2d_version = getattr(base, "_s2d_version", 0) + 1


def repack(old, new):
    """A module's cached packed weight copy after its sources changed: when the previous copy has the same shape it is overwritten
    IN PLACE (torch's counter moves, so the caches hanging off its address -- split images, transposed / flipped copies -- refresh
    into their existing buffers); otherwise `new` becomes the copy.  A fresh tensor per optimizer step would leave a dead generation of
    every such cache behind per step."""
    if old is not None and old.shape == new.shape and old.device == new.device and old.dtype == new.dtype:
        old.copy_(new)
        return old
    new = new.contiguous()
    if new._base is not None:
        new = new.clone()
    return mark_static(new)


def mark_static(t):
    """Declare a tensor a static weight (a packed / concatenated copy of parameters that its module caches): dense launches
    reading it as the B operand may then use a cached pre-split fp16 image instead of splitting it in every launch."""
    t._s2d_static = True
    return t


def owner_of(t):
    """the tensor whose version and lifetime a copy derived from `t` follows.  Identify it BEFORE detaching: a detached alias is a fresh
    object on every call (and does not carry the library's version attribute), so keying on it would rebuild the copy at every call"""
    return t._base if t._base is not None else t


_CACHES = []


def clear_weight_cache():
    """drop every entry of every DerivedCache (a checkpoint load: the copies are rebuilt at the next use)"""
    for c in _CACHES:
        c.clear()


class DerivedCache:
    """key -> [copy, weak references to its owners, their versions].  static: the copies are themselves static operands of the dense
    kernels (mark_static, with a version of their own that every refresh moves).  floor: the smallest size at which a sweep runs."""

    def __init__(self, static=False, floor=256):
        self.entries, self.static, self.floor, self.threshold = {}, static, floor, floor
        _CACHES.append(self)

    def __len__(self):
        return len(self.entries)

    def clear(self):
        self.entries.clear()
        self.threshold = self.floor

    def get(self, key, owners, build, refresh):
        """the copy under `key` of the tensors `owners` (owner_of-resolved): build() makes a new one, refresh(buf) rewrites one in place"""
        ent = self.entries.get(key)
        if ent is not None:
            refs, vers = ent[1], ent[2]
            stale, i = False, 0
            for o in owners:
                if refs[i]() is not o:           # an owner is dead, or another tensor now sits at this address: build anew
                    break
                if vers[i] != o._version + getattr(o, "_s2d_version", 0):      # version_of(o), spelled out: o is an owner already
                    stale = True
                i += 1
            else:
                if stale:
                    # the same tensors with new contents (an optimizer step): the same buffer again -- a fresh one per iteration would
                    # enter the caches keyed by its address anew every time and never leave them (0.5 GB per iteration at c4)
                    refresh(ent[0])
                    ent[2] = [version_of(o) for o in owners]
                    if hasattr(ent[0], "_s2d_version"):
                        ent[0]._s2d_version += 1
                return ent[0]
        buf = build()
        if self.static:
            mark_static(buf)._s2d_version = 0
        if len(self.entries) >= self.threshold:
            for k in [k for k, e in self.entries.items() if any(r() is None for r in e[1])]:
                del self.entries[k]
            self.threshold = max(self.floor, 2 * len(self.entries))
        # WEAK references: a copy must not keep a replaced weight alive
        self.entries[key] = [buf, [weakref.ref(o) for o in owners], [version_of(o) for o in owners]]
        return buf


class PackedSlot:
    """A module's packed copy (or tuple of copies) of some of its parameters: rebuilt when a source's version or the device changes,
    each member refreshed into the previous member's storage (repack)."""
    key = value = None

    def reset(self):
        self.key = self.value = None

    def get(self, sources, build):
        """the tuple of copies; build() returns a tensor or a tuple of tensors (None members stay None)"""
        key = tuple(version_of(s) for s in sources) + (sources[0].device,)
        if key != self.key:
            new = build()
            new = new if isinstance(new, tuple) else (new,)
            prev = self.value if self.value is not None and len(self.value) == len(new) else (None,) * len(new)
            self.value = tuple(None if n is None else repack(p, n) for p, n in zip(prev, new))
            self.key = key
        return self.value
