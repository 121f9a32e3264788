"""Host reference of the hole filling of u8 index maps (ops.fill_index_holes, s2d_amd/index_components.py) and the constructed cases
of its tests.

The rule.  `conn` is the connectivity of the instances; the zero pixels of an image are labelled under the complementary
connectivity c' (8 -> 4, 4 -> 8).  A zero component is a hole iff none of its pixels lies on the frame border.  Its owners are the
ids on binary_dilation(component, structure(c')) & ~component.  A hole is filled iff its area <= max_hole_area and it has exactly one
owner k: its pixels become k, and colors[k - 1] in `rgb`; with `rgb`, a hole whose owner has no row in `colors` is left alone.  The
case builders take the kernel's tile (th, tw), so that their borders and corners sit where the kernel's do."""
import numpy as np
from scipy import ndimage

from tests.index_components_refs import frame_shape, make_rgb, structure  # noqa: F401

ALL = 2 ** 31 - 1


def hole_conn(conn):
    if conn not in (4, 8):
        raise ValueError(f"connectivity {conn}: 4 or 8")
    return 4 if conn == 8 else 8


def _holes(image, conn):
    """u8 [H,W] -> (box, part, area, sorted owner ids) per hole, in raster order of the first pixel: `part` is the hole's pixels inside
    `box`, the slices of its bounding box grown by one pixel"""
    st = structure(hole_conn(conn))
    lab, k = ndimage.label(image == 0, st)
    H, W = image.shape
    for i, (sy, sx) in enumerate(ndimage.find_objects(lab), 1):
        if sy.start == 0 or sx.start == 0 or sy.stop == H or sx.stop == W:
            continue                                                  # a pixel on the frame border: no hole
        box = (slice(sy.start - 1, sy.stop + 1), slice(sx.start - 1, sx.stop + 1))      # the component and its neighbours
        part = lab[box] == i
        ring = ndimage.binary_dilation(part, st) & ~part
        assert (image[box][ring] != 0).all()                          # maximality: every neighbour outside is an instance pixel
        yield box, part, int(part.sum()), sorted(set(image[box][ring].tolist()))


def holes(image, conn):
    """u8 [H,W] -> [(component bool [H,W], area, sorted owner ids)] of the holes of one image"""
    out = []
    for box, part, area, owners in _holes(image, conn):
        comp = np.zeros(image.shape, bool)
        comp[box] = part
        out.append((comp, area, owners))
    return out


def ref_fill_holes(index, max_hole_area, conn, rgb=None, colors=None):
    """-> (out u8 [N,H,W], filled int32 [N], rgb after the call or None)"""
    index = np.asarray(index)
    assert index.dtype == np.uint8 and index.ndim == 3
    max_hole_area = ALL if max_hole_area == "all" else int(max_hole_area)
    assert max_hole_area >= 1
    out, filled = index.copy(), np.zeros(index.shape[0], np.int32)
    rgb = None if rgb is None else np.array(rgb, copy=True)
    if rgb is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.ndim == 2 and colors.shape[1] == 3
    for n in range(index.shape[0]):
        for box, part, area, owners in _holes(index[n], conn):
            if area > max_hole_area or len(owners) != 1:
                continue
            k = owners[0]
            if rgb is not None:
                if k > len(colors):
                    continue
                rgb[n][box][part] = colors[k - 1]
            out[n][box][part] = k
            filled[n] += area
    return out, filled, rgb


def color_table(n, seed=11):
    """u8 [n,3] of distinct non-zero rows, none of them make_rgb's background sentinel (7, 7, 7)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(8, 256, (n, 3), dtype=np.uint8)
    t[:, 0] = 8 + np.arange(n) % 248
    t[:, 1] = 8 + np.arange(n) // 248
    return t


# ---------------------------------------------------------------------------------------------------------------- constructed cases
def _solid(th, tw, value=1):
    H, W = frame_shape(th, tw)
    return np.full((H, W), value, np.uint8)


def one_pixel(th, tw):
    m = _solid(th, tw, 3)
    m[5, 7] = 0
    return m[None]


def diagonal_pair(th, tw):
    """two zero pixels that touch only diagonally inside one id.  The zeros join under the COMPLEMENTARY connectivity: instances of
    conn 4 give one hole of 2 pixels (the zeros join by 8), instances of conn 8 two holes of 1"""
    m = _solid(th, tw, 2)
    m[4, 4] = m[5, 5] = 0
    return m[None]


def crossing(th, tw, where):
    """a 3 x 3 hole across the first vertical tile border, the first horizontal one, or the four-tile corner"""
    m = _solid(th, tw, 9)
    y, x = {"vertical": (5, tw - 1), "horizontal": (th - 1, 5), "corner": (th - 1, tw - 1)}[where]
    m[y - 1:y + 2, x - 1:x + 2] = 0
    return m[None]


def corner_diagonal(th, tw, anti=False):
    """two zero pixels that touch only diagonally AT the four-tile corner"""
    m = _solid(th, tw, 4)
    if anti:
        m[th - 1, tw] = m[th, tw - 1] = 0
    else:
        m[th - 1, tw - 1] = m[th, tw] = 0
    return m[None]


def reaches_border(th, tw, side):
    """a 3-pixel bar of zeros that ends ON the frame border at `side`: no hole"""
    m = _solid(th, tw, 6)
    H, W = m.shape
    if side == "top":
        m[0:3, W // 2] = 0
    elif side == "bottom":
        m[H - 3:H, W // 2] = 0
    elif side == "left":
        m[H // 2, 0:3] = 0
    elif side == "right":
        m[H // 2, W - 3:W] = 0
    else:
        raise KeyError(side)
    return m[None]


def area_pair(th, tw, n=6):
    """one hole of exactly n pixels and one of n + 1, both rows of zeros inside one id"""
    m = _solid(th, tw, 5)
    m[3, 2:2 + n] = 0
    m[th + 3, 2:2 + n + 1] = 0
    return m[None]


def two_owners(th, tw):
    """a gap between two touching instances: a hole with owners 1 and 2"""
    m = _solid(th, tw, 1)
    m[:, tw:] = 2
    m[th // 2:th // 2 + 3, tw - 1:tw + 1] = 0
    return m[None]


def diagonal_owner(th, tw):
    """a one-pixel hole in id 1 whose only contact with id 2 is diagonal: one owner where the zeros join by 4 (instances conn 8: filled),
    two where they join by 8 (instances conn 4: not filled) -- the owners are taken under the HOLES' connectivity"""
    m = _solid(th, tw, 1)
    m[:th // 2, :tw // 2] = 2
    m[th // 2, tw // 2] = 0
    return m[None]


def island(th, tw):
    """an island of id 2 inside a zero ring inside id 1: the ring has two owners and stays; the island's own one-pixel hole is filled
    with 2"""
    m = _solid(th, tw, 1)
    y, x = th - 4, tw - 4
    m[y:y + 9, x:x + 9] = 0
    m[y + 2:y + 7, x + 2:x + 7] = 2
    m[y + 4, x + 4] = 0
    return m[None]


def owner_ids(th, tw):
    """three one-pixel holes, in ids 1, 254 and 255"""
    H, W = frame_shape(th, tw)
    m = np.zeros((H, W), np.uint8)
    for i, v in enumerate((1, 254, 255)):
        m[2 + 6 * i:7 + 6 * i, 2:7] = v
        m[4 + 6 * i, 4] = 0
    return m[None]


def spiral_hole(th, tw):
    """a one-pixel-wide spiral of zeros from near the border to the centre inside one id: ONE hole that winds through every tile"""
    H, W = frame_shape(th, tw)
    m = np.full((H, W), 7, np.uint8)
    y, x, d = 1, 1, 0
    m[y, x] = 0
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def can(d):
        dy, dx = steps[d]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        return 1 <= y1 < H - 1 and 1 <= x1 < W - 1 and m[y1, x1] != 0 and not (1 <= y2 < H - 1 and 1 <= x2 < W - 1 and m[y2, x2] == 0)

    while True:
        if not can(d):
            d = (d + 1) % 4
            if not can(d):
                break
        y, x = y + steps[d][0], x + steps[d][1]
        m[y, x] = 0
    return m[None]


def frame_ring(H, W, value=1):
    """a one-pixel ring of `value` on the frame border round ONE hole of (H-2)(W-2) pixels"""
    m = np.zeros((H, W), np.uint8)
    m[0], m[-1], m[:, 0], m[:, -1] = value, value, value, value
    return m[None]


def blobs_with_speckle(H, W, n_blobs=20, speckle=0.01, seed=0, ids=None):
    """seeded discs of ids 1..n_blobs (a later one over an earlier one), then `speckle` of all pixels set to a random id or 0"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    ids = list(range(1, n_blobs + 1)) if ids is None else list(ids)
    for v in ids:
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(min(H, W) // 12, min(H, W) // 4)
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v
    hit = rng.random((H, W)) < speckle
    noise = rng.choice(np.array([0] + ids, np.uint8), size=(H, W))
    return np.where(hit, noise, m).astype(np.uint8)[None]


GEOMETRY_CASES = ("one_pixel", "diagonal", "cross_vertical", "cross_horizontal", "cross_corner", "corner_diagonal", "corner_anti",
                  "border_top", "border_bottom", "border_left", "border_right", "area_pair", "two_owners", "island", "diagonal_owner", "owner_ids",
                  "spiral_hole")


def geometry_case(name, th, tw):
    if name == "one_pixel":
        return one_pixel(th, tw)
    if name == "diagonal":
        return diagonal_pair(th, tw)
    if name.startswith("cross_"):
        return crossing(th, tw, name[len("cross_"):])
    if name in ("corner_diagonal", "corner_anti"):
        return corner_diagonal(th, tw, name == "corner_anti")
    if name.startswith("border_"):
        return reaches_border(th, tw, name[len("border_"):])
    if name == "area_pair":
        return area_pair(th, tw)
    if name == "two_owners":
        return two_owners(th, tw)
    if name == "island":
        return island(th, tw)
    if name == "diagonal_owner":
        return diagonal_owner(th, tw)
    if name == "owner_ids":
        return owner_ids(th, tw)
    if name == "spiral_hole":
        return spiral_hole(th, tw)
    raise KeyError(name)
