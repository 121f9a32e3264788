"""Host references of the connected-component ops (s2d_amd/index_components.py) and the constructed cases of their tests.

An index map is u8 [N,H,W]: 0 background, any other byte an instance id.  A component is a maximal set of pixels of one id
connected under 4- or 8-connectivity; its label is 1 + the flat index of its first pixel in raster order.  `ref_components` labels
with scipy.ndimage.label per id and renames; `ref_filter` is the cleanup rule: keep iff area >= min_area and (keep_largest) the
component is the largest of its (image, id), equal areas to the lower first pixel.  The case builders take the kernel's tile
(th, tw) as arguments, so that their borders and corners sit where the kernel's do."""
import numpy as np
from scipy import ndimage


def structure(conn):
    if conn not in (4, 8):
        raise ValueError(f"connectivity {conn}: 4 or 8")
    return ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)


def ref_components(index, conn):
    """u8 [N,H,W] -> (labels int32 [N,H,W], area int32 [N,H,W]): area holds a component's pixel count at its first pixel"""
    index = np.asarray(index)
    assert index.dtype == np.uint8 and index.ndim == 3
    N, H, W = index.shape
    labels, area = np.zeros((N, H * W), np.int32), np.zeros((N, H * W), np.int32)
    for n in range(N):
        for v in np.unique(index[n]):
            if v == 0:
                continue
            lab, k = ndimage.label(index[n] == v, structure(conn))
            flat = lab.reshape(-1)
            pos = np.flatnonzero(flat)
            first = np.full(k + 1, H * W, np.int64)
            np.minimum.at(first, flat[pos], pos)
            labels[n, pos] = first[flat[pos]] + 1
            area[n, first[1:]] = np.bincount(flat, minlength=k + 1)[1:]
    return labels.reshape(N, H, W), area.reshape(N, H, W)


def count_components(index, conn):
    return int((ref_components(index, conn)[1] > 0).sum())


def ref_filter(index, min_area, keep_largest, conn, rgb=None):
    """-> (out u8 [N,H,W], removed int32 [N], rgb after the call or None)"""
    index = np.asarray(index)
    labels, area = ref_components(index, conn)
    N = index.shape[0]
    out, removed = index.copy(), np.zeros(N, np.int32)
    rgb = None if rgb is None else np.array(rgb, copy=True)
    for n in range(N):
        roots = np.flatnonzero(area[n])                               # ascending first pixels
        ids, a = index[n].reshape(-1)[roots], area[n].reshape(-1)[roots]
        keep = a >= min_area
        if keep_largest:
            for v in np.unique(ids):
                sel = np.flatnonzero(ids == v)
                best = sel[np.lexsort((roots[sel], -a[sel].astype(np.int64)))[0]]      # largest area, then lowest first pixel
                lose = np.ones(len(roots), bool)
                lose[best] = False
                keep &= ~((ids == v) & lose)
        gone = (index[n] != 0) & ~np.isin(labels[n], roots[keep] + 1)
        out[n][gone] = 0
        removed[n] = gone.sum()
        if rgb is not None:
            rgb[n][gone] = 0
    return out, removed, rgb


def make_rgb(index, seed=0):
    """u8 [N,H,W,3]: 7 on background (a sentinel a stray store would destroy), 1..255 on the instances' pixels"""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(1, 256, index.shape + (3,), dtype=np.uint8)
    rgb[np.asarray(index) == 0] = 7
    return rgb


# ---------------------------------------------------------------------------------------------------------------- constructed cases
def frame_shape(th, tw):
    return 3 * th + 1, 3 * tw + 1


def spiral(H, W, value=1):
    """a one-pixel-wide spiral from the corner (0, 0) round the outer border to the centre, its arms one empty pixel apart: ONE
    component under both connectivities, and the longest chain of dependencies across tiles a map of this size has"""
    m = np.zeros((H, W), np.uint8)
    y = x = d = 0
    m[0, 0] = value
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or m[yy, xx] == 0

    def can(d):
        dy, dx = steps[d]
        return 0 <= y + dy < H and 0 <= x + dx < W and m[y + dy, x + dx] == 0 and free(y + 2 * dy, x + 2 * dx)

    while True:
        if not can(d):
            d = (d + 1) % 4
            if not can(d):
                break
        y, x = y + steps[d][0], x + steps[d][1]
        m[y, x] = value
    return m[None]


def u_shape(th, tw, flip=None, value=3):
    """two vertical arms that start in the tiles (0, 0) and (0, 2) -- the right one higher, so it owns the first pixel -- and meet only
    through a bar that crosses tile (2, 1); flip "lr" / "ud" mirrors the map"""
    H, W = frame_shape(th, tw)
    m = np.zeros((H, W), np.uint8)
    cl, cr, yb = tw // 2, 2 * tw + tw // 2, 2 * th + th // 2
    m[3:yb + 1, cl] = value
    m[0:yb + 1, cr] = value
    m[yb, cl:cr + 1] = value
    if flip == "lr":
        m = m[:, ::-1]
    elif flip == "ud":
        m = m[::-1]
    elif flip is not None:
        raise ValueError(flip)
    return np.ascontiguousarray(m)[None]


def corner_pair(th, tw, anti=False, value=2):
    """two pixels that touch only diagonally at the four-tile corner: (th-1, tw-1) / (th, tw), or (th-1, tw) / (th, tw-1)"""
    H, W = frame_shape(th, tw)
    m = np.zeros((H, W), np.uint8)
    if anti:
        m[th - 1, tw] = m[th, tw - 1] = value
    else:
        m[th - 1, tw - 1] = m[th, tw] = value
    return m[None]


def two_ids_along_border(th, tw):
    """id 1 left of the first vertical tile border, id 2 right of it, over the whole height; below the second horizontal border the
    ids are 3 and 4: four components that must not join"""
    H, W = frame_shape(th, tw)
    m = np.zeros((H, W), np.uint8)
    m[:2 * th, :tw], m[:2 * th, tw:] = 1, 2
    m[2 * th:, :tw], m[2 * th:, tw:] = 3, 4
    return m[None]


def full_frame(H, W, value=255):
    return np.full((1, H, W), value, np.uint8)


def checkerboard(H, W, a=9, b=0):
    """a on the squares with even y + x, b on the others"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, a, b).astype(np.uint8)[None]


def tie_case(th, tw, value=5):
    """one id with two components of 9 pixels (the first in tile (0, 0), the second across a tile corner), a smaller one of 4, and a
    second id with components of 6 and 2"""
    H, W = frame_shape(th, tw)
    m = np.zeros((H, W), np.uint8)
    m[2:5, 2:5] = value
    m[th - 1:th + 2, tw - 1:tw + 2] = value
    m[2 * th + 3:2 * th + 5, 7:9] = value
    m[8:10, tw + 3:tw + 6] = 254
    m[H - 1, W - 2:W] = 254
    return m[None]


def striped_random(N, H, W, ids=(1, 254, 255), density=0.59, seed=0, stripe=37):
    """sites set with probability `density` (near the 4-connected percolation threshold: ragged components that span tiles), the id
    of a site by diagonal stripes `stripe` pixels wide, so that every id is dense where it lives"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    which = np.asarray(ids, np.uint8)[((yy + xx) // stripe) % len(ids)]
    return np.where(rng.random((N, H, W)) < density, which[None], 0).astype(np.uint8)


GEOMETRY_CASES = ("spiral", "u", "u_lr", "u_ud", "corner", "corner_anti", "two_ids_border", "full", "checker_one", "checker_two")


def geometry_case(name, th, tw):
    H, W = frame_shape(th, tw)
    if name == "spiral":
        return spiral(H, W)
    if name in ("u", "u_lr", "u_ud"):
        return u_shape(th, tw, {"u": None, "u_lr": "lr", "u_ud": "ud"}[name])
    if name in ("corner", "corner_anti"):
        return corner_pair(th, tw, name == "corner_anti")
    if name == "two_ids_border":
        return two_ids_along_border(th, tw)
    if name == "full":
        return full_frame(H, W)
    if name == "checker_one":
        return checkerboard(H, W, 9, 0)
    if name == "checker_two":
        return checkerboard(H, W, 9, 200)
    raise KeyError(name)
