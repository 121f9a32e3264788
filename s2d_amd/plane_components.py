"""Connected components and cleanup of a CHUNK of bit planes of different sizes on the device: `plane_components` and `clean_planes`,
the bindings of s2d_plane_components_ragged / s2d_plane_clean_ragged (csrc/plane_components.hip).  The planes are the flat buffer
and the plane table of rle_ragged.decode_ragged: the overlapping masks of an annotation file, which the index-map kernels
(index_components.py) cannot label.  `s2d_amd.ops` re-exports the functions; they are defined here, not in ops.py, for the reason
index_components.py gives.  Their rows are tests/test_gpu_plane_components.py.

The rule (one definition: kernel, tests/plane_components_refs.py, INTEGRATION.md "Cleaning annotation files").  It is this project's
own: the reference cleans nothing.  A plane is H x W pixels, pixel i = y*W + x in word i/32, bit i%32 of its words; padding bits of
the last word are ignored on input and 0 on output.  A component is a maximal set of pixels of one value connected under 4- or
8-connectivity; its label is 1 + the flat index of its first pixel in raster order, its area the number of its pixels.  The cleanup
of a plane is fill(filter(plane)) -- in an annotation file, of the plane smoothed first by the opening and closing of plane_morph.py
(the rule is stated there), when those are asked for:
  filter (min_area > 0 or keep_largest)  a component of set pixels is kept iff area >= min_area and, with keep_largest, it is the
         largest of its plane, among equal areas the one with the lowest first pixel; every other set pixel becomes 0;
  fill   (max_hole_area > 0)  the ZERO pixels of the filtered plane are labelled under the complementary connectivity (8 -> 4,
         4 -> 8); a component with no pixel in row 0, row H-1, column 0 or column W-1 is a hole, and a hole of at most max_hole_area
         pixels becomes set.  With FILL_ALL this is scipy.ndimage.binary_fill_holes.
The order matters: an island inside a ring is removed by min_area and then the whole interior is filled."""
from collections import Counter

import numpy as np
import torch

from .index_components import CONNECTIVITIES, component_options

FILL_ALL = 2 ** 31 - 1          # max_hole_area: every hole
LIB_CALLS = Counter()          # library calls made by this module, by export name


def _lib_call(name, *args):
    from ._lib import lib
    LIB_CALLS[name] += 1
    return lib().call(name, *args)


def component_tile():
    """-> (th, tw): the tile a workgroup labels locally (the tests build their border cases from it)"""
    import ctypes
    from ._lib import lib
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    lib().call("s2d_plane_components_tile", ctypes.addressof(th), ctypes.addressof(tw))
    return th.value, tw.value


def plane_tiles(plane_table):
    """plane int64 numpy [P, 4] = {word0, H, W, 0} -> tiles int32 numpy [n_tiles, 3] = {plane, tile row, tile column}: every tile of
    every plane once, plane after plane, in raster order"""
    th, tw = component_tile()
    plane = np.asarray(plane_table, np.int64).reshape(-1, 4)
    ny, nx = (plane[:, 1] + th - 1) // th, (plane[:, 2] + tw - 1) // tw
    n = ny * nx
    if n.sum() >= 2 ** 31:
        raise ValueError(f"{int(n.sum())} tiles in one chunk: fewer than 2^31")
    f = np.repeat(np.arange(len(plane)), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    nxr = np.repeat(nx, n)
    return np.stack([f, k // np.maximum(nxr, 1), k % np.maximum(nxr, 1)], 1).astype(np.int32).reshape(-1, 3)


def component_hole_options(opts):
    """component_options plus the hole rule: -> (min_component_area, keep_largest, component_connectivity, max_hole_area) with the
    defaults (0, False, 8, 0); max_hole_area is an integer >= 0, 0 is off"""
    min_area, largest, conn = component_options(opts)
    hole = opts.get("max_hole_area", 0)
    if isinstance(hole, bool) or int(hole) != hole or not 0 <= int(hole) <= FILL_ALL:
        raise ValueError(f"max_hole_area = {hole!r}: an integer, at least 0 and at most 2^31 - 1")
    return min_area, largest, conn, int(hole)


def check_chunk(name, bits, plane_table):
    """a flat buffer and its plane table (numpy, or the device tensor decode_ragged returns), checked -> (plane numpy [P, 4], plane on
    the device): shared by the ops of this module and of plane_morph.py"""
    from . import ops
    if bits.dtype != torch.int32 or bits.dim() != 1:
        raise ValueError(f"{name} needs the flat int32 buffer of a ragged chunk, got {bits.dtype} {tuple(bits.shape)}")
    ops._chk(bits, torch.int32)
    if isinstance(plane_table, torch.Tensor):
        plane_dev, plane = plane_table, plane_table.cpu().numpy()
        if plane_dev.dtype != torch.int64 or not plane_dev.is_contiguous() or plane_dev.device != bits.device:
            raise ValueError(f"{name}: the plane table must be a contiguous int64 tensor on the device of bits")
    else:
        plane = np.ascontiguousarray(plane_table, np.int64)
        plane_dev = None
    if plane.ndim != 2 or plane.shape[1] != 4:
        raise ValueError(f"{name}: the plane table must be int64 [P, 4], got {plane.shape}")
    H, W = plane[:, 1], plane[:, 2]
    if len(plane) and (H.min() < 1 or W.min() < 1 or (H * W).max() >= 2 ** 31 or plane[:, 0].min() < 0
                       or (plane[:, 0] + (H * W + 31) // 32).max() > bits.numel()):
        raise ValueError(f"{name}: a plane of the table does not fit the buffer of {bits.numel()} words")
    if plane_dev is None:
        plane_dev = torch.from_numpy(plane).to(bits.device)
    return plane, plane_dev


def _chunk(name, bits, plane_table):
    """-> (plane numpy [P, 4], plane on the device, tiles on the device, n_tiles) for a flat buffer and its table, checked"""
    plane, plane_dev = check_chunk(name, bits, plane_table)
    tiles = plane_tiles(plane)
    tiles_dev = torch.from_numpy(tiles).to(bits.device) if len(tiles) else None
    return plane, plane_dev, tiles_dev, len(tiles)


def _workspace(bits, P):
    from ._lib import lib
    return torch.empty((lib().call("s2d_plane_components_workspace_bytes", bits.numel(), P),), device=bits.device, dtype=torch.uint8)


def plane_components(bits, plane_table, value=1, connectivity=8, want_area=True):
    """bits int32 CUDA [words] and plane_table int64 [P, 4] = {word0, H, W, 0} (numpy, or the device tensor decode_ragged returns) ->
    (labels int32 CUDA [32 * words], area int32 CUDA [32 * words] or None).  Pixel i of plane p is element 32 * word0 + i: labels 0
    where the bit is not `value`, else 1 + the flat index of the component's first pixel in its plane; area holds at a component's
    first pixel its pixel count and 0 elsewhere.  Positions of no pixel hold 0."""
    from . import ops
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"plane_components: connectivity {connectivity!r}: 4 or 8")
    if value not in (0, 1):
        raise ValueError(f"plane_components: value {value!r}: 0 or 1")
    plane, plane_dev, tiles, n_tiles = _chunk("plane_components", bits, plane_table)
    labels = torch.empty((32 * bits.numel(),), device=bits.device, dtype=torch.int32)
    area = torch.empty((32 * bits.numel(),), device=bits.device, dtype=torch.int32) if want_area else None
    _lib_call("s2d_plane_components_ragged", bits, plane_dev, len(plane), bits.numel(), int(value), int(connectivity), tiles, n_tiles,
              labels, area, _workspace(bits, len(plane)), ops._stream())
    return labels, area


def clean_planes(bits, plane_table, min_area=0, keep_largest=False, max_hole_area=0, connectivity=8, out=None):
    """fill(filter(plane)) for every plane of the chunk (module docstring) -> (out int32 CUDA [words], removed int32 CUDA [P], filled
    int32 CUDA [P]): the pixels cleared and set per plane.  `out` may be given, and may be `bits` itself.  With every option off the
    planes are copied with their padding bits zeroed."""
    from . import ops
    min_area, keep_largest, connectivity, max_hole_area = component_hole_options(
        {"min_component_area": min_area, "keep_largest": keep_largest, "component_connectivity": connectivity, "max_hole_area": max_hole_area})
    plane, plane_dev, tiles, n_tiles = _chunk("clean_planes", bits, plane_table)
    if out is None:
        out = torch.zeros_like(bits)
    else:
        ops._chk(out, torch.int32)
        if out.shape != bits.shape or out.device != bits.device:
            raise ValueError(f"clean_planes: out must be int32 [{bits.numel()}] on the device of bits, got {tuple(out.shape)}")
    P = len(plane)
    removed = torch.zeros((P,), device=bits.device, dtype=torch.int32)
    filled = torch.zeros((P,), device=bits.device, dtype=torch.int32)
    _lib_call("s2d_plane_clean_ragged", bits, plane_dev, P, bits.numel(), connectivity, min_area, int(keep_largest), max_hole_area, tiles,
              n_tiles, out, removed, filled, _workspace(bits, P), ops._stream())
    return out, removed, filled
