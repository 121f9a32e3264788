"""Connected components of u8 instance index maps on the device: `index_components`, `filter_components` and `fill_index_holes`, the
bindings of s2d_index_components_i32 / s2d_index_filter_components_u8 / s2d_index_fill_holes_u8 (csrc/index_components.hip; the
hole-filling rule stands above `fill_index_holes`, its rows are tests/test_gpu_index_fill.py).  `s2d_amd.ops` re-exports them beside
`infer_index` and `paint_frames`, whose maps they clean; they are defined here, not in ops.py, for the reason index_map.py gives: the
recorded-entry-point tables of tests/test_gpu_forward_c4.py and tests/test_gpu_eval_720p.py list every function DEFINED in ops.py.
Their rows are tests/test_gpu_index_components.py.

The rule (one definition: kernel, tests/index_components_refs.py, INTEGRATION.md "Stage-1 frame masks").  index u8 [N,H,W]: 0 is
background, any other byte an instance id.  A component is a maximal set of pixels of one id connected under 4- or 8-connectivity;
its label is 1 + the flat index y*W + x of its first pixel in raster order, its area the number of its pixels.  The filter keeps a
component iff area >= min_area and, with keep_largest, it is the largest of its (image, id), among equal areas the one with the
lowest first pixel; the pixels of every other component become 0 (and black in `rgb`)."""
import numbers

import torch

CONNECTIVITIES = (4, 8)
COMPONENT_KEYS = ("min_component_area", "keep_largest", "component_connectivity")   # of the paint / index_map option dicts


def component_tile():
    """-> (th, tw): the tile a workgroup labels locally (the tests build their border cases from it)"""
    import ctypes
    from ._lib import lib
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    lib().call("s2d_index_components_tile", ctypes.addressof(th), ctypes.addressof(tw))
    return th.value, tw.value


def _check(name, index, connectivity):
    from . import ops
    ops._chk(index, torch.uint8)
    if index.dim() != 3 or min(index.shape) < 1 or index.shape[1] * index.shape[2] >= 2 ** 31 - 1:
        raise ValueError(f"{name} needs a u8 index map [N, H, W] with N, H, W >= 1 and H*W < 2^31 - 1, got {tuple(index.shape)}")
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"{name}: connectivity {connectivity!r}: 4 or 8")
    return tuple(index.shape)


def _workspace(index):
    from ._lib import lib
    N, H, W = index.shape
    return torch.empty((lib().call("s2d_index_components_workspace_bytes", N, H, W),), device=index.device, dtype=torch.uint8)


def index_components(index, connectivity=8, want_area=True, workspace=None):
    """index u8 [N,H,W] on the device -> (labels int32 [N,H,W], area int32 [N,H,W] or None): labels 0 on background, else 1 + the flat
    index of the component's first pixel; area[n] holds at a component's first pixel its pixel count and 0 everywhere else"""
    from . import ops
    from ._lib import lib
    N, H, W = _check("index_components", index, connectivity)
    ws = _workspace(index) if workspace is None else workspace
    labels = torch.empty((N, H, W), device=index.device, dtype=torch.int32)
    area = torch.empty((N, H, W), device=index.device, dtype=torch.int32) if want_area else None
    lib().call("s2d_index_components_i32", index, N, H, W, int(connectivity), labels, area, ws, ops._stream())
    return labels, area


def filter_components(index, min_area=0, keep_largest=False, connectivity=8, rgb=None, out=None):
    """label and filter in one call -> (out u8 [N,H,W], removed int32 [N]): index where the pixel's component is kept (module
    docstring), else 0; rgb u8 [N,H,W,3], if given, is changed in place -- the three bytes of every removed pixel become 0, no other
    byte is touched.  `out` may be given, and may be `index` itself."""
    from . import ops
    from ._lib import lib
    N, H, W = _check("filter_components", index, connectivity)
    if int(min_area) < 0:
        raise ValueError(f"filter_components: min_area = {min_area}: at least 0")
    if rgb is not None:
        ops._chk(rgb, torch.uint8)
        if tuple(rgb.shape) != (N, H, W, 3):
            raise ValueError(f"filter_components: rgb must be u8 [{N}, {H}, {W}, 3], got {tuple(rgb.shape)}")
    if out is None:
        out = torch.empty((N, H, W), device=index.device, dtype=torch.uint8)
    else:
        ops._chk(out, torch.uint8)
        if tuple(out.shape) != (N, H, W):
            raise ValueError(f"filter_components: out must be u8 [{N}, {H}, {W}], got {tuple(out.shape)}")
    ws = _workspace(index)
    labels, area = index_components(index, connectivity, True, ws)
    removed = torch.empty((N,), device=index.device, dtype=torch.int32)
    lib().call("s2d_index_filter_components_u8", index, labels, area, N, H, W, int(min_area), int(bool(keep_largest)), out, rgb, removed,
               ws, ops._stream())
    return out, removed


def component_options(opts):
    """the cleanup keys of a paint / index_map option dict -> (min_component_area, keep_largest, component_connectivity) with the
    defaults (0, False, 8); a negative area and a connectivity other than 4 or 8 are refused.  (0, False, *) is "off": the drivers
    launch nothing for it."""
    min_area, largest, conn = opts.get("min_component_area", 0), opts.get("keep_largest", False), opts.get("component_connectivity", 8)
    if isinstance(min_area, bool) or int(min_area) != min_area or int(min_area) < 0:
        raise ValueError(f"min_component_area = {min_area!r}: an integer, at least 0")
    if conn not in CONNECTIVITIES:
        raise ValueError(f"component_connectivity = {conn!r}: 4 or 8")
    return int(min_area), bool(largest), int(conn)


# ------------------------------------------------------------------------------------------------------------------- hole filling
# The rule (one definition: kernel, include/s2d_hip.h, tests/index_fill_refs.py).  `connectivity` is the instances'; the zero pixels
# of an image are labelled under the complementary one c' (8 -> 4, 4 -> 8).  A zero component is a hole iff none of its pixels lies
# on the frame border; its owners are the ids of the non-zero c'-neighbours of its pixels.  A hole is filled iff its area <=
# max_hole_area and it has exactly one owner k: its pixels become k (and colors[k-1] in `rgb`).  Holes with two or more owners stay,
# and so does, with `rgb`, a hole whose owner has no row in `colors`.  Nothing but zero pixels ever changes.
FILL_KEYS = ("fill_holes",)                                           # of the paint / index_map option dicts
FILL_ALL = 2 ** 31 - 1


def fill_index_holes(index, max_hole_area, connectivity=8, rgb=None, colors=None, out=None):
    """-> (out u8 [N,H,W], filled int32 [N]): index with every one-owner hole of at most max_hole_area pixels (an int >= 1, or "all")
    set to its owner's id; rgb u8 [N,H,W,3], if given, is changed in place -- a filled pixel takes colors[owner - 1] (colors a CUDA u8
    [K,3] tensor, required with rgb), no other byte is touched.  `out` may be given, and may be `index` itself."""
    from . import ops
    from ._lib import lib
    N, H, W = _check("fill_index_holes", index, connectivity)
    if max_hole_area == "all":
        max_hole_area = FILL_ALL
    if isinstance(max_hole_area, bool) or not isinstance(max_hole_area, int) or not 1 <= max_hole_area <= FILL_ALL:
        raise ValueError(f"fill_index_holes: max_hole_area = {max_hole_area!r}: an integer >= 1 or 'all'")
    n_colors = 0
    if rgb is not None:
        ops._chk(rgb, torch.uint8)
        if tuple(rgb.shape) != (N, H, W, 3):
            raise ValueError(f"fill_index_holes: rgb must be u8 [{N}, {H}, {W}, 3], got {tuple(rgb.shape)}")
        if colors is None:
            raise ValueError("fill_index_holes: rgb needs the colour table it was painted with (colors u8 [K, 3])")
        ops._chk(colors, torch.uint8)
        if colors.dim() != 2 or colors.shape[1] != 3 or not 1 <= colors.shape[0] <= 255:
            raise ValueError(f"fill_index_holes: colors must be u8 [K, 3] with 1 <= K <= 255, got {tuple(colors.shape)}")
        n_colors = int(colors.shape[0])
    else:
        colors = None
    if out is None:
        out = torch.empty((N, H, W), device=index.device, dtype=torch.uint8)
    else:
        ops._chk(out, torch.uint8)
        if tuple(out.shape) != (N, H, W):
            raise ValueError(f"fill_index_holes: out must be u8 [{N}, {H}, {W}], got {tuple(out.shape)}")
    ws = torch.empty((lib().call("s2d_index_fill_holes_workspace_bytes", N, H, W),), device=index.device, dtype=torch.uint8)
    filled = torch.empty((N,), device=index.device, dtype=torch.int32)
    lib().call("s2d_index_fill_holes_u8", index, N, H, W, int(connectivity), int(max_hole_area), out, rgb, colors, n_colors, filled, ws,
               ops._stream())
    return out, filled


def fill_holes_argument(text):
    """the argparse type of the drivers' --fill-holes N|all (as clean_annotations parses its own) -> 0, N or 2^31 - 1"""
    if str(text).lower() == "all":
        return FILL_ALL
    v = int(text)
    if not 0 <= v <= FILL_ALL:
        raise ValueError(f"--fill-holes {text}: a pixel count >= 0, or `all`")
    return v


def fill_options(opts):
    """the hole-filling key of a paint / index_map option dict -> max_hole_area: "fill_holes" 0 (the default: off; the drivers launch
    nothing for it), a positive int, or "all" -> 0, N or 2^31 - 1; bools, negatives and non-integers are refused"""
    v = opts.get("fill_holes", 0)
    if v == "all":
        return FILL_ALL
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) <= FILL_ALL:
        raise ValueError(f"fill_holes = {v!r}: 0 (off), a positive integer or 'all'")
    return int(v)

