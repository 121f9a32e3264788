"""Connected components of u8 instance index maps on the device: `index_components` and `filter_components`, the bindings of
s2d_index_components_i32 / s2d_index_filter_components_u8 (csrc/index_components.hip).  `s2d_amd.ops` re-exports them beside
`infer_index` and `paint_frames`, whose maps they clean; they are defined here, not in ops.py, for the reason index_map.py gives: the
recorded-entry-point tables of tests/test_gpu_forward_c4.py and tests/test_gpu_eval_720p.py list every function DEFINED in ops.py.
Their rows are tests/test_gpu_index_components.py.

The rule (one definition: kernel, tests/index_components_refs.py, INTEGRATION.md "Stage-1 frame masks").  index u8 [N,H,W]: 0 is
background, any other byte an instance id.  A component is a maximal set of pixels of one id connected under 4- or 8-connectivity;
its label is 1 + the flat index y*W + x of its first pixel in raster order, its area the number of its pixels.  The filter keeps a
component iff area >= min_area and, with keep_largest, it is the largest of its (image, id), among equal areas the one with the
lowest first pixel; the pixels of every other component become 0 (and black in `rgb`)."""
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

