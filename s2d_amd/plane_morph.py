"""Binary morphology of a CHUNK of bit planes of different sizes on the device, every plane at a radius of its own: `morph_planes`,
the binding of s2d_plane_morph_ragged (csrc/plane_morph.hip).  The planes are the flat buffer and the plane table of
rle_ragged.decode_ragged, as for plane_components.py.  `s2d_amd.ops` re-exports the functions; they are defined here, not in ops.py,
for the reason index_components.py gives.  Their rows are tests/test_gpu_plane_morph.py.

The rule (one definition: kernel, tests/plane_morph_refs.py, INTEGRATION.md "Cleaning annotation files").  It is this project's own:
the reference cleans nothing.  The structuring element B(r, shape), 1 <= r <= 64, is
  disk    {dx^2 + dy^2 <= r^2}, the disk of the DAVIS boundary dilation (s2d_disk_dilate_bits_u32),
  square  {|dx|, |dy| <= r}.
Per plane of H x W pixels:
  dilate(X)  pixel p is set iff some set pixel of X lies in p + B; nothing outside the image is set;
  erode(X)   pixel p is set iff every pixel of p + B that lies INSIDE the image is set: pixels outside the image count as set;
  open(X)  = dilate(erode(X)),     close(X) = erode(dilate(X)).
In scipy: binary_erosion(X, B, border_value=1) and binary_dilation(X, B, border_value=0) -- NOT binary_opening / binary_closing,
whose zero-border erosion takes a band of width r off every mask that touches the image edge.  With this border open(X) <= X <=
close(X), close(X) = ~open(~X), erode(X) = ~dilate(~X) (complements inside the image: the kernel has one body), a full plane stays
full, an empty one empty, a rectangle at the image edge keeps its edge corners and a 1-pixel strip along the edge goes.  r = 0 copies
the plane with its padding zeroed.  Disks do not compose, so a radius over 64 is refused rather than chained.

The annotation cleanup (clean_annotations.py) is fill(filter(close(open(plane)))): smoothing first, opening before closing, each
skipped at radius 0, then the filter / fill of plane_components.py on the smoothed plane."""
from collections import Counter

import numpy as np
import torch

OPS = ("erode", "dilate", "open", "close")      # the op codes of s2d_plane_morph_ragged
SHAPES = ("disk", "square")                     # its shape codes
MAX_RADIUS = 64
LIB_CALLS = Counter()          # library calls made by this module, by export name
_TILE = {}
_LDS = {}


def _lib_call(name, *args):
    from ._lib import lib
    LIB_CALLS[name] += 1
    return lib().call(name, *args)


def morph_tile(r):
    """-> (rows, words): the tile a workgroup handles at radius r -- at most `rows` rows (a plane's rows are cut evenly into
    ceil(H / rows) tile rows) of at most `words` row-aligned 32-pixel words (the tests build their tile-crossing planes from it)"""
    import ctypes
    from ._lib import lib
    r = int(r)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"morph_tile: radius {r}: 0 .. {MAX_RADIUS}")
    if r not in _TILE:
        rows, words = ctypes.c_int(0), ctypes.c_int(0)
        lib().call("s2d_plane_morph_tile", r, ctypes.addressof(rows), ctypes.addressof(words))
        _TILE[r] = rows.value, words.value
    return _TILE[r]


def morph_tiles(plane_table, radius):
    """plane int64 numpy [P, 4] and radius int [P] -> tiles int32 numpy [n_tiles, 3] = {plane, tile row, tile column}: every tile of
    every plane with a radius > 0 once, plane after plane, in raster order"""
    plane = np.asarray(plane_table, np.int64).reshape(-1, 4)
    radius = np.asarray(radius, np.int64).reshape(-1)
    rows = np.array([morph_tile(r)[0] for r in range(MAX_RADIUS + 1)], np.int64)[radius]
    words = morph_tile(0)[1]
    ny, nx = (plane[:, 1] + rows - 1) // rows, ((plane[:, 2] + 31) // 32 + words - 1) // words
    n = np.where(radius > 0, ny * nx, 0)
    if n.sum() >= 2 ** 31:
        raise ValueError(f"{int(n.sum())} tiles in one chunk: fewer than 2^31")
    f = np.repeat(np.arange(len(plane)), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    nxr = np.repeat(nx, n)
    return np.stack([f, k // np.maximum(nxr, 1), k % np.maximum(nxr, 1)], 1).astype(np.int32).reshape(-1, 3)


def morph_lds_words(plane_table, radius):
    """plane int64 numpy [P, 4] and radius int [P] -> the LDS words of a launch over them: the need of the largest tile of any plane
    (s2d_plane_morph_lds_words, once per distinct (radius, tile rows, tile words): a plane's largest tile is th = ceil(H / ceil(H /
    rows(r))) rows of tw = min(S, words) words, and needs what a th x 32 tw plane of one tile needs); 0 when no plane has a radius > 0"""
    from ._lib import lib
    plane = np.asarray(plane_table, np.int64).reshape(-1, 4)
    radius = np.asarray(radius, np.int64).reshape(-1)
    on = radius > 0
    if not on.any():
        return 0
    r, H, S = radius[on], plane[on, 1], (plane[on, 2] + 31) // 32
    rows = np.array([morph_tile(k)[0] for k in range(MAX_RADIUS + 1)], np.int64)[r]
    nty = (H + rows - 1) // rows
    th, tw = (H + nty - 1) // nty, np.minimum(S, morph_tile(0)[1])
    need = 0
    for key in np.unique((r << 16) | (th << 8) | tw).tolist():
        if key not in _LDS:
            _LDS[key] = int(lib().call("s2d_plane_morph_lds_words", key >> 16, (key >> 8) & 255, 32 * (key & 255)))
        need = max(need, _LDS[key])
    return need


def smooth_radius(spec, H, W, name=None):
    """a radius given as an int N (pixels) or a string "N" / "X%" -> pixels for an H x W image.  "X%" is X percent of the image
    diagonal through the ONE rule of the Boundary IoU band, ytvis_eval.boundary_dilation(H, W, X / 100) (at least 1 for X > 0) --
    the only definition: coco_eval's Boundary AP imports the same function, so "the rule of coco_eval" is this one.  A
    result over 64 raises a ValueError that names the image or video."""
    r = parse_radius(spec)
    if isinstance(r, float):
        from .ytvis_eval import boundary_dilation
        r = boundary_dilation(int(H), int(W), r / 100.0) if r > 0 else 0
    if r > MAX_RADIUS:
        raise ValueError(f"smoothing radius {spec!r} is {r} pixels for the {H} x {W} image"
                         f"{'' if name is None else ' ' + str(name)}: at most {MAX_RADIUS} (disks do not compose: there is no chained pass)")
    return int(r)


def parse_radius(spec):
    """the grammar of a radius: an int N >= 0 or a string "N" (pixels, -> int), or "X%" with X >= 0 (-> float X); else ValueError"""
    if isinstance(spec, bool):
        raise ValueError(f"radius {spec!r}: N pixels or 'X%' of the image diagonal")
    if isinstance(spec, (int, np.integer)):
        v = int(spec)
    else:
        text = str(spec).strip() if isinstance(spec, str) else None
        try:
            if text is None:
                raise ValueError
            if text.endswith("%"):
                x = float(text[:-1])
                if not (0 <= x < float("inf")):
                    raise ValueError
                return x
            v = int(text)
        except ValueError:
            raise ValueError(f"radius {spec!r}: N pixels or 'X%' of the image diagonal") from None
    if v < 0:
        raise ValueError(f"radius {spec!r}: at least 0")
    return v


def morph_planes(bits, plane_table, op, radius, shape="disk", out=None):
    """op ("erode", "dilate", "open", "close") of every plane of the chunk under B(radius, shape) (module docstring) -> (out int32 CUDA
    [words], cleared int32 CUDA [P], set int32 CUDA [P]): the pixels the op cleared and set per plane.  radius: an int, or an int array
    / tensor [P], 0 .. 64 (0: the plane is copied with its padding zeroed).  `out` may be given; it must not be `bits`: a tile reads its
    neighbours' halos.  Words of `out` between the planes are not written."""
    from . import ops
    from .plane_components import check_chunk
    if op not in OPS:
        raise ValueError(f"morph_planes: op {op!r}: one of {OPS}")
    if shape not in SHAPES:
        raise ValueError(f"morph_planes: shape {shape!r}: one of {SHAPES}")
    if not isinstance(bits, torch.Tensor) or not bits.is_cuda or not bits.is_contiguous():
        raise ValueError("morph_planes needs the flat int32 buffer of a ragged chunk as a contiguous CUDA tensor")
    if bits.dtype != torch.int32 or bits.dim() != 1:
        raise ValueError(f"morph_planes needs the flat int32 buffer of a ragged chunk, got {bits.dtype} {tuple(bits.shape)}")
    P = len(plane_table)
    if isinstance(radius, torch.Tensor):
        radius = radius.cpu().numpy()
    rad = np.asarray(radius)
    if rad.dtype == bool or not np.issubdtype(rad.dtype, np.integer) or rad.ndim > 1 or (rad.ndim == 1 and len(rad) != P):
        raise ValueError(f"morph_planes: radius must be an int or an int array [{P}], got {rad.dtype} {rad.shape}")
    rad = np.ascontiguousarray(np.broadcast_to(rad.astype(np.int64), (P,)))
    if P and (rad.min() < 0 or rad.max() > MAX_RADIUS):
        raise ValueError(f"morph_planes: radius {int(rad.min())} .. {int(rad.max())}: 0 .. {MAX_RADIUS}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or not out.is_contiguous() or out.dtype != torch.int32 \
                or out.shape != bits.shape or out.device != bits.device:
            raise ValueError(f"morph_planes: out must be a contiguous int32 [{bits.numel()}] tensor on the device of bits")
        lo, hi = out.data_ptr(), out.data_ptr() + 4 * out.numel()
        if lo < bits.data_ptr() + 4 * bits.numel() and bits.data_ptr() < hi:
            raise ValueError("morph_planes: out must not alias bits (a tile reads its neighbours' halos)")
    plane, plane_dev = check_chunk("morph_planes", bits, plane_table)
    tiles = morph_tiles(plane, rad)
    tiles_dev = torch.from_numpy(tiles).to(bits.device) if len(tiles) else None
    rad_dev = torch.from_numpy(rad.astype(np.int32)).to(bits.device)
    if out is None:
        out = torch.zeros_like(bits)
    cleared = torch.zeros((P,), device=bits.device, dtype=torch.int32)
    set_ = torch.zeros((P,), device=bits.device, dtype=torch.int32)
    from ._lib import lib
    ws = torch.empty((lib().call("s2d_plane_morph_workspace_bytes", bits.numel(), P),), device=bits.device, dtype=torch.uint8)
    _lib_call("s2d_plane_morph_ragged", bits, plane_dev, P, bits.numel(), OPS.index(op), SHAPES.index(shape), rad_dev, tiles_dev,
              len(tiles), morph_lds_words(plane, rad), out, cleared, set_, ws, ops._stream())
    return out, cleared, set_


def plane_diff_counts(a, b, plane_table):
    """two flat buffers of one chunk -> (cleared int32 CUDA [P], set int32 CUDA [P]) = popcount(a & ~b), popcount(b & ~a) over the pixels
    of every plane (s2d_plane_diff_counts_ragged): how the annotation cleanup counts a decoded plane against its smoothed one"""
    from . import ops
    from .plane_components import check_chunk
    ops._chk(a, torch.int32)
    ops._chk(b, torch.int32)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"plane_diff_counts: two buffers of one chunk, got {tuple(a.shape)} and {tuple(b.shape)}")
    plane, plane_dev = check_chunk("plane_diff_counts", a, plane_table)
    cleared = torch.zeros((len(plane),), device=a.device, dtype=torch.int32)
    set_ = torch.zeros((len(plane),), device=a.device, dtype=torch.int32)
    _lib_call("s2d_plane_diff_counts_ragged", a, b, plane_dev, len(plane), a.numel(), cleared, set_, ops._stream())
    return cleared, set_
