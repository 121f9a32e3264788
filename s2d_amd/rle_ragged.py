"""COCO RLE <-> bit planes for a CHUNK of images of different sizes.  decode_ragged: the host staging of the whole chunk at once and
three library calls per chunk -- parse, decode, tight boxes -- however many images it holds (csrc/rle_ragged.hip); encode_ragged,
the way back: count, positions, strings for a selection of the chunk's planes, three calls as well.  The per-image path
(ytvis_eval.stage_rle / decode_staged / plane_bboxes, what coco_eval.decode_segmentations calls) costs four small uploads and two or
three calls per image; on very many small images with a handful of masks each that is what the time goes to.

Layout.  The planes of the chunk are numbered flat, image after image, in the order given; plane p of an H x W image occupies
ceil(H*W/32) words of ONE flat int32 buffer, the planes back to back.  With an image's D planes followed by its G planes this is
the COCO chunk layout (include/s2d_hip.h, "Ragged layout"), so coco_eval.staged_chunk / mask_iou_staged read the buffer in place.
Every plane has the bits ytvis_eval.decode_frames gives it: both paths run the same device bodies (csrc/rle_planes.h).

Polygon segmentations (lists) are the rare path: their planes stay zero through the ragged decode and are rasterised afterwards by
one data.image_clip.polygons_to_bits call per image that has any, into that image's rows of the flat buffer.  RLE and polygon decode
are restated from pycocotools, which is on none of the project's machines: parity unpinned."""
from collections import Counter
from types import SimpleNamespace

import numpy as np

LIB_CALLS = Counter()          # library calls made by decode_ragged and encode_ragged, by export name


def _lib_call(name, *args):
    from ._lib import lib
    LIB_CALLS[name] += 1
    lib().call(name, *args)


def stage_rle_ragged(segs_per_image, sizes, names=None):
    """segs_per_image: per image its segmentations -- RLE dicts (compressed or uncompressed), polygon lists, or None for an absent
    plane --; sizes: per image (H, W); names: what to call an image in an error (default: its position).  -> SimpleNamespace of numpy
    arrays, the inputs of the three ragged calls:
      chars u8, str_off int64 [P+1], ends int32, nrun int32 [P]    as ytvis_eval.stage_rle's, over all planes of all images:
                          compressed strings are left for the device (nrun = -1); uncompressed counts get their running sums here,
                          clamped to THEIR OWN image's H*W; an absent or polygon plane has no slots and nrun = 0
      plane int64 [P, 4]  {word0, H, W, 0}                          tiles int32 [n_tiles, 2]  {plane, column block of 256}: ceil(W/256)
      words               the flat buffer's length                                           per plane
      plane0 int64 [N+1]  the first plane of every image            polygons  [(image, [row in the image], [that row's polygon list])]
    An RLE whose `size` is not its image's is refused by name."""
    N = len(segs_per_image)
    if len(sizes) != N:
        raise ValueError(f"{N} images and {len(sizes)} sizes")
    counts = np.array([len(s) for s in segs_per_image], np.int64)
    plane0 = np.zeros(N + 1, np.int64)
    np.cumsum(counts, out=plane0[1:])
    P = int(plane0[-1])
    H = np.array([int(s[0]) for s in sizes], np.int64).reshape(-1)
    W = np.array([int(s[1]) for s in sizes], np.int64).reshape(-1)
    for n in range(N):
        if H[n] < 1 or W[n] < 1 or H[n] * W[n] >= 1 << 31:
            raise ValueError(f"image {n if names is None else names[n]}: an image of {H[n]}x{W[n]}")
    wpp = (H * W + 31) // 32
    plane = np.zeros((P, 4), np.int64)
    plane[:, 1], plane[:, 2] = np.repeat(H, counts), np.repeat(W, counts)
    pw = np.repeat(wpp, counts)
    plane[:, 0] = np.cumsum(pw) - pw
    words = int(pw.sum())
    nt = (plane[:, 2] + 255) // 256                                       # column blocks per plane
    t0 = np.cumsum(nt) - nt
    tiles = np.stack([np.repeat(np.arange(P), nt), np.arange(int(nt.sum())) - np.repeat(t0, nt)], 1).astype(np.int32).reshape(-1, 2)

    lens = np.zeros(P, np.int64)
    nrun = np.zeros(P, np.int32)
    chunks, unc, polygons = [], [], []
    p = 0
    for n, segs in enumerate(segs_per_image):
        hw, size = int(H[n] * W[n]), [int(H[n]), int(W[n])]
        rows, polys = [], []
        for k, s in enumerate(segs):
            if isinstance(s, dict):
                if [int(v) for v in s["size"]] != size:
                    raise ValueError(f"image {n if names is None else names[n]}: RLE of size {s['size']} in an image of size {size}")
                c = s["counts"]
                if isinstance(c, (list, tuple)):
                    e = np.minimum(np.cumsum(np.asarray(c, np.int64)), hw)
                    lens[p] = nrun[p] = len(e)
                    chunks.append(bytes(len(e)))                          # slots only: the ends are written below
                    unc.append((p, e))
                else:
                    c = c.encode() if isinstance(c, str) else bytes(c)
                    chunks.append(c)
                    lens[p] = len(c)
                    nrun[p] = -1                                          # parsed on the device
            elif isinstance(s, (list, tuple)):
                rows.append(k)
                polys.append(s)
            elif s is not None:
                raise ValueError(f"image {n if names is None else names[n]}: no segmentation to decode: {s!r}")
            p += 1
        if rows:
            polygons.append((n, rows, polys))
    str_off = np.zeros(P + 1, np.int64)
    np.cumsum(lens, out=str_off[1:])
    total = max(int(str_off[-1]), 1)
    chars = np.zeros(total, np.uint8)
    buf = b"".join(chunks)
    chars[:len(buf)] = np.frombuffer(buf, np.uint8)
    ends = np.zeros(total, np.int32)
    for q, e in unc:
        ends[str_off[q]:str_off[q] + len(e)] = e
    return SimpleNamespace(chars=chars, str_off=str_off, ends=ends, nrun=nrun, plane=plane, tiles=tiles, words=words, plane0=plane0,
                           polygons=polygons, P=P, N=N)


def _upload(arrays, dev):
    """the arrays packed into one host buffer, ONE transfer, then typed views of the device copy (16-byte aligned each)"""
    import torch
    offs, n = [], 0
    for a in arrays:
        offs.append(n)
        n += (a.nbytes + 15) & ~15
    flat = np.zeros(max(n, 16), np.uint8)
    for a, o in zip(arrays, offs):
        flat[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.from_numpy(flat).to(dev)
    dt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}
    return [d[o:o + a.nbytes].view(dt[a.dtype]).view(a.shape) for a, o in zip(arrays, offs)]


def decode_ragged(staged, device=None, bbox_out=None):
    """stage_rle_ragged's arrays -> SimpleNamespace(bits int32 CUDA [words], the chunk's flat buffer; bbox int32 CUDA [P, 4] = x, y,
    w, h per plane, 0, 0, 0, 0 for an empty one; plane_dev) on the current stream.  One upload, then three library calls whatever the
    chunk holds (s2d_rle_parse_ragged, s2d_rle_decode_ragged, s2d_mask_plane_bbox_ragged_u32), plus one polygons_to_bits call per
    image that has polygons (before the boxes).  bbox_out: an int32 CUDA [P, 4] view to write the boxes into."""
    import torch
    from . import ops
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    s = staged
    bits = torch.empty((s.words,), device=dev, dtype=torch.int32)
    bbox = bbox_out if bbox_out is not None else torch.empty((s.P, 4), device=dev, dtype=torch.int32)
    if bbox.shape != (s.P, 4) or bbox.dtype != torch.int32 or not bbox.is_contiguous() or bbox.device != bits.device:
        raise ValueError(f"bbox_out must be contiguous int32 CUDA [{s.P}, 4]")
    out = SimpleNamespace(bits=bits, bbox=bbox, plane_dev=None)
    if s.P == 0:
        return out
    chars, str_off, ends, nrun, plane, tiles = _upload([s.chars, s.str_off, s.ends, s.nrun, s.plane, s.tiles], dev)
    st = ops._stream()
    _lib_call("s2d_rle_parse_ragged", chars, str_off, plane, s.P, ends, nrun, st)
    _lib_call("s2d_rle_decode_ragged", ends, str_off, nrun, plane, s.P, tiles, len(s.tiles), bits, s.words, st)
    if s.polygons:
        from .data.image_clip import _valid_polygons, polygons_to_bits
        for n, rows, polys in s.polygons:
            p0, F = int(s.plane0[n]), int(s.plane0[n + 1] - s.plane0[n])
            w0, H, W = int(s.plane[p0, 0]), int(s.plane[p0, 1]), int(s.plane[p0, 2])
            wpp = (H * W + 31) // 32
            polygons_to_bits([_valid_polygons(q) for q in polys], H, W, out=bits[w0:w0 + F * wpp].view(F, wpp), rows=rows)
            LIB_CALLS["s2d_polygons_to_bits"] += 1
    _lib_call("s2d_mask_plane_bbox_ragged_u32", bits, plane, s.P, s.words, bbox, st)
    out.plane_dev = plane
    return out


def encode_ragged(bits, staged_or_plane_table, sel):
    """the way back: bits int32 CUDA [words], the flat buffer of a chunk; staged_or_plane_table: what stage_rle_ragged returned, or a
    plane table int64 numpy [P, 4] = {word0, H, W, 0}; sel: the planes to encode, in any order -> (list of {"size": [H, W], "counts":
    str} in the order of sel, areas int64 numpy [S], boxes float64 numpy [S, 4] = x, y, w, h).  One upload, three library calls and
    two read-backs (the boundary counts, then the strings) however many planes are selected.  A plane's string is byte for byte what
    s2d_amd.rle.encode writes for the same mask: both run the device bodies of csrc/rle_encode.h."""
    import torch
    from . import ops
    from ._lib import lib
    plane = np.ascontiguousarray(getattr(staged_or_plane_table, "plane", staged_or_plane_table), np.int64).reshape(-1, 4)
    sel = np.ascontiguousarray(sel, np.int32).reshape(-1)
    P, S = len(plane), len(sel)
    if S == 0:
        return [], np.zeros((0,), np.int64), np.zeros((0, 4), np.float64)
    if bits.dtype != torch.int32 or bits.dim() != 1 or not bits.is_cuda or not bits.is_contiguous():
        raise ValueError(f"encode_ragged needs the flat int32 CUDA buffer of a chunk, got {bits.dtype} {tuple(bits.shape)}")
    if sel.min() < 0 or sel.max() >= P:
        raise ValueError(f"encode_ragged: a selected plane outside [0, {P})")
    rows = plane[sel]
    H, W = rows[:, 1], rows[:, 2]
    if H.min() < 1 or W.min() < 1 or (H * W).max() >= 1 << 31 or rows[:, 0].min() < 0 or (rows[:, 0] + (H * W + 31) // 32).max() > bits.numel():
        raise ValueError(f"encode_ragged: a selected plane does not fit the buffer of {bits.numel()} words")
    col0 = np.cumsum(W) - W
    dev, st = bits.device, ops._stream()
    plane_d, sel_d, col0_d = _upload([plane, sel, col0], dev)
    col_off = torch.empty((int(W.sum()),), device=dev, dtype=torch.int32)
    nb = torch.empty((S,), device=dev, dtype=torch.int32)
    area = torch.empty((S,), device=dev, dtype=torch.int32)
    bbox = torch.empty((S, 4), device=dev, dtype=torch.int32)
    _lib_call("s2d_rle_count_ragged_u32", bits, plane_d, P, bits.numel(), sel_d, S, col0_d, col_off, nb, area, bbox, st)
    frame_off = torch.zeros((S + 1,), device=dev, dtype=torch.int64)
    torch.cumsum(nb, 0, out=frame_off[1:])
    total = int(frame_off[-1])                                            # read-back 1: sizes the outputs
    ncounts = total + S
    pos = torch.empty((max(total, 1),), device=dev, dtype=torch.int32)
    _lib_call("s2d_rle_positions_ragged_u32", bits, plane_d, P, bits.numel(), sel_d, S, col0_d, col_off, frame_off, pos, st)
    ws = torch.empty((lib().call("s2d_rle_strings_ragged_workspace_bytes", ncounts),), device=dev, dtype=torch.uint8)
    chars = torch.empty((7 * ncounts,), device=dev, dtype=torch.uint8)
    str_off = torch.empty((S + 1,), device=dev, dtype=torch.int64)
    _lib_call("s2d_rle_strings_ragged", pos, frame_off, plane_d, P, sel_d, S, ncounts, ws, ws.numel(), chars, str_off, st)
    so = str_off.cpu().numpy()                                            # read-back 2
    buf = chars[:int(so[-1])].cpu().numpy().tobytes()
    rles = [{"size": [int(H[s]), int(W[s])], "counts": buf[so[s]:so[s + 1]].decode("ascii")} for s in range(S)]
    return rles, area.cpu().numpy().astype(np.int64), bbox.cpu().numpy().astype(np.float64)
