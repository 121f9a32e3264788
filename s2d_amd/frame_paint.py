"""Stage-1 frame masks on the device: `infer_frame_areas`, `infer_paint` and `paint_frames`, the bindings of
s2d_infer_frame_areas_i32 / s2d_infer_paint_u8 (csrc/infer.hip).  `s2d_amd.ops` re-exports them beside `infer_index`; they are defined
here, not in ops.py, for the reason index_map.py gives: the recorded-entry-point tables of tests/test_gpu_forward_c4.py and
tests/test_gpu_eval_720p.py list every function DEFINED in ops.py.  Their rows are tests/test_gpu_frame_paint.py.

The paint rule (one definition: kernel, tests/frame_masks_refs.py, INTEGRATION.md "Stage-1 frame masks").  K proposals in score
order, planes m_k,t = "proposal k holds the pixel", the bit infer_masks writes.  area[k][t] = set pixels of m_k,t; order[t] = the
proposals by descending area, equal areas in proposal order; the frame starts black and the proposals are painted in order[t], a
later one over an earlier one: a pixel belongs to the holder with the largest position in order[t] -- the smallest area, among equal
areas the higher k.  rgb = colors[k] of that owner (by k, not by position) or black; index = k + 1 or 0."""
import torch

from .index_map import INDEX_MAX_PROPOSALS

PAINT_MAX_PROPOSALS = INDEX_MAX_PROPOSALS


def mask_colors(n):
    """-> u8 numpy [n, 3]: n <= 254 distinct non-black colours, entries 1..n of the DAVIS palette (davis_eval.DAVIS_PALETTE: the
    PASCAL VOC colour map, whose 256 entries are distinct and whose entry 0 alone is black)"""
    import numpy as np
    from .davis_eval import DAVIS_PALETTE
    if not 0 <= int(n) <= PAINT_MAX_PROPOSALS:
        raise ValueError(f"mask_colors({n}): 0..{PAINT_MAX_PROPOSALS} colours")
    return np.asarray(DAVIS_PALETTE, np.uint8).reshape(256, 3)[1:int(n) + 1].copy()


def _geometry(name, mask_logits, dims, query):
    from . import ops
    ops._chk(mask_logits); ops._chk(query, torch.int32)
    T, hm, wm = dims
    K = query.shape[0] if query.dim() == 1 else -1
    ldq = mask_logits.shape[-1]
    if mask_logits.dim() != 2 or mask_logits.shape[0] != T * hm * wm or not 1 <= K <= PAINT_MAX_PROPOSALS or ldq > 128 or ldq % 4:
        raise ValueError(f"{name} needs [T*hm*wm, ldq] logits with ldq <= 128 a multiple of 4 and 1 <= K <= {PAINT_MAX_PROPOSALS} "
                         f"proposals, got {tuple(mask_logits.shape)} for dims {tuple(dims)} and query {tuple(query.shape)}")
    return T, hm, wm, K, ldq


def infer_frame_areas(mask_logits, dims, padded, img_size, out_size, query, want_order=True):
    """mask_logits pixel-major [T*hm*wm, ldq]; dims = (T, hm, wm); query int32 [K] in proposal order -> (areas int32 [K,T], order
    int32 [T,K] or None): the set pixels of every infer_masks plane at output size, and per frame the proposals by descending area,
    equal areas in proposal order (what mask_frame_areas gives for those planes).  The [K,T,oh,ow] planes never exist."""
    from . import ops
    from ._lib import lib
    T, hm, wm, K, ldq = _geometry("infer_frame_areas", mask_logits, dims, query)
    (Hp, Wp), (ih, iw), (oh, ow) = padded, img_size, out_size
    areas = torch.empty((K, T), device=mask_logits.device, dtype=torch.int32)
    order = torch.empty((T, K), device=mask_logits.device, dtype=torch.int32) if want_order else None
    lib().call("s2d_infer_frame_areas_i32", mask_logits, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, query, K, areas, order, ops._stream())
    return areas, order


def infer_paint(mask_logits, dims, padded, img_size, out_size, query, order, colors, want_index=True):
    """order int32 [T,K] (infer_frame_areas), colors u8 [K,3] on the device -> (rgb u8 [T,oh,ow,3], index u8 [T,oh,ow] or None): the
    paint rule of the module docstring, straight from the logits."""
    from . import ops
    from ._lib import lib
    T, hm, wm, K, ldq = _geometry("infer_paint", mask_logits, dims, query)
    if not torch.is_tensor(order) or order.dtype != torch.int32 or tuple(order.shape) != (T, K):
        raise ValueError(f"order must be int32 [{T}, {K}] (frames x proposals), got "
                         f"{getattr(order, 'dtype', type(order).__name__)} {tuple(getattr(order, 'shape', ()))}")
    if not torch.is_tensor(colors) or colors.dtype != torch.uint8 or tuple(colors.shape) != (K, 3):
        raise ValueError(f"colors must be uint8 [{K}, 3], got {getattr(colors, 'dtype', type(colors).__name__)} "
                         f"{tuple(getattr(colors, 'shape', ()))}")
    ops._chk(order, torch.int32); ops._chk(colors, torch.uint8)
    (Hp, Wp), (ih, iw), (oh, ow) = padded, img_size, out_size
    rgb = torch.empty((T, oh, ow, 3), device=mask_logits.device, dtype=torch.uint8)
    index = torch.empty((T, oh, ow), device=mask_logits.device, dtype=torch.uint8) if want_index else None
    lib().call("s2d_infer_paint_u8", mask_logits, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, query, K, order, colors, rgb, index,
               ops._stream())
    return rgb, index


def paint_frames(mask_logits, dims, padded, img_size, out_size, query, colors, want_index=True):
    """infer_frame_areas then infer_paint -> (rgb, index or None, areas, order)"""
    areas, order = infer_frame_areas(mask_logits, dims, padded, img_size, out_size, query)
    rgb, index = infer_paint(mask_logits, dims, padded, img_size, out_size, query, order, colors, want_index)
    return rgb, index, areas, order
