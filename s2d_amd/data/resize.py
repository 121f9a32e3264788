"""Test-time frame resize: detectron2's ResizeShortestEdge -> ResizeTransform.apply_image on uint8 frames, which is
PIL Image.resize(BILINEAR).  PIL's bilinear (third party, restated: libImaging/Resample.c, ImagingResample for 8-bit images) is
not the textbook 2-tap filter: its triangle's support scales with the downscale factor, weights are 22-bit fixed point, and the
two separable passes (horizontal first) go through a uint8 intermediate.

`pil_coeffs` builds one axis's table in float64 in PIL's order of operations; `resize_frames` runs the device kernel
(s2d_resize_bilinear_u8, csrc/resize.hip) on those tables; `resize_np` is the same integer arithmetic in numpy, the statement the
tests hold both PIL and the kernel to."""
import math

import numpy as np

PREC = 22                        # PRECISION_BITS of the 8-bit path: 32 - 8 - 2
BW = 64                          # output columns per workgroup of the kernel
LDS_LIMIT = 65536


def pil_coeffs(in_size, out_size):
    """-> (bounds int32 [out, 2] = (xmin, taps), coeffs int32 [out, k]): precompute_coeffs + normalize_coeffs_8bpc for a box of
    the whole axis.  An unchanged axis gets the identity table (PIL skips that pass; one tap of 2^22 gives the same bytes)."""
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize of an axis {in_size} -> {out_size}")
    if in_size == out_size:
        return (np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1).astype(np.int32),
                np.full((out_size, 1), 1 << PREC, np.int32))
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                                  # bilinear support 1.0
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ws = []
        ww = 0.0
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            w = 1.0 - t if t < 1.0 else 0.0
            ws.append(w)
            ww += w
        for x in range(xmax):
            w = ws[x] / ww if ww != 0.0 else ws[x]
            kk[xx, x] = int(-0.5 + w * (1 << PREC)) if w < 0 else int(0.5 + w * (1 << PREC))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _clip8(s):
    return np.where(s >= (1 << PREC << 8), 255, np.where(s <= 0, 0, s >> PREC)).astype(np.uint8)


def _pass(img, bounds, kk, axis):
    """one separable pass of HWC u8 `img` along axis 1 (horizontal) or 0 (vertical), int64 arithmetic"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.full((bounds.shape[0],) + src.shape[1:], 1 << (PREC - 1), np.int64)
    for i, (lo, n) in enumerate(bounds):
        for k in range(n):
            out[i] += src[lo + k] * int(kk[i, k])
    return np.moveaxis(_clip8(out), 0, axis)


def resize_np(img, out_hw):
    """HWC u8 numpy image -> HWC u8 [H1, W1, C]: the integer two-pass resize on pil_coeffs' tables"""
    H0, W0 = img.shape[:2]
    H1, W1 = out_hw
    out = img
    if W1 != W0:
        out = _pass(out, *pil_coeffs(W0, W1), axis=1)
    if H1 != H0:
        out = _pass(out, *pil_coeffs(H0, H1), axis=0)
    return np.ascontiguousarray(out)


def _check_monotone(bounds):
    lo, hi = bounds[:, 0].astype(np.int64), bounds[:, 0].astype(np.int64) + bounds[:, 1]
    if (np.diff(lo) < 0).any() or (np.diff(hi) < 0).any():
        raise ValueError("resize coefficient table is not monotone")


def plan(hb, hk, vb):
    """launch plan of s2d_resize_bilinear_u8 -> (band_rows, rows_max, span_q), the largest band of output rows (<= 16) whose
    workgroup LDS fits in 64 KiB"""
    _check_monotone(hb); _check_monotone(vb)
    W1, H1 = hb.shape[0], vb.shape[0]
    first = np.arange(0, W1, BW)
    last = np.minimum(first + BW, W1) - 1
    nbytes = (hb[last, 0].astype(np.int64) + hb[last, 1] - hb[first, 0]) * 3
    span_q = int(((nbytes + 15 + 15) // 16).max())               # + 15: the first chunk starts up to 15 bytes early
    kh = hk.shape[1]
    for band in (16, 8, 4, 2, 1):
        y0 = np.arange(0, H1, band)
        y1 = np.minimum(y0 + band, H1) - 1
        rows_max = int((vb[y1, 0].astype(np.int64) + vb[y1, 1] - vb[y0, 0]).max())
        lds = rows_max * span_q * 16 + 3 * rows_max * BW + kh * BW * 4
        if lds <= LDS_LIMIT:
            return band, rows_max, span_q
    raise ValueError(f"resize {W1}x{H1}: the downscale factor is too large for one workgroup's LDS")


_TABLES = {}


def _tables(H0, W0, H1, W1, device):
    import torch
    key = (H0, W0, H1, W1, str(device))
    ent = _TABLES.get(key)
    if ent is None:
        hb, hk = pil_coeffs(W0, W1)
        vb, vk = pil_coeffs(H0, H1)
        p = plan(hb, hk, vb)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (hb, hk, vb, vk)]
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = ent = (dev, hk.shape[1], vk.shape[1], p)
    return ent


def resize_frames(frames, out_hw, stream=None):
    """u8 CUDA frames [T, H0, W0, 3] (HWC RGB, as decoded) -> u8 CUDA [T, 3, H1, W1] (CHW, the mapper's `image` layout), bit-exact
    to PIL Image.resize((W1, H1), BILINEAR) per frame.  Enqueued on `stream` (default: the current stream)."""
    import torch
    from .. import ops
    from .._lib import lib
    ops._chk(frames, torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames must be [T, H, W, 3], got {tuple(frames.shape)}")
    T, H0, W0, _ = frames.shape
    H1, W1 = (int(v) for v in out_hw)
    out = torch.empty((T, 3, H1, W1), device=frames.device, dtype=torch.uint8)
    if T == 0:
        return out
    (hb, hk, vb, vk), kh, kv, (band, rows_max, span_q) = _tables(H0, W0, H1, W1, frames.device)
    st = stream if stream is not None else ops._stream()
    lib().call("s2d_resize_bilinear_u8", frames, T, H0, W0, hb, hk, kh, vb, vk, kv, H1, W1, band, rows_max, span_q, out, st)
    return out
