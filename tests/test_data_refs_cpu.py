"""Float64 references of the data-path kernels (csrc/augment.hip) and the proof, without a GPU, that they and the band rule hold on
the inputs tests/test_gpu_data_720p.py uses: the float32 mirror of the oracle (oracle_np.aug_warp_frames / aug_warp_masks) and CPU
torch's own F.interpolate (what the reference's copy-paste calls) are compared with them under the same rule and the same cap the
GPU module applies to the kernels.  The GPU module imports the references, the inputs and the rule from here.

References (plain numpy float64; nothing of s2d_amd / libs2d_hip.so in them)
  warp_frames_f64 / warp_masks_f64   the clip augmentation: the inverse affine map from the float32 params row evaluated in float64, the
      crop-rectangle test, taps clamped to the crop, bilinear (frames) / nearest (masks), the rounding chain rint -> trunc(clip(bright
      * q)) -> trunc(clip((1 - c) * mean + c * q)), the crop mean from the exact integer sum.
  paste_frame_f64    one target frame of the trainer's copy-paste: s = max(0, in / out * (dst + 0.5) - 0.5), two taps per axis, image
      truncated to a byte, masks non-zero, placed at (h_shift, w_shift), alpha = union of the (kept) pasted masks.
  paste_frame_torch  the same frame with CPU torch.nn.functional.interpolate(bilinear, align_corners=False).
  shift_planes_np    the sparse-mask densification, by slicing.

Band rule (derived from the number formats and the inputs, never from a kernel's output)
  EPS  A float32 coordinate of magnitude below 2048 carries at most 3 roundings of 2^-13 from the map (two products and the sums of
       a11 * px + a12 * py + a13; `scale * (dst + 0.5) - 0.5` of the paste has as many): EPS = 3 * 2^-13 source pixels.
  masks / canvas   compared exactly unless the float64 source coordinate lies within EPS of an integer (the nearest tap), of a crop
       edge (an integer too) or of a zero bilinear weight (l = 0: the `.bool()` of the interpolated mask) -- AND the other side gives
       another value: the reference is evaluated at the coordinates moved by -EPS and +EPS per axis (and, for the paste, unmoved);
       a pixel is excluded only when those evaluations disagree.  Stricter than excluding every pixel near an integer (that alone
       would be 4 * EPS = 1.5e-3 of a rotated plane).
  frames / composite   within 1 level everywhere; equal unless the float64 value lies in the band of a rounding tie:
       * bilinear value v before rint (x.5) or before the `.byte()` truncation (an integer): |v32 - v64| <= EPS * (Sx + Sy) + 6 * 255
         * 2^-24.  First term: the coordinate error times the steepest horizontal / vertical step between adjacent taps in the 4 x 4
         source neighbourhood of the pixel (a bilinear surface is continuous and moves at most that much per source pixel).  Second:
         each of the 4 taps passes through at most 6 float32 roundings (its weight 1 - l, two products, two sums, the outer weight),
         2^-24 relative each, and the weights sum to 1 over taps of at most 255.
       * t = bright * q before its trunc: one rounding, 2^-24 * |t|.
       * u = (1 - c) * m + c * q before its trunc: 1 - c is exact (c in [0.5, 2]); m carries two roundings (the mean to float32, the
         product with bright); two products and one sum: 2^-24 * (4 |1 - c| m + 2 * 255 c).
       A frame pixel whose crop-rectangle test flips within EPS (the rotation fill, 0, against a source value) is excluded, and so is a
       composite pixel whose alpha is ambiguous.  Pixels in the band are still compared (1 level); the cap counts excluded + differing.
       One level is a theorem only for gains up to 1: a rint that flips (1 level) times a brightness of 1.1 is 1.1 levels before the
       trunc, which can come out as 2 (the float32 mirror does, on draws with a gain above 1).  The draws of the frame cases are
       therefore chosen with brightness and contrast below 1 (asserted); gains above 1 and the upper clip run against the mirror in
       tests/test_gpu_data.py.
  CAP  excluded or differing pixels are at most 1e-3 of a plane (the cap of tests/test_gpu_data.py and tests/test_gpu_eval_720p.py)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from s2d_amd.utils import synth

EPS = 3 * 2.0 ** -13
ARITH = 6 * 255 * 2.0 ** -24
CAP = 1e-3


# --------------------------------------------------------------------------- shared pieces
def _steps(p):
    """p float64 [H, W] -> (Sx, Sy): the largest |horizontal| / |vertical| step between adjacent pixels in the 4 x 4 neighbourhood
    [y - 1, y + 2] x [x - 1, x + 2] of (y, x), the cells a point of cell (y, x) can reach by moving less than one pixel"""
    H, W = p.shape
    out = []
    for axis in (1, 0):
        g = np.zeros((H + 3, W + 3))
        d = np.abs(np.diff(p, axis=axis))
        g[1:1 + d.shape[0], 1:1 + d.shape[1]] = d
        s = np.zeros((H, W))
        ny, nx = (4, 3) if axis == 1 else (3, 4)               # steps x -> x + 1 start at x - 1 .. x + 1; rows y - 1 .. y + 2
        for dy in range(ny):
            for dx in range(nx):
                np.maximum(s, g[dy:dy + H, dx:dx + W], out=s)
        out.append(s)
    return out


def _near_int(v, d):
    return np.abs(v - np.rint(v)) < d


def check_levels(name, got, ref, band, excluded=None):
    """the frame rule: got within 1 level of ref everywhere and equal outside the band (excluded pixels apart); excluded + differing
    pixels under the cap.  -> (largest difference, share in the band, share differing, share excluded); prints before asserting"""
    ex = np.zeros(got.shape, bool) if excluded is None else np.broadcast_to(excluded, got.shape)
    d = np.where(ex, 0, np.abs(got.astype(np.int32) - ref.astype(np.int32)))
    n_band, n_ex, n_diff, n_out = int((band & ~ex).sum()), int(ex.sum()), int((d != 0).sum()), int(((d != 0) & ~band).sum())
    print(f"datarow {name}: max diff {int(d.max())}, differing {n_diff} ({n_diff / got.size:.3e}), {n_out} of them outside the band; in the band "
          f"{n_band} ({n_band / got.size:.3e}), excluded {n_ex} ({n_ex / got.size:.3e}); {got.size} values")
    assert int(d.max()) <= 1, (name, int(d.max()))
    assert n_out == 0, (name, n_out)
    assert n_ex + n_diff <= CAP * got.size, (name, n_ex, n_diff)
    return int(d.max()), n_band / got.size, n_diff / got.size, n_ex / got.size


def check_exact(name, got, ref, amb):
    """the mask rule: equal outside the ambiguous pixels, those under the cap.  -> (excluded share, differing share)"""
    dif = (got != 0) != (ref != 0)
    n_amb, n_diff, n_out = int(amb.sum()), int(dif.sum()), int((dif & ~amb).sum())
    print(f"datarow {name}: excluded {n_amb} ({n_amb / max(got.size, 1):.3e}), differing {n_diff}, {n_out} of them outside the band; {got.size} pixels")
    assert n_out == 0, (name, n_out)
    assert n_amb <= CAP * got.size, (name, n_amb)
    return n_amb / max(got.size, 1), n_diff / max(got.size, 1)


# --------------------------------------------------------------------------- clip augmentation
def _source_points(row, H1, W1):
    a = row.astype(np.float64)
    px = (np.arange(W1) + 0.5)[None, :]
    py = (np.arange(H1) + 0.5)[:, None]
    return a[0] * px + a[1] * py + a[2], a[3] * px + a[4] * py + a[5]


def _inside(sx, sy, cx, cy, cw, ch):
    return (sx >= cx) & (sy >= cy) & (sx < cx + cw) & (sy < cy + ch)


def _inside_flips(sx, sy, crop):
    """pixels whose crop-rectangle test changes when the point moves by EPS along either axis"""
    c = [_inside(sx + ex, sy + ey, *crop) for ex in (-EPS, EPS) for ey in (-EPS, EPS)]
    return (c[0] | c[1] | c[2] | c[3]) & ~(c[0] & c[1] & c[2] & c[3])


def crop_mean_f64(frames_t, row):
    """float64 (exact integer sum / count) * bright, and the float32 the kernels must write back into params[12]"""
    cx, cy, cw, ch = (int(v) for v in row[6:10])
    crop = frames_t[:, cy:cy + ch, cx:cx + cw]
    mean = int(crop.astype(np.int64).sum()) / (3.0 * cw * ch)
    return mean * float(row[10]), np.float32(np.float32(mean) * np.float32(row[10]))


def warp_frames_f64(frames, params, out_hw):
    """frames u8 [T,3,H0,W0], params f32 [T,16] -> (u8 [T,3,H1,W1], band bool [T,3,H1,W1]: a rounding tie, excluded bool [T,1,H1,W1]:
    the crop-rectangle test flips)"""
    T = frames.shape[0]
    H1, W1 = out_hw
    out = np.zeros((T, 3, H1, W1), np.uint8)
    band = np.zeros((T, 3, H1, W1), bool)
    excl = np.zeros((T, 1, H1, W1), bool)
    for t in range(T):
        row = params[t]
        crop = tuple(float(v) for v in row[6:10])
        bright, contrast = float(row[10]), float(row[11])
        sx, sy = _source_points(row, H1, W1)
        inside = _inside(sx, sy, *crop)
        flips = _inside_flips(sx, sy, crop)
        fx, fy = sx - 0.5, sy - 0.5
        x0f, y0f = np.floor(fx), np.floor(fy)
        lx, ly = fx - x0f, fy - y0f
        xl, xh, yl, yh = int(crop[0]), int(crop[0] + crop[2]) - 1, int(crop[1]), int(crop[1] + crop[3]) - 1
        x0 = np.clip(x0f.astype(np.int64), xl, xh); x1 = np.clip(x0f.astype(np.int64) + 1, xl, xh)
        y0 = np.clip(y0f.astype(np.int64), yl, yh); y1 = np.clip(y0f.astype(np.int64) + 1, yl, yh)
        mean = float(row[12])
        if mean < 0:
            mean = crop_mean_f64(frames[t], row)[0]
        for c in range(3):
            p = frames[t, c].astype(np.float64)
            Sx, Sy = _steps(p)
            v = (1 - ly) * ((1 - lx) * p[y0, x0] + lx * p[y0, x1]) + ly * ((1 - lx) * p[y1, x0] + lx * p[y1, x1])
            tie = _near_int(v - 0.5, EPS * (Sx[y0, x0] + Sy[y0, x0]) + ARITH)
            q = np.rint(v)
            if bright != 1:
                tb = bright * q
                tie |= _near_int(tb, 2.0 ** -24 * np.abs(tb))
                q = np.trunc(np.clip(tb, 0, 255))
            if contrast != 1:
                u = (1 - contrast) * mean + contrast * q
                tie |= _near_int(u, 2.0 ** -24 * (4 * abs(1 - contrast) * abs(mean) + 2 * 255 * abs(contrast)))
                q = np.trunc(np.clip(u, 0, 255))
            out[t, c] = np.where(inside, q, 0).astype(np.uint8)
            band[t, c] = tie & inside
        excl[t, 0] = flips
    return out, band, excl


def warp_masks_f64(masks, params, out_hw):
    """masks u8 [N,T,H0,W0] -> (u8 [N,T,H1,W1] 0/1, ambiguous bool [N,T,H1,W1]): nearest tap of the float64 point; ambiguous = the
    four evaluations at (sx -+ EPS, sy -+ EPS) disagree (a tap or the crop test changes AND the value with it)"""
    N, T, H0, W0 = masks.shape
    H1, W1 = out_hw
    out = np.zeros((N, T, H1, W1), np.uint8)
    amb = np.zeros((N, T, H1, W1), bool)
    for t in range(T):
        crop = tuple(float(v) for v in params[t, 6:10])
        sx, sy = _source_points(params[t], H1, W1)

        def tap(x, y):
            ins = _inside(x, y, *crop)
            return ins, np.clip(np.floor(y).astype(np.int64), 0, H0 - 1), np.clip(np.floor(x).astype(np.int64), 0, W0 - 1)
        centre = tap(sx, sy)
        corners = [tap(sx + ex, sy + ey) for ex in (-EPS, EPS) for ey in (-EPS, EPS)]
        for n in range(N):
            m = masks[n, t] != 0
            ins, iy, ix = centre
            ref = ins & m[iy, ix]
            out[n, t] = ref
            for ins, iy, ix in corners:
                amb[n, t] |= (ins & m[iy, ix]) != ref
    return out, amb


# --------------------------------------------------------------------------- video copy-paste
def _axis_taps(n_dst, in_size, out_size, delta=0.0):
    """-> (i0, i1, has1): the taps of F.interpolate(bilinear, align_corners=False) along one axis with the coordinate moved by delta;
    has1: the second tap has a non-zero weight"""
    s = np.maximum(0.0, in_size / out_size * (np.arange(n_dst) + 0.5) - 0.5 + delta)
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, (s - i0 != 0) & (i1 != i0), s - i0


def _resize_bool(cur, yt, xt, rows=None, cols=None):
    """cur bool [K,Hc,Wc] -> bool [K, rows, cols]: `.bool()` of the bilinear resize = OR over the taps of non-zero weight"""
    r0, r1, hy = (a if rows is None else a[rows] for a in yt[:3])
    c0, c1, hx = (a if cols is None else a[cols] for a in xt[:3])
    need = np.unique(np.concatenate([r0, r1]))
    sub = cur[:, need]
    a = sub[:, :, c0] | (sub[:, :, c1] & hx[None, None, :])
    return a[:, np.searchsorted(need, r0)] | (a[:, np.searchsorted(need, r1)] & hy[None, :, None])


def _differs(a, b):
    return (a[0] != b[0]) | (a[1] != b[1]) | (a[2] != b[2])


def paste_frame_f64(src_frame, cur_masks, tgt_frame, tgt_masks, geo, keep=None):
    """One target frame.  src_frame u8 [3,Hs,Ws]; cur_masks u8 [K,Hc,Wc] (0 / non-0); tgt_frame u8 [3,H,W]; tgt_masks u8 [N,H,W];
    geo = (h_new, w_new, h_shift, w_shift) with the patch inside the target; keep: bool [K] or None (all kept).
    -> dict: canvas u8 [K,H,W] (before keep), amb bool [K,H,W], alpha / alpha_amb bool [H,W], frame u8 [3,H,W], frame_band bool
    [3,H,W] (a truncation tie; alpha_amb not included), tgt u8 [N,H,W], inter [K,N], tarea [N], alive [N] (int64, of the unmoved
    evaluation)"""
    h_new, w_new, h_shift, w_shift = geo
    K, Hc, Wc = cur_masks.shape
    _, Hs, Ws = src_frame.shape
    N, H, W = tgt_masks.shape[0], tgt_frame.shape[1], tgt_frame.shape[2]
    assert 0 <= h_shift and h_shift + h_new <= H and 0 <= w_shift and w_shift + w_new <= W
    cur = cur_masks != 0
    yv = [_axis_taps(h_new, Hc, h_new, d) for d in (0.0, -EPS, EPS)]
    xv = [_axis_taps(w_new, Wc, w_new, d) for d in (0.0, -EPS, EPS)]
    m = _resize_bool(cur, yv[0], xv[0])
    a = np.zeros_like(m)
    rows = np.nonzero(_differs(yv[0], yv[1]) | _differs(yv[0], yv[2]))[0]
    cols = np.nonzero(_differs(xv[0], xv[1]) | _differs(xv[0], xv[2]))[0]
    for y in yv:
        for x in xv:
            if rows.size:
                a[:, rows] |= _resize_bool(cur, y, x, rows=rows) != m[:, rows]
            if cols.size:
                a[:, :, cols] |= _resize_bool(cur, y, x, cols=cols) != m[:, :, cols]
    ys, xs = slice(h_shift, h_shift + h_new), slice(w_shift, w_shift + w_new)
    canvas = np.zeros((K, H, W), np.uint8); canvas[:, ys, xs] = m
    amb = np.zeros((K, H, W), bool); amb[:, ys, xs] = a
    kept = np.ones(K, bool) if keep is None else np.asarray(keep, bool)
    alpha = (canvas[kept] != 0).any(0)
    alpha_amb = amb[kept].any(0)
    # the image patch, from the source frame
    y0, y1, _, ly = _axis_taps(h_new, Hs, h_new)
    x0, x1, _, lx = _axis_taps(w_new, Ws, w_new)
    ly, lx = ly[:, None], lx[None, :]
    frame = tgt_frame.copy()
    frame_band = np.zeros((3, H, W), bool)
    for c in range(3):
        p = src_frame[c].astype(np.float64)
        Sx, Sy = _steps(p)
        r0, r1 = p[y0], p[y1]
        v = (1 - ly) * ((1 - lx) * r0[:, x0] + lx * r0[:, x1]) + ly * ((1 - lx) * r1[:, x0] + lx * r1[:, x1])
        tie = _near_int(v, EPS * (Sx[y0][:, x0] + Sy[y0][:, x0]) + ARITH)
        frame[c, ys, xs] = np.where(alpha[ys, xs], np.trunc(v).astype(np.uint8), tgt_frame[c, ys, xs])
        frame_band[c, ys, xs] = tie & alpha[ys, xs]
    tm = tgt_masks != 0
    tgt = (tm & ~alpha[None]).astype(np.uint8)
    cb = canvas != 0
    inter = np.array([[int((cb[k] & tm[n]).sum()) for n in range(N)] for k in range(K)], np.int64).reshape(K, N)
    return dict(canvas=canvas, amb=amb, alpha=alpha, alpha_amb=alpha_amb, frame=frame, frame_band=frame_band, tgt=tgt, inter=inter,
                tarea=np.array([int(tm[n].sum()) for n in range(N)], np.int64), alive=np.array([int(tgt[n].sum()) for n in range(N)], np.int64))


def paste_patch_torch(src_frame, cur_masks, geo):
    """the two F.interpolate calls of engine/train_loop.py:471 / :487 on CPU tensors -> (image patch u8 [3,h_new,w_new], masks bool
    [K,h_new,w_new])"""
    size = (geo[0], geo[1])
    img = F.interpolate(torch.from_numpy(np.array(src_frame))[None].float(), size=size, mode="bilinear", align_corners=False).byte().squeeze(0)
    msk = F.interpolate(torch.from_numpy((cur_masks != 0))[None].float(), size=size, mode="bilinear", align_corners=False).bool().squeeze(0)
    return img.numpy(), msk.numpy()


def paste_frame_torch(src_frame, cur_masks, tgt_frame, tgt_masks, geo, keep=None):
    """paste_frame_f64's canvas, frame and tgt from the torch patch (train_loop.py:490-548: empty canvas, alpha composite)"""
    h_new, w_new, h_shift, w_shift = geo
    K, (H, W) = cur_masks.shape[0], tgt_frame.shape[1:]
    img, msk = paste_patch_torch(src_frame, cur_masks, geo)
    ys, xs = slice(h_shift, h_shift + h_new), slice(w_shift, w_shift + w_new)
    canvas = np.zeros((K, H, W), np.uint8); canvas[:, ys, xs] = msk
    kept = np.ones(K, bool) if keep is None else np.asarray(keep, bool)
    alpha = (canvas[kept] != 0).any(0)
    frame = tgt_frame.copy()
    frame[:, ys, xs] = np.where(alpha[None, ys, xs], img, tgt_frame[:, ys, xs])
    return dict(canvas=canvas, alpha=alpha, frame=frame, tgt=((tgt_masks != 0) & ~alpha[None]).astype(np.uint8))


def check_paste(name, got, ref):
    """got: dict with canvas, frame, tgt (a kernel's or torch's) against paste_frame_f64's dict under the band rule.  The composite and
    the target masks are compared where alpha is not ambiguous.  -> figures (dict)"""
    K = ref["canvas"].shape[0]
    fig = {}
    fig["canvas"] = check_exact(f"{name} canvas", got["canvas"], ref["canvas"], ref["amb"]) if K else (0.0, 0.0)
    aa = ref["alpha_amb"]
    if got["tgt"].size:
        fig["tgt"] = check_exact(f"{name} out_tgt", got["tgt"], ref["tgt"], np.broadcast_to(aa[None], got["tgt"].shape))
    fig["frame"] = check_levels(f"{name} composite", got["frame"], ref["frame"], ref["frame_band"], aa[None])
    return fig


# --------------------------------------------------------------------------- sparse-mask densification
def shift_planes_np(planes, shifts):
    """planes: list of [H,W] arrays (bool / u8), shifts: list of (dx, dy) -> u8 [n,H,W]: out[j][y][x] = planes[j][y + dy][x + dx] != 0
    inside the frame, else 0"""
    H, W = planes[0].shape
    out = np.zeros((len(planes), H, W), np.uint8)
    for j, (p, (dx, dy)) in enumerate(zip(planes, shifts)):
        ys0, ys1 = max(0, -dy), min(H, H - dy)
        xs0, xs1 = max(0, -dx), min(W, W - dx)
        if ys0 < ys1 and xs0 < xs1:
            out[j, ys0:ys1, xs0:xs1] = np.asarray(p)[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx] != 0
    return out


# --------------------------------------------------------------------------- the inputs both modules use
def _augmentation(min_size, crop):
    from s2d_amd.data.augment import ClipAugmentation
    return ClipAugmentation(min_size=(min_size,), sample_style="choice_by_clip", random_flip="flip_by_clip",
                            augmentations=("brightness", "contrast", "rotation"), crop=crop, num_frames=2)


# name: (H0, W0, min_size, crop, seed of the draws); the crop cases must draw a flip (asserted in frame_case)
FRAME_CASES = {
    "crop360": (720, 1280, 360, ("absolute_range", (480, 640)), 244),
    "nocrop361": (720, 1280, 203, None, 11),                             # W1 = 361: > 256 and W1 % 4 != 0
}
MASK_CASES = {
    "m480": (480, 854, 241, ("absolute_range", (300, 480)), 1),         # W0 % 32 != 0; 241 x 315 output: odd planes
    "m720": (720, 1280, 361, None, 7),                                   # 361 x 642: planes start 2 bytes off a word
}


@functools.lru_cache(maxsize=None)
def frame_case(name):
    """-> (frames u8 [2,3,H0,W0], params f32 [2,16], (H1, W1), ref u8, band, excluded)"""
    H0, W0, size, crop, seed = FRAME_CASES[name]
    fr = synth.smooth_frames_u8(100 + seed, 1, 2, H0, W0)
    P, hw = _augmentation(size, crop).sample(2, H0, W0, rng=np.random.RandomState(seed))
    assert (P[:, 10] != 1).all() and (P[:, 11] != 1).all() and (P[:, 12] < 0).all() and (np.abs(P[:, 1]) > 1e-3).all()
    if crop is not None:
        assert (P[:, 0] < 0).all() and min(hw) == size, (P[:, 0], hw)    # flipped; short edge of the output
    else:
        assert hw[1] > 256 and hw[1] % 4 != 0, hw
    assert (P[:, 10:12] < 1).all(), P[:, 10:12]                          # gains below 1: see the module docstring
    ref, band, excl = warp_frames_f64(fr, P, hw)
    for a in (fr, P, ref, band, excl):
        a.setflags(write=False)
    return fr, P, hw, ref, band, excl


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """-> (planes u8 [P,H0,W0], plane_of int32 [T,S], masks u8 [S,T,H0,W0] (the same planes per slot), params, (H1, W1), ref u8
    [S,T,H1,W1], ambiguous): T = 2, S = 4 with dummy slots"""
    H0, W0, size, crop, seed = MASK_CASES[name]
    T, S, n = 2, 4, 3
    m, _ = synth.ellipse_targets(200 + seed, 2, n, T, H0, W0, sparse=0.0)
    planes = np.ascontiguousarray((m > 0).astype(np.uint8).reshape(n * T, H0, W0))
    yy, xx = np.mgrid[0:H0, 0:W0]
    for k in range(n * T):                                               # a coarse lattice under the ellipses: edges all over the plane
        planes[k] |= ((yy // (13 + k) + xx // (17 + 2 * k)) % 3 == 0).astype(np.uint8)
    planes[0, -1, :] = 1; planes[1, :, -1] = 1; planes[2, 0, :] = 1; planes[3, :, 0] = 1      # the frame's own edges
    plane_of = np.array([[0, -1, 2, 4], [1, 3, -1, 5]], np.int32)
    P, hw = _augmentation(size, crop).sample(T, H0, W0, rng=np.random.RandomState(seed))
    assert hw[1] % 4 != 0 and (hw[0] * hw[1]) % 4 != 0, hw
    u8 = np.zeros((S, T, H0, W0), np.uint8)
    for t in range(T):
        for s in range(S):
            if plane_of[t, s] >= 0:
                u8[s, t] = planes[plane_of[t, s]]
    ref, amb = warp_masks_f64(u8, P, hw)
    for a in (planes, plane_of, u8, P, ref, amb):
        a.setflags(write=False)
    return planes, plane_of, u8, P, hw, ref, amb


# copy-paste through s2d_copy_paste_frame_u8: target 720 x 1278, source 480 x 854; two consecutive frames' geometry
PASTE_H, PASTE_W, PASTE_HS, PASTE_WS = 720, 1278, 480, 854
PASTE_GEO = [(613, 1087, 107, 191), (577, 1031, 0, 247)]                 # frame 0 ends in the last row and column of the target
PASTE_KN = [(1, 0), (5, 3), (64, 2)]


@functools.lru_cache(maxsize=None)
def paste_inputs(K, N):
    """-> (src_frame u8 [3,Hs,Ws], src_masks u8 [K,Hs,Ws], tgt_frames u8 [2,3,H,W], tgt_masks u8 [2,N,H,W]); every source mask
    family has one member set in its last row and last column, target 0 reaches the target's last row and column"""
    sf = synth.smooth_frames_u8(300 + K, 1, 1, PASTE_HS, PASTE_WS)[0]
    tf = synth.smooth_frames_u8(400 + K, 1, 2, PASTE_H, PASTE_W)
    base, _ = synth.ellipse_targets(500 + K, 2, min(K, 6), 1, PASTE_HS, PASTE_WS, sparse=0.0, rmin=20.0, rmax=90.0)
    base = (base[:, 0] > 0).astype(np.uint8)
    sm = np.stack([np.roll(base[k % len(base)], (7 * (k // len(base)), 11 * (k // len(base))), (0, 1)) for k in range(K)])
    sm[0, -1, :] = 1; sm[0, :, -1] = 1
    sm[K - 1, -1, -1] = 1; sm[K - 1, 0, 0] = 1
    tm = np.zeros((2, N, PASTE_H, PASTE_W), np.uint8)
    if N:
        t, _ = synth.ellipse_targets(600 + K, 2, N, 2, PASTE_H, PASTE_W, sparse=0.0, rmin=60.0, rmax=200.0)
        tm = np.ascontiguousarray((t > 0).astype(np.uint8).transpose(1, 0, 2, 3))
        tm[:, 0, -1, :] = 1; tm[:, 0, :, -1] = 1; tm[:, 0, :, 0] = 1
    for a in (sf, sm, tf, tm):
        a.setflags(write=False)
    return sf, sm, tf, tm


# s2d_copy_paste_u8 / s2d_copy_paste_overlap: T = 2, target 200 x 300, K = 3, N = 2, one keep entry 0
CLIP_GEO = [(151, 227, 49, 73), (173, 260, 11, 0)]
CLIP_KEEP = (1, 0, 1)


@functools.lru_cache(maxsize=None)
def clip_inputs():
    """-> (src_frame u8 [3,120,182], src_masks u8 [3,120,182], tgt_frames u8 [2,3,200,300], tgt_masks u8 [2(N),2(T),200,300])"""
    sf = synth.smooth_frames_u8(700, 1, 1, 120, 182)[0]
    tf = synth.smooth_frames_u8(701, 1, 2, 200, 300)
    sm, _ = synth.ellipse_targets(702, 2, 3, 1, 120, 182, sparse=0.0, rmin=10.0, rmax=40.0)
    sm = np.ascontiguousarray((sm[:, 0] > 0).astype(np.uint8))
    sm[1, -1, :] = 1; sm[2, :, -1] = 1
    tm, _ = synth.ellipse_targets(703, 2, 2, 2, 200, 300, sparse=0.0, rmin=30.0, rmax=80.0)
    tm = (tm > 0).astype(np.uint8)
    tm[0, :, -1, :] = 1; tm[1, :, :, -1] = 1
    for a in (sf, sm, tf, tm):
        a.setflags(write=False)
    return sf, sm, tf, tm


# --------------------------------------------------------------------------- the CPU checks
def test_float32_mirror_of_the_frame_warp_stays_inside_the_band():
    from oracle import oracle_np
    for name in FRAME_CASES:
        fr, P, hw, ref, band, excl = frame_case(name)
        check_levels(f"mirror frames {name}", oracle_np.aug_warp_frames(fr, P, hw), ref, band, excl)


def test_float32_mirror_of_the_mask_warp_stays_inside_the_band():
    from oracle import oracle_np
    for name in MASK_CASES:
        _, _, u8, P, hw, ref, amb = mask_case(name)
        assert ref.any(axis=(2, 3)).sum() == 6 and not ref[1, 0].any() and not ref[2, 1].any()      # dummy slots stay empty
        check_exact(f"mirror masks {name}", oracle_np.aug_warp_masks(u8, P, hw), ref, amb)


def test_crop_mean_written_back_is_the_float32_of_the_exact_mean():
    """what params[12] must hold after the call, against the mirror's own statement of it on a small crop"""
    fr, P = frame_case("crop360")[:2]
    m64, m32 = crop_mean_f64(fr[0], P[0])
    assert abs(float(m32) - m64) <= 2 * 2.0 ** -24 * m64 and 0 < m64 < 281


def test_torch_interpolate_stays_inside_the_band_of_the_paste_reference():
    """CPU F.interpolate (what the reference calls) against paste_frame_f64 on the GPU module's inputs: both frames of (K, N) = (5, 3),
    the second resizing the first's canvas, and the small clip"""
    sf, sm, tf, tm = paste_inputs(5, 3)
    cur = sm
    for f, geo in enumerate(PASTE_GEO):
        ref = paste_frame_f64(sf, cur, tf[f], tm[f], geo)
        assert ref["alpha"].any() and ref["inter"].any() and (ref["alive"] < ref["tarea"]).any()
        check_paste(f"torch paste frame {f}", paste_frame_torch(sf, cur, tf[f], tm[f], geo), ref)
        cur = ref["canvas"]
    assert ref["canvas"][:, PASTE_GEO[1][2]:, :].any()
    sf, sm, tf, tm = clip_inputs()
    for t, geo in enumerate(CLIP_GEO):
        ref = paste_frame_f64(sf, sm, tf[t], tm[:, t], geo, keep=CLIP_KEEP)
        check_paste(f"torch clip frame {t}", paste_frame_torch(sf, sm, tf[t], tm[:, t], geo, keep=CLIP_KEEP), ref)


def test_paste_reference_edges():
    """hand cases of the tap rule: an identity resize copies; the last destination row / column never reads past the source; a
    destination pixel whose second weight is zero takes one tap only"""
    rng = np.random.default_rng(0)
    m = (rng.random((2, 9, 13)) < 0.4).astype(np.uint8)
    f = rng.integers(0, 256, (3, 9, 13), dtype=np.uint8)
    tf = rng.integers(0, 256, (3, 12, 20), dtype=np.uint8)
    tm = (rng.random((1, 12, 20)) < 0.5).astype(np.uint8)
    ref = paste_frame_f64(f, m, tf, tm, (9, 13, 2, 5))
    np.testing.assert_array_equal(ref["canvas"][:, 2:11, 5:18], m)
    a = ref["alpha"][2:11, 5:18]
    np.testing.assert_array_equal(ref["frame"][:, 2:11, 5:18], np.where(a, f, tf[:, 2:11, 5:18]))
    np.testing.assert_array_equal(ref["inter"][:, 0], [(ref["canvas"][k] & tm[0]).sum() for k in range(2)])
    i0, i1, has1, _ = _axis_taps(3, 9, 3)                               # scale 3: s = 1, 4, 7 exactly -> one tap
    assert i0.tolist() == [1, 4, 7] and not has1.any()
    i0, i1, has1, _ = _axis_taps(20, 9, 20)
    assert i1.max() == 8 and i0[-1] == 8 and i1[-1] == 8 and not has1[-1]


def test_shift_planes_np_is_the_translate_of_the_reference():
    rng = np.random.default_rng(1)
    p = rng.integers(0, 3, (5, 7), dtype=np.uint8) * 127
    out = shift_planes_np([p, p, p], [(0, 0), (2, -1), (-7, 0)])
    np.testing.assert_array_equal(out[0], p != 0)
    for y in range(5):
        for x in range(7):
            sy, sx = y - 1, x + 2
            assert out[1, y, x] == (p[sy, sx] != 0 if 0 <= sy < 5 and 0 <= sx < 7 else 0)
    assert not out[2].any() and out.max() == 1
