"""Shared helpers of the zero-mean tracker tests (not a test module).

* `zm_track_ref`: a numpy restatement of s2d_block_track_zm_u8 (include/s2d_hip.h), with `mean`, `zcost` and `dev` of its rule.
  The kernel makes integer decisions only, so the device output has to equal it bit for bit.  Points are worked through in
  chunks on the window of absolute positions of tests/live_tracker_ref.py, so S = 64 stays within memory.
* the *squeezed* scenes: the textured scenes of tests/block_tracker_ref.py with every RGB value c mapped to 48 + (c * 5) // 8
  (48 .. 207), and the *lit* scenes: the squeezed ones plus k_t = (-1)^t min(5 t, 40) on all three channels of frame t.  The grey
  weights sum to 256, so the grey frame moves by exactly k_t, and nothing saturates; `lit_grey` asserts both.
* FLAT: an object of one colour stepping 3 px per frame over a textured background, beside a textured object; `flat_truth`,
  `flat_clean` in the sense of block_tracker_ref.truth / clean, which serve the lit scenes as they are (the geometry is theirs).
* `edge_case`, `checker_case`: the hand-built frames of the threshold and largest-cost tests, shared by the CPU and the GPU test."""
import functools
import os

import numpy as np
from PIL import Image

from tests import block_tracker_ref as B
from tests import live_tracker_ref as L
from tests.golden import keymask_stub_tracker as S

R, SEARCH, TAU, REFRESH, TEXTURE = 5, 32, 12, -1, 4          # ZeroMeanBlockTracker's defaults
LIT_SEARCH = 16                                              # the search of the lit calls (block_tracker_ref's, so `clean` is shared)


def light(t):
    """the brightness offset of frame t of a lit scene"""
    return (-1) ** t * min(5 * t, 40)


# ----------------------------------------------------------------------------------------------------------------- the kernel
def mean(sums, n):
    """the rounded mean of patches of n bytes with these sums: half rounds up"""
    return (2 * sums + n) // (2 * n)


def zcost(a, b):
    """zero-mean cost of two patches (any equal shape)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return int(np.abs((a - mean(a.sum(), a.size)) - (b - mean(b.sum(), b.size))).sum())


def dev(a):
    a = np.asarray(a, np.int64)
    return int(np.abs(a - mean(a.sum(), a.size)).sum())


def _template(patch):
    """u8 [n,P,P] -> int16 [n,P,P] with the rounded mean removed"""
    p = patch.astype(np.int64)
    return (p - mean(p.sum((1, 2)), p.shape[1] * p.shape[2])[:, None, None]).astype(np.int16)


def _track_chunk(grey, pts, q, backward, R, S, tau, tau_u, tracks, vis):
    T, H, W = grey.shape
    P = 2 * R + 1
    nn = P * P
    Cy, Cx = min(2 * S + 1, H), min(2 * S + 1, W)
    n = len(pts)
    big = np.iinfo(np.int64).max
    for step in ((1, -1) if backward else (1,)):
        cx, cy = pts[:, 0].copy(), pts[:, 1].copy()
        A = _template(L._window(grey[q], cy - R, cx - R, P, P))                      # L_i - mean(L), int16 [n,P,P]
        for t in range(q + step, T if step > 0 else -1, step):
            wy0, wx0 = np.clip(cy - S, 0, H - Cy), np.clip(cx - S, 0, W - Cx)        # as in live_tracker_ref
            reg = L._window(grey[t], wy0 - R, wx0 - R, Cy + 2 * R, Cx + 2 * R)
            c = np.zeros((n, Cy + 2 * R + 1, Cx + 2 * R + 1), np.int64)
            c[:, 1:, 1:] = reg.astype(np.int64).cumsum(1).cumsum(2)
            sums = c[:, P:, P:] - c[:, :-P, P:] - c[:, P:, :-P] + c[:, :-P, :-P]     # the patch sum of every candidate, [n,Cy,Cx]
            mx = mean(sums, nn).astype(np.int16)
            reg = reg.astype(np.int16)
            cost = np.zeros((n, Cy, Cx), np.int32)                                   # 510 * 15^2 < 2^17
            for j in range(P):
                for i in range(P):
                    cost += np.abs(reg[:, j:j + Cy, i:i + Cx] - mx - A[:, j, i][:, None, None])
            dy = wy0[:, None] + np.arange(Cy)[None] - cy[:, None]
            dx = wx0[:, None] + np.arange(Cx)[None] - cx[:, None]
            valid = (np.abs(dy) <= S)[:, :, None] & (np.abs(dx) <= S)[:, None, :]
            tie = ((dy[:, :, None] ** 2 + dx[:, None, :] ** 2) << 16) | ((dy[:, :, None] + S) << 8) | (dx[:, None, :] + S)
            key = np.where(valid, (cost.astype(np.int64) << 30) | tie, big).reshape(n, -1)
            best = key.min(1)
            bc = best >> 30
            visible = bc <= tau * nn
            cx = np.where(visible, cx + (best & 255) - S, cx)
            cy = np.where(visible, cy + ((best >> 8) & 255) - S, cy)
            tracks[t, :, 0], tracks[t, :, 1], vis[t] = cx, cy, visible
            refresh = visible & (bc <= tau_u * nn)                                   # tau_u = -1: never
            if refresh.any():
                A[refresh] = _template(L._window(grey[t], cy[refresh] - R, cx[refresh] - R, P, P))


def zm_track_ref(grey, points, q, backward, R=R, S=SEARCH, tau=TAU, tau_u=REFRESH, texture=TEXTURE):
    """grey u8 [T,H,W], points int [N,2] (x, y) -> (tracks f32 [T,N,2], vis u8 [T,N], trackable u8 [N])"""
    grey = np.asarray(grey)
    T, H, W = grey.shape
    if not (1 <= R <= 7 and 1 <= S <= 64 and 0 <= tau <= 255 and -1 <= tau_u <= tau and 0 <= texture <= 127 and 0 <= q < T
            and H < 1 << 15 and W < 1 << 15):
        raise ValueError("outside the contract of s2d_block_track_zm_u8")
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    pts = np.stack([np.clip(pts[:, 0], 0, W - 1), np.clip(pts[:, 1], 0, H - 1)], -1)
    N, P = len(pts), 2 * R + 1
    tracks = np.zeros((T, N, 2), np.float32)
    vis = np.zeros((T, N), np.uint8)
    tracks[:] = pts[None]                                                            # an untrackable point stays at p throughout
    vis[q] = 1
    tm = _template(L._window(grey[q], pts[:, 1] - R, pts[:, 0] - R, P, P)).astype(np.int64)
    trackable = np.abs(tm).sum((1, 2)) >= texture * P * P
    idx = np.flatnonzero(trackable)
    chunk = max(1, (1 << 19) // (min(2 * S + 1, H) * min(2 * S + 1, W)))             # about 0.5 M costs at a time
    for a in range(0, len(idx), chunk):
        sel = idx[a:a + chunk]
        tr, vs = tracks[:, sel], vis[:, sel]                                         # copies: fancy indexing
        _track_chunk(grey, pts[sel], q, backward, R, S, tau, tau_u, tr, vs)
        tracks[:, sel], vis[:, sel] = tr, vs
    return tracks, vis, trackable.astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------- the scenes
def squeeze(rgb):
    """u8 RGB -> 48 + (c * 5) // 8, in 48 .. 207"""
    return (48 + (rgb.astype(np.int64) * 5) // 8).astype(np.uint8)


def _lit(frames):
    """u8 [T,H,W,3] squeezed frames -> the lit frames"""
    k = np.array([light(t) for t in range(len(frames))], np.int64)
    out = frames.astype(np.int64) + k[:, None, None, None]
    assert out.min() >= 0 and out.max() <= 255                                      # nothing saturates
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def squeezed_video(name):
    """u8 [T,H,W,3] (read-only)"""
    v = squeeze(B.textured_video(name))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def lit_video(name):
    v = _lit(squeezed_video(name))
    v.setflags(write=False)
    return v


def video_f32(frames):
    """u8 [T,H,W,3] -> f32 [T,3,H,W], the tracker's layout without the batch axis"""
    return np.ascontiguousarray(frames.transpose(0, 3, 1, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def squeezed_grey(name):
    g = B.grey_ref(video_f32(squeezed_video(name)))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def lit_grey(name):
    g = B.grey_ref(video_f32(lit_video(name)))
    k = np.array([light(t) for t in range(len(g))], np.int64)
    assert np.array_equal(g.astype(np.int64), squeezed_grey(name).astype(np.int64) + k[:, None, None])   # exactly k_t
    assert g.min() > 0 and g.max() < 255
    g.setflags(write=False)
    return g


def write_dataset(root, lit):
    """block_tracker_ref.write_textured_dataset with the lit (or the squeezed) frames; the colour masks are the stub's"""
    for name, sc in S.SCENES.items():
        fd, md = os.path.join(root, S.FRAMES_DIR, name), os.path.join(root, S.MASKS_DIR, name)
        os.makedirs(fd, exist_ok=True)
        os.makedirs(md, exist_ok=True)
        frames = lit_video(name) if lit else squeezed_video(name)
        for t in range(sc["T"]):
            Image.fromarray(frames[t]).save(os.path.join(fd, f"{t:05d}.png"))
            Image.fromarray(S.render(sc, t)[1]).save(os.path.join(md, f"{t:05d}.png"))


class LitTruthTracker(S.StubTracker):
    """the stub tracker (ground-truth motion and occlusion), recognising the scenes by their lit first frames"""

    def __init__(self):
        super().__init__()
        self.first = {name: lit_video(name)[0] for name in S.SCENES}


# the flat object (index 0) and a textured one (index 1), both stepping 3 px per frame over a textured background
FLAT = dict(T=6, H=96, W=160, objects=[
    dict(color=(200, 40, 40), shade=(120, 120, 120), box=(10, 12, 44, 56), step=(0, 3), absent=()),
    dict(color=(40, 40, 200), shade=(70, 80, 190), box=(60, 84, 30, 40), step=(0, 3), absent=()),
])
FLAT_SEED = 20260


@functools.lru_cache(maxsize=None)
def flat_grey():
    """u8 [T,H,W] (read-only): object 0 has the one colour of its `shade`, object 1 and the background are textured"""
    sc = FLAT
    T, H, W = sc["T"], sc["H"], sc["W"]
    rng = np.random.default_rng(FLAT_SEED)
    bg = squeeze(B._texture(rng, H, W))
    o1 = sc["objects"][1]
    tex = squeeze(B._texture(rng, o1["box"][2], o1["box"][3]))
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        lab = S.label_map(sc, t)
        frame = bg.copy()
        frame[lab == 1] = sc["objects"][0]["shade"]
        m = lab == 2
        frame[m] = tex[yy[m] - o1["box"][0] - o1["step"][0] * t, xx[m] - o1["box"][1] - o1["step"][1] * t]
        out[t] = frame
    g = B.grey_ref(video_f32(out))
    g.setflags(write=False)
    return g


def flat_points(obj, q=0):
    g = B.grid_ref(24, FLAT["H"], FLAT["W"])
    return g[S.label_map(FLAT, q)[g[:, 1], g[:, 0]] == obj + 1]


def flat_truth(q, points, obj):
    """int [T,N,2]: every point moved by the object's step per frame"""
    dy, dx = FLAT["objects"][obj]["step"]
    dt = np.arange(FLAT["T"])[:, None] - q
    return np.stack([points[None, :, 0] + dx * dt, points[None, :, 1] + dy * dt], -1)


def flat_clean(q, points, obj, R=R):
    """bool [T,N], forward from q: continuously clean in the sense of block_tracker_ref.clean"""
    H, W = FLAT["H"], FLAT["W"]
    tr = flat_truth(q, points, obj)
    ok = np.zeros((FLAT["T"], len(points)), bool)
    for t in range(q, FLAT["T"]):
        xy = tr[t]
        inside = (xy[:, 0] - R >= 0) & (xy[:, 0] + R < W) & (xy[:, 1] - R >= 0) & (xy[:, 1] + R < H)
        ok[t] = inside & (B._patches(S.label_map(FLAT, t), xy[:, 0], xy[:, 1], R) == obj + 1).all((1, 2))
    ok[q:] = np.logical_and.accumulate(ok[q:], 0)
    return ok


# ------------------------------------------------------------------------------------------------------------ hand-built cases
EDGE_R, EDGE_S = 1, 4
EDGE_PATCH = np.array([[90, 140, 60], [150, 100, 170], [70, 160, 120]], np.int64)


def edge_case():
    """(grey u8 [3,16,20], point [1,2]): R = 1.  A 3 x 3 patch on a flat ground moves by (2, 1) per frame; in frame 1 its centre
    pixel is 81 higher than in frame 0, in frame 2 its top-left pixel is 81 higher as well.  81 = 9 n: the patch sum moves by
    81, the rounded mean by exactly 9, so against the frame-0 patch the frame-1 patch costs 8 * 9 + 72 = 144 = 16 n, and the
    frame-2 patch costs 144 against the frame-1 patch and 7 * 18 + 2 * 63 = 252 = 28 n against the frame-0 patch."""
    grey = np.full((3, 16, 20), 100, np.uint8)
    p = EDGE_PATCH.copy()
    for t in range(3):
        if t == 1:
            p[1, 1] += 81
        if t == 2:
            p[0, 0] += 81
        grey[t, 5 + t:8 + t, 6 + 2 * t:9 + 2 * t] = p
    return grey, np.array([(7, 6)])


def edge_patch(grey, t):
    return grey[t, 5 + t:8 + t, 6 + 2 * t:9 + 2 * t]


def dev_case():
    """(grey u8 [2,12,12], point): R = 1, a patch of 100 with one pixel at 118 and one at 82 on a ground of 100:
    dev = 36 = 4 n exactly"""
    grey = np.full((2, 12, 12), 100, np.uint8)
    grey[:, 5, 5], grey[:, 7, 7] = 118, 82
    return grey, np.array([(6, 6)])


CHECKER_R, CHECKER_S = 7, 64


def checker_case():
    """(grey u8 [2,40,48], points): a one-pixel 0 / 255 checkerboard and its inverse.  Every candidate at an even dx + dy shows
    the inverse of the template, the largest cost there is; every odd one costs 0."""
    yy, xx = np.mgrid[0:40, 0:48]
    a = (((yy + xx) & 1) * 255).astype(np.uint8)
    return np.stack([a, 255 - a]), np.array([(24, 20), (9, 30), (40, 8)])


# ------------------------------------------------------------------------------------- references, computed once and shared
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference_call(kind, name, q, obj, texture=TEXTURE):
    """(points, tracks, vis, trackable) of zm_track_ref for one call of block_tracker_ref.CALLS on the "lit" or the "squeezed"
    scene at search 16 with the fixed template, backward when q > 0 (read-only)"""
    grey = lit_grey(name) if kind == "lit" else squeezed_grey(name)
    pts = B.call_points(name, q, obj)
    return _frozen(pts, *zm_track_ref(grey, pts, q, q > 0, R, LIT_SEARCH, TAU, REFRESH, texture))


@functools.lru_cache(maxsize=None)
def reference_default_call(name, q, obj):
    """the same on the lit scene with every default (search 32)"""
    pts = B.call_points(name, q, obj)
    return _frozen(pts, *zm_track_ref(lit_grey(name), pts, q, q > 0))
