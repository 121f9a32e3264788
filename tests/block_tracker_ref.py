"""Shared helpers of the block-tracker tests (not a test module).

* `grey_ref`, `block_track_ref`: numpy restatements of s2d_video_grey_u8 and s2d_block_track_u8 (include/s2d_hip.h).  Both
  kernels make integer decisions only, so the device output has to equal these bit for bit.
* textured scenes: the geometry of tests/golden/keymask_stub_tracker.py (SCENES, label_map), but every object and the
  background carry their own random RGB texture of 2 x 2-pixel cells, and an object's texture moves with it.
* `truth`: a point moves by the step of the object under it in the query frame.
* `clean`: the continuously clean point-frames, where the true position has cost 0 and the tracker must therefore be exact
  (unless the texture repeats), and `replaced`, where the whole patch at the true position shows another texture.
* `CALLS`: the stage-1 tracker calls (video, query frame, object) that the CPU and the GPU test both check."""
import functools
import os

import numpy as np
from PIL import Image

from tests.golden import keymask_stub_tracker as S

R, SEARCH, TAU = 5, 16, 12               # BlockTracker's defaults
TEXTURE_SEED = 20240

# (video, query frame, object index): stage 1 tracks the mask of every object of every frame on grid 50, backward from frame 1
# on.  The subset holds vid_b object 0 sliding under object 4, vid_a object 3 absent in frames 6-8, vid_a object 2 at 12 px per
# frame, and query frames > 0 (backward tracking).
CALLS = (("vid_a", 0, 2), ("vid_a", 0, 3), ("vid_a", 4, 3), ("vid_a", 5, 2), ("vid_a", 9, 0),
         ("vid_b", 0, 0), ("vid_b", 0, 4), ("vid_b", 5, 0), ("vid_b", 4, 2), ("vid_b", 8, 1))


# ---------------------------------------------------------------------------------------------------------------- the kernels
def grey_ref(video):
    """video f32 [T,3,H,W] -> u8 [T,H,W]"""
    v = np.asarray(video, np.float32)
    c = np.rint(np.clip(np.where(np.isnan(v), np.float32(0), v), 0, 255)).astype(np.int64)      # rint: half to even
    return ((77 * c[:, 0] + 150 * c[:, 1] + 29 * c[:, 2] + 128) >> 8).astype(np.uint8)


def _patches(frame, cx, cy, half):
    """int32 [N, 2 half + 1, 2 half + 1]: the window round every (cx, cy), border replicate"""
    H, W = frame.shape
    o = np.arange(-half, half + 1)
    yy = np.clip(cy[:, None] + o[None], 0, H - 1)
    xx = np.clip(cx[:, None] + o[None], 0, W - 1)
    return frame[yy[:, :, None], xx[:, None, :]].astype(np.int32)


def block_track_ref(grey, points, q, backward, R=R, S=SEARCH, tau=TAU):
    """grey u8 [T,H,W], points int [N,2] (x, y) -> (tracks f32 [T,N,2], vis u8 [T,N])"""
    T, H, W = grey.shape
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    N, P, C = len(pts), 2 * R + 1, 2 * S + 1
    tracks = np.zeros((T, N, 2), np.float32)
    vis = np.zeros((T, N), np.uint8)
    tracks[:q + 1] = pts[None]
    vis[q] = 1
    if N == 0:
        return tracks, vis
    tm = _patches(grey[q], pts[:, 0], pts[:, 1], R)
    d = np.arange(-S, S + 1)
    d2 = (d[:, None] ** 2 + d[None, :] ** 2).astype(np.int64)                                    # [dy, dx]
    # the lexicographic order (cost, d2, dy, dx) as one integer: d2 < 2^11, dy + S and dx + S < 2^6
    tie = (d2 << 12) | ((d[:, None] + S) << 6) | (d[None, :] + S)
    for step in ((1, -1) if backward else (1,)):
        cx, cy = pts[:, 0].copy(), pts[:, 1].copy()
        for t in range(q + step, T if step > 0 else -1, step):
            reg = _patches(grey[t], cx, cy, R + S)
            cost = np.zeros((N, C, C), np.int64)
            for j in range(P):
                for i in range(P):
                    cost += np.abs(reg[:, j:j + C, i:i + C] - tm[:, j, i][:, None, None])
            ny, nx = cy[:, None, None] + d[None, :, None], cx[:, None, None] + d[None, None, :]
            valid = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
            key = np.where(valid, (cost << 23) | tie[None], np.iinfo(np.int64).max).reshape(N, -1)
            best = key.min(1)
            visible = (best >> 23) <= tau * P * P
            cx = np.where(visible, cx + (best & 63) - S, cx)
            cy = np.where(visible, cy + ((best >> 6) & 63) - S, cy)
            tracks[t, :, 0], tracks[t, :, 1], vis[t] = cx, cy, visible
    return tracks, vis


def grid_ref(grid_size, H, W):
    """the stub tracker's grid as int [g*g, 2] of (x, y)"""
    ys = (np.arange(grid_size) * 2 + 1) * H // (2 * grid_size)
    xs = (np.arange(grid_size) * 2 + 1) * W // (2 * grid_size)
    gy, gx = (a.reshape(-1) for a in np.meshgrid(ys, xs, indexing="ij"))
    return np.stack([gx, gy], -1)


# ------------------------------------------------------------------------------------------------------------ textured scenes
def _texture(rng, h, w):
    cells = rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 3), dtype=np.uint8)
    return np.repeat(np.repeat(cells, 2, 0), 2, 1)[:h, :w]


@functools.lru_cache(maxsize=None)
def textured_video(name):
    """u8 [T,H,W,3] (read-only)"""
    sc = S.SCENES[name]
    T, H, W = sc["T"], sc["H"], sc["W"]
    rng = np.random.default_rng([TEXTURE_SEED, sorted(S.SCENES).index(name)])
    bg = _texture(rng, H, W)
    tex = [_texture(rng, o["box"][2], o["box"][3]) for o in sc["objects"]]
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        lab = S.label_map(sc, t)
        frame = bg.copy()
        for i, o in enumerate(sc["objects"]):
            y0, x0 = o["box"][0] + o["step"][0] * t, o["box"][1] + o["step"][1] * t
            m = lab == i + 1
            frame[m] = tex[i][yy[m] - y0, xx[m] - x0]
        out[t] = frame
    out.setflags(write=False)
    return out


def video_f32(name):
    """f32 [T,3,H,W], the tracker's layout without the batch axis"""
    return np.ascontiguousarray(textured_video(name).transpose(0, 3, 1, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def textured_grey(name):
    g = grey_ref(video_f32(name))
    g.setflags(write=False)
    return g


def write_textured_dataset(root):
    """S.write_dataset with the textured frames (the colour masks are the stub's)"""
    for name, sc in S.SCENES.items():
        fd, md = os.path.join(root, S.FRAMES_DIR, name), os.path.join(root, S.MASKS_DIR, name)
        os.makedirs(fd, exist_ok=True)
        os.makedirs(md, exist_ok=True)
        for t in range(sc["T"]):
            Image.fromarray(textured_video(name)[t]).save(os.path.join(fd, f"{t:05d}.png"))
            Image.fromarray(S.render(sc, t)[1]).save(os.path.join(md, f"{t:05d}.png"))


class TruthTracker(S.StubTracker):
    """the stub tracker (ground-truth motion and occlusion), recognising the scenes by their textured first frames"""

    def __init__(self):
        super().__init__()
        self.first = {name: textured_video(name)[0] for name in S.SCENES}


# ------------------------------------------------------------------------------------------------------------------ the truth
# `scenes`: the table that holds scene `name` (tests/live_tracker_ref.py passes its own)
def call_mask(name, q, obj, scenes=S.SCENES):
    """u8 [H,W] with {0,255}: the stage-1 mask of object `obj` in frame q"""
    return ((S.label_map(scenes[name], q) == obj + 1) * 255).astype(np.uint8)


def call_points(name, q, obj, scenes=S.SCENES):
    sc = scenes[name]
    g = grid_ref(50, sc["H"], sc["W"])
    return g[call_mask(name, q, obj, scenes)[g[:, 1], g[:, 0]] > 0]


def truth(name, q, points, obj, scenes=S.SCENES):
    """int [T,N,2]: every point moved by the object's step per frame"""
    sc = scenes[name]
    dy, dx = sc["objects"][obj]["step"]
    dt = np.arange(sc["T"])[:, None] - q
    return np.stack([points[None, :, 0] + dx * dt, points[None, :, 1] + dy * dt], -1)


def _patch_labels(name, t, xy, R, scenes):
    """(int [N,P,P] labels of the patch round xy in frame t, bool [N] the patch lies inside the frame)"""
    sc = scenes[name]
    H, W = sc["H"], sc["W"]
    inside = (xy[:, 0] - R >= 0) & (xy[:, 0] + R < W) & (xy[:, 1] - R >= 0) & (xy[:, 1] + R < H)
    return _patches(S.label_map(sc, t), xy[:, 0], xy[:, 1], R), inside


def clean(name, q, points, obj, backward, R=R, S_=SEARCH, scenes=S.SCENES):
    """bool [T,N]: point-frame (t, n) is continuously clean -- at every frame from q to t the (2R+1)^2 patch at the true position
    lies wholly inside the frame and shows the point's object only, and the object steps by at most S per axis"""
    sc = scenes[name]
    T = sc["T"]
    tr = truth(name, q, points, obj, scenes)
    ok = np.zeros((T, len(points)), bool)
    if max(abs(s) for s in sc["objects"][obj]["step"]) > S_:
        return ok
    for t in range(T):
        lab, inside = _patch_labels(name, t, tr[t], R, scenes)
        ok[t] = inside & (lab == obj + 1).all((1, 2))
    out = np.zeros_like(ok)
    out[q:] = np.logical_and.accumulate(ok[q:], 0)
    if backward:
        out[:q + 1] = np.logical_and.accumulate(ok[q::-1], 0)[::-1]
    return out


def replaced(name, q, points, obj, backward, R=R, scenes=S.SCENES):
    """bool [T,N]: the whole patch at the true position lies inside the frame and shows only other textures (another object's
    or the background's).  A true position whose patch leaves the frame shows nothing and is not claimed."""
    sc = scenes[name]
    tr = truth(name, q, points, obj, scenes)
    out = np.zeros((sc["T"], len(points)), bool)
    for t in range(0 if backward else q, sc["T"]):
        lab, inside = _patch_labels(name, t, tr[t], R, scenes)
        out[t] = inside & (lab != obj + 1).all((1, 2))
    return out


@functools.lru_cache(maxsize=None)
def reference_call(name, q, obj):
    """(points int [N,2], tracks f32 [T,N,2], vis u8 [T,N]) of the numpy tracker for one stage-1 call; computed once and shared
    (read-only)"""
    pts = call_points(name, q, obj)
    tracks, vis = block_track_ref(textured_grey(name), pts, q, q > 0)
    for a in (pts, tracks, vis):
        a.setflags(write=False)
    return pts, tracks, vis
