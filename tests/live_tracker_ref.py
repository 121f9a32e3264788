"""Shared helpers of the live-template tracker tests (not a test module).

* `live_track_ref`: a numpy restatement of s2d_block_track_live_u8 (include/s2d_hip.h).  The kernel makes integer decisions
  only, so the device output has to equal it bit for bit.  It works through the points in chunks, and it evaluates the costs on
  a window of absolute positions of min(2S+1, H) x min(2S+1, W) that holds every candidate inside the frame, so that S = 64 stays
  within memory and a search window larger than the frame costs no more than the frame.
* two scenes in the dict layout of tests/golden/keymask_stub_tracker.py, rendered with block_tracker_ref._texture:
  FAST (two objects stepping by more than 24 px per frame, the largest search radius of s2d_block_track_u8, and a static one)
  and DRIFT (objects stepping 5-7 px whose 2 x 2 texture cells each change by their own fixed integer in -3..3 per frame).
* `truth`, `clean`, `replaced` in the sense of block_tracker_ref, for a scene dict.
* `FAST_CALLS`, `DRIFT_CALLS`: (query frame, object) of the tracker calls that the CPU and the GPU test both check; query
  frames > 0 track backward too, as stage 1 does."""
import functools

import numpy as np

from tests import block_tracker_ref as B
from tests.golden import keymask_stub_tracker as S

R, SEARCH, TAU, REFRESH = 5, 32, 12, 4          # LiveBlockTracker's defaults
FAST_SEARCH = 40
DRIFT_SEARCH = 16
TEXTURE_SEED = 20250

FAST = dict(T=6, H=120, W=216, objects=[
    dict(color=(40, 200, 40), shade=(60, 170, 90), box=(50, 92, 28, 36), step=(0, 0), absent=()),          # static, passed over
    dict(color=(200, 40, 40), shade=(180, 90, 60), box=(8, 4, 40, 48), step=(2, 30), absent=()),
    dict(color=(40, 40, 200), shade=(70, 80, 190), box=(76, 152, 36, 52), step=(-1, -26), absent=()),
])
DRIFT = dict(T=10, H=120, W=216, objects=[
    dict(color=(200, 40, 40), shade=(180, 90, 60), box=(10, 8, 44, 56), step=(1, 6), absent=()),
    dict(color=(40, 40, 200), shade=(70, 80, 190), box=(66, 150, 40, 50), step=(-1, -7), absent=()),
    dict(color=(210, 210, 40), shade=(200, 200, 120), box=(70, 20, 36, 44), step=(0, 5), absent=()),
])
SCENES = {"fast": FAST, "drift": DRIFT}
# (query frame, object index); backward tracking when the query frame is > 0
FAST_CALLS = ((0, 1), (0, 2), (3, 1), (3, 2))
DRIFT_CALLS = ((0, 0), (0, 1), (0, 2), (2, 0), (2, 1))


# ----------------------------------------------------------------------------------------------------------------- the kernel
def _window(frame, y0, x0, h, w):
    """u8 [N,h,w]: rows y0[n] .. y0[n] + h - 1 and columns x0[n] .. x0[n] + w - 1 of the frame, border replicate"""
    H, W = frame.shape
    yy = np.clip(y0[:, None] + np.arange(h)[None], 0, H - 1)
    xx = np.clip(x0[:, None] + np.arange(w)[None], 0, W - 1)
    return frame[yy[:, :, None], xx[:, None, :]]


def _track_chunk(grey, pts, q, backward, R, S, tau, tau_u, tracks, vis):
    T, H, W = grey.shape
    P = 2 * R + 1
    Cy, Cx = min(2 * S + 1, H), min(2 * S + 1, W)
    n = len(pts)
    big = np.iinfo(np.int64).max
    for step in ((1, -1) if backward else (1,)):
        cx, cy = pts[:, 0].copy(), pts[:, 1].copy()
        L = _window(grey[q], cy - R, cx - R, P, P)                                   # the live template, u8 [n,P,P]
        for t in range(q + step, T if step > 0 else -1, step):
            # absolute positions wy0 .. wy0 + Cy - 1: every candidate row inside the frame is among them (Cy = H: all rows)
            wy0, wx0 = np.clip(cy - S, 0, H - Cy), np.clip(cx - S, 0, W - Cx)
            reg = _window(grey[t], wy0 - R, wx0 - R, Cy + 2 * R, Cx + 2 * R)
            cost = np.zeros((n, Cy, Cx), np.uint16)                                  # 255 * 15^2 < 2^16
            for j in range(P):
                for i in range(P):
                    v, m = reg[:, j:j + Cy, i:i + Cx], L[:, j, i][:, None, None]
                    cost += np.maximum(v, m) - np.minimum(v, m)                      # |v - m| in u8
            dy = wy0[:, None] + np.arange(Cy)[None] - cy[:, None]                    # [n,Cy]
            dx = wx0[:, None] + np.arange(Cx)[None] - cx[:, None]                    # [n,Cx]
            valid = (np.abs(dy) <= S)[:, :, None] & (np.abs(dx) <= S)[:, None, :]
            # the lexicographic order (cost, d2, dy, dx) as one integer: d2 <= 2 * 64^2 < 2^14, dy + S and dx + S < 2^8
            tie = ((dy[:, :, None] ** 2 + dx[:, None, :] ** 2) << 16) | ((dy[:, :, None] + S) << 8) | (dx[:, None, :] + S)
            key = np.where(valid, (cost.astype(np.int64) << 30) | tie, big).reshape(n, -1)
            best = key.min(1)
            bc = best >> 30
            visible = bc <= tau * P * P
            cx = np.where(visible, cx + (best & 255) - S, cx)
            cy = np.where(visible, cy + ((best >> 8) & 255) - S, cy)
            tracks[t, :, 0], tracks[t, :, 1], vis[t] = cx, cy, visible
            refresh = visible & (bc <= tau_u * P * P)                                # tau_u = -1: never
            if refresh.any():
                L[refresh] = _window(grey[t], cy[refresh] - R, cx[refresh] - R, P, P)


def live_track_ref(grey, points, q, backward, R=R, S=SEARCH, tau=TAU, tau_u=REFRESH):
    """grey u8 [T,H,W], points int [N,2] (x, y) -> (tracks f32 [T,N,2], vis u8 [T,N])"""
    grey = np.asarray(grey)
    T, H, W = grey.shape
    if not (1 <= R <= 7 and 1 <= S <= 64 and 0 <= tau <= 255 and -1 <= tau_u <= tau and 0 <= q < T):
        raise ValueError("outside the contract of s2d_block_track_live_u8")
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    pts = np.stack([np.clip(pts[:, 0], 0, W - 1), np.clip(pts[:, 1], 0, H - 1)], -1)
    N = len(pts)
    tracks = np.zeros((T, N, 2), np.float32)
    vis = np.zeros((T, N), np.uint8)
    tracks[:q + 1] = pts[None]
    vis[q] = 1
    chunk = max(1, (1 << 19) // (min(2 * S + 1, H) * min(2 * S + 1, W)))            # about 0.5 M costs at a time
    for a in range(0, N, chunk):
        _track_chunk(grey, pts[a:a + chunk], q, backward, R, S, tau, tau_u, tracks[:, a:a + chunk], vis[:, a:a + chunk])
    return tracks, vis


# ----------------------------------------------------------------------------------------------------------------- the scenes
@functools.lru_cache(maxsize=None)
def scene_video(name):
    """u8 [T,H,W,3] (read-only): block_tracker_ref.textured_video for FAST and DRIFT; in DRIFT every 2 x 2 cell of an object's
    texture changes by its own fixed integer in -3..3 per frame (all three channels), clipped to 0..255"""
    sc = SCENES[name]
    T, H, W = sc["T"], sc["H"], sc["W"]
    rng = np.random.default_rng([TEXTURE_SEED, sorted(SCENES).index(name)])
    bg = B._texture(rng, H, W)
    tex = [B._texture(rng, o["box"][2], o["box"][3]).astype(np.int64) for o in sc["objects"]]
    rate = []
    for o in sc["objects"]:
        h, w = o["box"][2], o["box"][3]
        cells = rng.integers(-3, 4, ((h + 1) // 2, (w + 1) // 2)) if name == "drift" else np.zeros(((h + 1) // 2, (w + 1) // 2), np.int64)
        rate.append(np.repeat(np.repeat(cells, 2, 0), 2, 1)[:h, :w, None])
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        lab = S.label_map(sc, t)
        frame = bg.copy()
        for i, o in enumerate(sc["objects"]):
            y0, x0 = o["box"][0] + o["step"][0] * t, o["box"][1] + o["step"][1] * t
            m = lab == i + 1
            frame[m] = np.clip(tex[i] + rate[i] * t, 0, 255).astype(np.uint8)[yy[m] - y0, xx[m] - x0]
        out[t] = frame
    out.setflags(write=False)
    return out


def scene_video_f32(name):
    """f32 [T,3,H,W], the tracker's layout without the batch axis"""
    return np.ascontiguousarray(scene_video(name).transpose(0, 3, 1, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_grey(name):
    g = B.grey_ref(scene_video_f32(name))
    g.setflags(write=False)
    return g


# ------------------------------------------------------------------------------------------------------------------ the truth
# block_tracker_ref's helpers on the scenes of this module
def call_mask(name, q, obj):
    return B.call_mask(name, q, obj, SCENES)


def call_points(name, q, obj):
    return B.call_points(name, q, obj, SCENES)


def truth(name, q, points, obj):
    return B.truth(name, q, points, obj, SCENES)


def clean(name, q, points, obj, backward, R=R, S_=SEARCH):
    return B.clean(name, q, points, obj, backward, R, S_, SCENES)


def replaced(name, q, points, obj, backward, R=R):
    return B.replaced(name, q, points, obj, backward, R, SCENES)


# ------------------------------------------------------------------------------------- references, computed once and shared
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference_call(name, q, obj):
    """(points int [N,2], tracks f32 [T,N,2], vis u8 [T,N]) of live_track_ref for one call on FAST (search 40) or DRIFT
    (search 16), refresh 4, backward when q > 0 (read-only)"""
    pts = call_points(name, q, obj)
    tracks, vis = live_track_ref(scene_grey(name), pts, q, q > 0, R, FAST_SEARCH if name == "fast" else DRIFT_SEARCH, TAU, REFRESH)
    return _frozen(pts, tracks, vis)


@functools.lru_cache(maxsize=None)
def reference_default_call(name, q, obj):
    """the same with the defaults for one call of block_tracker_ref.CALLS on its textured scenes (read-only)"""
    pts = B.call_points(name, q, obj)
    tracks, vis = live_track_ref(B.textured_grey(name), pts, q, q > 0)
    return _frozen(pts, tracks, vis)
