"""A deterministic point tracker for keymask discovery tests, built from a synthetic scene description.

Each scene is a few rectangles that move by an integer offset per frame, drawn back to front; an object may be absent for some
frames.  `write_dataset(root)` writes the frames (RGB PNG) and the colour pseudo masks (one colour per object, black
background) under `root/DAVIS/...`.  `StubTracker` takes the call of the tracker boundary (s2d_amd/keymask/tracker.py): it
recognises the scene from the video's first frame, lays its own grid of grid_size x grid_size pixel centres over the frame,
keeps the points inside segm_mask, and moves each point by the offset of the object under it in the query frame.  A point is
visible where its object is the front-most one at its position.  Without backward_tracking a point stays at its query
position, invisible, in the frames before the query frame.  Every coordinate is an integer held in a float32, so host and
device code round it identically.  Every call is recorded."""
import os

import numpy as np
import torch
from PIL import Image

# object: mask colour, frame shade, (y, x, h, w) in frame 0, (dy, dx) per frame, frames where it is absent.  Later objects are
# drawn over earlier ones.
SCENES = {
    "vid_a": dict(T=10, H=120, W=216, objects=[
        dict(color=(200, 40, 40), shade=(180, 90, 60), box=(8, 6, 40, 52), step=(0, 5), absent=()),
        dict(color=(40, 200, 40), shade=(60, 170, 90), box=(70, 150, 30, 36), step=(0, 0), absent=()),
        dict(color=(40, 40, 200), shade=(70, 80, 190), box=(62, 60, 48, 50), step=(0, 12), absent=()),
        dict(color=(210, 210, 40), shade=(200, 200, 120), box=(10, 160, 34, 40), step=(1, -2), absent=(6, 7, 8)),
    ]),
    "vid_b": dict(T=9, H=120, W=216, objects=[
        dict(color=(90, 90, 90), shade=(140, 140, 140), box=(30, 140, 40, 40), step=(0, 0), absent=()),
        dict(color=(0, 128, 255), shade=(30, 120, 220), box=(20, 20, 44, 60), step=(1, 3), absent=()),
        dict(color=(255, 0, 128), shade=(220, 40, 120), box=(60, 120, 40, 50), step=(-1, 6), absent=()),
        dict(color=(128, 255, 0), shade=(120, 220, 40), box=(78, 10, 30, 40), step=(0, 2), absent=(3, 4)),
        dict(color=(250, 250, 250), shade=(240, 230, 200), box=(26, 118, 48, 30), step=(0, 3), absent=()),   # slides over object 0
    ]),
}
FRAMES_DIR = os.path.join("DAVIS", "JPEGImages", "480p")
MASKS_DIR = os.path.join("DAVIS", "pseudo_masks")


def label_map(scene, t):
    """int [H,W]: index + 1 of the front-most object at each pixel of frame t, 0 = background"""
    H, W = scene["H"], scene["W"]
    lab = np.zeros((H, W), np.int64)
    for i, o in enumerate(scene["objects"]):
        if t in o["absent"]:
            continue
        y, x, h, w = o["box"]
        y, x = y + o["step"][0] * t, x + o["step"][1] * t
        lab[max(y, 0):max(min(y + h, H), 0), max(x, 0):max(min(x + w, W), 0)] = i + 1
    return lab


def render(scene, t):
    """(frame RGB u8 [H,W,3], colour mask RGB u8 [H,W,3]) of frame t"""
    H, W = scene["H"], scene["W"]
    lab = label_map(scene, t)
    yy, xx = np.mgrid[0:H, 0:W]
    frame = np.stack([(xx * 255) // W, (yy * 255) // H, np.full((H, W), 96)], -1).astype(np.uint8)
    shades = np.array([(0, 0, 0)] + [o["shade"] for o in scene["objects"]], np.uint8)
    colors = np.array([(0, 0, 0)] + [o["color"] for o in scene["objects"]], np.uint8)
    frame = np.where(lab[..., None] > 0, shades[lab], frame)
    return frame, colors[lab]


def write_dataset(root, scenes=SCENES):
    """frames under root/FRAMES_DIR/<video>/%05d.png, masks under root/MASKS_DIR/<video>/%05d.png"""
    for name, sc in scenes.items():
        fd, md = os.path.join(root, FRAMES_DIR, name), os.path.join(root, MASKS_DIR, name)
        os.makedirs(fd, exist_ok=True)
        os.makedirs(md, exist_ok=True)
        for t in range(sc["T"]):
            frame, mask = render(sc, t)
            Image.fromarray(frame).save(os.path.join(fd, f"{t:05d}.png"))
            Image.fromarray(mask).save(os.path.join(md, f"{t:05d}.png"))


class StubTracker:
    def __init__(self, scenes=SCENES):
        self.scenes = scenes
        self.first = {name: render(sc, 0)[0] for name, sc in scenes.items()}
        self.labels = {name: [label_map(sc, t) for t in range(sc["T"])] for name, sc in scenes.items()}
        self.calls = []

    def cuda(self):
        return self

    def _scene(self, video):
        f0 = video[0, 0].detach().cpu().numpy().transpose(1, 2, 0)
        for name, img in self.first.items():
            if img.shape == f0.shape and np.array_equal(img.astype(np.float32), f0):
                return name
        raise ValueError("video of no known scene")

    def __call__(self, video, grid_size=50, grid_query_frame=0, segm_mask=None, backward_tracking=False):
        name = self._scene(video)
        sc, labs = self.scenes[name], self.labels[name]
        T, H, W, q = sc["T"], sc["H"], sc["W"], int(grid_query_frame)
        assert video.shape[1] == T and video.shape[-2:] == (H, W)
        ys = (np.arange(grid_size) * 2 + 1) * H // (2 * grid_size)
        xs = (np.arange(grid_size) * 2 + 1) * W // (2 * grid_size)
        gy, gx = (a.reshape(-1) for a in np.meshgrid(ys, xs, indexing="ij"))
        m = segm_mask.detach().cpu().numpy().reshape(H, W)
        keep = m[gy, gx] > 0
        py, px = gy[keep], gx[keep]
        obj = labs[q][py, px]                                   # 1-based object under each point in the query frame
        steps = np.array([(0, 0)] + [o["step"] for o in sc["objects"]], np.int64)[obj]
        tracks = np.zeros((T, len(py), 2), np.float32)
        vis = np.zeros((T, len(py)), bool)
        for t in range(T):
            if t < q and not backward_tracking:
                tracks[t, :, 0], tracks[t, :, 1] = px, py
                continue
            y, x = py + steps[:, 0] * (t - q), px + steps[:, 1] * (t - q)
            tracks[t, :, 0], tracks[t, :, 1] = x, y
            inb = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            vis[t, inb] = labs[t][y[inb], x[inb]] == obj[inb]
        self.calls.append({"video": name, "grid_size": int(grid_size), "grid_query_frame": q,
                           "backward_tracking": bool(backward_tracking), "points": int(len(py)), "mask_pixels": int((m > 0).sum())})
        dev = video.device
        return torch.from_numpy(tracks)[None].to(dev), torch.from_numpy(vis)[None].to(dev)


def make_tracker(checkpoint=None):
    """factory for `--tracker tests.golden.keymask_stub_tracker:make_tracker`"""
    return StubTracker()
