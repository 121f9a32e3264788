"""The stage-1 paint rule in numpy (`ops.paint_frames`, csrc/infer.hip infer_frame_areas_kernel / infer_paint_kernel) and the shared
inputs of tests/test_frame_masks_refs_cpu.py and tests/test_gpu_frame_paint.py.  Numpy only; nothing here calls a kernel.

The rule.  K planes m_k,t = "proposal k holds the pixel", k = 0 the best-scored.  area[k][t] = set pixels; order[t] = the
proposals by descending area, equal areas in proposal order (a stable sort).  The frame starts black, the proposals are painted in
order[t], a later one over an earlier one.  `paint_literal` says exactly that -- the reference's overlay_masks_numpy
(cutler/demo/predictor.py:237-355) as a loop over argsort with np.where; `paint_owner` says the same as "a pixel belongs to the
holder with the largest position in order[t]" (the smallest area, among equal areas the higher k), the form the kernel evaluates.
rgb = colors[k] of the owner (by k, not by position) or black; index = k + 1 or 0."""
import numpy as np

from tests import davis_index_refs as R


def stable_order(areas):
    """areas [K, T] -> order [T, K]: per frame the proposals by descending area, equal areas in proposal order"""
    return np.argsort(-np.asarray(areas, np.int64).T, axis=1, kind="stable").astype(np.int32)


def plane_areas(masks):
    return (np.asarray(masks) != 0).sum(axis=(2, 3)).astype(np.int32)


def paint_literal(masks, colors):
    """masks [K, T, H, W] (0 / non-0), colors u8 [K, 3] -> (rgb u8 [T, H, W, 3], index u8 [T, H, W]): paint in argsort order"""
    m = np.asarray(masks) != 0
    K, T, H, W = m.shape
    rgb = np.zeros((T, H, W, 3), np.uint8)
    index = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        areas = m[:, t].sum(axis=(1, 2))
        for k in np.argsort(-areas, kind="stable"):
            rgb[t] = np.where(m[k, t][..., None], np.asarray(colors[k], np.uint8), rgb[t])
            index[t] = np.where(m[k, t], np.uint8(k + 1), index[t])
    return rgb, index


def paint_owner(masks, colors, order=None):
    """the same picture from the owner form: per pixel the holder with the largest position in order[t] (default: stable_order of
    the planes' areas)"""
    m = np.asarray(masks) != 0
    K, T, H, W = m.shape
    order = stable_order(plane_areas(m)) if order is None else np.asarray(order)
    table = np.concatenate([np.zeros((1, 3), np.uint8), np.asarray(colors, np.uint8)[:K]])
    rgb = np.zeros((T, H, W, 3), np.uint8)
    index = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        pos = np.empty(K, np.int64)
        pos[order[t]] = np.arange(K)                                  # position of proposal k in the frame's draw order
        top = np.where(m[:, t], pos[:, None, None] + 1, 0).max(axis=0)   # 1 + the largest position among the holders, 0: none
        owner = np.where(top > 0, order[t][np.maximum(top - 1, 0)] + 1, 0)
        index[t] = owner.astype(np.uint8)
        rgb[t] = table[owner]
    return rgb, index


def case_colors(K):
    """K distinct non-black colours that are no function of the draw position: a fixed pseudo-random table"""
    rng = np.random.default_rng(99)
    flat = rng.permutation(np.arange(1, 1 << 24))[:K]
    return np.stack([flat & 255, (flat >> 8) & 255, (flat >> 16) & 255], -1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ kernel cases
# geometry rows: name -> (T, hm, wm, padded, img, out)
GEOMETRIES = {
    "two_stage": (3, 9, 13, (36, 52), (33, 50), (37, 131)),         # ragged tiles both ways, ow no multiple of 4, 3 x 3 tiles
    "same": (2, 8, 12, (32, 48), (30, 45), (30, 45)),
}
DIRECT = (1, 40, 60, (160, 240), (160, 240), (20, 30))              # K = 254: K * window > 40 KB, the direct path
WIDTHS = {8: 6, 128: 100}                                           # ldq -> Q
KS = (1, 3, 50, 254)


def cases():
    out = [dict(name=f"{g}-ldq{ldq}-K{K}", geo=geo, ldq=ldq, Q=Q, K=K)
           for g, geo in GEOMETRIES.items() for ldq, Q in WIDTHS.items() for K in KS]
    out.append(dict(name="direct-ldq128-K254", geo=DIRECT, ldq=128, Q=100, K=254))
    return out


CASES = cases()
CASE_IDS = [c["name"] for c in CASES]


def make_inputs(case):
    """-> (ml f32 [T*hm*wm, ldq], dims, padded, img, out, query int32 [K]): Q smooth columns (davis_index_refs.smooth_logits), zero
    pad columns, query a random order of the columns, repeated past Q -- a repeat has its first copy's area, so the tie rule of
    the order is exercised wherever K > Q"""
    T, hm, wm, padded, img, out = case["geo"]
    ldq, Q, K = case["ldq"], case["Q"], case["K"]
    rng = np.random.default_rng(R.hash_name("paint-" + case["name"]))
    ml = np.zeros((T * hm * wm, ldq), np.float32)
    ml[:, :Q] = R.smooth_logits(rng, Q * T, hm, wm).reshape(Q, T * hm * wm).T
    query = np.concatenate([rng.permutation(Q) for _ in range(-(-K // Q))])[:K].astype(np.int32)
    return ml, (T, hm, wm), padded, img, out, query


# ------------------------------------------------------------------------------------------------------------------ named rows
NAMED_GEO = (3, 9, 13, (36, 52), (33, 50), (37, 131))
NAMED = ("nested", "tie", "same_column", "empty_in_one_frame", "order_differs", "all_negative_frame", "nan_neg_zero")


def _box(pl, t, col, r0, r1, c0, c1):
    """column `col` of frame t: +1 inside the low-resolution box rows r0..r1-1, columns c0..c1-1 (the rest stays at -1)"""
    pl[t, r0:r1, c0:c1, col] = 1.0


def named_inputs(name):
    """-> (ml, dims, padded, img, out, query) of a named row on constructed logits, ldq = 8: every column is -1 except where a box
    of +1 is drawn (`_box`), so a proposal's mask is that box, grown or shrunk by less than a low-resolution cell by the resize.

    nested              k = 0 a small box strictly inside the large box of k = 1, all frames: the small one shows on top, though k = 1
                        is painted by a rule that lets the higher k win, and a walk of the order from its front shows the large one
    tie                 k = 0 and k = 1 are the constants +1 and +2 -- every pixel, equal areas --, k = 2 a box: outside the box k = 1
                        (the higher k of the equal pair) owns every pixel
    same_column         query = [c, c]: one mask twice, the second copy owns it
    empty_in_one_frame  k = 1 is -1 everywhere in frame 1 of three (area 0 there) and a box elsewhere
    order_differs       k = 0 is large in frame 0 and small in frame 1, k = 1 the other way round, the boxes overlap; frame 2: as 0
    all_negative_frame  frame 2 holds nothing for any proposal: black, index 0
    nan_neg_zero        k = 0 NaN, k = 1 -0.0, k = 2 a box: only k = 2 holds anything"""
    T, hm, wm, padded, img, out = NAMED_GEO
    pl = np.full((T, hm, wm, 8), -1.0, np.float32)
    if name == "nested":
        for t in range(T):
            _box(pl, t, 5, 3, 5, 5 + t, 8 + t)
            _box(pl, t, 2, 1, 8, 2, 12)
        query = [5, 2]
    elif name == "tie":
        pl[..., 1], pl[..., 4] = 1.0, 2.0
        for t in range(T):
            _box(pl, t, 6, 2, 6, 3 + t, 9)
        query = [1, 4, 6]
    elif name == "same_column":
        for t in range(T):
            _box(pl, t, 3, 2, 7, 1 + 2 * t, 7 + 2 * t)
        query = [3, 3]
    elif name == "empty_in_one_frame":
        for t in range(T):
            _box(pl, t, 0, 1, 8, 1, 9)
            if t != 1:
                _box(pl, t, 7, 4, 8, 6, 12)
        query = [0, 7]
    elif name == "order_differs":
        for t in range(T):
            big, small = (1, 0) if t == 1 else (0, 1)
            _box(pl, t, (2, 6)[big], 1, 8, 1, 11)
            _box(pl, t, (2, 6)[small], 3, 6, 8, 13)
        query = [2, 6]
    elif name == "all_negative_frame":
        for t in range(2):
            _box(pl, t, 1, 2, 6, 2, 8)
            _box(pl, t, 3, 4, 9, 5, 12)
        query = [1, 3, 5]
    elif name == "nan_neg_zero":
        pl[..., 0] = np.nan
        pl[..., 1] = np.float32(-0.0)
        for t in range(T):
            _box(pl, t, 2, 2, 7, 3, 10)
        query = [0, 1, 2]
    else:
        raise KeyError(name)
    return pl.reshape(T * hm * wm, 8), (T, hm, wm), padded, img, out, np.asarray(query, np.int32)


def planes_float64(row):
    """the holding planes bool [K, T, oh, ow] of a row from the float64 restatement of the resize (davis_index_refs.two_stage)"""
    ml, dims, padded, img, out, query = row
    return R.two_stage(R.planes_of(ml, dims, query), padded, img, out) > 0


def check_named_property(name, m, rgb, index, colors):
    """assert what the row is named for, on holding planes m bool [K, T, H, W] and the picture painted from them"""
    areas = plane_areas(m)
    col = [tuple(int(v) for v in c) for c in colors]

    def shown(k, where):
        return bool((index[where] == k + 1).all()) and bool((rgb[where] == np.asarray(col[k], np.uint8)).all())
    if name == "nested":
        assert m[0].any(axis=(1, 2)).all() and not (m[0] & ~m[1]).any() and (areas[0] < areas[1]).all()
        assert shown(0, m[0]) and shown(1, m[1] & ~m[0])
    elif name == "tie":
        assert m[0].all() and m[1].all() and (areas[0] == areas[1]).all() and m[2].any() and not m[2].all()
        assert shown(2, m[2]) and shown(1, ~m[2])
    elif name == "same_column":
        assert (m[0] == m[1]).all() and m[0].any()
        assert shown(1, m[1]) and bool((index[~m[1]] == 0).all())
    elif name == "empty_in_one_frame":
        assert areas[1].tolist()[1] == 0 and areas[1][0] > 0 and areas[1][2] > 0 and (areas[0] > 0).all()
        f1 = (np.arange(3) == 1)[:, None, None]
        assert shown(0, m[0] & f1) and shown(1, m[1])                    # the smaller box is on top where it exists
    elif name == "order_differs":
        assert areas[0][0] > areas[1][0] and areas[0][1] < areas[1][1] and (m[0] & m[1]).any(axis=(1, 2)).all()
        both = m[0] & m[1]
        f = (np.arange(3) == 1)[:, None, None]
        assert shown(1, both & ~f) and shown(0, both & f)
    elif name == "all_negative_frame":
        assert not m[:, 2].any() and m[:2, :2].any()
        assert not rgb[2].any() and not index[2].any() and index[:2].any()
    elif name == "nan_neg_zero":
        assert not m[0].any() and not m[1].any() and m[2].any()
        assert shown(2, m[2]) and bool((index[~m[2]] == 0).all()) and not rgb[~m[2]].any()
    else:
        raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------ hand-off scene
# Three boxes per video that drift one pixel per frame and never touch, in the layout of tests/golden/keymask_stub_tracker.SCENES:
# box = (y, x, h, w) in frame 0, step = (dy, dx) per frame.  The logits are constructed at frame size (hm x wm = H x W, no padding,
# output size = frame size: the resize is the identity), so proposal i's mask is exactly box i of the frame.
HANDOFF_SCENES = {
    "drift_a": dict(T=8, H=120, W=216, objects=[dict(box=(8, 10, 44, 56), step=(0, 1)), dict(box=(64, 90, 40, 50), step=(1, 0)),
                                                  dict(box=(12, 150, 36, 40), step=(0, -1))]),
    "drift_b": dict(T=8, H=120, W=216, objects=[dict(box=(60, 12, 48, 60), step=(-1, 0)), dict(box=(10, 100, 38, 44), step=(0, 1)),
                                                  dict(box=(70, 150, 34, 46), step=(0, -1))]),
}


def handoff_boxes(scene, t):
    return [(o["box"][0] + o["step"][0] * t, o["box"][1] + o["step"][1] * t, o["box"][2], o["box"][3]) for o in scene["objects"]]


def handoff_logits(scene):
    """-> (ml f32 [T*H*W, 8], dims, size, query): column i is +1 inside box i and -1 outside"""
    T, H, W = scene["T"], scene["H"], scene["W"]
    pl = np.full((T, H, W, 8), -1.0, np.float32)
    for t in range(T):
        for i, (y, x, h, w) in enumerate(handoff_boxes(scene, t)):
            pl[t, y:y + h, x:x + w, i] = 1.0
    return pl.reshape(T * H * W, 8), (T, H, W), (H, W), np.arange(len(scene["objects"]), dtype=np.int32)


def handoff_frames(scene, seed):
    """u8 [T, H, W, 3]: a fixed random texture of 2 x 2 cells as background and one per box that moves with it (the frames of
    tests/block_tracker_ref.textured_video, for these scenes)"""
    T, H, W = scene["T"], scene["H"], scene["W"]
    rng = np.random.default_rng(seed)

    def texture(h, w):
        cells = rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 3), dtype=np.uint8)
        return np.repeat(np.repeat(cells, 2, 0), 2, 1)[:h, :w]
    bg = texture(H, W)
    tex = [texture(o["box"][2], o["box"][3]) for o in scene["objects"]]
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        out[t] = bg
        for i, (y, x, h, w) in enumerate(handoff_boxes(scene, t)):
            out[t, y:y + h, x:x + w] = tex[i]
    return out
