"""CPU checks of the COCO image-clip path: the float64 restatement of the polygon fill rule (the reference the GPU test uses),
its float32 mirror, the band that is excluded from comparisons, the staging tables, and the host side of the loader (records,
plans, resume, format detection).

Fill rule: pixel (x, y) of a plane is set iff its centre (x + 0.5, y + 0.5) is inside at least one of the plane's polygons by the
even-odd rule; edge (x0, y0)-(x1, y1) counts for (cx, cy) when (y0 <= cy) != (y1 <= cy) and
cx < x0 + (cy - y0) * (x1 - x0) / (y1 - y0); a polygon closes last vertex -> first; fewer than 3 vertices set nothing.

Band rule: a pixel whose centre is within BAND px of any edge of the plane (float64 point-to-segment distance) is left out of a
comparison between two evaluations of the rule; the share left out may not exceed MAX_EXCLUDED (the cap of the eval and data
parity tests).  float32 places a crossing of a coordinate below 2^10 within ~1e-4 px (a few ulp of 6e-5), so BAND = 1e-3 covers a
float32 evaluation; test_float32_mirror_agrees_outside_the_band shows it without a GPU."""
import json
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
BAND = 1e-3
MAX_EXCLUDED = 1e-3
CASES = [(97, 131, 0), (97, 131, 1), (33, 257, 2), (480, 854, 3)]


# ------------------------------------------------------------------------------------------------------------ reference
def star_planes(H, W, seed, planes=6):
    """the shared generator: per plane 1-3 star polygons of 3-12 float32 vertices, centres up to 10 px outside the frame"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(planes):
        polys = []
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(3, 13))
            cx, cy = rng.uniform(-10, W + 10), rng.uniform(-10, H + 10)
            ang = np.sort(rng.uniform(0, 2 * np.pi, n))
            r = rng.uniform(4, 0.6 * max(H, W), n)
            polys.append(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).astype(np.float32))
        out.append(polys)
    return out


def _verts(poly, dtype):
    return np.asarray(poly, np.float32).reshape(-1, 2).astype(dtype)


def fill_reference(polys, H, W, dtype=np.float64):
    """the fill rule on one plane, every operation in `dtype` -> bool [H, W]"""
    cx = (np.arange(W) + 0.5).astype(dtype)
    cy = (np.arange(H) + 0.5).astype(dtype)
    out = np.zeros((H, W), bool)
    for poly in polys:
        v = _verts(poly, dtype)
        n = len(v)
        if n < 3:
            continue
        par = np.zeros((H, W), bool)
        for i in range(n):
            (x0, y0), (x1, y1) = v[i], v[(i + 1) % n]
            rows = (y0 <= cy) != (y1 <= cy)
            if rows.any():
                xi = x0 + (cy[rows] - y0) * (x1 - x0) / (y1 - y0)
                assert xi.dtype == dtype
                par[rows] ^= cx[None, :] < xi[:, None]
        out |= par
    return out


def edge_band(polys, H, W, band=BAND):
    """bool [H, W]: pixel centres within `band` of an edge of the plane's polygons (float64 point-to-segment distance)"""
    out = np.zeros((H, W), bool)
    for poly in polys:
        v = _verts(poly, np.float64)
        n = len(v)
        if n < 3:
            continue
        for i in range(n):
            a, b = v[i], v[(i + 1) % n]
            lo, hi = np.minimum(a, b) - band - 0.5, np.maximum(a, b) + band - 0.5    # pixel indices whose centres can be that near
            xs = np.arange(max(int(np.floor(lo[0])), 0), min(int(np.ceil(hi[0])) + 1, W))
            ys = np.arange(max(int(np.floor(lo[1])), 0), min(int(np.ceil(hi[1])) + 1, H))
            if not len(xs) or not len(ys):
                continue
            px, py = np.meshgrid(xs + 0.5, ys + 0.5)
            d = b - a
            dd = float(d @ d)
            t = np.clip(((px - a[0]) * d[0] + (py - a[1]) * d[1]) / dd, 0.0, 1.0) if dd > 0 else np.zeros_like(px)
            dist = np.hypot(px - (a[0] + t * d[0]), py - (a[1] + t * d[1]))
            out[np.ix_(ys, xs)] |= dist <= band
    return out


_CACHE = {}


def reference_planes(H, W, seed):
    """(planes, float64 fills bool [6, H, W], bands bool [6, H, W]) of a generator case, computed once and left unchanged"""
    key = (H, W, seed)
    if key not in _CACHE:
        planes = star_planes(H, W, seed)
        fill = np.stack([fill_reference(p, H, W) for p in planes])
        band = np.stack([edge_band(p, H, W) for p in planes])
        fill.setflags(write=False); band.setflags(write=False)
        _CACHE[key] = (planes, fill, band)
    return _CACHE[key]


def unpack_bits(words, H, W):
    """int32 / uint32 [P, ceil(H*W/32)] bit planes -> (bool [P, H, W], the tail bits of every plane as a flat bool array)"""
    w = np.ascontiguousarray(words).view(np.uint32)
    flat = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(len(w), -1)
    return flat[:, :H * W].reshape(len(w), H, W), flat[:, H * W:]


@pytest.mark.parametrize("H,W,seed", CASES)
def test_band_share_and_fill_of_the_generator(H, W, seed):
    planes, fill, band = reference_planes(H, W, seed)
    share = band.mean()
    fills = fill.reshape(len(planes), -1).mean(1)
    print(f"({H}, {W}, seed {seed}): excluded share {share:.3g}, plane fills {np.round(fills, 3).tolist()}")
    assert share <= MAX_EXCLUDED
    assert (fills > 0.02).sum() >= 3 and fills.max() > 0.2 and fills.max() < 1.0          # a non-trivial comparison
    assert all(p.dtype == np.float32 for pl in planes for p in pl)
    far = [p for pl in planes for p in pl if (p < 0).any() or (p[:, 0] > W).any() or (p[:, 1] > H).any()]
    assert far                                                                            # vertices outside the frame occur


@pytest.mark.parametrize("H,W,seed", CASES)
def test_float32_mirror_agrees_outside_the_band(H, W, seed):
    planes, fill, band = reference_planes(H, W, seed)
    f32 = np.stack([fill_reference(p, H, W, np.float32) for p in planes])
    assert np.array_equal(f32[~band], fill[~band])


def test_reference_on_shapes_with_a_known_answer():
    H, W = 9, 13
    sq = [[2, 3, 7, 3, 7, 6, 2, 6]]                                    # integer corners: centres 2.5 .. 6.5 x 3.5 .. 5.5
    want = np.zeros((H, W), bool)
    want[3:6, 2:7] = True
    assert np.array_equal(fill_reference(sq, H, W), want)
    assert np.array_equal(fill_reference(sq, H, W, np.float32), want)
    assert not fill_reference([[1, 1, 8, 8]], H, W).any()               # 2 vertices
    assert fill_reference([[-5, -5, 50, -5, 50, 50, -5, 50]], H, W).all()
    hole = fill_reference([[1, 1, 11, 1, 11, 8, 1, 8, 1, 1, 4, 3, 8, 3, 8, 6, 4, 6, 4, 3]], H, W)      # even-odd: a hole
    assert hole[2, 2] and not hole[4, 5]
    two = fill_reference([[1, 1, 11, 1, 11, 8, 1, 8], [4, 3, 8, 3, 8, 6, 4, 6]], H, W)                 # two polygons: the union
    assert two[2, 2] and two[4, 5]
    assert edge_band(sq, H, W, 0.5 + 1e-9)[3, 2] and not edge_band(sq, H, W, 0.49)[3, 2]


def test_stage_polygons_tables():
    from s2d_amd.data.image_clip import stage_polygons
    planes = star_planes(33, 257, 2)
    planes.insert(2, [])                                               # a plane without polygons
    verts, poly_off, plane_off = stage_polygons(planes)
    assert verts.dtype == np.float32 and poly_off.dtype == plane_off.dtype == np.int32
    assert plane_off.tolist()[:4] == [0, len(planes[0]), len(planes[0]) + len(planes[1]), len(planes[0]) + len(planes[1])]
    assert plane_off[-1] == len(poly_off) - 1 and poly_off[-1] == len(verts)
    q = 0
    for pl in planes:
        for p in pl:
            assert np.array_equal(verts[poly_off[q]:poly_off[q + 1]], p)
            q += 1
    flat = stage_polygons([[[1, 2, 3, 4, 5, 6]]])                      # COCO's flat coordinate lists
    assert flat[0].tolist() == [[1, 2], [3, 4], [5, 6]]
    empty = stage_polygons([])
    assert empty[0].shape == (0, 2) and empty[1].tolist() == [0] and empty[2].tolist() == [0]


# ------------------------------------------------------------------------------------------------------------ dataset
def _rle(H, W, counts):
    return {"size": [H, W], "counts": counts}


def _coco_doc():
    H, W = 40, 60
    tri = [5.0, 5.0, 30.0, 8.0, 12.0, 30.0]
    images = [{"id": 7, "height": H, "width": W, "file_name": "b.jpg"}, {"id": 3, "height": W, "width": H, "file_name": "a.jpg"},
              {"id": 9, "height": H, "width": W, "file_name": "c.jpg"}, {"id": 11, "height": H, "width": W, "file_name": "d.jpg"}]
    anns = [
        {"id": 1, "image_id": 7, "category_id": 18, "iscrowd": 0, "segmentation": [tri, [1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7]]},
        {"id": 2, "image_id": 7, "category_id": 4, "iscrowd": 0, "segmentation": _rle(H, W, [10, 20, H * W - 30])},
        {"id": 3, "image_id": 7, "category_id": 4, "iscrowd": 1, "segmentation": _rle(H, W, [0, 50, H * W - 50])},
        {"id": 4, "image_id": 7, "category_id": 18, "segmentation": _rle(H, W, "0e0")},      # compressed string, no iscrowd key
        {"id": 5, "image_id": 7, "category_id": 4, "iscrowd": 0, "segmentation": [[1, 2, 3, 4]]},          # no valid polygon
        {"id": 6, "image_id": 7, "category_id": 4, "iscrowd": 0, "segmentation": None},
        {"id": 7, "image_id": 3, "category_id": 9, "iscrowd": 0, "segmentation": [tri, tri[::-1]]},
        {"id": 8, "image_id": 9, "category_id": 9, "iscrowd": 1, "segmentation": [tri]},                   # crowd only
    ]                                                                                                        # image 11: nothing
    return {"images": images, "annotations": anns, "categories": [{"id": 18}, {"id": 4}, {"id": 9}]}


def test_load_coco_image_train_records():
    from s2d_amd.data.image_clip import load_coco_image_train
    doc = _coco_doc()
    recs = load_coco_image_train(doc, "/root_dir")
    assert [r["image_id"] for r in recs] == [3, 7]                     # sorted by id; crowd-only and empty images filtered
    assert recs[0]["file_name"] == os.path.join("/root_dir", "a.jpg") and (recs[0]["height"], recs[0]["width"]) == (60, 40)
    assert set(recs[1]) == {"file_name", "height", "width", "image_id", "annotations"}
    a = recs[1]["annotations"]
    assert [o["id"] for o in a] == [1, 2, 3, 4]                        # 5 (no valid polygon) and 6 (null) skipped
    assert all(set(o) == {"id", "category_id", "iscrowd", "segmentation"} for o in a)
    assert [o["category_id"] for o in a] == [2, 0, 0, 2] and recs[0]["annotations"][0]["category_id"] == 1    # 4, 9, 18 -> 0, 1, 2
    assert [o["iscrowd"] for o in a] == [0, 0, 1, 0]
    assert a[0]["segmentation"] == [[5.0, 5.0, 30.0, 8.0, 12.0, 30.0]]                     # the 4- and 7-coordinate polygons dropped
    assert a[1]["segmentation"]["counts"] == [10, 20, 2370] and a[3]["segmentation"]["counts"] == "0e0"
    assert len(recs[0]["annotations"][0]["segmentation"]) == 2
    every = load_coco_image_train(doc, "/root_dir", filter_empty=False)
    assert [r["image_id"] for r in every] == [3, 7, 9, 11] and every[3]["annotations"] == []
    assert [o["iscrowd"] for o in every[2]["annotations"]] == [1]


def test_load_coco_image_train_refuses_an_rle_of_another_size(tmp_path):
    from s2d_amd.data.image_clip import load_coco_image_train
    doc = _coco_doc()
    doc["annotations"][1]["segmentation"] = _rle(60, 40, [10, 20, 2370])
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(doc))
    with pytest.raises(ValueError, match="image 7"):
        load_coco_image_train(str(path), "/root_dir")


def test_train_format_detection():
    from s2d_amd.data.image_clip import detect_train_format
    from s2d_amd.train import parse_args
    assert detect_train_format(_coco_doc()) == "coco_image"
    assert detect_train_format({"videos": [], "annotations": []}) == "ytvis"
    assert detect_train_format({"videos": [], "images": [], "annotations": []}) == "ytvis"
    assert detect_train_format({"annotations": []}) == "ytvis"
    base = ["--config-file", "c", "--train-json", "j", "--image-root", "r", "--output-dir", "o"]
    assert parse_args(base).train_format == "auto"
    assert parse_args(base + ["--train-format", "coco_image"]).train_format == "coco_image"
    with pytest.raises(SystemExit):
        parse_args(base + ["--train-format", "lvis"])


# ------------------------------------------------------------------------------------------------------------ plans
def _settings(T=3):
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import ClipSettings
    return ClipSettings(load_config(KD_CFG, ["INPUT.MIN_SIZE_TRAIN", "(32, 48)", "INPUT.SAMPLING_FRAME_NUM", str(T)]))


def _plan_key(plans):
    return [(p["record"]["image_id"], p["params"].tobytes(), p["out_hw"], p["plane_of"].tobytes(), p["gt_ids"].tobytes(),
             p["gt_classes"].tobytes(), p["poly_slots"]) for p in plans]


def test_plan_image_clip_slots_and_purity():
    from s2d_amd.data.image_clip import load_coco_image_train, plan_image_clip
    from s2d_amd.data.train_loader import clip_generators
    st = _settings(T=3)
    rec = load_coco_image_train(_coco_doc(), "/root_dir")[1]
    plan = plan_image_clip(rec, *clip_generators(5, 17), st)
    T, S = 3, 3                                                        # annotations 1, 2, 4: the crowd one has no slot
    assert plan["plane_of"].shape == plan["gt_ids"].shape == plan["gt_classes"].shape == (T, S)
    assert plan["plane_of"].dtype == np.int32 and plan["gt_ids"].dtype == np.int64 and plan["gt_classes"].dtype == np.int64
    assert all(plan["plane_of"][t, s] == s and plan["gt_ids"][t, s] == s for t in range(T) for s in range(S))
    assert plan["gt_classes"][0].tolist() == [2, 0, 2]
    assert plan["poly_slots"] == [0] and plan["polys"] == [rec["annotations"][0]["segmentation"]]
    assert [r is None for r in plan["rle"]] == [True, False, False]
    assert plan["params"].shape == (T, 16)
    # size and flip once per clip, the rest per frame: one output size, the brightness draws differ
    want, hw = st.aug.sample(T, rec["height"], rec["width"], rng=clip_generators(5, 17)[1])
    assert np.array_equal(plan["params"], want) and plan["out_hw"] == hw
    # a pure function of (seed, position), and the global generators are not touched
    random.seed(3); np.random.seed(3)
    a = (random.random(), np.random.rand())
    random.seed(3); np.random.seed(3)
    again = plan_image_clip(rec, *clip_generators(5, 17), st)
    assert (random.random(), np.random.rand()) == a
    assert _plan_key([again]) == _plan_key([plan])
    assert _plan_key([plan_image_clip(rec, *clip_generators(5, 18), st)]) != _plan_key([plan])


def test_resumed_image_loader_reproduces_the_plans():
    from s2d_amd.data.image_clip import COCOImageTrainLoader
    from s2d_amd.data.train_loader import YTVISTrainLoader
    assert issubclass(COCOImageTrainLoader, YTVISTrainLoader)
    st = _settings(T=2)
    tri = [[5.0, 5.0, 30.0, 8.0, 12.0, 30.0]]
    recs = [{"file_name": f"{i}.jpg", "height": 40 + 30 * (i % 2), "width": 55, "image_id": i,
             "annotations": [{"id": 10 * i + j, "category_id": 0, "iscrowd": 0, "segmentation": tri} for j in range(1 + i % 3)]}
            for i in range(7)]
    for rank in (0, 1):
        full = COCOImageTrainLoader(recs, st, 2, seed=11, rank=rank, world=2, device="cpu").plans()
        first = [_plan_key(next(full)) for _ in range(9)]
        k = 5
        resumed = COCOImageTrainLoader(recs, st, 2, seed=11, rank=rank, world=2, start_iter=k, device="cpu").plans()
        assert [_plan_key(next(resumed)) for _ in range(4)] == first[k:k + 4]
        assert all(len(b) == 2 for b in first)
    with pytest.raises(ValueError):
        COCOImageTrainLoader([], st, 2, seed=0, device="cpu")
