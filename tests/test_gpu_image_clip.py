"""GPU checks of training on COCO image annotations as pseudo-clips: s2d_polygons_to_bits against the float64 restatement of
the fill rule (tests/test_polygon_refs_cpu.py: reference, generator and band rule), polygon and RLE instances of one record in
one bit-plane tensor, map_image_clip against the existing warp kernels, and `python -m s2d_amd.train` on a COCO file."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_polygon_refs_cpu import (MAX_EXCLUDED, edge_band, fill_reference, reference_planes, star_planes,
                                         unpack_bits)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
DEV = "cuda:0"


def _bits(planes, H, W, **kw):
    from s2d_amd.data.image_clip import polygons_to_bits
    out = polygons_to_bits(planes, H, W, device=DEV, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ the kernel
# (5, 31): a row is shorter than a word.  Its 6 planes hold 930 pixels, so the 1e-3 cap admits no band pixel at all there: seed 6
# is the first seed from 4 on whose float64 band is empty (4 and 5 put 3 and 1 centres inside it).
@pytest.mark.parametrize("H,W,seed", [(97, 131, 0), (33, 257, 2), (5, 31, 6)])
def test_polygons_to_bits_matches_float64_outside_the_band(H, W, seed):
    planes, fill, band = reference_planes(H, W, seed)
    words = _bits(planes, H, W)
    assert words.shape == (6, (H * W + 31) // 32) and words.dtype == np.int32
    got, tail = unpack_bits(words, H, W)
    share = band.mean()
    wrong = int((got != fill)[~band].sum())
    print(f"({H}, {W}, seed {seed}): excluded share {share:.3g}, mismatches outside the band {wrong}, inside "
          f"{int((got != fill)[band].sum())} of {int(band.sum())}")
    assert share <= MAX_EXCLUDED
    assert wrong == 0
    assert not tail.any()
    # planes built in one call equal planes built one call each
    for p, pl in enumerate(planes):
        assert np.array_equal(_bits([pl], H, W)[0], words[p])


def test_polygons_to_bits_special_planes():
    H, W = 97, 131
    rng = np.random.default_rng(7)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 300))
    r = rng.uniform(20, 45, 300)
    big = np.stack([60 + r * np.cos(ang), 50 + r * np.sin(ang)], 1).astype(np.float32)      # 300 edges: two LDS chunks
    planes = [[],                                                                            # no polygons
              [[200.0, 10.0, 260.0, 20.0, 230.0, 90.0], [-50.0, -40.0, -5.0, -40.0, -5.0, -3.0]],       # wholly outside
              [[10.0, 10.0, 80.0, 80.0]],                                                    # 2 vertices
              [[-5.0, -5.0, W + 5.0, -5.0, W + 5.0, H + 5.0, -5.0, H + 5.0]],                # covers the frame
              [big],
              [[10.0, 10.0, 80.0, 80.0], big, []]]                                           # dead polygons beside a live one
    words = _bits(planes, H, W)
    got, tail = unpack_bits(words, H, W)
    assert not tail.any()
    assert not got[0].any() and not got[1].any() and not got[2].any()
    assert got[3].all()
    want, band = fill_reference([big], H, W), edge_band([big], H, W)
    assert band.mean() <= MAX_EXCLUDED and 0.2 < want.mean() < 0.8
    assert np.array_equal(got[4][~band], want[~band])
    assert np.array_equal(words[5], words[4])
    assert _bits([], H, W).shape == (0, (H * W + 31) // 32)


def test_polygons_to_bits_rows_and_argument_errors():
    from s2d_amd._lib import lib
    from s2d_amd.data.image_clip import polygons_to_bits, stage_polygons
    H, W = 33, 257
    planes, _, _ = reference_planes(H, W, 2)
    alone = _bits(planes[:3], H, W)
    out = torch.full((5, alone.shape[1]), -1, device=DEV, dtype=torch.int32)
    polygons_to_bits(planes[:3], H, W, out=out, rows=[4, 0, 2])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(o[[4, 0, 2]], alone) and (o[[1, 3]] == -1).all()                  # the other rows are not touched
    with pytest.raises(ValueError):
        polygons_to_bits(planes[:3], H, W, out=out, rows=[1, 1, 2])
    with pytest.raises(ValueError):
        polygons_to_bits(planes[:3], H, W, out=out, rows=[1, 5, 2])
    # a non-monotone offset table is refused before anything is launched
    verts, poly_off, plane_off = stage_polygons(planes[:2])
    bad = poly_off.copy()
    bad[1] = bad[2] + 1
    assert (np.diff(bad) < 0).any()
    up = lambda a: torch.from_numpy(a).to(DEV)                                               # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    dst = torch.zeros((2, alone.shape[1]), device=DEV, dtype=torch.int32)
    args = lambda po, pl: ("s2d_polygons_to_bits", up(verts), len(verts), up(po), po, len(po) - 1, up(pl), pl, 2, None, 2, H, W,  # noqa: E731
                           dst, st)
    lib().call(*args(poly_off, plane_off))
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), alone[:2])
    with pytest.raises(RuntimeError, match="code -1"):
        lib().call(*args(bad, plane_off))
    past = plane_off.copy()
    past[-1] += 1                                                                            # a polygon range past NP
    with pytest.raises(RuntimeError, match="code -1"):
        lib().call(*args(poly_off, past))


# ------------------------------------------------------------------------------------------------------------ records
def _col_major_counts(m):
    """uncompressed COCO RLE counts of a [H, W] 0/1 mask (column-major runs, zeros first)"""
    flat = np.asarray(m, np.uint8).T.reshape(-1)
    edges = np.flatnonzero(np.diff(flat)) + 1
    counts = np.diff(np.concatenate([[0], edges, [len(flat)]])).tolist()
    return ([0] if flat[0] else []) + counts


def _image(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 3) % 256, (yy * 5) % 256, ((xx + yy) * 2) % 256], -1).astype(np.int32)
    return np.clip(img + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)


def _mixed_record(root, H=48, W=64, name="img.jpg", image_id=5, seed=0):
    """one image on disk with 6 instances in the order polygon, RLE, RLE, polygon, RLE (compressed), polygon, plus a crowd RLE;
    the last polygon is a 3 x 3 px corner"""
    from PIL import Image
    from s2d_amd.rle import encode_video_predictions
    Image.fromarray(_image(H, W, seed)).save(os.path.join(root, name), quality=92)
    rng = np.random.default_rng(seed + 100)
    masks = (rng.random((3, H, W)) < 0.3).astype(np.uint8)
    masks[0, H // 4: H // 2, W // 3:] = 1
    masks[2, : H // 3, : W // 2] = 1
    comp = encode_video_predictions(torch.from_numpy(masks[2][None, None]).to(DEV))[0][0]
    rles = [{"size": [H, W], "counts": _col_major_counts(masks[0])}, {"size": [H, W], "counts": _col_major_counts(masks[1])}, comp]
    stars = star_planes(H, W, seed + 200, planes=2)
    polys = [[p.reshape(-1).tolist() for p in stars[0]], [p.reshape(-1).tolist() for p in stars[1]],
             [[0.0, 0.0, 3.0, 0.0, 3.0, 3.0, 0.0, 3.0]]]
    segs = [polys[0], rles[0], rles[1], polys[1], rles[2], polys[2]]
    anns = [{"id": 50 + i, "category_id": i % 2, "iscrowd": 0, "segmentation": s} for i, s in enumerate(segs)]
    anns.insert(2, {"id": 99, "category_id": 0, "iscrowd": 1, "segmentation": rles[0]})
    rec = {"file_name": os.path.join(root, name), "height": H, "width": W, "image_id": image_id, "annotations": anns}
    return rec, rles, polys, masks


def _settings(opts):
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import ClipSettings
    return ClipSettings(load_config(KD_CFG, opts))


IDENTITY = ["INPUT.MIN_SIZE_TRAIN", "(48,)", "INPUT.RANDOM_FLIP", "none", "INPUT.AUGMENTATIONS", "[]", "INPUT.CROP.ENABLED", "False",
            "INPUT.SAMPLING_FRAME_NUM", "3"]


def test_mixed_record_planes(tmp_path):
    from s2d_amd.data.image_clip import image_clip_bits, plan_image_clip, polygons_to_bits
    from s2d_amd.ytvis_eval import decode_frames
    rec, rles, polys, masks = _mixed_record(str(tmp_path))
    H, W = rec["height"], rec["width"]
    plan = plan_image_clip(rec, None, np.random.RandomState(0), _settings(IDENTITY))
    assert plan["poly_slots"] == [0, 3, 5]
    bits = image_clip_bits(plan, torch.device(DEV))
    want_rle = decode_frames(rles, H, W, device=DEV)
    want_poly = polygons_to_bits(polys, H, W, device=DEV)
    torch.cuda.synchronize()
    assert bits.shape == (6, (H * W + 31) // 32)
    assert torch.equal(bits[[1, 2, 4]], want_rle) and torch.equal(bits[[0, 3, 5]], want_poly)
    got, _ = unpack_bits(bits.cpu().numpy(), H, W)
    assert np.array_equal(got[[1, 2, 4]], masks.astype(bool))
    assert got[5].sum() == 9 and got[5][:3, :3].all()


def test_map_image_clip_identity(tmp_path):
    from s2d_amd.data.image_clip import image_clip_bits, map_image_clip, plan_image_clip
    from s2d_amd.data.test_loader import read_frame
    rec, _, _, _ = _mixed_record(str(tmp_path))
    H, W = rec["height"], rec["width"]
    st = _settings(IDENTITY)
    got = map_image_clip(rec, None, np.random.RandomState(1), st, device=DEV)
    planes, _ = unpack_bits(image_clip_bits(plan_image_clip(rec, None, np.random.RandomState(1), st), torch.device(DEV)).cpu().numpy(), H, W)
    img = torch.from_numpy(np.ascontiguousarray(read_frame(rec["file_name"], st.fmt).transpose(2, 0, 1)))
    assert len(got["image"]) == len(got["instances"]) == 3 and got["length"] == 3
    assert got["file_names"] == [rec["file_name"]] * 3 and (got["height"], got["width"]) == (H, W) and got["image_id"] == 5
    assert set(got) >= {"image", "instances", "height", "width", "length", "video_id", "file_names"}
    for t in range(3):
        assert got["image"][t].dtype == torch.uint8 and torch.equal(got["image"][t].cpu(), img)
        g = got["instances"][t]
        assert g["gt_masks"].dtype == torch.bool and np.array_equal(g["gt_masks"].cpu().numpy(), planes)
        assert g["gt_ids"].tolist() == [0, 1, 2, 3, 4, 5] and g["gt_ids"].dtype == np.int64
        assert g["gt_classes"].tolist() == [0, 1, 0, 1, 0, 1] and g["gt_classes"].dtype == np.int64


def test_map_image_clip_equals_the_existing_warps(tmp_path):
    """the shipped augmentation list (crop, resize, flip_by_clip, brightness, contrast, rotation), T = 4: frames and masks are
    bit-identical to augment_clip on the replicated image and the unpacked planes"""
    from s2d_amd.data import augment_clip
    from s2d_amd.data.image_clip import image_clip_bits, map_image_clip, plan_image_clip
    from s2d_amd.data.test_loader import read_frame
    rec, _, _, _ = _mixed_record(str(tmp_path), H=90, W=120, seed=3)
    H, W = rec["height"], rec["width"]
    st = _settings(["INPUT.MIN_SIZE_TRAIN", "(48, 61)", "INPUT.CROP.SIZE", "[40, 70]", "INPUT.SAMPLING_FRAME_NUM", "4"])
    assert st.aug.augmentations == ("brightness", "contrast", "rotation") and st.aug.random_flip == "flip_by_clip" and st.aug.crop
    T, S = 4, 6
    bits = image_clip_bits(plan_image_clip(rec, None, np.random.RandomState(0), st), torch.device(DEV))
    planes, _ = unpack_bits(bits.cpu().numpy(), H, W)
    frame = torch.from_numpy(np.ascontiguousarray(read_frame(rec["file_name"], st.fmt).transpose(2, 0, 1))).to(DEV)
    frames = frame[None].expand(T, 3, H, W).contiguous()
    m = torch.from_numpy(planes.astype(np.uint8)).to(DEV)[:, None].expand(S, T, H, W).contiguous()
    dropped = flips = 0
    for k in range(8):
        got = map_image_clip(rec, None, np.random.RandomState(k), st, device=DEV)
        params, hw = st.aug.sample(T, H, W, rng=np.random.RandomState(k))
        img, mw = augment_clip(frames, m, params, hw)
        assert len(got["image"]) == T
        for t in range(T):
            assert torch.equal(got["image"][t], img[t])
            g = got["instances"][t]
            assert torch.equal(g["gt_masks"], mw[:, t].bool())
            alive = mw[:, t].reshape(S, -1).any(1).cpu().numpy()
            assert g["gt_ids"].tolist() == [s if alive[s] else -1 for s in range(S)]
            dropped += int((~alive).sum())
            assert alive[:5].any()
        flips += int(params[0, 0] < 0)
    assert dropped > 0                            # the 3 x 3 corner polygon falls outside some crops: gt_ids -1
    assert 0 < flips < 8


# ------------------------------------------------------------------------------------------------------------ the driver
def _write_coco(root):
    """4 JPEG images; per image two polygon instances, an uncompressed-RLE instance and (image 1) a crowd RLE.  Categories 5 and 9"""
    from PIL import Image
    images, anns, aid = [], [], 0
    for iid, (H, W) in enumerate([(90, 120), (120, 90), (72, 128), (100, 100)], start=1):
        name = f"im{iid}.jpg"
        Image.fromarray(_image(H, W, iid)).save(os.path.join(root, name), quality=90)
        images.append({"id": iid, "height": H, "width": W, "file_name": name})
        stars = star_planes(H, W, 40 + iid, planes=2)
        m = np.zeros((H, W), np.uint8)
        m[H // 2:, : W // 2] = 1
        segs = [[p.reshape(-1).tolist() for p in stars[0]], [p.reshape(-1).tolist() for p in stars[1]],
                {"size": [H, W], "counts": _col_major_counts(m)}]
        for j, s in enumerate(segs):
            aid += 1
            anns.append({"id": aid, "image_id": iid, "category_id": (5, 9)[j % 2], "iscrowd": 0, "segmentation": s,
                         "bbox": [0, 0, 1, 1], "area": 1})
        if iid == 1:
            aid += 1
            anns.append({"id": aid, "image_id": iid, "category_id": 9, "iscrowd": 1, "segmentation": segs[2]})
    path = os.path.join(root, "train.json")
    with open(path, "w") as fh:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": 5, "name": "a"}, {"id": 9, "name": "b"}]}, fh)
    return path


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from s2d_amd.checkpoint import kd_to_plain
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(KD_CFG)
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg)
    path = str(tmp_path_factory.mktemp("init") / "init.pth")
    torch.save({"model": kd_to_plain({k: v.detach().cpu() for k, v in model.state_dict().items()})}, path)
    return path


TRAIN_OPTS = ["INPUT.MIN_SIZE_TRAIN", "(64,)", "INPUT.MIN_SIZE_TEST", "64", "SOLVER.IMS_PER_BATCH", "2", "SOLVER.BASE_LR", "1e-4",
              "SOLVER.CHECKPOINT_PERIOD", "1", "SEED", "1", "SOLVER.MAX_ITER", "2"]


def _train(path, root, checkpoint, out, extra=()):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "s2d_amd.train", "--config-file", KD_CFG, "--train-json", path, "--image-root", root,
           "--output-dir", str(out), "--weights", checkpoint, "--threads", "4"] + list(extra) + TRAIN_OPTS
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-5000:])
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def test_driver_trains_on_a_coco_image_file_and_resumes(checkpoint, tmp_path):
    from s2d_amd.config import load_config
    from s2d_amd.data.image_clip import COCOImageTrainLoader, load_coco_image_train
    root = str(tmp_path)
    path = _write_coco(root)
    out = tmp_path / "out"
    lines = _train(path, root, checkpoint, out)                       # --train-format auto: `images` and no `videos`
    assert lines[0]["start_iter"] == 0 and lines[0]["seed"] == 1
    summary = [l for l in lines if "iterations" in l][-1]
    assert summary["iterations"] == 2 and summary["clips"] == 4
    recs = [json.loads(l) for l in open(out / "metrics.json")]
    assert [r["iteration"] for r in recs] == [1]
    assert "total_loss" in recs[0] and any(k.startswith("loss_mask") for k in recs[0]) and any(k.startswith("loss_dice") for k in recs[0])
    assert all(np.isfinite(v) for v in recs[0].values() if isinstance(v, float))
    for name in ("model_0000000.pth", "model_final.pth"):
        assert (out / name).exists(), name
    # resume after iteration 0: iteration 1 again, from the same sample stream
    res = tmp_path / "resumed"
    shutil.copytree(out, res)
    (res / "last_checkpoint").write_text("model_0000000.pth")
    os.remove(res / "metrics.json")
    lines = _train(path, root, checkpoint, res, extra=["--resume", "--train-format", "coco_image", "SEED", "-1"])
    assert lines[0]["start_iter"] == 1 and lines[0]["optimizer_step"] == 1 and lines[0]["seed"] == 1
    assert [l for l in lines if "iterations" in l][-1]["iterations"] == 1
    again = [json.loads(l) for l in open(res / "metrics.json")]
    assert [r["iteration"] for r in again] == [1] and np.isfinite(again[0]["total_loss"])
    # the plan the resumed loader draws for iteration 1 is the uninterrupted run's
    cfg = load_config(KD_CFG, TRAIN_OPTS)
    records = load_coco_image_train(path, root)
    key = lambda plans: [(p["record"]["image_id"], p["params"].tobytes(), p["out_hw"]) for p in plans]     # noqa: E731
    full = COCOImageTrainLoader.from_config(cfg, records, seed=lines[0]["seed"], device=DEV).plans()
    next(full)
    resumed = COCOImageTrainLoader.from_config(cfg, records, seed=lines[0]["seed"], start_iter=1, device=DEV).plans()
    assert key(next(resumed)) == key(next(full))
