"""GPU checks of the eval-only and pseudo-label drivers: the PIL-exact resize kernel, the rleToBbox kernel, the test loader
against a host-only PIL path, weights loaded after a forward, `python -m s2d_amd.evaluate` (1 and 2 ranks) and the
results -> annotations round trip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_discovery_refs_cpu import rle_to_bbox as _rle_to_bbox
from tests.test_eval_drivers_cpu import RESIZE_GRID, _rle_counts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
DEV = "cuda:0"
MIN_TEST = "64"


# ------------------------------------------------------------------------------------------------------------ resize kernel
@pytest.mark.parametrize("src,dst", RESIZE_GRID)
def test_resize_kernel_matches_pil(src, dst):
    from PIL import Image
    from s2d_amd.data.resize import resize_frames
    T = 36 if src[0] * src[1] <= 128 * 128 else 3
    rng = np.random.default_rng(src[1] + 3 * dst[0])
    fr = rng.integers(0, 256, (T,) + src + (3,), dtype=np.uint8)
    fr[:, : src[0] // 4] = 255
    got = resize_frames(torch.from_numpy(fr).to(DEV), dst).cpu().numpy()
    want = np.stack([np.asarray(Image.fromarray(f).resize((dst[1], dst[0]), Image.BILINEAR)).transpose(2, 0, 1) for f in fr])
    assert got.shape == (T, 3) + dst
    assert np.array_equal(got, want)


def test_resize_kernel_unaligned_source_and_many_workgroups():
    """a source view that starts at an odd byte (byte-load edges of the staging) and a 36-frame 720p video (8 280 workgroups)"""
    from PIL import Image
    from s2d_amd.data.resize import resize_frames
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (36, 720, 1280, 3), dtype=np.uint8)
    got = resize_frames(torch.from_numpy(fr).to(DEV), (360, 640)).cpu().numpy()
    for t in (0, 17, 35):
        want = np.asarray(Image.fromarray(fr[t]).resize((640, 360), Image.BILINEAR)).transpose(2, 0, 1)
        assert np.array_equal(got[t], want), t
    small = rng.integers(0, 256, (2 * 37 * 53 * 3 + 5,), dtype=np.uint8)
    dev = torch.from_numpy(small).to(DEV)[5:].view(2, 37, 53, 3)
    got = resize_frames(dev, (20, 31)).cpu().numpy()
    host = small[5:].reshape(2, 37, 53, 3)
    want = np.stack([np.asarray(Image.fromarray(f).resize((31, 20), Image.BILINEAR)).transpose(2, 0, 1) for f in host])
    assert np.array_equal(got, want)


# -------------------------------------------------------------------------------------------------------------- bbox kernel
def test_plane_bbox_kernel_matches_rle_to_bbox():
    from s2d_amd import ops
    from s2d_amd.ytvis_eval import plane_areas, plane_bboxes
    for H, W in ((7, 9), (33, 45), (64, 64), (5, 3)):                     # odd H*W: a partial last word
        planes = []
        planes.append(np.zeros((H, W), np.uint8))                          # empty
        planes.append(np.ones((H, W), np.uint8))                           # full
        p = np.zeros((H, W), np.uint8); p[H // 2, W - 1] = 1; planes.append(p)          # one pixel
        p = np.zeros((H, W), np.uint8); p[H - 1, 1] = 1; p[0, 2] = 1; planes.append(p)  # a run crossing a column boundary
        p = np.zeros((H, W), np.uint8); p[H - 2:, 0] = 1; p[:2, 1] = 1; p[1, W - 1] = 1; planes.append(p)
        rng = np.random.default_rng(H * W)
        for _ in range(4):
            planes.append((rng.random((H, W)) < rng.uniform(0.02, 0.6)).astype(np.uint8))
        m = torch.from_numpy(np.stack(planes)).to(DEV).view(len(planes), -1).contiguous()
        bits = ops.pack_mask_bits(m)
        got = plane_bboxes(bits, H, W).cpu().tolist()
        want = [_rle_to_bbox(_rle_counts(p), H, W) for p in planes]
        assert got == want, (H, W)
        assert plane_areas(bits).cpu().tolist() == [int(p.sum()) for p in planes]


def test_device_bboxes_areas_on_rle_with_null_frames():
    from s2d_amd.keymask.results_to_annotations import device_bboxes_areas
    from s2d_amd.rle import encode_video_predictions
    H, W = 21, 17
    rng = np.random.default_rng(2)
    m = (rng.random((1, 4, H, W)) < 0.1).astype(np.uint8)
    m[0, 1] = 0
    rles = encode_video_predictions(torch.from_numpy(m).to(DEV))[0]
    segs = [rles[0], None, rles[1], rles[3]]
    frames = [m[0, 0], None, m[0, 1], m[0, 3]]
    bb, ar = device_bboxes_areas(segs, H, W)
    assert bb == [None if f is None else [float(v) for v in _rle_to_bbox(_rle_counts(f), H, W)] for f in frames]
    assert ar == [None if f is None else int(f.sum()) for f in frames]


# ----------------------------------------------------------------------------------------------- synthetic YTVIS + the model
def _write_dataset(root, seed=0):
    """JPEG videos of mixed sizes (one EXIF-rotated), T not a multiple of SAMPLING_FRAME_NUM (3); GT: one track per video"""
    from PIL import Image
    from s2d_amd.rle import encode_video_predictions
    rng = np.random.default_rng(seed)
    specs = [(1, 90, 120, 4, None), (2, 120, 90, 5, None), (3, 72, 128, 7, 6), (4, 100, 100, 2, None)]
    videos, anns = [], []
    for vid, h, w, T, orient in specs:
        names = []
        os.makedirs(os.path.join(root, f"v{vid}"), exist_ok=True)
        yy, xx = np.mgrid[0:h, 0:w]
        for t in range(T):
            img = np.stack([(xx * 2 + t * 9) % 256, (yy * 3) % 256, ((xx + yy) * (vid + 1)) % 256], -1).astype(np.uint8)
            img = np.clip(img.astype(np.int32) + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
            name = f"v{vid}/{t:05d}.jpg"
            im = Image.fromarray(img)
            if orient is not None:
                ex = Image.Exif()
                ex[274] = orient
                im.save(os.path.join(root, name), quality=90, exif=ex)
            else:
                im.save(os.path.join(root, name), quality=90)
            names.append(name)
        H, W = (w, h) if orient in (5, 6, 7, 8) else (h, w)             # the size after the EXIF rotation
        videos.append({"id": vid, "height": H, "width": W, "length": T, "file_names": names})
        gm = np.zeros((1, T, H, W), np.uint8)
        gm[0, :, H // 4: H // 2, W // 3: 2 * W // 3] = 1
        segs = encode_video_predictions(torch.from_numpy(gm).to(DEV))[0]
        anns.append({"id": vid, "video_id": vid, "category_id": 1, "iscrowd": 0, "segmentations": segs,
                     "areas": [int(gm[0, t].sum()) for t in range(T)], "bboxes": [None] * T, "height": H, "width": W, "length": T})
    gt = {"info": {"description": "synthetic"}, "licenses": [], "categories": [{"id": 1, "name": "fg"}], "videos": videos,
          "annotations": anns}
    path = os.path.join(root, "gt.json")
    with open(path, "w") as fh:
        json.dump(gt, fh)
    return path


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ytvis"))
    return root, _write_dataset(root)


def _model(seed=0):
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TEST", MIN_TEST])
    torch.manual_seed(seed)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(DEV)
    with torch.no_grad():
        for p in model.teacher[1].predictor.class_embed.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
        model.teacher[1].predictor.class_embed.bias.copy_(torch.tensor([1.0, -1.0]))
    return cfg, model


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """a seeded KD model saved as a PLAIN checkpoint (backbone.* / sem_seg_head.*): loading fans it out to student and teacher"""
    from s2d_amd.checkpoint import kd_to_plain
    _, model = _model(0)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    path = str(tmp_path_factory.mktemp("ckpt") / "model.pth")
    torch.save({"model": kd_to_plain(sd), "iteration": 7}, path)
    return path


def _host_inputs(rec, min_size=int(MIN_TEST), max_size=1333):
    """host-only reference path: PIL decode + PIL resize + torch.as_tensor(arr.transpose(2, 0, 1))"""
    from PIL import Image
    from s2d_amd.data.augment import shortest_edge_shape
    from s2d_amd.data.test_loader import read_frame
    imgs = []
    for f in rec["file_names"]:
        a = read_frame(f)
        h, w = shortest_edge_shape(a.shape[0], a.shape[1], min_size, max_size)
        a = np.asarray(Image.fromarray(a).resize((w, h), Image.BILINEAR))
        imgs.append(torch.as_tensor(np.ascontiguousarray(a.transpose(2, 0, 1))))
    return dict(rec, image=imgs)


def test_loader_matches_host_pil_path_and_predictions(dataset):
    from s2d_amd.data.test_loader import YTVISTestLoader, load_videos
    root, gt = dataset
    recs = {r["video_id"]: r for r in load_videos(gt, root)}
    loader = YTVISTestLoader(gt, root, int(MIN_TEST), 1333, device=DEV, threads=4, prefetch=2)
    _, model = _model(1)
    model.eval()
    model.inference_rle = True
    seen = []
    for inp in loader:
        ref = _host_inputs(recs[inp["video_id"]])
        assert len(inp["image"]) == inp["length"] == len(ref["image"])
        assert set(inp) >= {"image", "height", "width", "length", "video_id", "file_names"}
        for a, b in zip(inp["image"], ref["image"]):
            assert a.is_cuda and a.dtype == torch.uint8 and a.shape == b.shape
            assert torch.equal(a.cpu(), b)
        o1 = model([inp])
        o2 = model([ref])
        assert o1["pred_scores"] == o2["pred_scores"] and o1["pred_labels"] == o2["pred_labels"]
        assert o1["pred_masks"] == o2["pred_masks"]
        seen.append(inp["video_id"])
    assert seen == [1, 2, 3, 4]
    assert recs[3]["height"] == 128                                       # the EXIF-rotated video is portrait after decode
    assert loader.wait_s >= 0.0


def test_loader_rejects_mixed_frame_sizes(tmp_path):
    from PIL import Image
    from s2d_amd.data.test_loader import YTVISTestLoader
    os.makedirs(tmp_path / "v")
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(tmp_path / "v" / "0.jpg")
    Image.fromarray(np.zeros((30, 20, 3), np.uint8)).save(tmp_path / "v" / "1.jpg")
    doc = {"videos": [{"id": 1, "height": 20, "width": 30, "length": 2, "file_names": ["v/0.jpg", "v/1.jpg"]}]}
    with pytest.raises(ValueError):
        list(YTVISTestLoader(doc, str(tmp_path), 16, 1333, device=DEV, threads=2, prefetch=1))


def test_weights_loaded_after_a_forward_take_effect(dataset, checkpoint):
    from s2d_amd.checkpoint import load_checkpoint
    from s2d_amd.data.test_loader import load_videos
    root, gt = dataset
    inp = _host_inputs(load_videos(gt, root)[0])
    _, fresh = _model(0)
    load_checkpoint(fresh, checkpoint)
    fresh.eval(); fresh.inference_rle = True
    want = fresh([inp])
    _, used = _model(42)                                                  # other weights, and a forward before the load
    used.eval(); used.inference_rle = True
    before = used([inp])
    info = load_checkpoint(used, checkpoint)
    assert not [k for k in info["missing"] if k.startswith("teacher.")] and not info["mismatched"]
    got = used([inp])
    assert got == want and before != want


def _run_driver(dataset, checkpoint, out, nproc=1, port=29681, extra=()):
    root, gt = dataset
    args = ["--config-file", KD_CFG, "--gt", gt, "--image-root", root, "--output-dir", str(out), "--weights", checkpoint,
            "--threads", "4", "INPUT.MIN_SIZE_TEST", MIN_TEST] + list(extra)
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    if nproc == 1:
        cmd = [sys.executable, "-m", "s2d_amd.evaluate"] + args
    else:
        env["MASTER_ADDR"] = "127.0.0.1"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
               "127.0.0.1", "--master-port", str(port), "-m", "s2d_amd.evaluate"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.fixture(scope="module")
def driver_run(dataset, checkpoint, tmp_path_factory):
    out = tmp_path_factory.mktemp("eval1")
    stdout = _run_driver(dataset, checkpoint, out)
    return out, stdout


def test_driver_metrics_equal_evaluate_ytvis(dataset, driver_run):
    from s2d_amd.ytvis_eval import derive_results, evaluate_ytvis
    _, gt = dataset
    out, stdout = driver_run
    line = json.loads([l for l in stdout.splitlines() if l.startswith("{")][-1])
    assert line["videos"] == 4 and line["frames"] == 18
    assert line["videos_per_s"] > 0 and 0.0 <= line["loader_wait_fraction"] <= 1.0
    results = json.load(open(out / "results.json"))
    assert {r["video_id"] for r in results} == {1, 2, 3, 4} and {r["category_id"] for r in results} == {1}
    assert all(len(r["segmentations"]) == {1: 4, 2: 5, 3: 7, 4: 2}[r["video_id"]] for r in results)
    metrics = json.load(open(out / "metrics.json"))
    ev = evaluate_ytvis(gt, str(out / "results.json"))
    ev.summarize(out=lambda *a, **k: None)
    assert json.dumps(metrics, sort_keys=True) == json.dumps(derive_results(ev.stats), sort_keys=True)    # nan compares as text


def test_driver_two_gloo_ranks_share_the_gpu(dataset, checkpoint, driver_run, tmp_path):
    out1, _ = driver_run
    _run_driver(dataset, checkpoint, tmp_path, nproc=2)
    key = lambda r: (r["video_id"], r["score"], json.dumps(r["segmentations"]))   # noqa: E731
    a = sorted(json.load(open(out1 / "results.json")), key=key)
    b = sorted(json.load(open(tmp_path / "results.json")), key=key)
    assert a == b


def test_driver_without_annotations_writes_results_only(dataset, checkpoint, tmp_path):
    root, gt = dataset
    doc = json.load(open(gt))
    doc.pop("annotations")
    p = tmp_path / "test_split.json"
    p.write_text(json.dumps(doc))
    _run_driver((root, str(p)), checkpoint, tmp_path / "out")
    assert (tmp_path / "out" / "results.json").exists() and not (tmp_path / "out" / "metrics.json").exists()


def test_pseudo_labels_from_driver_results_round_trip(dataset, driver_run, tmp_path):
    from s2d_amd.keymask.results_to_annotations import main
    from s2d_amd.ytvis_eval import GroundTruth, evaluate_ytvis
    _, gt = dataset
    out, _ = driver_run
    results = json.load(open(out / "results.json"))
    scores = sorted(r["score"] for r in results)
    thr = scores[len(scores) // 2]                                        # about half the predictions are skipped
    merged = tmp_path / "merged.json"
    merged.write_text(json.dumps({"categories": [{"id": 1, "name": "fg"}]}))
    main(["--annotation-file", str(merged), "--gt-annotation-file", gt, "--results-file", str(out / "results.json"),
          "--score-threshold", repr(thr), "--output-dir", str(tmp_path), "--output-filename", "pseudo"])
    doc = json.load(open(tmp_path / "pseudo.json"))
    kept = [i for i, r in enumerate(results) if r["score"] >= thr]
    assert [a["id"] for a in doc["annotations"]] == [i + 1 for i in kept]
    vids = {v["id"]: v for v in doc["videos"]}
    for a in doc["annotations"]:
        r = results[a["id"] - 1]
        assert a["segmentations"] == r["segmentations"] and a["video_id"] == r["video_id"]
        H, W = vids[a["video_id"]]["height"], vids[a["video_id"]]["width"]
        for s, bb, ar in zip(r["segmentations"], a["bboxes"], a["areas"]):
            counts = _counts_from_string(s["counts"])
            assert bb == [float(v) for v in _rle_to_bbox(counts, H, W)]
            assert ar == int(sum(counts[1::2]))
    # the pseudo annotations as ground truth: every kept prediction is its own ground truth, the skipped ones score lower
    GroundTruth(str(tmp_path / "pseudo.json"))
    assert all(sum(a["areas"]) > 0 for a in doc["annotations"])
    ev = evaluate_ytvis(str(tmp_path / "pseudo.json"), str(out / "results.json"))
    ev.summarize(out=lambda *a, **k: None)
    assert ev.stats[0] == 1.0


def _counts_from_string(s):
    """pycocotools rleFrString"""
    s = s.encode() if isinstance(s, str) else s
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, 1
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = c & 0x20
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts
