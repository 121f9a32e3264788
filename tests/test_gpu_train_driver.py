"""GPU checks of the training driver: the bit-plane mask warp and the HWC frame warp against the existing exports and the oracle,
map_clip against the host composition of the existing pieces, and `python -m s2d_amd.train` end to end (checkpoints, resume, eval,
two gloo ranks).  Every subprocess runs under a timeout."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
DEV = "cuda:0"


def _aug(min_size, crop=(40, 60)):
    from s2d_amd.data.augment import ClipAugmentation
    return ClipAugmentation(min_size=min_size, sample_style="choice_by_clip", random_flip="flip_by_clip",
                            augmentations=("brightness", "contrast", "rotation"), crop=("absolute_range", crop))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------ mask bit planes
@pytest.mark.parametrize("T,H0,W0,S,min_size,seed", [(3, 50, 75, 4, (37,), 0),    # W0 % 32 != 0, odd output size
                                                     (1, 64, 64, 3, (64,), 1),    # T = 1, W1 % 4 == 0 (vector stores)
                                                     (2, 33, 47, 0, (21,), 2),    # S = 0
                                                     (4, 45, 90, 6, (31,), 3)])
def test_warp_mask_bits_matches_u8_export_and_oracle(T, H0, W0, S, min_size, seed):
    from oracle import oracle_np
    from s2d_amd import ops
    from s2d_amd._lib import lib
    from s2d_amd.data.augment import warp_mask_bits
    rng = np.random.default_rng(seed)
    P = 5
    planes = (rng.random((P, H0, W0)) < 0.3).astype(np.uint8)
    planes[0, : H0 // 3, : W0 // 3] = 1
    plane_of = rng.integers(-1, P, (T, S)).astype(np.int32)              # -1: dummy slots
    if S:
        plane_of[-1, 0] = -1
    params, hw = _aug(min_size, crop=(min(H0, W0) // 2, min(H0, W0))).sample(T, H0, W0, rng=np.random.RandomState(seed))
    H1, W1 = hw
    p = torch.from_numpy(params).to(DEV)
    bits = ops.pack_mask_bits(torch.from_numpy(planes).to(DEV).view(P, -1).contiguous())
    out, area = warp_mask_bits(bits, plane_of, H0, W0, p, hw)
    torch.cuda.synchronize()
    assert out.shape == (T, S, H1, W1) and area.shape == (T, S)
    # the same planes unpacked to u8 [S][T][H0][W0] through the existing export
    u8 = np.zeros((S, T, H0, W0), np.uint8)
    for t in range(T):
        for s in range(S):
            if plane_of[t, s] >= 0:
                u8[s, t] = planes[plane_of[t, s]]
    want = np.zeros((S, T, H1, W1), np.uint8)
    if S:
        mo = torch.empty((S, T, H1, W1), device=DEV, dtype=torch.uint8)
        lib().call("s2d_aug_warp_masks_u8", torch.from_numpy(u8).to(DEV), S, T, H0, W0, p, H1, W1, mo, _stream())
        want = mo.cpu().numpy()
        np.testing.assert_array_equal(want, oracle_np.aug_warp_masks(u8, params, hw))
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, want.transpose(1, 0, 2, 3))
    assert area.cpu().numpy().tolist() == got.reshape(T, S, H1 * W1).sum(-1).tolist()
    if S:
        assert got.max() == 1 and (plane_of < 0).any() and all(not got[t, s].any() for t, s in zip(*np.nonzero(plane_of < 0)))


# ------------------------------------------------------------------------------------------------------------ HWC frame warp
@pytest.mark.parametrize("T,H0,W0,min_size,seed", [(3, 120, 200, (96,), 0), (2, 77, 61, (45,), 1), (1, 720, 1280, (360,), 2)])
def test_warp_frames_hwc_equals_chw_export(T, H0, W0, min_size, seed):
    from s2d_amd._lib import lib
    from s2d_amd.data.augment import augment_frames_hwc
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, (T, H0, W0, 3), dtype=np.uint8)
    params, hw = _aug(min_size, crop=(min(H0, W0) // 2, min(H0, W0))).sample(T, H0, W0, rng=np.random.RandomState(seed))
    assert (params[:, 11] != 1.0).all() and (params[:, 12] < 0).all()    # contrast on, the crop mean computed by the call
    H1, W1 = hw
    x = torch.from_numpy(fr).to(DEV)
    p_hwc = torch.from_numpy(params).to(DEV)
    p_chw = torch.from_numpy(params).to(DEV)
    got = augment_frames_hwc(x, p_hwc, hw)
    want = torch.empty((T, 3, H1, W1), device=DEV, dtype=torch.uint8)
    lib().call("s2d_aug_warp_frames_u8", x.permute(0, 3, 1, 2).contiguous(), T, H0, W0, p_chw, H1, W1, want, _stream())
    assert torch.equal(got, want)
    assert torch.equal(p_hwc, p_chw)                                     # same cmean bits, scratch words back to 0


# ------------------------------------------------------------------------------------------------------------ synthetic dataset
def _col_major_counts(m):
    """uncompressed COCO RLE counts of a [H, W] 0/1 mask (column-major runs, zeros first)"""
    flat = np.asarray(m, np.uint8).T.reshape(-1)
    counts, cur, n = [], 0, 0
    for v in flat:
        if v != cur:
            counts.append(n); cur, n = v, 0
        n += 1
    counts.append(n)
    return counts


def _write_dataset(root, seed=0):
    """JPEG videos; per video a compressed-RLE track, an uncompressed-RLE track with null frames, a small corner track that crops
    and rotations push out of the clip, and (video 1) a crowd track.  Categories 5 and 9 (contiguous 0 and 1)."""
    from PIL import Image
    from s2d_amd.rle import encode_video_predictions
    rng = np.random.default_rng(seed)
    specs = [(1, 90, 120, 8), (2, 120, 90, 7), (3, 72, 128, 9), (4, 100, 100, 6)]
    videos, anns, aid = [], [], 0
    for vid, H, W, T in specs:
        names = []
        os.makedirs(os.path.join(root, f"v{vid}"), exist_ok=True)
        yy, xx = np.mgrid[0:H, 0:W]
        for t in range(T):
            img = np.stack([(xx * 2 + t * 9) % 256, (yy * 3) % 256, ((xx + yy) * (vid + 1)) % 256], -1).astype(np.uint8)
            img = np.clip(img.astype(np.int32) + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
            name = f"v{vid}/{t:05d}.jpg"
            Image.fromarray(img).save(os.path.join(root, name), quality=90)
            names.append(name)
        videos.append({"id": vid, "height": H, "width": W, "length": T, "file_names": names})
        big = np.zeros((1, T, H, W), np.uint8)
        for t in range(T):
            big[0, t, H // 4 + t: H // 2 + t, W // 3: 2 * W // 3] = 1
        segs = encode_video_predictions(torch.from_numpy(big).to(DEV))[0]
        aid += 1
        anns.append({"id": aid, "video_id": vid, "category_id": 9, "iscrowd": 0, "segmentations": segs,
                     "bboxes": [[0, 0, 1, 1]] * T, "areas": [int(big[0, t].sum()) for t in range(T)]})
        segs, bbs = [], []
        for t in range(T):
            if t % 3 == 1:
                segs.append(None); bbs.append(None)
                continue
            m = np.zeros((H, W), np.uint8)
            m[H // 2:, : W // 2 - t] = 1
            m[rng.random((H, W)) < 0.05] = 1
            segs.append({"size": [H, W], "counts": _col_major_counts(m)}); bbs.append([0, 0, 1, 1])
        aid += 1
        anns.append({"id": aid, "video_id": vid, "category_id": 5, "segmentations": segs, "bboxes": bbs,
                     "areas": [None if s is None else 1 for s in segs]})
        corner = np.zeros((H, W), np.uint8)
        corner[:3, :3] = 1
        aid += 1
        anns.append({"id": aid, "video_id": vid, "category_id": 5, "iscrowd": 0,
                     "segmentations": [{"size": [H, W], "counts": _col_major_counts(corner)}] * T, "bboxes": [[0, 0, 3, 3]] * T,
                     "areas": [9] * T})
        if vid == 1:
            aid += 1
            anns.append({"id": aid, "video_id": vid, "category_id": 9, "iscrowd": 1, "segmentations": segs[:1] * T,
                         "bboxes": [[0, 0, 1, 1]] * T, "areas": [1] * T})
    doc = {"info": {}, "licenses": [], "categories": [{"id": 5, "name": "a"}, {"id": 9, "name": "b"}], "videos": videos,
           "annotations": anns}
    path = os.path.join(root, "train.json")
    with open(path, "w") as fh:
        json.dump(doc, fh)
    return path


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ytvis_train"))
    return root, _write_dataset(root)


def _counts_from_string(s):
    """pycocotools rleFrString: compressed RLE string -> run counts"""
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


def _rle_decode_host(seg, H, W):
    """numpy decode of a COCO RLE (compressed string or uncompressed counts), column-major"""
    c = seg["counts"]
    counts = _counts_from_string(c) if isinstance(c, str) else list(c)
    flat = np.zeros(H * W, np.uint8)
    pos, val = 0, 0
    for n in counts:
        flat[pos:pos + n] = val
        pos += n
        val ^= 1
    return flat.reshape(W, H).T


def _host_clip(record, py_rng, np_rng, st):
    """the host composition: read_frame -> numpy RLE decode -> augment_clip -> assemble_clip_instances, same generators"""
    from s2d_amd.data import assemble_clip_instances, augment_clip, dense_frame_selection
    from s2d_amd.data.test_loader import read_frame
    annos, L, H, W = record["annotations"], record["length"], record["height"], record["width"]
    sel = dense_frame_selection(annos, L, st.num_frames, st.frame_range, st.shuffle, py_rng, np_rng)
    T = len(sel)
    params, hw = st.aug.sample(T, H, W, rng=np_rng)
    frames = torch.stack([torch.from_numpy(np.ascontiguousarray(read_frame(record["file_names"][f]).transpose(2, 0, 1)))
                          for f in sel]).to(DEV)
    ids = sorted({a["id"] for f in sel for a in annos[f]})
    row = {i: n for n, i in enumerate(ids)}
    m = np.zeros((len(ids), T, H, W), np.uint8)
    for t, f in enumerate(sel):
        for a in annos[f]:
            m[row[a["id"]], t] = _rle_decode_host(a["segmentation"], H, W)
    img, mw = augment_clip(frames, torch.from_numpy(m).to(DEV) if ids else None, params, hw)
    warped = {}
    for t, f in enumerate(sel):
        warped[f] = [dict(a, mask=mw[row[a["id"]], t]) for a in annos[f]]
    inst = assemble_clip_instances(warped, sel, hw, st.num_classes, device=DEV)
    return img, inst


def test_map_clip_equals_host_composition(dataset):
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import ClipSettings, load_ytvis_train, map_clip
    root, path = dataset
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TRAIN", "(48, 61)", "INPUT.CROP.SIZE", "[40, 70]"])
    st = ClipSettings(cfg)
    recs = load_ytvis_train(path, root)
    dropped = crowd_seen = 0
    for k in range(12):
        rec = recs[k % len(recs)]
        got = map_clip(rec, random.Random(k), np.random.RandomState(k), st, device=DEV)
        img, inst = _host_clip(rec, random.Random(k), np.random.RandomState(k), st)
        assert len(got["image"]) == len(inst) == 3
        for t in range(3):
            assert torch.equal(got["image"][t], img[t])
            g, w = got["instances"][t], inst[t]
            assert g["gt_masks"].dtype == torch.bool and torch.equal(g["gt_masks"], w["gt_masks"])
            assert np.array_equal(g["gt_ids"], w["gt_ids"]) and np.array_equal(g["gt_classes"], w["gt_classes"])
            assert g["gt_ids"].dtype == np.int64 and g["gt_classes"].dtype == np.int64
            sel_f = rec["annotations"][int(rec["file_names"].index(got["file_names"][t]))]
            annotated = {a["id"] for a in sel_f if a.get("iscrowd", 0) == 0}
            dropped += len(annotated - set(g["gt_ids"].tolist()))
        crowd_seen += int(rec["video_id"] == 1)
        assert set(got) >= {"image", "instances", "height", "width", "length", "video_id", "file_names"}
    assert dropped > 0 and crowd_seen > 0                                 # filter_empty_instances and crowd slots exercised


def test_loader_batches_equal_map_clip(dataset):
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import ClipSettings, YTVISTrainLoader, batch_plan, clip_generators, load_ytvis_train, map_clip
    root, path = dataset
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TRAIN", "(48,)", "SOLVER.IMS_PER_BATCH", "2"])
    recs = load_ytvis_train(path, root)
    loader = YTVISTrainLoader.from_config(cfg, recs, seed=3, device=DEV, threads=4, prefetch=2)
    it = iter(loader)
    batches = [next(it) for _ in range(3)]
    it.close()
    plan = batch_plan(recs, 3, 2, 0, 1, True)
    st = ClipSettings(cfg)
    for b in batches:
        for d, (pos, i) in zip(b, next(plan)):
            want = map_clip(recs[i], *clip_generators(3, pos), st, device=DEV)
            assert d["video_id"] == want["video_id"]
            assert all(torch.equal(a, c) for a, c in zip(d["image"], want["image"]))
            assert all(torch.equal(a["gt_masks"], c["gt_masks"]) and np.array_equal(a["gt_ids"], c["gt_ids"])
                       for a, c in zip(d["instances"], want["instances"]))
    assert loader.wait_s >= 0.0


# ------------------------------------------------------------------------------------------------------------ the driver
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
              "SOLVER.CHECKPOINT_PERIOD", "3", "SEED", "1"]


def _run(module, args, nproc=1, port=29701, timeout=900):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    if nproc == 1:
        cmd = [sys.executable, "-m", module] + args
    else:
        env["MASTER_ADDR"] = "127.0.0.1"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
               "127.0.0.1", "--master-port", str(port), "-m", module] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-5000:])
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def _train(dataset, checkpoint, out, max_iter, extra=(), opts=(), nproc=1):
    root, path = dataset
    args = ["--config-file", KD_CFG, "--train-json", path, "--image-root", root, "--output-dir", str(out), "--weights", checkpoint,
            "--threads", "4"] + list(extra) + TRAIN_OPTS + ["SOLVER.MAX_ITER", str(max_iter)] + list(opts)
    return _run("s2d_amd.train", args, nproc)


@pytest.fixture(scope="module")
def run6(dataset, checkpoint, tmp_path_factory):
    root, path = dataset
    out = tmp_path_factory.mktemp("train6")
    lines = _train(dataset, checkpoint, out, 6, extra=["--eval-gt", path, "--eval-image-root", root])
    return out, lines


def test_driver_trains_checkpoints_and_evaluates(dataset, checkpoint, run6):
    from s2d_amd.checkpoint import plain_to_kd
    from s2d_amd.ytvis_eval import derive_results, evaluate_ytvis
    out, lines = run6
    assert lines[0]["start_iter"] == 0 and lines[0]["optimizer_step"] == 0
    summary = [l for l in lines if "iterations" in l][-1]
    assert summary["iterations"] == 6 and summary["clips_per_s"] > 0 and 0.0 <= summary["loader_wait_fraction"] <= 1.0
    recs = [json.loads(l) for l in open(out / "metrics.json")]
    assert [r["iteration"] for r in recs] == [5]
    assert all(np.isfinite(v) for k, v in recs[0].items() if isinstance(v, float)) and "total_loss" in recs[0] and recs[0]["lr"] > 0
    for name in ("model_0000002.pth", "model_0000005.pth", "model_final.pth"):
        assert (out / name).exists(), name
    assert (out / "last_checkpoint").read_text() == "model_final.pth"
    ck = torch.load(out / "model_final.pth", map_location="cpu", weights_only=True)
    assert set(ck) == {"model", "optimizer", "scheduler", "iteration", "seed"} and ck["iteration"] == 5 and ck["seed"] == 1
    init = plain_to_kd(torch.load(checkpoint, map_location="cpu", weights_only=True)["model"])
    fin = ck["model"]
    stud = [k for k in init if k.startswith("student.") and init[k].is_floating_point()]
    teach = [k for k in init if k.startswith("teacher.") and init[k].is_floating_point()]
    assert sum(not torch.equal(init[k], fin[k]) for k in stud) > len(stud) // 2
    assert any(not torch.equal(init[k], fin[k]) for k in teach)               # the EMA moved the teacher
    metrics = json.load(open(out / "inference" / "metrics.json"))
    ev = evaluate_ytvis(dataset[1], str(out / "inference" / "results.json"))
    ev.summarize(out=lambda *a, **k: None)
    assert json.dumps(metrics, sort_keys=True) == json.dumps(derive_results(ev.stats), sort_keys=True)


def test_driver_resume_and_evaluate_the_checkpoint(dataset, checkpoint, run6, tmp_path):
    import shutil
    root, path = dataset
    out, _ = run6
    res = tmp_path / "resumed"
    shutil.copytree(out, res)
    lines = _train(dataset, checkpoint, res, 8, extra=["--resume"], opts=["SEED", "-1"])
    assert lines[0]["start_iter"] == 6 and lines[0]["optimizer_step"] == 6
    assert lines[0]["seed"] == 1                                             # SEED -1: the first run's seed, from the checkpoint
    assert [l for l in lines if "iterations" in l][-1]["iterations"] == 2
    ck = torch.load(res / "model_final.pth", map_location="cpu", weights_only=True)
    assert ck["iteration"] == 7 and ck["scheduler"]["last_epoch"] == 8
    ev = _run("s2d_amd.evaluate", ["--config-file", KD_CFG, "--gt", path, "--image-root", root, "--output-dir", str(tmp_path / "ev"),
                                   "--weights", str(out / "model_final.pth"), "--threads", "4", "INPUT.MIN_SIZE_TEST", "64"])
    assert ev[-1]["videos"] == 4


def test_driver_two_gloo_ranks_share_the_gpu(dataset, checkpoint, tmp_path):
    lines = _train(dataset, checkpoint, tmp_path, 4, nproc=2)
    digests = {l["rank"]: l["student_digest"] for l in lines if "student_digest" in l}
    assert set(digests) == {0, 1} and digests[0] == digests[1]
    assert len([l for l in lines if "iterations" in l]) == 1                 # rank 0 alone reports and writes
    assert (tmp_path / "model_final.pth").exists() and (tmp_path / "model_0000002.pth").exists()
