"""GPU checks of windowed inference (s2d_amd/modeling/window_inference.py, csrc/window.hip): the cross-window counts bit for bit
against numpy and against the composition of the existing mask ops, the track permutation recovered from shuffled windows, one
window == one clip, the first window untouched by the stitching, and the eval driver on videos that span several windows."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
DEV = "cuda:0"
TEST_KEYS = "MODEL.MASK_FORMER.TEST."


# ------------------------------------------------------------------------------------- the association rule, restated in numpy
def counts_np(a, b, Q):
    """inter [Q,Q], area_a [Q], area_b [Q] (int64) of the masks `logit > 0` of the first Q columns of two [n, ldq] blocks"""
    ma, mb = a[:, :Q] > 0, b[:, :Q] > 0
    inter = (ma.T.astype(np.float64) @ mb.astype(np.float64)).astype(np.int64)      # exact: every count is far below 2^53
    return inter, ma.sum(0).astype(np.int64), mb.sum(0).astype(np.int64)


def iou_cost_np(inter, area_a, area_b):
    """IoU = inter / (area_a[i] + area_b[j] - inter) in float32, 0 for an empty union; cost = 1 - IoU (float32)"""
    union = area_a[:, None] + area_b[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, inter.astype(np.float32) / union.astype(np.float32), np.float32(0.0)).astype(np.float32)
    return iou, (np.float32(1.0) - iou).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- 1. counts, bit-exact
def _logit_block(rng, n, Q, ldq):
    x = rng.standard_normal((n, ldq)).astype(np.float32)
    x[:, :Q] *= rng.uniform(0.2, 3.0, Q).astype(np.float32)
    x[:, :Q] -= rng.uniform(-1.0, 2.0, Q).astype(np.float32)                        # columns of different fill
    k = max(1, n * ldq // 50)
    x.reshape(-1)[rng.integers(0, n * ldq, k)] = 0.0                                # exact zeros: outside the mask
    x.reshape(-1)[rng.integers(0, n * ldq, k)] = -0.0                               # and negative zeros
    x[0, 0], x[n // 2, 0], x[n - 1, Q - 1] = 0.0, -0.0, -0.0                        # (some of them surely in query columns)
    if ldq > Q:
        x[:, Q:] = rng.uniform(0.5, 9.0, (n, ldq - Q)).astype(np.float32)           # pad columns: positive, must not be counted
    if Q > 2:
        x[:, 1] = -np.abs(x[:, 1]) - 1.0                                            # an empty mask
        x[:, 2] = np.abs(x[:, 2]) + 1.0                                             # a full one
    return x


COUNT_SIZES = [1 * 24 * 40, 4 * 92 * 160, 2 * 184 * 320, 1237, 4 * 92 * 160 + 17, 31]


@pytest.mark.parametrize("Q", [100, 9])
@pytest.mark.parametrize("n", COUNT_SIZES)
def test_pair_counts_equal_numpy_and_the_composition_of_existing_ops(Q, n):
    from s2d_amd import ops
    ldq = (Q + 3) // 4 * 4
    rng = np.random.default_rng(7 * n + Q)
    a, b = _logit_block(rng, n, Q, ldq), _logit_block(rng, n, Q, ldq)
    assert (a[:, :Q] == 0).any() and np.signbit(a[:, :Q][a[:, :Q] == 0]).any() and not np.isnan(a).any()
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    inter, area_a, area_b = ops.window_pair_counts(ad, bd, Q)
    assert inter.dtype == area_a.dtype == area_b.dtype == torch.int64
    want = counts_np(a, b, Q)
    got = [t.cpu().numpy() for t in (inter, area_a, area_b)]
    for g, w, name in zip(got, want, ("inter", "area_a", "area_b")):
        assert g.shape == w.shape and np.array_equal(g, w), (name, int(np.abs(g - w).max()))
    # the same counts from the existing ops: query-major byte planes -> bit words -> the pair counts of the 2Q set
    planes = torch.cat([(ad[:, :Q] > 0).t(), (bd[:, :Q] > 0).t()]).to(torch.uint8).contiguous()
    full = ops.mask_pair_counts(ops.pack_mask_bits(planes)).cpu().numpy()
    assert np.array_equal(full[:Q, Q:], got[0])
    assert np.array_equal(np.diagonal(full)[:Q], got[1]) and np.array_equal(np.diagonal(full)[Q:], got[2])


def test_scatter_columns_permutes_query_columns_and_copies_the_pad():
    from s2d_amd import ops
    rng = np.random.default_rng(3)
    for Q in (100, 9, 1):
        ldq = (Q + 3) // 4 * 4
        rows, R, row0 = 1237, 3000, 811
        src = rng.standard_normal((rows, ldq)).astype(np.float32)
        perm = rng.permutation(Q).astype(np.int32)
        dst0 = rng.standard_normal((R, ldq)).astype(np.float32)
        dst = torch.from_numpy(dst0).to(DEV)
        ops.window_scatter_columns(torch.from_numpy(src).to(DEV), torch.from_numpy(perm).to(DEV), dst, row0, Q)
        want = dst0.copy()
        want[row0:row0 + rows, :Q] = src[:, perm]
        want[row0:row0 + rows, Q:] = src[:, Q:]
        assert np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        ops.window_scatter_columns(torch.zeros((8, 12), device=DEV), torch.zeros((9,), device=DEV, dtype=torch.int32),
                                   torch.zeros((10, 12), device=DEV), 3, 9)


# ------------------------------------------------------------------------------------------------------ 2. permutation recovery
def _blob_video(seed=0, T=20, hm=48, wm=80, Q=100, nblob=30):
    """pixel-major logits [T*hm*wm, Q]: `nblob` columns hold a moving rectangle each (positive inside, negative outside; every
    rectangle stays inside its own 8 x 16 cell, so different blobs never meet, and the rectangles have distinct areas), the other
    columns are negative everywhere.  -> (logits, blob columns, per blob (cell y, cell x, h, w))"""
    rng = np.random.default_rng(seed)
    x = -rng.uniform(0.5, 5.0, (T, hm, wm, Q)).astype(np.float32)
    cols = np.sort(rng.choice(Q, nblob, replace=False))
    sizes, seen = [], set()
    for h in range(2, 7):
        for w in range(3, 13):
            if h * w not in seen:
                seen.add(h * w)
                sizes.append((h, w))
    sizes = [sizes[i] for i in rng.permutation(len(sizes))[:nblob]]
    assert len(sizes) == nblob and len({h * w for h, w in sizes}) == nblob
    geo = []
    for k, c in enumerate(cols):
        cy, cx = (k // 5) * 8, (k % 5) * 16
        h, w = sizes[k]
        geo.append((cy, cx, h, w))
        for t in range(T):
            y0, x0 = cy + t % 3, cx + t % 5
            x[t, y0:y0 + h, x0:x0 + w, c] = rng.uniform(0.5, 5.0, (h, w)).astype(np.float32)
    return x.reshape(T * hm * wm, Q), cols, geo


@pytest.mark.parametrize("shuffle_first", [False, True])
def test_stitch_recovers_shuffled_tracks(shuffle_first):
    from scipy.optimize import linear_sum_assignment
    from s2d_amd.modeling.window_inference import plan_windows, stitch
    T, hm, wm, Q, W, O = 20, 48, 80, 100, 8, 3
    hw = hm * wm
    orig, cols, geo = _blob_video()
    plan = plan_windows(T, W, O)
    assert plan == [(0, 8), (5, 13), (10, 18), (15, 20)]
    rng = np.random.default_rng(11)
    sig, wins, clss = [], [], []
    base_cls = rng.standard_normal((len(plan), Q, 2)).astype(np.float32)           # class logits per window and TRACK
    for w, (s, e) in enumerate(plan):
        ml = orig[s * hw:e * hw].copy()
        if w > 0:
            # the frames this window shares with its predecessor are not its own: there the two windows disagree by one pixel per
            # blob and frame, so the IoU of a true pair is (A - 1) / A with the blob's area A -- distinct per blob
            v = ml.reshape(e - s, hm, wm, Q)
            for (cy, cx, h, wd), c in zip(geo, cols):
                for t in range(O):
                    v[t, cy + (s + t) % 3, cx + (s + t) % 5, c] = -1.0
        p = rng.permutation(Q) if (w > 0 or shuffle_first) else np.arange(Q)
        sig.append(p)                                                              # query j of window w carries column p[j]
        wins.append(np.ascontiguousarray(ml[:, p]))
        clss.append(np.ascontiguousarray(base_cls[w][p]))
    record = []
    outs = ((torch.from_numpy(c).to(DEV), torch.from_numpy(m).to(DEV)) for c, m in zip(clss, wins))
    cls, buf = stitch(plan, outs, (Q, hm, wm), O, record)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got.shape == orig.shape
    blob_tracks = [p for p in range(Q) if sig[0][p] in set(cols)]
    assert len(blob_tracks) == 30
    for p in range(Q):
        if p in blob_tracks:                                                       # track p = query p of window 0 = column sig[0][p]
            assert np.array_equal(got[:, p].view(np.uint32), orig[:, sig[0][p]].view(np.uint32)), p
        else:
            assert (got[:, p] < 0).all(), p
    # class logits: the mean over the windows, in order, of the logits of the query that carries the track
    want_cls = base_cls[0][sig[0]].copy()
    for w in range(1, len(plan)):
        want_cls = want_cls + base_cls[w][sig[0]]
    want_cls = want_cls / np.float32(len(plan))
    assert np.array_equal(cls.cpu().numpy()[blob_tracks].view(np.uint32), want_cls[blob_tracks].view(np.uint32))
    # the matched pairs of every window pair == scipy's on the same float32 cost matrix, restricted to IoU > 0
    assert len(record) == len(plan) - 1
    for w, rec in enumerate(record, 1):
        s = plan[w][0]
        prev = wins[w - 1][(s - plan[w - 1][0]) * hw:(s - plan[w - 1][0] + O) * hw]
        cur = wins[w][:O * hw]
        iou, cost = iou_cost_np(*counts_np(prev, cur, Q))
        pos = np.sort(iou[iou > 0])
        assert len(pos) == 30 and (np.diff(pos) > 0).all(), "precondition: no two candidate pairs of equal positive IoU"
        assert np.array_equal(rec["cost"].cpu().numpy().view(np.uint32), cost.view(np.uint32))
        r, c = linear_sum_assignment(cost)
        want_pairs = {(int(i), int(j)) for i, j in zip(r, c) if iou[i, j] > 0}
        ip, ic, valid = (rec[k].cpu().numpy() for k in ("idx_prev", "idx_cur", "valid"))
        got_pairs = {(int(i), int(j)) for i, j, v in zip(ip, ic, valid) if v}
        assert got_pairs == want_pairs and len(got_pairs) == 30
        assert sorted(rec["perm"].cpu().tolist()) == list(range(Q))


# ------------------------------------------------------------------------------------------------ models with seeded weights
def _model(meta_arch, W, O, seed=0, on=True):
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(KD_CFG, ["MODEL.META_ARCHITECTURE", meta_arch, TEST_KEYS + "WINDOW_INFERENCE", str(on),
                               TEST_KEYS + "WINDOW_SIZE", str(W), TEST_KEYS + "WINDOW_OVERLAP", str(O)])
    torch.manual_seed(seed)
    model = META_ARCH_REGISTRY.get(meta_arch).from_config(cfg).to(DEV)
    head = model.teacher[1] if meta_arch == "KDVideoMaskFormer" else model.sem_seg_head
    with torch.no_grad():
        for p in head.predictor.class_embed.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
    return model.eval()


def _video(T, H=96, W=160, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    frames = []
    for t in range(T):
        base = torch.stack([(xx * 2 + t * 9) % 256, (yy * 3 + t * 5) % 256, (xx + yy + 11 * t) % 256]).to(torch.int32)
        frames.append((base + torch.randint(-20, 20, base.shape, generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8))
    return [{"image": frames, "height": H, "width": W}]


def _net_and_images(model, inputs):
    from s2d_amd import ops
    from s2d_amd.modeling.meta_arch import _frames_to_device
    images = ops.normalize_pad(_frames_to_device(inputs, model.device), model.size_divisibility,
                               model.pixel_mean.flatten().cpu().numpy(), model.pixel_std.flatten().cpu().numpy())
    if hasattr(model, "teacher"):
        return model.teacher, images
    return (lambda x, training: model.sem_seg_head(model.backbone(x), training)), images


def _forms(model, inputs):
    """the result dict in the three pred_masks forms: host bool tensors, COCO RLE, device u8"""
    out = {}
    for form in ("host", "rle", "device"):
        model.inference_rle, model.inference_device_masks = form == "rle", form == "device"
        with torch.no_grad():
            out[form] = model(inputs)
    model.inference_rle = model.inference_device_masks = False
    return out


def _same(a, b):
    assert a["pred_scores"] == b["pred_scores"] and a["pred_labels"] == b["pred_labels"] and a["image_size"] == b["image_size"]
    ma, mb = a["pred_masks"], b["pred_masks"]
    if isinstance(ma, torch.Tensor):
        assert torch.equal(ma, mb)
    elif ma and isinstance(ma[0], torch.Tensor):
        assert len(ma) == len(mb) and all(torch.equal(x, y) for x, y in zip(ma, mb))
    else:
        assert ma == mb


# ------------------------------------------------------------------------------------------- 3. one window equals one clip
@pytest.mark.parametrize("meta_arch", ["KDVideoMaskFormer", "VideoMaskFormer"])
def test_one_window_equals_one_clip(meta_arch):
    model = _model(meta_arch, 8, 2)
    assert model.window_inference and model.window_size == 8
    inputs = _video(6)
    on = _forms(model, inputs)
    assert model.last_windows == 1
    model.window_inference = False
    off = _forms(model, inputs)
    for form in on:
        assert len(on[form]["pred_scores"]) == 10
        _same(on[form], off[form])


# ---------------------------------------------------------------------------------------------- 4. first window untouched
@pytest.mark.parametrize("meta_arch", ["KDVideoMaskFormer", "VideoMaskFormer"])
def test_first_window_untouched_and_output_shapes(meta_arch):
    from s2d_amd.modeling.window_inference import run_windows
    T, W, O, H, Wd = 14, 6, 2, 96, 160
    model = _model(meta_arch, W, O)
    inputs = _video(T)
    net, images = _net_and_images(model, inputs)
    with torch.no_grad():
        cls, buf, dims, nwin = run_windows(net, images, W, O)
        clip = net(images[:W], False)
        hw = clip.hm * clip.wm
        first = clip.mask_logits[-1][0]
    assert nwin == 3 and dims == (T, clip.hm, clip.wm) and tuple(buf.shape) == (T * hw, first.shape[1])
    assert tuple(cls.shape) == tuple(clip.class_logits[-1][0].shape)
    assert torch.equal(buf[:W * hw].view(torch.int32), first.view(torch.int32))
    assert bool(torch.isfinite(buf).all())
    a = _forms(model, inputs)
    assert model.last_windows == 3
    b = _forms(model, inputs)
    K = len(a["host"]["pred_scores"])
    assert K == 10
    assert len(a["host"]["pred_masks"]) == K and all(tuple(m.shape) == (T, H, Wd) and m.dtype == torch.bool for m in a["host"]["pred_masks"])
    assert len(a["rle"]["pred_masks"]) == K and all(len(r) == T and r[0]["size"] == [H, Wd] for r in a["rle"]["pred_masks"])
    assert tuple(a["device"]["pred_masks"].shape) == (K, T, H, Wd) and a["device"]["pred_masks"].dtype == torch.uint8
    assert torch.equal(a["device"]["pred_masks"].cpu().bool(), torch.stack(a["host"]["pred_masks"]))
    for form in a:
        _same(a[form], b[form])


# ------------------------------------------------------------------------------------------------------------------ 5. driver
def _write_dataset(root, seed=0):
    """JPEG videos of mixed sizes (one EXIF-rotated), 4 / 5 / 7 / 2 frames; GT: one track per video (the builder of
    tests/test_gpu_eval_drivers.py)"""
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


def test_eval_driver_runs_videos_over_several_windows(tmp_path):
    from s2d_amd.config import load_config
    from s2d_amd.evaluate import evaluate_model
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    from s2d_amd.modeling.window_inference import plan_windows
    root = str(tmp_path / "ytvis")
    os.makedirs(root)
    gt = _write_dataset(root)
    W, O = 3, 1
    lengths = {1: 4, 2: 5, 3: 7, 4: 2}
    assert len(plan_windows(7, W, O)) == 3                                # the 7-frame video spans three windows
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TEST", "64", TEST_KEYS + "WINDOW_INFERENCE", "True", TEST_KEYS + "WINDOW_SIZE", str(W),
                               TEST_KEYS + "WINDOW_OVERLAP", str(O)])
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(DEV)
    with torch.no_grad():
        for p in model.teacher[1].predictor.class_embed.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
    out = tmp_path / "out"
    _, line = evaluate_model(cfg, model, gt, root, str(out), torch.device(DEV), threads=4, prefetch=2)
    assert line["videos"] == 4 and line["frames"] == 18
    assert line["windows"] == sum(len(plan_windows(T, W, O)) for T in lengths.values()) == 8
    results = json.load(open(out / "results.json"))
    assert len(results) == 4 * cfg.MODEL.MASK_FORMER.TEST.NUM_PREDICTIONS
    assert {r["video_id"] for r in results} == set(lengths)
    for r in results:
        assert len(r["segmentations"]) == lengths[r["video_id"]]
        assert all(isinstance(s, dict) and "counts" in s for s in r["segmentations"])
    assert (out / "metrics.json").exists()
    # switch off: one window per video
    model.window_inference = False
    _, line = evaluate_model(cfg, model, gt, root, str(tmp_path / "out1"), torch.device(DEV), threads=4, prefetch=2)
    assert line["windows"] == 4
