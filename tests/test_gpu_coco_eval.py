"""GPU checks of the COCO image evaluator: the ragged mask-IoU, box-IoU and matching kernels (csrc/coco_eval.hip) against the numpy
restatement of tests/coco_refs.py and the host matcher, `python -m s2d_amd.evaluate --test-format auto` on a COCO image file (1 and
2 ranks), and the training driver's eval hook on one.  Every subprocess runs under a timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import coco_refs as R
from tests.test_gpu_train_driver import _col_major_counts, _rle_decode_host
from tests.test_polygon_refs_cpu import fill_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
DEV = "cuda:0"
MIN_TEST = "64"


# ------------------------------------------------------------------------------------------------------------ ragged mask IoU
def _pack(masks, H, W, dirty=True):
    """uint8 [K, H, W] -> int32 CUDA bit planes [K, ceil(H*W/32)]; dirty: the bits past H*W of the last word are SET, so a kernel that
    counted them would be caught"""
    from s2d_amd import ops
    K = len(masks)
    if K == 0:
        return torch.empty((0, (H * W + 31) // 32), device=DEV, dtype=torch.int32)
    bits = ops.pack_mask_bits(torch.from_numpy(np.ascontiguousarray(masks, np.uint8)).to(DEV).view(K, H * W).contiguous())
    if dirty and K and (H * W) % 32:
        bits[:, -1] |= ((0xffffffff << ((H * W) % 32)) & 0xffffffff) - (1 << 32)          # the word's upper bits, as an int32
    return bits


def _planes(H, W, D, G, seed):
    """D detection and G ground-truth masks with the special planes in front: empty, full, one pixel"""
    rng = np.random.default_rng(seed)
    def draw(K, specials):
        m = (rng.random((K, H, W)) < rng.uniform(0.05, 0.7, (K, 1, 1))).astype(np.uint8)
        for k, s in enumerate(specials[:K]):
            m[k] = 0
            if s == "full":
                m[k] = 1
            elif s == "pixel":
                m[k, H - 1, W - 1] = 1                                   # the plane's last valid bit
        return m
    return draw(D, ["empty", "full", "pixel"] if D >= 3 else []), draw(G, ["empty", "pixel", "full"] if G >= 3 else [])


SMALL = [((5, 3), 0, 3), ((7, 9), 3, 0), ((33, 45), 1, 1), ((64, 64), 4, 5), ((37, 53), 101, 2)]


@pytest.fixture(scope="module")
def iou_cases():
    """name -> (H, W, dt masks, gt masks, crowd flags, reference tuple): built and referenced once, left unchanged"""
    out = {}
    for n, ((H, W), D, G) in enumerate(SMALL):
        d, g = _planes(H, W, D, G, n)
        crowd = [0] * G
        if (D, G) == (4, 5):
            crowd = [1, 0, 0, 1, 0]                   # g0 is empty and a crowd; d0 is empty: the crowd's detection has area 0 (u = 0)
            g[4] = 0                                  # g4 is empty and NOT a crowd: d0 against it is u = a_d + a_g - i = 0
        if (D, G) == (101, 2):
            crowd = [0, 1]
        out[f"{H}x{W}"] = (H, W, d, g, crowd)
    rng = np.random.default_rng(99)
    H, W = 480, 640
    d = np.zeros((100, H, W), np.uint8)
    g = np.zeros((7, H, W), np.uint8)
    for m in (d, g):
        for k in range(len(m)):
            y, x = rng.integers(0, H - 40), rng.integers(0, W - 40)
            m[k, y:y + rng.integers(8, 300), x:x + rng.integers(8, 300)] = 1
    d[:7, :, :] |= g * (rng.random((7, H, W)) < 0.9)                      # the first detections overlap the ground truths well
    out["480x640"] = (H, W, d, g, [0, 0, 0, 0, 0, 1, 0])
    ref = {k: R.mask_iou(v[2], v[3], v[4]) for k, v in out.items()}
    for r in ref.values():
        for a in r:
            a.setflags(write=False)
    return out, ref


def _check_ragged(cases, ref, names):
    from s2d_amd.coco_eval import mask_iou_ragged
    planes = [(_pack(cases[k][2], cases[k][0], cases[k][1]), _pack(cases[k][3], cases[k][0], cases[k][1]), cases[k][0], cases[k][1])
              for k in names]
    r = mask_iou_ragged(planes, [cases[k][4] for k in names], DEV)
    r2 = mask_iou_ragged(planes, [cases[k][4] for k in names], DEV)
    torch.cuda.synchronize()
    for t in ("iou", "inter", "area_d", "area_g"):
        assert torch.equal(getattr(r, t), getattr(r2, t)), t                              # a second call is bitwise equal
    iou, inter, ad, ag = (getattr(r, t).cpu().numpy() for t in ("iou", "inter", "area_d", "area_g"))
    for n, k in enumerate(names):
        ri, rad, rag, riou = ref[k]
        D, G = riou.shape
        assert np.array_equal(inter[r.pair0[n]:r.pair0[n + 1]].reshape(D, G), ri), k
        assert np.array_equal(ad[r.dt0[n]:r.dt0[n + 1]], rad) and np.array_equal(ag[r.gt0[n]:r.gt0[n + 1]], rag), k
        got = iou[r.pair0[n]:r.pair0[n + 1]].reshape(D, G)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), riou.view(np.int64)), k     # bit-equal
    return r


def test_ragged_mask_iou_small_images_in_one_chunk(iou_cases):
    cases, ref = iou_cases
    names = [f"{H}x{W}" for (H, W), _, _ in SMALL]
    assert all((H * W) % 32 for (H, W), _, _ in SMALL[:3] + SMALL[4:])                   # partial last words (64 x 64 is the aligned one)
    r = _check_ragged(cases, ref, names)
    assert r.pair0.tolist() == [0, 0, 0, 1, 21, 223] and r.iou.numel() == 223
    iou = ref["64x64"][3]
    assert iou[0, 0] == 0.0 and ref["64x64"][1][0] == 0 and cases["64x64"][4][0] == 1    # empty det against the empty crowd: u = 0 -> 0
    assert iou[1, 3] == ref["64x64"][0][1, 3] / 4096 and iou[1, 3] > 0                   # the full det against a crowd: i / a_d
    assert iou[0, 4] == 0.0 and ref["64x64"][2][4] == 0 and cases["64x64"][4][4] == 0    # empty det against an empty regular gt: u = 0
    assert iou[1, 4] == 0.0 and iou[1, 2] == 1.0                                         # full det against the empty / the full gt


def test_ragged_mask_iou_480x640_alone_and_sharing_a_chunk(iou_cases):
    cases, ref = iou_cases
    _check_ragged(cases, ref, ["480x640"])
    _check_ragged(cases, ref, ["7x9", "480x640", "64x64", "37x53"])
    assert (ref["480x640"][3] > 0.5).sum() >= 5


def test_ragged_mask_iou_refuses_mismatched_inputs():
    from s2d_amd.coco_eval import mask_iou_ragged
    b = _pack(np.zeros((2, 7, 9), np.uint8), 7, 9)
    with pytest.raises(ValueError):
        mask_iou_ragged([(b, b, 7, 10)], [[0, 0]], DEV)                                  # 63 pixels' planes for a 70-pixel image
    with pytest.raises(ValueError):
        mask_iou_ragged([(b, b, 7, 9)], [[0]], DEV)
    r = mask_iou_ragged([], [], DEV)
    assert r.iou.numel() == 0
    r = mask_iou_ragged([(None, None, 7, 9)], [[]], DEV)
    assert r.iou.numel() == 0 and r.area_d.numel() == 0


# ---------------------------------------------------------------------------------------------------------------- box IoU
def test_ragged_box_iou_bit_equal():
    from s2d_amd.coco_eval import box_iou_ragged
    rng = np.random.default_rng(4)
    hand_d = [[0, 0, 2, 2], [1, 1, 2, 2], [0.5, 0.25, 1.5, 2.0], [4, 4, 0, 3], [10.1, 10.7, 33.3, 7.9], [0.1, 0.2, 0.3, 0.7]]
    hand_g = [[0, 0, 2, 2], [2, 0, 2, 2], [0, 0, 4, 4], [9.9, 11.3, 40.7, 3.3], [100, 100, 5, 5], [0, 0, 50, 50]]
    # identical, touching (w = 0), disjoint, nested, zero-width, fractional; the last ground truth is a crowd
    dts = [np.array(hand_d, np.float64), rng.uniform(0, 50, (37, 4)), np.zeros((0, 4)), rng.uniform(0, 9, (3, 4)), rng.uniform(0, 600, (100, 4))]
    gts = [np.array(hand_g, np.float64), rng.uniform(0, 50, (9, 4)), rng.uniform(0, 9, (2, 4)), np.zeros((0, 4)), rng.uniform(0, 600, (7, 4))]
    crowds = [[0, 0, 0, 0, 0, 1], (rng.random(9) < 0.3).astype(int).tolist(), [0, 1], [], [0, 0, 1, 0, 0, 0, 0]]
    r = box_iou_ragged(dts, gts, crowds, DEV)
    r2 = box_iou_ragged(dts, gts, crowds, DEV)
    assert torch.equal(r.iou, r2.iou)
    got = r.iou.cpu().numpy()
    assert r.pair0.tolist() == [0, 36, 36 + 333, 369, 369, 369 + 700]
    for n, (d, g, c) in enumerate(zip(dts, gts, crowds)):
        want = R.bb_iou(d, g, c)
        assert np.array_equal(got[r.pair0[n]:r.pair0[n + 1]].reshape(want.shape).view(np.int64), want.view(np.int64)), n
    first = got[:36].reshape(6, 6)
    assert first[0, 0] == 1.0 and first[0, 1] == 0.0 and first[0, 4] == 0.0 and (first[3] == 0).all() and np.isfinite(got).all()
    assert first[0, 5] == 1.0 and 0 < first[4, 3] < 1                                   # nested in the crowd: i / a_d
    assert abs(first[5, 5] - 1.0) <= 2.0 ** -52                 # fractional corners: (0.3 + 0.1) - 0.1 is one ulp above 0.3, as in bbIou
    assert (got[36:369] > 0).sum() > 50


# ----------------------------------------------------------------------------------------------------------------- matching
def _three_way(probs, n_cats=1, use_cats=False):
    """the device matcher, the host matcher and the restatement on the same problems -> (device eval, reference cells)"""
    from s2d_amd.coco_eval import COCOEval
    doc, prod, ref = R.dataset_from_problems(probs, n_cats)
    cats = [c["id"] for c in doc["categories"]]
    dev = COCOEval(doc, use_cats=use_cats).evaluate(prod, matcher="device", device=DEV)
    host = COCOEval(doc, use_cats=use_cats).evaluate(prod, matcher="host")
    cells, precision, recall, stats = R.evaluate_dataset(ref, cats, use_cats=use_cats)
    assert dev.launches["match"] == int(any(p["ious"].size or sum(p["ious"].shape) for p in probs))   # one launch for all; none for nothing
    assert len(dev.eval_imgs) == len(host.eval_imgs) == len(cells)
    for n, (a, b, c) in enumerate(zip(dev.eval_imgs, host.eval_imgs, cells)):
        assert R.cells_equal(a, c), ("device", n)
        assert R.cells_equal(b, c), ("host", n)
        if a is not None:
            assert a["dtIgnore"].dtype == b["dtIgnore"].dtype == bool and a["dtMatches"].shape == b["dtMatches"].shape
    dev.accumulate(), host.accumulate()
    for ev in (dev, host):
        assert np.array_equal(ev.eval["precision"], precision) and np.array_equal(ev.eval["recall"], recall)
        assert np.array_equal(ev.summarize(out=None), stats)
    return dev, cells


def test_matching_named_cases_in_one_launch_and_one_by_one():
    named = R.named_problems()
    dev, cells = _three_way(list(named.values()))
    assert sum(c is None for c in cells) == 4                                            # (e) neither: no record in any range
    for name, p in named.items():
        d1, c1 = _three_way([p])
        assert R.cells_equal(d1.eval_imgs[p["a"]], R.solve(p)), name
    # the properties, on the device's output
    names = list(named)
    cell = lambda name: dev.eval_imgs[named[name]["a"] * len(names) + names.index(name)]   # noqa: E731
    assert (cell("a_tie_later_gt_wins")["dtMatches"][:3, 0] == cell("a_tie_later_gt_wins")["gtIds"][1]).all()
    assert cell("b_iou_equals_half")["dtMatches"][0, 0] != 0 and cell("b_iou_equals_three_quarters")["dtMatches"][5, 0] != 0
    assert cell("c_crowd_matched_by_three")["dtIgnore"][0].all() and (cell("c_crowd_matched_by_three")["dtMatches"][0] != 0).all()
    assert cell("d_area_ignored_gt_and_break")["gtIgnore"].tolist() == [0, 1] and not cell("d_area_ignored_gt_and_break")["dtIgnore"][0, 0]
    assert len(cell("f_101_detections")["dtIds"]) == 100
    assert cell("g_out_of_range_detections")["dtIgnore"][0].tolist() == [False, True, False]


def test_matching_dataset_cases_h_and_i():
    """(h) truncation to maxDets 1 / 10 and (i) a category whose only ground truth is a crowd: both in one launch and as launches
    of their own, device == host == restatement down to precision and recall, the named property on the device's output"""
    from tests.test_coco_refs_cpu import check_case_h, check_case_i
    cases = R.dataset_cases()
    (h,), _, _ = cases["h_max_dets_truncation"]
    (i,), n_cats, use_cats = cases["i_category_with_only_a_crowd"]
    _three_way([h, i], n_cats=2, use_cats=True)
    _three_way([h, i], n_cats=2, use_cats=False)
    dev, _ = _three_way([h], n_cats=1, use_cats=False)
    check_case_h(dev.eval["precision"], dev.eval["recall"], dev.stats)
    assert dev.eval_imgs[0]["dtMatches"].shape == (10, 12) and (dev.eval_imgs[0]["dtMatches"] != 0).all()
    dev, _ = _three_way([i], n_cats=n_cats, use_cats=use_cats)
    check_case_i(dev.eval["precision"], dev.eval["recall"])
    crowd_cells = dev.eval_imgs[4:]                                                      # category 2: its four ranges
    assert all(c["gtIgnore"].tolist() == [1] and c["dtMatches"].shape == (10, 0) for c in crowd_cells)


def test_match_kernel_raw_layout():
    """the documented index outputs of s2d_coco_match on case (a) and (c): sorted positions / detection positions, -1 for none"""
    from s2d_amd.coco_eval import AREA_RNG, match_ragged
    iou = torch.tensor([0.6, 0.6, 0.9, 0.8, 0.7], dtype=torch.float64, device=DEV)         # image 0: [1, 2]; image 1: [3, 1]
    groups = [[0, 2, 0, 0, 0, 1, 0, 2], [2, 1, 1, 2, 1, 3, 2, 1]]
    dtm, gtm, dti, gti, gpm = match_ragged(iou, groups, [0, 1, 2, 3], [0, 1, 2], [2000.0] * 4, [2000.0] * 3, [0, 0, 1], [0, 0, 1], R.IOU_THRS, AREA_RNG)
    T, A = 10, 4
    assert dtm.shape == (T * A * 4,) and gtm.shape == (T * A * 3,) and gpm.shape == (A * 3,)
    assert gpm[:2].tolist() == [0, 1] and gti[:2].tolist() == [0, 0]                      # group 0, range "all"
    assert dtm[0] == 1 and gtm[:2].tolist() == [-1, 0] and dtm[3] == -1                   # t = .5: the later gt; t = .65: none
    assert gti[2:4].tolist() == [1, 1]                                                   # range "small": both out of range
    db, gb = A * 1, A * 2                                                                # group 1: dsel0 = 1, gsel0 = 2
    assert dtm[T * db:T * db + 3].tolist() == [0, 0, 0] and gtm[T * gb] == 2 and dti[T * db:T * db + 3].tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        match_ragged(iou, [[0, 2, 0, 0, 0, 1, 0, 3]], [0], [0, 1, 2], [1.0], [1.0] * 3, [0] * 3, [0] * 3)      # column 2 of a 2-wide block


@pytest.fixture(scope="module")
def random200():
    return R.random_problems(200)


def test_matching_200_random_problems_one_launch(random200):
    dev, cells = _three_way(random200)
    assert sum(c is not None for c in cells) > 700
    ties = sum(int((np.unique(p["ious"], axis=None).size < p["ious"].size)) for p in random200)
    assert ties > 150                                                                    # the rational set makes equal IoUs the rule


def test_matching_random_problems_per_category(random200):
    _three_way(random200[:40], n_cats=3, use_cats=True)
    _three_way(random200[40:80], n_cats=3, use_cats=False)


# --------------------------------------------------------------------------------------------------------------- end to end
def _rect_poly(x0, y0, x1, y1):
    return [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]


def _write_coco(root):
    """five JPEGs of mixed sizes: one EXIF-rotated, one without annotations, one whose only annotation is a crowd; ground truth as
    polygons (integer corners: no pixel centre lies on an edge), compressed RLE and an uncompressed-RLE crowd"""
    from PIL import Image
    from s2d_amd.rle import encode_video_predictions
    rng = np.random.default_rng(1)
    specs = [(1, 90, 120, None), (2, 120, 90, None), (3, 72, 128, 6), (4, 100, 100, None), (5, 64, 80, None)]
    images, anns = [], []
    for iid, h, w, orient in specs:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 2 + iid * 9) % 256, (yy * 3) % 256, ((xx + yy) * (iid + 1)) % 256], -1).astype(np.uint8)
        img = np.clip(img.astype(np.int32) + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
        name = f"im{iid}.jpg"
        im = Image.fromarray(img)
        if orient is not None:
            ex = Image.Exif()
            ex[274] = orient
            im.save(os.path.join(root, name), quality=90, exif=ex)
        else:
            im.save(os.path.join(root, name), quality=90)
        H, W = (w, h) if orient in (5, 6, 7, 8) else (h, w)
        images.append({"id": iid, "height": H, "width": W, "file_name": name})

    def crle(m):
        return encode_video_predictions(torch.from_numpy(m[None, None]).to(DEV))[0][0]

    def add(iid, seg, crowd=0, **kw):
        anns.append(dict({"id": len(anns) + 1, "image_id": iid, "category_id": 1, "iscrowd": crowd, "segmentation": seg}, **kw))

    m = np.zeros((90, 120), np.uint8); m[20:60, 30:90] = 1
    add(1, [_rect_poly(10, 10, 50, 40), _rect_poly(60, 50, 100, 80)], area=2400.0, bbox=[10.0, 10.0, 90.0, 70.0])   # two polygons, one instance
    add(1, crle(m))                                                                       # no `area`, no `bbox`: from the mask
    c = np.zeros((90, 120), np.uint8); c[:, 100:] = 1
    add(1, {"size": [90, 120], "counts": _col_major_counts(c)}, crowd=1, area=float(c.sum()), bbox=[100.0, 0.0, 20.0, 90.0])
    add(2, [_rect_poly(5, 30, 85, 110)], area=6400.0)
    m = np.zeros((128, 72), np.uint8); m[32:64, 24:48] = 1
    add(3, crle(m), area=float(m.sum()), bbox=[24.0, 32.0, 24.0, 32.0])
    c = np.zeros((64, 80), np.uint8); c[10:50, 10:70] = 1
    add(5, {"size": [64, 80], "counts": _col_major_counts(c)}, crowd=1)
    doc = {"info": {}, "licenses": [], "categories": [{"id": 1, "name": "fg"}], "images": images, "annotations": anns}
    path = os.path.join(root, "instances.json")
    with open(path, "w") as fh:
        json.dump(doc, fh)
    return path


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("coco"))
    return root, _write_coco(root)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from s2d_amd.checkpoint import kd_to_plain
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TEST", MIN_TEST])
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(DEV)
    with torch.no_grad():
        for p in model.teacher[1].predictor.class_embed.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
        model.teacher[1].predictor.class_embed.bias.copy_(torch.tensor([1.0, -1.0]))
    path = str(tmp_path_factory.mktemp("ckpt") / "model.pth")
    torch.save({"model": kd_to_plain({k: v.detach().cpu() for k, v in model.state_dict().items()}), "iteration": 7}, path)
    return path


def _run(module, args, nproc=1, port=29721, timeout=600):
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


def _evaluate(dataset, checkpoint, out, nproc=1, extra=()):
    root, gt = dataset
    return _run("s2d_amd.evaluate", ["--config-file", KD_CFG, "--gt", gt, "--image-root", root, "--output-dir", str(out), "--weights", checkpoint,
                                     "--threads", "4", "--test-format", "auto"] + list(extra) + ["INPUT.MIN_SIZE_TEST", MIN_TEST], nproc)


@pytest.fixture(scope="module")
def driver_run(dataset, checkpoint, tmp_path_factory):
    out = tmp_path_factory.mktemp("eval1")
    return out, _evaluate(dataset, checkpoint, out)


def _tight_box(m):
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def _gt_mask(a, H, W):
    seg = a["segmentation"]
    return fill_reference(seg, H, W).astype(np.uint8) if isinstance(seg, list) else _rle_decode_host(seg, H, W)


def _host_reference(doc, results, iou_type):
    """the numpy restatement fed with host-decoded masks: -> (precision, stats)"""
    by_img = {}
    for n, r in enumerate(results):
        by_img.setdefault(r["image_id"], []).append(n)
    ims = []
    for im in sorted(doc["images"], key=lambda i: i["id"]):
        H, W = im["height"], im["width"]
        anns = [a for a in doc["annotations"] if a["image_id"] == im["id"]]
        gm = [_gt_mask(a, H, W) for a in anns]
        idx = by_img.get(im["id"], [])
        dm = [_rle_decode_host(results[n]["segmentation"], H, W) for n in idx]
        crowd = [a["iscrowd"] for a in anns]
        if iou_type == "segm":
            _, ad, ag, iou = R.mask_iou(np.zeros((0, H, W), np.uint8) if not dm else np.stack(dm),
                                        np.zeros((0, H, W), np.uint8) if not gm else np.stack(gm), crowd)
            d_area, g_area = [float(a) for a in ad], [float(a) for a in ag]
        else:
            db = [_tight_box(m) for m in dm]
            gb = [a["bbox"] if "bbox" in a else _tight_box(m) for a, m in zip(anns, gm)]
            iou = R.bb_iou(db, gb, crowd)
            d_area, g_area = [b[2] * b[3] for b in db], [b[2] * b[3] for b in gb]
        ims.append({"dets": [{"id": n + 1, "score": results[n]["score"], "cat": results[n]["category_id"], "area": d_area[k]}
                             for k, n in enumerate(idx)],
                    "gts": [{"id": a["id"], "cat": a["category_id"], "crowd": a["iscrowd"], "area": a.get("area", g_area[j])}
                            for j, a in enumerate(anns)], "ious": iou})
    _, precision, _, stats = R.evaluate_dataset(ims, [c["id"] for c in doc["categories"]])
    return precision, stats


def test_evaluate_driver_on_coco_images(dataset, driver_run):
    from s2d_amd.coco_eval import METRICS, derive_results, evaluate_coco
    _, gt = dataset
    out, lines = driver_run
    line = lines[-1]
    assert line["images"] == 5 and line["frames"] == 5 and line["images_per_s"] > 0 and "videos" not in line
    assert 0.0 <= line["loader_wait_fraction"] <= 1.0
    assert not (out / "results.json").exists()
    results = json.load(open(out / "coco_instances_results.json"))
    doc = json.load(open(gt))
    sizes = {im["id"]: [im["height"], im["width"]] for im in doc["images"]}
    assert {r["image_id"] for r in results} == {1, 2, 3, 4, 5} and {r["category_id"] for r in results} == {1}
    assert [r["image_id"] for r in results] == sorted(r["image_id"] for r in results)
    for r in results:
        assert set(r) == {"image_id", "category_id", "score", "segmentation"} and isinstance(r["score"], float)
        assert r["segmentation"]["size"] == sizes[r["image_id"]] and isinstance(r["segmentation"]["counts"], str)
    assert sizes[3] == [128, 72]                                                         # the EXIF-rotated image is portrait
    metrics = json.load(open(out / "metrics.json"))
    assert list(metrics) == ["segm", "bbox"] and all(list(metrics[k]) == METRICS for k in metrics)
    for t in ("segm", "bbox"):
        ev = evaluate_coco(gt, str(out / "coco_instances_results.json"), iou_type=t, device=DEV)
        stats = ev.summarize(out=None)
        assert json.dumps(metrics[t]) == json.dumps(derive_results(stats)), t            # nan compares as text
        host = evaluate_coco(gt, results, iou_type=t, device=DEV, matcher="host")
        assert np.array_equal(host.eval["precision"], ev.eval["precision"]) and np.array_equal(host.summarize(out=None), stats)
        precision, rstats = _host_reference(doc, results, t)
        assert np.array_equal(ev.eval["precision"], precision), t
        assert np.array_equal(stats, rstats), t
        assert ev.launches["iou"] == 1 and ev.launches["match"] == 1
    # the seeded model's masks hardly overlap the ground truth: the same comparison with good detections added -- every regular
    # ground truth shifted by two pixels, as an uncompressed RLE beside the driver's compressed ones
    extra = []
    for a in doc["annotations"]:
        if not a["iscrowd"]:
            H, W = sizes[a["image_id"]]
            m = np.roll(_gt_mask(a, H, W), 2, axis=1)
            m[:, :2] = 0
            extra.append({"image_id": a["image_id"], "category_id": 1, "score": 0.99 - 0.01 * len(extra),
                          "segmentation": {"size": [H, W], "counts": [int(c) for c in _col_major_counts(m)]}})
    for t in ("segm", "bbox"):
        ev = evaluate_coco(doc, results + extra, iou_type=t, device=DEV)
        precision, rstats = _host_reference(doc, results + extra, t)
        stats = ev.summarize(out=None)
        assert np.array_equal(ev.eval["precision"], precision) and np.array_equal(stats, rstats), t
        # a copy overlaps its ground truth by (w - 2) / (w + 2) >= 22 / 26 = 0.846 (the narrowest rectangle is 24 wide), so at the
        # seven thresholds up to 0.8 every regular ground truth is matched, by its copy or by a detection that scored higher: AR100 >=
        # 0.7.  AP has no such floor: the model's detections may outscore the copies.
        assert stats[8] >= 0.7 and stats[0] > 0, t


def test_evaluate_driver_two_gloo_ranks_write_the_same_results(dataset, checkpoint, driver_run, tmp_path):
    out1, _ = driver_run
    lines = _evaluate(dataset, checkpoint, tmp_path, nproc=2)
    assert sorted(l["images"] for l in lines if "images" in l) == [2, 3]
    assert json.load(open(out1 / "coco_instances_results.json")) == json.load(open(tmp_path / "coco_instances_results.json"))
    assert (out1 / "metrics.json").read_text() == (tmp_path / "metrics.json").read_text()


def test_evaluate_driver_refuses_boundary_ap_and_skips_metrics_without_annotations(dataset, checkpoint, tmp_path):
    from s2d_amd.evaluate import main
    root, gt = dataset
    with pytest.raises(ValueError, match="boundary-ap"):
        main(["--config-file", KD_CFG, "--gt", gt, "--image-root", root, "--output-dir", str(tmp_path / "b"), "--weights", checkpoint,
              "--boundary-ap"])
    doc = json.load(open(gt))
    doc.pop("annotations")
    p = tmp_path / "test_split.json"
    p.write_text(json.dumps(doc))
    _evaluate((root, str(p)), checkpoint, tmp_path / "out")
    assert (tmp_path / "out" / "coco_instances_results.json").exists() and not (tmp_path / "out" / "metrics.json").exists()


def test_image_loader_decodes_concurrently_in_order(dataset):
    from s2d_amd.data.coco_image_loader import COCOImageTestLoader, images_as_videos
    from s2d_amd.data.test_loader import YTVISTestLoader
    root, gt = dataset
    loader = COCOImageTestLoader(gt, root, int(MIN_TEST), 1333, device=DEV, threads=3, prefetch=2)
    video = YTVISTestLoader(images_as_videos(gt), root, int(MIN_TEST), 1333, device=DEV, threads=1, prefetch=1)
    seen = []
    for a, b in zip(loader, video):
        assert a["image_id"] == a["video_id"] == b["video_id"] and a["length"] == 1 and len(a["image"]) == 1
        assert a["file_name"] == b["file_names"][0] and a["image"][0].is_cuda and a["image"][0].dtype == torch.uint8
        assert torch.equal(a["image"][0], b["image"][0])
        seen.append(a["image_id"])
    assert seen == [1, 2, 3, 4, 5]


def test_perfect_predictions_score_one_on_the_device(tmp_path):
    """case (j): the non-crowd ground-truth masks as predictions, distinct scores, `bbox` and `area` written from the masks: AP =
    AR100 = 1.0 exactly in every area range (each holds at least two ground truths: a lone true positive has precision
    1 / (1 + eps))"""
    from s2d_amd.coco_eval import evaluate_coco
    from s2d_amd.rle import encode_video_predictions
    rng = np.random.default_rng(0)
    doc = {"images": [], "annotations": [], "categories": [{"id": 1, "name": "fg"}]}
    results = []
    for n, (H, W) in enumerate([(40, 50), (120, 130), (140, 150), (200, 220), (240, 260)]):
        g = np.zeros((3, H, W), np.uint8)
        g[0, 2:12, 3:13] = 1
        g[1, : H // 2, : W // 2] = 1
        g[1, 0, 0] = 0
        g[2] = rng.random((H, W)) < 0.5
        doc["images"].append({"id": n + 1, "height": H, "width": W, "file_name": f"{n}.jpg"})
        segs = encode_video_predictions(torch.from_numpy(g[:, None]).to(DEV))
        for j in range(3):
            doc["annotations"].append({"id": 3 * n + j + 1, "image_id": n + 1, "category_id": 1, "iscrowd": int(j == 2),
                                       "segmentation": segs[j][0], "area": float(g[j].sum()), "bbox": _tight_box(g[j])})
            if j < 2:
                results.append({"image_id": n + 1, "category_id": 1, "score": 0.9 - 0.1 * j - 0.01 * n, "segmentation": segs[j][0]})
    for t in ("segm", "bbox"):
        ev = evaluate_coco(doc, results, iou_type=t, device=DEV)
        stats = ev.summarize(out=None)
        assert stats[0] == 1.0 and stats[8] == 1.0, t
        assert (stats[[1, 2, 3, 4, 5, 9, 10, 11]] == 1.0).all(), (t, stats.tolist())
        assert (ev.eval["precision"][:, :, 0, :, 2] == 1.0).all()


# -------------------------------------------------------------------------------------------------------------- training hook
def test_training_hook_scores_an_image_eval_file(dataset, checkpoint, tmp_path):
    from s2d_amd.coco_eval import METRICS
    root, gt = dataset
    out = tmp_path / "train"
    lines = _run("s2d_amd.train", ["--config-file", KD_CFG, "--train-json", gt, "--image-root", root, "--output-dir", str(out), "--weights",
                                   checkpoint, "--threads", "4", "--eval-gt", gt, "--eval-image-root", root, "INPUT.MIN_SIZE_TRAIN", "(64,)",
                                   "INPUT.MIN_SIZE_TEST", MIN_TEST, "SOLVER.IMS_PER_BATCH", "2", "SOLVER.BASE_LR", "1e-4", "SEED", "1",
                                   "SOLVER.MAX_ITER", "2"], timeout=900)
    ev = [l for l in lines if "eval_iteration" in l][-1]
    assert ev["eval_iteration"] == 1 and ev["images"] == 5 and "segm" in ev and "bbox" in ev
    metrics = json.load(open(out / "inference" / "metrics.json"))
    assert list(metrics) == ["segm", "bbox"] and list(metrics["segm"]) == METRICS and list(metrics["bbox"]) == METRICS
    assert (out / "inference" / "coco_instances_results.json").exists()
