"""GPU checks of COCO Boundary AP: the ragged band kernel (csrc/mask_boundary.hip, erode_ragged_kernel) on chunks of images of
different sizes and radii against scipy's morphology, its refusals, and evaluate_coco(iou_type="boundary") -- IoUs, cells, precision,
recall and stats against tests/coco_boundary_refs.py --, the chained fallback, the worked case, COCOImageEvaluator, the command
line and the driver's --iou-types.  Every equality is exact."""
import json

import numpy as np
import pytest
import torch

from tests import boundary_refs as B
from tests import coco_boundary_refs as CB
from tests import coco_refs as R
from tests.test_gpu_coco_eval import KD_CFG, MIN_TEST, _rect_poly, _tight_box, _write_coco
from tests.test_gpu_train_driver import _col_major_counts
from tests.test_polygon_refs_cpu import fill_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADII = (1, 2, 3, 15, 16, 17, 31, 32, 33, 60, 64)
PATTERN = 0x5a5a5a5a
GAP = 7                                                                         # words of the image listed with F = 0


# ------------------------------------------------------------------------------------------------------------- ragged bands
def _shapes():
    s = dict(B.SHAPES)
    s["two_word_tiles"], s["two_row_bands"] = CB.EXTRA_SHAPES["two_word_tiles"], CB.EXTRA_SHAPES["two_row_bands"]
    return s


def _mixed_images():
    """every shape twice, each time with another radius: all of RADII occur, 150 x 1024 gets 60 (two row bands) and 15, 21 x 1100
    gets 33 (clamped to 11) and 3, and e.g. 1 x 70 at 64 or 64 x 64 at 32 have windows that do not fit"""
    shapes = list(_shapes().items())
    out = []
    for off in (9, 3):
        for n, (name, (H, W)) in enumerate(shapes):
            out.append((name, H, W, RADII[(n + off) % len(RADII)]))
    return out


@pytest.fixture(scope="module")
def band_cases():
    """(name, H, W, d) -> (masks bool [5, H, W], packed input with the padding bits set [5, wpp], packed reference band [5, wpp]):
    built and referenced once, left unchanged"""
    rng = np.random.default_rng(5)
    out = {}
    for key in _mixed_images():
        name, H, W, d = key
        masks = list(B.contents(rng, H, W).values()) + [B.discs(rng, H, W, edge=True)]
        src = np.stack([B.pack_bits(m, pad_ones=True) for m in masks])
        ref = np.stack([B.pack_bits(B.boundary_ref(m, d)) for m in masks])          # the unclamped d: the clamp must not show
        src.setflags(write=False), ref.setflags(write=False)
        out[key] = (np.stack(masks), src, ref)
    return out


def _i32(a):
    return torch.from_numpy(np.array(a, np.uint32).view(np.int32)).to(DEV)              # a copy: the cases stay read-only


def _check_chunk(band_cases, keys):
    """the images `keys` in one ragged call, an image with F = 0 and GAP words of its own in the middle"""
    from s2d_amd.coco_eval import LIB_CALLS, boundary_bands_ragged
    from s2d_amd.ytvis_eval import boundary_planes
    mid = len(keys) // 2
    spec, parts, word = [], [], 0
    for n, key in enumerate(keys):
        if n == mid:
            spec.append([word, 0, 480, 640, 16])
            parts.append(np.full(GAP, 0xffffffff, np.uint32))
            gap0, word = word, word + GAP
        _, H, W, d = key
        src = band_cases[key][1]
        spec.append([word, len(src), H, W, d])
        parts.append(src.reshape(-1))
        word += src.size
    bits = _i32(np.concatenate(parts))
    assert bits.numel() == word
    out = torch.full_like(bits, PATTERN)
    calls = LIB_CALLS["s2d_mask_boundary_ragged_u32"]
    got = boundary_bands_ragged(bits, spec, out=out)
    assert got is out and LIB_CALLS["s2d_mask_boundary_ragged_u32"] == calls + 1      # one library call, hence one launch
    second = boundary_bands_ragged(bits, spec)
    torch.cuda.synchronize()
    spec_planes = [s for s in spec if s[1]]
    unaligned = any(s[3] % 32 for s in spec_planes)
    host = out.cpu().numpy().view(np.uint32)
    for key, (w0, F, H, W, d) in zip(keys, spec_planes):
        wpp = (H * W + 31) // 32
        mine = host[w0:w0 + F * wpp].reshape(F, wpp)
        assert np.array_equal(mine, band_cases[key][2]), key                          # word for word, the padding bits included:
        if (H * W) % 32:                                                              # the reference packs them as 0
            assert (mine[:, -1] >> ((H * W) % 32) == 0).all(), key
        per_image = boundary_planes(bits[w0:w0 + F * wpp].view(F, wpp), H, W, d)
        assert torch.equal(per_image.reshape(-1), out[w0:w0 + F * wpp]), key
    gap = host[gap0:gap0 + GAP]
    assert (gap == (0 if unaligned else PATTERN)).all()                               # zeroed with the fill, else left alone
    mask = torch.ones(word, dtype=torch.bool, device=DEV)
    mask[gap0:gap0 + GAP] = bool(unaligned)
    assert torch.equal(second[mask], out[mask])                                       # a second call is bitwise equal


def test_ragged_bands_one_launch_over_a_mixed_chunk(band_cases):
    keys = _mixed_images()
    assert len(keys) == 24 and {k[3] for k in keys} == set(RADII)
    assert ("two_row_bands", 150, 1024, 60) in keys and CB.plan_rule(150, 1024, 60)[5] >= 2
    assert any(CB.clamp(H, W, d) < d for _, H, W, d in keys) and any(CB.clamp(H, W, d) == d and d >= 15 for _, H, W, d in keys)
    _check_chunk(band_cases, keys)


def test_ragged_bands_aligned_only_and_unaligned_only_chunks(band_cases):
    keys = _mixed_images()
    aligned = [k for k in keys if k[2] % 32 == 0]
    assert len(aligned) == 6 and {k[0] for k in aligned} == {"w32", "aligned", "two_row_bands"}
    _check_chunk(band_cases, aligned)                                                 # no zero fill: plain stores cover every word
    _check_chunk(band_cases, [k for k in keys if k[2] % 32])


def test_ragged_bands_refusals_launch_nothing(band_cases):
    from s2d_amd._lib import lib
    from s2d_amd.coco_eval import boundary_bands_ragged
    key = ("straddle", 40, 45, 17)
    src = band_cases[key][1]
    spec = np.array([[0, len(src), 40, 45, 17]], np.int64)
    bits = _i32(src.reshape(-1))
    out = torch.full_like(bits, PATTERN)
    plan, nwg, lds = np.zeros((1, 12), np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64)
    lib().call("s2d_mask_boundary_ragged_plan", spec, 1, bits.numel(), plan, nwg, lds)
    assert nwg[0] == 5 and plan[0, 4] == 17
    plan_dev = torch.from_numpy(plan).to(DEV)
    raw = lib()._raw_s2d_mask_boundary_ragged_u32
    stream = torch.cuda.current_stream().cuda_stream

    def call(b, ph, pd, o):
        return raw(b, bits.numel(), ph, pd, 1, o, stream)

    good = (bits.data_ptr(), plan.ctypes.data, plan_dev.data_ptr(), out.data_ptr())
    for col, delta in ((8, 1), (7, 1), (11, 1), (5, 1), (6, 1), (9, 1), (10, 1)):     # a derived column altered after planning
        bad = plan.copy()
        bad[0, col] += delta
        assert call(good[0], bad.ctypes.data, good[2], good[3]) == -1, col
    assert call(good[0], good[1], good[2], good[0]) == -1                             # out == bits
    for k in range(4):                                                               # a null pointer in each place
        args = list(good)
        args[k] = None
        assert call(*args) == -1, k
    torch.cuda.synchronize()
    assert (out == PATTERN).all()
    assert call(*good) == 0                                                          # the table itself is fine
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(src.shape), band_cases[key][2])
    for bad_spec in ([[0, 5, 150, 140, 65]], [[0, 6, 40, 45, 17]], [[0, -1, 40, 45, 17]], [[0, 1, 40, 45, 0]],
                     [[0, 2, 40, 45, 3], [57, 1, 40, 45, 3]]):
        with pytest.raises(ValueError):
            boundary_bands_ragged(bits, bad_spec)
    with pytest.raises(ValueError):
        boundary_bands_ragged(bits, spec, out=bits)


# ------------------------------------------------------------------------------------------------------------ the evaluator
def _urle(m):
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": [int(c) for c in _col_major_counts(m)]}


def _crle(m):
    from s2d_amd.rle import encode_video_predictions
    s = encode_video_predictions(torch.from_numpy(np.ascontiguousarray(m, np.uint8)[None, None]).to(DEV))[0][0]
    return dict(s, counts=s["counts"].decode() if isinstance(s["counts"], bytes) else s["counts"])


def _dataset(sizes, seed=0, poly=True):
    """-> (COCO document, results, {image id: (dt masks, gt masks)}): per image of sizes = [(H, W, n dets, n gts)] ground truth as
    compressed RLE, an uncompressed-RLE crowd and a polygon rectangle (integer corners), detections as shifted copies of the ground
    truths and random discs; categories 1 and 2; `area` on some annotations only"""
    rng = np.random.default_rng(seed)
    doc = {"images": [], "annotations": [], "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}]}
    results, masks = [], {}
    for n, (H, W, D, G) in enumerate(sizes):
        iid = n + 1
        doc["images"].append({"id": iid, "height": H, "width": W, "file_name": f"{iid}.jpg"})
        gm = []
        for j in range(G):
            kind = ("crle", "urle_crowd", "poly")[j % 3]
            if kind == "poly" and poly and H >= 8 and W >= 8:
                x0, y0 = int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2))
                seg = [_rect_poly(x0, y0, int(rng.integers(x0 + 2, W + 1)), int(rng.integers(y0 + 2, H + 1)))]
                m = fill_reference(seg, H, W)
            else:
                m = B.discs(rng, H, W, n=2, salt=0.0, edge=bool(j % 2)) if H * W > 1 else np.ones((1, 1), bool)
                seg = _urle(m) if kind == "urle_crowd" else _crle(m)
            a = {"id": len(doc["annotations"]) + 1, "image_id": iid, "category_id": int(rng.integers(1, 3)),
                 "iscrowd": int(kind == "urle_crowd"), "segmentation": seg}
            if j % 2 == 0:
                a["area"] = float(m.sum())
            doc["annotations"].append(a)
            gm.append(m)
        dm = []
        for i in range(D):
            if i < G:                                                          # a near copy: two columns to the right
                m = np.roll(gm[i], 2 if W > 4 else 0, axis=1)
            else:
                m = B.discs(rng, H, W, n=2, salt=0.0)
            results.append({"image_id": iid, "category_id": int(rng.integers(1, 3)), "score": round(0.99 - 0.013 * len(results), 4),
                            "segmentation": _urle(m) if i % 2 else _crle(m)})
            dm.append(m)
        masks[iid] = (dm, gm)
    return doc, results, masks


def _reference(doc, results, masks, ratio, use_cats):
    """-> ({image id: min IoU [D, G]}, cells, precision, recall, stats) by coco_boundary_refs"""
    ims, ious = [], {}
    for im in doc["images"]:
        iid, H, W = im["id"], im["height"], im["width"]
        anns = [a for a in doc["annotations"] if a["image_id"] == iid]
        idx = [n for n, r in enumerate(results) if r["image_id"] == iid]
        dm, gm = masks[iid]
        crowd = [a["iscrowd"] for a in anns]
        z = np.zeros((0, H, W), bool)
        iou, ad, ag = CB.min_iou_ref(np.stack(dm) if dm else z, np.stack(gm) if gm else z, crowd, CB.dilation(H, W, ratio))
        ious[iid] = iou
        ims.append({"dets": [{"id": n + 1, "score": results[n]["score"], "cat": results[n]["category_id"], "area": float(ad[k])}
                             for k, n in enumerate(idx)],
                    "gts": [{"id": a["id"], "cat": a["category_id"], "crowd": a["iscrowd"], "area": a.get("area", float(ag[j]))}
                            for j, a in enumerate(anns)], "ious": iou})
    return (ious,) + tuple(R.evaluate_dataset(ims, [1, 2], use_cats=use_cats))


SIZES = [(1, 1, 1, 1), (9, 33, 4, 3), (21, 1100, 5, 4), (64, 64, 6, 3), (40, 45, 3, 5), (37, 100, 4, 2),
         (50, 70, 3, 0), (7, 5, 0, 2), (12, 20, 0, 0)]                           # ..., detections only, ground truth only, neither


@pytest.fixture(scope="module")
def synthetic():
    doc, results, masks = _dataset(SIZES)
    assert any(isinstance(a["segmentation"], list) for a in doc["annotations"]) and sum(a["iscrowd"] for a in doc["annotations"]) >= 4
    refs = {uc: _reference(doc, results, masks, 0.02, uc) for uc in (False, True)}
    return doc, results, refs


def _same(ev, other):
    assert len(ev.eval_imgs) == len(other.eval_imgs)
    assert all(R.cells_equal(a, b) for a, b in zip(ev.eval_imgs, other.eval_imgs))
    assert np.array_equal(ev.eval["precision"], other.eval["precision"]) and np.array_equal(ev.eval["recall"], other.eval["recall"])
    assert np.array_equal(ev.summarize(out=None), other.summarize(out=None))


@pytest.mark.parametrize("use_cats", [False, True])
def test_evaluate_coco_boundary_equals_the_reference(synthetic, use_cats, monkeypatch):
    from s2d_amd import coco_eval
    doc, results, refs = synthetic
    ious, cells, precision, recall, stats = refs[use_cats]
    ev = coco_eval.evaluate_coco(doc, results, iou_type="boundary", use_cats=use_cats, device=DEV)
    assert ev.launches["boundary"] == 1 and ev.launches["iou"] == 2 and ev.launches["match"] == 1 and ev.launches["boundary_chained"] == 0
    seen = 0
    for (iid, cat), got in ev.ious.items():                                     # every IoU: the float64 reference minimum
        labels = [r["category_id"] for r in results if r["image_id"] == iid]
        scores = [r["score"] for r in results if r["image_id"] == iid]
        gcat = [a["category_id"] for a in doc["annotations"] if a["image_id"] == iid]
        cats = [cat] if use_cats else [1, 2]
        di = [i for c in cats for i, l in enumerate(labels) if l == c]
        di = [di[i] for i in np.argsort([-scores[i] for i in di], kind="mergesort")]
        gi = [j for c in cats for j, l in enumerate(gcat) if l == c]
        if di or gi:
            want = ious[iid][np.ix_(np.asarray(di, np.intp), np.asarray(gi, np.intp))]
            assert np.array_equal(np.asarray(got, np.float64).reshape(want.shape), want), (iid, cat)
            seen += want.size
    assert seen >= (60 if not use_cats else 10)
    assert len(ev.eval_imgs) == len(cells)
    for n, (a, b) in enumerate(zip(ev.eval_imgs, cells)):
        assert R.cells_equal(a, b), n
    assert np.array_equal(ev.eval["precision"], precision) and np.array_equal(ev.eval["recall"], recall)
    assert np.array_equal(ev.summarize(out=None), stats) and len(stats) == 12
    host = coco_eval.evaluate_coco(doc, results, iou_type="boundary", use_cats=use_cats, device=DEV, matcher="host")
    _same(host, ev)
    # one image per chunk: the image with neither detections nor ground truth is the only empty chunk
    monkeypatch.setattr(coco_eval, "CHUNK_WORDS", 1)
    many = coco_eval.evaluate_coco(doc, results, iou_type="boundary", use_cats=use_cats, device=DEV)
    assert many.launches["boundary"] == len(SIZES) - 1 and many.launches["iou"] == 2 * (len(SIZES) - 1)
    _same(many, ev)
    assert all(np.array_equal(np.asarray(many.ious[k]), np.asarray(ev.ious[k])) for k in ev.ious)


def test_boundary_differs_from_segm_and_segm_is_untouched(synthetic):
    """the min rule bites on this set (else the tests above would pass on mask IoU alone), and "segm" counts what it did"""
    from s2d_amd.coco_eval import evaluate_coco
    doc, results, refs = synthetic
    segm = evaluate_coco(doc, results, iou_type="segm", device=DEV)
    assert segm.launches["iou"] == 1 and "boundary" not in segm.launches
    bnd = evaluate_coco(doc, results, iou_type="boundary", device=DEV)
    lower = sum(int((np.asarray(bnd.ious[k]) < np.asarray(segm.ious[k])).sum()) for k in segm.ious if np.size(segm.ious[k]))
    assert lower >= 8 and all((np.asarray(bnd.ious[k]) <= np.asarray(segm.ious[k])).all() for k in segm.ious if np.size(segm.ious[k]))
    assert not np.array_equal(segm.summarize(out=None), bnd.summarize(out=None))


def test_chained_fallback_for_a_band_wider_than_one_pass():
    from s2d_amd.coco_eval import evaluate_coco
    ratio = 0.35
    assert CB.dilation(150, 140, ratio) == 72 and CB.clamp(150, 140, 72) == 70 and CB.clamp(40, 45, CB.dilation(40, 45, ratio)) <= 64
    doc, results, masks = _dataset([(40, 45, 3, 2), (150, 140, 4, 3), (9, 33, 2, 2)], seed=3)
    ious, cells, precision, recall, stats = _reference(doc, results, masks, ratio, False)
    ev = evaluate_coco(doc, results, iou_type="boundary", dilation_ratio=ratio, device=DEV)
    assert ev.launches["boundary_chained"] == 1 and ev.launches["boundary"] == 1 and ev.launches["iou"] == 2
    assert all(R.cells_equal(a, b) for a, b in zip(ev.eval_imgs, cells))
    assert np.array_equal(ev.eval["precision"], precision) and np.array_equal(ev.eval["recall"], recall)
    assert np.array_equal(ev.summarize(out=None), stats)
    got = np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in ev.ious.values()])
    assert np.array_equal(np.sort(got), np.sort(np.concatenate([v.reshape(-1) for v in ious.values()])))


def _square_set():
    doc, g, m = CB.square_doc()
    doc["annotations"][0]["segmentation"] = _crle(g)
    return doc, [{"image_id": 1, "category_id": 1, "score": 0.9, "segmentation": _urle(m)}]


def test_worked_case_through_the_device():
    from s2d_amd.coco_eval import evaluate_coco
    doc, results = _square_set()
    for ratio, iou, ap in ((0.02, 152 / 456, 0.0), (0.05, 560 / 840, 0.4)):
        ev = evaluate_coco(doc, results, iou_type="boundary", dilation_ratio=ratio, device=DEV)
        assert np.asarray(ev.ious[1, -1]).reshape(-1).tolist() == [iou]
        ap_got = float(ev.summarize(out=None)[0])
        assert abs(ap_got - ap) <= 1e-15 and (ap > 0 or ap_got == 0.0)           # a lone true positive: precision 1 / (1 + 2^-52)
    doc["annotations"][0]["iscrowd"] = 1                                         # the crowd rule on the bands: / |Bd(detection)|
    doc["annotations"].append(dict(doc["annotations"][0], id=2, iscrowd=0))      # (a regular one beside it, so that there is a cell)
    ev = evaluate_coco(doc, results, iou_type="boundary", dilation_ratio=0.05, device=DEV)
    assert np.asarray(ev.ious[1, -1]).reshape(-1).tolist() == [560 / 700, 560 / 840]
    segm = evaluate_coco(*_square_set(), iou_type="segm", device=DEV)
    assert np.asarray(segm.ious[1, -1]).reshape(-1).tolist() == [1520 / 1680] and abs(float(segm.summarize(out=None)[0]) - 0.9) <= 1e-15


def test_perfect_predictions_score_boundary_ap_one():
    from s2d_amd.coco_eval import evaluate_coco
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
        for j in range(3):
            seg = _crle(g[j])
            doc["annotations"].append({"id": 3 * n + j + 1, "image_id": n + 1, "category_id": 1, "iscrowd": int(j == 2),
                                       "segmentation": seg, "area": float(g[j].sum()), "bbox": _tight_box(g[j])})
            if j < 2:
                results.append({"image_id": n + 1, "category_id": 1, "score": 0.9 - 0.1 * j - 0.01 * n, "segmentation": seg})
    stats = evaluate_coco(doc, results, iou_type="boundary", device=DEV).summarize(out=None)
    assert stats[0] == 1.0 and stats[8] == 1.0
    assert (stats[[1, 2, 3, 4, 5, 9, 10, 11]] == 1.0).all(), stats.tolist()


def test_image_evaluator_returns_both_dicts(synthetic):
    from s2d_amd.coco_eval import METRICS, COCOImageEvaluator
    doc, results, _ = synthetic
    both = COCOImageEvaluator(json_file=doc, distributed=False, iou_types=("segm", "boundary"))
    both._records = list(results)
    default = COCOImageEvaluator(json_file=doc, distributed=False)
    default._records = list(results)
    a, b = both.evaluate(), default.evaluate()
    assert list(a) == ["segm", "boundary"] and list(b) == ["segm", "bbox"] and list(a["boundary"]) == METRICS
    assert json.dumps(a["segm"]) == json.dumps(b["segm"])                        # nan compares as text
    assert a["boundary"] != a["segm"] and both.coco_eval["boundary"].params.iouType == "boundary"


def test_command_line_prints_the_boundary_table(tmp_path, capsys):
    from s2d_amd.coco_eval import main
    doc, results = _square_set()
    (tmp_path / "gt.json").write_text(json.dumps(doc))
    (tmp_path / "res.json").write_text(json.dumps(results))
    main(["--gt", str(tmp_path / "gt.json"), "--results", str(tmp_path / "res.json"), "--iou-type", "boundary", "--dilation-ratio", "0.05"])
    lines = [l for l in capsys.readouterr().out.splitlines() if "Average" in l]
    assert len(lines) == 12 and lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.400"


def test_driver_writes_the_three_tables(tmp_path):
    """python -m s2d_amd.evaluate --iou-types segm,bbox,boundary (its main, in this process) on the image split of the COCO evaluator's
    tests: metrics.json holds the three dicts in the order asked for, and `boundary` is evaluate_coco's on the results written"""
    from s2d_amd.checkpoint import kd_to_plain
    from s2d_amd.coco_eval import METRICS, derive_results, evaluate_coco
    from s2d_amd.config import load_config
    from s2d_amd.evaluate import main
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    root = tmp_path / "coco"
    root.mkdir()
    gt = _write_coco(str(root))
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TEST", MIN_TEST])
    torch.manual_seed(0)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(DEV)
    with torch.no_grad():                                                       # as the COCO evaluator's tests seed it: some predictions
        for p in model.teacher[1].predictor.class_embed.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
        model.teacher[1].predictor.class_embed.bias.copy_(torch.tensor([1.0, -1.0]))
    ckpt = str(tmp_path / "model.pth")
    torch.save({"model": kd_to_plain({k: v.detach().cpu() for k, v in model.state_dict().items()}), "iteration": 1}, ckpt)
    del model
    out = tmp_path / "out"
    main(["--config-file", KD_CFG, "--gt", gt, "--image-root", str(root), "--output-dir", str(out), "--weights", ckpt, "--threads", "4",
          "--iou-types", "segm,bbox,boundary", "--dilation-ratio", "0.05", "INPUT.MIN_SIZE_TEST", MIN_TEST])
    metrics = json.load(open(out / "metrics.json"))
    assert list(metrics) == ["segm", "bbox", "boundary"] and all(list(metrics[k]) == METRICS for k in metrics)
    ev = evaluate_coco(gt, str(out / "coco_instances_results.json"), iou_type="boundary", dilation_ratio=0.05, device=DEV)
    assert json.dumps(metrics["boundary"]) == json.dumps(derive_results(ev.summarize(out=None)))
    with pytest.raises(ValueError, match="boundary-ap"):
        main(["--config-file", KD_CFG, "--gt", gt, "--image-root", str(root), "--output-dir", str(out), "--weights", ckpt, "--boundary-ap"])
