"""CPU checks of the COCO image evaluator: the numpy restatement (tests/coco_refs.py) pinned on hand-computed cases, every named
case shown to have the property it is named for, and the parts of s2d_amd.coco_eval that need no device -- document and result
parsing, the test-format detection, and the host matching path given IoU matrices, which must equal the restatement on every
array."""
import numpy as np
import pytest

from tests import coco_refs as R


# ------------------------------------------------------------------------------------------------------------------ IoU refs
def test_mask_iou_hand_cases_and_crowd_rule():
    d = np.zeros((3, 4, 4), np.uint8)
    g = np.zeros((2, 4, 4), np.uint8)
    d[0, :2] = 1                    # 8 px
    d[1, 1:3, :2] = 1               # 4 px
    g[0, :, :2] = 1                 # 8 px; & d0 = 4, & d1 = 4
    g[1, :2, :3] = 1                # 6 px; & d0 = 6, & d1 = 2
    inter, ad, ag, iou = R.mask_iou(d, g, [0, 1])
    assert inter.tolist() == [[4, 6], [4, 2], [0, 0]] and ad.tolist() == [8, 4, 0] and ag.tolist() == [8, 6]
    assert iou[0, 0] == 4 / 12 and iou[1, 0] == 4 / 8                        # i / (a_d + a_g - i)
    assert iou[0, 1] == 6 / 8 and iou[1, 1] == 2 / 4                         # crowd: i / a_d
    assert iou[2, 0] == 0.0 and iou[2, 1] == 0.0                             # empty det: u = a_g, and u = 0 against the crowd
    assert R.mask_iou(d[2:], np.zeros((1, 4, 4), np.uint8), [0])[3][0, 0] == 0.0        # empty against empty: u = 0 -> 0


def test_bb_iou_hand_cases():
    dt = [[0, 0, 2, 2], [1, 1, 2, 2], [0.5, 0.25, 1.5, 2.0], [4, 4, 0, 3]]
    gt = [[0, 0, 2, 2], [2, 0, 2, 2], [0, 0, 4, 4]]
    o = R.bb_iou(dt, gt, [0, 0, 1])
    assert o[0, 0] == 1.0 and o[0, 1] == 0.0                                 # identical; touching edges: w = 0
    assert o[1, 0] == 1 / 7 and o[1, 1] == 1 / 7
    assert o[0, 2] == 1.0 and o[1, 2] == 1.0 and o[2, 2] == 1.0              # nested in a crowd: i / a_d
    assert o[2, 0] == (1.5 * 1.75) / (3.0 + 4.0 - 1.5 * 1.75)
    assert (o[3] == 0).all()                                                 # zero width: never a division


# ------------------------------------------------------------------------------------------------------------ named cases
def test_case_a_later_of_two_equal_ious_is_taken():
    e = R.solve(R.named_problems()["a_tie_later_gt_wins"])
    assert (e["dtMatches"][:3, 0] == 2).all() and (e["gtMatches"][:3, 0] == 0).all() and (e["gtMatches"][:3, 1] == 1).all()
    assert (e["dtMatches"][3:] == 0).all()                                   # 0.6 < 0.65


def test_case_b_iou_equal_to_a_threshold_matches_there():
    P = R.named_problems()
    e = R.solve(P["b_iou_equals_half"])
    assert R.IOU_THRS[0] == 0.5 and e["dtMatches"][0, 0] == 1 and (e["dtMatches"][1:] == 0).all()
    e = R.solve(P["b_iou_equals_three_quarters"])
    hit = [bool(3 / 4 >= t) for t in R.IOU_THRS]                             # against the array's own entries
    assert hit[4] and not hit[6] and hit[5] == (R.IOU_THRS[5] <= 0.75)
    assert (e["dtMatches"][:, 0] != 0).tolist() == hit


def test_case_c_crowd_takes_three_detections_and_all_are_ignored():
    e = R.solve(R.named_problems()["c_crowd_matched_by_three"])
    assert (e["dtMatches"][0] == 1).all() and e["dtIgnore"][0].all() and e["gtIgnore"].tolist() == [1]
    assert e["gtMatches"][0, 0] == 3                                         # the last detection that took it
    assert (e["dtMatches"][5] == [1, 1, 0]).all() and e["dtIgnore"][5].tolist() == [True, True, False]     # 0.7 < 0.75


def test_case_d_area_ignored_gt_sorts_last_and_the_scan_breaks():
    p = R.named_problems()["d_area_ignored_gt_and_break"]
    e = R.solve(p)
    assert e["gtIds"] == [2, 1] and e["gtIgnore"].tolist() == [0, 1]
    assert e["dtMatches"][0, 0] == 2 and not e["dtIgnore"][0, 0]             # t = .5: the regular gt (0.6), although 0.9 is on offer
    assert e["dtMatches"][3, 0] == 1 and e["dtIgnore"][3, 0]                 # t = .65: only the ignored one is left
    q = dict(p, a=0)                                                         # the same pair with both in range: 0.9 wins
    assert R.solve(q)["dtMatches"][0, 0] == 1


def test_case_e_empty_sides():
    P = R.named_problems()
    e = R.solve(P["e_no_detections"])
    assert e["dtMatches"].shape == (10, 0) and e["gtMatches"].shape == (10, 3) and (e["gtMatches"] == 0).all()
    e = R.solve(P["e_no_ground_truth"])
    assert e["dtMatches"].shape == (10, 2) and (e["dtMatches"] == 0).all() and not e["dtIgnore"].any()
    assert R.solve(P["e_neither"]) is None


def test_case_f_the_101st_detection_is_never_scored():
    p = R.named_problems()["f_101_detections"]
    e = R.solve(p)
    lowest = int(np.argmin(p["scores"])) + 1
    assert len(e["dtIds"]) == 100 and lowest not in e["dtIds"] and e["dtMatches"].shape == (10, 100)
    assert lowest not in e["gtMatches"]
    assert e["dtScores"] == sorted(p["scores"], reverse=True)[:100]


def test_case_g_unmatched_out_of_range_detection_is_ignored():
    e = R.solve(R.named_problems()["g_out_of_range_detections"])
    assert e["dtMatches"][0].tolist() == [1, 0, 0]
    assert e["dtIgnore"][0].tolist() == [False, True, False]                 # matched + large: kept; unmatched + large: ignored


def _perfect_dataset(n=12):
    """n images, one regular ground truth each, detection i is ground truth i exactly; distinct scores"""
    probs = [{"ious": np.ones((1, 1)), "scores": [0.9 - 0.01 * i], "dt_areas": [2000.0], "gt_areas": [2000.0], "crowd": [0], "a": 0}
             for i in range(n)]
    return probs


LONE = 1 / (1 + np.spacing(1))                                               # a single true positive: tp / (fp + tp + eps) < 1


def check_case_h(precision, recall, stats):
    """recall at maxDets 1 / 10 / 100 is 1/12, 10/12, 1"""
    assert (recall[:, 0, 0, 0] == 1 / 12).all() and (recall[:, 0, 0, 1] == 10 / 12).all() and (recall[:, 0, 0, 2] == 1.0).all()
    mean10 = lambda v: np.mean(np.full(10, v))                               # noqa: E731  (the stat is a mean over ten thresholds)
    assert stats[6] == mean10(1 / 12) and stats[7] == mean10(10 / 12) and stats[8] == 1.0
    assert (precision[:, :9, 0, 0, 0] == LONE).all() and (precision[:, 9:, 0, 0, 0] == 0.0).all()     # recall stops at 1/12 = 0.083
    assert (precision[:, :, 0, 0, 2] == 1.0).all()                           # from two on the envelope lifts it to exactly 1


def check_case_i(precision, recall):
    """the category whose only ground truth is a crowd stays -1; the other one is scored"""
    assert (precision[:, :, 1] == -1).all() and (recall[:, 1] == -1).all()
    assert (precision[:9, :, 0, 0, 2] == LONE).all() and (precision[9, :, 0, 0, 2] == 0).all()        # 0.9 < 0.95
    assert (recall[:9, 0, 0, 2] == 1.0).all() and recall[9, 0, 0, 2] == 0.0


def _both(name):
    """a dataset case through the restatement and through the product's host path -> (precision, recall, stats) of each"""
    from s2d_amd.coco_eval import COCOEval
    probs, n_cats, use_cats = R.dataset_cases()[name]
    doc, prod, ref = R.dataset_from_problems(probs, n_cats)
    _, precision, recall, stats = R.evaluate_dataset(ref, list(range(1, n_cats + 1)), use_cats=use_cats)
    ev = COCOEval(doc, use_cats=use_cats).evaluate(prod, matcher="host").accumulate()
    hstats = ev.summarize(out=None)
    assert np.array_equal(ev.eval["precision"], precision) and np.array_equal(ev.eval["recall"], recall) and np.array_equal(hstats, stats)
    return (precision, recall, stats), (ev.eval["precision"], ev.eval["recall"], hstats)


def test_case_h_accumulate_truncates_to_max_dets():
    for precision, recall, stats in _both("h_max_dets_truncation"):
        check_case_h(precision, recall, stats)


def test_case_i_category_without_regular_gt_stays_minus_one():
    for precision, recall, _ in _both("i_category_with_only_a_crowd"):
        check_case_i(precision, recall)


def test_case_j_perfect_predictions_score_one_in_every_populated_range():
    rng = np.random.default_rng(0)
    ims = []
    # two true positives at least in every range: a lone one has precision 1 / (1 + eps), which no envelope lifts to 1
    for n, (H, W) in enumerate([(40, 50), (120, 130), (140, 150), (200, 220), (240, 260)]):
        g = np.zeros((3, H, W), np.uint8)
        g[0, 2:12, 3:13] = 1                                                 # 100 px: small
        g[1, : H // 2, : W // 2] = 1
        g[2] = rng.random((H, W)) < 0.5
        crowd = [0, 0, 1]
        keep = [j for j in range(3) if not crowd[j]]
        _, ad, ag, iou = R.mask_iou(g[keep], g, crowd)
        ims.append({"dets": [{"id": 10 * n + i + 1, "score": 0.9 - 0.1 * i - 0.01 * n, "cat": 1, "area": float(ad[i])} for i in range(len(keep))],
                    "gts": [{"id": 10 * n + j + 1, "cat": 1, "crowd": crowd[j], "area": float(ag[j])} for j in range(3)], "ious": iou})
    _, precision, recall, stats = R.evaluate_dataset(ims, [1])
    populated = [a for a in range(4) if any(R.AREA_RNG[a][0] <= g["area"] <= R.AREA_RNG[a][1] and not g["crowd"] for im in ims for g in im["gts"])]
    assert populated == [0, 1, 2, 3]
    assert stats[0] == 1.0 and stats[8] == 1.0 and (stats[[1, 2, 3, 4, 5, 9, 10, 11]] == 1.0).all()
    assert (precision[:, :, 0, :, 2] == 1.0).all() and (recall[:, 0, :, 2] == 1.0).all()


# --------------------------------------------------------------------------------------------------- the product, no device
def _doc():
    return {"images": [{"id": 7, "height": 20, "width": 30, "file_name": "a.jpg"}, {"id": 3, "height": 10, "width": 12, "file_name": "b.jpg"}],
            "categories": [{"id": 5, "name": "x"}, {"id": 2, "name": "y"}],
            "annotations": [
                {"id": 1, "image_id": 7, "category_id": 5, "iscrowd": 0, "area": 12.5, "bbox": [1, 2, 3, 4],
                 "segmentation": [[1, 2, 4, 2, 4, 6, 1, 6]]},
                {"id": 2, "image_id": 7, "category_id": 2, "iscrowd": 1, "segmentation": {"size": [20, 30], "counts": [5, 10, 585]}},
                {"id": 3, "image_id": 3, "category_id": 2, "segmentation": {"size": [10, 12], "counts": "0X3"}}]}


def test_ground_truth_parsing():
    from s2d_amd.coco_eval import COCOGroundTruth
    gt = COCOGroundTruth(_doc())
    assert gt.img_ids == [3, 7] and gt.cat_ids == [2, 5] and gt.has_annotations
    a, b = gt.gts(7)
    assert (a.id, a.category_id, a.iscrowd, a.ignore, a.area, a.bbox) == (1, 5, 0, False, 12.5, [1, 2, 3, 4]) and isinstance(a.segmentation, list)
    assert (b.iscrowd, b.ignore, b.area, b.bbox) == (1, True, None, None) and isinstance(b.segmentation["counts"], list)
    c, = gt.gts(3)
    assert c.iscrowd == 0 and not c.ignore and isinstance(c.segmentation["counts"], str)
    assert gt.gts(99) == []
    doc = _doc()
    doc.pop("annotations")
    assert not COCOGroundTruth(doc).has_annotations
    with pytest.raises(ValueError):
        COCOGroundTruth({"videos": []})
    bad = _doc()
    bad["annotations"][0]["image_id"] = 99
    with pytest.raises(ValueError):
        COCOGroundTruth(bad)


def test_results_for_an_unknown_image_and_missing_areas_are_refused():
    from s2d_amd.coco_eval import COCOEval
    rec = {"dt_ids": [1], "scores": [0.5], "labels": [2], "areas": [4.0], "ious": np.zeros((1, 1))}
    with pytest.raises(ValueError, match="image 99"):
        COCOEval(_doc()).evaluate({99: rec}, matcher="host")
    with pytest.raises(ValueError, match="no area"):
        COCOEval(_doc()).evaluate({3: rec}, matcher="host")                  # annotation 3 has no `area`: evaluate_coco supplies it
    with pytest.raises(ValueError, match="matcher"):
        COCOEval(_doc()).evaluate({}, matcher="numpy", gt_areas={7: [12.5, 5.0], 3: [3.0]})


def test_test_format_detection_and_boundary_refusal():
    from s2d_amd.evaluate import parse_args, resolve_test_format
    coco, ytvis = _doc(), {"videos": [], "annotations": []}
    assert resolve_test_format("auto", coco) == "coco_image" and resolve_test_format("auto", ytvis) == "ytvis"
    assert resolve_test_format("ytvis", coco) == "ytvis" and resolve_test_format("coco_image", ytvis) == "coco_image"
    with pytest.raises(ValueError, match="boundary-ap"):
        resolve_test_format("auto", coco, boundary=True)
    assert resolve_test_format("auto", ytvis, boundary=True) == "ytvis"
    a = parse_args(["--config-file", "c", "--gt", "g", "--image-root", "r", "--output-dir", "o"])
    assert a.test_format == "auto"


@pytest.mark.parametrize("use_cats", [False, True])
def test_host_path_equals_the_restatement_on_every_array(use_cats):
    from s2d_amd.coco_eval import COCOEval
    probs = list(R.named_problems().values()) + R.random_problems(40, seed=5) + _perfect_dataset(3)
    doc, prod, ref = R.dataset_from_problems(probs, n_cats=3 if use_cats else 2)
    cats = [c["id"] for c in doc["categories"]]
    ev = COCOEval(doc, use_cats=use_cats).evaluate(prod, matcher="host").accumulate()
    stats = ev.summarize(out=None)
    cells, precision, recall, rstats = R.evaluate_dataset(ref, cats, use_cats=use_cats)
    assert len(ev.eval_imgs) == len(cells) == (3 if use_cats else 1) * 4 * len(probs)
    assert sum(e is None for e in cells) > 0 and sum(e is not None for e in cells) > 100
    for a, b in zip(ev.eval_imgs, cells):
        assert R.cells_equal(a, b)
    assert np.array_equal(ev.eval["precision"], precision) and np.array_equal(ev.eval["recall"], recall)
    assert np.array_equal(stats, rstats) and len(stats) == 12
    assert (precision > -1).any() and 0 < rstats[0] < 1


def test_summary_lines_and_derived_names():
    from s2d_amd.coco_eval import METRICS, COCOEval, derive_results
    doc, prod, _ = R.dataset_from_problems(_perfect_dataset(4))
    ev = COCOEval(doc).evaluate(prod, matcher="host").accumulate()
    lines = []
    stats = ev.summarize(out=lines.append)
    assert len(lines) == 12 and lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000"
    assert lines[9].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area= small")
    d = derive_results(stats)
    assert list(d) == METRICS and d["AP"] == 100.0 and d["AR100"] == 100.0 and np.isnan(d["APs"]) and d["APm"] == 100.0
