"""Host stage of the YTVIS evaluator (s2d_amd/ytvis_eval.py) against the reference's YTVOSeval on the committed fixture
(tests/golden/ytvis_eval.json, tests/golden/make_golden_ytvis.py): fed the reference's own IoU matrices, scores and areas,
the matching, accumulation and summary must reproduce evalImgs, precision, recall and stats.  No GPU needed."""
import base64
import copy
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLDEN, "ytvis_eval.json")) as fh:
        return json.load(fh)


def unpack(p):
    idx = np.frombuffer(base64.b64decode(p["index"]), np.uint16).astype(np.intp)
    return np.asarray(p["values"], np.float64)[idx].reshape(p["shape"])


def host_videos(fx):
    """per video: detections in result order with the reference's loadRes scores / categories / avg_area, and their IoU against
    every ground truth of the video in document order, permuted out of the reference's full (maxDets = inf) matrices"""
    res = fx["results"]
    gt_order = {}
    for a in fx["gt"]["annotations"]:
        gt_order.setdefault(a["video_id"], []).append(a["id"])
    videos = {}
    for v in fx["full_ious"]:
        if not v["dt_ids"]:
            continue
        m = np.asarray(v["ious"], np.float64).reshape(len(v["dt_ids"]), len(v["gt_ids"]))
        ids = sorted(v["dt_ids"])
        rows = [v["dt_ids"].index(i) for i in ids]
        cols = [v["gt_ids"].index(g) for g in gt_order.get(v["video_id"], [])]
        videos[v["video_id"]] = {"dt_ids": ids, "scores": [res[i - 1]["score"] for i in ids], "labels": [res[i - 1]["category_id"] for i in ids],
                                 "avg_areas": [fx["dt_avg_area"][str(i)] for i in ids], "ious": m[np.ix_(rows, cols)]}
    return videos


def check_against(ev, ref, check_ious=True):
    if check_ious:
        for e in ref["ious"]:
            got = ev.ious[e["video_id"], e["category_id"]]
            if not e["ious"]:
                assert len(got) == 0
            else:
                assert np.array_equal(np.asarray(got), np.asarray(e["ious"])), (e["video_id"], e["category_id"])
    assert len(ev.eval_vids) == len(ref["eval_vids"])
    for got, want in zip(ev.eval_vids, ref["eval_vids"]):
        if want is None:
            assert got is None
            continue
        assert got["video_id"] == want["video_id"] and got["category_id"] == want["category_id"] and list(got["aRng"]) == want["aRng"]
        assert got["dtIds"] == want["dtIds"] and got["gtIds"] == want["gtIds"] and got["dtScores"] == want["dtScores"]
        shp_d, shp_g = want["shapes"]
        for k, shp in (("dtMatches", shp_d), ("gtMatches", shp_g), ("dtIgnore", shp_d)):
            assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k], np.int64).reshape(shp)), (k, want["video_id"])
        assert np.array_equal(np.asarray(got["gtIgnore"]).astype(np.int64), np.asarray(want["gtIgnore"], np.int64))
    assert np.array_equal(ev.eval["precision"], unpack(ref["precision"]))
    assert np.array_equal(ev.eval["recall"], unpack(ref["recall"]))
    np.testing.assert_allclose(ev.stats, ref["stats"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("use_cats", [0, 1])
def test_host_stage_matches_reference(fx, use_cats, capsys):
    from s2d_amd.ytvis_eval import YTVISEval, derive_results
    ev = YTVISEval(fx["gt"], use_cats=use_cats).evaluate(host_videos(fx)).accumulate()
    ev.summarize()
    ref = fx[f"use_cats_{use_cats}"]
    check_against(ev, ref)
    assert capsys.readouterr().out.strip() == ref["summary"].strip()          # the reference's 12-line table
    d = derive_results(ev.stats)
    assert list(d) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100"]
    assert d["AP"] == pytest.approx(ref["stats"][0] * 100, abs=1e-10)


def test_settings_differ(fx):
    """the fixture exercises both groupings: pooled categories (YTVISEvaluator's setting) and per-category matching"""
    assert fx["use_cats_0"]["stats"] != fx["use_cats_1"]["stats"]


def test_no_results_and_unknown_video(fx):
    from s2d_amd.ytvis_eval import YTVISEval
    ev = YTVISEval(fx["gt"]).evaluate({}).accumulate()
    assert ev.summarize(out=None)[0] == 0.0                                  # ground truth, no detections: AP 0, not -1
    with pytest.raises(ValueError):
        YTVISEval(fx["gt"]).evaluate({999: {"dt_ids": [], "scores": [], "labels": [], "avg_areas": [], "ious": np.zeros((0, 0))}})


def test_polygon_ground_truth_is_refused(fx):
    from s2d_amd.ytvis_eval import GroundTruth, YTVISEvaluator, evaluate_ytvis
    doc = copy.deepcopy(fx["gt"])
    doc["annotations"][0]["segmentations"][1] = [[10.0, 10.0, 50.0, 10.0, 50.0, 40.0]]
    with pytest.raises(NotImplementedError, match="polygon"):
        GroundTruth(doc)
    with pytest.raises(NotImplementedError, match="polygon"):
        YTVISEvaluator(json_file=doc)
    with pytest.raises(NotImplementedError, match="polygon"):
        evaluate_ytvis(doc, [])


def test_mean_area_drops_none_and_zero():
    from s2d_amd.ytvis_eval import mean_area
    assert mean_area([None, 0, 4, 6]) == 5.0
    assert mean_area([None, 0]) == 0


def test_evaluator_needs_a_ground_truth_source():
    from s2d_amd.ytvis_eval import YTVISEvaluator
    with pytest.raises(ValueError):
        YTVISEvaluator()
