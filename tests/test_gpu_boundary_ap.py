"""GPU side of Boundary AP (csrc/mask_boundary.hip, s2d_amd/ytvis_eval.py): the boundary-band kernel against the published
routine in scipy (tests/boundary_refs.py), word for word with no element excluded, and the evaluator's boundary path against
integer references and a worked case.  The kernel's launch is one workgroup per tile with no cap or grid stride (it refuses
F x tiles >= 2^31), so there is no case past a cap."""
import json
import os

import numpy as np
import pytest
import torch

from tests import boundary_refs as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device_bits(masks, pad_ones=False):
    w = np.stack([R.pack_bits(m, pad_ones) for m in masks])
    return torch.from_numpy(w.view(np.int32)).to(DEV)


def band_words(masks, H, W, d, pad_ones=False):
    from s2d_amd.ytvis_eval import boundary_planes
    return boundary_planes(device_bits(masks, pad_ones), H, W, d).cpu().numpy().view(np.uint32)


def ref_words(masks, d):
    return np.stack([R.pack_bits(R.boundary_ref(m, d)) for m in masks])


_contents = {}


def contents(H, W):
    if (H, W) not in _contents:
        _contents[H, W] = R.contents(np.random.default_rng(H * 1000 + W), H, W)
    return _contents[H, W]


@pytest.mark.parametrize("d", R.RADII)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_kernel_matches_published_routine(name, d):
    H, W = R.SHAPES[name]
    c = contents(H, W)
    got = band_words(list(c.values()), H, W, d)
    want = ref_words(list(c.values()), d)
    for f, cn in enumerate(c):
        assert np.array_equal(got[f], want[f]), cn


@pytest.mark.parametrize("hw,d", list(R.CHAINED) + list(R.WIDE))
def test_kernel_chained_passes_and_word_tiles(hw, d):
    """radii past one pass (64 | 65, and three passes) on frames whose window fits; rows of more than 32 words"""
    from s2d_amd._lib import lib
    H, W = hw
    rng = np.random.default_rng(H + W + d)
    hole = np.ones((H, W), bool)
    hole[H // 2 + 3, W // 2 - 5] = False
    masks = [np.ones((H, W), bool), hole, R.discs(rng, H, W, n=2, salt=0, edge=True), R.discs(rng, H, W)]
    assert (lib().call("s2d_mask_boundary_workspace_words", len(masks), H, W, d) > 0) == (d > 64)
    got = band_words(masks, H, W, d, pad_ones=True)
    want = ref_words(masks, d)
    assert want[0].any() and not np.array_equal(want[0], R.pack_bits(masks[0]))       # an interior survives the erosion
    for f in range(len(masks)):
        assert np.array_equal(got[f], want[f]), f


def test_planes_and_padding():
    """five different planes in one call (the plane stride); the same call with every plane's padding bits set on input: the
    output padding is 0 and the areas are those of the bands"""
    from s2d_amd.ytvis_eval import boundary_planes, plane_areas
    H, W, d = 40, 45, 3
    assert (H * W) % 32 != 0
    rng = np.random.default_rng(5)
    masks = [R.discs(rng, H, W) for _ in range(5)]
    want = ref_words(masks, d)
    assert len({w.tobytes() for w in want}) == 5
    clean = boundary_planes(device_bits(masks), H, W, d)
    dirty = boundary_planes(device_bits(masks, pad_ones=True), H, W, d)
    for out in (clean, dirty):
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want)
        for f in range(5):
            assert not R.unpack_bits(got[f], H, W)[1].any()
        assert plane_areas(out).cpu().numpy().tolist() == [int(R.boundary_ref(m, d).sum()) for m in masks]


@pytest.mark.parametrize("hw,d", [((480, 854), 20), ((720, 1280), 29), ((1080, 1920), 44)])
def test_evaluator_frame_sizes(hw, d):
    """480 x 854: every row straddles words; 1080 x 1920: a plane larger than the LDS; discs touching the image edges"""
    from s2d_amd.ytvis_eval import boundary_dilation
    H, W = hw
    assert boundary_dilation(H, W) == d
    masks = [R.discs(np.random.default_rng(H + W), H, W, n=4, salt=0, edge=True), np.ones((H, W), bool)]
    got = band_words(masks, H, W, d, pad_ones=True)
    want = ref_words(masks, d)
    assert np.array_equal(got, want)


def test_second_call_is_bitwise_equal():
    H, W, d = 37, 100, 3
    masks = list(contents(H, W).values())
    assert np.array_equal(band_words(masks, H, W, d), band_words(masks, H, W, d))


def test_bad_arguments_are_refused_and_launch_nothing():
    from s2d_amd import ops
    from s2d_amd._lib import lib
    H, W = 9, 33
    bits = device_bits([np.ones((H, W), bool)])
    out = torch.full_like(bits, 0x5a5a5a5a)
    raw = lib()._raw_s2d_mask_boundary_bits_u32
    st = ops._stream()
    assert raw(bits.data_ptr(), 1, H, W, 0, None, 0, out.data_ptr(), st) == -1
    assert raw(bits.data_ptr(), 1, 0, W, 1, None, 0, out.data_ptr(), st) == -1
    assert raw(None, 1, H, W, 1, None, 0, out.data_ptr(), st) == -1
    assert raw(bits.data_ptr(), 1, H, W, 1, None, 0, None, st) == -1
    assert raw(bits.data_ptr(), 1, H, W, 1, None, 0, bits.data_ptr(), st) == -1                      # out aliases bits
    assert raw(bits.data_ptr(), 1, 150, 140, 65, None, 0, out.data_ptr(), st) == -1                  # needs a workspace
    assert lib().call("s2d_mask_boundary_workspace_words", 1, H, W, 0) == -1
    torch.cuda.synchronize()
    assert (out == 0x5a5a5a5a).all()


def _video():
    """3 detection and 2 ground-truth tracks x 4 frames at 40 x 45: detection 1 is an empty track, frame 2 of detection 0 and
    frame 0 of ground truth 1 are absent"""
    rng = np.random.default_rng(11)
    H, W, T = 40, 45, 4
    base = [R.discs(rng, H, W, n=2, salt=0) for _ in range(T)]
    dts = [[np.roll(b, 2, axis=1) for b in base], [np.zeros((H, W), bool)] * T, [R.discs(rng, H, W) for _ in range(T)]]
    gts = [list(base), [np.roll(b, 3, axis=0) for b in base]]
    dts[0][2] = None
    gts[1][0] = None
    return H, W, T, dts, gts


def _planes(tracks, H, W):
    return device_bits([m if m is not None else np.zeros((H, W), bool) for t in tracks for m in t])


def test_video_ious_with_boundary():
    from s2d_amd.ytvis_eval import video_ious
    H, W, T, dts, gts = _video()
    d = 2
    db, gb = _planes(dts, H, W), _planes(gts, H, W)
    ious0, areas0 = video_ious(db, 3, gb, 2, T)
    ious, areas, bious = video_ious(db, 3, gb, 2, T, boundary_d=d, size=(H, W))
    assert ious.tobytes() == ious0.tobytes() and np.array_equal(areas, areas0)
    want = np.zeros((3, 2))
    for i, dt in enumerate(dts):
        for j, gt in enumerate(gts):
            inter, union = R.video_boundary_iou_ref(dt, gt, d)
            want[i, j] = inter / union if union else 0.0
    assert bious.dtype == np.float64 and bious.tobytes() == want.tobytes()
    assert (want[1] == 0).all() and (want[0] > 0).all()                # the empty track; bands that do overlap


def _square_doc():
    from tests.test_gpu_ytvis_eval import compressed
    g, d = R.square_case()
    doc = {"videos": [{"id": 1, "height": 64, "width": 64, "length": 1}], "categories": [{"id": 1, "name": "a"}],
           "annotations": [{"id": 1, "video_id": 1, "category_id": 1, "iscrowd": 0, "segmentations": [compressed(g)], "areas": [int(g.sum())]}]}
    results = [{"video_id": 1, "score": 0.9, "category_id": 1, "segmentations": [compressed(d)]}]
    return doc, results, d


def test_worked_case_end_to_end():
    """mask IoU 1520 / 1680 -> AP 0.9, AP50 = AP75 = 1; boundary IoU 76 / 236 at d = 1 -> all 0 (tests/test_boundary_refs_cpu.py
    holds the arithmetic); from RLE through evaluate_ytvis, and from a device mask tensor through one `process` call"""
    from s2d_amd.ytvis_eval import YTVISEvaluator, boundary_dilation, evaluate_ytvis
    doc, results, det = _square_doc()
    ratio = 0.01
    assert boundary_dilation(64, 64, ratio) == 1
    seg = evaluate_ytvis(doc, results, iou_type="segm")
    assert seg.ious[1, -1].tobytes() == np.array([[1520 / 1680]]).tobytes()
    assert seg.summarize(out=None)[:3] == pytest.approx([0.9, 1.0, 1.0], abs=1e-12)
    bnd = evaluate_ytvis(doc, results, iou_type="boundary", dilation_ratio=ratio)
    assert bnd.ious[1, -1].tobytes() == np.array([[76 / 236]]).tobytes()
    assert list(bnd.summarize(out=None)[:3]) == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        evaluate_ytvis(doc, results, iou_type="bbox")

    ev = YTVISEvaluator(json_file=doc, boundary=True, dilation_ratio=ratio)
    ev.process([{"video_id": 1, "length": 1}], {"pred_scores": [0.9], "pred_labels": [1],
                                                "pred_masks": torch.from_numpy(det[None, None]).to(DEV)})
    res = ev.evaluate()
    assert list(res) == ["segm", "boundary"]
    assert [res["segm"][k] for k in ("AP", "AP50", "AP75")] == pytest.approx([90.0, 100.0, 100.0], abs=1e-9)
    assert [res["boundary"][k] for k in ("AP", "AP50", "AP75")] == [0.0, 0.0, 0.0]
    assert ev.ytvis_eval.ious[1, -1].tobytes() == seg.ious[1, -1].tobytes()
    assert ev.ytvis_eval_boundary.ious[1, -1].tobytes() == bnd.ious[1, -1].tobytes()


def test_cli_prints_the_boundary_table(tmp_path, capsys):
    from s2d_amd.ytvis_eval import main
    doc, results, _ = _square_doc()
    (tmp_path / "gt.json").write_text(json.dumps(doc))
    (tmp_path / "res.json").write_text(json.dumps(results))
    main(["--gt", str(tmp_path / "gt.json"), "--results", str(tmp_path / "res.json"), "--iou-type", "boundary", "--dilation-ratio", "0.01"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 12 and lines[0].endswith("= 0.000") and "Average Precision" in lines[0]


def test_defaults_compute_nothing_new(monkeypatch):
    """without the new arguments: the fixture's stats and IoU matrices as before (tests/test_gpu_ytvis_eval.py holds them at
    length), no boundary kernel call, and no boundary entry"""
    from s2d_amd._lib import lib
    from s2d_amd.ytvis_eval import YTVISEvaluator, evaluate_ytvis
    from tests.test_gpu_ytvis_eval import _feed
    from tests.test_ytvis_eval_cpu import check_against
    with open(os.path.join(GOLDEN, "ytvis_eval.json")) as fh:
        fx = json.load(fh)
    called = []
    real = lib().call
    monkeypatch.setattr(lib(), "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    ev = evaluate_ytvis(fx["gt"], fx["results"])
    ev.summarize(out=None)
    check_against(ev, fx["use_cats_0"])
    e2 = YTVISEvaluator(json_file=fx["gt"])
    _feed(e2, fx, "rle")
    res = e2.evaluate()
    assert set(res) == {"segm"} and not hasattr(e2, "ytvis_eval_boundary")
    check_against(e2.ytvis_eval, fx["use_cats_0"])
    assert "s2d_mask_cross_counts_u64" in called and not [n for n in called if "boundary" in n]
    evaluate_ytvis(fx["gt"], fx["results"], iou_type="boundary")
    assert "s2d_mask_boundary_bits_u32" in called                      # the spy does see the kernel when it is asked for


def test_eval_driver_writes_both_entries(tmp_path):
    """evaluate_model(boundary=True), what `python -m s2d_amd.evaluate --boundary-ap` runs: metrics.json holds the mask table and
    the boundary table, each equal to evaluate_ytvis on the results.json of the same run; the flags parse"""
    from s2d_amd.evaluate import evaluate_model, parse_args
    from s2d_amd.ytvis_eval import derive_results, evaluate_ytvis
    from tests.test_gpu_eval_drivers import _model, _write_dataset
    a = parse_args(["--config-file", "c", "--gt", "g", "--image-root", "r", "--output-dir", "o", "--boundary-ap", "--dilation-ratio", "0.05"])
    assert a.boundary_ap is True and a.dilation_ratio == 0.05
    b = parse_args(["--config-file", "c", "--gt", "g", "--image-root", "r", "--output-dir", "o"])
    assert b.boundary_ap is False and b.dilation_ratio == 0.02
    root = str(tmp_path / "ytvis")
    gt = _write_dataset(root)
    cfg, model = _model(0)
    out = tmp_path / "out"
    results, _ = evaluate_model(cfg, model, gt, root, str(out), torch.device(DEV), threads=4, prefetch=2, boundary=True, dilation_ratio=0.05)
    assert list(results) == ["segm", "boundary"]
    metrics = json.load(open(out / "metrics.json"))
    assert list(metrics) == ["segm", "boundary"]
    for kind in ("segm", "boundary"):
        ev = evaluate_ytvis(gt, str(out / "results.json"), iou_type=kind, dilation_ratio=0.05)
        ev.summarize(out=None)
        assert json.dumps(metrics[kind], sort_keys=True) == json.dumps(derive_results(ev.stats), sort_keys=True)    # nan compares as text
        assert json.dumps(results[kind], sort_keys=True) == json.dumps(metrics[kind], sort_keys=True)
