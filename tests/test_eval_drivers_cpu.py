"""CPU checks of the eval-only / pseudo-label drivers: the PIL-exact resize arithmetic on the library's own coefficient tables,
the ResizeShortestEdge sizes, config loading, checkpoint key conversions and the results -> annotations layout."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H0, W0) -> (H1, W1): 2x / 3x downscale (720p, 1080p -> 360p), non-integer ratios, odd sizes, portrait, upscale, identity,
# one side unchanged
RESIZE_GRID = [((72, 128), (36, 64)), ((108, 192), (36, 64)), ((720, 1280), (360, 640)), ((1080, 1920), (360, 640)),
               ((50, 77), (33, 51)), ((97, 61), (72, 47)), ((1280, 720), (640, 360)), ((30, 40), (45, 60)),
               ((41, 67), (41, 67)), ((41, 67), (41, 29)), ((41, 67), (23, 67)), ((480, 854), (360, 640))]


@pytest.mark.parametrize("src,dst", RESIZE_GRID)
def test_integer_resize_matches_pil(src, dst):
    from PIL import Image
    from s2d_amd.data.resize import resize_np
    rng = np.random.default_rng(src[0] * 7 + dst[1])
    img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    img[: src[0] // 3] = 255                                    # saturated and black regions exercise clip8
    img[-(src[0] // 4):, : src[1] // 2] = 0
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
    np.testing.assert_array_equal(resize_np(img, dst), want)


def test_coefficient_tables_are_monotone_and_plannable():
    from s2d_amd.data.resize import pil_coeffs, plan
    for (h0, w0), (h1, w1) in RESIZE_GRID:
        hb, hk = pil_coeffs(w0, w1)
        vb, _ = pil_coeffs(h0, h1)
        band, rows, span = plan(hb, hk, vb)
        assert band >= 1 and rows >= 1 and span >= 1
        assert (hk.sum(1) > (1 << 22) - hk.shape[1]).all() and (hk.sum(1) < (1 << 22) + hk.shape[1]).all()


def test_shortest_edge_sizes():
    from s2d_amd.data.augment import shortest_edge_shape
    assert shortest_edge_shape(720, 1280, 360, 1333) == (360, 640)
    assert shortest_edge_shape(1080, 1920, 360, 1333) == (360, 640)
    assert shortest_edge_shape(1280, 720, 360, 1333) == (640, 360)
    assert shortest_edge_shape(480, 854, 360, 1333) == (360, 641)
    assert shortest_edge_shape(100, 500, 360, 1333) == (267, 1333)      # MAX_SIZE_TEST caps the long side
    assert shortest_edge_shape(500, 100, 360, 1000) == (1000, 200)
    assert shortest_edge_shape(360, 360, 360, 1333) == (360, 360)


def test_load_config_base_chain_and_overrides(tmp_path):
    from s2d_amd.config import load_config
    (tmp_path / "sub").mkdir()
    (tmp_path / "a.yaml").write_text("MODEL:\n  PIXEL_STD: [1.0, 2.0, 3.0]\n  MASK_FORMER:\n    NHEADS: 4\n"
                                     "INPUT:\n  MIN_SIZE_TRAIN: (360, 480)\n  MIN_SIZE_TEST: 480\n")
    (tmp_path / "sub" / "b.yaml").write_text("_BASE_: ../a.yaml\nMODEL:\n  MASK_FORMER:\n    NHEADS: 6\n    DEC_LAYERS: 4\n")
    (tmp_path / "sub" / "c.yaml").write_text("_BASE_: b.yaml\nINPUT:\n  MIN_SIZE_TEST: 360\nEXTRA:\n  KEY: x\n")
    cfg = load_config(str(tmp_path / "sub" / "c.yaml"), ["MODEL.MASK_FORMER.DEC_LAYERS", "7", "INPUT.FORMAT", "RGB"])
    assert cfg.MODEL.MASK_FORMER.NHEADS == 6 and cfg.MODEL.MASK_FORMER.DEC_LAYERS == 7
    assert cfg.MODEL.PIXEL_STD == [1.0, 2.0, 3.0]
    assert cfg.INPUT.MIN_SIZE_TRAIN == (360, 480) and cfg.INPUT.MIN_SIZE_TEST == 360
    assert cfg.INPUT.MAX_SIZE_TEST == 1333 and cfg.INPUT.FORMAT == "RGB"            # defaults fill omitted keys
    assert cfg.MODEL.MASK_FORMER.TEST.EVAL_STUDENT is False
    assert cfg.EXTRA.KEY == "x"
    with pytest.raises(KeyError):
        load_config(str(tmp_path / "sub" / "c.yaml"), ["MODEL.MASK_FORMER.NO_SUCH_KEY", "1"])
    with pytest.raises(KeyError):
        load_config(str(tmp_path / "sub" / "c.yaml"), ["NOPE.X", "1"])


def test_shipped_config_loads_and_builds_the_kd_model():
    from s2d_amd.config import load_config
    from s2d_amd.modeling.meta_arch import META_ARCH_REGISTRY
    cfg = load_config(os.path.join(ROOT, "tests", "golden", "kd_config.json"), ["INPUT.MIN_SIZE_TEST", "64"])
    assert cfg.MODEL.META_ARCHITECTURE == "KDVideoMaskFormer" and cfg.INPUT.MIN_SIZE_TEST == 64
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg)
    assert model.num_queries == cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES and model.inference_rle is False


def test_checkpoint_key_conversions():
    from s2d_amd.checkpoint import convert_state_dict, kd_to_plain, plain_to_kd
    a, b, c = torch.zeros(2), torch.ones(3), torch.full((1,), 5.0)
    plain = {"backbone.res2.0.conv1.weight": a, "sem_seg_head.predictor.query_feat.weight": b, "criterion.empty_weight": c}
    kd = plain_to_kd(plain)
    assert set(kd) == {"student.0.res2.0.conv1.weight", "teacher.0.res2.0.conv1.weight",
                       "student.1.predictor.query_feat.weight", "teacher.1.predictor.query_feat.weight"}
    assert kd["teacher.0.res2.0.conv1.weight"] is a and kd["student.1.predictor.query_feat.weight"] is b
    kd2 = {"student.0.x": c, "teacher.0.x": a, "teacher.1.y.z": b, "criterion.empty_weight": c}
    assert kd_to_plain(kd2) == {"backbone.x": a, "sem_seg_head.y.z": b}
    # the direction follows the (checkpoint, model) pair; matching layouts pass through
    assert set(convert_state_dict(plain, ["student.0.w", "teacher.0.w"])) == set(kd)
    assert set(convert_state_dict(kd2, ["backbone.x", "sem_seg_head.y.z"])) == {"backbone.x", "sem_seg_head.y.z"}
    assert convert_state_dict(kd2, ["student.0.x"]) == kd2


def test_load_checkpoint_reports_and_skips_mismatches(tmp_path):
    from s2d_amd.checkpoint import load_checkpoint

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = torch.nn.Linear(3, 2)
            self.sem_seg_head = torch.nn.Linear(2, 4)

    src = {"model": {"teacher.0.weight": torch.full((2, 3), 2.0), "teacher.0.bias": torch.ones(5),
                     "teacher.1.weight": torch.full((4, 2), 3.0), "teacher.1.extra": torch.zeros(1),
                     "student.0.weight": torch.zeros(2, 3)}}
    p = tmp_path / "kd.pth"
    torch.save(src, p)
    net = Net()
    info = load_checkpoint(net, str(p))
    assert torch.equal(net.backbone.weight, torch.full((2, 3), 2.0)) and torch.equal(net.sem_seg_head.weight, torch.full((4, 2), 3.0))
    assert info["mismatched"] == [("backbone.bias", (5,), (2,))]
    assert set(info["missing"]) == {"backbone.bias", "sem_seg_head.bias"}
    assert info["unexpected"] == ["sem_seg_head.extra"]


def _rle_counts(m):
    flat = m.T.reshape(-1).astype(np.uint8)
    counts, cur, n = [], 0, 0
    for v in flat:
        if v != cur:
            counts.append(n); cur, n = v, 0
        n += 1
    counts.append(n)
    return counts


def _stub(segs, H, W):
    """bbox / area stand-in: deterministic values from the counts (the layout test does not need the device)"""
    return ([[float(len(s["counts"])), 0.0, 1.0, 2.0] if s else None for s in segs],
            [int(sum(s["counts"][1::2])) if s else None for s in segs])


def test_results_to_annotations_layout_threshold_and_ids(tmp_path):
    from s2d_amd.keymask.results_to_annotations import convert, convert_files
    m = np.zeros((4, 5), np.uint8); m[1:3, 2] = 1
    seg = {"size": [4, 5], "counts": _rle_counts(m)}
    gt = {"info": {"v": 1}, "licenses": [{"id": 1}], "categories": [{"id": 7, "name": "gt"}],
          "videos": [{"id": 1, "height": 4, "width": 5, "length": 2, "file_names": ["a/0.jpg", "a/1.jpg"]},
                     {"id": 2, "height": 4, "width": 5, "length": 1, "file_names": ["b/0.jpg"]}]}
    merged = {"categories": [{"id": 1, "name": "fg"}]}
    results = [{"video_id": 1, "score": 0.9, "category_id": 1, "segmentations": [seg, None]},
               {"video_id": 1, "score": 0.5, "category_id": 1, "segmentations": [seg, seg]},
               {"video_id": 2, "score": 0.75, "category_id": 1, "segmentations": [seg]},
               {"video_id": 9, "score": 0.99, "category_id": 1, "segmentations": [seg]}]
    doc, low = convert(merged, gt, results, 0.75, _stub)
    assert low == 1
    assert list(doc) == ["info", "licenses", "videos", "categories", "annotations"]
    assert doc["categories"] == merged["categories"] and doc["videos"] == gt["videos"] and doc["info"] == gt["info"]
    anns = doc["annotations"]
    assert [a["id"] for a in anns] == [1, 3]                       # skipped predictions still use up ids
    a0 = anns[0]
    assert a0 == {"video_id": 1, "iscrowd": 0, "height": 4, "width": 5, "length": 2, "segmentations": [seg, None],
                  "bboxes": [[float(len(seg["counts"])), 0.0, 1.0, 2.0], None], "areas": [2, None], "category_id": 1, "id": 1}
    bad = [{"video_id": 1, "score": 0.9, "category_id": 1, "segmentations": [seg]}]
    with pytest.raises(ValueError):
        convert(merged, gt, bad, 0.75, _stub)
    for name, d in (("m.json", merged), ("g.json", gt), ("r.json", results)):
        (tmp_path / name).write_text(json.dumps(d))
    out = convert_files(str(tmp_path / "m.json"), str(tmp_path / "g.json"), str(tmp_path / "r.json"), 0.75, str(tmp_path / "o"),
                        "pseudo", _stub)
    assert out == str(tmp_path / "o" / "pseudo.json") and json.load(open(out)) == json.loads(json.dumps(doc))
