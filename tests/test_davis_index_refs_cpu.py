"""CPU checks of the index-map references (tests/davis_index_refs.py: the reference alone, never the kernel) and of the host logic of the
DAVIS driver: the video document and its refusals, the test-format resolution, the flags, the palette, the PNG round trip and the
merge of per-rank results."""
import os

import numpy as np
import pytest

from tests import davis_index_refs as R


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.fixture(scope="module")
def values():
    cache = {}

    def get(case):
        if case["name"] not in cache:
            ml, dims, padded, img, out, query, score = R.make_inputs(case)
            planes = R.planes_of(ml, dims, query)
            cache[case["name"]] = (R.two_stage(planes, padded, img, out), R.two_stage(planes, padded, img, out, np.float32),
                                   R.mask_band(planes, dims, padded, out), score, planes)
        return cache[case["name"]]
    return get


@pytest.mark.parametrize("rule", ["rank", "prob"])
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_exclusion_cap_and_float32_restatement(case, rule, values):
    """on every GPU case's input: the excluded share is at most CAP, and the same rule evaluated in numpy float32 (float32 resize,
    np.exp on float32, float32 divide) agrees with float64 everywhere outside the exclusion -- the proof, from the reference alone,
    that band_v and the allowance c = 16 cover float32"""
    v64, v32, band, score, planes = values(case)
    assert v32.dtype == np.float32 and planes.dtype == np.float32
    assert 2.0 ** -24 < band < 1e-3 and float(np.abs(planes).max()) < 12                       # smooth fields of amplitude 3
    excl = R.excluded(v64, band, score, rule)
    assert excl.mean() <= R.CAP, f"{int(excl.sum())} of {excl.size} pixels excluded"
    r64, r32 = R.index_from_values(v64, score, rule), R.index_from_values(v32, score, rule, np.float32)
    assert not ((r64 != r32) & ~excl).any()
    assert float(np.abs(v64 - v32).max()) < band                                             # the sign band holds for numpy's float32
    if rule == "prob":
        assert not (excl & ~R.excluded_wide(v64, band, score)).any()                          # narrower than the first statement


def test_inputs_are_two_signed_and_the_rules_differ(values):
    flips = []
    for case in R.CASES:
        v64, _, _, score, planes = values(case)
        assert (planes > 0).mean() > 0.2 and (planes < 0).mean() > 0.2
        if case["K"] >= 3:
            flips.append(float((R.index_from_values(v64, score, "rank") != R.index_from_values(v64, score, "prob")).mean()))
    assert min(flips) > 0.02                                                                 # prob is no restatement of rank on these inputs


def test_repeated_queries_at_k254():
    for case in R.CASES:
        query = R.make_inputs(case)[5]
        assert len(query) == case["K"] and query.dtype == np.int32 and 0 <= query.min() and query.max() < case["Q"]
        assert (len(set(query.tolist())) < len(query)) == (case["K"] > case["Q"])
    assert not np.array_equal(R.make_inputs(R.CASES[0])[0], R.make_inputs(R.CASES[1])[0])


@pytest.mark.parametrize("name", R.NAMED)
def test_named_rows_have_the_property_they_are_named_for(name):
    ml, dims, padded, img, out, query, score, exp = R.named_inputs(name)
    planes = R.planes_of(ml, dims, query)
    v = R.two_stage(planes, padded, img, out)
    for rule in ("rank", "prob"):
        np.testing.assert_array_equal(R.index_from_values(v, score, rule), exp[rule])
        np.testing.assert_array_equal(R.index_from_values(R.two_stage(planes, padded, img, out, np.float32), score, rule, np.float32), exp[rule])
    if name == "all_negative":
        assert (planes < 0).all() and not exp["rank"].any()
    elif name == "nan":
        assert np.isnan(planes).all() and np.isnan(v).all() and not exp["prob"].any()
    elif name == "neg_zero":
        assert (planes == 0).all() and np.signbit(planes).all() and not exp["rank"].any()
    elif name == "nested":
        hold = v > 0
        assert hold[0].all() and (hold[1] <= hold[0]).all() and hold[1].any() and not hold[1].all()
        assert (exp["rank"] == 1).all() and ((exp["prob"] == 2) == hold[1]).all()             # the pair flips exactly inside
        assert all(float(s) == float(np.float32(s)) and (float(s) * 4).is_integer() for s in score)      # dyadic scores
    else:
        p = R.products(v, score)
        assert (p[0] == p[1]).all() and (p[2] < p[0]).all() and (exp["prob"] == 1).all()


def test_two_stage_matches_torch_interpolate():
    """the numpy resize is F.interpolate's: float64 to rounding, float32 bit for bit on the CPU"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 2, 5, 7)).astype(np.float32)
    for padded, img, out in ((20, 28), (18, 27), (37, 53)), ((20, 28), (18, 27), (18, 27)), ((20, 28), (18, 27), (9, 13)):
        for dt, tol in ((np.float64, 1e-13), (np.float32, 2e-6)):
            t = torch.from_numpy(x.astype(dt))
            ref = F.interpolate(t, size=padded, mode="bilinear", align_corners=False)[..., :img[0], :img[1]]
            if img != out:
                ref = F.interpolate(ref, size=out, mode="bilinear", align_corners=False)
            np.testing.assert_allclose(R.two_stage(x, padded, img, out, dt), ref.numpy(), rtol=0, atol=tol)


def test_select_proposals_restatement():
    s = [0.9, 0.7, 0.5, 0.3, 0.1]
    assert R.select_proposals(s, None, 20, 0.0) == [0, 1, 2, 3, 4]
    assert R.select_proposals(s, None, 2, 0.4) == [0, 1]
    assert R.select_proposals(s, [0, 2], 20, 0.4) == [0, 2]
    assert R.select_proposals(s, [0, 2, 3], 2, 0.2) == [0, 2]


# ------------------------------------------------------------------------------------------------------------------ document
def _tree(root, seqs=(("a", 3), ("b", 2)), size=(24, 32)):
    from PIL import Image
    from s2d_amd.davis_eval import save_index_png
    img_root, gt_dir = os.path.join(root, "JPEGImages"), os.path.join(root, "Annotations")
    for name, T in seqs:
        os.makedirs(os.path.join(img_root, name))
        os.makedirs(os.path.join(gt_dir, name))
        for t in range(T):
            Image.fromarray(np.zeros(size + (3,), np.uint8)).save(os.path.join(img_root, name, f"{t:05d}.jpg"))
            save_index_png(os.path.join(gt_dir, name, f"{t:05d}.png"), np.full(size, t % 3, np.uint8))
    return img_root, gt_dir


def test_davis_video_document(tmp_path):
    from s2d_amd.data.davis_loader import davis_video_document
    from s2d_amd.data.test_loader import load_videos
    img_root, gt_dir = _tree(str(tmp_path))
    doc = davis_video_document(img_root, gt_dir)
    assert [v["name"] for v in doc["videos"]] == ["a", "b"] and [v["id"] for v in doc["videos"]] == [1, 2]
    a = doc["videos"][0]
    assert (a["height"], a["width"], a["length"]) == (24, 32, 3)
    assert a["file_names"] == [os.path.join("a", f"{t:05d}.jpg") for t in range(3)] and a["gt_files"] == [f"{t:05d}.png" for t in range(3)]
    recs = load_videos(doc, img_root)                                                        # what YTVISTestLoader consumes
    assert recs[1]["video_id"] == 2 and all(os.path.isfile(f) for f in recs[1]["file_names"])
    assert os.path.basename(os.path.dirname(recs[1]["file_names"][0])) == doc["videos"][1]["name"] == "b"
    assert [v["name"] for v in davis_video_document(img_root, gt_dir, ["b"])["videos"]] == ["b"]
    lst = tmp_path / "seqs.txt"
    lst.write_text("b\n\na\n")
    assert [v["name"] for v in davis_video_document(img_root, gt_dir, str(lst))["videos"]] == ["b", "a"]
    with pytest.raises(FileNotFoundError, match="nope"):
        davis_video_document(img_root, gt_dir, ["nope"])


def test_davis_video_document_refusals(tmp_path):
    from PIL import Image
    from s2d_amd.data.davis_loader import davis_video_document
    img_root, gt_dir = _tree(str(tmp_path / "t1"))
    os.remove(os.path.join(gt_dir, "a", "00001.png"))
    with pytest.raises(FileNotFoundError, match="00001.png"):
        davis_video_document(img_root, gt_dir)
    img_root, gt_dir = _tree(str(tmp_path / "t2"))
    os.remove(os.path.join(img_root, "b", "00000.jpg"))
    with pytest.raises(FileNotFoundError, match="00000"):
        davis_video_document(img_root, gt_dir)
    img_root, gt_dir = _tree(str(tmp_path / "t3"))
    Image.fromarray(np.zeros((20, 32, 3), np.uint8)).save(os.path.join(img_root, "a", "00002.jpg"))
    with pytest.raises(ValueError, match="00002.jpg"):
        davis_video_document(img_root, gt_dir)
    img_root, gt_dir = _tree(str(tmp_path / "t4"))
    Image.fromarray(np.zeros((24, 32, 3), np.uint8)).save(os.path.join(gt_dir, "b", "00001.png"))
    with pytest.raises(ValueError, match="00001.png"):
        davis_video_document(img_root, gt_dir)


# ------------------------------------------------------------------------------------------------------------------ driver logic
def test_resolve_test_format_with_a_directory(tmp_path):
    from s2d_amd.evaluate import parse_args, resolve_test_format
    d = str(tmp_path)
    assert resolve_test_format("auto", d) == "davis" and resolve_test_format("davis", d) == "davis"
    with pytest.raises(ValueError, match="--boundary-ap"):
        resolve_test_format("auto", d, boundary=True)
    with pytest.raises(ValueError, match="--iou-types"):
        resolve_test_format("davis", d, iou_types=("segm",))
    with pytest.raises(ValueError, match="directory"):
        resolve_test_format("davis", {"videos": []})
    with pytest.raises(ValueError, match="directory"):
        resolve_test_format("ytvis", d)
    assert resolve_test_format("auto", {"videos": [], "annotations": []}) == "ytvis"          # documents resolve as before
    base = ["--config-file", "c.yaml", "--gt", d, "--image-root", "i", "--output-dir", "o"]
    a = parse_args(base)
    assert (a.test_format, a.index_rule, a.max_proposals, a.score_threshold, a.bound_th, a.sequences) == ("auto", "rank", 20, 0.0, 0.008, None)
    a = parse_args(base + ["--test-format", "davis", "--index-rule", "prob", "--max-proposals", "7", "--score-threshold", "0.25",
                           "--bound-th", "0.01", "--sequences", "s.txt"])
    assert (a.test_format, a.index_rule, a.max_proposals, a.score_threshold, a.bound_th, a.sequences) == ("davis", "prob", 7, 0.25, 0.01, "s.txt")
    for bad in (["--index-rule", "last"], ["--test-format", "davis2016"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


def test_index_map_options():
    from s2d_amd.modeling.postprocess import index_map_options
    assert index_map_options({}) == ("rank", 20, 0.0)
    assert index_map_options({"rule": "prob", "max_proposals": 254, "score_threshold": 0.5}) == ("prob", 254, 0.5)
    for bad in ({"rule": "last"}, {"max_proposals": 0}, {"max_proposals": 255}, {"threshold": 0.1}):
        with pytest.raises(ValueError):
            index_map_options(bad)


def test_palette_and_index_png_round_trip(tmp_path):
    from PIL import Image
    from s2d_amd import demo
    from s2d_amd.davis_eval import DAVIS_PALETTE, read_index_png, save_index_png
    assert len(DAVIS_PALETTE) == 768 and all(isinstance(v, int) and 0 <= v <= 255 for v in DAVIS_PALETTE)
    assert DAVIS_PALETTE[:39] == demo.PALETTE and len(demo.PALETTE) == 39

    def voc(i):
        c = [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                c[ch] |= ((i >> ch) & 1) << (7 - j)
            i >>= 3
        return c
    for i in range(13, 256):
        assert DAVIS_PALETTE[3 * i: 3 * i + 3] == voc(i)
    assert voc(13) == [192, 0, 128] and voc(20) == [0, 64, 128] and voc(255) == [224, 224, 192]
    assert len({tuple(DAVIS_PALETTE[3 * i: 3 * i + 3]) for i in range(256)}) == 256           # every label its own colour
    index = np.array([[0, 20, 254, 255], [255, 254, 20, 0], [1, 13, 12, 21]], np.uint8)
    path = str(tmp_path / "m.png")
    save_index_png(path, index)
    np.testing.assert_array_equal(read_index_png(path), index)
    with Image.open(path) as im:
        assert im.mode == "P" and im.getpalette() == DAVIS_PALETTE
    with pytest.raises(ValueError):
        save_index_png(path, index.astype(np.int32))


def test_merge_sequence_results():
    from s2d_amd.davis_eval import merge_sequence_results
    r = {n: {"J": np.full((1, 2), i / 4), "F": np.full((1, 2), i / 8)} for i, n in enumerate("abcd")}
    merged = merge_sequence_results([[("c", r["c"]), ("a", r["a"])], [("d", r["d"])], [("b", r["b"])]], list("abcd"))
    assert list(merged) == list("abcd") and all(merged[n] is r[n] for n in "abcd")
    assert list(merge_sequence_results([[("b", r["b"])], [("a", r["a"])]], ["b", "a"])) == ["b", "a"]
    with pytest.raises(ValueError, match="more than one"):
        merge_sequence_results([[("a", r["a"])], [("a", r["a"])]], ["a"])
    with pytest.raises(ValueError, match="no result"):
        merge_sequence_results([[("a", r["a"])]], ["a", "b"])
    with pytest.raises(ValueError, match="does not have"):
        merge_sequence_results([[("a", r["a"]), ("z", r["b"])]], ["a"])


def test_davis_evaluator_refuses_the_semi_supervised_task(tmp_path):
    from s2d_amd.davis_eval import DAVISEvaluator
    os.makedirs(tmp_path / "gt" / "a")
    with pytest.raises(ValueError, match="first-frame"):
        DAVISEvaluator(str(tmp_path / "gt"), None, task="semi-supervised")
    with pytest.raises(ValueError):
        DAVISEvaluator(str(tmp_path / "gt"), None, task="interactive")
    ev = DAVISEvaluator(str(tmp_path / "gt"), None)
    with pytest.raises(ValueError, match="index_u8"):
        ev.process([{"file_names": ["a/0.jpg"]}], {"pred_masks": [], "pred_scores": []})
