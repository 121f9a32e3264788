"""CPU checks of the stage-1 frame masks: the two statements of the paint rule agree, the named rows have the properties they are
named for (on the float64 restatement of the resize), the colour table, the driver's folder document and file names against
discover's own rules, the CLI defaults, the refusals of inference_video(paint=...) and the exported symbols."""
import ctypes
import os

import numpy as np
import pytest

from tests import frame_masks_refs as F


def _random_planes(rng, K, T, H, W):
    """planes with equal areas, empty planes and duplicates among them"""
    m = rng.random((K, T, H, W)) < rng.random((K, 1, 1, 1))
    if K > 2:
        m[1] = m[0]                                                   # a duplicate: equal areas in every frame
        m[2, 0] = False                                               # area 0 in one frame
    return m


@pytest.mark.parametrize("K,T,H,W", [(1, 1, 5, 7), (3, 2, 9, 11), (7, 3, 12, 10), (50, 2, 8, 9), (254, 1, 6, 6)])
def test_literal_equals_owner_on_random_planes(K, T, H, W):
    rng = np.random.default_rng(K * 100 + T)
    m = _random_planes(rng, K, T, H, W)
    colors = F.case_colors(K)
    rgb_l, idx_l = F.paint_literal(m, colors)
    rgb_o, idx_o = F.paint_owner(m, colors)
    np.testing.assert_array_equal(idx_l, idx_o)
    np.testing.assert_array_equal(rgb_l, rgb_o)
    assert ((idx_o == 0) == ~m.any(0)).all()
    assert (rgb_o[idx_o == 0] == 0).all()


@pytest.mark.parametrize("name", F.NAMED)
def test_named_rows_have_their_property(name):
    row = F.named_inputs(name)
    m = F.planes_float64(row)
    K = m.shape[0]
    colors = F.case_colors(K)
    rgb_l, idx_l = F.paint_literal(m, colors)
    rgb_o, idx_o = F.paint_owner(m, colors)
    np.testing.assert_array_equal(idx_l, idx_o)
    np.testing.assert_array_equal(rgb_l, rgb_o)
    F.check_named_property(name, m, rgb_o, idx_o, colors)


def test_stable_order_is_the_counting_rank():
    """position of k = #{j : a_j > a_k or (a_j = a_k and j < k)}, the rule the ranking kernel evaluates"""
    rng = np.random.default_rng(4)
    areas = rng.integers(0, 5, (17, 6))
    order = F.stable_order(areas)
    for t in range(areas.shape[1]):
        a = areas[:, t]
        rank = [int(((a > a[k]) | ((a == a[k]) & (np.arange(len(a)) < k))).sum()) for k in range(len(a))]
        assert [int(order[t][r]) for r in rank] == list(range(len(a)))


def test_case_geometries_cover_what_they_are_named_for():
    T, hm, wm, padded, img, out = F.GEOMETRIES["two_stage"]
    assert out[1] % 4 and out[0] % 16 and out[1] % 64 and -(-out[0] // 16) == 3 and -(-out[1] // 64) == 3 and img != out
    assert F.GEOMETRIES["same"][4] == F.GEOMETRIES["same"][5]
    assert {c["K"] for c in F.CASES} == {1, 3, 50, 254} and {c["ldq"] for c in F.CASES} == {8, 128}
    ml, dims, padded, img, out, query = F.make_inputs(F.CASES[-1])
    assert F.CASES[-1]["name"].startswith("direct") and len(query) == 254 and len(set(query.tolist())) == 100


def test_mask_colors_are_distinct_and_not_black():
    from s2d_amd.frame_paint import mask_colors
    c = mask_colors(254)
    assert c.dtype == np.uint8 and c.shape == (254, 3)
    assert len({tuple(x) for x in c.tolist()}) == 254 and (c.astype(int).sum(1) > 0).all()
    np.testing.assert_array_equal(mask_colors(50), c[:50])
    with pytest.raises(ValueError):
        mask_colors(255)


# ------------------------------------------------------------------------------------------------------------------ the driver
def _folders(root, spec, ext=".jpg"):
    from PIL import Image
    for name, stems in spec.items():
        os.makedirs(os.path.join(root, name))
        for s in stems:
            Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(os.path.join(root, name, s + ext))
    open(os.path.join(root, "notes.txt"), "w").close()                # not a directory: no video


def test_folder_document_order_clips_and_job_slices(tmp_path):
    from s2d_amd.keymask import frame_masks as D
    from s2d_amd.keymask.discover import make_paths, video_and_mask_dirs
    root, masks = str(tmp_path / "frames"), str(tmp_path / "masks")
    _folders(root, {"vb": ["10", "9", "100", "1"], "va": ["00002", "00000", "00001"], "vc": ["3", "4", "5", "6", "7"]})
    doc, clips, counts = D.folder_document(root, masks, frames_per_call=2)
    assert counts == {"videos": 3, "skipped": 0}
    per_video = {}
    for v in doc["videos"]:
        per_video.setdefault(v["name"], []).append(v)
        assert (v["height"], v["width"], v["length"]) == (6, 8, len(v["file_names"]))
        assert clips[v["id"]] == (os.path.join(masks, v["name"]), [os.path.splitext(os.path.basename(f))[0] + ".png" for f in v["file_names"]])
    assert list(per_video) == ["va", "vb", "vc"]                                           # sorted folders
    assert [v["file_names"] for v in per_video["vb"]] == [["vb/1.jpg", "vb/9.jpg"], ["vb/10.jpg", "vb/100.jpg"]]   # numeric stems
    assert [len(v["file_names"]) for v in per_video["vc"]] == [2, 2, 1]                     # the last clip is short
    assert [len(v["file_names"]) for v in per_video["va"]] == [2, 1]
    assert [v["id"] for v in doc["videos"]] == list(range(1, len(doc["videos"]) + 1))
    # the frame order IS make_paths' for the dataset rule, and the slices are video_and_mask_dirs'
    for name in ("va", "vb", "vc"):
        frames = [f for v in per_video[name] for f in v["file_names"]]
        assert [os.path.join(root, f) for f in frames] == make_paths(os.path.join(root, name), os.path.join(root, name))[0]
    for job, n in ((0, 2), (1, 2), (2, 2), (0, -1), (1, 1)):
        d, _, c = D.folder_document(root, masks, 1, job, n)
        want = [os.path.basename(p) for p in video_and_mask_dirs(root, masks, job, n)[0]]
        assert list(dict.fromkeys(v["name"] for v in d["videos"])) == want and c["videos"] == len(want)
    with pytest.raises(ValueError):
        D.folder_document(root, masks, 0)


def test_sa_v_rule_and_dataset_detection(tmp_path):
    from s2d_amd.keymask import frame_masks as D
    root = str(tmp_path / "sa-v" / "frames")
    _folders(root, {"v": ["f_10", "f_9", "f_2"]})
    assert D.dataset_rule(root) == "SA-V" and D.dataset_rule("/data/clips") == "DAVIS" and D.dataset_rule(root, "ovis") == "ovis"
    doc, _, _ = D.folder_document(root, str(tmp_path / "m"), 8)
    assert doc["videos"][0]["file_names"] == ["v/f_2.jpg", "v/f_9.jpg", "v/f_10.jpg"]


def test_mask_names_pair_with_make_paths_and_complete_folders_are_skipped(tmp_path):
    from s2d_amd.keymask import frame_masks as D
    from s2d_amd.keymask.discover import make_paths
    root, masks = str(tmp_path / "frames"), str(tmp_path / "masks")
    _folders(root, {"va": ["00010", "00009", "00100"], "vb": ["1", "2"]})
    doc, clips, _ = D.folder_document(root, masks, 2)
    for v in doc["videos"]:
        mdir, names = clips[v["id"]]
        os.makedirs(mdir, exist_ok=True)
        for n in names:
            D.write_frame_png(os.path.join(mdir, n), np.zeros((6, 8, 3), np.uint8))
    for name in ("va", "vb"):
        imgs, labels = make_paths(os.path.join(root, name), os.path.join(masks, name))
        assert len(imgs) == len(labels) > 0
        for i, l in zip(imgs, labels):                                                       # frame i <-> mask i
            assert os.path.splitext(os.path.basename(i))[0] == os.path.splitext(os.path.basename(l))[0] and l.endswith(".png")
    from PIL import Image
    with Image.open(os.path.join(masks, "va", "00009.png")) as im:
        assert im.mode == "RGB" and im.size == (8, 6)
    doc2, _, counts = D.folder_document(root, masks, 2)
    assert counts == {"videos": 2, "skipped": 2} and doc2["videos"] == []
    os.remove(os.path.join(masks, "va", "00100.png"))                                        # incomplete: the whole video again
    doc3, _, counts = D.folder_document(root, masks, 2)
    assert counts == {"videos": 2, "skipped": 1} and {v["name"] for v in doc3["videos"]} == {"va"}
    assert len(D.folder_document(root, masks, 2, overwrite=True)[0]["videos"]) == 3
    with pytest.raises(ValueError):
        D.write_frame_png(os.path.join(masks, "x.png"), np.zeros((6, 8), np.uint8))


def test_cli_defaults():
    from s2d_amd.keymask.frame_masks import parse_args
    a = parse_args(["--config-file", "c.yaml", "--video-base-path", "D", "--mask-base-path", "M"])
    assert (a.confidence_threshold, a.max_masks, a.frames_per_call) == (0.35, 50, 1)
    assert (a.job_id, a.videos_per_job, a.overwrite, a.threads, a.prefetch, a.weights, a.opts) == (0, -1, False, 8, 2, None, [])
    a = parse_args(["--config-file", "c.yaml", "--video-base-path", "D", "--mask-base-path", "M", "--frames-per-call", "3", "--overwrite",
                    "INPUT.MIN_SIZE_TEST", "64"])
    assert a.frames_per_call == 3 and a.overwrite and a.opts == ["INPUT.MIN_SIZE_TEST", "64"]


def test_inference_video_paint_refuses_the_other_outputs():
    """refused before any tensor is touched: a stub is enough"""
    from s2d_amd.modeling.postprocess import inference_video, paint_options
    stub = object()
    for kw in ({"rle": True}, {"device_masks": True}, {"index_map": {"rule": "rank"}}):
        with pytest.raises(ValueError, match="paint"):
            inference_video(stub, stub, (1, 2, 2), (8, 8), (8, 8), (8, 8), 5, paint={}, **kw)
    assert paint_options({})[:2] == (50, 0.35) and paint_options({})[2].shape == (50, 3)
    for bad in ({"max_masks": 0}, {"max_masks": 255}, {"colour": 1}, {"colors": np.zeros((3, 3), np.uint8)},
                {"colors": np.zeros((50, 3), np.int32)}):
        with pytest.raises(ValueError):
            paint_options(bad)


def test_paint_switch_is_refused_under_window_inference():
    from s2d_amd.modeling.meta_arch import _inference
    with pytest.raises(ValueError, match="inference_paint.*TEST.WINDOW_INFERENCE"):
        _inference(None, None, [{}], 5, False, 0.75, window=(8, 2), paint={})


def test_new_symbols_are_declared_and_exported():
    from s2d_amd._lib import parse_header
    from s2d_amd.build import build
    protos = parse_header()
    dll = ctypes.CDLL(build(verbose=False))
    for name in ("s2d_infer_frame_areas_i32", "s2d_infer_paint_u8", "s2d_infer_index_u8"):
        assert name in protos and hasattr(dll, name)
    assert len(protos["s2d_infer_frame_areas_i32"][0]) == 16 and len(protos["s2d_infer_paint_u8"][0]) == 18
    from s2d_amd import ops
    for name in ("infer_frame_areas", "infer_paint", "paint_frames", "mask_colors"):
        assert getattr(ops, name).__module__ == "s2d_amd.frame_paint"
