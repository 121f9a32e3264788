"""CPU checks of the video demo (s2d_amd/demo.py): the reference's flag contract, the input list and output path rules, the
colour table, save_masks against the reference's own PNGs (tests/golden/demo_masks.npz, make_golden_demo.py) and the numpy
raster rule the HIP kernels are held to."""
import os

import numpy as np
import pytest

from s2d_amd import demo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo_masks.npz")
CASES = ("overlap", "many", "border", "column", "row")


# ------------------------------------------------------------------------------------------------------------------- flags
def test_parser_defaults_and_required_weights():
    a = demo.get_parser().parse_args(["--weights", "w.pth", "--input", "d/v/*.jpg"])
    assert a.config_file == "configs/youtubevis_2019/video_maskformer2_R50_bs16_8ep.yaml"
    assert a.weights == "w.pth" and a.input == ["d/v/*.jpg"]
    assert a.output is None and a.video_input is None
    assert a.save_frames is False and a.save_masks is False
    assert a.confidence_threshold == 0.5 and a.opts == []
    with pytest.raises(SystemExit):
        demo.get_parser().parse_args(["--input", "x/y.jpg"])


def test_opts_take_the_rest_of_the_line():
    a = demo.get_parser().parse_args(["--weights", "w", "--input", "a/b/1.jpg", "a/b/2.jpg", "--confidence-threshold", "0.8",
                                      "--opts", "MODEL.WEIGHTS", "x.pth", "INPUT.MIN_SIZE_TEST", "64"])
    assert a.input == ["a/b/1.jpg", "a/b/2.jpg"] and a.confidence_threshold == 0.8
    assert a.opts == ["MODEL.WEIGHTS", "x.pth", "INPUT.MIN_SIZE_TEST", "64"]


@pytest.mark.parametrize("value,on", [("True", True), ("False", True), ("0", True), ("no", True), ("", False)])
def test_save_flags_are_truthy_strings(value, on):
    a = demo.get_parser().parse_args(["--weights", "w", "--input", "a/b/c.jpg", "--save-frames", value, "--save-masks", value])
    assert demo.flag_on(a.save_frames) is on and demo.flag_on(a.save_masks) is on
    assert demo.flag_on(demo.get_parser().parse_args(["--weights", "w"]).save_frames) is False


# ---------------------------------------------------------------------------------------------------- inputs and paths
def test_glob_is_sorted_and_a_list_keeps_its_order(tmp_path):
    vdir = tmp_path / "clip7"
    vdir.mkdir()
    for n in ("00010.jpg", "00002.jpg", "00001.jpg", "note.txt"):
        (vdir / n).write_bytes(b"")
    name, files = demo.expand_inputs([str(vdir / "*.jpg")])
    assert name == "clip7"
    assert [os.path.basename(f) for f in files] == ["00001.jpg", "00002.jpg", "00010.jpg"]
    given = [str(vdir / "00010.jpg"), str(vdir / "00001.jpg")]
    name, files = demo.expand_inputs(given)
    assert name == "clip7" and files == given
    with pytest.raises(AssertionError):
        demo.expand_inputs([str(tmp_path / "missing" / "*.jpg")])


def test_video_name_is_taken_from_the_raw_first_argument(tmp_path):
    assert demo.expand_inputs(["a/b/c/x.jpg", "q/r.jpg"])[0] == "c"
    assert demo.expand_inputs(["frames/*.png", "other/1.png"])[0] == "frames"
    assert demo.expand_inputs(["~/vid/a.jpg", "~/vid/b.jpg"])[0] == "vid"      # cut before expanduser
    with pytest.raises(IndexError):
        demo.expand_inputs(["x.jpg", "y.jpg"])


def test_mask_path_replaces_jpg_on_the_whole_path():
    assert demo.mask_path("out/v", "/data/v/00001.jpg") == "out/v/mask_00001.png"
    assert demo.mask_path("out/v", "/data/v/00001.png") == "out/v/mask_00001.png"
    assert demo.mask_path("out/v", "/data/v/00001.jpeg") == "out/v/mask_00001.jpeg"
    assert demo.mask_path("out.jpg/v", "/d/v/3.jpg") == "out.png/v/mask_3.png"
    assert demo.frame_path("out.jpg/v", "/d/v/3.jpg") == "out.jpg/v/3.jpg"


def test_video_input_is_refused_before_any_work(tmp_path):
    with pytest.raises(SystemExit) as e:
        demo.main(["--weights", str(tmp_path / "none.pth"), "--video-input", "clip.mp4", "--output", str(tmp_path / "o")])
    assert "video" in str(e.value.code)
    assert not (tmp_path / "o").exists()


# --------------------------------------------------------------------------------------------------------------- colours
def test_instance_colors_deterministic_and_distinct():
    c = demo.instance_colors(255)
    assert c.dtype == np.uint8 and c.shape == (255, 3)
    assert np.array_equal(c, demo.instance_colors(255))
    assert np.array_equal(c[:10], demo.instance_colors(10))
    assert len({tuple(v) for v in c[:64]}) == 64
    assert demo.instance_colors(0).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ save_masks vs reference
def test_palette_is_the_reference_constant():
    g = np.load(GOLDEN)
    assert demo.PALETTE == g["palette_constant"].tolist()


@pytest.mark.parametrize("case", CASES)
def test_save_masks_restatement_matches_reference_png(case, tmp_path):
    from PIL import Image
    g = np.load(GOLDEN)
    masks = g[case + "_masks"]
    idx = demo.index_map(list(masks))
    assert np.array_equal(idx, g[case + "_index"])
    p = tmp_path / "mask_0.png"
    demo.save_index_png(idx, str(p))
    with Image.open(p) as im:
        assert im.mode == str(g[case + "_mode"]) == "P"
        assert np.array_equal(np.asarray(im), g[case + "_index"])
        assert np.array_equal(np.asarray(im.getpalette(), np.uint8), g[case + "_palette"])


def test_index_map_without_instances_and_above_255():
    assert np.array_equal(demo.index_map([], (3, 5)), np.zeros((3, 5), np.uint8))
    with pytest.raises(ValueError):
        demo.index_map([np.zeros((2, 2), np.uint8)] * 256)


# ---------------------------------------------------------------------------------------------------- numpy raster rule
def _blend(c, p):
    return (c * 128 + p * 128 + 128) >> 8


def test_render_rounding_and_boundary_on_a_single_pixel_interior():
    fr = np.full((1, 5, 5, 3), 101, np.uint8)
    m = np.zeros((1, 1, 5, 5), np.uint8)
    m[0, 0, 1:4, 1:4] = 1
    col = np.array([[200, 7, 0]], np.uint8)
    ov, ix = demo.render_host(fr, m, col)
    assert ov[0, 2, 2].tolist() == [_blend(200, 101), _blend(7, 101), _blend(0, 101)] == [151, 54, 51]
    ring = m[0, 0].astype(bool).copy()
    ring[2, 2] = False
    assert (ov[0][ring] == [200, 7, 0]).all()
    assert (ov[0][m[0, 0] == 0] == 101).all()
    assert np.array_equal(ix[0], m[0, 0])
    # round half up: (c + p + 1) >> 1 where c + p is odd; a lone mask pixel is its own boundary (opaque)
    fr2 = np.full((1, 5, 5, 3), 2, np.uint8)
    m2 = np.zeros((1, 1, 5, 5), np.uint8)
    m2[0, 0, 1:4, 1:4] = 1
    ov2, _ = demo.render_host(fr2, m2, np.array([[3, 1, 255]], np.uint8))
    assert ov2[0, 2, 2].tolist() == [3, 2, 129]
    lone = np.zeros((1, 1, 5, 5), np.uint8)
    lone[0, 0, 2, 2] = 1
    ov3, _ = demo.render_host(fr2, lone, np.array([[3, 3, 3]], np.uint8))
    assert ov3[0, 2, 2].tolist() == [3, 3, 3]


def test_render_boundary_at_frame_edges():
    fr = np.zeros((1, 4, 6, 3), np.uint8)
    m = np.ones((1, 1, 4, 6), np.uint8)
    col = np.array([[255, 255, 255]], np.uint8)
    ov, ix = demo.render_host(fr, m, col)
    edge = np.zeros((4, 6), bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    assert (ov[0][edge] == 255).all()
    assert (ov[0][~edge] == _blend(255, 0)).all()
    assert (ix == 1).all()


def test_render_draw_order_by_area_and_stable_ties():
    H, W = 8, 8
    fr = np.full((2, H, W, 3), 40, np.uint8)
    m = np.zeros((3, 2, H, W), np.uint8)
    m[0, 0, 2:4, 2:4] = 1                 # frame 0: instance 0 small, instance 1 large -> 1 drawn first, 0 on top
    m[1, 0, 0:8, 0:8] = 1
    m[0, 1, 0:8, 0:8] = 1                 # frame 1: instance 0 large -> drawn first, 1 and 2 tie (equal areas) -> 1 then 2
    m[1, 1, 2:6, 2:6] = 1
    m[2, 1, 2:6, 2:6] = 1
    col = np.array([[250, 0, 0], [0, 250, 0], [0, 0, 250]], np.uint8)
    ov, ix = demo.render_host(fr, m, col)
    # frame 0, pixel (2,2): instance 1 blended (interior of 1), then instance 0's boundary paints it opaque red
    assert ov[0, 2, 2].tolist() == [250, 0, 0]
    assert ix[0, 2, 2] == 2 and ix[0, 0, 0] == 2
    # frame 1, pixel (3,3): 0 blends, 1 blends, 2 blends last (tie kept in instance order)
    p = np.array([40, 40, 40])
    for c in col:
        p = _blend(c.astype(np.int64), p)
    assert ov[1, 3, 3].tolist() == p.tolist()
    assert ov[1, 2, 2].tolist() == [0, 0, 250]                              # boundary of 2, painted last
    assert ix[1, 3, 3] == 3 and ix[1, 0, 0] == 1
    # the tie order is instance order, not reversed: swapping which instance is drawn last changes the pixel
    ov_sw, _ = demo.render_host(fr, m[[0, 2, 1]], col[[0, 2, 1]])
    assert ov_sw[1, 2, 2].tolist() == [0, 250, 0]


def test_render_without_instances_copies_and_zero_index():
    fr = np.random.default_rng(0).integers(0, 256, (2, 3, 5, 3), dtype=np.uint8)
    ov, ix = demo.render_host(fr, np.zeros((0, 2, 3, 5), np.uint8), np.zeros((0, 3), np.uint8))
    assert np.array_equal(ov, fr) and not ix.any()


def test_render_index_is_save_masks_loop():
    g = np.load(GOLDEN)
    m = g["many_masks"]
    fr = np.zeros((1,) + m.shape[1:] + (3,), np.uint8)
    _, ix = demo.render_host(fr, m[:, None], demo.instance_colors(len(m)))
    assert np.array_equal(ix[0], g["many_index"])
