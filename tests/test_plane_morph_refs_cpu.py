"""The references of tests/plane_morph_refs.py proven on the host (the scipy restatements against a brute-force double loop, the
properties of the rule, each named case for its property), the smoothing options of s2d_amd/clean_annotations.py, and
clean_document's host logic with the reference device side injected.  No GPU."""
import copy
import ctypes
import json

import numpy as np
import pytest

from tests import plane_components_refs as C
from tests import plane_morph_refs as R

RADII = (1, 2, 3, 8, 31, 33, 64)


# ---------------------------------------------------------------------------------------------------------------- scipy == brute force
@pytest.mark.parametrize("shape", R.SHAPES)
def test_scipy_restatement_equals_brute_force(shape):
    rng = np.random.default_rng(0)
    n = 0
    for H in range(1, 10):
        for W in range(1, 12):
            x = rng.random((H, W)) < rng.choice([0.2, 0.5, 0.85])
            for r in (1, 2, 3, 4):
                if r > 2 and (H * W) % 3:                                # every size at r <= 2, a third of them at 3 and 4
                    continue
                for op in R.OPS:
                    np.testing.assert_array_equal(R.morph(x, op, r, shape), R.brute(x, op, r, shape), err_msg=f"{op} {H}x{W} r={r}")
                    n += 1
    assert n > 700


def test_brute_force_equals_scipy_at_the_large_radii_of_the_gpu_rows():
    """the GPU rows at r >= 31 compare against R.brute; scipy with the whole element, and with the element cut to the plane, agree"""
    rng = np.random.default_rng(3)
    planes = [rng.random((5, 7)) < 0.5, R.blobs(33, 31, rng), rng.random((3, 200)) < 0.1, rng.random((20, 40)) < 0.97]
    for shape in R.SHAPES:
        for r in (31, 32, 33, 64):
            for x in planes:
                for op in ("erode", "dilate"):
                    whole = {"erode": R.erode, "dilate": R.dilate}[op](x, r, shape, fit=False)
                    np.testing.assert_array_equal(R.morph(x, op, r, shape), whole)
                    np.testing.assert_array_equal(R.brute(x, op, r, shape), whole)
                for op in ("open", "close"):
                    np.testing.assert_array_equal(R.brute(x, op, r, shape), R.morph(x, op, r, shape))


def test_structuring_elements():
    assert R.disk(1).sum() == 5 and R.disk(2).sum() == 13 and R.disk(3).sum() == 29 and R.square(2).sum() == 25
    for r in (1, 5, 64):
        d = R.disk(r)
        assert d.shape == (2 * r + 1,) * 2 and d[r, 0] and d[0, r] and not d[0, 0] and (d == d[::-1]).all() and (d == d.T).all()


# ---------------------------------------------------------------------------------------------------------------- the properties
@pytest.mark.parametrize("shape", R.SHAPES)
def test_properties_of_the_rule(shape):
    """every size, density and radius of the list: the scipy restatement up to r = 8, above it the offset loop the test above holds
    equal to scipy there (scipy needs seconds per plane once the element is larger than the plane)"""
    rng = np.random.default_rng(1)
    sizes = [(1, 1), (1, 9), (2, 5), (7, 7), (13, 40), (40, 13), (3, 200)]
    for r in RADII:
        f = (lambda x, op: R.morph(x, op, r, shape)) if r <= 8 else (lambda x, op: R.brute(x, op, r, shape))
        for H, W in sizes:
            for density in (0.0, 0.1, 0.5, 0.9, 1.0):
                x = rng.random((H, W)) < density
                o, c = f(x, "open"), f(x, "close")
                assert not (o & ~x).any() and not (x & ~c).any()                         # open(X) <= X <= close(X)
                np.testing.assert_array_equal(c, ~f(~x, "open"))                         # duality, complements inside the image
                np.testing.assert_array_equal(f(x, "erode"), ~f(~x, "dilate"))
                np.testing.assert_array_equal(f(o, "open"), o)                           # idempotent
                np.testing.assert_array_equal(f(c, "close"), c)
            full, empty = np.ones((H, W), bool), np.zeros((H, W), bool)
            for op in R.OPS:
                assert f(full, op).all() and not f(empty, op).any()


def test_scipy_opening_and_closing_are_not_the_rule():
    full = np.ones((20, 20), bool)
    from scipy import ndimage
    assert ndimage.binary_closing(full, R.disk(2)).sum() == 256 and R.close(full, 2).sum() == 400


# ---------------------------------------------------------------------------------------------------------------- named cases
def test_whisker_goes_under_open_and_its_object_stays():
    m, obj = R.whisker(), R.whisker_object()
    from scipy import ndimage
    assert ndimage.label(m)[1] == 1 and (m & ~obj).sum() == 40
    assert C.ref_clean(m, min_area=30)[1] == 0                           # one component: the component rule keeps the whisker
    np.testing.assert_array_equal(R.open_(m, 1, "square"), obj)
    o = R.open_(m, 2, "disk")
    # the disk leaves the one pixel of the whisker's root that it reaches from inside the object
    assert (o & ~obj).sum() == 1 and o[10, 16] and o[8:14, 6:14].all() and C.tight_box(o)[2] == 13 and C.tight_box(m)[2] == 52


def test_crack_closes_under_close_and_two_components_become_one():
    from scipy import ndimage
    m = R.crack()
    assert ndimage.label(m)[1] == 2 and (ndimage.binary_fill_holes(m) == m).all()      # neither side is a hole
    for shape in R.SHAPES:
        c = R.close(m, 1, shape)
        # the square makes the rectangle whole; the disk (a cross at r = 1) leaves the two pixels at either end of the crack
        assert ndimage.label(c)[1] == 1 and c[6:16, 6:28].all() and c.sum() == 12 * 22 - (4 if shape == "disk" else 0)


def test_edge_rectangle_keeps_its_edge_corners_and_the_edge_strip_goes():
    from scipy import ndimage
    for H, W in ((20, 30), (37, 45)):
        for edge in R.EDGES:
            m = R.edge_rect(H, W, edge)
            o = R.open_(m, 2)
            assert m.sum() == 60 and o.sum() == 54                       # only the two inner corners lose 3 pixels each
            assert ndimage.binary_opening(m, R.disk(2)).sum() == 48      # a zero border rounds the edge corners too
            np.testing.assert_array_equal(R.open_(m, 2, "square"), m)
            s = R.edge_strip(H, W, edge)
            for shape in R.SHAPES:
                assert not R.open_(s, 1, shape).any()


# ---------------------------------------------------------------------------------------------------------------- options
def _parse(argv):
    from s2d_amd import clean_annotations as A
    return A.cleanup_options(A.build_parser().parse_args(["--ann", "a", "--save-path", "b"] + argv))


def test_option_parsing(capsys):
    from s2d_amd import clean_annotations as A
    off = _parse([])
    assert off == {"min_component_area": 0, "keep_largest": False, "fill_holes": 0, "component_connectivity": 8} and not A.cleanup_is_on(off)
    assert _parse(["--open", "0", "--close", "0%", "--smooth-shape", "square"]) == off
    on = _parse(["--open", "2", "--close", "1%"])
    assert on == dict(off, open_radius=2, close_radius="1%", smooth_shape="disk") and A.cleanup_is_on(on)
    assert _parse(["--close", "3", "--smooth-shape", "square"]) == dict(off, open_radius=0, close_radius=3, smooth_shape="square")
    assert A.cleanup_is_on({"open_radius": "0.5%"}) and not A.cleanup_is_on({"open_radius": 0, "close_radius": "0%"})
    for bad in (["--open", "-1"], ["--open", "two"], ["--close", "1.5"], ["--close", "-2%"], ["--open", "%"], ["--smooth-shape", "cross"],
                ["--close", "nan%"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for bad in ({"open_radius": -1}, {"close_radius": 1.5}, {"open_radius": True}, {"smooth_shape": "cross"}, {"close_radius": "x%"}):
        with pytest.raises(ValueError):
            A.clean_document({"images": [], "annotations": []}, **bad)
    # the three drivers that write an annotation file carry the same options
    from s2d_amd import selftrain, selftrain_video
    from s2d_amd.keymask import results_to_annotations
    for mod in (A, selftrain, selftrain_video, results_to_annotations):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            mod.main(["--help"])
        text = capsys.readouterr().out
        assert "--open R" in text and "--close R" in text and "--smooth-shape {disk,square}" in text


def test_smooth_radius():
    from s2d_amd.plane_morph import smooth_radius
    from s2d_amd.ytvis_eval import boundary_dilation
    assert smooth_radius(3, 10, 10) == 3 and smooth_radius("3", 480, 640) == 3 and smooth_radius(0, 5, 5) == 0 and smooth_radius("0%", 5, 5) == 0
    assert smooth_radius("1%", 480, 640) == 8 == boundary_dilation(480, 640, 0.01) == R.ref_radius("1%", 480, 640)
    assert smooth_radius("1%", 720, 1280) == 15 and smooth_radius("1%", 30, 40) == 1 and smooth_radius("0.1%", 30, 40) == 1
    for H, W in ((33, 200), (120, 97), (5, 7), (1080, 1920)):
        for spec in ("1%", "2%", "0.5%"):
            assert smooth_radius(spec, H, W) == R.ref_radius(spec, H, W)
    assert smooth_radius(64, 10, 10) == 64
    with pytest.raises(ValueError, match="video 7"):
        smooth_radius("5%", 1080, 1920, "video 7")
    with pytest.raises(ValueError, match="65"):
        smooth_radius(65, 10, 10)


# ---------------------------------------------------------------------------------------------------------------- the host logic
OPTS = dict(open_radius=2, close_radius="1%", min_component_area=4, fill_holes=6)


@pytest.mark.parametrize("make", (R.make_coco_doc, R.make_ytvis_doc))
def test_clean_document_host_logic_equals_the_reference(make):
    from s2d_amd import clean_annotations as A
    doc, _ = make()
    before = copy.deepcopy(doc)
    seen = []

    def fn(chunk, opts):
        seen.append(opts)
        return R.ref_device_fn()(chunk, opts)

    want, want_stats = R.ref_clean_document(doc, area_rule="bbox", **OPTS)
    got, stats = A.clean_document(doc, area_rule="bbox", device_fn=fn, **OPTS)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats and doc == before
    assert seen and all(o == (4, False, 8, 6, 2, "1%", "disk") for o in seen)
    assert list(stats) == list(A.STAT_KEYS) + list(A.SMOOTH_STAT_KEYS)
    assert stats["pixels_opened"] > 0 and stats["pixels_closed"] > 0 and stats["planes_changed"] > 0
    # smoothing off: today's tuple, today's stats, today's document
    seen.clear()
    off = dict(min_component_area=4, fill_holes=6)
    got, stats = A.clean_document(doc, device_fn=fn, **off)
    want, want_stats = C.ref_clean_document(doc, **off)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats and list(stats) == list(A.STAT_KEYS)
    assert all(o == (4, False, 8, 6) for o in seen)
    assert R.ref_clean_document(doc, **off) == (want, want_stats)


def test_a_mask_changed_by_smoothing_alone_is_re_encoded_with_a_tight_box():
    from s2d_amd import clean_annotations as A
    m, obj = R.whisker(), R.whisker_object()
    H, W = m.shape
    keep = {"id": 2, "image_id": 1, "category_id": 1, "iscrowd": 0, "segmentation": C.uncompressed(obj), "bbox": [0.0, 0.0, 1.0, 1.0], "area": 7}
    doc = {"images": [{"id": 1, "height": H, "width": W}], "categories": [{"id": 1, "name": "fg"}],
           "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "iscrowd": 0, "segmentation": C.encode_mask(m),
                            "bbox": [float(v) for v in C.tight_box(m)], "area": int(m.sum())}, keep]}
    got, stats = A.clean_document(doc, open_radius=1, smooth_shape="square", device_fn=R.ref_device_fn())
    a = got["annotations"][0]
    assert a["segmentation"] == C.encode_mask(obj) and a["bbox"] == [4.0, 6.0, 12.0, 10.0] and a["area"] == 120
    assert got["annotations"][1] is keep                                  # unchanged: the same object, box and area untouched
    assert stats == {"planes": 2, "planes_changed": 1, "pixels_removed": 0, "pixels_filled": 0, "annotations_dropped": 0,
                     "frames_emptied": 0, "pixels_opened": 40, "pixels_closed": 0}
    assert doc["annotations"][0]["bbox"][2] == 52.0
    # a device side that leaves the smoothing counts out, or a selection that ignores them, is refused
    def bad(chunk, opts):
        r = R.ref_device_fn()(chunk, opts)
        del r.opened
        return r
    with pytest.raises((ValueError, AttributeError)):
        A.clean_document(doc, open_radius=1, device_fn=bad)


def test_radius_over_64_names_the_image():
    from s2d_amd import clean_annotations as A
    doc, _ = R.make_coco_doc()
    doc["images"][2]["height"], doc["images"][2]["width"] = 3000, 4000
    chunk_names = []

    def fn(chunk, opts):
        from s2d_amd.plane_morph import smooth_radius
        for (H, W), name in zip(chunk.sizes, chunk.names):
            chunk_names.append(name)
            smooth_radius(opts[4], H, W, name)
        raise AssertionError("not reached")
    with pytest.raises(ValueError, match=r"12 \(annotation"):
        A.clean_document(doc, open_radius="2%", device_fn=fn)


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_and_exported():
    from s2d_amd._lib import parse_header
    from s2d_amd.build import build
    protos = parse_header()
    dll = ctypes.CDLL(build(verbose=False))
    for name in ("s2d_plane_morph_tile", "s2d_plane_morph_lds_words", "s2d_plane_morph_workspace_bytes", "s2d_plane_morph_ragged",
                 "s2d_plane_diff_counts_ragged"):
        assert name in protos and hasattr(dll, name)
    assert len(protos["s2d_plane_morph_ragged"][0]) == 15 and len(protos["s2d_plane_morph_tile"][0]) == 3
    assert protos["s2d_plane_morph_workspace_bytes"][1] == "long"
    # the three host-only entry points run without a device
    tile, need = dll.s2d_plane_morph_tile, dll.s2d_plane_morph_lds_words
    need.restype, need.argtypes = ctypes.c_long, [ctypes.c_int] * 3
    rows, words = ctypes.c_int(0), ctypes.c_int(0)
    got = []
    for r in range(65):
        assert tile(r, ctypes.byref(rows), ctypes.byref(words)) == 0
        got.append(rows.value)
        # the run table (36 words), the rows with their 2r halo rows and two halo words either side, V and the accumulators: at most
        # 10240 words = 40 KiB, so that four workgroups share the 160 KiB of a CU, and one row more would not fit
        full = 36 + (rows.value + 2 * r) * 36 + rows.value * 36 + rows.value * 32
        assert words.value == 32 and full <= 10240 < full + 104
        if r:
            assert need(r, rows.value, 1024) == need(r, 4 * rows.value, 5000) == full       # the largest tile is the full one
            assert need(r, rows.value + 1, 1024) < full                                     # cut evenly: two tiles of half the rows
            assert need(r, 1, 1) == 36 + (1 + 2 * r) * 5 + 5 + 1 and need(r, 40, 40) == 36 + (40 + 2 * r) * 6 + 40 * 6 + 40 * 2
    assert got == sorted(got, reverse=True) and got[0] == 98 and got[64] == 53
    assert need(0, 10, 10) == 0 and need(65, 10, 10) == -1 and need(1, 0, 10) == -1 and need(1, 10, 0) == -1
    assert tile(65, ctypes.byref(rows), ctypes.byref(words)) == -1 and tile(-1, ctypes.byref(rows), ctypes.byref(words)) == -1
    assert tile(1, None, ctypes.byref(words)) == -1
    # the figure of a launch is the largest per-plane need, whatever the mix of sizes and radii
    from s2d_amd import plane_morph
    rng = np.random.default_rng(0)
    table = np.stack([np.zeros(300, int), rng.integers(1, 800, 300), rng.integers(1, 1400, 300), np.zeros(300, int)], 1).astype(np.int64)
    radii = rng.integers(0, 65, 300)
    assert plane_morph.morph_lds_words(table, radii) == max(need(int(r), int(H), int(W)) for r, (_, H, W, _) in zip(radii, table))
    assert plane_morph.morph_lds_words(table, np.zeros(300, int)) == 0
    assert plane_morph.morph_lds_words(table[:1], [2]) == need(2, int(table[0, 1]), int(table[0, 2])) < 10240
    ws = dll.s2d_plane_morph_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_long, [ctypes.c_long, ctypes.c_int]
    assert ws(1000, 3) >= 4000 and ws(-1, 0) == -1 and ws(1 << 33, 1) >= 4 << 33
    from s2d_amd import ops
    for name in ("morph_planes", "morph_tile", "smooth_radius"):
        assert getattr(ops, name).__module__ == "s2d_amd.plane_morph"
