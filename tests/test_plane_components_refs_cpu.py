"""The references of tests/plane_components_refs.py proven without a device -- against a brute-force flood fill, and each named case
for the property it is named for --, and the host side of s2d_amd/clean_annotations.py with the device side injected from them."""
import copy
import ctypes
import json

import numpy as np
import pytest

from tests import plane_components_refs as R

TH, TW = 32, 64          # stand-ins for the kernel's tile: the properties below hold for any tile of at least 8 x 8


def test_labels_and_holes_match_a_flood_fill():
    rng = np.random.default_rng(0)
    for it in range(150):
        H, W = rng.integers(1, 13, 2)
        m = rng.random((H, W)) < rng.random()
        for conn in (4, 8):
            for value in (0, 1):
                a, b = R.ref_labels(m, value, conn), R.flood_labels(m, value, conn)
                np.testing.assert_array_equal(a[0], b[0])
                np.testing.assert_array_equal(a[1], b[1])
            holes = R.flood_holes(m, conn)
            np.testing.assert_array_equal(R.ref_fill(m, R.FILL_ALL, conn), m | holes)
            # the size limit: exactly the holes of at most n pixels, by the flood fill's areas
            labels, area = R.flood_labels(m, 0, 4 if conn == 8 else 8)
            size = np.zeros(H * W + 1, np.int64)
            size[np.flatnonzero(area.reshape(-1)) + 1] = area.reshape(-1)[area.reshape(-1) > 0]
            for n in (1, 2, 5):
                np.testing.assert_array_equal(R.ref_fill(m, n, conn), m | (holes & (size[labels] <= n)))


def test_filter_rule_on_a_hand_made_plane():
    m = R.tie_plane(TH, TW)
    for conn in (4, 8):
        labels, area = R.ref_labels(m, 1, conn)
        assert sorted(area[area > 0].tolist()) == [1, 4, 9, 9]           # "these two components have equal area"
        firsts = np.flatnonzero(area.reshape(-1) == 9)
        assert firsts[0] == 2 * m.shape[1] + 2 and firsts[1] == (TH - 1) * m.shape[1] + TW - 1
        kept = R.ref_filter(m, 0, True, conn)
        assert kept.sum() == 9 and kept[2:5, 2:5].all()                  # the lower first pixel wins the tie
        assert R.ref_filter(m, 9, False, conn).sum() == 18 and R.ref_filter(m, 10, False, conn).sum() == 0
        assert R.ref_filter(m, 10, True, conn).sum() == 0 and R.ref_filter(m, 9, True, conn).sum() == 9
    # the second nine crosses the corner of four tiles
    ys, xs = np.nonzero(R.ref_labels(m, 1, 8)[0] == (TH - 1) * m.shape[1] + TW)
    assert {(y // TH, x // TW) for y, x in zip(ys, xs)} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_named_cases_have_their_properties():
    cases = R.hole_cases(TH, TW)
    ring = cases["ring"]
    hole = R.flood_holes(ring, 8)
    assert hole.sum() == (TH + 2) * (TW + 2)
    ys, xs = np.nonzero(hole)
    assert len({(y // TH, x // TW) for y, x in zip(ys, xs)}) >= 4        # the hole crosses tile borders
    nested = cases["nested"]
    filled = R.ref_fill(nested, R.FILL_ALL, 8)
    assert R.ref_labels(nested, 1, 8)[1].astype(bool).sum() == 2         # two rings,
    assert filled[1:-1, 1:-1].all() and not filled[0].any()              # everything inside the outer one is filled, as scipy does
    for conn in (4, 8):
        assert not R.flood_holes(cases["open"], conn).any()              # "this hole is open to the border"
    assert not cases["open"][0, 8] and cases["open"][0, 7] and cases["open"][0, 9]
    dg = cases["diagonal"]
    assert not dg[4, 4] and dg[4, 5] and dg[5, 4] and not dg[5, 5]       # "this hole touches the outside only diagonally"
    assert R.flood_holes(dg, 8).sum() == 49 and R.flood_holes(dg, 4).sum() == 0
    isl = cases["island"]
    assert sorted(R.ref_labels(isl, 1, 8)[1][R.ref_labels(isl, 1, 8)[1] > 0].tolist())[0] == 2
    inner = R.flood_holes(R.ref_filter(isl, 3, False, 8), 8)
    assert inner[10, 10:12].all()                                        # filter first: the island's pixels are part of the hole
    assert not R.ref_fill(isl, R.FILL_ALL, 8)[9, 10] or R.ref_fill(isl, R.FILL_ALL, 8)[10, 10]
    out, removed, filled = R.ref_clean(isl, 3, False, R.FILL_ALL, 8)
    assert removed == 2 and filled == (TH + 2) * (TW + 2)
    # row wrap: flat neighbours that are no neighbours
    for W in (33, 64):
        m = R.row_wrap(TH + 3, W)
        assert (R.ref_labels(m, 1, 4)[1] > 0).sum() == m.sum() == TH + 3
        flat = m.reshape(-1)
        assert (flat[:-1] & flat[1:]).sum() == (TH + 3) // 2             # (y, W-1) and (y+1, 0) ARE adjacent in the flat plane
    assert (R.ref_labels(R.row_wrap(TH + 3, 1), 1, 4)[1] > 0).sum() == 1
    # merge cases
    mc = R.merge_cases(TH, TW)
    for conn in (4, 8):
        assert (R.ref_labels(mc["spiral"], 1, conn)[1] > 0).sum() == 1 and (R.ref_labels(mc["comb"], 1, conn)[1] > 0).sum() == 1
    assert (R.ref_labels(mc["checker"], 1, 4)[1] > 0).sum() == mc["checker"].sum()
    for name in ("corner", "corner_anti"):
        ys, xs = np.nonzero(mc[name])
        assert len(ys) == 2 and abs(ys[0] - ys[1]) == 1 and abs(xs[0] - xs[1]) == 1
        assert {(y // TH, x // TW) for y, x in zip(ys, xs)} in ({(0, 0), (1, 1)}, {(0, 1), (1, 0)})
    assert mc["spiral"].shape[0] > 2 * TH and mc["spiral"].shape[1] > 2 * TW     # 3 x 3 tiles and a remainder


def test_pack_sets_padding_and_sizes_cover_the_list():
    planes = R.size_chunk(TH, TW)
    bits, plane = R.pack_planes(planes, set_padding=True, gap_words=2)
    padded = 0
    for m, row in zip(planes, plane):
        got, pad = R.unpack_plane(bits, row, with_padding=True)
        np.testing.assert_array_equal(got, m)
        assert pad.all()                                                 # "this plane's padding bits are set"
        padded += len(pad) > 0
    assert padded > 10
    clean, _ = R.pack_planes(planes)
    assert all(not R.unpack_plane(clean, r, True)[1].any() for r in R.pack_planes(planes)[1])
    sizes = R.size_cases(TH, TW)
    assert {w for _, w in sizes} >= {1, 2, 31, 32, 33, 63, 64, 65, TW - 1, TW, TW + 1, 2 * TW + 5}
    assert {h for h, _ in sizes} >= {1, 2, TH - 1, TH, TH + 1, 2 * TH + 5}
    assert any(m.shape == (1, 1) for m in planes) and any(m.all() and m.size > 1 for m in planes) and any(not m.any() for m in planes)


def test_numpy_rle_round_trip_and_known_strings():
    rng = np.random.default_rng(1)
    for it in range(100):
        H, W = rng.integers(1, 40, 2)
        m = rng.random((H, W)) < rng.random()
        counts = R.rle_counts(m)
        assert counts.sum() == H * W and (counts[1:] > 0).all()
        s = R.rle_to_string(counts)
        np.testing.assert_array_equal(R.rle_from_string(s), counts)
        np.testing.assert_array_equal(R.rle_decode(R.rle_from_string(s), H, W), m)
        np.testing.assert_array_equal(R.decode_segmentation(R.uncompressed(m), H, W), m)
    assert R.rle_counts(np.zeros((3, 4), bool)).tolist() == [12] and R.rle_counts(np.ones((3, 4), bool)).tolist() == [0, 12]
    assert R.rle_to_string([12]) == b"<" and R.rle_to_string([0, 12]) == b"0<"
    big = np.zeros((480, 854), bool)
    big[100:300, 200:500] = True
    np.testing.assert_array_equal(R.decode_segmentation(R.encode_mask(big), 480, 854), big)
    assert R.tight_box(big) == [200, 100, 300, 200] and R.tight_box(np.zeros((2, 2), bool)) == [0, 0, 0, 0]


def test_cli_parsing():
    from s2d_amd import clean_annotations as C
    a = C.build_parser().parse_args(["--ann", "a.json", "--save-path", "b.json"])
    assert C.cleanup_options(a) == {"min_component_area": 0, "keep_largest": False, "fill_holes": 0, "component_connectivity": 8}
    assert not C.cleanup_is_on(C.cleanup_options(a)) and not C.cleanup_is_on(None) and a.area_rule == "pixels"
    a = C.build_parser().parse_args(["--ann", "a.json", "--save-path", "b.json", "--min-component-area", "16", "--keep-largest",
                                     "--fill-holes", "all", "--component-connectivity", "4", "--area-rule", "bbox"])
    assert C.cleanup_options(a) == {"min_component_area": 16, "keep_largest": True, "fill_holes": C.FILL_ALL, "component_connectivity": 4}
    assert C.cleanup_is_on(C.cleanup_options(a)) and a.area_rule == "bbox"
    assert C.build_parser().parse_args(["--ann", "a", "--save-path", "b", "--fill-holes", "7"]).fill_holes == 7
    for bad in (["--fill-holes", "-1"], ["--fill-holes", "some"], ["--component-connectivity", "6"], ["--area-rule", "box"]):
        with pytest.raises(SystemExit):
            C.build_parser().parse_args(["--ann", "a", "--save-path", "b"] + bad)
    with pytest.raises(ValueError):
        C.clean_document({"images": [], "annotations": []}, min_component_area=-1)
    with pytest.raises(ValueError):
        C.clean_document({"images": [], "annotations": []}, min_component_area=1, area_rule="box")
    # the same four options on the three drivers that write an annotation file
    import argparse
    ap = C.add_cleanup_arguments(argparse.ArgumentParser())
    assert C.cleanup_options(ap.parse_args(["--fill-holes", "ALL"]))["fill_holes"] == C.FILL_ALL


def test_drivers_accept_the_options_and_pass_them_on(monkeypatch, tmp_path):
    from s2d_amd import clean_annotations as C, selftrain, selftrain_video
    from s2d_amd.keymask import results_to_annotations
    seen = []
    monkeypatch.setattr(selftrain, "merge_files", lambda *a, **k: seen.append(k["cleanup"]) or {"images": [], "annotations": []})
    selftrain.main(["--min-component-area", "9", "--fill-holes", "all"])
    monkeypatch.setattr(selftrain_video, "merge_files", lambda *a, **k: seen.append(k["cleanup"]) or {"videos": [], "annotations": []})
    selftrain_video.main(["--results-file", "r", "--prev-ann", "p", "--save-path", "s", "--keep-largest"])
    monkeypatch.setattr(results_to_annotations, "convert_files", lambda *a, **k: seen.append(k["cleanup"]) or "path")
    results_to_annotations.main(["--annotation-file", "a", "--gt-annotation-file", "g", "--results-file", "r", "--output-dir", "d",
                                 "--output-filename", "n", "--component-connectivity", "4"])
    assert seen[0] == {"min_component_area": 9, "keep_largest": False, "fill_holes": C.FILL_ALL, "component_connectivity": 8}
    assert seen[1]["keep_largest"] is True and seen[2]["component_connectivity"] == 4 and not C.cleanup_is_on(seen[2])


OPTION_SETS = (dict(min_component_area=4), dict(fill_holes=R.FILL_ALL), dict(keep_largest=True),
               dict(min_component_area=3, keep_largest=True, fill_holes=5, component_connectivity=4))


@pytest.mark.parametrize("make", (R.make_coco_doc, R.make_ytvis_doc))
def test_clean_document_host_logic(make):
    from s2d_amd import clean_annotations as C
    doc, masks = make()
    before = copy.deepcopy(doc)
    video = "videos" in doc
    for opts in OPTION_SETS:
        for rule in C.AREA_RULES:
            want, want_stats = R.ref_clean_document(doc, area_rule=rule, **opts)
            got, stats = C.clean_document(doc, area_rule=rule, device_fn=R.ref_device_fn(), **opts)
            assert json.dumps(got) == json.dumps(want) and stats == want_stats
            assert doc == before                                         # the input is not modified
            by_id = {a["id"]: a for a in got["annotations"]}
            for ann in doc["annotations"]:
                new = by_id.get(ann["id"])
                if ann.get("iscrowd") == 1:
                    assert new is ann                                    # crowd annotations are left alone
                if new is not None and new == ann:
                    assert new is ann                                    # unchanged: the same object
            assert [a["id"] for a in got["annotations"]] == [a["id"] for a in doc["annotations"] if a["id"] in by_id]   # no renumbering
            assert stats["annotations_dropped"] == len(doc["annotations"]) - len(got["annotations"])
    # the emptied and dropped rules on what the synthetic document was built to hold
    got, stats = C.clean_document(doc, min_component_area=2, device_fn=R.ref_device_fn())
    assert stats["annotations_dropped"] >= 1 and stats["pixels_filled"] == 0 and stats["planes_changed"] < stats["planes"]
    if video:
        assert stats["frames_emptied"] > 3 * stats["annotations_dropped"] - 3
        for a in got["annotations"]:
            assert len(a["segmentations"]) == len(a["bboxes"]) == len(a["areas"])
            for s, b, ar in zip(a["segmentations"], a["bboxes"], a["areas"]):
                assert (s is None) == (b is None) == (ar is None)
            assert any(s is not None for s in a["segmentations"])
        mixed = [a for a in got["annotations"] if a["segmentations"][1] is None and before["annotations"][0]["id"] != a["id"]]
        assert mixed                                                     # a frame of speckle became None, its track stayed
    else:
        for a, b in zip(got["annotations"], [x for x in doc["annotations"] if x["id"] in {y["id"] for y in got["annotations"]}]):
            if a is not b:
                m = R.decode_segmentation(a["segmentation"], *a["segmentation"]["size"])
                assert isinstance(a["segmentation"]["counts"], str) and a["area"] == m.sum() and a["bbox"] == [float(v) for v in R.tight_box(m)]
        boxed, _ = C.clean_document(doc, min_component_area=2, area_rule="bbox", device_fn=R.ref_device_fn())
        changed = [a for a, b in zip(boxed["annotations"], got["annotations"]) if a.get("area") != b.get("area")]
        assert changed and all(a["area"] == a["bbox"][2] * a["bbox"][3] for a in changed)


def test_options_off_returns_the_document_and_calls_nothing():
    from s2d_amd import clean_annotations as C
    for make in (R.make_coco_doc, R.make_ytvis_doc):
        doc, _ = make()

        def boom(chunk, opts):
            raise AssertionError("the device function was called with every option off")
        got, stats = C.clean_document(doc, device_fn=boom)
        assert got is doc and set(stats) == set(C.STAT_KEYS) and not any(stats.values())
        got, stats = C.clean_document(doc, component_connectivity=4, area_rule="bbox", device_fn=boom)
        assert got is doc
        assert C.clean_merged(doc, C.cleanup_options(C.build_parser().parse_args(["--ann", "a", "--save-path", "b"]))) is doc


def test_chunks_respect_the_bound(monkeypatch):
    from s2d_amd import clean_annotations as C
    doc, _ = R.make_coco_doc()
    monkeypatch.setattr(C, "CLEAN_CHUNK_WORDS", 300)
    sizes = []
    inner = R.ref_device_fn()

    def fn(chunk, opts):
        sizes.append([(h * w + 31) // 32 for h, w in chunk.sizes])
        return inner(chunk, opts)
    got, stats = C.clean_document(doc, min_component_area=4, device_fn=fn)
    want, want_stats = R.ref_clean_document(doc, min_component_area=4)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats
    assert len(sizes) > 3 and any(len(s) == 1 and s[0] > 300 for s in sizes)          # a plane over the bound is alone
    assert all(sum(s) <= 300 or len(s) == 1 for s in sizes)


def test_abi_additions():
    from s2d_amd import ops
    from s2d_amd._lib import LIBPATH, parse_header
    protos = parse_header()
    for name, n in (("s2d_plane_components_ragged", 12), ("s2d_plane_clean_ragged", 15), ("s2d_plane_components_tile", 2),
                    ("s2d_rle_count_ragged_u32", 12), ("s2d_rle_positions_ragged_u32", 11), ("s2d_rle_strings_ragged", 12)):
        assert len(protos[name][0]) == n
    assert protos["s2d_plane_components_workspace_bytes"][1] == "long" and protos["s2d_rle_strings_ragged_workspace_bytes"][1] == "long"
    dll = ctypes.CDLL(LIBPATH)
    assert dll.s2d_abi_version() == 11
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert dll.s2d_plane_components_tile(ctypes.byref(th), ctypes.byref(tw)) == 0 and th.value >= 2 and tw.value >= 2
    ws = dll.s2d_plane_components_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_long, [ctypes.c_long, ctypes.c_int]
    assert ws(-1, 1) == -1 and ws(1, -1) == -1 and ws(1000, 10) >= 12 * 32 * 1000 + 80
    for name in ("plane_components", "clean_planes", "plane_component_tile"):
        assert getattr(ops, name).__module__ == "s2d_amd.plane_components"
    assert ops.component_tile.__module__ == "s2d_amd.index_components"
    from s2d_amd.plane_components import plane_tiles
    tiles = plane_tiles(np.array([[0, th.value + 1, 2 * tw.value, 0], [99, 1, 1, 0]], np.int64))
    assert tiles.tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0]]
