"""ops.morph_planes (csrc/plane_morph.hip) and the annotation cleanup with smoothing (clean_annotations.py) against
tests/plane_morph_refs.py.  Every comparison is an integer or byte equality over every element: output words (padding, the words
between planes and a guard region included), cleared and set counts, whole documents.  The tile-crossing planes are built from the
tile the library reports.

The issue asks that every row be an equality with the scipy restatement.  The rows at r <= 8 and every document row are.  The rows at
r = 31, 32, 33 and 64 compare against the brute-force offset loop of the same definitions (plane_morph_refs.brute) instead: once the
element is larger than the plane scipy builds a table of pixels x offsets and needs 3 to 6 s per row.  The loop is independent of the
kernel, and tests/test_plane_morph_refs_cpu.py holds it equal to scipy at exactly these radii, with the whole element and with the
element cut to the plane."""
import copy
import json

import numpy as np
import pytest
import torch

from tests import plane_components_refs as C
from tests import plane_morph_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0x5a5a5a5a
GUARD = 8
RADII = (1, 2, 3, 8, 31, 32, 33, 64)
_REF = {}


def _ref(key, planes, op, r, shape):
    """the reference of one plane list under one op, computed once: open and close from the cached primitives.  The scipy
    restatement up to r = 8; from r = 31 on the elements are larger than the planes, scipy takes seconds per row for its offset tables,
    and the reference is the brute-force loop of the same definitions (tests/test_plane_morph_refs_cpu.py holds the two equal at
    these radii too)"""
    k = (key, op, r, shape)
    fn = R.morph if r <= 8 else R.brute
    if k not in _REF:
        if op in ("erode", "dilate"):
            _REF[k] = [fn(m, op, r, shape) for m in planes]
        else:
            first = _ref(key, planes, "erode" if op == "open" else "dilate", r, shape)
            _REF[k] = [fn(m, "dilate" if op == "open" else "erode", r, shape) for m in first]
    return _REF[k]


def _chunk(planes, gap_words=3):
    """planes -> (bits with the padding bits set, gap words of ones between the planes and GUARD words of ones behind, table)"""
    bits, plane = C.pack_planes(planes, set_padding=True, gap_words=gap_words)
    return np.concatenate([bits, np.full(GUARD, -1, np.int32)]), plane


def _expected(ref_planes, plane, words):
    """the words of `out`: FILL wherever no plane lies, the reference planes with their padding bits 0"""
    want = np.full(words, FILL, np.int32)
    for m, row in zip(ref_planes, plane):
        w, _ = C.pack_planes([m])
        want[int(row[0]):int(row[0]) + len(w)] = w
    return want


def check(planes, ref_planes, op, radius, shape, twice=False):
    """out, cleared and set of a chunk against the reference planes; the input unchanged -> (cleared, set) of the reference"""
    from s2d_amd import ops
    bits, plane = _chunk(planes)
    src = torch.from_numpy(bits).to(DEV)
    want = _expected(ref_planes, plane, len(bits))
    want_cleared = np.array([(m & ~o).sum() for m, o in zip(planes, ref_planes)], np.int32)
    want_set = np.array([(o & ~m).sum() for m, o in zip(planes, ref_planes)], np.int32)
    runs = []
    for _ in range(2 if twice else 1):
        dst = torch.full_like(src, FILL)
        out, cleared, set_ = ops.morph_planes(src, plane, op, radius, shape, out=dst)
        assert out.data_ptr() == dst.data_ptr()
        runs.append((out.cpu().numpy(), cleared.cpu().numpy(), set_.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0], want, err_msg=f"{op} {shape} r={radius}")
    np.testing.assert_array_equal(runs[0][1], want_cleared)
    np.testing.assert_array_equal(runs[0][2], want_set)
    if op in ("open", "erode"):
        assert not want_set.any()
    if op in ("close", "dilate"):
        assert not want_cleared.any()
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[-1]))
    np.testing.assert_array_equal(src.cpu().numpy(), bits)
    return want_cleared, want_set


# ---------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("r", RADII)
def test_sizes_one_chunk(r, shape):
    from s2d_amd import ops
    rows, words = ops.morph_tile(r)
    assert rows >= 2 and words <= 32                                     # 3 x 1030 = 33 row words crosses a word tile
    planes = R.size_chunk(rows, seed=r)
    assert len(planes) == 30 and planes[-1].shape == (rows + 1, 40)
    for op in R.OPS:
        check(planes, _ref(("sizes", r), planes, op, r, shape), op, r, shape)


# ---------------------------------------------------------------------------------------------------------------- halo words
@pytest.mark.parametrize("r", (31, 32, 33, 64))
def test_a_pixel_exactly_r_away_across_a_word_and_across_the_word_tile_seam(r):
    """one set pixel r columns before / after a word boundary reaches across it and no further, inside a word tile and across the
    seam between two: from r = 33 on the pixel lies in the SECOND word beside the one it changes"""
    from s2d_amd import ops
    seam = 32 * ops.morph_tile(r)[1]
    W = seam + 3 * 32 + 7
    planes = []
    for edge in (seam, 5 * 32):
        for x in (edge - r, edge - 1 + r):
            m = np.zeros((3, W), bool)
            m[1, x] = True
            planes.append(m)
    for shape in R.SHAPES:
        ref = _ref(("halo", r), planes, "dilate", r, shape)
        for k, edge in enumerate((seam, 5 * 32)):
            assert ref[2 * k][1, edge] and not ref[2 * k][1, edge + 1] and ref[2 * k + 1][1, edge - 1] and not ref[2 * k + 1][1, edge - 2]
        check(planes, ref, "dilate", r, shape)
        holes = [~m for m in planes]
        check(holes, _ref(("halo holes", r), holes, "erode", r, shape), "erode", r, shape)


# ---------------------------------------------------------------------------------------------------------------- per-plane radii
@pytest.mark.parametrize("shape", R.SHAPES)
def test_per_plane_radii_in_one_launch(shape):
    from s2d_amd import ops
    planes = R.size_chunk(ops.morph_tile(64)[0], seed=3)
    radii = np.array([(0, 1, 5, 64)[(i % 3 + i // 3 + 1) % 4] for i in range(len(planes))], np.int32)
    assert {(m.shape, int(r)) for m, r in zip(planes, radii)} >= {((1, 1), 64), ((3, 1030), 5), ((3, 1030), 64)}
    for op in R.OPS:
        ref = [(R.morph if r <= 8 else R.brute)(m, op, int(r), shape) for m, r in zip(planes, radii)]
        for m, o, r in zip(planes, ref, radii):
            if r == 0:
                assert (o == m).all()                                    # r = 0: the plane itself, its padding zeroed in `out`
        check(planes, ref, op, radii, shape)
        check(planes, ref, op, torch.from_numpy(radii).to(DEV), shape)
    # each plane equals its own single-radius result on the device as well
    bits, plane = _chunk(planes)
    src = torch.from_numpy(bits).to(DEV)
    mixed = ops.morph_planes(src, plane, "open", radii, shape)[0].cpu().numpy()
    for r in (0, 1, 5, 64):
        single = ops.morph_planes(src, plane, "open", r, shape)[0].cpu().numpy()
        for row in plane[radii == r]:
            w0, n = int(row[0]), (int(row[1]) * int(row[2]) + 31) // 32
            np.testing.assert_array_equal(mixed[w0:w0 + n], single[w0:w0 + n])


# ---------------------------------------------------------------------------------------------------------------- border rule, named shapes
def test_border_rule_and_named_shapes():
    planes, names = [], []
    for H, W in ((20, 32), (37, 45)):                                    # word-aligned rows, and an unaligned plane
        planes += [np.ones((H, W), bool), np.zeros((H, W), bool)]
        names += ["full", "empty"]
        for edge in R.EDGES:
            planes += [R.edge_rect(H, W, edge), R.edge_strip(H, W, edge)]
            names += [f"rect {edge}", f"strip {edge}"]
    last = np.zeros((37, 45), bool)
    last[36, 44] = last[0, 44] = last[36, 0] = True                       # the last row / column of an unaligned plane
    planes += [last, R.whisker(), R.crack()]
    names += ["last", "whisker", "crack"]
    for shape in R.SHAPES:
        for r in (1, 2):
            for op in R.OPS:
                ref = _ref("named", planes, op, r, shape)
                cleared, set_ = check(planes, ref, op, r, shape)
                for n, m, o in zip(names, planes, ref):
                    if n == "full":
                        assert o.all()
                    if n == "empty":
                        assert not o.any()
                    if n.startswith("strip") and op in ("open", "erode"):
                        assert not o.any()
                    if n.startswith("rect") and op == "open" and r == 2:
                        assert o.sum() == (54 if shape == "disk" else 60)   # the edge corners stay: 48 with a zero border
    got = dict(zip(names, _ref("named", planes, "open", 1, "square")))
    np.testing.assert_array_equal(got["whisker"], R.whisker_object())
    from scipy import ndimage
    assert ndimage.label(dict(zip(names, _ref("named", planes, "close", 1, "disk")))["crack"])[1] == 1


# ---------------------------------------------------------------------------------------------------------------- determinism, refusals
def test_second_call_is_bitwise_equal():
    from s2d_amd import ops
    planes = R.size_chunk(ops.morph_tile(8)[0], seed=7)
    for op in ("open", "close"):
        check(planes, _ref("twice", planes, op, 8, "disk"), op, 8, "disk", twice=True)


def test_refusals_write_nothing():
    from s2d_amd import ops, plane_morph
    from s2d_amd._lib import lib
    planes = [np.ones((5, 7), bool), np.ones((40, 40), bool)]
    bits, plane = _chunk(planes)
    src = torch.from_numpy(bits).to(DEV)
    out = torch.full_like(src, FILL)
    both = torch.from_numpy(np.concatenate([bits, bits])).to(DEV)
    for bad in (lambda: ops.morph_planes(src, plane, "open", 1, out=src),                       # aliased
                lambda: ops.morph_planes(both[:len(bits)], plane, "open", 1, out=both[4:4 + len(bits)]),   # overlapping
                lambda: ops.morph_planes(src, plane, "open", 65, out=out),
                lambda: ops.morph_planes(src, plane, "open", [1, 65], out=out),
                lambda: ops.morph_planes(src, plane, "open", -1, out=out),
                lambda: ops.morph_planes(src, plane, "open", [1], out=out),
                lambda: ops.morph_planes(src, plane, "open", 1.5, out=out),
                lambda: ops.morph_planes(src, plane, "smooth", 1, out=out),
                lambda: ops.morph_planes(src, plane, "open", 1, "cross", out=out),
                lambda: ops.morph_planes(src, np.array([[0, 50, 70, 0]], np.int64), "open", 1, out=out),   # does not fit the buffer
                lambda: ops.morph_planes(src.cpu(), plane, "open", 1),
                lambda: ops.morph_planes(src.float(), plane, "open", 1),
                lambda: ops.morph_planes(src, plane, "open", 1, out=out.cpu()),
                lambda: ops.morph_planes(src, plane, "open", 1, out=out[:-1])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        ops.morph_tile(65)
    # the library itself: an error code before anything is launched, nothing written
    raw = lib()
    p = lambda t: t.data_ptr()                                           # noqa: E731
    n = len(bits)
    plane_d, rad = torch.from_numpy(plane).to(DEV), torch.ones((2,), dtype=torch.int32, device=DEV)
    tiles = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    tiles[1, 0] = 1
    ws = torch.full((raw.call("s2d_plane_morph_workspace_bytes", n, 2),), 0x5a, dtype=torch.uint8, device=DEV)
    cnt = torch.full((2, 2), 77, dtype=torch.int32, device=DEV)
    morph = raw._raw_s2d_plane_morph_ragged
    ERR = -1
    lds = raw.call("s2d_plane_morph_lds_words", 1, 40, 40)                # the larger of the two planes' needs
    assert lds == plane_morph.morph_lds_words(plane, [1, 1]) > raw.call("s2d_plane_morph_lds_words", 1, 5, 7) > 0
    ok = (p(src), p(plane_d), 2, n, 2, 0, p(rad), p(tiles), 2, lds, p(out), p(cnt[0]), p(cnt[1]), p(ws), None)
    for i, v in ((10, p(src)), (10, p(src) + 4), (10, p(ws)), (13, p(out)), (13, p(src)), (4, 4), (4, -1), (5, 2), (2, -1), (3, -1), (8, -1),
                 (9, -1), (9, 0), (9, 10241), (0, None), (1, None), (6, None), (7, None), (10, None), (11, None), (12, None), (13, None),
                 (10, p(out) + 2)):
        args = list(ok)
        args[i] = v
        assert morph(*args) == ERR, (i, v)
    torch.cuda.synchronize()
    assert (out == FILL).all() and (cnt == 77).all() and (ws == 0x5a).all()
    np.testing.assert_array_equal(src.cpu().numpy(), bits)
    assert raw.call("s2d_plane_morph_workspace_bytes", -1, 1) == ERR
    # the same arguments unchanged are accepted: the refusals above are the arguments', not the call's
    assert morph(*ok) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), _expected(planes, plane, n))      # full planes stay full under open


# ---------------------------------------------------------------------------------------------------------------- realistic size
def test_realistic_planes():
    planes = [C.blob_with_speckle(480, 854, 1), C.blob_with_speckle(720, 1280, 2)]
    radii = np.array([R.ref_radius("1%", *m.shape) for m in planes], np.int32)
    assert radii.tolist() == [10, 15]
    for op in ("open", "close"):
        ref = [R.morph(m, op, int(r), "disk") for m, r in zip(planes, radii)]
        cleared, set_ = check(planes, ref, op, radii, "disk")
        assert (cleared + set_).min() > 100


# ---------------------------------------------------------------------------------------------------------------- the pipeline
OPTS = dict(open_radius=2, close_radius="1%", min_component_area=4, fill_holes=6)


@pytest.mark.parametrize("make", (R.make_coco_doc, R.make_ytvis_doc))
def test_clean_document_on_the_device_equals_the_reference(make, monkeypatch, tmp_path):
    from s2d_amd import clean_annotations as A, plane_morph
    doc, _ = make()
    before = copy.deepcopy(doc)
    want, want_stats = R.ref_clean_document(doc, area_rule="bbox", **OPTS)
    c0 = dict(plane_morph.LIB_CALLS)
    got, stats = A.clean_document(doc, area_rule="bbox", device=DEV, **OPTS)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats and doc == before
    assert stats["pixels_opened"] > 0 and stats["pixels_closed"] > 0 and stats["annotations_dropped"] > 0
    # one chunk: an opening, a closing and the difference counts
    assert {k: v - c0.get(k, 0) for k, v in plane_morph.LIB_CALLS.items()} == {"s2d_plane_morph_ragged": 2, "s2d_plane_diff_counts_ragged": 1}
    # several chunks and a plane that exceeds the bound alone: the same document
    monkeypatch.setattr(A, "CLEAN_CHUNK_WORDS", 200)
    chunks = []
    real = A.device_clean
    monkeypatch.setattr(A, "device_clean", lambda chunk, *a, **k: chunks.append(len(chunk.segs)) or real(chunk, *a, **k))
    got, stats = A.clean_document(doc, area_rule="bbox", device=DEV, **OPTS)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats
    assert len(chunks) > 3 and 1 in chunks
    # the command line writes the same file
    src, dst = str(tmp_path / "in.json"), str(tmp_path / "out.json")
    with open(src, "w") as fh:
        json.dump(doc, fh)
    monkeypatch.setattr(A, "CLEAN_CHUNK_WORDS", 5 << 19)
    A.main(["--ann", src, "--save-path", dst, "--open", "2", "--close", "1%", "--min-component-area", "4", "--fill-holes", "6",
            "--area-rule", "bbox"])
    with open(dst) as fh:
        assert json.load(fh) == json.loads(json.dumps(want))
    # the closing alone, with the square: speckle survives it, so the component rules work on the smoothed planes
    alone = dict(close_radius=1, smooth_shape="square", min_component_area=4, fill_holes=6)
    want, want_stats = R.ref_clean_document(doc, **alone)
    got, stats = A.clean_document(doc, device=DEV, **alone)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats and stats["pixels_opened"] == 0 < stats["pixels_closed"]
    assert stats["pixels_removed"] > 0


def test_a_radius_over_64_names_the_image_before_any_launch():
    from s2d_amd import clean_annotations as A, plane_morph, plane_components
    doc, _ = R.make_coco_doc()
    doc["images"][2]["height"], doc["images"][2]["width"] = 3000, 4000
    c0 = sum(plane_morph.LIB_CALLS.values()), sum(plane_components.LIB_CALLS.values())
    with pytest.raises(ValueError, match=r"12 \(annotation"):
        A.clean_document(doc, open_radius="2%", device=DEV)
    assert c0 == (sum(plane_morph.LIB_CALLS.values()), sum(plane_components.LIB_CALLS.values()))


# ---------------------------------------------------------------------------------------------------------------- the off path
def _all_calls():
    from s2d_amd import coco_eval, plane_components, plane_morph, rle_ragged, selftrain, selftrain_video
    return {m.__name__: dict(m.LIB_CALLS) for m in (coco_eval, plane_components, plane_morph, rle_ragged, selftrain, selftrain_video)}


def _delta(a, b):
    return {m: {k: b[m].get(k, 0) - a[m].get(k, 0) for k in b[m] if b[m].get(k, 0) != a[m].get(k, 0)} for m in b}


def test_with_both_radii_zero_the_drivers_write_the_same_bytes_with_the_same_calls(tmp_path):
    from tests import selftrain_refs, selftrain_video_refs
    from s2d_amd import clean_annotations as A, plane_morph, selftrain, selftrain_video
    from s2d_amd.keymask import results_to_annotations
    off = A.cleanup_options(A.build_parser().parse_args(["--ann", "a", "--save-path", "b", "--open", "0", "--close", "0%"]))
    assert sorted(off) == ["component_connectivity", "fill_holes", "keep_largest", "min_component_area"]
    prev, preds = selftrain_refs.random_case(12, seed=0)
    vdoc, vpreds = selftrain_video_refs.merge_case()
    known = {v["id"] for v in vdoc["videos"]}
    kpreds = [r for r in vpreds if r["video_id"] in known]
    cdoc, _ = R.make_coco_doc()
    paths = {}
    for name, d in (("preds", preds), ("prev", prev), ("vpreds", vpreds), ("vdoc", vdoc), ("kpreds", kpreds), ("cdoc", cdoc)):
        paths[name] = str(tmp_path / f"{name}.json")
        with open(paths[name], "w") as fh:
            json.dump(d, fh)
    morph0 = dict(plane_morph.LIB_CALLS)
    runs = []
    for cleanup in (None, off):
        tag = "plain" if cleanup is None else "off"
        c0 = _all_calls()
        selftrain.merge_files(paths["preds"], paths["prev"], str(tmp_path / f"img_{tag}.json"), device=DEV, cleanup=cleanup)
        selftrain_video.merge_files(paths["vpreds"], paths["vdoc"], str(tmp_path / f"vid_{tag}.json"), device=DEV, cleanup=cleanup)
        results_to_annotations.convert_files(paths["vdoc"], paths["vdoc"], paths["kpreds"], 0.5, str(tmp_path), f"key_{tag}", cleanup=cleanup)
        A.clean_file(paths["cdoc"], str(tmp_path / f"clean_{tag}.json"), device=DEV, **(cleanup or {}))
        runs.append((_delta(c0, _all_calls()),) + tuple(open(tmp_path / f"{n}_{tag}.json", "rb").read() for n in ("img", "vid", "key", "clean")))
    assert runs[0] == runs[1] and not runs[1][0]["s2d_amd.plane_morph"] and not runs[1][0]["s2d_amd.plane_components"]
    assert all(len(b) > 100 for b in runs[1][1:])
    assert dict(plane_morph.LIB_CALLS) == morph0                         # zero calls of this module on the off path
    # with a radius on, the post-pass of a driver is clean_document over the merged document
    on = dict(off, open_radius=1, close_radius="1%", smooth_shape="square")
    merged = json.loads(runs[0][2])
    got = selftrain_video.merge_files(paths["vpreds"], paths["vdoc"], str(tmp_path / "vid_on.json"), device=DEV, cleanup=on)
    assert json.dumps(got) == json.dumps(R.ref_clean_document(merged, **on)[0])
