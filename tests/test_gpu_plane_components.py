"""ops.plane_components / ops.clean_planes (csrc/plane_components.hip), rle_ragged.encode_ragged and clean_annotations.clean_document
against tests/plane_components_refs.py.  Every comparison is an integer or byte equality over every element: labels, areas, output
words (padding included), removed and filled counts, RLE strings and whole documents.  The border and corner cases are built from
the tile the library reports."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import plane_components_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CONNS = (4, 8)
_REF = {}


@pytest.fixture(scope="module")
def tile():
    from s2d_amd import ops
    th, tw = ops.plane_component_tile()
    assert th >= 2 and tw >= 2
    return th, tw


def _ref_labels(key, planes, value, conn):
    """the reference labelling of a named chunk, computed once"""
    k = (key, value, conn)
    if k not in _REF:
        _REF[k] = [R.ref_labels(m, value, conn) for m in planes]
    return _REF[k]


def check_labels(key, planes, conn, value=1, set_padding=False, gap_words=0):
    """labels and areas of a chunk, twice, and the input unchanged -> the per-plane reference [(labels, area)]"""
    from s2d_amd import ops
    bits, plane = R.pack_planes(planes, set_padding=set_padding, gap_words=gap_words)
    want = _ref_labels(key, planes, value, conn)
    want_labels = R.expected_per_pixel([w[0] for w in want], plane, len(bits))
    want_area = R.expected_per_pixel([w[1] for w in want], plane, len(bits))
    dev = torch.from_numpy(bits).to(DEV)
    runs = []
    for _ in range(2):
        labels, area = ops.plane_components(dev, plane, value, conn)
        runs.append((labels.cpu().numpy(), area.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0], want_labels)
    np.testing.assert_array_equal(runs[0][1], want_area)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    only, none = ops.plane_components(dev, torch.from_numpy(plane).to(DEV), value, conn, want_area=False)
    assert none is None
    np.testing.assert_array_equal(only.cpu().numpy(), want_labels)
    np.testing.assert_array_equal(dev.cpu().numpy(), bits)
    return want


def check_clean(planes, conn, min_area=0, keep_largest=False, max_hole_area=0, set_padding=False, alias=False):
    """out, removed and filled of a chunk against the reference, twice -> (out planes, removed, filled) of the reference"""
    from s2d_amd import ops
    bits, plane = R.pack_planes(planes, set_padding=set_padding)
    ref = [R.ref_clean(m, min_area, keep_largest, max_hole_area, conn) for m in planes]
    want_bits, _ = R.pack_planes([r[0] for r in ref])
    want_removed, want_filled = np.array([r[1] for r in ref], np.int32), np.array([r[2] for r in ref], np.int32)
    runs = []
    for _ in range(2):
        src = torch.from_numpy(bits).to(DEV)
        dst = src if alias else torch.full_like(src, 0x5a5a5a5a)
        out, removed, filled = ops.clean_planes(src, plane, min_area, keep_largest, max_hole_area, conn, out=dst)
        assert out.data_ptr() == dst.data_ptr()
        runs.append((out.cpu().numpy(), removed.cpu().numpy(), filled.cpu().numpy()))
        if not alias:
            np.testing.assert_array_equal(src.cpu().numpy(), bits)
    np.testing.assert_array_equal(runs[0][0], want_bits)
    np.testing.assert_array_equal(runs[0][1], want_removed)
    np.testing.assert_array_equal(runs[0][2], want_filled)
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
    return [r[0] for r in ref], want_removed, want_filled


# ---------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("conn", CONNS)
def test_sizes_one_chunk(tile, conn):
    planes = R.size_chunk(*tile)
    assert len(planes) > 30
    check_labels("sizes", planes, conn)
    check_labels("sizes", planes, conn, value=0)
    check_clean(planes, conn, min_area=4, max_hole_area=3)


# ---------------------------------------------------------------------------------------------------------------- row wrap
@pytest.mark.parametrize("conn", CONNS)
def test_row_wrap(tile, conn):
    th, _ = tile
    planes = [R.row_wrap(th + 3, W) for W in (1, 33, 64)]
    want = check_labels("wrap", planes, conn)
    if conn == 4:
        for (labels, area), m in zip(want[1:], planes[1:]):             # W = 33, 64: every pixel its own component
            assert (area > 0).sum() == m.sum() and area.max() == 1
    assert (want[0][1] > 0).sum() == 1 and want[0][1].max() == th + 3    # W = 1: vertical neighbours, one component
    check_labels("wrap", planes, conn, value=0)


# ---------------------------------------------------------------------------------------------------------------- padding
@pytest.mark.parametrize("conn", CONNS)
def test_padding_bits_are_no_pixels(tile, conn):
    planes = R.size_chunk(*tile, seed=5)
    for value in (1, 0):
        check_labels("pad", planes, conn, value=value, set_padding=True, gap_words=3)
    # the zero pixels of a plane add up to H*W - set pixels: no background area comes from padding or from outside the plane
    for (labels, area), m in zip(_ref_labels("pad", planes, 0, conn), planes):
        assert area.sum() == m.size - m.sum()
    check_clean(planes, conn, set_padding=True)                          # every option off: a copy with the padding zeroed
    check_clean(planes, conn, min_area=3, max_hole_area=R.FILL_ALL, set_padding=True)


# ---------------------------------------------------------------------------------------------------------------- merge worst cases
@pytest.mark.parametrize("conn", CONNS)
def test_merge_worst_cases(tile, conn):
    cases = R.merge_cases(*tile)
    names = sorted(cases)
    planes = [cases[n] for n in names]
    want = dict(zip(names, check_labels("merge", planes, conn)))
    count = {n: int((want[n][1] > 0).sum()) for n in names}
    assert count["spiral"] == 1 and count["comb"] == 1
    assert count["checker"] == (cases["checker"].sum() if conn == 4 else 1)
    assert count["corner"] == count["corner_anti"] == (2 if conn == 4 else 1)
    check_labels("merge", planes, conn, value=0)
    check_clean(planes, conn, min_area=2, max_hole_area=R.FILL_ALL)


# ---------------------------------------------------------------------------------------------------------------- filter
def test_filter_thresholds_tie_and_emptied(tile):
    th, tw = tile
    m = R.tie_plane(th, tw)
    for conn in CONNS:
        _, removed, _ = check_clean([m, m], conn, min_area=9)             # at a component's area: the two nines stay
        assert removed.tolist() == [5, 5]
        _, removed, _ = check_clean([m], conn, min_area=10)              # at area + 1: every component is under it, the plane is emptied
        assert removed.tolist() == [int(m.sum())]
        outs, removed, _ = check_clean([m, np.zeros((3, 3), bool), m[:, ::-1]], conn, keep_largest=True)
        assert outs[0].sum() == 9 and outs[0][2:5, 2:5].all()             # the exact tie: the lower first pixel wins
        assert removed.tolist() == [int(m.sum()) - 9, 0, int(m.sum()) - 9]
        check_clean([m], conn, min_area=9, keep_largest=True)
        check_clean([m], conn, min_area=10, keep_largest=True)


# ---------------------------------------------------------------------------------------------------------------- holes
def test_holes(tile):
    cases = R.hole_cases(*tile)
    names = sorted(cases)
    planes = [cases[n] for n in names]
    for conn in CONNS:
        outs, _, filled = check_clean(planes, conn, max_hole_area=R.FILL_ALL)
        got = dict(zip(names, zip(outs, filled)))
        assert got["ring"][1] > 0 and got["nested"][1] > 0 and got["open"][1] == 0
        assert (got["diagonal"][1] > 0) == (conn == 8)                   # foreground 8 / background 4 closes it
    ring = cases["ring"]
    hole = int((R.ref_fill(ring, R.FILL_ALL, 8) & ~ring).sum())
    _, _, filled = check_clean([ring, ring], 8, max_hole_area=hole)
    assert filled.tolist() == [hole, hole]
    _, _, filled = check_clean([ring], 8, max_hole_area=hole - 1)
    assert filled.tolist() == [0]
    for conn in CONNS:                                                   # the island goes, then its ring is filled whole
        outs, removed, filled = check_clean([cases["island"]], conn, min_area=3, max_hole_area=R.FILL_ALL)
        assert removed.tolist() == [2] and outs[0][10, 10:12].all() and filled[0] > 2


# ---------------------------------------------------------------------------------------------------------------- aliasing, refusals
def test_alias_and_repeat(tile):
    planes = R.size_chunk(*tile, seed=9)
    for conn in CONNS:
        check_clean(planes, conn, min_area=5, keep_largest=False, max_hole_area=4, set_padding=True, alias=True)
        check_clean(planes, conn, keep_largest=True, max_hole_area=R.FILL_ALL, alias=True)


def test_refusals_write_nothing(tile):
    from s2d_amd import ops
    from s2d_amd._lib import lib
    planes = [np.ones((5, 7), bool)]
    bits, plane = R.pack_planes(planes)
    dev = torch.from_numpy(bits).to(DEV)
    for bad in (lambda: ops.plane_components(dev, plane, 1, 6), lambda: ops.plane_components(dev, plane, 2, 8),
                lambda: ops.clean_planes(dev, plane, min_area=-1), lambda: ops.clean_planes(dev, plane, max_hole_area=-1),
                lambda: ops.clean_planes(dev, plane, connectivity=6), lambda: ops.plane_components(dev.cpu(), plane),
                lambda: ops.plane_components(dev, np.array([[0, 50, 70, 0]], np.int64))):
        with pytest.raises((ValueError, RuntimeError)):
            bad()
    # the library itself: an error code before anything is launched, nothing written
    raw = lib()
    plane_d, tiles = torch.from_numpy(plane).to(DEV), torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    ws = torch.zeros((raw.call("s2d_plane_components_workspace_bytes", len(bits), 1),), dtype=torch.uint8, device=DEV)
    labels = torch.full((32 * len(bits),), 77, dtype=torch.int32, device=DEV)
    out = torch.full_like(dev, 77)
    cnt = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    comp, clean = raw._raw_s2d_plane_components_ragged, raw._raw_s2d_plane_clean_ragged
    p = lambda t: t.data_ptr()
    ERR = -1
    assert comp(p(dev), p(plane_d), 1, len(bits), 1, 6, p(tiles), 1, p(labels), None, p(ws), None) == ERR
    assert comp(p(dev), p(plane_d), 1, len(bits), 3, 8, p(tiles), 1, p(labels), None, p(ws), None) == ERR
    assert comp(None, p(plane_d), 1, len(bits), 1, 8, p(tiles), 1, p(labels), None, p(ws), None) == ERR
    assert comp(p(dev), p(plane_d), 1, len(bits), 1, 8, p(tiles), 1, None, None, p(ws), None) == ERR
    assert comp(p(dev), p(plane_d), 1, len(bits), 1, 8, None, 1, p(labels), None, p(ws), None) == ERR
    assert comp(p(dev), p(plane_d), 1, len(bits), 1, 8, p(tiles), 1, p(labels), None, None, None) == ERR
    assert clean(p(dev), p(plane_d), 1, len(bits), 6, 0, 0, 0, p(tiles), 1, p(out), p(cnt), p(cnt[1:]), p(ws), None) == ERR
    assert clean(p(dev), p(plane_d), 1, len(bits), 8, -1, 0, 0, p(tiles), 1, p(out), p(cnt), p(cnt[1:]), p(ws), None) == ERR
    assert clean(p(dev), p(plane_d), 1, len(bits), 8, 0, 0, -1, p(tiles), 1, p(out), p(cnt), p(cnt[1:]), p(ws), None) == ERR
    assert clean(p(dev), p(plane_d), 1, len(bits), 8, 1, 0, 0, p(tiles), 1, None, p(cnt), p(cnt[1:]), p(ws), None) == ERR
    assert clean(p(dev), p(plane_d), 1, len(bits), 8, 1, 0, 0, p(tiles), 1, p(out), None, p(cnt[1:]), p(ws), None) == ERR
    assert raw.call("s2d_plane_components_workspace_bytes", -1, 1) == ERR
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert raw._raw_s2d_plane_components_tile(None, ctypes.addressof(tw)) == ERR
    torch.cuda.synchronize()
    assert (labels == 77).all() and (out == 77).all() and (cnt == 77).all()
    np.testing.assert_array_equal(dev.cpu().numpy(), bits)


# ---------------------------------------------------------------------------------------------------------------- encode
def _encode_planes(tile):
    th, tw = tile
    rng = np.random.default_rng(11)
    planes = [R.random_plane(H, W, rng, 0.5) for H, W in R.size_cases(th, tw)[::3]]
    ends = np.zeros((7, 9), bool)
    ends[0, 0] = ends[-1, -1] = True                                      # starts and ends on a set pixel
    planes += [np.zeros((5, 33), bool), np.ones((5, 33), bool), ends, np.ones((1, 1), bool), np.zeros((1, 1), bool),
               R.speckled_mask(97, 130, rng)]
    return planes


def test_encode_ragged_strings_boxes_and_round_trip(tile):
    from s2d_amd import rle, rle_ragged
    planes = _encode_planes(tile)
    bits, plane = R.pack_planes(planes, set_padding=True)
    dev = torch.from_numpy(bits).to(DEV)
    sel = np.random.default_rng(2).permutation(len(planes))[: len(planes) - 3]       # a subset in a shuffled order
    calls0 = sum(rle_ragged.LIB_CALLS.values())
    rles, areas, boxes = rle_ragged.encode_ragged(dev, plane, sel)
    assert sum(rle_ragged.LIB_CALLS.values()) - calls0 == 3               # whatever the selection holds
    assert len(rles) == len(sel)
    for r, a, b, p in zip(rles, areas, boxes, sel):
        m = planes[p]
        assert r == R.encode_mask(m)                                      # the numpy encoder
        fixed, fa, fb = rle.encode(torch.from_numpy(m[None].astype(np.uint8)).to(DEV))
        assert fixed[0]["counts"].decode("ascii") == r["counts"] and fixed[0]["size"] == r["size"]      # the fixed-size call
        assert a == m.sum() == fa[0] and b.tolist() == [float(v) for v in R.tight_box(m)] == fb[0].tolist()
    np.testing.assert_array_equal(dev.cpu().numpy(), bits)
    # all planes, through the staged form, and back: decode_ragged(encode_ragged(x)) == x
    rles, _, _ = rle_ragged.encode_ragged(dev, plane, np.arange(len(planes)))
    staged = rle_ragged.stage_rle_ragged([[r] for r in rles], [m.shape for m in planes])
    dec = rle_ragged.decode_ragged(staged, DEV)
    want, _ = R.pack_planes(planes)
    np.testing.assert_array_equal(dec.bits.cpu().numpy(), want)
    again, _, _ = rle_ragged.encode_ragged(dec.bits, staged, np.arange(len(planes)))
    assert again == rles
    assert rle_ragged.encode_ragged(dev, plane, [])[0] == []
    with pytest.raises(ValueError):
        rle_ragged.encode_ragged(dev, plane, [len(planes)])


# ---------------------------------------------------------------------------------------------------------------- realistic size
def test_realistic_planes_through_clean_encode_decode():
    from s2d_amd import ops, rle_ragged
    planes = [R.blob_with_speckle(480, 854, 1), R.blob_with_speckle(720, 1280, 2)]
    bits, plane = R.pack_planes(planes)
    dev = torch.from_numpy(bits).to(DEV)
    out, removed, filled = ops.clean_planes(dev, plane, min_area=16, max_hole_area=R.FILL_ALL)
    ref = [R.ref_clean(m, 16, False, R.FILL_ALL, 8) for m in planes]
    np.testing.assert_array_equal(out.cpu().numpy(), R.pack_planes([r[0] for r in ref])[0])
    assert removed.tolist() == [r[1] for r in ref] and filled.tolist() == [r[2] for r in ref] and min(removed.tolist() + filled.tolist()) > 100
    rles, areas, boxes = rle_ragged.encode_ragged(out, plane, [1, 0])
    assert rles == [R.encode_mask(ref[1][0]), R.encode_mask(ref[0][0])] and areas.tolist() == [int(ref[1][0].sum()), int(ref[0][0].sum())]
    dec = rle_ragged.decode_ragged(rle_ragged.stage_rle_ragged([[rles[1]], [rles[0]]], [m.shape for m in planes]), DEV)
    np.testing.assert_array_equal(dec.bits.cpu().numpy(), out.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("make", (R.make_coco_doc, R.make_ytvis_doc))
def test_clean_document_on_the_device_equals_the_reference(make, monkeypatch, tmp_path):
    import json
    from s2d_amd import clean_annotations as C
    doc, _ = make()
    before = copy.deepcopy(doc)
    opts = dict(min_component_area=4, fill_holes=6, component_connectivity=8)
    want, want_stats = R.ref_clean_document(doc, area_rule="bbox", **opts)
    got, stats = C.clean_document(doc, area_rule="bbox", device=DEV, **opts)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats and doc == before
    assert stats["planes_changed"] > 0 and stats["annotations_dropped"] > 0
    # several chunks and a plane that exceeds the bound alone: the same document
    monkeypatch.setattr(C, "CLEAN_CHUNK_WORDS", 200)
    chunks = []
    real = C.device_clean
    monkeypatch.setattr(C, "device_clean", lambda chunk, *a, **k: chunks.append(len(chunk.segs)) or real(chunk, *a, **k))
    got, stats = C.clean_document(doc, area_rule="bbox", device=DEV, **opts)
    assert json.dumps(got) == json.dumps(want) and stats == want_stats
    assert len(chunks) > 3 and 1 in chunks and max((h * w + 31) // 32 for h, w in
                                                   [(r["height"], r["width"]) for r in doc.get("images", doc.get("videos"))]) > 200
    # the command line, and the loaders of s2d_amd.train read what it writes
    src, dst = str(tmp_path / "in.json"), str(tmp_path / "out.json")
    with open(src, "w") as fh:
        json.dump(doc, fh)
    monkeypatch.setattr(C, "CLEAN_CHUNK_WORDS", 5 << 19)
    C.main(["--ann", src, "--save-path", dst, "--min-component-area", "4", "--fill-holes", "6", "--area-rule", "bbox"])
    with open(dst) as fh:
        assert json.load(fh) == json.loads(json.dumps(want))
    from s2d_amd.data.image_clip import detect_train_format, load_coco_image_train
    from s2d_amd.data.train_loader import load_ytvis_train
    if detect_train_format(want) == "coco_image":
        records = load_coco_image_train(dst, str(tmp_path))
        assert sum(len(r["annotations"]) for r in records) == len(want["annotations"])
    else:
        assert len(load_ytvis_train(dst, str(tmp_path))) == len({a["video_id"] for a in want["annotations"]})


def _all_calls():
    from s2d_amd import coco_eval, plane_components, rle_ragged, selftrain, selftrain_video
    return {m.__name__: dict(m.LIB_CALLS) for m in (coco_eval, plane_components, rle_ragged, selftrain, selftrain_video)}


def _delta(a, b):
    return {m: {k: b[m].get(k, 0) - a[m].get(k, 0) for k in b[m] if b[m].get(k, 0) != a[m].get(k, 0)} for m in b}


def test_drivers_with_the_options_off_write_the_same_bytes_with_the_same_calls(tmp_path):
    import json
    from tests import selftrain_refs, selftrain_video_refs
    from s2d_amd import clean_annotations as C, selftrain, selftrain_video
    off = C.cleanup_options(C.build_parser().parse_args(["--ann", "a", "--save-path", "b"]))
    prev, preds = selftrain_refs.random_case(12, seed=0)
    vdoc, vpreds = selftrain_video_refs.merge_case()
    paths = {}
    for name, d in (("preds", preds), ("prev", prev), ("vpreds", vpreds), ("vdoc", vdoc)):
        paths[name] = str(tmp_path / f"{name}.json")
        with open(paths[name], "w") as fh:
            json.dump(d, fh)
    runs = []
    for cleanup in (None, off):
        tag = "plain" if cleanup is None else "off"
        c0 = _all_calls()
        a = selftrain.merge_files(paths["preds"], paths["prev"], str(tmp_path / f"img_{tag}.json"), device=DEV, cleanup=cleanup)
        b = selftrain_video.merge_files(paths["vpreds"], paths["vdoc"], str(tmp_path / f"vid_{tag}.json"), device=DEV, cleanup=cleanup)
        runs.append((a, b, _delta(c0, _all_calls()), open(tmp_path / f"img_{tag}.json", "rb").read(), open(tmp_path / f"vid_{tag}.json", "rb").read()))
    assert runs[0][0] == runs[1][0] == selftrain.merge_round(prev, preds, device=DEV)
    assert runs[0][1] == runs[1][1] == selftrain_video.merge_round(vdoc, vpreds, device=DEV)
    assert runs[0][2] == runs[1][2] and not runs[1][2]["s2d_amd.plane_components"]
    assert runs[0][3] == runs[1][3] and runs[0][4] == runs[1][4]
    # with an option on, the post-pass is clean_document over the merged document
    on = dict(off, min_component_area=3)
    got = selftrain_video.merge_files(paths["vpreds"], paths["vdoc"], str(tmp_path / "vid_on.json"), device=DEV, cleanup=on)
    assert json.dumps(got) == json.dumps(R.ref_clean_document(runs[0][1], **on)[0])
    got = selftrain.merge_files(paths["preds"], paths["prev"], str(tmp_path / "img_on.json"), device=DEV, cleanup=on)
    want, _ = R.ref_clean_document(runs[0][0], area_rule="bbox", decode=lambda s, H, W: selftrain_refs.seg_mask(s, H, W).astype(bool), **on)
    assert json.dumps(got) == json.dumps(want)
