"""The image self-training merge without a device: merge_round's host logic against the restated tool, the integer keep rule against
the reference's float32 comparison, the refusals, and the host staging of the ragged RLE decode."""
import copy

import numpy as np
import pytest

from tests.selftrain_refs import (NAMED_PAIRS, SIZES, compress, counts_of, f32_keep, named_case, numpy_keep, pair, random_case,
                                  reference_merge, rle_c, rle_u)


def test_merge_round_equals_the_restated_tool_on_hand_built_documents():
    from s2d_amd.data.image_clip import load_coco_image_train
    from s2d_amd.selftrain import merge_round
    prev, preds = named_case()
    before = copy.deepcopy((prev, preds))
    doc = merge_round(prev, preds, keep_fn=numpy_keep)
    assert doc == reference_merge(prev, preds)
    assert (prev, preds) == before                                        # inputs are not modified
    anns = doc["annotations"]
    assert [a["id"] for a in anns] == list(range(1, len(anns) + 1))
    assert all(a["iscrowd"] == 0 and a["area"] == a["bbox"][2] * a["bbox"][3] for a in anns)
    size = {im["id"]: (im["height"], im["width"]) for im in prev["images"]}
    assert all((a["width"], a["height"]) == size[a["image_id"]] for a in anns)            # swapped: width = size[0] = the height
    assert doc["images"] is prev["images"] and doc["info"] == prev["info"] and "licenses" not in doc
    # order: image 7 (first among the annotations) with its predictions first; then the named pairs; 3, 8; then prediction-only image 2
    ids = [a["image_id"] for a in anns]
    first = [ids.index(i) for i in dict.fromkeys(ids)]
    assert list(dict.fromkeys(ids)) == [7] + [10 + k for k in range(len(NAMED_PAIRS))] + [3, 8, 2] and first == sorted(first)
    seven = [a for a in anns if a["image_id"] == 7]
    assert [("score" in a) for a in seven] == [True, True, False, False]                 # 2 kept predictions, then previous 1 and 3
    assert [a["score"] for a in seven[:2]] == [0.9, 0.75] and seven[1]["bbox"] == [5, 5, 5, 5]
    assert all(isinstance(v, float) for v in seven[0]["bbox"])                            # filled from the mask
    for k, (name, (_, _, _, kept)) in enumerate(NAMED_PAIRS.items()):
        got = [a for a in anns if a["image_id"] == 10 + k]
        assert len(got) == 1 + kept and "score" in got[0], name                           # a score equal to the threshold is kept
        assert ("score" not in got[-1]) == kept, name
    assert [("score" in a) for a in anns if a["image_id"] == 8] == [False]                # its prediction is below the threshold
    assert len([a for a in anns if a["image_id"] == 3]) == 3 and [a for a in anns if a["image_id"] == 3][1]["bbox"] == [1.0, 2.0, 3.0, 4.0]
    recs = load_coco_image_train(doc, "/images")
    assert len(recs) == len(set(ids)) and sum(len(r["annotations"]) for r in recs) == len(anns)


def test_merge_round_on_random_documents_and_without_categories():
    from s2d_amd.selftrain import merge_round
    prev, preds = random_case(24, seed=3)
    del prev["categories"]
    doc = merge_round(prev, preds, threshold=0.8, keep_fn=numpy_keep)
    assert doc == reference_merge(prev, preds, 0.8)
    assert doc["categories"] == [{"id": 1, "name": "fg", "supercategory": "fg"}] and len(doc["annotations"]) > 30


def test_integer_rule_equals_float32_comparison_around_one_half():
    from s2d_amd.selftrain import keep_rule
    us = np.array([1, 2, 3, 4, 5, 6, 7, 8, 999, 1000, 65535, 65536, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1], np.int64)
    rng = np.random.default_rng(0)
    us = np.concatenate([us, rng.integers(1, 1 << 24, 4000), (1 << 24) - 1 - rng.integers(0, 4000, 2000)])
    cases = []
    for half in (us // 2, (us + 1) // 2):
        for delta in (-1, 0, 1):
            i = half + delta
            ok = (i >= 0) & (i <= us)
            cases.append(np.stack([i[ok], us[ok]], 1))
    cases = np.concatenate(cases)
    i, u = cases[:, 0], cases[:, 1]
    want = i.astype(np.float32) / u.astype(np.float32) < np.float32(0.5)
    # one previous mask of u pixels against one prediction that is its subset of i pixels: union = u
    got = np.array([keep_rule([[a]], [b], [a])[0] for a, b in zip(i.tolist(), u.tolist())])
    assert np.array_equal(got, want) and want.any() and not want.all()
    assert np.array_equal(got, 2 * i < u)
    # several predictions: every one must stay below one half; none: kept; union 0: dropped, as NaN < 0.5
    assert keep_rule([[1, 0], [2, 0]], [4, 4], [2, 3]).tolist() == [True, False]
    assert keep_rule(np.zeros((2, 0)), [0, 5], []).tolist() == [True, True]
    assert keep_rule([[0]], [0], [0]).tolist() == [False] and f32_keep([[0]], [0], [0]).tolist() == [False]


@pytest.mark.parametrize("what", ["size", "size_pred", "absent_image", "absent_image_ann", "no_segmentation", "empty_polygons", "category"])
def test_refusals_name_the_image(what):
    from s2d_amd.selftrain import merge_round
    prev, preds = named_case()
    if what == "size":
        prev["annotations"][0]["segmentation"]["size"] = [300, 37]
        iid = prev["annotations"][0]["image_id"]
    elif what == "size_pred":
        preds[0]["segmentation"] = dict(preds[0]["segmentation"], size=[4, 254])
        iid = preds[0]["image_id"]
    elif what == "absent_image":
        preds[1]["image_id"] = iid = 777
    elif what == "absent_image_ann":
        prev["annotations"][2]["image_id"] = iid = 778
    elif what == "no_segmentation":
        del preds[0]["segmentation"]
        iid = preds[0]["image_id"]
    elif what == "empty_polygons":
        prev["annotations"][1]["segmentation"] = []
        iid = prev["annotations"][1]["image_id"]
    else:
        preds[0]["category_id"] = 4
        iid = preds[0]["image_id"]
    with pytest.raises(ValueError, match=f"image {iid}\\b"):
        merge_round(prev, preds, keep_fn=numpy_keep)


def test_a_low_score_prediction_for_an_absent_image_is_not_read():
    from s2d_amd.selftrain import merge_round
    prev, preds = named_case()
    preds.append({"image_id": 999, "category_id": 1, "score": 0.2, "segmentation": None})
    assert merge_round(prev, preds, keep_fn=numpy_keep) == reference_merge(prev, preds[:-1])


def test_chunks_respect_both_limits(monkeypatch):
    from s2d_amd import selftrain
    prev, preds = random_case(24, seed=1)
    want = reference_merge(prev, preds)
    sizes = []

    def spy(chunk):
        sizes.append((len(chunk.items), sum((len(s) * ((H * W + 31) // 32)) for s, (H, W) in zip(chunk.segs, chunk.sizes))))
        assert all(len(s) == d + g > 0 for s, d, g in zip(chunk.segs, chunk.Ds, chunk.Gs))
        return numpy_keep(chunk)

    monkeypatch.setattr(selftrain, "CHUNK_IMAGES", 5)
    assert selftrain.merge_round(prev, preds, keep_fn=spy) == want
    assert max(n for n, _ in sizes) == 5 and len(sizes) >= 4
    sizes.clear()
    monkeypatch.setattr(selftrain, "CHUNK_IMAGES", 1024)
    monkeypatch.setattr(selftrain, "CHUNK_WORDS", 2000)
    assert selftrain.merge_round(prev, preds, keep_fn=spy) == want
    assert len(sizes) >= 3 and all(w <= 2000 or n == 1 for n, w in sizes)


def test_stage_rle_ragged_tables():
    from s2d_amd.rle_ragged import stage_rle_ragged
    from s2d_amd.ytvis_eval import stage_rle
    rng = np.random.default_rng(2)
    sizes = [(480, 640), (2, 31), (3, 256), (7, 65), (2, 257)]
    masks = [[rng.random((H, W)) < 0.4 for _ in range(k)] for (H, W), k in zip(sizes, (2, 3, 0, 4, 1))]
    segs = [[rle_c(m) if j % 2 else rle_u(m) for j, m in enumerate(ms)] for ms in masks]
    segs[1][1] = None                                                     # an absent plane
    segs[1][2] = {"size": [2, 31], "counts": [10, 40, 500]}              # runs past hw = 62, behind a 480 x 640 image
    segs[3][0] = [[0, 0, 4, 0, 4, 4, 0, 4]]                               # a polygon: no slots, listed for the fill
    s = stage_rle_ragged(segs, sizes)
    P = sum(len(x) for x in segs)
    assert s.P == P and s.N == 5 and s.plane0.tolist() == [0, 2, 5, 5, 9, 10]
    H = np.repeat([h for h, _ in sizes], [len(x) for x in segs])
    W = np.repeat([w for _, w in sizes], [len(x) for x in segs])
    wpp = (H * W + 31) // 32
    assert s.plane.dtype == np.int64 and s.plane.shape == (P, 4) and (s.plane[:, 3] == 0).all()
    assert np.array_equal(s.plane[:, 1], H) and np.array_equal(s.plane[:, 2], W)
    assert np.array_equal(s.plane[:, 0], np.cumsum(wpp) - wpp) and s.words == wpp.sum()
    # tiles: ceil(W / 256) column blocks per plane, each once, plane-major
    assert s.tiles.dtype == np.int32 and len(s.tiles) == int(((W + 255) // 256).sum())
    want_tiles = [(p, c) for p in range(P) for c in range((W[p] + 255) // 256)]
    assert [tuple(t) for t in s.tiles.tolist()] == want_tiles
    # per image the strings, slots and ends are stage_rle's (with that image's clamp), at the chunk's offsets
    flat = [x for im in segs for x in im]
    lens = [0 if not isinstance(x, dict) else len(x["counts"]) for x in flat]
    assert s.str_off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    for n, (im, (h, w)) in enumerate(zip(segs, sizes)):
        if not im:
            continue
        chars, off, ends, nrun = stage_rle([x if isinstance(x, dict) else None for x in im], h, w)
        p0, p1 = s.plane0[n], s.plane0[n + 1]
        a, b = s.str_off[p0], s.str_off[p1]
        assert np.array_equal(s.nrun[p0:p1], nrun) and np.array_equal(s.str_off[p0:p1 + 1] - a, off)
        assert np.array_equal(s.chars[a:b], chars[:b - a]) and np.array_equal(s.ends[a:b], ends[:b - a])
    q = 4                                                                 # the plane of the overlong counts
    assert s.ends[s.str_off[q]:s.str_off[q + 1]].tolist() == [10, 50, 62] and s.nrun[q] == 3
    assert s.nrun[3] == 0 and s.nrun[5] == 0 and s.polygons == [(3, [0], [segs[3][0]])]
    assert (s.nrun[[1, 6, 8]] == -1).all()                                  # compressed strings are left for the device
    with pytest.raises(ValueError, match="image seven: RLE of size"):
        stage_rle_ragged([[rle_c(masks[1][0])]], [(31, 2)], names=["seven"])
    with pytest.raises(ValueError, match="image 0"):
        stage_rle_ragged([[5]], [(3, 3)])
    e = stage_rle_ragged([], [])
    assert e.P == 0 and e.words == 0 and e.tiles.shape == (0, 2) and e.str_off.tolist() == [0]


def test_case_builders_are_consistent():
    for name, (i, ad, ag, kept) in NAMED_PAIRS.items():
        d, g = pair(4, 255, i, ad, ag)
        assert (int((d & g).sum()), int(d.sum()), int(g.sum())) == (i, ad, ag), name
        assert f32_keep([[i]], [ad], [ag])[0] == kept, name
    m = np.random.default_rng(0).random((SIZES[7][0], SIZES[7][1])) < 0.5
    from oracle import oracle_np
    assert compress(counts_of(m)).encode() == oracle_np.rle_encode(m)[0]["counts"]
