"""GPU checks of the video self-training merge: the tube-count and keep kernels (csrc/selftrain_video.hip) and the ragged plane areas
against the restatement of tests/selftrain_video_refs.py, on one chunk of videos of different sizes and lengths; the slab path; the
call count; the refusals; merge_round / merge_files / main against the restated tool; the written file through the training
loader.  All comparisons are equalities."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import selftrain_refs as R
from tests import selftrain_video_refs as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def kernel_case():
    """(items, names, {frames: (inter, union, keep)}, areas, boxes): built and referenced once, left unchanged"""
    items, names = V.kernel_case()
    chunk = _chunk(items)
    want = {}
    for frames in ("annotated", "all"):
        keep, areas, boxes = V.numpy_device(chunk, frames)
        want[frames] = V.chunk_counts(items, frames) + (keep,)
    return items, names, want, areas, boxes


def _chunk(items, slabs=None):
    from types import SimpleNamespace
    return SimpleNamespace(items=items, slabs=slabs)


def _calls():
    from s2d_amd import rle_ragged, selftrain_video as S
    own = sum(v for k, v in S.LIB_CALLS.items() if k.startswith("s2d_"))
    return own + sum(rle_ragged.LIB_CALLS.values()), S.LIB_CALLS["readbacks"]


@pytest.mark.parametrize("frames", ["annotated", "all"])
def test_kernel_rows_equal_the_restatement(kernel_case, frames):
    from s2d_amd import selftrain_video as S
    items, names, want, want_areas, want_boxes = kernel_case
    inter, union, want_keep = want[frames]
    counts, again = {}, {}
    calls0, reads0 = _calls()
    keep, areas, boxes = S.device_merge(_chunk(items), frames, DEV, counts=counts)
    calls, reads = _calls()
    assert (calls - calls0, reads - reads0) == (6, 1)                             # parse, decode, boxes, areas, counts, keep; one read-back
    assert counts["inter"].dtype == np.int64 and len(inter) == 1 * 2 + 9 * 17 + 4 + 2 * 3 + 1
    for row, (gi, gu, wi, wu) in enumerate(zip(counts["inter"].tolist(), counts["union"].tolist(), inter, union)):
        assert (gi, gu) == (wi, wu), (frames, row)
    assert keep.dtype == np.int32 and keep.tolist() == want_keep.tolist()
    assert areas.tolist() == want_areas.tolist() and np.array_equal(boxes, want_boxes)
    keep2, areas2, boxes2 = S.device_merge(_chunk(items), frames, DEV, counts=again)             # a second call: bitwise equal
    assert np.array_equal(again["inter"], counts["inter"]) and np.array_equal(again["union"], counts["union"])
    assert np.array_equal(keep2, keep) and np.array_equal(areas2, areas) and np.array_equal(boxes2, boxes)
    d0 = np.cumsum([0] + [len(it.dsegs) for it in items])
    for name, (_, kept_annotated, kept_all) in V.NAMED_TUBES.items():
        assert bool(keep[d0[names[name]]]) == (kept_annotated if frames == "annotated" else kept_all), name
    big = d0[names["big"]]
    assert bool(keep[big + 3]) == (frames == "all")                               # no annotated frame: union 0 under `annotated`
    assert keep[0] == 0 and keep[1:3].tolist() == [1, 1]                          # 1 x 1 identical: dropped; G == 0: kept


def test_all_frames_equal_the_ytvis_evaluators_counts(kernel_case):
    """ytvis_eval._track_ious on the same planes: its float64 quotient of exact integers is inter / union of the kernel's rows"""
    from s2d_amd import selftrain_video as S, ytvis_eval
    items, names, _, _, _ = kernel_case
    counts = {}
    S.device_merge(_chunk(items), "all", DEV, counts=counts)
    row = 0
    for k, it in enumerate(items):
        D, G = len(it.dsegs), len(it.gsegs)
        if D and G and k in (names["big"], names["half"], names["below_dense"]):
            db = ytvis_eval.decode_frames([s for tr in it.dsegs for s in tr], it.H, it.W, device=DEV)
            gb = ytvis_eval.decode_frames([s for tr in it.gsegs for s in tr], it.H, it.W, device=DEV)
            ious, _ = ytvis_eval._track_ious(db, D, gb, G, it.T)
            i, u = counts["inter"][row:row + D * G].reshape(D, G), counts["union"][row:row + D * G].reshape(D, G)
            assert (u > 0).all() and np.array_equal(ious, i / u), it.vid
        row += D * G
    assert row == len(counts["inter"])


def _raw_counts(bits, vids, tiles, present, max_tw, n_pairs, accumulate=0, inter=None, union=None):
    from s2d_amd._lib import lib
    b = torch.from_numpy(bits.view(np.int32)).to(DEV)
    v, t, p = torch.from_numpy(vids).to(DEV), torch.from_numpy(tiles).to(DEV), torch.from_numpy(present).to(DEV)
    inter = torch.full((n_pairs,), -1, device=DEV, dtype=torch.int64) if inter is None else inter
    union = torch.full((n_pairs,), -1, device=DEV, dtype=torch.int64) if union is None else union
    lib().call("s2d_tube_counts_ragged", b, b.numel(), v, len(vids), p, p.numel(), t, len(tiles), max_tw, inter, union, n_pairs, accumulate, None)
    torch.cuda.synchronize()
    return inter, union


def test_tail_bits_of_the_last_word_are_not_counted():
    """planes of 35 pixels whose second word carries set bits at and beyond bit 3, on either side and on both: the counts are those
    of the clean planes; and `accumulate` adds a second pass on top of the first"""
    rng = np.random.default_rng(2)
    H, W, T = 5, 7, 2
    masks = rng.random((2, T, H, W)) < 0.5                                        # one P-side and one Q-side track
    clean = np.concatenate([R.pack_bits(m) for side in masks for m in side])
    want_i = int((masks[0] & masks[1]).sum())
    want_u = int(masks[0].sum() + masks[1].sum()) - want_i
    vids = np.array([[0, 4, 2, 35, T, 1, 1, 0, 0, 0, 0]], np.int64)
    tiles, present = np.zeros((1, 3), np.int32), np.ones(T, np.uint8)
    for dirty_words in ([1], [7], [1, 3, 5, 7]):
        bits = clean.copy()
        bits[dirty_words] |= np.uint32(0xFFFFFFF8)
        inter, union = _raw_counts(bits, vids, tiles, present, 4, 1)
        assert (inter.item(), union.item()) == (want_i, want_u), dirty_words
    inter, union = _raw_counts(clean, vids, tiles, present, 4, 1, accumulate=1, inter=inter, union=union)
    assert (inter.item(), union.item()) == (2 * want_i, 2 * want_u)


def test_slab_path_equals_the_one_call_result(kernel_case, monkeypatch):
    from s2d_amd import coco_eval, selftrain_video as S
    items, names, want, _, _ = kernel_case
    big = items[names["big"]]                                                     # 26 tracks x 5 frames x 32 words
    item = copy.copy(big)
    whole = next(S._chunks([item]))
    assert whole.slabs is None
    monkeypatch.setattr(coco_eval, "CHUNK_WORDS", 26 * 32 * 2)                    # two frames a slab: slabs of 2, 2 and 1 frames
    slabbed = next(S._chunks([item]))
    assert slabbed.slabs == [(0, 2), (2, 4), (4, 5)]
    for frames in ("annotated", "all"):
        one, cut = {}, {}
        k1, a1, b1 = S.device_merge(whole, frames, DEV, counts=one)
        calls0, reads0 = _calls()
        k2, a2, b2 = S.device_merge(slabbed, frames, DEV, counts=cut)
        calls, reads = _calls()
        assert (calls - calls0, reads - reads0) == (3 * 5 + 1, 1)
        assert np.array_equal(one["inter"], cut["inter"]) and np.array_equal(one["union"], cut["union"])
        assert np.array_equal(k1, k2) and np.array_equal(a1, a2) and np.array_equal(b1, b2)
        lo = 2
        assert one["inter"].tolist() == want[frames][0][lo:lo + 9 * 17] and one["union"].tolist() == want[frames][1][lo:lo + 9 * 17]


def test_call_count_does_not_depend_on_the_number_of_videos():
    from s2d_amd import selftrain_video as S
    spent = []
    for n in (3, 30):
        items = V.many_videos(n)
        calls0, reads0 = _calls()
        keep, _, _ = S.device_merge(_chunk(items), "annotated", DEV)
        calls, reads = _calls()
        spent.append((calls - calls0, reads - reads0))
        assert keep.tolist() == V.numpy_device(_chunk(items), "annotated")[0].tolist()
    assert spent == [(6, 1), (6, 1)]


def test_calls_refuse_bad_arguments_and_leave_the_outputs_alone():
    from s2d_amd._lib import lib
    L, ptr = lib(), lambda t: t.data_ptr()                                        # noqa: E731
    bits = torch.zeros((8,), device=DEV, dtype=torch.int32)
    vids = torch.tensor([[0, 4, 2, 35, 2, 1, 1, 0, 0, 0, 0]], device=DEV, dtype=torch.int64)
    tiles = torch.zeros((1, 3), device=DEV, dtype=torch.int32)
    present = torch.ones((2,), device=DEV, dtype=torch.uint8)
    inter = torch.full((1,), -5, device=DEV, dtype=torch.int64)
    union, keep, area = inter.clone(), torch.full((1,), -5, device=DEV, dtype=torch.int32), torch.full((4,), -5, device=DEV, dtype=torch.int32)
    plane = torch.tensor([[0, 5, 7, 0], [2, 5, 7, 0], [4, 5, 7, 0], [6, 5, 7, 0]], device=DEV, dtype=torch.int64)
    cnt = [ptr(bits), 8, ptr(vids), 1, ptr(present), 2, ptr(tiles), 1, 4, ptr(inter), ptr(union), 1, 0, None]
    for k in (0, 2, 4, 6, 9, 10):                                                 # every pointer null in turn
        assert L._raw_s2d_tube_counts_ragged(*(cnt[:k] + [None] + cnt[k + 1:])) == -1, k
    for k in (1, 3, 5, 7, 8, 11):                                                 # every count negative in turn
        assert L._raw_s2d_tube_counts_ragged(*(cnt[:k] + [-1] + cnt[k + 1:])) == -1, k
    kp = [ptr(inter), ptr(union), 1, ptr(vids), 1, ptr(keep), 1, None]
    for k in (0, 1, 3, 5):
        assert L._raw_s2d_selftrain_keep_tube_ragged(*(kp[:k] + [None] + kp[k + 1:])) == -1, k
    for k in (2, 4, 6):
        assert L._raw_s2d_selftrain_keep_tube_ragged(*(kp[:k] + [-1] + kp[k + 1:])) == -1, k
    ar = [ptr(bits), ptr(plane), 4, 8, ptr(area), None]
    for k in (0, 1, 4):
        assert L._raw_s2d_mask_plane_areas_ragged_u32(*(ar[:k] + [None] + ar[k + 1:])) == -1, k
    for k in (2, 3):
        assert L._raw_s2d_mask_plane_areas_ragged_u32(*(ar[:k] + [-1] + ar[k + 1:])) == -1, k
    # count 0: a no-op that succeeds, null pointers and all
    assert L._raw_s2d_tube_counts_ragged(None, 0, None, 0, None, 0, None, 0, 0, None, None, 0, 0, None) == 0
    assert L._raw_s2d_tube_counts_ragged(*(cnt[:11] + [0] + cnt[12:])) == 0
    assert L._raw_s2d_selftrain_keep_tube_ragged(None, None, 0, None, 0, None, 0, None) == 0
    assert L._raw_s2d_mask_plane_areas_ragged_u32(None, None, 0, 0, None, None) == 0
    torch.cuda.synchronize()
    assert inter.item() == union.item() == keep.item() == -5 and (area == -5).all()
    # a table row that does not fit the buffers it names is skipped: outputs zeroed by the call, nothing counted
    bad = vids.clone()
    bad[0, 1] = 6                                                                 # the Q-side track would end past the buffer
    assert L._raw_s2d_tube_counts_ragged(*(cnt[:2] + [ptr(bad)] + cnt[3:])) == 0
    torch.cuda.synchronize()
    assert inter.item() == union.item() == 0


@pytest.fixture(scope="module")
def merge_case(tmp_path_factory):
    root = tmp_path_factory.mktemp("selftrain_video")
    doc, preds = V.merge_case()
    want = {fr: V.reference_merge(doc, preds, frames=fr) for fr in ("annotated", "all")}
    paths = (str(root / "results.json"), str(root / "round0.json"))
    for p, d in zip(paths, (preds, doc)):
        with open(p, "w") as fh:
            json.dump(d, fh)
    return root, paths, doc, preds, want


def test_merge_equals_the_restated_tool(merge_case, monkeypatch, capsys):
    from s2d_amd import coco_eval, selftrain_video as S
    root, (res, ann), doc, preds, want = merge_case
    for frames in ("annotated", "all"):
        assert S.merge_round(doc, preds, frames=frames, device=DEV) == want[frames]
    out = str(root / "round1.json")
    reads0, chunks0 = S.LIB_CALLS["readbacks"], S.LIB_CALLS["chunks"]
    got = S.merge_files(res, ann, out, device=DEV)
    assert (S.LIB_CALLS["readbacks"] - reads0, S.LIB_CALLS["chunks"] - chunks0) == (1, 1)
    with open(out) as fh:
        assert json.load(fh) == json.loads(json.dumps(want["annotated"])) and got == want["annotated"]
    kinds = {("score" in a) for a in got["annotations"]}
    assert kinds == {True, False} and len(want["all"]["annotations"]) > len(got["annotations"])
    out2 = str(root / "round1_main.json")
    S.main(["--results-file", res, "--prev-ann", ann, "--save-path", out2, "--gt-annotation-file", ann, "--frames", "all"])
    assert capsys.readouterr().out.strip().endswith(f"Done: 12 videos; {len(want['all']['annotations'])} anns.")
    with open(out2) as fh:
        assert json.load(fh) == json.loads(json.dumps(want["all"]))
    monkeypatch.setattr(coco_eval, "CHUNK_WORDS", 400)                            # several chunks, some videos in slabs
    chunks0 = S.LIB_CALLS["chunks"]
    assert S.merge_round(doc, preds, device=DEV) == want["annotated"] and S.LIB_CALLS["chunks"] - chunks0 > 3


def test_wrong_size_and_wrong_length_raise_by_name(merge_case):
    from s2d_amd import selftrain_video as S
    _, _, doc, preds, _ = merge_case
    kept = next(k for k, p in enumerate(preds) if p["score"] >= 0.75 and p["video_id"] == 6)
    bad = copy.deepcopy(preds)
    bad[kept]["segmentations"].append(None)
    with pytest.raises(ValueError, match="video 6"):
        S.merge_round(doc, bad, device=DEV)
    bad = copy.deepcopy(preds)
    seg = next(s for s in bad[kept]["segmentations"] if s is not None)
    seg["size"] = [seg["size"][0] + 1, seg["size"][1]]
    with pytest.raises(ValueError, match="video 6"):
        S.merge_round(doc, bad, device=DEV)


def test_written_file_parses_through_the_training_loader(merge_case):
    from s2d_amd.data.train_loader import load_ytvis_train
    from s2d_amd.data.image_clip import detect_train_format                   # what s2d_amd.train decides the loader by
    root, _, doc, preds, want = merge_case
    out = str(root / "round1.json")
    if not os.path.exists(out):
        from s2d_amd import selftrain_video as S
        S.merge_files(str(root / "results.json"), str(root / "round0.json"), out, device=DEV)
    with open(out) as fh:
        written = json.load(fh)
    assert detect_train_format(written) == "ytvis"
    records = load_ytvis_train(out, str(root))
    assert [r["video_id"] for r in records] == sorted(a for a in {a["video_id"] for a in want["annotated"]["annotations"]})
    for r in records:
        mine = [a for a in want["annotated"]["annotations"] if a["video_id"] == r["video_id"]]
        for t, objs in enumerate(r["annotations"]):
            assert [o["id"] for o in objs] == [a["id"] for a in mine if a["segmentations"][t] and a["bboxes"][t]]
            for o in objs:
                a = next(a for a in mine if a["id"] == o["id"])
                assert o["segmentation"] == json.loads(json.dumps(a["segmentations"][t]))
