"""The video self-training merge without a GPU: the restatement of tests/selftrain_video_refs.py against ytvis_eval's host-side
integer rule, its named cases and ordering rules, results_to_annotations.convert on the prediction-only part, and the host logic of
s2d_amd.selftrain_video (planning, chunking, assembly, refusals) with the restatement's numpy device_fn in place of the device."""
import copy
import json

import numpy as np
import pytest
import torch

from tests import selftrain_refs as R
from tests import selftrain_video_refs as V


@pytest.fixture(scope="module")
def kernel_case():
    return V.kernel_case()


@pytest.fixture(scope="module")
def merge_case():
    doc, preds = V.merge_case()
    return doc, preds, V.reference_merge(doc, preds)


def _packed(tracks, H, W):
    return torch.from_numpy(np.stack([R.pack_bits(m) for tr in tracks for m in V.track_masks(tr, H, W)]).view(np.int32))


def test_all_frames_equal_the_ytvis_evaluators_integer_rule(kernel_case, monkeypatch):
    """ytvis_eval._track_ious with its two device calls replaced by popcounts of the same packed planes: its quotient is
    inter / union of the restatement under `all`, and 0 where the union is 0"""
    from s2d_amd import ytvis_eval
    pop = lambda b: np.array([bin(int(w)).count("1") for w in b.numpy().view(np.uint32).reshape(-1)]).reshape(b.shape).sum(-1)   # noqa: E731
    monkeypatch.setattr(ytvis_eval, "plane_areas", lambda bits: torch.from_numpy(pop(bits).astype(np.int32)))
    monkeypatch.setattr(ytvis_eval, "cross_counts", lambda a, b: torch.from_numpy(
        np.array([[pop(x & y) for y in b] for x in a], np.int64).reshape(a.shape[0], b.shape[0])))
    items, names = kernel_case
    seen = 0
    for it in items:
        D, G = len(it.dsegs), len(it.gsegs)
        if not (D and G):
            continue
        ious, _ = ytvis_eval._track_ious(_packed(it.dsegs, it.H, it.W), D, _packed(it.gsegs, it.H, it.W), G, it.T)
        inter, union = V.chunk_counts([it], "all")
        want = np.array([i / u if u > 0 else 0.0 for i, u in zip(inter, union)]).reshape(D, G)
        assert np.array_equal(ious, want), it.vid
        seen += D * G
    assert seen >= 9 * 17


def test_named_cases_have_their_property(kernel_case):
    items, names = kernel_case
    for name, (frames, kept_annotated, kept_all) in V.NAMED_TUBES.items():
        it = items[names[name]]
        (i, u), (ia, ua) = V.tube_counts(it.dsegs[0], it.gsegs[0], it.H, it.W, "annotated"), V.tube_counts(it.dsegs[0], it.gsegs[0], it.H, it.W, "all")
        assert (2 * i < u) == kept_annotated and (2 * ia < ua) == kept_all, name
        if name.startswith("half"):
            assert 2 * i == u
        if name.startswith("below"):
            assert 2 * i == u - 1
    big = items[names["big"]]
    assert (len(big.dsegs), len(big.gsegs)) == (9, 17)
    assert all(s is None for s in big.dsegs[3])                                    # a track with no annotated frame: union 0, dropped
    assert all(V.tube_counts(big.dsegs[3], q, big.H, big.W, "annotated") == (0, 0) for q in big.gsegs)
    assert not V.keep_track(big.dsegs[3], big.gsegs, big.H, big.W, "annotated")
    assert big.dsegs[1][1] is None and big.gsegs[1][1] is None and big.dsegs[2][2] is None and big.gsegs[2][2] is None
    ia, ua = V.chunk_counts([big], "annotated")
    il, ul = V.chunk_counts([big], "all")
    assert ia == il and ua != ul and all(a <= b for a, b in zip(ua, ul))           # an empty P plane meets nothing: only the union grows
    assert V.keep_track(items[2].dsegs[0], [], 5, 7, "annotated")                 # G == 0: kept
    assert not V.keep_track(items[0].dsegs[0], items[0].gsegs, 1, 1, "all")


def test_reference_merge_ordering_and_fields(merge_case):
    doc, preds, want = merge_case
    anns = want["annotations"]
    assert [a["id"] for a in anns] == list(range(1, len(anns) + 1))
    prev_order = list(dict.fromkeys(a["video_id"] for a in doc["annotations"]))
    assert prev_order[0] == 7
    kept = [p for p in preds if p["score"] >= 0.75 and p["video_id"] != 99]
    only_pred = [v for v in dict.fromkeys(p["video_id"] for p in kept) if v not in prev_order]
    assert only_pred == [3]
    assert list(dict.fromkeys(a["video_id"] for a in anns)) == prev_order + only_pred
    for vid in prev_order + only_pred:
        mine = [a for a in anns if a["video_id"] == vid]
        n_pred = sum(p["video_id"] == vid for p in kept)
        assert [a["segmentations"] for a in mine[:n_pred]] == [p["segmentations"] for p in kept if p["video_id"] == vid]
        assert all("score" in a for a in mine[:n_pred]) and not any("score" in a for a in mine[n_pred:])
        prev_ids = [a["segmentations"] for a in doc["annotations"] if a["video_id"] == vid]
        pos = [prev_ids.index(a["segmentations"]) for a in mine[n_pred:]]
        assert pos == sorted(pos)
    by = lambda vid: [a for a in anns if a["video_id"] == vid]                     # noqa: E731
    assert len(by(4)) == sum(a["video_id"] == 4 for a in doc["annotations"])       # previous tracks only: all kept
    assert len(by(5)) == sum(a["video_id"] == 5 for a in doc["annotations"])       # low scores only: as previous only
    assert any(p["score"] == 0.75 for p in kept) and not any(a["video_id"] == 99 for a in anns)
    n_prev_kept = sum("score" not in a for a in anns)
    assert 0 < n_prev_kept < len(doc["annotations"])                               # some previous tracks survive, some are covered
    assert len(V.reference_merge(doc, preds, frames="all")["annotations"]) > len(anns)   # all-frame IoU keeps keymasks beside their duplicates


def test_prediction_only_part_is_what_convert_writes(merge_case):
    from s2d_amd.keymask.results_to_annotations import convert
    doc, preds, _ = merge_case
    empty = dict(doc, annotations=[])
    want, low = convert(empty, doc, preds, 0.75, bbox_area_fn=V.numpy_bbox_area)
    got = V.reference_merge(empty, preds)
    assert low == sum(p["score"] < 0.75 for p in preds) and len(got["annotations"]) == len(want["annotations"]) > 5
    for w in want["annotations"]:                                                  # convert keeps file order; the merge groups by video
        g = dict(next(a for a in got["annotations"] if a["segmentations"] is w["segmentations"]))
        assert g.pop("score") >= 0.75
        g.pop("id"), w.pop("id")
        assert g == w
    assert {k: got[k] for k in ("info", "licenses", "videos", "categories")} == {k: want[k] for k in ("info", "licenses", "videos", "categories")}


def test_module_host_logic_equals_the_restatement(merge_case, tmp_path, monkeypatch):
    from s2d_amd import coco_eval, selftrain_video as S
    doc, preds, want = merge_case
    before = copy.deepcopy((doc, preds))
    for frames in S.FRAME_SETS:
        assert S.merge_round(doc, preds, frames=frames, device_fn=V.numpy_device) == V.reference_merge(doc, preds, frames=frames)
    assert (doc, preds) == before                                                  # the inputs are not modified
    gt = {"info": {"description": "gt"}, "videos": [v for v in doc["videos"] if v["id"] != 3]}    # video 3's predictions are skipped
    with_gt = S.merge_round(doc, preds, gt, device_fn=V.numpy_device)
    assert with_gt == V.reference_merge(doc, preds, gt) and "licenses" not in with_gt and with_gt["info"] == gt["info"]
    assert with_gt["videos"] is gt["videos"] and not any(a["video_id"] == 3 for a in with_gt["annotations"])
    with pytest.raises(ValueError, match="video 2"):                               # a previous track of a video `videos` lacks
        S.merge_round(doc, preds, {"videos": [v for v in doc["videos"] if v["id"] != 2]}, device_fn=V.numpy_device)
    paths = [str(tmp_path / n) for n in ("results.json", "round0.json", "round1.json")]
    for p, d in zip(paths, (preds, doc)):
        with open(p, "w") as fh:
            json.dump(d, fh)
    seconds = {}
    got = S.merge_files(paths[0], paths[1], paths[2], device_fn=V.numpy_device, seconds=seconds)
    with open(paths[2]) as fh:
        assert json.load(fh) == json.loads(json.dumps(want)) and got == want
    assert {"json", "assemble"} <= set(seconds)
    # chunking: a small bound cuts the chunks and sends the videos over it through slabs of frames; the document is the same
    chunks = []
    monkeypatch.setattr(coco_eval, "CHUNK_WORDS", 400)
    fn = lambda c, fr: (chunks.append(c), V.numpy_device(c, fr))[1]                # noqa: E731
    assert S.merge_round(doc, preds, device_fn=fn) == want
    slabbed = [c for c in chunks if c.slabs]
    assert len(chunks) > 3 and slabbed and all(len(c.items) == 1 for c in slabbed)
    for c in slabbed:
        assert [a for a, _ in c.slabs] == [0] + [b for _, b in c.slabs][:-1] and c.slabs[-1][1] == c.items[0].T and len(c.slabs) > 1


def test_module_refusals_name_the_video(merge_case):
    from s2d_amd import selftrain_video as S
    doc, preds, _ = merge_case
    kept = next(k for k, p in enumerate(preds) if p["score"] >= 0.75 and p["video_id"] == 6)
    bad = copy.deepcopy(preds)
    bad[kept]["segmentations"] = bad[kept]["segmentations"][:-1]
    with pytest.raises(ValueError, match="video 6"):
        S.merge_round(doc, bad, device_fn=V.numpy_device)
    bad = copy.deepcopy(preds)
    seg = next(s for s in bad[kept]["segmentations"] if s is not None)
    seg["size"] = [seg["size"][1], seg["size"][0]]
    with pytest.raises(ValueError, match="video 6"):
        S.merge_round(doc, bad, device_fn=V.numpy_device)
    bad = copy.deepcopy(preds)
    bad[kept]["category_id"] = 2
    with pytest.raises(ValueError, match="video 6.*category_id 2"):
        S.merge_round(doc, bad, device_fn=V.numpy_device)
    low = copy.deepcopy(preds)
    k5 = next(k for k, p in enumerate(low) if p["video_id"] == 5)
    low[k5]["segmentations"] = []                                                  # below the threshold: never looked at
    S.merge_round(doc, low, device_fn=V.numpy_device)
    with pytest.raises(ValueError, match="frames"):
        S.merge_round(doc, preds, frames="some", device_fn=V.numpy_device)
    with pytest.raises(SystemExit):
        S.main(["--results-file", "a", "--prev-ann", "b", "--save-path", "c", "--frames", "some"])
