"""GPU checks of the image self-training merge: the ragged RLE parse / decode / tight-box calls (csrc/rle_ragged.hip) against the
per-image path and the numpy oracle, their refusals, the keep kernel against the numpy rule, `merge_files` against the restated tool
of tests/selftrain_refs.py, and the command line's output through the COCO image training mapper.  All comparisons are equalities."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import selftrain_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
DEV = "cuda:0"

# a plane with W % 32 != 0 follows one with W % 32 == 0 and the reverse; the small 2 x 257 image follows the large one
CHUNK_SIZES = [(1, 1), (3, 32), (1, 33), (5, 64), (37, 1), (2, 31), (3, 256), (5, 63), (7, 65), (480, 640), (2, 257), (4, 255), (37, 300)]


def _noise(H, W, rng, p=0.3):
    return rng.random((H, W)) < p


@pytest.fixture(scope="module")
def ragged_chunk():
    """(segs per image, sizes, expected masks per plane): built and referenced once, left unchanged"""
    rng = np.random.default_rng(11)
    segs = []
    for H, W in CHUNK_SIZES:
        hw = H * W
        if (H, W) == (3, 32):
            s = [R.rle_c(R.blob(H, W, rng)), None, {"size": [H, W], "counts": [0, hw]}]           # absent; all ones
        elif (H, W) == (5, 64):
            s = [R.rle_c(np.zeros((H, W), bool)), R.rle_u(_noise(H, W, rng))]                     # all zero; uncompressed counts
        elif (H, W) == (480, 640):
            m = R.blob(H, W, rng)
            m[rng.integers(0, H, 300), rng.integers(0, W, 300)] ^= True
            s = [R.rle_c(m), R.rle_u(R.blob(H, W, rng))]
        elif (H, W) == (2, 257):
            # counts that run past hw = 514 right behind the 480 x 640 image: a clamp with the wrong plane's size lets them through
            s = [{"size": [H, W], "counts": [5, 300, 1000]}, {"size": [H, W], "counts": R.compress([3, 200, 100000, 7])},
                 R.rle_c(_noise(H, W, rng))]
        elif (H, W) == (37, 300):
            s = [R.rle_c(_noise(H, W, rng)), R.rle_c(R.blob(H, W, rng)), {"size": [H, W], "counts": [0, hw]}]
        else:
            s = [R.rle_c(R.blob(H, W, rng)), R.rle_u(_noise(H, W, rng, 0.5))][:1 + (hw > 1)]
            if (H, W) == (7, 65):
                s.append(R.rle_c(_noise(H, W, rng, 0.1)))
        segs.append(s)
    assert len(segs[-1][0]["counts"]) > 64 and len(segs[9][0]["counts"]) > 64                     # a second parse step
    masks = [R.seg_mask(x, H, W) for s, (H, W) in zip(segs, CHUNK_SIZES) for x in s]
    assert len(masks) % 4 != 0
    return segs, CHUNK_SIZES, masks


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_ragged_decode_equals_the_per_image_path_and_the_oracle(ragged_chunk):
    from s2d_amd import rle_ragged
    from s2d_amd.ytvis_eval import decode_frames, plane_bboxes
    segs, sizes, masks = ragged_chunk
    staged = rle_ragged.stage_rle_ragged(segs, sizes)
    before = sum(rle_ragged.LIB_CALLS.values())
    out = rle_ragged.decode_ragged(staged, DEV)
    assert sum(rle_ragged.LIB_CALLS.values()) - before == 3               # parse, decode, bbox: whatever the chunk holds
    again = rle_ragged.decode_ragged(rle_ragged.stage_rle_ragged(segs, sizes), DEV)
    torch.cuda.synchronize()
    assert out.bits.shape == (staged.words,) and out.bbox.shape == (staged.P, 4)
    assert torch.equal(out.bits, again.bits) and torch.equal(out.bbox, again.bbox)
    flat, boxes = _u32(out.bits), out.bbox.cpu().numpy()
    p = 0
    for n, (s, (H, W)) in enumerate(zip(segs, sizes)):
        wpp = (H * W + 31) // 32
        want_bits = decode_frames(s, H, W, device=DEV)
        want_box = plane_bboxes(want_bits, H, W).cpu().numpy()
        want_bits = _u32(want_bits)
        for k in range(len(s)):
            w0 = int(staged.plane[p, 0])
            got = flat[w0:w0 + wpp]
            assert np.array_equal(got, want_bits[k]), (n, k, H, W)
            assert np.array_equal(got, R.pack_bits(masks[p])), (n, k, H, W)
            if (H * W) % 32:
                assert got[-1] >> np.uint32((H * W) % 32) == 0, (n, k)    # tail bits
            assert boxes[p].tolist() == want_box[k].tolist() == R.box_of(masks[p]), (n, k, H, W)
            p += 1
    assert p == staged.P and int(staged.plane[-1, 0]) + (37 * 300 + 31) // 32 == staged.words


def test_ragged_calls_refuse_bad_arguments_and_leave_the_buffer_alone():
    from s2d_amd import rle_ragged
    from s2d_amd._lib import lib
    rng = np.random.default_rng(0)
    staged = rle_ragged.stage_rle_ragged([[R.rle_c(R.blob(5, 63, rng)), R.rle_u(R.blob(5, 63, rng))], [R.rle_c(R.blob(3, 32, rng))]], [(5, 63), (3, 32)])
    chars, off, ends, nrun, plane, tiles = rle_ragged._upload([staged.chars, staged.str_off, staged.ends, staged.nrun, staged.plane, staged.tiles], DEV)
    P, T, words = staged.P, len(staged.tiles), staged.words
    bits = torch.full((words,), 0x5A5A5A5A, device=DEV, dtype=torch.int32)
    bbox = torch.full((P, 4), -7, device=DEV, dtype=torch.int32)
    nrun0, ends0 = nrun.clone(), ends.clone()
    L, ptr = lib(), lambda t: t.data_ptr()                                # noqa: E731
    dec = [ptr(ends), ptr(off), ptr(nrun), ptr(plane), P, ptr(tiles), T, ptr(bits), words, None]
    bad = []
    for k in (0, 1, 2, 3, 5, 7):                                          # every pointer null in turn
        bad.append(dec[:k] + [None] + dec[k + 1:])
    for k in (4, 6, 8):                                                   # every count negative in turn
        bad.append(dec[:k] + [-1] + dec[k + 1:])
    for args in bad:
        assert L._raw_s2d_rle_decode_ragged(*args) == -1, args
    par = [ptr(chars), ptr(off), ptr(plane), P, ptr(ends), ptr(nrun), None]
    for k in (0, 1, 2, 4, 5):
        assert L._raw_s2d_rle_parse_ragged(*(par[:k] + [None] + par[k + 1:])) == -1
    assert L._raw_s2d_rle_parse_ragged(*(par[:3] + [-1] + par[4:])) == -1
    box = [ptr(bits), ptr(plane), P, words, ptr(bbox), None]
    for k in (0, 1, 4):                                                   # 4: out == nullptr
        assert L._raw_s2d_mask_plane_bbox_ragged_u32(*(box[:k] + [None] + box[k + 1:])) == -1
    for k in (2, 3):
        assert L._raw_s2d_mask_plane_bbox_ragged_u32(*(box[:k] + [-1] + box[k + 1:])) == -1
    assert L._raw_s2d_selftrain_keep_ragged(None, None, None, None, 1, None, None) == -1
    assert L._raw_s2d_selftrain_keep_ragged(None, None, None, None, -1, None, None) == -1
    # P == 0 (N == 0): a no-op that succeeds
    assert L._raw_s2d_rle_decode_ragged(*(dec[:4] + [0] + dec[5:])) == 0
    assert L._raw_s2d_rle_parse_ragged(*(par[:3] + [0] + par[4:])) == 0
    assert L._raw_s2d_mask_plane_bbox_ragged_u32(*(box[:2] + [0] + box[3:])) == 0
    assert L._raw_s2d_selftrain_keep_ragged(None, None, None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert (bits == 0x5A5A5A5A).all() and (bbox == -7).all() and torch.equal(nrun, nrun0) and torch.equal(ends, ends0)
    e = rle_ragged.decode_ragged(rle_ragged.stage_rle_ragged([], []), DEV)
    assert e.bits.numel() == 0 and e.bbox.shape == (0, 4)


def _keep_chunk():
    H, W = 4, 255
    segs, Ds, Gs = [], [], []
    for i, ad, ag, _ in R.NAMED_PAIRS.values():
        d, g = R.pair(H, W, i, ad, ag)
        segs.append([R.rle_c(d), R.rle_c(g)]); Ds.append(1); Gs.append(1)
    rng = np.random.default_rng(4)
    d = R.pair(H, W, 0, 40, 0)[0]
    far = [R.pair(H, W, 0, 100 + 20 * k, 15)[1] for k in range(9)]       # 9 predictions away from d: more than one pair tile
    segs.append([R.rle_c(R.blob(H, W, rng)), R.rle_u(R.blob(H, W, rng))]); Ds.append(2); Gs.append(0)      # G == 0: kept
    segs.append([R.rle_c(R.blob(H, W, rng)), R.rle_u(R.blob(H, W, rng))]); Ds.append(0); Gs.append(2)      # D == 0
    segs.append([R.rle_c(d)] + [R.rle_c(m) for m in far]); Ds.append(1); Gs.append(9)                      # all below one half: kept
    segs.append([R.rle_c(d)] + [R.rle_c(m) for m in far[:8]] + [R.rle_u(d)]); Ds.append(1); Gs.append(9)   # the 9th is d itself: dropped
    segs.append([R.rle_c(m) for m in far] + [R.rle_c(far[8])]); Ds.append(9); Gs.append(1)                 # only the 9th previous mask dropped
    return SimpleNamespace(segs=segs, sizes=[(H, W)] * len(segs), Ds=Ds, Gs=Gs, names=list(range(len(segs))))


def test_keep_kernel_equals_the_numpy_rule():
    from s2d_amd.selftrain import device_keep
    chunk = _keep_chunk()
    keep, boxes = device_keep(chunk, DEV)
    want_keep, want_boxes = R.numpy_keep(chunk)
    assert keep.dtype == np.int32 and keep.tolist() == want_keep.tolist()
    assert np.array_equal(boxes, want_boxes)
    named = [bool(k) for k in keep[:len(R.NAMED_PAIRS)]]
    assert named == [kept for _, _, _, kept in R.NAMED_PAIRS.values()]
    assert keep[len(named):].tolist() == [1, 1] + [1] + [0] + [1] * 8 + [0]


@pytest.fixture(scope="module")
def merge_case(tmp_path_factory):
    root = tmp_path_factory.mktemp("selftrain")
    prev, preds = R.random_case(40, seed=0)
    want = R.reference_merge(prev, preds)
    paths = (str(root / "results.json"), str(root / "round0.json"))
    for p, d in zip(paths, (preds, prev)):
        with open(p, "w") as fh:
            json.dump(d, fh)
    return root, paths, prev, preds, want


def _calls():
    from s2d_amd import coco_eval, rle_ragged, selftrain
    return (sum(rle_ragged.LIB_CALLS.values()) + coco_eval.LIB_CALLS["s2d_coco_mask_iou_ragged"]
            + selftrain.LIB_CALLS["s2d_selftrain_keep_ragged"]), selftrain.LIB_CALLS["chunks"]


@pytest.mark.parametrize("chunk_images", [1024, 16])
def test_merge_files_equals_the_restated_tool(merge_case, monkeypatch, chunk_images):
    from s2d_amd import selftrain
    root, (res, ann), prev, preds, want = merge_case
    assert not any("bbox" in e for e in preds + prev["annotations"])
    monkeypatch.setattr(selftrain, "CHUNK_IMAGES", chunk_images)
    out = str(root / f"round1_{chunk_images}.json")
    calls0, chunks0 = _calls()
    doc = selftrain.merge_files(res, ann, out, device=DEV)
    calls, chunks = _calls()
    with open(out) as fh:
        written = json.load(fh)
    assert written == json.loads(json.dumps(want)) and doc == want
    n_items = len({e["image_id"] for e in prev["annotations"]} | {e["image_id"] for e in preds if e["score"] >= 0.7})
    assert chunks - chunks0 == -(-n_items // chunk_images)
    assert calls - calls0 == 5 * (chunks - chunks0) + 1                   # five per chunk, and one polygon fill for the one image that has any
    kinds = {("score" in a) for a in written["annotations"]}
    assert kinds == {True, False} and len(written["annotations"]) < len(prev["annotations"]) + sum(e["score"] >= 0.7 for e in preds)


def test_command_line_output_feeds_the_image_training_mapper(merge_case, tmp_path):
    from PIL import Image
    from s2d_amd.config import load_config
    from s2d_amd.data.image_clip import load_coco_image_train, map_image_clip
    from s2d_amd.data.train_loader import ClipSettings
    root, (res, ann), prev, preds, want = merge_case
    out = str(tmp_path / "round1.json")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-m", "s2d_amd.selftrain", "--new-pred", res, "--prev-ann", ann, "--save-path", out],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith(f"Done: {len(want['images'])} images; {len(want['annotations'])} anns.")
    with open(out) as fh:
        doc = json.load(fh)
    assert doc == json.loads(json.dumps(want))
    records = load_coco_image_train(out, str(tmp_path))
    rec = next(r for r in records if (r["height"], r["width"]) == (120, 160) and len(r["annotations"]) >= 2)
    rng = np.random.default_rng(1)
    Image.fromarray(rng.integers(0, 255, (120, 160, 3), dtype=np.uint8)).save(rec["file_name"], quality=90)
    st = ClipSettings(load_config(KD_CFG, ["INPUT.MIN_SIZE_TRAIN", "(120,)", "INPUT.RANDOM_FLIP", "none", "INPUT.AUGMENTATIONS", "[]",
                                           "INPUT.CROP.ENABLED", "False", "INPUT.SAMPLING_FRAME_NUM", "2"]))
    clip = map_image_clip(rec, None, np.random.RandomState(0), st, device=DEV)
    masks = np.stack([R.seg_mask(a["segmentation"], 120, 160) for a in rec["annotations"]])
    assert len(clip["instances"]) == 2
    for t in range(2):
        assert np.array_equal(clip["instances"][t]["gt_masks"].cpu().numpy(), masks)
