"""GPU side of the YTVIS evaluator (csrc/ytvis_eval.hip, s2d_amd/ytvis_eval.py): the device RLE decode against the oracle's
rleDecode, the cross counts against s2d_mask_pair_counts_u64 and numpy, and the whole evaluation against the reference-generated
fixture (tests/golden/ytvis_eval.json) -- IoU matrices bit for bit -- from results.json, from each form of `process` input,
from the model's eval branch, and from two gloo ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, ROOT
from tests.test_ytvis_eval_cpu import check_against

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(GOLDEN, "ytvis_eval.json")) as fh:
        return json.load(fh)


def runs(m):
    flat = np.asarray(m, bool).T.reshape(-1)
    pos = np.flatnonzero(np.diff(np.concatenate([[False], flat]).astype(np.int8)))
    return np.diff(np.concatenate([[0], pos, [flat.size]]))


def compressed(m):
    from s2d_amd.rle import strings_from_runs
    r = runs(m).astype(np.int64)
    return {"size": list(m.shape), "counts": strings_from_runs(r, np.array([0, len(r)], np.int64))[0].decode()}


def packed(m):
    """row-major flat index i -> word i/32, bit i%32"""
    flat = np.asarray(m, bool).reshape(-1)
    n = (flat.size + 31) // 32 * 32
    b = np.packbits(np.concatenate([flat, np.zeros(n - flat.size, bool)]), bitorder="little")
    return b.view(np.uint32)


def blobs(rng, H, W, n):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.5, max(H, W) / 3 + 1)
        m ^= (yy - cy) ** 2 + ((xx - cx) * 0.7) ** 2 < r * r
    return m


@pytest.mark.parametrize("H,W", [(1, 1), (5, 37), (64, 64), (257, 291), (720, 1280)])
def test_decode_matches_oracle(oracle, H, W):
    from s2d_amd.ytvis_eval import decode_frames, plane_areas
    rng = np.random.default_rng(H * 7 + W)
    masks = [blobs(rng, H, W, 3), np.ones((H, W), bool), np.zeros((H, W), bool), rng.random((H, W)) < 0.5]
    if H >= 720:                                                  # long runs: multi-character counts and deltas
        masks.append(np.zeros((H, W), bool)); masks[-1][100:700, 5:1200] = True
    segs = [compressed(m) if k % 2 == 0 else {"size": [H, W], "counts": [int(c) for c in runs(m)]} for k, m in enumerate(masks)]
    segs.insert(1, None)                                          # an absent frame: zero plane, zero area
    masks.insert(1, None)
    bits = decode_frames(segs, H, W, DEV)
    area = plane_areas(bits).cpu().numpy()
    got = bits.cpu().numpy().view(np.uint32)
    for f, (s, m) in enumerate(zip(segs, masks)):
        if s is None:
            assert not got[f].any() and area[f] == 0
            continue
        ref = oracle.rle_decode(s) if isinstance(s["counts"], str) else m
        assert np.array_equal(ref, m)
        assert np.array_equal(got[f], packed(ref)), f
        assert area[f] == ref.sum()


# the last case is 9000 words per track: three chunks of the word range add into every entry (the others are one chunk)
@pytest.mark.parametrize("D,G,T,H,W", [(1, 1, 3, 45, 70), (10, 5, 3, 45, 70), (13, 9, 3, 45, 70), (13, 9, 2, 360, 400)],
                         ids=["1-1", "10-5", "13-9", "13-9-chunks"])
def test_cross_counts_match_pair_counts(D, G, T, H, W):
    from s2d_amd import ops
    from s2d_amd.ytvis_eval import cross_counts
    rng = np.random.default_rng(D * 31 + G)
    m = torch.from_numpy((rng.random((D + G, T, H, W)) < 0.3).astype(np.uint8)).to(DEV)
    bits = ops.pack_mask_bits(m.view(D + G, -1))
    got = cross_counts(bits[:D].contiguous(), bits[D:].contiguous()).cpu().numpy()
    full = ops.mask_pair_counts(bits).cpu().numpy()
    assert np.array_equal(got, full[:D, D:])
    h = m.cpu().numpy().reshape(D + G, -1).astype(bool)
    assert np.array_equal(got, (h[:D, None] & h[None, D:]).sum(-1))


@pytest.mark.parametrize("use_cats", [0, 1])
def test_evaluate_ytvis_matches_reference(fx, use_cats):
    from s2d_amd.ytvis_eval import evaluate_ytvis
    ev = evaluate_ytvis(fx["gt"], fx["results"], use_cats=bool(use_cats))
    ev.summarize(out=None)
    check_against(ev, fx[f"use_cats_{use_cats}"])                 # IoU matrices bit-identical, matches, precision, recall, stats


def _videos(fx):
    out = {}
    for r in fx["results"]:
        out.setdefault(r["video_id"], []).append(r)
    return out


def _feed(ev, fx, form, vids=None):
    from s2d_amd.ytvis_eval import decode_frames
    info = {v["id"]: v for v in fx["gt"]["videos"]}
    byvid = _videos(fx)
    for vid in (vids if vids is not None else list(byvid)):
        rs = byvid[vid]
        out = {"pred_scores": [r["score"] for r in rs], "pred_labels": [r["category_id"] for r in rs]}
        H, W, T = info[vid]["height"], info[vid]["width"], len(rs[0]["segmentations"])
        if form == "rle":
            out["pred_masks"] = [r["segmentations"] for r in rs]
            out["pred_masks_format"] = "coco_rle"
        else:
            bits = decode_frames([s for r in rs for s in r["segmentations"]], H, W, DEV).cpu().numpy().view(np.uint32)
            m = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :H * W].reshape(len(rs), T, H, W).astype(bool)
            if form == "cpu":
                out["pred_masks"] = [torch.from_numpy(x) for x in m]
            else:
                out["pred_masks"] = torch.from_numpy(m).to(DEV)
        ev.process([{"video_id": vid, "length": T}], out)


@pytest.mark.parametrize("form", ["cpu", "rle", "device"])
def test_evaluator_process_forms(fx, form, tmp_path):
    from s2d_amd.ytvis_eval import YTVISEvaluator, derive_results, evaluate_ytvis
    ev = YTVISEvaluator(None, None, True, str(tmp_path) if form == "device" else None, json_file=fx["gt"])
    ev.reset()
    _feed(ev, fx, form)
    res = ev.evaluate()
    want = derive_results(fx["use_cats_0"]["stats"])
    assert set(res) == {"segm"}
    for k, v in want.items():
        assert res["segm"][k] == pytest.approx(v, abs=1e-9), k
    check_against(ev.ytvis_eval, fx["use_cats_0"])
    if form == "device":                                           # results.json: the device encoder's strings re-score the same
        written = json.load(open(tmp_path / "results.json"))
        assert len(written) == len(fx["results"])
        ev2 = evaluate_ytvis(fx["gt"], written)
        ev2.summarize(out=None)
        np.testing.assert_array_equal(ev2.stats, ev.ytvis_eval.stats)


def test_model_eval_branch_into_evaluator():
    """KDVideoMaskFormer eval branch -> process (CPU bool masks) == its masks through the device encoder (what rle=True
    returns) -> evaluate_ytvis"""
    from s2d_amd.modeling import build_kd_model
    from s2d_amd.rle import encode_video_predictions
    from s2d_amd.utils import synth
    from s2d_amd.ytvis_eval import YTVISEvaluator, evaluate_ytvis
    from tests.parity import seeded_load
    T, H0, W0, Q, NL, K = 3, 60, 90, 12, 4, 5
    model = build_kd_model(num_queries=Q, num_frames=2, num_points=64, dec_layers=NL)
    seeded_load(model.student, 7)
    seeded_load(model.teacher, 8)
    model = model.to(DEV).eval()
    model.num_predictions_inference = K
    frames = synth.smooth_frames_u8(9, 1, T, H0, W0)
    out = model([{"image": [torch.from_numpy(f) for f in frames], "height": 90, "width": 135}])
    assert len(out["pred_masks"]) == K
    preds = torch.stack(out["pred_masks"]).to(DEV)
    gts = []
    for k in range(3):                                            # ground truth: two of the predictions, shifted, and a box
        m = preds[k].cpu().numpy().copy() if k < 2 else np.zeros((T, 90, 135), bool)
        if k < 2:
            m = np.roll(m, 3 * (k + 1), axis=-1)
        else:
            m[:, 20:60, 30:90] = True
        gts.append({"id": 1 + k, "video_id": 7, "category_id": 1 + (k % 2), "iscrowd": 0,
                    "segmentations": [compressed(f) for f in m], "areas": [int(f.sum()) for f in m]})
    doc = {"videos": [{"id": 7, "height": 90, "width": 135, "length": T}],
           "categories": [{"id": c, "name": str(c)} for c in sorted(set(out["pred_labels"]) | {1, 2})],
           "annotations": gts}
    ev = YTVISEvaluator(json_file=doc)
    ev.process([{"video_id": 7, "length": T}], out)
    res = ev.evaluate()["segm"]
    rles = encode_video_predictions(preds)
    results = [{"video_id": 7, "score": s, "category_id": l, "segmentations": r} for s, l, r in zip(out["pred_scores"], out["pred_labels"], rles)]
    ev2 = evaluate_ytvis(doc, results)
    ev2.summarize(out=None)
    np.testing.assert_array_equal(ev.ytvis_eval.stats, ev2.stats)
    assert np.array_equal(ev.ytvis_eval.ious[7, -1], ev2.ious[7, -1])
    assert res["AP"] == (ev2.stats[0] * 100 if ev2.stats[0] >= 0 else res["AP"])


def test_two_gloo_ranks_share_the_gpu(fx, tmp_path):
    """two ranks (torch.distributed.run, gloo, both on cuda:0), each processing half the videos: rank 0's result equals one
    process over all the videos in the same order"""
    from s2d_amd.ytvis_eval import YTVISEvaluator
    out = tmp_path / "rank0.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", S2D_YTVIS_OUT=str(out))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29673", os.path.join(ROOT, "tests", "_ytvis_eval_worker.py")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.load(open(out))
    vids = sorted(_videos(fx))
    ev = YTVISEvaluator(json_file=fx["gt"], distributed=True)
    _feed(ev, fx, "rle", vids[0::2] + vids[1::2])                  # rank 0's videos first, as the gather concatenates them
    want = ev.evaluate()
    assert got["segm"] == json.loads(json.dumps(want["segm"]))
    assert got["stats"] == ev.ytvis_eval.stats.tolist()
