"""GPU checks of keymask discovery: the driver against the golden of the reference's own stages
(tests/golden/make_golden_keymask_driver.py) with the stub tracker, its skip / failure rules, the round trip into the training
loader, and s2d_track_point_id_counts against the two-launch path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden import keymask_stub_tracker as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT_DIRS = ("vis_maps", "vis_clusters", "seg_masks", "annotations")


def _args(extra=()):
    from s2d_amd.keymask.discover import parse_args
    # relative paths: the stages derive a split from substrings such as "test" or "val" of the video path
    return parse_args(["--video-base-path", S.FRAMES_DIR, "--mask-base-path", S.MASKS_DIR, "--save-path", "seg_masks",
                       "--visibility-maps-output-base", "vis_maps", "--visibility-clusters-output-base", "vis_clusters",
                       "--annotation-output-path", "annotations", *extra])


def _run_in(work, tracker, extra=()):
    from s2d_amd.keymask.discover import run
    cwd = os.getcwd()
    os.chdir(work)
    try:
        return run(_args(extra), tracker=tracker)
    finally:
        os.chdir(cwd)


def _tree(root):
    files, texts, pngs = [], {}, {}
    from PIL import Image
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            rel = os.path.relpath(p, root)
            files.append(rel)
            if f.endswith(".png"):
                pngs[rel] = np.array(Image.open(p))
            else:
                texts[rel] = open(p).read()
    return sorted(files), texts, pngs


def _canon(rel, text):
    """JSON compared as data (floats by their exact repr, NaN included); TXT as text"""
    return json.dumps(json.loads(text), sort_keys=True) if rel.endswith(".json") else text


@pytest.fixture(scope="module")
def discovered(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("keymask"))
    cwd = os.getcwd()
    os.chdir(work)
    try:
        S.write_dataset(".")
    finally:
        os.chdir(cwd)
    stub = S.StubTracker()
    report = _run_in(work, stub)
    return work, stub, report


def test_driver_reproduces_the_reference_stages(discovered):
    work, stub, report = discovered
    g = json.load(open(os.path.join(GOLDEN, "keymask_driver.json")))
    pngs = np.load(os.path.join(GOLDEN, "keymask_driver_png.npz"))
    assert report["done"] == g["counts"]["done"] == 2 and report["failed"] == 0 and report["skipped"] == 0
    assert report["tracker_s"] > 0 and report["wall_s"] >= report["tracker_s"]
    assert stub.calls == g["calls"]                                         # the same tracker calls in the same order
    n_png = 0
    for top in OUT_DIRS:
        files, texts, arrs = _tree(os.path.join(work, top))
        assert files == g["files"][top], top
        for rel, text in texts.items():
            assert _canon(rel, text) == _canon(rel, g["texts"][f"{top}/{rel}"]), f"{top}/{rel}"
        for rel, a in arrs.items():
            want = pngs[f"{top}/{rel}"]
            assert a.dtype == want.dtype and np.array_equal(a, want), f"{top}/{rel}"
            n_png += 1
    assert n_png == len(pngs.files)
    # the RLE strings of the annotation JSONs are compared as text above: the device encoder and the fixture's oracle encoder
    # both follow pycocotools' format
    ann = json.load(open(os.path.join(work, "annotations", "vid_b.json")))
    assert any(a["one2x"] > 0 for a in ann["annotations"])


def test_second_run_skips_every_video(discovered):
    work, _, _ = discovered
    stub = S.StubTracker()
    report = _run_in(work, stub)
    assert (report["videos"], report["skipped"], report["done"], report["failed"]) == (2, 2, 0, 0)
    assert stub.calls == []


def test_empty_mask_folder_counts_as_failed(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("keymask_empty"))
    cwd = os.getcwd()
    os.chdir(work)
    try:
        S.write_dataset(".", {"vid_b": S.SCENES["vid_b"]})
        for f in os.listdir(os.path.join(S.MASKS_DIR, "vid_b")):
            os.remove(os.path.join(S.MASKS_DIR, "vid_b", f))
    finally:
        os.chdir(cwd)
    report = _run_in(work, S.StubTracker())
    assert (report["videos"], report["done"], report["failed"], report["skipped"]) == (1, 0, 1, 0)
    assert not os.path.exists(os.path.join(work, "annotations", "vid_b.json"))


def test_cli_discover_merge_and_train_loader_round_trip(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("keymask_cli"))
    cwd = os.getcwd()
    os.chdir(work)
    try:
        S.write_dataset(".")
    finally:
        os.chdir(cwd)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    a = _args(["--tracker", "tests.golden.keymask_stub_tracker:make_tracker"])
    argv = ["--video-base-path", a.video_base_path, "--mask-base-path", a.mask_base_path, "--save-path", a.save_path,
            "--visibility-maps-output-base", a.visibility_maps_output_base,
            "--visibility-clusters-output-base", a.visibility_clusters_output_base,
            "--annotation-output-path", a.annotation_output_path, "--tracker", a.tracker]
    r = subprocess.run([sys.executable, "-m", "s2d_amd.keymask.discover", *argv], capture_output=True, text=True, cwd=work,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert (report["videos"], report["done"], report["failed"]) == (2, 2, 0)
    merged = os.path.join(work, "merged", "train.json")
    r = subprocess.run([sys.executable, "-m", "s2d_amd.keymask.merge", os.path.join(work, "annotations"), merged, "0.1"],
                       capture_output=True, text=True, cwd=work, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    doc = json.load(open(merged))
    assert [v["id"] for v in doc["videos"]] == [1, 2]
    assert len(doc["annotations"]) == 8 and all(a["one2x"] <= 0.1 for a in doc["annotations"])   # one noisy group dropped
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import ClipSettings, load_ytvis_train, map_clip
    import random
    recs = load_ytvis_train(merged, os.path.join(work, S.FRAMES_DIR))
    assert len(recs) == 2
    st = ClipSettings(load_config(os.path.join(GOLDEN, "kd_config.json"), ["INPUT.MIN_SIZE_TRAIN", "(64,)", "INPUT.CROP.ENABLED", "False"]))
    for k, rec in enumerate(recs):
        clip = map_clip(rec, random.Random(k), np.random.RandomState(k), st, device="cuda:0")
        assert len(clip["image"]) == st.num_frames
        assert sum(int(i["gt_masks"].shape[0]) for i in clip["instances"]) > 0


# -------------------------------------------------------------------------------------------------- s2d_track_point_id_counts
def _two_launch(tracks, H, W, idmap):
    from s2d_amd.keymask import point_id_counts, pred_tracks_to_binary_masks
    return point_id_counts(pred_tracks_to_binary_masks(tracks[None], H, W)[0], idmap)


def _tracks(rng, T, P, H, W):
    """integers, exact halves and random fractions around and outside the frame, with repeated points"""
    xy = np.stack([rng.integers(-3, W + 3, (T, P)), rng.integers(-3, H + 3, (T, P))], -1).astype(np.float32)
    frac = rng.choice(np.array([0.0, 0.5, -0.5, 0.49999997, 1.5], np.float32), (T, P, 2))
    xy += np.where(rng.random((T, P, 2)) < 0.3, rng.random((T, P, 2)).astype(np.float32) - 0.5, frac)
    if P > 4:
        dup = rng.integers(0, P, P // 4)
        xy[:, dup] = xy[:, rng.integers(0, P, P // 4)]
    return torch.from_numpy(xy).cuda()


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 1000, 2500, 4097, 32768, 32769])
@pytest.mark.parametrize("resized", [False, True])
def test_fused_counts_equal_two_launch_path(P, resized):
    from s2d_amd.keymask import IdMap, point_id_counts_from_tracks
    from s2d_amd.keymask.propagate import TRACK_COUNTS_MAX_POINTS
    rng = np.random.default_rng(P * 2 + resized)
    T, H, W = 6, 47, 83
    Hi, Wi = (61, 29) if resized else (H, W)
    ids = rng.integers(0, 9, (T, Hi, Wi))
    ids[2] = 0                                                             # a frame without objects
    idmap = IdMap(torch.from_numpy(ids), max_id=8190 if P == 65 else None)
    tr = _tracks(rng, T, P, H, W)
    c1, t1 = point_id_counts_from_tracks(tr, H, W, idmap)
    c2, t2 = _two_launch(tr, H, W, idmap)
    assert torch.equal(c1, c2) and torch.equal(t1, t2)
    if 0 < P <= TRACK_COUNTS_MAX_POINTS:
        assert int(t1.max()) > 0
    if P > TRACK_COUNTS_MAX_POINTS:                                          # the export itself refuses: the wrapper fell back
        from s2d_amd._lib import lib
        with pytest.raises(RuntimeError):
            lib().call("s2d_track_point_id_counts", tr, T, P, H, W, idmap.ids, Hi, Wi, idmap.max_id, c1, t1,
                       torch.cuda.current_stream().cuda_stream)


def test_fused_counts_drop_non_finite_points():
    from s2d_amd.keymask import IdMap, point_id_counts_from_tracks
    rng = np.random.default_rng(5)
    T, P, H, W = 4, 700, 50, 70
    idmap = IdMap(torch.from_numpy(rng.integers(0, 5, (T, H, W))))
    tr = _tracks(rng, T, P, H, W).cpu().numpy()
    bad = rng.random((T, P)) < 0.2
    poison = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), (T, P))
    which = rng.integers(0, 2, (T, P))
    tr_bad = tr.copy()
    for t in range(T):
        for p in np.nonzero(bad[t])[0]:
            tr_bad[t, p, which[t, p]] = poison[t, p]
    c1, t1 = point_id_counts_from_tracks(torch.from_numpy(tr_bad).cuda(), H, W, idmap)
    for t in range(T):                                                       # the same frame with those points removed
        keep = torch.from_numpy(tr[t][~bad[t]]).cuda()[None]
        sub = IdMap(idmap.ids[t:t + 1].cpu(), max_id=idmap.max_id)
        c2, t2 = _two_launch(keep, H, W, sub)
        assert torch.equal(c1[t], c2[0]) and int(t1[t]) == int(t2[0])


def test_fused_matching_variant_equals_extract_mask_matches():
    from s2d_amd import keymask as km
    from tests.conftest import golden
    g = golden("keymask")
    tracks = torch.from_numpy(g["tracks"]).cuda()
    idmap = km.IdMap(torch.from_numpy(g["idmap"].astype(np.int64)))
    T, H, W = idmap.T, idmap.Hi, idmap.Wi
    for hw, tr, vr in (((H, W), tracks, (0, T - 1)), ((H + 7, W - 5), tracks * 1.1, (1, T - 2))):
        assert km.extract_mask_matches_from_tracks(hw, tr, idmap, vr) == km.extract_mask_matches(hw, tr, idmap, vr)
