"""GPU checks of the wide-search tracker with a live template (s2d_block_track_live_u8 in csrc/block_track.hip,
s2d_amd/keymask/block_tracker.py LiveBlockTracker).  The kernel makes integer decisions only, so every comparison with the numpy
restatement (tests/live_tracker_ref.py) and with the fixed-template export is an equality; together with
tests/test_live_tracker_refs_cpu.py the device therefore equals the ground truth wherever that is guaranteed.  The last test runs
discovery end to end with `--tracker block-live` on the textured scenes and records (does not assert) how its groups compare with
a ground-truth tracker's."""
import functools
import glob
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import block_tracker_ref as B
from tests import live_tracker_ref as L
from tests.golden import keymask_stub_tracker as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _track_dev(grey, points, q, backward, R, S_, tau, tau_u=None):
    """s2d_block_track_live_u8, or with tau_u = None the fixed-template s2d_block_track_u8, on outputs filled with NaN and 7"""
    from s2d_amd._lib import lib
    g = torch.from_numpy(np.array(grey)).cuda()                              # a copy: the shared scenes are read-only
    T, H, W = g.shape
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.int32)).cuda()
    N = pts.shape[0]
    tracks = torch.full((T, N, 2), float("nan"), device="cuda")
    vis = torch.full((T, N), 7, device="cuda", dtype=torch.uint8)            # every element has to be written
    if tau_u is None:
        lib().call("s2d_block_track_u8", g, T, H, W, pts, N, q, int(backward), R, S_, tau, tracks, vis, _stream())
    else:
        lib().call("s2d_block_track_live_u8", g, T, H, W, pts, N, q, int(backward), R, S_, tau, tau_u, tracks, vis, _stream())
    return tracks.cpu().numpy(), vis.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _small_scene():
    """u8 [6,37,53]: a textured background with two textured patches that move, one of them out of the frame (the scene of
    tests/test_gpu_block_tracker.py), and from frame 2 on the first patch brightens by 4 per frame, so a live template matters"""
    rng = np.random.default_rng(7)
    T, H, W = 6, 37, 53
    bg = B._texture(rng, H, W)[..., 0]
    a, b = B._texture(rng, 14, 16)[..., 0], B._texture(rng, 12, 12)[..., 0]
    out = np.empty((T, H, W), np.uint8)
    for t in range(T):
        f = bg.copy()
        y, x = 4 + t, 6 + 5 * t                                              # (1, 5) per frame
        f[y:y + 14, x:x + 16] = np.clip(a.astype(np.int64) + 4 * max(t - 1, 0), 0, 255)
        y, x = 22 - 2 * t, 38 + 3 * t                                        # (-2, 3) per frame, leaves on the right
        f[y:y + 12, x:min(x + 12, W)] = b[:, :max(min(12, W - x), 0)]
        out[t] = f
    out.setflags(write=False)
    return out


def _small_points(H, W):
    g = B.grid_ref(8, H, W)
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    border = [(W // 2, 0), (W // 3, H - 1), (0, H // 2), (W - 1, H // 3), (1, 1), (W - 2, H - 2)]
    return np.concatenate([g, np.array(corners + border)]).astype(np.int32)


SMALL_CALLS = ((2, True), (0, False), (5, True), (3, False))


@functools.lru_cache(maxsize=None)
def _small_reference(R, S_, tau, tau_u):
    """the numpy reference of the four small-frame calls, computed once per parameter set (read-only)"""
    grey = _small_scene()
    pts = _small_points(*grey.shape[1:])
    out = []
    for q, back in SMALL_CALLS:
        t, v = L.live_track_ref(grey, pts, q, back, R, S_, tau, tau_u)
        t.setflags(write=False)
        v.setflags(write=False)
        out.append((t, v))
    return out


@pytest.mark.parametrize("params", [(5, 64, 12, 4), (7, 64, 255, 255), (3, 40, 12, -1), (1, 1, 0, 0), (5, 16, 12, 0)])
def test_small_frame_equals_the_reference(params):
    R, S_, tau, tau_u = params
    grey = _small_scene()
    T, H, W = grey.shape
    assert T == 6 and SMALL_CALLS[2][0] == T - 1
    pts = _small_points(H, W)
    assert len(pts) <= 100
    moved = 0
    for (q, back), (want_t, want_v) in zip(SMALL_CALLS, _small_reference(*params)):
        got_t, got_v = _track_dev(grey, pts, q, back, R, S_, tau, tau_u)
        assert np.array_equal(got_v, want_v), (q, back)
        assert np.array_equal(got_t, want_t), (q, back)
        moved += int((want_t != pts[None].astype(np.float32)).any(-1).sum())
    assert moved > 0 or S_ < 4                              # 5 px per frame is beyond a search radius of 1


def test_small_frame_refresh_changes_the_outcome():
    # the brightening patch: with the same search the live and the fixed template must part somewhere, else the cases above
    # would not tell a kernel that never refreshes from one that does
    grey = _small_scene()
    pts = _small_points(*grey.shape[1:])
    q, back = SMALL_CALLS[1]
    live = _small_reference(5, 64, 12, 4)[1]
    fixed = L.live_track_ref(grey, pts, q, back, 5, 64, 12, -1)
    assert not (np.array_equal(live[0], fixed[0]) and np.array_equal(live[1], fixed[1]))
    got = _track_dev(grey, pts, q, back, 5, 64, 12, -1)
    assert np.array_equal(got[0], fixed[0]) and np.array_equal(got[1], fixed[1])


def test_tie_rule_at_the_widest_search():
    T, H, W, R, S_ = 4, 48, 64, 3, 64
    yy, xx = np.mgrid[0:H, 0:W]
    pts = np.concatenate([B.grid_ref(6, H, W), np.array([(0, 0), (W - 1, H - 1)])]).astype(np.int32)
    m = R + 2 * T + 4                                   # a point drifts by 2 px per frame at the most; one stripe period
    interior = (pts[:, 0] >= m) & (pts[:, 0] < W - m) & (pts[:, 1] >= m) & (pts[:, 1] < H - m)
    assert interior.sum() >= 4
    base = pts[None].astype(np.float32)

    def run(frames, q=0, back=False, tau_u=4):
        got = _track_dev(frames, pts, q, back, R, S_, 12, tau_u)
        want = L.live_track_ref(frames, pts, q, back, R, S_, 12, tau_u)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        return got

    # constant frames: every candidate inside the frame costs 0, d^2 = 0 wins although d^2 goes up to 2 * 64^2
    tr, vis = run(np.full((T, H, W), 93, np.uint8), q=1, back=True)
    assert np.array_equal(tr, np.broadcast_to(base, tr.shape)) and vis.all()
    stripes = lambda shift_x, shift_y: np.stack([(((xx - shift_x * t) % 4 < 2) * 200 + ((yy - shift_y * t) % 4 < 2) * 40 * (shift_y != 0))
                                                 .astype(np.uint8) for t in range(T)])
    # period-4 vertical stripes shifted by 2 px: zero cost at every dx = 2 (mod 4) and every dy; dx = -2 and +2 share d^2 = 4
    # and dy = 0: the smaller dx wins
    for tau_u in (4, -1):
        tr, vis = run(stripes(2, 0), tau_u=tau_u)
        for t in range(T):
            assert np.array_equal(tr[t, interior], (pts[interior] + (-2 * t, 0)).astype(np.float32)) and vis[t, interior].all()
    # a period-4 pattern in both axes shifted by (2, 2): (+-2, +-2) all cost 0 with d^2 = 8: the smaller dy, then the smaller dx
    tr, vis = run(stripes(2, 2))
    for t in range(T):
        assert np.array_equal(tr[t, interior], (pts[interior] + (-2 * t, -2 * t)).astype(np.float32)) and vis[t, interior].all()


@pytest.mark.parametrize("S_", [16, 24])
def test_without_refresh_equals_the_fixed_template_export(S_):
    grey = _small_scene()
    pts = _small_points(*grey.shape[1:])
    for R, tau in ((5, 12), (7, 255), (2, 30)):
        for q, back in SMALL_CALLS:
            want = _track_dev(grey, pts, q, back, R, S_, tau)
            got = _track_dev(grey, pts, q, back, R, S_, tau, -1)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (R, tau, q, back)
    for name, q, obj in (("vid_a", 5, 2), ("vid_b", 0, 0)):
        assert (name, q, obj) in B.CALLS
        grey, pts = B.textured_grey(name), B.call_points(name, q, obj)
        want = _track_dev(grey, pts, q, q > 0, B.R, S_, B.TAU)
        got = _track_dev(grey, pts, q, q > 0, B.R, S_, B.TAU, -1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, q, obj)
        assert want[1].any() and not want[1].all()


@pytest.fixture(scope="module")
def videos():
    return {name: torch.from_numpy(L.scene_video_f32(name)).cuda()[None] for name in L.SCENES}


@pytest.mark.parametrize("name,calls,search", [("fast", L.FAST_CALLS, L.FAST_SEARCH), ("drift", L.DRIFT_CALLS, L.DRIFT_SEARCH)])
def test_fast_and_drift_calls_equal_the_reference(videos, name, calls, search):
    from s2d_amd.keymask.block_tracker import LiveBlockTracker
    tracker = LiveBlockTracker(search=search)
    assert (tracker.radius, tracker.tau, tracker.refresh) == (L.R, L.TAU, L.REFRESH)
    for q, obj in calls:
        pts, want_t, want_v = L.reference_call(name, q, obj)
        mask = torch.from_numpy(L.call_mask(name, q, obj))[None, None]
        tracks, vis = tracker(videos[name], grid_size=50, grid_query_frame=q, segm_mask=mask, backward_tracking=q > 0)
        assert tracks.shape == (1, want_t.shape[0], len(pts), 2) and tracks.dtype == torch.float32 and tracks.is_cuda
        assert vis.shape == tracks.shape[:3] and vis.dtype == torch.bool
        assert np.array_equal(vis[0].cpu().numpy(), want_v.astype(bool)), (name, q, obj)
        assert np.array_equal(tracks[0].cpu().numpy(), want_t), (name, q, obj)


def test_default_call_on_a_textured_scene_equals_the_reference():
    from s2d_amd.keymask.block_tracker import LiveBlockTracker
    name, q, obj = B.CALLS[7]                               # vid_b object 0 from frame 5: it slides under object 4, backward too
    pts, want_t, want_v = L.reference_default_call(name, q, obj)
    video = torch.from_numpy(B.video_f32(name)).cuda()[None]
    mask = torch.from_numpy(B.call_mask(name, q, obj))[None, None]
    tracks, vis = LiveBlockTracker()(video, grid_size=50, grid_query_frame=q, segm_mask=mask, backward_tracking=True)
    assert np.array_equal(vis[0].cpu().numpy(), want_v.astype(bool)) and np.array_equal(tracks[0].cpu().numpy(), want_t)


def test_empty_mask_grey_cache_and_size_refusal(videos):
    from s2d_amd.keymask.block_tracker import LiveBlockTracker
    tracker = LiveBlockTracker(search=L.FAST_SEARCH)
    video = videos["fast"].clone()
    T, H, W = video.shape[1], video.shape[-2], video.shape[-1]
    tracks, vis = tracker(video, grid_size=50, grid_query_frame=0, segm_mask=torch.zeros((1, 1, H, W), dtype=torch.uint8))
    assert tracks.shape == (1, T, 0, 2) and vis.shape == (1, T, 0) and vis.dtype == torch.bool
    assert tracker._grey is None                                               # nothing was launched, not even the grey pass
    q, obj = L.FAST_CALLS[0]
    mask = torch.from_numpy(L.call_mask("fast", q, obj))[None, None]
    pts, want_t, want_v = L.reference_call("fast", q, obj)
    t1, v1 = tracker(video, grid_size=50, grid_query_frame=q, segm_mask=mask)
    grey = tracker._grey
    assert np.array_equal(grey.cpu().numpy(), L.scene_grey("fast"))
    t2, v2 = tracker(video, grid_size=50, grid_query_frame=q, segm_mask=mask)
    assert tracker._grey is grey                                               # the second call took the cached frames
    assert torch.equal(t1, t2) and torch.equal(v1, v2) and np.array_equal(t1[0].cpu().numpy(), want_t)
    # an in-place edit: the frames after the query frame become copies of it, so nothing moves any more
    video[:, 1:] = video[:, :1]
    t3, v3 = tracker(video, grid_size=50, grid_query_frame=q, segm_mask=mask)
    assert tracker._grey is not grey
    assert np.array_equal(t3[0].cpu().numpy(), np.broadcast_to(pts.astype(np.float32), want_t.shape)) and bool(v3.all())
    assert not np.array_equal(want_t, np.broadcast_to(pts.astype(np.float32), want_t.shape))
    with pytest.raises(ValueError):
        tracker(video, grid_size=50, segm_mask=torch.zeros((1, 1, W, H), dtype=torch.uint8))


@pytest.mark.parametrize("bad", [dict(S_=65), dict(S_=0), dict(R=8), dict(tau_u=13), dict(tau_u=-2), dict(q=6), dict(tau=256)])
def test_export_refuses(bad):
    # every case is refused by the argument check in front of the launch
    grey = _small_scene()
    kw = dict(q=0, backward=False, R=5, S_=16, tau=12, tau_u=4)
    assert grey.shape[0] == 6 and kw["tau"] + 1 == 13
    kw.update(bad)
    with pytest.raises(RuntimeError):
        _track_dev(grey, _small_points(*grey.shape[1:]), **kw)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _discover(work, tracker=None, extra=()):
    from s2d_amd.keymask.discover import parse_args, run
    cwd = os.getcwd()
    os.chdir(work)                  # relative paths: the stages derive a split from substrings such as "test" of the video path
    try:
        args = parse_args(["--video-base-path", S.FRAMES_DIR, "--mask-base-path", S.MASKS_DIR, "--save-path", "seg_masks",
                           "--visibility-maps-output-base", "vis_maps", "--visibility-clusters-output-base", "vis_clusters",
                           "--annotation-output-path", "annotations", *extra])
        return run(args, tracker=tracker)
    finally:
        os.chdir(cwd)


def _stage1(work, name):
    path, = glob.glob(os.path.join(work, "vis_maps", "DAVIS", "*", "data", name + ".json"))
    doc = json.load(open(path))["video_data"]
    rows = [(f["frame_id"], o["object_id"]) for f in doc for o in f["data"]]
    curves = np.array([o["visibility"] for f in doc for o in f["data"]], np.float64)
    return rows, curves


def _figures(work):
    out = {}
    for name in sorted(S.SCENES):
        ann = json.load(open(os.path.join(work, "annotations", name + ".json")))["annotations"]
        out[name] = {"annotations": len(ann),
                     "frames_covered": [sum(s is not None for s in a["segmentations"]) for a in ann]}
    return out


def test_discovery_end_to_end_with_the_live_tracker(tmp_path):
    from s2d_amd.config import load_config
    from s2d_amd.data.train_loader import ClipSettings, load_ytvis_train, map_clip
    from s2d_amd.keymask.formats import merge_ytvis_jsons
    works = {}
    for kind in ("block-live", "truth"):
        works[kind] = str(tmp_path / kind)
        os.makedirs(works[kind])
        B.write_textured_dataset(works[kind])
    report = _discover(works["block-live"], extra=["--tracker", "block-live", "--tracker-options", "search=32,refresh=4"])
    assert (report["videos"], report["done"], report["failed"]) == (2, 2, 0)
    truth_report = _discover(works["truth"], tracker=B.TruthTracker())
    assert (truth_report["done"], truth_report["failed"]) == (2, 0)
    figures = {"block-live": _figures(works["block-live"]), "truth": _figures(works["truth"]), "stage1_binarised_at_0.3": {}}
    for name in sorted(S.SCENES):
        rows, curves = _stage1(works["block-live"], name)
        rows_t, curves_t = _stage1(works["truth"], name)
        assert rows == rows_t
        diff = int(((curves > 0.3) != (curves_t > 0.3)).sum())
        figures["stage1_binarised_at_0.3"][name] = {"entries": int(curves.size), "differ_from_truth": diff}
        assert figures["block-live"][name]["annotations"] >= 1
    print(json.dumps(figures))
    out = os.environ.get("S2D_LIVE_TRACKER_FIGURES")                           # a measurement: recorded, not asserted
    if out:
        with open(out, "w") as f:
            json.dump(figures, f, indent=1)
    # the output feeds the merge step and the training loader, as the stub-tracker driver test does
    merged = os.path.join(works["block-live"], "merged", "train.json")
    os.makedirs(os.path.dirname(merged))
    doc = merge_ytvis_jsons(os.path.join(works["block-live"], "annotations"), merged, -1.0)
    assert [v["id"] for v in doc["videos"]] == [1, 2] and len(doc["annotations"]) >= 2
    recs = load_ytvis_train(merged, os.path.join(works["block-live"], S.FRAMES_DIR))
    assert len(recs) == 2
    st = ClipSettings(load_config(os.path.join(GOLDEN, "kd_config.json"), ["INPUT.MIN_SIZE_TRAIN", "(64,)", "INPUT.CROP.ENABLED", "False"]))
    for k, rec in enumerate(recs):
        clip = map_clip(rec, random.Random(k), np.random.RandomState(k), st, device="cuda:0")
        assert len(clip["image"]) == st.num_frames
        assert sum(int(i["gt_masks"].shape[0]) for i in clip["instances"]) > 0
