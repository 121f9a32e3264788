"""GPU checks of the zero-mean block tracker (s2d_block_track_zm_u8 in csrc/block_track.hip, s2d_amd/keymask/block_tracker.py
ZeroMeanBlockTracker).  The kernel makes integer decisions only, so every comparison with the numpy restatement
(tests/zm_tracker_ref.py) is an equality; together with tests/test_zm_tracker_refs_cpu.py the device therefore equals the ground
truth wherever that is guaranteed, and is as blind to a brightness offset as the rule says.  The last test runs discovery end to
end with `--tracker block-zm` on the lit and on the unlit dataset and wants the same annotations from both."""
import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import block_tracker_ref as B
from tests import zm_tracker_ref as Z
from tests.golden import keymask_stub_tracker as S

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _track_dev(grey, points, q, backward, R, S_, tau, tau_u, texture):
    """s2d_block_track_zm_u8 on outputs filled with NaN, 7 and 9: every element has to be written"""
    from s2d_amd._lib import lib
    g = torch.from_numpy(np.array(grey)).cuda()                              # a copy: the shared scenes are read-only
    T, H, W = g.shape
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.int32)).cuda()
    N = pts.shape[0]
    tracks = torch.full((T, N, 2), float("nan"), device="cuda")
    vis = torch.full((T, N), 7, device="cuda", dtype=torch.uint8)
    trackable = torch.full((N,), 9, device="cuda", dtype=torch.uint8)
    lib().call("s2d_block_track_zm_u8", g, T, H, W, pts, N, q, int(backward), R, S_, tau, tau_u, texture, tracks, vis, trackable, _stream())
    return tracks.cpu().numpy(), vis.cpu().numpy(), trackable.cpu().numpy()


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def _small_scene(lit=True):
    """u8 [5,41,57]: a textured ground (48 .. 207) with a flat rectangle, two textured patches that move, one of them out of the
    frame, and a flat patch that moves; lit: plus zm_tracker_ref.light(t) in frame t"""
    rng = np.random.default_rng(11)
    T, H, W = 5, 41, 57
    tex = lambda h, w: Z.squeeze(B._texture(rng, h, w)[..., 0])
    bg = tex(H, W)
    bg[24:41, 0:20] = 131                                                    # flat down to the corner (0, H - 1)
    a, b = tex(14, 16), tex(12, 12)
    out = np.empty((T, H, W), np.int64)
    for t in range(T):
        f = bg.astype(np.int64)
        y, x = 3 + t, 5 + 5 * t                                              # (1, 5) per frame
        f[y:y + 14, x:x + 16] = a
        y, x = 26 - 2 * t, 40 + 3 * t                                        # (-2, 3) per frame, leaves on the right
        f[y:y + 12, x:min(x + 12, W)] = b[:, :max(min(12, W - x), 0)]
        f[2:12, 30 + 2 * t:44 + 2 * t] = 90                                  # flat, 2 px per frame
        out[t] = f + (Z.light(t) if lit else 0)
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    out.setflags(write=False)
    return out


def _small_points(H, W):
    g = B.grid_ref(7, H, W)
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    border = [(W // 2, 0), (W // 3, H - 1), (0, H // 2), (W - 1, H // 3), (1, 1), (W - 2, H - 2), (36, 6), (8, 33)]
    return np.concatenate([g, np.array(corners + border)]).astype(np.int32)


# (query frame, backward): the first, a middle and the last frame
SMALL_CALLS = ((0, False), (2, True), (4, True), (2, False))
TAU = 12
# (tau_u, texture, call): a covering of tau_u in {-1, 4, tau} x texture in {0, 4} with every call, not their full product -- the
# three do not interact in the kernel (the gate is decided before the search, the refresh after a frame's decision)
COMBOS = ((-1, 0, 0), (4, 4, 1), (TAU, 0, 2), (-1, 4, 3), (4, 0, 2), (TAU, 4, 1), (4, 4, 0))


# R = 1, 5, 7: 1, 3 and 4 dwords per patch row with three valid bytes in the last; R = 2, 4, 6: 2, 3 and 4 dwords with one.
# S = 25 and 64: a window larger than the frame
@pytest.mark.parametrize("R,S_", [(R, S_) for R in (1, 5, 7) for S_ in (1, 16, 25, 64)] + [(2, 16), (4, 25), (6, 64), (3, 9)])
def test_small_frame_equals_the_reference(R, S_):
    grey = _small_scene()
    T, H, W = grey.shape
    assert (T, H, W) == (5, 41, 57) and 2 * 25 + 1 > H and 2 * 64 + 1 > W and SMALL_CALLS[2][0] == T - 1
    pts = _small_points(H, W)
    assert len(pts) <= 64
    moved = gated = 0
    for tau_u, texture, c in COMBOS:
        q, back = SMALL_CALLS[c]
        want = Z.zm_track_ref(grey, pts, q, back, R, S_, TAU, tau_u, texture)
        got = _track_dev(grey, pts, q, back, R, S_, TAU, tau_u, texture)
        assert np.array_equal(got[2], want[2]), (tau_u, texture, q, back)
        assert np.array_equal(got[1], want[1]), (tau_u, texture, q, back)
        assert np.array_equal(got[0], want[0]), (tau_u, texture, q, back)
        moved += int((want[0] != pts[None].astype(np.float32)).any(-1).sum())
        gated += int((want[2] == 0).sum())
    assert gated > 0 and (moved > 0 or S_ < 4)                              # the flat ground is gated; 5 px per frame is beyond S = 1


def test_small_frame_extreme_thresholds_and_refresh_matters():
    grey = _small_scene()
    pts = _small_points(*grey.shape[1:])
    for R, S_, tau, tau_u, texture in ((7, 64, 255, 255, 127), (5, 16, 0, 0, 0), (1, 1, 0, -1, 1), (5, 25, 255, -1, 0)):
        for q, back in SMALL_CALLS[:2]:
            assert _same(_track_dev(grey, pts, q, back, R, S_, tau, tau_u, texture), Z.zm_track_ref(grey, pts, q, back, R, S_, tau, tau_u, texture))
    # a live template must part from the fixed one somewhere, else no case would tell a kernel that never refreshes
    outs = [Z.zm_track_ref(grey, pts, 0, False, 5, 16, TAU, u, 0) for u in (-1, TAU)]
    if _same(outs[0], outs[1]):
        drift = np.array(grey).astype(np.int64)
        for t in range(len(drift)):
            drift[t, ::2] += 6 * t                                           # every other row brightens: not an offset of the frame
        grey = np.clip(drift, 0, 255).astype(np.uint8)
        outs = [Z.zm_track_ref(grey, pts, 0, False, 5, 16, TAU, u, 0) for u in (-1, TAU)]
    assert not _same(outs[0], outs[1])
    for u, want in zip((-1, TAU), outs):
        assert _same(_track_dev(grey, pts, 0, False, 5, 16, TAU, u, 0), want)


def test_a_brightness_offset_changes_nothing_on_the_device():
    lit, plain = _small_scene(True), _small_scene(False)
    assert not np.array_equal(lit, plain) and np.array_equal(lit[0], plain[0])
    pts = _small_points(*lit.shape[1:])
    for R, S_, tau_u, texture in ((5, 16, -1, 4), (7, 64, 4, 0), (2, 25, TAU, 4)):
        for q, back in SMALL_CALLS[:3]:
            a = _track_dev(lit, pts, q, back, R, S_, TAU, tau_u, texture)
            b = _track_dev(plain, pts, q, back, R, S_, TAU, tau_u, texture)
            assert _same(a, b), (R, S_, tau_u, texture, q, back)
            assert a[1].sum() > a[1].shape[1]                               # points are visible beyond the query frame


def test_threshold_edges_through_the_export():
    R, S_ = Z.EDGE_R, Z.EDGE_S
    grey, pts = Z.edge_case()
    for tau, tau_u, tr, vs in ((16, -1, [[7, 6], [9, 7], [9, 7]], [1, 1, 0]), (15, -1, [[7, 6], [7, 6], [7, 6]], [1, 0, 0]),
                               (20, 16, [[7, 6], [9, 7], [11, 8]], [1, 1, 1]), (20, 15, [[7, 6], [9, 7], [9, 7]], [1, 1, 0])):
        got = _track_dev(grey, pts, 0, False, R, S_, tau, tau_u, 0)
        assert _same(got, Z.zm_track_ref(grey, pts, 0, False, R, S_, tau, tau_u, 0))
        assert got[0][:, 0].tolist() == tr and got[1][:, 0].tolist() == vs, (tau, tau_u)
    last = np.array([(11, 8)])
    for tau_u, tr, vs in ((16, [[7, 6], [9, 7], [11, 8]], [1, 1, 1]), (15, [[9, 7], [9, 7], [11, 8]], [0, 1, 1])):
        got = _track_dev(grey, last, 2, True, R, S_, 20, tau_u, 0)
        assert got[0][:, 0].tolist() == tr and got[1][:, 0].tolist() == vs, tau_u
    grey, pts = Z.dev_case()
    assert Z.dev(grey[0, 5:8, 5:8]) == 4 * 9
    for texture, k, vs in ((4, 1, [1, 1]), (5, 0, [1, 0])):
        got = _track_dev(grey, pts, 0, False, R, S_, 12, -1, texture)
        assert _same(got, Z.zm_track_ref(grey, pts, 0, False, R, S_, 12, -1, texture))
        assert got[2].tolist() == [k] and got[1][:, 0].tolist() == vs and got[0][:, 0].tolist() == [[6, 6], [6, 6]]


def test_the_largest_cost_through_the_export():
    grey, pts = Z.checker_case()
    for tau in (255, 0):
        got = _track_dev(grey, pts, 0, False, Z.CHECKER_R, Z.CHECKER_S, tau, -1, 4)
        assert _same(got, Z.zm_track_ref(grey, pts, 0, False, Z.CHECKER_R, Z.CHECKER_S, tau, -1, 4))
        assert got[2].all() and got[1].all() and np.array_equal(got[0][1], (pts + (0, -1)).astype(np.float32))


def test_tie_rule_and_flat_templates_at_the_widest_search():
    T, H, W, R, S_ = 4, 48, 64, 3, 64
    yy, xx = np.mgrid[0:H, 0:W]
    pts = np.concatenate([B.grid_ref(6, H, W), np.array([(0, 0), (W - 1, H - 1)])]).astype(np.int32)
    m = R + 2 * T + 4
    interior = (pts[:, 0] >= m) & (pts[:, 0] < W - m) & (pts[:, 1] >= m) & (pts[:, 1] < H - m)
    assert interior.sum() >= 4
    base = pts[None].astype(np.float32)

    def run(frames, q=0, back=False, tau_u=4, texture=0):
        got = _track_dev(frames, pts, q, back, R, S_, 12, tau_u, texture)
        assert _same(got, Z.zm_track_ref(frames, pts, q, back, R, S_, 12, tau_u, texture))
        return got

    flat = np.full((T, H, W), 93, np.uint8)
    flat[2:] = 201                                                           # and a jump in brightness, which costs nothing
    # gate off: every candidate inside the frame costs 0, d^2 = 0 wins although d^2 goes up to 2 * 64^2
    tr, vis, ok = run(flat, q=1, back=True)
    assert np.array_equal(tr, np.broadcast_to(base, tr.shape)) and vis.all() and ok.all()
    # gate on: the kernel leaves before any search, and still writes every frame of both directions
    for q, back in ((1, True), (0, False), (3, True), (2, False)):
        tr, vis, ok = run(flat, q=q, back=back, texture=4)
        assert not ok.any() and np.array_equal(tr, np.broadcast_to(base, tr.shape))
        assert vis[q].all() and vis.sum() == len(pts)
    stripes = lambda shift_x, shift_y: np.stack([(((xx - shift_x * t) % 4 < 2) * 200 + ((yy - shift_y * t) % 4 < 2) * 40 * (shift_y != 0)
                                                  + 3 * t).astype(np.uint8) for t in range(T)])
    # period-4 vertical stripes shifted by 2 px (and 3 grey levels brighter per frame): zero cost at every dx = 2 (mod 4) and every
    # dy; dx = -2 and +2 share d^2 = 4 and dy = 0: the smaller dx wins
    for tau_u in (4, -1):
        tr, vis, ok = run(stripes(2, 0), tau_u=tau_u, texture=4)
        assert ok[interior].all()
        for t in range(T):
            assert np.array_equal(tr[t, interior], (pts[interior] + (-2 * t, 0)).astype(np.float32)) and vis[t, interior].all()
    # a period-4 pattern in both axes shifted by (2, 2): (+-2, +-2) all cost 0 with d^2 = 8: the smaller dy, then the smaller dx
    tr, vis, ok = run(stripes(2, 2))
    for t in range(T):
        assert np.array_equal(tr[t, interior], (pts[interior] + (-2 * t, -2 * t)).astype(np.float32)) and vis[t, interior].all()


STAGE1_CALL = ("vid_a", 4, 3)                                # backward too; the object is absent in frames 6-8


def test_default_call_on_a_lit_scene_equals_the_reference():
    from s2d_amd.keymask.block_tracker import ZeroMeanBlockTracker
    name, q, obj = STAGE1_CALL
    assert STAGE1_CALL in B.CALLS
    pts, want_t, want_v, want_k = Z.reference_default_call(name, q, obj)
    assert want_k.all()
    video = torch.from_numpy(Z.video_f32(Z.lit_video(name))).cuda()[None]
    mask = torch.from_numpy(B.call_mask(name, q, obj))[None, None]
    tracker = ZeroMeanBlockTracker()
    tracks, vis = tracker(video, grid_size=50, grid_query_frame=q, segm_mask=mask, backward_tracking=True)
    assert tracks.shape == (1, want_t.shape[0], len(pts), 2) and tracks.dtype == torch.float32 and tracks.is_cuda
    assert vis.shape == tracks.shape[:3] and vis.dtype == torch.bool
    assert np.array_equal(tracker._grey.cpu().numpy(), Z.lit_grey(name))
    assert np.array_equal(vis[0].cpu().numpy(), want_v.astype(bool)) and np.array_equal(tracks[0].cpu().numpy(), want_t)
    assert not want_v.all() and want_v[[q - 1, q + 1]].any()


def test_gated_points_empty_results_and_the_grey_cache():
    from s2d_amd.keymask.block_tracker import ZeroMeanBlockTracker
    grey = Z.flat_grey()
    T, H, W = grey.shape
    video = torch.from_numpy(np.repeat(grey[:, None], 3, 1).astype(np.float32)).cuda()[None]      # r = g = b: the grey pass returns it
    both = torch.from_numpy(((S.label_map(Z.FLAT, 0) > 0) * 255).astype(np.uint8))[None, None]
    g = B.grid_ref(24, H, W)
    pts = g[both[0, 0].numpy()[g[:, 1], g[:, 0]] > 0]
    want_t, want_v, want_k = Z.zm_track_ref(grey, pts, 0, False, Z.R, 16, Z.TAU, -1, 4)
    assert 0 < want_k.sum() < len(pts)
    keep = want_k > 0
    tracker = ZeroMeanBlockTracker(search=16)
    empty_t, empty_v = tracker(video, grid_size=24, grid_query_frame=0, segm_mask=torch.zeros((1, 1, H, W), dtype=torch.uint8))
    assert empty_t.shape == (1, T, 0, 2) and empty_v.shape == (1, T, 0) and empty_v.dtype == torch.bool
    assert tracker._grey is None                                             # nothing was launched, not even the grey pass
    # the gate drops the columns of the flat object's points
    t1, v1 = tracker(video, grid_size=24, grid_query_frame=0, segm_mask=both)
    cached = tracker._grey
    assert np.array_equal(cached.cpu().numpy(), grey)
    assert t1.shape == (1, T, int(keep.sum()), 2) and v1.shape == (1, T, int(keep.sum())) and v1.dtype == torch.bool and t1.is_contiguous()
    assert np.array_equal(t1[0].cpu().numpy(), want_t[:, keep]) and np.array_equal(v1[0].cpu().numpy(), want_v[:, keep].astype(bool))
    # texture 0 keeps every column
    t0, v0 = ZeroMeanBlockTracker(search=16, texture=0)(video, grid_size=24, grid_query_frame=0, segm_mask=both)
    ref0 = Z.zm_track_ref(grey, pts, 0, False, Z.R, 16, Z.TAU, -1, 0)
    assert np.array_equal(t0[0].cpu().numpy(), ref0[0]) and np.array_equal(v0[0].cpu().numpy(), ref0[1].astype(bool))
    t2, v2 = tracker(video, grid_size=24, grid_query_frame=0, segm_mask=both)
    assert tracker._grey is cached and torch.equal(t1, t2) and torch.equal(v1, v2)      # the second call took the cached frames
    # every point dropped: a mask inside the flat object gives what the empty mask gives
    (by, bx, bh, bw) = Z.FLAT["objects"][0]["box"]
    inner = torch.zeros((1, 1, H, W), dtype=torch.uint8)
    inner[..., by + Z.R + 1:by + bh - Z.R - 1, bx + Z.R + 1:bx + bw - Z.R - 1] = 255
    assert (inner[0, 0].numpy()[g[:, 1], g[:, 0]] > 0).sum() >= 8
    t3, v3 = tracker(video, grid_size=24, grid_query_frame=0, segm_mask=inner)
    assert t3.shape == empty_t.shape and t3.dtype == empty_t.dtype and t3.device == empty_t.device
    assert v3.shape == empty_v.shape and v3.dtype == empty_v.dtype and v3.device == empty_v.device
    with pytest.raises(ValueError):
        tracker(video, grid_size=24, segm_mask=torch.zeros((1, 1, W, H), dtype=torch.uint8))


@pytest.mark.parametrize("bad", [dict(S_=65), dict(S_=0), dict(R=8), dict(R=0), dict(tau_u=13), dict(tau_u=-2), dict(q=5), dict(q=-1),
                                 dict(tau=256), dict(tau=-1, tau_u=-1), dict(texture=128), dict(texture=-1)])
def test_export_refuses(bad):
    # every case is refused by the argument check in front of the launch
    grey = _small_scene()
    kw = dict(q=0, backward=False, R=5, S_=16, tau=12, tau_u=4, texture=4)
    assert grey.shape[0] == 5 and kw["tau"] + 1 == 13
    kw.update(bad)
    with pytest.raises(RuntimeError):
        _track_dev(grey, _small_points(*grey.shape[1:]), **kw)


def test_no_points_is_no_launch():
    got = _track_dev(_small_scene(), np.zeros((0, 2), np.int32), 0, False, 5, 16, 12, 4, 4)
    assert got[0].shape == (5, 0, 2) and got[1].shape == (5, 0) and got[2].shape == (0,)


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


def _annotations(work):
    return {os.path.basename(p): json.load(open(p)) for p in sorted(glob.glob(os.path.join(work, "annotations", "*.json")))}


def _figures(work):
    return {name: {"annotations": len(doc["annotations"]),
                   "frames_covered": [sum(s is not None for s in a["segmentations"]) for a in doc["annotations"]]}
            for name, doc in _annotations(work).items()}


def test_discovery_end_to_end_is_blind_to_the_lighting(tmp_path):
    works = {}
    for kind in ("lit", "squeezed"):
        works[kind] = str(tmp_path / kind)
        os.makedirs(works[kind])
        Z.write_dataset(works[kind], lit=kind == "lit")
    options = ["--tracker", "block-zm", "--tracker-options", "search=16,texture=4"]
    reports = {kind: _discover(works[kind], extra=options) for kind in works}
    for kind, rep in reports.items():
        assert (rep["videos"], rep["done"], rep["failed"]) == (2, 2, 0), (kind, rep)
    lit, plain = _annotations(works["lit"]), _annotations(works["squeezed"])
    assert sorted(lit) == sorted(plain) == [name + ".json" for name in sorted(S.SCENES)]
    for name in lit:
        assert lit[name] == plain[name], name
        assert len(lit[name]["annotations"]) >= 1, name
    out = os.environ.get("S2D_ZM_TRACKER_FIGURES")                             # a measurement: recorded, not asserted
    if out:
        figures = {"block-zm": _figures(works["lit"])}
        for kind, extra, tracker in (("block-live", ["--tracker", "block-live", "--tracker-options", "search=16"], None),
                                     ("truth", [], Z.LitTruthTracker())):
            work = str(tmp_path / kind)
            os.makedirs(work)
            Z.write_dataset(work, lit=True)
            rep = _discover(work, tracker=tracker, extra=extra)
            figures[kind] = {"report": {k: rep[k] for k in ("done", "skipped", "failed")}, **_figures(work)}
        with open(out, "w") as f:
            json.dump(figures, f, indent=1)
