"""The live-template tracker without a GPU: the numpy restatement of its kernel (tests/live_tracker_ref.py) against the
fixed-template restatement, against the ground truth of the textured scenes and of the FAST and DRIFT scenes, the refresh rule on
a hand-built case, and the host-side wiring (tracker spec, options, command line).

What the tracker can guarantee is what tests/test_block_tracker_refs_cpu.py states: at a continuously clean point-frame the
true position costs 0 (in DRIFT: far less than any other position) and nothing undercuts it.  FAST and DRIFT are built so that
the fixed-template rule with its defaults loses such point-frames (motion beyond its search radius, appearance drifting past
tau), which each test checks, so the scenes exercise what is new.  tests/test_gpu_live_tracker.py then holds the device to this
reference bit for bit."""
import numpy as np
import pytest
import torch

from tests import block_tracker_ref as B
from tests import live_tracker_ref as L


def test_without_refresh_the_reference_is_the_fixed_template_reference():
    for name, q, obj in B.CALLS:
        pts, want_t, want_v = B.reference_call(name, q, obj)
        got_t, got_v = L.live_track_ref(B.textured_grey(name), pts, q, q > 0, B.R, 16, B.TAU, -1)
        assert np.array_equal(got_v, want_v), (name, q, obj)
        assert np.array_equal(got_t, want_t), (name, q, obj)


def test_small_frame_window_larger_than_the_frame_equals_the_fixed_template_reference():
    # the reference's window of absolute positions against the fixed-template reference's window of displacements where the
    # search window exceeds the frame (24 is the largest radius the latter is defined for)
    rng = np.random.default_rng(3)
    grey = rng.integers(0, 256, (4, 19, 31), dtype=np.uint8)
    grey[1:, 3:15, 4:20] = grey[0, 2:14, 1:17]
    pts = np.concatenate([B.grid_ref(5, 19, 31), np.array([(0, 0), (30, 18), (30, 0), (0, 18)])])
    for q, back in ((0, False), (2, True)):
        want = B.block_track_ref(grey, pts, q, back, 3, 24, 40)
        got = L.live_track_ref(grey, pts, q, back, 3, 24, 40, -1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", ["vid_a", "vid_b"])
def test_defaults_equal_the_truth_on_the_textured_scenes(name):
    n_clean = n_replaced = 0
    for vid, q, obj in B.CALLS:
        if vid != name:
            continue
        pts, tracks, vis = L.reference_default_call(vid, q, obj)
        back = q > 0
        tr = B.truth(vid, q, pts, obj)
        cl = B.clean(vid, q, pts, obj, back, S_=L.SEARCH)
        assert cl[q].any(), (vid, q, obj)
        assert np.array_equal(tracks[cl], tr[cl].astype(np.float32)), (vid, q, obj)
        assert vis[cl].all(), (vid, q, obj)
        rp = B.replaced(vid, q, pts, obj, back)
        assert not vis[rp].any(), (vid, q, obj)
        if not back:
            assert np.array_equal(tracks[:q], np.broadcast_to(pts.astype(np.float32), tracks[:q].shape)) and not vis[:q].any()
        n_clean += int(cl.sum())
        n_replaced += int(rp.sum())
    print(f"{name}: {n_clean} continuously clean point-frames exact and visible, {n_replaced} replaced point-frames invisible")
    assert n_clean > 1000 and n_replaced > 0


@pytest.mark.parametrize("name,calls,search", [("fast", L.FAST_CALLS, L.FAST_SEARCH), ("drift", L.DRIFT_CALLS, L.DRIFT_SEARCH)])
def test_fast_and_drift_equal_the_truth_where_the_fixed_template_rule_does_not(name, calls, search):
    assert any(q == 0 for q, _ in calls) and any(0 < q < L.SCENES[name]["T"] - 1 for q, _ in calls)
    total = total_old = 0
    for q, obj in calls:
        pts, tracks, vis = L.reference_call(name, q, obj)
        back = q > 0
        tr = L.truth(name, q, pts, obj).astype(np.float32)
        cl = L.clean(name, q, pts, obj, back, S_=search)
        after = cl.copy()
        after[q] = False
        assert after.any(), (name, q, obj)                                      # clean point-frames beyond the query frame
        assert np.array_equal(tracks[cl], tr[cl]), (name, q, obj)
        assert vis[cl].all(), (name, q, obj)
        old_t, old_v = B.block_track_ref(L.scene_grey(name), pts, q, back)       # the fixed-template rule with its defaults
        old_exact = int(((old_t == tr).all(-1) & (old_v > 0))[cl].sum())
        assert old_exact < int(cl.sum()), (name, q, obj)
        total += int(cl.sum())
        total_old += old_exact
    print(f"{name}: {total} continuously clean point-frames exact and visible; the fixed-template rule (search 16): {total_old}")


def test_the_scenes_hold_what_they_must():
    fast, drift = L.SCENES["fast"], L.SCENES["drift"]
    assert (fast["H"], fast["W"]) == (120, 216) and fast["T"] >= 6 and drift["T"] == 10
    steps = [max(abs(s) for s in o["step"]) for o in fast["objects"]]
    assert sum(s > 24 for s in steps) >= 2 and sum(s == 0 for s in steps) >= 1 and max(steps) <= L.FAST_SEARCH
    assert all(5 <= max(abs(s) for s in o["step"]) <= 7 for o in drift["objects"])
    # DRIFT: inside an object every 2 x 2 cell changes by one fixed integer in -3..3 per frame until it clips
    v = L.scene_video("drift").astype(np.int64)
    o = drift["objects"][0]
    (y, x, h, w), (dy, dx) = o["box"], o["step"]
    a, b, c = (v[t, y + dy * t:y + dy * t + h, x + dx * t:x + dx * t + w] for t in (0, 1, 2))
    d = b - a
    assert d.min() >= -3 and d.max() <= 3 and len(np.unique(d)) == 7
    free = lambda *frames: np.logical_and.reduce([((f > 0) & (f < 255)).all(-1) for f in frames])      # no channel has clipped
    u = free(a, b)
    assert u.mean() > 0.9 and (d[u] == d[u][:, :1]).all()                        # one integer for the three channels
    both = u[0::2, 0::2] & u[1::2, 1::2]
    assert np.array_equal(d[0::2, 0::2][both], d[1::2, 1::2][both])              # and for the 2 x 2 cell
    u = free(a, b, c)
    assert np.array_equal((c - b)[u], d[u])                                      # fixed from frame to frame
    # FAST keeps its textures
    o = fast["objects"][1]
    (y, x, h, w), (dy, dx) = o["box"], o["step"]
    f = L.scene_video("fast")
    assert np.array_equal(f[0, y:y + h, x:x + w], f[1, y + dy:y + dy + h, x + dx:x + dx + w])


def test_the_refresh_rule_in_isolation():
    """R = 1, tau = 12, tau_u = 4: a 3 x 3 textured patch on black moves by (2, 1) per frame and every pixel of it gains 8 per
    frame.  Frame 1 costs 72 against the query patch, between tau_u * 9 = 36 and tau * 9 = 108: visible, not refreshed.  Frame 2
    costs 144 against the query patch (invisible) and 72 against the frame-1 patch (visible)."""
    R, S_, tau, tau_u = 1, 4, 12, 4
    patch = np.array([[90, 140, 60], [150, 100, 170], [70, 160, 120]], np.int64)
    grey = np.zeros((3, 16, 20), np.uint8)
    for t in range(3):
        grey[t, 5 + t:8 + t, 6 + 2 * t:9 + 2 * t] = patch + 8 * t
    pts = np.array([(7, 6)])
    at = lambda t: grey[t, 5 + t:8 + t, 6 + 2 * t:9 + 2 * t].astype(np.int64)
    cost1 = int(np.abs(at(1) - at(0)).sum())
    assert tau_u * 9 < cost1 < tau * 9
    assert int(np.abs(at(2) - at(0)).sum()) > tau * 9 >= int(np.abs(at(2) - at(1)).sum())
    kept_t, kept_v = L.live_track_ref(grey, pts, 0, False, R, S_, tau, tau_u)             # frame 1 is not good enough to refresh
    live_t, live_v = L.live_track_ref(grey, pts, 0, False, R, S_, tau, tau)               # refreshed at every visible frame
    assert kept_v[:, 0].tolist() == [1, 1, 0] and kept_t[:, 0].tolist() == [[7, 6], [9, 7], [9, 7]]
    assert live_v[:, 0].tolist() == [1, 1, 1] and live_t[:, 0].tolist() == [[7, 6], [9, 7], [11, 8]]
    never = L.live_track_ref(grey, pts, 0, False, R, S_, tau, -1)
    assert np.array_equal(never[0], kept_t) and np.array_equal(never[1], kept_v)
    # backward from the last frame the two directions are independent and start from the query patch: the mirror image
    back_t, back_v = L.live_track_ref(grey, np.array([(11, 8)]), 2, True, R, S_, tau, tau)
    assert back_v[:, 0].tolist() == [1, 1, 1] and back_t[:, 0].tolist() == [[7, 6], [9, 7], [11, 8]]
    back_t, back_v = L.live_track_ref(grey, np.array([(11, 8)]), 2, True, R, S_, tau, tau_u)
    assert back_v[:, 0].tolist() == [0, 1, 1] and back_t[:, 0].tolist() == [[9, 7], [9, 7], [11, 8]]


def test_reference_refuses_what_the_export_refuses():
    grey = np.zeros((2, 8, 8), np.uint8)
    for kw in (dict(S=65), dict(S=0), dict(R=8), dict(tau_u=13), dict(tau_u=-2), dict(q=2), dict(tau=256)):
        with pytest.raises(ValueError):
            L.live_track_ref(grey, np.array([(1, 1)]), **{**dict(q=0, backward=False, R=5, S=16, tau=12, tau_u=4), **kw})


# ---------------------------------------------------------------------------------------------------------------- host wiring
def test_load_tracker_block_live_and_options():
    from s2d_amd.keymask.block_tracker import BlockTracker, LiveBlockTracker
    from s2d_amd.keymask.tracker import load_tracker
    t = load_tracker("block-live")
    assert isinstance(t, LiveBlockTracker) and isinstance(t, BlockTracker) and t.cuda() is t
    assert (t.radius, t.search, t.tau, t.refresh) == (L.R, L.SEARCH, L.TAU, L.REFRESH) == (5, 32, 12, 4)
    t = load_tracker("block-live", options={"search": 48, "refresh": -1})
    assert (t.radius, t.search, t.tau, t.refresh) == (5, 48, 12, -1)
    t = load_tracker("block-live", None, {"radius": 3, "tau": 20})
    assert (t.radius, t.search, t.tau, t.refresh) == (3, 32, 20, 4)
    # "block" is unchanged, takes its own options and has no refresh
    t = load_tracker("block")
    assert type(t) is BlockTracker and (t.radius, t.search, t.tau) == (B.R, B.SEARCH, B.TAU) and not hasattr(t, "refresh")
    t = load_tracker("block", options={"search": 24})
    assert type(t) is BlockTracker and (t.radius, t.search, t.tau) == (5, 24, 12)
    assert type(load_tracker("block", options={})) is BlockTracker
    with pytest.raises(ValueError):
        load_tracker("block", options={"refresh": 4})
    with pytest.raises(ValueError):
        load_tracker("block-live", options={"pyramid": 3})
    with pytest.raises(ValueError):
        load_tracker("cotracker", "scaled_offline.pth", {"search": 48})
    with pytest.raises(ValueError):
        load_tracker("cotracker", options={"search": 48})


def test_the_command_line():
    from s2d_amd.keymask import discover
    a = discover.parse_args(["--tracker", "block-live", "--tracker-options", "search=48,refresh=-1"])
    assert a.tracker == "block-live" and discover.parse_tracker_options(a.tracker_options) == {"search": 48, "refresh": -1}
    a = discover.parse_args([])
    assert a.tracker == "cotracker" and a.tracker_options is None and discover.parse_tracker_options(a.tracker_options) == {}
    assert discover.parse_tracker_options("") == {}
    assert discover.parse_tracker_options(" tau = 20 , radius=3 ") == {"tau": 20, "radius": 3}
    for bad in ("search", "search=", "search=4.5", "=3", "search=48;refresh=1", "search=forty"):
        with pytest.raises(ValueError):
            discover.parse_tracker_options(bad)
    import io
    from contextlib import redirect_stdout
    buf = io.StringIO()
    with pytest.raises(SystemExit), redirect_stdout(buf):
        discover.parse_args(["--help"])
    assert "block-live" in buf.getvalue() and "--tracker-options" in buf.getvalue()


def test_live_tracker_refuses_a_segm_mask_of_another_size():
    from s2d_amd.keymask.block_tracker import LiveBlockTracker
    video = torch.zeros((1, 3, 3, 20, 30))
    with pytest.raises(ValueError):
        LiveBlockTracker()(video, grid_size=4, segm_mask=torch.zeros((1, 1, 30, 20), dtype=torch.uint8))
