"""The zero-mean tracker without a GPU: the numpy restatement of its kernel (tests/zm_tracker_ref.py) against the ground truth of
the lit scenes (the textured scenes under a brightness offset of up to 40 grey levels that changes sign from frame to frame),
against itself on the same scenes without the offsets, against the fixed-template rule, which loses most of those point-frames,
on a flat object, where the texture gate decides, at the edges of its three thresholds and at its largest cost; and the host-side
wiring (tracker spec, options, command line).

What the tracker can guarantee is what tests/test_block_tracker_refs_cpu.py states -- at a continuously clean point-frame the true
position costs 0 and nothing undercuts it -- and a whole-frame offset does not change a single cost.
tests/test_gpu_zm_tracker.py then holds the device to this reference bit for bit."""
import numpy as np
import pytest
import torch

from tests import block_tracker_ref as B
from tests import zm_tracker_ref as Z


def test_the_lit_scenes_hold_what_they_must():
    assert [Z.light(t) for t in range(10)] == [0, -5, 10, -15, 20, -25, 30, -35, 40, -40]
    for name in ("vid_a", "vid_b"):
        sq, lit = Z.squeezed_video(name).astype(np.int64), Z.lit_video(name).astype(np.int64)
        assert sq.min() >= 48 and sq.max() <= 207 and lit.min() >= 8 and lit.max() <= 247
        assert np.array_equal(sq, 48 + (B.textured_video(name).astype(np.int64) * 5) // 8)
        for t in range(len(sq)):
            assert np.array_equal(lit[t], sq[t] + Z.light(t))
        g = Z.lit_grey(name).astype(np.int64)                                    # asserts the exact grey offset itself
        assert max(abs(int(g[t].mean() - g[0].mean())) for t in range(len(g))) > Z.TAU


@pytest.mark.parametrize("name", ["vid_a", "vid_b"])
def test_lit_calls_equal_the_truth_and_the_unlit_run_where_the_plain_cost_does_not(name):
    total = total_old = 0
    for vid, q, obj in B.CALLS:
        if vid != name:
            continue
        back = q > 0                                                             # forward, and backward too from a later query frame
        pts, tracks, vis, trackable = Z.reference_call("lit", vid, q, obj)
        _, tracks0, vis0, trackable0 = Z.reference_call("squeezed", vid, q, obj)
        assert np.array_equal(tracks, tracks0) and np.array_equal(vis, vis0) and np.array_equal(trackable, trackable0), (vid, q, obj)
        assert trackable.all(), (vid, q, obj)                                    # no point of a textured object is gated at texture 4
        tr = B.truth(vid, q, pts, obj).astype(np.float32)
        cl = B.clean(vid, q, pts, obj, back, S_=Z.LIT_SEARCH)
        after = cl.copy()
        after[q] = False
        assert after.any(), (vid, q, obj)
        assert np.array_equal(tracks[cl], tr[cl]) and vis[cl].all(), (vid, q, obj)
        if not back:
            assert np.array_equal(tracks[:q], np.broadcast_to(pts.astype(np.float32), tracks[:q].shape)) and not vis[:q].any()
        old_t, old_v = B.block_track_ref(Z.lit_grey(vid), pts, q, back)           # the plain cost, fixed template, same R, S, tau
        old_exact = int(((old_t == tr).all(-1) & (old_v > 0))[cl].sum())
        assert old_exact < int(cl.sum()), (vid, q, obj)
        total += int(cl.sum())
        total_old += old_exact
    print(f"{name}: {total} continuously clean point-frames exact and visible under the offsets; the plain cost: {total_old}")
    assert total > 1000


def test_the_texture_gate_on_a_flat_object():
    grey = Z.flat_grey()
    T = grey.shape[0]
    flat, tex = Z.flat_points(0), Z.flat_points(1)
    # interior: the patch round the query position shows the flat object in every frame, although the object moves on
    (by, bx, bh, bw), (sy, sx) = Z.FLAT["objects"][0]["box"], Z.FLAT["objects"][0]["step"]
    assert sy == 0 and sx == 3
    interior = ((flat[:, 0] - Z.R >= bx + sx * (T - 1)) & (flat[:, 0] + Z.R < bx + bw) & (flat[:, 1] - Z.R >= by) & (flat[:, 1] + Z.R < by + bh))
    assert interior.sum() >= 8 and len(tex) >= 8
    pts = np.concatenate([flat, tex])
    is_tex = np.arange(len(pts)) >= len(flat)
    truth = np.concatenate([Z.flat_truth(0, flat, 0), Z.flat_truth(0, tex, 1)], 1).astype(np.float32)
    clean = np.concatenate([Z.flat_clean(0, flat, 0), Z.flat_clean(0, tex, 1)], 1)
    assert clean[-1, :len(flat)][interior].any() and clean[-1, is_tex].any()
    # gate off: a point inside the flat object finds cost 0 where it stands, stays, and is called visible -- not at the truth
    t0, v0, k0 = Z.zm_track_ref(grey, pts, 0, False, Z.R, 16, Z.TAU, -1, 0)
    assert k0.all()
    inner = np.flatnonzero(~is_tex)[interior]
    assert v0[:, inner].all() and np.array_equal(t0[:, inner], np.broadcast_to(pts[inner].astype(np.float32), t0[:, inner].shape))
    assert (t0[1:, inner] != truth[1:, inner]).any(-1).all()
    # gate at 4: they are untrackable (p in every frame, visible in the query frame only); what remains is exact where clean
    t4, v4, k4 = Z.zm_track_ref(grey, pts, 0, False, Z.R, 16, Z.TAU, -1, 4)
    assert not k4[inner].any() and k4[is_tex].all()
    gone = k4 == 0
    assert np.array_equal(t4[:, gone], np.broadcast_to(pts[gone].astype(np.float32), t4[:, gone].shape))
    assert v4[0, gone].all() and not v4[1:, gone].any()
    keep = clean & (k4 > 0)[None]
    assert keep[1:].sum() >= 4 * (T - 1)
    assert np.array_equal(t4[keep], truth[keep]) and v4[keep].all()
    assert np.array_equal(t4[:, ~gone], t0[:, ~gone]) and np.array_equal(v4[:, ~gone], v0[:, ~gone])      # the gate changes nothing else


def test_the_threshold_edges():
    R, S_ = Z.EDGE_R, Z.EDGE_S
    n = (2 * R + 1) ** 2
    grey, pts = Z.edge_case()
    p0, p1, p2 = (Z.edge_patch(grey, t) for t in range(3))
    assert Z.zcost(p0, p1) == 16 * n == Z.zcost(p1, p2) and Z.zcost(p0, p2) == 28 * n
    run = lambda tau, tau_u, texture=0: tuple(a[:, 0].tolist() for a in Z.zm_track_ref(grey, pts, 0, False, R, S_, tau, tau_u, texture)[:2])
    # cost == tau n: visible; one less: not
    assert run(16, -1) == ([[7, 6], [9, 7], [9, 7]], [1, 1, 0])
    assert run(15, -1) == ([[7, 6], [7, 6], [7, 6]], [1, 0, 0])
    # cost == tau_u n: refreshed, so frame 2 costs 16 n against the frame-1 patch; one less: kept, and 28 n > 20 n hides it
    assert run(20, 16) == ([[7, 6], [9, 7], [11, 8]], [1, 1, 1])
    assert run(20, 15) == ([[7, 6], [9, 7], [9, 7]], [1, 1, 0])
    assert run(20, -1) == run(20, 15)
    # backward from the last frame: the mirror image, from the frame-2 patch
    back = lambda tau, tau_u: tuple(a[:, 0].tolist() for a in Z.zm_track_ref(grey, np.array([(11, 8)]), 2, True, R, S_, tau, tau_u, 0)[:2])
    assert back(20, 16) == ([[7, 6], [9, 7], [11, 8]], [1, 1, 1])
    assert back(20, 15) == ([[9, 7], [9, 7], [11, 8]], [0, 1, 1])
    # dev == texture n: trackable; one more: not
    grey, pts = Z.dev_case()
    assert Z.dev(grey[0, 5:8, 5:8]) == 4 * n
    t, v, k = Z.zm_track_ref(grey, pts, 0, False, R, S_, 12, -1, 4)
    assert k.tolist() == [1] and v[:, 0].tolist() == [1, 1]
    t, v, k = Z.zm_track_ref(grey, pts, 0, False, R, S_, 12, -1, 5)
    assert k.tolist() == [0] and v[:, 0].tolist() == [1, 0] and t[:, 0].tolist() == [[6, 6], [6, 6]]


def test_the_largest_cost_orders_in_the_key():
    R, S_ = Z.CHECKER_R, Z.CHECKER_S
    n = (2 * R + 1) ** 2
    grey, pts = Z.checker_case()
    a = grey[0, :2 * R + 1, :2 * R + 1]
    top = Z.zcost(a, 255 - a)
    assert top == Z.zcost(255 - a, a) == 113 * 254 + 112 * 256 and 1 << 15 < top < 1 << 17 and top <= 255 * n
    # displacement 0 costs `top`, within tau n at tau = 255, and still loses to cost 0 at d^2 = 1: smallest dy, then dx
    for tau in (255, 0):
        t, v, k = Z.zm_track_ref(grey, pts, 0, False, R, S_, tau, -1, 4)
        assert k.all() and v.all() and np.array_equal(t[1], (pts + (0, -1)).astype(np.float32))
    assert 510 * n < 1 << 17                                                     # the bound of the rule, whatever the patches


def test_a_constant_offset_changes_no_cost_and_a_gain_does():
    rng = np.random.default_rng(5)
    for P in (3, 11, 15):
        a, b = rng.integers(40, 200, (P, P)), rng.integers(40, 200, (P, P))
        assert Z.zcost(a, b + 37) == Z.zcost(a, b) == Z.zcost(a - 40, b) and Z.zcost(a, a + 55) == 0
        assert Z.zcost(a, (a * 3) // 2) > 0                                      # contrast is not removed
    assert Z.mean(np.array([4, 5, 13, 14]), 9).tolist() == [0, 1, 1, 2]          # 4/9 -> 0, 5/9 -> 1, 13/9 -> 1, 14/9 -> 2
    assert int(Z.mean(np.array([1]), 2)[0]) == 1                                 # a half rounds up


def test_reference_refuses_what_the_export_refuses():
    grey = np.zeros((2, 8, 8), np.uint8)
    for kw in (dict(S=65), dict(S=0), dict(R=8), dict(R=0), dict(tau_u=13), dict(tau_u=-2), dict(q=2), dict(q=-1), dict(tau=256),
               dict(tau=-1, tau_u=-1), dict(texture=-1), dict(texture=128)):
        with pytest.raises(ValueError):
            Z.zm_track_ref(grey, np.array([(1, 1)]), **{**dict(q=0, backward=False, R=5, S=16, tau=12, tau_u=4, texture=4), **kw})


# ---------------------------------------------------------------------------------------------------------------- host wiring
def test_load_tracker_block_zm_and_options():
    from s2d_amd.keymask.block_tracker import BlockTracker, LiveBlockTracker, ZeroMeanBlockTracker
    from s2d_amd.keymask.tracker import load_tracker
    t = load_tracker("block-zm")
    assert isinstance(t, ZeroMeanBlockTracker) and isinstance(t, BlockTracker) and not isinstance(t, LiveBlockTracker) and t.cuda() is t
    assert (t.radius, t.search, t.tau, t.refresh, t.texture) == (Z.R, Z.SEARCH, Z.TAU, Z.REFRESH, Z.TEXTURE) == (5, 32, 12, -1, 4)
    t = load_tracker("block-zm", options={"search": 48, "texture": 0})
    assert (t.radius, t.search, t.tau, t.refresh, t.texture) == (5, 48, 12, -1, 0)
    t = load_tracker("block-zm", None, {"radius": 3, "tau": 20, "refresh": 4})
    assert (t.radius, t.search, t.tau, t.refresh, t.texture) == (3, 32, 20, 4, 4)
    with pytest.raises(ValueError):
        load_tracker("block-zm", options={"pyramid": 3})
    # the other two keep their options and have no texture
    for spec in ("block", "block-live"):
        assert not hasattr(load_tracker(spec), "texture")
        with pytest.raises(ValueError):
            load_tracker(spec, options={"texture": 4})
    with pytest.raises(ValueError):
        load_tracker("cotracker", options={"texture": 4})
    with pytest.raises(ValueError):
        load_tracker("block-zm:")


def test_the_command_line():
    from s2d_amd.keymask import discover
    a = discover.parse_args(["--tracker", "block-zm", "--tracker-options", "search=48,refresh=4,texture=0"])
    assert a.tracker == "block-zm"
    assert discover.parse_tracker_options(a.tracker_options) == {"search": 48, "refresh": 4, "texture": 0}
    import io
    from contextlib import redirect_stdout
    buf = io.StringIO()
    with pytest.raises(SystemExit), redirect_stdout(buf):
        discover.parse_args(["--help"])
    assert "block-zm" in buf.getvalue() and "texture" in buf.getvalue()


def test_zm_tracker_refuses_a_segm_mask_of_another_size():
    from s2d_amd.keymask.block_tracker import ZeroMeanBlockTracker
    video = torch.zeros((1, 3, 3, 20, 30))
    with pytest.raises(ValueError):
        ZeroMeanBlockTracker()(video, grid_size=4, segm_mask=torch.zeros((1, 1, 30, 20), dtype=torch.uint8))
