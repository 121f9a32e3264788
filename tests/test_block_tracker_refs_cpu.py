"""The block tracker without a GPU: the numpy restatement of its kernels (tests/block_tracker_ref.py) against the ground truth of
the textured scenes, and the host-side wiring (grid, tracker spec, command line, argument check).

The guarantee checked here is the one the tracker can give: at a continuously clean point-frame the true position costs 0, which
no other candidate undercuts, and (cost, d^2, dy, dx) prefers it unless another candidate also costs 0 nearer by, i.e. unless the
random texture repeats.  tests/test_gpu_block_tracker.py then holds the device to this reference bit for bit."""
import numpy as np
import pytest
import torch

from tests import block_tracker_ref as B
from tests.golden import keymask_stub_tracker as S


@pytest.mark.parametrize("name", ["vid_a", "vid_b"])
def test_reference_equals_the_truth_where_it_is_guaranteed(name):
    n_clean = n_replaced = 0
    for vid, q, obj in B.CALLS:
        if vid != name:
            continue
        pts, tracks, vis = B.reference_call(vid, q, obj)
        assert len(pts) > 0
        back = q > 0
        tr = B.truth(vid, q, pts, obj)
        cl = B.clean(vid, q, pts, obj, back)
        assert cl[q].any(), (vid, q, obj)                                        # the call has interior points at all
        assert np.array_equal(tracks[cl], tr[cl].astype(np.float32)), (vid, q, obj)
        assert vis[cl].all(), (vid, q, obj)
        rp = B.replaced(vid, q, pts, obj, back)
        assert not vis[rp].any(), (vid, q, obj)
        if not back:                                                            # frames before the query frame: the point, invisible
            assert np.array_equal(tracks[:q], np.broadcast_to(pts.astype(np.float32), tracks[:q].shape)) and not vis[:q].any()
        n_clean += int(cl.sum())
        n_replaced += int(rp.sum())
    print(f"{name}: {n_clean} continuously clean point-frames exact and visible, {n_replaced} replaced point-frames invisible")
    assert n_clean > 1000 and n_replaced > 0


def test_the_subset_holds_the_cases_it_must():
    calls = set(B.CALLS)
    assert any(v == "vid_b" and o == 0 for v, q, o in calls) and any(v == "vid_a" and o == 3 and q < 6 for v, q, o in calls)
    assert any(v == "vid_a" and o == 2 for v, q, o in calls) and any(q > 0 for v, q, o in calls)
    # vid_b object 0 is covered by object 4 in later frames; vid_a object 3 is gone in frames 6-8: both must show as replaced
    pts = B.call_points("vid_b", 0, 0)
    assert B.replaced("vid_b", 0, pts, 0, False)[1:].any()
    pts = B.call_points("vid_a", 0, 3)
    assert B.replaced("vid_a", 0, pts, 3, False)[6:9].any()
    # 12 px per frame lies inside the search radius, so object 2 of vid_a has clean point-frames after the query frame
    pts = B.call_points("vid_a", 0, 2)
    assert S.SCENES["vid_a"]["objects"][2]["step"] == (0, 12) and B.clean("vid_a", 0, pts, 2, False)[1:].any()


def test_grey_reference_rounds_half_to_even_and_clamps():
    v = np.zeros((1, 3, 1, 8), np.float32)
    v[0, :, 0] = np.array([0.5, 1.5, 2.5, 254.5, -3, 300, np.nan, np.inf], np.float32)
    assert B.grey_ref(v)[0, 0].tolist() == [0, 2, 2, 254, 0, 255, 0, 255]
    v = np.zeros((1, 3, 1, 1), np.float32)
    v[0, :, 0, 0] = (200, 100, 50)
    assert int(B.grey_ref(v)[0, 0, 0]) == (77 * 200 + 150 * 100 + 29 * 50 + 128) >> 8


@pytest.mark.parametrize("g,H,W", [(50, 120, 216), (25, 120, 216), (50, 480, 854), (7, 37, 53)])
def test_grid_points_is_the_stub_grid(g, H, W):
    from s2d_amd.keymask.block_tracker import grid_points
    got = grid_points(g, H, W)
    assert got.dtype == np.int32 and got.shape == (g * g, 2)
    assert np.array_equal(got, B.grid_ref(g, H, W))
    assert (got[:, 0] < W).all() and (got[:, 1] < H).all() and (got >= 0).all()


def test_load_tracker_block_and_the_command_line():
    from s2d_amd.keymask import discover
    from s2d_amd.keymask.block_tracker import BlockTracker
    from s2d_amd.keymask.tracker import load_tracker
    t = load_tracker("block")
    assert isinstance(t, BlockTracker) and (t.radius, t.search, t.tau) == (B.R, B.SEARCH, B.TAU) and t.cuda() is t
    assert discover.parse_args(["--tracker", "block"]).tracker == "block"
    assert discover.parse_args([]).tracker == "cotracker"                     # the default stays


def test_segm_mask_of_another_size_is_refused():
    from s2d_amd.keymask.block_tracker import BlockTracker
    video = torch.zeros((1, 3, 3, 20, 30))
    with pytest.raises(ValueError):
        BlockTracker()(video, grid_size=4, segm_mask=torch.zeros((1, 1, 30, 20), dtype=torch.uint8))
