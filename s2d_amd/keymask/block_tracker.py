"""The built-in point tracker of keymask discovery: integer block matching on grey frames (csrc/block_track.hip).

    tracker = BlockTracker(radius=5, search=16, tau=12)            # load_tracker("block"), --tracker block
    pred_tracks, pred_visibility = tracker(video, grid_size=g, grid_query_frame=f, segm_mask=m, backward_tracking=b)

A baseline, not a CoTracker replacement: its quality against CoTracker is unmeasured.  Each point keeps the (2 radius + 1)^2
grey patch round it in the query frame as its template; in every further frame the patch with the smallest sum of absolute
differences within `search` pixels of the point's last good position is taken, and the point is visible there when the mean
absolute difference is at most `tau`.  Limits: motion above `search` pixels per frame loses the point; the template is never
updated, so appearance change (lighting, scale, rotation) makes a point invisible; positions are whole pixels.  The consumers
of the tracks round them to pixels anyway (s2d_track_point_id_counts) and stage 1 reads only the mean visibility.

The exact rule is in include/s2d_hip.h (s2d_video_grey_u8, s2d_block_track_u8); tests/block_tracker_ref.py restates it in
numpy, bit for bit.

    tracker = LiveBlockTracker(radius=5, search=32, tau=12, refresh=4)   # load_tracker("block-live"), --tracker block-live

lifts two of these limits with the same search (s2d_block_track_live_u8, restated in tests/live_tracker_ref.py): `search` goes
up to 64 pixels, and the template is live -- after a frame where the point is visible with a mean absolute difference of at
most `refresh`, the patch round the new position becomes the template (-1: never, the fixed template; `tau`: at every visible
frame).  The defaults are design choices, not tuned on real video: an exhaustive search costs with the number of candidates, so
search 32 is about 4 times the work of search 16 and search 64 about 15 times; refresh 4 is a third of `tau`, so that only a
close match may replace the template.  Limits that stay: whole-pixel positions; drift -- a live template can slide off its object
step by step, and nothing anchors it to the query frame; untextured regions match anywhere; a sudden appearance change above
`tau` still hides the point; quality against CoTracker is unmeasured.

    tracker = ZeroMeanBlockTracker(radius=5, search=32, tau=12, refresh=-1, texture=4)   # load_tracker("block-zm"), --tracker block-zm

is the live tracker's search under another cost (s2d_block_track_zm_u8, restated in tests/zm_tracker_ref.py): both patches lose
their rounded mean before the absolute differences are summed, so a brightness offset of a whole frame (auto-exposure, a cloud, a
fade) cancels exactly as long as no pixel saturates, and `tau` and `refresh` bound the mean absolute zero-mean difference.  Under
such a cost a flat template costs about 0 against every flat patch, so a point whose query-frame patch deviates from its own mean
by less than `texture` grey levels on average is refused: with `texture` > 0 such points are not tracked and their columns are
left out of pred_tracks and pred_visibility (0 keeps every point).  The defaults are design choices, not tuned on real video:
refresh -1 because the fixed template is anchored to the query frame and cannot drift, and the zero-mean cost is what lets it
survive a lighting change; texture 4 because it is a third of `tau`, so a template must deviate from its mean by a margin before
a `tau`-sized mismatch means anything.  Keymask discovery reads the visibility in stage 1 only; stage 2 ignores it, so what this
tracker changes there is the positions, and which points exist at all.  Limits that stay: whole-pixel positions; a change of gain
(contrast) is not removed, only an offset; scale and rotation; repeated texture; quality against CoTracker is unmeasured."""
import numpy as np
import torch

from .._lib import lib


def grid_points(grid_size, H, W):
    """host int32 [grid_size^2, 2] of (x, y): ys = ((2i+1) H) // (2g), xs = ((2i+1) W) // (2g), row-major (y outer) -- the
    cell centres of a g x g partition of the frame, the grid of the tests' stub tracker.  CoTracker's own grid cannot be pinned
    here: the package is on none of the project's machines."""
    g = int(grid_size)
    i = np.arange(g, dtype=np.int64) * 2 + 1
    ys, xs = (i * H) // (2 * g), (i * W) // (2 * g)
    gy, gx = np.meshgrid(ys, xs, indexing="ij")
    return np.stack([gx.reshape(-1), gy.reshape(-1)], -1).astype(np.int32)


class BlockTracker:
    """callable with the tracker contract of tracker.py"""

    def __init__(self, radius=5, search=16, tau=12):
        self.radius, self.search, self.tau = int(radius), int(search), int(tau)
        self._video = self._version = self._grey = None

    def cuda(self):
        return self

    def grey(self, video):
        """u8 [T,H,W] of video [1,T,3,H,W]; kept while the calls pass the same tensor object, unmodified (the reference held
        here keeps the object alive, so its identity cannot be reused by another tensor)"""
        if self._video is not video or self._version != video._version:
            if video.dim() != 5 or video.shape[0] != 1 or video.shape[2] != 3 or video.dtype != torch.float32 or not video.is_cuda:
                raise ValueError("video must be a float32 [1,T,3,H,W] tensor on the device")
            v = video.contiguous()
            _, T, _, H, W = v.shape
            grey = torch.empty((T, H, W), device=v.device, dtype=torch.uint8)
            lib().call("s2d_video_grey_u8", v, T, H, W, grey, torch.cuda.current_stream().cuda_stream)
            self._video, self._version, self._grey = video, video._version, grey
        return self._grey

    def __call__(self, video, grid_size=50, grid_query_frame=0, segm_mask=None, backward_tracking=False):
        T, H, W = video.shape[1], video.shape[-2], video.shape[-1]
        pts = grid_points(grid_size, H, W)
        if segm_mask is not None:
            if tuple(segm_mask.shape[-2:]) != (H, W):
                raise ValueError(f"segm_mask is {tuple(segm_mask.shape[-2:])}, the video {(H, W)}")
            m = segm_mask.detach().cpu().numpy().reshape(H, W)
            pts = np.ascontiguousarray(pts[m[pts[:, 1], pts[:, 0]] != 0])
        N = len(pts)
        dev = video.device
        tracks = torch.empty((1, T, N, 2), device=dev, dtype=torch.float32)
        vis = torch.empty((1, T, N), device=dev, dtype=torch.uint8)
        if N > 0:
            tracks, vis = self._track(self.grey(video), T, H, W, torch.from_numpy(pts).to(dev), N, int(grid_query_frame),
                                      int(bool(backward_tracking)), tracks, vis)
        return tracks, vis.bool()

    def _track(self, grey, T, H, W, pts, N, q, backward, tracks, vis):
        """fills tracks [1,T,N,2] and vis [1,T,N] (u8) and returns them, or the columns of them that the tracker keeps"""
        lib().call("s2d_block_track_u8", grey, T, H, W, pts, N, q, backward, self.radius, self.search, self.tau, tracks, vis,
                   torch.cuda.current_stream().cuda_stream)
        return tracks, vis


class LiveBlockTracker(BlockTracker):
    """BlockTracker (its grid, mask selection and grey-frame cache) with the wide search and the live template of
    s2d_block_track_live_u8"""

    def __init__(self, radius=5, search=32, tau=12, refresh=4):
        super().__init__(radius, search, tau)
        self.refresh = int(refresh)

    def _track(self, grey, T, H, W, pts, N, q, backward, tracks, vis):
        lib().call("s2d_block_track_live_u8", grey, T, H, W, pts, N, q, backward, self.radius, self.search, self.tau, self.refresh,
                   tracks, vis, torch.cuda.current_stream().cuda_stream)
        return tracks, vis


class ZeroMeanBlockTracker(BlockTracker):
    """BlockTracker (its grid, mask selection and grey-frame cache) with the zero-mean cost and the texture gate of
    s2d_block_track_zm_u8"""

    def __init__(self, radius=5, search=32, tau=12, refresh=-1, texture=4):
        super().__init__(radius, search, tau)
        self.refresh, self.texture = int(refresh), int(texture)

    def _track(self, grey, T, H, W, pts, N, q, backward, tracks, vis):
        trackable = torch.empty((N,), device=tracks.device, dtype=torch.uint8)
        lib().call("s2d_block_track_zm_u8", grey, T, H, W, pts, N, q, backward, self.radius, self.search, self.tau, self.refresh,
                   self.texture, tracks, vis, trackable, torch.cuda.current_stream().cuda_stream)
        if self.texture <= 0:
            return tracks, vis
        keep = trackable.bool()                             # the select reads the number of kept points back
        return tracks[:, :, keep], vis[:, :, keep]
