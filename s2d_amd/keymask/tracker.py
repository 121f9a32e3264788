"""The point-tracker boundary of keymask discovery.

A tracker is a callable with the call the reference makes (cotracker_occlusions.py:355, cotracker_matching.py:1071):

    pred_tracks, pred_visibility = tracker(video, grid_size=g, grid_query_frame=f, segm_mask=m, backward_tracking=b)

video float [1,T,3,H,W] (RGB, 0..255) on the device, segm_mask uint8 [1,1,H,W] with values {0,255} on the host;
pred_tracks [1,T,N,2] (x, y) pixels and pred_visibility [1,T,N] bool.

`load_tracker("cotracker", checkpoint)` builds CoTracker's offline predictor as the reference does (:318-328).  CoTracker is
third party and optional: it is imported only there.  `load_tracker("block")` returns the built-in block-matching baseline
(block_tracker.BlockTracker: no package, no weights; its limits are stated there) and `load_tracker("block-live")` the same
search with a wider reach and a live template (block_tracker.LiveBlockTracker), and `load_tracker("block-zm")` that search under
a zero-mean cost with a texture gate (block_tracker.ZeroMeanBlockTracker), which a change of brightness does not disturb.
`options` (a dict, `--tracker-options`) are keyword arguments of these built-in trackers, e.g. {"search": 48, "refresh": -1}; a key the tracker does not have, or
options for any other tracker, raise ValueError.  `load_tracker("pkg.module:attr")` imports a factory and calls it (with
`checkpoint=` when one is given); that is how tests and other trackers plug in."""
import importlib
import inspect


def _built_in(cls, spec, options):
    options = dict(options or {})
    known = [p for p in inspect.signature(cls.__init__).parameters if p != "self"]
    unknown = sorted(set(options) - set(known))
    if unknown:
        raise ValueError(f"tracker {spec!r} has no option {', '.join(unknown)} (it has {', '.join(known)})")
    return cls(**options)


def load_tracker(spec, checkpoint=None, options=None):
    if spec == "block":
        from .block_tracker import BlockTracker
        return _built_in(BlockTracker, spec, options)
    if spec == "block-live":
        from .block_tracker import LiveBlockTracker
        return _built_in(LiveBlockTracker, spec, options)
    if spec == "block-zm":
        from .block_tracker import ZeroMeanBlockTracker
        return _built_in(ZeroMeanBlockTracker, spec, options)
    if options:
        raise ValueError(f"tracker {spec!r} takes no options: they are for 'block', 'block-live' and 'block-zm'")
    if spec == "cotracker":
        try:
            from cotracker.predictor import CoTrackerPredictor
        except ImportError as e:
            raise ImportError("--tracker cotracker needs the `cotracker` package (CoTracker, facebookresearch/co-tracker), "
                              "which is not installed; install it or pass --tracker pkg.module:factory") from e
        if checkpoint is None:
            raise ValueError("--tracker cotracker needs --tracker-checkpoint (e.g. scaled_offline.pth)")
        model = CoTrackerPredictor(checkpoint=checkpoint)
        import torch
        return model.cuda() if torch.cuda.is_available() else model
    mod, sep, attr = spec.partition(":")
    if not sep or not mod or not attr:
        raise ValueError(f"tracker spec {spec!r}: expected 'cotracker', 'block', 'block-live', 'block-zm' or 'pkg.module:attr'")
    factory = getattr(importlib.import_module(mod), attr)
    return factory(checkpoint=checkpoint) if checkpoint is not None else factory()
