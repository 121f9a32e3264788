"""The --fill-holes option of the stage-1 driver (`python -m s2d_amd.keymask.frame_masks`) and of the DAVIS driver
(`python -m s2d_amd.evaluate --test-format davis`): what a run with --min-component-area / --keep-largest and --fill-holes all
writes is the reference fill (tests/index_fill_refs.py) of the reference filter (tests/index_components_refs.py) of what the plain
run writes, the reports count the filled pixels, and --fill-holes 0 launches no fill and leaves every output byte as it was.
A constructed three-frame clip through inference_video(paint=...) covers more than one frame per call.
Checkpoint, frames and DAVIS tree are the fixtures of the two drivers' own tests, by way of tests/test_gpu_component_options.py."""
import json
import os

import numpy as np
import pytest

from tests import index_components_refs as C
from tests import index_fill_refs as R
from tests.test_gpu_component_options import MIN_AREA, OPTIONS, _bytes_tree, _davis_line, _png_tree
from tests.test_gpu_davis_driver import SEQS, _main as _davis_main, checkpoint as davis_checkpoint, tree  # noqa: F401
from tests.test_gpu_frame_masks_driver import VIDEOS, _argv, _main as _stage1_main, checkpoint, frames  # noqa: F401

pytestmark = pytest.mark.gpu

# the issue's options: --min-component-area 6 --keep-largest, then --fill-holes all.  The random-weight masks of the DAVIS fixture
# give filled pixels at this area (asserted below).  Those of the stage-1 fixture are sparse (889 of 21,504 pixels painted): at three
# frames per call no area leaves an enclosed hole, at one frame per call (949 painted, 11 instances) the first area that does is 15
# -- areas 6 to 14 fill nothing, 15 removes a 14-pixel speckle of another instance and fills 52 pixels in one frame -- so that test
# runs one frame per call with --min-component-area 15, and --max-masks 50, the count it was probed with.
FILL = ["--fill-holes", "all"]
OFF = ["--fill-holes", "0"]
STAGE1_AREA, STAGE1_MASKS, STAGE1_PER_CALL = 15, 50, 1
STAGE1 = ["--max-masks", str(STAGE1_MASKS)]
STAGE1_OPTIONS = STAGE1 + ["--min-component-area", str(STAGE1_AREA), "--keep-largest"]


def _no_fill(monkeypatch):
    from s2d_amd import ops
    monkeypatch.setattr(ops, "fill_index_holes", lambda *a, **k: pytest.fail("the fill was launched"))


def test_stage1_driver(frames, checkpoint, tmp_path, capsys, monkeypatch):  # noqa: F811
    from s2d_amd.frame_paint import mask_colors
    names = {v: [f"{t:05d}.png" for t in range(T)] for v, T in VIDEOS.items()}
    plain, cleaned, filled_dir, off = (str(tmp_path / d) for d in ("plain", "cleaned", "filled", "off"))
    line0 = _stage1_main(_argv(frames, plain, checkpoint, STAGE1_PER_CALL, STAGE1), capsys)
    line1 = _stage1_main(_argv(frames, cleaned, checkpoint, STAGE1_PER_CALL, STAGE1_OPTIONS), capsys)
    line2 = _stage1_main(_argv(frames, filled_dir, checkpoint, STAGE1_PER_CALL, STAGE1_OPTIONS + FILL), capsys)
    assert line0["filled_pixels"] == 0 and line1["filled_pixels"] == 0
    colors = mask_colors(STAGE1_MASKS)
    code = lambda rgb: (rgb[..., 0].astype(np.int64) << 16) | (rgb[..., 1].astype(np.int64) << 8) | rgb[..., 2]  # noqa: E731
    table = {int(code(c)): k + 1 for k, c in enumerate(colors)}
    table[0] = 0
    before, mid, after = _png_tree(plain, names), _png_tree(cleaned, names), _png_tree(filled_dir, names)
    filled = removed = frames_hit = 0
    for key, (mode, rgb) in before.items():
        assert mode == "RGB" and after[key][0] == "RGB"
        index = np.vectorize(table.__getitem__, otypes=[np.uint8])(code(rgb))  # KeyError: a colour outside the table
        step, gone, step_rgb = C.ref_filter(index[None], STAGE1_AREA, True, 8, rgb[None])
        np.testing.assert_array_equal(mid[key][1], step_rgb[0], err_msg=str(key))
        out, got, want = R.ref_fill_holes(step, "all", 8, step_rgb, colors)
        np.testing.assert_array_equal(after[key][1], want[0], err_msg=str(key))
        hit = out[0] != step[0]
        assert (want[0][hit] == colors[out[0][hit].astype(np.int64) - 1]).all()       # a filled pixel carries its owner's colour
        assert ((out[0] == 0) == (want[0] == 0).all(-1)).all()
        filled += int(got[0])
        removed += int(gone[0])
        frames_hit += int(got[0] > 0)
    with capsys.disabled():
        print(f"stage 1: removed {removed}, filled {filled} pixels in {frames_hit} of {len(before)} frames")
    assert line2["filled_pixels"] == filled and line2["removed_pixels"] == removed == line1["removed_pixels"]
    assert filled >= 1 and frames_hit >= 1                                     # not vacuous
    # --fill-holes 0: no fill is launched, every output byte as before
    _no_fill(monkeypatch)
    line3 = _stage1_main(_argv(frames, off, checkpoint, STAGE1_PER_CALL, STAGE1 + OFF), capsys)
    assert line3["filled_pixels"] == 0 and line3["removed_pixels"] == 0
    assert _bytes_tree(off, names) == _bytes_tree(plain, names)


def test_davis_driver(tree, davis_checkpoint, tmp_path, capsys, monkeypatch):  # noqa: F811
    from s2d_amd.davis_eval import evaluate_davis, read_index_png
    names = {s: [f"{t:05d}.png" for t in range(T)] for s, (T, _) in SEQS.items()}
    plain, cleaned, filled_dir, off = tmp_path / "plain", tmp_path / "cleaned", tmp_path / "filled", tmp_path / "off"
    capsys.readouterr()
    _davis_main(tree, davis_checkpoint, plain)
    line0 = _davis_line(capsys)
    _davis_main(tree, davis_checkpoint, cleaned, extra=OPTIONS)
    line1 = _davis_line(capsys)
    results = _davis_main(tree, davis_checkpoint, filled_dir, extra=OPTIONS + FILL)
    line2 = _davis_line(capsys)
    assert "filled_pixels" not in line0 and "filled_pixels" not in line1 and "removed_pixels" not in line0
    filled = removed = frames_hit = 0
    for s, files in names.items():
        assert sorted(os.listdir(filled_dir / "davis" / s)) == files
        for f in files:
            index = read_index_png(str(plain / "davis" / s / f))
            step, gone, _ = C.ref_filter(index[None], MIN_AREA, True, 8)
            np.testing.assert_array_equal(read_index_png(str(cleaned / "davis" / s / f)), step[0], err_msg=f"{s}/{f}")
            out, got, _ = R.ref_fill_holes(step, "all", 8)
            np.testing.assert_array_equal(read_index_png(str(filled_dir / "davis" / s / f)), out[0], err_msg=f"{s}/{f}")
            filled += int(got[0])
            removed += int(gone[0])
            frames_hit += int(got[0] > 0)
    with capsys.disabled():
        print(f"davis: removed {removed}, filled {filled} pixels in {frames_hit} frames")
    assert line2["filled_pixels"] == filled and line2["removed_pixels"] == removed == line1["removed_pixels"]
    assert filled >= 1 and frames_hit >= 1                                     # not vacuous
    # the filled maps are the ones that were scored: the table equals the one the written PNGs give from disk
    metrics = json.load(open(filled_dir / "metrics.json"))
    disk = evaluate_davis(tree[1], str(filled_dir / "davis"), sequences=tree[2])
    assert metrics["davis"] == dict(disk["global"]) and results == metrics
    # --fill-holes 0: no fill is launched, no new key, every PNG byte and metrics.json as before
    _no_fill(monkeypatch)
    _davis_main(tree, davis_checkpoint, off, extra=OFF)
    line3 = _davis_line(capsys)
    assert set(line3) == set(line0)
    assert _bytes_tree(str(off / "davis"), names) == _bytes_tree(str(plain / "davis"), names)
    assert json.load(open(off / "metrics.json")) == json.load(open(plain / "metrics.json"))


def test_inference_paint_three_frames_per_clip():
    """constructed logits through inference_video(paint=...), three frames as ONE clip: a large box (proposal 1), and of proposal 2 a
    6 x 6 blob, a 2 x 2 speckle inside the box and a 2 x 2 speckle on the box's edge, all moving with the frame.  The cleanup removes
    both speckles; the fill gives the inner one back to the box in map and picture and leaves the one open to the background black"""
    import torch
    from s2d_amd import ops
    from s2d_amd.modeling.postprocess import inference_video
    T, H, W = 3, 40, 56
    pl = np.full((T, H, W, 8), -1.0, np.float32)
    pl[:, 4:36, 4:52, 0] = 1.0
    for t in range(T):
        pl[t, 10:16, 10 + t:16 + t, 1] = 1.0                         # the blob that stays
        pl[t, 24 + t:26 + t, 30:32, 1] = 1.0                         # a speckle inside the box
        pl[t, 34:36, 20 + 3 * t:22 + 3 * t, 1] = 1.0                 # a speckle on the box's lower edge
    cls = np.tile(np.array([[-6.0, 6.0]], np.float32), (8, 1))
    cls[0], cls[1] = (6.0, -6.0), (5.0, -5.0)
    dev = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    args = (dev(cls), dev(pl.reshape(T * H * W, 8)), (T, H, W), (H, W), (H, W), (H, W), 8)
    base = {"max_masks": 50, "score_threshold": 0.35}
    plain = inference_video(*args, paint=dict(base))
    got = inference_video(*args, paint=dict(base, min_component_area=6, fill_holes="all"))
    assert len(plain["pred_scores"]) == 2 and "pred_filled" not in plain and "pred_removed" not in plain
    index0, rgb0 = plain["pred_index"].cpu().numpy(), plain["pred_masks"].cpu().numpy()
    assert (index0[:, 4:36, 4:52] != 0).all() and [int((index0[t] == 2).sum()) for t in range(T)] == [36 + 4 + 4] * T
    colors = ops.mask_colors(50)
    step, removed, step_rgb = C.ref_filter(index0, 6, False, 8, rgb0)
    want, filled, want_rgb = R.ref_fill_holes(step, "all", 8, step_rgb, colors)
    np.testing.assert_array_equal(got["pred_index"].cpu().numpy(), want)
    np.testing.assert_array_equal(got["pred_masks"].cpu().numpy(), want_rgb)
    assert got["pred_removed"].tolist() == removed.tolist() == [8] * T and got["pred_filled"].tolist() == filled.tolist() == [4] * T
    for t in range(T):
        assert (want[t, 24 + t:26 + t, 30:32] == 1).all() and (want_rgb[t, 24 + t:26 + t, 30:32] == colors[0]).all()
        assert (want[t, 34:36, 20 + 3 * t:22 + 3 * t] == 0).all() and (want[t, 10:16, 10 + t:16 + t] == 2).all()


def test_option_is_refused_with_the_ytvis_format(tree, davis_checkpoint, tmp_path, monkeypatch):  # noqa: F811
    from s2d_amd import evaluate
    from tests.test_gpu_eval_drivers import KD_CFG
    gt = tmp_path / "ytvis.json"
    gt.write_text(json.dumps({"videos": [], "annotations": [], "categories": [{"id": 1, "name": "object"}]}))
    monkeypatch.setattr(evaluate, "build_model", lambda *a, **k: pytest.fail("the model was built"))
    base = ["--config-file", KD_CFG, "--gt", str(gt), "--image-root", tree[0], "--output-dir", str(tmp_path / "out"), "--weights",
            davis_checkpoint, "--test-format", "ytvis"]
    for extra in (["--fill-holes", "all"], ["--fill-holes", "4"]):
        with pytest.raises(ValueError, match="--fill-holes.*--test-format ytvis"):
            evaluate.main(base + extra)
    assert not (tmp_path / "out").exists()
