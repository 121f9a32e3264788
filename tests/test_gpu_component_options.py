"""The component cleanup options of the stage-1 driver (`python -m s2d_amd.keymask.frame_masks`) and of the DAVIS driver
(`python -m s2d_amd.evaluate --test-format davis`): what a run with --min-component-area / --keep-largest writes is the reference
filter (tests/index_components_refs.py) applied to what the plain run writes, the reports count the removed pixels, and the default
options leave every output byte as it was.  Checkpoint, frames and DAVIS tree are the fixtures of the two drivers' own tests."""
import json
import os

import numpy as np
import pytest

from tests import index_components_refs as R
from tests.test_gpu_davis_driver import SEQS, _main as _davis_main, checkpoint as davis_checkpoint, tree  # noqa: F401
from tests.test_gpu_frame_masks_driver import MAX_MASKS, VIDEOS, _argv, _main as _stage1_main, checkpoint, frames  # noqa: F401

pytestmark = pytest.mark.gpu

# the issue's options.  The random-weight masks of the tiny fixtures give, at these values, both removed pixels and surviving ones
# (asserted below), so the area did not have to be raised.
MIN_AREA = 6
OPTIONS = ["--min-component-area", str(MIN_AREA), "--keep-largest"]
DEFAULTS = ["--min-component-area", "0", "--component-connectivity", "8"]


def _png_tree(root, names):
    from PIL import Image
    out = {}
    for sub, files in names.items():
        assert sorted(os.listdir(os.path.join(root, sub))) == files
        for f in files:
            with Image.open(os.path.join(root, sub, f)) as im:
                out[(sub, f)] = (im.mode, np.asarray(im).copy())
    return out


def _bytes_tree(root, names):
    return {(sub, f): open(os.path.join(root, sub, f), "rb").read() for sub, files in names.items() for f in files}


def test_stage1_driver(frames, checkpoint, tmp_path, capsys):  # noqa: F811
    from s2d_amd.frame_paint import mask_colors
    names = {v: [f"{t:05d}.png" for t in range(T)] for v, T in VIDEOS.items()}
    plain, cleaned, default = (str(tmp_path / d) for d in ("plain", "cleaned", "default"))
    line0 = _stage1_main(_argv(frames, plain, checkpoint, 3), capsys)
    line1 = _stage1_main(_argv(frames, cleaned, checkpoint, 3, OPTIONS), capsys)
    line2 = _stage1_main(_argv(frames, default, checkpoint, 3, DEFAULTS), capsys)
    assert line0["removed_pixels"] == 0 and line2["removed_pixels"] == 0
    assert _bytes_tree(default, names) == _bytes_tree(plain, names)            # the defaults: every output byte as before
    colors = mask_colors(MAX_MASKS)
    code = lambda rgb: (rgb[..., 0].astype(np.int64) << 16) | (rgb[..., 1].astype(np.int64) << 8) | rgb[..., 2]  # noqa: E731
    table = {int(code(c)): k + 1 for k, c in enumerate(colors)}
    table[0] = 0
    before, after = _png_tree(plain, names), _png_tree(cleaned, names)
    removed = kept = frames_hit = 0
    for key, (mode, rgb) in before.items():
        assert mode == "RGB" and after[key][0] == "RGB"
        index = np.vectorize(table.__getitem__, otypes=[np.uint8])(code(rgb))  # KeyError: a colour outside the table
        out, gone, want = R.ref_filter(index[None], MIN_AREA, True, 8, rgb[None])
        np.testing.assert_array_equal(after[key][1], want[0], err_msg=str(key))
        assert ((out[0] == 0) == (want[0] == 0).all(-1)).all()
        removed += int(gone[0])
        frames_hit += int(gone[0] > 0)
        kept += int((out != 0).sum())
    print(f"stage 1: removed {removed} pixels in {frames_hit} of {len(before)} frames, {kept} kept")
    assert line1["removed_pixels"] == removed
    assert frames_hit >= 1 and kept >= 1                                       # not vacuous
    assert {k: v for k, v in line1.items() if k in ("videos", "skipped", "frames", "masks", "empty_frames")} == \
           {k: v for k, v in line0.items() if k in ("videos", "skipped", "frames", "masks", "empty_frames")}


def _davis_line(capsys):
    return json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])


def test_davis_driver(tree, davis_checkpoint, tmp_path, capsys):  # noqa: F811
    from s2d_amd.davis_eval import evaluate_davis, read_index_png
    names = {s: [f"{t:05d}.png" for t in range(T)] for s, (T, _) in SEQS.items()}
    plain, cleaned, default = tmp_path / "plain", tmp_path / "cleaned", tmp_path / "default"
    capsys.readouterr()
    _davis_main(tree, davis_checkpoint, plain)
    line0 = _davis_line(capsys)
    results = _davis_main(tree, davis_checkpoint, cleaned, extra=OPTIONS)
    line1 = _davis_line(capsys)
    _davis_main(tree, davis_checkpoint, default, extra=DEFAULTS)
    line2 = _davis_line(capsys)
    assert "removed_pixels" not in line0 and "removed_pixels" not in line2
    assert _bytes_tree(str(default / "davis"), names) == _bytes_tree(str(plain / "davis"), names)
    assert json.load(open(default / "metrics.json")) == json.load(open(plain / "metrics.json"))
    removed = kept = frames_hit = 0
    for s, files in names.items():
        assert sorted(os.listdir(cleaned / "davis" / s)) == files
        for f in files:
            index = read_index_png(str(plain / "davis" / s / f))
            out, gone, _ = R.ref_filter(index[None], MIN_AREA, True, 8)
            np.testing.assert_array_equal(read_index_png(str(cleaned / "davis" / s / f)), out[0], err_msg=f"{s}/{f}")
            removed += int(gone[0])
            frames_hit += int(gone[0] > 0)
            kept += int((out != 0).sum())
    print(f"davis: removed {removed} pixels in {frames_hit} frames, {kept} kept")
    assert line1["removed_pixels"] == removed
    assert frames_hit >= 1 and kept >= 1                                       # not vacuous
    # the cleaned maps are the ones that were scored: the table equals the one the written PNGs give from disk
    metrics = json.load(open(cleaned / "metrics.json"))
    disk = evaluate_davis(tree[1], str(cleaned / "davis"), sequences=tree[2])
    assert metrics["davis"] == dict(disk["global"]) and results == metrics


def test_options_are_refused_with_the_ytvis_format(tree, davis_checkpoint, tmp_path, monkeypatch):  # noqa: F811
    from s2d_amd import evaluate
    from tests.test_gpu_eval_drivers import KD_CFG
    gt = tmp_path / "ytvis.json"
    gt.write_text(json.dumps({"videos": [], "annotations": [], "categories": [{"id": 1, "name": "object"}]}))
    monkeypatch.setattr(evaluate, "build_model", lambda *a, **k: pytest.fail("the model was built"))
    base = ["--config-file", KD_CFG, "--gt", str(gt), "--image-root", tree[0], "--output-dir", str(tmp_path / "out"), "--weights",
            davis_checkpoint, "--test-format", "ytvis"]
    for extra, name in ((["--min-component-area", "6"], "--min-component-area"), (["--keep-largest"], "--keep-largest"),
                        (["--component-connectivity", "4"], "--component-connectivity"), (OPTIONS, "--min-component-area, --keep-largest")):
        with pytest.raises(ValueError, match=name + ".*--test-format ytvis"):
            evaluate.main(base + extra)
    assert not (tmp_path / "out").exists()
