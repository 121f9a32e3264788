"""`python -m s2d_amd.evaluate --test-format davis` on a synthetic DAVIS tree: a checkpoint goes through the test loader, the model's
proposal index maps (ops.infer_index) and DAVISEvaluator; the PNGs it writes, scored from disk by evaluate_davis, give the very table
of metrics.json -- both paths divide the same integers.  Model and checkpoint as tests/test_gpu_eval_drivers.py builds them."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_eval_drivers import KD_CFG, MIN_TEST, _model

pytestmark = pytest.mark.gpu
SEQS = {"bear": (4, 2), "camel": (5, 3)}                                   # name -> (frames, objects)
H, W = 48, 64


def _write_tree(root):
    """JPEGImages/480p/<seq>/<frame>.jpg, Annotations_unsupervised/480p/<seq>/<frame>.png (objects as boxes that drift, a block of
    void 255), sequences.txt"""
    from PIL import Image
    from s2d_amd.davis_eval import save_index_png
    rng = np.random.default_rng(3)
    img_root, gt_dir = os.path.join(root, "JPEGImages", "480p"), os.path.join(root, "Annotations_unsupervised", "480p")
    yy, xx = np.mgrid[0:H, 0:W]
    for si, (name, (T, G)) in enumerate(SEQS.items()):
        os.makedirs(os.path.join(img_root, name))
        os.makedirs(os.path.join(gt_dir, name))
        for t in range(T):
            img = np.stack([(xx * 3 + t * 11) % 256, (yy * 5) % 256, ((xx + yy) * (si + 2)) % 256], -1).astype(np.uint8)
            img = np.clip(img.astype(np.int32) + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(img_root, name, f"{t:05d}.jpg"), quality=90)
            gt = np.zeros((H, W), np.uint8)
            for g in range(G):
                gt[6 + 12 * g: 16 + 12 * g, 4 + 14 * g + t: 20 + 14 * g + t] = g + 1
            gt[40:46, 50:60] = 255
            save_index_png(os.path.join(gt_dir, name, f"{t:05d}.png"), gt)
    seqs = os.path.join(root, "sequences.txt")
    with open(seqs, "w") as fh:
        fh.write("camel\nbear\n")                                           # not the sorted order: the list decides
    return img_root, gt_dir, seqs


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _write_tree(str(tmp_path_factory.mktemp("davis")))


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from s2d_amd.checkpoint import kd_to_plain
    _, model = _model(0)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    path = str(tmp_path_factory.mktemp("ckpt") / "model.pth")
    torch.save({"model": kd_to_plain(sd), "iteration": 7}, path)
    return path


def _main(tree, checkpoint, out, fmt="davis", extra=(), opts=()):
    from s2d_amd import evaluate
    img_root, gt_dir, seqs = tree
    args = ["--config-file", KD_CFG, "--gt", gt_dir, "--image-root", img_root, "--output-dir", str(out), "--weights", checkpoint,
            "--threads", "4", "--test-format", fmt, "--sequences", seqs] + list(extra) + \
           ["INPUT.MIN_SIZE_TEST", MIN_TEST, "MODEL.MASK_FORMER.TEST.NUM_PREDICTIONS", "30"] + list(opts)
    return evaluate.main(args)


def _check_outputs(tree, out, capsys, windows_over=None):
    from PIL import Image
    from s2d_amd.davis_eval import DAVIS_PALETTE, GLOBAL_KEYS, evaluate_davis, read_index_png
    _, gt_dir, seqs = tree
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert line["videos"] == 2 and line["frames"] == 9 and line["frames_per_s"] > 0 and 0.0 <= line["loader_wait_fraction"] <= 1.0
    if windows_over is not None:
        assert line["windows"] > windows_over
    for name, (T, _) in SEQS.items():
        for t in range(T):
            path = out / "davis" / name / f"{t:05d}.png"
            assert path.is_file(), path
            with Image.open(path) as im:
                assert im.mode == "P" and im.size == (W, H) and im.getpalette() == DAVIS_PALETTE
            assert int(read_index_png(path).max()) <= 20
    metrics = json.load(open(out / "metrics.json"))
    assert list(metrics) == ["davis"] and set(metrics["davis"]) == set(GLOBAL_KEYS)
    disk = evaluate_davis(gt_dir, str(out / "davis"), sequences=seqs)
    assert metrics["davis"] == dict(disk["global"])                         # ==: the same integers divided on both paths
    rows = list(csv.reader(open(out / "global_results.csv")))
    assert rows[0] == list(GLOBAL_KEYS) and [float(v) for v in rows[1]] == [round(metrics["davis"][k], 3) for k in GLOBAL_KEYS]
    per = list(csv.reader(open(out / "per-sequence_results.csv")))
    assert per[0] == ["Sequence", "J-Mean", "F-Mean"]
    assert [r[0] for r in per[1:]] == ["camel_1", "camel_2", "camel_3", "bear_1", "bear_2"] and all(0 <= float(r[1]) <= 1 for r in per[1:])
    return metrics


@pytest.mark.parametrize("rule", ["rank", "prob"])
def test_driver_scores_a_checkpoint(tree, checkpoint, tmp_path, capsys, rule):
    results = _main(tree, checkpoint, tmp_path, extra=["--index-rule", rule])
    metrics = _check_outputs(tree, tmp_path, capsys)
    assert results == metrics


def test_driver_auto_and_windowed(tree, checkpoint, tmp_path, capsys):
    """auto with a directory takes the DAVIS path; the 5-frame sequence runs in more than one window of 3 and still scores"""
    _main(tree, checkpoint, tmp_path, fmt="auto", opts=["MODEL.MASK_FORMER.TEST.WINDOW_INFERENCE", "True",
                                                        "MODEL.MASK_FORMER.TEST.WINDOW_SIZE", "3",
                                                        "MODEL.MASK_FORMER.TEST.WINDOW_OVERLAP", "1"])
    _check_outputs(tree, tmp_path, capsys, windows_over=2)


def test_driver_refusals(tree, checkpoint, tmp_path):
    from s2d_amd.davis_eval import DAVISEvaluator
    with pytest.raises(ValueError, match="--boundary-ap"):
        _main(tree, checkpoint, tmp_path, extra=["--boundary-ap"])
    with pytest.raises(ValueError, match="--iou-types"):
        _main(tree, checkpoint, tmp_path, extra=["--iou-types", "segm"])
    with pytest.raises(ValueError, match="first-frame"):
        DAVISEvaluator(tree[1], str(tmp_path), task="semi-supervised")
    assert not (tmp_path / "metrics.json").exists()


def test_missing_ground_truth_frame_raises_before_the_model_runs(tree, checkpoint, tmp_path, monkeypatch):
    import shutil
    from s2d_amd import evaluate
    root = tmp_path / "tree"
    shutil.copytree(os.path.dirname(os.path.dirname(tree[0])), root)
    img_root, gt_dir = str(root / "JPEGImages" / "480p"), str(root / "Annotations_unsupervised" / "480p")
    os.remove(os.path.join(gt_dir, "camel", "00003.png"))
    monkeypatch.setattr(evaluate, "build_model", lambda *a, **k: pytest.fail("the model was built"))
    with pytest.raises(FileNotFoundError, match="00003"):
        _main((img_root, gt_dir, str(root / "sequences.txt")), checkpoint, tmp_path / "out")
