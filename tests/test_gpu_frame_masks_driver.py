"""The stage-1 driver (`python -m s2d_amd.keymask.frame_masks`) end to end: every PNG against paint_owner of the masks the same model
returns for that clip, the report line, the skip / overwrite rule, discovery's own reader on the tree, and the hand-off of painted
masks of a constructed scene into `discover --tracker block`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import frame_masks_refs as F
from tests.test_gpu_eval_drivers import KD_CFG, MIN_TEST, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
VIDEOS = {"va": 3, "vb": 4}
H, W, MAX_MASKS = 48, 64, 12


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from s2d_amd.checkpoint import kd_to_plain
    _, model = _model(0)
    path = str(tmp_path_factory.mktemp("ckpt") / "model.pth")
    torch.save({"model": kd_to_plain({k: v.detach().cpu() for k, v in model.state_dict().items()}), "iteration": 1}, path)
    return path


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    from PIL import Image
    root = str(tmp_path_factory.mktemp("frames"))
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    for v, (name, T) in enumerate(VIDEOS.items()):
        os.makedirs(os.path.join(root, name))
        for t in range(T):
            img = np.stack([(xx * 4 + t * 13) % 256, (yy * 5 + v * 40) % 256, ((xx + yy) * 3) % 256], -1)
            img = np.clip(img + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, name, f"{t:05d}.jpg"), quality=90)
    return root


def _argv(frames, masks, checkpoint, per_call, extra=()):
    return ["--config-file", KD_CFG, "--weights", checkpoint, "--video-base-path", frames, "--mask-base-path", masks,
            "--confidence-threshold", "0", "--max-masks", str(MAX_MASKS), "--frames-per-call", str(per_call), "--threads", "4",
            *extra, "INPUT.MIN_SIZE_TEST", MIN_TEST]


def _main(argv, capsys):
    from s2d_amd.keymask import frame_masks
    capsys.readouterr()
    line = frame_masks.main(argv)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    return line


def _expected(frames, checkpoint, per_call):
    """{(video, mask file): rgb [H,W,3]} and the number of non-empty planes, from the same model with inference_device_masks and the
    driver's selection (threshold 0: every prediction; the first MAX_MASKS)"""
    from s2d_amd.config import load_config
    from s2d_amd.data.test_loader import YTVISTestLoader
    from s2d_amd.evaluate import build_model
    from s2d_amd.frame_paint import mask_colors
    from s2d_amd.keymask.frame_masks import folder_document
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TEST", MIN_TEST])
    model = build_model(cfg, checkpoint, torch.device(DEV))
    model.inference_rle, model.inference_device_masks = False, True
    doc, clips, _ = folder_document(frames, "/nonexistent", per_call, overwrite=True)
    want, nmasks = {}, 0
    with torch.no_grad():
        for inputs in YTVISTestLoader.from_config(cfg, doc, frames, device=DEV, threads=2, prefetch=1, shard=False):
            out = model([inputs])
            planes = out["pred_masks"][:MAX_MASKS].cpu().numpy()
            assert planes.shape[0] >= 2 and planes.shape[1:] == (len(inputs["image"]), H, W)
            rgb, _ = F.paint_owner(planes, mask_colors(MAX_MASKS))
            nmasks += int((F.plane_areas(planes) > 0).sum())
            mdir, names = clips[inputs["video_id"]]
            for t, n in enumerate(names):
                want[(os.path.basename(mdir), n)] = rgb[t]
    return want, nmasks


def _check_tree(masks, want):
    from PIL import Image
    assert len(want) == sum(VIDEOS.values())
    for (video, name), rgb in want.items():
        with Image.open(os.path.join(masks, video, name)) as im:
            assert im.mode == "RGB" and im.size == (W, H)
            np.testing.assert_array_equal(np.asarray(im), rgb, err_msg=f"{video}/{name}")
    for video, T in VIDEOS.items():
        assert sorted(os.listdir(os.path.join(masks, video))) == [f"{t:05d}.png" for t in range(T)]


def test_cli_one_frame_per_call(frames, checkpoint, tmp_path):
    """the command line itself, in a process of its own: the reference's per-image behaviour"""
    masks = str(tmp_path / "masks")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "s2d_amd.keymask.frame_masks", *_argv(frames, masks, checkpoint, 1)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    want, nmasks = _expected(frames, checkpoint, 1)
    _check_tree(masks, want)
    assert (line["videos"], line["skipped"], line["frames"], line["masks"]) == (2, 0, 7, nmasks)
    assert set(line) >= {"videos", "skipped", "frames", "masks", "empty_frames", "wall_s", "frames_per_s", "loader_wait_fraction"}
    assert line["empty_frames"] == sum(1 for rgb in want.values() if not rgb.any())


def test_three_frames_per_call_skip_overwrite_and_discovery_reader(frames, checkpoint, tmp_path, capsys):
    from PIL import Image
    from s2d_amd.keymask.discover import load_idmap
    masks = str(tmp_path / "masks")
    line = _main(_argv(frames, masks, checkpoint, 3), capsys)
    want, nmasks = _expected(frames, checkpoint, 3)
    _check_tree(masks, want)
    assert (line["videos"], line["skipped"], line["frames"], line["masks"]) == (2, 0, 7, nmasks)
    # a second run skips both videos and touches nothing; --overwrite rewrites them
    probe = os.path.join(masks, "va", "00001.png")
    Image.fromarray(np.full((H, W, 3), 7, np.uint8)).save(probe)
    line = _main(_argv(frames, masks, checkpoint, 3), capsys)
    assert (line["videos"], line["skipped"], line["frames"], line["masks"]) == (2, 2, 0, 0)
    assert int(np.asarray(Image.open(probe)).min()) == 7
    line = _main(_argv(frames, masks, checkpoint, 3, ["--overwrite"]), capsys)
    assert (line["videos"], line["skipped"], line["frames"], line["masks"]) == (2, 0, 7, nmasks)
    _check_tree(masks, want)
    # discovery's reader on the tree: per frame as many ids as the PNG has distinct non-black colours
    for video, T in VIDEOS.items():
        idmap = load_idmap(os.path.join(masks, video))
        assert idmap.T == T and (idmap.Hi, idmap.Wi) == (H, W)
        for t in range(T):
            px = np.asarray(Image.open(os.path.join(masks, video, f"{t:05d}.png"))).reshape(-1, 3)
            colours = {tuple(c) for c in np.unique(px, axis=0).tolist()} - {(0, 0, 0)}
            assert len(idmap.frame_object_ids(t)) == len(colours)


def test_switches_are_restored(frames, checkpoint, tmp_path):
    from s2d_amd.keymask.frame_masks import write_masks
    cfg, model = _model(0)
    model.train()
    model.inference_rle, model.inference_index = True, {"rule": "rank"}
    line = write_masks(cfg, model, frames, str(tmp_path / "m"), 0.0, MAX_MASKS, 2, videos_per_job=1, threads=2)
    assert (line["videos"], line["frames"]) == (1, 3)
    assert model.training and model.inference_rle is True and model.inference_index == {"rule": "rank"}
    assert model.inference_paint is None and model.inference_device_masks is False
    model.window_inference, model.window_size, model.window_overlap = True, 2, 1
    with pytest.raises(ValueError, match="inference_paint"):
        write_masks(cfg, model, frames, str(tmp_path / "m2"), 0.0, MAX_MASKS, 3, videos_per_job=1, threads=2)
    assert model.training and model.inference_paint is None


def test_painted_masks_hand_off_to_discovery(tmp_path):
    """constructed logits (three boxes that drift one pixel per frame over textured frames) -> paint_frames -> the driver's writer ->
    discover --tracker block: no failed video, one annotation JSON per video"""
    from s2d_amd import ops
    from s2d_amd.keymask.discover import parse_args, run
    from s2d_amd.keymask.frame_masks import write_frame_png
    from PIL import Image
    from tests.golden import keymask_stub_tracker as S
    work = str(tmp_path)
    for v, (name, sc) in enumerate(F.HANDOFF_SCENES.items()):
        fd, md = os.path.join(work, S.FRAMES_DIR, name), os.path.join(work, S.MASKS_DIR, name)
        os.makedirs(fd)
        os.makedirs(md)
        ml, dims, size, query = F.handoff_logits(sc)
        colors = torch.from_numpy(ops.mask_colors(len(query))).to(DEV)
        rgb, index, areas, _ = ops.paint_frames(torch.from_numpy(ml).to(DEV), dims, size, size, size, torch.from_numpy(query).to(DEV), colors)
        assert areas.cpu().numpy().tolist() == [[o["box"][2] * o["box"][3]] * sc["T"] for o in sc["objects"]]
        rgb = rgb.cpu().numpy()
        for t, frame in enumerate(F.handoff_frames(sc, 20 + v)):
            Image.fromarray(frame).save(os.path.join(fd, f"{t:05d}.png"))
            write_frame_png(os.path.join(md, f"{t:05d}.png"), rgb[t])
    cwd = os.getcwd()
    os.chdir(work)                  # relative paths: the stages derive a split from substrings such as "test" of the video path
    try:
        report = run(parse_args(["--video-base-path", S.FRAMES_DIR, "--mask-base-path", S.MASKS_DIR, "--save-path", "seg_masks",
                                 "--visibility-maps-output-base", "vis_maps", "--visibility-clusters-output-base", "vis_clusters",
                                 "--annotation-output-path", "annotations", "--tracker", "block"]))
    finally:
        os.chdir(cwd)
    print(json.dumps(report))
    assert (report["videos"], report["failed"], report["done"]) == (2, 0, 2)
    for name in F.HANDOFF_SCENES:
        doc = json.load(open(os.path.join(work, "annotations", name + ".json")))
        assert len(doc["annotations"]) >= 1
