"""GPU checks of the video demo: the area / draw-order and render kernels against the numpy raster rule (demo.render_host) bit for
bit, the meta-arch's device-mask output form, and `python -m s2d_amd.demo` end to end on a seeded checkpoint."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from s2d_amd import demo, ops
from tests.test_gpu_eval_drivers import KD_CFG, MIN_TEST, _model, checkpoint  # noqa: F401  (checkpoint is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _masks(rng, K, T, H, W, ties=True):
    """rectangles (some on every border, some with equal areas) and speckle"""
    m = np.zeros((K, T, H, W), np.uint8)
    for k in range(K):
        for t in range(T):
            kind = (k + t) % 5
            if kind == 0:                                                  # the frame's border ring
                m[k, t, 0, :] = m[k, t, -1, :] = m[k, t, :, 0] = m[k, t, :, -1] = 1
            elif kind == 1:
                m[k, t] = rng.random((H, W)) < 0.2
            else:
                h, w = max(1, H // (2 + kind)), max(1, W // (1 + kind))
                y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
                m[k, t, y:y + h, x:x + w] = 1 if ties else kind
    return m


def _device_render(frames, masks, colors, want_index=True):
    fd = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(DEV)
    md = torch.from_numpy(masks).to(DEV)
    _, order = ops.mask_frame_areas(md)
    ov, ix = ops.render_instances(fd, md, order, torch.from_numpy(colors).to(DEV), demo.ALPHA, want_index=want_index)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), (ix.cpu().numpy() if ix is not None else None)


@pytest.mark.parametrize("K", [0, 1, 13, 100])
@pytest.mark.parametrize("W", [1, 37, 1280])
def test_render_matches_numpy_rule(K, W):
    rng = np.random.default_rng(K * 7 + W)
    T, H = (3, 19) if W < 1280 else (2, 9)
    fr = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    m = _masks(rng, K, T, H, W)
    col = demo.instance_colors(K)
    got_ov, got_ix = _device_render(fr, m, col)
    want_ov, want_ix = demo.render_host(fr, m, col)
    assert np.array_equal(got_ov, want_ov)
    assert np.array_equal(got_ix, want_ix)
    if K == 0:
        assert np.array_equal(got_ov, fr) and not got_ix.any()


def test_render_tied_areas_border_masks_and_values_other_than_one():
    rng = np.random.default_rng(3)
    T, H, W = 2, 16, 20
    fr = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    m = np.zeros((6, T, H, W), np.uint8)
    for k in range(5):                                                      # five 4 x 4 squares, all of one area, overlapping
        m[k, :, 2 + k:6 + k, 3 + 2 * k:7 + 2 * k] = 1 + 100 * (k % 2)
    m[5, :, :, :] = 0
    m[5, :, 0, :] = m[5, :, -1, :] = m[5, :, :, 0] = m[5, :, :, -1] = 7
    col = demo.instance_colors(6)
    got_ov, got_ix = _device_render(fr, m, col)
    want_ov, want_ix = demo.render_host(fr, m, col)
    assert np.array_equal(got_ov, want_ov) and np.array_equal(got_ix, want_ix)
    ov_only, none = _device_render(fr, m, col, want_index=False)
    assert none is None and np.array_equal(ov_only, want_ov)


def test_render_frames_view_at_an_odd_byte_offset():
    rng = np.random.default_rng(8)
    T, H, W, K = 2, 13, 40, 5                                               # W % 4 == 0: only the offset forces the byte path
    flat = rng.integers(0, 256, (T * H * W * 3 + 3,), dtype=np.uint8)
    fd = torch.from_numpy(flat).to(DEV)[3:].view(T, H, W, 3)
    m = _masks(rng, K, T, H, W)
    col = demo.instance_colors(K)
    got_ov, got_ix = _device_render(fd, m, col)
    want_ov, want_ix = demo.render_host(flat[3:].reshape(T, H, W, 3), m, col)
    assert np.array_equal(got_ov, want_ov) and np.array_equal(got_ix, want_ix)


def test_render_36_frames_720p():
    rng = np.random.default_rng(36)
    T, H, W, K = 36, 720, 1280, 10
    fr = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    m = np.zeros((K, T, H, W), np.uint8)
    for k in range(K):
        for t in range(T):
            y, x = (37 * k + 11 * t) % (H - 200), (97 * k + 23 * t) % (W - 300)
            m[k, t, y:y + 100 + 9 * k, x:x + 150 + 13 * k] = 1
    m[3, :, :, 0] = 1                                                       # left border
    m[4, :, -1, :] = 1                                                      # bottom border
    col = demo.instance_colors(K)
    got_ov, got_ix = _device_render(fr, m, col)
    for t in (0, 17, 35):
        want_ov, want_ix = demo.render_host(fr[t:t + 1], m[:, t:t + 1], col)
        assert np.array_equal(got_ov[t], want_ov[0]), t
        assert np.array_equal(got_ix[t], want_ix[0]), t


def test_more_than_255_instances_raise():
    m = torch.zeros((256, 1, 4, 4), dtype=torch.uint8, device=DEV)
    fr = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.mask_frame_areas(m)
    with pytest.raises(ValueError):
        ops.render_instances(fr, m, torch.zeros((1, 256), dtype=torch.int32, device=DEV),
                             torch.zeros((256, 3), dtype=torch.uint8, device=DEV))
    from s2d_amd._lib import lib
    out = torch.empty_like(fr)
    with pytest.raises(RuntimeError):                                       # the C ABI refuses it too (S2D_ERR_ARG)
        lib().call("s2d_render_instances_u8", fr, 1, 4, 4, m, 256, torch.zeros((1, 256), dtype=torch.int32, device=DEV),
                   torch.zeros((256, 3), dtype=torch.uint8, device=DEV), 128, out, None, ops._stream())
    with pytest.raises(RuntimeError):
        lib().call("s2d_mask_frame_areas_i32", m, 256, 1, 4, 4, torch.empty((256, 1), dtype=torch.int32, device=DEV), None,
                   ops._stream())


@pytest.mark.parametrize("shape", [(3, 4, 16, 16), (17, 5, 7, 9), (2, 3, 720, 1280), (1, 1, 1, 1)])
def test_areas_and_draw_order(shape):
    rng = np.random.default_rng(sum(shape))
    m = (rng.random(shape) < 0.3).astype(np.uint8) * rng.integers(1, 256, shape, dtype=np.uint8)
    m[: shape[0] // 2] = (rng.random((shape[0] // 2,) + shape[1:]) < 0.5)   # some planes 0 / 1
    if shape[0] > 2:
        m[1] = m[0]                                                         # exact ties
    areas, order = ops.mask_frame_areas(torch.from_numpy(m).to(DEV))
    want = (m != 0).sum((2, 3))
    assert np.array_equal(areas.cpu().numpy(), want)
    want_order = np.stack([np.argsort(-want[:, t], kind="stable") for t in range(shape[1])])
    assert np.array_equal(order.cpu().numpy(), want_order)
    a2, none = ops.mask_frame_areas(torch.from_numpy(m).to(DEV), want_order=False)
    assert none is None and torch.equal(a2, areas)


# ----------------------------------------------------------------------------------------------------- device-mask form
def _clip_inputs(T=3, H=70, W=97, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    fr = []
    for t in range(T):
        img = np.stack([(xx * 3 + t * 11) % 256, (yy * 2) % 256, ((xx + yy) * 5) % 256], -1).astype(np.int32)
        fr.append(np.clip(img + rng.integers(-25, 25, img.shape), 0, 255).astype(np.uint8))
    return np.stack(fr)


@pytest.mark.parametrize("use_nms", [False, True])
def test_device_mask_form_equals_cpu_bool_form(use_nms):
    cfg, model = _model(3)
    model.eval()
    model.use_nms = use_nms
    frames = torch.from_numpy(_clip_inputs()).to(DEV)
    inp = demo.model_inputs(cfg, frames)
    base = model([inp])
    assert "pred_masks_format" not in base                                  # the default form is unchanged
    assert all(m.dtype == torch.bool and not m.is_cuda for m in base["pred_masks"])
    model.inference_device_masks = True
    dev = model([inp])
    assert dev["pred_masks_format"] == "device_u8"
    pm = dev["pred_masks"]
    assert pm.is_cuda and pm.dtype == torch.uint8 and tuple(pm.shape) == (len(base["pred_masks"]), 3, 70, 97)
    assert dev["pred_scores"] == base["pred_scores"] and dev["pred_labels"] == base["pred_labels"]
    assert torch.equal(pm.cpu().bool(), torch.stack(base["pred_masks"]))
    assert int(pm.max()) <= 1
    model.inference_device_masks = False
    assert model([inp])["pred_scores"] == base["pred_scores"]


# -------------------------------------------------------------------------------------------------------------- end to end
def _write_clip(d, frames, ext, orient=None):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    for t, f in enumerate(frames):
        im = Image.fromarray(f)
        p = os.path.join(d, f"{t:05d}.{ext}")
        if orient is not None:
            ex = Image.Exif()
            ex[274] = orient
            im.save(p, quality=95, exif=ex)
        else:
            im.save(p)


def _run_demo(inputs, out, weights, thr, extra=()):
    cmd = [sys.executable, "-m", "s2d_amd.demo", "--config-file", KD_CFG, "--weights", weights, "--input"] + list(inputs) + [
        "--output", str(out), "--confidence-threshold", repr(thr)] + list(extra) + ["--opts", "INPUT.MIN_SIZE_TEST", MIN_TEST]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.fixture(scope="module")
def png_clip(tmp_path_factory):
    root = tmp_path_factory.mktemp("demo")
    frames = _clip_inputs(T=5, H=70, W=97, seed=4)
    _write_clip(str(root / "clipA"), frames, "png")
    return root, frames


@pytest.fixture(scope="module")
def in_process(png_clip, checkpoint):  # noqa: F811
    """the driver's predictions from an in-process model([inputs]) call, CPU bool masks (the default form)"""
    from s2d_amd.config import load_config
    from s2d_amd.evaluate import build_model
    root, _ = png_clip
    cfg = load_config(KD_CFG, ["INPUT.MIN_SIZE_TEST", MIN_TEST])
    model = build_model(cfg, checkpoint, torch.device(DEV))
    model.inference_rle = False
    _, files = demo.expand_inputs([str(root / "clipA" / "*.png")])
    host = demo.decode_frames(files)
    with torch.no_grad():
        pred = model([demo.model_inputs(cfg, host.to(DEV))])
    return files, host.numpy().copy(), pred


def test_driver_writes_fixture_exact_masks_and_oracle_overlays(png_clip, checkpoint, in_process, tmp_path):  # noqa: F811
    from PIL import Image
    root, _ = png_clip
    files, frames, pred = in_process
    scores = pred["pred_scores"]
    assert len(scores) >= 2
    thr = float(np.float32((scores[0] + scores[-1]) / 2))
    n = demo.kept_count(scores, thr)
    line = _run_demo([str(root / "clipA" / "*.png")], tmp_path, checkpoint, thr, ["--save-frames", "True", "--save-masks", "True"])
    assert line["frames"] == 5 and line["height"] == 70 and line["width"] == 97 and line["instances"] == n
    assert line["video"] == "clipA" and all(line[k] >= 0 for k in ("decode_s", "model_s", "render_s", "write_s", "wall_s"))
    kept = [m.numpy() for m in pred["pred_masks"][:n]]
    want_ov, _ = demo.render_host(frames, np.stack(kept) if n else np.zeros((0, 5, 70, 97), np.uint8), demo.instance_colors(n))
    vdir = tmp_path / "clipA"
    assert sorted(os.listdir(vdir)) == sorted([os.path.basename(f) for f in files] + ["mask_" + os.path.basename(f) for f in files])
    for t, f in enumerate(files):
        with Image.open(demo.mask_path(str(vdir), f)) as im:
            assert im.mode == "P" and im.getpalette() == demo.PALETTE
            assert np.array_equal(np.asarray(im), demo.index_map([m[t] for m in kept], (70, 97)))
        with Image.open(demo.frame_path(str(vdir), f)) as im:
            assert np.array_equal(np.asarray(im), want_ov[t]), t


def test_driver_threshold_above_every_score_writes_unchanged_frames(png_clip, checkpoint, tmp_path):  # noqa: F811
    from PIL import Image
    root, frames = png_clip
    line = _run_demo([str(root / "clipA" / "*.png")], tmp_path, checkpoint, 2.0, ["--save-frames", "False", "--save-masks", "False"])
    assert line["instances"] == 0
    for t in range(5):
        with Image.open(tmp_path / "clipA" / f"{t:05d}.png") as im:
            assert np.array_equal(np.asarray(im), frames[t])
        with Image.open(tmp_path / "clipA" / f"mask_{t:05d}.png") as im:
            assert im.mode == "P" and not np.asarray(im).any() and np.asarray(im).shape == (70, 97)


def test_driver_exif_rotated_jpegs_and_flag_gating(checkpoint, tmp_path):  # noqa: F811
    frames = _clip_inputs(T=3, H=48, W=80, seed=9)
    _write_clip(str(tmp_path / "in" / "clipJ"), frames, "jpg", orient=6)   # ROTATE_270 on decode: 80 x 48 portrait frames
    files = [str(tmp_path / "in" / "clipJ" / f"{t:05d}.jpg") for t in (2, 0, 1)]
    line = _run_demo(files, tmp_path / "out", checkpoint, 2.0, ["--save-frames", "1", "--save-masks", "1"])
    assert (line["height"], line["width"], line["frames"]) == (80, 48, 3)
    from PIL import Image
    vdir = tmp_path / "out" / "clipJ"
    assert sorted(os.listdir(vdir)) == ["00000.jpg", "00001.jpg", "00002.jpg", "mask_00000.png", "mask_00001.png", "mask_00002.png"]
    for t in range(3):
        with Image.open(vdir / f"{t:05d}.jpg") as im:
            assert im.size == (48, 80)
        with Image.open(vdir / f"mask_{t:05d}.png") as im:
            assert im.size == (48, 80) and not np.asarray(im).any()
    _run_demo(files, tmp_path / "masks_only", checkpoint, 0.0, ["--save-masks", "True"])
    assert os.listdir(tmp_path / "masks_only") == []                        # --save-masks alone writes nothing
