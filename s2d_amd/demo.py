"""Video demo: `demo_video/demo.py` + `predictor.py` (the frame-list path) without detectron2, cv2 or matplotlib.

    python -m s2d_amd.demo --config-file X.yaml --weights ckpt.pth --input "<dir>/*.jpg" --output OUT \
        --save-frames True --save-masks True [--confidence-threshold 0.5] [--opts KEY VALUE ...]

The flags are the reference's.  `--weights` overrides MODEL.WEIGHTS.  One `--input` argument is a glob (sorted matches, an
assertion when nothing matches); several are taken in the order given.  The video's name is `input[0].split("/")[-2]` of the raw
first argument.  `--save-frames` / `--save-masks` take a string and any non-empty one turns the flag on: `--save-frames False`
turns it ON, as in the reference.

The frames are decoded as detectron2's read_image does (data/test_loader.read_frame), put on the device once as RGB u8
[T,H,W,3], resized by the PIL-exact kernel (INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST, channel order INPUT.FORMAT) and run as one
clip through `model([inputs])` with the masks kept on the device (`inference_device_masks`).  The predictions with
score >= --confidence-threshold are kept (a prefix: scores come sorted).  With `--output`, `--save-frames` writes every frame's
overlay to OUT/<video>/<frame basename> and, with `--save-masks` too, its palette index map to
join(OUT/<video>, "mask_" + basename).replace(".jpg", ".png").  Overlay and index map are made on the device in one pass
(ops.render_instances; the raster rule is `render_host`), copied back through a pinned staging buffer and written by a pool of
at most 16 threads while the next frames are copied.  Ends with one JSON line on stdout; progress goes to stderr.

Deviations from the reference (INTEGRATION.md "Video demo"): no kept instance writes all-zero index maps and unchanged frames
(the reference's save_masks raises IndexError); more than 255 kept instances raise ValueError before rendering; `--video-input`
exits with an error (no video decoder on the target machines); the model runs the library's fp32-class path, not autocast; the
overlay is this module's exact raster rule, not detectron2's antialiased matplotlib rendering, and carries no text labels."""
import argparse
import colorsys
import glob
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MAX_THREADS = 16
ALPHA = 128                      # detectron2 overlay_instances alpha = 0.5, as an integer weight out of 256
# The DAVIS annotation palette the reference's save_masks writes into every mask PNG (13 entries; tests/golden/demo_masks.npz)
PALETTE = [0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0, 0, 0, 128, 128, 0, 128, 0, 128, 128, 128, 128, 128, 64, 0, 0, 191, 0, 0,
           64, 128, 0, 191, 128, 0, 64, 0, 128]


def _log(msg):
    print(msg, file=sys.stderr, flush=True)


def get_parser():
    """demo.py get_parser(): the same flags, defaults and types"""
    ap = argparse.ArgumentParser(description="S2D video demo: instance overlays and palette mask PNGs of a frame list")
    ap.add_argument("--config-file", default="configs/youtubevis_2019/video_maskformer2_R50_bs16_8ep.yaml", metavar="FILE",
                    help="path to config file")
    ap.add_argument("--weights", required=True, help="path to weights file (overrides MODEL.WEIGHTS)")
    ap.add_argument("--video-input", help="Path to video file (not supported: no video decoder; pass the frames with --input)")
    ap.add_argument("--input", nargs="+", help="A list of space separated input images; or a single glob pattern such as "
                    "'directory/*.jpg'; this will be treated as frames of a video")
    ap.add_argument("--output", help="A directory to save output visualizations")
    ap.add_argument("--save-frames", default=False, help="Save frame level image outputs (any non-empty string turns it on)")
    ap.add_argument("--save-masks", default=False, help="Save frame level image masks (any non-empty string turns it on)")
    ap.add_argument("--confidence-threshold", type=float, default=0.5, help="Minimum score for instance predictions to be shown")
    ap.add_argument("--opts", help="Modify config options using the command-line 'KEY VALUE' pairs", default=[],
                    nargs=argparse.REMAINDER)
    return ap


def flag_on(value):
    """the reference tests `if args.save_frames:` on the raw string: every non-empty value is on, "False" included"""
    return bool(value)


def expand_inputs(inputs):
    """--input -> (video_name, frame paths): the name is input[0].split("/")[-2] of the raw first argument; one argument is a
    glob (sorted, an assertion when empty), several are kept in the order given"""
    video_name = inputs[0].split("/")[-2]
    if len(inputs) == 1:
        files = sorted(glob.glob(os.path.expanduser(inputs[0])))
        assert files, "The input path(s) was not found"
    else:
        files = list(inputs)
    return video_name, files


def frame_path(video_dir, path):
    return os.path.join(video_dir, os.path.basename(path))


def mask_path(video_dir, path):
    """the reference's expression: the ".jpg" -> ".png" replacement runs over the whole joined path"""
    return os.path.join(video_dir, "mask_" + os.path.basename(path)).replace(".jpg", ".png")


def instance_colors(n):
    """u8 RGB [n, 3]: instance k's overlay colour, the same in every frame.  Hues step by the golden ratio from 0, saturation
    and value cycle through 4 levels each (period 4 x 4), so the first 64 entries are distinct."""
    out = np.zeros((n, 3), np.uint8)
    sat = (0.85, 0.55, 1.0, 0.7)
    val = (1.0, 0.8, 0.9, 0.7)
    for k in range(n):
        h = (k * 0.6180339887498949) % 1.0
        r, g, b = colorsys.hsv_to_rgb(h, sat[k % 4], val[(k // 4) % 4])
        out[k] = [int(round(r * 255)), int(round(g * 255)), int(round(b * 255))]
    return out


def index_map(frame_masks, shape=None):
    """save_masks' loop on the masks of one frame (list of [H,W]): pixel = i + 1 of the last mask holding it, else 0.  With no
    masks, an all-zero map of `shape` (the reference raises IndexError)."""
    if len(frame_masks) > 255:
        raise ValueError(f"at most 255 instances fit a u8 index map, got {len(frame_masks)}")
    out = np.zeros(frame_masks[0].shape if len(frame_masks) else shape, np.uint8)
    for i, m in enumerate(frame_masks):
        out[np.asarray(m) != 0] = i + 1
    return out


def save_index_png(index, path):
    """a P-mode PNG of the u8 index map with PALETTE (save_masks' file)"""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(index))
    im.putpalette(PALETTE)
    im.save(path)


def render_host(frames, masks, colors, alpha=ALPHA):
    """The demo's raster rule in numpy (the oracle of ops.render_instances).  frames u8 [T,H,W,3], masks [K,T,H,W] (0 / non-0),
    colors u8 [K,3] -> (overlay u8 [T,H,W,3], index u8 [T,H,W]).  Per frame the instances are drawn in descending order of their
    area in that frame, ties in instance order; instance k blends its mask pixels to (c*a + p*(256-a) + 128) >> 8 and then paints
    the mask pixels with a 4-neighbour outside the frame or outside the mask opaque c.  index = 1 + the last instance holding the
    pixel."""
    frames = np.asarray(frames)
    masks = np.asarray(masks) != 0
    K, T = masks.shape[0], frames.shape[0]
    if K > 255:
        raise ValueError(f"at most 255 instances, got {K}")
    out = frames.astype(np.int32)
    index = np.zeros(frames.shape[:3], np.uint8)
    cols = np.asarray(colors, np.int32)
    for t in range(T):
        m = masks[:, t]
        areas = m.reshape(K, -1).sum(1) if K else np.zeros(0, np.int64)
        img = out[t]
        for k in np.argsort(-areas, kind="stable"):
            mk = m[k]
            if not areas[k]:
                continue
            pad = np.pad(mk, 1)
            inner = mk & pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]
            img[mk] = (cols[k] * alpha + img[mk] * (256 - alpha) + 128) >> 8
            img[mk & ~inner] = cols[k]
        for k in range(K):
            index[t][m[k]] = k + 1
    return out.astype(np.uint8), index


def decode_frames(files, threads=MAX_THREADS):
    """read_frame (EXIF-rotated RGB) of every file in a pool of at most 16 threads -> pinned u8 [T,H,W,3]; frames of different
    sizes raise ValueError"""
    import torch
    from .data.test_loader import read_frame
    buf = None
    with ThreadPoolExecutor(max(1, min(int(threads), MAX_THREADS, len(files)))) as pool:
        futs = [pool.submit(read_frame, f, "RGB") for f in files]
        for t, fu in enumerate(futs):
            a = fu.result()
            if buf is None:
                buf = torch.empty((len(files),) + a.shape, dtype=torch.uint8, pin_memory=True)
            elif a.shape != tuple(buf.shape[1:]):
                raise ValueError(f"frame {files[t]} is {a.shape[:2]}, frame {files[0]} is {tuple(buf.shape[1:3])}")
            buf[t].numpy()[...] = a
    return buf


def model_inputs(cfg, frames):
    """device RGB u8 [T,H,W,3] -> the predictor's input dict: frames resized with ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST)
    by the PIL-exact kernel, channels in INPUT.FORMAT, height / width of the original frames"""
    from .data.augment import shortest_edge_shape
    from .data.resize import resize_frames
    T, H, W, _ = frames.shape
    fmt = cfg.INPUT.FORMAT
    if fmt == "BGR":
        src = frames.flip(-1).contiguous()
    elif fmt == "RGB":
        src = frames
    else:
        raise NotImplementedError(f"INPUT.FORMAT {fmt}")
    mn, mx = int(cfg.INPUT.MIN_SIZE_TEST), int(cfg.INPUT.MAX_SIZE_TEST)
    img = resize_frames(src, (H, W) if mn == 0 else shortest_edge_shape(H, W, mn, mx))
    return {"image": [img[t] for t in range(T)], "height": H, "width": W}


def kept_count(scores, threshold):
    """number of predictions with score >= threshold; they must be a prefix (inference_video sorts scores descending)"""
    n = sum(1 for s in scores if s >= threshold)
    assert all(s >= threshold for s in scores[:n]), "scores are not in descending order: the kept set is not a prefix"
    return n


def write_outputs(overlay, index, files, video_dir, threads=MAX_THREADS, chunk=4):
    """copy overlay u8 [T,H,W,3] (and index u8 [T,H,W] unless None) back in chunks of frames through pinned staging buffers on a
    side stream; a pool of at most 16 threads encodes and writes each chunk as soon as its copy has landed"""
    import torch
    from PIL import Image
    T = overlay.shape[0]
    host_ov = torch.empty(overlay.shape, dtype=torch.uint8, pin_memory=True)
    host_ix = torch.empty(index.shape, dtype=torch.uint8, pin_memory=True) if index is not None else None
    side = torch.cuda.Stream(overlay.device)
    side.wait_stream(torch.cuda.current_stream(overlay.device))
    chunks = []
    with torch.cuda.stream(side):
        for c0 in range(0, T, chunk):
            c1 = min(T, c0 + chunk)
            host_ov[c0:c1].copy_(overlay[c0:c1], non_blocking=True)
            if host_ix is not None:
                host_ix[c0:c1].copy_(index[c0:c1], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
            chunks.append((c0, c1, ev))

    def put_frame(t):
        Image.fromarray(host_ov[t].numpy()).save(frame_path(video_dir, files[t]))

    def put_mask(t):
        save_index_png(host_ix[t].numpy(), mask_path(video_dir, files[t]))

    with ThreadPoolExecutor(max(1, min(int(threads), MAX_THREADS))) as pool:
        futs = []
        for c0, c1, ev in chunks:
            ev.synchronize()
            for t in range(c0, c1):
                futs.append(pool.submit(put_frame, t))
                if host_ix is not None:
                    futs.append(pool.submit(put_mask, t))
        for fu in futs:
            fu.result()


def run(args):
    """the demo on parsed arguments -> the report dict"""
    import torch
    from . import ops
    from .config import load_config
    from .evaluate import build_model

    t_start = time.perf_counter()
    if not args.input:
        if args.video_input:
            raise SystemExit("--video-input is not supported: there is no video decoder on this platform; extract the frames and "
                             "pass them with --input")
        raise SystemExit("nothing to do: pass the frames with --input")
    save_frames, save_masks = flag_on(args.save_frames), flag_on(args.save_masks)
    video_name, files = expand_inputs(args.input)

    cfg = load_config(args.config_file, args.opts or [])
    cfg.MODEL.WEIGHTS = args.weights
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_model(cfg, cfg.MODEL.WEIGHTS, device)
    model.inference_rle = False
    model.inference_device_masks = True

    t0 = time.perf_counter()
    host = decode_frames(files)
    frames = host.to(device, non_blocking=True)
    T, H, W, _ = frames.shape
    t1 = time.perf_counter()
    with torch.no_grad():
        pred = model([model_inputs(cfg, frames)])
    n = kept_count(pred["pred_scores"], args.confidence_threshold)
    masks = pred["pred_masks"][:n] if n else torch.empty((0, T, H, W), dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    _log(f"detected {n} instances per frame in {t2 - t1:.2f}s")

    render_s = write_s = 0.0
    if args.output:
        os.makedirs(args.output, exist_ok=True)
        if save_frames:
            if n > 255:
                raise ValueError(f"{n} instances kept: a u8 mask index map holds at most 255 (raise --confidence-threshold)")
            video_dir = os.path.join(args.output, video_name)
            os.makedirs(video_dir, exist_ok=True)
            colors = torch.from_numpy(instance_colors(n)).to(device)
            _, order = ops.mask_frame_areas(masks)
            overlay, index = ops.render_instances(frames, masks, order, colors, ALPHA, want_index=save_masks)
            torch.cuda.synchronize(device)
            t3 = time.perf_counter()
            render_s = t3 - t2
            write_outputs(overlay, index, files, video_dir)
            write_s = time.perf_counter() - t3
            _log(f"wrote {T} frames{' and masks' if save_masks else ''} to {video_dir}")
    return {"video": video_name, "frames": T, "height": H, "width": W, "instances": n, "decode_s": round(t1 - t0, 4),
            "model_s": round(t2 - t1, 4), "render_s": round(render_s, 4), "write_s": round(write_s, 4),
            "wall_s": round(time.perf_counter() - t_start, 4)}


def main(argv=None):
    args = get_parser().parse_args(argv)
    _log("Arguments: " + str(args))
    line = run(args)
    print(json.dumps(line), flush=True)
    return line


if __name__ == "__main__":
    main(sys.argv[1:])
