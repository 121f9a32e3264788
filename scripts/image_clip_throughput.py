#!/usr/bin/env python3
"""The COCO image-to-clip mapper on one synthetic 480 x 854 JPEG with 10 polygon instances of 40 vertices, T = 8, the shipped
augmentation list of the KD config (MI355X):

  * mapper: ms per clip of data.image_clip.map_image_clip (JPEG decode, upload, replicate + warp, rasterise, mask warp, area
    read-back), host clock around the call, which ends in a stream synchronise; and the device half alone between two events.
  * polygon stage: data.image_clip.polygons_to_bits (table staging, upload, s2d_polygons_to_bits) against the same 10 planes
    drawn on the host with PIL.ImageDraw, bit-packed with numpy and uploaded; both host clock ending in a synchronise, the two
    alternated in one loop; and the kernel alone between device events with its tables already on the device.
    PIL's polygon fill is another rule, so the two sets of planes differ at boundary pixels: the share that differs is recorded.

Every timing: --warmup untimed rounds, then the median (and min) of --iters.  No bar is set: nobody had measured either number.

    python scripts/image_clip_throughput.py --out DIR [--iters 50] [--warmup 10] [--commit REV]

Prints one JSON line and writes DIR/throughput.json (kept as profiles/image_clip/throughput.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KD_CFG = os.path.join(ROOT, "tests", "golden", "kd_config.json")
H, W, T, N_INST, N_VERT = 480, 854, 8, 10, 40


def star(rng, n):
    cx, cy = rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.2 * H, 0.8 * H)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = rng.uniform(30, 160, n)
    return np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).astype(np.float32)


def pil_planes(polys, dev, torch):
    """the host alternative: one ImageDraw fill per instance, packed to the bit-plane layout, one upload"""
    from PIL import Image, ImageDraw
    wpp = (H * W + 31) // 32
    words = np.zeros((len(polys), wpp * 4), np.uint8)
    for p, pl in enumerate(polys):
        im = Image.new("L", (W, H), 0)
        d = ImageDraw.Draw(im)
        for poly in pl:
            d.polygon([tuple(v) for v in np.asarray(poly, np.float32).reshape(-1, 2).tolist()], fill=1)
        packed = np.packbits(np.asarray(im, np.uint8).reshape(-1), bitorder="little")
        words[p, :len(packed)] = packed
    return torch.from_numpy(words.view(np.int32)).to(dev)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--commit", default=None, help="revision the library was built from (recorded)")
    a = ap.parse_args(argv)
    import torch
    from PIL import Image
    from s2d_amd._lib import lib
    from s2d_amd.config import load_config
    from s2d_amd.data import image_clip as ic
    from s2d_amd.data.train_loader import ClipSettings
    if not torch.cuda.is_available():
        raise SystemExit("image_clip_throughput needs a GPU: nothing is measured on the host")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 2) % 256, (yy * 3) % 256, (xx + yy) % 256], -1).astype(np.int32)
    img = np.clip(img + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
    name = os.path.join(tempfile.mkdtemp(prefix="image_clip_"), "480x854.jpg")
    Image.fromarray(img).save(name, quality=90)
    polys = [[star(rng, N_VERT).reshape(-1).tolist()] for _ in range(N_INST)]
    rec = {"file_name": name, "height": H, "width": W, "image_id": 1,
           "annotations": [{"id": i, "category_id": 0, "iscrowd": 0, "segmentation": p} for i, p in enumerate(polys)]}
    st = ClipSettings(load_config(KD_CFG, ["INPUT.SAMPLING_FRAME_NUM", str(T)]))

    def sync():
        torch.cuda.current_stream(dev).synchronize()

    def host_ms(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def event_ms(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    # ---- the mapper
    def clip(k):
        return ic.map_image_clip(rec, None, np.random.RandomState(k), st, device=dev)

    def device_half(k):
        plan = ic.plan_image_clip(rec, None, np.random.RandomState(k), st)
        buf = ic._stage_image(plan, ic._read_image(plan, None, st.fmt))
        return event_ms(lambda: ic._launch_image_clip(plan, buf, dev))

    for k in range(a.warmup):
        clip(k)
        device_half(k)
    mapper = [host_ms(lambda: clip(k)) for k in range(a.iters)]
    half = [device_half(k) for k in range(a.iters)]

    # ---- the polygon stage
    verts, poly_off, plane_off = ic.stage_polygons(polys)
    verts_d, po_d, pl_d = (torch.from_numpy(x).to(dev) for x in (verts, poly_off, plane_off))
    bits = torch.empty((N_INST, (H * W + 31) // 32), device=dev, dtype=torch.int32)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def kernel():
        lib().call("s2d_polygons_to_bits", verts_d, len(verts), po_d, poly_off, N_INST, pl_d, plane_off, N_INST, None, N_INST, H, W,
                   bits, stream)

    for _ in range(a.warmup):
        ic.polygons_to_bits(polys, H, W, device=dev)
        pil_planes(polys, dev, torch)
        kernel()
    sync()
    stage_dev, stage_pil = [], []
    for _ in range(a.iters):                                  # alternated: both see the same machine state
        stage_dev.append(host_ms(lambda: ic.polygons_to_bits(polys, H, W, device=dev)))
        stage_pil.append(host_ms(lambda: pil_planes(polys, dev, torch)))
    kern = [event_ms(kernel) for _ in range(a.iters)]
    ours = ic.polygons_to_bits(polys, H, W, device=dev)
    theirs = pil_planes(polys, dev, torch)
    sync()
    differ = int(sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in (ours ^ theirs).reshape(-1).cpu().numpy().tolist()))
    set_px = int(sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in ours.reshape(-1).cpu().numpy().tolist()))

    out = {"commit": a.commit, "device": torch.cuda.get_device_name(dev), "H": H, "W": W, "T": T, "instances": N_INST,
           "vertices_per_instance": N_VERT, "iters": a.iters, "warmup": a.warmup,
           "mapper_ms_per_clip": stats(mapper), "mapper_device_half_ms": stats(half),
           "polygon_stage_device_ms": stats(stage_dev), "polygon_stage_pil_upload_ms": stats(stage_pil),
           "polygon_kernel_ms": stats(kern),
           "pixels_set": set_px, "pixels_differing_from_pil": differ,
           "note": "host clock around calls that end in a stream synchronise, except *_device_half_ms and polygon_kernel_ms "
                   "(device events); PIL fills by another rule, so boundary pixels differ; no bar is set"}
    with open(os.path.join(a.out, "throughput.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
