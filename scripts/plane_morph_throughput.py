#!/usr/bin/env python3
"""Throughput of the ragged bit-plane morphology (csrc/plane_morph.hip, s2d_amd/plane_morph.py) and of the annotation cleanup with
smoothing on (s2d_amd/clean_annotations.py --open / --close).

Sets: those of scripts/clean_annotations_throughput.py (ImageNet-shaped, COCO-val-shaped, YTVIS-shaped, with its seeded speckle and
pinhole model).  Cases: disk, radius 2 pixels and radius 1% of the image diagonal, opening then closing.

Per set, medians of 3, warmed, synchronised:
  * ragged `open` + `close` (two morph_planes calls) on the first --kernel-chunks chunks (decoded beforehand), per chunk and plane;
  * the baseline on the first --baseline-planes planes: scipy.ndimage binary_erosion / binary_dilation per mask on the CPU with the
    border values of the rule, REQUIRED to give the planes the ragged calls give before a time is reported;
  * clean_file with smoothing on (open 2, close 1%) against smoothing off, by phase (json, stage, decode, smooth, clean, encode,
    assemble), with the peak device memory of either.
Once: ragged `dilate` of 70 planes of 480 x 854 at disk radius 8 against the fixed-size kernel s2d_disk_dilate_bits_u32 on the same
planes, outputs REQUIRED equal.

    python scripts/plane_morph_throughput.py [--images 20000] [--coco-images 1000] [--videos 2000] [--limit 1100]
        [--out profiles/plane_morph/throughput.json]

The measurement runs in a child process under a time limit; prints one JSON line.  Progress goes to stderr."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = (("r2", 2), ("1pct", "1%"))
MIN_AREA, CONN = 16, 8
FILL = 2 ** 31 - 1


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _timed(fn):
    import torch
    fn()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return _median(ts)


def scipy_smooth(mask, r):
    import numpy as np
    from scipy import ndimage
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    B = yy * yy + xx * xx <= r * r
    m = ndimage.binary_dilation(ndimage.binary_erosion(mask, B, border_value=1), B, border_value=0)
    return ndimage.binary_erosion(ndimage.binary_dilation(m, B, border_value=0), B, border_value=1)


def kernels_and_baseline(units, dev, log, kernel_chunks, baseline_planes):
    import numpy as np
    import clean_annotations_throughput as T
    from s2d_amd import clean_annotations as C, ops, rle_ragged
    from s2d_amd.plane_morph import morph_lds_words, smooth_radius
    parts = []
    for part in T._chunks(units, C.CLEAN_CHUNK_WORDS):
        parts.append(part)
        if len(parts) >= kernel_chunks:
            break
    decoded = []
    for part in parts:
        staged = rle_ragged.stage_rle_ragged([[u[0]] for u in part], [(u[1], u[2]) for u in part])
        decoded.append((staged, rle_ragged.decode_ragged(staged, dev).bits))
    planes = sum(s.P for s, _ in decoded)
    rec = {"chunks": len(decoded), "planes": planes, "words": int(sum(s.words for s, _ in decoded))}

    def smooth(bits, table, rad):
        return ops.morph_planes(ops.morph_planes(bits, table, "open", rad)[0], table, "close", rad)[0]

    def unpack(words, r):
        w0, H, W = int(r[0]), int(r[1]), int(r[2])
        flat = np.unpackbits(words[w0:w0 + (H * W + 31) // 32].view(np.uint8), bitorder="little")
        return flat[:H * W].reshape(H, W).astype(bool)

    for name, spec in CASES:
        radii = [np.array([smooth_radius(spec, int(r[1]), int(r[2])) for r in s.plane], np.int32) for s, _ in decoded]
        t = _timed(lambda: [smooth(bits, s.plane, rad) for (s, bits), rad in zip(decoded, radii)])
        k = {"open_close_s": round(t, 4), "us_per_plane": round(1e6 * t / planes, 2), "radius_min": int(min(r.min() for r in radii)),
             "radius_max": int(max(r.max() for r in radii)),
             "lds_bytes_per_workgroup": [4 * morph_lds_words(s.plane, rad) for (s, _), rad in zip(decoded, radii)]}
        staged, bits = decoded[0]
        n = min(baseline_planes, staged.P)
        rows, rad = staged.plane[:n], radii[0][:n]
        sub = bits[:int(rows[-1, 0] + (rows[-1, 1] * rows[-1, 2] + 31) // 32)].contiguous()
        got = smooth(sub, rows, rad).cpu().numpy()
        t_ragged = _timed(lambda: smooth(sub, rows, rad))
        host = sub.cpu().numpy()
        masks = [unpack(host, r) for r in rows]
        t0 = time.perf_counter()
        want = [scipy_smooth(m, int(r)) for m, r in zip(masks, rad)]
        t_scipy = time.perf_counter() - t0
        equal = all(np.array_equal(w, unpack(got, r)) for w, r in zip(want, rows))
        k["baseline"] = {"planes": n, "ragged_s": round(t_ragged, 5), "scipy_s": round(t_scipy, 4), "scipy_equal": bool(equal)}
        if not equal:
            raise RuntimeError(f"scipy disagrees with the ragged calls: {k}")
        k["baseline"]["speedup_vs_scipy"] = round(t_scipy / max(t_ragged, 1e-9), 1)
        rec[name] = k
        log(f"{name}: {k}")
    return rec


def dilate_against_fixed(dev, log):
    """70 planes of 480 x 854 (DAVIS 480p, the boundary maps' size), disk radius 8: the ragged dilate against the fixed-size kernel"""
    import numpy as np
    import torch
    from s2d_amd import davis_eval, ops
    F, H, W, R = 70, 480, 854, 8
    wpp = (H * W + 31) // 32
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    lo = torch.randint(0, 1 << 16, (F, wpp), generator=gen, device=dev, dtype=torch.int32)
    bits = lo
    for _ in range(5):                                                    # every bit set with probability 2^-6, low half-words
        bits = bits & torch.randint(0, 1 << 16, (F, wpp), generator=gen, device=dev, dtype=torch.int32)
    bits[:, -1] &= (1 << (H * W - 32 * (wpp - 1))) - 1 if (H * W) % 32 else -1
    table = np.stack([np.arange(F) * wpp, np.full(F, H), np.full(F, W), np.zeros(F)], 1).astype(np.int64)
    flat = bits.reshape(-1)
    fixed = davis_eval.disk_dilate_planes(bits, H, W, R)
    ragged = ops.morph_planes(flat, table, "dilate", R)[0]
    equal = bool(torch.equal(fixed.reshape(-1), ragged))
    rec = {"planes": F, "H": H, "W": W, "radius": R, "equal": equal}
    if not equal:
        raise RuntimeError("the ragged dilate disagrees with s2d_disk_dilate_bits_u32")
    t_fixed = [_timed(lambda: davis_eval.disk_dilate_planes(bits, H, W, R)) for _ in range(3)]
    t_ragged = [_timed(lambda: ops.morph_planes(flat, table, "dilate", R)) for _ in range(3)]
    table_dev = torch.from_numpy(table).to(dev)
    t_ragged_dev_table = [_timed(lambda: ops.morph_planes(flat, table_dev, "dilate", R)) for _ in range(3)]
    rec.update(fixed_us=[round(1e6 * t, 1) for t in t_fixed], ragged_call_us=[round(1e6 * t, 1) for t in t_ragged],
               ragged_call_device_table_us=[round(1e6 * t, 1) for t in t_ragged_dev_table])
    # the launches alone: the library call with the tables already on the device
    from s2d_amd import plane_morph
    from s2d_amd._lib import lib
    tiles = torch.from_numpy(plane_morph.morph_tiles(table, np.full(F, R))).to(dev)
    rad = torch.full((F,), R, dtype=torch.int32, device=dev)
    lds = plane_morph.morph_lds_words(table, np.full(F, R))
    out, cnt = torch.empty_like(flat), torch.zeros((2, F), dtype=torch.int32, device=dev)
    ws = torch.empty((lib().call("s2d_plane_morph_workspace_bytes", flat.numel(), F),), dtype=torch.uint8, device=dev)
    t_lib = [_timed(lambda: lib().call("s2d_plane_morph_ragged", flat, table_dev, F, flat.numel(), 1, 0, rad, tiles, len(tiles), lds, out, cnt[0],
                                       cnt[1], ws, ops._stream())) for _ in range(3)]
    rec.update(ragged_library_call_us=[round(1e6 * t, 1) for t in t_lib], ragged_tiles=len(tiles), ragged_lds_bytes=4 * lds, equal_library_call=bool(torch.equal(out, ragged)))
    log(f"dilate: {rec}")
    return rec


def document_phases(doc, dev, log):
    import torch
    from s2d_amd import clean_annotations as C
    base = dict(min_component_area=MIN_AREA, fill_holes=FILL, component_connectivity=CONN)
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.json"), os.path.join(tmp, "out.json")
        with open(src, "w") as fh:
            json.dump(doc, fh)
        for name, opts in (("smoothing_off", base), ("smoothing_on", dict(base, open_radius=2, close_radius="1%"))):
            runs = []
            for k in range(4):                                            # the first run warms up
                seconds = {}
                torch.cuda.reset_peak_memory_stats(dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, stats = C.clean_file(src, dst, device=dev, seconds=seconds, **opts)
                torch.cuda.synchronize()
                seconds["total"] = time.perf_counter() - t0
                if k:
                    runs.append(seconds)
            phases = ("json", "stage", "decode", "smooth", "clean", "encode", "assemble", "total")
            rec[name] = {"seconds": {p: round(_median([r.get(p, 0.0) for r in runs]), 4) for p in phases},
                         "all_runs_total_s": [round(r["total"], 4) for r in runs], "stats": stats,
                         "peak_device_bytes": max(r["device_bytes"] for r in runs)}
    rec["extra_peak_device_bytes"] = rec["smoothing_on"]["peak_device_bytes"] - rec["smoothing_off"]["peak_device_bytes"]
    log(f"clean_file: {rec}")
    return rec


def measure(a):
    import torch
    import clean_annotations_throughput as T

    def log(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "shape": "disk", "cases": dict(CASES),
           "sets": {"images": a.images, "coco_images": a.coco_images, "videos": a.videos}}
    res["dilate_vs_fixed"] = dilate_against_fixed(dev, log)

    def run(name, doc, video):
        units, where = [], []
        sizes = {r["id"]: (r["height"], r["width"]) for r in doc["videos" if video else "images"]}
        for k, ann in enumerate(doc["annotations"]):
            H, W = sizes[ann["video_id" if video else "image_id"]]
            for t, s in enumerate(ann["segmentations"] if video else [ann["segmentation"]]):
                if s is not None:
                    units.append((s, H, W))
                    where.append((k, t))
        noisy = T.speckle_segs(units, dev, 7)
        doc = dict(doc, annotations=[dict(x, segmentations=list(x["segmentations"])) if video else dict(x) for x in doc["annotations"]])
        for (k, t), s in zip(where, noisy):
            if video:
                doc["annotations"][k]["segmentations"][t] = s
            else:
                doc["annotations"][k]["segmentation"] = s
        units = [(s, u[1], u[2]) for s, u in zip(noisy, units)]
        log(f"{name}: {len(units)} masks with speckle")
        rec = {"masks": len(units), "annotations": len(doc["annotations"])}
        rec["kernels"] = kernels_and_baseline(units, dev, log, a.kernel_chunks, a.baseline_planes)
        rec["clean_file"] = document_phases(doc, dev, log)
        res[name] = rec

    if a.images:
        import selftrain_throughput as S
        doc, preds = S.make_set(a.images)
        doc = dict(doc, annotations=doc["annotations"] + [dict(p, id=10 ** 7 + i, iscrowd=0) for i, p in enumerate(preds) if p["score"] >= 0.7])
        run("imagenet_shaped", doc, False)
    if a.coco_images:
        import coco_eval_throughput as K
        cdoc, cres = K.make_set(a.coco_images, dev, log)
        cdoc = dict(cdoc, annotations=cdoc["annotations"] + [dict(p, id=10 ** 7 + i, iscrowd=0) for i, p in enumerate(cres)])
        run("coco_val_shaped", cdoc, False)
    if a.videos:
        import selftrain_video_throughput as V
        vdoc, _ = V.make_set("ytvis", a.videos)
        run("ytvis_shaped", vdoc, True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20000, help="images of the ImageNet-shaped set; 0 leaves it out")
    ap.add_argument("--coco-images", type=int, default=1000, help="images of the COCO-val-shaped set; 0 leaves it out")
    ap.add_argument("--videos", type=int, default=2000, help="videos of the YTVIS-shaped set; 0 leaves it out")
    ap.add_argument("--kernel-chunks", type=int, default=4)
    ap.add_argument("--baseline-planes", type=int, default=60)
    ap.add_argument("--limit", type=int, default=1100, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)), flush=True)
        return 0
    t0 = time.perf_counter()
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--images", str(a.images), "--coco-images", str(a.coco_images), "--videos",
           str(a.videos), "--kernel-chunks", str(a.kernel_chunks), "--baseline-planes", str(a.baseline_planes)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print(f"the measurement exceeded {a.limit} s", file=sys.stderr)
        return 1
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        print(f"the measurement failed with status {r.returncode}", file=sys.stderr)
        return 1
    res = json.loads(lines[-1])
    res["script_s"] = round(time.perf_counter() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
