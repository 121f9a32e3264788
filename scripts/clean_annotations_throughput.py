#!/usr/bin/env python3
"""Throughput of the annotation cleanup (s2d_amd/clean_annotations.py) and of the two kernel families under it: the ragged bit-plane
components / cleanup (csrc/plane_components.hip) and the ragged RLE encoder (csrc/rle_ragged.hip, csrc/rle_encode.h).

Sets: the synthetic sets of the self-training scripts -- the ImageNet-shaped image set of scripts/selftrain_throughput.py (previous
masks and kept predictions), the COCO-val-shaped set of scripts/coco_eval_throughput.py and the YTVIS-shaped previous-round
document of scripts/selftrain_video_throughput.py -- with a seeded speckle and pinhole model on top: every mask is decoded on the
device, on every second mask (a seeded coin per mask) a pixel outside it is set with probability 2^-9 and a pixel inside it cleared
with probability 2^-8 (ANDs of seeded random words), and the result is encoded back to RLE.  Options: min_component_area 16,
fill_holes all, connectivity 8.

Per set, medians of 3, warmed, synchronised:
  * `clean` alone and `encode` alone on the first --kernel-chunks chunks (decoded beforehand), per chunk and per plane;
  * clean_document on the whole set by phase (stage, decode, clean, encode: device-inclusive; assemble; and json for clean_file),
    with the share of planes changed and the peak device memory;
  * two baselines on the first --baseline-planes planes, neither of which is the code under test, each REQUIRED to give the planes
    the ragged call gives before a time is reported: (1) scipy.ndimage.label + binary_fill_holes per plane on the CPU; (2) the
    existing kernels used per plane: the plane expanded to a u8 index map, then ops.filter_components (it has no hole rule, so it
    is compared with the ragged call with the fill off).

    python scripts/clean_annotations_throughput.py [--images 20000] [--coco-images 1000] [--videos 2000] [--limit 1100]
        [--out profiles/clean_annotations/throughput.json]

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

MIN_AREA, CONN = 16, 8
FILL = 2 ** 31 - 1


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _random_words(n, k, gen, dev):
    """int32 [n]: every bit set with probability 2^-k"""
    import torch
    acc = None
    for _ in range(k):
        lo = torch.randint(0, 1 << 16, (n,), generator=gen, device=dev, dtype=torch.int32)
        hi = torch.randint(0, 1 << 16, (n,), generator=gen, device=dev, dtype=torch.int32)
        r = lo | (hi << 16)
        acc = r if acc is None else acc & r
    return acc


def _chunks(units, limit):
    chunk, words = [], 0
    for u in units:
        w = (u[1] * u[2] + 31) // 32
        if chunk and words + w > limit:
            yield chunk
            chunk, words = [], 0
        chunk.append(u)
        words += w
    if chunk:
        yield chunk


def speckle_segs(units, dev, seed):
    """units [(seg, H, W)] -> the RLE dicts of the same masks with speckle and pinholes (module docstring)"""
    import numpy as np
    import torch
    from s2d_amd import clean_annotations as C, rle_ragged
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    rng = np.random.default_rng(seed)
    out = []
    for part in _chunks(units, C.CLEAN_CHUNK_WORDS):
        staged = rle_ragged.stage_rle_ragged([[u[0]] for u in part], [(u[1], u[2]) for u in part])
        bits = rle_ragged.decode_ragged(staged, dev).bits
        coin = rng.random(staged.P) < 0.5                                 # the masks that get noise
        wpp = (staged.plane[:, 1] * staged.plane[:, 2] + 31) // 32
        on = torch.from_numpy(np.repeat(np.where(coin, -1, 0).astype(np.int32), wpp)).to(dev)
        noisy = (bits & ~(on & _random_words(bits.numel(), 8, gen, dev))) | (~bits & on & _random_words(bits.numel(), 9, gen, dev))
        out += rle_ragged.encode_ragged(noisy, staged, np.arange(staged.P))[0]
    return out


def scipy_clean(mask):
    import numpy as np
    from scipy import ndimage
    lab, k = ndimage.label(mask, np.ones((3, 3), bool))
    keep = np.bincount(lab.reshape(-1), minlength=k + 1) >= MIN_AREA
    keep[0] = False
    return ndimage.binary_fill_holes(keep[lab])


def kernels_and_baselines(units, dev, log, kernel_chunks, baseline_planes):
    import numpy as np
    import torch
    from s2d_amd import clean_annotations as C, ops, rle_ragged
    rec = {}
    parts = []
    for part in _chunks(units, C.CLEAN_CHUNK_WORDS):
        parts.append(part)
        if len(parts) >= kernel_chunks:
            break
    decoded = []
    for part in parts:
        staged = rle_ragged.stage_rle_ragged([[u[0]] for u in part], [(u[1], u[2]) for u in part])
        decoded.append((staged, rle_ragged.decode_ragged(staged, dev).bits))
    planes = sum(s.P for s, _ in decoded)

    def timed(fn):
        fn()
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return _median(ts)

    cleaned = []

    def clean_all():
        cleaned.clear()
        for s, bits in decoded:
            cleaned.append(ops.clean_planes(bits, s.plane, MIN_AREA, False, FILL, CONN))

    t_clean = timed(clean_all)
    changed = [np.flatnonzero((r + f).cpu().numpy() > 0) for _, r, f in cleaned]
    t_enc_changed = timed(lambda: [rle_ragged.encode_ragged(o[0], s, c) for (s, _), o, c in zip(decoded, cleaned, changed)])
    t_enc_all = timed(lambda: [rle_ragged.encode_ragged(o[0], s, np.arange(s.P)) for (s, _), o in zip(decoded, cleaned)])
    rec["kernels"] = {"chunks": len(decoded), "planes": planes, "words": int(sum(s.words for s, _ in decoded)),
                      "clean_s": round(t_clean, 4), "clean_us_per_plane": round(1e6 * t_clean / planes, 2),
                      "encode_changed_s": round(t_enc_changed, 4), "planes_changed": int(sum(len(c) for c in changed)),
                      "encode_all_s": round(t_enc_all, 4), "encode_all_us_per_plane": round(1e6 * t_enc_all / planes, 2)}
    log(f"kernels: {rec['kernels']}")

    # the baselines, on the first planes of the first chunk
    staged, bits = decoded[0]
    n = min(baseline_planes, staged.P)
    rows = staged.plane[:n]
    sub_words = int(rows[-1, 0] + (rows[-1, 1] * rows[-1, 2] + 31) // 32)
    sub = bits[:sub_words].contiguous()
    full = ops.clean_planes(sub, rows, MIN_AREA, False, FILL, CONN)[0].cpu().numpy()
    filt = ops.clean_planes(sub, rows, MIN_AREA, False, 0, CONN)[0].cpu().numpy()
    t_ragged_full = timed(lambda: ops.clean_planes(sub, rows, MIN_AREA, False, FILL, CONN))
    t_ragged_filter = timed(lambda: ops.clean_planes(sub, rows, MIN_AREA, False, 0, CONN))
    host = sub.cpu().numpy()

    def unpack(words, r):
        w0, H, W = int(r[0]), int(r[1]), int(r[2])
        flat = np.unpackbits(words[w0:w0 + (H * W + 31) // 32].view(np.uint8), bitorder="little")
        return flat[:H * W].reshape(H, W).astype(bool)

    masks = [unpack(host, r) for r in rows]
    t0 = time.perf_counter()
    got = [scipy_clean(m) for m in masks]
    t_scipy = time.perf_counter() - t0
    equal1 = all(np.array_equal(g, unpack(full, r)) for g, r in zip(got, rows))

    shifts = torch.arange(32, device=dev, dtype=torch.int32)

    def per_plane():
        outs = []
        for r in rows:
            w0, H, W = int(r[0]), int(r[1]), int(r[2])
            px = ((sub[w0:w0 + (H * W + 31) // 32, None] >> shifts) & 1).reshape(-1)[:H * W].to(torch.uint8).view(1, H, W)
            outs.append(ops.filter_components(px, MIN_AREA, False, CONN)[0])
        return outs

    outs = per_plane()
    equal2 = all(np.array_equal(o[0].cpu().numpy().astype(bool), unpack(filt, r)) for o, r in zip(outs, rows))
    t_per_plane = timed(per_plane)
    rec["baselines"] = {"planes": n, "ragged_clean_s": round(t_ragged_full, 5), "ragged_filter_only_s": round(t_ragged_filter, 5),
                        "scipy_s": round(t_scipy, 4), "scipy_equal": bool(equal1),
                        "per_plane_u8_filter_s": round(t_per_plane, 4), "per_plane_equal": bool(equal2)}
    if not (equal1 and equal2):
        raise RuntimeError(f"a baseline disagrees with the ragged call: {rec['baselines']}")
    rec["baselines"]["speedup_vs_scipy"] = round(t_scipy / max(t_ragged_full, 1e-9), 1)
    rec["baselines"]["speedup_vs_per_plane"] = round(t_per_plane / max(t_ragged_filter, 1e-9), 1)
    log(f"baselines: {rec['baselines']}")
    return rec


def document_phases(doc, dev, log):
    import torch
    from s2d_amd import clean_annotations as C
    opts = dict(min_component_area=MIN_AREA, fill_holes=FILL, component_connectivity=CONN)
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.json"), os.path.join(tmp, "out.json")
        with open(src, "w") as fh:
            json.dump(doc, fh)
        runs = []
        for k in range(4):                                                # the first run warms up
            seconds = {}
            torch.cuda.reset_peak_memory_stats(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, stats = C.clean_file(src, dst, device=dev, seconds=seconds, **opts)
            torch.cuda.synchronize()
            seconds["total"] = time.perf_counter() - t0
            if k:
                runs.append(seconds)
    phases = ("json", "stage", "decode", "clean", "encode", "assemble", "total")
    rec = {"seconds": {p: round(_median([r[p] for r in runs]), 4) for p in phases}, "all_runs_total_s": [round(r["total"], 4) for r in runs],
           "stats": stats, "share_of_planes_changed": round(stats["planes_changed"] / max(stats["planes"], 1), 4),
           "peak_device_bytes": max(r["device_bytes"] for r in runs), "chunk_words": C.CLEAN_CHUNK_WORDS}
    log(f"clean_file: {rec}")
    return rec


def measure(a):
    import torch

    def log(msg):
        print(f"[{time.perf_counter() - t_start:7.1f} s] {msg}", file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "options": {"min_component_area": MIN_AREA, "fill_holes": "all", "connectivity": CONN},
           "noise": {"speckle_p": 2 ** -9, "pinhole_p": 2 ** -8, "share_of_masks": 0.5}}

    def run(name, doc, video):
        units, where = [], []
        sizes = {r["id"]: (r["height"], r["width"]) for r in doc["videos" if video else "images"]}
        for k, ann in enumerate(doc["annotations"]):
            H, W = sizes[ann["video_id" if video else "image_id"]]
            for t, s in enumerate(ann["segmentations"] if video else [ann["segmentation"]]):
                if s is not None:
                    units.append((s, H, W))
                    where.append((k, t))
        noisy = speckle_segs(units, dev, 7)
        doc = dict(doc, annotations=[dict(x, segmentations=list(x["segmentations"])) if video else dict(x) for x in doc["annotations"]])
        for (k, t), s in zip(where, noisy):
            if video:
                doc["annotations"][k]["segmentations"][t] = s
            else:
                doc["annotations"][k]["segmentation"] = s
        units = [(s, u[1], u[2]) for s, u in zip(noisy, units)]
        log(f"{name}: {len(units)} masks with speckle")
        rec = {"masks": len(units), "annotations": len(doc["annotations"])}
        rec.update(kernels_and_baselines(units, dev, log, a.kernel_chunks, a.baseline_planes))
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
    ap.add_argument("--kernel-chunks", type=int, default=8)
    ap.add_argument("--baseline-planes", type=int, default=400)
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
