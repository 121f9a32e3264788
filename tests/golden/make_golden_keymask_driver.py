#!/usr/bin/env python3
"""Golden of the keymask discovery driver: the reference's own per-video stage functions, run in the order of
keymask_ident/main_keymask_ident.py over the synthetic scenes of keymask_stub_tracker.py.  Container-only; re-run with

    python tests/golden/make_golden_keymask_driver.py

Stand-ins for the third-party names the stages touch (none is installed here):
  * cv2: imread / cvtColor served by PIL (as g_idmaps in make_golden.py), IMREAD_UNCHANGED keeping the PNG's own channels;
  * pycocotools.mask: encode / area / toBbox served by the oracle's restatement of maskApi.c (as g_formats);
  * cotracker.predictor.CoTrackerPredictor: the stub tracker, one instance recording every call;
  * the hard-coded checkpoint-directory test of both tracker stages: `os.path.exists` of that one path answers True inside
    the two reference modules' namespaces only.

The stages run with relative paths from a temporary working directory, so no path holds a split name ("test", "val", ...)
that would move the stages' output directories.  main_keymask_ident.py itself is not run: temporal_correspondence_match
returns None after a full run, which its `status > 0` cannot compare; this loop treats a return other than -1 as success.

Output: keymask_driver.json (the stub's call list, the text of every JSON / TXT file the stages wrote, the file list of each
tree) and keymask_driver_png.npz (every PNG as an array)."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_shim as R  # noqa: E402
import keymask_stub_tracker as S  # noqa: E402

OUT_DIRS = ("vis_maps", "vis_clusters", "seg_masks", "annotations")


def _cv2():
    cv2 = sys.modules["cv2"]
    cv2.IMREAD_COLOR, cv2.IMREAD_UNCHANGED, cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2BGR = 1, -1, 4, 4

    def imread(p, flag=1):
        try:
            im = Image.open(p)
        except OSError:
            return None
        if flag == -1:
            a = np.array(im)
            return np.ascontiguousarray(a[..., ::-1]) if a.ndim == 3 else a
        return np.ascontiguousarray(np.array(im.convert("RGB"))[..., ::-1])
    cv2.imread = imread
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[..., ::-1])


def _pycocotools():
    from oracle import oracle_np as O
    pm = types.ModuleType("pycocotools.mask")
    pm.encode = lambda arr: [dict(size=[arr.shape[0], arr.shape[1]], counts=O.rle_encode(np.ascontiguousarray(arr[..., f]))[0]["counts"])
                             for f in range(arr.shape[2])]
    pm.area = lambda r: O.rle_area_bbox(O.rle_decode(r))[0]
    pm.toBbox = lambda r: np.asarray(O.rle_area_bbox(O.rle_decode(r))[1], np.float64)
    pk = types.ModuleType("pycocotools")
    pk.mask = pm
    sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pk, pm
    sys.modules.setdefault("imageio", types.ModuleType("imageio"))


def _patch_checkpoint_dir(module):
    osp = types.ModuleType("os.path")
    osp.__dict__.update(os.path.__dict__)
    osp.exists = lambda p: p == "/mnt/data/checkpoints" or os.path.exists(p)
    fake = types.ModuleType("os")
    fake.__dict__.update(os.__dict__)
    fake.path = osp
    module.os = fake


def tree(root):
    """relative file list, {rel: text} of JSON / TXT files, {rel: array} of PNGs under root"""
    files, texts, pngs = [], {}, {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            rel = os.path.relpath(p, root)
            files.append(rel)
            if f.endswith(".png"):
                pngs[rel] = np.array(Image.open(p))
            else:
                texts[rel] = open(p).read()
    return sorted(files), texts, pngs


def run_reference(work):
    """the stages of main_keymask_ident.py:78-139 on the scenes written under `work` -> (stub, counts)"""
    R.install()
    _cv2()
    _pycocotools()
    occ, win, crw, ku, cm, an = (R.ref(m) for m in ("cotracker_occlusions", "identify_visibility_windows", "crw_utils",
                                                     "keymask_utils", "cotracker_matching", "annotations"))
    stub = S.StubTracker()
    for m in (occ, cm):
        m.CoTrackerPredictor = lambda checkpoint=None: stub
        _patch_checkpoint_dir(m)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        S.write_dataset(".")
        base, mbase = S.FRAMES_DIR, S.MASKS_DIR
        dataset_name, split = "DAVIS", "all"                            # main_keymask_ident.py:40-43
        names = sorted(os.listdir(base))
        counts = {"done": 0, "failed": 0}
        for name in names:
            vp, mp = os.path.join(base, name), os.path.join(mbase, name)
            vdata = occ.extract_object_visibility_data(vp, mp, "videos", "vis_maps", False)
            if vdata is None:
                counts["failed"] += 1
                continue
            vis = win.get_visibility_windows_for_video(vdata, dataset_name, split, name, "vis_clusters", 0.3, False)
            imgs, imgs_orig, lbls, meta = crw.load_frames_and_masks(vp, mp, vis, dataset_name)
            cpath = ku.save_segmentation_masks(imgs, imgs_orig, lbls, meta, "seg_masks", False)
            status = cm.temporal_correspondence_match(vp, mp, cpath, "vis_maps", "vis_clusters", 0.5, False)
            if status == -1:
                counts["failed"] += 1
                continue
            an.write_annotation_for_video(vp, cpath, "annotations", vis)
            counts["done"] += 1
    finally:
        os.chdir(cwd)
    return stub, counts


def main():
    assert R.available(), "/root/reference not present: goldens can only be generated in the build container"
    torch.set_num_threads(8)
    with tempfile.TemporaryDirectory() as d:
        stub, counts = run_reference(d)
        out = {"calls": stub.calls, "counts": counts, "files": {}, "texts": {}}
        pngs = {}
        for top in OUT_DIRS:
            files, texts, arrs = tree(os.path.join(d, top))
            out["files"][top] = files
            out["texts"].update({f"{top}/{k}": v for k, v in texts.items()})
            pngs.update({f"{top}/{k}": v for k, v in arrs.items()})
    with open(os.path.join(HERE, "keymask_driver.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "keymask_driver_png.npz"), **pngs)
    print(f"  {counts}, {len(stub.calls)} tracker calls, {len(pngs)} PNGs")
    for n in ("keymask_driver.json", "keymask_driver_png.npz"):
        print(f"  wrote {n} ({os.path.getsize(os.path.join(HERE, n)) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
