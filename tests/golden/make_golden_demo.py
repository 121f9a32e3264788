#!/usr/bin/env python3
"""Golden of the video demo's mask PNGs: the reference's own `save_masks` and `PALETTE` (model_training/demo_video/demo.py) on
synthetic per-frame masks.  Container-only; re-run with

    python tests/golden/make_golden_demo.py

demo.py imports cv2, detectron2 and the Mask2Former packages at module level, none of which is installed, so the module is
not imported: the two top-level nodes (the PALETTE assignment and the save_masks function) are compiled from the file's AST
where it lies and executed in a namespace holding numpy and PIL.Image.  Nothing is copied.

Cases: overlapping instances, 14 instances (indices past the palette's 13 entries), a mask on every border, odd frame sizes.
Output demo_masks.npz: per case c, c_masks u8 [K,H,W] (the input), c_index u8 [H,W] (the written PNG read back with PIL),
c_palette u8 (getpalette() of the written PNG), c_mode (its mode)."""
import ast
import os
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shim as R  # noqa: E402

DEMO = os.path.join(R.MT, "demo_video", "demo.py")


def reference_save_masks():
    tree = ast.parse(open(DEMO).read(), DEMO)
    keep = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name == "save_masks")
            or (isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "PALETTE" for t in n.targets))]
    assert len(keep) == 2, "PALETTE or save_masks not found in demo.py"
    ns = {"np": np, "Image": Image}
    exec(compile(ast.Module(body=keep, type_ignores=[]), DEMO, "exec"), ns)
    return ns["save_masks"], ns["PALETTE"]


def cases():
    rng = np.random.default_rng(11)
    out = {}
    H, W = 23, 31                                                     # overlaps across several instances
    m = np.zeros((5, H, W), np.uint8)
    m[0, 2:15, 3:20] = 1
    m[1, 8:22, 10:28] = 1
    m[2, 5:12, 5:30] = 1
    m[3] = rng.random((H, W)) < 0.3
    m[4, 10:13, 0:31] = 1
    out["overlap"] = m
    H, W = 17, 29                                                     # 14 instances: indices 13 and 14 past the palette
    m = np.zeros((14, H, W), np.uint8)
    for k in range(14):
        y, x = (k * 5) % (H - 4), (k * 7) % (W - 5)
        m[k, y:y + 6, x:x + 8] = 1
    out["many"] = m
    H, W = 9, 11                                                      # a mask on every border (and one filling the frame)
    m = np.zeros((3, H, W), np.uint8)
    m[0, 0, :] = 1; m[0, -1, :] = 1; m[0, :, 0] = 1; m[0, :, -1] = 1
    m[1] = 1
    m[2, 3:6, 4:8] = 255                                              # non-0 values other than 1
    out["border"] = m
    out["column"] = (rng.random((4, 13, 1)) < 0.5).astype(np.uint8)   # odd sizes down to one pixel wide
    out["row"] = (rng.random((2, 1, 7)) < 0.5).astype(np.uint8)
    return out


def main():
    save_masks, palette = reference_save_masks()
    arrays = {"palette_constant": np.asarray(palette, np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, m in cases().items():
            p = os.path.join(tmp, name + ".png")
            save_masks([mk for mk in m], p)
            with Image.open(p) as im:
                arrays[name + "_mode"] = np.asarray(im.mode)
                arrays[name + "_palette"] = np.asarray(im.getpalette(), np.uint8)
                arrays[name + "_index"] = np.asarray(im).copy()
            arrays[name + "_masks"] = m
    dst = os.path.join(HERE, "demo_masks.npz")
    np.savez_compressed(dst, **arrays)
    print("wrote", dst, sorted(arrays))


if __name__ == "__main__":
    main()
