"""Merge per-video YTVIS JSONs into one dataset JSON: the positional CLI of keymask_ident/merge_ytvis_jsons.py over
formats.merge_ytvis_jsons.

    python -m s2d_amd.keymask.merge SRC_DIR OUT ONE2X_THRESHOLD

A positive ONE2X_THRESHOLD drops the annotations whose one2x exceeds it."""
import argparse
import glob
import json
import os

from .formats import merge_ytvis_jsons


def main(argv=None):
    p = argparse.ArgumentParser(description="Merge single-video YTVIS JSONs into one dataset JSON.")
    p.add_argument("src_dir", help="Folder containing per-video JSON files")
    p.add_argument("output", help="Destination merged JSON file")
    p.add_argument("one2x_threshold", type=float, default=-1.0, help="Threshold for one2x score")
    args = p.parse_args(argv)
    merged = merge_ytvis_jsons(args.src_dir, args.output, args.one2x_threshold)
    docs = [json.load(open(f)) for f in glob.glob(os.path.join(os.path.abspath(args.src_dir), "*.json"))]
    n_in = sum(len(d.get("annotations", [])) for d in docs if d.get("videos"))
    print(f"Merged {len(merged['videos'])} videos -> {args.output}")
    print(f"   annotations: {len(merged['annotations'])}")
    print(f"   one2x noisy annotations removed: {n_in - len(merged['annotations'])}")
    return merged


if __name__ == "__main__":
    main()
