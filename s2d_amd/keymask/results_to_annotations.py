"""Pseudo annotations from a results.json, the step between two self-distillation rounds: the reference's
keymask_ident/convert_results_to_annotations.py:10-111 with its observable behaviour kept:

* a prediction with score < threshold is skipped, and so is one whose video is not in the GT file;
* `id` is the prediction's index in the results list + 1, so skipped predictions still use up ids;
* a prediction whose frame count differs from the video's `length` is an error;
* `categories` come from the merged annotation file; `info`, `licenses` and `videos` from the GT file;
* per frame, `bboxes` are [x, y, w, h] float lists (mask_util.toBbox) and `areas` ints (mask_util.area), None for a null frame.

The RLE strings are decoded on the device (ytvis_eval.decode_frames) and the boxes and areas come from the bit planes
(s2d_mask_plane_bbox_u32, s2d_mask_plane_areas_u32).

    python -m s2d_amd.keymask.results_to_annotations --annotation-file merged.json --gt-annotation-file gt.json \\
        --results-file results.json --score-threshold 0.75 --output-dir D --output-filename NAME \\
        [--min-component-area N] [--keep-largest] [--fill-holes N|all] [--component-connectivity 4|8]

The four cleanup options (s2d_amd/clean_annotations.py) are this project's own and off by default.
"""
import argparse
import json
import os


def device_bboxes_areas(segs, H, W):
    """frames of one prediction (RLE dicts or None) -> (bboxes [[x, y, w, h] floats or None], areas [int or None])"""
    from ..ytvis_eval import decode_frames, plane_areas, plane_bboxes
    bits = decode_frames(segs, H, W)
    bb = plane_bboxes(bits, H, W).cpu().tolist()
    ar = plane_areas(bits).cpu().tolist()
    return ([[float(v) for v in bb[f]] if s is not None else None for f, s in enumerate(segs)],
            [int(ar[f]) if s is not None else None for f, s in enumerate(segs)])


def convert(merged, gt, results, score_threshold=0.75, bbox_area_fn=device_bboxes_areas):
    """loaded documents -> (the new annotation document, number of predictions skipped for their score)"""
    videos = {v["id"]: v for v in gt["videos"]}
    out = {"info": gt["info"], "licenses": gt["licenses"], "videos": gt["videos"], "categories": merged["categories"],
           "annotations": []}
    low = 0
    for i, pred in enumerate(results):
        vid = pred["video_id"]
        if pred["score"] < score_threshold:
            low += 1
            continue
        if vid not in videos:
            continue
        v = videos[vid]
        n = v["length"]
        segs = pred["segmentations"]
        if n != len(segs):
            raise ValueError(f"Number of frames in video {vid} ({n}) does not match the number of segmentations ({len(segs)})")
        bboxes, areas = bbox_area_fn(segs, v["height"], v["width"])
        out["annotations"].append({"video_id": vid, "iscrowd": 0, "height": v["height"], "width": v["width"], "length": n,
                                   "segmentations": segs, "bboxes": bboxes, "areas": areas,
                                   "category_id": pred["category_id"], "id": i + 1})
    return out, low


def convert_files(annotation_file, gt_annotation_file, results_file, score_threshold, output_dir, filename,
                  bbox_area_fn=device_bboxes_areas, cleanup=None):
    """cleanup: a clean_annotations.cleanup_options dict; when it asks for anything the masks of the new document are cleaned just
    before it is written (this project's own; the reference cleans nothing)"""
    with open(annotation_file) as fh:
        merged = json.load(fh)
    with open(results_file) as fh:
        results = json.load(fh)
    with open(gt_annotation_file) as fh:
        gt = json.load(fh)
    doc, low = convert(merged, gt, results, score_threshold, bbox_area_fn)
    if cleanup:
        from ..clean_annotations import clean_merged
        doc = clean_merged(doc, cleanup)
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f"{filename}.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=2)
    if results:
        print(f"Skipped {low}/{len(results)} ({round(low / len(results) * 100, 2)}%) low scoring predictions.")
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description="Convert a results.json file to a YTVIS-style annotation file.")
    ap.add_argument("--annotation-file", required=True, help="merged annotation JSON (categories)")
    ap.add_argument("--gt-annotation-file", required=True, help="GT annotation JSON (info, licenses, videos)")
    ap.add_argument("--results-file", required=True)
    ap.add_argument("--score-threshold", type=float, default=0.75)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--output-filename", required=True)
    from ..clean_annotations import add_cleanup_arguments, cleanup_options
    a = add_cleanup_arguments(ap).parse_args(argv)
    print(convert_files(a.annotation_file, a.gt_annotation_file, a.results_file, a.score_threshold, a.output_dir,
                        a.output_filename, cleanup=cleanup_options(a)))


if __name__ == "__main__":
    main()
