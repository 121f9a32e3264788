"""Eval-only driver: `train_net_video.py --eval-only` without detectron2.

    python -m s2d_amd.evaluate --config-file X.yaml --gt ann.json --image-root DIR --output-dir OUT [--weights ckpt.pth] [KEY VALUE ...]

Builds MODEL.META_ARCHITECTURE through the registry from the yaml (config.load_config), loads the weights with the reference's
key conversions (checkpoint.load_checkpoint; every tensor of the evaluated network must load), and runs every video of the
split through `model([inputs])` with the test loader (data/test_loader.py) and YTVISEvaluator.process.  Predictions stay on the
device until they are COCO RLE (the meta-arch's inference_rle switch); labels map to the GT file's category ids in sorted order, as
the registered dataset's metadata maps them.  Writes OUT/results.json (the reference layout),
OUT/metrics.json (the "segm" dict; with --boundary-ap {"segm": ..., "boundary": ...}, Boundary AP beside mask AP from the same
pass over the videos; not for a split without annotations) and prints one JSON timing line: videos/s, frames/s, the
number of windows run (one per video unless MODEL.MASK_FORMER.TEST.WINDOW_INFERENCE cuts long videos) and the fraction of the wall
time the model waited on the loader.  Under torch.distributed.run the videos are split round-robin by
rank and rank 0 writes the files.

--test-format auto|ytvis|coco_image (auto: a --gt document with `images` and no `videos` is a COCO image file,
data/image_clip.detect_train_format): a COCO instances document is scored image by image -- every image a one-frame video through
the same `model([inputs])` (data/coco_image_loader.COCOImageTestLoader, coco_eval.COCOImageEvaluator) -- and the run writes
OUT/coco_instances_results.json and OUT/metrics.json as {"segm": ..., "bbox": ...} (mask AP and box AP of the masks' tight boxes,
12 metrics each); the timing line counts `images`.  --iou-types segm,bbox[,boundary] (image format only; default segm,bbox) chooses
the dicts of metrics.json: `boundary` adds Boundary AP (coco_eval.py), bands --dilation-ratio of the image diagonal wide.
--boundary-ap is a YTVIS option: with the image format it is refused (--iou-types is the image format's switch).

--test-format davis (auto: --gt is a directory): DAVIS-2017 unsupervised J&F of the checkpoint.  --gt is the annotation directory
(Annotations_unsupervised/480p), --image-root is JPEGImages/480p, --sequences a text file of sequence names (default: every
sub-directory of --gt).  Every sequence runs through the same `model([inputs])` with the model's inference_index switch: the
proposals (--max-proposals of at most 254, default 20, scored --score-threshold or better) become one non-overlapping index map
per frame on the device (ops.infer_index; --index-rule rank: a pixel goes to its best-ranked proposal; prob: to the largest
score * sigmoid(logit)), which davis_eval.DAVISEvaluator scores where it is (--bound-th: the F-measure's boundary tolerance) and
writes as OUT/davis/<sequence>/<frame>.png.  OUT/global_results.csv, OUT/per-sequence_results.csv, OUT/metrics.json =
{"davis": {...}}; the timing line counts `videos`.  --boundary-ap and --iou-types are refused.  Parity with the DAVIS toolkit is
unpinned (davis_eval.py).  --min-component-area N (default 0), --keep-largest and --component-connectivity {4,8} (default 8) clean
every map on the device before it is scored and written (ops.filter_components: of a proposal's pixels in a frame, connected
components smaller than N pixels become background, and with --keep-largest every component but its largest); the timing line then
counts `removed_pixels`.  --fill-holes N|all (default 0: off) then fills the holes of the cleaned map (ops.fill_index_holes: a zero
region of at most N pixels that does not touch the frame border and is enclosed by ONE proposal takes its label; the zero pixels are
connected under the complementary connectivity); the timing line then counts `filled_pixels`.  They are DAVIS options: any other
--test-format refuses them by name.  With the defaults no component or fill kernel is launched."""
import argparse
import json
import os
import sys
import time

import torch

from .index_components import fill_holes_argument

TEST_FORMATS = ("auto", "ytvis", "coco_image", "davis")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="YTVIS eval-only run of a checkpoint (mask AP / AR, results.json)")
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--gt", required=True, help="YTVIS annotation JSON of the split")
    ap.add_argument("--image-root", required=True, help="directory the JSON's file_names are relative to")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--weights", default=None, help="torch .pth or detectron2 .pkl (default: MODEL.WEIGHTS)")
    ap.add_argument("--threads", type=int, default=8, help="JPEG decode threads (<= 16)")
    ap.add_argument("--prefetch", type=int, default=2, help="videos decoded ahead (1 or 2)")
    ap.add_argument("--dist-backend", default="gloo", help="process group backend under torch.distributed.run")
    ap.add_argument("--boundary-ap", action="store_true", help="also score Boundary AP (matching on min(mask IoU, boundary IoU))")
    ap.add_argument("--dilation-ratio", type=float, default=0.02, help="boundary band width as a fraction of the image diagonal")
    ap.add_argument("--iou-types", default=None, help="image format only: comma-separated list of segm, bbox, boundary (default segm,bbox)")
    ap.add_argument("--test-format", choices=TEST_FORMATS, default="auto",
                    help="the --gt document: YTVIS videos, COCO images or a DAVIS annotation directory (auto: a directory is davis, "
                         "`images` without `videos` is coco_image)")
    ap.add_argument("--sequences", default=None, help="davis: text file of sequence names (default: every sub-directory of --gt)")
    ap.add_argument("--index-rule", choices=("rank", "prob"), default="rank", help="davis: which proposal takes a contested pixel")
    ap.add_argument("--max-proposals", type=int, default=20, help="davis: proposals per sequence (<= 254)")
    ap.add_argument("--score-threshold", type=float, default=0.0, help="davis: proposals scored below it are dropped")
    ap.add_argument("--bound-th", type=float, default=0.008, help="davis: boundary tolerance of the F-measure")
    ap.add_argument("--min-component-area", type=int, default=0, help="davis: connected components of a proposal smaller than this "
                                                                      "become background (0: off)")
    ap.add_argument("--keep-largest", action="store_true", help="davis: keep only the largest connected component of every proposal "
                                                                "per frame")
    ap.add_argument("--component-connectivity", type=int, choices=(4, 8), default=None, help="davis: pixel connectivity of the "
                                                                                             "components (default 8)")
    ap.add_argument("--fill-holes", type=fill_holes_argument, default=0, metavar="N|all",
                    help="davis: fill holes of at most N pixels that one proposal encloses, after the cleanup (0: off)")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="config overrides KEY VALUE ...")
    return ap.parse_args(argv)


def build_model(cfg, weights, device):
    from .checkpoint import evaluated_prefixes, load_checkpoint
    from .modeling.meta_arch import META_ARCH_REGISTRY
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(device)
    if not weights:
        raise ValueError("no weights: pass --weights or set MODEL.WEIGHTS")
    info = load_checkpoint(model, weights)
    pre = evaluated_prefixes(model)
    missing = [k for k in info["missing"] if k.startswith(pre)]
    if missing:
        raise RuntimeError(f"{len(missing)} tensors of the evaluated network were not loaded from {weights}: {missing[:8]}")
    model.eval()
    model.inference_rle = True
    return model


IOU_TYPES = ("segm", "bbox", "boundary")


def parse_iou_types(text):
    """--iou-types -> tuple of names in the order given (None: the default ("segm", "bbox")); unknown, repeated or no names are
    refused"""
    if text is None:
        return ("segm", "bbox")
    names = tuple(t.strip() for t in (text.split(",") if isinstance(text, str) else text))
    if not names or any(t not in IOU_TYPES for t in names) or len(set(names)) != len(names):
        raise ValueError(f"--iou-types {text!r}: a comma-separated list of distinct names from {', '.join(IOU_TYPES)}")
    return names


def resolve_test_format(fmt, doc, boundary=False, iou_types=None):
    """--test-format -> "ytvis", "coco_image" or "davis" for the loaded --gt document (davis: the annotation directory's path);
    --boundary-ap with the image format is refused, and so is --iou-types (anything but None) with the YTVIS format; the DAVIS
    format refuses both"""
    from .data.image_clip import detect_train_format
    if fmt not in TEST_FORMATS:
        raise ValueError(f"test format {fmt!r}: auto, ytvis, coco_image or davis")
    is_dir = isinstance(doc, (str, os.PathLike)) and os.path.isdir(doc)
    if fmt == "davis" or (fmt == "auto" and is_dir):
        if not is_dir:
            raise ValueError("--test-format davis scores against an annotation directory (Annotations_unsupervised/480p): --gt is not one")
        if boundary:
            raise ValueError("--boundary-ap scores YTVIS videos: it is not available with --test-format davis "
                             "(the F-measure is DAVIS' boundary score; its tolerance: --bound-th)")
        if iou_types is not None:
            raise ValueError("--iou-types chooses the tables of a COCO image split: it is not available with --test-format davis")
        return "davis"
    if is_dir:
        raise ValueError(f"--test-format {fmt} reads an annotation JSON: --gt is a directory (a DAVIS tree: --test-format davis)")
    fmt = detect_train_format(doc) if fmt == "auto" else fmt
    if fmt == "coco_image" and boundary:
        raise ValueError("--boundary-ap scores YTVIS videos: it is not available with --test-format coco_image "
                         "(Boundary AP of images: --iou-types segm,bbox,boundary)")
    if fmt != "coco_image" and iou_types is not None:
        raise ValueError("--iou-types chooses the tables of a COCO image split: it is not available with --test-format ytvis "
                         "(Boundary AP of videos: --boundary-ap)")
    return fmt


def component_arguments(a, fmt):
    """the component cleanup options of the parsed command line -> the keys they add to the `davis` dict; with any format but davis
    an option that was given is refused by name"""
    given = [name for name, on in (("--min-component-area", a.min_component_area != 0), ("--keep-largest", a.keep_largest),
                                   ("--component-connectivity", a.component_connectivity is not None)) if on]
    if fmt != "davis":
        if given:
            raise ValueError(f"{', '.join(given)} clean{'s' if len(given) == 1 else ''} DAVIS index maps: not available with "
                             f"--test-format {fmt}")
        return {}
    return {"min_component_area": a.min_component_area, "keep_largest": a.keep_largest,
            "component_connectivity": 8 if a.component_connectivity is None else a.component_connectivity}


def fill_arguments(a, fmt):
    """the hole-filling option of the parsed command line -> the key it adds to the `davis` dict; with any format but davis the
    option, if given, is refused by name"""
    if fmt != "davis":
        if a.fill_holes != 0:
            raise ValueError(f"--fill-holes fills DAVIS index maps: not available with --test-format {fmt}")
        return {}
    return {"fill_holes": a.fill_holes}


def evaluate_model(cfg, model, gt, image_root, output_dir, device, threads=8, prefetch=2, boundary=False, dilation_ratio=0.02,
                   test_format="ytvis", iou_types=None, davis=None):
    """score `model` on a YTVIS split: every video through `model([inputs])` (eval mode, predictions as COCO RLE) with the test
    loader and YTVISEvaluator; writes output_dir/results.json and, on rank 0 of a split with annotations, output_dir/metrics.json
    (boundary: Boundary AP as well, and metrics.json holds {"segm", "boundary"}).
    test_format "coco_image" ("auto": decided by the document): a COCO image split instead -- COCOImageTestLoader and
    COCOImageEvaluator, files output_dir/coco_instances_results.json and metrics.json = {"segm", "bbox"}, `images` in the timing line;
    iou_types (image format only; None: ("segm", "bbox")) chooses those dicts, "boundary" among them.
    A directory as `gt` (test_format "davis" or "auto"): a DAVIS tree -- davis_video_document, the model's inference_index switch and
    DAVISEvaluator; `davis` = {"sequences", "rule", "max_proposals", "score_threshold", "bound_th"} (defaults: every sequence, "rank",
    20, 0.0, 0.008) and the cleanup keys "min_component_area", "keep_largest", "component_connectivity" (0, False, 8:
    postprocess.index_map_options; the cleaned maps are the ones scored and written, the timing line gains `removed_pixels`) and
    "fill_holes" (0: off; N or "all": ops.fill_index_holes after the cleanup, the timing line gains `filled_pixels`); files
    output_dir/davis/<sequence>/<frame>.png, the two CSVs and metrics.json = {"davis": the global table}.
    The model's training mode and inference switches are restored afterwards.  -> (results, timing line dict)"""
    from .data.test_loader import YTVISTestLoader
    from .ytvis_eval import YTVISEvaluator
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_initialized() else 0
    is_davis = isinstance(gt, (str, os.PathLike)) and os.path.isdir(gt) and \
        resolve_test_format(test_format, gt, boundary, iou_types) == "davis"
    index_map = None
    if is_davis:
        from .data.davis_loader import davis_video_document
        opt = {"sequences": None, "rule": "rank", "max_proposals": 20, "score_threshold": 0.0, "bound_th": 0.008,
               "min_component_area": 0, "keep_largest": False, "component_connectivity": 8, "fill_holes": 0, **(davis or {})}
        gt_dir, gt = gt, davis_video_document(image_root, gt, opt["sequences"])     # refuses a broken tree before the model runs
        index_map = {"rule": opt["rule"], "max_proposals": opt["max_proposals"], "score_threshold": opt["score_threshold"],
                     "min_component_area": opt["min_component_area"], "keep_largest": opt["keep_largest"],
                     "component_connectivity": opt["component_connectivity"]}
        if opt["fill_holes"] != 0:                                      # a default run passes the dict it passed before
            index_map["fill_holes"] = opt["fill_holes"]
    elif test_format == "davis":
        resolve_test_format(test_format, gt, boundary, iou_types)                    # raises: not a directory
    if isinstance(gt, str):
        with open(gt) as fh:
            gt = json.load(fh)
    # labels -> dataset category ids as the registered dataset's metadata maps them (load_ytvis_json: sorted ids, contiguous)
    id_map = {c: i for i, c in enumerate(sorted(c["id"] for c in gt.get("categories", [])))} or None
    images = not is_davis and resolve_test_format(test_format, gt, boundary, iou_types) == "coco_image"
    iou_types = parse_iou_types(iou_types)
    if is_davis:
        from .davis_eval import DAVISEvaluator
        from .modeling.postprocess import index_map_options
        index_map_options(index_map)
        evaluator = DAVISEvaluator(gt_dir, output_dir, bound_th=opt["bound_th"], max_proposals=opt["max_proposals"], distributed=True,
                                   sequences=[v["name"] for v in gt["videos"]], threads=min(max(int(threads), 1), 16),
                                   video_names={v["id"]: v["name"] for v in gt["videos"]})
        loader = YTVISTestLoader.from_config(cfg, gt, image_root, device=device, threads=threads, prefetch=prefetch)
    elif images:
        from .coco_eval import COCOImageEvaluator
        from .data.coco_image_loader import COCOImageTestLoader
        evaluator = COCOImageEvaluator(json_file=gt, distributed=True, output_dir=output_dir, dataset_id_to_contiguous_id=id_map,
                                       iou_types=iou_types, dilation_ratio=dilation_ratio)
        loader = COCOImageTestLoader.from_config(cfg, gt, image_root, device=device, threads=threads, prefetch=prefetch)
    else:
        evaluator = YTVISEvaluator(json_file=gt, distributed=True, output_dir=output_dir, dataset_id_to_contiguous_id=id_map,
                                   boundary=boundary, dilation_ratio=dilation_ratio)
        loader = YTVISTestLoader.from_config(cfg, gt, image_root, device=device, threads=threads, prefetch=prefetch)
    evaluator.reset()

    was_training, was_rle, was_index = model.training, getattr(model, "inference_rle", False), getattr(model, "inference_index", None)
    model.eval()
    model.inference_rle = not is_davis
    model.inference_index = index_map
    nvid = nfr = nwin = 0
    removed, filled = [], []                                          # device counts of the cleanup and the fill: read after the loop
    try:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        with torch.no_grad():
            for inputs in loader:
                outputs = model([inputs])
                evaluator.process([inputs], outputs)
                if "pred_removed" in outputs:
                    removed.append(outputs["pred_removed"])
                if "pred_filled" in outputs:
                    filled.append(outputs["pred_filled"])
                nvid += 1
                nfr += len(inputs["image"])
                nwin += getattr(model, "last_windows", 1)
        torch.cuda.synchronize(device)
        wall = time.perf_counter() - t0
    finally:
        model.train(was_training)
        model.inference_rle = was_rle
        model.inference_index = was_index

    results = evaluator.evaluate()
    if rank == 0:
        os.makedirs(output_dir, exist_ok=True)
        if is_davis and results:
            with open(os.path.join(output_dir, "metrics.json"), "w") as fh:
                json.dump(results, fh)
        elif images and results:
            with open(os.path.join(output_dir, "metrics.json"), "w") as fh:
                json.dump({k: results[k] for k in iou_types}, fh)
        elif "segm" in results:
            with open(os.path.join(output_dir, "metrics.json"), "w") as fh:
                json.dump({k: results[k] for k in ("segm", "boundary")} if boundary else results["segm"], fh)
    line = {"rank": rank, "images" if images else "videos": nvid, "frames": nfr, "windows": nwin, "wall_s": round(wall, 4),
            "images_per_s" if images else "videos_per_s": round(nvid / wall, 4) if wall > 0 else None,
            "frames_per_s": round(nfr / wall, 3) if wall > 0 else None,
            "loader_wait_fraction": round(loader.wait_s / wall, 4) if wall > 0 else None}
    if is_davis and (opt["min_component_area"] > 0 or opt["keep_largest"]):
        line["removed_pixels"] = sum(int(r.sum()) for r in removed)
    if is_davis and opt["fill_holes"] != 0:
        line["filled_pixels"] = sum(int(f.sum()) for f in filled)
    return results, line


def main(argv=None):
    a = parse_args(argv)
    from .config import load_config
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(a.dist_backend)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    device = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(device)

    cfg = load_config(a.config_file, a.opts)
    iou_types = parse_iou_types(a.iou_types) if a.iou_types is not None else None
    davis = None
    if os.path.isdir(a.gt) or a.test_format == "davis":
        gt_doc = a.gt                                                   # the annotation directory; evaluate_model lists it
        davis = {"sequences": a.sequences, "rule": a.index_rule, "max_proposals": a.max_proposals,
                 "score_threshold": a.score_threshold, "bound_th": a.bound_th}
    else:
        with open(a.gt) as fh:
            gt_doc = json.load(fh)
    fmt = resolve_test_format(a.test_format, gt_doc, a.boundary_ap, iou_types)
    cleanup = {**component_arguments(a, fmt), **fill_arguments(a, fmt)}
    if fmt == "davis":                                                  # a broken tree is refused before the model is built
        from .data.davis_loader import davis_video_document
        from .modeling.postprocess import index_map_options
        index_map_options({"rule": a.index_rule, "max_proposals": a.max_proposals, "score_threshold": a.score_threshold, **cleanup})
        davis.update(cleanup)
        davis_video_document(a.image_root, a.gt, a.sequences)
    model = build_model(cfg, a.weights or cfg.MODEL.WEIGHTS, device)
    results, line = evaluate_model(cfg, model, gt_doc, a.image_root, a.output_dir, device, a.threads, a.prefetch,
                                   boundary=a.boundary_ap, dilation_ratio=a.dilation_ratio, test_format=fmt, iou_types=iou_types,
                                   davis=davis)
    print(json.dumps(line), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return results


if __name__ == "__main__":
    main(sys.argv[1:])
