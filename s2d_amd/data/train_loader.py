"""Training loader of YTVIS-format videos: the reference's train-time data path (load_ytvis_json, data_video/datasets/ytvis.py:259-389;
filter_images_with_only_crowd_annotations, data_video/build.py:38-71; detectron2's TrainingSampler and AspectRatioGroupedDataset;
YTVISDatasetMapper(is_train=True), data_video/dataset_mapper.py:294-474) without detectron2, with the annotation masks decoded and
warped on the device.

Per clip (`map_clip`): frames are selected on the host (data/sampling.py), the augmentation drawn (ClipAugmentation.sample), the
JPEGs decoded as read_image decodes them, and then on the device: the frames go up as decoded ([T][H0][W0][3]) and are warped by
s2d_aug_warp_frames_hwc_u8; the clip's RLE strings are parsed and decoded to bit planes (ytvis_eval.stage_rle / decode_staged) and
s2d_aug_warp_mask_bits warps them straight into the slot order of the mapper, counting each plane's pixels.  filter_empty_instances
is `gt_ids = -1` where that count is 0.  The dict is the one assemble_clip_instances + augment_clip give.

Randomness: the loader never draws from the global `random` / `numpy.random` (the trainer's copy-paste does).  Clip j of the
global sample stream draws from its own pair of generators seeded from (seed, j), so a run resumed at iteration k sees exactly the
clips an uninterrupted run sees from k on."""
import json
import os
import queue
import random
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .assemble import clip_id_slots
from .augment import ClipAugmentation, augment_frames_hwc, warp_mask_bits
from .sampling import dense_frame_selection, random_frame_selection
from .test_loader import MAX_THREADS, read_frame

_ANN_KEYS = ("iscrowd", "category_id", "id")


# ------------------------------------------------------------------------------------------------------------------ dataset
def load_ytvis_train(json_file, image_root, filter_empty=True):
    """load_ytvis_json for training: one record per video (sorted by id) with `annotations[frame]` = list of {"id",
    "category_id" (contiguous, sorted order), "iscrowd" (if present), "segmentation" (RLE dict)}.  A frame's object is skipped
    where its bbox or segmentation is null.  filter_empty: drop videos without a non-crowd annotation (DATALOADER.
    FILTER_EMPTY_ANNOTATIONS).  Polygons are not supported; an RLE whose size is not the video's is an error."""
    doc = json.load(open(json_file)) if isinstance(json_file, str) else json_file
    cat_ids = sorted(c["id"] for c in doc.get("categories", []))
    id_map = {v: i for i, v in enumerate(cat_ids)}
    by_vid = {}
    for a in doc.get("annotations", []):
        by_vid.setdefault(a["video_id"], []).append(a)
    out = []
    for v in sorted(doc["videos"], key=lambda v: v["id"]):
        vid, H, W, L = v["id"], v["height"], v["width"], v["length"]
        frames = []
        for f in range(L):
            objs = []
            for a in by_vid.get(vid, []):
                bb, sg = a.get("bboxes"), a.get("segmentations")
                if not (bb and sg and bb[f] and sg[f]):
                    continue
                seg = sg[f]
                if not isinstance(seg, dict):
                    raise NotImplementedError(f"video {vid}: polygon segmentations are not supported: convert them to RLE")
                if [int(s) for s in seg["size"]] != [H, W]:
                    raise ValueError(f"video {vid}: RLE of size {seg['size']} in a video of size {[H, W]}")
                obj = {k: a[k] for k in _ANN_KEYS if k in a}
                obj["segmentation"] = seg
                if id_map:
                    obj["category_id"] = id_map[obj["category_id"]]
                objs.append(obj)
            frames.append(objs)
        out.append({"file_names": [os.path.join(image_root, n) for n in v["file_names"][:L]], "height": H, "width": W,
                    "length": L, "video_id": vid, "annotations": frames})
    if filter_empty:
        out = [r for r in out if any(o.get("iscrowd", 0) == 0 for fr in r["annotations"] for o in fr)]
    return out


# ------------------------------------------------------------------------------------------------------------------ sampling
def clip_generators(seed, index):
    """the (random.Random, numpy RandomState) pair clip `index` of the global sample stream draws from"""
    a, b = np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(index)]).generate_state(2)
    return random.Random(int(a)), np.random.RandomState(int(b))


def global_indices(n, seed):
    """TrainingSampler._infinite_indices: an endless stream of seeded permutations of range(n) -> (position, dataset index)"""
    g = torch.Generator()
    g.manual_seed(int(seed))
    pos = 0
    while True:
        for i in torch.randperm(n, generator=g).tolist():
            yield pos, i
            pos += 1


def batch_plan(records, seed, batch, rank=0, world=1, aspect_grouping=True):
    """the per-rank batches of TrainingSampler (rank r takes stream positions r::world) + AspectRatioGroupedDataset (buckets
    w > h and w <= h, a batch is yielded when its bucket fills): an endless iterator of lists of (position, dataset index)"""
    buckets = ([], [])
    cur = []
    for pos, i in global_indices(len(records), seed):
        if pos % world != rank:
            continue
        if aspect_grouping:
            r = records[i]
            b = buckets[0 if r["width"] > r["height"] else 1]
            b.append((pos, i))
            if len(b) == batch:
                yield list(b)
                del b[:]
        else:
            cur.append((pos, i))
            if len(cur) == batch:
                yield cur
                cur = []


# ------------------------------------------------------------------------------------------------------------------ the mapper
def _device(device):
    d = torch.device(device) if device is not None else torch.device("cuda")
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


class ClipSettings:
    """what the mapper reads from the config"""

    def __init__(self, cfg):
        self.aug = ClipAugmentation.from_config(cfg)
        i = cfg.INPUT
        self.num_frames, self.frame_range, self.shuffle = i.SAMPLING_FRAME_NUM, i.SAMPLING_FRAME_RANGE, i.SAMPLING_FRAME_SHUFFLE
        self.dense = bool(i.DENSE_ANNOTATION_SELECTION)
        self.fmt = i.FORMAT
        self.num_classes = cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES


def plan_clip(record, py_rng, np_rng, st):
    """host half of the mapper: frame selection, augmentation parameters, slot numbering and the plane of every (frame, slot)"""
    annos, L = record["annotations"], record["length"]
    if st.dense:
        sel = dense_frame_selection(annos, L, st.num_frames, st.frame_range, st.shuffle, py_rng, np_rng)
    else:
        sel = random_frame_selection(L, st.num_frames, st.frame_range, st.shuffle, py_rng, np_rng)
    sel = [int(f) for f in sel]
    T, H0, W0 = len(sel), record["height"], record["width"]
    params, out_hw = st.aug.sample(T, H0, W0, rng=np_rng)
    ids = clip_id_slots(annos, sel)
    S = len(ids)
    plane_of = np.full((T, S), -1, np.int32)
    gt_ids = np.full((T, S), -1, np.int64)
    classes = np.full((T, S), st.num_classes, np.int64)
    segs = []
    for t, f in enumerate(sel):
        for a in annos[f]:
            if a.get("iscrowd", 0) != 0:
                continue
            s = ids[a["id"]]
            plane_of[t, s] = len(segs)
            segs.append(a["segmentation"])
            gt_ids[t, s] = a["id"]
            classes[t, s] = a["category_id"]
    return {"record": record, "selected": sel, "params": params, "out_hw": out_hw, "plane_of": plane_of, "gt_ids": gt_ids,
            "gt_classes": classes, "segs": segs}


def _read_frames(plan, pool, fmt):
    """futures (or arrays, without a pool) of the selected frames, decoded as read_image decodes them"""
    names = [plan["record"]["file_names"][f] for f in plan["selected"]]
    return [pool.submit(read_frame, n, fmt) for n in names] if pool is not None else [read_frame(n, fmt) for n in names]


def _stage_frames(plan, frames):
    """the decoded frames (arrays or futures) -> one pinned [T][H0][W0][3] buffer"""
    rec = plan["record"]
    H0, W0 = rec["height"], rec["width"]
    buf = torch.empty((len(frames), H0, W0, 3), dtype=torch.uint8, pin_memory=True)
    for t, a in enumerate(frames):
        a = a.result() if hasattr(a, "result") else a
        if a.shape[:2] != (H0, W0):
            raise ValueError(f"video {rec['video_id']}: frame {rec['file_names'][plan['selected'][t]]} is {a.shape[:2]}, "
                             f"the record says {(H0, W0)}")
        buf[t].numpy()[...] = a
    return buf


def _launch_clip(plan, frames_pinned, device):
    """device half on the current stream: frames and RLE go up non-blocking from pinned memory, then decode, warp, count"""
    from ..ytvis_eval import decode_staged, stage_rle
    rec = plan["record"]
    H0, W0 = rec["height"], rec["width"]
    x = frames_pinned.to(device, non_blocking=True)
    p = torch.from_numpy(np.ascontiguousarray(plan["params"], np.float32)).pin_memory().to(device, non_blocking=True)
    img = augment_frames_hwc(x, p, plan["out_hw"])
    bits = decode_staged(stage_rle(plan["segs"], H0, W0), H0, W0, device, pinned=True)
    masks, area = warp_mask_bits(bits, plan["plane_of"], H0, W0, p, plan["out_hw"])
    area_h = torch.empty(area.shape, dtype=torch.int32, pin_memory=True)
    area_h.copy_(area, non_blocking=True)
    return img, masks, area_h


def _finish_clip(plan, img, masks, area_h):
    """filter_empty_instances on the counts (call after the stream that produced area_h has been synchronised)"""
    rec = plan["record"]
    gt_ids = plan["gt_ids"].copy()
    gt_ids[area_h.numpy() == 0] = -1
    mb = masks.view(torch.bool)
    T = img.shape[0]
    inst = [{"gt_masks": mb[t], "gt_ids": gt_ids[t].copy(), "gt_classes": plan["gt_classes"][t].copy()} for t in range(T)]
    return {"image": [img[t] for t in range(T)], "instances": inst, "height": rec["height"], "width": rec["width"],
            "length": rec["length"], "video_id": rec["video_id"], "file_names": [rec["file_names"][f] for f in plan["selected"]]}


def map_clip(record, py_rng, np_rng, settings, device=None, pool=None):
    """the train-time mapper on one clip, synchronously on the current stream: -> the dict of assemble_clip_instances +
    augment_clip ({"image": T x u8 [3,H1,W1], "instances": T x {"gt_masks" bool [S,H1,W1], "gt_ids", "gt_classes"}, ...})"""
    device = _device(device)
    plan = plan_clip(record, py_rng, np_rng, settings)
    buf = _stage_frames(plan, _read_frames(plan, pool, settings.fmt))
    img, masks, area_h = _launch_clip(plan, buf, device)
    torch.cuda.current_stream(device).synchronize()
    return _finish_clip(plan, img, masks, area_h)


# ------------------------------------------------------------------------------------------------------------------ the loader
class YTVISTrainLoader:
    """it = iter(YTVISTrainLoader(...)); data = next(it): an endless stream of per-rank batches (lists of mapper dicts).

    batch: clips per rank (SOLVER.IMS_PER_BATCH // world); seed: the sampler seed shared by every rank; start_iter: the first
    batch (a resumed run); threads: JPEG decode threads (<= 16); prefetch: batches prepared ahead.  `wait_s` accumulates the time
    the consumer spent blocked on the loader."""

    # the mapper's halves: a subclass maps another kind of record through the same sampler, prefetch thread and side stream
    _plan, _read, _stage = staticmethod(plan_clip), staticmethod(_read_frames), staticmethod(_stage_frames)
    _launch, _finish = staticmethod(_launch_clip), staticmethod(_finish_clip)

    def __init__(self, records, settings, batch, seed, rank=0, world=1, aspect_grouping=True, start_iter=0, device=None,
                 threads=8, prefetch=2):
        if not 1 <= int(threads) <= MAX_THREADS:
            raise ValueError(f"threads must be in [1, {MAX_THREADS}]")
        if int(prefetch) < 1:
            raise ValueError("prefetch must be >= 1")
        if not records:
            raise ValueError("no training videos")
        self.records, self.settings, self.batch, self.seed = records, settings, int(batch), int(seed)
        self.rank, self.world, self.aspect_grouping, self.start_iter = int(rank), int(world), bool(aspect_grouping), int(start_iter)
        self.device = _device(device)
        self.threads, self.prefetch = int(threads), int(prefetch)
        self.wait_s = 0.0

    @classmethod
    def from_config(cls, cfg, records, rank=0, world=1, seed=0, **kw):
        ims = int(cfg.SOLVER.IMS_PER_BATCH)
        if ims % world:
            raise ValueError(f"SOLVER.IMS_PER_BATCH ({ims}) must be divisible by the number of workers ({world})")
        return cls(records, ClipSettings(cfg), ims // world, seed, rank, world, cfg.DATALOADER.ASPECT_RATIO_GROUPING, **kw)

    def plans(self):
        """the clip plans of every batch from start_iter on (host only: what a resumed loader must reproduce)"""
        for k, b in enumerate(batch_plan(self.records, self.seed, self.batch, self.rank, self.world, self.aspect_grouping)):
            if k < self.start_iter:
                continue
            yield [self._plan(self.records[i], *clip_generators(self.seed, pos), self.settings) for pos, i in b]

    def _produce(self, q, stop):
        try:
            torch.cuda.set_device(self.device)
            side = torch.cuda.Stream(self.device)
            with ThreadPoolExecutor(self.threads) as pool:
                for plans in self.plans():
                    if stop.is_set():
                        return
                    futs = [self._read(p, pool, self.settings.fmt) for p in plans]         # every frame of the batch at once
                    bufs = [self._stage(p, f) for p, f in zip(plans, futs)]
                    with torch.cuda.stream(side):
                        outs = [self._launch(p, b, self.device) for p, b in zip(plans, bufs)]
                        ev = torch.cuda.Event()
                        ev.record(side)
                    ev.synchronize()                         # this thread only: the pixel counts decide gt_ids
                    item = ([self._finish(p, *o) for p, o in zip(plans, outs)], [(o[0], o[1]) for o in outs], ev)
                    while not stop.is_set():
                        try:
                            q.put(item, timeout=0.1)
                            break
                        except queue.Full:
                            continue
        except BaseException as e:                           # handed to the consumer
            q.put(e)

    def __iter__(self):
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        th = threading.Thread(target=self._produce, args=(q, stop), daemon=True)
        th.start()
        try:
            while True:
                t0 = time.perf_counter()
                item = q.get()
                self.wait_s += time.perf_counter() - t0
                if isinstance(item, BaseException):
                    raise item
                data, tensors, ev = item
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                for img, masks in tensors:
                    img.record_stream(cur)
                    masks.record_stream(cur)
                yield data
        finally:
            stop.set()
            while th.is_alive():
                try:
                    q.get(timeout=0.1)
                except queue.Empty:
                    pass
            th.join()
