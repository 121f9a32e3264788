"""DAVIS J&F evaluation of a folder of index PNGs (`<sequence>/<frame>.png`, or the `<sequence>/mask_<frame>.png` that
`python -m s2d_amd.demo --save-frames True --save-masks True` writes) against DAVIS ground truth: J&F-Mean, J / F mean,
recall and decay, for the unsupervised and the semi-supervised task.

The metric restates the DAVIS-2017 evaluation code (Pont-Tuset et al., "The 2017 DAVIS Challenge on Video Object
Segmentation"; Perazzi et al., CVPR 2016).  The DAVIS toolkit is not part of this stack (no cv2, no skimage, no davis2017), so
PARITY WITH THE TOOLKIT IS UNPINNED: the definition below, written out literally in tests/davis_refs.py, is what the numbers mean.

  labels    index value k in 1..K is object k; 255 in the ground truth is void and is cleared from both masks first; the ground
            truth's objects are 1..max label of the sequence
  J         |P & G| / |P | G| per frame, 1 when the union is empty
  boundary  b = (M != E) | (M != S) | (M != SE), east / south / south-east neighbours with the image edge replicated (seg2bmap
            without resize)
  radius    R = ceil(bound_th * sqrt(H^2 + W^2)) for bound_th < 1, else bound_th; the structuring element is the disk
            dx^2 + dy^2 <= R^2, pixels outside the image count as 0
  F         precision = |b_P & dil(b_G)| / |b_P|, recall = |b_G & dil(b_P)| / |b_G|; (1, 0) without a proposal boundary,
            (0, 1) without a ground-truth boundary, (1, 1) without both; F = 2PR / (P + R), 0 if P + R = 0
  unsupervised     proposals are the result labels 1..P, P <= max_proposals, padded with empty ones up to the number of objects;
            every (proposal, object, frame) is scored, objects take proposals by linear_sum_assignment(-(mean_t J + mean_t F) / 2)
  semi-supervised  proposal k against object k (a missing one is empty), first and last frame dropped
  statistics       per object over its frames: mean, recall = mean(v > 0.5), decay = mean(first quarter) - mean(last quarter)
            with the bins of db_statistics; the global table averages them over all objects of all sequences.

The device does integer work only (csrc/davis_eval.hip: index maps -> bit planes, boundary maps, disk dilations, per-frame pair
popcounts; plane areas from csrc/ytvis_eval.hip); every quotient is float64 on the host from exact integers, as in
ytvis_eval.video_ious.  There is no CPU fallback.  The assignment is scipy's linear_sum_assignment.

    python -m s2d_amd.davis_eval --gt DIR --results DIR [--sequences FILE] [--task unsupervised|semi-supervised]
                                 [--bound-th 0.008] [--out DIR]
"""
import argparse
import csv
import math
import os
from collections import OrderedDict

import numpy as np

from .ytvis_eval import plane_areas

TASKS = ("unsupervised", "semi-supervised")
GLOBAL_KEYS = ("J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay")
MAX_RADIUS = 64


def davis_bound_pix(H, W, bound_th=0.008):
    """the dilation radius of the F-measure for an H x W frame"""
    if bound_th >= 1:
        if int(bound_th) != bound_th:
            raise ValueError(f"bound_th = {bound_th}: a radius in pixels is an integer")
        return int(bound_th)
    return int(math.ceil(bound_th * math.sqrt(H * H + W * W)))


# --------------------------------------------------------------------------------------------------------------- device
def _words(H, W):
    return (H * W + 31) // 32


def index_planes(index, K):
    """uint8 CUDA index maps [T, H, W] -> (int32 planes [K, T, wpf] of the labels 1..K, int32 void plane [T, wpf] of label
    255); labels K+1..254 set no bit (s2d_index_planes_u32)"""
    import torch
    from . import ops
    from ._lib import lib
    ops._chk(index, torch.uint8)
    if index.dim() != 3 or not 0 <= K <= 254:
        raise ValueError(f"index planes: maps of shape {tuple(index.shape)}, K = {K}")
    T, H, W = index.shape
    planes = torch.empty((K, T, _words(H, W)), device=index.device, dtype=torch.int32)
    void = torch.empty((T, _words(H, W)), device=index.device, dtype=torch.int32)
    if T:
        lib().call("s2d_index_planes_u32", index, T, H, W, K, planes if K else None, void, ops._stream())
    return planes, void


def _chk_planes(bits, H, W):
    import torch
    from . import ops
    ops._chk(bits, torch.int32)
    if bits.dim() != 2 or bits.shape[1] != _words(H, W):
        raise ValueError(f"planes of shape {tuple(bits.shape)} for a {H}x{W} image")


def seg2bmap_planes(bits, H, W):
    """int32 CUDA bit planes [F, ceil(H*W/32)] -> their boundary maps in the same layout (s2d_seg2bmap_bits_u32)"""
    import torch
    from . import ops
    from ._lib import lib
    _chk_planes(bits, H, W)
    out = torch.empty_like(bits)
    if bits.shape[0]:
        lib().call("s2d_seg2bmap_bits_u32", bits, bits.shape[0], H, W, out, ops._stream())
    return out


def disk_dilate_planes(bits, H, W, R):
    """int32 CUDA bit planes [F, ceil(H*W/32)] -> the planes dilated by the disk dx^2 + dy^2 <= R^2 with a zero border,
    1 <= R <= 64 (s2d_disk_dilate_bits_u32)"""
    import torch
    from . import ops
    from ._lib import lib
    _chk_planes(bits, H, W)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"disk dilation takes a radius of 1..{MAX_RADIUS}, not {R} ({H}x{W} frames)")
    out = torch.empty_like(bits)
    if bits.shape[0]:
        lib().call("s2d_disk_dilate_bits_u32", bits, bits.shape[0], H, W, int(R), out, ops._stream())
    return out


def frame_cross_counts(a, b):
    """int32 CUDA planes a [P, T, wpf], b [G, T, wpf] -> int32 CUDA [P, G, T]: popcount(a[p, t] & b[g, t])
    (s2d_mask_frame_cross_counts_i32)"""
    import torch
    from . import ops
    from ._lib import lib
    ops._chk(a, torch.int32); ops._chk(b, torch.int32)
    if a.dim() != 3 or b.dim() != 3 or a.shape[1:] != b.shape[1:]:
        raise ValueError(f"frame cross counts of planes {tuple(a.shape)} and {tuple(b.shape)}")
    P, T, wpf = a.shape
    G = b.shape[0]
    out = torch.zeros((P, G, T), device=a.device, dtype=torch.int32)
    if P and G and T:
        lib().call("s2d_mask_frame_cross_counts_i32", a, P, b, G, T, wpf, out, ops._stream())
    return out


# --------------------------------------------------------------------------------------------------------------- metric
def _jaccard(inter, area_p, area_g):
    union = area_p + area_g - inter
    J = np.ones(inter.shape)
    pos = union > 0
    J[pos] = inter[pos] / union[pos]
    return J


def _f_measure(pm, rm, n_fg, n_gt):
    prec, rec = np.ones(pm.shape), np.ones(pm.shape)
    both = (n_fg > 0) & (n_gt > 0)
    prec[both] = pm[both] / n_fg[both]
    rec[both] = rm[both] / n_gt[both]
    rec[(n_fg == 0) & (n_gt > 0)] = 0.0
    prec[(n_fg > 0) & (n_gt == 0)] = 0.0
    s = prec + rec
    F = np.zeros(pm.shape)
    nz = s != 0
    F[nz] = 2 * prec[nz] * rec[nz] / s[nz]
    return F


def _host(t, shape):
    return t.cpu().numpy().astype(np.int64).reshape(shape)


def _max_labels(index):
    """-> (largest label, largest label below 255) of an index video, numpy or tensor"""
    if isinstance(index, np.ndarray):
        return (int(index.max()), int(np.where(index == 255, 0, index).max())) if index.size else (0, 0)
    import torch
    return (int(index.max()), int(torch.where(index == 255, torch.zeros_like(index), index).max())) if index.numel() else (0, 0)


def sequence_metrics(gt_index, res_index, task="unsupervised", bound_th=0.008, max_proposals=20, device=None):
    """uint8 index videos [T, H, W] of one sequence (numpy or CUDA tensors) -> {"J": float64 [G, T'], "F": float64 [G, T'],
    "assignment": int64 [G], the 0-based proposal each object took, "radius": R}; T' = T, or T - 2 for the semi-supervised task"""
    import torch
    if task not in TASKS:
        raise ValueError(f"task {task!r}: one of {TASKS}")
    if tuple(gt_index.shape) != tuple(res_index.shape) or len(gt_index.shape) != 3:
        raise ValueError(f"ground truth {tuple(gt_index.shape)} and results {tuple(res_index.shape)}")
    T, H, W = (int(v) for v in gt_index.shape)
    R = davis_bound_pix(H, W, bound_th)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"bound_th = {bound_th} makes a radius of {R} on {H}x{W} frames: 1..{MAX_RADIUS} is supported")
    G = _max_labels(gt_index)[1]
    semi = task == "semi-supervised"
    if semi:
        if T < 3:
            raise ValueError(f"the semi-supervised task drops the first and last frame: {T} frames leave none")
        P = G
    else:
        P = _max_labels(res_index)[0]
        if P > max_proposals:
            raise ValueError(f"{P} proposals, more than max_proposals = {max_proposals}")
    Tk = T - 2 if semi else T
    if G == 0:
        return {"J": np.zeros((0, Tk)), "F": np.zeros((0, Tk)), "assignment": np.zeros(0, np.int64), "radius": R}
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    up = lambda a: (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(dev).contiguous()
    gplanes, void = index_planes(up(gt_index), G)
    pplanes, _ = index_planes(up(res_index), P)
    keep = ~void
    gplanes &= keep
    pplanes &= keep
    Pn = max(P, G)
    if Pn > P:                                                          # fewer proposals than objects: empty ones fill up
        pplanes = torch.cat([pplanes, torch.zeros((Pn - P,) + tuple(pplanes.shape[1:]), device=dev, dtype=torch.int32)])
    wpf = gplanes.shape[2]
    flat_p, flat_g = pplanes.view(Pn * T, wpf), gplanes.view(G * T, wpf)
    bnd_p, bnd_g = seg2bmap_planes(flat_p, H, W), seg2bmap_planes(flat_g, H, W)
    dil_p, dil_g = disk_dilate_planes(bnd_p, H, W, R), disk_dilate_planes(bnd_g, H, W, R)
    area_p, area_g = _host(plane_areas(flat_p), (Pn, T)), _host(plane_areas(flat_g), (G, T))
    n_fg, n_gt = _host(plane_areas(bnd_p), (Pn, T)), _host(plane_areas(bnd_g), (G, T))
    if semi:                                                            # object k against proposal k: (k, t) as one frame axis
        one = lambda x: x.view(1, G * T, wpf)
        inter = _host(frame_cross_counts(one(flat_p), one(flat_g)), (G, T))
        pm = _host(frame_cross_counts(one(bnd_p), one(dil_g)), (G, T))
        rm = _host(frame_cross_counts(one(dil_p), one(bnd_g)), (G, T))
        J = _jaccard(inter, area_p, area_g)[:, 1:-1]
        F = _f_measure(pm, rm, n_fg, n_gt)[:, 1:-1]
        return {"J": np.ascontiguousarray(J), "F": np.ascontiguousarray(F), "assignment": np.arange(G), "radius": R}
    tri = lambda x, n: x.view(n, T, wpf)
    inter = _host(frame_cross_counts(pplanes, gplanes), (Pn, G, T))
    pm = _host(frame_cross_counts(tri(bnd_p, Pn), tri(dil_g, G)), (Pn, G, T))
    rm = _host(frame_cross_counts(tri(dil_p, Pn), tri(bnd_g, G)), (Pn, G, T))
    shape = (Pn, G, T)
    Jall = _jaccard(inter, np.broadcast_to(area_p[:, None, :], shape), np.broadcast_to(area_g[None], shape))
    Fall = _f_measure(pm, rm, np.broadcast_to(n_fg[:, None, :], shape), np.broadcast_to(n_gt[None], shape))
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(-(np.mean(Jall, axis=2) + np.mean(Fall, axis=2)) / 2)
    assign = np.zeros(G, np.int64)
    assign[cols] = rows
    J = np.stack([Jall[assign[g], g] for g in range(G)])
    F = np.stack([Fall[assign[g], g] for g in range(G)])
    return {"J": J, "F": F, "assignment": assign, "radius": R}


def db_statistics(v):
    """per-frame values of one object -> (mean, recall, decay)"""
    v = np.asarray(v, np.float64)
    ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.int64)
    bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
    return float(np.mean(v)), float(np.mean(v > 0.5)), float(np.mean(bins[0]) - np.mean(bins[3]))


def tables(per_sequence):
    """{sequence name: sequence_metrics result} -> (global table, per-sequence rows `<sequence>_<object>`: J-Mean, F-Mean)"""
    cols = OrderedDict((k, []) for k in GLOBAL_KEYS[1:])
    rows = []
    for name, r in per_sequence.items():
        for g in range(r["J"].shape[0]):
            stats = db_statistics(r["J"][g]) + db_statistics(r["F"][g])
            for k, v in zip(cols, stats):
                cols[k].append(v)
            rows.append(OrderedDict([("Sequence", f"{name}_{g + 1}"), ("J-Mean", stats[0]), ("F-Mean", stats[3])]))
    if not rows:
        raise ValueError("no object in any sequence: nothing to average")
    table = OrderedDict((k, float(np.mean(v))) for k, v in cols.items())
    table["J&F-Mean"] = (table["J-Mean"] + table["F-Mean"]) / 2
    table.move_to_end("J&F-Mean", last=False)
    return table, rows


# --------------------------------------------------------------------------------------------------------------- files
def _sequence_names(gt_dir, sequences):
    if sequences is None:
        return sorted(d for d in os.listdir(gt_dir) if os.path.isdir(os.path.join(gt_dir, d)))
    if isinstance(sequences, (str, os.PathLike)):
        with open(sequences) as fh:
            return [s for s in (line.strip() for line in fh) if s]
    return list(sequences)


def _open_index(path):
    from PIL import Image
    im = Image.open(path)
    if im.mode not in ("P", "L"):
        raise ValueError(f"{path}: an index PNG is in mode P or L, this one is {im.mode}")
    return im


def read_index_png(path):
    """a `P` or `L` mode PNG -> uint8 index map [H, W]"""
    with _open_index(path) as im:
        return np.array(im, dtype=np.uint8)


def _check_files(gt_dir, results_dir, names):
    """-> {sequence: (ground-truth frame files, result frame files)}; every frame exists on both sides in mode P / L and in one
    size (headers only).  A result frame is `<frame>.png`, or `mask_<frame>.png` where that exists (what the demo writes beside
    its overlay frames)"""
    frames = OrderedDict()
    for name in names:
        gdir = os.path.join(gt_dir, name)
        if not os.path.isdir(gdir):
            raise FileNotFoundError(f"{gdir}: no ground truth for sequence {name}")
        files = sorted(f for f in os.listdir(gdir) if f.lower().endswith(".png"))
        if not files:
            raise FileNotFoundError(f"{gdir}: no PNG frames")
        rfiles = []
        for f in files:
            rf = "mask_" + f if os.path.isfile(os.path.join(results_dir, name, "mask_" + f)) else f     # the demo's name for its index PNG
            rpath = os.path.join(results_dir, name, rf)
            if not os.path.isfile(rpath):
                raise FileNotFoundError(f"{rpath}: result frame missing")
            with _open_index(os.path.join(gdir, f)) as g, _open_index(rpath) as r:
                if r.size != g.size:
                    raise ValueError(f"{rpath}: size {r.size[1]}x{r.size[0]}, its ground truth is {g.size[1]}x{g.size[0]}")
            rfiles.append(rf)
        frames[name] = (files, rfiles)
    return frames


def _read_video(root, name, files, limit=None):
    out = []
    for f in files:
        path = os.path.join(root, name, f)
        fr = read_index_png(path)
        if out and fr.shape != out[0].shape:
            raise ValueError(f"{path}: size {fr.shape[0]}x{fr.shape[1]} in a sequence of {out[0].shape[0]}x{out[0].shape[1]}")
        if limit is not None and int(fr.max()) > limit:
            raise ValueError(f"{path}: label {int(fr.max())}, more than max_proposals = {limit} proposals")
        out.append(fr)
    return np.stack(out)


def evaluate_davis(gt_dir, results_dir, *, sequences=None, task="unsupervised", bound_th=0.008, max_proposals=20, device=None):
    """score results_dir/<sequence>/<frame>.png against gt_dir/<sequence>/<frame>.png -> {"global": the J&F table,
    "per_sequence": rows `<sequence>_<object>` with J-Mean and F-Mean, "sequences": {name: sequence_metrics result}}.
    sequences: a list of names, or a text file with one per line; default every sub-directory of gt_dir.  An RGB result, a
    missing result frame, a frame whose size differs from its ground truth and (unsupervised task) a label above max_proposals
    raise with the file's name before any device work: the result frames are decoded once for that check and again when their
    sequence is scored, so that one sequence's maps are on the host at a time."""
    if task not in TASKS:
        raise ValueError(f"task {task!r}: one of {TASKS}")
    frames = _check_files(gt_dir, results_dir, _sequence_names(gt_dir, sequences))
    if task == "unsupervised":
        for name, (_, rfiles) in frames.items():
            _read_video(results_dir, name, rfiles, limit=max_proposals)
    per = OrderedDict()
    for name, (files, rfiles) in frames.items():
        gt, res = _read_video(gt_dir, name, files), _read_video(results_dir, name, rfiles)
        per[name] = sequence_metrics(gt, res, task=task, bound_th=bound_th, max_proposals=max_proposals, device=device)
    table, rows = tables(per)
    return {"global": table, "per_sequence": rows, "sequences": per}


# --------------------------------------------------------------------------------------------------------------- palette, writing
def _voc_colour(i):
    """entry i of the PASCAL-VOC colour map: for j = 0..7, bits 3j, 3j + 1, 3j + 2 of i become bit 7 - j of r, g, b"""
    r = g = b = 0
    for j in range(8):
        r |= ((i >> 0) & 1) << (7 - j)
        g |= ((i >> 1) & 1) << (7 - j)
        b |= ((i >> 2) & 1) << (7 - j)
        i >>= 3
    return [r, g, b]


# 256 entries: the first 13 are the demo's PALETTE (what its mask PNGs carry; they differ from the formula by 191 for 192), the
# rest the VOC formula, so that all 20 proposals of the unsupervised protocol -- and any label up to 255 -- have a colour
DAVIS_PALETTE = [0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0, 0, 0, 128, 128, 0, 128, 0, 128, 128, 128, 128, 128, 64, 0, 0, 191, 0, 0,
                 64, 128, 0, 191, 128, 0, 64, 0, 128] + [c for i in range(13, 256) for c in _voc_colour(i)]


def save_index_png(path, index):
    """uint8 index map [H, W] -> a P-mode PNG with DAVIS_PALETTE (read_index_png reads the labels back)"""
    from PIL import Image
    index = np.ascontiguousarray(index)
    if index.dtype != np.uint8 or index.ndim != 2:
        raise ValueError(f"{path}: an index map is uint8 [H, W], not {index.dtype} {index.shape}")
    im = Image.fromarray(index)
    im.putpalette(DAVIS_PALETTE)                                        # an L image with a palette is saved in mode P
    im.save(path)


# --------------------------------------------------------------------------------------------------------------- driver side
def merge_sequence_results(parts, names):
    """parts: per rank, a list of (sequence name, sequence_metrics result) -> OrderedDict in the order of `names`.  A sequence
    scored twice or not at all, or one that is not in the list, is an error: the ranks split the list, nothing else"""
    got = {}
    for part in parts:
        for name, r in part:
            if name in got:
                raise ValueError(f"sequence {name} was scored by more than one rank")
            got[name] = r
    extra = sorted(set(got) - set(names))
    if extra:
        raise ValueError(f"results for sequences the list does not have: {extra}")
    missing = [n for n in names if n not in got]
    if missing:
        raise ValueError(f"no result for sequences {missing}")
    return OrderedDict((n, got[n]) for n in names)


class DAVISEvaluator:
    """reset / process(inputs, outputs) / evaluate() on the proposal index maps a model returns (`inference_index`,
    modeling/postprocess.inference_video index_map=...): `process` reads the sequence's ground-truth PNGs and scores the CUDA index
    tensor where it is (sequence_metrics), and queues the PNGs output_dir/davis/<sequence>/<frame>.png to a small thread pool;
    evaluate() gathers the per-sequence results of all ranks, orders them by the sequence list, writes global_results.csv and
    per-sequence_results.csv and returns {"davis": the global table}.  Only the unsupervised task: the model takes no first-frame
    mask.  PARITY WITH THE DAVIS TOOLKIT IS UNPINNED (module docstring)."""

    def __init__(self, gt_dir, output_dir=None, task="unsupervised", bound_th=0.008, max_proposals=20, distributed=True, sequences=None,
                 threads=4, video_names=None):
        if task not in TASKS:
            raise ValueError(f"task {task!r}: one of {TASKS}")
        if task != "unsupervised":
            raise ValueError("the semi-supervised task needs a first-frame mask, which the model does not take: DAVISEvaluator scores "
                             "the unsupervised task (a folder of semi-supervised results: python -m s2d_amd.davis_eval --task semi-supervised)")
        if not 1 <= int(threads) <= 16:
            raise ValueError("threads must be in [1, 16]")
        self._gt_dir, self._output_dir, self._distributed = gt_dir, output_dir, distributed
        self._bound_th, self._max_proposals, self._threads = bound_th, int(max_proposals), int(threads)
        self._names = _sequence_names(gt_dir, sequences)
        self._video_names = dict(video_names or {})                     # video_id -> sequence name (davis_video_document's records)
        self._pool, self._writes = None, []
        self.reset()

    def reset(self):
        self._drain()
        self._results = []

    def _drain(self):
        for fu in self._writes:
            fu.result()                                                 # a failed write raises here
        self._writes = []
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None

    def process(self, inputs, outputs):
        """inputs: one video of the test loader over davis_video_document (`name`, `file_names`); outputs: inference_video's dict with
        "pred_masks_format": "index_u8" """
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        video = inputs[0]
        out = outputs[0] if isinstance(outputs, (list, tuple)) else outputs
        if out.get("pred_masks_format") != "index_u8":
            raise ValueError("DAVISEvaluator scores proposal index maps: set the model's inference_index (pred_masks_format 'index_u8')")
        # the loader's records carry video_id and file_names: the sequence is the id's name in the document, else the frames' folder
        name = video.get("name") or self._video_names.get(video.get("video_id")) or os.path.basename(os.path.dirname(video["file_names"][0]))
        if name not in self._names:
            raise ValueError(f"sequence {name} is not in the sequence list")
        stems = [os.path.splitext(os.path.basename(f))[0] for f in video["file_names"]]
        gt = _read_video(self._gt_dir, name, [s + ".png" for s in stems])
        index = out["pred_masks"]
        if tuple(index.shape) != gt.shape:
            raise ValueError(f"sequence {name}: index maps {tuple(index.shape)}, ground truth {gt.shape}")
        r = sequence_metrics(gt, index, task="unsupervised", bound_th=self._bound_th, max_proposals=self._max_proposals,
                             device=index.device)
        self._results.append((name, r))
        if self._output_dir:
            from concurrent.futures import ThreadPoolExecutor
            if self._pool is None:
                self._pool = ThreadPoolExecutor(self._threads)
            sdir = os.path.join(self._output_dir, "davis", name)
            os.makedirs(sdir, exist_ok=True)
            host = index.cpu().numpy()
            self._writes += [self._pool.submit(save_index_png, os.path.join(sdir, s + ".png"), host[t]) for t, s in enumerate(stems)]

    def evaluate(self):
        self._drain()
        parts = [self._results]
        try:
            import torch.distributed as dist
            if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                parts = [None] * dist.get_world_size()
                dist.all_gather_object(parts, self._results)
                if dist.get_rank() != 0:
                    return {}
        except ImportError:
            pass
        per = merge_sequence_results(parts, self._names)
        table, rows = tables(per)
        self.result = {"global": table, "per_sequence": rows, "sequences": per}
        if self._output_dir:
            write_csvs(self.result, self._output_dir)
        return {"davis": dict(table)}


# --------------------------------------------------------------------------------------------------------------- CLI
def format_table(table):
    keys = list(table)
    return "\n".join([" ".join(f"{k:>9}" for k in keys), " ".join(f"{table[k]:9.3f}" for k in keys)])


def write_csvs(result, out_dir):
    """global_results.csv and per-sequence_results.csv, three decimals"""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "global_results.csv"), "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(list(result["global"]))
        w.writerow([f"{v:.3f}" for v in result["global"].values()])
    with open(os.path.join(out_dir, "per-sequence_results.csv"), "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Sequence", "J-Mean", "F-Mean"])
        for r in result["per_sequence"]:
            w.writerow([r["Sequence"], f"{r['J-Mean']:.3f}", f"{r['F-Mean']:.3f}"])


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="DAVIS J&F of a folder of index PNGs (toolkit parity unpinned)")
    ap.add_argument("--gt", required=True, help="ground truth: DIR/<sequence>/<frame>.png")
    ap.add_argument("--results", required=True, help="results: DIR/<sequence>/<frame>.png")
    ap.add_argument("--sequences", default=None, help="text file of sequence names (default: every sub-directory of --gt)")
    ap.add_argument("--task", default="unsupervised", choices=TASKS)
    ap.add_argument("--bound-th", type=float, default=0.008)
    ap.add_argument("--max-proposals", type=int, default=20)
    ap.add_argument("--out", default=None, help="directory for global_results.csv and per-sequence_results.csv")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    result = evaluate_davis(a.gt, a.results, sequences=a.sequences, task=a.task, bound_th=a.bound_th, max_proposals=a.max_proposals)
    print(format_table(result["global"]))
    if a.out:
        write_csvs(result, a.out)
    return result


if __name__ == "__main__":
    main()
