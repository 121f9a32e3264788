"""Training driver: `train_net_video.py` + detectron2's DefaultTrainer without detectron2.

    python -m s2d_amd.train --config-file X.yaml --train-json ann.json --image-root DIR --output-dir OUT
           [--train-format auto|ytvis|coco_image] [--weights W.pth] [--resume] [--eval-gt val.json --eval-image-root DIR]
           [--threads N] [KEY VALUE ...]

One process per GPU (or `torch.distributed.run`, gloo or nccl).  The model comes from MODEL.META_ARCHITECTURE through the registry,
its weights from --weights / MODEL.WEIGHTS (checkpoint.load_checkpoint: a plain checkpoint fans out to student and teacher).  The
optimizer is optim.build_optimizer, the LR scheduler solver.build_lr_scheduler.  Each iteration (engine/train_loop.py:690-770):
next batch of the training loader (data/train_loader.py for YTVIS videos; data/image_clip.py for a COCO image annotation
file, RLE or polygons, every image a pseudo-clip of SAMPLING_FRAME_NUM augmented copies: --train-format coco_image, which `auto`
picks for a JSON with `images` and no `videos`), copy-paste with DATALOADER.COPY_PASTE (`copy_and_paste(deepcopy(
data[::-1]), data)`, :703), engine.run_step with the EMA momentum of the iteration, scheduler.step().

EMA: a model with a teacher gets MODEL.MASK_FORMER.EMA_MOMENTUM at iteration 0; with EMA_MOMENTUM_SCHEDULE iteration i > 0 uses
ema_momentum_schedule(i - 1, ...) (the reference updates m after it has used it, :751-768), so a resumed run recomputes it from i.

Loss weights (loss_schedule.py): MODEL.MASK_FORMER.LOSS_WEIGHT_DECAY_STEP (the one-off decay of the supervised weights, :692-699) and
KD_WEIGHT_SCHEDULER linear / cosine with KD_WEIGHT_DECAY_START / _END, SUPERVISED_MIN_WEIGHT, KD_MIN_WEIGHT, DECAY_ONLY_SUPERVISED_LOSS
and DECAY_ONLY_KD_LOSS (:776-811) are honoured for KDVideoMaskFormer: iteration i trains with LossWeightSchedule.weights_at(i), the
dict the reference's model sees at self.iter == i (it updates the dict after it has used it, like m).  weights_at is a pure function of
i, so a resumed run gets the weights of the uninterrupted run; the reference restarts from the initial weights on resume.  An
active schedule prints one JSON line at start and adds weight/<key> for the six base keys to every metrics.json record; with the
default keys nothing is applied and every output is what it was without the schedule.  --resume also puts the per-process seed
counters (point sampling, dropout) where the uninterrupted run has them at that iteration, so that the two runs draw the same
points and masks.

Logs: every 20 iterations (and at the last) rank 0 appends one JSON line to OUT/metrics.json in the layout of detectron2's
JSONWriter (losses averaged over ranks, median over the window; lr and grad_norm latest; time and data_time median; data_time
is the wait for the batch plus copy-paste, as the reference measures it).  Small collectives (seed, losses) run on the host
under gloo and on the GPU under nccl.  At the end
one summary JSON line is printed.  A non-finite loss stops the run.  Checkpoints follow PeriodicCheckpointer: OUT/model_{iter:07d}.pth
when (iter + 1) % CHECKPOINT_PERIOD == 0, OUT/model_final.pth at MAX_ITER - 1, each {"model", "optimizer", "scheduler",
"iteration", "seed"}, OUT/last_checkpoint names the latest; rank 0 writes.  --resume restores model, optimizer, scheduler and
continues at iteration + 1; with SEED < 0 it also reuses the saved sampler seed, so the resumed run draws the clips an
uninterrupted run would (with SEED >= 0 the config's seed is used).
With --eval-gt the model is scored (evaluate.evaluate_model) every TEST.EVAL_PERIOD iterations and after the last one, into
OUT/inference/.  An --eval-gt document with `images` and no `videos` is scored as COCO images (coco_eval.COCOImageEvaluator: mask
AP and box AP, OUT/inference/metrics.json = {"segm", "bbox"}); a YTVIS document as before; a directory is a DAVIS annotation tree
(--eval-image-root: JPEGImages/480p; evaluate.py --test-format davis with its defaults, metrics.json = {"davis"}).

Not supported (refused): INPUT.DISENTANGLE_DISTILLATION_LOADER (the meta-archs take no distill_image), optimizers other than
ADAMW, and of the loss-weight keys: a KD_WEIGHT_SCHEDULER other than constant / linear / cosine; linear or cosine with
KD_WEIGHT_DECAY_END <= KD_WEIGHT_DECAY_START (the reference divides by zero) or with KD_WEIGHT_DECAY_END < SOLVER.MAX_ITER (past the
end the reference extrapolates: supervised weights fall below their minimum and can turn negative); a negative
SUPERVISED_MIN_WEIGHT or KD_MIN_WEIGHT.  SOLVER.AMP.ENABLED is ignored with a message: the arithmetic is fp32-class, as in evaluate.py."""
import argparse
import copy
import json
import logging
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

_log = logging.getLogger("s2d_amd.train")
LOG_PERIOD = 20


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="train a meta-architecture on a YTVIS-format annotation file")
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--train-json", required=True, help="YTVIS annotation JSON to train on (ground truth or pseudo labels), or a "
                    "COCO image annotation JSON (--train-format)")
    ap.add_argument("--train-format", choices=("auto", "ytvis", "coco_image"), default="auto",
                    help="auto: coco_image when the JSON has `images` and no `videos`, else ytvis")
    ap.add_argument("--image-root", required=True, help="directory the JSON's file_names are relative to")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--weights", default=None, help="initial weights, torch .pth or detectron2 .pkl (default: MODEL.WEIGHTS)")
    ap.add_argument("--resume", action="store_true", help="continue from OUTPUT_DIR/last_checkpoint")
    ap.add_argument("--eval-gt", default=None, help="YTVIS or COCO image annotation JSON, or a DAVIS annotation directory, to score on (EvalHook)")
    ap.add_argument("--eval-image-root", default=None)
    ap.add_argument("--threads", type=int, default=8, help="JPEG decode threads (<= 16)")
    ap.add_argument("--prefetch", type=int, default=2, help="batches prepared ahead")
    ap.add_argument("--dist-backend", default="gloo", help="process group backend under torch.distributed.run")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="config overrides KEY VALUE ...")
    a = ap.parse_args(argv)
    if a.eval_gt and not a.eval_image_root:
        ap.error("--eval-gt needs --eval-image-root")
    return a


def check_config(cfg, world=1):
    """the configurations this driver refuses, before anything touches the GPU"""
    if cfg.INPUT.DISENTANGLE_DISTILLATION_LOADER:
        raise ValueError("INPUT.DISENTANGLE_DISTILLATION_LOADER True is not supported: the meta-architectures take no distill_image")
    if cfg.SOLVER.OPTIMIZER != "ADAMW":
        raise ValueError(f"SOLVER.OPTIMIZER {cfg.SOLVER.OPTIMIZER} is not supported: only ADAMW runs on the device")
    if int(cfg.SOLVER.IMS_PER_BATCH) % world:
        raise ValueError(f"SOLVER.IMS_PER_BATCH ({cfg.SOLVER.IMS_PER_BATCH}) must be divisible by the number of workers ({world})")
    from .loss_schedule import check_schedule_config
    check_schedule_config(cfg)
    if cfg.SOLVER.AMP.ENABLED:
        _log.warning("SOLVER.AMP.ENABLED is ignored: the library's arithmetic is fp32-class")


def checkpoints_at(iteration, period, max_iter):
    """PeriodicCheckpointer.step: the file names saved after `iteration`"""
    out = []
    if period > 0 and (iteration + 1) % period == 0:
        out.append(f"model_{iteration:07d}.pth")
    if iteration >= max_iter - 1:
        out.append("model_final.pth")
    return out


def ema_momentum_at(cfg, iteration, accum_iter=1):
    """the EMA momentum run_step gets at `iteration` (never None for a model with a teacher)"""
    from .optim import ema_momentum_schedule
    mf = cfg.MODEL.MASK_FORMER
    if not mf.EMA_MOMENTUM_SCHEDULE or iteration == 0:
        return float(mf.EMA_MOMENTUM)
    return float(ema_momentum_schedule(iteration - 1, mf.EMA_MOMENTUM, mf.EMA_MOMENTUM_END, mf.EMA_MOMENTUM_UNTIL_STEP, accum_iter))


def seed_draws_per_iteration(model):
    """the per-process seed counters one run_step call advances: (criterion.seed and matcher.seed, ops._DROP_CALLS).  Each criterion
    call draws one point-sampling seed and one matcher seed (ground truth, and pseudo targets for a model with a teacher); every
    deformable encoder layer in training mode with dropout draws one Philox key per forward."""
    from .modeling.pixel_decoder import MSDeformAttnTransformerEncoderLayer
    crit = 2 if getattr(model, "teacher", None) is not None else 1
    drop = sum(1 for m in model.modules() if isinstance(m, MSDeformAttnTransformerEncoderLayer) and m.training and m.dropout_p > 0.0)
    return crit, drop


def fast_forward_seeds(model, iteration):
    """put the seed counters where an uninterrupted run has them before `iteration`, so that a resumed run draws the same sampled
    points and dropout masks (the counters are not part of a checkpoint: they are a function of the iteration)"""
    from . import ops
    crit, drop = seed_draws_per_iteration(model)
    model.criterion.seed = model.criterion.matcher.seed = crit * int(iteration)
    ops._DROP_CALLS[0] = drop * int(iteration)


def save_checkpoint(out_dir, name, model, optimizer, scheduler, iteration, seed=None):
    """{"model", "optimizer", "scheduler", "iteration"} (+ "seed": the sampler seed the run used, so that a resumed run of a
    config with SEED < 0 draws the same clips)"""
    path = os.path.join(out_dir, name)
    tmp = path + ".tmp"
    ck = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "optimizer": optimizer.state_dict(),
          "scheduler": scheduler.state_dict(), "iteration": int(iteration)}
    if seed is not None:
        ck["seed"] = int(seed)
    torch.save(ck, tmp)
    os.replace(tmp, path)
    with open(os.path.join(out_dir, "last_checkpoint"), "w") as fh:
        fh.write(name)
    return path


def load_resume(out_dir):
    """-> the checkpoint OUT/last_checkpoint names, or None"""
    p = os.path.join(out_dir, "last_checkpoint")
    if not os.path.exists(p):
        return None
    with open(p) as fh:
        name = fh.read().strip()
    return torch.load(os.path.join(out_dir, name), map_location="cpu", weights_only=True)


def collective_device(dist, device):
    """where the driver's small collectives run: the host for a gloo group, `device` otherwise (an "nccl" group has no CPU
    backend)"""
    return torch.device("cpu") if dist.get_backend() == "gloo" else torch.device(device)


def _shared_seed(seed, dist, device="cpu"):
    """SEED < 0: a random seed drawn on rank 0 and shared (detectron2's shared_random_seed)"""
    if seed >= 0:
        return int(seed)
    s = int(np.random.SeedSequence().generate_state(1)[0] & 0x7FFFFFFF)
    if dist.is_initialized() and dist.get_world_size() > 1:
        t = torch.tensor([s], dtype=torch.int64, device=collective_device(dist, device))
        dist.broadcast(t, 0)
        s = int(t.cpu())
    return s


def _reduce_losses(values, dist, device="cpu"):
    """[n] float64 host vector averaged over the ranks"""
    if not (dist.is_initialized() and dist.get_world_size() > 1):
        return [float(v) for v in values]
    t = torch.tensor(values, dtype=torch.float64, device=collective_device(dist, device))
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    t /= dist.get_world_size()
    return t.cpu().tolist()


def broadcast_model(model, dist):
    """every rank starts from rank 0's parameters and buffers, as DistributedDataParallel's construction makes them"""
    from .checkpoint import invalidate_weight_caches
    if not (dist.is_initialized() and dist.get_world_size() > 1):
        return
    invalidate_weight_caches(model)
    with torch.no_grad():
        for v in model.state_dict().values():
            if dist.get_backend() == "gloo" and v.is_cuda:
                h = v.cpu()
                dist.broadcast(h, 0)
                v.copy_(h)
            else:
                dist.broadcast(v, 0)


def main(argv=None):
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(name)s %(levelname)s: %(message)s")
    from .config import load_config
    world = int(os.environ.get("WORLD_SIZE", "1"))
    cfg = load_config(a.config_file, a.opts)
    check_config(cfg, world)

    import torch.distributed as dist
    from .checkpoint import load_checkpoint
    from .data.copy_paste import copy_and_paste
    from .data.image_clip import COCOImageTrainLoader, detect_train_format, load_coco_image_train
    from .data.train_loader import YTVISTrainLoader, load_ytvis_train
    from .engine import run_step
    from .evaluate import evaluate_model
    from .loss_schedule import BASE_KEYS, LossWeightSchedule
    from .modeling.meta_arch import META_ARCH_REGISTRY
    from .optim import build_optimizer
    from .solver import build_lr_scheduler
    local = int(os.environ.get("LOCAL_RANK", "0"))
    device = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(device)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(a.dist_backend)
    rank = dist.get_rank() if dist.is_initialized() else 0
    os.makedirs(a.output_dir, exist_ok=True)

    ck = load_resume(a.output_dir) if a.resume else None
    if ck is not None and int(cfg.SEED) < 0 and "seed" in ck:
        seed = int(ck["seed"])                                 # the resumed run continues the same sample stream
    else:
        seed = _shared_seed(int(cfg.SEED), dist, device)
    random.seed(seed + rank)                                   # detectron2 seed_all_rng(seed + rank): copy-paste, dropout
    np.random.seed((seed + rank) & 0xFFFFFFFF)
    torch.manual_seed(seed + rank)

    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE).from_config(cfg).to(device)
    weights = a.weights or cfg.MODEL.WEIGHTS
    if weights:
        load_checkpoint(model, weights)
    else:
        _log.warning("no initial weights: training from the module initialisation")
    broadcast_model(model, dist)
    model.train()
    optimizer = build_optimizer(cfg, model)
    scheduler = build_lr_scheduler(cfg, optimizer)
    start_iter = 0
    if ck is not None:
        load_checkpoint(model, ck["model"])
        optimizer.load_state_dict(ck["optimizer"])
        scheduler.load_state_dict(ck["scheduler"])
        start_iter = int(ck["iteration"]) + 1
        del ck
    max_iter, period = int(cfg.SOLVER.MAX_ITER), int(cfg.SOLVER.CHECKPOINT_PERIOD)
    eval_period = int(cfg.TEST.EVAL_PERIOD)
    has_teacher = getattr(model, "teacher", None) is not None
    if start_iter > 0:
        fast_forward_seeds(model, start_iter)
    schedule = LossWeightSchedule(cfg, model.criterion.weight_dict)
    accum = max(int(getattr(model, "accum_iter", 1)), 1)
    dl = cfg.DATALOADER
    if rank == 0:
        print(json.dumps({"start_iter": start_iter, "max_iter": max_iter, "optimizer_step": optimizer._step, "seed": seed}), flush=True)
        if schedule.active:
            print(json.dumps(schedule.describe()), flush=True)

    with open(a.train_json) as fh:
        doc = json.load(fh)
    fmt = detect_train_format(doc) if a.train_format == "auto" else a.train_format
    if fmt == "coco_image":
        records, loader_cls = load_coco_image_train(doc, a.image_root, dl.FILTER_EMPTY_ANNOTATIONS), COCOImageTrainLoader
    else:
        records, loader_cls = load_ytvis_train(doc, a.image_root, dl.FILTER_EMPTY_ANNOTATIONS), YTVISTrainLoader
    del doc
    loader = loader_cls.from_config(cfg, records, rank, world, seed, start_iter=start_iter, device=device, threads=a.threads,
                                    prefetch=a.prefetch)

    def run_eval():
        if a.eval_gt:
            out = os.path.join(a.output_dir, "inference")
            results, line = evaluate_model(cfg, model, a.eval_gt, a.eval_image_root, out, device, a.threads, test_format="auto")
            if rank == 0:
                print(json.dumps({"eval_iteration": it, **line, **{k: results[k] for k in ("segm", "bbox", "davis") if k in results}}),
                      flush=True)

    hist, names = [], None
    n_iter, clips = 0, 0
    it = start_iter - 1
    torch.cuda.synchronize(device)
    t_start = time.perf_counter()
    t_prev = t_start
    wait0 = 0.0
    data_iter = iter(loader)
    try:
        for it in range(start_iter, max_iter):
            t_data = time.perf_counter()
            data = next(data_iter)
            if dl.COPY_PASTE:
                data = copy_and_paste(copy.deepcopy(data[::-1]), data, dl.COPY_PASTE_RATE, dl.COPY_PASTE_RANDOM_NUM,
                                      dl.COPY_PASTE_MIN_RATIO, dl.COPY_PASTE_MAX_RATIO, dl.COPY_PASTE_DENSIFY_SPARSE)
            data_time = time.perf_counter() - t_data          # as train_loop.py:702-704: the wait for the batch + copy-paste
            ema_m = ema_momentum_at(cfg, it, accum) if has_teacher else None
            weights = schedule.apply(model, it) if schedule.active else None
            losses = run_step(model, optimizer, data, it, ema_m)
            if names is None:
                names = sorted(losses)
            vals = torch.stack([losses[k].detach().float().reshape(()) for k in names]).cpu().double().tolist()
            lr = optimizer.param_groups[0]["lr"]
            scheduler.step()
            vals = _reduce_losses(vals, dist, device)
            total = float(sum(vals))
            if not math.isfinite(total):
                raise FloatingPointError(f"loss became infinite or NaN at iteration={it}: "
                                         + ", ".join(f"{k}={v}" for k, v in zip(names, vals)))
            t_now = time.perf_counter()
            hist.append((vals, total, t_now - t_prev, data_time))
            hist = hist[-LOG_PERIOD:]
            t_prev = t_now
            n_iter += 1
            clips += len(data)
            if rank == 0 and ((it + 1) % LOG_PERIOD == 0 or it == max_iter - 1):
                rec = {"iteration": it}
                for j, k in enumerate(names):
                    rec[k] = statistics.median(h[0][j] for h in hist)
                rec["total_loss"] = statistics.median(h[1] for h in hist)
                rec["lr"] = lr
                rec["grad_norm"] = optimizer.grad_norm() if optimizer.clip_norm > 0 else None
                rec["time"] = statistics.median(h[2] for h in hist)
                rec["data_time"] = statistics.median(h[3] for h in hist)
                if weights is not None:
                    rec.update({f"weight/{k}": weights[k] for k in BASE_KEYS if k in weights})
                with open(os.path.join(a.output_dir, "metrics.json"), "a") as fh:
                    fh.write(json.dumps(rec) + "\n")
            if rank == 0:
                for name in checkpoints_at(it, period, max_iter):
                    save_checkpoint(a.output_dir, name, model, optimizer, scheduler, it, seed)
            if a.eval_gt and eval_period > 0 and (it + 1) % eval_period == 0 and it != max_iter - 1:
                run_eval()
        torch.cuda.synchronize(device)
        wall = time.perf_counter() - t_start
        waited = loader.wait_s - wait0
    finally:
        data_iter.close()
    if a.eval_gt:
        run_eval()
    if rank == 0:
        print(json.dumps({"iterations": n_iter, "clips": clips * world, "wall_s": round(wall, 4),
                          "clips_per_s": round(clips * world / wall, 4) if wall > 0 else None,
                          "loader_wait_fraction": round(waited / wall, 4) if wall > 0 else None}), flush=True)
    if dist.is_initialized() and dist.get_world_size() > 1:
        # every rank's student after the last step: data-parallel training keeps them identical
        import hashlib
        h = hashlib.sha1()
        for p in (model.student if hasattr(model, "student") else model).parameters():
            h.update(p.detach().cpu().numpy().tobytes())
        print(json.dumps({"rank": rank, "student_digest": h.hexdigest()}), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
