"""Test-time loader of YTVIS-format videos: the reference's YTVISDatasetMapper(is_train=False) behind build_test_loader
(train_net_video.py:120-123; data_video/dataset_mapper.py:294-404), over a YTVIS JSON and an image root, without detectron2.

Per video it yields the mapper's dict: `image` (the T frames as CHW uint8 CUDA tensors, ALL frames of the video), `height`,
`width`, `length`, `video_id`, `file_names`.  Frames are read as detectron2's read_image reads them (PIL, EXIF orientation tag
274 applied, converted to RGB; BGR flips the channels) and resized with ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST),
i.e. PIL's bilinear, by the bit-exact device kernel of data/resize.py.

JPEG decode runs in a bounded thread pool and fills pinned host buffers for the next `prefetch` videos; the host-to-device
copy and the resize run on a side stream, ordered to the consumer's stream by an event, so decoding video i+1 overlaps the
inference of video i.  With torch.distributed initialised and world size > 1, rank r takes videos r, r + world, ... (the
evaluator gathers the ranks' records)."""
import json
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .augment import shortest_edge_shape
from .resize import resize_frames

_EXIF_ORIENT = 274
MAX_THREADS = 16


def read_frame(path, fmt="RGB"):
    """detectron2 utils.read_image: PIL open -> EXIF orientation -> convert -> HWC uint8 numpy"""
    from PIL import Image
    with Image.open(path) as im:
        try:
            exif = im.getexif()
        except Exception:
            exif = None
        method = None
        if exif is not None:
            method = {2: Image.Transpose.FLIP_LEFT_RIGHT, 3: Image.Transpose.ROTATE_180, 4: Image.Transpose.FLIP_TOP_BOTTOM,
                      5: Image.Transpose.TRANSPOSE, 6: Image.Transpose.ROTATE_270, 7: Image.Transpose.TRANSVERSE,
                      8: Image.Transpose.ROTATE_90}.get(exif.get(_EXIF_ORIENT))
        img = im.transpose(method) if method is not None else im
        arr = np.asarray(img.convert("RGB"))
    if fmt == "BGR":
        arr = arr[:, :, ::-1]
    elif fmt != "RGB":
        raise NotImplementedError(f"INPUT.FORMAT {fmt}")
    return np.ascontiguousarray(arr)


def load_videos(json_file, image_root):
    """load_ytvis_json's video records (file names joined to the image root), in the file's order"""
    doc = json.load(open(json_file)) if isinstance(json_file, str) else json_file
    out = []
    for v in doc["videos"]:
        out.append({"file_names": [os.path.join(image_root, f) for f in v["file_names"]], "height": v["height"],
                    "width": v["width"], "length": v["length"], "video_id": v["id"]})
    return out


class YTVISTestLoader:
    """for inputs in YTVISTestLoader(...): outputs = model([inputs])

    min_size / max_size: INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST (MIN_SIZE_TEST 0: no resize); threads: decode threads (<= 16);
    prefetch: videos decoded ahead of the consumer (1 or 2).  `wait_s` accumulates the time the consumer spent blocked on the
    loader."""

    def __init__(self, json_file, image_root, min_size=360, max_size=1333, fmt="RGB", device=None, threads=8, prefetch=2,
                 shard=True):
        if not 1 <= int(threads) <= MAX_THREADS:
            raise ValueError(f"threads must be in [1, {MAX_THREADS}]")
        if int(prefetch) not in (1, 2):
            raise ValueError("prefetch must be 1 or 2")
        self.videos = load_videos(json_file, image_root)
        if shard and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            self.videos = self.videos[torch.distributed.get_rank()::torch.distributed.get_world_size()]
        self.min_size, self.max_size, self.fmt = int(min_size), int(max_size), fmt
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.threads, self.prefetch = int(threads), int(prefetch)
        self.wait_s = 0.0

    @classmethod
    def from_config(cls, cfg, json_file, image_root, **kw):
        return cls(json_file, image_root, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, cfg.INPUT.FORMAT, **kw)

    def __len__(self):
        return len(self.videos)

    def output_shape(self, h, w):
        if self.min_size == 0:
            return h, w
        return shortest_edge_shape(h, w, self.min_size, self.max_size)

    # ---------------------------------------------------------------------------------------------------- producer side
    def _decode_video(self, pool, rec):
        futs = [pool.submit(read_frame, f, self.fmt) for f in rec["file_names"]]
        buf = None
        for t, fu in enumerate(futs):
            a = fu.result()
            if buf is None:
                buf = torch.empty((len(futs),) + a.shape, dtype=torch.uint8, pin_memory=True)
                shape = a.shape
            elif a.shape != shape:
                raise ValueError(f"video {rec['video_id']}: frame {rec['file_names'][t]} is {a.shape[:2]}, frame 0 is {shape[:2]}")
            buf[t].numpy()[...] = a
        return buf

    def _produce(self, q, stop):
        try:
            torch.cuda.set_device(self.device)
            side = torch.cuda.Stream(self.device)
            with ThreadPoolExecutor(self.threads) as pool:
                for rec in self.videos:
                    if stop.is_set():
                        return
                    buf = self._decode_video(pool, rec)
                    T, H0, W0, _ = buf.shape
                    with torch.cuda.stream(side):
                        x = buf.to(self.device, non_blocking=True)
                        img = resize_frames(x, self.output_shape(H0, W0), stream=side.cuda_stream)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    while not stop.is_set():
                        try:
                            q.put((rec, img, ev), timeout=0.1)
                            break
                        except queue.Full:
                            continue
            q.put(None)
        except BaseException as e:               # handed to the consumer
            q.put(e)

    # ---------------------------------------------------------------------------------------------------- consumer side
    def __iter__(self):
        import time
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        th = threading.Thread(target=self._produce, args=(q, stop), daemon=True)
        th.start()
        try:
            while True:
                t0 = time.perf_counter()
                item = q.get()
                self.wait_s += time.perf_counter() - t0
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                rec, img, ev = item
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                img.record_stream(cur)
                yield {"image": [img[t] for t in range(img.shape[0])], "height": rec["height"], "width": rec["width"],
                       "length": rec["length"], "video_id": rec["video_id"], "file_names": list(rec["file_names"])}
        finally:
            stop.set()
            while th.is_alive():
                try:
                    q.get(timeout=0.1)
                except queue.Empty:
                    pass
            th.join()
