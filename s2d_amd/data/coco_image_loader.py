"""Test-time loader of the images of a COCO instances document: the image-side sibling of test_loader.YTVISTestLoader, for
`python -m s2d_amd.evaluate --test-format coco_image` and the trainer's eval hook on an image file.

One image is a one-frame video: per image it yields `image` (a list of one CHW uint8 CUDA tensor), `height`, `width`,
`length` = 1, `video_id`, `file_names`, and also `image_id` and `file_name`.  Reading (read_frame: PIL, EXIF orientation, RGB /
BGR), the INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST resize on the device, the side stream, the prefetch queue and the rank sharding are
the video loader's.  The video loader's decode pool only works inside one video, which for images is one thread: here the next
`threads` images are decoded concurrently, ahead of the one being staged, and handed on in the file's order."""
import json
import queue
from concurrent.futures import ThreadPoolExecutor

import torch

from .resize import resize_frames
from .test_loader import YTVISTestLoader, read_frame


def images_as_videos(json_file):
    """the images of a COCO instances document as one-frame video records (load_videos' input), in the file's order"""
    doc = json_file
    if isinstance(json_file, str):
        with open(json_file) as fh:
            doc = json.load(fh)
    return {"videos": [{"id": im["id"], "file_names": [im["file_name"]], "height": im["height"], "width": im["width"], "length": 1}
                       for im in doc["images"]]}


class COCOImageTestLoader(YTVISTestLoader):
    """for inputs in COCOImageTestLoader(...): outputs = model([inputs]) -- arguments as YTVISTestLoader's"""

    def __init__(self, json_file, image_root, *args, **kw):
        super().__init__(images_as_videos(json_file), image_root, *args, **kw)

    def _produce(self, q, stop):
        try:
            torch.cuda.set_device(self.device)
            side = torch.cuda.Stream(self.device)
            with ThreadPoolExecutor(self.threads) as pool:
                futs = {}
                for n, rec in enumerate(self.videos):
                    if stop.is_set():
                        return
                    for k in range(n, min(n + self.threads, len(self.videos))):         # keep `threads` decodes in flight
                        if k not in futs:
                            futs[k] = pool.submit(read_frame, self.videos[k]["file_names"][0], self.fmt)
                    a = futs.pop(n).result()
                    buf = torch.empty((1,) + a.shape, dtype=torch.uint8, pin_memory=True)
                    buf[0].numpy()[...] = a
                    with torch.cuda.stream(side):
                        x = buf.to(self.device, non_blocking=True)
                        img = resize_frames(x, self.output_shape(a.shape[0], a.shape[1]), stream=side.cuda_stream)
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

    def __iter__(self):
        for inputs in super().__iter__():
            inputs["image_id"] = inputs["video_id"]
            inputs["file_name"] = inputs["file_names"][0]
            yield inputs
