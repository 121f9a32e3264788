"""A DAVIS tree as the video document the test loader consumes.

    JPEGImages/480p/<sequence>/<frame>.jpg            (image_root)
    Annotations_unsupervised/480p/<sequence>/<frame>.png   (gt_dir)

`davis_video_document` lists the sequences and returns {"videos": [...]} with the keys data/test_loader.YTVISTestLoader reads
(`file_names` relative to the image root, `height`, `width`, `length`, `id`) plus the sequence's `name` and its ground-truth frame
files `gt_files`.  Only headers are read.  Whatever would make the run fail after the model has started is refused here, by file
name: a sequence whose JPEG stems and ground-truth PNG stems differ, frames of more than one size, an RGB ground-truth PNG."""
import os

from ..davis_eval import _open_index, _sequence_names

_JPEG = (".jpg", ".jpeg")


def _stem(f):
    return os.path.splitext(f)[0]


def davis_video_document(image_root, gt_dir, sequences=None):
    """-> {"videos": [{"id", "name", "file_names", "gt_files", "height", "width", "length"}, ...]} in the order of `sequences` (a list of
    names, or a text file with one per line; default: every sub-directory of gt_dir, sorted).  Frame files are sorted by name."""
    from PIL import Image
    videos = []
    for vid, name in enumerate(_sequence_names(gt_dir, sequences), 1):
        idir, gdir = os.path.join(image_root, name), os.path.join(gt_dir, name)
        if not os.path.isdir(gdir):
            raise FileNotFoundError(f"{gdir}: no ground truth for sequence {name}")
        if not os.path.isdir(idir):
            raise FileNotFoundError(f"{idir}: no frames for sequence {name}")
        jpgs = sorted(f for f in os.listdir(idir) if f.lower().endswith(_JPEG))
        pngs = sorted(f for f in os.listdir(gdir) if f.lower().endswith(".png"))
        if not jpgs:
            raise FileNotFoundError(f"{idir}: no JPEG frames")
        js, ps = {_stem(f): f for f in jpgs}, {_stem(f): f for f in pngs}
        for s in sorted(set(js) - set(ps)):
            raise FileNotFoundError(f"{os.path.join(gdir, s + '.png')}: frame {js[s]} of sequence {name} has no ground truth")
        for s in sorted(set(ps) - set(js)):
            raise FileNotFoundError(f"{os.path.join(idir, s + '.jpg')}: ground truth {ps[s]} of sequence {name} has no frame")
        size = None
        for j, p in zip(jpgs, pngs):
            with Image.open(os.path.join(idir, j)) as im:
                jsize = im.size
            with _open_index(os.path.join(gdir, p)) as im:            # raises on an RGB PNG, with the path
                psize = im.size
            size = size or jsize
            for path, sz in ((os.path.join(idir, j), jsize), (os.path.join(gdir, p), psize)):
                if sz != size:
                    raise ValueError(f"{path}: size {sz[1]}x{sz[0]} in a sequence of {size[1]}x{size[0]}")
        videos.append({"id": vid, "name": name, "file_names": [os.path.join(name, f) for f in jpgs], "gt_files": pngs,
                       "height": size[1], "width": size[0], "length": len(jpgs)})
    if not videos:
        raise ValueError(f"{gt_dir}: no sequence")
    return {"videos": videos}
