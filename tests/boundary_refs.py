"""References for the Boundary AP tests that do not restate the kernel (csrc/mask_boundary.hip works on bit planes, separably,
by doubling; these work on bool images with scipy's morphology and on Python integers), and the shared cases."""
import numpy as np
from scipy import ndimage

# the smallest shapes at which the kernel can go wrong, by the property each is named for
SHAPES = {"one_pixel": (1, 1), "one_row": (1, 70), "one_column": (70, 1), "rows_per_word": (7, 5), "w31": (9, 31), "w32": (9, 32),
          "w33": (9, 33), "straddle": (40, 45), "wide_straddle": (37, 100), "aligned": (64, 64)}
RADII = (1, 2, 3, 15, 16, 17, 31, 32, 33, 60, 200)
# where the one-pass kernel hands over to chained passes (radius 64 | 65), and a third pass: frames larger than any listed above,
# since a window that does not fit the image is clamped away before the passes are counted
CHAINED = (((150, 140), 63), ((150, 140), 64), ((150, 140), 65), ((150, 141), 69), ((290, 275), 130))
# more than 32 words per row: two word tiles per row band
WIDE = (((21, 1100), 7),)


def boundary_ref(mask, d):
    """the published mask_to_boundary on a bool image: pad one ring of zeros, erode d times by a 3 x 3 square (the padded
    image's own border taken as 1, as cv2.erode's default border is), crop, mask & ~eroded"""
    m = np.asarray(mask, bool)
    padded = np.pad(m, 1, mode="constant", constant_values=False)
    er = ndimage.binary_erosion(padded, structure=np.ones((3, 3), bool), iterations=int(d), border_value=1)
    return m & ~er[1:-1, 1:-1]


def boundary_square(mask, d):
    """the same band from one erosion by a (2d+1) x (2d+1) square with a zero border"""
    m = np.asarray(mask, bool)
    er = ndimage.minimum_filter(m.astype(np.uint8), size=2 * int(d) + 1, mode="constant", cval=0).astype(bool)
    return m & ~er


def pack_bits(mask, pad_ones=False):
    """bool image (or any bool array, flattened row-major) -> uint32 words: flat pixel i -> word i/32, bit i%32; the padding
    bits of the last word 0, or all 1 (pad_ones)"""
    flat = np.asarray(mask, bool).reshape(-1)
    n = (flat.size + 31) // 32 * 32
    full = np.concatenate([flat, np.full(n - flat.size, bool(pad_ones))])
    return np.packbits(full, bitorder="little").view(np.uint32)


def unpack_bits(words, H, W):
    """uint32 words -> (bool image [H, W], the padding bits of the last word as a bool array)"""
    b = np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little").astype(bool)
    return b[:H * W].reshape(H, W), b[H * W:]


def discs(rng, H, W, n=3, salt=0.02, edge=False):
    """n random discs xor `salt` of salt noise; edge: centres on the image border, so the discs touch it"""
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for j in range(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        if edge:
            cy, cx = ((0, cx), (H - 1, cx), (cy, 0), (cy, W - 1))[j % 4]
        r = rng.uniform(1, max(H, W) / 2.5 + 1)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    if salt:
        m ^= rng.random((H, W)) < salt
    return m


def contents(rng, H, W):
    """the mask contents every shape is checked on: name -> bool image"""
    one = np.zeros((H, W), bool)
    one[H // 2, W // 2] = True
    return {"discs": discs(rng, H, W), "ones": np.ones((H, W), bool), "zeros": np.zeros((H, W), bool), "pixel": one}


def video_boundary_iou_ref(dt, gt, d):
    """dt, gt: one track each, a list of bool images or None (an absent frame: an empty plane) per frame ->
    (intersection, union) of the boundary bands summed over the frames, as Python integers"""
    inter = union = 0
    for a, b in zip(dt, gt):
        ba = boundary_ref(a, d) if a is not None else None
        bb = boundary_ref(b, d) if b is not None else None
        if ba is None and bb is None:
            continue
        if ba is None:
            ba = np.zeros_like(bb)
        if bb is None:
            bb = np.zeros_like(ba)
        inter += int((ba & bb).sum())
        union += int((ba | bb).sum())
    return inter, union


def square_case():
    """the worked AP case: a 64 x 64 one-frame video, the ground truth a 40 x 40 square at rows and columns 10..49, one
    detection the same square two columns to the right -> (gt image, detection image)"""
    g = np.zeros((64, 64), bool)
    g[10:50, 10:50] = True
    return g, np.roll(g, 2, axis=1)
