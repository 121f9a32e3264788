"""Independent references and case builders for the keymask kernels (csrc/keymask.hip) and the YTVIS-evaluator kernels
(csrc/ytvis_eval.hip), and the proof, without a GPU, that the cases are what they claim to be.  tests/test_gpu_discovery_eval.py
imports the references and the builders from here and compares the kernels with them, exactly.

References (plain numpy / CPU torch; nothing of libs2d_hip.so, and no call into the C oracle inside them)
  ref_point_id_counts   np.rint on float32, non-finite and out-of-frame points dropped, the set of distinct pixels, each mapped through
                        CPU F.interpolate(ids.float(), size=(H, W), mode="nearest") (what cotracker_matching.py:688 calls), np.bincount.
  palette frames        colours chosen by the table's key -> slot function ((key * 2654435761) mod 2^32) >> 19; the id maps themselves
                        are checked against np.unique / searchsorted (oracle.color_masks_to_ids, which is exactly that).
  rle_fr_string / rle_to_string / rle_decode_np   maskApi.c's rleFrString / rleToString / rleDecode as sequential Python, with the
                        m > 2 delta and the uint truncation; run ends clamped to h * w, pixels behind the last run 0.
  decode_words_torch    the same decode as whole-tensor torch operations in chunks (for planes too large for a per-pixel host array);
                        proved equal to rle_decode_np here, on the CPU.
  rle_to_bbox           maskApi.c's rleToBbox on run counts.
  ref_visibility        count / Np rounded once to float32.
  ref_local_corr        float64, the sampling position taken as the float32 sum coords + offset; with the per-element bound
                        (C + 8) * 2^-24 * sum_c (sum_k |w_k f_k|) |s_c|: a float32 chain of C fused multiply-adds has first-order
                        error C * 2^-24 * sum |terms|; each staged neighbourhood value carries the roundings of 1 - f (1), the weight
                        product (1), and per tap a product and a sum (the four-tap blend): at most 8 * 2^-24 of sum_k |w_k f_k|."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import golden

U32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ keymask: counts
def nearest_src_f32(out, inp):
    """F.interpolate(mode="nearest") source index per destination index: floor(dst * (float32)(inp / out)), capped"""
    scale = np.float32(inp) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), inp - 1)


def nearest_src_exact(out, inp):
    return np.arange(out, dtype=np.int64) * inp // out


def discriminating(out, inp):
    """destination indices at which the float32 rule and the exact quotient pick different source indices"""
    return np.flatnonzero(nearest_src_f32(out, inp) != nearest_src_exact(out, inp))


def ref_point_id_counts(tracks, H, W, ids, max_id):
    """tracks f32 [T,P,2] (x, y), ids int [T,Hi,Wi] -> (counts int32 [T,max_id+1], total int32 [T])"""
    tr = np.asarray(tracks, np.float32)
    T = tr.shape[0]
    ids = np.asarray(ids, np.int64)
    assert np.abs(ids).max(initial=0) < 2 ** 24                       # .float() keeps them exact
    res = F.interpolate(torch.from_numpy(ids).float()[:, None], size=(H, W), mode="nearest")[:, 0].numpy().astype(np.int64)
    counts = np.zeros((T, max_id + 1), np.int32)
    total = np.zeros((T,), np.int32)
    r = np.rint(tr)
    for t in range(T):
        x, y = r[t, :, 0], r[t, :, 1]
        ok = np.isfinite(x) & np.isfinite(y)
        ok &= (x >= 0) & (x < W) & (y >= 0) & (y < H)
        pix = np.unique(y[ok].astype(np.int64) * W + x[ok].astype(np.int64))
        v = res[t].reshape(-1)[pix]
        total[t] = len(pix)
        v = v[(v >= 0) & (v <= max_id)]
        counts[t] = np.bincount(v, minlength=max_id + 1)
    return counts, total


# (frame H, W) <- (id map Hi, Wi)
RESIZE_CASES = {"small_93x62": ((21, 14), (93, 62)), "small_124x84": ((14, 20), (124, 84)), "up_480_to_720": ((720, 1280), (480, 854)),
                "down_720_to_480": ((480, 854), (720, 1280)), "identity": ((47, 83), (47, 83))}
# cases the issue names as discriminating, per axis: (out, in)
DISCRIMINATING_AXES = {"small_93x62": [(21, 93), (14, 62)], "small_124x84": [(14, 124), (20, 84)]}
POISON = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 1e19, -1e19, 3.4e38, -3.4e38], np.float32)


def edge_tracks(rng, T, P, H, W, Hi, Wi):
    """P points per frame: every row and column where the two nearest rules differ gets points along its whole length (as far as P
    allows), then exact halves, duplicates, points around and outside the frame"""
    rows, cols = discriminating(H, Hi), discriminating(W, Wi)
    pts = []
    if H * W <= P:
        yy, xx = np.mgrid[:H, :W]
        pts.append(np.stack([xx.reshape(-1), yy.reshape(-1)], -1))
    else:
        for y in rows:
            xs = np.unique(np.concatenate([[0, W - 1], rng.integers(0, W, 24)]))
            pts.append(np.stack([xs, np.full_like(xs, y)], -1))
        for x in cols:
            ys = np.unique(np.concatenate([[0, H - 1], rng.integers(0, H, 8)]))
            pts.append(np.stack([np.full_like(ys, x), ys], -1))
    fixed = np.concatenate(pts, 0).astype(np.float32) if pts else np.zeros((0, 2), np.float32)
    fixed = fixed[:P]
    out = np.empty((T, P, 2), np.float32)
    for t in range(T):
        n = P - len(fixed)
        xy = np.stack([rng.integers(-3, W + 3, n), rng.integers(-3, H + 3, n)], -1).astype(np.float32)
        xy += rng.choice(np.array([0.0, 0.5, -0.5, 0.49999997, 1.5, 0.25], np.float32), (n, 2))
        if n > 4:
            xy[rng.integers(0, n, n // 4)] = xy[rng.integers(0, n, n // 4)]
        out[t] = np.concatenate([fixed + rng.choice(np.array([0.0, 0.25, -0.5], np.float32), fixed.shape) * (t > 0), xy], 0)
    return out


def poisoned_tracks(rng, T, P, H, W):
    """-> (tracks [T,P,2] with non-finite / huge coordinates, keep mask [T,P] of the untouched points).  Every POISON value appears
    in x alone, in y alone and in both, the other coordinate inside the frame."""
    tr = np.stack([rng.integers(0, W, (T, P)), rng.integers(0, H, (T, P))], -1).astype(np.float32)
    tr += rng.choice(np.array([0.0, 0.5, -0.25], np.float32), tr.shape)
    keep = np.ones((T, P), bool)
    k = 0
    for t in range(T):
        for v in POISON:
            for where in ((0,), (1,), (0, 1)):
                p = (k * 7 + 3) % P
                while not keep[t, p]:
                    p = (p + 1) % P
                for a in where:
                    tr[t, p, a] = v
                keep[t, p] = False
                k += 1
    return tr, keep


def test_ref_counts_equal_the_oracle_on_the_golden(oracle):
    g = golden("keymask")
    tracks, idm = g["tracks"][0], g["idmap"].astype(np.int64)
    idm = idm[..., 0] if idm.ndim == 4 else idm
    T, H, W = idm.shape
    H2, W2 = (int(v) for v in g["resized_dims"])
    tr2 = tracks * np.array([W2 / W, H2 / H], np.float32)
    for (h, w), tr in (((H, W), tracks), ((H2, W2), tr2)):
        counts, total = ref_point_id_counts(tr, h, w, idm, int(idm.max()))
        assert np.array_equal(total, oracle.tracks_to_masks(tr, h, w).reshape(T, -1).sum(1))
        _, allc = oracle.extract_mask_matches(tr, idm, h, w, (0, T - 1))
        assert len(allc) > 0
        for fid, oid, iou in allc:
            t, o = int(fid), int(oid)
            assert iou == (0.0 if total[t] == 0 else int(counts[t, o]) / int(total[t]))


def test_discriminating_pairs_discriminate():
    assert discriminating(14, 62).tolist() == [7]
    assert discriminating(21, 93).tolist() == [7, 14]
    n = sum(1 for o in range(1, 200) for i in range(1, 200) if len(discriminating(o, i)))
    assert n == 631
    for name, axes in DISCRIMINATING_AXES.items():
        for out, inp in axes:
            d = discriminating(out, inp)
            assert len(d) > 0, (name, out, inp)
            # CPU F.interpolate follows the float32 rule on them
            got = F.interpolate(torch.arange(inp).float()[None, None, :, None], size=(out, 1), mode="nearest")[0, 0, :, 0].numpy()
            assert np.array_equal(got.astype(np.int64), nearest_src_f32(out, inp))
    # every pair used before this file was blind to the difference
    for out, inp in ((47, 61), (83, 29)):
        assert len(discriminating(out, inp)) == 0
    rng = np.random.default_rng(0)
    for name, ((H, W), (Hi, Wi)) in RESIZE_CASES.items():
        tr = np.rint(edge_tracks(rng, 2, 700, H, W, Hi, Wi)[0])
        for y in discriminating(H, Hi):
            assert np.any((tr[:, 1] == y) & (tr[:, 0] >= 0) & (tr[:, 0] < W)), (name, "row", y)
        for x in discriminating(W, Wi):
            assert np.any((tr[:, 0] == x) & (tr[:, 1] >= 0) & (tr[:, 1] < H)), (name, "col", x)


def test_poisoned_tracks_hold_every_value_in_x_y_and_both():
    tr, keep = poisoned_tracks(np.random.default_rng(1), 2, 300, 50, 70)
    for t in range(2):
        bad = tr[t][~keep[t]]
        assert len(bad) == 3 * len(POISON)
        for v in POISON:
            same = (bad == v) | (np.isnan(bad) & np.isnan(v))
            assert (same[:, 0] & ~same[:, 1]).any() and (~same[:, 0] & same[:, 1]).any() and (same[:, 0] & same[:, 1]).any()
        assert np.isfinite(tr[t][keep[t]]).all() and np.abs(tr[t][keep[t]]).max() < 100
    c1, t1 = ref_point_id_counts(tr, 50, 70, np.ones((2, 50, 70), np.int64), 1)
    for t in range(2):
        c2, t2 = ref_point_id_counts(tr[t][keep[t]][None], 50, 70, np.ones((1, 50, 70), np.int64), 1)
        assert np.array_equal(c1[t], c2[0]) and t1[t] == t2[0]


# --------------------------------------------------------------------------------------------------------- keymask: colour palettes
IDSLOTS, IDMAX = 8192, 4096


def key_slot(key):
    return ((np.asarray(key, np.uint64) * np.uint64(2654435761)) & np.uint64(U32)) >> np.uint64(19)


@functools.lru_cache(None)
def _keys_by_slot():
    keys = np.arange(1, 1 << 24, dtype=np.uint64)
    slot = key_slot(keys).astype(np.int64)
    order = np.argsort(slot, kind="stable")
    return keys[order].astype(np.int64), np.searchsorted(slot[order], np.arange(IDSLOTS + 1))


def keys_of_slot(s):
    keys, start = _keys_by_slot()
    return keys[start[s]:start[s + 1]]


def palette(kind):
    """-> int64 keys (R << 16 | G << 8 | B), none black
    wrap       every colour hashes to slot 8190 or 8191: one cluster that wraps from 8191 to 0 and runs on for ~4090 slots
    spread     4096 colours in 4096 distinct slots (no probing at all)
    n4096 / n4097 / n8192 / n8193   that many random colours"""
    rng = np.random.default_rng(len(kind))
    if kind == "wrap":
        both = np.concatenate([keys_of_slot(8190), keys_of_slot(8191)])
        return rng.permutation(both)[:IDMAX]
    if kind == "spread":
        slots = rng.permutation(IDSLOTS)[:IDMAX]
        return np.array([keys_of_slot(s)[rng.integers(0, len(keys_of_slot(s)))] for s in slots], np.int64)
    n = int(kind[1:])
    return rng.permutation(np.unique(rng.integers(1, 1 << 24, 2 * n)))[:n].astype(np.int64)


def palette_frame(keys, H, W, seed=0, black=0.1):
    """u8 [H,W,3]: every key at least once (H * W >= len(keys)), in random order with repeats and some black"""
    rng = np.random.default_rng(seed)
    n = len(keys)
    assert H * W >= n
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, H * W - n)])
    k = keys[idx]
    k[n:][rng.random(H * W - n) < black] = 0
    k = k[rng.permutation(H * W)].reshape(H, W)
    return np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8)


def frame_keys(frame):
    f = frame.astype(np.int64)
    return (f[..., 0] << 16) | (f[..., 1] << 8) | f[..., 2]


@pytest.mark.parametrize("kind,n", [("wrap", 4096), ("spread", 4096), ("n4096", 4096), ("n4097", 4097), ("n8192", 8192), ("n8193", 8193)])
def test_palettes_are_what_they_claim(kind, n):
    keys = palette(kind)
    assert len(keys) == n == len(np.unique(keys)) and keys.min() > 0 and keys.max() < 1 << 24
    slots = key_slot(keys).astype(np.int64)
    if kind == "wrap":
        assert set(slots.tolist()) == {8190, 8191}
    if kind == "spread":
        assert len(np.unique(slots)) == n
    H, W = (96, 96) if n > 4608 else (72, 64)
    fr = palette_frame(keys, H, W)
    u = np.unique(frame_keys(fr))
    assert len(u[u != 0]) == n and (u == 0).any()


def test_slot_function_spreads_as_the_issue_says():
    _, start = _keys_by_slot()
    per = np.diff(start)
    assert per.sum() == (1 << 24) - 1 and 2040 <= per.min() and per.max() <= 2056          # about 2048 keys per slot
    assert len(keys_of_slot(8190)) + len(keys_of_slot(8191)) >= IDMAX


# -------------------------------------------------------------------------------------------------------------------- COCO RLE
def rle_fr_string(s):
    """maskApi.c rleFrString: -> list of counts as uint32 values.  A string that stops on a "more" character ends with the partial
    count (no sign extension), the delta still applied."""
    s = s.encode() if isinstance(s, str) else bytes(s)
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more and p < len(s):
            c = s[p] - 48
            x |= ((c & 0x1F) << (5 * k)) & U32
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= (-1 << (5 * k)) & U32
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & U32)
    return cnts


def _chars(x):
    out = bytearray()
    more = True
    while more:
        c = x & 0x1F
        x >>= 5
        more = (x != -1) if (c & 0x10) else (x != 0)
        if more:
            c |= 0x20
        out.append(c + 48)
    return bytes(out)


def rle_to_string(cnts):
    """maskApi.c rleToString"""
    return b"".join(_chars(int(x) - (int(cnts[i - 2]) if i > 2 else 0)) for i, x in enumerate(cnts))


def run_ends(cnts, hw):
    return np.minimum(np.cumsum(np.asarray(cnts, np.int64)), hw) if len(cnts) else np.zeros(0, np.int64)


def rle_decode_np(cnts, H, W):
    """rleDecode, sequentially: run j (value j & 1) fills its pixels in column-major order; ends clamp at H * W; the rest is 0"""
    flat = np.zeros(H * W, bool)
    pos = 0
    for j, c in enumerate(cnts):
        end = min(pos + int(c), H * W)
        if j & 1:
            flat[pos:end] = True
        pos = end
    return flat.reshape(W, H).T


def pack_words(m):
    """[H,W] bool -> uint32 words of the row-major bit plane (flat index i -> word i / 32, bit i % 32)"""
    flat = np.asarray(m, bool).reshape(-1)
    pad = (-flat.size) % 32
    return np.packbits(np.concatenate([flat, np.zeros(pad, bool)]), bitorder="little").view(np.uint32)


def decode_words_torch(cnts, H, W, device="cpu", chunk=1 << 25):
    """the words of pack_words(rle_decode_np(cnts, H, W)) as an int32 tensor, without a per-pixel array of the whole plane:
    row-major pixel i = (y, x) is column-major c = x * H + y, its run is the first whose end lies past c"""
    hw = H * W
    ends = torch.from_numpy(run_ends(cnts, hw)).to(device)
    nw = (hw + 31) // 32
    out = torch.empty(nw, dtype=torch.int32, device=device)
    sh = torch.arange(32, device=device, dtype=torch.int64)
    for w0 in range(0, nw, chunk // 32):
        w1 = min(nw, w0 + chunk // 32)
        i = torch.arange(w0 * 32, w1 * 32, device=device, dtype=torch.int64)
        y = torch.div(i, W, rounding_mode="floor")
        c = (i - y * W) * H + y
        j = torch.searchsorted(ends, c, right=True)
        v = ((j & 1) == 1) & (j < len(ends)) & (i < hw)
        out[w0:w1] = (v.view(-1, 32).to(torch.int64) << sh).sum(1).to(torch.int32)
    return out


def rle_to_bbox(counts, h, w):
    """pycocotools rleToBbox (maskApi.c) on the run counts, in numpy-free integer steps"""
    m = (len(counts) // 2) * 2
    if m == 0:
        return [0, 0, 0, 0]
    xs, ys, xe, ye, cc, xp = w, h, 0, 0, 0, 0
    for j in range(m):
        cc += counts[j]
        t = cc - j % 2
        y = t % h
        x = (t - y) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [xs, ys, xe - xs + 1, ye - ys + 1]


def mask_runs(m):
    """[H,W] -> run counts of the column-major scan, the first run of zeros"""
    flat = np.asarray(m, bool).T.reshape(-1)
    pos = np.flatnonzero(np.diff(np.concatenate([[False], flat]).astype(np.int8)))
    return np.diff(np.concatenate([[0], pos, [flat.size]])).tolist()


def count_spans(s):
    """-> [(first char, last char)] of every count of the string"""
    s = s.encode() if isinstance(s, str) else bytes(s)
    spans, a = [], 0
    for p, ch in enumerate(s):
        if not ((ch - 48) & 0x20) or p == len(s) - 1:
            spans.append((a, p))
            a = p + 1
    return spans


BIG = 46340                                   # 46340^2 = 2 147 395 600, just under 2^31


def _straddle_counts():
    """62 one-character counts, a 5-character count at chars 62..66, a 5-character negative delta at 68..72, one-character counts up
    to char 125, a 5-character count at 126..130 (across the second 64-character step), and the way back down"""
    c = [3, 2] * 31                                                    # m = 0..61
    c += [3 + (1 << 19) + 5, 4, 1]                                     # m = 62 (5 chars), 63, 64 (delta -(2^19 + 7): 5 chars)
    c += [2, 3] * 26 + [2]                                             # m = 65..117: chars 73..125
    c += [3 + (1 << 19) + 9, 2, 5, 1]                                  # m = 118 at 126..130; m = 120 comes back down
    return c


def _neg_after_step_counts():
    c = [5, 7] * 31 + [15, 7]                                          # m = 0..63, one character each: chars 0..63
    return c + [3, 7, 3]                                               # m = 64: delta 3 - 15 = -12, its only character is char 64


RLE_CASES = {
    # name: (H, W, counts or None, string or None)
    "straddle_62_66_and_126_130": (1031, 1033, _straddle_counts(), None),
    "negative_delta_after_step": (37, 53, _neg_after_step_counts(), None),
    "zero_runs_in_the_middle": (7, 33, [4, 3, 0, 5, 0, 0, 2, 9, 0, 1, 30], None),
    "first_count_zero": (7, 31, [0, 7, 2, 40, 11], None),
    "sum_past_hw": (7, 32, [3, 4, 50, 100, 100, 7], None),
    "uint_truncation": (7, 63, [3, 4, 5], b"34" + _chars(5) + _chars(2 - 4 - 4)),          # 4th count 4 - 6 = -2 -> 4294967294
    "empty_string": (7, 65, [], None),
    "cut_on_more": (7, 96, None, rle_to_string([5, 100, 3, 2000])[:-1]),
    "cut_on_more_first_char": (1, 160, None, rle_to_string([40])[:1]),
    "big_2p30_2p25": (BIG, BIG, [5, (1 << 30) + 7, 3, (1 << 25) + 11, 100, (1 << 25) + 5, 12345, 77], None),
    "big_first_zero": (BIG, BIG, [0, (1 << 25) + 1, (1 << 30) + 3, 999, (1 << 30) + 5, 77, 5], None),
}


def rle_case(name):
    """-> (H, W, string bytes)"""
    H, W, cnts, s = RLE_CASES[name]
    return H, W, (s if s is not None else rle_to_string(cnts))


def test_python_rle_equals_the_oracle_on_random_masks(oracle):
    rng = np.random.default_rng(3)
    for H, W, p in ((1, 1, 0.5), (5, 37, 0.5), (23, 41, 0.05), (64, 64, 0.9), (40, 70, 0.0), (40, 70, 1.0), (300, 200, 0.001)):
        m = rng.random((H, W)) < p
        rle, cnts = oracle.rle_encode(m)
        assert [int(c) for c in cnts] == mask_runs(m) and rle_to_string(cnts) == rle["counts"]
        assert rle_fr_string(rle["counts"]) == [int(c) for c in cnts]
        ref = oracle.rle_decode(rle).astype(bool)
        assert np.array_equal(ref, m) and np.array_equal(rle_decode_np(cnts, H, W), ref)
        assert np.array_equal(decode_words_torch(cnts, H, W, chunk=1 << 10).numpy().view(np.uint32), pack_words(ref))
        ys, xs = np.nonzero(m)
        want = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if m.any() else [0, 0, 0, 0]
        assert rle_to_bbox(cnts, H, W) == want


def test_rle_cases_have_their_named_properties():
    for name, (H, W, cnts, s) in RLE_CASES.items():
        _, _, st = rle_case(name)
        parsed = rle_fr_string(st)
        if cnts is not None:
            assert parsed[:len(cnts)] == cnts or name == "uint_truncation", name
        if H < BIG:                                                       # the torch decode agrees on everything small enough
            assert np.array_equal(decode_words_torch(parsed, H, W).numpy().view(np.uint32), pack_words(rle_decode_np(parsed, H, W))), name
    sp = count_spans(rle_case("straddle_62_66_and_126_130")[2])
    assert (62, 66) in sp and (126, 130) in sp and (68, 72) in sp
    assert sum(_straddle_counts()) <= 1031 * 1033
    _, _, st = rle_case("negative_delta_after_step")
    sp = count_spans(st)
    assert sp[64] == (64, 64) and (st[64] - 48) & 0x10 and rle_fr_string(st)[64] == 3 < rle_fr_string(st)[62]
    c = RLE_CASES["zero_runs_in_the_middle"][2]
    assert 0 in c[1:-1] and c[0] != 0
    assert RLE_CASES["first_count_zero"][2][0] == 0
    assert sum(RLE_CASES["sum_past_hw"][2]) > 7 * 32
    assert rle_fr_string(rle_case("uint_truncation")[2]) == [3, 4, 5, 4294967294]
    assert rle_case("empty_string")[2] == b"" and rle_fr_string(b"") == []
    for name in ("cut_on_more", "cut_on_more_first_char"):
        st = rle_case(name)[2]
        assert (st[-1] - 48) & 0x20
    assert rle_fr_string(rle_case("cut_on_more")[2]) == [5, 100, 3, (1900 & 0x3FF) + 100]      # two of the delta 1900's three characters
    assert rle_fr_string(rle_case("cut_on_more_first_char")[2]) == [40 & 0x1F]
    for name in ("big_2p30_2p25", "big_first_zero"):
        H, W, st = rle_case(name)
        c = rle_fr_string(st)
        assert H * W < 1 << 31 and (1 << 31) - H * W < 1 << 17
        lens = [b - a + 1 for a, b in count_spans(st)]
        assert any(v >= 1 << 30 for v in c) and any(1 << 25 <= v < 1 << 29 for v in c) and 6 in lens and 7 in lens
    assert sum(RLE_CASES["big_2p30_2p25"][2]) < BIG * BIG < sum(RLE_CASES["big_first_zero"][2])


# ------------------------------------------------------------------------------------------------------------------ K2: visibility
def ref_visibility(vis):
    """vis [T,Np] (any byte values; non-zero = visible) -> float32 [T]: count / Np rounded once.  The float64 quotient of two
    integers below 2^24 is never close enough to a float32 tie for the second rounding to matter (it misses one by at least
    2^-25 / Np relative, far above 2^-53)."""
    v = np.asarray(vis) != 0
    return np.array([np.float32(int(r.sum()) / v.shape[1]) for r in v], np.float32)


# ---------------------------------------------------------------------------------------------------------- K1: local correlation
def ref_local_corr(fmap, coords, support, r):
    """fmap f32 [T,H,W,C], coords f32 [T,Np,2] (x, y), support f32 [Np,S,C] -> (corr float64 [T,Np,S,S], bound float64 same shape)"""
    T, H, W, C = fmap.shape
    Np = coords.shape[1]
    D = 2 * r + 1
    S = D * D
    dy, dx = np.divmod(np.arange(S), D)
    dx, dy = (dx - r).astype(np.float32), (dy - r).astype(np.float32)
    f64, s64 = fmap.astype(np.float64), support.astype(np.float64)
    ref = np.zeros((T, Np, S, S))
    bound = np.zeros((T, Np, S, S))
    for t in range(T):
        x = coords[t, :, 0, None].astype(np.float32) + dx[None]                           # float32 sums [Np,S]
        y = coords[t, :, 1, None].astype(np.float32) + dy[None]
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0).astype(np.float64), (y - y0).astype(np.float64)
        nb, nba = np.zeros((Np, S, C)), np.zeros((Np, S, C))
        for ky in (0, 1):
            for kx in (0, 1):
                xx, yy = x0.astype(np.int64) + kx, y0.astype(np.int64) + ky
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                w = (fx if kx else 1 - fx) * (fy if ky else 1 - fy)
                v = f64[t, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * (ok * w)[..., None]
                nb += v
                nba += np.abs(v)
        ref[t] = np.einsum("nic,njc->nij", nb, s64)
        bound[t] = (C + 8) * 2.0 ** -24 * np.einsum("nic,njc->nij", nba, np.abs(s64))
    return ref, bound


K1_CASES = [(3, 128), (2, 128), (1, 64), (0, 32), (3, 4)]
K1_T, K1_H, K1_W, K1_NP = 2, 24, 40, 64


def k1_coords(r, seed=0):
    """f32 [T,Np,2] and the index sets of the named kinds: lattice points, every combination of x in {-1, 0, W-1, W} and y in
    {-1, 0, H-1, H}, +-r from each border, 50 px outside (output exactly 0), half pixels; the rest random"""
    H, W, Np, T = K1_H, K1_W, K1_NP, K1_T
    rng = np.random.default_rng(100 + r + seed)
    pts, kinds = [], {}

    def add(kind, p):
        kinds.setdefault(kind, []).extend(range(len(pts), len(pts) + len(p)))
        pts.extend(p)
    add("lattice", [(float(rng.integers(4, W - 4)), float(rng.integers(4, H - 4))) for _ in range(6)])
    add("border", [(float(x), float(y)) for x in (-1, 0, W - 1, W) for y in (-1, 0, H - 1, H)])
    add("r_from_border", [(float(x), 11.0) for x in (-r, r, W - 1 - r, W - 1 + r)] + [(17.0, float(y)) for y in (-r, r, H - 1 - r, H - 1 + r)])
    add("outside", [(-50.0, 10.0), (W + 50.0, 10.0), (20.0, -50.0), (20.0, H + 50.0), (-50.0, -50.0)])
    add("half", [(float(rng.integers(0, W - 1)) + 0.5, float(rng.integers(0, H - 1)) + 0.5) for _ in range(4)] + [(-0.5, 3.5), (W - 0.5, H - 0.5)])
    n = Np - len(pts)
    add("random", [(float(a), float(b)) for a, b in rng.random((n, 2)) * np.array([W + 6, H + 6]) - 3])
    base = np.array(pts, np.float32)
    co = np.stack([base, base[::-1].copy()])                                           # frame 1: the same points on other tracks
    kinds = {k: np.array(v) for k, v in kinds.items()}
    return co, kinds


def k1_inputs(r, C):
    rng = np.random.default_rng(1000 * r + C)
    fmap = rng.standard_normal((K1_T, K1_H, K1_W, C)).astype(np.float32)
    sup = rng.standard_normal((K1_NP, (2 * r + 1) ** 2, C)).astype(np.float32)
    co, kinds = k1_coords(r)
    return fmap, co, sup, kinds


@pytest.mark.parametrize("r,C", K1_CASES)
def test_k1_cases_and_reference(oracle, r, C):
    fmap, co, sup, kinds = k1_inputs(r, C)
    assert co.shape == (K1_T, K1_NP, 2) and sum(len(v) for v in kinds.values()) == K1_NP
    ref, bound = ref_local_corr(fmap, co, sup, r)
    out = kinds["outside"]
    assert not ref[0, out].any() and not bound[0, out].any()                            # exactly 0: no tap inside the map
    assert not ref[1, K1_NP - 1 - out].any()
    lat = co[0, kinds["lattice"]]
    assert np.array_equal(lat, np.rint(lat))
    b = co[0, kinds["border"]]
    assert set(b[:, 0].tolist()) == {-1.0, 0.0, K1_W - 1.0, float(K1_W)} and set(b[:, 1].tolist()) == {-1.0, 0.0, K1_H - 1.0, float(K1_H)}
    assert np.all(co[0, kinds["half"]] % 1 == 0.5)
    # a lattice point samples the map itself: one tap of weight 1
    n = kinds["lattice"][0]
    x, y = int(co[0, n, 0]), int(co[0, n, 1])
    centre = ((2 * r + 1) ** 2) // 2
    want = sup[n].astype(np.float64) @ fmap[0, y, x].astype(np.float64)
    np.testing.assert_allclose(ref[0, n, centre], want, rtol=1e-13, atol=1e-13)
    # the oracle's own float64 restatement agrees to its float32 output rounding; the bound is of the size of float32 chain error
    orc = oracle.local_correlation(fmap, co, sup, r)
    assert np.all(np.abs(orc - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-30)
    big = bound > 0
    assert bound.max() < 1e-4 * np.abs(ref).max() and big.mean() > 0.5            # tighter than the oracle test's 1e-4 * max|ref|
