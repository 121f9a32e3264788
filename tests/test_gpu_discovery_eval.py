"""The keymask kernels (csrc/keymask.hip) and the YTVIS-evaluator kernels (csrc/ytvis_eval.hip) against the independent references
of tests/test_discovery_refs_cpu.py, at the smallest shapes that reach each path and at the sizes the drivers run.  Every comparison
is exact array equality over every element, except K1 (element-wise |got - float64| <= the derived bound).  Lines starting with
`discrow` are the figures kept in profiles/discovery_eval_parity.txt."""
import numpy as np
import pytest
import torch

from tests.test_discovery_refs_cpu import (BIG, K1_CASES, RESIZE_CASES, RLE_CASES, decode_words_torch, discriminating, edge_tracks,
                                           frame_keys, k1_inputs, mask_runs, pack_words, palette, palette_frame, poisoned_tracks,
                                           ref_local_corr, ref_point_id_counts, ref_visibility, rle_case, rle_decode_np,
                                           rle_fr_string, rle_to_bbox, rle_to_string, run_ends)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _both_paths(tr, H, W, idmap):
    """-> [(name, counts, total)] of the fused kernel and of scatter + histogram, as numpy"""
    from s2d_amd.keymask import point_id_counts, point_id_counts_from_tracks, pred_tracks_to_binary_masks
    trd = torch.from_numpy(tr).to(DEV)
    c1, t1 = point_id_counts_from_tracks(trd, H, W, idmap)
    c2, t2 = point_id_counts(pred_tracks_to_binary_masks(trd[None], H, W)[0], idmap)
    return [("fused", c1.cpu().numpy(), t1.cpu().numpy()), ("two-launch", c2.cpu().numpy(), t2.cpu().numpy())]


def _check_counts(tr, H, W, ids, max_id, tag):
    from s2d_amd.keymask import IdMap
    want_c, want_t = ref_point_id_counts(tr, H, W, ids, max_id)
    for name, c, t in _both_paths(tr, H, W, IdMap(torch.from_numpy(ids), max_id=max_id)):
        assert np.array_equal(t, want_t), (tag, name)
        assert np.array_equal(c, want_c), (tag, name)
    return want_c, want_t


# ------------------------------------------------------------------------------------------------------------------ keymask: counts
@pytest.mark.parametrize("case", list(RESIZE_CASES))
def test_counts_vs_interpolate_reference(case):
    """both count paths on frame / id-map pairs where floorf(y * (float)Hi / H) and y * Hi // H differ, with points on every such
    row and column, ids outside 0..max_id (counted in `total` only) and random ids per pixel (adjacent source rows differ)"""
    (H, W), (Hi, Wi) = RESIZE_CASES[case]
    rng = np.random.default_rng(len(case))
    T, P, max_id = 2, 700, 8
    ids = rng.integers(-2, 12, (T, Hi, Wi))
    tr = edge_tracks(rng, T, P, H, W, Hi, Wi)
    c, t = _check_counts(tr, H, W, ids, max_id, case)
    assert t.min() > 0 and (c.sum(1) < t).all()                        # some points sit on ids outside the table
    print(f"discrow counts {case}: frame {H}x{W} <- ids {Hi}x{Wi}, rows {discriminating(H, Hi).tolist()} cols "
          f"{discriminating(W, Wi).tolist()} differ between the float32 and the exact rule; totals {t.tolist()}: equal")


def test_counts_full_lds_32768_points_max_id_8190():
    """P = 32768 keys (128 KiB) beside the 8192-entry histogram (32 KiB): all 160 KiB of LDS"""
    rng = np.random.default_rng(7)
    (H, W), (Hi, Wi) = RESIZE_CASES["down_720_to_480"]
    T, P, max_id = 2, 32768, 8190
    ids = rng.integers(0, max_id + 3, (T, Hi, Wi))
    tr = edge_tracks(rng, T, P, H, W, Hi, Wi)
    tr[:, 2000:] = (rng.random((T, P - 2000, 2)) * np.array([W + 8, H + 8]) - 4).astype(np.float32)   # spread over the frame
    c, t = _check_counts(tr, H, W, ids, max_id, "full LDS")
    assert t.min() > 20000 and (c > 0).sum() > 6000
    print(f"discrow counts P=32768 max_id=8190 (163840 B of LDS): totals {t.tolist()}, {int((c > 0).sum())} non-zero bins: equal")


def test_counts_one_frame_one_pixel_and_empty():
    rng = np.random.default_rng(8)
    H, W = 21, 14
    ids = rng.integers(0, 6, (1, 93, 62))
    tr = edge_tracks(rng, 1, 300, H, W, 93, 62)                         # T = 1
    _check_counts(tr, H, W, ids, 5, "T=1")
    one = (np.array([5.0, 7.0], np.float32) + (rng.random((1, 500, 2)).astype(np.float32) - 0.5) * 0.8)   # all round to (5, 7)
    c, t = _check_counts(one, H, W, ids, 5, "one pixel")
    assert t.tolist() == [1] and c.sum() == 1
    outside = one + np.float32(100.0)
    c, t = _check_counts(outside, H, W, ids, 5, "no point inside")
    assert t.tolist() == [0] and c.sum() == 0


def test_non_finite_and_huge_points_are_dropped_on_both_paths():
    """NaN, +-inf, +-3e9, +-1e19, +-3.4e38 in x, in y and in both: every such point is dropped, by the fused kernel and by
    scatter_tracks_kernel (whose float -> long cast of such a value is undefined in C++)"""
    from s2d_amd.keymask import pred_tracks_to_binary_masks
    rng = np.random.default_rng(9)
    T, P, H, W = 2, 300, 50, 70
    ids = rng.integers(0, 5, (T, H, W))
    tr, keep = poisoned_tracks(rng, T, P, H, W)
    clean = [ref_point_id_counts(tr[t][keep[t]][None], H, W, ids[t:t + 1], 4) for t in range(T)]
    want_c = np.concatenate([c for c, _ in clean])
    want_t = np.concatenate([t for _, t in clean])
    full_c, full_t = ref_point_id_counts(tr, H, W, ids, 4)
    assert np.array_equal(full_c, want_c) and np.array_equal(full_t, want_t)
    mask = pred_tracks_to_binary_masks(torch.from_numpy(tr).to(DEV)[None], H, W)[0].cpu().numpy()
    want_mask = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        p = np.rint(tr[t][keep[t]]).astype(np.int64)
        ok = (p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H)
        want_mask[t, p[ok, 1], p[ok, 0]] = 1
    extra = np.argwhere(mask != want_mask)
    print(f"discrow non-finite: scatter path marks {len(extra)} pixels it should not" + (f", first (t, y, x) = {extra[:6].tolist()}" if len(extra) else ""))
    from s2d_amd.keymask import IdMap
    res = _both_paths(tr, H, W, IdMap(torch.from_numpy(ids), max_id=4))
    for name, c, t in res:
        print(f"discrow non-finite {name}: totals {t.tolist()} want {want_t.tolist()}")
    assert len(extra) == 0
    for name, c, t in res:
        assert np.array_equal(t, want_t) and np.array_equal(c, want_c), name


# ---------------------------------------------------------------------------------------------------------- keymask: colour -> ids
def _ids(frames):
    from s2d_amd.keymask import color_masks_to_ids
    return color_masks_to_ids(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)).cpu().numpy()


def _plain_frame(H, W, seed):
    return palette_frame(palette("n4096")[:37], H, W, seed=seed, black=0.5)


@pytest.mark.parametrize("kind", ["wrap", "spread", "n4096"])
def test_color_ids_4096_colours_accepted(oracle, kind):
    """wrap: every colour hashes to slot 8190 or 8191, one probe cluster running from 8190 over the end of the table to ~4094;
    spread: no probing; n4096: random.  The frame after it in the same call keeps its own table"""
    frames = np.stack([palette_frame(palette(kind), 72, 64, seed=1), _plain_frame(72, 64, 2)])
    got = _ids(frames)
    assert np.array_equal(got, oracle.color_masks_to_ids(frames))
    assert got[0].max() == 4096 and len(np.unique(got[0])) == 4097 and got[1].max() == 37
    order = np.argsort(frame_keys(frames[0]).reshape(-1), kind="stable")
    assert np.all(np.diff(got[0].reshape(-1)[order]) >= 0)               # ids ascend with the 24-bit key


@pytest.mark.parametrize("kind", ["n4097", "n8192", "n8193"])
def test_color_ids_too_many_colours_raise(kind):
    from s2d_amd.keymask import color_masks_to_ids
    fr = palette_frame(palette(kind), 96, 96, seed=3)[None]
    with pytest.raises(RuntimeError):
        color_masks_to_ids(torch.from_numpy(fr).to(DEV))


def test_color_ids_refused_frame_among_valid_ones_raises(oracle):
    from s2d_amd.keymask import color_masks_to_ids
    frames = np.stack([_plain_frame(96, 96, 4), palette_frame(palette("n4097"), 96, 96, seed=5), _plain_frame(96, 96, 6)])
    with pytest.raises(RuntimeError):
        color_masks_to_ids(torch.from_numpy(frames).to(DEV))
    ok = frames[[0, 2]]
    assert np.array_equal(_ids(ok), oracle.color_masks_to_ids(ok))


def test_color_ids_frame_shapes(oracle):
    """1080 x 1920: the collect grid at its cap of 256 slices of 8100 pixels (not a multiple of 256); 1 x 1; 1 x 4097; T = 0"""
    from s2d_amd.keymask import color_masks_to_ids
    rng = np.random.default_rng(10)
    keys = palette("n4096")[:300]
    lab = np.repeat(np.repeat(rng.integers(0, 300, (1080 // 8, 1920 // 8)), 8, 0), 8, 1)
    noisy = rng.random((1080, 1920)) < 0.05
    lab[noisy] = rng.integers(0, 300, int(noisy.sum()))
    k = keys[lab]
    k[rng.random((1080, 1920)) < 0.02] = 0
    k[-1, -3:] = palette("n4097")[-3:]                                  # colours seen only by the last thread of the last slice
    fr = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8)[None]
    assert (1080 * 1920 // 4096) > 256 and -(-1080 * 1920 // 256) % 256 != 0
    assert np.array_equal(_ids(fr), oracle.color_masks_to_ids(fr))
    for one in (np.zeros((1, 1, 1, 3), np.uint8), np.full((1, 1, 1, 3), 255, np.uint8)):
        assert np.array_equal(_ids(one), oracle.color_masks_to_ids(one))
    k = np.concatenate([[0], palette("n4096")])[rng.permutation(4097)].reshape(1, 4097)
    line = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8)[None]
    got = _ids(line)
    assert np.array_equal(got, oracle.color_masks_to_ids(line)) and got.max() == 4096
    empty = color_masks_to_ids(torch.zeros((0, 5, 7, 3), dtype=torch.uint8, device=DEV))
    assert tuple(empty.shape) == (0, 5, 7, 1) and empty.dtype == torch.int64


# ------------------------------------------------------------------------------------------------------- keymask: select, K2, presence
@pytest.mark.parametrize("H,W,T", [(37, 53, 3), (481, 853, 2), (480, 854, 2), (1440, 2560, 2)])
def test_select_masks_tail_path_and_second_trip(H, W, T):
    """HW % 8 != 0 takes the scalar path for every element; 1440 x 2560 is 3 686 400 pixels, past the 2 097 152 one trip of the
    grid-stride loop covers"""
    from s2d_amd.keymask import select_masks
    rng = np.random.default_rng(H)
    ids = rng.integers(0, 5, (T, H, W))
    ids[:, -1, -9:] = np.arange(9) % 5                                  # the last elements of the plane
    frames, objs = [T - 1, 0, -1, 0, 1 % T], [2, -1, 4, 77, 0]          # obj -1: every non-background id; 77: absent
    if H * W > 2 ** 21:
        frames, objs = frames[:3], objs[:3]                             # K = 3
    got = select_masks(torch.from_numpy(ids), frames, objs)
    want = np.stack([np.where(ids[f] != 0 if o < 0 else ids[f] == o, 255, 0).astype(np.uint8) for f, o in zip(frames, objs)])
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if len(objs) > 3:
        assert not got[3].any()
    assert select_masks(torch.from_numpy(ids), [], []).shape == (0, H, W)            # K = 0


@pytest.mark.parametrize("T", [1, 33])
@pytest.mark.parametrize("Np", [1, 63, 64, 255, 256, 257, 2500])
def test_visibility_curve_counts(Np, T):
    from s2d_amd.keymask import visibility_curve
    rng = np.random.default_rng(Np * 40 + T)
    mixed = rng.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), (T, Np))
    for vis in (np.ones((T, Np), np.uint8), np.zeros((T, Np), np.uint8), mixed, np.ones((T, Np), bool)):
        got = visibility_curve(torch.from_numpy(vis)[None]).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, ref_visibility(vis))
    assert np.array_equal(ref_visibility(np.ones((T, Np), np.uint8)), np.ones(T, np.float32))


def test_idmap_presence_edges():
    from s2d_amd.keymask import IdMap
    T, Hi, Wi = 3, 61, 29                                               # 1769 ids in 32 slices of 56: the last holds 33
    rng = np.random.default_rng(11)
    ids = rng.integers(-3, 40, (T, Hi, Wi))
    ids[0].reshape(-1)[-3:] = [8190, 8000, 41]                          # only in the last, partial slice
    ids[1].reshape(-1)[-1] = 8191                                       # above max_id
    ids[2] = -7
    im = IdMap(torch.from_numpy(ids), max_id=8190)
    want = np.zeros((T, 8191), np.uint8)
    for t in range(T):
        u = np.unique(ids[t])
        want[t, u[(u >= 0) & (u <= 8190)]] = 1
    assert np.array_equal(im.presence.cpu().numpy(), want)
    assert want[0, [41, 8000, 8190]].all() and not want[2].any()
    assert im.frame_object_ids(0).tolist() == np.flatnonzero(want[0])[1:].tolist()
    with pytest.raises(RuntimeError):
        IdMap(torch.from_numpy(ids), max_id=8191)


# ---------------------------------------------------------------------------------------------------------- K1: local correlation
@pytest.mark.parametrize("r,C", K1_CASES)
def test_local_correlation_within_derived_bound(r, C):
    from s2d_amd.keymask import local_correlation
    fmap, co, sup, kinds = k1_inputs(r, C)
    ref, bound = ref_local_corr(fmap, co, sup, r)
    got = local_correlation(torch.from_numpy(fmap).to(DEV), torch.from_numpy(co).to(DEV), torch.from_numpy(sup).to(DEV), r).cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"discrow K1 r={r} C={C}: max err / bound {ratio.max():.4f}, max err {err.max():.3e}, max |ref| {np.abs(ref).max():.3e}, "
          f"{int((bound == 0).sum())} elements with bound 0 (all exactly 0: {not got[bound == 0].any()})")
    assert not got[0, kinds["outside"]].any()                             # 50 px outside: exactly 0
    assert np.all(err <= bound)


def test_local_correlation_refuses_what_it_cannot_stage():
    from s2d_amd.keymask import local_correlation
    for r, C in ((1, 6), (3, 256)):                                       # channels not in 16-B vectors; 104 000 B of LDS
        f = torch.zeros((1, 8, 8, C), device=DEV)
        with pytest.raises(RuntimeError):
            local_correlation(f, torch.zeros((1, 2, 2), device=DEV), torch.zeros((2, (2 * r + 1) ** 2, C), device=DEV), r)


# ------------------------------------------------------------------------------------------------------------ evaluator: RLE decode
def _blobs(rng, H, W, n=3):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.5, max(H, W) / 3 + 1)
        m ^= (yy - cy) ** 2 + ((xx - cx) * 0.7) ** 2 < r * r
    return m


def _seg(m, kind):
    c = mask_runs(m)
    if kind == "u":
        return {"size": list(m.shape), "counts": c}
    return {"size": list(m.shape), "counts": rle_to_string(c).decode()}


def _check_decode(segs, H, W, tag):
    """every plane and area of decode_frames against the sequential parse + decode"""
    from s2d_amd.ytvis_eval import decode_frames, plane_areas
    bits = decode_frames(segs, H, W, DEV)
    area = plane_areas(bits).cpu().numpy()
    got = bits.cpu().numpy().view(np.uint32)
    assert got.shape == (len(segs), (H * W + 31) // 32)
    for f, s in enumerate(segs):
        cnts = [] if s is None else (s["counts"] if isinstance(s["counts"], list) else rle_fr_string(s["counts"]))
        ref = rle_decode_np(cnts, H, W)
        assert np.array_equal(got[f], pack_words(ref)), (tag, f)
        assert area[f] == ref.sum(), (tag, f)


@pytest.mark.parametrize("name", [n for n in RLE_CASES if RLE_CASES[n][0] < BIG])
def test_decode_built_strings(name):
    H, W, st = rle_case(name)
    _check_decode([{"size": [H, W], "counts": st}], H, W, name)
    # the same string beside others: its wave's lane in a block of four strings
    m = _blobs(np.random.default_rng(1), H, W)
    _check_decode([_seg(m, "c"), {"size": [H, W], "counts": st.decode()}, None, _seg(m, "u"), {"size": [H, W], "counts": st}], H, W, name)


@pytest.mark.parametrize("F", [1, 2, 3, 5, 7, 9])
def test_decode_mixed_batches(F):
    """compressed, uncompressed and absent frames in batches that do not fill the parse kernel's four waves: frames whose runs
    are already in place (nrun >= 0) stay as they are"""
    H, W = 37, 53
    rng = np.random.default_rng(F)
    kinds = ["c", "u", None, "c", "u", "c", None, "u", "c"][:F]
    masks = [_blobs(rng, H, W) if k % 2 else rng.random((H, W)) < 0.4 for k in range(F)]
    _check_decode([None if k is None else _seg(m, k) for k, m in zip(kinds, masks)], H, W, F)
    _check_decode([None if k is None else _seg(m, k) for k, m in zip(kinds[::-1], masks)], H, W, -F)


@pytest.mark.parametrize("H", [1, 7])
@pytest.mark.parametrize("W", [31, 32, 33, 63, 65, 96, 160])
def test_decode_widths(H, W):
    """W % 64 == 32 aligned (the nb <= 32 arm), widths in 33..63, one word more than a wave's columns"""
    rng = np.random.default_rng(H * 1000 + W)
    masks = [_blobs(rng, H, W), rng.random((H, W)) < 0.5, np.ones((H, W), bool), np.zeros((H, W), bool)]
    masks[3][:, -1] = True
    masks.append(~masks[3])
    _check_decode([_seg(m, "c" if k % 2 == 0 else "u") for k, m in enumerate(masks)], H, W, (H, W))


@pytest.mark.parametrize("H,W", [(480, 854), (720, 1278)])
def test_decode_project_sizes(H, W):
    rng = np.random.default_rng(W)
    m = _blobs(rng, H, W, 5) ^ (rng.random((H, W)) < 0.01)
    m[-1, -1] = True
    _check_decode([_seg(m, "c")], H, W, (H, W))


def test_decode_largest_frame():
    """[46340, 46340]: 2 147 395 600 pixels, 67 106 113 words (268 MB) per plane, counts of 2^25 and 2^30 (6 and 7 characters);
    the reference planes are decode_words_torch on the device (equal to the sequential decode: tests/test_discovery_refs_cpu.py)"""
    import time
    from s2d_amd.ytvis_eval import decode_frames, plane_areas
    names = [n for n in RLE_CASES if RLE_CASES[n][0] == BIG]
    segs = [{"size": [BIG, BIG], "counts": rle_case(n)[2]} for n in names]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bits = decode_frames(segs, BIG, BIG, DEV)
    area = plane_areas(bits).cpu().numpy()
    t1 = time.perf_counter()
    for f, n in enumerate(names):
        cnts = rle_fr_string(rle_case(n)[2])
        ref = decode_words_torch(cnts, BIG, BIG, device=DEV)
        assert torch.equal(bits[f], ref), n
        e = np.concatenate([[0], run_ends(cnts, BIG * BIG)])
        assert int(area[f]) == int(np.diff(e)[1::2].sum()), n
        del ref
    print(f"discrow decode largest frame: [{BIG}, {BIG}] used, {bits.shape[1]} words per plane, {len(names)} planes; decode + areas "
          f"{t1 - t0:.2f} s, areas {area.tolist()}")


# -------------------------------------------------------------------------------------------------------- evaluator: bbox and areas
def _upload(planes):
    return torch.from_numpy(np.stack([pack_words(p) for p in planes]).view(np.int32)).to(DEV)


@pytest.mark.parametrize("H,W", [(720, 1280), (480, 854), (481, 853), (100, 3)])
def test_plane_bboxes_and_areas_past_256_words(H, W):
    """more than 256 words per plane (the w += 256 loop of one workgroup per plane); 481 x 853 ends in a partial word; W = 3: a word
    spans 11 rows"""
    from s2d_amd.ytvis_eval import plane_areas, plane_bboxes
    rng = np.random.default_rng(H + W)
    planes = []
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        p = np.zeros((H, W), bool); p[y, x] = True; planes.append(p)
    p = np.zeros((H, W), bool); p.reshape(-1)[(H * W - 1) // 32 * 32] = True; planes.append(p)      # first bit of the last word
    planes += [np.ones((H, W), bool), np.zeros((H, W), bool)]
    p = np.zeros((H, W), bool); p[H // 3, W // 2] = True; p[H - 2, W // 3] = True; planes.append(p)
    planes += [_blobs(rng, H, W, 2), rng.random((H, W)) < 0.001]
    bits = _upload(planes)
    assert bits.shape[1] > 256 or W == 3
    want = [rle_to_bbox(mask_runs(p), H, W) for p in planes]
    assert plane_bboxes(bits, H, W).cpu().tolist() == want
    assert plane_areas(bits).cpu().tolist() == [int(p.sum()) for p in planes]


# --------------------------------------------------------------------------------------------------------- evaluator: cross counts
_LUT = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint8)


def _popcount(words):
    return int(_LUT[np.ascontiguousarray(words).view(np.uint16)].sum(dtype=np.int64))


def _pair_counts(a, b):
    return np.array([[_popcount(x & y) for y in b] for x in a], np.int64).reshape(len(a), len(b))


@pytest.mark.parametrize("D,G,words", [(9, 17, 12293), (1, 65, 300), (65, 1, 300), (3, 5, 1), (8, 8, 4097)])
def test_cross_counts_chunks_and_partial_tiles(D, G, words):
    """(9, 17) at 12 293 words: four chunks of 3074 words (not a multiple of 256) and partial 8 x 8 tiles on both sides"""
    from s2d_amd.ytvis_eval import cross_counts
    rng = np.random.default_rng(D * 100 + G)
    a = rng.integers(0, 1 << 32, (D, words), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, (G, words), dtype=np.uint64).astype(np.uint32)
    b[:, -1] |= 0x80000001                                               # the last word of the last chunk matters
    got = cross_counts(torch.from_numpy(a.view(np.int32)).to(DEV), torch.from_numpy(b.view(np.int32)).to(DEV)).cpu().numpy()
    assert np.array_equal(got, _pair_counts(a, b))


@pytest.fixture(scope="module")
def video_case():
    """D = 20 detections, G = 6 ground truths, 36 frames of 720p: planes drawn on the device, counted pair by pair on the host"""
    D, G, T, wpf = 20, 6, 36, 720 * 1280 // 32
    gen = torch.Generator(device=DEV).manual_seed(5)
    def draw(n):
        w = torch.randint(-2 ** 31, 2 ** 31, (n * T, wpf), device=DEV, dtype=torch.int64, generator=gen).to(torch.int32)
        w &= torch.randint(-2 ** 31, 2 ** 31, (n * T, wpf), device=DEV, dtype=torch.int64, generator=gen).to(torch.int32)
        w[::5] = 0                                                       # absent frames
        return w.contiguous()
    dt, gt = draw(D), draw(G)
    dh, gh = dt.cpu().numpy().view(np.uint32), gt.cpu().numpy().view(np.uint32)
    inter = _pair_counts(dh.reshape(D, -1), gh.reshape(G, -1))
    d_area = np.array([_popcount(p) for p in dh], np.int64).reshape(D, T)
    g_area = np.array([_popcount(p) for p in gh], np.int64).reshape(G, T)
    return dict(D=D, G=G, T=T, wpf=wpf, dt=dt, gt=gt, inter=inter, d_area=d_area, g_area=g_area)


def test_cross_counts_video_sized(video_case):
    from s2d_amd.ytvis_eval import cross_counts
    v = video_case
    got = cross_counts(v["dt"].view(v["D"], -1), v["gt"].view(v["G"], -1)).cpu().numpy()
    assert np.array_equal(got, v["inter"]) and v["inter"].min() > 0


def test_video_ious_are_the_integer_quotients(video_case):
    from s2d_amd.ytvis_eval import plane_areas, video_ious
    v = video_case
    ious, da = video_ious(v["dt"], v["D"], v["gt"], v["G"], v["T"])
    assert np.array_equal(da, v["d_area"]) and da.dtype == np.int64
    assert np.array_equal(plane_areas(v["gt"]).cpu().numpy().reshape(v["G"], v["T"]), v["g_area"])
    want = np.zeros((v["D"], v["G"]))
    for d in range(v["D"]):
        for g in range(v["G"]):
            i = int(v["inter"][d, g])
            u = int(v["d_area"][d].sum()) + int(v["g_area"][g].sum()) - i
            want[d, g] = i / u                                            # Python's correctly rounded integer quotient
    assert ious.dtype == np.float64 and np.array_equal(ious, want)
