"""Exact inputs for the point loss (csrc/loss.hip) and a float64 reference of loss_masks (criterion.py:292-356) on injected points.

Why exact inputs: the loss keeps the n_unc oversampled points with the smallest |logit|, and what happens among points whose key EQUALS
the threshold is a rule of this project (the reference's torch.topk leaves it open): ascending |x|, then ascending point index.  Smooth
random maps never produce two bit-equal keys, so no rule is exercised.  Here the logit map holds small integers and a coordinate is

    u = (j + 1/2 + f) / wm,  v = (i + 1/2 + g) / hm,   j, i pixel indices, f, g multiples of 1/den in [-1/2, 1/2), den in {2, 8}

so that x = ((2u - 1 + 1) wm - 1) / 2 = j + f, every bilinear weight and the sampled logit are exact in fp32 whatever the order of the
operations, and equal to the float64 value (wm, hm powers of two; the target planes are sampled exactly too: u * W is a short dyadic
number for any W).  The keys then tie massively and identically on the device and in float64, the selected set is fully determined by
the rule, and which tied points are taken changes the loss because their labels differ.

No GPU needed here; tests/test_point_loss_refs_cpu.py checks the properties that keep the GPU tests from passing vacuously."""
import numpy as np

# the GPU tolerances the cases are built for (tests/test_gpu_point_loss_ties.py)
LOSS_RTOL = 1e-5          # op-level summation-order bar of the point loss (tests/test_gpu_c4_oracle.py)
GRAD_REL = 2e-5           # max-norm relative bar of the point-loss gradient (tests/test_gpu_backward.py)


def sample_np(planes, coords, dtype=np.float64):
    """grid_sample(bilinear, zeros padding, align_corners=False) of planes [R,h,w] at coords [R,n,2] = (u, v) in [0,1], evaluated in
    `dtype` with the device's expression tree (csrc/loss.hip sample_plane) -> [R,n]"""
    R, h, w = planes.shape
    pl = planes.astype(dtype)
    u, v = coords[..., 0].astype(dtype), coords[..., 1].astype(dtype)
    one, half, two = dtype(1), dtype(0.5), dtype(2)
    x = ((two * u - one + one) * dtype(w) - one) * half
    y = ((two * v - one + one) * dtype(h) - one) * half
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = x - x0.astype(dtype), y - y0.astype(dtype)
    x1, y1 = x0 + 1, y0 + 1
    zero = dtype(0)
    wxa = np.where((x0 >= 0) & (x0 < w), one - fx, zero); wxb = np.where((x1 >= 0) & (x1 < w), fx, zero)
    wya = np.where((y0 >= 0) & (y0 < h), one - fy, zero); wyb = np.where((y1 >= 0) & (y1 < h), fy, zero)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)
    r = np.arange(R)[:, None]
    acc = pl[r, ya, xa] * (wxa * wya)
    acc = acc + pl[r, ya, xb] * (wxb * wya)
    acc = acc + pl[r, yb, xa] * (wxa * wyb)
    acc = acc + pl[r, yb, xb] * (wxb * wyb)
    assert acc.dtype == dtype
    return acc


def select_stats(src, cov, n_unc):
    """keys [R,n_over] (float64 |sampled logit|) and, per row: threshold key, points below it, points at it, how many of those are taken"""
    keys = np.abs(sample_np(src, cov, np.float64))
    thr = np.sort(keys, axis=1)[:, n_unc - 1]
    below = (keys < thr[:, None]).sum(1)
    ties = (keys == thr[:, None]).sum(1)
    return keys, thr, below, ties, n_unc - below


def select_points(keys, n_unc, rule="low"):
    """indices [R,n_unc] of the kept oversampled points: ascending key, then ascending (rule 'low', the project's) or descending
    ('high', the reversed rule the tests must tell apart) point index"""
    idx = np.broadcast_to(np.arange(keys.shape[1]), keys.shape)
    order = np.lexsort((idx if rule == "low" else -idx, keys), axis=-1)
    return np.sort(order[:, :n_unc], axis=1)


def loss_masks_ref(src, tt, cov, crd, n_unc, num_masks, w_mask=5.0, w_dice=5.0, rule="low"):
    """float64 loss_masks on R rows: src [R,hm,wm] logit maps, tt [R,H,W] target planes, cov [R,n_over,2] oversampled and crd [R,n_rand,2]
    extra points -> (loss_mask, loss_dice, d(w_mask loss_mask + w_dice loss_dice)/d src [R,hm,wm]) by autograd through grid_sample"""
    import torch
    import torch.nn.functional as F
    keys = np.abs(sample_np(src, cov, np.float64))
    sel = select_points(keys, n_unc, rule)
    coords = np.concatenate([np.take_along_axis(cov.astype(np.float64), sel[..., None], 1), crd.astype(np.float64)], 1)
    ps = lambda inp, c: F.grid_sample(inp[:, None], 2.0 * c[:, :, None, :] - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0, :, 0]
    s = torch.tensor(np.asarray(src, np.float64), requires_grad=True)
    c = torch.tensor(coords)
    with torch.no_grad():
        labels = ps(torch.tensor(np.asarray(tt, np.float64)), c)
    lg = ps(s, c)
    loss_mask = F.binary_cross_entropy_with_logits(lg, labels, reduction="none").mean(1).sum() / num_masks
    sg = lg.sigmoid()
    loss_dice = (1 - (2 * (sg * labels).sum(-1) + 1) / (sg.sum(-1) + labels.sum(-1) + 1)).sum() / num_masks
    (w_mask * loss_mask + w_dice * loss_dice).backward()
    return float(loss_mask.detach()), float(loss_dice.detach()), s.grad.numpy()


def rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def rule_spread(case, w_mask=5.0, w_dice=5.0):
    """how far the reversed tie rule moves the result: (max relative difference of loss_mask / loss_dice, max-norm relative difference
    of the gradient)"""
    a = loss_masks_ref(case["src"], case["tt"], case["cov"], case["crd"], case["n_unc"], case["num_masks"], w_mask, w_dice, "low")
    b = loss_masks_ref(case["src"], case["tt"], case["cov"], case["crd"], case["n_unc"], case["num_masks"], w_mask, w_dice, "high")
    return max(abs(a[0] - b[0]) / abs(a[0]), abs(a[1] - b[1]) / abs(a[1])), rel(b[2], a[2])


# ---------------------------------------------------------------------------------------------------------------- generators
def block_targets(rng, n, H, W, cells=(8, 16)):
    """n binary [H,W] planes: a random cells[0] x cells[1] bit pattern (about half set, never empty) enlarged to (H, W)"""
    out = np.zeros((n, H, W), np.uint8)
    yy, xx = np.arange(H) * cells[0] // H, np.arange(W) * cells[1] // W
    for i in range(n):
        bits = rng.integers(0, 2, cells).astype(np.uint8)
        bits[rng.integers(0, cells[0]), rng.integers(0, cells[1])] = 1
        out[i] = bits[yy][:, xx]
    return out


def dyadic_coords(rng, R, n, hm, wm, den):
    """[R,n,2] float32 coordinates (u, v) whose map position is pixel + k/den, k/den in [-1/2, 1/2): exact in fp32"""
    j, i = rng.integers(0, wm, (R, n)), rng.integers(0, hm, (R, n))
    f, g = rng.integers(-(den // 2), den - den // 2, (R, n)) / den, rng.integers(-(den // 2), den - den // 2, (R, n)) / den
    uv = np.stack([(j + 0.5 + f) / wm, (i + 0.5 + g) / hm], -1)
    out = uv.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), uv)
    return out


# name: map (hm, wm), target planes (H, W), P, integer logit values, fraction denominator, seed, then what the case must show:
# `ties` = (lo, hi) bounds on every row's number of points at the threshold, `take` one of 'inner' (0 < take < ties), 'one', 'all',
# 'n_unc' (threshold key 0: nothing below), `force` = 'one' / 'all': coordinates rewritten so that take = 1 / take = ties
_V3 = (-3, -2, -1, 0, 1, 2, 3)
_V1 = (-1, 0, 1)
_V2 = (-2, -1, 1, 2)
CASES = {
    # A: the list path (<= 512 ties), one map part, streamed
    "A_p256": dict(map=(16, 32), tgt=(64, 128), P=256, vals=_V3, den=8, seed=2, ties=(2, 512), take="inner"),
    "A_p1024": dict(map=(16, 32), tgt=(64, 128), P=1024, vals=_V3, den=8, seed=1, ties=(2, 512), take="inner"),
    "A_take1": dict(map=(16, 32), tgt=(64, 128), P=256, vals=_V3, den=8, seed=1, ties=(2, 512), take="one", force="one"),
    "A_takeall": dict(map=(16, 32), tgt=(64, 128), P=256, vals=_V3, den=8, seed=2, ties=(2, 512), take="all", force="all"),
    # B: the block-scan path (> 512 ties)
    "B_zero": dict(map=(16, 32), tgt=(64, 128), P=4096, vals=_V1, den=2, seed=3, ties=(513, 1 << 30), take="n_unc"),
    "B_above": dict(map=(16, 32), tgt=(64, 128), P=4096, vals=_V2, den=2, seed=2, ties=(513, 1 << 30), take="inner"),
    # C: two map parts (128 x 256: part_geom gives 117 rows per part)
    "C_list": dict(map=(128, 256), tgt=(256, 512), P=2048, vals=_V3, den=8, seed=3, ties=(2, 512), take="inner", parts=True),
    "C_scan": dict(map=(128, 256), tgt=(256, 512), P=4096, vals=_V1, den=2, seed=2, ties=(513, 1 << 30), take="n_unc", parts=True),
    # E: the recompute path (3P or P/4 not a multiple of 4, or H*W not a multiple of 32): forward only
    "E_p250": dict(map=(16, 32), tgt=(64, 128), P=250, vals=_V3, den=8, seed=1, ties=(2, 512), take="inner"),
    "E_p1026": dict(map=(16, 32), tgt=(64, 128), P=1026, vals=_V3, den=8, seed=2, ties=(2, 512), take="inner"),
    "E_scan_p1026": dict(map=(16, 32), tgt=(64, 128), P=1026, vals=_V1, den=2, seed=1, ties=(513, 1 << 30), take="n_unc"),
    "E_scan_above_p1026": dict(map=(16, 32), tgt=(64, 128), P=1026, vals=_V2, den=2, seed=3, ties=(513, 1 << 30), take="inner"),
    "E_hw": dict(map=(16, 32), tgt=(60, 124), P=256, vals=_V3, den=8, seed=2, ties=(2, 512), take="inner"),
}
PART_ROWS = 117           # part_geom(128, 256): 124 * 1024 / ((256 + 8) * 4) - 3


def _force_take(src, cov, n_unc, mode):
    """rewrite a few oversampled coordinates of every row so that exactly one tied point is taken ('one': points above the threshold
    become copies of a point below it) or all of them ('all': the surplus tied points become copies of a point above it)"""
    keys, thr, below, ties, take = select_stats(src, cov, n_unc)
    cov = cov.copy()
    for r in range(cov.shape[0]):
        lo, at, hi = (np.flatnonzero(c) for c in (keys[r] < thr[r], keys[r] == thr[r], keys[r] > thr[r]))
        if mode == "one":
            cov[r, hi[len(hi) - (take[r] - 1):]] = cov[r, lo[0]]
        else:                                                              # every other tie goes first: the survivors are not an index prefix
            cov[r, np.concatenate([at[1::2], at[0::2][::-1]])[:ties[r] - take[r]]] = cov[r, hi[0]]
    return cov


def exact_case(name, R=4):
    """the named case as reference-side arrays: src [R,hm,wm] f32 integer logit maps, tt [R,H,W] u8 planes, cov / crd f32 points"""
    c = dict(CASES[name])
    (hm, wm), (H, W), P = c["map"], c["tgt"], c["P"]
    rng = np.random.default_rng([c["seed"], hm, P])
    n_over, n_unc = int(P * 3.0), int(0.75 * P)
    src = rng.choice(np.array(c["vals"], np.float32), (R, hm, wm))
    tt = block_targets(rng, R, H, W)
    cov = dyadic_coords(rng, R, n_over, hm, wm, c["den"])
    crd = dyadic_coords(rng, R, P - n_unc, hm, wm, c["den"])
    if c.get("force"):
        cov = _force_take(src, cov, n_unc, c["force"])
    c.update(name=name, src=src, tt=tt, cov=cov, crd=crd, n_over=n_over, n_unc=n_unc, n_rand=P - n_unc, num_masks=2.0, P=P)
    return c


def check_structure(c):
    """the ties / take a case promises, on every row; returns (ties, take) per row"""
    keys, thr, below, ties, take = select_stats(c["src"], c["cov"], c["n_unc"])
    lo, hi = c["ties"]
    assert ((ties >= lo) & (ties <= hi)).all(), (c["name"], ties)
    if c["take"] == "inner":
        assert ((take > 0) & (take < ties)).all() and (thr > 0).all() and (below > 0).all(), (c["name"], take, ties, thr)
    elif c["take"] == "one":
        assert (take == 1).all() and (ties > 1).all(), (c["name"], take, ties)
    elif c["take"] == "all":
        assert (take == ties).all() and (below > 0).all(), (c["name"], take, ties)
    else:
        assert (thr == 0).all() and (below == 0).all() and (take == c["n_unc"]).all() and (ties > take).all(), (c["name"], thr, take, ties)
    if c.get("parts"):
        y0 = np.floor(c["cov"][..., 1].astype(np.float64) * c["map"][0] - 0.5)
        for r in range(keys.shape[0]):
            t = keys[r] == thr[r]
            assert (t & (y0[r] < PART_ROWS)).sum() >= 2 and (t & (y0[r] >= PART_ROWS)).sum() >= 2, (c["name"], r)
    return ties, take


def op_inputs(c, Q=4, T=2):
    """the case in the layout ops.point_loss takes (B = 1, Q queries of which two are matched, T = 2 frames: rows = (pair, frame)):
    mask logits [1, 1, T*hm*wm, Q] pixel-major, targets [1, 2, T, H, W], idx_q / idx_t [1, 2], n_match [1], coords [1, 4, n, 2]"""
    (hm, wm), (H, W) = c["map"], c["tgt"]
    rng = np.random.default_rng(c["seed"] + 1000)
    iq, it = np.array([[1, 3]], np.int32), np.array([[1, 0]], np.int32)
    masks = rng.choice(np.array(c["vals"], np.float32), (Q, T, hm, wm))
    tgt = np.zeros((1, 2, T, H, W), np.uint8)
    for s in range(2):
        for t in range(T):
            masks[iq[0, s], t] = c["src"][s * T + t]
            tgt[0, it[0, s], t] = c["tt"][s * T + t]
    ml = np.ascontiguousarray(masks.reshape(Q, T * hm * wm).T)[None, None]
    return dict(ml=ml, tgt=tgt, cnt=np.array([2], np.int32), iq=iq, it=it, nm=np.array([2], np.int32), dims=(Q, T, hm, wm),
                cov=c["cov"][None], crd=c["crd"][None])


# ---------------------------------------------------------------------------------------------------------------- case F
F_DIMS = dict(NL=10, B=2, Q=32, T=8, map=(16, 32), tgt=(64, 128), P=64)


def many_rows_case(kind, seed=5):
    """more than 4096 active rows in one call: NL = 10 layers with the same logits, B = 2 clips, Q = Nmax = 32 all matched, T = 8 ->
    512 rows per layer, 5120 in all (4096 streamed, 1024 recomputed).  kind 'smooth': smooth random maps and uniform random points;
    'ties': exact integer maps and dyadic points, the oversampled points of a row ordered label 1 first so that the rule moves every
    row's loss the same way (over 512 rows a random sign would average out)."""
    from s2d_amd.utils import synth
    d = F_DIMS
    (hm, wm), (H, W), P, B, Q, T = d["map"], d["tgt"], d["P"], d["B"], d["Q"], d["T"]
    R = B * Q * T
    rng = np.random.default_rng([seed, 77])
    n_over, n_unc = 3 * P, int(0.75 * P)
    tt = block_targets(rng, R, H, W)
    if kind == "smooth":
        src = synth.smooth_logits(seed, 2, (R,), (hm, wm)).astype(np.float32)
        cov = rng.random((R, n_over, 2), dtype=np.float32)
        crd = rng.random((R, P - n_unc, 2), dtype=np.float32)
    else:
        src = rng.choice(np.array(_V1, np.float32), (R, hm, wm))
        cov = dyadic_coords(rng, R, n_over, hm, wm, 2)
        crd = dyadic_coords(rng, R, P - n_unc, hm, wm, 2)
        lab = sample_np(tt.astype(np.float64), cov)
        cov = np.take_along_axis(cov, np.argsort(-lab, axis=1, kind="stable")[..., None], 1)
    # rows in the reference's order (clip, slot, frame); slot s of clip b: query iq[b, s], target it[b, s]
    iq = np.stack([rng.permutation(Q) for _ in range(B)]).astype(np.int32)
    it = np.stack([rng.permutation(Q) for _ in range(B)]).astype(np.int32)
    masks = np.zeros((B, Q, T, hm, wm), np.float32)
    tgt = np.zeros((B, Q, T, H, W), np.uint8)
    for b in range(B):
        for s in range(Q):
            for t in range(T):
                r = (b * Q + s) * T + t
                masks[b, iq[b, s], t] = src[r]
                tgt[b, it[b, s], t] = tt[r]
    ml1 = np.ascontiguousarray(np.moveaxis(masks.reshape(B, Q, T * hm * wm), 1, 2))               # [B, T*hm*wm, Q]
    NL = d["NL"]
    return dict(name="F_" + kind, src=src, tt=tt, cov=cov, crd=crd, n_over=n_over, n_unc=n_unc, n_rand=P - n_unc, P=P,
                num_masks=float(B * Q), map=(hm, wm), tgt=(H, W),
                op=dict(ml=np.ascontiguousarray(np.broadcast_to(ml1, (NL,) + ml1.shape)), tgt=tgt, cnt=np.full((B,), Q, np.int32),
                        iq=np.ascontiguousarray(np.tile(iq, (NL, 1))), it=np.ascontiguousarray(np.tile(it, (NL, 1))),
                        nm=np.full((NL * B,), Q, np.int32), dims=(Q, T, hm, wm),
                        cov=np.ascontiguousarray(np.broadcast_to(cov, (NL,) + cov.shape)),
                        crd=np.ascontiguousarray(np.broadcast_to(crd, (NL,) + crd.shape))))


# ---------------------------------------------------------------------------------------------------------------- case G
G_PLACEMENTS = ("centre", "corner", "block")
G_WEIGHTS = ((5.0, 5.0), (5.0 * 2 ** 20, 5.0 * 2 ** 20), (5.0 * 2 ** -20, 5.0 * 2 ** -20), (1e4, 0.0), (0.0, 1e4))


def cluster_case(placement, P=1024, seed=9):
    """every point of a row (oversampled and extra) on one pixel centre, on one four-tap corner (f = g = 1/2), or inside one 2 x 2 pixel
    block: up to P taps land on one pixel of the gradient plane (the int32 fixed-point tile and its provable cap, loss.hip FX_CAP)"""
    c = dict(map=(16, 32), tgt=(64, 128), P=P, vals=_V3, den=8, seed=seed)
    hm, wm = c["map"]
    R = 4
    rng = np.random.default_rng([seed, 31])
    n_over, n_unc = 3 * P, int(0.75 * P)
    src = rng.choice(np.array(_V3, np.float32), (R, hm, wm))
    tt = block_targets(rng, R, *c["tgt"])
    j0, i0 = rng.integers(2, wm - 3, (R, 1)), rng.integers(2, hm - 3, (R, 1))

    def pts(n):
        if placement == "centre":
            f = g = np.zeros((R, n))
        elif placement == "corner":
            f = g = np.full((R, n), 0.5)
        else:
            f, g = rng.integers(0, 8, (R, n)) / 8, rng.integers(0, 8, (R, n)) / 8
        uv = np.stack([(j0 + 0.5 + f) / wm, (i0 + 0.5 + g) / hm], -1)
        out = uv.astype(np.float32)
        assert np.array_equal(out.astype(np.float64), uv)
        return out
    c.update(name="G_" + placement, src=src, tt=tt, cov=pts(n_over), crd=pts(P - n_unc), n_over=n_over, n_unc=n_unc, n_rand=P - n_unc,
             num_masks=2.0, hot=(i0[:, 0], j0[:, 0]))
    return c
