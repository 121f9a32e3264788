"""Host references for the matcher cost kernels (s2d_amd/csrc/matcher.hip), numpy only.

cost64          the cost matrix with float64 contractions on the oracle's fp32 point samples, and the largest-term scale
matcher_points  the device point generator (mix64 / rand2 / gen_points_kernel) restated in uint64 numpy: exact float32 results
batch_census    cell_key_kernel, the stable sort, the partition into 32-point batches over CHM chunks and the span / staged rule of
                matcher_cost_f16_body::setup restated on the host: which path each batch of a point set takes
case builders   seeded inputs whose batches are built on purpose to take each path; every builder carries the census predicate it
                was built for, and tests/test_matcher_refs_cpu.py checks that predicate without a GPU

The census is a restatement, not an instrument in the kernel: it is used only on case points that lie at least 1e-3 of a cell away
from every cell edge (the builders place them at fractions 0.05 .. 0.95 of a cell), so that the last bit of the host's and the
device's fp32 cell arithmetic cannot put a point into different cells."""
import numpy as np

from s2d_amd.utils import synth

SB = 32            # points per batch
CHM = 16           # chunks (blocks) per (problem, frame): chunk c walks batches c, c + CHM, ...
SPANMAX = 24       # staged pixel rows per tap row
BOUND = 3e-5       # entry check: |C_dev - cost64| <= BOUND * (largest cost term); the looser of the two bounds already asserted for this kernel
WEIGHTS = (2.0, 5.0, 5.0)   # class, mask, dice
BORDER8 = np.array([[0, 0], [1, 1], [0, 1], [1, 0], [0.5, 0], [0, 0.5], [1, 0.5], [0.5, 1]], np.float32)


# ------------------------------------------------------------------------------------------------ cost in float64
def cost64(oracle, logits, masks, tgt, coords, wc, wm, wd):
    """matcher.py:236-287 on the oracle's fp32 point samples (point_features.py:19-42) with the contractions and the activation
    sums in float64: the value both fp32 implementations (the reference's einsum, the device's split-fp16 MFMA + double
    reduction) approximate.  logits [Q,C1], masks [Q,T,h,w], tgt [N,T,H,W] (any nonzero byte = set), coords [1,P,2].
    -> (C [Q,N] float64, the magnitude of the largest cost term)"""
    tgt = (np.asarray(tgt) != 0).astype(np.uint8)
    Q, N = masks.shape[0], tgt.shape[0]
    tm = oracle.point_sample(tgt, np.repeat(coords, N, 0)).reshape(N, -1).astype(np.float64)
    om = oracle.point_sample(masks.astype(np.float32), np.repeat(coords, Q, 0)).reshape(Q, -1).astype(np.float64)
    sp = np.maximum(om, 0) + np.log1p(np.exp(-np.abs(om)))
    cost_mask = (sp.sum(-1)[:, None] - om @ tm.T) / om.shape[1]
    with np.errstate(over="ignore"):                      # exp(-x) = inf for x < -709: sigmoid 0, which is its float64 value there
        sg = 1.0 / (1.0 + np.exp(-om))
    cost_dice = 1 - (2 * (sg @ tm.T) + 1) / (sg.sum(-1)[:, None] + tm.sum(-1)[None, :] + 1)
    l = logits.astype(np.float32)
    if l.shape[-1] > 2:                                   # class-aware heads: -softmax(l)[:, 0] over all C1 columns, in float64
        l = l.astype(np.float64)
    e = np.exp(l - l.max(-1, keepdims=True))
    cost_class = -np.repeat((e / e.sum(-1, keepdims=True))[:, :1].astype(np.float64), N, axis=1)
    # second value: the magnitude of the cost's terms (the sum itself can cancel to ~0: a random-init layer whose class, mask and
    # dice terms nearly offset has max|C| = 0.37 from terms of size 5 -- errors are measured against the terms)
    return wm * cost_mask + wc * cost_class + wd * cost_dice, float((abs(wm) * np.abs(cost_mask) + abs(wc) * np.abs(cost_class) + abs(wd) * np.abs(cost_dice)).max())


# ------------------------------------------------------------------------------------------------ the device point generator
_M64 = (1 << 64) - 1


def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def matcher_points(seed, nprob, P):
    """gen_points_kernel: point i of problem `prob` is rand2(seed, stream = prob, i) -- two uniforms in [0, 1) of 24 random bits
    each (bits 0..23 and 32..55 of one mix64 word) times 2^-24.  -> float32 [nprob, P, 2], bit for bit the device's."""
    with np.errstate(over="ignore"):
        stream = np.arange(nprob, dtype=np.uint64)[:, None]
        i = np.arange(P, dtype=np.uint64)[None, :]
        s = np.full((1, 1), int(seed) & _M64, np.uint64)
        r = _mix64(s ^ _mix64(stream * np.uint64(0xD1342543DE82EF95) + i))
    u = (r & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    v = ((r >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.stack([u, v], -1)


# ------------------------------------------------------------------------------------------------ which path a batch takes
def _taps(c, n):
    """upper-left tap index of normalised coordinates c on an axis of n pixels, in the device's fp32 steps (bil_setup)"""
    c = np.asarray(c, np.float32)
    g = np.float32(2) * c - np.float32(1)
    f = ((g + np.float32(1)) * np.float32(n) - np.float32(1)) * np.float32(0.5)
    return np.floor(f).astype(np.int64)


def edge_margin(coords, hm, wm):
    """smallest distance, in cells, of any point from a cell edge of the (hm, wm) map (float64)"""
    c = np.asarray(coords, np.float64).reshape(-1, 2)
    fx, fy = c[:, 0] * wm - 0.5, c[:, 1] * hm - 0.5
    d = np.minimum(np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy)))
    return float(d.min())


def batch_census(coords, hm, wm, P=None):
    """coords [nprob, P, 2] -> per problem: the batches of its cell-sorted points as the f16 kernels see them.
    dict of arrays [nprob]: staged, direct (batch counts), partial (1 if the last batch has fewer than 32 points), absent (chunks of
    the CHM that get no batch), and flags over the STAGED batches: left (a tap at x0 = -1), right (x1 = wm), top (y0 = -1), bottom
    (y1 = hm), row_cross (points of one batch in two map rows: its run crosses a row end), lower_past (the lower run reaches past
    the map's last pixel).  `batches`[prob] lists (kind 'S' / 'D', span, cmin, npoints) in batch order: chunk c owns entries c::CHM."""
    coords = np.asarray(coords, np.float32)
    nprob = coords.shape[0]
    P = coords.shape[1] if P is None else P
    keys = ("staged", "direct", "partial", "absent", "left", "right", "top", "bottom", "row_cross", "lower_past")
    out = {k: np.zeros(nprob, np.int64) for k in keys}
    out["batches"] = []
    npix = hm * wm
    for pr in range(nprob):
        x0, y0 = _taps(coords[pr, :P, 0], wm), _taps(coords[pr, :P, 1], hm)
        cell = np.clip(y0, 0, hm - 1) * wm + np.clip(x0, 0, wm - 1)
        order = np.argsort(cell, kind="stable")              # the radix sort of (problem * cells + cell, index) pairs is stable
        x0, y0, cell = x0[order], y0[order], cell[order]
        nb = (P + SB - 1) // SB
        lst = []
        for j in range(nb):
            sl = slice(j * SB, min((j + 1) * SB, P))
            cmin, cmax = int(cell[sl].min()), int(cell[sl].max())
            span = (cmax - cmin + 3) & ~1
            staged = span <= SPANMAX and span < wm
            lst.append(("S" if staged else "D", span, cmin, sl.stop - sl.start))
            out["staged" if staged else "direct"][pr] += 1
            if staged:
                out["left"][pr] |= int((x0[sl] == -1).any())
                out["right"][pr] |= int((x0[sl] == wm - 1).any())
                out["top"][pr] |= int((y0[sl] == -1).any())
                out["bottom"][pr] |= int((y0[sl] == hm - 1).any())
                out["row_cross"][pr] |= int(cmin // wm != cmax // wm)
                out["lower_past"][pr] |= int(cmin + wm + span > npix)
        out["partial"][pr] = int(P % SB != 0)
        out["absent"][pr] = max(0, CHM - nb)
        out["batches"].append(lst)
    return out


def census_line(cen, pr=0):
    kinds = "".join(b[0] for b in cen["batches"][pr])
    flags = ",".join(k for k in ("left", "right", "top", "bottom", "row_cross", "lower_past") if cen[k][pr])
    spans = sorted({(b[1], b[0]) for b in cen["batches"][pr]})
    return (f"staged {cen['staged'][pr]} direct {cen['direct'][pr]} partial {cen['partial'][pr]} absent-chunks {cen['absent'][pr]} "
            f"order {kinds} spans {' '.join(f'{s}{k}' for s, k in spans)} staged-flags [{flags}]")


# ------------------------------------------------------------------------------------------------ point sets by tap cell
def points_at(rng, taps, hm, wm):
    """taps: sequence of (y0, x0) upper-left tap indices, y0 in -1 .. hm-1, x0 in -1 .. wm-1 -> coords [P, 2] float32 inside [0, 1],
    each at a random fraction 0.05 .. 0.95 of its cell (0.55 .. 0.95 for a tap at -1, 0.05 .. 0.45 in the last cell, where the
    image ends half a cell in), then shuffled so that the device's sort has work to do."""
    t = np.asarray(taps, np.int64).reshape(-1, 2)
    out = np.empty((len(t), 2), np.float32)
    for ax, n in ((0, wm), (1, hm)):
        i0 = t[:, 1 - ax]
        lo = np.where(i0 == -1, 0.55, 0.05)
        hi = np.where(i0 == n - 1, 0.45, 0.95)
        f = lo + (hi - lo) * rng.random(len(t))
        out[:, ax] = ((i0 + 0.5 + f) / n).astype(np.float32)
    return out[rng.permutation(len(t))]


def taps_of_cells(rng, cells, hm, wm):
    """clamped cells (linear indices) -> tap indices: a point in column 0 / row 0 gets its tap at -1 (outside the map) half the time"""
    cells = np.asarray(cells, np.int64)
    y, x = cells // wm, cells % wm
    x = np.where((x == 0) & (rng.random(len(cells)) < 0.5), -1, x)
    y = np.where((y == 0) & (rng.random(len(cells)) < 0.5), -1, y)
    return np.stack([y, x], -1)


def _run(start, width, n=SB):
    """n points spread over the cells start .. start + width - 1, both end cells occupied"""
    return [start + (i * (width - 1)) // max(n - 1, 1) for i in range(n)] if width > 1 else [start] * n


def _expect(width, wm):
    span = (width + 2) & ~1
    return ("S" if span <= SPANMAX and span < wm else "D", span)


# Every pattern returns (cells in sorted order, predicate over (census, problem index)).  P is the length of the cell list.
def pat_one_cell(hm, wm):
    """the 1 x 1 map: span 2 >= wm, every batch direct; taps at -1 and 0 on both axes; 2 full batches + 5 points"""
    return [0] * 69, lambda c, p: c["staged"][p] == 0 and c["direct"][p] == 3 and c["partial"][p] == 1 and c["absent"][p] == 13


def pat_staged(hm, wm):
    """all batches staged as runs of at most 11 cells: uniform density over the whole map (so runs cross row ends, touch all four
    borders and reach the last row), more than CHM batches (chunks with two or three) and a partial last batch"""
    npix = hm * wm
    if wm <= 3:                                            # 2 x 3: a batch is staged only inside one cell (span 2 < 3)
        cells = [c for c in range(npix) for _ in range(2 * SB)] + [npix - 1] * 5
        return cells, lambda c, p: c["direct"][p] == 0 and c["staged"][p] == 13 and c["partial"][p] == 1 and all(
            c[k][p] for k in ("left", "right", "top", "bottom", "lower_past"))
    nb = max(CHM + 2, -(-npix // 7))
    P = nb * SB + 5
    cells = [(i * npix) // P for i in range(P)]
    return cells, lambda c, p: c["direct"][p] == 0 and c["staged"][p] == nb + 1 and c["partial"][p] == 1 and max(
        b[1] for b in c["batches"][p]) <= 12 and all(c[k][p] for k in ("left", "right", "top", "bottom", "row_cross", "lower_past"))


def pat_direct(hm, wm):
    """all batches direct: 16 points in each of an even number of cells 24 apart (span 26), so every 32 sorted points alternate
    between two far cells; on the 2 x 3 map 16 points per cell (two cells: span 4 >= wm)"""
    npix = hm * wm
    chain = list(range(0, npix, SPANMAX if npix > 6 else 1))
    chain = chain[:len(chain) & ~1]
    cells = [c for c in chain for _ in range(SB // 2)]
    n = len(chain) // 2
    return cells, lambda c, p: c["staged"][p] == 0 and c["direct"][p] == n and n >= 2 and c["partial"][p] == 0


def pat_mixed(hm, wm):
    """CHM + 3 batches, batches 0 and CHM + 2 direct (two cells 24 apart), the others staged runs of two cells: chunk 0 walks a direct
    batch and then a staged one (batches 0 and 16), chunk 2 a staged and then a direct one (batches 2 and 18), so the prefetch of
    the next batch's rows switches off and on inside a chunk"""
    npix = hm * wm
    if npix <= 6:
        cells = [(i * npix) // 100 for i in range(100)]     # batches that straddle two cells are direct, the others staged
        return cells, lambda c, p: c["staged"][p] >= 1 and c["direct"][p] >= 1
    cells, cur = [], 0
    for j in range(CHM + 3):
        if j in (0, CHM + 2):
            cells += [cur] * (SB // 2) + [cur + SPANMAX] * (SB // 2)
            cur += SPANMAX + 1
        else:
            cells += _run(cur, 2)
            cur += 2
    assert cur <= npix

    def pred(c, p):
        k = "".join(b[0] for b in c["batches"][p])
        return len(k) == CHM + 3 and k[0] != k[CHM] and k[2] != k[CHM + 2] and "S" in k and "D" in k
    return cells, pred


def pat_spans(hm, wm):
    """one batch per run width 18, 20, 22, 24 cells (span 20, 22, 24, 26), each starting in column 0 with taps at x0 = -1 in its
    first cell: both sides of span == wm (24-wide map), of span == SPANMAX and SPANMAX + 2 (26-wide map), of span < wm (21- and
    25-wide maps); then 5 points in the last cell"""
    npix = hm * wm
    cells, want, row = [], [], 0
    for w in (18, 20, 22, 24):
        cells += _run(row * wm, w)
        want.append(_expect(w, wm))
        row += -(-w // wm)
    assert cells[-1] < npix - 1
    cells += [npix - 1] * 5
    want.append(("S", 2))
    return cells, lambda c, p: [(b[0], b[1]) for b in c["batches"][p]] == want and c["left"][p] == 1


def pat_last_row(hm, wm):
    """points in the last map row only: y1 = hm on every point, every lower run past the last pixel"""
    cells = [(hm - 1) * wm + (i * wm) // (5 * SB + 7) for i in range(5 * SB + 7)]
    return cells, lambda c, p: c["direct"][p] == 0 and c["bottom"][p] == 1 and c["lower_past"][p] == 1 and c["top"][p] == 0


def pat_first_row(hm, wm):
    """points in the first map row with v < 0.5 / hm only: y0 = -1 on every point (forced by the builder)"""
    cells = [(i * wm) // (5 * SB + 7) for i in range(5 * SB + 7)]
    return cells, lambda c, p: c["direct"][p] == 0 and c["top"][p] == 1 and c["bottom"][p] == 0


def pat_columns(hm, wm):
    """points in the first and the last column only: 32 in cell (0, 0), then 16 in (y, wm-1) and 16 in (y+1, 0) per batch: staged
    runs of two cells that cross a row end, with a right tap at x1 = wm and a left tap at x0 = -1 in one batch"""
    cells = [0] * SB
    for y in range(hm - 1):
        cells += [y * wm + wm - 1] * (SB // 2) + [(y + 1) * wm] * (SB // 2)
    return cells, lambda c, p: c["direct"][p] == 0 and all(c[k][p] for k in ("left", "right", "row_cross")) and all(
        b[1] == 4 for b in c["batches"][p][1:])


PATH_MAPS = [(1, 1), (2, 3), (5, 24), (5, 25), (7, 26), (13, 21)]
PATTERNS = {"staged": pat_staged, "direct": pat_direct, "mixed": pat_mixed, "spans": pat_spans, "last_row": pat_last_row,
            "first_row": pat_first_row, "columns": pat_columns}


def path_case_ids():
    ids = [("one_cell", 1, 1)]
    for hm, wm in PATH_MAPS[1:]:
        for name in PATTERNS:
            if wm <= 3 and name in ("spans", "last_row", "first_row", "columns"):
                continue                                   # the 2 x 3 map has no room for them: its staged / direct / mixed sets touch every border
            ids.append((name, hm, wm))
    return ids


class Case:
    """inputs of one ops.matcher_cost call in the reference's layouts: masks [NL,B,Q,T,hm,wm], cls [NL,B,Q,2], tgt u8 [B,Nmax,T,H,W],
    cnt i32 [B], coords [NL,B,P,2]; `predicate(census, problem)` is what the point set was built for (None: not a census case)"""

    def __init__(self, name, masks, cls, tgt, cnt, coords, H, W, predicate=None, census=True):
        self.name, self.masks, self.cls, self.tgt, self.cnt, self.coords = name, masks, cls, tgt, cnt, coords
        self.NL, self.B, self.Q, self.T, self.hm, self.wm = masks.shape
        self.H, self.W, self.Nmax, self.P = H, W, tgt.shape[1], coords.shape[2]
        self.predicate, self.has_census = predicate, census

    def census(self):
        return batch_census(self.coords.reshape(self.NL * self.B, self.P, 2), self.hm, self.wm)

    def ok(self):
        cen = self.census()
        return all(self.predicate(cen, p) for p in range(self.NL * self.B))


def random_inputs(seed, NL, B, Q, T, hm, wm, H, W, counts, Nmax=None, amp=4.0, density=0.4):
    """white-noise logits and targets: every pixel differs from its neighbours, so a tap read one pixel off changes the sums"""
    masks = synth.randn(seed, 1, (NL, B, Q, T, hm, wm), amp)
    cls = synth.randn(seed, 2, (NL, B, Q, 2))
    Nmax = Nmax or max(max(counts), 1)
    tgt = (synth.rng_for(seed, 3).random((B, Nmax, T, H, W)) < density).astype(np.uint8)
    return masks, cls, tgt, np.asarray(counts, np.int32)


def path_case(name, hm, wm, Q, seed=0, border=False):
    """one problem (NL = B = 1, T = 2, three targets) whose point set is pattern `name` on the (hm, wm) map; border=True appends the
    eight image-border points of test_matcher_cost_vs_oracle_odd_shapes (cell-edge points: such a case takes no part in the census)"""
    rng = synth.rng_for(1000 + seed, hm * 64 + wm)
    cells, pred = (pat_one_cell if name == "one_cell" else PATTERNS[name])(hm, wm)
    taps = taps_of_cells(rng, cells, hm, wm)
    if name == "first_row":
        taps[:, 0] = -1
    if name == "spans":                                    # taps at x0 = -1 in the first cell of every run (column 0)
        taps[np.asarray(cells) % wm == 0, 1] = np.where(np.arange((np.asarray(cells) % wm == 0).sum()) % 2 == 0, -1, 0)
    pts = points_at(rng, taps, hm, wm)
    if border:
        pts = np.concatenate([pts, BORDER8])
    masks, cls, tgt, cnt = random_inputs(2000 + seed + hm * 64 + wm + Q, 1, 1, Q, 2, hm, wm, 4 * hm, 4 * wm, [3])
    return Case(f"{name}-{hm}x{wm}-Q{Q}" + ("-border" if border else ""), masks, cls, tgt, cnt, pts[None, None], 4 * hm, 4 * wm,
                predicate=pred, census=not border)


def uniform_case(name, seed, NL, B, Q, T, hm, wm, H, W, counts, P, Nmax=None, amp=4.0):
    """seeded uniform points kept off the cell edges (fractions 0.05 .. 0.95 of a cell, clipped into the image)"""
    rng = synth.rng_for(3000 + seed, P)
    masks, cls, tgt, cnt = random_inputs(seed, NL, B, Q, T, hm, wm, H, W, counts, Nmax, amp)
    ix, iy = rng.integers(-1, wm, (NL, B, P)), rng.integers(-1, hm, (NL, B, P))
    pts = points_at(rng, np.stack([iy.ravel(), ix.ravel()], -1), hm, wm)
    return Case(name, masks, cls, tgt, cnt, pts.reshape(NL, B, P, 2), H, W)


# ------------------------------------------------------------------------------------------------ the trained regime
def trained_case(A, N, Q=100, seed=0, shift=0.03):
    """Confident, correct queries.  Target n is an ellipse; query n is clip(3 A d_n, -A, A) for the ellipse field d_n (1 at the centre,
    0 on the outline, negative outside) sampled at the logit map's pixel centres; query N + n is the same field with the ellipse
    moved by `shift` of the image width (a near-duplicate); queries 2N .. Q-1 are smooth noise of amplitude A clipped to +-A.  The planted
    assignment is target n <-> query n.  One clip, T = 2 (the ellipse moves between the frames), 24 x 40 map, 96 x 160 targets."""
    hm, wm, H, W, T = 24, 40, 96, 160, 2
    rng = synth.rng_for(4000 + seed, N)
    gy, gx = 5, 8                                          # ellipse centres on a jittered 5 x 8 lattice: distinct objects
    slots = rng.permutation(gy * gx)[:N]
    cy = (slots // gx + 0.5 + rng.uniform(-0.15, 0.15, N)) / gy
    cx = (slots % gx + 0.5 + rng.uniform(-0.15, 0.15, N)) / gx
    ry, rx = rng.uniform(0.06, 0.09, N), rng.uniform(0.04, 0.055, N)

    def field(h, w, t, dx):
        y = (np.arange(h) + 0.5)[None, :, None] / h
        x = (np.arange(w) + 0.5)[None, None, :] / w
        ccx = cx + 0.01 * t + dx
        return 1.0 - np.sqrt(((y - cy[:, None, None]) / ry[:, None, None]) ** 2 + ((x - ccx[:, None, None]) / rx[:, None, None]) ** 2)

    tgt = np.stack([(field(H, W, t, 0.0) > 0) for t in range(T)], 1).astype(np.uint8)            # [N,T,H,W]
    masks = np.empty((Q, T, hm, wm), np.float32)
    for t in range(T):
        masks[:N, t] = np.clip(3 * A * field(hm, wm, t, 0.0), -A, A)
        masks[N:2 * N, t] = np.clip(3 * A * field(hm, wm, t, shift), -A, A)
    masks[2 * N:] = np.clip(synth.smooth_logits(5000 + seed, N, (Q - 2 * N, T), (hm, wm), amp=float(A)), -A, A)
    cls = synth.randn(6000 + seed, N, (1, 1, Q, 2), 0.1)
    coords = synth.rng_for(7000 + seed, N).random((1, 1, 1024, 2), dtype=np.float32)
    return Case(f"trained-A{A}-N{N}", masks[None, None], cls, tgt[None], np.array([N], np.int32), coords, H, W, census=False)


def dominance(C, scale, N):
    """smallest margin by which a planted entry C[n, n] is below the rest of its column, in units of the entry-check error scale"""
    C = np.asarray(C, np.float64)
    d = np.array([np.delete(C[:, n], n).min() - C[n, n] for n in range(N)])
    return float(d.min() / (BOUND * scale))
