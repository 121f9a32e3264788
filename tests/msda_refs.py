"""References and input generators for the MSDeformAttn kernels of csrc/msda.hip (numpy / torch on the CPU, no GPU needed).

`msda_ref` restates the core op and its three gradients from the reference's formulas (ms_deform_im2col_cuda.cuh: range test :293,
floor, four corners, zero padding :38-89, gradients :92-164) in float64 (or, for the exactness proofs, float32 in a chosen summation
order); it does not call oracle.msda_core.  On a lattice sample the cell is `floor`, so the derivative is the one from the right /
below, as in the CUDA code.  A sample that fails the range test contributes nothing to any output or gradient.
`fused_ref` is the fused form on top of it (reference points at pixel centres, loc = ref + off / (W, H), softmax over L * P, and the
chain back to raw offsets and logits).  tests/test_msda_refs_cpu.py proves without a GPU that the references and the generated
inputs are what they claim; tests/test_gpu_msda_edges.py compares the kernels with them."""
import numpy as np

MAX_L = 8            # msda.hip: MAX_L
BAD = (float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3e9, -3e9)      # the last two are past int32 after the floor


def level_starts(shapes):
    hw = [h * w for h, w in shapes]
    return np.concatenate([[0], np.cumsum(hw)[:-1]]).astype(np.int64)


def cells(loc, shapes, dtype=np.float64):
    """loc [N,Lq,M,L,P,2] -> (inside bool, h0, w0 int64, h_im, w_im in `dtype`) [N,Lq,M,L,P]: `loc * (W, H) - 0.5` evaluated in `dtype`,
    the range test and the floor (0 where the test fails)"""
    dt = np.dtype(dtype).type
    loc = np.asarray(loc).astype(dtype)
    H = np.array([h for h, _ in shapes], dtype)[None, None, None, :, None]
    W = np.array([w for _, w in shapes], dtype)[None, None, None, :, None]
    with np.errstate(all="ignore"):
        h_im = loc[..., 1] * H - dt(0.5)
        w_im = loc[..., 0] * W - dt(0.5)
        inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)            # cuh:293; false for NaN
        h0 = np.floor(np.where(inside, h_im, 0)).astype(np.int64)
        w0 = np.floor(np.where(inside, w_im, 0)).astype(np.int64)
    return inside, h0, w0, h_im, w_im


def msda_ref(value, shapes, loc, attn, grad_out=None, dtype=np.float64, reverse=False, cell=None):
    """value [N,S,M,D], loc [N,Lq,M,L,P,2], attn [N,Lq,M,L,P], grad_out [N,Lq,M*D] or None
    -> out [N,Lq,M*D], and with grad_out also (grad_value, grad_loc, grad_attn), all in `dtype`.
    Sums run sample by sample (l, p ascending, corners 1..4, channels ascending); reverse=True runs every one of them backwards.
    cell=(h0, w0) [N,Lq,M,L,P]: evaluate every sample in THAT bilinear cell instead of floor's (a cell outside [-1, H-1] x [-1, W-1]
    means skipped): the one-sided value of a neighbouring cell, for samples whose float32 position lands an ulp across the lattice."""
    dt = np.dtype(dtype).type
    value = np.asarray(value).astype(dtype)
    attn = np.asarray(attn).astype(dtype)
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    starts = level_starts(shapes)
    inside, h0, w0, h_im, w_im = cells(loc, shapes, dtype)
    if cell is not None:
        h0, w0 = (np.asarray(c, np.int64) for c in cell)
        Hs = np.array([h for h, _ in shapes])[None, None, None, :, None]
        Ws = np.array([w for _, w in shapes])[None, None, None, :, None]
        with np.errstate(all="ignore"):
            inside = (h0 >= -1) & (h0 <= Hs - 1) & (w0 >= -1) & (w0 <= Ws - 1) & np.isfinite(h_im) & np.isfinite(w_im)
    with np.errstate(all="ignore"):
        lh = np.where(inside, h_im - h0.astype(dtype), 0).astype(dtype)
        lw = np.where(inside, w_im - w0.astype(dtype), 0).astype(dtype)
    hh, hw = dt(1) - lh, dt(1) - lw
    a_eff = np.where(inside, attn, 0).astype(dtype)
    ni = np.arange(N)[:, None, None]
    mi = np.arange(M)[None, None, :]
    grad = grad_out is not None
    out = np.zeros((N, Lq, M, D), dtype)
    if grad:
        go = np.asarray(grad_out).astype(dtype).reshape(N, Lq, M, D)
        gv = np.zeros((N, S, M, D), dtype)
        gl = np.zeros((N, Lq, M, L, P, 2), dtype)
        ga = np.zeros((N, Lq, M, L, P), dtype)
    order = [(l, p) for l in range(L) for p in range(P)]
    chans = list(range(D))
    if reverse:
        order, chans = order[::-1], chans[::-1]
    for l, p in order:
        H, W = shapes[l]
        ins = inside[:, :, :, l, p]
        y0, x0 = h0[:, :, :, l, p], w0[:, :, :, l, p]
        corner = []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            yy, xx = y0 + dy, x0 + dx
            ok = ins & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = starts[l] + np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)
            wy = lh[:, :, :, l, p] if dy else hh[:, :, :, l, p]
            wx = lw[:, :, :, l, p] if dx else hw[:, :, :, l, p]
            v = np.where(ok[..., None], value[ni, idx, mi], dt(0))
            corner.append((ok, idx, (wy * wx).astype(dtype), v))
        a = a_eff[:, :, :, l, p]
        cs = corner[::-1] if reverse else corner
        s = cs[0][2][..., None] * cs[0][3]
        for k in range(1, 4):
            s = s + cs[k][2][..., None] * cs[k][3]
        out = out + s * a[..., None]
        if not grad:
            continue
        d = []
        for ok, idx, cw, v in corner:
            t = np.zeros((N, Lq, M), dtype)
            for c in chans:
                t = t + go[..., c] * v[..., c]
            d.append(t)
            contrib = np.where(ok, cw * a, dt(0))[..., None] * go
            nn, ii, mm = np.broadcast_arrays(ni, idx, mi)
            sel = ok.reshape(-1)
            flat = (nn.reshape(-1)[sel], ii.reshape(-1)[sel], mm.reshape(-1)[sel])
            src = contrib.reshape(-1, D)[sel]
            if reverse:
                flat, src = tuple(f[::-1] for f in flat), src[::-1]
            np.add.at(gv, flat, src)
        c1, c2, c3, c4 = (c[2] for c in corner)
        if reverse:
            ga[:, :, :, l, p] = np.where(ins, c4 * d[3] + c3 * d[2] + c2 * d[1] + c1 * d[0], 0)
        else:
            ga[:, :, :, l, p] = np.where(ins, c1 * d[0] + c2 * d[1] + c3 * d[2] + c4 * d[3], 0)
        yh, yl, xh, xl = hh[:, :, :, l, p], lh[:, :, :, l, p], hw[:, :, :, l, p], lw[:, :, :, l, p]
        gl[:, :, :, l, p, 0] = dt(W) * a * (yh * (d[1] - d[0]) + yl * (d[3] - d[2]))              # cuh:146-149
        gl[:, :, :, l, p, 1] = dt(H) * a * (xh * (d[2] - d[0]) + xl * (d[3] - d[1]))
    out = out.reshape(N, Lq, M * D)
    return (out, gv, gl, ga) if grad else out


def reference_points(shapes, dtype=np.float64):
    """[S,2] (x, y): the normalised centre of every pixel of the flattened pyramid"""
    pts = []
    for H, W in shapes:
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pts.append(np.stack([((xs.astype(dtype) + 0.5) / dtype(W)).reshape(-1), ((ys.astype(dtype) + 0.5) / dtype(H)).reshape(-1)], -1))
    return np.concatenate(pts, 0).astype(dtype)


def fused_expand(oa, shapes, M, P, dtype=np.float64):
    """oa [N,S,>=M*L*P*3]: raw offsets [M][L][P][2] then raw logits [M][L*P] per query -> (loc [N,S,M,L,P,2], attn [N,S,M,L,P]) in `dtype`
    (ms_deform_attn.py:101-109 with the query's own pixel centre as its reference point on every level)"""
    dt = np.dtype(dtype).type
    oa = np.asarray(oa).astype(dtype)
    N, S, _ = oa.shape
    L = len(shapes)
    LP = L * P
    off = oa[..., :M * LP * 2].reshape(N, S, M, L, P, 2)
    lg = oa[..., M * LP * 2:M * LP * 3].reshape(N, S, M, LP)
    norm = np.array([[w, h] for h, w in shapes], dtype)[None, None, None, :, None, :]
    with np.errstate(all="ignore"):
        loc = reference_points(shapes, dt)[None, :, None, None, None, :] + off / norm
    e = np.exp(lg - lg.max(-1, keepdims=True))
    attn = (e / e.sum(-1, keepdims=True)).reshape(N, S, M, L, P)
    return loc.astype(dtype), attn.astype(dtype)


def fused_ref(value, shapes, oa, M, P, grad_out=None, cell=None):
    """float64: value [N,S,M*D], oa as fused_expand -> out [N,S,M*D], with grad_out also (d_value [N,S,M*D], d_oa [N,S,M*L*P*3])"""
    N, S, C = value.shape
    L = len(shapes)
    loc, attn = fused_expand(oa, shapes, M, P)
    v4 = np.asarray(value, np.float64).reshape(N, S, M, C // M)
    if grad_out is None:
        return msda_ref(v4, shapes, loc, attn, cell=cell)
    out, gv, gl, ga = msda_ref(v4, shapes, loc, attn, grad_out, cell=cell)
    norm = np.array([[w, h] for h, w in shapes], np.float64)[None, None, None, :, None, :]
    d_off = gl / norm
    dot = (attn * ga).sum((-1, -2), keepdims=True)
    d_lg = attn * (ga - dot)                                         # softmax backward; an exactly skipped sample has ga = 0
    d_oa = np.concatenate([d_off.reshape(N, S, -1), d_lg.reshape(N, S, -1)], -1)
    return out, gv.reshape(N, S, C), d_oa


def cells_fused(oa, shapes, M, P, dtype):
    """the bilinear cells of the fused form's samples with loc = ref + off / (W, H) evaluated in `dtype`, as the kernels do"""
    dt = np.dtype(dtype).type
    oa = np.asarray(oa)
    N, S, _ = oa.shape
    L = len(shapes)
    off = oa[..., :M * L * P * 2].reshape(N, S, M, L, P, 2).astype(dtype)
    norm = np.array([[w, h] for h, w in shapes], dtype)[None, None, None, :, None, :]
    with np.errstate(all="ignore"):
        loc = reference_points(shapes, dt)[None, :, None, None, None, :] + off / norm
    return cells(loc.astype(dtype), shapes, dtype)


# ----------------------------------------------------------------------------- torch restatement (grid_sample), for the rule's float32 figure
def msda_torch(value, shapes, loc, attn, grad_out=None):
    """ms_deform_attn_core_pytorch (ms_deform_attn_func.py:52-72) in the operands' dtype on their device.  grid_sample's behaviour on a
    NaN / infinite / huge coordinate is not specified, so such a location is first moved far outside every map, where it is skipped
    like the original.  -> out, and with grad_out also (grad_value, grad_loc, grad_attn) by autograd."""
    import torch
    import torch.nn.functional as F
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    grad = grad_out is not None
    v = value.detach().clone().requires_grad_(grad)
    bad = ~(loc.abs() < 1e6)
    lo_in = torch.where(bad, torch.full_like(loc, -10.0), loc).detach().clone().requires_grad_(grad)
    w = attn.detach().clone().requires_grad_(grad)
    starts = level_starts(shapes)
    acc = 0
    for l, (H, W) in enumerate(shapes):
        vl = v[:, int(starts[l]):int(starts[l]) + H * W].reshape(N, H * W, M * D).transpose(1, 2).reshape(N * M, D, H, W)
        grid = (2 * lo_in[:, :, :, l] - 1).transpose(1, 2).reshape(N * M, Lq, P, 2)
        smp = F.grid_sample(vl, grid, mode="bilinear", padding_mode="zeros", align_corners=False)              # [N*M, D, Lq, P]
        wl = w[:, :, :, l].transpose(1, 2).reshape(N * M, 1, Lq, P)
        acc = acc + (smp * wl).sum(-1)
    out = acc.reshape(N, M * D, Lq).transpose(1, 2)
    if not grad:
        return out.detach()
    (out * grad_out).sum().backward()
    return out.detach(), v.grad, lo_in.grad, w.grad


def fused_torch(value, shapes, oa, M, P, grad_out=None):
    """the fused form with torch arithmetic in the operands' dtype / device -> out, and with grad_out also (d_value, d_oa)"""
    import torch
    N, S, C = value.shape
    L = len(shapes)
    LP = L * P
    grad = grad_out is not None
    v = value.detach().clone().requires_grad_(grad)
    o = oa[..., :M * LP * 3].detach().clone().requires_grad_(grad)
    off = o[..., :M * LP * 2].reshape(N, S, M, L, P, 2)
    okoff = off.abs() < 1e6
    off = torch.where(okoff, off, torch.full_like(off, -1e4))           # far outside every map: skipped like the original
    lg = o[..., M * LP * 2:].reshape(N, S, M, LP)
    ref = torch.as_tensor(reference_points(shapes), dtype=value.dtype, device=value.device)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=value.dtype, device=value.device)
    loc = ref[None, :, None, None, None, :] + off / norm[None, None, None, :, None, :]
    attn = torch.softmax(lg, -1).reshape(N, S, M, L, P)
    starts = level_starts(shapes)
    acc = 0
    import torch.nn.functional as F
    v4 = v.reshape(N, S, M, C // M)
    D = C // M
    for l, (H, W) in enumerate(shapes):
        vl = v4[:, int(starts[l]):int(starts[l]) + H * W].reshape(N, H * W, M * D).transpose(1, 2).reshape(N * M, D, H, W)
        grid = (2 * loc[:, :, :, l] - 1).transpose(1, 2).reshape(N * M, S, P, 2)
        smp = F.grid_sample(vl, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        acc = acc + (smp * attn[:, :, :, l].transpose(1, 2).reshape(N * M, 1, S, P)).sum(-1)
    out = acc.reshape(N, M * D, S).transpose(1, 2)
    if not grad:
        return out.detach()
    (out * grad_out).sum().backward()
    return out.detach(), v.grad, o.grad


# ----------------------------------------------------------------------------- case generators
LATTICE_PYRAMIDS = {"pow2": [(4, 8), (2, 4), (1, 2)], "h1": [(1, 8), (1, 4), (1, 2)], "w1": [(8, 1), (4, 1), (2, 1)]}
OFFGRID_PYRAMID = [(5, 9), (11, 19), (23, 37)]


def axis_targets(W):
    """pixel-space positions -2, -1.5, -1, ..., W + 0.5, W + 1: loc = (k + 0.5) / W for every integer k in -2 .. W + 1, and the half steps"""
    return np.arange(-4, 2 * (W + 1) + 1) / 2.0


def _f32(x):
    return np.float32(x)


def border_neighbours(W):
    """float32 positions next to -1 and to W on either side (np.nextafter), each one the nearest for which `w_im + 0.5` is a float32 --
    so that loc = (w_im + 0.5) / W (W a power of two: an exact division) gives back exactly this w_im in float32 and in float64.
    (Just below W the adjacent float fails that: W - ulp/2 + 0.5 is not a float32; the next one down is taken.)"""
    res = []
    for edge, toward in ((-1.0, -np.inf), (-1.0, np.inf), (float(W), -np.inf), (float(W), np.inf)):
        x = _f32(edge)
        for _ in range(4):
            x = np.nextafter(x, _f32(toward))
            t = _f32(x + _f32(0.5))
            if float(t) == float(x) + 0.5 and float(_f32(_f32(t / _f32(W)) * _f32(W)) - _f32(0.5)) == float(x):
                break
        else:
            raise AssertionError("no exact neighbour")
        res.append(float(x))
    return res


def _dyadic(rng, shape, lo, hi, den):
    return (rng.integers(lo, hi + 1, shape) / den).astype(np.float32)


def lattice_case(pyramid="pow2", P=4, M=8, D=32, N=2, seed=0):
    """Drop-in operands on power-of-two levels.  Heads 0 .. M-2: every (y, x) pair of axis_targets on every level, dealt over (query,
    point, head).  Head M-1: positions one float off the -1 / W borders in one axis, on a pixel centre in the other (their weights
    are powers of two around 2^-20, so they get a head of their own: exact among themselves, not beside weights of order 1).
    Values, attention weights and grad_out are small dyadic numbers."""
    shapes = LATTICE_PYRAMIDS[pyramid]
    L = len(shapes)
    rng = np.random.default_rng(seed)
    combos = []
    for H, W in shapes:
        ys, xs = axis_targets(H), axis_targets(W)
        combos.append(np.array([(y, x) for y in ys for x in xs]))
    reg = M - 1
    Lq = max(-(-len(c) // (P * reg)) for c in combos)
    Lq = max(Lq, -(-max(4 * (h + w) for h, w in shapes) // P))           # and every near-border position of head M-1
    S = sum(h * w for h, w in shapes)
    tgt = np.zeros((N, Lq, M, L, P, 2))                               # pixel-space (x, y)
    for l, (H, W) in enumerate(shapes):
        c = combos[l]
        near = []
        for x in border_neighbours(W):
            near += [(float(y), x) for y in range(H)]
        for y in border_neighbours(H):
            near += [(y, float(x)) for x in range(W)]
        near = np.array(near)
        for n in range(N):
            for q in range(Lq):
                for p in range(P):
                    j = q * P + p
                    for m in range(reg):
                        y, x = c[(j * reg + m + 11 * n) % len(c)]
                        tgt[n, q, m, l, p] = (x, y)
                    y, x = near[(j + 5 * n) % len(near)]
                    tgt[n, q, M - 1, l, p] = (x, y)
    norm = np.array([[w, h] for h, w in shapes], np.float64)[None, None, None, :, None, :]
    loc = ((tgt + 0.5) / norm).astype(np.float32)
    assert np.array_equal(loc.astype(np.float64), (tgt + 0.5) / norm), "a lattice location is not a float32"
    value = _dyadic(rng, (N, S, M, D), -8, 8, 4)
    attn = _dyadic(rng, (N, Lq, M, L, P), 1, 4, 8)
    grad_out = _dyadic(rng, (N, Lq, M * D), -8, 8, 4)
    props = {"targets": tgt, "covered": [len(c) for c in combos], "near_head": M - 1}
    return {"shapes": shapes, "value": value, "loc": loc, "attn": attn, "grad_out": grad_out, "props": props}


def fused_lattice_case(pyramid="pow2", seed=1, N=2):
    """Fused operands (M = 8, D = 32, L = 3, P = 4) whose raw offsets put every sample on a lattice target of a power-of-two level:
    off = target - ((q + 0.5) * W_l / W_q - 0.5), exact in float32; logits are random (the softmax is not dyadic).
    pyramid="offgrid": the same on OFFGRID_PYRAMID, where the offset is rounded to float32 and the kernels' float32
    `(ref + off / W) * W - 0.5` may land an ulp off the target."""
    shapes = OFFGRID_PYRAMID if pyramid == "offgrid" else LATTICE_PYRAMIDS[pyramid]
    M, D, L, P = 8, 32, 3, 4
    rng = np.random.default_rng(seed)
    S = sum(h * w for h, w in shapes)
    ref = reference_points(shapes)
    tgt = np.zeros((N, S, M, L, P, 2))
    for l, (H, W) in enumerate(shapes):
        c = np.array([(y, x) for y in axis_targets(H) for x in axis_targets(W)])
        idx = (np.arange(N)[:, None, None, None] * 11 + (np.arange(S)[None, :, None, None] * P + np.arange(P)[None, None, None, :]) * M
               + np.arange(M)[None, None, :, None]) % len(c)
        tgt[:, :, :, l, :, 0] = c[idx, 1]
        tgt[:, :, :, l, :, 1] = c[idx, 0]
    norm = np.array([[w, h] for h, w in shapes], np.float64)[None, None, None, :, None, :]
    off64 = tgt - (ref[None, :, None, None, None, :] * norm - 0.5)
    off = off64.astype(np.float32)
    assert pyramid == "offgrid" or np.array_equal(off.astype(np.float64), off64)
    lg = rng.standard_normal((N, S, M, L * P)).astype(np.float32)
    oa = np.concatenate([off.reshape(N, S, -1), lg.reshape(N, S, -1)], -1)
    value = rng.standard_normal((N, S, M * D)).astype(np.float32)
    grad_out = rng.standard_normal((N, S, M * D)).astype(np.float32)
    return {"shapes": shapes, "value": value, "oa": oa, "grad_out": grad_out, "M": M, "P": P, "props": {"targets": tgt}}


def offgrid_case(seed=2, N=1, Lq=160, M=8, D=32, P=4):
    """The lattice targets on levels that are no powers of two: float32 `loc * W - 0.5` may land an ulp off the lattice.  Points 0, 1
    of every (query, head, level) are deliberate lattice / border targets, points 2, 3 are drawn from rand * 1.2 - 0.1."""
    shapes = OFFGRID_PYRAMID
    L = len(shapes)
    rng = np.random.default_rng(seed)
    S = sum(h * w for h, w in shapes)
    loc = (rng.random((N, Lq, M, L, P, 2)) * 1.2 - 0.1).astype(np.float32)
    tgt = np.full((N, Lq, M, L, P, 2), np.nan)
    for l, (H, W) in enumerate(shapes):
        c = np.array([(y, x) for y in axis_targets(H) for x in axis_targets(W)])
        j = ((np.arange(N)[:, None, None, None] * Lq + np.arange(Lq)[None, :, None, None]) * M + np.arange(M)[None, None, :, None]) * 2 + np.arange(2)[None, None, None, :]
        idx = (j * 7) % len(c)
        tgt[:, :, :, l, :2, 0] = c[idx, 1]
        tgt[:, :, :, l, :2, 1] = c[idx, 0]
        loc[:, :, :, l, :2, 0] = ((tgt[:, :, :, l, :2, 0] + 0.5) / W).astype(np.float32)
        loc[:, :, :, l, :2, 1] = ((tgt[:, :, :, l, :2, 1] + 0.5) / H).astype(np.float32)
    deliberate = ~np.isnan(tgt[..., 0])
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    attn = rng.random((N, Lq, M, L, P)).astype(np.float32)
    attn /= attn.sum((-1, -2), keepdims=True)
    grad_out = rng.standard_normal((N, Lq, M * D)).astype(np.float32)
    return {"shapes": shapes, "value": value, "loc": loc, "attn": attn, "grad_out": grad_out,
            "props": {"targets": tgt, "deliberate": deliberate}}


def adjacent_cells(tgt):
    """lattice targets [...,2] (x, y) -> ((h_hi, w_hi), (h_lo, w_lo)): the cell right of / below an integer target and the one left of /
    above it; both are floor(target) where the target is not an integer"""
    t = np.nan_to_num(tgt)
    hi = np.floor(t).astype(np.int64)
    lo = hi - (t == np.floor(t)).astype(np.int64)
    return (hi[..., 1], hi[..., 0]), (lo[..., 1], lo[..., 0])


# The finest level last and larger than the other two together: the condition under which S2D_MSDA_WIN=1 selects the windowed fused
# kernel.  That kernel computes the queries of the LAST level only (the TILED kernel beside it takes the others), so the fused case
# poisons queries of the last level as well as of level 0.
NONFINITE_PYRAMID = [(5, 9), (6, 7), (11, 19)]


def _poison(arr, bases=(0,)):
    """arr [N,Lq,M,L,P,2] (locations or raw offsets), in place, once per base query q0 in `bases`.  Row (n = 0, q = q0 + k, m = k % M),
    k = 0..6: BAD[k] in x of one sample; q = q0 + 7 + k: in y; q = q0 + 14 + k: in both, and in two samples.  Row (n = N-1, q = q0 + 3,
    m = 2): every sample, cycling through BAD.  -> (bool mask of the poisoned samples, mixed rows [(n, q, m)], all-bad rows [(n, q, m)])"""
    N, Lq, M, L, P, _ = arr.shape
    bad = np.zeros((N, Lq, M, L, P), bool)
    mixed, allbad = [], []
    for q0 in bases:
        for k, b in enumerate(BAD):
            m = k % M
            arr[0, q0 + k, m, k % L, k % P, 0] = b
            bad[0, q0 + k, m, k % L, k % P] = True
            arr[0, q0 + 7 + k, m, (k + 1) % L, (k + 2) % P, 1] = b
            bad[0, q0 + 7 + k, m, (k + 1) % L, (k + 2) % P] = True
            for s in ((0, 0), (L - 1, P - 1)):
                arr[0, q0 + 14 + k, m, s[0], s[1], :] = b
                bad[0, q0 + 14 + k, m, s[0], s[1]] = True
            mixed += [(0, q0 + k, m), (0, q0 + 7 + k, m), (0, q0 + 14 + k, m)]
        i = 0
        for l in range(L):
            for p in range(P):
                arr[N - 1, q0 + 3, 2, l, p, i % 2] = BAD[i % len(BAD)]
                if i % 3 == 0:
                    arr[N - 1, q0 + 3, 2, l, p, :] = BAD[i % len(BAD)]
                i += 1
        bad[N - 1, q0 + 3, 2] = True
        allbad.append((N - 1, q0 + 3, 2))
    return bad, mixed, allbad


def nonfinite_case(seed=3, N=2, Lq=24, M=8, D=32, P=4):
    shapes = NONFINITE_PYRAMID
    L = len(shapes)
    rng = np.random.default_rng(seed)
    S = sum(h * w for h, w in shapes)
    loc = (rng.random((N, Lq, M, L, P, 2)) * 0.9 + 0.05).astype(np.float32)        # ordinary samples: inside the maps
    bad, mixed, allbad = _poison(loc)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    attn = rng.random((N, Lq, M, L, P)).astype(np.float32) + 0.1
    attn /= attn.sum((-1, -2), keepdims=True)
    grad_out = rng.standard_normal((N, Lq, M * D)).astype(np.float32)
    return {"shapes": shapes, "value": value, "loc": loc, "attn": attn, "grad_out": grad_out,
            "props": {"bad": bad, "all_rows": allbad, "mixed_rows": mixed}}


def fused_nonfinite_case(seed=4, N=2):
    """the poisoned rows sit in queries 0 .. 20 of level 0 and in queries 5 .. 25 of the last level (rows 0 and 1 of its first two
    8 x 8 query patches, which the windowed kernel computes)"""
    shapes = NONFINITE_PYRAMID
    M, D, L, P = 8, 32, 3, 4
    rng = np.random.default_rng(seed)
    S = sum(h * w for h, w in shapes)
    off = (rng.standard_normal((N, S, M, L, P, 2)) * 0.7).astype(np.float32)        # ordinary samples: within a pixel or two of the query
    last = int(level_starts(shapes)[-1])
    bad, mixed, allbad = _poison(off, bases=(0, last + 5))
    lg = rng.standard_normal((N, S, M, L * P)).astype(np.float32)
    oa = np.concatenate([off.reshape(N, S, -1), lg.reshape(N, S, -1)], -1)
    value = rng.standard_normal((N, S, M * D)).astype(np.float32)
    grad_out = rng.standard_normal((N, S, M * D)).astype(np.float32)
    return {"shapes": shapes, "value": value, "oa": oa, "grad_out": grad_out, "M": M, "P": P,
            "props": {"bad": bad, "all_rows": allbad, "mixed_rows": mixed, "last_level_start": last}}


def offgrid_disagreement(c):
    """-> (mask of the offgrid samples whose float32 cell or range test differs from the float64 one, its share among the samples that
    are not deliberately on the lattice, its share among the deliberate ones)"""
    i64, h64, w64, _, _ = cells(c["loc"], c["shapes"])
    i32, h32, w32, _, _ = cells(c["loc"], c["shapes"], np.float32)
    diff = (i64 != i32) | (i64 & ((h64 != h32) | (w64 != w32)))
    d = c["props"]["deliberate"]
    return diff, float(diff[~d].mean()), float(diff[d].mean())


def fused_offgrid_disagreement(c):
    """-> mask of the fused offgrid samples whose float32 cell or range test (the kernels' arithmetic) differs from the float64 one"""
    i64, h64, w64, _, _ = cells_fused(c["oa"], c["shapes"], c["M"], c["P"], np.float64)
    i32, h32, w32, _, _ = cells_fused(c["oa"], c["shapes"], c["M"], c["P"], np.float32)
    return (i64 != i32) | (i64 & ((h64 != h32) | (w64 != w32)))


SEGMENT_PYRAMID = [(6, 7), (3, 5)]
SEGMENT_COUNTS = {(1, 1): 1, (1, 2): 7, (1, 3): 8, (2, 1): 9, (2, 2): 16, (2, 3): 17, (3, 3): 0}       # level 0 cell (h0, w0) -> samples


def _cell_loc(rng, shapes, l, h0, w0, n):
    """n locations inside cell (h0, w0) of level l, away from its edges"""
    H, W = shapes[l]
    fy, fx = rng.random(n) * 0.8 + 0.1, rng.random(n) * 0.8 + 0.1
    return np.stack([(w0 + fx + 0.5) / W, (h0 + fy + 0.5) / H], -1).astype(np.float32)


def segments_case(kind="counts", seed=5, N=2, M=8, D=32, P=4):
    """kind "counts": within (frame 0, head 0) the level-0 cells of SEGMENT_COUNTS receive exactly that many samples (8 is the batch
    size of msda_bwd_value_kernel) and no other level-0 sample of that head is inside the map; everything else is random.
    "one_cell": every sample of the call in cell (1, 1) of its level.  "all_outside": every sample outside every map (all keys kmax).
    "corners": every sample in cell (-1, -1) or (H - 1, W - 1) of its level."""
    shapes = SEGMENT_PYRAMID
    L = len(shapes)
    rng = np.random.default_rng(seed)
    S = sum(h * w for h, w in shapes)
    Lq = 16
    loc = (rng.random((N, Lq, M, L, P, 2)) * 1.2 - 0.1).astype(np.float32)
    if kind == "counts":
        slots = [(q, p) for q in range(Lq) for p in range(P)]
        rng.shuffle(slots)
        loc[0, :, 0, 0] = -5.0
        i = 0
        for (h0, w0), cnt in SEGMENT_COUNTS.items():
            pts = _cell_loc(rng, shapes, 0, h0, w0, cnt)
            for k in range(cnt):
                q, p = slots[i]
                loc[0, q, 0, 0, p] = pts[k]
                i += 1
    elif kind == "one_cell":
        for l in range(L):
            loc[:, :, :, l] = _cell_loc(rng, shapes, l, 1, 1, N * Lq * M * P).reshape(N, Lq, M, P, 2)
    elif kind == "all_outside":
        loc = (2.0 + rng.random((N, Lq, M, L, P, 2))).astype(np.float32)
        loc[:, ::2] *= -1
    elif kind == "corners":
        for l, (H, W) in enumerate(shapes):
            a = _cell_loc(rng, shapes, l, -1, -1, N * Lq * M * P).reshape(N, Lq, M, P, 2)
            b = _cell_loc(rng, shapes, l, H - 1, W - 1, N * Lq * M * P).reshape(N, Lq, M, P, 2)
            loc[:, :, :, l] = np.where((np.arange(Lq) % 2 == 0)[None, :, None, None, None], a, b)
    else:
        raise ValueError(kind)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    attn = rng.random((N, Lq, M, L, P)).astype(np.float32)
    attn /= attn.sum((-1, -2), keepdims=True)
    grad_out = rng.standard_normal((N, Lq, M * D)).astype(np.float32)
    return {"shapes": shapes, "value": value, "loc": loc, "attn": attn, "grad_out": grad_out, "props": {"kind": kind}}


def cell_counts(loc, shapes, n, m, l):
    """{(h0, w0): samples} of frame n, head m, level l (float32 cells, as msda_cell_key_kernel forms them)"""
    inside, h0, w0, _, _ = cells(loc, shapes, np.float32)
    sel = inside[n, :, m, l]
    out = {}
    for a, b in zip(h0[n, :, m, l][sel].tolist(), w0[n, :, m, l][sel].tolist()):
        out[(a, b)] = out.get((a, b), 0) + 1
    return out


# ----------------------------------------------------------------------------- geometries and the branches they reach
_LEVEL_POOL = [(7, 9), (5, 6), (3, 5), (1, 5), (2, 3), (6, 1), (3, 3), (2, 5), (1, 1), (2, 2), (3, 2), (5, 3)]      # no extent pair of multiples of 4


def pyramid(L):
    return _LEVEL_POOL[:L]


DROPIN_LQ = (1, 5, 33)
DROPIN_GEOMETRIES = [(8, 32, 4, 4), (8, 32, 4, 8), (8, 32, 1, 1), (8, 32, 2, 8), (3, 32, 2, 3), (1, 32, 3, 4), (16, 32, 3, 4)]     # (M, D, L, P): forward + backward
DROPIN_FORWARD_ONLY = [(8, 2, 3, 4), (8, 10, 3, 4), (8, 16, 3, 4), (8, 64, 3, 4)]
FUSED_GEOMETRIES = [(8, 4, 3), (8, 2, 6), (8, 1, 12), (8, 12, 1), (4, 3, 4), (16, 3, 4), (1, 3, 4)]                                # (M, L, P)
TWO_STEP_LP = [(1, 4), (2, 4), (3, 4), (4, 4)]                                                                                      # (L, P): L * P in 4, 8, 12, 16


def dropin_branches(M, D, L, P, Lq, shapes=None):
    """the selecting conditions of launch_forward, msda_fwd_kernel and msda_bwd_loc_kernel (msda.hip), restated"""
    b = set()
    V = 4 if D % 4 == 0 else 1                                        # launch_forward: (D & 3) == 0
    b.add("fwd<4>" if V == 4 else "fwd<1>")
    dv = D // V
    if V == 4 and dv == 8 and L * P <= 16:                            # msda_fwd_kernel: the 8-lane shuffle path
        b.add("fwd:shuffle")
        if L * P == 16:
            b.add("fwd:shuffle_full")                                 # both of a lane's sample slots live in every lane
        if L * P <= 8:
            b.add("fwd:shuffle_one_slot")
    else:
        b.add("fwd:loops")
        if V == 4:
            b.add("fwd<4>:loops")
    items = Lq * M * dv
    if items % 256:
        b.add("fwd:ragged_block")                                     # the `item >= Lq * M * dv` exit is taken by part of a block
    if items > 256:
        b.add("fwd:several_blocks")
    if D == 32:                                                       # the float32 backward exists for D == 32 only
        b.add("bwd_loc:shuffle" if L * P <= 16 else "bwd_loc:loops")
        if Lq * M * 8 < 256:
            b.add("bwd_loc:under_one_block")
        if Lq * M * 8 > 256:
            b.add("bwd_loc:several_blocks")
        if M != 8:
            b.add("bwd:M!=8")
    else:
        b.add("bwd:rejected")
    if shapes is not None and any(h == 1 or w == 1 for h, w in shapes):
        b.add("level:H1_or_W1")
    return b


DROPIN_BRANCHES = {"fwd<4>", "fwd<1>", "fwd:shuffle", "fwd:shuffle_full", "fwd:shuffle_one_slot", "fwd:loops", "fwd<4>:loops", "fwd:ragged_block",
                   "fwd:several_blocks", "bwd_loc:shuffle", "bwd_loc:loops", "bwd_loc:under_one_block",
                   "bwd_loc:several_blocks", "bwd:M!=8", "bwd:rejected", "level:H1_or_W1"}


def fused_branch(M, L, P, env=None, shapes=None, S=None):
    """the kernel s2d_msda_fused_forward_f32 selects (msda.hip), restated; env: the S2D_MSDA_* switches as a dict of ints"""
    env = env or {}
    if L < 1 or L > MAX_L or L * P != 12:
        return "rejected"                                             # fill_levels: L > MAX_L; the entry point: L * P != 12
    share, tiled = env.get("SHARE", 1), env.get("TILED", 1)
    if tiled and M == 8:
        if env.get("WIN", 0) and L == 3 and P == 4 and shapes is not None:
            lq = max(range(L), key=lambda l: (shapes[l][0] * shapes[l][1], -l))
            if lq == L - 1 and 2 * shapes[lq][0] * shapes[lq][1] > S:
                return "win+tiled"
        if env.get("HEAD", 0) and L > 1:
            return "head"
        rec = env.get("REC", 1)
        if rec and L == 3 and P == 4:
            return "rec4" if rec == 2 else "rec8"
        return "tiled"
    return "share" if share else "plain"


FUSED_BRANCHES = {"rejected", "win+tiled", "head", "rec8", "rec4", "tiled", "share", "plain"}
FUSED_ENVS = [{}, {"REC": 0}, {"REC": 2}, {"TILED": 0}, {"TILED": 0, "SHARE": 0}, {"WIN": 1}, {"HEAD": 1}]


def geometry_case(M, D, L, P, Lq, seed=6, N=2):
    shapes = pyramid(L)
    rng = np.random.default_rng(seed + 7 * M + D + 3 * L + P + Lq)
    S = sum(h * w for h, w in shapes)
    loc = (rng.random((N, Lq, M, L, P, 2)) * 1.2 - 0.1).astype(np.float32)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    attn = rng.random((N, Lq, M, L, P)).astype(np.float32)
    attn /= attn.sum((-1, -2), keepdims=True)
    grad_out = rng.standard_normal((N, Lq, M * D)).astype(np.float32)
    return {"shapes": shapes, "value": value, "loc": loc, "attn": attn, "grad_out": grad_out, "props": {}}


def fused_geometry_case(M, L, P, seed=7, N=2, D=32, shapes=None):
    shapes = shapes or pyramid(L)
    rng = np.random.default_rng(seed + 5 * M + L)
    S = sum(h * w for h, w in shapes)
    off = (rng.standard_normal((N, S, M, L, P, 2)) * 2.0).astype(np.float32)
    lg = rng.standard_normal((N, S, M, L * P)).astype(np.float32)
    oa = np.concatenate([off.reshape(N, S, -1), lg.reshape(N, S, -1)], -1)
    value = rng.standard_normal((N, S, M * D)).astype(np.float32)
    grad_out = rng.standard_normal((N, S, M * D)).astype(np.float32)
    return {"shapes": shapes, "value": value, "oa": oa, "grad_out": grad_out, "M": M, "P": P, "props": {}}
