"""Float64 restatement of the proposal index maps (`ops.infer_index`, csrc/infer.hip `infer_index_kernel`), the bands inside which
float32 may decide differently, and the shared inputs of tests/test_davis_index_refs_cpu.py and tests/test_gpu_infer_index.py.
Numpy only; nothing here calls a kernel.

Definition.  For proposal k (column query[k] of the pixel-major logits) v_k = bilinear(bilinear(plane -> padded size)[:ih, :iw] ->
output size), align_corners=False, the second resize skipped when the output size is the image size.  Proposal k HOLDS a pixel iff
v_k > 0 (NaN and -0.0 hold nothing).  rule "rank": label = 1 + the lowest holding k.  rule "prob": label = 1 + the holding k with the
largest score[k] * sigmoid(v_k), ties to the lower k.  No holder: label 0.

Sign band (band_v; `_mask_band` of tests/test_gpu_eval_720p.py, restated).  The kernel forms each source coordinate
`scale * (dst + 0.5) - 0.5` in float32 -- the scale rounded once, one product, one difference: at most 3 units of 2^-24 of a
coordinate as large as the SOURCE size of its stage.  Stage 1 (hm x wm -> Hp x Wp): <= 3 * 2^-24 * max(hm, wm) low-resolution
pixels, over a bilinear surface that moves at most D per low-resolution pixel along an axis (D = the largest difference of
adjacent taps of the input), so <= 3 * 2^-24 * max(hm, wm) * D per axis.  Stage 2 moves the coordinate by <= 3 * 2^-24 * max(ih, iw)
padded pixels over a surface of slope <= D * hm / Hp per padded pixel: the same figure.  Two axes, two stages: 12 * 2^-24 *
max(hm, wm) * D.  The coarser statement -- 2^-24 of a coordinate as large as the largest padded / output extent C, times D, per axis
and stage -- is 4 * 2^-24 * C * D; the band takes the larger.  Arithmetic: each stage is a 4-tap float32 sum of products with
weights in [0, 1], a few units of 2^-24 of the largest tap A per stage, taken as 8 each:

    band_v = 2^-24 * (max(4 * C, 12 * max(hm, wm)) * D + 16 * A)

Outside |v_k| < band_v the float32 sign of v_k is the float64 sign, so the holding sets agree.

Rank rule exclusion.  The label is 1 + the first k with v_k > 0.  Let k* be the first k whose float64 v_k > -band_v (the first
that float32 could see as holding).  If v_{k*} >= band_v, every k < k* is negative in float32 too and k* holds in both: the label
is decided.  So a pixel is excluded iff k* exists and |v_{k*}| < band_v.  (Every pixel with some selected |v_k| < band_v before its
first definite holder is in this set; the later ones cannot change the label.)

Prob rule band.  With |dv| <= band_v and sigmoid' <= 1/4, sigmoid(v_k) moves by at most band_v / 4.  The float32 formula
s / (1.f + expf(-v)) adds the rounding of expf (a few ulp at most), of the add and of the divide, each relative to a result <= 1:
an allowance of c = 16 units of 2^-24 covers them with room.  A product therefore moves by at most

    bound_p = s_max * (band_v / 4 + 16 * 2^-24)

and the order of two products can change only when they differ by less than 2 * bound_p.  The first statement of the exclusion
(`excluded_wide`) is: any selected |v_k| < band_v (a holding set that float32 may see differently), or the best and second-best
float64 products among the holders closer than 2 * bound_p.  Its first clause grows linearly with K -- every plane has its own
zero crossings -- and measures 3e-2 of the pixels at K = 254, thirty times the cap, although a proposal that flickers at
sigmoid = 1/2 far below the winner changes nothing.  `excluded(rule="prob")` is therefore the narrower set that the same
two bounds justify, in the form of the rank rule's: the CANDIDATES are the k with v_k > -band_v (float32 could see them holding),
q_k = score_k * sigmoid(v_k) for them (for a candidate below zero this is the product float32 would form if it saw it holding,
within bound_p); a pixel is excluded iff its best candidate has |v| < band_v (the winner itself may not hold), or the best and
second-best q differ by less than (s_best + s_second) * (band_v / 4 + 16 * 2^-24) -- each product with the bound of its own
score, which is at most 2 * bound_p.  Otherwise the best candidate holds in both precisions and beats every other
possible holder by more than both errors: the label is decided.  Every pixel excluded this way is excluded by the first
statement too (asserted on the CPU), so the comparison asks more, never less.  Equal products of the named tie row are built
from dyadic numbers and are not compared through this band.

The excluded share is capped at 1e-3 (CAP) for every input of CASES, on the CPU, from the reference alone."""
import numpy as np

CAP = 1e-3
EXP_ALLOWANCE = 16


# ------------------------------------------------------------------------------------------------------------------ resize
def _taps(out_size, in_size, scale, dtype):
    """F.interpolate(mode="bilinear", align_corners=False) source taps of every destination index, in `dtype` arithmetic"""
    d = np.arange(out_size).astype(dtype)
    s = dtype(scale) * (d + dtype(0.5)) - dtype(0.5)
    s = np.where(s < 0, dtype(0), s).astype(dtype)
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (s - i0.astype(dtype)).astype(dtype)
    return i0, i1, (dtype(1) - l1).astype(dtype), l1


def _bilinear(x, size, dtype):
    """x [..., h, w] -> [..., size]; weights and sums in `dtype` in F.interpolate's order: (hy * (hx*a + lx*b) + ly * (hx*c + lx*d))"""
    h, w = x.shape[-2:]
    oh, ow = size
    sy = dtype(h) / dtype(oh) if dtype is np.float64 else np.float32(np.float32(h) / np.float32(oh))
    sx = dtype(w) / dtype(ow) if dtype is np.float64 else np.float32(np.float32(w) / np.float32(ow))
    y0, y1, hy, ly = _taps(oh, h, sy, dtype)
    x0, x1, hx, lx = _taps(ow, w, sx, dtype)
    r0, r1 = x[..., y0, :], x[..., y1, :]
    top = hx * r0[..., x0] + lx * r0[..., x1]
    bot = hx * r1[..., x0] + lx * r1[..., x1]
    return (hy[:, None] * top + ly[:, None] * bot).astype(dtype)


def two_stage(planes, padded, img_size, out_size, dtype=np.float64):
    """planes [..., hm, wm] -> [..., oh, ow] in `dtype`: to the padded size, crop to the image, to the output size unless equal"""
    with np.errstate(invalid="ignore"):
        v = _bilinear(np.asarray(planes, dtype), tuple(padded), dtype)[..., :img_size[0], :img_size[1]]
        return v if tuple(img_size) == tuple(out_size) else _bilinear(v, tuple(out_size), dtype)


# ------------------------------------------------------------------------------------------------------------------ rules
def products(v, score, dtype=np.float64):
    """v [K, ...], score [K] -> score_k / (1 + exp(-v_k)) in `dtype`, -inf where proposal k does not hold the pixel"""
    v = np.asarray(v, dtype)
    s = np.asarray(score, dtype).reshape((-1,) + (1,) * (v.ndim - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        p = (s / (dtype(1) + np.exp(-v).astype(dtype))).astype(dtype)
    return np.where(v > 0, p, -np.inf)


def index_from_values(v, score=None, rule="rank", dtype=np.float64):
    """v [K, T, oh, ow] -> uint8 labels [T, oh, ow] by the definition of the module docstring"""
    hold = v > 0                                                    # NaN > 0 and -0.0 > 0 are False
    any_ = hold.any(axis=0)
    if rule == "rank":
        first = np.argmax(hold, axis=0)
    elif rule == "prob":
        first = np.argmax(products(v, score, dtype), axis=0)       # argmax returns the first of equal maxima: ties to the lower k
    else:
        raise ValueError(rule)
    return np.where(any_, first + 1, 0).astype(np.uint8)


def planes_of(ml, dims, query):
    """pixel-major logits [T*hm*wm, ldq] -> the selected planes [K, T, hm, wm]"""
    T, hm, wm = dims
    return np.ascontiguousarray(np.asarray(ml)[:, np.asarray(query)].T.reshape(len(query), T, hm, wm))


def reference_index(ml, dims, padded, img_size, out_size, query, score=None, rule="rank", dtype=np.float64):
    return index_from_values(two_stage(planes_of(ml, dims, query), padded, img_size, out_size, dtype), score, rule, dtype)


# ------------------------------------------------------------------------------------------------------------------ bands
def mask_band(planes, dims, padded, out_size):
    """band_v of the module docstring, from the inputs alone; planes [..., hm, wm]"""
    T, hm, wm = dims
    planes = np.asarray(planes, np.float64)
    D = max(float(np.abs(np.diff(planes, axis=-2)).max()) if hm > 1 else 0.0, float(np.abs(np.diff(planes, axis=-1)).max()) if wm > 1 else 0.0)
    A = float(np.abs(planes).max())
    C = max(*padded, *out_size)
    return 2.0 ** -24 * (max(4 * C, 12 * max(hm, wm)) * D + 16 * A)


def prob_bound(band_v, score):
    """bound_p of the module docstring"""
    return float(np.max(np.abs(score))) * (band_v / 4 + EXP_ALLOWANCE * 2.0 ** -24)


def excluded(v64, band_v, score=None, rule="rank"):
    """bool [T, oh, ow]: the pixels whose label float32 may decide differently (module docstring)"""
    near = np.abs(v64) < band_v
    if rule == "rank":
        maybe = v64 > -band_v                                       # float32 could see k holding
        kstar = np.argmax(maybe, axis=0)
        return maybe.any(axis=0) & np.take_along_axis(near, kstar[None], axis=0)[0]
    cand = v64 > -band_v                                            # float32 could see k holding
    s = np.asarray(score, np.float64).reshape((-1,) + (1,) * (v64.ndim - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.where(cand, s / (1.0 + np.exp(-v64)), -np.inf)
    order = np.argsort(-q, axis=0, kind="stable")[:2]               # best, second best (ties: lower k first)
    best = order[0]
    unsure = cand.any(axis=0) & np.take_along_axis(near, best[None], axis=0)[0]
    if q.shape[0] == 1:
        return unsure
    qb, qs = np.take_along_axis(q, best[None], axis=0)[0], np.take_along_axis(q, order[1][None], axis=0)[0]
    sc = np.asarray(score, np.float64)
    thr = (sc[best] + sc[order[1]]) * (band_v / 4 + EXP_ALLOWANCE * 2.0 ** -24)      # each product moves by its own score's bound
    with np.errstate(invalid="ignore"):
        close = np.isfinite(qs) & (qb - qs < thr)
    return unsure | close


def excluded_wide(v64, band_v, score):
    """the prob rule's exclusion as first stated (any selected |v_k| < band_v, or the two best holders closer than 2 * bound_p):
    a superset of excluded(..., rule="prob"), kept so that the CPU tests can assert the inclusion"""
    p = products(v64, score)
    wide = (np.abs(v64) < band_v).any(axis=0)
    if p.shape[0] > 1:
        top2 = -np.partition(-p, 1, axis=0)[:2]
        with np.errstate(invalid="ignore"):
            wide |= np.isfinite(top2[1]) & (top2[0] - top2[1] < 2 * prob_bound(band_v, score))
    return wide


# ------------------------------------------------------------------------------------------------------------------ inputs
def _cubic_w(t, A=-0.75):
    """the four cubic-convolution weights (A = -0.75, as torch's bicubic) of a fractional offset t"""
    t = np.asarray(t, np.float64)
    w0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
    w1 = ((A + 2) * t - (A + 3)) * t * t + 1
    w2 = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1
    w3 = ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A
    return np.stack([w0, w1, w2, w3])


def _cubic_axis(x, n, axis):
    """bicubic along one axis with align_corners=True and the border replicated"""
    m = x.shape[axis]
    pos = np.arange(n) * ((m - 1) / (n - 1) if n > 1 else 0.0)
    i = np.floor(pos).astype(np.int64)
    w = _cubic_w(pos - i)
    out = 0.0
    for j in range(4):
        idx = np.clip(i - 1 + j, 0, m - 1)
        shape = [1] * x.ndim
        shape[axis] = n
        out = out + np.take(x, idx, axis=axis) * w[j].reshape(shape)
    return out


def smooth_logits(rng, n, hm, wm, amp=3.0):
    """n smooth two-signed float32 maps [n, hm, wm]: a 6 x 6 normal grid times amp, bicubic (align_corners=True) to (hm, wm) -- the
    construction of `_smooth_logits` of tests/test_gpu_forward_c4.py, on the host"""
    c = rng.standard_normal((n, 6, 6)) * amp
    return _cubic_axis(_cubic_axis(c, hm, 1), wm, 2).astype(np.float32)


# geometry rows: name -> (T, hm, wm, padded, img, out)
GEOMETRIES = {
    "two_stage": (2, 5, 7, (20, 28), (18, 27), (37, 53)),          # T*oh*ow = 3922, no multiple of 4
    "same": (2, 5, 7, (20, 28), (18, 27), (18, 27)),
    "downscale": (2, 5, 7, (20, 28), (18, 27), (9, 13)),
    "tiles": (2, 5, 7, (20, 28), (18, 27), (70, 150)),             # 5 x 3 tiles of 16 x 64, the last of each axis ragged
}
WIDTHS = {8: 6, 128: 100}                                          # ldq -> Q
KS = (1, 3, 20, 254)
# rows whose K * window exceeds the kernel's 40 KB of LDS: the direct-gather path (asserted on the GPU through
# s2d_infer_index_lds_bytes); SAME and two-stage
DIRECT = {
    "direct_same": (2, 12, 16, (48, 64), (45, 61), (45, 61)),
    "direct_two_stage": (2, 12, 16, (48, 64), (45, 61), (50, 70)),
}


def cases():
    """-> list of case dicts: every geometry x ldq x K, and the direct rows at ldq = 128, K = 254"""
    out = []
    for g, geo in GEOMETRIES.items():
        for ldq, Q in WIDTHS.items():
            for K in KS:
                out.append(dict(name=f"{g}-ldq{ldq}-K{K}", geo=geo, ldq=ldq, Q=Q, K=K))
    for g, geo in DIRECT.items():
        out.append(dict(name=f"{g}-ldq128-K254", geo=geo, ldq=128, Q=100, K=254))
    return out


# The smallest case has 234 pixels, where one excluded pixel is already four times CAP: the cap can hold there only with none.
# The salt of the seeds was taken as the first one at which every case meets CAP under both rules -- a choice made on the float64
# reference alone (test_davis_index_refs_cpu.py asserts it), before any kernel ran.
SEED_SALT = 5
CASES = cases()
CASE_IDS = [c["name"] for c in CASES]


def make_inputs(case):
    """-> (ml f32 [T*hm*wm, ldq], dims, padded, img, out, query int32 [K], score f32 [K]).  The Q columns are smooth fields of amplitude
    3, the pad columns up to ldq are zero; query is a random order of the columns (K > Q: every column, then repeats: a repeated
    proposal holds what its first copy holds and never wins, under either rule); score is 0.8^k: descending as infer_select returns
    it, with a ratio at which the prob rule still overturns the rank rule on a tenth of the pixels (sigmoid(v_a) / sigmoid(v_b) <
    0.8 is common at amplitude 3) while two products within 2 * bound_p of each other stay rare -- with evenly spaced scores the
    best two of a hundred holders are that close on 1e-2 of the pixels, from the reference alone.  Seeded by the case's name, so
    CPU and GPU tests see one input."""
    T, hm, wm, padded, img, out = case["geo"]
    ldq, Q, K = case["ldq"], case["Q"], case["K"]
    rng = np.random.default_rng(hash_name(case["name"]) + SEED_SALT)
    ml = np.zeros((T * hm * wm, ldq), np.float32)
    ml[:, :Q] = smooth_logits(rng, Q * T, hm, wm).reshape(Q, T * hm * wm).T
    query = np.concatenate([rng.permutation(Q) for _ in range(-(-K // Q))])[:K].astype(np.int32)
    score = (0.8 ** np.arange(K)).astype(np.float32)
    return ml, (T, hm, wm), padded, img, out, query, score


def hash_name(name):
    """a stable 32-bit hash (python's own is salted per process)"""
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


# ------------------------------------------------------------------------------------------------------------------ named rows
NAMED_GEO = (2, 5, 7, (20, 28), (18, 27), (37, 53))


def named_inputs(name):
    """-> (ml, dims, padded, img, out, query, score, expected {rule: uint8 [T, oh, ow] or None}) of a named row; ldq = 8.

    all_negative   every selected plane < 0: all zeros
    nan / neg_zero the selected planes are NaN / -0.0 everywhere: nothing holds, all zeros
    nested         proposal 0 (the outer one, score 1/2) is the constant plane +1 in both frames; proposal 1 (the inner one, score
                   1) is the constant +1 in frame 0 and the constant -1 in frame 1, so its holding set lies inside proposal 0's.
                   rank: proposal 0 everywhere (label 1).  prob: in frame 0 the products are sigmoid(1) = 0.73 against
                   sigmoid(1) / 2 = 0.37, so proposal 1 takes the whole of its holding set (label 2), frame 1 stays label 1.  A
                   constant dyadic plane resizes to that constant up to a few ulp in any precision (the weights of a tap pair sum
                   to 1), the scores are dyadic and the margin is 0.37: float32 decides as float64 does.
    equal_products proposals 0 and 1 are the same constant plane +2 with the same score 1/2 (and proposal 2 is +2 with score
                   1/4): the products of 0 and 1 are one float32 number, the lower k wins: label 1 everywhere, both rules."""
    T, hm, wm, padded, img, out = NAMED_GEO
    ml = np.zeros((T * hm * wm, 8), np.float32)
    pl = ml.reshape(T, hm, wm, 8)
    zeros = np.zeros((T,) + tuple(out), np.uint8)
    if name == "all_negative":
        rng = np.random.default_rng(7)
        pl[...] = -np.abs(smooth_logits(rng, 8 * T, hm, wm)).reshape(8, T, hm, wm).transpose(1, 2, 3, 0) - np.float32(0.25)
        query, score, exp = [3, 0, 5], [0.9, 0.5, 0.25], {"rank": zeros, "prob": zeros}
    elif name == "nan":
        pl[...] = np.nan
        query, score, exp = [1, 2], [0.75, 0.5], {"rank": zeros, "prob": zeros}
    elif name == "neg_zero":
        pl[...] = np.float32(-0.0)
        query, score, exp = [1, 2], [0.75, 0.5], {"rank": zeros, "prob": zeros}
    elif name == "nested":
        pl[..., 4] = 1.0
        pl[0, ..., 2] = 1.0
        pl[1, ..., 2] = -1.0
        query, score = [4, 2], [0.5, 1.0]
        prob = np.ones_like(zeros)
        prob[0] = 2
        exp = {"rank": np.ones_like(zeros), "prob": prob}
    elif name == "equal_products":
        pl[..., 1] = 2.0
        pl[..., 6] = 2.0
        pl[..., 3] = 2.0
        query, score, exp = [6, 1, 3], [0.5, 0.5, 0.25], {"rank": np.ones_like(zeros), "prob": np.ones_like(zeros)}
    else:
        raise KeyError(name)
    return ml, (T, hm, wm), padded, img, out, np.asarray(query, np.int32), np.asarray(score, np.float32), exp


NAMED = ("all_negative", "nan", "neg_zero", "nested", "equal_products")


# ------------------------------------------------------------------------------------------------------------------ host selection
def select_proposals(scores, keep_after_nms, max_proposals, score_threshold):
    """the proposal selection of inference_video(index_map=...), restated: scores [N] descending (infer_select's order);
    keep_after_nms: None, or the indices (into the thresholded list) that the NMS kept, ascending.  -> indices into scores"""
    idx = [i for i, s in enumerate(scores) if not s < score_threshold]
    if keep_after_nms is not None:
        idx = [idx[j] for j in keep_after_nms]
    return idx[:max_proposals]
