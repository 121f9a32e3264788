"""References and constructed inputs of tests/test_gpu_classes_c4.py (the class-aware kernels at Q = 100, B = 2), and the checks on them
that need no GPU: every input decides like float64.

The selections (ops.kd_targets at C1 > 2, ops.infer_select) are discrete, so their inputs are built, not drawn: a case names the
softmax scores it wants at chosen flat indices q*C + c (`hot`), logits_from_scores() takes the logarithm of a probability table that
holds them, and every other foreground score of a row shares a mass of 0.01 (the rest goes to "no object").  The designed scores form
ladders whose steps are far wider than the score tolerance of the GPU tests (rtol 1e-5); the tests below assert, on the float64 softmax
of the float32 logits, that
  * the K + 1 largest scores of a clip are pairwise apart by at least 10 x that tolerance (GAP, relative) -- or exactly equal, which
    is allowed only between bit-identical logit rows (the tie rule decides those: lower flat index first);
  * no score of a clip lies within GAP (relative) of the threshold;
  * the float32 restatement of each reference (plain torch float32 softmax, stable sort) selects the same sets in the same order.
A failure here means the inputs, not a kernel, are at fault.

The reference statement of the distillation selection is the reference model's prepare_distillation_targets: float64 softmax without the
last column, flattened q*C + c; the K = min(topk, Q*C) largest (equal scores: lower flat index first); of those the ones with
score >= thr; emitted in ascending flat index; truncated to Nmax; count = min(kept, Nmax).

The mask logits of the kd cases (kd_mask_logits) are smooth fields with whole planes shifted until no float64 bilinear value of any
plane lies within 4 x the sign band of tests/test_gpu_forward_c4.py (2^-20 x the largest logit) of zero: the planes are then compared
on every element."""
import functools

import numpy as np
import pytest
import torch

B, Q, T, HM, WM, H, W = 2, 100, 2, 16, 24, 64, 96
NL, P = 10, 256
SCORE_RTOL = 1e-5                   # tolerance of a selected score (tests/test_gpu_classes.py, tests/test_gpu_eval_720p.py)
GAP = 10 * SCORE_RTOL               # least relative distance of two deciding scores, and of any score from thr
BG_MASS = 0.01                      # foreground mass of a row that is not designed
ROW_CAP = 0.93                      # designed scores of one row sum to at most this
SIGN_BAND = 2.0 ** -20              # tests/test_gpu_forward_c4._BAND


# --------------------------------------------------------------------------- builders
def ladder(top, step, n):
    return [top - step * j for j in range(n)]


def logits_from_scores(Qn, C, hot, rng):
    """hot {(q, c): score} -> float32 [Qn, C + 1] logits whose softmax holds the designed scores (up to the rounding of the logits)"""
    p = np.zeros((Qn, C + 1), np.float64)
    share = np.exp(0.3 * rng.standard_normal((Qn, C)))
    taken = np.zeros((Qn, C), bool)
    for (q, c) in hot:
        taken[q, c] = True
    for q in range(Qn):
        free = ~taken[q]
        if free.any():
            p[q, :C][free] = BG_MASS * share[q][free] / share[q][free].sum()
    for (q, c), s in hot.items():
        p[q, c] = s
    p[:, C] = 1.0 - p[:, :C].sum(1)
    assert (p[:, C] > 0.04).all() and (p > 0).all()
    return np.log(p).astype(np.float32)


def place(scores, Qn, C, rng, rows=None, flat=None, per_row=3, hot=None):
    """give every score a free (q, c): a random row among those (of `rows`) whose designed scores stay under ROW_CAP and per_row, a
    random free column of it; flat = (lo, hi): only positions with lo <= q*C + c < hi.  Extends and returns `hot`"""
    hot = {} if hot is None else hot
    rows = list(range(Qn)) if rows is None else list(rows)
    lo, hi = (0, Qn * C) if flat is None else flat
    total = {q: sum(s for (r, _), s in hot.items() if r == q) for q in rows}
    count = {q: sum(1 for (r, _) in hot if r == q) for q in rows}
    for s in sorted(scores, reverse=True):
        ok = []
        for q in rows:
            c0, c1 = max(lo - q * C, 0), min(hi - q * C, C)
            if total[q] + s <= ROW_CAP and count[q] < per_row and c1 - c0 > count[q]:
                ok.append((q, c0, c1))
        assert ok, ("no row left for", s)
        q, c0, c1 = ok[rng.integers(len(ok))]
        while True:
            c = int(rng.integers(c0, c1))
            if (q, c) not in hot:
                break
        hot[(q, c)] = s
        total[q] += s; count[q] += 1
    return hot


def _pairs(rng, C, rows, cols=None):
    """eight scores above 0.3 on four rows, two to a row (cases e and f); cols: the admissible columns of each row"""
    scores = [(0.6, 0.31), (0.55, 0.33), (0.5, 0.4), (0.47, 0.36)]
    hot = {}
    for q, (a, b_) in zip(rows, scores):
        lo, hi = (0, C) if cols is None or q not in cols else cols[q]
        ca, cb = rng.choice(np.arange(lo, hi), 2, replace=False)
        hot[(q, int(ca))], hot[(q, int(cb))] = a, b_
    return hot


def _dup_rows(half):
    """[Q/2, C1] -> [Q, C1]: rows 2k and 2k + 1 both row k, bit for bit"""
    return np.repeat(half, 2, axis=0)


@functools.lru_cache(maxsize=None)
def kd_cases():
    """{name: dict(C, topk, thr, Nmax, cls float32 [B, Q, C + 1], ties)} -- the cases a .. j of the module docstring of
    tests/test_gpu_classes_c4.py"""
    out = {}

    def add(name, C, topk, thr, Nmax, clips, ties=False):
        out[name] = dict(C=C, topk=topk, thr=thr, Nmax=Nmax, cls=np.stack(clips), ties=ties)

    def mixed(seed, C, per_row=3):
        """clip 0: 30 scores pass thr 0.3 on 20 rows (more than K = 20, rows with two of the 20 largest: the K-th row best lies below the
        K-th score); clip 1: 12 pass, 16 do not"""
        r = np.random.default_rng(seed)
        h0 = place(ladder(0.6, 0.01, 30), Q, C, r, rows=r.choice(Q, 20, replace=False), per_row=per_row)
        h1 = place(ladder(0.88, 0.04, 12) + ladder(0.28, 0.015, 16), Q, C, r, per_row=per_row)
        return [logits_from_scores(Q, C, h0, r), logits_from_scores(Q, C, h1, r)]

    add("a", 40, 20, 0.3, 20, mixed(1, 40))
    r = np.random.default_rng(2)
    add("b", 40, 128, 0.3, 128, [logits_from_scores(Q, 40, place(ladder(top, 0.006, 136), Q, 40, r), r) for top in (0.903, 0.9015)])
    r = np.random.default_rng(3)
    add("c", 40, 100, 0.3, 16, [logits_from_scores(Q, 40, place(ladder(top, 0.012, 40) + ladder(0.28, 0.004, 64), Q, 40, r), r)
                                for top in (0.9, 0.897)])
    r = np.random.default_rng(4)
    add("d", 40, 20, 0.3, 20, [logits_from_scores(Q, 40, place(ladder(0.28, 0.009, 28), Q, 40, r), r),
                               logits_from_scores(Q, 40, place(ladder(0.9, 0.02, 28), Q, 40, r), r)])
    r = np.random.default_rng(5)
    add("e", 40, 20, 0.3, 20, [logits_from_scores(Q, 40, place(ladder(top, 0.012, 20), Q, 40, r, flat=(0, 3840), hot=_pairs(r, 40, (96, 97, 98, 99))), r)
                               for top in (0.28, 0.277)])
    r = np.random.default_rng(6)
    add("f", 40, 20, 0.3, 20, [logits_from_scores(Q, 40, place(ladder(top, 0.012, 20), Q, 40, r, flat=(256, 4000),
                                                              hot=_pairs(r, 40, (0, 2, 5, 6), cols={6: (0, 16)})), r) for top in (0.28, 0.277)])
    r = np.random.default_rng(7)
    add("g", 40, 21, 0.3, 21, [_dup_rows(logits_from_scores(Q // 2, 40, place(ladder(top, 0.02, 14), Q // 2, 40, r, per_row=2), r))
                               for top in (0.9, 0.895)], ties=True)
    r = np.random.default_rng(8)
    clips = []
    for q, cols in ((6, (14, 15, 17)), (12, (30, 31, 33))):                    # flat 254, 255, 257 and 510, 511, 513
        hot = {(q, c): s for c, s in zip(cols, (0.3, 0.26, 0.23))}
        others = [x for x in range(Q) if x != q]
        clips.append(logits_from_scores(Q, 40, place(ladder(0.8, 0.03, 10) + ladder(0.18, 0.008, 14), Q, 40, r, rows=others, hot=hot), r))
    add("h", 40, 20, 0.2, 20, clips)
    add("i", 1203, 20, 0.3, 20, mixed(9, 1203))
    add("j", 2, 20, 0.3, 20, mixed(10, 2, per_row=2))
    return out


INFER_SHAPES = [(100, 40, 10), (100, 80, 100), (100, 1203, 50), (128, 128, 10), (128, 129, 10), (100, 40, 128)]     # the last: K > Q


@functools.lru_cache(maxsize=None)
def infer_cases():
    """{name: (cls float32 [Q, C + 1], K, ties)}: K + 8 designed scores each; "ties": the duplicated rows of kd case g"""
    out = {}
    for n, (Qn, C, K) in enumerate(INFER_SHAPES):
        r = np.random.default_rng(100 + n)
        M = K + 8
        out[f"{Qn}-{C}-{K}"] = (logits_from_scores(Qn, C, place(ladder(0.9, 0.8 / M, M), Qn, C, r), r), K, False)
    out["ties-100-40-21"] = (kd_cases()["g"]["cls"][0], 21, True)
    return out


# --------------------------------------------------------------------------- references
def flat_scores(cls, dtype=torch.float64):
    """float32 logits [..., Qn, C + 1] (numpy or tensor) -> softmax without the last column, flattened q*C + c: [..., Qn*C] in dtype"""
    t = torch.as_tensor(cls).to(dtype)
    s = torch.softmax(t, -1)[..., :-1]
    return s.reshape(s.shape[:-2] + (-1,))


def kd_select_ref(cls, thr, topk, Nmax, dtype=torch.float64):
    """the reference statement of the module docstring, per clip: dict(count, kept, label, passing)"""
    C = cls.shape[-1] - 1
    s = flat_scores(cls, dtype)
    K = min(int(topk), s.shape[-1])
    out = []
    for b in range(s.shape[0]):
        v, i = torch.sort(s[b], descending=True, stable=True)
        top = i[:K][v[:K] >= torch.tensor(thr, dtype=dtype)]
        sel = top.sort().values
        out.append(dict(count=min(sel.numel(), Nmax), kept=(sel // C)[:Nmax].int(), label=(sel % C)[:Nmax].int(), passing=sel.numel()))
    return out


def infer_select_ref(cls, K, dtype=torch.float64):
    """-> (scores [K], query [K], label [K]): the K largest flat scores in descending order, equal scores lower flat index first"""
    C = cls.shape[-1] - 1
    v, i = torch.sort(flat_scores(cls, dtype), descending=True, stable=True)
    return v[:K], (i[:K] // C).int(), (i[:K] % C).int()


def gap_report(cls, K, thr=None):
    """one clip's float32 logits [Qn, C + 1] -> (least relative gap of distinct neighbours among the K + 1 largest float64 scores, the
    (flat, flat) pairs of exactly equal neighbours among them, least relative distance of any score from thr)"""
    s = flat_scores(cls)
    v, i = torch.sort(s, descending=True, stable=True)
    head, idx = v[:K + 1], i[:K + 1]
    d = (head[:-1] - head[1:]) / head[:-1]
    ties = [(int(idx[k]), int(idx[k + 1])) for k in torch.nonzero(d == 0)[:, 0].tolist()]
    gap = float(d[d > 0].min())
    thr_gap = float(((s - thr).abs() / thr).min()) if thr is not None else float("inf")
    return gap, ties, thr_gap


def assert_ties_are_identical_rows(cls, ties):
    C = cls.shape[-1] - 1
    for f0, f1 in ties:
        assert f0 % C == f1 % C and f0 < f1 and np.array_equal(cls[f0 // C], cls[f1 // C]), (f0, f1)


@functools.lru_cache(maxsize=None)
def kd_mask_logits():
    """-> (mask logits float32 [B, Q, T, HM, WM], their float64 bilinear interpolation > 0 as bool [B, Q, T, H, W], the least
    |float64 value| over the sign band): planes shifted by 2^-6 until the margin is 4 bands"""
    from s2d_amd.utils import synth
    ml = synth.smooth_logits(21, 4, (B * Q * T,), (HM, WM)).astype(np.float32)
    band = SIGN_BAND * (float(np.abs(ml).max()) + 0.5)
    interp = lambda a: torch.nn.functional.interpolate(torch.from_numpy(a).double()[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    v = interp(ml)
    for _ in range(64):
        low = torch.nonzero(v.abs().flatten(1).min(1).values < 4 * band)[:, 0].numpy()
        if not len(low):
            break
        ml[low] += np.float32(2.0 ** -6)
        v[low] = interp(ml[low])
    assert float(np.abs(ml).max()) * SIGN_BAND <= band
    return ml.reshape(B, Q, T, HM, WM), (v > 0).view(B, Q, T, H, W).numpy(), float(v.abs().min()) / band


def pixel_major(ml, ldq):
    """[B, Q, T, h, w] -> [B, T*h*w, ldq] (the layout the kernels read), pad columns NaN"""
    b, q = ml.shape[:2]
    out = np.full((b, ml[0, 0].size, ldq), np.nan, np.float32)
    out[..., :q] = np.moveaxis(ml.reshape(b, q, -1), 1, 2)
    return out


def matcher_inputs(C1):
    """seeded operands of ops.matcher_cost at NL = 10, B = 2, Q = 100, T = 2, 16 x 24 masks, 64 x 96 targets, P = 256, target counts
    [3, 10] -> (class logits [NL,B,Q,C1], mask logits [NL,B,Q,T,HM,WM], targets u8 [B,10,T,H,W], counts, coords [NL,B,P,2])"""
    from s2d_amd.utils import synth
    logits = synth.randn(31, C1, (NL, B, Q, C1), 2.0)
    masks = synth.smooth_logits(31, 1000 + C1, (NL, B, Q, T), (HM, WM)).astype(np.float32)
    ns = [3, 10]
    tgt = np.zeros((B, max(ns), T, H, W), np.uint8)
    for b, n in enumerate(ns):
        tgt[b, :n] = synth.ellipse_targets(31, 2000 + C1 + b, n, T, H, W)[0]
    coords = synth.rng_for(31, 3000 + C1).random((NL, B, P, 2)).astype(np.float32)
    return logits, masks, tgt, np.array(ns, np.int32), coords


def cost_class64(logits):
    """the matcher's class column in float64: -softmax(logits)[..., 0] over all C1 columns"""
    return -torch.softmax(torch.as_tensor(logits).double(), -1)[..., 0].numpy()


CLASS_LOSS_C1 = [3, 41, 81, 1204]
CLASS_LOSS_MATCHES = {"none": [0, 0], "all": [100, 100], "some": [10, 37]}


def class_loss_inputs(C1, n_match, wide=False):
    """-> (logits float32 [B, Q, C1], idx_q int32 [B, maxm], n_match int32 [B]); wide: logits uniform in +-30, so exp(l - max) underflows
    in float32 (below -87.3) for some columns of some rows"""
    rng = np.random.default_rng(1000 * C1 + 10 * sum(n_match) + int(wide))
    logits = (rng.uniform(-30, 30, (B, Q, C1)) if wide else rng.standard_normal((B, Q, C1)) * 2.0).astype(np.float32)
    if wide:
        logits[:, ::7, 0] = 60.0                             # rows whose other columns sit more than 87.3 below the maximum: exp underflows to 0
        logits[:, ::7, 1:] -= 40.0
    maxm = max(max(n_match), 4)
    iq = np.zeros((B, maxm), np.int32)
    for b, n in enumerate(n_match):
        iq[b, :n] = np.sort(rng.choice(Q, n, replace=False))
    return logits, iq, np.array(n_match, np.int32)


def class_loss_ref(logits, iq, nm, w_ce, eos, dtype=torch.float64):
    """(weighted cross-entropy: matched -> class 0, the others -> C1 - 1 with weight eos; d(w_ce * loss) / d logits), through autograd"""
    x = torch.as_tensor(logits).to(dtype).clone().requires_grad_()
    Bn, Qn, C1 = x.shape
    tgt = torch.full((Bn, Qn), C1 - 1, dtype=torch.long)
    for b in range(Bn):
        tgt[b, torch.as_tensor(iq[b, :int(nm[b])]).long()] = 0
    wt = torch.ones(C1, dtype=dtype); wt[-1] = eos
    loss = torch.nn.functional.cross_entropy(x.reshape(-1, C1), tgt.reshape(-1), wt)
    (w_ce * loss).backward()
    return loss.detach(), x.grad


# --------------------------------------------------------------------------- the checks that need no GPU
@pytest.mark.parametrize("name", list("abcdefghij"))
def test_kd_case_decides_like_float64(name):
    case = kd_cases()[name]
    cls, C, thr = case["cls"], case["C"], case["thr"]
    K = min(case["topk"], Q * C)
    assert cls.shape == (B, Q, C + 1) and cls.dtype == np.float32
    r64 = kd_select_ref(cls, thr, case["topk"], case["Nmax"])
    r32 = kd_select_ref(cls, thr, case["topk"], case["Nmax"], torch.float32)
    for b in range(B):
        gap, ties, thr_gap = gap_report(cls[b], K, thr)
        print(f"kd case {name} clip {b}: least gap {gap:.2e}, {len(ties)} exact ties, least distance from thr {thr_gap:.2e}, "
              f"{r64[b]['passing']} selected, count {r64[b]['count']}")
        assert gap >= GAP and thr_gap >= GAP
        assert bool(ties) == case["ties"]
        assert_ties_are_identical_rows(cls[b], ties)
        assert r32[b]["count"] == r64[b]["count"] and r32[b]["passing"] == r64[b]["passing"]
        assert torch.equal(r32[b]["kept"], r64[b]["kept"]) and torch.equal(r32[b]["label"], r64[b]["label"])


def test_kd_cases_reach_what_they_are_for():
    """the property each case exists for, on the float64 reference"""
    cs = kd_cases()
    ref = {n: kd_select_ref(c["cls"], c["thr"], c["topk"], c["Nmax"]) for n, c in cs.items()}
    sel = lambda n, b: (ref[n][b]["kept"].long() * cs[n]["C"] + ref[n][b]["label"].long())
    # a: K <= Q; clip 0 is cut by K, clip 1 by thr; the K-th row best lies below the K-th score (the floor admits candidates of rank >= K)
    assert [r["passing"] for r in ref["a"]] == [20, 12]
    s = flat_scores(cs["a"]["cls"][0])
    rb = s.view(Q, 40).max(1).values.sort(descending=True).values
    assert rb[19] < s.sort(descending=True).values[19] and int((s >= max(0.3, float(rb[19]))).sum()) > 20
    # b: K > Q, nothing truncated
    assert cs["b"]["topk"] > Q and all(100 < r["passing"] <= 128 and r["count"] == r["passing"] for r in ref["b"])
    # c: truncation
    assert all(r["passing"] == 40 and r["count"] == 16 for r in ref["c"])
    # d: an empty clip beside a full one
    assert [r["count"] for r in ref["d"]] == [0, 20]
    # e / f: everything selected in the last, ragged 256-tile / in the first
    for b in range(B):
        assert ref["e"][b]["count"] == 8 and int(sel("e", b).min()) >= 3840
        assert ref["f"][b]["count"] == 8 and int(sel("f", b).max()) < 256
        for n, inside in (("e", lambda f: f >= 3840), ("f", lambda f: f < 256)):
            cand = torch.nonzero(flat_scores(cs[n]["cls"][b]) >= 0.3)[:, 0]
            assert all(inside(int(f)) for f in cand)
    # g: ranks K - 1 and K are one tied pair; the lower flat index is selected, its twin is not
    for b in range(B):
        s = flat_scores(cs["g"]["cls"][b])
        v, i = torch.sort(s, descending=True, stable=True)
        assert v[20] == v[21] and i[20] < i[21] and i[21] - i[20] == 40
        chosen = set(sel("g", b).tolist())
        assert ref["g"][b]["count"] == 21 and int(i[20]) in chosen and int(i[21]) not in chosen
    # h: one query, three labels, across a multiple of 256
    for b, (q, flats) in enumerate(((6, (254, 255, 257)), (12, (510, 511, 513)))):
        chosen = sel("h", b).tolist()
        assert all(f in chosen for f in flats) and ref["h"][b]["kept"].tolist().count(q) == 3
    # i: 470 tiles; j: the smallest class-aware size
    assert cs["i"]["cls"].shape[-1] == 1204 and -(-Q * 1203 // 256) == 470 and cs["j"]["cls"].shape[-1] == 3
    assert [r["passing"] for r in ref["i"]] == [20, 12] and [r["passing"] for r in ref["j"]] == [20, 12]


@pytest.mark.parametrize("name", list(infer_cases()))
def test_infer_case_decides_like_float64(name):
    cls, K, tied = infer_cases()[name]
    gap, ties, _ = gap_report(cls, K)
    print(f"infer case {name}: least gap {gap:.2e}, {len(ties)} exact ties among the first {K + 1}")
    assert gap >= GAP and bool(ties) == tied
    assert_ties_are_identical_rows(cls, ties)
    s64, q64, l64 = infer_select_ref(cls, K)
    s32, q32, l32 = infer_select_ref(cls, K, torch.float32)
    assert torch.equal(q32, q64) and torch.equal(l32, l64)
    assert float(((s32.double() - s64).abs() / s64).max()) < SCORE_RTOL


def test_infer_shapes_sit_on_both_sides_of_the_lds_bound():
    from s2d_amd import ops
    sizes = [q * c for q, c, _ in INFER_SHAPES]
    assert ops.INFER_SELECT_LDS_SCORES in sizes and min(s for s in sizes if s > ops.INFER_SELECT_LDS_SCORES) == 128 * 129


def test_kd_mask_planes_have_no_value_in_the_sign_band():
    ml, ref, margin = kd_mask_logits()
    print(f"kd mask logits: least |float64 bilinear value| is {margin:.1f} sign bands")
    assert margin >= 4.0 and ml.dtype == np.float32 and ref.shape == (B, Q, T, H, W)
    assert 0.2 < ref.mean() < 0.8
    v32 = torch.nn.functional.interpolate(torch.from_numpy(ml).view(-1, 1, HM, WM), size=(H, W), mode="bilinear", align_corners=False)
    assert np.array_equal((v32 > 0).view(B, Q, T, H, W).numpy(), ref)


@pytest.mark.parametrize("C1", [3, 41, 81])
def test_matcher_class_term_restatements_agree(C1):
    logits, masks, tgt, cnt, coords = matcher_inputs(C1)
    assert logits.shape == (NL, B, Q, C1) and masks.shape == (NL, B, Q, T, HM, WM) and coords.shape == (NL, B, P, 2)
    assert cnt.tolist() == [3, 10] and all(tgt[b, :n].reshape(n, -1).any(1).all() for b, n in enumerate(cnt))
    c64 = cost_class64(logits)
    c32 = -torch.softmax(torch.from_numpy(logits), -1)[..., 0].double().numpy()
    assert np.abs(c32 - c64).max() < 1e-6 and c64.min() >= -1.0 and c64.max() < 0.0


@pytest.mark.parametrize("C1", CLASS_LOSS_C1)
def test_class_loss_restatements_agree(C1):
    for key, nm in list(CLASS_LOSS_MATCHES.items()) + [("wide", [10, 37])]:
        logits, iq, n = class_loss_inputs(C1, nm, wide=key == "wide")
        l64, g64 = class_loss_ref(logits, iq, n, 2.0, 0.1)
        l32, g32 = class_loss_ref(logits, iq, n, 2.0, 0.1, torch.float32)
        assert torch.isfinite(l64) and torch.isfinite(g64).all()
        assert abs(float(l32) - float(l64)) <= 1e-5 * abs(float(l64))
        assert float((g32.double() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
        if key == "wide":
            x = torch.from_numpy(logits)
            assert bool((torch.exp(x - x.max(-1, keepdim=True).values) == 0).any())           # float32 exp underflows somewhere


def test_cost64_class_term(oracle):
    """tests/test_gpu_e2e._cost64: at two logits the value it always had, bit for bit (its class column is a float32 softmax widened);
    beyond two, the class column is -softmax64(logits)[:, 0]"""
    from tests.test_gpu_e2e import _cost64
    logits, masks, tgt, cnt, coords = matcher_inputs(3)
    m, t, co = masks[0, 1], tgt[1, :10], coords[0, 1][None]
    two = np.ascontiguousarray(logits[0, 1, :, :2])
    got, scale = _cost64(oracle, two, m, t, co, 1.0, 0.0, 0.0)                # weights (1, 0, 0): the class column itself, exactly
    e = np.exp(two - two.max(-1, keepdims=True))
    old = -np.repeat((e / e.sum(-1, keepdims=True))[:, :1].astype(np.float64), 10, axis=1)
    assert e.dtype == np.float32 and np.array_equal(got, old) and scale > 0
    got3, _ = _cost64(oracle, logits[0, 1], m, t, co, 1.0, 0.0, 0.0)
    np.testing.assert_allclose(got3, np.repeat(cost_class64(logits[0, 1])[:, None], 10, axis=1), rtol=1e-14)       # numpy's float64 against torch's
    assert 0 < np.abs(got3 - (-torch.softmax(torch.from_numpy(logits[0, 1]), -1)[:, :1].double().numpy())).max() < 1e-6      # not the float32 one
