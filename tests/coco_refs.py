"""An independent numpy / plain-Python restatement of COCO evaluation, written from the definitions (COCOeval.computeIoU,
evaluateImg, accumulate, summarize; maskApi.c bbIou) and not by calling the product's YTVISEval / COCOEval: the second reference of
the COCO evaluator's tests.  Also the named cases the CPU and the GPU tests share: the matching problems (a)-(g) and the
dataset-level cases (h), (i), whose property shows in accumulate."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]


# ------------------------------------------------------------------------------------------------------------------ IoU
def mask_iou(dt, gt, crowd):
    """uint8 masks dt [D, H, W], gt [G, H, W] -> (inter int64 [D, G], area_d [D], area_g [G], iou float64 [D, G]):
    i / (a_d + a_g - i), i / a_d against a crowd, 0 where the denominator is 0"""
    D, G = len(dt), len(gt)
    n = int(np.prod(np.shape(dt)[1:])) if D else int(np.prod(np.shape(gt)[1:])) if G else 0
    d = np.asarray(dt).reshape(D, n).astype(bool)
    g = np.asarray(gt).reshape(G, n).astype(bool)
    ad = d.sum(1).astype(np.int64)
    ag = g.sum(1).astype(np.int64)
    inter, iou = np.zeros((D, G), np.int64), np.zeros((D, G), np.float64)
    for i in range(D):
        for j in range(G):
            n = int(np.count_nonzero(d[i] & g[j]))
            u = int(ad[i]) if crowd[j] else int(ad[i]) + int(ag[j]) - n
            inter[i, j] = n
            iou[i, j] = np.float64(n) / np.float64(u) if u > 0 else 0.0
    return inter, ad, ag, iou


def bb_iou(dt, gt, crowd):
    """[x, y, w, h] float64 boxes -> iou [D, G] in bbIou's operation order"""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    o = np.zeros((len(dt), len(gt)), np.float64)
    for j, G in enumerate(gt):
        ga = G[2] * G[3]
        for i, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i_ = w * h
            u = da if crowd[j] else da + ga - i_
            o[i, j] = i_ / u
    return o


# ------------------------------------------------------------------------------------------------------------ evaluateImg
def evaluate_img(ious, scores, dt_areas, dt_ids, gt_ids, gt_areas, gt_crowd, rng, max_det=100, thrs=IOU_THRS):
    """one (image[, category]) at one area range.  Detections in result order, ground truths in document order, ious [D, G] in
    those orders.  -> the evaluateImg dict (rows in descending score order, columns in sorted ground-truth order), None if both
    are empty"""
    D, G = len(scores), len(gt_ids)
    if D == 0 and G == 0:
        return None
    ious = np.asarray(ious, np.float64).reshape(D, G)
    lo, hi = rng
    ig = [bool(gt_crowd[j]) or gt_areas[j] < lo or gt_areas[j] > hi for j in range(G)]
    gorder = [j for j in range(G) if not ig[j]] + [j for j in range(G) if ig[j]]
    dorder = sorted(range(D), key=lambda i: -scores[i])[:max_det]          # sorted() is stable
    T, Dk = len(thrs), len(dorder)
    dtm, gtm, dti = np.zeros((T, Dk)), np.zeros((T, G)), np.zeros((T, Dk), bool)
    for ti, t in enumerate(thrs):
        taken = {}
        for r, d in enumerate(dorder):
            best, m = min(t, 1 - 1e-10), None
            for k, j in enumerate(gorder):
                if k in taken and not gt_crowd[j]:
                    continue
                if m is not None and not ig[gorder[m]] and ig[j]:
                    break
                if ious[d, j] < best:
                    continue
                best, m = ious[d, j], k
            if m is None:
                dti[ti, r] = dt_areas[d] < lo or dt_areas[d] > hi
                continue
            taken[m] = r
            dtm[ti, r] = gt_ids[gorder[m]]
            gtm[ti, m] = dt_ids[d]
            dti[ti, r] = ig[gorder[m]]
    return {"dtIds": [dt_ids[d] for d in dorder], "gtIds": [gt_ids[j] for j in gorder], "dtMatches": dtm, "gtMatches": gtm,
            "dtScores": [scores[d] for d in dorder], "gtIgnore": np.array([int(ig[j]) for j in gorder], np.int64), "dtIgnore": dti}


CELL_KEYS = ("dtIds", "gtIds", "dtMatches", "gtMatches", "dtScores", "gtIgnore", "dtIgnore")


def cells_equal(a, b):
    """two evaluateImg dicts (or None) agree on every array"""
    if a is None or b is None:
        return a is None and b is None
    return all(np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)) for k in CELL_KEYS)


# ------------------------------------------------------------------------------------------------------------- accumulate
def accumulate(cells, K, A, n_img, max_dets=(1, 10, 100), thrs=IOU_THRS):
    """cells: evaluateImg dicts in (category, area range, image) order, None for an empty one -> (precision [T, R, K, A, M],
    recall [T, K, A, M])"""
    T, R, M = len(thrs), len(REC_THRS), len(max_dets)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            E = [e for e in cells[(k * A + a) * n_img:(k * A + a + 1) * n_img] if e is not None]
            if not E:
                continue
            for m, md in enumerate(max_dets):
                sc = np.array([s for e in E for s in e["dtScores"][:md]], np.float64)
                order = np.argsort(-sc, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, :md] for e in E], 1)[:, order]
                dti = np.concatenate([e["dtIgnore"][:, :md] for e in E], 1)[:, order]
                npig = sum(int(np.count_nonzero(np.asarray(e["gtIgnore"]) == 0)) for e in E)
                if npig == 0:
                    continue
                for t in range(T):
                    tps = np.cumsum((dtm[t] != 0) & ~dti[t].astype(bool)).astype(np.float64)
                    fps = np.cumsum((dtm[t] == 0) & ~dti[t].astype(bool)).astype(np.float64)
                    nd = len(tps)
                    rc = tps / npig
                    pr = tps / (fps + tps + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    for ri, rt in enumerate(REC_THRS):
                        pos = int(np.searchsorted(rc, rt, side="left"))
                        if pos < nd:
                            q[ri] = pr[pos]
                    precision[t, :, k, a, m] = q
    return precision, recall


def stats12(precision, recall, max_dets=(1, 10, 100), thrs=IOU_THRS):
    """AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl: means over the entries > -1, -1 if there is none"""
    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    last = len(max_dets) - 1
    t50, t75 = np.where(thrs == .5)[0], np.where(thrs == .75)[0]             # the entries that ARE .5 / .75, if any
    out = [mean(precision[:, :, :, 0, last]), mean(precision[t50][:, :, :, 0, last]), mean(precision[t75][:, :, :, 0, last])]
    out += [mean(precision[:, :, :, a, last]) for a in (1, 2, 3)]
    out += [mean(recall[:, :, 0, m]) for m in range(len(max_dets))]
    out += [mean(recall[:, :, a, last]) for a in (1, 2, 3)]
    return np.array(out)


def evaluate_dataset(images, cat_ids, use_cats=False, max_dets=(1, 10, 100)):
    """images: in ascending image-id order, each {"dets": [{"id", "score", "cat", "area"}] in result order, "gts": [{"id", "cat",
    "crowd", "area"}] in document order, "ious": [D, G]} -> (cells, precision, recall, stats)"""
    cats = sorted(cat_ids) if use_cats else [None]
    cells = []
    for cat in cats:
        for rng in AREA_RNG:
            for im in images:
                if cat is None:                                            # pooled: grouped by category in sorted order
                    di = [i for c in sorted(cat_ids) for i, d in enumerate(im["dets"]) if d["cat"] == c]
                    gi = [j for c in sorted(cat_ids) for j, g in enumerate(im["gts"]) if g["cat"] == c]
                else:
                    di = [i for i, d in enumerate(im["dets"]) if d["cat"] == cat]
                    gi = [j for j, g in enumerate(im["gts"]) if g["cat"] == cat]
                ious = np.asarray(im["ious"], np.float64).reshape(len(im["dets"]), len(im["gts"]))[np.ix_(di, gi)] \
                    if di and gi else np.zeros((len(di), len(gi)))
                d, g = [im["dets"][i] for i in di], [im["gts"][j] for j in gi]
                cells.append(evaluate_img(ious, [x["score"] for x in d], [x["area"] for x in d], [x["id"] for x in d],
                                          [x["id"] for x in g], [x["area"] for x in g], [x["crowd"] for x in g], rng, max(max_dets)))
    precision, recall = accumulate(cells, len(cats), len(AREA_RNG), len(images), sorted(max_dets))
    return cells, precision, recall, stats12(precision, recall, sorted(max_dets))


# ------------------------------------------------------------------------------------------------------------ named cases
def named_problems():
    """name -> one matching problem {"ious" [D, G], "scores", "dt_areas", "gt_areas", "crowd", "a" (area range index)}: the cases
    (a)-(g) of the COCO evaluator's tests.  Areas default to 2000 (medium)."""
    def prob(ious, scores=None, dt_areas=None, gt_areas=None, crowd=None, a=0):
        ious = np.asarray(ious, np.float64)
        D, G = ious.shape
        return {"ious": ious, "scores": list(scores) if scores is not None else [1.0 - 0.001 * i for i in range(D)],
                "dt_areas": list(dt_areas) if dt_areas is not None else [2000.0] * D,
                "gt_areas": list(gt_areas) if gt_areas is not None else [2000.0] * G, "crowd": list(crowd) if crowd is not None else [0] * G,
                "a": a}
    rng = np.random.default_rng(7)
    P = {
        "a_tie_later_gt_wins": prob([[0.6, 0.6]]),
        "b_iou_equals_half": prob([[1 / 2]]),
        "b_iou_equals_three_quarters": prob([[3 / 4]]),
        "c_crowd_matched_by_three": prob([[0.9], [0.8], [0.7]], crowd=[1]),
        "d_area_ignored_gt_and_break": prob([[0.9, 0.6]], gt_areas=[50000.0, 2000.0], a=2),
        "e_no_detections": prob(np.zeros((0, 3))),
        "e_no_ground_truth": prob(np.zeros((2, 0))),
        "e_neither": prob(np.zeros((0, 0))),
        "f_101_detections": prob(np.clip(rng.integers(0, 21, (101, 2)) / 20.0, 0, 1), scores=[0.5 + 0.001 * ((i * 37) % 101) for i in range(101)]),
        "g_out_of_range_detections": prob([[0.9], [0.1], [0.1]], dt_areas=[5000.0, 5000.0, 500.0], gt_areas=[500.0], a=1),
    }
    return P


def dataset_cases():
    """name -> (problems, number of categories, use_cats): the cases whose property shows in accumulate.  (h): 12 detections, each
    the exact copy of one of 12 ground truths, so recall at maxDets 1 / 10 / 100 is 1/12, 10/12, 1.  (i): category 2's only ground
    truth is a crowd (and it has no detection), so per category its precision and recall stay -1.  Categories are fixed."""
    h = {"ious": np.eye(12), "scores": [0.9 - 0.01 * i for i in range(12)], "dt_areas": [2000.0] * 12, "gt_areas": [2000.0] * 12,
         "crowd": [0] * 12, "a": 0, "dt_cats": [1] * 12, "gt_cats": [1] * 12}
    i = {"ious": np.array([[0.9, 0.8]]), "scores": [0.9], "dt_areas": [2000.0], "gt_areas": [2000.0, 2000.0], "crowd": [0, 1], "a": 0,
         "dt_cats": [1], "gt_cats": [1, 2]}
    return {"h_max_dets_truncation": ([h], 1, False), "i_category_with_only_a_crowd": ([i], 2, True)}


def solve(p, max_det=100):
    """evaluate_img on a named / random problem: detection ids are positions + 1, ground-truth ids positions + 1"""
    D, G = p["ious"].shape
    return evaluate_img(p["ious"], p["scores"], p["dt_areas"], list(range(1, D + 1)), list(range(1, G + 1)), p["gt_areas"], p["crowd"],
                        AREA_RNG[p["a"]], max_det)


def random_problems(n=200, seed=11):
    """n problems with D in 0..100, G in 0..20 and IoUs from a small rational set (ties and threshold hits are frequent)"""
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, 0.1, 0.3, 1 / 2, 0.55, 0.6, 0.65, 0.7, 3 / 4, 0.8, 0.85, 0.9, 0.95, 1.0] + list(IOU_THRS))
    areas = np.array([100.0, 1024.0, 1025.0, 5000.0, 9216.0, 9217.0, 40000.0])
    out = []
    for k in range(n):
        D, G = int(rng.integers(0, 101)), int(rng.integers(0, 21))
        if k % 17 == 0:
            D = 0
        if k % 23 == 0:
            G = 0
        out.append({"ious": rng.choice(vals, (D, G)), "scores": rng.choice(np.arange(1, 40) / 40.0, D).tolist(),
                    "dt_areas": rng.choice(areas, D).tolist(), "gt_areas": rng.choice(areas, G).tolist(),
                    "crowd": (rng.random(G) < 0.15).astype(int).tolist(), "a": int(rng.integers(0, 4))})
    return out


def dataset_from_problems(problems, n_cats=1, seed=3):
    """problems -> one image each: (COCO document with `area` written from gt_areas, {image id: the product's per-image record},
    the same images in evaluate_dataset's form).  Categories 1..n_cats are drawn at random for n_cats > 1, unless the problem fixes
    them ("dt_cats", "gt_cats")."""
    rng = np.random.default_rng(seed)
    doc = {"images": [], "annotations": [], "categories": [{"id": c, "name": str(c)} for c in range(1, n_cats + 1)]}
    product, ref, aid, did = {}, [], 0, 0
    for n, p in enumerate(problems):
        iid = n + 1
        D, G = p["ious"].shape
        doc["images"].append({"id": iid, "height": 480, "width": 640, "file_name": f"{iid}.jpg"})
        gcat = rng.integers(1, n_cats + 1, G).tolist()
        dcat = rng.integers(1, n_cats + 1, D).tolist()
        gcat, dcat = list(p.get("gt_cats", gcat)), list(p.get("dt_cats", dcat))
        gts = []
        for j in range(G):
            aid += 1
            doc["annotations"].append({"id": aid, "image_id": iid, "category_id": gcat[j], "iscrowd": int(p["crowd"][j]),
                                       "area": p["gt_areas"][j]})
            gts.append({"id": aid, "cat": gcat[j], "crowd": int(p["crowd"][j]), "area": p["gt_areas"][j]})
        ids = list(range(did + 1, did + D + 1))
        did += D
        product[iid] = {"dt_ids": ids, "scores": list(p["scores"]), "labels": dcat, "areas": list(p["dt_areas"]), "ious": p["ious"]}
        ref.append({"dets": [{"id": ids[i], "score": p["scores"][i], "cat": dcat[i], "area": p["dt_areas"][i]} for i in range(D)],
                    "gts": gts, "ious": p["ious"]})
    return doc, product, ref
