"""Seeded inputs of the class-aware fixtures (make_golden_classes.py) shared with the tests that read them.  Data only."""
import numpy as np

from s2d_amd.utils import synth

LARGE_C = 1203                 # an LVIS-sized vocabulary
CLASS_COUNTS = (40, LARGE_C)

# criterion / matcher shapes (matcher_small's): B, Q, T, h, w, H, W, P, ns
CRIT_DIMS = (2, 16, 2, 16, 24, 64, 96, 256, [3, 5])
# distillation targets: B, Q, T, h, w, Hp, Wp, NUM_PREDICTIONS_DISTILLATION, SCORE_THRESHOLD_DISTILLATION, nms threshold
KD_DIMS = (2, 16, 2, 16, 24, 64, 96, 20, 0.3, 0.5)
# inference: Q, K, T, h, w, Hp, Wp, ih, iw, oh, ow, nms threshold
INFER_DIMS = (16, 10, 2, 16, 24, 64, 96, 60, 90, 48, 70, 0.5)


def seed_of(kind, C):
    return {"loss": 301, "matcher": 401, "kd": 501, "infer": 601}[kind] + (0 if C == 40 else 1)


def class_logits(seed, lead, C):
    """[*lead, C+1] logits: normal(0, 2) background with a few confident classes per query.  Per query one of: a single strong
    class, two classes sharing the mass (both above 0.3: one query -> two pseudo targets), or nothing strong."""
    rng = synth.rng_for(seed, 11)
    cls = rng.normal(0.0, 2.0, tuple(lead) + (C + 1,)).astype(np.float32)
    flat = cls.reshape(-1, C + 1)
    for r in range(flat.shape[0]):
        kind = rng.integers(3)
        a, b = rng.choice(C, 2, replace=False)
        if kind == 0:
            flat[r, a] = np.float32(rng.uniform(9.0, 14.0))
        elif kind == 1:
            v = np.float32(rng.uniform(10.0, 13.0))
            flat[r, a] = v
            flat[r, b] = v - np.float32(rng.uniform(0.05, 0.6))
    return cls


def query_masks(seed, Q, T, h, w, dup):
    """[Q,T,h,w] soft-ellipse mask logits; queries in `dup` (q, src, shift) repeat src's mask slightly shifted"""
    rng = synth.rng_for(seed, 12)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    par = [(rng.uniform(0.25 * h, 0.75 * h), rng.uniform(0.25 * w, 0.75 * w), rng.uniform(0.15 * h, 0.3 * h),
            rng.uniform(0.15 * w, 0.3 * w), rng.uniform(-0.6, 0.6, (T, 2))) for _ in range(Q)]
    for q, src, sh in dup:
        cy, cx, ry, rx, dr = par[src]
        par[q] = (cy + sh, cx - sh, ry, rx, dr)
    masks = np.empty((Q, T, h, w), np.float32)
    for q in range(Q):
        cy, cx, ry, rx, dr = par[q]
        for t in range(T):
            d = np.sqrt(((yy - cy - dr[:t + 1, 0].sum()) / ry) ** 2 + ((xx - cx - dr[:t + 1, 1].sum()) / rx) ** 2)
            masks[q, t] = (1.0 - d) * 4.0 + rng.normal(0, 0.05, (h, w)).astype(np.float32)
    return masks


KD_DUP = [(3, 1, 0.3), (7, 5, 0.4), (12, 10, 0.2)]
INFER_DUP = [(2, 0, 0.3), (9, 8, 0.2), (14, 13, 0.4)]


def with_shared_labels(cls, dup):
    """duplicated masks also share their class logits (minus a small no-object bump), so that label-aware NMS fires"""
    cls = cls.copy()
    for q, src, _ in dup:
        cls[..., q, :] = cls[..., src, :]
        cls[..., q, -1] += np.float32(0.05) * (q + 1)
    return cls


def kd_inputs(C):
    B, Q, T, h, w = KD_DIMS[:5]
    seed = seed_of("kd", C)
    cls = with_shared_labels(class_logits(seed, (B, Q), C), KD_DUP)
    masks = np.stack([query_masks(seed + 10 * b, Q, T, h, w, KD_DUP) for b in range(B)])
    return cls, masks


def infer_inputs(C):
    Q, K, T, h, w = INFER_DIMS[:5]
    seed = seed_of("infer", C)
    return with_shared_labels(class_logits(seed, (Q,), C), INFER_DUP), query_masks(seed, Q, T, h, w, INFER_DUP)


def crit_inputs(kind, C):
    """(class logits [B,Q,C+1], mask logits [B,Q,T,h,w]) of the loss / matcher cases"""
    B, Q, T, h, w = CRIT_DIMS[:5]
    seed = seed_of(kind, C)
    return class_logits(seed, (B, Q), C), synth.smooth_logits(seed, 2, (B, Q, T), (h, w))


def loss_indices(C):
    """matched (query, target) pairs of the loss case"""
    B, Q = CRIT_DIMS[:2]
    rng = np.random.default_rng(seed_of("loss", C))
    out = []
    for n in CRIT_DIMS[8]:
        out.append((np.sort(rng.choice(Q, n, replace=False)), rng.permutation(n)))
    return out
