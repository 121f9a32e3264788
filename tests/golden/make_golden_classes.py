#!/usr/bin/env python3
"""Generate the class-aware golden vectors (NUM_CLASSES > 1) under tests/golden/classes_*.npz by running the reference's own
Python (loaded unmodified through _ref_shim.py) on the seeded inputs of classes_cases.py.  Container-only; re-run with

    python tests/golden/make_golden_classes.py

Fixtures hold the reference's outputs and the torch.rand draws it made; inputs are regenerated from their seeds.  The
reference's topk(sorted=False) leaves the order of the distillation candidates undefined; the harness fixes it as ascending
flat index q*C + c (the library's documented order) by wrapping torch.topk for that one call.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_shim as R  # noqa: E402
import classes_cases as K  # noqa: E402
from make_golden import RandRecorder, _FakeSelf, make_targets, save  # noqa: E402

torch.set_num_threads(8)


def g_loss_and_matcher():
    """criterion.py:227-251 (loss_labels at C classes, labels zeroed) and matcher.py:225-294 (class cost -softmax(C+1)[:, 0])"""
    cr = R.ref("mask2former_video.modeling.criterion")
    mt = R.ref("mask2former_video.modeling.matcher")
    B, Q, T, h, w, H, W, P, ns = K.CRIT_DIMS
    arrs = {}
    for C in K.CLASS_COUNTS:
        logits, masks = K.crit_inputs("loss", C)
        tg = make_targets(K.seed_of("loss", C), 100, ns, T, H, W)
        crit = cr.VideoSetCriterion(C, matcher=None, weight_dict={}, eos_coef=0.1, losses=["labels", "masks"], num_points=P,
                                    oversample_ratio=3.0, importance_sample_ratio=0.75, loss_strategy="masks-only",
                                    distillation_loss_strategy="masks-only")
        ind = [(torch.as_tensor(i), torch.as_tensor(j)) for i, j in K.loss_indices(C)]
        ll = crit.loss_labels({"pred_logits": torch.from_numpy(logits), "pred_masks": torch.from_numpy(masks)}, tg, ind,
                              float(sum(ns)), False)
        arrs[f"loss_ce_{C}"] = np.float32(ll["loss_ce"])

        logits, masks = K.crit_inputs("matcher", C)
        seed = K.seed_of("matcher", C)
        tg = make_targets(seed, 100, ns, T, H, W)
        m = mt.VideoHungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=5.0, num_points=P)
        with RandRecorder(seed) as rr:
            idx = m({"pred_logits": torch.from_numpy(logits), "pred_masks": torch.from_numpy(masks)}, tg)
        for b in range(B):
            arrs[f"m{C}_coords{b}"] = rr.log[b]
            arrs[f"m{C}_i{b}"] = idx[b][0]
            arrs[f"m{C}_j{b}"] = idx[b][1]
    save("classes_criterion", **arrs)


class _AscendingTopk:
    """torch.topk(sorted=False) -> the same set, in ascending index order"""

    def __enter__(self):
        self._orig = torch.topk
        orig = self._orig

        def fn(x, k, *a, sorted=True, **kw):
            v, i = orig(x, k, *a, sorted=True, **kw)
            if not sorted:
                i, o = torch.sort(i)
                v = v[o]
            return v, i

        torch.topk = fn
        torch.Tensor.topk = lambda self_, k, *a, **kw: fn(self_, k, *a, **kw)
        return self

    def __exit__(self, *a):
        torch.topk = self._orig
        del torch.Tensor.topk


def g_kd():
    """prepare_distillation_targets (kd_video_maskformer_model.py:418-528): flat top-K over Q*C, threshold, optional label-aware
    NMS; a threshold below 0.5 so that one query gives several targets"""
    kd = R.ref("mask2former_video.kd_video_maskformer_model")
    B, Q, T, h, w, Hp, Wp, npd, thr, nms_thr = K.KD_DIMS
    arrs = {}
    for C in K.CLASS_COUNTS:
        cls, masks = K.kd_inputs(C)
        fs = _FakeSelf()
        fs.teacher = [None, _FakeSelf()]
        fs.teacher[1].num_classes = C
        fs.device = torch.device("cpu")
        fs.num_queries = Q
        fs.num_predictions_distillation = npd
        fs.num_frames = T
        fs.nms_threshold = nms_thr
        images = _FakeSelf()
        images.tensor = torch.zeros(B * T, 3, Hp, Wp)
        for nms in (False, True):
            with _AscendingTopk():
                out = kd.KDVideoMaskFormer.prepare_distillation_targets(
                    fs, {"pred_logits": torch.from_numpy(cls), "pred_masks": torch.from_numpy(masks)}, images, None, nms=nms,
                    score_threshold=thr)
            tag = f"{C}_{int(nms)}"
            for b in range(B):
                # the candidates in order (flat index ascending, score >= thr among the top npd), then the kept subsequence
                sc = F.softmax(torch.from_numpy(cls[b]), -1)[:, :-1].flatten()
                top = torch.sort(torch.topk(sc, npd).indices).values
                cand = [int(i) for i in top if sc[i] >= thr]
                up = F.interpolate(torch.from_numpy(masks[b]), size=(Hp, Wp), mode="bilinear", align_corners=False) > 0
                labels = out[b]["labels"].tolist()
                got, j = [], 0
                for k in range(len(labels)):
                    while not (cand[j] % C == labels[k] and torch.equal(up[cand[j] // C], out[b]["masks"][k])):
                        j += 1
                    got.append(cand[j])
                    j += 1
                arrs[f"kd{tag}_n{b}"] = len(labels)
                arrs[f"kd{tag}_q{b}"] = np.array([i // C for i in got], np.int64)
                arrs[f"kd{tag}_l{b}"] = np.array(labels, np.int64)
                arrs[f"kd{tag}_masks{b}"] = np.packbits(out[b]["masks"].numpy().astype(np.uint8), axis=-1)
                if not nms:
                    assert len(set(i // C for i in got)) < len(got), "the case must give a query two pseudo targets"
            print(f"    kd C={C} nms={nms}: kept {[int(arrs[f'kd{tag}_n{b}']) for b in range(B)]}")
    save("classes_kd", **arrs)


def g_inference():
    """inference_video (:530-610): sorted top-K over Q*C with labels from the flat index, optional label-aware NMS"""
    kd = R.ref("mask2former_video.kd_video_maskformer_model")
    Q, Kp, T, h, w, Hp, Wp, ih, iw, oh, ow, nms_thr = K.INFER_DIMS
    arrs = {}
    for C in K.CLASS_COUNTS:
        cls, masks = K.infer_inputs(C)
        for nms in (False, True):
            fs = _FakeSelf()
            fs.teacher = [None, _FakeSelf()]
            fs.teacher[1].num_classes = C
            fs.device = torch.device("cpu")
            fs.num_queries = Q
            fs.num_predictions_inference = Kp
            fs.use_nms, fs.nms_threshold = nms, nms_thr
            up = F.interpolate(torch.from_numpy(masks), size=(Hp, Wp), mode="bilinear", align_corners=False)
            out = kd.KDVideoMaskFormer.inference_video(fs, torch.from_numpy(cls), up, (ih, iw), oh, ow)
            tag = f"{C}_{int(nms)}"
            n = len(out["pred_scores"])
            arrs[f"inf{tag}_scores"] = np.array(out["pred_scores"], np.float32)
            arrs[f"inf{tag}_labels"] = np.array(out["pred_labels"], np.int64)
            arrs[f"inf{tag}_out"] = np.packbits(torch.stack(out["pred_masks"]).numpy().astype(np.uint8), axis=-1)
            print(f"    inference C={C} nms={nms}: kept {n} of {Kp}")
    save("classes_inference", **arrs)


if __name__ == "__main__":
    if not R.available():
        sys.exit("the reference tree is not available")
    R.install()
    g_loss_and_matcher()
    g_kd()
    g_inference()
