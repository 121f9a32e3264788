"""GPU parity of the class-aware path (NUM_CLASSES > 1, C + 1 logits per query) against the reference's goldens
(tests/golden/make_golden_classes.py) at C = 40 and at an LVIS-sized C = 1203, and bit-equality of the class-aware kernels with
the class-agnostic ones at C = 1."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import golden
from tests.test_gpu_criterion import _dev, make_targets, pad_targets, pixel_major

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))      # classes_cases.py (seeded inputs)


def _indices(C):
    from classes_cases import CRIT_DIMS, loss_indices
    B, Q = CRIT_DIMS[:2]
    maxm = max(CRIT_DIMS[8])
    iq = np.zeros((B, maxm), np.int32); nm = np.zeros(B, np.int32)
    for b, (i, _) in enumerate(loss_indices(C)):
        iq[b, :len(i)], nm[b] = i, len(i)
    return iq, nm


@pytest.mark.parametrize("C", [40, 1203])
def test_class_loss_forward_golden_and_backward_float64(C):
    from classes_cases import crit_inputs
    from s2d_amd import ops
    g = golden("classes_criterion")
    logits, _ = crit_inputs("loss", C)
    iq, nm = _indices(C)
    ce = float(ops.class_loss(_dev(logits), _dev(iq), _dev(nm), 0.1))
    np.testing.assert_allclose(ce, float(g[f"loss_ce_{C}"]), rtol=1e-6)
    # gradient of w_ce * weighted CE against float64 autograd of the same expression
    x = torch.from_numpy(logits).double().requires_grad_()
    B, Q, C1 = logits.shape
    tgt = torch.full((B, Q), C1 - 1, dtype=torch.long)
    for b in range(B):
        tgt[b, torch.from_numpy(iq[b, :nm[b]]).long()] = 0
    wt = torch.ones(C1, dtype=torch.float64); wt[-1] = 0.1
    loss = 2.0 * torch.nn.functional.cross_entropy(x.reshape(-1, C1), tgt.reshape(-1), wt)
    np.testing.assert_allclose(ce, float(loss.detach()) / 2.0, rtol=1e-6)
    loss.backward()
    d = ops.class_loss_backward(_dev(logits), _dev(iq), _dev(nm), 2.0, 0.1).cpu().double().numpy()
    ref = x.grad.numpy()
    np.testing.assert_allclose(d, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())


@pytest.mark.parametrize("C", [40, 1203])
def test_matcher_indices_golden(C):
    from classes_cases import CRIT_DIMS, crit_inputs, seed_of
    from s2d_amd import ops
    g = golden("classes_criterion")
    B, Q, T, h, w, H, W, P, ns = CRIT_DIMS
    logits, masks = crit_inputs("matcher", C)
    tgt, cnt = pad_targets(make_targets(seed_of("matcher", C), 100, ns, T, H, W), max(ns), T, H, W)
    coords = np.stack([g[f"m{C}_coords{b}"][0] for b in range(B)])[None]
    Cm = ops.matcher_cost(_dev(pixel_major(masks)[None]), _dev(logits[None]), _dev(tgt), _dev(cnt), (Q, T, h, w), P,
                          (2.0, 5.0, 5.0), coords=_dev(coords))
    iq, it, nm = (t.cpu().numpy() for t in ops.lsap(Cm, _dev(cnt), B))
    for b in range(B):
        k = min(Q, ns[b])
        assert nm[b] == k
        np.testing.assert_array_equal(iq[b, :k], g[f"m{C}_i{b}"])
        np.testing.assert_array_equal(it[b, :k], g[f"m{C}_j{b}"])


@pytest.mark.parametrize("nms", [False, True])
@pytest.mark.parametrize("C", [40, 1203])
def test_kd_targets_golden(C, nms):
    from classes_cases import KD_DIMS, kd_inputs
    from s2d_amd import ops
    from s2d_amd.modeling.meta_arch import KDVideoMaskFormer
    g = golden("classes_kd")
    B, Q, T, h, w, Hp, Wp, npd, thr, nms_thr = KD_DIMS
    cls, masks = kd_inputs(C)
    Nmax = min(npd, Q * C)
    tgt, cnt, kept, ne, lab = ops.kd_targets(_dev(cls), _dev(pixel_major(masks)), (Q, T, h, w), Hp, Wp, Nmax, thr, npd,
                                             want_labels=True)
    if nms:
        fake = KDVideoMaskFormer.__new__(KDVideoMaskFormer)
        fake.nms_threshold = nms_thr
        tgt, cnt, ne = KDVideoMaskFormer._kd_nms(fake, tgt, cnt, ne, kept, lab)
    tag = f"{C}_{int(nms)}"
    cnt, kept, lab, tgt = cnt.cpu().numpy(), kept.cpu().numpy(), lab.cpu().numpy(), tgt.cpu().numpy()
    for b in range(B):
        n = int(g[f"kd{tag}_n{b}"])
        assert cnt[b] == n
        np.testing.assert_array_equal(kept[b, :n], g[f"kd{tag}_q{b}"])
        np.testing.assert_array_equal(lab[b, :n], g[f"kd{tag}_l{b}"])
        np.testing.assert_array_equal(np.packbits(tgt[b, :n], axis=-1), g[f"kd{tag}_masks{b}"])
    if not nms:
        assert any(len(set(kept[b, :cnt[b]].tolist())) < cnt[b] for b in range(B))     # one query, several labels


@pytest.mark.parametrize("nms", [False, True])
@pytest.mark.parametrize("C", [40, 1203])
def test_inference_video_golden(C, nms):
    from classes_cases import INFER_DIMS, infer_inputs
    from s2d_amd.modeling.postprocess import inference_video
    from tests.test_gpu_infer import pixel_major as pm_infer
    g = golden("classes_inference")
    Q, K, T, h, w, Hp, Wp, ih, iw, oh, ow, thr = INFER_DIMS
    cls, masks = infer_inputs(C)
    out = inference_video(torch.from_numpy(cls).cuda(), pm_infer(masks), (T, h, w), (Hp, Wp), (ih, iw), (oh, ow), K, nms, thr)
    tag = f"{C}_{int(nms)}"
    np.testing.assert_allclose(out["pred_scores"], g[f"inf{tag}_scores"], rtol=1e-6)
    assert out["pred_labels"] == g[f"inf{tag}_labels"].tolist()
    got = np.packbits(torch.stack(out["pred_masks"]).numpy().astype(np.uint8), axis=-1)
    np.testing.assert_array_equal(got, g[f"inf{tag}_out"])


def test_large_vocabulary_selection_matches_torch_topk():
    """the multi-workgroup select at Q = 100, C = 1203 (beyond the single-workgroup LDS bound) against torch.topk"""
    from s2d_amd import ops
    rng = np.random.default_rng(5)
    Q, C, K = 100, 1203, 50
    cls = rng.normal(0, 3, (Q, C + 1)).astype(np.float32)
    s, q, l = (t.cpu().numpy() for t in ops.infer_select(_dev(cls), K))
    ref = torch.softmax(torch.from_numpy(cls).double(), -1)[:, :-1].flatten()      # float64: fp32 sums of 1204 terms differ by order
    v, i = torch.topk(ref, K)
    np.testing.assert_allclose(s, v.numpy(), rtol=1e-5)
    np.testing.assert_array_equal(q * C + l, i.numpy())


def test_class_aware_kernels_equal_class_agnostic_ones_at_one_class():
    """C1 = 2 through the class-aware entry points gives the class-agnostic kernels' bits"""
    from s2d_amd import ops
    from s2d_amd._lib import lib
    from s2d_amd.ops import _stream
    rng = np.random.default_rng(9)
    B, Q, T, h, w, H, W, P = 2, 16, 2, 16, 24, 64, 96, 256
    cls = _dev(rng.normal(0, 2, (B, Q, 2)).astype(np.float32))
    iq = _dev(np.stack([np.sort(rng.choice(Q, 5, replace=False)) for _ in range(B)]).astype(np.int32))
    nm = _dev(np.array([5, 3], np.int32))
    # class loss forward / backward
    a = torch.zeros(1, device="cuda"); b = torch.zeros(1, device="cuda")
    lib().call("s2d_class_loss_f32", cls, iq, nm, B, Q, 5, 0.1, a, _stream())
    lib().call("s2d_class_loss_c_f32", cls, 2, iq, nm, B, Q, 5, 0.1, b, _stream())
    assert torch.equal(a, b)
    da, db = torch.empty_like(cls), torch.empty_like(cls)
    lib().call("s2d_class_loss_backward_f32", cls, iq, nm, B, Q, 5, 0.1, 2.0, da, _stream())
    lib().call("s2d_class_loss_backward_c_f32", cls, 2, iq, nm, B, Q, 5, 0.1, 2.0, db, _stream())
    assert torch.equal(da, db)
    # matcher cost
    from s2d_amd.utils import synth
    masks = synth.smooth_logits(3, 2, (B, Q, T), (h, w))
    tgt, cnt = pad_targets(make_targets(3, 100, [3, 5], T, H, W), 5, T, H, W)
    ml, tg, cn = _dev(pixel_major(masks)[None]), _dev(tgt), _dev(cnt)
    Ca = ops.matcher_cost(ml, cls[None], tg, cn, (Q, T, h, w), P, (2.0, 5.0, 5.0), seed=4)
    ws = torch.empty(lib().call("s2d_matcher_c_workspace_floats", 1, B, Q, T, P, H, W), device="cuda")
    Cb = torch.empty_like(Ca)
    lib().call("s2d_matcher_cost_c_f32", ml, cls[None].contiguous(), 2, tg, cn, None, 4, 1, B, Q, ml.shape[-1], T, h, w, H, W, 5, P,
               2.0, 5.0, 5.0, ws, Cb, _stream())
    assert torch.equal(Ca, Cb)
    # KD targets (threshold 0.3: ties in count / order would show)
    ka = ops.kd_targets(cls, ml[0], (Q, T, h, w), H, W, Q, 0.3, 10)
    kb = [torch.zeros_like(t) for t in ka]
    lab = torch.zeros_like(ka[2])
    wsk = torch.empty(lib().call("s2d_kd_targets_c_workspace_bytes", B, Q, 2), device="cuda", dtype=torch.uint8)
    lib().call("s2d_kd_targets_c_u8", cls, 2, ml[0], 0.3, 10, B, Q, ml.shape[-1], T, h, w, H, W, Q, wsk, kb[0], kb[1], kb[2], lab, kb[3],
               _stream())
    n = ka[1].cpu()
    assert torch.equal(n, kb[1].cpu()) and int(n.sum()) > 0 and not lab.any()
    for b in range(B):
        k = int(n[b])
        assert torch.equal(ka[2][b, :k], kb[2][b, :k])
        assert torch.equal(ka[0][b, :k], kb[0][b, :k]) and torch.equal(ka[3][b, :k], kb[3][b, :k])
    # inference select
    c1 = cls[0].contiguous()
    sa, qa, la = ops.infer_select(c1, 8)
    sb, qb, lb = torch.empty_like(sa), torch.empty_like(qa), torch.empty_like(la)
    wsi = torch.empty(lib().call("s2d_infer_select_c_workspace_bytes", Q, 2), device="cuda", dtype=torch.uint8)
    lib().call("s2d_infer_select_c_f32", c1, Q, 2, 8, wsi, sb, qb, lb, _stream())
    assert torch.equal(sa, sb) and torch.equal(qa, qb) and torch.equal(la, lb)


def test_kd_run_step_at_40_classes_is_finite_and_reproducible():
    """one engine.run_step of a class-aware KDVideoMaskFormer on a mapper-shaped batch: finite losses, bitwise-equal gradients
    over two runs from the same state"""
    from tests.test_classes_cpu import build_model
    from s2d_amd import engine
    from s2d_amd.optim import FullModelGradientClippingAdamW
    from s2d_amd.utils import synth
    T, H0, W0 = 2, 60, 90
    data = []
    for b in range(2):
        fr = synth.smooth_frames_u8(3, b, T, H0, W0)
        m, ids = synth.ellipse_targets(3, 10 + b, 3, T, H0, W0, sparse=0.0)
        data.append({"image": [torch.from_numpy(f) for f in fr],
                     "instances": [{"gt_masks": torch.from_numpy(m[:, t]), "gt_ids": torch.from_numpy(ids[:, t])} for t in range(T)]})
    grads = []
    for _ in range(2):
        torch.manual_seed(0)
        model = build_model("KDVideoMaskFormer", 40, small=True).cuda()
        model.train()
        params = [p for p in model.student.parameters() if p.requires_grad]
        opt = FullModelGradientClippingAdamW(params, lr=0.0, clip_norm=1.0)
        losses = engine.run_step(model, opt, data, 0)
        assert "loss_ce" in losses and all(np.isfinite(float(v)) for v in losses.values())
        assert model.student[1].predictor.class_embed.weight.shape[0] == 41
        grads.append([p.grad.detach().clone() for p in params if p.grad is not None])
    assert len(grads[0]) == len(grads[1]) > 0
    assert all(torch.equal(a, b) for a, b in zip(*grads))
