"""The class-aware kernels (SEM_SEG_HEAD.NUM_CLASSES > 1: C + 1 class logits per query) at the benched head sizes -- Q = 100, 10 decoder
heads, B = 2 -- each compared with a float64 restatement of the same operation (nothing of s2d_amd / libs2d_hip.so in the reference).
The class-aware counterpart of tests/test_gpu_forward_c4.py, tests/test_gpu_backward_c4.py and tests/test_gpu_eval_720p.py, whose
recorders, signature functions, `_case_*` functions, bound rule and `c4row` vocabulary it uses by importing them.  The references and the
constructed inputs live in tests/test_classes_refs_cpu.py, which checks without a GPU that every input decides like float64.

A. Recorded rows.  record_class_steps builds tests/test_classes_cpu.build_model("KDVideoMaskFormer", C) (the full configuration: Q = 100,
10 heads) for C = 40 and for C = 1 from the same configuration otherwise, and runs one forward_losses, one forward_backward and one
eval-mode model([video]) of each under the forward and the backward recorder, on a small clip (B = 2, T = 2, 64 x 96, P = 256: the
class-dependent shapes depend on NL, B, Q and C only).  In both models the teacher's class-0 bias is raised until every query passes the
distillation threshold, so both runs fill the same 100 pseudo-target slots and no slot count differs between them.  TABLE is the set
difference: every (entry point, signature) the 40-class run makes that the 1-class run does not.  test_table_covers_the_class_aware_step
re-records and fails when the 40-class run makes a call that is neither in TABLE nor made by the 1-class run, or when a row of TABLE
is no longer seen.  Rows run the `_case_*` of the c4 modules on the recorded signature (same bound: max(bound of the small-size test,
2 x the float32-torch error of the same restatement on these operands), never read off the kernel).  matcher_cost rows have no
`_case_`: the kernel draws its own points there; test_matcher_cost_matrix_and_assignment compares the whole matrix of the class-aware
form at the recorded NL, B, Q, C1 with injected points.  EXTRA_ROWS are the class-head rows at C = 80 (COCO images), which no recorded
run makes.

B. Named cases of the discrete kernels, all at Q = 100, B = 2, no element excluded from any comparison.
  ops.kd_targets (test_kd_targets_case; reference: refs.kd_select_ref; count, kept, label exact; planes == (float64 bilinear > 0) on
  every pixel -- the logits are built so that no value lies in the sign band -- and nonempty == any(plane)), 16 x 24 masks, 64 x 96 targets:
    a  C = 40, topk = 20, thr 0.3            K <= Q: the floor comes from the row bests, and lies below the K-th score
    b  C = 40, topk = 128 > Q, Nmax = 128    the floor is thr alone
    c  40 scores pass, Nmax = 16             truncation in ascending flat index, count == Nmax
    d  clip 0 has no score at thr            count[0] == 0 beside a full clip
    e  passing scores at flat index >= 3840  only the last, ragged workgroup has candidates
    f  passing scores below flat index 256   only the first workgroup has candidates
    g  logit rows 2k and 2k + 1 identical    an exact tie straddles rank K - 1 (K = 21): the lower flat index is kept
    h  one query, three labels above thr     flat indices 254, 255, 257 / 510, 511, 513: across a 256-step of the compaction
    i  C = 1203, topk = 20                   n = 120 300 scores, 470 workgroups
    j  C = 2                                 C1 = 3, the smallest class-aware size
  ops.infer_select (test_infer_select_case): scores at rtol 1e-5, query and label exact, at (Q, C, K) = refs.INFER_SHAPES -- Q*C = 16384
  is the last size the single-workgroup LDS kernel takes, 128 x 129 the first the multi-workgroup form takes -- K > Q, and the tied rows
  of case g.  Wherever the LDS kernel can run, s2d_infer_select_c_f32 is also called directly and equals ops.infer_select bit for bit.
  ops.matcher_cost + ops.lsap, C1 in {3, 41, 81}, class weight 2.0, NL = 10: the whole cost matrix against tests/test_gpu_e2e._cost64
  (class column -softmax64(logits)[:, 0]) at 1e-5 of the largest cost term; the device assignment against
  scipy.optimize.linear_sum_assignment of the float64 matrix through _same_assignment (only a proven tie passes).
  ops.class_loss / ops.class_loss_backward, C1 in {3, 41, 81, 1204}, n_match [0, 0], [100, 100], [10, 37], and logits spanning +-30
  (exp(l - max) underflows in float32): float64 cross_entropy and its autograd, bound max(1e-6, 2 x float32-torch error).

The figures of one run, the recorded table and the mutants this module was run against are in profiles/classes_parity.txt."""
import time

import numpy as np
import pytest
import torch

from tests import test_classes_refs_cpu as refs
from tests import test_gpu_backward_c4 as bc4
from tests import test_gpu_eval_720p as ev
from tests import test_gpu_forward_c4 as fc4
from tests.test_gpu_backward_c4 import DEV, F32, F64, _Rep, _gen, _row_id, _sh

pytestmark = pytest.mark.gpu

C_AWARE, C_PLAIN = 40, 1
B, T, H0, W0, N_GT = 2, 2, 64, 96, 3
CONFIG = ("INPUT.SAMPLING_FRAME_NUM", str(T), "MODEL.MASK_FORMER.TRAIN_NUM_POINTS", "256")


def _sig_class_loss_backward(class_logits, idx_q, n_match, w_ce, eos_coef=0.1):
    return _sh(class_logits) + (idx_q.shape[-1],)


ENTRY_POINTS = dict(ev.ENTRY_POINTS, class_loss_backward=_sig_class_loss_backward)
NO_ROWS = fc4.NO_ROWS


# --------------------------------------------------------------------------- recording
def build(C):
    """the full KD configuration with C classes; every query of the teacher passes the distillation threshold on class 0"""
    from tests.test_classes_cpu import build_model
    torch.manual_seed(0)
    model = build_model("KDVideoMaskFormer", C, extra=CONFIG).to(DEV)
    with torch.no_grad():
        model.teacher[1].predictor.class_embed.bias[0] += 12.0
    return model


def record(C):
    """one forward_losses, one forward_backward, one eval-mode model([video]) -> the set of (entry point, signature) pairs"""
    import bench
    from s2d_amd import backward, ops
    from s2d_amd.modeling import TargetSet
    dev = torch.device(DEV)
    model = build(C)
    frames, masks = bench.synth_batch(0, B, T, H0, W0, N_GT, dev)
    fwd, bwd = [], []
    model.train()
    with fc4.recording(ops, fwd, backward, ENTRY_POINTS, ev.LIB_CALLS), bc4.recording(backward, bwd):
        for step in (model.forward_losses, model.forward_backward):
            model.criterion.seed = 0; model.criterion.matcher.seed = 0
            torch.manual_seed(5); ops._DROP_CALLS[0] = 0
            step(ops.normalize_pad(frames), TargetSet.from_list(masks, device=dev))
            torch.cuda.synchronize()
        last = getattr(model, "last", None) or {}
        counts = last["kd_count"].cpu().tolist() if "kd_count" in last else None
        model.last_tapes = None
        model.eval()
        model([{"image": list(frames[:T])}])
        torch.cuda.synchronize()
    assert counts is None or all(c == 100 for c in counts), counts          # the same pseudo-target slots in both models
    del model, frames, masks
    torch.cuda.empty_cache()
    return set(fwd) | set(bwd)


_RECORDED = {}


def record_class_steps():
    """both models, once per process -> (signatures of the 40-class run, of the 1-class run)"""
    if not _RECORDED:
        t0 = time.perf_counter()
        _RECORDED.update(aware=record(C_AWARE), plain=record(C_PLAIN))
        print(f"classtable: both recordings took {time.perf_counter() - t0:.1f} s")
    return _RECORDED["aware"], _RECORDED["plain"]


# --------------------------------------------------------------------------- what a 40-class step calls that a 1-class step does not
TABLE = [
    ('bias_grad', 200, 41, 1.0),
    ('bias_grad', 200, 41, None),
    ('class_loss', 2, 100, 41, 100),
    ('class_loss', 2, 100, 41, 3),
    ('class_loss_backward', 2, 100, 41, 3),
    ('gemm_nt', 1, 100, 41, 256, False, True, False, True, None, False, 41, None),
    ('gemm_nt', 1, 200, 41, 256, False, True, False, True, None, False, 41, None),
    ('infer_select', 100, 41, 10),
    ('input_grad', 200, 41, 256, True, None, False),
    ('kd_targets', 2, 41, 100, 2, 16, 24, 100, 64, 96, 100, 100, True),
    ('matcher_cost', 10, 2, 768, 100, 41, 100, 2, 64, 96, 256, False),
    ('matcher_cost', 10, 2, 768, 100, 41, 3, 2, 64, 96, 256, False),
    ('weight_grad', 200, 41, 256, 1.0, None),
    ('weight_grad', 200, 41, 256, None, None),
]

# the class head at C = 80 (COCO image annotations as pseudo-clips): the rows above with 41 -> 81; no recorded run makes them
EXTRA_ROWS = [
    ('bias_grad', 200, 81, 1.0),
    ('bias_grad', 200, 81, None),
    ('class_loss', 2, 100, 81, 100),
    ('class_loss', 2, 100, 81, 3),
    ('class_loss_backward', 2, 100, 81, 3),
    ('gemm_nt', 1, 100, 81, 256, False, True, False, True, None, False, 81, None),
    ('gemm_nt', 1, 200, 81, 256, False, True, False, True, None, False, 81, None),
    ('input_grad', 200, 81, 256, True, None, False),
    ('weight_grad', 200, 81, 256, 1.0, None),
    ('weight_grad', 200, 81, 256, None, None),
]


def test_table_covers_the_class_aware_step():
    """TABLE == (signatures of the 40-class run) - (signatures of the 1-class run): a call only the class-aware step makes fails here
    until it has a row, and so does a row the step no longer makes"""
    aware, plain = record_class_steps()
    assert len(aware) > 100 and len(plain) > 100
    table = set(TABLE)
    assert len(table) == len(TABLE) and not table & plain
    for row in sorted(aware - plain, key=repr):
        print("classtable:", row)
    missing = sorted(aware - table - plain, key=repr)
    gone = sorted(table - aware, key=repr)
    assert not missing and not gone, (missing, gone)
    for row in TABLE:
        assert row[0] in NO_ROWS or _case_of(row[0]) is not None, row


# --------------------------------------------------------------------------- rows
def _case_class_loss_backward(rep, g, Bn, Qn, C1, maxm):
    """bound 1e-6 (test_class_loss_forward_golden_and_backward_float64): d(w_ce * weighted cross-entropy) / d logits against float64
    autograd, on the operands _case_class_loss draws"""
    from s2d_amd import ops
    logits = bc4._rn(g, Bn, Qn, C1) * 2.0
    iq = torch.zeros((Bn, maxm), device=DEV, dtype=torch.int32)
    nm = torch.tensor([maxm, max(maxm - 3, 0)][:Bn] + [maxm // 2] * max(Bn - 2, 0), device=DEV, dtype=torch.int32)
    for b in range(Bn):
        q = torch.randperm(Qn, device=DEV, generator=g)[:int(nm[b])].sort().values
        iq[b, :q.numel()] = q.int()
    d = ops.class_loss_backward(logits, iq, nm, 2.0, 0.1)
    rep.same("second call", ops.class_loss_backward(logits, iq, nm, 2.0, 0.1), d)
    host = (logits.cpu().numpy(), iq.cpu().numpy(), nm.cpu().numpy())
    g64, g32 = (refs.class_loss_ref(*host, 2.0, 0.1, dt)[1].to(DEV) for dt in (F64, F32))
    rep.cmp("dlogits", d, g64, g32, 1e-6)


def _case_of(name):
    for mod in (globals(), vars(fc4), vars(bc4), vars(ev)):
        if "_case_" + name in mod:
            return mod["_case_" + name]
    return None


def _rows():
    return [r for r in TABLE + EXTRA_ROWS if r[0] not in NO_ROWS]


def _run(rep, fn):
    """fn() with plain-float32 torch matmuls, timed on the host around a synchronisation"""
    old = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old
    print(f"c4row {rep.row} time: {(time.perf_counter() - t0) * 1e3:.1f} ms (kernel calls, references and comparisons)")
    rep.done()


@pytest.mark.parametrize("row", _rows(), ids=_row_id)
def test_class_row_vs_float64(row):
    rep = _Rep(row)
    _run(rep, lambda: _case_of(row[0])(rep, _gen(row), *row[1:]))


# --------------------------------------------------------------------------- named cases: distillation targets
_SHARED = {}


def _kd_masks():
    """the shared mask logits on the device, pixel-major with four NaN pad columns, and the float64 sign reference (computed once)"""
    if "pm" not in _SHARED:
        ml, ref, _ = refs.kd_mask_logits()
        _SHARED["pm"] = torch.from_numpy(refs.pixel_major(ml, refs.Q + 4)).to(DEV)
        _SHARED["planes"] = torch.from_numpy(ref).to(DEV)
    return _SHARED["pm"], _SHARED["planes"]


@pytest.mark.parametrize("name", list("abcdefghij"))
def test_kd_targets_case(name):
    from s2d_amd import ops
    case = refs.kd_cases()[name]
    rep = _Rep(("kd_targets", "case", name, case["C"], case["topk"], case["thr"], case["Nmax"]))
    Q, Tn, hm, wm, H, W = refs.Q, refs.T, refs.HM, refs.WM, refs.H, refs.W

    def body():
        pm, planes = _kd_masks()
        cls = torch.from_numpy(case["cls"]).to(DEV)
        run = lambda: ops.kd_targets(cls, pm, (Q, Tn, hm, wm), H, W, case["Nmax"], case["thr"], case["topk"], want_labels=True)
        got, again = run(), run()
        tgt, count, kept, ne, lab = got
        ref = refs.kd_select_ref(case["cls"], case["thr"], case["topk"], case["Nmax"])
        for b in range(refs.B):
            n, r = ref[b]["count"], ref[b]
            print(f"c4row {rep.row} clip {b}: reference selects {r['passing']}, count {n}; kernel count {int(count[b])}")
            fc4._check(rep, f"clip {b}: count", int(count[b]) == n)
            fc4._check(rep, f"clip {b}: count second call", int(again[1][b]) == int(count[b]))
            rep.same(f"clip {b}: kept", kept[b, :n].cpu(), r["kept"])
            rep.same(f"clip {b}: label", lab[b, :n].cpu(), r["label"])
            for k, what in ((0, "planes"), (2, "kept"), (3, "nonempty"), (4, "label")):
                rep.same(f"clip {b}: {what} second call", again[k][b, :n], got[k][b, :n])
            want = planes[b, r["kept"].long().to(DEV)]                               # [n, T, H, W] bool
            wrong = int(((tgt[b, :n] != 0) != want).sum())
            print(f"c4row {rep.row} clip {b} planes: {wrong} of {want.numel()} pixels wrong, none excluded")
            if wrong:
                rep.bad.append(("planes", b, wrong))
            fc4._check(rep, f"clip {b}: planes are 0 / 1", n == 0 or int(tgt[b, :n].max()) <= 1)
            rep.same(f"clip {b}: nonempty != 0", ne[b, :n] != 0, want.flatten(2).any(-1))
    _run(rep, body)


# --------------------------------------------------------------------------- named cases: inference selection
@pytest.mark.parametrize("name", list(refs.infer_cases()))
def test_infer_select_case(name):
    from s2d_amd import ops
    cls_h, K, tied = refs.infer_cases()[name]
    Qn, C1 = cls_h.shape
    rep = _Rep(("infer_select", "case", name))

    def body():
        cls = torch.from_numpy(cls_h).to(DEV)
        s, q, l = ops.infer_select(cls, K)
        s2, q2, l2 = ops.infer_select(cls, K)
        rs, rq, rl = (t.to(DEV) for t in refs.infer_select_ref(cls_h, K))
        lds = Qn * (C1 - 1) <= ops.INFER_SELECT_LDS_SCORES
        forms = [("LDS kernel" if lds else "multi-workgroup form", s, q, l)]
        if lds:                                                   # the other form on the same input, straight through the C ABI
            L = ops.lib()
            sb, qb, lb = torch.empty_like(s), torch.empty_like(q), torch.empty_like(l)
            ws = torch.empty(L.call("s2d_infer_select_c_workspace_bytes", Qn, C1), device=DEV, dtype=torch.uint8)
            L.call("s2d_infer_select_c_f32", cls, Qn, C1, K, ws, sb, qb, lb, ops._stream())
            forms.append(("multi-workgroup form", sb, qb, lb))
            for a, b_, what in ((sb, s, "scores"), (qb, q, "query"), (lb, l, "label")):
                rep.same(f"{what}: s2d_infer_select_c_f32 == ops.infer_select", a, b_)
        for a, b_, what in ((s2, s, "scores"), (q2, q, "query"), (l2, l, "label")):
            rep.same(f"{what} second call", a, b_)
        for form, fs, fq, fl in forms:
            err = float(((fs.double() - rs).abs() / rs).max())
            print(f"c4row {rep.row} {form}: scores max rel error {err:.3e} bound {refs.SCORE_RTOL:.3e}")
            if not err < refs.SCORE_RTOL:
                rep.bad.append((form, "scores", err))
            rep.same(f"{form}: query", fq, rq)
            rep.same(f"{form}: label", fl, rl)
    _run(rep, body)


# --------------------------------------------------------------------------- named cases: matcher cost and assignment
@pytest.mark.parametrize("C1", [3, 41, 81])
def test_matcher_cost_matrix_and_assignment(C1, oracle):
    from scipy.optimize import linear_sum_assignment
    from s2d_amd import ops
    from tests.test_gpu_criterion import _dev, pixel_major
    from tests.test_gpu_e2e import _cost64, _same_assignment
    rep = _Rep(("matcher_cost", "case", refs.NL, refs.B, refs.Q, C1))
    weights = (2.0, 5.0, 5.0)

    def body():
        logits, masks, tgt, cnt, coords = refs.matcher_inputs(C1)
        Cm = ops.matcher_cost(_dev(pixel_major(masks)), _dev(logits), _dev(tgt), _dev(cnt), (refs.Q, refs.T, refs.HM, refs.WM), refs.P, weights,
                              coords=_dev(coords))
        Cm2 = ops.matcher_cost(_dev(pixel_major(masks)), _dev(logits), _dev(tgt), _dev(cnt), (refs.Q, refs.T, refs.HM, refs.WM), refs.P, weights,
                               coords=_dev(coords))
        rep.same("second call", Cm2, Cm)
        iq, it, nm = (t.cpu().numpy() for t in ops.lsap(Cm, _dev(cnt), refs.B))
        Ch = Cm.cpu().numpy().astype(np.float64)
        worst = 0.0
        for layer in range(refs.NL):
            for b in range(refs.B):
                n, prob = int(cnt[b]), layer * refs.B + b
                Co, scale = _cost64(oracle, logits[layer, b], masks[layer, b], tgt[b, :n], coords[layer, b][None], *weights)
                worst = max(worst, float(np.abs(Ch[prob][:, :n] - Co).max() / scale))         # every element of the matrix
                assert nm[prob] == n
                ri, rj = linear_sum_assignment(Co)
                _same_assignment(iq[prob, :n], it[prob, :n], ri, rj, Co)
        print(f"c4row {rep.row} cost matrix, {refs.NL * refs.B} problems: max error {worst:.3e} of the largest cost term, bound 1.000e-05")
        if not worst <= 1e-5:
            rep.bad.append(("cost", worst))
    _run(rep, body)


# --------------------------------------------------------------------------- named cases: class loss and its gradient
@pytest.mark.parametrize("key", list(refs.CLASS_LOSS_MATCHES) + ["wide"])
@pytest.mark.parametrize("C1", refs.CLASS_LOSS_C1)
def test_class_loss_case(C1, key):
    from s2d_amd import ops
    wide = key == "wide"
    nm_h = [10, 37] if wide else refs.CLASS_LOSS_MATCHES[key]
    rep = _Rep(("class_loss", "case", refs.B, refs.Q, C1, key))

    def body():
        logits, iq, nm = refs.class_loss_inputs(C1, nm_h, wide)
        (l64, g64), (l32, g32) = (refs.class_loss_ref(logits, iq, nm, 2.0, 0.1, dt) for dt in (F64, F32))
        x, i, n = (torch.from_numpy(a).to(DEV) for a in (logits, iq, nm))
        ce = ops.class_loss(x, i, n, 0.1)
        d = ops.class_loss_backward(x, i, n, 2.0, 0.1)
        rep.same("loss second call", ops.class_loss(x, i, n, 0.1), ce)
        rep.same("gradient second call", ops.class_loss_backward(x, i, n, 2.0, 0.1), d)
        rep.cmp("loss_ce", ce.reshape(1), l64.reshape(1).to(DEV), l32.reshape(1).to(DEV), 1e-6)
        rep.cmp("dlogits", d, g64.to(DEV), g32.to(DEV), 1e-6)
    _run(rep, body)
