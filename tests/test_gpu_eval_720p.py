"""Eval-path kernel calls at 720p video lengths, each compared with a float64 restatement of the same operation written in plain torch
on the device (nothing of s2d_amd / libs2d_hip.so in the reference).  The eval counterpart of tests/test_gpu_forward_c4.py, whose
recorder, signature functions, `_case_*` functions, bound rule and `c4row` vocabulary it uses by importing them.

Scenarios (record_eval_scenarios): the KD model as bench.py builds it for c4 (Q = 100, seeded weights, bench.calibrate_teacher) in
.eval(), synthetic 720 x 1280 u8 frames through model([video]):

    S16  T = 16  one clip, output 720 x 1280 (the SAME resize), NMS off, host bool masks
    S36  T = 36  one clip (the longest YTVIS video), height / width 1080 x 1920 (the two-stage resize), use_nms, inference_rle
    S64  T = 64  one clip (the largest size the throughput ladder of profiles/window_inference ran), device masks
    W40  T = 40  WINDOW_SIZE 16, WINDOW_OVERLAP 2: windows (0,16), (14,30), (28,40) -- a 12-frame window and the stitch calls

TABLE is the set of (entry point, shape signature) pairs those four runs make that the c4 step does not; COVERED_BY_C4 the ones that are
rows of the c4 forward TABLE already (run there, not here); COVERED_ELSEWHERE the ones a named existing test checks at this very size.
test_table_covers_the_eval_scenarios re-records the scenarios and fails on a call none of the three holds, when COVERED_BY_C4 is not
exactly what it sees, or when ops.py has a public name without a signature (there or here) and without a reason in NOT_KERNELS.

Rows of entry points shared with training run the c4 module's `_case_*` on the new signature: same bound (max(bound of the small-size
test named in the case, 2 x the float32-torch error of the same restatement on these operands), never read off the kernel), same
second-call bit equality.  EXTRA_ROWS are rows the issue of this module asks for at eval sizes that no scenario makes: the 64-bit
index branch of infer_resize_kernel (K = 1, 23 x 40 maps, T * 1080 * 1920 just over 2^31, and -- because the 32-bit branch is unsigned
and so still exact below 2^32 -- just over 2^32), a two-stage resize whose two scales differ, pack_mask_bits at the
S36 mask size (mask_pair_counts at that size is a recorded row), and a scatter with pad columns (ldq > Q).

Sign band of the infer_masks rows (derived from the inputs alone, _mask_band): the kernel forms each source coordinate
`scale * (dst + 0.5) - 0.5` in float32 -- the scale rounded once, one product, one difference: at most 3 units of 2^-24 of a
coordinate whose magnitude is the SOURCE size of that stage.  Stage 1 (low-res hm x wm -> padded Hp x Wp): <= 3 * 2^-24 * max(hm, wm)
low-res pixels; a bilinear surface moves at most D per low-res pixel along an axis, D = the largest adjacent-tap difference of the
input, so <= 3 * 2^-24 * max(hm, wm) * D per axis.  Stage 2 (ih x iw -> oh x ow): <= 3 * 2^-24 * max(ih, iw) padded pixels, over a
surface of slope <= D * hm / Hp per padded pixel: the same figure again.  Two axes, two stages: 12 * 2^-24 * max(hm, wm) * D.  The
issue's own, coarser statement of this term -- 2^-24 of a coordinate as large as the largest padded / output extent C, times D, per
axis and stage -- is 4 * 2^-24 * C * D; the band takes the larger of the two.  Arithmetic: each stage is a 4-tap float32 sum of
products with weights in [0, 1]: a few units of 2^-24 of the largest tap A per stage, taken as 8, so 16 * 2^-24 * A.

    band = 2^-24 * (max(4 * C, 12 * max(hm, wm)) * D + 16 * A)

about 1e-4 on the smooth two-signed fields of amplitude 3 used here (as the small test's inputs; _smooth_logits of the c4 module).
Signs are compared outside |float64 value| < band; the excluded share is printed and capped at 1e-3 (the cap of
test_select_masks_and_pair_counts_vs_oracle).  torch's own two float32 F.interpolate calls are evaluated too: every pixel where they
disagree with the kernel must lie inside the band.  CPU pre-check of the share on one frame of the reference alone and the figures
of one run: profiles/eval_720p_parity.txt.

RLE: rle.encode on the S36-size masks; every frame's string decodes (oracle_np.rle_decode) to the mask, area and box equal
oracle_np.rle_area_bbox, and oracle_np.rle_encode (pure-python loops over 2 M pixels) gives the identical string on the frames
_RLE_EXACT_FRAMES; the run-length string of a mask is unique, so a string that decodes to the mask and is canonical is the string.

Composition (test_composition_at_size): the class and mask logits the recorder saw reach inference_video with, under S36 and W40,
go through a float64 restatement of inference_video (softmax top-K, two-stage resize, greedy NMS on exact counts) and are compared
with what model([video]) returned: labels and kept set equal, scores at rtol 1e-5, masks equal outside the band."""
import time

import numpy as np
import pytest
import torch

from tests import test_gpu_forward_c4 as fc4
from tests.test_gpu_backward_c4 import DEV, F32, F64, _Rep, _gen, _rn, _row_id

pytestmark = pytest.mark.gpu

H0, W0, Q, NPRED = 720, 1280, 100, 10
WINDOW, OVERLAP = 16, 2


# --------------------------------------------------------------------------- shape signatures of the eval-only entry points
def _sig_infer_select(class_logits, K):
    return (class_logits.shape[0], class_logits.shape[1], int(K))


def _sig_infer_masks(mask_logits, dims, padded, img_size, out_size, query, want_bits=False):
    return tuple(int(v) for v in dims) + (int(mask_logits.shape[-1]),) + tuple(int(v) for v in (*padded, *img_size, *out_size)) + (
        query.shape[0], bool(want_bits))


def _sig_pack_mask_bits(masks):
    return (masks.shape[0], masks[0].numel() if masks.shape[0] else 0)


def _sig_mask_pair_counts(bits):
    return (bits.shape[0], bits.shape[1])


def _sig_window_pair_counts(a, b, Q):
    return (a.shape[0], a.shape[1], int(Q))


def _sig_window_scatter_columns(src, perm, dst, row0, Q):
    return (src.shape[0], src.shape[1], int(Q), dst.shape[0], int(row0))


# the three library calls of s2d_amd/rle.py; the number of frames F (instances kept by the NMS x T) and the number of runs are data
def _sig_s2d_rle_count_u8(masks, F, H, W, *rest):
    return (H, W)


def _sig_s2d_rle_positions_u8(masks, F, H, W, *rest):
    return (H, W)


def _sig_s2d_rle_strings_u8(positions, frame_off, F, hw, *rest):
    return (int(hw),)


LIB_CALLS = dict(fc4.LIB_CALLS, s2d_rle_count_u8=_sig_s2d_rle_count_u8, s2d_rle_positions_u8=_sig_s2d_rle_positions_u8,
                 s2d_rle_strings_u8=_sig_s2d_rle_strings_u8)
OWN_ENTRY_POINTS = {n[5:]: f for n, f in list(globals().items()) if n.startswith("_sig_") and n[5:] not in LIB_CALLS}
ENTRY_POINTS = dict(fc4.ENTRY_POINTS, **OWN_ENTRY_POINTS)


def unknown_public_functions(ops):
    """public functions and classes of s2d_amd/ops.py with no signature in the c4 module or here and no reason in its NOT_KERNELS"""
    import inspect
    public = {n for n, f in vars(ops).items() if not n.startswith("_") and (inspect.isfunction(f) or inspect.isclass(f))
              and getattr(f, "__module__", None) in (ops.__name__, "s2d_amd._lib")}
    return sorted(public - set(ENTRY_POINTS) - set(fc4.ALIASES) - set(fc4.NOT_KERNELS))


# --------------------------------------------------------------------------- the scenarios
SCENARIOS = {
    "S16": dict(T=16),
    "S36": dict(T=36, height=1080, width=1920, use_nms=True, inference_rle=True),
    "S64": dict(T=64, inference_device_masks=True),
    "W40": dict(T=40, window=True),
}


class _Timer:
    """HIP events around every top-level call of a recorded entry point: {name: summed ms} of one scenario"""

    def __init__(self):
        self.pairs, self.depth = [], 0

    def wrap(self, name, fn):
        def timed(*a, **k):
            if self.depth:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.depth += 1
            try:
                return fn(*a, **k)
            finally:
                self.depth -= 1
                e1.record()
                self.pairs.append((name, e0, e1))
        return timed

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.pairs:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def build_eval_model():
    """the c4 model of bench.py, calibrated on the c4 batch as the c4 modules calibrate it, in .eval()"""
    import bench
    from s2d_amd import ops
    from s2d_amd.modeling import build_kd_model
    dev = torch.device(DEV)
    B, T, h0, w0, q, P, N = bench.CONFIGS["c4"]
    assert (h0, w0, q) == (H0, W0, Q)
    model = build_kd_model(num_queries=Q, num_frames=T, num_points=P, dropout=0.3).to(dev)
    frames, _ = bench.synth_batch(0, B, T, H0, W0, 0, dev)
    bench.calibrate_teacher(model, ops.normalize_pad(frames))
    del frames
    model.eval()
    model.num_predictions_inference = NPRED
    return model


def run_scenario(model, name, log=None, capture=None, timer=None):
    """model([video]) of one scenario under the recorder -> the model's output.  capture (a dict): receives the arguments
    inference_video's infer_select / infer_masks calls were made with (the logits at the end of the forward)."""
    import bench
    from s2d_amd import ops
    sc = SCENARIOS[name]
    frames, _ = bench.synth_batch(0, 1, sc["T"], H0, W0, 0, torch.device(DEV))
    video = {"image": list(frames)}
    if "height" in sc:
        video["height"], video["width"] = sc["height"], sc["width"]
    model.use_nms = bool(sc.get("use_nms", False))
    model.inference_rle = bool(sc.get("inference_rle", False))
    model.inference_device_masks = bool(sc.get("inference_device_masks", False))
    model.window_inference, model.window_size, model.window_overlap = bool(sc.get("window", False)), WINDOW, OVERLAP
    eps = dict(ENTRY_POINTS)
    if capture is not None:
        def sel(class_logits, K):
            capture["cls"] = class_logits
            return _sig_infer_select(class_logits, K)

        def msk(mask_logits, dims, padded, img_size, out_size, query, want_bits=False):
            capture.update(ml=mask_logits, dims=dims, padded=padded, img_size=img_size, out_size=out_size)
            return _sig_infer_masks(mask_logits, dims, padded, img_size, out_size, query, want_bits)
        eps.update(infer_select=sel, infer_masks=msk)
    saved = []
    if timer is not None:                                  # inside the recorder's wrappers: the recorder patches on top of these
        for n in ENTRY_POINTS:
            saved.append((n, getattr(ops, n)))
            setattr(ops, n, timer.wrap(n, getattr(ops, n)))
    try:
        with fc4.recording(ops, [] if log is None else log, None, eps, LIB_CALLS):
            out = model([video])
            torch.cuda.synchronize()
    finally:
        for n, f in saved:
            setattr(ops, n, f)
        model.use_nms = model.inference_rle = model.inference_device_masks = model.window_inference = False
    return out


_RECORDED = {}


def record_eval_scenarios():
    """the four scenarios, once per process -> {"log": all signatures, "S36" / "W40": (captured logits, model output), "ms": {scenario:
    {entry point: ms}}}; the T = 64 clip is run last but one and released before W40"""
    if _RECORDED:
        return _RECORDED
    model = build_eval_model()
    log, ms, keep = [], {}, {}
    for name in ("S16", "S36", "S64", "W40"):
        cap, timer = {}, _Timer()
        out = run_scenario(model, name, log, cap)          # recorded cold: a cached result (pe_sine keeps its last one) hides no call
        t0 = time.perf_counter()
        run_scenario(model, name, None, None, timer)       # timed warm
        wall = time.perf_counter() - t0
        ms[name] = dict(timer.totals(), _wall=wall * 1e3)
        if name in ("S36", "W40"):
            keep[name] = (cap, out)
        del out, cap
        torch.cuda.empty_cache()
    del model
    torch.cuda.empty_cache()
    _RECORDED.update(log=log, ms=ms, **keep)
    return _RECORDED


# --------------------------------------------------------------------------- the eval scenarios (recorded; see the coverage test)
# rows of the c4 forward TABLE the scenarios make too: compared there, not run again here
COVERED_BY_C4 = [
    ('conv2d_nhwc', 16, 184, 320, 128, 128, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 16, 184, 320, 256, 256, 3, 3, 1, 1, False, False, False, False, True),
    ('conv2d_nhwc', 16, 184, 320, 256, 512, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 16, 184, 320, 64, 64, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 16, 23, 40, 512, 512, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 16, 46, 80, 1024, 2048, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 16, 46, 80, 256, 256, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 16, 46, 80, 512, 512, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 16, 736, 1280, 4, 64, 7, 7, 2, 3, True, True, False, True, True),
    ('conv2d_nhwc', 16, 92, 160, 128, 128, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 16, 92, 160, 256, 256, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 16, 92, 160, 512, 1024, 1, 1, 2, 0, True, True, False, False, True),
    ('gemm_nt', 1, 1, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 14720, 2048, 512, False, True, True, True, (2048, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 14720, 256, 2048, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 14720, 512, 2048, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 14720, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 19320, 288, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 235520, 128, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 235520, 256, 512, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 235520, 256, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 235520, 512, 128, False, True, True, True, (512, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 235520, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 309120, 544, 256, False, True, False, True, (288, 19320, 288, False), False, None, None),
    ('gemm_nt', 1, 58880, 1024, 256, False, True, True, True, (1024, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 58880, 256, 1024, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 58880, 256, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 58880, 512, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 58880, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 942080, 128, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 942080, 256, 256, False, True, False, False, None, False, None, None),
    ('gemm_nt', 1, 942080, 256, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 942080, 256, 64, False, True, True, True, (256, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 942080, 256, 64, False, True, True, True, None, False, None, None),
    ('gemm_nt', 1, 942080, 64, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 942080, 64, 64, False, True, True, True, None, True, None, None),
    ('groupnorm_nhwc', 16, 184, 320, 256, 32, (92, 160), False),
    ('groupnorm_nhwc', 16, 184, 320, 256, 32, None, True),
    ('groupnorm_nhwc', 16, 23, 40, 256, 32, None, False),
    ('groupnorm_nhwc', 16, 46, 80, 256, 32, None, False),
    ('groupnorm_nhwc', 16, 92, 160, 256, 32, None, False),
    ('maxpool3x3s2', 16, 368, 640, 64, False),
    ('msda_fused_forward', 16, 256, ((23, 40), (46, 80), (92, 160)), 544, 544, 288, 8, 4),
    ('normalize_pad', 16, 720, 1280, 32),
]

# rows an existing test checks at this very size; each with the test
COVERED_ELSEWHERE = {
    ('lsap', 1, 100, 100, 1):
        "tests/test_gpu_window_inference.py::test_stitch_recovers_shuffled_tracks (Q = 100: every assignment against scipy on the same cost matrix)",
    ('window_pair_counts', 117760, 100, 100):
        "tests/test_gpu_window_inference.py::test_pair_counts_equal_numpy_and_the_composition_of_existing_ops[117760-100]",
    ('s2d_rle_positions_u8', 1080, 1920):
        "the s2d_rle_count_u8 row of this module: rle.encode's three calls are checked together through its strings",
    ('s2d_rle_strings_u8', 2073600):
        "the s2d_rle_count_u8 row of this module",
}

TABLE = [
    ('add_bcast', 11304960, 11304960),
    ('add_bcast', 135659520, 135659520),
    ('add_bcast', 15073280, 15073280),
    ('add_bcast', 241172480, 241172480),
    ('add_bcast', 25600, 25600),
    ('add_bcast', 2826240, 2826240),
    ('add_bcast', 33914880, 33914880),
    ('add_bcast', 3768320, 3768320),
    ('add_bcast', 45219840, 45219840),
    ('add_bcast', 60293120, 60293120),
    ('add_bcast', 8478720, 8478720),
    ('attn_mask_bits', 1, 100, 12, 184, 320, 23, 40, 100, False),
    ('attn_mask_bits', 1, 100, 12, 184, 320, 46, 80, 100, False),
    ('attn_mask_bits', 1, 100, 12, 184, 320, 92, 160, 100, False),
    ('attn_mask_bits', 1, 100, 16, 184, 320, 23, 40, 100, False),
    ('attn_mask_bits', 1, 100, 16, 184, 320, 46, 80, 100, False),
    ('attn_mask_bits', 1, 100, 16, 184, 320, 92, 160, 100, False),
    ('attn_mask_bits', 1, 100, 36, 184, 320, 23, 40, 100, False),
    ('attn_mask_bits', 1, 100, 36, 184, 320, 46, 80, 100, False),
    ('attn_mask_bits', 1, 100, 36, 184, 320, 92, 160, 100, False),
    ('attn_mask_bits', 1, 100, 64, 184, 320, 23, 40, 100, False),
    ('attn_mask_bits', 1, 100, 64, 184, 320, 46, 80, 100, False),
    ('attn_mask_bits', 1, 100, 64, 184, 320, 92, 160, 100, False),
    ('conv2d_nhwc', 12, 184, 320, 128, 128, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 12, 184, 320, 256, 256, 3, 3, 1, 1, False, False, False, False, True),
    ('conv2d_nhwc', 12, 184, 320, 256, 512, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 12, 184, 320, 64, 64, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 12, 23, 40, 512, 512, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 12, 46, 80, 1024, 2048, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 12, 46, 80, 256, 256, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 12, 46, 80, 512, 512, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 12, 736, 1280, 4, 64, 7, 7, 2, 3, True, True, False, True, True),
    ('conv2d_nhwc', 12, 92, 160, 128, 128, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 12, 92, 160, 256, 256, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 12, 92, 160, 512, 1024, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 36, 184, 320, 128, 128, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 36, 184, 320, 256, 256, 3, 3, 1, 1, False, False, False, False, True),
    ('conv2d_nhwc', 36, 184, 320, 256, 512, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 36, 184, 320, 64, 64, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 36, 23, 40, 512, 512, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 36, 46, 80, 1024, 2048, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 36, 46, 80, 256, 256, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 36, 46, 80, 512, 512, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 36, 736, 1280, 4, 64, 7, 7, 2, 3, True, True, False, True, True),
    ('conv2d_nhwc', 36, 92, 160, 128, 128, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 36, 92, 160, 256, 256, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 36, 92, 160, 512, 1024, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 64, 184, 320, 128, 128, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 64, 184, 320, 256, 256, 3, 3, 1, 1, False, False, False, False, True),
    ('conv2d_nhwc', 64, 184, 320, 256, 512, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 64, 184, 320, 64, 64, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 64, 23, 40, 512, 512, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 64, 46, 80, 1024, 2048, 1, 1, 2, 0, True, True, False, False, True),
    ('conv2d_nhwc', 64, 46, 80, 256, 256, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 64, 46, 80, 512, 512, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 64, 736, 1280, 4, 64, 7, 7, 2, 3, True, True, False, True, True),
    ('conv2d_nhwc', 64, 92, 160, 128, 128, 3, 3, 1, 1, True, True, False, True, True),
    ('conv2d_nhwc', 64, 92, 160, 256, 256, 3, 3, 2, 1, True, True, False, True, True),
    ('conv2d_nhwc', 64, 92, 160, 512, 1024, 1, 1, 2, 0, True, True, False, False, True),
    ('ffn_fused', 1236480, 1024, True, True, None, False, (544, 19320, 288, 288), True),
    ('ffn_fused', 1236480, 1024, True, True, None, False, None, True),
    ('ffn_fused', 231840, 1024, True, True, None, False, (544, 19320, 288, 288), True),
    ('ffn_fused', 231840, 1024, True, True, None, False, None, True),
    ('ffn_fused', 309120, 1024, True, True, None, False, (544, 19320, 288, 288), True),
    ('ffn_fused', 309120, 1024, True, True, None, False, None, True),
    ('ffn_fused', 695520, 1024, True, True, None, False, (544, 19320, 288, 288), True),
    ('ffn_fused', 695520, 1024, True, True, None, False, None, True),
    ('gemm_nt', 1, 100, 2, 256, False, True, False, True, None, False, 2, None),
    ('gemm_nt', 1, 100, 2048, 256, False, True, False, True, None, True, None, None),
    ('gemm_nt', 1, 100, 256, 2048, False, True, False, True, (256, 0, 0, False), False, None, None),
    ('gemm_nt', 1, 100, 256, 256, False, True, False, True, (256, 0, 0, False), False, None, None),
    ('gemm_nt', 1, 100, 256, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 100, 256, 256, False, True, False, True, None, True, None, None),
    ('gemm_nt', 1, 100, 512, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 11040, 2048, 512, False, True, True, True, (2048, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 11040, 256, 2048, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 11040, 512, 2048, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 11040, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 1236480, 544, 256, False, True, False, True, (288, 19320, 288, False), False, None, None),
    ('gemm_nt', 1, 132480, 1024, 256, False, True, True, True, (1024, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 132480, 256, 1024, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 132480, 256, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 132480, 512, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 132480, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 176640, 128, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 176640, 256, 512, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 176640, 256, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 176640, 512, 128, False, True, True, True, (512, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 176640, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 2119680, 100, 256, True, False, False, False, None, False, 100, None),
    ('gemm_nt', 1, 2119680, 128, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 2119680, 256, 256, False, True, False, False, None, False, None, None),
    ('gemm_nt', 1, 2119680, 256, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 2119680, 256, 64, False, True, True, True, (256, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 2119680, 256, 64, False, True, True, True, None, False, None, None),
    ('gemm_nt', 1, 2119680, 64, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 2119680, 64, 64, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 231840, 544, 256, False, True, False, True, (288, 19320, 288, False), False, None, None),
    ('gemm_nt', 1, 235520, 1024, 256, False, True, True, True, (1024, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 235520, 256, 1024, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 235520, 256, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 235520, 512, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 33120, 2048, 512, False, True, True, True, (2048, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 33120, 256, 2048, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 33120, 512, 2048, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 33120, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 3768320, 100, 256, True, False, False, False, None, False, 100, None),
    ('gemm_nt', 1, 3768320, 128, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 3768320, 256, 256, False, True, False, False, None, False, None, None),
    ('gemm_nt', 1, 3768320, 256, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 3768320, 256, 64, False, True, True, True, (256, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 3768320, 256, 64, False, True, True, True, None, False, None, None),
    ('gemm_nt', 1, 3768320, 64, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 3768320, 64, 64, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 44160, 1024, 256, False, True, True, True, (1024, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 44160, 256, 1024, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 44160, 256, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 44160, 512, 1024, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 44160, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 529920, 128, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 529920, 256, 512, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 529920, 256, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 529920, 512, 128, False, True, True, True, (512, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 529920, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 58880, 2048, 512, False, True, True, True, (2048, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 58880, 256, 2048, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 58880, 512, 2048, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 695520, 544, 256, False, True, False, True, (288, 19320, 288, False), False, None, None),
    ('gemm_nt', 1, 706560, 100, 256, True, False, False, False, None, False, 100, None),
    ('gemm_nt', 1, 706560, 128, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 706560, 256, 256, False, True, False, False, None, False, None, None),
    ('gemm_nt', 1, 706560, 256, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 706560, 256, 64, False, True, True, True, (256, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 706560, 256, 64, False, True, True, True, None, False, None, None),
    ('gemm_nt', 1, 706560, 64, 256, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 706560, 64, 64, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 942080, 100, 256, True, False, False, False, None, False, 100, None),
    ('gemm_nt', 1, 942080, 128, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 942080, 256, 512, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 942080, 256, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 942080, 512, 128, False, True, True, True, (512, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 942080, 768, 256, False, True, False, True, None, False, None, None),
    ('groupnorm_nhwc', 12, 184, 320, 256, 32, (92, 160), False),
    ('groupnorm_nhwc', 12, 184, 320, 256, 32, None, True),
    ('groupnorm_nhwc', 12, 23, 40, 256, 32, None, False),
    ('groupnorm_nhwc', 12, 46, 80, 256, 32, None, False),
    ('groupnorm_nhwc', 12, 92, 160, 256, 32, None, False),
    ('groupnorm_nhwc', 36, 184, 320, 256, 32, (92, 160), False),
    ('groupnorm_nhwc', 36, 184, 320, 256, 32, None, True),
    ('groupnorm_nhwc', 36, 23, 40, 256, 32, None, False),
    ('groupnorm_nhwc', 36, 46, 80, 256, 32, None, False),
    ('groupnorm_nhwc', 36, 92, 160, 256, 32, None, False),
    ('groupnorm_nhwc', 64, 184, 320, 256, 32, (92, 160), False),
    ('groupnorm_nhwc', 64, 184, 320, 256, 32, None, True),
    ('groupnorm_nhwc', 64, 23, 40, 256, 32, None, False),
    ('groupnorm_nhwc', 64, 46, 80, 256, 32, None, False),
    ('groupnorm_nhwc', 64, 92, 160, 256, 32, None, False),
    ('infer_masks', 16, 184, 320, 100, 736, 1280, 720, 1280, 720, 1280, 10, False),
    ('infer_masks', 36, 184, 320, 100, 736, 1280, 720, 1280, 1080, 1920, 10, True),
    ('infer_masks', 40, 184, 320, 100, 736, 1280, 720, 1280, 720, 1280, 10, False),
    ('infer_masks', 64, 184, 320, 100, 736, 1280, 720, 1280, 720, 1280, 10, False),
    ('infer_select', 100, 2, 10),
    ('layernorm', 100, 256, False),
    ('mask_pair_counts', 10, 2332800),
    ('masked_attn', 1, 100, 100, 256, 8, False, False, 512, 256, False),
    ('masked_attn', 1, 100, 11040, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 132480, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 14720, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 176640, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 235520, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 33120, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 44160, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 529920, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 58880, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 1, 100, 942080, 256, 8, True, True, 768, 768, False),
    ('maxpool3x3s2', 12, 368, 640, 64, False),
    ('maxpool3x3s2', 36, 368, 640, 64, False),
    ('maxpool3x3s2', 64, 368, 640, 64, False),
    ('msda_fused_forward', 12, 256, ((23, 40), (46, 80), (92, 160)), 544, 544, 288, 8, 4),
    ('msda_fused_forward', 36, 256, ((23, 40), (46, 80), (92, 160)), 544, 544, 288, 8, 4),
    ('msda_fused_forward', 64, 256, ((23, 40), (46, 80), (92, 160)), 544, 544, 288, 8, 4),
    ('normalize_pad', 36, 720, 1280, 32),
    ('normalize_pad', 40, 720, 1280, 32),
    ('normalize_pad', 64, 720, 1280, 32),
    ('pe_sine', 12, 23, 40, 128, True),
    ('pe_sine', 12, 46, 80, 128, True),
    ('pe_sine', 12, 92, 160, 128, True),
    ('pe_sine', 16, 23, 40, 128, True),
    ('pe_sine', 16, 46, 80, 128, True),
    ('pe_sine', 16, 92, 160, 128, True),
    ('pe_sine', 36, 23, 40, 128, True),
    ('pe_sine', 36, 46, 80, 128, True),
    ('pe_sine', 36, 92, 160, 128, True),
    ('pe_sine', 64, 23, 40, 128, True),
    ('pe_sine', 64, 46, 80, 128, True),
    ('pe_sine', 64, 92, 160, 128, True),
    ('s2d_rle_count_u8', 1080, 1920),
    ('window_scatter_columns', 588800, 100, 100, 2355200, 1766400),
    ('window_scatter_columns', 824320, 100, 100, 2355200, 942080),
    ('window_scatter_columns', 942080, 100, 100, 2355200, 0),
]

# rows no scenario makes, asked for at eval sizes (module docstring)
EXTRA_ROWS = [
    ('infer_masks', 1036, 23, 40, 100, 96, 160, 90, 160, 1080, 1920, 1, True),             # T*oh*ow = 2 148 249 600 > 2^31: 64-bit branch
    # the 32-bit decomposition is unsigned, so it is still exact between 2^31 and 2^32: only past 2^32 does the branch matter
    ('infer_masks', 2072, 23, 40, 100, 96, 160, 90, 160, 1080, 1920, 1, True),             # T*oh*ow = 4 296 499 200 > 2^32
    # an output of another aspect than the image: s2y != s2x (equal at 1080 x 1920 from 720 x 1280), at the 12-frame window length
    ('infer_masks', 12, 184, 320, 100, 736, 1280, 720, 1280, 720, 1600, 10, True),
    ('pack_mask_bits', 10, 36 * 1080 * 1920),
    ('window_scatter_columns', 14 * 184 * 320, 104, 100, 40 * 184 * 320, 16 * 184 * 320),   # pad columns: ldq > Q
]


def test_table_covers_the_eval_scenarios():
    """every (entry point, signature) the four scenarios make is a row of TABLE, a row of the c4 forward TABLE (COVERED_BY_C4, which
    must be exactly the set of such rows) or named in COVERED_ELSEWHERE; every public name of ops.py has a signature or a reason"""
    from s2d_amd import ops
    assert not unknown_public_functions(ops), unknown_public_functions(ops)
    rec = record_eval_scenarios()
    seen = set(rec["log"])
    assert len(seen) > 100
    for name, d in rec["ms"].items():
        T = SCENARIOS[name]["T"]
        print(f"evaltime {name} T={T} wall {d['_wall']:.1f} ms " + " ".join(f"{k}={v / T:.4f}" for k, v in sorted(d.items()) if k != "_wall")
              + " (ms per frame, HIP events around the top-level calls)")
    table, c4 = set(TABLE), set(fc4.TABLE)
    assert len(table) == len(TABLE) and not table & c4
    assert set(COVERED_BY_C4) == seen & c4, (sorted((seen & c4) - set(COVERED_BY_C4), key=repr), sorted(set(COVERED_BY_C4) - seen, key=repr))
    for row in sorted(table - seen, key=repr):
        print("evaltable: row no longer made by a scenario:", row)
    missing = sorted(seen - table - c4 - set(COVERED_ELSEWHERE), key=repr)
    assert not missing, missing
    for row in COVERED_ELSEWHERE:
        assert row in seen, row


# --------------------------------------------------------------------------- float64 restatements
def _interp(x, size):
    return torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False)


def _two_stage(planes, padded, img_size, out_size):
    """planes [n, c, hm, wm] (any float dtype) -> [n, c, oh, ow]: bilinear to the padded size, crop to the image, bilinear to the
    output size unless it is the image size already -- inference_video's two F.interpolate calls"""
    v = _interp(planes, tuple(padded))[..., :img_size[0], :img_size[1]]
    return v if tuple(img_size) == tuple(out_size) else _interp(v, tuple(out_size))


def _mask_band(planes, dims, padded, img_size, out_size):
    """the sign band of the module docstring, from the inputs alone; planes [..., hm, wm]"""
    T, hm, wm = dims
    D = max(float((planes[..., 1:, :] - planes[..., :-1, :]).abs().max()), float((planes[..., :, 1:] - planes[..., :, :-1]).abs().max()))
    A = float(planes.abs().max())
    C = max(*padded, *out_size)
    return 2.0 ** -24 * (max(4 * C, 12 * max(hm, wm)) * D + 16 * A)


def _frame_chunks(T, per_frame, budget=1 << 26):
    step = max(1, budget // per_frame)
    return [(t, min(t + step, T)) for t in range(0, T, step)]


def _compare_masks(rep, name, masks, planes, dims, padded, img_size, out_size, band, cap=1e-3):
    """masks u8 [K,T,oh,ow] against the sign of the float64 two-stage resize of planes [K,T,hm,wm] f32, a few frames at a time;
    also torch's float32 pair of calls against the kernel.  -> nothing; failures go to rep.bad"""
    K, T = planes.shape[:2]
    oh, ow = out_size
    n_ex = n_wrong = n_dis = n_dis_out = 0
    for t0, t1 in _frame_chunks(T, K * oh * ow):
        pl = planes[:, t0:t1]
        v64 = _two_stage(pl.double(), padded, img_size, out_size)
        v32 = _two_stage(pl, padded, img_size, out_size)
        got = masks[:, t0:t1] != 0
        excl = v64.abs() < band
        n_ex += int(excl.sum())
        n_wrong += int(((got != (v64 > 0)) & ~excl).sum())
        dis = got != (v32 > 0)
        n_dis += int(dis.sum())
        n_dis_out += int((dis & ~excl).sum())
    total = K * T * oh * ow
    print(f"c4row {rep.row} {name}: band {band:.3e}, {n_ex} of {total} pixels excluded (share {n_ex / total:.3e}, cap {cap:.0e}), {n_wrong} wrong "
          f"outside the band; float32 torch and the kernel disagree on {n_dis} pixels, {n_dis_out} of them outside the band")
    if n_wrong or n_dis_out or not n_ex < cap * total:
        rep.bad.append((name, n_ex, n_wrong, n_dis_out))


def _pack_words(flat):
    """u8 / bool [K, n] -> int32 words [K, ceil(n / 32)] (bit i % 32 of word i / 32, tail bits zero), in torch, chunked"""
    K, n = flat.shape
    words = (n + 31) // 32
    out = torch.empty((K, words), device=flat.device, dtype=torch.int32)
    sh = torch.arange(32, device=flat.device, dtype=torch.int64)
    step = max(1, (1 << 27) // (32 * K))
    for w0 in range(0, words, step):
        w1 = min(w0 + step, words)
        seg = flat[:, w0 * 32:min(w1 * 32, n)] != 0
        if seg.shape[1] < (w1 - w0) * 32:
            seg = torch.nn.functional.pad(seg, (0, (w1 - w0) * 32 - seg.shape[1]))
        v = (seg.view(K, w1 - w0, 32).to(torch.int64) << sh).sum(-1)
        out[:, w0:w1] = torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)
    return out


def _pair_counts(flat):
    """bool [K, n] -> int64 [K, K] intersection counts: an integer product, chunked"""
    K, n = flat.shape
    out = torch.zeros((K, K), device=flat.device, dtype=torch.int64)
    step = max(1, (1 << 28) // (K * K))
    for i0 in range(0, n, step):
        seg = flat[:, i0:i0 + step]
        out += (seg[:, None, :] & seg[None, :, :]).sum(-1, dtype=torch.int64)
    return out


def _spaced_logits(g, n, C1):
    """[n, C1] float32 class logits whose softmax scores are pairwise apart by far more than 1e-5 relative: column 0 takes n values
    0.08 apart in shuffled order, the other columns small noise"""
    l = _rn(g, n, C1) * 0.01
    l[:, 0] = (torch.arange(n, device=DEV, dtype=F32) * 0.08 - 0.04 * n)[torch.randperm(n, device=DEV, generator=g)]
    return l


def _select_ref(cls, K):
    """float64 softmax[:, :-1], stable descending sort of the flat scores -> (scores, query, label, all sorted scores)"""
    C = cls.shape[1] - 1
    s = torch.softmax(cls.double(), -1)[:, :C].reshape(-1)
    v, i = torch.sort(s, descending=True, stable=True)
    return v[:K], (i[:K] // C).int(), (i[:K] % C).int(), v


# --------------------------------------------------------------------------- the eval-only cases
def _case_infer_select(rep, g, Qn, C1, K):
    """scores at rtol 1e-5 (test_select_masks_and_pair_counts_vs_oracle), query and label exact on logits whose float64 score gaps
    exceed that tolerance; a second input made of identical row pairs: every score has an exact tie, the lower flat index first"""
    from s2d_amd import ops
    for name, cls in (("distinct", _spaced_logits(g, Qn, C1)), ("ties", _spaced_logits(g, (Qn + 1) // 2, C1).repeat(2, 1)[:Qn].contiguous())):
        s, q, l = ops.infer_select(cls, K)
        s2, q2, l2 = ops.infer_select(cls, K)
        for a, b, n in ((s, s2, "scores"), (q, q2, "query"), (l, l2, "label")):
            rep.same(f"{name}: {n} second call", b, a)
        rs, rq, rl, allv = _select_ref(cls, K)
        gaps = (allv[:-1] - allv[1:])[:K + 1] / allv[:K + 1]
        distinct = gaps[gaps > 0]
        fc4._check(rep, f"{name}: input gaps {float(distinct.min()):.2e} > 2e-5 relative ({int((gaps == 0).sum())} exact ties among the first {K + 1})",
                   bool((distinct > 2e-5).all()) and (name == "ties") == bool((gaps == 0).any()))
        err = float(((s.double() - rs).abs() / rs).max())
        print(f"c4row {rep.row} {name}: scores max rel error {err:.3e} bound 1.000e-05")
        if not err < 1e-5:
            rep.bad.append((name, "scores", err))
        rep.same(f"{name}: query", q, rq)
        rep.same(f"{name}: label", l, rl)


def _case_infer_masks(rep, g, T, hm, wm, ldq, Hp, Wp, ih, iw, oh, ow, K, want_bits):
    """signs against the float64 two-stage resize outside the derived band (module docstring), excluded share < 1e-3; bytes and bit
    words agree, tail bits zero, bytes and words behind the last element untouched; the unselected and pad columns of the pixel-major
    logits hold NaN (a read of the wrong column gives an empty mask)"""
    from s2d_amd import ops
    dims, padded, img, out = (T, hm, wm), (Hp, Wp), (ih, iw), (oh, ow)
    planes = fc4._smooth_logits(g, K * T, hm, wm, amp=3.0).view(K, T, hm, wm)
    query = torch.randperm(min(Q, ldq), device=DEV, generator=g)[:K].int()
    pm = torch.full((T * hm * wm, ldq), float("nan"), device=DEV)
    pm[:, query.long()] = planes.reshape(K, -1).t()
    band = _mask_band(planes, dims, padded, img, out)
    masks, bits = ops.infer_masks(pm, dims, padded, img, out, query, want_bits=want_bits)
    N = T * oh * ow
    words = (N + 31) // 32
    fc4._check(rep, f"index branch: N = {N} {'>=' if N >= 2 ** 31 else '<'} 2^31, {'SAME' if img == out else 'two-stage'} template", True)
    again = ops.infer_masks(pm, dims, padded, img, out, query, want_bits=want_bits)
    rep.same("bytes second call", again[0], masks)
    if want_bits:
        rep.same("bit words second call", again[1], bits)
    del again
    # third call, straight through the C ABI into buffers with a sentinel behind the last element
    L = ops.lib()
    ws = torch.empty((L.call("s2d_infer_workspace_floats", K, T, hm, wm),), device=DEV)
    m2 = torch.full((K * N + 64,), 7, device=DEV, dtype=torch.uint8)
    b2 = torch.full((K * words + 4,), 0x5A5A5A5A, device=DEV, dtype=torch.int32) if want_bits else None
    L.call("s2d_infer_masks_u8", pm, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, query, K, ws, m2, b2, ops._stream())
    rep.same("bytes through the C ABI", m2[:K * N].view(K, T, oh, ow), masks)
    fc4._check(rep, "bytes behind the last element untouched", bool((m2[K * N:] == 7).all()))
    fc4._check(rep, "bytes are 0 / 1", int(masks.max()) <= 1)
    del m2, ws
    if want_bits:
        rep.same("bit words through the C ABI", b2[:K * words].view(K, words), bits)
        fc4._check(rep, "words behind the last one untouched", bool((b2[K * words:] == 0x5A5A5A5A).all()))
        del b2
        rep.same("bit words == packed bytes (tail bits zero)", bits, _pack_words(masks.view(K, N)))
    _compare_masks(rep, "signs", masks, planes, dims, padded, img, out, band)


def _case_pack_mask_bits(rep, g, K, n):
    """exact: word i / 32, bit i % 32 = (byte != 0), tail bits zero; bytes take the values 0, 1 and others"""
    from s2d_amd import ops
    m = torch.randint(0, 4, (K, n), device=DEV, generator=g, dtype=torch.uint8) * 85            # 0, 85, 170, 255
    m[0] = 0; m[K - 1] = 1
    bits = ops.pack_mask_bits(m)
    rep.same("second call", ops.pack_mask_bits(m), bits)
    rep.same("bit words", bits, _pack_words(m))


def _case_mask_pair_counts(rep, g, K, words):
    """exact against the integer product of the unpacked masks (test_select_masks_and_pair_counts_vs_oracle: array equality); masks of
    different densities, an empty one and a full one among them"""
    from s2d_amd import ops
    n = words * 32
    dens = torch.linspace(0.05, 0.9, K, device=DEV)[:, None]
    m = torch.rand((K, n), device=DEV, generator=g) < dens
    if K > 2:
        m[1] = False; m[2] = True
    bits = _pack_words(m)
    inter = ops.mask_pair_counts(bits)
    rep.same("second call", ops.mask_pair_counts(bits), inter)
    rep.same("counts", inter, _pair_counts(m))


def _case_window_scatter_columns(rep, g, rows, ldq, Qn, R, row0):
    """exact against index_select: dst[row0 + r, p] = src[r, perm[p]], pad columns copied, rows outside [row0, row0 + rows) keep a
    sentinel; src is a row-offset view, as the stitching passes the owned rows of a window"""
    from s2d_amd import ops
    hw = 184 * 320
    src = _rn(g, rows + OVERLAP * hw, ldq)[OVERLAP * hw:]
    perm = torch.randperm(Qn, device=DEV, generator=g)
    dst = torch.full((R, ldq), 7.0, device=DEV)
    ops.window_scatter_columns(src, perm.int(), dst, row0, Qn)
    ref = torch.cat([src.index_select(1, perm), src[:, Qn:]], 1)
    rep.same("owned rows (query columns permuted, pad columns copied)", dst[row0:row0 + rows], ref)
    fc4._check(rep, "rows outside keep the sentinel", bool((dst[:row0] == 7.0).all()) and bool((dst[row0 + rows:] == 7.0).all()))
    fc4._check(rep, f"{ldq - Qn} pad columns", ldq >= Qn)
    first = dst.clone()
    ops.window_scatter_columns(src, perm.int(), dst, row0, Qn)
    rep.same("second call", dst, first)


_RLE_EXACT_FRAMES = (0, 1, 17, -1)


def _case_s2d_rle_count_u8(rep, g, H, W):
    """exact: rle.encode (count, positions, strings) on K = 4 x T = 36 masks of H x W made by infer_masks from smooth fields, frame 0
    emptied and frame 1 filled; see the module docstring for what is compared on which frames"""
    from oracle import oracle_np
    from s2d_amd import ops, rle
    K, T, hm, wm = 4, 36, 184, 320
    planes = fc4._smooth_logits(g, K * T, hm, wm, amp=3.0)
    pm = planes.view(K, T * hm * wm).t().contiguous()
    pm = torch.nn.functional.pad(pm, (0, 100 - K))
    query = torch.arange(K, device=DEV, dtype=torch.int32)
    masks, _ = ops.infer_masks(pm, (T, hm, wm), (736, 1280), (720, 1280), (H, W), query)
    masks = masks.view(K * T, H, W)
    masks[0] = 0; masks[1] = 1
    rles, areas, boxes = rle.encode(masks)
    r2, a2, b2 = rle.encode(masks)
    fc4._check(rep, "second call", [r["counts"] for r in r2] == [r["counts"] for r in rles] and np.array_equal(a2, areas) and np.array_equal(b2, boxes))
    host = masks.cpu().numpy()
    bad_dec = bad_area = bad_box = 0
    for f in range(K * T):
        bad_dec += not np.array_equal(oracle_np.rle_decode(rles[f]), host[f])
        a, b = oracle_np.rle_area_bbox(host[f])
        bad_area += int(areas[f]) != a
        bad_box += list(boxes[f]) != b
    print(f"c4row {rep.row} {K * T} frames of {H} x {W}: {bad_dec} strings do not decode to the mask, {bad_area} areas, {bad_box} boxes differ; "
          f"{sum(len(r['counts']) for r in rles)} characters")
    if bad_dec or bad_area or bad_box or any(r["size"] != [H, W] for r in rles):
        rep.bad.append(("rle", bad_dec, bad_area, bad_box))
    for f in _RLE_EXACT_FRAMES:
        fc4._check(rep, f"frame {f % (K * T)}: string == oracle_np.rle_encode", oracle_np.rle_encode(host[f])[0]["counts"] == rles[f]["counts"])


def _rows():
    return [r for r in TABLE + EXTRA_ROWS if r[0] not in fc4.NO_ROWS]


@pytest.mark.parametrize("row", _rows(), ids=_row_id)
def test_eval_row_vs_float64(row):
    from s2d_amd import ops
    case = globals().get("_case_" + row[0]) or getattr(fc4, "_case_" + row[0])
    rep = _Rep(row)
    timer = _Timer()
    from s2d_amd import rle
    holder, attr = (ops, row[0]) if hasattr(ops, row[0]) else (rle, "encode") if row[0].startswith("s2d_rle") else (None, None)
    orig = getattr(holder, attr) if holder is not None else None
    if orig is not None:                                                  # the time of the row's second call (rle rows: of rle.encode)
        setattr(holder, attr, timer.wrap(attr, orig))
    old = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False      # the float32 restatement is plain float32
    try:
        case(rep, _gen(row), *row[1:])
        torch.cuda.synchronize()
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old
        if orig is not None:
            setattr(holder, attr, orig)
    if len(timer.pairs) > 1:
        print(f"c4row {rep.row} second call: {timer.pairs[1][1].elapsed_time(timer.pairs[1][2]):.3f} ms (HIP events)")
    elif timer.pairs:
        print(f"c4row {rep.row} only call: {timer.pairs[0][1].elapsed_time(timer.pairs[0][2]):.3f} ms (HIP events)")
    rep.done()
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------- composition at size
def _greedy_nms(inter, labels, thr):
    """greedy same-label mask NMS on exact counts, candidates in descending score order; IoU in float64"""
    K = len(labels)
    keep, dead = [], set()
    for i in range(K):
        if i in dead:
            continue
        keep.append(i)
        for j in range(i + 1, K):
            if j in dead or labels[j] != labels[i]:
                continue
            u = inter[i][i] + inter[j][j] - inter[i][j]
            if u > 0 and inter[i][j] / u > thr:
                dead.add(j)
    return keep


@pytest.mark.parametrize("name", ["S36", "W40"])
def test_composition_at_size(name):
    """the logits inference_video was handed under the scenario -> float64 restatement of inference_video (softmax top-K, two-stage
    resize, greedy NMS on exact counts) against what model([video]) returned: labels and kept set equal, scores at rtol 1e-5
    (test_inference_video_golden), masks equal outside the band.  The sizes are the ones _inference must have passed: padded
    736 x 1280, image 720 x 1280, output height x width of the video dict"""
    from oracle import oracle_np
    rec = record_eval_scenarios()
    cap, out = rec[name]
    sc = SCENARIOS[name]
    T = sc["T"]
    out_size = (sc.get("height", H0), sc.get("width", W0))
    rep = _Rep((name, "composition"))
    cls, ml = cap["cls"], cap["ml"]
    dims, padded, img = (T, 184, 320), (736, 1280), (H0, W0)
    fc4._check(rep, "sizes handed to inference_video", (tuple(cap["dims"]), tuple(cap["padded"]), tuple(cap["img_size"]), tuple(cap["out_size"]))
               == (dims, padded, img, out_size) and out["image_size"] == out_size)
    rs, rq, rl, _ = _select_ref(cls, NPRED)
    planes = ml[:, rq.long()].t().contiguous().view(NPRED, T, 184, 320)
    band = _mask_band(planes, dims, padded, img, out_size)
    oh, ow = out_size
    ref = torch.empty((NPRED, T, oh, ow), device=DEV, dtype=torch.bool)
    excl = torch.empty_like(ref)
    for t0, t1 in _frame_chunks(T, NPRED * oh * ow):
        v = _two_stage(planes[:, t0:t1].double(), padded, img, out_size)
        ref[:, t0:t1], excl[:, t0:t1] = v > 0, v.abs() < band
    keep = list(range(NPRED))
    if sc.get("use_nms"):
        inter = _pair_counts(ref.view(NPRED, -1)).tolist()
        keep = _greedy_nms(inter, rl.tolist(), 0.75)
        print(f"c4row {rep.row} NMS keeps {keep} of {NPRED}")
    fc4._check(rep, "kept set (number of predictions)", len(out["pred_scores"]) == len(keep) == len(out["pred_masks"]))
    fc4._check(rep, "labels", out["pred_labels"] == [int(rl[k]) for k in keep])
    got_s = torch.tensor(out["pred_scores"], dtype=F64, device=DEV)
    if len(keep) == got_s.numel():
        err = float(((got_s - rs[keep]).abs() / rs[keep]).max())
        print(f"c4row {rep.row} scores max rel error {err:.3e} bound 1.000e-05")
        if not err < 1e-5:
            rep.bad.append(("scores", err))
        n_ex = n_wrong = 0
        for i, k in enumerate(keep):
            if sc.get("inference_rle"):
                m = torch.from_numpy(np.stack([oracle_np.rle_decode(r) for r in out["pred_masks"][i]])).to(DEV) != 0
            else:
                m = out["pred_masks"][i].to(DEV) != 0
            n_ex += int(excl[k].sum())
            n_wrong += int(((m != ref[k]) & ~excl[k]).sum())
        total = len(keep) * T * oh * ow
        print(f"c4row {rep.row} masks: band {band:.3e}, {n_ex} of {total} pixels excluded (share {n_ex / total:.3e}, cap 1e-03), {n_wrong} wrong outside the band")
        if n_wrong or not n_ex < 1e-3 * total:
            rep.bad.append(("masks", n_ex, n_wrong))
    rep.done()


