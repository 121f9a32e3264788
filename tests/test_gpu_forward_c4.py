"""Forward kernels at the shapes of the benchmarked c4 step (2 clips x T=8 x 720p, Q=100, P=160 000, encoder dropout 0.3), each compared
with a float64 restatement of the same operation written here in plain torch on the device (nothing of s2d_amd / libs2d_hip.so in the
reference).  The forward counterpart of tests/test_gpu_backward_c4.py, whose vocabulary (TABLE, recording, `c4row` lines, rel) and helpers
it shares by importing them.

TABLE is the set of (entry point of s2d_amd/ops.py, shape signature) pairs ONE step of the model bench.py builds for c4 makes under BOTH
forward paths: `forward_losses` (the metric: fused forward-only launches, teacher with aux_masks=False) and `forward_backward` (the taped
path: gemm_nt(dropout=) + layernorm where the metric path runs ffn_fused).  Entry points of s2d_amd/backward.py are not recorded (a call
into ops from inside one belongs to it; tests/test_gpu_backward_c4.py has them); the calls the model's own backward methods make straight
into ops (the regenerated dropout masks, the mask-feature gradient GEMM, s2d_transpose_f32) are.  test_table_covers_the_c4_step re-records
the step and fails when it calls something the table does not hold, or when ops.py has a public name that has neither a signature here
nor an entry in NOT_KERNELS.

Every row runs the kernel at full size on seeded float32 operands of the recorded shapes and strides, the float64 restatement, and the
SAME restatement in float32 through torch.  Bound of a row: max(bound the small-size test asserts for that function in the default f16x3
mode, 2 x the float32-torch error on these operands) -- the factor 2 covers the dropped low x low term of the split-fp16 x3 product and
another summation order; it is never read off the kernel's own output.  Where the small test asserts a catch-all for every dense mode
(test_gemm_nt, test_conv_nhwc, test_conv3x3_halo: 1e-4) the f16x3 figure of the neighbouring static-weight test is used; each case names
the test its figure comes from.  Metric: `rel` of tests/test_gpu_backward.py (max abs error / max abs reference); contractions also print
the scale-invariant error of tests/test_gpu_split_range.py (max|C - C_ref| / max(|A| . |B|)).  A second call of every row is bitwise equal
to the first, and where a recorded row has an in-process opt-out form that form meets the same bound against the same reference on the
same operands: S2D_CONV_HALO_PIPE for the 3 x 3 rows, and inside the ffn_fused rows the launches the encoder layer makes with fuse_pre /
fuse_next / fuse_ffn = False (the attention's own gemm_nt(res, dropout) feeding ffn_fused without `pre`; ffn_fused without `post`
followed by gemm_nt with the row-periodic pos residual; layernorm + gemm_nt(dropout) x 2 + layernorm).  Dropout masks come from oracle.dropout_multipliers (numpy Philox, pinned by Random123's vectors in
tests/test_oracle.py).  Sign outputs (attn_mask_bits, the kd_targets planes) are compared with the sign of the float64 bilinear
interpolation outside a band of 2^-20 x the largest input logit around zero: a four-tap float32 bilinear sum carries a few units of 2^-24
of the largest tap, so only there may a float32 evaluation legitimately land on the other side (derived, not measured on the kernel).
The figures of one run are in profiles/c4_forward_parity.txt (the `c4row` lines this module prints).

matcher_cost, lsap and point_loss have signatures (the coverage test accounts for them) but no rows: tests/test_gpu_c4_oracle.py checks
them in isolation at this size.  gemm_nt_presplit and the direct s2d_normalize_pad_nhwc4_f32 call (clips of different sizes) have
signatures but the c4 step never makes them.

No frame subset is needed for the convolution rows: their restatement is one matmul per tap on strided views of the zero-padded input (as
the backward module restates the convolution gradients), which is fast in float64, so all N frames are compared."""
import contextlib

import numpy as np
import pytest
import torch

from tests.test_gpu_backward_c4 import DEV, F32, F64, _Rep, _gen, _out_hw, _pack_bits, _rn, _row_id, _sh

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- shape signatures (what selects a kernel and a branch; no data)
def _static(B):
    """does ops._static_split hand the launch a cached pre-split image of B (a parameter or a module's packed copy)"""
    base = B._base if B._base is not None else B
    return bool(isinstance(base, torch.nn.Parameter) or getattr(base, "_s2d_static", False) or getattr(B, "_s2d_static", False))


def _drop(dropout, n):
    """None, or row0 of the mask (dropout = (p, seed, site.., [row0]) with n leading entries)"""
    if dropout is None or not dropout[0] > 0.0:
        return None
    return int(dropout[n]) if len(dropout) > n else 0


def _sig_gemm_nt(A, B, scale=None, bias=None, res=None, relu=False, out=None, res_rows=0, res_cols=0, dropout=None):
    bs = A.shape[0] if A.dim() == 3 else 1
    r = None if res is None else (int(res.shape[-1]), int(res_rows), int(res_cols), res.dim() == 3)
    return (bs, A.shape[-2], B.shape[-2], A.shape[-1], B.dim() == 3, _static(B), scale is not None, bias is not None, r, bool(relu),
            None if out is None else int(out.shape[-1]), _drop(dropout, 3))


def _sig_gemm_nt_presplit(A_split, M, K, B, bias=None, res=None, relu=False, out=None, res_rows=0, res_cols=0):
    r = None if res is None else (int(res.shape[-1]), int(res_rows), int(res_cols))
    return (M, B.shape[0], K, bias is not None, r, bool(relu), None if out is None else int(out.shape[-1]))


def _sig_conv2d_nhwc(x, w, stride=1, pad=0, scale=None, bias=None, res=None, relu=False):
    return _sh(x) + (w.shape[0], w.shape[1], w.shape[2], stride, pad, scale is not None, bias is not None, res is not None, bool(relu), _static(w))


def _sig_ffn_fused(x, W1, b1, W2, b2, ln1=None, ln2=None, dropout=None, eps=1e-5, want_xn=False, post=None, pre=None):
    po = None
    if post is not None:
        pp = post[2]
        po = (post[0].shape[0],) + ((0, 0, 0) if pp is None else (int(pp.shape[0]), int(pp.shape[1]), int(pp.stride(0))))
    return (x.shape[0], W1.shape[0], ln1 is not None, ln2 is not None, _drop(dropout, 4), bool(want_xn), po, pre is not None)


def _sig_msda_fused_forward(value, shapes, offs_logits, M=8, P=4):
    sh = tuple(tuple(int(v) for v in r) for r in torch.as_tensor(np.asarray(shapes)).tolist())
    return (value.shape[0], value.shape[2], sh, int(value.stride(1)), int(offs_logits.stride(1)), offs_logits.shape[2], M, P)


def _sig_masked_attn(q, k, v, bits=None, unmasked=None, H=8, want_lse=False):
    B, Q, C = q.shape
    return (B, Q, k.shape[1], C, H, bits is not None, unmasked is not None, int(k.stride(1)), int(v.stride(1)), bool(want_lse))


def _sig_attn_mask_bits(mask_logits, B, Q, T, hm, wm, hl, wl, compact=False):
    return (B, Q, T, hm, wm, hl, wl, int(mask_logits.shape[-1]), bool(compact))


def _sig_attn_mask_tap_index(T, hm, wm, hl, wl, device):
    return (T, hm, wm, hl, wl)


def _sig_groupnorm_nhwc(x, G, gamma, beta, up=None, relu=False, eps=1e-5):
    return _sh(x) + (G, None if up is None else (int(up.shape[1]), int(up.shape[2])), bool(relu))


def _sig_layernorm(x, gamma, beta, res=None, eps=1e-5):
    C = x.shape[-1]
    return (x.numel() // C, C, res is not None)


def _sig_maxpool3x3s2(x, want_idx=False):
    return _sh(x) + (bool(want_idx),)


def _sig_normalize_pad(frames_u8, div=32, mean=None, std=None):
    return (frames_u8.shape[0], frames_u8.shape[2], frames_u8.shape[3], div)


def _sig_add_bcast(x, b):
    return (x.numel(), b.numel())


def _sig_pe_sine(T, H, W, num_pos_feats=128, add_c=None, device="cuda"):
    return (T, H, W, num_pos_feats, add_c is not None)


def _sig_dropout_apply(x, p, seed, site, row0=0, out=None):
    return (x.shape[0], x.shape[1], int(row0), out is not None)


def _sig_kd_targets(t_class_logits, t_mask_logits, dims, H, W, Nmax, thr=0.75, topk=100, want_labels=False):
    return (t_class_logits.shape[0], t_class_logits.shape[2]) + tuple(int(v) for v in dims) + (int(t_mask_logits.shape[-1]), H, W, Nmax, int(topk), bool(want_labels))


def _sig_class_loss(class_logits, idx_q, n_match, eos_coef=0.1):
    return _sh(class_logits) + (idx_q.shape[-1],)


def _sig_target_nonempty(tgt, count):
    return _sh(tgt)


def _sig_matcher_cost(mask_logits, class_logits, tgt, tgt_count, dims, P, weights, coords=None, seed=0):
    return _sh(mask_logits) + (class_logits.shape[-1],) + _sh(tgt)[1:] + (int(P), coords is not None)


def _sig_lsap(C, tgt_count, B):
    return _sh(C) + (B,)


def _sig_point_loss(mask_logits, tgt, tgt_count, nonempty, idx_q, idx_t, n_match, dims, P, oversample=3.0, importance=0.75, coords_over=None,
                    coords_rand=None, seed=0, drop_empty=True, world_size=1.0, keep=False):
    return _sh(mask_logits) + _sh(tgt)[1:] + (idx_q.shape[-1], int(P), coords_over is not None, bool(drop_empty), bool(keep))


# the two library calls the model makes outside ops (meta_arch._normalize_batch, VideoDecoder's mask-feature gradient): recorded at lib().call
def _sig_s2d_normalize_pad_nhwc4_f32(x, n, h, w, Hp, Wp, mean, std, out, stream):
    return (n, h, w, Hp, Wp)


def _sig_s2d_transpose_f32(src, rows, cols, lds, dst, ldd, stream):
    return (rows, cols, lds, ldd)


LIB_CALLS = {"s2d_normalize_pad_nhwc4_f32": _sig_s2d_normalize_pad_nhwc4_f32, "s2d_transpose_f32": _sig_s2d_transpose_f32}
ENTRY_POINTS = {n[5:]: f for n, f in list(globals().items()) if n.startswith("_sig_") and n[5:] not in LIB_CALLS}
ALIASES = {"dropout": "dropout_apply"}                    # ops.dropout is ops.dropout_apply
NO_ROWS = {"matcher_cost", "lsap", "point_loss"}           # tests/test_gpu_c4_oracle.py checks them in isolation at this size
# public names of ops.py that are no forward entry point of the training step, each with its reason
NOT_KERNELS = {
    "lib": "the binding, imported",
    "version_of": "cache management", "bump_version": "cache management", "repack": "cache management", "mark_static": "cache management",
    "clear_weight_cache": "cache management",
    "set_dense_mode": "process-wide arithmetic switch (tests/test_gpu_dense.py walks the modes)",
    "amp_fp16": "context manager; the c4 step runs fp32-class arithmetic", "amp_active": "state query",
    "gate_fusable": "capability query", "ffn_fusable": "capability query", "dropout_scale": "host arithmetic", "next_dropout_seed": "host arithmetic",
    "gemm_nt_gate": "backward epilogue form: reached through backward.input_grad (tests/test_gpu_backward_c4.py rows with a gate)",
    "conv2d_nhwc_gate": "backward epilogue form: reached through backward.conv_input_grad (tests/test_gpu_backward_c4.py)",
    "split_rows": "feeds gemm_nt_presplit, which the step does not call",
    "msda_forward": "the reference's general MSDeformAttn signature; the step runs msda_fused_forward",
    "msda_backward": "backward of msda_forward", "msda_forward_dev": "drop-in op with device-side shapes; not in the step",
    "msda_backward_dev": "backward of msda_forward_dev", "msda_dev_status": "status read-back of the *_dev ops",
    "point_loss_kept_rows": "read-back of point_loss's workspace", "point_loss_backward": "backward (tests/test_gpu_backward.py)",
    "class_loss_backward": "backward (tests/test_gpu_backward.py)",
    "infer_select": "eval path: signature and float64 rows in tests/test_gpu_eval_720p.py", "infer_masks": "eval path: tests/test_gpu_eval_720p.py",
    "pack_mask_bits": "eval path / evaluator: tests/test_gpu_eval_720p.py", "mask_pair_counts": "eval path: tests/test_gpu_eval_720p.py",
    "window_pair_counts": "windowed inference: tests/test_gpu_eval_720p.py records it, tests/test_gpu_window_inference.py checks it at that size",
    "window_scatter_columns": "windowed inference: tests/test_gpu_eval_720p.py", "mask_frame_areas": "demo rendering",
    "render_instances": "demo rendering",
}


def unknown_public_functions(ops):
    """public functions and classes of s2d_amd/ops.py the recorder has no signature for: a new entry point must not pass unseen"""
    import inspect
    public = {n for n, f in vars(ops).items() if not n.startswith("_") and (inspect.isfunction(f) or inspect.isclass(f))
              and getattr(f, "__module__", None) in (ops.__name__, "s2d_amd._lib")}
    return sorted(public - set(ENTRY_POINTS) - set(ALIASES) - set(NOT_KERNELS))


@contextlib.contextmanager
def recording(ops, log, backward=None, entry_points=None, lib_calls=None):
    """wrap every forward entry point of s2d_amd.ops (and lib().call for LIB_CALLS) with a recorder of its shape signature; a call made from
    inside another recorded entry point belongs to the outer row, and so does everything inside an entry point of `backward`.
    entry_points / lib_calls: the caller's own {name: signature function} maps in place of ENTRY_POINTS / LIB_CALLS (tests/
    test_gpu_eval_720p.py records the eval path with the maps of this module plus its own)"""
    from tests import test_gpu_backward_c4 as bc4
    entry_points = ENTRY_POINTS if entry_points is None else entry_points
    lib_calls = LIB_CALLS if lib_calls is None else lib_calls
    saved, depth = [], [0]

    def wrap(name, fn, sig):
        def rec(*a, **k):
            if depth[0] == 0 and sig is not None:
                log.append((name,) + tuple(sig(*a, **k)))
            depth[0] += 1
            try:
                return fn(*a, **k)
            finally:
                depth[0] -= 1
        return rec

    def patch(obj, attr, new):
        saved.append((obj, attr, getattr(obj, attr)))
        setattr(obj, attr, new)

    for name, sig in entry_points.items():
        patch(ops, name, wrap(name, getattr(ops, name), sig))
    for alias, name in ALIASES.items():
        patch(ops, alias, getattr(ops, name))
    if backward is not None:
        for name in bc4.ENTRY_POINTS:
            patch(backward, name, wrap(name, getattr(backward, name), None))
    L = ops.lib()
    raw = L.call

    def call(name, *a):
        if depth[0] == 0 and name in lib_calls:
            log.append((name,) + tuple(lib_calls[name](*a)))
        return raw(name, *a)
    L.call = call                                            # instance attribute in front of the class's method
    try:
        yield log
    finally:
        del L.call
        for obj, attr, fn in reversed(saved):
            setattr(obj, attr, fn)


def record_c4_step():
    """the c4 model as bench.py builds it, ONE forward_losses and ONE forward_backward under the recorder -> the list of signatures"""
    import bench
    from s2d_amd import backward, ops
    from s2d_amd.modeling import TargetSet, build_kd_model
    dev = torch.device(DEV)
    B, T, H0, W0, Q, P, N = bench.CONFIGS["c4"]
    model = build_kd_model(num_queries=Q, num_frames=T, num_points=P, dropout=0.3).to(dev)
    frames, masks = bench.synth_batch(0, B, T, H0, W0, N, dev)
    bench.calibrate_teacher(model, ops.normalize_pad(frames))
    assert model.teacher_aux_masks is False
    log = []
    with recording(ops, log, backward):
        for step in (model.forward_losses, model.forward_backward):
            model.criterion.seed = 0; model.criterion.matcher.seed = 0
            torch.manual_seed(5); ops._DROP_CALLS[0] = 0
            step(ops.normalize_pad(frames), TargetSet.from_list(masks, device=dev))
            torch.cuda.synchronize()
    model.last_tapes = None
    del model, frames, masks
    return log


# --------------------------------------------------------------------------- the c4 step (recorded; see test_table_covers_the_c4_step)
TABLE = [
    ('add_bcast', 15073280, 7536640),
    ('add_bcast', 3768320, 1884160),
    ('add_bcast', 51200, 25600),
    ('add_bcast', 60293120, 30146560),
    ('attn_mask_bits', 2, 100, 8, 184, 320, 23, 40, 100, False),
    ('attn_mask_bits', 2, 100, 8, 184, 320, 23, 40, 100, True),
    ('attn_mask_bits', 2, 100, 8, 184, 320, 46, 80, 100, False),
    ('attn_mask_bits', 2, 100, 8, 184, 320, 46, 80, 100, True),
    ('attn_mask_bits', 2, 100, 8, 184, 320, 92, 160, 100, False),
    ('attn_mask_tap_index', 8, 184, 320, 23, 40),
    ('attn_mask_tap_index', 8, 184, 320, 46, 80),
    ('class_loss', 2, 100, 2, 10),
    ('class_loss', 2, 100, 2, 100),
    ('class_loss', 2, 100, 2, 12),
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
    ('dropout_apply', 309120, 256, 0, False),
    ('ffn_fused', 309120, 1024, True, True, 0, False, (544, 19320, 288, 288), True),
    ('ffn_fused', 309120, 1024, True, True, 0, False, None, True),
    ('gemm_nt', 1, 1, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 14720, 2048, 512, False, True, True, True, (2048, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 14720, 256, 2048, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 14720, 512, 2048, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 14720, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 19320, 288, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 200, 2, 256, False, True, False, True, None, False, 2, None),
    ('gemm_nt', 1, 200, 2048, 256, False, True, False, True, None, True, None, None),
    ('gemm_nt', 1, 200, 256, 2048, False, True, False, True, (256, 0, 0, False), False, None, None),
    ('gemm_nt', 1, 200, 256, 256, False, True, False, True, (256, 0, 0, False), False, None, None),
    ('gemm_nt', 1, 200, 256, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 200, 256, 256, False, True, False, True, None, True, None, None),
    ('gemm_nt', 1, 200, 512, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 235520, 128, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 235520, 256, 512, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 235520, 256, 512, False, True, True, True, None, True, None, None),
    ('gemm_nt', 1, 235520, 512, 128, False, True, True, True, (512, 0, 0, False), True, None, None),
    ('gemm_nt', 1, 235520, 768, 256, False, True, False, True, None, False, None, None),
    ('gemm_nt', 1, 309120, 1024, 256, False, True, False, True, None, True, None, 0),
    ('gemm_nt', 1, 309120, 256, 1024, False, True, False, True, (256, 0, 0, False), False, None, 0),
    ('gemm_nt', 1, 309120, 256, 256, False, True, False, True, (256, 0, 0, False), False, None, 0),
    ('gemm_nt', 1, 309120, 544, 256, False, True, False, True, (288, 19320, 288, False), False, None, None),
    ('gemm_nt', 1, 471040, 256, 120, False, False, False, False, (256, 0, 0, False), False, 256, None),
    ('gemm_nt', 1, 471040, 256, 120, False, False, False, False, None, False, 256, None),
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
    ('gemm_nt', 2, 117760, 100, 256, True, False, False, False, None, False, None, None),
    ('gemm_nt', 2, 29440, 100, 256, True, False, False, False, None, False, None, None),
    ('gemm_nt', 2, 471040, 100, 256, True, False, False, False, None, False, 100, None),
    ('groupnorm_nhwc', 16, 184, 320, 256, 32, (92, 160), False),
    ('groupnorm_nhwc', 16, 184, 320, 256, 32, None, True),
    ('groupnorm_nhwc', 16, 23, 40, 256, 32, None, False),
    ('groupnorm_nhwc', 16, 46, 80, 256, 32, None, False),
    ('groupnorm_nhwc', 16, 92, 160, 256, 32, None, False),
    ('kd_targets', 2, 2, 100, 8, 184, 320, 100, 736, 1280, 100, 100, True),
    ('layernorm', 200, 256, False),
    ('layernorm', 309120, 256, False),
    ('lsap', 20, 100, 10, 2),
    ('lsap', 20, 100, 100, 2),
    ('lsap', 20, 100, 12, 2),
    ('masked_attn', 2, 100, 100, 256, 8, False, False, 512, 256, False),
    ('masked_attn', 2, 100, 100, 256, 8, False, False, 512, 256, True),
    ('masked_attn', 2, 100, 117760, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 2, 100, 117760, 256, 8, True, True, 768, 768, True),
    ('masked_attn', 2, 100, 29440, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 2, 100, 29440, 256, 8, True, True, 768, 768, True),
    ('masked_attn', 2, 100, 7360, 256, 8, True, True, 768, 768, False),
    ('masked_attn', 2, 100, 7360, 256, 8, True, True, 768, 768, True),
    ('matcher_cost', 10, 2, 471040, 100, 2, 10, 8, 736, 1280, 160000, False),
    ('matcher_cost', 10, 2, 471040, 100, 2, 100, 8, 736, 1280, 160000, False),
    ('matcher_cost', 10, 2, 471040, 100, 2, 12, 8, 736, 1280, 160000, False),
    ('maxpool3x3s2', 16, 368, 640, 64, False),
    ('maxpool3x3s2', 16, 368, 640, 64, True),
    ('msda_fused_forward', 16, 256, ((23, 40), (46, 80), (92, 160)), 544, 544, 288, 8, 4),
    ('normalize_pad', 16, 720, 1280, 32),
    ('pe_sine', 0, 23, 40, 128, True),
    ('pe_sine', 0, 46, 80, 128, True),
    ('pe_sine', 0, 92, 160, 128, True),
    ('pe_sine', 8, 23, 40, 128, True),
    ('pe_sine', 8, 46, 80, 128, True),
    ('pe_sine', 8, 92, 160, 128, True),
    ('point_loss', 10, 2, 471040, 100, 10, 8, 736, 1280, 10, 160000, False, True, False),
    ('point_loss', 10, 2, 471040, 100, 10, 8, 736, 1280, 10, 160000, False, True, True),
    ('point_loss', 10, 2, 471040, 100, 100, 8, 736, 1280, 100, 160000, False, True, False),
    ('point_loss', 10, 2, 471040, 100, 12, 8, 736, 1280, 12, 160000, False, True, True),
    ('s2d_transpose_f32', 10, 471040, 471040, 120),
    ('s2d_transpose_f32', 12, 471040, 471040, 120),
    ('target_nonempty', 2, 10, 8, 736, 1280),
]

def test_table_covers_the_c4_step():
    """every (entry point, signature) the benchmarked step makes under either forward path is a row of TABLE -- a dispatch change that
    brings a new shape or branch into the step fails here until the row (and with it the float64 comparison) is added -- and every public
    name of ops.py is either recorded or listed in NOT_KERNELS with its reason"""
    from s2d_amd import ops
    assert not unknown_public_functions(ops), unknown_public_functions(ops)
    seen = set(record_c4_step())
    assert len(seen) > 60
    table = set(TABLE)
    assert len(table) == len(TABLE)
    for row in sorted(table - seen, key=repr):
        print("c4table: row no longer used by the step:", row)
    missing = sorted(seen - table, key=repr)
    assert not missing, missing


# --------------------------------------------------------------------------- helpers
_MASKS = {}


def _mask(M, N, p, seed, site, row0=0):
    """oracle.dropout_multipliers (numpy Philox) for rows row0 .. row0 + M, once per distinct key, on the device"""
    from oracle import oracle_np
    key = (M, N, p, seed, site, row0)
    if key not in _MASKS:
        if len(_MASKS) >= 4:
            _MASKS.clear()
        m = oracle_np.dropout_multipliers(M + row0, N, p, seed, site)[row0:]
        _MASKS[key] = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    return _MASKS[key]


def _check(rep, name, ok):
    print(f"c4row {rep.row} {name}: {'ok' if ok else 'FAILS'}")
    if not ok:
        rep.bad.append((name,))


def _param(t):
    return torch.nn.Parameter(t, requires_grad=False)


_P, _SEED = 0.3, 0x1234567887654321


# --------------------------------------------------------------------------- one case per entry point
def _case_gemm_nt(rep, g, bs, M, N, K, b_batched, static, has_scale, has_bias, res, relu, ldc, row0):
    """bound 2e-6: test_gemm_few_rows_static_weights / test_short_k_static_weights_with_residual (f16x3), the static-weight neighbours of
    test_gemm_nt and test_gemm_row_periodic_residual (1e-4 in every dense mode)"""
    from s2d_amd import ops
    lead = (bs,) if bs > 1 or b_batched or (res is not None and res[3]) else ()
    A = _rn(g, *lead, M, K)
    Bm = _rn(g, *(lead if b_batched else ()), N, K) / K ** 0.5
    if static:
        Bm = ops.mark_static(Bm)
    sc = torch.rand((N,), device=DEV, generator=g) + 0.5 if has_scale else None
    bias = _rn(g, N) if has_bias else None
    r = rr = rc = None
    if res is not None:
        ldr, rr, rc, r3 = res
        r = _rn(g, *(lead if r3 else ()), rr or M, ldr)
    site = 1 if N == 1024 else 2                                          # the sites of the encoder's linear1 / linear2 masks
    drop = None if row0 is None else (_P, _SEED, site, row0)

    def run():
        out = None if ldc is None else torch.full(lead + (M, ldc), 7.0, device=DEV)
        y = ops.gemm_nt(A, Bm, scale=sc, bias=bias, res=r, relu=relu, out=out, res_rows=rr or 0, res_cols=rc or 0, dropout=drop)
        if out is not None and ldc > N:
            _check(rep, "columns behind N untouched", bool((out[..., N:] == 7.0).all()))
        return y[..., :N]

    y = run()
    rep.same("second call", run(), y)
    mask = None if row0 is None else _mask(M, N, _P, _SEED, site, row0)

    def ref(dt, A=A, Bm=Bm, absolute=False):
        v = A.to(dt) @ Bm.to(dt).transpose(-1, -2)
        if sc is not None:
            v = v * sc.to(dt)
        if bias is not None:
            v = v + (bias.abs() if absolute else bias).to(dt)
        pre = v
        if mask is not None and not absolute:
            v = v * mask.to(dt)
        if r is not None:
            rd = (r.abs() if absolute else r).to(dt)
            if rr:
                rd = rd.repeat(*((1,) * (rd.dim() - 2)), M // rr, 1)
            cols = rc or N
            v = torch.cat([v[..., :cols] + rd[..., :cols], v[..., cols:]], -1)
        if relu:
            v = torch.relu(v)
        return v, pre

    r64, pre64 = ref(F64)
    den = ref(F32, A.abs(), Bm.abs(), True)[0].max()
    rep.cmp("out", y, r64, ref(F32)[0], 2e-6, den)
    if mask is not None:
        # zero pattern == the mask's, where the pre-mask float64 value decides it: with a residual a kept value below half a unit in the last
        # place of the residual is absorbed, with a ReLU a kept value within the bound of zero may round to either side -- both are
        # left out below 1e-5 (operands are O(1)); without either, every non-zero pre-mask value counts
        kept = mask != 0
        if r is not None and not relu:
            sel = pre64.abs() > 1e-5
            print(f"c4row {rep.row} zero pattern: {int((~sel).sum())} of {sel.numel()} elements left out (|pre-mask f64| <= 1e-5), {int((~sel & kept).sum())} of them kept by the mask")
            _check(rep, "zero pattern of (out - res) == mask", bool((((y != r) == kept) | ~sel).all()))
        elif relu and r is None:
            sel = pre64 > 1e-5
            print(f"c4row {rep.row} zero pattern: {int((pre64.abs() <= 1e-5).sum())} of {sel.numel()} elements left out (|pre-mask f64| <= 1e-5); {int((pre64 < -1e-5).sum())} negative ones must be 0")
            _check(rep, "zero pattern == mask (positive pre-mask values)", bool((((y != 0) == kept) | ~sel).all()) and bool((y[pre64 < -1e-5] == 0).all()))
        elif r is None:
            _check(rep, "zero pattern == mask", bool((((y != 0) == kept) | (pre64 == 0)).all()))


def _conv_ref(x, w, stride, pad, dt):
    """one matmul per tap on the strided view of the zero-padded input (float64 convolutions through torch's conv2d have no fast path)"""
    N, H, W, Ci = x.shape
    Co, KH, KW, _ = w.shape
    Ho, Wo = _out_hw(H, W, KH, KW, stride, pad)
    xp = torch.nn.functional.pad(x.to(dt), (0, 0, pad, pad, pad, pad))
    wd = w.to(dt)
    out = torch.zeros((N * Ho * Wo, Co), device=x.device, dtype=dt)
    for ky in range(KH):
        for kx in range(KW):
            xs = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            out.addmm_(xs.reshape(-1, Ci), wd[:, ky, kx].t())
    return out.view(N, Ho, Wo, Co)


def _case_conv2d_nhwc(rep, g, N, H, W, Ci, Co, KH, KW, stride, pad, has_scale, has_bias, has_res, relu, static):
    """bound 2e-6: test_stem_conv_halo (f16x3), the neighbour of test_conv_nhwc / test_conv3x3_halo (1e-4 in every dense mode).  All N
    frames are compared: the per-tap matmul restatement is fast enough in float64"""
    import os
    from s2d_amd import ops
    Ho, Wo = _out_hw(H, W, KH, KW, stride, pad)
    x = _rn(g, N, H, W, Ci)
    if Ci == 4:
        x[..., 3] = 0.0                                                   # the stem reads normalize_pad's output: channel 3 is padding
    w = _rn(g, Co, KH, KW, Ci) / (Ci * KH * KW) ** 0.5
    if static:
        w = ops.mark_static(w)
    sc = torch.rand((Co,), device=DEV, generator=g) + 0.5 if has_scale else None
    bias = _rn(g, Co) if has_bias else None
    r = _rn(g, N, Ho, Wo, Co) if has_res else None
    run = lambda: ops.conv2d_nhwc(x, w, stride, pad, sc, bias, r, relu)
    y = run()
    rep.same("second call", run(), y)

    def ref(dt, x=x, w=w, absolute=False):
        v = _conv_ref(x, w, stride, pad, dt)
        if sc is not None:
            v = v * sc.to(dt)
        if bias is not None:
            v = v + (bias.abs() if absolute else bias).to(dt)
        if r is not None:
            v = v + (r.abs() if absolute else r).to(dt)
        return torch.relu(v) if relu else v

    r64, r32 = ref(F64), ref(F32)
    den = ref(F32, x.abs(), w.abs(), True).max()
    rep.cmp("out", y, r64, r32, 2e-6, den)
    if KH == 3:                                                           # the other form of the input-halo kernel (read per call)
        old = os.environ.get("S2D_CONV_HALO_PIPE")
        os.environ["S2D_CONV_HALO_PIPE"] = "0" if old == "1" else "1"
        try:
            rep.cmp("out, other S2D_CONV_HALO_PIPE form", run(), r64, r32, 2e-6, den)
        finally:
            if old is None:
                del os.environ["S2D_CONV_HALO_PIPE"]
            else:
                os.environ["S2D_CONV_HALO_PIPE"] = old


def _ln(v, gb, dt):
    return torch.nn.functional.layer_norm(v, (v.shape[-1],), gb[0].to(dt), gb[1].to(dt), 1e-5)


def _case_ffn_fused(rep, g, M, F, has_ln1, has_ln2, row0, want_xn, post, has_pre):
    """bound 2e-5 on the outputs (test_ffn_fused_vs_oracle and its two neighbours), 5e-6 on xn (test_ffn_fused_with_attention_output_
    projection).  The masks act in front of LayerNorms, so their zero pattern is not visible in an output: a shifted or wrong mask shows
    as an error of order 1"""
    from s2d_amd import ops
    C = 256
    x = _rn(g, M, C) * 1.5
    W1, b1, W2, b2 = _param(_rn(g, F, C) * 0.06), _rn(g, F) * 0.1, _param(_rn(g, C, F) * 0.03), _rn(g, C) * 0.1
    ln1 = (_rn(g, C) * 0.2 + 1, _rn(g, C) * 0.1) if has_ln1 else None
    ln2 = (_rn(g, C) * 0.2 + 1, _rn(g, C) * 0.1) if has_ln2 else None
    drop = None if row0 is None else (_P, _SEED, 1, 2, row0)
    kw = {}
    if has_pre:
        Wq, qb, qres = _param(_rn(g, C, C) * 0.07), _rn(g, C) * 0.1, _rn(g, M, C) * 1.5
        kw["pre"] = (Wq, qb, qres, 0)
    if post is not None:
        Np, S, npos, ldpos = post
        Wp = ops.mark_static(_rn(g, Np, C) * 0.05)
        pb = torch.cat([torch.zeros((npos,), device=DEV), _rn(g, Np - npos) * 0.1])     # the pos term carries the first npos columns' bias
        pos = (_rn(g, S, ldpos) * 0.5)[:, :npos] if S else None
        kw["post"] = (Wp, pb, pos)
    run = lambda: ops.ffn_fused(x, W1, b1, W2, b2, ln1=ln1, ln2=ln2, dropout=drop, want_xn=want_xn, **kw)
    got, again = run(), run()
    got, again = (got if isinstance(got, tuple) else (got,)), (again if isinstance(again, tuple) else (again,))
    names = ["y"] + (["xn"] if want_xn else []) + (["out_post"] if post is not None else [])
    mk = (lambda n, site: _mask(M, n, _P, _SEED, site, row0)) if row0 is not None else None

    def ref(dt):
        v = x.to(dt)
        if has_pre:
            a = v @ Wq.to(dt).t() + qb.to(dt)
            if mk:
                a = a * mk(C, 0).to(dt)
            v = qres.to(dt) + a
        xn = _ln(v, ln1, dt) if ln1 else v
        hid = torch.relu(xn @ W1.to(dt).t() + b1.to(dt))
        if mk:
            hid = hid * mk(F, 1).to(dt)
        o = hid @ W2.to(dt).t() + b2.to(dt)
        del hid
        if mk:
            o = o * mk(C, 2).to(dt)
        y = xn + o
        if ln2:
            y = _ln(y, ln2, dt)
        outs = [y] + ([xn] if want_xn else [])
        if post is not None:
            po = y @ Wp.to(dt).t() + pb.to(dt)
            if pos is not None:
                po[:, :npos] += pos.to(dt).repeat(M // S, 1)
            outs.append(po)
        return outs

    r64, r32 = ref(F64), ref(F32)
    for i, name in enumerate(names):
        rep.same(name + " second call", again[i], got[i])
        rep.cmp(name, got[i], r64[i], r32[i], 5e-6 if name == "xn" else 2e-5)
    # the launches the encoder layer makes instead with fuse_pre / fuse_next / fuse_ffn = False (pixel_decoder.py), on the same operands
    # against the same references
    ipost = len(names) - 1
    if has_pre:
        d1 = None if row0 is None else (_P, _SEED, 0, row0)
        x1 = ops.gemm_nt(x, Wq, bias=qb, res=qres, dropout=d1)             # the attention's own output projection + dropout1 + residual
        o = ops.ffn_fused(x1, W1, b1, W2, b2, ln1=ln1, ln2=ln2, dropout=drop, **({"post": kw["post"]} if post is not None else {}))
        o = o if isinstance(o, tuple) else (o,)
        rep.cmp("y, fuse_pre = False form", o[0], r64[0], r32[0], 2e-5)
        if post is not None:
            rep.cmp("out_post, fuse_pre = False form", o[-1], r64[ipost], r32[ipost], 2e-5)
    else:
        x1 = x
    if post is not None and pos is not None:
        y0 = ops.ffn_fused(x, W1, b1, W2, b2, ln1=ln1, ln2=ln2, dropout=drop, **({"pre": kw["pre"]} if has_pre else {}))
        rep.same("y, fuse_next = False form", y0, got[0])
        po = ops.gemm_nt(y0, Wp, bias=pb, res=pos.contiguous(), res_rows=S, res_cols=npos)
        rep.cmp("out_post, fuse_next = False form", po, r64[ipost], r32[ipost], 2e-5)
        del y0, po
    if has_ln1 and has_ln2:
        d2, d3 = (None, None) if row0 is None else ((_P, _SEED, 1, row0), (_P, _SEED, 2, row0))
        s1 = ops.layernorm(x1, *ln1)
        h = ops.gemm_nt(s1, W1, bias=b1, relu=True, dropout=d2)
        if M * F * 4 > 0xFFFFFF00:
            # the hidden activation, which only this form materialises, is a GEMM operand beyond the 32-bit buffer offsets of
            # s2d_gemm_nt_f32 (4 GB - 256 B; M > 1 048 575 rows at F = 1024: no c4 row): the C ABI must refuse it, before any launch
            # (h itself was written by the first GEMM -- the C side of a GEMM is addressed with 64-bit pointers -- and is compared with
            # nothing: it only serves as the operand whose size is refused)
            try:
                ops.gemm_nt(h, W2, bias=b2, res=s1, dropout=d3)
                refused = False
            except RuntimeError as e:
                refused = "s2d_gemm_nt_f32 failed with code -1" in str(e)
            _check(rep, f"fuse_ffn = False form: hidden operand of {M * F * 4} bytes refused with S2D_ERR_ARG", refused)
        else:
            y2 = ops.layernorm(ops.gemm_nt(h, W2, bias=b2, res=s1, dropout=d3), *ln2)
            rep.cmp("y, fuse_ffn = False form", y2, r64[0], r32[0], 2e-5)
        del h


def _case_msda_fused_forward(rep, g, N, C, shapes, vstride, ostride, owidth, M, P):
    """bound 1e-5: test_msda_fused_vs_oracle_720p_shapes.  value / offsets+logits are column slices of one buffer, as the merged projection
    leaves them; offsets of several pixels, so samples leave the maps"""
    from s2d_amd import ops
    from tests.test_gpu_backward import _msda_fused_torch
    S = sum(h * w for h, w in shapes)
    assert vstride == ostride == owidth + C
    both = torch.cat([_rn(g, N, S, 2 * owidth // 3) * 2.0, _rn(g, N, S, owidth // 3), _rn(g, N, S, C)], -1)
    oa, value = both[..., :owidth], both[..., owidth:]
    shp = [tuple(s) for s in shapes]
    out = ops.msda_fused_forward(value, np.array(shp), oa, M, P)
    rep.same("second call", ops.msda_fused_forward(value, np.array(shp), oa, M, P), out)

    def ref(dt, step=4):
        with torch.device(DEV), torch.no_grad():
            return torch.cat([_msda_fused_torch(value[n:n + step].to(dt), shp, oa[n:n + step].to(dt), M, P) for n in range(0, N, step)])
    rep.cmp("out", out, ref(F64), ref(F32), 1e-5)


def _case_masked_attn(rep, g, Bc, Q, K, C, H, has_bits, has_unm, ks, vs, want_lse):
    """bound 2e-5: test_masked_attention_backward_vs_autograd holds the gradients of this kernel's output to it (the forward's own small
    test, test_mask_and_cross_attention, asserts a looser 1e-4 with no dense mode in play)"""
    from s2d_amd import ops
    from tests.test_gpu_backward import _masked_attn_torch
    q = _rn(g, Bc, Q, C)
    assert has_bits == has_unm
    if ks == vs and ks >= 2 * C:                                           # k | v: the last two column blocks of one [B,K,ks] buffer
        kv = torch.zeros((Bc, K, ks), device=DEV)
        k, v = kv[..., ks - 2 * C:ks - C], kv[..., ks - C:]
    else:                                                                  # each a column block of its own buffer
        k, v = torch.zeros((Bc, K, ks), device=DEV)[..., ks - C:], torch.zeros((Bc, K, vs), device=DEV)[..., vs - C:]
    k.copy_(_rn(g, Bc, K, C)); v.copy_(_rn(g, Bc, K, C))
    assert (k.stride(1), v.stride(1)) == (ks, vs)
    mask = torch.zeros((Bc, Q, K), device=DEV, dtype=torch.bool)
    bits = unm = None
    if has_bits:
        mask = torch.rand((Bc, Q, K), device=DEV, generator=g) < 0.6
        mask[0, 3] = True                                                  # every key masked: attends everywhere, `unmasked` bit clear
        mask[-1, 7] = True; mask[-1, 7, K - 5] = False                     # a single free key late in the stream
        bits, unm = _pack_bits(mask)
        assert not (int(unm[0, 0]) >> 3) & 1
    run = lambda: ops.masked_attn(q, k, v, bits, unm, H=H, want_lse=want_lse)
    got, again = run(), run()
    got, again = (got if want_lse else (got,)), (again if want_lse else (again,))

    def ref(dt):
        o = _masked_attn_torch(q.to(dt), k.to(dt), v.to(dt), mask, H)
        if not want_lse:
            return (o,)
        D = C // H
        eff = mask.clone(); eff[eff.all(-1)] = False
        sc = torch.einsum("bqhd,bkhd->bhqk", q.to(dt).reshape(Bc, Q, H, D), k.to(dt).reshape(Bc, K, H, D)) / D ** 0.5
        return o, torch.logsumexp(sc.masked_fill(eff[:, None], float("-inf")), -1) * 1.4426950408889634     # base 2
    r64, r32 = ref(F64), ref(F32)
    rep.same("out second call", again[0], got[0])
    rep.cmp("out", got[0], r64[0], r32[0], 2e-5)
    if want_lse:
        rep.same("lse second call", again[1][..., :Q], got[1][..., :Q])
        rep.cmp("lse (base 2)", got[1][..., :Q], r64[1], r32[1], 2e-5)


def _smooth_logits(g, n, hm, wm, amp=4.0):
    """n smooth float32 maps [n, hm, wm] with continuous values: a 6 x 6 normal grid, bicubic to (hm, wm) (the device-side counterpart of
    s2d_amd.utils.synth.smooth_logits, which fills 1 600 maps of 184 x 320 one by one on the host)"""
    c = _rn(g, n, 1, 6, 6) * amp
    return torch.nn.functional.interpolate(c, size=(hm, wm), mode="bicubic", align_corners=True)[:, 0].contiguous()


def _unpack(bits, Q):
    """bits int32 [B,K,4] -> bool [B,Q,K]"""
    qs = torch.arange(Q, device=bits.device)
    w = bits.long()[:, :, (qs >> 5)]                                       # [B,K,Q]
    return ((w >> (qs & 31)[None, None, :]) & 1).bool().permute(0, 2, 1)


_BAND = 2.0 ** -20


def _sign_reference(rep, ml, hl, wl):
    """ml [n, hm, wm] float32 -> (the float64 bilinear interpolation [n, hl, wl], excluded bool: |float64 value| within _BAND x
    the largest logit of zero).  Also checks the band on the reference alone: every float64-vs-float32 disagreement lies inside it, and the
    excluded share stays under 1e-4"""
    interp = lambda t: torch.nn.functional.interpolate(t[:, None], size=(hl, wl), mode="bilinear", align_corners=False)[:, 0]
    v64, v32 = interp(ml.double()), interp(ml)
    excl = v64.abs() < _BAND * float(ml.abs().max())
    dis = (v64 < 0) != (v32 < 0)
    n_ex, n_dis, n_out = int(excl.sum()), int(dis.sum()), int((dis & ~excl).sum())
    print(f"c4row {rep.row} sign reference {hl}x{wl}: {n_ex} of {excl.numel()} elements excluded (|f64| < 2^-20 max|logit|), f64 / f32 torch disagree on {n_dis}, "
          f"{n_out} of them outside the band")
    if n_out or not n_ex < 1e-4 * excl.numel():
        rep.bad.append(("sign band", n_ex, n_dis, n_out))
    return v64, excl


def _case_attn_mask_bits(rep, g, B, Q, T, hm, wm, hl, wl, ldq, compact):
    """exact against the sign of the float64 interpolation outside the excluded band (test_mask_and_cross_attention asserts array equality);
    compact rows: the tap-gathered form on the same logits, also bit for bit equal to the full form"""
    from s2d_amd import ops
    ml = _smooth_logits(g, B * Q * T, hm, wm).view(B, Q, T, hm, wm)
    ml[:, 1] = -ml[:, 1].abs() - 0.1                                       # query 1: masked on every key
    ml[0, 5] = ml[0, 5].abs() + 0.1                                        # query 5 of clip 0: masked nowhere
    width = ldq
    pm = torch.zeros((B, T * hm * wm, width), device=DEV)
    pm[..., :Q] = ml.permute(0, 2, 3, 4, 1).reshape(B, T * hm * wm, Q)
    assert width >= Q
    full = ops.attn_mask_bits(pm, B, Q, T, hm, wm, hl, wl)
    if compact:
        idx = ops.attn_mask_tap_index(T, hm, wm, hl, wl, DEV)
        sub = pm.index_select(1, idx).contiguous()
        got = ops.attn_mask_bits(sub, B, Q, T, hm, wm, hl, wl, compact=True)
        again = ops.attn_mask_bits(sub, B, Q, T, hm, wm, hl, wl, compact=True)
        rep.same("bits == full form", got[0], full[0])
        rep.same("unmasked == full form", got[1], full[1])
    else:
        got, again = full, ops.attn_mask_bits(pm, B, Q, T, hm, wm, hl, wl)
    rep.same("bits second call", again[0], got[0])
    rep.same("unmasked second call", again[1], got[1])
    K = T * hl * wl
    v64, excl = _sign_reference(rep, ml.view(-1, hm, wm), hl, wl)
    ref, excl = (v64 < 0).view(B, Q, K), excl.view(B, Q, K)
    m = _unpack(got[0], Q)
    wrong = int(((m != ref) & ~excl).sum())
    print(f"c4row {rep.row} bits: {wrong} wrong outside the band")
    if wrong:
        rep.bad.append(("bits", wrong))
    has = _unpack(got[1][:, None, :], Q)[:, :, 0]                          # [B,Q]: query has a free key
    clean = ~excl.any(-1)
    _check(rep, f"unmasked words on the {int(clean.sum())} of {B * Q} queries without an excluded element", bool(((has == ~ref.all(-1)) | ~clean).all()))
    _check(rep, "query 1 masked everywhere, query 5 of clip 0 nowhere", bool(ref[:, 1].all()) and not bool(has[:, 1].any()) and not bool(ref[0, 5].any()))


def _case_attn_mask_tap_index(rep, g, T, hm, wm, hl, wl):
    """exact: the four pixels F.interpolate(bilinear, align_corners=False) reads for every key, from the rule in float64"""
    from s2d_amd import ops
    idx = ops.attn_mask_tap_index(T, hm, wm, hl, wl, DEV)
    sy = ((torch.arange(hl, dtype=F64, device=DEV) + 0.5) * (hm / hl) - 0.5).clamp(min=0)
    sx = ((torch.arange(wl, dtype=F64, device=DEV) + 0.5) * (wm / wl) - 0.5).clamp(min=0)
    y0, x0 = sy.floor().long(), sx.floor().long()
    y1, x1 = (y0 + 1).clamp(max=hm - 1), (x0 + 1).clamp(max=wm - 1)
    rows, cols = torch.stack([y0, y0, y1, y1], -1), torch.stack([x0, x1, x0, x1], -1)
    pix = rows[:, None, :] * wm + cols[None, :, :]
    ref = (torch.arange(T, device=DEV)[:, None, None, None] * (hm * wm) + pix[None]).reshape(-1)
    rep.same("indices", idx, ref)


def _case_kd_targets(rep, g, B, C1, Q, T, hm, wm, ldq, H, W, Nmax, topk, want_labels):
    """exact outside the excluded band (test_full_criterion_and_kd_targets_golden asserts array equality of the planes): the targets
    kept are those of the top `topk` flat scores that reach thr (scores drawn well away from thr: a float32 softmax decides like float64,
    and fewer than topk reach it, so thr alone decides), count and kept exact, every plane == (float64 bilinear interpolation > 0),
    nonempty == any() of the plane.  C1 = 2: the score of class 0.  C1 > 2 (tests/test_gpu_classes_c4.py): a hot query q scores on
    class q % C, the other foreground logits sit at -20; kept / label are the flat indices q*C + c that reach thr, in ascending order"""
    from s2d_amd import ops
    C = C1 - 1
    assert C1 >= 2 and topk >= Q
    thr = 0.75
    cls = torch.zeros((B, Q, C1), device=DEV)
    if C1 > 2:
        cls[..., :C] = -20.0
    cls[..., 0] = -1.0 - torch.rand((B, Q), device=DEV, generator=g)                 # score <= 0.27
    for b in range(B):
        hot = torch.randperm(Q, device=DEV, generator=g)[:12 + b]
        heat = 3.0 + torch.rand((12 + b,), device=DEV, generator=g)                  # score >= 0.95
        if C1 > 2:
            cls[b, hot, 0] = -20.0
        cls[b, hot, hot % C] = heat
    ml = _smooth_logits(g, B * Q * T, hm, wm).view(B, Q, T, hm, wm)
    pm = torch.zeros((B, T * hm * wm, ldq), device=DEV)
    pm[..., :Q] = ml.permute(0, 2, 3, 4, 1).reshape(B, T * hm * wm, Q)
    run = lambda: ops.kd_targets(cls, pm, (Q, T, hm, wm), H, W, Nmax, thr, topk, want_labels=want_labels)
    got, again = run(), run()
    tgt, count, kept, ne = got[:4]
    score = torch.softmax(cls.double(), -1)[..., :C].reshape(B, Q * C)
    for b in range(B):
        want = torch.nonzero(score[b] >= thr)[:, 0]
        n = int(count[b])
        if C1 == 2:
            _check(rep, f"clip {b}: count {n} and kept queries", n == want.numel() and torch.equal(kept[b, :n].long().sort().values, want))
        else:
            _check(rep, f"clip {b}: count {n}, kept queries and labels in ascending flat index", n == want.numel() and want_labels
                   and torch.equal(kept[b, :n].long(), want // C) and torch.equal(got[4][b, :n].long(), want % C))
            rep.same(f"clip {b}: labels second call", again[4][b, :n], got[4][b, :n])
        rep.same(f"clip {b}: planes second call", again[0][b, :n], tgt[b, :n])
        rep.same(f"clip {b}: nonempty second call", again[3][b, :n], ne[b, :n])
        if n != want.numel():
            continue
        v64, excl = _sign_reference(rep, ml[b, kept[b, :n].long()].reshape(n * T, hm, wm), H, W)
        ref = (v64 > 0).view(n, T, H, W)
        excl = excl.view(n, T, H, W)
        wrong = int((((tgt[b, :n] != 0) != ref) & ~excl).sum())
        print(f"c4row {rep.row} clip {b} planes: {wrong} wrong outside the band")
        if wrong:
            rep.bad.append(("planes", b, wrong))
        clean = ~excl.flatten(2).any(-1)
        _check(rep, f"clip {b}: nonempty on the {int(clean.sum())} of {n * T} planes without an excluded element",
               bool((((ne[b, :n] != 0) == ref.flatten(2).any(-1)) | ~clean).all()))
    if want_labels and C1 == 2:
        _check(rep, "no labels at two classes", got[4] is None)


def _case_class_loss(rep, g, B, Q, C1, maxm):
    """bound 1e-4: test_loss_golden_and_droploss_empty.  Weighted cross-entropy: matched queries -> class 0, the others -> no object with
    weight eos_coef, sum of weighted terms over the sum of weights"""
    from s2d_amd import ops
    logits = _rn(g, B, Q, C1) * 2.0
    iq = torch.zeros((B, maxm), device=DEV, dtype=torch.int32)
    nm = torch.tensor([maxm, max(maxm - 3, 0)][:B] + [maxm // 2] * max(B - 2, 0), device=DEV, dtype=torch.int32)
    tg = torch.full((B, Q), C1 - 1, device=DEV, dtype=torch.long)
    for b in range(B):
        q = torch.randperm(Q, device=DEV, generator=g)[:int(nm[b])].sort().values
        iq[b, :q.numel()] = q.int()
        tg[b, q] = 0
    out = ops.class_loss(logits, iq, nm, 0.1)
    rep.same("second call", ops.class_loss(logits, iq, nm, 0.1), out)
    w = torch.ones((C1,), device=DEV, dtype=F64); w[-1] = 0.1
    ref = lambda dt: torch.nn.functional.cross_entropy(logits.to(dt).view(-1, C1), tg.view(-1), weight=w.to(dt)).reshape(1)
    rep.cmp("loss_ce", out.reshape(1), ref(F64), ref(F32), 1e-4)


def _case_target_nonempty(rep, g, B, Nmax, T, H, W):
    """exact (test_loss_golden_and_droploss_empty): nonempty[b, n, t] != 0 iff plane (b, n, t) of a counted target has a set pixel; planes
    with a single pixel in a corner, empty planes, and slots behind count (zero planes here) among them"""
    from s2d_amd import ops
    tgt = (torch.rand((B, Nmax, T, H, W), device=DEV, generator=g) < 0.01).to(torch.uint8)
    count = torch.tensor([Nmax, max(Nmax - 2, 1)][:B] + [Nmax] * max(B - 2, 0), device=DEV, dtype=torch.int32)
    for b in range(B):
        tgt[b, int(count[b]):] = 0
    tgt[0, 0, 0] = 0                                                                # an empty plane
    tgt[0, 0, 1] = 0; tgt[0, 0, 1, H - 1, W - 1] = 1                                # one pixel, the last
    tgt[-1, 1, T - 1] = 0; tgt[-1, 1, T - 1, 0, 0] = 1                              # one pixel, the first
    ne = ops.target_nonempty(tgt, count)
    rep.same("second call", ops.target_nonempty(tgt, count), ne)
    rep.same("nonempty != 0", ne != 0, tgt.flatten(3).any(-1))


def _case_groupnorm_nhwc(rep, g, N, H, W, C, G, up, relu):
    """bound 1e-5: test_groupnorm_layernorm_add_pe / test_groupnorm_both_sides_of_the_size_thresholds"""
    from s2d_amd import ops
    Fn = torch.nn.functional
    x, ga, be = _rn(g, N, H, W, C) * 3 + 1, _rn(g, C) * 0.1 + 1, _rn(g, C) * 0.1
    u = _rn(g, N, up[0], up[1], C) if up else None
    run = lambda: ops.groupnorm_nhwc(x, G, ga, be, up=u, relu=relu)
    y = run()
    rep.same("second call", run(), y)

    def ref(dt):
        v = Fn.group_norm(x.to(dt).permute(0, 3, 1, 2), G, ga.to(dt), be.to(dt), 1e-5)
        if u is not None:
            v = v + Fn.interpolate(u.to(dt).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
        v = v.permute(0, 2, 3, 1)
        return torch.relu(v) if relu else v
    rep.cmp("out", y, ref(F64), ref(F32), 1e-5)


def _case_layernorm(rep, g, rows, C, has_res):
    """bound 1e-5: test_groupnorm_layernorm_add_pe / test_layernorm_both_kernels_and_every_tail"""
    from s2d_amd import ops
    x, ga, be = _rn(g, rows, C) * 2 + 0.5, _rn(g, C) * 0.1 + 1, _rn(g, C) * 0.1
    r = _rn(g, rows, C) if has_res else None
    y = ops.layernorm(x, ga, be, res=r)
    rep.same("second call", ops.layernorm(x, ga, be, res=r), y)
    ref = lambda dt: _ln(x.to(dt) if r is None else x.to(dt) + r.to(dt), (ga, be), dt)
    rep.cmp("out", y, ref(F64), ref(F32), 1e-5)


def _case_maxpool3x3s2(rep, g, N, H, W, C, want_idx):
    """exact (test_normalize_pad_maxpool asserts array equality); the arg-max tap points into the map at an element equal to the maximum"""
    from s2d_amd import ops
    x = torch.relu(_rn(g, N, H, W, C))                                    # ReLU outputs: many exact ties at 0
    got = ops.maxpool3x3s2(x, want_idx=want_idx)
    y, idx = got if want_idx else (got, None)
    ref = torch.nn.functional.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    _check(rep, "values bit-equal to float64 max_pool2d", torch.equal(y.double(), ref))
    del ref
    again = ops.maxpool3x3s2(x, want_idx=want_idx)
    rep.same("second call", again[0] if want_idx else again, y)
    if want_idx:
        rep.same("idx second call", again[1], idx)
        Ho, Wo = y.shape[1:3]
        ok = True
        for n in range(N):                                                # frame by frame: the index tensors are int64
            ky, kx = (idx[n] // 3).long(), (idx[n] % 3).long()
            yy = torch.arange(Ho, device=DEV)[:, None, None] * 2 - 1 + ky
            xx = torch.arange(Wo, device=DEV)[None, :, None] * 2 - 1 + kx
            inside = (ky < 3) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            c = torch.arange(C, device=DEV)[None, None, :].expand_as(ky)
            ok = ok and bool(inside.all()) and torch.equal(x[n][yy.clamp(0, H - 1), xx.clamp(0, W - 1), c], y[n])
        _check(rep, "idx inside the map, at an element equal to the maximum", ok)


def _case_normalize_pad(rep, g, Fr, H0, W0, div):
    """bound 1e-6: test_normalize_pad_maxpool"""
    from s2d_amd import ops
    fr = torch.randint(0, 256, (Fr, 3, H0, W0), device=DEV, generator=g, dtype=torch.uint8)
    out = ops.normalize_pad(fr, div)
    rep.same("second call", ops.normalize_pad(fr, div), out)
    Hp, Wp = (H0 + div - 1) // div * div, (W0 + div - 1) // div * div
    _check(rep, "shape", tuple(out.shape) == (Fr, Hp, Wp, 4))

    def ref(dt):
        mean = torch.tensor([float(v) for v in ops.PIXEL_MEAN], dtype=dt, device=DEV)    # the float32 constants, exactly
        std = torch.tensor([float(v) for v in ops.PIXEL_STD], dtype=dt, device=DEV)
        v = torch.zeros((Fr, Hp, Wp, 4), dtype=dt, device=DEV)
        v[:, :H0, :W0, :3] = (fr.permute(0, 2, 3, 1).to(dt) - mean) / std
        return v
    r64 = ref(F64)
    rep.cmp("out", out, r64, ref(F32), 1e-6)
    _check(rep, "padding and channel 3 exactly zero", bool((out[r64 == 0] == 0).all()))


def _case_add_bcast(rep, g, n, bn):
    """exact: one float32 addition per element"""
    from s2d_amd import ops
    C = 256
    x, b = _rn(g, n // bn, bn // C, C), _rn(g, bn // C, C)
    y = ops.add_bcast(x, b)
    rep.same("x + b", y, x + b[None])
    _check(rep, "== float64 sum rounded once", torch.equal(y, (x.double() + b.double()[None]).float()))


def _case_pe_sine(rep, g, T, H, W, npf, has_c):
    """2e-5 absolute (the bound of the golden test in test_groupnorm_layernorm_add_pe): the sine position encodings restated in float64 --
    normalised 1-based coordinates x 2 pi over 10000^(2 floor(j / 2) / F), sin on even and cos on odd channels, (y | x) channel blocks,
    with T the temporal term over all 2 F channels added -- plus the per-channel constant"""
    import math
    from s2d_amd import ops
    add_c = _rn(g, 2 * npf) if has_c else None
    out = ops.pe_sine(T, H, W, npf, add_c=add_c, device=DEV)
    rep.same("second call", ops.pe_sine(T, H, W, npf, add_c=add_c, device=DEV), out)

    def sc(n, F):
        e = torch.arange(1, n + 1, dtype=F64, device=DEV) / (n + 1e-6) * (2 * math.pi)
        j = torch.arange(F, dtype=F64, device=DEV)
        a = e[:, None] / 10000.0 ** (2 * torch.floor(j / 2) / F)
        return torch.where((torch.arange(F, device=DEV) % 2 == 0)[None], torch.sin(a), torch.cos(a))        # [n, F]
    Tn = max(T, 1)
    ref = torch.cat([sc(H, npf)[None, :, None, :].expand(Tn, H, W, npf), sc(W, npf)[None, None, :, :].expand(Tn, H, W, npf)], -1)
    if T > 0:
        ref = ref + sc(T, 2 * npf)[:, None, None, :]
    if add_c is not None:
        ref = ref + add_c.double()
    err = float((out.double() - ref.reshape(-1, 2 * npf)).abs().max())
    print(f"c4row {rep.row} out: max abs error {err:.3e} bound 2.000e-05 (+ one rounding of the sum with add_c)")
    if not err < 2e-5 + (2.0 ** -24 * float(ref.abs().max()) if has_c else 0.0):
        rep.bad.append(("pe", err))


def _case_dropout_apply(rep, g, M, N, row0, into_out):
    """x * mask / P(keep): one float32 product per element (bound 2^-23: one rounding), zero pattern exactly the mask's"""
    from s2d_amd import ops
    x = _rn(g, M, N)
    mask = _mask(M, N, _P, _SEED, 2, row0)
    run = lambda: ops.dropout_apply(x, _P, _SEED, 2, row0, out=torch.empty_like(x) if into_out else None)
    y = run()
    rep.same("second call", run(), y)
    rep.cmp("out", y, x.double() * mask.double(), x * mask, 2.0 ** -23)
    _check(rep, "zero pattern == mask", bool((((y != 0) == (mask != 0)) | (x == 0)).all()))


def _case_s2d_transpose_f32(rep, g, rows, cols, lds, ldd):
    """exact, the columns of the destination outside the block untouched"""
    from s2d_amd import ops
    src = _rn(g, rows, lds)
    off = (ldd - rows) // 2 // 4 * 4
    dst = torch.full((cols, ldd), 7.0, device=DEV)
    ops.lib().call("s2d_transpose_f32", src, rows, cols, lds, dst[:, off:], ldd, ops._stream())
    rep.same("block", dst[:, off:off + rows], src[:, :cols].t())
    _check(rep, "columns outside the block untouched", bool((dst[:, :off] == 7.0).all()) and bool((dst[:, off + rows:] == 7.0).all()))


ROWS = [r for r in TABLE if r[0] not in NO_ROWS]


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_c4_row_vs_float64(row):
    case = globals()["_case_" + row[0]]
    rep = _Rep(row)
    old = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False      # the float32 restatement is plain float32
    try:
        case(rep, _gen(row), *row[1:])
        torch.cuda.synchronize()
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old
    rep.done()
