"""Backward kernels at the shapes of the benchmarked c4 training iteration (2 clips x T=8 x 720p, Q=100, P=160 000), each compared with a
float64 restatement of the same operation written here in plain torch on the device (nothing of s2d_amd / libs2d_hip.so in the reference).

TABLE is the set of (entry point of s2d_amd/backward.py, shape signature) pairs one c4 `forward_backward` makes;
test_table_covers_the_c4_iteration re-records it from the model bench.py builds and fails when the iteration calls something the table
does not hold.  Every row runs the kernel at full size on seeded float32 operands, the float64 restatement, and the SAME restatement in
float32 through torch (rocBLAS / aten).  Bound of a row: max(bound tests/test_gpu_backward.py asserts for that function at small size,
2 x the float32-torch error on these operands) -- the factor 2 covers the split-fp16 x3 product (which drops the low x low term, 2^-22
per product) and another summation order; it is never read off the kernel's own output.  Metric: `rel` of tests/test_gpu_backward.py
(max abs error / max abs reference); contractions also print the scale-invariant error of tests/test_gpu_split_range.py
(max|C - C_ref| / max(|A| . |B|)).  Each row also keeps the self-consistency checks of the small tests: a second call is bitwise equal,
and the opt-out forms (_CONV_WGRAD_IMPLICIT / _CONV_DGRAD_S2 / _MSDA_BWD_REC = False) meet the same bound against the same reference.
The figures of one run are in profiles/c4_backward_parity.txt (the `c4row` lines this module prints).  One comparison is restricted:
MSDeformAttn's offset gradient jumps where a sample crosses a pixel-cell edge, so it is compared with float64 on the samples farther than
1e-4 px from an edge (their count is printed and capped) and, on every element, with the two-step form of the kernel.

linear_backward, resize_bilinear_backward and transpose have signatures but no rows: the iteration never calls them directly
(resize_bilinear_backward runs inside the groupnorm_up_relu_backward row with up_hw, relu_scale_backward / groupnorm_backward inside it too).

test_conv_weight_grad_index_arithmetic sweeps the 3 x 3 weight gradient's magic-number divisions and slice starts at small sizes.

Out of scope here: the point-loss / class-loss backward and kd_compact (tests/test_gpu_backward.py has their part-walking and
padded-vs-compact tests).  The operands `out` / `lse` of the attention rows and `idx` of the max-pool row are what the library's own
forward stores for its backward (their layouts are private to it); the references do not use them."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# --------------------------------------------------------------------------- shape signatures (what selects a kernel and a branch; no data)
def _sh(t):
    return None if t is None else tuple(int(v) for v in t.shape)


def _sig_conv_weight_grad(dy, x, KH, KW, stride, pad):
    N, H, W, Ci = x.shape
    return (N, H, W, Ci, dy.shape[3], KH, KW, stride, pad)


def _sig_conv_input_grad(dy, w, stride, pad, in_hw, gate=None, scale=None):
    N, Ho, Wo, Co = dy.shape
    return (N, in_hw[0], in_hw[1], w.shape[3], Co, w.shape[1], w.shape[2], stride, pad, gate is not None, scale is not None)


def _sig_weight_grad(dy, x, out=None, beta=0.0, bias_out=None, bias_beta=0.0):
    return (dy.shape[0], dy.shape[1], x.shape[1], None if out is None else float(beta), None if bias_out is None else float(bias_beta))


def _sig_input_grad(dy, w, res=None, gate=None, gate_scale=1.0, scale=None):
    M = dy.shape[0]
    gs = None
    if gate is not None:                       # row stride of the gate as the GEMM epilogue reads it (selects the fused form)
        g2 = gate.reshape(-1, w.shape[1])
        gs = (int(g2.stride(0)), float(gate_scale))
    return (M, w.shape[0], w.shape[1], res is not None, gs, scale is not None)


def _sig_linear_backward(x, w, dy, need_dx=True, has_bias=True):
    return (x.shape[0], w.shape[0], w.shape[1], bool(need_dx), bool(has_bias))


def _sig_bias_grad(dy, out=None, beta=0.0):
    return (dy.shape[0], dy.shape[1], None if out is None else float(beta))


def _sig_layernorm_backward(x, dy, gamma, res=None, eps=1e-5):
    C = x.shape[-1]
    return (x.numel() // C, C, res is not None)


def _sig_groupnorm_up_relu_backward(x, y, dy, G, gamma, up_hw=None, relu=False, eps=1e-5):
    return _sh(x) + (G, None if up_hw is None else tuple(up_hw), bool(relu))


def _sig_groupnorm_backward(x, dy, G, gamma, eps=1e-5):
    return _sh(x) + (G,)


def _sig_resize_bilinear_backward(dy, hu, wu):
    return _sh(dy) + (hu, wu)


def _sig_maxpool_backward(x, dy, idx=None):
    return _sh(x) + (idx is not None,)


def _sig_msda_fused_backward(value, shapes, offs_logits, grad_out, M=8, P=4, merged=False):
    sh = tuple(tuple(int(v) for v in r) for r in torch.as_tensor(shapes).tolist())
    return (value.shape[0], value.shape[2], sh, int(value.stride(1)), int(offs_logits.stride(1)), offs_logits.shape[2], M, P, bool(merged))


def _sig_masked_attn_backward(q, k, v, out, lse, dout, bits=None, unmasked=None, H=8, dk_out=None, dv_out=None):
    B, Q, C = q.shape
    return (B, Q, k.shape[1], C, H, bits is not None, unmasked is not None, int(k.stride(1)), int(v.stride(1)),
            None if dk_out is None else int(dk_out.stride(1)), None if dv_out is None else int(dv_out.stride(1)))


def _sig_relu_scale_backward(dy, y=None, scale=None, want_res=False):
    return (dy.numel() // dy.shape[-1], dy.shape[-1], y is not None, scale is not None, bool(want_res))


def _sig_relu_gate_add(a, g, y):
    return (a.numel(),)


def _sig_sum_slices(x):
    return (x.shape[0], x[0].numel())


def _sig_transpose(x, pad_to=None):
    return (x.shape[0], x.shape[1], pad_to)


ENTRY_POINTS = {n[5:]: f for n, f in list(globals().items()) if n.startswith("_sig_")}
# public functions of backward.py that compute no gradient themselves: gradient accumulation (they call weight_grad / bias_grad, which are
# recorded under their own names) and the root scale
NOT_KERNELS = {"begin_deferred_acc", "flush_acc", "grad_scale", "scale_grads", "acc", "acc_wgrad", "acc_wbgrad", "acc_bgrad"}


def unknown_public_functions(backward):
    """public functions of s2d_amd/backward.py the recorder has no signature for: a new entry point must not pass unseen"""
    import inspect
    public = {n for n, f in vars(backward).items() if inspect.isfunction(f) and f.__module__ == backward.__name__ and not n.startswith("_")}
    return sorted(public - set(ENTRY_POINTS) - NOT_KERNELS)


@contextlib.contextmanager
def recording(backward, log):
    """wrap every entry point of s2d_amd.backward with a recorder of its shape signature; a call made from inside another recorded
    entry point (conv_weight_grad -> weight_grad, groupnorm_up_relu_backward -> its three steps, ...) belongs to the outer row"""
    saved, depth = {}, [0]

    def wrap(name, fn, sig):
        def rec(*a, **k):
            if depth[0] == 0:
                log.append((name,) + tuple(sig(*a, **k)))
            depth[0] += 1
            try:
                return fn(*a, **k)
            finally:
                depth[0] -= 1
        return rec

    for name, sig in ENTRY_POINTS.items():
        saved[name] = getattr(backward, name)
        setattr(backward, name, wrap(name, saved[name], sig))
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(backward, name, fn)


def record_c4_iteration():
    """the c4 model as tests/test_gpu_fullsize.py::setup builds it, ONE forward_backward under the recorder -> the set of signatures"""
    import bench
    from s2d_amd import backward, ops
    from s2d_amd.modeling import TargetSet, build_kd_model
    dev = torch.device(DEV)
    B, T, H0, W0, Q, P, N = bench.CONFIGS["c4"]
    model = build_kd_model(num_queries=Q, num_frames=T, num_points=P, dropout=0.3).to(dev)
    frames, masks = bench.synth_batch(0, B, T, H0, W0, N, dev)
    bench.calibrate_teacher(model, ops.normalize_pad(frames))
    model.criterion.seed = 0; model.criterion.matcher.seed = 0
    torch.manual_seed(5); ops._DROP_CALLS[0] = 0
    log = []
    with recording(backward, log):
        model.forward_backward(ops.normalize_pad(frames), TargetSet.from_list(masks, device=dev))
        torch.cuda.synchronize()
    del model, frames, masks
    return log


# --------------------------------------------------------------------------- the c4 iteration (recorded; see test_table_covers_the_c4_iteration)
TABLE = [
    ('bias_grad', 14720, 256, None),
    ('bias_grad', 14720, 768, None),
    ('bias_grad', 200, 2, 1.0),
    ('bias_grad', 200, 2, None),
    ('bias_grad', 200, 256, None),
    ('bias_grad', 200, 512, None),
    ('bias_grad', 235520, 256, None),
    ('bias_grad', 235520, 768, None),
    ('bias_grad', 3680, 256, None),
    ('bias_grad', 58880, 256, None),
    ('bias_grad', 58880, 768, None),
    ('bias_grad', 920, 256, None),
    ('bias_grad', 942080, 256, None),
    ('conv_input_grad', 16, 184, 320, 128, 128, 3, 3, 2, 1, True, True),
    ('conv_input_grad', 16, 184, 320, 256, 256, 3, 3, 1, 1, False, False),
    ('conv_input_grad', 16, 184, 320, 256, 512, 1, 1, 2, 0, False, False),
    ('conv_input_grad', 16, 184, 320, 64, 64, 3, 3, 1, 1, True, True),
    ('conv_input_grad', 16, 23, 40, 512, 512, 3, 3, 1, 1, True, True),
    ('conv_input_grad', 16, 46, 80, 1024, 2048, 1, 1, 2, 0, False, False),
    ('conv_input_grad', 16, 46, 80, 256, 256, 3, 3, 1, 1, True, True),
    ('conv_input_grad', 16, 46, 80, 512, 512, 3, 3, 2, 1, True, True),
    ('conv_input_grad', 16, 92, 160, 128, 128, 3, 3, 1, 1, True, True),
    ('conv_input_grad', 16, 92, 160, 256, 256, 3, 3, 2, 1, True, True),
    ('conv_input_grad', 16, 92, 160, 512, 1024, 1, 1, 2, 0, False, False),
    ('conv_weight_grad', 16, 184, 320, 128, 128, 3, 3, 2, 1),
    ('conv_weight_grad', 16, 184, 320, 256, 128, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 184, 320, 256, 256, 3, 3, 1, 1),
    ('conv_weight_grad', 16, 184, 320, 256, 512, 1, 1, 2, 0),
    ('conv_weight_grad', 16, 184, 320, 256, 64, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 184, 320, 64, 256, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 184, 320, 64, 64, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 184, 320, 64, 64, 3, 3, 1, 1),
    ('conv_weight_grad', 16, 23, 40, 2048, 512, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 23, 40, 512, 2048, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 23, 40, 512, 512, 3, 3, 1, 1),
    ('conv_weight_grad', 16, 46, 80, 1024, 2048, 1, 1, 2, 0),
    ('conv_weight_grad', 16, 46, 80, 1024, 256, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 46, 80, 1024, 512, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 46, 80, 256, 1024, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 46, 80, 256, 256, 3, 3, 1, 1),
    ('conv_weight_grad', 16, 46, 80, 512, 512, 3, 3, 2, 1),
    ('conv_weight_grad', 16, 736, 1280, 4, 64, 7, 7, 2, 3),
    ('conv_weight_grad', 16, 92, 160, 128, 128, 3, 3, 1, 1),
    ('conv_weight_grad', 16, 92, 160, 128, 512, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 92, 160, 256, 256, 3, 3, 2, 1),
    ('conv_weight_grad', 16, 92, 160, 512, 1024, 1, 1, 2, 0),
    ('conv_weight_grad', 16, 92, 160, 512, 128, 1, 1, 1, 0),
    ('conv_weight_grad', 16, 92, 160, 512, 256, 1, 1, 1, 0),
    ('groupnorm_backward', 16, 23, 40, 256, 32),
    ('groupnorm_backward', 16, 46, 80, 256, 32),
    ('groupnorm_backward', 16, 92, 160, 256, 32),
    ('groupnorm_up_relu_backward', 16, 184, 320, 256, 32, (92, 160), False),
    ('groupnorm_up_relu_backward', 16, 184, 320, 256, 32, None, True),
    ('input_grad', 1, 768, 256, False, None, False),
    ('input_grad', 14720, 2048, 512, False, (512, 1.0), True),
    ('input_grad', 14720, 256, 2048, False, None, False),
    ('input_grad', 14720, 512, 2048, True, (2048, 1.0), False),
    ('input_grad', 14720, 768, 256, False, None, False),
    ('input_grad', 14720, 768, 256, True, None, False),
    ('input_grad', 19320, 288, 256, False, None, False),
    ('input_grad', 200, 2, 256, True, None, False),
    ('input_grad', 200, 2048, 256, True, None, False),
    ('input_grad', 200, 256, 2048, False, (2048, 1.0), False),
    ('input_grad', 200, 256, 256, False, (256, 1.0), False),
    ('input_grad', 200, 256, 256, False, None, False),
    ('input_grad', 200, 256, 256, True, None, False),
    ('input_grad', 200, 512, 256, False, None, False),
    ('input_grad', 235520, 128, 512, True, (512, 1.0), False),
    ('input_grad', 235520, 256, 512, False, None, False),
    ('input_grad', 235520, 256, 512, True, (512, 1.0), False),
    ('input_grad', 235520, 512, 128, False, (128, 1.0), True),
    ('input_grad', 235520, 768, 256, False, None, False),
    ('input_grad', 235520, 768, 256, True, None, False),
    ('input_grad', 309120, 1024, 256, True, None, False),
    ('input_grad', 309120, 256, 1024, False, (1024, 1.430167555809021), False),
    ('input_grad', 309120, 256, 256, False, None, False),
    ('input_grad', 309120, 544, 256, True, None, False),
    ('input_grad', 58880, 1024, 256, False, (256, 1.0), True),
    ('input_grad', 58880, 256, 1024, False, None, False),
    ('input_grad', 58880, 256, 1024, True, (1024, 1.0), False),
    ('input_grad', 58880, 512, 1024, True, (1024, 1.0), False),
    ('input_grad', 58880, 768, 256, False, None, False),
    ('input_grad', 58880, 768, 256, True, None, False),
    ('input_grad', 942080, 128, 256, True, (256, 1.0), False),
    ('input_grad', 942080, 256, 256, False, None, False),
    ('input_grad', 942080, 256, 64, False, (64, 1.0), True),
    ('input_grad', 942080, 256, 64, False, None, False),
    ('input_grad', 942080, 64, 256, True, (256, 1.0), False),
    ('input_grad', 942080, 64, 64, True, None, False),
    ('layernorm_backward', 200, 256, False),
    ('layernorm_backward', 309120, 256, False),
    ('masked_attn_backward', 2, 100, 100, 256, 8, False, False, 512, 256, None, None),
    ('masked_attn_backward', 2, 100, 117760, 256, 8, True, True, 768, 768, 768, 768),
    ('masked_attn_backward', 2, 100, 29440, 256, 8, True, True, 768, 768, 768, 768),
    ('masked_attn_backward', 2, 100, 7360, 256, 8, True, True, 768, 768, 768, 768),
    ('maxpool_backward', 16, 368, 640, 64, True),
    ('msda_fused_backward', 16, 256, ((23, 40), (46, 80), (92, 160)), 544, 544, 288, 8, 4, True),
    ('relu_gate_add', 120586240),
    ('relu_gate_add', 241172480),
    ('relu_gate_add', 60293120),
    ('relu_scale_backward', 14720, 2048, True, True, True),
    ('relu_scale_backward', 3768320, 64, True, True, False),
    ('sum_slices', 16, 10510080),
    ('sum_slices', 2, 25600),
    ('weight_grad', 14720, 256, 2048, None, None),
    ('weight_grad', 14720, 768, 256, None, 0.0),
    ('weight_grad', 14720, 768, 256, None, None),
    ('weight_grad', 19320, 288, 256, None, None),
    ('weight_grad', 200, 2, 256, 1.0, None),
    ('weight_grad', 200, 2, 256, None, None),
    ('weight_grad', 200, 2048, 256, None, 0.0),
    ('weight_grad', 200, 256, 2048, None, 0.0),
    ('weight_grad', 200, 256, 256, 1.0, 1.0),
    ('weight_grad', 200, 256, 256, None, 0.0),
    ('weight_grad', 200, 256, 256, None, None),
    ('weight_grad', 200, 512, 256, None, None),
    ('weight_grad', 235520, 256, 512, None, None),
    ('weight_grad', 235520, 768, 256, None, 0.0),
    ('weight_grad', 235520, 768, 256, None, None),
    ('weight_grad', 309120, 1024, 256, None, 0.0),
    ('weight_grad', 309120, 256, 1024, None, 0.0),
    ('weight_grad', 309120, 256, 256, None, 0.0),
    ('weight_grad', 309120, 544, 256, None, 0.0),
    ('weight_grad', 471040, 120, 256, None, None),
    ('weight_grad', 58880, 256, 1024, None, None),
    ('weight_grad', 58880, 768, 256, None, 0.0),
    ('weight_grad', 58880, 768, 256, None, None),
    ('weight_grad', 942080, 256, 256, None, None),
]


def _row_id(row):
    return "-".join(str(v).replace(" ", "") for v in row)


def test_table_covers_the_c4_iteration():
    """every (entry point, signature) the benchmarked iteration makes is a row of TABLE -- a dispatch change that brings a new shape or
    branch into the iteration fails here until the row (and with it the float64 comparison) is added"""
    from s2d_amd import backward
    assert not unknown_public_functions(backward), unknown_public_functions(backward)
    seen = set(record_c4_iteration())
    assert len(seen) > 100
    table = set(TABLE)
    assert len(table) == len(TABLE)
    for row in sorted(table - seen, key=repr):
        print("c4table: row no longer used by the iteration:", row)
    missing = sorted(seen - table, key=repr)
    assert not missing, missing


# --------------------------------------------------------------------------- comparison
class _Rep:
    """collects one row's figures: prints every one, asserts at the end"""

    def __init__(self, row):
        self.row, self.bad = _row_id(row), []

    def cmp(self, name, got, r64, r32, small, den=None, keep=None):
        """got: the kernel's result; r64 / r32: the restatement in float64 / float32; small: the bound asserted at small size;
        den: max(|A| . |B|) of a contraction; keep: bool mask of the elements compared (None: all)"""
        assert got.shape == r64.shape, (name, got.shape, r64.shape)
        top = max(float(r64.abs().max()), 1e-30)
        dk, d32 = (got.double() - r64).abs(), (r32.double() - r64).abs()
        if keep is not None:
            dk, d32 = dk * keep, d32 * keep
        err = float(dk.max())
        e32 = float(d32.max()) / top
        bound = max(small, 2.0 * e32)
        inv = "-" if den is None else "%.3e" % (err / max(float(den), 1e-30))
        print(f"c4row {self.row} {name}: kernel {err / top:.3e} f32-torch {e32:.3e} bound {bound:.3e} scale-inv {inv}")
        if not err / top < bound:
            self.bad.append((name, err / top, bound))

    def close(self, name, a, b, bound):
        """two forms of one kernel against each other: max|a - b| / max|b| < bound"""
        r = float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"c4row {self.row} {name}: rel {r:.3e} bound {bound:.3e}")
        if not r < bound:
            self.bad.append((name, r, bound))

    def same(self, name, a, b):
        ok = torch.equal(a, b)
        print(f"c4row {self.row} {name}: {'bitwise equal' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append((name, "not bitwise equal"))

    def done(self):
        assert not self.bad, self.bad


def _gen(row):
    import zlib
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(row).encode()))


def _rn(g, *shape):
    return torch.randn(shape, device=DEV, generator=g)


def _leaf(t, dtype):
    """a fresh differentiable copy of an operand in `dtype` (the operand itself stays as it is)"""
    return t.detach().to(dtype).clone().requires_grad_(True)


@contextlib.contextmanager
def _flag(module, name, value):
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


# --------------------------------------------------------------------------- restatements (plain torch, any dtype, on the device)
F64, F32 = torch.float64, torch.float32


def _out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def _conv_wgrad(dy, x, KH, KW, stride, pad, dtype):
    """dW[:, ky, kx, :] = dY^T . X_shift: one matmul per tap on the strided view of the zero-padded input"""
    N, Ho, Wo, Co = dy.shape
    Ci = x.shape[3]
    xp = torch.nn.functional.pad(x.to(dtype), (0, 0, pad, pad, pad, pad))
    dyt = dy.to(dtype).reshape(-1, Co).t()
    dw = torch.empty((Co, KH, KW, Ci), device=x.device, dtype=dtype)
    for ky in range(KH):
        for kx in range(KW):
            xs = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            dw[:, ky, kx] = dyt @ xs.reshape(-1, Ci)
    return dw


def _conv_dgrad(dy, w, stride, pad, H, W, dtype, gate=None, scale=None):
    """the transposed statement: every tap adds dY . W[:, ky, kx, :] onto its strided view of the zero-padded input gradient"""
    N, Ho, Wo, Co = dy.shape
    _, KH, KW, Ci = w.shape
    dxp = torch.zeros((N, H + 2 * pad, W + 2 * pad, Ci), device=dy.device, dtype=dtype)
    d2, wd = dy.to(dtype).reshape(-1, Co), w.to(dtype)
    for ky in range(KH):
        for kx in range(KW):
            dxp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] += (d2 @ wd[:, ky, kx]).view(N, Ho, Wo, Ci)
    dx = dxp[:, pad:pad + H, pad:pad + W]
    if scale is not None:
        dx = dx * scale.to(dtype)
    if gate is not None:
        dx = torch.where(gate > 0, dx, torch.zeros((), device=dx.device, dtype=dtype))
    return dx.contiguous()


def _layernorm_grads(x, r, dy, gam, dtype):
    C = x.shape[-1]
    xd, gd, bd = _leaf(x, dtype), _leaf(gam, dtype), _leaf(torch.zeros_like(gam), dtype)
    inp = xd if r is None else xd + r.to(dtype)
    (torch.nn.functional.layer_norm(inp, (C,), gd, bd, 1e-5) * dy.to(dtype)).sum().backward()
    return xd.grad, gd.grad, bd.grad


def _groupnorm_expr(x, gam, bet, u, gate, G, dtype):
    """x / u NHWC -> (y NHWC, the leaves).  gate: the ReLU output the backward kernel reads (NHWC; None: no ReLU) -- the ReLU is applied
    through that fixed mask in every dtype, so a float32 evaluation differs from float64 by arithmetic only, never by a flipped gate"""
    xd, gd, bd = _leaf(x, dtype), _leaf(gam, dtype), _leaf(bet, dtype)
    ud = None if u is None else _leaf(u, dtype)
    y = torch.nn.functional.group_norm(xd.permute(0, 3, 1, 2), G, gd, bd, 1e-5)
    if ud is not None:
        y = y + torch.nn.functional.interpolate(ud.permute(0, 3, 1, 2), size=tuple(x.shape[1:3]), mode="bilinear", align_corners=False)
    y = y.permute(0, 2, 3, 1)
    if gate is not None:
        y = y * (gate > 0)
    return y, (xd, gd, bd, ud)


def _msda_grads(value, oa, go, shapes, dtype, step=4):
    """autograd of tests/test_gpu_backward.py::_msda_fused_torch on the device, `step` batch entries at a time"""
    from tests.test_gpu_backward import _msda_fused_torch
    dv, do = [], []
    with torch.device(DEV):
        for n in range(0, value.shape[0], step):
            v, o = _leaf(value[n:n + step], dtype), _leaf(oa[n:n + step], dtype)
            (_msda_fused_torch(v, shapes, o) * go[n:n + step].to(dtype)).sum().backward()
            dv.append(v.grad); do.append(o.grad)
    return torch.cat(dv), torch.cat(do)


_EDGE_PX = 1e-4


def _msda_away_from_cell_edges(oa, shapes, M, P):
    """-> (bool [N,S,M*L*P*2]: the offset elements whose sample lies more than _EDGE_PX pixels from every pixel-cell edge, number of samples
    that do not).  The bilinear sample is continuous in its position, so the value and logit gradients are continuous too; its DERIVATIVE by
    the position -- the offset gradient -- jumps where the position crosses an integer pixel coordinate.  A sample position in float32
    (coordinates up to 160, a few roundings of 2^-24 relative each: < 5e-5 px off) can sit in the neighbouring cell of the float64 one only
    inside that margin; there the float64 value is not a reference for a float32 evaluation, anyone's."""
    N, S, _ = oa.shape
    L = len(shapes)
    ref = []
    for (H, W) in shapes:
        yy, xx = torch.meshgrid(torch.arange(H, dtype=F64, device=DEV), torch.arange(W, dtype=F64, device=DEV), indexing="ij")
        ref.append(torch.stack([(xx.reshape(-1) + 0.5) / W, (yy.reshape(-1) + 0.5) / H], -1))
    ref = torch.cat(ref, 0)                                                       # [S,2] (x, y), normalised
    wh = torch.tensor([[w, h] for (h, w) in shapes], dtype=F64, device=DEV)       # [L,2]
    pos = ref[None, :, None, None, None, :] * wh[None, None, None, :, None, :] - 0.5 + oa[..., :M * L * P * 2].double().reshape(N, S, M, L, P, 2)
    near = ((pos - pos.round()).abs() < _EDGE_PX).any(-1, keepdim=True)           # either coordinate: both components of the sample go
    return (~near).expand(N, S, M, L, P, 2).reshape(N, S, M * L * P * 2), int(near.sum())


def _attn_grads(q, k, v, dout, mask, H, dtype):
    from tests.test_gpu_backward import _masked_attn_torch
    qd, kd, vd = (_leaf(t, dtype) for t in (q, k, v))
    (_masked_attn_torch(qd, kd, vd, mask, H) * dout.to(dtype)).sum().backward()
    return qd.grad, kd.grad, vd.grad


def _pack_bits(mask):
    """mask [B,Q,K] bool (True: masked) -> (bits int32 [B,K,4]: bit q of a key's words, unmasked int32 [B,4]: bit q set when query q has a free key)"""
    B, Q, K = mask.shape
    words = torch.zeros((B, K, 4), device=mask.device, dtype=torch.int64)
    unw = torch.zeros((B, 4), device=mask.device, dtype=torch.int64)
    free = (~mask).any(-1)
    for q in range(Q):
        words[:, :, q >> 5] |= mask[:, q, :].long() << (q & 31)
        unw[:, q >> 5] |= free[:, q].long() << (q & 31)
    wrap = lambda t: ((t + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).contiguous()
    return wrap(words), wrap(unw)


# --------------------------------------------------------------------------- one case per entry point
def _case_conv_weight_grad(rep, g, N, H, W, Ci, Co, KH, KW, stride, pad):
    from s2d_amd import backward as B
    Ho, Wo = _out_hw(H, W, KH, KW, stride, pad)
    x, dy = _rn(g, N, H, W, Ci), _rn(g, N, Ho, Wo, Co)
    dw = B.conv_weight_grad(dy, x, KH, KW, stride, pad)
    rep.same("dW second call", B.conv_weight_grad(dy, x, KH, KW, stride, pad), dw)
    r64, r32 = _conv_wgrad(dy, x, KH, KW, stride, pad, F64), _conv_wgrad(dy, x, KH, KW, stride, pad, F32)
    den = _conv_wgrad(dy.abs(), x.abs(), KH, KW, stride, pad, F32).max()
    rep.cmp("dW", dw, r64, r32, 5e-6, den)
    if KH > 1 and Ci * KH * KW > 256:
        assert B._CONV_WGRAD_IMPLICIT
        with _flag(B, "_CONV_WGRAD_IMPLICIT", False):
            dw0 = B.conv_weight_grad(dy, x, KH, KW, stride, pad)
        rep.cmp("dW padded-copy form", dw0, r64, r32, 5e-6, den)


def _case_conv_input_grad(rep, g, N, H, W, Ci, Co, KH, KW, stride, pad, gated, scaled):
    from s2d_amd import backward as B
    Ho, Wo = _out_hw(H, W, KH, KW, stride, pad)
    w, dy = _rn(g, Co, KH, KW, Ci) / (Ci * KH * KW) ** 0.5, _rn(g, N, Ho, Wo, Co)
    gate = torch.relu(_rn(g, N, H, W, Ci)) if gated else None              # a ReLU output: exact zeros where the gradient stops
    sc = torch.rand((Ci,), device=DEV, generator=g) + 0.5 if scaled else None
    dx = B.conv_input_grad(dy, w, stride, pad, (H, W), gate=gate, scale=sc)
    rep.same("dX second call", B.conv_input_grad(dy, w, stride, pad, (H, W), gate=gate, scale=sc), dx)
    r64, r32 = _conv_dgrad(dy, w, stride, pad, H, W, F64, gate, sc), _conv_dgrad(dy, w, stride, pad, H, W, F32, gate, sc)
    den = _conv_dgrad(dy.abs(), w.abs(), stride, pad, H, W, F32, None, sc).max()
    rep.cmp("dX", dx, r64, r32, 2e-6, den)
    if stride == 2 and KH == 3:
        assert B._CONV_DGRAD_S2
        with _flag(B, "_CONV_DGRAD_S2", False):
            dx0 = B.conv_input_grad(dy, w, stride, pad, (H, W), gate=gate, scale=sc)
        rep.cmp("dX zero-dilated form", dx0, r64, r32, 2e-6, den)


def _case_weight_grad(rep, g, M, N, K, beta, bias_beta):
    from s2d_amd import backward as B
    dy, x = _rn(g, M, N), _rn(g, M, K)
    out0 = _rn(g, N, K) if beta is not None else None
    b0 = _rn(g, N) if bias_beta is not None else None

    def run(deferred):
        out, bo = (None if out0 is None else out0.clone()), (None if b0 is None else b0.clone())
        if deferred:
            B.begin_deferred_acc()
        try:
            dw = B.weight_grad(dy, x, out=out, beta=beta or 0.0, bias_out=bo, bias_beta=bias_beta or 0.0)
        finally:
            if deferred:
                B.flush_acc(end=True)
        return dw, bo

    r = {}
    for dt in (F64, F32):
        dw = dy.to(dt).t() @ x.to(dt)
        db = dy.to(dt).sum(0)
        r[dt] = (dw if not beta else dw + beta * out0.to(dt), db if not bias_beta else db + bias_beta * b0.to(dt))
    den_w = (dy.abs().t() @ x.abs()).max() + (out0.abs().max() if beta else 0.0)
    den_b = dy.abs().sum(0).max() + (b0.abs().max() if bias_beta else 0.0)
    # the iteration accumulates (beta = 1) between begin_deferred_acc and flush_acc: a one-slice result then joins the pending multi-tensor add
    for deferred in ((False, True) if beta == 1.0 else (False,)):
        tag = " deferred add" if deferred else ""
        dw, db = run(deferred)
        dw2, db2 = run(deferred)
        rep.same("dW second call" + tag, dw2, dw)
        rep.cmp("dW" + tag, dw, r[F64][0], r[F32][0], 5e-6, den_w)
        if db is not None:
            rep.same("db second call" + tag, db2, db)
            rep.cmp("db" + tag, db, r[F64][1], r[F32][1], 5e-6, den_b)


def _case_input_grad(rep, g, M, N, K, has_res, gs, scaled):
    from s2d_amd import backward as B
    dy, w = _rn(g, M, N), _rn(g, N, K) / K ** 0.5
    res = _rn(g, M, K) if has_res else None
    gate = torch.relu(_rn(g, M, K)) if gs is not None else None
    assert gs is None or gs[0] == K                                     # the recorded gates are contiguous
    gsc = 1.0 if gs is None else gs[1]
    sc = torch.rand((K,), device=DEV, generator=g) + 0.5 if scaled else None
    run = lambda: B.input_grad(dy, w, res=res, gate=gate, gate_scale=gsc, scale=sc)
    dx = run()
    rep.same("dX second call", run(), dx)

    def ref(dy, w, res, dt, gate=gate):
        r = dy.to(dt) @ w.to(dt)
        if sc is not None:
            r = r * sc.to(dt)
        if res is not None:
            r = r + res.to(dt)
        if gate is not None:
            r = torch.where(gate > 0, r * gsc, torch.zeros((), device=DEV, dtype=dt))
        return r
    den = ref(dy.abs(), w.abs(), None if res is None else res.abs(), F32, None).max() * gsc
    rep.cmp("dX", dx, ref(dy, w, res, F64), ref(dy, w, res, F32), 2e-6, den)


def _case_bias_grad(rep, g, M, N, beta):
    from s2d_amd import backward as B
    dy = _rn(g, M, N)
    o0 = _rn(g, N) if beta is not None else None
    run = lambda: B.bias_grad(dy, out=None if o0 is None else o0.clone(), beta=beta or 0.0)
    db = run()
    rep.same("db second call", run(), db)
    ref = lambda dt: dy.to(dt).sum(0) + (beta * o0.to(dt) if beta else 0.0)
    rep.cmp("db", db, ref(F64), ref(F32), 5e-6, dy.abs().sum(0).max() + (beta * o0.abs().max() if beta else 0.0))


def _case_layernorm_backward(rep, g, rows, C, has_res):
    from s2d_amd import backward as B
    x, dy, gam = _rn(g, rows, C), _rn(g, rows, C), _rn(g, C)
    r = _rn(g, rows, C) if has_res else None
    got = B.layernorm_backward(x, dy, gam, r)
    again = B.layernorm_backward(x, dy, gam, r)
    r64, r32 = _layernorm_grads(x, r, dy, gam, F64), _layernorm_grads(x, r, dy, gam, F32)
    for i, name in enumerate(("dX", "dgamma", "dbeta")):
        rep.same(name + " second call", again[i], got[i])
        rep.cmp(name, got[i], r64[i], r32[i], 5e-6)


def _groupnorm_case(rep, g, N, H, W, C, G, up, relu, fused):
    from s2d_amd import backward as B
    x, dy, gam, bet = _rn(g, N, H, W, C), _rn(g, N, H, W, C), _rn(g, C), _rn(g, C)
    u = _rn(g, N, up[0], up[1], C) if up else None
    refs = {}
    with torch.no_grad():                                             # the forward's output (float64 evaluation, rounded), which the ReLU gate reads
        y_op = _groupnorm_expr(x, gam, bet, u, None, G, F64)[0]
        y_op = (torch.relu(y_op) if relu else y_op).float().contiguous()
    for dt in (F64, F32):
        y, leaves = _groupnorm_expr(x, gam, bet, u, y_op if relu else None, G, dt)
        (y * dy.to(dt)).sum().backward()
        refs[dt] = [None if t is None else t.grad for t in leaves]
        del y, leaves
    run = (lambda: B.groupnorm_up_relu_backward(x, y_op, dy, G, gam, up, relu)) if fused else (lambda: B.groupnorm_backward(x, dy, G, gam))
    got, again = run(), run()
    for i, (name, small) in enumerate((("dX", 1e-5), ("dgamma", 1e-5), ("dbeta", 1e-5), ("dup", 2e-6))):
        if i < len(got) and got[i] is not None:
            rep.same(name + " second call", again[i], got[i])
            rep.cmp(name, got[i], refs[F64][i], refs[F32][i], small)


def _case_groupnorm_up_relu_backward(rep, g, N, H, W, C, G, up, relu):
    _groupnorm_case(rep, g, N, H, W, C, G, up, relu, True)


def _case_groupnorm_backward(rep, g, N, H, W, C, G):
    _groupnorm_case(rep, g, N, H, W, C, G, None, False, False)


def _case_maxpool_backward(rep, g, N, H, W, C, with_idx):
    from s2d_amd import backward as B, ops
    x = torch.relu(_rn(g, N, H, W, C))                                  # ReLU outputs: many exact ties at 0, the first maximum takes the gradient
    dy = _rn(g, N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    idx = ops.maxpool3x3s2(x, want_idx=True)[1] if with_idx else None
    dx = B.maxpool_backward(x, dy, idx)
    rep.same("dX second call", B.maxpool_backward(x, dy, idx), dx)
    refs = {}
    for dt in (F64, F32):
        xd = _leaf(x, dt)
        (torch.nn.functional.max_pool2d(xd.permute(0, 3, 1, 2), 3, 2, 1) * dy.to(dt).permute(0, 3, 1, 2)).sum().backward()
        refs[dt] = xd.grad
    # routing is exact; a pixel that is the arg-max of several windows adds 2..4 gradients (test_maxpool_backward_vs_autograd: rtol 2e-6, atol 1e-6)
    same = torch.equal(dx != 0, refs[F64] != 0)
    print(f"c4row {rep.row} dX routing: {'same pixels' if same else 'DIFFERS'}")
    if not same:
        rep.bad.append(("dX routing",))
    rep.cmp("dX", dx, refs[F64], refs[F32], 2e-6)


def _case_msda_fused_backward(rep, g, N, C, shapes, vstride, ostride, owidth, M, P, merged):
    from s2d_amd import backward as B
    S = sum(h * w for h, w in shapes)
    assert merged and vstride == ostride == owidth + C                   # as the decoder calls it: column slices of the merged projection output
    both = torch.cat([_rn(g, N, S, 2 * owidth // 3) * 2.0, _rn(g, N, S, owidth // 3), _rn(g, N, S, C)], -1)   # offsets of several pixels: samples leave the maps
    oa, value, go = both[..., :owidth], both[..., owidth:], _rn(g, N, S, C)
    shp = [tuple(s) for s in shapes]
    dv, doa, buf = B.msda_fused_backward(value, shp, oa, go, M=M, P=P, merged=True)
    dv2, doa2, _ = B.msda_fused_backward(value, shp, oa, go, M=M, P=P, merged=True)
    rep.same("d_value second call", dv2, dv)
    rep.same("d_offs_logits second call", doa2, doa)
    rep.same("merged buffer holds both", torch.cat([doa, dv], -1), buf)
    (v64, o64), (v32, o32) = _msda_grads(value, oa, go, shp, F64), _msda_grads(value, oa, go, shp, F32)
    rep.cmp("d_value", dv, v64, v32, 1e-5)
    # the offset gradient is compared where float64 is a reference for it (see _msda_away_from_cell_edges); the logit gradient everywhere
    L = len(shp)
    away, n_near = _msda_away_from_cell_edges(oa, shp, M, P)
    n_samples = N * S * M * L * P
    # fractional pixel positions are spread evenly: 2 coordinates x 2 _EDGE_PX of every cell = 4e-4 of the samples expected; cap at 1e-3
    print(f"c4row {rep.row} samples within {_EDGE_PX} px of a cell edge (offset gradient not compared there): {n_near} of {n_samples}")
    if not n_near < 1e-3 * n_samples:
        rep.bad.append(("too many samples excluded", n_near, n_samples))
    keep = torch.cat([away, torch.ones((N, S, owidth - away.shape[-1]), device=DEV, dtype=torch.bool)], -1)
    rep.cmp("d_offs_logits (all elements, figure only)", doa, o64, o32, float("inf"))
    rep.cmp("d_offs_logits", doa, o64, o32, 1e-5, keep=keep)
    assert B._MSDA_BWD_REC
    with _flag(B, "_MSDA_BWD_REC", False):
        dv0, doa0, _ = B.msda_fused_backward(value, shp, oa, go, M=M, P=P, merged=True)
    rep.same("d_value two-step form", dv0, dv)
    rep.cmp("d_offs_logits two-step form", doa0, o64, o32, 1e-5, keep=keep)
    rep.close("d_offs_logits record form vs two-step form", doa, doa0, 2e-6)     # test_msda_fused_backward_vs_autograd's bound, every element


def _case_masked_attn_backward(rep, g, Bc, Q, K, C, H, has_bits, has_unm, ks, vs, dks, dvs):
    from s2d_amd import backward as B, ops
    q, dout = _rn(g, Bc, Q, C), _rn(g, Bc, Q, C)
    assert has_bits == has_unm and dks == dvs
    if ks == vs:                                                           # k | v: the last two column blocks of one [B,K,ks] buffer
        kv = torch.zeros((Bc, K, ks), device=DEV)
        k, v = kv[..., ks - 2 * C:ks - C], kv[..., ks - C:]
    else:                                                                  # k a column block of its own buffer, v of another
        k, v = torch.zeros((Bc, K, ks), device=DEV)[..., ks - C:], torch.zeros((Bc, K, vs), device=DEV)[..., vs - C:]
    k.copy_(_rn(g, Bc, K, C)); v.copy_(_rn(g, Bc, K, C))
    assert (k.stride(1), v.stride(1)) == (ks, vs)
    mask = torch.rand((Bc, Q, K), device=DEV, generator=g) < 0.6 if has_bits else torch.zeros((Bc, Q, K), device=DEV, dtype=torch.bool)
    bits = unm = None
    if has_bits:
        mask[0, 3] = True                                                  # a query with every key masked attends everywhere
        bits, unm = _pack_bits(mask)
    o_h, lse = ops.masked_attn(q, k, v, bits, unm, H=H, want_lse=True)

    def run():
        wide = torch.zeros((Bc, K, dks), device=DEV) if dks else None
        dk_out = None if dks is None else wide[..., dks - 2 * C:dks - C]
        dv_out = None if dvs is None else wide[..., dvs - C:]
        got = B.masked_attn_backward(q, k, v, o_h, lse, dout, bits, unm, H=H, dk_out=dk_out, dv_out=dv_out)
        if wide is not None:                                               # the columns in front of the two slices belong to someone else
            clean = not bool(wide[..., :dks - 2 * C].any())
            print(f"c4row {rep.row} columns outside dk_out / dv_out: {'untouched' if clean else 'WRITTEN'}")
            if not clean:
                rep.bad.append(("columns outside dk_out / dv_out written",))
        return got
    got, again = run(), run()
    r64, r32 = _attn_grads(q, k, v, dout, mask, H, F64), _attn_grads(q, k, v, dout, mask, H, F32)
    for i, name in enumerate(("dQ", "dK", "dV")):
        rep.same(name + " second call", again[i], got[i])
        rep.cmp(name, got[i], r64[i], r32[i], 2e-5)


def _case_relu_scale_backward(rep, g, rows, C, has_y, has_scale, want_res):
    from s2d_amd import backward as B
    dy = _rn(g, rows, C)
    y = torch.relu(_rn(g, rows, C)) if has_y else None
    sc = torch.rand((C,), device=DEV, generator=g) + 0.5 if has_scale else None
    got = B.relu_scale_backward(dy, y, sc, want_res=want_res)
    dres = dy * (y > 0) if has_y else dy
    rep.same("dz == dy * (y > 0) * scale", got[0] if want_res else got, dres * sc if has_scale else dres)
    if want_res:
        rep.same("dres == dy * (y > 0)", got[1], dres)


def _case_relu_gate_add(rep, g, n):
    from s2d_amd import backward as B
    a, b, y = _rn(g, n // 256, 256), _rn(g, n // 256, 256), torch.relu(_rn(g, n // 256, 256))
    rep.same("a + g * (y > 0)", B.relu_gate_add(a, b, y), a + torch.where(y > 0, b, torch.zeros_like(b)))


def _case_sum_slices(rep, g, S, n):
    from s2d_amd import backward as B
    x = _rn(g, S, n)
    out = B.sum_slices(x)
    rep.same("second call", B.sum_slices(x), out)
    # the last step of every weight gradient (S float32 additions in a fixed order), held to the weight gradients' bound
    rep.cmp("sum", out, x.double().sum(0), x.sum(0), 5e-6, x.abs().sum(0).max())


@pytest.mark.parametrize("row", TABLE, ids=_row_id)
def test_c4_row_vs_float64(row):
    case = globals()["_case_" + row[0]]
    rep = _Rep(row)
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False                         # the float32 restatement is plain float32
    try:
        case(rep, _gen(row), *row[1:])
        torch.cuda.synchronize()
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    rep.done()


# --------------------------------------------------------------------------- index arithmetic of the 3 x 3 weight gradient, kept small
_HW = [(2, 320), (3, 129), (5, 128), (7, 127), (63, 65), (64, 64), (65, 63), (127, 7), (128, 5), (129, 3), (320, 2)]     # (Ho, Wo): powers of two, neighbours, primes


@pytest.mark.parametrize("Ci", [16, 32, 128])          # 16: im2col (Ci * 9 <= 256); 32: the 64-wide tile; 128: the 128-wide tile
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Ho,Wo", _HW)
def test_conv_weight_grad_index_arithmetic(Ho, Wo, stride, Ci, monkeypatch):
    """3 x 3 / pad 1 weight gradient, N = 3, output sizes around the powers of two (the magic-number divisions by Wo and Ho), odd input sizes
    under stride 2, and -- backward._slices replaced on the Python side -- slice boundaries at arbitrary (n, yo, xo): one slice, 32
    positions per slice, a chunk that does not divide a row, a chunk longer than one image.  Same float64 reference, same bound rule."""
    from s2d_amd import backward as B
    row = ("conv_weight_grad_index", Ho, Wo, stride, Ci)
    N, Co = 3, 12
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo - 1)
    assert _out_hw(H, W, 3, 3, stride, 1) == (Ho, Wo)
    g = _gen(row)
    x, dy = _rn(g, N, H, W, Ci), _rn(g, N, Ho, Wo, Co)
    r64, r32 = _conv_wgrad(dy, x, 3, 3, stride, 1, F64), _conv_wgrad(dy, x, 3, 3, stride, 1, F32)
    den = _conv_wgrad(dy.abs(), x.abs(), 3, 3, stride, 1, F32).max()
    rep = _Rep(row)
    rep.cmp("dW default slices", B.conv_weight_grad(dy, x, 3, 3, stride, 1), r64, r32, 5e-6, den)
    P = N * Ho * Wo
    up32 = lambda v: (v + 31) // 32 * 32
    for chunk in (up32(P), 32, 96 if 96 % Wo else 160, up32(Ho * Wo + 32)):
        S = (P + chunk - 1) // chunk
        monkeypatch.setattr(B, "_slices", lambda M, out_tiles, slots=512, c=chunk: ((M + c - 1) // c, c))
        dw = B.conv_weight_grad(dy, x, 3, 3, stride, 1)
        rep.same(f"dW S={S} chunk={chunk} second call", B.conv_weight_grad(dy, x, 3, 3, stride, 1), dw)
        rep.cmp(f"dW S={S} chunk={chunk}", dw, r64, r32, 5e-6, den)
    rep.done()
