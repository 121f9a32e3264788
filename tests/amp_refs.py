"""Exact references of the AMP dense mode (s2d_amd/csrc/gemm_amp.hip: both operands rounded to fp16, round-to-nearest-even, products
accumulated in f32, f32 out), the table of its launch forms, and the operand values at which a conversion can go wrong.  Plain numpy in
float64 / int64: nothing of s2d_amd.  tests/test_amp_refs_cpu.py pins this module; tests/test_gpu_amp_forms.py holds the kernels to it.

A *form* is what selects a branch of gemm_amp.hip, without sizes (gemm_form / conv_form).  GEMM_ROWS / CONV_ROWS give every form at the
smallest sizes at which the 128 x 128 x 64 tile (four waves of 64 x 64, double-buffered LDS, workgroup ids remapped over 8 XCDs) can still
go wrong; the CPU test checks that the sizes cover what they are meant to cover."""
import numpy as np

F64 = np.float64

# Measured on gfx950 (profiles/amp_parity.txt): v_mfma_f32_32x32x16_f16 takes fp16 subnormal operands at their exact value, and
# v_cvt_f16_f32 produces them.  True would mean: an operand whose fp16 image is subnormal contributes exactly nothing.
FLUSH_SUBNORMAL_OPERANDS = False
F16_MIN_NORMAL = 2.0 ** -14


def round_fp16(a, flush=None):
    """float32 array -> float64 array holding the fp16 image of every element (nearest, ties to even; beyond 65520 in magnitude +-inf;
    NaN stays NaN), as numpy's astype(float16) computes it.  flush (default: FLUSH_SUBNORMAL_OPERANDS): subnormal images become 0"""
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = a.astype(np.float16).astype(F64)
    if FLUSH_SUBNORMAL_OPERANDS if flush is None else flush:
        h = np.where(np.abs(h) < F16_MIN_NORMAL, 0.0 * h, h)
    return h


# --------------------------------------------------------------------------- the operations, in float64 on the operands as given
def ref_gemm_nt(A, B, scale=None, bias=None, res=None, relu=False, res_rows=0, res_cols=0):
    """act(A[(b), M, K] @ B[(b), N, K]^T * scale + bias + res): res is [(b), M or res_rows, ldr]; row r takes res[r % res_rows] when
    res_rows > 0, and only the first res_cols columns take it when res_cols > 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(A, F64) @ np.swapaxes(np.asarray(B, F64), -1, -2)
        M, N = v.shape[-2:]
        if scale is not None:
            v = v * np.asarray(scale, F64)
        if bias is not None:
            v = v + np.asarray(bias, F64)
        if res is not None:
            r = np.asarray(res, F64)
            if res_rows:
                r = np.take(r, np.arange(M) % res_rows, axis=-2)
            c = res_cols or N
            v = np.concatenate([v[..., :c] + r[..., :c], v[..., c:]], -1)
        return np.maximum(v, 0.0) if relu else v


def conv_out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def ref_conv2d_nhwc(x, w, stride=1, pad=0, scale=None, bias=None, res=None, relu=False):
    """x [N, H, W, Ci], w [Co, KH, KW, Ci] -> act(conv(x, w) * scale + bias + res) [N, Ho, Wo, Co]: one matmul per tap on the strided
    view of the zero-padded input"""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    N, H, W, Ci = x.shape
    Co, KH, KW, _ = w.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, Ci), F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    v = np.zeros((N * Ho * Wo, Co), F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for ky in range(KH):
            for kx in range(KW):
                xs = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
                v += xs.reshape(-1, Ci) @ w[:, ky, kx].T
        v = v.reshape(N, Ho, Wo, Co)
        if scale is not None:
            v = v * np.asarray(scale, F64)
        if bias is not None:
            v = v + np.asarray(bias, F64)
        if res is not None:
            v = v + np.asarray(res, F64)
        return np.maximum(v, 0.0) if relu else v


def elementwise_error(got, ref):
    """max |got - ref| / (1 + |ref|): the figure an rtol = atol comparison bounds"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max())


# --------------------------------------------------------------------------- forms
def residual_kind(has_res, batched, res_rows, res_cols, N):
    if not has_res:
        return "none"
    tags = [t for t, on in (("batched", batched), ("periodic", res_rows > 0), ("cols", 0 < res_cols < N)) if on]
    return "+".join(tags) if tags else "full"


def gemm_form(bs, b_batched, M, N, ldc, scale, bias, relu, res_kind):
    """what selects a branch of the AMP GEMM: batched, B per batch, N % 4 == 0 (vector or scalar epilogue), the row stride of `out`
    ("N", "N+4k": padded, still 16-B rows, "N+odd": padded, scalar epilogue), scale / bias / relu given, the residual form, M == 1"""
    pad = "N" if ldc == N else ("N+4k" if (ldc - N) % 4 == 0 else "N+odd")
    return ("gemm_nt", bs > 1, bool(b_batched) and bs > 1, N % 4 == 0, pad, bool(scale), bool(bias), bool(relu), res_kind, M == 1)


def conv_form(Cin, Cout, k, stride, pad, scale, bias, relu, res):
    return ("conv2d_nhwc", (k, stride, pad), Cin == 4, Cout % 4 == 0, bool(scale), bool(bias), bool(relu), bool(res))


def gemm_row_form(row):
    bs, bb, M, N, K, ldc_extra, scale, bias, relu, res = row
    kind = "none" if res is None else (res if isinstance(res, str) else res[0])
    return gemm_form(bs, bb, M, N, N + ldc_extra, scale, bias, relu, kind)


def conv_row_form(row):
    N, H, W, Cin, Cout, k, stride, pad, scale, bias, relu, res = row
    return conv_form(Cin, Cout, k, stride, pad, scale, bias, relu, res)


def gemm_row_vector_epilogue(row):
    """the kernel's own condition: N, ldc, ldr and res_cols all multiples of 4"""
    bs, bb, M, N, K, ldc_extra, scale, bias, relu, res = row
    ldr, rc = (res[2], res[1]) if isinstance(res, tuple) and res[0] == "cols" else (N, N)
    return (N | (N + ldc_extra) | ldr | rc) % 4 == 0


def gemm_row_workgroups(row):
    return -(-row[2] // 128) * -(-row[3] // 128)


# (bs, B per batch, M, N, K, ldc - N, scale, bias, relu, residual): residual None, "full" [M, N], "batched" [bs, M, N],
# ("periodic", res_rows) [res_rows, N] or ("cols", res_cols, ldr) [M, ldr]
M_SET, N_SET, K_SET = (1, 63, 65, 129, 257), (2, 41, 100, 132, 260), (4, 60, 64, 68, 128, 196)
GEMM_ROWS = [
    # 16-B row epilogue
    (1, False, 1, 100, 4, 0, False, True, False, None),                  # the level-embed form: one row, one workgroup, one masked k-tile
    (1, False, 63, 132, 60, 0, True, True, True, "full"),                # a bottleneck's conv3: scale + bias + residual + ReLU
    (1, False, 65, 260, 64, 0, False, True, True, ("periodic", 7)),
    (1, False, 129, 100, 68, 4, False, True, False, ("cols", 8, 12)),
    (1, False, 257, 260, 128, 0, True, True, True, ("periodic", 65)),    # 9 workgroups
    (3, False, 129, 132, 196, 0, False, True, False, "batched"),
    (3, True, 65, 100, 64, 0, False, False, False, None),                # the mask-logit product
    (3, True, 1, 132, 128, 4, False, True, True, None),
    (1, False, 700, 260, 68, 0, False, True, False, "full"),             # 18 workgroups: both branches of the XCD remap; out_proj / linear2
    (1, False, 1000, 260, 4, 0, True, False, False, None),               # 24 workgroups: every XCD the same share
    (1, False, 63, 100, 64, 0, True, True, True, None),                  # a bottleneck's conv1
    (1, False, 65, 132, 128, 0, True, True, False, None),                # a stride-1 shortcut
    (1, False, 129, 260, 60, 0, False, True, False, None),               # q / k / v projections
    (1, False, 63, 100, 196, 0, False, True, True, None),                # linear1, the mask MLP
    # scalar epilogue
    (1, False, 1, 2, 4, 0, False, True, False, None),                    # the class head, class-agnostic
    (1, False, 63, 41, 60, 0, False, True, False, None),                 # the class head, 40 classes
    (1, False, 65, 100, 64, 3, True, True, True, "full"),
    (1, False, 129, 41, 68, 0, False, True, True, "full"),
    (1, False, 257, 260, 128, 3, False, True, False, ("periodic", 7)),   # 9 workgroups
    (3, True, 65, 2, 196, 0, False, False, False, None),
    (3, False, 129, 132, 196, 3, False, True, False, "batched"),
    (1, False, 257, 41, 4, 0, True, False, True, ("periodic", 65)),
    (1, False, 700, 260, 60, 3, False, False, False, ("cols", 8, 12)),   # 18 workgroups
    (1, False, 63, 41, 128, 0, False, True, False, ("cols", 8, 12)),
]

# (N, H, W, Cin, Cout, k, stride, pad, scale, bias, relu, residual)
CONV_ROWS = [
    (1, 33, 47, 4, 64, 7, 2, 3, True, True, True, False),                # the stem
    (2, 9, 11, 64, 64, 3, 1, 1, True, True, True, True),
    (1, 10, 13, 128, 66, 3, 2, 1, True, True, True, False),              # Cout % 4 != 0: scalar epilogue
    (2, 8, 12, 256, 128, 1, 2, 0, True, True, False, False),             # the downsample shortcut
    (1, 5, 5, 8, 132, 3, 1, 1, False, True, False, True),                # K = 72: a tail inside a tap; every output touches the padding
    (2, 9, 11, 64, 64, 3, 1, 1, True, True, True, False),                # a bottleneck's conv2
    (1, 10, 13, 128, 64, 3, 2, 1, True, True, True, False),              # a bottleneck's strided conv2
]


# --------------------------------------------------------------------------- operand values at which a conversion can go wrong
def _f32(v):
    return np.float32(v)


def tie_values():
    """(1 + (2j + 1) 2^-11) 2^e: exactly halfway between two fp16 numbers, for even and odd j, with the float32 neighbours on either
    side; both signs.  j = 1023 rounds up into the next binade.  (e = 15 with j = 1023 is 65520, which overflows: see nonfinite_values)"""
    out = []
    for e, js in ((-14, (0, 1, 2, 1023)), (-3, (0, 1, 510, 1023)), (0, (0, 1, 2, 1023)), (7, (0, 1, 511, 1023)), (15, (0, 1, 1022))):
        for j in js:
            t = _f32((1.0 + (2 * j + 1) * 2.0 ** -11) * 2.0 ** e)
            assert float(t) == (1.0 + (2 * j + 1) * 2.0 ** -11) * 2.0 ** e
            out += [t, np.nextafter(t, _f32(np.inf)), np.nextafter(t, _f32(-np.inf))]
    return np.array(out + [-v for v in out], np.float32)


def edge_values():
    """the largest finite results and both zeros"""
    return np.array([65504.0, 65519.996, -65504.0, -65519.996, 0.0, -0.0, 1.0, -1.0], np.float32)


def subnormal_values():
    """float32 values whose fp16 image is subnormal, zero or the smallest normal number"""
    below = np.nextafter(_f32(2.0 ** -25), _f32(0.0))
    v = [2.0 ** -24, 3 * 2.0 ** -25, below, 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14, 1023 * 2.0 ** -24, 5 * 2.0 ** -24, 2.0 ** -15]
    return np.array(v + [-x for x in v], np.float32)


def nonfinite_values():
    """values whose fp16 image is +-inf or NaN"""
    return np.array([65520.0, 1e5, -65520.0, -1e5, np.nan], np.float32)


# input -> fp16 image, written by hand (tests/test_amp_refs_cpu.py holds round_fp16 to them)
HAND_PINNED = [
    (1.0 + 2.0 ** -11, 1.0), (1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -9), (1.0 + 5 * 2.0 ** -11, 1.0 + 2.0 ** -9),
    (float(np.nextafter(_f32(1.0 + 2.0 ** -11), _f32(2.0))), 1.0 + 2.0 ** -10), (float(np.nextafter(_f32(1.0 + 2.0 ** -11), _f32(0.0))), 1.0),
    (-(1.0 + 2.0 ** -11), -1.0), (2.0 ** 7 * (1.0 + 1023 * 2.0 ** -11), 1.5 * 2.0 ** 7), (2.0 ** 7 * (1.0 + 2047 * 2.0 ** -11), 2.0 ** 8),
    (65504.0, 65504.0), (float(_f32(65519.996)), 65504.0), (65520.0, np.inf), (1e5, np.inf), (-65520.0, -np.inf), (-1e5, -np.inf),
    (0.0, 0.0), (-0.0, -0.0),
    (2.0 ** -24, 2.0 ** -24), (3 * 2.0 ** -25, 2.0 ** -23), (float(np.nextafter(_f32(2.0 ** -25), _f32(0.0))), 0.0), (2.0 ** -25, 0.0),
    (2.0 ** -14 - 2.0 ** -25, 2.0 ** -14), (2.0 ** -14, 2.0 ** -14), (1023 * 2.0 ** -24, 1023 * 2.0 ** -24),
]


def one_hot_operand(K, scales=(0.25, 1.0, 4.0)):
    """[K, K]: row n is zero except entry n, a power of two that cycles through `scales` -> (matrix, the K factors)"""
    s = np.array([scales[n % len(scales)] for n in range(K)], np.float32)
    return np.diag(s).astype(np.float32), s


def latin_rows(values, K):
    """[len(values), K] with element (m, k) = values[(m + k) % len(values)]: every value visits every k"""
    L = len(values)
    return values[(np.arange(L)[:, None] + np.arange(K)[None, :]) % L].astype(np.float32)
