"""Accuracy of the split-fp16 x3 arithmetic across operand magnitudes.

Every fp32 operand of the default dense arithmetic is split as x = h + l * 2^-11 with h = fp16_rtz(x), l = fp16_rtz((x - h) * 2^11),
and A.B^T = Ah.Bh^T + 2^-11 (Ah.Bl^T + Al.Bh^T).  That is fp32-class only while h is a normal fp16 number: the guaranteed window is
an operand tensor amax in [2^-14, 65504].  Below it h and l lose bits, above it the round-toward-zero conversion saturates.

Each launch family is compared with a float64 restatement of the same operation on the metric
    err = max|C - C_ref| / max(|A| . |B|^T)
(the same contraction on absolute values), which is invariant under a power-of-two scaling of either operand:
- inside the window err <= BOUND (2^-17) at every scale, and <= CORE (2^-20) where every operand's amax is >= 2^-8;
- everywhere err <= FACTOR * emu + BOUND, where emu is the error of `split16` below (a numpy restatement of the split rule: the
  operands replaced by h + l * 2^-11, the operation in float64).  A kernel worse than its own rule fails; the rule's own loss of
  bits outside the window is the documented behaviour, and `test_split_rule_window` pins where the window lies from the rule alone.
The model-level contract -- gradient operands are kept inside the window by the power-of-two gradient scale at the root of the
backward (backward.grad_scale), undone exactly where the gradients land -- is tested at the end of the file on the tiny KD parity case."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BOUND = 2.0 ** -17          # inside the window, both operands possibly at its lower edge
CORE, CORE_LO = 2.0 ** -20, 2.0 ** -8      # every operand amax >= 2^-8: the unit-scale class of the kernels
FACTOR = 1.5
WIN_LO, WIN_HI = 2.0 ** -14, 65504.0
SCALES = [-40, -30, -24, -20, -17, -14, -8, 0, 8, 14]       # log2 of the operand's amax
SPAN = 30                                                   # mixed rows: row i has amax 2^-(i * SPAN / (rows - 1)), rounded


def rtz16(x):
    """fp16 round-toward-zero of float32 values (saturating at +-65504, subnormals kept), as float64"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)                            # nearest-even
    bad = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))
    h[bad] = np.nextafter(h[bad], np.float16(0))
    return h.astype(np.float64)


def split_parts(x):
    """(h, l * 2^-11) of the split, float64"""
    x = np.asarray(x, np.float32)
    h = rtz16(x)
    r = (x - h.astype(np.float32)) * np.float32(2048.0)     # exact in float32, as in the kernels
    return h, rtz16(r) / 2048.0


def split16(x):
    """the value the split-fp16 kernels represent x by: h + l * 2^-11 (float64)"""
    h, l = split_parts(x)
    return h + l


def emulate(f, operands):
    """f (outputs at most bilinear in the operands) under the split rule: Ah.Bh + 2^-11 (Ah.Bl + Al.Bh), the l.l product dropped -- it
    is the whole difference once h underflows.  With g(t) = f(h + t l): the kernels compute g(0) + g'(0) = g(0) + (g(1) - g(-1)) / 2."""
    parts = [split_parts(a) for a in operands]
    g = {t: [r.numpy() for r in f(*[torch.from_numpy(h + t * l) for h, l in parts])] for t in (0.0, 1.0, -1.0)}
    return [a + (b - c) / 2 for a, b, c in zip(g[0.0], g[1.0], g[-1.0])]


def in_window(a):
    m = float(np.abs(a).max())
    return m == 0.0 or WIN_LO <= m <= WIN_HI


def unit(shape, seed, rows_span=False):
    """float32 randn with amax exactly 1 (so that power-of-two scalings stay exact); rows_span: row i scaled by 2^-e_i, e_i spread
    over 0..SPAN"""
    g = np.random.default_rng(seed)
    a = g.standard_normal(shape).astype(np.float32)
    a /= np.abs(a).max()
    if rows_span:
        e = np.round(np.linspace(0, SPAN, a.shape[0])).astype(np.int64)
        r = a.reshape(a.shape[0], -1)
        r /= np.abs(r).max(1, keepdims=True)
        r *= np.ldexp(np.float32(1.0), -e)[:, None].astype(np.float32)
        a = r.reshape(a.shape)
    return a.astype(np.float32)


def errs(got, ref, den):
    den = float(den)
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    return e / den if den > 0 else e


class Family:
    """gpu(*operands) -> outputs (numpy), ref(*operands as float64 torch) -> outputs, all operands split by the kernel.
    rows: for each output, the operand whose rows are the output's rows (None: no row correspondence)"""

    def __init__(self, name, shapes, gpu, ref, rows=None):
        self.name, self.shapes, self.gpu, self.ref, self.rows = name, shapes, gpu, ref, rows

    def check(self, ops_np, per_row=False):
        got = self.gpu(*ops_np)
        t = [torch.from_numpy(np.asarray(a, np.float64)) for a in ops_np]
        ref = [r.numpy() for r in self.ref(*t)]
        emu = emulate(self.ref, ops_np)
        den = [r.numpy() for r in self.ref(*[x.abs() for x in t])]
        inside = all(in_window(a) for a in ops_np)
        out = []
        for i, (g, r, e, d) in enumerate(zip(got, ref, emu, den)):
            assert np.isfinite(g).all(), (self.name, i)
            err, eerr = errs(g, r, np.abs(d).max()), errs(e, r, np.abs(d).max())
            assert err <= FACTOR * eerr + BOUND, (self.name, i, err, eerr)
            if inside:
                assert err <= BOUND, (self.name, i, err)
            if all(CORE_LO <= float(np.abs(a).max()) <= WIN_HI for a in ops_np):
                assert err <= CORE, (self.name, i, err)
            out.append((err, eerr))
            if per_row and self.rows is not None and self.rows[i] is not None:
                src = ops_np[self.rows[i]]
                R = src.shape[0]
                g2, r2, e2, d2 = (np.asarray(v, np.float64).reshape(R, -1) for v in (g, r, e, d))
                for row in range(R):
                    dr = np.abs(d2[row]).max()
                    if dr == 0:
                        assert np.all(g2[row] == 0), (self.name, i, row)
                        continue
                    er, eer = errs(g2[row], r2[row], dr), errs(e2[row], r2[row], dr)
                    assert er <= FACTOR * eer + BOUND, (self.name, i, row, er, eer)
                    if in_window(src[row]) and all(in_window(a) for j, a in enumerate(ops_np) if j != self.rows[i]):
                        assert er <= BOUND, (self.name, i, row, er)
        return out


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _n(t):
    return t.detach().double().cpu().numpy()


def _conv_ref(stride, pad):
    # NHWC x, [Co, KH, KW, Ci] w
    return lambda x, w: [torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad)
                         .permute(0, 2, 3, 1)]


def _dgrad_ref(stride, pad, H, W):
    def f(dy, w):
        N, Ho, Wo, Co = dy.shape
        xs = (N, w.shape[3], H, W)
        dx = torch.nn.grad.conv2d_input(xs, w.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), stride=stride, padding=pad)
        return [dx.permute(0, 2, 3, 1)]
    return f


def _wgrad_ref(stride, pad, KH):
    def f(dy, x):
        ws = (dy.shape[3], x.shape[3], KH, KH)
        dw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), ws, dy.permute(0, 3, 1, 2), stride=stride, padding=pad)
        return [dw.permute(0, 2, 3, 1)]
    return f


def _families():
    from s2d_amd import backward, ops
    F = {}

    def gemm(M, N, K, static=False):
        def g(A, B):
            Bt = _d(B)
            if static:
                Bt = ops.mark_static(Bt)
            return [_n(ops.gemm_nt(_d(A), Bt))]
        return Family(f"gemm_nt{'_static' if static else ''}_{M}x{N}x{K}", [(M, K), (N, K)], g, lambda A, B: [A @ B.T], rows=[0])

    F["gemm_nt"] = gemm(700, 288, 260)
    F["gemm_small"] = gemm(100, 256, 256)                                 # M <= 256: the few-rows kernel
    F["gemm_static"] = gemm(700, 256, 256, static=True)                  # cached pre-split image of B

    def presplit(A, B):
        W = ops.mark_static(_d(B))
        M, K = A.shape
        return [_n(ops.gemm_nt_presplit(ops.split_rows(_d(A)), M, K, W))]
    F["gemm_presplit_a"] = Family("gemm_nt_presplit", [(700, 256), (256, 256)], presplit, lambda A, B: [A @ B.T], rows=[0])

    def conv(shape_x, Co, KH, stride, pad, static):
        def g(x, w):
            wt = ops.mark_static(_d(w)) if static else _d(w)
            return [_n(ops.conv2d_nhwc(_d(x), wt, stride, pad))]
        return Family(f"conv{KH}x{KH}s{stride}{'_static' if static else ''}", [shape_x, (Co, KH, KH, shape_x[3])], g, _conv_ref(stride, pad))

    F["conv_implicit"] = conv((2, 23, 40, 64), 64, 3, 1, 1, False)
    F["conv_halo"] = conv((1, 23, 40, 128), 192, 3, 1, 1, True)
    F["conv_stem"] = conv((2, 37, 53, 4), 64, 7, 2, 3, True)

    def lin(M, N, K):
        def g(x, w, dy):
            dx, dw, _ = backward.linear_backward(_d(x), _d(w), _d(dy), has_bias=False)
            return [_n(dx), _n(dw)]
        # dx = dy . w (dy's rows are dx's rows); dw = dy^T . x
        return Family(f"linear_backward_{M}x{N}x{K}", [(M, K), (N, K), (M, N)], g, lambda x, w, dy: [dy @ w, dy.T @ x], rows=[2, None])

    F["linear_backward"] = lin(1000, 256, 96)
    F["linear_backward_pad"] = lin(5000, 100, 256)                      # N % 4 != 0: the zero-padded contraction of the dgrad

    def dgrad(N, H, W, Ci, Co, KH, stride, pad, gate=False, s2=True):
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KH) // stride + 1
        g_ = np.random.default_rng(N + H).standard_normal((N, H, W, Ci)).astype(np.float32)
        sc = np.ldexp(np.ones((Ci,), np.float32), np.random.default_rng(H).integers(-1, 2, (Ci,))).astype(np.float32)   # exact factors

        def g(dy, w):
            old = backward._CONV_DGRAD_S2
            backward._CONV_DGRAD_S2 = s2
            try:
                dx = backward.conv_input_grad(_d(dy), _d(w), stride, pad, (H, W), gate=_d(g_) if gate else None,
                                              scale=_d(sc) if gate else None)
            finally:
                backward._CONV_DGRAD_S2 = old
            return [_n(dx)]
        base = _dgrad_ref(stride, pad, H, W)
        gm = torch.from_numpy((g_ > 0).astype(np.float64)) * torch.from_numpy(sc.astype(np.float64))
        ref = (lambda dy, w: [base(dy, w)[0] * gm]) if gate else base
        return Family(f"conv_input_grad_{KH}x{KH}s{stride}{'_gate' if gate else ''}{'' if s2 else '_dilated'}",
                      [(N, Ho, Wo, Co), (Co, KH, KH, Ci)], g, ref)

    F["dgrad_s1"] = dgrad(2, 23, 40, 64, 64, 3, 1, 1)
    F["dgrad_s2"] = dgrad(2, 24, 41, 128, 64, 3, 2, 1)
    F["dgrad_s2_gate"] = dgrad(2, 24, 41, 128, 64, 3, 2, 1, gate=True)
    F["dgrad_s2_dilated"] = dgrad(2, 24, 41, 128, 64, 3, 2, 1, s2=False)

    def wgrad(N, H, W, Ci, Co, KH, stride, pad, implicit=True):
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KH) // stride + 1

        def g(dy, x):
            old = backward._CONV_WGRAD_IMPLICIT
            backward._CONV_WGRAD_IMPLICIT = implicit
            try:
                return [_n(backward.conv_weight_grad(_d(dy), _d(x), KH, KH, stride, pad))]
            finally:
                backward._CONV_WGRAD_IMPLICIT = old
        return Family(f"conv_weight_grad_{KH}x{KH}s{stride}{'' if implicit else '_padded'}_{Ci}", [(N, Ho, Wo, Co), (N, H, W, Ci)], g,
                      _wgrad_ref(stride, pad, KH))

    F["wgrad_implicit"] = wgrad(2, 23, 40, 64, 64, 3, 1, 1)
    F["wgrad_implicit_s2"] = wgrad(2, 31, 27, 128, 256, 3, 2, 1)
    F["wgrad_padded"] = wgrad(2, 23, 40, 64, 64, 3, 1, 1, implicit=False)
    F["wgrad_im2col"] = wgrad(2, 37, 53, 4, 64, 7, 2, 3)                 # the stem: Ci * KH * KW <= 256

    def wbias(M, N, K):
        def g(dy, x):
            db = torch.empty((N,), device=DEV)
            dw = backward.weight_grad(_d(dy), _d(x), bias_out=db)
            return [_n(dw), _n(db)]
        # the bias gradient is a plain fp32 column sum of dy: it has to be at least as good as the split
        return Family(f"weight_grad_bias_{M}x{N}x{K}", [(M, N), (M, K)], g, lambda dy, x: [dy.T @ x, dy.sum(0)])

    F["weight_grad_bias"] = wbias(5000, 256, 256)
    F["weight_grad_bias_nt"] = wbias(999, 66, 128)                       # N % 4 != 0: transposed operands + batched NT GEMM
    return F


NOPS = {"linear_backward": 3, "linear_backward_pad": 3}
FAMILIES = ["gemm_nt", "gemm_small", "gemm_static", "gemm_presplit_a", "conv_implicit", "conv_halo", "conv_stem", "linear_backward",
            "linear_backward_pad", "dgrad_s1", "dgrad_s2", "dgrad_s2_gate", "dgrad_s2_dilated", "wgrad_implicit", "wgrad_implicit_s2",
            "wgrad_padded", "wgrad_im2col", "weight_grad_bias", "weight_grad_bias_nt"]
_CACHE = {}


def _fam(name):
    if not _CACHE:
        _CACHE.update(_families())
    return _CACHE[name]


def _operands(fam, seed):
    ops_ = [unit(s, seed + 17 * i) for i, s in enumerate(fam.shapes)]
    if len(fam.shapes[0]) == 4 and fam.shapes[0][3] == 4 and fam.name.startswith("conv"):
        ops_[0][..., 3] = 0                                              # the stem's NHWC4 input: channel 3 is padding
    return ops_


def test_split_rule_window():
    """the window follows from the rule alone (no kernel involved): at every amax inside [2^-14, 65504] the emulated split keeps the
    metric below BOUND for a K = 512 contraction; one binade below 2^-14 it no longer does at some scale, and above 65504 it saturates"""
    g = np.random.default_rng(1)
    B = (g.standard_normal((128, 512)) / np.sqrt(512)).astype(np.float32)
    X = g.standard_normal((256, 512)).astype(np.float32)
    X /= np.abs(X).max()
    mm = lambda A, B_: [A @ B_.T]                                        # noqa: E731
    ref64 = lambda A: A.astype(np.float64) @ B.astype(np.float64).T     # noqa: E731
    den = np.abs(X).astype(np.float64) @ np.abs(B).astype(np.float64).T
    for e in range(-14, 16):
        A = X * np.float32(2.0 ** e)
        assert errs(emulate(mm, [A, B])[0], ref64(A), (den * 2.0 ** e).max()) <= (CORE if e >= -8 else BOUND), e
        Bs = B * np.float32(2.0 ** e / np.abs(B).max())                 # both operands at amax 2^e
        ref = A.astype(np.float64) @ Bs.astype(np.float64).T
        dd = (np.abs(A).astype(np.float64) @ np.abs(Bs).astype(np.float64).T).max()
        assert errs(emulate(mm, [A, Bs])[0], ref, dd) <= (CORE if e >= -8 else BOUND), e
    worst = max(errs(emulate(mm, [X * np.float32(2.0 ** e), B])[0], ref64(X * np.float32(2.0 ** e)), (den * 2.0 ** e).max())
                for e in range(-24, -14))
    assert worst > BOUND
    assert split16(np.float32([70000.0, -1e6]))[0] == 65504.0 + 65504.0 / 2048.0
    assert split16(np.float32([65504.0]))[0] == 65504.0


@pytest.mark.parametrize("name,which", [(n, w) for n in FAMILIES for w in list(range(NOPS.get(n, 2))) + ["all"]])
def test_magnitude_sweep(name, which):
    """power-of-two operand scales 2^-40 .. 2^14, each operand alone, then all together (see the module docstring for the contract)"""
    fam = _fam(name)
    base = _operands(fam, 11)
    worst_inside = 0.0
    for e in SCALES:
        s = np.float32(2.0 ** e)
        ops_ = [a * s if which in ("all", i) else a for i, a in enumerate(base)]
        res = fam.check(ops_)
        if all(in_window(a) for a in ops_):
            worst_inside = max(worst_inside, max(r[0] for r in res))
    assert worst_inside <= BOUND


@pytest.mark.parametrize("name", ["gemm_nt", "gemm_small", "gemm_static", "gemm_presplit_a", "linear_backward"])
def test_mixed_row_magnitudes(name):
    """rows of one operand spanning 2^0 .. 2^-30 inside one tensor: the per-tensor metric, and the per-row metric on the rows whose
    operands lie in the window"""
    fam = _fam(name)
    ops_ = _operands(fam, 12)
    r = fam.rows[0]
    ops_[r] = unit(fam.shapes[r], 99, rows_span=True)
    fam.check(ops_, per_row=True)


@pytest.mark.parametrize("name", FAMILIES)
def test_exact_zeros(name):
    """operands with zero entries, zero rows and an all-zero operand: the bound inside the window, and an exactly zero product"""
    fam = _fam(name)
    ops_ = _operands(fam, 13)
    g = np.random.default_rng(5)
    ops_[0] = np.where(g.random(ops_[0].shape) < 0.5, 0.0, ops_[0]).astype(np.float32)
    ops_[0].reshape(ops_[0].shape[0], -1)[::3] = 0.0
    fam.check(ops_)
    zs = [np.zeros_like(ops_[0])] + ops_[1:]
    outs = fam.gpu(*zs)
    if name.startswith("linear_backward"):
        outs = outs[1:]                                        # an all-zero x leaves dx = dy . w as it is; dw = dy^T . x is zero
    for out in outs:
        assert np.all(out == 0), name


@pytest.mark.parametrize("name", ["gemm_nt", "gemm_small", "gemm_static", "conv_implicit", "linear_backward", "wgrad_implicit"])
def test_fp16_range_edge(name):
    """entries at +-65504 are inside the window (exact h, zero l); entries just above it saturate to 65504 + 65504 / 2048 with no
    error and no non-finite value -- the documented behaviour of the round-toward-zero split (the gradient scale keeps every gradient
    operand <= 2^12 so that it cannot happen in training), pinned here so that a change of it is seen: the kernel's own error must match
    the saturating rule's from below as well as from above"""
    fam = _fam(name)
    ops_ = _operands(fam, 14)
    a = ops_[0] * np.float32(2.0 ** 12)
    flat = a.reshape(-1)
    idx = np.random.default_rng(3).choice(flat.size, 64, replace=False)
    flat[idx[:32]] = np.float32(65504.0) * np.sign(flat[idx[:32]] + 0.5)
    fam.check([a] + ops_[1:])
    flat[idx[32:]] = np.float32(70000.0) * np.sign(flat[idx[32:]] + 0.5)
    assert not in_window(a)
    res = fam.check([a] + ops_[1:])
    # check() bounds the kernel's error from above by the rule's; the rule loses about 4.5e3 per saturated entry, and so must the kernel
    assert max(r[1] for r in res) > 10 * BOUND
    for err, eerr in res:
        assert err >= eerr / FACTOR - BOUND, (name, err, eerr)


# ------------------------------------------------------------------------------------------------ attention
def _attn_case(B, Q, K, seed):
    g = torch.Generator().manual_seed(seed)
    C = 256
    q, k, v, dout = (torch.randn(s, generator=g) for s in ((B, Q, C), (B, K, C), (B, K, C), (B, Q, C)))
    return q, k, v, dout


def _attn_ref(q, k, v, dout, H=8):
    B, Q, C = q.shape
    K = k.shape[1]
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    sc = torch.einsum("bqhd,bkhd->bhqk", qd.view(B, Q, H, 32), kd.view(B, K, H, 32)) / 32 ** 0.5
    pr = torch.softmax(sc, -1)
    out = torch.einsum("bhqk,bkhd->bqhd", pr, vd.view(B, K, H, 32)).reshape(B, Q, C)
    (out * dout.double()).sum().backward()
    dp = torch.einsum("bqhd,bkhd->bhqk", dout.double().view(B, Q, H, 32), v.double().view(B, K, H, 32))
    ds = pr * (dp - (dp * pr).sum(-1, keepdim=True))
    return out.detach(), qd.grad, kd.grad, vd.grad, pr.detach(), float(ds.detach().abs().max())


@pytest.mark.parametrize("B,Q,K", [(2, 100, 1500), (1, 37, 333)])
def test_masked_attention_value_and_gradient_scales(B, Q, K):
    """masked_attn splits v (the output is linear in v) and its backward splits dout (dq, dk, dv are linear in dout): both swept over
    2^-40 .. 2^14.  Metric: max error / max(|P| . |V|) for the output, / max(|P|^T . |dout|) for dv, / max|ref| for dq and dk.
    Inside the window the attention family's own fp32 bound (exp2 of the scores, softmax normalisation) holds at every scale.  Outside
    it the kernel also splits the recomputed probabilities and dS, which the test does not restate: only finiteness is asserted there,
    and the model-level tests below keep the decoder's attention gradients inside the window.  The backward's window takes its inner
    operand dS = P (dP - D) too (the dq / dk contractions split it)."""
    from s2d_amd import backward, ops
    ATTN = 2e-5            # tests/test_gpu_backward.py's bound at unit scale: the scale must not change it
    q, k, v, dout = _attn_case(B, Q, K, B * 1000 + Q + K)
    o_ref, dq_ref, dk_ref, dv_ref, pr, ds_max = _attn_ref(q, k, v, dout)
    H = 8
    pv_den = torch.einsum("bhqk,bkhd->bqhd", pr, v.double().abs().view(B, K, H, 32)).abs().max()
    for e in SCALES:
        s = 2.0 ** e
        vs = (v * s).float()
        o, lse = ops.masked_attn(q.to(DEV), k.to(DEV), vs.to(DEV), want_lse=True)
        assert bool(torch.isfinite(o).all())
        err = float((o.double().cpu() / s - o_ref).abs().max() / pv_den)
        if WIN_LO <= float(vs.abs().max()) <= WIN_HI:
            assert err <= ATTN, ("out", e, err)
        o1, lse1 = ops.masked_attn(q.to(DEV), k.to(DEV), v.to(DEV), want_lse=True)
        ds = (dout * s).float()
        dq, dk, dv = backward.masked_attn_backward(q.to(DEV), k.to(DEV), v.to(DEV), o1, lse1, ds.to(DEV))
        for nm, got, ref in (("dq", dq, dq_ref), ("dk", dk, dk_ref), ("dv", dv, dv_ref)):
            assert bool(torch.isfinite(got).all()), (nm, e)
            err = float((got.double().cpu() / s - ref).abs().max()) / float(ref.abs().max())
            if WIN_LO <= float(ds.abs().max()) <= WIN_HI and ds_max * s >= WIN_LO:
                assert err <= ATTN, (nm, e, err)


# ------------------------------------------------------------------------------------------------ fused FFN
@pytest.mark.parametrize("M", [4096, 333])
def test_ffn_fused_residual_against_exact_fp32_input(M):
    """ffn_fused (no LayerNorm, p = 0, zero biases: y = x + W2 relu(W1 x) is positively homogeneous in x) against x + FFN(x) in
    float64 from the exact fp32 x, at power-of-two scales of x from 2^14 down to the fp16 subnormal end (2^-24).  The residual path
    (S2D_FFN_EPI=1 rebuilds x as hi + lo / 2048 from the resident fp16 fragments) is held to 5e-7 of max|x| per row inside the window;
    below it the residual carries split16(x), not x, and the error stays within FACTOR of that rule's.  W2 is small, so that the
    branch's own contraction error stays far below the residual's."""
    from s2d_amd import ops
    g = np.random.default_rng(M)
    F = 1024
    W1 = (g.standard_normal((F, 256)) * 0.06).astype(np.float32)
    W2 = (g.standard_normal((256, F)) * 0.003).astype(np.float32)
    z1, z2 = torch.zeros((F,), device=DEV), torch.zeros((256,), device=DEV)
    W1d, W2d = ops.mark_static(_d(W1)), ops.mark_static(_d(W2))
    x0 = unit((M, 256), M)
    W1_64, W2_64 = W1.astype(np.float64), W2.astype(np.float64)
    for e in [14, 8, 0, -8, -12, -14, -17, -20, -24]:
        x = x0 * np.float32(2.0 ** e)
        y = _n(ops.ffn_fused(_d(x), W1d, z1, W2d, z2))
        x64 = x.astype(np.float64)
        hid = np.maximum(x64 @ W1_64.T, 0)
        ref = x64 + hid @ W2_64.T
        # the rule: residual = h + l * 2^-11 of x; hidden = split product of x and W1, ReLU, then split again for W2
        xs = split16(x)
        hs = np.maximum(emulate(lambda a, b: [a @ b.T], [x, W1])[0], 0).astype(np.float32)
        emu = xs + emulate(lambda a, b: [a @ b.T], [hs, W2])[0]
        amx = np.abs(x64).max(1)
        err, eerr = np.abs(y - ref).max(1) / amx, np.abs(emu - ref).max(1) / amx
        assert np.isfinite(y).all(), e
        # inside the window: every row's amax >= 2^-13 (its entries down to 2^-14 of it keep their bits to ~2^-21 of the row's amax) and the
        # hidden activation below 65504
        if float(amx.min()) >= 2.0 ** -13 and float(hid.max()) < WIN_HI:
            assert float(err.max()) <= 5e-7, (e, float(err.max()))
        assert np.all(err <= FACTOR * eerr + 5e-7), (e, float(err.max()), float(eerr.max()))


# ------------------------------------------------------------------------------------------------ the whole model's gradients
def _census_module():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "split_operand_census.py")
    spec = importlib.util.spec_from_file_location("split_operand_census", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TINY = {}


def _tiny_kd():
    """the KD parity case of test_whole_model_gradient_directional_derivative: injected sample points and assignment"""
    if _TINY:
        return _TINY
    from s2d_amd import ops
    from s2d_amd.modeling import TargetSet, build_kd_model
    from tests.parity import make_case, make_coords, seeded_load
    seed, B, T, H0, W0, Q, P, ns, NL = 5, 2, 2, 60, 90, 16, 256, (3, 4), 4
    model = build_kd_model(num_queries=Q, num_frames=T, num_points=P, weights=(2.0, 5.0, 5.0), dec_layers=NL)
    seeded_load(model.student, seed); seeded_load(model.teacher, seed + 1)
    model = model.to(DEV)
    model.criterion.importance_sample_ratio = 0.0
    frames, tg = make_case(seed, B, T, H0, W0, Q, P, ns)
    images = ops.normalize_pad(torch.from_numpy(frames).to(DEV))
    Hp, Wp = images.shape[1:3]
    gts = []
    for m, ids in tg:
        pad = np.zeros((m.shape[0], T, Hp, Wp), np.uint8)
        pad[:, :, :H0, :W0] = m
        gts.append(torch.from_numpy(pad[(ids != -1).any(-1)]))
    Ngt = max(max(g_.shape[0] for g_ in gts), 1)
    to = lambda c: {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}      # noqa: E731
    cg, ck = to(make_coords(seed + 10, NL, B, Q, Ngt, T, P)), to(make_coords(seed + 11, NL, B, Q, Q, T, P))
    gen = torch.Generator(device=DEV).manual_seed(7)
    for c in (cg, ck):
        c["rand"] = torch.rand((NL, c["rand"].shape[1], P, 2), device=DEV, generator=gen)
    gt = TargetSet.from_list(gts, device=DEV)
    # the assignment of both criteria held at that of a first pass, as the directional-derivative test does
    model.forward_backward(images, gt, cg, ck, kd_nmax=Q)
    st, te = model.last["student"], model.last["teacher"]
    model.criterion(st, gt, False, cg); cg["indices"] = model.criterion.last_indices
    kdt = ops.kd_targets(te.class_logits[-1], te.mask_logits[-1], te.dims, Hp, Wp, Q, 0.75, 100)
    model.criterion(st, TargetSet(kdt[0], kdt[1], kdt[3]), True, ck); ck["indices"] = model.criterion.last_indices
    params = [p for p in model.student.parameters() if p.requires_grad]
    _TINY.update(model=model, images=images, gt=gt, cg=cg, ck=ck, Q=Q, params=params)
    return _TINY


def _grads(loss_scale, calls=1, census=None):
    """.grad of every student parameter after `calls` forward_backward calls at loss_scale, from no gradient (float64 copies)"""
    c = _tiny_kd()
    for p in c["params"]:
        p.grad = None
    for _ in range(calls):
        if census is not None:
            with census:
                c["model"].forward_backward(c["images"], c["gt"], c["cg"], c["ck"], kd_nmax=c["Q"], loss_scale=loss_scale)
        else:
            c["model"].forward_backward(c["images"], c["gt"], c["cg"], c["ck"], kd_nmax=c["Q"], loss_scale=loss_scale)
    return [p.grad.detach().double().clone() for p in c["params"]]


def _normwise(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def test_split_operands_stay_in_window_during_forward_backward():
    """every tensor handed to a split-fp16 export during forward_backward has amax <= 2^12 and >= 2^-14 (or is all zeros), at every
    loss_scale of the scale-invariance sweep"""
    cen = _census_module()
    for m in (-2, 0, 3, 8):
        c = cen.Census()
        _grads(2.0 ** -m, census=c)
        recs = c.records()
        assert sum(r["phase"] == "backward" for r in recs) > 100
        bad = cen.outside_window(recs)
        assert not bad, (m, len(bad), sorted({(r["phase"], r["export"], r["arg"], r["amax"]) for r in bad}, key=lambda r: r[3])[:12])


def test_gradients_invariant_under_power_of_two_loss_scale():
    """forward_backward at loss_scale 2^-m, times 2^m, equals the m = 0 gradients (normwise per parameter tensor <= 1e-5): exact in fp32
    apart from underflow, so any difference is bits the split-fp16 arithmetic lost to the operands' magnitude"""
    g0 = _grads(1.0)
    worst = {}
    for m in (-2, 3, 8):
        gm = _grads(2.0 ** -m)
        worst[m] = max(_normwise(a * 2.0 ** m, b) for a, b in zip(gm, g0))
    assert all(v <= 1e-5 for v in worst.values()), worst


def test_gradient_accumulation_over_two_half_scaled_calls():
    """two calls with loss_scale 1/2 accumulate to the gradients of one call with loss_scale 1 (ACCUM_ITER = 2), and the root scale is
    undone exactly: the accumulated gradients are those of one call"""
    g1 = _grads(1.0)
    g2 = _grads(0.5, calls=2)
    worst = max(_normwise(a, b) for a, b in zip(g2, g1))
    assert worst <= 1e-5, worst


def test_gradient_scale_is_undone_where_the_gradients_land():
    """the root scale S never reaches .grad: the gradients with the scale at 2^8 (the default) and at 2^0 (the unscaled backward of
    the parent arithmetic) agree to the split's accuracy: a wrong or missing 1 / S would be off by powers of two (a missing scale of the
    existing gradient before accumulation fails test_gradient_accumulation_over_two_half_scaled_calls)"""
    from s2d_amd import backward
    k0 = backward.GRAD_SCALE_LOG2
    try:
        backward.GRAD_SCALE_LOG2 = 0
        g_unscaled = _grads(1.0)
    finally:
        backward.GRAD_SCALE_LOG2 = k0
    g = _grads(1.0)
    worst = max(_normwise(a, b) for a, b in zip(g, g_unscaled))
    assert worst <= 1e-4, worst
