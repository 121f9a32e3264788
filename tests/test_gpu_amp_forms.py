"""The AMP dense kernels (s2d_amd/csrc/gemm_amp.hip: s2d_gemm_nt_amp_f32, s2d_conv2d_nhwc_amp_f32), form by form, against the exact
references of tests/amp_refs.py (numpy float64 / int64, pinned on the CPU by tests/test_amp_refs_cpu.py).  The vocabulary is that of
tests/test_gpu_forward_c4.py / test_gpu_backward_c4.py (recording, signature functions, _Rep, _row_id, a TABLE and a test that it is
complete), imported from there.

A *form* is what selects a branch of gemm_amp.hip, without sizes (amp_refs.gemm_form / conv_form).  TABLE holds every form at the smallest
sizes at which the 128 x 128 x 64 tile can still go wrong (amp_refs.GEMM_ROWS / CONV_ROWS); test_table_covers_the_amp_forward records the
calls that reach the two exports during a no-grad forward of the small model with AMP compute on, class-agnostic and with 40 classes, and
fails when one has a form without a row.

Every row makes three comparisons:
  a. integer operands in [-8, 8], integer bias and residual, scale a power of two in {0.5, 1, 2}: everything is exact in fp16 and f32 and
     every partial sum in any order is an integer below 2^24, so the result must EQUAL the int64 / float64 evaluation bit for bit;
  b. seeded float32 operands of unit scale against float64 on the fp16-rounded operands; error = max |y - ref| / (1 + |ref|) (what the
     rtol = atol of test_gpu_e2e.py::test_amp_gemm_kernel_vs_fp16_rounded_reference bounds), bound = max(2e-5 -- that test's figure --,
     2 x the error of torch's own float32 matmul / conv2d on the same rounded operands): never read off the kernel;
  c. a second call, bitwise equal to the first.
Then the conversion itself, bit for bit: against a one-hot other operand holding a power of two C[m, n] is fp16(A[m, k_n]) 2^s with no
accumulation, at rounding ties, the largest finite values, overflow, zeros, the fp16 subnormal range and NaN; both operands, both
exports.  test_fp16_subnormal_operands pins what the MFMA does with subnormal operands (amp_refs.FLUSH_SUBNORMAL_OPERANDS).
The figures of one run (the `amprow` lines) are in profiles/amp_parity.txt."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

from tests import amp_refs as R
from tests.test_gpu_backward_c4 import DEV, _Rep, _row_id
from tests.test_gpu_forward_c4 import recording

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5                       # what the columns of `out` behind N hold before a launch, and must hold after it


# --------------------------------------------------------------------------- form signatures of the two exports (arguments of lib().call)
def _sig_s2d_gemm_nt_amp_f32(A, B, C, M, N, K, lda, ldb, ldc, batch, sA, sB, sC, scale, bias, res, ldr, sR, res_rows, res_cols, relu, stream):
    kind = R.residual_kind(res is not None, sR != 0 and batch > 1, res_rows, res_cols, N)
    return R.gemm_form(batch, sB != 0, M, N, ldc, scale is not None, bias is not None, relu, kind) + ((batch, M, N, K),)


def _sig_s2d_conv2d_nhwc_amp_f32(x, w, y, N, H, W, Cin, Cout, KH, KW, stride, pad, scale, bias, res, relu, stream):
    assert KH == KW
    return R.conv_form(Cin, Cout, KH, stride, pad, scale is not None, bias is not None, relu, res is not None) + ((N, H, W, Cin, Cout),)


AMP_EXPORTS = {"s2d_gemm_nt_amp_f32": _sig_s2d_gemm_nt_amp_f32, "s2d_conv2d_nhwc_amp_f32": _sig_s2d_conv2d_nhwc_amp_f32}


@contextlib.contextmanager
def _amp_calls(log):
    """every call that reaches an AMP export, as (form..., sizes), whichever entry point of ops made it"""
    from s2d_amd import ops
    with recording(ops, log, entry_points={}, lib_calls=AMP_EXPORTS):
        yield log


# form + sizes: one row per entry of amp_refs.GEMM_ROWS / CONV_ROWS
TABLE = [R.gemm_row_form(r) + (r,) for r in R.GEMM_ROWS] + [R.conv_row_form(r) + (r,) for r in R.CONV_ROWS]
FORMS = {row[:-1] for row in TABLE}


def test_table_covers_the_amp_forward():
    """every form the model makes under AMP compute has a row: a dispatch change that brings a new branch of gemm_amp.hip into the forward
    fails here until the row (and with it the three comparisons) is added.  Recorded: the whole no-grad forward_losses of the small
    class-agnostic KD model (student and teacher: N = 2 class heads), then the student's forward with a 40-class head (N = 41)"""
    from s2d_amd.modeling import set_amp_compute
    from tests.parity import run_case
    log = []
    with _amp_calls(log):
        hip, _ = run_case(None, seed=3, B=2, T=2, H0=60, W0=90, Q=16, P=256, ns=(3, 4), amp=True)
    n_agnostic = len(log)
    model, images = hip["model"], hip["inputs"][0]
    torch.manual_seed(0)
    model.student[1].predictor.class_embed = torch.nn.Linear(256, 41).to(images.device)          # SEM_SEG_HEAD.NUM_CLASSES = 40
    set_amp_compute(model, True)
    with _amp_calls(log), torch.no_grad():
        out = model.student(images, True)
        torch.cuda.synchronize()
    assert out.class_logits.shape[-1] == 41 and bool(torch.isfinite(out.class_logits).all())
    assert n_agnostic > 100 and len(log) > n_agnostic + 50, "the recorder saw no AMP launches: the hook is dead"
    names = {c[0] for c in log}
    assert names == {"s2d_gemm_nt_amp_f32", "s2d_conv2d_nhwc_amp_f32"}, names
    gemm_sizes = {c[-1] for c in log if c[0] == "s2d_gemm_nt_amp_f32"}
    assert {2, 41} <= {s[2] for s in gemm_sizes}, "both class heads must reach the scalar epilogue"
    seen = {c[1:-1] for c in log}
    for f in sorted(seen, key=repr):
        print("ampform", _row_id(f), "x", sum(1 for c in log if c[1:-1] == f), "e.g.", next(c[-1] for c in log if c[1:-1] == f))
    for f in sorted(FORMS - seen, key=repr):
        print("ampform not made by the model (kept: a branch of the kernel):", _row_id(f))
    missing = sorted(seen - FORMS, key=repr)
    assert not missing, missing
    # the forms the issue names as untested before this module
    assert any(f[0] == "gemm_nt" and not f[3] for f in seen)                                       # scalar epilogue
    assert any(f[0] == "gemm_nt" and f[1] and f[2] for f in seen)                                  # batched, B per batch
    assert any(f[0] == "gemm_nt" and f[8] == "full" and f[5] and f[7] for f in seen)               # conv3: scale, residual, ReLU


# --------------------------------------------------------------------------- comparison
class _AmpRep(_Rep):
    """_Rep with the figures of this module: `amprow` lines, the elementwise rtol = atol error, exact comparisons"""

    def cmp(self, name, got, r64, r32, small):
        err, e32 = R.elementwise_error(got, r64), R.elementwise_error(r32, r64)
        bound = max(small, 2.0 * e32)
        print(f"amprow {self.row} {name}: kernel {err:.3e} bound {bound:.3e} f32-torch {e32:.3e}")
        if not err < bound:
            self.bad.append((name, err, bound))

    def exact(self, name, got, want, equal_nan=False):
        """got float32 == want float64, element by element (and bit for bit where the value is not a zero)"""
        want32 = np.asarray(want, np.float64).astype(np.float32)
        ok = got.shape == want32.shape and np.array_equal(want32.astype(np.float64), want, equal_nan=True) and np.array_equal(got, want32, equal_nan=equal_nan)
        n_bad = -1 if got.shape != want32.shape else int((~((got == want32) | (np.isnan(got) & np.isnan(want32) & equal_nan))).sum())
        print(f"amprow {self.row} {name}: {'equal' if ok else 'DIFFERS'} ({n_bad} of {got.size} elements differ)")
        if not ok:
            self.bad.append((name, n_bad))

    def same(self, name, a, b):
        ok = np.array_equal(a.view(np.int32), b.view(np.int32))
        print(f"amprow {self.row} {name}: {'bitwise equal' if ok else 'DIFFERS'}")
        if not ok:
            self.bad.append((name, "not bitwise equal"))

    def check(self, name, ok):
        print(f"amprow {self.row} {name}: {'ok' if ok else 'FAILS'}")
        if not ok:
            self.bad.append((name,))


def _rng(row, salt):
    return np.random.default_rng(zlib.crc32(repr((row, salt)).encode()))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _t32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _draw(rng, integer):
    if integer:
        return lambda *s: rng.integers(-8, 9, s).astype(np.float32)
    return lambda *s: rng.standard_normal(s).astype(np.float32)


def _scale(rng, n, integer):
    return rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n) if integer else (rng.random(n) + 0.5).astype(np.float32)


# --------------------------------------------------------------------------- GEMM rows
def _gemm_operands(row, integer):
    bs, bb, M, N, K, extra, has_s, has_b, relu, res = row
    rng = _rng(row, integer)
    draw = _draw(rng, integer)
    lead = (bs,) if bs > 1 else ()
    A, B = draw(*lead, M, K), draw(*(lead if bb else ()), N, K)
    sc = _scale(rng, N, integer) if has_s else None
    bi = draw(N) if has_b else None
    r, rr, rc = None, 0, 0
    if res == "full":
        r = draw(M, N)
    elif res == "batched":
        r = draw(bs, M, N)
    elif res is not None and res[0] == "periodic":
        rr = res[1]
        r = draw(rr, N)
    elif res is not None:
        rc, ldr = res[1], res[2]
        r = draw(M, ldr)
    return A, B, sc, bi, r, rr, rc


def _launch_gemm(rep, row, A, B, sc, bi, r, rr, rc):
    """the row through ops.gemm_nt inside amp_fp16 -> float32 [.., M, N] on the host; checks that the launch reached the AMP export in the
    row's form and that the pad columns of `out` survive"""
    from s2d_amd import ops
    bs, bb, M, N, K, extra, has_s, has_b, relu, res = row
    out = None
    if extra:
        out = torch.full(((bs,) if bs > 1 else ()) + (M, N + extra), SENTINEL, device=DEV)
    log = []
    with _amp_calls(log), ops.amp_fp16(True):
        y = ops.gemm_nt(_dev(A), _dev(B), scale=_dev(sc), bias=_dev(bi), res=_dev(r), relu=relu, out=out, res_rows=rr, res_cols=rc)
    torch.cuda.synchronize()
    if not (len(log) == 1 and log[0][1:-1] == R.gemm_row_form(row) and log[0][-1] == (bs, M, N, K)):
        rep.bad.append(("launch is not the row's form", log))
    if out is not None:
        rep.check("columns behind N untouched", bool((out[..., N:] == SENTINEL).all()))
    return y[..., :N].cpu().numpy()


def _f32_gemm(A, B, sc, bi, r, relu, rr, rc):
    """the restatement in float32 through torch (CPU), on the operands as given"""
    v = _t32(A) @ _t32(B).transpose(-1, -2)
    M, N = v.shape[-2:]
    if sc is not None:
        v = v * _t32(sc)
    if bi is not None:
        v = v + _t32(bi)
    if r is not None:
        t = _t32(r)
        if rr:
            t = t[torch.arange(M) % rr]
        c = rc or N
        v = torch.cat([v[..., :c] + t[..., :c], v[..., c:]], -1)
    return (torch.relu(v) if relu else v).numpy()


def _gemm_id(row):
    return _row_id(R.gemm_row_form(row)[1:] + row[:5])


@pytest.mark.parametrize("row", R.GEMM_ROWS, ids=_gemm_id)
def test_amp_gemm_form(row):
    bs, bb, M, N, K, extra, has_s, has_b, relu, res = row
    rep = _AmpRep(("gemm_nt",) + R.gemm_row_form(row)[1:] + row[:5])
    # a. integers: exact
    A, B, sc, bi, r, rr, rc = _gemm_operands(row, True)
    assert float((np.abs(A).astype(np.float64) @ np.swapaxes(np.abs(B).astype(np.float64), -1, -2)).max()) * 2 + 16 < 2 ** 24
    y = _launch_gemm(rep, row, A, B, sc, bi, r, rr, rc)
    want = R.ref_gemm_nt(A.astype(np.int64), B.astype(np.int64), sc, bi, r, relu, rr, rc)
    rep.exact("integer operands", y, want)
    rep.same("integer operands, bit patterns", y, want.astype(np.float32))
    # b. float32 operands of unit scale: float64 on the fp16-rounded operands
    A, B, sc, bi, r, rr, rc = _gemm_operands(row, False)
    y = _launch_gemm(rep, row, A, B, sc, bi, r, rr, rc)
    A16, B16 = R.round_fp16(A), R.round_fp16(B)
    r64 = R.ref_gemm_nt(A16, B16, sc, bi, r, relu, rr, rc)
    r32 = _f32_gemm(A16, B16, sc, bi, r, relu, rr, rc)
    rep.cmp("float operands", y, r64, r32, 2e-5)
    # c. a second call
    rep.same("second call", _launch_gemm(rep, row, A, B, sc, bi, r, rr, rc), y)
    rep.done()


# --------------------------------------------------------------------------- convolution rows
def _conv_operands(row, integer):
    N, H, W, Ci, Co, k, stride, pad, has_s, has_b, relu, has_r = row
    rng = _rng(row, integer)
    draw = _draw(rng, integer)
    Ho, Wo = R.conv_out_hw(H, W, k, stride, pad)
    x, w = draw(N, H, W, Ci), draw(Co, k, k, Ci)
    return x, w, (_scale(rng, Co, integer) if has_s else None), (draw(Co) if has_b else None), (draw(N, Ho, Wo, Co) if has_r else None)


def _launch_conv(rep, row, x, w, sc, bi, r):
    from s2d_amd import ops
    N, H, W, Ci, Co, k, stride, pad, has_s, has_b, relu, has_r = row
    log = []
    with _amp_calls(log), ops.amp_fp16(True):
        y = ops.conv2d_nhwc(_dev(x), _dev(w), stride, pad, _dev(sc), _dev(bi), _dev(r), relu)
    torch.cuda.synchronize()
    if not (len(log) == 1 and log[0][1:-1] == R.conv_row_form(row)):
        rep.bad.append(("launch is not the row's form", log))
    return y.cpu().numpy()


def _f32_conv(x, w, stride, pad, sc, bi, r, relu):
    v = torch.nn.functional.conv2d(_t32(x).permute(0, 3, 1, 2), _t32(w).permute(0, 3, 1, 2), None, stride, pad).permute(0, 2, 3, 1)
    if sc is not None:
        v = v * _t32(sc)
    if bi is not None:
        v = v + _t32(bi)
    if r is not None:
        v = v + _t32(r)
    return (torch.relu(v) if relu else v).numpy()


def _conv_id(row):
    return _row_id(R.conv_row_form(row)[1:] + row[:5])


@pytest.mark.parametrize("row", R.CONV_ROWS, ids=_conv_id)
def test_amp_conv_form(row):
    N, H, W, Ci, Co, k, stride, pad, has_s, has_b, relu, has_r = row
    rep = _AmpRep(("conv2d_nhwc",) + R.conv_row_form(row)[1:] + row[:5])
    x, w, sc, bi, r = _conv_operands(row, True)
    assert 64 * k * k * Ci * 2 + 16 < 2 ** 24                              # |x| . |w| <= 8 * 8 * K
    y = _launch_conv(rep, row, x, w, sc, bi, r)
    want = R.ref_conv2d_nhwc(x, w, stride, pad, sc, bi, r, relu)
    rep.exact("integer operands", y, want)
    rep.same("integer operands, bit patterns", y, want.astype(np.float32))
    x, w, sc, bi, r = _conv_operands(row, False)
    y = _launch_conv(rep, row, x, w, sc, bi, r)
    x16, w16 = R.round_fp16(x), R.round_fp16(w)
    rep.cmp("float operands", y, R.ref_conv2d_nhwc(x16, w16, stride, pad, sc, bi, r, relu), _f32_conv(x16, w16, stride, pad, sc, bi, r, relu), 2e-5)
    rep.same("second call", _launch_conv(rep, row, x, w, sc, bi, r), y)
    rep.done()


# --------------------------------------------------------------------------- the conversion, bit for bit
K1 = 68                                    # two k-tiles; the second holds one live 16-B piece; all four slots of a lane's 16 B are visited


def _finite_specials():
    return np.concatenate([R.tie_values(), R.edge_values(), R.subnormal_values()])


def _special_matrix(K):
    """[rows, K] float32: the finite special values, each at every k, then rows of their own for the values whose fp16 image is inf or
    NaN -- one such value per row, at k = 0, 3, 63, 64, K - 1 -> (matrix, number of finite rows)"""
    fin = R.latin_rows(_finite_specials(), K)
    bad = []
    for i, v in enumerate(R.nonfinite_values()):
        for k in (0, 3, 63, 64, K - 1):
            row = fin[(7 * i + k) % len(fin)].copy()
            row[k] = v
            bad.append(row)
    return np.concatenate([fin, np.array(bad, np.float32)]), len(fin)


def _conversion_checks(rep, name, got, S, nfin, factors):
    """got [rows of S, K]: must be fp16(S) * factor of the column, exactly; rows >= nfin hold an inf or a NaN"""
    S16 = R.round_fp16(S)
    assert np.isfinite(S16[:nfin]).all() and not np.isfinite(S16[nfin:]).all(axis=1).any()
    rep.exact(name + ", finite rows == fp16(operand) * 2^s", got[:nfin], S16[:nfin] * factors)
    # an inf meets the zeros of the one-hot operand: the row is inf and NaN by the definition itself
    want = R.ref_gemm_nt(S16[nfin:], np.diag(factors.astype(np.float64)))
    assert np.isnan(want).any() and np.isinf(want).any()
    rep.exact(name + ", rows holding inf / NaN", got[nfin:], want, equal_nan=True)


def test_gemm_operand_conversion_bit_for_bit():
    from s2d_amd import ops
    rep = _AmpRep(("convert", "gemm_nt", K1))
    S, nfin = _special_matrix(K1)
    H, f = R.one_hot_operand(K1)
    with ops.amp_fp16(True):
        cA = ops.gemm_nt(_dev(S), _dev(H)).cpu().numpy()                  # A special, B one-hot: C[m, n] = fp16(A[m, n]) f[n]
        cB = ops.gemm_nt(_dev(H), _dev(S)).cpu().numpy()                  # the roles swapped:    C[m, n] = fp16(B[n, m]) f[m]
    print(f"amprow {rep.row}: {nfin} finite rows ({len(_finite_specials())} values x every k), {len(S) - nfin} rows with inf / NaN")
    _conversion_checks(rep, "A", cA, S, nfin, f)
    _conversion_checks(rep, "B", np.ascontiguousarray(cB.T), S, nfin, f)
    rep.done()


def test_conv_operand_conversion_bit_for_bit():
    """the same through the implicit-GEMM convolution, 3 x 3 x 8 taps (K = 72): a weight that is one-hot in (kh, kw, ci) reads the input's
    conversion, an input that is one-hot in its single 3 x 3 window reads the weight's"""
    from s2d_amd import ops
    rep = _AmpRep(("convert", "conv2d_nhwc", 72))
    K, Ci = 72, 8
    H1, f = R.one_hot_operand(K)
    S, nfin = _special_matrix(K)
    with ops.amp_fp16(True):
        # weight special [rows, 3, 3, 8], input [72, 3, 3, 8] one-hot at flat position n: y[n, 0, 0, co] = fp16(w[co, n]) f[n]
        cW = ops.conv2d_nhwc(_dev(H1.reshape(K, 3, 3, Ci)), _dev(S.reshape(-1, 3, 3, Ci)), 1, 0).cpu().numpy().reshape(K, len(S))
    _conversion_checks(rep, "weight", np.ascontiguousarray(cW.T), S, nfin, f)
    # input special: image 0 holds the finite values, image 1 the same with the inf / NaN values scattered; weight one-hot [72, 3, 3, 8]:
    # y[n, oy, ox, co = (kh, kw, ci)] = fp16(x[n, oy + kh, ox + kw, ci]) f[co]
    vals = _finite_specials()
    x = np.resize(vals, (2, 10, 10, Ci)).astype(np.float32)
    bad = R.nonfinite_values()
    for i, v in enumerate(bad):
        x[1, (3 * i + 1) % 10, (7 * i + 2) % 10, (5 * i) % Ci] = v
    with ops.amp_fp16(True):
        cX = ops.conv2d_nhwc(_dev(x), _dev(H1.reshape(K, 3, 3, Ci)), 1, 0).cpu().numpy()
    x16 = R.round_fp16(x)
    want = R.ref_conv2d_nhwc(x16, H1.reshape(K, 3, 3, Ci), 1, 0)
    direct = np.stack([x16[:, kh:kh + 8, kw:kw + 8, ci] * f[(kh * 3 + kw) * Ci + ci] for kh in range(3) for kw in range(3) for ci in range(Ci)], -1)
    assert np.array_equal(want[0], direct[0]) and np.isfinite(want[0]).all() and np.isnan(want[1]).any() and np.isinf(want[1]).any()
    rep.exact("input, finite image == fp16(operand) * 2^s", cX[0], want[0])
    rep.exact("input, image holding inf / NaN", cX[1], want[1], equal_nan=True)
    rep.done()


def test_fp16_subnormal_operands():
    """what v_mfma_f32_32x32x16_f16 does with an operand whose fp16 image is subnormal: it contributes its exact value or exactly nothing,
    never anything in between, the same for both operands, and which of the two is what gemm_amp.hip's header, oracle_np._r16 and
    amp_refs.FLUSH_SUBNORMAL_OPERANDS say"""
    from oracle import oracle_np
    from s2d_amd import ops
    rep = _AmpRep(("subnormal", "gemm_nt", K1))
    S = R.latin_rows(R.subnormal_values(), K1)
    H, f = R.one_hot_operand(K1)
    with ops.amp_fp16(True):
        cA = ops.gemm_nt(_dev(S), _dev(H)).cpu().numpy().astype(np.float64)
        cB = ops.gemm_nt(_dev(H), _dev(S)).cpu().numpy().astype(np.float64).T
    exact = R.round_fp16(S, flush=False)
    sub = (np.abs(exact) > 0) & (np.abs(exact) < R.F16_MIN_NORMAL)
    assert sub.sum() > 500
    for name, got in (("A", cA), ("B", cB)):
        kept, gone = got == exact * f, got == 0
        n_kept, n_gone = int((kept & sub).sum()), int((gone & sub).sum())
        print(f"amprow {rep.row} operand {name}: of {int(sub.sum())} products with a subnormal fp16 operand {n_kept} hold its exact value, {n_gone} are 0; "
              f"{int((kept & ~sub).sum())} of {int((~sub).sum())} other elements exact")
        rep.check(f"operand {name}: every subnormal contributes its exact value or nothing", bool(((kept | gone) | ~sub).all()))
        rep.check(f"operand {name}: one rule for all of them", n_kept == int(sub.sum()) or n_gone == int(sub.sum()))
        rep.check(f"operand {name}: the rule is the documented one (flush = {R.FLUSH_SUBNORMAL_OPERANDS})", (n_gone if R.FLUSH_SUBNORMAL_OPERANDS else n_kept) == int(sub.sum()))
        rep.check(f"operand {name}: zeros, rounded-to-zero and normal results exact", bool((kept | sub).all()))
    # the oracle's restatement follows the same rule
    prev, oracle_np._AMP_ON[0] = oracle_np._AMP_ON[0], True
    try:
        rep.check("oracle_np._r16 == amp_refs.round_fp16", np.array_equal(oracle_np._r16(S).astype(np.float64), R.round_fp16(S)))
    finally:
        oracle_np._AMP_ON[0] = prev
    rep.done()


# --------------------------------------------------------------------------- gating
def _refused(name, *args):
    from s2d_amd import ops
    try:
        ops.lib().call(name, *args)
    except RuntimeError as e:
        return f"{name} failed with code -1" in str(e)
    return False


def test_exports_refuse_what_they_cannot_run():
    """S2D_ERR_ARG through lib().call, decided on the host: the output buffer is untouched"""
    C = torch.full((16, 16), SENTINEL, device=DEV)
    A, B, res = torch.ones((16, 16), device=DEV), torch.ones((16, 16), device=DEV), torch.ones((16, 16), device=DEV)

    def gemm(M=8, N=8, K=8, lda=16, ldb=16, ldc=16, res=None, ldr=16, res_rows=0, res_cols=0):
        return _refused("s2d_gemm_nt_amp_f32", A, B, C, M, N, K, lda, ldb, ldc, 1, 0, 0, 0, None, None, res, ldr, 0, res_rows, res_cols, 0, 0)

    def conv(Cin):
        x, w = torch.ones((1, 4, 4, Cin), device=DEV), torch.ones((4, 1, 1, Cin), device=DEV)
        return _refused("s2d_conv2d_nhwc_amp_f32", x, w, C, 1, 4, 4, Cin, 4, 1, 1, 1, 0, None, None, None, 0, 0)

    assert gemm(K=6), "K % 4 != 0"
    assert gemm(lda=18), "lda % 4 != 0"
    assert gemm(ldb=18), "ldb % 4 != 0"
    assert gemm(res=res, res_cols=2), "res_cols % 4 != 0"
    assert gemm(res=res, res_cols=12), "res_cols > N"
    assert conv(3) and conv(6), "Cin % 4 != 0"
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all()), "a refused call launched something"
    # the same calls with legal arguments run
    assert not gemm(res=res, res_cols=4)
    torch.cuda.synchronize()
    assert bool((C[:8, :4] == 9.0).all()) and bool((C[:8, 4:8] == 8.0).all()) and bool((C[:8, 8:] == SENTINEL).all()) and bool((C[8:] == SENTINEL).all())
    assert not conv(4)
    torch.cuda.synchronize()
    assert bool((C.view(-1)[:64] == 4.0).all())


def test_gemm_nt_under_amp_refuses_a_residual_of_two_columns():
    """the one shape ops.gemm_nt takes in fp32-class arithmetic and refuses inside amp_fp16 (its docstring says so): res_cols % 4 != 0"""
    from s2d_amd import ops
    rng = np.random.default_rng(5)
    A, B, r = rng.standard_normal((9, 8)).astype(np.float32), rng.standard_normal((8, 8)).astype(np.float32), rng.standard_normal((9, 4)).astype(np.float32)
    y = ops.gemm_nt(_dev(A), _dev(B), res=_dev(r), res_cols=2).cpu().numpy()
    np.testing.assert_allclose(y, R.ref_gemm_nt(A, B, res=r, res_cols=2), rtol=1e-5, atol=1e-5)
    with ops.amp_fp16(True):
        with pytest.raises(RuntimeError, match="s2d_gemm_nt_amp_f32 failed with code -1"):
            ops.gemm_nt(_dev(A), _dev(B), res=_dev(r), res_cols=2)
        with pytest.raises(RuntimeError, match="s2d_gemm_nt_amp_f32 failed with code -1"):
            ops.gemm_nt(_dev(A[:, :6]), _dev(B[:, :6]))                     # K % 4 != 0: refused in every mode
    with pytest.raises(RuntimeError, match="s2d_gemm_nt_f32 failed with code -1"):
        ops.gemm_nt(_dev(A[:, :6]), _dev(B[:, :6]))
    assert not ops.amp_active()


def test_amp_scope_only_in_the_f16x3_mode_nests_and_unwinds():
    from s2d_amd import ops
    rng = np.random.default_rng(6)
    A, B = _dev(rng.standard_normal((70, 64)).astype(np.float32)), _dev(rng.standard_normal((36, 64)).astype(np.float32))
    assert not ops.amp_active()
    try:
        for mode in ("bf16x3", "f32"):
            ops.set_dense_mode(mode)
            outside = ops.gemm_nt(A, B)
            with ops.amp_fp16(True):
                assert not ops.amp_active()
                log = []
                with _amp_calls(log):
                    inside = ops.gemm_nt(A, B)
                assert not log and torch.equal(inside, outside), mode
    finally:
        ops.set_dense_mode("f16x3")
    outside = ops.gemm_nt(A, B)
    with ops.amp_fp16(True):
        assert ops.amp_active()
        inside = ops.gemm_nt(A, B)
        with ops.amp_fp16(False):
            assert ops.amp_active()                                         # a disabled scope inside an enabled one changes nothing
            with ops.amp_fp16(True):
                assert ops.amp_active() and torch.equal(ops.gemm_nt(A, B), inside)
            assert ops.amp_active()
        assert ops.amp_active()
    assert not ops.amp_active() and not torch.equal(inside, outside)
    with ops.amp_fp16(False):
        assert not ops.amp_active() and torch.equal(ops.gemm_nt(A, B), outside)
    with pytest.raises(ZeroDivisionError):
        with ops.amp_fp16(True):
            with ops.amp_fp16(True):
                1 / 0
    assert not ops.amp_active() and torch.equal(ops.gemm_nt(A, B), outside)


def test_training_iteration_ignores_amp_compute():
    """forward_backward is fp32-class whatever set_amp_compute says (the gradient kernels differentiate the fp32-class forward): the same
    losses and the same gradients, bit for bit, and not one launch reaches an AMP export"""
    from s2d_amd.modeling import TargetSet, set_amp_compute
    from tests.parity import run_case
    hip, _ = run_case(None, seed=3, B=2, T=2, H0=60, W0=90, Q=16, P=256, ns=(3, 4), NL=4)
    model = hip["model"]
    images, gts, cg = hip["inputs"]
    ck = {k: torch.from_numpy(v).to(images.device) for k, v in hip["coords_kd"].items()}
    params = [p for p in model.student.parameters() if p.requires_grad]

    def once(amp):
        set_amp_compute(model, amp)
        for p in params:
            p.grad = None
        log = []
        try:
            with _amp_calls(log):
                out = model.forward_backward(images, TargetSet.from_list(gts, device=images.device), cg, ck, kd_nmax=16)
                torch.cuda.synchronize()
        finally:
            set_amp_compute(model, False)
        return {k: float(v) for k, v in out.items()}, [p.grad.clone() for p in params], len(log)

    l0, g0, n0 = once(False)
    l1, g1, n1 = once(True)
    model.last_tapes = None
    assert n0 == 0 and n1 == 0, (n0, n1)
    assert len(g0) > 100 and l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    # ... while the flag does reach the forward-only path
    log = []
    set_amp_compute(model, True)
    try:
        with _amp_calls(log):
            model.forward_losses(images, TargetSet.from_list(gts, device=images.device), cg, ck, kd_nmax=16)
    finally:
        set_amp_compute(model, False)
    assert len(log) > 100
