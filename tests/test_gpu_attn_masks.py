"""The masked cross-attention kernels of csrc/attn.hip (cross_attn_kernel, attn_merge_kernel, attn_bwd_mfma_kernel, the scalar pair
attn_bwd_kv_kernel / attn_bwd_q_kernel, attn_bwd_merge_kernel) on the inputs the other attention tests never present:

  a. object-shaped masks (tests/attn_refs.object_masks): most (query, 32-key tile), (query, forward split) and (query, backward split)
     pairs wholly masked, so the online softmax carries m = -1e30, l = 0 across tiles, the merges drop partials of weight 0 and the
     backward leaves exact zeros; rows with one free key, one free tile, one masked tile, a whole wave attending by the all-masked rule;
  b. K = 1, one ragged tile, K = 32 k +- 1 against Q = 1, 32, 33, 128;
  c. score magnitudes of a trained decoder: q and k scaled to |s| ~ 21 and ~ 86, a common-mode shift that softmax cancels, and one
     key 14..16 binades above a long flat tail (un-normalised probabilities in the fp16-subnormal range of the split);
  d. (a) and (b) again on the scalar backward (S2D_ATTN_BWD_MFMA=0, read once per process: a child process).

Every numeric comparison: references in float64 and float32 on the device (tests/attn_refs.masked_attn_ref), error = max|kernel - f64|
/ max|f64|, bound = max(2e-5, FACTOR x the float32 restatement's error) with FACTOR = 2 (the rule of test_gpu_backward_c4.py; the
score-scale rows may use _SCORE_SCALE_FACTOR, see there), one `attnrow` line each; a second call of each entry point is bitwise equal;
k and v once contiguous and once as column slices of one [B, K, 3 C] buffer.  The figures of one run: profiles/attn_masks_parity.txt."""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
C, H, D = 256, 8, 32
F64, F32 = torch.float64, torch.float32
FLOOR = 2e-5                   # the attention family's bound at unit scale
# Factor over float32 torch for the score-scale rows (c).  split_f16.h documents ~3 * 2^-22 per product against float32's 2^-24, so the
# scheme is entitled to at most 12 x float32's error.  Measured (profiles/attn_masks_parity.txt): every (c) row is inside factor 2 except dq under
# the common-mode shift, 7.0 x float32 torch.  There the keys share a component ~400 times their spread, sum_k dS = 0 cancels it in dQ = dS . K, and
# what survives is the rounding of the products (22-bit split operands against float32's 24 bits) amplified by that ratio -- the documented
# per-product error, not the fp32 lse (the scalar fp32 backward fed the same lse is measured beside it).  8 covers 7.0, one step of headroom: 9
_SCORE_SCALE_FACTOR = 9.0
assert _SCORE_SCALE_FACTOR <= 12.0


@pytest.fixture(autouse=True)
def _plain_float32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False                      # the float32 restatement is plain float32
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


class _Rep:
    """collects one row's figures: prints every one, asserts at the end"""

    def __init__(self, row):
        self.row, self.bad = row, []

    def cmp(self, name, got, r64, r32, factor=2.0):
        assert got.shape == r64.shape, (name, got.shape, r64.shape)
        top = max(float(r64.abs().max()), 1e-30)
        err = float((got.double() - r64).abs().max()) / top
        e32 = float((r32.double() - r64).abs().max()) / top
        bound = max(FLOOR, factor * e32)
        print(f"attnrow {self.row} {name}: kernel {err:.3e} f32-torch {e32:.3e} bound {bound:.3e}")
        if not err < bound:
            self.bad.append((name, err, bound))

    def below(self, name, value, bound):
        print(f"attnrow {self.row} {name}: {value:.3e} bound {bound:.3e}")
        if not value < bound:
            self.bad.append((name, value, bound))

    def true(self, name, ok):
        print(f"attnrow {self.row} {name}: {'ok' if ok else 'FAILS'}")
        if not ok:
            self.bad.append((name,))

    def done(self):
        assert not self.bad, self.bad


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(shape, device=DEV, generator=g)


def _layouts(k, v):
    yield "contiguous", k.contiguous(), v.contiguous()
    wide = torch.full((k.shape[0], k.shape[1], 3 * C), float("nan"), device=DEV)       # the q columns are nobody's business
    wide[..., C:2 * C], wide[..., 2 * C:] = k, v
    yield "column slices", wide[..., C:2 * C], wide[..., 2 * C:]


_NAMES = ("out", "lse", "dq", "dk", "dv")


def _check(rep, q, k, v, dout, mask, factor=2.0, skip=()):
    """both entry points on both layouts against the float64 / float32 restatements; -> (kernel results of the contiguous layout, r64, r32)"""
    from s2d_amd import backward as B, ops
    Q = q.shape[1]
    bits, unm = R.pack_bits(mask) if mask is not None else (None, None)
    r64, r32 = R.masked_attn_ref(q, k, v, mask, H, F64, dout), R.masked_attn_ref(q, k, v, mask, H, F32, dout)
    first = None
    for lname, kk, vv in _layouts(k, v):
        fwd = lambda: ops.masked_attn(q, kk, vv, bits, unm, H=H, want_lse=True)
        out, lse = fwd()
        bwd = lambda: B.masked_attn_backward(q, kk, vv, out, lse, dout, bits, unm, H=H)
        got = (out, lse[:, :, :Q]) + tuple(bwd())
        again = fwd() + tuple(bwd())
        again = (again[0], again[1][:, :, :Q]) + again[2:]
        differ = [name for i, name in enumerate(_NAMES) if not torch.equal(again[i], got[i])]
        rep.true(f"{lname} second call of both entry points bitwise equal ({', '.join(_NAMES)})" + (": " + ", ".join(differ) + " differ" if differ else ""), not differ)
        for i, name in enumerate(_NAMES):
            if name not in skip:
                rep.cmp(f"{lname} {name}", got[i], r64[i], r32[i], factor)
        first = first or got
    return first, r64, r32


# --------------------------------------------------------------------------- a. object masks
@pytest.mark.parametrize("B,Q,T,hl,wl", [(2, 100, 3, 23, 40), (2, 37, 1, 9, 37), (2, 128, 2, 16, 33)])
def test_object_masks_forward_backward(B, Q, T, hl, wl):
    K = T * hl * wl
    rep = _Rep(f"object-{B}-{Q}-{T}x{hl}x{wl}")
    mask, info = R.object_masks(B, Q, T, hl, wl, torch.Generator().manual_seed(K))
    tile, fsplit, bsplit = R.masked_shares(R.effective(mask))
    print(f"attnrow {rep.row} wholly masked pairs: (query, tile) {tile:.3f} (query, forward split) {fsplit:.3f} (query, backward split) {bsplit:.3f}; "
          f"empty forward splits {R.splits(K)['empty']}")
    assert tile >= 0.5
    mask = mask.to(DEV)
    g = _gen(K)
    q, k, v, dout = _rn(g, B, Q, C), _rn(g, B, K, C), _rn(g, B, K, C), _rn(g, B, Q, C)
    (out, lse, dq, dk, dv), r64, r32 = _check(rep, q, k, v, dout, mask)

    # keys no query of clip 1 attends: the reference's gradient rows are exact zeros, and exp2(-inf) = 0 gives the kernel's the same
    if info["reserved_frame"] is not None:
        dead = R.effective(mask)[1].all(0)
        assert int(dead.sum()) >= hl * wl
        assert not bool(r64[3][1][dead].any()) and not bool(r64[4][1][dead].any())
        rep.true(f"dk rows of the {int(dead.sum())} keys masked for every query of clip 1 are bitwise 0.0", not bool(dk[1][dead].view(torch.int32).any()))
        rep.true(f"dv rows of the {int(dead.sum())} keys masked for every query of clip 1 are bitwise 0.0", not bool(dv[1][dead].view(torch.int32).any()))
    # one free key j: the output row is v[j], and softmax over one key has no gradient in q
    dq_top = float(dq.abs().max())
    for qq, j in info["single"].items():
        vj = v[:, j]
        rep.below(f"q{qq} (only key {j} free) |out - v[j]| / max|v[j]|", float((out[:, qq] - vj).abs().max()) / float(vj.abs().max()), 1e-6)
        rep.below(f"q{qq} (only key {j} free) |dq| / max|dq|", float(dq[:, qq].abs().max()) / dq_top, 1e-6)
    # q7 sees one tile, q8 everything but that tile: each output recomputed from its own keys alone
    for qq in (7, 8):
        for b in range(B):
            idx = (~mask[b, qq]).nonzero().flatten()
            if qq == 7:
                assert idx.tolist() == list(range(32 * info["tile"], 32 * info["tile"] + 32))
            args = (q[b:b + 1, qq:qq + 1], k[b:b + 1, idx], v[b:b + 1, idx], None, H)
            rep.cmp(f"out(q{qq}, clip {b}) from its {idx.numel()} free keys alone", out[b:b + 1, qq:qq + 1],
                    R.masked_attn_ref(*args, F64)[0], R.masked_attn_ref(*args, F32)[0])
    rep.done()


# --------------------------------------------------------------------------- b. small K and edge Q
@pytest.mark.parametrize("Q", [1, 32, 33, 128])
@pytest.mark.parametrize("K", [1, 31, 32, 33, 127, 129])
def test_small_k_edge_q_forward_backward(K, Q):
    rep = _Rep(f"small-K{K}-Q{Q}")
    g = _gen(1000 * K + Q)
    q, k, v, dout = _rn(g, 1, Q, C), _rn(g, 1, K, C), _rn(g, 1, K, C), _rn(g, 1, Q, C)
    masks = [("no mask", None)]
    rnd = lambda: torch.rand((1, Q, K), device=DEV, generator=g) < 0.5
    if Q > 1:
        m = rnd()
        m[0, 0] = True                                                   # every key masked: attends everywhere
        m[0, Q - 1] = True
        m[0, Q - 1, K // 2] = False                                      # a single free key
        masks.append(("masked", m))
    else:                                                                # one query cannot be both
        m0 = torch.ones((1, 1, K), device=DEV, dtype=torch.bool)
        m1 = m0.clone()
        m1[0, 0, K // 2] = False
        masks += [("all masked", m0), ("one free key", m1)]
    # where softmax runs over one key, dq and dk are 0 in the reference: the difference of two terms p dP k / sqrt(d) and p delta k / sqrt(d)
    # (q in place of k for dk) that are equal in exact arithmetic.  "0 to 1e-6" is taken relative to the size of those terms, and such
    # a gradient is not compared relative to max|0|
    dp_top = float(torch.einsum("bqhd,bkhd->bhqk", dout.reshape(1, Q, H, D), v.reshape(1, K, H, D)).abs().max()) / math.sqrt(D)
    for mname, mask in masks:
        rep.row = f"small-K{K}-Q{Q} {mname}"
        zero_grads = K == 1 or mname == "one free key"
        (out, lse, dq, dk, dv), r64, r32 = _check(rep, q, k, v, dout, mask, skip=("dq", "dk") if zero_grads else ())
        if zero_grads:
            j = K // 2
            assert float(r64[2].abs().max()) < 1e-12 and float(r64[3].abs().max()) < 1e-12
            rep.below("|out - v[j]| / max|v[j]|", float((out - v[:, j:j + 1]).abs().max()) / float(v[:, j].abs().max()), 1e-6)
            rep.below("|dq| / (max|dP| max|k| / sqrt(d))", float(dq.abs().max()) / (dp_top * float(k.abs().max())), 1e-6)
            # dk sums Q such residues
            rep.below("|dk| / (Q max|dP| max|q| / sqrt(d))", float(dk.abs().max()) / (Q * dp_top * float(q.abs().max())), 1e-6)
        elif mask is not None and Q > 1:
            j = K // 2
            rep.below("single free key: |out - v[j]| / max|v[j]|", float((out[:, Q - 1] - v[:, j]).abs().max()) / float(v[:, j].abs().max()), 1e-6)
            rep.below("single free key: |dq| / (max|dP| max|k| / sqrt(d))", float(dq[:, Q - 1].abs().max()) / (dp_top * float(k.abs().max())), 1e-6)
    rep.done()


# --------------------------------------------------------------------------- c. score scale
def _scores_max(q, k):
    s = torch.einsum("bqhd,bkhd->bhqk", q.double().reshape(q.shape[0], -1, H, D), k.double().reshape(k.shape[0], -1, H, D)) / math.sqrt(D)
    return s


def _case_scale(g, sigma):
    mask, _ = R.object_masks(1, 100, 3, 23, 40, torch.Generator().manual_seed(2760))
    q, k, v, dout = _rn(g, 1, 100, C), _rn(g, 1, 2760, C), _rn(g, 1, 2760, C), _rn(g, 1, 100, C)
    return q * math.sqrt(sigma), k * math.sqrt(sigma), v, dout, mask.to(DEV)


def _case_shift(g):
    """sigma = 1; every k row gains, per head, a multiple of the head's mean query so that the scores of a query move together:
    q_i . dk = c q_i . mean_q, on average over the queries c |mean_q|^2 = 40 sqrt(32) (the scaled score moves by +40 on average, by
    -190 .. +270 for single queries): a large part that softmax has to cancel"""
    q, k, v, dout, mask = _case_scale(g, 1.0)
    mq = q.reshape(1, 100, H, D).mean(1, keepdim=True)                     # [1,1,H,D]
    c = 40.0 * math.sqrt(D) / (mq * mq).sum(-1, keepdim=True)
    k = (k.reshape(1, -1, H, D) + c * mq).reshape(1, -1, C).contiguous()
    return q, k, v, dout, mask


def _case_peaked(g):
    """no mask, K = 20000: per head every query and key 12345 share a direction u (q = a u + 0.3 n, k_peak = a u, the other keys 0.3 n
    with a^2 / sqrt(32) = 15 ln 2), so the peak sits 15 +- 1 binades above ~2^14.3 flat keys whose total mass is comparable; v has mean 1
    so that the tail adds coherently.  In the peak's forward split and everywhere in the backward the tail's probabilities are
    ~2^-15: their split high parts are fp16 subnormals, which the f16 MFMA has to keep"""
    Q, K, peak = 100, 20000, 12345
    a = math.sqrt(15.0 * math.log(2.0) * math.sqrt(D))
    u = torch.nn.functional.normalize(_rn(g, 1, 1, H, D), dim=-1)
    q = (a * u + 0.3 * _rn(g, 1, Q, H, D)).reshape(1, Q, C)
    k = 0.3 * _rn(g, 1, K, H, D)
    k[:, peak] = a * u[:, 0]
    v, dout = _rn(g, 1, K, C) + 1.0, _rn(g, 1, Q, C)
    return q, k.reshape(1, K, C), v, dout, None


_SCALE_CASES = {"sigma1": lambda g: _case_scale(g, 1.0), "sigma4": lambda g: _case_scale(g, 4.0), "sigma16": lambda g: _case_scale(g, 16.0),
                "shift": _case_shift, "peaked": _case_peaked}


@pytest.mark.parametrize("case", list(_SCALE_CASES))
def test_score_scale_forward_backward(case):
    rep = _Rep("scale-" + case)
    q, k, v, dout, mask = _SCALE_CASES[case](_gen(sum(case.encode())))
    s = _scores_max(q, k)
    print(f"attnrow {rep.row} max|s| = {float(s.abs().max()):.1f}")
    if case == "peaked":
        gap = (s[..., 12345] - s.median(-1).values) / math.log(2.0)
        mass = torch.exp(s - s[..., 12345:12346]).sum(-1) - 1.0
        print(f"attnrow {rep.row} peak above the median key: {float(gap.min()):.1f} .. {float(gap.max()):.1f} binades; tail mass / peak {float(mass.min()):.2f} .. {float(mass.max()):.2f}")
        assert 12.0 < float(gap.min()) and float(gap.max()) < 18.0 and 0.1 < float(mass.min()) and float(mass.max()) < 10.0
    del s
    _check(rep, q, k, v, dout, mask, factor=_SCORE_SCALE_FACTOR)
    rep.done()


# --------------------------------------------------------------------------- d. the scalar backward
def test_scalar_backward_subprocess():
    """(a) and (b) on attn_bwd_kv_kernel / attn_bwd_q_kernel: S2D_ATTN_BWD_MFMA=0 is read once per process, hence a child"""
    if os.environ.get("S2D_ATTN_BWD_MFMA") is not None:
        pytest.skip("once, from the default dispatch, outside a forced run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, S2D_ATTN_BWD_MFMA="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(root, "tests", "test_gpu_attn_masks.py"),
                        "-k", "test_object_masks_forward_backward or test_small_k_edge_q_forward_backward"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=900)
    print("\n".join("attnrow scalar-backward " + line.split("attnrow ", 1)[1] for line in r.stdout.splitlines() if "attnrow " in line))      # -s: progress dots may precede
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "27 passed" in r.stdout, r.stdout[-500:]
