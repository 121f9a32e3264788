"""Pins tests/amp_refs.py, the references tests/test_gpu_amp_forms.py holds the AMP dense kernels to, without a GPU: the fp16 rounding
against constants written by hand, the float64 restatements against direct loops and torch, and the size table against what it is meant
to cover."""
import numpy as np
import pytest
import torch

from tests import amp_refs as R


def test_round_fp16_against_hand_written_constants():
    for x, want in R.HAND_PINNED:
        got = R.round_fp16(np.array([x], np.float32), flush=False)[0]
        assert got == want and np.signbit(got) == np.signbit(want), (x, got, want)
    assert np.isnan(R.round_fp16(np.array([np.nan], np.float32))[0])
    # the rounding is torch's `.half()` too, on every special value the GPU test uses
    v = np.concatenate([R.tie_values(), R.edge_values(), R.subnormal_values(), R.nonfinite_values()])
    np.testing.assert_array_equal(R.round_fp16(v, flush=False), torch.from_numpy(v).half().double().numpy())


def test_tie_values_are_ties_and_their_neighbours_are_not():
    v = R.tie_values().astype(np.float64).reshape(2, -1, 3)
    h = R.round_fp16(R.tie_values(), flush=False).reshape(2, -1, 3)
    assert np.isfinite(h).all()
    ulp = 2.0 ** (np.floor(np.log2(np.abs(v[..., 0]))) - 10)
    np.testing.assert_array_equal(np.abs(h[..., 0] - v[..., 0]), ulp / 2)                # the tie sits half an fp16 ulp from its image ...
    assert (np.abs(h[..., 1:] - v[..., 1:]) < ulp[..., None] / 2).all()                   # ... its float32 neighbours closer to theirs
    assert (h[..., 1] != h[..., 2]).all()                                                 # and they round apart
    m = np.abs(h[..., 0]) / ulp                                                           # ties go to the even mantissa
    assert (m % 2 == 0).all()
    up, down = h[0, :, 0] > v[0, :, 0], h[0, :, 0] < v[0, :, 0]
    assert up.any() and down.any()


def test_flush_rule_and_subnormal_values():
    v = R.subnormal_values()
    kept, flushed = R.round_fp16(v, flush=False), R.round_fp16(v, flush=True)
    sub = (np.abs(kept) > 0) & (np.abs(kept) < R.F16_MIN_NORMAL)
    assert sub.sum() >= 8 and (~sub).sum() >= 6
    assert (flushed[sub] == 0).all() and np.array_equal(flushed[~sub], kept[~sub])
    assert np.array_equal(R.round_fp16(v), flushed if R.FLUSH_SUBNORMAL_OPERANDS else kept)
    nf = R.round_fp16(R.nonfinite_values())
    assert np.isinf(nf[:4]).all() and np.isnan(nf[4])


def test_ref_gemm_nt_against_loops():
    rng = np.random.default_rng(0)
    bs, M, N, K = 2, 5, 6, 8
    A, B = rng.integers(-8, 9, (bs, M, K)).astype(np.float32), rng.integers(-8, 9, (bs, N, K)).astype(np.float32)
    sc, bi = np.array([0.5, 1, 2, 0.5, 1, 2], np.float32), rng.integers(-8, 9, (N,)).astype(np.float32)
    res = rng.integers(-8, 9, (3, 7)).astype(np.float32)
    got = R.ref_gemm_nt(A, B, sc, bi, res, True, res_rows=3, res_cols=4)
    for b in range(bs):
        for m in range(M):
            for n in range(N):
                v = sum(int(A[b, m, k]) * int(B[b, n, k]) for k in range(K)) * float(sc[n]) + float(bi[n])
                if n < 4:
                    v += float(res[m % 3, n])
                assert got[b, m, n] == max(v, 0.0)
    # shared B, full and batched residuals, against torch in float64
    r2, r3 = rng.standard_normal((M, N)), rng.standard_normal((bs, M, N))
    tA, tB = torch.from_numpy(A).double(), torch.from_numpy(B[0]).double()
    np.testing.assert_array_equal(R.ref_gemm_nt(A, B[0], res=r2), (tA @ tB.t() + torch.from_numpy(r2)).numpy())
    np.testing.assert_array_equal(R.ref_gemm_nt(A, B[0], res=r3), (tA @ tB.t() + torch.from_numpy(r3)).numpy())


@pytest.mark.parametrize("row", R.CONV_ROWS, ids=str)
def test_ref_conv_against_torch_float64(row):
    N, H, W, Ci, Co, k, stride, pad, has_s, has_b, relu, has_r = row
    rng = np.random.default_rng(1)
    x, w = rng.integers(-8, 9, (N, H, W, Ci)).astype(np.float32), rng.integers(-8, 9, (Co, k, k, Ci)).astype(np.float32)
    Ho, Wo = R.conv_out_hw(H, W, k, stride, pad)
    sc = rng.choice([0.5, 1.0, 2.0], Co).astype(np.float32) if has_s else None
    bi = rng.integers(-8, 9, (Co,)).astype(np.float32) if has_b else None
    res = rng.integers(-8, 9, (N, Ho, Wo, Co)).astype(np.float32) if has_r else None
    got = R.ref_conv2d_nhwc(x, w, stride, pad, sc, bi, res, relu)
    t = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double().permute(0, 3, 1, 2), None, stride, pad)
    t = t.permute(0, 2, 3, 1)
    if has_s:
        t = t * torch.from_numpy(sc).double()
    if has_b:
        t = t + torch.from_numpy(bi).double()
    if has_r:
        t = t + torch.from_numpy(res).double()
    t = torch.relu(t) if relu else t
    assert got.shape == (N, Ho, Wo, Co)
    np.testing.assert_array_equal(got, t.numpy())                       # integers: exact in any order


def test_size_table_covers_what_it_is_meant_to():
    vec = [r for r in R.GEMM_ROWS if R.gemm_row_vector_epilogue(r)]
    sca = [r for r in R.GEMM_ROWS if not R.gemm_row_vector_epilogue(r)]
    for rows, ns in ((vec, {n for n in R.N_SET if n % 4 == 0}), (sca, set(R.N_SET))):
        assert {r[2] for r in rows} >= set(R.M_SET)
        assert {r[3] for r in rows} >= ns
        assert {r[4] for r in rows} >= set(R.K_SET)
        wg = {R.gemm_row_workgroups(r) for r in rows}
        assert 1 in wg and 9 in wg and any(2 <= n <= 7 for n in wg) and any(n >= 16 for n in wg)
    assert all(r[3] % 4 == 0 for r in vec) and {2, 41} <= {r[3] for r in sca}
    assert {r[5] for r in vec} == {0, 4} and 3 in {r[5] for r in sca if r[3] % 4 == 0}
    kinds = lambda rows: {R.gemm_row_form(r)[8] for r in rows}           # noqa: E731
    assert kinds(vec) == kinds(sca) == {"none", "full", "batched", "periodic", "cols"}
    assert {r[9][1] for r in R.GEMM_ROWS if isinstance(r[9], tuple) and r[9][0] == "periodic"} == {7, 65}
    assert {r[9][1:] for r in R.GEMM_ROWS if isinstance(r[9], tuple) and r[9][0] == "cols"} == {(8, 12)}
    for rows in (vec, sca):
        assert {(r[0], r[1]) for r in rows} >= {(1, False), (3, False), (3, True)}
    assert len({R.gemm_row_form(r) + r[2:5] for r in R.GEMM_ROWS}) == len(R.GEMM_ROWS)
    # every K is a multiple of 4 (the export's rule); K = 68 leaves one live 16-B piece in the second k-tile
    assert all(r[4] % 4 == 0 for r in R.GEMM_ROWS) and 68 - 64 == 4
    geo = {r[:8] for r in R.CONV_ROWS}
    assert geo >= {(1, 33, 47, 4, 64, 7, 2, 3), (2, 9, 11, 64, 64, 3, 1, 1), (1, 10, 13, 128, 66, 3, 2, 1), (2, 8, 12, 256, 128, 1, 2, 0), (1, 5, 5, 8, 132, 3, 1, 1)}
    assert (2, 9, 11, 64, 64, 3, 1, 1, True, True, True, True) in R.CONV_ROWS and (2, 8, 12, 256, 128, 1, 2, 0, True, True, False, False) in R.CONV_ROWS
    assert len({R.conv_row_form(r) for r in R.CONV_ROWS}) == len(R.CONV_ROWS)


def test_one_hot_and_latin_operands():
    Bm, s = R.one_hot_operand(68)
    assert Bm.shape == (68, 68) and (np.count_nonzero(Bm, axis=1) == 1).all() and set(s.tolist()) == {0.25, 1.0, 4.0}
    v = np.arange(5, dtype=np.float32)
    A = R.latin_rows(v, 68)
    assert A.shape == (5, 68) and all(set(A[:, k].tolist()) == set(v.tolist()) for k in range(68))
    # the product against the one-hot operand is the rounded operand times the factor: no accumulation
    np.testing.assert_array_equal(R.ref_gemm_nt(R.round_fp16(A), Bm), R.round_fp16(A) * s)
