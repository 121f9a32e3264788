"""The row-resident short-K GEMM kernel (csrc/gemm_rows.hip, switch S2D_GEMM_ROWS): bit-identical to the kernels that run its launches
with the switch off, inside the split-fp16 static-weight bound against float64, and taken for exactly the launches it is meant for."""
import itertools

import numpy as np
import pytest
import torch

from s2d_amd.utils import synth

pytestmark = pytest.mark.gpu

MS = (1, 31, 128, 129, 300)      # a single row, a partial wave, an exact tile, a tile plus one row, several tiles with a tail
NS = (128, 132, 192, 544)        # one column tile, a 4-column tail, three tiles, the benchmark's odd width
KS = (32, 64, 96, 256)           # one k-block, two, a count that is no power of two, the maximum
SHAPES = list(itertools.product(MS, NS, KS))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _launches():
    from s2d_amd._lib import lib
    return lib().call("s2d_gemm_rows_launches")


def _operands(M, N, K):
    """A of mixed magnitude (rows x 1e-3, x 1, x 1e3 in turn), static weights, and what the epilogue forms read"""
    a = synth.randn(11, 1, (M, K))
    a *= np.array([1e-3, 1.0, 1e3], np.float32)[np.arange(M) % 3][:, None]
    A = _dev(a)
    W = torch.nn.Parameter(_dev(synth.randn(11, 2, (N, K)) * K ** -0.5), requires_grad=False)
    sc = _dev(synth.randn(11, 3, (N,)) * 0.5 + 1)
    bi = _dev(synth.randn(11, 4, (N,)))
    rc = (N // 2) & ~3
    return A, W, sc, bi, _dev(synth.randn(11, 5, (M, N))), _dev(synth.randn(11, 6, (64, N))), _dev(synth.randn(11, 7, (100, rc))), rc


def _forms(M, N, K):
    """-> [(name, run() -> tensor [M, N], float64 reference)]: every epilogue form of the launches the kernel takes"""
    from s2d_amd import ops
    A, W, sc, bi, R, R64, R100, rc = _operands(M, N, K)
    prod = A.double() @ W.double().t()
    rows = torch.arange(M, device="cuda")

    def wide():
        out = torch.full((M, N + 12), 7.0, device="cuda")          # a column slice of a wider buffer: ldc > N
        ops.gemm_nt(A, W, out=out)
        assert bool((out[:, N:] == 7.0).all())
        return out[:, :N].contiguous()

    ref100 = prod + bi.double()
    ref100[:, :rc] += R100.double()[rows % 100]
    return [
        ("plain, ldc > N", wide, prod),
        ("scale bias residual relu", lambda: ops.gemm_nt(A, W, sc, bi, R, relu=True), torch.relu(prod * sc.double() + bi.double() + R.double())),
        ("bias", lambda: ops.gemm_nt(A, W, bias=bi), prod + bi.double()),
        ("residual of 64 rows", lambda: ops.gemm_nt(A, W, res=R64, res_rows=64, relu=True), torch.relu(prod + R64.double()[rows % 64])),
        ("residual of 100 rows on res_cols < N", lambda: ops.gemm_nt(A, W, bias=bi, res=R100, res_rows=100, res_cols=rc), ref100),
    ]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bit_equal_to_the_tiled_kernels(monkeypatch, M, N, K):
    """S2D_GEMM_ROWS=2 against =0 on the same operands: torch.equal, and the launch counter says which kernel ran"""
    for name, run, _ in _forms(M, N, K):
        monkeypatch.setenv("S2D_GEMM_ROWS", "0")
        n0 = _launches()
        old = run()
        assert _launches() == n0, name
        monkeypatch.setenv("S2D_GEMM_ROWS", "2")
        new = run()
        assert _launches() == n0 + 1, name
        assert torch.equal(old, new), f"{name}: {int((old != new).sum())} of {old.numel()} values differ, max {float((old - new).abs().max()):.3e}"


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_against_float64(monkeypatch, M, N, K):
    """the bound tests/test_gpu_dense.py holds the split-fp16 static-weight kernels to, on rows of A scaled by 1e-3, 1 and 1e3"""
    monkeypatch.setenv("S2D_GEMM_ROWS", "2")
    for name, run, ref in _forms(M, N, K):
        n0 = _launches()
        y = run()
        assert _launches() == n0 + 1, name
        np.testing.assert_allclose(y.cpu().numpy(), ref.cpu().numpy(), rtol=2e-6, atol=2e-6 * float(ref.abs().max()), err_msg=name)


def test_routing(monkeypatch):
    """launches the kernel is not meant for stay where they are, whatever the switch says"""
    from s2d_amd import ops
    M = 300

    def par(N, K):
        return torch.nn.Parameter(_dev(synth.randn(12, 2, (N, K)) * K ** -0.5), requires_grad=False)

    A256, A288, A40 = (_dev(synth.randn(12, 1, (M, K))) for K in (256, 288, 40))
    A3 = _dev(synth.randn(12, 3, (2, M, 64)))
    B3 = _dev(synth.randn(12, 4, (2, 128, 64)))
    Bdyn = _dev(synth.randn(12, 5, (128, 256)))
    gate = _dev(synth.randn(12, 6, (M, 128)))
    W288, W40, W64, W256 = par(128, 288), par(128, 40), par(64, 256), par(128, 256)
    calls = [
        ("K = 288", lambda: ops.gemm_nt(A288, W288)),
        ("K = 40", lambda: ops.gemm_nt(A40, W40)),
        ("N = 64", lambda: ops.gemm_nt(A256, W64)),
        ("3-D B", lambda: ops.gemm_nt(A3, B3)),
        ("dynamic B", lambda: ops.gemm_nt(A256, Bdyn)),
        ("gate", lambda: ops.gemm_nt_gate(A256, W256, gate, 2.0)),
        ("dropout", lambda: ops.gemm_nt(A256, W256, dropout=(0.25, 1234, 3))),
    ]
    for name, run in calls:
        monkeypatch.setenv("S2D_GEMM_ROWS", "0")
        old = run()
        monkeypatch.setenv("S2D_GEMM_ROWS", "2")
        n0 = _launches()
        new = run()
        assert _launches() == n0, name
        assert torch.equal(old, new), name
    # the same weights, an eligible launch: the counter does move
    n0 = _launches()
    ops.gemm_nt(A256, W256)
    assert _launches() == n0 + 1
