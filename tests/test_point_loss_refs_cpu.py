"""The exact point-loss cases (tests/point_loss_refs.py) show what they promise -- without a GPU.  tests/test_gpu_point_loss_ties.py compares
the HIP point loss with the float64 reference on these cases; a case whose keys do not tie, whose fp32 samples differ from the float64
ones, or on which the tie rule moves nothing would let that comparison pass whatever the kernel does with ties."""
import numpy as np
import pytest

from tests import point_loss_refs as R


def _exact_in_fp32(c):
    """coordinates, sampled logits and sampled labels: the fp32 evaluation (the device's expression tree) equals float64 bit for bit"""
    for pts in (c["cov"], c["crd"]):
        assert pts.dtype == np.float32 and (pts >= 0).all() and (pts < 1).all()
        for planes in (c["src"], c["tt"].astype(np.float32)):
            a32, a64 = R.sample_np(planes, pts, np.float32), R.sample_np(planes, pts, np.float64)
            assert a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64)
    hm, wm = c["map"]
    for k, n in ((0, wm), (1, hm)):                      # the map position is pixel + k/8 exactly
        pos = c["cov"][..., k].astype(np.float64) * n - 0.5
        assert np.array_equal(pos * 8, np.round(pos * 8))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_exact_case_ties_and_rule_spread(name):
    c = R.exact_case(name)
    assert c["n_over"] == 3 * c["P"] and c["n_unc"] == int(0.75 * c["P"]) and all(t.any() for t in c["tt"])
    _exact_in_fp32(c)
    ties, take = R.check_structure(c)
    sp_loss, sp_grad = R.rule_spread(c)
    print(f"ptcase {name} ties {ties.tolist()} take {take.tolist()} rule spread: loss {sp_loss:.2e} grad {sp_grad:.2e}")
    if c["take"] == "all":
        # every tied point is taken: no rule can matter (what the case pins is the count: one tie more or fewer is a different loss)
        assert sp_loss == 0 and sp_grad == 0
    else:
        assert sp_loss >= 100 * R.LOSS_RTOL and sp_grad >= 100 * R.GRAD_REL


def test_stream_eligibility_of_the_cases():
    """A-C are sized for the streamed kernels (3P and P/4 multiples of 4, H*W a multiple of 32), every E case for the recompute ones"""
    for name, c in R.CASES.items():
        P, (H, W) = c["P"], c["tgt"]
        streamed = (3 * P) % 4 == 0 and (P - int(0.75 * P)) % 4 == 0 and (H * W) % 32 == 0
        assert streamed == (not name.startswith("E_")), name
        assert (H * W) % 16 == 0
    assert R.PART_ROWS == 124 * 1024 // ((256 + 8) * 4) - 3 and -(-128 // R.PART_ROWS) == 2


def test_op_inputs_hold_the_rows_in_reference_order():
    c = R.exact_case("A_p256")
    op = R.op_inputs(c)
    Q, T, hm, wm = op["dims"]
    maps = op["ml"][0, 0].T.reshape(Q, T, hm, wm)
    for s in range(2):
        for t in range(T):
            assert np.array_equal(maps[op["iq"][0, s], t], c["src"][s * T + t])
            assert np.array_equal(op["tgt"][0, op["it"][0, s], t], c["tt"][s * T + t])


def test_many_rows_case():
    d = R.F_DIMS
    c = R.many_rows_case("ties")
    op = c["op"]
    assert op["ml"].shape == (10, 2, 8 * 16 * 32, 32) and op["cov"].shape == (10, 512, 192, 2) and op["crd"].shape == (10, 512, 16, 2)
    assert d["NL"] * d["B"] * d["Q"] * d["T"] == 5120 and all(t.any() for t in c["tt"])        # every row active: 4096 streamed + 1024
    _exact_in_fp32(c)
    keys, thr, below, ties, take = R.select_stats(c["src"], c["cov"], c["n_unc"])
    inner = (take > 0) & (take < ties)
    assert inner.sum() >= 500                                        # nearly every one of a layer's 512 rows has a tie to break
    sp_loss, sp_grad = R.rule_spread(c)
    print(f"ptcase F_ties rows with 0 < take < ties: {inner.sum()} of 512, rule spread: loss {sp_loss:.2e}")
    assert sp_loss >= 100 * R.LOSS_RTOL
    s = R.many_rows_case("smooth")
    k = np.sort(np.abs(R.sample_np(s["src"], s["cov"])), axis=1)
    assert (np.diff(k, axis=1) > 0).all()                            # smooth maps, uniform points: no two keys equal


@pytest.mark.parametrize("placement", R.G_PLACEMENTS)
def test_cluster_case_piles_taps_on_one_pixel(placement):
    c = R.cluster_case(placement)
    _exact_in_fp32(c)
    g = R.loss_masks_ref(c["src"], c["tt"], c["cov"], c["crd"], c["n_unc"], c["num_masks"])[2]
    hm, wm = c["map"]
    for r in range(g.shape[0]):
        i0, j0 = c["hot"][0][r], c["hot"][1][r]
        out = g[r].copy()
        out[i0:i0 + 2, j0:j0 + 2] = 0
        assert not out.any() and g[r, i0:i0 + 2, j0:j0 + 2].any()      # the whole row's gradient sits in one 2 x 2 block
    # all P points add to the hot pixel with weight >= 1/4 (centre: 1): far beyond the few dozen taps the density argument assumes
    x = c["cov"][..., 0].astype(np.float64) * wm - 0.5
    assert (np.floor(x) == c["hot"][1][:, None]).all()
