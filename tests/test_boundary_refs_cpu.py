"""The references of the Boundary AP tests (tests/boundary_refs.py) checked on the CPU: the published iterated routine equals the
square form the kernel is built on, every named case has the property it is named for, the dilation of the usual frame sizes,
and the worked AP case through the host half of the evaluator."""
import math

import numpy as np
import pytest

from tests import boundary_refs as R

ALL_CASES = [(n, hw, d) for n, hw in R.SHAPES.items() for d in R.RADII] + [("chained", hw, d) for hw, d in R.CHAINED] + \
            [("wide", hw, d) for hw, d in R.WIDE]


@pytest.mark.parametrize("name,hw,d", ALL_CASES, ids=[f"{n}-{h}x{w}-d{d}" for n, (h, w), d in ALL_CASES])
def test_iterated_routine_equals_square_form(name, hw, d):
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    for cn, m in R.contents(rng, H, W).items():
        assert np.array_equal(R.boundary_ref(m, d), R.boundary_square(m, d)), cn


@pytest.mark.parametrize("hw,d", [((480, 854), 20), ((720, 1280), 29), ((1080, 1920), 44)])
def test_iterated_routine_equals_square_form_at_frame_sizes(hw, d):
    m = R.discs(np.random.default_rng(sum(hw)), *hw, n=4, salt=0, edge=True)
    b = R.boundary_ref(m, d)
    assert np.array_equal(b, R.boundary_square(m, d))
    assert 0 < b.sum() < m.sum()                                  # discs large enough to keep an interior
    assert m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any()


def test_named_cases_have_their_property():
    S = R.SHAPES
    assert S["w31"][1] % 32 == 31 and S["w32"][1] % 32 == 0 and S["w33"][1] % 32 == 1
    assert S["straddle"][1] % 32 != 0 and S["wide_straddle"][1] % 32 != 0 and S["wide_straddle"][1] > 64
    assert 32 // S["rows_per_word"][1] >= 3                        # several rows in one word
    assert S["one_column"][1] == 1 and S["one_row"][0] == 1 and S["one_pixel"] == (1, 1)
    assert S["aligned"][1] % 32 == 0 and S["aligned"][0] * S["aligned"][1] % 32 == 0
    assert any(d < 32 for d in R.RADII) and 32 in R.RADII and any(d > 32 for d in R.RADII)
    assert {15, 16, 17, 31, 32, 33} <= set(R.RADII)                # either side of the powers of two the doubling stops at
    for (H, W) in S.values():
        ones = np.ones((H, W), bool)
        for d in R.RADII:
            if d >= math.ceil(min(H, W) / 2):                      # a window that does not fit: the band is the whole mask
                for cn, m in R.contents(np.random.default_rng(d), H, W).items():
                    assert np.array_equal(R.boundary_ref(m, d), m), (H, W, d, cn)
            else:
                assert R.boundary_ref(ones, d).sum() == H * W - (H - 2 * d) * (W - 2 * d)
    for (H, W), d in R.CHAINED:                                   # the window fits, so the radius is not clamped away
        assert 2 * d + 1 <= min(H, W) and d >= 63
    assert {d for _, d in R.CHAINED} >= {64, 65} and max(d for _, d in R.CHAINED) > 128
    assert all(W > 32 * 32 for (H, W), d in R.WIDE)


def test_pack_unpack_roundtrip_and_padding():
    m = R.discs(np.random.default_rng(3), 7, 5)
    w = R.pack_bits(m)
    img, pad = R.unpack_bits(w, 7, 5)
    assert np.array_equal(img, m) and not pad.any() and len(w) == 2
    img1, pad1 = R.unpack_bits(R.pack_bits(m, pad_ones=True), 7, 5)
    assert np.array_equal(img1, m) and pad1.all() and len(pad1) == 64 - 35
    assert R.pack_bits(np.array([[True] + [False] * 32 + [True]]))[1] == 2    # pixel 33 -> word 1, bit 1


def test_boundary_dilation_values():
    from s2d_amd.ytvis_eval import boundary_dilation
    assert boundary_dilation(720, 1280) == 29
    assert boundary_dilation(480, 854) == 20
    assert boundary_dilation(1080, 1920) == 44
    assert boundary_dilation(10, 10) == 1
    assert boundary_dilation(720, 1280, 0.02) == max(1, int(round(0.02 * math.sqrt(720 ** 2 + 1280 ** 2))))
    assert boundary_dilation(64, 64, 0.01) == 1 and boundary_dilation(64, 64, 0.0) == 1


def test_worked_case_arithmetic_and_host_half():
    """mask IoU 1520 / 1680, boundary IoU 76 / 236 at d = 1; through YTVISEval: AP 0.9 on the mask IoU, 0 on the minimum"""
    from s2d_amd.ytvis_eval import GroundTruth, YTVISEval
    g, d = R.square_case()
    assert (int((g & d).sum()), int((g | d).sum())) == (1520, 1680)
    assert R.boundary_ref(g, 1).sum() == 156 and R.boundary_ref(d, 1).sum() == 156
    assert R.video_boundary_iou_ref([d], [g], 1) == (76, 236)
    assert R.video_boundary_iou_ref([d, None], [g, g], 1) == (76, 236 + 156)      # an absent frame is an empty plane
    doc = {"videos": [{"id": 1, "height": 64, "width": 64, "length": 1}], "categories": [{"id": 1, "name": "a"}],
           "annotations": [{"id": 1, "video_id": 1, "category_id": 1, "iscrowd": 0, "segmentations": [None], "areas": [1600]}]}
    stats = {}
    for kind, iou in (("segm", 1520 / 1680), ("boundary", min(1520 / 1680, 76 / 236))):
        video = {1: {"dt_ids": [1], "scores": [0.9], "labels": [1], "avg_areas": [1600.0], "ious": np.array([[iou]])}}
        ev = YTVISEval(GroundTruth(doc)).evaluate(video).accumulate()
        stats[kind] = ev.summarize(out=None)
    assert stats["segm"][:3] == pytest.approx([0.9, 1.0, 1.0], abs=1e-12)
    assert list(stats["boundary"][:3]) == [0.0, 0.0, 0.0]
