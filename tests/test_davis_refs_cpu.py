"""The DAVIS references (tests/davis_refs.py) proved without a GPU: against independently written forms, on hand-worked cases,
and that each named case of the GPU file has the property it is named for; then the host side of s2d_amd/davis_eval.py (CLI
parsing, PNG reading, the error paths, the statistics and the quotients)."""
import numpy as np
import pytest
from scipy import ndimage

from tests import davis_refs as R

ALL_DILATE = [(hw, r) for hw in R.DILATE_SMALL for r in R.RADII] + list(R.DILATE_LARGE)


# --------------------------------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("hw,r", ALL_DILATE)
def test_dilate_refs_are_scipys_disk_dilation(hw, r):
    """explicit shifted ORs == scipy.ndimage.binary_dilation(structure=disk(R), border_value=0) == the distance-transform form,
    for every shape and radius of the GPU file: on all its contents where that is cheap, else (scipy's dilation costs image x
    disk) on the sparse ones merged into one image"""
    H, W = hw
    c = R.dilate_contents(np.random.default_rng(H + W + r), H, W)
    if H * W * (2 * r + 1) ** 2 > 5e6:
        c = {"sparse": c["bleed"] | c["noise"] | c["br"] | c["mid_top"]}
    for name, m in c.items():
        want = ndimage.binary_dilation(m, structure=R.disk(r), border_value=0)
        assert np.array_equal(R.dilate_ref(m, r), want), name
        assert np.array_equal(R.dilate_fast(m, r), want), name


@pytest.mark.parametrize("hw", R.BMAP_SHAPES)
def test_seg2bmap_two_forms_agree(hw):
    H, W = hw
    for name, m in R.bmap_contents(np.random.default_rng(H * 1000 + W), H, W).items():
        assert np.array_equal(R.seg2bmap_ref(m), R.seg2bmap_pad(m)), name


def test_single_pixel_has_a_four_pixel_boundary():
    m = np.zeros((9, 11), bool)
    m[4, 6] = True
    b = R.seg2bmap_ref(m)
    assert sorted(zip(*np.nonzero(b))) == [(3, 5), (3, 6), (4, 5), (4, 6)]
    last = np.zeros((9, 11), bool)
    last[8, 10] = True                                                 # the corner pixel itself is never boundary
    assert sorted(zip(*np.nonzero(R.seg2bmap_ref(last)))) == [(7, 9), (7, 10), (8, 9)]
    row = np.zeros((9, 11), bool)
    row[8, 3:6] = True                                                 # last row: compares only east
    assert [x for x in np.nonzero(R.seg2bmap_ref(row)[8])[0]] == [2, 5]


def test_identical_and_empty_masks():
    m = R.disc_mask(40, 70, 20, 30, 9)
    z = np.zeros_like(m)
    assert R.jaccard_ref(m, m) == 1.0 and R.f_measure_ref(m, m, 1) == (1.0, 1.0, 1.0)
    assert R.jaccard_ref(z, z) == 1.0 and R.f_measure_ref(z, z, 1) == (1.0, 1.0, 1.0)
    assert R.jaccard_ref(z, m) == 0.0 and R.f_measure_ref(z, m, 1) == (1.0, 0.0, 0.0)
    assert R.f_measure_ref(m, z, 1) == (0.0, 1.0, 0.0)


@pytest.mark.parametrize("radius", [1, 3, 8])
def test_half_plane_pins_the_radius(radius):
    """a full-height half-plane's boundary map is its last column; shifted by k columns it is matched for k <= R and missed at
    R + 1"""
    H, W = 24, 60
    g = np.zeros((H, W), bool)
    g[:, :20] = True
    for k, want in [(0, 1.0), (radius, 1.0), (radius + 1, 0.0)]:
        p = np.zeros((H, W), bool)
        p[:, :20 + k] = True
        assert R.f_measure_ref(p, g, radius, dilate=R.dilate_ref)[2] == want, k


@pytest.mark.parametrize("radius", [1, 2, 3, 8])
def test_single_pixel_dilates_to_the_clipped_disk(radius):
    H, W = 12, 14
    for y, x in [(6, 7), (0, 0), (11, 13), (2, 12)]:
        m = np.zeros((H, W), bool)
        m[y, x] = True
        yy, xx = np.mgrid[:H, :W]
        assert np.array_equal(R.dilate_ref(m, radius), (yy - y) ** 2 + (xx - x) ** 2 <= radius * radius)
    assert R.disk(2).sum() == 13 and R.disk(1).sum() == 5 and R.disk(8)[0, 8] and not R.disk(8)[1, 1]


def test_bound_pix():
    assert [R.bound_pix(*hw) for hw in ((480, 854), (720, 1280), (1080, 1920), (40, 70), (120, 214))] == [8, 12, 18, 1, 2]
    assert R.bound_pix(480, 854, 5) == 5


def test_db_statistics_on_a_ramp():
    """10 values: ids = round(linspace(1, 10, 5) + 1e-10) - 1 = round([1, 3.25, 5.5, 7.75, 10]) - 1 = [0, 2, 5, 7, 9] (5.5 plus the
    epsilon rounds up), so the bins are v[0:3], v[2:6], v[5:8], v[7:10]"""
    v = np.arange(10) / 10.0
    mean, recall, decay = R.db_statistics_ref(v)
    assert mean == pytest.approx(0.45, abs=1e-15) and recall == 0.4
    assert decay == pytest.approx((0.0 + 0.1 + 0.2) / 3 - (0.7 + 0.8 + 0.9) / 3, abs=1e-15)


def test_assignment_follows_j_and_f_not_j():
    """one object (a 20 x 30 rectangle), two proposals: label 1 a blob well inside it (J = 375 / 600, every side off by more than
    R = 1: F = 0), label 2 its one-pixel outline ring (J = 96 / 600, F = 1).  The blob has the better J, the ring the better J&F."""
    H, W, T = 40, 70, 3
    assert R.bound_pix(H, W) == 1
    gt = np.zeros((T, H, W), np.uint8)
    gt[:, 10:30, 20:50] = 1
    ring = np.zeros((H, W), bool)
    ring[10:30, 20:50] = True
    ring[11:29, 21:49] = False
    res = np.zeros_like(gt)
    res[:, ring] = 2
    res[:, 13:28, 23:48] = 1
    g = gt[0] == 1
    j_blob, j_ring = R.jaccard_ref(res[0] == 1, g), R.jaccard_ref(res[0] == 2, g)
    f_blob, f_ring = R.f_measure_ref(res[0] == 1, g, 1)[2], R.f_measure_ref(res[0] == 2, g, 1)[2]
    assert (j_blob, f_blob) == (0.625, 0.0) and (j_ring, f_ring) == (0.16, 1.0)
    assert j_blob > j_ring and (j_blob + f_blob) / 2 < (j_ring + f_ring) / 2
    out = R.sequence_ref(gt, res)
    assert out["assignment"].tolist() == [1] and (out["J"] == 0.16).all() and (out["F"] == 1.0).all()
    semi = R.sequence_ref(gt, res, task="semi-supervised")             # proposal 1 against object 1, one frame left
    assert semi["J"].tolist() == [[0.625]] and semi["F"].tolist() == [[0.0]]


def test_cases_have_their_properties():
    rng = np.random.default_rng(0)
    assert [R.bound_pix(h, w) for h, w in ((40, 70), (120, 214), (480, 854))] == [1, 2, 8]
    gt = R.moving_discs(6, 40, 70, 3, rng)
    assert (gt == 255).any() and sorted(set(np.unique(gt)) - {0, 255}) == [1, 2, 3]
    res = R.proposals(gt, 20, rng)
    assert int(res.max()) == 20 and len(np.unique(res)) >= 15
    few = R.proposals(gt, 2, rng, drop=(3,))
    assert int(few.max()) == 2                                          # fewer proposals than objects
    for hw in R.DILATE_SMALL:
        H, W = hw
        b = R.dilate_contents(rng, H, W)["bleed"]
        assert b.reshape(-1)[np.flatnonzero(b.reshape(-1))[0] + 1] or H == 1   # the two pixels are neighbours in the flat layout
    assert any(W % 32 for (_, W) in R.DILATE_SMALL) and any(W % 32 == 0 for (_, W) in R.DILATE_SMALL)
    assert any(H < 8 for (H, _) in R.DILATE_SMALL) and any(W < 8 for (_, W) in R.DILATE_SMALL)
    assert any(W > 32 * 32 for ((_, W), _) in R.DILATE_LARGE)
    w = R.pack_bits(np.ones((5, 7), bool), pad_ones=True)
    img, pad = R.unpack_bits(w, 5, 7)
    assert img.all() and pad.all() and len(pad) == 29 and not R.unpack_bits(R.pack_bits(np.ones((5, 7), bool)), 5, 7)[1].any()


# --------------------------------------------------------------------------------------------------- the evaluator's host side
def test_host_quotients_and_statistics_match_the_references():
    from s2d_amd import davis_eval as D
    rng = np.random.default_rng(3)
    v = rng.random(37)
    assert D.db_statistics(v) == R.db_statistics_ref(v)
    assert [D.davis_bound_pix(*hw) for hw in ((480, 854), (720, 1280), (1080, 1920))] == [8, 12, 18]
    assert D.davis_bound_pix(480, 854, 3) == 3
    with pytest.raises(ValueError):
        D.davis_bound_pix(480, 854, 2.5)
    pm, rm = np.array([3, 0, 5, 0, 0]), np.array([2, 0, 0, 7, 0])
    n_fg, n_gt = np.array([4, 0, 6, 0, 9]), np.array([5, 0, 0, 8, 3])
    want = [2 * (3 / 4) * (2 / 5) / (3 / 4 + 2 / 5), 1.0, 0.0, 0.0, 0.0]
    assert D._f_measure(pm, rm, n_fg, n_gt).tolist() == want
    assert D._jaccard(np.array([2, 0]), np.array([3, 0]), np.array([4, 0])).tolist() == [2 / 5, 1.0]
    per = {"a": {"J": rng.random((2, 9)), "F": rng.random((2, 9))}, "b": {"J": rng.random((1, 5)), "F": rng.random((1, 5))}}
    table, rows = D.tables(per)
    rt, rr = R.tables_ref(per)
    assert list(table) == list(D.GLOBAL_KEYS) and dict(table) == rt and [dict(r) for r in rows] == rr
    assert [r["Sequence"] for r in rows] == ["a_1", "a_2", "b_1"]


def test_cli_parsing_and_table_text(tmp_path):
    from s2d_amd import davis_eval as D
    a = D.parse_args(["--gt", "g", "--results", "r"])
    assert (a.task, a.bound_th, a.sequences, a.out, a.max_proposals) == ("unsupervised", 0.008, None, None, 20)
    a = D.parse_args(["--gt", "g", "--results", "r", "--task", "semi-supervised", "--bound-th", "0.01", "--sequences", "s.txt", "--out", "o"])
    assert (a.task, a.bound_th, a.sequences, a.out) == ("semi-supervised", 0.01, "s.txt", "o")
    with pytest.raises(SystemExit):
        D.parse_args(["--gt", "g", "--results", "r", "--task", "interactive"])
    table = dict(zip(D.GLOBAL_KEYS, (0.5, 0.25, 1, 0, 0.75, 0.125, -0.5)))
    text = D.format_table(table).splitlines()
    assert text[0].split() == list(D.GLOBAL_KEYS) and text[1].split() == ["0.500", "0.250", "1.000", "0.000", "0.750", "0.125", "-0.500"]
    result = {"global": table, "per_sequence": [{"Sequence": "a_1", "J-Mean": 0.25, "F-Mean": 0.75}]}
    D.write_csvs(result, str(tmp_path / "o"))
    assert (tmp_path / "o" / "global_results.csv").read_text().splitlines()[1] == "0.500,0.250,1.000,0.000,0.750,0.125,-0.500"
    assert (tmp_path / "o" / "per-sequence_results.csv").read_text().splitlines() == ["Sequence,J-Mean,F-Mean", "a_1,0.250,0.750"]
    (tmp_path / "s.txt").write_text("b\n\n a \n")
    assert D._sequence_names(str(tmp_path), str(tmp_path / "s.txt")) == ["b", "a"]
    assert D._sequence_names(str(tmp_path), None) == ["o"] and D._sequence_names(str(tmp_path), ["x"]) == ["x"]


def test_png_reading(tmp_path):
    from s2d_amd import davis_eval as D
    vid = R.moving_discs(2, 12, 17, 2, np.random.default_rng(1))
    R.write_sequence(str(tmp_path), "p", vid, palette=True)
    R.write_sequence(str(tmp_path), "l", vid, palette=False)
    from PIL import Image
    assert Image.open(tmp_path / "p" / "00000.png").mode == "P" and Image.open(tmp_path / "l" / "00000.png").mode == "L"
    for name in ("p", "l"):
        got = D._read_video(str(tmp_path), name, ["00000.png", "00001.png"])
        assert got.dtype == np.uint8 and np.array_equal(got, vid)


def _folders(tmp_path):
    rng = np.random.default_rng(2)
    gt = R.moving_discs(3, 12, 17, 2, rng)
    R.write_sequence(str(tmp_path / "gt"), "s", gt)
    R.write_sequence(str(tmp_path / "res"), "s", R.proposals(gt, 3, rng))
    return str(tmp_path / "gt"), str(tmp_path / "res"), gt


def test_error_paths_name_the_file_and_need_no_device(tmp_path, monkeypatch):
    from PIL import Image
    from s2d_amd import davis_eval as D
    gt_dir, res_dir, gt = _folders(tmp_path)
    monkeypatch.setattr(D, "sequence_metrics", lambda *a, **k: pytest.fail("device work before the checks"))
    bad = tmp_path / "res" / "s" / "00001.png"
    keep = bad.read_bytes()

    Image.fromarray(np.zeros((12, 17, 3), np.uint8)).save(bad)         # an RGB result
    with pytest.raises(ValueError, match="00001.png.*RGB"):
        D.evaluate_davis(gt_dir, res_dir)
    bad.unlink()                                                       # a missing result frame
    with pytest.raises(FileNotFoundError, match="00001.png"):
        D.evaluate_davis(gt_dir, res_dir)
    Image.fromarray(np.zeros((12, 18), np.uint8), mode="L").save(bad)  # another size
    with pytest.raises(ValueError, match="00001.png.*12x18.*12x17"):
        D.evaluate_davis(gt_dir, res_dir)
    many = np.zeros((12, 17), np.uint8)
    many[3, 4] = 21
    Image.fromarray(many, mode="L").save(bad)                          # a 21st proposal
    with pytest.raises(ValueError, match="00001.png.*21.*max_proposals = 20"):
        D.evaluate_davis(gt_dir, res_dir)
    with pytest.raises(ValueError, match="max_proposals = 2"):
        D.evaluate_davis(gt_dir, res_dir, max_proposals=2, sequences=["s"])
    bad.write_bytes(keep)
    with pytest.raises(FileNotFoundError, match="nothing"):
        D.evaluate_davis(gt_dir, res_dir, sequences=["nothing"])
    with pytest.raises(ValueError, match="task"):
        D.evaluate_davis(gt_dir, res_dir, task="interactive")


def test_demo_mask_names_are_found(tmp_path, monkeypatch):
    """the demo writes its index PNG as mask_<frame>.png beside the overlay frame: that file is the result frame"""
    import os
    from PIL import Image
    from s2d_amd import davis_eval as D
    gt_dir, res_dir, gt = _folders(tmp_path)
    res = D._read_video(res_dir, "s", ["00000.png", "00001.png", "00002.png"])
    for f in sorted(os.listdir(os.path.join(res_dir, "s"))):
        os.rename(os.path.join(res_dir, "s", f), os.path.join(res_dir, "s", "mask_" + f))
        Image.fromarray(np.zeros((12, 17, 3), np.uint8)).save(os.path.join(res_dir, "s", f))        # the RGB overlay frame
    seen = {}
    monkeypatch.setattr(D, "sequence_metrics", lambda g, r, **k: seen.update(g=g, r=r) or {"J": np.ones((2, 3)), "F": np.ones((2, 3))})
    out = D.evaluate_davis(gt_dir, res_dir)
    assert np.array_equal(seen["g"], gt) and np.array_equal(seen["r"], res) and out["global"]["J&F-Mean"] == 1.0


def test_no_cpu_fallback(tmp_path):
    """with the files in order the evaluator goes to the device, and a host tensor is refused, not scored on the host"""
    import torch
    from s2d_amd import davis_eval as D
    with pytest.raises(RuntimeError):
        D.index_planes(torch.zeros((1, 4, 4), dtype=torch.uint8), 1)
    with pytest.raises(RuntimeError):
        D.seg2bmap_planes(torch.zeros((1, 1), dtype=torch.int32), 4, 4)
    with pytest.raises(ValueError):
        D.sequence_metrics(np.zeros((3, 480, 854), np.uint8), np.zeros((3, 480, 854), np.uint8), bound_th=65)
