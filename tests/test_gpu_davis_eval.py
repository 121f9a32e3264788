"""GPU side of the DAVIS J&F evaluator (csrc/davis_eval.hip, s2d_amd/davis_eval.py): each kernel word for word against the numpy
restatement of the metric (tests/davis_refs.py, proved in tests/test_davis_refs_cpu.py), with no element excluded and no
tolerance, and the evaluator end to end on PNG folders against the same references: per-frame J and F as equal float64
quotients of equal integers, the assignment, and the tables (1e-12 on the final means).

The disk-dilation and index-plane launches are one workgroup per tile with no grid cap or stride loop (they refuse F x tiles
>= 2^31), and the boundary-map launch is one thread per word, so those have no case past a cap; the per-frame count kernel loops
over a frame's words in trips of 256 and splits long frames into chunks, and has cases for both."""
import numpy as np
import pytest
import torch

from tests import davis_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device_bits(masks, pad_ones=False):
    w = np.stack([R.pack_bits(m, pad_ones) for m in masks])
    return torch.from_numpy(w.view(np.int32)).to(DEV)


def words(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- index planes
def _index_video(rng, T, H, W, kind):
    if kind == "void":
        return np.full((T, H, W), 255, np.uint8)
    v = rng.integers(0, 256, (T, H, W)).astype(np.uint8)                # every label, 255 and those above any K included
    if kind == "sparse":
        v[rng.random((T, H, W)) < 0.7] = 0
    return v


@pytest.mark.parametrize("K", [1, 20, 254])
@pytest.mark.parametrize("hw", R.INDEX_SHAPES)
def test_index_planes(hw, K):
    from s2d_amd.davis_eval import index_planes
    H, W = hw
    T = 1 if H * W > 10000 else 3
    rng = np.random.default_rng(H * W + K)
    for kind in ("dense", "sparse", "void"):
        v = _index_video(rng, T, H, W, kind)
        planes, void = index_planes(torch.from_numpy(v).to(DEV), K)
        assert planes.shape == (K, T, (H * W + 31) // 32) and void.shape == planes.shape[1:]
        got, gv = words(planes), words(void)
        for t in range(T):
            assert np.array_equal(gv[t], R.pack_bits(v[t] == 255)), (kind, t)
            for k in range(1, K + 1):
                assert np.array_equal(got[k - 1, t], R.pack_bits(v[t] == k)), (kind, t, k)


def test_index_planes_without_labels_and_bad_arguments():
    from s2d_amd import ops
    from s2d_amd._lib import lib
    from s2d_amd.davis_eval import index_planes
    v = torch.from_numpy(_index_video(np.random.default_rng(0), 2, 7, 33, "dense")).to(DEV)
    planes, void = index_planes(v, 0)
    assert planes.shape == (0, 2, 8) and np.array_equal(words(void)[1], R.pack_bits(v[1].cpu().numpy() == 255))
    with pytest.raises(ValueError):
        index_planes(v, 255)
    raw = lib()._raw_s2d_index_planes_u32
    assert raw(v.data_ptr(), 2, 7, 33, 255, void.data_ptr(), void.data_ptr(), ops._stream()) == -1
    assert raw(v.data_ptr(), 2, 0, 33, 1, void.data_ptr(), void.data_ptr(), ops._stream()) == -1
    assert raw(v.data_ptr(), 2, 7, 33, 1, None, void.data_ptr(), ops._stream()) == -1


# ------------------------------------------------------------------------------------------------------------- boundary maps
@pytest.mark.parametrize("hw", R.BMAP_SHAPES)
def test_seg2bmap(hw):
    """every content in one call (the plane stride), the input's padding bits all ones: the output's are 0"""
    from s2d_amd.davis_eval import seg2bmap_planes
    H, W = hw
    c = R.bmap_contents(np.random.default_rng(H * 1000 + W), H, W)
    got = words(seg2bmap_planes(device_bits(list(c.values()), pad_ones=True), H, W))
    for f, (name, m) in enumerate(c.items()):
        assert np.array_equal(got[f], R.pack_bits(R.seg2bmap_ref(m))), name
        assert not R.unpack_bits(got[f], H, W)[1].any(), name
    clean = words(seg2bmap_planes(device_bits(list(c.values())), H, W))
    assert np.array_equal(clean, got)


# ------------------------------------------------------------------------------------------------------------- disk dilation
def _check_dilation(H, W, radius):
    from s2d_amd.davis_eval import disk_dilate_planes
    c = R.dilate_contents(np.random.default_rng(H + W + radius), H, W)
    got = words(disk_dilate_planes(device_bits(list(c.values()), pad_ones=True), H, W, radius))
    for f, (name, m) in enumerate(c.items()):
        assert np.array_equal(got[f], R.pack_bits(R.dilate_fast(m, radius))), name
        assert not R.unpack_bits(got[f], H, W)[1].any(), name


@pytest.mark.parametrize("radius", R.RADII)
@pytest.mark.parametrize("hw", R.DILATE_SMALL)
def test_disk_dilation_small_frames(hw, radius):
    """unaligned and aligned rows, H < R, W < R, a disk larger than the image"""
    _check_dilation(*hw, radius)


@pytest.mark.parametrize("hw,radius", R.DILATE_LARGE)
def test_disk_dilation_row_and_word_tiles(hw, radius):
    """several row tiles per plane; rows of more than 32 words (two word tiles)"""
    _check_dilation(*hw, radius)


def test_disk_dilation_radius_65_is_refused():
    from s2d_amd import ops
    from s2d_amd._lib import lib
    from s2d_amd.davis_eval import disk_dilate_planes, sequence_metrics
    H, W = 9, 33
    bits = device_bits([np.ones((H, W), bool)])
    out = torch.full_like(bits, 0x5a5a5a5a)
    raw = lib()._raw_s2d_disk_dilate_bits_u32
    st = ops._stream()
    assert raw(bits.data_ptr(), 1, H, W, 65, out.data_ptr(), st) == -1
    assert raw(bits.data_ptr(), 1, H, W, 0, out.data_ptr(), st) == -1
    assert raw(bits.data_ptr(), 1, H, W, 1, bits.data_ptr(), st) == -1                   # out aliases bits
    assert raw(None, 1, H, W, 1, out.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert (out == 0x5a5a5a5a).all()
    assert raw(bits.data_ptr(), 1, H, W, 64, out.data_ptr(), st) == 0
    assert np.array_equal(words(out)[0], R.pack_bits(np.ones((H, W), bool)))
    with pytest.raises(ValueError):
        disk_dilate_planes(bits, H, W, 65)
    with pytest.raises(ValueError):
        sequence_metrics(np.zeros((3, H, W), np.uint8), np.zeros((3, H, W), np.uint8), bound_th=65)


# ------------------------------------------------------------------------------------------------------------- per-frame counts
@pytest.mark.parametrize("shape", [(1, 1, 1, 40, 45), (20, 5, 7, 40, 45), (9, 3, 2, 300, 1100), (2, 2, 1, 600, 1000)])
def test_frame_cross_counts(shape):
    """(P, G, T) = (1, 1, 1) and (20, 5, 7) at an unaligned wpf (57 words: a partial trip, three proposal tiles); 10313 words in
    three chunks of 14 trips each; 18750 words and one pair tile: five chunks"""
    from s2d_amd.davis_eval import frame_cross_counts
    P, G, T, H, W = shape
    rng = np.random.default_rng(P * 100 + G)
    a = rng.random((P, T, H, W)) < 0.4
    b = rng.random((G, T, H, W)) < 0.6
    if P > 1:
        a[1] = False
    da = device_bits(a.reshape(P * T, H * W)).view(P, T, -1)
    db = device_bits(b.reshape(G * T, H * W)).view(G, T, -1)
    got = frame_cross_counts(da, db)
    assert got.dtype == torch.int32 and got.shape == (P, G, T)
    want = (a.reshape(P, 1, T, -1) & b.reshape(1, G, T, -1)).sum(-1)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(frame_cross_counts(da, db).cpu().numpy(), want)                # the output is zeroed by every call


# ------------------------------------------------------------------------------------------------------------- the evaluator
SEQUENCES = {"small": (6, 40, 70, 3, 20, ()), "middle": (5, 120, 214, 3, 7, ()), "davis": (5, 480, 854, 3, 20, ()),
             "few": (5, 40, 70, 3, 2, (3,))}                            # T, H, W, objects, proposals, objects without a proposal
_made = {}


def dataset():
    """name -> (gt, res, res_semi) index videos (res: permuted labels; res_semi: the objects keep theirs), and the references of
    both tasks, computed once"""
    if not _made:
        rng = np.random.default_rng(2017)
        for name, (T, H, W, G, n, drop) in SEQUENCES.items():
            gt = R.moving_discs(T, H, W, G, rng)
            _made[name] = (gt, R.proposals(gt, n, rng, drop=drop), R.proposals(gt, min(n, G + 2), rng, drop=drop, permute=False))
        _made["unsupervised"] = {name: R.sequence_ref(_made[name][0], _made[name][1]) for name in SEQUENCES}
        _made["semi-supervised"] = {name: R.sequence_ref(_made[name][0], _made[name][2], task="semi-supervised") for name in SEQUENCES}
    return _made


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    root = tmp_path_factory.mktemp("davis")
    d = dataset()
    for name in SEQUENCES:
        R.write_sequence(str(root / "gt"), name, d[name][0], palette=True)
        R.write_sequence(str(root / "res"), name, d[name][1], palette=name != "middle")
        R.write_sequence(str(root / "res_semi"), name, d[name][2], palette=True)
    return str(root / "gt"), str(root / "res"), str(root / "res_semi")


def _same(got, want):
    assert got["J"].dtype == np.float64 and got["J"].shape == want["J"].shape
    assert got["J"].tobytes() == want["J"].tobytes() and got["F"].tobytes() == want["F"].tobytes()
    assert got["assignment"].tolist() == want["assignment"].tolist()


@pytest.mark.parametrize("task", ["unsupervised", "semi-supervised"])
def test_evaluator_matches_the_references(folders, task):
    from s2d_amd.davis_eval import GLOBAL_KEYS, evaluate_davis
    d = dataset()
    assert [R.bound_pix(*SEQUENCES[n][1:3]) for n in ("small", "middle", "davis")] == [1, 2, 8]
    gt_dir, res_dir = folders[0], folders[1 if task == "unsupervised" else 2]
    out = evaluate_davis(gt_dir, res_dir, task=task)
    assert list(out["sequences"]) == sorted(SEQUENCES)
    for name in SEQUENCES:
        _same(out["sequences"][name], d[task][name])
    if task == "unsupervised":
        a = d[task]["small"]["assignment"].tolist()
        assert a != [0, 1, 2] and len(set(a)) == 3                      # the labels were permuted: the assignment has work to do
        assert int(d["few"][1].max()) == 2 and 2 in d[task]["few"]["assignment"].tolist()        # fewer proposals than objects: one takes an empty one
    else:
        assert all(d[task][n]["J"].shape[1] == SEQUENCES[n][0] - 2 and d[task][n]["J"][0].mean() > 0.3 for n in SEQUENCES)
    table, rows = R.tables_ref({name: d[task][name] for name in sorted(SEQUENCES)})
    assert list(out["global"]) == list(GLOBAL_KEYS)
    for k in GLOBAL_KEYS:
        assert abs(out["global"][k] - table[k]) <= 1e-12, k
    assert [r["Sequence"] for r in out["per_sequence"]] == [r["Sequence"] for r in rows]
    for r, w in zip(out["per_sequence"], rows):
        assert abs(r["J-Mean"] - w["J-Mean"]) <= 1e-12 and abs(r["F-Mean"] - w["F-Mean"]) <= 1e-12
    again = evaluate_davis(gt_dir, res_dir, task=task)
    for name in SEQUENCES:                                             # a second call: bitwise equal
        _same(again["sequences"][name], out["sequences"][name])
    assert again["global"] == out["global"]


def test_sequence_subset_and_cli(folders, tmp_path, capsys):
    from s2d_amd.davis_eval import evaluate_davis, main
    d = dataset()
    (tmp_path / "val.txt").write_text("few\nsmall\n")
    out = evaluate_davis(*folders[:2], sequences=str(tmp_path / "val.txt"))
    assert list(out["sequences"]) == ["few", "small"]
    table, rows = R.tables_ref({n: d["unsupervised"][n] for n in ("few", "small")})
    assert abs(out["global"]["J&F-Mean"] - table["J&F-Mean"]) <= 1e-12
    main(["--gt", folders[0], "--results", folders[1], "--sequences", str(tmp_path / "val.txt"), "--out", str(tmp_path / "o")])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].split()[0] == "J&F-Mean" and lines[1].split()[0] == f"{table['J&F-Mean']:.3f}"
    per = (tmp_path / "o" / "per-sequence_results.csv").read_text().splitlines()
    assert per[0] == "Sequence,J-Mean,F-Mean" and [l.split(",")[0] for l in per[1:]] == [r["Sequence"] for r in rows]
    assert (tmp_path / "o" / "global_results.csv").read_text().splitlines()[0].startswith("J&F-Mean,J-Mean,J-Recall")


def test_sequence_metrics_takes_device_tensors():
    from s2d_amd.davis_eval import sequence_metrics
    d = dataset()
    gt, res, _ = d["small"]
    got = sequence_metrics(torch.from_numpy(gt).to(DEV), torch.from_numpy(res).to(DEV))
    _same(got, d["unsupervised"]["small"])
    assert got["radius"] == 1
    with pytest.raises(ValueError, match="max_proposals"):
        sequence_metrics(gt, res, max_proposals=19)
