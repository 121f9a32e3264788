"""CPU checks of the keymask discovery driver (python -m s2d_amd.keymask.discover): CLI, dataset detection, path rules, job
slicing, the tracker boundary and the fused kernel's export."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_flags_and_defaults_match_keymask_args():
    from s2d_amd.keymask.discover import parse_args
    a = parse_args([])
    assert (a.workers, a.manualSeed, a.gpu_id, a.batchSize) == (4, 777, "0", 1)
    assert a.video_base_path == "/mnt/data/datasets/DAVIS/JPEGImages/480p"
    assert a.mask_base_path == "/mnt/data/outputs/DAVIS/cuts3d/pseudo_annotations"
    assert a.save_path == "/mnt/data/outputs/cotracker/segmentation_masks/DAVIS/all/"
    assert a.video_output_dir == "/mnt/data/outputs/cotracker/videos"
    assert a.visibility_maps_output_base == "/mnt/data/outputs/cotracker/visibility_maps"
    assert a.visibility_clusters_output_base == "/mnt/data/outputs/cotracker/visibility_clusters"
    assert a.annotation_output_path == "/mnt/data/outputs/cotracker/annotations/DAVIS/all/"
    assert (a.visibility_threshold, a.matching_threshold) == (0.3, 0.5)
    assert (a.job_id, a.videos_per_job, a.debug) == (0, -1, False)
    assert (a.tracker, a.tracker_checkpoint, a.dataset_name) == ("cotracker", None, None)
    b = parse_args(["--video-base-path", "v", "--mask-base-path", "m", "--save-path", "s", "--visibility-maps-output-base", "vm",
                    "--visibility-clusters-output-base", "vc", "--annotation-output-path", "an", "--visibility-threshold", "0.4",
                    "--matching-threshold", "0.7", "--job-id", "3", "--videos-per-job", "5", "--debug", "--tracker", "a.b:c",
                    "--tracker-checkpoint", "ck.pth", "--dataset-name", "MOSE"])
    assert (b.video_base_path, b.mask_base_path, b.save_path, b.visibility_maps_output_base, b.visibility_clusters_output_base,
            b.annotation_output_path) == ("v", "m", "s", "vm", "vc", "an")
    assert (b.visibility_threshold, b.matching_threshold, b.job_id, b.videos_per_job, b.debug) == (0.4, 0.7, 3, 5, True)
    assert (b.tracker, b.tracker_checkpoint, b.dataset_name) == ("a.b:c", "ck.pth", "MOSE")


@pytest.mark.parametrize("path,want", [
    ("/d/DAVIS/JPEGImages/480p", ("DAVIS", "all")),
    ("/d/DAVIS/trainval/480p", ("DAVIS", "all")),
    ("/d/ytvis2021/train/JPEGImages", ("ytvis2021", "train")),
    ("/d/ytvis2021/valid/JPEGImages", ("ytvis2021", "valid")),
    ("/d/ytvis2019/test/JPEGImages", ("ytvis2019", "valid")),
    ("/d/ovis/train", ("ovis", "train")),
    ("/d/VIPSeg/imgs", ("VIPSeg", "imgs")),
    ("/d/MOSE/valid", ("MOSE", "valid")),
    ("/d/sa-v/sav_000", ("SA-V", "train")),
])
def test_dataset_and_split_detection(path, want):
    from s2d_amd.keymask.discover import detect_dataset
    assert detect_dataset(path) == want


def test_unknown_dataset_raises_and_the_override():
    from s2d_amd.keymask.discover import detect_dataset, stage_dataset
    with pytest.raises(ValueError, match="Unknown dataset"):
        detect_dataset("/d/mydata/frames")
    with pytest.raises(ValueError, match="Unknown dataset"):
        stage_dataset("/d/mydata/frames/v1")
    assert detect_dataset("/d/mydata/train/frames", "ovis") == ("ovis", "train")
    assert detect_dataset("/d/DAVIS/frames", "MOSE") == ("MOSE", "valid")      # the override wins over the substring
    assert detect_dataset("/d/mydata/frames", "mine") == ("mine", "all")
    assert stage_dataset("/d/mydata/frames/v1", "mine") == ("mine", "all")


@pytest.mark.parametrize("path,want", [
    ("/d/DAVIS/480p/bear", ("DAVIS", "all")),
    ("/d/DAVIS/trainval/bear", ("DAVIS", "train")),                           # the stages' own split rule
    ("/d/ytvis2021/valid/JPEGImages/v", ("ytvis2021", "valid")),
    ("/d/ytvis2019/test/v", ("ytvis2019", "test")),
    ("/d/MOSE/val/v", ("MOSE", "val")),
    ("/d/VIPSeg/imgs/v", ("VIPSeg", "imgs")),
])
def test_stage_dataset_detection(path, want):
    from s2d_amd.keymask.discover import stage_dataset
    assert stage_dataset(path) == want


def _touch(d, names):
    os.makedirs(d, exist_ok=True)
    for n in names:
        open(os.path.join(d, n), "w").close()


def test_make_paths_davis_numeric_order(tmp_path):
    from s2d_amd.keymask.discover import make_paths
    _touch(tmp_path / "f", ["10.jpg", "2.jpg", "1.jpg", "notes.txt"])
    _touch(tmp_path / "l", ["10.png", "1.png", "2.png", "x.npy"])
    imgs, lbls = make_paths(str(tmp_path / "f"), str(tmp_path / "l"), "DAVIS")
    assert [os.path.basename(p) for p in imgs] == ["1.jpg", "2.jpg", "10.jpg"]
    assert [os.path.basename(p) for p in lbls] == ["1.png", "2.png", "10.png"]
    assert imgs[0] == f"{tmp_path / 'f'}/1.jpg"


def test_make_paths_sav_and_ovis(tmp_path):
    from s2d_amd.keymask.discover import make_paths
    _touch(tmp_path / "f", ["sav_10.jpg", "sav_9.jpg", "sav_100.jpg"])
    _touch(tmp_path / "l", ["sav_100.png", "sav_9.png", "sav_10.png"])
    imgs, lbls = make_paths(str(tmp_path / "f"), str(tmp_path / "l"), "SA-V")
    assert [os.path.basename(p) for p in imgs] == ["sav_9.jpg", "sav_10.jpg", "sav_100.jpg"]
    assert [os.path.basename(p) for p in lbls] == ["sav_9.png", "sav_10.png", "sav_100.png"]
    imgs, lbls = make_paths(str(tmp_path / "f"), str(tmp_path / "l"), "ovis")
    assert [os.path.basename(p) for p in imgs] == ["sav_9.jpg", "sav_10.jpg", "sav_100.jpg"]
    # ovis: the reference sorts the frames twice and leaves the labels in directory order
    assert [os.path.basename(p) for p in lbls] == [n for n in os.listdir(tmp_path / "l")]
    with pytest.raises(ValueError):
        make_paths(str(tmp_path / "f"), str(tmp_path / "l"), "DAVIS")              # int("sav_10") as the reference


def test_job_slicing_and_pairing(tmp_path):
    from s2d_amd.keymask.discover import video_and_mask_dirs
    names = [f"v{i}" for i in range(7)]
    for n in names:
        os.makedirs(tmp_path / "vid" / n)
        os.makedirs(tmp_path / "msk" / n)
    _touch(tmp_path / "vid", ["a_file.txt"])
    v, m = video_and_mask_dirs(str(tmp_path / "vid"), str(tmp_path / "msk"))
    assert [os.path.basename(p) for p in v] == names and [os.path.basename(p) for p in m] == names
    for job, want in ((0, ["v0", "v1", "v2"]), (1, ["v3", "v4", "v5"]), (2, ["v6"]), (3, [])):
        v, m = video_and_mask_dirs(str(tmp_path / "vid"), str(tmp_path / "msk"), job, 3)
        assert [os.path.basename(p) for p in v] == want == [os.path.basename(p) for p in m]
    os.rmdir(tmp_path / "msk" / "v1")                                            # a missing mask folder shifts the pairing
    v, m = video_and_mask_dirs(str(tmp_path / "vid"), str(tmp_path / "msk"), 0, 3)
    assert [os.path.basename(p) for p in m] == ["v0", "v2", "v3"]


def test_load_tracker_from_a_factory_spec():
    from s2d_amd.keymask.tracker import load_tracker
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        t = load_tracker("keymask_stub_tracker:make_tracker")
    finally:
        sys.path.remove(os.path.join(ROOT, "tests", "golden"))
    assert callable(t) and t.calls == []
    t = load_tracker("collections:OrderedDict")
    assert type(t).__name__ == "OrderedDict"
    with pytest.raises(ValueError):
        load_tracker("no_colon_here")


def test_load_cotracker_without_the_package_is_a_clear_error():
    from s2d_amd.keymask.tracker import load_tracker
    try:
        import cotracker  # noqa: F401
        pytest.skip("cotracker is installed")
    except ImportError:
        pass
    with pytest.raises(ImportError, match="cotracker"):
        load_tracker("cotracker", "scaled_offline.pth")


def test_discover_imports_without_cotracker():
    code = ("import sys; sys.modules['cotracker'] = None; import s2d_amd.keymask.discover, s2d_amd.keymask.merge; "
            "assert 'cotracker.predictor' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    for dp, _, fs in os.walk(os.path.join(ROOT, "s2d_amd")):
        for f in fs:
            if f.endswith(".py") and f != "tracker.py":
                assert "cotracker." not in open(os.path.join(dp, f)).read().replace("cotracker_", ""), f


def test_fused_export_in_library_and_abi_unchanged():
    from s2d_amd.build import build
    from s2d_amd._lib import parse_header
    dll = ctypes.CDLL(build(verbose=False))
    assert hasattr(dll, "s2d_track_point_id_counts") and "s2d_track_point_id_counts" in parse_header()
    assert dll.s2d_abi_version() == 11
