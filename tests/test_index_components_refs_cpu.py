"""The host references of the connected-component ops against an independent flood fill, the constructed cases against the property
each is named for, the option plumbing of both drivers, and the argument refusals of the C ABI (returned before any launch, so no
GPU is needed)."""
import ctypes

import numpy as np
import pytest

from tests import index_components_refs as R

ERR_ARG = -1                                                                   # S2D_ERR_ARG


def flood_components(index, conn):
    """pure Python: pixels in raster order, an unlabelled one floods its component with 1 + its own flat index"""
    N, H, W = index.shape
    near = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    labels, area = np.zeros((N, H, W), np.int32), np.zeros((N, H, W), np.int32)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                v = index[n, y, x]
                if v == 0 or labels[n, y, x]:
                    continue
                name, stack, count = 1 + y * W + x, [(y, x)], 0
                labels[n, y, x] = name
                while stack:
                    cy, cx = stack.pop()
                    count += 1
                    for dy, dx in near:
                        ny, nx = cy + dy, cx + dx
                        if 0 <= ny < H and 0 <= nx < W and index[n, ny, nx] == v and not labels[n, ny, nx]:
                            labels[n, ny, nx] = name
                            stack.append((ny, nx))
                area[n, y, x] = count
    return labels, area


@pytest.fixture(scope="module")
def dll():
    from s2d_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.s2d_index_components_tile.argtypes = [P, P]
    lib.s2d_index_components_workspace_bytes.argtypes = [I, I, I]
    lib.s2d_index_components_workspace_bytes.restype = ctypes.c_long
    lib.s2d_index_components_i32.argtypes = [P, I, I, I, I, P, P, P, P]
    lib.s2d_index_filter_components_u8.argtypes = [P, P, P, I, I, I, I, I, P, P, P, P, P]
    return lib


@pytest.fixture(scope="module")
def tile(dll):
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert dll.s2d_index_components_tile(ctypes.addressof(th), ctypes.addressof(tw)) == 0
    assert th.value >= 2 and tw.value >= 2 and th.value * tw.value <= 65536          # tile-local offsets fit 16 bits
    return th.value, tw.value


@pytest.mark.parametrize("conn", [4, 8])
def test_reference_equals_flood_fill_on_small_maps(conn):
    rng = np.random.default_rng(5)
    maps = [rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(2, h, w), p=[0.4, 0.3, 0.2, 0.1])
            for h, w in ((1, 1), (1, 12), (12, 1), (5, 7), (12, 12), (11, 12))]
    maps += [R.checkerboard(12, 12), R.checkerboard(7, 5, 3, 4), R.spiral(12, 11), np.zeros((1, 4, 4), np.uint8), R.full_frame(3, 5)]
    for m in maps:
        want = flood_components(m, conn)
        got = R.ref_components(m, conn)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        assert got[1].sum() == (m != 0).sum()


def test_reference_filter_on_a_hand_made_map():
    m = np.array([[[1, 1, 0, 1, 0, 2],
                   [0, 0, 0, 1, 0, 2],
                   [1, 0, 0, 0, 2, 0],
                   [0, 1, 0, 0, 0, 0]]], np.uint8)
    # conn 4: id 1 has components {0,1} (2), {3,9} (2), {12} (1), {19} (1); id 2 has {5,11} (2), {16} (1)
    out, removed, _ = R.ref_filter(m, 2, False, 4)
    assert removed.tolist() == [3] and out[0].tolist() == [[1, 1, 0, 1, 0, 2], [0, 0, 0, 1, 0, 2], [0] * 6, [0] * 6]
    out, removed, _ = R.ref_filter(m, 0, True, 4)                    # the tie among id 1 goes to the component that starts at pixel 0
    assert removed.tolist() == [5] and out[0].tolist() == [[1, 1, 0, 0, 0, 2], [0, 0, 0, 0, 0, 2], [0] * 6, [0] * 6]
    out, removed, rgb = R.ref_filter(m, 0, True, 8, R.make_rgb(m))   # conn 8: id 2 is one component of 3, id 1's {12,19} joins
    assert removed.tolist() == [4] and out[0].tolist() == [[1, 1, 0, 0, 0, 2], [0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 2, 0], [0] * 6]
    assert (rgb[0][(m[0] != 0) & (out[0] == 0)] == 0).all() and (rgb[0][m[0] == 0] == 7).all() and (rgb[0][out[0] != 0] != 0).all()
    out, removed, _ = R.ref_filter(m, 3, True, 4)                    # a min_area above the largest area removes the whole id
    assert removed.tolist() == [int((m != 0).sum())] and not out.any()


def _tiles_of(mask, th, tw):
    ys, xs = np.nonzero(mask)
    return {(int(y) // th, int(x) // tw) for y, x in zip(ys, xs)}


def test_named_cases_have_the_property_they_are_named_for(tile):
    th, tw = tile
    H, W = R.frame_shape(th, tw)
    sp = R.geometry_case("spiral", th, tw)
    assert sp.shape == (1, H, W) and R.count_components(sp, 4) == 1 and R.count_components(sp, 8) == 1
    assert _tiles_of(sp[0], th, tw) >= {(i, j) for i in range(3) for j in range(3)}
    assert int((sp != 0).sum()) > 2 * (H + W) and sp[0, H // 2 - 1:H // 2 + 2, W // 2 - 1:W // 2 + 2].any()      # it reaches the centre
    # one pixel wide: no 2 x 2 block of the path
    assert not (sp[0, :-1, :-1] & sp[0, 1:, :-1] & sp[0, :-1, 1:] & sp[0, 1:, 1:]).any()
    for name in ("u", "u_lr", "u_ud"):
        u = R.geometry_case(name, th, tw)
        assert R.count_components(u, 4) == 1 and R.count_components(u, 8) == 1
        # without the tile the bar crosses in the middle tile column, the arms fall apart
        bar_rows = np.nonzero(u[0][:, W // 2])[0]
        assert len(bar_rows) == 1
        by, bx0, cut = int(bar_rows[0]), tw, u.copy()
        cut[0, (by // th) * th:(by // th + 1) * th, bx0:bx0 + tw] = 0
        assert R.count_components(cut, 8) == 2
        labels, area = R.ref_components(cut, 8)
        starts = [divmod(int(p), W) for p in np.flatnonzero(area[0])]
        start_tiles = {(y // th, x // tw) for y, x in starts}
        assert len(start_tiles) == 2 and (by // th, bx0 // tw) not in start_tiles
    first = {name: int(np.flatnonzero(R.geometry_case(name, th, tw))[0]) % W for name in ("u", "u_lr")}
    assert first["u"] > W // 2 > first["u_lr"]                       # the first pixel is on the right arm in one, the left in the other
    for name in ("corner", "corner_anti"):
        c = R.geometry_case(name, th, tw)
        assert int((c != 0).sum()) == 2 and R.count_components(c, 8) == 1 and R.count_components(c, 4) == 2
        assert len(_tiles_of(c[0], th, tw)) == 2 and _tiles_of(c[0], th, tw) <= {(0, 0), (0, 1), (1, 0), (1, 1)}
    b = R.geometry_case("two_ids_border", th, tw)
    assert R.count_components(b, 8) == 4 and b[0, 0, tw - 1] != b[0, 0, tw] and b[0, 2 * th - 1, 0] != b[0, 2 * th, 0] and b.all()
    assert R.count_components(R.geometry_case("full", th, tw), 4) == 1
    c1 = R.geometry_case("checker_one", th, tw)
    assert R.count_components(c1, 4) == (H * W + 1) // 2 and R.count_components(c1, 8) == 1
    c2 = R.geometry_case("checker_two", th, tw)
    assert R.count_components(c2, 4) == H * W                         # every pixel alone under 4 ...
    labels8, area8 = R.ref_components(c2, 8)
    assert (area8 > 0).sum() == 2                                     # ... and each id ONE diagonal lattice under 8
    t = R.tie_case(th, tw)
    _, area = R.ref_components(t, 8)
    a5 = sorted(area[0][(area[0] > 0) & (t[0] == 5)].tolist())
    assert a5 == [4, 9, 9] and sorted(area[0][(area[0] > 0) & (t[0] == 254)].tolist()) == [2, 6]
    out, removed, _ = R.ref_filter(t, 0, True, 8)
    assert out[0, 2:5, 2:5].all() and not out[0, th - 1:th + 2, tw - 1:tw + 2].any() and removed.tolist() == [9 + 4 + 2]
    rnd = R.striped_random(1, 97, 131, seed=1)
    assert set(np.unique(rnd).tolist()) == {0, 1, 254, 255} and abs(float((rnd != 0).mean()) - 0.59) < 0.02
    _, ar = R.ref_components(rnd, 4)
    big = int(np.argmax(ar[0]))
    assert len(_tiles_of(R.ref_components(rnd, 4)[0][0] == big + 1, th, tw)) >= 2      # ragged components that span tiles


def test_option_plumbing():
    from s2d_amd import ops
    from s2d_amd.evaluate import component_arguments, parse_args
    from s2d_amd.keymask import frame_masks
    from s2d_amd.modeling.postprocess import index_map_options, paint_options
    assert ops.component_options({}) == (0, False, 8)
    assert ops.component_options({"min_component_area": 6, "keep_largest": True, "component_connectivity": 4}) == (6, True, 4)
    for name in ("index_components", "filter_components", "component_options", "component_tile"):
        assert getattr(ops, name).__module__ == "s2d_amd.index_components"
    for bad in ({"min_component_area": -1}, {"min_component_area": 1.5}, {"component_connectivity": 6}):
        for check in (ops.component_options, index_map_options, paint_options):
            with pytest.raises(ValueError):
                check(bad)
    assert index_map_options({"keep_largest": True, "min_component_area": 3}) == ("rank", 20, 0.0)
    assert paint_options({"component_connectivity": 4})[:2] == (50, 0.35)
    base = ["--config-file", "c.yaml", "--video-base-path", "D", "--mask-base-path", "M"]
    a = frame_masks.parse_args(base)
    assert (a.min_component_area, a.keep_largest, a.component_connectivity) == (0, False, 8)
    a = frame_masks.parse_args(base + ["--min-component-area", "6", "--keep-largest", "--component-connectivity", "4"])
    assert (a.min_component_area, a.keep_largest, a.component_connectivity) == (6, True, 4)
    with pytest.raises(SystemExit):
        frame_masks.parse_args(base + ["--component-connectivity", "6"])
    base = ["--config-file", "c.yaml", "--gt", "g", "--image-root", "i", "--output-dir", "o"]
    assert component_arguments(parse_args(base), "ytvis") == {} and component_arguments(parse_args(base), "coco_image") == {}
    assert component_arguments(parse_args(base), "davis") == {"min_component_area": 0, "keep_largest": False, "component_connectivity": 8}
    a = parse_args(base + ["--min-component-area", "6", "--keep-largest", "--component-connectivity", "4"])
    assert component_arguments(a, "davis") == {"min_component_area": 6, "keep_largest": True, "component_connectivity": 4}
    for extra, name in ((["--min-component-area", "6"], "--min-component-area"), (["--keep-largest"], "--keep-largest"),
                        (["--component-connectivity", "8"], "--component-connectivity")):
        for fmt in ("ytvis", "coco_image"):
            with pytest.raises(ValueError, match=name + ".*--test-format " + fmt):
                component_arguments(parse_args(base + extra), fmt)


def test_bad_arguments_are_refused_before_any_launch(dll, tile):
    from s2d_amd._lib import parse_header
    protos = parse_header()
    assert len(protos["s2d_index_components_i32"][0]) == 9 and len(protos["s2d_index_filter_components_u8"][0]) == 13
    assert protos["s2d_index_components_workspace_bytes"][1] == "long" and "s2d_index_components_tile" in protos
    assert dll.s2d_abi_version() == 11
    buf = np.zeros(64, np.int64)                                      # a host address: nothing may be launched on it
    p = buf.ctypes.data
    comp, filt, ws = dll.s2d_index_components_i32, dll.s2d_index_filter_components_u8, dll.s2d_index_components_workspace_bytes
    assert dll.s2d_index_components_tile(None, p) == ERR_ARG and dll.s2d_index_components_tile(p, None) == ERR_ARG
    assert ws(1, 4, 4) >= 4 * 16 + 256 * 8 and ws(3, 4, 4) > ws(1, 4, 4)
    for N, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 46341, 46341), (1, 1, 2 ** 31 - 1)):
        assert ws(N, H, W) == ERR_ARG, (N, H, W)
        assert comp(p, N, H, W, 8, p, p, p, None) == ERR_ARG, (N, H, W)
        assert filt(p, p, p, N, H, W, 0, 0, p, p, p, p, None) == ERR_ARG, (N, H, W)
    for conn in (0, 1, 6, 16, -8):
        assert comp(p, 1, 4, 4, conn, p, p, p, None) == ERR_ARG, conn
    assert comp(None, 1, 4, 4, 8, p, p, p, None) == ERR_ARG and comp(p, 1, 4, 4, 8, None, p, p, None) == ERR_ARG
    assert comp(p, 1, 4, 4, 8, p, p, None, None) == ERR_ARG
    assert comp(p, 1, 4, 4, 8, p + 2, p, p, None) == ERR_ARG and comp(p, 1, 4, 4, 8, p, p + 1, p, None) == ERR_ARG   # misaligned i32
    assert filt(p, p, p, 1, 4, 4, -1, 0, p, p, p, p, None) == ERR_ARG
    for hole in (0, 1, 2, 8, 10, 11):                                 # index, labels, area, out, removed, workspace; rgb (9) may be NULL
        args = [p, p, p, 1, 4, 4, 0, 0, p, p, p, p, None]
        args[hole] = None
        assert filt(*args) == ERR_ARG, hole
    assert not buf.any()
