"""The host reference of the hole filling (tests/index_fill_refs.py) against an independent flood fill, the properties the rule
promises, the constructed cases against the property each is named for, the option plumbing of both drivers, and the argument
refusals of the C ABI (returned before any launch, so no GPU is needed)."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

from tests import index_components_refs as C
from tests import index_fill_refs as R

ERR_ARG = -1                                                                   # S2D_ERR_ARG
ALL = 2 ** 31 - 1


def flood_fill_holes(index, max_area, conn):
    """pure Python: every unvisited zero pixel floods its component under the complementary connectivity and collects, on the way,
    whether it met the frame border and the ids it touched"""
    N, H, W = index.shape
    near = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 4 else [])
    out, filled = index.copy(), np.zeros(N, np.int32)
    for n in range(N):
        seen = np.zeros((H, W), bool)
        for y in range(H):
            for x in range(W):
                if index[n, y, x] or seen[y, x]:
                    continue
                stack, comp, owners, border = [(y, x)], [], set(), False
                seen[y, x] = True
                while stack:
                    cy, cx = stack.pop()
                    comp.append((cy, cx))
                    border |= cy in (0, H - 1) or cx in (0, W - 1)
                    for dy, dx in near:
                        ny, nx = cy + dy, cx + dx
                        if not (0 <= ny < H and 0 <= nx < W):
                            continue
                        if index[n, ny, nx]:
                            owners.add(int(index[n, ny, nx]))
                        elif not seen[ny, nx]:
                            seen[ny, nx] = True
                            stack.append((ny, nx))
                if not border and len(owners) == 1 and len(comp) <= max_area:
                    for cy, cx in comp:
                        out[n, cy, cx] = next(iter(owners))
                    filled[n] += len(comp)
    return out, filled


def _random_maps(seed, count, ids=(0, 1, 2, 255), p=(0.15, 0.55, 0.2, 0.1)):
    rng = np.random.default_rng(seed)
    shapes = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (5, 7), (12, 12), (11, 13))
    return [rng.choice(np.array(ids, np.uint8), size=(2,) + shapes[i % len(shapes)], p=p) for i in range(count)]


@pytest.fixture(scope="module")
def dll():
    from s2d_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.s2d_index_components_tile.argtypes = [P, P]
    lib.s2d_index_fill_holes_workspace_bytes.argtypes = [I, I, I]
    lib.s2d_index_fill_holes_workspace_bytes.restype = ctypes.c_long
    lib.s2d_index_fill_holes_u8.argtypes = [P, I, I, I, I, I, P, P, P, I, P, P, P]
    return lib


@pytest.fixture(scope="module")
def tile(dll):
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    assert dll.s2d_index_components_tile(ctypes.addressof(th), ctypes.addressof(tw)) == 0
    assert th.value >= 12 and tw.value >= 12                                 # the constructed cases need this much room in a tile
    return th.value, tw.value


@pytest.mark.parametrize("conn", [4, 8])
def test_reference_equals_flood_fill_on_small_maps(conn):
    maps = _random_maps(5, 24) + [np.zeros((1, 4, 4), np.uint8), C.full_frame(3, 5), R.frame_ring(5, 6), R.frame_ring(3, 3, 255)]
    hits = 0
    for m in maps:
        for max_area in (1, 2, ALL):
            want = flood_fill_holes(m, max_area, conn)
            got = R.ref_fill_holes(m, max_area, conn)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
            hits += int(want[1].sum() > 0)
    assert hits >= 6
    assert np.array_equal(R.ref_fill_holes(maps[0], "all", conn)[0], R.ref_fill_holes(maps[0], ALL, conn)[0])


def test_reference_on_a_hand_made_map():
    m = np.array([[[1, 1, 1, 1, 1, 2, 2],
                   [1, 0, 1, 1, 0, 2, 2],
                   [1, 1, 0, 1, 1, 0, 2],
                   [1, 1, 1, 1, 1, 2, 2],
                   [1, 0, 1, 1, 1, 2, 0]]], np.uint8)
    # instances 8-connected: zeros join by 4.  (1,1), (2,2) are two holes of id 1; (1,4) touches 1 and 2; (2,5) too; (4,1), (4,6): border
    colors = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    out, filled, rgb = R.ref_fill_holes(m, ALL, 8, C.make_rgb(m), colors)
    want = m.copy()
    want[0, 1, 1] = want[0, 2, 2] = 1
    assert np.array_equal(out, want) and filled.tolist() == [2]
    assert rgb[0, 1, 1].tolist() == [10, 20, 30] and rgb[0, 2, 2].tolist() == [10, 20, 30] and rgb[0, 1, 4].tolist() == [7, 7, 7]
    # instances 4-connected: zeros join by 8.  {(1,1), (2,2)} is one hole of 2 owned by 1; {(1,4), (2,5)} one of 2 with two owners
    out, filled, _ = R.ref_fill_holes(m, ALL, 4)
    assert np.array_equal(out, want) and filled.tolist() == [2]
    assert R.ref_fill_holes(m, 1, 4)[1].tolist() == [0] and R.ref_fill_holes(m, 1, 8)[1].tolist() == [2]
    # a colour table that ends before the owner: the hole is left alone in both outputs
    out, filled, rgb = R.ref_fill_holes(np.where(m == 1, 3, m).astype(np.uint8), ALL, 8, C.make_rgb(m), colors)
    assert filled.tolist() == [0] and out[0, 1, 1] == 0 and rgb[0, 1, 1].tolist() == [7, 7, 7]


@pytest.mark.parametrize("conn", [4, 8])
def test_properties_of_the_rule(conn):
    """idempotent; no id gains a component; the smallest component area never drops; only zero pixels change; on a single-id map
    with "all" it is scipy's binary_fill_holes under the complementary structure"""
    maps = _random_maps(9, 40) + _random_maps(10, 16, ids=(0, 7), p=(0.35, 0.65)) + \
        [C.striped_random(1, 40, 50, seed=3, stripe=9, density=0.8)]
    changed = 0
    for m in maps:
        for max_area in (1, 3, ALL):
            out, filled, _ = R.ref_fill_holes(m, max_area, conn)
            again, filled2, _ = R.ref_fill_holes(out, max_area, conn)
            assert np.array_equal(again, out) and not filled2.any()
            assert ((out == m) | (m == 0)).all() and ((out != m).reshape(len(m), -1).sum(1) == filled).all()
            for n in range(len(m)):
                a0, a1 = C.ref_components(m[n:n + 1], conn)[1], C.ref_components(out[n:n + 1], conn)[1]
                for v in np.unique(m[n]):
                    if v:
                        sel0, sel1 = a0[0][(a0[0] > 0) & (m[n] == v)], a1[0][(a1[0] > 0) & (out[n] == v)]
                        assert len(sel1) <= len(sel0) and sel1.min() >= sel0.min()
                assert set(np.unique(out[n])) <= set(np.unique(m[n]))
            changed += int(filled.sum() > 0)
    assert changed >= 10
    for m in _random_maps(10, 16, ids=(0, 7), p=(0.35, 0.65)):
        out, _, _ = R.ref_fill_holes(m, "all", conn)
        for n in range(len(m)):
            want = ndimage.binary_fill_holes(m[n] != 0, C.structure(R.hole_conn(conn)))
            assert np.array_equal(out[n] != 0, want) and set(np.unique(out[n])) <= {0, 7}


def _filled_mask(m, max_area, conn):
    return (R.ref_fill_holes(m, max_area, conn)[0] != m)[0]


def test_named_cases_have_the_property_they_are_named_for(tile):
    th, tw = tile
    H, W = R.frame_shape(th, tw)
    for name in R.GEOMETRY_CASES:
        assert R.geometry_case(name, th, tw).shape == (1, H, W), name
    for conn in (4, 8):
        assert [(a, o) for _, a, o in R.holes(R.geometry_case("one_pixel", th, tw)[0], conn)] == [(1, [3])]
        for where, tiles in (("vertical", {(0, 0), (0, 1)}), ("horizontal", {(0, 0), (1, 0)}),
                             ("corner", {(0, 0), (0, 1), (1, 0), (1, 1)})):
            m = R.geometry_case("cross_" + where, th, tw)
            (comp, area, owners), = R.holes(m[0], conn)
            ys, xs = np.nonzero(comp)
            assert area == 9 and owners == [9] and {(int(y) // th, int(x) // tw) for y, x in zip(ys, xs)} == tiles
        for side in ("top", "bottom", "left", "right"):
            m = R.geometry_case("border_" + side, th, tw)
            assert int((m == 0).sum()) == 3 and R.holes(m[0], conn) == [] and not _filled_mask(m, ALL, conn).any()
            inner = m.copy()                                          # one pixel shorter, it is a hole: only the border pixel decides
            inner[0, 0, :][m[0, 0, :] == 0] = 6
            inner[0, -1, :][m[0, -1, :] == 0] = 6
            inner[0, :, 0][m[0, :, 0] == 0] = 6
            inner[0, :, -1][m[0, :, -1] == 0] = 6
            assert [(a, o) for _, a, o in R.holes(inner[0], conn)] == [(2, [6])]
        m = R.geometry_case("area_pair", th, tw)
        assert sorted(a for _, a, _ in R.holes(m[0], conn)) == [6, 7]
        assert R.ref_fill_holes(m, 6, conn)[1].tolist() == [6] and R.ref_fill_holes(m, 7, conn)[1].tolist() == [13]
        assert R.ref_fill_holes(m, 5, conn)[1].tolist() == [0]
        m = R.geometry_case("two_owners", th, tw)
        assert [(a, o) for _, a, o in R.holes(m[0], conn)] == [(6, [1, 2])] and not _filled_mask(m, ALL, conn).any()
        m = R.geometry_case("island", th, tw)
        assert sorted((a, tuple(o)) for _, a, o in R.holes(m[0], conn)) == [(1, (2,)), (81 - 25, (1, 2))]
        out, filled, _ = R.ref_fill_holes(m, ALL, conn)
        assert filled.tolist() == [1] and out[0, th, tw] == 2 and int((out == 0).sum()) == 81 - 25
        m = R.geometry_case("owner_ids", th, tw)
        assert sorted((a, tuple(o)) for _, a, o in R.holes(m[0], conn)) == [(1, (1,)), (1, (254,)), (1, (255,))]
        table = R.color_table(254)
        assert len({tuple(r) for r in table.tolist()}) == 254 and (table >= 8).all()
        out, filled, rgb = R.ref_fill_holes(m, ALL, conn, C.make_rgb(m), table)
        assert filled.tolist() == [2] and out[0, 16, 4] == 0 and out[0, 10, 4] == 254 and rgb[0, 10, 4].tolist() == table[253].tolist()
        assert R.ref_fill_holes(m, ALL, conn)[1].tolist() == [3]
        sp = R.geometry_case("spiral_hole", th, tw)
        (comp, area, owners), = R.holes(sp[0], conn)
        ys, xs = np.nonzero(comp)
        assert owners == [7] and area > 2 * (H + W) and {(int(y) // th, int(x) // tw) for y, x in zip(ys, xs)} >= \
            {(i, j) for i in range(3) for j in range(3)}
        assert not (comp[:-1, :-1] & comp[1:, :-1] & comp[:-1, 1:] & comp[1:, 1:]).any()      # one pixel wide
        ring = R.frame_ring(9, 11)
        assert [(a, o) for _, a, o in R.holes(ring[0], conn)] == [(7 * 9, [1])]
    # the complementary connectivity: diagonal zeros are one hole where the instances are 4-connected, two where they are 8-connected
    for name in ("diagonal", "corner_diagonal", "corner_anti"):
        m = R.geometry_case(name, th, tw)
        assert sorted(a for _, a, _ in R.holes(m[0], 4)) == [2] and sorted(a for _, a, _ in R.holes(m[0], 8)) == [1, 1]
        assert R.ref_fill_holes(m, 1, 4)[1].tolist() == [0] and R.ref_fill_holes(m, 1, 8)[1].tolist() == [2]
    m = R.geometry_case("diagonal_owner", th, tw)
    assert [(a, o) for _, a, o in R.holes(m[0], 8)] == [(1, [1])] and [(a, o) for _, a, o in R.holes(m[0], 4)] == [(1, [1, 2])]
    assert R.ref_fill_holes(m, ALL, 8)[1].tolist() == [1] and R.ref_fill_holes(m, ALL, 4)[1].tolist() == [0]
    for name in ("corner_diagonal", "corner_anti"):
        ys, xs = np.nonzero(R.geometry_case(name, th, tw)[0] == 0)
        assert len({(int(y) // th, int(x) // tw) for y, x in zip(ys, xs)}) == 2
    b = R.blobs_with_speckle(120, 160, seed=1)
    assert b.shape == (1, 120, 160) and len(np.unique(b)) > 5
    cleaned = C.ref_filter(b, 6, True, 8)[0]
    assert R.ref_fill_holes(cleaned, ALL, 8)[1][0] > 0                 # the cleanup leaves holes, and the fill closes some


def test_option_plumbing():
    from s2d_amd import index_components, ops
    from s2d_amd.evaluate import component_arguments, fill_arguments, parse_args
    from s2d_amd.keymask import frame_masks
    from s2d_amd.modeling.postprocess import index_map_options, paint_options
    assert ops.fill_options({}) == 0 and ops.fill_options({"fill_holes": 0}) == 0 and ops.fill_options({"fill_holes": 9}) == 9
    assert ops.fill_options({"fill_holes": "all"}) == ALL and ops.fill_options({"fill_holes": ALL}) == ALL
    assert index_components.FILL_KEYS == ("fill_holes",)
    assert index_components.COMPONENT_KEYS == ("min_component_area", "keep_largest", "component_connectivity")
    assert ops.component_options({"fill_holes": 3}) == (0, False, 8)
    for name in ("fill_index_holes", "fill_options"):
        assert getattr(ops, name).__module__ == "s2d_amd.index_components"
    for bad in (True, False, -1, 1.5, 2.0, "some", None, ALL + 1):
        for check in (ops.fill_options, index_map_options, paint_options):
            with pytest.raises(ValueError):
                check({"fill_holes": bad})
    assert index_map_options({"fill_holes": "all", "min_component_area": 3}) == ("rank", 20, 0.0)
    assert paint_options({"fill_holes": 4})[:2] == (50, 0.35)
    for check, known in ((index_map_options, "rule, max_proposals, score_threshold"), (paint_options, "max_masks, score_threshold, colors")):
        with pytest.raises(ValueError, match=known + " and min_component_area, keep_largest, component_connectivity are known.*fill_holes"):
            check({"fill_hole": 1})
    base = ["--config-file", "c.yaml", "--video-base-path", "D", "--mask-base-path", "M"]
    assert frame_masks.parse_args(base).fill_holes == 0
    assert frame_masks.parse_args(base + ["--fill-holes", "12"]).fill_holes == 12
    assert frame_masks.parse_args(base + ["--fill-holes", "all"]).fill_holes == ALL
    for bad in ("-1", "x", "1.5"):
        with pytest.raises(SystemExit):
            frame_masks.parse_args(base + ["--fill-holes", bad])
    base = ["--config-file", "c.yaml", "--gt", "g", "--image-root", "i", "--output-dir", "o"]
    assert fill_arguments(parse_args(base), "ytvis") == {} and fill_arguments(parse_args(base), "coco_image") == {}
    assert fill_arguments(parse_args(base), "davis") == {"fill_holes": 0}
    assert fill_arguments(parse_args(base + ["--fill-holes", "5"]), "davis") == {"fill_holes": 5}
    assert ops.fill_options(fill_arguments(parse_args(base + ["--fill-holes", "all"]), "davis")) == ALL
    a = parse_args(base + ["--fill-holes", "all"])
    assert component_arguments(a, "davis") == {"min_component_area": 0, "keep_largest": False, "component_connectivity": 8}
    assert component_arguments(a, "ytvis") == {}                       # the fill flag is fill_arguments' to refuse
    for fmt in ("ytvis", "coco_image"):
        with pytest.raises(ValueError, match="--fill-holes.*--test-format " + fmt):
            fill_arguments(a, fmt)
    with pytest.raises(SystemExit):
        parse_args(base + ["--fill-holes", "-3"])


def test_bad_arguments_are_refused_before_any_launch(dll):
    from s2d_amd._lib import parse_header
    protos = parse_header()
    assert len(protos["s2d_index_fill_holes_workspace_bytes"][0]) == 3 and protos["s2d_index_fill_holes_workspace_bytes"][1] == "long"
    assert len(protos["s2d_index_fill_holes_u8"][0]) == 13
    assert len(protos["s2d_index_components_i32"][0]) == 9 and len(protos["s2d_index_filter_components_u8"][0]) == 13
    assert dll.s2d_abi_version() == 11
    buf = np.zeros(64, np.int64)                                      # a host address: nothing may be launched on it
    p = buf.ctypes.data
    fill, ws = dll.s2d_index_fill_holes_u8, dll.s2d_index_fill_holes_workspace_bytes
    good = [p, 1, 4, 4, 8, 1, p, p, p, 3, p, p, None]
    assert ws(1, 4, 4) >= 16 * 16 and ws(3, 4, 4) > ws(1, 4, 4)
    for N, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 46341, 46341), (1, 1, 2 ** 31 - 1)):
        assert ws(N, H, W) == ERR_ARG, (N, H, W)
        args = list(good)
        args[1:4] = [N, H, W]
        assert fill(*args) == ERR_ARG, (N, H, W)
    for conn in (0, 1, 6, 16, -8):
        args = list(good)
        args[4] = conn
        assert fill(*args) == ERR_ARG, conn
    for area in (0, -1, -(2 ** 31)):
        args = list(good)
        args[5] = area
        assert fill(*args) == ERR_ARG, area
    for hole in (0, 6, 8, 10, 11):                                    # index, out, colors (with rgb), filled, workspace
        args = list(good)
        args[hole] = None
        assert fill(*args) == ERR_ARG, hole
    for n_colors in (0, -1, 256, 1000):                               # with rgb given
        args = list(good)
        args[9] = n_colors
        assert fill(*args) == ERR_ARG, n_colors
    for off in (1, 2, 3):                                             # a misaligned filled
        args = list(good)
        args[10] = p + off
        assert fill(*args) == ERR_ARG, off
    assert not buf.any()
