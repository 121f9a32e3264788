"""ops.fill_index_holes (csrc/index_components.hip) against tests/index_fill_refs.py.  Every comparison is an integer equality: out,
filled and the in-place rgb, for instances of 4- and 8-connectivity; every call is made twice and must be bitwise equal, and the
input is untouched where out is not index.  The border and corner cases are built from the tile the library reports."""
import numpy as np
import pytest
import torch

from tests import index_components_refs as C
from tests import index_fill_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = 2 ** 31 - 1
TABLE = R.color_table(254)                                            # owner 255 has no colour: skipped with rgb, filled without


@pytest.fixture(scope="module")
def tile():
    from s2d_amd import ops
    th, tw = ops.component_tile()
    assert th >= 12 and tw >= 12
    return th, tw


def _offset_view(host, offset):
    """a device copy of `host` that starts `offset` bytes into its allocation"""
    buf = torch.zeros(host.size + offset + 8, dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 4 == (buf.data_ptr() + offset) % 4 and view.is_contiguous()
    return view


def check(index, conn, max_area=ALL, offsets=(0, 0), alias=False, colors=TABLE):
    """with an rgb, twice, then without one into a new tensor -> (out, filled) of the reference WITHOUT rgb"""
    from s2d_amd import ops
    index = np.ascontiguousarray(index)
    rgb0 = C.make_rgb(index, seed=3)
    want_out, want_filled, want_rgb = R.ref_fill_holes(index, max_area, conn, rgb0, colors)
    table = torch.from_numpy(colors).to(DEV)
    dev = _offset_view(index, offsets[0])
    runs = []
    for _ in range(2):
        src = _offset_view(index, offsets[0]) if alias else dev
        dst = src if alias else _offset_view(np.full(index.shape, 77, np.uint8), offsets[1])
        rgb = torch.from_numpy(rgb0).to(DEV)
        out, filled = ops.fill_index_holes(src, "all" if max_area == ALL else max_area, conn, rgb=rgb, colors=table, out=dst)
        assert out.data_ptr() == dst.data_ptr() and filled.dtype == torch.int32 and tuple(filled.shape) == (index.shape[0],)
        runs.append((out.cpu().numpy(), filled.cpu().numpy(), rgb.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0], want_out)
    np.testing.assert_array_equal(runs[0][1], want_filled)
    np.testing.assert_array_equal(runs[0][2], want_rgb)
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
    np.testing.assert_array_equal(dev.cpu().numpy(), index)           # the input is read only
    plain_out, plain_filled, _ = R.ref_fill_holes(index, max_area, conn)
    out, filled = ops.fill_index_holes(dev, max_area, conn)           # without rgb, into a new tensor
    np.testing.assert_array_equal(out.cpu().numpy(), plain_out)
    np.testing.assert_array_equal(filled.cpu().numpy(), plain_filled)
    assert (((plain_out == index) | (index == 0)).all())              # nothing but zero pixels changes
    return plain_out, plain_filled


# ------------------------------------------------------------------------------------------------------------ constructed cases
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", R.GEOMETRY_CASES)
def test_geometry(tile, name, conn):
    index = R.geometry_case(name, *tile)
    assert index.shape == (1,) + R.frame_shape(*tile)
    out, filled = check(index, conn)
    print(f"{name} conn {conn}: filled {int(filled[0])} of {int((index == 0).sum())} zero pixels")
    if name.startswith("border_") or name == "two_owners":
        assert filled.tolist() == [0] and np.array_equal(out, index)
    elif name == "diagonal_owner":
        assert filled.tolist() == [1 if conn == 8 else 0]             # the owners are taken under the holes' connectivity
    elif name == "island":
        assert filled.tolist() == [1] and int((out == 0).sum()) == 81 - 25
    elif name == "owner_ids":
        assert filled.tolist() == [3]                                 # without rgb the 255 hole is filled too ...
        with_rgb = R.ref_fill_holes(index, ALL, conn, C.make_rgb(index, seed=3), TABLE)
        assert with_rgb[1].tolist() == [2]                            # ... with the 254-row table it is skipped (compared in check)
    else:
        assert filled[0] == (index == 0).sum() and out.all()


@pytest.mark.parametrize("conn", [4, 8])
def test_area_bound(tile, conn):
    index = R.geometry_case("area_pair", *tile)                       # holes of 6 and 7 pixels
    assert check(index, conn, 6)[1].tolist() == [6]
    assert check(index, conn, 7)[1].tolist() == [13]
    assert check(index, conn, 5)[1].tolist() == [0]
    diag = R.geometry_case("diagonal", *tile)                         # one hole of 2 where the zeros join by 8, two of 1 where by 4
    assert check(diag, conn, 1)[1].tolist() == [0 if conn == 4 else 2]
    assert check(diag, conn, 2)[1].tolist() == [2]


# ------------------------------------------------------------------------------------------------------------------- edge sizes
@pytest.mark.parametrize("conn", [4, 8])
def test_edge_sizes(tile, conn):
    th, tw = tile
    for shape in ((1, 1, 1), (1, 1, 2 * tw + 5), (1, 2 * th + 5, 1), (1, 2, 2), (1, 3, 3)):
        rng = np.random.default_rng(sum(shape))
        check(rng.choice(np.array([0, 1, 255], np.uint8), size=shape, p=[0.4, 0.4, 0.2]), conn)
        check(np.zeros(shape, np.uint8), conn)
        check(np.full(shape, 255, np.uint8), conn)
    assert check(R.frame_ring(3, 3, 255), conn)[1].tolist() == [1]    # the smallest frame that holds a hole
    assert check(R.frame_ring(3, 3, 255), conn, colors=R.color_table(255))[0].all()
    H, W = R.frame_shape(th, tw)
    assert check(np.zeros((1, H, W), np.uint8), conn)[1].tolist() == [0]             # an all-zero map: one component, on the border
    assert check(np.full((1, H, W), 9, np.uint8), conn)[1].tolist() == [0]           # a map without a zero


@pytest.mark.parametrize("conn", [4, 8])
def test_three_images_with_an_all_zero_one_in_the_middle(tile, conn):
    th, tw = tile
    index = C.striped_random(3, th + 5, 2 * tw + 3, seed=2, density=0.85, stripe=23)
    index[1] = 0
    _, filled = check(index, conn)
    assert filled[1] == 0 and filled[0] > 0 and filled[2] > 0


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("offsets", [(1, 3), (3, 1), (2, 0)])
def test_views_offset_from_their_allocations(tile, offsets, conn):
    th, tw = tile
    # H*W odd: the second image starts at another alignment
    index = C.striped_random(2, th + 3, tw + 7, seed=4, density=0.85, stripe=23)
    _, filled = check(index, conn, 4, offsets=offsets)
    assert (filled > 0).all()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("offset", [0, 1])
def test_out_aliasing_index(tile, offset, conn):
    th, tw = tile
    index = C.striped_random(2, th + 3, tw + 7, seed=4, density=0.85, stripe=23)
    check(index, conn, offsets=(offset, 0), alias=True)


# ------------------------------------------------------------------------------------------------------------------ full frames
@pytest.mark.parametrize("conn", [4, 8])
def test_frame_sized_ring_of_480_by_854(conn):
    """ONE hole of (H-2)(W-2) pixels whose every boundary pixel reports to one root: the contention case"""
    index = R.frame_ring(480, 854, 200)
    want = np.full((1, 480, 854), 200, np.uint8)
    out, filled = check(index, conn)
    assert filled.tolist() == [478 * 852] and np.array_equal(out, want)


@pytest.fixture(scope="module")
def speckled():
    """one 480 x 854 frame of seeded blobs with 1 % speckle, and what the reference filter makes of it"""
    index = R.blobs_with_speckle(480, 854, n_blobs=20, speckle=0.01, seed=6)
    return index, {conn: C.ref_filter(index, 6, True, conn)[0] for conn in (4, 8)}


@pytest.mark.parametrize("conn", [4, 8])
def test_filter_then_fill_on_480_by_854(speckled, conn):
    from s2d_amd import ops
    index, cleaned = speckled
    dev = torch.from_numpy(index).to(DEV)
    mid, removed = ops.filter_components(dev, 6, True, conn)
    np.testing.assert_array_equal(mid.cpu().numpy(), cleaned[conn])
    want_out, want_filled, _ = R.ref_fill_holes(cleaned[conn], ALL, conn)
    runs = []
    for _ in range(2):
        out, filled = ops.fill_index_holes(mid, "all", conn)
        runs.append((out.cpu().numpy(), filled.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0], want_out)
    np.testing.assert_array_equal(runs[0][1], want_filled)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(mid.cpu().numpy(), cleaned[conn])
    small, few = ops.fill_index_holes(mid, 1, conn, out=mid)          # a bound, in place
    want_small, want_few, _ = R.ref_fill_holes(cleaned[conn], 1, conn)
    np.testing.assert_array_equal(small.cpu().numpy(), want_small)
    np.testing.assert_array_equal(few.cpu().numpy(), want_few)
    print(f"480 x 854 conn {conn}: removed {int(removed[0])}, filled {int(want_filled[0])} (holes of 1: {int(want_few[0])})")
    assert 0 < want_few[0] < want_filled[0] and removed[0] > 0


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from s2d_amd import ops
    good = torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV)
    rgb = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=DEV)
    table = torch.zeros((3, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.fill_index_holes(torch.zeros((1, 4, 4), dtype=torch.uint8), 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.fill_index_holes(good, 1, rgb=rgb, colors=torch.zeros((3, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.fill_index_holes(good.to(torch.int32), 1)
    fill, u8 = ops.fill_index_holes, dict(dtype=torch.uint8, device=DEV)
    for bad in (lambda: fill(good, 0), lambda: fill(good, -1), lambda: fill(good, True),
                lambda: fill(good, 1.5), lambda: fill(good, "some"), lambda: fill(good, 2 ** 31),
                lambda: fill(good, 1, 6), lambda: fill(good[0], 1),
                lambda: fill(good, 1, rgb=rgb), lambda: fill(good, 1, rgb=torch.zeros((1, 4, 4, 2), **u8), colors=table),
                lambda: fill(good, 1, rgb=rgb, colors=torch.zeros((3, 2), **u8)),
                lambda: fill(good, 1, rgb=rgb, colors=torch.zeros((256, 3), **u8)),
                lambda: fill(good, 1, out=torch.zeros((1, 4, 5), **u8))):
        with pytest.raises(ValueError):
            bad()
    out, filled = ops.fill_index_holes(good, "all", rgb=rgb, colors=table)
    assert not out.any() and filled.tolist() == [0] and not rgb.any()
