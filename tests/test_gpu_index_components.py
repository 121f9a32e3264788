"""ops.index_components / ops.filter_components (csrc/index_components.hip) against tests/index_components_refs.py.  Every comparison
is an integer equality: labels, area, out, removed and the in-place rgb, for 4- and 8-connectivity, and a second call must be
bitwise equal to the first.  The border and corner cases are built from the tile the library reports."""
import numpy as np
import pytest
import torch

from tests import index_components_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_REF = {}


@pytest.fixture(scope="module")
def tile():
    from s2d_amd import ops
    th, tw = ops.component_tile()
    assert th >= 2 and tw >= 2
    return th, tw


def _ref(key, index, conn):
    """the reference labelling of a named map, computed once"""
    if (key, conn) not in _REF:
        _REF[(key, conn)] = R.ref_components(index, conn)
    return _REF[(key, conn)]


def _offset_view(host, offset):
    """a device copy of `host` that starts `offset` bytes into its allocation"""
    buf = torch.zeros(host.size + offset + 8, dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + host.size].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 4 == (buf.data_ptr() + offset) % 4 and view.is_contiguous()
    return view


def check(key, index, conn, min_area=0, keep_largest=False, offsets=(0, 0), alias=False):
    """labels and area, then the filter with an rgb, each twice; -> (area reference, removed)"""
    from s2d_amd import ops
    index = np.ascontiguousarray(index)
    want_labels, want_area = _ref(key, index, conn)
    rgb0 = R.make_rgb(index, seed=3)
    want_out, want_removed, want_rgb = R.ref_filter(index, min_area, keep_largest, conn, rgb0)
    dev = _offset_view(index, offsets[0])
    runs = []
    for _ in range(2):
        labels, area = ops.index_components(dev, conn)
        runs.append((labels.cpu().numpy(), area.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0], want_labels)
    np.testing.assert_array_equal(runs[0][1], want_area)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    only_labels, none = ops.index_components(dev, conn, want_area=False)
    assert none is None
    np.testing.assert_array_equal(only_labels.cpu().numpy(), want_labels)
    outs = []
    for _ in range(2):
        src = _offset_view(index, offsets[0]) if alias else dev
        dst = src if alias else _offset_view(np.full(index.shape, 77, np.uint8), offsets[1])
        rgb = torch.from_numpy(rgb0).to(DEV)
        out, removed = ops.filter_components(src, min_area, keep_largest, conn, rgb=rgb, out=dst)
        assert out.data_ptr() == dst.data_ptr()
        outs.append((out.cpu().numpy(), removed.cpu().numpy(), rgb.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], want_out)
    np.testing.assert_array_equal(outs[0][1], want_removed)
    np.testing.assert_array_equal(outs[0][2], want_rgb)
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    if not alias:
        np.testing.assert_array_equal(dev.cpu().numpy(), index)       # the input is read only
        plain, removed = ops.filter_components(dev, min_area, keep_largest, conn)       # without rgb, into a new tensor
        np.testing.assert_array_equal(plain.cpu().numpy(), want_out)
        np.testing.assert_array_equal(removed.cpu().numpy(), want_removed)
    return want_area, want_removed


# ------------------------------------------------------------------------------------------------------------ tile-local geometry
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", R.GEOMETRY_CASES)
def test_geometry(tile, name, conn):
    index = R.geometry_case(name, *tile)
    assert index.shape == (1,) + R.frame_shape(*tile)
    area, _ = check(name, index, conn, min_area=3, keep_largest=True)
    print(f"{name} conn {conn}: {int((area > 0).sum())} components")


# ------------------------------------------------------------------------------------------------------------------- edge sizes
def _edge_shapes(th, tw):
    return {"h1": (1, 1, 2 * tw + 5), "w1": (1, 2 * th + 5, 1), "one": (1, 1, 1), "short_wide": (1, th - 1, tw + 1),
            "row": (1, 1, 2 * tw + 3), "column": (1, 2 * th + 3, 1)}


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["h1", "w1", "one", "short_wide", "row", "column"])
def test_edge_sizes(tile, name, conn):
    N, H, W = _edge_shapes(*tile)[name]
    rng = np.random.default_rng(len(name) + H + W)
    index = rng.choice(np.array([0, 1, 254, 255], np.uint8), size=(N, H, W), p=[0.3, 0.3, 0.2, 0.2])
    check(name, index, conn, min_area=2, keep_largest=False)
    check(name, index, conn, min_area=0, keep_largest=True)
    check(name + "_full", np.full((N, H, W), 255, np.uint8), conn, min_area=H * W + 1)


@pytest.mark.parametrize("conn", [4, 8])
def test_three_images_with_an_empty_one_in_the_middle(tile, conn):
    th, tw = tile
    index = R.striped_random(3, th + 5, 2 * tw + 3, seed=2)
    index[1] = 0
    _, removed = check("empty_middle", index, conn, min_area=4, keep_largest=True)
    assert removed[1] == 0 and removed[0] > 0 and removed[2] > 0


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("offsets", [(1, 3), (3, 1), (2, 0)])
def test_views_offset_from_their_allocations(tile, offsets, conn):
    th, tw = tile
    index = R.striped_random(2, th + 3, tw + 7, seed=4)               # H*W odd: the second image starts at another alignment
    check("offsets", index, conn, min_area=5, keep_largest=False, offsets=offsets)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("offset", [0, 1])
def test_out_aliasing_index(tile, offset, conn):
    th, tw = tile
    index = R.striped_random(2, th + 3, tw + 7, seed=4)
    check("offsets", index, conn, min_area=5, keep_largest=True, offsets=(offset, 0), alias=True)


# ------------------------------------------------------------------------------------------------------------------ random maps
@pytest.mark.parametrize("conn", [4, 8])
def test_random_maps_near_the_percolation_threshold(conn):
    index = R.striped_random(3, 97, 131, seed=7)
    area, removed = check("random_97x131", index, conn, min_area=12, keep_largest=False)
    assert (removed > 0).all() and int(area.max()) > 200
    check("random_97x131", index, conn, min_area=0, keep_largest=True)


@pytest.mark.parametrize("conn", [4, 8])
def test_one_frame_of_480_by_854(conn):
    index = R.striped_random(1, 480, 854, seed=8, stripe=151)
    area, removed = check("random_480x854", index, conn, min_area=30, keep_largest=True)
    print(f"480 x 854 conn {conn}: {int((area > 0).sum())} components, largest {int(area.max())}, removed {int(removed[0])}")


# ------------------------------------------------------------------------------------------------------------------- filter rule
@pytest.mark.parametrize("conn", [4, 8])
def test_filter_rule(tile, conn):
    from s2d_amd import ops
    th, tw = tile
    index = R.tie_case(th, tw)
    # off: the input comes back and nothing is removed
    _, removed = check("tie", index, conn, 0, False)
    assert removed.tolist() == [0]
    dev = torch.from_numpy(index).to(DEV)
    out, _ = ops.filter_components(dev, 0, False, conn)
    assert torch.equal(out, dev)
    # a min_area equal to a component's area keeps it, one more removes it (id 5: 9, 9, 4; id 254: 6, 2)
    assert check("tie", index, conn, 9, False)[1].tolist() == [4 + 6 + 2]
    assert check("tie", index, conn, 10, False)[1].tolist() == [9 + 9 + 4 + 6 + 2]
    assert check("tie", index, conn, 6, False)[1].tolist() == [4 + 2]
    assert check("tie", index, conn, 7, False)[1].tolist() == [4 + 6 + 2]
    # keep_largest: of the two components of 9 pixels the one with the lower first pixel stays
    check("tie", index, conn, 0, True)
    out, removed = ops.filter_components(dev, 0, True, conn)
    out = out.cpu().numpy()
    assert removed.tolist() == [9 + 4 + 2] and (out[0, 2:5, 2:5] == 5).all() and not out[0, th - 1:th + 2, tw - 1:tw + 2].any()
    # ... and the mirrored map keeps the other blob: the rule looks at the first pixel, not at the blob
    flipped = np.ascontiguousarray(index[:, ::-1, ::-1])
    check("tie_flipped", flipped, conn, 0, True)
    # keep_largest with a min_area above the largest area of an id removes the whole id
    assert check("tie", index, conn, 7, True)[1].tolist() == [9 + 4 + 6 + 2]
    assert check("tie", index, conn, 10, True)[1].tolist() == [int((index != 0).sum())]


def test_refusals():
    from s2d_amd import ops
    good = torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.index_components(torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.filter_components(torch.zeros((1, 4, 4), dtype=torch.uint8), 1)
    with pytest.raises(RuntimeError):
        ops.index_components(good.to(torch.int32))
    for bad in (lambda: ops.index_components(good, 6), lambda: ops.index_components(good[0]), lambda: ops.filter_components(good, -1),
                lambda: ops.filter_components(good, 1, rgb=torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV)),
                lambda: ops.filter_components(good, 1, out=torch.zeros((1, 4, 5), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            bad()
