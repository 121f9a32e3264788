"""Size refusals of the eval-side post-processing (csrc/infer.hip, window.hip, rle.hip), DESIGN.md "Eval path at 720p video lengths":
where a kernel's index arithmetic is 32-bit, the C ABI answers S2D_ERR_ARG from its argument checks, before the first launch.  No device
is needed or touched: every pointer is null, so anything but the argument check would not return S2D_ERR_ARG.  The library itself must
have been built (`build()`): these are calls into libs2d_hip.so.  check_clip_size is plain python: the one-clip path's refusal of a clip
whose 1/4-resolution activations the dense kernels cannot address, raised before the network is called."""
import pytest

ERR_ARG = -1


def _code(name, *args):
    from s2d_amd._lib import lib
    with pytest.raises(RuntimeError) as e:
        lib().call(name, *args)
    return str(e.value)


@pytest.mark.parametrize("name,args", [
    # the shared rows of two windows: n = O * hm * wm pixel rows, 32-bit in the pass structure
    ("s2d_window_pair_counts", (None, None, 1 << 31, 100, 100, None, None, None, None)),
    # run positions x * H + y are int32: one frame has fewer than 2^31 pixels
    ("s2d_rle_count_u8", (None, 1, 46341, 46341, None, None, None, None, None)),
    ("s2d_rle_positions_u8", (None, 1, 46341, 46341, None, None, None, None)),
    ("s2d_rle_strings_u8", (None, None, 1, 1 << 31, 2, None, 0, None, None, None)),
    # character offsets are int32: at most 7 characters per run
    ("s2d_rle_strings_u8", (None, None, 1, 921600, (1 << 31) // 7 + 1, None, 0, None, None, None)),
    # one workgroup per 256 elements along grid x
    ("s2d_pack_mask_bits_u8", (None, 1, 1 << 40, None, None)),
])
def test_refused_with_err_arg_before_a_launch(name, args):
    assert f"{name} failed with code {ERR_ARG}" in _code(name, *args)


def test_one_clip_refusal_names_window_inference():
    """720p (padded 736 x 1280): [T * 184 * 320, 256] f32 is T * 60 293 120 bytes; 71 frames fit under 0xFFFFFF00, 72 do not"""
    from s2d_amd.modeling.window_inference import GEMM_OPERAND_BYTES, check_clip_size
    assert 71 * 184 * 320 * 256 * 4 <= GEMM_OPERAND_BYTES < 72 * 184 * 320 * 256 * 4
    for T in (1, 16, 36, 64, 71):
        check_clip_size(T, 736, 1280)
    for T in (72, 128, 1 << 20):
        with pytest.raises(ValueError, match="WINDOW_INFERENCE"):
            check_clip_size(T, 736, 1280)
    check_clip_size(284, 368, 640)                                  # 360p: four times as many frames
    with pytest.raises(ValueError, match="WINDOW_INFERENCE"):
        check_clip_size(285, 368, 640)


def test_inference_refuses_before_the_network_is_called():
    """_inference on a 72-frame 720p clip (a meta tensor: no memory, no device) raises before `net` is touched"""
    import torch
    from s2d_amd.modeling.meta_arch import _inference

    def net(*a, **k):
        raise AssertionError("the network was called")
    images = torch.empty((72, 736, 1280, 4), device="meta")
    with pytest.raises(ValueError, match="WINDOW_INFERENCE"):
        _inference(net, images, [{"image": [torch.empty((3, 720, 1280), device="meta")]}], 10, False, 0.75)
    with pytest.raises(ValueError, match="WINDOW_INFERENCE"):      # a window that is itself too long
        _inference(net, images[:200], [{"image": [torch.empty((3, 720, 1280), device="meta")]}], 10, False, 0.75, window=(100, 2))
