"""Proposal index maps on the device: `infer_index`, the binding of s2d_infer_index_u8 (csrc/infer.hip).  `s2d_amd.ops` re-exports it
as `ops.infer_index` beside `infer_select` / `infer_masks`.  It is defined here, not in ops.py, because the tables of recorded
entry points in tests/test_gpu_forward_c4.py and tests/test_gpu_eval_720p.py list every function DEFINED in ops.py, and this op is
no part of the scenarios they record: its rows -- exactness against infer_masks, float64, the 2^31 row, the refusals -- are
tests/test_gpu_infer_index.py."""
import torch

INDEX_RULES = {"rank": 0, "prob": 1}
INDEX_MAX_PROPOSALS = 254             # label 255 is DAVIS' void


def infer_index(mask_logits, dims, padded, img_size, out_size, query, score=None, rule="rank"):
    """mask_logits pixel-major [T*hm*wm, ldq]; dims = (T, hm, wm); query int32 [K] and score f32 [K] in proposal order (best
    first, as infer_select returns them) -> index u8 [T,oh,ow]: 0 where no proposal holds the pixel, k + 1 for proposal k.
    rule "rank": the first proposal whose infer_masks plane is set; "prob": among those, the largest score * sigmoid(value),
    ties to the lower k (needs score).  1 <= K <= 254; ldq <= 128 and a multiple of 4.  The [K,T,oh,ow] planes never exist."""
    from . import ops
    from ._lib import lib
    ops._chk(mask_logits); ops._chk(query, torch.int32)
    if rule not in INDEX_RULES:
        raise ValueError(f"index rule {rule!r}: one of {', '.join(INDEX_RULES)}")
    T, hm, wm = dims
    (Hp, Wp), (ih, iw), (oh, ow) = padded, img_size, out_size
    K = query.shape[0] if query.dim() == 1 else -1
    ldq = mask_logits.shape[-1]
    if mask_logits.dim() != 2 or mask_logits.shape[0] != T * hm * wm or not 1 <= K <= INDEX_MAX_PROPOSALS or ldq > 128 or ldq % 4:
        raise ValueError(f"infer_index needs [T*hm*wm, ldq] logits with ldq <= 128 a multiple of 4 and 1 <= K <= {INDEX_MAX_PROPOSALS} "
                         f"proposals, got {tuple(mask_logits.shape)} for dims {tuple(dims)} and query {tuple(query.shape)}")
    if rule == "prob":
        if score is None:
            raise ValueError("index rule 'prob' weighs the proposals by their scores: pass score")
    if score is not None:
        ops._chk(score)
        if tuple(score.shape) != (K,):
            raise ValueError(f"score {tuple(score.shape)} for {K} proposals")
    index = torch.empty((T, oh, ow), device=mask_logits.device, dtype=torch.uint8)
    lib().call("s2d_infer_index_u8", mask_logits, ldq, T, hm, wm, Hp, Wp, ih, iw, oh, ow, query, score, K, INDEX_RULES[rule], index,
               ops._stream())
    return index
