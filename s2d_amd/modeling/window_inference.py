"""Windowed inference of a long video (MODEL.MASK_FORMER.TEST.WINDOW_INFERENCE; DESIGN.md section 1, "Windowed inference").

The network runs on windows of W frames that share O frames with their neighbour; the queries of consecutive windows are
associated by the IoU of their binary masks on the shared frames, and every window's owned rows are written, columns permuted
into track order, into one pixel-major mask-logit buffer [T*hm*wm, ldq] that `inference_video` reads like the output of a single
clip.  Everything between two windows runs on the device (csrc/window.hip, the matcher's assignment solver and a few torch ops on
Q-element tensors); nothing is read back."""
import torch

from .. import ops

MAX_WINDOW_QUERIES = 113      # the device solver takes Q * Nmax <= 12800 (s2d_lsap_f32), and the association is Q x Q


def check_window_config(enabled, size, overlap, num_queries=None):
    """refuse, as ValueError, window keys the stitching cannot take: W <= 0, O < 1 or O >= W with the switch on"""
    if not enabled:
        return
    W, O = int(size), int(overlap)
    if W <= 0:
        raise ValueError(f"TEST.WINDOW_SIZE = {W}: windowed inference needs a positive number of frames per window")
    if O < 1 or O >= W:
        raise ValueError(f"TEST.WINDOW_OVERLAP = {O}: consecutive windows share 1 <= O < WINDOW_SIZE = {W} frames")
    if num_queries is not None and int(num_queries) > MAX_WINDOW_QUERIES:
        raise ValueError(f"TEST.WINDOW_INFERENCE with NUM_OBJECT_QUERIES = {num_queries}: the Q x Q association takes at most "
                         f"{MAX_WINDOW_QUERIES} queries")


GEMM_OPERAND_BYTES = 0xFFFFFF00   # s2d_gemm_nt_f32 / s2d_conv2d_nhwc_f32 address an operand with 32-bit buffer offsets (gemm_bf16.hip)
CLIP_CHANNELS = 256               # channels of the 1/4-resolution pixel-decoder maps, the widest activation a clip's GEMMs read


def check_clip_size(T, Hp, Wp):
    """refuse, as ValueError, a clip whose 1/4-resolution activation [T * Hp/4 * Wp/4, 256] f32 -- an operand of the mask-feature
    GEMMs and convolutions -- exceeds what the dense kernels address (4 GB - 256 B; T = 71 at 720p is the last that fits).  Called
    before the network runs, so nothing is launched; without it the forward ends in a bare `s2d_gemm_nt_f32 failed with code -1`."""
    rows = int(T) * (int(Hp) // 4) * (int(Wp) // 4)
    if rows * CLIP_CHANNELS * 4 > GEMM_OPERAND_BYTES:
        per = (int(Hp) // 4) * (int(Wp) // 4) * CLIP_CHANNELS * 4
        raise ValueError(f"a clip of {T} frames at {Hp} x {Wp} has {rows * CLIP_CHANNELS * 4} bytes of 1/4-resolution activations; the dense "
                         f"kernels take at most {GEMM_OPERAND_BYTES} ({GEMM_OPERAND_BYTES // per} frames at this size).  Run longer videos "
                         f"with MODEL.MASK_FORMER.TEST.WINDOW_INFERENCE (WINDOW_SIZE frames per window)")


def window_kwargs(mf):
    """the three MODEL.MASK_FORMER.TEST.WINDOW_* keys as constructor arguments, checked (absent keys: the switch is off)"""
    t = getattr(mf, "TEST", None)
    on = bool(getattr(t, "WINDOW_INFERENCE", False))
    W, O = int(getattr(t, "WINDOW_SIZE", 0)), int(getattr(t, "WINDOW_OVERLAP", 0))
    check_window_config(on, W, O, mf.NUM_OBJECT_QUERIES)
    return {"window_inference": on, "window_size": W, "window_overlap": O}


def plan_windows(T, W, O):
    """frames [start, end) of every window of a T-frame video: stride S = W - O, window w = [w*S, min(w*S + W, T)), the last
    window is the first whose end reaches T, and a last window shorter than O + 1 frames (it would own none) is merged into its
    predecessor -- a guard: with that rule for the last window its predecessor ended before T, so it starts more than O frames
    before T.  T <= W: one window."""
    T, W, O = int(T), int(W), int(O)
    if T < 1:
        raise ValueError(f"a video has at least one frame, got T = {T}")
    check_window_config(True, W, O)
    S = W - O
    plan, start = [], 0
    while True:
        end = min(start + W, T)
        plan.append((start, end))
        if end == T:
            break
        start += S
    if len(plan) > 1 and plan[-1][1] - plan[-1][0] < O + 1:
        plan.pop()
        plan[-1] = (plan[-1][0], T)
    return plan


@torch.no_grad()
def associate(prev_logits, cur_logits, dims):
    """prev_logits, cur_logits: pixel-major [O*hm*wm, ldq] logits of the SAME O frames in two consecutive windows; dims = (Q, O,
    hm, wm).  -> dict of device tensors: cost f32 [Q,Q] = 1 - IoU of the masks `logit > 0` (row: query of the previous window,
    column: query of the current one; IoU = 0 for an empty union), idx_prev / idx_cur int64 [Q] = the solver's assignment, iou
    f32 [Q] = the IoU of every assigned pair, valid bool [Q] = iou > 0 (a pair without overlap counts as unmatched)."""
    Q, O, hm, wm = dims
    n = O * hm * wm
    if prev_logits.shape != cur_logits.shape or prev_logits.shape[0] != n:
        raise ValueError(f"associate: blocks {tuple(prev_logits.shape)} / {tuple(cur_logits.shape)} for dims {dims}")
    inter, area_p, area_c = ops.window_pair_counts(prev_logits, cur_logits, Q)
    union = area_p[:, None] + area_c[None, :] - inter
    iou = torch.where(union > 0, inter.to(torch.float32) / union.to(torch.float32), torch.zeros((), device=inter.device))
    cost = (1.0 - iou).contiguous()
    count = torch.full((1,), Q, device=cost.device, dtype=torch.int32)
    iq, it, _ = ops.lsap(cost.view(1, Q, Q), count, 1)
    iq, it = iq[0].long(), it[0].long()
    pair = iou[iq, it]
    return {"cost": cost, "idx_prev": iq, "idx_cur": it, "iou": pair, "valid": pair > 0}


def _track_permutation(match, slot_prev):
    """perm int64 [Q]: the query of the current window that carries track p.  A matched query takes the track of its partner in the
    previous window (slot_prev[i] = track of the previous window's query i); the unmatched queries take the unmatched tracks, both
    in ascending order -- so the result does not depend on what the solver does among zero-IoU ties.  Device ops on Q elements."""
    Q = slot_prev.numel()
    dev = slot_prev.device
    valid, it = match["valid"], match["idx_cur"]
    track = slot_prev[match["idx_prev"]]                                   # a permutation: the assignment is complete (Q x Q)
    perm = torch.full((Q,), -1, device=dev, dtype=torch.long)
    perm.scatter_(0, track, torch.where(valid, it, torch.full_like(it, -1)))
    used = torch.zeros((Q,), device=dev, dtype=torch.bool)
    used.scatter_(0, it, valid)
    free_q = torch.argsort(used.to(torch.int32), stable=True)              # the unmatched queries first, ascending
    free_t = perm < 0
    rank = (torch.cumsum(free_t.to(torch.long), 0) - 1).clamp_(min=0)      # k-th unmatched track <- k-th unmatched query
    return torch.where(free_t, free_q[rank], perm)


@torch.no_grad()
def stitch(plan, outputs, dims, overlap, record=None):
    """plan: plan_windows(T, W, O); outputs: an iterable giving, window by window, (class_logits [Q,C1], mask_logits pixel-major
    [Tw*hm*wm, ldq]) -- a generator, so that a window's activations can be released before the next one runs; dims = (Q, hm, wm);
    overlap = O.  -> (class logits [Q,C1] = mean over the windows of the logits of the query carrying each track, stitched mask
    logits [T*hm*wm, ldq]: column p = track p, every frame from the first window that contains it).  Track p of window 0 is its
    query p.  record (a list): receives per window >= 1 the associate() dict plus "perm"."""
    Q, hm, wm = dims
    O, hw = int(overlap), hm * wm
    T = plan[-1][1]
    buf = cls_sum = prev_shared = slot_prev = None
    it = iter(outputs)
    for k, (start, end) in enumerate(plan):
        try:                                                               # (no zip: it would hold window k - 1's tensors while the
            cls, ml = next(it)                                             # generator runs window k)
        except StopIteration:
            raise ValueError(f"stitch: {len(plan)} windows planned, {k} given") from None
        rows = (end - start) * hw
        if ml.dim() != 2 or ml.shape[0] != rows or cls.shape[0] != Q:
            raise ValueError(f"stitch: window [{start}, {end}) gave mask logits {tuple(ml.shape)}, class logits {tuple(cls.shape)}")
        dev = ml.device
        if k == 0:
            buf = torch.empty((T * hw, ml.shape[1]), device=dev, dtype=torch.float32)
            perm = torch.arange(Q, device=dev)
            own = 0
        else:
            match = associate(prev_shared, ml[:O * hw], (Q, O, hm, wm))
            perm = _track_permutation(match, slot_prev)
            own = O
            if record is not None:
                record.append(dict(match, perm=perm))
        ops.window_scatter_columns(ml[own * hw:], perm.to(torch.int32), buf, (start + own) * hw, Q)
        track_cls = cls.index_select(0, perm).to(torch.float32)
        cls_sum = track_cls if cls_sum is None else cls_sum + track_cls
        if end < T:                                                        # what the next window is associated with
            prev_shared = ml[rows - O * hw:].clone()
            slot_prev = torch.empty_like(perm).scatter_(0, perm, torch.arange(Q, device=dev))
        del cls, ml
    return (cls_sum / len(plan) if len(plan) > 1 else cls_sum), buf


@torch.no_grad()
def run_windows(net, images, window_size, window_overlap, record=None):
    """the network on every window of images [T,Hp,Wp,4], one after another, stitched: -> (class logits [Q,C1], mask logits
    [T*hm*wm, ldq], (T, hm, wm), number of windows).  Between two windows only the stitched buffer, the previous window's O shared
    frames and the class-logit sum stay allocated."""
    T = images.shape[0]
    plan = plan_windows(T, window_size, window_overlap)

    def run(start, end):
        check_clip_size(end - start, images.shape[1], images.shape[2])
        out = net(images[start:end], False)
        return (out.class_logits[-1][0], out.mask_logits[-1][0]), (out.Q, out.hm, out.wm)

    first = [run(*plan[0])]                                                # the first window tells the map size
    dims = first[0][1]

    def outputs():
        for k, (start, end) in enumerate(plan):
            pair = first.pop()[0] if k == 0 else run(start, end)[0]
            yield pair
            pair = None                                                    # on resumption, before the next window runs

    cls, buf = stitch(plan, outputs(), dims, window_overlap, record)
    return cls, buf, (T, dims[1], dims[2]), len(plan)
