"""References and input generators for the masked cross-attention kernels of csrc/attn.hip (plain torch / numpy, no GPU needed).

tests/test_attn_refs_cpu.py proves without a GPU that the generated inputs have the properties they are named for;
tests/test_gpu_attn_masks.py compares the kernels with `masked_attn_ref` on them."""
import math

import torch

LOG2E = 1.4426950408889634
KT = 32          # keys per forward tile / per MFMA backward tile (attn.hip: KT)
BT = 64          # keys per tile of the backward's split count and of the scalar backward (attn.hip: BT)


def effective(mask):
    """mask bool [B,Q,K] (True: masked) after the all-masked rule: a query whose every key is masked attends everywhere"""
    eff = mask.clone()
    eff[eff.all(-1)] = False
    return eff


def masked_attn_ref(q, k, v, mask, H, dtype, dout=None):
    """softmax(q k^T / sqrt(d) with masked keys at -inf) v per head, evaluated in `dtype` on the operands' device.
    q [B,Q,C], k / v [B,K,C], mask bool [B,Q,K] (True: masked) or None; a query with every key masked attends everywhere.
    -> (out [B,Q,C], lse2 [B,H,Q]: the base-2 log-sum-exp of the scaled scores), and with `dout` also (dq, dk, dv) by autograd."""
    B, Q, C = q.shape
    K, D = k.shape[1], C // H
    grad = dout is not None
    qd, kd, vd = (t.detach().to(dtype).clone().requires_grad_(grad) for t in (q, k, v))
    sc = torch.einsum("bqhd,bkhd->bhqk", qd.reshape(B, Q, H, D), kd.reshape(B, K, H, D)) / math.sqrt(D)
    if mask is not None:
        sc = sc.masked_fill(effective(mask)[:, None], float("-inf"))
    lse2 = torch.logsumexp(sc, -1) * LOG2E
    out = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), vd.reshape(B, K, H, D)).reshape(B, Q, C)
    if not grad:
        return out.detach(), lse2.detach()
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), lse2.detach(), qd.grad, kd.grad, vd.grad


def pack_bits(mask):
    """mask bool [B,Q,K] (True: masked), Q <= 128 -> (bits int32 [B,K,4]: bit q & 31 of word q >> 5 of a key's row is set when query q
    may not attend the key; unmasked int32 [B,4]: bit q set when query q has a free key).  Bits of queries >= Q are 0."""
    B, Q, K = mask.shape
    assert Q <= 128
    qi = torch.arange(Q, device=mask.device)
    sh = (qi & 31).to(torch.int64)
    words = torch.zeros((B, K, 4), device=mask.device, dtype=torch.int64)
    unw = torch.zeros((B, 4), device=mask.device, dtype=torch.int64)
    free = (~mask).any(-1)
    for w in range(4):
        sel = (qi >> 5) == w
        if sel.any():
            words[:, :, w] = (mask[:, sel, :].to(torch.int64) << sh[sel][None, :, None]).sum(1)
            unw[:, w] = (free[:, sel].to(torch.int64) << sh[sel][None, :]).sum(1)
    wrap = lambda t: ((t + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).contiguous()
    return wrap(words), wrap(unw)


def unpack_bits(bits, unmasked, Q):
    """the inverse of pack_bits -> (mask bool [B,Q,K], free bool [B,Q])"""
    qi = torch.arange(Q, device=bits.device)
    w = bits.to(torch.int64) & 0xFFFFFFFF
    u = unmasked.to(torch.int64) & 0xFFFFFFFF
    mask = ((w[:, :, qi >> 5] >> (qi & 31)) & 1).bool().permute(0, 2, 1).contiguous()
    free = ((u[:, qi >> 5] >> (qi & 31)) & 1).bool()
    return mask, free


def splits(K):
    """The launch arithmetic of the attention entry points, restated for choosing inputs.

    Forward (s2d_masked_attn_f32: `tiles = (K + KT - 1) / KT; S = tiles / 4` clamped to [1, 32]; `tiles_per_split = (tiles + S - 1) / S`;
    cross_attn_kernel: `tile0 = split * tiles_per_split`, `tile1 = min(ntiles_all, tile0 + tiles_per_split)`): trailing splits with
    tile0 >= tiles have no tile and leave m = -1e30, l = 0, o = 0 for the merge to drop.
    Backward (attn_bwd_splits: `tiles = (K + BT - 1) / BT; S = tiles / 4` clamped to [1, 64]; s2d_masked_attn_backward_strided_f32:
    `tiles_per_split = (tiles + S - 1) / S` 64-key tiles on the scalar path, `(tiles32 + S - 1) / S` 32-key tiles on the MFMA path)."""
    tiles = (K + KT - 1) // KT
    S = min(max(tiles // 4, 1), 32)
    tps = (tiles + S - 1) // S
    nonempty = (tiles + tps - 1) // tps
    tiles64 = (K + BT - 1) // BT
    Sb = min(max(tiles64 // 4, 1), 64)
    return {
        "tiles": tiles, "S": S, "tiles_per_split": tps, "nonempty": nonempty, "empty": list(range(nonempty, S)),
        "bwd_S": Sb, "bwd_tiles_per_split": (tiles + Sb - 1) // Sb, "bwd_scalar_tiles_per_split": (tiles64 + Sb - 1) // Sb,
    }


def group_all(eff, keys_per_group):
    """eff bool [B,Q,K] -> bool [B,Q,G]: group g (keys_per_group consecutive keys, the last one ragged) is wholly masked for the query"""
    B, Q, K = eff.shape
    G = (K + keys_per_group - 1) // keys_per_group
    pad = torch.ones((B, Q, G * keys_per_group), dtype=torch.bool, device=eff.device)
    pad[:, :, :K] = eff
    return pad.reshape(B, Q, G, keys_per_group).all(-1)


def masked_shares(eff):
    """-> the shares of wholly masked (query, 32-key tile), (query, non-empty forward split) and (query, MFMA backward split) pairs"""
    sp = splits(eff.shape[-1])
    tile = group_all(eff, KT).float().mean().item()
    fwd = group_all(eff, KT * sp["tiles_per_split"])
    assert fwd.shape[-1] == sp["nonempty"]
    bwd = group_all(eff, KT * sp["bwd_tiles_per_split"])
    return tile, fwd.float().mean().item(), bwd.float().mean().item()


def object_masks(B, Q, T, hl, wl, gen):
    """Masks shaped like the decoder's own: key index (t * hl + y) * wl + x, K = T * hl * wl.  An ordinary query is free inside one
    random box (height < hl / 2, width < wl / 3) in a random non-empty subset of the T frames and masked elsewhere.  Then special
    rows are overwritten (those whose number is < Q; in every clip unless stated):
      q0 (clip 0 only) every key masked;  q1 only key 0 free;  q2 only key K - 1 free;  q3 only the first key of the last tile free
      (the ragged one when K % 32 != 0);  q4 free only in the last non-empty forward split;  q5 free only in tile 0;  q6 nothing
      masked;  q7 free on exactly one aligned 32-key tile in the interior;  q8 masked on exactly that tile;  q32..q63 of one clip
      every key masked (a whole wave with the mask off between waves that keep it).
    With T >= 3 and B >= 2 the middle frame of clip 1 is reserved: clip 1's boxes are drawn from the other frames and the frame is
    masked for every query of clip 1 AFTER the special rows, so that its keys have exactly zero key / value gradients.  For that to
    hold on the effective masks clip 1 may not contain a query that attends everywhere by the all-masked rule, so the masked wave
    sits in the last clip other than clip 1 (clip 0 when B <= 2), and q7's tile is the interior tile nearest the middle of the key
    range that lies outside the reserved frame; q6 and q8 of clip 1 are free everywhere outside the reserved frame.
    -> (mask bool [B,Q,K] True: masked, info dict)"""
    K = T * hl * wl
    sp = splits(K)
    hw = hl * wl
    mask = torch.ones((B, Q, K), dtype=torch.bool)
    reserved = T // 2 if (T >= 3 and B >= 2) else None
    hmax, wmax = (hl - 1) // 2, -(-wl // 3) - 1                  # the largest height < hl / 2 and width < wl / 3
    assert hmax >= 1 and wmax >= 1
    ri = lambda hi: int(torch.randint(0, hi, (1,), generator=gen))         # uniform in [0, hi)
    for b in range(B):
        frames = [t for t in range(T) if not (b == 1 and t == reserved)]
        for qq in range(Q):
            while True:
                sel = torch.rand(len(frames), generator=gen) < 0.5
                if sel.any():
                    break
            h, w = 1 + ri(hmax), 1 + ri(wmax)
            y0, x0 = ri(hl - h + 1), ri(wl - w + 1)
            plane = torch.ones((hl, wl), dtype=torch.bool)
            plane[y0:y0 + h, x0:x0 + w] = False
            for t, s in zip(frames, sel.tolist()):
                if s:
                    mask[b, qq, t * hw:(t + 1) * hw] = plane.reshape(-1)
    tile = sp["tiles"] // 2
    if reserved is not None and (tile + 1) * KT > reserved * hw and tile * KT < (reserved + 1) * hw:
        tile = reserved * hw // KT - 1                           # the last aligned tile wholly in front of the reserved frame
    assert 0 < tile < sp["tiles"] - 1 or sp["tiles"] < 3
    last_tile_key = (sp["tiles"] - 1) * KT
    last_split_key = (sp["nonempty"] - 1) * sp["tiles_per_split"] * KT
    single = {1: 0, 2: K - 1, 3: last_tile_key}

    def only(qq, lo, hi):
        if qq < Q:
            mask[:, qq] = True
            mask[:, qq, lo:hi] = False
    if Q > 0:
        mask[0, 0] = True
    for qq, j in single.items():
        only(qq, j, j + 1)
    only(4, last_split_key, K)
    only(5, 0, min(KT, K))
    if Q > 6:
        mask[:, 6] = False
    only(7, tile * KT, (tile + 1) * KT)
    if Q > 8:
        mask[:, 8] = False
        mask[:, 8, tile * KT:(tile + 1) * KT] = True
    wave_clip = None
    if Q >= 64:
        wave_clip = B - 1 if B - 1 != 1 else 0
        mask[wave_clip, 32:64] = True
    if reserved is not None:
        lo, hi = reserved * hw, (reserved + 1) * hw
        for j in (0, K - 1, last_tile_key, last_split_key, tile * KT, (tile + 1) * KT - 1, KT - 1):
            assert not lo <= j < hi, "a special row's free keys fall into the reserved frame"
        mask[1, :, lo:hi] = True
    info = {"K": K, "tile": tile, "single": {qq: j for qq, j in single.items() if qq < Q}, "last_split_key": last_split_key,
            "reserved_frame": reserved, "wave_clip": wave_clip}
    return mask, info
