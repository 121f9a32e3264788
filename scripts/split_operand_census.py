"""Magnitudes of the operands the split-fp16 x3 kernels split, per launch.

The split (x = h + l * 2^-11, h = fp16_rtz(x), l = fp16_rtz((x - h) * 2^11)) keeps fp32-class accuracy only while every operand
tensor lies in the window 2^-14 <= amax <= 65504 (csrc/gemm_bf16.hip, DESIGN.md "Dense arithmetic").  `Census` wraps the library's
`call` and records, for each launch of a split-fp16 export, every tensor operand's amax and the share of its nonzero entries
below 2^-14 and below 2^-24.  Operands handed over as raw addresses (the padded-copy weight gradient's shifted taps) are listed
as unrecorded, not guessed.

    python scripts/split_operand_census.py [--config c4] [--out DIR] [--json]        (S2D_GRAD_SCALE_LOG2=0: the unscaled backward)

runs one training iteration's device work (KDVideoMaskFormer.forward_backward at the bench's synthetic batch, loss_scale 1 as
engine.run_step passes it at ACCUM_ITER 1) under the census and writes the summary as JSON and text."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# export -> argument positions of the operands it splits (include/s2d_hip.h)
SPLIT_OPERANDS = {
    "s2d_gemm_nt_f32": (0, 1),
    "s2d_gemm_nt_dropout_f32": (0, 1),
    "s2d_gemm_nt_gate_f32": (0, 1),
    "s2d_gemm_nt_presplit_f32": (1,),             # A arrives as a split image (recorded at its s2d_split_weights_f16)
    "s2d_split_weights_f16": (0,),
    "s2d_conv2d_nhwc_f32": (0, 1),
    "s2d_conv2d_nhwc_gate_f32": (0, 1),
    "s2d_ffn_pack_f16": (0, 1, 4, 6),
    "s2d_ffn_fused_f32": (0,),
    "s2d_masked_attn_f32": (0, 1, 2),
    "s2d_masked_attn_backward_f32": (0, 1, 2, 7, 9),
    "s2d_masked_attn_backward_strided_f32": (0, 1, 2, 7, 9),
    "s2d_gemm_tn_f32": (0, 1),
    "s2d_conv_wgrad_tn_f32": (0, 1),
}
LO, HI = 2.0 ** -14, 2.0 ** 12       # the gradient contract: operands inside [2^-14, 2^12] (16x headroom below 65504)


class Census:
    """with Census() as c: ...  -> c.records(): one dict per (launch, operand).  phase: "forward" until the first loss backward
    launch (ops.point_loss_backward / class_loss_backward), "backward" after it."""

    def __init__(self):
        self._raw = []
        self.phase = "forward"

    def __enter__(self):
        from s2d_amd import ops
        from s2d_amd._lib import lib
        self._lib = lib()
        self._orig = self._lib.call
        self._ops = ops
        self._orig_plb, self._orig_clb = ops.point_loss_backward, ops.class_loss_backward

        def call(name, *args):
            pos = SPLIT_OPERANDS.get(name)
            if pos is not None:
                for i in pos:
                    a = args[i] if i < len(args) else None
                    if a is None:
                        continue
                    if isinstance(a, torch.Tensor):
                        t = a.detach()
                        ab = t.abs()
                        nz = t != 0
                        stats = torch.stack([ab.amax().double() if t.numel() else torch.zeros((), dtype=torch.float64, device=t.device),
                                             nz.sum().double(), (nz & (ab < 2.0 ** -14)).sum().double(),
                                             (nz & (ab < 2.0 ** -24)).sum().double()])
                        self._raw.append((name, i, self.phase, tuple(t.shape), stats))
                    else:
                        self._raw.append((name, i, self.phase, None, None))
            return self._orig(name, *args)

        def plb(*a, **k):
            self.phase = "backward"
            return self._orig_plb(*a, **k)

        def clb(*a, **k):
            self.phase = "backward"
            return self._orig_clb(*a, **k)

        self._lib.call = call
        ops.point_loss_backward, ops.class_loss_backward = plb, clb
        return self

    def __exit__(self, *exc):
        del self._lib.call                                   # the instance attribute goes, the class method is back
        self._ops.point_loss_backward, self._ops.class_loss_backward = self._orig_plb, self._orig_clb

    def records(self):
        torch.cuda.synchronize()
        out = []
        for name, i, phase, shape, st in self._raw:
            if st is None:
                out.append(dict(export=name, arg=i, phase=phase, recorded=False))
                continue
            amax, nz, b14, b24 = (float(v) for v in st.cpu())
            out.append(dict(export=name, arg=i, phase=phase, recorded=True, shape=shape, amax=amax, nonzero=int(nz),
                            below_2m14=b14 / max(nz, 1.0), below_2m24=b24 / max(nz, 1.0)))
        return out


def summarize(recs):
    """per (phase, export): launches, operands recorded / unrecorded, amax range, worst shares below 2^-14 / 2^-24, and how many
    operands fall outside [2^-14, 2^12] (all-zero operands count as inside)"""
    rows = {}
    for r in recs:
        k = (r["phase"], r["export"])
        s = rows.setdefault(k, dict(phase=r["phase"], export=r["export"], operands=0, unrecorded=0, amax_min=None, amax_max=None,
                                    max_below_2m14=0.0, max_below_2m24=0.0, below_window=0, above_window=0, all_zero=0))
        if not r["recorded"]:
            s["unrecorded"] += 1
            continue
        s["operands"] += 1
        if r["nonzero"] == 0:
            s["all_zero"] += 1
            continue
        a = r["amax"]
        s["amax_min"] = a if s["amax_min"] is None else min(s["amax_min"], a)
        s["amax_max"] = a if s["amax_max"] is None else max(s["amax_max"], a)
        s["max_below_2m14"] = max(s["max_below_2m14"], r["below_2m14"])
        s["max_below_2m24"] = max(s["max_below_2m24"], r["below_2m24"])
        s["below_window"] += a < LO
        s["above_window"] += a > HI
    return list(rows.values())


def outside_window(recs):
    """the recorded operands with amax outside [2^-14, 2^12] that are not all zeros"""
    return [r for r in recs if r["recorded"] and r["nonzero"] and not (LO <= r["amax"] <= HI)]


def _fmt(rows):
    lines = [f"{'phase':9s} {'export':38s} {'ops':>5s} {'unrec':>5s} {'amax min':>10s} {'amax max':>10s} {'<2^-14':>7s} {'<2^-24':>7s} "
             f"{'below':>5s} {'above':>5s} {'zero':>4s}"]
    for s in rows:
        lo = f"{s['amax_min']:.3e}" if s["amax_min"] is not None else "-"
        hi = f"{s['amax_max']:.3e}" if s["amax_max"] is not None else "-"
        lines.append(f"{s['phase']:9s} {s['export']:38s} {s['operands']:5d} {s['unrecorded']:5d} {lo:>10s} {hi:>10s} "
                     f"{s['max_below_2m14']:7.4f} {s['max_below_2m24']:7.4f} {s['below_window']:5d} {s['above_window']:5d} {s['all_zero']:4d}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--out", default="profiles/split_range")
    ap.add_argument("--json", action="store_true", help="also write every record as JSON")
    ap.add_argument("--loss-scale", type=float, default=1.0)
    args = ap.parse_args()
    import bench
    from s2d_amd import backward, ops
    from s2d_amd.modeling import TargetSet, build_kd_model
    dev = torch.device("cuda")
    B, T, H0, W0, Q, P, N = bench.CONFIGS[args.config]
    model = build_kd_model(num_queries=Q, num_frames=T, num_points=P, weights=(0.0, 5.0, 5.0), kd_weights=(0.0, 5.0, 5.0)).to(dev)
    model.train()
    frames, masks = bench.synth_batch(0, B, T, H0, W0, N, dev)
    bench.calibrate_teacher(model, ops.normalize_pad(frames))
    mean, std = model.pixel_mean.flatten().cpu().numpy(), model.pixel_std.flatten().cpu().numpy()
    images = ops.normalize_pad(frames, 32, mean, std)
    targets = TargetSet.from_list(masks, device=dev)
    # two passes, the second at twice the backward's root scale: an operand whose amax doubles carries the gradient (the rest are the
    # forward's activations and weights the backward reads); both passes make the same launches in the same order
    model.forward_backward(images, targets, loss_scale=args.loss_scale)      # warm: the weight caches' splits happen once, not per pass
    runs = []
    k0 = backward.GRAD_SCALE_LOG2
    for k in (k0, k0 + 1):
        backward.GRAD_SCALE_LOG2 = k
        for p in model.student.parameters():
            p.grad = None
        with Census() as c:
            model.forward_backward(images, targets, loss_scale=args.loss_scale)
        runs.append(c.records())
    backward.GRAD_SCALE_LOG2 = k0
    recs = runs[0]
    assert len(recs) == len(runs[1])
    for a, b in zip(recs, runs[1]):
        a["gradient"] = bool(a["recorded"] and a["nonzero"] and b["export"] == a["export"] and 1.9 <= b["amax"] / a["amax"] <= 2.1)
    rows = summarize(recs)
    grad_rows = summarize([r for r in recs if r.get("gradient")])
    gops = [r["amax"] for r in recs if r.get("gradient")]
    grads = [p.grad for p in model.student.parameters() if p.grad is not None]      # of the second pass (root scale doubled)
    gmax = max(float(g.abs().max()) for g in grads)
    gmin = min(float(g.abs().max()) for g in grads if float(g.abs().max()) > 0)
    os.makedirs(args.out, exist_ok=True)
    import math
    meta = dict(config=args.config, loss_scale=args.loss_scale, grad_scale_log2=backward.GRAD_SCALE_LOG2, num_points=P,
                root_scale_log2=math.log2(backward.grad_scale(args.loss_scale)),          # gradient operands = raw ones * 2^this
                param_grad_amax_max=gmax, param_grad_amax_min_nonzero=gmin, launches_recorded=len(recs),
                outside_window=len(outside_window(recs)), gradient_operands=len(gops),
                gradient_operand_amax_min=min(gops) if gops else None, gradient_operand_amax_max=max(gops) if gops else None)
    tag = f"census_{args.config}_k{backward.GRAD_SCALE_LOG2}"
    if args.json:
        with open(os.path.join(args.out, tag + ".json"), "w") as f:
            json.dump(dict(meta=meta, summary=rows, gradient_summary=grad_rows, records=recs), f, indent=1)
    txt = json.dumps(meta) + "\n\nall split operands\n" + _fmt(rows) + "\n\ngradient operands\n" + _fmt(grad_rows)
    with open(os.path.join(args.out, tag + ".txt"), "w") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
