"""The short-K static-weight GEMM launches of the c4 step, each in isolation, with the row-resident kernel off and forced
(S2D_GEMM_ROWS=0 / 2, read per launch): python scripts/mb_gemm_rows.py [rounds] -> ms per launch, median over the rounds, both settings
alternating in one process.  This table decides gemm_rows_wins() in csrc/gemm_route.h."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from s2d_amd import ops
from s2d_amd._lib import lib

# (M, N, K, form): "res" = folded-BN scale + bias + residual + ReLU (a bottleneck's conv3), "bias" = a projection
SHAPES = [(58880, 1024, 256, "res"), (235520, 768, 256, "bias"), (235520, 512, 128, "res"), (942080, 256, 64, "res"),
          (942080, 256, 256, "bias"), (58880, 768, 256, "bias"), (14720, 768, 256, "bias"), (309120, 544, 256, "bias"),
          (942080, 128, 256, "bias")]
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda")
torch.manual_seed(0)
print(f"{'M x N x K':>22} {'form':>5} {'ROWS=0 ms':>10} {'ROWS=2 ms':>10} {'0 / 2':>7}  floor ms (bytes / 4.5 TB/s)")
for M, N, K, form in SHAPES:
    x = torch.randn((M, K), device=dev)
    w = torch.nn.Parameter(torch.randn((N, K), device=dev) / K ** 0.5, requires_grad=False)
    b = torch.randn((N,), device=dev)
    s = torch.rand((N,), device=dev) + 0.5
    r = torch.randn((M, N), device=dev) if form == "res" else None
    y = torch.empty((M, N), device=dev)

    def run():
        if form == "res":
            ops.gemm_nt(x, w, s, b, r, relu=True, out=y)
        else:
            ops.gemm_nt(x, w, bias=b, out=y)

    ms = {"0": [], "2": []}
    reps = 20
    for rnd in range(rounds + 1):                  # round 0 warms both up
        for mode in ("0", "2"):
            os.environ["S2D_GEMM_ROWS"] = mode
            n0 = lib().call("s2d_gemm_rows_launches")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            assert lib().call("s2d_gemm_rows_launches") - n0 == (reps if mode == "2" else 0)
            if rnd:
                ms[mode].append(e0.elapsed_time(e1) / reps)
    m0, m2 = statistics.median(ms["0"]), statistics.median(ms["2"])
    floor = 4.0 * (M * K + N * K + M * N * (2 if form == "res" else 1)) / 4.5e12 * 1e3
    print(f"{M:>8} x {N:>4} x {K:>3} {form:>5} {m0:>10.3f} {m2:>10.3f} {m0 / m2:>7.3f}  {floor:.3f}   spread 0: {min(ms['0']):.3f}-{max(ms['0']):.3f}  2: {min(ms['2']):.3f}-{max(ms['2']):.3f}", flush=True)
    del x, w, b, s, r, y
