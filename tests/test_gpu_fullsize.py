"""Size-independent properties of the hot path at BASELINE's full metric shapes (T=8, 720p, Q=100, P=160000,
2 clips): run-to-run determinism (bitwise), clip-order equivariance, valid assignments, finite losses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    import bench
    from s2d_amd import ops
    from s2d_amd.modeling import TargetSet, build_kd_model
    dev = torch.device("cuda:0")
    B, T, H0, W0, Q, P, N = bench.CONFIGS["c4"]
    # encoder dropout 0.3 as every shipped yaml sets it (MODEL.MASK_FORMER.DROPOUT) and as bench.py times it: the schedule /
    # determinism properties below are checked on the benched configuration, masks included
    model = build_kd_model(num_queries=Q, num_frames=T, num_points=P, dropout=0.3).to(dev)
    frames, masks = bench.synth_batch(0, B, T, H0, W0, N, dev)
    bench.calibrate_teacher(model, ops.normalize_pad(frames))
    return model, frames, masks, (B, T, Q, N)


def _run(model, frames, masks):
    from s2d_amd import ops
    from s2d_amd.modeling import TargetSet
    model.criterion.seed = 0
    model.criterion.matcher.seed = 0
    torch.manual_seed(5); ops._DROP_CALLS[0] = 0          # the dropout masks' Philox keys: same keys every run
    losses = model.forward_losses(ops.normalize_pad(frames), TargetSet.from_list(masks, device=frames.device))
    torch.cuda.synchronize()
    iq, it, nm = (x.cpu().numpy() for x in model.criterion.last_indices)
    return {k: float(v) for k, v in losses.items()}, (iq, it, nm), model.last["kd_count"].cpu().numpy()


def test_fullsize_properties(setup):
    model, frames, masks, (B, T, Q, N) = setup
    l1, (iq1, it1, nm1), kd1 = _run(model, frames, masks)
    assert len(l1) == 42 and all(np.isfinite(v) for v in l1.values())
    # every assignment is a valid partial matching: queries ascending and distinct, targets a permutation
    for p in range(iq1.shape[0]):
        k = nm1[p]
        assert k == min(Q, int(kd1[p % B]))
        q, t = iq1[p, :k], it1[p, :k]
        assert (np.diff(q) > 0).all() and sorted(t.tolist()) == list(range(k))
    # determinism: a second run with the same RNG seeds is bitwise identical (fixed-order reductions everywhere)
    l2, (iq2, it2, nm2), kd2 = _run(model, frames, masks)
    assert l1 == l2 and (iq1 == iq2).all() and (it1 == it2).all() and (kd1 == kd2).all()
    # clips are independent units: swapping the two clips swaps the per-clip KD counts (the path shards by clip)
    fr = frames.view(B, T, *frames.shape[1:]).flip(0).reshape(frames.shape).contiguous()
    l3, _, kd3 = _run(model, fr, masks[::-1])
    assert (kd3 == kd1[::-1]).all()
    # ... and the class loss (no point sampling involved) is unchanged up to summation order over clips
    np.testing.assert_allclose(l3["kd_loss_ce"], l1["kd_loss_ce"], rtol=1e-6, atol=1e-7)


def test_two_stream_schedule_bitwise(setup):
    """the optional two-stream schedule (teacher forward + GT criterion on a second HIP stream) changes no bit of the
    losses, the assignments or the teacher's pseudo targets -- repeated, since a violation would be a race"""
    model, frames, masks, _ = setup
    try:
        model.overlap_teacher = model.overlap_criteria = False
        ref = _run(model, frames, masks)
        model.overlap_teacher = model.overlap_criteria = True
        for _ in range(8):
            cur = _run(model, frames, masks)
            assert cur[0] == ref[0]
            assert all((a == b).all() for a, b in zip(cur[1], ref[1])) and (cur[2] == ref[2]).all()
    finally:
        model.overlap_teacher = model.overlap_criteria = False


def test_teacher_tap_gathered_masks_bitwise(setup):
    """evaluating the teacher's intermediate mask logits only at the attention masks' source pixels (aux_masks=False)
    leaves its final prediction -- all the KD pass reads -- bit-identical"""
    from s2d_amd import ops
    model, frames, _, _ = setup
    images = ops.normalize_pad(frames)
    torch.manual_seed(5); ops._DROP_CALLS[0] = 0
    full = model.teacher(images, True, aux_masks=True)
    torch.manual_seed(5); ops._DROP_CALLS[0] = 0          # same dropout masks in both evaluations
    thin = model.teacher(images, True, aux_masks=False)
    torch.cuda.synchronize()
    assert thin.mask_logits.shape[0] < full.mask_logits.shape[0]
    assert torch.equal(thin.mask_logits[-1], full.mask_logits[-1])
    assert torch.equal(thin.class_logits, full.class_logits)


def test_two_stream_schedule_on_round1_attention_mask_source():
    """The kernel source that produced wrong attention-mask words under the two-stream schedule in round 1
    (attn_mask_kernel_dword_taps: guarded 4-B tap loads; ~9 wrong words per repetition while SLP vectorisation turned its
    arithmetic into a packed op straight behind the load wait -- profiles/r2_two_stream_diagnosis/) gives 0 wrong words now
    that the library is built without that shape (scripts/isa_lint.py).  Own process: the variant is chosen at first launch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "race_diag.py"), "4"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, S2D_ATTN_MASK_DWORD_TAPS="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DWORD_TAPS=1" in r.stdout
    tot = [l for l in r.stdout.splitlines() if l.startswith("TOTAL")]
    assert tot and "first-launch wrong words 0, second-launch wrong words 0" in tot[0], r.stdout[-2000:]


def test_bench_two_ranks_share_the_gpu_gloo():
    """bench.py --gpus 2 --full started without a launcher: it spawns its two ranks, they rendezvous (gloo: RCCL refuses two ranks
    on one device), both run the metric step and the full training iteration incl. the gradient-arena all-reduce, and rank 0
    prints one line with n_gpus == 2"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, S2D_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "tiny", "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["value"] > 0 and j["schedules"]["losses_bitwise_equal_between_schedules"] is True
    ts = j["train_step"]
    assert "error" not in ts, ts
    assert ts["n_gpus"] == 2 and ts["allreduce_bytes"] > 100e6 and ts["ms_per_iteration"] > 0


def test_bench_dump_outputs_reproducible(tmp_path):
    """bench.py --dump-outputs: two runs with the same arguments write the same arrays, bit for bit (float32 / float64, within
    the budget); the line reports the --steps timed steps and ms_per_step; loss_total is the sum of the dumped losses"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "tiny", "--steps", "3", "--warmup", "1",
                            "--no-cpu-baseline", "--no-train-step", "--no-keymask", "--dump-outputs", d],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        runs.append((d, json.loads(lines[0])))
    (da, ja), (db, _) = runs
    assert ja["steps"] == 3 and ja["ms_per_step"] > 0
    names = sorted(os.listdir(da))
    assert names == sorted(os.listdir(db)) and ja["dumped_outputs"]["arrays"] == len(names)
    assert {"loss_total.npy", "pred_logits.npy", "pred_masks.npy", "loss_ce.npy", "kd_loss_dice.npy"} <= set(names)
    arrays = {n[:-4]: (np.load(os.path.join(da, n)), np.load(os.path.join(db, n))) for n in names}
    assert sum(a.nbytes for a, _ in arrays.values()) <= 64 * 2 ** 20
    for n, (a, b) in arrays.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), n
    losses = [a for n, (a, _) in arrays.items() if "loss_" in n and n != "loss_total"]
    np.testing.assert_allclose(arrays["loss_total"][0], np.sum(losses, dtype=np.float64), rtol=1e-5)


def test_bench_plain_run_is_lean_and_full_run_adds_the_reports(tmp_path):
    """a plain bench.py run prints the metric line without the reports that take runs of their own; --full adds every one of
    them after the timed steps and leaves the timed path alone: both runs dump the same arrays, bit for bit"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = {}
    for name, extra in (("plain", []), ("full", ["--full"])):
        d = str(tmp_path / name)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "tiny", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", d] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        runs[name] = (d, json.loads(lines[0]))
    (dp, jp), (df, jf) = runs["plain"], runs["full"]
    for j in (jp, jf):
        assert j["steps"] == 3 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0
        assert j["unit"] == "clip-frames/s" and j["higher_is_better"] is True and j["dtype"] == jp["dtype"]
    extras = ("amp", "train_step", "keymask", "cpu_baseline")
    assert not any(k in jp for k in extras) and jp["schedules"]["other_ms_per_step"] is None, jp
    assert jp["schedules"]["losses_bitwise_equal_between_schedules"] is None
    assert all(k in jf and "error" not in jf[k] for k in extras), {k: jf.get(k) for k in extras}
    assert jf["schedules"]["losses_bitwise_equal_between_schedules"] is True and jf["schedules"]["other_ms_per_step"] > 0
    assert "roofline" in jf
    names = sorted(os.listdir(dp))
    assert names == sorted(os.listdir(df)) and jp["dumped_outputs"]["arrays"] == len(names)
    for n in names:
        a, b = np.load(os.path.join(dp, n)), np.load(os.path.join(df, n))
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), n


def test_train_step_at_config4_gradients_finite_and_reproducible(setup):
    """BASELINE configs[3]'s training leg at full size (the whole iteration has no autograd oracle that fits there; each backward kernel
    call it makes is compared with float64 at these shapes in tests/test_gpu_backward_c4.py): every one of the 345 student gradients
    is finite, and two iterations on the same batch with the same seeds agree bit for bit (no float atomics are left in the step:
    MSDeformAttn's grad_value is a sorted gather, the point-loss scatter accumulates in fixed point)"""
    from s2d_amd import ops
    from s2d_amd.modeling import TargetSet
    model, frames, masks, _ = setup
    model.overlap_teacher = model.overlap_criteria = False
    params = [p for p in model.student.parameters()]

    def once():
        for p in params:
            p.grad = None
        model.criterion.seed = 0; model.criterion.matcher.seed = 0
        torch.manual_seed(5); ops._DROP_CALLS[0] = 0
        out = model.forward_backward(ops.normalize_pad(frames), TargetSet.from_list(masks, device=frames.device))
        torch.cuda.synchronize()
        return {k: float(v) for k, v in out.items()}, [p.grad.clone() for p in params]

    l1, g1 = once()
    l2, g2 = once()
    # ... and the overlapped schedule of the iteration (teacher forward beside the student's, GT criterion and its point-loss backward
    # beside the KD pass's, on a second stream) gives the same losses and the same 345 gradients, bit for bit
    model.overlap_teacher = model.overlap_criteria = True
    l3, g3 = once()
    # ... also when the side stream is held back ~0.1 s in front of the GT criterion (the weighted loss dict is formed on
    # the main stream and must be ordered behind the side stream's loss kernels, whichever stream finishes first)
    model._side_delay_cycles = 200_000_000
    l4, g4 = once()
    model._side_delay_cycles = 0
    model.overlap_teacher = model.overlap_criteria = False
    model.last_tapes = None
    assert l3 == l1 and all(torch.equal(a, b) for a, b in zip(g1, g3))
    assert l4 == l1 and all(torch.equal(a, b) for a, b in zip(g1, g4))
    del g3, g4
    assert len(g1) == 345 and l1 == l2
    assert all(bool(torch.isfinite(g).all()) for g in g1)
    spread = max(float((a - b).abs().max() / (a.abs().max() + 1e-30)) for a, b in zip(g1, g2))
    nbit = sum(int(torch.equal(a, b)) for a, b in zip(g1, g2))
    print(f"c4 train-step gradient reproducibility: {nbit} of 345 tensors bitwise equal, worst relative spread {spread:.3e}")
    # every gradient kernel is order-fixed now (MSDeformAttn: sorted gather; point loss: fixed-point integer scatter)
    assert nbit == 345 and spread == 0.0
