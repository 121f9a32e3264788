"""bench.py --dump-outputs on the host side: what capture_outputs keeps of a step's results, and the budget it keeps to."""
import numpy as np
import torch


def _outputs(B, Q, T, hm, wm, seed=0):
    from s2d_amd.modeling.video_decoder import MaskOutputs
    g = torch.Generator().manual_seed(seed)
    return MaskOutputs(torch.randn(2, B, Q, 2, generator=g), torch.randn(2, B, T * hm * wm, Q + 4, generator=g), Q, T, hm, wm)


class _Model:
    def __init__(self, student):
        self.last = {"student": student}


def test_capture_outputs_full_maps_and_losses():
    import bench
    st = _outputs(2, 16, 2, 16, 24)
    losses = {"loss_ce": torch.tensor(1.5), "kd_loss_mask_3": torch.tensor(0.25)}
    out = bench.capture_outputs(_Model(st), losses, sum(losses.values()))
    assert set(out) == {"loss_ce", "kd_loss_mask_3", "loss_total", "pred_logits", "pred_masks"}
    assert out["loss_total"] == np.float32(1.75) and out["loss_ce"] == np.float32(1.5)
    np.testing.assert_array_equal(out["pred_logits"], st.class_logits[-1].numpy())
    np.testing.assert_array_equal(out["pred_masks"], st.pred_masks(-1).numpy())
    # the clip pipeline's per-clip outputs give the same arrays as one batch
    clips = [_outputs(1, 16, 2, 16, 24, seed=s) for s in (1, 2)]
    out2 = bench.capture_outputs(_Model(clips), losses, sum(losses.values()))
    np.testing.assert_array_equal(out2["pred_masks"], np.concatenate([c.pred_masks(-1).numpy() for c in clips]))


def test_capture_outputs_samples_large_maps_within_budget():
    import bench
    st = _outputs(1, 16, 8, 264, 256)                     # 8.7 M mask logits: more than half the budget
    out = bench.capture_outputs(_Model(st), {"loss_ce": torch.tensor(1.0)}, torch.tensor(1.0))
    assert "pred_masks" not in out and sum(a.nbytes for a in out.values()) <= bench.DUMP_BYTES
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    idx = out["pred_masks_sample_index"].astype(np.int64)
    assert len(idx) > bench.MASK_SAMPLE // 2 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(out["pred_masks_sample"], st.pred_masks(-1).reshape(-1).numpy()[idx])
    again = bench.capture_outputs(_Model(st), {"loss_ce": torch.tensor(1.0)}, torch.tensor(1.0))
    np.testing.assert_array_equal(again["pred_masks_sample_index"], out["pred_masks_sample_index"])
