"""Worker of tests/test_gpu_ytvis_eval.py::test_two_gloo_ranks_share_the_gpu (one process per rank, started by
torch.distributed.run, backend gloo, both ranks on cuda:0): each rank feeds YTVISEvaluator.process half the fixture's videos as
RLE; evaluate() gathers the per-video records; rank 0 writes its result to $S2D_YTVIS_OUT, the other rank must get {}."""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    from s2d_amd.ytvis_eval import YTVISEvaluator
    with open(os.path.join(ROOT, "tests", "golden", "ytvis_eval.json")) as fh:
        fx = json.load(fh)
    byvid = {}
    for r in fx["results"]:
        byvid.setdefault(r["video_id"], []).append(r)
    ev = YTVISEvaluator(json_file=fx["gt"], distributed=True)
    ev.reset()
    for vid in sorted(byvid)[rank::world]:
        rs = byvid[vid]
        ev.process([{"video_id": vid, "length": len(rs[0]["segmentations"])}],
                   {"pred_scores": [r["score"] for r in rs], "pred_labels": [r["category_id"] for r in rs],
                    "pred_masks": [r["segmentations"] for r in rs], "pred_masks_format": "coco_rle"})
    res = ev.evaluate()
    if rank == 0:
        with open(os.environ["S2D_YTVIS_OUT"], "w") as fh:
            json.dump({"segm": res["segm"], "stats": ev.ytvis_eval.stats.tolist()}, fh)
    else:
        assert res == {}, res
    dist.barrier()
    dist.destroy_process_group()
    print(f"YTVIS_WORKER_OK rank={rank}")


if __name__ == "__main__":
    main()
