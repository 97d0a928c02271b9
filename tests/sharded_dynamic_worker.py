"""One rank of the sharded frame loop with DYNAMIC frame assignment on the REAL (mini, seeded) models: tests/sharded_mini_worker.py's
program with run_sharded(assignment="dynamic"): the ranks claim groups of consecutive mini frames from a counter in a TCPStore rank 0
hosts on MASTER_PORT + 1 (gloo process group: the record gather runs on host tensors, so two ranks can share the one GPU of the test
box).  Rank 0 writes the BOP csv; every rank writes the group indices it claimed to <out.csv>.rank<r>.json.
Launched by tests/test_gpu_zz_sharded_dynamic.py:  python -m tests.sharded_dynamic_worker <out.csv> <group_size>"""
import json
import os
import sys

import torch


def main():
    out, group = sys.argv[1], int(sys.argv[2])
    import torch.distributed as dist

    from sam6d_amd.utils import shard
    from tests.sharded_mini_worker import frame_table
    from tests.test_gpu_zz_pipeline import build_mini, mini_frames
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    store = None
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        store = dist.TCPStore(os.environ["MASTER_ADDR"], int(os.environ["MASTER_PORT"]) + 1, world, is_master=(rank == 0))
    pipe, frame = build_mini(torch.device("cuda", 0), top_k="keys", sync_stages=False)
    ids, load = frame_table(mini_frames(frame))
    if world > 1:
        dist.barrier()          # the ranks enter the loop together: a rank still building its models would find every group taken
    # prefetch=False: a rank claims when idle.  With the loader thread it claims its second group as it starts its first (look-ahead
    # 1), and with two groups in all the other rank's share would hang on which first claim came a microsecond earlier.
    res = shard.run_sharded(ids, load, pipe, group_size=group, dataset_name="ycbv", device=None, fixed_time=0.0, prefetch=False,
                            assignment="dynamic", store=store)
    with open(f"{out}.rank{rank}.json", "w") as f:
        json.dump(dict(groups_claimed=res["groups_claimed"], frames=int(res["stats"][rank, 1])), f)
    if rank == 0:
        with open(out, "w+") as f:
            f.writelines(res["csv_lines"])
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
