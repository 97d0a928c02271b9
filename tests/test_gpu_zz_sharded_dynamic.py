"""Dynamic frame assignment on the REAL (mini, seeded) models: the four mini frames through
  (a) frame-by-frame FramePipeline calls,
  (b) utils/shard.run_sharded(assignment="dynamic") at world size 2 in groups of 2 (two processes sharing this GPU, gloo record
      gather, the claim counter in a TCPStore: tests/sharded_dynamic_worker.py); which rank takes frames 0,1 and which 2,3 is decided
      at run time
must write the SAME BOP csv, byte for byte (benched dtypes; DESIGN 2: a frame's poses are independent of which frames share its SAM /
PEM batch and of which rank computed them), and each rank must have claimed one of the two groups.  tests/test_dist_dynamic.py checks
the policy itself with a stand-in pipeline on the CPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dynamic_sharded_csv_is_byte_identical_to_frame_by_frame(tmp_path, monkeypatch):
    # the benched extractor, as in tests/test_gpu_zz_sharded.py (the fp32 extractor's rocBLAS kernels follow the row count)
    monkeypatch.setenv("S6D_PEM_VIT_DTYPE", "fp16")
    from sam6d_amd.utils import shard
    from tests.sharded_mini_worker import frame_table
    from tests.test_gpu_zz_pipeline import build_mini, mini_frames
    pipe, frame = build_mini(torch.device("cuda", 0), top_k="keys", sync_stages=False)
    frames = mini_frames(frame)
    ids, load = frame_table(frames)
    blocks = []
    for (s, i), f in zip(ids, frames):
        det, poses = pipe(*f)
        det.scene_id, det.image_id = s, i
        blocks.append(shard.frame_records(det, poses, "ycbv", 0.0))
    csv_a = shard.to_bop_csv_lines(torch.cat(blocks))
    assert len(ids) == 4 and len(csv_a) >= 4, "the mini frames should give at least one pose each"
    # world 1, dynamic: groups in split order, no store
    one = shard.run_sharded(ids, load, pipe, group_size=2, dataset_name="ycbv", device=None, fixed_time=0.0, assignment="dynamic")
    assert one["csv_lines"] == csv_a and one["groups_claimed"] == [0, 1]
    del pipe
    torch.cuda.empty_cache()
    out = str(tmp_path / "w2_dynamic.csv")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, "-m", "tests.sharded_dynamic_worker", out, "2"], cwd=ROOT, env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=600)[0].decode())
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    assert open(out).readlines() == csv_a
    claimed = [json.load(open(f"{out}.rank{r}.json")) for r in range(2)]
    assert sorted(claimed[0]["groups_claimed"] + claimed[1]["groups_claimed"]) == [0, 1], claimed
    assert all(len(c["groups_claimed"]) == 1 and c["frames"] == 2 for c in claimed), claimed
