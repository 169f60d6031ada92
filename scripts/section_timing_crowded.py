"""Development helper: scripts/section_timing.py with a chosen episode of the bench workload in block 0, the block whose waves
the FS_TIMING build prints.  Block 0 of the bench is a light episode; a launch lasts as long as its most crowded ones
(scripts/block_clocks.py names them: seed 148 at frame 81), and the sections that grow with the candidate lists -- sort, hist +
allot, words -- are only seen at their launch-setting size there.
usage: FLINGSIM_LIB=variants/libfs_timing.so section_timing_crowded.py [seed for block 0, default 148]
The episode with that seed and episode 0 change places; every other block keeps its own."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench
from flingbot_amd import sim as fsim

E = 256
seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 148
ctx = fsim.FlingSim(n_envs=E, solver=int(os.environ.get("FS_SOLVER", "2")))
for e in range(E):
    bench.setup_episode(ctx.env(e), seed0 if e == 0 else 0 if e == seed0 else e)
os.environ["FS_QUIET"] = "1"
fd = os.dup(1); devnull = os.open(os.devnull, os.O_WRONLY)
os.dup2(devnull, 1)          # silence the warm-up launches' device printf
ctx.step(80); ctx.sync()
sys.stdout.flush(); os.dup2(fd, 1)
ctx.step(1); ctx.sync()
cnt, _ = ctx.get_last_neighbors(0)
print("block 0 = seed %d: %d particles with candidates, %d lists longer than 4, longest %d" % (
    seed0, int((cnt > 0).sum()), int((cnt > 4).sum()), int(cnt.max())))
