import sys, numpy as np, torch
sys.path.insert(0, "go-jpeg2000_amd")
from j2kgfx.codec import FramePlan
plans = [FramePlan(512, 512, 3, precision=8, lossless=True, num_resolutions=4, cb=(64, 64), tile=(0, 0), coder=1) for _ in range(3)]
x = torch.zeros((3, 512, 512), dtype=torch.int32, device=plans[0].device)
c = plans[0].forward(x)
# a graph whose plan was closed under it: stale (j2k_graph_stale: 3), never launched, never closed, alive at interpreter shutdown
c1 = plans[1].forward(x)
plans[1].ctx.sync()
with plans[1].ctx.capture() as g:
    plans[1].forward(x, c1)
plans[1].close()
assert g.stale == 3
keep = (plans, c, c1, g)   # alive at interpreter shutdown, never closed, work possibly still queued
raise SystemExit(3)
