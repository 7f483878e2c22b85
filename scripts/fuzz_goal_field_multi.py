"""Developer tool: time-boxed random parity run of the goal field with many sources (rna_goal_field_build_multi,
csrc/goal_field.hip) against the plain-Python oracle of tests/test_gpu_goal_field_multi.py: every cell of field, next and
owner, the counts of both info records, over random map shapes (not multiples of the 64-cell tile), obstacle densities,
unknown cells, robot radii, moved maps, clearance-cost tables, tile-ordering widths, 1-2000 sources with random start costs,
duplicates and blocked cells among them, owners on or off, host or device form.
usage: python scripts/fuzz_goal_field_multi.py [seconds] [seed]
Exits non-zero on the first mismatch and prints the configuration that reproduces it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (initialises the HIP runtime before librna.so loads)
import ros_navigation_amd as R  # noqa: E402
from _gpu import TABLE, Hip  # noqa: E402
from test_gpu_goal_field_multi import LIMIT, Want  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.zeros(1, device="cuda")
hip = Hip()
rng = np.random.default_rng(seed)
t_end = time.time() + budget
fields = cells = sources = maps = moved = with_radius = with_table = with_owners = on_device = 0


def fail(what, here, *more):
    print("MISMATCH", what, here, *more)
    sys.exit(1)


while time.time() < t_end:
    rows, cols = int(rng.integers(3, 260)), int(rng.integers(3, 260))
    density = float(rng.choice([0.0, 0.05, 0.2, 0.3, 0.45, 0.6]))
    side_hi = int(rng.integers(2, max(3, min(rows, cols) // 3 + 2)))
    mseed = int(rng.integers(0, 1 << 30))
    master = R.synth.obstacles_rect(rows, cols, density=density, seed=mseed, side=(1, side_hi)).copy()
    if rng.random() < 0.5:
        m2 = master.reshape(cols, rows)
        m2[0, :] = m2[-1, :] = m2[:, 0] = m2[:, -1] = 0.0       # no border wall (it would lie along a moved map's seam)
    if rng.random() < 0.5:
        master[rng.random(rows * cols) < 0.05] = np.nan
    e = R.Engine(rows * 0.05, cols * 0.05, 0.05)
    assert (e.rows, e.cols) == (rows, cols)
    cfg = dict(rows=rows, cols=cols, density=density, side_hi=side_hi, mseed=mseed, fuzz_seed=seed, field=fields)
    if rng.random() < 0.4:
        # moved first, filled afterwards: the buffer holds the random map whatever the start index is
        target = (float(rng.uniform(-0.4, 0.4) * rows * 0.05), float(rng.uniform(-0.4, 0.4) * cols * 0.05))
        e.move(*target)
        cfg["moved_to"] = target
        moved += 1
    e.upload(R.capi.LAYER_MASTER, master)
    if rng.random() < 0.3:
        r = float(rng.choice([0.05, 0.1, 0.3])) if min(rows, cols) > 20 else 0.05
        e.astar_robot_radius(r)
        cfg["radius"] = r
        with_radius += 1
    table = None
    if rng.random() < 0.3:
        table = TABLE[:int(rng.integers(2, len(TABLE) + 1))]
        e.goal_field_clearance_cost(table)
        cfg["table"] = len(table)
        with_table += 1
    blocked = e.astar_blocked_mask()
    free = np.flatnonzero(blocked == 0)
    maps += 1
    for rep in range(int(rng.integers(1, 4))):
        n = int(rng.choice([1, 2, 3, 17, 200, 2000])) if rng.random() < 0.5 else int(rng.integers(1, 2001))
        n = min(n, rows * cols)
        anywhere = rng.integers(0, rows * cols, n)
        goals = np.where(rng.random(n) < 0.9, rng.choice(free, n), anywhere) if len(free) else anywhere
        if n > 3 and rng.random() < 0.5:
            goals[rng.integers(0, n, n // 3)] = goals[rng.integers(0, n, n // 3)]       # duplicates
        kind = rng.random()
        seeds = None if kind < 0.2 else rng.integers(0, 3000 if kind < 0.6 else (200000 if kind < 0.95 else LIMIT), n)
        owners = bool(rng.random() < 0.7)
        device = bool(rng.random() < 0.3)
        width = int(rng.choice([0, 3000, 64000, 256000]))
        os.environ["RNA_GOAL_FIELD_WIDTH"] = str(width)
        here = dict(cfg, n=n, gseed=int(goals[0]), owners=owners, device=device, width=width,
                    seeds=None if seeds is None else int(seeds.max()))
        g32 = goals.astype(np.int32)
        s32 = None if seeds is None else seeds.astype(np.int32)
        if device:
            d_g, d_s = hip.upload(g32), (None if s32 is None else hip.upload(s32))
            info = e.goal_field_multi_device(d_g, d_s, n, owners=owners)
            hip.free(d_g)
            if d_s:
                hip.free(d_s)
            on_device += 1
        else:
            info = e.goal_field_multi(g32, s32, owners=owners)
        w = Want(e, g32, s32, table)
        field, nx = e.goal_field_download(want_next=True)
        for what, got, want in (("field", field, w.field), ("next", nx, w.next)) + ((("owner", e.goal_field_owners(), w.owner),) if owners else ()):
            bad = np.flatnonzero(got != want)
            if bad.size:
                fail(what, here, bad[:8], got[bad[:8]], want[bad[:8]], "goals", g32[:16], "seeds", None if s32 is None else s32[:16])
        src = e.goal_field_sources_info()
        status = 2 if w.blocked_sources == n else 0
        if (info["goal"], info["status"], info["reached"], info["max_cost"]) != (int(g32[0]), status, w.reached, w.max_cost):
            fail("info", here, info, w.reached, w.max_cost)
        if (src["sources"], src["blocked_sources"], src["terminals"], src["owners"]) != (n, w.blocked_sources, w.terminals, int(owners)):
            fail("sources info", here, src, w.blocked_sources, w.terminals)
        if owners and src["owner_rounds"] > int(np.ceil(np.log2(max(2, rows * cols)))) + 1:
            fail("owner rounds", here, src)
        fields += 1
        cells += rows * cols
        sources += n
        with_owners += int(owners)
    e.close()
print("fuzz ok: %d fields (%d cells, %d sources; %d with owners, %d through the device form) on %d maps: %d moved, %d with a robot radius, "
      "%d with a clearance cost, in %.0f s, seed %d" % (fields, cells, sources, with_owners, on_device, maps, moved, with_radius, with_table,
                                                        budget, seed))
