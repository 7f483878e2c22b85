"""Developer tool: time-boxed random run of the engine's map state against the model of tests/_mapmodel.py -- the generator and
the checks of tests/test_gpu_map_sequences.py with fresh seeds: sequences of 14 operations (HIMM on every layer, compose in both
modes, update, upload, fill, moves by a few cells / more than a tile / more than the map / back to start index (0, 0), radius
changes, clones that both go on) on maps of 140 x 96 and 200 x 150 cells, and after every operation geometry, layers, blocked
set, neighbour masks, the dirty-tile report, sixteen searches (every third step pipelined across the next operation) and the
stale flags of clearance, goal field and frontiers (rebuilt after every such check, so that each operation is tried from flags
that read 0); a rebuild of the three through their own checkers at the end.
usage: python scripts/fuzz_map_sequences.py [seconds] [seed] [--masks-only]
--masks-only stops every step after the masks: no search, snapshot or rebuild runs (for trying a deliberately wrong refresh).
Exits non-zero on the first difference and prints the step and the sequence so far as a literal that replays it."""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (initialises the HIP runtime before librna.so loads)
import numpy as np  # noqa: E402
import ros_navigation_amd as R  # noqa: E402
import _mapmodel as M  # noqa: E402
import test_gpu_map_sequences as T  # noqa: E402  (run_sequence: the checks of the suite)

argv = [a for a in sys.argv[1:] if a != "--masks-only"]
masks_only = "--masks-only" in sys.argv[1:]
budget = float(argv[0]) if len(argv) > 0 else 120.0
seed = int(argv[1]) if len(argv) > 1 else 0
torch.zeros(1, device="cuda")
R.capi.lib()
rng = np.random.default_rng(seed)
t_end = time.time() + budget
tally = collections.Counter()
n = 0
while time.time() < t_end:
    shape = M.SHAPES[n % len(M.SHAPES)]
    sseed = int(rng.integers(0, 1 << 30))
    try:
        T.run_sequence(R, shape, sseed, M.generate(shape, sseed), masks_only=masks_only, tally=tally)
    except AssertionError as err:
        print("MISMATCH in sequence %d (fuzz seed %d%s)\n%s" % (n, seed, ", masks only" if masks_only else "", err))
        sys.exit(1)
    n += 1
ops = " ".join("%s:%d" % (k[3:], v) for k, v in sorted(tally.items()) if k.startswith("op "))
composes = " ".join("%s:%d" % (k[8:], v) for k, v in sorted(tally.items()) if k.startswith("compose "))
masks = ", ".join("%d %s" % (v, k) for k, v in sorted(tally.items()) if k.startswith("masks "))
stale = ", ".join("%d %s" % (v, k) for k, v in sorted(tally.items()) if k.startswith("stale "))
print("map sequence fuzz ok: %d sequences%s in %.0f s, seed %d; operations %s; composes by expected path %s; %s; %d searches (%d in "
      "%d pipelined batches); %s" % (tally["sequences"], " (masks only)" if masks_only else "", budget, seed, ops, composes, masks,
                                     tally["searches"], T.NQ * tally["pipelined batches"], tally["pipelined batches"], stale or "no stale checks"))
print("searches with a path %d; cells the rebuilt fields reach %d; frontier cells at the rebuilds %d"
      % (tally["searches with a path"], tally["cells the rebuilt fields reach"], tally["frontier cells at the rebuild"]))
