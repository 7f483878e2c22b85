"""Generates tests/golden/gridmap_ref_recorded.npz from the REFERENCE's own grid_map_core, MapUpdater::lineOnMap and
RrtPlanner::makePlan (oracle/_ref/libref_gridmap.so, built by `make -C oracle ref` where the reference sources are
present): its answers to the fixed-seed cases of tests/test_oracle_refpin.py, so that those tests also run where
oracle/_ref is not built.  Also writes tests/golden/submap_far_edge_case.npz, the getSubmap input on which the oracle
once disagreed with the reference.  The fixtures are data only (the reference's outputs and a digest of the inputs
they answer).

    python tests/golden/gen_gridmap_ref_recorded.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle as O  # noqa: E402
import test_oracle_refpin as T  # noqa: E402


def main():
    assert O.ref_gridmap() is not None, "build oracle/_ref first (make -C oracle ref)"
    out = {"inputs_sha256": np.array(T.inputs_digest())}
    for f in T.FAMILIES:
        out.update(T.answers(f, True))
    np.savez_compressed(os.path.join(HERE, "gridmap_ref_recorded.npz"), **out)
    print("wrote gridmap_ref_recorded.npz:", {k: v.shape for k, v in out.items()})

    c = T.SUBMAP_FAR_EDGE_CASE
    g = O.make_geom(*c["geometry"])
    layer = np.arange(g.size[0] * g.size[1], dtype=np.float32)
    ok, sub, data = O.get_submap(g, layer, c["center"], c["length"], reference=True)
    assert ok
    np.savez_compressed(os.path.join(HERE, "submap_far_edge_case.npz"), geometry=np.array(c["geometry"][:3], np.float64),
                        position=np.array(c["geometry"][3:], np.float64), center=np.array(c["center"], np.float64),
                        length=np.array(c["length"], np.float64), layer=layer,
                        ref_geom=np.array(list(sub.len) + list(sub.pos) + [sub.res] + list(sub.size), np.float64),
                        ref_data=data)
    print("wrote submap_far_edge_case.npz")


if __name__ == "__main__":
    main()
