"""Generates tests/golden/vfh_params_recorded.npz from the REFERENCE's own vfh.cpp (oracle/_ref, built by `make -C oracle ref`
where the reference sources are present): its answers to the sequences of tests/_vfh_cases.py at every parameter set, and
its precomputed tables at three of them, so that tests/test_oracle_vfh_params.py also runs where oracle/_ref is not built.
Data only: per step the chosen speed, the turn rate and the picked angle, per sequence one sha256 over its Hist and OriginHist
bytes, per set a sha256 of the inputs and parameters these answer.  Run it in a fresh process: the reference's pinned clock is
one per process.

    python tests/golden/gen_vfh_params_recorded.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle as O  # noqa: E402
import _vfh_cases as V  # noqa: E402
import test_oracle_vfh as T  # noqa: E402
import test_oracle_vfh_params as TP  # noqa: E402


def main():
    assert O.ref() is not None, "build oracle/_ref first (make -C oracle ref)"
    out = {}
    for name in V.SETS:
        out[name + "_inputs_sha256"] = np.array(V.inputs_digest(name))
        for k, v in TP.reference_answers(name).items():
            out[name + "_" + k] = v
    for name in TP.TABLE_SETS:
        out.update({name + "_tables_" + k: v for k, v in T.reference_tables(V.params(name)).items()})
    path = os.path.join(HERE, "vfh_params_recorded.npz")
    np.savez_compressed(path, **out)
    print("wrote vfh_params_recorded.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
