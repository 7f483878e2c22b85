"""Generates tests/golden/vfh_ref_recorded.npz from the REFERENCE's own vfh.cpp (oracle/_ref, built by
`make -C oracle ref` where the reference sources are present): its answers to the fixed-seed fuzz of
tests/test_oracle_vfh.py and its precomputed tables, so that those tests also run where oracle/_ref is not built.
The fixture is data only (the reference's outputs and a digest of the inputs they answer).  Run it in a fresh process:
the reference's pinned clock is one per process.

    python tests/golden/gen_vfh_ref_recorded.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle as O  # noqa: E402
import test_oracle_vfh as T  # noqa: E402


def main():
    assert O.ref() is not None, "build oracle/_ref first (make -C oracle ref)"
    answers = T.reference_fuzz_answers()
    out = {"fuzz_inputs_sha256": np.array(T.fuzz_inputs_digest()),
           "fuzz_chosen_speed": np.array([a[0] for a in answers], np.int32),
           "fuzz_chosen_turnrate": np.array([a[1] for a in answers], np.int32),
           "fuzz_hist": np.stack([a[2] for a in answers]).astype(np.float32),
           "fuzz_origin_hist": np.stack([a[3] for a in answers]).astype(np.float32),
           "fuzz_picked": np.array([a[4] for a in answers], np.float32)}
    out.update({"tables_" + k: v for k, v in T.reference_tables().items()})
    np.savez_compressed(os.path.join(HERE, "vfh_ref_recorded.npz"), **out)
    print("wrote vfh_ref_recorded.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
