"""Recorder of tests/golden/byte_family_state.npz (run by hand on a gfx950 device, from the repository root):

    python tests/golden/make_byte_family_state.py

Through the public Python classes alone (tests/byte_family_cases.py) it runs every scene on ByteTrack and BoT-SORT under lsap_fast
0 / 1 and epoch_frames 1 / 0, and the two-stream bank, and stores every frame's rows and conf, the final export() and counters()
without the cycle fields, with build.sources_digest() of the tree it ran on.  tests/test_gpu_byte_family_pinned.py replays the
scenes and demands the same bits: the file pins what the epoch kernels computed at the commit whose digest it carries."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import byte_family_cases as C            # noqa: E402
from conftest import pkg                 # noqa: E402


def main(out=os.path.join(HERE, "byte_family_state.npz")):
    records = {name: run() for name, run in C.runs()}
    flat = C.pack(records)
    flat["sources_digest"] = np.array(pkg("build").sources_digest())
    np.savez_compressed(out, **flat)
    print(out, os.path.getsize(out), "bytes,", len(records), "runs, sources_digest", flat["sources_digest"])


if __name__ == "__main__":
    main(*sys.argv[1:2])
