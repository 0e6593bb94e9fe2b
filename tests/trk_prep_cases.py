"""Cases of tests/test_gpu_trk_prep.py and the child process that runs them.  Which form of the epoch prep kernel a launch takes is read
once per process (AICAM_TRK_PREP_V1=1: the first form), so the test starts this file twice and compares what the two leave behind:

    python tests/trk_prep_cases.py OUT.npz

Per case the child writes the SM and GRAM tables as aic_trk_prep_test returns them: every cell the kernel does not write holds -1
(a cosine distance is never negative), so two forms that write different SETS of cells differ too."""
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KMAX = 16
GLENS = (1, 15, 16, 17, 100, 0)        # both sides of the 16-row group, a full budget, and an empty gallery


@dataclass
class PrepCase:
    id: str
    tracks: tuple                 # live tracks per stream
    dn: tuple                     # epoch rows per stream
    k: int
    dim: int
    gmax: int = 100
    glens: tuple = GLENS
    bank: bool = False
    has_sm: tuple = ()

    @property
    def streams(self):
        return len(self.tracks)


CASES = (
    PrepCase("t30_d480_k16_dim512", (30,), (480,), 16, 512),
    PrepCase("t1_d1_k1_dim512", (1,), (1,), 1, 512, glens=(100,)),
    PrepCase("t64_d33_k16_dim128", (64,), (33,), 16, 128),
    PrepCase("t64_d480_k1_dim128", (64,), (480,), 1, 128),
    PrepCase("t30_d31_k1_dim80", (30,), (31,), 1, 80),
    PrepCase("t30_d32_k16_dim80", (30,), (32,), 16, 80),
    PrepCase("t0_d33_k16_dim128", (0,), (33,), 16, 128),                                  # GRAM alone: the first epoch of a stream
    PrepCase("t30_d33_k16_dim128_g130", (30,), (33,), 16, 128, gmax=130, glens=(130, 113, 112, 1, 0, 17)),   # nine row groups
    PrepCase("bank3_dim128", (30, 64, 1), (33, 31, 32), 16, 128, bank=True, has_sm=(1, 0, 1)),
    PrepCase("bank3_dim512", (1, 30, 30), (480, 1, 32), 16, 512, bank=True, has_sm=(1, 1, 0)),
    PrepCase("bank3_dim80", (64, 30, 30), (31, 33, 1), 1, 80, bank=True, has_sm=(0, 1, 1)),
)


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def build(case):
    """The arguments of aic_trk_prep_test for a case, as a dict of arrays and ints."""
    rng = np.random.default_rng(sum(map(ord, case.id)))
    S = case.streams
    cap = max(max(case.tracks), 1) + 3
    sgh = np.zeros((S, cap, 3), np.int32)
    gal = np.empty((S, cap, case.gmax, case.dim), np.float32)
    for s in range(S):
        gal[s] = unit_rows(rng, cap * case.gmax, case.dim).reshape(cap, case.gmax, case.dim)
        slots = rng.permutation(cap)
        for i in range(case.tracks[s]):
            glen = case.glens[i % len(case.glens)]
            # heads: the last position (any gallery of two rows wraps), 0, and two inside the ring
            head = (case.gmax - 1, 0, case.gmax // 2, 7)[i % 4]
            sgh[s, i] = (slots[i], glen, head)
    dn_pad = max(32, max((d + 31) // 32 * 32 for d in case.dn))
    rows = sum(case.dn) + 5
    feat = unit_rows(rng, rows, case.dim)
    if case.bank:
        perm = rng.permutation(rows)                      # a stream's rows lie anywhere among the call's, in no order
        row_map = np.ascontiguousarray(perm[:sum(case.dn)].astype(np.int32))
    else:
        row_map = np.zeros(1, np.int32)
    return dict(streams=S if case.bank else 0, cap=cap, n_tracks=np.asarray(case.tracks, np.int32), sgh=sgh, gal=gal, gmax=case.gmax,
                dim=case.dim, feat=feat, rows=rows, dn=np.asarray(case.dn, np.int32), row_map=row_map,
                has_sm=np.asarray(case.has_sm if case.bank else (1,), np.int32), k=case.k, dn_pad=dn_pad)


def run(L, a):
    S = max(a["streams"], 1)
    sm = np.empty((S, a["cap"], KMAX + 1, a["dn_pad"]), np.float32)
    gram = np.empty((S, a["dn_pad"], a["dn_pad"]), np.float32)
    L.call("aic_trk_prep_test", 0, a["streams"], a["cap"], L.ptr(a["n_tracks"]), L.ptr(a["sgh"]), L.ptr(a["gal"]), a["gmax"], a["dim"],
           L.ptr(a["feat"]), a["rows"], L.ptr(a["dn"]), L.ptr(a["row_map"]), L.ptr(a["has_sm"]), a["k"], a["dn_pad"], L.ptr(sm), L.ptr(gram))
    return sm, gram


def main(out_path):
    import importlib
    L = importlib.import_module("ai-camera_amd._lib")
    L.load()
    out = {}
    for case in CASES:
        sm, gram = run(L, build(case))
        out[case.id + "_sm"], out[case.id + "_gram"] = sm, gram
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
