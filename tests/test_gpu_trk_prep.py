"""The epoch prep kernel's two forms, table against table: the chunk-in-LDS, pipelined form (the default) must leave the SM and GRAM
tables of the first form (AICAM_TRK_PREP_V1=1) bit for bit -- the same MFMA, operand roles and K walk per dot product, only the dealing
of the work and the order of the (exact, order-free) fminf merge differ.  Shapes at the edges of the tiling (tests/trk_prep_cases.py):
1 / 30 / 64 tracks; galleries of 1, 15, 16, 17 and 100 rows with the ring wrapped, one empty, and 112 / 113 / 130 rows at gmax 130;
1, 31, 32, 33 and 480 epoch rows; k = 1 and 16; dim 512, 128 and 80 (the guarded tail); the bank form with three streams, one of them
without SM work.  Each table is also held against float64 where it is written, and must hold -1 everywhere else."""
import os
import subprocess
import sys

import numpy as np
import pytest

import trk_prep_cases as P
import trk_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = np.float32(3.0e38)


@pytest.fixture(scope="module")
def tables(gpu, tmp_path_factory):
    """(second form, first form): what a child process per form leaves for every case."""
    work = tmp_path_factory.mktemp("trk_prep")
    out = []
    for tag, env in (("new", {}), ("v1", {"AICAM_TRK_PREP_V1": "1"})):
        path = str(work / f"{tag}.npz")
        e = {k: v for k, v in os.environ.items() if k not in ("AICAM_TRK_PREP_V1", "AICAM_TRK_PREP_REPEAT")}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "trk_prep_cases.py"), path], env=dict(e, **env), capture_output=True,
                           text=True, timeout=300)
        if r.returncode < 0 or r.returncode in (134, 139):
            pytest.exit(f"prep child ({tag}) died with {r.returncode}, stopping: {r.stderr[-600:]}", returncode=1)
        assert r.returncode == 0, (tag, r.stdout[-600:], r.stderr[-1200:])
        out.append(np.load(path))
    return out


def expected(case, a, s):
    """float64 SM [T, k + 1, dn] and GRAM [dn, dn] of stream s, NaN where the kernel writes nothing."""
    T, dn, k = case.tracks[s], case.dn[s], case.k
    m0 = int(np.sum(case.dn[:s])) if case.bank else 0
    rows = a["row_map"][m0:m0 + dn] if case.bank else np.arange(dn)
    det = a["feat"][rows].astype(np.float64)
    sm = np.full((T, k + 1, dn), np.nan)
    for t in range(T):
        slot, glen, head = a["sgh"][s, t]
        sm[t, glen:] = BIG                                            # empty suffix
        if glen:
            fifo = a["gal"][s, slot, (head + np.arange(glen)) % case.gmax].astype(np.float64)
            d = np.maximum(0.0, 1.0 - fifo @ det.T)                  # [glen, dn]
            suffix = np.minimum.accumulate(d[::-1], axis=0)[::-1]
            sm[t, :min(glen, k + 1)] = suffix[:k + 1]
    gram = np.maximum(0.0, 1.0 - det @ det.T)
    return sm, gram


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_second_form_equals_first(tables, case):
    new, v1 = tables
    a = P.build(case)
    sm, gram = new[case.id + "_sm"], new[case.id + "_gram"]
    # ---- the claim: bit for bit, written cells and untouched cells alike
    assert np.array_equal(sm, v1[case.id + "_sm"]), case.id
    assert np.array_equal(gram, v1[case.id + "_gram"]), case.id
    # ---- the case is what its name says
    sgh = np.concatenate([a["sgh"][s, :case.tracks[s]] for s in range(case.streams)])
    if len(sgh) > 1:
        assert (sgh[:, 1] + sgh[:, 2] > case.gmax).any(), "no gallery wraps"
        assert (sgh[:, 1] == 0).any(), "no empty gallery"
        assert not np.array_equal(sgh[:, 0], np.arange(len(sgh))), "slots in list order"
    elif len(sgh) == 1:
        assert sgh[0, 1] == case.gmax and sgh[0, 1] + sgh[0, 2] > case.gmax
    assert case.dim % 4 == 0 and (case.dim != 80 or case.dim % 64 == 16)
    if case.bank:
        assert case.streams == 3 and 0 in case.has_sm and not np.array_equal(a["row_map"], np.arange(len(a["row_map"])))
    # ---- each stream's tables: float64 where written, -1 elsewhere
    bound = R.app_bound(case.dim)                                    # covers the dot product of two fp32 unit rows and the 1 - dot rounding
    for s in range(case.streams):
        if case.bank and not case.has_sm[s]:
            assert (sm[s] == -1).all() and (gram[s] == -1).all(), (case.id, s)
            continue
        T, dn, k = case.tracks[s], case.dn[s], case.k
        pitch = max(32, (dn + 31) // 32 * 32)                        # the stream's own pitch, from the start of its slice
        sm_s = sm[s].reshape(-1)[:a["cap"] * (P.KMAX + 1) * pitch].reshape(a["cap"], P.KMAX + 1, pitch)
        gram_s = gram[s].reshape(-1)[:pitch * pitch].reshape(pitch, pitch)
        want_sm, want_gram = expected(case, a, s)
        assert (sm_s[T:] == -1).all() and (sm_s[:T, k + 1:] == -1).all(), (case.id, s)
        got = sm_s[:T, :k + 1, :dn].astype(np.float64)
        big = want_sm == BIG
        assert np.array_equal(got == BIG, big), (case.id, s)
        err = float(np.abs(got - want_sm)[~big].max()) if (~big).any() else 0.0
        # GRAM: a 16-row group is written against a 32-column chunk unless all its rows are later than all the chunk's columns
        ri, ci = np.arange(pitch)[:, None] // 16, np.arange(pitch)[None, :] // 32
        written = ri <= 2 * ci + 1
        assert np.array_equal(gram_s != -1, written), (case.id, s)
        live = written[:dn, :dn]
        err_g = float(np.abs(gram_s[:dn, :dn].astype(np.float64) - want_gram)[live].max())
        print(f"{case.id} stream {s}: SM {err:.2e}, GRAM {err_g:.2e} of {bound:.2e}")
        assert err <= bound and err_g <= bound, (case.id, s, err, err_g, bound)
