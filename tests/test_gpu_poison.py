"""No result depends on uninitialised device memory.

One test per group of tests/poison_scenarios.py.  Each starts the group's children one after the other -- AICAM_POISON_ALLOC=zero, big,
nan, and `dirty` (zero, behind one call of other content on every stateless handle) where the group has one -- and asserts that every
child's allocation probe shows its mode and that every output of big, nan and dirty is the zero child's, byte for byte.  The variable
goes into the children's environment only: the library reads it once per process, and this process must stay as it is.

A child that ends by a signal, runs into its time limit or reports a HIP error ends the session (pytest.exit): nothing more is started
on a device that may have faulted.  A poisoned child that faults is a finding about an uninitialised read -- found by reading the code
of the scenario that ran, never by running it again.

Child times measured on an MI355X are in DESIGN.md section 50; the limits below are those times with generous room."""
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import poison_scenarios as P                                            # noqa: E402

pytestmark = pytest.mark.gpu

GROUP_NAMES = ("detector", "detectors32", "reid", "pipeline", "banks", "analytics", "codecs")
TIMEOUT_S = {"detector": 60, "detectors32": 60, "reid": 60, "pipeline": 90, "banks": 90, "analytics": 90, "codecs": 60}      # seconds per child
PROBE_TIMEOUT_S = 30                       # a child that runs the probe alone: process start and library load, the floor of every child
HIP_ERROR_WORDS = ("AicError", "hipError", "HIP error", "illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")


def run_child(group, out_dir, tag, mode, dirty=False):
    """One child under `timeout`.  Ends the session on a signal, a time limit or a HIP error; fails the test on any other failure."""
    env = {k: v for k, v in os.environ.items() if k != "AICAM_POISON_ALLOC"}
    env["AICAM_POISON_ALLOC"] = mode
    limit = TIMEOUT_S.get(group, PROBE_TIMEOUT_S)
    t0 = time.perf_counter()
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "tests", "poison_scenarios.py"), group, str(out_dir), tag]
    r = subprocess.run(cmd + (["dirty"] if dirty else []), env=env, capture_output=True, text=True)
    tail = (r.stdout[-300:] + r.stderr[-1500:])
    print(f"poison child {group} / {tag}: {time.perf_counter() - t0:.1f} s, status {r.returncode}")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or any(w in tail for w in HIP_ERROR_WORDS):
        pytest.exit(f"poison child {group} / {tag} ended with status {r.returncode} (a signal, its {limit} s limit or a HIP error); "
                    f"stopping, nothing more is started on this device:\n{tail}", returncode=1)
    assert r.returncode == 0, f"child {group} / {tag} failed:\n{tail}"
    return P.load_recording(str(out_dir), tag)


def check_group(group, tmp_path):
    assert "AICAM_POISON_ALLOC" not in os.environ, "this process must not run under the hook: the children get it, one value each"
    recs = {}
    for mode in P.MODES:                                                 # one child at a time
        recs[mode] = run_child(group, tmp_path, mode, mode)
        assert P.probe_shows(mode, recs[mode]), (group, mode, {k: recs[mode][k] for k in P.PROBE_KEYS})
    if group in P.DIRTY:
        recs["dirty"] = run_child(group, tmp_path, "dirty", "zero", dirty=True)
        assert P.probe_shows("zero", recs["dirty"])
    assert len(recs["zero"]) > len(P.PROBE_KEYS), "the group recorded nothing"
    strip = lambda r: {k: v for k, v in r.items() if k not in P.PROBE_KEYS}                  # noqa: E731
    findings = {tag: P.compare(strip(recs["zero"]), strip(recs[tag]), group) for tag in recs if tag != "zero"}
    for tag, f in findings.items():
        print(group, tag, f[:20])
    assert not any(findings.values()), f"{group}: outputs that depend on what memory held: " + "; ".join(
        f"{tag}: {k} {what} at {idx}" for tag, f in findings.items() for k, what, idx in f[:8])
    # positive control: the probe IS an uninitialised read, and the comparer says so with key and index
    probes = lambda r: {k: r[k] for k in P.PROBE_KEYS}                                       # noqa: E731
    for tag in ("big", "nan"):
        f = P.compare(probes(recs["zero"]), probes(recs[tag]))
        assert [(k, what, idx) for k, what, idx in f] == [(k, "bytes", (0,)) for k in sorted(P.PROBE_KEYS)], f


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_outputs_do_not_depend_on_what_memory_held(gpu, tmp_path, group):
    check_group(group, tmp_path)


def test_probe_alone_shows_each_mode(gpu, tmp_path):
    """The hook is live in a child and off in this process's environment; the time of these children is the floor of all the others."""
    assert "AICAM_POISON_ALLOC" not in os.environ
    for mode in P.MODES:
        rec = run_child("probe", tmp_path, mode, mode)
        assert sorted(rec) == sorted(P.PROBE_KEYS) and P.probe_shows(mode, rec), (mode, rec)
        assert [P.probe_shows(m, rec) for m in P.MODES] == [m == mode for m in P.MODES]
