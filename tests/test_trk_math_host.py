"""csrc/trk_math.hpp on the CPU: the one copy of the xyah Kalman filter, the gate, the box of a mean and 1 - IoU that every
DeepSORT-family kernel calls, compiled by the system compiler into tests/trk_math_probe.cpp (-ffp-contract=off, address and
undefined-behaviour sanitizers, a child process of its own) and run ONCE on everything below.

  the wave form (the per-lane compute part for lanes 0 .. 63, then the stores: kf_*_wave emulated) and the row form (gain row, S K and mean
      element once per row, kf_cov_elem per element: the thread-per-row update of trk_epoch_kernel) agree bit for bit on every case and on
      the planted frame's predicted states; on the device only test_epoch_kernel_both_update_forms holds the two together, at 192 / 193 tracks
  initiate and predict at dt = 1 are the restatement's bits (oracle.deepsort_oracle.kf_initiate / kf_predict), the claim
      test_form1_bit_equal_to_restatement makes on the device
  every operation against kf_ref's float64 inside the allowance tests/test_kf_ref.py derives: max(4 x the fp32 NumPy restatement's
      figure, 8 x 2^-24) -- no tolerance of this file's own
  mean_box and iou_dist are O.mean_to_tlwh's and O.iou_cost_matrix's bits, a mean with h <= 0 and a pair with zero union among them."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import kf_ref as K
from conftest import ROOT
from oracle import deepsort_oracle as O
from test_kf_ref import OracleKF, base_plan, oracle_figures

F32 = np.float32
INITIATE, PREDICT, PROJECT, UPDATE, GATING, BOXES = range(6)


class Probe:
    """Jobs for one run of the probe.  While `results` is None a call only records its job and answers zeros of the right shapes; after
    run() the same calls in the same order are answered from the results, so kf_ref.measure and kf_ref.gate_runs drive it as they stand."""

    def __init__(self):
        self.jobs, self.shapes, self.results, self.cursor = [], [], None, 0

    def job(self, op, n, m, flag, dt, arrays, shapes):
        if self.results is None:
            self.jobs.append(struct.pack("<4if", op, n, m, flag, dt) + b"".join(np.ascontiguousarray(a, F32).tobytes() for a in arrays))
            self.shapes.append(shapes)
            return [np.zeros(s, F32) for s in shapes]
        assert shapes == self.shapes[self.cursor], "replay out of step"
        self.cursor += 1
        return self.results[self.cursor - 1]

    def run(self, exe, tmp):
        jobs, res = str(tmp / "jobs.bin"), str(tmp / "results.bin")
        with open(jobs, "wb") as f:
            f.write(b"".join(self.jobs))
        r = subprocess.run([exe, jobs, res], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
        flat = np.fromfile(res, F32)
        assert flat.size == sum(int(np.prod(s)) for shapes in self.shapes for s in shapes)
        self.results, at = [], 0
        for shapes in self.shapes:
            out = []
            for s in shapes:
                out.append(flat[at:at + int(np.prod(s))].reshape(s))
                at += int(np.prod(s))
            self.results.append(out)

    # the interface kf_ref.measure / gate_runs take
    def initiate(self, z):
        n = len(z)
        return tuple(self.job(INITIATE, n, 0, 0, 1.0, [z], [(n, 8), (n, 8, 8)]))

    def predict(self, mean, cov, dt=1.0):
        n = len(mean)
        return tuple(self.job(PREDICT, n, 0, 0, float(F32(dt)), [mean, cov], [(n, 8), (n, 8, 8)]))

    def project(self, mean, cov):
        n = len(mean)
        return tuple(self.job(PROJECT, n, 0, 0, 1.0, [mean, cov], [(n, 4), (n, 4, 4)]))

    def update_both(self, mean, cov, z):
        n = len(mean)
        return self.job(UPDATE, n, 0, 0, 1.0, [mean, cov, z], [(n, 8), (n, 8, 8), (n, 8), (n, 8, 8)])

    def update(self, mean, cov, z):
        return tuple(self.update_both(mean, cov, z)[:2])

    def gating(self, mean, cov, zs, shared_z, only_position):
        n, m = len(mean), zs.shape[-2]
        return self.job(GATING, n, m, int(shared_z) | 2 * int(only_position), 1.0, [mean, cov, zs], [(n, m)])[0]

    def boxes(self, mean, det):
        n, m = len(mean), len(det)
        return self.job(BOXES, n, m, 0, 1.0, [mean, det], [(n, 4), (n, m)])


def box_inputs():
    """Means: every case state, its predicted state (two of them predict h <= 0), one with h exactly 0.  Boxes: the planted frame's
    detections, the tlwh of a few of the means themselves, and an empty box on the h = 0 mean's corner (zero union)."""
    mean = [c.mean for c in K.CASES] + [O.kf_predict(c.mean, c.cov)[0].astype(F32) for c in K.CASES]
    flat = K.CASES[0].mean.copy()
    flat[3] = 0
    mean.append(flat)
    mean = np.stack(mean).astype(F32)
    own = np.stack([O.mean_to_tlwh(m) for m in mean[::9]])
    det = np.concatenate([base_plan().det, own, [[flat[0], flat[1], 0, 0]]]).astype(F32)
    return mean, det


def everything(p):
    """The calls of one pass, in one order: recorded on the first pass, answered on the second."""
    mean, cov, z = K.batch(range(len(K.CASES)))
    out = dict(cases=(mean, cov, z))
    out["initiate"] = p.initiate(z)
    out["predict"] = p.predict(mean, cov)
    out["update"] = p.update_both(mean, cov, z)
    plan = base_plan()
    ts = sorted(plan.pair)
    pm, pp = OracleKF().predict(plan.mean[ts], plan.cov[ts])
    out["planted"] = p.update_both(pm, pp, K.xyah32(plan.det)[[plan.pair[t] for t in ts]])
    out["measure"] = K.measure(p)
    out["gate"] = K.gate_runs(p.gating)
    out["box_inputs"] = box_inputs()
    out["boxes"] = p.boxes(*out["box_inputs"])
    return out


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the tracker-math host test builds tests/trk_math_probe.cpp with the system compiler")
    tmp = tmp_path_factory.mktemp("trk_math")
    exe = str(tmp / "trk_math_probe")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "trk_math_probe.cpp"), "-o", exe], check=True)
    p = Probe()
    with np.errstate(all="ignore"):
        everything(p)                                                   # records; the zeros it answers with mean nothing
    p.run(exe, tmp)
    out = everything(p)
    assert p.cursor == len(p.jobs)
    return out


def test_wave_form_and_row_form_are_bit_equal(probed):
    for key in ("update", "planted"):
        wm, wc, rm, rc = probed[key]
        assert len(wm) >= 28 and np.isfinite(wc).all()
        assert np.array_equal(wm, rm) and np.array_equal(wc, rc), key
    mean, cov, _ = probed["cases"]
    assert not np.array_equal(probed["update"][1], cov)                 # an update did happen


def test_initiate_and_predict_are_the_restatements_bits(probed):
    mean, cov, z = probed["cases"]
    orc = OracleKF()
    for got, want in ((probed["initiate"], orc.initiate(z)), (probed["predict"], orc.predict(mean, cov))):
        assert want[0].dtype == F32 and want[1].dtype == F32
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_every_operation_against_fp64(probed):
    fig, _ = oracle_figures()
    dev = probed["measure"]
    assert set(dev) == set(fig) - {"gating"}
    for k in sorted(dev):
        print(f"trk_math.hpp on the host, {k}: covariance {dev[k][0]:.2e} of {K.allow(fig[k][0]):.2e}, mean {dev[k][1]:.2e} of {K.allow(fig[k][1]):.2e}")
    for k in dev:
        assert dev[k][0] <= K.allow(fig[k][0]) and dev[k][1] <= K.allow(fig[k][1]), (k, dev[k], fig[k])
    plan = base_plan()                                                  # the planted frame's updates, from the fp32 predicted state
    ts = sorted(plan.pair)
    z = K.xyah32(plan.det)
    pm, pp = OracleKF().predict(plan.mean[ts], plan.cov[ts])
    e = [K.update_errs(probed["planted"][0][i], probed["planted"][1][i], pm[i], pp[i], z[plan.pair[t]]) for i, t in enumerate(ts)]
    assert max(a for a, _ in e) <= K.allow(fig["update"][0]) and max(b for _, b in e) <= K.allow(fig["update"][1])


def test_gating_against_fp64(probed):
    fig, _ = oracle_figures()
    recs = probed["gate"]
    dev = K.gate_figure(recs)                                           # (also asserts that exactly the +inf cells of float64 are +inf)
    print(f"trk_math.hpp on the host, gating: {dev:.2e} of {K.allow(fig['gating']):.2e} over {sum(r[5].size for r in recs)} cells")
    assert dev <= K.allow(fig["gating"])
    for r, s in zip(recs, K.gate_sure(recs, fig["gating"])):
        assert np.array_equal((r[6] > K.CHI2_4)[s], (r[5] > K.CHI2_4)[s]), r[:5]


def test_mean_box_and_iou_dist_are_the_restatements_bits(probed):
    mean, det = probed["box_inputs"]
    box, cost = probed["boxes"]
    want = np.stack([O.mean_to_tlwh(m) for m in mean])
    assert want.dtype == F32 and np.array_equal(box, want)
    assert (mean[:, 3] < 0).any() and (mean[:, 3] == 0).any() and (want[mean[:, 3] <= 0, 2:] == 0).all()      # h <= 0: an empty box
    ref = O.iou_cost_matrix(list(want), det)
    assert ref.dtype == F32 and np.array_equal(cost, ref)
    union = want[:, None, 2] * want[:, None, 3] + det[None, :, 2] * det[None, :, 3]
    assert (union == 0).any() and (cost[union == 0] == 1).all()          # zero union: 0 / 1e-7
    assert (cost == 0).any() and ((cost > 0) & (cost < 1)).any()         # a box on itself, and partial overlaps
