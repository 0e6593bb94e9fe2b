"""The ByteTrack and BoT-SORT epoch kernels (csrc/byte_epoch.hpp through csrc/kernels_bytetrack.hip and csrc/kernels_botsort.hip) replay
the scenes of tests/byte_family_cases.py and must give what tests/golden/byte_family_state.npz recorded at the kernels before the
shared skeleton: every frame's rows and conf, the final export() (mean, cov, smoothed features, ...) and the counters, floats compared
as bits.  The oracle tests allow the ByteTrack Kalman state a tolerance; this file allows nothing."""
import numpy as np
import pytest

import byte_family_cases as C

pytestmark = pytest.mark.gpu

RUNS = dict(C.runs())
_GOT = {}


def replay(run):
    """The device's record of a run, made once."""
    if run not in _GOT:
        _GOT[run] = RUNS[run]()
    return _GOT[run]


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("byte_family_state")


@pytest.mark.parametrize("run", list(RUNS))
def test_replay_equals_the_recorded_bits(fixture, run):
    got, want = replay(run), C.expected(fixture, run)
    assert got.keys() == want.keys() and len(got) > 10
    for key in got:
        assert C.same_bits(np.asarray(got[key]), want[key]), (run, key)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("lsap_fast,epoch_frames", C.CONFIGS)
def test_device_met_the_promised_regimes(kind, lsap_fast, epoch_frames):
    """The counters show the problems and the largest side the oracles promise (tests/test_byte_family_cases.py holds those to the four
    regimes); without the read-off every one of them went through the LSAP of its regime."""
    def check(c, sid):
        problems, side = C.PROMISED[kind][sid]
        assert c["max_side"] == side and c["n_fast"] + c["n_lsap"] == problems, (sid, c)
        assert lsap_fast or c["n_fast"] == 0, (sid, c)

    cfg = f"fast{lsap_fast}_epoch{epoch_frames}"
    for fs in C.SCENES:
        rec = replay(f"{kind}/{fs.id}/{cfg}")
        check({k: int(rec["final/counters/" + k]) for k in ("n_fast", "n_lsap", "max_side")}, fs.id)
    rec = replay(f"{kind}/bank/{cfg}")
    for s, sid in enumerate(C.BANK):
        check({k: int(rec[f"stream{s}/final/counters/{k}"]) for k in ("n_fast", "n_lsap", "max_side")}, sid)
