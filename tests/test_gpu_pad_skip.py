"""Column tiles and halo skipping in the 3x3 patch kernels on ReID's narrow maps (ai-camera_amd/csrc/pad_skip_map.hpp):
the (tile, tap) pairs whose sixteen pixels all read the zero padding issue no MFMA.  Leaving out a tap on a tile that does NOT read only
padding drops real products of border pixels, so every layer here sees a 1x1 linear stem's output -- both signs, non-zero on the map's
border rows and columns (asserted) -- and its OUTPUT TENSOR is compared

  bit for bit  with a child process running AICAM_NO_PAD_SKIP=1 (row-piece tiles, every tap: the kernels as they were), and
  within conv_ref's derived tolerance of the fp64 reference computed from the layer's actual inputs.

Both runs are child processes (tests/pad_skip_cases.py): the switch and AICAM_PP_MIN=0, which lets the patch kernels take these layers
at small n, are read once per process.  The two children run every case once; the tests below read their files.

  map      channels    kernel                                   n
  8 x 4    128 -> 256  v6 (SpPatch), with and without residual  1; 8 k + 1 (the last tile holds one image); 2047 tiles dealt in runs of
  16 x 8   128 -> 256  v6 (SpPatch), with and without residual    two (the last run ends inside it); a device-side count below the bound
(v5, the kernel of the conv2 + downsample layers, keeps its tiles -- DESIGN.md 35 -- and has no case here.)

And the seeded ReID engine at 24 and 416 crops: embeddings equal to the switched-off child's bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_ref as R
import pad_skip_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs(gpu, engines, tmp_path_factory):
    """-> (column tiles on, off): the two children's files"""
    work = tmp_path_factory.mktemp("pad_skip")
    out = []
    for tag, env in (("on", {}), ("off", {"AICAM_NO_PAD_SKIP": "1"})):
        path = str(work / f"{tag}.npz")
        e = {k: v for k, v in os.environ.items() if k != "AICAM_NO_PAD_SKIP"}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pad_skip_cases.py"), path, engines[1], str(work)],
                           env=dict(e, AICAM_PP_MIN="0", **env), capture_output=True, text=True, timeout=600)
        if r.returncode < 0 or r.returncode in (134, 139):
            pytest.exit(f"pad-skip child ({tag}) died with {r.returncode}, stopping: {r.stderr[-600:]}", returncode=1)
        assert r.returncode == 0, (tag, r.stdout[-600:], r.stderr[-1200:])
        out.append(np.load(path))
    return out


@pytest.mark.parametrize("c", PC.CASES, ids=[c.id for c in PC.CASES])
def test_layer_equals_the_unskipped_kernel_and_the_fp64_reference(runs, c):
    on, off = runs
    B, layer, _ = PC.build(c)
    rows = c.n if c.live < 0 else c.live
    p = min(PC.P, c.n)
    # ---- which kernel ran, in both children
    for tag, f in (("on", on), ("off", off)):
        plan = json.loads(str(f[c.id + "/plan"]))
        got = {k: plan.get(k) for k in c.form}
        assert plan["kind"] == "conv" and got == c.form, f"{c.id} ({tag}): expected {c.form}, the engine plans {plan}"
        if c.big:
            tiles = -(-c.n // PC.NI[(c.H, c.W)])
            assert plan["run"] >= 2 and tiles % plan["run"], (c.id, plan)
        assert bool(f[c.id + "/ok"]), f"{c.id} ({tag}): a non-finite embedding, or a tensor that does not repeat the {p} distinct images"
    # ---- inputs: the same in both, and able to show a tap dropped on a border tile
    for name in PC.inputs_of(c):
        a = on[f"{c.id}/in_{name}"]
        assert np.array_equal(R.bits(a), R.bits(off[f"{c.id}/in_{name}"])), (c.id, name)
        for edge in (a[:, 0], a[:, -1], a[:, :, 0], a[:, :, -1]):
            assert (edge != 0).all() and (edge > 0).any() and (edge < 0).any(), f"{c.id}: input {name} cannot show a dropped border product"
    # ---- bit for bit against the kernels without the skipping
    got = on[c.id + "/out"]
    assert str(on[c.id + "/sha"]) == str(off[c.id + "/sha"]) and np.array_equal(R.bits(got), R.bits(off[c.id + "/out"])), \
        f"{c.id}: the output tensor differs from the AICAM_NO_PAD_SKIP=1 run"
    # ---- against the fp64 reference of the layer's actual inputs
    ref, tol = PC.reference(c, B, layer, lambda name: on[f"{c.id}/in_{name}"].astype(np.float64))
    live = got[:p] if c.big else got[:rows]                       # (the large case: all n images repeat these bit for bit, asserted above)
    ratio, where = R.worst_ratio(live, ref[:p], tol[:p])
    print(f"pad skip {c.id} n={c.n}: worst error / tolerance {ratio:.3f} at {where}")
    assert ratio <= 1.0, f"{c.id}: error is {ratio:.3f} x the derived tolerance at (image, y, x, channel) {where}"
    if c.live >= 0:
        dirty = on[c.id + "/dirty"]
        assert np.array_equal(R.bits(got[rows:]), R.bits(dirty[rows:])), f"{c.id}: rows at and past the count were written"
        d_ratio = min(R.worst_ratio(dirty[j:j + 1], ref[j % p:j % p + 1], tol[j % p:j % p + 1])[0] for j in range(rows))
        assert d_ratio > 1.0, f"{c.id}: the dirty tensor is within the tolerance on a live image: a missing store would not show"


@pytest.mark.parametrize("n", PC.REID_CROPS)
def test_reid_embeddings_equal_the_unskipped_kernels(runs, n):
    on, off = runs
    e = on[f"reid/{n}"]
    assert e.shape[0] == n and np.isfinite(e).all() and np.allclose(np.linalg.norm(e, axis=1), 1, atol=1e-3)
    assert np.array_equal(R.bits(e), R.bits(off[f"reid/{n}"])), (n, float(np.abs(e - off[f"reid/{n}"]).max()))
