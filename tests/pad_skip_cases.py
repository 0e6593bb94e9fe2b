"""Cases of tests/test_gpu_pad_skip.py and the child process that runs them.  The kernel choices under test are read once per process
(AICAM_PP_MIN=0: the patch kernels take their layers at any batch; AICAM_NO_PAD_SKIP=1: row-piece tiles and every tap, as before the
column tiles), so the test starts this file twice -- column tiles on and off -- and compares what the two leave behind:

    python tests/pad_skip_cases.py OUT.npz REID_ENGINE WORKDIR

Per case the child writes the planned form of the layer under test, the layer's input tensors for the P distinct images, and the
layer's output tensor: whole for the small cases, for the large one its first P images, whether all n images repeat them bit for bit,
and a SHA-256 of the whole tensor.  A case under a device-side count first runs other images of the same shape without a count and
keeps what that leaves in the output tensor ("dirty").  Last, the seeded ReID engine's embeddings of 24 and 416 crops."""
import hashlib
import json
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_ref as R          # noqa: E402

ef = R.ef
P = 9                         # distinct images: more than the 8 images of an 8 x 4 block, so no two images of a block are equal
NI = {(16, 8): 2, (8, 4): 8}  # images per 256-pixel block
REID_CROPS = (24, 416)


@dataclass
class PadCase:
    id: str
    H: int                    # the map of the layer under test
    W: int
    n: int
    res: bool = False
    live: int = -1            # device-side item count (>= 0), below the bound n
    big: bool = False         # the block's run of tiles is longer than one and the last run ends inside it

    @property
    def form(self):
        return dict(form="SpPatch", th=self.H, tw=self.W)

    def conv_case(self):
        """The conv_ref case of a plain layer: 128 -> 256 on the map, ReLU, optional residual from a second stem."""
        return R.Case(self.id, self.H, self.W, 128, 256, self.n, self.form, act=R.RELU, res=ef.RES_ADD_THEN_ACT if self.res else 0, P=P,
                      seed=100 + len(self.id))


def _cases():
    C = []
    for (h, w), ni in NI.items():
        m = f"{h}x{w}"
        C.append(PadCase(f"sp_{m}_n1", h, w, 1))
        C.append(PadCase(f"sp_{m}_last_tile_one_image", h, w, 3 * ni + 1))
        C.append(PadCase(f"sp_{m}_res", h, w, 3 * ni + 1, res=True))
        # 2047 tiles: the planner deals runs of two (conv_plan.cpp tile_run: four rounds of blocks at least), the last run holds one tile
        C.append(PadCase(f"sp_{m}_run_ends_mid_run", h, w, 2046 * ni + 1, big=True))
        C.append(PadCase(f"sp_{m}_res_count", h, w, 3 * ni + 1, res=True, live=ni + 1))
    return C


CASES = _cases()


def build(c: PadCase):
    """-> (conv_ref.Built, name of the layer under test, conv_ref.Case for the images)"""
    rc = c.conv_case()
    return R.build_graph(rc), "layer", rc


def inputs_of(c: PadCase):
    return ("x", "r") if c.res else ("x",)


def reference(c: PadCase, B, layer, read):
    """fp64 reference and derived tolerance of the layer's output for the P distinct images; read(name) -> fp64 [P, h, w, c]."""
    l = B.layers[layer]
    return R.layer_ref(read("x"), l["w"], l["b"], 3, 1, R.RELU, "fp16", res=read("r") if c.res else None, res_mode=l["res_mode"])[:2]


def reid_crops(n):
    return np.random.default_rng(11).standard_normal((n, 3, 128, 64)).astype(np.float32)


def _periodic(a, p):
    return all(np.array_equal(R.bits(a[j::p]), np.broadcast_to(R.bits(a[j]), a[j::p].shape)) for j in range(min(p, len(a))))


def main(out_path, reid_engine, work):
    import importlib
    HipEngine = importlib.import_module("ai-camera_amd.hip_engine").HipEngine
    rec = {}
    for c in CASES:
        B, layer, rc = build(c)
        path = os.path.join(work, c.id + ".aicw")
        ef.write_engine(path, B.g)
        base, x = R.images(rc)
        p = len(base)
        eng = HipEngine(path, dtype="fp16", max_items=c.n, warm_up=False)
        try:
            rec[c.id + "/plan"] = json.dumps(eng.conv_plan(B.layers[layer]["op"], c.n, live=c.live >= 0))
            if c.live >= 0:
                eng.reid_infer_np(R.images(rc, salt=1)[1])
                rec[c.id + "/dirty"] = eng.read_buffer_np(B.bufs["out"], c.n)
                emb = eng.reid_infer_np(x, n_live=c.live)
            else:
                emb = eng.reid_infer_np(x)
            rows = c.n if c.live < 0 else c.live
            ok = bool(np.isfinite(emb).all())
            for name in inputs_of(c):
                a = eng.read_buffer_np(B.bufs[name], max(rows, 1))[:rows]
                ok = ok and _periodic(a, p)
                rec[f"{c.id}/in_{name}"] = a[:p]
            out = eng.read_buffer_np(B.bufs["out"], c.n)
            rec[c.id + "/ok"] = np.array(ok and _periodic(out[:rows], p))
            rec[c.id + "/sha"] = np.array(hashlib.sha256(out.tobytes()).hexdigest())
            rec[c.id + "/out"] = out[:p] if c.big else out
        finally:
            eng.close()
    for n in REID_CROPS:
        eng = HipEngine(reid_engine, dtype="fp16", max_items=n, warm_up=False)
        try:
            rec[f"reid/{n}"] = eng.reid_infer_np(reid_crops(n))
        finally:
            eng.close()
    np.savez(out_path, **rec)


if __name__ == "__main__":
    main(*sys.argv[1:4])
