"""Build libaicam.so in-tree with hipcc for gfx950 (no cmake, no JIT cache).

    python ai-camera_amd/build.py [--force]

One hipcc invocation per translation unit (objects cached under csrc/build/ by mtime), then a
shared link.  -ffp-contract=off everywhere: the integer-exact preprocessing and the association
arithmetic must round like the NumPy oracle; the MFMA kernels are unaffected.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libaicam.so")
SOURCES = ["runtime.cpp", "lsap.cpp", "assoc_host.cpp", "global_id.cpp", "tracker.cpp", "bytetrack.cpp", "ocsort.cpp", "botsort.cpp", "deepsort_bank.cpp", "xcam.cpp", "archive.cpp", "zones.cpp", "bestshot.cpp", "scene.cpp", "left.cpp", "colours.cpp", "heat.cpp", "prox.cpp", "jpeg_host.cpp", "jpeg.cpp", "jpegdec_host.cpp", "jpegdec.cpp","render_host.cpp", "render.cpp", "gmc.cpp", "yuv.cpp", "engine.cpp", "pipeline.cpp", "conv_plan.cpp", "row_band.cpp",
           "kernels_conv.hip", "kernels_conv_pp.hip", "kernels_conv_sp.hip", "kernels_conv_wide.hip", "kernels_conv_direct.hip", "kernels_conv_block.hip", "kernels_conv_c2f.hip", "kernels_elt.hip",
           "kernels_pre.hip", "kernels_det.hip", "kernels_trk.hip", "kernels_trk_dev.hip", "kernels_bytetrack.hip", "kernels_ocsort.hip", "kernels_botsort.hip", "kernels_gmc.hip", "kernels_overlay.hip", "kernels_xcam.hip", "kernels_archive.hip", "kernels_zones.hip", "kernels_bestshot.hip", "kernels_scene.hip", "kernels_left.hip", "kernels_colours.hip", "kernels_heat.hip", "kernels_prox.hip", "kernels_render.hip", "kernels_yuv.hip", "kernels_jpeg.hip", "kernels_jpegdec.hip"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall",
         "-Wno-unused-function", "-Wno-unused-variable", "-DNDEBUG"] + os.environ.get("AICAM_EXTRA_FLAGS", "").split()


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def sources_digest():
    """sha256 over the kernel / host sources the library is built from (names + bytes, sorted).  A measurement that is committed
    as a file (profiles/pmc_traffic.json) records it; bench.py quotes that measurement only while the digest still matches."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".hpp")))
    for f in files + ["../../include/aicam.h"]:
        h.update(f.encode())
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:16]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    bdir = os.path.join(CSRC, "build")
    os.makedirs(bdir, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "aicam.h"))
    cc = hipcc()
    jobs = []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(bdir, src + ".o")
        if force or _stale(obj, [sp] + headers):
            cmd = [cc] + FLAGS + (["-x", "hip"] if src.endswith(".hip") else ["-x", "hip"]) + ["-c", sp, "-o", obj]
            jobs.append((src, cmd))
    def run(job):
        src, cmd = job
        r = subprocess.run(cmd, capture_output=True, text=True)
        return src, r.returncode, r.stdout + r.stderr
    failed = False
    with ThreadPoolExecutor(max_workers=min(6, max(1, len(jobs)))) as ex:
        for src, rc, out in ex.map(run, jobs):
            if verbose and (rc or out.strip()):
                print(f"[{src}] rc={rc}\n{out}", file=sys.stderr)
            failed |= rc != 0
    if failed:
        raise RuntimeError("hipcc failed")
    objs = [os.path.join(bdir, s + ".o") for s in SOURCES]
    if force or jobs or _stale(OUT, objs):
        cmd = [cc, "-shared", "-fPIC", "--offload-arch=gfx950", "-pthread", "-o", OUT] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError("link failed:\n" + r.stdout + r.stderr)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
