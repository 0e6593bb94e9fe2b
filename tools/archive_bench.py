#!/usr/bin/env python3
"""Kernel time of an identity-archive search against its bandwidth floor and against what a user would write
today: torch fp16 matmul + topk on the device.

    python tools/archive_bench.py [--rows 65536,1048576] [--queries 1,16,64,256] [--dim 512] [--k 8]

The archive holds `rows` sightings of rows / 8 identities (unit rows, cosine about 0.8 between two sightings of one identity); a query is
one more sighting of a random identity.  Both searches run in this process, alternating, 2 warm-up and 7 timed passes each: the archive's
time is the library's HIP-event bracket around the query prologue, the search and the merge; torch's is a torch.cuda.Event bracket around
matmul + topk.  Floor: rows * (pitch + 64) bytes (row, scale and metadata) per sweep of 64 queries at 6.29 TB/s, the copy rate measured
on this device.  recall@k of both against a float64 search of the unquantised rows is reported, not gated.
One JSON line per shape."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12
CHUNK = 65536


def pkg(name):
    return importlib.import_module("ai-camera_amd." + name)


def sightings(torch, chunk, per, dim, seed, pick=None):
    """fp32 [n * per, dim] on the device: `per` sightings of the identities of chunk `chunk` (8192 identities; pick = some of them).  An
    identity's centre is the same whatever `seed` (the sighting noise) is."""
    g = torch.Generator(device="cuda")
    g.manual_seed(7 + chunk)
    c = torch.randn(CHUNK // 8, dim, generator=g, device="cuda")
    c = c / c.norm(dim=1, keepdim=True)
    if pick is not None:
        c = c[pick]
    g.manual_seed((seed << 32) + chunk)
    v = c[:, None, :] + 0.5 * torch.randn(len(c), per, dim, generator=g, device="cuda") / dim ** 0.5
    return (v / v.norm(dim=2, keepdim=True)).reshape(len(c) * per, dim)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", default="65536,1048576")
    p.add_argument("--queries", default="1,16,64,256")
    p.add_argument("--dim", type=int, default=512)
    p.add_argument("--k", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--steps", type=int, default=7)
    args = p.parse_args()
    import numpy as np
    import torch                                                            # before libaicam.so: one HIP runtime in the process
    L = pkg("_lib")
    dim, k = args.dim, args.k
    pitch = (dim + 63) // 64 * 64
    stat = lambda t: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)))   # noqa: E731
    for N in (int(x) for x in args.rows.split(",")):
        assert N % CHUNK == 0, "rows must be a multiple of 65536"
        arc = pkg("archive").IdentityArchive(N, dim)
        half = torch.empty(N, dim, dtype=torch.float16, device="cuda")
        for c0 in range(0, N, CHUNK):
            rows = sightings(torch, c0 // CHUNK, 8, dim, seed=1)
            arc.put(np.arange(c0, c0 + CHUNK, dtype=np.int64), (np.arange(CHUNK) % 256).astype(np.int32), c0 // CHUNK, rows)
            half[c0:c0 + CHUNK] = rows.half()
        for Q in (int(x) for x in args.queries.split(",")):
            ident = torch.randint(0, N // 8, (Q,), generator=torch.Generator().manual_seed(Q)).tolist()
            q = torch.cat([sightings(torch, i // (CHUNK // 8), 1, dim, seed=2 + n, pick=[i % (CHUNK // 8)]) for n, i in enumerate(ident)])
            qh = q.half()
            # the float64 answer on the unquantised rows, chunk by chunk
            best_v = torch.full((Q, 0), 0.0, dtype=torch.float64, device="cuda")
            best_i = torch.zeros((Q, 0), dtype=torch.int64, device="cuda")
            for c0 in range(0, N, CHUNK):
                rows = sightings(torch, c0 // CHUNK, 8, dim, seed=1).double()
                v, i = (q.double() @ rows.T).topk(k, dim=1)
                best_v, best_i = torch.cat([best_v, v], 1), torch.cat([best_i, i + c0], 1)
                v, j = best_v.topk(k, dim=1)
                best_v, best_i = v, best_i.gather(1, j)
            truth = best_i.cpu().numpy()

            def run_archive():
                L.call("aic_prof_reset", 0)
                out = arc.search(q, k=k)
                return L.prof_read(0)["tracker"]["ms"], out[1]

            def run_torch():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                idx = (qh @ half.T).topk(k, dim=1).indices
                b.record()
                b.synchronize()
                return a.elapsed_time(b), idx.cpu().numpy()

            L.call("aic_prof_enable", 0, 1 << 6)
            for _ in range(args.warmup):
                run_archive(), run_torch()
            ta, tt = [], []
            for s in range(args.steps):                                     # alternating order
                for which in ((0, 1) if s % 2 == 0 else (1, 0)):
                    if which == 0:
                        ms, slots = run_archive()
                        ta.append(ms)
                    else:
                        ms, idx = run_torch()
                        tt.append(ms)
            L.call("aic_prof_enable", 0, 0)
            recall = lambda got: float(np.mean([len(set(g.tolist()) & set(t.tolist())) / k for g, t in zip(got, truth)]))   # noqa: E731
            sweeps = (Q + 63) // 64
            floor_ms = 1e3 * N * (pitch + 64) * sweeps / COPY_RATE
            print(json.dumps(dict(rows=N, queries=Q, dim=dim, k=k, block_rows=arc.block_rows(Q), archive_ms=stat(ta), torch_fp16_ms=stat(tt),
                                  floor_ms=floor_ms, archive_over_floor=float(np.median(ta)) / floor_ms,
                                  torch_over_archive=float(np.median(tt)) / float(np.median(ta)),
                                  recall_archive=recall(slots), recall_torch_fp16=recall(idx))), flush=True)
        arc.close()
        del half
    return 0


if __name__ == "__main__":
    sys.exit(main())
