"""The identity archive's arithmetic and bookkeeping in NumPy: what csrc/kernels_archive.hip and csrc/archive.cpp
must equal bit for bit.  Shared by tests/test_archive_host.py and tests/test_gpu_archive.py."""
import numpy as np

K_INFTY = np.float32(1e5)
F127 = np.float32(127)
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def pitch_of(dim):
    return (dim + 63) // 64 * 64


def quantise(v):
    """fp32 [dim] -> (int8 [dim], fp32 scale), or None for a row that has no code: all zero, a non-finite element, no finite 127 / m."""
    v = np.asarray(v, np.float32)
    if not np.isfinite(v).all():
        return None
    m = np.abs(v).max()
    if not m > 0:
        return None
    with np.errstate(over="ignore"):
        inv = F127 / m                                   # one correctly rounded fp32 division
    if not np.isfinite(inv):
        return None
    q = np.rint((v * inv).astype(np.float32)).astype(np.int8)   # half to even
    return q, np.float32(m / F127)


def distance(qa, sa, qb, sb):
    """Rows qa [N, dim] int8 with scales sa [N] against ONE query (qb [dim], sb): fp32 [N]."""
    dot = qa.astype(np.int32) @ qb.astype(np.int32)      # exact: |dot| <= 1024 * 127^2 < 2^24
    sim = ((dot.astype(np.float32) * np.asarray(sa, np.float32)).astype(np.float32) * np.float32(sb)).astype(np.float32)
    d = (np.float32(1) - sim).astype(np.float32)
    return np.where(d > 0, d, np.float32(0)).astype(np.float32)


class IndexRef:
    """A row is known by an int64 key >= 0.  Put is an upsert: a known key keeps its slot and t_first; a new key takes the lowest free
    slot; a full archive evicts the occupied slot with the smallest (t_last, slot).  Where one call names a slot twice the last row
    keeps it and the earlier rows get slot -1."""

    def __init__(self, capacity):
        self.cap, self.hw = capacity, 0
        self.key, self.cam, self.t_first, self.t_last = [], [], [], []

    def find(self, key):
        return self.key.index(key) if key >= 0 and key in self.key else -1

    def assign(self, keys, cameras, tick):
        slots, evicted, last = [], [], {}
        for i, (k, c) in enumerate(zip(keys, cameras)):
            k, ev = int(k), -1
            s = self.find(k)
            if s < 0:
                free = [x for x in range(self.hw) if self.key[x] < 0]
                if free:
                    s = free[0]
                elif self.hw < self.cap:
                    s = self.hw
                    self.hw += 1
                    self.key.append(-1), self.cam.append(0), self.t_first.append(0), self.t_last.append(0)
                else:
                    s = min(range(self.hw), key=lambda x: (self.t_last[x], x))
                    ev = self.key[s]
                self.key[s], self.t_first[s] = k, tick
            self.t_last[s], self.cam[s] = tick, int(c)
            if s in last:
                slots[last[s]] = -1
            last[s] = i
            slots.append(s), evicted.append(ev)
        return slots, evicted

    def remove(self, key):
        s = self.find(key)
        if s >= 0:
            self.key[s] = -1
        return s

    def size(self):
        return sum(k >= 0 for k in self.key)


class ArchiveRef(IndexRef):
    """The index plus the stored codes.  put() raises ValueError, storing nothing, when a row has no code."""

    def __init__(self, capacity, dim):
        super().__init__(capacity)
        self.dim = dim
        self.q = np.zeros((0, dim), np.int8)
        self.scale = np.zeros(0, np.float32)

    def put(self, keys, cameras, tick, rows):
        codes = [quantise(r) for r in np.asarray(rows, np.float32).reshape(len(keys), self.dim)]
        if any(c is None for c in codes):
            raise ValueError("a row has no code")
        slots, _ = self.assign(keys, cameras, tick)
        if self.hw > len(self.q):
            self.q = np.concatenate([self.q, np.zeros((self.hw - len(self.q), self.dim), np.int8)])
            self.scale = np.concatenate([self.scale, np.zeros(self.hw - len(self.scale), np.float32)])
        for s, (q, sc) in zip(slots, codes):
            if s >= 0:
                self.q[s], self.scale[s] = q, sc
        return slots

    def search(self, queries, k=1, exclude_camera=-1, t_lo=I64_MIN, t_hi=I64_MAX, exclude_key=-1, max_distance=np.inf):
        """-> (keys, slots, dist) [n, k]; every filter may be a scalar or one value per query."""
        queries = np.asarray(queries, np.float32).reshape(-1, self.dim)
        n = len(queries)
        per = lambda x: np.broadcast_to(np.asarray(x), (n,))      # noqa: E731
        exclude_camera, t_lo, t_hi, exclude_key = per(exclude_camera), per(t_lo), per(t_hi), per(exclude_key)
        max_distance = per(np.asarray(max_distance, np.float32))
        out_k, out_s, out_d = np.full((n, k), -1, np.int64), np.full((n, k), -1, np.int32), np.full((n, k), K_INFTY, np.float32)
        key, cam, tl = np.asarray(self.key, np.int64), np.asarray(self.cam, np.int64), np.asarray(self.t_last, np.int64)
        for i in range(n):
            qq, qs = quantise(queries[i])
            if self.hw == 0:
                continue
            d = distance(self.q[:self.hw], self.scale[:self.hw], qq, qs)
            ok = (key >= 0) & (tl >= t_lo[i]) & (tl <= t_hi[i]) & (d <= max_distance[i])
            if exclude_camera[i] >= 0:
                ok &= cam != exclude_camera[i]
            if exclude_key[i] >= 0:
                ok &= key != exclude_key[i]
            rank = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(self.hw, dtype=np.uint64)
            best = np.sort(rank[ok])[:k]
            s = (best & np.uint64(0xffffffff)).astype(np.int32)
            out_s[i, :len(s)], out_d[i, :len(s)], out_k[i, :len(s)] = s, d[s], key[s]
        return out_k, out_s, out_d
