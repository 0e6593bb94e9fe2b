"""The executable specification of the zone / line counting stage (aic_zones_*): pure Python integers, one stream
per ZonesOracle.  The device is held to it bit for bit (tests/test_gpu_zones.py).

A frame is rows [n, 6] int32 = x1 y1 x2 y2 id cls, what every tracker here delivers.  All geometry runs on DOUBLED integer coordinates
(Python ints: no width), so the anchor needs no rounding:  bottom = (x1 + x2, 2 * y2), centre = (x1 + x2, y1 + y2).

Frame f of a stream (f counts every frame handed in, empty ones too):
  1. the counted rows: rows whose four coordinates are all within +-COORD_MAX, the first of every id in row order.  Rows outside the
     bound are ignored altogether (they do not claim their id); later rows of an id are ignored everywhere.
  2. capacity: slots in use and not expiring now, plus counted rows whose id is in none of them, may not exceed max_tracks.  Otherwise
     the stream STOPS: frame f and every later one deliver nothing (no events, zero occupancy, counters and table as after frame f - 1).
  3. expiry, in slot order: a slot with f - last_seen > forget_after is freed; by zone index a LOST event for every zone it was inside
     (dwell = last_seen + 1 - enter_frame, cls and anchor as last seen) and zone_out += 1.
  4. the counted rows in row order.  First sighting: the lowest free slot, ENTER (value 0) by zone index for the zones it is inside.
     Known id: by zone index EXIT (dwell = f - enter_frame) or ENTER where the inside bit changed, then by line index CROSS (value +-1).
Events are [kind, index, id, cls, frame, value, ax, ay]."""
import numpy as np

ENTER, EXIT, LOST, CROSS = 1, 2, 3, 4
COORD_MAX = 1 << 20
MAX_ZONES = MAX_LINES = MAX_VERTS = 32
MAX_ROWS = MAX_TRACKS = 512
ERR_CAPACITY = -5


def cross(ux, uy, vx, vy):
    return ux * vy - vx * uy


def inside(poly2, px, py):
    """Even-odd rule with half-open edges on doubled coordinates; poly2 = [(x, y), ...] doubled."""
    odd = False
    n = len(poly2)
    for i in range(n):
        (ax, ay), (bx, by) = poly2[i], poly2[(i + 1) % n]
        d = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
        if ((ay > py) != (by > py)) and ((d > 0) == (by > ay)):
            odd = not odd
    return odd


def line_cross(line2, p0, p1):
    """0 = no crossing, +1 / -1 = the side of A->B the track ends on.  line2 = ((ax, ay), (bx, by)) doubled; p0, p1 doubled anchors."""
    (ax, ay), (bx, by) = line2
    s0 = cross(bx - ax, by - ay, p0[0] - ax, p0[1] - ay) >= 0
    s1 = cross(bx - ax, by - ay, p1[0] - ax, p1[1] - ay) >= 0
    ta = cross(p1[0] - p0[0], p1[1] - p0[1], ax - p0[0], ay - p0[1]) >= 0
    tb = cross(p1[0] - p0[0], p1[1] - p0[1], bx - p0[0], by - p0[1]) >= 0
    if s0 != s1 and ta != tb:
        return 1 if s1 else -1
    return 0


class ZonesOracle:
    def __init__(self, zones=(), lines=(), max_tracks=512, forget_after=70, anchor="bottom"):
        assert 1 <= max_tracks <= MAX_TRACKS and forget_after >= 0 and anchor in ("bottom", "centre")
        self.max_tracks, self.forget_after, self.anchor = max_tracks, forget_after, anchor
        self.set(zones, lines)

    def set(self, zones, lines):
        assert len(zones) <= MAX_ZONES and len(lines) <= MAX_LINES
        for z in zones:
            assert 3 <= len(z) <= MAX_VERTS
        self.zones = [[(2 * int(x), 2 * int(y)) for x, y in z] for z in zones]
        self.lines = [((2 * int(a[0]), 2 * int(a[1])), (2 * int(b[0]), 2 * int(b[1]))) for a, b in lines]
        self.reset()

    def reset(self):
        Z, L = len(self.zones), len(self.lines)
        self.frame = 0
        self.status = 0
        self.slots = [None] * self.max_tracks            # dict(id, ax, ay, cls, last, mask, enter[Z])
        self.zone_in, self.zone_out = [0] * Z, [0] * Z
        self.line_pos, self.line_neg = [0] * L, [0] * L

    def counters(self):
        return (np.array(self.zone_in, np.int64), np.array(self.zone_out, np.int64), np.array(self.line_pos, np.int64),
                np.array(self.line_neg, np.int64))

    def _anchor(self, r):
        x1, y1, x2, y2 = (int(v) for v in r[:4])
        return (x1 + x2, 2 * y2 if self.anchor == "bottom" else y1 + y2)

    def step(self, rows):
        """One frame.  Returns (events list of 8-tuples, occupancy list [Z]); ([], zeros) for a stopped stream."""
        Z = len(self.zones)
        if self.status:
            return [], [0] * Z
        f = self.frame
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
        assert len(rows) <= MAX_ROWS
        counted, seen = [], set()
        for r in rows:
            if any(abs(int(v)) > COORD_MAX for v in r[:4]) or int(r[4]) in seen:
                continue
            seen.add(int(r[4]))
            counted.append(r)
        expiring = [s for s, t in enumerate(self.slots) if t is not None and f - t["last"] > self.forget_after]
        kept = {t["id"]: s for s, t in enumerate(self.slots) if t is not None and s not in expiring}
        new = sum(int(r[4]) not in kept for r in counted)
        if len(kept) + new > self.max_tracks:
            self.status = ERR_CAPACITY
            return [], [0] * Z
        ev = []
        for s in expiring:
            t = self.slots[s]
            for z in range(Z):
                if t["mask"] >> z & 1:
                    ev.append((LOST, z, t["id"], t["cls"], f, t["last"] + 1 - t["enter"][z], t["ax"], t["ay"]))
                    self.zone_out[z] += 1
            self.slots[s] = None
        occ = [0] * Z
        for r in counted:
            tid, cls = int(r[4]), int(r[5])
            ax, ay = self._anchor(r)
            mask = 0
            for z, poly in enumerate(self.zones):
                if inside(poly, ax, ay):
                    mask |= 1 << z
                    occ[z] += 1
            if tid in kept:
                t = self.slots[kept[tid]]
                for z in range(Z):
                    was, now = t["mask"] >> z & 1, mask >> z & 1
                    if was and not now:
                        ev.append((EXIT, z, tid, cls, f, f - t["enter"][z], ax, ay))
                        self.zone_out[z] += 1
                    elif now and not was:
                        ev.append((ENTER, z, tid, cls, f, 0, ax, ay))
                        t["enter"][z] = f
                        self.zone_in[z] += 1
                for l, line in enumerate(self.lines):
                    d = line_cross(line, (t["ax"], t["ay"]), (ax, ay))
                    if d:
                        ev.append((CROSS, l, tid, cls, f, d, ax, ay))
                        if d > 0:
                            self.line_pos[l] += 1
                        else:
                            self.line_neg[l] += 1
                t.update(ax=ax, ay=ay, cls=cls, last=f, mask=mask)
            else:
                s = self.slots.index(None)
                t = dict(id=tid, ax=ax, ay=ay, cls=cls, last=f, mask=mask, enter=[0] * Z)
                for z in range(Z):
                    if mask >> z & 1:
                        ev.append((ENTER, z, tid, cls, f, 0, ax, ay))
                        t["enter"][z] = f
                        self.zone_in[z] += 1
                self.slots[s] = t
        self.frame += 1
        return ev, occ


def run_bank(oracles, frames, cap_events):
    """frames[s] = list of rows arrays of stream s.  The flat outputs of aic_zones_update, stream-major:
    (n_events [F], events [F, cap, 8], occupancy [F, 32], status [S])."""
    F = sum(len(fr) for fr in frames)
    n_events = np.zeros(F, np.int32)
    events = np.zeros((F, cap_events, 8), np.int32)
    occupancy = np.zeros((F, MAX_ZONES), np.int32)
    status = np.zeros(len(oracles), np.int32)
    i = 0
    for s, (o, fr) in enumerate(zip(oracles, frames)):
        for rows in fr:
            ev, occ = o.step(rows)
            n_events[i] = len(ev)
            for k, e in enumerate(ev[:cap_events]):
                events[i, k] = e
            occupancy[i, :len(occ)] = occ
            i += 1
        status[s] = o.status
    return n_events, events, occupancy, status
