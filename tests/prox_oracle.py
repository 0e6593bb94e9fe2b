"""The executable specification of the proximity stage (aic_prox_*): Python ints and NumPy integer arrays only, one
stream per ProxOracle.  The device is held to it with np.array_equal (tests/test_gpu_prox.py).

A tick of a stream is rows [n, 6] int32 = x1 y1 x2 y2 id cls, what every tracker here delivers.  VALID, FIRST, NONEMPTY, COUNTED, the foot
anchor (fx, fy) in doubled pixels and the whole life cycle of the slot table are tests/heat_oracle.py's, to the letter.  hc = clamp(y2 -
y1, 1, 32767) is the row's height.

Placement.  metric 0 (ground plane; H[9] int32, shift): nx = H0 fx + H1 fy + 2 H2, ny = H3 fx + H4 fy + 2 H5, den = H6 fx + H7 fy + 2 H8;
placed when den > 0 and |gx|, |gy| <= 2^24 for gx = floor((nx << shift) / den), gy alike.  metric 1 (relative to body height): every
counted row is placed with gx = fx, gy = fy.

Near (two placed rows).  metric 0: dgx^2 + dgy^2 <= near^2.  metric 1: 256 max(hc) <= height_ratio_q8 min(hc) and 1 000 000 (dfx^2 + dfy^2)
<= near^2 (hc_i + hc_j)^2.  Reported distance: isqrt(d2), or isqrt(1 000 000 D2) // (hc_i + hc_j).

Readings of this oracle where the rules leave a gap (DESIGN.md section 55 lists them):
  * metric 1's speed divides by the height of the CURRENT row: moved = 1000 isqrt(Dstep^2) // (2 hc).
  * speed = min(moved // dt, 2^22), so that speed << 8 and with it v_q8 and max_v_q8 stay at or below 2^30.
  * a tick without a measurement (a new slot, a row that is not placed, a slot that was not placed when last seen) leaves the slot's gait
    and v_q8 as they are; a new slot starts with gait 0 and v_q8 0.  A slot that is not placed keeps the last placed gx, gy.
  * still wins over running when still_speed == run_speed and v_q8 >> 8 equals both.
  * n_running, n_still count the tick's placed counted rows by their slot's gait behind the speed step.
  * a row tag: gx gy v_q8 gait party party_size n_near flags.  flags = VALID 1 | FIRST 2 | NONEMPTY 4 | PLACED 8 | NEW 16.  v_q8 is -1 while
    the slot's gait is 0.  A row that is not counted: 0 0 -1 0 -1 0 0 flags; counted, not placed: 0 0 v_q8 gait -1 0 0 flags.
  * the record of a tick a stopped stream did not walk is all -1, its n_pair_events 0.
  * export_pairs looks at pairs of LIVE slots (not ENDED ones that wait in pending).
  * `links`, `party_ticks` saturate at 2^30 like every slot counter."""
import numpy as np

LIVE, EXPIRED, FLUSHED = 0, 1, 2
COORD_MAX = 1 << 20
MAX_ROWS = MAX_TRACKS = 512
ERR_CAPACITY = -5
SAT = 1 << 30
G_MAX = 1 << 24
ON_MAX = 32767
SPEED_MAX = 1 << 22
GROUND, BODY = 0, 1
LINK, UNLINK = 1, 2
F_VALID, F_FIRST, F_NONEMPTY, F_PLACED, F_NEW = 1, 2, 4, 8, 16
EVENT_FIELDS = ("reason", "stream", "id", "cls", "first_frame", "last_seen", "sightings", "links", "dist", "max_v_q8", "v_q8", "party_ticks",
                "max_party", "gx", "gy", "gait")
RECORD_FIELDS = ("frame", "n_counted", "n_placed", "n_near_pairs", "largest_near", "n_linked_pairs", "n_parties", "n_singles", "largest_party",
                 "n_units", "n_running", "n_still", "n_link", "n_unlink", "zero0", "zero1")
TAG_FIELDS = ("gx", "gy", "v_q8", "gait", "party", "party_size", "n_near", "flags")
PAIR_EVENT_FIELDS = ("kind", "frame", "id_lo", "id_hi", "duration", "distance", "ticks", "zero")
DEFAULTS = dict(max_tracks=128, forget_after=70, metric=BODY, near=700, height_ratio_q8=384, link_ticks=30, unlink_ticks=60, speed_shift=2,
                still_speed=5, run_speed=70)
IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)


# ---------------------------------------------------------------------------------------------------- arithmetic
def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def valid_row(row):
    return all(abs(int(v)) <= COORD_MAX for v in row[:4]) and int(row[2]) >= int(row[0]) and int(row[3]) >= int(row[1])


def isqrt(v):
    """The largest r with r * r <= v, bit by bit (0 <= v < 2^62), as csrc/prox_math.hpp does it."""
    v = int(v)
    assert 0 <= v < 1 << 62
    r, bit = 0, 1 << 60
    while bit > v:
        bit >>= 2
    while bit:
        if v >= r + bit:
            v -= r + bit
            r = (r >> 1) + bit
        else:
            r >>= 1
        bit >>= 2
    return r


def place(metric, H, shift, fx, fy):
    """(placed, gx, gy); 0, 0 when not placed."""
    if metric == BODY:
        return True, fx, fy
    nx, ny, den = H[0] * fx + H[1] * fy + 2 * H[2], H[3] * fx + H[4] * fy + 2 * H[5], H[6] * fx + H[7] * fy + 2 * H[8]
    assert abs(nx) < 1 << 47 and abs(ny) < 1 << 47 and abs(den) < 1 << 47
    if den <= 0:
        return False, 0, 0
    gx, gy = (nx << shift) // den, (ny << shift) // den                      # Python's // is the floor division
    if abs(gx) > G_MAX or abs(gy) > G_MAX:
        return False, 0, 0
    return True, gx, gy


def near_rule(metric, near, ratio_q8, a, b):
    """a, b = (gx, gy, hc) of two placed rows."""
    d2 = (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
    if metric == GROUND:
        return d2 <= near * near
    lo, hi = min(a[2], b[2]), max(a[2], b[2])
    return 256 * hi <= ratio_q8 * lo and 1000000 * d2 <= near * near * (a[2] + b[2]) ** 2


def distance(metric, a, b):
    d2 = (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
    return isqrt(d2) if metric == GROUND else isqrt(1000000 * d2) // (a[2] + b[2])


def moved(metric, dx, dy, hc):
    s = isqrt(dx * dx + dy * dy)
    return s if metric == GROUND else 1000 * s // (2 * hc)


def gait_of(v_q8, still_speed, run_speed):
    v = v_q8 >> 8
    return 1 if v <= still_speed else 3 if v >= run_speed else 2


class ProxOracle:
    def __init__(self, frame_hw, stream=0, **kw):
        p = dict(DEFAULTS)
        p.update(kw)
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        assert 1 <= self.H <= 16384 and 1 <= self.W <= 16384 and 1 <= p["max_tracks"] <= MAX_TRACKS
        self.max_tracks, self.stream = p["max_tracks"], stream
        self.p = p
        self.check_params()
        self.ground, self.shift = IDENTITY, 0
        # what tests/test_prox_oracle.py counts
        self.log = dict(link_at=0, link_before=0, unlink_at=0, frozen=0, frozen_back=0, reused_with_partner=0, duplicate=0, den_le_0=0, beyond=0,
                        capacity_stop=0, pending_over_cap=0, truncated=0, gait=[0] * 4, dt_gt_1=0, on_saturated=0, expired=0, flushed=0,
                        unplaced_then_placed=0)
        self.reset()

    def check_params(self):
        p = self.p
        assert 0 <= p["forget_after"] <= 1 << 24 and p["metric"] in (GROUND, BODY)
        assert 1 <= p["near"] <= (1 << 24 if p["metric"] == GROUND else 4096) and 256 <= p["height_ratio_q8"] <= 1 << 16
        assert 1 <= p["link_ticks"] <= 32767 and 1 <= p["unlink_ticks"] <= 32767 and 0 <= p["speed_shift"] <= 12
        assert 0 <= p["still_speed"] <= p["run_speed"] <= 1 << 20

    def option(self, key, value):
        self.p[key] = int(value)
        self.check_params()

    def set_ground(self, H, shift):
        H = tuple(int(v) for v in H)
        assert len(H) == 9 and all(abs(v) <= 1 << 30 for v in H) and 0 <= shift <= 14
        self.ground, self.shift = H, int(shift)

    def reset(self):
        self.frame, self.status = 0, 0
        self.slots = [None] * self.max_tracks
        self.pairs = {}                                                      # (slot_lo, slot_hi) -> [linked, on, off, since]
        self.frozen = set()                                                  # (only counted) pairs with one row absent since they were judged

    # ------------------------------------------------------------------------------------------------ rows of one frame
    def measure(self, rows):
        """(flags per row, [(row index, id, cls, fx, fy, hc, placed, gx, gy)] of the counted rows, in row order)."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
        assert len(rows) <= MAX_ROWS
        flags, out, seen = [0] * len(rows), [], set()
        for i, r in enumerate(rows):
            if not valid_row(r):
                continue
            flags[i] |= F_VALID
            if int(r[4]) in seen:
                self.log["duplicate"] += 1
            else:
                flags[i] |= F_FIRST
            seen.add(int(r[4]))
            if r[0] < self.W and r[2] >= 0 and r[1] < self.H and r[3] >= 0:
                flags[i] |= F_NONEMPTY
            if flags[i] != F_VALID | F_FIRST | F_NONEMPTY:
                continue
            x1, y1, x2, y2 = (int(v) for v in r[:4])
            fx, fy, hc = clamp(x1 + x2, 0, 2 * self.W - 1), clamp(2 * y2, 0, 2 * self.H - 1), clamp(y2 - y1, 1, 32767)
            ok, gx, gy = place(self.p["metric"], self.ground, self.shift, fx, fy)
            if not ok:
                H = self.ground
                self.log["den_le_0" if H[6] * fx + H[7] * fy + 2 * H[8] <= 0 else "beyond"] += 1
            else:
                flags[i] |= F_PLACED
            out.append((i, int(r[4]), int(r[5]), fx, fy, hc, ok, gx, gy))
        return flags, out

    # ------------------------------------------------------------------------------------------------ events
    def _event(self, s, reason):
        t = self.slots[s]
        return np.array([reason, self.stream, t["id"], t["cls"], t["first"], t["last"], t["sightings"], t["links"], t["dist"], t["max_v"], t["v"],
                         t["party_ticks"], t["max_party"], t["gx"], t["gy"], t["gait"]], np.int32)

    def _emit(self, out, cap):
        for s, t in enumerate(self.slots):
            if t is not None and t["ended"] and len(out) < cap:
                out.append(self._event(s, t["ended"]))
                self.slots[s] = None
        self.log["pending_over_cap"] += self.pending() > 0

    def pending(self):
        return sum(t is not None and t["ended"] != 0 for t in self.slots)

    # ------------------------------------------------------------------------------------------------ one tick
    def step(self, rows, out, cap):
        """One tick -> (row tags [n, 8], record [16], [pair event [8]] -- all of them, untruncated)."""
        n = len(rows)
        tags, rec = np.full((n, 8), -1, np.int32), np.full(16, -1, np.int32)
        if self.status:
            return tags, rec, []
        p, f = self.p, self.frame
        flags, counted = self.measure(rows)
        live = {t["id"]: s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] <= p["forget_after"]}
        expiring = [s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] > p["forget_after"]]
        ended = [s for s, t in enumerate(self.slots) if t is not None and (t["ended"] or s in expiring)]          # slot order
        kept = ended[max(0, cap - len(out)):]                                # no room in the output list: they keep their slots
        occupied = len(live) + sum(self.slots[s]["ended"] != 0 for s in ended) + sum(s in expiring for s in kept)
        if occupied + sum(c[1] not in live for c in counted) > self.max_tracks:
            self.status = ERR_CAPACITY
            self.log["capacity_stop"] += 1
            return tags, rec, []
        for s in expiring:
            self.slots[s]["ended"] = EXPIRED
            self.log["expired"] += 1
        self._emit(out, cap)
        for i in range(n):
            tags[i] = [0, 0, -1, 0, -1, 0, 0, flags[i]]
        # ---- 1. slots and speed
        placed = []                                                          # (row, slot, id, gx, gy, hc) in row order
        for i, tid, cls, fx, fy, hc, ok, gx, gy in counted:
            if tid in live:
                s = live[tid]
                t = self.slots[s]
                if ok and t["placed"]:
                    dt = f - t["last"]
                    assert dt >= 1
                    self.log["dt_gt_1"] += dt > 1
                    mv = moved(p["metric"], gx - t["gx"], gy - t["gy"], hc)
                    speed = min(mv // dt, SPEED_MAX)
                    t["v"] = speed << 8 if t["gait"] == 0 else t["v"] + (((speed << 8) - t["v"]) >> p["speed_shift"])
                    t["dist"], t["max_v"] = min(t["dist"] + mv, SAT), max(t["max_v"], t["v"])
                    t["gait"] = gait_of(t["v"], p["still_speed"], p["run_speed"])
                elif ok:
                    self.log["unplaced_then_placed"] += 1
            else:
                s = self.slots.index(None)
                partners = [k for k in self.pairs if s in k]
                for k in partners:
                    other = k[0] if k[1] == s else k[1]
                    self.log["reused_with_partner"] += self.slots[other] is not None and not self.slots[other]["ended"]
                    del self.pairs[k]                                        # no state is inherited
                    self.frozen.discard(k)
                t = self.slots[s] = dict(id=tid, first=f, sightings=0, ended=0, gx=0, gy=0, v=0, gait=0, dist=0, max_v=0, party_ticks=0, max_party=0,
                                         links=0)
                flags[i] |= F_NEW
            t.update(last=f, cls=cls, sightings=t["sightings"] + 1, placed=ok)
            if ok:
                t["gx"], t["gy"] = gx, gy
                placed.append((i, s, tid, gx, gy, hc))
            self.log["gait"][t["gait"]] += 1
            tags[i] = [gx, gy, t["v"] if t["gait"] else -1, t["gait"], -1, 0, 0, flags[i]]
        # ---- 2. the near graph
        P = len(placed)
        geo = [(q[3], q[4], q[5]) for q in placed]
        near = [[a != b and near_rule(p["metric"], p["near"], p["height_ratio_q8"], geo[a], geo[b]) for b in range(P)] for a in range(P)]
        n_near_pairs = sum(near[a][b] for a in range(P) for b in range(a + 1, P))
        near_comp = components(P, [(a, b) for a in range(P) for b in range(a + 1, P) if near[a][b]])
        # ---- 3. pair state
        events, edges, n_link, n_unlink, n_linked = [], [], 0, 0, 0
        present = {q[1] for q in placed}
        for k, e in self.pairs.items():                                      # (only counted) a pair with one row absent is frozen
            if (k[0] in present) != (k[1] in present) and any(e[:3]) and k not in self.frozen:
                self.frozen.add(k)
                self.log["frozen"] += 1
        for a in range(P):
            for b in range(a + 1, P):
                sa, sb = placed[a][1], placed[b][1]
                key = (min(sa, sb), max(sa, sb))
                e = self.pairs.setdefault(key, [0, 0, 0, 0])
                if key in self.frozen:
                    self.frozen.discard(key)
                    self.log["frozen_back"] += 1
                ids = (min(placed[a][2], placed[b][2]), max(placed[a][2], placed[b][2]))
                if near[a][b]:
                    self.log["on_saturated"] += e[1] == ON_MAX
                    e[1], e[2] = min(e[1] + 1, ON_MAX), 0
                    if not e[0]:
                        if e[1] >= p["link_ticks"]:
                            self.log["link_at"] += e[1] == p["link_ticks"]
                            e[0], e[3] = 1, f
                            n_link += 1
                            events.append(np.array([LINK, f, ids[0], ids[1], 0, distance(p["metric"], geo[a], geo[b]), e[1], 0], np.int32))
                            for s in (sa, sb):
                                self.slots[s]["links"] = min(self.slots[s]["links"] + 1, SAT)
                        else:
                            self.log["link_before"] += e[1] == p["link_ticks"] - 1
                else:
                    e[2], e[1] = min(e[2] + 1, ON_MAX), 0
                    if e[0] and e[2] >= p["unlink_ticks"]:
                        self.log["unlink_at"] += e[2] == p["unlink_ticks"]
                        e[0] = 0
                        n_unlink += 1
                        events.append(np.array([UNLINK, f, ids[0], ids[1], f - e[3], distance(p["metric"], geo[a], geo[b]), e[2], 0], np.int32))
                if e[0]:
                    n_linked += 1
                    edges.append((a, b))
        # ---- 4. parties
        comp = components(P, edges)
        n_parties = n_singles = largest = n_running = n_still = 0
        for members in comp:
            size, party = len(members), min(placed[a][2] for a in members)
            n_parties += size >= 2
            n_singles += size == 1
            largest = max(largest, size)
            for a in members:
                i, s = placed[a][0], placed[a][1]
                t = self.slots[s]
                if size >= 2:
                    t["party_ticks"] = min(t["party_ticks"] + 1, SAT)
                t["max_party"] = max(t["max_party"], size)
                tags[i, 4:7] = party, size, sum(near[a])
        for q in placed:
            g = self.slots[q[1]]["gait"]
            n_running += g == 3
            n_still += g == 1
        # ---- 5. the record
        rec[:] = [f, len(counted), P, n_near_pairs, max((len(c) for c in near_comp), default=0), n_linked, n_parties, n_singles, largest,
                  n_parties + n_singles, n_running, n_still, n_link, n_unlink, 0, 0]
        self.frame += 1
        return tags, rec, events

    # ------------------------------------------------------------------------------------------------ calls
    def update(self, rows, cap):
        """rows[t] for the ticks of one call -> ([event], pending, status, [tags per tick], [record per tick], [[pair event] per tick]);
        no ticks: a drain."""
        out = []
        if len(rows) == 0:
            self._emit(out, cap)
        steps = [self.step(r, out, cap) for r in rows]
        return out, self.pending(), self.status, [s[0] for s in steps], [s[1] for s in steps], [s[2] for s in steps]

    def flush(self, cap):
        out = []
        for t in self.slots:
            if t is not None and not t["ended"]:
                t["ended"] = FLUSHED
                self.log["flushed"] += 1
        self._emit(out, cap)
        return out, self.pending(), self.status, [], [], []

    def export(self):
        return [self._event(s, t["ended"]) for s, t in enumerate(self.slots) if t is not None]

    def export_pairs(self):
        """[n, 6] id_a id_b linked on off since: the nonzero entries among live slots, in (slot_lo, slot_hi) order; id_a is slot_lo's."""
        live = lambda s: self.slots[s] is not None and not self.slots[s]["ended"]          # noqa: E731
        out = [[self.slots[a]["id"], self.slots[b]["id"]] + e for (a, b), e in sorted(self.pairs.items()) if any(e) and live(a) and live(b)]
        return np.array(out, np.int32).reshape(-1, 6)


def components(n, edges):
    """The connected components of an undirected graph on 0..n-1 as lists of members, ordered by their smallest member."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for a in range(n):
        groups.setdefault(find(a), []).append(a)
    return [groups[r] for r in sorted(groups)]


def pack(results, cap, cap_pairs, ticks=0):
    """Per-stream results -> the flat outputs of aic_prox_update / _flush: n_final [S], events [S, cap, 16], pending [S], status [S], records
    [F, 16], row_tags [rows, 8], n_pair_events [F], pair_events [F, cap_pairs, 8] (F = ticks * S, tick-major)."""
    S = len(results)
    n_final, pending, status = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    events = np.zeros((S, cap, 16), np.int32)
    for s, (out, pend, st, *_) in enumerate(results):
        n_final[s], pending[s], status[s] = len(out), pend, st
        for k, ev in enumerate(out):
            events[s, k] = ev
    F = ticks * S
    records, n_pe, pe = np.zeros((F, 16), np.int32), np.zeros(F, np.int32), np.zeros((F, cap_pairs, 8), np.int32)
    tags = []
    for t in range(ticks):
        for s in range(S):
            tags.append(results[s][3][t])
            records[t * S + s] = results[s][4][t]
            evs = results[s][5][t]
            n_pe[t * S + s] = len(evs)
            for k, ev in enumerate(evs[:cap_pairs]):
                pe[t * S + s, k] = ev
    row_tags = np.concatenate(tags).reshape(-1, 8).astype(np.int32) if tags else np.zeros((0, 8), np.int32)
    return n_final, events, pending, status, records, row_tags, n_pe, pe


def run_bank(oracles, rows, cap, cap_pairs):
    """rows[t][s] = rows array.  One call of a bank, packed."""
    T = len(rows)
    res = [o.update([rows[t][s] for t in range(T)], cap) for s, o in enumerate(oracles)]
    for o, r in zip(oracles, res):
        o.log["truncated"] += any(len(e) > cap_pairs for e in r[5])
    return pack(res, cap, cap_pairs, T)


def flush_bank(oracles, cap, stream=None):
    res = [o.flush(cap) if stream is None or stream == s else ([], o.pending(), o.status, [], [], []) for s, o in enumerate(oracles)]
    return pack(res, cap, 0)
