"""The arithmetic of a frame-bank call (ai-camera_amd/csrc/bank_call.hpp) on the CPU.

tests/bank_call_probe.cpp is built with the system g++ under the address and undefined-behaviour sanitizers and run as a child process;
it is never loaded into Python.  Every line it prints is compared with the four call sites' formulas AS THEY WERE before they shared a
header -- restated here, one function per site -- and with the launch loop every stage spelled out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the call sites as they were: ints of the staging buffer, and of the slot stages' output buffer
def bestshot_was(S, F, total, cap, host):
    o_mode, o_off = S, 2 * S
    o_rows = o_off + F + 1
    o_ev = (3 * S + 3) // 4 * 4
    return dict(o_mode=o_mode, o_off=o_off, o_rows=o_rows, n_ints=o_rows + (total * 6 if host else 0), staged=host,
                o_pending=S, o_status=2 * S, o_events=o_ev, out_ints=o_ev + S * cap * 16)


def colours_was(S, F, total, cap, host):
    o_mode, o_off = S, 2 * S
    o_rows = o_off + F + 1
    o_ev = (3 * S + 3) // 4 * 4
    return dict(o_mode=o_mode, o_off=o_off, o_rows=o_rows, n_ints=o_rows + (total * 6 if host else 0), staged=host,
                o_pending=S, o_status=2 * S, o_events=o_ev, out_ints=o_ev + S * cap * 48)


def scene_was(S, F, total, cap, host):
    o_off = S
    o_rows = o_off + F + 1
    return dict(o_mode=0, o_off=o_off, o_rows=o_rows, n_ints=o_rows + (total * 6 if host else 0), staged=host)


def left_was(S, F, total, cap, host):
    o_off = S
    o_rows = o_off + F + 1
    return dict(o_mode=0, o_off=o_off, o_rows=o_rows, n_ints=o_rows + (total * 6 if host else 0), staged=host)


WAS = {"bestshot": bestshot_was, "colours": colours_was, "scene": scene_was, "left": left_was}
EVENT_INTS = {"bestshot": 16, "colours": 48}


# ---- the launch loop as every stage had it; stage_bytes(lo, hi1) = the stage's own term for ticks [lo, hi1)
def launches_were(ticks, ticks_per_launch, budget, host_frames, tick_bytes, stage_bytes):
    out, lo = [], 0
    while lo < ticks:
        hi = lo + 1                                                          # one tick at the least
        while (hi < ticks and (ticks_per_launch == 0 or hi - lo < ticks_per_launch) and stage_bytes(lo, hi + 1) <= budget
               and (not host_frames or (hi + 1 - lo) * tick_bytes <= budget)):
            hi += 1
        out.append((lo, hi))
        lo = hi
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the bank call test builds tests/bank_call_probe.cpp with the system compiler")
    exe = str(tmp_path_factory.mktemp("bank_call") / "bank_call_probe")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "bank_call_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def fields(text, conv=int):
    return {k: conv(v) for k, v in (t.split("=") for t in text.split())}


def test_every_offset_is_where_the_call_sites_had_it(printed):
    seen = set()
    for line in printed:
        if not line.startswith("layout "):
            continue
        head, tail = line[len("layout "):].split(" | ")
        p = fields(head, str)
        site = p.pop("site")
        p = {k: int(v) for k, v in p.items()}
        got = fields(tail)
        assert got == {k: int(v) for k, v in WAS[site](**p).items()}, line
        S, F, total, cap, host = p["S"], p["F"], p["total"], p["cap"], p["host"]
        # the blocks in the order they lie, none over another: reset | (mode) | frame_off | rows
        blocks = [(0, S)] + ([(got["o_mode"], S)] if site in EVENT_INTS else []) + [(got["o_off"], F + 1), (got["o_rows"], total * 6 if host else 0)]
        at = 0
        for start, size in blocks:
            assert start == at, line
            at += size
        assert at == got["n_ints"], line
        if site in EVENT_INTS:                                               # n_final | pending | status | (16-byte aligned) events
            assert (0, got["o_pending"], got["o_status"]) == (0, S, 2 * S) and got["o_events"] >= 3 * S, line
            assert got["o_events"] * 4 % 16 == 0 and got["o_events"] - 3 * S < 4, line
            assert got["out_ints"] == got["o_events"] + S * cap * EVENT_INTS[site], line
        seen.add((site, S, F, total, cap, host))
    assert len(seen) == 4 * 4 * 5 * 4 * 3 * 2                                # sites x S x F x rows x cap x host / device rows


def tick_rows(k, ticks):
    return 40 if k == ticks // 2 else 3


def test_the_planner_cuts_a_call_where_the_launch_loops_did(printed):
    seen = 0
    for line in printed:
        if not line.startswith("plan "):
            continue
        head, _, tail = line[len("plan "):].partition(" |")
        p = fields(head)
        ticks, prefix = p["ticks"], p["prefix"]
        got = [tuple(int(x) for x in t.split(":")) for t in tail.split()]
        if prefix:                                                           # colours and best shots: rows of [lo, hi) x bytes a row
            off = [0]
            for k in range(ticks):
                off.append(off[-1] + tick_rows(k, ticks))
            stage_bytes = lambda lo, hi: (off[hi] - off[lo]) * 128
            unit = 3 * 128
        else:                                                                # scene and left: ticks x what a tick of cells takes
            stage_bytes = lambda lo, hi: (hi - lo) * 1000
            unit = 1000
        assert p["frame"] in (0, unit) and p["budget"] in (unit, unit - 1, unit * 5 // 2, 1 << 40), line
        assert got == launches_were(ticks, p["tpl"], p["budget"], p["frame"] != 0, unit, stage_bytes), line
        # the launches tile [0, ticks): no gap, none empty, one tick at the least
        assert [lo for lo, _ in got] == [0] * bool(ticks) + [hi for _, hi in got][:-1] and all(hi > lo for lo, hi in got), line
        assert (got[-1][1] if got else 0) == ticks, line
        if p["tpl"]:
            assert all(hi - lo <= p["tpl"] for lo, hi in got), line
        if p["budget"] < unit:                                               # below one tick: a launch still takes one
            assert got == [(k, k + 1) for k in range(ticks)], line
        seen += 1
    assert seen == 5 * 4 * 2 * 4 * 2                                         # ticks x ticks_per_launch x cost x budget x host / device frames


def test_fill_writes_prefix_sums_and_only_staged_rows(printed):
    counts = [2, 0, 3, 1, 0, 4]
    rows = [1000 + i for i in range(60)]
    seen = 0
    for line in printed:
        if not line.startswith("fill mode="):
            continue
        head, body, tail = line[len("fill "):].split(" | ")
        p = fields(head)
        h = [int(x) for x in body.split()]
        S, F = 2, 6
        o_off = (2 if p["mode"] else 1) * S
        c = counts if p["counts"] else [0] * F
        want = [-7] * o_off + [sum(c[:i]) for i in range(F + 1)]            # the blocks in front are the caller's: untouched
        staged = p["host"] and p["counts"]
        want += rows if staged else []
        assert h == want and len(h) == p["n_ints"], line
        assert tail == f"rows_of_1_3={sum(c[2:6])} d_rows={'staged' if p['host'] else 'caller'}", line
        seen += 1
    assert seen == 8
    (z,) = [line for line in printed if line.startswith("fill zones ")]
    h = [int(x) for x in z.split(" | ")[1].split()]
    assert h == [-7] * 6 + [sum(counts[:i]) for i in range(7)] + [-7] * 6 + rows
