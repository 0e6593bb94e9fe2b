"""What AICAM_POISON_ALLOC fills a fresh allocation with (ai-camera_amd/csrc/poison_pattern.hpp) on the CPU.

tests/poison_pattern_probe.cpp is built with the system g++ under the address and undefined-behaviour sanitizers and run as a child
process; it is never loaded into Python.  The table it prints is compared with the table the design states, restated here."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# type -> (size, class): "float", "int" (integer of 4 or 8 bytes) or "other"
TYPES = {"float": (4, "float"), "double": (8, "float"), "int": (4, "int"), "long long": (8, "int"), "unsigned long long": (8, "int"),
         "uint8_t": (1, "other"), "int16_t": (2, "other"), "char": (1, "other"), "struct": (12, "other")}


def expected(size, cls, mode):
    """-> (width, value, the bytes of one element)"""
    if mode == "zero":
        return 1, 0, bytes(size)
    if mode == "nan":
        return 1, 0xFF, b"\xff" * size
    if cls == "int":
        return size, 0x7B7B, (0x7B7B).to_bytes(size, "little")
    return 1, 0x7B, b"\x7b" * size


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the poison pattern test builds tests/poison_pattern_probe.cpp with the system compiler")
    exe = str(tmp_path_factory.mktemp("poison_pattern") / "poison_pattern_probe")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "poison_pattern_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_width_value_and_bytes_per_type_and_mode(printed):
    seen = set()
    for line in printed:
        if not line.startswith("type="):
            continue
        head, fill, body, first = line.split(" | ")
        name = head[len("type="):head.index(" size=")]
        size, mode = int(head.split(" size=")[1].split()[0]), head.split(" mode=")[1]
        assert size == TYPES[name][0], line
        width, value, elem = expected(size, TYPES[name][1], mode)
        assert fill == f"width={width} value=0x{value:x}", line
        assert bytes.fromhex(body[len("bytes="):]) == elem * 5, line            # every element, to the buffer's last byte
        seen.add((name, mode))
        first = first[len("first="):]
        # the element as its type reads it: what the table in the design promises a kernel sees
        if name == "float":
            want = struct.unpack("<f", elem)[0]
            assert (np.isnan(float(first)) and np.isnan(want)) or np.float32(float(first)) == np.float32(want), line
            assert mode != "big" or 1.2e36 < float(first) < 1.4e36, line
        elif name == "double":
            want = struct.unpack("<d", elem)[0]
            assert (np.isnan(float(first)) and np.isnan(want)) or float(first) == want, line
            assert mode != "big" or (np.isfinite(float(first)) and float(first) > 1e30), line
        elif name in ("int", "long long"):
            assert int(first) == {"zero": 0, "big": 31611, "nan": -1}[mode], line
        elif name == "unsigned long long":
            assert int(first) == {"zero": 0, "big": 31611, "nan": 2 ** 64 - 1}[mode], line
        elif name == "uint8_t":
            assert int(first) == {"zero": 0, "big": 123, "nan": 255}[mode], line
        elif name == "char":
            assert int(first) & 0xFF == {"zero": 0, "big": 123, "nan": 255}[mode], line
        elif name == "int16_t":
            assert int(first) == {"zero": 0, "big": 0x7B7B, "nan": -1}[mode], line
            h = np.frombuffer(elem, np.float16)[0]                               # a 16-bit buffer is fp16 as often as int16
            assert {"zero": h == 0, "big": h == 61280, "nan": np.isnan(h)}[mode], line
        else:
            a, b, c = first.split("/")
            assert int(c) == {"zero": 0, "big": 123, "nan": 255}[mode], line
            assert int(b) == {"zero": 0, "big": 0x7B7B7B7B, "nan": -1}[mode], line   # an int inside a struct is bytes, not the value 31611
    assert seen == {(t, m) for t in TYPES for m in ("zero", "big", "nan")}


def test_only_the_three_mode_names_are_accepted(printed):
    got = {}
    for line in printed:
        if line.startswith("parse "):
            head, tail = line[len("parse value="):].split(" | mode=")
            got[head] = int(tail)
    assert got == {"(unset)": 0, "zero": 1, "big": 2, "nan": 3, "(empty)": -1, "1": -1, "NaN": -1, "zero ": -1}
