"""csrc/jpegdec_split_core.h, the parallel entropy decode inside a restart interval, run on the host: tests/jpeg_split_core_main.cpp is
built with the address and undefined-behaviour sanitizers (a stand-alone program, run directly) and fed every case of
tests/jpeg_split_cases.py.  Per case and per segment size of 32, 64, 128 and 1024 bytes the program compares the split decode with
jpegdec_interval on the same bytes: equal coefficients, equal status, intact canaries, silent sanitizers.  The counts it prints show that
the cases did exercise the method."""
import os
import re
import struct
import subprocess

import numpy as np

from tests import jpeg_decode_cases as DK
from tests import jpeg_decode_restatement as D
from tests import jpeg_split_cases as SK
from tests.test_jpeg_decode_core import _compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tests", "jpeg_split_core_main.cpp")
MAGIC = 0x3143534A


def _record(name, hostile, data, desc, intervals):
    iv = np.asarray(intervals, dtype=np.uint32).reshape(-1, 2)
    name = name.encode()
    return b"".join([struct.pack("<I", len(name)), name, struct.pack("<II", hostile, len(data)), data, DK.struct_bytes(desc),
                     struct.pack("<I", len(iv)), iv.tobytes()])


def _case_file(path):
    records = []
    for case in SK.CASES:
        data = SK.make_file(case)
        iv, _ = D.scan_intervals(data, D.read_header(data)["scan_off"])
        records.append(_record(DK.case_id(case), 0, data, DK.descriptor(data), iv))
    records += [_record(h.name, 1, h.data, h.desc, h.intervals) for h in SK.hostile_cases()]
    with open(path, "wb") as f:
        f.write(struct.pack("<III", MAGIC, len(records), DK.C.sizeof(DK.L.JpegFile)) + b"".join(records))
    return len(records)


def test_split_decode_equals_the_interval_path_under_the_sanitizers(tmp_path):
    exe, cases = str(tmp_path / "jpeg_split_core_main"), str(tmp_path / "cases.bin")
    build = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SOURCE, "-o", exe]
    done = subprocess.run(build, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    n = _case_file(cases)
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and "runtime error" not in run.stderr
    assert lines[0] == f"{n} cases, {n * len(SK.SEGMENT_BYTES)} runs, 0 failed"
    counts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[1])}
    assert counts["max_segments"] >= 64                          # an interval of 64 segments or more
    assert counts["wrong"] >= 1 and counts["max_rounds"] >= 2    # a speculative end state was wrong, and an interval took two rounds or more
    assert min(counts[k] for k in ("ok", "truncated", "run", "code")) >= 1   # every way an interval ends, among the hostile expectations
    assert counts["trailing_ignored"] >= 1 and counts["dc_decides"] >= 1
