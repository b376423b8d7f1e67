"""csrc/jpegdec_core.h, the per-interval entropy decode of the JPEG decoder, run on the host: tests/jpeg_decode_core_main.cpp is built
with the address and undefined-behaviour sanitizers (a stand-alone program, run directly) and fed every good case of
tests/jpeg_decode_cases.py and the hostile ones (truncations at every byte of the first interval, seeded single-byte corruptions, crafted
streams).  The sanitizers stay silent, no write leaves the file's coefficient area, and status and coefficients equal what the
restatement decodes from the same bytes: the issue's bar for a hostile case (a nonzero status, or the restatement's coefficients) and
more."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_cases as DK
from tests import jpeg_decode_restatement as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tests", "jpeg_decode_core_main.cpp")
MAGIC = 0x3143444A


def _compiler():
    for c in ("g++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c):
            return c
    pytest.fail("no host C++ compiler")


def _record(name, data, desc, intervals, status, coefs):
    iv = np.asarray(intervals, dtype=np.uint32).reshape(-1, 2)
    flat = DK.flat_coefficients(coefs)
    name = name.encode()
    return b"".join([struct.pack("<I", len(name)), name, struct.pack("<I", len(data)), data, DK.struct_bytes(desc),
                     struct.pack("<I", len(iv)), iv.tobytes(), struct.pack("<i", status), struct.pack("<I", flat.size), flat.tobytes()])


def _case_file(path):
    records = []
    for case in DK.CASES:
        data, ref = DK.make_file(case), DK.reference(case)
        iv, _ = D.scan_intervals(data, ref["header"]["scan_off"])
        records.append(_record(DK.case_id(case), data, DK.descriptor(data), iv, 0, ref["coefs"]))
    kinds = {}
    for i, h in enumerate(DK.hostile_cases()):
        coefs, status = DK.hostile_reference(i)
        kinds[status] = kinds.get(status, 0) + 1
        records.append(_record(h.name, h.data, h.desc, h.intervals, status, coefs))
    with open(path, "wb") as f:
        f.write(struct.pack("<III", MAGIC, len(records), DK.C.sizeof(DK.L.JpegFile)) + b"".join(records))
    return len(records), kinds


def test_core_decode_under_the_sanitizers(tmp_path):
    exe, cases = str(tmp_path / "jpeg_decode_core_main"), str(tmp_path / "cases.bin")
    build = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SOURCE, "-o", exe]
    done = subprocess.run(build, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    n, kinds = _case_file(cases)
    print(f"{n} cases: {len(DK.CASES)} good, hostile by expected status {dict(sorted(kinds.items()))}")
    assert set(kinds) == {D.OK, D.TRUNCATED, D.RUN, D.CODE}          # the hostile set reaches every way an interval ends, and survival
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    assert run.returncode == 0 and run.stdout.strip() == f"{n} cases, 0 failed" and "runtime error" not in run.stderr
