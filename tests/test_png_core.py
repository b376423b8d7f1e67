"""csrc/png_core.h, the PNG encoder's code construction and checksum combination, run on the host: tests/png_core_main.cpp is built with
the address and undefined-behaviour sanitizers (a stand-alone program, run directly) and fed the per-block histograms of every case of
tests/png_cases.py, as tests/png_restatement.py states the token pass.  The program adds adversarial and random histograms, checks
limits, Kraft sums, the header read back, block sizes and the CRC-32 / Adler-32 combination, and prints counts that show the limits
were met."""
import os
import re
import struct
import subprocess

from tests import png_cases as K
from tests import png_restatement as R
from tests.test_jpeg_decode_core import _compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tests", "png_core_main.cpp")
MAGIC = 0x31434E50


def _case_file(path):
    records = []
    for case in K.CASES:
        _, stream = K.reference(case)
        for hist, matches, extra in R.block_records(stream, case.w * (1 if case.mode == "gray" else 3) + 1, K.rows_per_block(case)):
            records.append(struct.pack("<288I", *hist, matches, extra))
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC, len(records)) + b"".join(records))
    return len(records)


def test_core_under_the_sanitizers(tmp_path):
    exe, cases = str(tmp_path / "png_core_main"), str(tmp_path / "cases.bin")
    build = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SOURCE, "-o", exe]
    done = subprocess.run(build, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    n = _case_file(cases)
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    print(run.stdout, run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and "runtime error" not in run.stderr
    m = re.fullmatch(r"(\d+) histograms, 0 failed", lines[-2])
    assert m and int(m.group(1)) > n >= len(K.CASES)
    counts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[-1])}
    assert counts["lit_limited"] >= 1 and counts["cl_direct"] >= 1       # both limits were met
    assert counts["fixed"] >= 1 and counts["dynamic"] >= 1 and counts["checksums"] >= 30
    assert counts["max_header_bits"] <= R.HEADER_BITS_MAX
