"""csrc/pngdec_core.h, the serial parts of the PNG decoder, run on the host: tests/png_decode_core_main.cpp is built with the address and
undefined-behaviour sanitizers (a stand-alone program, run directly) and fed every good case of tests/png_decode_cases.py and every
hostile one (crafted streams, truncations at every byte, seeded corruptions).  The sanitizers stay silent, no write leaves the file's
areas, and status, rows finished and pixels in the three layouts equal what tests/png_decode_restatement.py makes of the same bytes:
the bar for a corrupted file (a non-zero status, or Pillow's pixels; tests/test_png_decode_host.py holds the restatement to it) and more."""
import os
import struct
import subprocess

from tests import png_decode_cases as K
from tests import png_decode_restatement as R
from tests.test_jpeg_decode_core import _compiler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tests", "png_decode_core_main.cpp")
MAGIC = 0x3144504E


def _record(name, data):
    info, _, status, done, _ = R.decode_stream(data)
    name = name.encode()
    parts = [struct.pack("<I", len(name)), name, struct.pack("<IIII", info["h"], info["w"], info["color_type"], info["bpp"]),
             info["palette"].tobytes(), struct.pack("<I", len(info["stream"])), info["stream"], struct.pack("<iI", status, done)]
    for layout in K.LAYOUTS:
        px = R.decode(data, layout)[0].tobytes()
        parts += [struct.pack("<I", len(px)), px]
    return b"".join(parts), status


def _case_file(path):
    records, kinds = [], {}
    for case in K.CASES:
        rec, status = _record(case.name, K.make_file(case))
        assert status == R.OK
        records.append(rec)
    for h in K.hostile_cases():
        rec, status = _record(h.name, h.data)
        kinds[status] = kinds.get(status, 0) + 1
        records.append(rec)
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC, len(records)) + b"".join(records))
    return len(records), kinds


def test_core_decode_under_the_sanitizers(tmp_path):
    exe, cases = str(tmp_path / "png_decode_core_main"), str(tmp_path / "cases.bin")
    build = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SOURCE, "-o", exe]
    done = subprocess.run(build, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    n, kinds = _case_file(cases)
    print(f"{n} cases: {len(K.CASES)} good, hostile by expected status {dict(sorted(kinds.items()))}")
    assert set(kinds) == set(range(7))          # the hostile set reaches every status, and survival
    run = subprocess.run([exe, cases], capture_output=True, text=True)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == f"{n} cases, 0 failed" and "runtime error" not in run.stderr
