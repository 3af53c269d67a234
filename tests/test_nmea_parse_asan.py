"""The host NMEA parser under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program
(tests/emul_nmea_parse/parse_san.cpp + gr-ais_amd/csrc/aisx_nmea_parse.cpp): the cases of tests/nmea_parse_cases.py,
seeded byte-level mutations of them under random cuts, very long lines and 10^5 lines in one call, every call fed from
a heap block of exactly its size.  Nothing is loaded into Python; the program inherits the environment as it is.  -m "not gpu"."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import nmea_parse_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = [os.path.join(HERE, "emul_nmea_parse", "parse_san.cpp"), os.path.join(ROOT, "gr-ais_amd", "csrc", "aisx_nmea_parse.cpp")]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nmea_parse_san") / "parse_san")
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    # the sanitizer runtimes linked statically: the program then runs whatever else the environment has loaded first
    probe = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout.lower()
    static = ["-static-libsan"] if "clang" in probe else ["-static-libasan", "-static-libubsan"]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined"] + static + ["-o", out] + SRC, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr or "libsan" in r.stderr:
            pytest.skip("the compiler cannot link the sanitizers: " + r.stderr[-300:])
        raise AssertionError(r.stderr[-3000:])
    return out


def write_cases(path, cases):
    with open(path, "wb") as f:
        for calls in cases:
            f.write(struct.pack("<I", len(calls)))
            for c in calls:
                f.write(struct.pack("<I", len(c)) + c)


def run(program, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stderr[-3000:])
    return r.stdout


def test_cases_and_mutations(program, tmp_path):
    rng = np.random.default_rng(4242)
    cases = []
    for name, text in nc.build_cases():
        cases.append([text])
        cases.append(nc.pieces(text, nc.random_cuts(rng, len(text), 5)))
        for m in nc.mutations(rng, text, 12 if name != "mixed" else 60):
            cases.append(nc.pieces(m, nc.random_cuts(rng, len(m), int(rng.integers(0, 6)))))
    for k in range(40):  # random bytes, with the grammar's own characters frequent
        alphabet = np.frombuffer(b"!\\,*\r\n\nAIVDM0123456789ABc:" + bytes(range(256)), dtype=np.uint8)
        t = bytes(alphabet[rng.integers(0, len(alphabet), int(rng.integers(1, 3000)))])
        cases.append(nc.pieces(t, nc.random_cuts(rng, len(t), k % 7)))
    path = str(tmp_path / "cases.bin")
    write_cases(path, cases)
    out = run(program, path)
    assert out.startswith("%d cases" % len(cases))


def test_long_lines_and_many_lines(program, tmp_path):
    good = nc.GOOD + b"\n"
    long_line = b"\\" + b"c:1," * 5000 + b"\\" + nc.GOOD
    cases = [
        [good * 100000],                                      # 10^5 lines in one call
        [long_line + b"\n" + good],                           # 20 KB in one line, whole
        [long_line[:7000], long_line[7000:], b"\n" + good],   # ... in three calls
        [b"!" * 100000, b"\n"],                               # no line end for 100 KB
        [b"\n" * 100000],
        [b"\\" * 129, b"\\" * 129 + b"\n" + good],
        [b"\r" * 300 + b"\n" + good],
        [b"\\c:" + b"\x80" * 18 + b",c:" + b"\xff" * 18 + b"\\" + nc.GOOD + b"\n"],  # no digits where 18 digits may stand
    ]
    path = str(tmp_path / "long.bin")
    write_cases(path, cases)
    out = run(program, path)
    assert out.startswith("8 cases") and "100006 messages" not in out
    lines = int(out.split(" lines")[0].split()[-1])
    assert lines == 100000 + 2 + 2 + 1 + 100000 + 2 + 2 + 1
