"""The standard-form NMEA armouring under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program
(tests/emul_nmea_std `make san`: nmea_std_san.cpp = the lane model of the kernel bodies + the host function): the lists
of tests/nmea_std_cases.py and the cuts, calls and refusals of tests/test_nmea_std_model.py, every call fed from heap
blocks of exactly its size, every text compared with the host function's inside the program.  Nothing is loaded into
Python; the program inherits the environment as it is.  -m "not gpu"."""
import os
import struct
import subprocess

import numpy as np
import pytest

import nmea_std_cases as sc

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul_nmea_std")


@pytest.fixture(scope="module")
def program():
    subprocess.check_call(["make", "-C", EMUL, "-s", "san"])
    return os.path.join(EMUL, "nmea_std_san")


def write_cases(path, cases):
    """cases: [(case dict, [call dict: time / npdus / reset / records, defaults from the case])]"""
    with open(path, "wb") as f:
        for case, calls in cases:
            f.write(struct.pack("<I", len(case["designators"])))
            for d, s in zip(case["designators"], case["stations"]):
                f.write(bytes([len(d)]) + d.encode("latin-1") + bytes([len(s)]) + s.encode("latin-1"))
            max_pdus = case.get("max_pdus", max([len(c.get("records", case["records"])) for c in calls] + [1]))
            f.write(struct.pack("<iiqI", case["length_max"], max_pdus, case.get("text_cap", 0), len(calls)))
            for c in calls:
                recs = c.get("records", case["records"])
                f.write(struct.pack("<qiBI", c.get("time", case.get("time", -1)), c.get("npdus", len(recs)), int(c.get("reset", 0)),
                                    len(recs)))
                for chan, _, p in recs:
                    f.write(struct.pack("<ii", chan, len(p)) + bytes(p))


def test_lists_cuts_calls_and_refusals(program, tmp_path):
    rng = np.random.default_rng(41)
    cases = [(c, [{}]) for c in sc.all_cases(rng)]
    cases.append((sc.many(rng, 2 * 1024 + 300, 1024), [{}]))  # more than one scan tile of the model
    # ids over three calls with the wrap, a reset, a call of single sentences only
    mixed = sc.mixed(rng)
    cases.append((mixed, [dict(time=-1), dict(time=7), dict(time=sc.T18), dict(reset=1), dict(records=mixed["records"][:3])]))
    # text_cap at, just before and just after a record of two sentences, two calls each
    want = sc.expected(mixed)[0]
    k = 150 + [sc.is_multi(p) for _, _, p in mixed["records"][150:]].index(True)
    before = sum(len(t) + 1 for _, _, t in want[:k] if t)
    whole = before + len(want[k][2]) + 1
    for cap in (before, before + 1, before + len(want[k][2].split("\n")[0]) + 1, whole - 1, whole, whole + 1, 1):
        cases.append((dict(mixed, text_cap=cap), [{}, {}]))
    # counts out of range between good calls, empty lists
    cases.append((mixed, [dict(npdus=-1), {}, dict(npdus=len(mixed["records"]) + 1), {}, dict(npdus=0), dict(records=[])]))
    path = str(tmp_path / "cases.bin")
    write_cases(path, cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.returncode, r.stderr[-3000:])
    assert r.stdout.startswith("%d cases, %d calls" % (len(cases), sum(len(c) for _, c in cases))), r.stdout
