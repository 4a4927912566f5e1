"""Shared helpers: golden-case loading, column comparison, the constants of thresholds.hpp, the host layer's test programs."""
import json
import os
import re
import subprocess

import numpy as np

from rivulus_amd.capi import Column, Predicate, Term

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cases.json")
THRESHOLDS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rivulus_amd", "csrc", "thresholds.hpp")
_NP = {"i": np.int64, "f": np.float64, "b": np.bool_}


def _decode_col(c):
    if c["kind"] == "f":
        vals = np.array([float.fromhex(x) for x in c["values"]], np.float64)
    else:
        vals = np.array(c["values"], _NP[c["kind"]])
    valid = None if c["valid"] is None else np.array(c["valid"], bool)
    return Column.from_numpy(vals, valid)


def load_golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for case in doc["cases"]:
        terms = []
        for t in case["predicate"]["terms"]:
            lit = t["literal"]
            if t["literal_is_float"]:
                lit = float.fromhex(lit)
            terms.append(Term(t["column"], t["op"], lit))
        out.append({
            "name": case["name"],
            "columns": [_decode_col(c) for c in case["columns"]],
            "predicate": Predicate(terms, case["predicate"]["nulls"], case["predicate"].get("expr")),
            "projection": case["projection"],
            "rows": case["rows"],
            "expected": [_decode_col(c) for c in case["expected"]],
        })
    return out


def assert_columns_equal(got, expected, what=""):
    assert len(got) == len(expected), f"{what}: {len(got)} columns != {len(expected)}"
    for j, (g, e) in enumerate(zip(got, expected)):
        diff = g.same_as(e)
        assert diff is None, f"{what} column {j}: {diff}"


def const(name):
    """The value of constant `name` in rivulus_amd/csrc/thresholds.hpp (tests name a switch, never its value)."""
    with open(THRESHOLDS) as f:
        m = re.search(rf"\b{name} = ([^;,]+)[;,]", f.read())
    v = m.group(1).strip()
    if "<<" in v:
        a, b = re.findall(r"\d+", v)[-2:]
        return int(a) << int(b)
    return float(v) if "." in v else int(v)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_host_runs = {}


def host_cases(binary):
    """(CPU case names, GPU case names) of tests/cpp/<binary>.cpp"""
    with open(os.path.join(ROOT, "tests", "cpp", binary + ".cpp")) as f:
        src = f.read()
    return re.findall(r"^CPU_TEST\((\w+)\)", src, re.M), re.findall(r"^GPU_TEST\((\w+)\)", src, re.M)


def assert_host_case(binary, case, cpu_only, arg=None, timeout=300):
    """`case` of the host test program `binary` printed "ok".  The library and the program are built, and the program run, once per
    mode (cpu_only: its --cpu cases alone); arg() gives the program's own argument, a directory, when it takes one."""
    import pytest

    if (binary, cpu_only) not in _host_runs:
        subprocess.run(["make", "-C", os.path.join(ROOT, "rivulus_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
        subprocess.run(["make", "-C", os.path.join(ROOT, "rivulus_amd", "host"), binary], check=True, stdout=subprocess.DEVNULL)
        cmd = [os.path.join(ROOT, "rivulus_amd", "host", binary)] + (["--cpu"] if cpu_only else []) + ([arg()] if arg else [])
        _host_runs[binary, cpu_only] = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    result = _host_runs[binary, cpu_only]
    for line in result.stdout.splitlines():
        if line.split()[1:2] == [case] or line.startswith(f"FAIL {case}:"):
            assert line.startswith("ok "), line
            return
    pytest.fail(f"case {case} produced no line; stdout: {result.stdout[-1000:]} stderr: {result.stderr[-1000:]}")
