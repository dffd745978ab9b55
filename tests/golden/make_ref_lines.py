#!/usr/bin/env python3
"""Regenerates tests/golden/ref_lines.json: what the reference's own lines (oracle/_ref/, built by
oracle/make_ref.sh from the reference checkout) answered to every call the pin tests make —
readMtx, COO->CSR, B init, the CPU golden loop and the mmio.hpp header parser — as fingerprints
keyed by the fingerprints of the inputs (tests/ref_lines.py). Run where oracle/_ref is built:

    python tests/golden/make_ref_lines.py

It runs those tests against the live lines and records every answer; machines without the
reference replay the record, machines with it check the record against the lines.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_py  # noqa: E402

TESTS = ["tests/test_ref_pin.py", "tests/test_oracle_loader.py"]


def main():
    if not ref_py.available():
        raise SystemExit("oracle/_ref is not built: run __graft_entry__.build() where the reference checkout is")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "ref_lines.json")
        env = dict(os.environ, GESPMM_RECORD_REF_LINES=out)
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env)
        if r.returncode != 0:
            raise SystemExit("the pin tests failed against the live reference lines: nothing recorded")
        with open(out) as f:
            data = f.read()
    with open(os.path.join(HERE, "ref_lines.json"), "w") as f:
        f.write(data)
    print("wrote tests/golden/ref_lines.json (%d bytes)" % len(data))


if __name__ == "__main__":
    main()
