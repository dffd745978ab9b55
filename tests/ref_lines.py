"""The reference's own lines as the tests see them: live from oracle/_ref/ where it was built, else replayed from
tests/golden/ref_lines.json — what those lines returned, recorded where the reference was built.

Every call is keyed by the fingerprints of its inputs (a file by its bytes) and answers with fingerprints of its outputs, so a
test compares `fp(mine) == REF.<call>(...)` the same way in both modes: bit for bit for floats, by value for integers. Live, each
answer is also checked against the record, so the record cannot drift from the lines it stands for; a call the record lacks is
an error when replaying. Regenerate the record (`python tests/golden/make_ref_lines.py`) where oracle/_ref is built.
"""
import atexit
import hashlib
import json
import os

import numpy as np

import oracle_py
import ref_py

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_lines.json")
RECORD_ENV = "GESPMM_RECORD_REF_LINES"  # set to a path: run live and write every answer there at exit


def fp(a):
    """Fingerprint of an array: shape + integers by value (any int dtype) or floats by their float32 bits. A fingerprint passes
    through unchanged."""
    if isinstance(a, str):
        return a
    a = np.asarray(a)
    if a.dtype.kind in "iub":
        kind, data = "i", np.ascontiguousarray(a, dtype=np.int64)
    elif a.dtype.kind == "f":
        kind, data = "f", np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    else:
        raise TypeError("no fingerprint for dtype %s" % a.dtype)
    h = hashlib.sha256(("%s%r" % (kind, tuple(a.shape))).encode())
    h.update(data.tobytes())
    return h.hexdigest()[:32]


def _file_fp(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:32]


def _key(name, *parts):
    return name + ":" + hashlib.sha256(json.dumps([str(p) for p in parts]).encode()).hexdigest()[:32]


class RefLines:
    def __init__(self):
        self.record_to = os.environ.get(RECORD_ENV)
        self.live = ref_py.available() or bool(self.record_to)
        self.record = {}
        if os.path.exists(RECORD) and not self.record_to:
            with open(RECORD) as f:
                self.record = json.load(f)
        self.seen = {}
        if self.record_to:
            atexit.register(self._write)

    def _write(self):
        with open(self.record_to, "w") as f:
            json.dump(dict(sorted(self.seen.items())), f, indent=0, sort_keys=True)
            f.write("\n")

    def _answer(self, key, live_fn):
        if not self.live:
            assert key in self.record, ("%s is not in tests/golden/ref_lines.json: regenerate it where oracle/_ref is built "
                                        "(python tests/golden/make_ref_lines.py)" % key)
            return self.record[key]
        got = json.loads(json.dumps(live_fn()))
        if key in self.record:
            assert got == self.record[key], "the reference's lines no longer answer what tests/golden/ref_lines.json recorded: %s" % key
        self.seen[key] = got
        return got

    # ---- util.hpp readMtx<float> (as a process), spmm_test.cu COO->CSR, B init, CPU golden loop, mmio.hpp header parser
    def read_mtx(self, path):
        def live():
            r = ref_py.read_mtx(path)
            if r["rc"] != 0:
                return {"rc": r["rc"]}
            out = {k: r[k] for k in ("rc", "nrows", "ncols", "nvals", "tuples")}
            out.update({k: fp(r[k]) for k in ("row", "col", "val")})
            return out

        return self._answer(_key("read_mtx", _file_fp(path)), live)

    def coo_to_csr(self, nrows, ncols, row, col):
        def live():
            ip, ix, d = ref_py.coo_to_csr(nrows, ncols, row, col)
            return {"indptr": fp(ip), "indices": fp(ix), "data": fp(d)}

        return self._answer(_key("coo_to_csr", nrows, ncols, fp(row), fp(col)), live)

    def fill_B(self, seed, max_ncols, A_ncols):
        return self._answer(_key("fill_B", seed, max_ncols, A_ncols), lambda: fp(ref_py.fill_B(seed, max_ncols, A_ncols)))

    def golden(self, indptr, indices, data, B):
        return self._answer(_key("golden", fp(indptr), fp(indices), fp(data), fp(B)),
                            lambda: fp(ref_py.golden(indptr, indices, data, B)))

    def mmio_probe(self, path):
        def live():
            r = oracle_py.ref_mmio_probe(path)
            assert r is not None, "oracle/_ref/mmio_probe was not built with the other reference lines"
            return r

        return self._answer(_key("mmio_probe", _file_fp(path)), live)


REF = RefLines()
