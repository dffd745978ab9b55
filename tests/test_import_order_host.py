"""``import gespmm_amd`` in a process that has not imported torch yet must end with ONE HIP runtime mapped: libgespmm.so loaded before
torch pulls in the system's libamdhip64, torch then loads the copy it ships, and with two runtimes in the process every call of the
library fails with "no ROCm-capable device is detected" (seen on the MI355X from a script that imported the package first). The
package therefore imports torch before it loads the library; a fresh child process is what this is about."""
import os
import subprocess
import sys

from helpers import ROOT

CHILD = """
import sys
sys.path.insert(0, %r)
%s
names = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
print("\\n".join(names))
"""


def _hip_runtimes(imports):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, imports)], check=True, capture_output=True, text=True, env=env).stdout
    return [line for line in out.splitlines() if line]


def test_package_first_maps_one_hip_runtime():
    first = _hip_runtimes("import gespmm_amd")
    assert len(first) == 1, first
    assert _hip_runtimes("import torch, gespmm_amd") == first
