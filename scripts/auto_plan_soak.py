"""Soak of the auto-plan cache (csrc/auto_plan.cpp) on two streams: seeded random sequences of stateless calls (valued and unweighted
sums, the max reducer, the DGL sum), weight flips in place, value-pointer switches, in-place pattern edits, new dense operands and
short gates on the headline graph, no host synchronisation per call — every call against the product of the same state with the switch
off, bit for bit. The engine is tests/helpers.py: auto_plan_soak (the suite runs one short seed of it). One line per seed.
    python scripts/auto_plan_soak.py [first_seed] [count] [steps]"""
import os, sys, time
import torch
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import gespmm_amd
from gespmm_amd import _lib, graphs
from helpers import auto_plan_soak, sleep_cycles_per_ms


def main(first, count, steps):
    t0 = time.time()
    g = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda")
    cpms = sleep_cycles_per_ms()
    print(f"com-amazon-sbm M={g['M']} nnz={g['nnz']} N=128, {steps} steps per seed, sleep clock {cpms:.0f} cycles/ms", flush=True)
    calls = bad_seeds = 0
    for seed in range(first, first + count):
        ts = time.time()
        failures, d, ncalls = auto_plan_soak(_lib, g, seed=seed, steps=steps, cycles_per_ms=cpms)
        calls += ncalls
        bad_seeds += bool(failures)
        print(f"seed {seed}: {ncalls} calls, {len(failures)} mismatching; planned {d['calls_planned']} async {d['calls_async']} "
              f"fingerprints {d['fingerprints']} plans {d['plans_created']} invalidated {d['invalidated']} "
              f"values_refreshed {d['values_refreshed']}; {time.time() - ts:.1f} s"
              + (f"; first failures (step, stream, op, state, words): {failures[:5]}" if failures else ""), flush=True)
    print(f"TOTAL {count} seeds, {calls} calls, {bad_seeds} seeds with mismatches, {time.time() - t0:.0f} s", flush=True)
    return 1 if bad_seeds else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    sys.exit(main(int(a[0]) if a else 0, int(a[1]) if len(a) > 1 else 20, int(a[2]) if len(a) > 2 else 1000))
