"""One n=16384 RGG engine run, summarised as JSON on the last stdout line.

The sweep tunables MV_NO_ITER1 / MV_SLOTS / MV_SLOTS_FIRST / MV_FIRST_ITERS
are read once per process, so test_gpu_sweep_switches.py runs this file as a
fresh child with them set; run() is also imported for the in-process cases.

usage: _sweep_child.py WORLD {unit|w}     (WORLD > 1: loopback on one GPU)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NV = 16384


def run(world, unit):
    """{"ranks": [{iters, final_mod_hex, iter_mod_hex}], "iter_target_sha",
    "sweep_launches"}; targets are stitched over the ranks before hashing."""
    from oracle.oracle import sha
    if world == 1:
        from test_gpu_parity import _run_engine_single
        mod, iters, tt, tm, stats = _run_engine_single(NV, unit=unit)
        results = {0: (mod, iters, tt, [float(m).hex() for m in tm])}
        launches = stats["sweep_launches"]
    else:
        from test_gpu_loopback import _run_loopback
        results = _run_loopback(NV, world, unit=unit)
        launches = None
    iters = results[0][1]
    parts = [(NV * r) // world for r in range(world + 1)]
    shas = []
    for k in range(min(iters, 64)):
        full = np.zeros(NV, dtype=np.int64)
        for r in range(world):
            full[parts[r]:parts[r + 1]] = results[r][2][k]
        shas.append(sha(full))
    return {
        "ranks": [{"iters": results[r][1],
                   "final_mod_hex": float(results[r][0]).hex(),
                   "iter_mod_hex": results[r][3]} for r in range(world)],
        "iter_target_sha": shas,
        "sweep_launches": launches,
    }


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]), sys.argv[2] == "unit")))
