"""One engine run per rank on a _unit_count_graphs input: the target traces
go to the .npz named on the command line, {rank: {mod, iters, mods, info}}
as JSON to the last stdout line.

MV_SLOTS / MV_SLOTS_FIRST / MV_NO_ITER1 are read once per process, so
test_gpu_unit_counts.py runs this file as a fresh child with them set.

usage: _unit_counts_child.py GRAPH MODE WORLD OUT.npz   (WORLD > 1: loopback
on one GPU)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(name, mode, world, out):
    import _tie_graphs as tg
    import _unit_count_graphs as ug
    from test_gpu_tie_parity import _run_engines
    csr = ug.graph(name, mode)
    parts = tg.even_parts(len(csr[0]) - 1, world)
    results = _run_engines(csr, parts)
    np.savez(out, **{f"targets{r}": res[2] for r, res in results.items()})
    print(json.dumps({r: {"mod": float(res[0]).hex(), "iters": res[1],
                          "mods": res[3], "info": res[4]}
                      for r, res in results.items()}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4])
