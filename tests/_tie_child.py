"""One p=1 engine run on the relabelled composite (unit weights): the trace
goes to the .npz named on the command line, Engine.sweep_info() as JSON to
the last stdout line.

MV_LH_THRESH / MV_HI_THRESH are read once per process, so
test_gpu_tie_parity.py runs this file as a fresh child with them set.

usage: _tie_child.py OUT.npz
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(out):
    import _tie_graphs as tg
    from minivite_amd import Graph, Engine
    xadj, tails, w = tg.composite_relabelled()
    nv = len(xadj) - 1
    g = Graph.from_csr(nv, 0, 1, tg.even_parts(nv, 1), xadj, tails, w)
    e = Engine(device=0)
    e.load_graph(g)
    e.set_trace(64)
    mod, iters = e.run()
    tt, tm = e.trace(iters)
    info = e.sweep_info()
    np.savez(out, mod=mod, iters=iters, targets=tt, mods=tm)
    e.destroy()
    g.free()
    print(json.dumps(info))


if __name__ == "__main__":
    main(sys.argv[1])
