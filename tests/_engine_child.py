"""One engine run per rank in a process of its own: the target rows and
communities go to the .npz named on the command line, the rest of every
rank's record ({rank: record}, see _gpu_run.py) as JSON to the last stdout
line.

MV_NO_ITER1 / MV_SLOTS / MV_SLOTS_FIRST / MV_FIRST_ITERS / MV_LH_THRESH /
MV_HI_THRESH are read once per process, so the tests that set them run this
file as a fresh child through _gpu_run.in_child().

usage: _engine_child.py SPEC WORLD OUT.npz   (WORLD > 1: loopback on one GPU)
  SPEC  rgg:NV:unit | rgg:NV:w      the generated RGG, split evenly
        tie:NAME                    _tie_graphs.NAME(), split evenly
        unitcount:NAME:MODE         _unit_count_graphs.graph(NAME, MODE)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def run(spec, world):
    import _gpu_run as gr
    import _tie_graphs as tg
    kind, *args = spec.split(":")
    if kind == "rgg":
        nv, weights = args
        return gr.run_rgg(int(nv), world, unit={"unit": True,
                                                 "w": False}[weights])
    if kind == "tie":
        csr = getattr(tg, args[0])()
    elif kind == "unitcount":
        import _unit_count_graphs as ug
        csr = ug.graph(*args)
    else:
        raise SystemExit(f"unknown graph spec {spec!r}")
    parts = tg.even_parts(len(csr[0]) - 1, world)
    records, = gr.run_csrs(tg.split(csr, parts), parts, join_s=300)
    return records


def main(spec, world, out):
    from _gpu_run import _ARRAYS
    records = run(spec, world)
    np.savez(out, **{f"{f}{r}": rec[f] for r, rec in records.items()
                     for f in _ARRAYS})
    print(json.dumps({r: {k: v for k, v in rec.items() if k not in _ARRAYS}
                      for r, rec in records.items()}))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3])
