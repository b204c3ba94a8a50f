"""Baseline timing of the multi-phase driver: unit RGG n=2^22 (the bench
workload's graph), run_ms and coarsen_ms per phase from mv_phase_info.

run_ms is the wall time of the phase's mv_engine_run (setup + loop, ends in
a stream synchronise); coarsen_ms is the wall time of the aggregation
(device pipeline, synchronised, + the copy of the coarse CSR to the host
level). The graph upload (mv_engine_load_graph) of each level is outside
both and shows in the total. The first pass warms code objects and hipCUB;
the passes after it are the figures to quote.

Usage: python experiments/multiphase_timing.py [log2_nv] [passes]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from minivite_amd import Graph, Engine  # noqa: E402


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    g = Graph.rgg(1 << lg, 0, 1)
    print(f"unit RGG n=2^{lg}: {g.lne} directed edges")
    e = Engine(device=0)
    for k in range(passes):
        t0 = time.perf_counter()
        h = e.run_multiphase(g)
        total = (time.perf_counter() - t0) * 1e3
        print(f"pass {k}{' (warm-up)' if k == 0 else ''}: {h.phases} phases, "
              f"{h.levels} levels, q={h.modularity(h.levels):.10f}, "
              f"total {total:.1f} ms")
        for p in range(1, h.phases + 1):
            i = h.phase_info(p)
            print(f"  phase {p}: nv_in={i['nv_in']} ne_in={i['ne_in']} "
                  f"iters={i['iters']} run_ms={i['run_ms']:.3f} "
                  f"coarsen_ms={i['coarsen_ms']:.3f} nv_out={i['nv_out']} "
                  f"q_out={i['q_out']:.6f} kept={int(i['kept'])}")
        h.free()
    e.destroy()
    g.free()


if __name__ == "__main__":
    main()
