"""Baseline timing of the multi-phase driver: unit RGG n=2^22 (the bench
workload's graph), run_ms and coarsen_ms per phase from mv_phase_info.

run_ms is the wall time of the phase's mv_engine_run (setup + loop, ends in
a stream synchronise); coarsen_ms is the wall time of the aggregation
(device pipeline, synchronised, + the copy of the coarse CSR to the host
level). The graph upload (mv_engine_load_graph) of each level is outside
both and shows in the total. The first pass warms code objects and hipCUB;
the passes after it are the figures to quote.

With a rank count above 1 the distributed driver runs over the loopback
transport: that many engines on ONE device, one host thread per rank, every
exchange a device-to-device copy between host barriers. The ranks share
the device, so these are single-device loopback figures for the protocol's
overhead, not scaling numbers. Rank 0's records are printed.

Usage: python experiments/multiphase_timing.py [log2_nv] [passes] [ranks]
"""
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from minivite_amd import Graph, Engine, LoopbackSession  # noqa: E402


def report(k, h, total):
    print(f"pass {k}{' (warm-up)' if k == 0 else ''}: {h.phases} phases, "
          f"{h.levels} levels, q={h.modularity(h.levels):.10f}, "
          f"total {total:.1f} ms")
    for p in range(1, h.phases + 1):
        i = h.phase_info(p)
        print(f"  phase {p}: nv_in={i['nv_in']} ne_in={i['ne_in']} "
              f"iters={i['iters']} run_ms={i['run_ms']:.3f} "
              f"coarsen_ms={i['coarsen_ms']:.3f} nv_out={i['nv_out']} "
              f"q_out={i['q_out']:.6f} kept={int(i['kept'])}", flush=True)


def loopback(lg, passes, world):
    ses = LoopbackSession(world)
    errors = []

    def rank_main(r):
        try:
            g = Graph.rgg(1 << lg, r, world)
            e = Engine.loopback(ses, r, device=0)
            for k in range(passes):
                t0 = time.perf_counter()
                h = e.run_multiphase_dist(g)
                total = (time.perf_counter() - t0) * 1e3
                if r == 0:
                    report(k, h, total)
                h.free()
            e.destroy()
            g.free()
        except Exception as ex:
            errors.append((r, repr(ex)))

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True)
               for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    if errors or any(t.is_alive() for t in threads):
        sys.exit(f"loopback run failed: {errors or 'a rank is stuck'}")
    ses.destroy()


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    world = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    if world > 1:
        print(f"unit RGG n=2^{lg}, {world} loopback ranks on one device")
        return loopback(lg, passes, world)
    g = Graph.rgg(1 << lg, 0, 1)
    print(f"unit RGG n=2^{lg}: {g.lne} directed edges")
    e = Engine(device=0)
    for k in range(passes):
        t0 = time.perf_counter()
        h = e.run_multiphase(g)
        total = (time.perf_counter() - t0) * 1e3
        report(k, h, total)
        h.free()
    e.destroy()
    g.free()


if __name__ == "__main__":
    main()
