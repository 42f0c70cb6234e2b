"""What one exchange of dist.ExactShardedTracer costs on one device: halo_export_fixed, the int64 all_reduce, halo_import_fixed + the
closing fold, at 1920 x 1080 for a scalar plane (a discrete wavelength) and for X, Y, Z (an illuminant).

  python tools/exact_shards_cost.py [--iters 20] [--gloo]

Per call it prints the host wall time (the calls wait for the device, so wall time is what a rank pays) and HIP events on the backend's stream
around the import kernel and around the fold.  The kernels' own durations come from running this script under `rocprofv3 --kernel-trace` (the dispatches of
halo_export_fixed_kernel, halo_import_fixed_kernel, halo_fold_fixed_kernel in its kernel table).  --gloo adds a one-rank-per-process all_reduce over gloo with two
ranks on this device: device -> host -> TCP -> device, a rehearsal of the call path that says nothing about RCCL over xGMI."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ice_halo_sim_amd import abi, scenes  # noqa: E402


def measure(iters, wl, label, reduce=False):
    import torch
    from ice_halo_sim_amd.backend import HipTraceBackend
    full = {"type": "uniform", "mean": 0.0, "std": 360.0}
    sc = scenes.scene([(0.0, [scenes.entry(scenes.prism_crystal(1.0), scenes.axis(zenith=full, azimuth=full, roll=full), 1.0, 1)])], max_hits=7)
    rd = scenes.render(abi.LENS_FISHEYE_EQUAL_AREA, 1920, 1080, fov=180.0, el=30.0, visible=abi.VISIBLE_UPPER)
    stream = torch.cuda.Stream()
    hb = HipTraceBackend(device=0, seed=42, deterministic=1)
    hb.set_stream(stream.cuda_stream)
    n = 1 << 20
    t_exp, t_red, t_imp, ev_imp, ev_fold = [], [], [], [], []
    words = None
    for it in range(iters + 2):
        hb.BeginSession(sc, rd, wl, n)
        hb.TraceLayer(n)
        hb.EndSession()
        hb.sync()
        if words is None:
            words = torch.empty(hb.fixed_words(), dtype=torch.int64, device="cuda:0")
        t0 = time.perf_counter()
        layout = hb.export_fixed(words)
        t1 = time.perf_counter()
        if reduce:
            import torch.distributed as dist
            dist.all_reduce(words, op=dist.ReduceOp.SUM)
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        # HIP events on the backend's stream: around the import kernel (the call queues it at once and then reads the 8-byte landed word behind
        # it), and around the fold.  The export kernel cannot be bracketed from outside — the call first reads the tally and waits for the host —
        # so its own duration comes from the kernel trace.
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(stream)
        hb.import_fixed(words, *layout, n)
        e1.record(stream)
        hb.flush()
        e2.record(stream)
        stream.synchronize()
        t3 = time.perf_counter()
        if it >= 2:
            t_exp.append((t1 - t0) * 1e6), t_red.append((t2 - t1) * 1e6), t_imp.append((t3 - t2) * 1e6)
            ev_imp.append(e0.elapsed_time(e1) * 1e3), ev_fold.append(e1.elapsed_time(e2) * 1e3)
    hb.ReadbackXyzAccum()
    hb.close()
    med = statistics.median
    mb = words.numel() * 8 / 1e6
    print("%-14s words %9d (%.1f MB)  export call %7.1f us  all_reduce %9.1f us  import + fold call %7.1f us  (HIP events: import %6.1f us, fold %6.1f us)"
          % (label, words.numel(), mb, med(t_exp), med(t_red), med(t_imp), med(ev_imp), med(ev_fold)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--gloo", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    if args.gloo:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    measure(args.iters, scenes.wl_discrete(550.0), "scalar plane", reduce=args.gloo)
    measure(args.iters, scenes.wl_illuminant("D65", 31), "X, Y, Z", reduce=args.gloo)
    if args.gloo:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
