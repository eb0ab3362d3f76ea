#!/usr/bin/env python3
"""What checkpoint / resume costs on one MI355X (profiles/r06_resume.txt).

    python tools/resume_timing.py [--chains 65536] [--n-steps 100000]

1. The restore kernel (mcq_run_device_from with placements and streams) and the checkpoint kernel against the init kernel of the same
   launch (mcq_run_device_timed's init_ms), N = 12, board and full_3d.
2. The headline shape (N = 12 board, full trace) as 1, 4 and 16 device-resident segments: moves/s of each, wall time around the whole
   chain of launches (restore + sweep + checkpoint per segment, nothing copied to the host in between)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--n-steps", type=int, default=100000)
    args = ap.parse_args()
    import torch

    import mcq_amd

    abi = mcq_amd.abi
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    st = torch.cuda.current_stream()
    seeds = abi.seeds_for(42, args.chains)
    for mode in ("board", "full_3d"):
        k = 2000
        p = abi.make_params(12, k, "random", sp, args.chains, mcmc_type=mode)
        run = mcq_amd._lib.DeviceRun(p, seeds, schedule_steps=2 * k)
        run.launch_from(0, stream=st)
        ss = run.checkpoint(stream=st)
        state = run.t["final_state"].clone()
        st.synchronize()
        init_ms = min(run.launch_from(0, stream=st, timed=True)[0] for _ in range(3))
        restore_ms = min(run.launch_from(k, state=state, stream_state=ss, stream=st, timed=True)[0] for _ in range(3))
        seeded_ms = min(run.launch_from(k, state=state, stream=st, timed=True)[0] for _ in range(3))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ck = []
        for _ in range(3):
            e0.record(st)
            run.checkpoint(ss, stream=st)
            e1.record(st)
            st.synchronize()
            ck.append(e0.elapsed_time(e1))
        print(f"{mode} N=12 chains={args.chains}: init kernel {init_ms:.3f} ms | restore kernel {restore_ms:.3f} ms (placements + streams), "
              f"{seeded_ms:.3f} ms (placements, seeded) | checkpoint kernel {min(ck):.3f} ms", flush=True)
        del run
    total = args.n_steps
    for segments in (1, 4, 16):
        k = total // segments
        p = abi.make_params(12, k, "random", sp, args.chains, mcmc_type="board")
        run = mcq_amd._lib.DeviceRun(p, seeds, schedule_steps=k * segments)
        best = None
        for rep in range(3):
            state = ss = None
            st.synchronize()
            t0 = time.perf_counter()
            for i in range(segments):
                run.launch_from(i * k, state=state, stream_state=ss, stream=st)
                if segments > 1:
                    ss = run.checkpoint(ss, stream=st)
                    state = run.t["final_state"]  # (the restore kernel has read it before the sweep of the same launch writes it)
            st.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        print(f"board N=12 chains={args.chains} steps={k * segments} full trace, {segments:2d} segment(s): {best * 1e3:8.2f} ms  "
              f"{args.chains * k * segments / best:.4e} moves/s", flush=True)
        del run


if __name__ == "__main__":
    main()
