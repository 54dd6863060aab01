"""usage (GPU box): python tools/adaptive_rate.py [out.txt] -- adaptive sampling (wpt_render_adaptive_block_device) against the
plain render (wpt_render_block_device).  Milliseconds, median of 5 runs after one untimed run.
  1. The cost of the adaptive kernel at a constant map n = 8 (64 spp), with and without the moment film: the Cornell frame of
     BASELINE config 2 (GGX + glass, scene in LDS) at 1024^2 and the Sponza-class frame (scene in HBM) at 1920x1080.
  2. The cost order on (default) against off (variant bit 0x40), for a map with 24 8x8 tiles at n = 32 and the rest at n = 2.
  3. The value at equal time, on the Sponza-class scene at 960x540: the RMSE against a 32^2-spp plain render of (a) the
     uniform render at n = 8 and (b) a pilot at n = 4 with moments, then the adaptive render from samples_sqrt_for_error, whose
     relError is chosen (bisection on the measured time) so that pilot and adaptive render together take the uniform render's
     time.  The pilot's time counts in (b); its samples are not merged into the final frame.  For comparison, (b) also at an
     equal sample count.
Every map is a CUDA tensor of torch.uint16 made before the timed calls: the adaptive launch is timed without any host-side work
on the map."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import device, host

REPS = 5


def timed(fn, reps=REPS):
    """median milliseconds of `reps` runs of fn() on the current stream, after one untimed run"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def u16(a):
    """a map as a CUDA tensor of torch.uint16 (the binding takes it as it is)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint16)).view(np.int16)).to("cuda").view(torch.uint16)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adaptive_rate.txt")
    L = device.lib()
    stream = torch.cuda.current_stream()
    lines = ["# python tools/adaptive_rate.py on one MI355X; milliseconds, median of %d runs after one untimed run" % REPS,
             "# library %s" % bench.library_identity()]

    lines.append("# 1. constant map n = 8 (64 spp): plain / adaptive without moments / adaptive with moments")
    for name, make in (("cornell_1024x1024", lambda: host.cornell(1024, 1024, 1, 2)),
                       ("sponza_like_1920x1080", lambda: host.sponza_like(1920, 1080))):
        sc = make()
        ds = device.DeviceScene(sc)
        h, w = sc.height, sc.width
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        moments = torch.zeros_like(frame)
        m = u16(np.full((h, w), 8))
        t_plain = timed(lambda: ds.render_block_into(frame, 8, stream=stream))
        t_ad = timed(lambda: ds.render_adaptive_into(frame, m, None, stream=stream))
        kernel = L.wpt_kernel_name().decode()
        t_adm = timed(lambda: ds.render_adaptive_into(frame, m, moments, stream=stream))
        ms = w * h * 64 / 1e6
        lines.append("%-24s plain %8.2f ms (%6.1f Msamples/s)  adaptive %8.2f ms (x%.3f)  with moments %8.2f ms (x%.3f)  [%s]"
                     % (name, t_plain, ms / t_plain * 1e3, t_ad, t_ad / t_plain, t_adm, t_adm / t_plain, kernel))
        print(lines[-1], flush=True)

        # 2. the cost order, same scene and frame
        mh = np.full((h, w), 2, np.int32)
        rng = np.random.default_rng(5)
        for _ in range(24):
            ty, tx = rng.integers(0, h // 8), rng.integers(0, w // 8)
            mh[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = 32
        mt = u16(mh)
        t_on = timed(lambda: ds.render_adaptive_into(frame, mt, None, stream=stream))
        try:
            L.wpt_set_launch_config(0, 0x40)
            t_off = timed(lambda: ds.render_adaptive_into(frame, mt, None, stream=stream))
        finally:
            L.wpt_set_launch_config(0, 0)
        lines.append("%-24s 2. heavy tiles (24 at n = 32, rest n = 2): cost order %8.2f ms, plain order (0x40) %8.2f ms (order gains x%.3f)"
                     % (name, t_on, t_off, t_off / t_on))
        print(lines[-1], flush=True)
        ds.close()

    lines.append("# 3. value at equal time (and at equal samples), Sponza-class 960x540: RMSE against a 32^2-spp plain render")
    sc = host.sponza_like(960, 540)
    ds = device.DeviceScene(sc)
    h, w = sc.height, sc.width
    frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ref = ds.render(32)[0].astype(np.float64)
    n_u, n_p = 8, 4
    t_u = timed(lambda: ds.render_block_into(frame, n_u, stream=stream))
    uni = ds.render(n_u)[0].astype(np.float64)
    pm = u16(np.full((h, w), n_p))
    moments = torch.zeros_like(frame)
    t_p = timed(lambda: ds.render_adaptive_into(frame, pm, moments, stream=stream))
    pilot, pmom = ds.render_adaptive(pm, with_moments=True)
    pilot, pmom = pilot.cpu().numpy(), pmom.cpu().numpy()
    budget = (n_u * n_u - n_p * n_p) * w * h
    rmse_u = float(np.sqrt(np.mean((uni - ref) ** 2)))
    lines.append("uniform n = %d: %d samples, %8.2f ms, RMSE %.5f" % (n_u, n_u * n_u * w * h, t_u, rmse_u))
    # floor 0.01: relative error down to dark pixels; floor = the pilot's mean value: about an absolute error where the frame is
    # darker than its mean, the measure RMSE rewards
    for floor in (0.01, float(np.mean(pilot))):
        def adaptive_for(rel):
            amap = device.samples_sqrt_for_error(pilot, pmom, n_p, rel, 1, 64, floor)
            am = u16(amap)
            return amap, am, timed(lambda: ds.render_adaptive_into(frame, am, None, stream=stream), reps=1)
        for target, what in ((t_u - t_p, "equal time"), (None, "equal samples")):
            lo, hi = 1e-4, 10.0
            for _ in range(25 if target is not None else 60):  # bisection on a log scale; a larger relError is cheaper
                mid = float(np.sqrt(lo * hi))
                if target is not None:
                    over = adaptive_for(mid)[2] > target
                else:
                    over = int((device.samples_sqrt_for_error(pilot, pmom, n_p, mid, 1, 64, floor).astype(np.int64) ** 2).sum()) > budget
                lo, hi = (mid, hi) if over else (lo, mid)
            rel = hi
            amap, am, _ = adaptive_for(rel)
            t_a = timed(lambda: ds.render_adaptive_into(frame, am, None, stream=stream))
            ad = ds.render_adaptive(am).cpu().numpy().astype(np.float64)
            rmse_a = float(np.sqrt(np.mean((ad - ref) ** 2)))
            total_a = int((amap.astype(np.int64) ** 2).sum())
            lines.append("%-13s pilot n = %d + adaptive (floor %.4f, relError %.4f, n in %d..%d): %d + %d samples, %8.2f + %8.2f = %8.2f ms, RMSE %.5f"
                         % (what, n_p, floor, rel, int(amap.min()), int(amap.max()), n_p * n_p * w * h, total_a, t_p, t_a, t_p + t_a, rmse_a))
            lines.append("  RMSE ratio adaptive / uniform %.3f at time ratio %.3f" % (rmse_a / rmse_u, (t_p + t_a) / t_u))
            print("\n".join(lines[-2:]), flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
