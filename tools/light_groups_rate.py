"""usage (GPU box): python tools/light_groups_rate.py [out.txt] -- cost of light groups (DeviceScene.render_light_groups,
wpt_render_light_groups_block_device): Msamples/s of the plain render against one light-groups render with K = 1 / 4 / 16 groups,
and against K plain renders of the muted twins (the only way to the groups' frames without the sensor).  The K twin renders are
not all run: one twin is timed and its time is scaled by K (every twin render is a plain render of the same paths).
Workloads: host.light_groups_scene variant 0 at 1024^2 and 64 spp (scene in LDS; its two lamps in the first and the last group),
and the Sponza-class frame (1920x1080, 16 spp) with grouped lamps: its ModPhong surfaces are given an emission, which changes no
path, and are dealt to the groups in turn, the environment to group 0.  Each figure is the median of REPS runs; the spread is
(max - min) / median of those runs."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import _abi, device, host

REPS = 5


def timed(fn, reps=REPS):
    """(median milliseconds, spread in percent) of `reps` runs of fn() on the current stream, after one untimed run"""
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
    med = float(np.median(times))
    return med, 100.0 * (max(times) - min(times)) / med


def box():
    return host.light_groups_scene(1024, 1024, 0)


def sponza_with_lamps():
    sc = host.sponza_like(1920, 1080)
    d = sc.d
    glow = [(0.9, 0.6, 0.3), (0.3, 0.5, 0.9), (0.6, 0.9, 0.4)]
    n = 0
    for i in range(d.material_count):
        m = d.materials[i]
        if m.type == _abi.MAT_MODPHONG and m.tex[4] < 0:
            for c in range(3):
                m.v[3][c] = glow[n % 3][c]
            m.v[3][3] = sum(glow[n % 3]) / 3.0
            n += 1
    assert n > 0, "the Sponza-class scene has no ModPhong surface to light"
    return sc


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    lines = ["# tools/light_groups_rate.py: light groups against the plain render and against K plain renders of the muted twins (median of %d; spread = (max - min) / median)" % REPS,
             "# library %s" % bench.library_identity(),
             "# 'K twins' = the measured time of one plain render of a muted twin x K",
             "# workload                       emitters   K    plain ms (spread)  groups ms (spread)  x plain  K twins ms  twins/groups  Msamples/s (groups)  kernel"]
    print("\n".join(lines), flush=True)
    for label, make, S in (("light_groups_0_1024_64spp", box, 8), ("sponza_like_lamps_1920x1080_16spp", sponza_with_lamps, 4)):
        sc = make()
        w, h = sc.width, sc.height
        em = host.emitters(sc)
        has_env = sc.d.envmap.type != 0
        ds = device.DeviceScene(sc)
        stream = torch.cuda.current_stream()
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        plain_ms, plain_spread = timed(lambda: ds.render_block_into(frame, S, stream=stream))
        plain_kernel = device.lib().wpt_kernel_name().decode()
        tw = make()
        host.mute_emitters(tw, em[:1])
        dt = device.DeviceScene(tw)
        twin_ms, _ = timed(lambda: dt.render_block_into(frame, S, stream=stream))
        dt.close()
        samples = w * h * S * S
        lines.append("%-32s  %8d  %3s  %9.2f (%4.2f %%)  %18s  %7s  %10s  %12s  %19.1f  %s" % (
            label, len(em) + has_env, "-", plain_ms, plain_spread, "-", "-", "-", "-", samples / plain_ms / 1e3, plain_kernel))
        print(lines[-1], flush=True)
        for K in (1, 4, 16):
            table = np.full(sc.d.material_count, _abi.LIGHT_GROUP_NONE, np.uint8)
            for n, e in enumerate(em):
                table[e] = (n * (K - 1) // max(1, len(em) - 1)) if len(em) <= K else n % K
            planes = torch.zeros((K, h, w, 3), dtype=torch.float32, device="cuda")
            g_ms, g_spread = timed(lambda: ds.render_light_groups_into(frame, planes, S, table, K, 0 if has_env else _abi.LIGHT_GROUP_NONE,
                                                                      stream=stream))
            ds.check()
            lines.append("%-32s  %8d  %3d  %9.2f (%4.2f %%)  %9.2f (%4.2f %%)  %7.3f  %10.1f  %12.2f  %19.1f  %s" % (
                label, len(em) + has_env, K, plain_ms, plain_spread, g_ms, g_spread, g_ms / plain_ms, twin_ms * K, twin_ms * K / g_ms,
                samples / g_ms / 1e3, device.lib().wpt_kernel_name().decode()))
            print(lines[-1], flush=True)
            del planes
            torch.cuda.empty_cache()
        ds.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
