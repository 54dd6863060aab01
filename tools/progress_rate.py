"""usage (GPU box): python tools/progress_rate.py [out.txt] [--frames cornell,sponza,measured] [--reps 3] -- what rendering a frame in
stages (wpt_progress_*, DeviceScene.progressive) costs against the one-shot launch.  The Cornell frame, the Sponza-class frame
and the measured-BRDF frame of bench.py, each as one wpt_render_block_device launch and as a session of 1, 2, 4 and samples_sqrt
stages of equal rows; the forms alternate within a repeat, one untimed one-shot run first, median and spread (max - min) /
median over the repeats.  A stage costs its launch's end (lanes run out of pixels one by one), 32 bytes of carry per pixel each
way, the order kernels, and for the scene in LDS the twin that hands pixels out in slices, which a session never takes; the time
of a session is the sum over its stages, measured with events around all of them on one stream (wpt_progress_begin, which
allocates and clears 40 bytes per pixel, is timed on its own by the host's clock).  One preview is timed after the last stage."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from wurblpt_amd import device

FRAMES = {"cornell": "cornell_1024x1024_1024spp_ggx_glass", "sponza": "sponza_like_1920x1080_256spp_envmap_is",
          "measured": "measured_like_3840x2160_529spp_rgl"}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def plan(samples_sqrt, stages):
    """rows of each of `stages` stages, as equal as they come"""
    return [samples_sqrt // stages + (1 if k < samples_sqrt % stages else 0) for k in range(stages)]


def main():
    argv = sys.argv[1:]
    opts = {argv[i]: argv[i + 1] for i in range(len(argv) - 1) if argv[i].startswith("--")}
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or not argv[i - 1].startswith("--"))]
    out = args[0] if args else None
    reps = int(opts.get("--reps", 3))
    frames = opts.get("--frames", "cornell,sponza,measured").split(",")
    L = device.lib()
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/progress_rate.py: a frame as one launch and as a progressive session of k stages (ms, median of %d alternating repeats)" % reps,
             "# library %s" % bench.library_identity(),
             "# device %s, %d CUs" % (props.name, props.multi_processor_count),
             "# frame                                     form         ms   spread  / one-shot  all runs (ms)                  kernel, form of the last launch"]
    print("\n".join(lines), flush=True)
    stream = torch.cuda.current_stream()
    for key in frames:
        name = FRAMES[key]
        w = bench.WORKLOADS[name]
        sc = bench.build_scene(w)
        ds = device.DeviceScene(sc)
        W, H, S = w["width"], w["height"], w["samples_sqrt"]
        frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        forms = [("one-shot", None)] + [("%d stage%s" % (k, "" if k == 1 else "s"), plan(S, k)) for k in sorted({1, 2, 4, S})]
        times = {label: [] for label, _ in forms}
        described = {}
        begin_ms, preview_ms = [], []
        ds.render_block_into(frame, S, stream=stream)
        torch.cuda.synchronize()
        want = frame.clone()
        for rep in range(reps):
            for label, rows in forms:
                if rows is None:
                    times[label].append(timed(lambda: ds.render_block_into(frame, S, stream=stream)))
                else:
                    t0 = time.perf_counter()
                    session = ds.progressive(S, tag=0)
                    begin_ms.append((time.perf_counter() - t0) * 1e3)
                    frame.zero_()

                    def stages():
                        for r in rows:
                            session.advance(r, frame, stream)
                    times[label].append(timed(stages))
                    assert torch.equal(frame.view(torch.int32), want.view(torch.int32)), "the staged frame differs from the one-shot frame"
                    if rep == 0 and len(rows) == 2:
                        preview = torch.empty_like(frame)
                        preview_ms.append(timed(lambda: session.preview(preview, stream)))
                    session.close()
                described[label] = "%s%s" % (L.wpt_kernel_name().decode(), (", " + L.wpt_kernel_form().decode()) if L.wpt_kernel_form() else "")
                ds.check()
        base = float(np.median(times["one-shot"]))
        for label, _ in forms:
            t = times[label]
            ms = float(np.median(t))
            lines.append("%-42s %-9s %9.2f  %5.2f %%  %9.4f  %-30s %s" % (name, label, ms, 100.0 * (max(t) - min(t)) / ms, ms / base,
                                                                         " ".join("%.2f" % x for x in t), described[label]))
            print(lines[-1], flush=True)
        lines.append("%-42s one preview call %.3f ms; wpt_progress_begin (40 bytes per pixel allocated and cleared) %.2f ms by the host's clock, median of %d"
                     % (name, preview_ms[0], float(np.median(begin_ms)), len(begin_ms)))
        print(lines[-1], flush=True)
        ds.close()
        del ds, sc, frame, want
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
