"""usage (GPU box): python tools/denoise_rate.py [--libs lib,lib_x,...] [--quality quality.txt] [out.txt] -- cost and effect of the
denoiser (device.denoise, wpt_postproc_denoise).

Cost: the Cornell box at 1024^2 and 3840x2160, rendered at 16 spp through the adaptive entry point with its moment film, the three
guide arrays of the first-hit pass, then the filter with 0 .. 8 iterations.  Milliseconds per call are the median of CALLS timings
between two events (after three untimed calls; 16 calls back to back per timing at 1024^2, 2 at 3840x2160); the iteration with step 2^k costs what a call with k + 1 iterations takes more than one with k; a call with
no iteration is the pack and the unpack.  Achieved bytes/s are set against the compulsory traffic of an iteration, computed from
the frame's shape: every pixel's three 16-byte records read once (48 B) and one written (16 B); the nine variance taps of the
neighbourhood mean re-read records that the 25 taps read anyway, and count 9 * 4 B more in the second figure.
--libs names builds of the libraries under wurblpt_amd/ (WPT_LIB_DIR), e.g. one made with
  make -C wurblpt_amd/csrc BUILD=build_gather LIB=../lib_gather EXTRA=-DWPT_DENOISE_LDS_MAX_STEP=0
so that a step's tile form (a workgroup's pixels and halo in LDS) stands beside its gather form: every build is measured in a
process of its own, REPEATS times in turn (build A, build B, ..., build A, ...), and a figure's spread is (max - min) / median
over those repeats.

Effect (--quality): Cornell at 64^2 and 256^2, 16 spp, relative L2 error against a converged render (2304 / 1024 spp) of the noisy
and of the filtered frame for the default parameters and for the published sigma_l = 4, and where the filtered frame's error
lies."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
CALLS = 5
SIZES = ((1024, 1024), (3840, 2160))


def measure(width, height):
    """one build, one size: ms of the render, the first-hit pass and the filter with 0 .. 8 iterations"""
    import numpy as np
    import torch
    from wurblpt_amd import _abi, device, host
    ds = device.DeviceScene(host.cornell(width, height))
    m = torch.full((height, width), 4, dtype=torch.int16, device="cuda").view(torch.uint16)
    frame = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros_like(frame)

    inner = max(1, (1 << 24) // (width * height))  # calls between a pair of events: short calls are timed back to back

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / inner)
        return float(np.median(times))
    result = {"render": timed(lambda: ds.render_adaptive_into(frame, m, moments))}
    guide = ds.ground_truth_device()
    result["guide"] = timed(lambda: ds.ground_truth_device())
    result["calls"] = [timed(lambda: device.denoise(frame, moments, m, guide, _abi.DenoiseParams(iterations=k))) for k in range(9)]
    result["forms"] = [device.denoise_form(1 << k) for k in range(8)]
    ds.check()
    ds.close()
    return result


def quality(path):
    import numpy as np
    import torch
    from wurblpt_amd import _abi, device, host
    lines = ["# python tools/denoise_rate.py --quality: Cornell at 16 spp (render_adaptive, n = 4, with the moment film), guided by the first-hit",
             "# pass and filtered on the device; relative L2 error sqrt(sum (f - ref)^2 / sum ref^2) against the converged render",
             "# size : converged spp : noisy : filtered with the defaults (sigma_l %g, sigma_z %g, normal_log2 %d, iterations %d) : ratio : filtered with sigma_l = 4 : ratio"
             % (_abi.DenoiseParams().sigma_l, _abi.DenoiseParams().sigma_z, _abi.DenoiseParams().normal_log2, _abi.DenoiseParams().iterations)]
    for size, nref in ((64, 48), (256, 32)):
        ds = device.DeviceScene(host.cornell(size, size))
        m = np.full((size, size), 4, np.uint16)
        frame, moments = ds.render_adaptive(m, with_moments=True)
        guide = ds.ground_truth_device()
        ref = np.asarray(ds.render(nref)[0]).reshape(size, size, 3).astype(np.float64)
        err2 = lambda f: ((f.cpu().numpy().astype(np.float64) - ref) ** 2).sum(axis=2)
        rel = lambda f: float(np.sqrt(err2(f).sum() / (ref ** 2).sum()))
        ours = device.denoise(frame, moments, m, guide)
        published = device.denoise(frame, moments, m, guide, _abi.DenoiseParams(sigma_l=4.0))
        torch.cuda.synchronize()
        lines.append("%dx%d : %d : %.5f : %.5f : %.4f : %.5f : %.4f" % (size, size, nref * nref, rel(frame), rel(ours), rel(ours) / rel(frame),
                                                                         rel(published), rel(published) / rel(frame)))
        # where the error lies: the pixels beside the lamp, whose footprint holds a part of it while the ray through their centre
        # (the guide's) hits the ceiling
        mat = guide["materials"].cpu().numpy().reshape(size, size)
        lamp = mat == mat[np.unravel_index(np.argmax(ref.sum(axis=2)), mat.shape)]
        near = np.zeros_like(lamp)
        ys, xs = np.where(lamp)
        near[max(ys.min() - 2, 0):ys.max() + 3, max(xs.min() - 2, 0):xs.max() + 3] = True
        near &= ~lamp
        for name, f in (("noisy", frame), ("defaults", ours), ("sigma_l = 4", published)):
            e = err2(f)
            lines.append("#   %s: %.1f %% of the squared error in the %d pixels within 2 of the lamp, %.1f %% in its own %d"
                         % (name, 100 * e[near].sum() / e.sum(), near.sum(), 100 * e[lamp].sum() / e.sum(), lamp.sum()))
        ds.close()
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    args = sys.argv[1:]
    if args[:1] == ["--measure"]:
        print("RESULT " + json.dumps(measure(int(args[1]), int(args[2]))))
        return
    libs, out = ["lib"], None
    while args:
        a = args.pop(0)
        if a == "--libs":
            libs = args.pop(0).split(",")
        elif a == "--quality":
            quality(args.pop(0))
        else:
            out = a
    if out is None:
        return
    import numpy as np
    runs = {}
    for _ in range(REPEATS):
        for lib in libs:
            for w, h in SIZES:
                env = dict(os.environ, WPT_LIB_DIR=lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", str(w), str(h)], env=env, capture_output=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("measuring %s at %dx%d failed (%d):\n%s" % (lib, w, h, r.returncode, r.stderr.decode()[-3000:]))
                line = [l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1]
                runs.setdefault((lib, w, h), []).append(json.loads(line[7:]))

    def stat(values):
        med = float(np.median(values))
        return med, 100.0 * (max(values) - min(values)) / med if med > 0 else 0.0
    lines = ["# python tools/denoise_rate.py --libs %s: Cornell at 16 spp, %d alternating repeats per build, each the median of %d timings; spread = (max - min) / median over the repeats"
             % (",".join(libs), REPEATS, CALLS),
             "# compulsory traffic of an iteration: width * height * 64 B (48 B read, 16 B written); with the nine variance taps: * 100 B"]
    for w, h in SIZES:
        for lib in libs:
            rs = runs[(lib, w, h)]
            lines.append("%dx%d, build %s, forms of the steps 1 .. 128: %s" % (w, h, lib, " ".join(rs[0]["forms"])))
            lines.append("  render at 16 spp %.3f ms (spread %.1f %%), first-hit pass %.3f ms (%.1f %%)" % (stat([r["render"] for r in rs]) + stat([r["guide"] for r in rs])))
            for k in range(9):
                lines.append("  call with %d iterations: %.3f ms (spread %.1f %%)" % ((k,) + stat([r["calls"][k] for r in rs])))
            for k in range(8):
                ms, spread = stat([r["calls"][k + 1] - r["calls"][k] for r in rs])
                lines.append("  iteration with step %3d (%s): %.3f ms (spread %.1f %%), %.0f GB/s of compulsory traffic, %.0f GB/s with the variance taps"
                             % (1 << k, rs[0]["forms"][k], ms, spread, w * h * 64 / ms / 1e6, w * h * 100 / ms / 1e6))
            d, _ = stat([r["calls"][_default_iterations()] for r in rs])
            rr, _ = stat([r["render"] for r in rs])
            lines.append("  the default call (%d iterations) takes %.3f ms beside the %.3f ms of the 16-spp render it follows: %.1f %%"
                         % (_default_iterations(), d, rr, 100 * d / rr))
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def _default_iterations():
    from wurblpt_amd import _abi
    return _abi.DenoiseParams().iterations


if __name__ == "__main__":
    main()
