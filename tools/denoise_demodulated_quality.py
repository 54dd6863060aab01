"""usage (GPU box): python tools/denoise_demodulated_quality.py [quality.txt] [--rate rate.txt] -- effect and cost of the first-hit
colour pass (DeviceScene.first_hit_colours_device) and of the denoiser on the demodulated frame (device.denoise_demodulated).

Effect: two textured scenes (the small Sponza-class scene of the tests: textured Lambertian and ModPhong walls under a sun and sky
environment; host.cornell_checker: the Cornell box whose walls carry checkers) and the untextured Cornell box, 64 x 64 at 16 spp
(render_adaptive, n = 4, with the moment film) against a converged render (2304 spp): relative L2 error sqrt(sum (f - ref)^2 / sum ref^2) of the noisy frame, of the frame filtered as radiance
(device.denoise) and of the frame filtered demodulated, all with the default parameters.  The result is recorded, not asserted
(profiles/denoise_demodulated_quality.txt): no test holds a bound on it.

Cost (--rate): the Cornell box at 1024^2 and 3840 x 2160; the colour pass with all five outputs beside ground_truth_device of the
three guide arrays, and denoise_demodulated beside denoise (16-spp frame, default parameters).  Every size is measured in a process
of its own; in it the four calls are timed in turn, REPEATS times over (A, B, C, D, A, ...), each timing the median of CALLS
timings between two events after three untimed calls; a figure's spread is (max - min) / median over the repeats."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
CALLS = 5
SIZES = ((1024, 1024), (3840, 2160))
SMALL_SPONZA = dict(detail=0.05, tex_size=32, env_width=64, importance_n=16)   # tests/test_gpu_first_hit_colours.py's


def errors(ds, size=64, nref=48):
    """relative L2 against nref^2 spp of the 16-spp frame: noisy, filtered, filtered demodulated"""
    import numpy as np
    import torch
    from wurblpt_amd import device
    m = np.full((size, size), 4, np.uint16)
    frame, moments = ds.render_adaptive(m, with_moments=True)
    colours = ds.first_hit_colours_device()
    plain = device.denoise(frame, moments, m, colours)
    demodulated = device.denoise_demodulated(frame, moments, m, colours)
    ref = np.asarray(ds.render(nref)[0]).reshape(size, size, 3).astype(np.float64)
    torch.cuda.synchronize()
    rel = lambda f: float(np.sqrt(((f.cpu().numpy().astype(np.float64) - ref) ** 2).sum() / (ref ** 2).sum()))
    return rel(frame), rel(plain), rel(demodulated)


def quality(path):
    from wurblpt_amd import device, host
    lines = ["# python tools/denoise_demodulated_quality.py: 64 x 64 at 16 spp against 2304 spp, default parameters, albedo floor 1/64;",
             "# relative L2 error sqrt(sum (f - ref)^2 / sum ref^2)",
             "# scene : noisy : filtered (denoise) : filtered demodulated (denoise_demodulated) : demodulated over filtered : demodulated over noisy"]
    for name, scene in (("sponza_like small (textured)", host.sponza_like(64, 64, **SMALL_SPONZA)),
                        ("cornell_checker (textured)", host.cornell_checker(64, 64)), ("cornell (untextured)", host.cornell(64, 64))):
        ds = device.DeviceScene(scene)
        noisy, plain, demodulated = errors(ds)
        ds.check()
        ds.close()
        lines.append("%s : %.5f : %.5f : %.5f : %.4f : %.4f" % (name, noisy, plain, demodulated, demodulated / plain, demodulated / noisy))
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def measure(width, height):
    import numpy as np
    import torch
    from wurblpt_amd import device, host
    ds = device.DeviceScene(host.cornell(width, height))
    m = torch.full((height, width), 4, dtype=torch.int16, device="cuda").view(torch.uint16)
    frame = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda")
    moments = torch.zeros_like(frame)
    ds.render_adaptive_into(frame, m, moments)
    colours = ds.first_hit_colours_device()
    inner = max(1, (1 << 24) // (width * height))

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
    calls = {"first_hit_colours": lambda: ds.first_hit_colours_device(), "ground_truth_guide": lambda: ds.ground_truth_device(),
             "denoise_demodulated": lambda: device.denoise_demodulated(frame, moments, m, colours), "denoise": lambda: device.denoise(frame, moments, m, colours)}
    result = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, fn in calls.items():
            result[k].append(timed(fn))
    ds.check()
    ds.close()
    return result


def rate(path):
    import numpy as np
    lines = ["# python tools/denoise_demodulated_quality.py --rate: Cornell, the four calls timed in turn, %d repeats, each the median of %d timings;"
             % (REPEATS, CALLS), "# ms per call (spread = (max - min) / median over the repeats); both first-hit calls allocate their outputs (torch.zeros) inside the timing",
             "# size : first_hit_colours_device, five outputs : ground_truth_device, three guide arrays : denoise_demodulated : denoise"]
    for w, h in SIZES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", str(w), str(h)], capture_output=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("measuring at %dx%d failed (%d):\n%s" % (w, h, r.returncode, r.stderr.decode()[-3000:]))
        res = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("RESULT ")][-1][7:])
        stat = lambda v: "%.3f (%.1f %%)" % (float(np.median(v)), 100.0 * (max(v) - min(v)) / float(np.median(v)))
        lines.append("%dx%d : %s : %s : %s : %s" % (w, h, stat(res["first_hit_colours"]), stat(res["ground_truth_guide"]),
                                                   stat(res["denoise_demodulated"]), stat(res["denoise"])))
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    args = sys.argv[1:]
    if args[:1] == ["--measure"]:
        print("RESULT " + json.dumps(measure(int(args[1]), int(args[2]))))
        return
    while args:
        a = args.pop(0)
        if a == "--rate":
            rate(args.pop(0))
        else:
            quality(a)


if __name__ == "__main__":
    main()
