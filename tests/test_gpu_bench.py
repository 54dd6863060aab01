"""bench.py as a program, N = 1: a plain run prints the headline line and measures nothing else; --full adds the counted pass
and roofline, the CPU baseline and the parity of a block; both write the same frames with --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD = "cornell_256x256_64spp_lambertian"


def _line(*args, workload=WORKLOAD):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload, "--steps", "2", "--warmup", "1"] + list(args)
    r = subprocess.run(cmd, capture_output=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout.decode()[-2000:] + r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    return json.loads(lines[0])


def _same_dumps(a, b, names):
    assert sorted(os.listdir(str(a))) == sorted(os.listdir(str(b))) == sorted(n + ".npy" for n in names)
    for n in names:
        x, y = np.load(str(a / (n + ".npy"))), np.load(str(b / (n + ".npy")))
        assert x.dtype == np.float32 and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), n


def test_plain_line_is_the_headline_figure_and_full_adds_the_checks(tmp_path):
    plain = _line("--dump-outputs", str(tmp_path / "plain"))
    assert plain["metric"] == "Msamples/s" and plain["unit"] == "Msamples/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["frame_finite"] is True and plain["ms_per_step"] > 0
    assert abs(plain["value"] - 256 * 256 * 64 / (plain["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * plain["value"]
    assert not {"roofline", "cpu_baseline", "parity", "secondary"} & set(plain)
    full = _line("--full", "--cpu-seconds", "1", "--dump-outputs", str(tmp_path / "full"))
    assert full["roofline"]["bound"] in ("valu", "hbm") and full["roofline"]["per_sample"]["rays"] > 0
    assert full["cpu_baseline"]["kind"] == "port" and full["parity"]["bits_differ"] == 0 and full["parity"]["pixels"] > 0
    assert "secondary" not in full      # the secondary workloads go with the default workload only
    _same_dumps(tmp_path / "plain", tmp_path / "full", [WORKLOAD])
    assert np.load(str(tmp_path / "plain" / (WORKLOAD + ".npy"))).shape == (256, 256, 3)


def test_plain_run_dumps_the_secondary_frames_the_full_line_dumps(tmp_path):
    # the default workload with the Sponza-class secondary alone (the other two take minutes): a plain run renders its frame
    # once, untimed, and writes the same bits as the last timed step of the --full line
    primary = "cornell_1024x1024_1024spp_ggx_glass"
    args = ["--skip-secondary", "courtyard_like_10M_1920x1080_121spp", "--skip-secondary", "measured_like_3840x2160_529spp_rgl"]
    plain = _line(*args, "--dump-outputs", str(tmp_path / "plain"), workload=primary)
    assert "secondary" not in plain
    full = _line(*args, "--full", "--cpu-seconds", "1", "--secondary-steps", "1", "--dump-outputs", str(tmp_path / "full"), workload=primary)
    assert [s["workload"] for s in full["secondary"]] == [bench.SECONDARY]
    _same_dumps(tmp_path / "plain", tmp_path / "full", [primary, bench.SECONDARY])

