"""The device's wptm::sincosf_ (one reduction, both polynomials, selects) and the select form of the sampler's inUnitDisk, through
the probes 13 .. 16 of wpt_selftest_kernel, against the oracle's sinf_ / cosf_ -- which do not go through sincosf_ -- bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1 << 20
K_PI_2 = np.float32(1.5707963267948966)
K_PI_4 = np.float32(0.7853981633974483)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from wurblpt_amd import device
    assert device.device_count() >= 1
    return device


def sincos_arguments():
    """2^20 arguments: every float within 2^12 ulps of +-2^-12, +-pi/4, +-120, +-pi/2, +-3pi/4, +-2pi (the borders of sincosf_'s
    size classes and of the quadrants), +-0, denormals, +-inf, NaNs, and a fixed-seed spread of random bit patterns."""
    parts = []
    for centre in (2.0 ** -12, np.pi / 4, 120.0, np.pi / 2, 3 * np.pi / 4, 2 * np.pi):
        bits = np.float32(centre).view(np.uint32).astype(np.int64) + np.arange(-(1 << 12), (1 << 12) + 1, dtype=np.int64)
        parts.append(bits.astype(np.uint32))
        parts.append((bits | 0x80000000).astype(np.uint32))
    special = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x00800000, 0x80800000]
    special += [1 << k for k in range(23)] + [0x80000000 | (1 << k) for k in range(23)]  # denormals of every magnitude
    special += [0x007fffff, 0x807fffff, 0x00000003, 0x80000003, 0x00400001, 0x80400001]
    parts.append(np.array(special, dtype=np.uint32))
    fixed = np.concatenate(parts)
    rng = np.random.RandomState(1314)
    spread = rng.randint(0, 1 << 32, N - fixed.size, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([fixed, spread]).view(np.float32)
    assert x.size == N
    return x


def assert_same_bits(got, ref, what):
    """Bit for bit wherever the expected value is a number.  Where it is NaN (sinf_ / cosf_ of an infinity or a NaN: (y - y) / (y - y))
    the result must be NaN: sign and payload of a NaN that an operation produces are the processor's (x86-64 makes the negative
    default NaN out of inf - inf, gfx950 the positive one), not the arithmetic under test."""
    g, r = got.view(np.uint32), ref.view(np.uint32)
    nan = np.isnan(ref)
    strict = int(np.count_nonzero(g != r))
    numbers = int(np.count_nonzero((g != r) & ~nan))
    nans = int(np.count_nonzero(nan & ~np.isnan(got)))
    print("%s: %d of %d differ in bits, %d of them where a number is expected; %d expected NaNs are not NaN" % (what, strict, g.size, numbers, nans))
    assert numbers == 0 and nans == 0, what


def test_sincos_pair_on_device_equals_oracle_sine_and_cosine(dev, oracle):
    x = sincos_arguments()
    assert_same_bits(dev.selftest_math(13, x), oracle.math(0, x), "sine of sincosf_")
    assert_same_bits(dev.selftest_math(14, x), oracle.math(1, x), "cosine of sincosf_")


def disk_arguments():
    """2^20 pairs in [0, 1)^2, as the generator makes them (multiples of 2^-24) and finer ones next to 0: u.x == 0.5, u.y == 0.5,
    both (the centre), |ox| == |oy| with either sign, values next to 0 and next to 1, and a fixed-seed spread."""
    rng = np.random.RandomState(1516)
    grid = lambda n: (rng.randint(0, 1 << 24, n).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    half = np.float32(0.5)
    edge = np.array([0.0, 2.0 ** -24, 2.0 ** -23, 3 * 2.0 ** -24, 1e-45, 1e-40, 1.17549435e-38, 1e-30, 2.0 ** -25,
                     1 - 2.0 ** -24, 1 - 2.0 ** -23, 1 - 3 * 2.0 ** -24, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, 0.5 - 2.0 ** -24, 0.5, 0.25, 0.75],
                    dtype=np.float32)
    ex, ey = np.meshgrid(edge, edge)
    n = 1 << 12
    a = grid(n)
    ux = [ex.ravel(), np.full(n, half), grid(n), np.full(1, half), a, a, np.repeat(edge, n // 16), grid(edge.size * (n // 16))]
    uy = [ey.ravel(), grid(n), np.full(n, half), np.full(1, half), a, (np.float32(1.0) - a).astype(np.float32), grid(edge.size * (n // 16)), np.repeat(edge, n // 16)]
    ux, uy = np.concatenate(ux).astype(np.float32), np.concatenate(uy).astype(np.float32)
    keep = (ux < 1.0) & (uy < 1.0)  # 1 - 0 is not in [0, 1)
    ux, uy = ux[keep], uy[keep]
    rest = N - ux.size
    ux, uy = np.concatenate([ux, grid(rest)]), np.concatenate([uy, grid(rest)])
    assert ux.size == N and uy.size == N and ux.min() >= 0.0 and ux.max() < 1.0 and uy.min() >= 0.0 and uy.max() < 1.0
    return ux, uy


def disk_expected(oracle, ux, uy):
    """Sampler::inUnitDisk as the reference writes it, two arms, in IEEE float32 operations; sine and cosine from the oracle."""
    two, one = np.float32(2.0), np.float32(1.0)
    ox = (two * ux - one).astype(np.float32)
    oy = (two * uy - one).astype(np.float32)
    centre = (ox == 0.0) & (oy == 0.0)
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        theta_wide = (K_PI_4 * (oy / ox).astype(np.float32)).astype(np.float32)
        theta_tall = (K_PI_2 - (K_PI_4 * (ox / oy).astype(np.float32)).astype(np.float32)).astype(np.float32)
    theta = np.where(wide, theta_wide, theta_tall).astype(np.float32)
    theta[centre] = 0.0
    rad = np.where(wide, ox, oy).astype(np.float32)
    s, c = oracle.math(0, theta), oracle.math(1, theta)
    x = (rad * c).astype(np.float32)
    y = (rad * s).astype(np.float32)
    x[centre] = 0.0
    y[centre] = 0.0
    assert np.isfinite(x).all() and np.isfinite(y).all()
    assert centre.any() and (np.abs(ox) == np.abs(oy)).sum() > 4000 and wide.sum() > 1000 and (~wide).sum() > 1000
    return x, y


def test_disk_sample_on_device_equals_the_two_arm_sampler(dev, oracle):
    ux, uy = disk_arguments()
    x, y = disk_expected(oracle, ux, uy)
    assert_same_bits(dev.selftest_math(15, ux, uy), x, "x of inUnitDisk")
    assert_same_bits(dev.selftest_math(16, ux, uy), y, "y of inUnitDisk")
