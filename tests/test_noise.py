"""Seeded per-scenario noise on the host (cmpc_noise_*_host, include/cmpc.h,
DESIGN.md §3.17) against tests/noise_ref.py: the Philox known answers, the
uniforms bit for bit, every refusal, invariance under a split of the batch,
the element update bit for bit from the host's own normals, the normals
against a long-double model, and the moments of a long draw.  No device.
"""
import ctypes

import numpy as np
import pytest

import cmpc
import golden_cases as GC
import noise_ref as R
from cmpc._abi import CmpcNoiseKey, load_library

SEED = 20261020
STEP_EDGES = (0, 1, 2 ** 32 - 1)

# The host normals' largest distance from the long-double model in units of
# eps r (r = sqrt(-2 ln u1)), measured on seed 20261020, step 3, B = 4096,
# n = 5: 1.15 (a plain float64 numpy evaluation that forms cos(2 pi u2): 3.08).
# Rounded up, the host bound.
HOST_UNITS_MEASURED = 1.15
HOST_UNITS_BOUND = 2.0


def test_philox_known_answers_in_the_model():
    for ctr, key, out in R.KNOWN_ANSWERS:
        assert R.philox4x32_10(ctr, key) == out


@pytest.mark.parametrize("k", range(len(R.KNOWN_ANSWERS)))
def test_known_answers_through_the_library(k):
    """The counter is (scenario0 + b, step, pair, stream) and the key (seed
    low, seed high), so each known answer is one call with B = 1; k1 and k2
    hold the top 27 and 26 bits of the words."""
    ctr, key, out = R.KNOWN_ANSWERS[k]
    if ctr[2] > 64:
        # a pair word the ABI reaches only with n = 2 * word + 1 channels (tens
        # of gigabytes of uniforms): the answer is checked in the model, and the
        # library against the model at pair 0 with the other five words kept
        assert R.philox4x32_10(ctr, key) == out
        ctr = (ctr[0], ctr[1], 0, ctr[3])
        out = R.philox4x32_10(ctr, key)
    n = 2 * ctr[2] + 1                      # the last channel's pair index is the counter word
    seed = key[0] | (key[1] << 32)
    lib = load_library()
    kk = CmpcNoiseKey(seed, ctr[3], ctr[0])
    u = np.zeros(((n + 1) // 2, 2))
    # (one scenario, read the last pair)
    assert lib.cmpc_noise_uniforms_host(ctypes.byref(kk), ctr[1], 1, n, u.ctypes.data_as(
        ctypes.POINTER(ctypes.c_double))) == 0, lib.cmpc_last_error()
    k1 = int(u[-1, 0] * 2.0 ** 53) - 1
    k2 = int(u[-1, 1] * 2.0 ** 53)
    assert (k1 >> 26, k1 & (2 ** 26 - 1)) == (out[0] >> 5, out[1] >> 6)
    assert (k2 >> 26, k2 & (2 ** 26 - 1)) == (out[2] >> 5, out[3] >> 6)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
@pytest.mark.parametrize("step", STEP_EDGES)
def test_uniforms_match_the_model(n, step):
    B = 9
    for scenario0 in (0, 2 ** 32 - B):
        for stream in (0, 1, 77):
            u = cmpc.noise_uniforms_host(SEED, step, B, n, stream=stream, scenario0=scenario0)
            ref = R.uniforms(SEED, step, B, n, stream=stream, scenario0=scenario0)
            assert u.shape == (B, (n + 1) // 2, 2)
            assert np.array_equal(R.bits(u), R.bits(ref)), (n, step, scenario0, stream)
            assert (u[:, :, 0] > 0).all() and (u[:, :, 0] <= 1).all()
            assert (u[:, :, 1] >= 0).all() and (u[:, :, 1] < 1).all()
    # a seed with a high word
    big = (0xDEADBEEF << 32) | 0x12345678
    assert np.array_equal(R.bits(cmpc.noise_uniforms_host(big, step, 3, n)), R.bits(R.uniforms(big, step, 3, n)))


def test_refusals():
    lib = load_library()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    key = CmpcNoiseKey(SEED, 0, 0)
    out, w, rho = np.zeros(8), np.zeros(8), np.zeros(8)

    def refused(rc, match):
        assert rc == -1
        assert match in lib.cmpc_last_error().decode(), lib.cmpc_last_error()

    refused(lib.cmpc_noise_check(None, 0, 2, 4), "null key")
    refused(lib.cmpc_noise_step_host(None, 0, 2, 4, None, None, None, None, dp(out)), "null key")
    refused(lib.cmpc_noise_step_host(ctypes.byref(key), 0, 2, 4, None, None, None, None, None), "null out")
    refused(lib.cmpc_noise_uniforms_host(ctypes.byref(key), 0, 2, 4, None), "null u")
    refused(lib.cmpc_noise_check(ctypes.byref(key), 0, 0, 4), "B must be >= 1")
    refused(lib.cmpc_noise_check(ctypes.byref(key), 0, 2, 0), "n must be >= 1")
    refused(lib.cmpc_noise_check(ctypes.byref(key), 2 ** 32, 2, 4), "step")
    assert lib.cmpc_noise_check(ctypes.byref(key), 2 ** 32 - 1, 2, 4) == 0
    edge = CmpcNoiseKey(SEED, 0, 2 ** 32 - 2)
    assert lib.cmpc_noise_check(ctypes.byref(edge), 0, 2, 4) == 0
    refused(lib.cmpc_noise_check(ctypes.byref(edge), 0, 3, 4), "scenario0 + B")
    refused(lib.cmpc_noise_step_host(ctypes.byref(edge), 0, 3, 2, None, None, None, None, dp(out)), "scenario0 + B")
    refused(lib.cmpc_noise_step_host(ctypes.byref(key), 0, 2, 4, None, dp(rho), None, None, dp(out)), "rho needs")
    assert lib.cmpc_noise_step_host(ctypes.byref(key), 0, 2, 4, None, dp(rho), dp(w), None, dp(out)) == 0
    # the device entry points refuse the same before they touch a device
    refused(lib.cmpc_noise_step(0, None, None, 0, 2, 4, None, None, None, None, None), "null key")
    refused(lib.cmpc_noise_step(0, None, ctypes.byref(key), 0, 2, 4, None, None, None, None, None), "null out")
    refused(lib.cmpc_noise_step(0, None, ctypes.byref(key), 2 ** 32, 2, 4, None, None, None, None,
                                ctypes.c_void_p(8)), "step")
    refused(lib.cmpc_noise_step(0, None, ctypes.byref(key), 0, 2, 4, None, ctypes.c_void_p(8), None, None,
                                ctypes.c_void_p(8)), "rho needs")
    refused(lib.cmpc_noise_uniforms(0, None, ctypes.byref(key), 0, 0, 4, ctypes.c_void_p(8)), "B must be >= 1")
    refused(lib.cmpc_noise_uniforms(0, None, ctypes.byref(key), 0, 2, 4, None), "null u")
    # the Python layer's own range checks
    with pytest.raises(ValueError, match="seed"):
        cmpc.noise_key(2 ** 64)
    with pytest.raises(ValueError, match="scenario0"):
        cmpc.noise_key(1, 0, 2 ** 32)
    with pytest.raises(RuntimeError, match="step"):
        cmpc.noise_uniforms_host(SEED, 2 ** 32, 2, 4)


def test_check_params():
    cmpc.noise_check_params(3, 2, None, None)
    sg, rh = cmpc.noise_check_params(3, 2, [0.0, 1.5], [-1.0, 1.0])
    assert sg.shape == rh.shape == (3, 2)
    for bad in (-1e-300, np.inf, np.nan):
        s = np.ones((3, 2))
        s[2, 1] = bad
        with pytest.raises(RuntimeError, match="scenario 2, channel 1: sigma"):
            cmpc.noise_check_params(3, 2, s, None)
    for bad in (1.0000000000000002, -1.5, np.nan):
        r = np.zeros((3, 2))
        r[1, 0] = bad
        with pytest.raises(RuntimeError, match="scenario 1, channel 0: rho"):
            cmpc.noise_check_params(3, 2, None, r)
    with pytest.raises(ValueError, match="sigma must be"):
        cmpc.noise_check_params(3, 2, np.ones(3), None)


@pytest.mark.parametrize("n", [3, 4])
def test_split_invariance(n):
    """A batch of 70 is the batches of 33 and 37 at scenario0 0 and 33, bit for
    bit: the uniforms, and out and the AR(1) state over 5 steps."""
    rng = np.random.default_rng(5)
    sigma, rho = rng.uniform(0.1, 2.0, (70, n)), rng.uniform(-0.95, 0.95, (70, n))
    base = rng.normal(size=(70, n))
    w = [np.zeros((70, n)), np.zeros((33, n)), np.zeros((37, n))]
    for k in range(5):
        u = cmpc.noise_uniforms_host(SEED, k, 70, n, stream=1, scenario0=0)
        ua = cmpc.noise_uniforms_host(SEED, k, 33, n, stream=1, scenario0=0)
        ub = cmpc.noise_uniforms_host(SEED, k, 37, n, stream=1, scenario0=33)
        assert np.array_equal(R.bits(u), R.bits(np.concatenate([ua, ub])))
        o = cmpc.noise_step_host(SEED, k, 70, n, sigma, rho, w[0], base, stream=1, scenario0=0)
        oa = cmpc.noise_step_host(SEED, k, 33, n, sigma[:33], rho[:33], w[1], base[:33], stream=1, scenario0=0)
        ob = cmpc.noise_step_host(SEED, k, 37, n, sigma[33:], rho[33:], w[2], base[33:], stream=1,
                                  scenario0=33)
        assert np.array_equal(R.bits(o), R.bits(np.concatenate([oa, ob]))), k
        assert np.array_equal(R.bits(w[0]), R.bits(np.concatenate([w[1], w[2]]))), k
    assert np.abs(w[0]).min() > 0


@pytest.mark.parametrize("n", [1, 4, 5])
def test_element_update_from_the_hosts_own_normals(n):
    """Given the host's z (sigma, rho, base NULL), numpy reproduces w and out
    bit for bit, the d == 0 copy and rho = +-1 included."""
    B = 40
    rng = np.random.default_rng(7 + n)
    sigma = rng.uniform(0.0, 3.0, (B, n))
    sigma[::5] = 0.0                                   # d == 0: out is base, bit for bit
    rho = rng.uniform(-1.0, 1.0, (B, n))
    rho[1::7], rho[2::7] = 1.0, -1.0
    base = rng.normal(size=(B, n))
    base[::10] = -0.0
    w = rng.normal(size=(B, n))
    w[::5] = 0.0                                       # (with sigma 0: the AR(1)'s d == 0 too)
    w_lib = w.copy()
    for k in range(5):
        z = cmpc.noise_step_host(SEED, k, B, n, stream=3)
        # white
        o = cmpc.noise_step_host(SEED, k, B, n, sigma, None, None, base, stream=3)
        _, ref = R.step_model(z, sigma, None, None, base)
        assert np.array_equal(R.bits(o), R.bits(ref)), k
        assert np.array_equal(R.bits(o[::5]), R.bits(base[::5]))
        # AR(1)
        o = cmpc.noise_step_host(SEED, k, B, n, sigma, rho, w_lib, base, stream=3)
        w, ref = R.step_model(z, sigma, rho, w, base)
        assert np.array_equal(R.bits(w_lib), R.bits(w)), k
        assert np.array_equal(R.bits(o), R.bits(ref)), k
        assert np.array_equal(R.bits(o[::5]), R.bits(base[::5]))
        # no base: out is d (0 where d == 0)
        o = cmpc.noise_step_host(SEED, k, B, n, sigma, stream=3)
        assert np.array_equal(R.bits(o), R.bits(R.step_model(z, sigma)[1]))
    # rho = +-1 keeps |w|: g = 0
    assert np.array_equal(np.abs(w[1::7]), np.abs(w_lib[1::7]))


def test_normals_against_the_long_double_model():
    B, n, step = 4096, 5, 3
    u = cmpc.noise_uniforms_host(SEED, step, B, n)
    z_ld, r = R.normals_ld(u, n)
    z = cmpc.noise_step_host(SEED, step, B, n)
    plain = R.error_units(R.normals_f64(u, n), z_ld, r)
    host = R.error_units(z, z_ld, r)
    print(f"distance to the long-double model in eps r: host {host:.3f}, float64 model with cos(2 pi u2) {plain:.3f}")
    assert 3.0 < plain < 3.2          # (the yardstick's own scale: 3.08)
    assert host <= HOST_UNITS_BOUND, host
    # u1 = 1 gives r = 0 and both channels 0 exactly
    assert (z[r == 0] == 0).all()


def test_moments_and_independence():
    B, n, T = 4096, 4, 16
    Z = np.stack([cmpc.noise_step_host(SEED, k, B, n) for k in range(T)])              # (T, B, n)
    Z1 = np.stack([cmpc.noise_step_host(SEED, k, B, n, stream=1) for k in range(T)])
    N = Z.size
    stats = {"mean": Z.mean() * np.sqrt(N), "var": (Z.var() - 1.0) / np.sqrt(2.0 / N),
             "m4": ((Z ** 4).mean() - 3.0) / np.sqrt(96.0 / N)}
    lag = lambda a: a.mean() * np.sqrt(a.size)
    stats["lag step"] = lag(Z[1:] * Z[:-1])
    stats["lag scenario"] = lag(Z[:, 1:] * Z[:, :-1])
    for i, j in ((0, 1), (0, 2), (1, 2)):
        stats[f"channels {i}{j}"] = lag(Z[:, :, i] * Z[:, :, j])
    stats["streams 0 1"] = lag(Z * Z1)
    print({k: round(float(v), 3) for k, v in stats.items()}, "max |z|", float(np.abs(Z).max()))
    for k, v in stats.items():
        assert abs(v) <= 4.0, (k, v)
    assert np.isfinite(Z).all()


def test_host_arithmetic_under_sanitizers():
    """csrc/noise_body.h, the text the host entry points and the kernels share,
    in a stand-alone program under AddressSanitizer and
    UndefinedBehaviorSanitizer (tests/cpp/noise_body_asan.cpp): exact-size heap
    arrays, odd and even n, every optional array left out in turn."""
    import os
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    subprocess.check_call(["make", "-s", "-C", here, "-f", "noise_body_asan.mk", "noise_body_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "noise_body_asan")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("noise_body_asan ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]


# ---- score_ensemble on the host: the refusals and the layout helper ---------------------

def test_score_ensemble_refusals_and_layout():
    lib = load_library()
    out = np.zeros(4)
    assert lib.cmpc_score_ensemble(None, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert b"null argument" in lib.cmpc_last_error()
    cfg = GC.case("coop-par", p=50)[0]
    dims = cmpc.CmpcDims.from_config(cfg, 3)
    n, S = cmpc.score_len(dims), dims.S
    flat = np.arange(n * S * 6, dtype=np.float64)
    st = cmpc.score_ensemble_unpack(dims, flat)
    fields = cmpc.score_fields(dims)
    assert set(st) == set(fields)
    for name, sl in fields.items():
        assert set(st[name]) == {"mean", "std", "min", "max", "argmax", "count"}
        for k, stat in enumerate(("mean", "std", "min", "max", "argmax", "count")):
            a = st[name][stat]
            assert a.shape == (S, sl.stop - sl.start)
            assert a.dtype == (np.int64 if stat in ("argmax", "count") else np.float64)
            for s in range(S):
                for i, f in enumerate(range(sl.start, sl.stop)):
                    assert a[s, i] == (f * S + s) * 6 + k
    with pytest.raises(ValueError, match="expected"):
        cmpc.score_ensemble_unpack(dims, flat[:-1])
