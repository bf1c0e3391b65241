"""The host half of the start in front of EM without a GPU (csrc/ref_rand.cpp, csrc/kmeans_plan.cpp, csrc/kmeans_host.cpp):
tests/host/kmeans_checks.cpp, a stand-alone program (host code only, nothing loaded into Python), built once under AddressSanitizer +
UBSan and once under ThreadSanitizer.  Its driver run on a plain-loop back end must reproduce the means the DEVICE recorded into
tests/golden/kmeans_parent_bits.npz bit for bit: the arithmetic that feeds every decision is correctly rounded IEEE in a fixed order
on both sides."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kmeans_parent_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speaker-recognition_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host", "kmeans_checks.cpp")] + [os.path.join(CSRC, f) for f in ("ref_rand.cpp", "kmeans_plan.cpp",
                                                                                                         "kmeans_host.cpp")]
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(path, sanitize):
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=" + sanitize, "-ffp-contract=off", "-pthread", "-I", CSRC]
    if "undefined" in sanitize:
        cmd.append("-fno-sanitize-recover=undefined")
    if sanitize == "thread":
        cmd.append("-no-pie")           # (a position-independent program can land where ThreadSanitizer's shadow map does not reach)
    b = subprocess.run(cmd + SOURCES + ["-o", path], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    return path


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(r.stdout)
    assert r.returncode == 0 and "kmeans checks ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.fixture(scope="module")
def checks(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("kmeans_checks") / "kmeans_checks"), "address,undefined")


@pytest.fixture(scope="module")
def host_means(checks, tmp_path_factory):
    """-> {name: (means [K][D], sigma [D]) or the refusal} of the host cases, from one run of the program's drivers"""
    d = tmp_path_factory.mktemp("kmeans_driver")
    lines = []
    for name in pc.HOST_NAMES:
        _name, n, K, D, conc, seed, km, _eng, _kind = pc.BY_NAME[name]
        path = str(d / (name + ".f32"))
        pc.frames(pc.BY_NAME[name]).tofile(path)
        lines.append("%s %d %d %d %d %d %d %s" % (name, n, K, D, conc, seed, km, path))
    manifest = str(d / "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    _run(checks, "driver", manifest, str(d))
    out = {}
    for name in pc.HOST_NAMES:
        K, D = pc.BY_NAME[name][2:4]
        if os.path.exists(str(d / (name + ".error"))):
            out[name] = open(str(d / (name + ".error"))).read()
        else:
            v = np.fromfile(str(d / (name + ".means")), dtype=np.float64)
            assert v.size == K * D + D
            out[name] = (v[:K * D].reshape(K, D), v[K * D:])
    return out


def test_plans_and_stream_under_asan_ubsan(checks):
    _run(checks, "plans")


@pytest.mark.parametrize("name", pc.HOST_NAMES)
def test_host_driver_has_the_devices_recorded_bits(host_means, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "kmeans_parent_bits.npz"))
    got = host_means[name]
    if name + "/error" in g.files:
        assert isinstance(got, str) and got in str(g[name + "/error"]), (got, str(g[name + "/error"]))
        return
    assert not isinstance(got, str), got
    K = pc.BY_NAME[name][2]
    assert np.array_equal(got[0], g[name + "/means"]), (name, np.max(np.abs(got[0] - g[name + "/means"])))
    assert np.array_equal(np.tile(got[1], (K, 1)), g[name + "/sigmas"])


@pytest.mark.parametrize("name", ["k17", "conc37_n3001"])
def test_host_driver_equals_the_numpy_restatement(host_means, name):
    from oracle import init_oracle as io
    _name, _n, K, _D, conc, seed, km, _eng, _kind = pc.BY_NAME[name]
    X = pc.frames(pc.BY_NAME[name])
    _w0, mu0, sg0 = io.init_gaussians(X.astype(np.float64), K, km, conc, io.GlibcRand(seed + 1))
    mu, sg = host_means[name]
    assert np.max(np.abs(mu - mu0)) < 1e-9 * max(1.0, np.max(np.abs(mu0))), np.max(np.abs(mu - mu0))
    assert np.max(np.abs(np.tile(sg, (K, 1)) - sg0) / sg0) < 1e-12


def test_threaded_stages_under_tsan(tmp_path):
    _run(_build(str(tmp_path / "kmeans_checks_tsan"), "thread"), "threads")
