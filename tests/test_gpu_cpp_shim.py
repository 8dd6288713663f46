"""Runs the C++ program that drives the hot path through the C++17 shim (include/dfx_shim.hpp), i.e. the way the
reference's CameraTracker / PhotometricFactor would call it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(exe, verdict, timeout=120):
    """Runs a C++ test program.  The programs flush their verdict line before they exit: a process that has printed it and then does not come back within the
    timeout is stuck in the teardown of the GPU runtime (seen once in ~70 runs on a box where the pytest process holds a second GPU context) -- reported as a
    warning, not as a failure of the code under test; a process that hangs BEFORE its verdict fails the test."""
    import warnings
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=timeout, stdin=subprocess.DEVNULL)
    except subprocess.TimeoutExpired as e:
        so = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        assert verdict in so, f"{os.path.basename(exe)} hung before its verdict; output so far: {so[-2000:]}"
        warnings.warn(f"{os.path.basename(exe)} printed '{verdict}' and then did not exit within {timeout} s (GPU runtime teardown)")
        return so
    assert out.returncode == 0, out.stdout + out.stderr
    assert verdict in out.stdout
    return out.stdout


@pytest.mark.gpu
def test_cpp_shim_tracker():
    exe = os.path.join(ROOT, "tests", "cpp", "shim_test")
    assert os.path.exists(exe), "tests/cpp/shim_test not built: run __graft_entry__.build()"
    _run(exe, "shim_test OK")


@pytest.mark.gpu
def test_cpp_host_layer():
    """include/dfx_host.hpp (C++17 keyframe store + LinearizeAll over the C ABI): tests/cpp/host_test.cpp, compiled with plain g++."""
    exe = os.path.join(ROOT, "tests", "cpp", "host_test")
    assert os.path.exists(exe), "tests/cpp/host_test not built: run __graft_entry__.build()"
    _run(exe, "host_test OK")


@pytest.mark.gpu
def test_reference_callers_compiled_unmodified_against_the_shim():
    """tests/cpp/ref_callers_test.cpp #includes the reference's core/gtsam/photometric_factor.cpp and core/system/camera_tracker.cpp whole and
    unmodified (built into oracle/_ref/ by oracle/Makefile where the reference tree exists, and travels with oracle/_ref/ like libdfx_ref.so;
    the build FAILS if a reference call site stops compiling against include/dfx_shim.hpp) and checks linearize() / error() / TrackFrame()
    against the C ABI bit for bit."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_callers_test")
    assert os.path.exists(exe), "oracle/_ref/ref_callers_test not built: run __graft_entry__.build() where the reference tree exists"
    _run(exe, "ref_callers_test OK")
