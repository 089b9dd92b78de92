"""object_hulls_hip.hpp compiles at the reference's language level against the mirror of its types (`make check98_hulls`)
and against the reference's real moped.hpp of both trees (`make check_ref_hulls`; reported as skipped where that tree
is absent)."""
import os
import subprocess

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moped_amd", "host")


def test_hull_helper_is_gnu98_clean_and_fits_the_reference_types():
    out = subprocess.run(["make", "-s", "-B", "-C", HOST, "check98_hulls", "check_ref_hulls"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error" not in out.stderr, out.stderr
    assert "check_ref_hulls: getObjectHulls_HIP compiles" in out.stdout or "check_ref_hulls: skipped" in out.stdout, out.stdout


def test_hull_helper_includes_no_hip_header():
    text = open(os.path.join(HOST, "object_hulls_hip.hpp")).read()
    assert "hip/hip_runtime" not in text and "hip_runtime_api" not in text
