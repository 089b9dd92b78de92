"""moped_amd/host/sensor_image_test run for real: hipSensorGray (SENSOR_IMAGE_HIP.hpp), the replacement for the node's
cv_bridge "mono8" line (moped3d/moped3d.cpp:249), against the program's own plain C++ loop on the same camera buffer -- 0
differing bytes, for an interleaved, a four-byte and a Bayer encoding, at the camera's size and at a small odd one, with
packed and with padded rows."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "moped_amd", "host", "sensor_image_test")


def run(args):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    t = r.stdout.split()
    assert t[:1] == ["DIFF"] and t[2] == "OF", (r.returncode, r.stdout, r.stderr[-2000:])
    return r.returncode, int(t[1]), int(t[3])


@pytest.mark.parametrize("encoding", ["bgr8", "rgba8", "bayer_grbg8"])
@pytest.mark.parametrize("size,pad", [((640, 480), 0), ((33, 17), 0), ((33, 17), 5)],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "pad%d" % v)
def test_helper_equals_the_host_loop(encoding, size, pad):
    rc, diff, total = run(["--encoding", encoding, "--size", size[0], size[1], "--pad", pad])
    assert total == size[0] * size[1]
    assert diff == 0 and rc == 0, (diff, rc)
